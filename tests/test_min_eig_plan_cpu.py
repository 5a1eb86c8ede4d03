"""The two host-only pieces of the certificate's eigensolver, under ASan + UBSan (CPU only; each a stand-alone program
with its own main, compiled as tests/test_session_blocks_cpu.py compiles rank_change.cpp):
  lanczos_restart.h   the thick-restart recurrence, driven with a basis in plain arrays on matrices whose eigenvalues are
                      known (tests/cpp/lanczos_restart.cpp)
  min_eig_plan.h      the plan of computeMinimumEigenPair: the decision after the first run under both policies, the
                      eigenvalue corrections, the shift ladder's sequences (tests/cpp/min_eig_plan.cpp)"""
from test_session_blocks_cpu import _compile, _run


def test_thick_restart_recurrence_on_known_spectra(tmp_path):
    """{-2, 1 x 200, 3 x 200} plain and spectrum-shifted; 2 I (dead at step 1 by the relative test); the zero matrix;
    order 1; an order below ncv; the 1-D Laplacian of order 300 with ncv = 6 (at least three restarts).  Each: ok, the
    eigenvalue within 2 tol max(eps^(2/3), |theta|) at tol = 1e-8, |v| = 1 to 1e-12, matvecs within the Krylov budget"""
    out = _run([_compile(tmp_path, "lanczos_restart")])
    print(out)
    assert out.count("ok ") == 7, out


def test_min_eig_plan_decisions_and_shift_ladder(tmp_path):
    out = _run([_compile(tmp_path, "min_eig_plan")])
    assert out.count("ok ") == 7, out
