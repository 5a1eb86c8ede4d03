"""dcora_amd -- MI355X-native implementation of DCORA's per-agent Riemannian local solver, certification and
RBCD loop.  This package is a thin Python view (for tests and bench.py) of the C ABI in include/dcora_hip.h;
the product is libdcora_hip.so (HIP kernels for gfx950 + C++ host code).  Class and method names mirror the
reference's C++ API (QuadraticProblem / QuadraticOptimizer / ROptParameters, ref include/DCORA/*.h).
"""
import ctypes as C
import gzip
import os
import shutil
import tempfile

import numpy as np

from . import capi
from .capi import DcoraError, Dims, ROptParams, ROptResult, RbcdOptions, F, unF, check

__all__ = ["QuadraticProblem", "QuadraticOptimizer", "ROptParameters", "Dataset", "Csr", "RbcdSession", "RaRbcdSession", "DcoraError",
           "build_Q_pgo", "dual_certificate", "is_psd", "min_eig", "fast_verification", "manifold_project",
           "device_count"]


def device_count():
    return capi.lib().dcora_device_count()


class Csr:
    """row-major CSR, int32 indices (ref include/DCORA/DCORA_types.h:36)"""

    def __init__(self, n, rp, ci, v):
        self.n = int(n)
        self.rp = np.ascontiguousarray(rp, dtype=np.int32)
        self.ci = np.ascontiguousarray(ci, dtype=np.int32)
        self.v = np.ascontiguousarray(v, dtype=np.float64)

    @property
    def nnz(self):
        return int(self.rp[-1])

    def to_scipy(self):
        import scipy.sparse as sp
        return sp.csr_matrix((self.v, self.ci, self.rp), shape=(self.n, self.n))

    @staticmethod
    def from_scipy(A):
        A = A.tocsr()
        A.sort_indices()
        return Csr(A.shape[0], A.indptr, A.indices, A.data)


class Dataset:
    """measurement list: ids m x 4 (r1,p1,r2,p2), vals m x (d*d+d+3) (R col-major, t, kappa, tau, weight)"""

    def __init__(self, d, n, ids, vals):
        self.d, self.n = int(d), int(n)
        self.ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1, 4)
        self.vals = np.ascontiguousarray(vals, dtype=np.float64).reshape(self.ids.shape[0], self.d * self.d + self.d + 3)

    @property
    def m(self):
        return self.ids.shape[0]

    @staticmethod
    def load_g2o(path):
        """read_g2o_file (ref src/DCORA_utils.cpp:179-375); accepts .g2o and .g2o.gz"""
        L = capi.lib()
        tmp = None
        if str(path).endswith(".gz"):
            fd, tmp = tempfile.mkstemp(suffix=".g2o")
            with os.fdopen(fd, "wb") as out, gzip.open(path, "rb") as src:
                shutil.copyfileobj(src, out)
            path = tmp
        try:
            h = C.c_void_p()
            check(L.dcora_dataset_load_g2o(str(path).encode(), C.byref(h)))
        finally:
            if tmp:
                os.unlink(tmp)
        d, n, m = C.c_int(), C.c_int(), C.c_int()
        check(L.dcora_dataset_info(h, C.byref(d), C.byref(n), C.byref(m)))
        ids = np.zeros((m.value, 4), np.int32)
        vals = np.zeros((m.value, d.value * d.value + d.value + 3), np.float64)
        check(L.dcora_dataset_copy(h, ids, vals))
        L.dcora_dataset_destroy(h)
        return Dataset(d.value, n.value, ids, vals)

    def handle(self):
        h = C.c_void_p()
        check(capi.lib().dcora_dataset_create(self.d, self.n, self.m, self.ids, self.vals, C.byref(h)))
        return h


def chordal_initialization(ds, device=None):
    """chordalInitialization (ref src/DCORA_solver.cpp:218-268); returns T, d x (d+1) n.  device: solve the two SPD
    systems on that GPU (large graphs) instead of on the host"""
    h = ds.handle()
    out = np.zeros(ds.d * (ds.d + 1) * ds.n)
    try:
        if device is None:
            check(capi.lib().dcora_dataset_chordal_init(h, out))
        else:
            check(capi.lib().dcora_dataset_chordal_init_device(h, int(device), out))
    finally:
        capi.lib().dcora_dataset_destroy(h)
    return unF(out, ds.d, (ds.d + 1) * ds.n)


def build_Q_pgo(ds, n=None, agent=0, ids=None, vals=None):
    """Graph::constructQuadraticCostTermPGO (ref src/Graph.cpp:579-683)"""
    ids = ds.ids if ids is None else np.ascontiguousarray(ids, np.int32)
    vals = ds.vals if vals is None else np.ascontiguousarray(vals, np.float64)
    h = C.c_void_p()
    check(capi.lib().dcora_graph_build_Q_pgo(ds.d, ds.n if n is None else n, agent, ids.shape[0], ids, vals,
                                             C.byref(h)))
    return Csr(*capi.take_csr(h))


class RADataset:
    """centralised range-aided SLAM problem read from a .pyfg file (ref src/DCORA_utils.cpp:437-1167, 1169-1365;
    Q: ref src/Graph.cpp:824-1188).  X is r x k in the RA ordering [Y1..Yn | s1..sl | p1..pn | L1..Lb]."""

    def handle(self):
        """a fresh dcora_radataset_t of the file, with the pose-pose weights of set_pose_pose_weights if any (the caller
        destroys it)"""
        L = capi.lib()
        path, tmp = self.path, None
        if str(path).endswith(".gz"):
            fd, tmp = tempfile.mkstemp(suffix=".pyfg")
            with os.fdopen(fd, "wb") as out, gzip.open(path, "rb") as src:
                shutil.copyfileobj(src, out)
            path = tmp
        try:
            h = C.c_void_p()
            check(L.dcora_radataset_load_pyfg(str(path).encode(), C.byref(h)))
        finally:
            if tmp:
                os.unlink(tmp)
        w = getattr(self, "pose_pose_weights", None)
        if w is not None:
            st = L.dcora_radataset_set_pose_pose_weights(h, w)
            if st:
                L.dcora_radataset_destroy(h)
                check(st)
        return h

    def __init__(self, path, init_seed=20250310):
        L = capi.lib()
        self.path = path
        h = self.handle()
        info = np.zeros(7, np.int32)
        check(L.dcora_radataset_info(h, info))
        self.d, self.n, self.l, self.b = (int(x) for x in info[:4])
        self.num_pose_pose, self.num_pose_landmark, self.num_range = (int(x) for x in info[4:])
        self.k = (self.d + 1) * self.n + self.l + self.b
        gt = np.zeros(self.d * self.k)
        check(L.dcora_radataset_ground_truth(h, gt))
        self.gt = unF(gt, self.d, self.k)
        q = C.c_void_p()
        check(L.dcora_radataset_build_Q(h, C.byref(q)))
        self.Q = Csr(*capi.take_csr(q))
        # start point of the centralised CORA driver (ref examples/SingleRobotExample_RASLAM.cpp:92-150), d x k
        x0 = np.zeros(self.d * self.k)
        check(L.dcora_radataset_odometry_init(h, init_seed, x0))
        self.X_odom = unF(x0, self.d, self.k)
        # ownership of the merged variables and every robot's columns in its own RA ordering
        # (ref src/DCORA_utils.cpp:1370-1512, src/Graph.cpp:584-616, 1092-1097)
        self.pose_robot = np.zeros(max(self.n, 1), np.int32)
        self.sphere_robot = np.zeros(max(self.l, 1), np.int32)
        self.landmark_robot = np.zeros(max(self.b, 1), np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        check(L.dcora_radataset_ownership(h, vp(self.pose_robot), vp(self.sphere_robot), vp(self.landmark_robot)))
        self.pose_robot, self.sphere_robot = self.pose_robot[:self.n], self.sphere_robot[:self.l]
        self.landmark_robot = self.landmark_robot[:self.b]
        self.robots = sorted(set(self.pose_robot.tolist()))
        self.agent_columns = {}
        for rb in sorted(set(self.robots) | set(self.landmark_robot.tolist())):
            dims3, own, ka = np.zeros(3, np.int32), np.zeros(self.k, np.int32), C.c_int()
            check(L.dcora_radataset_agent_columns(h, rb, dims3, vp(own), C.byref(ka)))
            self.agent_columns[rb] = (tuple(int(x) for x in dims3), own[:ka.value].copy())
        L.dcora_radataset_destroy(h)

    def loop_closures(self):
        """one flag per pose-pose measurement (the order of dcora_radataset_copy): True for a loop closure, False for
        odometry -- both poses of one robot and consecutive in its own numbering (as driver.loop_closure_mask)"""
        h = self.handle()
        try:
            mask = np.zeros(max(self.num_pose_pose, 1), np.int32)
            check(capi.lib().dcora_radataset_loop_closures(h, mask))
        finally:
            capi.lib().dcora_radataset_destroy(h)
        return mask[:self.num_pose_pose].astype(bool)

    def rank_edges(self, rank, world_size):
        """(touches, owns), one flag per pose-pose measurement each, of rank `rank` of a robust job of world_size ranks
        (ra_robust_ranked_session; host only): either pose belongs to an agent the rank hosts; it hosts the owner of p1"""
        h = self.handle()
        try:
            t = np.zeros(max(self.num_pose_pose, 1), np.int32)
            o = np.zeros(max(self.num_pose_pose, 1), np.int32)
            check(capi.lib().dcora_radataset_rank_edges(h, int(rank), int(world_size), t, o))
        finally:
            capi.lib().dcora_radataset_destroy(h)
        return t[:self.num_pose_pose].astype(bool), o[:self.num_pose_pose].astype(bool)

    def loop_closure_stats(self, robot):
        """Graph::statistics (ref src/Graph.cpp:475-521) of one robot on the current weights, host only: accepted
        (weight 1), rejected (weight 0) and all loop closures -- pose-pose loop closures, pose-landmark measurements and
        ranges -- with an end at the robot: what a session of this dataset starts with (RaRbcdSession.loop_closure_stats)"""
        h = self.handle()
        try:
            c = np.zeros(3, np.int32)
            check(capi.lib().dcora_radataset_loop_closure_stats(h, int(robot), c))
        finally:
            capi.lib().dcora_radataset_destroy(h)
        return {"accepted": int(c[0]), "rejected": int(c[1]), "total": int(c[2])}

    def set_pose_pose_weights(self, w):
        """the weights of the pose-pose measurements (each finite and >= 0): kept by this object, applied to every
        handle() -- so every session created afterwards sees them -- and to Q, which is rebuilt.  None: the file's (1)."""
        if w is not None:
            w = np.ascontiguousarray(w, np.float64).copy()
            if w.shape != (self.num_pose_pose,):
                raise ValueError("set_pose_pose_weights needs one weight per pose-pose measurement")
        old = getattr(self, "pose_pose_weights", None)
        self.pose_pose_weights = w
        try:
            h = self.handle()
        except Exception:
            self.pose_pose_weights = old
            raise
        try:
            q = C.c_void_p()
            check(capi.lib().dcora_radataset_build_Q(h, C.byref(q)))
            self.Q = Csr(*capi.take_csr(q))
        finally:
            capi.lib().dcora_radataset_destroy(h)

    def pose_pose(self):
        """(ids m_pp x 2, vals m_pp x (d*d + d + 3): R column-major, t, kappa, tau, weight) as dcora_radataset_copy
        writes the pose-pose measurements"""
        h = self.handle()
        try:
            m, wd = self.num_pose_pose, self.d * self.d + self.d + 3
            ids, vals = np.zeros((max(m, 1), 2), np.int32), np.zeros((max(m, 1), wd))
            vp = lambda a: a.ctypes.data_as(C.c_void_p)
            check(capi.lib().dcora_radataset_copy(h, vp(ids), vp(vals), None, None, None, None))
        finally:
            capi.lib().dcora_radataset_destroy(h)
        return ids[:m], vals[:m]

    def measurements(self):
        """all three measurement lists as dcora_radataset_copy writes them, a dict of (ids, vals) pairs: pose_pose (as
        pose_pose()), pose_landmark (ids m x 2: pose, landmark; vals m x (d + 2): t, tau, weight) and ranges (ids m x 5:
        type1, i, type2, j, unit sphere, type 0 a pose and 1 a landmark; vals m x 3: range, precision, weight)"""
        h = self.handle()
        try:
            d = self.d
            shapes = [(self.num_pose_pose, 2, d * d + d + 3), (self.num_pose_landmark, 2, d + 2), (self.num_range, 5, 3)]
            arrs = [(np.zeros((max(m, 1), wi), np.int32), np.zeros((max(m, 1), wv))) for m, wi, wv in shapes]
            vp = lambda a: a.ctypes.data_as(C.c_void_p)
            check(capi.lib().dcora_radataset_copy(h, *[vp(a) for pair in arrs for a in pair]))
        finally:
            capi.lib().dcora_radataset_destroy(h)
        return {name: (ids[:m], vals[:m])
                for name, (m, _, _), (ids, vals) in zip(("pose_pose", "pose_landmark", "ranges"), shapes, arrs)}

    def colours(self):
        """(colours, number of colours) of the agents -- the robots owning poses, in id order -- as a session of this
        file will colour them (dcora_radataset_agent_colours: host only, no device needed)"""
        h = self.handle()
        try:
            col, nc = np.zeros(len(self.robots), np.int32), C.c_int()
            check(capi.lib().dcora_radataset_agent_colours(h, col, C.byref(nc)))
        finally:
            capi.lib().dcora_radataset_destroy(h)
        return col, nc.value

    def agent_blocks(self, robot, Q=None):
        """(n_a, l_a, b_a), own columns, Q_aa (Csr, agent ordering), coupling C (scipy k_a x k, global columns):
        the agent's local problem is 1/2 <Q_aa, X_a^T X_a> + <X_a, X_global C^T>"""
        import scipy.sparse as sp
        Q = self.Q if Q is None else Q
        dims3, own = self.agent_columns[robot]
        own = np.ascontiguousarray(own, np.int32)
        qa, cc = C.c_void_p(), C.c_void_p()
        check(capi.lib().dcora_graph_extract_agent_blocks(Q.n, Q.rp, Q.ci, Q.v, own.size, own, C.byref(qa),
                                                          C.byref(cc)))
        Qaa = Csr(*capi.take_csr(qa))
        ka, rp, ci, v = capi.take_csr(cc)
        return dims3, own, Qaa, sp.csr_matrix((v, ci, rp), shape=(ka, Q.n))


def precond_regularization(Q, device=0):
    """Graph::computePreconditionerRegularization (ref src/Graph.cpp:1921-1960)"""
    reg = C.c_double()
    check(capi.lib().dcora_graph_precond_regularization(Q.n, Q.rp, Q.ci, Q.v, device, C.byref(reg)))
    return reg.value


class ROptParameters:
    """ref include/DCORA/DCORA_types.h:152-168"""
    RTR, RGD = 0, 1

    def __init__(self, **kw):
        self.c = ROptParams()
        capi.lib().dcora_ropt_params_default(C.byref(self.c))
        for k, v in kw.items():
            setattr(self.c, k, v)

    def __getattr__(self, k):
        return getattr(self.__dict__["c"], k)


class QuadraticProblem:
    """ref include/DCORA/QuadraticProblem.h: f, RieGrad, RieGradNorm, Retract, PreCondition, escapeSaddle"""

    def __init__(self, r, d, n, Q, G=None, reg=0.1, l=0, b=0, device=0, layout=0):
        """layout: 0 = SE ordering when l = b = 0, RA otherwise; capi.LAYOUT_RA keeps the RA ordering of a range-aided
        graph that holds neither ranges nor landmarks (ref src/Graph.cpp:68-75)"""
        self.r, self.d, self.n, self.l, self.b = r, d, n, l, b
        self.k = (d + 1) * n + l + b
        if Q.n != self.k:
            raise ValueError("Q is %d x %d, expected %d" % (Q.n, Q.n, self.k))
        dims = Dims(r, d, n, l, b, layout)
        g = None
        if G is not None:
            self._G = F(G)
            g = self._G.ctypes.data_as(C.c_void_p)
        self.h = C.c_void_p()
        check(capi.lib().dcora_problem_create(C.byref(dims), Q.rp, Q.ci, Q.v, g, float(reg), device, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            capi.lib().dcora_problem_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def relaxation_rank(self):
        return self.r

    def problem_dimension(self):
        return self.k

    def _out(self):
        return np.zeros(self.r * self.k)

    def set_linear_term(self, G):
        g = None
        if G is not None:
            self._G = F(G)
            g = self._G.ctypes.data_as(C.c_void_p)
        check(capi.lib().dcora_problem_set_linear_term(self.h, g))

    def f(self, Y):
        out = C.c_double()
        check(capi.lib().dcora_problem_cost(self.h, F(Y), C.byref(out)))
        return out.value

    def EucGrad(self, Y):
        out = self._out()
        check(capi.lib().dcora_problem_eucgrad(self.h, F(Y), out))
        return unF(out, self.r, self.k)

    def RieGrad(self, Y):
        out = self._out()
        nrm = C.c_double()
        check(capi.lib().dcora_problem_riegrad(self.h, F(Y), out.ctypes.data_as(C.c_void_p), C.byref(nrm)))
        return unF(out, self.r, self.k)

    def RieGradNorm(self, Y):
        nrm = C.c_double()
        check(capi.lib().dcora_problem_riegrad(self.h, F(Y), None, C.byref(nrm)))
        return nrm.value

    def HessVec(self, Y, V):
        out = self._out()
        check(capi.lib().dcora_problem_hessvec(self.h, F(Y), F(V), out))
        return unF(out, self.r, self.k)

    def HessVecSolverForm(self, Y, V):
        """test hook: H[V] as the generic solver loop forms it (one launch) and {<V, H V> from that kernel's partial
        sums, the same from the two-launch form}"""
        out = self._out()
        dots = np.zeros(2)
        check(capi.lib().dcora_debug_hessvec_solver_form(self.h, F(Y), F(V), out, dots))
        return unF(out, self.r, self.k), dots

    def PreCondition(self, Y, V):
        out = self._out()
        check(capi.lib().dcora_problem_precondition(self.h, F(Y), F(V), out))
        return unF(out, self.r, self.k)

    def Retract(self, Y, V):
        out = self._out()
        check(capi.lib().dcora_problem_retract(self.h, F(Y), F(V), out))
        return unF(out, self.r, self.k)

    def projectToTangentSpace(self, Y, V):
        out = self._out()
        check(capi.lib().dcora_problem_tangent_project(self.h, F(Y), F(V), out))
        return unF(out, self.r, self.k)

    def escapeSaddle(self, Xopt, theta, v, gradient_tolerance=1e-6, preconditioned_gradient_tolerance=1e-6,
                     isSecondOrder=False):
        out = self._out()
        ok = C.c_int()
        check(capi.lib().dcora_problem_escape_saddle(self.h, F(Xopt), float(theta),
                                                     np.ascontiguousarray(v, np.float64), gradient_tolerance,
                                                     preconditioned_gradient_tolerance, int(isSecondOrder), out,
                                                     C.byref(ok)))
        return (unF(out, self.r, self.k) if ok.value else None)

    def time_qapply(self, reps=100):
        ms, by = C.c_double(), C.c_double()
        check(capi.lib().dcora_problem_time_qapply(self.h, reps, C.byref(ms), C.byref(by)))
        return ms.value, by.value


def _time_precond(self, reps=100):
    ms, by = C.c_double(), C.c_double()
    check(capi.lib().dcora_problem_time_precond(self.h, reps, C.byref(ms), C.byref(by)))
    return ms.value, by.value


QuadraticProblem.time_precond = _time_precond


def _precond_info(self):
    """how (Q + reg I)^-1 is held on the device: dense inverse or partitioned sparse inverse"""
    info = np.zeros(5)
    check(capi.lib().dcora_problem_precond_info(self.h, info))
    return {"kind": {0: "none", 1: "dense", 2: "sparse"}[int(info[0])], "launches": int(info[1]),
            "nnzL": int(info[2]), "setup_ms": float(info[3]), "stored_doubles_per_apply": float(info[4])}


QuadraticProblem.precond_info = _precond_info


def _qapply_info(self):
    info = np.zeros(4)
    check(capi.lib().dcora_problem_qapply_info(self.h, info))
    return {"kernel": "k_spmm_bsrq" if info[0] else "k_spmm", "nnz": int(info[1]), "blocks": int(info[2]),
            "stored_matrix_bytes": float(info[3])}


QuadraticProblem.qapply_info = _qapply_info


def _solver_info(self):
    """how the tCG iteration runs: 'three launches', 'two launches' or 'one launch per run' (k_tcg_run)"""
    info = np.zeros(2)
    check(capi.lib().dcora_problem_solver_info(self.h, info))
    return {"tcg": {0: "three launches", 1: "two launches", 2: "one launch per run"}[int(info[0])]}


QuadraticProblem.solver_info = _solver_info


def _gather_info(self):
    """how the one-launch tCG run gathers its neighbours' columns (DCORA_GATHER): the column-slot map of its 2-pose
    workgroups and whether the run uses it ('columns') or every row gathers its own entries ('entries')"""
    info = np.zeros(5)
    check(capi.lib().dcora_problem_gather_info(self.h, info))
    return {"map": bool(info[0]), "workgroups": int(info[1]), "overflow": int(info[2]), "max_poses": int(info[3]),
            "gather": "columns" if info[4] else "entries"}


QuadraticProblem.gather_info = _gather_info


def _debug_rerank(self, r_new):
    """test hook: the problem at rank r_new in place, as a session's lift or projection leaves it (G = 0 afterwards)"""
    check(capi.lib().dcora_debug_problem_rerank(self.h, int(r_new)))
    self.r = int(r_new)
    self._G = None


QuadraticProblem.debug_rerank = _debug_rerank


def column_slots(rp, ci, n, dh, pb, cap_cols):
    """the column-slot map of a workgroup tiling (host only): dict of lp, list, count, overflow, slot"""
    rp = np.ascontiguousarray(rp, dtype=np.int32)
    ci = np.ascontiguousarray(ci, dtype=np.int32)
    nwg = (n + pb - 1) // pb
    cap = nwg * max(1, min(n, cap_cols // dh))
    out = {"lp": np.zeros(nwg + 1, np.int32), "list": np.zeros(cap, np.int32), "count": np.zeros(nwg, np.int32),
           "overflow": np.zeros(nwg, np.int32), "slot": np.zeros(len(ci), np.int32)}
    check(capi.lib().dcora_debug_column_slots(rp, ci, n, dh, pb, cap_cols, cap, out["lp"], out["list"], out["count"],
                                              out["overflow"], out["slot"]))
    out["list"] = out["list"][:out["lp"][-1]]
    return out


def time_qapply_rotating(problems, reps=60):
    """average launch time of the Q-apply over several problems in turn on one stream (HBM-cold when their bytes
    exceed the Infinity Cache)"""
    arr = (C.c_void_p * len(problems))(*[getattr(p.h, 'value', p.h) for p in problems])
    ms = C.c_double()
    check(capi.lib().dcora_problem_time_qapply_rotating(arr, len(problems), reps, C.byref(ms)))
    return ms.value


def precond_cache_info():
    v = np.zeros(4)
    check(capi.lib().dcora_precond_cache_info(v))
    return {"hits": int(v[0]), "misses": int(v[1]), "entries": int(v[2]), "device_bytes": float(v[3])}


def precond_cache_clear():
    check(capi.lib().dcora_precond_cache_clear())


class QuadraticOptimizer:
    """ref include/DCORA/QuadraticOptimizer.h: optimize(Y), getOptResult()"""

    def __init__(self, problem, params=None):
        self.problem = problem
        self.params = params or ROptParameters()
        self.result = ROptResult()

    def optimize(self, Y):
        out = np.zeros(self.problem.r * self.problem.k)
        check(capi.lib().dcora_optimizer_optimize(self.problem.h, C.byref(self.params.c), F(Y), out,
                                                  C.byref(self.result)))
        return unF(out, self.problem.r, self.problem.k)

    def getOptResult(self):
        return self.result.as_dict()


def manifold_project(r, d, n, M, l=0, b=0, device=0, layout=0):
    """projectToSEMatrix / projectToRAMatrix (ref src/DCORA_utils.cpp:2201-2220)"""
    dims = Dims(r, d, n, l, b, layout)
    k = (d + 1) * n + l + b
    out = np.zeros(r * k)
    check(capi.lib().dcora_manifold_project(C.byref(dims), F(M), out, device))
    return unF(out, r, k)


def dual_certificate(r, d, n, X, Q, l=0, b=0, device=0, layout=0):
    """constructDualCertificateMatrixPGO / RASLAM (ref src/DCORA_utils.cpp:1898-1982)"""
    dims = Dims(r, d, n, l, b, layout)
    h = C.c_void_p()
    check(capi.lib().dcora_cert_dual_matrix(C.byref(dims), F(X), Q.rp, Q.ci, Q.v, device, C.byref(h)))
    return Csr(*capi.take_csr(h))


def is_psd(S, block=1):
    out = C.c_int()
    check(capi.lib().dcora_cert_is_psd(S.n, S.rp, S.ci, S.v, block, C.byref(out)))
    return bool(out.value)


def cert_prepare(Q, d, n, l=0, b=0, block=1, device=0, layout=0):
    """analysis of the PSD test of the dual certificate S = Q - Lambda ahead of time (dcora_cert_prepare): its pattern
    is known from Q's; meant for another host thread while the agents iterate"""
    k = (d + 1) * n + l + b
    if Q.n != k:  # the library cannot see the length of rp: it reads k + 1 entries
        raise ValueError("Q is %d x %d, expected %d" % (Q.n, Q.n, k))
    dims = Dims(1, d, n, l, b, layout)
    check(capi.lib().dcora_cert_prepare(C.byref(dims), Q.rp, Q.ci, block, device))


def is_psd_device(S, block=1, device=0, info=False):
    """the PSD test with the numeric factorisation on the device (dcora_cert_is_psd_device)"""
    out = C.c_int()
    i6 = np.zeros(8)
    check(capi.lib().dcora_cert_is_psd_device(S.n, S.rp, S.ci, S.v, block, device, C.byref(out), i6))
    if info:
        return bool(out.value), {"symbolic_ms": i6[0], "numeric_ms": i6[1], "arena_bytes": i6[2], "flops": i6[3],
                                 "levels": int(i6[4]), "launches": int(i6[5]), "logdet": i6[6],
                                 "lookup_ms": i6[7]}
    return bool(out.value)


def chol_host_selftest(S, block=1):
    """(is_pd, max |P A P^T - L L^T|, info) of the multifrontal schedule executed on the host (validation only)"""
    out, res = C.c_int(), C.c_double()
    i4 = np.zeros(4)
    check(capi.lib().dcora_chol_host_selftest(S.n, S.rp, S.ci, S.v, block, C.byref(out), C.byref(res), i4))
    return bool(out.value), res.value, {"pieces": int(i4[0]), "levels": int(i4[1]), "arena": int(i4[2]),
                                        "flops": i4[3]}


def stream_triad_gbps(n=1 << 28, reps=20, device=0):
    """measured HBM stream figure of the box: a = b + s c over three arrays of n doubles (6.4 GB by default, far
    beyond the 256 MiB Infinity Cache)"""
    L = capi.lib()
    L.dcora_debug_stream_triad.restype = C.c_int
    L.dcora_debug_stream_triad.argtypes = [C.c_int, C.c_size_t, C.c_int, C.POINTER(C.c_double)]
    out = C.c_double()
    check(L.dcora_debug_stream_triad(device, n, reps, C.byref(out)))
    return out.value


def chol_cache_clear():
    check(capi.lib().dcora_chol_cache_clear())


def min_eig(S, max_iterations=1000, tol=1e-3, ncv=20, seed=12345, device=0):
    lam, mv = C.c_double(), C.c_long()
    v = np.zeros(S.n)
    st = capi.lib().dcora_cert_min_eig(S.n, S.rp, S.ci, S.v, max_iterations, tol, ncv, seed, device, C.byref(lam), v,
                                       C.byref(mv))
    if st not in (0, 5):
        check(st)
    return st == 0, lam.value, v, mv.value


def fast_verification(S, eta, block=1, device=0):
    psd, th, lm = C.c_int(), C.c_double(), C.c_double()
    v = np.zeros(S.n)
    st = capi.lib().dcora_cert_fast_verification(S.n, S.rp, S.ci, S.v, float(eta), block, device, C.byref(psd),
                                                 C.byref(th), v, C.byref(lm))
    if st not in (0, 5):
        check(st)
    return bool(psd.value), th.value, v, lm.value


def lambda_min_certified(S, eta, block=1, max_iterations=120):
    """certified lower bound of lambda_min(S) after the certificate S + eta I >= 0 was accepted: the Lanczos estimate on
    (S + eta I)^-1 minus its Ritz residual, verified by a Cholesky factorisation of S - bound I (-eta if that fails)"""
    lam, it = C.c_double(), C.c_int()
    check(capi.lib().dcora_cert_lambda_min_certified(S.n, S.rp, S.ci, S.v, eta, block, max_iterations, C.byref(lam),
                                                     C.byref(it)))
    return lam.value, it.value


def suboptimality_gap(r, d, n, X, psd, eta, lambda_min=None, l=0, b=0, lambda_bound=None):
    """bound on f(X) - f* that goes with a certificate (dcora_cert_suboptimality_gap, an addition of this library): after
    fast_verification(S, eta) returned psd (S + eta I >= 0) or, otherwise, its lambda_min output (of S + eta I);
    lambda_bound overrides (e.g. min(lambda_min_certified(S, eta), 0))"""
    lam = lambda_bound if lambda_bound is not None else (-eta if psd else float(lambda_min) - eta)
    gap, neff = C.c_double(), C.c_double()
    dims = Dims(r, d, n, l, b)
    check(capi.lib().dcora_cert_suboptimality_gap(C.byref(dims), F(X), lam, C.byref(gap), C.byref(neff)))
    return gap.value, neff.value


def _session_certify(fn, h, k, eta):
    """dcora_rbcd_certify / dcora_ra_rbcd_certify -> (psd, theta, v, lambda_min, info): the first four as
    fast_verification returns them, info = the PSD test's figures (is_psd_device) and the Lanczos products"""
    psd, th, lm, mv = C.c_int(), C.c_double(), C.c_double(), C.c_longlong()
    v, i8 = np.zeros(k), np.zeros(8)
    st = fn(h, float(eta), C.byref(psd), C.byref(th), C.byref(lm), v.ctypes.data_as(C.c_void_p), C.byref(mv),
            i8.ctypes.data_as(C.c_void_p))
    if st not in (0, 5):
        check(st)
    info = {"symbolic_ms": i8[0], "numeric_ms": i8[1], "arena_bytes": i8[2], "flops": i8[3], "levels": int(i8[4]),
            "launches": int(i8[5]), "logdet": i8[6], "lookup_ms": i8[7], "matvecs": mv.value}
    return bool(psd.value), th.value, v, lm.value, info


def _session_lift(self, fn, rank_fn, theta, v, gradient_tolerance, preconditioned_gradient_tolerance,
                  is_second_order, central_reg):
    """dcora_rbcd_lift / dcora_ra_rbcd_lift -> (escaped, info); self.r follows the session's rank"""
    v = np.ascontiguousarray(v, np.float64)
    if v.shape != (self.k,):
        raise ValueError("lift needs the certificate's v: k numbers")
    p = capi.LiftParams()
    check(capi.lib().dcora_lift_params_default(C.byref(p)))
    p.gradient_tolerance = gradient_tolerance
    p.preconditioned_gradient_tolerance = preconditioned_gradient_tolerance
    p.is_second_order = int(bool(is_second_order))
    if central_reg is not None:
        p.central_reg = central_reg
    esc, i8, r = C.c_int(), np.zeros(8), C.c_int()
    check(fn(self.h, float(theta), v, C.byref(p), C.byref(esc), i8.ctypes.data_as(C.c_void_p)))
    check(rank_fn(self.h, C.byref(r)))
    self.r = r.value
    info = {"trials": int(i8[0]), "alpha": i8[1], "f_before": i8[2], "f_after": i8[3],
            "precond_built": bool(i8[4]), "precond_ms": i8[5], "redimension_ms": i8[6], "total_ms": i8[7]}
    return bool(esc.value), info


def _run_coloured(fn, h, max_sweeps, rgrad_tol):
    """the coloured run loop of a session or an exchange: sweeps of one tick per colour, each followed by an evaluation"""
    it = C.c_int()
    cost, gn = np.zeros(max(max_sweeps, 1)), np.zeros(max(max_sweeps, 1))
    check(fn(h, max_sweeps, rgrad_tol, C.byref(it), cost.ctypes.data_as(C.c_void_p), gn.ctypes.data_as(C.c_void_p)))
    n = it.value
    return dict(iters=n, cost=cost[:n], gradnorm=gn[:n])


def _rbcd_options(num_robots, r, acceleration, restart_interval, params, rank, world_size, device, stream):
    o = RbcdOptions()
    capi.lib().dcora_rbcd_options_default(C.byref(o))
    o.num_robots, o.r, o.acceleration, o.restart_interval = num_robots, r, int(acceleration), restart_interval
    if params is not None:
        o.local = params.c
    o.rank, o.world_size, o.device = rank, world_size, device
    o.stream = stream  # raw hipStream_t (int) or None
    return o


def _fixed_flags(ds, fixed_weight):
    if fixed_weight is None:
        return None
    fx = np.ascontiguousarray(fixed_weight, np.int32)
    if fx.shape != (ds.m,):
        raise ValueError("fixed_weight needs one flag per measurement")
    return fx


def _round_anchor(anchor, r, d):
    """an anchor passed to round(): r x (d+1) numbers, column-major for the library (None stays None)"""
    if anchor is None:
        return None
    a = np.asarray(anchor, dtype=np.float64)
    if a.shape != (r, d + 1):
        raise ValueError("round needs an anchor of r x (d+1) numbers")
    return F(a)


class _Session:
    """what RbcdSession and RaRbcdSession share: the calls that differ only in the prefix of their entry point
    (_prefix: dcora_rbcd_ / dcora_ra_rbcd_) and in one word of a message (_per)"""
    _prefix = None
    _per = "measurement"   # what a weight belongs to, in set_weights' message

    def _fn(self, name):
        return getattr(capi.lib(), self._prefix + name)

    def close(self):
        if getattr(self, "h", None):
            self._fn("destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_X(self, X):
        check(self._fn("set_X")(self.h, F(X)))

    def get_X(self):
        out = np.zeros(self.r * self.k)
        check(self._fn("get_X")(self.h, out))
        return unF(out, self.r, self.k)

    def certify(self, eta):
        """fastVerification of S = Q - Lambda(X) on the device, with the Q the session holds now (its current weights) and
        its current iterate (dcora_rbcd_certify / dcora_ra_rbcd_certify) -> (psd, theta, v, lambda_min, info); v in the
        session's global ordering; the session is left as it was"""
        return _session_certify(self._fn("certify"), self.h, self.k, eta)

    def round(self, anchor_pose=0, anchor=None, cost=False):
        """The last step of a solve on the device, where the iterate lies (dcora_rbcd_round / dcora_ra_rbcd_round): the
        current iterate rounded to SE(d) in the frame of the lifted pose anchor_pose (read on the device; 0 is what the
        reference's drivers share) or of `anchor` (r x (d+1), setGlobalAnchor), the anchor's translation at the origin.
        -> dict: trajectory (d x (d+1) n, SE ordering); on a range-aided session unit_spheres (d x l, rotated only) and
        landmarks (d x b); with cost=True cost_2f -- 2 f of the rounded solution on the matrix the session holds now, its
        current weights included (sphere columns normalised in the point evaluated) -- and gradnorm; info: kernel_ms,
        eval_ms, ms.  The session is left as it was."""
        d, n, l, b = self._round_dims()
        a = _round_anchor(anchor, self.r, d)
        T, i4, c2 = np.zeros(d * (d + 1) * n), np.zeros(4), C.c_double()
        tail = (None if a is None else a.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p))
        S, Lm = np.zeros(max(d * l, 1)), np.zeros(max(d * b, 1))
        if self._prefix == "dcora_ra_rbcd_":
            tail += (S.ctypes.data_as(C.c_void_p), Lm.ctypes.data_as(C.c_void_p))
        check(self._fn("round")(self.h, int(anchor_pose), *tail, C.byref(c2) if cost else None,
                                i4.ctypes.data_as(C.c_void_p)))
        out = {"trajectory": unF(T, d, (d + 1) * n),
               "info": {"kernel_ms": float(i4[1]), "eval_ms": float(i4[2]), "ms": float(i4[3])}}
        if self._prefix == "dcora_ra_rbcd_":
            out["unit_spheres"], out["landmarks"] = unF(S[:d * l], d, l), unF(Lm[:d * b], d, b)
        if cost:
            out["cost_2f"], out["gradnorm"] = c2.value, float(i4[0])
        return out

    def project(self):
        """How CORA ends a certified solve, in place (dcora_rbcd_project / dcora_ra_rbcd_project; ref
        projectSolutionRASLAM): the session goes from rank r to rank d at Proj(V_d^T X), V_d the top-d eigenvectors of
        X X^T with the reflection rule folded in, and keeps its matrices, preconditioners, weights and team; afterwards
        self.r == d.  At r == d nothing of the session changes (projected False, basis None).  -> dict: projected,
        reflected, positive_dets, sigma (r singular values of X), basis (r x d, the new iterate is Proj(basis^T X)), gram
        (r x r, X X^T as the device formed it), cost_2f and gradnorm of the adopted point on the matrix the session holds
        now, ms_kernels, ms_redimension, ms_total, gram_chunk (columns per workgroup of the Gram kernel)."""
        r, d = self.r, self._round_dims()[0]
        sg, B, G, i8, c2, rr = np.zeros(r), np.zeros(r * d), np.zeros(r * r), np.zeros(8), C.c_double(), C.c_int()
        check(self._fn("project")(self.h, *(a.ctypes.data_as(C.c_void_p) for a in (sg, B, G)), C.byref(c2),
                                  i8.ctypes.data_as(C.c_void_p)))
        check(self._fn("rank")(self.h, C.byref(rr)))
        self.r = rr.value
        projected = bool(i8[0])
        return dict(projected=projected, reflected=bool(i8[1]), positive_dets=int(i8[2]), sigma=sg,
                    basis=unF(B, r, d) if projected else None, gram=unF(G, r, r), cost_2f=c2.value,
                    gradnorm=float(i8[3]), ms_kernels=float(i8[4]), ms_redimension=float(i8[5]), ms_total=float(i8[6]),
                    gram_chunk=int(i8[7]))

    def _lift(self, theta, v, gradient_tolerance, preconditioned_gradient_tolerance, is_second_order, central_reg):
        return _session_lift(self, self._fn("lift"), self._fn("rank"), theta, v, gradient_tolerance,
                             preconditioned_gradient_tolerance, is_second_order, central_reg)

    def reserve_rank(self, r_reserve):
        """room for the ranks to come (dcora_rbcd_reserve_rank / dcora_ra_rbcd_reserve_rank): an Exchange created on
        this session afterwards can lift the job up to r_reserve; d <= r <= r_reserve <= 16, before the exchange exists"""
        check(self._fn("reserve_rank")(self.h, int(r_reserve)))

    def _eval(self, fn, *first):
        c2, gn, nxt = C.c_double(), C.c_double(), C.c_int()
        bn = np.zeros(self.R)
        check(fn(self.h, *first, C.byref(c2), C.byref(gn), bn.ctypes.data_as(C.c_void_p), C.byref(nxt)))
        return c2.value, gn.value, bn, nxt.value

    def iterate(self, selected):
        return self._eval(self._fn("iterate"), selected)

    def evaluate(self):
        return self._eval(self._fn("evaluate"))

    def run(self, max_iters=1000, rgrad_tol=0.1):
        it = C.c_int()
        cost, gn = np.zeros(max_iters), np.zeros(max_iters)
        sel = np.zeros(max_iters, np.int32)
        check(self._fn("run")(self.h, max_iters, rgrad_tol, C.byref(it), cost.ctypes.data_as(C.c_void_p),
                              gn.ctypes.data_as(C.c_void_p), sel.ctypes.data_as(C.c_void_p)))
        n = it.value
        return dict(iters=n, cost=cost[:n], gradnorm=gn[:n], selected=sel[:n])

    def iterate_set(self, agents, allow_adjacent=False):
        """the agents of the set update at the same time from one snapshot of their neighbours' states"""
        a = np.ascontiguousarray(agents, dtype=np.int32)
        check(self._fn("iterate_set")(self.h, a, a.size, int(allow_adjacent)))

    def set_acceleration(self, on):
        check(self._fn("set_acceleration")(self.h, int(bool(on))))

    def colours(self):
        col, nc = np.zeros(self.R, np.int32), C.c_int()
        check(self._fn("agent_colours")(self.h, col, C.byref(nc)))
        return col, nc.value

    def run_coloured(self, max_sweeps=1000, rgrad_tol=0.1):
        """sweeps of iterate_set per colour of colours(), each followed by evaluate(), until |rgrad| < rgrad_tol
        (dcora_rbcd_run_coloured / dcora_ra_rbcd_run_coloured; acceleration off); iters counts sweeps"""
        return _run_coloured(self._fn("run_coloured"), self.h, max_sweeps, rgrad_tol)

    def last_result(self):
        r = ROptResult()
        check(self._fn("last_result")(self.h, C.byref(r)))
        return r.as_dict()

    # ---- robust sessions (created with robust=...); weights in the job's order (range-aided: pose-pose) ----
    def update_weights(self, reset_to_initial=False):
        """Agent::updateMeasurementWeights of every agent on the current iterate; returns the loop closures'
        {accepted, rejected, undecided} counts"""
        c = np.zeros(3, np.int32)
        check(self._fn("update_weights")(self.h, int(bool(reset_to_initial)), c.ctypes.data_as(C.c_void_p)))
        return {"accepted": int(c[0]), "rejected": int(c[1]), "undecided": int(c[2])}

    def set_weights(self, w):
        w = np.ascontiguousarray(w, np.float64)
        if w.shape != (self.m,):
            raise ValueError("set_weights needs one weight per " + self._per)
        check(self._fn("set_weights")(self.h, w))

    def get_weights(self):
        w = np.zeros(max(self.m, 1))  # (never an empty buffer: its pointer would be NULL)
        check(self._fn("get_weights")(self.h, w))
        return w[:self.m]

    def robust_info(self):
        mu, n = C.c_double(), C.c_int()
        check(self._fn("robust_info")(self.h, C.byref(mu), C.byref(n)))
        return {"mu": mu.value, "updates": n.value}


class RbcdSession(_Session):
    """Agents + synchronous RBCD++ driver on the device (ref examples/MultiRobotExample.cpp:121-307)"""
    _prefix = "dcora_rbcd_"

    def __init__(self, ds, num_robots=5, r=5, acceleration=True, restart_interval=30, params=None, rank=0,
                 world_size=1, device=0, stream=None, robust=None, fixed_weight=None):
        """robust: a robust.RobustCostParameters -> a session whose measurement weights update in place
        (update_weights / set_weights / get_weights / robust_info); it starts with weight 1 on every loop closure whose
        fixed_weight flag (m booleans, default none) is off (Agent::initializeRobustOptimization)"""
        self.ds, self.R, self.r = ds, num_robots, r
        self.k = (ds.d + 1) * ds.n
        o = _rbcd_options(num_robots, r, acceleration, restart_interval, params, rank, world_size, device, stream)
        dsh = ds.handle()
        self.h = C.c_void_p()
        try:
            if robust is None:
                check(capi.lib().dcora_rbcd_create(dsh, C.byref(o), C.byref(self.h)))
            else:
                fx = _fixed_flags(ds, fixed_weight)
                check(capi.lib().dcora_rbcd_create_robust(dsh, C.byref(o), C.byref(robust.c),
                                                          None if fx is None else fx.ctypes.data_as(C.c_void_p),
                                                          C.byref(self.h)))
        finally:
            capi.lib().dcora_dataset_destroy(dsh)
        self.m = ds.m

    def _round_dims(self):
        return self.ds.d, self.ds.n, 0, 0

    def lift(self, theta, v, gradient_tolerance=1e-6, preconditioned_gradient_tolerance=1e-6, is_second_order=False,
             central_reg=None):
        """The staircase's step in place (dcora_rbcd_lift): escapeSaddle along the refused certificate's (theta, v) into
        rank r + 1 inside this session, which keeps its matrices, preconditioners, weights, GNC state and team
        -> (escaped, info).  escaped False: nothing has changed.  self.r is the session's rank afterwards."""
        return self._lift(theta, v, gradient_tolerance, preconditioned_gradient_tolerance, is_second_order, central_reg)

    # ---- multi-process pieces ----
    def X_device_ptr(self):
        p = C.c_void_p()
        check(capi.lib().dcora_rbcd_X_device_ptr(self.h, C.byref(p)))
        return p.value

    def public_count(self, agent):
        c = C.c_int()
        check(capi.lib().dcora_rbcd_public_count(self.h, agent, C.byref(c)))
        return c.value

    def public_indices(self, agent):
        idx = np.zeros(max(self.public_count(agent), 1), np.int32)
        check(capi.lib().dcora_rbcd_public_indices(self.h, agent, idx))
        return idx[:self.public_count(agent)]

    def pack_public_dev(self, agent, ptr):
        check(capi.lib().dcora_rbcd_pack_public_dev(self.h, agent, C.c_void_p(ptr)))

    def unpack_public_dev(self, agent, ptr):
        check(capi.lib().dcora_rbcd_unpack_public_dev(self.h, agent, C.c_void_p(ptr)))

    def phase_nonselected(self, selected):
        check(capi.lib().dcora_rbcd_phase_nonselected(self.h, selected))

    def phase_selected(self, selected):
        check(capi.lib().dcora_rbcd_phase_selected(self.h, selected))

    def debug_launches(self):
        """kernel launches of the RBCD chain this session's iterate() calls have enqueued (debug counter)"""
        out = C.c_longlong(0)
        check(capi.lib().dcora_debug_rbcd_launches(self.h, C.byref(out)))
        return int(out.value)

    def phase_evaluate_dev(self, ptr):
        check(capi.lib().dcora_rbcd_phase_evaluate_dev(self.h, C.c_void_p(ptr)))

    def synchronize(self):
        check(capi.lib().dcora_rbcd_synchronize(self.h))

    def profile_tcg_runs(self, enable=True):
        """HIP events around every one-launch tCG run (k_tcg_run) of the agents while enabled (a measurement hook)"""
        check(capi.lib().dcora_rbcd_profile_tcg_runs(self.h, int(enable)))

    def profile_tcg_read(self):
        out = np.zeros(2)
        check(capi.lib().dcora_rbcd_profile_tcg_read(self.h, out))
        return {"launches": int(out[0]), "total_us": float(out[1])}


class Exchange:
    """neighbour exchange of public poses between the ranks of one node (dcora_exchange_*): the session must have been
    created with rank / world_size; every rank creates the exchange under the same job name"""
    IPC, STAGED = 1, 2
    _prefix = "dcora_exchange_"

    def __init__(self, session, job_name, _handle=None):
        self.s = session
        self.h = C.c_void_p()
        if _handle is not None:  # (made together with its session: robust_ranked_session / ra_robust_ranked_session)
            self.h = _handle
            return
        create = capi.lib().dcora_exchange_create_ra if isinstance(session, RaRbcdSession) else capi.lib().dcora_exchange_create
        check(create(session.h, job_name.encode(), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            capi.lib().dcora_exchange_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        v = np.zeros(10)
        check(capi.lib().dcora_exchange_info(self.h, v))
        return dict(transport={1: "ipc peer stores", 2: "shared host segment"}.get(int(v[0]), "?"), mode=int(v[0]),
                    halo_finegrained=bool(v[8]), wait="device (the scatter kernel polls the flag)" if v[9] else "host spin",
                    peers=int(v[1]), posts=int(v[2]), waits=int(v[3]), bytes_posted=float(v[4]), post_s=float(v[5]),
                    wait_s=float(v[6]), eval_wait_s=float(v[7]))

    def link_report(self):
        """what the start-up link check of dcora_exchange_create did: rounds run, whether the device-side wait / the IPC
        transport were given up, microseconds of the last round"""
        v = np.zeros(4)
        check(capi.lib().dcora_exchange_link_report(self.h, v))
        return dict(rounds=int(v[0]), gave_up_device_wait=bool(v[1]), gave_up_ipc=bool(v[2]), last_round_us=float(v[3]))

    def all_ready(self, ready):
        """AND over the ranks of `ready` (Agent::shouldTerminate's team condition, ref src/Agent.cpp:1137-1153)"""
        out = C.c_int()
        check(capi.lib().dcora_exchange_all_ready(self.h, int(bool(ready)), C.byref(out)))
        return bool(out.value)

    def certify(self, Q, eta, k):
        """fastVerification of the current iterate across the ranks (dcora_exchange_certify); Q: the global Csr on rank 0,
        None elsewhere; k = (d + 1) n.  -> (certified, theta, lambda_min of S + eta I, v, matvecs, distributed)"""
        cert, dist = C.c_int(), C.c_int()
        th, lm, mv = C.c_double(), C.c_double(), C.c_longlong()
        v = np.zeros(k)
        if Q is None:
            check(capi.lib().dcora_exchange_certify(self.h, k, None, None, None, eta, C.byref(cert), C.byref(th),
                                                    C.byref(lm), v, C.byref(mv), C.byref(dist)))
        else:
            check(capi.lib().dcora_exchange_certify(self.h, k, Q.rp.ctypes.data, Q.ci.ctypes.data, Q.v.ctypes.data, eta,
                                                    C.byref(cert), C.byref(th), C.byref(lm), v, C.byref(mv),
                                                    C.byref(dist)))
        return bool(cert.value), th.value, lm.value, v, mv.value, bool(dist.value)

    def certify_live(self, eta):
        """The same certificate of the matrices the ranks hold on the device now, with the job's current weights
        (dcora_exchange_certify_live; SPMD, the same eta on every rank): no Q is passed in, no X crosses to a host.
        -> (certified, theta, lambda_min of S + eta I, v, matvecs, distributed, info); info: the PSD test's eight
        numbers (as is_psd_device reports them), "rounds" through the segment's X area, "ms" to the verdict on rank 0"""
        cert, dist = C.c_int(), C.c_int()
        th, lm, mv = C.c_double(), C.c_double(), C.c_longlong()
        v, i10 = np.zeros(self.s.k), np.zeros(10)
        check(capi.lib().dcora_exchange_certify_live(self.h, float(eta), C.byref(cert), C.byref(th), C.byref(lm),
                                                     v.ctypes.data_as(C.c_void_p), C.byref(mv), C.byref(dist),
                                                     i10.ctypes.data_as(C.c_void_p)))
        info = {"symbolic_ms": i10[0], "numeric_ms": i10[1], "arena_bytes": i10[2], "flops": i10[3],
                "levels": int(i10[4]), "launches": int(i10[5]), "logdet": i10[6], "lookup_ms": i10[7],
                "rounds": int(i10[8]), "ms": float(i10[9]), "info10": i10}
        return bool(cert.value), th.value, lm.value, v, mv.value, bool(dist.value), info

    def post(self, agents):
        a = np.ascontiguousarray(agents, dtype=np.int32)
        check(capi.lib().dcora_exchange_post(self.h, a, a.size))

    def wait(self, agents):
        a = np.ascontiguousarray(agents, dtype=np.int32)
        check(capi.lib().dcora_exchange_wait(self.h, a, a.size))

    def _eval(self, fn, *first):
        c2, gn, nxt = C.c_double(), C.c_double(), C.c_int()
        bn = np.zeros(self.s.R)
        check(fn(self.h, *first, C.byref(c2), C.byref(gn), bn.ctypes.data_as(C.c_void_p), C.byref(nxt)))
        return c2.value, gn.value, bn, nxt.value

    def evaluate(self):
        return self._eval(capi.lib().dcora_exchange_evaluate)

    def iterate(self, selected):
        return self._eval(capi.lib().dcora_exchange_rbcd_iterate, int(selected))

    def tick(self, agents, allow_adjacent=False):
        a = np.ascontiguousarray(agents, dtype=np.int32)
        check(capi.lib().dcora_exchange_rbcd_tick(self.h, a, a.size, int(allow_adjacent)))

    def run_coloured(self, max_sweeps=1000, rgrad_tol=0.1):
        """the sessions' run_coloured across the ranks: tick per colour, then evaluate (dcora_exchange_run_coloured)"""
        return _run_coloured(capi.lib().dcora_exchange_run_coloured, self.h, max_sweeps, rgrad_tol)

    def set_X(self, X):
        check(capi.lib().dcora_exchange_set_X(self.h, F(X)))

    def gather_X(self):
        out = np.zeros(self.s.r * self.s.k)
        check(capi.lib().dcora_exchange_gather_X(self.h, out))
        return unF(out, self.s.r, self.s.k)

    def barrier(self):
        check(capi.lib().dcora_exchange_barrier(self.h))

    def round(self, anchor_pose=0, anchor=None):
        """The sessions' round() across the ranks of the job (dcora_exchange_round; collective, the same arguments on
        every rank): every rank rounds the states of the agents it hosts against the shared anchor -- the lifted pose
        anchor_pose, sent by the rank that hosts it, or `anchor` (r x (d+1)) -- and every rank returns everything
        -> dict: trajectory and, on a range-aided job, unit_spheres and landmarks: the bits a single-process session at
        the same iterate returns.  No rounded cost: no rank holds the whole problem."""
        d, n, l, b = self.s._round_dims()
        a = _round_anchor(anchor, self.s.r, d)
        T, S, Lm = np.zeros(d * (d + 1) * n), np.zeros(max(d * l, 1)), np.zeros(max(d * b, 1))
        check(capi.lib().dcora_exchange_round(self.h, int(anchor_pose), None if a is None else a.ctypes.data_as(C.c_void_p),
                                              T.ctypes.data_as(C.c_void_p), S.ctypes.data_as(C.c_void_p),
                                              Lm.ctypes.data_as(C.c_void_p)))
        out = {"trajectory": unF(T, d, (d + 1) * n)}
        if isinstance(self.s, RaRbcdSession):
            out["unit_spheres"], out["landmarks"] = unF(S[:d * l], d, l), unF(Lm[:d * b], d, b)
        return out

    def lift(self, theta, v, gradient_tolerance=1e-6, preconditioned_gradient_tolerance=1e-6, is_second_order=False):
        """The staircase's step of the whole job (dcora_exchange_lift; SPMD: the same theta, v -- k numbers, as certify
        returns them -- and tolerances on every rank): the session lift's search over trial points the ranks form
        together, the preconditioned norm taken with the agents' own preconditioners -> (escaped, info).  escaped
        False: the job is as it was.  The session's r follows its rank.  Needs room: reserve_rank on the session before
        the exchange is created, or r_reserve of robust_ranked_session / ra_robust_ranked_session."""
        v = None if v is None else np.ascontiguousarray(v, np.float64)
        if v is not None and v.shape != (self.s.k,):
            raise ValueError("lift needs the certificate's v: k numbers")
        p = capi.LiftParams()
        check(capi.lib().dcora_lift_params_default(C.byref(p)))
        p.gradient_tolerance = gradient_tolerance
        p.preconditioned_gradient_tolerance = preconditioned_gradient_tolerance
        p.is_second_order = int(bool(is_second_order))
        esc, i8, r = C.c_int(), np.zeros(8), C.c_int()
        check(capi.lib().dcora_exchange_lift(self.h, float(theta), None if v is None else v.ctypes.data_as(C.c_void_p),
                                             C.byref(p), C.byref(esc), i8.ctypes.data_as(C.c_void_p)))
        rank_fn = capi.lib().dcora_ra_rbcd_rank if isinstance(self.s, RaRbcdSession) else capi.lib().dcora_rbcd_rank
        check(rank_fn(self.s.h, C.byref(r)))
        self.s.r = r.value
        info = {"trials": int(i8[0]), "alpha": i8[1], "f_before": i8[2], "f_after": i8[3],
                "redimension_ms": i8[6], "total_ms": i8[7]}
        return bool(esc.value), info

    def project(self):
        """The sessions' project() across the ranks of the job (dcora_exchange_project; collective): the job goes from
        rank r to rank d at Proj(V_d^T X) without leaving the library and keeps what lift keeps.  G = X X^T is the sum
        of the agents' own X_a X_a^T, formed by the ranks that host them and added in agent order on every rank: the
        same bits on every rank and for any number of ranks.  -> the dict RbcdSession.project returns (basis None where
        not projected; positive_dets counts over the job; cost_2f and gradnorm are evaluate() at the adopted point);
        everything but the three times is identical on every rank.  The session's r follows its rank."""
        r, d = self.s.r, self.s._round_dims()[0]
        sg, B, G, i8, c2, rr = np.zeros(r), np.zeros(r * d), np.zeros(r * r), np.zeros(8), C.c_double(), C.c_int()
        check(capi.lib().dcora_exchange_project(self.h, *(a.ctypes.data_as(C.c_void_p) for a in (sg, B, G)),
                                                C.byref(c2), i8.ctypes.data_as(C.c_void_p)))
        rank_fn = capi.lib().dcora_ra_rbcd_rank if isinstance(self.s, RaRbcdSession) else capi.lib().dcora_rbcd_rank
        check(rank_fn(self.s.h, C.byref(rr)))
        self.s.r = rr.value
        projected = bool(i8[0])
        return dict(projected=projected, reflected=bool(i8[1]), positive_dets=int(i8[2]), sigma=sg,
                    basis=unF(B, r, d) if projected else None, gram=unF(G, r, r), cost_2f=c2.value,
                    gradnorm=float(i8[3]), ms_kernels=float(i8[4]), ms_redimension=float(i8[5]), ms_total=float(i8[6]),
                    gram_chunk=int(i8[7]))

    # ---- robust jobs (robust_ranked_session / ra_robust_ranked_session: m is then the pose-pose count) ----
    def update_weights(self, reset_to_initial=False):
        """Agent::updateMeasurementWeights of every agent on every rank (collective); returns the loop closures'
        {accepted, rejected, undecided} counts of the whole job"""
        c = np.zeros(3, np.int32)
        check(capi.lib().dcora_exchange_update_weights(self.h, int(bool(reset_to_initial)),
                                                       c.ctypes.data_as(C.c_void_p)))
        return {"accepted": int(c[0]), "rejected": int(c[1]), "undecided": int(c[2])}

    def set_weights(self, w):
        """all m weights in dataset order, the same on every rank (collective)"""
        w = np.ascontiguousarray(w, np.float64)
        if w.shape != (self.s.m,):
            raise ValueError("set_weights needs one weight per measurement")
        check(capi.lib().dcora_exchange_set_weights(self.h, w))

    def get_weights(self):
        """all m weights of the job, the same on every rank (collective)"""
        w = np.zeros(self.s.m)
        check(capi.lib().dcora_exchange_get_weights(self.h, w))
        return w


def robust_ranked_session(ds, job_name, num_robots=5, r=5, robust=None, fixed_weight=None, rank=0, world_size=1,
                          device=0, acceleration=True, restart_interval=30, params=None, stream=None, r_reserve=0):
    """(RbcdSession, Exchange) of one rank of a robust multi-rank job (dcora_rbcd_create_robust_ranks): the robust
    session of RbcdSession(robust=...) for the agents this rank hosts, and its exchange under job_name.  Every rank
    calls this with the same arguments but rank; weights change through the exchange (update_weights / set_weights /
    get_weights), collectively.  The session's get_weights() is this rank's view (NaN for measurements touching none
    of its agents).  r_reserve: room for Exchange.lift up to that rank (dcora_rbcd_create_robust_ranks_reserved)."""
    from . import robust as rb
    robust = robust or rb.RobustCostParameters("GNC_TLS")
    o = _rbcd_options(num_robots, r, acceleration, restart_interval, params, rank, world_size, device, stream)
    fx = _fixed_flags(ds, fixed_weight)
    dsh = ds.handle()
    hs, hx = C.c_void_p(), C.c_void_p()
    try:
        check(capi.lib().dcora_rbcd_create_robust_ranks_reserved(dsh, C.byref(o), C.byref(robust.c),
                                                                 None if fx is None else fx.ctypes.data_as(C.c_void_p),
                                                                 int(r_reserve), job_name.encode(), C.byref(hs),
                                                                 C.byref(hx)))
    finally:
        capi.lib().dcora_dataset_destroy(dsh)
    s = RbcdSession.__new__(RbcdSession)
    s.ds, s.R, s.r, s.k, s.m, s.h = ds, num_robots, r, (ds.d + 1) * ds.n, ds.m, hs
    return s, Exchange(s, job_name, _handle=hx)


def ra_robust_ranked_session(ra, job_name, r, robust=None, fixed_weight=None, rank=0, world_size=1, device=0,
                             acceleration=True, restart_interval=30, params=None, r_reserve=0):
    """(RaRbcdSession, Exchange) of one rank of a robust multi-rank range-aided job (dcora_ra_rbcd_create_robust_ranks):
    robust_ranked_session's contract with the robust session of RaRbcdSession(robust=...) for the agents this rank
    hosts.  Every rank calls this with the same arguments but rank; the job's weights (pose-pose order) change through
    the exchange (update_weights / set_weights / get_weights), collectively.  The session's get_weights() is this
    rank's view (NaN for pose-pose measurements touching none of its agents).  r_reserve: room for Exchange.lift up to
    that rank (dcora_ra_rbcd_create_robust_ranks_reserved)."""
    from . import robust as rb
    s = RaRbcdSession(ra, r, acceleration=acceleration, restart_interval=restart_interval, params=params,
                      device=device, rank=rank, world_size=world_size,
                      robust=robust or rb.RobustCostParameters("GNC_TLS"), fixed_weight=fixed_weight,
                      _ranked_job=job_name, _r_reserve=r_reserve)
    hx, s._exchange_handle = s._exchange_handle, None
    return s, Exchange(s, job_name, _handle=hx)


class RaRbcdSession(_Session):
    """the agents of a multi-robot range-aided SLAM problem + the synchronous RBCD++ driver on the device
    (ref examples/MultiRobotExample_RASLAM.cpp); X is the merged r x k matrix in the RA ordering; a robust session's
    weights are in pose-pose order"""
    _prefix = "dcora_ra_rbcd_"
    _per = "pose-pose measurement"

    def __init__(self, ra, r, acceleration=True, restart_interval=30, params=None, device=0, rank=0, world_size=1,
                 robust=None, fixed_weight=None, _ranked_job=None, _r_reserve=0):
        """robust: a robust.RobustCostParameters -> a session whose pose-pose weights update in place (update_weights /
        set_weights / get_weights / robust_info, as RbcdSession's); it starts with weight 1 on every loop closure
        (ra.loop_closures()) whose fixed_weight flag (one per pose-pose measurement, default none) is off"""
        self.ra, self.r, self.k = ra, r, ra.k
        self.m = ra.num_pose_pose
        o = RbcdOptions()
        capi.lib().dcora_rbcd_options_default(C.byref(o))
        o.r, o.acceleration, o.restart_interval, o.device = r, int(acceleration), restart_interval, device
        o.rank, o.world_size = rank, world_size
        if params is not None:
            o.local = params.c
        fx = None
        if robust is not None and fixed_weight is not None:
            fx = np.ascontiguousarray(fixed_weight, np.int32)
            if fx.shape != (self.m,):
                raise ValueError("fixed_weight needs one flag per pose-pose measurement")
        fxp = None if fx is None else fx.ctypes.data_as(C.c_void_p)
        dsh = ra.handle()
        self.h = C.c_void_p()
        try:
            if robust is None:
                check(capi.lib().dcora_ra_rbcd_create(dsh, C.byref(o), C.byref(self.h)))
            elif _ranked_job is None:
                check(capi.lib().dcora_ra_rbcd_create_robust(dsh, C.byref(o), C.byref(robust.c), fxp, C.byref(self.h)))
            else:  # (ra_robust_ranked_session: made together with its exchange, whose handle goes to _exchange_handle)
                self._exchange_handle = C.c_void_p()
                check(capi.lib().dcora_ra_rbcd_create_robust_ranks_reserved(dsh, C.byref(o), C.byref(robust.c), fxp,
                                                                            int(_r_reserve), _ranked_job.encode(),
                                                                            C.byref(self.h),
                                                                            C.byref(self._exchange_handle)))
        finally:
            capi.lib().dcora_radataset_destroy(dsh)
        n = C.c_int()
        check(capi.lib().dcora_ra_rbcd_info(self.h, C.byref(n), None))
        self.R = n.value
        rb = np.zeros(self.R, np.int32)
        check(capi.lib().dcora_ra_rbcd_info(self.h, C.byref(n), rb.ctypes.data_as(C.c_void_p)))
        self.robots = rb.tolist()

    def _round_dims(self):
        return self.ra.d, self.ra.n, self.ra.l, self.ra.b

    def lift(self, theta, v, gradient_tolerance=1e-4, preconditioned_gradient_tolerance=1e-4, is_second_order=False,
             central_reg=None):
        """RbcdSession.lift on the merged problem (dcora_ra_rbcd_lift); v in the global RA ordering.  The tolerances
        default to multi_robot_raslam_example's."""
        return self._lift(theta, v, gradient_tolerance, preconditioned_gradient_tolerance, is_second_order, central_reg)


def align_lifted_trajectory_to_frame(X, anchor, d, n, global_alignment=True, device=0):
    """alignLiftedTrajectoryToFrame (ref src/DCORA_utils.cpp:2262-2289): X r x (d+1) n (SE ordering), anchor
    r x (d+1) -> d x (d+1) n with rotation blocks in SO(d)"""
    X = np.asarray(X, dtype=np.float64)
    dims = Dims(X.shape[0], d, n, 0, 0)
    out = np.zeros(d * (d + 1) * n)
    a = None if anchor is None else F(anchor)
    check(capi.lib().dcora_round_align_trajectory(C.byref(dims), F(X), None if a is None else a.ctypes.data_as(C.c_void_p),
                                                  int(global_alignment), out, None, None, device))
    return unF(out, d, (d + 1) * n)


def ra_states_in_local_frame(X, r, d, n, l, b, device=0):
    """Agent::getStatesInLocalFrame (ref src/Agent.cpp:950-1003): X r x k (RA ordering) -> (trajectory d x (d+1) n in
    the SE ordering, unit spheres d x l, landmarks d x b), all in the frame of pose 0"""
    dims = Dims(r, d, n, l, b, capi.LAYOUT_RA)
    T, S, Lm = np.zeros(d * (d + 1) * n), np.zeros(max(d * l, 1)), np.zeros(max(d * b, 1))
    check(capi.lib().dcora_round_align_trajectory(C.byref(dims), F(X), None, 0, T, S.ctypes.data_as(C.c_void_p),
                                                  Lm.ctypes.data_as(C.c_void_p), device))
    return unF(T, d, (d + 1) * n), unF(S[:d * l], d, l), unF(Lm[:d * b], d, b)


def project_solution_raslam(X, r, d, n, l, b, device=0):
    """projectSolutionRASLAM (ref src/DCORA_utils.cpp:1984-2031): r x k -> d x k"""
    dims = Dims(r, d, n, l, b, capi.LAYOUT_RA)
    k = (d + 1) * n + l + b
    out = np.zeros(d * k)
    check(capi.lib().dcora_round_project_solution_raslam(C.byref(dims), F(X), out, device))
    return unF(out, d, k)


def log_trajectory(path, T, d, n):
    """Logger::logTrajectory (ref src/Logger.cpp:107-145): T is d x (d+1) n"""
    check(capi.lib().dcora_log_trajectory(str(path).encode(), d, n, F(np.asarray(T, dtype=np.float64))))


def _agent_iterate(self, agent, do_optimization=True):
    """Agent::iterate(doOptimization) of one agent (agents advance in lockstep)"""
    check(capi.lib().dcora_rbcd_agent_iterate(self.h, agent, int(bool(do_optimization))))


def _agent_info(self, agent):
    npz, first, it = C.c_int(), C.c_int(), C.c_int()
    check(capi.lib().dcora_rbcd_agent_info(self.h, agent, C.byref(npz), C.byref(first), C.byref(it)))
    return dict(num_poses=npz.value, first_pose=first.value, iteration_number=it.value)


def _agent_get_X(self, agent):
    cols = (self.ds.d + 1) * _agent_info(self, agent)["num_poses"]
    out = np.zeros(self.r * cols)
    check(capi.lib().dcora_rbcd_agent_get_X(self.h, agent, out))
    return unF(out, self.r, cols)


def _agent_set_X(self, agent, X):
    check(capi.lib().dcora_rbcd_agent_set_X(self.h, agent, F(X)))


RbcdSession.agent_iterate = _agent_iterate
RbcdSession.agent_get_X = _agent_get_X
RbcdSession.agent_set_X = _agent_set_X
RbcdSession.agent_info = _agent_info


# ---- agent status and the team's decisions (ref src/Agent.cpp:558-586, 1123-1156, 1280-1330) ----
def team_params(**kw):
    """capi.TeamParams with the reference's defaults (ref include/DCORA/Agent.h:113-125), fields overridden by kw"""
    p = capi.TeamParams()
    capi.lib().dcora_team_params_default(C.byref(p))
    for k, v in kw.items():
        if k not in dict(capi.TeamParams._fields_):
            raise TypeError("unknown team parameter %r" % k)
        setattr(p, k, v)
    return p


def _as_status(s):
    if isinstance(s, capi.AgentStatus):
        return s
    return capi.AgentStatus(int(s["agent_id"]), int(s.get("state", capi.AGENT_INITIALIZED)),
                            int(s.get("instance_number", 0)), int(s["iteration_number"]),
                            int(bool(s["ready_to_terminate"])), float(s["relative_change"]))


def team_ready_to_terminate(params, robust, weight_update_count, success, relative_change, accepted, rejected, total):
    """the local rule of Agent::iterate (ref src/Agent.cpp:567-585)"""
    ready = C.c_int()
    check(capi.lib().dcora_team_ready_to_terminate(C.byref(params), int(bool(robust)), int(weight_update_count),
                                                   int(bool(success)), float(relative_change), int(accepted),
                                                   int(rejected), int(total), C.byref(ready)))
    return bool(ready.value)


def team_decide(params, robust, iteration_number, weight_update_count, inner_iter, latest_weight_update_iteration,
                statuses, active=None):
    """Agent::shouldTerminate and shouldUpdateMeasurementWeights (ref src/Agent.cpp:1123-1156, 1280-1330) on the host.
    statuses: one entry per robot -- a status (capi.AgentStatus or the dict RbcdSession.agent_status returns) or None
    where it is absent; active: flags per robot (None: all active).  Returns (should_terminate, should_update_weights)"""
    n = len(statuses)
    arr = (capi.AgentStatus * max(n, 1))()
    have = np.zeros(max(n, 1), np.int32)
    for q, s in enumerate(statuses):
        if s is not None:
            arr[q] = _as_status(s)
            have[q] = 1
    act = None if active is None else np.ascontiguousarray(active, np.int32)
    term, upd = C.c_int(), C.c_int()
    check(capi.lib().dcora_team_decide(C.byref(params), int(bool(robust)), int(iteration_number),
                                       int(weight_update_count), int(inner_iter),
                                       int(latest_weight_update_iteration), arr, have.ctypes.data_as(C.c_void_p),
                                       None if act is None else act.ctypes.data_as(C.c_void_p), n, C.byref(term),
                                       C.byref(upd)))
    return bool(term.value), bool(upd.value)


def max_translation_distance(X, Y, d):
    """LiftedArray::maxTranslationDistance (ref src/manifold/Elements.cpp:59-69) of two r x (d+1) n lifted pose arrays,
    on the device by the kernel of the agents' relative change"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    if X.shape != Y.shape or X.ndim != 2 or X.shape[1] % (d + 1):
        raise ValueError("max_translation_distance needs two r x (d+1) n arrays")
    out = C.c_double()
    check(capi.lib().dcora_max_translation_distance(X.shape[0], d, X.shape[1] // (d + 1), F(X), F(Y), C.byref(out)))
    return out.value


def ra_max_translation_distance(X, Y, d, n, l=0, b=0):
    """the same over the poses of two r x k arrays in the RA ordering [rotations | l unit spheres | translations |
    b landmarks], k = (d+1) n + l + b, by the kernel of a range-aided agent's relative change: unit spheres and
    landmarks never count"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    if X.shape != Y.shape or X.ndim != 2 or X.shape[1] != (d + 1) * n + l + b:
        raise ValueError("ra_max_translation_distance needs two r x ((d+1) n + l + b) arrays")
    out = C.c_double()
    check(capi.lib().dcora_ra_max_translation_distance(X.shape[0], d, n, l, b, F(X), F(Y), C.byref(out)))
    return out.value


def debug_launch_count():
    """kernel launches of the RBCD chain's wrappers in this process so far (dcora_debug_launch_count): the counter
    RbcdSession.debug_launches reads, for sessions and exchanges of either kind"""
    out = C.c_longlong()
    check(capi.lib().dcora_debug_launch_count(C.byref(out)))
    return out.value


def _team_fn(self, name):
    """the team entry of a session (dcora_rbcd_<name>, dcora_ra_rbcd_<name>) or of a job's exchange of either kind
    (dcora_exchange_<name>: Exchange(session, ...), robust_ranked_session, ra_robust_ranked_session)"""
    return getattr(capi.lib(), self._prefix + name)


def _enable_team(self, params=None, **kw):
    """opt in to the team protocol (dcora_rbcd_team_enable / dcora_ra_rbcd_team_enable; on an Exchange
    dcora_exchange_team_enable, SPMD): every
    iterate(true) of an agent stores its status -- across the ranks of a job, on every rank"""
    self.team = params if params is not None else team_params(**kw)
    check(_team_fn(self, "team_enable")(self.h, C.byref(self.team)))
    return self.team


def _agent_status(self, agent):
    """the agent's AgentStatus as a dict, or None when it has not optimised since the statuses were last cleared"""
    st, known = capi.AgentStatus(), C.c_int()
    check(_team_fn(self, "agent_status")(self.h, agent, C.byref(st), C.byref(known)))
    return st.as_dict() if known.value else None


def _loop_closure_stats(self, agent):
    c = np.zeros(3, np.int32)
    check(_team_fn(self, "loop_closure_stats")(self.h, agent, c))
    return {"accepted": int(c[0]), "rejected": int(c[1]), "total": int(c[2])}


def _should_terminate(self):
    yes = C.c_int()
    check(_team_fn(self, "should_terminate")(self.h, C.byref(yes)))
    return bool(yes.value)


def _should_update_weights(self):
    yes = C.c_int()
    check(_team_fn(self, "should_update_weights")(self.h, C.byref(yes)))
    return bool(yes.value)


def _team_info(self):
    c = np.zeros(4, np.int32)
    check(_team_fn(self, "team_info")(self.h, c))
    return {"inner_iter": int(c[0]), "latest_weight_update_iteration": int(c[1]), "weight_updates": int(c[2]),
            "resets": int(c[3])}


def _run_team(self):
    """the agents' own loop (dcora_rbcd_run_team / dcora_ra_rbcd_run_team / dcora_exchange_run_team): until
    should_terminate(), each pass
    re-weights when should_update_weights() says so, then iterates the greedily selected agent"""
    n = max(int(self.team.max_num_iters), 1)
    it, nupd, why = C.c_int(), C.c_int(), C.c_int()
    cost, gn = np.zeros(n), np.zeros(n)
    sel, upd = np.zeros(n, np.int32), np.zeros(n, np.int32)
    check(_team_fn(self, "run_team")(self.h, C.byref(it), cost.ctypes.data_as(C.c_void_p),
                                     gn.ctypes.data_as(C.c_void_p), sel.ctypes.data_as(C.c_void_p),
                                     upd.ctypes.data_as(C.c_void_p), C.byref(nupd), C.byref(why)))
    k = it.value
    return dict(iters=k, cost=cost[:k], gradnorm=gn[:k], selected=sel[:k], updated=upd[:k],
                weight_updates=nupd.value,
                stop_reason={capi.TEAM_STOP_ALL_READY: "all_ready", capi.TEAM_STOP_MAX_ITERS: "max_iters"}[why.value])


# the same records from a session of either kind and from the exchange of a multi-rank job
def _enable_team_ra(self, params=None, **kw):
    """Exchange.enable_team for the exchange of a range-aided job (dcora_exchange_team_enable_ra, SPMD; enable_team keeps
    refusing such an exchange): Exchange(RaRbcdSession, ...) or the exchange of ra_robust_ranked_session.  Afterwards
    agent_status, loop_closure_stats, should_terminate, should_update_weights, team_info and run_team are the exchange's
    as on a pose-graph job"""
    self.team = params if params is not None else team_params(**kw)
    check(capi.lib().dcora_exchange_team_enable_ra(self.h, C.byref(self.team)))
    return self.team


Exchange.enable_team_ra = _enable_team_ra

for _cls in (RbcdSession, RaRbcdSession, Exchange):
    _cls.enable_team = _enable_team
    _cls.agent_status = _agent_status
    _cls.loop_closure_stats = _loop_closure_stats
    _cls.should_terminate = _should_terminate
    _cls.should_update_weights = _should_update_weights
    _cls.team_info = _team_info
    _cls.run_team = _run_team
