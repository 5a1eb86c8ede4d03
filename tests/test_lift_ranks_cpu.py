"""Room for the ranks to come, without a device (dcora_amd/csrc/exchange_slots.h through tests/cpp/lift_layout.cpp, a
plain host program): the segment of a job at rank r that reserved reserve_r is, offset by offset, the segment of a job
created at max(r, reserve_r); with no reserve it is the layout a job had before there was one (slot = maxcols r rounded
up to 16 doubles, an X area of r k doubles: what Exchange::init computed); and the reserve entries accept
d <= r <= r_reserve <= 16 only."""
import os
import subprocess

import pytest

import common

ROOT = os.path.dirname(common.HERE)
BAD_ARG = 1


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lift") / "lift_layout")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "dcora_amd", "csrc"), "-I",
                    os.path.join(ROOT, "include"), os.path.join(common.HERE, "cpp", "lift_layout.cpp"), "-lpthread", "-o",
                    out], check=True, capture_output=True, timeout=600)
    return out


def run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (args, out.stdout, out.stderr)
    return out.stdout.strip()


SHAPES = [  # world, R, maxcols, k, w
    (1, 1, 1, 4, 0), (2, 4, 100, 500, 0), (2, 5, 37, 500, 312), (4, 5, 88, 500, 0), (3, 2, 1, 181, 40),
    (64, 64, 2000, 400000, 123457),
]


@pytest.mark.parametrize("world,R,maxcols,k,w", SHAPES)
def test_reserved_layout_is_the_layout_of_a_job_created_at_the_larger_rank(exe, world, R, maxcols, k, w):
    for r, reserve in ((3, 4), (3, 9), (5, 16), (4, 4), (7, 5), (2, 3)):
        top = max(r, reserve)
        got = run(exe, "layout", world, R, maxcols, r, reserve, k, w)
        assert got == run(exe, "layout", world, R, maxcols, top, 0, k, w), (r, reserve)
        assert got == run(exe, "layout", world, R, maxcols, top, top, k, w)


@pytest.mark.parametrize("world,R,maxcols,k,w", SHAPES)
def test_no_reserve_is_the_layout_jobs_had(exe, world, R, maxcols, k, w):
    """what Exchange::init computed before it knew of a reserve: slot = align_up(maxcols r, 16), x = r k"""
    for r in (2, 3, 5, 8, 16):
        slot = (maxcols * r + 15) // 16 * 16
        assert run(exe, "layout", world, R, maxcols, r, 0, k, w) == run(exe, "plain", world, R, slot, r * k, w), r


def test_only_slots_and_the_x_area_follow_the_reserve(exe):
    """every area before the staged slots lies where it lay; the staged slots begin where they began"""
    a = run(exe, "layout", 2, 5, 37, 3, 0, 500, 312).split()
    b = run(exe, "layout", 2, 5, 37, 3, 8, 500, 312).split()
    bar = a.index("|")
    names = ["ranks", "flags", "evals", "consumed", "red", "status", "status_read", "probe_flags", "probe_res",
             "probe_stage", "staged", "x", "w", "total"]
    offs_a, offs_b = dict(zip(names, a[bar + 1:])), dict(zip(names, b[bar + 1:]))
    for name in names[:names.index("staged") + 1]:
        assert offs_a[name] == offs_b[name], name
    assert int(offs_b["x"]) > int(offs_a["x"]) and int(offs_b["total"]) > int(offs_a["total"])
    assert (a[2], b[2]) == (str((37 * 3 + 15) // 16 * 16), str((37 * 8 + 15) // 16 * 16))
    assert (a[3], b[3]) == (str(3 * 500), str(8 * 500))


def test_reserve_argument_checks(exe):
    """dcora_rbcd_reserve_rank / dcora_ra_rbcd_reserve_rank (0 is no reserve only for the *_reserved creators)"""
    ok = lambda d, r, rr, zero=0: int(run(exe, "check", d, r, rr, zero))
    for d, r, rr in ((3, 3, 3), (3, 3, 4), (3, 5, 16), (2, 2, 16), (3, 16, 16)):
        assert ok(d, r, rr) == 0 and ok(d, r, rr, 1) == 0
    for d, r, rr in ((3, 5, 4), (3, 5, 17), (3, 2, 5), (3, 5, -1), (2, 3, 2)):
        assert ok(d, r, rr) == BAD_ARG and ok(d, r, rr, 1) == BAD_ARG
    assert ok(3, 5, 0) == BAD_ARG and ok(3, 5, 0, 1) == 0
