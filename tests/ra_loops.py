"""A loop-closure variant of tiers.pyfg: the only real multi-robot range-aided fixture has odometry and ranges but not one
pose-pose loop closure, so the robust-session tests write a variant of it at run time.  Kept: the first P poses of each
of the four robots (by pose number), the landmark, the odometry among the kept poses and every range whose two ends are
kept.  Added after the file's own lines, so that they are the last pose-pose measurements of the dataset, in this order:

    inter-robot closures, `per_pair` for each of the six robot pairs         kind "inter"
    intra-robot closures, `intra` per robot, between poses >= 5 apart        kind "intra"
    gross outliers, `outliers` of them, alternating inter- and intra-robot   kind "outlier"

A closure's measurement is the relative pose of the file's ground-truth vertices (VERTEX_SE2), exactly; an outlier's is
a seeded rotation uniform in (-pi, pi] and a translation 5 * N(0, I) off the true one.  All carry the covariance
diag(0.01, 0.01, 0.0025), i.e. tau = 100, kappa = 400.  Numbers are written with repr(), so a re-read returns them.

The GNC fixture (GNC_FIXTURE, GNC_PARAMS): P = 60, seed 11, 3 closures per robot pair, 2 per robot, 6 outliers;
GNC-TLS with GNCBarc = 10 and GNCMuStep = 2, the values of the pose-graph GNC tests, which needed no change; rank 3, 12
weight updates.  Under the same schedule over the oracle's centralised solver (test_ra_robust_cpu.py) the ground-truth
closures end with residuals <= 0.77 and the outliers with residuals >= 45.4: a factor 6 and a factor 4 beyond the
factor 2 of room the tests ask for on either side of GNCBarc."""
import gzip
import itertools
import os

import numpy as np

import common

ROBOTS = "ABCD"
COV = "0.01 0.0 0.0 0.01 0.0 0.0025"
TAU, KAPPA = 100.0, 400.0

# The GNC fixture (test_ra_robust_cpu.py checks the condition, test_ra_gnc_session_gpu.py runs the flow): the variant
# at P = 60 with this seed and these counts, GNC-TLS with GNCBarc = 10 and GNCMuStep = 2 (the values of the pose-graph
# GNC tests), rank 3.  With them the reference algorithm alone -- the GNC schedule over the oracle's centralised solver
# -- leaves every ground-truth closure with a residual below GNCBarc / 2 and every outlier above 2 GNCBarc.
GNC_FIXTURE = dict(P=60, seed=11, per_pair=3, intra=2, outliers=6)
GNC_PARAMS = dict(GNCBarc=10.0, GNCMuStep=2.0)


def _wrap(a):
    return float(np.arctan2(np.sin(a), np.cos(a)))


def relative_pose(pa, pb):
    """(x, y, theta) of pose b in the frame of pose a; poses are (x, y, theta)"""
    c, s = np.cos(pa[2]), np.sin(pa[2])
    dx, dy = pb[0] - pa[0], pb[1] - pa[1]
    return float(c * dx + s * dy), float(-s * dx + c * dy), _wrap(pb[2] - pa[2])


def write_loops_variant(directory, P, seed=1, per_pair=3, intra=2, outliers=4, tag=None):
    """-> path of the variant (plain .pyfg) in `directory` and a dict: closures (list of (symbol a, symbol b, x, y, theta)
    in file order), kind (one of "inter" / "intra" / "outlier" each), n_odometry (pose-pose measurements before them),
    n_ranges, poses (symbol -> ground-truth (x, y, theta))"""
    path = os.path.join(str(directory), tag or ("tiers_loops_%d_%d.pyfg" % (P, seed)))
    with gzip.open(os.path.join(common.DATA, "tiers.pyfg.gz"), "rt") as src:
        lines = src.readlines()
    numbers = {rb: [] for rb in ROBOTS}
    for line in lines:
        f = line.split()
        if f and f[0] == "VERTEX_SE2":
            numbers[f[2][0]].append(int(f[2][1:]))
    kept = set()
    order = {}
    for rb in ROBOTS:
        order[rb] = sorted(numbers[rb])[:P]
        kept.update("%s%d" % (rb, i) for i in order[rb])
    poses, out = {}, []
    n_odometry = n_ranges = 0
    for line in lines:
        f = line.split()
        if not f:
            continue
        if f[0] == "VERTEX_SE2":
            if f[2] not in kept:
                continue
            poses[f[2]] = (float(f[3]), float(f[4]), float(f[5]))
        elif f[0] == "VERTEX_XY":
            kept.add(f[1])
        elif f[0] == "EDGE_SE2":
            if f[2] not in kept or f[3] not in kept:
                continue
            n_odometry += 1
        elif f[0] == "EDGE_RANGE":
            if f[2] not in kept or f[3] not in kept:
                continue
            n_ranges += 1
        out.append(line if line.endswith("\n") else line + "\n")
    rng = np.random.default_rng(seed)
    sym = lambda rb, q: "%s%d" % (rb, order[rb][q])
    closures, kind = [], []

    def inter_pair(ra, rb):
        return sym(ra, int(rng.integers(0, P))), sym(rb, int(rng.integers(0, P)))

    def intra_pair(rb):
        i = int(rng.integers(0, P - 5))
        j = int(rng.integers(i + 5, P))
        return sym(rb, i), sym(rb, j)

    def add(a, b, what):
        x, y, th = relative_pose(poses[a], poses[b])
        if what == "outlier":
            x, y = x + 5.0 * rng.standard_normal(), y + 5.0 * rng.standard_normal()
            th = float(rng.uniform(-np.pi, np.pi))
        closures.append((a, b, float(x), float(y), float(th)))
        kind.append(what)

    for ra, rb in itertools.combinations(ROBOTS, 2):
        for _ in range(per_pair):
            add(*inter_pair(ra, rb), "inter")
    for rb in ROBOTS:
        for _ in range(intra):
            add(*intra_pair(rb), "intra")
    pairs = list(itertools.combinations(ROBOTS, 2))
    for q in range(outliers):
        if q % 2 == 0:
            ra, rb = pairs[int(rng.integers(0, len(pairs)))]
            add(*inter_pair(ra, rb), "outlier")
        else:
            add(*intra_pair(ROBOTS[int(rng.integers(0, len(ROBOTS)))]), "outlier")
    for a, b, x, y, th in closures:
        out.append("EDGE_SE2 0.0 %s %s %r %r %r %s\n" % (a, b, x, y, th, COV))
    with open(path, "w") as dst:
        dst.writelines(out)
    return path, dict(closures=closures, kind=kind, n_odometry=n_odometry, n_ranges=n_ranges, poses=poses)


def closure_masks(info):
    """(inlier closures, outliers): boolean masks over the pose-pose measurements of the variant"""
    m = info["n_odometry"] + len(info["kind"])
    inl, outl = np.zeros(m, bool), np.zeros(m, bool)
    for q, what in enumerate(info["kind"]):
        (outl if what == "outlier" else inl)[info["n_odometry"] + q] = True
    return inl, outl
