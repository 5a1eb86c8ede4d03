"""The refusals of the robust, team and create entries of both session kinds, word for word: status, full text, and
the session left as it was (get_weights() and get_X() unchanged).  Both kinds state them once, composed from the
session's tag ("rbcd" / "ra_rbcd"); the texts below are the literals of the two copies that stood before that, entry
names included.  The datasets are the smallest of tests/golden: 6 poses, 8 pose-pose measurements, 2 robots."""
import uuid

import numpy as np
import pytest

import common
from test_raslam import ra_path

pytestmark = pytest.mark.gpu

BAD_ARG, UNSUPPORTED = 1, 8
R_RELAX = 4
ZERO_EDGE = 6  # a loop closure inside the first robot in both datasets: fixed at weight 0, so in no pattern

TEXTS = {
    "rbcd": dict(
        not_robust="rbcd robust: the session was not created by dcora_rbcd_create_robust",
        multi_process="rbcd robust: only single-process sessions (world_size 1) update weights",
        create_world="rbcd robust: dcora_rbcd_create_robust makes single-process sessions (world_size 1); a multi-rank "
                     "job creates its sessions with dcora_rbcd_create_robust_ranks",
        reserve="rbcd robust: r_reserve is 0 (no reserve) or d <= r <= r_reserve <= 16",
        ranked="rbcd robust: the session belongs to a multi-rank job (dcora_rbcd_create_robust_ranks): "
               "its weights change through ",
        team="rbcd team: the session has not called dcora_rbcd_team_enable",
        weights="rbcd robust: weights must be finite and >= 0",
        zero="rbcd robust: a weight that was 0 at creation cannot become nonzero (the session's patterns "
             "do not hold that measurement)"),
    "ra_rbcd": dict(
        not_robust="ra_rbcd robust: the session was not created by dcora_ra_rbcd_create_robust",
        multi_process="ra_rbcd robust: only single-process sessions (world_size 1) update weights",
        create_world="ra_rbcd robust: dcora_ra_rbcd_create_robust makes single-process sessions (world_size 1); "
                     "a multi-rank job creates its sessions with dcora_ra_rbcd_create_robust_ranks",
        reserve="ra_rbcd robust: r_reserve is 0 (no reserve) or d <= r <= r_reserve <= 16",
        ranked="ra_rbcd robust: the session belongs to a multi-rank job "
               "(dcora_ra_rbcd_create_robust_ranks): its weights change through ",
        team="ra_rbcd team: the session has not called dcora_ra_rbcd_team_enable",
        weights="ra_rbcd robust: weights must be finite and >= 0",
        zero="ra_rbcd robust: a weight that was 0 at creation cannot become nonzero (the session's patterns "
             "do not hold that measurement)"),
}


@pytest.fixture(scope="module")
def da(built):
    import dcora_amd
    if dcora_amd.device_count() < 1:
        pytest.fail("no GPU visible: the product has no CPU fallback")
    return dcora_amd


class Kind:
    """one session kind on its dataset, whose measurement ZERO_EDGE carries weight 0: sessions of every flavour, a
    start point, the fixed flags that keep the 0"""

    def __init__(self, da, kind):
        self.da, self.kind = da, kind
        rng = np.random.default_rng(7)
        if kind == "rbcd":
            self.ds = common.product_dataset("pose_graph_optimization_test_3d")
            self.ds.vals[ZERO_EDGE, -1] = 0.0
            self.m = self.ds.m
            self.X0 = da.manifold_project(R_RELAX, 3, self.ds.n, rng.uniform(-1, 1, (R_RELAX, 4 * self.ds.n)))
        else:
            self.ds = da.RADataset(ra_path("range_aided_slam_test_3d"))
            self.m = self.ds.num_pose_pose
            w = np.ones(self.m)
            w[ZERO_EDGE] = 0.0
            self.ds.set_pose_pose_weights(w)
            self.X0 = da.manifold_project(R_RELAX, 3, self.ds.n, rng.uniform(-1, 1, (R_RELAX, self.ds.k)),
                                          l=self.ds.l, b=self.ds.b)
        self.fixed = np.zeros(self.m, bool)
        self.fixed[ZERO_EDGE] = True

    def session(self, robust=None, **kw):
        if robust is not None:
            kw.update(robust=robust, fixed_weight=self.fixed)
        if self.kind == "rbcd":
            return self.da.RbcdSession(self.ds, num_robots=2, r=R_RELAX, **kw)
        return self.da.RaRbcdSession(self.ds, R_RELAX, **kw)

    def ranked(self, robust, **kw):
        job = "rf%s" % uuid.uuid4().hex[:10]
        if self.kind == "rbcd":
            return self.da.robust_ranked_session(self.ds, job, num_robots=2, r=R_RELAX, robust=robust,
                                                 fixed_weight=self.fixed, **kw)
        return self.da.ra_robust_ranked_session(self.ds, job, R_RELAX, robust=robust, fixed_weight=self.fixed, **kw)


def refused(da, call, status, text):
    with pytest.raises(da.DcoraError) as e:
        call()
    assert e.value.status == status
    assert str(e.value) == "dcora status %d: %s" % (status, text)


@pytest.mark.parametrize("kind", ["rbcd", "ra_rbcd"])
def test_refusals_word_for_word(da, kind):
    from dcora_amd import robust as rb
    T = TEXTS[kind]
    K = Kind(da, kind)
    params = rb.RobustCostParameters("GNC_TLS", GNCBarc=10.0, GNCMuStep=2.0)
    w_any = np.ones(K.m)

    # ---- creation: a robust session of one process with world_size != 1, a reserve that is no rank
    refused(da, lambda: K.session(robust=params, world_size=2), UNSUPPORTED, T["create_world"])
    refused(da, lambda: K.ranked(params, r_reserve=17), BAD_ARG, T["reserve"])

    # ---- a plain session asked for weights, of one process and of a job; a team query before team_enable
    for world, status, text in ((1, BAD_ARG, T["not_robust"]), (2, UNSUPPORTED, T["multi_process"])):
        P = K.session(world_size=world)
        P.set_X(K.X0)
        for call in (P.update_weights, lambda: P.set_weights(w_any), P.get_weights, P.robust_info):
            refused(da, call, status, text)
        for call in (lambda: P.agent_status(0), lambda: P.loop_closure_stats(0), P.should_terminate,
                     P.should_update_weights, P.team_info):
            refused(da, call, BAD_ARG, T["team"])
        assert np.array_equal(P.get_X(), K.X0)
        P.close()

    # ---- a robust session: a team query before team_enable, weights that are no weights, a creation zero made nonzero
    S = K.session(robust=params)
    S.set_X(K.X0)
    S.run(max_iters=3, rgrad_tol=0.0)
    w0, X = S.get_weights(), S.get_X()
    assert w0[ZERO_EDGE] == 0.0 and w0.shape == (K.m,)
    refused(da, S.should_terminate, BAD_ARG, T["team"])
    for at, v, text in ((1, -0.5, T["weights"]), (1, np.nan, T["weights"]), (K.m - 1, np.inf, T["weights"]),
                        (ZERO_EDGE, 0.5, T["zero"])):
        w = w0.copy()
        w[at] = v
        refused(da, lambda: S.set_weights(w), BAD_ARG, text)
        assert np.array_equal(S.get_weights(), w0) and np.array_equal(S.get_X(), X)
    info = S.robust_info()
    S.update_weights()  # ... and it is still a robust session that works
    assert S.robust_info()["updates"] == info["updates"] + 1 and S.get_weights()[ZERO_EDGE] == 0.0
    S.close()

    # ---- the session of a job's rank asked for a weight change of its own
    B, ex = K.ranked(params)
    try:
        ex.set_X(K.X0)
        w0, X = B.get_weights(), B.get_X()
        refused(da, B.update_weights, UNSUPPORTED, T["ranked"] + "dcora_exchange_update_weights")
        refused(da, lambda: B.set_weights(w0), UNSUPPORTED, T["ranked"] + "dcora_exchange_set_weights")
        assert np.array_equal(B.get_weights(), w0) and np.array_equal(B.get_X(), X)
        assert np.array_equal(ex.get_weights(), w0)
        # the exchange hands the session's own refusals through, the job as it was
        w = w0.copy()
        w[ZERO_EDGE] = 0.5
        refused(da, lambda: ex.set_weights(w), BAD_ARG, T["zero"])
        w[ZERO_EDGE], w[0] = 0.0, -1.0
        refused(da, lambda: ex.set_weights(w), BAD_ARG, T["weights"])
        assert np.array_equal(B.get_weights(), w0) and np.array_equal(ex.get_weights(), w0)
        assert np.array_equal(B.get_X(), X)
    finally:
        ex.close()
        B.close()
