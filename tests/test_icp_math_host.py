"""The cases of tests/icp_edge_util.py held to their purpose, on the oracle alone: each system, argument, twist and scene is in the lists because
it takes a path that no room or stress frame takes, and this module asserts that it does.  A case that misses its condition is changed, not
the condition (as with PROGRAMS in tests/op_program_util.py).  The device runs the same lists in tests/test_gpu_icp_math.py and
tests/test_gpu_tracking_edges.py."""
import numpy as np
import pytest

from oracle.binding import oracle_se3_exp, oracle_sincos, oracle_solve6
from tests import icp_edge_util as U


def test_every_column_fails_for_some_system_and_leaves_x_zero():
    vals, exact = U.solve_systems()
    x, col = U.oracle_solve_all(vals)
    assert 3000 > len(vals) > 800
    for i, j in exact:                          # built to give up at exactly this column (6: to go through)
        assert col[i] == j, (i, j, col[i])
    for j in range(6):
        hit = np.flatnonzero(col == j)
        assert len(hit) >= 24, (j, len(hit))
        assert (x[hit].view(np.uint32) == 0).all()          # +0, bit for bit
    ok = col == 6
    assert ok.sum() > 300 and np.isfinite(x[ok]).mean() > 0.9
    assert np.isnan(x[ok]).any()                # an inf below the pivots goes through the factorisation and comes out as NaN
    assert np.isnan(vals).any() and np.isinf(vals).any() and (vals == 0).all(axis=1).any()


def test_the_wrappers_agree_with_each_other():
    vals, _ = U.solve_systems()
    x, col = oracle_solve6(vals[0])
    assert x.dtype == np.float32 and x.shape == (6,) and 0 <= col <= 6
    T = oracle_se3_exp(np.zeros(6, np.float32))
    assert (T == np.eye(4, dtype=np.float32)).all()
    s, c = oracle_sincos(np.float32([0.0, -0.0]))
    assert (s.view(np.uint32) == 0).all() and (c == 1).all()      # sin(-0) = +0: r + (z * r) * poly = -0 + +0


def test_sine_arguments_cover_the_quadrants_and_the_twists_too():
    x = U.sincos_arguments()
    assert x.size <= 8_000_000
    assert (np.bincount(U.quadrant(x), minlength=4) > 100_000).all()
    neg = x < 0
    assert (np.bincount(U.quadrant(x[neg]), minlength=4) > 100_000).all()
    tsq, th = U.theta_of(U.twists())
    big = tsq >= U.EPS * U.EPS                     # the exponential calls the sine only there
    assert (np.bincount(U.quadrant(np.float32(0.5) * th[big]), minlength=4)[:3] > 10).all()
    assert (np.bincount(U.quadrant(th[big]), minlength=4) > 10).all()


def test_both_small_angle_tests_are_taken_on_either_side():
    tsq, th = U.theta_of(U.twists())
    eps = U.EPS
    ulps = np.abs(th.view(np.int32).astype(np.int64) - int(eps.view(np.int32)))
    near = (ulps <= 64) & (th > 0)
    for cond in (tsq < eps * eps, th < eps):
        assert (cond & near).sum() >= 20 and (~cond & near).sum() >= 20
    assert (tsq == 0).sum() >= 3


def test_finalize_cases_carry_their_twists_and_straddle_the_threshold():
    fc = U.finalize_cases()
    ref = U.finalize_reference(fc["partial"], fc["pose"], fc["thr"])
    tw = U.twists()
    n = fc["n_twists"]
    assert n == len(tw)
    assert (ref["col"][:n] == 6).all()
    assert (ref["x"][:n].view(np.uint32) == (tw + np.float32(0)).view(np.uint32)).all()      # C = I, b = twist: x = b (-0 becomes +0 in the sums)
    rest = slice(n, None)
    assert (ref["col"][rest] < 6).any() and (ref["col"][rest] == 6).sum() > 40
    assert (ref["conv"] == 1).sum() > 100 and (ref["conv"] == 0).sum() > 100
    # the same block and pose with icp_threshold = |x|, one ulp above and one ulp below: not converged, converged, not converged
    trip, norm = ref["conv"][fc["n_base"]:].reshape(-1, 3), ref["norm"][fc["n_base"]::3]
    assert (trip == [0, 1, 0]).all() and (norm > 0).sum() > 50
    assert (norm == 0).sum() >= 1          # |x| = 0: 0 < 0 is false, 0 < 1e-45 is true, 0 < -1e-45 is false
    nz_strips = (fc["partial"] != 0).any(axis=(2, 3)).sum(axis=1)
    nz_segments = (fc["partial"] != 0).any(axis=(1, 3)).sum(axis=1)
    assert {0, 1, 3, 8} <= set(nz_strips.tolist()) and {0, 1, 5, U.SEGMENTS} <= set(nz_segments.tolist())
    drift = np.abs(np.einsum("nij,nkj->nik", fc["pose"].reshape(-1, 4, 4)[:, :3, :3], fc["pose"].reshape(-1, 4, 4)[:, :3, :3]) - np.eye(3)).max(axis=(1, 2))
    assert (drift < 1e-5).sum() > 100 and (drift > 1e-4).sum() > 100       # rigid poses and poses that have drifted


def _ulp_distance(a, b):
    def key(v):
        i = (v + np.float32(0)).view(np.int32).astype(np.int64)         # (+ 0: -0 -> +0, the sign of zero is ignored)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def test_defined_sincos_is_within_one_ulp_of_libm_in_double():
    """The defined sine / cosine against np.sin / np.cos of the float64 argument, rounded to float, for |x| <= 64.  Bound, derived: there the
    double evaluation (two-part Cody-Waite reduction with |k| <= 41, the fdlibm kernels) errs by ~1e-16 relative, seven orders of magnitude below
    half a float ulp (6e-8), and so does libm's double result; two double values that close round to the same float or, when a rounding boundary
    lies between them, to neighbouring floats: 1 ulp at most.  Measured on these arguments: 0 ulp everywhere (sin(-0) = +0 aside)."""
    x = U.sincos_arguments()
    x = x[np.abs(x) <= 64]
    assert x.size > 3_000_000
    s, c = oracle_sincos(x)
    xd = x.astype(np.float64)
    ds, dc = _ulp_distance(s, np.sin(xd).astype(np.float32)), _ulp_distance(c, np.cos(xd).astype(np.float32))
    print(f"{x.size} arguments: sine differs on {(ds > 0).sum()}, cosine on {(dc > 0).sum()}; worst {ds.max()} / {dc.max()} ulp;",
          f"sign-of-zero mismatches {(np.signbit(s) != np.signbit(np.sin(xd))).sum()}")
    assert ds.max() <= 1 and dc.max() <= 1


# ---- the end-to-end cases of tests/test_gpu_tracking_edges.py, from the oracle's trace
def _theta(trace):
    return U.theta_of(trace["x"])[1]


def test_deep_pyramids_reach_the_inner_failure_the_quadrants_and_the_loss_of_every_inlier():
    S = U.deep_scene()
    runs = {p: S.track(p) for p in U.DEEP_PYRAMIDS}
    traces = [r[5] for r in runs.values()]
    for p, r in runs.items():
        assert len(r[5]) == r[4] <= sum(p)                  # one record per iteration that ran
        assert (r[5]["sums"][-1].view(np.uint32) == r[3].view(np.uint32)).all()
    cols = np.concatenate([t["fail_col"] for t in traces])
    assert ((cols >= 1) & (cols <= 5)).any()                # the solve gives up at an inner column
    theta = np.concatenate([_theta(t) for t in traces])
    assert (theta >= np.pi / 2).any() and (theta >= np.pi).any()
    assert {0, 1, 2} <= set(U.quadrant(theta).tolist())
    last = runs[(0, 0, 0, 0, 6)]
    assert last[5]["sums"][0, 28] > 0 and last[5]["sums"][-1, 28] == 0 and last[5]["fail_col"][-1] == 0 and not last[0]
    tiny = runs[(0, 0, 0, 0, 0, 3)]
    assert tiny[4] == 1 and 1 <= tiny[5]["fail_col"][0] <= 5 and (tiny[5]["x"] == 0).all() and not tiny[0]
    none = runs[(0, 0, 0, 0, 0, 0, 2)]
    assert none[4] == 1 and none[3][28] == 0 and not none[0]
    assert runs[(2, 2, 2, 2, 2, 2)][0]                      # recovers through all six levels
    assert (S.W >> 5, S.H >> 5) == (5, 3) and (S.W >> 6, S.H >> 6) == (2, 1)       # fewer rows than strips, fewer pixels than segments
    for p in set(U.GROWTH_ORDER):
        assert S.track(p)[0]
    assert len(U.GROWTH_ORDER[0]) < len(U.GROWTH_ORDER[1]) > len(U.GROWTH_ORDER[2])


def test_ragged_deep_pyramid_is_tracked_from_a_level_smaller_than_the_grid():
    S = U.ragged_scene()
    ok, _, _, red, it, tr = S.track(U.RAGGED_PYRAMID)
    top = len(U.RAGGED_PYRAMID) - 1
    assert (S.W >> top, S.H >> top) == (10, 6)
    assert ok and tr["level"][0] == top and tr["sums"][0, 28] > 0 and red[28] > 0.3 * S.W * S.H


def test_no_inlier_frames_run_one_iteration_per_level():
    S, G = U.deep_scene(), U.gate_scene()
    zero = S.track((10, 5, 4), depth=np.zeros_like(S.track_depth), key="zero-depth")
    far = G.track((10, 5, 4), start=U.far_pose(G), key="far")
    for ok, pose, _, red, it, tr in (zero, far):
        assert not ok and it == 3 and red[28] == 0 and (tr["fail_col"] == 0).all() and (tr["sums"][:, 28] == 0).all()
        assert tr["level"].tolist() == [2, 1, 0]
    assert zero[3][31] == S.W * S.H                          # every pixel without a normal
    assert (far[1].view(np.uint32) == U.far_pose(G).view(np.uint32)).all() and (far[3][29:] > 0).sum() >= 2


@pytest.mark.parametrize("shape", U.LARGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_large_images_are_accepted_and_take_several_trips(shape):
    S = U.large_scene(*shape)
    ok, _, _, red, it, tr = S.track((10, 5, 4))
    batch = 5 * U.LANES                                      # SE_TRACK_BATCH pixels per lane and trip
    seg = S.segment_length()
    assert seg == U.LARGE_SEGMENTS[shape]
    assert -(-seg // batch) == (3 if seg > 2 * batch else 2) and seg % batch != 0       # full trips and a partial last one
    assert ok and red[28] > 0.5 * S.W * S.H and it >= 10
