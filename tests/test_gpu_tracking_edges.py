"""Tracking at the edges of the reduction, end to end against the oracle: pyramid levels smaller than the reduction's grid (fewer than 8 rows:
strips without a row; fewer pixels than SE_TRACK_SEGMENTS: segments without a pixel), iterations whose solve gives up at an inner column or
whose update turns by more than pi, frames without a single inlier, pyramid buffers that grow after a first call, and images large enough for
a lane to take several trips of SE_TRACK_BATCH pixels.  The decision, the iteration count, the 32 sums, the pose and tracking_result_ are
compared bit for bit.  The scenes, the pyramids and the oracle's runs come from tests/icp_edge_util.py; tests/test_icp_math_host.py asserts
from the oracle's trace that they reach what they are listed for."""
import numpy as np
import pytest

from supereight_amd.pipeline import SDF, DenseSLAMPipeline
from tests import icp_edge_util as U

pytestmark = pytest.mark.gpu


def _replay(S):
    """The scene's map and last raycast on a fresh handle (frames at ground-truth poses, as Scene builds them on the oracle)."""
    gpu = DenseSLAMPipeline((S.W, S.H), S.N, S.dim, field_type=SDF)
    for f in range(S.frames):
        gpu.set_depth(S.depths[f]); gpu.setPose(S.poses[f])
        gpu.integration(S.k, 1, S.mu, f); gpu.raycasting(S.k, S.mu, f)
    v, n = gpu.vertex_normal()
    assert (v.view(np.uint32) == S.ref_vertex.view(np.uint32)).all() and (n.view(np.uint32) == S.ref_normal.view(np.uint32)).all()
    return gpu


def _track_and_compare(gpu, S, pyramid, depth=None, start=None, key=None):
    """One tracking() call (tracking does not touch the map; depth and start pose are set before each call) against the oracle's."""
    ok_c, pose_c, track_c, red_c, it_c, _ = S.track(pyramid, depth=depth, start=start, key=key)
    gpu.set_depth(S.track_depth if depth is None else depth)
    gpu.setPose(S.start_pose if start is None else start)
    ok_g = gpu.tracking(S.k, 1e-5, 1, S.frames, pyramid)
    track_g, red_g, it_g = gpu.track_data()
    pose_g = gpu.getPose()
    print(S.name, pyramid, key or "", "accepted", ok_c, "iterations", it_c, "inliers", red_c[28])
    assert (ok_g, it_g) == (ok_c, it_c) and it_c > 0
    assert U.same_bits(red_g, red_c).all(), (red_g, red_c)
    assert U.same_bits(pose_g, pose_c).all(), (pose_g, pose_c)
    lvl = next(i for i, n in enumerate(pyramid) if n > 0)              # tracking_result_ holds the finest level that ran (row stride = W)
    w, h = S.W >> lvl, S.H >> lvl
    assert (track_g["result"][:h, :w] == track_c["result"][:h, :w]).all()
    good = track_c["result"][:h, :w] == 1
    assert (track_g["error"][:h, :w][good].view(np.uint32) == track_c["error"][:h, :w][good].view(np.uint32)).all()
    assert (track_g["J"][:h, :w][good].view(np.uint32) == track_c["J"][:h, :w][good].view(np.uint32)).all()
    return ok_g, it_g, red_g, pose_g, track_g["result"][:h, :w].copy()


@pytest.fixture(scope="module")
def deep():
    gpu = _replay(U.deep_scene())
    yield gpu
    gpu.close()


@pytest.mark.parametrize("pyramid", U.DEEP_PYRAMIDS, ids=lambda p: "-".join(map(str, p)))
def test_deep_pyramids(deep, pyramid):
    """160x120 down to 10x7, 5x3 and 2x1: strips without a row and segments without a pixel, a solve that gives up at column 4, updates of
    1.9 and 3.6 rad, the loss of every inlier in the sixth iteration, and the recovery through all six levels."""
    _track_and_compare(deep, U.deep_scene(), pyramid)


def test_pyramid_buffers_grow_after_the_first_call():
    """3 levels, then 6, then 3 again on one handle: the buffers grow after a first call, and the smaller pyramid afterwards gives what it gives
    on a fresh handle."""
    S = U.deep_scene()
    fresh, grown = _replay(S), _replay(S)
    try:
        first = _track_and_compare(fresh, S, U.GROWTH_ORDER[2])
        for pyramid in U.GROWTH_ORDER:
            last = _track_and_compare(grown, S, pyramid)
        assert first[:2] == last[:2]
        for a, b in zip(first[2:], last[2:]):
            assert (a.view(np.uint32) == b.view(np.uint32)).all()
    finally:
        fresh.close(); grown.close()


def test_ragged_deep_pyramid():
    """163x101 with a general camera down to 10x6: every level ragged, the coarsest with two strips without a row and 10 pixels per strip."""
    S = U.ragged_scene()
    gpu = _replay(S)
    try:
        _track_and_compare(gpu, S, U.RAGGED_PYRAMID)
    finally:
        gpu.close()


def test_frame_without_depth(deep):
    """An all-zero depth image: no pixel has a normal; one iteration per level, the solve gives up at column 0, the entry pose comes back."""
    S = U.deep_scene()
    ok, it, red, pose, _ = _track_and_compare(deep, S, (10, 5, 4), depth=np.zeros_like(S.track_depth), key="zero-depth")
    assert not ok and it == 3 and red[28] == 0
    assert (pose.view(np.uint32) == S.start_pose.view(np.uint32)).all()


def test_frame_from_a_far_pose():
    """The far pose of test_tracking_gate_and_rejection in full: sums, iteration count and the restored pose, not only the decision."""
    S = U.gate_scene()
    far = U.far_pose(S)
    gpu = _replay(S)
    try:
        ok, it, red, pose, _ = _track_and_compare(gpu, S, (10, 5, 4), start=far, key="far")
        assert not ok and it == 3 and red[28] == 0
        assert (pose.view(np.uint32) == far.view(np.uint32)).all()
    finally:
        gpu.close()


@pytest.mark.parametrize("shape", U.LARGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_more_than_one_trip_of_the_batch_loop(shape):
    """Segments of 1302, 1875 and 2592 pixels: a lane's second and third trips of SE_TRACK_BATCH pixels (loads issued inside the loop instead
    of before the prologue) and the partial last trip."""
    S = U.large_scene(*shape)
    gpu = _replay(S)
    try:
        ok, *_ = _track_and_compare(gpu, S, (10, 5, 4))
        assert ok
    finally:
        gpu.close()
