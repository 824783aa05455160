"""CPU side of tests/test_gpu_edge_configs.py: the camera-general room stream is the synthetic stream where their cameras agree, and every edge
configuration the GPU tests compare with the oracle is well posed there (no key-buffer truncation, no undefined out-of-volume read) and non-trivial
(a stated least number of blocks and raycast hits), so that no case can turn into a comparison of two empty maps unnoticed."""
import numpy as np
import pytest

from oracle.binding import OraclePipeline
from supereight_amd.synthetic import SyntheticStream, intrinsics, render_depth_mm
from tests.edge_frames import ALL_CASES, MAP_CASES, RoomStream, edge_stream, render_room_mm


@pytest.mark.parametrize("W,H,negative_fy", [(160, 120, False), (83, 61, False), (161, 97, True), (7, 5, False)])
def test_room_stream_is_the_synthetic_stream_at_its_camera(W, H, negative_fy):
    dim = 4.8
    k = intrinsics(W, negative_fy)
    a = SyntheticStream(W, H, dim, negative_fy=negative_fy)
    b = RoomStream(W, H, dim, k)
    assert (b.k.view(np.uint32) == a.k.view(np.uint32)).all()
    for f in range(3):
        mm = render_room_mm(f, W, H, dim, k)
        assert mm.dtype == np.uint16 and (mm == render_depth_mm(f, W, H, dim, negative_fy)).all()
        da, db = a.depth(f), b.depth(f)
        assert da.shape == db.shape == (H, W) and (da.view(np.uint32) == db.view(np.uint32)).all()
        assert (a.pose(f) == b.pose(f)).all()
    assert (da == 0).any() or W * H < 100            # the hole stream is there


def test_room_stream_follows_its_camera():
    """A different camera gives a different image of the same scene: the principal point shifts it, fx / fy scale it."""
    W, H, dim = 161, 97, 4.8
    base = render_room_mm(0, W, H, dim, (200.0, 200.0, 80.5, 48.5))
    shifted = render_room_mm(0, W, H, dim, (200.0, 200.0, 90.5, 48.5))
    assert (shifted[:, 10:] == base[:, :-10]).all() and not (shifted == base).all()
    flipped = render_room_mm(0, W, H, dim, (200.0, -200.0, 80.5, 48.5))
    assert (flipped == base[::-1]).all()
    mm = RoomStream(W, H, dim, (200.0, 200.0, 80.5, 48.5)).depth_mm(0)
    assert ((mm == 0) | (mm == base)).all() and 0 < (mm == 0).mean() < 0.05


@pytest.mark.parametrize("case", ALL_CASES, ids=[c["name"] for c in ALL_CASES])
def test_edge_case_is_well_posed_on_the_oracle(case):
    s = edge_stream(case)
    o = OraclePipeline(case["field"], case["N"], case["dim"], case["W"], case["H"])
    o.count_stats(True)
    hits = []
    try:
        for f in range(case["frames"]):
            pose = s.pose(f)
            o.integrate(s.depth(f), pose, s.k, case["mu"], f)
            ran, _, n = o.raycast(pose, s.k, case["mu"], f)
            if ran:
                hits.append(int((n[..., 0] != -2).sum()))
        if case in MAP_CASES:
            assert not hits
            _, _, n = o.raycast(pose, s.k, case["mu"], 100)
            hits.append(int((n[..., 0] != -2).sum()))
        st = o.stats()
        blocks = len(o.blocks()[0])
    finally:
        o.close()
    print(case["name"], "blocks", blocks, "hits", hits, st)
    assert st["truncated"] == 0 and st["oob_ub"] == 0, st
    assert blocks >= case["min_blocks"], blocks
    assert hits and min(hits) >= case["min_hits"], hits
