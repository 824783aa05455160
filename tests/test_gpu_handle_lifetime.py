"""The lifetime of a handle: everything it creates lazily (the pinned input ring, the tracker's pyramids and records, the render target, the
mesh counters, the staging buffer, the edit event, the timing event pool, borrowed streams) is created once and released by close(), the
caller's streams are left alone, and nothing is lost per create / close cycle (se_host_resources.h: every resource has one owner)."""
import numpy as np
import pytest
import torch

from supereight_amd.pipeline import OFUSION, SDF, DenseSLAMPipeline
from supereight_amd.synthetic import make_stream
from tests.gpu_state_util import H, W, map_state

pytestmark = pytest.mark.gpu

N, DIM = 64, 4.8          # the smallest volume se_hip_create accepts
FIRST = 3                 # frame number of the first of the three frames: raycasting() runs from frame 3 on (DenseSLAMSystem.cpp:195)


def _frames(kind="room"):
    s = make_stream(kind, W, H, DIM, holes=False)
    return s.k, [(s.depth(f), s.pose(f)) for f in range(3)]


def _frame(p, k, mu, depth, pose, frame):
    p.set_depth(depth)                      # (host depth: the pinned input ring)
    p.setPose(pose)
    assert p.integration(k, 1, mu, frame)
    assert p.raycasting(k, mu, frame)


def _three_frames(field, max_blocks, mu, k, frames):
    p = DenseSLAMPipeline((W, H), N, DIM, field_type=field, max_blocks=max_blocks)
    for i, (d, T) in enumerate(frames):
        _frame(p, k, mu, d, T, FIRST + i)
    return p


@pytest.mark.parametrize("field,max_blocks,mu", [(SDF, 0, 0.1), (OFUSION, 1024, 0.02)], ids=["sdf_dense", "ofusion_pooled"])
def test_every_lazy_resource_then_close(field, max_blocks, mu, monkeypatch):
    monkeypatch.setenv("SE_HIP_SHIFT_KEEP_MIB", "0")      # (read by se_hip_create: the shift gives its staging buffer back when it returns)
    k, frames = _frames()
    plain = _three_frames(field, max_blocks, mu, k, frames)
    try:
        assert ("pooled" in plain.memory_info()["layout"]) == bool(max_blocks)
        want = map_state(plain)
        assert len(want[0]) > 0 and (want[8] != 0).any()     # blocks were allocated, the raycast hit something
    finally:
        plain.close()

    scan_stream, main_stream = torch.cuda.Stream(), torch.cuda.Stream()
    p = _three_frames(field, max_blocks, mu, k, frames)
    try:
        p.tracking(k, 1e-5, 1, FIRST + 2)                    # pyramids, track data, ICP state and its pinned record
        assert p.track_data()[0].shape == (H, W)
        assert p.renderVolume(frames[2][1], k, mu, 0.75 * mu) is not None
        assert len(p.mesh()) > 0
        mb = p.mesh_blocks()
        assert len(mb["coords"]) > 0 and len(mb["triangles"]) > 0
        q = p.query(np.array([[DIM / 2, DIM / 2, DIM / 2], [0.1, 0.2, 0.3]], np.float32))
        assert q["status"].shape == (2,)
        x_in = 0.5 if field == SDF else -1.0
        counts = p.edit(np.array([[0, 0, 0, N, N, N]], np.int32), x=x_in)      # (the edit event)
        assert counts[0] > 0 and counts[3] == 0
        staged = p.memory_info()["device_bytes"]
        kept = p.shift([8, 0, 0])
        assert kept[0] > 0
        assert p.memory_info()["device_bytes"] < staged      # the staging buffer (it held the queries' and the mesh's outputs) was released on return
        p.enable_timing(True)
        _frame(p, k, mu, *frames[2], FIRST + 3)
        t = p.timings()
        assert t["integrate"]["launches"] == 1 and t["raycast"]["launches"] == 1 and t["raycast"]["ms_sum"] > 0
        p.enable_timing(False)
        p.set_scan_stream(scan_stream.cuda_stream)
        _frame(p, k, mu, *frames[2], FIRST + 4)
        p.set_scan_stream(0)                                 # back to a scan stream of the handle's own
        _frame(p, k, mu, *frames[2], FIRST + 5)
        p.set_stream(main_stream.cuda_stream)
        _frame(p, k, mu, *frames[2], FIRST + 6)
        p.sync()
    finally:
        p.close()
    p.close()                                                # a second close() is a no-op
    for s in (scan_stream, main_stream):                     # the borrowed streams are the caller's still
        with torch.cuda.stream(s):
            y = torch.arange(1024, device="cuda:0", dtype=torch.float32) * 2
        s.synchronize()
        assert float(y.sum()) == 1023 * 1024

    fresh = _three_frames(field, max_blocks, mu, k, frames)
    try:
        got = map_state(fresh)
        assert len(got) == len(want) and all(u.shape == w.shape and (u == w).all() for u, w in zip(got, want))
    finally:
        fresh.close()


def test_no_loss_per_create_close_cycle():
    """Six create / three frames / close cycles of a 256^3 dense SDF handle (a brick grid of 128 MiB).  The card may be shared, so the free
    memory after each close is judged by its trend: of the five consecutive differences at least one loses less than half a grid.  A grid
    that is not released loses 128 MiB in every cycle; a neighbour's allocation disturbs single cycles."""
    n, dim, mu = 256, 4.8, 0.1
    s = make_stream("room", W, H, dim, holes=False)
    frames = [(s.depth(f), s.pose(f)) for f in range(3)]
    free = []
    for _ in range(6):
        p = DenseSLAMPipeline((W, H), n, dim, field_type=SDF)
        try:
            info = p.memory_info()
            assert info["layout"] == "dense brick grid" and info["brick_bytes"] == 128 << 20
            for i, (d, T) in enumerate(frames):
                _frame(p, s.k, mu, d, T, FIRST + i)
            p.sync()
        finally:
            p.close()
        free.append(torch.cuda.mem_get_info()[0])
    lost = [a - b for a, b in zip(free, free[1:])]
    assert min(lost) < 64 << 20, f"free device memory fell by {[round(v / 2**20, 1) for v in lost]} MiB over five consecutive cycles"
