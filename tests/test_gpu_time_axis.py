"""The frame number on the device against the oracle, bit for bit: OFusion's timestamp (1.f / 30.f) * frame through se_bfusion_apply /
se_bfusion_apply_nb (dt >= 4: the max(0.5, .) clamp; dt == 0: the plateaus beyond 2^24 frames and at the top of uint32; dt < 0 and the pole
dt = -4 on a schedule that runs backwards), the gates frame % rate == 0 || frame <= 3 and frame > 2 with real depth on every frame, and the
image-ring slot frame % slots.  The room stream at 160x120 into 128^3 supplies depth and pose by stream index; the frame number comes from
the schedules of tests/time_axis_util.py, whose oracle runs are computed once and shared (tests/test_oracle_time_and_setter.py asserts on
the oracle alone that every regime is entered).  After EVERY frame of the eager calls: block and node sets, x, y, node x and y, active
flags, the return values and both raycast images.  frame() on a streaming handle: every slot of the ring, the return values, the launch
counters and the final map."""
import numpy as np
import pytest

from supereight_amd.pipeline import OFUSION, SDF, DenseSLAMPipeline
from supereight_amd.synthetic import to_colmajor
from tests import time_axis_util as T
from tests.time_axis_util import DIM, H, MU, N, W

pytestmark = pytest.mark.gpu
POOL = 2048
SDF_SCHEDULES = ("gapped", "top_2p32", "rate3", "rate7")         # (SDF: only the gates and the slot depend on the frame number)
CASES = ([(OFUSION, name, mb) for name in T.SCHEDULES for mb in (0, POOL)] + [(SDF, name, mb) for name in SDF_SCHEDULES for mb in (0, POOL)])
IDS = [f"{'sdf' if f == SDF else 'ofusion'}_{name}_{'pooled' if mb else 'dense'}" for f, name, mb in CASES]


@pytest.mark.parametrize("field,name,max_blocks", CASES, ids=IDS)
def test_eager_calls_follow_the_oracle_after_every_frame(field, name, max_blocks):
    recs, _ = T.oracle_schedule(field, name)
    frames, rate = T.SCHEDULES[name]
    k, depths, poses = T.stream_frames()
    gpu = DenseSLAMPipeline((W, H), N, DIM, field_type=field, max_blocks=max_blocks)
    try:
        for i, (f, r) in enumerate(zip(frames, recs)):
            gpu.set_depth(depths[i])
            gpu.setPose(poses[i])
            assert gpu.integration(k, rate, MU[field], f) == r["ran_i"], f
            assert gpu.raycasting(k, MU[field], f) == r["ran_r"], f
            T.assert_same_state(r["state"], gpu, (name, f))
            if r["ran_r"]:
                v, n = gpu.vertex_normal()
                T.assert_same_images(r["v"], r["n"], v, n, (name, f))
    finally:
        gpu.close()


@pytest.mark.parametrize("field,name,max_blocks", CASES, ids=IDS)
def test_streamed_frames_fill_their_ring_slots(field, name, max_blocks):
    """se_hip_frame back to back on a streaming handle, nothing else called in between: the raycast of frame f is held back and runs in the
    launch that scans the next integrating frame (counted), or alone where the next frame does not integrate; its images go to slot
    f % slots, and the ring is sized so that the schedule's frames fall into distinct slots."""
    import torch
    recs, _ = T.oracle_schedule(field, name)
    frames, rate = T.SCHEDULES[name]
    k, depths, poses = T.stream_frames()
    slots = T.ring_slots(frames)
    assert len({f % slots for f in frames}) == len(frames)
    dev = torch.from_numpy(np.stack(depths[:len(frames)])).cuda()
    pcm = [to_colmajor(q) for q in poses]
    gpu = DenseSLAMPipeline((W, H), N, DIM, field_type=field, max_blocks=max_blocks, streaming=True)
    try:
        ring = torch.zeros((slots, 2, H, W, 3), dtype=torch.float32, device="cuda")
        gpu.set_image_ring(ring.data_ptr(), slots, keepalive=ring)
        assert gpu.frame_is_fused()
        gpu.launch_counts(reset=True)
        for i, (f, r) in enumerate(zip(frames, recs)):
            assert gpu.frame(dev[i].data_ptr(), pcm[i], k, MU[field], f, rate) == (1 if r["ran_i"] else 0) | (2 if r["ran_r"] else 0), f
        ran_i, ran_r = [r["ran_i"] for r in recs], [r["ran_r"] for r in recs]
        fused = sum(1 for i in range(len(recs) - 1) if ran_r[i] and ran_i[i + 1])
        if rate == 1:
            assert fused == sum(ran_r) - 1 and fused >= 5
        n = gpu.launch_counts()
        print(name, n)
        assert n["pending"] and n["fused"] == fused and n["raycast"] == sum(ran_r) - 1, n          # the last raycast is still held back
        assert n["integrate"] == sum(ran_i) and n["alloc_scan"] == sum(ran_i), n
        gpu.sync()
        n = gpu.launch_counts()
        assert not n["pending"] and n["raycast"] == sum(ran_r) and n["fused"] == fused, n
        out = ring.cpu().numpy()
        used = set()
        for f, r in zip(frames, recs):
            s = f % slots
            used.add(s)
            if r["ran_r"]:
                T.assert_same_images(r["v"], r["n"], out[s, 0], out[s, 1], (name, f, s))
            else:
                assert not out[s].any(), (f, s)
        for s in set(range(slots)) - used:
            assert not out[s].any(), s
        T.assert_same_state(recs[-1]["state"], gpu, (name, "end"))
    finally:
        gpu.close()
