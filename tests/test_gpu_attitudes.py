"""The two kernels that write the map -- the allocation scans (se_scan_sdf_wg, se_scan_ofusion_wg) and the sweep (k_integrate with
se_in_frustum and se_update_node_corner) -- against the oracle from the camera attitudes of tests/attitude_frames.py: along every axis with
exact zeros in R, rolled by right angles, generic, outside the volume, at surfaces outside it, looking out of it, on a block's min corner, and
all of them in turn on one map, so that most of it lies beside or behind the camera.  Bit for bit: block and node sets, every voxel, every
active flag, every node value after every frame, and every raycast that runs.  tests/test_attitude_frames_oracle.py shows on the oracle alone
that each case exercises what it is there for."""
import json

import numpy as np
import pytest

from oracle.binding import OraclePipeline
from supereight_amd.synthetic import intrinsics, to_colmajor
from tests.attitude_frames import (ATTITUDES, CORNER_ATTITUDES, DIM, FIELDS, SHAPES, TUMBLE, AttitudeStream, aniso_k, attitude_pose, block_key,
                                   corner_block, metres, render_scene_mm)
from tests.parity_util import compare_maps, compare_raycast, run_both

pytestmark = pytest.mark.gpu

SMALL, LARGE = list(SHAPES)
POOLS = {"dense": {SMALL: 0, LARGE: 0}, "pooled": {SMALL: 1 << 13, LARGE: 1 << 14}}      # (the tumble fuses 11 200 blocks at 256^3)


def _assert_same_map(cpu, gpu, what):
    m = compare_maps(cpu, gpu)
    assert m["same_block_set"] and m["same_node_set"], (what, m)
    assert m["x_mismatch"] == 0 and m["y_mismatch"] == 0 and m["active_mismatch"] == 0, (what, m)
    assert m["node_x_mismatch"] == 0 and m["node_y_mismatch"] == 0, (what, m)
    return m


def _assert_same_raycast(rec, voxel, what):
    r = compare_raycast(rec, voxel)
    assert r["hitmask_mismatch"] == 0 and r["vertex_bit_mismatch_px"] == 0 and r["normal_bit_mismatch_px"] == 0, (what, r)
    return r


@pytest.mark.parametrize("pool", ["dense", "pooled"])
@pytest.mark.parametrize("field_name", list(FIELDS))
@pytest.mark.parametrize("name", list(ATTITUDES))
def test_single_attitude(name, field_name, pool):
    """Two frames of one image and one pose on both sides, the whole map compared after each.  The corner cameras find the block on whose min
    corner they stand created beforehand; looking_out runs on a map that a +z frame filled, and must leave its block set as the oracle does."""
    from supereight_amd.pipeline import DenseSLAMPipeline
    W, H, N = SHAPES[SMALL]
    field, mu = FIELDS[field_name]
    k = intrinsics(W)
    cpu = OraclePipeline(field, N, DIM, W, H)
    gpu = DenseSLAMPipeline((W, H), N, DIM, field_type=field, max_blocks=1 << 13 if pool == "pooled" else 0)

    def fuse(pose_name, frame):
        T = attitude_pose(pose_name, DIM, N)
        depth = metres(render_scene_mm(T, W, H, DIM, k))
        gpu.set_depth(depth)
        gpu.setPose(T)
        assert gpu.integration(k, 1, mu, frame) and cpu.integrate(depth, T, k, mu, frame)
        return _assert_same_map(cpu, gpu, (pose_name, frame))

    try:
        first = 0
        if name in CORNER_ATTITUDES:
            c = corner_block(N)
            assert int(gpu.allocate(np.concatenate([c, c + 8])[None].astype(np.int32))[0]) == 1
            cpu.insert_octants(block_key(cpu.lib, c, N))
            m = _assert_same_map(cpu, gpu, "seeded")
            assert m["blocks_gpu"] == 1
        if name == "looking_out":
            filled = fuse("+z", 0)["blocks_gpu"]
            assert filled >= 50
            first = 1
        for f in (first, first + 1):
            m = fuse(name, f)
        print(name, field_name, pool, json.dumps(m))
        if name == "looking_out":
            assert m["blocks_gpu"] == filled
        else:
            assert m["blocks_gpu"] >= 50
    finally:
        cpu.close(); gpu.close()


TUMBLE_RUNS = [(s, f, p, False) for s in SHAPES for f in FIELDS for p in POOLS] + [(LARGE, "sdf", "dense", True), (SMALL, "ofusion", "pooled", True)]


@pytest.mark.parametrize("shape,field_name,pool,aniso", TUMBLE_RUNS, ids=[f"{s}-{f}-{p}{'-aniso' if a else ''}" for s, f, p, a in TUMBLE_RUNS])
def test_tumble(shape, field_name, pool, aniso):
    """TUMBLE frame by frame on one map: the same map comparison after every frame, and every raycast that runs."""
    W, H, N = SHAPES[shape]
    field, mu = FIELDS[field_name]
    stream = AttitudeStream(W, H, N, k=aniso_k(W) if aniso else None)
    seen = []

    def on_frame(f, cpu, gpu, rec):
        m = _assert_same_map(cpu, gpu, (f, stream.names[f]))
        seen.append((m["blocks_gpu"], int(cpu.blocks()[3].sum())))
        if rec["raycast"]:
            rec["cmp"] = _assert_same_raycast(rec, DIM / N, (f, stream.names[f]))

    cpu, gpu, recs = run_both(field, W, H, N, DIM, mu, len(stream), max_blocks=POOLS[pool][shape], on_frame=on_frame, stream=stream)
    try:
        hits = [r["cmp"]["hits_gpu"] for r in recs if r["raycast"]]
        print(shape, field_name, pool, "blocks, active per frame", seen, "hits", hits)
        assert len(hits) == len(TUMBLE) - 3 and sum(h >= 50 for h in hits) * 2 >= len(hits)
        assert seen[-1][0] > 1000 and min(a / b for b, a in seen) < 0.5          # most of the map out of view at some point
        assert cpu.stats()["truncated"] == 0
    finally:
        cpu.close(); gpu.close()


@pytest.mark.parametrize("field_name", list(FIELDS))
def test_tumble_swept_counts(field_name):
    """How many blocks the sweep takes, per frame: the only observable of a block that is swept -- because it was active, or because its min
    corner projects into the image, through a negative z too (se_in_frustum, filter.hpp:38-49) -- and holds nothing visible.  `probes` is
    defined alike on both sides, one count per band step inside the volume (se_oracle.cpp buildAllocationList / buildOctantList, se_kernels.h
    se_scan_sdf_wg / se_scan_ofusion_wg), so it is compared per frame as well.  A handle that counts takes other kernel instantiations and
    never fuses, hence a test of its own."""
    from supereight_amd.pipeline import DenseSLAMPipeline
    W, H, N = SHAPES[SMALL]
    field, mu = FIELDS[field_name]
    stream = AttitudeStream(W, H, N)
    cpu = OraclePipeline(field, N, DIM, W, H)
    gpu = DenseSLAMPipeline((W, H), N, DIM, field_type=field)
    cpu.count_stats(True)
    gpu.enable_stats(True)
    swept, probes, blocks = [], [], []
    try:
        probes_before = 0
        for f in range(len(stream)):
            depth, T = stream.depth(f), stream.pose(f)
            gpu.set_depth(depth)
            gpu.setPose(T)
            assert gpu.integration(stream.k, 1, mu, f) and cpu.integrate(depth, T, stream.k, mu, f)
            g, c = gpu.stats(reset=True), cpu.stats()
            swept.append((g["swept"], c["swept"]))
            probes.append((g["probes"], c["probes"] - probes_before))
            probes_before = c["probes"]
            blocks.append(cpu.counts()[0])
        print(field_name, "swept (device, oracle)", swept, "probes", probes, "blocks", blocks)
        assert all(g == c for g, c in swept), swept
        assert all(g == c for g, c in probes), probes
        assert any(0 < c < b for (_, c), b in zip(swept, blocks))
        _assert_same_map(cpu, gpu, "end")
    finally:
        cpu.close(); gpu.close()


@pytest.mark.parametrize("streaming", [False, True], ids=["two-queue", "one-queue"])
@pytest.mark.parametrize("field_name", list(FIELDS))
def test_tumble_streamed(field_name, streaming):
    """The tumble as bench.py feeds frames: device-resident images, frame() calls back to back without synchronisation, so that each frame's
    scan runs beside or inside the previous frame's raycast -- from a pose that has nothing to do with it.  Final map and last raycast."""
    import torch
    from supereight_amd.pipeline import DenseSLAMPipeline
    W, H, N = SHAPES[LARGE]
    field, mu = FIELDS[field_name]
    stream = AttitudeStream(W, H, N)
    frames = len(stream)
    depths = [stream.depth(f) for f in range(frames)]
    poses = [stream.pose(f) for f in range(frames)]
    dev = torch.from_numpy(np.stack(depths)).cuda()
    gpu = DenseSLAMPipeline((W, H), N, DIM, field_type=field, streaming=streaming)
    cpu = OraclePipeline(field, N, DIM, W, H)
    try:
        assert gpu.scan_overlaps() and gpu.frame_is_fused() == streaming
        for f in range(frames):
            assert gpu.frame(dev[f].data_ptr(), to_colmajor(poses[f]), stream.k, mu, f) == (3 if f > 2 else 1)
        # the rule of test_pipelined_stream_parity: the raycasts of frames 3 .. frames - 2 each ride in the next frame's scan launch
        # (frame_can_fuse holds for every frame here: a plain handle without stats, 20 x 15 raycast tiles)
        assert gpu.launch_counts()["fused"] == (frames - 4 if streaming else 0)
        for f in range(frames):
            cpu.integrate(depths[f], poses[f], stream.k, mu, f)
            _, v_c, n_c = cpu.raycast(poses[f], stream.k, mu, f)
        m = _assert_same_map(cpu, gpu, "end")
        assert m["blocks_gpu"] > 5000
        v_g, n_g = gpu.vertex_normal()
        r = _assert_same_raycast({"v_c": v_c, "n_c": n_c, "v_g": v_g, "n_g": n_g}, DIM / N, "last")
        assert r["hits_gpu"] > 1000, r
    finally:
        cpu.close(); gpu.close()


@pytest.mark.parametrize("field_name", list(FIELDS))
def test_fast_and_ieee_sweeps_agree_on_the_tumble(field_name, monkeypatch):
    """test_gpu_sweep_arith.py's end-to-end case away from the +z half-space: k_integrate<FAST> (shared refined reciprocal, products by zero
    dropped) and the compiler's own divisions (SE_HIP_IEEE_SWEEP=1) give byte-identical blocks and nodes on the tumble."""
    import torch
    from supereight_amd.pipeline import DenseSLAMPipeline
    W, H, N = SHAPES[LARGE]
    field, mu = FIELDS[field_name]
    stream = AttitudeStream(W, H, N)
    frames = len(stream)
    dev = torch.from_numpy(np.stack([stream.depth(f) for f in range(frames)])).cuda()

    def run(ieee):
        if ieee:
            monkeypatch.setenv("SE_HIP_IEEE_SWEEP", "1")
        else:
            monkeypatch.delenv("SE_HIP_IEEE_SWEEP", raising=False)
        p = DenseSLAMPipeline((W, H), N, DIM, field_type=field)      # (the knob is read once, here)
        for f in range(frames):
            p.frame(dev[f].data_ptr(), to_colmajor(stream.pose(f)), stream.k, mu, f)
        out = p.blocks() + p.nodes()
        p.close()
        return out

    a, b = run(False), run(True)
    assert len(a[0]) > 5000
    for u, v in zip(a, b):
        assert u.shape == v.shape and (u.view(np.uint8) == v.view(np.uint8)).all()
