"""Oracle parity, bit for bit, at the configurations the other parity tests leave out (the case table: tests/edge_frames.py, held to be
well posed and non-trivial by tests/test_edge_configs_oracle.py):
  * image shapes that are not whole 8x8 tiles -- partial last tile columns and rows, an odd tile count (the raycast's last workgroup then has a
    wave with no tile), images narrower or shorter than one tile, an image with more raycast workgroups than one round of the chip;
  * cameras other than synthetic.intrinsics(W): fx != fy, principal points off centre, negative fy, a wide and a narrow lens;
  * the ends of the volume resolutions se_hip_create accepts, 64^3 and 4096^3.
Each shape / camera case runs three schedules: eager from host depth (the allocation scan maps 64-pixel row pieces), the one-queue stream from
device depth (8x8 tiles; every frame's images in a ring) and, for a subset, pooled bricks.  Then mesh() and query() at 64^3 and 4096^3, and the
consumers of the images -- renderDepth / renderVolume / renderTrack, tracking on an odd-sized pyramid, the subsampling millimetre upload -- at a
ragged shape with a general camera."""
import json
import time

import numpy as np
import pytest

from oracle.binding import SDF, OFUSION, OraclePipeline, load, oracle_half_sample, oracle_tracking
from supereight_amd.pipeline import DenseSLAMPipeline
from tests.edge_frames import CONSUMER, MAP_CASES, RES_CASES, SHAPE_CASES, RoomStream, edge_stream
from tests.parity_util import compare_maps, compare_raycast, run_both
from tests.test_gpu_map_query import _compare, _Map
from tests.test_gpu_stress_parity import _pipelined_case

pytestmark = pytest.mark.gpu

CASES = SHAPE_CASES + RES_CASES
POOLED = [c for c in CASES if c["pooled"]]


def _ids(cases):
    return [c["name"] for c in cases]


def _assert_same_map(cpu, gpu):
    m = compare_maps(cpu, gpu)
    assert m["same_block_set"] and m["same_node_set"], m
    assert m["x_mismatch"] == 0 and m["y_mismatch"] == 0 and m["active_mismatch"] == 0, m
    assert m["node_x_mismatch"] == 0 and m["node_y_mismatch"] == 0, m
    return m


def _assert_same_images(rec, voxel, what):
    r = compare_raycast(rec, voxel)
    assert r["hitmask_mismatch"] == 0 and r["vertex_bit_mismatch_px"] == 0 and r["normal_bit_mismatch_px"] == 0, (what, r)
    return r["hits_gpu"]


def _eager(case, max_blocks):
    t0 = time.time()
    cpu, gpu, recs = run_both(case["field"], case["W"], case["H"], case["N"], case["dim"], case["mu"], case["frames"], max_blocks=max_blocks,
                              stream=edge_stream(case))
    try:
        st = cpu.stats()
        assert st["truncated"] == 0 and st["oob_ub"] == 0, st
        assert gpu.memory_info()["layout"] == ("pooled bricks" if max_blocks else "dense brick grid")
        m = _assert_same_map(cpu, gpu)
        assert m["blocks_gpu"] >= case["min_blocks"], m
        hits = [_assert_same_images(rec, case["dim"] / case["N"], (case["name"], rec["frame"])) for rec in recs if rec["raycast"]]
        assert len(hits) == case["frames"] - 3 and min(hits) >= case["min_hits"], hits
        print(case["name"], "max_blocks", max_blocks, "blocks", m["blocks_gpu"], "hits", hits, f"{time.time() - t0:.1f} s")
    finally:
        cpu.close(); gpu.close()


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_eager_from_host_depth(case):
    """set_depth from host memory, integration, raycasting: the map and every frame's raycast.  4096^3 runs on its pooled map only (the dense
    brick grid of 4096^3 is 2^27 bricks)."""
    _eager(case, case["pooled"] if case["N"] == 4096 else 0)


@pytest.mark.parametrize("case", [c for c in POOLED if c["N"] != 4096], ids=_ids([c for c in POOLED if c["N"] != 4096]))
def test_eager_pooled(case):
    _eager(case, case["pooled"])


def _fuses(W, H):
    """Whether a one-queue handle of this image fuses its raycast into the next frame's scan: only while the raycast's workgroups (two 8x8 tiles
    each) fit the chip in one round, ten per compute unit (se_hip_api.hip, frame_can_fuse)."""
    import torch
    pairs = (((W + 7) // 8) * ((H + 7) // 8) + 1) // 2
    return pairs <= 10 * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_one_queue_stream_from_device_depth(case):
    """se_hip_frame from device-resident depth back to back on a streaming handle, every frame's images in a ring and compared (the pooled cases
    once more with the serial pooled schedule).  Fused launches asserted through the launch counters wherever the shape fuses."""
    t0 = time.time()
    fuses = _fuses(case["W"], case["H"])
    if case["name"].startswith("large_"):
        print(case["name"], "fuses" if fuses else "does not fuse (more raycast workgroups than one round)")
    _pipelined_case(None, case["W"], case["H"], case["field"], case["N"], case["mu"], case["frames"], case["pooled"] if case["N"] == 4096 else 0, True,
                    min_hits_per_frame=case["min_hits"] - 1, stream=edge_stream(case), fuses=fuses)
    print(case["name"], f"one-queue {time.time() - t0:.1f} s")


@pytest.mark.parametrize("case", [c for c in POOLED if c["N"] != 4096], ids=_ids([c for c in POOLED if c["N"] != 4096]))
def test_one_queue_stream_pooled(case):
    _pipelined_case(None, case["W"], case["H"], case["field"], case["N"], case["mu"], case["frames"], case["pooled"], True,
                    min_hits_per_frame=case["min_hits"] - 1, stream=edge_stream(case), fuses=_fuses(case["W"], case["H"]))


def _canon(m):
    b = np.ascontiguousarray(m.reshape(-1, 9)).view(np.uint32)
    return b[np.lexsort(b.T[::-1])]


MAP_RUNS = [(c, mb) for c in MAP_CASES for mb in ((0, 1 << 14) if c["N"] == 64 else (1 << 14,))]


@pytest.mark.parametrize("case,max_blocks", MAP_RUNS, ids=[c["name"] + ("_pooled" if mb else "_dense") for c, mb in MAP_RUNS])
def test_mesh_and_query_at_the_resolution_extremes(oracle, case, max_blocks):
    """mesh() against the oracle's marching cubes (the same triangles, bit for bit), and query() against the oracle's octree built from the
    device map (as tests/test_gpu_map_query.py does at 256^3), at 64^3 (dense and pooled) and 4096^3 (pooled)."""
    W, H, N, dim, mu, field = case["W"], case["H"], case["N"], case["dim"], case["mu"], case["field"]
    s = edge_stream(case)
    cpu = OraclePipeline(field, N, dim, W, H)
    gpu = DenseSLAMPipeline((W, H), N, dim, field_type=field, max_blocks=max_blocks)
    m = None
    try:
        for f in range(case["frames"]):
            depth, pose = s.depth(f), s.pose(f)
            cpu.integrate(depth, pose, s.k, mu, f)
            gpu.set_depth(depth); gpu.setPose(pose); gpu.integration(s.k, 1, mu, f)
        assert gpu.raycasting(s.k, mu, 100)
        _, v_c, n_c = cpu.raycast(pose, s.k, mu, 100)
        v_g, n_g = gpu.vertex_normal()
        assert _assert_same_images({"v_c": v_c, "n_c": n_c, "v_g": v_g, "n_g": n_g}, dim / N, case["name"]) >= case["min_hits"]
        mm = _assert_same_map(cpu, gpu)
        mo, mg = cpu.mesh(), gpu.mesh()
        assert mo.shape == mg.shape and mo.shape[0] > 200, (mo.shape, mg.shape)
        assert (_canon(mo) == _canon(mg)).all()
        m = _Map(oracle, gpu, field, n=N, dim=dim)
        pts = m.points(gpu, np.random.default_rng(23 + field))
        got = gpu.query(pts, fine=True, coarse=True, interp=True, grad=True, status=True)
        _compare(got, m.expected(pts))
        st = got["status"]
        for bit in (1, 2, 4):
            assert ((st & bit) != 0).any() and ((st & bit) == 0).any(), bit
        assert np.unique(got["interp"]).size > 50 and np.abs(got["grad"]).max() > 0
        print(case["name"], "max_blocks", max_blocks, "blocks", mm["blocks_gpu"], "triangles", mg.shape[0], "points", len(pts))
    finally:
        if m is not None:
            m.close()
        cpu.close(); gpu.close()


def _consumer_stream(holes=True):
    c = CONSUMER
    return RoomStream(c["W"], c["H"], c["dim"], c["k"], holes=holes)


@pytest.mark.parametrize("field,mu", [(SDF, 0.1), (OFUSION, 0.02)], ids=["sdf", "ofusion"])
def test_render_kernels_at_a_ragged_shape(field, mu):
    """renderDepth, renderVolume (from the raycast pose: shades the cached images; from another pose: re-raycasts through k_render_volume's own
    tiling) and renderTrack at 163x101 (21 x 13 tiles) with fx != fy and an off-centre principal point, byte for byte as test_gpu_render.py."""
    W, H, N, dim, frames = CONSUMER["W"], CONSUMER["H"], CONSUMER["N"], CONSUMER["dim"], 6
    lib = load()
    s = _consumer_stream()
    cpu = OraclePipeline(field, N, dim, W, H)
    gpu = DenseSLAMPipeline((W, H), N, dim, field_type=field)
    try:
        for f in range(frames):
            depth, pose = s.depth(f), s.pose(f)
            gpu.set_depth(depth); gpu.setPose(pose)
            cpu.integrate(depth, pose, s.k, mu, f); gpu.integration(s.k, 1, mu, f)
            ran, v, n = cpu.raycast(pose, s.k, mu, f); gpu.raycasting(s.k, mu, f)
        v_g, n_g = gpu.vertex_normal()
        assert _assert_same_images({"v_c": v, "n_c": n, "v_g": v_g, "n_g": n_g}, dim / N, "raycast") > 0.6 * W * H
        ref = np.zeros((H, W, 4), np.uint8)
        lib.so_render_depth(ref.reshape(-1), np.ascontiguousarray(depth, np.float32).reshape(-1), W, H)
        assert (gpu.renderDepth() == ref).all() and len(np.unique(ref.reshape(-1, 4), axis=0)) > 50
        largestep = 0.75 * mu
        a = gpu.renderVolume(pose, s.k, mu, largestep)
        b = cpu.render_volume(pose, pose, s.k, mu, largestep, v, n)
        assert (a == b).all() and (a[..., 0] > 0).mean() > 0.6
        for view in (s.pose(frames + 20), s.pose(frames + 60)):
            a = gpu.renderVolume(view, s.k, mu, largestep)
            b = cpu.render_volume(view, pose, s.k, mu, largestep, v, n)
            assert (a == b).all() and (a[..., 0] > 0).mean() > 0.5
        d2 = s.depth(frames)
        gpu.set_depth(d2)
        ok_g = gpu.tracking(s.k, 1e-5, 1, frames)
        ok_c, _, track_c, _, _ = oracle_tracking(d2, s.k, pose, pose, v, n)
        ref = np.zeros((H, W, 4), np.uint8)
        lib.so_render_track(ref.reshape(-1), track_c.ctypes.data, W, H)
        assert ok_g == ok_c and (gpu.renderTrack() == ref).all() and len(np.unique(ref.reshape(-1, 4), axis=0)) > 1
    finally:
        cpu.close(); gpu.close()


def test_tracking_at_a_ragged_shape():
    """Two tracked frames with a 3-level pyramid whose levels are all odd-sized or ragged (163x101 -> 81x50 -> 40x25) and a general camera: the
    pyramid, the decision, the iteration count, the TrackData, the 32 reduction sums and the pose, bit for bit (as test_slam_loop_with_tracking)."""
    W, H, N, dim, mu, frames = CONSUMER["W"], CONSUMER["H"], CONSUMER["N"], CONSUMER["dim"], 0.1, 6
    s = _consumer_stream()
    cpu = OraclePipeline(SDF, N, dim, W, H)
    gpu = DenseSLAMPipeline((W, H), N, dim, field_type=SDF)
    try:
        pose_c = s.pose(0).copy()
        gpu.setPose(pose_c)
        v_c = n_c = rp_c = None
        for f in range(frames):
            depth = s.depth(f)
            gpu.set_depth(depth)
            if f >= 4:
                ok_c, pose_c, track_c, red_c, it_c = oracle_tracking(depth, s.k, pose_c, rp_c, v_c, n_c, 1e-5, (10, 5, 4))
                ok_g = gpu.tracking(s.k, 1e-5, 1, f, (10, 5, 4))
                l1, l2 = gpu.scaled_depth(1), gpu.scaled_depth(2)
                h1 = oracle_half_sample(depth, 0.1 * 3, 1)
                h2 = oracle_half_sample(h1, 0.1 * 3, 1)
                assert l1.shape == h1.shape == (50, 81) and l2.shape == h2.shape == (25, 40)
                assert (l1.view(np.uint32) == h1.view(np.uint32)).all() and (l2.view(np.uint32) == h2.view(np.uint32)).all()
                track_g, red_g, it_g = gpu.track_data()
                print("frame", f, "accepted", ok_c, "iterations", it_c, "inliers", red_c[28])
                assert ok_g == ok_c and it_g == it_c, (ok_g, ok_c, it_g, it_c)
                assert (track_g["result"] == track_c["result"]).all()
                good = track_c["result"] == 1
                assert (track_g["error"][good].view(np.uint32) == track_c["error"][good].view(np.uint32)).all()
                assert (track_g["J"][good].view(np.uint32) == track_c["J"][good].view(np.uint32)).all()
                assert (red_g.view(np.uint32) == red_c.view(np.uint32)).all(), (red_g, red_c)
                assert (gpu.getPose().view(np.uint32) == pose_c.view(np.uint32)).all()
                assert ok_c and red_c[28] > 0.5 * W * H
            else:
                pose_c = s.pose(f).copy()
                gpu.setPose(pose_c)
            cpu.integrate(depth, pose_c, s.k, mu, f)
            gpu.integration(s.k, 1, mu, f)
            ran, vv, nn = cpu.raycast(pose_c, s.k, mu, f)
            gpu.raycasting(s.k, mu, f)
            if ran:
                v_c, n_c, rp_c = vv, nn, pose_c.copy()
                v_g, n_g = gpu.vertex_normal()
                assert (v_g.view(np.uint32) == v_c.view(np.uint32)).all() and (n_g.view(np.uint32) == n_c.view(np.uint32)).all(), f
        _assert_same_map(cpu, gpu)
    finally:
        cpu.close(); gpu.close()


def test_subsampled_millimetre_upload_at_an_odd_size():
    """set_depth_mm of a 326x202 image into a 163x101 handle (ratio 2, mm2metersKernel's subsampling, preprocessing.cpp:161-188) against the
    oracle's map of the subsampled metres: the map and every raycast, bit for bit."""
    W, H, N, dim, mu, frames = CONSUMER["W"], CONSUMER["H"], CONSUMER["N"], CONSUMER["dim"], 0.1, 5
    fx, fy, cx, cy = CONSUMER["k"]
    big = RoomStream(2 * W, 2 * H, dim, (2 * fx, 2 * fy, 2 * cx, 2 * cy))
    k = np.asarray(CONSUMER["k"], np.float32)
    cpu = OraclePipeline(SDF, N, dim, W, H)
    gpu = DenseSLAMPipeline((W, H), N, dim, field_type=SDF)
    try:
        hits = []
        for f in range(frames):
            mm = big.depth_mm(f)
            depth = np.ascontiguousarray(mm[::2, ::2].astype(np.float32) / np.float32(1000.0))
            pose = big.pose(f)
            gpu.set_depth_mm(mm); gpu.setPose(pose)
            gpu.integration(k, 1, mu, f)
            ran = gpu.raycasting(k, mu, f)
            cpu.integrate(depth, pose, k, mu, f)
            ran_c, v_c, n_c = cpu.raycast(pose, k, mu, f)
            assert ran == ran_c
            if ran:
                v_g, n_g = gpu.vertex_normal()
                hits.append(_assert_same_images({"v_c": v_c, "n_c": n_c, "v_g": v_g, "n_g": n_g}, dim / N, f))
        m = _assert_same_map(cpu, gpu)
        assert m["blocks_gpu"] > 500 and min(hits) > 0.6 * W * H, (m, hits)
        print("set_depth_mm ratio 2:", json.dumps({"blocks": m["blocks_gpu"], "hits": hits}))
    finally:
        cpu.close(); gpu.close()
