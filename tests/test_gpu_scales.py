"""Oracle parity, bit for bit, off the 1.2 * 2^k voxel grid: the scan, the sweep, the raycast and the readers of the map at the volume dimensions,
resolutions and mu of tests/scale_frames.py (held to be well posed and non-trivial by tests/test_scale_frames_oracle.py).  Every other stream
of the suite has a voxel size of 1.2 * 2^j and a mu / voxel between about 0.4 and 20, so every scale constant the kernels receive has had one
float32 mantissa; here the voxel sizes have more than thirty, mu / voxel runs from 8e-8 to 25.6, and mu stands on either side of the switch
between the fast and the IEEE sweep.

Per named case, dense and pooled: the whole map after every frame and every raycast that runs; from the final map the camera's rays through
cast_rays, renderVolume from another pose, interp and grad at the hit points and around the faces, and the marching-cubes triangles.  Then the
scan's band steps and the sweep's block count per frame, the one-queue schedule from device-resident depth, the fast against the IEEE sweep,
and the seeded table."""
import time

import numpy as np
import pytest

from oracle.binding import OFUSION, SDF, OraclePipeline
from supereight_amd.pipeline import DenseSLAMPipeline
from supereight_amd.synthetic import to_colmajor
from tests import ray_cast_util as U
from tests.map_query_util import Map, compare
from tests.parity_util import compare_maps, compare_raycast
from tests.scale_frames import MU_FAST_MIN, NAMED, SEEDED, SEEDED_TRIPLES, scale_stream
from tests.test_gpu_stress_parity import _pipelined_case

pytestmark = pytest.mark.gpu

IDS = [c["name"] for c in NAMED]
UP_TO_256 = [c for c in NAMED if c["N"] <= 256]
FAST = [c for c in NAMED if c["mu"] >= MU_FAST_MIN]


def _assert_same_map(cpu, gpu, what):
    m = compare_maps(cpu, gpu)
    assert m["same_block_set"] and m["same_node_set"], (what, m)
    assert m["x_mismatch"] == 0 and m["y_mismatch"] == 0 and m["active_mismatch"] == 0, (what, m)
    assert m["node_x_mismatch"] == 0 and m["node_y_mismatch"] == 0, (what, m)
    return m


def _assert_same_raycast(rec, voxel, what):
    r = compare_raycast(rec, voxel)
    assert r["hitmask_mismatch"] == 0 and r["vertex_bit_mismatch_px"] == 0 and r["normal_bit_mismatch_px"] == 0, (what, r)
    return r["hits_cpu"]


def _face_points(rng, dim, N, n=256):
    """Points (metres) on the six faces of the volume, up to two voxels beyond them, and on its edges and corners."""
    vox = dim / N
    p = rng.uniform(0, dim, (n, 3))
    for i in range(n):
        for a in rng.choice(3, 1 + i % 3, replace=False):
            side = rng.integers(0, 2)
            p[i, a] = (dim if side else 0.0) + (0.0 if i % 4 == 0 else rng.uniform(-2, 2) * vox)
    return p.astype(np.float32)


def _canon(m):
    b = np.ascontiguousarray(m.reshape(-1, 9)).view(np.uint32)
    return b[np.lexsort(b.T[::-1])]


@pytest.mark.parametrize("pool", ["dense", "pooled"])
@pytest.mark.parametrize("case", NAMED, ids=IDS)
def test_named_scale_equals_the_oracle(oracle, case, pool):
    t0 = time.time()
    Wd, Ht, N, dim, mu, field, frames = case["W"], case["H"], case["N"], case["dim"], case["mu"], case["field"], case["frames"]
    s = scale_stream(case)
    lib = U.load()
    cpu = U.oracle_pipeline(lib, field, N, dim, Wd, Ht)
    cpu.count_stats(True)
    gpu = DenseSLAMPipeline((Wd, Ht), N, dim, field_type=field, max_blocks=case["pooled"] if pool == "pooled" else 0)
    m = None
    try:
        assert gpu.memory_info()["layout"] == ("pooled bricks" if pool == "pooled" else "dense brick grid")
        hits = []
        for f in range(frames):
            depth, pose = s.depth(f), s.pose(f)
            gpu.set_depth(depth); gpu.setPose(pose)
            assert gpu.integration(s.k, 1, mu, f) and cpu.integrate(depth, pose, s.k, mu, f)
            mm = _assert_same_map(cpu, gpu, (case["name"], f))
            ran, v_c, n_c = cpu.raycast(pose, s.k, mu, f)
            assert gpu.raycasting(s.k, mu, f) == ran == (f > 2)
            if ran:
                v_g, n_g = gpu.vertex_normal()
                hits.append(_assert_same_raycast({"v_c": v_c, "n_c": n_c, "v_g": v_g, "n_g": n_g}, dim / N, (case["name"], f)))
        st = cpu.stats()
        assert st["truncated"] == 0 and st["oob_ub"] == 0, st
        assert mm["blocks_gpu"] >= case["min_blocks"] and len(hits) == frames - 3 and min(hits) >= case["min_hits"], (mm, hits)
        if case["min_hits"] == 0:
            assert int((gpu.blocks()[2] != 0).sum()) >= case["min_written"]
        # the camera's rays through the batch
        rays = U.camera_rays(lib, pose, s.k, Wd, Ht)
        got = gpu.cast_rays(rays[:, 0:3].copy(), rays[:, 3:6].copy(), rays[:, 6].copy(), rays[:, 7].copy(), mu=mu)
        exp, trips = U.cast_rays(lib, cpu.h, rays, mu)
        for k in ("hit", "normal", "status"):
            bad = U.mismatches(got[k], exp[k])
            assert len(bad) == 0, (k, len(bad), rays[bad[:3]].tolist(), got[k][bad[:3]].tolist(), exp[k][bad[:3]].tolist())
        assert int(((exp["status"] & 4) != 0).sum()) >= case["min_hits"]
        # renderVolume from a second pose: its own march from the near plane, with largestep = 0.75 * mu.  Not that largestep for the SDF rows
        # at 2^-30: there 0.75 * mu is below half an ulp of t, so that the reference's own march (rendering_impl.hpp: `t += stepsize` with
        # stepsize = largestep at a voxel of weight 0) stops advancing at the first unobserved voxel a ray meets and never ends, on the oracle
        # as on the device.  Those two rows march with a largestep of one voxel, which does advance.
        stalls = field == SDF and 0.75 * mu < 2.0 ** -22
        largestep = dim / N if stalls else 0.75 * mu
        view = s.pose(frames + 20)
        a = gpu.renderVolume(view, s.k, mu, largestep)
        b = cpu.render_volume(view, pose, s.k, mu, largestep, v_c, n_c)
        assert (a == b).all() and (case["min_hits"] == 0 or (b[..., 0] > 0).sum() >= 100), int((b[..., 0] > 0).sum())
        # interp and grad at the hit points and around the faces (the oracle's octree is rebuilt from the device map voxel by voxel in
        # Python: most of the time of the two 512^3 rows)
        pts = np.concatenate([v_c[n_c[..., 0] != -2].reshape(-1, 3), _face_points(np.random.default_rng(5 + field), dim, N)])
        pts = np.ascontiguousarray(pts.astype(np.float32))
        m = Map(oracle, gpu, field, n=N, dim=dim)
        compare(gpu.query(pts, fine=False, coarse=False, interp=True, grad=True, status=False), m.expected(pts), what=("interp", "grad"))
        # the marching-cubes triangles (order unspecified)
        mo, mg = cpu.mesh(), gpu.mesh()
        flat = field == SDF and mu < 1e-6                 # every written x is 1.0: no crossing anywhere
        assert mo.shape == mg.shape and (mo.shape[0] == 0 if flat else mo.shape[0] > 1000), (mo.shape, mg.shape)
        assert (_canon(mo) == _canon(mg)).all()
        print(case["name"], pool, "blocks", mm["blocks_gpu"], "hits", hits, "ray trips", trips, "triangles", mg.shape[0],
              f"{time.time() - t0:.1f} s")
    finally:
        if m is not None:
            m.close()
        cpu.close(); gpu.close()


@pytest.mark.parametrize("pool", ["dense", "pooled"])
@pytest.mark.parametrize("case", NAMED, ids=IDS)
def test_scan_steps_and_swept_blocks_per_frame(case, pool):
    """`probes`, one count per band step inside the volume, and `swept`, the blocks the sweep takes, per frame against the oracle's: a scan that
    takes another number of band steps and ends with the same block set shows only here (as tests/test_gpu_attitudes.py
    test_tumble_swept_counts; a handle that counts takes other kernel instantiations, of the scan and of the sweep and others again on a
    pooled map, hence a test of its own over both layouts)."""
    s = scale_stream(case)
    cpu = OraclePipeline(case["field"], case["N"], case["dim"], case["W"], case["H"])
    gpu = DenseSLAMPipeline((case["W"], case["H"]), case["N"], case["dim"], field_type=case["field"], max_blocks=case["pooled"] if pool == "pooled" else 0)
    swept, probes = [], []
    try:
        assert gpu.memory_info()["layout"] == ("pooled bricks" if pool == "pooled" else "dense brick grid")
        cpu.count_stats(True)
        gpu.enable_stats(True)
        probes_before = 0
        for f in range(case["frames"]):
            depth, pose = s.depth(f), s.pose(f)
            gpu.set_depth(depth); gpu.setPose(pose)
            assert gpu.integration(s.k, 1, case["mu"], f) and cpu.integrate(depth, pose, s.k, case["mu"], f)
            g, c = gpu.stats(reset=True), cpu.stats()
            swept.append((g["swept"], c["swept"]))                          # (the oracle's is the last sweep's, its probes accumulate)
            probes.append((g["probes"], c["probes"] - probes_before))
            probes_before = c["probes"]
        print(case["name"], pool, "swept (device, oracle)", swept, "probes", probes)
        assert all(g == c for g, c in swept), swept
        assert all(g == c for g, c in probes), probes
        assert min(c for _, c in probes) > case["W"] * case["H"] // 2 and min(c for _, c in swept) >= case["min_blocks"] // 2
        _assert_same_map(cpu, gpu, "end")
    finally:
        cpu.close(); gpu.close()


@pytest.mark.parametrize("pool", ["dense", "pooled"])
@pytest.mark.parametrize("case", UP_TO_256, ids=[c["name"] for c in UP_TO_256])
def test_one_queue_stream_from_device_depth(case, pool):
    """se_hip_frame from device-resident depth back to back on a streaming handle, every frame's images in a ring: every slot, the final map,
    and the fused launches (k_raycast_scan, the launch the benchmark times) through the launch counters."""
    _pipelined_case(None, case["W"], case["H"], case["field"], case["N"], case["mu"], case["frames"], case["pooled"] if pool == "pooled" else 0, True,
                    min_hits_per_frame=case["min_hits"] - 1, stream=scale_stream(case))


@pytest.mark.parametrize("case", FAST, ids=[c["name"] for c in FAST])
def test_fast_and_ieee_sweeps_give_the_same_map(case, monkeypatch):
    """k_integrate<FAST> (shared refined reciprocal) and the compiler's own divisions (SE_HIP_IEEE_SWEEP=1) give byte-identical blocks and
    nodes at every scale whose mu the fast sweep admits.  (The two cases below 2^-30 take the IEEE sweep either way: for them the comparison
    with the oracle above is the test.)"""
    import torch
    s = scale_stream(case)
    frames = case["frames"]
    dev = torch.from_numpy(np.stack([s.depth(f) for f in range(frames)])).cuda()
    k = np.ascontiguousarray(s.k, np.float32)

    def run(ieee):
        if ieee:
            monkeypatch.setenv("SE_HIP_IEEE_SWEEP", "1")
        else:
            monkeypatch.delenv("SE_HIP_IEEE_SWEEP", raising=False)
        p = DenseSLAMPipeline((case["W"], case["H"]), case["N"], case["dim"], field_type=case["field"])      # (the knob is read once, here)
        for f in range(frames):
            p.frame(dev[f].data_ptr(), to_colmajor(s.pose(f)), k, case["mu"], f)
        out = p.blocks() + p.nodes()
        p.close()
        return out

    a, b = run(False), run(True)
    assert len(a[0]) >= case["min_blocks"]
    for u, v in zip(a, b):
        assert u.shape == v.shape and (u.view(np.uint8) == v.view(np.uint8)).all()


@pytest.mark.parametrize("field", [SDF, OFUSION], ids=["sdf", "ofusion"])
def test_seeded_scales_equal_the_oracle(field):
    """The sixteen seeded (dim, N, mu) of a field, dense and eager, one pipeline per case: the map after every frame and every raycast."""
    cases = [c for c in SEEDED if c["field"] == field]
    assert len(cases) == len(SEEDED_TRIPLES[field]) == 16
    for case in cases:
        name, N, dim, mu = case["name"], case["N"], case["dim"], case["mu"]
        s = scale_stream(case)
        cpu = OraclePipeline(field, N, dim, case["W"], case["H"])
        gpu = DenseSLAMPipeline((case["W"], case["H"]), N, dim, field_type=field)
        try:                                              # (a case that fails leaves no handle open for the cases and tests behind it)
            cpu.count_stats(True)
            hits = []
            for f in range(case["frames"]):
                depth, pose = s.depth(f), s.pose(f)
                gpu.set_depth(depth); gpu.setPose(pose)
                assert gpu.integration(s.k, 1, mu, f) and cpu.integrate(depth, pose, s.k, mu, f), (name, f)
                _assert_same_map(cpu, gpu, (name, f))
                ran, v_c, n_c = cpu.raycast(pose, s.k, mu, f)
                assert gpu.raycasting(s.k, mu, f) == ran == (f > 2), (name, f)
                if ran:
                    v_g, n_g = gpu.vertex_normal()
                    hits.append(_assert_same_raycast({"v_c": v_c, "n_c": n_c, "v_g": v_g, "n_g": n_g}, dim / N, (name, f)))
            st = cpu.stats()
            assert st["truncated"] == 0 and st["oob_ub"] == 0, (name, st)
            assert cpu.counts()[0] >= case["min_blocks"] and len(hits) == case["frames"] - 3 and min(hits) >= case["min_hits"], (name, hits)
        finally:
            cpu.close(); gpu.close()
