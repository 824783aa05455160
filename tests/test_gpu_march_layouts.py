"""Every instantiation of the marches (se_cast_ray_sdf_lean / se_cast_ray_sdf_pooled, se_cast_ray_of over the brick-layout policies of se_kernels.h) at a small shape,
bit for bit against the oracle: {SDF, OFusion} x {dense grid with 32-bit byte offsets, dense grid with (block, local) pairs, pooled bricks}.

The dense (block, local) policy and the searches with has_deep are otherwise reached only from 1024^3 on.  Here SE_HIP_RAY_CACHE_LEVELS = 2
selects them at 128^3: leaf_level = log2(128 / 8) = 4 and two occupancy levels are staged in LDS, so has_deep = (2 < leaf_level - 1) is set; the
launch is then not `shallow`, and o32 = dense && shallow && planes <= 4 GiB is false: k_raycast / k_cast_rays run <.., DENSE, !SHALLOW, !O32>
(se_hip_api.hip, ray_select).  se_hip_create reads the variable, so it is set before the pipeline is constructed.  The volume renderer always
marches with the (block, local) policy on a dense grid.

After six frames of the 160x120 room stream into 128^3 over 4.8 m (340 blocks; the oracle alone: 15 748 hits for SDF, 16 868 for OFusion,
no key dropped; integrated by the device and by the oracle), from the map both now hold:
the camera raycast, the same camera's rays through cast_rays, renderVolume from a second pose, and a query of interp and grad at the hit
points plus 256 points on and beyond the faces of the volume."""
import numpy as np
import pytest

from supereight_amd.pipeline import OFUSION, SDF, DenseSLAMPipeline
from supereight_amd.synthetic import make_stream
from tests import ray_cast_util as U
from tests.parity_util import compare_raycast
from tests.map_query_util import Map, compare

pytestmark = pytest.mark.gpu

W, H, N, DIM = 160, 120, 128, 4.8
FRAMES = 6
MU = {SDF: 0.1, OFUSION: 0.015}       # OFusion: below the 0.02 at which a 160x120 scan of 128^3 can outrun the reference's key reserve (tests/time_axis_util.py)
MIN_HITS = 300                        # the floor _pipelined_case (tests/test_gpu_stress_parity.py) puts under a 320x240 image
LAYOUTS = {"dense_o32": (0, None), "dense_64": (0, "2"), "pooled": (4096, None)}      # name -> (max_blocks, SE_HIP_RAY_CACHE_LEVELS)


def _face_points(rng, n=256):
    """Points (metres) on the six faces of the volume, up to two voxels beyond them, and on its edges and corners."""
    vox = DIM / N
    p = rng.uniform(0, DIM, (n, 3))
    for i in range(n):
        axes = rng.choice(3, 1 + i % 3, replace=False)
        for a in axes:
            side = rng.integers(0, 2)
            p[i, a] = (DIM if side else 0.0) + (0.0 if i % 4 == 0 else rng.uniform(-2, 2) * vox)
    return p.astype(np.float32)


@pytest.mark.parametrize("layout", list(LAYOUTS), ids=list(LAYOUTS))
@pytest.mark.parametrize("field", [SDF, OFUSION], ids=["sdf", "ofusion"])
def test_march_layouts_equal_the_oracle(oracle, monkeypatch, field, layout):
    max_blocks, cache_levels = LAYOUTS[layout]
    if cache_levels is not None:
        monkeypatch.setenv("SE_HIP_RAY_CACHE_LEVELS", cache_levels)
    else:
        monkeypatch.delenv("SE_HIP_RAY_CACHE_LEVELS", raising=False)
    mu = MU[field]
    s = make_stream("room", W, H, DIM, holes=False)
    lib = U.load()
    gpu = DenseSLAMPipeline((W, H), N, DIM, field_type=field, max_blocks=max_blocks)
    cpu = U.oracle_pipeline(lib, field, N, DIM, W, H)
    m = None
    try:
        assert gpu.memory_info()["layout"] == ("dense brick grid" if max_blocks == 0 else "pooled bricks")
        for f in range(FRAMES):
            depth, pose = s.depth(f), s.pose(f)
            gpu.set_depth(depth); gpu.setPose(pose)
            assert gpu.integration(s.k, 1, mu, f) == cpu.integrate(depth, pose, s.k, mu, f)
            gpu.raycasting(s.k, mu, f)
        # the camera raycast
        ran, v_c, n_c = cpu.raycast(pose, s.k, mu, FRAMES - 1)
        v_g, n_g = gpu.vertex_normal()
        r = compare_raycast({"v_c": v_c, "n_c": n_c, "v_g": v_g, "n_g": n_g}, DIM / N)
        print("raycast", r)
        assert ran and r["hits_cpu"] >= MIN_HITS, r
        assert r["hitmask_mismatch"] == 0 and r["vertex_bit_mismatch_px"] == 0 and r["normal_bit_mismatch_px"] == 0, r
        # the same camera's rays through the batch
        rays = U.camera_rays(lib, pose, s.k, W, H)
        got = gpu.cast_rays(rays[:, 0:3].copy(), rays[:, 3:6].copy(), rays[:, 6].copy(), rays[:, 7].copy(), mu=mu)
        exp, trips = U.cast_rays(lib, cpu.h, rays, mu)
        assert trips < 4096
        for k in ("hit", "normal", "status"):
            bad = U.mismatches(got[k], exp[k])
            assert len(bad) == 0, (k, len(bad), rays[bad[:3]].tolist(), got[k][bad[:3]].tolist(), exp[k][bad[:3]].tolist())
        assert int(((got["status"] & 4) != 0).sum()) == r["hits_cpu"]
        # renderVolume from a second pose: its own march from the near plane
        view = s.pose(FRAMES + 20)
        a = gpu.renderVolume(view, s.k, mu, 0.75 * mu)
        b = cpu.render_volume(view, pose, s.k, mu, 0.75 * mu, v_c, n_c)
        assert (a == b).all() and (b[..., 0] > 0).sum() >= MIN_HITS
        # interp and grad at the hit points and around the faces
        hits = v_c[n_c[..., 0] != -2].reshape(-1, 3)
        pts = np.ascontiguousarray(np.concatenate([hits, _face_points(np.random.default_rng(5 + field))]).astype(np.float32))
        m = Map(oracle, gpu, field, n=N, dim=DIM)
        compare(gpu.query(pts, fine=False, coarse=False, interp=True, grad=True, status=False), m.expected(pts), what=("interp", "grad"))
    finally:
        if m is not None:
            m.close()
        gpu.close(); cpu.close()
