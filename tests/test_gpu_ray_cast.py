"""Batched ray casts on the device (se_hip_cast_rays / DenseSLAMPipeline.cast_rays / DenseSLAMSystem::castRays) against the CPU helper
tests/cpp/ray_cast_oracle.cpp -- the per-pixel body of the oracle's raycastKernel for arbitrary rays, itself pinned to the oracle's camera
raycast by tests/test_ray_cast_host.py.  Device and oracle integrate the same stream; every comparison is bit for bit (memcmp, NaN-aware).
  - camera equivalence: the camera's own rays through the batch give se_hip_raycast's images and the oracle's, for SDF / OFusion, dense /
    pooled bricks, 512^3 / 1024^3 (and 2048^3 dense), the room and stress streams, 640x480 and ragged shapes;
  - arbitrary rays: origins inside, on faces / edges / corners and beyond each face, random, axis-aligned and near-axis directions, per-ray
    near / far (near > far, near <= 0, far beyond the cube), every output and status bit;
  - invalid rays, the schedule (a batch between frames sees exactly the frames before it and disturbs nothing), the four entry paths, a
    batch of 2^25 rays (several launches), n == 0 and the refusals."""
import ctypes as C

import numpy as np
import pytest

from supereight_amd.pipeline import OFUSION, SDF, DenseSLAMPipeline, SeHipError, _RayOut
from supereight_amd.synthetic import make_stream
from tests import ray_cast_util as U
from tests.edge_frames import SHAPE_CASES, edge_stream
from tests.gpu_state_util import map_state
from tests.mirror_util import build_mirror, run_mirror, write_scene
from tests.parity_util import compare_raycast, outside_view

pytestmark = pytest.mark.gpu
DIM = 4.8
MISS_NORMAL = np.float32([-2, 0, 0])


def _both(field, W, H, N, max_blocks, mu, frames, stream, dim=DIM):
    """Device handle and oracle pipeline (on the helper library) after the same frames; the device raycasts every frame."""
    lib = U.load()
    gpu = DenseSLAMPipeline((W, H), N, dim, field_type=field, max_blocks=max_blocks)
    cpu = U.oracle_pipeline(lib, field, N, dim, W, H)
    for f in range(frames):
        d, pose = stream.depth(f), stream.pose(f)
        gpu.set_depth(d); gpu.setPose(pose)
        gpu.integration(stream.k, 1, mu, f)
        gpu.raycasting(stream.k, mu, f)
        cpu.integrate(d, pose, stream.k, mu, f)
    assert gpu.memory_info()["layout"] == ("dense brick grid" if max_blocks == 0 else "pooled bricks")
    return lib, gpu, cpu


def _same(got, exp, rays=None):
    for k in ("hit", "normal", "status"):
        bad = U.mismatches(got[k], exp[k])
        assert len(bad) == 0, (k, len(bad), bad[:5].tolist(), None if rays is None else rays[bad[:3]].tolist(),
                               got[k][bad[:3]].tolist(), exp[k][bad[:3]].tolist())


def _cast_dev(gpu, rays, mu):
    return gpu.cast_rays(rays[:, 0:3].copy(), rays[:, 3:6].copy(), rays[:, 6].copy(), rays[:, 7].copy(), mu=mu)


def _images_of(res):
    """What the camera raycast writes for these outputs: vertex = hit xyz where w > 0, else 0; normal as is."""
    hit = (res["status"] & 4) != 0
    return np.where(hit[:, None], res["hit"][:, :3], np.float32(0)).astype(np.float32), res["normal"]


def _camera_check(lib, gpu, cpu, pose, k, W, H, mu, frame):
    rays = U.camera_rays(lib, pose, k, W, H)
    got = _cast_dev(gpu, rays, mu)
    exp, trips = U.cast_rays(lib, cpu.h, rays, mu)
    assert trips < 4096, f"a ray reached the iterator's trip cap ({trips})"
    _same(got, exp, rays)
    gpu.setPose(pose)
    assert gpu.raycasting(k, mu, frame)
    v_g, n_g = gpu.vertex_normal()
    v, n = _images_of(got)
    assert U.bits_equal(v, v_g.reshape(-1, 3)) and U.bits_equal(n, n_g.reshape(-1, 3)), "batch vs se_hip_raycast"
    ran, v_c, n_c = cpu.raycast(pose, k, mu, frame)
    assert ran and U.bits_equal(v, v_c.reshape(-1, 3)) and U.bits_equal(n, n_c.reshape(-1, 3)), "batch vs the oracle's raycast"
    return int(((got["status"] & 4) != 0).sum())


CAMERA = [
    # name, stream, field, N, max_blocks, mu, frames
    ("sdf_dense_512", "room", SDF, 512, 0, 0.1, 4),
    ("ofusion_dense_512", "room", OFUSION, 512, 0, 0.02, 4),
    ("sdf_pooled_512", "room", SDF, 512, 1 << 16, 0.1, 4),
    ("ofusion_pooled_512", "room", OFUSION, 512, 1 << 16, 0.02, 4),
    ("sdf_dense_1024", "room", SDF, 1024, 0, 0.1, 4),
    ("ofusion_dense_1024", "room", OFUSION, 1024, 0, 0.02, 4),
    ("sdf_pooled_1024", "room", SDF, 1024, 1 << 18, 0.1, 4),
    ("ofusion_pooled_1024", "room", OFUSION, 1024, 1 << 18, 0.02, 4),
    ("stress_sdf_dense_512", "stress", SDF, 512, 0, 0.1, 8),
    ("stress_ofusion_pooled_1024", "stress", OFUSION, 1024, 1 << 18, 0.008, 8),
]


@pytest.mark.parametrize("name,kind,field,N,max_blocks,mu,frames", CAMERA, ids=[c[0] for c in CAMERA])
def test_camera_rays_equal_the_camera_raycast(name, kind, field, N, max_blocks, mu, frames):
    W, H = 640, 480
    s = make_stream(kind, W, H, DIM, holes=False) if kind == "room" else make_stream(kind, W, H, DIM)
    lib, gpu, cpu = _both(field, W, H, N, max_blocks, mu, frames, s)
    try:
        hits = _camera_check(lib, gpu, cpu, s.pose(frames - 1), s.k, W, H, mu, frames)
        hits += _camera_check(lib, gpu, cpu, outside_view("+y_tilted", 0.03, DIM), s.k, W, H, mu, frames + 1)
        assert hits > 50000
    finally:
        gpu.close(); cpu.close()


def test_camera_rays_at_2048_dense():
    W, H, N, mu, frames = 320, 240, 2048, 0.1, 4
    s = make_stream("room", W, H, DIM, holes=False)
    try:
        lib, gpu, cpu = _both(SDF, W, H, N, 0, mu, frames, s)
    except SeHipError as e:
        pytest.skip(f"a dense 2048^3 map does not fit this device: {e}")
    try:
        assert _camera_check(lib, gpu, cpu, s.pose(frames - 1), s.k, W, H, mu, frames) > 10000
    finally:
        gpu.close(); cpu.close()


RAGGED = [c for c in SHAPE_CASES if c["name"] in ("ragged_161x97_aniso_sdf", "large_721x481_negfy_ofusion")]


@pytest.mark.parametrize("case", RAGGED, ids=[c["name"] for c in RAGGED])
def test_camera_rays_at_ragged_shapes(case):
    s = edge_stream(case)
    W, H = case["W"], case["H"]
    lib, gpu, cpu = _both(case["field"], W, H, case["N"], case["pooled"], case["mu"], case["frames"], s, dim=case["dim"])
    try:
        assert _camera_check(lib, gpu, cpu, s.pose(case["frames"] - 1), s.k, W, H, case["mu"], case["frames"]) > 0
    finally:
        gpu.close(); cpu.close()


def _unit(v):
    v = np.asarray(v, np.float32)
    z = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    return (v / np.sqrt(z)[:, None]).astype(np.float32)


def arbitrary_rays(rng, N, dim, n_each=800):
    """Origins inside the volume, on its faces / edges / corners and 1-3 voxels beyond each face; random unit, axis-aligned and near-axis
    directions (components below the iterator's epsilon 1 / N, both signs); default, random, inverted, non-positive and far-reaching planes."""
    vox = dim / N
    o = [rng.uniform(0, dim, (3 * n_each, 3))]
    for naxes in (1, 2, 3):                                   # faces, edges, corners
        p = rng.uniform(0, dim, (n_each, 3))
        for i in range(n_each):
            ax = rng.choice(3, naxes, replace=False)
            p[i, ax] = rng.choice([0.0, dim], naxes)
        o.append(p)
    for face in range(6):                                     # 1-3 voxels beyond each face
        p = rng.uniform(0, dim, (n_each // 2, 3))
        p[:, face // 2] = dim + rng.uniform(1, 3, n_each // 2) * vox if face & 1 else -rng.uniform(1, 3, n_each // 2) * vox
        o.append(p)
    o = np.concatenate(o).astype(np.float32)
    n = len(o)
    kind = rng.integers(0, 4, n)
    d = rng.normal(size=(n, 3))
    axis = np.zeros((n, 3)); axis[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-1.0, 1.0], n)
    d = np.where((kind == 1)[:, None], axis, d)
    tiny = axis + rng.choice([-1.0, 1.0], (n, 3)) * rng.uniform(0.01, 0.9, (n, 3)) / N * (axis == 0)
    d = np.where((kind == 2)[:, None], tiny, d)
    d = _unit(d)
    near = np.full(n, 0.4, np.float32); far = np.full(n, 4.0, np.float32)
    plane = rng.integers(0, 6, n)
    near = np.where(plane == 1, rng.uniform(0, 2, n), near)
    far = np.where(plane == 1, near + rng.uniform(0, 3, n), far)
    near = np.where(plane == 2, 3.0, near); far = np.where(plane == 2, 1.0, far)            # near > far
    near = np.where(plane == 3, rng.choice([0.0, -0.0, -1.0], n), near)                      # near <= 0
    far = np.where(plane == 4, 100.0, far)                                                   # far beyond the cube
    near = np.where(plane == 5, 0.0, near); far = np.where(plane == 5, 1e30, far)
    return np.ascontiguousarray(np.concatenate([o, d, near[:, None], far[:, None]], axis=1).astype(np.float32))


ARBITRARY = [
    ("sdf_dense_512", "room", SDF, 512, 0, 0.1),
    ("ofusion_pooled_512", "room", OFUSION, 512, 1 << 15, 0.02),
    ("sdf_pooled_1024", "room", SDF, 1024, 1 << 17, 0.1),
    ("ofusion_dense_1024", "room", OFUSION, 1024, 0, 0.02),
    ("stress_ofusion_dense_512", "stress", OFUSION, 512, 0, 0.008),
    ("stress_sdf_pooled_1024", "stress", SDF, 1024, 1 << 17, 0.1),
]


@pytest.mark.parametrize("name,kind,field,N,max_blocks,mu", ARBITRARY, ids=[c[0] for c in ARBITRARY])
def test_arbitrary_rays_equal_the_oracle(name, kind, field, N, max_blocks, mu):
    W, H, frames = 320, 240, 6
    s = make_stream(kind, W, H, DIM, holes=False) if kind == "room" else make_stream(kind, W, H, DIM)
    lib, gpu, cpu = _both(field, W, H, N, max_blocks, mu, frames, s)
    try:
        rays = arbitrary_rays(np.random.default_rng(N + 7 * field), N, DIM)
        got = _cast_dev(gpu, rays, mu)
        exp, trips = U.cast_rays(lib, cpu.h, rays, mu)
        assert trips < 4096, f"a ray reached the iterator's trip cap ({trips})"
        _same(got, exp, rays)
        st = got["status"]
        assert (st & 1).all()
        for bit in (2, 4, 8):                   # a non-trivial set: every status bit both set and clear somewhere
            assert ((st & bit) != 0).any() and ((st & bit) == 0).any(), bit
        assert not ((st & 4) & ~((st & 2) << 1)).any()      # a hit implies the march ran
        miss = (st & 4) == 0
        assert (got["normal"][miss] == MISS_NORMAL).all()
    finally:
        gpu.close(); cpu.close()


def _invalid_rays(N, dim):
    base = np.float32([dim / 2, dim / 2, 0.3, 0, 0, 1, 0.4, 4.0])
    out = []
    for slot in range(8):
        for v in (np.nan, np.inf, -np.inf):
            r = base.copy(); r[slot] = v; out.append(r)
    for scale in (0.98 ** 0.5 * 0.999, 1.02 ** 0.5 * 1.001, 0.0, 1e-3, 10.0):
        r = base.copy(); r[3:6] = np.float32([0.6, 0.0, 0.8]) * np.float32(scale); out.append(r)
    lim = np.float32(2.0 ** 20) / (np.float32(N) / np.float32(dim))
    for ax in range(3):
        for sgn in (1, -1):
            r = base.copy(); r[ax] = sgn * lim * np.float32(1.0001); out.append(r)
    r = base.copy(); r[0] = 1e30; out.append(r)
    return np.stack(out).astype(np.float32)


@pytest.mark.parametrize("field,max_blocks", [(SDF, 0), (OFUSION, 1 << 15)], ids=["sdf_dense", "ofusion_pooled"])
def test_invalid_rays_and_mixing(field, max_blocks):
    W, H, N, mu = 320, 240, 512, (0.1 if field == SDF else 0.02)
    s = make_stream("room", W, H, DIM, holes=False)
    lib, gpu, cpu = _both(field, W, H, N, max_blocks, mu, 4, s)
    try:
        bad = _invalid_rays(N, DIM)
        got = _cast_dev(gpu, bad, mu)
        assert (got["status"] == 0).all() and (got["hit"].view(np.uint32) == 0).all() and (got["normal"] == MISS_NORMAL).all()
        exp, _ = U.cast_rays(lib, cpu.h, bad, mu)
        _same(got, exp, bad)
        # the band's own edges are valid
        edge = np.repeat(bad[:1], 2, axis=0); edge[:, 0] = DIM / 2
        edge[0, 3:6] = [0, 0, np.sqrt(np.float32(0.981))]; edge[1, 3:6] = [0, 0, np.sqrt(np.float32(1.019))]
        assert (_cast_dev(gpu, edge, mu)["status"] & 1).all()
        good = arbitrary_rays(np.random.default_rng(3), N, DIM, n_each=200)
        alone = _cast_dev(gpu, good, mu)
        mixed = np.concatenate([good, bad])[np.random.default_rng(4).permutation(len(good) + len(bad))]
        res = _cast_dev(gpu, mixed, mu)
        order = np.argsort(np.random.default_rng(4).permutation(len(good) + len(bad)))
        for k in res:
            assert U.bits_equal(res[k][order][: len(good)], alone[k]), k
    finally:
        gpu.close(); cpu.close()


def test_batches_disturb_nothing_on_a_synchronous_handle():
    W, H, N, mu = 320, 240, 512, 0.1
    s = make_stream("room", W, H, DIM, holes=False)
    lib, gpu, cpu = _both(SDF, W, H, N, 0, mu, 4, s)
    try:
        rays = arbitrary_rays(np.random.default_rng(1), N, DIM, n_each=200)
        gpu.enable_timing(True)
        before, t0 = map_state(gpu), gpu.timings()
        n0 = gpu.launch_counts()
        first = _cast_dev(gpu, rays, mu)
        import torch
        t = torch.from_numpy(rays).cuda()
        gpu.cast_rays(t[:, 0:3].contiguous(), t[:, 3:6].contiguous(), t[:, 6], t[:, 7], mu=mu)
        assert gpu.launch_counts() == n0
        assert gpu.timings() == t0
        after = map_state(gpu)
        assert all((u == w).all() for u, w in zip(before, after))
        again = _cast_dev(gpu, rays, mu)
        for k in first:
            assert U.bits_equal(first[k], again[k]), k
    finally:
        gpu.close(); cpu.close()


@pytest.mark.parametrize("field,max_blocks", [(SDF, 0), (OFUSION, 1 << 15)], ids=["sdf_dense", "ofusion_pooled"])
def test_batches_between_streamed_frames(field, max_blocks):
    """A streaming handle (one-queue schedule, image ring, every frame's raycast deferred into the next frame's scan launch): a batch cast
    after frame f, with that frame's raycast still held back, equals the oracle after frame f; it launches nothing counted, leaves the
    deferral in place, and every ring slot and the final map stay bit-exact with the oracle."""
    import torch
    from supereight_amd.synthetic import to_colmajor
    W, H, N, frames = 320, 240, 512, 7
    mu = 0.1 if field == SDF else 0.02
    s = make_stream("room", W, H, DIM, holes=False)
    lib = U.load()
    depths = [s.depth(f) for f in range(frames)]
    poses = [s.pose(f) for f in range(frames)]
    dev = torch.from_numpy(np.stack(depths)).cuda()
    k = np.ascontiguousarray(s.k, np.float32)
    gpu = DenseSLAMPipeline((W, H), N, DIM, field_type=field, max_blocks=max_blocks)
    cpu = U.oracle_pipeline(lib, field, N, DIM, W, H)
    ring = torch.zeros((frames, 2, H, W, 3), dtype=torch.float32, device="cuda")
    gpu.set_image_ring(ring.data_ptr(), frames, keepalive=ring)
    try:
        assert gpu.set_streaming(True)
        rays = arbitrary_rays(np.random.default_rng(21), N, DIM, n_each=150)
        gpu.launch_counts(reset=True)
        n_pend, oracle_images = 0, []
        for f in range(frames):
            assert gpu.frame(dev[f].data_ptr(), to_colmajor(poses[f]), k, mu, f) == (3 if f > 2 else 1)
            cpu.integrate(depths[f], poses[f], s.k, mu, f)
            oracle_images.append(cpu.raycast(poses[f], s.k, mu, f))
            n = gpu.launch_counts()
            got = _cast_dev(gpu, rays, mu)
            assert gpu.launch_counts() == n, f
            n_pend += n["pending"]
            exp, _ = U.cast_rays(lib, cpu.h, rays, mu)
            _same(got, exp, rays)
        assert n_pend >= frames - 3
        n = gpu.launch_counts()
        assert n["fused"] == frames - 4 and n["raycast"] == frames - 4, n
        gpu.sync()
        ring_h = ring.cpu().numpy()
        for f in range(3, frames):
            ran, v_c, n_c = oracle_images[f]
            assert ran
            r = compare_raycast({"v_c": v_c, "n_c": n_c, "v_g": ring_h[f, 0], "n_g": ring_h[f, 1]}, DIM / N)
            assert r["hitmask_mismatch"] == 0 and r["vertex_bit_mismatch_px"] == 0 and r["normal_bit_mismatch_px"] == 0, (f, r)
        gc, gx, _, _ = gpu.blocks()
        nb, _ = cpu.counts()
        assert len(gc) == nb
    finally:
        gpu.close(); cpu.close()


@pytest.mark.parametrize("field,max_blocks", [(SDF, 1 << 15), (OFUSION, 0)], ids=["sdf_pooled", "ofusion_dense"])
def test_entry_paths_agree(tmp_path, field, max_blocks):
    """Host entry (numpy) = device entry (raw pointers) = torch path (packed on the device, normalize=True on unit vectors) = C++ castRays."""
    import torch
    from supereight_amd.synthetic import render_depth_mm
    W, H, N, dim, frames = 160, 120, 256, 2.4, 4
    mu = 0.1 if field == SDF else 0.02
    raw, pf, s = write_scene(tmp_path, W, H, dim, frames)
    mm = [render_depth_mm(f, W, H, dim) for f in range(frames)]
    poses = np.stack([s.pose(f) for f in range(frames)]).astype(np.float32)
    p = DenseSLAMPipeline((W, H), N, dim, field_type=field, max_blocks=max_blocks)
    try:
        for f in range(frames):
            p.set_depth_mm(mm[f]); p.setPose(poses[f])
            p.integration(s.k, 1, mu, f)
            p.raycasting(s.k, mu, f)
        rays = arbitrary_rays(np.random.default_rng(5), N, dim, n_each=300)
        host = _cast_dev(p, rays, mu)
        assert (host["status"] & 4).any()
        t = torch.from_numpy(rays).cuda()
        tor = p.cast_rays(t[:, 0:3].contiguous(), t[:, 3:6].contiguous(), t[:, 6].contiguous(), t[:, 7].contiguous(), mu=mu)
        for k in host:
            assert isinstance(tor[k], torch.Tensor) and tor[k].device.type == "cuda"
            assert U.bits_equal(tor[k].cpu().numpy(), host[k]), k
        out = {k: torch.empty((len(rays),) + v.shape[1:], dtype=tor[k].dtype, device="cuda") for k, v in host.items()}
        o = _RayOut(out["hit"].data_ptr(), out["normal"].data_ptr(), out["status"].data_ptr())
        assert p.lib.se_hip_cast_rays(p._h, t.data_ptr(), len(rays), mu, C.byref(o)) == 0
        p.sync()
        for k in host:
            assert U.bits_equal(out[k].cpu().numpy(), host[k]), k
        # a subset of the outputs: the same values
        part = p.cast_rays(rays[:, 0:3].copy(), rays[:, 3:6].copy(), rays[:, 6].copy(), rays[:, 7].copy(), mu=mu, hit=False, normal=True, status=False)
        assert set(part) == {"normal"} and U.bits_equal(part["normal"], host["normal"])
        # normalize=True: the wrapper's float32 normalisation (Eigen's normalized()), then the same casts
        nrm = p.cast_rays(rays[:, 0:3].copy(), rays[:, 3:6] * np.float32(1.005), rays[:, 6].copy(), rays[:, 7].copy(), mu=mu, normalize=True)
        ref = p.cast_rays(rays[:, 0:3].copy(), _unit(rays[:, 3:6] * np.float32(1.005)), rays[:, 6].copy(), rays[:, 7].copy(), mu=mu)
        for k in host:
            assert U.bits_equal(nrm[k], ref[k]), k
        # the C++ mirror
        exe = build_mirror(tmp_path, "ray_cast_mirror", "SDF" if field == SDF else "OFusion")
        rf, of = str(tmp_path / "rays.bin"), str(tmp_path / "out.bin")
        rays.tofile(rf)
        _, r = run_mirror(exe, [raw, pf, N, dim, mu, rf, of], timeout=300)
        data = np.fromfile(of, np.uint8)
        n = len(rays)
        cpp = {"hit": data[: 16 * n].view(np.float32).reshape(n, 4), "normal": data[16 * n: 28 * n].view(np.float32).reshape(n, 3), "status": data[28 * n:]}
        for k in host:
            assert U.bits_equal(cpp[k], host[k]), k
        assert f"rays {n} hits {int(((host['status'] & 4) != 0).sum())}" in r.stdout
    finally:
        p.close()


def test_a_batch_of_2_25_rays_runs_in_several_launches():
    import torch
    W, H, N, mu = 160, 120, 512, 0.1
    s = make_stream("room", W, H, DIM, holes=False)
    lib, gpu, cpu = _both(SDF, W, H, N, 0, mu, 4, s)
    try:
        base = arbitrary_rays(np.random.default_rng(8), N, DIM, n_each=512)[:4096]
        ref = _cast_dev(gpu, base, mu)
        exp, _ = U.cast_rays(lib, cpu.h, base, mu)
        _same(ref, exp, base)
        reps = (1 << 25) // len(base)
        t = torch.from_numpy(base).cuda().repeat(reps, 1)
        res = gpu.cast_rays(t[:, 0:3].contiguous(), t[:, 3:6].contiguous(), t[:, 6].contiguous(), t[:, 7].contiguous(), mu=mu)
        del t
        assert res["status"].shape[0] == 1 << 25
        for k in ref:
            r = torch.from_numpy(ref[k]).cuda()
            v = res[k].view(reps, len(base), *ref[k].shape[1:])
            if v.dtype == torch.float32:
                v, r = v.view(torch.int32), r.view(torch.int32)
            assert bool((v == r.unsqueeze(0)).all()), k
    finally:
        gpu.close(); cpu.close()


def test_cast_entries_refuse_bad_arguments():
    import torch
    p = DenseSLAMPipeline((64, 48), 256, DIM, field_type=SDF)
    lib = p.lib
    try:
        rays = np.tile(np.float32([1, 1, 1, 0, 0, 1, 0.4, 4]), (4, 1))
        st_h = np.zeros(4, np.uint8)
        dev_rays = torch.from_numpy(rays).cuda()
        st_d = torch.zeros(4, dtype=torch.uint8, device="cuda")
        none = _RayOut(None, None, None)
        for fn, ra, sa in ((lib.se_hip_cast_rays_host, rays.ctypes.data, st_h.ctypes.data), (lib.se_hip_cast_rays, dev_rays.data_ptr(), st_d.data_ptr())):
            good = _RayOut(None, None, sa)
            for args in ((ra, -1, 0.1, C.byref(good)), (None, 4, 0.1, C.byref(good)), (ra, 4, 0.1, C.byref(none)), (ra, 4, 0.1, None),
                         (ra, 4, 0.0, C.byref(good)), (ra, 4, -0.1, C.byref(good)), (ra, 4, float("nan"), C.byref(good)), (ra, 4, float("inf"), C.byref(good))):
                assert fn(p._h, *args) == -1, args
                assert lib.se_hip_last_error().decode()
            assert fn(p._h, ra, 0, 0.1, C.byref(good)) == 0
            assert fn(p._h, None, 0, 0.1, C.byref(good)) == 0
            assert fn(p._h, ra, 4, 0.1, C.byref(good)) == 0
        p.sync()
        assert (st_h == 1).all() and (st_d.cpu().numpy() == 1).all()        # valid rays through an empty map
        assert lib.se_hip_cast_rays_host(None, rays.ctypes.data, 4, 0.1, C.byref(_RayOut(None, None, st_h.ctypes.data))) == -1
        empty = p.cast_rays(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), mu=0.1)
        assert all(v.shape[0] == 0 for v in empty.values())
    finally:
        p.close()
