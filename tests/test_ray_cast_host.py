"""Batched ray casts, host side (no GPU).  The CPU helper tests/cpp/ray_cast_oracle.cpp against the oracle's own camera raycast: the rays of
raycastKernel (rco_camera_rays) cast one by one through rco_cast_rays give so_pipe_raycast's vertex and normal images bit for bit, for SDF and
OFusion, stream poses and cameras outside every face, at ragged shapes.  This pins the helper -- the reference the GPU tests hold
se_hip_cast_rays to -- to the camera raycast that the parity tests already pin.  Plus the header, the wrapper's refusals before any library
call, and the C++ mirror program compiling against the header."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle.binding import OFUSION, SDF
from supereight_amd.synthetic import make_stream
from tests import ray_cast_util as U
from tests.edge_frames import SHAPE_CASES, edge_stream
from tests.host_util import bare_pipeline
from tests.parity_util import OUTSIDE_VIEWS, outside_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _integrate(lib, field, W, H, N, dim, mu, frames, stream):
    cpu = U.oracle_pipeline(lib, field, N, dim, W, H)
    for f in range(frames):
        cpu.integrate(stream.depth(f), stream.pose(f), stream.k, mu, f)
    return cpu


def _check_camera(lib, cpu, pose, k, W, H, mu, frame):
    ran, v, n = cpu.raycast(pose, k, mu, frame)
    assert ran
    res, trips = U.cast_rays(lib, cpu.h, U.camera_rays(lib, pose, k, W, H), mu)
    assert trips < 4096
    hit = (res["status"] & 4) != 0
    assert U.bits_equal(np.where(hit[:, None], res["hit"][:, :3], 0).astype(np.float32), v.reshape(-1, 3)), "vertex image"
    assert U.bits_equal(res["normal"], n.reshape(-1, 3)), "normal image"
    # the status bits say what the outputs show
    st = res["status"]
    assert (st & 1).all()
    assert ((st & 4) != 0).tolist() == (res["hit"][:, 3] > 0).tolist()
    assert not ((st & 4) & ~((st & 2) << 1)).any()     # a hit implies the march ran
    assert ((st & 8) != 0).tolist() == (((st & 4) != 0) & (res["normal"][:, 0] != -2)).tolist()
    return int(hit.sum())


@pytest.mark.parametrize("field,mu", [(SDF, 0.1), (OFUSION, 0.02)], ids=["sdf", "ofusion"])
def test_camera_rays_reproduce_the_camera_raycast(field, mu):
    lib = U.load()
    W, H, N, dim, frames = 160, 120, 256, 4.8, 5
    s = make_stream("room", W, H, dim, holes=False)
    cpu = _integrate(lib, field, W, H, N, dim, mu, frames, s)
    hits = 0
    poses = [s.pose(f) for f in range(frames)] + [outside_view(name, 0.05, dim) for name in OUTSIDE_VIEWS]
    for i, pose in enumerate(poses):
        hits += _check_camera(lib, cpu, pose, s.k, W, H, mu, frames + i)
    assert hits > 20000
    cpu.close()


SMALL_SHAPES = [c for c in SHAPE_CASES if not c["name"].startswith("large_")]


@pytest.mark.parametrize("case", SMALL_SHAPES, ids=[c["name"] for c in SMALL_SHAPES])
def test_camera_rays_at_ragged_shapes(case):
    lib = U.load()
    s = edge_stream(case)
    W, H = case["W"], case["H"]
    cpu = _integrate(lib, case["field"], W, H, case["N"], case["dim"], case["mu"], case["frames"], s)
    hits = _check_camera(lib, cpu, s.pose(case["frames"] - 1), s.k, W, H, case["mu"], case["frames"])
    hits += _check_camera(lib, cpu, outside_view("+z_tilted", 0.02, case["dim"]), s.k, W, H, case["mu"], case["frames"])
    assert hits > 0
    cpu.close()


def test_invalid_rays_on_the_helper():
    lib = U.load()
    W, H, N, dim = 80, 60, 256, 4.8
    s = make_stream("room", W, H, dim, holes=False)
    cpu = _integrate(lib, SDF, W, H, N, dim, 0.1, 3, s)
    good = U.camera_rays(lib, s.pose(2), s.k, W, H)[::7]
    bad = np.repeat(good[:1], 4, axis=0)
    bad[0, 0] = np.nan
    bad[1, 7] = np.inf
    bad[2, 3:6] *= 1.2
    bad[3, 1] = 2.0 ** 20 * dim / N
    res, _ = U.cast_rays(lib, cpu.h, bad, 0.1)
    assert (res["status"] == 0).all() and (res["hit"] == 0).all()
    assert (res["normal"] == np.float32([-2, 0, 0])).all()
    cpu.close()


def test_header_declares_the_ray_entries():
    h = open(os.path.join(ROOT, "include", "se_hip.h")).read()
    assert re.search(r"int se_hip_cast_rays\(se_hip_pipeline\* p, const float\* device_rays, int64_t n, float mu, const se_hip_ray_out\* device_out\);", h)
    assert re.search(r"int se_hip_cast_rays_host\(se_hip_pipeline\* p, const float\* host_rays, int64_t n, float mu, const se_hip_ray_out\* host_out\);", h)
    body = re.search(r"typedef struct se_hip_ray_out \{(.*?)\} se_hip_ray_out;", h, re.S).group(1)
    fields = re.findall(r"(float|uint8_t)\* (\w+);", body)
    assert fields == [("float", "hit"), ("float", "normal"), ("uint8_t", "status")]
    assert "#define SE_HIP_K_COUNT 5" in h
    from supereight_amd.pipeline import EXPORTS, _RayOut
    assert [f[0] for f in _RayOut._fields_] == [f[1] for f in fields]
    for name in ("se_hip_cast_rays", "se_hip_cast_rays_host"):
        res, args = EXPORTS[name]
        assert res is C.c_int and args[2] is C.c_int64 and args[3] is C.c_float and len(args) == 5


def _pipeline():
    return bare_pipeline(_device=None)


O = np.zeros((4, 3), np.float32)
D = np.tile(np.float32([0, 0, 1]), (4, 1))


@pytest.mark.parametrize("kw,exc", [
    (dict(origins=O.astype(np.float64)), TypeError),
    (dict(directions=D[:, :2].copy()), ValueError),
    (dict(directions=D[:3].copy()), ValueError),
    (dict(origins=O.tolist()), TypeError),
    (dict(near=np.zeros(3, np.float32)), ValueError),
    (dict(far=np.zeros((4, 1), np.float32)), ValueError),
    (dict(mu=0.0), ValueError),
    (dict(mu=float("nan")), ValueError),
    (dict(hit=False, normal=False, status=False), ValueError),
], ids=["float64", "n_by_2", "count", "list", "near_shape", "far_shape", "mu_zero", "mu_nan", "no_output"])
def test_cast_rays_refuses_bad_input_before_any_library_call(kw, exc):
    args = dict(origins=O, directions=D, mu=0.1)
    args.update(kw)
    with pytest.raises(exc):
        _pipeline().cast_rays(**args)


def test_cast_rays_refuses_cpu_torch_tensors():
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError):
        _pipeline().cast_rays(torch.zeros((4, 3)), torch.zeros((4, 3)), mu=0.1)    # CPU tensors: the device entry reads device memory
    with pytest.raises(TypeError):
        _pipeline().cast_rays(torch.zeros((4, 3)), D, mu=0.1)


def test_cpp_mirror_ray_program_compiles(tmp_path):
    for tag in ("SDF", "OFusion"):
        r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-ffp-contract=off", f"-DSE_FIELD_TYPE={tag}", "-I" + os.path.join(ROOT, "include"),
                            "-c", os.path.join(ROOT, "tests", "cpp", "ray_cast_mirror.cpp"), "-o", str(tmp_path / f"rc_{tag}.o")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
