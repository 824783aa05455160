"""Motion collision queries, host side (no GPU): the header declares both entries, the output struct and the constant, the build lists the
kernel header, the Python wrapper refuses bad input before it calls the library, the host restatement (include/se/motion_collision.hpp) gives
the hand-worked answers, and its traversal equals the literal definition on random maps of both fields."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests.host_util import bare_pipeline, build_kats
from tests.motion_util import HAND_CASES, HAND_MAPS, INVALID, as_float32, motion_truth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_motion_entries():
    h = open(os.path.join(ROOT, "include", "se_hip.h")).read()
    flat = re.sub(r"\s+", " ", h)
    assert ("int se_hip_collide_motions(se_hip_pipeline* p, const int32_t* device_motions, int64_t n, const se_hip_collide_test* test, int32_t stop_at, "
            "const se_hip_motion_out* device_out);") in flat
    assert ("int se_hip_collide_motions_host(se_hip_pipeline* p, const int32_t* host_motions, int64_t n, const se_hip_collide_test* test, int32_t stop_at, "
            "const se_hip_motion_out* host_out);") in flat
    body = re.search(r"typedef struct se_hip_motion_out \{(.*?)\} se_hip_motion_out;", h, re.S).group(1)
    assert re.findall(r"(uint8_t|float)\* (\w+);", body) == [("uint8_t", "status"), ("float", "t_first")]
    assert "#define SE_HIP_MOTION_FREE 2.0f" in h
    assert "2^20" in h and "int64" in h              # the bound of a valid motion and its reason are stated
    assert "#define SE_HIP_K_COUNT 5" in h           # no new launch counter
    from supereight_amd import pipeline as P
    assert P.MOTION_FREE == 2.0 and P._MOTION_STOPS == {"occupied": P.COLLISION_OCCUPIED, "unseen": P.COLLISION_UNSEEN}
    assert [f[0] for f in P._MotionOut._fields_] == ["status", "t_first"]
    for name in ("se_hip_collide_motions", "se_hip_collide_motions_host"):
        res, args = P.EXPORTS[name]
        assert res is C.c_int and len(args) == 6 and args[2] is C.c_int64 and args[4] is C.c_int32


def test_build_lists_the_motion_kernel_header():
    from supereight_amd import build
    assert "se_motion_kernels.h" in build.HEADERS
    src = open(os.path.join(ROOT, "supereight_amd", "csrc", "se_hip_api.hip")).read()
    assert '#include "se_motion_kernels.h"' in src
    k = open(os.path.join(ROOT, "supereight_amd", "csrc", "se_motion_kernels.h")).read()
    assert "k_collide_motions" in k and "bounded" in k          # the header comment states why every loop ends


def _pipeline():
    return bare_pipeline(field=0)


@pytest.mark.parametrize("motions,exc", [
    (np.zeros((4, 9), np.int64), TypeError),
    (np.zeros((4, 9), np.float32), TypeError),
    (np.zeros((4, 6), np.int32), ValueError),
    (np.zeros(36, np.int32), ValueError),
    (np.zeros((2, 2, 9), np.int32), ValueError),
    ([[0, 0, 0, 1, 1, 1, 0, 0, 0]], TypeError),
    (None, TypeError),
], ids=["int64", "float32", "n_by_6", "flat", "3d", "list", "none"])
def test_collides_moving_refuses_bad_motions_before_any_library_call(motions, exc):
    with pytest.raises(exc):
        _pipeline().collides_moving(motions)


def test_collides_moving_refuses_bad_arguments_before_any_library_call():
    p = _pipeline()
    ok = np.zeros((4, 9), np.int32)
    with pytest.raises(ValueError):
        p.collides_moving(ok, stop_at="empty")
    with pytest.raises(ValueError):
        p.collides_moving(ok, stop_at=0)
    with pytest.raises(ValueError):
        p.collides_moving(ok, threshold=float("nan"))
    with pytest.raises(ValueError):
        p.collides_moving(ok, threshold=float("inf"))
    with pytest.raises(ValueError):
        p.collides_moving(ok, threshold=1e39)           # not finite as a float32
    with pytest.raises(TypeError):
        p.collides_moving(ok, occupied_above=2)
    with pytest.raises(TypeError):
        p.collides_moving(ok, occupied_above="yes")


def test_collides_moving_refuses_bad_torch_motions():
    torch = pytest.importorskip("torch")
    p = _pipeline()
    with pytest.raises(TypeError):
        p.collides_moving(torch.zeros((4, 9), dtype=torch.int64))
    with pytest.raises(ValueError):
        p.collides_moving(torch.zeros((4, 8), dtype=torch.int32))
    with pytest.raises(ValueError):
        p.collides_moving(torch.zeros((9, 4), dtype=torch.int32).t())          # [4, 9], not contiguous
    with pytest.raises(ValueError):
        p.collides_moving(torch.zeros((4, 9), dtype=torch.int32))              # a CPU tensor: the device entry reads device memory


def _parse(stdout):
    got = {}
    for f in (line.split() for line in stdout.splitlines()):
        v = [int(t) for t in f[1:]]
        got[f[0]] = (v[0], (v[1], Fraction(v[2], v[3])), (v[4], Fraction(v[5], v[6])), (v[2], v[3], v[5], v[6]))
    return got


def test_hand_cases_on_the_host_mirror(tmp_path):
    """The program itself ends with 1 if the traversal and the brute-force definition differ on a case, or a d = 0 motion from the strict box."""
    exe = build_kats("motion_kats", tmp_path)
    r = subprocess.run([exe, "kats"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = _parse(r.stdout)
    assert sorted(got) == sorted(HAND_CASES)
    for name, (_, _, _, _, occ, uns) in HAND_CASES.items():
        valid, g_occ, g_uns, terms = got[name]
        assert valid == (occ[0] != INVALID), name
        assert g_occ == occ and g_uns == uns, (name, g_occ, g_uns)
        # lowest terms, as the header promises
        assert terms == (occ[1].numerator, occ[1].denominator, uns[1].numerator, uns[1].denominator), name
    assert as_float32(HAND_CASES["Diagonal3"][4][1]) == np.float32(0.45) and as_float32(HAND_CASES["DiagonalTouches"][4][1]) == np.float32(0.5)


def test_numpy_truth_gives_the_hand_answers():
    """The numpy statement of the definition that the GPU tests use as truth (tests/motion_util.py) on the same cases."""
    grids = {}
    for name, spec in HAND_MAPS.items():
        g = np.full((64, 64, 64), 2, np.uint8)
        for x, y, z in spec.get("occupied", []):
            g[z, y, x] = 0
        if "wall" in spec:
            g[:, :, spec["wall"]] = 0
        if "gap" in spec:
            x0, y0, z0, x1, y1, z1 = spec["gap"]
            g[z0:z1, y0:y1, x0:x1] = 1
        grids[name] = g
    for name, (mp, lo, side, d, occ, uns) in HAND_CASES.items():
        st, t_occ, t_uns = motion_truth(grids[mp], list(lo) + list(side) + list(d))
        assert (st, t_occ) == occ and (st, t_uns) == uns, name


def test_traversal_equals_the_definition_on_random_maps(tmp_path):
    exe = build_kats("motion_kats", tmp_path)
    r = subprocess.run([exe, "random", "26", "7"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout
    f = r.stdout.split()
    assert f[0] == "checked" and int(f[1]) == 10400 and f[2] == "mismatches" and int(f[3]) == 0


def test_cpp_mirror_motion_program_compiles(tmp_path):
    """tests/cpp/motion_mirror.cpp (run on the GPU by test_gpu_motion_mirror.py) compiles against the headers for both field types."""
    for tag in ("SDF", "OFusion"):
        obj = str(tmp_path / f"mm_{tag}.o")
        r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-ffp-contract=off", f"-DSE_FIELD_TYPE={tag}", "-I" + os.path.join(ROOT, "include"),
                            "-c", os.path.join(ROOT, "tests", "cpp", "motion_mirror.cpp"), "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
