"""Clearance queries, host side (no GPU): the header declares both entries, the output struct and the constants, the build lists the kernel
header, the Python wrapper refuses bad input before it calls the library, the host restatement (include/se/clearance.hpp) gives the
hand-worked answers, and its pruned traversal equals the literal definition on random maps of both fields."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.clearance_util import CLEAR_MAPS, HAND_CASES, INVALID, NONE, NOWHERE, OCC, UNSEEN, clearance_truth, d2_of, hand_grid
from tests.host_util import bare_pipeline, build_kats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_clearance_entries():
    h = open(os.path.join(ROOT, "include", "se_hip.h")).read()
    flat = re.sub(r"\s+", " ", h)
    assert ("int se_hip_clearance_boxes(se_hip_pipeline* p, const int32_t* device_queries, int64_t n, const se_hip_collide_test* test, int32_t stop_at, "
            "const se_hip_clearance_out* device_out);") in flat
    assert ("int se_hip_clearance_boxes_host(se_hip_pipeline* p, const int32_t* host_queries, int64_t n, const se_hip_collide_test* test, int32_t stop_at, "
            "const se_hip_clearance_out* host_out);") in flat
    body = re.search(r"typedef struct se_hip_clearance_out \{(.*?)\} se_hip_clearance_out;", h, re.S).group(1)
    assert re.findall(r"(int32_t)\* (\w+);", body) == [("int32_t", "d2"), ("int32_t", "nearest")]
    assert "#define SE_HIP_CLEARANCE_NONE (-1)" in h and "#define SE_HIP_CLEARANCE_INVALID (-2)" in h
    assert "2^19" in h and "32767" in h and "(z, y, x)" in h     # the bounds of a valid query and the tie-break are stated
    assert "#define SE_HIP_K_COUNT 5" in h                       # no new launch counter
    from supereight_amd import pipeline as P
    assert P.CLEARANCE_NONE == NONE and P.CLEARANCE_INVALID == INVALID
    assert [f[0] for f in P._ClearanceOut._fields_] == ["d2", "nearest"]
    for name in ("se_hip_clearance_boxes", "se_hip_clearance_boxes_host"):
        res, args = P.EXPORTS[name]
        assert res is C.c_int and len(args) == 6 and args[2] is C.c_int64 and args[4] is C.c_int32
    mirror = open(os.path.join(ROOT, "include", "se", "DenseSLAMSystem.h")).read()
    assert "bool clearanceOf(const int32_t* host_queries, size_t n, const se_hip_collide_test& test, int32_t stop_at, se_hip_clearance_out& host_out)" in mirror


def test_build_lists_the_clearance_kernel_header():
    from supereight_amd import build
    assert "se_clearance_kernels.h" in build.HEADERS
    src = open(os.path.join(ROOT, "supereight_amd", "csrc", "se_hip_api.hip")).read()
    assert '#include "se_clearance_kernels.h"' in src
    k = open(os.path.join(ROOT, "supereight_amd", "csrc", "se_clearance_kernels.h")).read()
    assert "k_clearance_boxes" in k and "bounded" in k          # the header comment states why every loop ends


def _pipeline():
    return bare_pipeline(field=0, _device=0)


@pytest.mark.parametrize("boxes,exc", [
    (np.zeros((4, 6), np.int64), TypeError),
    (np.zeros((4, 6), np.float32), TypeError),
    (np.zeros((4, 7), np.int32), ValueError),
    (np.zeros(24, np.int32), ValueError),
    (np.zeros((2, 2, 6), np.int32), ValueError),
    ([[0, 0, 0, 1, 1, 1]], TypeError),
    (None, TypeError),
], ids=["int64", "float32", "n_by_7", "flat", "3d", "list", "none"])
def test_clearance_refuses_bad_boxes_before_any_library_call(boxes, exc):
    with pytest.raises(exc):
        _pipeline().clearance(boxes, 4)


@pytest.mark.parametrize("r_max,exc", [
    (4.0, TypeError),
    (np.full(4, 4.0, np.float32), TypeError),
    (True, TypeError),
    ("4", TypeError),
    (None, TypeError),
    (np.zeros(3, np.int32), ValueError),
    (np.zeros((4, 1), np.int32), ValueError),
    (np.zeros((2, 2), np.int64), ValueError),
], ids=["float", "float_array", "bool", "str", "none", "three_for_four", "n_by_1", "2d"])
def test_clearance_refuses_bad_r_max_before_any_library_call(r_max, exc):
    with pytest.raises(exc):
        _pipeline().clearance(np.zeros((4, 6), np.int32), r_max)


def test_clearance_refuses_bad_arguments_before_any_library_call():
    p = _pipeline()
    ok = np.zeros((4, 6), np.int32)
    with pytest.raises(ValueError):
        p.clearance(ok, 4, stop_at="empty")
    with pytest.raises(ValueError):
        p.clearance(ok, 4, stop_at=0)
    with pytest.raises(ValueError):
        p.clearance(ok, 4, threshold=float("nan"))
    with pytest.raises(ValueError):
        p.clearance(ok, 4, threshold=float("inf"))
    with pytest.raises(ValueError):
        p.clearance(ok, 4, threshold=1e39)           # not finite as a float32
    with pytest.raises(TypeError):
        p.clearance(ok, 4, occupied_above=2)
    with pytest.raises(TypeError):
        p.clearance(ok, 4, occupied_above="yes")


class _Recorder:
    """Stands in for libse_hip.so where a test wants to see what the wrapper passes: keeps the queries of the host entry."""
    def __init__(self):
        self.queries, self.stop, self.nearest = None, None, None

    def se_hip_clearance_boxes_host(self, h, queries, n, test, stop_at, out):
        self.queries = np.ctypeslib.as_array(C.cast(queries, C.POINTER(C.c_int32)), (n, 7)).copy() if n else np.zeros((0, 7), np.int32)
        self.stop, self.nearest = stop_at, bool(out._obj.nearest)
        return 0


def test_clearance_broadcasts_r_max_into_the_seventh_column():
    p = _pipeline()
    p.lib = _Recorder()
    boxes = np.arange(24, dtype=np.int32).reshape(4, 6)
    d2, near = p.clearance(boxes, 9)
    assert d2.shape == (4,) and d2.dtype == np.int32 and near.shape == (4, 3) and near.dtype == np.int32
    assert (p.lib.queries[:, :6] == boxes).all() and (p.lib.queries[:, 6] == 9).all() and p.lib.stop == 0 and p.lib.nearest
    for r in (np.array([1, 2, 3, 4], np.int64), np.array([1, 2, 3, 4], np.uint8), np.array([1, 2, 3, 4], np.int32)):
        alone = p.clearance(boxes[:, ::1], r, stop_at="unseen", nearest=False)
        assert alone.shape == (4,) and (p.lib.queries[:, 6] == [1, 2, 3, 4]).all() and p.lib.stop == 1 and not p.lib.nearest
    # what does not fit the int32 column stays invalid: negative -> -1, beyond 32767 -> 32768
    p.clearance(boxes, np.array([-5, 32767, 32768, 2 ** 40], np.int64))
    assert p.lib.queries[:, 6].tolist() == [-1, 32767, 32768, 32768]
    p.clearance(boxes, np.int16(7))
    assert (p.lib.queries[:, 6] == 7).all()
    empty = p.clearance(np.zeros((0, 6), np.int32), 3)
    assert empty[0].shape == (0,) and empty[1].shape == (0, 3) and empty[0].dtype == np.int32


def test_clearance_refuses_bad_torch_boxes():
    torch = pytest.importorskip("torch")
    p = _pipeline()
    with pytest.raises(TypeError):
        p.clearance(torch.zeros((4, 6), dtype=torch.int64), 4)
    with pytest.raises(ValueError):
        p.clearance(torch.zeros((4, 7), dtype=torch.int32), 4)
    with pytest.raises(ValueError):
        p.clearance(torch.zeros((6, 4), dtype=torch.int32).t(), 4)          # [4, 6], not contiguous
    with pytest.raises(ValueError):
        p.clearance(torch.zeros((4, 6), dtype=torch.int32), 4)              # a CPU tensor: the device entry reads device memory


def _parse(stdout):
    got = {}
    for f in (line.split() for line in stdout.splitlines()):
        v = [int(t) for t in f[1:]]
        got[f[0]] = ((v[0], tuple(v[1:4])), (v[4], tuple(v[5:8])))
    return got


def test_hand_cases_on_the_host_mirror(tmp_path):
    """The program itself ends with 1 if the traversal and the brute-force definition differ on a case."""
    exe = build_kats("clearance_kats", tmp_path)
    r = subprocess.run([exe, "kats"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = _parse(r.stdout)
    assert sorted(got) == sorted(HAND_CASES)
    for name, (_, _, _, _, occ, uns) in HAND_CASES.items():
        assert got[name] == (occ, uns), (name, got[name])
    # the cases the definition of the feature names
    assert HAND_CASES["CornerR15"][4] == (NONE, NOWHERE) and HAND_CASES["CornerR16"][4] == (243, (10, 10, 10))
    assert HAND_CASES["WallTie"][4] == (64, (20, 4, 4))
    assert HAND_CASES["FreeR30"][4][0] == NONE and HAND_CASES["FreeR30"][5] == (900, (29, 29, -1)) and HAND_CASES["FreeR29"][5][0] == NONE
    assert HAND_CASES["GapBox"][5] == (9, (9, 2, -1)) and HAND_CASES["GapBox"][4] == (841, (40, 3, 3))
    assert {c[0] for c in HAND_CASES.values()} == set(CLEAR_MAPS)


def test_numpy_truth_gives_the_hand_answers():
    """The numpy statement of the definition that the GPU tests use as truth (tests/clearance_util.py) on the same cases (but the one whose
    r_max makes the dilated box 65 536 voxels wide)."""
    grids = {name: hand_grid(name) for name in CLEAR_MAPS}
    checked = 0
    for name, (mp, lo, side, r_max, occ, uns) in HAND_CASES.items():
        if 64 < r_max <= 32767:
            continue
        q = list(lo) + list(side) + [r_max]
        for stop, exp in ((OCC, occ), (UNSEEN, uns)):
            d2, near, count = clearance_truth(grids[mp], q, stop)
            assert (d2, near) == exp, (name, stop, d2, near)
            if d2 >= 0:
                assert count >= 1 and d2_of(np.array([q[:6]]), np.array([near]))[0] == d2
        checked += 1
    assert checked == len(HAND_CASES) - 1
    assert clearance_truth(grids["wall"], [10, 5, 5, 2, 2, 2, 10], OCC)[2] == 16          # the tie: y, z in [4, 7]


def test_traversal_equals_the_definition_on_random_maps(tmp_path):
    exe = build_kats("clearance_kats", tmp_path)
    r = subprocess.run([exe, "random", "52", "7"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout
    f = r.stdout.split()
    assert f[0] == "sdf" and int(f[1]) >= 10000 and f[2] == "ofusion" and int(f[3]) >= 10000
    assert f[4] == "mismatches" and int(f[5]) == 0
    assert f[6] == "ties" and int(f[7]) > 1000


def test_cpp_mirror_clearance_program_compiles(tmp_path):
    """tests/cpp/clearance_mirror.cpp (run on the GPU by test_gpu_clearance_mirror.py) compiles against the headers for both field types."""
    for tag in ("SDF", "OFusion"):
        obj = str(tmp_path / f"cm_{tag}.o")
        r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-ffp-contract=off", f"-DSE_FIELD_TYPE={tag}", "-I" + os.path.join(ROOT, "include"),
                            "-c", os.path.join(ROOT, "tests", "cpp", "clearance_mirror.cpp"), "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
