"""The distance field, host side (no GPU): the header declares both entries and the structs, the build lists the kernel header, the host
restatement (include/se/distance_field.hpp) gives the hand-worked answers, its three passes equal the literal definition and the clearance
traversal on random maps of both fields, the numpy truth of the GPU tests gives the same hand answers, and the Python wrapper refuses every
request the C entry refuses before it calls the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.clearance_util import NONE, NOWHERE, OCC, UNSEEN, hand_grid
from tests.field_util import HAND_CASES, LIMIT, field_truth, valid
from tests.host_util import bare_pipeline, build_kats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_field_entries():
    h = open(os.path.join(ROOT, "include", "se_hip.h")).read()
    flat = re.sub(r"\s+", " ", h)
    assert ("int se_hip_distance_field(se_hip_pipeline* p, const se_hip_field_request* request, const se_hip_collide_test* test, "
            "const se_hip_field_out* device_out);") in flat
    assert ("int se_hip_distance_field_host(se_hip_pipeline* p, const se_hip_field_request* request, const se_hip_collide_test* test, "
            "const se_hip_field_out* host_out);") in flat
    body = re.search(r"typedef struct se_hip_field_request \{(.*?)\} se_hip_field_request;", h, re.S).group(1)
    assert re.findall(r"int32_t (\w+)(?:\[3\])?;", body) == ["lo", "side", "robot", "r_max", "stop_at"]
    body = re.search(r"typedef struct se_hip_field_out \{(.*?)\} se_hip_field_out;", h, re.S).group(1)
    assert re.findall(r"int32_t\* (\w+);", body) == ["d2", "nearest"]
    text = re.sub(r"\s*\n \*\s*", " ", h)                                                       # the comment's lines joined
    assert "2^24" in text and "2^28" in text and "side[k] + robot[k] + 2 r_max + 1" in text      # the bounds, the work buffer's among them
    assert "growing it waits for the work enqueued before" in text                                # the one exception to "asynchronous"
    assert "#define SE_HIP_K_COUNT 5" in h                                                        # no new launch counter
    from supereight_amd import pipeline as P
    assert [f[0] for f in P._FieldRequest._fields_] == ["lo", "side", "robot", "r_max", "stop_at"] and C.sizeof(P._FieldRequest) == 44
    assert [f[0] for f in P._FieldOut._fields_] == ["d2", "nearest"]
    for name in ("se_hip_distance_field", "se_hip_distance_field_host"):
        res, args = P.EXPORTS[name]
        assert res is C.c_int and len(args) == 4
    mirror = open(os.path.join(ROOT, "include", "se", "DenseSLAMSystem.h")).read()
    assert "bool distanceField(const se_hip_field_request& request, const se_hip_collide_test& test, se_hip_field_out& host_out)" in mirror


def test_build_lists_the_field_kernel_header():
    from supereight_amd import build
    assert "se_field_kernels.h" in build.HEADERS
    src = open(os.path.join(ROOT, "supereight_amd", "csrc", "se_hip_api.hip")).read()
    assert '#include "se_field_kernels.h"' in src
    k = open(os.path.join(ROOT, "supereight_amd", "csrc", "se_field_kernels.h")).read()
    for name in ("k_field_classify", "k_field_x", "k_field_y", "k_field_z"):
        assert name in k
    assert "bounded by the request" in k and "atomic" not in k.split("#pragma once")[1]          # why every loop ends; no atomics in the code


def _parse(stdout):
    got = {}
    for f in (line.split() for line in stdout.splitlines()):
        if f[1] == "invalid":
            got[f[0]] = None
            continue
        v = [int(t) for t in f[1:]]
        got.setdefault(f[0], ([], []))
        got[f[0]][0].append((v[0], tuple(v[1:4])))
        got[f[0]][1].append((v[4], tuple(v[5:8])))
    return got


@pytest.fixture(scope="module")
def kats(tmp_path_factory):
    return build_kats("field_kats", tmp_path_factory.mktemp("field_kats"))


def test_hand_cases_on_the_host_mirror(kats):
    """The program itself ends with 1 if the definition, the three passes and the clearance traversal differ on a case."""
    r = subprocess.run([kats, "kats"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = _parse(r.stdout)
    assert sorted(got) == sorted(HAND_CASES)
    for name, (_, lo, side, robot, r_max, occ, uns) in HAND_CASES.items():
        if occ is None:
            assert got[name] is None and not valid(lo, side, robot, r_max), name
        else:
            assert got[name] == (occ, uns), (name, got[name])
            assert valid(lo, side, robot, r_max) and len(occ) == side[0] * side[1] * side[2]
    assert HAND_CASES["CornerR15"][5] == [(NONE, NOWHERE)] and HAND_CASES["CornerR16"][5] == [(243, (10, 10, 10))]


def test_numpy_truth_gives_the_hand_answers():
    """field_truth (clearance_truth per voxel: what the GPU tests use as truth) on the same cases."""
    checked = 0
    for name, (mp, lo, side, robot, r_max, occ, uns) in HAND_CASES.items():
        if occ is None:
            continue
        for stop, exp in ((OCC, occ), (UNSEEN, uns)):
            d2, near, _ = field_truth(hand_grid(mp), (lo, side, robot, r_max), stop)
            assert d2.shape == (side[2], side[1], side[0]) and near.shape == d2.shape + (3,) and d2.dtype == np.int32
            assert [(int(d), tuple(w.tolist())) for d, w in zip(d2.reshape(-1), near.reshape(-1, 3))] == exp, (name, stop)
        checked += 1
    assert checked == 9
    d2, near, ties = field_truth(hand_grid("wall"), ((10, 5, 5), (2, 1, 1), (2, 2, 2), 10), OCC, only=[1])
    assert d2.tolist() == [49] and near.tolist() == [[20, 4, 4]] and ties.tolist() == [True]


def test_three_passes_equal_the_definition_on_random_maps(kats):
    r = subprocess.run([kats, "random", "80", "7"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout
    f = r.stdout.split()
    assert f[0] == "sdf" and int(f[1]) >= 2000 and f[2] == "ofusion" and int(f[3]) >= 2000
    assert f[4] == "voxels" and int(f[5]) > 50000 and f[6] == "none" and 0 < int(f[7]) < int(f[5])
    assert f[8] == "mismatches" and int(f[9]) == 0
    assert f[10] == "ties" and int(f[11]) > 100


def test_cpp_mirror_field_program_compiles(tmp_path):
    """tests/cpp/field_mirror.cpp (run on the GPU by test_gpu_field_mirror.py) compiles against the headers for both field types."""
    for tag in ("SDF", "OFusion"):
        obj = str(tmp_path / f"fm_{tag}.o")
        r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-ffp-contract=off", f"-DSE_FIELD_TYPE={tag}", "-I" + os.path.join(ROOT, "include"),
                            "-c", os.path.join(ROOT, "tests", "cpp", "field_mirror.cpp"), "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def _pipeline():
    return bare_pipeline(field=0, _device=0)


OK = dict(lo=(0, 0, 0), side=(4, 4, 4), r_max=4)

# every refusal of the C entry that a Python caller can express, one case each
REFUSED = {
    "side_zero": dict(side=(4, 0, 4)),
    "robot_zero": dict(robot=(1, 1, 0)),
    "robot_257": dict(robot=(257, 1, 1)),
    "r_max_negative": dict(r_max=-1),
    "r_max_256": dict(r_max=256),
    "lo_below_limit": dict(lo=(-LIMIT - 1, 0, 0)),
    "lo_above_limit": dict(lo=(0, LIMIT + 1, 0)),
    "end_above_limit": dict(lo=(0, 0, LIMIT - 5), side=(4, 4, 4), robot=(1, 1, 2)),
    "voxels_above_2_24": dict(side=(256, 256, 257), r_max=0),
    "work_above_2_28": dict(side=(1025, 2, 2), r_max=254),
    "stop_at_empty": dict(stop_at="empty"),
    "stop_at_int": dict(stop_at=0),
    "threshold_nan": dict(threshold=float("nan")),
    "threshold_inf": dict(threshold=float("inf")),
    "threshold_beyond_float32": dict(threshold=1e39),
}
WRONG_TYPE = {
    "occupied_above_int": dict(occupied_above=2),
    "occupied_above_str": dict(occupied_above="yes"),
    "r_max_float": dict(r_max=4.0),
    "r_max_bool": dict(r_max=True),
    "lo_float": dict(lo=(0.0, 0.0, 0.0)),
    "side_none": dict(side=None),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_distance_field_refuses_before_any_library_call(name):
    with pytest.raises(ValueError):
        _pipeline().distance_field(**{**OK, **REFUSED[name]})


@pytest.mark.parametrize("name", sorted(WRONG_TYPE))
def test_distance_field_refuses_wrong_types_before_any_library_call(name):
    with pytest.raises(TypeError):
        _pipeline().distance_field(**{**OK, **WRONG_TYPE[name]})


def test_distance_field_refuses_wrong_shapes():
    for kw in (dict(lo=(0, 0)), dict(side=(4, 4, 4, 4)), dict(robot=2), dict(lo=[[0, 0, 0]])):
        with pytest.raises(ValueError):
            _pipeline().distance_field(**{**OK, **kw})


class _Recorder:
    """Stands in for libse_hip.so where a test wants to see what the wrapper passes: keeps the request of the host entry."""
    def __init__(self):
        self.rq, self.test, self.nearest = None, None, None

    def se_hip_distance_field_host(self, h, rq, test, out):
        r, t = rq._obj, test._obj
        self.rq = (tuple(r.lo), tuple(r.side), tuple(r.robot), r.r_max, r.stop_at)
        self.test, self.nearest = (t.threshold, t.occupied_above), bool(out._obj.nearest)
        return 0


def test_the_bounds_themselves_pass_the_check():
    """A side product of exactly 2^24, a work buffer of exactly 2^28 entries, r_max 255, a robot of 256 and coordinates on +-2^19 reach the
    library (here: a recorder in its place)."""
    p = _pipeline()
    p.lib = _Recorder()
    d2 = p.distance_field((0, 0, 0), (256, 256, 256), 0)
    assert d2.shape == (256, 256, 256) and d2.dtype == np.int32 and p.lib.rq == ((0, 0, 0), (256, 256, 256), (1, 1, 1), 0, 0) and not p.lib.nearest
    assert valid((0, 0, 0), (256, 256, 256), (1, 1, 1), 0) and not valid((0, 0, 0), (256, 256, 257), (1, 1, 1), 0)
    # side[0] * D1 * D2 = 1024 * 512 * 512 = 2^28: D = side + robot + 2 r_max + 1 = 2 + 1 + 508 + 1
    assert valid((0, 0, 0), (1024, 2, 2), (1, 1, 1), 254) and not valid((0, 0, 0), (1025, 2, 2), (1, 1, 1), 254)
    assert p.distance_field((0, 0, 0), (1024, 2, 2), 254).shape == (2, 2, 1024) and p.lib.rq[1] == (1024, 2, 2)
    d2, near = p.distance_field((-LIMIT, 5, LIMIT - 258), (2, 3, 2), 255, robot=(1, 1, 256), stop_at="unseen", threshold=0.5, occupied_above=True, nearest=True)
    assert d2.shape == (2, 3, 2) and near.shape == (2, 3, 2, 3) and near.dtype == np.int32
    assert p.lib.rq == ((-LIMIT, 5, LIMIT - 258), (2, 3, 2), (1, 1, 256), 255, 1) and p.lib.test == (0.5, 1) and p.lib.nearest
    p.field = 1
    p.distance_field(np.array([1, 2, 3], np.int64), np.array([1, 1, 1], np.uint8), np.int32(3))
    assert p.lib.rq == ((1, 2, 3), (1, 1, 1), (1, 1, 1), 3, 0) and p.lib.test == (0.0, 1)          # OFusion: occupied above by default
