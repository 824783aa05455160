"""Batched map queries, host side (no GPU): the header declares both entries and the output struct, the Python wrapper refuses bad
input before it calls the library, and the C++ mirror's queryMap compiles against the header."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.host_util import bare_pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_query_entries():
    h = open(os.path.join(ROOT, "include", "se_hip.h")).read()
    assert re.search(r"int se_hip_query_points\(se_hip_pipeline\* p, const float\* device_points_m, int64_t n, const se_hip_query_out\* device_out\);", h)
    assert re.search(r"int se_hip_query_points_host\(se_hip_pipeline\* p, const float\* host_points_m, int64_t n, const se_hip_query_out\* host_out\);", h)
    body = re.search(r"typedef struct se_hip_query_out \{(.*?)\} se_hip_query_out;", h, re.S).group(1)
    fields = re.findall(r"(float|uint8_t)\* (\w+);", body)
    assert fields == [("float", "fine"), ("float", "coarse"), ("float", "interp"), ("float", "grad"), ("uint8_t", "status")]
    # the launch-counter slots are unchanged (SE_HIP_K_COUNT sizes arrays that callers pass in)
    assert "#define SE_HIP_K_COUNT 5" in h
    from supereight_amd.pipeline import EXPORTS, _QueryOut
    assert [f[0] for f in _QueryOut._fields_] == [f[1] for f in fields]
    for name in ("se_hip_query_points", "se_hip_query_points_host"):
        res, args = EXPORTS[name]
        assert res is C.c_int and args[2] is C.c_int64 and len(args) == 4


@pytest.mark.parametrize("points,exc", [
    (np.zeros((4, 3), np.float64), TypeError),
    (np.zeros((4, 3), np.int32), TypeError),
    (np.zeros((4, 2), np.float32), ValueError),
    (np.zeros(12, np.float32), ValueError),
    (np.zeros((2, 4, 3), np.float32), ValueError),
    ([[0.0, 0.0, 0.0]], TypeError),
    (None, TypeError),
], ids=["float64", "int32", "n_by_2", "flat", "3d", "list", "none"])
def test_query_refuses_bad_points_before_any_library_call(points, exc):
    with pytest.raises(exc):
        bare_pipeline().query(points)


def test_query_refuses_bad_torch_points_and_empty_requests():
    torch = pytest.importorskip("torch")
    p = bare_pipeline()
    with pytest.raises(ValueError):
        p.query(np.zeros((4, 3), np.float32), fine=False, coarse=False, interp=False, grad=False, status=False)
    with pytest.raises(TypeError):
        p.query(torch.zeros((4, 3), dtype=torch.float64))
    with pytest.raises(ValueError):
        p.query(torch.zeros((4, 2), dtype=torch.float32))
    with pytest.raises(ValueError):
        p.query(torch.zeros((3, 4), dtype=torch.float32).t())           # [4, 3], not contiguous
    with pytest.raises(ValueError):
        p.query(torch.zeros((4, 3), dtype=torch.float32))               # a CPU tensor: the device entry reads device memory


def test_cpp_mirror_query_program_compiles(tmp_path):
    """tests/cpp/map_query_mirror.cpp (run on the GPU by test_gpu_map_query_mirror.py) compiles against the header for both field types."""
    for tag in ("SDF", "OFusion"):
        obj = str(tmp_path / f"mq_{tag}.o")
        r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-ffp-contract=off", f"-DSE_FIELD_TYPE={tag}", "-I" + os.path.join(ROOT, "include"),
                            "-c", os.path.join(ROOT, "tests", "cpp", "map_query_mirror.cpp"), "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
