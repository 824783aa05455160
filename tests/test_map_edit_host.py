"""Region edits of the resident map, host side (no GPU): the header declares both entries, the edit record and the constants and the binding
agrees with them; the host restatement of se::functor::axis_aligned_map (include/se/axis_aligned.hpp) gives the reference's two known
answers; the edit-list function that defines the device's behaviour equals the literal one-edit-at-a-time loop on random maps and lists;
the Python wrapper refuses bad input before it calls the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.host_util import bare_pipeline, build_kats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_edit_entries():
    h = open(os.path.join(ROOT, "include", "se_hip.h")).read()
    flat = re.sub(r"\s+", " ", h)
    assert ("int se_hip_edit_boxes(se_hip_pipeline* p, const se_hip_edit* device_edits, int64_t n, const se_hip_collide_test* test, "
            "int32_t mode, int64_t* device_counts);") in flat
    assert ("int se_hip_edit_boxes_host(se_hip_pipeline* p, const se_hip_edit* host_edits, int64_t n, const se_hip_collide_test* test, "
            "int32_t mode, int64_t* host_counts);") in flat
    body = re.search(r"typedef struct se_hip_edit \{(.*?)\} se_hip_edit;", h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    assert [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()] == ["int32_t lo[3], hi[3]", "float x, y", "uint32_t flags", "uint32_t only"]
    consts = dict(re.findall(r"#define (SE_HIP_EDIT_\w+) (\d+)u?", h))
    assert consts == {"SE_HIP_EDIT_SET_X": "1", "SE_HIP_EDIT_SET_Y": "2", "SE_HIP_EDIT_BLOCKS": "4", "SE_HIP_EDIT_NODES": "8",
                      "SE_HIP_EDIT_STRICT": "0", "SE_HIP_EDIT_REFERENCE": "1"}
    assert "#define SE_HIP_K_COUNT 5" in h     # no new launch counter
    from supereight_amd import pipeline as P
    assert (P.EDIT_SET_X, P.EDIT_SET_Y, P.EDIT_BLOCKS, P.EDIT_NODES) == (1, 2, 4, 8)
    assert (P.EDIT_OCCUPIED, P.EDIT_UNSEEN, P.EDIT_EMPTY, P.EDIT_ANY) == (1 << P.COLLISION_OCCUPIED, 1 << P.COLLISION_UNSEEN, 1 << P.COLLISION_EMPTY, 7)
    assert P._EDIT_MODES == {"strict": 0, "reference": 1}
    assert [f[0] for f in P._Edit._fields_] == ["lo", "hi", "x", "y", "flags", "only"]
    assert C.sizeof(P._Edit) == 40 and P.EDIT_DTYPE.itemsize == 40
    assert [P.EDIT_DTYPE.fields[k][1] for k in ("lo", "hi", "x", "y", "flags", "only")] == [getattr(P._Edit, k).offset for k in ("lo", "hi", "x", "y", "flags", "only")]
    for name in ("se_hip_edit_boxes", "se_hip_edit_boxes_host"):
        res, args = P.EXPORTS[name]
        assert res is C.c_int and len(args) == 6 and args[2] is C.c_int64 and args[4] is C.c_int32


def test_build_lists_the_edit_kernel_header():
    from supereight_amd import build
    assert "se_edit_kernels.h" in build.HEADERS
    src = open(os.path.join(ROOT, "supereight_amd", "csrc", "se_hip_api.hip")).read()
    assert '#include "se_edit_kernels.h"' in src


def test_reference_known_answers_on_the_host_octree(tmp_path):
    """AxisAlignedTest.Init and .BBoxTest: 512 blocks; whole-map assignment reads back everywhere; box [100, 151): 10 inside 100 .. 150
    (51^3 voxels, all allocated), untouched elsewhere in every allocated block of [50, 200)^3."""
    exe = build_kats("edit_kats", tmp_path)
    r = subprocess.run([exe, "kats"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["blocks", "512", "Init", "0", "BBoxTest", str(51 ** 3), "0"]


def test_reference_node_positions(tmp_path):
    exe = build_kats("edit_kats", tmp_path)
    r = subprocess.run([exe, "positions"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    f = r.stdout.split()
    assert f[0] == "positions" and int(f[1]) >= 8 and int(f[3]) >= 3 and int(f[5]) == 0    # nodes of at least three levels


def test_edit_list_equals_the_literal_loop(tmp_path):
    exe = build_kats("edit_kats", tmp_path)
    r = subprocess.run([exe, "random", "30", "11"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout
    f = r.stdout.split()
    assert f[0] == "checked" and int(f[1]) == 2 * 30 * 4 and f[2] == "mismatches" and int(f[3]) == 0


def test_cpp_mirror_edit_program_compiles(tmp_path):
    """tests/cpp/edit_mirror.cpp (run on the GPU by test_gpu_map_edit_mirror.py) compiles against the headers for both field types."""
    for tag in ("SDF", "OFusion"):
        obj = str(tmp_path / f"em_{tag}.o")
        r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-ffp-contract=off", f"-DSE_FIELD_TYPE={tag}", "-I" + os.path.join(ROOT, "include"),
                            "-c", os.path.join(ROOT, "tests", "cpp", "edit_mirror.cpp"), "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def _pipeline():
    return bare_pipeline(field=0)


@pytest.mark.parametrize("boxes,exc", [
    (np.zeros((4, 6), np.int64), TypeError),
    (np.zeros((4, 6), np.float32), TypeError),
    (np.zeros((4, 3), np.int32), ValueError),
    (np.zeros(24, np.int32), ValueError),
    ([[0, 0, 0, 1, 1, 1]], TypeError),
    (None, TypeError),
], ids=["int64", "float32", "n_by_3", "flat", "list", "none"])
def test_edit_refuses_bad_boxes_before_any_library_call(boxes, exc):
    with pytest.raises(exc):
        _pipeline().edit(boxes, 1.0)
    with pytest.raises(exc):
        _pipeline().reset(boxes)


def test_edit_refuses_bad_arguments_before_any_library_call():
    p = _pipeline()
    ok = np.zeros((4, 6), np.int32)
    with pytest.raises(ValueError):
        p.edit(ok, 1.0, mode="loose")
    with pytest.raises(ValueError):
        p.edit(ok, 1.0, only="solid")
    with pytest.raises(ValueError):
        p.edit(ok, 1.0, only=0)
    with pytest.raises(ValueError):
        p.edit(ok, 1.0, only=8)
    with pytest.raises(ValueError):
        p.edit(ok, 1.0, only=[])
    with pytest.raises(TypeError):
        p.edit(ok, 1.0, only=True)
    with pytest.raises(ValueError):
        p.edit(ok, 1.0, threshold=float("nan"))
    with pytest.raises(TypeError):
        p.edit(ok, 1.0, occupied_above=2)
    with pytest.raises(TypeError):
        p.edit(ok, 1.0, blocks=1)
    with pytest.raises(ValueError):
        p.edit(ok, np.zeros(3, np.float32))           # one value per box, or a scalar
    with pytest.raises(ValueError):
        p.edit(ok, 1.0, np.zeros((4, 2), np.float32))
    with pytest.raises(TypeError):
        p.edit_records(np.zeros((4, 10), np.int32))     # host records are EDIT_DTYPE
    with pytest.raises(ValueError):
        p.edit_records(np.zeros(4, __import__("supereight_amd.pipeline", fromlist=["EDIT_DTYPE"]).EDIT_DTYPE), mode="loose")


def test_edit_refuses_bad_torch_boxes():
    torch = pytest.importorskip("torch")
    p = _pipeline()
    with pytest.raises(TypeError):
        p.edit(torch.zeros((4, 6), dtype=torch.int64), 1.0)
    with pytest.raises(ValueError):
        p.edit(torch.zeros((4, 5), dtype=torch.int32), 1.0)
    with pytest.raises(ValueError):
        p.edit(torch.zeros((4, 6), dtype=torch.int32), 1.0)              # a CPU tensor: the device entry reads device memory
    with pytest.raises(ValueError):
        p.edit_records(torch.zeros((4, 10), dtype=torch.int32))
