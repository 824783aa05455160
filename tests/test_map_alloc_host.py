"""Region allocation of the resident map, host side (no GPU): the header declares both entries and the box record and the binding agrees
with them; the host restatement se::allocate_boxes (include/se/allocate_region.hpp) equals a literal ancestor-closure truth on random maps
and lists (tests/cpp/alloc_kats.cpp) and a numpy closure written here; it equals the CPU oracle's Octree::allocate
(OraclePipeline.allocate_keys) on lists that hold the leaf block at the origin and differs from it by exactly the child-0 chain of the
keys[0] rule otherwise; the Python wrapper refuses bad input before it calls the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.host_util import LIMIT, bare_pipeline, box_records, build_kats, closure_truth, make_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_dump(exe, tmp_path, size, rec):
    inp, out = str(tmp_path / "boxes.bin"), str(tmp_path / "alloc.bin")
    rec.tofile(inp)
    r = subprocess.run([exe, "dump", str(size), inp, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(out, np.uint64)
    counts = raw[:4].view(np.int64)
    at, lists = 4, []
    for _ in range(3):
        n = int(raw[at]); lists.append(raw[at + 1:at + 1 + n]); at += 1 + n
    assert at == len(raw)
    return counts, lists[0], lists[1], lists[2]


CASES = {
    "leaf": lambda n: [((40, 40, 40), (104, 72, 57), 0), ((0, 0, 0), (8, 8, 8), 0)],
    "coarse": lambda n: [((100, 20, 30), (300, 90, 31), 3), ((0, 0, 0), (1, 1, 1), 2)],
    "mixed_overlapping": lambda n: [((40, 40, 40), (104, 72, 57), 0), ((60, 50, 30), (130, 130, 60), 0), ((60, 50, 30), (130, 130, 60), 4),
                                    ((40, 40, 40), (104, 72, 57), 0), ((0, 0, 0), (n, n, 16), 2), ((0, 0, 0), (8, 8, 8), 0)],
    "clipped": lambda n: [((n - 20, n - 9, n - 1), (n + 50, n + 50, n + 50), 0), ((-100, -100, -100), (9, 1, 17), 0), ((-5, 200, 200), (3, 280, 210), 3)],
    "outside_empty_inverted": lambda n: [((n, 0, 0), (n + 8, 8, 8), 0), ((-8, -8, -8), (0, 0, 0), 1), ((10, 10, 10), (10, 40, 40), 0),
                                         ((50, 60, 70), (40, 90, 90), 0), ((0, 0, 0), (8, 8, 8), 0)],
    "invalid": lambda n: [((0, 0, LIMIT + 1), (8, 8, 8), 0), ((-LIMIT - 1, 0, 0), (8, 8, 8), 0), ((0, 0, 0), (8, 2 ** 31 - 1, 8), 0),
                          ((0, 0, 0), (64, 64, 64), -1), ((0, 0, 0), (64, 64, 64), int(np.log2(n)) - 2), ((0, 0, 0), (64, 64, 64), 0, 1),
                          ((0, 0, 0), (64, 64, 64), 2, 0x80000000), ((0, 0, 0), (24, 8, 8), int(np.log2(n)) - 3), ((-LIMIT, -LIMIT, -LIMIT), (8, 8, LIMIT), 0)],
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("size", [64, 512])
def test_host_restatement_equals_the_closure_truth(tmp_path, case, size):
    exe = build_kats("alloc_kats", tmp_path)
    rec = box_records(CASES[case](size))
    requested, closure, pairs, invalid = closure_truth(size, rec)
    counts, bk, nk, keys = run_dump(exe, tmp_path, size, rec)
    leaf = int(np.log2(size)) - 3
    want_blocks = sorted(k for k in closure if k & 0x1FF == leaf)
    want_nodes = sorted([0] + [k for k in closure if k & 0x1FF != leaf])
    assert bk.tolist() == want_blocks and nk.tolist() == want_nodes
    assert counts.tolist() == [len(want_blocks), len(want_nodes) - 1, pairs, invalid]
    assert len(set(keys.tolist())) == len(keys) and set(keys.tolist()) <= requested
    if case == "invalid":
        assert invalid == 7 and pairs == 3 + size // 8          # the two valid ones: leaf level by its own number, and the limits themselves
    if case == "outside_empty_inverted":
        assert pairs == 1
    if case == "clipped":
        assert pairs == 3 * 2 * 1 + 2 * 1 * 3 + (1 * 2 * 1 if size == 512 else 0)


def test_host_restatement_on_random_maps_and_lists(tmp_path):
    exe = build_kats("alloc_kats", tmp_path)
    r = subprocess.run([exe, "random", "20", "7"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout
    f = r.stdout.split()
    assert f[0] == "checked" and int(f[1]) == 40 and f[2] == "mismatches" and int(f[3]) == 0


def _oracle_sets(field, size, keys):
    from oracle.binding import OraclePipeline
    o = OraclePipeline(field, size, 4.8, 32, 24)
    try:
        o.allocate_keys(np.asarray(sorted(keys), np.uint64))
        coords, x, y, act = o.blocks()
        code, side, nx, ny = o.nodes()
        init = (1.0, 0.0) if field == 0 else (0.0, 0.0)
        assert (x == init[0]).all() and (y == init[1]).all() and (act == 1).all() and (nx == init[0]).all() and (ny == init[1]).all()
        leaf = int(np.log2(size)) - 3
        return set(make_keys(coords, leaf).tolist()), set(int(c) for c in code)
    finally:
        o.close()


@pytest.mark.parametrize("field", [0, 1], ids=["sdf", "ofusion"])
def test_host_restatement_against_the_oracle(tmp_path, field):
    """Octree::allocate of the CPU oracle over the same keys, 512^3: equal on leaf lists, on lists with duplicates and on coarse or mixed
    lists that hold the leaf block at the origin; a purely coarse list differs by exactly the chain along child 0 below its smallest key."""
    exe = build_kats("alloc_kats", tmp_path)
    size, leaf = 512, 6
    origin = ((0, 0, 0), (8, 8, 8), 0)
    lists = {
        "leaf": [((200, 100, 50), (264, 132, 114), 0)],
        "leaf_duplicates": [((200, 100, 50), (264, 132, 114), 0), ((200, 100, 50), (264, 132, 114), 0), ((230, 110, 50), (270, 140, 70), 0)],
        "coarse_with_origin": [((100, 300, 30), (300, 400, 100), 4), origin],
        "mixed_with_origin": [((100, 300, 30), (300, 400, 100), 3), ((120, 310, 40), (150, 330, 90), 0), ((400, 400, 400), (512, 512, 512), 5), origin],
    }
    for name, rows in lists.items():
        rec = box_records(rows)
        requested, closure, pairs, invalid = closure_truth(size, rec)
        counts, bk, nk, _ = run_dump(exe, tmp_path, size, rec)
        ob, on = _oracle_sets(field, size, requested)
        assert set(bk.tolist()) == ob and set(nk.tolist()) == on, name
        assert counts[0] == len(ob) and counts[1] == len(on) - 1 and len(ob) + len(on) > 20, name
    # purely coarse: the reference walks keys[0] down along child 0
    rec = box_records([((128, 320, 64), (300, 400, 100), 4)])
    requested, closure, _, _ = closure_truth(size, rec)
    _, bk, nk, _ = run_dump(exe, tmp_path, size, rec)
    ob, on = _oracle_sets(field, size, requested)
    k0 = min(requested)
    corner = k0 & ~0x1FF
    chain_nodes = {corner | l for l in range(5, leaf)}
    chain_block = {corner | leaf}
    assert ob - set(bk.tolist()) == chain_block and on - set(nk.tolist()) == chain_nodes
    assert set(bk.tolist()) <= ob and set(nk.tolist()) <= on and len(chain_nodes) == 1


def test_header_declares_the_allocation_entries():
    h = open(os.path.join(ROOT, "include", "se_hip.h")).read()
    flat = re.sub(r"\s+", " ", h)
    assert ("int se_hip_allocate_boxes(se_hip_pipeline* p, const se_hip_alloc_box* device_boxes, int64_t n, int64_t* device_counts, "
            "uint64_t* device_new_keys, int64_t capacity_words);") in flat
    assert ("int se_hip_allocate_boxes_host(se_hip_pipeline* p, const se_hip_alloc_box* host_boxes, int64_t n, int64_t* host_counts, "
            "uint64_t* host_new_keys, int64_t capacity_words);") in flat
    body = re.search(r"typedef struct se_hip_alloc_box \{(.*?)\} se_hip_alloc_box;", h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()] == ["int32_t lo[3], hi[3]", "int32_t level", "uint32_t reserved"]
    assert "#define SE_HIP_K_COUNT 5" in h     # no new launch counter
    from supereight_amd import pipeline as P
    assert C.sizeof(P._AllocBox) == 32 and P.ALLOC_DTYPE.itemsize == 32
    assert [f[0] for f in P._AllocBox._fields_] == ["lo", "hi", "level", "reserved"]
    assert [P.ALLOC_DTYPE.fields[k][1] for k in ("lo", "hi", "level", "reserved")] == [getattr(P._AllocBox, k).offset for k in ("lo", "hi", "level", "reserved")]
    for name in ("se_hip_allocate_boxes", "se_hip_allocate_boxes_host"):
        res, args = P.EXPORTS[name]
        assert res is C.c_int and len(args) == 6 and args[2] is C.c_int64 and args[5] is C.c_int64


def test_build_lists_the_allocation_kernel_header():
    from supereight_amd import build
    assert "se_alloc_kernels.h" in build.HEADERS
    src = open(os.path.join(ROOT, "supereight_amd", "csrc", "se_hip_api.hip")).read()
    assert '#include "se_alloc_kernels.h"' in src
    assert os.path.exists(os.path.join(ROOT, "supereight_amd", "csrc", "se_alloc_kernels.h"))


def test_cpp_mirror_allocation_program_compiles(tmp_path):
    """tests/cpp/alloc_mirror.cpp (run on the GPU by test_gpu_map_alloc_mirror.py) compiles against the headers for both field types."""
    for tag in ("SDF", "OFusion"):
        obj = str(tmp_path / f"am_{tag}.o")
        r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-ffp-contract=off", f"-DSE_FIELD_TYPE={tag}", "-I" + os.path.join(ROOT, "include"),
                            "-c", os.path.join(ROOT, "tests", "cpp", "alloc_mirror.cpp"), "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def _pipeline():
    return bare_pipeline(field=0, size=256)


@pytest.mark.parametrize("boxes,exc", [
    (np.zeros((4, 6), np.int64), TypeError),
    (np.zeros((4, 6), np.float32), TypeError),
    (np.zeros((4, 3), np.int32), ValueError),
    (np.zeros(24, np.int32), ValueError),
    ([[0, 0, 0, 1, 1, 1]], TypeError),
    (None, TypeError),
], ids=["int64", "float32", "n_by_3", "flat", "list", "none"])
def test_allocate_refuses_bad_boxes_before_any_library_call(boxes, exc):
    with pytest.raises(exc):
        _pipeline().allocate(boxes)


def test_allocate_refuses_bad_arguments_before_any_library_call():
    from supereight_amd.pipeline import ALLOC_DTYPE
    p = _pipeline()
    ok = np.zeros((4, 6), np.int32)
    with pytest.raises(TypeError):
        p.allocate(ok, level=1.5)
    with pytest.raises(ValueError):
        p.allocate(ok, level=np.zeros(3, np.int32))
    with pytest.raises(TypeError):
        p.allocate(ok, return_keys=1)
    with pytest.raises(TypeError):
        p.allocate_records(np.zeros((4, 8), np.int32))          # host records are ALLOC_DTYPE
    with pytest.raises(ValueError):
        p.allocate_records(np.zeros((2, 2), ALLOC_DTYPE))
    with pytest.raises(ValueError):
        p.allocate_records(np.zeros(4, ALLOC_DTYPE), key_capacity=-1)
