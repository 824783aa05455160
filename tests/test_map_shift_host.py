"""The map shift, host side (no GPU): the header declares the entry and the binding agrees; the host restatement se::shift_map
(include/se/shift_map.hpp, through tests/cpp/shift_kats.cpp) equals a literal numpy truth -- move the corners, filter by the two survival
rules, take the ancestor closure with closure_truth and make_keys -- on hand-made trees at 64^3 and 128^3, every block value, node value,
active flag and count; a shift followed by its inverse restores every block when none left the cube; the Python wrapper refuses bad
input before it calls the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.host_util import LIMIT, bare_pipeline, build_kats, make_keys
from tests.shift_util import closure_by_records, closure_keys, equal_blocks_nodes, leaf_level, shift_truth, shifts_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hand_made_tree(size, seed, inner=False):
    """Blocks in clusters and singly, their ancestors, a few childless coarse nodes; random values and flags.  inner: every block at least
    16 voxels from every face.  Returns blocks and nodes sorted by key, in the form of DenseSLAMPipeline.blocks() / nodes()."""
    rng = np.random.default_rng(seed)
    leaf, nblk = leaf_level(size), size // 8
    lo, hi = (2, nblk - 2) if inner else (0, nblk)
    cells = set()
    for _ in range(4):
        c = rng.integers(lo, hi, 3)
        for d in np.ndindex(3, 2, 3):
            q = c + np.array(d)
            if (q >= lo).all() and (q < hi).all():
                cells.add(tuple(int(v) for v in q))
    for _ in range(10):
        cells.add(tuple(int(v) for v in rng.integers(lo, hi, 3)))
    cells |= {(lo, lo, lo), (hi - 1, hi - 1, hi - 1), (lo, hi - 1, lo)}
    coords = np.array(sorted(cells), np.int64) * 8
    coords = coords[np.argsort(make_keys(coords, leaf))]
    coarse = [(rng.integers(0, 1 << l, 3) * (size >> l), l) for l in rng.integers(1, leaf, 6)] if not inner else []
    corners = np.concatenate([coords] + [c[None, :] for c, _ in coarse])
    levels = np.concatenate([np.full(len(coords), leaf)] + [np.array([l]) for _, l in coarse])
    keys = closure_keys(size, corners, levels)
    code = np.array(sorted({0} | {k for k in keys if k & 0x1FF != leaf}), np.uint64)
    nb, nn = len(coords), len(code)
    pick = lambda shape, init: np.where(rng.random(shape) < 0.3, rng.integers(-3, 50, shape).astype(np.float32) / 4, np.float32(init)).astype(np.float32)
    blocks = (coords.astype(np.int32), pick((nb, 512), 1.0), pick((nb, 512), 0.0), (rng.random(nb) < 0.5).astype(np.uint8))
    nodes = (code, (size >> (code & np.uint64(0x1FF)).astype(np.int64)).astype(np.uint32), pick((nn, 8), 1.0), pick((nn, 8), 0.0))
    assert blocks[3].min() == 0 and blocks[3].max() == 1
    return blocks, nodes


def run_shift(exe, tmp_path, field, size, shifts, blocks, nodes, permute=True):
    """se::shift_map through shift_kats, the shifts one after the other: counts per shift, the final blocks and nodes.  permute: the tree is
    built from the octants in a random order (False: in key order, as getMap() delivers a snapshot)."""
    coords, x, y, act = blocks
    code, _, nx, ny = nodes
    inp, out = str(tmp_path / "tree.bin"), str(tmp_path / "shifted.bin")
    rng = np.random.default_rng(1)
    with open(inp, "wb") as f:
        f.write(np.array([size, len(shifts)], np.int32).tobytes())
        f.write(np.asarray(shifts, np.int32).reshape(-1, 3).tobytes())
        f.write(np.uint64(len(code)).tobytes())
        for i in (rng.permutation(len(code)) if permute else range(len(code))):          # (any order: finalize links level by level)
            f.write(code[i].tobytes()); f.write(nx[i].tobytes()); f.write(ny[i].tobytes())
        f.write(np.uint64(len(coords)).tobytes())
        for i in (rng.permutation(len(coords)) if permute else range(len(coords))):
            f.write(np.array([*coords[i], act[i]], np.int32).tobytes()); f.write(x[i].tobytes()); f.write(y[i].tobytes())
    r = subprocess.run([exe, "dump", "sdf" if field == 0 else "ofusion", inp, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    raw = open(out, "rb").read()
    at = 0

    def take(dtype, n):
        nonlocal at
        a = np.frombuffer(raw, dtype, n, at)
        at += a.nbytes
        return a
    counts = take(np.int64, 4 * len(shifts)).reshape(-1, 4)
    bad = int(take(np.int64, 1)[0])
    nn = int(take(np.uint64, 1)[0])
    got_nodes = (take(np.uint64, nn), take(np.uint32, nn), take(np.float32, nn * 8).reshape(nn, 8), take(np.float32, nn * 8).reshape(nn, 8))
    nb = int(take(np.uint64, 1)[0])
    bkeys = take(np.uint64, nb)
    got_blocks = (take(np.int32, nb * 3).reshape(nb, 3), take(np.uint8, nb), take(np.float32, nb * 512).reshape(nb, 512), take(np.float32, nb * 512).reshape(nb, 512))
    assert at == len(raw) and bad == 0
    assert (bkeys == make_keys(got_blocks[0], leaf_level(size))).all()
    return counts, (got_blocks[0], got_blocks[2], got_blocks[3], got_blocks[1]), got_nodes


def all_shifts(size):
    groups = shifts_for(size)
    out = [s for g in ("small", "aligned", "half", "size") for s in groups[g]]
    out += [(-size, 0, 0), (0, 0, size), (-LIMIT, 0, 0), (0, LIMIT, -LIMIT), (0, -size // 2, size // 2), (-32, 0, 32), (64, 64, 64), (16, 0, 0)]
    return out


@pytest.fixture(scope="module")
def kats(tmp_path_factory):
    return build_kats("shift_kats", tmp_path_factory.mktemp("shift_kats"))


@pytest.mark.parametrize("field", [0, 1], ids=["sdf", "ofusion"])
@pytest.mark.parametrize("size", [64, 128])
def test_host_restatement_equals_the_numpy_truth(kats, tmp_path, size, field):
    init = (1.0, 0.0) if field == 0 else (0.0, 0.0)
    blocks, nodes = hand_made_tree(size, 5 + size)
    seen = {"kept_nodes": 0, "partial": 0, "all": 0, "none": 0}
    for s in all_shifts(size):
        want_b, want_n, want_c = shift_truth(size, s, blocks, nodes, init, closure=closure_by_records)
        fast = shift_truth(size, s, blocks, nodes, init)                     # (the vectorised closure the GPU tests use: the same truth)
        assert equal_blocks_nodes(fast[0], fast[1], want_b, want_n) is None and (fast[2] == want_c).all(), s
        counts, got_b, got_n = run_shift(kats, tmp_path, field, size, [s], blocks, nodes)
        assert equal_blocks_nodes(got_b, got_n, want_b, want_n) is None, (s, equal_blocks_nodes(got_b, got_n, want_b, want_n))
        assert counts[0].tolist() == want_c.tolist(), s
        assert want_c[0] + want_c[1] == len(blocks[0]) and want_c[2] + want_c[3] == len(nodes[0])
        if any(s):
            assert (got_n[2][0] == init[0]).all() and (got_n[3][0] == init[1]).all()      # the root is a new one
            seen["kept_nodes"] += int(want_c[2] > 0)
            seen["partial"] += int(want_c[0] > 0 and want_c[1] > 0)
            seen["none"] += int(want_c[0] == 0 and len(got_n[0]) == 1)
        else:
            seen["all"] += int(equal_blocks_nodes(got_b, got_n, blocks, nodes) is None)
    assert seen["all"] == 1 and seen["kept_nodes"] >= 2 and seen["partial"] >= 6 and seen["none"] >= 6, seen


def test_aligned_shift_keeps_exactly_the_aligned_levels(kats, tmp_path):
    """(32, -32, 0) at 128^3: nodes of side 16 and 32 can survive, nodes of side 64 cannot, whatever lies under them."""
    size = 128
    blocks, nodes = hand_made_tree(size, 11)
    counts, got_b, got_n = run_shift(kats, tmp_path, 0, size, [(32, -32, 0)], blocks, nodes)
    want_b, want_n, want_c = shift_truth(size, (32, -32, 0), blocks, nodes, (1.0, 0.0))
    assert equal_blocks_nodes(got_b, got_n, want_b, want_n) is None
    code, side, nx, ny = nodes
    moved = {}
    for k, s_, vx in zip(code.tolist(), side.tolist(), nx):
        if s_ in (16, 32):
            moved[(k, s_)] = vx
    assert counts[0][2] > 0 and counts[0][2] <= len(moved)
    side64 = got_n[1] == 64
    assert side64.any() and (got_n[2][side64] == 1.0).all() and (got_n[3][side64] == 0.0).all()       # recreated, never carried


@pytest.mark.parametrize("size", [64, 128])
def test_shift_then_inverse_restores_every_block(kats, tmp_path, size):
    blocks, nodes = hand_made_tree(size, 3, inner=True)
    for s in [(16, 0, 0), (-8, 16, -16), (0, 0, 8), (16, 16, 16)]:
        inv = tuple(-v for v in s)
        counts, got_b, got_n = run_shift(kats, tmp_path, 0, size, [s, inv], blocks, nodes)
        assert counts[0][1] == 0 and counts[1][1] == 0 and counts[0][0] == len(blocks[0])
        assert equal_blocks_nodes(got_b, got_n[:2], blocks, nodes[:2]) is None, s      # blocks, values, flags; the same node set
    # a shift that a face clips does lose blocks: the inverse cannot bring them back
    counts, got_b, _ = run_shift(kats, tmp_path, 0, size, [(size - 16, 0, 0), (16 - size, 0, 0)], blocks, nodes)
    assert counts[0][1] > 0 and len(got_b[0]) == counts[0][0] < len(blocks[0])


def test_invalid_shifts_leave_the_snapshot_alone(kats, tmp_path):
    blocks, nodes = hand_made_tree(64, 9)
    for s in [(4, 0, 0), (0, -12, 0), (0, 0, LIMIT + 8), (-LIMIT - 8, 0, 0), (8, 8, 7)]:
        counts, got_b, got_n = run_shift(kats, tmp_path, 1, 64, [s], blocks, nodes, permute=False)
        assert counts[0].tolist() == [-1, -1, -1, -1] and equal_blocks_nodes(got_b, got_n, blocks, nodes) is None, s


def test_header_declares_the_shift_entry():
    h = open(os.path.join(ROOT, "include", "se_hip.h")).read()
    assert "int se_hip_shift_map(se_hip_pipeline* p, const int32_t shift_voxels[3], int64_t* host_counts);" in re.sub(r"\s+", " ", h)
    assert "#define SE_HIP_K_COUNT 5" in h     # no new launch counter
    from supereight_amd import build, pipeline as P
    res, args = P.EXPORTS["se_hip_shift_map"]
    assert res is C.c_int and len(args) == 3
    assert "se_shift_kernels.h" in build.HEADERS
    src = open(os.path.join(ROOT, "supereight_amd", "csrc", "se_hip_api.hip")).read()
    assert '#include "se_shift_kernels.h"' in src


@pytest.mark.parametrize("shift,exc", [
    (np.zeros(3, np.float32), TypeError),
    ([8.0, 0, 0], TypeError),
    (None, TypeError),
    (np.zeros(4, np.int32), ValueError),
    (np.zeros((1, 3), np.int32), ValueError),
    (8, ValueError),
    ([8, 0, 4], ValueError),
    ([0, -12, 0], ValueError),
    ([LIMIT + 8, 0, 0], ValueError),
    ([0, 0, -LIMIT - 8], ValueError),
], ids=["float32", "float_list", "none", "four", "two_dim", "scalar", "not_multiple", "negative_not_multiple", "above_limit", "below_limit"])
def test_shift_refuses_bad_arguments_before_any_library_call(shift, exc):
    p = bare_pipeline(field=0, size=256, dim=4.8)
    with pytest.raises(exc):
        p.shift(shift)
    from supereight_amd.livemesh import LiveMesh
    with pytest.raises(exc):
        LiveMesh.shift(LiveMesh.__new__(LiveMesh), shift)


def test_shift_accepts_the_limits_themselves():
    from supereight_amd.pipeline import DenseSLAMPipeline
    assert DenseSLAMPipeline._shift_argument([LIMIT, -LIMIT, 0]).tolist() == [LIMIT, -LIMIT, 0]
    assert DenseSLAMPipeline._shift_argument(np.array([8, -8, 16], np.int64)).dtype == np.int32


def test_cpp_mirror_shift_program_compiles(tmp_path):
    """tests/cpp/shift_mirror.cpp (run on the GPU by test_gpu_map_shift_mirror.py) compiles against the headers for both field types."""
    for tag in ("SDF", "OFusion"):
        obj = str(tmp_path / f"sm_{tag}.o")
        r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-ffp-contract=off", f"-DSE_FIELD_TYPE={tag}", "-I" + os.path.join(ROOT, "include"),
                            "-c", os.path.join(ROOT, "tests", "cpp", "shift_mirror.cpp"), "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
