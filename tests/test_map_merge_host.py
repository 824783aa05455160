"""The map merge, host side (no GPU): the header declares the entry and the binding agrees; the value-pair function se::merge_value and the
host restatement se::merge_map (include/se/merge_map.hpp, through tests/cpp/merge_kats.cpp) equal the literal numpy truth of
tests/merge_util.py on random small octrees -- the three modes, both field types, shifts 0, 8 (unaligned to every node), 64 (aligned to
nodes of side <= 64) and a negative one that clips, a smaller source volume, weight saturation, zero weights; the Python wrapper refuses bad
input before it calls the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.host_util import LIMIT, bare_pipeline, build_kats, make_keys
from tests.merge_util import FILL, FUSE, INIT, MODES, REPLACE, both_observed, merge_truth, merge_values
from tests.shift_util import closure_keys, equal_blocks_nodes, leaf_level

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELD_NAME = {0: "sdf", 1: "ofusion"}


def random_tree(size, seed, field, empty=False):
    """Blocks in clusters and singly, their ancestors, a few childless coarse nodes; values of the field's kind -- SDF: x in [-1, 1] and
    integer weights 0 .. 200 (some observed voxels with weight 0), OFusion: log-odds up to +-900 and times -- with about a third of the
    voxels observed.  Blocks and nodes sorted by key, in the form of DenseSLAMPipeline.blocks() / nodes()."""
    rng = np.random.default_rng(seed)
    leaf, nblk = leaf_level(size), size // 8
    cells = set()
    if not empty:
        for _ in range(5):
            c = rng.integers(0, nblk, 3)
            for d in np.ndindex(3, 2, 3):
                q = c + np.array(d)
                if (q < nblk).all():
                    cells.add(tuple(int(v) for v in q))
        for _ in range(12):
            cells.add(tuple(int(v) for v in rng.integers(0, nblk, 3)))
        cells |= {(0, 0, 0), (nblk - 1, nblk - 1, nblk - 1)}
    coords = np.array(sorted(cells), np.int64).reshape(-1, 3) * 8
    coords = coords[np.argsort(make_keys(coords, leaf))]
    coarse = [(rng.integers(0, 1 << l, 3) * (size >> l), l) for l in rng.integers(1, leaf, 6)] if not empty else []
    corners = np.concatenate([coords] + [c[None, :] for c, _ in coarse])
    levels = np.concatenate([np.full(len(coords), leaf)] + [np.array([l]) for _, l in coarse]).astype(np.int64)
    keys = closure_keys(size, corners, levels)
    code = np.array(sorted({0} | {k for k in keys if k & 0x1FF != leaf}), np.uint64)
    ix, iy = INIT[field]

    def values(shape):
        seen = (rng.random(shape) < 0.35) & (not empty)
        if field == 0:
            x = (rng.integers(-8, 9, shape) / 8).astype(np.float32)
            y = np.where(rng.random(shape) < 0.1, 0, rng.integers(1, 201, shape)).astype(np.float32)
        else:
            x = (rng.integers(-3600, 3601, shape) / 4).astype(np.float32)
            y = (rng.integers(0, 400, shape) / 30).astype(np.float32)
        return np.where(seen, x, np.float32(ix)).astype(np.float32), np.where(seen, y, np.float32(iy)).astype(np.float32)
    nb, nn = len(coords), len(code)
    bx, by = values((nb, 512))
    nx, ny = values((nn, 8))
    blocks = (coords.astype(np.int32), bx, by, (rng.random(nb) < 0.5).astype(np.uint8))
    nodes = (code, (size >> (code & np.uint64(0x1FF)).astype(np.int64)).astype(np.uint32), nx, ny)
    return blocks, nodes


def _write_tree(f, blocks, nodes, rng):
    coords, x, y, act = blocks
    code, _, nx, ny = nodes
    f.write(np.uint64(len(code)).tobytes())
    for i in rng.permutation(len(code)):                       # (any order: finalize links level by level)
        f.write(code[i].tobytes()); f.write(nx[i].tobytes()); f.write(ny[i].tobytes())
    f.write(np.uint64(len(coords)).tobytes())
    for i in rng.permutation(len(coords)):
        f.write(np.array([*coords[i], act[i]], np.int32).tobytes()); f.write(x[i].tobytes()); f.write(y[i].tobytes())


def run_merge(exe, tmp_path, field, dsize, dst, ssize, src, s, mode, max_weight=100.0, same=0, factor=1.0):
    """se::merge_map through merge_kats: counts, the destination afterwards, the source afterwards."""
    inp, out = str(tmp_path / "trees.bin"), str(tmp_path / "merged.bin")
    rng = np.random.default_rng(1)
    with open(inp, "wb") as f:
        f.write(np.array([dsize, ssize, *s, mode], np.int32).tobytes())
        f.write(np.float32(max_weight).tobytes()); f.write(np.int32(same).tobytes()); f.write(np.float32(factor).tobytes())
        _write_tree(f, *dst, rng)
        _write_tree(f, *src, rng)
    r = subprocess.run([exe, "dump", FIELD_NAME[field], inp, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    raw = open(out, "rb").read()
    at = 0

    def take(dtype, n):
        nonlocal at
        a = np.frombuffer(raw, dtype, n, at)
        at += a.nbytes
        return a

    def tree(size):
        nn = int(take(np.uint64, 1)[0])
        nodes = (take(np.uint64, nn), take(np.uint32, nn), take(np.float32, nn * 8).reshape(nn, 8), take(np.float32, nn * 8).reshape(nn, 8))
        nb = int(take(np.uint64, 1)[0])
        bkeys = take(np.uint64, nb)
        c, a = take(np.int32, nb * 3).reshape(nb, 3), take(np.uint8, nb)
        x, y = take(np.float32, nb * 512).reshape(nb, 512), take(np.float32, nb * 512).reshape(nb, 512)
        assert (bkeys == make_keys(c, leaf_level(size))).all()
        return (c, x, y, a), nodes
    counts = take(np.int64, 12)
    bad = int(take(np.int64, 1)[0])
    got_dst, got_src = tree(dsize), tree(ssize)
    assert at == len(raw) and bad == 0
    return counts, got_dst, got_src


def run_values(exe, tmp_path, field, mode, max_weight, quads):
    inp, out = str(tmp_path / "pairs.bin"), str(tmp_path / "values.bin")
    quads = np.ascontiguousarray(quads, np.float32).reshape(-1, 4)
    with open(inp, "wb") as f:
        f.write(np.array([len(quads), mode], np.int32).tobytes()); f.write(np.float32(max_weight).tobytes()); f.write(quads.tobytes())
    r = subprocess.run([exe, "values", FIELD_NAME[field], inp, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return np.fromfile(out, np.float32).reshape(-1, 2)


@pytest.fixture(scope="module")
def kats(tmp_path_factory):
    return build_kats("merge_kats", tmp_path_factory.mktemp("merge_kats"))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ the value-pair function
def test_known_values_of_the_pair_function():
    """The table of include/se_hip.h on literal pairs, in numpy (the truth itself is checked here, by hand)."""
    f = np.float32

    def one(a, b, mode, field, mw=100):
        x, y = merge_values([a[0]], [a[1]], [b[0]], [b[1]], mode, field, mw)
        return float(x[0]), float(y[0])
    # SDF: init (1, 0)
    assert one((0.5, 3), (1, 0), FUSE, 0) == (0.5, 3)                                    # b unseen: a stays
    assert one((1, 0), (-0.25, 7), FILL, 0) == (-0.25, 7)                                # a unseen: b
    assert one((1, 0), (-0.25, 200), FUSE, 0) == (-0.25, 100)                            # ... y capped
    assert one((0.5, 3), (-0.25, 7), REPLACE, 0) == (-0.25, 7)
    assert one((0.5, 3), (-0.25, 7), FILL, 0) == (0.5, 3)
    assert one((0.5, 3), (-0.25, 1), FUSE, 0) == (float((f(3) * f(0.5) + f(1) * f(-0.25)) / f(4)), 4)        # sdf_update's mean at weight 1
    assert one((0.5, 200), (-0.25, 100), FUSE, 0) == (0.25, 100)                         # 200 + 100: max_weight, not 44
    assert one((0.5, 200), (-0.25, 100), FUSE, 0, 255) == (0.25, 255)
    assert one((0.5, 3), (-0.25, 0), FUSE, 0) == (0.5, 3)                                # b.y == 0 leaves a
    assert one((0.5, 0), (-0.25, 7), FUSE, 0) == (-0.25, 7)                              # a.y == 0 takes b
    assert one((0.5, 0), (-0.25, 0), FUSE, 0) == (0.5, 0)
    # OFusion: init (0, 0)
    assert one((2.5, 1.5), (0, 0), REPLACE, 1) == (2.5, 1.5)
    assert one((0, 0), (-3, 0.5), FILL, 1) == (-3, 0.5)
    assert one((2.5, 1.5), (-3, 0.5), FUSE, 1) == (-0.5, 1.5)                            # log-odds add, the later time
    assert one((900, 1), (800, 2), FUSE, 1) == (1000, 2) and one((-900, 3), (-800, 2), FUSE, 1) == (-1000, 3)
    assert one((2.5, 1.5), (-3, 0.5), REPLACE, 1) == (-3, 0.5) and one((2.5, 1.5), (-3, 0.5), FILL, 1) == (2.5, 1.5)
    assert one((0, 0.5), (0, 0), FUSE, 1) == (0, 0.5) and one((0, 0.5), (1, 0), FUSE, 1) == (1, 0.5)        # (0, t > 0) is observed


@pytest.mark.parametrize("field", [0, 1], ids=["sdf", "ofusion"])
def test_value_function_equals_the_numpy_truth(kats, tmp_path, field):
    rng = np.random.default_rng(4 + field)
    ix, iy = INIT[field]
    n = 4000
    if field == 0:
        x = lambda: (rng.integers(-16, 17, n) / 16).astype(np.float32) * np.float32(0.999)
        y = lambda: np.where(rng.random(n) < 0.15, 0, rng.integers(1, 256, n)).astype(np.float32)
    else:
        x = lambda: (rng.normal(0, 400, n)).astype(np.float32)
        y = lambda: (rng.integers(0, 300, n) / 30).astype(np.float32)
    quads = np.stack([x(), y(), x(), y()], 1)
    for col in (0, 2):                                          # a fifth of either side unseen
        un = rng.random(n) < 0.2
        quads[un, col], quads[un, col + 1] = ix, iy
    specials = [(0.5, 200, -0.25, 100), (0.5, 0, -0.25, 7), (0.5, 3, -0.25, 0), (ix, iy, ix, iy), (ix, iy, 0.25, 255), (0.25, 255, 0.25, 255),
                (0.3, 1, 0.7, 2), (-1, 100, 1, 100), (999, 4, 999, 5), (-999, 4, -999, 3)]
    quads = np.concatenate([np.array(specials, np.float32), quads])
    seen = {}
    for mode in (FUSE, REPLACE, FILL):
        for mw in (100, 255, 1):
            got = run_values(kats, tmp_path, field, mode, mw, quads)
            wx, wy = merge_values(quads[:, 0], quads[:, 1], quads[:, 2], quads[:, 3], mode, field, mw)
            assert (_bits(got[:, 0]) == _bits(wx)).all() and (_bits(got[:, 1]) == _bits(wy)).all(), (mode, mw)
            seen[(mode, mw)] = got
    if field == 0:
        assert seen[(FUSE, 100)][0].tolist() == [0.25, 100.0] and seen[(FUSE, 255)][0].tolist() == [0.25, 255.0]         # 200 + 100
        assert seen[(FUSE, 100)][1].tolist() == [-0.25, 7.0] and seen[(FUSE, 100)][2].tolist() == [0.5, 3.0]             # zero weights
        took = ~((quads[:, 2] == ix) & (quads[:, 3] == iy)) & (quads[:, 3] != 0)        # (where b contributes; elsewhere a stays, whatever its weight)
        assert (seen[(FUSE, 100)][took, 1] <= 100).all() and (seen[(FUSE, 100)][took, 1] == 100).sum() > 100            # saturation happens


# ------------------------------------------------------------------ the trees
SHIFTS = [(0, 0, 0), (8, 0, 0), (0, -8, 16), (64, 0, 0), (0, 64, -64), (-24, 0, 0), (-40, -16, 8), (32, 32, 0)]
SIZES = [(64, 64), (128, 128), (128, 64), (64, 128)]


@pytest.mark.parametrize("field", [0, 1], ids=["sdf", "ofusion"])
@pytest.mark.parametrize("dsize,ssize", SIZES, ids=[f"{s}into{d}" for d, s in SIZES])
def test_host_restatement_equals_the_numpy_truth(kats, tmp_path, dsize, ssize, field):
    dst, src = random_tree(dsize, 5 + dsize, field), random_tree(ssize, 77 + ssize, field)
    seen = {k: 0 for k in ("combined", "created", "clipped", "both", "nodes_combined", "nodes_created", "nodes_skipped", "root")}
    for i, s in enumerate(SHIFTS):
        for mode in (FUSE, REPLACE, FILL):
            mw = (100, 255, 30)[(i + mode) % 3]
            want_b, want_n, want_c = merge_truth(dsize, *dst, ssize, *src, s, mode, field, mw)
            counts, (got_b, got_n), (src_b, src_n) = run_merge(kats, tmp_path, field, dsize, dst, ssize, src, s, mode, mw)
            assert equal_blocks_nodes(got_b, got_n, want_b, want_n) is None, (s, mode, equal_blocks_nodes(got_b, got_n, want_b, want_n))
            assert counts.tolist() == want_c.tolist(), (s, mode)
            assert equal_blocks_nodes(src_b, src_n, *src) is None                       # the source is only read
            assert want_c[0] + want_c[1] + want_c[2] == len(src[0][0]) and want_c[3] + want_c[4] + want_c[5] == len(src[1][0])
            assert len(want_b[0]) == len(dst[0][0]) + want_c[1]
        seen["combined"] += int(want_c[0] > 0); seen["created"] += int(want_c[1] > 0); seen["clipped"] += int(want_c[2] > 0)
        seen["both"] += int(both_observed(dsize, dst[0], ssize, src[0], s, field) > 0)
        seen["nodes_combined"] += int(want_c[3] > 0); seen["nodes_created"] += int(want_c[4] > 0); seen["nodes_skipped"] += int(want_c[5] > 0)
        if not any(s):
            seen["root"] += int(want_c[5] == 0 if dsize == ssize else want_c[5] >= 1)    # the source root: only for s = 0 and equal sizes
        if s in ((8, 0, 0), (0, -8, 16), (-24, 0, 0), (-40, -16, 8)):
            assert want_c[3] == 0 and want_c[4] == 0                                     # unaligned to every node
    assert seen["root"] == 1 and seen["created"] >= 4 and seen["clipped"] >= 4 and seen["nodes_skipped"] >= 4, seen
    assert seen["combined"] >= 2 and seen["both"] >= 2 and seen["nodes_combined"] >= 2, seen


def test_merging_into_an_empty_tree_reproduces_the_source(kats, tmp_path):
    for field in (0, 1):
        src, empty = random_tree(64, 3, field), random_tree(64, 0, field, empty=True)
        counts, (got_b, got_n), _ = run_merge(kats, tmp_path, field, 64, empty, 64, src, (0, 0, 0), FUSE, 255.0)
        assert equal_blocks_nodes(got_b, got_n, (src[0][0], src[0][1], src[0][2], np.ones_like(src[0][3])), src[1]) is None
        counts, (got_b, got_n), _ = run_merge(kats, tmp_path, field, 64, src, 64, empty, (0, 0, 0), FUSE)
        assert equal_blocks_nodes(got_b, got_n, *src) is None and counts.tolist() == [0, 0, 0, 1, 0, 0] + [0] * 6


def test_invalid_arguments_leave_both_snapshots_alone(kats, tmp_path):
    dst, src = random_tree(64, 9, 0), random_tree(64, 10, 0)
    bad = [dict(s=(4, 0, 0)), dict(s=(0, -12, 0)), dict(s=(0, 0, LIMIT + 8)), dict(s=(8, 8, 7)), dict(mode=3), dict(mode=-1),
           dict(max_weight=0.0), dict(max_weight=256.0), dict(max_weight=99.5), dict(same=1), dict(factor=2.0)]
    for kw in bad:
        args = dict(s=(0, 0, 0), mode=FUSE, max_weight=100.0, same=0, factor=1.0)
        args.update(kw)
        counts, (got_b, got_n), (src_b, src_n) = run_merge(kats, tmp_path, 0, 64, dst, 64, src, **args)
        assert counts.tolist() == [-1] * 12, kw
        assert equal_blocks_nodes(got_b, got_n, *dst) is None and equal_blocks_nodes(src_b, src_n, *src) is None, kw
    counts, _, _ = run_merge(kats, tmp_path, 0, 64, dst, 64, src, (LIMIT, -LIMIT, 0), REPLACE, 1.0)      # the limits themselves
    assert counts[:3].tolist() == [0, 0, len(src[0][0])]


# ------------------------------------------------------------------ the entry and its wrapper
def test_header_declares_the_merge_entry():
    h = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "se_hip.h")).read())
    assert ("int se_hip_merge_map(se_hip_pipeline* dst, se_hip_pipeline* src, const int32_t shift_voxels[3], const se_hip_merge_rule* rule, "
            "int64_t* host_counts /* optional, [12] */);") in h
    assert "#define SE_HIP_MERGE_FUSE 0" in h and "#define SE_HIP_MERGE_REPLACE 1" in h and "#define SE_HIP_MERGE_FILL 2" in h
    assert "typedef struct se_hip_merge_rule { int32_t mode; float max_weight;" in h
    assert "never pushed down into destination voxels" in h
    assert "#define SE_HIP_K_COUNT 5" in h     # no new launch counter
    from supereight_amd import build, pipeline as P
    res, args = P.EXPORTS["se_hip_merge_map"]
    assert res is C.c_int and len(args) == 5
    assert C.sizeof(P._MergeRule) == 8 and P.DenseSLAMPipeline.MERGE_MODES == MODES
    assert "se_merge_kernels.h" in build.HEADERS
    src = open(os.path.join(ROOT, "supereight_amd", "csrc", "se_hip_api.hip")).read()
    assert '#include "se_merge_kernels.h"' in src


def _pair(**kw):
    a = bare_pipeline(field=0, size=128, dim=4.8, _device=0)
    attrs = dict(field=0, size=64, dim=2.4, _device=0)
    attrs.update(kw)
    return a, bare_pipeline(**attrs)


@pytest.mark.parametrize("kw,exc", [
    (dict(shift=np.zeros(3, np.float32)), TypeError),
    (dict(shift=None), TypeError),
    (dict(shift=np.zeros(4, np.int32)), ValueError),
    (dict(shift=[8, 0, 4]), ValueError),
    (dict(shift=[LIMIT + 8, 0, 0]), ValueError),
    (dict(mode="add"), ValueError),
    (dict(mode=0), TypeError),
    (dict(max_weight=0), ValueError),
    (dict(max_weight=256), ValueError),
    (dict(max_weight=99.5), ValueError),
    (dict(max_weight=float("nan")), ValueError),
    (dict(max_weight="100"), TypeError),
    (dict(max_weight=True), TypeError),
], ids=["float32", "none", "four", "not_multiple", "above_limit", "unknown_mode", "mode_int", "weight_0", "weight_256", "weight_fraction",
        "weight_nan", "weight_str", "weight_bool"])
def test_merge_refuses_bad_arguments_before_any_library_call(kw, exc):
    dst, src = _pair()
    with pytest.raises(exc):
        dst.merge(src, **kw)


def test_merge_refuses_unfit_sources_before_any_library_call():
    dst, _ = _pair()
    with pytest.raises(ValueError, match="itself"):
        dst.merge(dst)
    with pytest.raises(TypeError):
        dst.merge(None)
    with pytest.raises(ValueError, match="field"):
        dst.merge(_pair(field=1)[1])
    with pytest.raises(ValueError, match="devices"):
        dst.merge(_pair(_device=1)[1])
    with pytest.raises(ValueError, match="voxel"):
        dst.merge(_pair(dim=4.8)[1])
    with pytest.raises(ValueError, match="voxel"):
        dst.merge(_pair(size=128, dim=4.8000005)[1])           # one float32 ulp apart
    # what passes the checks reaches the library (here: the stand-in that refuses every call)
    with pytest.raises(AssertionError, match="se_hip_merge_map"):
        dst.merge(_pair()[1], (8, -16, 0), mode="fill", max_weight=255)
    with pytest.raises(AssertionError, match="se_hip_merge_map"):
        dst.merge(_pair()[1], np.array([LIMIT, -LIMIT, 0]), max_weight=np.float32(1))


def test_cpp_mirror_merge_program_compiles(tmp_path):
    """tests/cpp/merge_mirror.cpp (run on the GPU by test_gpu_map_merge_mirror.py) compiles against the headers for both field types."""
    for tag in ("SDF", "OFusion"):
        obj = str(tmp_path / f"mm_{tag}.o")
        r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-ffp-contract=off", f"-DSE_FIELD_TYPE={tag}", "-I" + os.path.join(ROOT, "include"),
                            "-c", os.path.join(ROOT, "tests", "cpp", "merge_mirror.cpp"), "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
