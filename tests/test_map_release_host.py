"""The release of map regions, host side (no GPU): the header declares the entry and the binding agrees; the host restatement
se::release_map (include/se/release_map.hpp, through tests/cpp/release_kats.cpp) equals the literal numpy truth of tests/release_util.py on
maps the CPU oracle fused (room and stress streams, 64^3 and 128^3, both fields) and on hand-built trees that pin each clause of the
definition; the Python wrapper refuses bad input before it calls the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from supereight_amd.synthetic import make_stream
from tests.host_util import bare_pipeline, build_kats, make_keys
from tests.release_util import (ALL, INVALID_ROWS, LIMIT, UNSEEN, bits, equal_blocks_nodes, get_truth, leaf_level, record_sets, record_valid, records,
                                release_truth)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SDF, OFUSION = 0, 1
INIT = {SDF: (1.0, 0.0), OFUSION: (0.0, 0.0)}


def run_release(exe, tmp_path, field, size, rec, blocks, nodes, pts=None, permute=True):
    """se::release_map through release_kats, the records in one call: (accepted, counts, touched, blocks, nodes, get before, get after)."""
    coords, x, y, act = blocks
    code, _, nx, ny = nodes
    pts = np.zeros((0, 3), np.int32) if pts is None else np.asarray(pts, np.int32).reshape(-1, 3)
    inp, out = str(tmp_path / "tree.bin"), str(tmp_path / "released.bin")
    rng = np.random.default_rng(1)
    with open(inp, "wb") as f:
        f.write(np.array([size, len(rec)], np.int32).tobytes())
        f.write(rec.tobytes())
        f.write(np.uint64(len(code)).tobytes())
        for i in (rng.permutation(len(code)) if permute else range(len(code))):
            f.write(code[i].tobytes()); f.write(nx[i].astype(np.float32).tobytes()); f.write(ny[i].astype(np.float32).tobytes())
        f.write(np.uint64(len(coords)).tobytes())
        for i in (rng.permutation(len(coords)) if permute else range(len(coords))):
            f.write(np.array([*coords[i], act[i]], np.int32).tobytes()); f.write(x[i].astype(np.float32).tobytes()); f.write(y[i].astype(np.float32).tobytes())
        f.write(np.uint64(len(pts)).tobytes()); f.write(pts.tobytes())
    r = subprocess.run([exe, "dump", "sdf" if field == SDF else "ofusion", inp, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    raw = open(out, "rb").read()
    at = 0

    def take(dtype, n):
        nonlocal at
        a = np.frombuffer(raw, dtype, n, at)
        at += a.nbytes
        return a
    accepted = int(take(np.int64, 1)[0])
    counts, touched = take(np.int64, 5), take(np.int32, 6)
    bad = int(take(np.int64, 1)[0])
    nn = int(take(np.uint64, 1)[0])
    got_nodes = (take(np.uint64, nn), take(np.uint32, nn), take(np.float32, nn * 8).reshape(nn, 8), take(np.float32, nn * 8).reshape(nn, 8))
    nb = int(take(np.uint64, 1)[0])
    bkeys = take(np.uint64, nb)
    gb = (take(np.int32, nb * 3).reshape(nb, 3), take(np.uint8, nb), take(np.float32, nb * 512).reshape(nb, 512), take(np.float32, nb * 512).reshape(nb, 512))
    before, after = take(np.float32, len(pts) * 2).reshape(-1, 2), take(np.float32, len(pts) * 2).reshape(-1, 2)
    assert at == len(raw) and bad == 0
    assert (bkeys == make_keys(gb[0], leaf_level(size))).all()
    return accepted, counts, touched, (gb[0], gb[2], gb[3], gb[1]), got_nodes, before, after


def check(exe, tmp_path, field, size, rows, blocks, nodes, pts=None):
    """One call against the truth, everything bit for bit; returns (counts, info, blocks, nodes, get before, get after)."""
    rec = records(rows)
    want_b, want_n, want_c, want_t, info = release_truth(size, rec, blocks, nodes, INIT[field])
    accepted, counts, touched, got_b, got_n, before, after = run_release(exe, tmp_path, field, size, rec, blocks, nodes, pts)
    assert accepted == 1
    assert equal_blocks_nodes(got_b, got_n, want_b, want_n) is None, equal_blocks_nodes(got_b, got_n, want_b, want_n)
    assert counts.tolist() == want_c.tolist() and touched.tolist() == want_t.tolist()
    assert want_c[0] + want_c[1] == len(blocks[0]) and want_c[2] + want_c[3] == len(nodes[0])
    if pts is not None:
        assert (bits(before) == bits(get_truth(size, blocks, nodes, pts))).all() and (bits(after) == bits(get_truth(size, want_b, want_n, pts))).all()
    return want_c, info, got_b, got_n, before, after


@pytest.fixture(scope="module")
def kats(tmp_path_factory):
    return build_kats("release_kats", tmp_path_factory.mktemp("release_kats"))


# ------------------------------------------------------------------ maps the oracle fused
_MAPS = {}


def oracle_map(kind, field, size):
    """Six frames of the stream at 160 x 120 on the CPU oracle: (blocks, nodes), computed once and left unchanged."""
    key = (kind, field, size)
    if key not in _MAPS:
        from oracle.binding import OraclePipeline
        w, h, dim = 160, 120, 2.4 * size / 256
        s = make_stream(kind, w, h, dim, holes=False)
        o = OraclePipeline(field, size, dim, w, h)
        for f in range(6):
            o.integrate(s.depth(f), s.pose(f), s.k, 0.1 if field == SDF else 0.02, f)
        _MAPS[key] = (o.blocks(), o.nodes())
        o.close()
    return _MAPS[key]


@pytest.mark.parametrize("field", [SDF, OFUSION], ids=["sdf", "ofusion"])
@pytest.mark.parametrize("size", [64, 128])
@pytest.mark.parametrize("kind", ["room", "stress"])
def test_host_restatement_equals_the_numpy_truth_on_oracle_maps(kats, tmp_path, kind, size, field):
    blocks, nodes = oracle_map(kind, field, size)
    rng = np.random.default_rng(size)
    pts = rng.integers(0, size, (400, 3))
    seen = {}
    for name, rows in record_sets(size).items():
        c, info, _, _, before, after = check(kats, tmp_path, field, size, rows, blocks, nodes, pts)
        seen[name] = c
        if name == "unseen_everywhere":
            assert (bits(before) == bits(after)).all()                         # UNSEEN changes no answer of get
            assert c[1] == info["empty_blocks"] >= 5 and c[3] >= 1 and c[4] == 0, c      # the blocks fusion left all-unseen, and a parent of only such
        if name == "all_everything":
            assert c.tolist()[:4] == [0, len(blocks[0]), 1, len(nodes[0]) - 1] and c[4] > 0
            assert (bits(after[:, 0]) == bits(np.float32(INIT[field][0]))).all() and (bits(after[:, 1]) == bits(np.float32(INIT[field][1]))).all()
    assert seen["all_centre"][4] >= (10 if size == 128 else 1), seen["all_centre"]     # blocks that held observed voxels were forgotten
    assert seen["all_one_short"][1] <= seen["all_centre"][1]
    assert seen["exactly_65"].tolist() == seen["exactly_64"].tolist()


# ------------------------------------------------------------------ hand-built trees, a clause each
def tree(size, cells, values=None, node_values=None, extra_nodes=()):
    """Blocks at the given block cells (units of 8) with their ancestors, plus `extra_nodes` [(corner, level)] with theirs.  values: cell ->
    (x, y) written into voxel 5 of the block; node_values: (corner, level, child) -> (x, y).  SDF initValue() elsewhere."""
    from tests.shift_util import closure_keys
    leaf = leaf_level(size)
    coords = np.array(sorted(cells), np.int64).reshape(-1, 3) * 8
    coords = coords[np.argsort(make_keys(coords, leaf))]
    corners = np.concatenate([coords] + [np.array(c, np.int64)[None, :] for c, _ in extra_nodes])
    levels = np.concatenate([np.full(len(coords), leaf)] + [np.array([l]) for _, l in extra_nodes])
    keys = closure_keys(size, corners, levels)
    code = np.array(sorted({0} | {k for k in keys if k & 0x1FF != leaf}), np.uint64)
    nb, nn = len(coords), len(code)
    x, y = np.full((nb, 512), 1.0, np.float32), np.zeros((nb, 512), np.float32)
    for cell, (vx, vy) in (values or {}).items():
        i = int(np.nonzero((coords == np.array(cell) * 8).all(1))[0][0])
        x[i, 5], y[i, 5] = vx, vy
    nx, ny = np.full((nn, 8), 1.0, np.float32), np.zeros((nn, 8), np.float32)
    for (corner, level, child), (vx, vy) in (node_values or {}).items():
        i = int(np.nonzero(code == make_keys(np.array(corner)[None, :], level)[0])[0][0])
        nx[i, child], ny[i, child] = vx, vy
    act = (np.arange(nb) % 2).astype(np.uint8)
    return (coords.astype(np.int32), x, y, act), (code, (size >> (code & np.uint64(0x1FF)).astype(np.int64)).astype(np.uint32), nx, ny)


FULL16 = [(2 + i, 2 + j, 2 + k) for i in range(2) for j in range(2) for k in range(2)]       # the eight blocks of the side-16 node at (16, 16, 16)


def test_a_box_that_cuts_a_block_in_half_releases_nothing(kats, tmp_path):
    blocks, nodes = tree(64, [(1, 1, 1)], {(1, 1, 1): (0.5, 2.0)})
    for rows in ([((8, 8, 8), (4, 8, 8), ALL)], [((8, 8, 8), (8, 8, 7), ALL)], [((9, 8, 8), (8, 8, 8), ALL)], [((8, 8, 8), (8, 8, 7), UNSEEN)],
                 [((8, 8, 8), (4, 8, 8), ALL), ((12, 8, 8), (4, 8, 8), ALL)]):          # (two halves do not make a whole: containment is per record)
        c, _, got_b, got_n, _, _ = check(kats, tmp_path, SDF, 64, rows, blocks, nodes)
        assert c.tolist() == [1, 0, len(nodes[0]), 0, 0] and equal_blocks_nodes(got_b, got_n, blocks, nodes) is None


def test_a_box_that_equals_one_block(kats, tmp_path):
    blocks, nodes = tree(64, [(1, 1, 1), (1, 1, 0)], {(1, 1, 1): (0.5, 2.0), (1, 1, 0): (0.25, 1.0)})
    c, _, got_b, got_n, _, _ = check(kats, tmp_path, SDF, 64, [((8, 8, 8), 8, ALL)], blocks, nodes)
    assert c.tolist() == [1, 1, len(nodes[0]), 0, 1] and got_b[0].tolist() == [[8, 8, 0]] and got_b[3].tolist() == [blocks[3][0]]
    # alone under its ancestors: the box holds the block only, so the ancestors stay, childless
    blocks, nodes = tree(64, [(1, 1, 1)], {(1, 1, 1): (0.5, 2.0)})
    c, _, got_b, got_n, _, _ = check(kats, tmp_path, SDF, 64, [((8, 8, 8), 8, ALL)], blocks, nodes)
    assert c.tolist() == [0, 1, 3, 0, 1] and len(got_n[0]) == 3


@pytest.mark.parametrize("side", [16, 32])
def test_a_box_that_equals_a_node_whose_blocks_are_all_inside(kats, tmp_path, side):
    inside = FULL16 if side == 16 else FULL16 + [(0, 0, 0), (3, 0, 1)]
    lo = (16, 16, 16) if side == 16 else (0, 0, 0)
    outside = [(4, 4, 4), (7, 0, 0)]
    blocks, nodes = tree(64, inside + outside, {c: (0.5, 3.0) for c in inside + outside})
    c, _, got_b, got_n, _, _ = check(kats, tmp_path, SDF, 64, [(lo, side, ALL)], blocks, nodes)
    assert c[0] == 2 and c[1] == len(inside) == c[4] and c[3] == (1 if side == 16 else 1 + 3)     # the node itself (and, at 32, its three side-16 nodes)
    assert sorted(map(tuple, (got_b[0] // 8).tolist())) == sorted(outside)
    # one voxel short on one axis: the node is not contained, but the blocks that are go
    c2, _, _, _, _, _ = check(kats, tmp_path, SDF, 64, [(lo, (side, side - 1, side), ALL)], blocks, nodes)
    assert c2[3] < c[3] and 0 < c2[1] < c[1]


def test_unseen_over_a_node_that_keeps_one_valued_entry(kats, tmp_path):
    """The seven blocks of the side-16 node are all-init and go; the node has one valued entry (above the absent child 3), so it stays with
    that entry, and so do its ancestors."""
    blocks, nodes = tree(64, [c for c in FULL16 if c != (3, 3, 2)], node_values={((16, 16, 16), 2, 3): (0.5, 1.0)})
    c, info, got_b, got_n, _, _ = check(kats, tmp_path, SDF, 64, [((0, 0, 0), 64, UNSEEN)], blocks, nodes)
    assert c.tolist() == [0, 7, 3, 0, 0] and got_n[0].tolist() == nodes[0].tolist()
    assert equal_blocks_nodes((), got_n, (), nodes) is None
    # without the value the node goes, and its parent -- then childless and all-init -- with it; the root stays
    blocks, nodes = tree(64, FULL16)
    c, _, _, got_n, _, _ = check(kats, tmp_path, SDF, 64, [((0, 0, 0), 64, UNSEEN)], blocks, nodes)
    assert c.tolist() == [0, 8, 1, 2, 0] and got_n[0].tolist() == [0]


def test_unseen_over_an_all_init_block_under_a_valued_parent_entry(kats, tmp_path):
    """The block at cell (2, 2, 2) is child 0 of the side-16 node at (16, 16, 16); that entry is not init.  The entry is reset, so get is
    unchanged (init) at all 512 voxels; the valued entry of an ABSENT child (3) is not touched."""
    blocks, nodes = tree(64, [(2, 2, 2), (3, 3, 3)], {(3, 3, 3): (0.5, 1.0)}, {((16, 16, 16), 2, 0): (-0.5, 7.0), ((16, 16, 16), 2, 3): (0.25, 2.0)})
    pts = np.stack(np.meshgrid(*[np.arange(16, 24)] * 3, indexing="ij"), -1).reshape(-1, 3)
    pts = np.concatenate([pts, [[31, 31, 16], [24, 24, 16]]])             # ... and two voxels of absent child 3
    c, info, got_b, got_n, before, after = check(kats, tmp_path, SDF, 64, [((0, 0, 0), 64, UNSEEN)], blocks, nodes, pts)
    assert c.tolist() == [1, 1, 3, 0, 0] and info == {"reset": 1, "reset_valued": 1, "empty_blocks": 1}
    assert (bits(before) == bits(after)).all() and (before[:512] == [1.0, 0.0]).all() and (after[512:] == [0.25, 2.0]).all()
    i = int(np.nonzero(got_n[1] == 16)[0][0])
    assert (got_n[2][i, 0], got_n[3][i, 0]) == (1.0, 0.0) and (got_n[2][i, 3], got_n[3][i, 3]) == (0.25, 2.0)


def test_an_all_record_and_an_unseen_record_over_the_same_block(kats, tmp_path):
    blocks, nodes = tree(64, [(1, 1, 1), (5, 5, 5)], {(1, 1, 1): (0.5, 2.0), (5, 5, 5): (0.5, 2.0)})
    for rows in ([((8, 8, 8), 8, ALL), ((0, 0, 0), 64, UNSEEN)], [((0, 0, 0), 64, UNSEEN), ((8, 8, 8), 8, ALL)]):
        c, _, got_b, _, _, _ = check(kats, tmp_path, SDF, 64, rows, blocks, nodes)
        assert c[:2].tolist() == [1, 1] and c[4] == 1 and got_b[0].tolist() == [[40, 40, 40]]


def test_the_whole_volume_with_all_leaves_the_root(kats, tmp_path):
    blocks, nodes = tree(128, FULL16 + [(15, 15, 15)], {c: (0.5, 1.0) for c in FULL16}, {((0, 0, 0), 0, 7): (0.5, 1.0), ((0, 0, 0), 0, 1): (0.5, 1.0)})
    c, _, got_b, got_n, _, _ = check(kats, tmp_path, SDF, 128, [((0, 0, 0), 128, ALL)], blocks, nodes)
    assert c.tolist() == [0, 9, 1, len(nodes[0]) - 1, 8] and len(got_b[0]) == 0 and got_n[0].tolist() == [0]
    # entries 0 and 7 stood above released children: init; entry 1 stood above nothing and is the root's own
    assert got_n[2][0].tolist() == [1.0, 0.5] + [1.0] * 6 and got_n[3][0].tolist() == [0.0, 1.0] + [0.0] * 6


def test_no_records_change_nothing(kats, tmp_path):
    blocks, nodes = tree(64, FULL16, {FULL16[0]: (0.5, 1.0)})
    c, _, got_b, got_n, _, _ = check(kats, tmp_path, SDF, 64, [], blocks, nodes)
    assert c.tolist() == [8, 0, len(nodes[0]), 0, 0] and equal_blocks_nodes(got_b, got_n, blocks, nodes) is None


def test_every_invalid_record_leaves_the_snapshot_alone(kats, tmp_path):
    blocks, nodes = tree(64, FULL16, {FULL16[0]: (0.5, 1.0)})
    good = ((0, 0, 0), 64, ALL)
    for row in INVALID_ROWS:
        assert not record_valid(records([row])[0]), row
        for rows in ([row], [good, row], [row, good]):
            accepted, counts, touched, got_b, got_n, _, _ = run_release(kats, tmp_path, OFUSION, 64, records(rows), blocks, nodes, permute=False)
            assert accepted == 0 and counts.tolist() == [-1] * 5 and equal_blocks_nodes(got_b, got_n, blocks, nodes) is None, row
    accepted, counts = run_release(kats, tmp_path, SDF, 64, records([((0, 0, 0), 1, UNSEEN)] * 4097), blocks, nodes, permute=False)[:2]
    assert accepted == 0 and counts.tolist() == [-1] * 5
    assert run_release(kats, tmp_path, SDF, 64, records([((0, 0, 0), 1, UNSEEN)] * 4096), blocks, nodes)[0] == 1
    # the limits themselves are valid
    for row in [((-LIMIT, 0, 0), (1, 1, 1), ALL), ((LIMIT - 8, 0, 0), 8, UNSEEN), ((-LIMIT, -LIMIT, -LIMIT), 2 * LIMIT - 1, ALL)]:
        assert record_valid(records([row])[0]) and run_release(kats, tmp_path, SDF, 64, records([row]), blocks, nodes)[0] == 1, row


# ------------------------------------------------------------------ the header, the binding, the wrapper
def test_header_declares_the_release_entry():
    h = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "se_hip.h")).read())
    assert "#define SE_HIP_RELEASE_ALL 1" in h and "#define SE_HIP_RELEASE_UNSEEN 2" in h
    assert "typedef struct se_hip_release_box { int32_t lo[3]; int32_t side[3]; int32_t what; int32_t reserved; } se_hip_release_box;" in h
    assert "int se_hip_release_boxes(se_hip_pipeline* p, const se_hip_release_box* host_boxes, int64_t n, int64_t* host_counts" in h
    assert "#define SE_HIP_K_COUNT 5" in h     # no new launch counter
    from supereight_amd import build, pipeline as P
    res, args = P.EXPORTS["se_hip_release_boxes"]
    assert res is C.c_int and len(args) == 5
    assert P.RELEASE_DTYPE.itemsize == 32 and P.DenseSLAMPipeline.RELEASE_WHAT == {"all": ALL, "unseen": UNSEEN}
    assert "se_release_kernels.h" in build.HEADERS
    src = open(os.path.join(ROOT, "supereight_amd", "csrc", "se_hip_api.hip")).read()
    assert '#include "se_release_kernels.h"' in src


@pytest.mark.parametrize("boxes,what,exc", [
    ([((0, 0, 0), 8)], 2, TypeError),
    ([((0, 0, 0), 8)], "some", ValueError),
    ([((0, 0, 0), 8, "most")], "all", ValueError),
    ([((0, 0, 0), 8, 1)], "all", TypeError),
    (np.zeros((1, 6), np.int32), "all", TypeError),
    (7, "all", TypeError),
    ([(0, 0, 0, 8, 8, 8)], "all", TypeError),
    ([((0.0, 0, 0), 8)], "all", TypeError),
    ([((0, 0, 0), 8.0)], "all", TypeError),
    ([((0, 0), 8)], "all", ValueError),
    ([((0, 0, 0), (8, 8))], "all", ValueError),
    ([((0, 0, 0), 0)], "all", ValueError),
    ([((0, 0, 0), (8, -8, 8))], "unseen", ValueError),
    ([((-LIMIT - 1, 0, 0), 8)], "unseen", ValueError),
    ([((LIMIT - 7, 0, 0), 8)], "unseen", ValueError),
    ([((0, 0, 0), 8)] * 4097, "unseen", ValueError),
    ([((-LIMIT, 0, 0), (2 * LIMIT, 8, 8))], "all", ValueError),
], ids=["what_int", "what_unknown", "record_what_unknown", "record_what_int", "array", "scalar", "flat", "float_lo", "float_side", "short_lo", "short_side",
        "zero_side", "negative_side", "below_limit", "above_limit", "too_many", "side_2_31"])
def test_release_refuses_bad_arguments_before_any_library_call(boxes, what, exc):
    p = bare_pipeline(field=0, size=256, dim=4.8)
    with pytest.raises(exc):
        p.release(boxes, what)


def test_release_builds_the_records():
    p = bare_pipeline(field=0, size=256, dim=4.8)
    rec = p._release_arguments(None, "unseen")
    assert (rec == records([((0, 0, 0), 256, UNSEEN)])).all() and len(rec) == 1
    rec = p._release_arguments([((8, 0, -8), (8, 16, 24)), ([0, 0, 0], 5, "all"), ((-LIMIT, -LIMIT, -LIMIT), 2 * LIMIT - 1)], "unseen")
    assert (rec == records([((8, 0, -8), (8, 16, 24), UNSEEN), ((0, 0, 0), 5, ALL), ((-LIMIT, -LIMIT, -LIMIT), (2 * LIMIT - 1,) * 3, UNSEEN)])).all() and len(rec) == 3
    assert len(p._release_arguments([], "all")) == 0 and all(record_valid(r) for r in rec[:2])


def test_cpp_mirror_release_program_compiles(tmp_path):
    """tests/cpp/release_mirror.cpp (run on the GPU by test_gpu_map_release_mirror.py) compiles against the headers for both field types."""
    for tag in ("SDF", "OFusion"):
        obj = str(tmp_path / f"rm_{tag}.o")
        r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-ffp-contract=off", f"-DSE_FIELD_TYPE={tag}", "-I" + os.path.join(ROOT, "include"),
                            "-c", os.path.join(ROOT, "tests", "cpp", "release_mirror.cpp"), "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
