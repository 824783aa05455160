"""What the tests of the map shift share (se_hip_shift_map, se::shift_map): the literal numpy truth, the list of shifts, and the numpy form
of the file route (save, move the blocks, load)."""
import numpy as np

from tests.host_util import LIMIT, box_records, closure_truth, make_keys, unpack


def leaf_level(size):
    return int(np.log2(size)) - 3


def survivors(size, s, coords, code):
    """The two survival rules: masks over the blocks [nb, 3] (corners) and the nodes (keys), and the moved corners."""
    s = np.asarray(s, np.int64)
    nc = coords.astype(np.int64).reshape(-1, 3) + s
    keep_b = ((nc >= 0) & (nc <= size - 8)).all(1)
    code = np.asarray(code, np.uint64)
    level = (code & np.uint64(0x1FF)).astype(np.int64)
    side = (size >> level)[:, None]
    corner = unpack(code & ~np.uint64(0x1FF)) + s
    keep_n = ((s[None, :] % side) == 0).all(1) & ((corner >= 0) & (corner <= size - side)).all(1)
    return keep_b, nc, keep_n, corner, level


def closure_keys(size, corners, levels):
    """Keys of the octants (corner, level) and of all their ancestors, the root left out -- make_keys level by level."""
    out = set()
    corners, levels = np.asarray(corners, np.int64).reshape(-1, 3), np.asarray(levels, np.int64)
    for l in range(1, leaf_level(size) + 1):
        sel = levels >= l
        if sel.any():
            d = size >> l
            out.update(np.unique(make_keys(corners[sel] // d * d, l)).tolist())
    return out


def closure_by_records(size, corners, levels):
    """The same closure through closure_truth of tests/host_util.py: one box per octant (for small trees: a Python loop per record)."""
    leaf = leaf_level(size)
    rows = [(tuple(int(v) for v in c), tuple(int(v) + (size >> int(l)) for v in c), 0 if int(l) == leaf else int(l)) for c, l in zip(corners, levels)]
    return closure_truth(size, box_records(rows))[1]


def shift_truth(size, s, blocks, nodes, init, closure=closure_keys):
    """se_hip_shift_map by its definition.  blocks = (coords [nb, 3], x [nb, 512], y [nb, 512], active [nb]) and nodes = (code [nn], side,
    nx [nn, 8], ny [nn, 8]) sorted by key, as DenseSLAMPipeline.blocks() / nodes() deliver them; init = initValue() as (x, y).
    Returns (blocks, nodes, counts) in the same form."""
    coords, x, y, act = blocks
    code, side, nx, ny = nodes
    s = np.asarray(s, np.int64)
    assert (np.abs(s) <= LIMIT).all() and (s % 8 == 0).all()
    if not s.any():
        return blocks, nodes, np.array([len(coords), 0, len(code), 0], np.int64)
    leaf = leaf_level(size)
    keep_b, nc, keep_n, ncorner, level = survivors(size, s, coords, code)
    kb = make_keys(nc[keep_b], leaf)
    kn = make_keys(ncorner[keep_n], 0) | level[keep_n].astype(np.uint64)
    assert not (level[keep_n] == 0).any()          # a nonzero shift never keeps the root
    all_keys = closure(size, np.concatenate([nc[keep_b], ncorner[keep_n]]), np.concatenate([np.full(int(keep_b.sum()), leaf), level[keep_n]]))
    want_b = np.array(sorted(k for k in all_keys if k & 0x1FF == leaf), np.uint64)
    want_n = np.array(sorted({0} | {k for k in all_keys if k & 0x1FF != leaf}), np.uint64)
    assert set(want_b.tolist()) == set(kb.tolist())
    ob = np.argsort(kb)
    out_blocks = (nc[keep_b][ob].astype(np.int32), x[keep_b][ob], y[keep_b][ob], act[keep_b][ob])
    out_nx = np.full((len(want_n), 8), init[0], np.float32)
    out_ny = np.full((len(want_n), 8), init[1], np.float32)
    at = np.searchsorted(want_n, kn)
    assert (want_n[at] == kn).all()
    out_nx[at], out_ny[at] = nx[keep_n], ny[keep_n]
    out_side = (size >> (want_n & np.uint64(0x1FF)).astype(np.int64)).astype(np.uint32)
    counts = np.array([keep_b.sum(), (~keep_b).sum(), keep_n.sum(), (~keep_n).sum()], np.int64)
    return out_blocks, (want_n, out_side, out_nx, out_ny), counts


def shifts_for(size):
    """The shifts every layer is tested with, in groups that are applied one after the other to one map (each group ends with a shift that
    drops everything): 0, +-8 per axis, a mixed one, one that a side-64 node is aligned to, one that side-32 nodes are aligned to but side-64
    ones are not, half the volume, +-size, +-2^30."""
    u = size // 64
    return {
        "small": [(0, 0, 0), (8, 0, 0), (-8, 0, 0), (0, 8, 0), (0, -8, 0), (0, 0, 8), (0, 0, -8), (24 * u, -40 * u, 16 * u), (0, 0, -LIMIT)],
        "aligned": [(64, 0, -64), (32, -32, 0), (LIMIT, 8, 0)],
        "half": [(0, size // 2, 0), (0, -size, 0)],
        "size": [(size, 0, 0)],
    }


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def equal_blocks_nodes(got_blocks, got_nodes, want_blocks, want_nodes):
    """Bit-for-bit equality of (coords, x, y, active) and (code, side, nx, ny); returns the name of the first field that differs, or None."""
    names = ("coords", "x", "y", "active", "code", "side", "nx", "ny")
    for name, g, w in zip(names, list(got_blocks) + list(got_nodes), list(want_blocks) + list(want_nodes)):
        g, w = np.asarray(g), np.asarray(w)
        if g.shape != w.shape:
            return f"{name}: shape {g.shape} != {w.shape}"
        if g.dtype.kind == "f":
            g, w = bits(g.astype(np.float32)), bits(w.astype(np.float32))
        if not (g == w).all():
            return name
    return None


def write_map_file(path, size, dim, field, blocks, nodes):
    """The byte layout of se_hip_save_map / Octree::save from arrays in key order (field 0: SDF {float, float}; 1: OFusion {float, pad, double})."""
    coords, x, y, _ = blocks
    code, side, nx, ny = nodes
    vt = np.dtype([("x", "<f4"), ("y", "<f4")]) if field == 0 else np.dtype([("x", "<f4"), ("pad", "<u4"), ("y", "<f8")])
    nt = np.dtype([("code", "<u8"), ("side", "<i4"), ("v", vt, 8)])
    bt = np.dtype([("code", "<u8"), ("c", "<i4", 3), ("v", vt, 512)])
    nrec = np.zeros(len(code), nt)
    nrec["code"], nrec["side"], nrec["v"]["x"], nrec["v"]["y"] = code, side, nx, ny
    brec = np.zeros(len(coords), bt)
    brec["code"], brec["c"], brec["v"]["x"], brec["v"]["y"] = make_keys(coords, leaf_level(size)), coords, x, y
    with open(path, "wb") as f:
        f.write(np.int32(size).tobytes()); f.write(np.float32(dim).tobytes())
        f.write(np.uint64(len(nrec)).tobytes()); f.write(nrec.tobytes())
        f.write(np.uint64(len(brec)).tobytes()); f.write(brec.tobytes())
