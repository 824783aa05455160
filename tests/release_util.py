"""What the tests of the release share (se_hip_release_boxes, se::release_map): the literal numpy truth, the record lists, and -- from
tests/shift_util.py -- the numpy form of the file route (write_map_file) and the bit-for-bit comparison."""
import numpy as np

from tests.host_util import make_keys, unpack
from tests.shift_util import bits, equal_blocks_nodes, leaf_level, write_map_file  # noqa: F401  (re-exported for the tests)

ALL, UNSEEN = 1, 2          # SE_HIP_RELEASE_*
LIMIT = 1 << 30
MAX_BOXES = 4096


def records(rows):
    """[(lo, side, what[, reserved])] -> RELEASE_DTYPE records; side a scalar or three values.  Nothing is checked: invalid records are made this way."""
    from supereight_amd.pipeline import RELEASE_DTYPE
    rec = np.zeros(len(rows), RELEASE_DTYPE)
    for i, r in enumerate(rows):
        rec[i]["lo"], rec[i]["side"], rec[i]["what"] = r[0], r[1], r[2]
        rec[i]["reserved"] = r[3] if len(r) > 3 else 0
    return rec


def record_valid(r):
    lo, side = r["lo"].astype(np.int64), r["side"].astype(np.int64)
    return bool((side >= 1).all() and (lo >= -LIMIT).all() and (lo + side <= LIMIT).all() and int(r["what"]) in (ALL, UNSEEN) and int(r["reserved"]) == 0)


INVALID_ROWS = [
    ((0, 0, 0), (0, 8, 8), ALL), ((0, 0, 0), (8, -1, 8), UNSEEN), ((0, 0, 0), (8, 8, 8), 0), ((0, 0, 0), (8, 8, 8), 3), ((0, 0, 0), (8, 8, 8), -1),
    ((0, 0, 0), (8, 8, 8), ALL, 1), ((-LIMIT - 1, 0, 0), (8, 8, 8), ALL), ((0, LIMIT - 7, 0), (8, 8, 8), UNSEEN), ((0, 0, 1), (8, 8, 2 ** 31 - 1), ALL),
    ((0, 0, -2 ** 31), (8, 8, 8), ALL),
]


def _contains(rec, corner, side):
    """[n_octants, n_records]: record r contains the octant with that corner and side."""
    lo = rec["lo"].astype(np.int64)[None, :, :]
    hi = lo + rec["side"].astype(np.int64)[None, :, :]
    c = np.asarray(corner, np.int64).reshape(-1, 1, 3)
    d = np.asarray(side, np.int64).reshape(-1, 1, 1)
    return ((c >= lo) & (c + d <= hi)).all(2)


def release_truth(size, rec, blocks, nodes, init):
    """se_hip_release_boxes by its definition.  rec = RELEASE_DTYPE records, all valid, at most 4096; blocks = (coords [nb, 3], x [nb, 512],
    y [nb, 512], active [nb]) and nodes = (code [nn], side, nx [nn, 8], ny [nn, 8]) sorted by key, as DenseSLAMPipeline.blocks() / nodes()
    deliver them; init = initValue() as (x, y).  Returns (blocks, nodes, counts [5], touched [6], info) in the same form; info counts the
    parent entries reset and those of them that were not initValue() before."""
    coords, x, y, act = blocks
    code, side, nx, ny = nodes
    assert len(rec) <= MAX_BOXES and all(record_valid(r) for r in rec)
    leaf = leaf_level(size)
    ix, iy = bits(np.float32(init[0]))[0], bits(np.float32(init[1]))[0]
    nb, nn = len(coords), len(code)
    is_all = rec["what"] == ALL
    # blocks
    cb = _contains(rec, coords, np.full(nb, 8))
    empty_b = (bits(x.astype(np.float32)) == ix).all(1) & (bits(y.astype(np.float32)) == iy).all(1) if nb else np.zeros(0, bool)
    gone_b = (cb & is_all[None, :]).any(1) | (cb.any(1) & empty_b)
    # nodes
    level = (code & np.uint64(0x1FF)).astype(np.int64)
    corner = unpack(code & ~np.uint64(0x1FF))
    nside = size >> level
    cn = _contains(rec, corner, nside)
    empty_n = (bits(nx.astype(np.float32)) == ix).all(1) & (bits(ny.astype(np.float32)) == iy).all(1)
    releasable = ((cn & is_all[None, :]).any(1) | (cn.any(1) & empty_n)) & (level > 0)
    index = {int(k): i for i, k in enumerate(code.tolist())}

    def parents(corners, lvl):
        """Index of the parent node of every octant (corner, level lvl >= 1), and the child number of the octant in it."""
        d = size >> (lvl - 1)
        pk = make_keys(corners // d * d, lvl - 1)
        child = ((corners // (d // 2)) & 1) @ np.array([1, 2, 4])
        return np.array([index[int(k)] for k in pk.tolist()], np.int64), child

    stays = ~releasable
    pb, childb = parents(coords.astype(np.int64), leaf) if nb else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    stays[pb[~gone_b]] = True
    for l in range(leaf - 1, 0, -1):          # bottom-up: a node with a survivor beneath it stays
        sel = np.nonzero((level == l) & stays)[0]
        if len(sel):
            stays[parents(corner[sel], l)[0]] = True
    assert stays[level == 0].all() and (level == 0).sum() == 1
    # the entries of surviving parents above released octants
    out_nx, out_ny = nx.astype(np.float32).copy(), ny.astype(np.float32).copy()
    reset, reset_valued = 0, 0
    pairs = [(pb[gone_b], childb[gone_b])]
    for l in range(1, leaf):
        sel = np.nonzero((level == l) & ~stays)[0]
        if len(sel):
            pairs.append(parents(corner[sel], l))
    for pi, ch in pairs:
        live = stays[pi]
        pi, ch = pi[live], ch[live]
        reset += len(pi)
        reset_valued += int(((bits(out_nx[pi, ch]) != ix) | (bits(out_ny[pi, ch]) != iy)).sum())
        out_nx[pi, ch], out_ny[pi, ch] = np.float32(init[0]), np.float32(init[1])
    # the closure holds by construction: the parent of every survivor survives
    for l in range(1, leaf):
        sel = np.nonzero((level == l) & stays)[0]
        assert len(sel) == 0 or stays[parents(corner[sel], l)[0]].all()
    assert stays[pb[~gone_b]].all()
    kb = ~gone_b
    out_blocks = (coords[kb], x[kb], y[kb], act[kb])
    out_nodes = (code[stays], side[stays], out_nx[stays], out_ny[stays])
    counts = np.array([kb.sum(), gone_b.sum(), stays.sum(), (~stays).sum(), (gone_b & ~empty_b).sum()], np.int64)
    touched = np.zeros(6, np.int64)
    if gone_b.any():
        touched[:3], touched[3:] = coords[gone_b].min(0), coords[gone_b].max(0) + 8
    return out_blocks, out_nodes, counts, touched, {"reset": reset, "reset_valued": reset_valued, "empty_blocks": int(empty_b.sum())}


def get_truth(size, blocks, nodes, pts):
    """Octree::get at integer voxels pts [n, 3]: the voxel of the block that holds it, else value_[child] of the deepest node on the way down."""
    coords, x, y, _ = blocks
    code, _, nx, ny = nodes
    leaf = leaf_level(size)
    bindex = {int(k): i for i, k in enumerate(make_keys(coords, leaf).tolist())}
    nindex = {int(k): i for i, k in enumerate(code.tolist())}
    out = np.zeros((len(pts), 2), np.float32)
    for i, p in enumerate(np.asarray(pts, np.int64)):
        at = nindex[0]
        for l in range(1, leaf + 1):
            d = size >> l
            child = int(((p // d) & 1) @ np.array([1, 2, 4]))
            key = int(make_keys((p // d * d)[None, :], l)[0])
            nxt = bindex.get(key) if l == leaf else nindex.get(key)
            if nxt is None:
                out[i] = nx[at, child], ny[at, child]
                break
            at = nxt
        else:
            v = int((p % 8) @ np.array([1, 8, 64]))
            out[i] = x[at, v], y[at, v]
    return out


def record_sets(n):
    """The record lists the device tests cover, by name, for a volume of side n."""
    rng = np.random.default_rng(3)
    q = n // 4
    mixed = [((0, 0, 0), n, UNSEEN), ((q, q, q), 2 * q, ALL), ((q, q, q), 2 * q, ALL), ((q + 8, q, q), (2 * q, 16, 24), UNSEEN)]
    while len(mixed) < 70:
        lo = rng.integers(-8, n, 3)
        mixed.append((tuple(int(v) for v in lo), tuple(int(v) for v in rng.integers(1, n // 2, 3)), int(rng.choice([ALL, UNSEEN]))))
    rng.shuffle(mixed)
    small = [((int(8 * i), 0, 0), (8, n, n), UNSEEN) for i in range(n // 8)]
    while len(small) < 65:
        small.append(small[len(small) % (n // 8)])
    return {
        "unseen_everywhere": [((0, 0, 0), n, UNSEEN)],
        "all_centre": [((q, q, q), 2 * q, ALL)],
        "all_one_short": [((q, q, q), (2 * q - 1, 2 * q, 2 * q), ALL)],
        "all_everything": [((0, 0, 0), n, ALL)],
        "mixed_70": mixed,
        "exactly_64": small[:63] + [((q, q, q), 2 * q, ALL)],
        "exactly_65": small[:64] + [((q, q, q), 2 * q, ALL)],
    }
