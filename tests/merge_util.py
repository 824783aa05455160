"""What the tests of the map merge share (se_hip_merge_map, se::merge_map): the literal numpy truth -- the value-pair function element-wise in
float32 (contraction-free by nature) and the block / node rules of include/se_hip.h -- and the numpy form of the file route (save both,
combine, load)."""
import numpy as np

from tests.host_util import LIMIT, make_keys, unpack
from tests.shift_util import closure_keys, leaf_level

FUSE, REPLACE, FILL = 0, 1, 2
MODES = {"fuse": FUSE, "replace": REPLACE, "fill": FILL}
INIT = {0: (1.0, 0.0), 1: (0.0, 0.0)}        # voxel_traits<T>::initValue(): SDF, OFusion
COUNT_NAMES = ("blocks_combined", "blocks_created", "blocks_clipped", "nodes_combined", "nodes_created", "nodes_skipped")


def _clamp(v, lo, hi):
    """clamp(v, lo, hi) = std::max(lo, std::min(v, hi)) with the comparisons of <algorithm>."""
    lo, hi = np.float32(lo), np.float32(hi)
    t = np.where(hi < v, hi, v)
    return np.where(lo < t, t, lo).astype(np.float32)


def unseen(x, y, field):
    ix, iy = INIT[field]
    return (x == np.float32(ix)) & (y == np.float32(iy))


def merge_values(ax, ay, bx, by, mode, field, max_weight=100):
    """The value-pair function: a = destination, b = source, float32 arrays of one shape.  Returns (x, y)."""
    ax, ay, bx, by = (np.asarray(v, np.float32) for v in (ax, ay, bx, by))
    maxw = np.float32(max_weight)
    a_un, b_un = unseen(ax, ay, field), unseen(bx, by, field)
    ty = np.fmin(by, maxw) if field == 0 else by
    if mode == REPLACE:
        ox, oy = bx, ty
    elif mode == FILL:
        ox, oy = ax, ay
    elif field == 0:
        with np.errstate(all="ignore"):
            w = ay + by
            mean = (ay * ax + by * bx) / w
        ox, oy = _clamp(mean, -1.0, 1.0), np.fmin(w, maxw)
        ox, oy = np.where(ay == 0, bx, ox), np.where(ay == 0, ty, oy)
        ox, oy = np.where(by == 0, ax, ox), np.where(by == 0, ay, oy)
    else:
        ox, oy = _clamp(ax + bx, -1000.0, 1000.0), np.fmax(ay, by)
    ox, oy = np.where(a_un, bx, ox), np.where(a_un, ty, oy)
    ox, oy = np.where(b_un, ax, ox), np.where(b_un, ay, oy)
    return ox.astype(np.float32), oy.astype(np.float32)


def participants(dsize, ssize, s, coords, code):
    """Which source blocks (corners [nb, 3]) and source nodes (keys) take part: (keep_b, moved corners, keep_n, moved node corners,
    the nodes' levels in the destination)."""
    s = np.asarray(s, np.int64)
    nc = coords.astype(np.int64).reshape(-1, 3) + s
    keep_b = ((nc >= 0) & (nc <= dsize - 8)).all(1)
    code = np.asarray(code, np.uint64)
    slevel = (code & np.uint64(0x1FF)).astype(np.int64)
    side = ssize >> slevel
    corner = unpack(code & ~np.uint64(0x1FF)) + s
    keep_n = ((s[None, :] % side[:, None]) == 0).all(1) & ((corner >= 0) & (corner <= dsize - side[:, None])).all(1)
    keep_n &= (slevel >= 1) | ((dsize == ssize) and not s.any())          # the source root: only for s = 0 and equal sizes
    dlevel = int(np.log2(dsize)) - np.log2(np.maximum(side, 1)).astype(np.int64)
    return keep_b, nc, keep_n, corner, dlevel


def merge_truth(dsize, dst_blocks, dst_nodes, ssize, src_blocks, src_nodes, s, mode, field, max_weight=100):
    """se_hip_merge_map by its definition.  blocks = (coords [nb, 3], x [nb, 512], y [nb, 512], active [nb]) and nodes = (code [nn], side,
    nx [nn, 8], ny [nn, 8]) sorted by key, as DenseSLAMPipeline.blocks() / nodes() deliver them.
    Returns (blocks, nodes, counts int64 [12]) of the destination afterwards, in the same form."""
    dc, dx, dy, dact = dst_blocks
    dcode, _, dnx, dny = dst_nodes
    sc, sx, sy, sact = src_blocks
    scode, _, snx, sny = src_nodes
    s = np.asarray(s, np.int64)
    assert (np.abs(s) <= LIMIT).all() and (s % 8 == 0).all() and mode in (FUSE, REPLACE, FILL)
    ix, iy = INIT[field]
    leaf = leaf_level(dsize)
    keep_b, nc, keep_n, ncorner, dlevel = participants(dsize, ssize, s, sc, scode)
    kb = make_keys(nc[keep_b], leaf)
    kn = make_keys(ncorner[keep_n], 0) | dlevel[keep_n].astype(np.uint64)
    dkeys = make_keys(dc, leaf)
    assert (np.diff(dkeys.astype(np.int64)) > 0).all() and (np.diff(dcode.astype(np.int64)) > 0).all()

    # the block set and the node set afterwards: what was there, the participants, and all their ancestors
    closure = closure_keys(dsize, np.concatenate([nc[keep_b], ncorner[keep_n]]), np.concatenate([np.full(int(keep_b.sum()), leaf), dlevel[keep_n]]))
    out_bk = np.array(sorted(set(dkeys.tolist()) | set(kb.tolist())), np.uint64)
    out_nk = np.array(sorted(set(dcode.tolist()) | {0} | {k for k in closure if k & 0x1FF != leaf}), np.uint64)
    assert {k for k in closure if k & 0x1FF == leaf} == set(kb.tolist())

    nbo, nno = len(out_bk), len(out_nk)
    ox, oy = np.full((nbo, 512), ix, np.float32), np.full((nbo, 512), iy, np.float32)
    oact = np.ones(nbo, np.uint8)                                        # a created block is active, as insertion leaves it
    at_d = np.searchsorted(out_bk, dkeys)
    ox[at_d], oy[at_d], oact[at_d] = dx, dy, dact
    at_s = np.searchsorted(out_bk, kb)
    existed = np.isin(kb, dkeys)
    ox[at_s], oy[at_s] = merge_values(ox[at_s], oy[at_s], sx[keep_b], sy[keep_b], mode, field, max_weight)
    oact[at_s] = oact[at_s] | (sact[keep_b] != 0)
    ocoords = unpack(out_bk & ~np.uint64(0x1FF)).astype(np.int32)

    onx, ony = np.full((nno, 8), ix, np.float32), np.full((nno, 8), iy, np.float32)
    at_dn = np.searchsorted(out_nk, dcode)
    onx[at_dn], ony[at_dn] = dnx, dny
    at_sn = np.searchsorted(out_nk, kn)
    assert (out_nk[at_sn] == kn).all() and len(set(kn.tolist())) == len(kn)
    n_existed = np.isin(kn, dcode)
    onx[at_sn], ony[at_sn] = merge_values(onx[at_sn], ony[at_sn], snx[keep_n], sny[keep_n], mode, field, max_weight)
    oside = (dsize >> (out_nk & np.uint64(0x1FF)).astype(np.int64)).astype(np.uint32)

    counts = np.zeros(12, np.int64)
    counts[:6] = [existed.sum(), (~existed).sum(), (~keep_b).sum(), n_existed.sum(), (~n_existed).sum(), (~keep_n).sum()]
    if keep_b.any():
        counts[6:9], counts[9:12] = nc[keep_b].min(0), nc[keep_b].max(0) + 8
    return (ocoords, ox, oy, oact), (out_nk, oside, onx, ony), counts


def counts_of(result):
    """The dict DenseSLAMPipeline.merge returns -> int64 [12] in the order of the C ABI."""
    return np.array([result[k] for k in COUNT_NAMES] + list(result["region"][0]) + list(result["region"][1]), np.int64)


def both_observed(dsize, dst_blocks, ssize, src_blocks, s, field):
    """Voxels observed in both maps among the participating blocks that exist in the destination."""
    dc, dx, dy, _ = dst_blocks
    sc, sx, sy, _ = src_blocks
    keep_b, nc = participants(dsize, ssize, s, sc, np.zeros(0, np.uint64))[:2]
    leaf = leaf_level(dsize)
    dkeys, kb = make_keys(dc, leaf), make_keys(nc[keep_b], leaf)
    hit = np.isin(kb, dkeys)
    at = np.searchsorted(dkeys, kb[hit])
    return int((~unseen(dx[at], dy[at], field) & ~unseen(sx[keep_b][hit], sy[keep_b][hit], field)).sum())
