"""What the tests of the column projections share (se_hip_project_columns / DenseSLAMPipeline.project): the numpy truth of a request over a
dense class grid (the definition; the grid is motion_util.class_grid or a hand grid, padded with unseen), the hand maps -- stamped on 64^3
handles without depth, by allocate + edit -- with their class grids, the hand-worked cells of tests/cpp/project_kats.cpp, the requests of the
hand cases, and the conditions the inputs of the GPU tests have to meet."""
import numpy as np

OCC, UNSEEN, EMPTY = 0, 1, 2
NONE = -(1 << 31)
LIMIT = 1 << 20
STOPS = (("occupied", OCC), ("unseen", UNSEEN))
OUTPUTS = ("status", "first", "last", "count")

# ------------------------------------------------------------------ hand maps (64^3): boxes lo xyz, hi xyz, half open
#   free       blocks allocated and every voxel set empty;        occupied   voxels of allocated blocks set occupied
#   gap        voxels of allocated blocks back to initValue();    node_occ / node_empty   a level-2 octant (side 16) allocated as a node without
#   children, its eight value_ edited to occupied / empty: the blocks under it are absent and read that value.  Everything else is absent
#   under a node that holds initValue(): unseen.
HAND_N = 64
HAND_MAPS = {
    "mix": dict(free=[(0, 0, 0, 32, 32, 32)], occupied=[(10, 10, 10, 11, 11, 11), (12, 12, 12, 15, 15, 15), (3, 20, 27, 9, 21, 29)], gap=[(24, 0, 0, 32, 8, 8)],
                node_occ=[(32, 32, 32, 48, 48, 48)], node_empty=[(48, 48, 48, 64, 64, 64)]),
    "split": dict(free=[(32, 0, 0, 64, 32, 32)], occupied=[(40, 20, 9, 41, 21, 10), (50, 4, 20, 53, 7, 23)], gap=[(32, 24, 24, 40, 32, 32)],
                  node_occ=[(0, 48, 16, 16, 64, 32)], node_empty=[(16, 0, 48, 32, 16, 64)]),
}

LAYERS8 = [(3, 13), (8, 16), (7, 8), (0, 64), (-9, 70), (-12, -2), (70, 75), (-LIMIT, LIMIT)]
LAYERS16 = LAYERS8 + [(32, 48), (48, 64), (16, 32), (40, 56), (10, 11), (12, 15), (63, 64), (31, 33)]
LAYERS15 = [l for l in LAYERS16 if l != (-LIMIT, LIMIT)]
# footprints (lo_u, lo_v, side_u, side_v): side 1; not aligned to 8 on either edge; not square; the whole volume; overhanging each of the four
# sides by 5; wholly outside (above on u, below on both)
FOOTPRINTS = {"one": (10, 10, 1, 1), "ragged": (3, 3, 13, 13), "oblong": (3, 30, 13, 21), "whole": (0, 0, 64, 64), "overhang": (-5, -5, 74, 74),
              "outside_hi": (70, 3, 9, 9), "outside_lo": (-20, -20, 7, 7)}

# hand-worked cells on "mix" along z (tests/cpp/project_kats.cpp works them out): name -> (u, v, (a, b), answer with stop_at occupied, answer
# with stop_at unseen), an answer = (status, first, last, count)
HAND_CELLS = {
    "OneVoxel": (10, 10, (3, 13), (OCC, 10, 10, 1), (OCC, 10, 10, 1)),
    "CubeColumn": (13, 13, (0, 64), (OCC, 12, 14, 3), (OCC, 12, 63, 35)),
    "FreeColumn": (20, 5, (8, 16), (EMPTY, NONE, NONE, 0), (EMPTY, NONE, NONE, 0)),
    "GapColumn": (25, 3, (3, 13), (UNSEEN, NONE, NONE, 0), (UNSEEN, 3, 7, 5)),
    "OctantOccupied": (40, 40, (0, 64), (OCC, 32, 47, 16), (OCC, 0, 63, 64)),
    "OctantOccupiedInside": (40, 40, (40, 56), (OCC, 40, 47, 8), (OCC, 40, 55, 16)),
    "OctantEmpty": (50, 50, (48, 64), (EMPTY, NONE, NONE, 0), (EMPTY, NONE, NONE, 0)),
    "OctantEmptyAcross": (50, 50, (-9, 70), (UNSEEN, NONE, NONE, 0), (UNSEEN, -9, 69, 63)),
    "Below": (10, 10, (-12, -2), (UNSEEN, NONE, NONE, 0), (UNSEEN, -12, -3, 10)),
    "Above": (10, 10, (70, 75), (UNSEEN, NONE, NONE, 0), (UNSEEN, 70, 74, 5)),
    "OutsideColumn": (-3, 10, (3, 13), (UNSEEN, NONE, NONE, 0), (UNSEEN, 3, 12, 10)),
    "Everything": (10, 10, (-LIMIT, LIMIT), (OCC, 10, 10, 1), (OCC, -LIMIT, LIMIT - 1, 2 * LIMIT - 64 + 33)),
}


def axis_box(axis, box):
    """(u range, v range, w range) of a box lo xyz, hi xyz for columns along `axis`."""
    r = [(box[k], box[k + 3]) for k in range(3)]
    rest = [k for k in range(3) if k != axis]
    return r[rest[0]], r[rest[1]], r[axis]


def hand_grid(name):
    """The class grid [z][y][x] of the hand map `name`."""
    spec = HAND_MAPS[name]
    g = np.full((HAND_N,) * 3, UNSEEN, np.uint8)
    for key, cls in (("free", EMPTY), ("occupied", OCC), ("gap", UNSEEN), ("node_occ", OCC), ("node_empty", EMPTY)):
        for x0, y0, z0, x1, y1, z1 in spec.get(key, []):
            g[z0:z1, y0:y1, x0:x1] = cls
    return g


def stamp_hand_map(p, name, occupied_x, empty_x):
    """The hand map `name` on a fresh 64^3 handle, built without depth."""
    spec = HAND_MAPS[name]
    box = lambda rows: np.array(rows, np.int32).reshape(-1, 6)
    p.allocate(box(spec["free"]))
    p.edit(box(spec["free"]), empty_x, 1.0)
    p.edit(box(spec["occupied"]), occupied_x, 1.0)
    p.reset(box(spec["gap"]))
    for key, x in (("node_occ", occupied_x), ("node_empty", empty_x)):
        p.allocate(box(spec[key]), level=2)
        p.edit(box(spec[key]), x, 1.0, blocks=False, nodes=True)


def stamp_octants(p, n, occupied_x, empty_x):
    """On a fused n^3 map: the two octants of side 16 of stamps(n) allocated as nodes (where nothing is there yet) and their value_
    edited to occupied and to empty, so that the absent blocks under them read those values."""
    level = int(np.log2(n)) - 4
    for box, x in zip(stamps(n), (occupied_x, empty_x)):
        b = np.array([box], np.int32)
        p.allocate(b, level=level)
        p.edit(b, x, 1.0, blocks=False, nodes=True)


def stamps(n):
    """(the octant stamped occupied, the octant stamped empty) of stamp_octants, lo xyz, hi xyz: cubes on the volume's diagonal, so that they
    look the same along every axis."""
    return (0, 0, 0, 16, 16, 16), (n - 32, n - 32, n - 32, n - 16, n - 16, n - 16)


def project_truth(grid, axis, lo, side, layers, stop_at):
    """The definition over a dense class grid ([z][y][x] uint8 of the n^3 volume; every voxel outside it is unseen): a dict of the four
    arrays [L][side_v][side_u].  The footprint's columns are cut out of the grid padded with unseen; the part of a layer below 0 and from n
    on, where every voxel is unseen, is counted instead of materialised (a layer may be 2^21 voxels long)."""
    n = grid.shape[0]
    g = grid.transpose({2: (1, 2, 0), 1: (0, 2, 1), 0: (0, 1, 2)}[axis])                # [v][u][w]
    (lu, lv), (su, sv) = lo, side
    foot = np.full((sv, su, n), UNSEEN, np.uint8)
    u0, u1, v0, v1 = max(lu, 0), min(lu + su, n), max(lv, 0), min(lv + sv, n)
    if u0 < u1 and v0 < v1:
        foot[v0 - lv:v1 - lv, u0 - lu:u1 - lu] = g[v0:v1, u0:u1]
    out = {k: np.empty((len(layers), sv, su), np.uint8 if k == "status" else np.int32) for k in OUTPUTS}
    for l, (a, b) in enumerate(layers):
        a0, b1 = max(a, 0), min(b, n)
        below, above = max(0, min(b, 0) - a), max(0, b - max(a, n))
        status = np.full((sv, su), EMPTY, np.uint8)
        first = np.full((sv, su), NONE, np.int64)
        last = np.full((sv, su), NONE, np.int64)
        count = np.zeros((sv, su), np.int64)
        if a0 < b1:
            inner = foot[:, :, a0:b1]
            status = inner.min(-1)
            blocking = inner <= stop_at
            count = blocking.sum(-1).astype(np.int64)
            some = count > 0
            first = np.where(some, a0 + blocking.argmax(-1), NONE)
            last = np.where(some, b1 - 1 - blocking[:, :, ::-1].argmax(-1), NONE)
        if below + above:
            status = np.minimum(status, UNSEEN)
            if stop_at >= UNSEEN:
                if below:
                    last = np.where(count > 0, last, min(b, 0) - 1)
                    first = np.full((sv, su), a, np.int64)
                    count = count + below
                if above:
                    first = np.where(count > 0, first, max(a, n))
                    last = np.full((sv, su), b - 1, np.int64)
                    count = count + above
        out["status"][l], out["first"][l], out["last"][l], out["count"][l] = status, first, last, count
    return out


def conditions(n, axis, lo, side, layers, stop_at, truth, occ_box, empty_box):
    """What a request's truth has to contain for a comparison with it to mean something; a dict of counts, each of which must be nonzero:
    cells of each status, with first < last, first == last and none, cells inside the footprint of the octant stamped occupied (empty) whose
    layer lies inside it -- their answer is that node value alone -- and cells that leave the volume below and above."""
    st, first, last, count = (truth[k] for k in OUTPUTS)
    seen = {"occupied": int((st == OCC).sum()), "unseen": int((st == UNSEEN).sum()), "empty": int((st == EMPTY).sum()),
            "first_lt_last": int((first < last).sum()), "first_eq_last": int(((first == last) & (count > 0)).sum()), "none": int((count == 0).sum()),
            "below": sum(1 for a, b in layers if a < 0), "above": sum(1 for a, b in layers if b > n)}
    (lu, lv), (su, sv) = lo, side
    for key, box, cls in (("octant_occupied", occ_box, OCC), ("octant_empty", empty_box, EMPTY)):
        (u0, u1), (v0, v1), (w0, w1) = axis_box(axis, box)
        k = 0
        for l, (a, b) in enumerate(layers):
            if not (w0 <= a and b <= w1):
                continue
            cells = (slice(max(v0 - lv, 0), max(min(v1 - lv, sv), 0)), slice(max(u0 - lu, 0), max(min(u1 - lu, su), 0)))
            s, c = st[l][cells], count[l][cells]
            assert (s == cls).all() and (c == (b - a if cls <= stop_at else 0)).all(), (key, axis, (a, b))
            k += s.size
        seen[key] = k
    return seen


def check_identities(out, stop_at):
    """The relations among the four arrays of one answer."""
    st, first, last, count = (np.asarray(out[k]).astype(np.int64) for k in OUTPUTS)
    none = count == 0
    assert ((first == NONE) == none).all() and ((last == NONE) == none).all()
    assert (first[~none] <= last[~none]).all()
    assert (count[~none] <= last[~none] - first[~none] + 1).all()
    assert (count >= 0).all()
    if stop_at == OCC:
        assert ((st == OCC) == (count > 0)).all()
    else:
        assert ((st <= UNSEEN) == (count > 0)).all()


def merged(lower, upper):
    """What the two parts [a, w) and [w, b) of a layer give for [a, b): the min of the statuses, the sum of the counts, the min / max of first
    / last (NONE = INT32_MIN is the neutral element of max; for min it is mapped away)."""
    f = lambda x: np.where(x == NONE, np.int64(1) << 40, x.astype(np.int64))
    first = np.minimum(f(lower["first"]), f(upper["first"]))
    return {"status": np.minimum(lower["status"], upper["status"]), "count": lower["count"].astype(np.int64) + upper["count"],
            "first": np.where(first == np.int64(1) << 40, NONE, first), "last": np.maximum(lower["last"].astype(np.int64), upper["last"])}


def cell_boxes(axis, lo, side, layers):
    """The 1 x 1 x (b - a) box of every cell, [L * side_v * side_u, 6] int32 lo xyz, side xyz, in the order of the outputs."""
    (lu, lv), (su, sv) = lo, side
    rows = []
    for a, b in layers:
        v, u = np.meshgrid(np.arange(lv, lv + sv), np.arange(lu, lu + su), indexing="ij")
        u, v = u.reshape(-1), v.reshape(-1)
        w, one, h = np.full_like(u, a), np.ones_like(u), np.full_like(u, b - a)
        cols = {2: (u, v, w, one, one, h), 1: (u, w, v, one, h, one), 0: (w, u, v, h, one, one)}[axis]
        rows.append(np.stack(cols, 1))
    return np.ascontiguousarray(np.concatenate(rows).astype(np.int32))
