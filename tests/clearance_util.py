"""What the tests of the clearance queries share (se_hip_clearance_boxes / DenseSLAMPipeline.clearance): the hand-worked cases of
tests/cpp/clearance_kats.cpp with their answers, the maps they stand on, the numpy truth of a query over a dense class grid (the definition,
in int64), and the identities that tie a clearance to the strict box query."""
import numpy as np

from tests.motion_util import HAND_MAPS, stamp_hand_map

LIMIT = 1 << 19
R_MAX = 32767
NONE, INVALID = -1, -2
I32_MIN = -(1 << 31)
NOWHERE = (I32_MIN, I32_MIN, I32_MIN)
OCC, UNSEEN, EMPTY = 0, 1, 2
_NO = (NONE, NOWHERE)
_BAD = (INVALID, NOWHERE)

# the maps of the hand cases: four of motion_util.HAND_MAPS and `octant` -- nothing allocated but the level-2 octant [32, 48)^3, a node
# without children whose eight value_ are occupied
CLEAR_MAPS = ("a", "wall", "free", "gap", "octant")
OCTANT_BOX = (32, 32, 32, 48, 48, 48)

# case -> (map, lo, side, r_max, (d2, nearest) with stop_at occupied, (d2, nearest) with stop_at unseen); worked by hand in the header comment
# of tests/cpp/clearance_kats.cpp
HAND_CASES = {
    "CornerR15": ("a", (0, 0, 0), (1, 1, 1), 15, _NO, (0, (-1, -1, -1))),
    "CornerR16": ("a", (0, 0, 0), (1, 1, 1), 16, (243, (10, 10, 10)), (0, (-1, -1, -1))),
    "CornerR32767": ("a", (0, 0, 0), (1, 1, 1), R_MAX, (243, (10, 10, 10)), (0, (-1, -1, -1))),
    "Overlap": ("a", (9, 9, 9), (2, 2, 2), 0, (0, (10, 10, 10)), (0, (10, 10, 10))),
    "TouchFace": ("a", (11, 10, 10), (2, 2, 2), 0, (0, (10, 10, 10)), (0, (10, 10, 10))),
    "TouchCorner": ("a", (11, 11, 11), (1, 1, 1), 0, (0, (10, 10, 10)), (0, (10, 10, 10))),
    "OneAwayR0": ("a", (12, 10, 10), (1, 1, 1), 0, _NO, _NO),
    "OneAwayR1": ("a", (12, 10, 10), (1, 1, 1), 1, (1, (10, 10, 10)), (1, (10, 10, 10))),
    "WallTie": ("wall", (10, 5, 5), (2, 2, 2), 10, (64, (20, 4, 4)), (25, (9, 4, -1))),
    "WallTieAcrossBlocks": ("wall", (10, 7, 7), (2, 2, 2), 10, (64, (20, 6, 6)), (49, (9, 6, -1))),
    "FreeR30": ("free", (30, 30, 30), (2, 2, 2), 30, _NO, (900, (29, 29, -1))),
    "FreeR29": ("free", (30, 30, 30), (2, 2, 2), 29, _NO, _NO),
    "GapBox": ("gap", (10, 3, 3), (1, 1, 1), 32, (841, (40, 3, 3)), (9, (9, 2, -1))),
    "OctantCorner": ("octant", (20, 22, 25), (2, 2, 2), 14, (189, (32, 32, 32)), (0, (19, 21, 24))),
    "OctantClamped": ("octant", (36, 20, 50), (2, 2, 2), 11, (104, (35, 32, 47)), (0, (35, 19, 49))),
    "LimitLow": ("a", (-LIMIT, 5, 5), (1, 1, 1), 5, _NO, (0, (-LIMIT - 1, 4, 4))),
    "LimitHigh": ("a", (LIMIT - 1, 5, 5), (1, 1, 1), 5, _NO, (0, (LIMIT - 2, 4, 4))),
    "BeyondLimitLo": ("a", (-LIMIT - 1, 5, 5), (1, 1, 1), 5, _BAD, _BAD),
    "BeyondLimitHi": ("a", (LIMIT, 5, 5), (1, 1, 1), 5, _BAD, _BAD),
    "R32768": ("a", (0, 0, 0), (1, 1, 1), R_MAX + 1, _BAD, _BAD),
    "RNegative": ("a", (0, 0, 0), (1, 1, 1), -1, _BAD, _BAD),
    "ZeroSide": ("a", (5, 5, 5), (1, 0, 1), 5, _BAD, _BAD),
}


def stamp_clear_map(p, name, occupied_x, empty_x):
    """The hand map `name` on a fresh 64^3 handle, built without depth."""
    if name != "octant":
        return stamp_hand_map(p, HAND_MAPS[name], occupied_x, empty_x)
    box = np.array([OCTANT_BOX], np.int32)
    p.allocate(box, level=2)
    p.edit(box, occupied_x, 1.0, blocks=False, nodes=True)


def hand_grid(name):
    """The class grid [z][y][x] of the hand map `name`."""
    if name == "octant":
        g = np.full((64, 64, 64), UNSEEN, np.uint8)
        x0, y0, z0, x1, y1, z1 = OCTANT_BOX
        g[z0:z1, y0:y1, x0:x1] = OCC
        return g
    spec = HAND_MAPS[name]
    g = np.full((64, 64, 64), EMPTY, np.uint8)
    for x, y, z in spec.get("occupied", []):
        g[z, y, x] = OCC
    if "wall" in spec:
        g[:, :, spec["wall"]] = OCC
    if "gap" in spec:
        x0, y0, z0, x1, y1, z1 = spec["gap"]
        g[z0:z1, y0:y1, x0:x1] = UNSEEN
    return g


def valid(q):
    lo, side, r = np.asarray(q[0:3], np.int64), np.asarray(q[3:6], np.int64), int(q[6])
    return bool((side >= 1).all() and (np.abs(lo) <= LIMIT).all() and (np.abs(lo + side) <= LIMIT).all() and 0 <= r <= R_MAX)


def _gaps(lo, side, c):
    """g = max(0, c - (lo + side), lo - (c + 1)) of the voxels c along one axis."""
    return np.maximum(0, np.maximum(c - (lo + side), lo - (c + 1)))


def clearance_truth(grid, q, stop_at):
    """The definition over a dense class grid ([z][y][x] uint8 numpy array of the n^3 volume; outside it every voxel is unseen), in int64:
    (d2, nearest, how many blocking voxels attain d2) of the query q = lo, side, r_max.  Every voxel of the box dilated by r_max + 1 is
    looked at; d2 is the broadcast sum of the three per-axis squared gaps; nearest is the first minimiser in (z, y, x) order."""
    if not valid(q):
        return INVALID, NOWHERE, 0
    n = grid.shape[0]
    lo, side, r = np.asarray(q[0:3], np.int64), np.asarray(q[3:6], np.int64), int(q[6])
    b0, b1 = lo - (r + 1), lo + side + (r + 1)
    ax = [np.arange(b0[k], b1[k], dtype=np.int64) for k in range(3)]
    g = [_gaps(lo[k], side[k], ax[k]) ** 2 for k in range(3)]
    d2 = g[2][:, None, None] + g[1][None, :, None] + g[0][None, None, :]          # [z][y][x]
    cls = np.full(d2.shape, UNSEEN, np.uint8)
    i0, i1 = np.clip(b0, 0, n), np.clip(b1, 0, n)
    if (i0 < i1).all():
        cls[i0[2] - b0[2]:i1[2] - b0[2], i0[1] - b0[1]:i1[1] - b0[1], i0[0] - b0[0]:i1[0] - b0[0]] = grid[i0[2]:i1[2], i0[1]:i1[1], i0[0]:i1[0]]
    cand = np.where((cls <= stop_at) & (d2 <= r * r), d2, np.int64(1) << 62)
    flat = int(cand.argmin())                    # the first occurrence in C order: z, then y, then x
    best = int(cand.reshape(-1)[flat])
    if best == 1 << 62:
        return NONE, NOWHERE, 0
    z, y, x = np.unravel_index(flat, cand.shape)
    return best, (int(ax[0][x]), int(ax[1][y]), int(ax[2][z])), int((cand == best).sum())


def d2_of(boxes, voxels):
    """d2 between each box (lo xyz, side xyz) and the voxel of the same row, in int64."""
    b, v = np.asarray(boxes, np.int64), np.asarray(voxels, np.int64)
    g = np.maximum(0, np.maximum(v - (b[:, 0:3] + b[:, 3:6]), b[:, 0:3] - (v + 1)))
    return (g * g).sum(1)


def inflated(boxes, k):
    b = np.asarray(boxes, np.int64)
    return np.ascontiguousarray(np.concatenate([b[:, 0:3] - k, b[:, 3:6] + 2 * k], 1).astype(np.int32))


def check_identities(p, boxes, r_max, rng):
    """What the strict box query says about a clearance (boxes valid, r_max [N]).  Returns the
    answers with stop_at occupied and unseen, each (d2, nearest)."""
    from supereight_amd.pipeline import CLEARANCE_NONE
    out = {}
    for stop, code in (("occupied", OCC), ("unseen", UNSEEN)):
        d2, near = p.clearance(boxes, r_max, stop_at=stop)
        alone = p.clearance(boxes, r_max, stop_at=stop, nearest=False)
        assert (alone == d2).all()
        assert (d2 >= CLEARANCE_NONE).all()
        found = d2 >= 0
        assert (d2[found] <= np.asarray(r_max, np.int64)[found] ** 2).all()
        # d2 == 0 <=> the box grown by one voxel holds a blocking voxel
        assert ((d2 == 0) == (p.collides(inflated(boxes, 1)) <= code)).all()
        for k in (2, 5):
            blocked = p.collides(inflated(boxes, k)) <= code
            # (a blocking voxel of the inflated box has a gap of at most k - 1 per axis; it is found where r_max reaches that far)
            reach = 3 * (k - 1) ** 2 <= np.asarray(r_max, np.int64) ** 2
            assert ((d2 >= 0) & (d2 <= 3 * (k - 1) ** 2))[blocked & reach].all()
            assert ((d2 >= k * k) | (d2 == CLEARANCE_NONE))[~blocked].all()
        # the witness blocks, and gives d2 back
        assert (d2_of(boxes[found], near[found]) == d2[found]).all()
        assert (near[~found] == I32_MIN).all()
        assert (p.collides(np.ascontiguousarray(np.concatenate([near[found], np.ones_like(near[found])], 1))) <= code).all()
        # a larger r_max changes no answer that was found
        more = np.minimum(np.asarray(r_max, np.int64) + rng.integers(1, 9, len(boxes)), R_MAX).astype(np.int32)
        d2_more, near_more = p.clearance(boxes, more, stop_at=stop)
        assert (d2_more[found] == d2[found]).all() and (near_more[found] == near[found]).all()
        out[stop] = (d2, near)
    # unseen blocking can only bring the nearest blocking voxel closer
    d_occ, d_uns = out["occupied"][0].astype(np.int64), out["unseen"][0].astype(np.int64)
    big = np.int64(1) << 40
    assert (np.where(d_uns < 0, big, d_uns) <= np.where(d_occ < 0, big, d_occ)).all()
    return out
