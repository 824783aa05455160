"""What the tests of the segment traces share (se_hip_trace_segments / DenseSLAMPipeline.trace): the hand-worked cases of
tests/cpp/trace_kats.cpp with their answers, the truth of a segment over a dense class grid -- the three-axis integer DDA (trace_truth) and
the literal enumeration of the definition (trace_literal_truth), both in Python integers --, the class grid of a map given as blocks and
nodes, and the seeded segment families of the GPU test."""
from fractions import Fraction

import numpy as np

from tests.host_util import decode
from tests.motion_util import EMPTY, FREE, INVALID, INVALID_T, OCC, UNSEEN, as_float32  # noqa: F401  (re-exported)

SUB = 16
LIMIT = 1 << 22
SEED = 11           # of the segment set that the GPU test traces and the host test takes the census of
NONE = (-(1 << 31),) * 3

_L = LIMIT
# case -> (map of motion_util.HAND_MAPS, a, b, answer with stop_at occupied, answer with stop_at unseen); an answer is
# (status, t_first, first, (unseen count, empty count)), worked by hand:
#   DiagonalCorners      through the corners (16 i,) * 3: exactly the voxels (i, i, i), i = 0 .. 19
#   DiagonalCornersHit   the same on map "a": (10, 10, 10) is entered at 160 / 320 after ten empty voxels
#   Diagonal3            the motion case for the box's centre: from (8, 8, 8), (10, 10, 10) is entered at (160 - 8) / 320
#   DiagonalTouches      y = x + 16 in the slice z = 0: the voxels (i, i + 1, 0); (10, 11, 0) is entered at 160 / 320
#   DiagonalOpenEnd      the same segment on map "c": (10, 12, 0) shares only the edge x = 176, y = 192 with it -- not touched
#   SlideInWallFace      a_x = b_x = 320, the face plane of the wall x = 20: touches nothing
#   IntoWall             x reaches 320 at (320 - 168) / 320 = 19 / 40, where y = 88 + 76 = 164: voxel (20, 10, 5); before it ten x cells and
#                        five y crossings (at 8 + 16 j over 320 against 16 + 32 k over 320: never together): 15 empty voxels
#   UnseenGap            along x at y = z = 56: the unseen block x = 24 .. 31 is entered at (384 - 168) / 640 after 14 empty voxels, the
#                        obstacle (40, 3, 3) at (640 - 168) / 640 after 8 unseen and 14 + 8 empty ones
#   Leave*               from the centre of voxel 30 (488) over 640 sub-units: 31 voxels down to 0, leaving at 488 / 640; 34 voxels up to 63,
#                        leaving at (1024 - 488) / 640
#   StartOutside*        from x = -152 (voxel -10): blocked at once under stop_at unseen, else the volume is entered at 152 / 640
#   WhollyOutside        every voxel is unseen, none is counted
#   ZeroLength*          a point inside a voxel touches it, a point on a corner touches nothing
#   LimitLow / High      x from -2^22 to 2^22 (and back) through (10, 5, 5): entered at (160 + 2^22) / 2^23 after voxels 0 .. 9, and at
#                        (2^22 - 176) / 2^23 after voxels 63 .. 11
#   BeyondLimit          one sub-unit beyond the limit
HAND_CASES = {
    "DiagonalCorners": ("free", (0, 0, 0), (320, 320, 320), (EMPTY, FREE, NONE, (0, 20)), (EMPTY, FREE, NONE, (0, 20))),
    "DiagonalCornersHit": ("a", (0, 0, 0), (320, 320, 320), (OCC, Fraction(1, 2), (10, 10, 10), (0, 10)), (OCC, Fraction(1, 2), (10, 10, 10), (0, 10))),
    "Diagonal3": ("a", (8, 8, 8), (328, 328, 328), (OCC, Fraction(19, 40), (10, 10, 10), (0, 10)), (OCC, Fraction(19, 40), (10, 10, 10), (0, 10))),
    "DiagonalTouches": ("b", (0, 16, 8), (320, 336, 8), (OCC, Fraction(1, 2), (10, 11, 0), (0, 10)), (OCC, Fraction(1, 2), (10, 11, 0), (0, 10))),
    "DiagonalOpenEnd": ("c", (0, 16, 8), (320, 336, 8), (EMPTY, FREE, NONE, (0, 20)), (EMPTY, FREE, NONE, (0, 20))),
    "SlideInWallFace": ("wall", (320, 40, 40), (320, 500, 300), (EMPTY, FREE, NONE, (0, 0)), (EMPTY, FREE, NONE, (0, 0))),
    "IntoWall": ("wall", (168, 88, 88), (488, 248, 88), (OCC, Fraction(19, 40), (20, 10, 5), (0, 15)), (OCC, Fraction(19, 40), (20, 10, 5), (0, 15))),
    "UnseenGap": ("gap", (168, 56, 56), (808, 56, 56), (OCC, Fraction(59, 80), (40, 3, 3), (8, 22)), (UNSEEN, Fraction(27, 80), (24, 3, 3), (0, 14))),
    "LeaveXlo": ("free", (488, 488, 488), (-152, 488, 488), (UNSEEN, FREE, NONE, (0, 31)), (UNSEEN, Fraction(61, 80), (-1, 30, 30), (0, 31))),
    "LeaveXhi": ("free", (488, 488, 488), (1128, 488, 488), (UNSEEN, FREE, NONE, (0, 34)), (UNSEEN, Fraction(67, 80), (64, 30, 30), (0, 34))),
    "LeaveYlo": ("free", (488, 488, 488), (488, -152, 488), (UNSEEN, FREE, NONE, (0, 31)), (UNSEEN, Fraction(61, 80), (30, -1, 30), (0, 31))),
    "LeaveYhi": ("free", (488, 488, 488), (488, 1128, 488), (UNSEEN, FREE, NONE, (0, 34)), (UNSEEN, Fraction(67, 80), (30, 64, 30), (0, 34))),
    "LeaveZlo": ("free", (488, 488, 488), (488, 488, -152), (UNSEEN, FREE, NONE, (0, 31)), (UNSEEN, Fraction(61, 80), (30, 30, -1), (0, 31))),
    "LeaveZhi": ("free", (488, 488, 488), (488, 488, 1128), (UNSEEN, FREE, NONE, (0, 34)), (UNSEEN, Fraction(67, 80), (30, 30, 64), (0, 34))),
    "StartOutside": ("free", (-152, 488, 488), (488, 488, 488), (UNSEEN, FREE, NONE, (0, 31)), (UNSEEN, Fraction(0), (-10, 30, 30), (0, 0))),
    "StartOutsideHit": ("d", (-152, 88, 88), (488, 88, 88), (OCC, Fraction(39, 80), (10, 5, 5), (0, 10)), (UNSEEN, Fraction(0), (-10, 5, 5), (0, 0))),
    "WhollyOutside": ("free", (-168, -168, -168), (-24, -40, -8), (UNSEEN, FREE, NONE, (0, 0)), (UNSEEN, Fraction(0), (-11, -11, -11), (0, 0))),
    "ZeroLengthInside": ("a", (168, 168, 168), (168, 168, 168), (OCC, Fraction(0), (10, 10, 10), (0, 0)), (OCC, Fraction(0), (10, 10, 10), (0, 0))),
    "ZeroLengthFree": ("free", (168, 168, 168), (168, 168, 168), (EMPTY, FREE, NONE, (0, 1)), (EMPTY, FREE, NONE, (0, 1))),
    "ZeroLengthCorner": ("a", (160, 160, 160), (160, 160, 160), (EMPTY, FREE, NONE, (0, 0)), (EMPTY, FREE, NONE, (0, 0))),
    "LimitLow": ("d", (-_L, 88, 88), (_L, 88, 88), (OCC, Fraction(160 + _L, 2 * _L), (10, 5, 5), (0, 10)), (UNSEEN, Fraction(0), (-(_L // 16), 5, 5), (0, 0))),
    "LimitHigh": ("d", (_L, 88, 88), (-_L, 88, 88), (OCC, Fraction(_L - 176, 2 * _L), (10, 5, 5), (0, 53)), (UNSEEN, Fraction(0), (_L // 16 - 1, 5, 5), (0, 0))),
    "BeyondLimit": ("d", (_L + 1, 88, 88), (0, 88, 88), (INVALID, INVALID_T, NONE, (-1, -1)), (INVALID, INVALID_T, NONE, (-1, -1))),
}


def hand_grids():
    """The class grids [z][y][x] of motion_util.HAND_MAPS."""
    from tests.motion_util import HAND_MAPS
    grids = {}
    for name, spec in HAND_MAPS.items():
        g = np.full((64, 64, 64), EMPTY, np.uint8)
        for x, y, z in spec.get("occupied", []):
            g[z, y, x] = OCC
        if "wall" in spec:
            g[:, :, spec["wall"]] = OCC
        if "gap" in spec:
            x0, y0, z0, x1, y1, z1 = spec["gap"]
            g[z0:z1, y0:y1, x0:x1] = UNSEEN
        grids[name] = g
    return grids


def expected_float(fr):
    """The float the C ABI returns for a t_first of the tables and truths here."""
    return np.float32(2.0) if fr == FREE else (np.float32(-1.0) if fr == INVALID_T else as_float32(fr))


def valid(seg):
    return all(abs(int(c)) <= LIMIT for c in seg)


def degenerate(seg):
    """The segment lies in a grid plane: it touches nothing."""
    return any(int(seg[k]) == int(seg[3 + k]) and int(seg[k]) % SUB == 0 for k in range(3))


def _interval(a, d, c, s):
    """The cube test of the definition for the cube [c, c + s)^3 (voxels; c per axis): (L, U) as Fractions, L from 0 and U from 1, or None
    where an axis that does not move misses the cube.  The cube is touched iff L < U."""
    L, U = Fraction(0), Fraction(1)
    for k in range(3):
        lo, hi = SUB * c[k], SUB * (c[k] + s)
        if d[k] == 0:
            if not lo < a[k] < hi:
                return None
            continue
        lower = Fraction(lo - a[k], d[k]) if d[k] > 0 else Fraction(a[k] - hi, -d[k])
        upper = Fraction(hi - a[k], d[k]) if d[k] > 0 else Fraction(a[k] - lo, -d[k])
        L, U = max(L, lower), min(U, upper)
    return L, U


def _land(a, d, t):
    """The voxel that holds P(t + eps): per axis the floor of the exact position; on a grid plane the voxel above for d > 0, below for d < 0."""
    v = []
    for k in range(3):
        p = a[k] * t.denominator + t.numerator * d[k]
        q, r = divmod(p, SUB * t.denominator)
        v.append(q - 1 if (r == 0 and d[k] < 0) else q)
    return v


def _fold(visit, grid, stop_at):
    """The outputs from the touched voxels in traversal order (`visit` yields (t_in, voxel)): (status, t_first, first, (unseen, empty))."""
    n = grid.shape[0]
    status, counts = EMPTY, [0, 0]
    for t, v in visit:
        inside = all(0 <= c < n for c in v)
        cls = int(grid[v[2], v[1], v[0]]) if inside else UNSEEN
        status = min(status, cls)
        if cls <= stop_at:
            return status, t, tuple(v), tuple(counts)
        if inside:
            counts[cls - 1] += 1
    return status, FREE, NONE, tuple(counts)


def trace_truth(grid, seg, stop_at, info=None, octant_side=None):
    """The three-axis integer DDA over a dense class grid ([z][y][x] uint8 of the n^3 volume; outside it every voxel is unseen):
    (status, t_first as a Fraction, first, (unseen count, empty count)) of the segment a xyz, b xyz in sub-units.  The stretch before the
    volume is jumped, nothing is visited after the volume has been left.  info (a dict) receives what the walk met: 'ties2' / 'ties3' steps
    with two / three planes crossed at once, 'entered' (started outside and landed inside), 'absent' the largest side of an absent octant
    walked through (octant_side: [z][y][x] per block, 0 where the block is present)."""
    seg = [int(c) for c in seg]
    if not valid(seg):
        return INVALID, INVALID_T, NONE, (-1, -1)
    if degenerate(seg):
        return EMPTY, FREE, NONE, (0, 0)
    n = grid.shape[0]
    a, d = seg[0:3], [seg[3 + k] - seg[k] for k in range(3)]
    met = dict(ties2=0, ties3=0, entered=False, absent=0)

    def visit():
        t = Fraction(0)
        v = _land(a, d, t)
        entered = False
        while True:
            inside = all(0 <= c < n for c in v)
            yield t, v
            if not inside:
                if entered:
                    return
                lu = _interval(a, d, (0, 0, 0), n)
                if lu is None or not lu[0] < lu[1]:
                    return
                t = lu[0]
                v = _land(a, d, t)
                entered = met["entered"] = True
                continue
            entered = True
            if octant_side is not None:
                met["absent"] = max(met["absent"], int(octant_side[v[2] >> 3, v[1] >> 3, v[0] >> 3]))
            nxt = [Fraction(SUB * (v[k] + 1) - a[k], d[k]) if d[k] > 0 else (Fraction(a[k] - SUB * v[k], -d[k]) if d[k] < 0 else None) for k in range(3)]
            moving = [x for x in nxt if x is not None]
            if not moving or min(moving) >= 1:
                return
            t = min(moving)
            tied = [k for k in range(3) if nxt[k] == t]
            if len(tied) > 1:
                met["ties%d" % len(tied)] += 1
            v = [v[k] + ((1 if d[k] > 0 else -1) if k in tied else 0) for k in range(3)]

    out = _fold(visit(), grid, stop_at)
    if info is not None:
        info.update(met)
    return out


def trace_literal_truth(grid, seg, stop_at):
    """The definition, literally: every voxel of the segment's bounding box tested by the cube test, the touched ones sorted by their entry
    parameter (pairwise distinct: asserted) and folded.  For short segments."""
    seg = [int(c) for c in seg]
    if not valid(seg):
        return INVALID, INVALID_T, NONE, (-1, -1)
    a, d = seg[0:3], [seg[3 + k] - seg[k] for k in range(3)]
    lo = [min(seg[k], seg[3 + k]) // SUB for k in range(3)]
    hi = [max(seg[k], seg[3 + k]) // SUB for k in range(3)]
    touched = []
    for z in range(lo[2], hi[2] + 1):
        for y in range(lo[1], hi[1] + 1):
            for x in range(lo[0], hi[0] + 1):
                lu = _interval(a, d, (x, y, z), 1)
                if lu is not None and lu[0] < lu[1]:
                    touched.append((lu[0], (x, y, z)))
    touched.sort()
    assert all(p[0] < q[0] for p, q in zip(touched, touched[1:])), "two touched voxels with one entry parameter"
    return _fold(touched, grid, stop_at)


# ------------------------------------------------------------------ the class grid of a map given as blocks and nodes
def class_of(x, y, init, thr, above):
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    occ = (x > np.float32(thr)) if above else (x < np.float32(thr))
    return np.where((x == np.float32(init[0])) & (y == np.float32(init[1])), UNSEEN, np.where(occ, OCC, EMPTY)).astype(np.uint8)


def grids_from_octree(size, blocks, nodes, init, thr, above):
    """classify(Octree::get(v)) at every voxel ([z][y][x] uint8) of a map given as blocks() = (coords, x, y, ...) and nodes() = (code, side,
    x, y), and per block [z][y][x] the side in voxels of the absent octant that holds it (0: the block is present)."""
    grid = np.empty((size, size, size), np.uint8)
    nb = size // 8
    side_of = np.zeros((nb, nb, nb), np.int32)
    code, _, nx, ny = nodes
    order = sorted(range(len(code)), key=lambda i: decode(code[i])[3])          # by level: deeper nodes overwrite
    if not order:
        grid[:] = class_of(init[0], init[1], init, thr, above)
        side_of[:] = size
    for i in order:
        x0, y0, z0, level = decode(code[i])
        h = (size >> level) // 2
        cls = class_of(nx[i], ny[i], init, thr, above)
        for c in range(8):
            cx, cy, cz = x0 + (c & 1) * h, y0 + ((c >> 1) & 1) * h, z0 + (c >> 2) * h
            grid[cz:cz + h, cy:cy + h, cx:cx + h] = cls[c]
            side_of[cz // 8:(cz + h + 7) // 8, cy // 8:(cy + h + 7) // 8, cx // 8:(cx + h + 7) // 8] = h
    coords, bx, by = blocks[0], blocks[1], blocks[2]
    for i in range(len(coords)):
        x0, y0, z0 = (int(v) for v in coords[i])
        grid[z0:z0 + 8, y0:y0 + 8, x0:x0 + 8] = class_of(bx[i], by[i], init, thr, above).reshape(8, 8, 8)
        side_of[z0 // 8, y0 // 8, x0 // 8] = 0
    return grid, side_of


# ------------------------------------------------------------------ the seeded segment families
def seeded_segments(grid, seed):
    """About 2 000 segments for an n^3 class grid, by family: arbitrary endpoints; through occupied voxels; corner to corner along a space or
    face diagonal (three / two planes at once); arbitrary corners; half-voxel endpoints; axis-parallel ones, a quarter of them in a grid
    plane; from outside into the volume; long ones across the whole volume; points; invalid ones."""
    rng = np.random.default_rng(seed)
    n = grid.shape[0]
    S = SUB * n
    sets = []
    sets.append(rng.integers(-S // 6, S + S // 6, (500, 6)))
    occ = np.argwhere(grid == OCC)[:, ::-1]                                      # x y z
    assert len(occ) > 0
    target = occ[rng.integers(0, len(occ), 300)] * SUB + rng.integers(1, SUB, (300, 3))
    off = rng.integers(-30 * SUB, 30 * SUB + 1, (300, 3))
    sets.append(np.concatenate([target + off, target - (off * rng.integers(1, 5, (300, 1))) // 4], 1))
    # corners: along (+-1, +-1, +-1), and along (+-1, +-1) in a slice that is no grid plane
    a = rng.integers(-4, n + 5, (300, 3)) * SUB
    s = rng.choice([-1, 1], (300, 3))
    k = rng.integers(1, 41, (300, 1)) * SUB
    b = a + s * k
    flat = rng.integers(0, 3, 150)
    a[np.arange(150), flat] += rng.integers(1, SUB, 150)
    b[np.arange(150), flat] = a[np.arange(150), flat] + rng.integers(-40, 41, 150) * (rng.random(150) < 0.5)
    sets.append(np.concatenate([a, b], 1))
    sets.append(rng.integers(-4, n + 5, (100, 6)) * SUB)
    c = rng.integers(0, n, (150, 6)) * SUB + SUB // 2
    c[:50, 3:6] = c[:50, 0:3] + rng.choice([-1, 1], (50, 3)) * rng.integers(1, 30, (50, 1)) * SUB   # centre to centre along a diagonal
    sets.append(c)
    a = rng.integers(-2 * SUB, S + 2 * SUB, (200, 3))
    a[:50, 0] = rng.integers(0, n, 50) * SUB                                     # x on a grid plane
    b = a.copy()
    ax = rng.integers(0, 3, 200)
    ax[:50] = rng.integers(1, 3, 50)                                             # ... and x does not move: degenerate
    b[np.arange(200), ax] = rng.integers(-2 * SUB, S + 2 * SUB, 200)
    sets.append(np.concatenate([a, b], 1))
    a = rng.integers(0, S, (100, 3))
    a[np.arange(100), rng.integers(0, 3, 100)] = np.where(rng.random(100) < 0.5, rng.integers(-300, 0, 100), rng.integers(S + 1, S + 301, 100))
    sets.append(np.concatenate([a, rng.integers(0, S, (100, 3))], 1))
    a = rng.integers(-2000, S + 2000, (100, 3))
    sets.append(np.concatenate([a, S - a + rng.integers(-200, 201, (100, 3))], 1))
    e = S - 8
    sets.append(np.array([[8, 8, 8, e, e, e], [e, 8, 8, 8, e, e], [8, e, 8, e, 8, e], [e, e, 8, 8, 8, e], [0, 0, 0, S, S, S], [S, S, S, 0, 0, 0]]))
    p = rng.integers(0, S, (20, 3))
    p[:6] = p[:6] // SUB * SUB
    sets.append(np.concatenate([p, p], 1))
    bad = rng.integers(-S, 2 * S, (24, 6))
    bad[np.arange(24), rng.integers(0, 6, 24)] = rng.choice([LIMIT + 1, -LIMIT - 1, 2 ** 31 - 1, -2 ** 31, 1 << 25, -(1 << 27)], 24)
    sets.append(bad)
    lim = np.array([[-LIMIT, 700, 900, LIMIT, 900, 700], [LIMIT, LIMIT, LIMIT, -LIMIT, -LIMIT, -LIMIT], [1000, -LIMIT, 1000, 1001, LIMIT, 999],
                    [LIMIT, 5, 5, LIMIT, 700, 5]])
    sets.append(lim)
    return np.ascontiguousarray(np.concatenate(sets).astype(np.int32))


KINDS = ("occupied", "unseen_inside", "blocked_outside", "free", "ties2", "ties3", "degenerate", "entered", "absent32", "invalid",
         "unseen_count", "empty_count")


def census(grid, segments, octant_side=None):
    """(the truth per segment for stop_at occupied and unseen, how many segments are of each of KINDS)."""
    n = grid.shape[0]
    kinds = dict.fromkeys(KINDS, 0)
    truth = ([], [])
    for seg in segments.tolist():
        info = {}
        o = trace_truth(grid, seg, OCC, info, octant_side)
        u = trace_truth(grid, seg, UNSEEN)
        truth[0].append(o)
        truth[1].append(u)
        if o[0] == INVALID:
            kinds["invalid"] += 1
            continue
        if degenerate(seg):
            kinds["degenerate"] += 1
            continue
        kinds["occupied"] += o[1] != FREE
        kinds["free"] += o[1] == FREE
        if u[1] != FREE:
            inside = all(0 <= c < n for c in u[2])
            kinds["unseen_inside"] += inside and int(grid[u[2][2], u[2][1], u[2][0]]) == UNSEEN
            kinds["blocked_outside"] += not inside
        kinds["ties2"] += info["ties2"] > 0
        kinds["ties3"] += info["ties3"] > 0
        kinds["entered"] += bool(info["entered"])
        kinds["absent32"] += info["absent"] >= 32
        kinds["unseen_count"] += o[3][0] > 0
        kinds["empty_count"] += o[3][1] > 0
    return truth, kinds


def outputs_of(truth):
    """The arrays the entry returns for a list of truths: status uint8, t_first float32, first int32 [n, 3], counts int32 [n, 2]."""
    return (np.array([r[0] for r in truth], np.uint8), np.array([expected_float(r[1]) for r in truth], np.float32),
            np.array([r[2] for r in truth], np.int64).astype(np.int32).reshape(-1, 3), np.array([r[3] for r in truth], np.int32).reshape(-1, 2))
