"""What the tests of the oriented motion collision queries share (se_hip_collide_oriented_motions / DenseSLAMPipeline.collides_oriented_moving):
the numpy truth from the definition in include/se_hip.h -- the int64 interval form vectorised over the voxels of the sweep's bounding box, held
to the 21-axis form on every cube, and folded over a dense class grid --, the hand-worked cases of tests/cpp/oriented_motion_kats.cpp with the
maps they stand on, and seeded motion generators."""
from fractions import Fraction

import numpy as np

from tests import motion_util
from tests.clearance_util import hand_grid, stamp_clear_map
from tests.motion_util import FREE, INVALID_T
from tests.oriented_util import C_LIMIT, H_LIMIT, I32_MIN, SUB, axes_of, extent, random_boxes
from tests.oriented_util import valid as box_valid

MOVE_LIMIT = 1 << 18
OCC, UNSEEN, EMPTY, INVALID = 0, 1, 2, 255
SEED = 5            # of the motion set that the GPU test runs and the host test takes the census of

# ---------------------------------------------------------------------------------------------------- hand cases
# Maps (64^3, 1024 sub-units; motion_util.HAND_MAPS and clearance_util's `octant`): "a" every block allocated and empty, voxel (10, 10, 10) =
# sub-units [160, 176)^3 occupied; "free" the same without it; "wall" the plane x = 20; "octant" nothing but the level-2 octant [32, 48)^3 =
# sub-units [512, 768)^3, a node without children whose value_ are occupied (everything else unseen).
# case -> (map, centre, (h0, h1, h2), d, (status, t) with stop_at occupied, (status, t) with stop_at unseen); each is derived in the header
# comment of tests/cpp/oriented_motion_kats.cpp.  The diamond _D about x = 32 or 40 spans x in (c_x - 64, c_x + 64) and so starts with a part
# outside the volume: those rows see unseen voxels from t = 0 (status unseen where nothing occupied is touched, t = 0 with stop_at unseen);
# what they say about voxel (10, 10, 10) is the stop_at occupied column.
_A8 = ((8, 0, 0), (0, 8, 0), (0, 0, 8))
_D = ((32, 32, 0), (-32, 32, 0), (0, 0, 4))
_R = ((4, 3, 0), (-3, 4, 0), (0, 0, 5))
_R10 = ((40, 30, 0), (-30, 40, 0), (0, 0, 50))
_SK = ((16, 0, 0), (16, 16, 0), (0, 0, 8))
_BAD = (INVALID, INVALID_T)


def _same(status, t):
    return (status, t), (status, t)


HAND_CASES = {
    "AlignedIntoVoxel": ("a", (128, 168, 168), _A8, (64, 0, 0)) + _same(OCC, Fraction(3, 8)),
    "VertexSlidesOn": ("a", (96, 160, 168), _D, (16, 0, 0)) + _same(OCC, Fraction(0)),
    "VertexSlidesOff": ("a", (96, 160, 168), _D, (0, -16, 0)) + _same(EMPTY, FREE),
    "VertexArrives": ("a", (32, 160, 168), _D, (128, 0, 0), (OCC, Fraction(1, 2)), (OCC, Fraction(0))),
    "FlankArrives": ("a", (32, 152, 168), _D, (128, 0, 0), (OCC, Fraction(9, 16)), (OCC, Fraction(0))),
    "FlankGrazes": ("a", (32, 96, 168), _D, (128, 0, 0), (UNSEEN, FREE), (UNSEEN, Fraction(0))),
    "StopsShort": ("a", (32, 152, 168), _D, (71, 0, 0), (UNSEEN, FREE), (UNSEEN, Fraction(0))),
    "StopsAt": ("a", (32, 152, 168), _D, (72, 0, 0), (UNSEEN, FREE), (UNSEEN, Fraction(0))),
    "StopsPast": ("a", (32, 152, 168), _D, (73, 0, 0), (OCC, Fraction(72, 73)), (OCC, Fraction(0))),
    "DiagonalApproach": ("a", (40, 40, 168), _D, (200, 200, 0)) + ((OCC, Fraction(11, 25)), (OCC, Fraction(0))),
    "SkewMoves": ("a", (230, 160, 168), _SK, (-60, 0, 0)) + _same(OCC, Fraction(19, 30)),
    "Rot345": ("a", (100, 120, 150), _R10, (100, 90, 40)) + _same(OCC, Fraction(11, 67)),
    "Rot345Back": ("a", (300, 290, 200), _R10, (-200, -170, -50)) + _same(OCC, Fraction(294, 655)),
    # leaving the volume: ext = (7, 7, 5) about 168, so the low faces are reached at (168 - ext) / 400 and the high ones at (1024 - 168 - ext) / 900
    "LeaveXlo": ("free", (168, 168, 168), _R, (-400, 0, 0), (UNSEEN, FREE), (UNSEEN, Fraction(161, 400))),
    "LeaveYlo": ("free", (168, 168, 168), _R, (0, -400, 0), (UNSEEN, FREE), (UNSEEN, Fraction(161, 400))),
    "LeaveZlo": ("free", (168, 168, 168), _R, (0, 0, -400), (UNSEEN, FREE), (UNSEEN, Fraction(163, 400))),
    "LeaveXhi": ("free", (168, 168, 168), _R, (900, 0, 0), (UNSEEN, FREE), (UNSEEN, Fraction(849, 900))),
    "LeaveYhi": ("free", (168, 168, 168), _R, (3, 900, 0), (UNSEEN, FREE), (UNSEEN, Fraction(849, 900))),
    "LeaveZhi": ("free", (168, 168, 168), _R, (0, -5, 900), (UNSEEN, FREE), (UNSEEN, Fraction(851, 900))),
    "StaysInside": ("free", (168, 168, 168), _R, (100, 50, -20)) + _same(EMPTY, FREE),
    # absent octants: from the unseen octants of the root into the occupied node [512, 768)^3; the vertex c + h0 - h1 = c + (70, -10, 0) leads
    "OctantEnters": ("octant", (160, 640, 640), _R10, (400, 0, 0), (OCC, Fraction(141, 200)), (OCC, Fraction(0))),
    "OctantStopsBefore": ("octant", (160, 640, 640), _R10, (282, 0, 0), (UNSEEN, FREE), (UNSEEN, Fraction(0))),
    "OctantInside": ("octant", (640, 640, 640), _R10, (10, 10, 10)) + _same(OCC, Fraction(0)),
    # the wall x = 20 = sub-units [320, 336): the vertex c + (64, 0, 0) of the diamond reaches 320 at (320 - 164) / 200
    "IntoWall": ("wall", (100, 500, 500), _D, (200, 30, 7)) + _same(OCC, Fraction(39, 50)),
    "AlongWall": ("wall", (256, 500, 500), _D, (0, 300, 100)) + _same(EMPTY, FREE),
    # valid at the bounds: a voxel-sized box crosses the whole valid range onto voxel (10, 10, 10) -- from 200 - 2^18 its face c_x + 8 reaches
    # 160 at (2^18 - 48) / 2^18, from 100 + 2^18 its face c_x - 8 reaches 176 at (2^18 - 84) / 2^18; both start outside the volume
    "LimitMoveUp": ("a", (200 - MOVE_LIMIT, 168, 168), _A8, (MOVE_LIMIT, 0, 0), (OCC, Fraction(16381, 16384)), (OCC, Fraction(0))),
    "LimitMoveDown": ("a", (100 + MOVE_LIMIT, 168, 168), _A8, (-MOVE_LIMIT, 0, 0), (OCC, Fraction(65515, 65536)), (OCC, Fraction(0))),
    "LimitCentreEnd": ("a", (C_LIMIT - 11, 168, 168), _R, (11, 0, 0), (UNSEEN, FREE), (UNSEEN, Fraction(0))),
    # invalid motions
    "InvalidMove": ("a", (168, 168, 168), _R, (MOVE_LIMIT + 1, 0, 0), _BAD, _BAD),
    "InvalidMoveLow": ("a", (168, 168, 168), _R, (0, 0, -MOVE_LIMIT - 1), _BAD, _BAD),
    "InvalidEnd": ("a", (C_LIMIT - 10, 168, 168), _R, (11, 0, 0), _BAD, _BAD),
    "InvalidEndLow": ("a", (168, -C_LIMIT + 10, 168), _R, (0, -11, 0), _BAD, _BAD),
    "InvalidDet": ("a", (168, 168, 168), ((8, 8, 0), (1, 0, 0), (8, 8, 0)), (16, 0, 0), _BAD, _BAD),
    "InvalidCentre": ("a", (C_LIMIT + 1, 168, 168), _R, (-16, 0, 0), _BAD, _BAD),
    "InvalidAxis": ("a", (168, 168, 168), ((H_LIMIT + 1, 0, 0), (0, 8, 0), (0, 0, 8)), (16, 0, 0), _BAD, _BAD),
    "InvalidInt32MinMove": ("a", (168, 168, 168), _R, (I32_MIN, I32_MIN, I32_MIN), _BAD, _BAD),
    "InvalidInt32MinCentre": ("a", (I32_MIN, 168, 168), _R, (I32_MIN, 0, 0), _BAD, _BAD),
    "InvalidInt32MinAxes": ("a", (168, 168, 168), ((I32_MIN, I32_MIN, I32_MIN), (0, I32_MIN, 0), (0, 0, I32_MIN)), (0, 0, 0), _BAD, _BAD),
}
HAND_MAP_NAMES = ("a", "free", "wall", "octant")
# the cases small enough for the literal definition in the C++ program (the limit cases sweep 16 384 voxels: the numpy truth takes them)
BRUTE_CASES = tuple(k for k in HAND_CASES if not k.startswith("Limit"))


def motion_row(c, h, d):
    return list(c) + [v for hi in h for v in hi] + list(d)


def hand_motion(name):
    c = HAND_CASES[name]
    return motion_row(c[1], c[2], c[3])


def hand_motions(names):
    return np.array([hand_motion(k) for k in names], np.int64).astype(np.int32)


def from_aligned(m9):
    """An axis-aligned motion of collides_moving (lo, side, d in voxels) restated as an oriented one: c = 16 lo + 8 side, h = diag(8 side), 16 d."""
    lo, side, d = (np.asarray(m9[0:3], np.int64), np.asarray(m9[3:6], np.int64), np.asarray(m9[6:9], np.int64))
    return (SUB * lo + (SUB // 2) * side).tolist() + np.diag((SUB // 2) * side).reshape(-1).tolist() + (SUB * d).tolist()


def aligned_hand_cases():
    """The cases of motion_util.HAND_CASES that stay within this query's bounds, restated: name -> (map, fifteen ints, occupied answer, unseen
    answer).  A case that is invalid there stays invalid here (a zero side is a zero half-axis, a coordinate beyond 2^20 voxels is beyond 2^20
    sub-units); one that is valid there but not here is left out."""
    out = {}
    for name, (mp, lo, side, d, occ, uns) in motion_util.HAND_CASES.items():
        m = from_aligned(list(lo) + list(side) + list(d))
        if max(abs(v) for v in m) >= 1 << 31:
            continue
        if occ[0] == INVALID or valid(m):
            assert (occ[0] == INVALID) == (not valid(m)), name
            out[name] = (mp, m, occ, uns)
    return out


stamp_motion_map = stamp_clear_map
motion_hand_grid = hand_grid


def expected_float(fr):
    """What the C ABI returns for the reduced pair: (float)((double)num / (double)den)."""
    return np.float32(np.float64(fr.numerator) / np.float64(fr.denominator))


# ---------------------------------------------------------------------------------------------------- the definition, in numpy
def valid(m):
    m = np.asarray(m, np.int64)
    if not box_valid(m[0:12]):
        return False
    return bool((np.abs(m[12:15]) <= MOVE_LIMIT).all() and (np.abs(m[0:3] + m[12:15]) <= C_LIMIT).all())


def axes21(h, d):
    """The 21 axes of the swept zonotope, int64 [21, 3]: e_k, g_i x g_j, g_i x e_k with g = (h0, h1, h2, d)."""
    e = np.eye(3, dtype=np.int64)
    g = [h[0], h[1], h[2], np.asarray(d, np.int64)]
    rows = [e[0], e[1], e[2]] + [np.cross(g[i], g[j]) for i in range(4) for j in range(i + 1, 4)]
    rows += [np.cross(g[i], e[k]) for i in range(4) for k in range(3)]
    return np.stack(rows).astype(np.int64)


def _affine(a, m):
    return (a[2] * m[2])[:, None, None] + (a[1] * m[1])[None, :, None] + (a[0] * m[0])[None, None, :]


def _int(dtype, v):
    return int(v) if dtype is object else np.int64(v)


def entry_cubes(motion, v0, counts, s=1):
    """Both forms of the predicate on the grid of cubes of side s (voxels) with corners v0 + s * (i, j, k), arrays [z][y][x]: (touched by the
    interval form, the clamped L as numerator and denominator arrays, touched by the 21-axis form).  int64 where every cross product provably
    fits (it does for everything the tests generate), Python integers otherwise."""
    mo = np.asarray(motion, np.int64)
    c, h, d = mo[0:3], mo[3:12].reshape(3, 3), mo[12:15]
    shape = (counts[2], counts[1], counts[0])
    vmax = max(max(abs(int(v0[k])), abs(int(v0[k]) + s * counts[k])) for k in range(3))
    mmax = 32 * vmax + 16 * s + 2 * int(np.abs(c).max()) + int(np.abs(d).max())
    amax = max(int(np.abs(a).sum()) for a in axes21(h, d))
    hmax = int(np.abs(h).sum(0).max())
    num_max = amax * mmax + 2 * amax * hmax * 3 + 16 * s * amax      # |p'| + R, and both sides of the 21-axis form
    den_max = max(2 * amax * int(np.abs(d).max()), 1)
    dt = np.int64 if num_max * den_max < 1 << 62 else object
    v = [np.array([int(v0[k]) + s * i for i in range(counts[k])], dt) for k in range(3)]
    m = [32 * v[k] + _int(dt, 16 * s - 2 * int(c[k])) for k in range(3)]
    ok = np.ones(shape, bool)
    Ln, Ld = np.full(shape, _int(dt, 0), dt), np.full(shape, _int(dt, 1), dt)
    Un, Ud = np.full(shape, _int(dt, 1), dt), np.full(shape, _int(dt, 1), dt)
    for a in axes_of(h):
        if not a.any():
            continue                                   # a zero axis takes no part
        ai = [_int(dt, x) for x in a]
        p = _affine(ai, m)
        q = 2 * int(np.dot(a.astype(object), d.astype(object)))
        R = _int(dt, 2 * int(np.abs(h.astype(object) @ a.astype(object)).sum()) + 16 * s * int(np.abs(a).sum()))
        if q == 0:
            ok &= (np.abs(p) < R).astype(bool)
            continue
        pp, aq = (p if q > 0 else -p), _int(dt, abs(q))
        lower, upper = pp - R, pp + R
        up = (Ln * aq < lower * Ld).astype(bool)
        Ln, Ld = np.where(up, lower, Ln), np.where(up, aq, Ld)
        dn = (upper * Ud < Un * aq).astype(bool)
        Un, Ud = np.where(dn, upper, Un), np.where(dn, aq, Ud)
    touched = ok & (Ln * Ud < Un * Ld).astype(bool)
    m21 = [m[k] - _int(dt, int(d[k])) for k in range(3)]
    swept = np.ones(shape, bool)
    for a in axes21(h, d):
        if not a.any():
            continue
        ao = a.astype(object)
        rhs = _int(dt, 2 * int(np.abs(h.astype(object) @ ao).sum()) + abs(int(np.dot(ao, d.astype(object)))) + 16 * s * int(np.abs(a).sum()))
        swept &= (np.abs(_affine([_int(dt, x) for x in a], m21)) < rhs).astype(bool)
    return touched, Ln, Ld, swept


def sweep_voxels(motion):
    """lo, hi (exclusive) in voxels of the voxels the sweep's bounding interval per axis can touch."""
    mo = np.asarray(motion, np.int64)
    ext = extent(mo[0:12])
    a = mo[0:3] - ext + np.minimum(mo[12:15], 0)
    b = mo[0:3] + ext + np.maximum(mo[12:15], 0)
    return a // SUB, -((-b) // SUB)


def _exact_min(tn, td):
    """The smallest tn / td as a Fraction: a float64 estimate per voxel, exact arithmetic on those within 1e-6 of the smallest only."""
    if tn.size == 0:
        return FREE
    est = tn.astype(np.float64) / td.astype(np.float64)
    near = est <= est.min() + 1e-6
    pairs = {(int(a), int(b)) for a, b in zip(tn[near].tolist(), td[near].tolist())}
    return min(Fraction(a, b) for a, b in pairs)


def oriented_motion_truth(grid, motion, counts=None):
    """The definition over a dense class grid ([z][y][x] uint8 numpy array of the n^3 volume; outside it every voxel is unseen): (status,
    t_exact with stop_at occupied, t_exact with stop_at unseen) of the motion (fifteen ints); t_exact as Fractions.  The 21-axis form is
    asserted equal to the interval form on every cube looked at.  counts: a dict that receives how many cubes were compared."""
    if not valid(motion):
        return INVALID, INVALID_T, INVALID_T
    n = grid.shape[0]
    lo, hi = sweep_voxels(motion)
    touched, Ln, Ld, swept = entry_cubes(motion, lo, tuple(int(hi[k] - lo[k]) for k in range(3)))
    assert (touched == swept).all(), ("the two forms differ", list(motion))
    if counts is not None:
        counts["cubes"] = counts.get("cubes", 0) + touched.size
        counts["touched"] = counts.get("touched", 0) + int(touched.sum())
    cls = np.full(touched.shape, UNSEEN, np.uint8)
    i0, i1 = np.clip(lo, 0, n), np.clip(hi, 0, n)
    if (i0 < i1).all():
        cls[i0[2] - lo[2]:i1[2] - lo[2], i0[1] - lo[1]:i1[1] - lo[1], i0[0] - lo[0]:i1[0] - lo[0]] = grid[i0[2]:i1[2], i0[1]:i1[1], i0[0]:i1[0]]
    tc = cls[touched]
    status = int(tc.min()) if tc.size else EMPTY
    tn, td = Ln[touched], Ld[touched]
    return status, _exact_min(tn[tc <= OCC], td[tc <= OCC]), _exact_min(tn[tc <= UNSEEN], td[tc <= UNSEEN])


def outputs_of(truth, s):
    """The arrays the call returns for a list of truths with stop_at occupied (s = 0) or unseen (s = 1): status, t_first, t_exact."""
    st = np.array([t[0] for t in truth], np.uint8)
    fr = [t[1 + s] for t in truth]
    return st, np.array([expected_float(f) for f in fr], np.float32), np.array([[f.numerator, f.denominator] for f in fr], np.int64).reshape(-1, 2)


# ---------------------------------------------------------------------------------------------------- boxes a motion is compared with
def bounding_motion_boxes(motions):
    """The bounding axis-aligned box of each sweep in whole voxels, as lo xyz, side xyz (what collides() takes)."""
    m = np.asarray(motions, np.int64)
    ext = np.abs(m[:, 3:12].reshape(-1, 3, 3)).sum(1)
    a = m[:, 0:3] - ext + np.minimum(m[:, 12:15], 0)
    b = m[:, 0:3] + ext + np.maximum(m[:, 12:15], 0)
    lo, hi = a // SUB, -((-b) // SUB)
    return np.ascontiguousarray(np.concatenate([lo, hi - lo], 1).astype(np.int32))


def reversed_motions(motions):
    m = np.asarray(motions, np.int64).copy()
    m[:, 0:3] += m[:, 12:15]
    m[:, 12:15] = -m[:, 12:15]
    return np.ascontiguousarray(m.astype(np.int32))


def shuffled_axes(rng, motions):
    """The same motions with their half-axes permuted and negated at random: the same sets."""
    m = np.asarray(motions, np.int64).copy()
    h = m[:, 3:12].reshape(-1, 3, 3)
    perm = np.argsort(rng.random((len(m), 3)), axis=1)
    h = np.take_along_axis(h, perm[:, :, None], axis=1) * rng.choice([-1, 1], (len(m), 3, 1))
    m[:, 3:12] = h.reshape(-1, 9)
    return np.ascontiguousarray(m.astype(np.int32))


def shortened(motions, t_exact):
    """Each blocked motion (0 < t_exact <= 1) moved only as far as t_exact, rounded down to whole sub-units along the segment: with g the gcd
    of |d_k|, the points of the segment on the sub-unit lattice are c + (j / g) d, and the row moves by floor(t_exact g) (d / g).  In the
    shortened motion every blocking voxel's entry parameter is t_in / t' >= 1 (t' = floor(t_exact g) / g <= t_exact <= t_in; for t' = 0 the
    box stands still where no blocking voxel is touched yet), so none is touched: the motion is free for that stop_at.  Returns (the rows'
    indices, the shortened motions)."""
    from math import gcd
    m = np.asarray(motions, np.int64)
    te = np.asarray(t_exact, np.int64)
    idx = np.nonzero((te[:, 0] > 0) & (te[:, 0] <= te[:, 1]))[0]
    out = m[idx].copy()
    for r, i in enumerate(idx):
        d = [int(v) for v in m[i, 12:15]]
        g = gcd(gcd(abs(d[0]), abs(d[1])), abs(d[2]))
        j = int(te[i, 0]) * g // int(te[i, 1])
        out[r, 12:15] = [v // g * j for v in d]
    return idx, np.ascontiguousarray(out.astype(np.int32))


# ---------------------------------------------------------------------------------------------------- generators
def seeded_motions(grid, seed, n=300):
    """n motions for the class grid [z][y][x] of an n^3 volume: half-axis lengths log-uniform from 1 sub-unit to 4 voxels, uniform random
    rotations, a fifth skewed; three fifths of the centres within 10 voxels of an occupied voxel, a quarter in empty voxels, the rest anywhere
    from 6 voxels outside the volume, so that some motions leave it; displacements of up to 16 voxels in a random direction -- of the rows, in
    order, a tenth with d = 0, a tenth with d parallel to a half-axis, a fifth with a zero component."""
    rng = np.random.default_rng(seed)
    size = grid.shape[0]
    occ, emp = np.argwhere(grid == OCC)[:, ::-1], np.argwhere(grid == EMPTY)[:, ::-1]
    assert len(occ) and len(emp)
    k1, k2 = 3 * n // 5, n // 4
    centres = np.concatenate([occ[rng.integers(0, len(occ), k1)] + rng.uniform(-10, 10, (k1, 3)), emp[rng.integers(0, len(emp), k2)] + rng.uniform(0, 1, (k2, 3)),
                              rng.uniform(-6, size + 6, (n - k1 - k2, 3))]) * SUB
    centres = centres[rng.permutation(n)]
    boxes = random_boxes(rng, n, centres, min_len=1, max_len=4 * SUB, skew_share=0.2).astype(np.int64)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    d = np.rint(u * rng.uniform(0, 16 * SUB, (n, 1))).astype(np.int64)
    a, b, c = n // 10, n // 5, 2 * n // 5
    d[:a] = 0
    h = boxes[a:b, 3:12].reshape(-1, 3, 3)
    pick = h[np.arange(b - a), rng.integers(0, 3, b - a)]
    k = rng.choice([-3, -2, -1, 1, 2, 3], (b - a, 1))
    d[a:b] = np.clip(pick * k, -16 * SUB, 16 * SUB)
    far = np.abs(pick * k).max(1) > 16 * SUB                  # (clipping would turn it: take the half-axis itself)
    d[a:b][far] = pick[far]
    d[np.arange(b, c), rng.integers(0, 3, c - b)] = 0
    return np.ascontiguousarray(np.concatenate([boxes, d], 1).astype(np.int32))


def aligned_motions(rng, n, size, max_side=6, max_move=12):
    """n axis-aligned boxes on voxel boundaries moved by whole voxels, some leaving the volume: (oriented motions [n, 15], the same as lo xyz,
    side xyz, d xyz [n, 9] for collides_moving)."""
    lo = rng.integers(-4, size + 2, (n, 3))
    side = rng.integers(1, max_side + 1, (n, 3))
    d = rng.integers(-max_move, max_move + 1, (n, 3))
    d[rng.random((n, 3)) < 0.2] = 0
    m9 = np.concatenate([lo, side, d], 1)
    return (np.ascontiguousarray(np.array([from_aligned(r) for r in m9.tolist()], np.int64).astype(np.int32)), np.ascontiguousarray(m9.astype(np.int32)))


def census(truth):
    """What the seeded set must hold, by the truth alone (a list of (status, t occupied, t unseen)): the counts the tests assert on."""
    k = dict(occupied=0, unseen=0, empty=0, stops_differ=0, zero=0, free=0, between=0)
    for st, to, tu in truth:
        k["occupied"] += st == OCC
        k["unseen"] += st == UNSEEN
        k["empty"] += st == EMPTY
        k["stops_differ"] += to != tu
        k["zero"] += to == 0
        k["free"] += to == FREE
        k["between"] += 0 < to < 1
    return {a: int(b) for a, b in k.items()}
