"""What the tests of the oriented box collision queries share (se_hip_collide_oriented / DenseSLAMPipeline.collides_oriented): the numpy truth
from the definition in include/se_hip.h -- the int64 separating-axis test, vectorised over the voxels of the box's bounding box and folded over
a dense class grid --, the hand-worked cases of tests/cpp/oriented_kats.cpp with the maps they stand on, and seeded box generators."""
import numpy as np

from tests.clearance_util import hand_grid, stamp_clear_map

SUB = 16
C_LIMIT, H_LIMIT = 1 << 20, 1 << 14
OCC, UNSEEN, EMPTY, INVALID = 0, 1, 2, 255
I32_MIN = -(1 << 31)

# ---------------------------------------------------------------------------------------------------- hand cases
# Maps (64^3; motion_util.HAND_MAPS and clearance_util's `octant`): "a" every block allocated and empty, voxel (10, 10, 10) = sub-units
# [160, 176)^3 occupied; "free" the same without it; "octant" nothing but the level-2 octant [32, 48)^3 = sub-units [512, 768)^3, a node
# without children whose value_ are occupied (everything else unseen).
# case -> (map, centre, h0, h1, h2, status, strict status of the bounding axis-aligned box or None), worked by hand:
#   DiamondMissesCorner    |dx| + |dy| < 64 about (112, 112): the bounding box [48, 176)^2 holds voxel (10, 10) in its corner; the voxel's nearest
#                          corner (160, 160) has |dx| + |dy| = 96
#   DiamondVertexOnCorner  the vertex (96 + 64, 160) is the voxel's corner: the diamond stays in x < 160, the open sets do not meet
#   DiamondVertexInside    one sub-unit further: the vertex (161, 160) is inside the voxel's closure and the diamond meets y > 160 there
#   FaceSlides             a 3-4-5 turn about x: the face x = 160 slides along the voxel's face;  FaceSlidesIn: one sub-unit further
#   ThinPlate              a skew plate about 1.4 sub-units thick along the voxel's xy diagonal, through its centre
#   InsideVoxel            a 3-4-5 box of extent 7 about the voxel's centre (168): wholly inside it;  InsideNext: the same in voxel (11, 10, 10)
#   PartlyOutside          extent 14 about x = 8: reaches x < 0;  WhollyOutside: centred at x = -100
#   OctantValue            wholly inside the absent octants of the node [32, 48)^3: value_[child] decides;  OctantUnseen: inside absent octants of the root
#   SkewMisses             the parallelogram c + s0 (16, 0) + s1 (16, 16) about (192, 160): for y in (160, 176) it has x > 176, so voxel (10, 10), in the
#                          top left corner of its bounding box [160, 224) x [144, 176), is missed;  SkewTouches: one sub-unit to the left
#   Invalid*               det = 0; |c_k| = 2^20 + 1; |h_ik| = 2^14 + 1; INT32_MIN components
#   Limit*                 valid at the bounds: a centre at +-2^20 is far outside; half-axes of 2^14 hold the whole volume and leave it
_D = ((32, 32, 0), (-32, 32, 0), (0, 0, 4))
_R = ((4, 3, 0), (-3, 4, 0), (0, 0, 5))
_O = ((40, 30, 0), (-30, 40, 0), (0, 0, 50))
_B = ((H_LIMIT, 0, 0), (0, H_LIMIT, 0), (0, 0, H_LIMIT))
HAND_CASES = {
    "DiamondMissesCorner": ("a", (112, 112, 168)) + _D + (EMPTY, OCC),
    "DiamondVertexOnCorner": ("a", (96, 160, 168)) + _D + (EMPTY, EMPTY),
    "DiamondVertexInside": ("a", (97, 160, 168)) + _D + (OCC, OCC),
    "FaceSlides": ("a", (144, 168, 168), (16, 0, 0), (0, 8, 6), (0, -6, 8), EMPTY, EMPTY),
    "FaceSlidesIn": ("a", (145, 168, 168), (16, 0, 0), (0, 8, 6), (0, -6, 8), OCC, OCC),
    "ThinPlate": ("a", (168, 168, 168), (8, 8, 0), (1, 0, 0), (0, 0, 4), OCC, OCC),
    "InsideVoxel": ("a", (168, 168, 168)) + _R + (OCC, OCC),
    "InsideNext": ("a", (184, 168, 168)) + _R + (EMPTY, EMPTY),
    "PartlyOutside": ("free", (8, 168, 168), (8, 6, 0), (-6, 8, 0), (0, 0, 10), UNSEEN, UNSEEN),
    "WhollyOutside": ("free", (-100, 168, 168), (8, 6, 0), (-6, 8, 0), (0, 0, 10), UNSEEN, UNSEEN),
    "OctantValue": ("octant", (640, 640, 640)) + _O + (OCC, OCC),
    "OctantUnseen": ("octant", (160, 160, 160)) + _O + (UNSEEN, UNSEEN),
    "SkewMisses": ("a", (192, 160, 168), (16, 0, 0), (16, 16, 0), (0, 0, 8), EMPTY, OCC),
    "SkewTouches": ("a", (191, 160, 168), (16, 0, 0), (16, 16, 0), (0, 0, 8), OCC, OCC),
    "InvalidDet": ("a", (168, 168, 168), (8, 8, 0), (1, 0, 0), (8, 8, 0), INVALID, None),
    "InvalidDetZeroAxis": ("a", (168, 168, 168), (8, 8, 0), (0, 0, 0), (0, 0, 4), INVALID, None),
    "InvalidCentre": ("a", (C_LIMIT + 1, 168, 168)) + _R + (INVALID, None),
    "InvalidCentreLow": ("a", (168, -C_LIMIT - 1, 168)) + _R + (INVALID, None),
    "InvalidAxis": ("a", (168, 168, 168), (H_LIMIT + 1, 0, 0), (0, 8, 0), (0, 0, 8), INVALID, None),
    "InvalidAxisLow": ("a", (168, 168, 168), (8, 0, 0), (0, 8, 0), (0, 0, -H_LIMIT - 1), INVALID, None),
    "InvalidInt32MinCentre": ("a", (I32_MIN, 168, 168)) + _R + (INVALID, None),
    "InvalidInt32MinAxis": ("a", (168, 168, 168), (I32_MIN, I32_MIN, I32_MIN), (0, I32_MIN, 0), (0, 0, I32_MIN), INVALID, None),
    "LimitCentreHigh": ("a", (C_LIMIT, C_LIMIT, C_LIMIT)) + _R + (UNSEEN, None),
    "LimitCentreLow": ("a", (-C_LIMIT, 168, 168)) + _R + (UNSEEN, None),
    "LimitAxesFree": ("free", (512, 512, 512)) + _B + (UNSEEN, None),
    "LimitAxesOccupied": ("a", (512, 512, 512), (0, H_LIMIT, 0), (-H_LIMIT, 0, 0), (0, 0, -H_LIMIT), OCC, None),
}
HAND_MAP_NAMES = ("a", "free", "octant")
# the cases small enough for the literal definition (the limit cases have bounding boxes of up to 2048^3 voxels)
BRUTE_CASES = tuple(k for k in HAND_CASES if not k.startswith("Limit"))


def hand_box(name):
    c = HAND_CASES[name]
    return list(c[1]) + list(c[2]) + list(c[3]) + list(c[4])


def hand_boxes(names):
    return np.array([hand_box(k) for k in names], np.int64).astype(np.int32)


stamp_oriented_map = stamp_clear_map
oriented_hand_grid = hand_grid


# ---------------------------------------------------------------------------------------------------- the definition, in numpy
def valid(box):
    b = np.asarray(box, np.int64)
    c, h = b[0:3], b[3:12].reshape(3, 3)
    if (np.abs(c) > C_LIMIT).any() or (np.abs(h) > H_LIMIT).any():
        return False
    return int(np.dot(h[0], np.cross(h[1], h[2]))) != 0


def axes_of(h):
    """The 15 axes of the definition, int64 [15, 3]: e_x e_y e_z, h1 x h2, h2 x h0, h0 x h1, then h_i x e_k."""
    e = np.eye(3, dtype=np.int64)
    rows = [e[0], e[1], e[2], np.cross(h[1], h[2]), np.cross(h[2], h[0]), np.cross(h[0], h[1])]
    rows += [np.cross(h[i], e[k]) for i in range(3) for k in range(3)]
    return np.stack(rows).astype(np.int64)


def extent(box):
    """sum_i |h_ik| per axis k: the box spans the open interval (c_k - ext_k, c_k + ext_k)."""
    return np.abs(np.asarray(box, np.int64)[3:12].reshape(3, 3)).sum(0)


def touched_cubes(box, v0, counts, s=1):
    """The predicate on the grid of cubes of side s (voxels) with corners v0 + s * (i, j, k), i < counts[0] ...: a bool array [z][y][x].
    Per axis the left side a . m, m = 32 v + 16 s - 2 c, is the broadcast sum of three 1-D terms."""
    b = np.asarray(box, np.int64)
    c, h = b[0:3], b[3:12].reshape(3, 3)
    v = [np.int64(v0[k]) + np.int64(s) * np.arange(counts[k], dtype=np.int64) for k in range(3)]
    m = [32 * v[k] + 16 * s - 2 * c[k] for k in range(3)]
    ok = np.ones((counts[2], counts[1], counts[0]), bool)
    for a in axes_of(h):
        if not a.any():
            continue                                   # a zero axis separates nothing
        rhs = 2 * np.abs(h @ a).sum() + 16 * s * np.abs(a).sum()
        am = (a[2] * m[2])[:, None, None] + (a[1] * m[1])[None, :, None] + (a[0] * m[0])[None, None, :]
        ok &= np.abs(am) < rhs
    return ok


def touched(box, v, s):
    """The predicate for one cube (corner v, side s)."""
    return bool(touched_cubes(box, v, (1, 1, 1), s)[0, 0, 0])


def bounding_voxels(box):
    """lo, hi (exclusive) in voxels of the voxels the box's bounding interval per axis can touch."""
    b = np.asarray(box, np.int64)
    ext = extent(b)
    lo = (b[0:3] - ext) // SUB
    hi = -((-(b[0:3] + ext)) // SUB)
    return lo, hi


def oriented_truth(grid, box):
    """The definition over a dense class grid ([z][y][x] uint8 numpy array of the n^3 volume; outside it every voxel is unseen): the status of
    `box` (twelve ints)."""
    if not valid(box):
        return INVALID
    n = grid.shape[0]
    lo, hi = bounding_voxels(box)
    t = touched_cubes(box, lo, tuple(int(hi[k] - lo[k]) for k in range(3)))
    cls = np.full(t.shape, UNSEEN, np.uint8)
    i0, i1 = np.clip(lo, 0, n), np.clip(hi, 0, n)
    if (i0 < i1).all():
        cls[i0[2] - lo[2]:i1[2] - lo[2], i0[1] - lo[1]:i1[1] - lo[1], i0[0] - lo[0]:i1[0] - lo[0]] = grid[i0[2]:i1[2], i0[1]:i1[1], i0[0]:i1[0]]
    tc = cls[t]
    return int(tc.min()) if tc.size else EMPTY


def bounding_boxes(boxes):
    """The bounding axis-aligned box of each oriented box in whole voxels, as lo xyz, side xyz (what collides() takes)."""
    b = np.asarray(boxes, np.int64)
    ext = np.abs(b[:, 3:12].reshape(-1, 3, 3)).sum(1)
    lo = (b[:, 0:3] - ext) // SUB
    hi = -((-(b[:, 0:3] + ext)) // SUB)
    return np.ascontiguousarray(np.concatenate([lo, hi - lo], 1).astype(np.int32))


# ---------------------------------------------------------------------------------------------------- generators
def random_rotations(rng, n):
    """n rotation matrices, uniform over SO(3) (unit quaternions from normal deviates)."""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], 1)


def make_boxes(centres_sub, rotations, half_lengths_sub, skew=None):
    """int32 [N, 12] from centres (sub-units), rotations [N, 3, 3] (column i = direction of axis i) and half lengths (sub-units), rounded to
    the nearest sub-unit; skew [N] bool: h1 += h0 / 2 before rounding (a box that is not a rectangle).  A box whose rounded axes are
    dependent gets h_i += e_i (tiny boxes only)."""
    c = np.rint(np.asarray(centres_sub, np.float64))
    h = np.asarray(rotations, np.float64).transpose(0, 2, 1) * np.asarray(half_lengths_sub, np.float64)[:, :, None]     # [N, i, k]
    if skew is not None:
        h[:, 1] += np.where(np.asarray(skew)[:, None], 0.5 * h[:, 0], 0.0)
    h = np.rint(h).astype(np.int64)
    det = np.einsum("nk,nk->n", h[:, 0], np.cross(h[:, 1], h[:, 2]))
    h[det == 0] += np.eye(3, dtype=np.int64)
    det = np.einsum("nk,nk->n", h[:, 0], np.cross(h[:, 1], h[:, 2]))
    h[det == 0] = 2 * np.eye(3, dtype=np.int64)
    return np.ascontiguousarray(np.concatenate([c.astype(np.int64), h.reshape(-1, 9)], 1).astype(np.int32))


def random_boxes(rng, n, centres_sub, min_len=1, max_len=8 * SUB, skew_share=0.2):
    """n boxes at the given centres: half-axis lengths log-uniform in [min_len, max_len] sub-units (1 / 16 voxel to 8 voxels), uniform
    random rotations, a share of them skewed."""
    lengths = np.exp(rng.uniform(np.log(min_len), np.log(max_len), (n, 3)))
    return make_boxes(centres_sub, random_rotations(rng, n), lengths, rng.random(n) < skew_share)


def aligned_boxes(rng, n, size, max_side=12):
    """n axis-aligned boxes on voxel boundaries, some reaching outside the volume: (oriented [n, 12], the same box as lo xyz side xyz [n, 6]).
    Odd sides put the centre on a half voxel: everything is a whole number of sub-units."""
    lo = rng.integers(-6, size + 2, (n, 3))
    side = rng.integers(1, max_side + 1, (n, 3))
    o = np.zeros((n, 12), np.int64)
    o[:, 0:3] = SUB * lo + (SUB // 2) * side
    for i in range(3):
        o[:, 3 + 4 * i] = (SUB // 2) * side[:, i]
    return np.ascontiguousarray(o.astype(np.int32)), np.ascontiguousarray(np.concatenate([lo, side], 1).astype(np.int32))


def shuffled_axes(rng, boxes):
    """The same boxes with their half-axes permuted and negated at random: the same sets."""
    b = np.asarray(boxes, np.int64).copy()
    h = b[:, 3:12].reshape(-1, 3, 3)
    perm = np.argsort(rng.random((len(b), 3)), axis=1)
    h = np.take_along_axis(h, perm[:, :, None], axis=1) * rng.choice([-1, 1], (len(b), 3, 1))
    b[:, 3:12] = h.reshape(-1, 9)
    return np.ascontiguousarray(b.astype(np.int32))


def check_identities(p, rng, oriented, aligned, aligned_lo_side):
    """What the strict box query says about oriented boxes: an axis-aligned box on voxel boundaries is that box; permuting or negating the
    half-axes changes nothing; collides(bounding box) <= collides_oriented(box) in status code.  Returns (status of `oriented`, of `aligned`,
    the strict status of the bounding boxes of `oriented`)."""
    st = p.collides_oriented(oriented)
    sa = p.collides_oriented(aligned)
    assert (sa == p.collides(aligned_lo_side)).all()
    assert (p.collides_oriented(shuffled_axes(rng, oriented)) == st).all()
    assert (p.collides_oriented(shuffled_axes(rng, aligned)) == sa).all()
    bound = p.collides(bounding_boxes(oriented))
    assert (bound <= st).all()
    assert (p.collides(bounding_boxes(aligned)) == sa).all()
    return st, sa, bound
