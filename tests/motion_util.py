"""What the tests of the motion collision queries share (se_hip_collide_motions / DenseSLAMPipeline.collides_moving): the hand-worked cases
of tests/cpp/motion_kats.cpp with their answers, the numpy truth of a motion over a dense class grid (the definition, in int64), the class
grid itself, and the boxes a motion is compared with."""
from fractions import Fraction

import numpy as np

LIMIT = 1 << 20
FREE = Fraction(2)
INVALID_T = Fraction(-1)
OCC, UNSEEN, EMPTY, INVALID = 0, 1, 2, 255

# the 64^3 maps of the hand cases: every block allocated and empty, then `occupied` voxels, the `wall` plane x = 20, and the `gap` box unseen
HAND_MAPS = {
    "a": dict(occupied=[(10, 10, 10)]),
    "b": dict(occupied=[(10, 11, 0)]),
    "c": dict(occupied=[(10, 12, 0)]),
    "d": dict(occupied=[(10, 5, 5)]),
    "wall": dict(wall=20),
    "free": dict(),
    "gap": dict(occupied=[(40, 3, 3)], gap=(24, 0, 0, 32, 8, 8)),
}

# case -> (map, lo, side, d, (status, t_first) with stop_at occupied, (status, t_first) with stop_at unseen), worked by hand:
#   Diagonal3        voxel (10,10,10) is touched on the open interval (9/20, 11/20) on every axis
#   DiagonalTouches  x gives (9/20, 11/20), y gives (10/20, 12/20): entered at 1/2
#   DiagonalOpenEnd  x gives (9/20, 11/20), y gives (11/20, 13/20): they share only an open end, not touched
#   SlideAlongWall*  the box's face slides along the wall's face: nothing touched
#   IntoWall         the box's upper x face 12 + 16 t passes 20 at t = 1/2
#   Leave*           side 2 at 30: the lower face reaches 0 at 30/40, the upper face reaches 64 at 32/40
#   UnseenBefore...  side 1 at x = 10 moving 40: enters the unseen block at (24 - 11)/40, the obstacle at (40 - 11)/40
#   Limit*           x from -2^20 to 2^20 - 1 (or back): the obstacle at x = 10 is entered at (10 - 1 + 2^20)/(2^21 - 1) (back: (2^20 - 1 - 11)/(2^21 - 1))
HAND_CASES = {
    "Diagonal3": ("a", (0, 0, 0), (1, 1, 1), (20, 20, 20), (OCC, Fraction(9, 20)), (OCC, Fraction(9, 20))),
    "DiagonalTouches": ("b", (0, 0, 0), (1, 1, 1), (20, 20, 0), (OCC, Fraction(1, 2)), (OCC, Fraction(1, 2))),
    "DiagonalOpenEnd": ("c", (0, 0, 0), (1, 1, 1), (20, 20, 0), (EMPTY, FREE), (EMPTY, FREE)),
    "SlideAlongWall": ("wall", (19, 5, 5), (1, 2, 2), (0, 30, 7), (EMPTY, FREE), (EMPTY, FREE)),
    "SlideAlongWallFar": ("wall", (21, 40, 40), (3, 2, 2), (0, -30, -7), (EMPTY, FREE), (EMPTY, FREE)),
    "IntoWall": ("wall", (10, 5, 5), (2, 2, 2), (16, 30, 0), (OCC, Fraction(1, 2)), (OCC, Fraction(1, 2))),
    "ZeroMotion": ("a", (8, 9, 9), (3, 3, 3), (0, 0, 0), (OCC, Fraction(0)), (OCC, Fraction(0))),
    "ZeroMotionFree": ("a", (11, 9, 9), (3, 3, 3), (0, 0, 0), (EMPTY, FREE), (EMPTY, FREE)),
    "LeaveXlo": ("free", (30, 30, 30), (2, 2, 2), (-40, 0, 0), (UNSEEN, FREE), (UNSEEN, Fraction(3, 4))),
    "LeaveXhi": ("free", (30, 30, 30), (2, 2, 2), (40, 0, 0), (UNSEEN, FREE), (UNSEEN, Fraction(4, 5))),
    "LeaveYlo": ("free", (30, 30, 30), (2, 2, 2), (0, -40, 0), (UNSEEN, FREE), (UNSEEN, Fraction(3, 4))),
    "LeaveYhi": ("free", (30, 30, 30), (2, 2, 2), (3, 40, 0), (UNSEEN, FREE), (UNSEEN, Fraction(4, 5))),
    "LeaveZlo": ("free", (30, 30, 30), (2, 2, 2), (0, 0, -40), (UNSEEN, FREE), (UNSEEN, Fraction(3, 4))),
    "LeaveZhi": ("free", (30, 30, 30), (2, 2, 2), (0, -5, 40), (UNSEEN, FREE), (UNSEEN, Fraction(4, 5))),
    "Outside": ("free", (-10, -10, -10), (2, 2, 2), (3, 0, 0), (UNSEEN, FREE), (UNSEEN, Fraction(0))),
    "UnseenBeforeObstacle": ("gap", (10, 3, 3), (1, 1, 1), (40, 0, 0), (OCC, Fraction(29, 40)), (OCC, Fraction(13, 40))),
    "BlockedAtStart": ("a", (9, 9, 9), (2, 2, 2), (5, 5, 5), (OCC, Fraction(0)), (OCC, Fraction(0))),
    "LimitLow": ("d", (-LIMIT, 5, 5), (1, 1, 1), (2 * LIMIT - 1, 0, 0), (OCC, Fraction(LIMIT + 9, 2 * LIMIT - 1)), (OCC, Fraction(0))),
    "LimitHigh": ("d", (LIMIT - 1, 5, 5), (1, 1, 1), (-2 * LIMIT + 1, 0, 0), (OCC, Fraction(LIMIT - 12, 2 * LIMIT - 1)), (OCC, Fraction(0))),
    "BeyondLimitSide": ("d", (LIMIT - 1, 5, 5), (2, 1, 1), (0, 0, 0), (INVALID, INVALID_T), (INVALID, INVALID_T)),
    "BeyondLimitMove": ("d", (-LIMIT, 5, 5), (1, 1, 1), (2 * LIMIT, 0, 0), (INVALID, INVALID_T), (INVALID, INVALID_T)),
    "BeyondLimitLo": ("d", (-LIMIT - 1, 5, 5), (1, 1, 1), (0, 0, 0), (INVALID, INVALID_T), (INVALID, INVALID_T)),
    "ZeroSide": ("d", (5, 5, 5), (1, 0, 1), (1, 1, 1), (INVALID, INVALID_T), (INVALID, INVALID_T)),
}


def as_float32(fr):
    """What the C ABI returns for the exact rational: (float)num / (float)den."""
    return np.float32(fr.numerator) / np.float32(fr.denominator)


def stamp_hand_map(p, spec, occupied_x, empty_x):
    """The hand map `spec` on a fresh 64^3 handle, built without depth: the whole volume allocated, set empty, then the obstacles."""
    n = 64
    whole = np.array([[0, 0, 0, n, n, n]], np.int32)
    p.allocate(whole)
    p.edit(whole, empty_x, 1.0)
    boxes = [[x, y, z, x + 1, y + 1, z + 1] for x, y, z in spec.get("occupied", [])]
    if "wall" in spec:
        boxes.append([spec["wall"], 0, 0, spec["wall"] + 1, n, n])
    if boxes:
        p.edit(np.array(boxes, np.int32), occupied_x, 1.0)
    if "gap" in spec:
        p.reset(np.array([spec["gap"]], np.int32))


def valid(m):
    lo, side, d = (np.asarray(m[0:3], np.int64), np.asarray(m[3:6], np.int64), np.asarray(m[6:9], np.int64))
    v = np.concatenate([lo, lo + side, lo + d, lo + side + d])
    return bool((side >= 1).all() and (np.abs(v) <= LIMIT).all())


def _min_fraction(num, den):
    if num.size == 0:
        return FREE
    pairs = np.unique(np.stack([num, den], 1), axis=0)
    return min(Fraction(int(a), int(b)) for a, b in pairs)


def motion_truth(grid, m):
    """The definition over a dense class grid ([z][y][x] uint8 numpy array of the n^3 volume; outside it every voxel is unseen), in int64:
    (status, t_first with stop_at occupied, t_first with stop_at unseen) of the motion m = lo, side, d; t_first as Fractions."""
    if not valid(m):
        return INVALID, INVALID_T, INVALID_T
    n = grid.shape[0]
    lo, side, d = (np.asarray(m[0:3], np.int64), np.asarray(m[3:6], np.int64), np.asarray(m[6:9], np.int64))
    b0 = lo + np.minimum(d, 0)
    b1 = lo + side + np.maximum(d, 0)
    shape = tuple(int(b1[k] - b0[k]) for k in (2, 1, 0))          # [z][y][x]
    Ln, Ld = np.zeros(shape, np.int64), np.ones(shape, np.int64)
    Un, Ud = np.ones(shape, np.int64), np.ones(shape, np.int64)
    ok = np.ones(shape, bool)
    inside = np.ones(shape, bool)
    for k in range(3):
        c = np.arange(b0[k], b1[k], dtype=np.int64)
        view = [1, 1, 1]
        view[2 - k] = -1
        inside &= ((c >= 0) & (c < n)).reshape(view)
        if d[k] == 0:
            ok &= ((lo[k] < c + 1) & (lo[k] + side[k] > c)).reshape(view)
            continue
        a = abs(int(d[k]))
        lower = (c - side[k] - lo[k]) if d[k] > 0 else (lo[k] - c - 1)
        upper = (c + 1 - lo[k]) if d[k] > 0 else (lo[k] + side[k] - c)
        lower, upper = np.broadcast_to(lower.reshape(view), shape), np.broadcast_to(upper.reshape(view), shape)
        up = Ln * a < lower * Ld
        Ln, Ld = np.where(up, lower, Ln), np.where(up, a, Ld)
        dn = upper * Ud < Un * a
        Un, Ud = np.where(dn, upper, Un), np.where(dn, a, Ud)
    touched = ok & (Ln * Ud < Un * Ld)
    cls = np.full(shape, UNSEEN, np.uint8)
    i0, i1 = np.clip(b0, 0, n), np.clip(b1, 0, n)
    if (i0 < i1).all():
        cls[i0[2] - b0[2]:i1[2] - b0[2], i0[1] - b0[1]:i1[1] - b0[1], i0[0] - b0[0]:i1[0] - b0[0]] = grid[i0[2]:i1[2], i0[1]:i1[1], i0[0]:i1[0]]
    assert ((cls == UNSEEN) | inside).all()
    tc = cls[touched]
    status = int(tc.min()) if tc.size else EMPTY
    tn, td = Ln[touched], Ld[touched]
    return status, _min_fraction(tn[tc <= OCC], td[tc <= OCC]), _min_fraction(tn[tc <= UNSEEN], td[tc <= UNSEEN])


def classify(x, y, init, thr, above):
    import torch
    unseen = (x == init[0]) & (y == init[1])
    occ = (x > thr) if above else (x < thr)
    return torch.where(unseen, torch.full_like(x, 1, dtype=torch.uint8),
                       torch.where(occ, torch.zeros_like(x, dtype=torch.uint8), torch.full_like(x, 2, dtype=torch.uint8)))


def class_grid(p, n, dim, thr, above):
    """classify(Octree::get(v)) at every voxel v of the n^3 volume, from se_hip_query_points(coarse) at the voxel centres (a GPU tensor
    [z][y][x] of uint8)."""
    import torch
    dev = torch.device("cuda:0")
    grid = torch.empty((n, n, n), dtype=torch.uint8, device=dev)
    step = np.float32(dim) / np.float32(n)
    ax = (torch.arange(n, device=dev, dtype=torch.float32) + 0.5) * float(step)
    yy, xx = torch.meshgrid(ax, ax, indexing="ij")
    chunk = max(1, (1 << 24) // (n * n))
    for z in range(0, n, chunk):
        zs = ax[z:z + chunk]
        pts = torch.stack([xx.expand(len(zs), n, n), yy.expand(len(zs), n, n), zs.view(-1, 1, 1).expand(len(zs), n, n)], dim=-1).reshape(-1, 3).contiguous()
        c = p.query(pts, fine=False, coarse=True, interp=False, grad=False, status=False)["coarse"]
        grid[z:z + len(zs)] = classify(c[:, 0], c[:, 1], p.init_value(), thr, above).view(len(zs), n, n)
    return grid


def boxes_of(motions):
    """The start box, the end box and the bounding box of each motion, as lo xyz, side xyz (what collides() takes)."""
    m = np.asarray(motions, np.int64)
    lo, side, d = m[:, 0:3], m[:, 3:6], m[:, 6:9]
    start = np.concatenate([lo, side], 1)
    end = np.concatenate([lo + d, side], 1)
    bound = np.concatenate([lo + np.minimum(d, 0), side + np.abs(d)], 1)
    return [np.ascontiguousarray(b.astype(np.int32)) for b in (start, end, bound)]


def check_identities(p, motions, status):
    """What the existing strict box query says about a motion: d = 0 is the box; an axis-aligned d is the bounding box; otherwise, with the
    codes ordered as numbers, collides(bounding box) <= status <= min(collides(start box), collides(end box)).  Returns how many motions had
    each of the three relations checked."""
    start, end, bound = (p.collides(b) for b in boxes_of(motions))
    d = np.asarray(motions)[:, 6:9]
    moving = (d != 0).sum(1)
    assert (status[moving == 0] == start[moving == 0]).all()
    assert (status[moving <= 1] == bound[moving <= 1]).all()
    assert (bound <= status).all() and (status <= np.minimum(start, end)).all()
    return int((moving == 0).sum()), int((moving == 1).sum()), int((moving > 1).sum())
