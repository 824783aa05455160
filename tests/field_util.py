"""What the tests of the distance field share (se_hip_distance_field / DenseSLAMPipeline.distance_field): the validity rule of a request,
the numpy truth of a request over a dense class grid -- clearance_truth of tests/clearance_util.py asked once per voxel, so the definition is
literally the clearance's --, the hand-worked requests of tests/cpp/field_kats.cpp with their answers, and the requests the device is held to
on the hand maps of tests/clearance_util.py."""
import numpy as np

from tests.clearance_util import I32_MIN, NONE, NOWHERE, clearance_truth, hand_grid

LIMIT = 1 << 19
R_MAX = 255
ROBOT_MAX = 256
MAX_VOXELS = 1 << 24
MAX_WORK = 1 << 28
_NO = (NONE, NOWHERE)


def valid(lo, side, robot, r_max):
    """The request validity rule of include/se_hip.h."""
    lo, side, robot, r = np.asarray(lo, np.int64), np.asarray(side, np.int64), np.asarray(robot, np.int64), int(r_max)
    if not ((side >= 1).all() and (robot >= 1).all() and (robot <= ROBOT_MAX).all() and 0 <= r <= R_MAX):
        return False
    if (np.abs(lo) > LIMIT).any() or (np.abs(lo + side + robot) > LIMIT).any():
        return False
    if int(side[0]) * int(side[1]) * int(side[2]) > MAX_VOXELS:
        return False
    return int(side[0]) * int(side[1] + robot[1] + 2 * r + 1) * int(side[2] + robot[2] + 2 * r + 1) <= MAX_WORK


def field_truth(grid, request, stop_at, only=None):
    """The definition over a dense class grid ([z][y][x] uint8 numpy array of the n^3 volume; outside it every voxel is unseen): request =
    (lo, side, robot, r_max); returns (d2 [sz, sy, sx] int32, nearest [sz, sy, sx, 3] int32, ties [sz, sy, sx] bool: more than one blocking
    voxel attains d2), each voxel from clearance_truth.  With only (flat indices into [sz, sy, sx]) the three arrays hold those voxels only,
    in that order."""
    lo, side, robot, r = request
    assert valid(lo, side, robot, r)
    count = side[0] * side[1] * side[2]
    flat = np.arange(count) if only is None else np.asarray(only)
    d2, near, ties = np.empty(len(flat), np.int32), np.empty((len(flat), 3), np.int32), np.empty(len(flat), bool)
    for n, f in enumerate(flat.tolist()):
        i, j, k = f % side[0], (f // side[0]) % side[1], f // (side[0] * side[1])
        d, w, c = clearance_truth(grid, [lo[0] + i, lo[1] + j, lo[2] + k, robot[0], robot[1], robot[2], r], stop_at)
        d2[n], near[n], ties[n] = d, w, c > 1
    if only is None:
        shape = (side[2], side[1], side[0])
        return d2.reshape(shape), near.reshape(shape + (3,)), ties.reshape(shape)
    return d2, near, ties


# case -> (map, lo, side, robot, r_max, [(d2, nearest)] per voxel with stop_at occupied, the same with stop_at unseen); worked by hand in the
# header comment of tests/cpp/field_kats.cpp.  None: an invalid request.
_P = (10, 10, 10)
HAND_CASES = {
    "CornerR15": ("a", (0, 0, 0), (1, 1, 1), (1, 1, 1), 15, [_NO], [(0, (-1, -1, -1))]),
    "CornerR16": ("a", (0, 0, 0), (1, 1, 1), (1, 1, 1), 16, [(243, _P)], [(0, (-1, -1, -1))]),
    "WallTie": ("wall", (10, 5, 5), (1, 1, 1), (2, 2, 2), 10, [(64, (20, 4, 4))], [(25, (9, 4, -1))]),
    "FreeR30": ("free", (30, 30, 30), (1, 1, 1), (2, 2, 2), 30, [_NO], [(900, (29, 29, -1))]),
    "FreeR29": ("free", (30, 30, 30), (1, 1, 1), (2, 2, 2), 29, [_NO], [_NO]),
    "GapBox": ("gap", (10, 3, 3), (1, 1, 1), (1, 1, 1), 32, [(841, (40, 3, 3))], [(9, (9, 2, -1))]),
    "OctantCorner": ("octant", (20, 22, 25), (1, 1, 1), (2, 2, 2), 14, [(189, (32, 32, 32))], [(0, (19, 21, 24))]),
    "RowAway": ("a", (12, 10, 10), (3, 1, 1), (1, 1, 1), 3, [(1, _P), (4, _P), (9, _P)], [(1, _P), (4, _P), (9, _P)]),
    "RowRobot": ("a", (5, 10, 10), (4, 1, 1), (3, 1, 1), 2, [(4, _P), (1, _P), (0, _P), (0, _P)], [(4, _P), (1, _P), (0, _P), (0, _P)]),
    "RMax256": ("a", (0, 0, 0), (1, 1, 1), (1, 1, 1), 256, None, None),
    "ZeroRobot": ("a", (0, 0, 0), (1, 1, 1), (1, 0, 1), 4, None, None),
    "Robot257": ("a", (0, 0, 0), (1, 1, 1), (257, 1, 1), 4, None, None),
    "BeyondLimit": ("a", (LIMIT - 2, 0, 0), (1, 1, 1), (2, 1, 1), 4, None, None),
}

# What the device is held to on each hand map, against field_truth: (lo, side, robot, r_max).
_EVERY_MAP = [
    ((3, 5, 7), (13, 9, 11), (1, 1, 1), 9),        # not block-aligned: ragged against bytes and blocks on all sides
    ((20, 20, 20), (4, 4, 4), (1, 1, 1), 1),
    ((-5, -5, -5), (10, 10, 10), (1, 1, 1), 8),    # across the faces z = 0, y = 0, x = 0
    ((70, 70, 70), (4, 4, 4), (8, 8, 8), 7),       # wholly beyond size
    ((66, 3, 60), (3, 4, 6), (2, 2, 2), 1),        # beyond size in x, across the face z = 64
]
DEVICE_REQUESTS = {
    "a": _EVERY_MAP + [
        ((0, 0, 0), (1, 1, 1), (1, 1, 1), 15), ((0, 0, 0), (1, 1, 1), (1, 1, 1), 16),      # CornerR15 / CornerR16: NONE one side, 243 the other
        ((8, 8, 8), (5, 5, 5), (1, 1, 1), 0),
        ((2, 6, 9), (6, 5, 3), (9, 3, 1), 7),
        ((74, 10, 10), (3, 1, 1), (1, 1, 1), 63), ((74, 10, 10), (3, 1, 1), (1, 1, 1), 64), ((74, 10, 10), (3, 1, 1), (1, 1, 1), 65),   # gaps 63, 64, 65
        ((100, 10, 10), (1, 1, 1), (1, 1, 1), 255),                                         # gap 89 under the largest r_max
    ],
    "wall": _EVERY_MAP + [
        ((8, 3, 3), (4, 4, 4), (2, 2, 2), 8), ((8, 3, 3), (4, 4, 4), (2, 2, 2), 7),        # equidistant witnesses at different y and z (cf. WallTie)
        ((9, 6, 6), (5, 3, 3), (8, 8, 8), 9),
    ],
    "free": _EVERY_MAP + [((28, 28, 1), (4, 4, 6), (2, 2, 2), 1)],
    "gap": _EVERY_MAP + [((8, 1, 1), (6, 5, 5), (1, 1, 1), 9), ((36, 0, 0), (8, 6, 6), (2, 2, 2), 7), ((16, 0, 0), (6, 3, 3), (9, 3, 1), 1)],
    "octant": _EVERY_MAP + [((26, 26, 26), (8, 8, 8), (2, 2, 2), 7), ((44, 44, 44), (8, 8, 8), (9, 3, 1), 9), ((20, 30, 30), (5, 4, 4), (8, 8, 8), 8)],
}

_TRUTH = {}


def hand_truth(name, request, stop_at):
    """field_truth of a request on the hand map `name`, computed once."""
    key = (name, request, stop_at)
    if key not in _TRUTH:
        _TRUTH[key] = field_truth(hand_grid(name), request, stop_at)
    return _TRUTH[key]


def d2_of_field(request, nearest):
    """d2 between each voxel's box of the request and the voxel `nearest` names there ([sz, sy, sx, 3]), in int64."""
    lo, side, robot, _ = request
    ax = [np.arange(lo[k], lo[k] + side[k], dtype=np.int64) for k in range(3)]
    v = np.stack(np.broadcast_arrays(ax[0][None, None, :], ax[1][None, :, None], ax[2][:, None, None]), -1)
    w = np.asarray(nearest, np.int64)
    g = np.maximum(0, np.maximum(w - (v + np.asarray(robot, np.int64)), v - (w + 1)))
    return (g * g).sum(-1)


def voxel_boxes(request, grow=0):
    """The box of every voxel of the request, grown by `grow` voxels on every side, in (z, y, x) order: [N, 6] int32 lo xyz, side xyz."""
    lo, side, robot, _ = request
    ax = [np.arange(lo[k], lo[k] + side[k], dtype=np.int64) for k in range(3)]
    v = np.stack(np.broadcast_arrays(ax[0][None, None, :], ax[1][None, :, None], ax[2][:, None, None]), -1).reshape(-1, 3)
    s = np.broadcast_to(np.asarray(robot, np.int64) + 2 * grow, v.shape)
    return np.ascontiguousarray(np.concatenate([v - grow, s], 1).astype(np.int32))
