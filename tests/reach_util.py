"""What the tests of the reachability field share (se_hip_reach_field / DenseSLAMPipeline.reach_field): the validity rule of a request, the
numpy truth of a request over a dense class grid (the definition of include/se_hip.h, iterated to its fixed point), the hand map `comb`
beside the hand maps of tests/clearance_util.py, the hand-worked requests of tests/cpp/reach_kats.cpp with their answers, and the requests the
device is held to on the hand maps."""
import numpy as np

from tests.clearance_util import CLEAR_MAPS, EMPTY, OCC, UNSEEN, hand_grid, stamp_clear_map
from tests.motion_util import stamp_hand_map

LIMIT = 1 << 19
ROBOT_MAX = 256
MAX_POSITIONS = 1 << 24
MAX_SEEDS = 255
NONE, AT_SEED, NO_SEED, NO_MOVE = -1, 6, 255, 255
NOKEY = 0xFFFFFFFF
MOVES = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))      # codes 0 .. 5, as (x, y, z)

# `comb` on a 64^3 volume: every block allocated and empty; the planes x = 4 k, k = 1 .. 15, occupied over all y and z but for a slot left
# empty -- y in [0, 3) for odd k, y in [61, 64) for even k --; an unseen pocket x 41 .. 43, y 30 .. 37, z 20 .. 27
COMB_POCKET = (41, 30, 20, 44, 38, 28)
REACH_MAPS = CLEAR_MAPS + ("comb",)


def _comb_planes():
    return [[4 * k, 3, 0, 4 * k + 1, 64, 64] if k % 2 else [4 * k, 0, 0, 4 * k + 1, 61, 64] for k in range(1, 16)]


def stamp_reach_map(p, name, occupied_x, empty_x):
    """The hand map `name` on a fresh 64^3 handle, built without depth."""
    if name != "comb":
        return stamp_clear_map(p, name, occupied_x, empty_x)
    stamp_hand_map(p, {}, occupied_x, empty_x)
    p.edit(np.array(_comb_planes(), np.int32), occupied_x, 1.0)
    p.reset(np.array([COMB_POCKET], np.int32))


_GRIDS = {}


def reach_grid(name):
    """The class grid [z][y][x] of the hand map `name` (not to be written to)."""
    if name not in _GRIDS:
        if name == "comb":
            g = np.full((64, 64, 64), EMPTY, np.uint8)
            for x0, y0, z0, x1, y1, z1 in _comb_planes():
                g[z0:z1, y0:y1, x0:x1] = OCC
            x0, y0, z0, x1, y1, z1 = COMB_POCKET
            g[z0:z1, y0:y1, x0:x1] = UNSEEN
        else:
            g = hand_grid(name)
        _GRIDS[name] = g
    return _GRIDS[name]


def valid(lo, side, robot, n_seeds=1):
    """The request validity rule of include/se_hip.h."""
    lo, side, robot = np.asarray(lo, np.int64), np.asarray(side, np.int64), np.asarray(robot, np.int64)
    if not ((side >= 1).all() and (robot >= 1).all() and (robot <= ROBOT_MAX).all() and 1 <= n_seeds <= MAX_SEEDS):
        return False
    if (np.abs(lo) > LIMIT).any() or (np.abs(lo + side + robot) > LIMIT).any():
        return False
    return int(side[0]) * int(side[1]) * int(side[2]) <= MAX_POSITIONS


def free_positions(grid, request, stop_at):
    """free [sz, sy, sx] bool of request = (lo, side, robot) over a dense class grid ([z][y][x] uint8 of the n^3 volume; outside it every voxel
    is unseen): no voxel of [v, v + robot) has a class <= stop_at."""
    lo, side, robot = request
    n = grid.shape[0]
    lo, D = np.asarray(lo, np.int64), np.asarray(side, np.int64) + np.asarray(robot, np.int64) - 1
    cls = np.full((D[2], D[1], D[0]), UNSEEN, np.uint8)
    i0, i1 = np.clip(lo, 0, n), np.clip(lo + D, 0, n)
    if (i0 < i1).all():
        cls[i0[2] - lo[2]:i1[2] - lo[2], i0[1] - lo[1]:i1[1] - lo[1], i0[0] - lo[0]:i1[0] - lo[0]] = grid[i0[2]:i1[2], i0[1]:i1[1], i0[0]:i1[0]]
    blocked = cls <= stop_at
    for axis, r, s in ((2, robot[0], side[0]), (1, robot[1], side[1]), (0, robot[2], side[2])):      # separable: a window OR per axis
        acc = np.zeros_like(np.take(blocked, range(s), axis))
        for t in range(r):
            acc |= np.take(blocked, range(t, t + s), axis)
        blocked = acc
    return ~blocked


def reach_truth(grid, request, seeds, stop_at):
    """The definition: request = (lo, side, robot), seeds [n][3] absolute (x, y, z).  Returns free [sz, sy, sx] bool, steps int32, seed uint8,
    next uint8, counts (free positions, reached positions, the largest steps or -1) -- key = min(key, shifted neighbours + 256) under the free
    mask, iterated until nothing changes, in int64."""
    lo, side, robot = request
    assert valid(lo, side, robot, len(seeds))
    free = free_positions(grid, request, stop_at)
    big = np.int64(1) << 40
    key = np.full(free.shape, big, np.int64)
    for i, s in enumerate(np.asarray(seeds, np.int64).reshape(-1, 3).tolist()):
        r = [s[k] - lo[k] for k in range(3)]
        if all(0 <= r[k] < side[k] for k in range(3)) and free[r[2], r[1], r[0]]:
            key[r[2], r[1], r[0]] = min(key[r[2], r[1], r[0]], i)

    pad = np.pad(key, 1, constant_values=big)                   # `big` across the region's faces
    sz, sy, sx = key.shape
    inner = pad[1:-1, 1:-1, 1:-1]

    def neighbours():
        """views of the neighbour's key in each direction, in the order of MOVES"""
        return [pad[1 + dz:1 + dz + sz, 1 + dy:1 + dy + sy, 1 + dx:1 + dx + sx] for dx, dy, dz in MOVES]

    while True:
        new = np.where(free, np.minimum(inner, np.minimum.reduce(neighbours()) + 256), inner)
        if (new == inner).all():
            break
        inner[...] = new
    key = inner
    reached = key < big
    steps = np.where(reached, key >> 8, NONE).astype(np.int32)
    seed = np.where(reached, key & 255, NO_SEED).astype(np.uint8)
    nxt = np.full(free.shape, NO_MOVE, np.uint8)
    nxt[reached] = AT_SEED
    for code in range(5, -1, -1):                                 # descending: the lowest qualifying direction is the one kept
        nxt[reached & (steps > 0) & (neighbours()[code] + 256 == key)] = code
    counts = (int(free.sum()), int(reached.sum()), int(steps.max()) if reached.any() else -1)
    return free, steps, seed, nxt, counts


def next_choices(steps, seed):
    """How many directions qualify for next at each reached position with steps > 0 (from steps and seed alone: key = steps * 256 + seed)."""
    reached = steps >= 0
    key = np.where(reached, steps.astype(np.int64) * 256 + seed, np.int64(1) << 40)
    n = np.zeros(steps.shape, np.int32)
    for dx, dy, dz in MOVES:
        pad = np.pad(key, 1, constant_values=np.int64(1) << 40)
        n += pad[1 + dz:1 + dz + key.shape[0], 1 + dy:1 + dy + key.shape[1], 1 + dx:1 + dx + key.shape[2]] + 256 == key
    return np.where(reached & (steps > 0), n, 0)


def equidistant(grid, request, seeds, stop_at):
    """Positions whose nearest usable seed is not unique: the index rule decided.  (One truth per seed alone, compared.)"""
    _, steps, _, _, _ = reach_truth(grid, request, seeds, stop_at)
    best = np.zeros(steps.shape, np.int32)
    for s in {tuple(s) for s in np.asarray(seeds).reshape(-1, 3).tolist()}:
        one = reach_truth(grid, request, [s], stop_at)[1]
        best += (one >= 0) & (one == steps)
    return best >= 2


# The table of the issue: `comb` with seeds (1, 1, 4) and (62, 62, 4); (lo, side, robot, stop_at) -> (free, reached, max steps, usable seeds)
COMB_SEEDS = ((1, 1, 4), (62, 62, 4))
COMB_TABLE = [
    (((0, 0, 0), (64, 64, 8), (1, 1, 1)), OCC, (25448, 25448, 478), (0, 1)),
    (((0, 0, 0), (64, 64, 8), (3, 3, 3)), UNSEEN, (8792, 8792, 980), (0,)),
    (((0, 0, 0), (64, 64, 8), (3, 4, 1)), OCC, (10232, 2560, 67), (0, 1)),
    (((0, 0, 0), (64, 64, 8), (4, 1, 1)), UNSEEN, (1952, 608, 67), (0,)),
    (((-3, -3, 2), (70, 70, 6), (1, 1, 1)), OCC, (23910, 23910, 72), (0, 1)),
    (((-3, -3, 2), (70, 70, 6), (1, 1, 1)), UNSEEN, (19086, 19086, 477), (0, 1)),
]

# case -> (map, lo, side, robot, seeds, (steps, seed, next) flat in (z, y, x) order with stop_at occupied, the same with stop_at unseen); worked
# by hand in the header comment of tests/cpp/reach_kats.cpp.  None: an invalid request.
_X = (NONE, NO_SEED, NO_MOVE)
HAND_CASES = {
    # a row of five through (10, 10, 10), which is occupied: the seed at 8 reaches 8 and 9, the seed at 12 reaches 11 and 12
    "RowSplit": ("a", (8, 10, 10), (5, 1, 1), (1, 1, 1), ((8, 10, 10), (12, 10, 10)),
                 [(0, 0, AT_SEED), (1, 0, 0), _X, (1, 1, 1), (0, 1, AT_SEED)], [(0, 0, AT_SEED), (1, 0, 0), _X, (1, 1, 1), (0, 1, AT_SEED)]),
    # a free row of five, seeds at both ends: the middle is equidistant and goes to seed 0
    "RowTie": ("free", (30, 30, 30), (5, 1, 1), (1, 1, 1), ((30, 30, 30), (34, 30, 30)),
               [(0, 0, AT_SEED), (1, 0, 0), (2, 0, 0), (1, 1, 1), (0, 1, AT_SEED)], [(0, 0, AT_SEED), (1, 0, 0), (2, 0, 0), (1, 1, 1), (0, 1, AT_SEED)]),
    # a 2 x 2 square, one seed in a corner: the far corner may go -x or -y, the lower code wins; a duplicate seed and one outside change nothing
    "SquareNext": ("free", (30, 30, 30), (2, 2, 1), (1, 1, 1), ((30, 30, 30), (30, 30, 30), (29, 30, 30)),
                   [(0, 0, AT_SEED), (1, 0, 0), (1, 0, 2), (2, 0, 0)], [(0, 0, AT_SEED), (1, 0, 0), (1, 0, 2), (2, 0, 0)]),
    # a robot of two along x: the positions 9 and 10 hold (10, 10, 10) and cut 7, 8 off from 11; the seed at 9 is not free, the seed at 11 is
    "RobotTwo": ("a", (7, 10, 10), (5, 1, 1), (2, 1, 1), ((9, 10, 10), (11, 10, 10)),
                 [_X, _X, _X, _X, (0, 1, AT_SEED)], [_X, _X, _X, _X, (0, 1, AT_SEED)]),
    # across the wall x = 20, inside the volume: cut off
    "WallCut": ("wall", (18, 5, 5), (5, 1, 1), (1, 1, 1), ((18, 5, 5),),
                [(0, 0, AT_SEED), (1, 0, 0), _X, _X, _X], [(0, 0, AT_SEED), (1, 0, 0), _X, _X, _X]),
    # across the face x = 0: the positions outside are unseen, free with stop_at occupied only
    "AcrossFace": ("free", (-2, 5, 5), (4, 1, 1), (1, 1, 1), ((1, 5, 5),),
                   [(3, 0, 1), (2, 0, 1), (1, 0, 1), (0, 0, AT_SEED)], [_X, _X, (1, 0, 1), (0, 0, AT_SEED)]),
    # no usable seed at all: one on the occupied voxel, one at the ends of int32
    "NoSeed": ("a", (10, 10, 10), (2, 1, 1), (1, 1, 1), ((10, 10, 10), (2147483647, -2147483648, 0)),
               [_X, _X], [_X, _X]),
    "ZeroRobot": ("a", (0, 0, 0), (1, 1, 1), (1, 0, 1), ((0, 0, 0),), None, None),
    "Robot257": ("a", (0, 0, 0), (1, 1, 1), (257, 1, 1), ((0, 0, 0),), None, None),
    "BeyondLimit": ("a", (LIMIT - 2, 0, 0), (1, 1, 1), (2, 1, 1), ((0, 0, 0),), None, None),
}

# What the device is held to on each hand map, against reach_truth: (lo, side, robot, seeds).  The tile of the relaxation is 32 x 8 x 8.
_EVERY_MAP = [
    ((3, 5, 7), (13, 9, 11), (1, 1, 1), ((4, 6, 8), (15, 13, 17))),              # not block-aligned
    ((20, 20, 20), (1, 1, 1), (1, 1, 1), ((20, 20, 20),)),                       # one position
    ((-5, -5, -5), (10, 10, 10), (2, 2, 2), ((-5, -5, -5), (3, 3, 3))),          # across the faces at 0
    ((70, 70, 70), (4, 4, 4), (3, 3, 3), ((71, 71, 71),)),                       # wholly beyond size
    ((60, 3, 60), (9, 4, 6), (2, 2, 2), ((61, 4, 61), (67, 5, 64))),             # across the faces x = 64 and z = 64
    ((8, 8, 8), (32, 8, 8), (1, 1, 1), ((9, 9, 9), (39, 15, 15))),               # one tile
    ((1, 2, 3), (70, 19, 21), (1, 1, 1), ((2, 3, 4), (60, 20, 22), (60, 20, 22), (1, 1, 1))),   # three tiles along every axis, no multiple of it
]
DEVICE_REQUESTS = {
    "a": _EVERY_MAP + [((2, 6, 9), (16, 9, 5), (9, 3, 1), ((3, 7, 10), (17, 14, 13))), ((5, 5, 5), (12, 12, 12), (3, 3, 3), ((5, 5, 5), (16, 16, 16)))],
    "wall": _EVERY_MAP + [
        ((10, 4, 4), (20, 12, 6), (1, 1, 1), ((11, 5, 5),)),                     # straddles x = 20 inside the volume: cut off
        ((10, -4, 4), (20, 12, 6), (1, 1, 1), ((11, 5, 5),)),                    # reaches below y = 0: round the outside with stop_at occupied
        ((10, -4, 4), (20, 12, 6), (4, 1, 1), ((11, 5, 5), (25, 5, 5))),
    ],
    "free": _EVERY_MAP + [((28, 28, 1), (4, 4, 6), (2, 2, 2), ((28, 28, 1), (31, 31, 6)))],
    "gap": _EVERY_MAP + [((16, 0, 0), (30, 12, 12), (1, 1, 1), ((17, 1, 1), (44, 10, 10))), ((16, 0, 0), (30, 12, 12), (4, 1, 1), ((17, 1, 1),))],
    "octant": _EVERY_MAP + [((26, 26, 26), (30, 30, 30), (2, 2, 2), ((27, 27, 27), (50, 50, 50))), ((20, 30, 30), (40, 9, 9), (9, 3, 1), ((21, 31, 31),))],
    "comb": _EVERY_MAP + [(rq[0], rq[1], rq[2], COMB_SEEDS) for rq, _, _, _ in COMB_TABLE]
            + [((30, 20, 16), (24, 30, 16), (1, 1, 1), ((31, 25, 18), (50, 45, 30))), ((30, 20, 16), (24, 30, 16), (3, 3, 3), ((37, 25, 18),))],
}

_TRUTH = {}


def hand_truth(name, request, seeds, stop_at):
    """reach_truth of a request on the hand map `name`, computed once (not to be written to)."""
    k = (name, request, tuple(map(tuple, seeds)), stop_at)
    if k not in _TRUTH:
        _TRUTH[k] = reach_truth(reach_grid(name), request, seeds, stop_at)
    return _TRUTH[k]
