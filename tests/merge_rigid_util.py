"""What the tests of the rigid map merge share (se_hip_merge_map_rigid, se::merge_map_rigid): the case table of transforms, and the literal
numpy truth -- dense x, y and "block exists" arrays from the downloaded blocks of both maps, every binary32 operation of the definition
one numpy float32 operation in the defined order, the value-pair function of tests/merge_util.py."""
import numpy as np

from tests.host_util import make_keys, unpack
from tests.merge_util import INIT, merge_values, unseen
from tests.shift_util import closure_keys, leaf_level

COUNT_NAMES = ("blocks_combined", "blocks_created", "voxels_observed", "voxels_both")


# ------------------------------------------------------------------ the transforms (destination-from-source, voxels)
def rotation(axis, degrees):
    """Rodrigues' formula in float64."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(degrees)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def quarter_turn_z():
    return np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def half_turn_x():
    return np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]])


def case_transforms(ssize, dsize):
    """name -> (R, t): where the source's content goes in the destination, x_dst = R x_src + t, in voxels.  The rotations turn about the
    source's centre c and carry it to the destination's centre plus the case's translation, so that most of the source lands inside."""
    cs, cd = (ssize - 1) / 2.0 * np.ones(3), np.full(3, (dsize - ssize) // 2 + (ssize - 1) / 2.0)
    cd_int = np.full(3, float((dsize - ssize) // 2))

    def about(R, extra):
        return R, cd - R @ cs + np.asarray(extra, np.float64)
    Rq = quarter_turn_z()
    # quarter: an integer translation -- the centre terms are halves, so the translation is rounded to integers
    tq = np.floor(about(Rq, (0, 0, 0))[1] + np.array([2.0, -3.0, 4.0]))
    # half: fractions exactly 0.5
    th = np.floor(about(half_turn_x(), (0, 0, 0))[1]) + np.array([0.5, 0.5, 0.5])
    return {
        "whole": (np.eye(3), cd_int + np.array([3.0, 0.0, -5.0])),
        "quarter": (Rq, tq),
        "half": (half_turn_x(), th),
        "yaw": about(rotation((0, 1, 0), 30.0), (10.25, -3.5, 6.125)),       # (y is the room's vertical)
        "general": about(rotation((1, 2, 3), 50.0), (0.3 * ssize, -0.45 * ssize, 0.2 * ssize)),      # part of the source leaves the destination
    }


TRANSFORMS = ("whole", "quarter", "half", "yaw", "general")


def pull_of(R, t):
    """src_from_dst, float32 [12]: the inverse of x_dst = R x_src + t in float64, rounded once (what rigid_pull does from a metric pose)."""
    Ri = np.linalg.inv(np.asarray(R, np.float64))
    return np.ascontiguousarray(np.concatenate([Ri, -(Ri @ np.asarray(t, np.float64))[:, None]], 1), np.float32).reshape(12)


def metric_pose(R, t, voxel):
    """The 4x4 metric pose T_dst_src of the same transform."""
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, np.asarray(t, np.float64) * voxel
    return T


# ------------------------------------------------------------------ dense arrays
def dense_of(size, blocks, field):
    """(x [z, y, x], y, exists [bz, by, bx]) of a map from its blocks; initValue() where there is no block."""
    coords, bx, by, _ = blocks
    ix, iy = INIT[field]
    X, Y = np.full((size,) * 3, ix, np.float32), np.full((size,) * 3, iy, np.float32)
    E = np.zeros((size // 8,) * 3, bool)
    for c, vx, vy in zip(np.asarray(coords, np.int64).reshape(-1, 3), bx, by):
        X[c[2]:c[2] + 8, c[1]:c[1] + 8, c[0]:c[0] + 8] = vx.reshape(8, 8, 8)
        Y[c[2]:c[2] + 8, c[1]:c[1] + 8, c[0]:c[0] + 8] = vy.reshape(8, 8, 8)
        E[c[2] // 8, c[1] // 8, c[0] // 8] = True
    return X, Y, E


def positions(pull, dsize, z0=0, z1=None):
    """q of every destination voxel (of the layers z0 .. z1), three float32 arrays [z, y, x]: ((R_k0 vx + R_k1 vy) + R_k2 vz) + t_k, one
    float32 operation each."""
    P = np.asarray(pull, np.float32).reshape(3, 4)
    g = np.arange(dsize, dtype=np.float32)
    vz, vy, vx = np.meshgrid(g[z0:z1], g, g, indexing="ij")
    return [((P[k, 0] * vx + P[k, 1] * vy) + P[k, 2] * vz) + P[k, 3] for k in range(3)]


def samples(ssize, sX, sY, pull, dsize, field, details=False, slab=None):
    """The sample of every destination voxel: (observed [z, y, x], b.x, b.y); b = initValue() where the sample is not observed.
    details: also a dict of masks for the tests' conditions on the model.  slab: that many z layers at a time (large volumes)."""
    if slab is None:
        return _samples(ssize, sX, sY, pull, dsize, field, details, 0, None)
    parts = [_samples(ssize, sX, sY, pull, dsize, field, False, z, z + slab) for z in range(0, dsize, slab)]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def _samples(ssize, sX, sY, pull, dsize, field, details, z0, z1):
    ix, iy = INIT[field]
    q = positions(pull, dsize, z0, z1)
    assert all(a.dtype == np.float32 for a in q)
    fl = [np.floor(a) for a in q]
    f = [a - b for a, b in zip(q, fl)]
    inside = np.ones(q[0].shape, bool)
    for a in fl:
        inside &= (a >= 0) & (a <= ssize - 2)
    l = [np.where(inside, a, 0).astype(np.int64) for a in fl]
    p, w, corner_unseen = [], None, []
    for c in range(8):
        i, j, k = c & 1, (c >> 1) & 1, c >> 2
        px, py = sX[l[2] + k, l[1] + j, l[0] + i], sY[l[2] + k, l[1] + j, l[0] + i]
        p.append(px)
        corner_unseen.append(unseen(px, py, field))
        w = py if w is None else (np.fmin(w, py) if field == 0 else np.fmax(w, py))
    n_unseen = np.sum(corner_unseen, 0)
    valid = inside & (n_unseen == 0)
    one = np.float32(1)
    fx, fy, fz = f
    bx = (((p[0] * (one - fx) + p[1] * fx) * (one - fy) + (p[2] * (one - fx) + p[3] * fx) * fy) * (one - fz) +
          ((p[4] * (one - fx) + p[5] * fx) * (one - fy) + (p[6] * (one - fx) + p[7] * fx) * fy) * fz)
    assert bx.dtype == np.float32 and w.dtype == np.float32
    observed = valid & ~unseen(bx, w, field)
    bx, by = np.where(observed, bx, np.float32(ix)).astype(np.float32), np.where(observed, w, np.float32(iy)).astype(np.float32)
    if not details:
        return observed, bx, by
    straddle = [inside & ((a & 7) == 7) for a in l]
    n_straddle = np.sum(straddle, 0)
    info = {"outside": ~inside, "partly_unseen": inside & (n_unseen > 0) & (n_unseen < 8),
            "straddle_all": observed & (n_straddle == 3), "straddle_one": observed & (n_straddle == 1), "q": q, "f": f}
    return observed, bx, by, info


def _blocked(a):
    """[z, y, x] -> [bz, by, bx, 512] with voxel index x + 8 y + 64 z."""
    n = a.shape[0] // 8
    return a.reshape(n, 8, n, 8, n, 8).transpose(0, 2, 4, 1, 3, 5).reshape(n, n, n, 512)


def merge_rigid_truth(dsize, dst_blocks, dst_nodes, ssize, src_blocks, pull, mode, field, max_weight=100, details=False, slab=None):
    """se_hip_merge_map_rigid by its definition.  blocks = (coords [nb, 3], x [nb, 512], y [nb, 512], active [nb]) and nodes = (code [nn],
    side, nx [nn, 8], ny [nn, 8]) sorted by key, as DenseSLAMPipeline.blocks() / nodes() deliver them.
    Returns (blocks, nodes, counts int64 [10]) of the destination afterwards, in the same form (details: and the masks of samples())."""
    dc, _, _, dact = dst_blocks
    dcode, _, dnx, dny = dst_nodes
    ix, iy = INIT[field]
    leaf = leaf_level(dsize)
    sX, sY, _ = dense_of(ssize, src_blocks, field)
    dX, dY, dE = dense_of(dsize, dst_blocks, field)
    out = samples(ssize, sX, sY, pull, dsize, field, details, slab)
    observed, bx, by = out[:3]
    mx, my = merge_values(dX, dY, bx, by, mode, field, max_weight)          # (b = initValue() leaves a, bit for bit)
    received = _blocked(observed).any(3)                                    # [bz, by, bx]
    zyx = np.argwhere(received)
    rc = zyx[:, ::-1] * 8                                                   # corners (x, y, z) of the blocks that received samples
    rk = make_keys(rc, leaf) if len(rc) else np.zeros(0, np.uint64)
    dkeys = make_keys(dc, leaf) if len(dc) else np.zeros(0, np.uint64)
    out_bk = np.array(sorted(set(dkeys.tolist()) | set(rk.tolist())), np.uint64)
    ocoords = unpack(out_bk & ~np.uint64(0x1FF)).astype(np.int32).reshape(-1, 3)
    bmx, bmy = _blocked(mx), _blocked(my)
    at = (ocoords[:, 2] // 8, ocoords[:, 1] // 8, ocoords[:, 0] // 8)
    ox, oy = np.ascontiguousarray(bmx[at]), np.ascontiguousarray(bmy[at])
    oact = np.ones(len(out_bk), np.uint8)                                   # a block that received a sample is active, created or not
    keep = ~np.isin(out_bk, rk)
    oact[keep] = np.asarray(dact, np.uint8)[np.searchsorted(dkeys, out_bk[keep])]
    created = ~np.isin(rk, dkeys)
    closure = closure_keys(dsize, rc[created], np.full(int(created.sum()), leaf)) if created.any() else set()
    out_nk = np.array(sorted(set(dcode.tolist()) | {0} | {k for k in closure if k & 0x1FF != leaf}), np.uint64)
    onx, ony = np.full((len(out_nk), 8), ix, np.float32), np.full((len(out_nk), 8), iy, np.float32)
    at_dn = np.searchsorted(out_nk, dcode)
    onx[at_dn], ony[at_dn] = dnx, dny
    oside = (dsize >> (out_nk & np.uint64(0x1FF)).astype(np.int64)).astype(np.uint32)
    counts = np.zeros(10, np.int64)
    counts[:4] = [(~created).sum(), created.sum(), observed.sum(), (observed & ~unseen(dX, dY, field)).sum()]
    if len(rc):
        counts[4:7], counts[7:10] = rc.min(0), rc.max(0) + 8
    res = (ocoords, ox, oy, oact), (out_nk, oside, onx, ony), counts
    return res + (out[3],) if details else res


def counts_of(result):
    """The dict DenseSLAMPipeline.merge_rigid returns -> int64 [10] in the order of the C ABI."""
    return np.array([result[k] for k in COUNT_NAMES] + list(result["region"][0]) + list(result["region"][1]), np.int64)
