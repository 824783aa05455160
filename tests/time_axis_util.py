"""What the time-axis tests and the fuse-after-edit tests share: the frame-number schedules, the oracle's run of a schedule (computed once and
kept read-only), the regimes an OFusion update falls into (dt >= 4, dt == 0, dt < 0, judged from the stored values before and after a frame),
the edit lists that are fused over, and the comparisons of a device handle with an oracle snapshot.

The room stream at 160x120 into 128^3 (dim 1.2; mu below): stream index i supplies depth and pose, the frame NUMBER comes from a schedule.  The
frame number reaches the kernels as OFusion's timestamp (1.f / 30.f) * frame, the gates frame % rate == 0 || frame <= 3 and frame > 2, and the
image-ring slot frame % slots."""
import functools

import numpy as np

from oracle.binding import OraclePipeline
from supereight_amd.pipeline import EDIT_BLOCKS, EDIT_DTYPE, EDIT_NODES, EDIT_SET_X, EDIT_SET_Y, OFUSION, SDF
from supereight_amd.synthetic import make_stream
from tests import edit_util
from tests.gpu_state_util import bits

W, H, N, DIM = 160, 120, 128, 1.2
# mu: 0.02 for SDF.  OFusion at 0.02 overflows the reference's key buffer on the first frame: its scan of an empty 128^3 map emits 322 890 keys
# (a 6 mu = 0.12 m band is 12.8 voxels per ray, plus the coarse steps) into the (128 / 8) * 160 * 120 = 307 200 the reference reserves, and
# which keys it then drops depends on the thread interleaving -- the oracle's block set is not defined and stats.truncated counts the scan
# (INTEGRATION.md section 6).  0.015 is 9.6 voxels per ray: 266 378 keys at 128^3 and 513 946 of 614 400 at 256^3, seven eighths of the buffer.
MU = {SDF: 0.02, OFUSION: 0.015}
STREAM_FRAMES = 16

# name -> (frame numbers, integration rate)
SCHEDULES = {
    "gapped": ([0, 1, 2, 3, 60, 61, 200, 201, 700, 701], 1),                     # dt >= 4 at 200 and 700: the max(0.5, .) clamp
    "backwards": ([500, 501, 502, 503, 380, 381, 100, 101], 1),                  # dt < 0; 500 -> 380 is the pole dt = -4
    "plateau_2p24": (list(range(2 ** 24 - 3, 2 ** 24 + 3)), 1),                  # float(frame) stops advancing: dt == 0
    "top_2p32": (list(range(2 ** 32 - 6, 2 ** 32)), 1),                          # every frame maps to the same float
    "three_million": (list(range(3000000, 3000006)), 1),                         # nothing special: a large, still exact frame number
    "rate3": (list(range(12)), 3),                                               # integrates on 0-3, 6, 9
    "rate7": ([0, 1, 2, 3, 5, 7, 13, 14, 21, 22], 7),                            # integrates on 0-3, 7, 14, 21
}


def timestamp(frame):
    """(1.f / 30.f) * frame as the C++ evaluates it: the unsigned frame number rounded to float, one float product."""
    return (np.float32(1) / np.float32(30)) * np.float32(np.uint32(frame))


def ring_slots(frames):
    """The smallest ring in which the frames fall into distinct slots."""
    s = len(frames)
    while len({f % s for f in frames}) != len(frames):
        s += 1
    return s


@functools.lru_cache(maxsize=None)
def stream_frames():
    """(k, depths, poses) of the first STREAM_FRAMES frames of the room stream, read-only."""
    s = make_stream("room", W, H, DIM, holes=False)
    depths = [s.depth(i) for i in range(STREAM_FRAMES)]
    poses = [s.pose(i) for i in range(STREAM_FRAMES)]
    for a in depths + poses:
        a.flags.writeable = False
    return np.ascontiguousarray(s.k, np.float32), depths, poses


def snapshot(p):
    """blocks() + nodes() of an oracle or a device handle, read-only: coords, x, y, active, code, side, node x, node y."""
    st = tuple(p.blocks()) + tuple(p.nodes())
    for a in st:
        a.flags.writeable = False
    return st


def _prior(before, after, init):
    """For every voxel of `after`, what it held in `before` (initValue() where the block did not exist yet)."""
    c0, c1 = before[0].astype(np.int64), after[0].astype(np.int64)
    px = np.full(after[1].shape, np.float32(init[0]), np.float32)
    py = np.full(after[2].shape, np.float32(init[1]), np.float32)
    if len(c0):
        pack = lambda c: (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
        k0, k1 = pack(c0), pack(c1)
        order = np.argsort(k0)
        pos = np.clip(np.searchsorted(k0[order], k1), 0, len(k0) - 1)
        hit = k0[order][pos] == k1
        px[hit], py[hit] = before[1][order[pos[hit]]], before[2][order[pos[hit]]]
    return px, py


def regimes(field, before, after, frame):
    """What a frame did to the stored voxels, judged from the snapshots round it.  A voxel counts as updated when its bits changed (an
    undercount: an OFusion voxel pinned at a clamp with dt == 0 is rewritten with what it held).  OFusion: dt = timestamp - y as the functor
    forms it (in double, rounded to float).  SDF: weights that fell from above 100 to 100, and values outside [-1, 1] brought to +-1."""
    px, py = _prior(before, after, edit_util.INIT[field])
    x, y = after[1], after[2]
    upd = (bits(px) != bits(x)) | (bits(py) != bits(y))
    out = {"updated": int(upd.sum()), "nan": int(np.isnan(x).sum() + np.isnan(y).sum())}
    if field == OFUSION:
        dt = (np.float64(timestamp(frame)) - py.astype(np.float64)).astype(np.float32)
        out.update(dt_ge4=int((upd & (dt >= 4)).sum()), dt_eq0=int((upd & (dt == 0)).sum()), dt_lt0=int((upd & (dt < 0)).sum()),
                   pole=int((upd & (dt == -4)).sum()), clamped=int((upd & (np.abs(x) == 1000)).sum()),
                   plus1000=int((x == 1000).sum()), minus1000=int((x == -1000).sum()))
    else:
        out.update(weight_fell=int((upd & (py > 100) & (y == 100)).sum()), clamped=int((upd & (np.abs(px) > 1) & (np.abs(x) == 1)).sum()))
    return out


def node_nans(st):
    return int(np.isnan(st[6]).sum() + np.isnan(st[7]).sum())


# ------------------------------------------------------------------ the oracle's run of a schedule
@functools.lru_cache(maxsize=3)
def oracle_schedule(field, name):
    """The oracle over SCHEDULES[name]: per frame the return values, the images, the snapshot after the frame and its regimes; computed once,
    shared by the tests of that schedule (dense, pooled, eager, streaming) and left unchanged.  Returns (records, stats)."""
    frames, rate = SCHEDULES[name]
    k, depths, poses = stream_frames()
    cpu = OraclePipeline(field, N, DIM, W, H)
    cpu.count_stats(True)
    recs, before = [], snapshot(cpu)
    for i, f in enumerate(frames):
        ran_i = cpu.integrate(depths[i], poses[i], k, MU[field], f, rate)
        ran_r, v, n = cpu.raycast(poses[i], k, MU[field], f)
        after = snapshot(cpu)
        v.flags.writeable = n.flags.writeable = False
        recs.append({"frame": f, "ran_i": ran_i, "ran_r": ran_r, "v": v, "n": n, "state": after,
                     "regimes": regimes(field, before, after, f) if ran_i else None, "node_nans": node_nans(after)})
        before = after
    stats = cpu.stats()
    cpu.close()
    return recs, stats


# ------------------------------------------------------------------ comparisons
def assert_same_state(want, p, tag):
    """Block set, node set, x, y, node x, node y (bit patterns) and active flags of the handle `p` against an oracle snapshot."""
    got = snapshot(p)
    for nm, i in (("block set", 0), ("active flags", 3), ("node codes", 4), ("node sides", 5)):
        assert want[i].shape == got[i].shape and (want[i] == got[i]).all(), (tag, nm, want[i].shape, got[i].shape)
    for nm, i in (("x", 1), ("y", 2), ("node x", 6), ("node y", 7)):
        bad = np.argwhere(bits(want[i]) != bits(got[i]))
        assert len(bad) == 0, (tag, nm, len(bad), bad[:5].tolist(), want[i][tuple(bad[0])], got[i][tuple(bad[0])])


def assert_same_images(v_c, n_c, v_g, n_g, tag, min_hits=1000):
    hits = int((n_c[..., 0] != -2).sum())
    assert hits >= min_hits, (tag, hits)
    for nm, c, g in (("vertex", v_c, v_g), ("normal", n_c, n_g)):
        bad = (bits(c).reshape(-1, 3) != bits(g).reshape(-1, 3)).any(1)
        assert not bad.any(), (tag, nm, int(bad.sum()), np.nonzero(bad)[0][:5].tolist())


# ------------------------------------------------------------------ edit lists that depth is fused over
F0 = 300            # OFusion: a voxel that reset() puts back to y = 0 then meets dt >= 4 (120 frames) at the next frame
EDIT_KINDS = ("reset", "boxes", "nodes", "list")
SDF_X = np.float32([7, -3, -0.0, 1e-40, 0.99999994])
SDF_Y = np.float32([0, 1, 99, 100, 101, 200, 255])
OF_X = np.float32([1000, -1000, 999.99, -999.99, 0, -0.0, 5e-39])


def _record(lo, hi, x, y, flags, only=7):
    r = np.zeros((), EDIT_DTYPE)
    r["lo"], r["hi"], r["x"], r["y"], r["flags"], r["only"] = lo, hi, x, y, flags, only
    return r


def make_edit_list(kind, field, n, dim, state, v, nrm, next_frame, rng):
    """(records, mode) of the edit list `kind` for a map in `state` whose raycast gave v / nrm.  next_frame is the number of the first frame
    fused on top; its timestamp is "now" for the OFusion timestamps that are written, so that y = now is met with dt == 0 and y = now + 4
    with dt = -4, the pole."""
    coords = state[0]
    hit = nrm[..., 0] != -2
    hv = np.floor(v * np.float32(n / dim)).astype(np.int64)
    pack = lambda c: (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    seen = np.unique(pack((hv[hit] // 8) * 8))
    visible = coords[np.isin(pack(coords.astype(np.int64)), seen)].astype(np.int64)          # allocated blocks with a ray hit inside
    assert len(visible) >= 60, len(visible)
    allf = EDIT_BLOCKS | EDIT_NODES | EDIT_SET_X | EDIT_SET_Y
    init = edit_util.INIT[field]
    now = timestamp(next_frame)
    rows = []
    if kind == "reset":
        # the aligned octant (half the volume's edge) round a visible surface point, as in test_readers_see_the_edit
        centre = hv[H // 2, W // 2] if hit[H // 2, W // 2] else hv[hit][len(hv[hit]) // 2]
        s = n // 2
        lo = (centre // s) * s
        assert (hit & ((hv >= lo + 2) & (hv < lo + s - 2)).all(2)).sum() > 50
        rows.append(_record(lo, lo + s, init[0], init[1], allf))
    elif kind == "boxes":
        if field == SDF:
            values = [(x, y) for x in SDF_X for y in SDF_Y]
        else:
            of_y = np.float32([0, now, now + np.float32(4), now + np.float32(1000), -50, 1e9, 3e38])
            values = [(x, y) for x in OF_X for y in of_y]
        pick = visible[rng.choice(len(visible), len(values), replace=False)]
        for j, ((x, y), c) in enumerate(zip(values, pick)):
            # whole blocks and boxes that cut through one, alternating
            lo, hi = (c, c + 8) if j & 1 else (c + [1, 0, 2], c + [8, 7, 6])
            rows.append(_record(lo, hi, x, y, EDIT_BLOCKS | EDIT_SET_X | EDIT_SET_Y))
    elif kind == "nodes":
        # whole octants of every level above the blocks, round visible blocks: strict mode writes the node value of each
        values = ([(7, 255), (-3, 101), (0.99999994, 200), (-0.0, 100), (1e-40, 0), (0.5, 99)] if field == SDF else
                  [(1000, now), (-1000, now + np.float32(4)), (999.99, -50), (-999.99, 1e9), (5e-39, 0), (-0.0, now + np.float32(1000))])
        for j, (x, y) in enumerate(values):
            s = 16 << (j % 3)
            lo = (visible[rng.integers(len(visible))] // s) * s
            rows.append(_record(lo, lo + s, x, y, EDIT_NODES | EDIT_SET_X | EDIT_SET_Y))
    elif kind == "list":
        hits = v[hit].reshape(-1, 3)
        rec, _ = edit_util.make_edits(rng, field, n, dim, coords, hits)
        return rec, "reference"
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(np.stack(rows)), "strict"


@functools.lru_cache(maxsize=3)
def oracle_fuse_after_edit(field, kind, n):
    """The oracle's side of "fuse, edit, fuse on": 4 frames from F0, the edit list `kind` applied as edit_util.truth of the oracle's own download
    through set_values, a raycast at once, 4 more frames.  Returns a dict: rec, mode, test, before (snapshot the list was made for), edited
    (snapshot after the edit), counts, image (v, n right after the edit), frames (per re-fused frame: frame, v, n, state, regimes), and
    node_touched (edited node values that the next frame's update_node changed)."""
    k, depths, poses = stream_frames()
    mu = MU[field]
    cpu = OraclePipeline(field, n, DIM, W, H)
    cpu.count_stats(True)
    for i in range(4):
        assert cpu.integrate(depths[i], poses[i], k, mu, F0 + i)
    _, v, nrm = cpu.raycast(poses[3], k, mu, F0 + 3)
    before = snapshot(cpu)
    rng = np.random.default_rng(77 + 10 * EDIT_KINDS.index(kind) + field + n)
    rec, mode = make_edit_list(kind, field, n, DIM, before, v, nrm, F0 + 4, rng)
    test = (0.0, field == OFUSION)
    c, x, y, a, code, side, nx, ny = before
    ex, ey, enx, eny, counts, info = edit_util.truth(field, c, x, y, code, side, nx, ny, rec, test, mode)
    assert cpu.set_values(blocks=(c, ex, ey), nodes=(code, side, enx, eny)) == (len(c), len(code))
    edited = snapshot(cpu)
    _, v1, n1 = cpu.raycast(poses[3], k, mu, F0 + 3)
    out = {"rec": rec, "mode": mode, "test": test, "before": before, "edited": edited, "counts": counts, "info": info, "image": (v1, n1), "frames": []}
    prev = edited
    for i in range(4, 8):
        assert cpu.integrate(depths[i], poses[i], k, mu, F0 + i)
        _, vi, ni = cpu.raycast(poses[i], k, mu, F0 + i)
        st = snapshot(cpu)
        out["frames"].append({"frame": F0 + i, "i": i, "v": vi, "n": ni, "state": st, "regimes": regimes(field, prev, st, F0 + i), "node_nans": node_nans(st)})
        if i == 4:
            wrote = (bits(edited[6]) != bits(before[6])) | (bits(edited[7]) != bits(before[7]))
            at = np.searchsorted(st[4], edited[4])                       # (codes are sorted; nodes are never removed)
            assert (st[4][at] == edited[4]).all()
            moved = (bits(st[6][at]) != bits(edited[6])) | (bits(st[7][at]) != bits(edited[7]))
            out["node_written"], out["node_touched"] = int(wrote.sum()), int((wrote & moved).sum())
        prev = st
    out["stats"] = cpu.stats()
    cpu.close()
    return out
