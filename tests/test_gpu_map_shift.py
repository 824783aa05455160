"""The map shift on the device (se_hip_shift_map / DenseSLAMPipeline.shift) through the C ABI, everything bit for bit: the state after a
shift against the numpy truth of tests/shift_util.py applied to the state before (SDF and OFusion, dense and pooled, 128^3 and 256^3);
the derived structures, by running on after the shift beside a fresh handle that loaded the shifted map from a file; integer queries
that move with the map; the pool invariants; the contract (invalid shifts, tracking, capacity)."""
import ctypes as C

import numpy as np
import pytest

from supereight_amd.pipeline import COLLISION_UNSEEN, OFUSION, SDF, DenseSLAMPipeline, SeHipError
from supereight_amd.synthetic import make_stream
from tests.gpu_state_util import H, W, bits, map_state, run_stream, streamed_with
from tests.host_util import LIMIT
from tests.shift_util import equal_blocks_nodes, shift_truth, shifts_for, survivors, write_map_file

pytestmark = pytest.mark.gpu
INIT = {SDF: (1.0, 0.0), OFUSION: (0.0, 0.0)}    # voxel_traits<T>::initValue()
FRAMES = 6


def _dim(n):
    return 2.4 * n / 256


def _pool(n, pooled):
    return 0 if not pooled else (n // 8) ** 3 // 2


def _name(field, n, pooled):
    return f"{'sdf' if field == SDF else 'ofusion'}_{n}_{'pooled' if pooled else 'dense'}"


def _state(p):
    return p.blocks(), p.nodes()


def _same(a, b):
    return all((u == w).all() for u, w in zip(a, b))


def _shift_and_check(p, s, field):
    """p.shift(s) against the truth applied to the state before; the images must not change.  Returns the counts."""
    before_b, before_n = _state(p)
    images = [bits(a) for a in p.vertex_normal()]
    pose = p.pose_.copy()
    want_b, want_n, want_c = shift_truth(p.size, s, before_b, before_n, INIT[field])
    counts = p.shift(s)
    got_b, got_n = _state(p)
    print(f"shift {s}: counts {counts.tolist()} blocks {len(got_b[0])} nodes {len(got_n[0])}")
    assert equal_blocks_nodes(got_b, got_n, want_b, want_n) is None, (s, equal_blocks_nodes(got_b, got_n, want_b, want_n))
    assert counts.tolist() == want_c.tolist(), s
    assert p.counts() == (len(want_b[0]), len(want_n[0]))
    assert _same(images, [bits(a) for a in p.vertex_normal()])
    voxel = np.float32(p.dim) / np.float32(p.size)
    assert (bits(p.pose_[:3, 3]) == bits(pose[:3, 3] + np.asarray(s, np.float32) * voxel)).all() and (p.pose_[:, :3] == pose[:, :3]).all()
    return counts


CONFIGS = [(f, n, m) for f in (SDF, OFUSION) for n in (128, 256) for m in (0, 1)]


# ------------------------------------------------------------------ 1. the state equals the restatement
@pytest.mark.parametrize("group", ["small", "aligned", "half", "size"])
@pytest.mark.parametrize("field,n,pooled", CONFIGS, ids=[_name(*c) for c in CONFIGS])
def test_state_equals_the_restatement(field, n, pooled, group):
    p = run_stream("stress" if pooled else "room", field, n, _dim(n), _pool(n, pooled), FRAMES)
    try:
        assert ("pooled" in p.memory_info()["layout"]) == bool(pooled)
        (coords, x, y, act), (code, side, nx, ny) = _state(p)
        assert len(coords) > 100 and act.min() == 0 and act.max() == 1          # the active comparison sees both values
        shifts = list(shifts_for(n)[group])
        if group == "small":
            before = map_state(p)
            assert p.shift((0, 0, 0)).tolist() == [len(coords), 0, len(code), 0]
            assert _same(before, map_state(p))                                   # s = 0: the whole state, images included
        if group == "half":
            # half of the block bounding box leaves through the lower x face
            mid = (int(coords[:, 0].min()) + int(coords[:, 0].max()) + 8) // 2 // 8 * 8
            c = _shift_and_check(p, (-mid, 0, 0), field)
            assert c[0] > 0 and c[1] > 0
        if group == "aligned" and field == OFUSION:
            # a 64-aligned shift under which a node survives that holds something: node carry is tested (the first of the six that does)
            ix, iy = INIT[field]
            for s in [(64, 0, 0), (-64, 0, 0), (0, 64, 0), (0, -64, 0), (0, 0, 64), (0, 0, -64)]:
                keep_n = survivors(n, s, coords, code)[2]
                if ((nx[keep_n] != ix) | (ny[keep_n] != iy)).any():
                    shifts[0] = s
                    break
            else:
                raise AssertionError("no 64-aligned shift keeps a node with a value: node carry is not tested")
        for s in shifts:
            _shift_and_check(p, s, field)
        if group != "small":
            assert p.counts()[0] == 0 or group == "half"
    finally:
        p.close()


# ------------------------------------------------------------------ 2. the derived structures
def _run_on(p, s_, stream, frames, mu, move, check):
    for f in frames:
        p.set_depth(stream.depth(f))
        pose = stream.pose(f).copy()
        pose[:3, 3] += move
        p.setPose(pose)
        p.integration(stream.k, 1, mu, f)
        p.raycasting(stream.k, mu, f)
        check(p, f)


def _twin_run(kind, field, n, dim, max_blocks, pre, post, s, tmp_path):
    """Handle A: `pre` frames, shift(s), `post` frames with the poses moved by s * voxel.  Handle B, fresh: loads the file numpy makes of A's
    state before the shift, then the same frames.  The images after every frame, and the maps at the end."""
    mu = 0.1 if field == SDF else 0.02
    move = np.asarray(s, np.float32) * (np.float32(dim) / np.float32(n))
    a = run_stream(kind, field, n, dim, max_blocks, pre)
    b = DenseSLAMPipeline((W, H), n, dim, field_type=field, max_blocks=max_blocks)
    try:
        blocks, nodes = _state(a)
        want_b, want_n, want_c = shift_truth(n, s, blocks, nodes, INIT[field])
        path = str(tmp_path / "shifted.bin")
        write_map_file(path, n, dim, field, want_b, want_n)
        counts = a.shift(s)
        assert counts.tolist() == want_c.tolist() and counts[0] > 0 and counts[1] > 0
        b.load(path)
        (bc, bx, by, bact), b_nodes = _state(b)
        a_blocks, a_nodes = _state(a)
        assert (bact == 1).all() and equal_blocks_nodes(a_blocks, a_nodes, (bc, bx, by, a_blocks[3]), b_nodes) is None      # (load: all active)
        images, flags = {}, {}
        sa, sb = make_stream(kind, W, H, dim, holes=False), make_stream(kind, W, H, dim, holes=False)
        for st in (sa, sb):
            for f in range(pre):
                st.depth(f)                                    # (the streams hand out frames in order)
        frames = list(range(pre, pre + post))
        _run_on(a, s, sa, frames, mu, move, lambda p, f: (images.__setitem__(("a", f), [bits(v) for v in p.vertex_normal()]), flags.__setitem__(("a", f), p.block_flags())))
        _run_on(b, s, sb, frames, mu, move, lambda p, f: (images.__setitem__(("b", f), [bits(v) for v in p.vertex_normal()]), flags.__setitem__(("b", f), p.block_flags())))
        for f in frames:
            assert _same(images[("a", f)], images[("b", f)]), f
            assert (flags[("a", f)][0] == flags[("b", f)][0]).all(), f
            if f >= pre + 1:
                assert (flags[("a", f)][1] == flags[("b", f)][1]).all(), f
        assert images[("a", frames[-1])][0].any()
        assert equal_blocks_nodes(*_state(a), *_state(b)) is None
        assert a.counts() == b.counts()
    finally:
        a.close(); b.close()


TWINS = [(f, m) for f in (SDF, OFUSION) for m in (0, 1)]


@pytest.mark.parametrize("field,pooled", TWINS, ids=[_name(f, 256, m) for f, m in TWINS])
def test_frames_after_a_shift_equal_a_fresh_handle_with_the_shifted_map(field, pooled, tmp_path):
    _twin_run("room", field, 256, 2.4, _pool(256, pooled), 4, 4, (-64, 0, 32), tmp_path)


@pytest.mark.parametrize("pooled", [0, 1], ids=["dense", "pooled"])
def test_frames_after_a_shift_at_1024(pooled, tmp_path):
    """1024^3: fbits[] is not the block grid, lbits[] is consulted by the march, and the dense block list is sorted."""
    _twin_run("stress", SDF, 1024, 4.8, 65536 if pooled else 0, 3, 3, (-128, 0, 64), tmp_path)


def _streaming_handle(n, dim, field, slots):
    """A streaming handle whose raycasts go into an image ring (the streamed_with pattern): (pipeline, ring)."""
    import torch
    p = DenseSLAMPipeline((W, H), n, dim, field_type=field, streaming=True)
    ring = torch.zeros((slots, 2, W * H * 3), dtype=torch.float32, device="cuda:0")
    p.set_image_ring(ring.data_ptr(), slots, keepalive=ring)
    return p, ring


def test_a_held_back_raycast_is_launched_before_the_shift(tmp_path):
    """The twin run on the one-queue streaming schedule (deferred raycasts into an image ring, fused raycast + scan launches, occupancy bits
    deferred): handle A is shifted after frame 5 with that frame's raycast held back -- the launch counters show it flushed first, on its
    own -- and runs on with the poses moved by s * voxel; handle B, fresh and streaming too, loads the file numpy makes of the map before
    the shift (taken from an eager handle over the same frames: asking A would launch the held-back raycast) and replays the same
    frames.  Ring images of every frame after the shift, and the maps at the end, bit for bit."""
    n, dim, mu, s, at, frames, slots = 256, 2.4, 0.1, (-64, 0, 32), 5, 10, 12
    move = np.asarray(s, np.float32) * (np.float32(dim) / np.float32(n))
    plain, _ = streamed_with(lambda p, box: None, -1)
    eager = run_stream("room", SDF, n, dim, 0, at + 1)
    want_b, want_n, want_c = shift_truth(n, s, *_state(eager), INIT[SDF])
    eager.close()
    path = str(tmp_path / "shifted.bin")
    write_map_file(path, n, dim, SDF, want_b, want_n)

    def frame(p, stream, f):
        p.set_depth(stream.depth(f))
        pose = stream.pose(f).copy()
        if f > at:
            pose[:3, 3] += move
        p.setPose(pose)
        p.integration(stream.k, 1, mu, f)
        p.raycasting_deferred(stream.k, mu, f)

    a, ring_a = _streaming_handle(n, dim, SDF, slots)
    b, ring_b = _streaming_handle(n, dim, SDF, slots)
    try:
        sa, sb = make_stream("room", W, H, dim, holes=False), make_stream("room", W, H, dim, holes=False)
        for f in range(at + 1):
            frame(a, sa, f)
            sb.depth(f)                                        # (the streams hand out frames in order)
        assert a.frame_is_fused()
        before = a.launch_counts()
        counts = a.shift(s)
        after = a.launch_counts()
        a.shift((0, 0, 0))
        # the held-back raycast of frame 5 ran on its own, before the shift, and nothing was launched for the second call
        assert before["pending"] and not after["pending"]
        assert after["raycast"] == before["raycast"] + 1 and after["fused"] == before["fused"]
        assert all(after[k] == before[k] or k == "alloc_commit" for k in after if k not in ("raycast", "pending"))
        assert a.launch_counts() == after
        assert counts.tolist() == want_c.tolist() and counts[0] > 0 and counts[1] > 0
        assert equal_blocks_nodes(*_state(a), want_b, want_n) is None
        b.load(path)
        for f in range(at + 1, frames):
            frame(a, sa, f)
            frame(b, sb, f)
        a.sync(); b.sync()
        assert a.launch_counts()["fused"] > after["fused"]     # the frames after the shift ran on the fused schedule
        out_a, out_b = ring_a.cpu().numpy(), ring_b.cpu().numpy()
        for f in range(3, at + 1):                             # up to the shift: the images of the undisturbed run
            assert (bits(out_a[f]) == bits(plain[f])).all(), f
        for f in range(at + 1, frames):
            assert bits(out_a[f]).any() and (bits(out_a[f]) == bits(out_b[f])).all(), f
        assert equal_blocks_nodes(*_state(a), *_state(b)) is None and a.counts() == b.counts()
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------ 3. integer queries move with the map
@pytest.mark.parametrize("field", [SDF, OFUSION], ids=["sdf", "ofusion"])
def test_integer_queries_move_with_the_map(field):
    """200 seeded boxes beside the surface whose neighbourhood (every voxel within r_max of the box) lies inside the kept region AND inside allocated
    blocks: there clearance and collides read voxels only, which the shift carries bit for bit, so the answers must move with the map.
    (Where a block is absent both kernels answer from the parent node's value_[child]; the shift drops the nodes it is not aligned to and
    recreates them with initValue() -- by its definition -- so such answers legitimately change: measured at 256^3 with s = (-48, 16, 0),
    15 of 200 unfiltered boxes answered differently with stop_at "unseen", each from a dropped node's value.)"""
    n, s = 256, np.array([-48, 16, 0])
    p = run_stream("room", field, n, 2.4, 0, FRAMES)
    try:
        rng = np.random.default_rng(7)
        coords = p.blocks()[0]
        alloc = np.zeros((n // 8,) * 3, bool)
        alloc[tuple((coords // 8).T)] = True
        v, nrm = p.vertex_normal()
        hit = (v[nrm[..., 0] != -2] * np.float32(n / 2.4)).astype(np.int64)
        k = 6000
        side = rng.integers(1, 7, (k, 3))
        r_max = rng.integers(0, 5, k)
        lo = hit[rng.choice(len(hit), k)] + rng.integers(-8, 3, (k, 3))
        lo_ok, hi_ok = np.maximum(0, -s), np.minimum(n, n - s)                          # the kept region
        # a voxel c is within r_max of the box [lo, lo + side) when its gap max(c - (lo + side), lo - c - 1, 0) is: touching counts as 0, so the
        # neighbourhood reaches one voxel further than r_max on either side
        a0, a1 = lo - r_max[:, None] - 1, lo + side + r_max[:, None] + 1
        ok = (a0 >= lo_ok).all(1) & (a1 <= hi_ok).all(1)
        for i in np.nonzero(ok)[0]:
            b0, b1 = a0[i] // 8, (a1[i] - 1) // 8 + 1
            ok[i] = alloc[b0[0]:b1[0], b0[1]:b1[1], b0[2]:b1[2]].all()
        pick = np.nonzero(ok)[0][:200]
        assert len(pick) == 200
        boxes = np.concatenate([lo[pick], side[pick]], 1).astype(np.int32)
        r_max = r_max[pick].astype(np.int32)
        moved = boxes.copy(); moved[:, :3] += s.astype(np.int32)
        before = {st: p.clearance(boxes, r_max, stop_at=st) for st in ("occupied", "unseen")}
        hits = p.collides(boxes, mode="strict")
        d2 = before["occupied"][0]
        print("classes", np.bincount(hits, minlength=3).tolist(), "d2 < 0 / == 0 / > 0", int((d2 < 0).sum()), int((d2 == 0).sum()), int((d2 > 0).sum()))
        assert len(np.unique(hits)) >= 2 and (d2 > 0).sum() > 10 and (d2 == 0).sum() > 10
        p.shift(s)
        for st, (d2, near) in before.items():
            d2b, nearb = p.clearance(moved, r_max, stop_at=st)
            assert (d2b == d2).all(), st
            found = d2 >= 0
            assert (nearb[found] == near[found] + s.astype(np.int32)).all() and (nearb[~found] == near[~found]).all(), st
        assert (p.collides(moved, mode="strict") == hits).all()
        # the vacated side (x >= n - 48 here, y < 16) is unseen
        vac = np.array([[n - 40, 100, 100, 30, 30, 30], [n - 48, 0, 0, 48, n, n], [0, 0, 0, n, 16, n], [100, 3, 100, 20, 10, 20]], np.int32)
        assert (p.collides(vac, mode="strict") == COLLISION_UNSEEN).all()
        assert (p.clearance(vac[[0, 3]], 0, stop_at="unseen", nearest=False) == 0).all()
    finally:
        p.close()


# ------------------------------------------------------------------ 4. the pool invariants
@pytest.mark.parametrize("field,pooled", TWINS, ids=[_name(f, 128, m) for f, m in TWINS])
def test_pool_invariants(field, pooled):
    n = 128
    cells, nodes = (n // 8) ** 3, sum(8 ** l for l in range(0, 4))
    p = run_stream("room", field, n, _dim(n), cells if pooled else 0, FRAMES)
    fresh = DenseSLAMPipeline((W, H), n, _dim(n), field_type=field, max_blocks=cells if pooled else 0)
    try:
        ix, iy = (np.float32(v) for v in INIT[field])
        coords = p.blocks()[0]
        c = _shift_and_check(p, (16, -24, 0), field)
        assert p.counts()[0] == c[0] and c[1] > 0
        if not pooled:
            # the bricks of dropped blocks (they left through a face: their old places) and of the vacated side read initValue()
            kept = set(map(tuple, p.blocks()[0].tolist()))
            old = [tuple(v) for v in coords.tolist() if tuple(v) not in kept][:300]
            assert len(old) > 10
            pts = (np.array(old, np.float32) + 3.5) * np.float32(_dim(n) / n)
            vac = (np.array([[3, 50, 50], [12, 5, 100], [60, n - 20, 60], [100, n - 3, 7]], np.float32) + 0.5) * np.float32(_dim(n) / n)
            q = p.query(np.concatenate([pts, vac]).astype(np.float32), fine=True, coarse=False, interp=False, grad=False, status=True)
            assert (q["fine"][:, 0] == ix).all() and (q["fine"][:, 1] == iy).all() and (q["status"] & 2 == 0).all()
        c = _shift_and_check(p, (n, 0, 0), field)
        assert c[0] == 0 and p.counts() == (0, 1)
        assert _same(map_state(p)[:8], map_state(fresh)[:8])
        # every slot of both pools holds initValue(): the whole volume allocated, counted by an edit that assigns nothing
        whole = np.array([[0, 0, 0, n, n, n]], np.int32)
        assert p.allocate(whole).tolist() == [cells, nodes - 1, cells, 0]
        assert p.edit(whole, only="unseen", mode="strict").tolist() == [512 * cells, 8 * nodes, cells, 0]
    finally:
        p.close(); fresh.close()


# ------------------------------------------------------------------ 5. the contract
def test_invalid_shifts_are_refused_and_change_nothing():
    p = run_stream("room", SDF, 128, _dim(128), 0, 4)
    try:
        before = map_state(p)
        out = np.full(4, 77, np.int64)
        for s in [(4, 0, 0), (0, -12, 0), (8, 8, 7), (0, 0, LIMIT + 8), (-LIMIT - 8, 0, 0), (2 ** 31 - 8, 0, 0)]:
            a = np.array(s, np.int32)
            assert p.lib.se_hip_shift_map(p._h, a.ctypes.data, out.ctypes.data) == -1
            assert "se_hip_shift_map" in p.lib.se_hip_last_error().decode()
        assert p.lib.se_hip_shift_map(p._h, None, out.ctypes.data) == -1
        assert (out == 77).all() and _same(before, map_state(p))
        assert p.lib.se_hip_shift_map(p._h, np.array([8, 0, 0], np.int32).ctypes.data, None) == 0      # counts are optional
    finally:
        p.close()


def test_tracking_waits_for_a_raycast_after_a_shift():
    n, dim, mu = 256, 2.4, 0.1
    s = make_stream("room", W, H, dim, holes=False)
    p = run_stream("room", SDF, n, dim, 0, 5)
    try:
        for f in range(5):
            s.depth(f)
        p.set_depth(s.depth(5)); p.setPose(s.pose(5))
        assert p.tracking(s.k, 1e-5, 1, 5)
        p.shift((0, 0, 0))
        assert p.tracking(s.k, 1e-5, 1, 5)                     # s = 0 moves nothing
        p.shift((-32, 0, 0))
        pose = p.pose_.copy()
        with pytest.raises(SeHipError, match="vertex / normal images predate a map shift"):
            p.tracking(s.k, 1e-5, 1, 5)
        with pytest.raises(SeHipError, match="vertex / normal images predate a map shift"):
            p.frame_tracked(0, s.k, mu, 5)
        assert (p.pose_ == pose).all()
        assert p.raycasting(s.k, mu, 5)
        assert p.tracking(s.k, 1e-5, 1, 5)
        assert np.isfinite(p.pose_).all()
    finally:
        p.close()


def test_twenty_shifts_on_a_nearly_full_pool():
    n = 128
    probe = run_stream("room", SDF, n, _dim(n), (n // 8) ** 3, FRAMES)
    nb = probe.counts()[0]
    probe.close()
    p = run_stream("room", SDF, n, _dim(n), nb + 8, FRAMES)
    try:
        assert p.counts()[0] == nb and p.memory_info()["brick_slots"] == nb + 8
        state = _state(p)
        for i in range(20):
            s = [(8, 0, 0), (-8, 0, 0), (0, 16, -8), (0, -16, 8)][i % 4]
            want_b, want_n, want_c = shift_truth(n, s, state[0], state[1], INIT[SDF])
            assert p.shift(s).tolist() == want_c.tolist()          # (SeHipError on SE_HIP_E_CAPACITY)
            state = _state(p)
            assert equal_blocks_nodes(state[0], state[1], want_b, want_n) is None, i
            assert p.counts()[0] == len(want_b[0]) <= nb
        assert 0 < p.counts()[0] < nb
        assert p.clear_overflow() == 0
    finally:
        p.close()
