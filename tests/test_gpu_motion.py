"""Motion collision queries on the device (se_hip_collide_motions / DenseSLAMPipeline.collides_moving): the hand-worked cases on maps built
without depth (dense and pooled, both fields); status and the bits of t_first against the definition evaluated in numpy over a dense class
grid (room SDF and stress OFusion, dense and pooled); the identities that tie a motion to the strict box query; 2^18 motions in one batch;
invalid motions and the threshold direction; and the schedule (streaming handle, the map, the images and the launch counters left alone)."""
import ctypes as C

import numpy as np
import pytest

from supereight_amd.pipeline import (COLLISION_EMPTY, COLLISION_INVALID, COLLISION_OCCUPIED, COLLISION_UNSEEN, MOTION_FREE, OFUSION, SDF,
                                     DenseSLAMPipeline, _CollideTest, _MotionOut)
from tests.gpu_state_util import H, W, bits, map_state, run_stream, streamed_with
from tests.motion_util import (FREE, HAND_CASES, HAND_MAPS, INVALID_T, LIMIT, as_float32, boxes_of, check_identities, class_grid,
                               motion_truth, stamp_hand_map)

pytestmark = pytest.mark.gpu


def _expected_float(fr):
    return np.float32(MOTION_FREE) if fr == FREE else (np.float32(-1.0) if fr == INVALID_T else as_float32(fr))


@pytest.mark.parametrize("field", [SDF, OFUSION], ids=["sdf", "ofusion"])
@pytest.mark.parametrize("max_blocks", [0, 1024], ids=["dense", "pooled"])
def test_hand_cases_on_the_device(field, max_blocks):
    occupied_x, empty_x = (-0.5, 0.5) if field == SDF else (2.0, -2.0)
    p = DenseSLAMPipeline((W, H), 64, 1.28, field_type=field, max_blocks=max_blocks)
    try:
        for mp, spec in HAND_MAPS.items():
            stamp_hand_map(p, spec, occupied_x, empty_x)
            names = [k for k, c in HAND_CASES.items() if c[0] == mp]
            motions = np.array([list(HAND_CASES[k][1]) + list(HAND_CASES[k][2]) + list(HAND_CASES[k][3]) for k in names], np.int32)
            for stop, col in (("occupied", 4), ("unseen", 5)):
                st, t = p.collides_moving(motions, stop_at=stop)
                alone = p.collides_moving(motions, stop_at=stop, t_first=False)
                for i, k in enumerate(names):
                    e_st, e_t = HAND_CASES[k][col]
                    assert int(st[i]) == e_st and int(alone[i]) == e_st, (k, stop, st[i], alone[i])
                    assert bits(t[i:i + 1])[0] == bits(np.array([_expected_float(e_t)]))[0], (k, stop, t[i], e_t)
    finally:
        p.close()


def _hits(p, n, dim):
    v, nrm = p.vertex_normal()
    hits = v[nrm[..., 0] != -2].reshape(-1, 3)
    assert len(hits) > 100
    return (hits * (n / dim)).astype(np.int64)


def _motions(p, n, dim, rng, k=1100, max_side=8, max_d=32):
    """k random motions (sides 1..max_side, |d_k| <= max_d, starts in [-20, n + 8], a third centred on raycast hits), then d = 0, axis-aligned
    moves, the four diagonals of the volume and motions entirely outside."""
    side = rng.integers(1, max_side + 1, (k, 3))
    lo = rng.integers(-20, n + 9, (k, 3))
    d = rng.integers(-max_d, max_d + 1, (k, 3))
    hv = _hits(p, n, dim)
    third = k // 3
    lo[:third] = hv[rng.choice(len(hv), third)] - side[:third] // 2 - d[:third] // 2     # the surface near the middle of the motion
    sets = [np.concatenate([lo, side, d], 1)]
    q = k // 8
    still = np.concatenate([hv[rng.choice(len(hv), q)] - 2 + rng.integers(-6, 7, (q, 3)), rng.integers(1, max_side + 1, (q, 3)), np.zeros((q, 3), np.int64)], 1)
    sets.append(still)
    axis = np.concatenate([rng.integers(-20, n + 9, (2 * q, 3)), rng.integers(1, max_side + 1, (2 * q, 3)), np.zeros((2 * q, 3), np.int64)], 1)
    axis[np.arange(2 * q), 6 + rng.integers(0, 3, 2 * q)] = rng.integers(-max_d, max_d + 1, 2 * q)
    axis[:q, 0:3] = hv[rng.choice(len(hv), q)] - 3
    sets.append(axis)
    e = n - 2
    sets.append(np.array([[0, 0, 0, 2, 2, 2, e, e, e], [e, 0, 0, 2, 2, 2, -e, e, e], [0, e, 0, 2, 2, 2, e, -e, e], [e, e, 0, 2, 2, 2, -e, -e, e]]))
    sets.append(np.array([[-30, -30, -30, 4, 4, 4, 10, 5, -3], [n + 3, 5, 5, 2, 2, 2, 20, 1, 0], [5, -9, 5, 3, 3, 3, 9, 0, 30], [n, n, n, 1, 1, 1, 0, 0, 0]]))
    return np.ascontiguousarray(np.concatenate(sets).astype(np.int32))


BRUTE = [("room", SDF, 0), ("room", SDF, 2048), ("stress", OFUSION, 0), ("stress", OFUSION, 2048)]


@pytest.mark.parametrize("kind,field,max_blocks", BRUTE, ids=[f"{k}_{'sdf' if f == SDF else 'ofusion'}_{'dense' if m == 0 else 'pooled'}" for k, f, m in BRUTE])
def test_status_and_t_first_equal_the_definition(kind, field, max_blocks):
    n, dim = 128, 2.4
    rng = np.random.default_rng(n + field + max_blocks)
    p = run_stream(kind, field, n, dim, max_blocks, 4)
    try:
        grid = class_grid(p, n, dim, 0.0, field == OFUSION).cpu().numpy()
        motions = _motions(p, n, dim, rng)
        assert len(motions) >= 1500
        truth = [motion_truth(grid, m) for m in motions.tolist()]
        seen_status, seen_t = set(), set()
        for stop, col in (("occupied", 1), ("unseen", 2)):
            st, t = p.collides_moving(motions, stop_at=stop)
            alone = p.collides_moving(motions, stop_at=stop, t_first=False)
            exp_st = np.array([r[0] for r in truth], np.uint8)
            exp_t = np.array([_expected_float(r[col]) for r in truth], np.float32)
            bad = np.nonzero((st != exp_st) | (alone != exp_st) | (bits(t) != bits(exp_t)))[0]
            assert bad.size == 0, (stop, bad[:5], motions[bad[:5]], st[bad[:5]], exp_st[bad[:5]], t[bad[:5]], exp_t[bad[:5]])
            seen_status.update(np.unique(st).tolist())
            seen_t.update(np.where(t == 0, 0, np.where(t < 1, 1, 2)).tolist())
            assert ((t > 0) & (t < 1)).sum() > 20
        assert {COLLISION_OCCUPIED, COLLISION_UNSEEN, COLLISION_EMPTY} <= seen_status
        assert seen_t == {0, 1, 2}                                   # blocked at the start, part of the way, free
    finally:
        p.close()


@pytest.mark.parametrize("field,max_blocks", [(SDF, 8192), (OFUSION, 0)], ids=["sdf_pooled", "ofusion_dense"])
def test_identities_against_the_strict_box_query(field, max_blocks):
    n, dim = 256, 4.8
    p = run_stream("stress", field, n, dim, max_blocks, 4)
    try:
        motions = _motions(p, n, dim, np.random.default_rng(17 + field), k=1500, max_side=12, max_d=48)
        assert len(motions) >= 2000
        st, t = p.collides_moving(motions)
        still, axis, general = check_identities(p, motions, st)
        assert still > 100 and axis > 200 and general > 1000
        assert {COLLISION_OCCUPIED, COLLISION_UNSEEN, COLLISION_EMPTY} <= set(np.unique(st).tolist())
        # t_first is consistent with the status and with the start box
        start = p.collides(boxes_of(motions)[0])
        assert (t[start == COLLISION_OCCUPIED] == 0).all() and (t[start != COLLISION_OCCUPIED] >= 0).all()
        assert ((t < 1.5) == (st == COLLISION_OCCUPIED)).all()
    finally:
        p.close()


def test_quarter_million_motions_at_512():
    import torch
    n, dim = 512, 4.8
    p = run_stream("room", SDF, n, dim, 0, 3)
    try:
        rng = np.random.default_rng(8)
        m = 1 << 18
        motions = np.concatenate([rng.integers(-16, n + 8, (m, 3)), rng.integers(1, 9, (m, 3)), rng.integers(-32, 33, (m, 3))], 1)
        hv = _hits(p, n, dim)
        k = m // 4
        motions[:k, 0:3] = hv[rng.choice(len(hv), k)] - 4 - motions[:k, 6:9] // 2
        motions[k:2 * k, 6:8] = 0                                     # axis-aligned along z, some of them still
        motions[k:k + k // 4, 8] = 0
        motions = np.ascontiguousarray(motions.astype(np.int32))
        st, t = p.collides_moving(motions)
        still, axis, general = check_identities(p, motions, st)
        assert still > 1000 and axis > 10000 and general > 100000
        assert (st == COLLISION_OCCUPIED).any() and (st == COLLISION_EMPTY).any() and (st == COLLISION_UNSEEN).any()
        dst, dt = p.collides_moving(torch.from_numpy(motions).to("cuda:0"))
        assert isinstance(dst, torch.Tensor) and dst.dtype == torch.uint8 and dt.dtype == torch.float32 and dt.device.type == "cuda"
        assert (dst.cpu().numpy() == st).all() and (bits(dt.cpu().numpy()) == bits(t)).all()
        for stop in ("occupied", "unseen"):
            alone = p.collides_moving(torch.from_numpy(motions).to("cuda:0"), stop_at=stop, t_first=False)
            assert (alone.cpu().numpy() == st).all()
        empty = p.collides_moving(np.zeros((0, 9), np.int32))
        assert empty[0].shape == (0,) and empty[0].dtype == np.uint8 and empty[1].dtype == np.float32
        assert p.collides_moving(torch.zeros((0, 9), dtype=torch.int32, device="cuda:0"), t_first=False).shape == (0,)
    finally:
        p.close()


@pytest.mark.parametrize("field,max_blocks", [(SDF, 0), (OFUSION, 4096)], ids=["sdf_dense", "ofusion_pooled"])
def test_invalid_motions_and_threshold_direction(field, max_blocks):
    p = run_stream("room", field, 256, 2.4, max_blocks, 2)
    try:
        L = LIMIT
        bad = np.array([[0, 0, 0, 0, 1, 1, 1, 1, 1], [0, 0, 0, 1, -3, 1, 0, 0, 0], [0, 0, 0, 1, 1, -(1 << 31), 0, 0, 0], [-L - 1, 0, 0, 1, 1, 1, 5, 0, 0],
                        [0, L, 0, 1, 1, 1, 0, 0, 0], [0, 0, L - 4, 5, 5, 5, 0, 0, 0], [0, 0, 0, 1, 1, 1, L, 0, 0], [0, 0, 0, 1, 1, 1, 0, -L - 1, 0],
                        [0, 0, 0, 1, 1, 1, 0, 0, 2 ** 31 - 1], [0, 0, 0, 1, 1, 1, -(1 << 31), 0, 0], [2 ** 31 - 1, 0, 0, 2 ** 31 - 1, 1, 1, 2 ** 31 - 1, 0, 0]], np.int32)
        edge = np.array([[-L, 0, 0, 1, 1, 1, 0, 0, 0], [0, 0, L - 1, 1, 1, 1, 0, 0, -7], [-L, -L, -L, L, L, L, 0, 0, 0], [L - 1, 0, 0, 1, 1, 1, -2 * L + 1, 0, 0],
                         [0, 0, 0, 1, 1, 1, L - 1, L - 1, -L]], np.int32)
        for stop in ("occupied", "unseen"):
            st, t = p.collides_moving(bad, stop_at=stop)
            assert (st == COLLISION_INVALID).all() and (t == -1.0).all()
            st, t = p.collides_moving(edge, stop_at=stop)
            assert (st != COLLISION_INVALID).all() and (t >= 0).all()
            assert (st[:3] == COLLISION_UNSEEN).all()                  # valid, wholly outside
        rng = np.random.default_rng(3)
        motions = np.ascontiguousarray(np.concatenate([rng.integers(0, 240, (3000, 3)), rng.integers(1, 9, (3000, 3)), rng.integers(-24, 25, (3000, 3))], 1).astype(np.int32))
        default, t_default = p.collides_moving(motions)
        above = field == OFUSION
        same, t_same = p.collides_moving(motions, occupied_above=above)
        assert (default == same).all() and (bits(t_default) == bits(t_same)).all()
        flipped, _ = p.collides_moving(motions, occupied_above=not above)
        assert (default == COLLISION_OCCUPIED).any() and (flipped != default).any()
        # unseen does not depend on the threshold
        assert ((default == COLLISION_UNSEEN) == (flipped == COLLISION_UNSEEN)).sum() > 0
        # stop_at unseen can only stop earlier
        _, t_unseen = p.collides_moving(motions, stop_at="unseen")
        assert (t_unseen <= t_default).all() and (t_unseen < t_default).any()
    finally:
        p.close()


def _launches(p):
    return {k: d["launches"] for k, d in p.timings().items()}


@pytest.mark.parametrize("field", [SDF, OFUSION], ids=["sdf", "ofusion"])
def test_motions_see_the_map_of_the_frames_before_them(field):
    """On a streaming handle (scans on the side stream, raycasts held back) the answer after frame f equals the synchronous handle's; the
    calls change neither the map, the images nor the launch counters."""
    rng = np.random.default_rng(21)
    motions = np.ascontiguousarray(np.concatenate([rng.integers(-8, 250, (4000, 3)), rng.integers(1, 9, (4000, 3)), rng.integers(-32, 33, (4000, 3))], 1).astype(np.int32))
    ans = {True: [], False: []}

    def rec(streaming):
        def check(p, f):
            ans[streaming].append(p.collides_moving(motions) + p.collides_moving(motions, stop_at="unseen"))
        return check

    a = run_stream("room", field, 256, 2.4, 0, 4, streaming=True, check=rec(True))
    b = run_stream("room", field, 256, 2.4, 0, 4, streaming=False, check=rec(False))
    try:
        for u, w in zip(ans[True], ans[False]):
            assert all((bits(x) == bits(y)).all() if x.dtype == np.float32 else (x == y).all() for x, y in zip(u, w))
        assert any((u[0] != w[0]).any() for u, w in zip(ans[False], ans[False][1:]))       # the answers follow the map
        a.enable_timing(True)
        before, la = map_state(a), _launches(a)
        for _ in range(3):
            a.collides_moving(motions)
            a.collides_moving(motions, stop_at="unseen", t_first=False)
        after, lb = map_state(a), _launches(a)
        assert la == lb
        assert all((u == w).all() for u, w in zip(before, after))
    finally:
        a.close(); b.close()


def test_motions_between_frames_of_a_streaming_handle():
    """With frame 5's raycast held back on a streaming handle, the call flushes that raycast as a launch of its own, answers for the map with
    frame 5 fused, moves no other counter, and the image ring ends up as if the call had not been made."""
    f = 5
    rng = np.random.default_rng(5)
    motions = np.ascontiguousarray(np.concatenate([rng.integers(0, 250, (2000, 3)), rng.integers(1, 9, (2000, 3)), rng.integers(-32, 33, (2000, 3))], 1).astype(np.int32))
    got = {}

    def action(p, box):
        got["streamed"] = p.collides_moving(motions)

    ring, log = streamed_with(action, f)
    twin, _ = streamed_with(action, -1)
    assert log["fused"]
    assert (bits(ring) == bits(twin)).all()
    b, a, again = log["before"], log["after"], log["again"]
    assert b["pending"] and not a["pending"]
    assert a["raycast"] == b["raycast"] + 1 and a["fused"] == b["fused"]   # launched alone, not with a scan
    assert all(a[k] == b[k] for k in a if k not in ("raycast", "pending"))
    assert again == a
    ref = run_stream("room", SDF, 256, 2.4, 0, f + 1)
    try:
        st, t = ref.collides_moving(motions)
        assert (st == got["streamed"][0]).all() and (bits(t) == bits(got["streamed"][1])).all()
        assert (st == COLLISION_OCCUPIED).any()
    finally:
        ref.close()


def test_motion_entries_refuse_bad_arguments():
    import torch
    p = run_stream("room", SDF, 256, 2.4, 0, 1)
    try:
        lib = p.lib
        motions = np.zeros((4, 9), np.int32)
        st, tf = np.zeros(4, np.uint8), np.zeros(4, np.float32)
        dmo = torch.zeros((4, 9), dtype=torch.int32, device="cuda:0")
        dst, dtf = torch.zeros(4, dtype=torch.uint8, device="cuda:0"), torch.zeros(4, dtype=torch.float32, device="cuda:0")
        good = _CollideTest(0.0, 0)
        for fn, ma, out, no_status in ((lib.se_hip_collide_motions_host, motions.ctypes.data, _MotionOut(st.ctypes.data, tf.ctypes.data), _MotionOut(None, tf.ctypes.data)),
                                       (lib.se_hip_collide_motions, dmo.data_ptr(), _MotionOut(dst.data_ptr(), dtf.data_ptr()), _MotionOut(None, dtf.data_ptr()))):
            o = C.byref(out)
            for args in ((ma, -1, C.byref(good), 0, o), (None, 4, C.byref(good), 0, o), (ma, 4, C.byref(good), 0, C.byref(no_status)), (ma, 4, C.byref(good), 0, None),
                         (ma, 4, None, 0, o), (ma, 4, C.byref(_CollideTest(float("nan"), 0)), 0, o), (ma, 4, C.byref(_CollideTest(float("inf"), 0)), 0, o),
                         (ma, 4, C.byref(_CollideTest(0.0, 2)), 0, o), (ma, 4, C.byref(good), 2, o), (ma, 4, C.byref(good), -1, o), (ma, 4, C.byref(good), 255, o)):
                assert fn(p._h, *args) == -1
            assert fn(p._h, None, 0, C.byref(good), 0, C.byref(_MotionOut(None, None))) == 0
            assert fn(p._h, ma, 4, C.byref(good), 1, C.byref(_MotionOut(out.status, None))) == 0       # t_first not wanted
        p.sync()
    finally:
        p.close()
