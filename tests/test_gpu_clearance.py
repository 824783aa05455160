"""Clearance queries on the device (se_hip_clearance_boxes / DenseSLAMPipeline.clearance): the hand-worked cases on maps built without depth
(dense and pooled, both fields); d2 and the nearest voxel against the definition evaluated in numpy over a dense class grid (room SDF and
stress OFusion, dense and pooled); the identities that tie a clearance to the strict box query; 2^18 queries in one batch; invalid queries
and the threshold direction; and the schedule (streaming handle, the map, the images and the launch counters left alone).  Everything is
integer: every comparison is equality."""
import ctypes as C

import numpy as np
import pytest

from supereight_amd.pipeline import CLEARANCE_INVALID, CLEARANCE_NONE, OFUSION, SDF, DenseSLAMPipeline, _ClearanceOut, _CollideTest
from tests.clearance_util import (CLEAR_MAPS, HAND_CASES, I32_MIN, LIMIT, OCC, R_MAX, UNSEEN, check_identities, clearance_truth,
                                  stamp_clear_map)
from tests.gpu_state_util import H, W, bits, map_state, run_stream, streamed_with
from tests.motion_util import class_grid

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("field", [SDF, OFUSION], ids=["sdf", "ofusion"])
@pytest.mark.parametrize("max_blocks", [0, 1024], ids=["dense", "pooled"])
def test_hand_cases_on_the_device(field, max_blocks):
    occupied_x, empty_x = (-0.5, 0.5) if field == SDF else (2.0, -2.0)
    for mp in CLEAR_MAPS:
        p = DenseSLAMPipeline((W, H), 64, 1.28, field_type=field, max_blocks=max_blocks)
        try:
            stamp_clear_map(p, mp, occupied_x, empty_x)
            names = [k for k, c in HAND_CASES.items() if c[0] == mp]
            boxes = np.array([list(HAND_CASES[k][1]) + list(HAND_CASES[k][2]) for k in names], np.int32)
            r_max = np.array([HAND_CASES[k][3] for k in names], np.int64)
            for stop, col in (("occupied", 4), ("unseen", 5)):
                d2, near = p.clearance(boxes, r_max, stop_at=stop)
                alone = p.clearance(boxes, r_max, stop_at=stop, nearest=False)
                for i, k in enumerate(names):
                    e_d2, e_near = HAND_CASES[k][col]
                    assert int(d2[i]) == e_d2 and int(alone[i]) == e_d2, (k, stop, d2[i], alone[i])
                    assert tuple(near[i].tolist()) == e_near, (k, stop, near[i])
        finally:
            p.close()


def _hits(p, n, dim):
    v, nrm = p.vertex_normal()
    hits = v[nrm[..., 0] != -2].reshape(-1, 3)
    assert len(hits) > 100
    return (hits * (n / dim)).astype(np.int64)


def _queries(p, n, dim, rng, k, max_side=8, max_r=16):
    """k random queries (sides 1..max_side, r_max 0..max_r, starts in [-20, n + 8], a third centred within +-6 of raycast hits), then queries
    with r_max = 0, queries wholly outside the volume and the whole volume.  Returns boxes [N, 6] and r_max [N]."""
    side = rng.integers(1, max_side + 1, (k, 3))
    lo = rng.integers(-20, n + 9, (k, 3))
    r = rng.integers(0, max_r + 1, k)
    hv = _hits(p, n, dim)
    third = k // 3
    lo[:third] = hv[rng.choice(len(hv), third)] - side[:third] // 2 + rng.integers(-6, 7, (third, 3))
    r[third // 2:third // 2 + k // 16] = 0                                  # touching or nothing, near the surfaces and away from them
    r[third:third + k // 16] = 0
    sets = [np.concatenate([lo, side, r[:, None]], 1)]
    sets.append(np.array([[-30, -30, -30, 4, 4, 4, 16], [-30, 5, 5, 4, 4, 4, 30], [n + 3, 5, 5, 2, 2, 2, 2], [n + 3, 5, 5, 2, 2, 2, 3], [5, -9, 5, 3, 3, 3, 6],
                          [n, n, n, 1, 1, 1, 0], [5, 5, n + 12, 2, 2, 2, 11], [5, 5, n + 12, 2, 2, 2, 12], [-1, -1, -1, 1, 1, 1, 0], [0, 0, 0, n, n, n, 0],
                          [0, 0, 0, n, n, n, 3]]))
    q = np.concatenate(sets)
    return np.ascontiguousarray(q[:, :6].astype(np.int32)), np.ascontiguousarray(q[:, 6].astype(np.int32))


BRUTE = [("room", SDF, 0), ("room", SDF, 2048), ("stress", OFUSION, 0), ("stress", OFUSION, 2048)]


@pytest.mark.parametrize("kind,field,max_blocks", BRUTE, ids=[f"{k}_{'sdf' if f == SDF else 'ofusion'}_{'dense' if m == 0 else 'pooled'}" for k, f, m in BRUTE])
def test_d2_and_nearest_equal_the_definition(kind, field, max_blocks):
    n, dim = 128, 2.4
    rng = np.random.default_rng(n + field + max_blocks)
    p = run_stream(kind, field, n, dim, max_blocks, 4)
    try:
        grid = class_grid(p, n, dim, 0.0, field == OFUSION).cpu().numpy()
        boxes, r_max = _queries(p, n, dim, rng, 900)
        assert len(boxes) >= 800
        q = np.concatenate([boxes, r_max[:, None]], 1).tolist()
        seen = {"touching": 0, "apart": 0, "none": 0, "outside": 0, "ties": 0}
        for stop, code in (("occupied", OCC), ("unseen", UNSEEN)):
            truth = [clearance_truth(grid, row, code) for row in q]
            exp_d2 = np.array([t[0] for t in truth], np.int32)
            exp_near = np.array([t[1] for t in truth], np.int32)
            d2, near = p.clearance(boxes, r_max, stop_at=stop)
            alone = p.clearance(boxes, r_max, stop_at=stop, nearest=False)
            bad = np.nonzero((d2 != exp_d2) | (alone != exp_d2) | (near != exp_near).any(1))[0]
            assert bad.size == 0, (stop, bad[:5], boxes[bad[:5]], r_max[bad[:5]], d2[bad[:5]], exp_d2[bad[:5]], near[bad[:5]], exp_near[bad[:5]])
            seen["touching"] += int((d2 == 0).sum())
            seen["apart"] += int((d2 > 0).sum())
            seen["none"] += int((d2 == CLEARANCE_NONE).sum())
            seen["outside"] += int(((d2 >= 0) & ((near < 0) | (near >= n)).any(1)).sum())
            seen["ties"] += sum(1 for t in truth if t[2] > 1)
        print(seen)
        assert seen["touching"] > 0 and seen["apart"] > 0 and seen["none"] > 0 and seen["outside"] > 0
        assert seen["ties"] >= 20                                     # the truth found more than one minimiser: the tie-break decided
    finally:
        p.close()


@pytest.mark.parametrize("field,max_blocks", [(SDF, 8192), (OFUSION, 0)], ids=["sdf_pooled", "ofusion_dense"])
def test_identities_against_the_strict_box_query(field, max_blocks):
    n, dim = 256, 4.8
    p = run_stream("stress", field, n, dim, max_blocks, 4)
    try:
        rng = np.random.default_rng(17 + field)
        boxes, r_max = _queries(p, n, dim, rng, 2100, max_r=24)
        assert len(boxes) >= 2000
        out = check_identities(p, boxes, r_max, rng)
        d2 = out["occupied"][0]
        assert (d2 == 0).any() and (d2 > 0).any() and (d2 == CLEARANCE_NONE).any()
        assert (out["unseen"][0] != d2).any()
    finally:
        p.close()


def test_quarter_million_queries_at_512():
    import torch
    n, dim = 512, 2.4
    p = run_stream("room", SDF, n, dim, 0, 3)
    try:
        rng = np.random.default_rng(8)
        m = 1 << 18
        boxes = np.concatenate([rng.integers(-16, n + 8, (m, 3)), rng.integers(1, 9, (m, 3))], 1)
        hv = _hits(p, n, dim)
        k = m // 2
        boxes[:k, 0:3] = hv[rng.choice(len(hv), k)] - 4 + rng.integers(-10, 11, (k, 3))
        boxes = np.ascontiguousarray(boxes.astype(np.int32))
        r_max = rng.integers(0, 13, m).astype(np.int32)
        out = check_identities(p, boxes, r_max, rng)
        d2, near = out["occupied"]
        assert (d2 == 0).sum() > 1000 and (d2 > 0).sum() > 1000 and (d2 == CLEARANCE_NONE).sum() > 1000
        dev = torch.from_numpy(boxes).to("cuda:0")
        for stop in ("occupied", "unseen"):
            for r in (torch.from_numpy(r_max).to("cuda:0"), r_max):                  # r_max on the device, and as a host array beside device boxes
                dd, dn = p.clearance(dev, r, stop_at=stop)
                assert isinstance(dd, torch.Tensor) and dd.dtype == torch.int32 and dn.dtype == torch.int32 and dn.device.type == "cuda" and tuple(dn.shape) == (m, 3)
                assert (dd.cpu().numpy() == out[stop][0]).all() and (dn.cpu().numpy() == out[stop][1]).all()
            alone = p.clearance(dev, torch.from_numpy(r_max).to("cuda:0"), stop_at=stop, nearest=False)
            assert (alone.cpu().numpy() == out[stop][0]).all()
        scalar = p.clearance(dev[:1000], 7, nearest=False)
        assert (scalar.cpu().numpy() == p.clearance(boxes[:1000], np.full(1000, 7), nearest=False)).all()
        empty = p.clearance(np.zeros((0, 6), np.int32), 5)
        assert empty[0].shape == (0,) and empty[0].dtype == np.int32 and empty[1].shape == (0, 3) and empty[1].dtype == np.int32
        assert p.clearance(np.zeros((0, 6), np.int32), np.zeros(0, np.int64), nearest=False).shape == (0,)
        e = p.clearance(torch.zeros((0, 6), dtype=torch.int32, device="cuda:0"), 5)
        assert e[0].shape == (0,) and e[0].dtype == torch.int32 and tuple(e[1].shape) == (0, 3) and e[1].dtype == torch.int32
    finally:
        p.close()


@pytest.mark.parametrize("field,max_blocks", [(SDF, 0), (OFUSION, 4096)], ids=["sdf_dense", "ofusion_pooled"])
def test_invalid_queries_and_threshold_direction(field, max_blocks):
    p = run_stream("room", field, 256, 2.4, max_blocks, 2)
    try:
        L = LIMIT
        bad = np.array([[0, 0, 0, 0, 1, 1, 4], [0, 0, 0, 1, -3, 1, 4], [0, 0, 0, 1, 1, -(1 << 31), 4], [-L - 1, 0, 0, 1, 1, 1, 4], [0, L, 0, 1, 1, 1, 4],
                        [0, 0, L - 4, 5, 5, 5, 4], [0, 0, 0, 1, 1, 1, R_MAX + 1], [0, 0, 0, 1, 1, 1, -1], [2 ** 31 - 1, 0, 0, 2 ** 31 - 1, 1, 1, 4],
                        [-(1 << 31), 0, 0, 1, 1, 1, 4]], np.int64)
        edge = np.array([[-L, 0, 0, 1, 1, 1, 4], [0, 0, L - 1, 1, 1, 1, 4], [-L, -L, -L, 2 * L, 2 * L, 2 * L, 0], [100, 100, 100, 1, 1, 1, R_MAX], [0, 0, 0, 1, 1, 1, 0]], np.int64)
        for stop in ("occupied", "unseen"):
            d2, near = p.clearance(bad[:, :6].astype(np.int32), bad[:, 6], stop_at=stop)
            assert (d2 == CLEARANCE_INVALID).all() and (near == I32_MIN).all()
            assert (p.clearance(bad[:, :6].astype(np.int32), bad[:, 6], stop_at=stop, nearest=False) == CLEARANCE_INVALID).all()
            d2, near = p.clearance(edge[:, :6].astype(np.int32), edge[:, 6], stop_at=stop)
            assert (d2 != CLEARANCE_INVALID).all()
            if stop == "unseen":
                assert (d2[[0, 1, 2, 4]] == 0).all()                   # these touch the outside of the volume
        d2, near = p.clearance(edge[3:4, :6].astype(np.int32), R_MAX)          # the largest r_max: the surfaces of the room are found
        assert d2[0] >= 0 and (near[0] >= 0).all() and (near[0] < 256).all()
        rng = np.random.default_rng(3)
        boxes = np.ascontiguousarray(np.concatenate([rng.integers(0, 240, (3000, 3)), rng.integers(1, 9, (3000, 3))], 1).astype(np.int32))
        default, n_default = p.clearance(boxes, 12)
        above = field == OFUSION
        same, n_same = p.clearance(boxes, 12, occupied_above=above)
        assert (default == same).all() and (n_default == n_same).all()
        flipped, _ = p.clearance(boxes, 12, occupied_above=not above)
        assert (default >= 0).any() and (flipped != default).any()
        # unseen does not depend on the threshold direction: with everything seen counted as occupied either way, only unseen voxels differ
        lo_thr = p.clearance(boxes, 12, stop_at="unseen", threshold=-1e30, occupied_above=True, nearest=False)     # every seen voxel occupied
        hi_thr = p.clearance(boxes, 12, stop_at="unseen", threshold=1e30, occupied_above=False, nearest=False)     # the same, from the other side
        assert (lo_thr == hi_thr).all()
        # stop_at unseen can only bring the nearest blocking voxel closer
        unseen = p.clearance(boxes, 12, stop_at="unseen", nearest=False).astype(np.int64)
        big = np.int64(1) << 40
        d = default.astype(np.int64)
        assert (np.where(unseen < 0, big, unseen) <= np.where(d < 0, big, d)).all() and (unseen != d).any()
    finally:
        p.close()


def _launches(p):
    return {k: d["launches"] for k, d in p.timings().items()}


@pytest.mark.parametrize("field", [SDF, OFUSION], ids=["sdf", "ofusion"])
def test_clearance_sees_the_map_of_the_frames_before_it(field):
    """On a streaming handle (scans on the side stream, raycasts held back) the answer after frame f equals the synchronous handle's; the
    calls change neither the map, the images nor the launch counters."""
    rng = np.random.default_rng(21)
    boxes = np.ascontiguousarray(np.concatenate([rng.integers(-8, 250, (4000, 3)), rng.integers(1, 9, (4000, 3))], 1).astype(np.int32))
    r_max = rng.integers(0, 17, 4000)
    ans = {True: [], False: []}

    def rec(streaming):
        def check(p, f):
            ans[streaming].append(p.clearance(boxes, r_max) + p.clearance(boxes, r_max, stop_at="unseen"))
        return check

    a = run_stream("room", field, 256, 2.4, 0, 4, streaming=True, check=rec(True))
    b = run_stream("room", field, 256, 2.4, 0, 4, streaming=False, check=rec(False))
    try:
        for u, w in zip(ans[True], ans[False]):
            assert all((x == y).all() for x, y in zip(u, w))
        assert any((u[0] != w[0]).any() for u, w in zip(ans[False], ans[False][1:]))       # the answers follow the map
        a.enable_timing(True)
        before, la = map_state(a), _launches(a)
        for _ in range(3):
            a.clearance(boxes, r_max)
            a.clearance(boxes, r_max, stop_at="unseen", nearest=False)
        after, lb = map_state(a), _launches(a)
        assert la == lb
        assert all((u == w).all() for u, w in zip(before, after))
    finally:
        a.close(); b.close()


def test_clearance_between_frames_of_a_streaming_handle():
    """With frame 5's raycast held back on a streaming handle, the call flushes that raycast as a launch of its own, answers for the map with
    frame 5 fused, moves no other counter, and the image ring ends up as if the call had not been made."""
    f = 5
    rng = np.random.default_rng(5)
    boxes = np.ascontiguousarray(np.concatenate([rng.integers(0, 250, (2000, 3)), rng.integers(1, 9, (2000, 3))], 1).astype(np.int32))
    got = {}

    def action(p, box):
        got["streamed"] = p.clearance(boxes, 16)

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
        d2, near = ref.clearance(boxes, 16)
        assert (d2 == got["streamed"][0]).all() and (near == got["streamed"][1]).all()
        assert (d2 >= 0).any()
    finally:
        ref.close()


def test_clearance_entries_refuse_bad_arguments():
    import torch
    p = run_stream("room", SDF, 256, 2.4, 0, 1)
    try:
        lib = p.lib
        queries = np.zeros((4, 7), np.int32)
        queries[:, 3:6] = 1
        d2, near = np.zeros(4, np.int32), np.zeros((4, 3), np.int32)
        dq = torch.from_numpy(queries).to("cuda:0")
        dd2, dnear = torch.zeros(4, dtype=torch.int32, device="cuda:0"), torch.zeros((4, 3), dtype=torch.int32, device="cuda:0")
        good = _CollideTest(0.0, 0)
        for fn, qa, out, no_d2 in ((lib.se_hip_clearance_boxes_host, queries.ctypes.data, _ClearanceOut(d2.ctypes.data, near.ctypes.data), _ClearanceOut(None, near.ctypes.data)),
                                   (lib.se_hip_clearance_boxes, dq.data_ptr(), _ClearanceOut(dd2.data_ptr(), dnear.data_ptr()), _ClearanceOut(None, dnear.data_ptr()))):
            o = C.byref(out)
            for args in ((qa, -1, C.byref(good), 0, o), (None, 4, C.byref(good), 0, o), (qa, 4, C.byref(good), 0, C.byref(no_d2)), (qa, 4, C.byref(good), 0, None),
                         (qa, 4, None, 0, o), (qa, 4, C.byref(_CollideTest(float("nan"), 0)), 0, o), (qa, 4, C.byref(_CollideTest(float("inf"), 0)), 0, o),
                         (qa, 4, C.byref(_CollideTest(0.0, 2)), 0, o), (qa, 4, C.byref(good), 2, o), (qa, 4, C.byref(good), -1, o), (qa, 4, C.byref(good), 255, o)):
                assert fn(p._h, *args) == -1
            assert fn(p._h, None, 0, C.byref(good), 0, C.byref(_ClearanceOut(None, None))) == 0
            assert fn(p._h, qa, 4, C.byref(good), 1, C.byref(_ClearanceOut(out.d2, None))) == 0       # nearest not wanted
        p.sync()
    finally:
        p.close()
