"""The distance field of a map region on the device (se_hip_distance_field / DenseSLAMPipeline.distance_field): the hand maps against the
numpy truth (clearance_truth per voxel), fused maps against the device's own clearance query over every voxel of the region, the identities
that tie the field to the strict box query, the refusals through the C ABI, and the schedule (streaming handle; the map, the images and the
launch counters left alone; a growing work buffer).  Everything is integer: every comparison is equality."""
import ctypes as C

import numpy as np
import pytest

from supereight_amd.pipeline import CLEARANCE_NONE, OFUSION, SDF, DenseSLAMPipeline, _CollideTest, _FieldOut, _FieldRequest
from tests.clearance_util import CLEAR_MAPS, I32_MIN, OCC, UNSEEN, stamp_clear_map
from tests.field_util import DEVICE_REQUESTS, HAND_CASES, LIMIT, d2_of_field, field_truth, hand_truth, voxel_boxes
from tests.gpu_state_util import H, W, bits, map_state, run_stream, streamed_with
from tests.motion_util import class_grid

pytestmark = pytest.mark.gpu

STOPS = (("occupied", OCC), ("unseen", UNSEEN))
# Where the model itself cannot give all of d2 == 0, d2 > 0 and NONE: `free` holds no occupied voxel (everything is NONE with stop_at
# occupied); in `octant` every voxel outside the octant is unseen (every box touches a blocking voxel with stop_at unseen).
ONLY = {("free", "occupied"): "none", ("octant", "unseen"): "zero"}


def _same(got, exp, what):
    d2, near = got
    bad = np.argwhere((d2 != exp[0]) | (near != exp[1]).any(-1))
    assert bad.size == 0, (what, len(bad), bad[:3], [(d2[tuple(b)], exp[0][tuple(b)], near[tuple(b)], exp[1][tuple(b)]) for b in bad[:3]])


@pytest.mark.parametrize("field", [SDF, OFUSION], ids=["sdf", "ofusion"])
@pytest.mark.parametrize("max_blocks", [0, 1024], ids=["dense", "pooled"])
def test_hand_maps_against_the_truth(field, max_blocks):
    occupied_x, empty_x = (-0.5, 0.5) if field == SDF else (2.0, -2.0)
    ties = 0
    r_seen, robots_seen = set(), set()
    for mp in CLEAR_MAPS:
        p = DenseSLAMPipeline((W, H), 64, 1.28, field_type=field, max_blocks=max_blocks)
        try:
            stamp_clear_map(p, mp, occupied_x, empty_x)
            for stop, code in STOPS:
                seen = {"zero": 0, "pos": 0, "none": 0, "outside": 0}
                for rq in DEVICE_REQUESTS[mp]:
                    lo, side, robot, r = rq
                    exp_d2, exp_near, tie = hand_truth(mp, rq, code)
                    got = p.distance_field(lo, side, r, robot=robot, stop_at=stop, nearest=True)
                    _same(got, (exp_d2, exp_near), (mp, stop, rq))
                    alone = p.distance_field(lo, side, r, robot=robot, stop_at=stop)
                    assert (alone == exp_d2).all(), (mp, stop, rq)
                    seen["zero"] += int((exp_d2 == 0).sum()); seen["pos"] += int((exp_d2 > 0).sum()); seen["none"] += int((exp_d2 == CLEARANCE_NONE).sum())
                    seen["outside"] += int(((exp_d2 >= 0) & ((exp_near < 0) | (exp_near >= 64)).any(-1)).sum())
                    if mp in ("wall", "gap"):
                        ties += int(tie.sum())
                    r_seen.add(r); robots_seen.add(robot)
                only = ONLY.get((mp, stop))
                for k in ("zero", "pos", "none"):
                    assert (seen[k] > 0) == (only is None or only == k), (mp, stop, seen)
                if stop == "unseen":
                    assert seen["outside"] > 0, (mp, seen)
            # the hand-worked requests
            for name, (cmap, lo, side, robot, r, occ, uns) in HAND_CASES.items():
                if cmap != mp or occ is None:
                    continue
                for stop, exp in (("occupied", occ), ("unseen", uns)):
                    d2, near = p.distance_field(lo, side, r, robot=robot, stop_at=stop, nearest=True)
                    assert [(int(d), tuple(w.tolist())) for d, w in zip(d2.reshape(-1), near.reshape(-1, 3))] == exp, (name, stop)
        finally:
            p.close()
    assert ties >= 20                                                     # the truth found more than one minimiser: the tie rule decided
    assert {0, 1, 7, 8, 9, 63, 64, 65, 255} <= r_seen
    assert {(1, 1, 1), (2, 2, 2), (8, 8, 8), (9, 3, 1)} <= robots_seen


def _hit(p, n, dim, rng):
    v, nrm = p.vertex_normal()
    hits = v[nrm[..., 0] != -2].reshape(-1, 3)
    hits = hits[(hits > 0).all(1)]                                       # (a pixel without a surface may hold a zero vertex)
    assert len(hits) > 100
    return (hits[rng.integers(len(hits))] * (n / dim)).astype(np.int64)


def _around_hit(p, n, dim, side, r_max, robot=(1, 1, 1)):
    """A request whose region is centred on a raycast hit of the last frame."""
    h = _hit(p, n, dim, np.random.default_rng(11))
    return (tuple(int(h[k]) - side[k] // 2 for k in range(3)), side, robot, r_max)


def _clearance_field(p, rq, stop):
    """The device's clearance query over every voxel of the request, shaped as the field."""
    lo, side, robot, r = rq
    d2, near = p.clearance(voxel_boxes(rq), r, stop_at=stop)
    shape = (side[2], side[1], side[0])
    return d2.reshape(shape), near.reshape(shape + (3,))


FUSED = [("room", SDF, 0), ("room", SDF, 2048), ("stress", OFUSION, 0), ("stress", OFUSION, 2048)]


@pytest.mark.parametrize("kind,field,max_blocks", FUSED, ids=[f"{k}_{'sdf' if f == SDF else 'ofusion'}_{'dense' if m == 0 else 'pooled'}" for k, f, m in FUSED])
def test_fused_maps_against_the_clearance_query(kind, field, max_blocks):
    import torch
    n, dim = 128, 2.4
    rng = np.random.default_rng(n + field + max_blocks)
    p = run_stream(kind, field, n, dim, max_blocks, 4)
    try:
        grid = class_grid(p, n, dim, 0.0, field == OFUSION).cpu().numpy()
        h = _hit(p, n, dim, rng)
        requests = [(tuple(int(x) for x in h - (20, 12, 8)), (40, 24, 16), (1, 1, 1), 12),                       # on the raycast hits
                    ((-12, int(h[1]) - 12, int(h[2]) - 12), (24, 24, 24), (3, 3, 2), 6)]                         # across the face x = 0
        kinds = {"zero": 0, "pos": 0, "none": 0}
        for rq in requests:
            lo, side, robot, r = rq
            sample = rng.choice(side[0] * side[1] * side[2], 512, replace=False)
            for stop, code in STOPS:
                exp = _clearance_field(p, rq, stop)
                got = p.distance_field(lo, side, r, robot=robot, stop_at=stop, nearest=True)
                _same(got, exp, (rq, stop))
                t_d2, t_near, _ = field_truth(grid, rq, code, only=sample)
                assert (got[0].reshape(-1)[sample] == t_d2).all() and (got[1].reshape(-1, 3)[sample] == t_near).all(), (rq, stop)
                assert (p.distance_field(lo, side, r, robot=robot, stop_at=stop) == exp[0]).all()
                dev = p.distance_field(lo, side, r, robot=robot, stop_at=stop, nearest=True, device=True)
                assert all(isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.device.type == "cuda" for t in dev)
                assert tuple(dev[0].shape) == exp[0].shape and tuple(dev[1].shape) == exp[1].shape
                _same((dev[0].cpu().numpy(), dev[1].cpu().numpy()), exp, (rq, stop, "device"))
                alone = p.distance_field(lo, side, r, robot=robot, stop_at=stop, device=True)
                assert isinstance(alone, torch.Tensor) and (alone.cpu().numpy() == exp[0]).all()
                kinds["zero"] += int((exp[0] == 0).sum()); kinds["pos"] += int((exp[0] > 0).sum()); kinds["none"] += int((exp[0] == CLEARANCE_NONE).sum())
        print(kinds)
        assert kinds["zero"] > 0 and kinds["pos"] > 0 and kinds["none"] > 0
    finally:
        p.close()


@pytest.mark.parametrize("field,max_blocks", [(SDF, 2048), (OFUSION, 0)], ids=["sdf_pooled", "ofusion_dense"])
def test_identities_against_the_strict_box_query(field, max_blocks):
    n, dim = 128, 2.4
    rng = np.random.default_rng(3 + field)
    p = run_stream("stress", field, n, dim, max_blocks, 4)
    try:
        h = _hit(p, n, dim, rng)
        out = {}
        for rq in [(tuple(int(x) for x in h - (12, 10, 8)), (24, 20, 16), (2, 3, 1), 7), ((n - 10, int(h[1]) - 6, -6), (16, 12, 12), (1, 1, 1), 9)]:
            lo, side, robot, r = rq
            for stop, code in STOPS:
                d2, near = p.distance_field(lo, side, r, robot=robot, stop_at=stop, nearest=True)
                found = d2 >= 0
                assert (d2 >= CLEARANCE_NONE).all() and (d2[found] <= r * r).all() and (near[~found] == I32_MIN).all()
                # d2 == 0 <=> the voxel's box grown by one voxel holds a blocking voxel
                assert ((d2.reshape(-1) == 0) == (p.collides(voxel_boxes(rq, 1)) <= code)).all()
                # the witness blocks, and gives d2 back
                assert (d2_of_field(rq, near)[found] == d2[found]).all()
                w = near[found]
                assert (p.collides(np.ascontiguousarray(np.concatenate([w, np.ones_like(w)], 1))) <= code).all()
                # a larger r_max changes no answer that was found
                more_d2, more_near = p.distance_field(lo, side, r + 5, robot=robot, stop_at=stop, nearest=True)
                assert (more_d2[found] == d2[found]).all() and (more_near[found] == near[found]).all() and (more_d2 >= 0).sum() >= found.sum()
                out[(rq, stop)] = d2.astype(np.int64)
            # unseen blocking can only bring the nearest blocking voxel closer
            big = np.int64(1) << 40
            d_occ, d_uns = out[(rq, "occupied")], out[(rq, "unseen")]
            assert (np.where(d_uns < 0, big, d_uns) <= np.where(d_occ < 0, big, d_occ)).all()
        d2 = np.concatenate([v.reshape(-1) for v in out.values()])
        assert (d2 == 0).any() and (d2 > 0).any() and (d2 == CLEARANCE_NONE).any()
    finally:
        p.close()


def _request(lo=(0, 0, 0), side=(4, 4, 4), robot=(1, 1, 1), r_max=4, stop_at=0):
    rq = _FieldRequest()
    rq.r_max, rq.stop_at = r_max, stop_at
    for k in range(3):
        rq.lo[k], rq.side[k], rq.robot[k] = lo[k], side[k], robot[k]
    return rq


def test_field_entries_refuse_bad_requests():
    import torch
    p = run_stream("room", SDF, 128, 2.4, 0, 1)
    try:
        lib, L = p.lib, LIMIT
        bad_requests = [_request(side=(4, 0, 4)), _request(side=(-1, 4, 4)), _request(robot=(1, 1, 0)), _request(robot=(257, 1, 1)), _request(r_max=-1), _request(r_max=256),
                        _request(lo=(-L - 1, 0, 0)), _request(lo=(0, L + 1, 0)), _request(lo=(0, 0, L - 5), robot=(1, 1, 2)), _request(lo=(0, 0, L - 4), side=(4, 4, 4)),
                        _request(side=(256, 256, 257), r_max=0), _request(side=(1025, 2, 2), r_max=254), _request(side=(1 << 19, 1 << 19, 1 << 19), lo=(-L, -L, -L)),
                        _request(stop_at=2), _request(stop_at=-1), _request(stop_at=255)]
        host = [np.full((4, 4, 4), 77, np.int32), np.full((4, 4, 4, 3), 77, np.int32)]
        dev = [torch.full((4, 4, 4), 77, dtype=torch.int32, device="cuda:0"), torch.full((4, 4, 4, 3), 77, dtype=torch.int32, device="cuda:0")]
        good = _CollideTest(0.0, 0)
        untouched = {"host": lambda: all((a == 77).all() for a in host), "device": lambda: all(bool((a == 77).all()) for a in dev)}
        for which, fn, out, no_d2 in (("host", lib.se_hip_distance_field_host, _FieldOut(host[0].ctypes.data, host[1].ctypes.data), _FieldOut(None, host[1].ctypes.data)),
                                      ("device", lib.se_hip_distance_field, _FieldOut(dev[0].data_ptr(), dev[1].data_ptr()), _FieldOut(None, dev[1].data_ptr()))):
            o, ok = C.byref(out), C.byref(_request())
            for rq in bad_requests:
                assert fn(p._h, C.byref(rq), C.byref(good), o) == -1
            for args in ((None, C.byref(good), o), (ok, None, o), (ok, C.byref(good), None), (ok, C.byref(good), C.byref(no_d2)),
                         (ok, C.byref(_CollideTest(float("nan"), 0)), o), (ok, C.byref(_CollideTest(float("inf"), 0)), o), (ok, C.byref(_CollideTest(0.0, 2)), o),
                         (ok, C.byref(_CollideTest(0.0, -1)), o)):
                assert fn(p._h, *args) == -1
            p.sync()
            assert untouched[which]()                      # the outputs are untouched
            # the bounds themselves are valid: lo = -2^19, lo + side + robot = 2^19, r_max 255 with a robot of 256
            assert fn(p._h, C.byref(_request(lo=(-L, 5, L - 8), robot=(2, 1, 4), r_max=3)), C.byref(good), o) == 0
            assert fn(p._h, C.byref(_request(lo=(60, 60, 60), robot=(256, 1, 256), r_max=255, stop_at=1)), C.byref(good), o) == 0
            assert fn(p._h, C.byref(_request()), C.byref(good), C.byref(_FieldOut(out.d2, None))) == 0       # nearest not wanted
            p.sync()
        assert (host[0] != 77).all() and bool((dev[0] != 77).all())
        assert (host[0] == dev[0].cpu().numpy()).all() and (host[1] == dev[1].cpu().numpy()).all()
    finally:
        p.close()


def _launches(p):
    return {k: d["launches"] for k, d in p.timings().items()}


def _field(p, rq, **kw):
    return p.distance_field(rq[0], rq[1], rq[3], robot=rq[2], nearest=True, **kw)


@pytest.mark.parametrize("field", [SDF, OFUSION], ids=["sdf", "ofusion"])
def test_field_sees_the_map_of_the_frames_before_it(field):
    """On a streaming handle (scans on the side stream, raycasts held back) the answer after frame f equals the synchronous handle's; the
    calls change neither the map, the images nor the launch counters; the answers survive a work buffer that grows between two calls."""
    ans = {True: [], False: []}
    probe = run_stream("room", field, 256, 2.4, 0, 4)
    try:
        rq = _around_hit(probe, 256, 2.4, (96, 80, 48), 8)                  # around a raycast hit of the last frame, the same for both handles
    finally:
        probe.close()

    def rec(streaming):
        def check(p, f):
            ans[streaming].append(_field(p, rq) + _field(p, rq, stop_at="unseen"))
        return check

    b = run_stream("room", field, 256, 2.4, 0, 4, streaming=False, check=rec(False))
    a = run_stream("room", field, 256, 2.4, 0, 4, streaming=True, check=rec(True))
    try:
        for u, w in zip(ans[True], ans[False]):
            assert all((x == y).all() for x, y in zip(u, w))
        # the answers are those of a fused map: an empty one gives NONE everywhere with stop_at occupied and 0 everywhere with unseen
        u = ans[False][-1]
        assert (u[0] >= 0).any() and (u[0] == CLEARANCE_NONE).any() and (u[2] != 0).any()
        a.enable_timing(True)
        before, la = map_state(a), _launches(a)
        # small, then large (the work buffer grows), then small again: host entry and device entry
        SMALL, LARGE = (rq[0], (6, 5, 4), (1, 1, 1), 3), (rq[0], (64, 48, 40), (2, 2, 2), 20)       # LARGE holds the hit the region is centred on
        first = _field(a, SMALL)
        large = _field(a, LARGE)
        again = _field(a, SMALL)
        assert all((x == y).all() for x, y in zip(first, again))
        dev_first = _field(a, SMALL, device=True)
        dev_large = _field(a, (rq[0], (80, 64, 48), (2, 2, 2), 20), device=True)
        dev_again = _field(a, SMALL, device=True)
        assert all((x == y.cpu().numpy()).all() for x, y in zip(first, dev_first)) and all((x == y.cpu().numpy()).all() for x, y in zip(first, dev_again))
        assert (dev_large[0].cpu().numpy()[:40, :48, :64] == large[0]).all() and (large[0] >= 0).any()
        exp = _field(b, SMALL)
        assert all((x == y).all() for x, y in zip(first, exp))
        after, lb = map_state(a), _launches(a)
        assert la == lb
        assert all((u == w).all() for u, w in zip(before, after))
    finally:
        a.close(); b.close()


def test_field_between_frames_of_a_streaming_handle():
    """With frame 5's raycast held back on a streaming handle, the call flushes that raycast as a launch of its own, answers for the map with
    frame 5 fused, moves no other counter, and the image ring -- the next frames' raycasts included -- ends up bit-equal to a handle that
    never made the call."""
    f = 5
    ref = run_stream("room", SDF, 256, 2.4, 0, f + 1)
    rq = _around_hit(ref, 256, 2.4, (48, 40, 24), 8)
    got = {}

    def action(p, box):
        got["streamed"] = _field(p, rq)

    ring, log = streamed_with(action, f)
    twin, _ = streamed_with(action, -1)
    assert log["fused"]
    assert (bits(ring) == bits(twin)).all()
    b, a, again = log["before"], log["after"], log["again"]
    assert b["pending"] and not a["pending"]
    assert a["raycast"] == b["raycast"] + 1 and a["fused"] == b["fused"]   # launched alone, not with a scan
    assert all(a[k] == b[k] for k in a if k not in ("raycast", "pending"))
    assert again == a
    try:
        d2, near = _field(ref, rq)
        assert (d2 == got["streamed"][0]).all() and (near == got["streamed"][1]).all()
        assert (d2 >= 0).any()
    finally:
        ref.close()
