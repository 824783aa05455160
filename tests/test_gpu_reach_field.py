"""The reachability field of a map region on the device (se_hip_reach_field / DenseSLAMPipeline.reach_field): the hand maps against the numpy
truth, fused maps against the truth over the class grid, the identities that tie the field to the strict box query and to the motion query,
the refusals through the C ABI, and the schedule (streaming handle; the map, the images and the launch counters left alone; a growing work
buffer).  Everything is integer: every comparison is equality."""
import ctypes as C

import numpy as np
import pytest

from supereight_amd.pipeline import (MOTION_FREE, OFUSION, REACH_AT_SEED, REACH_MOVES, REACH_NONE, SDF, DenseSLAMPipeline, _CollideTest, _ReachOut,
                                     _ReachRequest, reach_path)
from tests.clearance_util import OCC, UNSEEN
from tests.gpu_state_util import H, W, bits, map_state, run_stream, streamed_with
from tests.motion_util import class_grid
from tests.reach_util import (COMB_SEEDS, COMB_TABLE, DEVICE_REQUESTS, HAND_CASES, LIMIT, REACH_MAPS, free_positions, hand_truth, reach_truth,
                              stamp_reach_map)

pytestmark = pytest.mark.gpu

STOPS = (("occupied", OCC), ("unseen", UNSEEN))
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def _ask(p, rq, stop, **kw):
    lo, side, robot, seeds = rq
    return p.reach_field(lo, side, np.array(seeds, np.int64), robot=robot, stop_at=stop, **kw)


def _same(got, truth, what):
    """steps, seed, next and the first three counts equal the truth; rounds <= max steps + 2"""
    _, steps, seed, nxt, counts = truth
    for k, exp in (("steps", steps), ("seed", seed), ("next", nxt)):
        bad = np.argwhere(got[k] != exp)
        assert bad.size == 0, (what, k, len(bad), bad[:3], [(got[k][tuple(b)], exp[tuple(b)]) for b in bad[:3]])
    assert tuple(got["counts"][:3].tolist()) == counts, (what, got["counts"], counts)
    assert 1 <= got["counts"][3] <= counts[2] + 2, (what, got["counts"], counts)


@pytest.mark.parametrize("field", [SDF, OFUSION], ids=["sdf", "ofusion"])
@pytest.mark.parametrize("max_blocks", [0, 1024], ids=["dense", "pooled"])
def test_hand_maps_against_the_truth(field, max_blocks):
    occupied_x, empty_x = (-0.5, 0.5) if field == SDF else (2.0, -2.0)
    robots_seen = set()
    seen = {"blocked": 0, "reached": 0, "cut": 0}
    for mp in REACH_MAPS:
        p = DenseSLAMPipeline((W, H), 64, 1.28, field_type=field, max_blocks=max_blocks)
        try:
            stamp_reach_map(p, mp, occupied_x, empty_x)
            for stop, code in STOPS:
                for rq in DEVICE_REQUESTS[mp]:
                    truth = hand_truth(mp, rq[:3], rq[3], code)
                    got = _ask(p, rq, stop, seed=True, next=True, counts=True)
                    _same(got, truth, (mp, stop, rq))
                    again = _ask(p, rq, stop, seed=True, next=True, counts=True)
                    assert all((got[k] == again[k]).all() for k in ("steps", "seed", "next")) and (got["counts"][:3] == again["counts"][:3]).all()
                    alone = _ask(p, rq, stop)
                    assert set(alone) == {"steps"} and (alone["steps"] == truth[1]).all(), (mp, stop, rq)
                    seen["blocked"] += int((~truth[0]).sum()); seen["reached"] += int((truth[1] >= 0).sum()); seen["cut"] += int((truth[0] & (truth[1] < 0)).sum())
                    robots_seen.add(rq[2])
            if mp == "comb":
                for rq, code, counts, usable in COMB_TABLE:
                    got = _ask(p, rq + (COMB_SEEDS,), STOPS[code][0], seed=True, counts=True)
                    assert tuple(got["counts"][:3].tolist()) == counts and got["counts"][3] <= counts[2] + 2
                    assert sorted(set(got["seed"][got["steps"] == 0].tolist())) == list(usable)
            if mp == "wall":
                inside, below = DEVICE_REQUESTS["wall"][-3], DEVICE_REQUESTS["wall"][-2]
                beyond = (slice(None), slice(None), slice(11, None))              # x > 20
                assert (_ask(p, inside, "occupied")["steps"][beyond] == REACH_NONE).all()
                assert (_ask(p, below, "occupied")["steps"][beyond] >= 0).all()            # round the outside, where unseen does not block
                assert (_ask(p, below, "unseen")["steps"][beyond] == REACH_NONE).all()
            # the hand-worked requests
            for name, (cmap, lo, side, robot, seeds, occ, uns) in HAND_CASES.items():
                if cmap != mp or occ is None:
                    continue
                for stop, exp in (("occupied", occ), ("unseen", uns)):
                    got = _ask(p, (lo, side, robot, seeds), stop, seed=True, next=True)
                    assert list(zip(*(got[k].reshape(-1).tolist() for k in ("steps", "seed", "next")))) == exp, (name, stop)
        finally:
            p.close()
    assert {(1, 1, 1), (2, 2, 2), (3, 3, 3), (9, 3, 1), (4, 1, 1)} <= robots_seen
    assert all(v > 0 for v in seen.values()), seen


def _hit(p, n, dim, rng):
    v, nrm = p.vertex_normal()
    hits = v[nrm[..., 0] != -2].reshape(-1, 3)
    hits = hits[(hits > 0).all(1)]                                       # (a pixel without a surface may hold a zero vertex)
    assert len(hits) > 100
    return (hits[rng.integers(len(hits))] * (n / dim)).astype(np.int64)


def _free_seeds(grid, region, code, rng, count=3):
    """`count` free positions of the region, from the truth's free mask (absolute x, y, z); where the region holds fewer, its min corner
    makes up the number (a seed that is not free: ignored)"""
    lo = region[0]
    free = np.argwhere(free_positions(grid, region, code))               # (k, j, i)
    pick = free[rng.choice(len(free), min(count, len(free)), replace=False)]
    return tuple((int(lo[0] + i), int(lo[1] + j), int(lo[2] + k)) for k, j, i in pick) + (tuple(lo),) * (count - len(pick))


def _fused_requests(p, grid, n, dim, rng, robots=((1, 1, 1), (2, 2, 2))):
    h = _hit(p, n, dim, rng)
    regions = [(tuple(int(x) for x in h - (20, 12, 8)), (40, 24, 16), robots[0]),                       # on the raycast hits
               ((-12, int(h[1]) - 12, int(h[2]) - 12), (24, 24, 24), robots[1])]                        # across the face x = 0
    return [(rg, code, stop, _free_seeds(grid, rg, code, rng)) for rg in regions for stop, code in STOPS]


FUSED = [("room", SDF, 0), ("room", SDF, 2048), ("stress", OFUSION, 0), ("stress", OFUSION, 2048)]


@pytest.mark.parametrize("kind,field,max_blocks", FUSED, ids=[f"{k}_{'sdf' if f == SDF else 'ofusion'}_{'dense' if m == 0 else 'pooled'}" for k, f, m in FUSED])
def test_fused_maps_against_the_truth(kind, field, max_blocks):
    import torch
    n, dim = 128, 2.4
    rng = np.random.default_rng(n + field + max_blocks)
    p = run_stream(kind, field, n, dim, max_blocks, 4)
    try:
        grid = class_grid(p, n, dim, 0.0, field == OFUSION).cpu().numpy()
        kinds = {"blocked": 0, "reached": 0, "unreached": 0, "cut": 0}
        for rg, code, stop, seeds in _fused_requests(p, grid, n, dim, rng):
            rq = rg + (seeds,)
            truth = reach_truth(grid, rg, seeds, code)
            got = _ask(p, rq, stop, seed=True, next=True, counts=True)
            _same(got, truth, (rq, stop))
            dev = _ask(p, rq, stop, seed=True, next=True, counts=True, device=True)
            for k, dt in (("steps", torch.int32), ("seed", torch.uint8), ("next", torch.uint8)):
                assert isinstance(dev[k], torch.Tensor) and dev[k].dtype == dt and dev[k].device.type == "cuda" and tuple(dev[k].shape) == truth[1].shape
            _same({k: (v.cpu().numpy() if k != "counts" else v) for k, v in dev.items()}, truth, (rq, stop, "device"))
            alone = _ask(p, rq, stop, device=True)
            assert set(alone) == {"steps"} and (alone["steps"].cpu().numpy() == truth[1]).all()
            kinds["blocked"] += int((~truth[0]).sum()); kinds["reached"] += int((truth[1] >= 0).sum()); kinds["unreached"] += int((truth[1] < 0).sum())
            kinds["cut"] += int((truth[0] & (truth[1] < 0)).sum())
        print(kinds)                                                         # (cut: free, yet cut off from every seed -- the scene decides)
        assert kinds["blocked"] > 0 and kinds["reached"] > 0 and kinds["unreached"] > 0, kinds
    finally:
        p.close()


@pytest.mark.parametrize("kind,field,max_blocks", [("room", SDF, 2048), ("stress", OFUSION, 0)], ids=["room_sdf_pooled", "stress_ofusion_dense"])
def test_identities_against_the_other_readers(kind, field, max_blocks):
    n, dim = 128, 2.4
    rng = np.random.default_rng(5 + field)
    p = run_stream(kind, field, n, dim, max_blocks, 4)
    try:
        grid = class_grid(p, n, dim, 0.0, field == OFUSION).cpu().numpy()
        walked = 0
        for rg, code, stop, seeds in _fused_requests(p, grid, n, dim, rng, robots=((2, 3, 1), (1, 1, 1))):
            lo, side, robot = rg
            got = _ask(p, rg + (seeds,), stop, seed=True, next=True)
            steps, seed, nxt = got["steps"], got["seed"], got["next"]
            # steps >= 0 implies that the strict box query of (v, robot) answers a status above stop_at, for every position
            ax = [np.arange(lo[k], lo[k] + side[k], dtype=np.int64) for k in range(3)]
            v = np.stack(np.broadcast_arrays(ax[0][None, None, :], ax[1][None, :, None], ax[2][:, None, None]), -1).reshape(-1, 3)
            boxes = np.ascontiguousarray(np.concatenate([v, np.broadcast_to(np.asarray(robot, np.int64), v.shape)], 1).astype(np.int32))
            status = p.collides(boxes).reshape(steps.shape)
            assert (status[steps >= 0] > code).all()
            assert ((steps >= 0) | (seed == 255)).all() and ((steps >= 0) == (nxt != 255)).all() and ((steps == 0) == (nxt == REACH_AT_SEED)).all()
            # sampled reached positions: the path arrives at seed seed[v] after steps[v] moves, and every move of it is free for the motion query
            reached = np.argwhere(steps >= 0)
            if len(reached) == 0:
                continue
            motions = []
            for k, j, i in reached[rng.choice(len(reached), min(256, len(reached)), replace=False)]:
                start = (lo[0] + int(i), lo[1] + int(j), lo[2] + int(k))
                path = reach_path(nxt, lo, start)
                assert len(path) == steps[k, j, i] + 1 and tuple(path[0]) == start and tuple(path[-1]) == tuple(seeds[seed[k, j, i]])
                d = np.diff(path, axis=0)
                assert (np.abs(d).sum(1) == 1).all()
                motions.append(np.concatenate([path[:-1], np.broadcast_to(np.asarray(robot, np.int64), d.shape), d], 1))
                walked += len(d)
            motions = np.ascontiguousarray(np.concatenate(motions).astype(np.int32))
            if len(motions):
                _, t_first = p.collides_moving(motions, stop_at=stop)
                assert (t_first == np.float32(MOTION_FREE)).all()
        assert walked > 1000
    finally:
        p.close()


def _request(seeds, lo=(0, 0, 0), side=(4, 4, 4), robot=(1, 1, 1), stop_at=0, n_seeds=None):
    rq = _ReachRequest()
    rq.stop_at, rq.n_seeds, rq.seeds = stop_at, len(seeds) if n_seeds is None else n_seeds, seeds.ctypes.data if seeds is not None else None
    for k in range(3):
        rq.lo[k], rq.side[k], rq.robot[k] = lo[k], side[k], robot[k]
    return rq


def test_reach_entries_refuse_bad_requests():
    import torch
    p = run_stream("room", SDF, 128, 2.4, 0, 1)
    try:
        lib, L = p.lib, LIMIT
        sd = np.array([[1, 1, 1], [2, 2, 2]], np.int32)
        many = np.zeros((256, 3), np.int32)
        ends = np.array([[I32_MIN, I32_MIN, I32_MIN], [I32_MAX, I32_MAX, I32_MAX], [I32_MAX, 0, I32_MIN], [1, 1, 1]], np.int32)
        bad_requests = [_request(sd, side=(4, 0, 4)), _request(sd, side=(-1, 4, 4)), _request(sd, robot=(1, 1, 0)), _request(sd, robot=(257, 1, 1)),
                        _request(sd, lo=(-L - 1, 0, 0)), _request(sd, lo=(0, L + 1, 0)), _request(sd, lo=(0, 0, L - 5), robot=(1, 1, 2)), _request(sd, lo=(0, 0, L - 4)),
                        _request(sd, side=(256, 256, 257)), _request(sd, side=(1 << 19, 1 << 19, 1 << 19), lo=(-L, -L, -L)),
                        _request(sd, stop_at=2), _request(sd, stop_at=-1), _request(sd, stop_at=255),
                        _request(sd, n_seeds=0), _request(sd, n_seeds=-1), _request(many, n_seeds=256), _request(None, n_seeds=2)]
        host = [np.full((4, 4, 4), 77, np.int32), np.full((4, 4, 4), 77, np.uint8), np.full((4, 4, 4), 77, np.uint8)]
        dev = [torch.full((4, 4, 4), 77, dtype=dt, device="cuda:0") for dt in (torch.int32, torch.uint8, torch.uint8)]
        counts = np.full(4, 77, np.int64)
        good = _CollideTest(0.0, 0)
        untouched = {"host": lambda: all((a == 77).all() for a in host), "device": lambda: all(bool((a == 77).all()) for a in dev)}
        for which, fn, ptrs in (("host", lib.se_hip_reach_field_host, [a.ctypes.data for a in host]), ("device", lib.se_hip_reach_field, [a.data_ptr() for a in dev])):
            counts[:] = 77
            out, no_steps = _ReachOut(*ptrs, counts.ctypes.data), _ReachOut(None, ptrs[1], ptrs[2], counts.ctypes.data)
            o, ok = C.byref(out), C.byref(_request(sd))
            for rq in bad_requests:
                assert fn(p._h, C.byref(rq), C.byref(good), o) == -1
            for args in ((None, C.byref(good), o), (ok, None, o), (ok, C.byref(good), None), (ok, C.byref(good), C.byref(no_steps)),
                         (ok, C.byref(_CollideTest(float("nan"), 0)), o), (ok, C.byref(_CollideTest(float("inf"), 0)), o), (ok, C.byref(_CollideTest(0.0, 2)), o),
                         (ok, C.byref(_CollideTest(0.0, -1)), o)):
                assert fn(p._h, *args) == -1
            p.sync()
            assert untouched[which]() and (counts == 77).all()      # the outputs are untouched
            # the bounds themselves are valid: lo = -2^19, lo + side + robot = 2^19, a robot of 256, 255 seeds
            assert fn(p._h, C.byref(_request(sd, lo=(-L, 5, L - 8), robot=(2, 1, 4))), C.byref(good), o) == 0
            assert fn(p._h, C.byref(_request(sd, lo=(60, 60, 60), robot=(256, 1, 256), stop_at=1)), C.byref(good), o) == 0
            assert fn(p._h, C.byref(_request(many, n_seeds=255)), C.byref(good), o) == 0
            assert fn(p._h, C.byref(_request(sd)), C.byref(good), C.byref(_ReachOut(ptrs[0], None, None, None))) == 0       # steps alone
            # seeds at the ends of int32 are accepted and ignored: the answer is that of the one seed inside
            assert fn(p._h, C.byref(_request(ends)), C.byref(good), o) == 0
            p.sync()
        assert all((h == d.cpu().numpy()).all() for h, d in zip(host, dev))
        one = p.reach_field((0, 0, 0), (4, 4, 4), [(1, 1, 1)], seed=True, next=True)
        assert (host[0] == one["steps"]).all() and (host[2] == one["next"]).all() and (np.where(host[1] == 255, 255, 0) == one["seed"]).all()
        assert set(host[1].reshape(-1).tolist()) <= {3, 255}
    finally:
        p.close()


def _field(p, rq, **kw):
    got = _ask(p, rq, kw.pop("stop_at", "occupied"), seed=True, next=True, **kw)
    return [got[k] if isinstance(got[k], np.ndarray) else got[k].cpu().numpy() for k in ("steps", "seed", "next")]


def _around_hit(p, n, dim, side, robot=(1, 1, 1), grid=None):
    """A request whose region is centred on a raycast hit of the last frame, seeded at three of its corners and its centre -- any of which
    the scene may leave unusable -- and, with the class grid of `p`, at three positions that are free even where unseen stops."""
    h = _hit(p, n, dim, np.random.default_rng(11))
    lo = tuple(int(h[k]) - side[k] // 2 for k in range(3))
    seeds = (lo, tuple(lo[k] + side[k] - 1 for k in range(3)), (lo[0] + side[0] - 1, lo[1], lo[2]), tuple(int(x) for x in h))
    if grid is not None:
        seeds += _free_seeds(grid, (lo, side, robot), UNSEEN, np.random.default_rng(12))
    return (lo, side, robot, seeds)


@pytest.mark.parametrize("field", [SDF, OFUSION], ids=["sdf", "ofusion"])
def test_reach_sees_the_map_of_the_frames_before_it(field):
    """On a streaming handle (scans on the side stream, raycasts held back) the answer after frame f equals the synchronous handle's; the
    calls change neither the map, the images nor the launch counters; the answers survive a work buffer that grows between two calls."""
    ans = {True: [], False: []}
    n = 128
    probe = run_stream("room", field, n, 2.4, 0, 4)
    try:
        grid = class_grid(probe, n, 2.4, 0.0, field == OFUSION).cpu().numpy()
        rq = _around_hit(probe, n, 2.4, (72, 40, 24), grid=grid)           # around a raycast hit of the last frame, the same for both handles
        assert free_positions(grid, rq[:3], UNSEEN).any()                  # (the last three seeds are usable under both stop_at)
    finally:
        probe.close()

    def rec(streaming):
        def check(p, f):
            ans[streaming].append(_field(p, rq) + _field(p, rq, stop_at="unseen"))
        return check

    b = run_stream("room", field, n, 2.4, 0, 4, streaming=False, check=rec(False))
    a = run_stream("room", field, n, 2.4, 0, 4, streaming=True, check=rec(True))
    try:
        for u, w in zip(ans[True], ans[False]):
            assert all((x == y).all() for x, y in zip(u, w))
        # the answers are those of a fused map: an empty one is free everywhere with stop_at occupied and nowhere with unseen
        u = ans[False][-1]
        assert (u[0] >= 0).any() and (u[0] == REACH_NONE).any() and (u[3] >= 0).any()
        a.enable_timing(True)
        before, la = map_state(a), {k: d["launches"] for k, d in a.timings().items()}
        # small, then large (the work buffer grows), then small again: host entry and device entry
        SMALL, LARGE = (rq[0], (6, 5, 4), (1, 1, 1), rq[3]), (rq[0], (72, 40, 24), (2, 2, 2), rq[3])
        first = _field(a, SMALL)
        large = _field(a, LARGE)
        again = _field(a, SMALL)
        assert all((x == y).all() for x, y in zip(first, again))
        dev_first = _field(a, SMALL, device=True)
        dev_large = _field(a, (rq[0], (100, 60, 40), (2, 2, 2), rq[3]), device=True)
        dev_again = _field(a, SMALL, device=True)
        assert all((x == y).all() for x, y in zip(first, dev_first)) and all((x == y).all() for x, y in zip(first, dev_again))
        assert (large[0] >= 0).any() and (dev_large[0] >= 0).any()
        assert all((x == y).all() for x, y in zip(large, _field(b, LARGE)))
        assert all((x == y).all() for x, y in zip(first, _field(b, SMALL)))
        after, lb = map_state(a), {k: d["launches"] for k, d in a.timings().items()}
        assert la == lb
        assert all((u == w).all() for u, w in zip(before, after))
    finally:
        a.close(); b.close()


def test_reach_between_frames_of_a_streaming_handle():
    """With frame 5's raycast held back on a streaming handle, the call flushes that raycast as a launch of its own, answers for the map with
    frame 5 fused, moves no other counter, and the image ring -- the next frames' raycasts included -- ends up bit-equal to a handle that
    never made the call."""
    f = 5
    ref = run_stream("room", SDF, 256, 2.4, 0, f + 1)
    rq = _around_hit(ref, 256, 2.4, (48, 40, 24))
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
        exp = _field(ref, rq)
        assert all((x == y).all() for x, y in zip(exp, got["streamed"]))
        assert (exp[0] >= 0).any()
    finally:
        ref.close()
