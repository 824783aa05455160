"""Column projections on the device (se_hip_project_columns / DenseSLAMPipeline.project): the hand cases on maps built without depth (dense
and pooled, both fields, every axis, both stop_at); the four arrays against the definition evaluated in numpy over a dense class grid (room
SDF and stress OFusion, dense and pooled) with the identities that tie them to each other and to the strict box query; invalid requests
and the threshold direction; and the schedule (streaming handle, the map, the images and the launch counters left alone, the device entry
asynchronous).  Everything is integer: every comparison is equality."""
import ctypes as C
import functools

import numpy as np
import pytest

from supereight_amd.pipeline import OFUSION, PROJECT_NONE, SDF, DenseSLAMPipeline, _CollideTest, _ProjectOut, _ProjectRequest
from tests.gpu_state_util import H, W, bits, map_state, run_stream, streamed_with
from tests.motion_util import class_grid
from tests.project_util import (FOOTPRINTS, HAND_CELLS, HAND_MAPS, LAYERS16, LAYERS8, LIMIT, NONE, OCC, OUTPUTS, STOPS, UNSEEN, cell_boxes,
                                check_identities, conditions, hand_grid, merged, project_truth, stamp_hand_map, stamp_octants, stamps)
from tests.test_project_host import FUSED_DIM, FUSED_FRAMES, FUSED_LAYERS, FUSED_N

pytestmark = pytest.mark.gpu


def _same(got, exp, where):
    for k in got:
        bad = np.argwhere(np.asarray(got[k]) != exp[k])
        assert bad.size == 0, (where, k, bad[:5], [int(got[k][tuple(b)]) for b in bad[:5]], [int(exp[k][tuple(b)]) for b in bad[:5]])


@functools.lru_cache(maxsize=None)
def _hand_truth(name, axis, code, foot, layers):
    return project_truth(hand_grid(name), axis, foot[:2], foot[2:], list(layers), code)


@pytest.mark.parametrize("field", [SDF, OFUSION], ids=["sdf", "ofusion"])
@pytest.mark.parametrize("max_blocks", [0, 1024], ids=["dense", "pooled"])
def test_hand_cases_on_the_device(field, max_blocks):
    assert PROJECT_NONE == NONE
    occupied_x, empty_x = (-0.5, 0.5) if field == SDF else (2.0, -2.0)
    subsets = [dict(first=bool(m & 1), last=bool(m & 2), count=bool(m & 4)) for m in range(8)]
    for name in HAND_MAPS:
        p = DenseSLAMPipeline((W, H), 64, 1.28, field_type=field, max_blocks=max_blocks)
        try:
            stamp_hand_map(p, name, occupied_x, empty_x)
            for axis in (0, 1, 2):
                for stop, code in STOPS:
                    for fname, foot in FOOTPRINTS.items():
                        got = p.project(axis, foot[:2], foot[2:], LAYERS8, stop_at=stop)
                        _same(got, _hand_truth(name, axis, code, foot, tuple(LAYERS8)), (name, axis, stop, fname))
                    # 16 layers in one call
                    for fname in ("ragged", "overhang"):
                        foot = FOOTPRINTS[fname]
                        got = p.project(axis, foot[:2], foot[2:], LAYERS16, stop_at=stop)
                        exp = _hand_truth(name, axis, code, foot, tuple(LAYERS16))
                        _same(got, exp, (name, axis, stop, fname, 16))
                        check_identities(got, code)
                    # each subset of the optional outputs left null
                    foot = FOOTPRINTS["oblong"]
                    exp = _hand_truth(name, axis, code, foot, tuple(LAYERS8))
                    for want in subsets:
                        got = p.project(axis, foot[:2], foot[2:], LAYERS8, stop_at=stop, **want)
                        assert sorted(got) == sorted(["status"] + [k for k, v in want.items() if v])
                        _same(got, exp, (name, axis, stop, want))
            if name == "mix":
                for cname, (u, v, layer, occ, uns) in HAND_CELLS.items():
                    for (stop, _), exp in zip(STOPS, (occ, uns)):
                        got = p.project(2, (u, v), (1, 1), [layer], stop_at=stop)
                        assert tuple(int(got[k][0, 0, 0]) for k in OUTPUTS) == exp, (cname, stop)
        finally:
            p.close()


BRUTE = [("room", SDF, 0), ("room", SDF, 2048), ("stress", OFUSION, 0), ("stress", OFUSION, 2048)]


@pytest.mark.parametrize("kind,field,max_blocks", BRUTE, ids=[f"{k}_{'sdf' if f == SDF else 'ofusion'}_{'dense' if m == 0 else 'pooled'}" for k, f, m in BRUTE])
def test_fused_maps_equal_the_definition_and_keep_the_identities(kind, field, max_blocks):
    """128^3 maps of 4 fused frames with two stamped octants: per axis the whole footprint grown by 8 on every side, 5 layers, both stop_at.
    Against the numpy truth over the class grid; then, on the same cells, status = the strict box query of the cell's box, the relations
    among the four arrays, and a layer split at some w = its two parts merged."""
    n, dim = FUSED_N, FUSED_DIM
    occupied_x, empty_x = (-0.5, 0.5) if field == SDF else (2.0, -2.0)
    rng = np.random.default_rng(n + field + max_blocks)
    p = run_stream(kind, field, n, dim, max_blocks, FUSED_FRAMES)
    try:
        stamp_octants(p, n, occupied_x, empty_x)
        grid = class_grid(p, n, dim, 0.0, field == OFUSION).cpu().numpy()
        lo, side = (-8, -8), (n + 16, n + 16)
        occ_box, empty_box = stamps(n)
        for axis in (0, 1, 2):
            for stop, code in STOPS:
                exp = project_truth(grid, axis, lo, side, FUSED_LAYERS, code)
                got = p.project(axis, lo, side, FUSED_LAYERS, stop_at=stop)
                _same(got, exp, (axis, stop))
                seen = conditions(n, axis, lo, side, FUSED_LAYERS, code, got, occ_box, empty_box)
                print(axis, stop, seen)
                assert all(v > 0 for v in seen.values()), seen
                # identities
                check_identities(got, code)
                strict = p.collides(cell_boxes(axis, lo, side, FUSED_LAYERS)).reshape(got["status"].shape)
                assert (strict == got["status"]).all()
                whole = [(0, n), (-9, n + 9), (-LIMIT, LIMIT)]
                full = p.project(axis, lo, side, whole, stop_at=stop)
                for w in [1, 8, n // 2 + 3, n - 1] + rng.integers(2, n - 1, 2).tolist():
                    lower = p.project(axis, lo, side, [(a, w) for a, _ in whole], stop_at=stop)
                    upper = p.project(axis, lo, side, [(w, b) for _, b in whole], stop_at=stop)
                    _same(merged(lower, upper), full, (axis, stop, "split", w))
    finally:
        p.close()


def _request(axis=2, lo=(0, 0), side=(8, 8), layers=((0, 8),), stop_at=0):
    rq = _ProjectRequest()
    rq.axis, rq.n_layers, rq.stop_at = axis, len(layers), stop_at
    for k in range(2):
        rq.lo[k], rq.side[k] = lo[k], side[k]
    for l, (a, b) in enumerate(layers[:16]):
        rq.layers[l][0], rq.layers[l][1] = a, b
    return rq


@pytest.mark.parametrize("field,max_blocks", [(SDF, 0), (OFUSION, 4096)], ids=["sdf_dense", "ofusion_pooled"])
def test_invalid_requests_and_threshold_direction(field, max_blocks):
    import torch
    p = run_stream("room", field, 256, 2.4, max_blocks, 2)
    try:
        lib = p.lib
        good = _CollideTest(0.0, 0)
        L = LIMIT
        I32 = 2 ** 31 - 1
        bad_requests = [_request(axis=3), _request(axis=-1), _request(side=(0, 8)), _request(side=(8, -3)), _request(side=(8, -(1 << 31))),
                        _request(layers=((4, 4),)), _request(layers=((0, 8), (9, 3))), _request(lo=(-L - 1, 0)), _request(lo=(0, L)),
                        _request(lo=(L - 4, 0), side=(5, 1)), _request(lo=(I32, 0), side=(I32, 1)), _request(layers=((-L - 1, 0),)),
                        _request(layers=((0, L + 1),)), _request(layers=((-(1 << 31), I32),)), _request(side=(1 << 14, 1 << 14), layers=((0, 8), (0, 9))),
                        _request(stop_at=2), _request(stop_at=-1), _request(stop_at=255)]
        zero, seventeen = _request(), _request()
        zero.n_layers, seventeen.n_layers = 0, 17
        bad_requests += [zero, seventeen]
        cells = 64
        host = {k: np.full(cells, 77, np.uint8 if k == "status" else np.int32) for k in OUTPUTS}
        dev = {k: torch.full((cells,), 77, dtype=torch.uint8 if k == "status" else torch.int32, device="cuda:0") for k in OUTPUTS}
        untouched = {"host": lambda: all((host[k] == 77).all() for k in OUTPUTS), "device": lambda: all(bool((dev[k] == 77).all()) for k in OUTPUTS)}
        for which, fn, out, no_status in (("host", lib.se_hip_project_columns_host, _ProjectOut(*(host[k].ctypes.data for k in OUTPUTS)), _ProjectOut(None, *(host[k].ctypes.data for k in OUTPUTS[1:]))),
                                          ("device", lib.se_hip_project_columns, _ProjectOut(*(dev[k].data_ptr() for k in OUTPUTS)), _ProjectOut(None, *(dev[k].data_ptr() for k in OUTPUTS[1:])))):
            o, ok = C.byref(out), C.byref(_request())
            for rq in bad_requests:
                assert fn(p._h, C.byref(rq), C.byref(good), o) == -1
            for args in ((None, C.byref(good), o), (ok, None, o), (ok, C.byref(good), None), (ok, C.byref(good), C.byref(no_status)),
                         (ok, C.byref(_CollideTest(float("nan"), 0)), o), (ok, C.byref(_CollideTest(float("inf"), 0)), o), (ok, C.byref(_CollideTest(0.0, 2)), o),
                         (ok, C.byref(_CollideTest(0.0, -1)), o)):
                assert fn(p._h, *args) == -1
            p.sync()
            assert untouched[which]()                      # the outputs are untouched
            # the bounds themselves are valid: lo = -2^20, lo + side = 2^20, a layer [-2^20, 2^20), 16 layers
            edge = _request(lo=(-L, L - 8), side=(8, 8), layers=((-L, L),))
            assert fn(p._h, C.byref(edge), C.byref(good), o) == 0
            assert fn(p._h, C.byref(_request(side=(2, 2), layers=((0, 8),) * 16)), C.byref(good), o) == 0
            p.sync()
        assert (host["status"] != 77).all() and bool((dev["status"] != 77).all())
        assert (host["status"] == dev["status"].cpu().numpy()).all() and (host["count"] == dev["count"].cpu().numpy()).all()
        # the threshold direction
        lo, side, layers = (-4, -4), (264, 264), [(0, 256), (100, 116)]
        above = field == OFUSION
        for axis in (0, 2):
            default = p.project(axis, lo, side, layers)
            same = p.project(axis, lo, side, layers, occupied_above=above)
            _same(same, default, "explicit direction")
            flipped = p.project(axis, lo, side, layers, occupied_above=not above)
            assert (default["count"] > 0).any() and (flipped["count"] != default["count"]).any()
            # unseen does not depend on the direction: with every seen voxel occupied either way, the answers agree
            lo_thr = p.project(axis, lo, side, layers, stop_at="unseen", threshold=-1e30, occupied_above=True)
            hi_thr = p.project(axis, lo, side, layers, stop_at="unseen", threshold=1e30, occupied_above=False)
            _same(lo_thr, hi_thr, "unseen either way")
            assert (lo_thr["status"] == OCC).any() and (lo_thr["status"] == UNSEEN).any()
            # stop_at unseen counts at least what stop_at occupied counts
            unseen = p.project(axis, lo, side, layers, stop_at="unseen")
            assert (unseen["count"] >= default["count"]).all() and (unseen["count"] > default["count"]).any()
            assert (unseen["status"] == default["status"]).all()
    finally:
        p.close()


def _launches(p):
    return {k: d["launches"] for k, d in p.timings().items()}


REQ = dict(lo=(-8, 3), side=(200, 231), layers=[(0, 256), (-5, 300), (90, 106), (128, 129)])


@pytest.mark.parametrize("field", [SDF, OFUSION], ids=["sdf", "ofusion"])
def test_project_sees_the_map_of_the_frames_before_it(field):
    """On a streaming handle (scans on the side stream, raycasts held back) the answer after frame f equals the synchronous handle's; the
    calls change neither the map, the images nor the launch counters; the device entry is asynchronous and right after se_hip_sync."""
    import torch
    ans = {True: [], False: []}

    def rec(streaming):
        def check(p, f):
            ans[streaming].append([p.project(f % 3, stop_at=stop, **REQ) for stop in ("occupied", "unseen")])
        return check

    a = run_stream("room", field, 256, 2.4, 0, 4, streaming=True, check=rec(True))
    b = run_stream("room", field, 256, 2.4, 0, 4, streaming=False, check=rec(False))
    try:
        for u, w in zip(ans[True], ans[False]):
            for x, y in zip(u, w):
                _same(x, y, "streaming")
        assert (ans[False][0][0]["count"] != ans[False][3][0]["count"]).any()       # the answers follow the map (both along axis 0)
        a.enable_timing(True)
        before, la = map_state(a), _launches(a)
        for axis in (0, 1, 2):
            a.project(axis, **REQ)
            a.project(axis, stop_at="unseen", first=False, last=False, count=False, **REQ)
            a.project(axis, device=True, **REQ)
        after, lb = map_state(a), _launches(a)
        assert la == lb
        assert all((u == w).all() for u, w in zip(before, after))
        # the device entry, called directly: nothing is waited for; after se_hip_sync the arrays hold the host entry's answer
        exp = b.project(1, stop_at="unseen", **REQ)
        shape = exp["status"].shape
        dev = {k: torch.full(shape, 77, dtype=torch.uint8 if k == "status" else torch.int32, device="cuda:0") for k in OUTPUTS}
        torch.cuda.synchronize()
        rq = _request(axis=1, lo=REQ["lo"], side=REQ["side"], layers=tuple(REQ["layers"]), stop_at=1)
        out = _ProjectOut(*(dev[k].data_ptr() for k in OUTPUTS))
        assert b.lib.se_hip_project_columns(b._h, C.byref(rq), C.byref(_CollideTest(0.0, int(field == OFUSION))), C.byref(out)) == 0
        b.sync()
        _same({k: dev[k].cpu().numpy() for k in OUTPUTS}, exp, "device entry")
        tens = b.project(1, stop_at="unseen", device=True, **REQ)
        assert all(isinstance(tens[k], torch.Tensor) and tens[k].device.type == "cuda" for k in OUTPUTS)
        assert tens["status"].dtype == torch.uint8 and tens["first"].dtype == torch.int32
        _same({k: tens[k].cpu().numpy() for k in OUTPUTS}, exp, "device=True")
    finally:
        a.close(); b.close()


def test_project_between_frames_of_a_streaming_handle():
    """With frame 5's raycast held back on a streaming handle, the call flushes that raycast as a launch of its own, answers for the map with
    frame 5 fused, moves no other counter, and the image ring ends up as if the call had not been made."""
    f = 5
    got = {}

    def action(p, box):
        got["streamed"] = p.project(2, **REQ)

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
        exp = ref.project(2, **REQ)
        _same(got["streamed"], exp, "held-back raycast")
        assert (exp["count"] > 0).any()
    finally:
        ref.close()
