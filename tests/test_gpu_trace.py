"""Segment traces on the device (se_hip_trace_segments / DenseSLAMPipeline.trace): the hand-worked cases on maps built without depth (dense
and pooled, both fields); every output of every segment of the seeded set against the integer DDA over the downloaded map (two fused frames
of the golden room fixture at 80x60 into 128^3: both fields, dense and pooled, both stop_at, host and device entry, with all outputs and
without counts); the identities that tie a trace to the strict box query; view_gain against the sums of the truth; and the schedule (a
streaming handle, the map, the images, the launch counters and the timing sums left alone)."""
import ctypes as C

import numpy as np
import pytest

from supereight_amd.pipeline import (COLLISION_EMPTY, COLLISION_INVALID, COLLISION_OCCUPIED, COLLISION_UNSEEN, MOTION_FREE, OFUSION, SDF, TRACE_NONE,
                                     DenseSLAMPipeline, _CollideTest, _TraceOut, view_segments)
from tests.golden_util import load
from tests.gpu_state_util import H, W, bits, map_state, run_stream
from tests.motion_util import HAND_MAPS, class_grid, stamp_hand_map
from tests.trace_util import (FREE, HAND_CASES, KINDS, OCC, SEED, SUB, UNSEEN, census, expected_float, grids_from_octree, outputs_of,
                              seeded_segments, trace_truth)

pytestmark = pytest.mark.gpu

GOLDEN = {SDF: "sdf_80x60_128.npz", OFUSION: "ofusion_80x60_128.npz"}
LAYOUTS = [(SDF, 0), (SDF, 4096), (OFUSION, 0), (OFUSION, 4096)]
LAYOUT_IDS = ["sdf_dense", "sdf_pooled", "ofusion_dense", "ofusion_pooled"]
_shared = {}      # field -> (grid, side_of, segments, truth, kinds): computed once, shared by the tests below and left unchanged


def _same(got, want):
    return (bits(got) == bits(want)).all() if np.asarray(want).dtype == np.float32 else (np.asarray(got) == want).all()


def _golden_map(field, max_blocks, frames=2, streaming=False):
    g = load(GOLDEN[field])
    Wg, Hg, N, _ = (int(v) for v in g["dims"])
    p = DenseSLAMPipeline((Wg, Hg), N, float(g["dim"]), field_type=field, max_blocks=max_blocks, streaming=streaming)
    for f in range(frames):
        p.set_depth(g["depth"][f]); p.setPose(g["pose"][f])
        p.integration(g["k"], 1, float(g["mu"]), f)
        if streaming:
            p.raycasting_deferred(g["k"], float(g["mu"]), f)
        else:
            p.raycasting(g["k"], float(g["mu"]), f)
    return p, g, N


def _truth(p, field, N):
    """The map as downloaded, classified in numpy, and the truth of the seeded set on it (once per field: dense and pooled hold one map)."""
    grid, side_of = grids_from_octree(N, p.blocks(), p.nodes(), p.init_value(), 0.0, field == OFUSION)
    if field not in _shared:
        segs = seeded_segments(grid, SEED)
        truth, kinds = census(grid, segs, side_of)
        _shared[field] = (grid, side_of, segs, truth, kinds)
    assert (_shared[field][0] == grid).all()
    return _shared[field]


@pytest.mark.parametrize("field", [SDF, OFUSION], ids=["sdf", "ofusion"])
@pytest.mark.parametrize("max_blocks", [0, 1024], ids=["dense", "pooled"])
def test_hand_cases_on_the_device(field, max_blocks):
    occupied_x, empty_x = (-0.5, 0.5) if field == SDF else (2.0, -2.0)
    p = DenseSLAMPipeline((W, H), 64, 1.28, field_type=field, max_blocks=max_blocks)
    try:
        for mp, spec in HAND_MAPS.items():
            names = [k for k, c in HAND_CASES.items() if c[0] == mp]
            if not names:
                continue
            stamp_hand_map(p, spec, occupied_x, empty_x)
            segs = np.array([list(HAND_CASES[k][1]) + list(HAND_CASES[k][2]) for k in names], np.int32)
            for stop, col in (("occupied", 3), ("unseen", 4)):
                r = p.trace(segs, stop_at=stop)
                j = p.trace(segs, stop_at=stop, counts=False)
                for i, k in enumerate(names):
                    e_st, e_t, e_first, e_counts = HAND_CASES[k][col]
                    got = (int(r["status"][i]), tuple(r["first"][i].tolist()), tuple(r["counts"][i].tolist()))
                    assert got == (e_st, e_first, e_counts), (k, stop, got)
                    assert bits(r["t_first"][i:i + 1])[0] == bits(np.array([expected_float(e_t)]))[0], (k, stop, r["t_first"][i], e_t)
                    assert int(j["status"][i]) == e_st and tuple(j["first"][i].tolist()) == e_first and bits(j["t_first"][i:i + 1])[0] == bits(r["t_first"][i:i + 1])[0]
    finally:
        p.close()


@pytest.mark.parametrize("field,max_blocks", LAYOUTS, ids=LAYOUT_IDS)
def test_every_output_of_the_seeded_set_equals_the_truth(field, max_blocks):
    import torch
    p, g, N = _golden_map(field, max_blocks)
    try:
        grid, side_of, segs, truth, kinds = _truth(p, field, N)
        assert len(segs) % 64 != 0                                     # the last wave is ragged
        assert all(kinds[k] >= 16 for k in KINDS), kinds
        if max_blocks == 0:     # the classification in numpy is the one the established readers give
            assert (class_grid(p, N, float(g["dim"]), 0.0, field == OFUSION).cpu().numpy() == grid).all()
        dsegs = torch.from_numpy(segs).to("cuda:0")
        for s, stop in enumerate(("occupied", "unseen")):
            want = dict(zip(("status", "t_first", "first", "counts"), outputs_of(truth[s])))
            for source in (segs, dsegs):
                full = p.trace(source, stop_at=stop)
                jump = p.trace(source, stop_at=stop, counts=False)
                alone = p.trace(source, stop_at=stop, t_first=False, first=False, counts=False)
                assert sorted(full) == ["counts", "first", "status", "t_first"] and sorted(jump) == ["first", "status", "t_first"] and sorted(alone) == ["status"]
                for name, r in (("full", full), ("jump", jump), ("alone", alone)):
                    for key, arr in r.items():
                        got = arr.cpu().numpy() if source is dsegs else arr
                        assert isinstance(arr, torch.Tensor) == (source is dsegs) and got.dtype == want[key].dtype and got.shape == want[key].shape
                        same = (bits(got) == bits(want[key])) if key == "t_first" else (got == want[key])
                        bad = np.nonzero(~same.reshape(len(segs), -1).all(1))[0]
                        assert bad.size == 0, (stop, name, key, bad[:5], segs[bad[:5]], got[bad[:5]], want[key][bad[:5]])
    finally:
        p.close()


@pytest.mark.parametrize("field,max_blocks", [(SDF, 4096), (OFUSION, 0)], ids=["sdf_pooled", "ofusion_dense"])
def test_identities_with_the_box_query(field, max_blocks):
    p, g, N = _golden_map(field, max_blocks)
    try:
        _, _, segs, _, _ = _truth(p, field, N)
        for stop, code in (("occupied", COLLISION_OCCUPIED), ("unseen", COLLISION_UNSEEN)):
            r = p.trace(segs, stop_at=stop)
            blocked = (r["t_first"] >= 0) & (r["t_first"] < 1.5)               # (an invalid segment has t_first -1 and no first)
            assert blocked.sum() > 100 and ((r["first"] == TRACE_NONE).all(1) == ~blocked).all()
            cls = p.collides(np.ascontiguousarray(np.concatenate([r["first"][blocked], np.ones((int(blocked.sum()), 3), np.int32)], 1)))
            assert (cls <= code).all()
            if stop == "occupied":
                assert (cls == r["status"][blocked]).all()
        # axis-parallel, centre to centre, nothing in the way: every voxel of the run is counted, and the status is the box's
        rng = np.random.default_rng(9)
        v0 = rng.integers(-6, N + 6, (600, 3))
        v1 = v0.copy()
        axis = rng.integers(0, 3, 600)
        v1[np.arange(600), axis] = rng.integers(-6, N + 6, 600)
        runs = np.ascontiguousarray(np.concatenate([v0, v1], 1).astype(np.int32) * SUB + SUB // 2)
        r = p.trace(runs)
        free = r["t_first"] > 1.5
        lo, hi = np.minimum(v0, v1), np.maximum(v0, v1) + 1
        inside = np.prod(np.clip(np.minimum(hi, N) - np.maximum(lo, 0), 0, None), 1)
        assert free.sum() > 50 and (r["counts"].sum(1)[free] == inside[free]).all() and (inside[free] > 0).any()
        box = p.collides(np.ascontiguousarray(np.concatenate([lo, hi - lo], 1).astype(np.int32)))
        assert (r["status"][free] == box[free]).all()
        assert ((box == COLLISION_OCCUPIED) == ~free).all()
        # n == 0 and n == 1
        e = p.trace(np.zeros((0, 6), np.int32))
        assert e["status"].shape == (0,) and e["t_first"].dtype == np.float32 and e["first"].shape == (0, 3) and e["counts"].shape == (0, 2)
        one = p.trace(segs[7:8])
        full = p.trace(segs)
        assert all(_same(one[k][0], full[k][7]) for k in one)
    finally:
        p.close()


def _launches(p):
    return {k: (d["launches"], d["ms_sum"]) for k, d in p.timings().items()}


def test_a_trace_disturbs_nothing():
    import torch
    p, g, N = _golden_map(SDF, 0)
    try:
        _, _, segs, _, _ = _truth(p, SDF, N)
        p.enable_timing(True)
        before, lb, cb = map_state(p), _launches(p), p.launch_counts()
        dsegs = torch.from_numpy(segs).to("cuda:0")
        for source in (segs, dsegs):
            p.trace(source)
            p.trace(source, stop_at="unseen", counts=False)
        after, la, ca = map_state(p), _launches(p), p.launch_counts()
        assert la == lb and ca == cb
        assert all((u == w).all() for u, w in zip(before, after))
    finally:
        p.close()


def test_view_gain_equals_the_sums_of_the_truth():
    p, g, N = _golden_map(SDF, 0)
    try:
        grid = _truth(p, SDF, N)[0]
        dim, k = float(g["dim"]), g["k"]
        Wg, Hg = int(g["dims"][0]), int(g["dims"][1])
        turned = np.array(g["pose"][1], np.float64)
        turned[:3, :3] = turned[:3, :3] @ np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])      # a quarter turn about the camera's y
        outside = np.eye(4)                                                                                  # half a metre outside the volume, looking along +x into it
        outside[:3, :3] = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
        outside[:3, 3] = [-0.5, dim / 2, dim / 2]
        poses = np.stack([np.array(g["pose"][0], np.float64), turned, outside])
        want = np.zeros((3, 4), np.int64)
        for v, T in enumerate(poses):
            fan, missed = view_segments(T, k, Wg, Hg, 4, 0.4, 4.0, dim, N)
            assert len(fan) + len(missed) == 20 * 15
            for sg in fan.tolist():
                st, _, _, (cu, ce) = trace_truth(grid, sg, OCC)
                want[v] += (cu, ce, st == OCC, 1)
        assert (want[:, 3] > 0).all() and (want[:, 0] > 0).any() and (want[:, 2] > 0).any()
        got = p.view_gain(poses, k, Wg, Hg, stride=4)
        assert got.dtype == np.int64 and (got == want).all(), (got, want)
        dev = p.view_gain(poses, k, Wg, Hg, stride=4, device=True)
        assert dev.device.type == "cuda" and (dev.cpu().numpy() == want).all()
    finally:
        p.close()


@pytest.mark.parametrize("field", [SDF, OFUSION], ids=["sdf", "ofusion"])
def test_traces_see_the_frame_enqueued_just_before(field):
    """On a streaming handle (scans on the side stream, raycasts held back) the answer after frame f equals the synchronous handle's."""
    rng = np.random.default_rng(21)
    segs = np.ascontiguousarray(rng.integers(-100, 128 * SUB + 100, (1500, 6)).astype(np.int32))
    ans = {True: [], False: []}

    def rec(streaming):
        def check(p, f):
            ans[streaming].append([p.trace(segs, stop_at=s) for s in ("occupied", "unseen")])
        return check

    a = run_stream("room", field, 128, 2.4, 0, 3, streaming=True, check=rec(True))
    b = run_stream("room", field, 128, 2.4, 0, 3, streaming=False, check=rec(False))
    try:
        for u, w in zip(ans[True], ans[False]):
            assert all(_same(x[k], y[k]) for x, y in zip(u, w) for k in x)
        assert any((u[0]["status"] != w[0]["status"]).any() or (u[0]["counts"] != w[0]["counts"]).any() for u, w in zip(ans[False], ans[False][1:]))   # the answers follow the map
    finally:
        a.close(); b.close()


def test_trace_entries_refuse_bad_arguments():
    import torch
    p, _, _ = _golden_map(SDF, 0, frames=1)
    try:
        lib = p.lib
        segs = np.zeros((4, 6), np.int32)
        st, tf, fi, co = np.zeros(4, np.uint8), np.zeros(4, np.float32), np.zeros((4, 3), np.int32), np.zeros((4, 2), np.int32)
        dsg = torch.zeros((4, 6), dtype=torch.int32, device="cuda:0")
        dst, dtf = torch.zeros(4, dtype=torch.uint8, device="cuda:0"), torch.zeros(4, dtype=torch.float32, device="cuda:0")
        dfi, dco = torch.zeros((4, 3), dtype=torch.int32, device="cuda:0"), torch.zeros((4, 2), dtype=torch.int32, device="cuda:0")
        good = _CollideTest(0.0, 0)
        for fn, sa, out, no_status in ((lib.se_hip_trace_segments_host, segs.ctypes.data, _TraceOut(st.ctypes.data, tf.ctypes.data, fi.ctypes.data, co.ctypes.data),
                                        _TraceOut(None, tf.ctypes.data, None, None)),
                                       (lib.se_hip_trace_segments, dsg.data_ptr(), _TraceOut(dst.data_ptr(), dtf.data_ptr(), dfi.data_ptr(), dco.data_ptr()),
                                        _TraceOut(None, dtf.data_ptr(), None, None))):
            o = C.byref(out)
            for args in ((sa, -1, C.byref(good), 0, o), (None, 4, C.byref(good), 0, o), (sa, 4, C.byref(good), 0, C.byref(no_status)), (sa, 4, C.byref(good), 0, None),
                         (sa, 4, None, 0, o), (sa, 4, C.byref(_CollideTest(float("nan"), 0)), 0, o), (sa, 4, C.byref(_CollideTest(float("inf"), 0)), 0, o),
                         (sa, 4, C.byref(_CollideTest(0.0, 2)), 0, o), (sa, 4, C.byref(good), 2, o), (sa, 4, C.byref(good), -1, o), (sa, 4, C.byref(good), 255, o)):
                assert fn(p._h, *args) == -1
            assert fn(p._h, None, 0, C.byref(good), 0, C.byref(_TraceOut(None, None, None, None))) == 0
            assert fn(p._h, sa, 4, C.byref(good), 1, C.byref(_TraceOut(out.status, None, None, None))) == 0       # status alone
        p.sync()
        # invalid segments read nothing and say so in every output
        bad = np.array([[(1 << 22) + 1, 0, 0, 0, 0, 0], [0, 0, 0, 0, -(1 << 22) - 1, 0], [2 ** 31 - 1, 0, 0, -2 ** 31, 0, 0]], np.int32)
        r = p.trace(bad)
        assert (r["status"] == COLLISION_INVALID).all() and (r["t_first"] == -1.0).all() and (r["first"] == TRACE_NONE).all() and (r["counts"] == -1).all()
        edge = np.array([[1 << 22, 5, 5, -(1 << 22), 5, 5]], np.int32)
        assert p.trace(edge)["status"][0] != COLLISION_INVALID and p.trace(edge, stop_at="unseen")["t_first"][0] == 0.0
        assert COLLISION_EMPTY == 2 and MOTION_FREE == 2.0 and FREE == 2 and UNSEEN == COLLISION_UNSEEN
    finally:
        p.close()
