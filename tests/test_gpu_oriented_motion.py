"""Oriented motion collision queries on the device (se_hip_collide_oriented_motions / DenseSLAMPipeline.collides_oriented_moving): the
hand-worked cases on maps built without depth (dense and pooled, both fields, host and device entry); status, t_exact and the bits of t_first
of the seeded set against the definition evaluated in numpy over the downloaded map (three fused frames of the golden room fixture at 80x60
into 128^3: both fields, dense and pooled, both stop_at, both entries); the identities that tie the query to collides_oriented, collides_moving
and collides; invalid rows and empty batches; the refusals of the C entries; and the schedule (a streaming handle, the map, the images and
the launch counters left alone).  Every comparison is equality."""
import ctypes as C

import numpy as np
import pytest

from supereight_amd.pipeline import (COLLISION_INVALID, COLLISION_OCCUPIED, COLLISION_UNSEEN, MOTION_FREE, OFUSION, SDF, DenseSLAMPipeline,
                                     _CollideTest, _OrientedMotionOut)
from tests import motion_util
from tests.golden_util import load
from tests.gpu_state_util import H, W, bits, map_state
from tests.motion_util import class_grid
from tests.oriented_motion_util import (HAND_CASES, HAND_MAP_NAMES, OCC, SEED, aligned_hand_cases, aligned_motions, bounding_motion_boxes, census,
                                        expected_float, from_aligned, hand_motions, motion_hand_grid, oriented_motion_truth, outputs_of,
                                        reversed_motions, seeded_motions, shortened, shuffled_axes, stamp_motion_map)
from tests.trace_util import grids_from_octree

pytestmark = pytest.mark.gpu

GOLDEN = {SDF: "sdf_80x60_128.npz", OFUSION: "ofusion_80x60_128.npz"}
LAYOUTS = [(SDF, 0), (SDF, 4096), (OFUSION, 0), (OFUSION, 4096)]
LAYOUT_IDS = ["sdf_dense", "sdf_pooled", "ofusion_dense", "ofusion_pooled"]
STOPS = (("occupied", COLLISION_OCCUPIED), ("unseen", COLLISION_UNSEEN))
_shared = {}      # field -> (grid, motions, truth): computed once, shared by the tests below and left unchanged


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _check(got, want, rows, what):
    """status, t_first (bit for bit) and t_exact of a call against the arrays of the truth."""
    st, tf, te = (_np(a) for a in got)
    assert st.dtype == np.uint8 and tf.dtype == np.float32 and te.dtype == np.int64 and te.shape == (len(rows), 2)
    same = (st == want[0]) & (bits(tf) == bits(want[1])) & (te == want[2]).all(1)
    bad = np.nonzero(~same)[0]
    assert bad.size == 0, (what, bad[:5], rows[bad[:5]], st[bad[:5]], want[0][bad[:5]], te[bad[:5]], want[2][bad[:5]], tf[bad[:5]], want[1][bad[:5]])


@pytest.mark.parametrize("field", [SDF, OFUSION], ids=["sdf", "ofusion"])
@pytest.mark.parametrize("max_blocks", [0, 1024], ids=["dense", "pooled"])
def test_hand_cases_on_the_device(field, max_blocks):
    import torch
    occupied_x, empty_x = (-0.5, 0.5) if field == SDF else (2.0, -2.0)
    aligned = aligned_hand_cases()
    for mp in HAND_MAP_NAMES + tuple(sorted({c[0] for c in aligned.values()} - set(HAND_MAP_NAMES))):
        p = DenseSLAMPipeline((W, H), 64, 1.28, field_type=field, max_blocks=max_blocks)
        try:
            stamp_motion_map(p, mp, occupied_x, empty_x)
            assert (class_grid(p, 64, 1.28, 0.0, field == OFUSION).cpu().numpy() == motion_hand_grid(mp)).all()
            names = [k for k, c in HAND_CASES.items() if c[0] == mp]
            also = [k for k, c in aligned.items() if c[0] == mp]
            rows = np.concatenate([hand_motions(names).reshape(-1, 15), np.array([aligned[k][1] for k in also], np.int64).astype(np.int32).reshape(-1, 15)])
            answers = [HAND_CASES[k][4:6] for k in names] + [aligned[k][2:4] for k in also]
            for s, (stop, _) in enumerate(STOPS):
                want = (np.array([a[s][0] for a in answers], np.uint8), np.array([expected_float(a[s][1]) for a in answers], np.float32),
                        np.array([[a[s][1].numerator, a[s][1].denominator] for a in answers], np.int64))
                _check(p.collides_oriented_moving(rows, stop_at=stop, exact=True), want, rows, (mp, stop, "host", names + also))
                _check(p.collides_oriented_moving(torch.from_numpy(rows).to("cuda:0"), stop_at=stop, exact=True), want, rows, (mp, stop, "device"))
                assert (p.collides_oriented_moving(rows, stop_at=stop, t_first=False) == want[0]).all()
                if also:        # the axis-aligned rows, asked as collides_moving asks them: the same status and the same float
                    m9 = np.array([list(motion_util.HAND_CASES[k][1]) + list(motion_util.HAND_CASES[k][2]) + list(motion_util.HAND_CASES[k][3]) for k in also],
                                  np.int64).astype(np.int32)
                    st9, t9 = p.collides_moving(m9, stop_at=stop)
                    assert (st9 == want[0][len(names):]).all() and (bits(t9) == bits(want[1][len(names):])).all()
        finally:
            p.close()


def _golden_map(field, max_blocks, frames=3, streaming=False, check=None):
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
        if check is not None:
            check(p, f)
    return p, g, N


def _truth(p, field, N):
    """The map as downloaded, classified in numpy, and the truth of the seeded set on it (once per field: dense and pooled hold one map)."""
    grid, _ = grids_from_octree(N, p.blocks(), p.nodes(), p.init_value(), 0.0, field == OFUSION)
    if field not in _shared:
        mo = seeded_motions(grid, SEED)
        _shared[field] = (grid, mo, [oriented_motion_truth(grid, m) for m in mo.tolist()])
    assert (_shared[field][0] == grid).all()
    return _shared[field]


@pytest.mark.parametrize("field,max_blocks", LAYOUTS, ids=LAYOUT_IDS)
def test_seeded_set_equals_the_definition(field, max_blocks):
    import torch
    p, g, N = _golden_map(field, max_blocks)
    try:
        grid, mo, truth = _truth(p, field, N)
        assert len(mo) == 300 and len(mo) % 64 != 0                    # the last wave of a grid-stride pass would be ragged
        kinds = census(truth)
        print(kinds)
        # by the truth alone: every class, both stop_at with different answers, blocked at the start, free, and strictly between
        assert all(v >= 16 for v in kinds.values()), kinds
        if max_blocks == 0:     # the classification in numpy is the one the established readers give
            assert (class_grid(p, N, float(g["dim"]), 0.0, field == OFUSION).cpu().numpy() == grid).all()
        dmo = torch.from_numpy(mo).to("cuda:0")
        for s, (stop, _) in enumerate(STOPS):
            want = outputs_of(truth, s)
            for source in (mo, dmo):
                full = p.collides_oriented_moving(source, stop_at=stop, exact=True)
                assert all(isinstance(a, torch.Tensor) == (source is dmo) for a in full)
                _check(full, want, mo, (stop, "device" if source is dmo else "host"))
                st, tf = p.collides_oriented_moving(source, stop_at=stop)
                assert (_np(st) == want[0]).all() and (bits(_np(tf)) == bits(want[1])).all()
                st, te = p.collides_oriented_moving(source, stop_at=stop, t_first=False, exact=True)
                assert (_np(st) == want[0]).all() and (_np(te) == want[2]).all()
                assert (_np(p.collides_oriented_moving(source, stop_at=stop, t_first=False)) == want[0]).all()
    finally:
        p.close()


@pytest.mark.parametrize("field,max_blocks", [(SDF, 4096), (OFUSION, 0)], ids=["sdf_pooled", "ofusion_dense"])
def test_identities_with_the_other_readers(field, max_blocks):
    p, g, N = _golden_map(field, max_blocks)
    try:
        _, mo, truth = _truth(p, field, N)
        rng = np.random.default_rng(12)
        # d = 0 is the static query
        still = mo.copy()
        still[:, 12:15] = 0
        st0, t0 = p.collides_oriented_moving(still)
        static = p.collides_oriented(np.ascontiguousarray(still[:, :12]))
        assert (st0 == static).all() and {0, 1, 2} <= set(static.tolist())
        assert ((t0 == 0) == (static == COLLISION_OCCUPIED)).all() and ((t0 == MOTION_FREE) == (static != COLLISION_OCCUPIED)).all()
        # aligned boxes moved by whole voxels are collides_moving's, bit for bit
        _, m9 = aligned_motions(rng, 400, N)
        near = np.argwhere(_shared[field][0] == OCC)[:, ::-1]
        m9[:200, 0:3] = near[rng.integers(0, len(near), 200)] + rng.integers(-8, 4, (200, 3))
        om = np.array([from_aligned(r) for r in m9.tolist()], np.int64).astype(np.int32)
        for stop, _ in STOPS:
            sa, ta = p.collides_oriented_moving(om, stop_at=stop)
            s9, t9 = p.collides_moving(m9, stop_at=stop)
            assert (sa == s9).all() and (bits(ta) == bits(t9)).all()
            assert ((t9 > 0) & (t9 < 1)).sum() >= 10 and (t9 == 0).any() and (t9 == MOTION_FREE).any()
        for s, (stop, code) in enumerate(STOPS):
            want = outputs_of(truth, s)
            # permuting and negating the half-axes changes nothing
            _check(p.collides_oriented_moving(shuffled_axes(rng, mo), stop_at=stop, exact=True), want, mo, (stop, "shuffled"))
            # the reversed motion sweeps the same set
            assert (p.collides_oriented_moving(reversed_motions(mo), stop_at=stop, t_first=False) == want[0]).all()
            # moving only as far as t_exact is free
            idx, cut = shortened(mo, want[2])
            assert len(idx) >= 16
            sc, tc = p.collides_oriented_moving(cut, stop_at=stop)
            assert (tc == MOTION_FREE).all() and (sc > code).all()
        # the bounding box of the sweep sees at least as much
        bound = p.collides(bounding_motion_boxes(mo))
        status = outputs_of(truth, 0)[0]
        assert (bound <= status).all() and (bound < status).any()
    finally:
        p.close()


def test_invalid_rows_and_empty_batches():
    import torch
    p, g, N = _golden_map(SDF, 0, frames=1)
    try:
        I32, MX, CL, HL, ML = -(1 << 31), 2 ** 31 - 1, 1 << 20, 1 << 14, 1 << 18
        r = [4, 3, 0, -3, 4, 0, 0, 0, 5]
        bad = np.array([[100, 100, 100] + r + [ML + 1, 0, 0], [100, 100, 100] + r + [0, -ML - 1, 0], [CL - 10, 0, 0] + r + [11, 0, 0], [0, 0, -CL + 10] + r + [0, 0, -11],
                        [100, 100, 100, 8, 8, 0, 1, 0, 0, 8, 8, 0, 16, 0, 0], [100, 100, 100, 0, 0, 0, 0, 8, 0, 0, 0, 8, 0, 0, 0], [CL + 1, 0, 0] + r + [-5, 0, 0],
                        [100, 100, 100, HL + 1, 0, 0, 0, 8, 0, 0, 0, 8, 0, 0, 0], [100, 100, 100] + r + [I32, I32, I32], [100, 100, 100] + r + [MX, 0, 0],
                        [I32, 100, 100] + r + [I32, 0, 0], [I32] * 15, [MX] * 15, [0] * 15], np.int64).astype(np.int32)
        edge = np.array([[100, 100, 100] + r + [ML, 0, 0], [100, 100, 100] + r + [0, 0, -ML], [CL - 11, 100, 100] + r + [11, 0, 0], [-CL + 11, 100, 100] + r + [-11, 0, 0],
                         [1024, 1024, 1024, HL, 0, 0, 0, HL, 0, 0, 0, HL, ML, -ML, ML]], np.int64).astype(np.int32)
        rows = np.ascontiguousarray(np.concatenate([bad, edge]))
        for source in (rows, torch.from_numpy(rows).to("cuda:0")):
            for stop, _ in STOPS:
                st, tf, te = (_np(a) for a in p.collides_oriented_moving(source, stop_at=stop, exact=True))
                k = len(bad)
                assert (st[:k] == COLLISION_INVALID).all() and (tf[:k] == -1.0).all() and (te[:k] == [-1, 1]).all()
                assert (st[k:] != COLLISION_INVALID).all() and (tf[k:] >= 0).all() and (te[k:, 1] >= 1).all() and (st[k:] <= COLLISION_UNSEEN).all()
        for empty in (np.zeros((0, 15), np.int32), torch.zeros((0, 15), dtype=torch.int32, device="cuda:0")):
            st, tf, te = p.collides_oriented_moving(empty, exact=True)
            assert tuple(st.shape) == (0,) and tuple(tf.shape) == (0,) and tuple(te.shape) == (0, 2)
    finally:
        p.close()


def _launches(p):
    return {k: d["launches"] for k, d in p.timings().items()}


@pytest.mark.parametrize("field", [SDF, OFUSION], ids=["sdf", "ofusion"])
def test_motions_see_the_map_of_the_frames_before_them(field):
    """On a streaming handle (scans on the side stream, raycasts held back) the answer after frame f equals the synchronous handle's: a scan
    still pending on the side stream is joined first.  The calls change neither the map, the images nor the launch counters."""
    g = load(GOLDEN[field])
    N = int(g["dims"][2])
    rng = np.random.default_rng(29)
    mo = seeded_motions(np.where(rng.random((N, N, N)) < 0.5, np.uint8(0), np.uint8(2)), 2, 256)      # anywhere in the volume, whatever the map
    ans = {True: [], False: []}

    def rec(streaming):
        def check(p, f):
            ans[streaming].append(p.collides_oriented_moving(mo, exact=True))
        return check

    a, _, _ = _golden_map(field, 0, frames=4, streaming=True, check=rec(True))
    b, _, _ = _golden_map(field, 0, frames=4, streaming=False, check=rec(False))
    try:
        for u, w in zip(ans[True], ans[False]):
            assert (u[0] == w[0]).all() and (bits(u[1]) == bits(w[1])).all() and (u[2] == w[2]).all()
        assert any((u[0] != w[0]).any() for u, w in zip(ans[False], ans[False][1:]))       # the answers follow the map
        a.enable_timing(True)
        before, la, ca = map_state(a), _launches(a), a.launch_counts()
        for stop, _ in STOPS:
            a.collides_oriented_moving(mo, stop_at=stop, exact=True)
            a.collides_oriented_moving(mo, stop_at=stop, t_first=False)
        after, lb, cb = map_state(a), _launches(a), a.launch_counts()
        assert la == lb and ca == cb
        assert all((u == w).all() for u, w in zip(before, after))
    finally:
        a.close(); b.close()


def test_entries_refuse_bad_arguments():
    import torch
    p, g, N = _golden_map(SDF, 0, frames=1)
    try:
        lib = p.lib
        mo = np.tile(np.array([[1000, 1000, 1000, 8, 0, 0, 0, 8, 0, 0, 0, 8, 40, 20, -10]], np.int32), (4, 1))
        st, tf, te = np.zeros(4, np.uint8), np.zeros(4, np.float32), np.zeros((4, 2), np.int64)
        dmo = torch.from_numpy(mo).to("cuda:0")
        dst, dtf, dte = (torch.zeros(4, dtype=torch.uint8, device="cuda:0"), torch.zeros(4, dtype=torch.float32, device="cuda:0"),
                         torch.zeros((4, 2), dtype=torch.int64, device="cuda:0"))
        good = _CollideTest(0.0, 0)
        for fn, ma, out, no_status in ((lib.se_hip_collide_oriented_motions_host, mo.ctypes.data, _OrientedMotionOut(st.ctypes.data, tf.ctypes.data, te.ctypes.data),
                                        _OrientedMotionOut(None, tf.ctypes.data, te.ctypes.data)),
                                       (lib.se_hip_collide_oriented_motions, dmo.data_ptr(), _OrientedMotionOut(dst.data_ptr(), dtf.data_ptr(), dte.data_ptr()),
                                        _OrientedMotionOut(None, dtf.data_ptr(), dte.data_ptr()))):
            for args in ((ma, -1, C.byref(good), 0, C.byref(out)), (None, 4, C.byref(good), 0, C.byref(out)), (ma, 4, C.byref(good), 0, C.byref(no_status)),
                         (ma, 4, C.byref(good), 0, None), (ma, 4, None, 0, C.byref(out)), (ma, 4, C.byref(_CollideTest(float("nan"), 0)), 0, C.byref(out)),
                         (ma, 4, C.byref(_CollideTest(float("inf"), 0)), 0, C.byref(out)), (ma, 4, C.byref(_CollideTest(0.0, 2)), 0, C.byref(out)),
                         (ma, 4, C.byref(_CollideTest(0.0, -1)), 0, C.byref(out)), (ma, 4, C.byref(good), 2, C.byref(out)), (ma, 4, C.byref(good), -1, C.byref(out)),
                         (ma, 4, C.byref(good), 255, C.byref(out))):
                assert fn(p._h, *args) == -1
            assert fn(p._h, None, 0, C.byref(good), 0, C.byref(_OrientedMotionOut(None, None, None))) == 0
            assert fn(p._h, ma, 4, C.byref(good), 1, C.byref(out)) == 0
        p.sync()
        assert (st == dst.cpu().numpy()).all() and (st != COLLISION_INVALID).all()
        assert (bits(tf) == bits(dtf.cpu().numpy())).all() and (te == dte.cpu().numpy()).all() and (te[:, 1] >= 1).all()
    finally:
        p.close()
