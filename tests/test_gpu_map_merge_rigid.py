"""The rigid map merge on the device (se_hip_merge_map_rigid / DenseSLAMPipeline.merge_rigid) through the C ABI, everything bit for bit: two
handles fuse different poses of the room stream, and the destination after the merge equals the numpy truth of tests/merge_rigid_util.py
computed from the two snapshots taken before -- blocks, nodes, values, flags, counts and region; the derived structures, beside a third
handle that loaded the truth from a file; the properties; the schedule; capacity; invalid arguments; fusion that goes on afterwards, against
the oracle seeded with the truth."""
import ctypes as C
import functools

import numpy as np
import pytest

from supereight_amd.pipeline import OFUSION, SDF, DenseSLAMPipeline, SeHipError, _MergeRule
from supereight_amd.synthetic import intrinsics, pose, render_depth_mm
from tests.gpu_state_util import bits, map_state
from tests.host_util import make_keys
from tests.merge_rigid_util import TRANSFORMS, case_transforms, counts_of, merge_rigid_truth, pull_of, rotation
from tests.merge_util import FUSE, MODES, unseen
from tests.shift_util import equal_blocks_nodes, leaf_level, write_map_file

pytestmark = pytest.mark.gpu
W, H = 80, 60
K = intrinsics(W)
DST_FRAMES, SRC_FRAMES = (0, 1, 2, 3), (60, 61, 62, 63)      # 12 degrees of yaw and 6 cm apart


def _dim(n):
    return 4.8 * n / 128                                      # one voxel size for every volume: 64^3 at 2.4 m, 128^3 at 4.8 m


def _mu(field):
    return 0.1 if field == SDF else 0.02


@functools.lru_cache(maxsize=None)
def _depth(f, n):
    d = np.ascontiguousarray(render_depth_mm(f, W, H, _dim(n)).astype(np.float32) / np.float32(1000.0))
    d.flags.writeable = False
    return d


def _fuse_frame(p, f, deferred=False):
    p.set_depth(_depth(f, p.size))
    p.setPose(pose(f, _dim(p.size)))
    p.integration(K, 1, _mu(p.field), f)
    (p.raycasting_deferred if deferred else p.raycasting)(K, _mu(p.field), f)


def _handle(field, n, pooled, frames=(), streaming=False, max_blocks=None):
    mb = max_blocks if max_blocks is not None else ((n // 8) ** 3 if pooled else 0)
    p = DenseSLAMPipeline((W, H), n, _dim(n), field_type=field, max_blocks=mb, streaming=streaming)
    assert ("pooled" in p.memory_info()["layout"]) == bool(mb)
    for f in frames:
        _fuse_frame(p, f)
    return p


def _state(p):
    return p.blocks(), p.nodes()


def _same(a, b):
    return all(np.asarray(u).shape == np.asarray(w).shape and (u == w).all() for u, w in zip(a, b))


def _pull(name, ssize=64, dsize=128):
    return pull_of(*case_transforms(ssize, dsize)[name])


def _merge_and_check(dst, src, pull, mode, max_weight=100):
    """dst.merge_rigid(src) against the truth computed from the two snapshots taken before; src and dst's images must not change.
    Returns (result dict, truth blocks, truth nodes, the snapshots before)."""
    db, dn = _state(dst)
    sb, sn = _state(src)
    src_before, images = map_state(src), [bits(a) for a in dst.vertex_normal()]
    want_b, want_n, want_c = merge_rigid_truth(dst.size, db, dn, src.size, sb, pull, MODES[mode], dst.field, max_weight)
    res = dst.merge_rigid(src, pull=pull, mode=mode, max_weight=max_weight)
    got_b, got_n = _state(dst)
    print(f"merge_rigid {src.size}->{dst.size} {mode} w{max_weight}: {res}; truth {want_c.tolist()}")
    assert counts_of(res).tolist() == want_c.tolist()
    assert equal_blocks_nodes(got_b, got_n, want_b, want_n) is None, equal_blocks_nodes(got_b, got_n, want_b, want_n)
    fc, fa = dst.block_flags()
    assert (fc == want_b[0]).all() and (fa == want_b[3]).all()
    assert dst.counts() == (len(want_b[0]), len(want_n[0]))
    assert _same(src_before, map_state(src))                              # src is only read
    assert _same(images, [bits(a) for a in dst.vertex_normal()])          # vertex_ / normal_ stay
    return res, want_b, want_n, (db, dn, sb, sn)


# ------------------------------------------------------------------ 1. the state equals the truth
# per layout pair the five transforms (64^3 into 128^3); field, mode and max_weight rotate so that every layout pair sees both fields, all
# three modes and every transform; then 128^3 into 64^3 once per field.
PAIRS = [(0, 0), (0, 1), (1, 0), (1, 1)]
CASES = [((SDF, OFUSION)[(i + j) % 2], dp, sp, ("fuse", "replace", "fill")[(i + j) % 3], (7, 100, 255)[(i + 2 * j) % 3], name)
         for j, (dp, sp) in enumerate(PAIRS) for i, name in enumerate(TRANSFORMS)]


def _case_id(c):
    field, dp, sp, mode, mw, name = c
    lay = lambda v: "pooled" if v else "dense"
    return f"{'sdf' if field == SDF else 'ofusion'}-{lay(dp)}-{lay(sp)}-{mode}-w{mw}-{name}"


def test_the_case_table_covers_every_factor_with_every_layout_pair():
    for pair in PAIRS:
        mine = [c for c in CASES if (c[1], c[2]) == pair]
        assert {c[0] for c in mine} == {SDF, OFUSION} and {c[3] for c in mine} == {"fuse", "replace", "fill"}
        assert {c[5] for c in mine} == set(TRANSFORMS)
    assert {c[4] for c in CASES if c[0] == SDF and c[3] == "fuse"} >= {7, 255}         # byte weights add wider than a byte


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_state_equals_the_truth(case):
    field, dp, sp, mode, mw, name = case
    dst = _handle(field, 128, dp, DST_FRAMES)
    src = _handle(field, 64, sp, SRC_FRAMES)
    try:
        if field == SDF and mode == "fuse":       # destination weights edited to 200, source weights to 100: sums beyond a byte, capped at mw
            for p, w in ((dst, 200.0), (src, 100.0)):
                assert p.edit(np.array([[0, 0, 0, p.size, p.size, p.size]], np.int32), y=w, only=("occupied", "empty"), nodes=False)[0] > 0
        res, want_b, want_n, _ = _merge_and_check(dst, src, _pull(name), mode, mw)
        if field == SDF and mode == "fuse":
            assert res["voxels_both"] >= 1 and (want_b[2] == mw).any()          # 200 + 100 gives mw, not 44
        # not vacuous
        assert res["voxels_observed"] >= 1000 and res["blocks_created"] + res["blocks_combined"] >= 8
        lo, hi = res["region"]
        assert all(0 <= a < b <= 128 for a, b in zip(lo, hi))
    finally:
        dst.close(); src.close()


@pytest.mark.parametrize("field,dp,sp,mode", [(SDF, 1, 0, "fuse"), (OFUSION, 0, 1, "replace")], ids=["sdf-pooled-dense", "ofusion-dense-pooled"])
def test_a_larger_source_is_clipped_by_the_destination(field, dp, sp, mode):
    """128^3 into 64^3 under a yaw about the source's centre: most of the source's image lies outside the destination."""
    dst = _handle(field, 64, dp, SRC_FRAMES)
    src = _handle(field, 128, sp, DST_FRAMES)
    try:
        R = rotation((0, 1, 0), 30.0)
        t = np.full(3, 31.5) - R @ np.full(3, 63.5) + np.array([10.25, -3.5, 6.125])
        res, want_b, _, _ = _merge_and_check(dst, src, pull_of(R, t), mode)
        assert res["voxels_observed"] >= 1000
    finally:
        dst.close(); src.close()


# ------------------------------------------------------------------ 2. the derived structures
def _sorted_mesh(p):
    t = np.ascontiguousarray(p.mesh()).reshape(-1, 9).view(np.uint32)
    return t[np.lexsort(t.T[::-1])]


@pytest.mark.parametrize("field,dp,sp,name", [(SDF, 0, 1, "yaw"), (SDF, 1, 0, "general"), (OFUSION, 0, 0, "general"), (OFUSION, 1, 1, "yaw")],
                         ids=["sdf-dense-pooled-yaw", "sdf-pooled-dense-general", "ofusion-dense-dense-general", "ofusion-pooled-pooled-yaw"])
def test_derived_state_equals_a_handle_that_loaded_the_truth(field, dp, sp, name, tmp_path):
    """The merged handle beside a third one that loaded the truth map from a file: a raycast taken at once, the sorted mesh, 64 box
    queries over created and combined blocks -- what occupancy bits or beam-start marks left wrong would change."""
    n = 128
    dst = _handle(field, n, dp, DST_FRAMES)
    src = _handle(field, 64, sp, SRC_FRAMES)
    third = _handle(field, n, dp)
    try:
        res, want_b, want_n, (db, dn, sb, sn) = _merge_and_check(dst, src, _pull(name), "fuse")
        path = str(tmp_path / "merged.bin")
        write_map_file(path, n, _dim(n), field, want_b, want_n)
        third.load(path)
        for p in (dst, third):
            p.setPose(pose(30, _dim(n)))
            assert p.raycasting(K, _mu(field), 30)
        va, vb = dst.vertex_normal(), third.vertex_normal()
        assert _same([bits(v) for v in va], [bits(v) for v in vb]) and (va[1][..., 0] != -2).any()
        leaf = leaf_level(n)
        dk, wk = make_keys(db[0], leaf), make_keys(want_b[0], leaf)
        new = want_b[0][~np.isin(wk, dk)]
        old = want_b[0][np.isin(wk, dk)]
        assert len(new) and len(old)
        rng = np.random.default_rng(3)
        corners = np.concatenate([c[rng.permutation(len(c))[:32]] for c in (new, old)])[:64]
        boxes = np.concatenate([corners + rng.integers(-3, 6, corners.shape), rng.integers(1, 13, corners.shape)], 1).astype(np.int32)
        for cm in ("strict", "reference"):
            ha, hb = dst.collides(boxes, mode=cm), third.collides(boxes, mode=cm)
            assert (ha == hb).all(), cm
        ma, mb = _sorted_mesh(dst), _sorted_mesh(third)
        assert ma.shape == mb.shape and (ma == mb).all() and (len(ma) > 0 or field == OFUSION)
    finally:
        dst.close(); src.close(); third.close()


# ------------------------------------------------------------------ 3. properties
@pytest.mark.parametrize("pooled", [0, 1], ids=["dense", "pooled"])
def test_merging_an_empty_source_changes_nothing(pooled):
    dst, src = _handle(SDF, 128, pooled, DST_FRAMES), _handle(SDF, 64, 1 - pooled)
    try:
        before, src_before = map_state(dst), map_state(src)
        for mode in MODES:
            res = dst.merge_rigid(src, pull=_pull("yaw"), mode=mode)
            assert counts_of(res).tolist() == [0] * 10
            assert _same(before, map_state(dst)) and _same(src_before, map_state(src))
    finally:
        dst.close(); src.close()


@pytest.mark.parametrize("field", [SDF, OFUSION], ids=["sdf", "ofusion"])
def test_fill_never_changes_an_observed_destination_voxel(field):
    dst, src = _handle(field, 128, 0, DST_FRAMES), _handle(field, 64, 0, SRC_FRAMES)
    try:
        res, want_b, want_n, (db, dn, sb, sn) = _merge_and_check(dst, src, _pull("yaw"), "fill")
        (gc, gx, gy, _), (gcode, _, gnx, gny) = _state(dst)
        leaf = leaf_level(128)
        at = np.searchsorted(make_keys(gc, leaf), make_keys(db[0], leaf))
        seen = ~unseen(db[1], db[2], field)
        assert seen.any() and (bits(gx[at])[seen] == bits(db[1])[seen]).all() and (bits(gy[at])[seen] == bits(db[2])[seen]).all()
        assert res["voxels_observed"] > res["voxels_both"] >= 1                                  # it did fill, and it did meet observed voxels
        atn = np.searchsorted(gcode, dn[0])
        assert (bits(gnx[atn]) == bits(dn[2])).all() and (bits(gny[atn]) == bits(dn[3])).all()   # node values are untouched
    finally:
        dst.close(); src.close()


# ------------------------------------------------------------------ 4. the schedule
def _streaming_handle(field, n, slots):
    import torch
    p = DenseSLAMPipeline((W, H), n, _dim(n), field_type=field, streaming=True)
    ring = torch.zeros((slots, 2, W * H * 3), dtype=torch.float32, device="cuda:0")
    p.set_image_ring(ring.data_ptr(), slots, keepalive=ring)
    return p, ring


def test_held_back_raycasts_of_both_handles_are_launched_first():
    """Both handles stream (raycasts deferred into an image ring); the merge launches the held-back raycast of either first -- the launch
    counters show exactly that and nothing else -- and the result is the truth from eager handles over the same frames."""
    pull = _pull("yaw")
    eager_d, eager_s = _handle(SDF, 128, 0, DST_FRAMES), _handle(SDF, 64, 0, SRC_FRAMES)
    want_b, want_n, want_c = merge_rigid_truth(128, *_state(eager_d), 64, eager_s.blocks(), pull, FUSE, SDF)
    eager_d.close(); eager_s.close()
    (dst, ring_d), (src, ring_s) = _streaming_handle(SDF, 128, 8), _streaming_handle(SDF, 64, 8)
    try:
        for f in DST_FRAMES:
            _fuse_frame(dst, f, deferred=True)
        for f in SRC_FRAMES:
            _fuse_frame(src, f, deferred=True)
        before = dst.launch_counts(), src.launch_counts()
        res = dst.merge_rigid(src, pull=pull)
        after = dst.launch_counts(), src.launch_counts()
        for b, a in zip(before, after):
            assert b["pending"] and not a["pending"] and a["raycast"] == b["raycast"] + 1
            assert all(a[k] == b[k] for k in a if k not in ("raycast", "pending", "alloc_commit")), (b, a)
        assert counts_of(res).tolist() == want_c.tolist()
        assert equal_blocks_nodes(*_state(dst), want_b, want_n) is None
        dst.sync(); src.sync()
        assert ring_d.cpu().numpy()[DST_FRAMES[-1] % 8].any() and ring_s.cpu().numpy()[SRC_FRAMES[-1] % 8].any()
        assert dst.launch_counts() == after[0]
    finally:
        dst.close(); src.close()


def test_a_scan_pending_on_the_side_stream_is_joined():
    """alloc_scan leaves the allocation scan of the next frame on the side stream, on both handles; the merge joins them: the result is the
    truth from twin handles whose scans were joined by the snapshot."""
    pull = _pull("general")

    def scanned(n, frames, nxt):
        p = _handle(SDF, n, 0, frames)
        p.set_depth(_depth(nxt, n)); p.setPose(pose(nxt, _dim(n)))
        nb = p.counts()[0]
        assert p.alloc_scan(K, 1, _mu(SDF), nxt)
        return p, nb
    (twin_d, nd), (twin_s, ns) = scanned(128, DST_FRAMES, 20), scanned(64, SRC_FRAMES, 90)
    want_b, want_n, want_c = merge_rigid_truth(128, *_state(twin_d), 64, twin_s.blocks(), pull, FUSE, SDF)
    assert twin_d.counts()[0] > nd and twin_s.counts()[0] > ns          # the scans did insert blocks
    twin_d.close(); twin_s.close()
    (dst, _), (src, _) = scanned(128, DST_FRAMES, 20), scanned(64, SRC_FRAMES, 90)
    try:
        res = dst.merge_rigid(src, pull=pull)
        assert counts_of(res).tolist() == want_c.tolist()
        assert equal_blocks_nodes(*_state(dst), want_b, want_n) is None
    finally:
        dst.close(); src.close()


def test_tracking_goes_on_and_no_launch_counter_moves():
    dst, src = _handle(SDF, 128, 0, DST_FRAMES), _handle(SDF, 64, 1, SRC_FRAMES)
    try:
        dst.enable_timing(True)
        dst.timings(reset=True)
        before = dst.launch_counts(), src.launch_counts()
        dst.merge_rigid(src, pull=_pull("yaw"))
        assert (dst.launch_counts(), src.launch_counts()) == before
        assert all(v["launches"] == 0 and v["ms_sum"] == 0 for v in dst.timings().values())
        dst.set_depth(_depth(4, 128)); dst.setPose(pose(4, _dim(128)))
        assert dst.tracking(K, 1e-5, 1, 4)
        assert np.isfinite(dst.pose_).all()
    finally:
        dst.close(); src.close()


# ------------------------------------------------------------------ 5. capacity
def test_a_pool_a_few_bricks_short_reports_capacity():
    """The pooled destination holds its own blocks and eight more; the merge wants more than that.  The call returns SE_HIP_E_CAPACITY
    (sticky, as from every other insertion); the blocks that did fit equal the truth restricted to them, the others were skipped."""
    n, pull = 128, _pull("general")
    probe = _handle(SDF, n, 1, DST_FRAMES)
    nb = probe.counts()[0]
    probe.close()
    dst, src = _handle(SDF, n, 1, DST_FRAMES, max_blocks=nb + 8), _handle(SDF, 64, 0, SRC_FRAMES)
    try:
        assert dst.counts()[0] == nb and dst.memory_info()["brick_slots"] == nb + 8
        want_b, want_n, want_c = merge_rigid_truth(n, *_state(dst), 64, src.blocks(), pull, FUSE, SDF)
        assert want_c[1] > 8
        src_before = map_state(src)
        with pytest.raises(SeHipError, match="pool exhausted"):
            dst.merge_rigid(src, pull=pull)
        assert dst.clear_overflow() != 0
        assert dst.counts()[0] == nb + 8                        # the pool is full, not overrun
        gc, gx, gy, ga = dst.blocks()
        leaf = leaf_level(n)
        gk, wk = make_keys(gc, leaf), make_keys(want_b[0], leaf)
        assert len(gc) == nb + 8 and np.isin(gk, wk).all()
        at = np.searchsorted(wk, gk)
        assert (bits(gx) == bits(want_b[1][at])).all() and (bits(gy) == bits(want_b[2][at])).all() and (ga == want_b[3][at]).all()
        assert _same(src_before, map_state(src))
        # a source whose own pool overflowed is refused
        small = _handle(SDF, 64, 1, max_blocks=8)
        try:
            small.set_depth(_depth(60, 64)); small.setPose(pose(60, _dim(64)))
            try:
                small.integration(K, 1, _mu(SDF), 60)
                small.sync()
            except SeHipError:
                pass
            before = map_state(dst)
            out = np.full(10, 77, np.int64)
            rule = _MergeRule(0, 100.0)
            assert dst.lib.se_hip_merge_map_rigid(dst._h, small._h, pull.ctypes.data, C.addressof(rule), out.ctypes.data) == -3      # SE_HIP_E_CAPACITY
            assert (out == 77).all() and _same(before, map_state(dst))
        finally:
            small.close()
    finally:
        dst.close(); src.close()


# ------------------------------------------------------------------ 6. invalid arguments
def test_invalid_arguments_are_refused_and_change_nothing():
    dst, src = _handle(SDF, 128, 0, DST_FRAMES), _handle(SDF, 64, 1, SRC_FRAMES)
    other_field, other_voxel = _handle(OFUSION, 64, 0), DenseSLAMPipeline((W, H), 64, 4.8, field_type=SDF)
    try:
        before = map_state(dst), map_state(src)
        out = np.full(10, 77, np.int64)
        lib, ok_rule, ok = dst.lib, _MergeRule(0, 100.0), _pull("yaw")

        def call(d, s_, pull, rule):
            return lib.se_hip_merge_map_rigid(d._h, s_._h, pull.ctypes.data if pull is not None else None,
                                              C.addressof(rule) if rule is not None else None, out.ctypes.data)

        def with_entry(i, v):
            p = ok.copy()
            p[i] = v
            return p
        assert call(dst, dst, ok, ok_rule) == -1 and "dst == src" in lib.se_hip_last_error().decode()
        assert call(dst, other_field, ok, ok_rule) == -1 and "field" in lib.se_hip_last_error().decode()
        assert call(dst, other_voxel, ok, ok_rule) == -1 and "voxel" in lib.se_hip_last_error().decode()
        off = (ok.reshape(3, 4) * np.array([1.005, 1.005, 1.005, 1.0], np.float32)).reshape(12).copy()          # R^T R - I = 1e-2
        bad = [with_entry(5, np.nan), with_entry(3, np.inf), with_entry(11, -np.inf), with_entry(7, 2.0 ** 20 + 1), with_entry(3, -2.0 ** 20 - 1),
               off, pull_of(np.diag([1.0, 1.0, -1.0]), np.zeros(3)), np.zeros(12, np.float32)]
        for p in bad:
            assert call(dst, src, p, ok_rule) == -1, p
            assert "se_hip_merge_map_rigid" in lib.se_hip_last_error().decode()
        assert call(dst, src, None, ok_rule) == -1
        assert call(dst, src, ok, None) == -1
        for mode, mw in [(3, 100.0), (-1, 100.0), (0, 0.0), (0, 256.0), (0, 99.5), (0, float("nan")), (0, -1.0), (0, float("inf"))]:
            assert call(dst, src, ok, _MergeRule(mode, mw)) == -1, (mode, mw)
        assert lib.se_hip_merge_map_rigid(None, src._h, ok.ctypes.data, C.addressof(ok_rule), out.ctypes.data) == -1
        assert lib.se_hip_merge_map_rigid(dst._h, None, ok.ctypes.data, C.addressof(ok_rule), out.ctypes.data) == -1
        assert (out == 77).all() and _same(before[0], map_state(dst)) and _same(before[1], map_state(src))
        nearly = (ok.reshape(3, 4).astype(np.float64) * np.array([1 + 5e-6, 1 + 5e-6, 1 + 5e-6, 1.0])).astype(np.float32).reshape(12).copy()
        assert lib.se_hip_merge_map_rigid(dst._h, src._h, nearly.ctypes.data, C.addressof(_MergeRule(2, 255.0)), None) == 0      # 1e-5 off; counts are optional
        far = with_entry(3, 2.0 ** 20)
        assert call(dst, src, far, _MergeRule(1, 1.0)) == 0 and (out == 0).all()           # the limit itself: nothing in reach
    finally:
        for p in (dst, src, other_field, other_voxel):
            p.close()


# ------------------------------------------------------------------ 7. fusion goes on
@pytest.mark.parametrize("field,dp", [(SDF, 1), (OFUSION, 0)], ids=["sdf-pooled", "ofusion-dense"])
def test_integration_after_a_merge_equals_the_oracle_on_the_loaded_truth(field, dp):
    """Two more frames after a `yaw` FUSE: the oracle, seeded with the truth map (insert_octants, set_values, activate), integrates and
    raycasts the same frames; maps and images stay equal, bit for bit.  (A seeded oracle holds every block active; the first sweep visits
    the extra ones, changes nothing and clears their flags: flags are compared after each frame.)"""
    from oracle.binding import OraclePipeline
    n = 128
    dst, src = _handle(field, n, dp, DST_FRAMES), _handle(field, 64, 1 - dp, SRC_FRAMES)
    cpu = OraclePipeline(field, n, _dim(n), W, H)
    try:
        res, want_b, want_n, _ = _merge_and_check(dst, src, _pull("yaw"), "fuse")
        coords, x, y, act = want_b
        code, side, nx, ny = want_n
        cpu.insert_octants(np.concatenate([code[(code & np.uint64(0x1FF)) > 0], make_keys(coords, leaf_level(n))]).astype(np.uint64))
        assert cpu.counts() == (len(coords), len(code))
        assert cpu.set_values(blocks=(coords, x, y), nodes=(code, side, nx, ny)) == (len(coords), len(code))
        cpu.activate(coords[act != 0])
        k = np.ascontiguousarray(K, np.float32)
        for f in (4, 5):
            _fuse_frame(dst, f)
            assert cpu.integrate(_depth(f, n), pose(f, _dim(n)), k, _mu(field), f)
            _, v, nrm = cpu.raycast(pose(f, _dim(n)), k, _mu(field), f)
            assert equal_blocks_nodes(*_state(dst), cpu.blocks(), cpu.nodes()) is None, (f, equal_blocks_nodes(*_state(dst), cpu.blocks(), cpu.nodes()))
            gv, gn = dst.vertex_normal()
            assert (bits(gv).reshape(-1) == bits(v).reshape(-1)).all() and (bits(gn).reshape(-1) == bits(nrm).reshape(-1)).all()
            assert (nrm[..., 0] != -2).any()
    finally:
        dst.close(); src.close(); cpu.close()
