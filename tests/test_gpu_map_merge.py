"""The map merge on the device (se_hip_merge_map / DenseSLAMPipeline.merge) through the C ABI, everything bit for bit: two handles fuse
different poses of the room stream (their block sets overlap, neither contains the other), and the destination after the merge equals the
numpy truth of tests/merge_util.py computed from the two snapshots taken before -- blocks, nodes, flags, counts and region; the derived
structures, beside a third handle that loaded the truth from a file; the properties; the schedule; capacity; invalid arguments."""
import ctypes as C

import numpy as np
import pytest

from supereight_amd.pipeline import OFUSION, SDF, DenseSLAMPipeline, SeHipError, _MergeRule
from supereight_amd.synthetic import intrinsics, pose, render_depth_mm
from tests.gpu_state_util import bits, map_state
from tests.host_util import LIMIT, make_keys
from tests.merge_util import FUSE, MODES, both_observed, counts_of, merge_truth, unseen
from tests.shift_util import equal_blocks_nodes, leaf_level, write_map_file

pytestmark = pytest.mark.gpu
W, H = 80, 60
K = intrinsics(W)
DST_FRAMES, SRC_FRAMES = (0, 1, 2, 3), (60, 61, 62, 63)      # 12 degrees of yaw and 6 cm apart


def _dim(n):
    return 4.8 * n / 128                                      # one voxel size for every volume: 64^3 at 2.4 m, 128^3 at 4.8 m


def _mu(field):
    return 0.1 if field == SDF else 0.02


def _depth(f, n):
    return np.ascontiguousarray(render_depth_mm(f, W, H, _dim(n)).astype(np.float32) / np.float32(1000.0))


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


def _merge_and_check(dst, src, s, mode, max_weight=100):
    """dst.merge(src) against the truth computed from the two snapshots taken before; src and dst's images must not change.
    Returns (result dict, truth blocks, truth nodes, the snapshots before)."""
    db, dn = _state(dst)
    sb, sn = _state(src)
    src_before, images = map_state(src), [bits(a) for a in dst.vertex_normal()]
    want_b, want_n, want_c = merge_truth(dst.size, db, dn, src.size, sb, sn, s, MODES[mode], dst.field, max_weight)
    res = dst.merge(src, s, mode=mode, max_weight=max_weight)
    got_b, got_n = _state(dst)
    print(f"merge {src.size}->{dst.size} s={s} {mode}: {res}; both observed {both_observed(dst.size, db, src.size, sb, s, dst.field)}")
    assert equal_blocks_nodes(got_b, got_n, want_b, want_n) is None, equal_blocks_nodes(got_b, got_n, want_b, want_n)
    fc, fa = dst.block_flags()
    assert (fc == want_b[0]).all() and (fa == want_b[3]).all()
    assert counts_of(res).tolist() == want_c.tolist()
    assert dst.counts() == (len(want_b[0]), len(want_n[0]))
    assert _same(src_before, map_state(src))                              # src is only read
    assert _same(images, [bits(a) for a in dst.vertex_normal()])          # vertex_ / normal_ stay
    return res, want_b, want_n, (db, dn, sb, sn)


# ------------------------------------------------------------------ 1. the state equals the truth
# per layout pair five cases: the four shifts at equal sizes and 64^3 into 128^3; field and mode rotate so that every layout pair sees both
# fields and all three modes.  (-16, 16, 0) clips the source's left wall; (64, 0, 0) and (32, 32, 64) are aligned to nodes.
SHIFTS = [(128, (0, 0, 0)), (128, (8, 0, -16)), (128, (64, 0, 0)), (128, (-16, 16, 0)), (64, (32, 32, 64))]
CLIPPING = (-16, 16, 0)
PAIRS = [(0, 0), (0, 1), (1, 0), (1, 1)]
CASES = [((SDF, OFUSION)[(i + j) % 2], dp, sp, ("fuse", "replace", "fill")[(i + j) % 3], ssize, s)
         for j, (dp, sp) in enumerate(PAIRS) for i, (ssize, s) in enumerate(SHIFTS)]


def _case_id(c):
    field, dp, sp, mode, ssize, s = c
    lay = lambda v: "pooled" if v else "dense"
    return f"{'sdf' if field == SDF else 'ofusion'}-{lay(dp)}-{lay(sp)}-{mode}-{ssize}-{'_'.join(str(v) for v in s)}"


def test_the_case_table_covers_every_factor_with_every_layout_pair():
    for pair in PAIRS:
        mine = [c for c in CASES if (c[1], c[2]) == pair]
        assert {c[0] for c in mine} == {SDF, OFUSION} and {c[3] for c in mine} == {"fuse", "replace", "fill"}
        assert {(c[4], c[5]) for c in mine} == set(SHIFTS)


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_state_equals_the_truth(case):
    field, dp, sp, mode, ssize, s = case
    dst = _handle(field, 128, dp, DST_FRAMES)
    src = _handle(field, ssize, sp, SRC_FRAMES)
    try:
        res, want_b, want_n, (db, dn, sb, sn) = _merge_and_check(dst, src, s, mode)
        # not vacuous
        assert res["blocks_combined"] >= 1 and res["blocks_created"] >= 1
        assert both_observed(128, db, ssize, sb, s, field) >= 1
        if s == CLIPPING:
            assert res["blocks_clipped"] >= 1
        if all(v % 16 == 0 for v in s):
            assert res["nodes_combined"] >= 1                 # (a shift that no node side divides -- (8, 0, -16) -- skips every node, by definition)
        else:
            assert res["nodes_combined"] == 0 and res["nodes_skipped"] == len(sn[0])
        lo, hi = res["region"]
        assert all(0 <= a < b <= 128 for a, b in zip(lo, hi))
    finally:
        dst.close(); src.close()


# ------------------------------------------------------------------ 2. the derived structures
def _sorted_mesh(p):
    t = np.ascontiguousarray(p.mesh()).reshape(-1, 9).view(np.uint32)
    return t[np.lexsort(t.T[::-1])]


@pytest.mark.parametrize("field,dp,sp", [(SDF, 0, 1), (SDF, 1, 0), (OFUSION, 0, 0), (OFUSION, 1, 1)],
                         ids=["sdf-dense-pooled", "sdf-pooled-dense", "ofusion-dense-dense", "ofusion-pooled-pooled"])
def test_derived_state_equals_a_handle_that_loaded_the_truth(field, dp, sp, tmp_path):
    """The merged handle beside a third one that loaded the truth map from a file (the existing file route): raycast images, collides on
    boxes over old, created and combined blocks, the mesh; then one further frame on both, and the maps again."""
    s, mode, n = (8, 0, -16), "fuse", 128
    dst = _handle(field, n, dp, DST_FRAMES)
    src = _handle(field, n, sp, SRC_FRAMES)
    third = _handle(field, n, dp)
    try:
        res, want_b, want_n, (db, dn, sb, sn) = _merge_and_check(dst, src, s, mode)
        path = str(tmp_path / "merged.bin")
        write_map_file(path, n, _dim(n), field, want_b, want_n)
        third.load(path)
        got_b, got_n = _state(third)
        assert equal_blocks_nodes((got_b[0], got_b[1], got_b[2], want_b[3]), got_n, want_b, want_n) is None      # (load: all active)
        # images from a pose between the two sets of frames
        for p in (dst, third):
            p.setPose(pose(30, _dim(n)))
            assert p.raycasting(K, _mu(field), 30)
        va, vb = dst.vertex_normal(), third.vertex_normal()
        assert _same([bits(v) for v in va], [bits(v) for v in vb]) and (va[1][..., 0] != -2).any()
        # boxes over blocks that only dst had, that the merge created, and that it combined
        leaf = leaf_level(n)
        dk, wk = make_keys(db[0], leaf), make_keys(want_b[0], leaf)
        moved = make_keys(sb[0].astype(np.int64) + np.array(s), leaf) if len(sb[0]) else np.zeros(0, np.uint64)
        old = want_b[0][np.isin(wk, dk) & ~np.isin(wk, moved)]
        new = want_b[0][~np.isin(wk, dk)]
        both = want_b[0][np.isin(wk, dk) & np.isin(wk, moved)]
        assert len(old) and len(new) and len(both)
        rng = np.random.default_rng(3)
        corners = np.concatenate([c[rng.permutation(len(c))[:40]] for c in (old, new, both)])
        boxes = np.concatenate([corners + rng.integers(-3, 6, corners.shape), rng.integers(1, 13, corners.shape)], 1).astype(np.int32)
        for cm in ("strict", "reference"):
            ha, hb = dst.collides(boxes, mode=cm), third.collides(boxes, mode=cm)
            assert (ha == hb).all() and len(np.unique(ha)) >= 2, cm
        ma, mb = _sorted_mesh(dst), _sorted_mesh(third)
        assert ma.shape == mb.shape and (ma == mb).all() and (len(ma) > 0 or field == OFUSION)
        # one further frame
        for p in (dst, third):
            _fuse_frame(p, 64)
        (ac, ax, ay, _), a_nodes = _state(dst)
        (bc, bx, by, bact), b_nodes = _state(third)
        assert equal_blocks_nodes((ac, ax, ay, bact), a_nodes, (bc, bx, by, bact), b_nodes) is None
        assert _same([bits(v) for v in dst.vertex_normal()], [bits(v) for v in third.vertex_normal()])
    finally:
        dst.close(); src.close(); third.close()


# ------------------------------------------------------------------ 3. properties
@pytest.mark.parametrize("field,dp,sp", [(SDF, 0, 1), (OFUSION, 1, 0)], ids=["sdf-dense-pooled", "ofusion-pooled-dense"])
def test_merging_into_a_fresh_map_reproduces_the_source(field, dp, sp):
    dst, src = _handle(field, 128, dp), _handle(field, 128, sp, SRC_FRAMES)
    try:
        sb, sn = _state(src)
        res = dst.merge(src)                                    # s = 0, FUSE
        got_b, got_n = _state(dst)
        # flags: a created block is active, as insertion leaves it -- the OR with the source's flag
        assert equal_blocks_nodes(got_b, got_n, (sb[0], sb[1], sb[2], np.ones_like(sb[3])), sn) is None
        assert res["blocks_created"] == len(sb[0]) and res["blocks_combined"] == 0 and res["blocks_clipped"] == 0
        assert res["nodes_combined"] == 1 and res["nodes_created"] == len(sn[0]) - 1 and res["nodes_skipped"] == 0      # (the root exists)
        assert res["region"] == (tuple(sb[0].min(0).tolist()), tuple((sb[0].max(0) + 8).tolist()))
    finally:
        dst.close(); src.close()


@pytest.mark.parametrize("pooled", [0, 1], ids=["dense", "pooled"])
def test_merging_an_empty_source_changes_nothing(pooled):
    dst, src = _handle(SDF, 128, pooled, DST_FRAMES), _handle(SDF, 64, 1 - pooled)
    try:
        before, src_before = map_state(dst), map_state(src)
        for mode in MODES:
            res = dst.merge(src, (16, 0, 8), mode=mode)
            assert counts_of(res).tolist() == [0, 0, 0, 0, 0, 1] + [0] * 6          # (the source's root: skipped)
            assert _same(before, map_state(dst)) and _same(src_before, map_state(src))
    finally:
        dst.close(); src.close()


@pytest.mark.parametrize("field", [SDF, OFUSION], ids=["sdf", "ofusion"])
def test_fill_never_changes_an_observed_destination_voxel(field):
    dst, src = _handle(field, 128, 0, DST_FRAMES), _handle(field, 128, 0, SRC_FRAMES)
    try:
        res, want_b, want_n, (db, dn, sb, sn) = _merge_and_check(dst, src, (0, 0, 0), "fill")
        (gc, gx, gy, _), (gcode, _, gnx, gny) = _state(dst)
        leaf = leaf_level(128)
        at = np.searchsorted(make_keys(gc, leaf), make_keys(db[0], leaf))
        seen = ~unseen(db[1], db[2], field)
        assert seen.any() and (bits(gx[at])[seen] == bits(db[1])[seen]).all() and (bits(gy[at])[seen] == bits(db[2])[seen]).all()
        assert (bits(gx[at])[~seen] != bits(db[1])[~seen]).any()           # ... and it did fill unseen ones
        atn = np.searchsorted(gcode, dn[0])
        seen_n = ~unseen(dn[2], dn[3], field)
        assert (bits(gnx[atn])[seen_n] == bits(dn[2])[seen_n]).all() and (bits(gny[atn])[seen_n] == bits(dn[3])[seen_n]).all()
    finally:
        dst.close(); src.close()


@pytest.mark.parametrize("max_weight,dp,sp", [(100, 0, 1), (255, 1, 0), (7, 1, 1)], ids=["100", "255", "7"])
def test_byte_weights_add_wider_than_a_byte(max_weight, dp, sp):
    """Destination weights edited to 200, source weights to 100: FUSE gives max_weight where both are observed, not (200 + 100) mod 256."""
    dst, src = _handle(SDF, 128, dp, DST_FRAMES), _handle(SDF, 128, sp, SRC_FRAMES)
    try:
        whole = np.array([[0, 0, 0, 128, 128, 128]], np.int32)
        for p, w in ((dst, 200.0), (src, 100.0)):
            assert p.edit(whole, y=w, only=("occupied", "empty"), nodes=False)[0] > 0
        res, want_b, want_n, (db, dn, sb, sn) = _merge_and_check(dst, src, (0, 0, 0), "fuse", max_weight)
        assert (db[2][~unseen(db[1], db[2], SDF)] == 200).all() and (sb[2][~unseen(sb[1], sb[2], SDF)] == 100).all()
        leaf = leaf_level(128)
        gc, gx, gy, _ = dst.blocks()
        dk, sk, gk = make_keys(db[0], leaf), make_keys(sb[0], leaf), make_keys(gc, leaf)
        common = np.intersect1d(dk, sk)
        a, b, g = np.searchsorted(dk, common), np.searchsorted(sk, common), np.searchsorted(gk, common)
        both = ~unseen(db[1][a], db[2][a], SDF) & ~unseen(sb[1][b], sb[2][b], SDF)
        assert both.sum() > 100 and (gy[g][both] == max_weight).all()
        only_src = unseen(db[1][a], db[2][a], SDF) & ~unseen(sb[1][b], sb[2][b], SDF)
        assert only_src.any() and (gy[g][only_src] == min(100, max_weight)).all()
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
    n, s = 128, (8, 0, -16)
    eager_d, eager_s = _handle(SDF, n, 0, DST_FRAMES), _handle(SDF, n, 0, SRC_FRAMES)
    want_b, want_n, want_c = merge_truth(n, *_state(eager_d), n, *_state(eager_s), s, FUSE, SDF)
    eager_d.close(); eager_s.close()
    (dst, ring_d), (src, ring_s) = _streaming_handle(SDF, n, 8), _streaming_handle(SDF, n, 8)
    try:
        for f in DST_FRAMES:
            _fuse_frame(dst, f, deferred=True)
        for f in SRC_FRAMES:
            _fuse_frame(src, f, deferred=True)
        before = dst.launch_counts(), src.launch_counts()
        res = dst.merge(src, s)
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
    n, s = 128, (64, 0, 0)

    def scanned(frames, nxt):
        p = _handle(SDF, n, 0, frames)
        p.set_depth(_depth(nxt, n)); p.setPose(pose(nxt, _dim(n)))
        nb = p.counts()[0]
        assert p.alloc_scan(K, 1, _mu(SDF), nxt)
        return p, nb
    (twin_d, nd), (twin_s, ns) = scanned(DST_FRAMES, 20), scanned(SRC_FRAMES, 90)
    want_b, want_n, want_c = merge_truth(n, *_state(twin_d), n, *_state(twin_s), s, FUSE, SDF)
    assert twin_d.counts()[0] > nd and twin_s.counts()[0] > ns          # the scans did insert blocks
    twin_d.close(); twin_s.close()
    (dst, _), (src, _) = scanned(DST_FRAMES, 20), scanned(SRC_FRAMES, 90)
    try:
        res = dst.merge(src, s)
        assert counts_of(res).tolist() == want_c.tolist()
        assert equal_blocks_nodes(*_state(dst), want_b, want_n) is None
    finally:
        dst.close(); src.close()


def test_tracking_goes_on_and_no_launch_counter_moves():
    n = 128
    dst, src = _handle(SDF, n, 0, DST_FRAMES), _handle(SDF, n, 1, SRC_FRAMES)
    try:
        dst.enable_timing(True)
        dst.timings(reset=True)
        before = dst.launch_counts(), src.launch_counts()
        dst.merge(src, (0, 0, 0))
        assert (dst.launch_counts(), src.launch_counts()) == before
        assert all(v["launches"] == 0 and v["ms_sum"] == 0 for v in dst.timings().values())
        dst.set_depth(_depth(4, n)); dst.setPose(pose(4, _dim(n)))
        assert dst.tracking(K, 1e-5, 1, 4)                     # (a shift would refuse: the images predate it; a merge does not move the frame of reference)
        assert np.isfinite(dst.pose_).all()
    finally:
        dst.close(); src.close()


# ------------------------------------------------------------------ 5. capacity
def test_a_pool_a_few_bricks_short_reports_capacity():
    """The pooled destination holds its own blocks and eight more; the merge wants more than that.  The call returns SE_HIP_E_CAPACITY
    (sticky, as from every other insertion); source blocks that found no slot are skipped by the kernel's slot check."""
    n = 128
    probe = _handle(SDF, n, 1, DST_FRAMES)
    nb = probe.counts()[0]
    probe.close()
    dst, src = _handle(SDF, n, 1, DST_FRAMES, max_blocks=nb + 8), _handle(SDF, n, 0, SRC_FRAMES)
    try:
        assert dst.counts()[0] == nb and dst.memory_info()["brick_slots"] == nb + 8
        sb = src.blocks()
        dk = make_keys(dst.blocks()[0], leaf_level(n))
        assert (~np.isin(make_keys(sb[0], leaf_level(n)), dk)).sum() > 8
        src_before = map_state(src)
        with pytest.raises(SeHipError, match="pool exhausted"):
            dst.merge(src)
        assert dst.clear_overflow() != 0
        assert dst.counts()[0] == nb + 8                        # the pool is full, not overrun
        gc, gx, gy, _ = dst.blocks()
        assert len(gc) == nb + 8 and np.isfinite(gx).all()
        assert _same(src_before, map_state(src))
        # a source whose own pool overflowed is refused
        small = _handle(SDF, n, 1, max_blocks=8)
        try:
            small.set_depth(_depth(0, n)); small.setPose(pose(0, _dim(n)))
            try:
                small.integration(K, 1, _mu(SDF), 0)
                small.sync()
            except SeHipError:
                pass
            before = map_state(dst)
            out = np.full(12, 77, np.int64)
            rule = _MergeRule(0, 100.0)
            s0 = np.zeros(3, np.int32)
            assert dst.lib.se_hip_merge_map(dst._h, small._h, s0.ctypes.data, C.addressof(rule), out.ctypes.data) == -3      # SE_HIP_E_CAPACITY
            assert (out == 77).all() and _same(before, map_state(dst))
        finally:
            small.close()
    finally:
        dst.close(); src.close()


# ------------------------------------------------------------------ 6. invalid arguments
def test_invalid_arguments_are_refused_and_change_nothing():
    n = 128
    dst, src = _handle(SDF, n, 0, DST_FRAMES), _handle(SDF, n, 1, SRC_FRAMES)
    other_field, other_voxel = _handle(OFUSION, n, 0), DenseSLAMPipeline((W, H), 64, 4.8, field_type=SDF)
    try:
        before = map_state(dst), map_state(src)
        out = np.full(12, 77, np.int64)
        lib, ok_rule, s0 = dst.lib, _MergeRule(0, 100.0), np.zeros(3, np.int32)

        def call(d, s_, shift, rule):
            return lib.se_hip_merge_map(d._h, s_._h, shift.ctypes.data if shift is not None else None,
                                        C.addressof(rule) if rule is not None else None, out.ctypes.data)
        assert call(dst, dst, s0, ok_rule) == -1 and "dst == src" in lib.se_hip_last_error().decode()
        assert call(dst, other_field, s0, ok_rule) == -1 and "field" in lib.se_hip_last_error().decode()
        assert call(dst, other_voxel, s0, ok_rule) == -1 and "voxel" in lib.se_hip_last_error().decode()
        for s in [(4, 0, 0), (0, -12, 0), (8, 8, 7), (0, 0, LIMIT + 8), (-LIMIT - 8, 0, 0), (2 ** 31 - 8, 0, 0)]:
            assert call(dst, src, np.array(s, np.int32), ok_rule) == -1
            assert "se_hip_merge_map" in lib.se_hip_last_error().decode()
        assert call(dst, src, None, ok_rule) == -1
        assert call(dst, src, s0, None) == -1
        for mode, mw in [(3, 100.0), (-1, 100.0), (0, 0.0), (0, 256.0), (0, 99.5), (0, float("nan")), (0, -1.0), (0, float("inf"))]:
            assert call(dst, src, s0, _MergeRule(mode, mw)) == -1, (mode, mw)
        assert lib.se_hip_merge_map(None, src._h, s0.ctypes.data, C.addressof(ok_rule), out.ctypes.data) == -1
        assert lib.se_hip_merge_map(dst._h, None, s0.ctypes.data, C.addressof(ok_rule), out.ctypes.data) == -1
        assert (out == 77).all() and _same(before[0], map_state(dst)) and _same(before[1], map_state(src))
        assert lib.se_hip_merge_map(dst._h, src._h, s0.ctypes.data, C.addressof(_MergeRule(2, 255.0)), None) == 0          # counts are optional
        assert lib.se_hip_merge_map(dst._h, src._h, np.array([LIMIT, -LIMIT, 0], np.int32).ctypes.data, C.addressof(_MergeRule(1, 1.0)), out.ctypes.data) == 0
        assert out[:3].tolist() == [0, 0, src.counts()[0]] and (out[6:] == 0).all()         # the limits themselves: everything clipped
    finally:
        for p in (dst, src, other_field, other_voxel):
            p.close()
