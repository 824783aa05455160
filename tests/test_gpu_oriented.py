"""Oriented box collision queries on the device (se_hip_collide_oriented / DenseSLAMPipeline.collides_oriented): the hand-worked cases on maps
built without depth (dense and pooled, both fields); the status against the definition evaluated in numpy over a dense class grid (room SDF
and stress OFusion, dense and pooled); the identities that tie an oriented box to the strict box query; 2^18 boxes in one batch; invalid
boxes and the threshold direction; and the schedule (streaming handle, the map, the images and the launch counters left alone).  Every
comparison is equality."""
import ctypes as C

import numpy as np
import pytest

from supereight_amd.pipeline import (COLLISION_EMPTY, COLLISION_INVALID, COLLISION_OCCUPIED, COLLISION_UNSEEN, OFUSION, SDF, DenseSLAMPipeline,
                                     _CollideTest)
from supereight_amd.synthetic import make_stream
from tests.gpu_state_util import H, W, bits, map_state, run_stream, streamed_with
from tests.motion_util import class_grid
from tests.oriented_util import (C_LIMIT, H_LIMIT, HAND_CASES, HAND_MAP_NAMES, I32_MIN, SUB, aligned_boxes, bounding_boxes, check_identities,
                                 hand_boxes, make_boxes, oriented_hand_grid, oriented_truth, random_boxes, stamp_oriented_map)

pytestmark = pytest.mark.gpu

ALL3 = {COLLISION_OCCUPIED, COLLISION_UNSEEN, COLLISION_EMPTY}


@pytest.mark.parametrize("field", [SDF, OFUSION], ids=["sdf", "ofusion"])
@pytest.mark.parametrize("max_blocks", [0, 1024], ids=["dense", "pooled"])
def test_hand_cases_on_the_device(field, max_blocks):
    import torch
    occupied_x, empty_x = (-0.5, 0.5) if field == SDF else (2.0, -2.0)
    for mp in HAND_MAP_NAMES:
        p = DenseSLAMPipeline((W, H), 64, 1.28, field_type=field, max_blocks=max_blocks)
        try:
            stamp_oriented_map(p, mp, occupied_x, empty_x)
            assert (class_grid(p, 64, 1.28, 0.0, field == OFUSION).cpu().numpy() == oriented_hand_grid(mp)).all()
            names = [k for k, c in HAND_CASES.items() if c[0] == mp]
            boxes = hand_boxes(names)
            st = p.collides_oriented(boxes)
            dev = p.collides_oriented(torch.from_numpy(boxes).to("cuda:0")).cpu().numpy()
            valid = np.array([HAND_CASES[k][6] is not None for k in names])
            bound = p.collides(bounding_boxes(boxes[valid]))
            for i, k in enumerate(names):
                assert int(st[i]) == HAND_CASES[k][5] and int(dev[i]) == HAND_CASES[k][5], (k, st[i], dev[i])
            for k, b in zip(np.array(names)[valid], bound):
                assert int(b) == HAND_CASES[k][6], (k, b)
        finally:
            p.close()


def _hits(p, n, dim, normals=False):
    v, nrm = p.vertex_normal()
    ok = nrm[..., 0] != -2
    hits = v[ok].reshape(-1, 3)
    assert len(hits) > 100
    return (hits * (n / dim), nrm[ok].reshape(-1, 3)) if normals else hits * (n / dim)      # voxels


def _plates_beside_the_surface(p, n, dim, rng, k, camera_m):
    """k thin plates (half lengths 3.5 x 3.5 x 0.3 voxels) tangent to the surface, 2 to 3.5 voxels in front of raycast hits whose normal is
    not along an axis (the spheres of the scenes): the plate stays in the free space before the surface while the corner of its bounding
    axis-aligned box reaches into it.  (Before an axis-aligned wall a box and its bounding box reach equally far.)"""
    hv, nv = _hits(p, n, dim, normals=True)
    nv = nv / np.linalg.norm(nv, axis=1, keepdims=True)
    oblique = np.nonzero(np.abs(nv).max(1) < 0.9)[0]
    assert len(oblique) >= 50
    pick = oblique[rng.choice(len(oblique), k)]
    h, u = hv[pick], nv[pick]
    u = u * np.sign(np.einsum("nk,nk->n", u, np.asarray(camera_m) * (n / dim) - h))[:, None]      # towards the camera
    t1 = np.cross(u, rng.normal(size=(k, 3)))
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    rot = np.stack([t1, np.cross(u, t1), u], 2)                                                    # columns: the box's axes
    centres = h + u * rng.uniform(2.0, 3.5, (k, 1))
    return make_boxes(centres * SUB, rot, np.tile(np.array([3.5, 3.5, 0.3]) * SUB, (k, 1)))


def _boxes(p, n, dim, rng, camera_m, k=1500):
    """k random boxes -- half-axis lengths 1 / 16 to 8 voxels, uniform random rotations, a fifth skewed; a third of them, of at least a voxel,
    centred within a few voxels of raycast hits, the rest anywhere from 8 voxels outside the volume --, then plates beside the curved
    surfaces, axis-aligned boxes on voxel boundaries and boxes wholly outside."""
    hv = _hits(p, n, dim)
    third = k // 3
    near = hv[rng.choice(len(hv), third)] + rng.uniform(-5, 5, (third, 3))
    sets = [random_boxes(rng, third, near * SUB, min_len=SUB), random_boxes(rng, k - third, rng.uniform(-8, n + 8, (k - third, 3)) * SUB)]
    sets.append(_plates_beside_the_surface(p, n, dim, rng, 300, camera_m))
    sets.append(aligned_boxes(rng, 120, n)[0])
    out = random_boxes(rng, 12, rng.uniform(-40, -12, (12, 3)) * SUB)
    out[6:, 0] = (n + 12) * SUB - out[6:, 0]
    sets.append(out)
    return np.ascontiguousarray(np.concatenate(sets))


BRUTE = [("room", SDF, 0), ("room", SDF, 2048), ("stress", OFUSION, 0), ("stress", OFUSION, 2048)]
_TRUTH = {}      # (kind, field) -> (class grid, boxes, truth): computed once, shared by the dense and the pooled case


@pytest.mark.parametrize("kind,field,max_blocks", BRUTE, ids=[f"{k}_{'sdf' if f == SDF else 'ofusion'}_{'dense' if m == 0 else 'pooled'}" for k, f, m in BRUTE])
def test_status_equals_the_definition(kind, field, max_blocks):
    n, dim = 128, 2.4
    p = run_stream(kind, field, n, dim, max_blocks, 4)
    try:
        grid = class_grid(p, n, dim, 0.0, field == OFUSION).cpu().numpy()
        if (kind, field) not in _TRUTH:
            boxes = _boxes(p, n, dim, np.random.default_rng(n + field), make_stream(kind, W, H, dim, holes=False).pose(3)[:3, 3])
            _TRUTH[(kind, field)] = (grid, boxes, np.array([oriented_truth(grid, b) for b in boxes.tolist()], np.uint8))
        grid0, boxes, truth = _TRUTH[(kind, field)]
        assert (grid == grid0).all()               # the brick layout does not change the map
        assert len(boxes) >= 1500
        bound = p.collides(bounding_boxes(boxes))
        print("truth", np.bincount(truth, minlength=3)[:3], "differs from the bounding box", int((bound != truth).sum()))
        assert ALL3 <= set(truth.tolist())
        assert (bound != truth).sum() >= 50        # the bounding box reports collisions (or unseen space) that the box does not touch
        assert (bound <= truth).all()
        st = p.collides_oriented(boxes)
        bad = np.nonzero(st != truth)[0]
        assert bad.size == 0, (bad[:5], boxes[bad[:5]], st[bad[:5]], truth[bad[:5]])
    finally:
        p.close()


@pytest.mark.parametrize("field,max_blocks", [(SDF, 8192), (OFUSION, 0)], ids=["sdf_pooled", "ofusion_dense"])
def test_identities_against_the_strict_box_query(field, max_blocks):
    n, dim = 256, 4.8
    p = run_stream("stress", field, n, dim, max_blocks, 4)
    try:
        rng = np.random.default_rng(19 + field)
        hv = _hits(p, n, dim)
        k = 1600
        centres = np.concatenate([hv[rng.choice(len(hv), k // 2)] + rng.uniform(-6, 6, (k // 2, 3)), rng.uniform(-10, n + 10, (k // 2, 3))])
        oriented = random_boxes(rng, k, centres * SUB, max_len=12 * SUB)
        aligned, lo_side = aligned_boxes(rng, 600, n)
        q = 300                                                # half of the aligned ones about the surface
        lo_side[:q, 0:3] = (hv[rng.choice(len(hv), q)] - 3).astype(np.int32)
        aligned[:q, 0:3] = SUB * lo_side[:q, 0:3] + (SUB // 2) * lo_side[:q, 3:6]
        assert len(oriented) + len(aligned) >= 2000
        st, sa, bound = check_identities(p, rng, oriented, aligned, lo_side)
        assert ALL3 <= set(np.unique(st).tolist())
        assert (bound < st).any()                              # the bounding box is not the box
    finally:
        p.close()


def test_quarter_million_boxes_at_512():
    import torch
    n, dim = 512, 4.8
    p = run_stream("room", SDF, n, dim, 0, 3)
    try:
        rng = np.random.default_rng(9)
        m = 1 << 18
        hv = _hits(p, n, dim)
        k = m // 2
        centres = np.concatenate([hv[rng.choice(len(hv), k // 2)] + rng.uniform(-6, 6, (k // 2, 3)), rng.uniform(-12, n + 12, (k - k // 2, 3))])
        oriented = random_boxes(rng, k, centres * SUB)
        aligned, lo_side = aligned_boxes(rng, m - k, n)
        q = (m - k) // 2
        lo_side[:q, 0:3] = (hv[rng.choice(len(hv), q)] - 3).astype(np.int32)
        aligned[:q, 0:3] = SUB * lo_side[:q, 0:3] + (SUB // 2) * lo_side[:q, 3:6]
        st, sa, bound = check_identities(p, rng, oriented, aligned, lo_side)
        assert ALL3 <= set(np.unique(st).tolist())
        assert (bound < st).any()
        boxes = np.ascontiguousarray(np.concatenate([oriented, aligned]))
        assert len(boxes) == m
        host = p.collides_oriented(boxes)
        assert (host == np.concatenate([st, sa])).all()
        dev = p.collides_oriented(torch.from_numpy(boxes).to("cuda:0"))
        assert isinstance(dev, torch.Tensor) and dev.dtype == torch.uint8 and dev.device.type == "cuda" and dev.shape == (m,)
        assert (dev.cpu().numpy() == host).all()
        empty = p.collides_oriented(np.zeros((0, 12), np.int32))
        assert empty.shape == (0,) and empty.dtype == np.uint8
        assert p.collides_oriented(torch.zeros((0, 12), dtype=torch.int32, device="cuda:0")).shape == (0,)
    finally:
        p.close()


@pytest.mark.parametrize("field,max_blocks", [(SDF, 0), (OFUSION, 4096)], ids=["sdf_dense", "ofusion_pooled"])
def test_invalid_boxes_and_threshold_direction(field, max_blocks):
    p = run_stream("room", field, 256, 2.4, max_blocks, 2)
    try:
        CL, HL, MX = C_LIMIT, H_LIMIT, 2 ** 31 - 1
        r = [4, 3, 0, -3, 4, 0, 0, 0, 5]
        bad = np.array([[100, 100, 100, 8, 8, 0, 1, 0, 0, 8, 8, 0], [100, 100, 100, 0, 0, 0, 0, 8, 0, 0, 0, 8], [100, 100, 100, 8, 0, 0, 16, 0, 0, 0, 0, 8],
                        [100, 100, 100, 1, 2, 3, 4, 5, 6, 5, 7, 9], [CL + 1, 0, 0] + r, [0, -CL - 1, 0] + r, [0, 0, MX] + r, [I32_MIN, 0, 0] + r,
                        [100, 100, 100, HL + 1, 0, 0, 0, 8, 0, 0, 0, 8], [100, 100, 100, 8, 0, 0, 0, -HL - 1, 0, 0, 0, 8], [100, 100, 100, 8, 0, 0, 0, 8, 0, 0, 0, MX],
                        [100, 100, 100, I32_MIN, 0, 0, 0, I32_MIN, 0, 0, 0, I32_MIN], [I32_MIN] * 12, [MX] * 12, [0] * 12], np.int64).astype(np.int32)
        edge = np.array([[CL, CL, CL] + r, [-CL, 100, 100] + r, [100, -CL, CL] + r, [2048, 2048, 2048, HL, 0, 0, 0, HL, 0, 0, 0, HL],
                         [2048, 2048, 2048, 0, 0, -HL, -HL, 0, 0, 0, HL, 0], [2048, 2048, 2048, HL, HL, HL, -HL, HL, 0, 0, -HL, HL]], np.int64).astype(np.int32)
        assert (p.collides_oriented(bad) == COLLISION_INVALID).all()
        st = p.collides_oriented(edge)
        assert (st != COLLISION_INVALID).all()
        assert (st[:3] == COLLISION_UNSEEN).all()                  # valid, wholly outside
        assert (st[3:] <= COLLISION_UNSEEN).all()                  # they hold the whole volume and leave it
        rng = np.random.default_rng(3)
        boxes = random_boxes(rng, 3000, rng.uniform(0, 250, (3000, 3)) * SUB, min_len=4)
        default = p.collides_oriented(boxes)
        above = field == OFUSION
        assert (default == p.collides_oriented(boxes, occupied_above=above)).all()
        flipped = p.collides_oriented(boxes, occupied_above=not above)
        assert (default == COLLISION_OCCUPIED).any() and (flipped != default).any()
        # unseen space does not depend on the test: where one direction finds nothing occupied and answers unseen or empty, so does ...
        both_free = (default != COLLISION_OCCUPIED) & (flipped != COLLISION_OCCUPIED)
        assert both_free.any() and (default[both_free] == flipped[both_free]).all()
        # a threshold nothing reaches: nothing is occupied
        far = p.collides_oriented(boxes, threshold=-1e30 if not above else 1e30)
        assert (far != COLLISION_OCCUPIED).all() and (far[default != COLLISION_OCCUPIED] == default[default != COLLISION_OCCUPIED]).all()
    finally:
        p.close()


def _launches(p):
    return {k: d["launches"] for k, d in p.timings().items()}


@pytest.mark.parametrize("field", [SDF, OFUSION], ids=["sdf", "ofusion"])
def test_boxes_see_the_map_of_the_frames_before_them(field):
    """On a streaming handle (scans on the side stream, raycasts held back) the answer after frame f equals the synchronous handle's; the
    calls change neither the map, the images nor the launch counters."""
    rng = np.random.default_rng(23)
    boxes = random_boxes(rng, 4000, rng.uniform(-8, 258, (4000, 3)) * SUB, min_len=4)
    ans = {True: [], False: []}

    def rec(streaming):
        def check(p, f):
            ans[streaming].append(p.collides_oriented(boxes))
        return check

    a = run_stream("room", field, 256, 2.4, 0, 4, streaming=True, check=rec(True))
    b = run_stream("room", field, 256, 2.4, 0, 4, streaming=False, check=rec(False))
    try:
        for u, w in zip(ans[True], ans[False]):
            assert (u == w).all()
        assert any((u != w).any() for u, w in zip(ans[False], ans[False][1:]))       # the answers follow the map
        a.enable_timing(True)
        before, la, ca = map_state(a), _launches(a), a.launch_counts()
        for _ in range(3):
            a.collides_oriented(boxes)
        after, lb, cb = map_state(a), _launches(a), a.launch_counts()
        assert la == lb and ca == cb
        assert all((u == w).all() for u, w in zip(before, after))
    finally:
        a.close(); b.close()


def test_boxes_between_frames_of_a_streaming_handle():
    """With frame 5's raycast held back on a streaming handle, the call flushes that raycast as a launch of its own, answers for the map with
    frame 5 fused, moves no other counter, and the image ring ends up as if the call had not been made."""
    f = 5
    rng = np.random.default_rng(6)
    boxes = random_boxes(rng, 2000, rng.uniform(0, 250, (2000, 3)) * SUB, min_len=4)
    got = {}

    def action(p, box):
        got["streamed"] = p.collides_oriented(boxes)

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
        st = ref.collides_oriented(boxes)
        assert (st == got["streamed"]).all()
        assert (st == COLLISION_OCCUPIED).any()
    finally:
        ref.close()


def test_oriented_entries_refuse_bad_arguments():
    import torch
    p = run_stream("room", SDF, 256, 2.4, 0, 1)
    try:
        lib = p.lib
        boxes = np.tile(np.array([[100, 100, 100, 8, 0, 0, 0, 8, 0, 0, 0, 8]], np.int32), (4, 1))
        st = np.zeros(4, np.uint8)
        dbx = torch.from_numpy(boxes).to("cuda:0")
        dst = torch.zeros(4, dtype=torch.uint8, device="cuda:0")
        good = _CollideTest(0.0, 0)
        for fn, ba, out in ((lib.se_hip_collide_oriented_host, boxes.ctypes.data, st.ctypes.data), (lib.se_hip_collide_oriented, dbx.data_ptr(), dst.data_ptr())):
            for args in ((ba, -1, C.byref(good), out), (None, 4, C.byref(good), out), (ba, 4, C.byref(good), None), (ba, 4, None, out),
                         (ba, 4, C.byref(_CollideTest(float("nan"), 0)), out), (ba, 4, C.byref(_CollideTest(float("inf"), 0)), out),
                         (ba, 4, C.byref(_CollideTest(0.0, 2)), out), (ba, 4, C.byref(_CollideTest(0.0, -1)), out)):
                assert fn(p._h, *args) == -1
            assert fn(p._h, None, 0, C.byref(good), None) == 0
            assert fn(p._h, ba, 4, C.byref(good), out) == 0
        p.sync()
        assert (st == dst.cpu().numpy()).all() and (st != COLLISION_INVALID).all()
    finally:
        p.close()
