"""Box collision queries on the device (se_hip_collide_boxes / DenseSLAMPipeline.collides): the reference's known answers and the quirk cases
in both modes on maps loaded with se_hip_load_map (dense and pooled); strict mode against a brute-force min over a dense class grid built from
se_hip_query_points(coarse) at every voxel (room and stress streams, SDF and OFusion, dense and pooled, 256^3 and 512^3); reference mode
against the C++ mirror's getMap() snapshot (tests/cpp/collision_mirror.cpp); invariants; and the schedule (streaming handle, the map, the
images and the launch counters left alone, the device path, n = 0, one batch of 1 M boxes at 1024^3)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from supereight_amd.pipeline import (COLLISION_EMPTY, COLLISION_INVALID, COLLISION_OCCUPIED, COLLISION_UNSEEN, OFUSION, SDF,
                                     DenseSLAMPipeline, _CollideTest)
from tests.gpu_state_util import H, W, map_state, run_stream
from tests.host_util import COLLISION_KATS_EXPECTED, build_kats
from tests.mirror_util import build_mirror, run_mirror, write_scene

pytestmark = pytest.mark.gpu
INIT = {SDF: (1.0, 0.0), OFUSION: (0.0, 0.0)}    # voxel_traits<T>::initValue()

# the KAT / quirk cases of tests/cpp/collision_kats.cpp: map, lo, side
CASES = {
    "TotallyUnseen": ("kat", (23, 0, 100), (2, 2, 2)),
    "PartiallyUnseen": ("kat", (47, 0, 239), (6, 6, 6)),
    "Empty": ("kat", (49, 1, 242), (1, 1, 1)),
    "Collision": ("kat_collision", (54, 10, 249), (5, 5, 3)),
    "CollisionFreeLeaf": ("kat_freeleaf", (61, 13, 253), (2, 2, 2)),
    "QuirkLeafOrder": ("q_order", (4, 0, 0), (8, 4, 4)),
    "QuirkParentSlot0": ("q_slot0", (9, 0, 0), (2, 2, 2)),
    "QuirkInclusive": ("q_inclusive", (2, 2, 2), (2, 2, 2)),
}


@pytest.mark.parametrize("max_blocks", [0, 64], ids=["dense", "pooled"])
def test_kats_and_quirks_on_the_device(tmp_path, max_blocks):
    exe = build_kats("collision_kats", tmp_path)
    r = subprocess.run([exe, "save", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    p = DenseSLAMPipeline((W, H), 256, 5.0, field_type=SDF, max_blocks=max_blocks)
    try:
        for name, (mp, lo, side) in CASES.items():
            p.load(str(tmp_path / f"{mp}.bin"))
            box = np.array([list(lo) + list(side)], np.int32)
            got = (int(p.collides(box, threshold=5.0, mode="reference")[0]), int(p.collides(box, threshold=5.0, mode="strict")[0]))
            assert got == COLLISION_KATS_EXPECTED[name], name
    finally:
        p.close()


def _classify(x, y, field, thr, above):
    import torch
    unseen = (x == INIT[field][0]) & (y == INIT[field][1])
    occ = (x > thr) if above else (x < thr)
    return torch.where(unseen, torch.full_like(x, 1, dtype=torch.uint8),
                       torch.where(occ, torch.zeros_like(x, dtype=torch.uint8), torch.full_like(x, 2, dtype=torch.uint8)))


def _class_grid(p, n, dim, field, thr, above):
    """classify(Octree::get(v)) at every voxel v of the n^3 volume, from se_hip_query_points(coarse) at the voxel centres (a GPU tensor
    [z][y][x] of uint8)."""
    import torch
    dev = torch.device("cuda:0")
    grid = torch.empty((n, n, n), dtype=torch.uint8, device=dev)
    step = np.float32(dim) / np.float32(n)
    ax = (torch.arange(n, device=dev, dtype=torch.float32) + 0.5) * float(step)
    yy, xx = torch.meshgrid(ax, ax, indexing="ij")
    for z in range(0, n, max(1, (1 << 24) // (n * n))):
        zs = ax[z:z + max(1, (1 << 24) // (n * n))]
        pts = torch.stack([xx.expand(len(zs), n, n), yy.expand(len(zs), n, n), zs.view(-1, 1, 1).expand(len(zs), n, n)], dim=-1).reshape(-1, 3).contiguous()
        c = p.query(pts, fine=False, coarse=True, interp=False, grad=False, status=False)["coarse"]
        grid[z:z + len(zs)] = _classify(c[:, 0], c[:, 1], field, thr, above).view(len(zs), n, n)
    return grid


def _strict_truth(grid, boxes, n):
    out = np.empty(len(boxes), np.uint8)
    for i, (x, y, z, a, b, c) in enumerate(boxes.tolist()):
        x0, y0, z0 = max(x, 0), max(y, 0), max(z, 0)
        x1, y1, z1 = min(x + a, n), min(y + b, n), min(z + c, n)
        outside = x < 0 or y < 0 or z < 0 or x + a > n or y + b > n or z + c > n
        st = COLLISION_UNSEEN if outside else COLLISION_EMPTY
        if x0 < x1 and y0 < y1 and z0 < z1:
            st = min(st, int(grid[z0:z1, y0:y1, x0:x1].min()))
        out[i] = st
    return out


def _boxes(p, n, dim, rng):
    """~2k boxes: anisotropic sides 1..64 at random positions (some partly or wholly outside), centred on raycast hits, a few of side 128,
    the whole volume, one larger than the volume."""
    sets = []
    k = 1200
    side = rng.integers(1, 65, (k, 3))
    lo = rng.integers(-80, n + 16, (k, 3))
    sets.append(np.concatenate([lo, side], 1))
    v, nrm = p.vertex_normal()
    hits = v[nrm[..., 0] != -2].reshape(-1, 3)
    assert len(hits) > 100
    hv = (hits[rng.choice(len(hits), 700)] * (n / dim)).astype(np.int64)
    side = rng.integers(1, 33, (700, 3))
    sets.append(np.concatenate([hv - side // 2, side], 1))
    sets.append(np.concatenate([rng.integers(-64, n - 32, (6, 3)), np.full((6, 3), 128)], 1))
    sets.append(np.array([[0, 0, 0, n, n, n], [-3, -7, -1, n + 10, n + 9, n + 20]]))
    return np.ascontiguousarray(np.concatenate(sets).astype(np.int32))


STRICT = [("room", SDF, 256, 2.4, 0), ("room", SDF, 256, 2.4, 8192), ("room", OFUSION, 256, 2.4, 0), ("room", OFUSION, 256, 2.4, 8192),
          ("stress", SDF, 512, 4.8, 0), ("stress", SDF, 512, 4.8, 16384), ("stress", OFUSION, 512, 4.8, 0), ("stress", OFUSION, 512, 4.8, 16384)]


@pytest.mark.parametrize("kind,field,n,dim,max_blocks", STRICT,
                         ids=[f"{k}_{'sdf' if f == SDF else 'ofusion'}_{n}_{'dense' if m == 0 else 'pooled'}" for k, f, n, _, m in STRICT])
def test_strict_mode_equals_brute_force(kind, field, n, dim, max_blocks):
    rng = np.random.default_rng(n + field + max_blocks)
    above = field == OFUSION
    seen = set()

    def check(p, f):
        if f not in (1, 3):
            return
        grid = _class_grid(p, n, dim, field, 0.0, above)
        boxes = _boxes(p, n, dim, rng)
        got = p.collides(boxes)
        exp = _strict_truth(grid, boxes, n)
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, (f, bad[:5], boxes[bad[:5]], got[bad[:5]], exp[bad[:5]])
        seen.update(np.unique(got).tolist())
        # a 1-voxel strict box at v is classify(query coarse at v)
        v = rng.integers(0, n, (500, 3))
        one = np.ascontiguousarray(np.concatenate([v, np.ones_like(v)], 1).astype(np.int32))
        exp1 = grid[torch_idx(v)].cpu().numpy()
        assert (p.collides(one) == exp1).all()

    p = run_stream(kind, field, n, dim, max_blocks, 4, check=check)
    p.close()
    assert {COLLISION_OCCUPIED, COLLISION_UNSEEN, COLLISION_EMPTY} <= seen


def torch_idx(v):
    import torch
    t = torch.as_tensor(v, device="cuda:0")
    return (t[:, 2], t[:, 1], t[:, 0])


@pytest.mark.parametrize("tag,mu", [("SDF", 0.1), ("OFusion", 0.02)], ids=["sdf", "ofusion"])
def test_reference_mode_equals_the_host_mirror(tmp_path, tag, mu):
    exe = build_mirror(tmp_path, "collision_mirror", tag)
    Wm, Hm, N, dim, frames = 320, 240, 256, 4.8, 3
    raw, pf, _ = write_scene(tmp_path, Wm, Hm, dim, frames)
    res, r = run_mirror(exe, [raw, pf, N, dim, mu], timeout=600)
    assert res["bad"] == 0, r.stderr
    assert res["checked"] > 2000 and res["occupied"] > 0 and res["unseen"] > 0 and res["empty"] > 0 and res["differ"] > 0


@pytest.mark.parametrize("field,max_blocks", [(SDF, 0), (OFUSION, 4096)], ids=["sdf_dense", "ofusion_pooled"])
def test_invalid_boxes_and_threshold_direction(field, max_blocks):
    p = run_stream("room", field, 256, 2.4, max_blocks, 2)
    try:
        L = 1 << 30
        bad = np.array([[0, 0, 0, 0, 1, 1], [0, 0, 0, 1, -3, 1], [0, 0, 0, 1, 1, -(1 << 31)], [-L - 1, 0, 0, 1, 1, 1], [0, L + 1, 0, 1, 1, 1],
                        [0, 0, L, 1, 1, 1], [L - 4, 0, 0, 5, 1, 1], [0, -L + 2, 0, 1, 2 ** 31 - 1, 1]], np.int32)
        edge = np.array([[-L, 0, 0, 1, 1, 1], [0, 0, L - 1, 1, 1, 1], [-L, -L, -L, L, L, L]], np.int32)   # valid, wholly outside
        for mode in ("strict", "reference"):
            assert (p.collides(bad, mode=mode) == COLLISION_INVALID).all()
            assert (p.collides(edge, mode=mode) != COLLISION_INVALID).all()
        assert (p.collides(edge, mode="strict") == COLLISION_UNSEEN).all()
        rng = np.random.default_rng(3)
        boxes = np.ascontiguousarray(np.concatenate([rng.integers(0, 240, (3000, 3)), rng.integers(1, 17, (3000, 3))], 1).astype(np.int32))
        default = p.collides(boxes)
        above = field == OFUSION
        assert (default == p.collides(boxes, occupied_above=above)).all()
        flipped = p.collides(boxes, occupied_above=not above)
        assert (default == COLLISION_OCCUPIED).any() and (flipped != default).any()
        # unseen does not depend on the threshold: a box all unseen stays unseen
        assert ((default == COLLISION_UNSEEN) == (flipped == COLLISION_UNSEEN)).sum() > 0
    finally:
        p.close()


def _launches(p):
    return {k: d["launches"] for k, d in p.timings().items()}


@pytest.mark.parametrize("field", [SDF, OFUSION], ids=["sdf", "ofusion"])
def test_collide_sees_the_map_of_the_frames_before_it(field):
    """On a streaming handle (scans on the side stream, raycasts held back) the answer after frame f equals the synchronous handle's; the
    calls change neither the map, the images nor the launch counters."""
    rng = np.random.default_rng(21)
    boxes = np.ascontiguousarray(np.concatenate([rng.integers(-8, 250, (4000, 3)), rng.integers(1, 33, (4000, 3))], 1).astype(np.int32))
    ans = {True: [], False: []}

    def rec(streaming):
        def check(p, f):
            ans[streaming].append((p.collides(boxes), p.collides(boxes, mode="reference")))
        return check

    a = run_stream("room", field, 256, 2.4, 0, 4, streaming=True, check=rec(True))
    b = run_stream("room", field, 256, 2.4, 0, 4, streaming=False, check=rec(False))
    try:
        for (s1, r1), (s2, r2) in zip(ans[True], ans[False]):
            assert (s1 == s2).all() and (r1 == r2).all()
        a.enable_timing(True)
        before, la = map_state(a), _launches(a)
        for _ in range(3):
            a.collides(boxes)
            a.collides(boxes, mode="reference")
        after, lb = map_state(a), _launches(a)
        assert la == lb
        assert all((u == w).all() for u, w in zip(before, after))
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("field,max_blocks", [(SDF, 4096), (OFUSION, 0)], ids=["sdf_pooled", "ofusion_dense"])
def test_device_path_equals_host_path(field, max_blocks):
    import torch
    p = run_stream("room", field, 256, 2.4, max_blocks, 2)
    try:
        rng = np.random.default_rng(4)
        boxes = np.ascontiguousarray(np.concatenate([rng.integers(-20, 260, (5000, 3)), rng.integers(1, 40, (5000, 3))], 1).astype(np.int32))
        for mode in ("strict", "reference"):
            host = p.collides(boxes, mode=mode)
            dev = p.collides(torch.from_numpy(boxes).to("cuda:0"), mode=mode)
            assert isinstance(dev, torch.Tensor) and dev.device.type == "cuda" and dev.dtype == torch.uint8
            assert (dev.cpu().numpy() == host).all()
        empty = p.collides(np.zeros((0, 6), np.int32))
        assert empty.shape == (0,) and empty.dtype == np.uint8
        assert p.collides(torch.zeros((0, 6), dtype=torch.int32, device="cuda:0")).shape == (0,)
    finally:
        p.close()


def test_collide_entries_refuse_bad_arguments():
    import torch
    p = run_stream("room", SDF, 256, 2.4, 0, 1)
    try:
        lib = p.lib
        boxes = np.zeros((4, 6), np.int32)
        st = np.zeros(4, np.uint8)
        dboxes = torch.zeros((4, 6), dtype=torch.int32, device="cuda:0")
        dst = torch.zeros(4, dtype=torch.uint8, device="cuda:0")
        good = _CollideTest(0.0, 0)
        for fn, ba, sa in ((lib.se_hip_collide_boxes_host, boxes.ctypes.data, st.ctypes.data), (lib.se_hip_collide_boxes, dboxes.data_ptr(), dst.data_ptr())):
            for args in ((ba, -1, C.byref(good), 0, sa), (None, 4, C.byref(good), 0, sa), (ba, 4, C.byref(good), 0, None), (ba, 4, None, 0, sa),
                         (ba, 4, C.byref(_CollideTest(float("nan"), 0)), 0, sa), (ba, 4, C.byref(_CollideTest(float("inf"), 0)), 0, sa),
                         (ba, 4, C.byref(_CollideTest(0.0, 2)), 0, sa), (ba, 4, C.byref(good), 2, sa), (ba, 4, C.byref(good), -1, sa)):
                assert fn(p._h, *args) == -1
            assert fn(p._h, None, 0, C.byref(good), 0, None) == 0
    finally:
        p.close()


def test_one_million_boxes_at_1024():
    import torch
    n, dim = 1024, 4.8
    p = run_stream("room", SDF, n, dim, 0, 3)
    try:
        rng = np.random.default_rng(8)
        m = 1 << 20
        boxes = np.concatenate([rng.integers(-16, n, (m, 3)), rng.integers(1, 9, (m, 3))], 1).astype(np.int32)
        v, nrm = p.vertex_normal()
        hits = v[nrm[..., 0] != -2].reshape(-1, 3)
        k = m // 4
        boxes[:k, :3] = (hits[rng.choice(len(hits), k)] * (n / dim)).astype(np.int32) - 4
        boxes = np.ascontiguousarray(boxes)
        got = p.collides(torch.from_numpy(boxes).to("cuda:0")).cpu().numpy()
        assert (got == COLLISION_OCCUPIED).any() and (got == COLLISION_EMPTY).any() and (got == COLLISION_UNSEEN).any()
        # a sample against classify(query coarse) over each box's voxels
        idx = rng.choice(m, 300, replace=False)
        for i in idx:
            x, y, z, a, b, c = boxes[i].tolist()
            g = np.stack(np.meshgrid(np.arange(x, x + a), np.arange(y, y + b), np.arange(z, z + c), indexing="ij"), -1).reshape(-1, 3)
            inside = ((g >= 0) & (g < n)).all(1)
            st = COLLISION_EMPTY if inside.all() else COLLISION_UNSEEN
            if inside.any():
                pts = ((g[inside].astype(np.float32) + np.float32(0.5)) * (np.float32(dim) / np.float32(n))).astype(np.float32)
                cz = p.query(np.ascontiguousarray(pts), fine=False, coarse=True, interp=False, grad=False, status=False)["coarse"]
                cls = _classify(torch.from_numpy(cz[:, 0]), torch.from_numpy(cz[:, 1]), SDF, 0.0, False).numpy()
                st = min(st, int(cls.min()))
            assert got[i] == st, (i, boxes[i], got[i], st)
    finally:
        p.close()
