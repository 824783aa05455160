"""Region edits on the device (se_hip_edit_boxes / DenseSLAMPipeline.edit): the reference's two known answers on maps loaded with
se_hip_load_map (dense and pooled); seeded lists of more than 200 edits against a numpy truth written here from the definitions of
include/se_hip.h (room and stress streams, SDF and OFusion, dense and pooled, 256^3 and 512^3, both modes); the readers see an edit
(query, mesh_blocks, cast_rays, the camera raycast, collides); the schedule (a deferred raycast is flushed first, launch counters, device
tensors without host synchronisation, n = 0, idempotence, 2^20 one-voxel edits and a whole-volume edit at 1024^3); the SDF weight rule."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from supereight_amd.pipeline import (COLLISION_EMPTY, EDIT_BLOCKS, EDIT_DTYPE, EDIT_NODES, EDIT_SET_X, EDIT_SET_Y, OFUSION, SDF,
                                     DenseSLAMPipeline, _CollideTest)
from supereight_amd.synthetic import make_stream
from tests.gpu_state_util import H, W, bits, map_state, run_stream, streamed_with
from tests.host_util import build_kats

pytestmark = pytest.mark.gpu
from tests.edit_util import CUM, DIR, INIT, LIMIT, OFF, _classes, _valid, make_edits, truth   # noqa: F401



def _check_list(p, field, n, dim, rng, mode, device):
    import torch
    c, x, y, a, code, side, nx, ny = p.blocks() + p.nodes()
    v, nrm = p.vertex_normal()
    hits = v[nrm[..., 0] != -2].reshape(-1, 3)
    assert len(hits) > 100
    rec, n_invalid = make_edits(rng, field, n, dim, c, hits)
    assert len(rec) >= 200
    test = (0.0, field == OFUSION)
    ex, ey, enx, eny, ecounts, info = truth(field, c, x, y, code, side, nx, ny, rec, test, mode)
    # the conditions under which the comparison means something
    assert ecounts[0] > 0 and ecounts[1] > 0 and ecounts[3] == n_invalid and info["rewritten"] > 0 and info["suppressed"] > 0, (ecounts, info)
    if device:
        drec = torch.from_numpy(rec.view(np.int32).reshape(-1, 10).copy()).to("cuda:0")
        got = p.edit_records(drec, test=test, mode=mode).cpu().numpy()
    else:
        got = p.edit_records(rec, test=test, mode=mode)
    c2, x2, y2, a2, code2, side2, nx2, ny2 = p.blocks() + p.nodes()
    print(f"{mode} device={device}: counts {got.tolist()} expected {ecounts.tolist()} {info}")
    assert (c2 == c).all() and (a2 == a).all() and (code2 == code).all() and (side2 == side).all()      # block set, node set, active flags
    assert (got == ecounts).all(), (got, ecounts)
    for nm, g, e in (("x", x2, ex), ("y", y2, ey), ("node x", nx2, enx), ("node y", ny2, eny)):
        bad = np.argwhere(bits(g) != bits(e))
        assert len(bad) == 0, (nm, len(bad), bad[:5].tolist(), g[tuple(bad[0])], e[tuple(bad[0])])
    assert (bits(x2) != bits(x)).any() and ((bits(nx2) != bits(nx)).any() or (bits(ny2) != bits(ny)).any())


LISTS = [("room", SDF, 256, 2.4, 0), ("room", SDF, 256, 2.4, 8192), ("room", OFUSION, 256, 2.4, 0), ("room", OFUSION, 256, 2.4, 8192),
         ("stress", SDF, 512, 4.8, 0), ("stress", SDF, 512, 4.8, 16384), ("stress", OFUSION, 512, 4.8, 0), ("stress", OFUSION, 512, 4.8, 16384)]


@pytest.mark.parametrize("kind,field,n,dim,max_blocks", LISTS,
                         ids=[f"{k}_{'sdf' if f == SDF else 'ofusion'}_{n}_{'dense' if m == 0 else 'pooled'}" for k, f, n, _, m in LISTS])
def test_edit_lists_equal_the_numpy_truth(kind, field, n, dim, max_blocks):
    """Truth by construction: strict mode through the host entry after frame 3, the reference mode through the device entry after frame 4
    (the map of frame 4 was fused on top of the first edit)."""
    rng = np.random.default_rng(1000 + n + field + max_blocks)

    def check(p, f):
        if f == 3:
            _check_list(p, field, n, dim, rng, "strict", device=False)
        if f == 4:
            _check_list(p, field, n, dim, rng, "reference", device=True)

    p = run_stream(kind, field, n, dim, max_blocks, 5, check=check)
    p.close()


# ------------------------------------------------------------------ the reference's known answers
@pytest.mark.parametrize("max_blocks", [0, 1024], ids=["dense", "pooled"])
def test_reference_known_answers_on_the_device(tmp_path, max_blocks):
    exe = build_kats("edit_kats", tmp_path)
    path = str(tmp_path / "band.bin")
    r = subprocess.run([exe, "save", path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    p = DenseSLAMPipeline((W, H), 256, 5.0, field_type=SDF, max_blocks=max_blocks)
    try:
        # BBoxTest: box [100, 151): 10 inside 100 .. 150, untouched elsewhere in every allocated block
        p.load(path)
        assert p.counts()[0] == 512
        counts = p.edit(np.array([[100, 100, 100, 151, 151, 151]], np.int32), 10.0, nodes=False, mode="reference")
        assert counts.tolist() == [51 ** 3, 0, 7 ** 3, 0]
        c, x, y, a = p.blocks()
        P = c.astype(np.int64)[:, None, :] + OFF[None]
        inside = ((P >= 100) & (P <= 150)).all(2)
        assert inside.sum() == 51 ** 3 and (x[inside] == 10).all() and (x[~inside] == 1).all() and (y == 0).all()
        # Init: a whole-map assignment reads back everywhere, voxels and node values
        p.load(path)
        counts = p.edit(np.array([[0, 0, 0, 256, 256, 256]], np.int32), 7.0, 3.0)
        nn = p.counts()[1]
        assert counts.tolist() == [512 * 512, 8 * nn, 512, 0]
        _, x, y, _ = p.blocks()
        _, _, nx, ny = p.nodes()
        assert (x == 7).all() and (y == 3).all() and (nx == 7).all() and (ny == 3).all()
    finally:
        p.close()


# ------------------------------------------------------------------ the readers see an edit
def test_readers_see_the_edit():
    from tests import ray_cast_util as U
    n, dim, mu, frames = 256, 2.4, 0.1, 5
    s = make_stream("room", W, H, dim, holes=False)
    p = run_stream("room", SDF, n, dim, 0, frames)
    try:
        lib = U.load()
        pose = s.pose(frames - 1)
        v, nrm = p.vertex_normal()
        hit = nrm[..., 0] != -2
        hv = np.floor(v * np.float32(n / dim)).astype(np.int64)
        centre = hv[H // 2, W // 2] if hit[H // 2, W // 2] else hv[hit][len(hv[hit]) // 2]
        # the aligned 64^3 octant around a visible surface point: every absent octant that meets it lies wholly inside it, so that assigning
        # "free" in strict mode leaves no unseen node value behind
        lo = (centre // 64) * 64
        hi = lo + 64
        box = np.array([list(lo) + list(hi)], np.int32)
        inbox = hit & ((hv >= lo + 2) & (hv < hi - 2)).all(2)
        assert inbox.sum() > 50                                  # a visible surface runs through the box
        rays = U.camera_rays(lib, pose, s.k, W, H)

        def cast(r):
            return p.cast_rays(r[:, 0:3].copy(), r[:, 3:6].copy(), r[:, 6].copy(), r[:, 7].copy(), mu=mu)

        before = cast(rays[inbox.reshape(-1)])
        hb = np.floor(before["hit"][:, :3] * np.float32(n / dim)).astype(np.int64)
        assert (((before["status"] & 4) != 0) & ((hb >= lo) & (hb < hi)).all(1)).sum() > 50
        counts = p.reset(box)
        assert counts[0] > 0 and counts[3] == 0
        # query(fine) at sampled voxels of the box: initValue()
        rng = np.random.default_rng(5)
        vox = rng.integers(lo, hi, (2000, 3))
        pts = ((vox.astype(np.float32) + np.float32(0.5)) * (np.float32(dim) / np.float32(n))).astype(np.float32)
        fine = p.query(np.ascontiguousarray(pts), fine=True, coarse=False, interp=False, grad=False, status=False)["fine"]
        assert (fine[:, 0] == 1).all() and (fine[:, 1] == 0).all()
        # mesh_blocks(region = box): its blocks are listed, without a triangle where the 9^3 dependency box lies inside the reset box
        mb = p.mesh_blocks(region=(tuple(int(q) for q in lo), tuple(int(q) for q in hi)))
        c = mb["coords"].astype(np.int64)
        dep_inside = ((c >= lo) & (c + 9 <= hi)).all(1)
        assert dep_inside.sum() > 8 and (mb["ranges"][dep_inside, 1] == 0).all()
        # rays through it no longer hit there
        after = cast(rays[inbox.reshape(-1)])
        ha = np.floor(after["hit"][:, :3] * np.float32(n / dim)).astype(np.int64)
        inside_after = ((after["status"] & 4) != 0) & ((ha >= lo + 1) & (ha < hi - 1)).all(1)
        assert inside_after.sum() == 0
        # the next camera raycast equals cast_rays of the same pixels
        allr = cast(rays)
        p.setPose(pose)
        assert p.raycasting(s.k, mu, frames)
        v2, n2 = p.vertex_normal()
        h2 = (allr["status"] & 4) != 0
        assert U.bits_equal(np.where(h2[:, None], allr["hit"][:, :3], np.float32(0)).astype(np.float32), v2.reshape(-1, 3))
        assert U.bits_equal(allr["normal"], n2.reshape(-1, 3))
        assert not U.bits_equal(v2, v)                          # and it is not the image from before the edit
        # "free" assigned to a box: a strict collision query inside it is EMPTY
        p.edit(box, 0.9, 5.0)
        inner = np.array([list(lo + 3) + [50, 40, 55]], np.int32)
        assert p.collides(inner, mode="strict")[0] == COLLISION_EMPTY
    finally:
        p.close()


# ------------------------------------------------------------------ schedule
def test_edit_flushes_a_deferred_raycast_first():
    """A streaming handle with an image ring and a twin without edits: the slot of frame f is the same on both when the edit is issued
    between frame f and f + 1, and the launch counters show that raycast as a launch of its own."""
    f = 5
    reset, quiet = (lambda p, box: p.reset(box)), (lambda p, box: p.reset(box, counts=False))
    edited, log = streamed_with(reset, f, again=quiet)
    twin, _ = streamed_with(reset, -1, again=quiet)
    assert log["fused"]
    for g in range(f + 1):
        assert (bits(edited[g]) == bits(twin[g])).all(), g
    assert (bits(edited[f + 1]) != bits(twin[f + 1])).any()           # the next frame's raycast saw the edit
    b, a, again = log["before"], log["after"], log["again"]
    assert b["pending"] and not a["pending"]
    assert a["raycast"] == b["raycast"] + 1 and a["fused"] == b["fused"]   # launched alone, not with a scan
    assert all(a[k] == b[k] for k in a if k not in ("raycast", "pending"))
    assert again == a                                                     # an edit itself moves no counter
    assert log["counts"][0] > 0 and log["counts"][3] == 0


def test_device_edits_without_host_synchronisation():
    """Frames, an edit on device tensors through the C entry and a device query, all enqueued without a host wait in between."""
    import torch
    n, dim, mu = 256, 2.4, 0.1
    s = make_stream("room", W, H, dim, holes=False)
    p = DenseSLAMPipeline((W, H), n, dim, field_type=SDF)
    try:
        for f in range(3):
            p.set_depth(s.depth(f)); p.setPose(s.pose(f)); p.integration(s.k, 1, mu, f); p.raycasting(s.k, mu, f)
        c = p.block_flags()[0].astype(np.int64)
        rec = np.zeros(len(c), EDIT_DTYPE)
        rec["lo"], rec["hi"] = c + 1, c + 3                                  # 8 voxels in every allocated block
        rec["x"], rec["y"] = -0.5, np.arange(len(c)) % 100
        rec["flags"], rec["only"] = EDIT_BLOCKS | EDIT_SET_X | EDIT_SET_Y, 7
        drec = torch.from_numpy(rec.view(np.int32).reshape(-1, 10).copy()).to("cuda:0")
        dcounts = torch.full((4,), -1, dtype=torch.int64, device="cuda:0")
        pts = ((c + 2).astype(np.float32) + np.float32(0.5)) * (np.float32(dim) / np.float32(n))
        dpts = torch.from_numpy(np.ascontiguousarray(pts.astype(np.float32))).to("cuda:0")
        torch.cuda.synchronize()
        f = 3
        p.set_depth(s.depth(f)); p.setPose(s.pose(f)); p.integration(s.k, 1, mu, f); p.raycasting(s.k, mu, f)
        assert p.lib.se_hip_edit_boxes(p._h, drec.data_ptr(), len(rec), None, 0, dcounts.data_ptr()) == 0
        res = p.query(dpts, fine=True, coarse=False, interp=False, grad=False, status=False)["fine"].cpu().numpy()    # (synchronises once, at its end)
        assert (res[:, 0] == np.float32(-0.5)).all() and (res[:, 1] == rec["y"]).all()
        assert dcounts.cpu().tolist() == [8 * len(c), 0, len(c), 0]
        # n == 0: nothing but the counts, zeroed
        assert p.edit(np.zeros((0, 6), np.int32), 1.0).tolist() == [0, 0, 0, 0]
        assert p.edit(torch.zeros((0, 6), dtype=torch.int32, device="cuda:0"), 1.0).cpu().tolist() == [0, 0, 0, 0]
        # the same unconditional list twice = once
        once = map_state(p)
        p.edit_records(rec)
        twice = map_state(p)
        assert all((u == w).all() for u, w in zip(once, twice))
        # refusals, before any launch
        good = _CollideTest(0.0, 0)
        for fn, addr in ((p.lib.se_hip_edit_boxes_host, rec.ctypes.data), (p.lib.se_hip_edit_boxes, drec.data_ptr())):
            for args in ((addr, -1, C.byref(good), 0, None), (None, 4, C.byref(good), 0, None), (addr, 4, C.byref(good), 2, None), (addr, 4, None, -1, None)):
                assert fn(p._h, *args) == -1
            assert fn(p._h, None, 0, None, 0, None) == 0
        assert all((u == w).all() for u, w in zip(twice, map_state(p)))
    finally:
        p.close()


def test_one_million_edits_at_1024():
    import torch
    n, dim = 1024, 4.8
    p = run_stream("room", SDF, n, dim, 0, 4)            # (the camera raycast runs from frame 3 on)
    try:
        rng = np.random.default_rng(8)
        m = 1 << 20
        vox = rng.integers(-4, n + 4, (m, 3))
        v, nrm = p.vertex_normal()
        hits = v[nrm[..., 0] != -2].reshape(-1, 3)
        k = m // 2
        vox[:k] = (hits[rng.choice(len(hits), k)] * (n / dim)).astype(np.int64) + rng.integers(-3, 4, (k, 3))
        rec = np.zeros(m, EDIT_DTYPE)
        rec["lo"], rec["hi"] = vox, vox + 1
        rec["x"] = (np.arange(m) % 1000).astype(np.float32) / np.float32(1024) - np.float32(0.5)
        rec["y"] = np.arange(m) % 101
        rec["flags"], rec["only"] = EDIT_BLOCKS | EDIT_SET_X | EDIT_SET_Y, 7
        drec = torch.from_numpy(rec.view(np.int32).reshape(-1, 10).copy()).to("cuda:0")
        pts = np.ascontiguousarray(((vox.astype(np.float32) + np.float32(0.5)) * (np.float32(dim) / np.float32(n))).astype(np.float32))
        st0 = p.query(pts, fine=False, coarse=False, interp=False, grad=False, status=True)["status"]
        counts = p.edit_records(drec).cpu().numpy()
        got = p.query(pts, fine=True, coarse=False, interp=False, grad=False, status=True)
        alloc = (st0 & 2) != 0
        assert (got["status"] == st0).all() and alloc.sum() > m // 4 and (~alloc).sum() > 1000
        # the last edit of a voxel wins
        key = (vox[:, 0] * (n + 8) + vox[:, 1]) * (n + 8) + vox[:, 2]
        order = np.argsort(key, kind="stable")                      # equal voxels stay in list order: a group's last entry is its last edit
        ks = key[order]
        ends = np.r_[np.nonzero(ks[1:] != ks[:-1])[0], m - 1]
        starts = np.r_[0, ends[:-1] + 1]
        last = np.empty(m, np.int64)
        last[order] = np.repeat(order[ends], ends - starts + 1)
        assert (last >= np.arange(m)).all() and (last != np.arange(m)).sum() > 100        # some voxels are edited more than once
        assert (got["fine"][alloc, 0] == rec["x"][last[alloc]]).all() and (got["fine"][alloc, 1] == rec["y"][last[alloc]]).all()
        assert (got["fine"][~alloc, 0] == 1).all() and (got["fine"][~alloc, 1] == 0).all()
        assert counts.tolist()[0] == int(alloc.sum()) and counts[1] == 0 and counts[3] == 0 and 0 < counts[2] <= p.counts()[0]
        # one whole-volume edit
        nb, nn = p.counts()
        counts = p.reset(np.array([[0, 0, 0, n, n, n]], np.int32))
        assert counts.tolist() == [nb * 512, nn * 8, nb, 0]
        _, x, y, _ = p.blocks()
        assert (x == 1).all() and (y == 0).all()
    finally:
        p.close()


# ------------------------------------------------------------------ the SDF weight rule
def test_sdf_weight_is_a_byte(tmp_path):
    p = run_stream("room", SDF, 256, 2.4, 0, 3)
    q = DenseSLAMPipeline((W, H), 256, 2.4, field_type=SDF)
    try:
        before = map_state(p)
        box = np.array([[0, 0, 0, 256, 256, 256]] * 2, np.int32)
        counts = p.edit(box, 0.25, np.float32([100.5, 256.0]))
        assert counts.tolist() == [0, 0, 0, 2]
        assert all((u == w).all() for u, w in zip(before, map_state(p)))
        counts = p.edit(box[:1], None, 255.0, nodes=False)
        assert counts[0] == before[1].size and counts[3] == 0
        _, x, y, _ = p.blocks()
        assert (y == 255).all() and (bits(x) == before[1]).all()
        path = str(tmp_path / "w255.bin")
        p.save(path)
        q.load(path)
        c2, x2, y2, _ = q.blocks()
        assert (c2 == before[0]).all() and (y2 == 255).all() and (bits(x2) == bits(x)).all()
    finally:
        p.close(); q.close()
