"""Batched map queries on the device (se_hip_query_points / DenseSLAMPipeline.query) against the CPU oracle's octree built from the
device's own map: fine.x / coarse.x / interp / grad bit for bit with so_ft_get_fine / so_ft_get / so_ft_interp / so_ft_grad, fine.y /
coarse.y against a gather from blocks() / nodes(), status bits against the downloaded block set.  Plus the defined answers for
points the reference leaves undefined, the schedule (streaming vs synchronous, queries leave the map and images alone), the device
path, and argument validation."""
import ctypes as C

import numpy as np
import pytest

from supereight_amd.pipeline import OFUSION, SDF, DenseSLAMPipeline
from supereight_amd.synthetic import make_stream
from tests.host_util import decode, morton

pytestmark = pytest.mark.gpu

W, H, N, DIM = 160, 120, 256, 2.4
INIT = {SDF: (1.0, 0.0), OFUSION: (0.0, 0.0)}    # voxel_traits<T>::initValue(); empty().x equals initValue().x for both


def _run(field, frames=3, max_blocks=0, kind="room", mu=None, streaming=False, query_points=None):
    mu = mu if mu is not None else (0.1 if field == SDF else 0.02)
    s = make_stream(kind, W, H, DIM, holes=False)
    p = DenseSLAMPipeline((W, H), N, DIM, field_type=field, max_blocks=max_blocks, streaming=streaming)
    answers = []
    for f in range(frames):
        p.set_depth(s.depth(f))
        p.setPose(s.pose(f))
        p.integration(s.k, 1, mu, f)
        if streaming:
            p.raycasting_deferred(s.k, mu, f)
        else:
            p.raycasting(s.k, mu, f)
        if query_points is not None:
            answers.append(p.query(query_points, coarse=True))
    return p, answers


class _Map:
    """The device map as downloaded, with the oracle's octree (FTree) built from it (a map of n^3 voxels over dim metres)."""

    def __init__(self, oracle, p, field, n=N, dim=DIM):
        self.lib, self.field = oracle, field
        self.N, self.dim = n, dim
        self.coords, self.x, self.y, _ = p.blocks()
        self.ncode, _, self.nx, self.ny = p.nodes()
        self.row = {tuple(int(v) for v in c): i for i, c in enumerate(self.coords)}
        self.nrow = {int(c): i for i, c in enumerate(self.ncode)}
        self.init = INIT[field]
        self.max_level = n.bit_length() - 1
        t = oracle.so_ft_create(n, dim, self.init[0], self.init[0])
        code, co, isb = C.c_uint64(0), np.zeros(3, np.int32), C.c_int(0)
        for c in sorted(self.ncode, key=lambda k: int(k) & 0x1FF):
            x, y, z, lvl = decode(c)
            if lvl:
                oracle.so_ft_insert(t, x, y, z, lvl, C.byref(code), co, C.byref(isb))
                assert int(code.value) == int(c)
        for i, c in enumerate(self.ncode):
            x, y, z, lvl = decode(c)
            for j in range(8):
                assert oracle.so_ft_set_octant_value(t, x, y, z, lvl, j, float(self.nx[i, j]))
        init_bits = np.float32(self.init[0]).view(np.uint32)
        for i, (bx, by, bz) in enumerate(self.coords):
            oracle.so_ft_insert(t, int(bx), int(by), int(bz), -1, C.byref(code), co, C.byref(isb))
            assert isb.value == 1 and tuple(co) == (bx, by, bz)
            for v in np.nonzero(self.x[i].view(np.uint32) != init_bits)[0]:
                oracle.so_ft_set(t, int(bx) + int(v & 7), int(by) + int((v >> 3) & 7), int(bz) + int(v >> 6), float(self.x[i, v]))
        self.t = t

    def close(self):
        self.lib.so_ft_destroy(self.t)

    def allocated(self, bx, by, bz):
        return (bx * 8, by * 8, bz * 8) in self.row

    def expected(self, pts):
        """Oracle answers for float32 points [n, 3] in metres."""
        lib, t, N = self.lib, self.t, self.N
        s = np.float32(N) / np.float32(self.dim)
        q = (s * pts).astype(np.float32)
        n = len(pts)
        fine, coarse = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
        interp, grad, status = np.zeros(n, np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
        g = np.zeros(3, np.float32)
        leaf = self.max_level - 3
        for i in range(n):
            qx, qy, qz = (float(v) for v in q[i])
            v = [int(a) for a in q[i]]        # (int) truncation
            x, y, z = v
            fine[i, 0] = lib.so_ft_get_fine(t, x, y, z)
            coarse[i, 0] = lib.so_ft_get(t, x, y, z)
            interp[i] = lib.so_ft_interp(t, qx, qy, qz)
            lib.so_ft_grad(t, qx, qy, qz, g)
            grad[i] = g
            fine[i, 1] = coarse[i, 1] = self.init[1]
            st = 0
            if all(0 <= a < N for a in v):
                st |= 1
                r = self.row.get((x & ~7, y & ~7, z & ~7))
                if r is not None:
                    st |= 2
                    fine[i, 1] = coarse[i, 1] = self.y[r, (x & 7) + 8 * (y & 7) + 64 * (z & 7)]
                else:
                    parent = self.nrow[0]
                    for lvl in range(1, leaf + 1):
                        side = N >> lvl
                        key = morton(x & ~(side - 1), y & ~(side - 1), z & ~(side - 1)) | lvl
                        if lvl < leaf and key in self.nrow:
                            parent = self.nrow[key]
                            continue
                        child = int((x & side) > 0) + 2 * int((y & side) > 0) + 4 * int((z & side) > 0)
                        coarse[i, 1] = self.ny[parent, child]
                        break
            lo = [max(int(np.floor(a)), 0) for a in q[i]]
            cross = [(a & 7) == 7 for a in lo]
            ok = True
            for k in range(8):
                d = (k & 1, (k >> 1) & 1, k >> 2)
                if all(cross[a] or d[a] == 0 for a in range(3)):
                    b = [(lo[a] + d[a]) >> 3 for a in range(3)]
                    ok = ok and all(0 <= c < N // 8 for c in b) and self.allocated(*b)
            st |= 4 if ok else 0
            status[i] = st
        return {"fine": fine, "coarse": coarse, "interp": interp, "grad": grad, "status": status}

    def points(self, p, rng):
        """Random points in the volume, jittered raycast hits, block faces / edges / corners, points next to missing blocks, and
        points just outside each face of the volume (metres, float32)."""
        N, DIM = self.N, self.dim
        vox = np.float32(DIM) / np.float32(N)
        sets = [rng.uniform(0, DIM, (600, 3))]
        v, nrm = p.vertex_normal()
        hits = v[nrm[..., 0] != -2]
        assert len(hits) > 100
        sets.append(hits[rng.choice(len(hits), 600)] + rng.uniform(-2, 2, (600, 3)) * vox)
        blocks = self.coords[rng.choice(len(self.coords), min(60, len(self.coords)), replace=False)].astype(np.float64)
        for off in ((7.5, 3.2, 4.1), (7.5, 7.5, 2.6), (7.5, 7.5, 7.5), (8.0, 8.0, 8.0), (7.999, 0.0, 7.999), (-0.001, 4.0, 4.0), (3.3, -0.5, 7.2)):
            sets.append((blocks + np.asarray(off)) * vox)
        near = []
        for bx, by, bz in blocks.astype(int):
            for d in ((8, 0, 0), (-8, 0, 0), (0, 8, 0), (0, -8, 0), (0, 0, 8), (0, 0, -8)):
                c = (bx + d[0], by + d[1], bz + d[2])
                if c not in self.row and all(0 <= a < N for a in c):
                    near.append(np.asarray(c) + rng.uniform(-1.5, 9.5, 3))
        assert near
        sets.append(np.asarray(near) * vox)
        for face in range(6):
            u = rng.uniform(0, N, (30, 3))
            u[:, face // 2] = N + rng.uniform(0, 1.5, 30) if face & 1 else -rng.uniform(0, 1.5, 30)
            sets.append(u * vox)
        return np.ascontiguousarray(np.concatenate(sets).astype(np.float32))


def _compare(got, exp, what=("fine", "coarse", "interp", "grad", "status")):
    for k in what:
        a, b = got[k], exp[k]
        if a.dtype == np.float32:
            bad = np.nonzero((a.view(np.uint32) != b.view(np.uint32)).reshape(len(a), -1).any(axis=1))[0]
        else:
            bad = np.nonzero(a != b)[0]
        assert bad.size == 0, (k, bad[:5], a[bad[:5]], b[bad[:5]])


CASES = [("room", SDF, 0), ("room", SDF, 4096), ("room", OFUSION, 0), ("room", OFUSION, 4096), ("stress", SDF, 0)]


@pytest.mark.parametrize("kind,field,max_blocks", CASES, ids=["sdf_dense", "sdf_pooled", "ofusion_dense", "ofusion_pooled", "stress_sdf"])
def test_query_equals_the_oracle(oracle, kind, field, max_blocks):
    p, _ = _run(field, frames=3, max_blocks=max_blocks, kind=kind)
    assert p.memory_info()["layout"] == ("dense brick grid" if max_blocks == 0 else "pooled bricks")
    m = _Map(oracle, p, field)
    try:
        assert 0 < len(m.coords) <= 2500
        pts = m.points(p, np.random.default_rng(11 + field))
        got = p.query(pts, fine=True, coarse=True, interp=True, grad=True, status=True)
        exp = m.expected(pts)
        _compare(got, exp)
        st = got["status"]
        # a non-trivial map and point set: allocated and unallocated, observed and unobserved cells, in and out of the volume
        for bit in (1, 2, 4):
            assert ((st & bit) != 0).any() and ((st & bit) == 0).any(), bit
        assert np.unique(got["interp"]).size > 100 and np.abs(got["grad"]).max() > 0
        if field == OFUSION:    # coarse node values where no block exists (OFusion's free space)
            assert ((st & 3) == 1).any() and (got["coarse"][(st & 3) == 1, 0] != INIT[OFUSION][0]).any()
    finally:
        m.close()
        p.close()


@pytest.mark.parametrize("field,max_blocks", [(SDF, 0), (OFUSION, 4096)], ids=["sdf_dense", "ofusion_pooled"])
def test_query_defined_beyond_the_reference(field, max_blocks):
    """Non-finite points and |s p| >= 2^20 give the defaults and status 0; points outside the volume give initValue() for fine / coarse."""
    p, _ = _run(field, frames=2, max_blocks=max_blocks)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    s = np.float32(N) / np.float32(DIM)
    big = np.float32(1048576.0) / s * np.float32(1.0001)
    pts = np.array([[nan, 1, 1], [1, nan, 1], [1, 1, nan], [inf, 1, 1], [1, -inf, 1], [1, 1, inf], [big, 1, 1], [1, -big, 1], [1, 1, 1e30],
                    [-1e30, -1e30, -1e30]], np.float32)
    r = p.query(pts, coarse=True)
    init = np.asarray(INIT[field], np.float32)
    assert (r["status"] == 0).all()
    assert (r["fine"] == init).all() and (r["coarse"] == init).all()
    assert (r["interp"] == np.float32(INIT[field][0])).all()
    assert (r["grad"].view(np.uint32) == 0).all()
    # outside the volume but finite: fine / coarse = initValue(), bit 0 clear
    out = np.array([[-0.5, 1, 1], [1, DIM * 1.5, 1], [1, 1, -3 * DIM], [DIM, DIM, DIM]], np.float32)
    r = p.query(out, coarse=True)
    assert (r["status"] & 1 == 0).all() and (r["fine"] == init).all() and (r["coarse"] == init).all()
    assert np.isfinite(r["interp"]).all() and np.isfinite(r["grad"]).all()
    p.close()


def _all_points(rng):
    return np.ascontiguousarray(rng.uniform(-0.05 * DIM, 1.05 * DIM, (3000, 3)).astype(np.float32))


@pytest.mark.parametrize("field", [SDF, OFUSION], ids=["sdf", "ofusion"])
def test_query_sees_the_map_of_the_frames_before_it(field):
    """A query after frame f on a streaming handle (frames enqueued back to back, scans on the side stream, raycasts held back) equals
    the same query after frame f of a synchronous handle; and queries after every frame change neither the map nor the images."""
    pts = _all_points(np.random.default_rng(5))
    frames = 4
    a, qa = _run(field, frames=frames, streaming=True, query_points=pts)
    b, qb = _run(field, frames=frames, streaming=False, query_points=pts)
    c, _ = _run(field, frames=frames, streaming=True)
    try:
        for f in range(frames):
            _compare(qa[f], qb[f])
        assert qa[-1]["status"].any()
        ca, xa, ya, aa = a.blocks()
        cc, xc, yc, ac = c.blocks()
        assert (ca == cc).all() and (xa.view(np.uint32) == xc.view(np.uint32)).all() and (ya == yc).all() and (aa == ac).all()
        na, nc = a.nodes(), c.nodes()
        assert all((u.view(np.uint32) == w.view(np.uint32)).all() if u.dtype == np.float32 else (u == w).all() for u, w in zip(na, nc))
        va, ua = a.vertex_normal()
        vc, uc = c.vertex_normal()
        assert (va.view(np.uint32) == vc.view(np.uint32)).all() and (ua.view(np.uint32) == uc.view(np.uint32)).all()
    finally:
        a.close(); b.close(); c.close()


@pytest.mark.parametrize("field,max_blocks", [(SDF, 4096), (OFUSION, 0)], ids=["sdf_pooled", "ofusion_dense"])
def test_device_path_equals_host_path(field, max_blocks):
    import torch
    p, _ = _run(field, frames=2, max_blocks=max_blocks)
    pts = _all_points(np.random.default_rng(9))
    host = p.query(pts, coarse=True)
    dev = p.query(torch.from_numpy(pts).to("cuda:0"), coarse=True)
    assert set(dev) == set(host)
    for k in host:
        assert isinstance(dev[k], torch.Tensor) and dev[k].device.type == "cuda"
        d = dev[k].cpu().numpy()
        assert d.shape == host[k].shape and d.dtype == host[k].dtype
        assert (d.view(np.uint8) == host[k].view(np.uint8)).all(), k
    # a subset of the outputs: the same values
    part = p.query(torch.from_numpy(pts).to("cuda:0"), fine=False, interp=True, grad=False, status=False)
    assert set(part) == {"interp"} and (part["interp"].cpu().numpy().view(np.uint32) == host["interp"].view(np.uint32)).all()
    empty = p.query(np.zeros((0, 3), np.float32))
    assert all(v.shape[0] == 0 for v in empty.values())
    p.close()


def test_query_entries_refuse_bad_arguments():
    import torch
    from supereight_amd.pipeline import _QueryOut
    p, _ = _run(SDF, frames=1)
    lib = p.lib
    pts = np.zeros((4, 3), np.float32)
    out_h = np.zeros(4, np.float32)
    dev_pts = torch.zeros((4, 3), dtype=torch.float32, device="cuda:0")
    dev_out = torch.zeros(4, dtype=torch.float32, device="cuda:0")
    none = _QueryOut(None, None, None, None, None)
    for fn, pa, oa in ((lib.se_hip_query_points_host, pts.ctypes.data, out_h.ctypes.data), (lib.se_hip_query_points, dev_pts.data_ptr(), dev_out.data_ptr())):
        good = _QueryOut(None, None, oa, None, None)
        for args in ((pa, -1, C.byref(good)), (None, 4, C.byref(good)), (pa, 4, C.byref(none)), (pa, 4, None)):
            assert fn(p._h, *args) == -1
            assert lib.se_hip_last_error().decode()
        assert fn(p._h, pa, 0, C.byref(good)) == 0
        assert fn(p._h, None, 0, C.byref(good)) == 0
        assert fn(p._h, pa, 4, C.byref(good)) == 0
    assert lib.se_hip_query_points_host(None, pts.ctypes.data, 4, C.byref(_QueryOut(None, None, out_h.ctypes.data, None, None))) == -1
    p.sync()
    p.close()
