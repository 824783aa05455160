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
from tests.map_query_util import INIT, Map as _Map, compare as _compare

pytestmark = pytest.mark.gpu

W, H, N, DIM = 160, 120, 256, 2.4


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
