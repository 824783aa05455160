"""Live meshing per block on the device (se_hip_mesh_blocks / DenseSLAMPipeline.mesh_blocks / LiveMesh / DenseSLAMSystem::meshBlocks).
Every comparison of triangles is bit for bit.
  - the whole volume equals the export (se_hip_mesh_download) and the oracle's mesh, sorted; the header equals se_hip_mesh_count;
  - block structure, determinism (two calls, and the payload rebuilt on the host in the defined cell order), regions, views (LiveMesh ends
    every update equal to the export; the device's selection lies within the loosened restatement and leaves blocks out), capacities,
    calls between streamed frames, the entry paths and the refusals."""
import ctypes as C

import numpy as np
import pytest

from oracle.binding import OraclePipeline
from supereight_amd.livemesh import LiveMesh
from supereight_amd.pipeline import OFUSION, SDF, DenseSLAMPipeline, _MeshOut, _MeshSelect, _MeshView
from supereight_amd.synthetic import make_stream
from tests import live_mesh_util as L
from tests.gpu_state_util import map_state
from tests.mirror_util import build_mirror, run_mirror, write_scene

pytestmark = pytest.mark.gpu
DIM = 4.8


def _mu(field):
    return 0.1 if field == SDF else 0.02


def _integrate(gpu, s, f, mu, cpu=None):
    d, pose = s.depth(f), s.pose(f)
    gpu.set_depth(d); gpu.setPose(pose)
    gpu.integration(s.k, 1, mu, f)
    gpu.raycasting(s.k, mu, f)
    if cpu is not None:
        cpu.integrate(d, pose, s.k, mu, f)


def _device(kind, field, N, max_blocks, W, H, frames, oracle=False):
    s = make_stream(kind, W, H, DIM, holes=False)
    gpu = DenseSLAMPipeline((W, H), N, DIM, field_type=field, max_blocks=max_blocks)
    cpu = OraclePipeline(field, N, DIM, W, H) if oracle else None
    for f in range(frames):
        _integrate(gpu, s, f, _mu(field), cpu)
    assert gpu.memory_info()["layout"] == ("dense brick grid" if max_blocks == 0 else "pooled bricks")
    return s, gpu, cpu


def _check_structure(gpu, res, N, allocated, skip_empty):
    coords, ranges, tris = res["coords"], res["ranges"], res["triangles"]
    vs = np.float32(DIM) / np.float32(N)
    assert len(np.unique(coords, axis=0)) == len(coords) and (coords % 8 == 0).all()
    # ranges: disjoint, covering [0, written)
    order = np.argsort(ranges[:, 0], kind="stable")
    r = ranges[order]
    r = r[r[:, 1] > 0]
    assert (ranges[:, 1] >= 0).all() and int(ranges[:, 1].sum()) == len(tris)
    if len(r):
        assert r[0, 0] == 0 and (r[1:, 0] == r[:-1, 0] + r[:-1, 1]).all() and r[-1, 0] + r[-1, 1] == len(tris)
    # every triangle of a block within the closed box [8b, 8b + 8] voxels
    owner = np.repeat(order, ranges[order, 1])      # (the ranges tile [0, written): triangle j belongs to the j-th entry of this list)
    lo = coords[owner].astype(np.float32) * vs
    hi = (coords[owner] + 8).astype(np.float32) * vs
    t = tris.reshape(-1, 3, 3)
    assert ((t >= lo[:, None, :]) & (t <= hi[:, None, :])).all()
    # the table against the allocated blocks
    alloc = {tuple(c) for c in allocated.tolist()}
    listed = {tuple(c) for c in coords.tolist()}
    assert listed <= alloc
    if skip_empty:
        assert (ranges[:, 1] > 0).all()
    return listed


WHOLE = [(f"{kind}_{'sdf' if field == SDF else 'ofusion'}_{'dense' if mb == 0 else 'pooled'}_{N}", kind, field, N, mb)
         for kind in ("room", "stress") for field in (SDF, OFUSION) for mb in (0, 1 << 17) for N in (256, 512)] + [("stress_sdf_dense_1024", "stress", SDF, 1024, 0)]


@pytest.mark.parametrize("name,kind,field,N,max_blocks", WHOLE, ids=[c[0] for c in WHOLE])
def test_whole_volume_equals_the_export_and_the_oracle(name, kind, field, N, max_blocks):
    W, H = (160, 120) if N == 256 else (320, 240)
    s, gpu, cpu = _device(kind, field, N, max_blocks, W, H, 6 if N < 1024 else 4, oracle=True)
    try:
        export = gpu.mesh()
        res = gpu.mesh_blocks()
        assert len(export) > 1000
        assert len(res["triangles"]) == len(export)             # the header's total = se_hip_mesh_count
        assert L.same_triangle_set(res["triangles"], export)
        assert L.same_triangle_set(res["triangles"], cpu.mesh())
        allocated = gpu.blocks()[0]
        listed = _check_structure(gpu, res, N, allocated, False)
        assert listed == {tuple(c) for c in allocated.tolist()}      # every allocated block, empty ones with count 0
        skip = gpu.mesh_blocks(skip_empty=True)
        _check_structure(gpu, skip, N, allocated, True)
        full = L.by_coords(res)
        assert L.by_coords(skip) == {c: p for c, p in full.items() if p}
    finally:
        gpu.close(); cpu.close()


@pytest.mark.parametrize("field,max_blocks", [(SDF, 0), (OFUSION, 1 << 17), (SDF, 1 << 17)], ids=["sdf_dense", "ofusion_pooled", "sdf_pooled"])
def test_payloads_are_a_function_of_the_map(field, max_blocks):
    """Two calls give byte-identical per-block payloads, and each equals the payload rebuilt on the host from the downloaded bricks in the
    defined order (cells x fastest, then y, then z; a cell's triangles in table order)."""
    N = 256
    s, gpu, _ = _device("stress", field, N, max_blocks, 160, 120, 8)
    try:
        a, b = L.by_coords(gpu.mesh_blocks()), L.by_coords(gpu.mesh_blocks())
        assert a == b and sum(len(p) for p in a.values()) > 0
        assert L.by_coords({k: v.cpu().numpy() for k, v in gpu.mesh_blocks(device=True).items()}) == a
        coords, x, y, _ = gpu.blocks()
        with_tris = sorted(c for c, p in a.items() if p)
        without = sorted(c for c, p in a.items() if not p)
        want = with_tris[:: max(1, len(with_tris) // 150)] + without[:: max(1, len(without) // 20)]
        # (blocks at the volume's low faces, where vertices are rejected, if the stream reaches them)
        want += [c for c in with_tris if min(c) == 0][:10]
        host = L.rebuild_payloads(coords, x, y, N, DIM, want=want)
        bad = [c for c in want if host[c].tobytes() != a[c]]
        assert not bad, (len(bad), bad[:3])
    finally:
        gpu.close()


def test_regions_select_exactly_the_intersecting_blocks():
    N = 256
    s, gpu, _ = _device("stress", SDF, N, 0, 160, 120, 8)
    try:
        full = L.by_coords(gpu.mesh_blocks())
        some = sorted(c for c, p in full.items() if p)[len(full) // 7]
        boxes = [(some, tuple(v + 8 for v in some)), (tuple(v + 7 for v in some), tuple(v + 9 for v in some)), ((0, 0, some[2] - 3), (N, N, some[2] + 14)),
                 ((-50, 90, -3), (140, 10**6, N + 77)), ((0, 0, 0), (N, N, N)), ((100, 100, 100), (100, 200, 200)),
                 ((120, 0, 0), (60, N, N)), ((-100, -100, -100), (0, 0, 0)), ((N, 0, 0), (N + 8, N, N))]
        # slabs cut by each face of the volume (40 voxels thick, reaching 10 beyond the face)
        faces = [(tuple(-10 if a == ax else 0 for a in range(3)), tuple(40 if a == ax else N for a in range(3))) for ax in range(3)] + \
                [(tuple(N - 40 if a == ax else 0 for a in range(3)), tuple(N + 10 if a == ax else N for a in range(3))) for ax in range(3)]
        n_nonempty, n_face = 0, 0
        for i, (lo, hi) in enumerate(boxes + faces):
            got = L.by_coords(gpu.mesh_blocks(region=(lo, hi)))
            exp = {c: p for c, p in full.items() if all(c[a] < hi[a] and c[a] + 8 > lo[a] for a in range(3))}
            assert got == exp, (lo, hi, len(got), len(exp))
            n_nonempty += bool(exp) and i < 5
            n_face += bool(exp) and i >= len(boxes)
        assert n_nonempty == 5 and n_face >= 1, (n_nonempty, n_face)
        assert len(L.by_coords(gpu.mesh_blocks(region=boxes[0]))) == 1 and len(L.by_coords(gpu.mesh_blocks(region=boxes[1]))) <= 8
    finally:
        gpu.close()


VIEWS = [("sdf_256", SDF, 256, 160, 120, 60), ("ofusion_256", OFUSION, 256, 160, 120, 40), ("sdf_512", SDF, 512, 640, 480, 30)]


@pytest.mark.parametrize("name,field,N,W,H,frames", VIEWS, ids=[c[0] for c in VIEWS])
def test_livemesh_follows_the_map_through_views(name, field, N, W, H, frames):
    """Stress stream, an update every 10 frames with those frames' views: LiveMesh equals the export after every update (nothing changed
    was missed); every block the device selects passes the float64 restatement loosened to 12 voxels and a 2-pixel border; and at the
    last update of the 60-frame 256^3 SDF stream the selection omits at least 10 % of the allocated blocks."""
    s = make_stream("stress", W, H, DIM, holes=False)
    gpu = DenseSLAMPipeline((W, H), N, DIM, field_type=field)
    live, views = LiveMesh(), []
    try:
        for f in range(frames):
            _integrate(gpu, s, f, _mu(field))
            views.append((np.asarray(s.pose(f), np.float32), np.asarray(s.k, np.float32)))
            if (f + 1) % 10:
                continue
            res = gpu.mesh_blocks(views=views)
            loose = L.possibly_touched(res["coords"], [L.view_of(p, k, W, H) for p, k in views], N, DIM, radius=12.0, border=2.0)
            assert loose.all(), (f, int((~loose).sum()))
            allocated = gpu.blocks()[0]
            rule = L.possibly_touched(allocated, [L.view_of(p, k, W, H) for p, k in views], N, DIM)
            got = {tuple(c) for c in res["coords"].tolist()}
            print(f"frame {f}: allocated {len(allocated)} selected {len(got)} float64 rule {int(rule.sum())}")
            live.update(gpu, views)
            assert L.same_triangle_set(live.triangles(), gpu.mesh()), f
            views = []
        if name == "sdf_256":
            assert len(got) <= 0.9 * len(allocated), (len(got), len(allocated))
    finally:
        gpu.close()


def _raw_host(gpu, sel, cap_t, cap_b):
    head = np.full(4, -7, np.int64)
    tris, coords, ranges = np.full((max(cap_t, 1), 9), np.nan, np.float32), np.full((max(cap_b, 1), 3), -1, np.int32), np.full((max(cap_b, 1), 2), -1, np.int64)
    out = _MeshOut(tris.ctypes.data if cap_t else None, cap_t, coords.ctypes.data if cap_b else None, ranges.ctypes.data if cap_b else None, cap_b, head.ctypes.data)
    rc = gpu.lib.se_hip_mesh_blocks_host(gpu._h, C.byref(sel), C.byref(out))
    return rc, head, tris, coords, ranges


def test_capacities():
    N = 256
    s, gpu, _ = _device("room", SDF, N, 0, 160, 120, 5)
    try:
        sel, keep = gpu._mesh_select(None, None, False)
        full = L.by_coords(gpu.mesh_blocks())
        rc, head, *_ = _raw_host(gpu, sel, 0, 0)                       # the sizing call
        nb, nt = int(head[0]), int(head[1])
        assert rc == 0 and nb == len(full) and nt == sum(len(p) for p in full.values()) // 36 and head[2] == 0 and head[3] == 0
        for cap_t, cap_b in ((nt, nb), (nt + 5, nb + 5), (nt - 1, nb), (nt // 2, nb), (nt, nb - 1), (nt, nb // 3), (0, nb), (nt, 0), (1, 1)):
            rc, head, tris, coords, ranges = _raw_host(gpu, sel, cap_t, cap_b)
            fits = cap_t >= nt and cap_b >= nb
            assert rc == (0 if fits else -3), (cap_t, cap_b, rc)
            assert head[0] == nb and head[1] == nt and head[2] <= cap_b and head[3] <= cap_t, (cap_t, cap_b, head)
            wb, wt = int(head[2]), int(head[3])
            assert (wb, wt) == (nb, nt) if fits else (wb < nb)
            # whole blocks only: the written rows' ranges tile [0, wt) and each payload is the block's
            r = ranges[:wb]
            assert int(r[:, 1].sum()) == wt
            got = {tuple(c): tris[f:f + n].tobytes() for c, (f, n) in zip(coords[:wb].tolist(), r.tolist())}
            assert len(got) == wb and all(full[c] == p for c, p in got.items())
            assert np.isnan(tris[wt:]).all() and (coords[wb:] == -1).all()      # nothing beyond what the header says
        assert gpu.mesh_blocks() and L.by_coords(gpu.mesh_blocks()) == full        # the handle works afterwards
        _integrate(gpu, s, 5, 0.1)
        assert L.same_triangle_set(gpu.mesh_blocks()["triangles"], gpu.mesh())
    finally:
        gpu.close()


@pytest.mark.parametrize("field,max_blocks", [(SDF, 0), (OFUSION, 1 << 15)], ids=["sdf_dense", "ofusion_pooled"])
def test_calls_between_streamed_frames(field, max_blocks):
    """A streaming handle (one-queue schedule, image ring, every frame's raycast deferred into the next frame's scan launch): mesh_blocks
    through both entries after every frame, with that frame's raycast still held back, launches nothing counted, leaves the deferral in
    place and the timing sums alone; every ring slot and the final map stay bit-exact with the oracle, and the last mesh equals the oracle's."""
    import torch
    from supereight_amd.synthetic import to_colmajor
    from tests.parity_util import compare_raycast
    W, H, N, frames = 320, 240, 512, 7
    mu = _mu(field)
    s = make_stream("room", W, H, DIM, holes=False)
    depths = [s.depth(f) for f in range(frames)]
    poses = [s.pose(f) for f in range(frames)]
    dev = torch.from_numpy(np.stack(depths)).cuda()
    k = np.ascontiguousarray(s.k, np.float32)

    def run(with_calls):
        gpu = DenseSLAMPipeline((W, H), N, DIM, field_type=field, max_blocks=max_blocks)
        ring = torch.zeros((frames, 2, H, W, 3), dtype=torch.float32, device="cuda")
        gpu.set_image_ring(ring.data_ptr(), frames, keepalive=ring)
        assert gpu.set_streaming(True)
        gpu.launch_counts(reset=True)
        n_pend, last, held = 0, None, []
        for f in range(frames):
            assert gpu.frame(dev[f].data_ptr(), to_colmajor(poses[f]), k, mu, f) == (3 if f > 2 else 1)
            if with_calls:
                n = gpu.launch_counts()
                last = gpu.mesh_blocks(views=[(poses[f], k)])                 # the host entry
                nb, nt = len(last["coords"]), len(last["triangles"])
                # the device entry with raw pointers: enqueued only, read after the last frame
                t = torch.empty((max(nt, 1), 9), dtype=torch.float32, device="cuda"); c = torch.empty((max(nb, 1), 3), dtype=torch.int32, device="cuda")
                r = torch.empty((max(nb, 1), 2), dtype=torch.int64, device="cuda"); h = torch.zeros(4, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                sel, keep = gpu._mesh_select(None, [(poses[f], k)], False)
                assert gpu.lib.se_hip_mesh_blocks(gpu._h, C.byref(sel), C.byref(_MeshOut(t.data_ptr(), nt, c.data_ptr(), r.data_ptr(), nb, h.data_ptr()))) == 0
                assert gpu.launch_counts() == n, f
                n_pend += n["pending"]
                held.append((last, t, c, r, h))
        n = gpu.launch_counts()
        assert n["fused"] == frames - 4 and n["raycast"] == frames - 4, n
        if with_calls:
            assert n_pend >= frames - 3
            gpu.sync()
            for host, t, c, r, h in held:
                nb, nt = len(host["coords"]), len(host["triangles"])
                assert h.tolist() == [nb, nt, nb, nt]
                assert L.by_coords({"coords": c.cpu().numpy()[:nb], "ranges": r.cpu().numpy()[:nb], "triangles": t.cpu().numpy()[:nt]}) == L.by_coords(host)
            last = gpu.mesh_blocks()
        gpu.sync()
        return gpu, ring.cpu().numpy(), n, last

    cpu = OraclePipeline(field, N, DIM, W, H)
    gpu0, ring0, n0, _ = run(False)
    gpu1, ring1, n1, last = run(True)
    try:
        assert n0 == n1
        assert (ring0.view(np.uint32) == ring1.view(np.uint32)).all()
        for f in range(frames):
            cpu.integrate(depths[f], poses[f], s.k, mu, f)
            ran, v_c, n_c = cpu.raycast(poses[f], s.k, mu, f)
            if f >= 3:
                assert ran
                r = compare_raycast({"v_c": v_c, "n_c": n_c, "v_g": ring1[f, 0], "n_g": ring1[f, 1]}, DIM / N)
                assert r["hitmask_mismatch"] == 0 and r["vertex_bit_mismatch_px"] == 0 and r["normal_bit_mismatch_px"] == 0, (f, r)
        assert L.same_triangle_set(last["triangles"], cpu.mesh())
        c0, x0, y0, _ = gpu0.blocks()
        c1, x1, y1, _ = gpu1.blocks()
        assert (c0 == c1).all() and (x0.view(np.uint32) == x1.view(np.uint32)).all() and (y0.view(np.uint32) == y1.view(np.uint32)).all()
    finally:
        gpu0.close(); gpu1.close(); cpu.close()


def test_calls_disturb_nothing_on_a_synchronous_handle():
    s, gpu, _ = _device("room", SDF, 512, 0, 320, 240, 4)
    try:
        gpu.enable_timing(True)
        before, t0, n0 = map_state(gpu), gpu.timings(), gpu.launch_counts()
        view = [(np.asarray(s.pose(3), np.float32), s.k)]
        first = L.by_coords(gpu.mesh_blocks(views=view))
        gpu.mesh_blocks(device=True)
        gpu.mesh_blocks(region=((0, 0, 0), (200, 200, 200)), skip_empty=True, device=True)
        assert gpu.launch_counts() == n0
        assert gpu.timings() == t0
        assert all((u == w).all() for u, w in zip(before, map_state(gpu)))
        assert L.by_coords(gpu.mesh_blocks(views=view)) == first and any(first.values())
    finally:
        gpu.close()


@pytest.mark.parametrize("field,max_blocks", [(SDF, 1 << 15), (OFUSION, 0)], ids=["sdf_pooled", "ofusion_dense"])
def test_entry_paths_agree(tmp_path, field, max_blocks):
    """Host entry (numpy) = device entry through torch = device entry with raw pointers = C++ meshBlocks, byte-identical per block."""
    import torch
    from supereight_amd.synthetic import render_depth_mm
    W, H, N, dim, frames, n_views = 160, 120, 256, 2.4, 5, 2
    mu = _mu(field)
    raw, pf, s = write_scene(tmp_path, W, H, dim, frames)
    mm = [render_depth_mm(f, W, H, dim) for f in range(frames)]
    poses = np.stack([s.pose(f) for f in range(frames)]).astype(np.float32)
    p = DenseSLAMPipeline((W, H), N, dim, field_type=field, max_blocks=max_blocks)
    try:
        for f in range(frames):
            p.set_depth_mm(mm[f]); p.setPose(poses[f])
            p.integration(s.k, 1, mu, f)
            p.raycasting(s.k, mu, f)
        lo, hi = 8, N - 24
        kw = dict(region=((lo,) * 3, (hi,) * 3), views=[(poses[f], s.k) for f in range(frames - n_views, frames)], skip_empty=True)
        host = p.mesh_blocks(**kw)
        ref = _payload_dict(host, N, dim)
        assert len(ref) > 20 and len(host["triangles"]) > 500
        tor = p.mesh_blocks(device=True, **kw)
        assert all(isinstance(v, torch.Tensor) and v.device.type == "cuda" for v in tor.values())
        assert _payload_dict({k: v.cpu().numpy() for k, v in tor.items()}, N, dim) == ref
        # raw pointers, exact capacities
        sel, keep = p._mesh_select(kw["region"], kw["views"], True)
        nb, nt = len(host["coords"]), len(host["triangles"])
        t = torch.empty((nt, 9), dtype=torch.float32, device="cuda"); c = torch.empty((nb, 3), dtype=torch.int32, device="cuda")
        r = torch.empty((nb, 2), dtype=torch.int64, device="cuda"); h = torch.zeros(4, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert p.lib.se_hip_mesh_blocks(p._h, C.byref(sel), C.byref(_MeshOut(t.data_ptr(), nt, c.data_ptr(), r.data_ptr(), nb, h.data_ptr()))) == 0
        p.sync()
        assert h.tolist() == [nb, nt, nb, nt]
        assert _payload_dict({"coords": c.cpu().numpy(), "ranges": r.cpu().numpy(), "triangles": t.cpu().numpy()}, N, dim) == ref
        # the C++ mirror
        exe = build_mirror(tmp_path, "mesh_blocks_mirror", "SDF" if field == SDF else "OFusion")
        of = str(tmp_path / "out.bin")
        _, res = run_mirror(exe, [raw, pf, N, dim, mu, n_views, lo, hi, 1, of], timeout=300)
        data = np.fromfile(of, np.uint8)
        hd = data[:32].view(np.int64)
        assert hd.tolist() == [nb, nt, nb, nt]
        o1, o2 = 32 + 12 * nb, 32 + 12 * nb + 16 * nb
        cpp = {"coords": data[32:o1].view(np.int32).reshape(nb, 3), "ranges": data[o1:o2].view(np.int64).reshape(nb, 2), "triangles": data[o2:].view(np.float32).reshape(nt, 9)}
        assert _payload_dict(cpp, N, dim) == ref
        assert f"blocks {nb} triangles {nt}" in res.stdout
    finally:
        p.close()


def _payload_dict(res, N, dim):
    return L.by_coords(res)


def test_entries_refuse_bad_arguments():
    import torch
    p = DenseSLAMPipeline((64, 48), 256, DIM, field_type=SDF)
    lib = p.lib
    try:
        n0 = p.launch_counts()
        hh = np.zeros(4, np.int64)
        hd = torch.zeros(4, dtype=torch.int64, device="cuda")
        buf_h = np.zeros(64, np.int64)
        buf_d = torch.zeros(64, dtype=torch.int64, device="cuda")
        view = _MeshView()
        view.pose[:] = np.eye(4, dtype=np.float32).reshape(16).tolist(); view.k[:] = [50, 50, 32, 24]; view.width, view.height = 64, 48

        def sel(n_views=0, flags=0, views=None, lo=(0, 0, 0), hi=(256, 256, 256)):
            s = _MeshSelect()
            s.lo[:], s.hi[:], s.n_views, s.flags = list(lo), list(hi), n_views, flags
            s.views = views
            return s

        def bad_view(**kw):
            v = _MeshView()
            C.memmove(C.byref(v), C.byref(view), C.sizeof(v))
            for k2, val in kw.items():
                if k2 == "pose0": v.pose[0] = val
                elif k2 == "k0": v.k[0] = val
                elif k2 == "k3": v.k[3] = val
                else: setattr(v, k2, val)
            return C.pointer(v)

        for fn, head, buf in ((lib.se_hip_mesh_blocks_host, hh.ctypes.data, buf_h.ctypes.data), (lib.se_hip_mesh_blocks, hd.data_ptr(), buf_d.data_ptr())):
            good = _MeshOut(None, 0, None, None, 0, head)
            bad = [(None, C.byref(good)), (C.byref(sel()), None), (C.byref(sel()), C.byref(_MeshOut(None, 0, None, None, 0, None))),
                   (C.byref(sel()), C.byref(_MeshOut(None, 4, buf, buf, 1, head))), (C.byref(sel()), C.byref(_MeshOut(buf, 4, None, buf, 1, head))),
                   (C.byref(sel()), C.byref(_MeshOut(buf, 4, buf, None, 1, head))), (C.byref(sel()), C.byref(_MeshOut(buf, -1, buf, buf, 1, head))),
                   (C.byref(sel()), C.byref(_MeshOut(buf, 1, buf, buf, -1, head))), (C.byref(sel(n_views=-1)), C.byref(good)),
                   (C.byref(sel(n_views=65, views=C.pointer(view))), C.byref(good)), (C.byref(sel(n_views=1)), C.byref(good)), (C.byref(sel(flags=2)), C.byref(good))]
            bad += [(C.byref(sel(n_views=1, views=bad_view(**kw))), C.byref(good)) for kw in
                    (dict(pose0=float("nan")), dict(pose0=float("inf")), dict(k0=0.0), dict(k3=float("nan")), dict(width=0), dict(height=-4))]
            for a in bad:
                assert fn(p._h, *a) == -1, a
                assert lib.se_hip_last_error().decode()
            assert fn(None, C.byref(sel()), C.byref(good)) == -1
            # good calls on an empty map, an empty box, negative fy
            assert fn(p._h, C.byref(sel()), C.byref(good)) == 0
            assert fn(p._h, C.byref(sel(lo=(5, 5, 5), hi=(5, 9, 9))), C.byref(good)) == 0
            assert fn(p._h, C.byref(sel(n_views=1, views=bad_view(k3=-24.0))), C.byref(good)) == 0
        p.sync()
        assert hh.tolist() == [0, 0, 0, 0] and hd.tolist() == [0, 0, 0, 0]
        assert p.launch_counts() == n0
        empty = p.mesh_blocks()
        assert empty["coords"].shape == (0, 3) and empty["triangles"].shape == (0, 3, 3)
        with pytest.raises(ValueError):
            p.mesh_blocks(views=[(np.eye(4), [1, 1, 1, 1])] * 65)
    finally:
        p.close()
