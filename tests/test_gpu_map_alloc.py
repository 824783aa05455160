"""Region allocation on the device (se_hip_allocate_boxes / DenseSLAMPipeline.allocate) through the C ABI: block and node sets against the
numpy ancestor-closure truth of tests/test_map_alloc_host.py on fresh maps (SDF and OFusion, dense and pooled, 512^3 and 1024^3, the whole
volume included), values, active flags and counts; bit-for-bit parity with the CPU oracle over the room and stress streams when both are
given the same keys before frame 0 and after frame 3 (eager and streaming schedule); what a fresh map gains (edit, collides, query,
mesh_blocks); an overlapping allocation leaves what existed untouched; new_keys on a second handle; capacity; the schedule."""
import numpy as np
import pytest

from oracle.binding import OraclePipeline
from supereight_amd.pipeline import ALLOC_DTYPE, COLLISION_EMPTY, COLLISION_UNSEEN, OFUSION, SDF, DenseSLAMPipeline, SeHipError
from supereight_amd.synthetic import make_stream
from tests.gpu_state_util import H, W, bits, run_stream, streamed_with
from tests.host_util import LIMIT, box_records, closure_truth, make_keys
from tests.parity_util import compare_maps, compare_raycast

pytestmark = pytest.mark.gpu
INIT = {SDF: (1.0, 0.0), OFUSION: (0.0, 0.0)}    # voxel_traits<T>::initValue()


def _sets(p):
    """block keys, node keys (root included), active flags of the device map"""
    coords, act = p.block_flags()
    code = p.nodes()[0]
    leaf = int(np.log2(p.size)) - 3
    return make_keys(coords, leaf), code, act


def _boxes(n):
    """leaf and coarse levels, overlapping and repeated boxes, clipped, outside, empty, inverted, every invalid rule: (rows, invalid)"""
    leaf = int(np.log2(n)) - 3
    rows = [((40, 40, 40), (104, 72, 57), 0), ((60, 50, 30), (130, 130, 60), 0), ((60, 50, 30), (130, 130, 60), 4), ((40, 40, 40), (104, 72, 57), 0),
            ((0, 0, 0), (n, n, 16), 2), ((0, 0, 0), (8, 8, 8), 0), ((300, 20, 30), (420, 90, 31), 3), ((17, 300, 300), (25, 310, 420), leaf),
            ((n - 20, n - 9, n - 1), (n + 50, n + 50, n + 50), 0), ((-100, -100, -100), (9, 1, 17), 0), ((-5, 200, 200), (3, 280, 210), 3),
            ((n, 0, 0), (n + 8, 8, 8), 0), ((-8, -8, -8), (0, 0, 0), 1), ((10, 10, 10), (10, 40, 40), 0), ((50, 60, 70), (40, 90, 90), 0),
            ((-LIMIT, 200, 200), (LIMIT, 201, 201), 0)]
    bad = [((0, 0, LIMIT + 1), (8, 8, 8), 0), ((-LIMIT - 1, 0, 0), (8, 8, 8), 0), ((0, 0, 0), (8, 2 ** 31 - 1, 8), 0), ((0, 0, 0), (64, 64, 64), -1),
           ((0, 0, 0), (64, 64, 64), leaf + 1), ((200, 200, 200), (264, 264, 264), 0, 1), ((200, 200, 200), (264, 264, 264), 2, 0x80000000)]
    rng = np.random.default_rng(n)
    for _ in range(150):                                     # many small boxes, some partly outside
        lo = rng.integers(-8, n, 3); rows.append((tuple(lo), tuple(lo + rng.integers(1, 24, 3)), 0))
    rows = rows + bad
    order = rng.permutation(len(rows))
    return [rows[i] for i in order], len(bad)


def _check_against_truth(p, field, rec, n_invalid, had_blocks=(), had_nodes=(0,), device=False):
    """Allocates `rec` on p and checks sets, counts, keys, values and flags against the closure truth; then the same call again."""
    import torch
    requested, closure, pairs, invalid = closure_truth(p.size, rec)
    assert invalid == n_invalid
    leaf = int(np.log2(p.size)) - 3
    want_b = set(had_blocks) | {k for k in closure if k & 0x1FF == leaf}
    want_n = set(had_nodes) | {k for k in closure if k & 0x1FF != leaf}
    cap = len(closure) + 8
    if device:
        drec = torch.from_numpy(rec.view(np.int32).reshape(-1, 8).copy()).to("cuda:0")
        counts, keys = p.allocate_records(drec, key_capacity=cap)
        counts, keys = counts.cpu().numpy(), keys.cpu().numpy().view(np.uint64)
    else:
        counts, keys = p.allocate_records(rec, key_capacity=cap)
    bk, nk, act = _sets(p)
    print(f"device={device}: counts {counts.tolist()} blocks {len(bk)} nodes {len(nk)} keys {int(keys[0])}")
    assert len(set(bk.tolist())) == len(bk) and set(bk.tolist()) == want_b
    assert len(set(nk.tolist())) == len(nk) and set(nk.tolist()) == want_n
    assert counts.tolist() == [len(want_b) - len(had_blocks), len(want_n) - len(had_nodes), pairs, n_invalid]
    klist = keys[1:1 + int(keys[0])].tolist()
    assert int(keys[0]) <= cap and len(set(klist)) == len(klist) and set(klist) <= requested - set(had_blocks) - set(had_nodes)
    implied = set(had_blocks) | set(had_nodes)
    for k in klist:
        lvl = k & 0x1FF
        for l in range(lvl, 0, -1):
            implied.add(((k & ~0x1FF) & ~((1 << (3 * (leaf + 3 - l))) - 1)) | l)
    assert implied == want_b | want_n
    if not had_blocks:
        assert (act == 1).all()
    # every voxel and node value is initValue(): an edit that assigns nothing counts the values of class "unseen" (= initValue())
    if not had_blocks:
        c = p.edit(np.array([[0, 0, 0, p.size, p.size, p.size]], np.int32), only="unseen", mode="strict")
        assert c.tolist() == [512 * len(bk), 8 * len(nk), len(bk), 0]
    again, keys2 = p.allocate_records(rec, key_capacity=4)
    assert again.tolist() == [0, 0, pairs, n_invalid] and int(keys2[0]) == 0
    bk2, nk2, act2 = _sets(p)
    assert (bk2 == bk).all() and (nk2 == nk).all() and (act2 == act).all()
    return want_b, want_n


FRESH = [(f, n, m) for f in (SDF, OFUSION) for n in (512, 1024) for m in (0, 1)]


@pytest.mark.parametrize("field,n,pooled", FRESH, ids=[f"{'sdf' if f == SDF else 'ofusion'}_{n}_{'pooled' if m else 'dense'}" for f, n, m in FRESH])
def test_fresh_map_equals_the_closure_truth(field, n, pooled):
    whole = n == 1024
    max_blocks = 0 if not pooled else ((n // 8) ** 3 if whole else 65536)
    p = DenseSLAMPipeline((W, H), n, 4.8, field_type=field, max_blocks=max_blocks)
    try:
        assert ("pooled" in p.memory_info()["layout"]) == bool(pooled)
        rows, n_invalid = _boxes(n)
        rec = box_records(rows)
        had_b, had_n = _check_against_truth(p, field, rec, n_invalid, device=bool(pooled))
        assert len(had_b) > 1000 and len(had_n) > 100
        _, x, y, act = p.blocks()
        _, _, nx, ny = p.nodes()
        ix, iy = np.float32(INIT[field][0]), np.float32(INIT[field][1])
        assert (x == ix).all() and (y == iy).all() and (nx == ix).all() and (ny == iy).all() and (act == 1).all()
        if whole:                                            # one whole-volume box on top: every block of the volume
            rec = box_records([((0, 0, 0), (n, n, n), 0)])
            counts = p.allocate_records(rec)[0]
            cells = (n // 8) ** 3
            nodes = sum(8 ** l for l in range(0, int(np.log2(n)) - 3))
            assert counts.tolist() == [cells - len(had_b), nodes - len(had_n), cells, 0]
            assert p.counts() == (cells, nodes)
            bk, nk, act = _sets(p)
            g = np.arange(n // 8) * 8
            allb = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
            assert (np.sort(bk) == np.sort(make_keys(allb, int(np.log2(n)) - 3))).all() and len(np.unique(nk)) == nodes and (act == 1).all()
            c = p.edit(np.array([[0, 0, 0, n, n, n]], np.int32), only="unseen", mode="strict")
            assert c.tolist() == [512 * cells, 8 * nodes, cells, 0]
            assert p.allocate_records(rec)[0].tolist() == [0, 0, cells, 0]
    finally:
        p.close()


# ------------------------------------------------------------------ oracle parity
def _parity_rows(n):
    return [((0, 0, 0), (8, 8, 8), 0), ((n // 2 - 40, n // 2 - 30, n // 2 - 20), (n // 2 + 37, n // 2 + 21, n // 2 + 50), 0),
            ((n // 4, n // 4, n // 8), (n // 2, n // 2, n // 4), 3), ((n // 2, 10, 10), (n - 9, 70, 90), 0), ((20, n // 2, n // 2), (90, n - 30, n - 11), 2)]


def _parity_rows_mid(n):
    return [((0, 0, 0), (8, 8, 8), 0), ((n // 3, n // 3, n // 3), (n // 3 + 90, n // 3 + 70, n // 3 + 110), 0), ((0, 0, n // 2), (n, n, n // 2 + 1), 4),
            ((n // 2 - 40, n // 2 - 30, n // 2 - 20), (n // 2 + 37, n // 2 + 21, n // 2 + 50), 0)]


PARITY = [("room", SDF, 256, 2.4, 0), ("room", OFUSION, 256, 2.4, 8192 * 4), ("stress", SDF, 512, 4.8, 65536), ("stress", OFUSION, 512, 4.8, 0)]


@pytest.mark.parametrize("streaming", [False, True], ids=["eager", "streaming"])
@pytest.mark.parametrize("kind,field,n,dim,max_blocks", PARITY,
                         ids=[f"{k}_{'sdf' if f == SDF else 'ofusion'}_{n}_{'dense' if m == 0 else 'pooled'}" for k, f, n, _, m in PARITY])
def test_oracle_parity_with_allocations(kind, field, n, dim, max_blocks, streaming):
    """The same keys to OraclePipeline.allocate_keys and to the device, before frame 0 and after frame 3; integration and raycast of every
    frame bit for bit.  Streaming: the raycasts are deferred and land in an image ring; the allocation flushes the one outstanding."""
    import torch
    frames = 6
    mu = 0.1 if field == SDF else 0.02
    s = make_stream(kind, W, H, dim, holes=False)
    cpu = OraclePipeline(field, n, dim, W, H)
    gpu = DenseSLAMPipeline((W, H), n, dim, field_type=field, max_blocks=max_blocks, streaming=streaming)
    try:
        ring = None
        if streaming:
            ring = torch.zeros((8, 2, W * H * 3), dtype=torch.float32, device="cuda:0")
            gpu.set_image_ring(ring.data_ptr(), 8, keepalive=ring)

        def allocate(rows):
            rec = box_records(rows)
            requested, _, pairs, _ = closure_truth(n, rec)
            cpu.allocate_keys(np.asarray(sorted(requested), np.uint64))
            counts = gpu.allocate_records(rec)[0]
            assert counts[2] == pairs and counts[3] == 0 and counts[0] > 0
            m = compare_maps(cpu, gpu)
            assert m["same_block_set"] and m["same_node_set"], m
            assert m["x_mismatch"] == 0 and m["y_mismatch"] == 0 and m["active_mismatch"] == 0 and m["node_x_mismatch"] == 0 and m["node_y_mismatch"] == 0, m

        allocate(_parity_rows(n))
        recs = []
        for f in range(frames):
            depth, pose = s.depth(f), s.pose(f)
            gpu.set_depth(depth); gpu.setPose(pose)
            assert gpu.integration(s.k, 1, mu, f) == cpu.integrate(depth, pose, s.k, mu, f)
            ran_c, v_c, n_c = cpu.raycast(pose, s.k, mu, f)
            ran_g = gpu.raycasting_deferred(s.k, mu, f) if streaming else gpu.raycasting(s.k, mu, f)
            assert ran_c == ran_g
            rec = {"frame": f, "raycast": ran_c, "v_c": v_c, "n_c": n_c}
            if ran_c and not streaming:
                rec["v_g"], rec["n_g"] = gpu.vertex_normal()
            recs.append(rec)
            if f == 3:
                allocate(_parity_rows_mid(n))
        gpu.sync()
        m = compare_maps(cpu, gpu)
        print(m)
        assert m["same_block_set"] and m["same_node_set"], m
        assert m["x_mismatch"] == 0 and m["y_mismatch"] == 0 and m["active_mismatch"] == 0 and m["node_x_mismatch"] == 0 and m["node_y_mismatch"] == 0, m
        rays = 0
        for rec in recs:
            if not rec["raycast"]:
                continue
            if streaming:
                slot = ring[rec["frame"] % 8].cpu().numpy()
                rec["v_g"], rec["n_g"] = slot[0].reshape(H, W, 3), slot[1].reshape(H, W, 3)
            r = compare_raycast(rec, dim / n)
            assert r["hitmask_mismatch"] == 0 and r["vertex_bit_mismatch_px"] == 0 and r["normal_bit_mismatch_px"] == 0, (rec["frame"], r)
            rays += r["hits_gpu"]
        assert rays > 1000
    finally:
        cpu.close(); gpu.close()


# ------------------------------------------------------------------ what a fresh map gains
@pytest.mark.parametrize("field,max_blocks", [(SDF, 0), (SDF, 8192), (OFUSION, 0)], ids=["sdf_dense", "sdf_pooled", "ofusion_dense"])
def test_a_start_volume_can_be_declared_free_on_a_fresh_map(field, max_blocks):
    n, dim = 256, 2.4
    p = DenseSLAMPipeline((W, H), n, dim, field_type=field, max_blocks=max_blocks)
    try:
        box = np.array([[96, 104, 112, 144, 136, 160]], np.int32)          # block-aligned: 6 x 4 x 6 blocks
        cbox = np.array([[96, 104, 112, 48, 32, 48]], np.int32)             # the same box as collides takes it: corner and sides
        nblocks = 6 * 4 * 6
        free = (0.9, 5.0) if field == SDF else (-3.0, 0.5)
        assert p.collides(cbox, mode="strict")[0] == COLLISION_UNSEEN
        assert p.edit(box, *free, only="unseen").tolist() == [0, 0, 0, 0]     # nothing exists: nothing is applied
        assert p.counts() == (0, 1)
        counts = p.allocate(box)
        assert counts.tolist()[0] == nblocks and counts[2] == nblocks and counts[3] == 0 and p.counts()[0] == nblocks
        # query: status bit 1 (block allocated) inside, clear outside; the voxels hold initValue()
        rng = np.random.default_rng(3)
        vin = rng.integers(box[0, :3], box[0, 3:], (500, 3))
        vout = vin + np.array([80, 0, 0])
        pts = lambda v: np.ascontiguousarray(((v.astype(np.float32) + np.float32(0.5)) * (np.float32(dim) / np.float32(n))).astype(np.float32))
        qi = p.query(pts(vin), fine=True, coarse=False, interp=False, grad=False, status=True)
        qo = p.query(pts(vout), fine=False, coarse=False, interp=False, grad=False, status=True)
        assert ((qi["status"] & 2) != 0).all() and ((qo["status"] & 2) == 0).all()
        assert (qi["fine"][:, 0] == np.float32(INIT[field][0])).all() and (qi["fine"][:, 1] == np.float32(INIT[field][1])).all()
        # mesh_blocks: the blocks are listed, without a triangle
        mb = p.mesh_blocks(region=(tuple(int(q) for q in box[0, :3]), tuple(int(q) for q in box[0, 3:])))
        assert len(mb["coords"]) == nblocks and (mb["ranges"][:, 1] == 0).all()
        # the edit that did nothing before now reaches every voxel, and the planner is unblocked
        assert p.collides(cbox, mode="strict")[0] == COLLISION_UNSEEN
        got = p.edit(box, *free, only="unseen", nodes=False)
        assert got.tolist() == [512 * nblocks, 0, nblocks, 0]
        assert p.collides(cbox, mode="strict")[0] == COLLISION_EMPTY
        inner = np.array([[100, 110, 120, 30, 21, 30]], np.int32)
        assert p.collides(inner, mode="strict")[0] == COLLISION_EMPTY
        c = mb["coords"].astype(np.int64)
        assert ((c >= box[0, :3]) & (c < box[0, 3:])).all()
    finally:
        p.close()


# ------------------------------------------------------------------ what existed stays
@pytest.mark.parametrize("kind,field,n,dim,max_blocks", [("room", SDF, 256, 2.4, 0), ("stress", OFUSION, 512, 4.8, 65536)], ids=["room_sdf_dense", "stress_ofusion_pooled"])
def test_an_overlapping_allocation_leaves_what_existed_untouched(kind, field, n, dim, max_blocks):
    p = run_stream(kind, field, n, dim, max_blocks, 5)
    try:
        c0, x0, y0, a0 = p.blocks()
        code0, side0, nx0, ny0 = p.nodes()
        assert len(c0) > 500
        leaf = int(np.log2(n)) - 3
        k0 = make_keys(c0, leaf)
        centre = c0[len(c0) // 2].astype(np.int64)
        rows = [(tuple(centre - 60), tuple(centre + 70), 0), (tuple(centre - 100), tuple(centre + 30), 3), ((0, 0, 0), (n, n, 24), 0),
                (tuple(c0[7].astype(np.int64)), tuple(c0[7].astype(np.int64) + 8), 0)]
        rec = box_records(rows)
        want_b, want_n = _check_against_truth(p, field, rec, 0, had_blocks=k0.tolist(), had_nodes=code0.tolist(), device=True)
        assert len(want_b) > len(k0) and len(want_n) > len(code0)
        c1, x1, y1, a1 = p.blocks()
        code1, side1, nx1, ny1 = p.nodes()
        k1 = make_keys(c1, leaf)
        old = np.isin(k1, k0)
        oldn = np.isin(code1, code0)
        assert old.sum() == len(k0) and oldn.sum() == len(code0)           # both downloads are in key order: the old rows keep their order
        assert (k1[old] == k0).all() and (code1[oldn] == code0).all() and (side1[oldn] == side0).all()
        assert (bits(x1[old]) == bits(x0)).all() and (bits(y1[old]) == bits(y0)).all() and (a1[old] == a0).all()
        assert (bits(nx1[oldn]) == bits(nx0)).all() and (bits(ny1[oldn]) == bits(ny0)).all()
        ix, iy = np.float32(INIT[field][0]), np.float32(INIT[field][1])
        assert (x1[~old] == ix).all() and (y1[~old] == iy).all() and (a1[~old] == 1).all() and (nx1[~oldn] == ix).all() and (ny1[~oldn] == iy).all()
        assert (x0 != ix).any()                                              # the map held fused values
    finally:
        p.close()


# ------------------------------------------------------------------ new_keys on a peer
def test_new_keys_commit_on_a_second_handle():
    import torch
    n = 512
    a = DenseSLAMPipeline((W, H), n, 4.8, field_type=SDF)
    b = DenseSLAMPipeline((W, H), n, 4.8, field_type=SDF, max_blocks=65536)
    c = DenseSLAMPipeline((W, H), n, 4.8, field_type=SDF)
    try:
        rows, _ = _boxes(n)
        boxes = np.array([list(r[0]) + list(r[1]) for r in rows if len(r) == 3 and max(map(abs, r[0] + r[1])) <= LIMIT and 0 <= r[2] <= 6], np.int32)
        level = np.array([r[2] for r in rows if len(r) == 3 and max(map(abs, r[0] + r[1])) <= LIMIT and 0 <= r[2] <= 6], np.int32)
        counts, keys = a.allocate(torch.from_numpy(boxes).to("cuda:0"), torch.from_numpy(level).to("cuda:0"), return_keys=True)
        counts = counts.cpu().numpy()
        assert counts[0] > 1000 and counts[3] == 0 and 0 < len(keys) <= counts[0] + counts[1]
        lst = torch.cat([torch.tensor([len(keys)], dtype=torch.int64, device="cuda:0"), keys])
        torch.cuda.synchronize()
        b.alloc_commit(lst.data_ptr(), 1, len(lst))
        ba, na, aa = _sets(a)
        bb, nb, ab = _sets(b)
        assert (ba == bb).all() and (na == nb).all() and (aa == ab).all() and len(ba) == counts[0] and len(na) == counts[1] + 1
        # a list that is too small still reports the number wanted, and what was written are keys of the list
        rec = np.zeros(len(boxes), ALLOC_DTYPE)
        rec["lo"], rec["hi"], rec["level"] = boxes[:, :3], boxes[:, 3:], level
        counts_c, small = c.allocate_records(rec, key_capacity=5)
        assert counts_c.tolist() == counts.tolist()
        assert int(small[0]) > 5 and len(small) == 6
        full = c.allocate_records(rec, key_capacity=1)[1]
        assert int(full[0]) == 0                             # nothing left to create
        requested = closure_truth(n, rec)[0]
        assert set(small[1:].tolist()) <= requested and len(set(small[1:].tolist())) == 5
    finally:
        a.close(); b.close(); c.close()


# ------------------------------------------------------------------ capacity
def test_a_small_pool_reports_capacity():
    p = DenseSLAMPipeline((W, H), 256, 2.4, field_type=SDF, max_blocks=1024)
    try:
        box = np.array([[0, 0, 0, 128, 128, 128]], np.int32)             # 4 096 blocks into a pool of 1 024
        with pytest.raises(SeHipError):
            p.allocate(box)
        with pytest.raises(SeHipError):                                    # sticky
            p.sync()
        assert p.clear_overflow() == 1
        p.sync()
        nb, nn = p.counts()
        assert nb == 1024
        bk, nk, act = _sets(p)
        assert len(set(bk.tolist())) == 1024 and (act == 1).all()
        assert p.clear_overflow() == 0
    finally:
        p.close()


# ------------------------------------------------------------------ schedule
def test_allocation_flushes_a_deferred_raycast_first():
    """A streaming handle with an image ring and a twin without the allocation: the slot of frame f is the same on both when the allocation
    is issued between frame f and f + 1 (new blocks hold initValue(): the later images are the same too), the launch counters show that
    raycast as a launch of its own, and the allocation itself moves no counter."""
    f = 5
    def blocks(p, log):
        log["blocks"] = p.counts()[0]

    alloc, log = streamed_with(lambda p, box: p.allocate(box), f, at_end=blocks)
    twin, tlog = streamed_with(lambda p, box: p.allocate(box), -1, at_end=blocks)
    assert log["fused"]
    for g in range(f + 1):
        assert (bits(alloc[g]) == bits(twin[g])).all(), g
    b, a, again = log["before"], log["after"], log["again"]
    assert b["pending"] and not a["pending"]
    assert a["raycast"] == b["raycast"] + 1 and a["fused"] == b["fused"]   # launched alone, not with a scan
    assert all(a[k] == b[k] for k in a if k not in ("raycast", "pending"))
    assert again == a
    assert log["counts"][0] > 10000 and log["counts"][3] == 0 and log["blocks"] > tlog["blocks"] + 10000


def test_device_allocation_without_host_synchronisation():
    """Frames, an allocation on device tensors through the C entry, an edit of the new region and a device query, all enqueued without a host
    wait in between; n = 0; the refusals."""
    import torch
    n, dim, mu = 256, 2.4, 0.1
    s = make_stream("room", W, H, dim, holes=False)
    p = DenseSLAMPipeline((W, H), n, dim, field_type=SDF)
    try:
        for f in range(3):
            p.set_depth(s.depth(f)); p.setPose(s.pose(f)); p.integration(s.k, 1, mu, f); p.raycasting(s.k, mu, f)
        nb0 = p.counts()[0]
        rec = box_records([((8, 8, 8), (40, 40, 40), 0)])
        drec = torch.from_numpy(rec.view(np.int32).reshape(-1, 8).copy()).to("cuda:0")
        dcounts = torch.full((4,), -1, dtype=torch.int64, device="cuda:0")
        dkeys = torch.full((100,), -1, dtype=torch.int64, device="cuda:0")
        vox = np.stack(np.meshgrid(np.arange(8, 40, 5), np.arange(8, 40, 5), np.arange(8, 40, 5), indexing="ij"), -1).reshape(-1, 3)
        dpts = torch.from_numpy(np.ascontiguousarray(((vox.astype(np.float32) + np.float32(0.5)) * (np.float32(dim) / np.float32(n))).astype(np.float32))).to("cuda:0")
        torch.cuda.synchronize()
        f = 3
        p.set_depth(s.depth(f)); p.setPose(s.pose(f)); p.integration(s.k, 1, mu, f); p.raycasting(s.k, mu, f)
        assert p.lib.se_hip_allocate_boxes(p._h, drec.data_ptr(), 1, dcounts.data_ptr(), dkeys.data_ptr(), 100) == 0
        st = p.query(dpts, fine=True, coarse=False, interp=False, grad=False, status=True)          # (synchronises once, at its end)
        assert ((st["status"].cpu().numpy() & 2) != 0).all()
        got = dcounts.cpu().tolist()
        assert 0 < got[0] <= 64 and got[2] == 64 and got[3] == 0 and p.counts()[0] >= nb0 + got[0]
        assert int(dkeys[0]) == got[0]
        # frames go on, bit for bit like a twin that was allocated through the host entry
        q = DenseSLAMPipeline((W, H), n, dim, field_type=SDF)
        s2 = make_stream("room", W, H, dim, holes=False)                     # (a stream hands its frames out in order, once)
        for g in range(4):
            q.set_depth(s2.depth(g)); q.setPose(s2.pose(g)); q.integration(s.k, 1, mu, g); q.raycasting(s.k, mu, g)
        assert q.allocate_records(rec)[0].tolist() == got
        for g in range(4, 6):
            depth = s.depth(g)
            for h in (p, q):
                h.set_depth(depth); h.setPose(s.pose(g)); h.integration(s.k, 1, mu, g); h.raycasting(s.k, mu, g)
        for u, w in zip(p.blocks() + p.nodes() + p.vertex_normal(), q.blocks() + q.nodes() + q.vertex_normal()):
            assert (bits(u) == bits(w)).all() if u.dtype == np.float32 else (u == w).all()
        q.close()
        # n == 0: nothing but the outputs, zeroed
        c0, k0 = p.allocate_records(np.zeros(0, ALLOC_DTYPE), key_capacity=3)
        assert c0.tolist() == [0, 0, 0, 0] and int(k0[0]) == 0
        dcounts.fill_(-1); dkeys.fill_(-1)
        assert p.lib.se_hip_allocate_boxes(p._h, None, 0, dcounts.data_ptr(), dkeys.data_ptr(), 100) == 0
        p.sync()
        assert dcounts.cpu().tolist() == [0, 0, 0, 0] and int(dkeys[0]) == 0
        # refusals, before any launch
        before = _sets(p)
        hk = np.zeros(8, np.uint64)
        for fn, addr, kaddr in ((p.lib.se_hip_allocate_boxes_host, rec.ctypes.data, hk.ctypes.data), (p.lib.se_hip_allocate_boxes, drec.data_ptr(), dkeys.data_ptr())):
            for args in ((addr, -1, None, None, 0), (None, 4, None, None, 0), (addr, 1, None, kaddr, 0), (addr, 1, None, kaddr, -5)):
                assert fn(p._h, *args) == -1
            assert fn(p._h, None, 0, None, None, 0) == 0
        assert all((u == w).all() for u, w in zip(before, _sets(p)))
    finally:
        p.close()
