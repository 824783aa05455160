"""Mixed programs of map operations on the device beside one model, step by step, everything bit for bit (tests/op_program_util.py: the
programs, the model -- the CPU oracle for fusion and raycasts, the numpy truths for edit, allocate, shift, merge and load -- and the device
runner; tests/test_op_programs_host.py asserts on the model alone that every program engages).  After EVERY step: block and node sets,
every voxel, both node arrays, the active flags, the counts, what the operation returned; after a frame its raycast; after an operation a
raycast taken at once and the reader battery of op_program_util.check_readers -- 64 box queries (strict collides, clearance), the column
projections, the distance field, moving and oriented boxes, point queries, ray casts and the mesh, against numpy over the class grid of
the model state or the oracle seeded with it -- these read the index, occupancy and beam-start marks the operation left behind, which no
twin handle shares; after a shift tracking is refused, the next frame's raycast is the first, and the battery runs all the same.  One
LiveMesh follows each run as its docstrings direct.  At the end the mesh, the LiveMesh against a fresh one, and the saved file.  Each
program once more on a streaming handle with an image ring, where every operation arrives while the previous frame's raycast is held back
(without the battery).  The staged programs put an operation between se_hip_alloc_scan and se_hip_integrate_sweep (include/se_hip.h,
"between the scan and the sweep").  One case at 1024^3, where the sorted block list and lbits[] exist, beside a twin that loaded the
expected map; it is as it was before the release and the rigid merge became step kinds (the dense resampling truth is about 8 GB there)."""
import numpy as np
import pytest

from supereight_amd.mapio import load_octree
from supereight_amd.pipeline import OFUSION, SDF, DenseSLAMPipeline, SeHipError
from supereight_amd.synthetic import make_stream
from tests import op_program_util as P
from tests import time_axis_util as T
from tests.gpu_state_util import bits, run_stream
from tests.host_util import make_keys
from tests.live_mesh_util import same_triangle_set
from tests.merge_util import FUSE, counts_of, merge_truth
from tests.op_program_util import H, K, MU, W
from tests.shift_util import equal_blocks_nodes, leaf_level, shift_truth, write_map_file

pytestmark = pytest.mark.gpu
FIELD_IDS = {SDF: "sdf", OFUSION: "ofusion"}
# (program, field) adjacent, so that the model's run with the battery's truths is computed once and shared by the dense and the pooled case
CASES = [(name, f, mb) for name in P.PROGRAMS for f in (SDF, OFUSION) for mb in (0, P.POOL)]
IDS = [f"{n}-{FIELD_IDS[f]}-{'pooled' if mb else 'dense'}" for n, f, mb in CASES]
TWINS = [(name, f) for name in P.PROGRAMS for f in (SDF, OFUSION)]


def _op(rec):
    return rec["inner"] if rec["kind"] == "staged" else rec


def _check_returned(j, rec, got):
    o = _op(rec)
    if o.get("counts") is not None:
        assert got is not None and np.asarray(got).tolist() == o["counts"].tolist(), (j, o["kind"], np.asarray(got).tolist(), o["counts"].tolist())


def _check_file(gpu, field, state, tmp_path):
    path = str(tmp_path / "end.bin")
    gpu.save(path)
    f = load_octree(path, "sdf" if field == SDF else "ofusion")
    c, x, y, _, code, side, nx, ny = state
    assert f["size"] == P.N and np.float32(f["dim"]) == np.float32(P.DIM)
    assert (f["blocks"]["coords"] == c).all() and (f["blocks"]["code"] == make_keys(c, leaf_level(P.N))).all()
    assert (f["nodes"]["code"] == code).all() and (f["nodes"]["side"] == side.astype(np.int32)).all()
    for got, want in ((f["blocks"]["voxels"], (x, y)), (f["nodes"]["value"], (nx, ny))):
        assert (bits(got["x"]) == bits(want[0])).all()
        assert (got["y"] == want[1]).all() and (bits(got["y"].astype(np.float32)) == bits(want[1])).all()


@pytest.mark.parametrize("name,field,max_blocks", CASES, ids=IDS)
def test_a_program_follows_the_model_after_every_step(name, field, max_blocks, tmp_path):
    recs, summary = P.model_run(name, field)
    mu = MU[field]
    asked = [r["queries"] for r in recs if "queries" in r]
    if asked:      # the batch meets all three classes, distances that are found and are not zero, and boxes with nothing occupied in reach
        assert {0, 1, 2} <= set(np.concatenate([q[0] for q in asked]).tolist())
        assert all(any((q[1][stop][0] > 0).any() for q in asked) for stop in ("occupied", "unseen"))
        assert any((q[1]["occupied"][0] < 0).any() for q in asked)

    live = P.TrackedLiveMesh()

    def check(j, rec, gpu, got):
        tag = (name, j, rec["kind"], _op(rec)["kind"])
        _check_returned(j, rec, got)
        T.assert_same_state(rec["state"], gpu, tag)
        assert gpu.counts() == rec["counts_after"], tag
        live.follow(gpu, rec)
        ran, v, n = rec["image"]
        if rec["kind"] in ("frame", "staged"):
            if ran:
                T.assert_same_images(v, n, *gpu.vertex_normal(), tag, min_hits=50)
            return
        if rec["kind"] == "shift":
            # the images predate the shift: no tracking until a raycast has run -- the next frame's, the first after the shift; no
            # reader is barred
            with pytest.raises(SeHipError, match="vertex / normal images predate a map shift"):
                gpu.tracking(K, 1e-5, 1, rec["number"])
        else:
            gpu.setPose(rec["pose"])
            assert gpu.raycasting(K, mu, rec["number"]) == ran
            if ran:
                T.assert_same_images(v, n, *gpu.vertex_normal(), tag + ("at once",), min_hits=50 if rec["fused_before"] else 0)
        P.check_readers(gpu, rec["readers"], tag)
        T.assert_same_state(rec["state"], gpu, tag + ("after the readers",))

    gpu, sources = P.run_on_device(name, field, max_blocks, False, check, tmp_path)
    try:
        assert ("pooled" in gpu.memory_info()["layout"]) == bool(max_blocks)
        assert gpu.clear_overflow() == 0
        if max_blocks and name in ("pool_churn", "pool_churn_release"):
            assert summary["created"] > gpu.memory_info()["brick_slots"] >= summary["peak"]          # bricks were handed back and drawn again
        assert same_triangle_set(gpu.mesh(), summary["mesh"]) and (len(summary["mesh"]) > 0 or field == OFUSION)
        print(name, "live mesh: blocks, of them moved by a shift and not meshed since:", live.check_against_fresh(gpu, (name, "end")))
        _check_file(gpu, field, recs[-1]["state"], tmp_path)
    finally:
        gpu.close()
        for p in sources.values():
            p.close()


@pytest.mark.parametrize("name,field", TWINS, ids=[f"{n}-{FIELD_IDS[f]}" for n, f in TWINS])
def test_the_streaming_twin_fills_its_ring_and_ends_in_the_same_map(name, field, tmp_path):
    """Deferred raycasts into an image ring; deferral is re-armed after every operation (two flushed raycasts in a row switch it off,
    include/se_hip.h), so each operation that follows a frame finds that frame's raycast held back and has to launch it first -- the launch
    counters show it -- while the next scan may ride in a raycast's launch.  SDF runs dense, OFusion pooled."""
    import torch
    recs, summary = P.model_run(name, field, False)          # (the reader battery belongs to the eager cases)
    numbers = [r["number"] for r in recs if r["kind"] in ("frame", "staged")]
    slots = T.ring_slots(numbers)
    box, seen = {}, {"held": 0}

    def ring(gpu):
        box["ring"] = torch.zeros((slots, 2, H, W, 3), dtype=torch.float32, device="cuda")
        gpu.set_image_ring(box["ring"].data_ptr(), slots, keepalive=box["ring"])
        assert gpu.frame_is_fused()

    def before(j, rec, gpu):
        box["counts"] = gpu.launch_counts()
        prev = recs[j - 1] if j else None
        held = rec["kind"] != "staged" and prev is not None and prev["kind"] in ("frame", "staged") and prev["image"][0]
        assert box["counts"]["pending"] == bool(held), (name, j, box["counts"])          # (staged: the scan took the raycast with it)
        seen["held"] += bool(held)

    def check(j, rec, gpu, got):
        if rec["kind"] == "frame":
            return
        _check_returned(j, rec, got)
        if rec["kind"] != "staged":
            c0, c1 = box["counts"], gpu.launch_counts()
            assert not c1["pending"] and c1["raycast"] == c0["raycast"] + (1 if c0["pending"] else 0), (name, j, c0, c1)
            assert c1["fused"] == c0["fused"] and c1["integrate"] == c0["integrate"] and c1["alloc_scan"] == c0["alloc_scan"], (name, j, c0, c1)
            assert gpu.set_streaming(True)

    gpu, sources = P.run_on_device(name, field, P.POOL if field == OFUSION else 0, True, check, tmp_path, ring=ring, before=before, queries=False)
    try:
        assert seen["held"] >= 1 or name.startswith("staged")          # an operation met a held-back raycast
        assert gpu.launch_counts()["fused"] >= 1
        gpu.sync()
        out = box["ring"].cpu().numpy()
        used = set()
        for r in recs:
            if r["kind"] in ("frame", "staged"):
                s = r["number"] % slots
                used.add(s)
                if r["image"][0]:
                    T.assert_same_images(r["image"][1], r["image"][2], out[s, 0], out[s, 1], (name, r["number"], s), min_hits=50)
                else:
                    assert not out[s].any(), (name, r["number"])
        for s in set(range(slots)) - used:
            assert not out[s].any(), s
        T.assert_same_state(recs[-1]["state"], gpu, (name, "end"))
        assert gpu.counts() == recs[-1]["counts_after"] and gpu.clear_overflow() == 0
        assert same_triangle_set(gpu.mesh(), summary["mesh"])
    finally:
        gpu.close()
        for p in sources.values():
            p.close()


@pytest.mark.parametrize("field", [SDF, OFUSION], ids=["sdf", "ofusion"])
def test_a_merge_from_a_source_between_its_scan_and_its_sweep(field):
    """The SOURCE handle has scanned its next frame (alloc_scan: the blocks exist, hold initValue() and are active) and not yet swept it when
    the destination merges from it; afterwards the source sweeps and raycasts that frame.  Both against models that do the same."""
    base, mu, s = P.base_frame(field), MU[field], (16, 0, -8)
    dm, sm = P.Model(field), P.Model(field)
    dst = DenseSLAMPipeline((W, H), P.N, P.DIM, field_type=field, max_blocks=P.POOL)
    src = DenseSLAMPipeline((W, H), P.N, P.DIM, field_type=field)
    try:
        for m, p, first in ((dm, dst, 0), (sm, src, 40)):
            for j in range(4):
                m.frame(first + j, base + j)
                p.set_depth(P.stream(first + j)[0]); p.setPose(m.pose(first + j))
                assert p.integration(K, 1, mu, base + j)
                p.raycasting(K, mu, base + j)
        i, number = 52, base + 4                                # three degrees further on: the scan inserts blocks
        nb = sm.counts()[0]

        def between():
            assert sm.counts()[0] > nb
            return dm.merge(P.N, sm.state(), s, "fuse")
        (counts, seen), (ran, v, n) = sm.staged_frame(i, number, between)
        assert counts[0] > 0 and counts[1] > 0 and seen > 0
        src.set_depth(P.stream(i)[0]); src.setPose(sm.pose(i))
        assert src.alloc_scan(K, 1, mu, number)
        assert counts_of(dst.merge(src, s)).tolist() == counts.tolist()
        T.assert_same_state(dm.state(), dst, "dst after the merge")
        assert src.integrate_sweep(K, 1, mu, number) and src.raycasting(K, mu, number) == ran
        T.assert_same_images(v, n, *src.vertex_normal(), "src after its sweep", min_hits=50)
        T.assert_same_state(sm.state(), src, "src after its sweep")
        _, v, n = dm.frame(4, number)                           # and the destination goes on
        dst.set_depth(P.stream(4)[0]); dst.setPose(dm.pose(4))
        assert dst.integration(K, 1, mu, number) and dst.raycasting(K, mu, number)
        T.assert_same_images(v, n, *dst.vertex_normal(), "dst after a frame", min_hits=50)
        T.assert_same_state(dm.state(), dst, "dst after a frame")
        assert dm.stats_truncated() == 0 and sm.stats_truncated() == 0
    finally:
        dm.close(); sm.close(); dst.close(); src.close()


def test_one_program_at_1024(tmp_path):
    """Dense SDF at 1024^3 over the stress stream: 3 frames, shift, merge, allocate, 2 frames -- the sizes at which the block list is kept
    address-ordered and lbits[] is consulted.  The oracle is too slow there for a model per step: the state after the three operations is
    compared with the numpy truths chained on the download taken before them, and the two frames that follow run beside a twin handle that
    loaded that expected map from a file (as test_frames_after_a_shift_at_1024 does): images after each frame, the maps at the end.
    (About as long as that test: two dense 1024^3 handles and two downloads of the map.)"""
    n, dim, mu, pre, post = 1024, 4.8, 0.1, 3, 2
    s, ms = (-128, 0, 64), (-120, 0, 56)
    rows = [((256, 256, 256), (384, 384, 384), 0), ((0, 0, 512), (512, 512, 1024), 3)]          # 4096 blocks; 64 childless nodes of side 128
    init = P.INIT[SDF]
    a = run_stream("stress", SDF, n, dim, 0, pre)
    src = run_stream("stress", SDF, n, dim, 65536, pre + 2)
    b = DenseSLAMPipeline((W, H), n, dim, field_type=SDF)
    try:
        before = a.blocks() + a.nodes()
        src_state = src.blocks() + src.nodes()
        blocks, nodes, c_shift = shift_truth(n, s, before[:4], before[4:], init)
        blocks, nodes, c_merge = merge_truth(n, blocks, nodes, n, src_state[:4], src_state[4:], ms, FUSE, SDF)
        want, c_alloc = P.allocate_truth(n, blocks + nodes, rows, init)
        assert c_shift[0] > 0 and c_shift[1] > 0 and c_merge[0] > 0 and c_merge[1] > 0 and c_alloc[0] > 0 and c_alloc[1] > 0
        assert before[3].min() == 0 and before[3].max() == 1
        assert a.shift(s).tolist() == c_shift.tolist()
        assert counts_of(a.merge(src, ms)).tolist() == c_merge.tolist()
        assert a.allocate_records(P.box_records(rows))[0].tolist() == c_alloc.tolist()
        assert equal_blocks_nodes(a.blocks(), a.nodes(), want[:4], want[4:]) is None
        print("1024^3:", c_shift.tolist(), c_merge.tolist(), c_alloc.tolist(), a.counts())
        assert a.counts()[0] >= 4096                            # from 4096 blocks on the next sweep sorts the block list
        path = str(tmp_path / "expected.bin")
        write_map_file(path, n, dim, SDF, want[:4], want[4:])
        b.load(path)
        move = np.asarray(s, np.float32) * (np.float32(dim) / np.float32(n))
        sa = make_stream("stress", W, H, dim, holes=False)
        for f in range(pre):
            sa.depth(f)                                        # (the stream hands out frames in order)
        for f in range(pre, pre + post):
            depth, pose = sa.depth(f), sa.pose(f).copy()
            pose[:3, 3] += move
            images = []
            for p in (a, b):
                p.set_depth(depth); p.setPose(pose)
                assert p.integration(sa.k, 1, mu, f) and p.raycasting(sa.k, mu, f)
                images.append([bits(v) for v in p.vertex_normal()])
            assert all((u == w).all() for u, w in zip(*images)) and images[0][0].any(), f
        assert equal_blocks_nodes(a.blocks(), a.nodes(), b.blocks(), b.nodes()) is None and a.counts() == b.counts()
    finally:
        a.close(); src.close(); b.close()
