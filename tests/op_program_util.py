"""Mixed programs of map operations -- frames, edit, allocate, shift, merge, rigid merge, release, save / load -- followed step by step by
one model, and the same steps on a device handle.

The model is the CPU oracle for depth fusion and raycasts and the numpy truths of the single operations for everything else
(tests/edit_util.truth, host_util.closure_truth, shift_util.shift_truth, merge_util.merge_truth, merge_rigid_util.merge_rigid_truth,
release_util.release_truth).  Where the oracle cannot perform an
operation itself (shift, merge, load) a fresh oracle is seeded with the expected map: insert_octants(node codes of level > 0 and the block
keys), set_values(blocks, nodes), activate().  (insert_octants is Octree::insert per key: allocate_keys would add the keys[0] chain of
unique_multiscale below a childless node that comes first in key order, which none of the device's map operations creates.)  The oracle has no way to clear an active flag, so a seeded oracle holds every block active;
the model keeps the expected flags beside it until the next sweep, which visits the extra blocks, finds no voxel of theirs in the image,
changes nothing and clears their flags (tests/test_op_programs_host.py checks this splice on the oracle alone).

Shapes: those of tests/time_axis_util.py -- the room stream at 160x120 into 128^3, dim 1.2, MU per field; OFusion's frame numbers start at
300.  Stream index i supplies depth and pose; after a shift the pose is moved by the accumulated shift times the voxel size.  Merge sources:
a 128^3 map and a 64^3 map of dim 0.6 (the same voxel size) that fused stream frames 60 .. 63.

A program is a literal list of steps:
    ("frame",)                               integrate + raycast of the next stream frame
    ("shift", s) / ("shift", "node64")       se_hip_shift_map; "node64": the first 64-aligned shift that keeps and drops blocks and under
                                             which a node with a value survives
    ("merge", source, s, mode)               se_hip_merge_map from SOURCES[source]; s = ("registered", d): d beside where the source's frames
                                             saw the content, that is the accumulated shift + the source's origin + d
    ("allocate", rows)                       se_hip_allocate_boxes; rows = [(lo, hi, level)]
    ("edit", kind[, box])                    se_hip_edit_boxes; kind "free" (box declared free), or a kind of time_axis_util.make_edit_list
    ("save_load",)                           se_hip_save_map + se_hip_load_map
    ("release", rows)                        se_hip_release_boxes; rows = [(lo, side, "all" | "unseen")], as DenseSLAMPipeline.release takes them
    ("merge_rigid", source, transform, mode) se_hip_merge_map_rigid from SOURCES[source] under RIGID[transform], registered: composed with the
                                             accumulated shift and the source's origin, so that the content lands where its frames saw it
    ("staged", step)                         alloc_scan, `step`, integrate_sweep, raycast of the next stream frame

After every operation that is not staged the model also records the truths of the reader battery (reader_truth): every batched reader of the
map asked about the places the operation touched; check_readers holds the device to them."""
import functools

import numpy as np

from supereight_amd.pipeline import EDIT_BLOCKS, EDIT_DTYPE, EDIT_NODES, EDIT_SET_X, EDIT_SET_Y, OFUSION, SDF
from supereight_amd.synthetic import intrinsics, pose as stream_pose, render_depth_mm
from tests import edit_util, field_util, map_query_util, motion_util, oriented_util, project_util, release_util
from tests import ray_cast_util as RC
from tests import time_axis_util as T
from tests.clearance_util import clearance_truth
from tests.gpu_state_util import bits
from tests.host_util import box_records, closure_truth, make_keys, unpack
from tests.merge_rigid_util import merge_rigid_truth, rotation
from tests.merge_util import MODES, both_observed, merge_truth
from tests.shift_util import leaf_level, shift_truth, survivors
from tests.time_axis_util import DIM, H, MU, N, W

POOL = 2048
INIT = edit_util.INIT
K = intrinsics(W)
VOXEL = np.float32(DIM) / np.float32(N)
SRC_FRAMES = (60, 61, 62, 63)                 # 12 degrees of yaw further along the trajectory
SRC64_ORIGIN = (32, 32, 64)                   # where the 64^3 source's corner lies in the destination's voxels: the cube round the far wall
SOURCES = {"src128": (128, DIM, (0, 0, 0)), "src64": (64, DIM / 2, SRC64_ORIGIN)}
FREE = {SDF: (0.9, 5.0), OFUSION: (-3.0, 0.5)}
# the rigid motions of ("merge_rigid", ...): a rotation about the volume centre and a sub-voxel translation, in the frame of the stream poses
RIGID = {"yaw": (rotation((0, 1, 0), 7.0), (0.3, -0.2, 0.4)), "general": (rotation((1, 2, 3), 5.0), (-0.4, 0.25, 0.35))}


def rigid_pull(transform, source, offset):
    """src_from_dst of RIGID[transform] for a destination whose accumulated shift is `offset` and the source's origin, float32 [12]: a
    destination voxel v lies at v - offset in the frame of the stream poses, the source voxel u at u + origin, and v - offset =
    R (u + origin - c) + c + tau.  Float64 throughout, rounded to float32 once: t' = t - R_pull offset."""
    R, tau = RIGID[transform]
    c = np.full(3, (N - 1) / 2.0)
    Ri = np.asarray(R, np.float64).T
    t = Ri @ (-(c + np.asarray(tau, np.float64))) + c - np.asarray(SOURCES[source][2], np.float64)
    t = t - Ri @ np.asarray(offset, np.float64)
    return np.ascontiguousarray(np.concatenate([Ri, t[:, None]], 1), np.float32).reshape(12)


def base_frame(field):
    return T.F0 if field == OFUSION else 0


@functools.lru_cache(maxsize=None)
def stream(i):
    """(depth, pose) of stream index i of the room stream without holes, read-only (SyntheticStream.depth / .pose)."""
    d = np.ascontiguousarray(render_depth_mm(i, W, H, DIM).astype(np.float32) / np.float32(1000.0))
    p = stream_pose(i, DIM)
    d.flags.writeable = p.flags.writeable = False
    return d, p


def moved_pose(i, offset_voxels):
    """The pose of stream index i translated by a whole number of voxels, in binary32."""
    p = stream(i)[1].copy()
    p[:3, 3] += np.asarray(offset_voxels, np.float32) * VOXEL
    return p


def _readonly(st):
    for a in st:
        a.flags.writeable = False
    return st


def class_grid(field, n, state, thr=0.0):
    """classify(Octree::get(v)) at every voxel of the volume, [z][y][x] uint8 (0 occupied, 1 unseen, 2 empty), from a state alone: a voxel of
    an allocated block holds the block's value; elsewhere the value_[child] of the deepest node on its path."""
    coords, x, y, _, code, side, nx, ny = state
    above = field == OFUSION
    g = np.full((n, n, n), 1, np.uint8)
    leaf = leaf_level(n)
    have = set(code.tolist()) | set(make_keys(coords, leaf).tolist())
    level = (code & np.uint64(0x1FF)).astype(np.int64)
    corner = unpack(code & ~np.uint64(0x1FF))
    ncls = edit_util._classes(nx, ny, field, (thr, above)).astype(np.uint8)
    for i in np.argsort(level, kind="stable"):           # coarse first: a deeper node overwrites the region it owns
        h = int(side[i]) // 2
        for j in range(8):
            c = corner[i] + edit_util.DIR[j] * h
            if int(make_keys(c[None], int(level[i]) + 1)[0]) in have:
                continue
            g[c[2]:c[2] + h, c[1]:c[1] + h, c[0]:c[0] + h] = ncls[i, j]
    bcls = edit_util._classes(x, y, field, (thr, above)).astype(np.uint8).reshape(-1, 8, 8, 8)      # [z][y][x] within the block
    for c, b in zip(coords.astype(np.int64), bcls):
        g[c[2]:c[2] + 8, c[1]:c[1] + 8, c[0]:c[0] + 8] = b
    return g


def collides_truth(grid, boxes):
    """The strict box query over a class grid: the min over the voxels of [lo, lo + side), outside the volume unseen."""
    n = grid.shape[0]
    out = np.empty(len(boxes), np.uint8)
    for i, b in enumerate(np.asarray(boxes, np.int64)):
        lo, hi = b[:3], b[:3] + b[3:6]
        a0, a1 = np.clip(lo, 0, n), np.clip(hi, 0, n)
        inside = (a0 < a1).all()
        v = int(grid[a0[2]:a1[2], a0[1]:a1[1], a0[0]:a1[0]].min()) if inside else 1
        if not inside or (a0 != lo).any() or (a1 != hi).any():
            v = min(v, 1)
        out[i] = v
    return out


def query_boxes(seed=11):
    """The fixed batch of 64 boxes (lo xyz, side xyz) and their r_max: 48 round where the room stream puts content -- the sphere, the far
    wall, the left wall, the free space in front of them -- and 16 anywhere, some across the volume's faces."""
    rng = np.random.default_rng(seed)
    anchors = np.array([[64, 64, 70], [56, 60, 76], [72, 68, 76], [64, 74, 80], [40, 40, 120], [64, 64, 121], [90, 80, 120], [30, 90, 119],
                        [7, 50, 100], [7, 70, 112], [50, 60, 50], [70, 64, 100]])
    lo = np.concatenate([anchors[rng.integers(len(anchors), size=48)] + rng.integers(-7, 4, (48, 3)), rng.integers(-4, N - 4, (16, 3))])
    side = rng.integers(1, 9, (64, 3))
    r_max = rng.integers(0, 21, 64)
    return np.ascontiguousarray(np.concatenate([lo, side], 1).astype(np.int32)), r_max.astype(np.int32)


def query_truth(field, state, grid=None):
    """(strict collides, {stop_at: (d2, nearest)}) of query_boxes() over the class grid of a state."""
    grid = class_grid(field, N, state) if grid is None else grid
    boxes, r_max = query_boxes()
    out = {}
    for stop, cls in (("occupied", 0), ("unseen", 1)):
        res = [clearance_truth(grid, list(b) + [int(r)], cls) for b, r in zip(boxes.tolist(), r_max.tolist())]
        out[stop] = (np.array([r[0] for r in res], np.int64), np.array([r[1] for r in res], np.int64))
    return collides_truth(grid, boxes), out


# ------------------------------------------------------------------ the reader battery
# Every batched reader of the map, asked after an operation about the places the operation touched: the column projections, the distance
# field, moving and oriented boxes, point queries, ray casts and the mesh.  All of them go through the index, occ[], bpos / npos or lbits,
# the state a shift or a release rebuilds and a merge or an allocation patches in place.  Fixed seeds, bit for bit.
FOOT_LO, FOOT_SIDE = (-5, -5), (138, 138)                                    # overhangs the volume on all four sides
LAYERS = [(0, 128), (-9, 70), (100, 125), (63, 64)]
FIELD_SIDE, FIELD_R = (12, 10, 9), 12
FIELD_CONTENT, FIELD_FACE = (58, 40, 100), (-5, 56, 104)                     # beside the sphere, in front of the far wall (moved with the accumulated shift); across the face x = 0
ROBOTS = ((1, 1, 1), (2, 2, 3))
FIELD_ONLY = np.arange(0, FIELD_SIDE[0] * FIELD_SIDE[1] * FIELD_SIDE[2], 7)  # the truth of every seventh voxel (7 is coprime to 12 and 10: every row, column and layer is met); the device computes the whole region
FAR_AHEAD = 20                                                               # stream indices: a pose no frame of a program has seen the map from


class _Download:
    """A state in the form map_query_util.Map reads a handle's download in."""

    def __init__(self, state):
        self.state = state

    def blocks(self):
        return self.state[:4]

    def nodes(self):
        return self.state[4:]


def field_requests(offset):
    """[(lo, side, robot, r_max)] of the battery for a map whose accumulated shift is `offset`."""
    content = tuple(int(v) for v in np.asarray(FIELD_CONTENT, np.int64) + np.asarray(offset, np.int64))
    return [(lo, FIELD_SIDE, robot, FIELD_R) for lo in (content, FIELD_FACE) for robot in ROBOTS]


def reader_truth(field, state, cpu, offset, region, image, pose, far_pose):
    """What every reader must answer on the map `state`: cpu is the oracle pipeline that holds it (on the library of tests/ray_cast_util.py),
    offset the accumulated shift, region the half-open voxel box the operation touched, image the (ran, vertex, normal) of the raycast
    taken at once from `pose`, far_pose a pose further along the stream.  A dict of inputs and expected outputs, for check_readers."""
    lib, mu = cpu.lib, MU[field]
    grid = class_grid(field, N, state)
    rng = np.random.default_rng(77)
    boxes, _ = query_boxes()
    t = {"field_type": field, "boxes": query_truth(field, state, grid)}
    t["project"] = {(axis, stop): project_util.project_truth(grid, axis, FOOT_LO, FOOT_SIDE, LAYERS, cls)
                    for axis in (0, 1, 2) for stop, cls in project_util.STOPS}
    t["field"] = {(req, stop): field_util.field_truth(grid, req, cls, only=FIELD_ONLY) for req in field_requests(offset) for stop, cls in project_util.STOPS}
    motions = np.ascontiguousarray(np.concatenate([boxes, rng.integers(-24, 25, (len(boxes), 3))], 1).astype(np.int32))
    res = [motion_util.motion_truth(grid, m) for m in motions.tolist()]
    t["motions"] = (motions, np.array([r[0] for r in res], np.uint8),
                    {stop: np.array([motion_util.as_float32(r[k]) for r in res], np.float32) for stop, k in (("occupied", 1), ("unseen", 2))})
    oriented = oriented_util.random_boxes(rng, len(boxes), (2 * boxes[:, :3].astype(np.int64) + boxes[:, 3:]) * (oriented_util.SUB // 2))
    t["oriented"] = (oriented, np.array([oriented_util.oriented_truth(grid, b) for b in oriented], np.uint8))
    # 512 points: at the hit points of the raycast taken at once (uniform where it hit nothing), uniform in the volume, round the region
    ran, v, nrm = image
    hits = v[nrm[..., 0] != -2] if ran else v[:0, 0]
    at = rng.integers(max(len(hits), 1), size=256)
    jitter, anywhere = rng.uniform(-2, 2, (256, 3)) * VOXEL, rng.uniform(0, DIM, (256, 3))
    lo, hi = np.asarray(region[0], np.float64), np.asarray(region[1], np.float64)
    pts = np.concatenate([hits[at] + jitter if len(hits) else anywhere[:256], rng.uniform(0, DIM, (128, 3)), rng.uniform(lo - 6, hi + 6, (128, 3)) * VOXEL])
    pts = np.ascontiguousarray(pts.astype(np.float32))
    m = map_query_util.Map(lib, _Download(state), field, N, DIM)
    try:
        t["query"] = (pts, m.expected(pts))
    finally:
        m.close()
    # 256 rays: every 100th camera ray of the pose of the raycast taken at once, 64 of a pose no frame has looked from
    rays = np.ascontiguousarray(np.concatenate([RC.camera_rays(lib, pose, K, W, H)[::100], RC.camera_rays(lib, far_pose, K, W, H)[37::300]]))
    exp, trips = RC.cast_rays(lib, cpu.h, rays, mu)
    assert trips < 4096 and len(rays) == 256, (trips, len(rays))
    t["rays"] = (rays, exp)
    t["mesh"] = cpu.mesh()
    return t


def reader_figures(truths):
    """What the battery's truths of a program's operations contain, taken together: a dict of sets and counts for the engagement conditions."""
    cat = lambda parts: np.concatenate([np.asarray(p).reshape(-1) for p in parts]) if parts else np.zeros(0, np.int64)
    d2 = cat([f[0] for t in truths for f in t["field"].values()])
    tf = cat([x for t in truths for x in t["motions"][2].values()])
    rs = cat([t["rays"][1]["status"] for t in truths])
    qs = cat([t["query"][1]["status"] for t in truths])
    return {
        "project": set(cat([p["status"] for t in truths for p in t["project"].values()]).tolist()),
        "field": {"zero": int((d2 == 0).sum()), "positive": int((d2 > 0).sum()), "none": int((d2 == field_util.NONE).sum()),
                  "ties": int(sum(f[2].sum() for t in truths for f in t["field"].values()))},
        "t_first": {"zero": int((tf == 0).sum()), "inside": int(((tf > 0) & (tf <= 1)).sum()), "free": int((tf == 2.0).sum())},
        "oriented": set(cat([t["oriented"][1] for t in truths]).tolist()),
        "rays": {"hits": int(((rs & 4) != 0).sum()), "entered_missed": int((((rs & 2) != 0) & ((rs & 4) == 0)).sum())},
        "query": {"allocated": int(((qs & 2) != 0).sum()), "unallocated": int((((qs & 1) != 0) & ((qs & 2) == 0)).sum())},
    }


def check_readers(gpu, truth, tag):
    """Every reader of the battery on the handle against reader_truth's answers, bit for bit."""
    from tests.live_mesh_util import same_triangle_set
    field = truth["field_type"]
    boxes, r_max = query_boxes()
    hits, clear = truth["boxes"]
    assert (gpu.collides(boxes, mode="strict") == hits).all(), tag
    for stop, (d2, near) in clear.items():
        g_d2, g_near = gpu.clearance(boxes, r_max, stop_at=stop)
        assert (g_d2 == d2).all() and (g_near == near).all(), tag + ("clearance", stop)
    for (axis, stop), want in truth["project"].items():
        got = gpu.project(axis, FOOT_LO, FOOT_SIDE, LAYERS, stop_at=stop)
        for k in project_util.OUTPUTS:
            assert got[k].dtype == want[k].dtype and (got[k] == want[k]).all(), tag + ("project", axis, stop, k, int((got[k] != want[k]).sum()))
    for ((lo, side, robot, r), stop), (d2, near, _) in truth["field"].items():
        g_d2, g_near = gpu.distance_field(lo, side, r, robot=robot, stop_at=stop, nearest=True)
        g_d2, g_near = g_d2.reshape(-1)[FIELD_ONLY], g_near.reshape(-1, 3)[FIELD_ONLY]
        assert (g_d2 == d2).all() and (g_near == near).all(), tag + ("distance_field", lo, robot, stop, int((g_d2 != d2).sum()), int((g_near != near).any(1).sum()))
    motions, status, t_first = truth["motions"]
    for stop, want in t_first.items():
        g_status, g_t = gpu.collides_moving(motions, stop_at=stop)
        assert (g_status == status).all() and (bits(g_t) == bits(want)).all(), tag + ("collides_moving", stop, np.nonzero(bits(g_t) != bits(want))[0][:5].tolist())
    oriented, status = truth["oriented"]
    got = gpu.collides_oriented(oriented)
    assert (got == status).all(), tag + ("collides_oriented", np.nonzero(got != status)[0][:5].tolist())
    pts, exp = truth["query"]
    try:
        map_query_util.compare(gpu.query(pts, fine=True, coarse=True, interp=True, grad=True, status=True), exp)
    except AssertionError as e:
        raise AssertionError(tag + ("query",) + e.args) from None
    rays, exp = truth["rays"]
    got = gpu.cast_rays(rays[:, 0:3].copy(), rays[:, 3:6].copy(), rays[:, 6].copy(), rays[:, 7].copy(), mu=float(MU[field]))
    for k in ("hit", "normal", "status"):
        bad = RC.mismatches(got[k], exp[k])
        assert len(bad) == 0, tag + ("cast_rays", k, len(bad), bad[:5].tolist())
    assert same_triangle_set(gpu.mesh(), truth["mesh"]), tag + ("mesh",)


class TrackedLiveMesh:
    """One LiveMesh driven through a run as its docstrings direct, which remembers the blocks that were meshed again since the last shift:
    those are bit-equal to a fresh mesh, the others carry the rounding of LiveMesh.shift's float32 move."""

    def __init__(self):
        from supereight_amd.livemesh import LiveMesh
        self.live, self.exact, self.shifted = LiveMesh(), set(), False

    def update(self, gpu, **kw):
        before = dict(self.live.blocks)                      # (holds the old arrays, so that `is` tells a replaced entry)
        self.live.update(gpu, **kw)
        self.exact |= {c for c, a in self.live.blocks.items() if before.get(c) is not a}
        self.exact &= set(self.live.blocks)

    def region(self, gpu, region):
        lo, hi = region
        self.update(gpu, region=(tuple(int(v) - 1 for v in lo), tuple(int(v) for v in hi)))

    def shift(self, gpu, s):
        self.live.shift(s)
        self.exact, self.shifted = set(), self.shifted or bool(np.any(np.asarray(s) != 0))
        for k in range(3):
            if s[k]:
                lo, hi = [0, 0, 0], [N, N, N]
                lo[k], hi[k] = (N - 9, N) if s[k] > 0 else (0, 8)
                self.update(gpu, region=(tuple(lo), tuple(hi)))

    def follow(self, gpu, rec):
        """After the step of a model record has run on the handle."""
        o = rec["inner"] if rec["kind"] == "staged" else rec
        if o["kind"] == "shift":
            self.shift(gpu, o["s"])
        elif o["kind"] in ("edit", "allocate", "merge", "release", "merge_rigid"):
            self.region(gpu, o["region"])
        if rec["kind"] in ("frame", "staged"):
            self.update(gpu, views=[(rec["pose"], K)])

    def check_against_fresh(self, gpu, tag):
        from supereight_amd.livemesh import LiveMesh
        fresh = LiveMesh()
        fresh.update(gpu)
        assert sorted(self.live.blocks) == sorted(fresh.blocks), tag + ("live mesh blocks", len(self.live.blocks), len(fresh.blocks))
        bound = np.float32(2.0 ** -22)                       # the float32 move of LiveMesh.shift at coordinates below 2 m (DIM = 1.2)
        moved = 0
        for c, want in fresh.blocks.items():
            got = self.live.blocks[c]
            assert got.shape == want.shape, tag + ("live mesh", c)
            if c in self.exact or not self.shifted:
                assert (bits(got) == bits(want)).all(), tag + ("live mesh, meshed since the last shift", c)
            else:
                moved += 1
                assert np.abs(got - want).max() <= bound, tag + ("live mesh, moved", c, float(np.abs(got - want).max()))
        return len(fresh.blocks), moved


# ------------------------------------------------------------------ the model
class Model:
    """An OraclePipeline plus what the oracle does not hold: the accumulated shift, the active flags of a seeded map, the counters of the
    engagement conditions.  origin: where this map's corner lies in the voxels of the frame of reference the stream poses are given in."""

    def __init__(self, field, n=N, dim=DIM, origin=(0, 0, 0)):
        self.field, self.n, self.dim, self.mu = field, n, dim, MU[field]
        self.offset = -np.asarray(origin, np.int64)          # added to the stream poses, in voxels
        self.cpu = None
        self.truncated = 0
        self.created = 0                                     # blocks created so far, by whatever step
        self.peak = 0
        self.last = (0, max(base_frame(field), 3))           # (stream index, frame number) the next immediate raycast uses
        self._flags = None                                   # (sorted block keys, flags) while the oracle's own flags are not the expected ones
        self._fresh()

    def _fresh(self):
        if self.cpu is not None:
            self.truncated += self.cpu.stats()["truncated"]
            self.cpu.close()
        self.cpu = RC.oracle_pipeline(RC.load(), self.field, self.n, self.dim, W, H)          # (so that rco_cast_rays can read it)
        self.cpu.count_stats(True)

    def close(self):
        self.cpu.close()

    def stats_truncated(self):
        return self.truncated + self.cpu.stats()["truncated"]

    # -- state
    def state(self):
        """(coords, x, y, active, code, side, nx, ny) in the order of time_axis_util.snapshot, read-only."""
        c, x, y, a = self.cpu.blocks()
        if self._flags is not None:
            assert (self._flags[0] == make_keys(c, leaf_level(self.n))).all()
            a = self._flags[1].copy()
        return _readonly((c, x, y, a) + tuple(self.cpu.nodes()))

    def counts(self):
        return self.cpu.counts()

    def _note(self, before_blocks):
        nb = self.counts()[0]
        self.peak = max(self.peak, nb)
        return nb

    def seed(self, blocks, nodes):
        """A fresh oracle that holds exactly this map; the expected active flags are kept beside it."""
        coords, x, y, act = blocks
        code, side, nx, ny = nodes
        self._fresh()
        leaf = leaf_level(self.n)
        level = code & np.uint64(0x1FF)
        self.cpu.insert_octants(np.concatenate([code[level > 0], make_keys(coords, leaf)]).astype(np.uint64))
        assert self.cpu.counts() == (len(coords), len(code)), (self.cpu.counts(), len(coords), len(code))
        assert self.cpu.set_values(blocks=(coords, x, y), nodes=(code, side, nx, ny)) == (len(coords), len(code))
        self.cpu.activate(coords[np.asarray(act) != 0])
        keys = make_keys(coords, leaf)
        order = np.argsort(keys)
        self._flags = (keys[order], np.asarray(act, np.uint8)[order])
        self.peak = max(self.peak, len(coords))

    # -- poses
    def pose(self, i):
        return moved_pose(i, self.offset)

    # -- depth
    def frame(self, i, number):
        d, _ = stream(i)
        nb = self.counts()[0]
        ran_i = self.cpu.integrate(d, self.pose(i), K, self.mu, number)
        assert ran_i
        self._flags = None
        self.created += self.counts()[0] - nb
        self._note(nb)
        self.last = (i, number)
        return self.raycast()

    def staged_frame(self, i, number, between):
        """scan_keys, allocate_keys, `between` (a callable: the operation), sweep with the pose as it is afterwards, raycast."""
        d, _ = stream(i)
        nb = self.counts()[0]
        st = self.state() if self._flags is not None else None
        keys = self.cpu.scan_keys(d, self.pose(i), K, self.mu, number)
        self.cpu.allocate_keys(keys)
        if st is not None:                                   # a seeded oracle: the scan's blocks are active, the others keep the expected flags
            self._carry_flags(st)
        self.created += self.counts()[0] - nb
        self._note(nb)
        out = between()
        self.cpu.sweep(d, self.pose(i), K, self.mu, number)
        self._flags = None
        self.last = (i, number)
        return out, self.raycast()

    def raycast(self, at_once=False):
        """The oracle's (ran, vertex, normal) from the pose of the last frame, with its frame number (at_once: at least 3, so that the
        raycast of an operation's result runs whatever the gate frame > 2 said to the frame before)."""
        i, number = self.last
        if at_once:
            number = max(number, 3)
        ran, v, n = self.cpu.raycast(self.pose(i), K, self.mu, number)
        v.flags.writeable = n.flags.writeable = False
        return ran, v, n

    # -- operations
    def edit(self, records, test, mode):
        c, x, y, a, code, side, nx, ny = self.state()
        ex, ey, enx, eny, counts, _ = edit_util.truth(self.field, c, x, y, code, side, nx, ny, records, test, mode)
        assert self.cpu.set_values(blocks=(c, ex, ey), nodes=(code, side, enx, eny)) == (len(c), len(code))
        return counts

    def _carry_flags(self, st):
        """After blocks were added to a seeded oracle whose state was st: the new ones are active, the others keep the expected flags."""
        keys = make_keys(self.cpu.blocks()[0], leaf_level(self.n))
        flags = np.ones(len(keys), np.uint8)
        flags[np.searchsorted(keys, make_keys(st[0], leaf_level(self.n)))] = st[3]
        self._flags = (keys, flags)

    def allocate(self, rows):
        rec = box_records(rows)
        requested, _, pairs, invalid = closure_truth(self.n, rec)
        nb, nn = self.counts()
        st = self.state()
        self.cpu.insert_octants(np.asarray(sorted(requested), np.uint64))
        nb1, nn1 = self.counts()
        if self._flags is not None:                          # the blocks just created are active; the others keep the expected flags
            self._carry_flags(st)
        self.created += nb1 - nb
        self._note(nb)
        return rec, np.array([nb1 - nb, nn1 - nn, pairs, invalid], np.int64)

    def shift(self, s):
        st = self.state()
        blocks, nodes, counts = shift_truth(self.n, s, st[:4], st[4:], INIT[self.field])
        if np.any(np.asarray(s) != 0):
            self.seed(blocks, nodes)
            self.offset = self.offset + np.asarray(s, np.int64)
        return counts

    def merge(self, src_n, src_state, s, mode, max_weight=100):
        st = self.state()
        blocks, nodes, counts = merge_truth(self.n, st[:4], st[4:], src_n, src_state[:4], src_state[4:], s, MODES[mode], self.field, max_weight)
        seen = both_observed(self.n, st[:4], src_n, src_state[:4], s, self.field)
        self.seed(blocks, nodes)
        self.created += int(counts[1])
        return counts, seen

    def save_load(self):
        st = self.state()
        self.seed((st[0], st[1], st[2], np.ones(len(st[0]), np.uint8)), st[4:])

    def release(self, rows):
        """Returns (records, counts [5] + region [6], info, coords of the released blocks)."""
        rec = release_util.records([(lo, side, release_util.ALL if what == "all" else release_util.UNSEEN) for lo, side, what in rows])
        st = self.state()
        blocks, nodes, counts, touched, info = release_util.release_truth(self.n, rec, st[:4], st[4:], INIT[self.field])
        gone = st[0][~np.isin(make_keys(st[0], leaf_level(self.n)), make_keys(blocks[0], leaf_level(self.n)))]
        if counts[1] or counts[3]:
            self.seed(blocks, nodes)
        return rec, np.concatenate([counts, touched]), info, gone

    def merge_rigid(self, src_n, src_state, pull, mode, max_weight=100):
        st = self.state()
        blocks, nodes, counts = merge_rigid_truth(self.n, st[:4], st[4:], src_n, src_state[:4], pull, MODES[mode], self.field, max_weight)
        self.seed(blocks, nodes)
        self.created += int(counts[1])
        return counts


@functools.lru_cache(maxsize=None)
def source_state(field, name):
    """The state of the merge source `name` after SRC_FRAMES, read-only."""
    n, dim, origin = SOURCES[name]
    m = Model(field, n, dim, origin)
    for j, i in enumerate(SRC_FRAMES):
        m.frame(i, base_frame(field) + j)
    st = m.state()
    assert m.stats_truncated() == 0 and len(st[0]) > 50, (name, len(st[0]))
    m.close()
    return st


def allocate_truth(n, state, rows, init):
    """se_hip_allocate_boxes on a state, from closure_truth: the requested octants and their ancestors exist afterwards, new blocks hold
    initValue() and are active, what existed is untouched.  Returns (state, counts)."""
    coords, x, y, act, code, side, nx, ny = state
    requested, closure, pairs, invalid = closure_truth(n, box_records(rows))
    leaf = leaf_level(n)
    bk = make_keys(coords, leaf)
    want = np.array(sorted(requested | closure), np.uint64)
    is_b = (want & np.uint64(0x1FF)) == np.uint64(leaf)
    new_b, new_n = np.setdiff1d(want[is_b], bk), np.setdiff1d(want[~is_b], code)
    ob, on = np.concatenate([bk, new_b]), np.concatenate([code, new_n])
    ib, i_n = np.argsort(ob), np.argsort(on)
    fill = lambda a, k, v: np.concatenate([a, np.full((k,) + a.shape[1:], v, a.dtype)])
    blocks = (unpack(ob[ib] & ~np.uint64(0x1FF)).astype(np.int32), fill(x, len(new_b), init[0])[ib], fill(y, len(new_b), init[1])[ib],
              fill(act, len(new_b), 1)[ib])
    nodes = (on[i_n], (n >> (on[i_n] & np.uint64(0x1FF)).astype(np.int64)).astype(np.uint32), fill(nx, len(new_n), init[0])[i_n],
             fill(ny, len(new_n), init[1])[i_n])
    return blocks + nodes, np.array([len(new_b), len(new_n), pairs, invalid], np.int64)


# ------------------------------------------------------------------ the programs
_F = ("frame",)
_BOX = ((40, 48, 24), (88, 80, 56))          # in front of the camera, between it and the far wall
_SIDE = ((0, 0, 0), (24, 128, 128))        # the side a shift by +16 along x vacates, and the column of blocks beside it, which holds the wall
_SLAB = ((0, 0, 0), (128, 32, 128))         # the quarter of the volume that a shift by -32 along y drops: 1024 blocks
PROGRAMS = {
    "rolling_submap": ("a rolling map that also receives a submap; the last shift carries a node value",
                       [_F, _F, _F, _F, ("shift", (-32, 0, 16)), _F, _F, ("merge", "src128", (-32, 0, 16), "fuse"), _F, ("edit", "nodes"),
                        ("shift", "node64"), _F, _F]),
    "declare_free": ("a start volume declared free, fused over, partly forgotten, replaced by a submap, rolled, declared free again",
                     [("allocate", [_BOX + (0,)]), ("edit", "free", _BOX), _F, _F, _F, _F, ("edit", "reset"), ("merge", "src64", (32, 32, 56), "replace"),
                      _F, ("shift", (16, 0, 8)), ("allocate", [_SIDE + (0,)]), ("edit", "free", _SIDE), _F, _F]),
    "merge_first": ("a submap into a fresh map, rolled, filled from the same submap elsewhere, saved and loaded",
                    [("merge", "src128", (0, 0, 0), "replace"), _F, ("shift", (-16, 8, 0)), ("merge", "src128", (8, 0, -16), "fill"), _F, _F, _F,
                     ("save_load",), _F, _F]),
    "pool_churn": ("quarter-volume shifts, merges and kilobrick allocations that hand bricks and node slots back and forth through a 2048-brick pool",
                   [_F, _F, ("allocate", [_SLAB + (0,)]), _F, ("shift", (0, -32, 0)), ("merge", "src128", ("registered", (0, 0, -8)), "fuse"),
                    ("allocate", [_SLAB + (0,)]), _F, ("shift", (0, -32, 0)), ("merge", "src64", ("registered", (8, 0, -8)), "fill"),
                    ("allocate", [_SLAB + (0,)]), _F, _F]),
    "staged_edit_allocate": ("an edit and an allocation between the allocation scan and the sweep of a frame",
                             [_F, _F, _F, _F, ("staged", ("edit", "boxes")), _F, ("staged", ("allocate", [_BOX + (0,), ((0, 0, 64), (64, 64, 128), 2)])), _F, _F]),
    "staged_shift_merge": ("a shift and a merge between the allocation scan and the sweep of a frame",
                           [_F, _F, _F, _F, ("staged", ("shift", (-16, 0, 8))), _F, ("staged", ("merge", "src128", (-16, 0, 8), "fuse")), _F, _F]),
}
_WHOLE_UNSEEN = ((0, 0, 0), (N, N, N), "unseen")
_FORGET = ((40, 40, 88), (48, 48, 40), "all")          # the far wall behind the sphere and the space in front of it
_CENTRE = ((56, 56, 64), (24, 24, 24), "all")           # part of the sphere, where the shift of forget_and_roll has moved it
_BACK = ((0, 0, 96), (N, N, 32))                       # (lo, side): the quarter of the volume the far wall stands in
_SLAB_SIDE = (_SLAB[0], tuple(h - l for l, h in zip(*_SLAB)))
PROGRAMS.update({
    "forget_and_roll": ("releases between frames, before and after a shift and a merge; a slab forgotten and allocated again",
                        [_F, _F, _F, _F, ("release", [_WHOLE_UNSEEN, _FORGET]), _F, ("shift", (0, 8, 8)), ("release", [_WHOLE_UNSEEN, _CENTRE]),
                         ("merge", "src128", ("registered", (0, 0, -8)), "fuse"), _F, ("release", [_BACK + ("all",)]),
                         ("allocate", [(_BACK[0], (N, N, N), 0)]), _F, _F]),
    "rigid_submap": ("rigid merges of submaps into a map that fuses on, is shifted and released: fuse, replace after the shift, fill",
                     [_F, _F, _F, _F, ("merge_rigid", "src128", "yaw", "fuse"), _F, ("shift", (0, 8, 8)), ("merge_rigid", "src64", "general", "replace"),
                      ("release", [_WHOLE_UNSEEN]), _F, ("merge_rigid", "src128", "general", "fill"), _F, _F]),
    "pool_churn_release": ("releases that hand bricks and node slots back to a 2048-brick pool; frames, kilobrick allocations and rigid merges draw them again",
                           [_F, _F, ("allocate", [_SLAB + (0,)]), _F, ("release", [_SLAB_SIDE + ("all",)]), ("merge_rigid", "src128", "yaw", "fuse"),
                            ("allocate", [_SLAB + (0,)]), _F, ("release", [_WHOLE_UNSEEN]), ("merge_rigid", "src64", "general", "fill"),
                            ("allocate", [_SLAB + (0,)]), ("release", [_BACK + ("all",), _WHOLE_UNSEEN]), _F, _F]),
    "staged_release_rigid": ("a release and a rigid merge between the allocation scan and the sweep of a frame",
                             [_F, ("staged", ("release", [_WHOLE_UNSEEN])), _F, _F, _F, ("staged", ("merge_rigid", "src128", "yaw", "fuse")), _F, _F]),
})
OLD_KINDS = ("shift", "merge", "allocate", "edit", "save_load", "staged")
STEP_KINDS = ("frame", "shift", "merge", "allocate", "edit", "save_load", "staged", "release", "merge_rigid")
_RANDOM_SHIFTS = [(-16, 0, 8), (-32, 0, 16), (0, 8, 8), (-8, -8, 16)]          # each pushes the far wall out: every one drops blocks
_RANDOM_MERGES = [("src128", ("registered", (0, 0, -8))), ("src64", ("registered", (8, 0, -8)))]
_RANDOM_ROWS = [[_BOX + (0,)], [((24, 40, 40), (72, 90, 100), 0), ((64, 64, 64), (128, 128, 128), 2)], [((50, 30, 60), (110, 100, 120), 0)]]


_RANDOM_RELEASES = [[_WHOLE_UNSEEN, _FORGET], [((0, 0, 64), (N, N, 64), "all")], [_WHOLE_UNSEEN, ((32, 32, 32), (64, 64, 96), "all")]]
_RANDOM_RIGID = [("src128", "yaw"), ("src64", "general"), ("src128", "general")]


def random_program(seed, kinds=OLD_KINDS):
    """Three frames, then four operations drawn from `kinds` with one or two frames after each; ends with two frames; at most 14 steps.
    (With the default kinds the draws are those of the programs random_a and random_b, which must not change.)"""
    rng = np.random.default_rng(seed)
    steps = [_F, _F, _F]
    new = len(kinds) > len(OLD_KINDS)

    def release():
        return ("release", _RANDOM_RELEASES[int(rng.integers(len(_RANDOM_RELEASES)))])

    def rigid():
        src, tr = _RANDOM_RIGID[int(rng.integers(len(_RANDOM_RIGID)))]
        return ("merge_rigid", src, tr, ("fuse", "replace", "fill")[int(rng.integers(3))])

    for kind in np.array(kinds)[rng.permutation(len(kinds))[:4]].tolist():
        if kind == "release":
            steps += [release(), _F]
            continue
        if kind == "merge_rigid":
            steps += [rigid(), _F]
            continue
        if kind == "staged" and new and rng.integers(2):
            steps.append(("staged", release() if rng.integers(2) else rigid()))
            continue
        if kind == "shift":
            op = ("shift", _RANDOM_SHIFTS[int(rng.integers(len(_RANDOM_SHIFTS)))])
        elif kind == "merge":
            src, s = _RANDOM_MERGES[int(rng.integers(len(_RANDOM_MERGES)))]
            op = ("merge", src, s, ("fuse", "replace", "fill")[int(rng.integers(3))])
        elif kind == "allocate":
            op = ("allocate", _RANDOM_ROWS[int(rng.integers(len(_RANDOM_ROWS)))])
        elif kind == "edit":
            op = ("edit", ("boxes", "reset", "nodes")[int(rng.integers(3))])
        elif kind == "save_load":
            op = ("save_load",)
        else:
            op = ("staged", ("edit", "boxes") if rng.integers(2) else ("allocate", _RANDOM_ROWS[int(rng.integers(len(_RANDOM_ROWS)))]))
        steps.append(op)
        if kind != "staged":
            steps.append(_F)
    return steps + [_F, _F]


RANDOM_SEEDS = {"random_a": 5, "random_b": 23}
for _name, _seed in RANDOM_SEEDS.items():
    PROGRAMS[_name] = (f"seeded random program, seed {_seed}", random_program(_seed))
RANDOM_SEEDS_ALL = {"random_c": 3, "random_d": 30}         # drawn from all eight kinds
for _name, _seed in RANDOM_SEEDS_ALL.items():
    PROGRAMS[_name] = (f"seeded random program over every step kind, seed {_seed}", random_program(_seed, OLD_KINDS + ("release", "merge_rigid")))
# reduced programs kept as regression cases next to the full ones: name -> (purpose, steps)
REGRESSIONS = {}
PROGRAMS.update(REGRESSIONS)


def kinds_of(steps):
    out = set()
    for st in steps:
        out.add(st[0])
        if st[0] == "staged":
            out.add(st[1][0])
    return out


# ------------------------------------------------------------------ the model's run of a program
def _free_record(field, box):
    r = np.zeros(1, EDIT_DTYPE)
    r["lo"], r["hi"] = box
    r["x"], r["y"] = FREE[field]
    r["flags"], r["only"] = EDIT_BLOCKS | EDIT_NODES | EDIT_SET_X | EDIT_SET_Y, 7
    return r


def edit_list(kind, field, n, dim, state, v, nrm, next_frame, rng):
    """The edit lists of time_axis_util.make_edit_list for maps of any size (that one wants 60 visible blocks): "reset" of the aligned octant
    round a visible surface point, "boxes" with the values the sensor never writes on up to 12 visible blocks, "nodes": six node values
    written directly, round visible blocks.  Strict mode."""
    coords = state[0]
    hit = nrm[..., 0] != -2
    assert hit.sum() >= 50, (kind, int(hit.sum()))
    hv = np.floor(v * np.float32(n / dim)).astype(np.int64)
    pack = lambda c: (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    seen = np.unique(pack((hv[hit] // 8) * 8))
    visible = coords[np.isin(pack(coords.astype(np.int64)), seen)].astype(np.int64)
    assert len(visible) >= 4, len(visible)
    allf = EDIT_BLOCKS | EDIT_NODES | EDIT_SET_X | EDIT_SET_Y
    now = T.timestamp(next_frame)
    rows = []
    if kind == "reset":
        centre = hv[hit][len(hv[hit]) // 2]
        lo = (centre // (n // 2)) * (n // 2)
        rows.append(T._record(lo, lo + n // 2, INIT[field][0], INIT[field][1], allf))
    elif kind == "boxes":
        xs, ys = (T.SDF_X, T.SDF_Y) if field == SDF else (T.OF_X, np.float32([0, now, now + np.float32(4), now + np.float32(1000), -50, 1e9, 3e38]))
        pick = visible[rng.permutation(len(visible))[:12]]
        for j, c in enumerate(pick):
            lo, hi = (c, c + 8) if j & 1 else (c + [1, 0, 2], c + [8, 7, 6])
            rows.append(T._record(lo, hi, xs[j % len(xs)], ys[(j * 3) % len(ys)], EDIT_BLOCKS | EDIT_SET_X | EDIT_SET_Y))
    elif kind == "nodes":
        values = ([(7, 255), (-3, 101), (0.99999994, 200), (-0.0, 100), (1e-40, 0), (0.5, 99)] if field == SDF else
                  [(1000, now), (-1000, now + np.float32(4)), (999.99, -50), (-999.99, 1e9), (5e-39, 0), (-0.0, now + np.float32(1000))])
        for j, (x, y) in enumerate(values):
            s = 16 << (j % 3)
            lo = (visible[rng.integers(len(visible))] // s) * s
            rows.append(T._record(lo, lo + s, x, y, EDIT_NODES | EDIT_SET_X | EDIT_SET_Y))
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(np.stack(rows))


def _node64(n, field, st):
    ix, iy = INIT[field]
    for s in [(64, 0, 0), (-64, 0, 0), (0, 64, 0), (0, -64, 0), (0, 0, 64), (0, 0, -64)]:
        keep_b, _, keep_n, _, _ = survivors(n, s, st[0], st[4])
        if keep_b.any() and not keep_b.all() and ((st[6][keep_n] != ix) | (st[7][keep_n] != iy)).any():
            return s
    raise AssertionError("no 64-aligned shift keeps and drops blocks and keeps a node with a value")


def _changed_inside(before, after, region, init):
    """Voxels whose bits differ between two states (a block that did not exist counts as initValue()) and that lie inside the half-open box."""
    px, py = T._prior(before, after, init)
    ch = (bits(px) != bits(after[1])) | (bits(py) != bits(after[2]))
    pos = after[0].astype(np.int64)[:, None, :] + edit_util.OFF[None]
    lo, hi = np.asarray(region[0]), np.asarray(region[1])
    return int((ch & ((pos >= lo) & (pos < hi)).all(2)).sum())


def _apply(m, step, number):
    """One non-frame step on the model.  Returns the record of what the device must be given and must answer."""
    kind = step[0]
    rec = {"kind": kind, "step": step}
    whole = ((0, 0, 0), (m.n,) * 3)
    if kind == "shift":
        st = m.state()
        s = _node64(m.n, m.field, st) if step[1] == "node64" else step[1]
        rec["flags_before"] = (int(st[3].min()), int(st[3].max())) if len(st[3]) else (1, 1)
        rec.update(s=tuple(s), counts=m.shift(s), region=whole)
        if step[1] == "node64":
            rec["node64"] = True
    elif kind == "merge":
        _, src, s, mode = step
        if s[0] == "registered":
            s = tuple(int(v) for v in m.offset + np.asarray(SOURCES[src][2], np.int64) + np.asarray(s[1], np.int64))
        counts, seen = m.merge(SOURCES[src][0], source_state(m.field, src), s, mode)
        rec.update(src=src, s=tuple(s), mode=mode, counts=counts, both_observed=seen, region=(tuple(counts[6:9]), tuple(counts[9:12])))
    elif kind == "allocate":
        records, counts = m.allocate(step[1])
        rec.update(records=records, counts=counts, region=(np.min([r[0] for r in step[1]], 0), np.max([r[1] for r in step[1]], 0)))
    elif kind == "edit":
        test = (0.0, m.field == OFUSION)
        if step[1] == "free":
            records, mode = _free_record(m.field, step[2]), "strict"
        else:
            ran, v, nrm = m.raycast(at_once=True)
            records, mode = edit_list(step[1], m.field, m.n, m.dim, m.state(), v, nrm, number, np.random.default_rng(1000 + number)), "strict"
        counts = m.edit(records, test, mode)
        rec.update(records=records, test=test, mode=mode, counts=counts, region=(records["lo"].min(0), records["hi"].max(0)))
    elif kind == "save_load":
        m.save_load()
        rec.update(region=whole)
    elif kind == "release":
        records, counts, info, gone = m.release(step[1])
        rec.update(rows=step[1], records=records, counts=counts, info=info, released=gone, region=(tuple(counts[5:8]), tuple(counts[8:11])))
    elif kind == "merge_rigid":
        _, src, transform, mode = step
        pull = rigid_pull(transform, src, m.offset)
        counts = m.merge_rigid(SOURCES[src][0], source_state(m.field, src), pull, mode)
        rec.update(src=src, transform=transform, pull=pull, mode=mode, counts=counts, region=(tuple(counts[4:7]), tuple(counts[7:10])))
    else:
        raise ValueError(kind)
    return rec


@functools.lru_cache(maxsize=2)
def model_run(name, field, queries=True):
    """The model over PROGRAMS[name]: per step a record -- kind, what the device is given (records, shift, source), the expected counts, the
    state afterwards, the raycast (ran, v, n) taken at once, the truths of the reader battery after an operation that is not a frame and
    not staged (queries; "queries" is the battery's box-query part), and the figures of the engagement conditions.  Computed once per (program, field), shared by the cases and left unchanged.
    Returns (records, summary)."""
    steps = PROGRAMS[name][1]
    assert len(steps) <= 14, (name, len(steps))
    m = Model(field)
    base, i = base_frame(field), 0
    recs, prev, pending = [], m.state(), []
    try:
        for step in steps:
            if step[0] == "frame":
                ran, v, n = m.frame(i, base + i)
                rec = {"kind": "frame", "step": step, "i": i, "number": base + i, "pose": m.pose(i)}
            elif step[0] == "staged":
                inner = {}
                before_pose = m.pose(i)
                _, (ran, v, n) = m.staged_frame(i, base + i, lambda: inner.update(_apply(m, step[1], base + i)))
                rec = {"kind": "staged", "step": step, "i": i, "number": base + i, "scan_pose": before_pose, "pose": m.pose(i), "inner": inner}
            else:
                rec = _apply(m, step, base + i)
                ran, v, n = m.raycast(at_once=True)
                rec["pose"], rec["number"] = m.pose(m.last[0]), max(m.last[1], 3)
            rec["state"], rec["counts_after"] = m.state(), m.counts()
            rec["image"] = (ran, v, n)
            rec["hits"] = int((n[..., 0] != -2).sum()) if ran else 0
            rec["fused_before"] = i > 0
            if step[0] in ("frame", "staged"):
                i += 1
                rec["changed_inside"] = [(p["kind"], _changed_inside(prev, rec["state"], p["region"], INIT[field])) for p in pending]
                pending = []
            if step[0] != "frame":
                if (step[1][0] if step[0] == "staged" else step[0]) == "shift":
                    pending = []                             # (regions of the frame of reference before the shift)
                pending.append(rec["inner"] if step[0] == "staged" else rec)
                if step[0] == "staged" and step[1][0] == "release":          # of the released blocks, those the scan had just created
                    had = make_keys(prev[0], leaf_level(N))
                    rec["inner"]["fresh_released"] = int((~np.isin(make_keys(rec["inner"]["released"], leaf_level(N)), had)).sum())
                if queries and step[0] != "staged":
                    rec["readers"] = reader_truth(field, rec["state"], m.cpu, m.offset, rec["region"], rec["image"], rec["pose"],
                                                  m.pose(m.last[0] + FAR_AHEAD))
                    rec["queries"] = rec["readers"]["boxes"]
            prev = rec["state"]
            recs.append(rec)
        mesh = m.cpu.mesh()
        summary = {"truncated": m.stats_truncated(), "created": m.created, "peak": m.peak, "mesh": mesh}
    finally:
        m.close()
    return recs, summary


def figures(recs, summary):
    """The model-side figures of a run, as one printable dict."""
    ops = lambda r: r["inner"] if r["kind"] == "staged" else r
    return {
        "shifts": [(ops(r)["s"], int(ops(r)["counts"][0]), int(ops(r)["counts"][1])) for r in recs if ops(r)["kind"] == "shift"],
        "merges": [(ops(r)["src"], ops(r)["mode"], int(ops(r)["counts"][1]), ops(r)["both_observed"]) for r in recs if ops(r)["kind"] == "merge"],
        # per release: blocks released, of them observed, nodes released, parent entries reset, of them valued
        "releases": [tuple(int(v) for v in (ops(r)["counts"][1], ops(r)["counts"][4], ops(r)["counts"][3], ops(r)["info"]["reset"], ops(r)["info"]["reset_valued"]))
                     for r in recs if ops(r)["kind"] == "release"],
        # per rigid merge: source, transform, mode, blocks combined, blocks created, voxels observed, voxels both observed
        "rigid": [(ops(r)["src"], ops(r)["transform"], ops(r)["mode"]) + tuple(int(v) for v in ops(r)["counts"][:4]) for r in recs if ops(r)["kind"] == "merge_rigid"],
        "hits": [r["hits"] for r in recs if r["image"][0]],
        "peak": summary["peak"], "created": summary["created"], "truncated": summary["truncated"],
    }


# ------------------------------------------------------------------ the same steps on a device handle
def device_op(gpu, rec, sources, tmp_path=None):
    """The operation of a model record on the handle.  Returns what the call returned, in the form of the record's counts (None: nothing)."""
    from tests.merge_util import counts_of
    kind = rec["kind"]
    if kind == "shift":
        return gpu.shift(rec["s"])
    if kind == "merge":
        return counts_of(gpu.merge(sources[rec["src"]], rec["s"], mode=rec["mode"]))
    if kind == "allocate":
        return gpu.allocate_records(rec["records"])[0]
    if kind == "edit":
        return gpu.edit_records(rec["records"], test=rec["test"], mode=rec["mode"])
    if kind == "save_load":
        path = str(tmp_path / "program_map.bin")
        gpu.save(path)
        gpu.load(path)
        return None
    if kind == "release":
        res = gpu.release(rec["rows"])
        return np.array([res[k] for k in gpu.RELEASE_COUNTS] + list(res["region"][0]) + list(res["region"][1]), np.int64)
    if kind == "merge_rigid":
        from tests.merge_rigid_util import counts_of as rigid_counts_of
        return rigid_counts_of(gpu.merge_rigid(sources[rec["src"]], pull=rec["pull"], mode=rec["mode"]))
    raise ValueError(kind)


def device_source(field, name, pooled):
    """A handle that fused SRC_FRAMES as source_state(field, name) did."""
    from supereight_amd.pipeline import DenseSLAMPipeline
    n, dim, origin = SOURCES[name]
    p = DenseSLAMPipeline((W, H), n, dim, field_type=field, max_blocks=min(POOL, (n // 8) ** 3) if pooled else 0)
    for j, i in enumerate(SRC_FRAMES):
        p.set_depth(stream(i)[0])
        p.setPose(moved_pose(i, -np.asarray(origin, np.int64)))
        assert p.integration(K, 1, MU[field], base_frame(field) + j)
        p.raycasting(K, MU[field], base_frame(field) + j)
    return p


def run_on_device(name, field, max_blocks, streaming, check, tmp_path, ring=None, before=None, queries=True):
    """PROGRAMS[name] on a DenseSLAMPipeline, step for step beside model_run(name, field); check(step index, model record, gpu, returned)
    runs after every step (returned = what the operation's call gave back, None for a frame).  Streaming: the raycasts are deferred into
    `ring` (a callable that gives the handle its image ring); before(step index, model record, gpu) runs in front of every operation that
    is not a frame -- in a staged step between the scan and the operation; queries: as model_run takes it.  Returns the handle (the caller closes it) and the source handles."""
    from supereight_amd.pipeline import DenseSLAMPipeline
    recs, _ = model_run(name, field, queries)
    mu = MU[field]
    gpu = DenseSLAMPipeline((W, H), N, DIM, field_type=field, max_blocks=max_blocks, streaming=streaming)
    sources = {}
    try:
        if ring is not None:
            ring(gpu)
        for src in {(r["inner"] if r["kind"] == "staged" else r).get("src") for r in recs} - {None}:
            sources[src] = device_source(field, src, bool(max_blocks))
        cast = gpu.raycasting_deferred if streaming else gpu.raycasting
        for j, rec in enumerate(recs):
            got = None
            if rec["kind"] == "frame":
                gpu.set_depth(stream(rec["i"])[0])
                gpu.setPose(rec["pose"])
                assert gpu.integration(K, 1, mu, rec["number"])
                assert cast(K, mu, rec["number"]) == rec["image"][0]
            elif rec["kind"] == "staged":
                gpu.set_depth(stream(rec["i"])[0])
                gpu.setPose(rec["scan_pose"])
                assert gpu.alloc_scan(K, 1, mu, rec["number"])
                if before is not None:
                    before(j, rec, gpu)
                got = device_op(gpu, rec["inner"], sources, tmp_path)
                gpu.setPose(rec["pose"])
                assert gpu.integrate_sweep(K, 1, mu, rec["number"])
                assert cast(K, mu, rec["number"]) == rec["image"][0]
            else:
                if before is not None:
                    before(j, rec, gpu)
                got = device_op(gpu, rec, sources, tmp_path)
            check(j, rec, gpu, got)
    except BaseException:
        gpu.close()
        for p in sources.values():
            p.close()
        raise
    return gpu, sources
