"""Float depth that no uint16 millimetre image holds, for tests/test_depth_domain_oracle.py (the oracle alone, and the stand-alone sanitized
replay tests/cpp/depth_domain_replay.cpp) and tests/test_gpu_depth_domain.py (the device against the oracle).

Every other depth image of the suite is a millimetre image divided by 1000: finite, non-negative, on a 1 mm grid.  The C ABI takes any float.
``CLASSES`` lists, as float32 bit patterns, what real callers send beside that: NaN for "no return", +inf and large numbers for sky, negative
and denormal values out of a filter, the render planes to the ulp, and (``offgrid``) the room rendered without the millimetre floor.
``domain_frames`` gives the room stream's frames with one class -- or all of them (``mixed``), or none (``holes``: zeros, the baseline) -- put into
a seeded 10 % of the pixels and into one 16x16 patch aligned to the scan's 8x8 tiles, from frame ``FIRST`` on, so that later frames fuse on top
of what the earlier ones did.  ``RELATION`` states per class, field and shape how the oracle's result differs from the ``holes`` run;
``STAGE_EXCLUDES`` lists the classes on which the reference is not defined at a stage.  supereight_amd/synthetic.py is untouched: the golden
fixtures pin it."""
from __future__ import annotations

import functools
import struct

import numpy as np

from supereight_amd import synthetic as S
from tests.attitude_frames import DIM, FIELDS, SHAPES          # 80x60 -> 128^3 and 160x120 -> 256^3, dim 2.4; sdf mu 0.1, ofusion mu 0.02
from tests.edge_frames import render_room_m

FRAMES = 4            # the raycast gate opens at frame 3
FIRST = 2             # the first frame that holds substituted pixels
FRACTION = 0.10
PATCH = 16
SEED = 20250917
CAP_M = 1000.0        # no finite depth beyond this, see check_cap
NEAR_PLANE, FAR_PLANE = np.float32(0.4), np.float32(4.0)      # nearPlane / farPlane of the raycast and of renderDepth


def _bits(*values) -> tuple:
    return tuple(int(np.float32(v).view(np.uint32)) for v in values)


def _ulps(v) -> tuple:
    b = int(np.float32(v).view(np.uint32))
    return (b - 1, b, b + 1)


OFFGRID = -1          # in place of a bit pattern: the pixel's own depth without the millimetre floor
CLASSES = {
    "nan": (0x7FC00000, 0xFFC00000, 0x7FC00001, 0x7FFFFFFF, 0xFFD12345, 0x7FE00000),       # quiet, both signs, several payloads
    "pinf": (0x7F800000,),
    "ninf": (0xFF800000,),
    "negative": _bits(-1e-3, -0.05, -0.7, -1.0, -5.0),
    "negzero": (0x80000000,),
    "tiny": (0x00000001,) + _bits(1e-40) + (0x00800000,) + _bits(1e-30, 1e-6),                # smallest denormal, 1e-40, FLT_MIN, ...
    "far": _bits(65.536, 100.0, 1000.0),
    "offgrid": (OFFGRID,),
    "planes": _ulps(NEAR_PLANE) + _ulps(FAR_PLANE),
}
ALONE = tuple(CLASSES)
CASES = ALONE + ("mixed",)

# Where the reference is not defined on a class: (stage, class) -> the reason, with the report of the sanitized replay
# (tests/test_depth_domain_oracle.py holds the replay to it: these and only these runs end in a report).
STAGE_EXCLUDES = {
    ("track", "pinf"): "vertices at infinity: trackKernel's projection is NaN, passes its range tests and becomes a pixel index "
                       "(se_oracle.cpp trackKernel: signed integer overflow: -2147483648 * W, then a read far outside the image)",
    ("render", "nan"): "renderDepthKernel takes neither branch for NaN and gs2rgb casts it "
                       "(se_oracle.cpp gs2rgb: nan is outside the range of representable values of type 'int')",
}
# (`tiny` under tracking -- vertices that all but coincide with the camera, normals 0 / 0 -- ends clean: at these poses the projection of such a
# vertex leaves the image and is rejected before any cast.  It stays in the tracker's table on the oracle; the GPU tests track TRACKED only.)
STAGES = ("sdf", "ofusion", "pyramid", "filter", "track", "render")


def stage_classes(stage: str) -> tuple:
    return tuple(c for c in ALONE if (stage, c) not in STAGE_EXCLUDES)


TRACKED = ("nan", "negative", "negzero", "offgrid")                                     # what the GPU consumer test puts into a tracked frame
RENDERED = ("planes", "negative", "tiny", "pinf", "ninf", "far", "offgrid")             # ... and into a rendered one
assert set(TRACKED) <= set(stage_classes("track")) and set(RENDERED) <= set(stage_classes("render"))


def check_cap(depth: np.ndarray) -> np.ndarray:
    """No finite depth beyond CAP_M.  The OFusion scan walks the whole ray from behind the surface to the camera, dist / stepsize trips (about
    1 800 at 1000 m into 128^3 here); beyond some 2^24 steps `travelled += stepsize` stops growing and the loop never ends -- the reference's own
    loop, a hang on the device.  No test sends such a value anywhere or looks for the limit."""
    d = np.asarray(depth, np.float32)
    finite = np.isfinite(d)
    assert not (np.abs(d[finite]) > CAP_M).any(), "a finite depth beyond the cap"
    return depth


def mask_of(W: int, H: int, frame: int) -> np.ndarray:
    """The substituted pixels of a frame: a seeded FRACTION of the image plus one PATCH x PATCH square on the 8x8 tile grid (whole waves of
    the scan), which moves by a tile per frame."""
    rng = np.random.default_rng(SEED + frame)
    m = rng.random((H, W)) < FRACTION
    x0 = (W // 2 // 8 + frame % 2) * 8
    y0 = (H // 2 // 8 - 1) * 8
    x0, y0 = min(x0, (W - PATCH) // 8 * 8), max(0, min(y0, (H - PATCH) // 8 * 8))
    m[y0:y0 + PATCH, x0:x0 + PATCH] = True
    return m


def class_values(classes) -> np.ndarray:
    """The bit patterns of the named classes as one int64 list (OFFGRID = -1 stands for the pixel's own unfloored depth)."""
    return np.asarray([b for c in classes for b in CLASSES[c]], np.int64)


def substitute(base: np.ndarray, room_m: np.ndarray, mask: np.ndarray, classes, seed: int) -> np.ndarray:
    """`base` with the masked pixels replaced by values drawn (seeded, uniformly over the patterns) from the classes; "holes" gives zeros.
    "offgrid" ALONE replaces every pixel that is no hole of the stream: the whole image is off the millimetre grid."""
    out = np.array(base, np.float32)
    if classes == ("holes",):
        out[mask] = 0.0
        return out
    if tuple(classes) == ("offgrid",):
        mask = mask | (base != 0)
    vals = class_values(classes)
    pick = vals[np.random.default_rng(seed).integers(0, len(vals), int(mask.sum()))]
    own = room_m[mask]
    new = np.where(pick == OFFGRID, own.view(np.uint32).astype(np.int64), pick).astype(np.uint32).view(np.float32)
    out[mask] = new
    return np.ascontiguousarray(check_cap(out))


def classes_of(case) -> tuple:
    if isinstance(case, (tuple, list)):
        return tuple(case)
    return ALONE if case == "mixed" else (case,)


class DomainStream:
    """The frame source run_both takes (``depth(f)``, ``pose(f)``, ``k``): `base` stream's frames, substituted from frame `first` on."""

    def __init__(self, case, W: int, H: int, dim: float = DIM, frames: int = FRAMES, first: int = FIRST, k=None, base=None):
        self.W, self.H, self.dim, self.case = W, H, float(dim), case
        base = S.SyntheticStream(W, H, dim) if base is None else base
        self.k = np.ascontiguousarray(base.k if k is None else k, np.float32)
        self.depths, self.poses, self.masks = [], [], []
        for f in range(frames):
            d = base.depth(f)
            m = mask_of(W, H, f) if f >= first else np.zeros((H, W), bool)
            if f >= first:
                d = substitute(d, render_room_m(f, W, H, dim, self.k), m, classes_of(case), SEED + 1000 + f)
            self.depths.append(np.ascontiguousarray(check_cap(d), np.float32))
            self.poses.append(base.pose(f))
            self.masks.append(m)

    def __len__(self):
        return len(self.depths)

    def depth(self, f: int) -> np.ndarray:
        return self.depths[f]

    def pose(self, f: int) -> np.ndarray:
        return self.poses[f]


@functools.lru_cache(maxsize=None)
def domain_frames(case, shape: str) -> DomainStream:
    """Built once per process and shared; nobody writes into the images."""
    W, H, _ = SHAPES[shape]
    s = DomainStream(case, W, H)
    for d in s.depths:
        d.setflags(write=False)
    return s


# ------------------------------------------------------------------------------------------------ the oracle's run, and its relation to holes
def oracle_replay(s, field_name: str, N: int, on_frame=None) -> dict:
    """A stream on the oracle: the final blocks and nodes, probes and swept blocks per frame, the last raycast, the out-of-bounds reads
    counted while integrating.  on_frame(f, pipeline, ran, vertex, normal) sees the state after every frame."""
    from oracle.binding import OraclePipeline
    field, mu = FIELDS[field_name]
    o = OraclePipeline(field, N, s.dim, s.W, s.H)
    o.count_stats(True)
    out = dict(probes=[], swept=[], oob_ub_integration=0)
    try:
        before = o.stats()
        for f in range(len(s)):
            assert o.integrate(s.depth(f), s.pose(f), s.k, mu, f)
            st = o.stats()
            out["probes"].append(st["probes"] - before["probes"])
            out["swept"].append(st["swept"])
            out["oob_ub_integration"] += st["oob_ub"] - before["oob_ub"]
            ran, v, n = o.raycast(s.pose(f), s.k, mu, f)
            assert ran == (f > 2)
            before = o.stats()
            if on_frame:
                on_frame(f, o, ran, v, n)
        out.update(blocks=o.blocks(), nodes=o.nodes(), vertex=v, normal=n, truncated=before["truncated"], hits=int((n[..., 0] != -2).sum()))
    finally:
        o.close()
    return out


def oracle_run(case, field_name: str, shape: str) -> dict:
    return _holes_run(field_name, shape) if case == "holes" else oracle_replay(domain_frames(case, shape), field_name, SHAPES[shape][2])


@functools.lru_cache(maxsize=None)
def _holes_run(field_name: str, shape: str) -> dict:
    return oracle_replay(domain_frames("holes", shape), field_name, SHAPES[shape][2])


def relation(run: dict, holes: dict) -> dict:
    """How a run's final map differs from the holes run's: `blocks` that exist in one and not the other, `voxels` of the blocks both hold
    whose (x, y) bits differ, and the difference in `probes` over all frames."""
    (c0, x0, y0, _), (c1, x1, y1, _) = run["blocks"], holes["blocks"]
    i0 = {tuple(c): i for i, c in enumerate(c0.tolist())}
    i1 = {tuple(c): i for i, c in enumerate(c1.tolist())}
    both = sorted(set(i0) & set(i1))
    a, b = np.array([i0[c] for c in both], np.int64), np.array([i1[c] for c in both], np.int64)
    differ = (x0[a].view(np.uint32) != x1[b].view(np.uint32)) | (y0[a].view(np.uint32) != y1[b].view(np.uint32))
    return dict(blocks=len(set(i0) ^ set(i1)), voxels=int(differ.sum()), probes=abs(sum(run["probes"]) - sum(holes["probes"])))


# (blocks, voxels, probes) per class, field and shape: 0 = identical to the holes run, exactly; n > 0 = differs by at least n, half of what the
# oracle gives; None = not pinned (a handful of blocks either way at the edge of the band).  Read by row:
#   nan       a hole for SDF; under OFusion the scan skips it (`travelled < NaN`) and the sweep marks its voxels free (H(NaN) clamps to 0.03)
#   pinf      no scan step (the walk's origin is NaN); sdf = 1 carves free space, OFusion marks free
#   ninf      a hole everywhere: no scan step, `depthSample <= 0` in both sweeps
#   negative  a hole for both sweeps, yet both scans test `== 0` only: bands near the camera allocate blocks that are never written
#   negzero   `-0.0 == 0`: a hole
#   tiny      denormals are not flushed: not holes for the scans (a band around the camera), nothing within reach of the sweeps
#   far       beyond the volume: the SDF band walk is outside it, the OFusion walk crosses it back to the camera; both sweeps carve
#   offgrid   ordinary depths between the millimetres: everything changes a little
#   planes    0.4 m and 4.0 m are depths like any other to the map
_S, _L = SHAPES
RELATION = {
    "nan": {"sdf": {_S: (0, 0, 0), _L: (0, 0, 0)}, "ofusion": {_S: (0, 20506, 0), _L: (0, 93463, 0)}},
    "pinf": {"sdf": {_S: (0, 20847, 0), _L: (0, 102350, 0)}, "ofusion": {_S: (0, 20506, 0), _L: (0, 93463, 0)}},
    "ninf": {"sdf": {_S: (0, 0, 0), _L: (0, 0, 0)}, "ofusion": {_S: (0, 0, 0), _L: (0, 0, 0)}},
    "negative": {"sdf": {_S: (6, 0, 3113), _L: (12, 0, 18282)}, "ofusion": {_S: (1, 0, 1941), _L: (4, 0, 11277)}},
    "negzero": {"sdf": {_S: (0, 0, 0), _L: (0, 0, 0)}, "ofusion": {_S: (0, 0, 0), _L: (0, 0, 0)}},
    "tiny": {"sdf": {_S: (2, 0, 7711), _L: (8, 0, 46926)}, "ofusion": {_S: (2, 0, 538), _L: (4, 0, 2943)}},
    "far": {"sdf": {_S: (0, 20847, 0), _L: (0, 102350, 0)}, "ofusion": {_S: (None, 20506, 2407), _L: (None, 93463, 14775)}},
    "offgrid": {"sdf": {_S: (None, 49621, 7711), _L: (None, 366393, 46926)}, "ofusion": {_S: (None, 57274, 7590), _L: (None, 380116, 42540)}},
    "planes": {"sdf": {_S: (23, 11202, 3998), _L: (118, 54075, 23144)}, "ofusion": {_S: (10, 11044, 4446), _L: (50, 49463, 23716)}},
    "mixed": {"sdf": {_S: (26, 6427, 2761), _L: (121, 30004, 17710)}, "ofusion": {_S: (13, 11071, 1785), _L: (55, 47823, 10229)}},
}


def expected_relation(case: str, field_name: str, shape: str) -> dict:
    return dict(zip(("blocks", "voxels", "probes"), RELATION[case][field_name][shape]))


# ------------------------------------------------------------------------------------------------ the file the stand-alone replay reads
def write_replay_file(path: str, sequences) -> None:
    """sequences: (name, DomainStream-like with depths / poses / k / W / H, N, dim).  Little-endian: a count, then per sequence the name (32
    bytes), W, H, N, frames (int32), dim and k (float32 x 5), then per frame the pose (16 float32, column-major) and the image."""
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(sequences)))
        for name, s, N, dim in sequences:
            f.write(struct.pack("<32s4i5f", name.encode(), s.W, s.H, N, len(s.depths), dim, *[float(v) for v in s.k]))
            for d, T in zip(s.depths, s.poses):
                f.write(S.to_colmajor(T).astype("<f4").tobytes())
                f.write(np.ascontiguousarray(d, "<f4").tobytes())


class ConsumerFrames:
    """Clean frames 0 .. frames - 1 of a stream and frame `frames` with the classes substituted: what the tracker and renderDepth are given."""

    def __init__(self, classes, W, H, dim, k=None, base=None, frames: int = 4):
        s = DomainStream(tuple(classes), W, H, dim, frames=frames + 1, first=frames, k=k, base=base)
        self.W, self.H, self.dim, self.k, self.depths, self.poses, self.masks = W, H, dim, s.k, s.depths, s.poses, s.masks
