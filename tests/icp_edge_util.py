"""Seeded cases for the tracker's scalar core and for tracking at the reduction's edges, shared by tests/test_icp_math_host.py (which holds
every case to its purpose on the oracle alone), tests/test_gpu_icp_math.py and tests/test_gpu_tracking_edges.py (which run them on the device).

  * sincos_arguments()   -- arguments of se_sincos_f32 / so_sincos: all four quadrants, the neighbourhoods of the multiples of pi/4 and of a
                            few large multiples of pi/2, the ends of the number format and of the stated range |x| < 2^20;
  * solve_systems()      -- 6x6 systems (b[6], upper triangle[21]) for se_solve6_wave / solve6: ICP-like normal equations from few and many
                            rows, exact Cholesky failures at every column, nearly singular systems, NaN / inf entries, the zero system;
  * finalize_cases()     -- partial-row blocks [8][SEGMENTS][32], poses and thresholds for se_icp_finalize; most of them carry a chosen twist
                            through an identity system (C = I, b = twist gives x = b exactly), so that they steer the SE(3) exponential;
  * finalize_reference() -- the reference of that entry: the sums in their stated order in numpy float32, the oracle's solve and exponential,
                            the 4x4 product in numpy float32;
  * the scenes and pyramids of the end-to-end cases, built once per process on the oracle.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle.binding import SDF, OraclePipeline, oracle_se3_exp, oracle_solve6, oracle_tracking

SEGMENTS = 32          # SE_TRACK_SEGMENTS / SO_TRACK_SEGMENTS
LANES = 256            # SE_TRACK_LANES
EPS = np.float32(1e-5)  # Sophus' epsilon in se3_exp
INV_PIO2 = 6.36619772367581382433e-01


def bits_around(center, half: int) -> np.ndarray:
    """Every float32 within +-half ulp of float32(center) (center != 0, away from the ends of its sign's range)."""
    b = int(np.float32(center).view(np.int32))
    return (b + np.arange(-half, half + 1, dtype=np.int64)).astype(np.int32).view(np.float32)


def quadrant(x) -> np.ndarray:
    """n = rint(x * 2/pi) & 3 of so_sincos, for float32 arguments."""
    kd = np.rint(np.asarray(x, np.float32).astype(np.float64) * INV_PIO2)
    return (kd.astype(np.int64) & 3).astype(np.int32)


# ------------------------------------------------------------------------------------------------ sine / cosine
@functools.lru_cache(maxsize=None)
def sincos_arguments() -> np.ndarray:
    rng = np.random.default_rng(20240611)
    parts = [rng.uniform(-64.0, 64.0, 2_000_000).astype(np.float32),
             (rng.choice([-1.0, 1.0], 2_000_000) * np.exp2(rng.uniform(-30.0, 20.0, 2_000_000))).astype(np.float32)]
    near = [np.arange(0, 513, dtype=np.int32).view(np.float32)]                     # k = 0: +0 and the 512 smallest subnormals
    near += [bits_around(k * np.pi / 4, 512) for k in range(1, 257)]
    near += [bits_around(k * np.pi / 2, 512) for k in (1000, 12345, 100000, 333333, 600000)]
    near = np.concatenate(near)
    parts += [near, -near]
    tiny, big = np.float32(1e-45), np.float32(2.0 ** 20)
    ends = np.asarray([0.0, tiny, np.float32(1.1754942e-38), np.float32(1.17549435e-38), np.nextafter(big, np.float32(0)), big,
                       np.nextafter(big, np.float32(np.inf))], np.float32)
    parts += [ends, -ends]
    x = np.ascontiguousarray(np.concatenate(parts), np.float32)
    assert x.size <= 8_000_000 and np.isfinite(x).all()
    return x


# ------------------------------------------------------------------------------------------------ 6x6 systems
TRI = [(r, c) for r in range(6) for c in range(r, 6)]        # the order of the upper triangle in the 27 values (after b[6])
DIAG = [6 + TRI.index((r, r)) for r in range(6)]


def icp_rows(rng, shape, scale):
    """ICP-like rows [n, p x n] (unit normals n, points p of magnitude `scale`) and residuals: J[shape + (6,)], e[shape], float32."""
    n = rng.normal(size=shape + (3,))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    p = rng.uniform(-1.0, 1.0, shape + (3,)) * scale
    J = np.concatenate([n, np.cross(p, n)], axis=-1).astype(np.float32)
    e = (rng.normal(size=shape) * 0.01 * scale).astype(np.float32)
    return J, e


def sums_of_rows(J, e) -> np.ndarray:
    """The 32 sums (tracking.cpp:113-170) of accepted rows J[..., m, 6], e[..., m], accumulated in float32."""
    out = np.zeros(J.shape[:-2] + (32,), np.float32)
    out[..., 0] = (e * e).sum(-1, dtype=np.float32)
    for i in range(6):
        out[..., 1 + i] = (e * J[..., i]).sum(-1, dtype=np.float32)
    for k, (i, j) in enumerate(TRI):
        out[..., 7 + k] = (J[..., i] * J[..., j]).sum(-1, dtype=np.float32)
    out[..., 28] = J.shape[-2]
    return out


def pack_system(Cm, b) -> np.ndarray:
    return np.asarray(list(b) + [Cm[r][c] for r, c in TRI], np.float32)


@functools.lru_cache(maxsize=None)
def solve_systems():
    """(vals[n, 27] float32, exact: list of (index, column) of the systems built to fail at exactly that column)."""
    rng = np.random.default_rng(77001)
    vals, exact = [], []
    # normal equations of few and many rows, over twelve decades of scale
    for m in (3, 5, 6, 7, 50, 5000):
        for scale in 10.0 ** np.arange(-6, 7):
            for _ in range(8 if m < 5000 else 2):
                J, e = icp_rows(rng, (m,), scale)
                vals.append(sums_of_rows(J, e)[1:28])
    # exact failures: C = L L^T of small integers is exact in float32, and so is its factorisation up to column j
    for j in range(6):
        for rep in range(24):
            L = np.tril(rng.integers(-3, 4, (6, 6))).astype(np.float64)
            L[np.arange(6), np.arange(6)] = rng.integers(1, 5, 6)
            Cm = L @ L.T
            Cm[j, j] -= L[j, j] ** 2 + (0 if rep % 2 == 0 else int(rng.integers(1, 6)))      # pivot exactly 0 / negative
            exact.append((len(vals), j))
            vals.append(pack_system(Cm, rng.integers(-9, 10, 6)))
        L = np.tril(rng.integers(-3, 4, (6, 6))).astype(np.float64)                           # ... and one that goes through
        L[np.arange(6), np.arange(6)] = rng.integers(1, 5, 6)
        exact.append((len(vals), 6))
        vals.append(pack_system(L @ L.T, rng.integers(-9, 10, 6)))
    # rank-deficient systems (2 to 5 rows, or 50 rows in a plane's null space) plus eps * I
    for eps in 10.0 ** np.arange(-12, -1):
        for m in (2, 3, 4, 5):
            J, e = icp_rows(rng, (m,), 1.0)
            v = sums_of_rows(J, e)[1:28]
            v[DIAG] += np.float32(eps)
            vals.append(v)
        J, e = icp_rows(rng, (50,), 1.0)
        J[:, :3] = np.float32([0, 0, 1]); J[:, 5] = 0                                         # one plane seen head-on: rank 3
        v = sums_of_rows(J, e)[1:28]
        v[DIAG] += np.float32(eps)
        vals.append(v)
    # one entry NaN or +-inf: every position of b, of the diagonal and off the diagonal
    for _ in range(2):
        J, e = icp_rows(rng, (50,), 1.0)
        base = sums_of_rows(J, e)[1:28]
        for pos in range(27):
            for bad in (np.nan, np.inf, -np.inf):
                v = base.copy()
                v[pos] = bad
                vals.append(v)
    vals.append(np.zeros(27, np.float32))
    exact.append((len(vals) - 1, 0))
    return np.ascontiguousarray(np.stack(vals), np.float32), exact


def oracle_solve_all(vals):
    x = np.zeros((len(vals), 6), np.float32)
    col = np.zeros(len(vals), np.int32)
    for i, v in enumerate(vals):
        x[i], col[i] = oracle_solve6(v)
    return x, col


# ------------------------------------------------------------------------------------------------ finalize cases
def theta_of(twist):
    """theta_sq and theta of se3_exp, in its float32 order."""
    w = np.asarray(twist, np.float32)[..., 3:6]
    tsq = (w[..., 0] * w[..., 0] + w[..., 1] * w[..., 1]) + w[..., 2] * w[..., 2]
    return tsq, np.sqrt(tsq)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


@functools.lru_cache(maxsize=None)
def twists() -> np.ndarray:
    """(upsilon, omega)[n, 6] float32."""
    rng = np.random.default_rng(4242)
    out = []
    ups = lambda: rng.uniform(-0.05, 0.05, 3)
    add = lambda u, w: out.append(np.concatenate([u, w]).astype(np.float32))
    zero = np.zeros(3)
    add(zero, zero); add(ups(), zero); add(ups(), zero)
    # |omega| within +-64 ulp of Sophus' epsilon: along an axis (|omega| = the component itself) and along the diagonal
    for axis in range(3):
        for t in bits_around(EPS, 64)[:: 1 if axis == 0 else 16]:
            w = np.zeros(3, np.float32); w[axis] = t
            add(ups() if axis else zero, w)
    for t in bits_around(float(EPS) / np.sqrt(3.0), 64):
        add(ups(), np.float32([t, t, t]))
    # updates as the ICP makes them
    for mag in 10.0 ** rng.uniform(-6, -2, 120):
        add(ups() * mag * 10, _unit(rng.normal(size=3)) * mag)
    # |omega| around every multiple of pi/4 up to 8 pi: sincos(theta) and sincos(theta / 2) go through their quadrants
    for k in range(1, 33):
        for d in (_unit([1, 0, 0]), _unit(rng.normal(size=3))):
            for rel in (0.0, -3e-7, 3e-7, -1e-3, 1e-3):
                add(ups(), d * (k * np.pi / 4) * (1.0 + rel))
    for mag in (10.0, 31.4, 100.0, 333.3, 1000.0):
        add(ups(), _unit(rng.normal(size=3)) * mag)
        add(zero, _unit(rng.normal(size=3)) * mag)
    return np.stack(out)


def _poses(rng, n):
    """Alternately rigid poses (an exponential plus a translation) and poses that have drifted off SE(3) by ~1e-3."""
    P = np.zeros((n, 4, 4), np.float32)
    for i in range(n):
        T = oracle_se3_exp(np.concatenate([rng.uniform(-2, 2, 3), _unit(rng.normal(size=3)) * rng.uniform(0, 3)]))
        if i % 2:
            T[:3, :] += rng.normal(size=(3, 4)).astype(np.float32) * np.float32(1e-3)
        P[i] = T
    return P.reshape(n, 16)


def twist_row(twist) -> np.ndarray:
    """A row of 32 sums whose system is C = I, b = twist: the solve returns the twist itself."""
    row = np.zeros(32, np.float32)
    row[0] = 1e-4; row[1:7] = twist; row[28] = 100
    row[[1 + d for d in DIAG]] = 1
    return row


@functools.lru_cache(maxsize=None)
def finalize_cases():
    """dict(partial[n, 8, SEGMENTS, 32], pose[n, 16], thr[n], n_twists: case i < n_twists carries twists()[i], n_base: the cases from there
    on are triples of one block and pose with three thresholds)."""
    rng = np.random.default_rng(99173)
    tw = twists()
    blocks = []
    for t in tw:                                     # the twist's row in one strip and one segment, zero everywhere else
        blk = np.zeros((8, SEGMENTS, 32), np.float32)
        blk[rng.integers(0, 8), rng.integers(0, SEGMENTS)] = twist_row(t)
        blocks.append(blk)
    n_twists = len(blocks)
    # every partial row non-zero: sums of four ICP-like rows each, so that the order of the 32 x 8 additions shows
    for scale in (1e-3, 1.0, 1.0, 1.0, 30.0, 1e3):
        for _ in range(8):
            J, e = icp_rows(rng, (8, SEGMENTS, 4), scale)
            blocks.append(sums_of_rows(J, e))
    # only some strips / segments non-zero: a level of 3 rows (strips 0..2), of 5 pixels per strip (segments 0..4), one strip, one segment, nothing
    for keep_b, keep_g in ((3, SEGMENTS), (8, 5), (3, 5), (1, SEGMENTS), (8, 1), (1, 1), (0, 0)):
        for _ in range(4):
            J, e = icp_rows(rng, (8, SEGMENTS, 6), 1.0)
            blk = sums_of_rows(J, e)
            blk[keep_b:] = 0; blk[:, keep_g:] = 0
            blocks.append(blk)
    partial = np.stack(blocks)
    pose = _poses(rng, len(partial))
    thr = np.full(len(partial), 1e-5, np.float32)
    # conv on either side of icp_threshold: the threshold is the update's own norm (not below it: 0), one ulp above (1), one ulp below (0)
    pick = np.concatenate([np.arange(0, n_twists, 7), np.arange(n_twists, len(partial))])
    norm = finalize_reference(partial[pick], pose[pick], thr[pick])["norm"]
    n_base = len(partial)
    extra_p, extra_q, extra_t = [], [], []
    for i, nv in zip(pick, norm):
        if not np.isfinite(nv):
            continue
        for t in (nv, np.nextafter(nv, np.float32(np.inf)), np.nextafter(nv, np.float32(-np.inf))):
            extra_p.append(partial[i]); extra_q.append(pose[i]); extra_t.append(t)
    partial = np.ascontiguousarray(np.concatenate([partial, np.stack(extra_p)]), np.float32)
    pose = np.ascontiguousarray(np.concatenate([pose, np.stack(extra_q)]), np.float32)
    thr = np.ascontiguousarray(np.concatenate([thr, np.asarray(extra_t, np.float32)]), np.float32)
    return dict(partial=partial, pose=pose, thr=thr, n_twists=n_twists, n_base=n_base)


def finalize_reference(partial, pose, thr):
    """se_icp_finalize by its stated order: per strip the segments in order, then the strips in order (numpy float32); the oracle's solve and
    exponential; delta * pose with inner sums left to right (numpy float32); |x| < icp_threshold.  Returns strip0[n, 32], pose[n, 16], conv[n],
    and x[n, 6], col[n], norm[n] for the tests that hold the cases to their purpose."""
    partial = np.asarray(partial, np.float32)
    n = len(partial)
    with np.errstate(all="ignore"):
        strip = np.zeros((n, 8, 32), np.float32)
        for g in range(SEGMENTS):
            strip = strip + partial[:, :, g, :]
        row0 = strip[:, 0].copy()
        for b in range(1, 8):
            row0 = row0 + strip[:, b]
        x, col = oracle_solve_all(row0[:, 1:28])
        D = np.stack([oracle_se3_exp(v) for v in x])
        P = np.asarray(pose, np.float32).reshape(n, 4, 4)
        out = ((D[:, :, 0:1] * P[:, 0:1, :] + D[:, :, 1:2] * P[:, 1:2, :]) + D[:, :, 2:3] * P[:, 2:3, :]) + D[:, :, 3:4] * P[:, 3:4, :]
        xn = np.zeros(n, np.float32)
        for q in range(6):
            xn = xn + x[:, q] * x[:, q]
        norm = np.sqrt(xn)
        conv = (norm < np.asarray(thr, np.float32)).astype(np.int32)
    return dict(strip0=row0, pose=out.reshape(n, 16).astype(np.float32), conv=conv, x=x, col=col, norm=norm)


def same_bits(got, want) -> np.ndarray:
    """Elementwise: bit-identical, or both NaN (payload and sign of a NaN are not part of the contract)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))


# ------------------------------------------------------------------------------------------------ end-to-end scenes
class Scene:
    """Frames 0..frames-1 fused and raycast at ground-truth poses on the oracle; frame `frames` is the one to track, from pose(frames - 1)."""

    def __init__(self, name, stream, N, dim, mu=0.1, frames=5):
        self.name, self.N, self.dim, self.mu, self.frames = name, N, dim, mu, frames
        self.W, self.H, self.k = stream.width, stream.height, np.asarray(stream.k, np.float32)
        self.depths = [stream.depth(f) for f in range(frames + 1)]
        self.poses = [stream.pose(f) for f in range(frames + 1)]
        cpu = OraclePipeline(SDF, N, dim, self.W, self.H)
        try:
            for f in range(frames):
                cpu.integrate(self.depths[f], self.poses[f], self.k, mu, f)
                ran, v, n = cpu.raycast(self.poses[f], self.k, mu, f)
                if ran:
                    self.ref_vertex, self.ref_normal, self.raycast_pose = v, n, self.poses[f].copy()
        finally:
            cpu.close()
        self.track_depth, self.start_pose = self.depths[frames], self.poses[frames - 1].copy()
        self._runs = {}

    def track(self, pyramid, depth=None, start=None, key=None):
        """oracle_tracking of the frame (or of `depth` from `start`, cached under `key`) with its trace:
        (tracked, pose, TrackData, sums, iterations, trace records)."""
        key = (tuple(pyramid), key)
        if key not in self._runs:
            tr = []
            r = oracle_tracking(self.track_depth if depth is None else depth, self.k, self.start_pose if start is None else start,
                                self.raycast_pose, self.ref_vertex, self.ref_normal, 1e-5, tuple(pyramid), trace=tr)
            self._runs[key] = r + (tr[0],)
        return self._runs[key]

    def segment_length(self, level=0, strip=0):
        w, h = self.W >> level, self.H >> level
        npx = ((h - strip + 7) // 8) * w
        return (npx + SEGMENTS - 1) // SEGMENTS


DEEP_PYRAMIDS = [(0, 0, 0, 0, 0, 3)] + [(0, 0, 0, 0, k) for k in range(1, 7)] + [(0, 0, 0, 0, 0, 0, 2), (2, 2, 2, 2, 2, 2)]
GROWTH_ORDER = [(4, 3, 2), (2, 2, 2, 2, 2, 2), (4, 3, 2)]          # 3 levels -> 6 levels -> 3 levels on one handle
RAGGED_PYRAMID = (4, 3, 2, 2, 3)                                   # 163x101 -> 81x50 -> 40x25 -> 20x12 -> 10x6
LARGE_SHAPES = [(672, 496), (800, 600), (1024, 648)]
LARGE_SEGMENTS = {(672, 496): 1302, (800, 600): 1875, (1024, 648): 2592}


@functools.lru_cache(maxsize=None)
def deep_scene() -> Scene:
    from supereight_amd.synthetic import SyntheticStream
    return Scene("deep", SyntheticStream(160, 120, 4.8), 128, 4.8)


@functools.lru_cache(maxsize=None)
def ragged_scene() -> Scene:
    from tests.edge_frames import CONSUMER, RoomStream
    c = CONSUMER
    return Scene("ragged", RoomStream(c["W"], c["H"], c["dim"], c["k"]), c["N"], c["dim"])


@functools.lru_cache(maxsize=None)
def gate_scene() -> Scene:
    """The scene of tests/test_gpu_tracking.py::test_tracking_gate_and_rejection: four frames, frame 4 tracked."""
    from supereight_amd.synthetic import SyntheticStream
    return Scene("gate", SyntheticStream(160, 120, 2.4), 128, 2.4, frames=4)


def far_pose(scene: Scene) -> np.ndarray:
    far = scene.start_pose.copy()
    far[:3, 3] += 1.0                 # nothing overlaps from here
    return far


@functools.lru_cache(maxsize=None)
def large_scene(W: int, H: int) -> Scene:
    from supereight_amd.synthetic import SyntheticStream
    return Scene(f"large_{W}x{H}", SyntheticStream(W, H, 4.8), 256, 4.8)
