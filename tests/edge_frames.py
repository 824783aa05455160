"""The room + sphere scene of supereight_amd/synthetic.py through any pinhole camera, and the table of edge configurations that
tests/test_gpu_edge_configs.py runs against the oracle.

``render_room_mm`` is ``synthetic.render_depth_mm`` with the intrinsics as an argument: with ``k = intrinsics(W)`` it gives the same image bit for
bit (tests/test_edge_configs_oracle.py).  ``RoomStream`` adds the hole stream and the millimetre quantisation of ``SyntheticStream`` and keeps its
pose path.  The default stream of synthetic.py is untouched: the golden fixtures pin it."""
from __future__ import annotations

import numpy as np

from oracle.binding import OFUSION, SDF
from supereight_amd import synthetic as S


def _render_room(frame: int, width: int, height: int, dim: float, k) -> np.ndarray:
    """float64 z-depth in metres of the room + sphere scene seen with intrinsics k = (fx, fy, cx, cy) from synthetic.pose(frame)."""
    k = np.asarray(k, np.float32).astype(np.float64)
    T = S.pose(frame, dim).astype(np.float64)
    xs = (np.arange(width) + 0.5 - k[2]) / k[0]
    ys = (np.arange(height) + 0.5 - k[3]) / k[1]
    u, v = np.meshgrid(xs, ys)
    d = np.stack([u, v, np.ones_like(u)], axis=-1) @ T[:3, :3].T     # t == camera z-depth
    o = T[:3, 3]
    lo, hi = S.ROOM_LO * dim, S.ROOM_HI * dim
    with np.errstate(divide="ignore", invalid="ignore"):
        t_axis = np.where(d > 0, (hi - o) / d, np.where(d < 0, (lo - o) / d, np.inf))
    t_room = t_axis.min(axis=-1)
    c = np.array(S.SPHERE_C) * dim
    r = S.SPHERE_R * dim
    oc = o - c
    A = (d * d).sum(-1)
    B = 2.0 * (d * oc).sum(-1)
    C = (oc * oc).sum() - r * r
    disc = B * B - 4 * A * C
    t_s = (-B - np.sqrt(np.maximum(disc, 0.0))) / (2 * A)
    t_s = np.where((disc >= 0) & (t_s > 0), t_s, np.inf)
    return np.minimum(t_room, t_s)


def render_room_mm(frame: int, width: int, height: int, dim: float, k) -> np.ndarray:
    """uint16 millimetre depth image of the room + sphere scene seen with intrinsics k = (fx, fy, cx, cy) from synthetic.pose(frame)."""
    mm = np.floor(_render_room(frame, width, height, dim, k) * 1000.0)
    return np.clip(mm, 0, 65535).astype(np.uint16)


def render_room_m(frame: int, width: int, height: int, dim: float, k) -> np.ndarray:
    """The same image in float32 metres WITHOUT the millimetre floor: depths no uint16 millimetre image holds (tests/depth_domain_frames.py)."""
    return np.ascontiguousarray(_render_room(frame, width, height, dim, k).astype(np.float32))


class RoomStream:
    """SyntheticStream with intrinsics of the caller's choice: ``depth(f)`` in frame order, ``pose(f)``, ``k``, ``depth_mm(f)``."""

    def __init__(self, width: int, height: int, dim: float, k, holes: bool = True):
        self.width, self.height, self.dim = width, height, float(dim)
        self.k = np.asarray(k, np.float32)
        self._holes = S.HoleStream() if holes else None
        self._next = 0

    def depth_mm(self, frame: int) -> np.ndarray:
        """The frame's millimetre image with its holes (0), consuming the hole stream like depth(frame)."""
        if frame != self._next:
            raise ValueError("RoomStream frames must be requested in order")
        self._next += 1
        mm = render_room_mm(frame, self.width, self.height, self.dim, self.k)
        if self._holes is not None:
            u = self._holes.uniform(self.width * self.height).reshape(self.height, self.width)
            mm = np.where(u < S.HOLE_FRACTION, np.uint16(0), mm)
        return np.ascontiguousarray(mm, dtype=np.uint16)

    def depth(self, frame: int) -> np.ndarray:
        return np.ascontiguousarray(self.depth_mm(frame).astype(np.float32) / np.float32(1000.0))   # mm2metersKernel: depth / 1000.0f

    def pose(self, frame: int) -> np.ndarray:
        return S.pose(frame, self.dim)


def edge_stream(case):
    return RoomStream(case["W"], case["H"], case["dim"], case["k"])


def _case(name, W, H, N, k, field, mu, frames, min_blocks, min_hits, dim=4.8, pooled=0):
    return dict(name=name, W=W, H=H, N=N, dim=dim, k=tuple(float(v) for v in k), field=field, mu=mu, frames=frames,
                min_blocks=min_blocks, min_hits=min_hits, pooled=pooled)


# Shapes x cameras.  Each case lists the least number of blocks the oracle allocates in `frames` frames and the least number of raycast hits in
# its last frame (test_edge_configs_oracle.py holds the oracle to them, so that no case turns vacuous), and the max_blocks of its pooled run
# (0: no pooled run).  Tiles are 8x8 pixels.
SHAPE_CASES = [
    # 21 x 13 tiles (odd count): partial last tile column and row; fx != fy, principal point far off centre
    _case("ragged_161x97_aniso_sdf", 161, 97, 256, (200.0, 90.0, 30.0, 80.0), SDF, 0.1, 6, 700, 8000, pooled=1 << 13),
    _case("ragged_161x97_aniso_ofusion", 161, 97, 256, (200.0, 90.0, 30.0, 80.0), OFUSION, 0.02, 6, 500, 8000),
    # narrower than a tile: one partial tile column; a narrow lens
    _case("narrow_5x67_tele_sdf", 5, 67, 256, (600.0, 600.0, 2.5, 33.5), SDF, 0.1, 6, 10, 200, pooled=1 << 12),
    _case("narrow_5x67_tele_ofusion", 5, 67, 256, (600.0, 600.0, 2.5, 33.5), OFUSION, 0.02, 6, 10, 200),
    # shorter than a tile: one partial tile row; negative fy, principal point off centre
    _case("short_75x5_tele_negfy_sdf", 75, 5, 256, (600.0, -150.0, 30.2, 2.9), SDF, 0.1, 6, 10, 100),
    _case("short_75x5_tele_negfy_ofusion", 75, 5, 256, (600.0, -150.0, 30.2, 2.9), OFUSION, 0.02, 6, 10, 100, pooled=1 << 12),
    # a wide lens (~115 deg across) on a ragged shape
    _case("wide_83x61_sdf", 83, 61, 512, (26.0, 26.0, 41.5, 30.5), SDF, 0.1, 6, 300, 1000),
    _case("wide_83x61_ofusion", 83, 61, 512, (26.0, 26.0, 41.5, 30.5), OFUSION, 0.02, 6, 300, 1000, pooled=1 << 14),
    # 81 x 61 tiles (odd count): 2 471 raycast workgroups, just inside one round of the chip (2 560 on 256 compute units); off-centre, fx != fy
    _case("large_641x481_sdf", 641, 481, 256, (470.0, 490.0, 300.7, 250.3), SDF, 0.1, 6, 1500, 150000),
    # 91 x 61 tiles (odd count): more raycast workgroups than one round of the chip; ICL-like camera with negative fy, off-centre
    _case("large_721x481_negfy_sdf", 721, 481, 256, (520.0, -505.0, 371.4, 233.8), SDF, 0.1, 6, 1500, 150000),
    _case("large_721x481_negfy_ofusion", 721, 481, 256, (520.0, -505.0, 371.4, 233.8), OFUSION, 0.02, 6, 1000, 150000, pooled=1 << 14),
]

# Volume resolutions at the ends of the range se_hip_create accepts.  64^3: leaf level 3, below the LDS-staged levels, no fine beam grid, OFusion
# octants at levels 1 and 2.  4096^3: leaf level 9, three occupancy levels beyond the staged ones; pooled bricks only, with a small explicit pool.
RES_CASES = [
    _case("n64_83x61_sdf", 83, 61, 64, (60.0, 60.0, 41.5, 30.5), SDF, 0.1, 6, 40, 1500, pooled=1 << 10),
    _case("n64_83x61_ofusion", 83, 61, 64, (60.0, 60.0, 41.5, 30.5), OFUSION, 0.02, 6, 40, 1500, pooled=1 << 10),
    _case("n4096_161x121_sdf", 161, 121, 4096, (481.2, 480.0, 77.3, 63.9), SDF, 0.02, 6, 40000, 15000, pooled=1 << 17),
    _case("n4096_161x121_ofusion", 161, 121, 4096, (481.2, 480.0, 77.3, 63.9), OFUSION, 0.01, 6, 40000, 15000, pooled=1 << 17),
]

# Small maps for mesh() and query() at the two resolutions (query()'s oracle octree is built point by point in Python).  Too few frames for the
# stream's own raycast gate: min_hits is that of one raycast from the last pose.
MAP_CASES = [
    _case("map_n64_sdf", 83, 61, 64, (60.0, 60.0, 41.5, 30.5), SDF, 0.1, 3, 40, 1000),
    _case("map_n64_ofusion", 83, 61, 64, (60.0, 60.0, 41.5, 30.5), OFUSION, 0.02, 3, 40, 1500),
    _case("map_n4096_sdf", 41, 31, 4096, (481.2, 480.0, 20.3, 15.9), SDF, 0.02, 2, 1000, 800),
    _case("map_n4096_ofusion", 41, 31, 4096, (481.2, 480.0, 20.3, 15.9), OFUSION, 0.01, 3, 1000, 800),
]

# The consumers (renderDepth / renderVolume / renderTrack, tracking, set_depth_mm) at a ragged shape with a general camera
CONSUMER = dict(W=163, H=101, N=256, dim=4.8, k=(150.0, 130.0, 70.3, 55.1))

ALL_CASES = SHAPE_CASES + RES_CASES + MAP_CASES
