"""The stress scene of supereight_amd/synthetic.py through any pinhole camera at any pose, and the tables of camera attitudes that
tests/test_gpu_attitudes.py integrates against the oracle.

Every frame the other suites integrate comes from ``synthetic.pose`` (+z, 0.2 deg of yaw per frame) or ``synthetic.stress_pose`` (yaw within +-90 deg,
pitch within +-5 deg, no roll).  ``ATTITUDES`` holds what those paths never reach: views along every axis with exact 0 / +-1 rotation entries, rolls
by right angles, rotations without a zero entry, cameras outside the volume, surfaces outside it, a camera that looks out of it and a camera that
stands exactly on a block's min corner.  ``TUMBLE`` strings them into one sequence on one map, so that most of the map lies beside or behind the
camera from the second frame on.  tests/test_attitude_frames_oracle.py holds the oracle alone to what each entry is meant to exercise, so that no
case can turn vacuous unnoticed.  synthetic.py itself is untouched: the golden fixtures pin it."""
from __future__ import annotations

import numpy as np

from oracle.binding import OFUSION, SDF
from supereight_amd import synthetic as S
from tests.parity_util import look

DIM = 2.4
SHAPES = {"80x60_128": (80, 60, 128), "160x120_256": (160, 120, 256)}
FIELDS = {"sdf": (SDF, 0.1), "ofusion": (OFUSION, 0.02)}


def aniso_k(W: int) -> np.ndarray:
    """The anisotropic, off-centre camera of edge_frames' ragged case, scaled to an image W wide."""
    return (np.array([200.0, 90.0, 30.0, 80.0]) * (W / 161.0)).astype(np.float32)


def render_scene_mm(T, W: int, H: int, dim: float, k) -> np.ndarray:
    """uint16 millimetre z-depth image of the stress scene (STRESS_ROOM_*, STRESS_SPHERES, STRESS_PILLAR) seen with intrinsics
    k = (fx, fy, cx, cy) from the camera->world pose T.  A camera inside the room sees its walls from inside, as render_stress_depth does; one
    outside sees only the spheres and the pillar.  A ray that meets nothing gives 0, the reference's "no measurement"."""
    k = np.asarray(k, np.float32).astype(np.float64)
    T = np.asarray(T, np.float32).astype(np.float64)
    xs = (np.arange(W) + 0.5 - k[2]) / k[0]
    ys = (np.arange(H) + 0.5 - k[3]) / k[1]
    u, v = np.meshgrid(xs, ys)
    d = np.stack([u, v, np.ones_like(u)], axis=-1) @ T[:3, :3].T   # t == camera z-depth
    o = T[:3, 3]
    lo, hi = np.array(S.STRESS_ROOM_LO) * dim, np.array(S.STRESS_ROOM_HI) * dim
    if ((o > lo) & (o < hi)).all():
        with np.errstate(divide="ignore", invalid="ignore"):
            t_axis = np.where(d > 0, (hi - o) / d, np.where(d < 0, (lo - o) / d, np.inf))
        depth = t_axis.min(axis=-1)
    else:
        depth = np.full(u.shape, np.inf)
    for c, r in S.STRESS_SPHERES:
        depth = np.minimum(depth, S._ray_sphere(o, d, np.array(c) * dim, r * dim))
    depth = np.minimum(depth, S._ray_box_outside(o, d, np.array(S.STRESS_PILLAR[0]) * dim, np.array(S.STRESS_PILLAR[1]) * dim))
    mm = np.where(np.isfinite(depth), np.clip(np.floor(depth * 1000.0), 0, 65535), 0.0)
    return np.ascontiguousarray(mm.astype(np.uint16))


def metres(mm: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(mm.astype(np.float32) / np.float32(1000.0))   # mm2metersKernel: depth / 1000.0f


# Rotations with entries exactly 0 and +-1 (columns: the camera's x, y, z axes in the world), so that the sweep's delta = R . (voxel, 0, 0) and
# cdelta = K3 . delta hold exact zeros; cos(90 deg) from look() would leave 6e-17 there.
_AXIS_R = {
    "+z": ((1, 0, 0), (0, 1, 0), (0, 0, 1)),
    "-z": ((-1, 0, 0), (0, 1, 0), (0, 0, -1)),
    "+x": ((0, 0, 1), (0, 1, 0), (-1, 0, 0)),
    "-x": ((0, 0, -1), (0, 1, 0), (1, 0, 0)),
    "+y": ((1, 0, 0), (0, 0, 1), (0, -1, 0)),
    "-y": ((1, 0, 0), (0, 0, -1), (0, 1, 0)),
    "roll90": ((0, -1, 0), (1, 0, 0), (0, 0, 1)),
    "roll180": ((-1, 0, 0), (0, -1, 0), (0, 0, 1)),
    "roll270": ((0, 1, 0), (-1, 0, 0), (0, 0, 1)),
}


def _exact(position, rot):
    def make(dim, N):
        T = look(np.asarray(position, np.float64) * dim)
        T[:3, :3] = np.asarray(_AXIS_R[rot], np.float32)
        return T
    return make


def _looking(position, **angles):
    return lambda dim, N: look(np.asarray(position, np.float64) * dim, **angles)


def corner_block(N: int) -> np.ndarray:
    """Voxel coordinates of the block on whose min corner the on_block_corner cameras stand: the block the room's +x wall (x = 0.93) crosses or
    just clears, half way up, at z = 0.625 -- a place the +z view of TUMBLE's first frame fuses."""
    return np.array([(int(0.93 * N) - 4) // 8 * 8, N // 2, 5 * N // 8], np.int32)


def _on_corner(rot=None, **angles):
    def make(dim, N):
        # the translation the kernels compute for that corner: float32(coordinate) * float32(dim / N), as projective_functor.hpp forms it
        T = look(np.zeros(3), **angles)
        T[:3, 3] = corner_block(N).astype(np.float32) * (np.float32(dim) / np.float32(N))
        if rot is not None:
            T[:3, :3] = np.asarray(_AXIS_R[rot], np.float32)
        return T
    return make


# name -> (pose(dim, N), purpose).  Positions are fractions of dim.  The scene: walls inside the volume at x = 0.93, y = 0.06 / 0.94, z = 0.04, walls
# outside it at x = -0.12 and z = 1.18, a pillar at x 0.6-0.7, z 0.36-0.44, spheres at (0.5, 0.5, 0.62) and, across the x = 0 face, (0.02, 0.4, 0.5).
_PLUS_Z_AT = (0.72, 0.5, 0.06)      # (the stream's own start position faces the wall outside the cube and fuses next to nothing)
ATTITUDES = {
    "+z": (_exact(_PLUS_Z_AT, "+z"), "optical axis exactly +z: R = I, the stream's own half-space with exact zeros"),
    "-z": (_exact((0.5, 0.5, 0.9), "-z"), "optical axis exactly -z: camera z falls as world z grows"),
    "+x": (_exact((0.1, 0.55, 0.55), "+x"), "optical axis exactly +x: delta = (0, 0, -voxel), the sweep's x loop runs along the ray"),
    "-x": (_exact((0.88, 0.5, 0.3), "-x"), "optical axis exactly -x: the x loop runs against the ray"),
    "+y": (_exact((0.45, 0.15, 0.5), "+y"), "optical axis exactly +y: image rows run along world z"),
    "-y": (_exact((0.45, 0.85, 0.5), "-y"), "optical axis exactly -y"),
    "roll90": (_exact(_PLUS_Z_AT, "roll90"), "+z view rolled by 90 deg: delta has a zero x and cdelta.x comes from y alone"),
    "roll180": (_exact(_PLUS_Z_AT, "roll180"), "+z view upside down: delta.x < 0 at R.z = +z"),
    "roll270": (_exact(_PLUS_Z_AT, "roll270"), "+z view rolled by 270 deg"),
    "generic": (_looking((0.3, 0.4, 0.2), yaw_deg=35, pitch_deg=20, roll_deg=25), "no zero entry in R"),
    "generic_pitched": (_looking((0.5, 0.75, 0.3), yaw_deg=-30, pitch_deg=55, roll_deg=-15), "no zero entry in R, pitched beyond 45 deg"),
    "outside_low": (_looking((0.3, 0.45, -0.5), yaw_deg=4, pitch_deg=-3), "camera 0.5 dim beyond the z = 0 face: band walks start outside the cube"),
    "outside_high": (_looking((1.5, 0.5, 0.55), yaw_deg=-93, pitch_deg=2), "camera 0.5 dim beyond the x = dim face, looking in"),
    "surface_outside": (_looking((0.3, 0.3, 0.5), yaw_deg=-45, pitch_deg=25), "the -x and +z walls outside the cube: whole bands at negative coordinates or beyond size"),
    # (through the x = 0 face, not z = dim: the wall beyond it is near enough that OFusion's 10- and 30-voxel steps towards the camera all land
    # outside the cube at both resolutions; at z = dim some land in the last quarter voxel in front of the camera)
    "looking_out": (_looking((0.002, 0.7, 0.8), yaw_deg=-87, pitch_deg=2), "inside, at the x = 0 face, looking out: valid pixels and not one band step in the volume"),
    "on_block_corner": (_on_corner(yaw_deg=-100, pitch_deg=15, roll_deg=20), "translation exactly a block's min corner, generic rotation"),
    "on_block_corner_axis": (_on_corner(rot="-z"), "translation exactly a block's min corner, R exact: that corner is (0, 0, 0) in the camera, 0 / 0 in se_in_frustum"),
}

CORNER_ATTITUDES = ("on_block_corner", "on_block_corner_axis")


def attitude_pose(name: str, dim: float, N: int) -> np.ndarray:
    return ATTITUDES[name][0](dim, N)


# One sequence on one map, frame number = index: consecutive frames look in opposite or orthogonal directions, so that from frame 1 on most of
# the map lies beside or behind the camera.  The corner cameras come late: by then their block exists through fusion (frame 0 sees that wall).
TUMBLE = ("+z", "-z", "+x", "-x", "roll90", "+y", "-y", "generic", "outside_high", "roll270", "on_block_corner", "outside_low",
          "on_block_corner_axis", "surface_outside")


class AttitudeStream:
    """The frame source run_both takes: ``depth(f)``, ``pose(f)``, ``k`` for a sequence of ATTITUDES names (default: TUMBLE)."""

    def __init__(self, W: int, H: int, N: int, dim: float = DIM, k=None, names=TUMBLE):
        self.W, self.H, self.N, self.dim, self.names = W, H, N, float(dim), tuple(names)
        self.k = np.ascontiguousarray(S.intrinsics(W) if k is None else k, np.float32)

    def __len__(self):
        return len(self.names)

    def pose(self, f: int) -> np.ndarray:
        return attitude_pose(self.names[f], self.dim, self.N)

    def depth_mm(self, f: int) -> np.ndarray:
        return render_scene_mm(self.pose(f), self.W, self.H, self.dim, self.k)

    def depth(self, f: int) -> np.ndarray:
        return metres(self.depth_mm(f))


def block_key(lib, coords, N: int) -> np.ndarray:
    """The (code | level) key of the block at voxel coordinates `coords` for OraclePipeline.insert_octants."""
    depth = int(np.log2(N))
    return np.array([lib.so_encode(int(coords[0]), int(coords[1]), int(coords[2]), depth - 3, depth)], np.uint64)


def sdf_steps(mu: float, dim: float, N: int) -> int:
    """numSteps of buildAllocationList (kfusion/alloc_impl.hpp:68): ceil(band / voxelSize) with band = 2 mu, in float32."""
    voxel = np.float32(dim) / np.float32(N)
    return int(np.ceil(np.float32(2 * np.float32(mu)) * (np.float32(1) / voxel)))


def ofusion_steps(depth, T, k, mu: float, dim: float, N: int) -> int:
    """The steps buildOctantList's walk takes over all valid pixels, inside the volume or not (bfusion/alloc_impl.hpp:84-127): a float32
    restatement of `for (travelled = 0; travelled < dist; travelled += stepsize)` with compute_stepsize, per pixel."""
    f32 = np.float32
    H, W = depth.shape
    voxel = f32(dim) / f32(N)
    band = f32(6) * f32(mu)
    fx, fy, cx, cy = (f32(v) for v in np.asarray(k, np.float32))
    T = np.asarray(T, np.float32)
    x, y = np.meshgrid(np.arange(W, dtype=np.float32) + f32(0.5), np.arange(H, dtype=np.float32) + f32(0.5))
    valid = depth != 0
    dd = depth[valid]
    cam_pt = np.stack([(x[valid] - cx) / fx * dd, (y[valid] - cy) / fy * dd, dd], axis=-1).astype(np.float32)
    world = (cam_pt @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    to_cam = (T[:3, 3] - world).astype(np.float32)
    direction = to_cam / np.sqrt((to_cam * to_cam).sum(-1, dtype=np.float32))[:, None]
    origin = world - (band * f32(0.5)) * direction
    dist = np.sqrt(((T[:3, 3] - origin) ** 2).sum(-1, dtype=np.float32)).astype(np.float32)
    travelled = np.zeros_like(dist)
    steps = 0
    live = travelled < dist
    while live.any():
        steps += int(live.sum())
        step = np.where(travelled < band, voxel, np.where(travelled < band + band * f32(0.5), f32(10) * voxel, f32(30) * voxel)).astype(np.float32)
        travelled = np.where(live, travelled + step, travelled).astype(np.float32)
        live = live & (travelled < dist)
    return steps


def camera_frame(points_m, T):
    """World points (metres) in the camera frame of the camera->world pose T, in float64."""
    T = np.asarray(T, np.float64)
    return (np.asarray(points_m, np.float64) - T[:3, 3]) @ T[:3, :3]


def behind_and_in_image(points_m, T, k, W: int, H: int, margin: float = 2.0) -> np.ndarray:
    """Mask of the world points with camera z < 0 whose projection (fx x / z + cx, fy y / z + cy) -- what se_in_frustum forms without a z > 0 test,
    filter.hpp:38-49 -- lies inside the image by `margin` pixels.  float64; the margin makes the float width irrelevant."""
    pc = camera_frame(points_m, T)
    k = np.asarray(k, np.float64)
    z = pc[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = k[0] * pc[:, 0] / z + k[2]
        v = k[1] * pc[:, 1] / z + k[3]
    return (z < 0) & (u >= margin) & (u <= W - 1 - margin) & (v >= margin) & (v <= H - 1 - margin)


def node_corners_m(lib, code, side, dim: float, N: int) -> np.ndarray:
    """The 8 child corners of every node, in metres, as update_node forms them (projective_functor.hpp:113-137): unpack_morton(code_), level
    bits included, plus 0 or side / 2 per axis."""
    out = np.zeros((len(code), 8, 3), np.float64)
    v = np.zeros(3, np.int32)
    voxel = dim / N
    for i, (c, s) in enumerate(zip(code, side)):
        lib.so_unpack_morton(int(c), v)
        for j in range(8):
            out[i, j] = (v + 0.5 * float(s) * np.array([j & 1, (j >> 1) & 1, (j >> 2) & 1])) * voxel
    return out.reshape(-1, 3)
