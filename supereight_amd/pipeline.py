"""Host-side mirror of the reference's DenseSLAMSystem hot-path interface over the C ABI.

``DenseSLAMPipeline`` keeps the reference's method names and semantics for the path this
repository implements (se_denseslam/include/se/DenseSLAMSystem.h:193-212, 295, 353):
``integration(k, integration_rate, mu, frame)`` and ``raycasting(k, mu, frame)`` return the
reference's "did this stage run" booleans, ``setPose`` injects the camera pose, ``getMap``-style
read-back comes from ``blocks()`` / ``nodes()``.  All compute happens in libse_hip.so
(hand-written HIP for gfx950); there is no CPU fallback -- loading fails loudly without it.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import build as _build

SDF, OFUSION = 0, 1
KERNELS = ("alloc_scan", "alloc_commit", "integrate", "raycast", "apply_bricks")
STAT_NAMES = ("probes", "new_keys", "swept", "nodes", "gets", "interps", "grads", "hits",
              "clk_iter", "clk_march", "clk_grad", "clk_wave_max", "clk_stage", "r13", "r14", "r15")

_f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
_LIB = None
# The per-frame entry points (se_hip_frame, se_hip_frame_tracked, se_hip_integrate, se_hip_raycast, se_hip_track, ...) take the pose, the
# intrinsics and the pyramid as plain addresses: an ndpointer argument costs ctypes 3 - 5 us of Python per call (type, dtype and flag checks),
# two of them were 10 % of a closed-loop frame.  DenseSLAMPipeline checks an array once (_addr) and remembers its address for as long as it
# holds the array.


class SeHipError(RuntimeError):
    pass


class _QueryOut(C.Structure):
    """se_hip_query_out of include/se_hip.h: output addresses, 0 = not wanted."""
    _fields_ = [("fine", C.c_void_p), ("coarse", C.c_void_p), ("interp", C.c_void_p), ("grad", C.c_void_p), ("status", C.c_void_p)]


class _RayOut(C.Structure):
    """se_hip_ray_out of include/se_hip.h: output addresses, 0 = not wanted."""
    _fields_ = [("hit", C.c_void_p), ("normal", C.c_void_p), ("status", C.c_void_p)]


class _MeshView(C.Structure):
    """se_hip_mesh_view of include/se_hip.h."""
    _fields_ = [("pose", C.c_float * 16), ("k", C.c_float * 4), ("width", C.c_int32), ("height", C.c_int32)]


class _MeshSelect(C.Structure):
    """se_hip_mesh_select of include/se_hip.h."""
    _fields_ = [("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("n_views", C.c_int32), ("flags", C.c_uint32), ("views", C.POINTER(_MeshView))]


class _MeshOut(C.Structure):
    """se_hip_mesh_out of include/se_hip.h: output addresses and capacities."""
    _fields_ = [("triangles", C.c_void_p), ("capacity_triangles", C.c_int64), ("block_coords", C.c_void_p), ("block_range", C.c_void_p),
                ("capacity_blocks", C.c_int64), ("header", C.c_void_p)]


MESH_MAX_VIEWS, MESH_SKIP_EMPTY = 64, 1

# status bits of se_hip_cast_rays
RAY_VALID, RAY_ENTERED, RAY_HIT, RAY_NORMAL = 1, 2, 4, 8


class _CollideTest(C.Structure):
    """se_hip_collide_test of include/se_hip.h."""
    _fields_ = [("threshold", C.c_float), ("occupied_above", C.c_int32)]


# status codes of se_hip_collide_boxes (the order of se::geometry::collision_status; combining takes the minimum)
COLLISION_OCCUPIED, COLLISION_UNSEEN, COLLISION_EMPTY, COLLISION_INVALID = 0, 1, 2, 255
_COLLIDE_MODES = {"strict": 0, "reference": 1}


class _MotionOut(C.Structure):
    """se_hip_motion_out of include/se_hip.h: output addresses, t_first 0 = not wanted."""
    _fields_ = [("status", C.c_void_p), ("t_first", C.c_void_p)]


# t_first of se_hip_collide_motions when nothing blocks the motion; what stop_at may name
MOTION_FREE = 2.0


class _OrientedMotionOut(C.Structure):
    """se_hip_oriented_motion_out of include/se_hip.h: output addresses, t_first / t_exact 0 = not wanted."""
    _fields_ = [("status", C.c_void_p), ("t_first", C.c_void_p), ("t_exact", C.c_void_p)]


_MOTION_STOPS = {"occupied": COLLISION_OCCUPIED, "unseen": COLLISION_UNSEEN}


class _ClearanceOut(C.Structure):
    """se_hip_clearance_out of include/se_hip.h: output addresses, nearest 0 = not wanted."""
    _fields_ = [("d2", C.c_void_p), ("nearest", C.c_void_p)]


# d2 of se_hip_clearance_boxes when nothing blocks within r_max, and for an invalid query
CLEARANCE_NONE, CLEARANCE_INVALID = -1, -2
_CLEARANCE_R_CLAMP = 32768   # an r_max above 32767 is invalid: larger ones are passed as this one, so that they fit the int32 column


class _ProjectRequest(C.Structure):
    """se_hip_project_request of include/se_hip.h."""
    _fields_ = [("axis", C.c_int32), ("lo", C.c_int32 * 2), ("side", C.c_int32 * 2), ("n_layers", C.c_int32), ("layers", (C.c_int32 * 2) * 16),
                ("stop_at", C.c_int32)]


class _ProjectOut(C.Structure):
    """se_hip_project_out of include/se_hip.h: output addresses, 0 = not wanted (status is required)."""
    _fields_ = [("status", C.c_void_p), ("first", C.c_void_p), ("last", C.c_void_p), ("count", C.c_void_p)]


# first / last of se_hip_project_columns for a cell without a blocking voxel; the bounds of a valid request
PROJECT_NONE, PROJECT_LIMIT, PROJECT_MAX_LAYERS, PROJECT_MAX_CELLS = -(1 << 31), 1 << 20, 16, 1 << 28


class _FieldRequest(C.Structure):
    """se_hip_field_request of include/se_hip.h."""
    _fields_ = [("lo", C.c_int32 * 3), ("side", C.c_int32 * 3), ("robot", C.c_int32 * 3), ("r_max", C.c_int32), ("stop_at", C.c_int32)]


class _FieldOut(C.Structure):
    """se_hip_field_out of include/se_hip.h: output addresses, nearest 0 = not wanted."""
    _fields_ = [("d2", C.c_void_p), ("nearest", C.c_void_p)]


# the bounds of a valid se_hip_distance_field request
FIELD_LIMIT, FIELD_R_MAX, FIELD_ROBOT_MAX, FIELD_MAX_VOXELS, FIELD_MAX_WORK = 1 << 19, 255, 256, 1 << 24, 1 << 28


class _ReachRequest(C.Structure):
    """se_hip_reach_request of include/se_hip.h (seeds: a host address)."""
    _fields_ = [("lo", C.c_int32 * 3), ("side", C.c_int32 * 3), ("robot", C.c_int32 * 3), ("stop_at", C.c_int32), ("n_seeds", C.c_int32),
                ("seeds", C.c_void_p)]


class _ReachOut(C.Structure):
    """se_hip_reach_out of include/se_hip.h: output addresses, 0 = not wanted (steps is required; counts is a host address)."""
    _fields_ = [("steps", C.c_void_p), ("seed", C.c_void_p), ("next", C.c_void_p), ("counts", C.c_void_p)]


# steps / next of se_hip_reach_field for an unreached position and at a seed; the most seeds a request may hold
REACH_NONE, REACH_AT_SEED, REACH_MAX_SEEDS = -1, 6, 255
# the moves that next's codes 0 .. 5 name (x, y, z)
REACH_MOVES = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))


def reach_path(next, lo, start) -> np.ndarray:
    """The path that DenseSLAMPipeline.reach_field's `next` [side z, side y, side x] describes from the position `start` (x, y, z; absolute
    voxel coordinates, `lo` the region's) to its seed: int64 [steps + 1, 3], `start` first, the seed last.  Empty [0, 3] where next is 255
    (not free, or cut off from every seed) or `start` lies outside the region.  Pure numpy; bounded by the array's size, so an array that
    is no navigation function raises ValueError instead of looping."""
    nx = np.asarray(next)
    if nx.ndim != 3 or nx.dtype != np.uint8:
        raise ValueError(f"reach_path: next must be a uint8 array [side z, side y, side x], got {nx.dtype} {list(nx.shape)}")
    lo = [int(v) for v in np.asarray(lo).reshape(3)]
    pos = [int(v) for v in np.asarray(start).reshape(3)]
    side = (nx.shape[2], nx.shape[1], nx.shape[0])
    path = []
    for _ in range(nx.size + 1):
        rel = [pos[k] - lo[k] for k in range(3)]
        if not all(0 <= rel[k] < side[k] for k in range(3)):
            if path:
                raise ValueError("reach_path: next leads out of the region")
            break
        code = int(nx[rel[2], rel[1], rel[0]])
        if code == 255:
            if path:
                raise ValueError("reach_path: next leads to a position without a move")
            break
        path.append(tuple(pos))
        if code == REACH_AT_SEED:
            return np.array(path, np.int64).reshape(-1, 3)
        if code > 5:
            raise ValueError(f"reach_path: unknown code {code}")
        pos = [pos[k] + REACH_MOVES[code][k] for k in range(3)]
    if path:
        raise ValueError("reach_path: next does not arrive at a seed")
    return np.zeros((0, 3), np.int64)


# se_hip_collide_oriented: sub-units per voxel, and the bounds of a valid box (|c_k|, |h_ik|, in sub-units)
ORIENTED_SUB, ORIENTED_CENTRE_LIMIT, ORIENTED_AXIS_LIMIT = 16, 1 << 20, 1 << 14


def oriented_boxes(centres_m, rotations, half_extents_m, dim, size):
    """The int32 [N, 12] boxes of DenseSLAMPipeline.collides_oriented from metric ones: centres_m [N, 3] in metres, rotations [N, 3, 3] (box
    frame to world; column i is the direction of the box's axis i), half_extents_m [N, 3] in metres, for a volume of `size` voxels over `dim`
    metres.  The centre and the scaled columns half_extents_m[i] * rotations[:, :, i] are rounded to the nearest sub-unit (1 / ORIENTED_SUB
    voxel).  The query's answer is exact for the rounded box: each of the four vectors moves by at most sqrt(3) / 2 sub-unit, so every point
    of the rounded box lies within 4 * sqrt(3) / 32 = sqrt(3) / 8 voxel of the corresponding point of the box asked for.  Values beyond int32
    are clamped to it (such a box is invalid anyway)."""
    c = np.asarray(centres_m, np.float64)
    r = np.asarray(rotations, np.float64)
    e = np.asarray(half_extents_m, np.float64)
    if c.ndim != 2 or c.shape[1] != 3:
        raise ValueError(f"oriented_boxes: centres_m must have shape [N, 3], got {list(c.shape)}")
    n = c.shape[0]
    if r.shape != (n, 3, 3):
        raise ValueError(f"oriented_boxes: rotations must have shape [{n}, 3, 3], got {list(r.shape)}")
    if e.shape != (n, 3):
        raise ValueError(f"oriented_boxes: half_extents_m must have shape [{n}, 3], got {list(e.shape)}")
    if not (np.isfinite(c).all() and np.isfinite(r).all() and np.isfinite(e).all()):
        raise ValueError("oriented_boxes: non-finite input")
    scale = ORIENTED_SUB * float(size) / float(dim)
    out = np.empty((n, 12), np.float64)
    out[:, 0:3] = c * scale
    for i in range(3):
        out[:, 3 + 3 * i:6 + 3 * i] = r[:, :, i] * e[:, i:i + 1] * scale
    return np.clip(np.rint(out), -(2 ** 31), 2 ** 31 - 1).astype(np.int32)


# se_hip_collide_oriented_motions: the bound of a valid displacement (|d_k|, in sub-units)
ORIENTED_MOVE_LIMIT = 1 << 18


def oriented_motions(centres_m, rotations, half_extents_m, displacements_m, dim, size):
    """The int32 [N, 15] motions of DenseSLAMPipeline.collides_oriented_moving from metric ones: the box as oriented_boxes() rounds it (centres_m
    [N, 3], rotations [N, 3, 3], half_extents_m [N, 3]), then displacements_m [N, 3] in metres rounded to the nearest sub-unit like the centre.
    The query's answer is exact for the rounded motion.  Values beyond int32 are clamped to it (such a motion is invalid anyway)."""
    boxes = oriented_boxes(centres_m, rotations, half_extents_m, dim, size)
    d = np.asarray(displacements_m, np.float64)
    if d.shape != (boxes.shape[0], 3):
        raise ValueError(f"oriented_motions: displacements_m must have shape [{boxes.shape[0]}, 3], got {list(d.shape)}")
    if not np.isfinite(d).all():
        raise ValueError("oriented_motions: non-finite input")
    scale = ORIENTED_SUB * float(size) / float(dim)
    dd = np.clip(np.rint(d * scale), -(2 ** 31), 2 ** 31 - 1).astype(np.int32)
    return np.ascontiguousarray(np.concatenate([boxes, dd], 1))


class _TraceOut(C.Structure):
    """se_hip_trace_out of include/se_hip.h: output addresses, 0 = not wanted (status is required)."""
    _fields_ = [("status", C.c_void_p), ("t_first", C.c_void_p), ("first", C.c_void_p), ("counts", C.c_void_p)]


# se_hip_trace_segments: the bound of a valid segment (|coordinate| of a and b, in sub-units of 1 / ORIENTED_SUB voxel), and `first` where nothing blocks
SEGMENT_LIMIT, TRACE_NONE = 1 << 22, -(1 << 31)


def _odd_sub_units(x):
    """float64 sub-units -> the nearest odd integer, 2 rint((x - 1) / 2) + 1, clamped to int32 (an odd value at either end)."""
    return np.clip(2.0 * np.rint((x - 1.0) / 2.0) + 1.0, -(2.0 ** 31 - 1), 2.0 ** 31 - 1).astype(np.int32)


def segments_from_points(a_m, b_m, dim, size):
    """The int32 [N, 6] segments of DenseSLAMPipeline.trace from metric endpoints: a_m, b_m [N, 3] in metres, for a volume of `size` voxels over
    `dim` metres.  Each coordinate x * ORIENTED_SUB * size / dim is rounded to the nearest *odd* sub-unit, 2 rint((x - 1) / 2) + 1: an endpoint
    therefore never lies on a voxel boundary (a multiple of 16), and an axis-parallel segment never lies in a grid plane, where it would touch
    nothing.  The query's answer is exact for the rounded segment: each coordinate moves by at most one sub-unit, an endpoint by at most
    sqrt(3) / 16 voxel.  Values beyond int32 are clamped to it (such a segment is invalid anyway)."""
    a = np.asarray(a_m, np.float64)
    b = np.asarray(b_m, np.float64)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"segments_from_points: a_m must have shape [N, 3], got {list(a.shape)}")
    if b.shape != a.shape:
        raise ValueError(f"segments_from_points: b_m must have shape {list(a.shape)}, got {list(b.shape)}")
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        raise ValueError("segments_from_points: non-finite input")
    if not (dim > 0 and size > 0):
        raise ValueError("segments_from_points: dim and size must be positive")
    scale = ORIENTED_SUB * float(size) / float(dim)
    return np.ascontiguousarray(np.concatenate([_odd_sub_units(a * scale), _odd_sub_units(b * scale)], 1))


def view_segments(pose, k, width, height, stride, near, far, dim, size):
    """The segments of a camera view for DenseSLAMPipeline.trace: pose (4 x 4, camera to world, metres), k = (fx, fy, cx, cy), the rays
    through the pixels (u, v), u = 0, stride, 2 stride, ... < width and v likewise (pixel centres are the integer coordinates, as in the
    raycast), row by row.  A ray runs from its origin + near * e to + far * e with e = R normalised((u - cx) / fx, (v - cy) / fy, 1), is
    clipped in float64 to the cube [0, dim]^3 and snapped as segments_from_points snaps (then kept within 1 .. 16 size - 1, so that it stays
    inside the cube).  Returns (segments int32 [M, 6] of the rays that meet the cube, in ray order; missed int64: the indices of the rays
    that do not)."""
    T = np.asarray(pose, np.float64)
    kk = np.asarray(k, np.float64).reshape(-1)
    if T.shape != (4, 4) or not np.isfinite(T).all():
        raise ValueError("view_segments: pose must be a finite 4x4 matrix")
    if kk.shape != (4,) or not np.isfinite(kk).all() or kk[0] == 0 or kk[1] == 0:
        raise ValueError("view_segments: k must be four finite numbers (fx, fy, cx, cy) with fx, fy != 0")
    for name, v in (("width", width), ("height", height), ("stride", stride)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"view_segments: {name} must be a positive integer, got {v!r}")
    if not (np.isfinite(near) and np.isfinite(far) and 0 <= near < far):
        raise ValueError(f"view_segments: 0 <= near < far must hold, got {near!r}, {far!r}")
    if not (dim > 0 and size > 0):
        raise ValueError("view_segments: dim and size must be positive")
    u, v = np.meshgrid(np.arange(0, width, stride, dtype=np.float64), np.arange(0, height, stride, dtype=np.float64))
    e = np.stack([(u.reshape(-1) - kk[2]) / kk[0], (v.reshape(-1) - kk[3]) / kk[1], np.ones(u.size)], 1)
    e = (e / np.linalg.norm(e, axis=1, keepdims=True)) @ T[:3, :3].T
    a, b = T[:3, 3] + near * e, T[:3, 3] + far * e
    # the part of a + s (b - a), s in [0, 1], inside the cube: the slab test per axis
    d = b - a
    s0, s1 = np.zeros(len(a)), np.ones(len(a))
    with np.errstate(divide="ignore", invalid="ignore"):
        for j in range(3):
            lo, hi = (0.0 - a[:, j]) / d[:, j], (float(dim) - a[:, j]) / d[:, j]
            still = d[:, j] == 0
            inside = (a[:, j] >= 0) & (a[:, j] <= dim)
            lo, hi = np.where(still, np.where(inside, -np.inf, np.inf), np.minimum(lo, hi)), np.where(still, np.where(inside, np.inf, -np.inf), np.maximum(lo, hi))
            s0, s1 = np.maximum(s0, lo), np.minimum(s1, hi)
    hit = s0 < s1
    a, b = (a + s0[:, None] * d)[hit], (a + s1[:, None] * d)[hit]
    seg = segments_from_points(np.clip(a, 0.0, dim), np.clip(b, 0.0, dim), dim, size)
    return np.ascontiguousarray(np.clip(seg, 1, ORIENTED_SUB * int(size) - 1)), np.nonzero(~hit)[0].astype(np.int64)


class _Edit(C.Structure):
    """se_hip_edit of include/se_hip.h (40 bytes)."""
    _fields_ = [("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("x", C.c_float), ("y", C.c_float), ("flags", C.c_uint32), ("only", C.c_uint32)]


# se_hip_edit as a numpy record (the host entry's input) -- on the device the same 40 bytes are a torch int32 [N, 10] tensor whose
# columns 6 and 7 hold the bits of the two floats
EDIT_DTYPE = np.dtype([("lo", np.int32, 3), ("hi", np.int32, 3), ("x", np.float32), ("y", np.float32), ("flags", np.uint32), ("only", np.uint32)])
EDIT_SET_X, EDIT_SET_Y, EDIT_BLOCKS, EDIT_NODES = 1, 2, 4, 8
EDIT_OCCUPIED, EDIT_UNSEEN, EDIT_EMPTY, EDIT_ANY = 1, 2, 4, 7      # bits of se_hip_edit.only: 1 << COLLISION_*
_EDIT_MODES = {"strict": 0, "reference": 1}
_EDIT_CLASSES = {"occupied": EDIT_OCCUPIED, "unseen": EDIT_UNSEEN, "empty": EDIT_EMPTY, "any": EDIT_ANY}


class _AllocBox(C.Structure):
    """se_hip_alloc_box of include/se_hip.h (32 bytes)."""
    _fields_ = [("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("level", C.c_int32), ("reserved", C.c_uint32)]


# se_hip_alloc_box as a numpy record (the host entry's input) -- on the device the same 32 bytes are a torch int32 [N, 8] tensor
ALLOC_DTYPE = np.dtype([("lo", np.int32, 3), ("hi", np.int32, 3), ("level", np.int32), ("reserved", np.uint32)])
# se_hip_release_box
RELEASE_DTYPE = np.dtype([("lo", np.int32, 3), ("side", np.int32, 3), ("what", np.int32), ("reserved", np.int32)])


class _Config(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("volume_resolution", C.c_int32),
                ("volume_dimension", C.c_float), ("field_type", C.c_int32), ("device", C.c_int32),
                ("max_blocks", C.c_int64), ("row_begin", C.c_int32), ("row_end", C.c_int32)]


class _MergeRule(C.Structure):      # se_hip_merge_rule
    _fields_ = [("mode", C.c_int32), ("max_weight", C.c_float)]


EXPORTS = {
    "se_hip_create": (C.c_int, [C.POINTER(_Config), C.POINTER(C.c_void_p)]),
    "se_hip_destroy": (C.c_int, [C.c_void_p]),
    "se_hip_last_error": (C.c_char_p, []),
    "se_hip_sync": (C.c_int, [C.c_void_p]),
    "se_hip_memory_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "se_hip_set_pinned_input": (C.c_int, [C.c_void_p, C.c_int32]),
    "se_hip_host_alloc": (C.c_void_p, [C.c_size_t]),
    "se_hip_host_free": (None, [C.c_void_p]),
    "se_hip_clear_overflow": (C.c_int, [C.c_void_p]),
    "se_hip_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "se_hip_set_scan_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "se_hip_scan_overlaps": (C.c_int, [C.c_void_p]),
    "se_hip_frame_is_fused": (C.c_int, [C.c_void_p]),
    "se_hip_set_streaming": (C.c_int, [C.c_void_p, C.c_int32]),
    "se_hip_set_image_ring": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "se_hip_raycast_deferred": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_uint32]),
    "se_hip_get_launch_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_int32]),
    "se_hip_upload_depth": (C.c_int, [C.c_void_p, _f32p]),
    "se_hip_upload_depth_mm": (C.c_int, [C.c_void_p, np.ctypeslib.ndpointer(dtype=np.uint16, flags="C_CONTIGUOUS"), C.c_int32, C.c_int32]),
    "se_hip_set_depth_device": (C.c_int, [C.c_void_p, C.c_void_p]),
    "se_hip_integrate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32]),
    "se_hip_alloc_scan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32]),
    "se_hip_new_keys_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "se_hip_set_new_keys_buffer": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "se_hip_alloc_commit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64]),
    "se_hip_set_exchange": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    "se_hip_alloc_exchange": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "se_hip_integrate_sweep": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32]),
    "se_hip_sweep_shard_bytes": (C.c_size_t, [C.c_size_t]),
    "se_hip_set_sweep_shard": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t]),
    "se_hip_apply_bricks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "se_hip_brick_exchange": (C.c_int, [C.c_void_p, C.c_void_p]),
    "se_hip_raycast": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_uint32]),
    "se_hip_image_tile_bytes": (C.c_size_t, [C.c_void_p, C.c_int32]),
    "se_hip_pack_image_tile": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "se_hip_apply_image_tiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "se_hip_gather_images": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "se_hip_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32]),
    "se_hip_download_vertex_normal": (C.c_int, [C.c_void_p, _f32p, _f32p]),
    "se_hip_vertex_normal_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "se_hip_frame_tracked": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint32, C.c_float, C.c_uint32]),
    "se_hip_track": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p]),
    "se_hip_filter_depth": (C.c_int, [C.c_void_p, C.c_int32]),
    "se_hip_download_scaled_depth": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "se_hip_download_track": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    "se_hip_render_volume": (C.c_int, [C.c_void_p, C.c_void_p, _f32p, _f32p, C.c_float, C.c_float, C.c_uint32, C.c_uint32]),
    "se_hip_render_depth": (C.c_int, [C.c_void_p, C.c_void_p]),
    "se_hip_render_track": (C.c_int, [C.c_void_p, C.c_void_p]),
    "se_hip_save_map": (C.c_int, [C.c_void_p, C.c_char_p]),
    "se_hip_load_map": (C.c_int, [C.c_void_p, C.c_char_p]),
    "se_hip_shift_map": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "se_hip_release_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "se_hip_merge_map": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "se_hip_merge_map_rigid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "se_hip_create_replicas": (C.c_int, [C.POINTER(_Config), C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_void_p)]),
    "se_hip_mesh_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "se_hip_mesh_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "se_hip_dump_mesh": (C.c_int, [C.c_void_p, C.c_char_p]),
    "se_hip_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "se_hip_download_blocks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "se_hip_download_nodes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "se_hip_enable_timing": (C.c_int, [C.c_void_p, C.c_int32]),
    "se_hip_get_timings": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int32]),
    "se_hip_enable_stats": (C.c_int, [C.c_void_p, C.c_int32]),
    "se_hip_get_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_int32]),
    "se_hip_query_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(_QueryOut)]),
    "se_hip_query_points_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(_QueryOut)]),
    "se_hip_collide_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(_CollideTest), C.c_int32, C.c_void_p]),
    "se_hip_collide_boxes_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(_CollideTest), C.c_int32, C.c_void_p]),
    "se_hip_collide_motions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(_CollideTest), C.c_int32, C.POINTER(_MotionOut)]),
    "se_hip_collide_motions_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(_CollideTest), C.c_int32, C.POINTER(_MotionOut)]),
    "se_hip_trace_segments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(_CollideTest), C.c_int32, C.POINTER(_TraceOut)]),
    "se_hip_trace_segments_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(_CollideTest), C.c_int32, C.POINTER(_TraceOut)]),
    "se_hip_clearance_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(_CollideTest), C.c_int32, C.POINTER(_ClearanceOut)]),
    "se_hip_clearance_boxes_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(_CollideTest), C.c_int32, C.POINTER(_ClearanceOut)]),
    "se_hip_project_columns": (C.c_int, [C.c_void_p, C.POINTER(_ProjectRequest), C.POINTER(_CollideTest), C.POINTER(_ProjectOut)]),
    "se_hip_project_columns_host": (C.c_int, [C.c_void_p, C.POINTER(_ProjectRequest), C.POINTER(_CollideTest), C.POINTER(_ProjectOut)]),
    "se_hip_distance_field": (C.c_int, [C.c_void_p, C.POINTER(_FieldRequest), C.POINTER(_CollideTest), C.POINTER(_FieldOut)]),
    "se_hip_distance_field_host": (C.c_int, [C.c_void_p, C.POINTER(_FieldRequest), C.POINTER(_CollideTest), C.POINTER(_FieldOut)]),
    "se_hip_reach_field": (C.c_int, [C.c_void_p, C.POINTER(_ReachRequest), C.POINTER(_CollideTest), C.POINTER(_ReachOut)]),
    "se_hip_reach_field_host": (C.c_int, [C.c_void_p, C.POINTER(_ReachRequest), C.POINTER(_CollideTest), C.POINTER(_ReachOut)]),
    "se_hip_collide_oriented": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(_CollideTest), C.c_void_p]),
    "se_hip_collide_oriented_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(_CollideTest), C.c_void_p]),
    "se_hip_collide_oriented_motions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(_CollideTest), C.c_int32, C.POINTER(_OrientedMotionOut)]),
    "se_hip_collide_oriented_motions_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(_CollideTest), C.c_int32, C.POINTER(_OrientedMotionOut)]),
    "se_hip_edit_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(_CollideTest), C.c_int32, C.c_void_p]),
    "se_hip_edit_boxes_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(_CollideTest), C.c_int32, C.c_void_p]),
    "se_hip_allocate_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]),
    "se_hip_allocate_boxes_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]),
    "se_hip_cast_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.POINTER(_RayOut)]),
    "se_hip_cast_rays_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.POINTER(_RayOut)]),
    "se_hip_mesh_blocks": (C.c_int, [C.c_void_p, C.POINTER(_MeshSelect), C.POINTER(_MeshOut)]),
    "se_hip_mesh_blocks_host": (C.c_int, [C.c_void_p, C.POINTER(_MeshSelect), C.POINTER(_MeshOut)]),
}


def _check_rigid(m, what):
    """A 3x4 (or 4x4) float64 transform in voxels: finite, |t| <= 2^20, max |R^T R - I| <= 1e-3, det R > 0 -- what se_hip_merge_map_rigid asks."""
    if not np.isfinite(m).all():
        raise ValueError(f"{what}: a non-finite entry")
    R, t = m[:3, :3], m[:3, 3]
    if (np.abs(t) > 2.0 ** 20).any():
        raise ValueError(f"{what}: a translation component beyond 2^20 voxels")
    if np.abs(R.T @ R - np.eye(3)).max() > 1e-3:
        raise ValueError(f"{what}: not rigid (max |R^T R - I| > 1e-3: no scale, no shear)")
    if not np.linalg.det(R) > 0:
        raise ValueError(f"{what}: a mirror (det R <= 0)")


def rigid_pull(T_dst_src, dim, size) -> np.ndarray:
    """The pull transform of DenseSLAMPipeline.merge_rigid / se_hip_merge_map_rigid, float32 [12] (row-major 3 x 4, voxels), from the
    metric 4x4 pose of the source map's frame in the destination's: x_dst = T_dst_src x_src in metres, voxel = dim / size on both sides.
    Inverted and scaled in float64, rounded once.  Raises TypeError / ValueError for anything that is not a finite rigid pose."""
    T = np.asarray(T_dst_src)
    if T.dtype.kind not in "fiu":
        raise TypeError(f"rigid_pull: T_dst_src must be a 4x4 array of numbers, got dtype {T.dtype}")
    if T.shape != (4, 4):
        raise ValueError(f"rigid_pull: T_dst_src must be 4x4, got {T.shape}")
    T = T.astype(np.float64)
    if not np.isfinite(T).all():
        raise ValueError("rigid_pull: a non-finite entry")
    if not (T[3] == (0, 0, 0, 1)).all():
        raise ValueError("rigid_pull: the last row must be (0, 0, 0, 1)")
    if not (dim > 0 and size > 0):
        raise ValueError("rigid_pull: dim and size must be positive")
    R, t = T[:3, :3], T[:3, 3]
    if np.abs(R.T @ R - np.eye(3)).max() > 1e-3 or not np.linalg.det(R) > 0:
        raise ValueError("rigid_pull: T_dst_src is not rigid (max |R^T R - I| > 1e-3, or a mirror)")
    Ri = np.linalg.inv(R)
    pull = np.concatenate([Ri, (-(Ri @ t) * (float(size) / float(dim)))[:, None]], 1)
    _check_rigid(pull, "rigid_pull")
    return np.ascontiguousarray(pull, np.float32).reshape(12)


def _share_torch_hip_runtime() -> None:
    """One HIP runtime per process.  The PyTorch-ROCm wheel bundles its own libamdhip64.so / libhsa-runtime64.so
    (torch/lib, found through an RPATH), libse_hip.so is linked against /opt/rocm's.  Loaded side by side, the copy that
    initialises second finds the GPU taken ("No HIP GPUs are available" from torch when libse_hip.so ran first).  Both
    copies carry the soname libamdhip64.so.7, so mapping torch's copy by path before libse_hip.so makes the dynamic
    loader resolve both users to that one object, whichever of them touches the GPU first.  No torch installed (or
    already imported: the soname is then mapped): nothing to do."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    for base in (spec.submodule_search_locations or []) if spec else []:
        cand = os.path.join(base, "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
            return


def load_library(rebuild: bool = True):
    """Load libse_hip.so (building it with hipcc first if it is missing or stale)."""
    global _LIB
    if _LIB is None:
        _share_torch_hip_runtime()
        path = _build.LIB
        alt = os.environ.get("SE_HIP_LIB")   # A/B of kernel variants built to another path (tools/)
        if alt:
            import sys
            print(f"supereight_amd: SE_HIP_LIB is set -- loading {alt} instead of the in-tree libse_hip.so (A/B tooling)", file=sys.stderr)
            path, rebuild = alt, False
        if rebuild:
            try:
                path = _build.build()
            except RuntimeError:
                if not os.path.exists(path):
                    raise
        lib = C.CDLL(path)
        for name, (res, args) in EXPORTS.items():
            fn = getattr(lib, name)  # AttributeError if the library does not export the symbol
            fn.restype, fn.argtypes = res, args
        _LIB = lib
    return _LIB


def _colmajor(m) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(m, dtype=np.float32).reshape(4, 4).T).reshape(16)


def _torch_module(obj):
    """torch, if `obj` is a torch tensor (without importing torch for callers that never use it)."""
    import sys
    torch = sys.modules.get("torch")
    return torch if torch is not None and isinstance(obj, torch.Tensor) else None


class DenseSLAMPipeline:
    # (class-level defaults: an object that adopts a handle made by se_hip_create_replicas does not run __init__)
    _k_last = _k_arr = _pyr_arr = None
    _k_addr = 0
    _device = None

    def __init__(self, input_size, volume_resolution: int, volume_dimension: float, init_pose=None,
                 field_type: int = SDF, device: int = 0, max_blocks: int = 0, rows=None, streaming: bool = False):
        self.lib = load_library()
        self.W, self.H = int(input_size[0]), int(input_size[1])
        self.size, self.dim, self.field = int(volume_resolution), float(volume_dimension), field_type
        self._device = int(device)
        rb, re_ = rows if rows is not None else (0, 0)
        cfg = _Config(self.W, self.H, self.size, self.dim, field_type, device, max_blocks, rb, re_)
        h = C.c_void_p()
        self._h = None
        self._check(self.lib.se_hip_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self.pose_ = np.eye(4, dtype=np.float32) if init_pose is None else init_pose
        self._keepalive = None
        self._ring_keepalive = None
        self._pinned = []
        if streaming:
            self.set_streaming(True)

    # pose_ (camera -> world, row-major 4x4) and its column-major copy for the C ABI; assign, do not
    # modify in place
    @property
    def pose_(self):
        if self._pose is None:      # the tracker updated the column-major copy in place (tracking, frame_tracked)
            self._pose = self._pose_cm.reshape(4, 4).T.copy()
        return self._pose

    @pose_.setter
    def pose_(self, m):
        self._pose = np.array(m, dtype=np.float32).reshape(4, 4)
        self._pose_cm = np.ascontiguousarray(self._pose.T).reshape(16)
        self._pose_cm_addr = self._pose_cm.ctypes.data

    @staticmethod
    def _addr(a, dtype, size: int) -> int:
        """Address of a C-contiguous array of `size` elements of `dtype` (checked here: the C ABI takes plain pointers)."""
        if not (type(a) is np.ndarray and a.dtype == dtype and a.size == size and a.flags.c_contiguous):
            raise TypeError(f"expected a C-contiguous {np.dtype(dtype).name}[{size}] array")
        return a.ctypes.data

    def _k(self, k) -> int:
        """Address of the float32[4] intrinsics (fx, fy, cx, cy) for the C ABI.  An int is taken as the address of such an array that the
        caller keeps alive (DenseSLAMPipeline.addr).  A float32[4] array is used in place and its address remembered while the caller
        keeps passing the same object; anything else is converted (and held) on every call."""
        if type(k) is int:
            return k
        if isinstance(k, np.integer):
            return int(k)
        if k is self._k_last:
            return self._k_addr
        if type(k) is np.ndarray and k.dtype == np.float32 and k.size == 4 and k.flags.c_contiguous:
            self._k_last, self._k_arr = k, k
        else:
            self._k_last, self._k_arr = None, np.ascontiguousarray(k, dtype=np.float32).reshape(4)
        self._k_addr = self._k_arr.ctypes.data
        return self._k_addr

    @staticmethod
    def addr(a) -> int:
        """Address of a float32 array for the entry points that accept plain addresses (frame, frame_tracked): check once, call many
        times.  The caller keeps the array alive and unchanged in size."""
        if not (type(a) is np.ndarray and a.dtype == np.float32 and a.flags.c_contiguous):
            raise TypeError("expected a C-contiguous float32 array")
        return a.ctypes.data

    # ------------------------------------------------------------------ plumbing
    def _check(self, status: int) -> int:
        if status < 0:
            raise SeHipError(f"se_hip error {status}: {self.lib.se_hip_last_error().decode()}")
        return status

    def close(self):
        if getattr(self, "_h", None):
            self.lib.se_hip_destroy(self._h)
            self._h = None
            for ptr in getattr(self, "_pinned", []):
                self.lib.se_hip_host_free(ptr)
            self._pinned = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._check(self.lib.se_hip_sync(self._h))

    def clear_overflow(self) -> int:
        """Acknowledge a sticky SE_HIP_E_CAPACITY; returns the pending code (0 none, 1 pool, 2 key list, 3 brick segment)."""
        return self._check(self.lib.se_hip_clear_overflow(self._h))

    def set_stream(self, hip_stream_ptr: int):
        self._check(self.lib.se_hip_set_stream(self._h, C.c_void_p(hip_stream_ptr)))

    def scan_overlaps(self) -> bool:
        return bool(self._check(self.lib.se_hip_scan_overlaps(self._h)))

    def frame_is_fused(self) -> bool:
        """True if frame() runs the one-queue streaming schedule (deferred raycast + next frame's scan in one launch, include/se_hip.h)."""
        return bool(self._check(self.lib.se_hip_frame_is_fused(self._h)))

    def set_streaming(self, on: bool = True) -> bool:
        """Opt into the one-queue streaming schedule (se_hip_set_streaming): frame() / raycasting_deferred() hold a frame's raycast back until the
        next frame's allocation scan.  Returns True if this handle will actually fuse."""
        return bool(self._check(self.lib.se_hip_set_streaming(self._h, int(on))))

    def set_image_ring(self, ptr: int, slots: int, keepalive=None):
        """vertex_ / normal_ of frame f go to slot f % slots of a caller-owned device ring (se_hip_set_image_ring); ptr = 0 restores the own images."""
        self._check(self.lib.se_hip_set_image_ring(self._h, C.c_void_p(ptr), slots))
        self._ring_keepalive = keepalive

    def launch_counts(self, reset: bool = False) -> dict:
        """Kernel launches per kind since the last reset, counted at enqueue time (does not flush a deferred raycast); 'pending' = a raycast is held back."""
        n = (C.c_int64 * (len(KERNELS) + 1))()
        pend = self._check(self.lib.se_hip_get_launch_counts(self._h, n, int(reset)))
        out = {k: int(n[i]) for i, k in enumerate(KERNELS)}
        out["fused"] = int(n[len(KERNELS)])
        out["pending"] = bool(pend)
        return out

    def set_scan_stream(self, hip_stream_ptr: int):
        self._check(self.lib.se_hip_set_scan_stream(self._h, C.c_void_p(hip_stream_ptr)))

    # ------------------------------------------------------------------ reference-shaped API
    def setPose(self, pose):
        """DenseSLAMSystem::setPose semantics minus the init-pose offset: pose is camera->world."""
        self.pose_ = pose

    def getPose(self):
        return self.pose_.copy()

    def set_depth(self, depth_m):
        """float_depth_ of the reference: host float32 metres (H, W)."""
        d = np.ascontiguousarray(depth_m, dtype=np.float32).reshape(-1)
        assert d.size == self.W * self.H
        self._check(self.lib.se_hip_upload_depth(self._h, d))

    def set_depth_mm(self, depth_mm):
        """preprocessing()'s mm2metersKernel fused into the upload: uint16 millimetres (h, w)."""
        d = np.ascontiguousarray(depth_mm, dtype=np.uint16)
        self._check(self.lib.se_hip_upload_depth_mm(self._h, d.reshape(-1), d.shape[1], d.shape[0]))

    def set_depth_device(self, ptr: int, keepalive=None):
        """Zero-copy: a float32 depth image already in HBM (e.g. a torch tensor's data_ptr())."""
        self._keepalive = keepalive
        self._check(self.lib.se_hip_set_depth_device(self._h, C.c_void_p(ptr)))

    def integration(self, k, integration_rate: int, mu: float, frame: int) -> bool:
        return bool(self._check(self.lib.se_hip_integrate(self._h, self._pose_cm_addr, self._k(k),
                                                          integration_rate, mu, frame)))

    def frame(self, depth_ptr: int, pose_cm, k, mu: float, frame: int, integration_rate: int = 1) -> int:
        """One frame in one FFI call: device depth pointer + integration() + raycasting().  pose_cm = the camera->world pose as
        16 float32 in column-major order (to_colmajor(pose)) or the address of such an array (DenseSLAMPipeline.addr: checked once by
        the caller, who keeps it alive -- the closed loop's per-frame Python cost is what the host adds to the frame); k likewise.
        Returns bit 0 = integrated, bit 1 = raycast."""
        if type(pose_cm) is not int:
            pose_cm = int(pose_cm) if isinstance(pose_cm, np.integer) else self._addr(pose_cm, np.float32, 16)
        return self._check(self.lib.se_hip_frame(self._h, depth_ptr, pose_cm, self._k(k), integration_rate, mu, frame))

    def raycasting(self, k, mu: float, frame: int) -> bool:
        return bool(self._check(self.lib.se_hip_raycast(self._h, self._pose_cm_addr, self._k(k), mu, frame)))

    def raycasting_deferred(self, k, mu: float, frame: int) -> bool:
        """raycasting() of a streaming caller: on a handle that fuses, launched together with the next integration()'s allocation scan."""
        return bool(self._check(self.lib.se_hip_raycast_deferred(self._h, self._pose_cm_addr, self._k(k), mu, frame)))

    def mesh(self) -> np.ndarray:
        """Marching-cubes triangles of the map, (n, 3, 3) float32 vertices in metres (order unspecified)."""
        n = C.c_int64()
        self._check(self.lib.se_hip_mesh_count(self._h, C.byref(n)))
        out = np.empty((n.value, 3, 3), np.float32)
        if n.value:
            w = C.c_int64()
            self._check(self.lib.se_hip_mesh_download(self._h, out.ctypes.data, n.value, C.byref(w)))
            out = out[: w.value]
        return out

    def dump_mesh(self, filename: str):
        """DenseSLAMSystem::dump_mesh: VTK polydata file."""
        self._check(self.lib.se_hip_dump_mesh(self._h, filename.encode()))

    def filter_depth(self, on: bool = True):
        """preprocessing(..., filterInput): tracking works on the bilateral-filtered depth image."""
        self._check(self.lib.se_hip_filter_depth(self._h, int(on)))

    def scaled_depth(self, level: int = 0) -> np.ndarray:
        out = np.empty((self.H >> level, self.W >> level), np.float32)
        self._check(self.lib.se_hip_download_scaled_depth(self._h, level, out.ctypes.data))
        return out

    TRACK_DTYPE = np.dtype([("result", np.int32), ("error", np.float32), ("J", np.float32, 6)])

    _PYRAMID = np.asarray((10, 5, 4), np.int32)
    _PYRAMID_ADDR = _PYRAMID.ctypes.data

    def _pyr(self, pyramid):
        if pyramid is None or pyramid is self._PYRAMID or tuple(pyramid) == (10, 5, 4):
            return self._PYRAMID_ADDR, 3
        self._pyr_arr = np.ascontiguousarray(pyramid, dtype=np.int32).reshape(-1)
        return self._pyr_arr.ctypes.data, self._pyr_arr.size

    def tracking(self, k, icp_threshold: float, tracking_rate: int, frame: int, pyramid=None) -> bool:
        """DenseSLAMSystem::tracking: ICP of the current depth image against the last raycast; updates pose_.
        pyramid = iterations per level, finest first (default (10, 5, 4))."""
        pa, n = self._pyr(pyramid)
        r = self._check(self.lib.se_hip_track(self._h, self._k(k), icp_threshold, tracking_rate, frame, pa, n, self._pose_cm_addr))
        self._pose = None      # (the column-major copy was updated in place; restored by the library if the check failed)
        return bool(r)

    def frame_tracked(self, depth_ptr: int, k, mu: float, frame: int, icp_threshold: float = 1e-5, tracking_rate: int = 1,
                      integration_rate: int = 1, pyramid=None) -> int:
        """One frame of the reference's loop with tracking on (se_apps/src/benchmark.cpp:115-150) in one FFI call: device depth
        pointer, tracked = tracking(); if tracked or frame <= 3: integration(); raycasting().  pose_ is updated.  Returns bit 0 =
        integrated, bit 1 = raycast, bit 2 = tracked."""
        pa, n = self._pyr(pyramid)
        r = self._check(self.lib.se_hip_frame_tracked(self._h, depth_ptr, self._k(k), icp_threshold, tracking_rate, pa, n,
                                                      self._pose_cm_addr, integration_rate, mu, frame))
        self._pose = None
        return r

    def track_data(self):
        t = np.zeros(self.W * self.H, self.TRACK_DTYPE)
        red = np.zeros(32, np.float32)
        it = C.c_int32()
        self._check(self.lib.se_hip_download_track(self._h, t.ctypes.data, red.ctypes.data, C.byref(it)))
        return t.reshape(self.H, self.W), red, it.value

    # the render*() methods (DenseSLAMSystem.h:241-286): RGBW uint8 images
    def renderVolume(self, view_pose, k, mu, largestep, frame=0, rate=1):
        out = np.zeros((self.H, self.W, 4), np.uint8)
        ran = self._check(self.lib.se_hip_render_volume(self._h, out.ctypes.data, _colmajor(view_pose), np.asarray(k, np.float32), mu, largestep, frame, rate))
        return out if ran else None

    def renderDepth(self):
        out = np.zeros((self.H, self.W, 4), np.uint8)
        self._check(self.lib.se_hip_render_depth(self._h, out.ctypes.data))
        return out

    def renderTrack(self):
        out = np.zeros((self.H, self.W, 4), np.uint8)
        self._check(self.lib.se_hip_render_track(self._h, out.ctypes.data))
        return out

    # stage split used by the multi-GPU driver
    def alloc_scan(self, k, integration_rate: int, mu: float, frame: int) -> bool:
        return bool(self._check(self.lib.se_hip_alloc_scan(self._h, self._pose_cm_addr, self._k(k),
                                                           integration_rate, mu, frame)))

    def new_keys_device(self):
        ptr, cap = C.c_void_p(), C.c_int64()
        self._check(self.lib.se_hip_new_keys_device(self._h, C.byref(ptr), C.byref(cap)))
        return ptr.value, cap.value

    def set_new_keys_buffer(self, ptr: int, capacity_words: int, keepalive=None):
        self._keys_keepalive = keepalive
        self._check(self.lib.se_hip_set_new_keys_buffer(self._h, C.c_void_p(ptr), capacity_words))

    def alloc_commit(self, lists_ptr: int, nlists: int, stride_words: int):
        self._check(self.lib.se_hip_alloc_commit(self._h, C.c_void_p(lists_ptr), nlists, stride_words))

    def set_exchange(self, nccl_comm: int, nccl_all_gather: int, world: int):
        self._check(self.lib.se_hip_set_exchange(self._h, C.c_void_p(nccl_comm), C.c_void_p(nccl_all_gather), world))

    def alloc_exchange(self, recv_ptr: int, words: int):
        self._check(self.lib.se_hip_alloc_exchange(self._h, C.c_void_p(recv_ptr), words))

    def sweep_shard_bytes(self, cap_bricks: int) -> int:
        return int(self.lib.se_hip_sweep_shard_bytes(cap_bricks))

    def set_sweep_shard(self, rank: int, world: int, send_ptr: int, cap_bricks: int, keepalive=None):
        """Sharded sweep (SURVEY 8e option 4): this replica integrates the blocks it owns and packs them into `send_ptr`."""
        self._check(self.lib.se_hip_set_sweep_shard(self._h, rank, world, C.c_void_p(send_ptr), cap_bricks))
        self._shard_keepalive = keepalive

    def apply_bricks(self, recv_ptr: int, world: int):
        self._check(self.lib.se_hip_apply_bricks(self._h, C.c_void_p(recv_ptr), world))

    def brick_exchange(self, recv_ptr: int):
        self._check(self.lib.se_hip_brick_exchange(self._h, C.c_void_p(recv_ptr)))

    def integrate_sweep(self, k, integration_rate: int, mu: float, frame: int) -> bool:
        return bool(self._check(self.lib.se_hip_integrate_sweep(self._h, self._pose_cm_addr, self._k(k),
                                                                integration_rate, mu, frame)))

    # ------------------------------------------------------------------ outputs
    def vertex_normal(self):
        v = np.zeros((self.H, self.W, 3), np.float32)
        n = np.zeros((self.H, self.W, 3), np.float32)
        self._check(self.lib.se_hip_download_vertex_normal(self._h, v.reshape(-1), n.reshape(-1)))
        return v, n

    def vertex_normal_device(self):
        v, n = C.c_void_p(), C.c_void_p()
        self._check(self.lib.se_hip_vertex_normal_device(self._h, C.byref(v), C.byref(n)))
        return v.value, n.value

    def set_pinned_input(self, on: bool = True):
        """Opt in to zero-copy host input: page-locked images handed to set_depth / set_depth_mm (pinned_image below) are read in place."""
        self._check(self.lib.se_hip_set_pinned_input(self._h, 1 if on else 0))

    def pinned_image(self, dtype=np.float32, shape=None):
        """A page-locked numpy image of the computation size (se_hip_host_alloc); freed with the pipeline."""
        shape = shape or (self.H, self.W)
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        ptr = self.lib.se_hip_host_alloc(nbytes)
        if not ptr:
            raise MemoryError("se_hip_host_alloc failed")
        self._pinned.append(ptr)
        return np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(ptr)).view(dtype).reshape(shape)

    def memory_info(self) -> dict:
        """Layout and device memory of the map: dense brick grid or pooled bricks, brick slots, bytes of the bricks / of the whole replica."""
        out = (C.c_int64 * 4)()
        self._check(self.lib.se_hip_memory_info(self._h, out))
        return {"layout": "dense brick grid" if out[0] else "pooled bricks", "brick_slots": int(out[1]), "brick_bytes": int(out[2]), "device_bytes": int(out[3])}

    def counts(self):
        nb, nn = C.c_int32(), C.c_int32()
        self._check(self.lib.se_hip_counts(self._h, C.byref(nb), C.byref(nn)))
        return nb.value, nn.value

    def blocks(self):
        nb, _ = self.counts()
        coords = np.zeros((nb, 3), np.int32)
        x = np.zeros((nb, 512), np.float32)
        y = np.zeros((nb, 512), np.float32)
        act = np.zeros(nb, np.uint8)
        if nb:
            self._check(self.lib.se_hip_download_blocks(self._h, coords.ctypes.data, x.ctypes.data, y.ctypes.data, act.ctypes.data))
        return coords, x, y, act

    # ---- full vertex_ / normal_ images on every rank of a row-sharded run (include/se_hip.h)
    def image_tile_bytes(self, max_rows: int) -> int:
        return int(self.lib.se_hip_image_tile_bytes(self._h, max_rows))

    def pack_image_tile(self, send_ptr: int, max_rows: int):
        self._check(self.lib.se_hip_pack_image_tile(self._h, C.c_void_p(send_ptr), max_rows))

    def apply_image_tiles(self, recv_ptr: int, parts, max_rows: int):
        b = np.ascontiguousarray([q[0] for q in parts], np.int32)
        e = np.ascontiguousarray([q[1] for q in parts], np.int32)
        self._check(self.lib.se_hip_apply_image_tiles(self._h, C.c_void_p(recv_ptr), len(parts), max_rows, b.ctypes.data, e.ctypes.data))

    def gather_images(self, send_ptr: int, recv_ptr: int, parts, max_rows: int):
        b = np.ascontiguousarray([q[0] for q in parts], np.int32)
        e = np.ascontiguousarray([q[1] for q in parts], np.int32)
        self._check(self.lib.se_hip_gather_images(self._h, C.c_void_p(send_ptr), C.c_void_p(recv_ptr), max_rows, b.ctypes.data, e.ctypes.data))

    def block_flags(self):
        """coords[n,3] and VoxelBlock::active_[n] of the allocated blocks (sorted by key) without the voxel planes."""
        nb, _ = self.counts()
        coords = np.zeros((nb, 3), np.int32)
        act = np.zeros(nb, np.uint8)
        if nb:
            self._check(self.lib.se_hip_download_blocks(self._h, coords.ctypes.data, None, None, act.ctypes.data))
        return coords, act

    def nodes(self):
        _, nn = self.counts()
        code = np.zeros(nn, np.uint64)
        side = np.zeros(nn, np.uint32)
        x = np.zeros((nn, 8), np.float32)
        y = np.zeros((nn, 8), np.float32)
        self._check(self.lib.se_hip_download_nodes(self._h, code.ctypes.data, side.ctypes.data, x.ctypes.data, y.ctypes.data))
        return code, side, x, y

    # ------------------------------------------------------------------ batched queries: what query, collides and cast_rays share
    def _batch_input(self, who, name, a, dtype, cols, contiguous=True):
        """The rule for an [N, cols] input of the batched queries: a numpy array of `dtype` (host entry) or a torch tensor of that dtype on
        this handle's GPU (device entry).  Returns (torch or None, the array or tensor, N); anything else raises before any library call.
        contiguous: a numpy array is made contiguous, a torch tensor has to be (False: the caller packs the rows itself)."""
        dt = np.dtype(dtype)
        is_numpy = type(a) is np.ndarray
        torch = None if is_numpy else _torch_module(a)
        if not is_numpy and torch is None:
            raise TypeError(f"{who}: {name} must be a numpy {dt.name} array or a torch tensor on the GPU, got {type(a).__name__}")
        if a.dtype != (dt if torch is None else getattr(torch, dt.name)):
            raise TypeError(f"{who}: {name} must be {dt.name}, got {a.dtype}")
        if a.ndim != 2 or a.shape[1] != cols:
            raise ValueError(f"{who}: {name} must have shape [N, {cols}], got {list(a.shape)}")
        if torch is None:
            return None, np.ascontiguousarray(a) if contiguous else a, a.shape[0]
        if contiguous and not a.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous")
        if a.device.type != "cuda" or (self._device is not None and a.device.index != self._device):
            raise ValueError(f"{who}: {name} must be on this handle's GPU (cuda:{self._device}), got {a.device}")
        return torch, a, int(a.shape[0])

    def _own_device(self, device: bool):
        """(torch, this handle's GPU as a torch device) for the entries that take `device=True` instead of a tensor; (None, None) for the host."""
        if not device:
            return None, None
        import torch
        return torch, torch.device("cuda", self._device if self._device is not None else torch.cuda.current_device())

    @staticmethod
    def _batch_outputs(torch, device, lead, table, want, struct, *tail):
        """The outputs asked for (`want`) of a (name, shape per item, numpy dtype) table, each of shape `lead` + its shape per item, as numpy
        arrays or as torch tensors on `device`, and the ctypes `struct` of their addresses (NULL where not asked for; `tail`: what the struct
        holds behind them)."""
        if torch is None:
            res = {k: np.empty(lead + shp, dt) for k, shp, dt in table if want[k]}
            return res, struct(*(res[k].ctypes.data if k in res else None for k, _, _ in table), *tail)
        res = {k: torch.empty(lead + shp, dtype=getattr(torch, np.dtype(dt).name), device=device) for k, shp, dt in table if want[k]}
        return res, struct(*(res[k].data_ptr() if k in res else None for k, _, _ in table), *tail)

    @staticmethod
    def _ptr(torch, a, n=1):
        """The address of a numpy array or a torch tensor for the C ABI; NULL for an empty batch (n == 0) and for None."""
        if a is None or not n:
            return None
        return a.ctypes.data if torch is None else a.data_ptr()

    def _call(self, torch, device, entry, *args):
        """The host / device fork of every batched entry.  Without torch: `entry`_host on numpy arrays (it synchronises itself).  With torch:
        `entry` on tensors -- the caller's current torch stream on `device` is synchronised first (the inputs must be complete when the
        handle's stream reads them), and the handle before the outputs are handed back."""
        if torch is None:
            self._check(getattr(self.lib, entry + "_host")(self._h, *args))
            return
        torch.cuda.current_stream(device).synchronize()
        self._check(getattr(self.lib, entry)(self._h, *args))
        self.sync()

    def _occupancy_test(self, who, threshold, occupied_above, records=False) -> _CollideTest:
        """se_hip_collide_test from threshold / occupied_above: occupied_above None defaults by field (False for SDF, True for OFusion), else
        it has to be a bool (TypeError); the threshold has to be finite as a float32 (ValueError).  records: the ready-made test of
        edit_records -- no default, and the threshold is left to the library."""
        if occupied_above is None and not records:
            occupied_above = self.field == OFUSION
        if not isinstance(occupied_above, (bool, np.bool_)):
            raise TypeError(f"{who}: occupied_above must be a bool, got {type(occupied_above).__name__}")
        thr = float(threshold)
        if not records and not np.isfinite(np.float32(thr)):
            raise ValueError(f"{who}: threshold must be finite as a float32, got {threshold!r}")
        return _CollideTest(thr, int(bool(occupied_above)))

    @staticmethod
    def _stop_at(who, stop_at) -> int:
        """The status code that stop_at names ("occupied" / "unseen"), ValueError for anything else."""
        if stop_at not in _MOTION_STOPS:
            raise ValueError(f"{who}: stop_at must be one of {sorted(_MOTION_STOPS)}, got {stop_at!r}")
        return _MOTION_STOPS[stop_at]

    @staticmethod
    def _ints(who, name, v, shape=None) -> np.ndarray:
        """`v` as an array that must hold integers (a bool is refused: TypeError) and, where given, have `shape` (ValueError)."""
        a = np.asarray(v)
        if isinstance(v, (bool, np.bool_)) or a.dtype.kind not in "iu":
            raise TypeError(f"{who}: {name} must hold integers, got {a.dtype}")
        if shape is not None and a.shape != tuple(shape):
            raise ValueError(f"{who}: {name} must have shape {list(shape)}, got {list(a.shape)}")
        return a

    @staticmethod
    def _region(who, lo, side, robot, noun, r_max=None):
        """The region rule of distance_field and reach_field on three Python ints each: side >= 1, robot in 1 .. 256, r_max (where the entry
        has one) in 0 .. 255, lo and lo + side + robot within +-2^19, at most 2^24 `noun`; ValueError otherwise."""
        if min(side) < 1 or min(robot) < 1 or max(robot) > FIELD_ROBOT_MAX:
            raise ValueError(f"{who}: side must be >= 1 and robot in 1 .. {FIELD_ROBOT_MAX}, got {side}, {robot}")
        if r_max is not None and not 0 <= r_max <= FIELD_R_MAX:
            raise ValueError(f"{who}: r_max must lie in 0 .. {FIELD_R_MAX}, got {r_max}")
        if any(abs(v) > FIELD_LIMIT for k in range(3) for v in (lo[k], lo[k] + side[k] + robot[k])):
            raise ValueError(f"{who}: lo and lo + side + robot must lie within +-2^19")
        if side[0] * side[1] * side[2] > FIELD_MAX_VOXELS:
            raise ValueError(f"{who}: {side[0] * side[1] * side[2]} {noun}, more than 2^24")

    # (shape of each output per point, dtype)
    _QUERY_OUTPUTS = (("fine", (2,), np.float32), ("coarse", (2,), np.float32), ("interp", (), np.float32), ("grad", (3,), np.float32),
                      ("status", (), np.uint8))

    def query(self, points, fine: bool = True, coarse: bool = False, interp: bool = True, grad: bool = True, status: bool = True) -> dict:
        """Batched map queries (se_hip_query_points, include/se_hip.h): for each point in metres, the reference's VolumeTemplate::get
        (fine: (x, y) of the voxel, initValue() where no block), operator[] (coarse: (x, y), the deepest existing node's value where no
        block), interp(p, x), grad(p, x), and status bits (1 in the volume, 2 block allocated, 4 interp reads allocated blocks only).
        Returns a dict of the outputs asked for.
          - numpy float32 [N, 3]: through the host entry; numpy arrays out.
          - a torch tensor on this handle's GPU (float32, contiguous, [N, 3]): through the device entry; outputs are torch tensors on the same
            device.  The caller's current torch stream is synchronised first (the points must be complete when the handle's stream reads
            them), and the handle is synchronised before the tensors are returned.
        Anything else raises TypeError / ValueError before any library call."""
        want = {"fine": fine, "coarse": coarse, "interp": interp, "grad": grad, "status": status}
        if not any(want.values()):
            raise ValueError("query: no output requested")
        torch, pts, n = self._batch_input("query", "points", points, np.float32, 3)
        dev = pts.device if torch else None
        res, out = self._batch_outputs(torch, dev, (n,), self._QUERY_OUTPUTS, want, _QueryOut)
        self._call(torch, dev, "se_hip_query_points", self._ptr(torch, pts, n), n, C.byref(out))
        return res

    def collides(self, boxes, threshold: float = 0.0, occupied_above=None, mode: str = "strict"):
        """Batched collision queries for axis-aligned boxes (se_hip_collide_boxes, include/se_hip.h): boxes [N, 6] int32 = lo xyz, side xyz
        in voxels.  Returns one status per box: COLLISION_OCCUPIED (0), COLLISION_UNSEEN (1), COLLISION_EMPTY (2), COLLISION_INVALID (255).
        A voxel is unseen where it equals initValue(), else occupied where x > threshold (occupied_above) or x < threshold, else empty;
        occupied_above defaults by field: False for SDF, True for OFusion.  mode "strict": the min over the voxels of [lo, lo + side)
        (outside the volume counts as unseen); "reference": exactly what the reference's se::geometry::collides_with returns.
          - numpy int32 [N, 6]: through the host entry; a numpy uint8 array out.
          - a torch int32 tensor on this handle's GPU (contiguous, [N, 6]): through the device entry; a torch uint8 tensor on the same
            device out.  The caller's current torch stream is synchronised first, and the handle before the tensor is returned.
        Anything else raises TypeError / ValueError before any library call."""
        if mode not in _COLLIDE_MODES:
            raise ValueError(f"collides: mode must be one of {sorted(_COLLIDE_MODES)}, got {mode!r}")
        test = self._occupancy_test("collides", threshold, occupied_above)
        torch, b, n = self._batch_input("collides", "boxes", boxes, np.int32, 6)
        dev = b.device if torch else None
        out = np.empty(n, np.uint8) if torch is None else torch.empty(n, dtype=torch.uint8, device=dev)
        self._call(torch, dev, "se_hip_collide_boxes", self._ptr(torch, b, n), n, C.byref(test), _COLLIDE_MODES[mode], self._ptr(torch, out, n))
        return out

    _MOTION_OUTPUTS = (("status", (), np.uint8), ("t_first", (), np.float32))

    def collides_moving(self, motions, threshold: float = 0.0, occupied_above=None, stop_at: str = "occupied", t_first: bool = True):
        """Batched collision queries for boxes moved along straight segments (se_hip_collide_motions, include/se_hip.h): motions [N, 9] int32 =
        lo xyz, side xyz, d xyz in voxels; the box [lo, lo + side) is translated by t * d, t in [0, 1].  Exact for the continuous motion: a
        voxel counts iff the moving box touches it (open inequalities), and is classified as collides() classifies it in strict mode
        (threshold / occupied_above as there; outside the volume is unseen).  Returns the status per motion -- the min class over the touched
        voxels, COLLISION_INVALID for side < 1 or coordinates beyond +-2^20 -- or, with t_first, (status, t_first): the parameter at which the
        motion first touches a voxel that blocks (stop_at "occupied": occupied voxels; "unseen": unseen ones too), 0 when it is blocked at its
        start, MOTION_FREE (2.0) when nothing blocks, -1 for an invalid motion.
          - numpy int32 [N, 9]: through the host entry; numpy arrays out.
          - a torch int32 tensor on this handle's GPU (contiguous, [N, 9]): through the device entry; torch tensors on the same device out.
            The caller's current torch stream is synchronised first, and the handle before the tensors are returned.
        Anything else raises TypeError / ValueError before any library call."""
        stop = self._stop_at("collides_moving", stop_at)
        test = self._occupancy_test("collides_moving", threshold, occupied_above)
        torch, mo, n = self._batch_input("collides_moving", "motions", motions, np.int32, 9)
        dev = mo.device if torch else None
        res, out = self._batch_outputs(torch, dev, (n,), self._MOTION_OUTPUTS, {"status": True, "t_first": bool(t_first)}, _MotionOut)
        self._call(torch, dev, "se_hip_collide_motions", self._ptr(torch, mo, n), n, C.byref(test), stop, C.byref(out))
        return (res["status"], res["t_first"]) if t_first else res["status"]

    _TRACE_OUTPUTS = (("status", (), np.uint8), ("t_first", (), np.float32), ("first", (3,), np.int32), ("counts", (2,), np.int32))

    def trace(self, segments, threshold: float = 0.0, occupied_above=None, stop_at: str = "occupied", t_first: bool = True, first: bool = True,
              counts: bool = True) -> dict:
        """Exact segment traces (se_hip_trace_segments, include/se_hip.h): segments [N, 6] int32 = a xyz, b xyz in sub-units of
        1 / ORIENTED_SUB voxel (segments_from_points() and view_segments() make them from metric ones).  The voxels a segment touches (open
        inequalities, exact) are visited in the order it touches them and classified as collides() classifies them in strict mode (threshold /
        occupied_above as there; outside the volume is unseen), up to the first that blocks (stop_at "occupied": occupied voxels; "unseen":
        unseen ones too).  Returns a dict of the outputs asked for:
          status   uint8 [N]: the min class up to and including the blocking voxel, COLLISION_EMPTY where nothing is touched,
                   COLLISION_INVALID for a coordinate beyond +-2^22;
          t_first  float32 [N]: the parameter at which the blocking voxel is entered, MOTION_FREE (2.0) when nothing blocks, -1 when invalid;
          first    int32 [N, 3]: that voxel (x y z), TRACE_NONE where there is none;
          counts   int32 [N, 2]: the unseen and the empty voxels inside the volume before it, (-1, -1) when invalid.  With stop_at "occupied"
                   counts[:, 0] is the information gain of the ray; without counts the call skips absent octants in one jump each.
          - numpy int32 [N, 6]: through the host entry; numpy arrays out.
          - a torch int32 tensor on this handle's GPU (contiguous, [N, 6]): through the device entry; torch tensors on the same device out.
            The caller's current torch stream is synchronised first, and the handle before the tensors are returned.
        Anything else raises TypeError / ValueError before any library call."""
        stop = self._stop_at("trace", stop_at)
        test = self._occupancy_test("trace", threshold, occupied_above)
        torch, sg, n = self._batch_input("trace", "segments", segments, np.int32, 6)
        dev = sg.device if torch else None
        want = {"status": True, "t_first": bool(t_first), "first": bool(first), "counts": bool(counts)}
        res, out = self._batch_outputs(torch, dev, (n,), self._TRACE_OUTPUTS, want, _TraceOut)
        self._call(torch, dev, "se_hip_trace_segments", self._ptr(torch, sg, n), n, C.byref(test), stop, C.byref(out))
        return res

    def view_gain(self, poses, k, width, height, stride: int = 8, near: float = 0.4, far: float = 4.0, threshold: float = 0.0, occupied_above=None,
                  device: bool = False):
        """Next-best-view scores of candidate camera poses [V, 4, 4] (camera to world, metres) with intrinsics k = (fx, fy, cx, cy): the fan of
        view_segments() per pose, traced with stop_at "occupied" in ONE trace() call for all views.  Returns int64 [V, 4] per view: the unseen
        voxels its rays look into before anything occupied (the information gain), the empty voxels they cross, the rays that ended on an
        occupied voxel, and the rays traced (those that meet the volume).  device: upload the segments and take the sums on this handle's GPU
        (a torch tensor out), else through the host entry (a numpy array out)."""
        T = np.asarray(poses, np.float64)
        if T.ndim != 3 or T.shape[1:] != (4, 4):
            raise ValueError(f"view_gain: poses must have shape [V, 4, 4], got {list(T.shape)}")
        if not isinstance(device, (bool, np.bool_)):
            raise TypeError(f"view_gain: device must be a bool, got {type(device).__name__}")
        self._occupancy_test("view_gain", threshold, occupied_above)
        fans = [view_segments(t, k, width, height, stride, near, far, self.dim, self.size)[0] for t in T]
        nv = len(fans)
        seg = np.ascontiguousarray(np.concatenate(fans)) if nv else np.zeros((0, 6), np.int32)
        view = np.repeat(np.arange(nv), [len(f) for f in fans])
        torch, dev = self._own_device(bool(device))
        if torch is None:
            r = self.trace(seg, threshold, occupied_above, "occupied", t_first=False, first=False)
            cols = np.stack([r["counts"][:, 0], r["counts"][:, 1], r["status"] == COLLISION_OCCUPIED, np.ones(len(seg), np.int64)], 1).astype(np.int64)
            out = np.zeros((nv, 4), np.int64)
            np.add.at(out, view, cols)
            return out
        r = self.trace(torch.from_numpy(seg).to(dev), threshold, occupied_above, "occupied", t_first=False, first=False)
        cols = torch.stack([r["counts"][:, 0].long(), r["counts"][:, 1].long(), (r["status"] == COLLISION_OCCUPIED).long(),
                            torch.ones(len(seg), dtype=torch.int64, device=dev)], 1)
        return torch.zeros((nv, 4), dtype=torch.int64, device=dev).index_add_(0, torch.from_numpy(view).to(dev), cols)

    def collides_oriented(self, boxes, threshold: float = 0.0, occupied_above=None):
        """Batched collision queries for oriented boxes (se_hip_collide_oriented, include/se_hip.h): boxes [N, 12] int32 = centre xyz, then the
        half-axes h0, h1, h2 xyz, in sub-units of 1 / ORIENTED_SUB voxel (oriented_boxes() makes them from metric ones).  The box is the open set
        {c + s0 h0 + s1 h1 + s2 h2 : |s_i| < 1}; the half-axes need not be orthogonal.  Exact: a voxel counts iff the box touches it (an integer
        separating-axis test, open inequalities), and is classified as collides() classifies it in strict mode (threshold / occupied_above as
        there; outside the volume is unseen).  Returns one status per box: the min class over the touched voxels, COLLISION_INVALID for
        det(h0, h1, h2) == 0, |c_k| > 2^20 or |h_ik| > 2^14.
          - numpy int32 [N, 12]: through the host entry; a numpy uint8 array out.
          - a torch int32 tensor on this handle's GPU (contiguous, [N, 12]): through the device entry; a torch uint8 tensor on the same
            device out.  The caller's current torch stream is synchronised first, and the handle before the tensor is returned.
        Anything else raises TypeError / ValueError before any library call."""
        test = self._occupancy_test("collides_oriented", threshold, occupied_above)
        torch, b, n = self._batch_input("collides_oriented", "boxes", boxes, np.int32, 12)
        dev = b.device if torch else None
        out = np.empty(n, np.uint8) if torch is None else torch.empty(n, dtype=torch.uint8, device=dev)
        self._call(torch, dev, "se_hip_collide_oriented", self._ptr(torch, b, n), n, C.byref(test), self._ptr(torch, out, n))
        return out

    _ORIENTED_MOTION_OUTPUTS = (("status", (), np.uint8), ("t_first", (), np.float32), ("t_exact", (2,), np.int64))

    def collides_oriented_moving(self, motions, threshold: float = 0.0, occupied_above=None, stop_at: str = "occupied", t_first: bool = True,
                                 exact: bool = False):
        """Batched collision queries for oriented boxes moved along straight segments (se_hip_collide_oriented_motions, include/se_hip.h):
        motions [N, 15] int32 = centre xyz, the half-axes h0, h1, h2 xyz, the displacement d xyz, in sub-units of 1 / ORIENTED_SUB voxel
        (oriented_motions() makes them from metric ones).  The box of collides_oriented() is translated by t * d, t in [0, 1], without turning.
        Exact for the continuous motion: a voxel counts iff the moving box touches it (open inequalities, integer arithmetic), and is classified
        as collides() classifies it in strict mode (threshold / occupied_above as there; outside the volume is unseen).  Returns the status per
        motion -- the min class over the touched voxels, COLLISION_INVALID for an invalid box, |d_k| > 2^18 or |c_k + d_k| > 2^20 -- or, with
        t_first, (status, t_first): the parameter at which the motion first touches a voxel that blocks (stop_at "occupied": occupied voxels;
        "unseen": unseen ones too), 0 when it is blocked at its start, MOTION_FREE (2.0) when nothing blocks, -1 for an invalid motion; with
        exact, the int64 [N, 2] reduced fractions num / den of that parameter come last ((2, 1) free, (-1, 1) invalid).
          - numpy int32 [N, 15]: through the host entry; numpy arrays out.
          - a torch int32 tensor on this handle's GPU (contiguous, [N, 15]): through the device entry; torch tensors on the same device out.
            The caller's current torch stream is synchronised first, and the handle before the tensors are returned.
        Anything else raises TypeError / ValueError before any library call."""
        stop = self._stop_at("collides_oriented_moving", stop_at)
        test = self._occupancy_test("collides_oriented_moving", threshold, occupied_above)
        torch, mo, n = self._batch_input("collides_oriented_moving", "motions", motions, np.int32, 15)
        dev = mo.device if torch else None
        want = {"status": True, "t_first": bool(t_first), "t_exact": bool(exact)}
        res, out = self._batch_outputs(torch, dev, (n,), self._ORIENTED_MOTION_OUTPUTS, want, _OrientedMotionOut)
        self._call(torch, dev, "se_hip_collide_oriented_motions", self._ptr(torch, mo, n), n, C.byref(test), stop, C.byref(out))
        got = [res["status"]] + ([res["t_first"]] if t_first else []) + ([res["t_exact"]] if exact else [])
        return got[0] if len(got) == 1 else tuple(got)

    _CLEARANCE_OUTPUTS = (("d2", (), np.int32), ("nearest", (3,), np.int32))

    def clearance(self, boxes, r_max, threshold: float = 0.0, occupied_above=None, stop_at: str = "occupied", nearest: bool = True):
        """Batched clearance queries (se_hip_clearance_boxes, include/se_hip.h): boxes [N, 6] int32 = lo xyz, side xyz in voxels; r_max the
        search radius in voxels, an integer or one per box ([N], any integer dtype; with device boxes a torch tensor or a scalar).  For each
        box the squared Euclidean distance d2 (int32, voxels^2; 0 when they touch) to the nearest voxel that blocks -- classified as
        collides() classifies it in strict mode (threshold / occupied_above as there; outside the volume is unseen); stop_at "occupied":
        occupied voxels block; "unseen": unseen ones too -- among those with d2 <= r_max^2: CLEARANCE_NONE (-1) if there is none,
        CLEARANCE_INVALID (-2) for side < 1, r_max outside 0 .. 32767 or coordinates beyond +-2^19.  With nearest, (d2, nearest): that voxel
        [N, 3] int32 x y z, among equally near ones the smallest in (z, y, x) order; INT32_MIN where d2 is negative.
          - numpy int32 [N, 6]: through the host entry; numpy arrays out.
          - a torch int32 tensor on this handle's GPU (contiguous, [N, 6]): through the device entry; torch tensors on the same device out.
            The caller's current torch stream is synchronised first, and the handle before the tensors are returned.
        Anything else raises TypeError / ValueError before any library call."""
        stop = self._stop_at("clearance", stop_at)
        test = self._occupancy_test("clearance", threshold, occupied_above)
        torch, b, n = self._batch_input("clearance", "boxes", boxes, np.int32, 6)
        if torch is not None and _torch_module(r_max) is not None:
            if r_max.dtype not in (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64):
                raise TypeError(f"clearance: r_max must be an integer or an integer array, got {r_max.dtype}")
            if tuple(r_max.shape) not in ((), (n,)):
                raise ValueError(f"clearance: r_max must be a scalar or have shape [{n}], got {list(r_max.shape)}")
            # (out of int32 range: invalid whatever it is, kept invalid by the clamp)
            r = r_max.to(device=b.device).clamp(-1, _CLEARANCE_R_CLAMP).to(torch.int32).expand(n)
            q = torch.cat([b, r.reshape(n, 1)], 1).contiguous()
        else:
            r = np.asarray(r_max)
            if isinstance(r_max, (bool, np.bool_)) or r.dtype.kind not in "iu":
                raise TypeError(f"clearance: r_max must be an integer or an integer array, got {r.dtype}")
            if r.shape not in ((), (n,)):
                raise ValueError(f"clearance: r_max must be a scalar or have shape [{n}], got {list(r.shape)}")
            r = np.broadcast_to(np.clip(r.astype(np.int64), -1, _CLEARANCE_R_CLAMP).astype(np.int32), (n,))
            if torch is None:
                q = np.ascontiguousarray(np.concatenate([b, r.reshape(n, 1)], 1))
            else:
                q = torch.cat([b, torch.from_numpy(r.copy()).to(b.device).reshape(n, 1)], 1).contiguous()
        dev = q.device if torch else None
        res, out = self._batch_outputs(torch, dev, (n,), self._CLEARANCE_OUTPUTS, {"d2": True, "nearest": bool(nearest)}, _ClearanceOut)
        self._call(torch, dev, "se_hip_clearance_boxes", self._ptr(torch, q, n), n, C.byref(test), stop, C.byref(out))
        return (res["d2"], res["nearest"]) if nearest else res["d2"]

    _PROJECT_OUTPUTS = (("status", (), np.uint8), ("first", (), np.int32), ("last", (), np.int32), ("count", (), np.int32))

    def project(self, axis, lo, side, layers, stop_at: str = "occupied", threshold: float = 0.0, occupied_above=None, first: bool = True,
                last: bool = True, count: bool = True, device: bool = False) -> dict:
        """Column projections of the map (se_hip_project_columns, include/se_hip.h): the 2D grids of a footprint.  axis 0 / 1 / 2: the axis w
        the columns run along; the two remaining axes in ascending order are u (the fastest index) and v (axis 2: u = x, v = y; axis 1:
        u = x, v = z; axis 0: u = y, v = z).  lo, side: two integers each, the footprint [lo, lo + side) on (u, v) in voxels; layers: 1 .. 16
        pairs (a, b), the half-open intervals [a, b) along w.  Cell (l, j, i) holds the voxels with u = lo[0] + i, v = lo[1] + j, w in
        [a_l, b_l), each classified as collides() classifies it in strict mode (threshold / occupied_above as there; outside the volume is
        unseen); a voxel blocks when it is occupied (stop_at "occupied") or occupied or unseen ("unseen").  Returns a dict of arrays
        [L, side[1], side[0]]: "status" (uint8, the min class over the cell: COLLISION_OCCUPIED / _UNSEEN / _EMPTY) and, where asked for,
        "first" and "last" (int32, the smallest and the largest w of a blocking voxel, PROJECT_NONE where none blocks) and "count" (int32,
        the number of blocking voxels).  Along z with stop_at "occupied", last is the elevation map and first the ceiling.
          - device=False: through the host entry; numpy arrays out.
          - device=True: through the device entry; torch tensors on this handle's GPU out, the handle synchronised before they are returned.
        A side < 1, an empty layer, a coordinate beyond +-2^20, more than 16 layers or more than 2^28 cells raise ValueError, wrong types
        TypeError, before any library call."""
        if isinstance(axis, (bool, np.bool_)) or not isinstance(axis, (int, np.integer)):
            raise TypeError(f"project: axis must be an int, got {type(axis).__name__}")
        if axis not in (0, 1, 2):
            raise ValueError(f"project: axis must be 0, 1 or 2, got {axis}")
        stop = self._stop_at("project", stop_at)
        test = self._occupancy_test("project", threshold, occupied_above)
        lo, side = (self._ints("project", nm, v, (2,)).astype(np.int64) for nm, v in (("lo", lo), ("side", side)))
        if isinstance(layers, (bool, np.bool_)) or layers is None:
            raise TypeError(f"project: layers must be pairs of integers, got {type(layers).__name__}")
        lay = np.asarray(layers)
        if lay.ndim != 2 or lay.shape[1] != 2 or not 1 <= lay.shape[0] <= PROJECT_MAX_LAYERS:
            raise ValueError(f"project: layers must have shape [L, 2] with L in 1 .. {PROJECT_MAX_LAYERS}, got {list(lay.shape)}")
        lay = self._ints("project", "layers", lay).astype(np.int64)
        if (side < 1).any():
            raise ValueError(f"project: side must be >= 1, got {side.tolist()}")
        if (lay[:, 0] >= lay[:, 1]).any():
            raise ValueError("project: every layer needs a < b")
        if (np.abs(np.concatenate([lo, lo + side, lay.reshape(-1)])) > PROJECT_LIMIT).any():
            raise ValueError("project: lo, lo + side and the layers must lie within +-2^20")
        n_l, cells = len(lay), len(lay) * int(side[0]) * int(side[1])
        if cells > PROJECT_MAX_CELLS:
            raise ValueError(f"project: {cells} cells, more than 2^28")
        rq = _ProjectRequest()
        rq.axis, rq.n_layers, rq.stop_at = int(axis), n_l, stop
        for k in range(2):
            rq.lo[k], rq.side[k] = int(lo[k]), int(side[k])
        for l in range(n_l):
            rq.layers[l][0], rq.layers[l][1] = int(lay[l, 0]), int(lay[l, 1])
        want = {"status": True, "first": bool(first), "last": bool(last), "count": bool(count)}
        torch, dev = self._own_device(device)
        res, out = self._batch_outputs(torch, dev, (n_l, int(side[1]), int(side[0])), self._PROJECT_OUTPUTS, want, _ProjectOut)
        self._call(torch, dev, "se_hip_project_columns", C.byref(rq), C.byref(test), C.byref(out))
        return res

    _FIELD_OUTPUTS = _CLEARANCE_OUTPUTS     # (the same two arrays, per voxel of the region)

    def distance_field(self, lo, side, r_max, robot=(1, 1, 1), stop_at: str = "occupied", threshold: float = 0.0, occupied_above=None,
                       nearest: bool = False, device: bool = False):
        """The distance field of a map region (se_hip_distance_field, include/se_hip.h): lo, side three integers each, the region
        [lo, lo + side) in voxels (x, y, z); robot the side of the box whose min corner is placed at each voxel ((1, 1, 1): the plain voxel
        field); r_max the search radius in voxels, 0 .. 255.  Returns d2 [side z, side y, side x] int32: entry (k, j, i) is exactly what
        clearance() answers for the box (lo + (i, j, k), robot) with this r_max, stop_at, threshold and occupied_above -- the squared distance
        to the nearest blocking voxel, 0 when they touch, CLEARANCE_NONE (-1) when none lies within r_max; blocking voxels outside the region
        and outside the volume (unseen) count.  With nearest, (d2, nearest): that voxel [side z, side y, side x, 3] int32 x y z, among
        equally near ones the smallest in (z, y, x) order; INT32_MIN where d2 is CLEARANCE_NONE.
          - device=False: through the host entry; numpy arrays out.
          - device=True: through the device entry; torch tensors on this handle's GPU out, the handle synchronised before they are returned.
        A side or robot < 1, a robot > 256, r_max outside 0 .. 255, lo or lo + side + robot beyond +-2^19, more than 2^24 voxels or
        side[0] * D1 * D2 > 2^28 (D_k = side[k] + robot[k] + 2 r_max + 1) raise ValueError, wrong types TypeError, before any library call."""
        stop = self._stop_at("distance_field", stop_at)
        test = self._occupancy_test("distance_field", threshold, occupied_above)
        if isinstance(r_max, (bool, np.bool_)) or not isinstance(r_max, (int, np.integer)):
            raise TypeError(f"distance_field: r_max must be an int, got {type(r_max).__name__}")
        lo, side, robot = ([int(x) for x in self._ints("distance_field", nm, v, (3,))] for nm, v in (("lo", lo), ("side", side), ("robot", robot)))
        r = int(r_max)
        self._region("distance_field", lo, side, robot, "voxels", r)
        work = side[0] * (side[1] + robot[1] + 2 * r + 1) * (side[2] + robot[2] + 2 * r + 1)
        if work > FIELD_MAX_WORK:
            raise ValueError(f"distance_field: side[0] * D1 * D2 = {work}, more than 2^28")
        rq = _FieldRequest()
        rq.r_max, rq.stop_at = r, stop
        for k in range(3):
            rq.lo[k], rq.side[k], rq.robot[k] = lo[k], side[k], robot[k]
        torch, dev = self._own_device(device)
        res, out = self._batch_outputs(torch, dev, (side[2], side[1], side[0]), self._FIELD_OUTPUTS, {"d2": True, "nearest": bool(nearest)}, _FieldOut)
        self._call(torch, dev, "se_hip_distance_field", C.byref(rq), C.byref(test), C.byref(out))
        return (res["d2"], res["nearest"]) if nearest else res["d2"]

    _REACH_OUTPUTS = (("steps", (), np.int32), ("seed", (), np.uint8), ("next", (), np.uint8))

    def reach_field(self, lo, side, seeds, robot=(1, 1, 1), stop_at: str = "occupied", threshold: float = 0.0, occupied_above=None,
                    seed: bool = False, next: bool = False, counts: bool = False, device: bool = False) -> dict:
        """The reachability field of a map region (se_hip_reach_field, include/se_hip.h): lo, side three integers each, the region
        [lo, lo + side) in voxels (x, y, z); seeds integers [n, 3], 1 <= n <= 255, absolute voxel positions (x, y, z); robot the side of the
        box whose min corner stands at a position.  A position is free iff collides() in strict mode answers a status above stop_at for the
        box there; moves are 6-connected between free positions of the region; a seed outside the region or at a position that is not free
        is ignored.  Returns a dict: "steps" [side z, side y, side x] int32, the moves to the nearest usable seed or REACH_NONE (-1); with
        seed, "seed" uint8, the lowest index among the nearest seeds or 255; with next, "next" uint8, the first move of a shortest path to
        that seed (0 .. 5: -x +x -y +y -z +z, REACH_AT_SEED at a seed, 255 where steps is REACH_NONE; reach_path follows it); with counts,
        "counts" numpy int64 [4]: free positions, reached positions, the largest steps (-1: nothing reached), relaxation rounds.
          - device=False: through the host entry; numpy arrays out.
          - device=True: through the device entry; torch tensors on this handle's GPU out ("counts" stays numpy).
        Either way the handle is synchronised when the call returns.  A side or robot < 1, a robot > 256, lo or lo + side + robot beyond
        +-2^19, more than 2^24 positions, no seed or more than 255, a seed coordinate beyond int32 raise ValueError, wrong types TypeError,
        before any library call."""
        stop = self._stop_at("reach_field", stop_at)
        test = self._occupancy_test("reach_field", threshold, occupied_above)
        lo, side, robot = ([int(x) for x in self._ints("reach_field", nm, v, (3,))] for nm, v in (("lo", lo), ("side", side), ("robot", robot)))
        sd = self._ints("reach_field", "seeds", seeds)
        if sd.ndim != 2 or sd.shape[1] != 3:
            raise ValueError(f"reach_field: seeds must have shape [n, 3], got {list(sd.shape)}")
        if not 1 <= sd.shape[0] <= REACH_MAX_SEEDS:
            raise ValueError(f"reach_field: 1 .. {REACH_MAX_SEEDS} seeds, got {sd.shape[0]}")
        if sd.min() < -(2 ** 31) or sd.max() > 2 ** 31 - 1:
            raise ValueError("reach_field: a seed coordinate beyond int32")
        sd = np.ascontiguousarray(sd, np.int32)
        self._region("reach_field", lo, side, robot, "positions")
        rq = _ReachRequest()
        rq.stop_at, rq.n_seeds, rq.seeds = stop, sd.shape[0], sd.ctypes.data
        for k in range(3):
            rq.lo[k], rq.side[k], rq.robot[k] = lo[k], side[k], robot[k]
        cnt = np.zeros(4, np.int64) if counts else None
        torch, dev = self._own_device(device)
        res, out = self._batch_outputs(torch, dev, (side[2], side[1], side[0]), self._REACH_OUTPUTS, {"steps": True, "seed": seed, "next": next}, _ReachOut,
                                       self._ptr(None, cnt))
        self._call(torch, dev, "se_hip_reach_field", C.byref(rq), C.byref(test), C.byref(out))
        if counts:
            res["counts"] = cnt
        return res

    @staticmethod
    def _edit_only(only) -> int:
        """se_hip_edit.only from "any", a class name, an iterable of class names or the bit mask itself (1 .. 7)."""
        if isinstance(only, (bool, np.bool_)):
            raise TypeError("edit: only must be a class name, an iterable of class names or an int in 1 .. 7, got bool")
        if isinstance(only, (int, np.integer)):
            if not 1 <= int(only) <= 7:
                raise ValueError(f"edit: only must lie in 1 .. 7, got {only}")
            return int(only)
        names = [only] if isinstance(only, str) else list(only)
        bits = 0
        for nm in names:
            if nm not in _EDIT_CLASSES:
                raise ValueError(f"edit: only names must be among {sorted(_EDIT_CLASSES)}, got {nm!r}")
            bits |= _EDIT_CLASSES[nm]
        if not bits:
            raise ValueError("edit: only selects no class")
        return bits

    def edit_records(self, records, *, test=None, mode: str = "strict", counts: bool = True):
        """se_hip_edit_boxes on a ready list of se_hip_edit records, applied in list order: a numpy array of EDIT_DTYPE [N] (host entry) or a
        torch int32 [N, 10] tensor on this handle's GPU (device entry; columns lo xyz, hi xyz, the bits of x and y, flags, only).  test: None
        or (threshold, occupied_above) for the class predicates.  Invalid records are skipped and counted by the library, not refused here.
        Returns int64 [4] -- voxel applications, node-value applications, blocks touched, invalid edits -- as a numpy array or a torch tensor
        (None with counts=False)."""
        if mode not in _EDIT_MODES:
            raise ValueError(f"edit: mode must be one of {sorted(_EDIT_MODES)}, got {mode!r}")
        ctest = None
        if test is not None:
            thr, above = test
            ctest = C.byref(self._occupancy_test("edit", thr, above, records=True))
        if type(records) is np.ndarray and records.dtype == EDIT_DTYPE:
            if records.ndim != 1:
                raise ValueError(f"edit: records must have shape [N], got {list(records.shape)}")
            torch, rec, n = None, np.ascontiguousarray(records), records.shape[0]
            out = np.zeros(4, np.int64) if counts else None
        else:
            torch, rec, n = self._batch_input("edit", "records", records, np.int32, 10)
            if torch is None:
                raise TypeError("edit: records must be a numpy array of EDIT_DTYPE or a torch int32 [N, 10] tensor on the GPU")
            out = torch.zeros(4, dtype=torch.int64, device=rec.device) if counts else None
        self._call(torch, rec.device if torch else None, "se_hip_edit_boxes", self._ptr(torch, rec, n), n, ctest, _EDIT_MODES[mode], self._ptr(torch, out))
        return out

    def edit(self, boxes, x=None, y=None, *, only="any", threshold: float = 0.0, occupied_above=None, mode: str = "strict", blocks: bool = True,
             nodes: bool = True, counts: bool = True):
        """Batched axis-aligned region edits of the resident map (se_hip_edit_boxes, include/se_hip.h): boxes [N, 6] int32 = lo xyz, hi xyz in
        voxels, half open, applied in list order (where boxes overlap the later one wins).  x, y: the value to assign -- None (leave it), a
        scalar or one value per box.  Only existing blocks (blocks=True: their voxels) and nodes (nodes=True: their value_[8]) are written;
        nothing is allocated.  only: the classes the current value may have -- "any", "occupied", "unseen", "empty", an iterable of these or
        the bit mask -- judged with threshold / occupied_above exactly as collides() judges (occupied_above defaults by field).  mode "strict":
        a node value is written iff its child octant lies wholly inside the box; "reference": the reference's update_node, quirks included.
          - numpy int32 [N, 6]: through the host entry; numpy counts out.
          - a torch int32 tensor on this handle's GPU (contiguous, [N, 6]): through the device entry; the caller's current torch stream is
            synchronised first, and the handle before the counts are returned.
        Returns int64 [4]: voxel applications, node-value applications, blocks touched, invalid edits (None with counts=False).  A box or value
        the library calls invalid (a coordinate beyond +-2^30, a non-finite value, for SDF a y that is not an integer in 0 .. 255) is skipped
        and counted there; wrong types and shapes raise TypeError / ValueError before any library call.  After an edit, a LiveMesh is brought
        up to date with update(pipe, region=(lo - 1, hi))."""
        if mode not in _EDIT_MODES:
            raise ValueError(f"edit: mode must be one of {sorted(_EDIT_MODES)}, got {mode!r}")
        bits = self._edit_only(only)
        test = self._occupancy_test("edit", threshold, occupied_above)
        for nm, v in (("blocks", blocks), ("nodes", nodes)):
            if not isinstance(v, (bool, np.bool_)):
                raise TypeError(f"edit: {nm} must be a bool, got {type(v).__name__}")
        torch, b, n = self._batch_input("edit", "boxes", boxes, np.int32, 6)
        flags = (EDIT_SET_X if x is not None else 0) | (EDIT_SET_Y if y is not None else 0) | (EDIT_BLOCKS if blocks else 0) | (EDIT_NODES if nodes else 0)
        vals = []
        for nm, v in (("x", x), ("y", y)):
            if v is None:
                v = 0.0
            if torch is not None and _torch_module(v) is not None:
                v = v.to(device=b.device, dtype=torch.float32)
            else:
                v = np.asarray(v, np.float32)
            if v.ndim != 0 and tuple(v.shape) != (n,):
                raise ValueError(f"edit: {nm} must be a scalar or have shape [{n}], got {list(v.shape)}")
            vals.append(v)
        if torch is None:
            rec = np.zeros(n, EDIT_DTYPE)
            rec["lo"], rec["hi"] = b[:, 0:3], b[:, 3:6]
            rec["x"], rec["y"] = vals
            rec["flags"], rec["only"] = flags, bits
        else:
            rec = torch.empty((n, 10), dtype=torch.int32, device=b.device)
            rec[:, 0:6] = b
            fl = rec[:, 6:8].view(torch.float32)
            for j, v in enumerate(vals):
                fl[:, j] = v if _torch_module(v) is not None else torch.as_tensor(v).to(b.device)
            rec[:, 8], rec[:, 9] = flags, bits
        return self.edit_records(rec, test=(test.threshold, bool(test.occupied_above)), mode=mode, counts=counts)

    def init_value(self):
        """initValue() of the handle's field type as (x, y): what a voxel holds before anything is fused into it."""
        return (0.0, 0.0) if self.field == OFUSION else (1.0, 0.0)

    def reset(self, boxes, **kw):
        """Forget regions: every voxel and node value the boxes select back to initValue(), so that the next frames re-fuse them
        (edit(boxes, x, y) with both values of initValue(); the keywords of edit apply)."""
        ix, iy = self.init_value()
        return self.edit(boxes, ix, iy, **kw)

    def allocate_records(self, records, *, counts: bool = True, key_capacity: int = 0):
        """se_hip_allocate_boxes on a ready list of se_hip_alloc_box records: a numpy array of ALLOC_DTYPE [N] (host entry) or a torch int32
        [N, 8] tensor on this handle's GPU (device entry; columns lo xyz, hi xyz, level, reserved).  Invalid records are skipped and counted
        by the library, not refused here.  key_capacity > 0: also the list [count, key ...] of the octants the call created on request, with
        room for that many keys (uint64 [key_capacity + 1]; count may exceed what was written).  Returns (counts, keys): int64 [4] -- blocks
        created, nodes created, requested (box, octant) pairs, invalid boxes -- and the list, numpy arrays or torch tensors; None where not
        asked for.  A pool that runs out raises SeHipError (SE_HIP_E_CAPACITY; clear_overflow acknowledges it)."""
        if isinstance(key_capacity, (bool, np.bool_)) or not isinstance(key_capacity, (int, np.integer)) or key_capacity < 0:
            raise ValueError(f"allocate: key_capacity must be an int >= 0, got {key_capacity!r}")
        words = int(key_capacity) + 1 if key_capacity else 0
        if type(records) is np.ndarray and records.dtype == ALLOC_DTYPE:
            if records.ndim != 1:
                raise ValueError(f"allocate: records must have shape [N], got {list(records.shape)}")
            torch, rec, n = None, np.ascontiguousarray(records), records.shape[0]
            out = np.zeros(4, np.int64) if counts else None
            keys = np.zeros(words, np.uint64) if words else None
        else:
            torch, rec, n = self._batch_input("allocate", "records", records, np.int32, 8)
            if torch is None:
                raise TypeError("allocate: records must be a numpy array of ALLOC_DTYPE or a torch int32 [N, 8] tensor on the GPU")
            out = torch.zeros(4, dtype=torch.int64, device=rec.device) if counts else None
            keys = torch.zeros(words, dtype=torch.int64, device=rec.device) if words else None      # (torch has no uint64 arithmetic: the bits)
        self._call(torch, rec.device if torch else None, "se_hip_allocate_boxes", self._ptr(torch, rec, n), n, self._ptr(torch, out), self._ptr(torch, keys),
                   words)
        return out, keys

    def allocate(self, boxes, level=0, return_keys: bool = False):
        """Batched region allocation of the resident map (se_hip_allocate_boxes, include/se_hip.h): boxes [N, 6] int32 = lo xyz, hi xyz in
        voxels, half open.  Every octant of `level` -- 0: the 8^3 blocks; 1 .. leaf level: the octants of that tree level, as nodes without
        children; a scalar or one value per box -- that a box touches inside the volume exists afterwards, with all its ancestors; new blocks
        hold initValue() and are active, what existed is untouched.  It is Octree::allocate over those keys without the keys[0] rule.  Use
        it in front of edit() for a region the camera has not seen.
          - numpy int32 [N, 6]: through the host entry; numpy out.
          - a torch int32 tensor on this handle's GPU (contiguous, [N, 6]): through the device entry; the caller's current torch stream is
            synchronised first, and the handle before the results are returned.
        Returns int64 [4]: blocks created, nodes created (ancestors included), requested (box, octant) pairs after clipping, invalid boxes.
        return_keys=True: (counts, keys) with keys the uint64 keys (torch: their bits as int64) of the octants the call created on request,
        fit for alloc_commit on a peer replica as [len(keys), *keys].  A box the library calls invalid (a coordinate beyond +-2^30, a level
        outside 0 .. leaf level) is skipped and counted there; wrong types and shapes raise TypeError / ValueError before any library call."""
        if not isinstance(return_keys, (bool, np.bool_)):
            raise TypeError(f"allocate: return_keys must be a bool, got {type(return_keys).__name__}")
        torch, b, n = self._batch_input("allocate", "boxes", boxes, np.int32, 6)
        if torch is not None and _torch_module(level) is not None:
            lv = level.to(device=b.device, dtype=torch.int32)
        else:
            lv = np.asarray(level)
            if lv.dtype.kind not in "iu":
                raise TypeError(f"allocate: level must be an integer or an integer array, got {lv.dtype}")
            lv = lv.astype(np.int32)
        if lv.ndim != 0 and tuple(lv.shape) != (n,):
            raise ValueError(f"allocate: level must be a scalar or have shape [{n}], got {list(lv.shape)}")
        if torch is None:
            rec = np.zeros(n, ALLOC_DTYPE)
            rec["lo"], rec["hi"], rec["level"] = b[:, 0:3], b[:, 3:6], lv
        else:
            rec = torch.zeros((n, 8), dtype=torch.int32, device=b.device)
            rec[:, 0:6] = b
            rec[:, 6] = lv if _torch_module(lv) is not None else torch.as_tensor(lv).to(b.device)
        if not return_keys:
            return self.allocate_records(rec)[0]
        # room for every key the call can write: at most one per requested pair (blocks are the finest request), never more than the tree holds
        cap = 0
        if n:
            bb = (b.cpu().numpy() if torch is not None else b).astype(np.int64)
            lo = np.clip(bb[:, 0:3], 0, self.size) // 8
            hi = (np.clip(bb[:, 3:6], 0, self.size) + 7) // 8
            cap = min(int(np.prod(np.maximum(hi - lo, 0), axis=1).sum()), (self.size // 8) ** 3 * 8 // 7 + 1)
        counts, keys = self.allocate_records(rec, key_capacity=max(cap, 1))
        k = int(keys[0])
        return counts, keys[1:1 + k]

    _RAY_OUTPUTS = (("hit", (4,), np.float32), ("normal", (3,), np.float32), ("status", (), np.uint8))

    def cast_rays(self, origins, directions, near=0.4, far=4.0, *, mu: float, normalize: bool = False, hit: bool = True, normal: bool = True,
                  status: bool = True) -> dict:
        """Batched ray casts (se_hip_cast_rays, include/se_hip.h): for each ray, the reference's raycastKernel body from `origins` along
        `directions` within [near, far] (metres, world frame) -- hit (x, y, z, t), normal, and status bits (RAY_VALID, RAY_ENTERED, RAY_HIT,
        RAY_NORMAL).  Returns a dict of the outputs asked for.  near / far: a scalar or one value per ray.  Directions are used as given
        (the library refuses rays whose squared norm lies outside [0.98, 1.02]); normalize=True divides them by their norm first, in the
        caller's framework (numpy: the float32 arithmetic of Eigen's normalized(); torch: torch's).  mu: the truncation distance of the
        SDF march, as raycasting() takes it.
          - numpy float32 [N, 3] arrays: through the host entry; numpy arrays out.
          - torch float32 [N, 3] tensors on this handle's GPU: packed to [N, 8] on the device, through the device entry; outputs are torch
            tensors on the same device.  The caller's current torch stream is synchronised first, and the handle before the tensors are
            returned.
        Anything else raises TypeError / ValueError before any library call."""
        want = {"hit": hit, "normal": normal, "status": status}
        if not any(want.values()):
            raise ValueError("cast_rays: no output requested")
        mu = float(mu)
        if not (np.isfinite(np.float32(mu)) and mu > 0):
            raise ValueError(f"cast_rays: mu must be finite and > 0, got {mu!r}")
        both_numpy = type(origins) is np.ndarray and type(directions) is np.ndarray
        if not both_numpy and (_torch_module(origins) is None or _torch_module(directions) is None):
            raise TypeError("cast_rays: origins and directions must both be numpy float32 arrays or both torch tensors on the GPU, got "
                            f"{type(origins).__name__} and {type(directions).__name__}")
        torch, origins, n = self._batch_input("cast_rays", "origins", origins, np.float32, 3, contiguous=False)
        _, d, nd = self._batch_input("cast_rays", "directions", directions, np.float32, 3, contiguous=False)
        if nd != n:
            raise ValueError(f"cast_rays: {n} origins but {nd} directions")
        # the [N, 8] rays, packed by the library the inputs came from (numpy on the host, torch on the device)
        xp = np if torch is None else torch
        if normalize:
            z = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            d = xp.where((z > 0)[:, None], d / xp.sqrt(z)[:, None], d)
        rays = np.empty((n, 8), np.float32) if torch is None else torch.empty((n, 8), dtype=torch.float32, device=origins.device)
        rays[:, 0:3] = origins
        rays[:, 3:6] = d
        for j, name, v in ((6, "near", near), (7, "far", far)):
            if torch is None:
                v = np.asarray(v)
            elif _torch_module(v) is None:
                v = torch.as_tensor(np.asarray(v, np.float32))
            if v.ndim != 0 and tuple(v.shape) != (n,):
                raise ValueError(f"cast_rays: {name} must be a scalar or have shape [{n}], got {list(v.shape)}")
            rays[:, j] = v.astype(np.float32) if torch is None else v.to(device=origins.device, dtype=torch.float32)
        dev = rays.device if torch else None
        res, out = self._batch_outputs(torch, dev, (n,), self._RAY_OUTPUTS, want, _RayOut)
        self._call(torch, dev, "se_hip_cast_rays", self._ptr(torch, rays, n), n, mu, C.byref(out))
        return res

    def _mesh_select(self, region, views, skip_empty):
        """se_hip_mesh_select for mesh_blocks, checked here (TypeError / ValueError) so that nothing bad reaches the library."""
        sel = _MeshSelect()
        if region is None:
            lo, hi = (0, 0, 0), (self.size,) * 3
        else:
            try:
                lo, hi = region
                lo, hi = tuple(lo), tuple(hi)
            except TypeError:
                raise TypeError("mesh_blocks: region must be (lo, hi), two triples of voxel coordinates") from None
            if len(lo) != 3 or len(hi) != 3:
                raise ValueError(f"mesh_blocks: region must be (lo, hi) with three coordinates each, got {len(lo)} and {len(hi)}")
            for v in lo + hi:
                if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                    raise TypeError(f"mesh_blocks: region coordinates must be integers (voxels), got {type(v).__name__}")
                if not -2**31 <= int(v) < 2**31:
                    raise ValueError(f"mesh_blocks: region coordinate {v} does not fit int32")
        sel.lo[:], sel.hi[:] = [int(v) for v in lo], [int(v) for v in hi]
        views = [] if views is None else list(views)
        if len(views) > MESH_MAX_VIEWS:
            raise ValueError(f"mesh_blocks: at most {MESH_MAX_VIEWS} views, got {len(views)}")
        arr = (_MeshView * max(len(views), 1))()
        for i, v in enumerate(views):
            try:
                pose, k = v[0], v[1]
                w, h = (self.W, self.H) if len(v) == 2 else (v[2], v[3])
            except (TypeError, IndexError, KeyError):
                raise TypeError("mesh_blocks: a view is (pose 4x4 camera-to-world, k) or (pose, k, width, height)") from None
            pose, k = np.asarray(pose), np.asarray(k)
            for name, a, n in (("pose", pose, 16), ("k", k, 4)):
                if a.dtype.kind not in "fiu":
                    raise TypeError(f"mesh_blocks: view {i}: {name} must be numeric, got {a.dtype}")
                if a.size != n:
                    raise ValueError(f"mesh_blocks: view {i}: {name} must have {n} values, got {a.size}")
            pose, k = pose.astype(np.float32).reshape(4, 4), k.astype(np.float32).reshape(4)
            if not (np.isfinite(pose).all() and np.isfinite(k).all()):
                raise ValueError(f"mesh_blocks: view {i}: non-finite pose or intrinsics")
            if k[0] == 0 or k[1] == 0:
                raise ValueError(f"mesh_blocks: view {i}: fx and fy must not be 0")
            if isinstance(w, (bool, np.bool_)) or isinstance(h, (bool, np.bool_)) or not (isinstance(w, (int, np.integer)) and isinstance(h, (int, np.integer))):
                raise TypeError(f"mesh_blocks: view {i}: width and height must be integers")
            if w <= 0 or h <= 0:
                raise ValueError(f"mesh_blocks: view {i}: image size must be positive, got {w} x {h}")
            arr[i].pose[:] = pose.T.reshape(16).tolist()
            arr[i].k[:] = k.tolist()
            arr[i].width, arr[i].height = int(w), int(h)
        sel.n_views, sel.flags = len(views), MESH_SKIP_EMPTY if skip_empty else 0
        sel.views = C.cast(arr, C.POINTER(_MeshView))
        return sel, arr

    def mesh_blocks(self, region=None, views=None, skip_empty: bool = False, device: bool = False) -> dict:
        """Live meshing per block (se_hip_mesh_blocks, include/se_hip.h): the marching-cubes triangles of the allocated blocks that intersect
        `region` ((lo, hi) in voxels, half-open; None = the whole volume) and, if `views` is given, may have been touched by one of them --
        up to 64 views, each (pose 4x4 camera-to-world, k) with this handle's image size or (pose, k, width, height).
        Returns {"coords": [B, 3] int32 voxel coordinates of the block corners, "ranges": [B, 2] int64 (first, count) into "triangles",
        "triangles": [T, 3, 3] float32 metres}.  A block's triangles are contiguous and in a defined order; blocks without a triangle are
        listed with count 0 unless skip_empty.  numpy arrays through the host entry (a sizing call, then the real one); device=True: torch
        tensors on this handle's GPU through the device entry.  Bad input raises TypeError / ValueError before any library call."""
        sel, keep = self._mesh_select(region, views, bool(skip_empty))
        if not device:
            fn, sync = self.lib.se_hip_mesh_blocks_host, lambda: None      # (the host entry synchronises itself)
            head = np.zeros(4, np.int64)
            alloc, addr = (lambda shape, dt: np.empty(shape, dt)), (lambda a: a.ctypes.data)
        else:
            import torch
            dev = torch.device("cuda", self._device or 0)
            head = torch.zeros(4, dtype=torch.int64, device=dev)
            torch.cuda.current_stream(dev).synchronize()
            fn, sync = self.lib.se_hip_mesh_blocks, self.sync
            alloc, addr = (lambda shape, dt: torch.empty(shape, dtype=getattr(torch, np.dtype(dt).name), device=dev)), (lambda a: a.data_ptr())
        # a sizing call (no capacity: the header alone), then the real one into arrays of exactly that size
        self._check(fn(self._h, C.byref(sel), C.byref(_MeshOut(None, 0, None, None, 0, addr(head)))))
        sync()
        nb, nt = (int(v) for v in head[:2].tolist())
        coords, ranges, tris = alloc((nb, 3), np.int32), alloc((nb, 2), np.int64), alloc((nt, 3, 3), np.float32)
        if nb:
            out = _MeshOut(addr(tris) if nt else None, nt, addr(coords), addr(ranges), nb, addr(head))
            self._check(fn(self._h, C.byref(sel), C.byref(out)))
            sync()
            assert head.tolist() == [nb, nt, nb, nt], head.tolist()
        return {"coords": coords, "ranges": ranges, "triangles": tris}

    def save(self, filename: str):
        """Octree::save of the reference (octree.hpp:898-914): same byte layout, entries sorted by key."""
        self._check(self.lib.se_hip_save_map(self._h, filename.encode()))

    def load(self, filename: str):
        """Octree::load counterpart (octree.hpp:917-950, minus its two defects): the map becomes what the file holds."""
        self._check(self.lib.se_hip_load_map(self._h, filename.encode()))

    @staticmethod
    def _shift_argument(shift_voxels) -> np.ndarray:
        """The shift as int32 [3], checked (TypeError / ValueError) before any library call: three integers, multiples of 8, within +-2^30."""
        s = np.asarray(shift_voxels)
        if s.dtype.kind not in "iu":
            raise TypeError(f"shift: shift_voxels must be integers (voxels), got {s.dtype}")
        if s.shape != (3,):
            raise ValueError(f"shift: shift_voxels must have shape (3,), got {list(s.shape)}")
        s = s.astype(np.int64)
        if (s % 8 != 0).any():
            raise ValueError(f"shift: every component must be a multiple of 8 (the block side), got {s.tolist()}")
        if (np.abs(s) > 1 << 30).any():
            raise ValueError(f"shift: every component must lie in [-2^30, 2^30], got {s.tolist()}")
        return s.astype(np.int32)

    def shift(self, shift_voxels) -> np.ndarray:
        """Rolling volume (se_hip_shift_map, include/se_hip.h): the map content is translated by shift_voxels (three integers, multiples of
        8) on the device -- content at voxel c is at c + s afterwards, what leaves the cube is forgotten, the vacated side is unseen;
        surviving blocks keep their values and active flags, nodes the shift is aligned to keep theirs.  pose_ is translated with the map
        (s * dim / size added to its translation), so the camera stays where it was relative to the content; a robot that walks towards +x
        passes a negative s[0].  The vertex / normal images stay in the old frame of reference: tracking() raises until a raycast has run.
        Returns int64 [4]: blocks kept, blocks dropped, nodes kept, nodes dropped.  Wrong types and shapes raise before any library call."""
        s = self._shift_argument(shift_voxels)
        out = np.zeros(4, np.int64)
        self._check(self.lib.se_hip_shift_map(self._h, s.ctypes.data, out.ctypes.data))
        pose = self.pose_.copy()
        pose[:3, 3] += s.astype(np.float32) * (np.float32(self.dim) / np.float32(self.size))
        self.pose_ = pose
        return out

    RELEASE_WHAT = {"all": 1, "unseen": 2}                  # SE_HIP_RELEASE_*
    RELEASE_COUNTS = ("blocks_kept", "blocks_released", "nodes_kept", "nodes_released", "blocks_released_observed")
    RELEASE_MAX_BOXES = 4096

    def _release_arguments(self, boxes, what) -> np.ndarray:
        """The records of release() as RELEASE_DTYPE [N], checked (TypeError / ValueError) before any library call."""
        def code(w):
            if not isinstance(w, str):
                raise TypeError(f"release: what must be one of {sorted(self.RELEASE_WHAT)}, got {type(w).__name__}")
            if w not in self.RELEASE_WHAT:
                raise ValueError(f"release: what must be one of {sorted(self.RELEASE_WHAT)}, got {w!r}")
            return self.RELEASE_WHAT[w]
        default = code(what)
        if boxes is None:
            boxes = [((0, 0, 0), (self.size,) * 3)]
        if isinstance(boxes, (str, bytes, np.ndarray)) or not hasattr(boxes, "__len__"):
            raise TypeError(f"release: boxes must be None or a list of (lo, side) or (lo, side, what), got {type(boxes).__name__}")
        if len(boxes) > self.RELEASE_MAX_BOXES:
            raise ValueError(f"release: at most {self.RELEASE_MAX_BOXES} boxes, got {len(boxes)}")
        rec = np.zeros(len(boxes), RELEASE_DTYPE)
        for i, b in enumerate(boxes):
            if not isinstance(b, (tuple, list)) or len(b) not in (2, 3):
                raise TypeError(f"release: box {i} must be (lo, side) or (lo, side, what)")
            lo, side = np.asarray(b[0]), np.asarray(b[1])
            if lo.dtype.kind not in "iu" or side.dtype.kind not in "iu":
                raise TypeError(f"release: box {i}: lo and side must be integers (voxels), got {lo.dtype} and {side.dtype}")
            if side.ndim == 0:
                side = np.repeat(side, 3)
            if lo.shape != (3,) or side.shape != (3,):
                raise ValueError(f"release: box {i}: lo must have shape (3,) and side be a scalar or have shape (3,)")
            lo, side = lo.astype(np.int64), side.astype(np.int64)
            if (side < 1).any() or (side >= 1 << 31).any():
                raise ValueError(f"release: box {i}: every side must lie in [1, 2^31), got {side.tolist()}")
            if (lo < -(1 << 30)).any() or (lo + side > 1 << 30).any():
                raise ValueError(f"release: box {i}: lo and lo + side must lie in [-2^30, 2^30], got {lo.tolist()} + {side.tolist()}")
            rec[i]["lo"], rec[i]["side"], rec[i]["what"] = lo, side, code(b[2]) if len(b) == 3 else default
        return rec

    def release(self, boxes=None, what: str = "unseen") -> dict:
        """Hands octants back on the device (se_hip_release_boxes, include/se_hip.h): every block and node that lies wholly inside a box
        [lo, lo + side) and -- what "unseen" -- holds nothing but initValue(), or -- what "all" -- whatever it holds (the region is
        forgotten).  boxes: None (the whole volume) or a list of (lo, side) or (lo, side, what), lo three integers in voxels, side one or
        three; a box need not be a multiple of 8, an octant cut by its border stays (partial forgetting is reset()).  A node goes only with
        everything beneath it; the root stays; the entry of a surviving parent above a released octant becomes initValue(), so get()
        answers initValue() at every released voxel and "unseen" changes no answer anywhere.  Survivors keep values and active flags; the
        pools are compact afterwards.  pose_ and the vertex / normal images are untouched: tracking goes on.  A block that holds nothing
        but is still in view and in the allocation band comes back with the next allocation scan.  Returns a dict: blocks_kept,
        blocks_released, nodes_kept, nodes_released, blocks_released_observed and region = (lo, hi), the half-open voxel box of the
        released blocks (zeros if none; a LiveMesh is brought up to date with update(pipe, region=(lo - 1, hi)), as after an edit: the
        last cells of the blocks below a released one read its first voxel layer).  Wrong arguments raise before any library call."""
        rec = self._release_arguments(boxes, what)
        out, box = np.zeros(5, np.int64), np.zeros(6, np.int32)
        self._check(self.lib.se_hip_release_boxes(self._h, rec.ctypes.data if len(rec) else None, len(rec), out.ctypes.data, box.ctypes.data))
        res = {k: int(v) for k, v in zip(self.RELEASE_COUNTS, out)}
        res["region"] = (tuple(int(v) for v in box[:3]), tuple(int(v) for v in box[3:]))
        return res

    MERGE_MODES = {"fuse": 0, "replace": 1, "fill": 2}      # SE_HIP_MERGE_*
    MERGE_COUNTS = ("blocks_combined", "blocks_created", "blocks_clipped", "nodes_combined", "nodes_created", "nodes_skipped")

    def _merge_arguments(self, src, shift, mode, max_weight):
        """The arguments of merge(), checked (TypeError / ValueError) before any library call: (int32 shift [3], rule)."""
        if not isinstance(src, DenseSLAMPipeline):
            raise TypeError(f"merge: src must be a DenseSLAMPipeline, got {type(src).__name__}")
        if src is self:
            raise ValueError("merge: src is the destination itself")
        if src.field != self.field:
            raise ValueError("merge: the two maps hold different field types")
        if src._device != self._device:
            raise ValueError("merge: the two maps live on different devices (save, load into a scratch handle on this device, merge)")
        if np.float32(src.dim) / np.float32(src.size) != np.float32(self.dim) / np.float32(self.size):
            raise ValueError(f"merge: different voxel sizes ({src.dim} / {src.size} and {self.dim} / {self.size})")
        try:
            s = self._shift_argument(shift)
        except (TypeError, ValueError) as e:
            raise type(e)(str(e).replace("shift:", "merge:", 1)) from None
        if not isinstance(mode, str):
            raise TypeError(f"merge: mode must be one of {sorted(self.MERGE_MODES)}, got {type(mode).__name__}")
        if mode not in self.MERGE_MODES:
            raise ValueError(f"merge: mode must be one of {sorted(self.MERGE_MODES)}, got {mode!r}")
        if isinstance(max_weight, (bool, np.bool_)) or not isinstance(max_weight, (int, float, np.integer, np.floating)):
            raise TypeError(f"merge: max_weight must be a number, got {type(max_weight).__name__}")
        if not (1 <= max_weight <= 255 and float(max_weight) == int(max_weight)):
            raise ValueError(f"merge: max_weight must be an integer in [1, 255], got {max_weight}")
        return s, _MergeRule(self.MERGE_MODES[mode], float(max_weight))

    def merge(self, src, shift=(0, 0, 0), mode: str = "fuse", max_weight=100) -> dict:
        """The content of `src` (another handle on the same device: same field type and voxel size, any volume size) folded into this map on
        the device (se_hip_merge_map, include/se_hip.h): source content at voxel c meets this map's content at c + shift (multiples of 8).
        mode "fuse" combines where both are observed (SDF: weighted mean, weights added and capped at max_weight; OFusion: log-odds added,
        the later time), "replace" lets the source win wherever it is observed, "fill" takes the source only where this map is unseen.
        `src` is only read; this map's vertex / normal images stay valid.  Returns the counts as a dict: blocks_combined, blocks_created,
        blocks_clipped, nodes_combined, nodes_created, nodes_skipped and region = (lo, hi), the half-open voxel box of this map that holds
        every block touched (zeros if none; a LiveMesh is brought up to date with update(pipe, region=(lo - 1, hi)), as after an edit).
        Wrong arguments raise before any library call."""
        s, rule = self._merge_arguments(src, shift, mode, max_weight)
        out = np.zeros(12, np.int64)
        self._check(self.lib.se_hip_merge_map(self._h, src._h, s.ctypes.data, C.addressof(rule), out.ctypes.data))
        res = {k: int(v) for k, v in zip(self.MERGE_COUNTS, out[:6])}
        res["region"] = (tuple(int(v) for v in out[6:9]), tuple(int(v) for v in out[9:12]))
        return res

    MERGE_RIGID_COUNTS = ("blocks_combined", "blocks_created", "voxels_observed", "voxels_both")

    def merge_rigid(self, src, T_dst_src=None, pull=None, mode: str = "fuse", max_weight=100) -> dict:
        """The content of `src` resampled into this map's lattice under a rigid transform and combined as merge() combines
        (se_hip_merge_map_rigid, include/se_hip.h): every voxel of this map reads `src` at a rotated position, blended from the eight voxels
        around it; cells with an unseen corner contribute nothing.  Give either T_dst_src, the metric 4x4 pose of the source map's frame
        in this map's (rigid_pull turns it into the pull transform), or `pull` itself: src_from_dst as float32 [12] or [3, 4], in voxels.
        Node values do not take part.  `src` is only read; this map's vertex / normal images stay valid.  Returns blocks_combined (existed
        and received a sample), blocks_created, voxels_observed (voxels that received a sample), voxels_both (of those, observed here before)
        and region = (lo, hi), the half-open voxel box of the blocks that received samples (zeros if none; a LiveMesh is brought up to
        date with update(pipe, region=(lo - 1, hi)), as after an edit).  Wrong arguments raise before any library call."""
        if (T_dst_src is None) == (pull is None):
            raise TypeError("merge_rigid: give exactly one of T_dst_src and pull")
        _, rule = self._merge_arguments(src, (0, 0, 0), mode, max_weight)
        if pull is None:
            p = rigid_pull(T_dst_src, self.dim, self.size)
        else:
            p = np.asarray(pull)
            if p.dtype.kind not in "fiu" or p.size != 12 or p.shape not in ((12,), (3, 4)):
                raise (TypeError if p.dtype.kind not in "fiu" else ValueError)("merge_rigid: pull must be 12 numbers, [12] or [3, 4]")
            p = np.ascontiguousarray(p, np.float32).reshape(12)
            _check_rigid(p.reshape(3, 4).astype(np.float64), "merge_rigid: pull")
        out = np.zeros(10, np.int64)
        self._check(self.lib.se_hip_merge_map_rigid(self._h, src._h, p.ctypes.data, C.addressof(rule), out.ctypes.data))
        res = {k: int(v) for k, v in zip(self.MERGE_RIGID_COUNTS, out[:4])}
        res["region"] = (tuple(int(v) for v in out[4:7]), tuple(int(v) for v in out[7:10]))
        return res

    # ------------------------------------------------------------------ measurement
    def enable_timing(self, on: bool = True):
        self._check(self.lib.se_hip_enable_timing(self._h, int(on)))

    def timings(self, reset: bool = False) -> dict:
        ms = (C.c_double * len(KERNELS))()
        n = (C.c_int64 * len(KERNELS))()
        self._check(self.lib.se_hip_get_timings(self._h, ms, n, int(reset)))
        return {k: {"ms_sum": ms[i], "launches": n[i]} for i, k in enumerate(KERNELS)}

    def enable_stats(self, on: bool = True):
        self._check(self.lib.se_hip_enable_stats(self._h, int(on)))

    def stats(self, reset: bool = False) -> dict:
        out = (C.c_uint64 * 16)()
        self._check(self.lib.se_hip_get_stats(self._h, out, int(reset)))
        return dict(zip(STAT_NAMES, (int(v) for v in out)))
