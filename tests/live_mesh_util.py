"""Host-side helpers of the live-meshing tests (se_hip_mesh_blocks): the selection rule of DESIGN.md 4.9 restated in float64 numpy, triangles
split by block, a block's payload rebuilt on the host in the defined cell order, and a fake mesh_blocks source made from a full mesh."""
from __future__ import annotations

import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MC_TABLE = np.load(os.path.join(ROOT, "tests", "golden", "mc_tri_table_i8.npy"))
# corner i of a cell and the corners of edge e (se::algorithms::marching_cube, meshing.hpp)
CORNERS = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 1], [0, 0, 1], [0, 1, 0], [1, 1, 0], [1, 1, 1], [0, 1, 1]])
EDGES = np.array([[0, 1], [1, 2], [2, 3], [0, 3], [4, 5], [5, 6], [6, 7], [4, 7], [0, 4], [1, 5], [2, 6], [3, 7]])


def sorted_triangles(t):
    """[n, 9] float32 rows in lexicographic order of their bit patterns (a canonical order for bit-for-bit comparison)."""
    t = np.ascontiguousarray(np.asarray(t, np.float32).reshape(-1, 9))
    if len(t) == 0:
        return t
    u = t.view(np.uint32)
    return t[np.lexsort(u.T[::-1])]


def same_triangle_set(a, b):
    a, b = sorted_triangles(a), sorted_triangles(b)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def view_of(pose, k, width, height):
    return (np.asarray(pose, np.float32).reshape(4, 4), np.asarray(k, np.float32).reshape(4), int(width), int(height))


def possibly_touched(corners, views, size, dim, radius=9.0, border=1.0):
    """The rule in float64: for block corners [B, 3] (voxels), True where the sphere of `radius` voxels about corner + 4 reaches into the
    half space z > 0 and inside the four side planes through pixel columns -border and W - 1 + border, rows -border and H - 1 + border, of at
    least one view (pose camera-to-world 4x4, k, W, H).  radius 9, border 1 is the rule itself; 12 and 2 the loosened one."""
    corners = np.asarray(corners, np.float64).reshape(-1, 3)
    vs = float(np.float32(dim) / np.float32(size))
    cen = (corners + 4.0) * vs
    r = radius * vs
    out = np.zeros(len(corners), bool)
    for pose, k, W, H in views:
        T = np.linalg.inv(np.asarray(pose, np.float64).reshape(4, 4))
        pc = cen @ T[:3, :3].T + T[:3, 3]
        fx, fy, cx, cy = (float(v) for v in k)
        sx, sy = (1.0 if fx > 0 else -1.0), (1.0 if fy > 0 else -1.0)
        xl, xr = (-border - cx) / fx, (W - 1 + border - cx) / fx
        yt, yb = (-border - cy) / fy, (H - 1 + border - cy) / fy
        ok = pc[:, 2] > -r
        for n in ([sx, 0, -sx * xl], [-sx, 0, sx * xr], [0, sy, -sy * yt], [0, -sy, sy * yb]):
            n = np.asarray(n, np.float64)
            ok &= pc @ (n / np.linalg.norm(n)) > -r
        out |= ok
    return out


def exactly_touched(corners, views, size, dim):
    """The exact set the rule must cover: blocks with a voxel of their 9^3 dependency box that passes update_block's visibility test
    (pos.z >= 0.0001, pixel + 0.5 within [0.5, W - 1.5] x [0.5, H - 1.5]) under some view; float64."""
    corners = np.asarray(corners, np.float64).reshape(-1, 3)
    vs = float(np.float32(dim) / np.float32(size))
    g = np.stack(np.meshgrid(np.arange(9), np.arange(9), np.arange(9), indexing="ij"), -1).reshape(-1, 3)
    out = np.zeros(len(corners), bool)
    for pose, k, W, H in views:
        T = np.linalg.inv(np.asarray(pose, np.float64).reshape(4, 4))
        fx, fy, cx, cy = (float(v) for v in k)
        for i in range(0, len(corners), 512):
            p = (corners[i:i + 512, None, :] + g[None]) * vs
            p = np.minimum(p, (size - 1) * vs)            # (voxels beyond the volume do not exist)
            pc = p @ T[:3, :3].T + T[:3, 3]
            z = pc[..., 2]
            with np.errstate(divide="ignore", invalid="ignore"):
                u, v = fx * pc[..., 0] / z + cx + 0.5, fy * pc[..., 1] / z + cy + 0.5
            vis = (z >= 0.0001) & (u >= 0.5) & (u <= W - 1.5) & (v >= 0.5) & (v <= H - 1.5)
            out[i:i + 512] |= vis.any(axis=1)
    return out


def split_by_block(tris, size, dim):
    """{block corner (x, y, z) in voxels -> [n, 9] float32, sorted} with each triangle assigned to the block of its centroid."""
    t = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    if len(t) == 0:
        return {}
    vs = float(np.float32(dim) / np.float32(size))
    b = np.floor(t.astype(np.float64).mean(axis=1) / vs / 8).astype(np.int64) * 8
    key = b[:, 0] + (b[:, 1] << 13) + (b[:, 2] << 26)
    order = np.argsort(key, kind="stable")
    ks, first = np.unique(key[order], return_index=True)
    bounds = list(first) + [len(t)]
    out = {}
    for j in range(len(ks)):
        idx = order[bounds[j]:bounds[j + 1]]
        out[tuple(int(v) for v in b[idx[0]])] = sorted_triangles(t[idx])
    return out


def payload_of(res, i):
    """Block i's triangles of a mesh_blocks result, [count, 9] float32 in the entry's own order."""
    first, count = (int(v) for v in res["ranges"][i])
    return np.asarray(res["triangles"]).reshape(-1, 9)[first:first + count]


def by_coords(res):
    """{block corner -> bytes of its payload} of a mesh_blocks result."""
    return {tuple(int(v) for v in c): payload_of(res, i).tobytes() for i, c in enumerate(np.asarray(res["coords"]))}


def rebuild_payloads(coords, x, y, size, dim, want=None):
    """Per-block payloads from downloaded bricks (coords [B, 3], x / y [B, 512], voxel x + 8y + 64z), in the defined order: cells x fastest,
    then y, then z, a cell's triangles in table order; float32 arithmetic of se_mc_vertex, operation for operation.  A missing neighbour reads
    as unknown.  `want`: only these block corners."""
    f = np.float32
    vs = f(dim) / f(size)
    dimf = f(dim)
    index = {tuple(int(v) for v in c): i for i, c in enumerate(coords)}
    out = {}
    for c in (index if want is None else want):
        c = tuple(int(v) for v in c)
        val = np.zeros((9, 9, 9), np.float32)     # [lz, ly, lx]
        kn = np.zeros((9, 9, 9), bool)
        for n in range(8):
            d = (n & 1, (n >> 1) & 1, n >> 2)
            j = index.get((c[0] + 8 * d[0], c[1] + 8 * d[1], c[2] + 8 * d[2]))
            if j is None:
                continue
            bx, by = x[j].reshape(8, 8, 8), y[j].reshape(8, 8, 8)
            sl = tuple(slice(8, 9) if d[a] else slice(0, 8) for a in (2, 1, 0))
            src = tuple(slice(0, 1) if d[a] else slice(0, 8) for a in (2, 1, 0))
            val[sl], kn[sl] = bx[src], by[src] != 0
        top = [min(c[a] + 8, size - 1) - c[a] for a in range(3)]
        tris = []
        cell_known = np.ones((8, 8, 8), bool)
        cell_index = np.zeros((8, 8, 8), np.int64)
        for i, (dx, dy, dz) in enumerate(CORNERS):
            cell_known &= kn[dz:dz + 8, dy:dy + 8, dx:dx + 8]
            cell_index |= (val[dz:dz + 8, dy:dy + 8, dx:dx + 8] < 0).astype(np.int64) << i
        cell_index[~cell_known] = 0
        cell_index[top[2]:, :, :] = 0; cell_index[:, top[1]:, :] = 0; cell_index[:, :, top[0]:] = 0
        for lz, ly, lx in zip(*np.nonzero(cell_index)):     # (C order: z slowest, x fastest)
            edges = MC_TABLE[cell_index[lz, ly, lx]]
            for e in range(0, 16, 3):
                if edges[e] == -1:
                    break
                tri = []
                for edge in edges[e:e + 3]:
                    a, b = EDGES[edge]
                    s = np.array([c[0] + lx + CORNERS[a][0], c[1] + ly + CORNERS[a][1], c[2] + lz + CORNERS[a][2]])
                    t = np.array([c[0] + lx + CORNERS[b][0], c[1] + ly + CORNERS[b][1], c[2] + lz + CORNERS[b][2]])
                    v1 = val[lz + CORNERS[a][2], ly + CORNERS[a][1], lx + CORNERS[a][0]]
                    v2 = val[lz + CORNERS[b][2], ly + CORNERS[b][1], lx + CORNERS[b][0]]
                    sp, tp = s.astype(np.float32) * vs, t.astype(np.float32) * vs
                    k = f(0.0 - np.float64(v1))
                    tri.append(sp + (k * (tp - sp)) / (v2 - v1))
                tri = np.concatenate(tri).astype(np.float32)
                if (tri <= 0).any() or (tri > dimf).any():
                    continue
                tris.append(tri)
        out[c] = np.array(tris, np.float32).reshape(-1, 9)
    return out


class MeshSource:
    """A stand-in for DenseSLAMPipeline.mesh_blocks made from a full mesh and the list of allocated blocks: the full mesh split by block,
    filtered by the restated rule.  (What the device entry returns, up to the order within a block.)"""

    def __init__(self, size, dim, width, height):
        self.size, self.dim, self.W, self.H = size, dim, width, height
        self.corners = np.zeros((0, 3), np.int64)
        self.per_block = {}

    def set(self, tris, corners):
        self.per_block = split_by_block(tris, self.size, self.dim)
        self.corners = np.asarray(corners, np.int64).reshape(-1, 3)

    def mesh_blocks(self, region=None, views=None, skip_empty=False):
        sel = np.ones(len(self.corners), bool)
        if views is not None:
            sel = possibly_touched(self.corners, [view_of(v[0], v[1], *(v[2:] if len(v) > 2 else (self.W, self.H))) for v in views], self.size, self.dim)
        if region is not None:
            lo, hi = np.asarray(region[0]), np.asarray(region[1])
            sel &= ((self.corners < hi) & (self.corners + 8 > lo)).all(axis=1)
        coords, ranges, tris, first = [], [], [], 0
        for c in self.corners[sel]:
            t = self.per_block.get(tuple(int(v) for v in c), np.zeros((0, 9), np.float32))
            if skip_empty and len(t) == 0:
                continue
            coords.append(c); ranges.append((first, len(t))); tris.append(t); first += len(t)
        return {"coords": np.array(coords, np.int32).reshape(-1, 3), "ranges": np.array(ranges, np.int64).reshape(-1, 2),
                "triangles": (np.concatenate(tris) if tris else np.zeros((0, 9), np.float32)).reshape(-1, 3, 3)}
