"""What the map-query tests share: the device map as downloaded with the oracle's octree built from it (answers of get_fine / get / interp /
grad / status for arbitrary points), and the bit-for-bit comparison of query outputs."""
import ctypes as C

import numpy as np

from supereight_amd.pipeline import OFUSION, SDF
from tests.host_util import decode, morton

N, DIM = 256, 2.4
INIT = {SDF: (1.0, 0.0), OFUSION: (0.0, 0.0)}    # voxel_traits<T>::initValue(); empty().x equals initValue().x for both


class Map:
    """The device map as downloaded, with the oracle's octree (FTree) built from it (a map of n^3 voxels over dim metres)."""

    def __init__(self, oracle, p, field, n=N, dim=DIM):
        self.lib, self.field = oracle, field
        self.N, self.dim = n, dim
        self.coords, self.x, self.y, _ = p.blocks()
        self.ncode, _, self.nx, self.ny = p.nodes()
        self.row = {tuple(int(v) for v in c): i for i, c in enumerate(self.coords)}
        self.nrow = {int(c): i for i, c in enumerate(self.ncode)}
        self.init = INIT[field]
        self.max_level = n.bit_length() - 1
        t = oracle.so_ft_create(n, dim, self.init[0], self.init[0])
        code, co, isb = C.c_uint64(0), np.zeros(3, np.int32), C.c_int(0)
        for c in sorted(self.ncode, key=lambda k: int(k) & 0x1FF):
            x, y, z, lvl = decode(c)
            if lvl:
                oracle.so_ft_insert(t, x, y, z, lvl, C.byref(code), co, C.byref(isb))
                assert int(code.value) == int(c)
        for i, c in enumerate(self.ncode):
            x, y, z, lvl = decode(c)
            for j in range(8):
                assert oracle.so_ft_set_octant_value(t, x, y, z, lvl, j, float(self.nx[i, j]))
        init_bits = np.float32(self.init[0]).view(np.uint32)
        for i, (bx, by, bz) in enumerate(self.coords):
            oracle.so_ft_insert(t, int(bx), int(by), int(bz), -1, C.byref(code), co, C.byref(isb))
            assert isb.value == 1 and tuple(co) == (bx, by, bz)
            for v in np.nonzero(self.x[i].view(np.uint32) != init_bits)[0]:
                oracle.so_ft_set(t, int(bx) + int(v & 7), int(by) + int((v >> 3) & 7), int(bz) + int(v >> 6), float(self.x[i, v]))
        self.t = t

    def close(self):
        self.lib.so_ft_destroy(self.t)

    def allocated(self, bx, by, bz):
        return (bx * 8, by * 8, bz * 8) in self.row

    def expected(self, pts):
        """Oracle answers for float32 points [n, 3] in metres."""
        lib, t, N = self.lib, self.t, self.N
        s = np.float32(N) / np.float32(self.dim)
        q = (s * pts).astype(np.float32)
        n = len(pts)
        fine, coarse = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
        interp, grad, status = np.zeros(n, np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
        g = np.zeros(3, np.float32)
        leaf = self.max_level - 3
        for i in range(n):
            qx, qy, qz = (float(v) for v in q[i])
            v = [int(a) for a in q[i]]        # (int) truncation
            x, y, z = v
            fine[i, 0] = lib.so_ft_get_fine(t, x, y, z)
            coarse[i, 0] = lib.so_ft_get(t, x, y, z)
            interp[i] = lib.so_ft_interp(t, qx, qy, qz)
            lib.so_ft_grad(t, qx, qy, qz, g)
            grad[i] = g
            fine[i, 1] = coarse[i, 1] = self.init[1]
            st = 0
            if all(0 <= a < N for a in v):
                st |= 1
                r = self.row.get((x & ~7, y & ~7, z & ~7))
                if r is not None:
                    st |= 2
                    fine[i, 1] = coarse[i, 1] = self.y[r, (x & 7) + 8 * (y & 7) + 64 * (z & 7)]
                else:
                    parent = self.nrow[0]
                    for lvl in range(1, leaf + 1):
                        side = N >> lvl
                        key = morton(x & ~(side - 1), y & ~(side - 1), z & ~(side - 1)) | lvl
                        if lvl < leaf and key in self.nrow:
                            parent = self.nrow[key]
                            continue
                        child = int((x & side) > 0) + 2 * int((y & side) > 0) + 4 * int((z & side) > 0)
                        coarse[i, 1] = self.ny[parent, child]
                        break
            lo = [max(int(np.floor(a)), 0) for a in q[i]]
            cross = [(a & 7) == 7 for a in lo]
            ok = True
            for k in range(8):
                d = (k & 1, (k >> 1) & 1, k >> 2)
                if all(cross[a] or d[a] == 0 for a in range(3)):
                    b = [(lo[a] + d[a]) >> 3 for a in range(3)]
                    ok = ok and all(0 <= c < N // 8 for c in b) and self.allocated(*b)
            st |= 4 if ok else 0
            status[i] = st
        return {"fine": fine, "coarse": coarse, "interp": interp, "grad": grad, "status": status}

    def points(self, p, rng):
        """Random points in the volume, jittered raycast hits, block faces / edges / corners, points next to missing blocks, and
        points just outside each face of the volume (metres, float32)."""
        N, DIM = self.N, self.dim
        vox = np.float32(DIM) / np.float32(N)
        sets = [rng.uniform(0, DIM, (600, 3))]
        v, nrm = p.vertex_normal()
        hits = v[nrm[..., 0] != -2]
        assert len(hits) > 100
        sets.append(hits[rng.choice(len(hits), 600)] + rng.uniform(-2, 2, (600, 3)) * vox)
        blocks = self.coords[rng.choice(len(self.coords), min(60, len(self.coords)), replace=False)].astype(np.float64)
        for off in ((7.5, 3.2, 4.1), (7.5, 7.5, 2.6), (7.5, 7.5, 7.5), (8.0, 8.0, 8.0), (7.999, 0.0, 7.999), (-0.001, 4.0, 4.0), (3.3, -0.5, 7.2)):
            sets.append((blocks + np.asarray(off)) * vox)
        near = []
        for bx, by, bz in blocks.astype(int):
            for d in ((8, 0, 0), (-8, 0, 0), (0, 8, 0), (0, -8, 0), (0, 0, 8), (0, 0, -8)):
                c = (bx + d[0], by + d[1], bz + d[2])
                if c not in self.row and all(0 <= a < N for a in c):
                    near.append(np.asarray(c) + rng.uniform(-1.5, 9.5, 3))
        assert near
        sets.append(np.asarray(near) * vox)
        for face in range(6):
            u = rng.uniform(0, N, (30, 3))
            u[:, face // 2] = N + rng.uniform(0, 1.5, 30) if face & 1 else -rng.uniform(0, 1.5, 30)
            sets.append(u * vox)
        return np.ascontiguousarray(np.concatenate(sets).astype(np.float32))


def compare(got, exp, what=("fine", "coarse", "interp", "grad", "status")):
    for k in what:
        a, b = got[k], exp[k]
        if a.dtype == np.float32:
            bad = np.nonzero((a.view(np.uint32) != b.view(np.uint32)).reshape(len(a), -1).any(axis=1))[0]
        else:
            bad = np.nonzero(a != b)[0]
        assert bad.size == 0, (k, bad[:5], a[bad[:5]], b[bad[:5]])
