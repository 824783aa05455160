"""A mesh that follows the resident map block by block (DenseSLAMPipeline.mesh_blocks, se_hip_mesh_blocks of include/se_hip.h).

``LiveMesh`` holds {block corner (voxels) -> that block's triangles}.  ``update(source, views)`` asks the source for the blocks the views may
have touched and replaces exactly those: a block that comes back with triangles replaces its entry, one that comes back empty is deleted,
every other entry stays.  A receiver (a viewer, a mesh publisher) sees the same stream of per-block replacements.
"""
from __future__ import annotations

import numpy as np

MAX_VIEWS = 64   # SE_HIP_MESH_MAX_VIEWS


class LiveMesh:
    def __init__(self):
        self.blocks = {}   # (x, y, z) voxel coordinates of the block corner -> [n, 3, 3] float32
        self.size = self.voxel = None   # the volume's side in voxels and the voxel's in metres, learnt from the source of the first update

    def update(self, source, views=None, region=None) -> int:
        """Brings the blocks up to date that `views` (the views integrated since the last update: (pose, k) or (pose, k, width, height)) may
        have touched within `region`.  `source` has mesh_blocks(region=, views=, skip_empty=) as DenseSLAMPipeline has.  With no views, or
        more than 64 of them, the region alone decides.  Returns the number of blocks replaced or deleted.
        After DenseSLAMPipeline.edit / reset the blocks of the edited box changed without any view: update(source, region=(lo - 1, hi)) --
        no views; lo - 1 because a block's cells also read the first voxel layer of the next block."""
        views = None if views is None else list(views)
        if views is not None and (len(views) == 0 or len(views) > MAX_VIEWS):
            views = None
        if getattr(source, "size", None):
            self.size, self.voxel = int(source.size), np.float32(source.dim) / np.float32(source.size)
        res = source.mesh_blocks(region=region, views=views, skip_empty=False)
        coords, ranges, tris = (np.asarray(res[k]) for k in ("coords", "ranges", "triangles"))
        for c, (first, count) in zip(coords.tolist(), ranges.tolist()):
            if count:
                self.blocks[tuple(c)] = tris[first:first + count].copy()
            else:
                self.blocks.pop(tuple(c), None)
        if views is None and self.blocks:
            # the region alone decided: every block of the map that intersects it was listed, so an entry there that was not is of a block
            # the map no longer holds (DenseSLAMPipeline.release handed it back)
            listed = set(map(tuple, coords.tolist()))
            lo, hi = ((0, 0, 0), (self.size or 0,) * 3) if region is None else (tuple(int(v) for v in region[0]), tuple(int(v) for v in region[1]))
            gone = [c for c in self.blocks if c not in listed and all(c[k] < hi[k] and c[k] + 8 > lo[k] for k in range(3))]
            for c in gone:
                del self.blocks[c]
            return len(coords) + len(gone)
        return len(coords)

    def shift(self, shift_voxels) -> int:
        """Follows DenseSLAMPipeline.shift(shift_voxels) (three integers, multiples of 8): every entry moves by s, its triangles by s * voxel
        metres (a float32 addition: within an ulp of what meshing the shifted map gives), and what left the cube is dropped -- the map is
        not meshed again.  What still has to be are the blocks that now lie on a face the content moved towards: on an upper face a block
        lost the neighbour its last cells read, on a lower face the mesher rejects triangles with a vertex at coordinate 0.  So for every
        axis k follow with update(source, region=(lo, hi)) over the slab [size - 9, size) of that axis if s[k] > 0, [0, 8) if s[k] < 0.
        Returns the number of entries dropped."""
        from .pipeline import DenseSLAMPipeline
        s = DenseSLAMPipeline._shift_argument(shift_voxels).astype(np.int64)
        if not self.blocks or not s.any():
            return 0
        if self.size is None:
            raise ValueError("LiveMesh.shift: the volume is not known yet (no update from a pipeline so far)")
        move = s.astype(np.float32) * self.voxel
        kept = {}
        for c, tris in self.blocks.items():
            q = np.asarray(c, np.int64) + s
            if (q >= 0).all() and (q <= self.size - 8).all():
                kept[tuple(int(v) for v in q)] = tris + move
        dropped = len(self.blocks) - len(kept)
        self.blocks = kept
        return dropped

    def triangles(self) -> np.ndarray:
        """All triangles, [n, 3, 3] float32 metres, blocks in coordinate order."""
        if not self.blocks:
            return np.empty((0, 3, 3), np.float32)
        return np.concatenate([self.blocks[c] for c in sorted(self.blocks)])
