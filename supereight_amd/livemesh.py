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

    def update(self, source, views=None, region=None) -> int:
        """Brings the blocks up to date that `views` (the views integrated since the last update: (pose, k) or (pose, k, width, height)) may
        have touched within `region`.  `source` has mesh_blocks(region=, views=, skip_empty=) as DenseSLAMPipeline has.  With no views, or
        more than 64 of them, the region alone decides.  Returns the number of blocks replaced or deleted.
        After DenseSLAMPipeline.edit / reset the blocks of the edited box changed without any view: update(source, region=(lo - 1, hi)) --
        no views; lo - 1 because a block's cells also read the first voxel layer of the next block."""
        views = None if views is None else list(views)
        if views is not None and (len(views) == 0 or len(views) > MAX_VIEWS):
            views = None
        res = source.mesh_blocks(region=region, views=views, skip_empty=False)
        coords, ranges, tris = (np.asarray(res[k]) for k in ("coords", "ranges", "triangles"))
        for c, (first, count) in zip(coords.tolist(), ranges.tolist()):
            if count:
                self.blocks[tuple(c)] = tris[first:first + count].copy()
            else:
                self.blocks.pop(tuple(c), None)
        return len(coords)

    def triangles(self) -> np.ndarray:
        """All triangles, [n, 3, 3] float32 metres, blocks in coordinate order."""
        if not self.blocks:
            return np.empty((0, 3, 3), np.float32)
        return np.concatenate([self.blocks[c] for c in sorted(self.blocks)])
