"""The frontier descent that the box, motion and clearance kernels share (supereight_amd/csrc/se_frontier.h), at its limits and at the
smallest shapes that reach them: maps with every block allocated and every voxel empty, and queries that nothing blocks and nothing prunes,
so each kernel must expand the whole pyramid.
  64^3    the level above the blocks holds all 64 octants at once: the capacity of a frontier level.
  128^3   a full level is drained 8 at a time while the level below is filled to 64 each time: the "next level is empty when it is filled"
          argument.
Then the single voxel (N-1, N-1, N-1) -- in the last block in Morton order -- is set occupied and everything is asked again.  Every query goes
once in a handful and once as 130 copies (130 waves); the re-rooting of the frontier by a wave's second query needs more queries than the
grid has waves, 2^20, and is asked of the box query in reference mode, whose search ends at the first block.  Everything is integer or an
exact rational: every comparison is equality."""
import functools
import math

import numpy as np
import pytest

from supereight_amd.pipeline import CLEARANCE_NONE, COLLISION_EMPTY, MOTION_FREE, SDF, DenseSLAMPipeline
from tests.clearance_util import I32_MIN, clearance_truth
from tests.gpu_state_util import H, W
from tests.motion_util import EMPTY, FREE, OCC, as_float32, class_grid, motion_truth
from tests.test_gpu_collision import _strict_truth

pytestmark = pytest.mark.gpu

OCCUPIED_X, EMPTY_X = -0.5, 0.5      # SDF, threshold 0: occupied below it


def _queries(n):
    h = n // 2
    boxes = np.array([[0, 0, 0, n, n, n]], np.int32)
    # the half volume swept along x over the other half; the low octant moved diagonally onto the high one; the whole volume at rest
    motions = np.array([[0, 0, 0, h, n, n, h, 0, 0], [0, 0, 0, h, h, h, h, h, h], [0, 0, 0, n, n, n, 0, 0, 0]], np.int32)
    # from the corner voxel: beyond the volume's diagonal, and half way
    clear = np.array([[0, 0, 0, 1, 1, 1, math.ceil(math.sqrt(3.0) * n) + 1], [0, 0, 0, 1, 1, 1, h]], np.int32)
    return boxes, motions, clear


def _grid(n, corner):
    g = np.full((n, n, n), EMPTY, np.uint8)
    if corner:
        g[n - 1, n - 1, n - 1] = OCC
    return g


@functools.lru_cache(maxsize=None)
def _expected(n, corner):
    """The answers over the class grid of the map: computed once per size, shared by the dense and the pooled case."""
    boxes, motions, clear = _queries(n)
    if not corner:   # nothing blocks
        none = np.full((len(clear), 3), I32_MIN, np.int32)
        return dict(strict=np.full(len(boxes), COLLISION_EMPTY, np.uint8), status=np.full(len(motions), COLLISION_EMPTY, np.uint8),
                    t={s: np.full(len(motions), MOTION_FREE, np.float32) for s in ("occupied", "unseen")},
                    d2=np.full(len(clear), CLEARANCE_NONE, np.int32), near=none)
    g = _grid(n, corner)
    mt = [motion_truth(g, m) for m in motions.tolist()]
    ct = [clearance_truth(g, q, OCC) for q in clear.tolist()]
    assert mt[0][1] == mt[1][1] != FREE and mt[2][1] == 0 and ct[0][0] == 3 * (n - 2) ** 2 and ct[1][0] == CLEARANCE_NONE
    return dict(strict=_strict_truth(g, boxes, n), status=np.array([t[0] for t in mt], np.uint8),
                t={"occupied": np.array([as_float32(t[1]) for t in mt], np.float32), "unseen": np.array([as_float32(t[2]) for t in mt], np.float32)},
                d2=np.array([t[0] for t in ct], np.int32), near=np.array([t[1] for t in ct], np.int32))


def _ask(p, n, exp, copies):
    boxes, motions, clear = (np.ascontiguousarray(np.tile(q, (copies, 1))) for q in _queries(n))
    tile = lambda a: np.tile(a, (copies,) + (1,) * (a.ndim - 1))
    assert (p.collides(boxes, mode="strict") == tile(exp["strict"])).all()
    # reference mode: a visited leaf replaces the running status and the last one visited is the block of smallest Morton code (DESIGN.md
    # 4.7) -- block 0, which is empty whatever the last block holds; no child is absent, so no node raises an event
    assert (p.collides(boxes, mode="reference") == COLLISION_EMPTY).all()
    for stop in ("occupied", "unseen"):
        status, t = p.collides_moving(motions, stop_at=stop)
        assert (status == tile(exp["status"])).all() and (t == tile(exp["t"][stop])).all(), (stop, status[:3], t[:3])
        assert (p.collides_moving(motions, stop_at=stop, t_first=False) == tile(exp["status"])).all()
    d2, near = p.clearance(clear[:, :6], clear[:, 6], stop_at="occupied")
    assert (d2 == tile(exp["d2"])).all() and (near == tile(exp["near"])).all(), (d2[:2], near[:2])
    assert (p.clearance(clear[:, :6], clear[:, 6], stop_at="occupied", nearest=False) == tile(exp["d2"])).all()


@pytest.mark.parametrize("n,max_blocks", [(64, 0), (64, 1024), (128, 0), (128, 8192)], ids=["64_dense", "64_pooled", "128_dense", "128_pooled"])
def test_full_pyramid_of_empty_blocks(n, max_blocks):
    dim = 0.02 * n
    p = DenseSLAMPipeline((W, H), n, dim, field_type=SDF, max_blocks=max_blocks)
    try:
        whole = np.array([[0, 0, 0, n, n, n]], np.int32)
        assert int(p.allocate(whole)[0]) == (n // 8) ** 3
        p.edit(whole, EMPTY_X, 1.0)
        for corner in (False, True):
            if corner:
                p.edit(np.array([[n - 1, n - 1, n - 1, n, n, n]], np.int32), OCCUPIED_X, 1.0)
            assert (class_grid(p, n, dim, 0.0, False).cpu().numpy() == _grid(n, corner)).all()
            exp = _expected(n, corner)
            _ask(p, n, exp, 1)
            _ask(p, n, exp, 130)
        if n == 64:   # more boxes than the grid has waves: the first 130 waves root the frontier a second time
            many = np.ascontiguousarray(np.tile(whole, ((1 << 20) + 130, 1)))
            assert (p.collides(many, mode="reference") == COLLISION_EMPTY).all()
    finally:
        p.close()
