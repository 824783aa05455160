"""The oriented box kernel on the frontier descent (supereight_amd/csrc/se_frontier.h) at its limits, on the shapes of test_gpu_frontier.py:
maps with every block allocated and every voxel empty, and boxes that nothing blocks, so the kernel must expand the whole pyramid.
  64^3    the level above the blocks holds all 64 octants at once: the capacity of a frontier level.
  128^3   a full level is drained 8 at a time while the level below is filled to 64 each time.
The axis-aligned box that is exactly the volume answers empty; a 3-4-5-rotated box that contains the volume answers unseen.  Then the single
voxel (N-1, N-1, N-1) -- in the last block in Morton order -- is set occupied and both answer occupied.  Each is asked once and as 130 copies;
at 64^3, 2^20 + 130 boxes -- more than the grid has waves -- make the first 130 waves root their frontier a second time."""
import numpy as np
import pytest

from supereight_amd.pipeline import COLLISION_EMPTY, COLLISION_OCCUPIED, COLLISION_UNSEEN, SDF, DenseSLAMPipeline
from tests.gpu_state_util import H, W
from tests.motion_util import EMPTY, OCC, class_grid
from tests.oriented_util import SUB, touched_cubes, valid

pytestmark = pytest.mark.gpu

OCCUPIED_X, EMPTY_X = -0.5, 0.5      # SDF, threshold 0: occupied below it


def _queries(n):
    """The volume itself, and a box turned by the 3-4-5 angle about z that contains it: a square of half side 15 n sub-units holds the
    axis-aligned one of half side 8 n (it needs 8 n * 7 / 5 = 11.2 n), and it is taller than the volume by half a voxel each way."""
    c, h = SUB * n // 2, SUB * n // 2
    whole = [c, c, c, h, 0, 0, 0, h, 0, 0, 0, h]
    turned = [c, c, c, 12 * n, 9 * n, 0, -9 * n, 12 * n, 0, 0, 0, h + 8]
    return np.array([whole, turned], np.int32)


@pytest.mark.parametrize("n,max_blocks", [(64, 0), (64, 1024), (128, 0), (128, 8192)], ids=["64_dense", "64_pooled", "128_dense", "128_pooled"])
def test_full_pyramid_of_empty_blocks(n, max_blocks):
    dim = 0.02 * n
    boxes = _queries(n)
    assert all(valid(b) for b in boxes)
    # what the definition says: the first touches every voxel of the volume and none outside, the second every voxel and some outside
    for b, reach in zip(boxes, (0, 1)):
        t = touched_cubes(b, (-1, -1, -1), (n + 2, n + 2, n + 2))
        assert t[1:-1, 1:-1, 1:-1].all() and bool(t[0].any() or t[-1].any()) == bool(reach)
        assert bool(t[:, 0].any() or t[:, -1].any() or t[:, :, 0].any() or t[:, :, -1].any()) == bool(reach)
    p = DenseSLAMPipeline((W, H), n, dim, field_type=SDF, max_blocks=max_blocks)
    try:
        whole = np.array([[0, 0, 0, n, n, n]], np.int32)
        assert int(p.allocate(whole)[0]) == (n // 8) ** 3
        p.edit(whole, EMPTY_X, 1.0)
        for corner in (False, True):
            grid = np.full((n, n, n), EMPTY, np.uint8)
            if corner:
                p.edit(np.array([[n - 1, n - 1, n - 1, n, n, n]], np.int32), OCCUPIED_X, 1.0)
                grid[n - 1, n - 1, n - 1] = OCC
            assert (class_grid(p, n, dim, 0.0, False).cpu().numpy() == grid).all()
            exp = np.array([COLLISION_OCCUPIED, COLLISION_OCCUPIED] if corner else [COLLISION_EMPTY, COLLISION_UNSEEN], np.uint8)
            assert (p.collides_oriented(boxes) == exp).all()
            assert (p.collides_oriented(np.ascontiguousarray(np.tile(boxes, (130, 1)))) == np.tile(exp, 130)).all()
        if n == 64:   # more boxes than the grid has waves: the first 130 waves root the frontier a second time, after a full expansion
            m = (1 << 20) + 130
            inside = [8, 8, 8, 4, 3, 0, -3, 4, 0, 0, 0, 5]                       # wholly inside voxel (0, 0, 0)
            many = np.ascontiguousarray(np.tile(np.array([inside], np.int32), (m, 1)))
            many[:130] = boxes[0]
            many[-130:] = boxes[0]
            st = p.collides_oriented(many)
            assert (st[:130] == COLLISION_OCCUPIED).all() and (st[-130:] == COLLISION_OCCUPIED).all() and (st[130:-130] == COLLISION_EMPTY).all()
    finally:
        p.close()
