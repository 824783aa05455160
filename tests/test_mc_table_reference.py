"""Pin of include/se_mc_table.h: case by case the same triangles, in the same order and orientation, as the reference's
triTable (se_core/include/se/algorithms/edge_tables.h:66).  The reference's 256 x 16 literals are stored as a data fixture,
tests/golden/mc_tri_table_i8.npy (-1 = no further edge), so the check needs no reference checkout."""
import os

import numpy as np

from tests.test_mesh_export import load_table

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "mc_tri_table_i8.npy")


def test_triangle_table_equals_the_reference_literals():
    ref = np.load(GOLDEN).astype(np.int64)
    assert ref.shape == (256, 16)
    assert (load_table() == ref).all()
