"""DenseSLAMSystem::distanceField on a live handle against the literal definition (include/se/distance_field.hpp) on the getMap() snapshot:
d2 and the nearest voxel of every voxel of every request, for both stop_at values (tests/cpp/field_mirror.cpp)."""
import pytest

from tests.mirror_util import build_mirror, run_mirror, write_scene

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag,mu", [("SDF", 0.1), ("OFusion", 0.02)], ids=["sdf", "ofusion"])
def test_distance_field_equals_the_definition(tmp_path, tag, mu):
    exe = build_mirror(tmp_path, "field_mirror", tag)
    Wm, Hm, N, dim, frames = 320, 240, 256, 4.8, 3
    raw, pf, _ = write_scene(tmp_path, Wm, Hm, dim, frames)
    res, r = run_mirror(exe, [raw, pf, N, dim, mu], timeout=600)
    print(r.stdout, r.stderr)
    assert res["bad"] == 0, r.stderr
    assert res["requests"] == 28 and res["voxels"] > 500
    assert res["touching"] > 0 and res["apart"] > 0 and res["none"] > 0 and res["outside"] > 0
