"""DenseSLAMSystem::editMap on a live handle against the host edit-list function (include/se/axis_aligned.hpp) applied to the getMap()
snapshot taken before, both modes, compared through a second getMap() (tests/cpp/edit_mirror.cpp)."""
import pytest

from tests.mirror_util import build_mirror, run_mirror, write_scene

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag,mu", [("SDF", 0.1), ("OFusion", 0.02)], ids=["sdf", "ofusion"])
def test_edit_map_equals_the_host_edit_list(tmp_path, tag, mu):
    exe = build_mirror(tmp_path, "edit_mirror", tag)
    Wm, Hm, N, dim, frames = 320, 240, 256, 4.8, 3
    raw, pf, _ = write_scene(tmp_path, Wm, Hm, dim, frames)
    res, r = run_mirror(exe, [raw, pf, N, dim, mu], timeout=600)
    print(r.stdout, r.stderr)
    assert res["bad"] == 0, r.stderr
    assert res["edits"] > 400 and res["voxels"] > 0 and res["nodes"] > 0 and res["blocks"] > 0 and res["changed"] > 0
    assert res["invalid"] == (10 if tag == "SDF" else 8)          # four per list, and for SDF the weight that is not a byte
