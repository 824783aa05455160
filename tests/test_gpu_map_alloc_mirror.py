"""DenseSLAMSystem::allocateRegion on a live handle against the host restatement (include/se/allocate_region.hpp) applied to the getMap()
snapshot taken before, compared through a second getMap() (tests/cpp/alloc_mirror.cpp)."""
import pytest

from tests.mirror_util import build_mirror, run_mirror, write_scene

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag,mu", [("SDF", 0.1), ("OFusion", 0.02)], ids=["sdf", "ofusion"])
def test_allocate_region_equals_the_host_restatement(tmp_path, tag, mu):
    exe = build_mirror(tmp_path, "alloc_mirror", tag)
    Wm, Hm, N, dim, frames = 320, 240, 256, 4.8, 3
    raw, pf, _ = write_scene(tmp_path, Wm, Hm, dim, frames)
    res, r = run_mirror(exe, [raw, pf, N, dim, mu], timeout=600)
    print(r.stdout, r.stderr)
    assert res["bad"] == 0, r.stderr
    assert res["boxes"] > 120 and res["blocks"] > 100 and res["nodes"] > 10 and res["pairs"] > res["blocks"] and res["keys"] > 0
    assert res["invalid"] == 4 and res["again"] == 0
