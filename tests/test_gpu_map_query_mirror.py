"""DenseSLAMSystem::queryMap (the C++ mirror, include/se/DenseSLAMSystem.h) against the host se::Octree that getMap() materialises from
the same device map: tests/cpp/map_query_mirror.cpp, compiled with g++ -ffp-contract=off and linked to libse_hip.so, runs a 640x480
SLAMBench .raw stream into a 512^3 volume and compares x and y of get_fine / get, interp and grad bit for bit."""
import pytest

from tests.mirror_util import build_mirror, run_mirror, write_scene

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag,mu", [("SDF", 0.1), ("OFusion", 0.02)], ids=["sdf", "ofusion"])
def test_query_map_equals_the_host_octree(tmp_path, tag, mu):
    exe = build_mirror(tmp_path, "map_query_mirror", tag)
    W, H, N, dim, frames = 640, 480, 512, 4.8, 3
    raw, pf, _ = write_scene(tmp_path, W, H, dim, frames)
    res, r = run_mirror(exe, [raw, pf, N, dim, mu], timeout=300)
    assert res["bad"] == 0, r.stderr
    assert res["checked"] > 5000 and 0 < res["allocated"] < res["in_volume"] < res["checked"]
    assert 0 < res["observed"] < res["checked"]
    if tag == "OFusion":
        assert res["coarse_node"] > 0      # Octree::get answered from a coarse node somewhere
