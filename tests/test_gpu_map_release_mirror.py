"""The C++ mirror of the release: DenseSLAMSystem::releaseMap on a live handle against the host restatement (include/se/release_map.hpp)
applied to the getMap() snapshot taken before, compared through a second getMap() (tests/cpp/release_mirror.cpp)."""
import pytest

from tests.mirror_util import build_mirror, run_mirror, write_scene

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag,mu", [("SDF", 0.1), ("OFusion", 0.02)], ids=["sdf", "ofusion"])
def test_release_map_equals_the_host_restatement(tmp_path, tag, mu):
    exe = build_mirror(tmp_path, "release_mirror", tag)
    Wm, Hm, N, dim, frames = 320, 240, 256, 4.8, 3
    raw, pf, _ = write_scene(tmp_path, Wm, Hm, dim, frames)
    res, r = run_mirror(exe, [raw, pf, N, dim, mu], timeout=600)
    print(r.stdout, r.stderr)
    assert res["bad"] == 0, r.stderr
    assert res["calls"] == 5 and res["unseen_only"] >= 5 and res["observed"] > 100 and res["nodes_released"] > 10 and res["left"] == 0
    assert res["released"] > res["observed"] and res["kept"] > res["released"]
    assert "a side below 1" in r.stderr               # the refused record, reported as the mirror reports errors
