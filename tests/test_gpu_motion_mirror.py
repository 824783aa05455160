"""DenseSLAMSystem::collidesMoving on a live handle against the host restatement (include/se/motion_collision.hpp) on the getMap() snapshot:
status and the bits of t_first for both stop_at values, a sample also against the brute-force definition (tests/cpp/motion_mirror.cpp)."""
import pytest

from tests.mirror_util import build_mirror, run_mirror, write_scene

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag,mu", [("SDF", 0.1), ("OFusion", 0.02)], ids=["sdf", "ofusion"])
def test_collides_moving_equals_the_host_restatement(tmp_path, tag, mu):
    exe = build_mirror(tmp_path, "motion_mirror", tag)
    Wm, Hm, N, dim, frames = 320, 240, 256, 4.8, 3
    raw, pf, _ = write_scene(tmp_path, Wm, Hm, dim, frames)
    res, r = run_mirror(exe, [raw, pf, N, dim, mu], timeout=600)
    print(r.stdout, r.stderr)
    assert res["bad"] == 0, r.stderr
    assert res["checked"] > 1800 and res["brute"] == 300
    assert res["occupied"] > 0 and res["unseen"] > 0 and res["empty"] > 0
    assert res["start"] > 0 and res["partial"] > 0 and res["free"] > 0
