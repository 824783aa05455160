"""DenseSLAMSystem::collidesOrientedMoving on a live handle against the host restatement (include/se/oriented_motion.hpp) on the getMap()
snapshot: motion for motion and for both stop_at on status, the reduced t_exact pair and the bits of t_first, a sample also against the
brute-force definition, and the mirror's rounding helper against the plain one (tests/cpp/oriented_motion_mirror.cpp)."""
import pytest

from tests.mirror_util import build_mirror, run_mirror, write_scene

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag,mu", [("SDF", 0.1), ("OFusion", 0.02)], ids=["sdf", "ofusion"])
def test_collides_oriented_moving_equals_the_host_restatement(tmp_path, tag, mu):
    exe = build_mirror(tmp_path, "oriented_motion_mirror", tag)
    Wm, Hm, N, dim, frames = 320, 240, 256, 4.8, 3
    raw, pf, _ = write_scene(tmp_path, Wm, Hm, dim, frames)
    res, r = run_mirror(exe, [raw, pf, N, dim, mu], timeout=600)
    print(r.stdout, r.stderr)
    assert res["bad"] == 0, r.stderr
    assert res["checked"] >= 1600 and res["brute"] == 300
    assert res["rounded"] == res["rotated"] == 1500
    assert res["occupied"] > 0 and res["unseen"] > 0 and res["empty"] > 0 and res["invalid"] >= 3 and res["blocked"] > 20 and res["free"] > 20
