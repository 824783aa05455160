"""DenseSLAMSystem::collidesOriented on a live handle against the host restatement (include/se/oriented_collision.hpp) on the getMap()
snapshot: box for box, a sample also against the brute-force definition, and the mirror's rounding helper against the plain one
(tests/cpp/oriented_mirror.cpp)."""
import pytest

from tests.mirror_util import build_mirror, run_mirror, write_scene

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag,mu", [("SDF", 0.1), ("OFusion", 0.02)], ids=["sdf", "ofusion"])
def test_collides_oriented_equals_the_host_restatement(tmp_path, tag, mu):
    exe = build_mirror(tmp_path, "oriented_mirror", tag)
    Wm, Hm, N, dim, frames = 320, 240, 256, 4.8, 3
    raw, pf, _ = write_scene(tmp_path, Wm, Hm, dim, frames)
    res, r = run_mirror(exe, [raw, pf, N, dim, mu], timeout=600)
    print(r.stdout, r.stderr)
    assert res["bad"] == 0, r.stderr
    assert res["checked"] >= 2000 and res["brute"] == 400
    assert res["rounded"] == res["rotated"] == 2000
    assert res["occupied"] > 0 and res["unseen"] > 0 and res["empty"] > 0 and res["invalid"] >= 3
