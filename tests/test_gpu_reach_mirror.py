"""DenseSLAMSystem::reachField on a live handle against the literal definition (include/se/reach_field.hpp) on the getMap() snapshot: steps,
seed, next and the counts of every position of every request, for both stop_at values (tests/cpp/reach_mirror.cpp)."""
import pytest

from tests.mirror_util import build_mirror, run_mirror, write_scene

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag,mu", [("SDF", 0.1), ("OFusion", 0.02)], ids=["sdf", "ofusion"])
def test_reach_field_equals_the_definition(tmp_path, tag, mu):
    exe = build_mirror(tmp_path, "reach_mirror", tag)
    Wm, Hm, N, dim, frames = 320, 240, 128, 2.4, 3
    raw, pf, _ = write_scene(tmp_path, Wm, Hm, dim, frames)
    res, r = run_mirror(exe, [raw, pf, N, dim, mu], timeout=600)
    print(r.stdout, r.stderr)
    assert res["bad"] == 0 and res["late"] == 0, r.stderr
    assert res["requests"] == 28 and res["positions"] > 100000
    assert res["blocked"] > 0 and res["reached"] > 0 and res["outside"] > 0
