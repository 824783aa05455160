"""The mirrors of the map shift: DenseSLAMSystem::shiftMap on a live handle against the host restatement (include/se/shift_map.hpp) applied to
the getMap() snapshot taken before, compared through a second getMap(), with the poses it moves (tests/cpp/shift_mirror.cpp);
DenseSLAMPipeline.shift moves pose_ the same way; LiveMesh.shift follows the map without meshing it again."""
import numpy as np
import pytest

from supereight_amd.livemesh import LiveMesh
from supereight_amd.pipeline import SDF
from tests.gpu_state_util import bits, run_stream
from tests.mirror_util import build_mirror, run_mirror, write_scene

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag,mu", [("SDF", 0.1), ("OFusion", 0.02)], ids=["sdf", "ofusion"])
def test_shift_map_equals_the_host_restatement(tmp_path, tag, mu):
    exe = build_mirror(tmp_path, "shift_mirror", tag)
    Wm, Hm, N, dim, frames = 320, 240, 256, 4.8, 3
    raw, pf, _ = write_scene(tmp_path, Wm, Hm, dim, frames)
    res, r = run_mirror(exe, [raw, pf, N, dim, mu], timeout=600)
    print(r.stdout, r.stderr)
    assert res["bad"] == 0, r.stderr
    assert res["shifts"] == 5 and res["kept"] > 100 and res["dropped"] > 100 and res["nodes_dropped"] > 10 and res["left"] == 0
    if tag == "OFusion":
        assert res["nodes_kept"] > 0
    assert "not a multiple of 8" in r.stderr          # the refused shift, reported as the mirror reports errors


def test_python_shift_moves_the_pose_with_the_map():
    n, dim = 256, 2.4
    p = run_stream("room", SDF, n, dim, 0, 4)
    try:
        pose = p.pose_.copy()
        handed_out = p.pose_
        s = np.array([-64, 8, 32])
        p.shift(s)
        want = pose.copy()
        want[:3, 3] = pose[:3, 3] + s.astype(np.float32) * (np.float32(dim) / np.float32(n))
        assert (bits(p.pose_) == bits(want)).all()
        assert (handed_out == pose).all() and p.pose_ is not handed_out          # by assignment, not in place
        assert (bits(p.getPose()) == bits(want)).all()
        with pytest.raises(ValueError):
            p.shift([4, 0, 0])
        assert (bits(p.pose_) == bits(want)).all()
    finally:
        p.close()


def test_live_mesh_follows_a_shift():
    n, dim = 256, 2.4
    p = run_stream("room", SDF, n, dim, 0, 6)
    try:
        live = LiveMesh()
        live.update(p)
        had = len(live.blocks)
        s = (48, -64, 0)
        p.shift(s)
        dropped = live.shift(s)
        fresh = LiveMesh()
        fresh.update(p)
        assert had > 100 and 0 < dropped < had and len(live.blocks) == had - dropped
        # what the table holds without any meshing: the entries of the shifted map, the triangles within the rounding of the float32 move
        # (coordinates below dim = 2.4 m: an ulp is at most 2^-22 m), except the blocks that now lie on the faces the content moved towards:
        # the upper x face (the neighbour left) and the lower y face (the mesher rejects triangles with a vertex at coordinate 0)
        inner = [c for c in fresh.blocks if c[0] < n - 8 and c[1] >= 8]
        assert set(inner) <= set(live.blocks) and len(inner) > 100
        for c in inner:
            assert live.blocks[c].shape == fresh.blocks[c].shape and np.abs(live.blocks[c] - fresh.blocks[c]).max() <= 2.0 ** -21, c
        # ... the two slabs the documentation asks for bring the table to the fresh one's entries
        slabbed = LiveMesh()
        slabbed.blocks, slabbed.size, slabbed.voxel = dict(live.blocks), live.size, live.voxel
        slabbed.update(p, region=((n - 9, 0, 0), (n, n, n)))
        slabbed.update(p, region=((0, 0, 0), (n, 8, n)))
        assert sorted(slabbed.blocks) == sorted(fresh.blocks)
        assert all(slabbed.blocks[c].shape == fresh.blocks[c].shape for c in fresh.blocks)
        # ... and after an update over the vacated side and everything else the triangles are equal bit for bit
        live.update(p, region=((0, 0, 0), (n, n, n)))
        assert sorted(live.blocks) == sorted(fresh.blocks)
        assert (bits(live.triangles()) == bits(fresh.triangles())).all() and len(fresh.triangles()) > 1000
    finally:
        p.close()
