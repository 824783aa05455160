"""The raycast seen from beyond every face of the volume, against the oracle bit for bit.  Each 8x8 tile's first-leaf search starts at
se_beam_start's t_safe, and a beam sample just outside the volume must count as occupied when the boundary cell it touches has its dilated bit set.
That shell test once accepted only the cells beyond the lower faces: from outside +x / +y / +z a tile could start inside a boundary cell, behind
the blocks there (the CPU model of the same arithmetic, ray by ray: tests/test_first_leaf_equivalence.py::test_beam_start_from_beyond_every_face).
Here the HIP path renders the same sweep of cameras -- the eager raycast, the deferred one that rides in the next frame's fused k_raycast_scan, a
pooled map, and the three settings of the beam-start knob -- and every image must be the oracle's.  The sweep also reaches hits up to a voxel
beyond an upper face, whose normals need the per-voxel gradient (se_hit_grad, se_sample.h)."""
import numpy as np
import pytest

from oracle.binding import SDF, OraclePipeline
from supereight_amd.pipeline import DenseSLAMPipeline
from supereight_amd.synthetic import make_stream
from tests.parity_util import OUTSIDE_VIEWS, compare_maps, compare_raycast, outside_view

pytestmark = pytest.mark.gpu

DIM, MU, FRAMES = 4.8, 0.1, 6
# camera offsets beyond the face, as fractions of the edge (a coarse cell is 1/32 of it): from inside the shell out to ~10 coarse cells
OFFSETS = [i * 0.0125 for i in range(1, 25)]
# name -> stream, N, W, H, views, offsets.  room 256^3: the back wall's band reaches the +z face's boundary cells (the case the model reproduced);
# stress 256^3: the stress room is cut by the -x and +z faces, blocks fill the boundary cells there
MAPS = {
    "room_256": ("room", 256, 160, 120, list(OUTSIDE_VIEWS), OFFSETS),
    "stress_256": ("stress", 256, 160, 120, list(OUTSIDE_VIEWS), OFFSETS),
    # the second stage (fbits) runs only where an 8x8 beam fits its clearance bound at working distance: a 640x480 camera at >= 512^3 (se_hip_api.hip)
    "stress_512_640x480": ("stress", 512, 640, 480, ["+z", "+z_tilted"], OFFSETS[1::2]),
}


class _Scene:
    """The map of frames 0-5 integrated by the oracle, and the oracle's images from every camera of the sweep."""

    def __init__(self, name):
        kind, self.N, self.W, self.H, views, offsets = MAPS[name]
        stream = make_stream(kind, self.W, self.H, DIM)
        self.k = np.asarray(stream.k, np.float32)
        self.frames = [(stream.depth(f), stream.pose(f)) for f in range(FRAMES)]
        self.cpu = OraclePipeline(SDF, self.N, DIM, self.W, self.H)
        for f, (depth, pose) in enumerate(self.frames):
            self.cpu.integrate(depth, pose, self.k, MU, f)
        self.cameras = [(v, d, outside_view(v, d, DIM)) for v in views for d in offsets]
        self.images = []
        for _, _, view in self.cameras:
            ran, v_c, n_c = self.cpu.raycast(view, self.k, MU, 100)
            assert ran
            self.images.append((v_c, n_c))

    def gpu(self, **kw):
        gpu = DenseSLAMPipeline((self.W, self.H), self.N, DIM, field_type=SDF, **kw)
        for f, (depth, pose) in enumerate(self.frames):
            gpu.set_depth(depth)
            gpu.setPose(pose)
            assert gpu.integration(self.k, 1, MU, f)
        m = compare_maps(self.cpu, gpu)
        assert m["same_block_set"] and m["same_node_set"] and m["x_mismatch"] == 0 and m["y_mismatch"] == 0, m
        return gpu

    def check(self, what, i, v_g, n_g):
        v_c, n_c = self.images[i]
        r = compare_raycast({"v_c": v_c, "n_c": n_c, "v_g": v_g, "n_g": n_g}, DIM / self.N)
        assert r["hitmask_mismatch"] == 0 and r["vertex_bit_mismatch_px"] == 0 and r["normal_bit_mismatch_px"] == 0, (what, self.cameras[i][:2], r)
        return r["hits_gpu"]


_scenes = {}


def _scene(name):
    if name not in _scenes:
        _scenes[name] = _Scene(name)
    return _scenes[name]


def teardown_module(module):
    for s in _scenes.values():
        s.cpu.close()
    _scenes.clear()


def _eager(scene, gpu):
    hits = {}
    for i, (name, _, view) in enumerate(scene.cameras):
        gpu.setPose(view)
        assert gpu.raycasting(scene.k, MU, 100 + i)
        v_g, n_g = gpu.vertex_normal()
        hits[name] = hits.get(name, 0) + scene.check("eager", i, v_g, n_g)
    return hits


@pytest.mark.parametrize("path", ["eager", "deferred", "pooled"])
@pytest.mark.parametrize("name", ["room_256", "stress_256"])
def test_raycast_from_beyond_every_face(name, path):
    """Six faces and four tilted views, 24 offsets each: eager raycasting() on a dense and on a pooled map; raycasting_deferred() on a streaming
    handle, where the raycast is launched with the next integration's allocation scan (k_raycast_scan).  That integration gets an empty depth
    image, so the map stays the oracle's (checked at the end) and the next camera sees the same map."""
    scene = _scene(name)
    if path == "deferred":
        gpu = scene.gpu(streaming=True)
        assert gpu.frame_is_fused()
        empty = np.zeros((scene.H, scene.W), np.float32)
        hits = {}
        for i, (view_name, _, view) in enumerate(scene.cameras):
            frame = 100 + 2 * i
            fused = gpu.launch_counts()["fused"]
            gpu.set_depth(empty)
            gpu.setPose(view)
            assert gpu.raycasting_deferred(scene.k, MU, frame)
            assert gpu.integration(scene.k, 1, MU, frame + 1)
            assert gpu.launch_counts()["fused"] == fused + 1           # the raycast rode in the scan's launch
            v_g, n_g = gpu.vertex_normal()
            hits[view_name] = hits.get(view_name, 0) + scene.check("deferred", i, v_g, n_g)
        m = compare_maps(scene.cpu, gpu)
        assert m["same_block_set"] and m["same_node_set"] and m["x_mismatch"] == 0 and m["y_mismatch"] == 0, m
    else:
        gpu = scene.gpu(max_blocks=(1 << 15) if path == "pooled" else 0)
        assert gpu.memory_info()["layout"] == ("pooled bricks" if path == "pooled" else "dense brick grid")
        hits = _eager(scene, gpu)
    print(name, path, hits)
    assert sum(hits.values()) > 50000                                   # the sweep looked at surfaces, not only at nothing
    assert all(hits[v] > 1000 for v in ("-x", "+x", "-y", "+y", "-z", "+z", "upper_corner")), hits
    gpu.close()


@pytest.mark.parametrize("name", ["room_256", "stress_512_640x480"])
def test_beam_knob_never_changes_the_images(name, monkeypatch):
    """SE_HIP_BEAM = 0 (every ray starts at the near plane), 1 (coarse stage), 2 (coarse and fine stage, the default) is read when the handle is
    created; results must not depend on it.  room_256 has no fine grid (stage 1 only); stress_512_640x480 runs both stages."""
    scene = _scene(name)
    for beam in ("0", "1", "2"):
        monkeypatch.setenv("SE_HIP_BEAM", beam)
        gpu = scene.gpu()
        hits = _eager(scene, gpu)
        print(name, "SE_HIP_BEAM", beam, hits)
        assert sum(hits.values()) > 50000, hits
        gpu.close()
