"""Depth fused on top of an edited map, device against oracle, bit for bit.  Both sides fuse 4 frames; the device applies an edit list
(se_hip_edit_boxes), the oracle gets tests/edit_util.truth of its own download through OraclePipeline.set_values; the states must be equal,
and so must the raycast taken at once, the raycast of each of 4 more frames, and the maps after each of them.  The lists put into the map
what the sensor never writes -- reset() of an octant round a visible surface (OFusion: y = 0, met 300 frames later), SDF values outside
[-1, 1], -0.0, a denormal and weights up to 255, OFusion values at +-1000 with timestamps now, in the future (the pole dt = -4 among them)
and far in the past, node values written directly, and the seeded 200-record list of the edit tests -- so that the sweep's weighted average,
its weight cap and OFusion's window run on stored values nobody bounds.  tests/test_oracle_time_and_setter.py asserts on the oracle alone
that each list engages (weights fall from above 100 to 100, values are clamped, dt >= 4, dt == 0 and dt < 0 all occur, no NaN is stored).
OFusion's frame numbers start at 300."""
import pytest

from supereight_amd.pipeline import OFUSION, SDF, DenseSLAMPipeline
from tests import time_axis_util as T
from tests.time_axis_util import DIM, F0, H, MU, N, W

pytestmark = pytest.mark.gpu
CASES = ([(f, kind, N, mb) for f in (SDF, OFUSION) for kind in T.EDIT_KINDS for mb in (0, 2048)] + [(OFUSION, "list", 256, 8192)])
IDS = [f"{'sdf' if f == SDF else 'ofusion'}_{kind}_{n}_{'pooled' if mb else 'dense'}" for f, kind, n, mb in CASES]


@pytest.mark.parametrize("field,kind,n,max_blocks", CASES, ids=IDS)
def test_fusion_onto_an_edited_map(field, kind, n, max_blocks):
    o = T.oracle_fuse_after_edit(field, kind, n)
    k, depths, poses = T.stream_frames()
    mu = MU[field]
    gpu = DenseSLAMPipeline((W, H), n, DIM, field_type=field, max_blocks=max_blocks)
    try:
        for i in range(4):
            gpu.set_depth(depths[i])
            gpu.setPose(poses[i])
            assert gpu.integration(k, 1, mu, F0 + i) and gpu.raycasting(k, mu, F0 + i)
        T.assert_same_state(o["before"], gpu, (kind, "before the edit"))
        counts = gpu.edit_records(o["rec"], test=o["test"], mode=o["mode"])
        print(kind, counts.tolist(), o["counts"].tolist(), o["frames"][0]["regimes"])
        assert (counts == o["counts"]).all(), (counts, o["counts"])
        T.assert_same_state(o["edited"], gpu, (kind, "after the edit"))
        assert gpu.raycasting(k, mu, F0 + 3)                               # at once, from the pose of the last frame
        v, nrm = gpu.vertex_normal()
        T.assert_same_images(o["image"][0], o["image"][1], v, nrm, (kind, "after the edit"), min_hits=50)
        for fr in o["frames"]:
            gpu.set_depth(depths[fr["i"]])
            gpu.setPose(poses[fr["i"]])
            assert gpu.integration(k, 1, mu, fr["frame"]) and gpu.raycasting(k, mu, fr["frame"])
            v, nrm = gpu.vertex_normal()
            T.assert_same_images(fr["v"], fr["n"], v, nrm, (kind, fr["frame"]))
            T.assert_same_state(fr["state"], gpu, (kind, fr["frame"]))
    finally:
        gpu.close()
