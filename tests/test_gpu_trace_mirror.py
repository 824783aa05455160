"""DenseSLAMSystem::traceSegments on a live handle against the host restatement (include/se/segment_trace.hpp) on the getMap() snapshot:
every output for both stop_at values, with and without counts, a sample also against the literal definition; and
DenseSLAMSystem::segmentOf against pipeline.segments_from_points (tests/cpp/trace_mirror.cpp)."""
import os

import numpy as np
import pytest

from supereight_amd.pipeline import segments_from_points
from tests.mirror_util import build_mirror, run_mirror, write_scene

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag,mu", [("SDF", 0.1), ("OFusion", 0.02)], ids=["sdf", "ofusion"])
def test_trace_segments_equal_the_host_restatement(tmp_path, tag, mu):
    exe = build_mirror(tmp_path, "trace_mirror", tag)
    Wm, Hm, N, dim, frames = 320, 240, 256, 4.8, 3
    raw, pf, _ = write_scene(tmp_path, Wm, Hm, dim, frames)
    pairs_file = os.path.join(str(tmp_path), "segments.bin")
    res, r = run_mirror(exe, [raw, pf, N, dim, mu, pairs_file], timeout=600)
    print(r.stdout, r.stderr)
    assert res["bad"] == 0, r.stderr
    assert res["checked"] > 1800 and res["literal"] == 400
    assert res["occupied"] > 0 and res["unseen"] > 0 and res["empty"] > 0
    assert res["blocked"] > 0 and res["free"] > 0 and res["gain"] > 0
    rec = np.fromfile(pairs_file, np.dtype([("m", np.float32, 6), ("s", np.int32, 6)]))
    assert len(rec) == res["pairs"] == 2000
    m = rec["m"].astype(np.float64)
    expect = segments_from_points(m[:, 0:3], m[:, 3:6], float(np.float32(dim)), N)
    assert (rec["s"] == expect).all()
    assert (rec["s"] % 2 != 0).all()
