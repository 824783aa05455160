"""What tools/query_bench.py, tools/collide_bench.py and tools/ray_bench.py share: the map they query (bench.py's synthetic room stream,
640x480, 4.8 m), the event-timed loop and the JSON-lines output."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from supereight_amd.pipeline import SDF, DenseSLAMPipeline  # noqa: E402
from supereight_amd.synthetic import SyntheticStream  # noqa: E402

W, H, DIM = 640, 480, 4.8


def build_map(res, field, pooled, frames):
    """The map after `frames` frames of the room stream, integrated and raycast: (pipeline, stream, mu)."""
    mu = 0.1 if field == SDF else 0.02
    s = SyntheticStream(W, H, DIM, holes=False)
    p = DenseSLAMPipeline((W, H), res, DIM, field_type=field, max_blocks=24 * (res // 8) ** 2 if pooled else 0)
    for f in range(frames):
        p.set_depth(s.depth(f))
        p.setPose(s.pose(f))
        p.integration(s.k, 1, mu, f)
        p.raycasting(s.k, mu, f)
    return p, s, mu


def hit_vertices(p):
    """Raycast hit vertices of the last frame (metres)."""
    v, n = p.vertex_normal()
    return v[n[..., 0] != -2]


def map_tag(res, field, pooled):
    """The keys every record starts with."""
    return {"res": res, "field": "sdf" if field == SDF else "ofusion", "layout": "pooled" if pooled else "dense"}


def timed(stream, reps, fn):
    """Microseconds per call of `fn`: HIP events on `stream` around `reps` back-to-back calls, after one warm-up call."""
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


class JsonLines:
    """One JSON line per record on stdout as it is measured; write(path) saves them all."""

    def __init__(self):
        self.records = []

    def emit(self, rec):
        print(json.dumps(rec), flush=True)
        self.records.append(rec)

    def write(self, path):
        with open(path, "w") as f:
            for rec in self.records:
                f.write(json.dumps(rec) + "\n")
