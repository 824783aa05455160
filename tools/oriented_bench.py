#!/usr/bin/env python3
"""Cost of batched oriented box collision queries (se_hip_collide_oriented) against the way the question could be asked before, on maps built
from bench.py's synthetic room stream (640x480, 4.8 m, --frames frames): SDF dense at every --res, and SDF pooled and OFusion dense once each
at the first.

Boxes of a 16 x 8 x 8 voxel robot (half lengths 8, 4, 4):
  uniform    64 k boxes with uniform random rotations at uniform positions in the volume
  surface    the same boxes centred beside raycast hit vertices of the last frame
  aligned    the same boxes axis-aligned (no rotation, on voxel boundaries)
For every set, timed on the same map in the same run through the device entries with events around --reps back-to-back batches after
--warmup (each variant twice, the variants alternating; the mean and both runs are recorded):
  oriented   se_hip_collide_oriented
  bbox       (a) se_hip_collide_boxes, strict, the bounding axis-aligned box of each box in whole voxels (for the aligned set: the identical
             query through the box kernel)
and the share of boxes for which (a) reports another status.  One JSON line per set and map."""
import argparse
import ctypes as C
import os

import numpy as np
import torch

from query_bench_common import DIM, ROOT, JsonLines, build_map, hit_vertices, map_tag   # (puts the repository root on sys.path)
from supereight_amd.pipeline import _COLLIDE_MODES, OFUSION, ORIENTED_SUB, SDF, _CollideTest, oriented_boxes

HALF = np.array([8.0, 4.0, 4.0])     # voxels


def rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], 1)


def box_sets(res, hits, rng, n=65536):
    vox = DIM / res
    half = np.tile(HALF * vox, (n, 1))
    rot = rotations(rng, n)
    out = {"uniform": oriented_boxes(rng.uniform(10, res - 10, (n, 3)) * vox, rot, half, DIM, res)}
    beside = hits[rng.choice(len(hits), n)] + rng.uniform(-6, 6, (n, 3)) * vox
    out["surface"] = oriented_boxes(beside, rot, half, DIM, res)
    whole = np.floor(beside / vox) * vox                     # centres on voxel corners: half lengths 8, 4, 4 end on voxel boundaries
    out["aligned"] = oriented_boxes(whole, np.tile(np.eye(3), (n, 1, 1)), half, DIM, res)
    return out


def bounding_boxes(b):
    b = b.astype(np.int64)
    ext = np.abs(b[:, 3:12].reshape(-1, 3, 3)).sum(1)
    lo = (b[:, 0:3] - ext) // ORIENTED_SUB
    hi = -((-(b[:, 0:3] + ext)) // ORIENTED_SUB)
    return np.ascontiguousarray(np.concatenate([lo, hi - lo], 1).astype(np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "oriented_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    log = JsonLines()
    configs = [(res, SDF, False) for res in args.res] + [(args.res[0], SDF, True), (args.res[0], OFUSION, False)]
    for res, field, pooled in configs:
        p, _, _ = build_map(res, field, pooled, args.frames)
        test = _CollideTest(0.0, int(field == OFUSION))

        def timed(call):
            for _ in range(args.warmup):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            p.sync()
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.reps):
                call()
            p.sync()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / args.reps

        for name, boxes in box_sets(res, hit_vertices(p), rng).items():
            n = len(boxes)
            d_or, d_bb = (torch.from_numpy(a).to(dev) for a in (boxes, bounding_boxes(boxes)))
            st = torch.empty(n, dtype=torch.uint8, device=dev)
            st_bb = torch.empty(n, dtype=torch.uint8, device=dev)
            strict = _COLLIDE_MODES["strict"]
            calls = {
                "oriented": lambda: p._check(p.lib.se_hip_collide_oriented(p._h, d_or.data_ptr(), n, C.byref(test), st.data_ptr())),
                "bbox": lambda: p._check(p.lib.se_hip_collide_boxes(p._h, d_bb.data_ptr(), n, C.byref(test), strict, st_bb.data_ptr())),
            }
            runs = {k: [] for k in calls}
            for _ in range(2):
                for k, call in calls.items():
                    runs[k].append(round(timed(call), 2))
            p.sync()
            s_or, s_bb = st.cpu().numpy(), st_bb.cpu().numpy()
            rec = {**map_tag(res, field, pooled), "set": name, "boxes": n}
            for k, v in runs.items():
                rec[k + "_us_per_batch"] = round(float(np.mean(v)), 2)
                rec[k + "_us_runs"] = v
            rec["oriented_ns_each"] = round(rec["oriented_us_per_batch"] * 1e3 / n, 1)
            rec["oriented_over_bbox"] = round(rec["oriented_us_per_batch"] / rec["bbox_us_per_batch"], 3)
            rec["bbox_differs"] = round(float((s_bb != s_or).mean()), 5)
            rec["bbox_more_severe"] = round(float((s_bb < s_or).mean()), 5)
            rec["status_counts"] = {str(k): int((s_or == k).sum()) for k in (0, 1, 2, 255)}
            log.emit(rec)
        p.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    log.write(args.out)


if __name__ == "__main__":
    main()
