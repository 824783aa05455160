#!/usr/bin/env python3
"""Cost of batched clearance queries (se_hip_clearance_boxes) against the only device alternative there was before, on SDF dense maps built
from the synthetic room and stress streams (640x480, 4.8 m, --frames frames) at --res.

Queries of an 8^3 robot, 64 k per set:
  surface    boxes centred on raycast hit vertices of the last frame
  free       boxes placed uniformly in the volume and kept where the strict box query answers empty
For every set and every r_max of --r-max, timed on the same map in the same run through the device entries with events around --reps
back-to-back batches after --warmup (each variant twice, the variants alternating; the mean and both runs are recorded):
  clearance       se_hip_clearance_boxes with nearest
  clearance_d2    se_hip_clearance_boxes, d2 only
  ladder          ceil(log2 r_max) + 1 calls of se_hip_collide_boxes, strict, on inflated boxes: the widest (inflated by r_max) first, then a
                  bisection per query for the smallest inflation that still blocks.  It brackets the Chebyshev distance and names no voxel.
                  The boxes of every rung are prepared beforehand (the bisection is run once, untimed): only the launches are timed, which
                  favours the ladder -- a real one decides each rung from the answer of the one before.
and the share of queries for which the ladder's bracket holds the clearance's answer.  One JSON line per map, set and r_max."""
import argparse
import ctypes as C
import math
import os

import numpy as np
import torch

from query_bench_common import DIM, H, ROOT, W, JsonLines, hit_vertices, map_tag   # (puts the repository root on sys.path)
from supereight_amd.pipeline import _COLLIDE_MODES, _MOTION_STOPS, COLLISION_EMPTY, COLLISION_OCCUPIED, SDF, DenseSLAMPipeline, _ClearanceOut, _CollideTest
from supereight_amd.synthetic import make_stream

ROBOT = 8


def build_map(kind, res, frames):
    mu = 0.1
    s = make_stream(kind, W, H, DIM, holes=False)
    p = DenseSLAMPipeline((W, H), res, DIM, field_type=SDF)
    for f in range(frames):
        p.set_depth(s.depth(f))
        p.setPose(s.pose(f))
        p.integration(s.k, 1, mu, f)
        p.raycasting(s.k, mu, f)
    return p


def query_sets(p, res, rng, n=65536):
    side = np.full((n, 3), ROBOT)
    hits = hit_vertices(p)
    c = (hits[rng.choice(len(hits), n)] * (res / DIM)).astype(np.int64)
    out = {"surface": np.concatenate([c - ROBOT // 2, side], 1)}
    free = np.zeros((0, 6), np.int64)
    while len(free) < n:
        cand = np.concatenate([rng.integers(0, res - ROBOT, (4 * n, 3)), np.full((4 * n, 3), ROBOT)], 1)
        keep = p.collides(np.ascontiguousarray(cand.astype(np.int32))) == COLLISION_EMPTY
        free = np.concatenate([free, cand[keep]])
    out["free"] = free[:n]
    return {name: np.ascontiguousarray(v.astype(np.int32)) for name, v in out.items()}


def inflated(boxes, k):
    """Each box grown by k[i] voxels on every side."""
    b = boxes.astype(np.int64)
    k = np.asarray(k, np.int64).reshape(-1, 1)
    return np.ascontiguousarray(np.concatenate([b[:, 0:3] - k, b[:, 3:6] + 2 * k], 1).astype(np.int32))


def ladder(p, boxes, r_max):
    """The rungs of the bisection, run once: (the boxes of each rung, per query the smallest inflation in 1 .. r_max that blocks or 0)."""
    n = len(boxes)
    rungs = [inflated(boxes, np.full(n, r_max))]
    blocked = p.collides(rungs[0]) == COLLISION_OCCUPIED
    lo, hi = np.zeros(n, np.int64), np.full(n, r_max, np.int64)        # not blocked at lo, blocked at hi (where blocked at all)
    for _ in range(math.ceil(math.log2(r_max))):
        mid = np.maximum((lo + hi) // 2, 1)
        rungs.append(inflated(boxes, mid))
        b = p.collides(rungs[-1]) == COLLISION_OCCUPIED
        hi = np.where(b & (mid < hi), mid, hi)
        lo = np.where(~b & (mid > lo), mid, lo)
    return rungs, np.where(blocked, hi, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--r-max", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clearance_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    log = JsonLines()
    res = args.res
    for kind in ("room", "stress"):
        p = build_map(kind, res, args.frames)
        test = _CollideTest(0.0, 0)

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

        for name, boxes in query_sets(p, res, rng).items():
            n = len(boxes)
            for r_max in args.r_max:
                queries = np.ascontiguousarray(np.concatenate([boxes, np.full((n, 1), r_max, np.int32)], 1))
                rungs, k_min = ladder(p, boxes, r_max)
                d_q = torch.from_numpy(queries).to(dev)
                d_rungs = [torch.from_numpy(r).to(dev) for r in rungs]
                d2 = torch.empty(n, dtype=torch.int32, device=dev)
                near = torch.empty((n, 3), dtype=torch.int32, device=dev)
                st = torch.empty(n, dtype=torch.uint8, device=dev)
                stop, strict = _MOTION_STOPS["occupied"], _COLLIDE_MODES["strict"]
                with_n, without_n = _ClearanceOut(d2.data_ptr(), near.data_ptr()), _ClearanceOut(d2.data_ptr(), None)

                def run_ladder():
                    for r in d_rungs:
                        p._check(p.lib.se_hip_collide_boxes(p._h, r.data_ptr(), n, C.byref(test), strict, st.data_ptr()))

                calls = {
                    "clearance": lambda: p._check(p.lib.se_hip_clearance_boxes(p._h, d_q.data_ptr(), n, C.byref(test), stop, C.byref(with_n))),
                    "clearance_d2": lambda: p._check(p.lib.se_hip_clearance_boxes(p._h, d_q.data_ptr(), n, C.byref(test), stop, C.byref(without_n))),
                    "ladder": run_ladder,
                }
                runs = {k: [] for k in calls}
                for _ in range(2):
                    for k, call in calls.items():
                        runs[k].append(round(timed(call), 2))
                calls["clearance"]()
                p.sync()
                h_d2 = d2.cpu().numpy().astype(np.int64)
                # the ladder's bracket: blocked first at inflation k <=> (k - 1)^2 <= d2 <= 3 (k - 1)^2; nothing within inflation r_max <=> d2 >= r_max^2 or none
                found = k_min > 0
                holds = np.where(found, (h_d2 >= (k_min - 1) ** 2) & (h_d2 <= 3 * (k_min - 1) ** 2) & (h_d2 >= 0), (h_d2 < 0) | (h_d2 >= r_max * r_max))
                # (a clearance beyond r_max in Euclidean terms can lie within the ladder's cube: those the ladder finds and the call does not)
                corner = found & (h_d2 < 0)
                rec = {**map_tag(res, SDF, False), "map": kind, "set": name, "r_max": r_max, "queries": n, "rungs": len(rungs)}
                for k, v in runs.items():
                    rec[k + "_us_per_batch"] = round(float(np.mean(v)), 2)
                    rec[k + "_us_runs"] = v
                rec["clearance_mqueries_per_s"] = round(n / rec["clearance_us_per_batch"], 3)
                rec["ladder_mqueries_per_s"] = round(n / rec["ladder_us_per_batch"], 3)
                rec["ladder_over_clearance"] = round(rec["ladder_us_per_batch"] / rec["clearance_us_per_batch"], 3)
                rec["bracket_holds"] = round(float((holds | corner).mean()), 5)
                rec["d2_counts"] = {"touching": int((h_d2 == 0).sum()), "apart": int((h_d2 > 0).sum()), "none": int((h_d2 < 0).sum())}
                log.emit(rec)
        p.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    log.write(args.out)


if __name__ == "__main__":
    main()
