#!/usr/bin/env python3
"""Cost of the distance field of a region (se_hip_distance_field) against the only other way to get these numbers on the device, one
se_hip_clearance_boxes query per voxel, on SDF dense maps built from the synthetic room and stress streams (640x480, 4.8 m, --frames
frames) at --res.

Regions of --sides^3 voxels, each placed twice:
  surface    centred on a raycast hit vertex of the last frame
  free       centred on the 8^3 box, of 4096 placed uniformly, that is farthest from any occupied voxel
For every region, every r_max of --r-max, robot (1,1,1) and (8,8,8), with and without nearest, timed on the same map in the same run through
the device entries with events around --reps back-to-back calls after --warmup (each variant twice, the variants alternating; the mean and
both runs are recorded):
  field        se_hip_distance_field
  clearance    se_hip_clearance_boxes over the region's voxels, the query array prepared beforehand
and whether the two answers are equal.  One JSON line per map, region and variant.
The split of a call over its four kernels is not timed here: the four launches happen inside one library call, which offers no place for
events between them and moves none of the SE_HIP_K_* counters.  It comes from a kernel trace instead: --trace makes every field call once
and nothing else, and `rocprofv3 --kernel-trace --stats -- python tools/field_bench.py --trace --maps room --sides 64 128` lists the
kernels in launch order, four per call in the order of the loops below; profiles/field_kernel_trace.txt is that list, one line per call."""
import argparse
import ctypes as C
import os

import numpy as np
import torch

from query_bench_common import DIM, ROOT, JsonLines, hit_vertices, map_tag   # (puts the repository root on sys.path)
from clearance_bench import build_map
from supereight_amd.pipeline import _MOTION_STOPS, SDF, _ClearanceOut, _CollideTest, _FieldOut, _FieldRequest


def voxel_queries(lo, side, robot, r_max):
    ax = [np.arange(lo[k], lo[k] + side[k], dtype=np.int32) for k in range(3)]
    v = np.stack(np.broadcast_arrays(ax[0][None, None, :], ax[1][None, :, None], ax[2][:, None, None]), -1).reshape(-1, 3)
    q = np.empty((len(v), 7), np.int32)
    q[:, 0:3], q[:, 3:6], q[:, 6] = v, robot, r_max
    return q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--sides", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--r-max", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--maps", nargs="+", default=["room", "stress"])
    ap.add_argument("--trace", action="store_true", help="the field calls only, once each: for a kernel trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    log = JsonLines()
    res = args.res
    for kind in args.maps:
        p = build_map(kind, res, args.frames)
        test = _CollideTest(0.0, 0)
        stop = _MOTION_STOPS["occupied"]

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

        hits = hit_vertices(p)
        surface = (hits[rng.integers(len(hits))] * (res / DIM)).astype(np.int64)
        cand = np.concatenate([rng.integers(64, res - 72, (4096, 3)), np.full((4096, 3), 8)], 1).astype(np.int32)
        far = p.clearance(np.ascontiguousarray(cand), 64, nearest=False).astype(np.int64)
        free = cand[int(np.argmax(np.where(far < 0, 1 << 40, far))), 0:3].astype(np.int64) + 4
        for side in args.sides:
            for place, centre in (("surface", surface), ("free", free)):
                lo = [int(c) - side // 2 for c in centre]
                n = side ** 3
                d2 = torch.empty((side, side, side), dtype=torch.int32, device=dev)
                near = torch.empty((side, side, side, 3), dtype=torch.int32, device=dev)
                c_d2 = torch.empty(n, dtype=torch.int32, device=dev)
                c_near = torch.empty((n, 3), dtype=torch.int32, device=dev)
                for r_max in args.r_max:
                    for robot in (1, 8):
                        rq = _FieldRequest()
                        rq.r_max, rq.stop_at = r_max, stop
                        for k in range(3):
                            rq.lo[k], rq.side[k], rq.robot[k] = lo[k], side, robot
                        d_q = torch.from_numpy(voxel_queries(lo, (side,) * 3, robot, r_max)).to(dev)
                        for nearest in (True, False):
                            f_out = _FieldOut(d2.data_ptr(), near.data_ptr() if nearest else None)
                            c_out = _ClearanceOut(c_d2.data_ptr(), c_near.data_ptr() if nearest else None)
                            calls = {
                                "field": lambda: p._check(p.lib.se_hip_distance_field(p._h, C.byref(rq), C.byref(test), C.byref(f_out))),
                                "clearance": lambda: p._check(p.lib.se_hip_clearance_boxes(p._h, d_q.data_ptr(), n, C.byref(test), stop, C.byref(c_out))),
                            }
                            if args.trace:
                                calls["field"]()
                                p.sync()
                                continue
                            runs = {k: [] for k in calls}
                            for _ in range(2):
                                for k, call in calls.items():
                                    runs[k].append(round(timed(call), 2))
                            p.sync()
                            equal = bool((d2.reshape(-1) == c_d2).all()) and (not nearest or bool((near.reshape(-1, 3) == c_near).all()))
                            rec = {**map_tag(res, SDF, False), "map": kind, "place": place, "side": side, "r_max": r_max, "robot": robot, "nearest": nearest, "voxels": n}
                            for k, v in runs.items():
                                rec[k + "_us_per_call"] = round(float(np.mean(v)), 2)
                                rec[k + "_us_runs"] = v
                            rec["field_mvoxels_per_s"] = round(n / rec["field_us_per_call"], 3)
                            rec["clearance_mvoxels_per_s"] = round(n / rec["clearance_us_per_call"], 3)
                            rec["clearance_over_field"] = round(rec["clearance_us_per_call"] / rec["field_us_per_call"], 3)
                            rec["equal"] = equal
                            h = d2.cpu().numpy()
                            rec["d2_counts"] = {"touching": int((h == 0).sum()), "apart": int((h > 0).sum()), "none": int((h < 0).sum())}
                            log.emit(rec)
        p.close()
    if not args.trace:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        log.write(args.out)


if __name__ == "__main__":
    main()
