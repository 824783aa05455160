#!/usr/bin/env python3
"""Cost of a column projection (se_hip_project_columns) against what a caller could do before, on SDF dense maps built from the synthetic
room and stress streams (640x480, 4.8 m, --frames frames) at --res.

The footprint is the whole res x res, the columns run along z, with two layer sets:
  full     the full height [0, res)
  three    the full height, a 16-voxel body band at 5/8 of the height and a one-voxel slice at 3/4 (where both streams put surfaces)
For every map and layer set, timed on the same map in the same run through the device entries with events around --reps back-to-back calls
after --warmup (each variant twice, the variants alternating; the mean and both runs are recorded):
  project_status  se_hip_project_columns, status only
  project_all     se_hip_project_columns, all four outputs
  boxes           se_hip_collide_boxes, strict, one 1 x 1 x (b - a) box per cell: the status only.  The boxes are prepared beforehand and
                  lie in device memory; only the launch is timed.
Before timing, the status of the projection and of the boxes is compared on every cell (the tool stops if they differ).  One JSON line per
map and layer set."""
import argparse
import ctypes as C
import os

import numpy as np
import torch

from query_bench_common import DIM, H, ROOT, W, JsonLines, map_tag   # (puts the repository root on sys.path)
from supereight_amd.pipeline import _COLLIDE_MODES, _MOTION_STOPS, SDF, DenseSLAMPipeline, _CollideTest, _ProjectOut, _ProjectRequest
from supereight_amd.synthetic import make_stream


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


def cell_boxes(res, layers):
    """One box per cell, in the order of the projection's outputs: [L * res * res, 6] int32 lo xyz, side xyz."""
    y, x = np.meshgrid(np.arange(res), np.arange(res), indexing="ij")
    x, y = x.reshape(-1), y.reshape(-1)
    one = np.ones_like(x)
    return np.ascontiguousarray(np.concatenate([np.stack([x, y, np.full_like(x, a), one, one, np.full_like(x, b - a)], 1) for a, b in layers]).astype(np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "project_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    log = JsonLines()
    res = args.res
    layer_sets = {"full": [(0, res)], "three": [(0, res), (5 * res // 8, 5 * res // 8 + 16), (3 * res // 4, 3 * res // 4 + 1)]}
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

        for name, layers in layer_sets.items():
            cells = len(layers) * res * res
            rq = _ProjectRequest()
            rq.axis, rq.n_layers, rq.stop_at = 2, len(layers), _MOTION_STOPS["occupied"]
            rq.lo[0] = rq.lo[1] = 0
            rq.side[0] = rq.side[1] = res
            for l, (a, b) in enumerate(layers):
                rq.layers[l][0], rq.layers[l][1] = a, b
            status = torch.empty(cells, dtype=torch.uint8, device=dev)
            first, last, count = (torch.empty(cells, dtype=torch.int32, device=dev) for _ in range(3))
            only, every = _ProjectOut(status.data_ptr(), None, None, None), _ProjectOut(status.data_ptr(), first.data_ptr(), last.data_ptr(), count.data_ptr())
            d_boxes = torch.from_numpy(cell_boxes(res, layers)).to(dev)
            st_boxes = torch.empty(cells, dtype=torch.uint8, device=dev)
            strict = _COLLIDE_MODES["strict"]
            calls = {
                "project_status": lambda: p._check(p.lib.se_hip_project_columns(p._h, C.byref(rq), C.byref(test), C.byref(only))),
                "project_all": lambda: p._check(p.lib.se_hip_project_columns(p._h, C.byref(rq), C.byref(test), C.byref(every))),
                "boxes": lambda: p._check(p.lib.se_hip_collide_boxes(p._h, d_boxes.data_ptr(), cells, C.byref(test), strict, st_boxes.data_ptr())),
            }
            # the two agree on every cell
            calls["project_all"](); calls["boxes"]()
            p.sync()
            if not bool((status == st_boxes).all()):
                raise SystemExit(f"{kind} {name}: the projection and the per-cell boxes differ")
            runs = {k: [] for k in calls}
            for _ in range(2):
                for k, call in calls.items():
                    runs[k].append(round(timed(call), 2))
            h = status.cpu().numpy()
            rec = {**map_tag(res, SDF, False), "map": kind, "layers": name, "cells": cells}
            for k, v in runs.items():
                rec[k + "_us_per_call"] = round(float(np.mean(v)), 2)
                rec[k + "_us_runs"] = v
            rec["boxes_over_project_status"] = round(rec["boxes_us_per_call"] / rec["project_status_us_per_call"], 2)
            rec["boxes_over_project_all"] = round(rec["boxes_us_per_call"] / rec["project_all_us_per_call"], 2)
            rec["status_counts"] = {"occupied": int((h == 0).sum()), "unseen": int((h == 1).sum()), "empty": int((h == 2).sum())}
            rec["blocking_voxels"] = int(count.sum(dtype=torch.int64).item())
            log.emit(rec)
        p.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    log.write(args.out)


if __name__ == "__main__":
    main()
