#!/usr/bin/env python3
"""Cost of batched motion collision queries (se_hip_collide_motions) against the two ways the question could be asked before, on maps built
from bench.py's synthetic room stream (640x480, 4.8 m, --frames frames): SDF dense at every --res, and SDF pooled and OFusion dense once each
at the first.

Motions of a 16^3 robot, |d_k| uniform up to 64 voxels per axis:
  uniform    64 k motions starting uniformly in the volume
  surface    64 k motions starting on raycast hit vertices of the last frame
  diagonal   1 k long diagonals (each |d_k| between a half and three quarters of the volume)
For every set, timed on the same map in the same run through the device entries with events around --reps back-to-back batches after
--warmup (each variant twice, the variants alternating; the mean and both runs are recorded):
  motion          se_hip_collide_motions with t_first
  motion_status   se_hip_collide_motions, status only
  bbox            (a) se_hip_collide_boxes, strict, one bounding box per motion
  chain           (b) se_hip_collide_boxes, strict, the chain of max|d_k| + 1 unit-step boxes per motion (the min over a chain taken afterwards is
                  not in the timed window)
and the share of motions for which (a) and (b) answer differently from the new call.  One JSON line per set and map."""
import argparse
import ctypes as C
import os

import numpy as np
import torch

from query_bench_common import DIM, ROOT, JsonLines, build_map, hit_vertices, map_tag   # (puts the repository root on sys.path)
from supereight_amd.pipeline import _COLLIDE_MODES, _MOTION_STOPS, OFUSION, SDF, _CollideTest, _MotionOut

ROBOT, MAX_D = 16, 64


def motion_sets(res, hits, rng, n=65536):
    side = np.full((n, 3), ROBOT)
    out = {"uniform": np.concatenate([rng.integers(0, res - ROBOT, (n, 3)), side, rng.integers(-MAX_D, MAX_D + 1, (n, 3))], 1)}
    c = (hits[rng.choice(len(hits), n)] * (res / DIM)).astype(np.int64)
    out["surface"] = np.concatenate([c - ROBOT // 2, side, rng.integers(-MAX_D, MAX_D + 1, (n, 3))], 1)
    k = 1024
    sign = rng.integers(0, 2, (k, 3)) * 2 - 1
    mag = rng.integers(res // 2, 3 * res // 4 + 1, (k, 3))
    lo = np.where(sign > 0, rng.integers(0, res // 4 - ROBOT, (k, 3)), res - ROBOT - rng.integers(0, res // 4 - ROBOT, (k, 3)))
    out["diagonal"] = np.concatenate([lo, side[:k], sign * mag], 1)
    return {name: np.ascontiguousarray(v.astype(np.int32)) for name, v in out.items()}


def bounding_boxes(m):
    m = m.astype(np.int64)
    return np.ascontiguousarray(np.concatenate([m[:, 0:3] + np.minimum(m[:, 6:9], 0), m[:, 3:6] + np.abs(m[:, 6:9])], 1).astype(np.int32))


def chains(m):
    """The unit-step chain of each motion: K + 1 boxes, K = max|d_k|, box i at lo + round(i d / K); (boxes, the motion each belongs to)."""
    m = m.astype(np.int64)
    K = np.abs(m[:, 6:9]).max(1)
    owner = np.repeat(np.arange(len(m)), K + 1)
    first = np.cumsum(K + 1) - (K + 1)
    i = np.arange(len(owner)) - first[owner]
    Ko = np.maximum(K[owner], 1)
    step = (2 * i[:, None] * m[owner, 6:9] + Ko[:, None]) // (2 * Ko[:, None])
    return np.ascontiguousarray(np.concatenate([m[owner, 0:3] + step, m[owner, 3:6]], 1).astype(np.int32)), owner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_bench.jsonl"))
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

        for name, motions in motion_sets(res, hit_vertices(p), rng).items():
            n = len(motions)
            chain, owner = chains(motions)
            d_mo, d_bb, d_ch = (torch.from_numpy(a).to(dev) for a in (motions, bounding_boxes(motions), chain))
            st = torch.empty(n, dtype=torch.uint8, device=dev)
            tf = torch.empty(n, dtype=torch.float32, device=dev)
            st_bb = torch.empty(n, dtype=torch.uint8, device=dev)
            st_ch = torch.empty(len(chain), dtype=torch.uint8, device=dev)
            stop, strict = _MOTION_STOPS["occupied"], _COLLIDE_MODES["strict"]
            with_t, without_t = _MotionOut(st.data_ptr(), tf.data_ptr()), _MotionOut(st.data_ptr(), None)
            calls = {
                "motion": lambda: p._check(p.lib.se_hip_collide_motions(p._h, d_mo.data_ptr(), n, C.byref(test), stop, C.byref(with_t))),
                "motion_status": lambda: p._check(p.lib.se_hip_collide_motions(p._h, d_mo.data_ptr(), n, C.byref(test), stop, C.byref(without_t))),
                "bbox": lambda: p._check(p.lib.se_hip_collide_boxes(p._h, d_bb.data_ptr(), n, C.byref(test), strict, st_bb.data_ptr())),
                "chain": lambda: p._check(p.lib.se_hip_collide_boxes(p._h, d_ch.data_ptr(), len(chain), C.byref(test), strict, st_ch.data_ptr())),
            }
            runs = {k: [] for k in calls}
            for _ in range(2):
                for k, call in calls.items():
                    runs[k].append(round(timed(call), 2))
            calls["motion"]()
            p.sync()
            s_mo, t_mo, s_bb = st.cpu().numpy(), tf.cpu().numpy(), st_bb.cpu().numpy()
            s_ch = np.full(n, 2, np.uint8)
            np.minimum.at(s_ch, owner, st_ch.cpu().numpy())
            rec = {**map_tag(res, field, pooled), "set": name, "motions": n, "chain_boxes": len(chain), "mean_chain": round(len(chain) / n, 2)}
            for k, v in runs.items():
                rec[k + "_us_per_batch"] = round(float(np.mean(v)), 2)
                rec[k + "_us_runs"] = v
            rec["motion_ns_each"] = round(rec["motion_us_per_batch"] * 1e3 / n, 1)
            rec["chain_over_motion"] = round(rec["chain_us_per_batch"] / rec["motion_us_per_batch"], 3)
            rec["bbox_over_motion"] = round(rec["bbox_us_per_batch"] / rec["motion_us_per_batch"], 3)
            rec["bbox_differs"] = round(float((s_bb != s_mo).mean()), 5)
            rec["chain_differs"] = round(float((s_ch != s_mo).mean()), 5)
            rec["status_counts"] = {str(k): int((s_mo == k).sum()) for k in (0, 1, 2)}
            rec["t_first_counts"] = {"start": int((t_mo == 0).sum()), "partial": int(((t_mo > 0) & (t_mo < 1.5)).sum()), "free": int((t_mo > 1.5).sum())}
            log.emit(rec)
        p.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    log.write(args.out)


if __name__ == "__main__":
    main()
