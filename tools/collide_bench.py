#!/usr/bin/env python3
"""Throughput of batched box collision queries (se_hip_collide_boxes) on maps built from bench.py's synthetic room stream (640x480, 4.8 m).

For every volume resolution, brick layout (dense grid / pooled) and field type (SDF / OFusion) it builds the map from --frames frames, then
times batches through the device entry with HIP events on the handle's stream (the mean of --reps back-to-back batches after --warmup) for
the box sets
  robot16 / robot32         64 k boxes of 16^3 / 32^3 voxels, uniform in the volume
  surface16 / surface32     the same, centred on raycast hit vertices of the last frame
  big128                    1 k boxes of 128^3
  whole                     one box of the whole volume
in both modes (strict, reference).  One JSON line per measurement.  Algorithmic bytes per box (strict mode, no early exit: an upper bound):
4-byte index entries of the eight children of every present overlapping internal octant, plus the voxel bytes (SDF 4 + 1, OFusion 8) of the
box's voxels in present blocks, estimated on a sample of each set.  Kernel durations come from a separate run under
rocprofv3 --kernel-trace --stats (k_collide_boxes in its kernel_stats.csv)."""
import argparse
import ctypes as C
import os
import time

import numpy as np
import torch

from query_bench_common import DIM, ROOT, JsonLines, build_map, hit_vertices, map_tag   # (puts the repository root on sys.path)
from supereight_amd.pipeline import _COLLIDE_MODES, OFUSION, SDF, _CollideTest
PEAK = 8e12   # HBM bytes/s of the part


def box_sets(res, hits, rng):
    out = {}
    for e in (16, 32):
        out[f"robot{e}"] = np.concatenate([rng.integers(0, res - e, (65536, 3)), np.full((65536, 3), e)], 1)
        c = (hits[rng.choice(len(hits), 65536)] * (res / DIM)).astype(np.int64)
        out[f"surface{e}"] = np.concatenate([c - e // 2, np.full((65536, 3), e)], 1)
    out["big128"] = np.concatenate([rng.integers(-32, res - 96, (1024, 3)), np.full((1024, 3), 128)], 1)
    out["whole"] = np.array([[0, 0, 0, res, res, res]])
    return {k: np.ascontiguousarray(v.astype(np.int32)) for k, v in out.items()}


def algorithmic_bytes(p, res, field, boxes, rng, sample=512):
    """mean over a sample of boxes: index entries read (8 x 4 B per present overlapping internal octant) + voxel bytes in present blocks"""
    coords, _, _, _ = p.blocks()
    nb = res // 8
    occ = np.zeros((nb, nb, nb), bool)
    occ[coords[:, 0] // 8, coords[:, 1] // 8, coords[:, 2] // 8] = True
    pyr = [occ]
    while pyr[-1].shape[0] > 1:
        o = pyr[-1]
        pyr.append(o.reshape(o.shape[0] // 2, 2, o.shape[1] // 2, 2, o.shape[2] // 2, 2).any(axis=(1, 3, 5)))
    vb = 5 if field == SDF else 8
    idx = rng.choice(len(boxes), min(sample, len(boxes)), replace=False)
    tot = 0.0
    for i in idx:
        lo = np.maximum(boxes[i, :3], 0)
        hi = np.minimum(boxes[i, :3] + boxes[i, 3:], res)
        if (hi <= lo).any():
            continue
        nodes = 1   # the root
        for lvl, g in enumerate(pyr[1:-1], start=1):   # internal levels below the root: block side 8 << lvl
            sd = 8 << lvl
            a, b = lo // sd, (hi - 1) // sd + 1
            nodes += int(g[a[0]:b[0], a[1]:b[1], a[2]:b[2]].sum())
        a, b = lo // 8, (hi - 1) // 8 + 1
        vox = 0
        for bx, by, bz in np.argwhere(occ[a[0]:b[0], a[1]:b[1], a[2]:b[2]]) + a:
            c = np.array([bx, by, bz]) * 8
            vox += int(np.prod(np.minimum(hi, c + 8) - np.maximum(lo, c)))
        tot += nodes * 8 * 4 + vox * vb
    return tot / len(idx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collide_bench.jsonl"))
    ap.add_argument("--quick", action="store_true", help="fewer reps, no byte estimate (for the rocprofv3 run)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    log = JsonLines()
    for res in args.res:
        for field in (SDF, OFUSION):
            for pooled in (False, True):
                p, _, _ = build_map(res, field, pooled, args.frames)
                hits = hit_vertices(p)
                sets = box_sets(res, hits, rng)
                for name, boxes in sets.items():
                    ab = None if args.quick else algorithmic_bytes(p, res, field, boxes, rng)
                    dboxes = torch.from_numpy(boxes).to(dev)
                    for mode in ("strict", "reference"):
                        for _ in range(args.warmup):
                            p.collides(dboxes, mode=mode)
                        st = p.collides(dboxes, mode=mode).cpu().numpy()
                        # back-to-back batches on the handle's stream, timed with events around them (the wrapper syncs after each
                        # call; the C entry is used directly here so that the batches queue up)
                        test = _CollideTest(0.0, int(field == OFUSION))
                        out = torch.empty(len(boxes), dtype=torch.uint8, device=dev)
                        t0 = time.perf_counter()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        p.sync()
                        torch.cuda.synchronize()
                        e0.record()
                        for _ in range(args.reps):
                            p._check(p.lib.se_hip_collide_boxes(p._h, dboxes.data_ptr(), len(boxes), C.byref(test), _COLLIDE_MODES[mode], out.data_ptr()))
                        p.sync()
                        e1.record()
                        torch.cuda.synchronize()
                        wall = (time.perf_counter() - t0) / args.reps
                        us = e0.elapsed_time(e1) * 1e3 / args.reps
                        rec = {**map_tag(res, field, pooled), "set": name,
                               "mode": mode, "boxes": len(boxes), "us_per_batch": round(us, 2), "wall_us_per_batch": round(wall * 1e6, 2),
                               "boxes_per_s": round(len(boxes) / (us * 1e-6), 1),
                               "status_counts": {str(k): int((st == k).sum()) for k in (0, 1, 2)}}
                        if ab is not None:
                            rec["alg_bytes_per_box_strict_upper"] = round(ab, 1)
                            rec["frac_of_8TBps"] = round(ab * len(boxes) / (us * 1e-6) / PEAK, 5)
                        log.emit(rec)
                p.close()
    if not args.quick:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        log.write(args.out)


if __name__ == "__main__":
    main()
