#!/usr/bin/env python3
"""Time of batched region edits (se_hip_edit_boxes) on maps built from bench.py's synthetic room stream (640x480, 4.8 m), against the only
route the library had before: se_hip_save_map, the edit applied to the file in numpy, se_hip_load_map.

For every volume resolution, brick layout (dense grid / pooled) and field type it builds the map from --frames frames, then times the device
entry (wall clock around --reps back-to-back calls and one synchronisation, after --warmup) for
  side16 x 1 / 64 / 4096    boxes of 16^3 voxels centred on raycast hit vertices of the last frame, blocks and nodes, both values assigned
  whole                     one box of the whole volume; also bytes of bricks touched (read + write: SDF 2 x 2560, OFusion 2 x 4096 per block
                            with an application) / time against the 8 TB/s of the README's rooflines
and, once per map and edit set, the save -> numpy -> load route (wall clock, one run: it takes seconds).  One JSON line per measurement.
Kernel durations come from a separate run under rocprofv3 --kernel-trace --stats (k_edit_blocks / k_edit_nodes in its kernel_stats.csv)."""
import argparse
import os
import tempfile
import time

import numpy as np
import torch

from query_bench_common import DIM, ROOT, JsonLines, build_map, hit_vertices, map_tag   # (puts the repository root on sys.path)
from supereight_amd.mapio import load_octree
from supereight_amd.pipeline import _EDIT_MODES, EDIT_DTYPE, OFUSION, SDF
PEAK = 8e12   # HBM bytes/s of the part


def edit_sets(res, hits, rng, field):
    out = {}
    for k in (1, 64, 4096):
        c = (hits[rng.choice(len(hits), k)] * (res / DIM)).astype(np.int64) - 8
        out[f"side16x{k}"] = np.concatenate([c, c + 16], 1)
    out["whole"] = np.array([[0, 0, 0, res, res, res]])
    recs = {}
    for name, b in out.items():
        r = np.zeros(len(b), EDIT_DTYPE)
        r["lo"], r["hi"] = b[:, :3], b[:, 3:]
        r["x"], r["y"] = (0.5, 7.0) if field == SDF else (-2.0, 1.0)
        r["flags"], r["only"] = 15, 7
        recs[name] = r
    return recs


def file_route(p, field, rec, tmp):
    """save -> the same boxes applied to the blocks of the file in numpy -> load; seconds of wall clock per stage"""
    path, path2 = os.path.join(tmp, "a.bin"), os.path.join(tmp, "b.bin")
    t0 = time.perf_counter()
    p.save(path)
    t1 = time.perf_counter()
    m = load_octree(path, "sdf" if field == SDF else "ofusion")
    blocks, c = m["blocks"], m["blocks"]["coords"].astype(np.int64)
    off = np.stack([np.arange(512) & 7, (np.arange(512) >> 3) & 7, np.arange(512) >> 6], 1)
    for e in rec:
        lo, hi = e["lo"].astype(np.int64), e["hi"].astype(np.int64)
        rows = np.nonzero(((c < hi) & (c + 8 > lo)).all(1))[0]
        if len(rows):
            inside = ((c[rows][:, None, :] + off[None] >= lo) & (c[rows][:, None, :] + off[None] < hi)).all(2)
            v = blocks["voxels"][rows]
            v["x"][inside], v["y"][inside] = e["x"], e["y"]
            blocks["voxels"][rows] = v
    with open(path2, "wb") as fh:
        np.array([m["size"]], "<i4").tofile(fh); np.array([m["dim"]], "<f4").tofile(fh)
        np.array([len(m["nodes"])], "<u8").tofile(fh); m["nodes"].tofile(fh)
        np.array([len(blocks)], "<u8").tofile(fh); blocks.tofile(fh)
    t2 = time.perf_counter()
    p.load(path2)
    p.sync()
    t3 = time.perf_counter()
    os.remove(path); os.remove(path2)
    return {"save_s": round(t1 - t0, 4), "numpy_s": round(t2 - t1, 4), "load_s": round(t3 - t2, 4), "total_s": round(t3 - t0, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--fields", nargs="+", default=["sdf", "ofusion"])
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_bench.jsonl"))
    ap.add_argument("--quick", action="store_true", help="no file route, nothing written (for the rocprofv3 run)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    log = JsonLines()
    tmp = tempfile.mkdtemp(prefix="edit_bench")
    for res in args.res:
        for field in [SDF if f == "sdf" else OFUSION for f in args.fields]:
            for pooled in (False, True):
                p, _, _ = build_map(res, field, pooled, args.frames)
                nb, nn = p.counts()
                for name, rec in edit_sets(res, hit_vertices(p), rng, field).items():
                    drec = torch.from_numpy(rec.view(np.int32).reshape(-1, 10).copy()).to(dev)
                    counts = p.edit_records(drec).cpu().numpy()
                    torch.cuda.synchronize()

                    def call():
                        p._check(p.lib.se_hip_edit_boxes(p._h, drec.data_ptr(), len(rec), None, _EDIT_MODES["strict"], None))
                    for _ in range(args.warmup):
                        call()
                    p.sync()
                    t0 = time.perf_counter()
                    for _ in range(args.reps):
                        call()
                    p.sync()
                    us = (time.perf_counter() - t0) * 1e6 / args.reps
                    out = {**map_tag(res, field, pooled), "set": name, "edits": len(rec), "blocks": nb, "nodes": nn, "us_per_call": round(us, 2),
                           "counts": counts.tolist()}
                    brick = 2 * (2560 if field == SDF else 4096)
                    out["brick_bytes"] = int(counts[2]) * brick
                    out["frac_of_8TBps"] = round(int(counts[2]) * brick / (us * 1e-6) / PEAK, 5)
                    if not args.quick:
                        out["file_route"] = file_route(p, field, rec, tmp)
                        out["speedup_vs_file_route"] = round(out["file_route"]["total_s"] * 1e6 / us, 1)
                    log.emit(out)
                p.close()
    if not args.quick:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        log.write(args.out)


if __name__ == "__main__":
    main()
