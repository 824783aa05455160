#!/usr/bin/env python3
"""Time of batched region allocation (se_hip_allocate_boxes) on maps built from bench.py's synthetic room stream (640x480, 4.8 m), against
the only route the library had before: se_hip_save_map, the blocks and their ancestors added to the file in numpy, se_hip_load_map.

For every volume resolution and brick layout (dense grid / pooled; SDF) it builds the map from --frames frames and saves it; then for
  side16 x 1 / 64 / 4096    boxes of 16^3 voxels, half of them beside raycast hit vertices of the last frame, half anywhere in the volume
  whole                     one box of the whole volume (the pooled handle is given a pool of the whole grid)
it reloads the saved map and times, through the device entry with the counts asked for,
  create_us                 the call that creates the octants (wall clock around the call and one synchronisation; one sample per reload,
                            the median of --creates reloads; the samples and their minimum are kept too)
  again_us                  the same call when everything exists (--reps back-to-back calls and one synchronisation): the price of the
                            look-up pass alone
and, once per map and box set, the save -> numpy -> load route (wall clock; skipped above --file-route-blocks blocks in the file, where it
writes gigabytes: "file_route": null).  One JSON line per measurement."""
import argparse
import os
import tempfile
import time

import numpy as np
import torch

from query_bench_common import DIM, H, ROOT, W, JsonLines, hit_vertices, map_tag   # (puts the repository root on sys.path)
from supereight_amd.mapio import load_octree
from supereight_amd.pipeline import ALLOC_DTYPE, SDF, DenseSLAMPipeline
from supereight_amd.synthetic import SyntheticStream


def spread(v):
    v = np.asarray(v, np.uint64)
    r = np.zeros_like(v)
    for i in range(21):
        r |= ((v >> np.uint64(i)) & np.uint64(1)) << np.uint64(3 * i)
    return r


def keys_of(corner, level):
    c = np.asarray(corner, np.int64).reshape(-1, 3)
    return spread(c[:, 0]) | (spread(c[:, 1]) << np.uint64(1)) | (spread(c[:, 2]) << np.uint64(2)) | np.uint64(level)


def box_sets(res, hits, rng):
    out = {}
    for k in (1, 64, 4096):
        near = (hits[rng.choice(len(hits), (k + 1) // 2)] * (res / DIM)).astype(np.int64) + rng.integers(-40, 41, ((k + 1) // 2, 3))
        far = rng.integers(0, res - 16, (k // 2, 3))
        c = np.clip(np.concatenate([near, far])[:k], 0, res - 16)                  # every box wholly inside the volume
        out[f"side16x{k}"] = np.concatenate([c, c + 16], 1)
    out["whole"] = np.array([[0, 0, 0, res, res, res]])
    recs = {}
    for name, b in out.items():
        r = np.zeros(len(b), ALLOC_DTYPE)
        r["lo"], r["hi"] = b[:, :3], b[:, 3:]
        recs[name] = r
    return recs


def file_route(p, res, rec, base, tmp):
    """save -> the blocks the boxes touch and their ancestors added to the file in numpy -> load; seconds of wall clock per stage"""
    path, path2 = os.path.join(tmp, "a.bin"), os.path.join(tmp, "b.bin")
    p.load(base); p.sync()
    t0 = time.perf_counter()
    p.save(path)
    t1 = time.perf_counter()
    m = load_octree(path, "sdf")
    leaf = int(np.log2(res)) - 3
    lo = np.clip(rec["lo"].astype(np.int64), 0, res) // 8
    hi = (np.clip(rec["hi"].astype(np.int64), 0, res) + 7) // 8
    corners = []
    for l, h in zip(lo, hi):
        if (l < h).all():
            corners.append(np.stack(np.meshgrid(*[np.arange(l[k], h[k]) for k in range(3)], indexing="ij"), -1).reshape(-1, 3) * 8)
    corners = np.unique(np.concatenate(corners), axis=0) if corners else np.zeros((0, 3), np.int64)
    bkeys = keys_of(corners, leaf)
    new = ~np.isin(bkeys, m["blocks"]["code"])
    nb = np.zeros(int(new.sum()), m["blocks"].dtype)
    nb["code"], nb["coords"] = bkeys[new], corners[new]
    nb["voxels"]["x"], nb["voxels"]["y"] = 1.0, 0.0
    blocks = np.concatenate([m["blocks"], nb])
    nkeys, sides = [], []
    for l in range(1, leaf):
        s = res >> l
        k = np.unique(keys_of(corners[new] // s * s, l))
        nkeys.append(k); sides.append(np.full(len(k), s, np.int32))
    nkeys, sides = np.concatenate(nkeys), np.concatenate(sides)
    newn = ~np.isin(nkeys, m["nodes"]["code"])
    nn = np.zeros(int(newn.sum()), m["nodes"].dtype)
    nn["code"], nn["side"] = nkeys[newn], sides[newn]
    nn["value"]["x"], nn["value"]["y"] = 1.0, 0.0
    nodes = np.concatenate([m["nodes"], nn])
    blocks, nodes = blocks[np.argsort(blocks["code"])], nodes[np.argsort(nodes["code"])]
    with open(path2, "wb") as fh:
        np.array([m["size"]], "<i4").tofile(fh); np.array([m["dim"]], "<f4").tofile(fh)
        np.array([len(nodes)], "<u8").tofile(fh); nodes.tofile(fh)
        np.array([len(blocks)], "<u8").tofile(fh); blocks.tofile(fh)
    t2 = time.perf_counter()
    p.load(path2)
    p.sync()
    t3 = time.perf_counter()
    os.remove(path); os.remove(path2)
    return {"save_s": round(t1 - t0, 4), "numpy_s": round(t2 - t1, 4), "load_s": round(t3 - t2, 4), "total_s": round(t3 - t0, 4),
            "blocks_after": int(p.counts()[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--creates", type=int, default=5)
    ap.add_argument("--file-route-blocks", type=int, default=1 << 30, help="skip the file route when the file would hold more blocks than this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alloc_bench.jsonl"))
    ap.add_argument("--quick", action="store_true", help="no file route, nothing written (for a rocprofv3 run)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    log = JsonLines()
    tmp = tempfile.mkdtemp(prefix="alloc_bench")
    base = os.path.join(tmp, "base.bin")
    mu = 0.1
    for res in args.res:
        cells = (res // 8) ** 3
        for pooled in (False, True):
            s = SyntheticStream(W, H, DIM, holes=False)
            p = DenseSLAMPipeline((W, H), res, DIM, field_type=SDF, max_blocks=cells if pooled else 0)
            for f in range(args.frames):
                p.set_depth(s.depth(f)); p.setPose(s.pose(f)); p.integration(s.k, 1, mu, f); p.raycasting(s.k, mu, f)
            nb, nn = p.counts()
            sets = box_sets(res, hit_vertices(p), np.random.default_rng(res))       # the same boxes for both layouts
            p.save(base)
            for name, rec in sets.items():
                drec = torch.from_numpy(rec.view(np.int32).reshape(-1, 8).copy()).to(dev)
                dcounts = torch.zeros(4, dtype=torch.int64, device=dev)
                torch.cuda.synchronize()

                def call():
                    p._check(p.lib.se_hip_allocate_boxes(p._h, drec.data_ptr(), len(rec), dcounts.data_ptr(), None, 0))
                create = []
                for _ in range(args.creates):
                    p.load(base); p.sync()
                    t0 = time.perf_counter()
                    call()
                    p.sync()
                    create.append((time.perf_counter() - t0) * 1e6)
                    counts = dcounts.cpu().tolist()
                call(); p.sync()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    call()
                p.sync()
                again = (time.perf_counter() - t0) * 1e6 / args.reps
                out = {**map_tag(res, SDF, pooled), "set": name, "boxes": len(rec), "blocks_before": nb, "nodes_before": nn, "counts": counts,
                       "create_us": round(float(np.median(create)), 2), "create_us_min": round(min(create), 2), "create_us_samples": [round(c, 1) for c in create], "again_us": round(again, 2)}
                if not args.quick:
                    out["file_route"] = file_route(p, res, rec, base, tmp) if nb + counts[0] <= args.file_route_blocks else None
                    if out["file_route"]:
                        assert out["file_route"]["blocks_after"] == nb + counts[0], (out["file_route"], nb, counts)
                        out["speedup_vs_file_route"] = round(out["file_route"]["total_s"] * 1e6 / out["create_us"], 1)
                if len(rec) == 1:
                    out["box"] = rec["lo"][0].tolist() + rec["hi"][0].tolist()
                log.emit(out)
            p.close()
    os.remove(base)
    if not args.quick:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        log.write(args.out)


if __name__ == "__main__":
    main()
