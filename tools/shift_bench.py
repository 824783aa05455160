#!/usr/bin/env python3
"""Time of the device-side map shift (se_hip_shift_map) on maps built from bench.py's synthetic room stream (640x480, 4.8 m), against the
only route the library had before: se_hip_save_map, the blocks and nodes moved in numpy, se_hip_load_map -- timed in the same process.

For every volume resolution and brick layout (dense grid / pooled; SDF) it builds the map from --frames frames and saves it; then for
  keep_most    (-64, 0, 0)              nearly every block survives
  drop_half    half of the block bounding box, along x: about half of the blocks leave
  drop_all     (size, 0, 0)
it reloads the saved map and times one call (wall clock around the call, which synchronises the handle itself): shift_us is the median
of --reloads reloads, the samples and their minimum are kept too; and once per map and shift the file route (wall clock per stage).
One JSON line per measurement."""
import argparse
import os
import tempfile
import time

import numpy as np

from query_bench_common import DIM, H, ROOT, W, JsonLines, map_tag   # (puts the repository root on sys.path)
from supereight_amd.mapio import load_octree
from supereight_amd.pipeline import SDF, DenseSLAMPipeline
from supereight_amd.synthetic import SyntheticStream


def spread(v):
    v = np.asarray(v, np.uint64)
    r = np.zeros_like(v)
    for i in range(21):
        r |= ((v >> np.uint64(i)) & np.uint64(1)) << np.uint64(3 * i)
    return r


def compact(code, axis):
    code = np.asarray(code, np.uint64)
    r = np.zeros(len(code), np.int64)
    for i in range(21):
        r |= ((code >> np.uint64(3 * i + axis)) & np.uint64(1)).astype(np.int64) << i
    return r


def keys_of(corner, level):
    c = np.asarray(corner, np.int64).reshape(-1, 3)
    return spread(c[:, 0]) | (spread(c[:, 1]) << np.uint64(1)) | (spread(c[:, 2]) << np.uint64(2)) | np.asarray(level).astype(np.uint64)


def file_route(p, res, s, base, tmp):
    """save -> blocks and nodes moved, filtered and closed in numpy -> load; seconds of wall clock per stage"""
    path, path2 = os.path.join(tmp, "a.bin"), os.path.join(tmp, "b.bin")
    p.load(base); p.sync()
    t0 = time.perf_counter()
    p.save(path)
    t1 = time.perf_counter()
    m = load_octree(path, "sdf")
    leaf = int(np.log2(res)) - 3
    s = np.asarray(s, np.int64)
    c = m["blocks"]["coords"].astype(np.int64) + s
    blocks = m["blocks"][((c >= 0) & (c <= res - 8)).all(1)].copy()
    blocks["coords"] = c[((c >= 0) & (c <= res - 8)).all(1)]
    blocks["code"] = keys_of(blocks["coords"], leaf)
    code = m["nodes"]["code"]
    level = (code & np.uint64(0x1FF)).astype(np.int64)
    side = (res >> level)[:, None]
    corner = np.stack([compact(code & ~np.uint64(0x1FF), k) for k in range(3)], 1) + s
    keep = ((s[None, :] % side) == 0).all(1) & ((corner >= 0) & (corner <= res - side)).all(1)
    nodes = m["nodes"][keep].copy()
    nodes["code"] = keys_of(corner[keep], level[keep])
    corners = np.concatenate([blocks["coords"].astype(np.int64), corner[keep]])
    levels = np.concatenate([np.full(len(blocks), leaf), level[keep]])
    nkeys, sides = [np.zeros(1, np.uint64)], [np.array([res], np.int32)]          # the root
    for l in range(1, leaf):
        d = res >> l
        k = np.unique(keys_of(corners[levels > l] // d * d, l))
        nkeys.append(k); sides.append(np.full(len(k), d, np.int32))
    nkeys, sides = np.concatenate(nkeys), np.concatenate(sides)
    new = ~np.isin(nkeys, nodes["code"])
    nn = np.zeros(int(new.sum()), nodes.dtype)
    nn["code"], nn["side"] = nkeys[new], sides[new]
    nn["value"]["x"], nn["value"]["y"] = 1.0, 0.0
    nodes = np.concatenate([nodes, nn])
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
            "blocks_after": int(p.counts()[0]), "nodes_after": int(p.counts()[1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--reloads", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shift_bench.jsonl"))
    ap.add_argument("--quick", action="store_true", help="no file route, nothing written (for a rocprofv3 run)")
    args = ap.parse_args()
    log = JsonLines()
    tmp = tempfile.mkdtemp(prefix="shift_bench")
    base = os.path.join(tmp, "base.bin")
    mu = 0.1
    for res in args.res:
        for pooled in (False, True):
            s = SyntheticStream(W, H, DIM, holes=False)
            p = DenseSLAMPipeline((W, H), res, DIM, field_type=SDF, max_blocks=24 * (res // 8) ** 2 if pooled else 0)
            for f in range(args.frames):
                p.set_depth(s.depth(f)); p.setPose(s.pose(f)); p.integration(s.k, 1, mu, f); p.raycasting(s.k, mu, f)
            nb, nn = p.counts()
            x = p.block_flags()[0][:, 0]
            half = (int(x.min()) + int(x.max()) + 8) // 2 // 8 * 8
            p.save(base)
            for name, shift in (("keep_most", (-64, 0, 0)), ("drop_half", (-half, 0, 0)), ("drop_all", (res, 0, 0))):
                arg = np.array(shift, np.int32)
                counts = np.zeros(4, np.int64)
                samples = []
                for _ in range(args.reloads):
                    p.load(base); p.sync()
                    t0 = time.perf_counter()
                    p._check(p.lib.se_hip_shift_map(p._h, arg.ctypes.data, counts.ctypes.data))
                    samples.append((time.perf_counter() - t0) * 1e6)
                after = p.counts()
                out = {**map_tag(res, SDF, pooled), "shift": name, "shift_voxels": list(shift), "blocks_before": nb, "nodes_before": nn, "counts": counts.tolist(),
                       "blocks_after": after[0], "nodes_after": after[1], "shift_us": round(float(np.median(samples)), 1), "shift_us_min": round(min(samples), 1),
                       "shift_us_samples": [round(v, 1) for v in samples]}
                if not args.quick:
                    out["file_route"] = file_route(p, res, shift, base, tmp)
                    assert (out["file_route"]["blocks_after"], out["file_route"]["nodes_after"]) == after, (out["file_route"], after)
                    out["speedup_vs_file_route"] = round(out["file_route"]["total_s"] * 1e6 / out["shift_us"], 1)
                log.emit(out)
            p.close()
    os.remove(base)
    if not args.quick:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        log.write(args.out)


if __name__ == "__main__":
    main()
