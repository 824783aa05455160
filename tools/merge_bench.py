#!/usr/bin/env python3
"""Time of the device-side map merge (se_hip_merge_map) on two maps built from disjoint halves of bench.py's synthetic room stream
(640x480, 4.8 m; the first --frames / 2 frames into the destination, the rest into the source), against the only route the library had
before: se_hip_save_map on both handles, the combine in numpy, se_hip_load_map -- timed in the same process.

For every volume resolution and brick layout (dense grid / pooled, the same on both handles; SDF, FUSE, max_weight 100) and for
  same_place   (0, 0, 0)       every source block takes part, every node is aligned
  moved        (-64, 0, 0)     the source moved by eight blocks: some blocks clip, nodes of side <= 64 take part
it reloads the destination's saved map and times one call (wall clock around the call, which synchronises both handles itself): merge_us is
the median of --reloads reloads, the samples and their minimum are kept too; and once per row the file route (wall clock per stage), whose
map must equal the device's afterwards, block for block and value for value.  One JSON line per measurement."""
import argparse
import ctypes as C
import os
import tempfile
import time

import numpy as np

from query_bench_common import DIM, H, ROOT, W, JsonLines, map_tag   # (puts the repository root on sys.path)
from shift_bench import compact, keys_of
from supereight_amd.mapio import load_octree
from supereight_amd.pipeline import SDF, DenseSLAMPipeline, _MergeRule
from supereight_amd.synthetic import intrinsics, pose, render_depth_mm

MAX_WEIGHT = 100


def fuse_sdf(ax, ay, bx, by):
    """The value-pair function of include/se_hip.h for SDF and FUSE, element-wise in float32."""
    f = np.float32
    a_un, b_un = (ax == f(1)) & (ay == f(0)), (bx == f(1)) & (by == f(0))
    ty = np.fmin(by, f(MAX_WEIGHT))
    with np.errstate(all="ignore"):
        w = ay + by
        mean = (ay * ax + by * bx) / w
    t = np.where(f(1) < mean, f(1), mean)
    ox, oy = np.where(f(-1) < t, t, f(-1)), np.fmin(w, f(MAX_WEIGHT))
    ox, oy = np.where(ay == 0, bx, ox), np.where(ay == 0, ty, oy)
    ox, oy = np.where(by == 0, ax, ox), np.where(by == 0, ay, oy)
    ox, oy = np.where(a_un, bx, ox), np.where(a_un, ty, oy)
    return np.where(b_un, ax, ox).astype(f), np.where(b_un, ay, oy).astype(f)


def file_route(dst, src, res, s, base, tmp):
    """save both -> the source's blocks and nodes moved, filtered, combined with the destination's and closed in numpy -> load; seconds per stage"""
    pa, pb, pc = (os.path.join(tmp, n) for n in ("a.bin", "b.bin", "c.bin"))
    dst.load(base); dst.sync()
    t0 = time.perf_counter()
    dst.save(pa); src.save(pb)
    t1 = time.perf_counter()
    a, b = load_octree(pa, "sdf"), load_octree(pb, "sdf")
    leaf = int(np.log2(res)) - 3
    s = np.asarray(s, np.int64)

    def combine(have, keys, vals, field):
        """`have` (sorted by code) with the octants `keys` / values `vals` folded in: existing ones combined, the others appended"""
        at = np.searchsorted(have["code"], keys)
        hit = (at < len(have)) & (have["code"][np.minimum(at, len(have) - 1)] == keys)
        new = np.zeros(int((~hit).sum()), have.dtype)
        new["code"] = keys[~hit]
        new[field]["x"], new[field]["y"] = 1.0, 0.0
        out = np.concatenate([have, new])
        out = out[np.argsort(out["code"])]
        at = np.searchsorted(out["code"], keys)
        out[field]["x"][at], out[field]["y"][at] = fuse_sdf(out[field]["x"][at], out[field]["y"][at], vals["x"], vals["y"])
        return out

    c = b["blocks"]["coords"].astype(np.int64) + s
    keep_b = ((c >= 0) & (c <= res - 8)).all(1)
    blocks = combine(a["blocks"], keys_of(c[keep_b], leaf), b["blocks"]["voxels"][keep_b], "voxels")
    blocks["coords"] = np.stack([compact(blocks["code"] & ~np.uint64(0x1FF), k) for k in range(3)], 1)
    code = b["nodes"]["code"]
    level = (code & np.uint64(0x1FF)).astype(np.int64)
    side = (res >> level)[:, None]
    corner = np.stack([compact(code & ~np.uint64(0x1FF), k) for k in range(3)], 1) + s
    keep_n = ((s[None, :] % side) == 0).all(1) & ((corner >= 0) & (corner <= res - side)).all(1) & ((level >= 1) | (not s.any()))
    nodes = combine(a["nodes"], keys_of(corner[keep_n], level[keep_n]), b["nodes"]["value"][keep_n], "value")
    # the closure: every ancestor of what is there now
    corners = np.concatenate([blocks["coords"].astype(np.int64), np.stack([compact(nodes["code"] & ~np.uint64(0x1FF), k) for k in range(3)], 1)])
    levels = np.concatenate([np.full(len(blocks), leaf), (nodes["code"] & np.uint64(0x1FF)).astype(np.int64)])
    up = [np.unique(keys_of(corners[levels > l] // (res >> l) * (res >> l), l)) for l in range(1, leaf)]
    up = np.concatenate(up) if up else np.zeros(0, np.uint64)
    new = np.zeros(int((~np.isin(up, nodes["code"])).sum()), nodes.dtype)
    new["code"] = up[~np.isin(up, nodes["code"])]
    new["value"]["x"], new["value"]["y"] = 1.0, 0.0
    nodes = np.concatenate([nodes, new])
    nodes = nodes[np.argsort(nodes["code"])]
    nodes["side"] = res >> (nodes["code"] & np.uint64(0x1FF)).astype(np.int64)
    with open(pc, "wb") as fh:
        np.array([a["size"]], "<i4").tofile(fh); np.array([a["dim"]], "<f4").tofile(fh)
        np.array([len(nodes)], "<u8").tofile(fh); nodes.tofile(fh)
        np.array([len(blocks)], "<u8").tofile(fh); blocks.tofile(fh)
    t2 = time.perf_counter()
    dst.load(pc)
    dst.sync()
    t3 = time.perf_counter()
    for path in (pa, pb, pc):
        os.remove(path)
    return {"save_s": round(t1 - t0, 4), "numpy_s": round(t2 - t1, 4), "load_s": round(t3 - t2, 4), "total_s": round(t3 - t0, 4),
            "blocks_after": int(dst.counts()[0]), "nodes_after": int(dst.counts()[1])}


def values_of(p):
    """The map's blocks and nodes without the active flags (which the file route loses), floats as bit patterns."""
    c, x, y, _ = p.blocks()
    code, side, nx, ny = p.nodes()
    return [c, x.view(np.uint32), y.view(np.uint32), code, side, nx.view(np.uint32), ny.view(np.uint32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--reloads", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_bench.jsonl"))
    ap.add_argument("--quick", action="store_true", help="no file route, nothing written (for a rocprofv3 run)")
    args = ap.parse_args()
    log = JsonLines()
    tmp = tempfile.mkdtemp(prefix="merge_bench")
    base = os.path.join(tmp, "base.bin")
    mu, k = 0.1, intrinsics(W)
    half = args.frames // 2
    for res in args.res:
        for pooled in (False, True):
            pair = []
            for frames in (range(0, half), range(half, args.frames)):
                p = DenseSLAMPipeline((W, H), res, DIM, field_type=SDF, max_blocks=24 * (res // 8) ** 2 if pooled else 0)
                for f in frames:
                    p.set_depth(np.ascontiguousarray(render_depth_mm(f, W, H, DIM).astype(np.float32) / np.float32(1000.0)))
                    p.setPose(pose(f, DIM)); p.integration(k, 1, mu, f); p.raycasting(k, mu, f)
                pair.append(p)
            dst, src = pair
            (nb, nn), (sb, sn) = dst.counts(), src.counts()
            dst.save(base)
            rule = _MergeRule(0, float(MAX_WEIGHT))
            for name, shift in (("same_place", (0, 0, 0)), ("moved", (-64, 0, 0))):
                arg = np.array(shift, np.int32)
                counts = np.zeros(12, np.int64)
                samples = []
                for _ in range(args.reloads):
                    dst.load(base); dst.sync()
                    t0 = time.perf_counter()
                    dst._check(dst.lib.se_hip_merge_map(dst._h, src._h, arg.ctypes.data, C.addressof(rule), counts.ctypes.data))
                    samples.append((time.perf_counter() - t0) * 1e6)
                after = dst.counts()
                out = {**map_tag(res, SDF, pooled), "shift": name, "shift_voxels": list(shift), "dst_blocks": nb, "dst_nodes": nn, "src_blocks": sb, "src_nodes": sn,
                       "counts": counts.tolist(), "blocks_after": after[0], "nodes_after": after[1], "merge_us": round(float(np.median(samples)), 1),
                       "merge_us_min": round(min(samples), 1), "merge_us_samples": [round(v, 1) for v in samples]}
                if not args.quick:
                    device = values_of(dst)
                    out["file_route"] = file_route(dst, src, res, shift, base, tmp)
                    assert (out["file_route"]["blocks_after"], out["file_route"]["nodes_after"]) == after, (out["file_route"], after)
                    assert all((u == v).all() for u, v in zip(device, values_of(dst))), "the file route's map differs from the device's"
                    out["speedup_vs_file_route"] = round(out["file_route"]["total_s"] * 1e6 / out["merge_us"], 1)
                log.emit(out)
            dst.close(); src.close()
    os.remove(base)
    if not args.quick:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        log.write(args.out)


if __name__ == "__main__":
    main()
