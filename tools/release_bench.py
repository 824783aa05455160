#!/usr/bin/env python3
"""Time of the device-side release (se_hip_release_boxes) on maps built from bench.py's synthetic room stream (640x480, 4.8 m), against the
only route the library had before: se_hip_save_map, the octants deleted in numpy, se_hip_load_map -- timed in the same process.

For every volume resolution and brick layout (dense grid / pooled; SDF) it builds the map from --frames frames and saves it; then for
  unseen_everywhere   one record over the whole volume, SE_HIP_RELEASE_UNSEEN
  all_one_octant      SE_HIP_RELEASE_ALL on the octant of the volume that holds the most blocks
  nothing_matches     one record that contains no whole block (the call returns after the decision kernels)
it reloads the saved map and times one call (wall clock around the call, which synchronises the handle itself): release_us is the median
of --reloads reloads, the samples and their minimum are kept too; and once per map and record the file route (wall clock per stage), with
the blocks before and after, the size of the saved map file before and after, and memory_info before and after.
Then, per map, the effect on later frames: the sweep and raycast times of se_hip_get_timings over --later further frames, with and without
a release of the all-unseen octants after frame --frames, and how many of the released blocks the next frame creates again.
One JSON line per measurement."""
import argparse
import os
import tempfile
import time

import numpy as np

from query_bench_common import DIM, H, ROOT, W, JsonLines, map_tag   # (puts the repository root on sys.path)
from supereight_amd.mapio import load_octree
from supereight_amd.pipeline import RELEASE_DTYPE, SDF, DenseSLAMPipeline
from supereight_amd.synthetic import SyntheticStream

ALL, UNSEEN = 1, 2


def compact(code, axis):
    code = np.asarray(code, np.uint64)
    r = np.zeros(len(code), np.int64)
    for i in range(21):
        r |= ((code >> np.uint64(3 * i + axis)) & np.uint64(1)).astype(np.int64) << i
    return r


def spread(v):
    v = np.asarray(v, np.uint64)
    r = np.zeros_like(v)
    for i in range(21):
        r |= ((v >> np.uint64(i)) & np.uint64(1)) << np.uint64(3 * i)
    return r


def keys_of(corner, level):
    c = np.asarray(corner, np.int64).reshape(-1, 3)
    return spread(c[:, 0]) | (spread(c[:, 1]) << np.uint64(1)) | (spread(c[:, 2]) << np.uint64(2)) | np.asarray(level).astype(np.uint64)


def file_route(p, res, rec, base, tmp):
    """save -> the released octants deleted in numpy (one record), parent entries reset -> load; seconds of wall clock per stage"""
    path, path2 = os.path.join(tmp, "a.bin"), os.path.join(tmp, "b.bin")
    p.load(base); p.sync()
    t0 = time.perf_counter()
    p.save(path)
    t1 = time.perf_counter()
    m = load_octree(path, "sdf")
    leaf = int(np.log2(res)) - 3
    lo, hi, what = rec["lo"].astype(np.int64), rec["lo"].astype(np.int64) + rec["side"], int(rec["what"])
    blocks, nodes = m["blocks"], m["nodes"].copy()
    c = blocks["coords"].astype(np.int64)
    empty_b = (blocks["voxels"]["x"] == 1.0).all(1) & (blocks["voxels"]["y"] == 0.0).all(1)
    gone_b = ((c >= lo) & (c + 8 <= hi)).all(1) & (empty_b | (what == ALL))
    code = nodes["code"]
    level = (code & np.uint64(0x1FF)).astype(np.int64)
    side = res >> level
    corner = np.stack([compact(code & ~np.uint64(0x1FF), k) for k in range(3)], 1)
    empty_n = (nodes["value"]["x"] == 1.0).all(1) & (nodes["value"]["y"] == 0.0).all(1)
    stays = ~(((corner >= lo) & (corner + side[:, None] <= hi)).all(1) & (empty_n | (what == ALL)) & (level > 0))
    order = np.argsort(code)
    find = lambda k: order[np.searchsorted(code[order], k)]

    def parent(corners, l):
        d = res >> (l - 1)
        return find(keys_of(corners // d * d, l - 1)), ((corners // (d // 2)) & 1) @ np.array([1, 2, 4])
    pb, cb = parent(c, leaf)
    stays[pb[~gone_b]] = True
    for l in range(leaf - 1, 0, -1):
        sel = np.nonzero((level == l) & stays)[0]
        stays[parent(corner[sel], l)[0]] = True
    pairs = [(pb[gone_b], cb[gone_b])] + [parent(corner[(level == l) & ~stays], l) for l in range(1, leaf)]
    for pi, ch in pairs:
        nodes["value"]["x"][pi, ch], nodes["value"]["y"][pi, ch] = 1.0, 0.0
    blocks, nodes = blocks[~gone_b], nodes[stays]
    with open(path2, "wb") as fh:
        np.array([m["size"]], "<i4").tofile(fh); np.array([m["dim"]], "<f4").tofile(fh)
        np.array([len(nodes)], "<u8").tofile(fh); nodes.tofile(fh)
        np.array([len(blocks)], "<u8").tofile(fh); blocks.tofile(fh)
    t2 = time.perf_counter()
    p.load(path2)
    p.sync()
    t3 = time.perf_counter()
    sizes = (os.path.getsize(path), os.path.getsize(path2))
    os.remove(path); os.remove(path2)
    return {"save_s": round(t1 - t0, 4), "numpy_s": round(t2 - t1, 4), "load_s": round(t3 - t2, 4), "total_s": round(t3 - t0, 4),
            "blocks_after": int(p.counts()[0]), "nodes_after": int(p.counts()[1]), "file_bytes_before": sizes[0], "file_bytes_after": sizes[1]}


def later_frames(res, pooled, frames, later, release, mu=0.1):
    """--frames frames, optionally a release of the all-unseen octants, then `later` frames timed by se_hip_get_timings."""
    s = SyntheticStream(W, H, DIM, holes=False)
    p = DenseSLAMPipeline((W, H), res, DIM, field_type=SDF, max_blocks=24 * (res // 8) ** 2 if pooled else 0)
    out = {}
    for f in range(frames + later):
        if f == frames:
            if release:
                before = set(map(tuple, p.blocks()[0].tolist()))
                r = p.release(what="unseen")
                gone = before - set(map(tuple, p.blocks()[0].tolist()))
                out.update(blocks_released=r["blocks_released"], nodes_released=r["nodes_released"], blocks_kept=r["blocks_kept"])
            p.enable_timing(True)
            p.timings(reset=True)
        p.set_depth(s.depth(f)); p.setPose(s.pose(f)); p.integration(s.k, 1, mu, f); p.raycasting(s.k, mu, f)
        if f == frames and release:
            out["recreated_by_next_frame"] = len(gone & set(map(tuple, p.blocks()[0].tolist())))
    t = p.timings()
    out.update(sweep_us=round(t["integrate"]["ms_sum"] * 1e3 / max(t["integrate"]["launches"], 1), 2),
               raycast_us=round(t["raycast"]["ms_sum"] * 1e3 / max(t["raycast"]["launches"], 1), 2), blocks_end=int(p.counts()[0]))
    p.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--reloads", type=int, default=5)
    ap.add_argument("--later", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "release_bench.jsonl"))
    args = ap.parse_args()
    log = JsonLines()
    tmp = tempfile.mkdtemp(prefix="release_bench")
    base = os.path.join(tmp, "base.bin")
    mu = 0.1
    for res in args.res:
        for pooled in (False, True):
            s = SyntheticStream(W, H, DIM, holes=False)
            p = DenseSLAMPipeline((W, H), res, DIM, field_type=SDF, max_blocks=24 * (res // 8) ** 2 if pooled else 0)
            for f in range(args.frames):
                p.set_depth(s.depth(f)); p.setPose(s.pose(f)); p.integration(s.k, 1, mu, f); p.raycasting(s.k, mu, f)
            nb, nn = p.counts()
            c = p.blocks()[0]
            h = res // 2
            octant = max(((x, y, z) for x in (0, h) for y in (0, h) for z in (0, h)), key=lambda o: int(((c >= o) & (c < np.array(o) + h)).all(1).sum()))
            p.save(base)
            for name, row in (("unseen_everywhere", ((0, 0, 0), res, UNSEEN)), ("all_one_octant", (octant, h, ALL)), ("nothing_matches", ((0, 0, 0), (res, res, 7), ALL))):
                rec = np.zeros(1, RELEASE_DTYPE)
                rec[0]["lo"], rec[0]["side"], rec[0]["what"] = row
                counts, box = np.zeros(5, np.int64), np.zeros(6, np.int32)
                samples = []
                for _ in range(args.reloads):
                    p.load(base); p.sync()
                    mem0 = p.memory_info()
                    t0 = time.perf_counter()
                    p._check(p.lib.se_hip_release_boxes(p._h, rec.ctypes.data, 1, counts.ctypes.data, box.ctypes.data))
                    samples.append((time.perf_counter() - t0) * 1e6)
                after = p.counts()
                out = {**map_tag(res, SDF, pooled), "records": name, "box": [list(map(int, rec[0]["lo"])), list(map(int, rec[0]["side"]))], "blocks_before": nb,
                       "nodes_before": nn, "counts": counts.tolist(), "touched": box.tolist(), "blocks_after": after[0], "nodes_after": after[1],
                       "release_us": round(float(np.median(samples)), 1), "release_us_min": round(min(samples), 1), "release_us_samples": [round(v, 1) for v in samples],
                       "memory_info_before": mem0, "memory_info_after": p.memory_info()}
                out["file_route"] = file_route(p, res, rec[0], base, tmp)
                assert (out["file_route"]["blocks_after"], out["file_route"]["nodes_after"]) == after, (out["file_route"], after)
                out["speedup_vs_file_route"] = round(out["file_route"]["total_s"] * 1e6 / out["release_us"], 1)
                log.emit(out)
            p.close()
            plain, released = later_frames(res, pooled, args.frames, args.later, False), later_frames(res, pooled, args.frames, args.later, True)
            log.emit({**map_tag(res, SDF, pooled), "later_frames": args.later, "without_release": plain, "with_release_unseen": released})
    os.remove(base)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    log.write(args.out)


if __name__ == "__main__":
    main()
