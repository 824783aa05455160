#!/usr/bin/env python3
"""Time of the device-side rigid map merge (se_hip_merge_map_rigid) on two maps built from disjoint halves of bench.py's synthetic room
stream (640x480, 4.8 m; the first --frames / 2 frames into the destination, the rest into the source), against the only route the library
had before: se_hip_save_map on both handles, the resampling in numpy (the literal truth of tests/merge_rigid_util.py, a slab of z layers
at a time), se_hip_load_map -- timed in the same process.

For every volume resolution and brick layout (dense grid / pooled, the same on both handles; SDF, FUSE, max_weight 100) and for
  yaw       30 degrees about the vertical through the volume's centre, translation (10.25, -3.5, 6.125) voxels
  general   50 degrees about (1, 2, 3) / sqrt(14) through the centre, a translation that takes part of the source out of the destination
it reloads the destination's saved map and times one call (wall clock around the call, which synchronises both handles itself): merge_us is
the median of --reloads reloads, the samples and their minimum are kept too; candidate blocks (the bitmap rule of se_resample_kernels.h,
restated in numpy) against participating blocks; observed samples per second.  Once per transform, at --file-route-res and the dense
layout, the file route (wall clock per stage), whose map must equal the device's afterwards, block for block and value for value.  Once
per resolution the geometry of a fresh map merged under `yaw`: the distance in voxels between the source's raycast hit vertices carried
through the transform and the destination's raycast from the carried pose.  One JSON line per measurement."""
import argparse
import ctypes as C
import os
import tempfile
import time

import numpy as np

from query_bench_common import DIM, H, ROOT, W, JsonLines, map_tag   # (puts the repository root on sys.path)
from supereight_amd.pipeline import SDF, DenseSLAMPipeline, _MergeRule
from supereight_amd.synthetic import intrinsics, pose, render_depth_mm
from tests.merge_rigid_util import merge_rigid_truth, pull_of, rotation
from tests.shift_util import write_map_file

MAX_WEIGHT = 100


def transforms(res):
    """name -> (R, t), x_dst = R x_src + t in voxels, both volumes of side `res`."""
    c = np.full(3, (res - 1) / 2.0)
    out = {}
    for name, R, extra in (("yaw", rotation((0, 1, 0), 30.0), np.array([10.25, -3.5, 6.125])),
                           ("general", rotation((1, 2, 3), 50.0), np.array([0.3, -0.45, 0.2]) * res)):
        out[name] = (R, c - R @ c + extra)
    return out


def candidate_blocks(coords, R, t, res):
    """The number of destination blocks the candidate kernel marks: per source block the bounding box of its cube's image, grown by a voxel,
    clipped."""
    c = np.asarray(coords, np.float64).reshape(-1, 3)
    corners = np.stack([c + 8.0 * np.array([i, j, k]) for i in (0, 1) for j in (0, 1) for k in (0, 1)], 1)          # [nb, 8, 3]
    image = corners @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)
    lo = np.maximum(np.floor(image.min(1)) - 1, 0).astype(np.int64) >> 3
    hi = np.minimum(np.ceil(image.max(1)) + 1, res - 1).astype(np.int64) >> 3
    marked = set()
    for a, b in zip(lo, hi):
        if (a <= b).all():
            marked.update((x, y, z) for x in range(a[0], b[0] + 1) for y in range(a[1], b[1] + 1) for z in range(a[2], b[2] + 1))
    return len(marked)


def values_of(p):
    """The map's blocks and nodes without the active flags (which the file route loses), floats as bit patterns."""
    c, x, y, _ = p.blocks()
    code, side, nx, ny = p.nodes()
    return [c, x.view(np.uint32), y.view(np.uint32), code, side, nx.view(np.uint32), ny.view(np.uint32)]


def file_route(dst, src, res, pull, base, tmp):
    """save both -> the maps read back, the numpy truth -> a map file -> load; seconds per stage"""
    from supereight_amd.mapio import load_octree
    pa, pb, pc = (os.path.join(tmp, n) for n in ("a.bin", "b.bin", "c.bin"))
    dst.load(base); dst.sync()
    t0 = time.perf_counter()
    dst.save(pa); src.save(pb)
    t1 = time.perf_counter()
    a, b = load_octree(pa, "sdf"), load_octree(pb, "sdf")

    def arrays(m):
        blocks = (m["blocks"]["coords"].astype(np.int32), np.ascontiguousarray(m["blocks"]["voxels"]["x"], np.float32),
                  np.ascontiguousarray(m["blocks"]["voxels"]["y"], np.float32), np.ones(len(m["blocks"]), np.uint8))
        nodes = (m["nodes"]["code"].astype(np.uint64), m["nodes"]["side"].astype(np.uint32),
                 np.ascontiguousarray(m["nodes"]["value"]["x"], np.float32), np.ascontiguousarray(m["nodes"]["value"]["y"], np.float32))
        return blocks, nodes
    (db, dn), (sb, _) = arrays(a), arrays(b)
    want_b, want_n, _ = merge_rigid_truth(res, db, dn, res, sb, pull, 0, SDF, MAX_WEIGHT, slab=16)
    write_map_file(pc, res, DIM, SDF, want_b, want_n)
    t2 = time.perf_counter()
    dst.load(pc)
    dst.sync()
    t3 = time.perf_counter()
    for path in (pa, pb, pc):
        os.remove(path)
    return {"save_s": round(t1 - t0, 4), "numpy_s": round(t2 - t1, 4), "load_s": round(t3 - t2, 4), "total_s": round(t3 - t0, 4),
            "blocks_after": int(dst.counts()[0]), "nodes_after": int(dst.counts()[1])}


def geometry(src, res, pooled, R, t, k, mu, frame):
    """A fresh destination merged under (R, t); the source's raycast from its last pose, carried through the transform, against the
    destination's raycast from the carried pose: the distance in voxels per pixel hit in both."""
    voxel = DIM / res
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t * voxel
    fresh = DenseSLAMPipeline((W, H), res, DIM, field_type=SDF, max_blocks=24 * (res // 8) ** 2 if pooled else 0)
    try:
        fresh.merge_rigid(src, T_dst_src=T)
        ps = pose(frame, DIM).astype(np.float64)
        src.setPose(ps.astype(np.float32)); src.raycasting(k, mu, frame)
        vs, ns = src.vertex_normal()
        fresh.setPose((T @ ps).astype(np.float32)); fresh.raycasting(k, mu, frame)
        vd, nd = fresh.vertex_normal()
        both = (ns[..., 0] != -2) & (nd[..., 0] != -2)
        carried = vs[both].astype(np.float64) @ R.T + t * voxel
        d = np.linalg.norm(carried - vd[both].astype(np.float64), axis=1) / voxel
        return {"pixels_source": int((ns[..., 0] != -2).sum()), "pixels_both": int(both.sum()),
                "distance_voxels_median": round(float(np.median(d)), 4), "distance_voxels_p99": round(float(np.percentile(d, 99)), 4)}
    finally:
        fresh.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--reloads", type=int, default=5)
    ap.add_argument("--file-route-res", type=int, default=512, help="the resolution at which the file route is timed (dense layout); 0: never")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_rigid_bench.jsonl"))
    ap.add_argument("--quick", action="store_true", help="no file route, no geometry, nothing written (for a rocprofv3 run)")
    args = ap.parse_args()
    log = JsonLines()
    tmp = tempfile.mkdtemp(prefix="merge_rigid_bench")
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
            src_coords = src.blocks()[0]
            for name, (R, t) in transforms(res).items():
                pull = pull_of(R, t)
                counts = np.zeros(10, np.int64)
                samples = []
                for _ in range(args.reloads):
                    dst.load(base); dst.sync()
                    t0 = time.perf_counter()
                    dst._check(dst.lib.se_hip_merge_map_rigid(dst._h, src._h, pull.ctypes.data, C.addressof(rule), counts.ctypes.data))
                    samples.append((time.perf_counter() - t0) * 1e6)
                after = dst.counts()
                med = float(np.median(samples))
                out = {**map_tag(res, SDF, pooled), "transform": name, "dst_blocks": nb, "dst_nodes": nn, "src_blocks": sb, "src_nodes": sn,
                       "counts": counts.tolist(), "candidate_blocks": candidate_blocks(src_coords, R, t, res),
                       "participating_blocks": int(counts[0] + counts[1]), "blocks_after": after[0], "nodes_after": after[1],
                       "merge_us": round(med, 1), "merge_us_min": round(min(samples), 1), "merge_us_samples": [round(v, 1) for v in samples],
                       "observed_samples_per_s": round(float(counts[2]) / (med * 1e-6), 0)}
                if not args.quick and res == args.file_route_res and not pooled:
                    device = values_of(dst)
                    out["file_route"] = file_route(dst, src, res, pull, base, tmp)
                    assert (out["file_route"]["blocks_after"], out["file_route"]["nodes_after"]) == after, (out["file_route"], after)
                    assert all((u == v).all() for u, v in zip(device, values_of(dst))), "the file route's map differs from the device's"
                    out["speedup_vs_file_route"] = round(out["file_route"]["total_s"] * 1e6 / out["merge_us"], 1)
                log.emit(out)
            if not args.quick and not pooled:
                R, t = transforms(res)["yaw"]
                log.emit({**map_tag(res, SDF, pooled), "geometry": "yaw", **geometry(src, res, pooled, R, t, k, mu, args.frames - 1)})
            dst.close(); src.close()
    os.remove(base)
    if not args.quick:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        log.write(args.out)


if __name__ == "__main__":
    main()
