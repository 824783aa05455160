#!/usr/bin/env python3
"""Cost of exact segment traces (se_hip_trace_segments) on maps built from bench.py's synthetic room stream (640x480, 4.8 m, --frames
frames) at --res: SDF dense and SDF pooled.

Segment sets:
  views      64 candidate views x the fan of a 640x480 camera at stride 8 (4 800 rays each), 0.4 m .. 4 m: poses around the room looking
             at raycast hits of the last frame
  short      64 k random segments of 0.5 m with a uniform start in the volume
  medium     64 k random segments of 2 m
  diagonal   4 k segments from a point near one face of the volume to one near the opposite face
For every set, timed on the same map in the same run through the device entry with events around --reps back-to-back batches after --warmup
(each variant twice, the variants alternating; the mean and both runs are recorded):
  trace            all four outputs (COUNT == true: absent octants are stepped through)
  trace_nocount    status, t_first, first (COUNT == false: absent octants are left in one jump)
  cast_rays        se_hip_cast_rays on the same segments as rays (origin a, direction b - a, near 0, far |b - a|): the float march through
                   allocated blocks.  Not the same answer -- it knows no classes and no counts; it serves only as a scale.
and on the dense map, through tools/trace_bench.cpp on the very segments: se::geometry::trace_walk on one host thread over a getMap()
snapshot (the first --host-segments of each set), with counts and without, and the getMap() itself; the host answers are compared with the
device's.  One JSON line per set and map."""
import argparse
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import torch

from query_bench_common import DIM, H, ROOT, W, JsonLines, build_map, hit_vertices, map_tag   # (puts the repository root on sys.path)
from supereight_amd import build
from supereight_amd.pipeline import _MOTION_STOPS, ORIENTED_SUB, SDF, _CollideTest, _RayOut, _TraceOut, segments_from_points, view_segments
from supereight_amd.rawio import write_raw
from supereight_amd.synthetic import SyntheticStream

MU = 0.1


def look_at(eye, target):
    z = target - eye
    z = z / np.linalg.norm(z)
    x = np.cross([0.0, 0.0, 1.0], z)
    x = x / np.linalg.norm(x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, np.cross(z, x), z, eye
    return T


def segment_sets(res, hits, k, rng, n=65536):
    eyes = rng.uniform(0.25 * DIM, 0.75 * DIM, (64, 3))
    fans = [view_segments(look_at(e, hits[rng.integers(len(hits))].astype(np.float64)), k, W, H, 8, 0.4, 4.0, DIM, res)[0] for e in eyes]
    out = {"views": np.concatenate(fans)}
    for name, length in (("short", 0.5), ("medium", 2.0)):
        a = rng.uniform(0.0, DIM, (n, 3))
        d = rng.normal(size=(n, 3))
        out[name] = segments_from_points(a, a + length * d / np.linalg.norm(d, axis=1, keepdims=True), DIM, res)
    m = 4096
    a, b = rng.uniform(0.0, DIM, (m, 3)), rng.uniform(0.0, DIM, (m, 3))
    axis = rng.integers(0, 3, m)
    a[np.arange(m), axis] = rng.uniform(0.0, 0.05 * DIM, m)
    b[np.arange(m), axis] = rng.uniform(0.95 * DIM, DIM, m)
    out["diagonal"] = segments_from_points(a, b, DIM, res)
    return {name: np.ascontiguousarray(v) for name, v in out.items()}


def host_route(tmp, res, frames, sets, host_segments):
    """tools/trace_bench.cpp on the same stream and the same segments: {set: its record}."""
    build.build()
    exe = os.path.join(tmp, "trace_bench")
    lib_dir = os.path.join(ROOT, "supereight_amd")
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-DSE_FIELD_TYPE=SDF", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "trace_bench.cpp"),
                        "-o", exe, "-L" + lib_dir, "-lse_hip", "-Wl,-rpath," + lib_dir], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("g++ failed:\n" + r.stderr[-4000:])
    s = SyntheticStream(W, H, DIM, holes=False)
    raw, pf = os.path.join(tmp, "room.raw"), os.path.join(tmp, "poses.bin")
    write_raw(raw, [np.rint(np.asarray(s.depth(f), np.float64) * 1000.0).astype(np.uint16) for f in range(frames)])
    np.stack([s.pose(f) for f in range(frames)]).astype(np.float32).tofile(pf)
    args = []
    for name, seg in sets.items():
        path = os.path.join(tmp, name + ".bin")
        seg.tofile(path)
        args.append(f"{name}={path}")
    r = subprocess.run([exe, raw, pf, str(res), str(DIM), str(MU), str(host_segments)] + args, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"trace_bench exited with {r.returncode}:\n{r.stderr[-2000:]}")
    return {rec["set"]: rec for rec in (json.loads(line) for line in r.stdout.splitlines())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-segments", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    log = JsonLines()
    sets = None
    for pooled in (False, True):
        p, s, _ = build_map(args.res, SDF, pooled, args.frames)
        test = _CollideTest(0.0, 0)
        if sets is None:
            sets = segment_sets(args.res, hit_vertices(p), s.k, np.random.default_rng(1))

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

        with tempfile.TemporaryDirectory() as tmp:
            host = host_route(tmp, args.res, args.frames, sets, args.host_segments) if not pooled else {}
        for name, seg in sets.items():
            n = len(seg)
            d_seg = torch.from_numpy(seg).to(dev)
            st = torch.empty(n, dtype=torch.uint8, device=dev)
            tf = torch.empty(n, dtype=torch.float32, device=dev)
            fi = torch.empty((n, 3), dtype=torch.int32, device=dev)
            co = torch.empty((n, 2), dtype=torch.int32, device=dev)
            metres = seg.astype(np.float64) * (DIM / (ORIENTED_SUB * args.res))
            d = metres[:, 3:6] - metres[:, 0:3]
            length = np.linalg.norm(d, axis=1, keepdims=True)
            rays = torch.from_numpy(np.concatenate([metres[:, 0:3], d / np.maximum(length, 1e-9), np.zeros((n, 1)), length], 1).astype(np.float32)).to(dev)
            hit, nrm = torch.empty((n, 4), dtype=torch.float32, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev)
            rst = torch.empty(n, dtype=torch.uint8, device=dev)
            stop = _MOTION_STOPS["occupied"]
            full, lean = _TraceOut(st.data_ptr(), tf.data_ptr(), fi.data_ptr(), co.data_ptr()), _TraceOut(st.data_ptr(), tf.data_ptr(), fi.data_ptr(), None)
            ray_out = _RayOut(hit.data_ptr(), nrm.data_ptr(), rst.data_ptr())
            calls = {
                "trace": lambda: p._check(p.lib.se_hip_trace_segments(p._h, d_seg.data_ptr(), n, C.byref(test), stop, C.byref(full))),
                "trace_nocount": lambda: p._check(p.lib.se_hip_trace_segments(p._h, d_seg.data_ptr(), n, C.byref(test), stop, C.byref(lean))),
                "cast_rays": lambda: p._check(p.lib.se_hip_cast_rays(p._h, rays.data_ptr(), n, MU, C.byref(ray_out))),
            }
            runs = {k: [] for k in calls}
            for _ in range(2):
                for k, call in calls.items():
                    runs[k].append(round(timed(call), 2))
            calls["trace"]()
            p.sync()
            s_tr, c_tr = st.cpu().numpy(), co.cpu().numpy().astype(np.int64)
            rec = {**map_tag(args.res, SDF, pooled), "set": name, "segments": n}
            for k, v in runs.items():
                rec[k + "_us_per_batch"] = round(float(np.mean(v)), 2)
                rec[k + "_us_runs"] = v
            rec["trace_ns_each"] = round(rec["trace_us_per_batch"] * 1e3 / n, 1)
            rec["trace_nocount_ns_each"] = round(rec["trace_nocount_us_per_batch"] * 1e3 / n, 1)
            rec["nocount_over_count"] = round(rec["trace_nocount_us_per_batch"] / rec["trace_us_per_batch"], 3)
            rec["cast_rays_over_trace"] = round(rec["cast_rays_us_per_batch"] / rec["trace_us_per_batch"], 3)
            rec["status_counts"] = {str(k): int((s_tr == k).sum()) for k in (0, 1, 2)}
            rec["mean_unseen"], rec["mean_empty"] = round(float(c_tr[:, 0].mean()), 2), round(float(c_tr[:, 1].mean()), 2)
            if name in host:
                h = host[name]
                m = h["host_segments"]
                rec["host_segments"] = m
                rec["host_walk_ns_each"] = round(h["walk_us"] * 1e3 / m, 1)
                rec["host_walk_nocount_ns_each"] = round(h["walk_nocount_us"] * 1e3 / m, 1)
                rec["host_getmap_us"] = h["getmap_us"]
                rec["host_differ"] = h["differ"]
                # the whole set on the host, one thread, against one device call: without and with the snapshot
                rec["host_over_trace"] = round(rec["host_walk_ns_each"] / rec["trace_ns_each"], 1)
                rec["host_with_getmap_over_trace"] = round((rec["host_walk_ns_each"] * n * 1e-3 + min(h["getmap_us"])) / rec["trace_us_per_batch"], 1)
            log.emit(rec)
        p.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    log.write(args.out)
    if any(rec.get("host_differ") for rec in log.records):
        raise SystemExit("the host walk and the device differ on some segments")


if __name__ == "__main__":
    main()
