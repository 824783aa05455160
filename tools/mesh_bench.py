#!/usr/bin/env python3
"""Live meshing per block (se_hip_mesh_blocks) against the export path, on maps built from the room and stress streams (640x480, 4.8 m, SDF,
dense grid).  For every stream and volume resolution, in one process and on the same map:
  a  the export path: wall time of se_hip_mesh_count + se_hip_mesh_download (allocation and copy included: what a caller waits for), and
     the count pass alone between HIP events (one k_mesh launch; the download's launch does the same reads and the stores on top, so
     twice this figure is a lower bound of the two launches);
  b  se_hip_mesh_blocks, whole volume, to device memory, between HIP events (begin + k_mesh_blocks + end);
  c  the same restricted to the last frame's view;
  d  streaming frames/s (se_hip_frame on a streaming handle, device images) without and with one view-restricted update (the last ten
     views) every ten frames, in alternating segments.
One JSON line per stream and resolution.  Kernel durations come from a separate run under rocprofv3 --kernel-trace --stats."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from supereight_amd.pipeline import SDF, DenseSLAMPipeline, _MeshOut  # noqa: E402
from supereight_amd.synthetic import make_stream, to_colmajor  # noqa: E402

W, H, DIM, MU = 640, 480, 4.8, 0.1


def events(stream, reps, fn):
    """Mean and spread [us] of fn's device time over `reps` single timings, after a warm-up."""
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return round(float(np.median(out)), 1), round(float(min(out)), 1), round(float(max(out)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=str, default="512,1024")
    ap.add_argument("--streams", type=str, default="room,stress")
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--segment", type=int, default=60, help="frames per streaming segment (d)")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    lines = []
    for kind in args.streams.split(","):
        s = make_stream(kind, W, H, DIM, holes=False)
        k = np.ascontiguousarray(s.k, np.float32)
        depth = torch.from_numpy(np.stack([s.depth(f) for f in range(args.frames)])).to(dev)
        poses = [np.asarray(s.pose(f), np.float32) for f in range(args.frames)]
        pingpong = list(range(args.frames)) + list(range(args.frames - 2, 0, -1))
        for res in [int(r) for r in args.res.split(",")]:
            p = DenseSLAMPipeline((W, H), res, DIM, field_type=SDF, streaming=True)
            p.set_stream(stream.cuda_stream)
            for f in range(args.frames):
                p.frame(depth[f].data_ptr(), to_colmajor(poses[f]), k, MU, f)
            p.sync()
            nb, _ = p.counts()
            rec = {"stream": kind, "res": res, "blocks": nb, "frames": args.frames}
            # a: the export path
            n = C.c_int64()
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                tri = p.mesh()
                t.append((time.perf_counter() - t0) * 1e6)
            rec["triangles"] = len(tri)
            rec["a_export_wall_us"] = round(float(np.median(t)), 1)
            rec["a_count_pass_us"], rec["a_count_min_us"], rec["a_count_max_us"] = events(stream, args.reps, lambda: p._check(p.lib.se_hip_mesh_count(p._h, C.byref(n))))
            rec["a_two_launches_lower_bound_us"] = round(2 * rec["a_count_pass_us"], 1)
            # b, c: the device entry with exact capacities
            whole = p.mesh_blocks(device=True)
            nbl, nt = len(whole["coords"]), len(whole["triangles"])
            assert nt == len(tri)
            hd = torch.zeros(4, dtype=torch.int64, device=dev)
            out = _MeshOut(whole["triangles"].data_ptr(), nt, whole["coords"].data_ptr(), whole["ranges"].data_ptr(), nbl, hd.data_ptr())
            sel_all, keep0 = p._mesh_select(None, None, False)
            sel_view, keep1 = p._mesh_select(None, [(poses[-1], k)], False)
            sel_ten, keep2 = p._mesh_select(None, [(poses[f], k) for f in range(args.frames - 10, args.frames)], False)
            rec["b_whole_us"], rec["b_min_us"], rec["b_max_us"] = events(stream, args.reps, lambda: p._check(p.lib.se_hip_mesh_blocks(p._h, C.byref(sel_all), C.byref(out))))
            rec["c_last_view_us"], rec["c_min_us"], rec["c_max_us"] = events(stream, args.reps, lambda: p._check(p.lib.se_hip_mesh_blocks(p._h, C.byref(sel_view), C.byref(out))))
            p.sync()
            rec["c_blocks"], rec["c_triangles"] = int(hd[2]), int(hd[3])
            rec["b_over_a_lower_bound"] = round(rec["b_whole_us"] / rec["a_two_launches_lower_bound_us"], 3)
            # d: streaming, alternating segments without / with an update every ten frames
            fps = {False: [], True: []}
            f = args.frames
            for seg in range(4):
                upd = bool(seg & 1)
                p.sync()
                t0 = time.perf_counter()
                for i in range(args.segment):
                    j = pingpong[f % len(pingpong)]
                    p.frame(depth[j].data_ptr(), to_colmajor(poses[j]), k, MU, f)
                    f += 1
                    if upd and (i + 1) % 10 == 0:
                        last = [pingpong[(f - 1 - q) % len(pingpong)] for q in range(10)]
                        sel, keep = p._mesh_select(None, [(poses[q], k) for q in last], False)
                        p._check(p.lib.se_hip_mesh_blocks(p._h, C.byref(sel), C.byref(out)))
                p.sync()
                fps[upd].append(args.segment / (time.perf_counter() - t0))
            rec["d_fps_without"] = [round(v, 1) for v in fps[False]]
            rec["d_fps_with_update_every_10"] = [round(v, 1) for v in fps[True]]
            rec["d_overflow_free"] = bool(int(hd[0]) == int(hd[2]))     # (the map grew past the buffers sized before the segments if False)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            p.close()
            del whole, hd
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fo:
            for rec in lines:
                fo.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
