#!/usr/bin/env python3
"""Throughput of batched ray casts (se_hip_cast_rays) on maps built from bench.py's synthetic room stream (640x480, 4.8 m).

For every volume resolution, brick layout (dense grid / pooled) and field type (SDF / OFusion) it builds the map from --frames frames, then
times batches of --sizes rays through the device entry with HIP events on the handle's stream (the mean of --reps back-to-back batches,
all three outputs) for two ray sets:
  camera   the 640x480 rays of the last frame's camera (origin, normalised pixel directions, near 0.4 / far 4.0) repeated to the batch size:
           coherent, what k_raycast casts
  random   origins uniform in the volume, uniform random unit directions, near 0.4 / far 4.0: incoherent
and, once per map, the camera raycast of the same pose (se_hip_raycast: k_raycast with its beam start and tile schedule) for the ratio on
coherent rays.  One JSON line per measurement.  Kernel durations come from a separate run under rocprofv3 --kernel-trace --stats."""
import argparse
import ctypes as C

import numpy as np
import torch

from query_bench_common import DIM, H, W, JsonLines, build_map, map_tag, timed   # (puts the repository root on sys.path)
from supereight_amd.pipeline import OFUSION, SDF, _RayOut


def camera_rays(pose, k, dev):
    """raycastKernel's rays for pose * K^-1, formed in float32 on the device (a benchmark input: bits need not match the camera's)."""
    fx, fy, cx, cy = (float(v) for v in k)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    d = torch.stack([(xs - cx) / fx, (ys - cy) / fy, torch.ones_like(xs)], -1).reshape(-1, 3)
    R = torch.from_numpy(np.ascontiguousarray(pose[:3, :3], np.float32)).to(dev)
    d = d @ R.T
    d = d / torch.linalg.norm(d, dim=1, keepdim=True)
    r = torch.empty((W * H, 8), device=dev)
    r[:, 0:3] = torch.from_numpy(np.ascontiguousarray(pose[:3, 3], np.float32)).to(dev)
    r[:, 3:6] = d
    r[:, 6], r[:, 7] = 0.4, 4.0
    return r


def random_rays(n, gen, dev):
    r = torch.empty((n, 8), device=dev)
    r[:, 0:3] = torch.rand((n, 3), generator=gen, device=dev) * DIM
    d = torch.randn((n, 3), generator=gen, device=dev)
    r[:, 3:6] = d / torch.linalg.norm(d, dim=1, keepdim=True)
    r[:, 6], r[:, 7] = 0.4, 4.0
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=str, default="512,1024")
    ap.add_argument("--sizes", type=str, default="4096,65536,1048576,4194304")
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    log = JsonLines()
    emit = log.emit
    gen = torch.Generator(device=dev)
    for res in [int(r) for r in args.res.split(",")]:
        for field in (SDF, OFUSION):
            for pooled in (False, True):
                p, s, mu = build_map(res, field, pooled, args.frames)
                p.sync()
                p.set_stream(stream.cuda_stream)       # the batches run on torch's stream, timed by its events
                nb, _ = p.counts()
                pose = s.pose(args.frames - 1)
                tag = dict(map_tag(res, field, pooled), blocks=nb)
                p.setPose(pose)
                us_cam = timed(stream, args.reps, lambda: p.raycasting(s.k, mu, args.frames))
                emit(dict(tag, kernel="k_raycast", rays=W * H, set="camera", us_per_batch=round(us_cam, 2), mrays_per_s=round(W * H / us_cam, 1)))
                cam = camera_rays(pose, s.k, dev)
                for n in [int(v) for v in args.sizes.split(",")]:
                    gen.manual_seed(1234)
                    sets = {"camera": cam.repeat((n + W * H - 1) // (W * H), 1)[:n].contiguous(), "random": random_rays(n, gen, dev)}
                    outs = {"hit": torch.empty((n, 4), device=dev), "normal": torch.empty((n, 3), device=dev),
                            "status": torch.empty(n, dtype=torch.uint8, device=dev)}
                    o = _RayOut(outs["hit"].data_ptr(), outs["normal"].data_ptr(), outs["status"].data_ptr())
                    for name, x in sets.items():
                        us = timed(stream, args.reps, lambda: p._check(p.lib.se_hip_cast_rays(p._h, x.data_ptr(), n, mu, C.byref(o))))
                        hits = int(((outs["status"] & 4) != 0).sum())
                        rec = dict(tag, kernel="k_cast_rays", rays=n, set=name, us_per_batch=round(us, 2), mrays_per_s=round(n / us, 1),
                                   hit_frac=round(hits / n, 3))
                        if name == "camera" and n >= W * H:
                            rec["ratio_to_k_raycast"] = round((W * H / us_cam) / (n / us), 2)    # k_raycast's rays/s over the batch's
                        emit(rec)
                    del sets, outs
                p.sync()
                p.close()
                torch.cuda.empty_cache()
    if args.out:
        log.write(args.out)


if __name__ == "__main__":
    main()
