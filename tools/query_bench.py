#!/usr/bin/env python3
"""Throughput of batched map queries (se_hip_query_points) on maps built from bench.py's synthetic room stream (640x480, 4.8 m).

For every volume resolution, brick layout (dense grid / pooled) and field type (SDF / OFusion) it builds the map from --frames
frames, then times batches of --sizes points through the device entry with HIP events on the handle's stream (the mean of --reps
back-to-back batches) for two point sets:
  uniform   uniform in the volume
  surface   raycast hit vertices of the last frame plus uniform 2-voxel jitter (clustered, what a planner asks near surfaces)
and two output selections: interp + grad (the planner's case) and all five outputs.  One JSON line per measurement.
Kernel durations come from a separate run under rocprofv3 --kernel-trace --stats (k_query_points in its kernel_stats.csv)."""
import argparse
import ctypes as C

import numpy as np
import torch

from query_bench_common import DIM, JsonLines, build_map, hit_vertices, map_tag, timed   # (puts the repository root on sys.path)
from supereight_amd.pipeline import OFUSION, SDF, _QueryOut


def algorithmic_bytes(field, pooled, outputs):
    """Bytes a point needs at the least: its 12 input bytes, the voxels each output reads (fine / coarse: one voxel, x + y; interp: 8 x values;
    grad: the 32 distinct x values of its stencil), one 4-byte index entry per distinct block when pooled (1 for fine, 1 for interp or grad in the
    common case of a cell inside one block), and the bytes written."""
    y = 1 if field == SDF else 4
    b = 12
    if "fine" in outputs or "coarse" in outputs:
        b += 4 + y + (4 if pooled else 0)
    if "interp" in outputs:
        b += 8 * 4 + (4 if pooled else 0)
    if "grad" in outputs:
        b += 32 * 4 + (4 if pooled and "interp" not in outputs else 0)
    b += sum({"fine": 8, "coarse": 8, "interp": 4, "grad": 12, "status": 1}[k] for k in outputs)
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=str, default="512,1024")
    ap.add_argument("--sizes", type=str, default="1048576,16777216")
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    log = JsonLines()
    gen = torch.Generator(device=dev)
    for res in [int(r) for r in args.res.split(",")]:
        vox = DIM / res
        for field in (SDF, OFUSION):
            for pooled in (False, True):
                p, _, _ = build_map(res, field, pooled, args.frames)
                hits = hit_vertices(p)
                p.sync()
                p.set_stream(stream.cuda_stream)       # the queries run on torch's stream, timed by its events
                nb, _ = p.counts()
                hits_d = torch.from_numpy(np.ascontiguousarray(hits)).to(dev)
                for n in [int(v) for v in args.sizes.split(",")]:
                    gen.manual_seed(1234)
                    pts = {"uniform": torch.rand((n, 3), generator=gen, device=dev) * DIM}
                    idx = torch.randint(0, hits_d.shape[0], (n,), generator=gen, device=dev)
                    pts["surface"] = (hits_d[idx] + (torch.rand((n, 3), generator=gen, device=dev) * 4 - 2) * vox).contiguous()
                    outs = {"fine": torch.empty((n, 2), device=dev), "coarse": torch.empty((n, 2), device=dev), "interp": torch.empty(n, device=dev),
                            "grad": torch.empty((n, 3), device=dev), "status": torch.empty(n, dtype=torch.uint8, device=dev)}
                    for sel in (("interp", "grad"), ("fine", "coarse", "interp", "grad", "status")):
                        q = _QueryOut(*(outs[k].data_ptr() if k in sel else None for k in ("fine", "coarse", "interp", "grad", "status")))
                        for name, x in pts.items():
                            us = timed(stream, args.reps, lambda: p._check(p.lib.se_hip_query_points(p._h, x.data_ptr(), n, C.byref(q))))
                            bpp = algorithmic_bytes(field, pooled, sel)
                            log.emit(dict(map_tag(res, field, pooled), blocks=nb, points=n, set=name, outputs="+".join(sel), us_per_batch=round(us, 2),
                                          mpoints_per_s=round(n / us, 1), alg_bytes_per_point=bpp, alg_gb_per_s=round(n * bpp / us / 1e3, 1)))
                    del pts, outs, idx
                p.sync()
                p.close()
                torch.cuda.empty_cache()
    if args.out:
        log.write(args.out)


if __name__ == "__main__":
    main()
