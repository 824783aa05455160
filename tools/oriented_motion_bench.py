#!/usr/bin/env python3
"""Cost of batched oriented motion collision queries (se_hip_collide_oriented_motions) against the two ways the question could be asked
before, on the map bench.py measures: its synthetic room stream (640x480, 4.8 m, --frames frames) fused into a dense 512^3 SDF volume.

65 536 motions of a 0.6 x 0.4 x 0.3 m box (half extents 0.3, 0.2, 0.15 m) at uniform random yaws -- half of the centres within 0.5 m of
raycast hit vertices of the last frame, half uniform in the volume -- moved by --lengths metres (0.25 and 1) in a horizontal direction drawn
independently of the yaw.  For each length, on the same map in the same process through the device entries:
  exact        se_hip_collide_oriented_motions with status, t_first and t_exact
  status       the same call with status only (the search stops at the first occupied step)
  chain        the question as it could be asked before: se_hip_collide_oriented at K + 1 poses every half voxel along each segment
               (K = ceil(length / half a voxel), centres rounded to the sub-unit), all poses of all motions in one batch; the status of a
               motion is the min over its poses.  chain_differs is the share of motions whose chain status is not the exact one,
               chain_misses the share where it is less severe (something between two samples is missed; the rest comes from the rounded
               sample centres, which leave the segment by up to half a sub-unit)
  bbox         se_hip_collide_motions on the bounding axis-aligned box of the box, in whole voxels, moved by the displacement rounded away
               from zero to whole voxels and padded where that rounding moved it (a superset of the sweep).  bbox_false_blocked is the
               share of the motions it reports occupied that the exact query reports not occupied
The handle runs on a torch stream and the events are recorded on that stream: after --warmup calls, --windows windows of --reps back-to-back
calls each; the variants alternate window by window; the median window and all windows are recorded.  One JSON line per length."""
import argparse
import ctypes as C
import os

import numpy as np
import torch

from query_bench_common import DIM, ROOT, JsonLines, build_map, hit_vertices, map_tag   # (puts the repository root on sys.path)
from supereight_amd.pipeline import COLLISION_OCCUPIED, ORIENTED_SUB, SDF, _CollideTest, _MotionOut, _OrientedMotionOut, oriented_motions

HALF_M = np.array([0.3, 0.2, 0.15])


def yaw_rotations(a):
    c, s, o, l = np.cos(a), np.sin(a), np.zeros_like(a), np.ones_like(a)
    return np.stack([np.stack([c, -s, o], -1), np.stack([s, c, o], -1), np.stack([o, o, l], -1)], 1)


def motion_set(res, hits, rng, length, n):
    centres = np.concatenate([hits[rng.choice(len(hits), n // 2)] + rng.uniform(-0.5, 0.5, (n // 2, 3)), rng.uniform(0.3, DIM - 0.3, (n - n // 2, 3))])
    heading = rng.uniform(0, 2 * np.pi, n)
    d = np.stack([np.cos(heading), np.sin(heading), np.zeros(n)], 1) * length
    return oriented_motions(centres, yaw_rotations(rng.uniform(0, 2 * np.pi, n)), np.tile(HALF_M, (n, 1)), d, DIM, res)


def chain_boxes(d_mo, step_sub):
    """The boxes of every motion at K + 1 evenly spaced poses, K = ceil(|d| / step) (>= 1), centres rounded to the nearest sub-unit, made on
    the device: (int32 [sum, 12], the motion of each box, the largest K)."""
    m = d_mo.long()
    k = torch.clamp(torch.ceil(torch.linalg.vector_norm(m[:, 12:15].double(), dim=1) / step_sub), min=1).long()
    owner = torch.repeat_interleave(torch.arange(len(m), device=m.device), k + 1)
    j = torch.arange(len(owner), device=m.device) - (torch.cumsum(k + 1, 0) - (k + 1))[owner]
    boxes = m[owner, :12].contiguous()
    boxes[:, 0:3] += torch.round(m[owner, 12:15].double() * (j.double() / k[owner].double())[:, None]).long()
    return boxes.int().contiguous(), owner, int(k.max())


def bounding_motions(mo):
    """lo, side, d of se_hip_collide_motions in whole voxels, a superset of the sweep: the bounding box of the box, the displacement rounded
    away from zero, and -- where that rounding moved it -- one more voxel on either side of that axis (at parameter t the rounded box is ahead
    of the exact one by less than a voxel)."""
    m = mo.astype(np.int64)
    ext = np.abs(m[:, 3:12].reshape(-1, 3, 3)).sum(1)
    d = np.sign(m[:, 12:15]) * (-((-np.abs(m[:, 12:15])) // ORIENTED_SUB))
    pad = (d * ORIENTED_SUB != m[:, 12:15]).astype(np.int64)
    lo = (m[:, 0:3] - ext) // ORIENTED_SUB - pad
    hi = -((-(m[:, 0:3] + ext)) // ORIENTED_SUB) + pad
    return np.ascontiguousarray(np.concatenate([lo, hi - lo, d], 1).astype(np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--motions", type=int, default=65536)
    ap.add_argument("--lengths", type=float, nargs="+", default=[0.25, 1.0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "oriented_motion_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    log = JsonLines()
    res, n = args.res, args.motions
    p, _, _ = build_map(res, SDF, False, args.frames)
    hits = hit_vertices(p)
    p.sync()
    stream = torch.cuda.Stream(dev)
    p.set_stream(stream.cuda_stream)       # the queries run on this stream, timed by its events
    test = _CollideTest(0.0, 0)
    stop = COLLISION_OCCUPIED

    def window(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.reps):
            call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.reps

    for length in args.lengths:
        mo = motion_set(res, hits, rng, length, n)
        d_mo, d_bb = (torch.from_numpy(a).to(dev) for a in (mo, bounding_motions(mo)))
        d_boxes, owner, k_max = chain_boxes(d_mo, ORIENTED_SUB // 2)
        st, st_alone, st_bb = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(3))
        tf, tf_bb = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2))
        te = torch.empty((n, 2), dtype=torch.int64, device=dev)
        st_chain = torch.empty(len(d_boxes), dtype=torch.uint8, device=dev)
        out = _OrientedMotionOut(st.data_ptr(), tf.data_ptr(), te.data_ptr())
        alone = _OrientedMotionOut(st_alone.data_ptr(), None, None)
        out_bb = _MotionOut(st_bb.data_ptr(), tf_bb.data_ptr())
        torch.cuda.synchronize()
        calls = {
            "exact": lambda: p._check(p.lib.se_hip_collide_oriented_motions(p._h, d_mo.data_ptr(), n, C.byref(test), stop, C.byref(out))),
            "status": lambda: p._check(p.lib.se_hip_collide_oriented_motions(p._h, d_mo.data_ptr(), n, C.byref(test), stop, C.byref(alone))),
            "chain": lambda: p._check(p.lib.se_hip_collide_oriented(p._h, d_boxes.data_ptr(), len(d_boxes), C.byref(test), st_chain.data_ptr())),
            "bbox": lambda: p._check(p.lib.se_hip_collide_motions(p._h, d_bb.data_ptr(), n, C.byref(test), stop, C.byref(out_bb))),
        }
        for call in calls.values():
            for _ in range(args.warmup):
                call()
        stream.synchronize()
        runs = {k: [] for k in calls}
        for _ in range(args.windows):
            for k, call in calls.items():
                runs[k].append(round(window(call), 2))
        stream.synchronize()
        s_ex, s_alone, s_bb, t_ex = st.cpu().numpy(), st_alone.cpu().numpy(), st_bb.cpu().numpy(), tf.cpu().numpy()
        s_chain = torch.full((n,), 255, dtype=torch.int32, device=dev).scatter_reduce(0, owner, st_chain.int(), "amin").cpu().numpy()
        assert (s_alone == s_ex).all() and (s_bb <= s_ex).all()
        rec = {**map_tag(res, SDF, False), "length_m": length, "motions": n, "chain_boxes": int(len(d_boxes)), "chain_poses_max": k_max + 1}
        for k, v in runs.items():
            rec[k + "_us_per_batch"] = round(float(np.median(v)), 2)
            rec[k + "_us_windows"] = v
        rec["exact_ns_each"] = round(rec["exact_us_per_batch"] * 1e3 / n, 1)
        rec["status_ns_each"] = round(rec["status_us_per_batch"] * 1e3 / n, 1)
        rec["chain_over_exact"] = round(rec["chain_us_per_batch"] / rec["exact_us_per_batch"], 3)
        rec["bbox_over_exact"] = round(rec["bbox_us_per_batch"] / rec["exact_us_per_batch"], 3)
        rec["chain_differs"] = round(float((s_chain != s_ex).mean()), 5)
        rec["chain_misses"] = round(float((s_chain > s_ex).mean()), 5)          # less severe than the truth: something between two samples
        rec["bbox_false_blocked"] = round(float(((s_bb == 0) & (s_ex != 0)).sum() / max(1, int((s_bb == 0).sum()))), 5)
        rec["status_counts"] = {str(k): int((s_ex == k).sum()) for k in (0, 1, 2, 255)}
        rec["blocked_on_the_way"] = int(((t_ex > 0) & (t_ex < 1)).sum())
        log.emit(rec)
    p.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    log.write(args.out)


if __name__ == "__main__":
    main()
