#!/usr/bin/env python3
"""Headline benchmark: frames/sec of integration() + raycasting() on the synthetic 640x480 depth
stream into a 512^3 / 4.8 m TSDF (BASELINE.json metric; configs[1] at N=1).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A "step" is one frame of the hot path: allocation scan + integration sweep + raycast.  The depth
frames are generated before the timed region and are resident in HBM; poses are 64-byte kernel
arguments.  Exactly K steps are timed (`ms_per_step` = wall time of the timed region / K); `--sustain` adds a
second timed region on request.  N > 1 shards the image rows of ONE stream across ranks with one RCCL all-gather of the
new-block key lists per frame (supereight_amd/multi_gpu.py): total work is fixed -> "strong".

Rank 0 prints ONE JSON line.  Besides the contract fields it carries
  roofline     for the dominant kernel (largest share of GPU time): algorithmic bytes per launch
               (SURVEY.md 8(d) formulas, work counts taken from an instrumented replay of the same
               frames) / average launch duration from HIP events recorded on the launch stream
               during the timed region; peak = 8 TB/s HBM3E.
  cpu_baseline the CPU oracle (reference-equivalent OpenMP restatement, kind "port") timed on this
               host's cores on a bounded sample of the same stream (N = 1 only).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); measured copy peak ~6300 GB/s


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--dim", type=float, default=4.8)
    ap.add_argument("--mu", type=float, default=0.1)
    ap.add_argument("--field", choices=["sdf", "ofusion"], default="sdf")
    ap.add_argument("--stream", choices=["room", "stress"], default="room",
                    help="room: SURVEY 8(d)'s box room + sphere (the contract workload); stress: the ICL-like stress stream of supereight_amd/synthetic.py "
                         "(scene clipped by the volume, occluders, cm-scale motion with a 180 deg pan, sensor noise, ICL intrinsics)")
    ap.add_argument("--icl-like", action="store_true",
                    help="the analytic stream seen through the ICL-NUIM camera (-k 481.2,-480,320,240: negative fy), BASELINE.json configs 1 / 3 without the data set")
    ap.add_argument("--raw", type=str, default=os.environ.get("SE_ICL_RAW", ""), help="SLAMBench .raw depth stream (e.g. ICL-NUIM living_room_traj2_loop) instead of the synthetic one")
    ap.add_argument("--traj", type=str, default=os.environ.get("SE_ICL_TRAJ", ""), help="ground-truth trajectory for --raw (... tx ty tz qx qy qz qw per line)")
    ap.add_argument("--init-pose", type=str, default="0.34,0.5,0.24", help="initial position as fractions of the volume edge (README.md:80 of the reference: -p 0.34,0.5,0.24)")
    ap.add_argument("--no-events", action="store_true", help="do not record per-kernel HIP events in the timed region")
    ap.add_argument("--event-stride", type=int, default=10,
                    help="record per-kernel HIP events on every n-th timed frame (1 = every frame; events cost host time)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-frames", type=int, default=20, help="timed frames of the CPU baseline sample")
    ap.add_argument("--cpu-reps", type=int, default=4, help="repetitions of the CPU baseline sample (the fastest is reported, all are listed)")
    ap.add_argument("--sustain", type=int, default=0, help="N = 1: after the K contract steps keep going, in a second timed region, until this many frames have been timed in total (0 = off)")
    ap.add_argument("--no-streaming", action="store_true", help="N = 1: the eager two-queue schedule instead of the one-queue streaming schedule (se_hip_set_streaming)")
    ap.add_argument("--sharded-streaming", action="store_true",
                    help="N > 1: the one-queue schedule for the row-sharded replicas too (all-gather and commit behind the fused launch on the main stream); "
                         "default is the two-queue plan, whose all-gather hides behind the raycast (DESIGN.md section 7)")
    ap.add_argument("--no-prewarm", action="store_true", help="skip the untimed GPU warm-up on a scratch map before the warm-up frames (see prewarm())")
    ap.add_argument("--shard-sweep", action="store_true", help="N > 1: owner-computes integration + brick all-gather instead of the replicated sweep (SURVEY 8e option 4; DESIGN.md section 7: measured slower, off by default)")
    ap.add_argument("--no-closed-loop", action="store_true", help="skip the value_closed_loop leg (profiling runs: nothing behind the timed loop)")
    ap.add_argument("--no-modes", action="store_true", help="skip the extra N = 1 legs (closed loop, tracking on, pooled bricks)")
    ap.add_argument("--mode-frames", type=int, default=60, help="timed frames of each extra leg")
    ap.add_argument("--config4", action="store_true", help="also run BASELINE configs[3] (1280x960 -> 2048^3) with the same rank layout and print it beside the contract line (default on for N > 1)")
    ap.add_argument("--no-config4", action="store_true", help="N > 1: skip the configs[3] leg")
    ap.add_argument("--config4-steps", type=int, default=20)
    ap.add_argument("--no-replicas", action="store_true", help="N > 1: skip the replicas-only leg (independent streams per GPU, the throughput upper bound of SURVEY 8e)")
    ap.add_argument("--detail", type=str, default="", help="write a detailed JSON report to this path")
    ap.add_argument("--dump-outputs", type=str, default="", metavar="DIR",
                    help="after the timed steps write what the last timed step computed (raycast images, map bricks) to DIR/<name>.npy; see dump_outputs()")
    return ap.parse_args()


def algorithmic_bytes(stats: dict, frames: int, W: int, H: int, voxel_bytes: int, value_bytes: int = 0) -> dict:
    """per-launch algorithmic bytes of each kernel (every kernel is launched once per
    frame), from work counts summed over the timed frames.  voxel_bytes = sizeof(voxel) of the
    reference layout (8 SDF, 16 OFusion).  value_bytes (device-layout figures only): what an interpolation / gradient
    corner costs when it reads the voxel's x alone (4) -- 0 = a whole voxel, as SURVEY 8(d) counts it."""
    n = max(1, frames)
    vb = value_bytes or voxel_bytes
    # A_int = N_swept*512*sizeof(voxel)*2 + W*H*4 + N_nodes*8*sizeof(voxel)*2 (every node is swept every frame)
    a_int = stats["swept"] / n * 512 * voxel_bytes * 2 + W * H * 4 + stats["nodes"] * 8 * voxel_bytes * 2
    a_alloc = W * H * 4 + stats["probes"] / n * 4
    a_ray = W * H * 24 + (stats["gets"] * voxel_bytes + (8 * stats["interps"] + 32 * stats["grads"]) * vb) / n
    return {"integrate": a_int, "alloc_scan": a_alloc, "raycast": a_ray}


DUMP_MAX_BYTES = 60_000_000   # --dump-outputs: all arrays together (under 64 MB with the .npy headers)
DUMP_SEED = 0                 # the fixed sample of bricks / nodes when the whole map does not fit


def _sample(n: int, m: int) -> np.ndarray:
    """indices of a fixed, seeded sample of m out of n rows (all rows when n <= m), ascending"""
    if n <= m:
        return np.arange(n)
    return np.sort(np.random.default_rng(DUMP_SEED).choice(n, m, replace=False))


def dump_outputs(out_dir: str, p) -> dict:
    """What a caller of integration() + raycasting() receives after the last timed frame, as float32 / float64 .npy files:
      vertex, normal            (H, W, 3) float32 raycast images (normal.x == -2: no hit)
      block_coords              (nb, 3) brick coordinates of every allocated block, key order (float64, exact)
      block_active              (nb,) VoxelBlock::active_ flags
      block_index               (m,) rows of block_coords whose voxel planes follow (a fixed seeded sample when the map is large)
      block_x, block_y          (m, 512) voxel planes of those blocks (SDF: x = tsdf, y = weight; OFusion: x = log-odds, y = time stamp)
      node_side                 (nn,) edge of every octree node, key order
      node_x, node_y            (nn', 8) node values of a fixed seeded sample (node_index)
    Inputs are generated from fixed seeds, so two builds run with the same arguments can be compared file for file."""
    v, n = p.vertex_normal()
    coords, x, y, act = p.blocks()
    _, side, nx, ny = p.nodes()
    arrays = {"vertex": v, "normal": n, "block_coords": coords.astype(np.float64), "block_active": act.astype(np.float32),
              "node_side": side.astype(np.float64)}
    fixed = sum(a.nbytes for a in arrays.values()) + 8 * (len(coords) + len(side))     # + the two index arrays at most
    room = DUMP_MAX_BYTES - fixed
    if room <= 0:
        raise SystemExit(f"--dump-outputs: images and key lists alone are {fixed} bytes (> {DUMP_MAX_BYTES})")
    # bricks get 7/8 of what is left, nodes the rest (a brick row pair is 4 KiB, a node row pair 64 B)
    bi = _sample(len(coords), (room * 7 // 8) // (2 * 512 * 4))
    ni = _sample(len(side), (room // 8) // (2 * 8 * 4))
    arrays.update({"block_index": bi.astype(np.float64), "block_x": x[bi], "block_y": y[bi],
                   "node_index": ni.astype(np.float64), "node_x": nx[ni], "node_y": ny[ni]})
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_MAX_BYTES, total
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a))
    return {"dir": out_dir, "files": sorted(arrays), "bytes": int(total), "blocks": len(coords), "blocks_dumped": len(bi),
            "nodes": len(side), "nodes_dumped": len(ni)}


def make_stream(args, n_frames: int = 0):
    """Frame source of the run: SLAMBench .raw + ground truth (configs 1, 3) or the analytic stream."""
    if args.raw:
        from supereight_amd.rawio import RawStream
        from supereight_amd.synthetic import intrinsics
        if not args.traj:
            raise SystemExit("--raw needs --traj (ground-truth poses are injected, as the reference's apps do with -g)")
        ip = [float(v) * args.dim for v in args.init_pose.split(",")]
        st = RawStream(args.raw, args.traj, intrinsics(args.width, negative_fy=True), ip, max_frames=n_frames)
        if (st.width, st.height) != (args.width, args.height):
            raise SystemExit(f"{args.raw}: frames are {st.width}x{st.height}, --width/--height say {args.width}x{args.height}")
        if n_frames and len(st) < n_frames:
            raise SystemExit(f"{args.raw}: {len(st)} frames, {n_frames} needed (--steps / --warmup)")
        return st, f"SLAMBench .raw stream {os.path.basename(args.raw)} (ICL-NUIM camera, negative fy)"
    from supereight_amd.synthetic import StressStream, SyntheticStream
    if args.stream == "stress":
        return StressStream(args.width, args.height, args.dim), "synthetic ICL-like stress stream (scene clipped by the volume, occluders, ~1.3 cm + 2 deg / frame with a 180 deg pan, 1 mm noise, ICL-NUIM camera)"
    name = "synthetic room+sphere depth stream" + (" through the ICL-NUIM camera (negative fy)" if args.icl_like else "")
    return SyntheticStream(args.width, args.height, args.dim, negative_fy=args.icl_like), name


def host_cpu():
    """(model name, physical cores, logical CPUs) of the box from /proc/cpuinfo."""
    model, cores, logical = "unknown", set(), 0
    try:
        phys = core = None
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name") and model == "unknown":
                model = line.split(":", 1)[1].strip()
            elif line.startswith("processor"):
                logical += 1
            elif line.startswith("physical id"):
                phys = line.split(":", 1)[1].strip()
            elif line.startswith("core id"):
                core = line.split(":", 1)[1].strip()
                cores.add((phys, core))
    except OSError:
        pass
    return model, (len(cores) or logical or 1), (logical or 1)


def cpu_baseline(args, n_timed: int):
    """Times the CPU oracle on frames 0..3 (warm-up, executed but excluded as in SURVEY 8(d)) plus
    n_timed frames of the same stream; fps = n / sum(t_integration + t_raycasting)."""
    from oracle import binding
    try:
        binding.load(native=True)
        native = True
    except Exception:
        native = False
    field = binding.SDF if args.field == "sdf" else binding.OFUSION
    model, physical, logical = host_cpu()
    probe = binding.OraclePipeline(field, args.res, args.dim, args.width, args.height, native=native)
    avail = probe.lib.so_num_threads()          # what the OpenMP runtime may use in this container
    probe.close()
    # The box is shared and has two sockets: 128 threads over both are not always faster than 64 on one, and single
    # repetitions vary by several x with the other tenants' load.  Every repetition of every thread count is listed;
    # the figure reported is the MEDIAN repetition of the better thread count, the fastest repetition stands beside it.
    cands = sorted({max(1, min(physical, avail)), max(1, min(physical // 2, avail))}, reverse=True)
    by_threads = {}
    for nthr in cands:
        reps = []
        for _ in range(max(1, args.cpu_reps)):
            o = binding.OraclePipeline(field, args.res, args.dim, args.width, args.height, native=native)
            o.lib.so_set_num_threads(nthr)
            s, _ = make_stream(args, 4 + n_timed)
            t_int_sum, t_ray_sum = 0.0, 0.0
            for f in range(4 + n_timed):
                d, pose = s.depth(f), s.pose(f)
                t0 = time.perf_counter()
                o.integrate(d, pose, s.k, args.mu, f)
                t1 = time.perf_counter()
                o.raycast(pose, s.k, args.mu, f)
                t2 = time.perf_counter()
                if f >= 4:
                    t_int_sum += t1 - t0
                    t_ray_sum += t2 - t1
            o.close()
            reps.append((n_timed / (t_int_sum + t_ray_sum), t_int_sum, t_ray_sum))
        reps.sort()
        by_threads[nthr] = reps
    # the thread count whose MEDIAN repetition is fastest; the value reported is that median, the best repetition goes beside it
    threads = max(by_threads, key=lambda t: by_threads[t][len(by_threads[t]) // 2][0])
    reps = by_threads[threads]
    fps, t_int_sum, t_ray_sum = reps[len(reps) // 2]
    best = reps[-1][0]
    # one thread, a shorter sample of the same frames (SURVEY 8d asks for the 1-thread figure beside it)
    n1 = max(2, min(n_timed, 6))
    o = binding.OraclePipeline(field, args.res, args.dim, args.width, args.height, native=native)
    o.lib.so_set_num_threads(1)
    s, _ = make_stream(args, 4 + n1)
    t1 = 0.0
    for f in range(4 + n1):
        d, pose = s.depth(f), s.pose(f)
        t0 = time.perf_counter()
        o.integrate(d, pose, s.k, args.mu, f)
        o.raycast(pose, s.k, args.mu, f)
        if f >= 4:
            t1 += time.perf_counter() - t0
    o.close()
    single = n1 / t1
    return {"value": fps, "value_kind": "median repetition of the better thread count (r02 and earlier: the fastest repetition, kept as best_repetition_fps)",
            "unit": "frames/s", "cores": int(threads), "kind": "port",
            "sample": f"frames 4..{3 + n_timed} of the same stream after 4 executed warm-up frames "
                      f"({n_timed} timed frames, median of {len(reps)} repetitions, OpenMP {threads} threads, "
                      f"{'-march=native' if native else '-march=x86-64-v3'} build)",
            "cpu": f"{model}, {physical} physical cores / {logical} logical CPUs",
            "ms_integration": 1e3 * t_int_sum / n_timed, "ms_raycasting": 1e3 * t_ray_sum / n_timed,
            "all_repetitions_fps": {str(t): [r[0] for r in v] for t, v in by_threads.items()}, "best_repetition_fps": best,
            "spread": reps[-1][0] / reps[0][0],
            "single_thread": {"value": single, "unit": "frames/s", "sample": f"frames 4..{3 + n1}, 1 OpenMP thread"}}


def freeze_gc():
    """The import-time heap (torch + numpy: ~10^6 objects) moved out of the cyclic collector's sight.  Without this, a full
    collection lands a few hundred frame calls into the first loop of the process -- the allocation count of the ctypes calls
    triggers it -- and holds the interpreter for 35-60 ms, 400-700 frames' worth (profiles/r04f_stall_attribution.md).  It is
    interpreter housekeeping of this harness, not part of the measured path (a C++ caller has no collector); nothing is
    disabled: young generations are still collected."""
    import gc
    gc.collect()
    gc.freeze()


def prewarm(args, field, depth_ptrs, poses, k, device, ms: float = 90.0):
    """Untimed: keeps the GPU busy with the same kernels on a scratch map for `ms` milliseconds right before a timed
    region (the pipeline to be timed already exists by then): clocks, caches and code paths warm, so that the K timed steps
    measure the steady state (frames run 78-81 us in the first ~20 ms of load after idle, 75-76 us ever after, r03 long-run measurement).
    r02-r03 also credited this with hiding "the one 35-40 ms clock-ramp stall"; that stall is CPython's garbage collector
    (profiles/r04f_stall_attribution.md) and is dealt with where it belongs: freeze_gc() below."""
    from supereight_amd.pipeline import DenseSLAMPipeline
    p = DenseSLAMPipeline((args.width, args.height), args.res, args.dim, field_type=field, device=device)
    n = min(len(depth_ptrs), 24)
    t0 = time.perf_counter()
    f = 0
    while time.perf_counter() - t0 < ms * 1e-3:
        for _ in range(16):
            i = f % n if (f // n) % 2 == 0 else n - 1 - f % n      # ping-pong over the first frames
            p.set_depth_device(depth_ptrs[i]); p.setPose(poses[i])
            p.integration(k, 1, args.mu, f); p.raycasting(k, args.mu, f)
            f += 1
        p.sync()
    return f, p      # the caller closes the scratch pipeline AFTER its timed region: freeing 2 GiB now would idle the GPU again


def extra_modes(args, field, depth_ptrs, poses, k, warm, n, device):
    """N = 1 legs beside the headline (same frames, same library, fresh map each), frames/s:
      closed_loop  integration() + raycasting() + se_hip_sync() per frame -- the reference's own bracketing
                   (se_apps/src/benchmark.cpp:148-167): nothing of frame f+1 is issued before frame f has finished,
                   i.e. what a SLAM loop whose next pose depends on this raycast can use;
      tracking_on  the full loop tracking() -> integration() (if tracked) -> raycasting() with the ICP-tracked pose (GT pose
                   for frames 0..3 only), one se_hip_frame_tracked call + one se_hip_sync per frame; the ICP loop runs on the
                   device and hands the host one record per frame;
      pooled       the headline's pipelined loop on pooled bricks (max_blocks set: bump-allocated bricks behind the
                   index instead of one brick slot per grid cell)."""
    from supereight_amd.pipeline import DenseSLAMPipeline
    from supereight_amd.synthetic import to_colmajor
    W, H, N, dim, mu = args.width, args.height, args.res, args.dim, args.mu
    poses_cm = [to_colmajor(q) for q in poses]
    k32 = np.ascontiguousarray(k, dtype=np.float32).reshape(4)
    # (addresses of arrays held above: an array argument costs ctypes microseconds of checks per call, which a closed loop pays per frame)
    pose_at = [DenseSLAMPipeline.addr(a) for a in poses_cm]
    k_at = DenseSLAMPipeline.addr(k32)
    out = {}

    def run(label, per_frame_sync, track, **kw):
        p = DenseSLAMPipeline((W, H), N, dim, field_type=field, device=device, **kw)
        _, scratch = prewarm(args, field, depth_ptrs, poses, k, device)
        tracked = 0
        t0 = None
        for f in range(warm + n):
            if f == warm:
                p.sync()
                t0 = time.perf_counter()
            if track:
                if f > 3:       # tracking(); if tracked: integration(); raycasting() -- benchmark.cpp:115-150 -- in one FFI call
                    tracked += (p.frame_tracked(depth_ptrs[f], k_at, mu, f) >> 2) & 1
                else:
                    p.setPose(poses[f])
                    p.set_depth_device(depth_ptrs[f])
                    p.integration(k, 1, mu, f)
                    p.raycasting(k, mu, f)
            else:
                p.frame(depth_ptrs[f], pose_at[f], k_at, mu, f)     # set_depth_device + integration + raycasting in one FFI call
            if per_frame_sync:
                p.sync()
        p.sync()
        dt = time.perf_counter() - t0
        rec = {"fps": n / dt, "ms_per_frame": 1e3 * dt / n, "frames": n}
        if track:
            err = np.abs(p.getPose()[:3, 3] - np.asarray(poses[warm + n - 1])[:3, 3]).max()
            rec.update(tracked_frames=tracked, of=warm + n - 4, final_position_error_m=float(err),
                       note="ICP-tracked poses (GT for frames 0..3 only).  On this analytic room the reference's point-to-plane ICP "
                            "under-tracks the 1 mm / frame translation -- the CPU oracle drifts identically (tests/test_gpu_tracking.py "
                            "pins GPU == oracle); the leg measures the loop's speed, not the tracker's accuracy")
        p.counts()   # raises on pool / key-list overflow
        p.close()
        scratch.close()
        out[label] = rec

    run("closed_loop", True, False)
    run("tracking_on", True, True)
    nb = {512: 1 << 16, 1024: 1 << 19}.get(N, 1 << 21)
    run("pooled", False, False, max_blocks=nb, streaming=not args.no_streaming)
    out["closed_loop"]["note"] = "per-frame se_hip_sync(); scan / sweep / raycast of a frame strictly in sequence"
    out["pooled"]["note"] = f"max_blocks = {nb}"
    return out


def cpp_mirror_leg(args, k, host_depth, poses, warm: int, n: int):
    """The drop-in surface itself: examples/denseslam_bench.cpp runs the loop of se_apps/src/benchmark.cpp:115-177 through the C++
    DenseSLAMSystem mirror (include/se/DenseSLAMSystem.h: preprocessing / setPose / integration / raycasting / synchroniseDevices) on the same
    frames, in its own process (no Python in the loop), and reports frames/s closed-loop (the reference's bracketing), streaming (the one-queue
    schedule through integration() + raycasting()) and closed-loop with the per-frame uint16 upload over PCIe."""
    import subprocess
    import tempfile
    exe = os.path.join(ROOT, "examples", "denseslam_bench")
    if not os.path.exists(exe):
        return {"error": "examples/denseslam_bench not built (__graft_entry__.build())"}
    F = warm + n
    with tempfile.NamedTemporaryFile(suffix=".bin", delete=False) as fh:
        path = fh.name
        np.asarray([args.width, args.height, F], np.int32).tofile(fh)
        np.asarray(k, np.float32).reshape(4).tofile(fh)
        for f in range(F):
            np.ascontiguousarray(poses[f], np.float32).reshape(16).tofile(fh)
            np.ascontiguousarray(host_depth[f], np.float32).reshape(-1).tofile(fh)
    try:
        r = subprocess.run([exe, path, str(args.res), str(args.dim), str(args.mu), str(warm), str(n)], capture_output=True, text=True, timeout=300)
    finally:
        os.unlink(path)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not line:
        return {"error": f"rc={r.returncode} {r.stderr[-400:]}"}
    return json.loads(line[-1])


def stress_leg(args, field, device, n: int):
    """N = 1 leg on the ICL-like stress stream: frames/s pipelined and closed-loop over `n` frames after 10
    warm-up frames, and what the stream does to the map per frame: new keys, swept blocks, blocks that left the frustum
    (active -> inactive), from an untimed instrumented replay."""
    import torch
    from supereight_amd.pipeline import DenseSLAMPipeline
    from supereight_amd.synthetic import StressStream, to_colmajor
    W, H, N, dim, mu = args.width, args.height, args.res, args.dim, args.mu
    warm = 10
    s = StressStream(W, H, dim)
    host = np.stack([s.depth(f) for f in range(warm + n)])
    poses = [s.pose(f) for f in range(warm + n)]
    pcm = [to_colmajor(q) for q in poses]
    k32 = np.ascontiguousarray(s.k, dtype=np.float32).reshape(4)
    dev = torch.from_numpy(host).to(torch.device("cuda", device))
    ptrs = [dev[f].data_ptr() for f in range(warm + n)]
    out = {"stream": "ICL-like stress (supereight_amd/synthetic.py StressStream)", "frames": n, "warmup": warm}
    for label, sync in (("fps", False), ("closed_loop_fps", True)):
        p = DenseSLAMPipeline((W, H), N, dim, field_type=field, device=device, streaming=(not sync) and not args.no_streaming)
        _, scratch = prewarm(args, field, ptrs, poses, k32, device)
        pose_at, k_at = [DenseSLAMPipeline.addr(a) for a in pcm], DenseSLAMPipeline.addr(k32)
        for f in range(warm):
            p.frame(ptrs[f], pose_at[f], k_at, mu, f)
        p.sync()
        t0 = time.perf_counter()
        for f in range(warm, warm + n):
            p.frame(ptrs[f], pose_at[f], k_at, mu, f)
            if sync:
                p.sync()
        p.sync()
        out[label] = n / (time.perf_counter() - t0)
        p.counts()
        p.close(); scratch.close()
    p = DenseSLAMPipeline((W, H), N, dim, field_type=field, device=device)
    p.enable_stats(True)
    prev = None
    new_keys, swept, deact, hits = [], [], [], []
    for f in range(warm + n):
        p.frame(ptrs[f], pcm[f], k32, mu, f)
        st = p.stats(reset=True)
        c, a = p.block_flags()
        cur = {tuple(v): int(fl) for v, fl in zip(c.tolist(), a.tolist())}
        if f >= warm:
            new_keys.append(st["new_keys"]); swept.append(st["swept"]); hits.append(st["hits"])
            deact.append(sum(1 for key, fl in cur.items() if fl == 0 and prev.get(key, 0) == 1))
        prev = cur
    out["blocks_allocated"] = len(prev)
    p.close()
    for name, v in (("new_keys_per_frame", new_keys), ("swept_blocks_per_frame", swept), ("deactivated_blocks_per_frame", deact), ("ray_hits_per_frame", hits)):
        out[name] = {"mean": float(np.mean(v)), "max": int(np.max(v)), "min": int(np.min(v))}
    del dev
    return out


def pmc_traffic(kernel: str, args):
    """HBM bytes per launch of `kernel` from the newest committed rocprofv3 PMC summary of this exact
    workload (profiles/*_pmc_traffic.json, written by tools/summarize_prof.py from separate
    --pmc FETCH_SIZE / WRITE_SIZE passes with the gfx950 corrections of MI355X_MICROARCH.md); None
    if there is none -- counters cannot be collected from inside bench.py."""
    import glob
    best = None
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_traffic.json"))):
        try:
            d = json.load(open(path))
        except Exception:
            continue
        w = d.get("workload", {})
        if (w.get("width"), w.get("height"), w.get("res"), w.get("field")) == (args.width, args.height, args.res, args.field) and \
                abs(w.get("mu", args.mu) - args.mu) < 1e-9 and w.get("stream", "room") == args.stream and not args.raw:
            if kernel in d.get("kernels", {}):
                best = (d["kernels"][kernel]["traffic_bytes"], os.path.basename(path))
    return best


def main():
    args = parse()
    # OpenMP placement for the CPU baseline leg must be set before libgomp is loaded
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # RCCL on this driver stack needs dmabuf IPC (multi-process runs)
    os.environ.setdefault("OMP_PROC_BIND", "close")
    os.environ.setdefault("OMP_PLACES", "cores")
    import torch
    import torch.distributed as dist
    from supereight_amd.multi_gpu import ShardedPipeline
    from supereight_amd.pipeline import OFUSION, SDF, DenseSLAMPipeline
    from supereight_amd.synthetic import SyntheticStream

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} needs torch.distributed.run with {args.gpus} processes (WORLD_SIZE={world})")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
    backend = os.environ.get("SE_BENCH_BACKEND", "nccl")     # "gloo": dry run of the N > 1 path with all ranks on one GPU
    if backend != "nccl":
        local_rank = 0
    torch.cuda.set_device(local_rank)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
    field = SDF if args.field == "sdf" else OFUSION
    W, H, N, dim, mu = args.width, args.height, args.res, args.dim, args.mu
    warm = max(args.warmup, 4)   # frames 0..3 are the reference's own warm-up (forced integration, no raycast before frame 3)
    K = args.steps
    # N = 1, on request: the K contract steps are followed, in a second timed region, by as many frames as it takes to have
    # `--sustain` frames timed in total (off by default: --steps alone sets the number of timed frames)
    extra = max(0, args.sustain - K) if (world == 1 and args.sustain > 0) else 0
    F = warm + K + extra

    # ---- inputs: the whole stream resident in HBM before anything is timed
    stream, stream_name = make_stream(args, F)
    host_depth = np.stack([stream.depth(f) for f in range(F)])
    from supereight_amd.synthetic import to_colmajor
    poses = [stream.pose(f) for f in range(F)]
    poses_cm = [to_colmajor(q) for q in poses]      # the C-ABI layout, converted outside the timed region
    k = np.ascontiguousarray(stream.k, dtype=np.float32).reshape(4)
    dev = torch.device("cuda", local_rank)
    depth = torch.from_numpy(host_depth).to(dev)
    depth_ptrs = [depth[f].data_ptr() for f in range(F)]

    # the pipeline is created BEFORE the pre-warm and the scratch map is freed AFTER the timed regions: allocating or
    # freeing gigabytes idles the GPU for tens of milliseconds, long enough for the clocks to drop again
    sp = ShardedPipeline((W, H), N, dim, field, rank, world, local_rank, shard_sweep=args.shard_sweep,
                         streaming=(not args.no_streaming) and (world == 1 or args.sharded_streaming))
    prewarm_frames, scratch = prewarm(args, field, depth_ptrs, poses, k, local_rank) if not args.no_prewarm else (0, None)

    def barrier():
        if world > 1:
            dist.barrier()

    freeze_gc()
    for f in range(warm):
        sp.frame(depth_ptrs[f], poses_cm[f], k, mu, f)
    # The timed window holds ALL the work of frames warm .. warm+K-1 and nothing else (se_apps/src/benchmark.cpp:148-152,166-167 brackets every
    # frame's integration + raycasting): the raycast of frame warm-1, held back by the streaming schedule, is launched and finished HERE, before t0,
    # and the raycast of frame warm+K-1 is launched and finished before t1 (sp.p.sync() does both: launch, then wait).  The launch counters read at t1
    # prove it in the JSON line: K allocation scans, K sweeps, K raycasts.
    sp.p.sync()    # (raises if a pool or key list overflowed during warm-up)
    torch.cuda.synchronize()
    sp.p.launch_counts(reset=True)
    # per-kernel HIP events on every stride-th contract step: each sampled frame costs 6 event records on the launch
    # streams (measured: every 2nd frame sampled lowers `value` by 9 %, every 5th by < 2 %), so at least 4 samples, not more
    stride = max(1, min(args.event_stride, K // 4 if K >= 4 else 1))
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    throttle = int(os.environ.get("SE_BENCH_THROTTLE", "0"))
    for f in range(warm, warm + K):
        if not args.no_events:
            sp.p.enable_timing((f - warm) % stride == 0)   # sampled: HIP events on the launch stream
        sp.frame(depth_ptrs[f], poses_cm[f], k, mu, f)
        if throttle and (f - warm) % throttle == throttle - 1:
            sp.p.sync()
    sp.p.sync()                 # launches the held-back raycast of the last timed frame, then waits for the handle's streams
    torch.cuda.synchronize()
    barrier()
    t1 = time.perf_counter()
    elapsed = t1 - t0
    launched = sp.p.launch_counts(reset=True)
    for kk in ("alloc_scan", "integrate", "raycast"):
        if launched[kk] != K or launched["pending"]:
            raise RuntimeError(f"timed region of {K} frames holds {launched}: every frame's scan, sweep and raycast must be inside it")
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    sustained = None
    if extra:
        t2 = time.perf_counter()
        sp.p.enable_timing(False)                   # kernel events (and the roofline) belong to the K contract steps
        for f in range(warm + K, F):
            sp.frame(depth_ptrs[f], poses_cm[f], k, mu, f)
        sp.p.sync()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        launched2 = sp.p.launch_counts(reset=True)
        for kk in ("alloc_scan", "integrate", "raycast"):
            if launched2[kk] != extra or launched2["pending"]:
                raise RuntimeError(f"second timed region of {extra} frames holds {launched2}")
        sustained = {"frames": K + extra, "fps": (K + extra) / (elapsed + (t3 - t2)), "fps_second_region": extra / (t3 - t2),
                     "launches_in_timed_regions": {kk: launched[kk] + launched2[kk] for kk in ("alloc_scan", "integrate", "raycast", "fused")},
                     "note": f"the K = {K} contract steps plus {extra} more frames of the same stream, two timed regions added up"}
    fused_schedule = sp.p.frame_is_fused()
    timings = sp.p.timings(reset=True) if not args.no_events else None
    sp.p.enable_timing(False)
    nblocks, nnodes = sp.p.counts()
    mem = sp.p.memory_info()
    dumped = None
    if args.dump_outputs:
        sp.gather_images()       # collective: every rank of a row-sharded run takes part, rank 0 writes
        if rank == 0:
            dumped = dump_outputs(args.dump_outputs, sp.p)
    sp.close()
    if scratch is not None:
        scratch.close()

    result = None
    if rank == 0:
        fps = K / elapsed
        result = {
            "metric": f"frames/sec (integrate+raycast), {W}x{H} depth -> {N}^3 TSDF",
            "value": fps, "unit": "frames/s", "n_gpus": world, "steps": K, "warmup": warm,
            "ms_per_step": 1e3 * elapsed / K, "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None,
            "launches_in_timed_region": {kk: launched[kk] for kk in ("alloc_scan", "integrate", "raycast", "fused")},
            "dtype": "f32", "data": "real (.raw)" if args.raw else "synthetic",
            "config": {"workload": f"{stream_name} {W}x{H} -> {N}^3 / {dim} m "
                                   f"{'TSDF (SDF)' if field == SDF else 'occupancy (OFusion)'}, mu={mu}, integration_rate=1, "
                                   f"GT poses, frames {warm}..{warm + K - 1} timed",
                       "schedule": ("one queue: raycast(f) + scan(f+1) in one launch, sweep(f+1) behind it (se_hip_set_streaming: se_hip_frame holds a frame's raycast back until the next call)" if fused_schedule and world == 1
                                    else "one queue: raycast(f) + scan(f+1) in one launch over the rank's rows, all-gather of the key lists + commit + sweep(f+1) behind it (--sharded-streaming)" if fused_schedule
                                    else "two queues: scan(f+1) on a side stream beside raycast(f), event wait in front of sweep(f+1)"),
                       "parallelism": "single replica" if world == 1 else f"image rows sharded over {world} ranks, map replicated, RCCL all-gather of new-block key lists" + (", sweep sharded by block owner + RCCL all-gather of the updated bricks" if sp.shard_sweep else ""),
                       "blocks_allocated": nblocks, "nodes_allocated": nnodes,
                       "memory_per_replica": {"layout": mem["layout"], "voxel_bricks_GiB": round(mem["brick_bytes"] / 2**30, 3), "device_GiB": round(mem["device_bytes"] / 2**30, 3),
                                              "payload_GiB": round(nblocks * 4096 / 2**30, 3)},
                       "prewarm": f"{prewarm_frames} untimed frames on a scratch map before the W warm-up frames (clocks / caches warm, see bench.py prewarm()); "
                                  "gc.collect() + gc.freeze() before the warm-up frames (the interpreter's full collection over the import-time heap otherwise "
                                  "lands inside the first loop: profiles/r04f_stall_attribution.md)"},
        }
        if sustained:
            result["sustained"] = sustained
        if dumped:
            result["dumped_outputs"] = dumped

    # ---- roofline of the dominant kernel (rank 0, its own share of the image)
    if timings is not None and world > 1:
        mine = {kk: {"avg_us": 1e3 * v["ms_sum"] / v["launches"], "launches": v["launches"]} for kk, v in timings.items() if v["launches"]}
        everyone = [None] * world
        dist.all_gather_object(everyone, mine)
        if rank == 0:
            result["kernels"] = mine
            result["per_rank_kernels"] = everyone    # rank r raycasts / scans rows row_partition(H, world)[r]; the sweep is replicated
    if rank == 0 and timings is not None and world == 1:
        voxel_bytes = 8 if field == SDF else 16     # the reference layout; the device stores 8 B per voxel for both field types
        windows = [("contract", warm, warm + K)] + ([("sustained", warm, F)] if extra else [])
        fused = fused_schedule
        # (1) instrumented replay of the same frames: exact work counts of the launches of each window
        rp = DenseSLAMPipeline((W, H), N, dim, field_type=field, device=local_rank)
        rp.enable_stats(True)
        counts, acc = {}, None
        for f in range(F if extra else warm + K):
            rp.set_depth_device(depth_ptrs[f])
            rp.setPose(poses[f])
            if f == warm:
                rp.stats(reset=True)
            rp.integration(k, 1, mu, f)
            rp.raycasting(k, mu, f)
            if f == warm + K - 1:
                counts["contract"] = rp.stats()
        if extra:
            counts["sustained"] = rp.stats()
        rp.close()
        # (2) untimed event replay: the same pipelined loop with HIP events on EVERY frame (the timed region above samples
        # every stride-th frame only, because events cost throughput there): per-kernel averages over each window
        replay = {}
        ep = ShardedPipeline((W, H), N, dim, field, 0, 1, local_rank, streaming=not args.no_streaming)
        for f in range(warm):
            ep.frame(depth_ptrs[f], poses_cm[f], k, mu, f)
        ep.p.sync()
        ep.p.enable_timing(True)
        for f in range(warm, F if extra else warm + K):
            ep.frame(depth_ptrs[f], poses_cm[f], k, mu, f)
            if f == warm + K - 1:
                replay["contract"] = ep.p.timings(reset=False)
        if extra:
            replay["sustained"] = ep.p.timings(reset=False)
        ep.p.enable_timing(False)
        ep.close()

        def per_kernel_of(tm, st, frames):
            ab = algorithmic_bytes(st, frames, W, H, voxel_bytes)
            if fused:   # one launch does the raycast of frame f AND the allocation scan of frame f+1 (k_raycast_scan): its units are both
                ab["raycast"] = ab["raycast"] + ab["alloc_scan"]
            out = {}
            for kk, v in tm.items():
                if v["launches"] == 0:
                    continue
                avg_ms = v["ms_sum"] / v["launches"]
                out[kk] = {"avg_us": 1e3 * avg_ms, "launches": v["launches"], "share": v["ms_sum"]}
                if kk in ab:
                    out[kk]["algorithmic_bytes"] = ab[kk]
                    out[kk]["GBps"] = ab[kk] / (avg_ms * 1e-3) / 1e9
            tot = sum(v["share"] for v in out.values())
            for v in out.values():
                v["share"] = v["share"] / tot if tot else 0.0
            return out

        def roofline_of(pk, dom, st, frames):
            r = {"kernel": dom, "bound": "hbm", "achieved": pk[dom]["GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                 "frac": pk[dom]["GBps"] / HBM_PEAK_GBS, "traffic": None, "avg_launch_us": pk[dom]["avg_us"], "launches_timed": pk[dom]["launches"],
                 "algorithmic_bytes_per_launch": pk[dom]["algorithmic_bytes"]}
            tr = pmc_traffic(dom, args)
            if tr:
                r["traffic"] = tr[0]
                r["traffic_source"] = "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes, profiles/" + tr[1]
                # what the memory system really moved per second of this kernel, against the same peak: the caches absorb the rest
                r["hbm_frac"] = tr[0] / (pk[dom]["avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS
            # the reference-layout figure flatters the device where it stores a voxel in fewer bytes (OFusion: float y instead of double, 8 of 16 B;
            # SDF since r06: the weight as a byte, 5 of 8 B): say what the device really moves
            db = algorithmic_bytes(st, frames, W, H, 8 if field != SDF else 5, 0 if field != SDF else 4)
            if fused:
                db["raycast"] = db["raycast"] + db["alloc_scan"]
            r["device_layout_bytes_per_launch"] = db[dom]
            r["device_layout_frac"] = db[dom] / (pk[dom]["avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS
            r["device_layout"] = "SDF voxel = float tsdf + uint8 weight (5 B of the reference's 8)" if field == SDF else "OFusion voxel = float + float (8 B of the reference's 16)"
            return r

        st = counts["contract"]
        per_kernel = per_kernel_of(timings, st, K)       # contract: events recorded live in the timed region
        # the dominant kernel = the longest launch of a frame (by share of the sampled time it could flip on the sample count: the deferred
        # raycast of the last sampled frame is launched, and timed, with the next call)
        # ... judged on the every-launch replay where there is one (the live sample is K / stride launches: one slow launch of ten moved it)
        judge = per_kernel_of(replay["contract"], st, K) if "contract" in replay else per_kernel
        cands = [kk for kk in per_kernel if "GBps" in per_kernel[kk] and kk in judge]
        dom = max([kk for kk in cands if judge[kk]["launches"] >= 2] or cands, key=lambda kk: judge[kk]["avg_us"])
        result["roofline"] = roofline_of(per_kernel, dom, st, K)
        result["roofline"]["sampling"] = f"HIP events on every {stride}-th of the K timed frames, on the launch streams"
        if fused:
            result["roofline"]["launch"] = ("k_raycast_scan: the raycast of frame f and the allocation scan of frame f+1 are ONE launch (one-queue streaming schedule, "
                                            "se_hip_frame); algorithmic bytes = A_ray + A_alloc of SURVEY 8(d), duration = that launch's")
        result["kernels"] = per_kernel
        result["work_per_frame"] = {kk: st[kk] / K for kk in ("probes", "new_keys", "swept", "gets", "interps", "grads", "hits")}
        # the same figure from the every-frame replay, for the contract window and for the sustained window
        result["roofline_replay"] = {"note": "untimed replay of the same pipelined loop with HIP events on every frame; shows how the figure moves with the window"}
        for name, lo, hi in windows:
            if name in replay and name in counts:
                pk = per_kernel_of(replay[name], counts[name], hi - lo)
                rr = roofline_of(pk, dom, counts[name], hi - lo)
                rr["frames"] = [lo, hi - 1]
                rr["kernels_us"] = {kk: round(v["avg_us"], 2) for kk, v in pk.items()}
                result["roofline_replay"][name] = rr
        # The fraction to quote is the longest window's, every launch of it timed (the live sample is K / stride launches -- three under the
        # driver's command -- and moves by 10 % with the window): `frac`, `achieved`, `avg_launch_us` are that replay's, measured by HIP events on the launch
        # stream in this same process on the same frames; the live sample of the timed region stays beside them as `*_live`.
        longest = result["roofline_replay"].get("sustained") or result["roofline_replay"].get("contract")
        if longest:
            rl = result["roofline"]
            for kk in ("frac", "achieved", "avg_launch_us", "launches_timed", "algorithmic_bytes_per_launch", "hbm_frac"):
                if kk in rl:
                    rl[kk + "_live"] = rl[kk]
                if kk in longest:
                    rl[kk] = longest[kk]
            rl["window"] = f"frames {longest['frames'][0]}..{longest['frames'][1]}, every launch timed by HIP events on the launch stream (replay of the timed loop in this process)"
            rl["sampling_live"] = rl.pop("sampling")
            rl["frac_sustained"] = longest["frac"]      # (the name earlier rounds' records carry)

    # ---- legs beside the contract line (every rank takes part)
    def timed_leg(make, ptrs, pcm, kk, warm_, K_):
        """warm_ untimed + K_ timed frames of one stream through make(); returns (max-over-ranks seconds, (blocks, nodes))."""
        q = make()
        for f in range(warm_):
            q.frame(ptrs[f], pcm[f], kk, mu, f)
        torch.cuda.synchronize()
        barrier()
        ta = time.perf_counter()
        for f in range(warm_, warm_ + K_):
            q.frame(ptrs[f], pcm[f], kk, mu, f)
        torch.cuda.synchronize()
        barrier()
        el = time.perf_counter() - ta
        if world > 1:
            tt = torch.tensor([el], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            el = float(tt.item())
        cnt = q.p.counts()
        q.close()
        return el, cnt

    if world > 1 and not args.no_replicas:
        # SURVEY 8(e) fallback, the throughput upper bound: every GPU runs its own full-image stream, no exchange at all
        el, cnt = timed_leg(lambda: ShardedPipeline((W, H), N, dim, field, 0, 1, local_rank), depth_ptrs, poses_cm, k, warm, K)
        if rank == 0:
            result["replicas_only"] = {"value": world * K / el, "unit": "frames/s (sum over ranks)", "per_gpu_fps": K / el, "steps": K, "scaling": "weak",
                                       "note": "independent streams, one per GPU, same workload as the contract line on every rank; no collective in the data path"}
    if (world > 1 and not args.no_config4) or (world == 1 and args.config4):
        # BASELINE.json configs[3]: 1280x960 -> 2048^3, same rank layout as the contract line (row-sharded for N > 1) -- the
        # configuration in which the image-space stages dominate a frame and sharding them can pay
        W4, H4, N4, K4, warm4 = 1280, 960, 2048, max(2, args.config4_steps), 6
        s4 = SyntheticStream(W4, H4, dim)
        host4 = np.stack([s4.depth(f) for f in range(warm4 + K4)])
        pcm4 = [to_colmajor(s4.pose(f)) for f in range(warm4 + K4)]
        k4 = np.ascontiguousarray(s4.k, dtype=np.float32).reshape(4)
        dev4 = torch.from_numpy(host4).to(dev)
        ptrs4 = [dev4[f].data_ptr() for f in range(warm4 + K4)]
        el, cnt = timed_leg(lambda: ShardedPipeline((W4, H4), N4, dim, field, rank, world, local_rank), ptrs4, pcm4, k4, warm4, K4)
        if rank == 0:
            result["config4"] = {"metric": "frames/sec (integrate+raycast), 1280x960 depth -> 2048^3 TSDF", "value": K4 / el, "unit": "frames/s", "n_gpus": world,
                                 "steps": K4, "warmup": warm4, "ms_per_step": 1e3 * el / K4, "scaling": "strong", "blocks_allocated": cnt[0],
                                 "config": {"workload": f"synthetic room+sphere depth stream {W4}x{H4} -> {N4}^3 / {dim} m, mu={mu}, GT poses",
                                            "parallelism": "single replica" if world == 1 else f"image rows sharded over {world} ranks, map replicated, RCCL all-gather of new-block key lists"}}
        del dev4

    if rank == 0 and world == 1 and not args.no_closed_loop:
        # SURVEY 8(d)'s own bracketing (se_apps/src/benchmark.cpp:148-167: wall clock around integration() + raycasting()
        # including the device sync, frame by frame): the SAME K frames as `value`, a fresh map, one se_hip_sync() per frame,
        # nothing of frame f+1 issued before frame f has finished.  This is the figure a SLAM loop whose next pose depends
        # on this frame's raycast gets; `value` is the pipelined rate of a caller that knows its poses in advance.
        cp = DenseSLAMPipeline((W, H), N, dim, field_type=field, device=local_rank)
        _, cscratch = prewarm(args, field, depth_ptrs, poses, k, local_rank) if not args.no_prewarm else (0, None)
        # (pose / intrinsics as addresses of the arrays held above: what a C++ caller passes; an array argument costs ctypes 3-5 us of checks)
        pose_at, k_at = [DenseSLAMPipeline.addr(a) for a in poses_cm], DenseSLAMPipeline.addr(k)
        for f in range(warm):
            cp.frame(depth_ptrs[f], pose_at[f], k_at, mu, f)
            cp.sync()
        tc0 = time.perf_counter()
        for f in range(warm, warm + K):
            cp.frame(depth_ptrs[f], pose_at[f], k_at, mu, f)
            cp.sync()
        tc1 = time.perf_counter()
        cp.counts()
        cp.close()
        if cscratch is not None:
            cscratch.close()
        result["value_closed_loop"] = K / (tc1 - tc0)
        result["ms_per_step_closed_loop"] = 1e3 * (tc1 - tc0) / K
        result["value_note"] = ("value = K pipelined frames / wall time (poses known in advance: scan(f+1) runs beside raycast(f)); "
                                "value_closed_loop = the same K frames with a device sync after every frame, SURVEY 8(d)'s bracketing")
    if rank == 0 and world == 1 and not args.no_modes and field == SDF and not args.raw:
        cm = cpp_mirror_leg(args, k, host_depth, poses, warm, min(K, F - warm))
        result["cpp_mirror"] = cm
        if "streaming_fps" in cm:
            result["value_cpp_mirror"] = cm["streaming_fps"]
            result["value_cpp_mirror_closed_loop"] = cm["closed_loop_fps"]
    if rank == 0 and world == 1 and not args.no_modes:
        result["modes"] = extra_modes(args, field, depth_ptrs, poses, k, warm, min(args.mode_frames, F - warm), local_rank)
        if args.stream != "stress" and not args.raw:
            result["modes"]["stress"] = stress_leg(args, field, local_rank, args.mode_frames)
    del depth
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        result["cpu_baseline"] = cpu_baseline(args, args.cpu_frames)
        result["speedup_vs_cpu_baseline"] = result["value"] / result["cpu_baseline"]["value"]
    if rank == 0:
        if args.detail:
            os.makedirs(os.path.dirname(os.path.abspath(args.detail)), exist_ok=True)
            with open(args.detail, "w") as fh:
                json.dump(result, fh, indent=1)
        print(json.dumps(result))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
