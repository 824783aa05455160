#!/usr/bin/env python3
"""Cost of the reachability field of a region (se_hip_reach_field) against the only route the library offered for these numbers before it:
DenseSLAMSystem::getMap() plus a flood fill on the host, se::geometry::reach_field (a) of include/se/reach_field.hpp -- on SDF dense maps
built from the synthetic room and stress streams (640x480, 4.8 m, --frames frames) at --res.

The measuring is done by tools/reach_bench.cpp, which this tool compiles against the built library and runs once per map: it replays the
stream through the C++ mirror, so the device call and the host route see the very same map, and compares their answers in every variant.
Regions of --sides^3 positions, each placed twice:
  surface    centred on a raycast hit vertex of the last frame
  free       centred on the empty 16^3 box, of 4096 placed uniformly, that is farthest from that hit
For every region: robot 1 and 4, one seed (the region's centre) and 16 seeds (spread over the region), stop_at occupied.  Every variant twice,
the two routes alternating:
  device     microseconds per call through the device entry (the call synchronises: wall time around --reps calls after two warm-up calls),
             and the rounds the call ran
  host       microseconds of reach_field (a) on the snapshot, and of getMap() itself (taken twice per map); the ratios to the device call
             with and without the getMap() share
One JSON line per map, region and variant.  --trace makes every device call once and nothing else: `rocprofv3 --kernel-trace --stats --
python tools/reach_bench.py --trace --maps room --sides 64` splits a call into its launches."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from supereight_amd import build  # noqa: E402
from supereight_amd.rawio import write_raw  # noqa: E402
from supereight_amd.synthetic import make_stream  # noqa: E402

W, H, DIM, MU = 640, 480, 4.8, 0.1


def compile_helper(out_dir):
    build.build()
    exe = os.path.join(out_dir, "reach_bench")
    lib_dir = os.path.join(ROOT, "supereight_amd")
    rocm = os.path.dirname(os.path.dirname(build.hipcc()))
    cmd = ["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-DSE_FIELD_TYPE=SDF", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(rocm, "include"), os.path.join(ROOT, "tools", "reach_bench.cpp"), "-o", exe, "-L" + lib_dir, "-lse_hip", "-L" + os.path.join(rocm, "lib"),
           "-lamdhip64", "-Wl,-rpath," + lib_dir, "-Wl,-rpath," + os.path.join(rocm, "lib")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("g++ failed:\n" + r.stderr[-4000:])
    return exe


def write_scene(out_dir, kind, frames):
    """The first `frames` frames of the stream as millimetre depth, and their poses (row-major float32 4x4)."""
    s = make_stream(kind, W, H, DIM, holes=False)
    raw, pf = os.path.join(out_dir, kind + ".raw"), os.path.join(out_dir, kind + "_poses.bin")
    write_raw(raw, [np.rint(np.asarray(s.depth(f), np.float64) * 1000.0).astype(np.uint16) for f in range(frames)])
    np.stack([s.pose(f) for f in range(frames)]).astype(np.float32).tofile(pf)
    return raw, pf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--sides", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--maps", nargs="+", default=["room", "stress"])
    ap.add_argument("--trace", action="store_true", help="the device calls only, once each: for a kernel trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reach_bench.jsonl"))
    args = ap.parse_args()
    records = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = compile_helper(tmp)
        for kind in args.maps:
            raw, pf = write_scene(tmp, kind, args.frames)
            cmd = [exe, raw, pf, str(args.res), str(DIM), str(MU), kind, str(args.reps), ",".join(str(s) for s in args.sides)] + (["trace"] if args.trace else [])
            proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
            for line in proc.stdout:
                print(line, end="", flush=True)
                records.append(json.loads(line))
            if proc.wait() != 0:
                raise RuntimeError(f"reach_bench exited with {proc.returncode} on the {kind} map")
    if not args.trace:
        unequal = [r for r in records if not r["equal"]]
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            for r in records:
                f.write(json.dumps(r) + "\n")
        if unequal:
            raise SystemExit(f"{len(unequal)} variants in which the device and the host route differ")


if __name__ == "__main__":
    main()
