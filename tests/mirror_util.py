"""The Python side of the tests/cpp/*_mirror.cpp programs (their scene driver is tests/cpp/mirror_scene.hpp): compile one against the built
library, write the SLAMBench .raw scene and the pose file it replays, run it and parse the `key value key value` line it prints."""
import os
import subprocess

import numpy as np

from supereight_amd.rawio import write_raw
from supereight_amd.synthetic import SyntheticStream, render_depth_mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_mirror(tmp_path, name, tag, extra=()) -> str:
    """tests/cpp/<name>.cpp for the field type `tag` ("SDF" / "OFusion"), linked to libse_hip.so: the executable's path."""
    exe = os.path.join(str(tmp_path), f"{name}_{tag}")
    lib_dir = os.path.join(ROOT, "supereight_amd")
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-ffp-contract=off", f"-DSE_FIELD_TYPE={tag}", "-I" + os.path.join(ROOT, "include"), *extra,
                        os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe, "-L" + lib_dir, "-lse_hip", "-Wl,-rpath," + lib_dir],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def write_scene(tmp_path, W, H, dim, frames, holes=False):
    """The first `frames` frames of the synthetic room stream as scene.raw, their poses (row-major float32 4x4) as poses.bin:
    (raw, poses_file, stream)."""
    s = SyntheticStream(W, H, dim, holes=holes)
    raw, pf = os.path.join(str(tmp_path), "scene.raw"), os.path.join(str(tmp_path), "poses.bin")
    write_raw(raw, [render_depth_mm(f, W, H, dim) for f in range(frames)])
    np.stack([s.pose(f) for f in range(frames)]).astype(np.float32).tofile(pf)
    return raw, pf, s


def run_mirror(exe, args, timeout):
    """Runs the program: (the `key value` pairs of its stdout line as a dict of ints, the CompletedProcess)."""
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr
    f = r.stdout.split()
    return {f[i]: int(f[i + 1]) for i in range(0, len(f), 2)}, r
