"""DenseSLAMSystem::queryMap (the C++ mirror, include/se/DenseSLAMSystem.h) against the host se::Octree that getMap() materialises from
the same device map: tests/cpp/map_query_mirror.cpp, compiled with g++ -ffp-contract=off and linked to libse_hip.so, runs a 640x480
SLAMBench .raw stream into a 512^3 volume and compares x and y of get_fine / get, interp and grad bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from supereight_amd.rawio import write_raw
from supereight_amd.synthetic import SyntheticStream, render_depth_mm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("tag,mu", [("SDF", 0.1), ("OFusion", 0.02)], ids=["sdf", "ofusion"])
def test_query_map_equals_the_host_octree(tmp_path, tag, mu):
    exe = str(tmp_path / f"map_query_mirror_{tag}")
    subprocess.run(["g++", "-std=c++14", "-O2", "-ffp-contract=off", f"-DSE_FIELD_TYPE={tag}", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "map_query_mirror.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "supereight_amd"), "-lse_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "supereight_amd")], check=True, capture_output=True)
    W, H, N, dim, frames = 640, 480, 512, 4.8, 3
    s = SyntheticStream(W, H, dim, holes=False)
    raw, pf = str(tmp_path / "scene.raw"), str(tmp_path / "poses.bin")
    write_raw(raw, [render_depth_mm(f, W, H, dim) for f in range(frames)])
    np.stack([s.pose(f) for f in range(frames)]).astype(np.float32).tofile(pf)
    r = subprocess.run([exe, raw, pf, str(N), str(dim), str(mu)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    f = r.stdout.split()
    res = {f[i]: int(f[i + 1]) for i in range(0, len(f), 2)}
    assert res["bad"] == 0, r.stderr
    assert res["checked"] > 5000 and 0 < res["allocated"] < res["in_volume"] < res["checked"]
    assert 0 < res["observed"] < res["checked"]
    if tag == "OFusion":
        assert res["coarse_node"] > 0      # Octree::get answered from a coarse node somewhere
