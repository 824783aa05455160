"""DenseSLAMSystem::allocateRegion on a live handle against the host restatement (include/se/allocate_region.hpp) applied to the getMap()
snapshot taken before, compared through a second getMap() (tests/cpp/alloc_mirror.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from supereight_amd.rawio import write_raw
from supereight_amd.synthetic import SyntheticStream, render_depth_mm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("tag,mu", [("SDF", 0.1), ("OFusion", 0.02)], ids=["sdf", "ofusion"])
def test_allocate_region_equals_the_host_restatement(tmp_path, tag, mu):
    exe = str(tmp_path / f"alloc_mirror_{tag}")
    subprocess.run(["g++", "-std=c++14", "-O2", "-ffp-contract=off", f"-DSE_FIELD_TYPE={tag}", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "alloc_mirror.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "supereight_amd"), "-lse_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "supereight_amd")], check=True, capture_output=True)
    Wm, Hm, N, dim, frames = 320, 240, 256, 4.8, 3
    s = SyntheticStream(Wm, Hm, dim, holes=False)
    raw, pf = str(tmp_path / "scene.raw"), str(tmp_path / "poses.bin")
    write_raw(raw, [render_depth_mm(f, Wm, Hm, dim) for f in range(frames)])
    np.stack([s.pose(f) for f in range(frames)]).astype(np.float32).tofile(pf)
    r = subprocess.run([exe, raw, pf, str(N), str(dim), str(mu)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    f = r.stdout.split()
    res = {f[i]: int(f[i + 1]) for i in range(0, len(f), 2)}
    print(r.stdout, r.stderr)
    assert res["bad"] == 0, r.stderr
    assert res["boxes"] > 120 and res["blocks"] > 100 and res["nodes"] > 10 and res["pairs"] > res["blocks"] and res["keys"] > 0
    assert res["invalid"] == 4 and res["again"] == 0
