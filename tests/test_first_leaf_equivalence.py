"""CPU test of the claim behind k_raycast's stack-free first-leaf search (se_first_leaf_lite): for every ray that is
regular at set-up and never descends from a cell it has, by t_corner, already left, the reference iterator's stack and `h`
carry no information -- a model without them (tests/cpp/first_leaf_equiv.cpp) returns the bit-identical t_min and the same
leaf-found decision as the oracle's restatement of se::ray_iterator (se_core/include/se/ray_iterator.hpp:53-226).  The
rays the model hands back (`flagged`, `irregular`) are the ones the kernel re-runs through the full iterator; the test also
bounds how many those are."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import binding
from supereight_amd.synthetic import make_stream, to_colmajor
from tests.edge_frames import RES_CASES, SHAPE_CASES, RoomStream
from tests.parity_util import OUTSIDE_VIEWS, outside_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fl") / "libfl.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-march=x86-64-v3", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                    "-Wno-unknown-pragmas", "-o", so, os.path.join(ROOT, "tests", "cpp", "first_leaf_equiv.cpp")], check=True, capture_output=True)
    lib = binding._declare(C.CDLL(so))
    lib.fl_compare.restype = None
    lib.fl_compare.argtypes = [C.c_void_p, binding.c_f32p, binding.c_f32p, np.ctypeslib.ndpointer(np.int64), np.ctypeslib.ndpointer(np.int32), C.c_int]
    return lib


FIELDS = ("rays", "irregular", "flagged", "mismatch", "found", "trips_ref", "trips_lite", "model_bug")


def _compare(lib, h, view, k, beam):
    out = np.zeros(8, np.int64)
    bad = np.zeros(2, np.int32)
    lib.fl_compare(h, to_colmajor(view), k, out, bad, beam)
    return out, bad


def _run(lib, field, kind, W, H, N, mu, frames, pose_shift=None, beam=0, first_view=3, stream=None):
    st = make_stream(kind, W, H, 4.8) if stream is None else stream
    h = lib.so_pipe_create(field, N, st.dim, W, H)
    tot = np.zeros(8, np.int64)
    try:
        for f in range(frames):
            d = np.ascontiguousarray(st.depth(f), np.float32).reshape(-1)
            pose = st.pose(f)
            k = np.asarray(st.k, np.float32)
            lib.so_pipe_integrate(h, d, to_colmajor(pose), k, 1, mu, f)
            if f >= first_view:
                view = pose.copy()
                if pose_shift is not None:
                    view[:3, 3] += np.asarray(pose_shift, np.float32)
                out, bad = _compare(lib, h, view, k, beam)
                assert out[3] == 0 and out[7] == 0, f"frame {f}: {out[3]} rays differ from the iterator (e.g. pixel {bad.tolist()}), model errors {out[7]}"
                tot += out
    finally:
        lib.so_pipe_destroy(h)
    return dict(zip(FIELDS, tot.tolist()))


@pytest.mark.parametrize("field,kind,N,mu", [(binding.SDF, "room", 512, 0.1), (binding.SDF, "stress", 256, 0.1), (binding.OFUSION, "stress", 512, 0.02),
                                             (binding.SDF, "stress", 1024, 0.1)])
def test_stack_free_search_equals_the_iterator(lib, field, kind, N, mu):
    r = _run(lib, field, kind, 320, 240, N, mu, 7)
    assert r["rays"] == 4 * 320 * 240 and r["found"] > 0
    assert r["irregular"] == 0                      # the camera is inside the volume: every ray is regular at set-up
    assert r["flagged"] <= r["rays"] // 20000       # the edge-grazing descents are a handful per million rays
    assert r["trips_lite"] <= r["trips_ref"]        # (a handed-back ray stops early; the others take the same trips)


def test_rays_that_miss_the_volume_are_handed_back(lib):
    # camera pulled 6 m out of the 4.8 m volume: most rays enter through a face (regular), the rest miss it (irregular set-up);
    # both kinds must agree with the iterator or be handed back
    r = _run(lib, binding.SDF, "room", 160, 120, 256, 0.1, 5, pose_shift=(0.0, 0.0, -6.0))
    assert r["irregular"] > 0 and r["mismatch"] == 0


@pytest.mark.parametrize("field,kind,W,H,N,mu,frames,first_view", [
    (binding.SDF, "room", 640, 480, 512, 0.1, 6, 3),         # the benchmark's geometry
    (binding.SDF, "stress", 320, 240, 512, 0.1, 40, 30),     # the pan: occluders, depth edges, the volume's faces, rays that leave the cube
    (binding.SDF, "stress", 320, 240, 1024, 0.1, 8, 4),
    (binding.OFUSION, "stress", 320, 240, 512, 0.02, 8, 4),  # coarse childless octants in the tree (not blocks: they never stop the search)
    (binding.SDF, "room", 160, 120, 128, 0.1, 6, 3),         # leaf level 4 < 5: the coarse grid IS the block grid
])
def test_beam_start_returns_the_iterators_leaf(lib, field, kind, W, H, N, mu, frames, first_view):
    """r05: with every 8x8 tile's rays entering the tree at the tile's t_safe (se_beam_start, restated in tests/cpp/first_leaf_equiv.cpp), the
    first leaf and its entry time are bit for bit those of the reference iterator started at the near plane, for every ray that is not handed
    back -- and the search takes fewer than half the trips."""
    base = _run(lib, field, kind, W, H, N, mu, frames, first_view=first_view)
    r = _run(lib, field, kind, W, H, N, mu, frames, beam=1, first_view=first_view)
    r2 = _run(lib, field, kind, W, H, N, mu, frames, beam=2, first_view=first_view)
    print("two-stage:", round(r2["trips_lite"] / r2["rays"], 2), "mismatch", r2["mismatch"], "flagged", r2["flagged"])
    print(W, H, N, "trips per ray:", round(base["trips_lite"] / base["rays"], 2), "->", round(r["trips_lite"] / r["rays"], 2), "handed back:", r["flagged"], "of", r["rays"])
    assert r["rays"] == base["rays"] and r["mismatch"] == 0 and r["model_bug"] == 0
    assert r["found"] + r["flagged"] >= base["found"]              # (a handed-back ray is not counted as found)
    assert r["flagged"] <= base["flagged"] + r["rays"] // 5000
    if N >= 512:
        assert r["trips_lite"] < 0.85 * base["trips_lite"]


EDGE_BEAM_CASES = [c for c in SHAPE_CASES + RES_CASES if c["W"] * c["H"] < 100000] + [
    # a 3-pixel column through a very narrow lens: one partial tile column, an 8x8 beam much thinner than a cell
    dict(name="column_3x203_fx1000_sdf", W=3, H=203, N=512, dim=4.8, k=(1000.0, 1000.0, 1.5, 101.5), field=binding.SDF, mu=0.1, frames=6),
]


@pytest.mark.parametrize("case", EDGE_BEAM_CASES, ids=[c["name"] for c in EDGE_BEAM_CASES])
def test_beam_start_at_edge_cameras_and_resolutions(lib, case):
    """The same claim for the cameras and volume resolutions of tests/test_gpu_edge_configs.py: partial tiles, fx != fy, off-centre principal
    points, negative fy, wide and narrow lenses, 64^3 (no fine grid, leaf level below the staged levels) and 4096^3 (three levels beyond them)."""
    args = (lib, case["field"], "room", case["W"], case["H"], case["N"], case["mu"], case["frames"])
    base = _run(*args, stream=RoomStream(case["W"], case["H"], case["dim"], case["k"]))
    for beam in (1, 2):
        r = _run(*args, beam=beam, stream=RoomStream(case["W"], case["H"], case["dim"], case["k"]))
        print(case["name"], "beam", beam, r)
        assert r["rays"] == base["rays"] == 3 * case["W"] * case["H"] and r["mismatch"] == 0 and r["model_bug"] == 0, r
        assert r["found"] + r["flagged"] >= base["found"] > 0
        assert r["flagged"] <= base["flagged"] + r["rays"] // 5000 + 1


def test_beam_start_from_outside_the_volume(lib):
    r = _run(lib, binding.SDF, "room", 160, 120, 256, 0.1, 5, pose_shift=(0.0, 0.0, -6.0), beam=1)
    assert r["irregular"] > 0 and r["mismatch"] == 0


# Maps for the views from beyond the faces (160x120, frames 0-5, 4.8 m): name -> field, stream, N, mu
FACE_MAPS = {
    "room_sdf_256": (binding.SDF, "room", 256, 0.1),          # the back wall's band reaches the +z face's boundary coarse cells
    "stress_sdf_256": (binding.SDF, "stress", 256, 0.1),      # the stress room is cut by the -x and +z faces: blocks in the boundary cells
    "stress_sdf_512": (binding.SDF, "stress", 512, 0.1),      # (the second stage's fine grid exists from leaf level 6 on)
    "stress_ofusion_512": (binding.OFUSION, "stress", 512, 0.02),
    "room_sdf_128": (binding.SDF, "room", 128, 0.1),          # leaf level 4: the coarse grid IS the block grid
}
# camera offsets beyond the face, as fractions of the edge: from inside the one-cell shell (a coarse cell is 1/32 of the edge, 1/16 at 128^3) out to
# ~10 coarse cells, a fifth of a coarse cell apart, so that the beam's samples (half a coarse cell apart) land at every depth of the shell
FACE_OFFSETS = [i * 0.00625 for i in range(1, 49)]


@pytest.fixture(scope="module")
def face_maps(lib):
    made = {}

    def get(name):
        if name not in made:
            field, kind, N, mu = FACE_MAPS[name]
            st = make_stream(kind, 160, 120, 4.8)
            h = lib.so_pipe_create(field, N, 4.8, 160, 120)
            k = np.asarray(st.k, np.float32)
            for f in range(6):
                lib.so_pipe_integrate(h, np.ascontiguousarray(st.depth(f), np.float32).reshape(-1), to_colmajor(st.pose(f)), k, 1, mu, f)
            made[name] = (h, k)
        return made[name]
    yield get
    for h, _ in made.values():
        lib.so_pipe_destroy(h)


@pytest.mark.parametrize("view", list(OUTSIDE_VIEWS))
@pytest.mark.parametrize("name", list(FACE_MAPS))
def test_beam_start_from_beyond_every_face(lib, face_maps, name, view):
    """A beam sample outside the volume but within one coarse (stage 2: fine) cell of it takes the dilated bit of the boundary cell it touches --
    on every face.  The shell test of se_beam_start once accepted only the cells -1 .. n-1: a sample just beyond an upper face counted as clear,
    and tiles seen from outside +z started their search up to ~0.9 cell inside the boundary cell, behind the blocks there (room 256^3 from
    0.075-0.30 edges beyond +z: 17 of 19 offsets with 2-61 rays each that missed the iterator's first leaf).  From each camera of OUTSIDE_VIEWS,
    at every offset and with one and two stages, every ray that is not handed back must find the iterator's leaf at its t_min."""
    h, k = face_maps(name)
    bad = []
    for d in FACE_OFFSETS:
        view_pose = outside_view(view, d, 4.8)
        for beam in (1, 2):
            out, px = _compare(lib, h, view_pose, k, beam)
            r = dict(zip(FIELDS, out.tolist()))
            if r["mismatch"] or r["model_bug"] or not r["found"]:
                bad.append((round(d, 5), beam, r["mismatch"], r["model_bug"], r["found"], px.tolist()))
    assert not bad, f"(offset, stage, rays that differ from the iterator, model errors, rays found, a differing pixel): {bad}"
