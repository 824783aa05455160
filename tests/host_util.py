"""What the host-side (no GPU) tests of the batched entry points share, and the GPU tests with them: a pipeline object without a library
behind it for the argument checks, the build of the tests/cpp/*_kats.cpp programs, Morton keys, and the numpy truth of region allocation."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 1 << 30


class NoLib:
    """Stands in for libse_hip.so: any call is a test failure (the checks must fire before the library is reached)."""
    def __getattr__(self, name):
        raise AssertionError(f"library call {name}: the argument checks come first")


def bare_pipeline(**attrs):
    """A DenseSLAMPipeline without a handle, on NoLib, with the attributes the method under test reads."""
    from supereight_amd.pipeline import DenseSLAMPipeline
    p = DenseSLAMPipeline.__new__(DenseSLAMPipeline)      # (no handle)
    p.lib, p._h = NoLib(), None
    for k, v in attrs.items():
        setattr(p, k, v)
    return p


def build_kats(name, out_dir) -> str:
    """tests/cpp/<name>.cpp (headers only, no library): the executable's path."""
    exe = os.path.join(str(out_dir), name)
    r = subprocess.run(["g++", "-std=c++14", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


# the cases of tests/cpp/collision_kats.cpp: case -> (reference mode, strict mode); 0 occupied, 1 unseen, 2 empty
COLLISION_KATS_EXPECTED = {
    "TotallyUnseen": (1, 1), "PartiallyUnseen": (1, 1), "Empty": (2, 2), "Collision": (0, 0), "CollisionFreeLeaf": (2, 2),
    # an occupied voxel in the block of larger Morton code: the reference's last visited leaf (the smaller one, all empty) replaces it
    "QuirkLeafOrder": (2, 0),
    # the absent child's own value_[1] is occupied, the reference reads the parent's value_[0] (empty)
    "QuirkParentSlot0": (2, 0),
    # box (2,2,2) side 2: the inclusive test reaches voxel (4,4,4), which is occupied
    "QuirkInclusive": (0, 2),
}


# ------------------------------------------------------------------ Morton keys: code of the voxel corner | level (include/se_hip.h)
def spread(v):
    v = np.asarray(v, np.uint64)
    r = np.zeros_like(v)
    for i in range(21):
        r |= ((v >> np.uint64(i)) & np.uint64(1)) << np.uint64(3 * i)
    return r


def unpack(code):
    """The inverse of spread on each axis, of uint64 codes taken whole (a key's level bits included): [n, 3]."""
    code = code.astype(np.uint64)
    out = np.zeros((len(code), 3), np.int64)
    for b in range(21):
        for k in range(3):
            out[:, k] |= ((code >> np.uint64(3 * b + k)) & np.uint64(1)).astype(np.int64) << b
    return out


def make_keys(corner, level):
    """Morton code of the voxel corners [n, 3] | level."""
    c = np.asarray(corner, np.int64).reshape(-1, 3)
    return spread(c[:, 0]) | (spread(c[:, 1]) << np.uint64(1)) | (spread(c[:, 2]) << np.uint64(2)) | np.uint64(level)


def morton(x, y, z):
    """Morton code of one voxel corner, a Python int."""
    k = 0
    for i in range(21):
        k |= ((x >> i) & 1) << (3 * i) | ((y >> i) & 1) << (3 * i + 1) | ((z >> i) & 1) << (3 * i + 2)
    return k


def decode(code):
    """One key -> (x, y, z, level)."""
    m = int(code) & ~0x1FF
    x = y = z = 0
    for i in range(21):
        x |= ((m >> (3 * i)) & 1) << i
        y |= ((m >> (3 * i + 1)) & 1) << i
        z |= ((m >> (3 * i + 2)) & 1) << i
    return x, y, z, int(code) & 0x1FF


# ------------------------------------------------------------------ region allocation: the truth, in numpy, from the definitions of include/se_hip.h
def box_records(rows):
    """[(lo, hi, level[, reserved])] -> ALLOC_DTYPE records."""
    from supereight_amd.pipeline import ALLOC_DTYPE
    rec = np.zeros(len(rows), ALLOC_DTYPE)
    for i, r in enumerate(rows):
        rec[i]["lo"], rec[i]["hi"], rec[i]["level"] = r[0], r[1], r[2]
        rec[i]["reserved"] = r[3] if len(r) > 3 else 0
    return rec


def valid(r, leaf):
    return (all(-LIMIT <= int(v) <= LIMIT for v in list(r["lo"]) + list(r["hi"])) and 0 <= int(r["level"]) <= leaf and int(r["reserved"]) == 0)


def closure_truth(size, rec):
    """The definition, literally: per valid box every octant of its level whose cube meets the box inside the volume; the requested keys,
    their ancestor closure (the root left out), the number of (box, octant) pairs and of invalid boxes."""
    max_level = int(np.log2(size))
    leaf = max_level - 3
    requested, closure, pairs, invalid = set(), set(), 0, 0
    for r in rec:
        if not valid(r, leaf):
            invalid += 1
            continue
        level = leaf if int(r["level"]) == 0 else int(r["level"])
        side = size >> level
        lo = np.maximum(r["lo"].astype(np.int64), 0)
        hi = np.minimum(r["hi"].astype(np.int64), size)
        if (lo >= hi).any():
            continue
        ax = [np.arange(lo[k] // side, (hi[k] - 1) // side + 1) for k in range(3)]
        g = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3) * side
        pairs += len(g)
        requested.update(make_keys(g, level).tolist())
        for l in range(level, 0, -1):
            s = size >> l
            closure.update(np.unique(make_keys(g // s * s, l)).tolist())
    return requested, closure, pairs, invalid
