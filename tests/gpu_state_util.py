"""What the GPU tests of the batched entry points share: a handle driven over a synthetic stream, the snapshot that the "a call disturbs
nothing" tests compare, and the streaming twin run of the "flushes a deferred raycast first" tests."""
import numpy as np

from supereight_amd.pipeline import SDF, DenseSLAMPipeline
from supereight_amd.synthetic import make_stream

W, H = 160, 120


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def map_state(p):
    """The map and both images as downloaded, floats as bit patterns: block coords, x, y, active flags; node code, side, x, y; vertex and
    normal image.  Two states are equal iff all((u == w).all() for u, w in zip(a, b))."""
    c, x, y, a = p.blocks()
    code, side, nx, ny = p.nodes()
    v, n = p.vertex_normal()
    return [c, bits(x), bits(y), a, code, side, bits(nx), bits(ny), bits(v), bits(n)]


def run_stream(kind, field, n, dim, max_blocks, frames, streaming=False, check=None):
    """A 160x120 handle after `frames` frames of the stream `kind`; check(p, f) is called after every frame."""
    mu = 0.1 if field == SDF else 0.02
    s = make_stream(kind, W, H, dim, holes=False)
    p = DenseSLAMPipeline((W, H), n, dim, field_type=field, max_blocks=max_blocks, streaming=streaming)
    for f in range(frames):
        p.set_depth(s.depth(f))
        p.setPose(s.pose(f))
        p.integration(s.k, 1, mu, f)
        if streaming:
            p.raycasting_deferred(s.k, mu, f)
        else:
            p.raycasting(s.k, mu, f)
        if check is not None:
            check(p, f)
    return p


def streamed_with(action, at_frame, frames=8, slots=8, again=None, at_end=None):
    """A streaming 256^3 SDF handle with an image ring over the room stream; after frame `at_frame` (-1: never), with that frame's raycast
    held back, action(p, box) and then again(p, box) (default: the action once more) run on a box over most of the room, the visible
    surfaces included.  Returns the ring's images and the log: fused, the launch counters before / after the first call / after the second,
    and the first call's result as counts.  at_end(p, log) runs after the last frame, before the handle is closed."""
    import torch
    n, dim, mu = 256, 2.4, 0.1
    s = make_stream("room", W, H, dim, holes=False)
    p = DenseSLAMPipeline((W, H), n, dim, field_type=SDF, streaming=True)
    ring = torch.zeros((slots, 2, W * H * 3), dtype=torch.float32, device="cuda:0")
    p.set_image_ring(ring.data_ptr(), slots, keepalive=ring)
    box = np.array([[0, 0, 0, n, n, 200]], np.int32)
    log = {}
    for f in range(frames):
        p.set_depth(s.depth(f)); p.setPose(s.pose(f))
        p.integration(s.k, 1, mu, f)
        p.raycasting_deferred(s.k, mu, f)
        if f == at_frame:
            log["fused"] = p.frame_is_fused()
            log["before"] = p.launch_counts()
            log["counts"] = action(p, box)
            log["after"] = p.launch_counts()
            (again or action)(p, box)
            log["again"] = p.launch_counts()
    p.sync()
    out = ring.cpu().numpy().copy()
    if at_end is not None:
        at_end(p, log)
    p.close()
    return out, log
