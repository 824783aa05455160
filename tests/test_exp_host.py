"""The exponential the bilateral filter is DEFINED with (oracle/se_oracle.cpp so_exp_f32; the device's se_exp_f32 says the same in the same
words and is held to it bit for bit in tests/test_gpu_icp_math.py) against exp at 120 bits, rounded once to float32, on every argument of
tests/bilateral_util.py exp_arguments(): the definition is the correctly rounded exponential there, denormal results included.  About 2^-28 of
all arguments lie so close to a rounding boundary that a double evaluation can round the other way; one that turns up in the list is named in
EXCEPTIONS with both bit patterns (three at the most, each 1 ulp off) -- measured: none."""
import numpy as np

from oracle.binding import oracle_exp
from tests import bilateral_util as B
from tests.icp_edge_util import same_bits

# argument bits -> (so_exp_f32's bits, the correctly rounded bits)
EXCEPTIONS: dict = {}


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))        # results are >= +0: the patterns are ordered


def test_the_list_holds_what_it_is_there_for():
    x = B.exp_arguments()
    fin = x[x >= -104]                                                         # (so_exp_f32 answers +0 below that, before any arithmetic)
    print(f"{x.size} arguments")
    assert x.size >= 250_000 and np.unique(x.view(np.uint32)).size == x.size
    assert np.isnan(x).sum() == 1 and (x == -np.inf).sum() == 1 and (x[np.isfinite(x) | np.isinf(x)] <= 0).all()
    assert (np.signbit(x) & (x == 0)).sum() == 1 and (~np.signbit(x) & (x == 0)).sum() == 1
    k = np.rint(fin.astype(np.float64) * 1.44269504088896338700e+00)
    assert set(range(-150, 1)) <= set(k.astype(int).tolist())                  # every scale 2^k the recipe can form
    ref = B.exp_reference()
    denormal = (ref > 0) & (ref < np.float32(1.17549435e-38))
    assert denormal.sum() > 20_000 and ((ref == 0) & np.isfinite(x)).sum() > 50 and (ref == 1).sum() > 10
    assert (ref.view(np.uint32) == 1).sum() > 30                               # ... down to the smallest denormal, next to those that round to 0
    w = B.workload_arguments()
    assert w.size > 400_000 and (w == 0).any() and w.min() < -104              # the filter's own arguments reach both ends
    assert np.isin(w.view(np.uint32), x.view(np.uint32)).all()


def test_definition_is_the_correctly_rounded_exponential():
    x, ref = B.exp_arguments(), B.exp_reference()
    got = oracle_exp(x)
    same = same_bits(got, ref)
    bad = np.flatnonzero(~same)
    print(f"{x.size} arguments, {bad.size} not correctly rounded; EXCEPTIONS holds {len(EXCEPTIONS)}")
    assert len(EXCEPTIONS) <= 3
    found = {int(x.view(np.uint32)[i]): (int(got.view(np.uint32)[i]), int(ref.view(np.uint32)[i])) for i in bad[:16]}
    assert found == EXCEPTIONS, {hex(a): (hex(g), hex(r)) for a, (g, r) in found.items()}
    assert all(abs(g - r) == 1 for g, r in EXCEPTIONS.values())
    assert (got.view(np.uint32)[x == 0] == 0x3F800000).all() and (got.view(np.uint32)[x < -104] == 0).all()       # 1 for both zeros, +0 below -104


def test_gaussian_table_literals():
    assert B.GAUSSIAN_ARGUMENTS.tolist() == [-0.125, -0.03125, 0.0, -0.03125, -0.125]
    got = oracle_exp(B.GAUSSIAN_ARGUMENTS)
    assert tuple(int(b) for b in got.view(np.uint32)) == B.GAUSSIAN_BITS, [hex(b) for b in got.view(np.uint32)]
    import mpmath
    with mpmath.workprec(120):
        want = [B.round_to_f32(mpmath.exp(mpmath.mpf(float(a)))) for a in B.GAUSSIAN_ARGUMENTS]
    assert tuple(int(np.float32(w).view(np.uint32)) for w in want) == B.GAUSSIAN_BITS


def test_definition_is_monotone():
    x = B.exp_arguments()[:-1]                                   # sorted ascending; the NaN is last
    assert (np.diff(x.astype(np.float64)) >= 0).all()
    got = oracle_exp(x)
    assert (np.diff(got.astype(np.float64)) >= 0).all()


def test_libm_expf_is_within_one_ulp_of_the_definition():
    """so_set_libm_exp(1) puts this host's expf in the definition's place.  A faithfully rounded expf returns one of the two floats around
    the exact value, the correctly rounded one the nearer of them: 1 ulp apart at the most."""
    x = B.exp_arguments()
    d, m = oracle_exp(x), oracle_exp(x, libm=True)
    nan = np.isnan(x)
    assert np.isnan(d[nan]).all() and np.isnan(m[nan]).all()
    u = _ulps(d[~nan], m[~nan])
    print(f"{x.size} arguments: this host's expf equals the definition on {100.0 * (u == 0).mean():.4f} %, worst {u.max()} ulp")
    assert u.max() <= 1
