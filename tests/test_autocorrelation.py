"""The device autocorrelation reducer (smcmc_autocorrelation_sums) against the restatement of
MakeAutocorrelation.C:108-148 in oracle/oracle.py."""
import numpy as np
import pytest


def _rho(total, lagged, nslots, nchains):
    n = (nslots - np.arange(lagged.shape[0]))[:, None] * float(nchains)
    mean = total / n[0]
    var = lagged[0] / n[0] - mean * mean
    return (lagged / n - mean * mean) / var


def test_pooled_sums_reproduce_the_macro_on_one_chain(oracle):
    """One chain, one dimension: the pooled-sum form equals the macro's ring-buffer loop."""
    rng = np.random.default_rng(1)
    n, phi = 4000, 0.8
    s = np.zeros(n)
    for t in range(1, n):
        s[t] = phi * s[t - 1] + rng.standard_normal()
    s += 3.0
    total, lagged = oracle.autocorrelation_sums(s[:, None, None], nlags=16)
    rho = _rho(total, lagged, n, 1)[:, 0]
    ref = oracle.autocorrelation_reference(s, 16)
    assert np.allclose(rho[1:], ref[1:], rtol=0, atol=1e-12)
    assert np.allclose(rho[1:6], phi ** np.arange(1, 6), atol=0.06)        # AR(1): a(k) = phi^k
    shifted, lagged2 = oracle.autocorrelation_sums(s[:, None, None], centre=[2.5], nlags=16)
    # a reference point only enters through the edges of the lagged sums: O(lag / n)
    assert np.allclose(_rho(shifted, lagged2, n, 1)[:, 0], rho, atol=16 / n * 3)


def test_python_autocorrelation_class(smcmc, oracle):
    rng = np.random.default_rng(2)
    x = rng.standard_normal((300, 3, 40)).cumsum(axis=0) * 0.01 + rng.standard_normal((300, 3, 40))
    total, lagged = oracle.autocorrelation_sums(x)
    a = smcmc.Autocorrelation(total, lagged, 300, 40)
    assert np.allclose(a.rho(), _rho(total, lagged, 300, 40))
    half = [oracle.autocorrelation_sums(x[:, :, :20]), oracle.autocorrelation_sums(x[:, :, 20:])]
    b = smcmc.Autocorrelation(*half[0], 300, 20) + smcmc.Autocorrelation(*half[1], 300, 20)
    assert np.allclose(b.rho(), a.rho(), rtol=1e-12, atol=1e-14)              # ranks add their sums
    assert np.all(a.tau() >= 1.0 - 0.2)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,nchains,steps,stride", [(5, 70, 640, 4), (50, 256, 512, 8), (100, 64, 80, 1)])
def test_device_sums_match_oracle(gpu, oracle, dim, nchains, steps, stride):
    import torch
    # D > 63 saves a trace with a frozen covariance only
    e = gpu.Engine(dim, nchains, seed=9, mode=gpu.MODE_FROZEN if dim > 63 else gpu.MODE_POOLED)
    assert e.Start(np.zeros(dim))
    e.Step(300)
    slots = steps // stride
    sx = torch.full((slots, e.dim_padded, e.nchains_padded), float("nan"), dtype=torch.float64, device="cuda")
    sl = torch.empty((slots, e.nchains_padded), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    e.StepSave(steps, sx.data_ptr(), sl.data_ptr(), stride=stride)
    torch.cuda.synchronize()
    centre = e.GetEstimatedCenter()
    a = e.AutocorrelationSums(sx.data_ptr(), slots, centre=centre)
    x = sx[:, :dim, :nchains].cpu().numpy()
    total, lagged = oracle.autocorrelation_sums(x, centre, nlags=64)
    assert np.allclose(a.sum, total, rtol=1e-11, atol=1e-9)
    assert np.allclose(a.lagged, lagged, rtol=1e-11, atol=1e-9)
    again = e.AutocorrelationSums(sx.data_ptr(), slots, centre=centre)
    plain = e.AutocorrelationSums(sx.data_ptr(), slots)                         # the macro's own origin
    assert np.allclose(plain.lagged, oracle.autocorrelation_sums(x, None, nlags=64)[1], rtol=1e-11, atol=1e-9)
    assert np.array_equal(a.lagged, again.lagged) and np.array_equal(a.sum, again.sum)   # fixed summation order
    rho = a.rho()
    assert np.allclose(rho[0], 1.0) and np.all(np.abs(rho[:min(slots, 64)]) < 1.5)
    assert np.all(a.tau() > 0.5)


@pytest.mark.gpu
def test_device_sums_reject_bad_arguments(gpu):
    import ctypes as C
    lib = gpu.load()
    out = (C.c_double * 64)()
    assert lib.smcmc_autocorrelation_sums(None, 4, 2, 2, 64, 64, None, out, out, None) == 1       # SMCMC_ERR_INVALID


# ---- the reducer against exact sums, at shapes free of an engine's (the C entry through ctypes) ----------------------

def _device_sums(gpu, x, nchains_padded, dim_stride, centre):
    """x[slot][dim][chain] written into a trace [slot][dim_stride][nchains_padded] whose padding lanes and rows >= dim
    are NaN; returns (sum[dim], lagged[64][dim]) of smcmc_autocorrelation_sums."""
    import ctypes as C
    import torch
    nslots, dim, nchains = x.shape
    trace = torch.full((nslots, dim_stride, nchains_padded), float("nan"), dtype=torch.float64, device="cuda")
    trace[:, :dim, :nchains] = torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    torch.cuda.synchronize()
    total = np.full(dim, np.nan)
    lagged = np.full((64, dim), np.nan)
    dp = C.POINTER(C.c_double)
    c = None if centre is None else np.ascontiguousarray(centre, dtype=np.float64)
    st = gpu.load().smcmc_autocorrelation_sums(C.c_void_p(trace.data_ptr()), nslots, dim, dim_stride, nchains, nchains_padded,
                                               None if c is None else c.ctypes.data_as(dp), total.ctypes.data_as(dp),
                                               lagged.ctypes.data_as(dp), None)
    assert st == 0, st
    return total, lagged


def _exact_sums(y):
    """y[slot][dim][chain], an int64 array of integers small enough that nothing here leaves int64 (the caller says
    why): (sum[dim], lagged[64][dim]) exactly."""
    assert y.dtype == np.int64
    nslots = y.shape[0]
    lagged = np.zeros((64, y.shape[1]), dtype=np.int64)
    for k in range(min(64, nslots)):
        lagged[k] = (y[k:] * y[:nslots - k]).sum(axis=(0, 2))
    return y.sum(axis=(0, 2)), lagged


SLOTS = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 100]


@pytest.mark.gpu
@pytest.mark.parametrize("nchains,extra_blocks", [(1, 0), (63, 0), (64, 0), (65, 0), (200, 0), (65, 2)])
def test_device_sums_are_exact_on_integers(gpu, nchains, extra_blocks):
    """Integer data in [-1024, 1024] about an integer centre: every product and every partial sum is an integer below
    2^53 (at most 100 * 200 * 2048^2 < 2^37: int64 holds the truth, a double every partial sum), so every summation order
    gives the same double and the tolerance is zero.
    nslots off the 16-slot register block and below 64 / 32 (lags that reach before the first slot in both passes), a last
    chain block with one live lane (65, and 1), padding of NaN.  Lags >= nslots are exactly 0."""
    rng = np.random.default_rng(nchains)
    npad = (nchains + 63) // 64 * 64 + 64 * extra_blocks
    for nslots in SLOTS:
        for dim, stride in ((1, 1), (3, 3), (1, 6), (3, 8)):
            x = rng.integers(-1024, 1025, size=(nslots, dim, nchains))
            centre = rng.integers(-1024, 1025, size=dim)
            for c in (None, centre):
                total, lagged = _exact_sums(x - (0 if c is None else c[None, :, None]))
                got_total, got_lagged = _device_sums(gpu, x.astype(np.float64), npad, stride, None if c is None else c.astype(np.float64))
                tag = "nslots=%d nchains=%d/%d dim=%d/%d centre=%s" % (nslots, nchains, npad, dim, stride, c is not None)
                assert np.array_equal(got_total, total.astype(np.float64)), tag
                assert np.array_equal(got_lagged, lagged.astype(np.float64)), tag
                assert np.all(got_lagged[min(nslots, 64):] == 0.0), tag


def _dyadic(a, extra=()):
    """Doubles as Python ints over one power of two: (object array of a's shape, ints of `extra`, den)."""
    flat = [float(v).as_integer_ratio() for v in np.ravel(a)] + [float(v).as_integer_ratio() for v in extra]
    den = max(d for _, d in flat)
    ints = [n * (den // d) for n, d in flat]
    out = np.empty(np.size(a), dtype=object)
    out[:] = ints[:np.size(a)]
    return out.reshape(np.shape(a)), ints[np.size(a):], den


@pytest.mark.gpu
@pytest.mark.parametrize("nslots,nchains", [(100, 200), (33, 65), (64, 130), (17, 1)])
def test_device_sums_within_the_rounding_bound(gpu, nslots, nchains):
    """AR(1) data about no centre, the ensemble mean, and mean + 1e8 (y = x - c is one rounding of a difference of
    doubles; about the far centre every product is ~1e16 and nothing cancels here, it cancels later in a(lag)).  Truth:
    exact integers (the doubles over one power of two).  Bound: gamma_m sum |y_t y_(t-k)| with m = terms per output + 2
    (the two roundings of y in each product; the fused multiply-add rounds once per term; the butterfly and the block sum
    are additions of the same sum), times 2 for the second order, as tests/truth.py has it; the plain sum has
    m = terms + 1 and S = sum |y|."""
    from fractions import Fraction
    rng = np.random.default_rng(nslots)
    dim = 2
    x = np.zeros((nslots, dim, nchains))
    x[0] = rng.standard_normal((dim, nchains))
    for t in range(1, nslots):
        x[t] = 0.9 * x[t - 1] + rng.standard_normal((dim, nchains))
    x += np.array([3.0, -40.0])[None, :, None]
    mean = x.mean(axis=(0, 2))
    u = Fraction(1, 2 ** 53)

    def gamma(m):
        return m * u / (1 - m * u)
    npad = (nchains + 63) // 64 * 64
    for centre in (None, mean, mean + 1e8):
        X, C, den = _dyadic(x, [0.0] * dim if centre is None else centre)
        Y = X - np.array(C, dtype=object)[None, :, None]
        A = np.abs(Y)
        got_total, got_lagged = _device_sums(gpu, x, npad, dim + 5, centre)
        worst = 0.0
        for d in range(dim):
            total, stotal = sum(Y[:, d].ravel().tolist()), sum(A[:, d].ravel().tolist())
            err = abs(Fraction(*float(got_total[d]).as_integer_ratio()) - Fraction(total, den))
            bound = 2 * gamma(nslots * nchains + 1) * Fraction(stotal, den)
            assert err <= bound, ("sum", d, float(err), float(bound))
            for k in range(64):
                if k >= nslots:
                    assert got_lagged[k, d] == 0.0
                    continue
                lag = sum((Y[k:, d] * Y[:nslots - k, d]).ravel().tolist())
                slag = sum((A[k:, d] * A[:nslots - k, d]).ravel().tolist())
                bound = 2 * gamma((nslots - k) * nchains + 2) * Fraction(slag, den * den)
                err = abs(Fraction(*float(got_lagged[k, d]).as_integer_ratio()) - Fraction(lag, den * den))
                worst = max(worst, float(err / bound))
                assert err <= bound, ("lag", k, d, float(err), float(bound), centre is not None)
        print("nslots=%d nchains=%d centre=%s: worst |error| / bound = %.3g" % (nslots, nchains, "none" if centre is None else "%.6g" % centre[0], worst))


@pytest.mark.gpu
def test_device_sums_reject_more_bad_arguments(gpu):
    import ctypes as C
    import torch
    lib = gpu.load()
    trace = torch.zeros((4, 2, 64), dtype=torch.float64, device="cuda")
    t = C.c_void_p(trace.data_ptr())
    out = (C.c_double * 128)()
    lag = (C.c_double * 128)()
    invalid = 1                                                                     # SMCMC_ERR_INVALID
    assert lib.smcmc_autocorrelation_sums(t, 4, 2, 2, 64, 64, None, out, lag, None) == 0
    assert lib.smcmc_autocorrelation_sums(t, 0, 2, 2, 64, 64, None, out, lag, None) == invalid      # nslots = 0
    assert lib.smcmc_autocorrelation_sums(t, 4, 2, 1, 64, 64, None, out, lag, None) == invalid      # dim_stride < dim
    assert lib.smcmc_autocorrelation_sums(t, 4, 2, 2, 60, 60, None, out, lag, None) == invalid      # not a multiple of 64
    assert lib.smcmc_autocorrelation_sums(t, 4, 2, 2, 65, 64, None, out, lag, None) == invalid      # padded < nchains
    assert lib.smcmc_autocorrelation_sums(t, 4, 2, 2, 64, 64, None, None, lag, None) == invalid     # null sum
    assert lib.smcmc_autocorrelation_sums(t, 4, 2, 2, 64, 64, None, out, None, None) == invalid     # null lagged
    assert lib.smcmc_autocorrelation_sums(t, 4, 0, 2, 64, 64, None, out, lag, None) == invalid      # dim = 0
    assert lib.smcmc_autocorrelation_sums(t, 4, 2, 2, 0, 64, None, out, lag, None) == invalid       # nchains = 0
