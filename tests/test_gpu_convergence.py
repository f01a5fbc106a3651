"""The device sums behind split R-hat and the multi-chain ESS (smcmc_trace_convergence) against the restatement and the
exact sums of tests/convergence_ref.py."""
import ctypes as C
import importlib.util
import os
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("smcmc_convergence_ref", os.path.join(HERE, "convergence_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

DP = C.POINTER(C.c_double)
INVALID = 1                                                      # SMCMC_ERR_INVALID
LAGS = 64


def _nan_trace(x, nchains_padded, dim_stride):
    """x[slot][dim][chain] in a device trace [slot][dim_stride][nchains_padded] whose padding lanes and rows >= dim
    are NaN."""
    import torch
    nslots, dim, nchains = x.shape
    trace = torch.full((nslots, dim_stride, nchains_padded), float("nan"), dtype=torch.float64, device="cuda")
    trace[:, :dim, :nchains] = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to("cuda")
    torch.cuda.synchronize()
    return trace


def _device(gpu, trace, nslots, dim, dim_stride, nchains, nchains_padded, S, centre, chain_sums=True):
    """dict(sum, sumsq_of_sums, within, chain_sums[S][dim][padded] or None) of smcmc_trace_convergence; the outputs are
    prefilled with NaN."""
    import torch
    total, sumsq, within = np.full(dim, np.nan), np.full(dim, np.nan), np.full((LAGS, dim), np.nan)
    cs = torch.full((S, dim, nchains_padded), float("nan"), dtype=torch.float64, device="cuda") if chain_sums else None
    torch.cuda.synchronize()
    c = None if centre is None else np.ascontiguousarray(centre, dtype=np.float64)
    st = gpu.load().smcmc_trace_convergence(C.c_void_p(trace.data_ptr()), nslots, dim, dim_stride, nchains, nchains_padded, S,
                                            None if c is None else c.ctypes.data_as(DP),
                                            C.c_void_p(cs.data_ptr()) if chain_sums else None, total.ctypes.data_as(DP),
                                            sumsq.ctypes.data_as(DP), within.ctypes.data_as(DP), None)
    assert st == 0, st
    torch.cuda.synchronize()
    return dict(sum=total, sumsq_of_sums=sumsq, within=within, chain_sums=cs.cpu().numpy() if chain_sums else None)


def _floats(a):
    return np.array([float(v) for v in a.ravel()]).reshape(a.shape)


# every L of {2, 4, 16, 32, 64, 128}, every S of {1, 2, 3} with r = 0 and with r of {1, 2}, every nchains / padded of
# {1/64, 63/64, 64/64, 65/128, 200/256, 65/256} and every (dim, dim_stride) of {(1,1), (3,8), (50,64), (64,64), (65,72)}
# at least once: (nslots, S, nchains, padded, dim, dim_stride)
INTEGER_CASES = [(2, 1, 1, 64, 1, 1), (8, 2, 63, 64, 3, 8), (49, 3, 64, 64, 50, 64), (65, 2, 65, 128, 64, 64),
                 (128, 2, 200, 256, 3, 8), (128, 1, 65, 256, 1, 1), (50, 3, 200, 256, 65, 72), (256, 2, 63, 64, 3, 8),
                 (14, 3, 65, 128, 50, 64), (64, 1, 1, 64, 65, 72), (5, 2, 65, 256, 64, 64), (96, 3, 64, 64, 1, 1),
                 (193, 3, 65, 128, 3, 8), (32, 2, 1, 64, 50, 64), (385, 3, 200, 256, 1, 1)]


def _integer_data(nslots, S, nchains, dim):
    rng = np.random.default_rng(1000 * nslots + 10 * nchains + dim + S)
    return rng.integers(-1024, 1025, size=(nslots, dim, nchains)), rng.integers(-1024, 1025, size=dim)


def _check_exact(got, x, S, nchains, centre):
    """Zero tolerance, and the premise of it: every partial sum of every output is below 2^53 in the unit of its terms
    (2^-2 log2 L for a product of two z; sum |z_t z_(t-k)| <= sum z^2 = within[0] by Cauchy-Schwarz)."""
    want = R.exact_sums(x, S, centre)
    L = want["L"]
    assert L & (L - 1) == 0
    assert np.all(want["within"][0] * L * L < 2 ** 53) and np.all(want["sumsq_of_sums"] < 2 ** 53)
    for name in ("sum", "sumsq_of_sums", "within"):
        assert np.array_equal(got[name], _floats(want[name])), name
    assert np.array_equal(got["within"][L:], np.zeros_like(got["within"][L:]))            # rows k >= L
    assert np.array_equal(got["chain_sums"][:, :, :nchains], _floats(want["chain_sums"]))
    assert np.array_equal(got["chain_sums"][:, :, nchains:], np.zeros_like(got["chain_sums"][:, :, nchains:]))


@pytest.mark.parametrize("nslots,S,nchains,npad,dim,stride", INTEGER_CASES)
def test_device_sums_are_exact_on_integers(gpu, nslots, S, nchains, npad, dim, stride):
    """Integers in [-1024, 1024] about an integer centre and L a power of two: s1 / L, z and every product are dyadic
    and every partial sum stays below 2^53 (asserted on the data), so every summation order gives the same double and
    the tolerance is zero.  One live lane in the last block (65, 1), a whole dead block (65 / 256), L on both sides of
    the register block of 16 and of the 32 lags of a launch, leading slots that are dropped; padding of NaN."""
    x, centre = _integer_data(nslots, S, nchains, dim)
    trace = _nan_trace(x, npad, stride)
    for c in (None, centre.astype(np.float64)):
        _check_exact(_device(gpu, trace, nslots, dim, stride, nchains, npad, S, c), x, S, nchains, c)


@pytest.mark.parametrize("nslots,S,nchains,npad,dim,stride", [INTEGER_CASES[3], INTEGER_CASES[6]])
def test_the_dropped_slots_are_not_read(gpu, nslots, S, nchains, npad, dim, stride):
    """r = 1 and r = 2: NaN in the r leading slots changes nothing."""
    x, centre = _integer_data(nslots, S, nchains, dim)
    r = R.layout(nslots, S)[1]
    assert r > 0
    y = x.astype(np.float64)
    y[:r] = np.nan
    got = _device(gpu, _nan_trace(y, npad, stride), nslots, dim, stride, nchains, npad, S, centre.astype(np.float64))
    for name in ("sum", "sumsq_of_sums", "within"):
        assert np.all(np.isfinite(got[name])), name
    _check_exact(got, x, S, nchains, centre.astype(np.float64))


def _ar1_trace(nslots, dim, nchains, seed):
    rng = np.random.default_rng(seed)
    x = np.zeros((nslots, dim, nchains))
    x[0] = rng.standard_normal((dim, nchains))
    for t in range(1, nslots):
        x[t] = 0.9 * x[t - 1] + rng.standard_normal((dim, nchains))
    return x * np.linspace(0.5, 3.0, dim)[None, :, None] + np.linspace(3.0, -40.0, dim)[None, :, None]


# L = 50, 16, 17, 43, 48: both sides of 16, 32, 48 and (with the integer cases) 64; none a power of two but 16
@pytest.mark.parametrize("nslots,nchains,dim,S", [(100, 200, 2, 2), (33, 65, 3, 2), (17, 1, 2, 1), (130, 65, 2, 3), (97, 64, 1, 2)])
def test_device_sums_within_the_rounding_bound(gpu, nslots, nchains, dim, S):
    """AR(1) data about no centre, the ensemble mean, and mean + 1e8 (there y is ~1e8 with a rounding of ~1e-8 each, and
    z = y - mean cancels back to the data's scale).  Truth: exact integers; bound: tests/convergence_ref.py derives it."""
    x = _ar1_trace(nslots, dim, nchains, nslots + dim)
    npad = (nchains + 63) // 64 * 64
    trace = _nan_trace(x, npad, dim + 5)
    mean = x.mean(axis=(0, 2))
    for centre in (None, mean, mean + 1e8):
        got = _device(gpu, trace, nslots, dim, dim + 5, nchains, npad, S, centre)
        got["chain_sums"] = got["chain_sums"][:, :, :nchains]
        worst = R.check_rounding_bound(got, x, S, centre, "centre=%s" % (None if centre is None else centre[0]))
        print("nslots=%d nchains=%d dim=%d S=%d centre=%s: worst |error| / bound = %.3g"
              % (nslots, nchains, dim, S, "none" if centre is None else "%.6g" % centre[0], worst))


def test_device_sums_give_the_same_bits_twice(gpu):
    for nslots, nchains, dim in ((40, 300, 50), (9, 130, 100)):
        x = _ar1_trace(nslots, dim, nchains, 3)
        npad = (nchains + 63) // 64 * 64
        trace = _nan_trace(x, npad, dim)
        a = _device(gpu, trace, nslots, dim, dim, nchains, npad, 2, x.mean(axis=(0, 2)))
        b = _device(gpu, trace, nslots, dim, dim, nchains, npad, 2, x.mean(axis=(0, 2)))
        for name in ("sum", "sumsq_of_sums", "within", "chain_sums"):
            assert np.array_equal(a[name], b[name]), name
            assert np.all(np.isfinite(a[name])), name


def test_one_chain_against_the_pooled_reducer(gpu):
    """S = 1 and a single chain: within[k] and smcmc_autocorrelation_sums describe the same chain,
    within[k] = lagged[k] - mean (sum_{t >= k} y + sum_{t < L - k} y) + (L - k) mean^2.  The identity is checked in
    exact arithmetic on the restatement's side; each device result is held to its own bound of its own exact value
    (the pooled sums: 2 gamma_(n+2) sum |y_t y_(t-k)|, n terms, as tests/trace_moments_ref.py has it).  Device is not
    compared with device."""
    nslots, dim = 80, 2
    x = _ar1_trace(nslots, dim, 1, 11)
    centre = x.mean(axis=(0, 2)) + 0.5
    trace = _nan_trace(x, 64, dim)
    got = _device(gpu, trace, nslots, dim, dim, 1, 64, 1, centre)
    got["chain_sums"] = got["chain_sums"][:, :, :1]
    exact = R.exact_sums(x, 1, centre)
    lagged_exact, lagged_abs, rebuilt = R.exact_pooled_lagged(x, centre)
    assert np.all(rebuilt == exact["within"])                                 # the identity, exactly
    worst = R.check_rounding_bound(got, x, 1, centre, "one chain", exact=exact)
    total, lagged = np.full(dim, np.nan), np.full((LAGS, dim), np.nan)
    st = gpu.load().smcmc_autocorrelation_sums(C.c_void_p(trace.data_ptr()), nslots, dim, dim, 1, 64, centre.ctypes.data_as(DP),
                                               total.ctypes.data_as(DP), lagged.ctypes.data_as(DP), None)
    assert st == 0
    worst_pooled = 0.0
    for k in range(LAGS):
        for d in range(dim):
            bound = 2 * R.gamma((nslots - k) + 2) * R.F(lagged_abs[k, d])
            err = abs(R.F(lagged[k, d]) - lagged_exact[k, d])
            assert err <= bound, (k, d, float(err), float(bound))
            worst_pooled = max(worst_pooled, float(err / bound))
    print("one chain: worst |error| / bound = %.3g (within), %.3g (pooled lagged)" % (worst, worst_pooled))


def _check_engine_trace(c, x, S, centre, tag):
    """c: the Convergence of the engine's method; x[slot][dim][chain] the copied-back trace."""
    got = dict(sum=c.sum, sumsq_of_sums=c.sumsq_of_sums, within=c.within)
    worst = R.check_rounding_bound(got, x, S, centre, tag)
    assert (c.L, c.M) == (x.shape[0] // S, S * x.shape[2])
    assert np.all(np.isfinite(c.rhat())), c.rhat()
    print("%s: worst |error| / bound = %.3g, rhat %s" % (tag, worst, np.array2string(c.rhat(), precision=3)))


def test_engine_trace(gpu):
    import torch
    dim, nchains, slots = 8, 130, 64
    e = gpu.Engine(dim, nchains, seed=9, mode=gpu.MODE_POOLED)
    assert e.Start(np.zeros(dim))
    e.Step(200)
    sx = torch.full((slots, e.dim_padded, e.nchains_padded), float("nan"), dtype=torch.float64, device="cuda")
    sl = torch.empty((slots, e.nchains_padded), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    e.StepSave(slots, sx.data_ptr(), sl.data_ptr(), stride=1)
    torch.cuda.synchronize()
    x = sx[:, :dim, :nchains].cpu().numpy()
    centre = e.GetEstimatedCenter()
    _check_engine_trace(e.Convergence(sx.data_ptr(), slots, centre=centre), x, 2, centre, "Engine about its centre")
    _check_engine_trace(e.Convergence(sx.data_ptr(), slots, nsegments=3), x, 3, None, "Engine in thirds about the origin")


def test_hmc_engine_trace(gpu):
    import torch
    dim, nchains, slots = 5, 64, 12
    h = gpu.HmcEngine(dim, nchains, seed=4)
    h.SetMeanEpsilon(-0.2)
    h.SetLeapFrog(5)
    h.Start(np.random.default_rng(1).normal(size=(dim, nchains)))
    trace = torch.full((slots, dim, h.nchains_padded), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for k in range(slots):
        h.Step(1)
        h.copy_positions(trace[k].data_ptr())
    h.sync()
    torch.cuda.synchronize()
    _check_engine_trace(h.Convergence(trace.data_ptr(), slots), trace[:, :, :nchains].cpu().numpy(), 2, None, "HmcEngine")


def test_vaat_engine_trace(gpu):
    import torch
    dim, nchains, steps, stride = 7, 70, 80, 4
    e = gpu.VaatEngine(dim, nchains, seed=2)
    assert e.Start(np.zeros(dim))
    slots = steps // stride
    sx = torch.full((slots, dim, e.nchains_padded), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    e.step_save(steps, stride, sx.data_ptr())
    torch.cuda.synchronize()
    _check_engine_trace(e.Convergence(sx.data_ptr(), slots), sx[:, :, :nchains].cpu().numpy(), 2, None, "VaatEngine")


def test_device_sums_reject_bad_arguments(gpu):
    import torch
    lib = gpu.load()
    trace = torch.zeros((8, 2, 64), dtype=torch.float64, device="cuda")
    sentinel = -12345.0
    cs = torch.full((2, 2, 64), sentinel, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    t, s = C.c_void_p(trace.data_ptr()), C.c_void_p(cs.data_ptr())
    out, sq, w = np.full(2, sentinel), np.full(2, sentinel), np.full((LAGS, 2), sentinel)
    po, ps, pw = out.ctypes.data_as(DP), sq.ctypes.data_as(DP), w.ctypes.data_as(DP)
    big = lib.smcmc_max_dim() + 1
    f = lib.smcmc_trace_convergence
    #           trace nslots dim stride nchains padded S centre chain_sums sum sumsq within stream
    bad = [(t, 8, 2, 2, 64, 64, 0, None, s, po, ps, pw, None),        # nsegments < 1
           (t, 8, 2, 2, 64, 64, -1, None, s, po, ps, pw, None),
           (t, 3, 2, 2, 64, 64, 2, None, s, po, ps, pw, None),        # L = 1
           (t, 8, 2, 2, 64, 64, 5, None, s, po, ps, pw, None),        # L = 1
           (t, 0, 2, 2, 64, 64, 1, None, s, po, ps, pw, None),        # L = 0
           (t, 8, 0, 2, 64, 64, 2, None, s, po, ps, pw, None),        # dim < 1
           (t, 8, big, big, 64, 64, 2, None, s, po, ps, pw, None),    # dim > smcmc_max_dim()
           (t, 8, 2, 1, 64, 64, 2, None, s, po, ps, pw, None),        # dim_stride < dim
           (t, 8, 2, 2, 0, 64, 2, None, s, po, ps, pw, None),         # nchains < 1
           (t, 8, 2, 2, 65, 64, 2, None, s, po, ps, pw, None),        # padded < nchains
           (t, 8, 2, 2, 60, 60, 2, None, s, po, ps, pw, None),        # not a multiple of 64
           (None, 8, 2, 2, 64, 64, 2, None, s, po, ps, pw, None),     # null trace
           (t, 8, 2, 2, 64, 64, 2, None, s, None, ps, pw, None),      # null sum
           (t, 8, 2, 2, 64, 64, 2, None, s, po, None, pw, None),      # null sumsq_of_sums
           (t, 8, 2, 2, 64, 64, 2, None, s, po, ps, None, None)]      # null within
    for args in bad:
        assert f(*args) == INVALID, args[1:7]
    torch.cuda.synchronize()
    assert np.all(out == sentinel) and np.all(sq == sentinel) and np.all(w == sentinel)
    assert bool(torch.all(cs == sentinel))
    assert f(t, 8, 2, 2, 64, 64, 2, None, s, po, ps, pw, None) == 0    # and the good call writes all of them
    torch.cuda.synchronize()
    assert np.all(out == 0.0) and np.all(sq == 0.0) and np.all(w == 0.0) and bool(torch.all(cs == 0.0))
    assert f(t, 8, 2, 2, 64, 64, 2, None, None, po, ps, pw, None) == 0  # chain_sums is optional
