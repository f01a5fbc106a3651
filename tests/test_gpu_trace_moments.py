"""The device mean / covariance sums of a saved trace (smcmc_trace_moments) and the device Cholesky chain
(smcmc_cholesky_chain) against the restatements of MakeCovariance.C and CholeskyChain.C in tests/trace_moments_ref.py
and against exact sums."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("smcmc_trace_moments_ref", os.path.join(HERE, "trace_moments_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

DP = C.POINTER(C.c_double)
INVALID, RUNTIME = 1, 3                                          # SMCMC_ERR_INVALID, SMCMC_ERR_RUNTIME


def _nan_trace(x, nchains_padded, dim_stride):
    """x[slot][dim][chain] in a device trace [slot][dim_stride][nchains_padded] whose padding lanes and rows >= dim
    are NaN."""
    import torch
    nslots, dim, nchains = x.shape
    trace = torch.full((nslots, dim_stride, nchains_padded), float("nan"), dtype=torch.float64, device="cuda")
    trace[:, :dim, :nchains] = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to("cuda")
    torch.cuda.synchronize()
    return trace


def _device_moments(gpu, trace, nslots, dim, dim_stride, nchains, nchains_padded, centre):
    total = np.full(dim, np.nan)
    sumsq = np.full((dim, dim), np.nan)
    c = None if centre is None else np.ascontiguousarray(centre, dtype=np.float64)
    st = gpu.load().smcmc_trace_moments(C.c_void_p(trace.data_ptr()), nslots, dim, dim_stride, nchains, nchains_padded,
                                        None if c is None else c.ctypes.data_as(DP), total.ctypes.data_as(DP),
                                        sumsq.ctypes.data_as(DP), None)
    assert st == 0, st
    return total, sumsq


# every value of nslots {1, 2, 3, 4, 5, 17, 100}, of nchains / padded {1/64, 63/64, 64/64, 65/128, 200/256, 65/256} and
# of (dim, dim_stride) {(1,1), (3,8), (15,15), (16,16), (17,24), (50,64), (63,63), (64,64), (65,72), (100,100)} at least
# once; the large ones together: (nslots, nchains, padded, dim, dim_stride)
INTEGER_CASES = [(1, 1, 64, 1, 1), (2, 63, 64, 3, 8), (3, 64, 64, 15, 15), (4, 65, 128, 16, 16), (5, 200, 256, 17, 24),
                 (17, 65, 256, 50, 64), (100, 1, 64, 63, 63), (1, 63, 64, 64, 64), (2, 64, 64, 65, 72),
                 (100, 200, 256, 100, 100), (100, 200, 256, 50, 64), (5, 65, 128, 63, 63), (17, 200, 256, 3, 8),
                 (3, 65, 256, 100, 100), (4, 1, 64, 50, 64)]


@pytest.mark.parametrize("nslots,nchains,npad,dim,stride", INTEGER_CASES)
def test_device_moments_are_exact_on_integers(gpu, nslots, nchains, npad, dim, stride):
    """Integer data in [-1024, 1024] about an integer centre: every product and every partial sum is an integer below
    100 * 200 * 2048^2 < 2^53, so every summation order gives the same double and the tolerance is zero.  One live lane
    in the last chain block (65, 1), a whole dead block (65 / 256), tile rows past dim in every tile-block shape, dim + 1
    on both sides of 16, 64 and of a tile block; padding of NaN."""
    rng = np.random.default_rng(1000 * nslots + nchains + dim)
    x = rng.integers(-1024, 1025, size=(nslots, dim, nchains))
    centre = rng.integers(-1024, 1025, size=dim)
    trace = _nan_trace(x, npad, stride)
    for c in (None, centre):
        y = (x - (0 if c is None else c[None, :, None])).transpose(1, 0, 2).reshape(dim, -1).astype(np.float64)
        want_total, want_sumsq = y.sum(axis=1), y @ y.T           # integers below 2^53: exact in any order
        total, sumsq = _device_moments(gpu, trace, nslots, dim, stride, nchains, npad, None if c is None else c.astype(np.float64))
        assert np.array_equal(total, want_total), c is not None
        assert np.array_equal(sumsq, want_sumsq), c is not None
        assert np.array_equal(sumsq, sumsq.T)


def _ar1_trace(nslots, dim, nchains, seed):
    rng = np.random.default_rng(seed)
    x = np.zeros((nslots, dim, nchains))
    x[0] = rng.standard_normal((dim, nchains))
    for t in range(1, nslots):
        x[t] = 0.9 * x[t - 1] + rng.standard_normal((dim, nchains))
    return x * np.linspace(0.5, 3.0, dim)[None, :, None] + np.linspace(3.0, -40.0, dim)[None, :, None]


@pytest.mark.parametrize("dim", [2, 50])
@pytest.mark.parametrize("nslots,nchains", [(100, 200), (33, 65), (17, 1)])
def test_device_moments_within_the_rounding_bound(gpu, nslots, nchains, dim):
    """AR(1) data about no centre, the ensemble mean, and mean + 1e8 (about the far centre every product is ~1e16 and
    nothing cancels here; it cancels later, in sumsq / n - mean mean^T).  Truth: exact integers.  Bound:
    2 gamma_m sum |y_i y_j|, m = terms + 2; 2 gamma_m sum |y|, m = terms + 1, for the plain sum."""
    x = _ar1_trace(nslots, dim, nchains, nslots + dim)
    npad = (nchains + 63) // 64 * 64
    trace = _nan_trace(x, npad, dim + 5)
    mean = x.mean(axis=(0, 2))
    for centre in (None, mean, mean + 1e8):
        total, sumsq = _device_moments(gpu, trace, nslots, dim, dim + 5, nchains, npad, centre)
        assert np.array_equal(sumsq, sumsq.T)
        worst = R.check_rounding_bound(total, sumsq, R.entries_of(x), centre, "centre=%s" % (None if centre is None else centre[0]))
        print("nslots=%d nchains=%d dim=%d centre=%s: worst |error| / bound = %.3g"
              % (nslots, nchains, dim, "none" if centre is None else "%.6g" % centre[0], worst))


def test_device_moments_give_the_same_bits_twice(gpu):
    for nslots, nchains, dim in ((40, 300, 50), (9, 130, 100)):
        x = _ar1_trace(nslots, dim, nchains, 3)
        npad = (nchains + 63) // 64 * 64
        trace = _nan_trace(x, npad, dim)
        a = _device_moments(gpu, trace, nslots, dim, dim, nchains, npad, x.mean(axis=(0, 2)))
        b = _device_moments(gpu, trace, nslots, dim, dim, nchains, npad, x.mean(axis=(0, 2)))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.all(np.isfinite(a[1]))


def _check_engine_trace(m, x, centre, tag):
    """m: the TraceMoments of the engine; x[slot][dim][chain] the copied-back trace.  The device sums are within the
    rounding bound of the exact sums; about the origin, the macro's own point, so is the macro restatement on the same
    entries (it sums in another order), so the two agree to within two bounds."""
    entries = R.entries_of(x)
    worst = R.check_rounding_bound(m.sum, m.sumsq, entries, centre, tag)
    if centre is None:                   # the macro knows the origin only
        macro = R.make_covariance(entries)
        assert R.check_rounding_bound(macro["sum"], macro["sumsq"], entries, None, tag + " (macro)") <= 1.0
    assert m.n == entries.shape[0] and np.array_equal(m.sumsq, m.sumsq.T)
    print("%s: worst |error| / bound = %.3g" % (tag, worst))


@pytest.mark.parametrize("dim,nchains,steps,stride", [(5, 70, 64, 4), (50, 130, 48, 4), (100, 64, 6, 1)])
def test_engine_trace(gpu, dim, nchains, steps, stride):
    import torch
    # D > 63 saves a trace with a frozen covariance only
    e = gpu.Engine(dim, nchains, seed=9, mode=gpu.MODE_FROZEN if dim > 63 else gpu.MODE_POOLED)
    assert e.Start(np.zeros(dim))
    e.Step(200)
    slots = steps // stride
    sx = torch.full((slots, e.dim_padded, e.nchains_padded), float("nan"), dtype=torch.float64, device="cuda")
    sl = torch.empty((slots, e.nchains_padded), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    e.StepSave(steps, sx.data_ptr(), sl.data_ptr(), stride=stride)
    torch.cuda.synchronize()
    x = sx[:, :dim, :nchains].cpu().numpy()
    centre = e.GetEstimatedCenter()
    _check_engine_trace(e.TraceMoments(sx.data_ptr(), slots, centre=centre), x, centre, "Engine D=%d about its centre" % dim)
    _check_engine_trace(e.TraceMoments(sx.data_ptr(), slots), x, None, "Engine D=%d about the origin" % dim)


def test_hmc_engine_trace(gpu):
    import torch
    dim, nchains, slots = 7, 130, 12
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
    _check_engine_trace(h.TraceMoments(trace.data_ptr(), slots), trace[:, :, :nchains].cpu().numpy(), None, "HmcEngine")


def test_vaat_engine_trace(gpu):
    import torch
    dim, nchains, steps, stride = 6, 100, 80, 4
    e = gpu.VaatEngine(dim, nchains, seed=2)
    assert e.Start(np.zeros(dim))
    slots = steps // stride
    sx = torch.full((slots, dim, e.nchains_padded), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    e.step_save(steps, stride, sx.data_ptr())
    torch.cuda.synchronize()
    _check_engine_trace(e.TraceMoments(sx.data_ptr(), slots), sx[:, :, :nchains].cpu().numpy(), None, "VaatEngine")


def test_device_moments_reject_bad_arguments(gpu):
    import torch
    lib = gpu.load()
    trace = torch.zeros((4, 2, 64), dtype=torch.float64, device="cuda")
    t = C.c_void_p(trace.data_ptr())
    out = (C.c_double * 128)()
    sq = (C.c_double * 128)()
    assert lib.smcmc_trace_moments(t, 4, 2, 2, 64, 64, None, out, sq, None) == 0
    assert lib.smcmc_trace_moments(None, 4, 2, 2, 64, 64, None, out, sq, None) == INVALID   # null trace
    assert lib.smcmc_trace_moments(t, 0, 2, 2, 64, 64, None, out, sq, None) == INVALID      # nslots = 0
    assert lib.smcmc_trace_moments(t, 4, 2, 1, 64, 64, None, out, sq, None) == INVALID      # dim_stride < dim
    assert lib.smcmc_trace_moments(t, 4, 2, 2, 60, 60, None, out, sq, None) == INVALID      # not a multiple of 64
    assert lib.smcmc_trace_moments(t, 4, 2, 2, 65, 64, None, out, sq, None) == INVALID      # padded < nchains
    assert lib.smcmc_trace_moments(t, 4, 2, 2, 64, 64, None, None, sq, None) == INVALID     # null sum
    assert lib.smcmc_trace_moments(t, 4, 2, 2, 64, 64, None, out, None, None) == INVALID    # null sumsq
    assert lib.smcmc_trace_moments(t, 4, 0, 2, 64, 64, None, out, sq, None) == INVALID      # dim = 0
    assert lib.smcmc_trace_moments(t, 4, 2, 2, 0, 64, None, out, sq, None) == INVALID       # nchains = 0
    big = lib.smcmc_max_dim() + 1
    assert lib.smcmc_trace_moments(t, 4, big, big, 64, 64, None, out, sq, None) == INVALID  # dim > smcmc_max_dim()


# ---- the Cholesky chain ------------------------------------------------------------------------------------------------

def _device_chain(gpu, mean, cov, nslots, nchains, dim_stride, seed, chain_offset=0):
    """(status, trace[slot][dim_stride][padded] as numpy, U) of smcmc_cholesky_chain on a NaN-prefilled trace."""
    import torch
    dim = mean.size
    npad = (nchains + 63) // 64 * 64
    trace = torch.full((nslots, dim_stride, npad), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    U = np.full((dim, dim), np.nan)
    mean, cov = np.ascontiguousarray(mean, dtype=np.float64), np.ascontiguousarray(cov, dtype=np.float64)
    st = gpu.load().smcmc_cholesky_chain(mean.ctypes.data_as(DP), cov.ctypes.data_as(DP), dim, nslots, nchains, npad,
                                         dim_stride, seed, chain_offset, C.c_void_p(trace.data_ptr()), U.ctypes.data_as(DP), None)
    torch.cuda.synchronize()
    return st, trace.cpu().numpy(), U


@pytest.mark.parametrize("nchains", [1, 65, 130])
@pytest.mark.parametrize("dim,stride", [(1, 1), (5, 8), (50, 64), (64, 64), (65, 72), (100, 100)])
def test_cholesky_chain_is_the_restatement_bit_for_bit(gpu, oracle, dim, stride, nchains):
    nslots, seed = 3, 20240607 + dim
    cov = R.random_spd(dim, dim)
    mean = np.random.default_rng(dim).normal(size=dim) * 10.0
    want, want_u = R.cholesky_chain(oracle, mean, cov, nslots, nchains, seed)
    st, got, U = _device_chain(gpu, mean, cov, nslots, nchains, stride, seed)
    assert st == 0
    assert np.array_equal(U, want_u)
    assert np.array_equal(got[:, :dim, :nchains], want)
    assert np.all(np.isnan(got[:, dim:, :])) and np.all(np.isnan(got[:, :, nchains:]))   # the padding is not written


def test_cholesky_chain_offset_is_a_slice(gpu):
    dim = 50
    cov, mean = R.random_spd(dim, 1), np.arange(dim, dtype=np.float64)
    st, whole, _ = _device_chain(gpu, mean, cov, 3, 65, 64, 77)
    st2, part, _ = _device_chain(gpu, mean, cov, 3, 25, 64, 77, chain_offset=40)
    assert st == 0 and st2 == 0
    assert np.array_equal(part[:, :dim, :25], whole[:, :dim, 40:65])


def test_cholesky_chain_refuses_a_negative_pivot(gpu):
    cov = np.array([[4.0, 2.0, 0.0], [2.0, 0.5, 0.0], [0.0, 0.0, 1.0]])          # second pivot: 0.5 - 1 < 0
    st, trace, _ = _device_chain(gpu, np.zeros(3), cov, 2, 70, 4, 5)
    assert st == RUNTIME
    assert np.all(np.isnan(trace))                                                # untouched
    with pytest.raises(gpu.SmcmcError) as err:
        gpu.cholesky_chain(np.zeros(3), cov, 2, 70)
    assert err.value.status == RUNTIME


def test_cholesky_round_trip(gpu):
    """cholesky_chain, then TraceMoments about the input mean: the moments of N = 64 x 4 096 Gaussian draws within six
    standard errors (a fixed seed: not a flaky test)."""
    dim, nslots, nchains = 8, 64, 4096
    sigma = R.random_spd(dim, 11, 0.1, 10.0)
    mean = np.linspace(-5.0, 50.0, dim)
    trace, U = gpu.cholesky_chain(mean, sigma, nslots, nchains, seed=20240607)
    assert tuple(trace.shape) == (nslots, dim, nchains)
    assert np.allclose(U.T @ U, sigma, rtol=1e-12)
    total, sumsq = _device_moments(gpu, trace, nslots, dim, dim, nchains, nchains, mean)
    m = gpu.TraceMoments(total, sumsq, nslots, nchains, mean)
    R.gaussian_round_trip(m.mean, m.covariance, mean, sigma, nslots * nchains)
    # the same through an engine's method on a strided trace, and the other reducers take the trace as it is
    e = gpu.Engine(dim, nchains, seed=1)
    padded, _ = gpu.cholesky_chain(mean, sigma, nslots, nchains, seed=20240607, dim_stride=e.dim_padded)
    m2 = e.TraceMoments(padded.data_ptr(), nslots, centre=mean)
    assert np.array_equal(m2.sum, m.sum) and np.array_equal(m2.sumsq, m.sumsq)
    a = e.AutocorrelationSums(padded.data_ptr(), nslots, centre=mean)
    assert np.allclose(a.lagged[0], np.diag(m.sumsq), rtol=1e-12)
    assert np.all(np.abs(a.rho()[1:8]) < 6.0 / np.sqrt(nslots * nchains / 2.0))   # independent draws
