"""The device histograms of a saved trace (smcmc_trace_ranges, smcmc_marginal_histograms, the engines' Marginals) against
the numpy restatement of TestMarginalization.C in tests/marginal_ref.py.

Every comparison is np.array_equal on integer counts, and ranges are equal as doubles: no tolerance anywhere.  Both sides
evaluate the same three IEEE operations per value (a subtraction, a multiplication, a correctly rounded division) and the
rest is integer counting."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("smcmc_marginal_ref", os.path.join(HERE, "marginal_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

DP = C.POINTER(C.c_double)
UP = C.POINTER(C.c_uint64)
IP = C.POINTER(C.c_int32)
INVALID = 1                                                                      # SMCMC_ERR_INVALID
MAX_BINS1, MAX_BINS2, MAX_PAIR_DIMS = 1000, 126, 32                              # SMCMC_MARGINAL_MAX_* of include/smcmc.h


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _trace(x, nchains_padded, dim_stride):
    """x[slot][dim][chain] in a device trace [slot][dim_stride][nchains_padded] whose padding lanes and rows are NaN."""
    import torch
    nslots, dim, nchains = x.shape
    trace = torch.full((nslots, dim_stride, nchains_padded), float("nan"), dtype=torch.float64, device="cuda")
    trace[:, :dim, :nchains] = torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    torch.cuda.synchronize()
    return trace


def _ranges(gpu, trace, shape, sample_stride):
    nslots, dim, nchains = shape
    lo, hi = np.full(dim, 123.0), np.full(dim, 123.0)
    st = gpu.load().smcmc_trace_ranges(C.c_void_p(trace.data_ptr()), nslots, dim, trace.shape[1], nchains, trace.shape[2],
                                       sample_stride, lo.ctypes.data_as(DP), hi.ctypes.data_as(DP), None)
    assert st == 0, st
    return lo, hi


def _hist(gpu, trace, shape, n1=0, lo1=None, hi1=None, dims=(), n2=0, lo2=None, hi2=None):
    """(counts1 or None, counts2 or None) of smcmc_marginal_histograms; the outputs start from a sentinel."""
    nslots, dim, nchains = shape
    P = len(dims)
    c1 = np.full((dim, n1 + 2), 77, dtype=np.uint64) if n1 else None
    c2 = np.full((P, P, n2 + 2, n2 + 2), 77, dtype=np.uint64) if P else None
    lo1, hi1 = (None, None) if not n1 else (_f(lo1), _f(hi1))
    lo2, hi2 = (None, None) if not P else (_f(lo2), _f(hi2))
    pd = np.ascontiguousarray(dims, dtype=np.int32)
    st = gpu.load().smcmc_marginal_histograms(
        C.c_void_p(trace.data_ptr()), nslots, dim, trace.shape[1], nchains, trace.shape[2],
        n1, lo1.ctypes.data_as(DP) if n1 else None, hi1.ctypes.data_as(DP) if n1 else None,
        c1.ctypes.data_as(UP) if n1 else None,
        P, pd.ctypes.data_as(IP) if P else None, n2, lo2.ctypes.data_as(DP) if P else None,
        hi2.ctypes.data_as(DP) if P else None, c2.ctypes.data_as(UP) if P else None, None)
    assert st == 0, st
    return c1, c2


# ---- synthetic traces through the bare C entry --------------------------------------------------------------------------

SLOTS = [1, 2, 15, 16, 17, 63, 64, 65, 100]
STRIDES = [1, 2, 7, 1000]                                                          # the last is larger than any nslots here
KINDS = ["normal", "integers", "identical", "specials"]


def _data(kind, rng, shape):
    """(x, lo[dim], hi[dim]): a trace of the kind and axes that leave some of it outside."""
    nslots, dim, nchains = shape
    if kind == "normal":
        x = rng.normal(size=shape) * rng.uniform(0.5, 3.0, size=(1, dim, 1)) + rng.normal(size=(1, dim, 1))
        lo = rng.uniform(-3.0, -1.0, size=dim)
        hi = rng.uniform(1.0, 3.0, size=dim)
    elif kind == "integers":                     # many values exactly on bin edges, on lo and on hi
        x = rng.integers(-2, 13, size=shape).astype(np.float64)
        lo, hi = np.zeros(dim), np.full(dim, 10.0)
    elif kind == "identical":                    # one bin takes everything: the contention worst case
        x = np.full(shape, 1.25)
        lo, hi = np.zeros(dim), np.full(dim, 2.0)
    else:                                        # live lanes holding NaN, +-inf and values far outside the axis
        x = rng.normal(size=shape)
        special = np.array([np.nan, np.inf, -np.inf, 1e300, -1e300, 5e-324, -0.0])
        mask = rng.random(size=shape) < 0.2
        x[mask] = rng.choice(special, size=int(mask.sum()))
        x[0, :, 0] = np.nan                      # the first entry too (the macro starts its ranges from it)
        lo, hi = np.full(dim, -1.5), np.full(dim, 1.5)
    return x, lo, hi


@pytest.mark.parametrize("nchains,extra_blocks", [(1, 0), (63, 0), (64, 0), (65, 0), (200, 0), (1, 1), (64, 2), (65, 2), (200, 1)])
def test_synthetic_traces_match_the_restatement(gpu, nchains, extra_blocks):
    """Chain counts around the wavefront and the 256-chain workgroup, with and without whole padded blocks; slot counts
    around the register blocks of the kernels; dim_stride > dim; NaN in every padding lane and row.  The bins (1, 2, 100,
    the 1-D maximum; 1, 2, 50, the 2-D maximum), the pair lists (1, 2 and 10 positions, out of order, with a repeated
    dimension) and the sample strides rotate through the cases so that each meets every kind of data."""
    rng = np.random.default_rng(1000 * nchains + extra_blocks)
    npad = (nchains + 63) // 64 * 64 + 64 * extra_blocks
    bins1 = [1, 2, 100, MAX_BINS1]
    bins2 = [1, 2, 50, MAX_BINS2]
    case = 0
    for nslots in SLOTS:
        for kind in KINDS:
            dim, dim_stride = [(1, 1), (3, 3), (2, 5), (12, 13)][case % 4]
            shape = (nslots, dim, nchains)
            x, lo, hi = _data(kind, rng, shape)
            trace = _trace(x, npad, dim_stride)
            tag = "case %d: %s nslots=%d nchains=%d/%d dim=%d/%d" % (case, kind, nslots, nchains, npad, dim, dim_stride)
            # ranges
            for stride in (STRIDES[case % 4], STRIDES[(case // 4 + 1) % 4]):
                got_lo, got_hi = _ranges(gpu, trace, shape, stride)
                want_lo, want_hi = R.ranges(x, stride)
                assert np.array_equal(got_lo, want_lo) and np.array_equal(got_hi, want_hi), (tag, stride, got_lo, want_lo)
            # 1-D alone, pairs alone, both in one call
            n1 = bins1[(case + case // 4) % 4]
            n2 = bins2[(case + case // 8) % 4]
            if dim >= 10:
                dims = [7, 0, 11, 3, 3, 9, 1, 10, 2, 5]            # 10 positions, out of order, dimension 3 twice
            else:
                dims = [[0], [dim - 1, 0], [0, 0]][(case // 4) % 3]
            if n2 == MAX_BINS2:
                dims = dims[:3]                                     # 128 x 128 tables: keep the result a few MB
            lo2, hi2 = lo[dims] - 0.25, hi[dims] + 0.125
            want1 = R.hist1(x, n1, lo, hi)
            want2 = R.hist2(x, dims, n2, lo2, hi2)
            c1, none = _hist(gpu, trace, shape, n1, lo, hi)
            assert none is None and np.array_equal(c1, want1), (tag, n1)
            none, c2 = _hist(gpu, trace, shape, dims=dims, n2=n2, lo2=lo2, hi2=hi2)
            assert none is None and np.array_equal(c2, want2), (tag, dims, n2)
            c1, c2 = _hist(gpu, trace, shape, n1, lo, hi, dims, n2, lo2, hi2)
            assert np.array_equal(c1, want1) and np.array_equal(c2, want2), (tag, "both")
            if kind == "identical":
                assert c1[:, 1 + int(n1 * 1.25 / 2.0)].tolist() == [nslots * nchains] * dim, tag
            case += 1


def test_a_quotient_that_rounds_up_to_n_is_counted_as_overflow(gpu):
    """Axes whose largest double below hi has n (x - lo) / (hi - lo) == n (about one random axis in five at n = 100):
    the formula sends it to counter n + 1, and so does the device."""
    rng = np.random.default_rng(5)
    dim, met = 64, 0
    lo = rng.normal(size=dim) * 10.0
    hi = lo + rng.uniform(0.1, 20.0, size=dim)
    below = np.nextafter(hi, -np.inf)
    x = np.stack([below, np.nextafter(below, -np.inf), lo, np.nextafter(lo, -np.inf), hi])[:, :, None] * np.ones((1, 1, 3))
    want = R.hist1(x, 100, lo, hi)
    met = int((want[:, 101] > 3).sum())
    assert 0 < met < dim                                            # the case is met, and not on every axis
    c1, _ = _hist(gpu, _trace(x, 64, dim), x.shape, 100, lo, hi)
    assert np.array_equal(c1, want)


# ---- invariants that do not lean on the restatement -------------------------------------------------------------------

def test_invariants_of_the_counts(gpu):
    rng = np.random.default_rng(77)
    nslots, dim, nchains = 37, 6, 333
    x = rng.normal(size=(nslots, dim, nchains)) * np.arange(1, dim + 1)[None, :, None]
    x[rng.random(size=x.shape) < 0.01] = np.nan
    shape = x.shape
    trace = _trace(x, 384, dim + 2)
    lo, hi = _ranges(gpu, trace, shape, 1)
    dims = [4, 1, 5, 1]
    n1, n2 = 40, 40
    lo2, hi2 = lo[dims], hi[dims]                                   # the same axes as the 1-D histograms of these dimensions
    c1, c2 = _hist(gpu, trace, shape, n1, lo, hi, dims, n2, lo2, hi2)
    total = nslots * nchains
    assert np.all(c1.sum(axis=1) == total)                          # every point is counted once, NaN as overflow
    assert np.all(c2.sum(axis=(2, 3)) == total)
    for p in range(len(dims)):
        for q in range(len(dims)):
            assert np.array_equal(c2[q, p], c2[p, q].T)
        assert np.count_nonzero(c2[p, p] - np.diag(np.diag(c2[p, p]))) == 0
        assert np.array_equal(np.diag(c2[p, p]), c1[dims[p]])
    assert np.array_equal(c2[1, 3], c2[1, 1]) and np.array_equal(c2[0, 3], c2[0, 1])     # a repeated dimension
    again1, again2 = _hist(gpu, trace, shape, n1, lo, hi, dims, n2, lo2, hi2)
    assert np.array_equal(again1, c1) and np.array_equal(again2, c2)                     # integer adds commute
    # two ranks with half of the chains each: their ranges merge to the whole's, their counts on common axes add up
    h = 150
    halves = [(x[:, :, :h], 192), (x[:, :, h:], 256)]
    parts, rngs = [], []
    for xh, npad in halves:
        t = _trace(xh, npad, dim)
        rngs.append(_ranges(gpu, t, xh.shape, 1))
        parts.append((t, xh.shape))
    mlo, mhi = gpu.Marginals.merge_ranges(rngs)
    assert np.array_equal(mlo, lo) and np.array_equal(mhi, hi)
    ms = []
    for t, shp in parts:
        a1, a2 = _hist(gpu, t, shp, n1, mlo, mhi, dims, n2, mlo[dims], mhi[dims])
        ms.append(gpu.Marginals(mlo, mhi, nslots, shp[2], mlo, mhi, a1, dims, mlo[dims], mhi[dims], a2))
    whole = ms[0] + ms[1]
    assert whole.nchains == nchains and whole.counts1.dtype == np.uint64
    assert np.array_equal(whole.counts1, c1) and np.array_equal(whole.counts2, c2)


# ---- traces the engines wrote, through their Marginals methods ----------------------------------------------------------

def _check_against_macro(m, x, tag):
    ref = R.macro(x)
    assert np.array_equal(m.lo, ref["lo"]) and np.array_equal(m.hi, ref["hi"]), tag
    assert m.macro_ranges()[0] == ref["abs"], tag
    assert np.all(m.lo1 == ref["abs"][0]) and np.all(m.hi1 == ref["abs"][1]), tag
    assert np.array_equal(m.pair_dims, ref["dims"]), tag
    assert np.array_equal(m.lo2, ref["lo2"]) and np.array_equal(m.hi2, ref["hi2"]), tag
    assert m.counts1.shape == ref["counts1"].shape and m.counts2.shape == ref["counts2"].shape, tag
    assert np.array_equal(m.counts1, ref["counts1"]), tag
    assert np.array_equal(m.counts2, ref["counts2"]), tag
    assert np.all(m.counts1.sum(axis=1) == x.shape[0] * x.shape[2]), tag
    assert np.count_nonzero(m.counts1[:, 1:-1]) > 1, tag                               # the chains moved
    lo68, hi68 = m.interval(0, 0.68)
    assert m.lo1[0] <= lo68 <= m.quantile(0, 0.5) <= hi68 <= m.hi1[0], tag


@pytest.mark.parametrize("dim,nchains,steps,stride", [(5, 70, 640, 4), (50, 256, 512, 8), (100, 64, 80, 1)])
def test_metropolis_engine_trace(gpu, dim, nchains, steps, stride):
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
    m = e.Marginals(sx.data_ptr(), slots)
    x = sx[:, :dim, :nchains].cpu().numpy()
    _check_against_macro(m, x, "Engine D=%d" % dim)
    assert (m.nslots, m.nchains, m.n1, m.n2) == (slots, nchains, 100, 50)
    # given ranges skip the range pass; other bins and another list of pair dimensions
    wide = (m.lo - 1.0, m.hi + 1.0)
    dims = [dim - 1, 0]
    g = e.Marginals(sx.data_ptr(), slots, n1=256, n2=7, pair_dims=dims, ranges=wide)
    (amin, amax), (lo2, hi2) = R.macro_axes(wide[0], wide[1], dims)
    assert np.array_equal(g.counts1, R.hist1(x, 256, np.full(dim, amin), np.full(dim, amax)))
    assert np.array_equal(g.counts2, R.hist2(x, dims, 7, lo2, hi2))
    assert g.counts1[:, 0].sum() == 0 and g.counts1[:, -1].sum() == 0                  # nothing outside the widened axis
    # a sample stride of the caller's
    s3 = e.Marginals(sx.data_ptr(), slots, sample_stride=3)
    want_lo, want_hi = R.ranges(x, 3)
    assert np.array_equal(s3.lo, want_lo) and np.array_equal(s3.hi, want_hi)


def test_hmc_engine_trace(gpu):
    import torch
    dim, nchains, slots = 7, 130, 40
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
    m = h.Marginals(trace.data_ptr(), slots)
    _check_against_macro(m, trace[:, :, :nchains].cpu().numpy(), "HmcEngine")


def test_vaat_engine_trace(gpu):
    import torch
    dim, nchains, steps, stride = 6, 100, 240, 4
    e = gpu.VaatEngine(dim, nchains, seed=2)
    assert e.Start(np.zeros(dim))
    slots = steps // stride
    sx = torch.full((slots, dim, e.nchains_padded), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    e.step_save(steps, stride, sx.data_ptr())
    torch.cuda.synchronize()
    m = e.Marginals(sx.data_ptr(), slots)
    _check_against_macro(m, sx[:, :, :nchains].cpu().numpy(), "VaatEngine")


def test_an_infinite_range_is_refused_by_the_fill(gpu):
    """The range pass returns an infinite end when the trace holds one; Engine.Marginals then gets the refusal from the fill."""
    import torch
    e = gpu.Engine(3, 64, seed=1)
    sx = torch.zeros((4, e.dim_padded, e.nchains_padded), dtype=torch.float64, device="cuda")
    sx[:, :3, :64] = torch.randn((4, 3, 64), dtype=torch.float64, device="cuda")
    sx[2, 1, 5] = float("inf")
    torch.cuda.synchronize()
    with pytest.raises(gpu.SmcmcError) as err:
        e.Marginals(sx.data_ptr(), 4)
    assert err.value.status == INVALID


# ---- argument checks -------------------------------------------------------------------------------------------------

def test_every_argument_check_refuses_and_leaves_the_outputs_untouched(gpu):
    import torch
    lib = gpu.load()
    trace = torch.zeros((4, 3, 64), dtype=torch.float64, device="cuda")
    t = C.c_void_p(trace.data_ptr())
    lo, hi = np.full(3, 5.0), np.full(3, 6.0)
    plo, phi = lo.ctypes.data_as(DP), hi.ctypes.data_as(DP)

    def ranges(*a):
        return lib.smcmc_trace_ranges(*a)
    assert ranges(t, 4, 3, 3, 64, 64, 1, plo, phi, None) == 0
    assert lo.tolist() == [0.0] * 3 and hi.tolist() == [0.0] * 3
    lo[:], hi[:] = 5.0, 6.0
    for bad in [(None, 4, 3, 3, 64, 64, 1, plo, phi, None),            # null trace
                (t, 0, 3, 3, 64, 64, 1, plo, phi, None),               # nslots = 0
                (t, 4, 0, 3, 64, 64, 1, plo, phi, None),               # dim = 0
                (t, 4, 3, 2, 64, 64, 1, plo, phi, None),               # dim_stride < dim
                (t, 4, 3, 3, 0, 64, 1, plo, phi, None),                # nchains = 0
                (t, 4, 3, 3, 60, 60, 1, plo, phi, None),               # not a multiple of 64
                (t, 4, 3, 3, 65, 64, 1, plo, phi, None),               # padded < nchains
                (t, 4, 3, 3, 64, 64, 0, plo, phi, None),               # sample_stride < 1
                (t, 4, 3, 3, 64, 64, -2, plo, phi, None),
                (t, 4, 3, 3, 64, 64, 1, None, phi, None),              # null lo
                (t, 4, 3, 3, 64, 64, 1, plo, None, None)]:             # null hi
        assert ranges(*bad) == INVALID, bad
    assert lo.tolist() == [5.0] * 3 and hi.tolist() == [6.0] * 3

    n1, n2 = 4, 3
    lo1, hi1 = np.full(3, -1.0), np.full(3, 1.0)
    dims = np.array([2, 0], dtype=np.int32)
    lo2, hi2 = np.full(2, -1.0), np.full(2, 1.0)
    c1 = np.full((3, MAX_BINS1 + 3), 9, dtype=np.uint64)              # room for every refused size
    c2 = np.full(2 * 2 * (MAX_BINS2 + 3) ** 2, 9, dtype=np.uint64)
    good = dict(trace=t, nslots=4, dim=3, dim_stride=3, nchains=64, npad=64, n1=n1, lo1=lo1, hi1=hi1, c1=c1, P=2, dims=dims,
                n2=n2, lo2=lo2, hi2=hi2, c2=c2)

    def hist(**change):
        a = dict(good, **change)
        def d(v): return None if v is None else v.ctypes.data_as(DP)
        return lib.smcmc_marginal_histograms(
            a["trace"], a["nslots"], a["dim"], a["dim_stride"], a["nchains"], a["npad"], a["n1"], d(a["lo1"]), d(a["hi1"]),
            None if a["c1"] is None else a["c1"].ctypes.data_as(UP), a["P"],
            None if a["dims"] is None else a["dims"].ctypes.data_as(IP), a["n2"], d(a["lo2"]), d(a["hi2"]),
            None if a["c2"] is None else a["c2"].ctypes.data_as(UP), None)
    nan, inf = np.nan, np.inf
    refused = [dict(trace=None), dict(nslots=0), dict(dim=0), dict(dim_stride=2), dict(nchains=0), dict(nchains=60, npad=60),
               dict(nchains=65), dict(n1=-1), dict(n1=MAX_BINS1 + 1), dict(lo1=None), dict(hi1=None),
               dict(hi1=np.array([1.0, -1.0, 1.0])),                    # an empty axis: lo == hi
               dict(hi1=np.array([1.0, -2.0, 1.0])),                    # lo > hi
               dict(lo1=np.array([-1.0, nan, -1.0])), dict(hi1=np.array([1.0, 1.0, inf])), dict(lo1=np.array([-inf, -1.0, -1.0])),
               dict(P=-1), dict(P=MAX_PAIR_DIMS + 1), dict(dims=None), dict(dims=np.array([2, 3], dtype=np.int32)),
               dict(dims=np.array([-1, 0], dtype=np.int32)), dict(n2=0), dict(n2=-3), dict(n2=MAX_BINS2 + 1),
               dict(lo2=None), dict(hi2=None), dict(c2=None), dict(hi2=np.array([1.0, -1.0])), dict(lo2=np.array([nan, -1.0])),
               dict(hi2=np.array([inf, 1.0])),
               dict(n1=0, P=0), dict(c1=None, P=0)]                     # nothing asked for
    for change in refused:
        assert hist(**change) == INVALID, change
        assert np.all(c1 == 9) and np.all(c2 == 9), change
    # the same call with nothing wrong, and its two halves
    assert hist() == 0
    got1 = c1.ravel()[:3 * (n1 + 2)].reshape(3, n1 + 2)
    got2 = c2[:2 * 2 * (n2 + 2) ** 2].reshape(2, 2, n2 + 2, n2 + 2)
    assert np.all(got1[:, 1 + 2] == 4 * 64) and got1.sum() == 3 * 4 * 64              # zeros: bin 1 + (int)(4 * 1 / 2)
    assert np.all(got2[:, :, 2, 2] == 4 * 64) and got2.sum() == 4 * 4 * 64            # bin 1 + (int)(3 * 1 / 2)
    assert np.all(c1.ravel()[3 * (n1 + 2):] == 9) and np.all(c2[2 * 2 * (n2 + 2) ** 2:] == 9)
    c1[:], c2[:] = 9, 9
    assert hist(n1=0) == 0 and np.all(c1 == 9) and c2[:100].sum() == 4 * 4 * 64        # the 1-D part skipped
    c2[:] = 9
    assert hist(c1=None) == 0 and c2[:100].sum() == 4 * 4 * 64                         # the same, by a null counts1
    c2[:] = 9
    assert hist(P=0) == 0 and np.all(c2 == 9) and c1.ravel()[:18].sum() == 3 * 4 * 64  # the pair part skipped
    # the limits themselves are served
    big = np.zeros((3, MAX_BINS1 + 2), dtype=np.uint64)
    assert hist(n1=MAX_BINS1, c1=big, P=0) == 0 and np.all(big.sum(axis=1) == 4 * 64)
