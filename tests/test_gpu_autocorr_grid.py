"""The device sums of a saved trace on a lag grid (smcmc_autocorrelation_grid_sums) and the macro built on them
(MakeAutocorrelation) against the exact sums and the restatement of tests/autocorr_grid_ref.py."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("smcmc_autocorr_grid_ref", os.path.join(HERE, "autocorr_grid_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

DP = C.POINTER(C.c_double)
INVALID = 1                                                      # SMCMC_ERR_INVALID


def _nan_trace(x, nchains_padded, dim_stride):
    """x[slot][dim][chain] in a device trace [slot][dim_stride][nchains_padded] whose padding lanes and rows >= dim
    are NaN."""
    import torch
    nslots, dim, nchains = x.shape
    trace = torch.full((nslots, dim_stride, nchains_padded), float("nan"), dtype=torch.float64, device="cuda")
    trace[:, :dim, :nchains] = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to("cuda")
    torch.cuda.synchronize()
    return trace


def _grid(gpu, trace, nslots, dim, dim_stride, nchains, nchains_padded, centre, grid):
    """(sum[dim], sumsq[dim], lagged[nlags][dim]) of the C entry; the outputs are prefilled with NaN."""
    lag_first, lag_step, nlags = grid
    total, sumsq, lagged = np.full(dim, np.nan), np.full(dim, np.nan), np.full((nlags, dim), np.nan)
    c = None if centre is None else np.ascontiguousarray(centre, dtype=np.float64)
    st = gpu.load().smcmc_autocorrelation_grid_sums(C.c_void_p(trace.data_ptr()), nslots, dim, dim_stride, nchains,
                                                    nchains_padded, None if c is None else c.ctypes.data_as(DP), lag_first,
                                                    lag_step, nlags, total.ctypes.data_as(DP), sumsq.ctypes.data_as(DP),
                                                    lagged.ctypes.data_as(DP), None)
    assert st == 0, (st, grid)
    return total, sumsq, lagged


def _contiguous(gpu, trace, nslots, dim, dim_stride, nchains, nchains_padded, centre):
    """(sum[dim], lagged[64][dim]) of smcmc_autocorrelation_sums."""
    total, lagged = np.full(dim, np.nan), np.full((64, dim), np.nan)
    c = None if centre is None else np.ascontiguousarray(centre, dtype=np.float64)
    st = gpu.load().smcmc_autocorrelation_sums(C.c_void_p(trace.data_ptr()), nslots, dim, dim_stride, nchains, nchains_padded,
                                               None if c is None else c.ctypes.data_as(DP), total.ctypes.data_as(DP),
                                               lagged.ctypes.data_as(DP), None)
    assert st == 0, st
    return total, lagged


SLOTS = [1, 2, 15, 16, 17, 33, 48, 65, 100]
# steps below and above the 16-slot block and the 32-wide window, grids that end beyond the trace, one that starts beyond it
GRIDS = [(0, 1, 64), (1, 1, 33), (1, 2, 32), (0, 3, 65), (5, 7, 31), (1, 17, 10), (2, 40, 4), (63, 1, 1), (0, 100, 2), (200, 5, 3)]


@pytest.mark.parametrize("nchains,extra_blocks", [(1, 0), (63, 0), (65, 0), (200, 0), (65, 2)])
def test_device_sums_are_exact_on_integers(gpu, nchains, extra_blocks):
    """Integer data in [-1024, 1024] about an integer centre in the same range: |y| <= 2048, every product and every
    partial sum is an integer below 2^53 (at most 100 * 200 * 2048^2 < 2^37: int64 holds the truth, a double every
    partial sum), so every summation order gives the same double and the tolerance is zero.  Rows whose lag lies
    beyond the trace are exactly 0.  9 nslots x 2 layouts x 10 grids x 2 centres = 360 calls per parameter."""
    rng = np.random.default_rng(nchains + extra_blocks)
    npad = (nchains + 63) // 64 * 64 + 64 * extra_blocks
    for nslots in SLOTS:
        for dim, stride in ((1, 1), (3, 8)):
            x = rng.integers(-1024, 1025, size=(nslots, dim, nchains))
            centre = rng.integers(-1024, 1025, size=dim)
            trace = _nan_trace(x, npad, stride)
            for c in (None, centre):
                y = x - (0 if c is None else c[None, :, None])
                for grid in GRIDS:
                    lags = R.grid_lags(*grid)
                    total, sumsq, lagged = R.integer_grid_sums(y, lags)
                    got = _grid(gpu, trace, nslots, dim, stride, nchains, npad, None if c is None else c.astype(np.float64), grid)
                    tag = "nslots=%d nchains=%d/%d dim=%d/%d centre=%s grid=%s" % (nslots, nchains, npad, dim, stride, c is not None, grid)
                    assert np.array_equal(got[0], total.astype(np.float64)), tag
                    assert np.array_equal(got[1], sumsq.astype(np.float64)), tag
                    assert np.array_equal(got[2], lagged.astype(np.float64)), tag
                    beyond = np.array(lags) >= nslots
                    assert np.all(got[2][beyond] == 0.0) and not np.any(np.signbit(got[2][beyond])), tag


def _ar1_trace(nslots, dim, nchains, seed):
    rng = np.random.default_rng(seed)
    x = np.zeros((nslots, dim, nchains))
    x[0] = rng.standard_normal((dim, nchains))
    for t in range(1, nslots):
        x[t] = 0.9 * x[t - 1] + rng.standard_normal((dim, nchains))
    return x + np.linspace(3.0, -40.0, dim)[None, :, None]


@pytest.mark.parametrize("nslots,nchains", [(100, 200), (33, 65)])
def test_device_sums_within_the_rounding_bound(gpu, nslots, nchains):
    """AR(1) data about no centre, the ensemble mean, and mean + 1e8 (y = x - c is one rounding of a difference of
    doubles; about the far centre every product is ~1e16 and nothing cancels here, it cancels later in a(lag)).  Truth:
    exact rationals.  Bound: tests/autocorr_grid_ref.py states it, 2 gamma_(terms+2) sum |y_t y_(t-k)| per row and
    2 gamma_(terms+1) sum |y| for the plain sum."""
    dim = 2
    x = _ar1_trace(nslots, dim, nchains, nslots)
    npad = (nchains + 63) // 64 * 64
    trace = _nan_trace(x, npad, dim + 5)
    mean = x.mean(axis=(0, 2))
    for centre in (None, mean, mean + 1e8):
        for grid in ((1, 3, 20), (1, 19, 5)):
            lags = R.grid_lags(*grid)
            exact = R.exact_grid_sums(x, centre, lags)
            got = _grid(gpu, trace, nslots, dim, dim + 5, nchains, npad, centre, grid)
            worst = R.check_rounding_bound(*got, exact, lags, nslots, nchains, "grid=%s" % (grid,))
            print("nslots=%d nchains=%d centre=%s grid=%s: worst |error| / bound = %.3g"
                  % (nslots, nchains, "none" if centre is None else "%.6g" % centre[0], grid, worst))


def _engine_trace(gpu, dim, nchains, slots, seed=9):
    import torch
    e = gpu.Engine(dim, nchains, seed=seed, mode=gpu.MODE_POOLED)
    assert e.Start(np.zeros(dim))
    e.Step(300)
    sx = torch.full((slots, e.dim_padded, e.nchains_padded), float("nan"), dtype=torch.float64, device="cuda")
    sl = torch.empty((slots, e.nchains_padded), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    e.StepSave(slots, sx.data_ptr(), sl.data_ptr(), stride=1)
    torch.cuda.synchronize()
    return e, sx


def test_step_one_has_the_bits_of_the_contiguous_reducer(gpu):
    """Grid (0, 1, 64) against smcmc_autocorrelation_sums: the same fused multiply-adds in the same order, so the same
    bits in `lagged` and `sum` -- on a StepSave trace and on an AR(1) tensor with a last block of one live lane."""
    e, sx = _engine_trace(gpu, 5, 70, 160)
    centre = e.GetEstimatedCenter()
    shapes = [(sx, 160, 5, e.dim_padded, 70, e.nchains_padded, centre)]
    x = _ar1_trace(33, 3, 65, 7)
    shapes.append((_nan_trace(x, 128, 8), 33, 3, 8, 65, 128, x.mean(axis=(0, 2))))
    for trace, nslots, dim, stride, nchains, npad, c in shapes:
        for centre in (None, c):
            total, sumsq, lagged = _grid(gpu, trace, nslots, dim, stride, nchains, npad, centre, (0, 1, 64))
            want_total, want_lagged = _contiguous(gpu, trace, nslots, dim, stride, nchains, npad, centre)
            assert np.all(np.isfinite(lagged)) and np.any(lagged != 0.0)
            assert np.array_equal(lagged, want_lagged)
            assert np.array_equal(total, want_total)
            assert np.array_equal(sumsq, want_lagged[0])              # lag 0 is the same chain of fused multiply-adds


def test_a_row_depends_on_its_lag_and_the_step_only(gpu):
    """Grid (1, 7, 40) against its rows fetched in other calls: (1, 7, 13) the first 13, (92, 7, 27) the rest, and
    (141, 7, 1) row 20 on its own.  The same bits; so has a second identical call."""
    nslots, nchains, dim = 300, 65, 2
    x = _ar1_trace(nslots, dim, nchains, 3)
    trace = _nan_trace(x, 128, dim)
    centre = x.mean(axis=(0, 2))
    args = (gpu, trace, nslots, dim, dim, nchains, 128, centre)
    total, sumsq, lagged = _grid(*args, (1, 7, 40))
    assert np.all(np.isfinite(lagged)) and np.all(lagged != 0.0)
    again = _grid(*args, (1, 7, 40))
    for a, b in zip((total, sumsq, lagged), again):
        assert np.array_equal(a, b)
    head, tail, one = _grid(*args, (1, 7, 13)), _grid(*args, (92, 7, 27)), _grid(*args, (141, 7, 1))
    assert np.array_equal(head[2], lagged[:13])
    assert np.array_equal(tail[2], lagged[13:])
    assert np.array_equal(one[2][0], lagged[20])
    for other in (head, tail, one):                                   # sum and sumsq do not depend on the grid's ends
        assert np.array_equal(other[0], total) and np.array_equal(other[1], sumsq)


def test_make_autocorrelation_end_to_end(gpu):
    """Engine(5, 70), 640 saved steps: MakeAutocorrelation (plan, pointer offset, device sums, bins) against
    MacroAutocorrelation.from_sums fed the exact rational sums of the copied-back trace, about the engine's estimated
    centre.  The device sums are held to their rounding bound, the binned autocorrelation to 1e-12."""
    slots = 640
    e, sx = _engine_trace(gpu, 5, 70, slots)
    centre = e.GetEstimatedCenter()
    m = e.MakeAutocorrelation(sx.data_ptr(), slots, centre=centre)
    p = gpu.autocorrelation_plan(slots)
    assert (p.max_lag, p.bins, p.lag_step, p.trials, len(p.lags)) == (614, 100, 3, 640, 205)
    assert m.plan == p and m.nchains == 70
    x = sx[:, :5, :70].cpu().numpy()
    lags = [int(k) for k in p.lags]
    exact = R.exact_grid_sums(x[slots - p.trials:], centre, lags)
    worst = R.check_rounding_bound(m.sum, m.sumsq, m.lagged, exact, lags, p.trials, 70, "MakeAutocorrelation")
    f = lambda a: np.array([float(v) for v in a.ravel()]).reshape(a.shape)   # noqa: E731
    want = gpu.MacroAutocorrelation.from_sums(p, f(exact["sum"]), f(exact["sumsq"]), f(exact["lagged"]), 70, centre)
    print("MakeAutocorrelation: worst |error| / bound = %.3g, max |autocorr - exact| = %.3g"
          % (worst, np.max(np.abs(m.autocorr - want.autocorr))))
    assert np.all(np.isfinite(want.autocorr))
    assert np.allclose(m.autocorr, want.autocorr, rtol=0, atol=1e-12)
    assert np.allclose(m.mean, x.mean(axis=(0, 2)), rtol=1e-12, atol=1e-14)
    assert np.allclose(m.average, want.autocorr.mean(axis=0), rtol=0, atol=1e-12) and m.spread.shape == (100,)
    # the grid method on the same lags gives the macro's rows
    g = e.AutocorrelationGrid(sx.data_ptr(), slots, lag_first=1, lag_step=p.lag_step, nlags=len(lags), centre=centre)
    assert np.array_equal(g.lagged, m.lagged) and np.array_equal(g.lags, p.lags)
    assert np.array_equal(g.counts, (slots - p.lags) * 70.0)
    # the macro's own origin, on a view of the trace that starts later
    tail = e.MakeAutocorrelation(sx[40:].data_ptr(), slots - 40)
    g2 = e.AutocorrelationGrid(sx[40:].data_ptr(), slots - 40, 1, tail.plan.lag_step, len(tail.plan.lags))
    assert np.array_equal(tail.lagged, g2.lagged) and np.all(np.isfinite(tail.autocorr))


def test_make_autocorrelation_reads_the_last_trials_slots(gpu):
    """A plan whose trials are fewer than the entries (the macro's own constants get there above a million entries):
    depth = 200 and precision = 0.25 give maxLag = 200, trials = 264 of 640, so the code under test offsets the pointer by
    376 slots.  Integer data: the sums of the last 264 slots exactly, and NaN in the slots before them changes nothing."""
    slots, dim, nchains = 640, 3, 65
    e = gpu.Engine(dim, nchains, seed=1)
    p = gpu.autocorrelation_plan(slots, depth=200, precision=0.25)
    assert (p.max_lag, p.bins, p.lag_step, p.trials, len(p.lags)) == (200, 100, 1, 264, 199)
    rng = np.random.default_rng(5)
    x = rng.integers(-1024, 1025, size=(slots, dim, nchains))
    centre = rng.integers(-1024, 1025, size=dim)
    y = x.astype(np.float64)
    y[:slots - p.trials] = np.nan
    lags = [int(k) for k in p.lags]
    total, sumsq, lagged = R.integer_grid_sums(x[slots - p.trials:] - centre[None, :, None], lags)
    for data in (x, y):
        trace = _nan_trace(data, e.nchains_padded, e.dim_padded)
        m = e.MakeAutocorrelation(trace.data_ptr(), slots, centre=centre.astype(np.float64), plan=p)
        assert m.plan == p
        assert np.array_equal(m.sum, total.astype(np.float64)) and np.array_equal(m.sumsq, sumsq.astype(np.float64))
        assert np.array_equal(m.lagged, lagged.astype(np.float64))
        assert np.all(np.isfinite(m.autocorr))
    assert np.allclose(m.mean, x[slots - p.trials:].mean(axis=(0, 2)), rtol=1e-13)
    with pytest.raises(ValueError):
        e.MakeAutocorrelation(trace.data_ptr(), slots - 1, plan=p)


def test_more_lags_than_one_call_takes_are_split(gpu):
    """600 lags of step 1 over a 700-slot trace: two calls behind AutocorrelationGrid, the rows of one grid."""
    e, sx = _engine_trace(gpu, 2, 64, 700, seed=3)
    g = e.AutocorrelationGrid(sx.data_ptr(), 700, lag_first=0, lag_step=1, nlags=600)
    assert g.lagged.shape == (600, 2) and np.all(np.isfinite(g.rho()))
    total, lagged = _contiguous(gpu, sx, 700, 2, e.dim_padded, 64, e.nchains_padded, None)
    assert np.array_equal(g.lagged[:64], lagged) and np.array_equal(g.sum, total)
    late = _grid(gpu, sx, 700, 2, e.dim_padded, 64, e.nchains_padded, None, (500, 1, 100))
    assert np.array_equal(g.lagged[500:], late[2])
    assert np.allclose(g.rho()[0], 1.0, rtol=1e-12)


def test_hmc_and_vaat_traces(gpu):
    import torch
    dim, nchains, slots = 5, 64, 64
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
    v = gpu.VaatEngine(7, 70, seed=2)
    assert v.Start(np.zeros(7))
    sx = torch.full((slots, 7, v.nchains_padded), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    v.step_save(slots * 4, 4, sx.data_ptr())
    torch.cuda.synchronize()
    for eng, ptr, d in ((h, trace.data_ptr(), dim), (v, sx.data_ptr(), 7)):
        g = eng.AutocorrelationGrid(ptr, slots, nlags=63)
        assert g.rho().shape == (63, d) and np.all(np.isfinite(g.rho()))
        m = eng.MakeAutocorrelation(ptr, slots)
        assert (m.plan.max_lag, m.plan.bins, m.plan.lag_step) == (56, 56, 1)
        assert m.autocorr.shape == (d, 56) and np.all(np.isnan(m.autocorr[:, 0])) and np.all(np.isfinite(m.autocorr[:, 1:]))
        assert np.array_equal(m.lagged, g.lagged[:55])
    # the contiguous reducer on the variable-at-a-time trace: the bits of the grid at step 1
    old = v.AutocorrelationSums(sx.data_ptr(), slots)
    same = v.AutocorrelationGrid(sx.data_ptr(), slots, lag_first=0, lag_step=1, nlags=64)
    assert np.array_equal(same.lagged, old.lagged) and np.array_equal(same.sum, old.sum)


def test_device_sums_reject_bad_arguments(gpu):
    import torch
    lib = gpu.load()
    trace = torch.zeros((8, 2, 64), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    t = C.c_void_p(trace.data_ptr())
    out, sq, lag = np.full(2, np.nan), np.full(2, np.nan), np.full((512, 2), np.nan)
    po, ps, pl = out.ctypes.data_as(DP), sq.ctypes.data_as(DP), lag.ctypes.data_as(DP)
    f = lib.smcmc_autocorrelation_grid_sums
    big = 2 ** 31 - 1
    #      trace nslots dim stride nchains padded centre first step nlags sum sumsq lagged stream
    bad = [(None, 8, 2, 2, 64, 64, None, 1, 1, 4, po, ps, pl, None),       # null trace
           (t, 0, 2, 2, 64, 64, None, 1, 1, 4, po, ps, pl, None),          # nslots = 0
           (t, 8, 0, 2, 64, 64, None, 1, 1, 4, po, ps, pl, None),          # dim = 0
           (t, 8, 2, 1, 64, 64, None, 1, 1, 4, po, ps, pl, None),          # dim_stride < dim
           (t, 8, 2, 2, 0, 64, None, 1, 1, 4, po, ps, pl, None),           # nchains = 0
           (t, 8, 2, 2, 65, 64, None, 1, 1, 4, po, ps, pl, None),          # padded < nchains
           (t, 8, 2, 2, 60, 60, None, 1, 1, 4, po, ps, pl, None),          # not a multiple of 64
           (t, 8, 2, 2, 64, 64, None, -1, 1, 4, po, ps, pl, None),         # lag_first < 0
           (t, 8, 2, 2, 64, 64, None, 1, 0, 4, po, ps, pl, None),          # lag_step < 1
           (t, 8, 2, 2, 64, 64, None, 1, -3, 4, po, ps, pl, None),
           (t, 8, 2, 2, 64, 64, None, 1, 1, 0, po, ps, pl, None),          # nlags < 1
           (t, 8, 2, 2, 64, 64, None, 1, 1, 513, po, ps, pl, None),        # nlags > SMCMC_AUTOCORR_GRID_MAX_LAGS
           (t, 8, 2, 2, 64, 64, None, big, 1, 2, po, ps, pl, None),        # the last lag overflows int
           (t, 8, 2, 2, 64, 64, None, 1, big // 2, 4, po, ps, pl, None),
           (t, 8, 2, 2, 64, 64, None, 1, 1, 4, None, ps, pl, None),        # null sum
           (t, 8, 2, 2, 64, 64, None, 1, 1, 4, po, None, pl, None),        # null sumsq
           (t, 8, 2, 2, 64, 64, None, 1, 1, 4, po, ps, None, None)]        # null lagged
    for args in bad:
        assert f(*args) == INVALID, args[1:10]
    assert np.all(np.isnan(out)) and np.all(np.isnan(sq)) and np.all(np.isnan(lag))
    assert f(t, 8, 2, 2, 64, 64, None, big - 1, 1, 2, po, ps, pl, None) == 0      # the last lag is INT_MAX: served
    assert np.all(out == 0.0) and np.all(sq == 0.0) and np.all(lag[:2] == 0.0) and np.all(np.isnan(lag[2:]))
    assert f(t, 8, 2, 2, 64, 64, None, 0, 1, 512, po, ps, pl, None) == 0          # and the most lags of one call
    assert np.all(lag == 0.0)
