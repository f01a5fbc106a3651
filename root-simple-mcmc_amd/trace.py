"""The reducers over a saved trace: what they return and the methods the engines share to call them.

A saved trace is [slot][dim_stride][nchains_padded] doubles on the device: Engine.StepSave writes dim_stride =
dim_padded rows per slot, HmcEngine.StepSave / copy_positions and VaatEngine.step_save write dim_stride = dim.  The
reducers of the HIP library (smcmc_autocorrelation_sums, smcmc_autocorrelation_grid_sums, smcmc_trace_ranges,
smcmc_marginal_histograms, smcmc_trace_moments, smcmc_trace_convergence; include/smcmc.h) take any of them.  The result
classes are host-side numpy over the raw sums and have nothing to do with any engine; `TraceReducers` gives an engine
class the six methods that call the library on a trace of its own layout.  `event_predictive` and its result,
`PosteriorPredictive`, are the seventh reducer (smcmc_event_predictive_sums): it needs a likelihood over a simulated event
sample besides the trace, so only Engine, the one engine that serves that family, has a method for it.  The order
statistics (smcmc_trace_order_statistics, smcmc_trace_digit_counts; `TraceQuantiles`) are selected values, not sums: the
mixin's OrderStatistics, Quantiles and DigitCounts, and order_statistics_combined for several ranks' shards.
`predictive_check` and its result, `PredictiveCheck`, are the posterior-predictive check of the buffer `event_predictive`
fills (smcmc_predictive_check): integer counts; `poisson_draw` is its Poisson variate on the host.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import SmcmcError

_dp = C.POINTER(C.c_double)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    return a.ctypes.data_as(_dp)


class TraceReducers:
    """The reducers over a saved trace as methods of an engine (Engine, HmcEngine, VaatEngine).  The engine class
    provides _lib, _check, dim, nchains, nchains_padded and one hook, `_trace_dim_stride`: the rows a slot of the traces
    it writes holds (dim_padded for Engine.StepSave, dim for HmcEngine.StepSave / copy_positions and
    VaatEngine.step_save).  Where a docstring says "a trace StepSave wrote", read the engine's own call."""

    def _trace_shape(self):
        return self.dim, self._trace_dim_stride, self.nchains, self.nchains_padded

    def AutocorrelationSums(self, trace_ptr, nslots, centre=None, stream=0):
        """Lagged-product sums of a trace StepSave wrote ([slot][dim_padded][nchains_padded] on the device), pooled
        over slots and chains about `centre` (default: the origin, as the macro has it): the inputs of the reference's
        autocorrelation (MakeAutocorrelation.C:108-148).  Returns an Autocorrelation."""
        c = _f64(np.zeros(self.dim) if centre is None else centre)
        s = np.zeros(self.dim)
        lagged = np.zeros((_capi.AUTOCORR_LAGS, self.dim))
        self._check(self._lib.smcmc_autocorrelation_sums(C.c_void_p(int(trace_ptr)), int(nslots), *self._trace_shape(),
                                                         _ptr(c), _ptr(s), _ptr(lagged), C.c_void_p(int(stream))))
        return Autocorrelation(s, lagged, int(nslots), self.nchains)

    def AutocorrelationGrid(self, trace_ptr, nslots, lag_first=1, lag_step=1, nlags=64, centre=None, stream=0):
        """The pooled sums of a trace StepSave wrote on the lags lag_first + i lag_step, i < nlags, taken on the device
        (smcmc_autocorrelation_grid_sums): as far back along the chain as the caller asks, where AutocorrelationSums
        stops at lag 63.  More than 512 lags are taken in several calls.  Returns an AutocorrelationGrid."""
        return _autocorrelation_grid(self._lib, self._check, trace_ptr, nslots, *self._trace_shape(), lag_first, lag_step,
                                     nlags, centre, stream)

    def MakeAutocorrelation(self, trace_ptr, nslots, stream=0, centre=None, plan=None):
        """MakeAutocorrelation.C over a trace StepSave wrote: the macro's plan for entries = nslots
        (autocorrelation_plan), the device sums over the last `trials` slots on its lag grid, its bins.  centre: the
        reference point of the sums (default: the origin, as the macro has it).  plan: another AutocorrelationPlan for
        entries = nslots, e.g. autocorrelation_plan(nslots, depth, bins, precision) with constants of the caller's own.
        Returns a MacroAutocorrelation."""
        return _make_autocorrelation(self._lib, self._check, trace_ptr, nslots, *self._trace_shape(), centre, stream, plan)

    def Marginals(self, trace_ptr, nslots, n1=100, n2=50, pair_dims=None, sample_stride=None, ranges=None, stream=0):
        """The histograms of TestMarginalization.C over a trace StepSave wrote, counted on the device: the ranges of the
        dimensions over every sample_stride-th slot (default: the macro's stride; skipped when `ranges` = (lo, hi) is
        given, e.g. the merged ranges of several ranks), then n1 bins over [absMin, absMax) for every dimension and
        n2 x n2 bins for every ordered pair of pair_dims (default: the first min(dim, 10) dimensions) over the
        dimensions' ranges widened by 5 %.  Returns a Marginals."""
        return _marginals(self._lib, self._check, trace_ptr, nslots, *self._trace_shape(), n1, n2, pair_dims, sample_stride,
                          ranges, stream)

    def TraceMoments(self, trace_ptr, nslots, centre=None, stream=0):
        """The sums behind the mean and covariance of a trace StepSave wrote (MakeCovariance.C:63-89), taken on the
        device over every slot of every chain about `centre` (default: the origin, as the macro has it; the mean of
        the run conditions the covariance better).  Returns a TraceMoments."""
        return _trace_moments(self._lib, self._check, trace_ptr, nslots, *self._trace_shape(), centre, stream)

    def Convergence(self, trace_ptr, nslots, nsegments=2, centre=None, stream=0):
        """The sums behind split R-hat and the multi-chain effective sample size of a trace StepSave wrote
        (smcmc_trace_convergence), taken on the device: every chain cut into `nsegments` segments (2: split R-hat, 1: the
        plain form), each about its own mean.  Pass a `centre` near the mean, e.g. TraceMoments(...).mean from one
        earlier pass: the variance of the segment means cancels like any E[yy] - E[y]^2.  Returns a Convergence."""
        return _convergence(self._lib, self._check, trace_ptr, nslots, *self._trace_shape(), nsegments, centre, stream)

    def OrderStatistics(self, trace_ptr, nslots, ranks, stream=0):
        """Exact order statistics of every dimension of a trace StepSave wrote, selected on the device
        (smcmc_trace_order_statistics): for each zero-based rank < nslots * nchains the entry with that many entries
        before it in the order of include/smcmc_order_key.h, with the numbers of smaller and of equal entries.  More than
        32 ranks are taken in several calls.  Returns a TraceQuantiles."""
        return _order_statistics(self._lib, self._check, trace_ptr, nslots, *self._trace_shape(), ranks, stream)

    def Quantiles(self, trace_ptr, nslots, q=(0.025, 0.16, 0.5, 0.84, 0.975), stream=0):
        """The quantiles `q` of every dimension of a trace StepSave wrote -- the median and the 68 % and 95 % credible
        intervals by default -- from exact order statistics taken on the device: only the ranks floor((N - 1) q) and
        ceil((N - 1) q) that TraceQuantiles.quantile interpolates between are asked for.  Returns a TraceQuantiles."""
        return _order_statistics(self._lib, self._check, trace_ptr, nslots, *self._trace_shape(),
                                 quantile_ranks(int(nslots) * self.nchains, q), stream)

    def DigitCounts(self, trace_ptr, nslots, pass_, prefixes=None, nprefix=None, stream=0):
        """One pass of the selection over this engine's trace (smcmc_trace_digit_counts): counts[dim][nprefix][256], the
        `count_fn` of order_statistics_combined for one rank's shard.  prefixes: [dim][nprefix] (None at pass 0, where
        nprefix says how many copies of the counts to return; default 1)."""
        return trace_digit_counts(trace_ptr, nslots, *self._trace_shape(), pass_, prefixes, nprefix, stream, _lib=self._lib,
                                  _check=self._check)


class Autocorrelation:
    """a(lag) = (E[x_t x_(t-lag)] - mean^2) / var per dimension (MakeAutocorrelation.C:127-139) from the pooled sums
    of Engine.AutocorrelationSums; sums of several ranks add (`+`)."""

    def __init__(self, total, lagged, nslots, nchains):
        self.sum, self.lagged, self.nslots, self.nchains = np.array(total), np.array(lagged), nslots, nchains

    def __add__(self, other):
        if self.nslots != other.nslots:
            raise ValueError("traces of different lengths do not pool")
        return Autocorrelation(self.sum + other.sum, self.lagged + other.lagged, self.nslots, self.nchains + other.nchains)

    def rho(self):
        """[lag][dim]"""
        nlag = min(self.lagged.shape[0], self.nslots)
        n = (self.nslots - np.arange(nlag))[:, None] * float(self.nchains)
        mean = self.sum / n[0]
        var = self.lagged[0] / n[0] - mean * mean
        return (self.lagged[:nlag] / n - mean * mean) / var

    def tau(self):
        """Integrated autocorrelation time per dimension in slots: 1 + 2 sum rho, the sum cut where a pair of
        consecutive lags turns negative (initial positive sequence)."""
        rho = self.rho()
        out = np.ones(rho.shape[1])
        for d in range(rho.shape[1]):
            for k in range(1, rho.shape[0] - 1, 2):
                pair = rho[k, d] + rho[k + 1, d]
                if pair < 0:
                    break
                out[d] += 2.0 * pair
        return out


class AutocorrelationGrid:
    """The pooled sums of smcmc_autocorrelation_grid_sums (include/smcmc.h) on the lags `lags` = lag_first + i lag_step:
    sum[dim], sumsq[dim] (lag 0) and lagged[lag][dim] about one reference point.
      counts   terms per lag, max(nslots - lag, 0) * nchains
      rho()    [lag][dim], (lagged / counts - mean^2) / (sumsq / n - mean^2); NaN for a lag beyond the trace
    Sums of several ranks add (`+`) when the grid and nslots agree."""

    def __init__(self, lags, total, sumsq, lagged, nslots, nchains):
        self.lags = np.array(lags, dtype=np.int64)
        self.sum, self.sumsq, self.lagged = _f64(total).copy(), _f64(sumsq).copy(), _f64(lagged).copy()
        self.nslots, self.nchains = int(nslots), int(nchains)
        if (self.lags.ndim != 1 or self.sum.ndim != 1 or self.sumsq.shape != self.sum.shape
                or self.lagged.shape != (self.lags.size, self.sum.size)):
            raise ValueError("lags[lag], sum[dim], sumsq[dim] and lagged[lag][dim] do not fit together")

    @property
    def counts(self):
        return np.maximum(self.nslots - self.lags, 0) * float(self.nchains)

    def __add__(self, other):
        if self.nslots != other.nslots:
            raise ValueError("traces of different lengths do not pool")
        if not np.array_equal(self.lags, other.lags):
            raise ValueError("sums on different lag grids do not add")
        return AutocorrelationGrid(self.lags, self.sum + other.sum, self.sumsq + other.sumsq, self.lagged + other.lagged,
                                   self.nslots, self.nchains + other.nchains)

    def rho(self):
        """[lag][dim]"""
        n = float(self.nslots) * self.nchains
        mean = self.sum / n
        var = self.sumsq / n - mean * mean
        with np.errstate(divide="ignore", invalid="ignore"):
            return (self.lagged / self.counts[:, None] - mean * mean) / var


def _autocorrelation_grid(lib, check, trace_ptr, nslots, dim, dim_stride, nchains, nchains_padded, lag_first, lag_step,
                          nlags, centre, stream):
    """The body of the engines' AutocorrelationGrid methods: calls of at most AUTOCORR_GRID_MAX_LAGS lags each, the rows
    concatenated (a row's bits do not depend on the call it is taken in)."""
    c = None if centre is None else _f64(centre)
    if c is not None and c.shape != (dim,):
        raise ValueError("centre must be [dim]")
    nslots, lag_first, lag_step, nlags = int(nslots), int(lag_first), int(lag_step), int(nlags)
    if nlags < 1:
        raise ValueError("nlags must be at least 1")
    total, sumsq, lagged = np.zeros(dim), np.zeros(dim), np.zeros((nlags, dim))
    for i0 in range(0, nlags, _capi.AUTOCORR_GRID_MAX_LAGS):
        n = min(_capi.AUTOCORR_GRID_MAX_LAGS, nlags - i0)
        rows = np.zeros((n, dim))
        check(lib.smcmc_autocorrelation_grid_sums(C.c_void_p(int(trace_ptr)), nslots, dim, dim_stride, nchains,
                                                  nchains_padded, None if c is None else _ptr(c),
                                                  lag_first + i0 * lag_step, lag_step, n, _ptr(total), _ptr(sumsq),
                                                  _ptr(rows), C.c_void_p(int(stream))))
        lagged[i0:i0 + n] = rows
    return AutocorrelationGrid(lag_first + lag_step * np.arange(nlags), total, sumsq, lagged, nslots, nchains)


class AutocorrelationPlan:
    """The constants MakeAutocorrelation.C derives from the number of entries (autocorrelation_plan): entries, depth,
    max_lag, bins, lag_step, trials, lags[lag], lag_bins[lag] (0-based bin of each lag) and bin_centres[bin]."""

    def __init__(self, entries, depth, max_lag, bins, lag_step, trials):
        self.entries, self.depth, self.max_lag, self.bins = entries, depth, max_lag, bins
        self.lag_step, self.trials = lag_step, trials
        self.lags = np.arange(1, max_lag, lag_step, dtype=np.int64)
        # the fixed-width axis of include/smcmc.h over [0, max_lag), filled at lag + 0.5 (:121)
        self.lag_bins = np.array([int(bins * (lag + 0.5) / max_lag) for lag in self.lags], dtype=np.int64)
        self.bin_centres = (np.arange(bins) + 0.5) * (float(max_lag) / bins)

    def __eq__(self, other):
        return (isinstance(other, AutocorrelationPlan)
                and (self.entries, self.depth, self.max_lag, self.bins, self.lag_step, self.trials)
                == (other.entries, other.depth, other.max_lag, other.bins, other.lag_step, other.trials))


def autocorrelation_plan(entries, depth=30000, bins=100, precision=0.01):
    """MakeAutocorrelation.C's constants for a tree of `entries` entries (:62, 70-73, 98-99, 104-106):
      maxLag  = min(int(entries - sqrt(entries)), depth)        bins    = min(bins, maxLag)
      lagStep = max(1, int(0.5 maxLag / bins))                  trials  = min(int(maxLag + 1 / precision^3), entries)
      lags 1, 1 + lagStep, ... < maxLag, each in bin int(bins (lag + 0.5) / maxLag).
    A pure function; returns an AutocorrelationPlan."""
    entries = int(entries)
    max_lag = min(int(entries - np.sqrt(float(entries))), int(depth)) if entries > 0 else 0
    if max_lag < 2:
        raise ValueError("the macro evaluates no lag below 4 entries")
    bins = min(int(bins), max_lag)
    lag_step = max(1, int(0.5 * max_lag / bins))
    trials = min(int(max_lag + 1.0 / (precision * precision * precision)), entries)
    return AutocorrelationPlan(entries, int(depth), max_lag, bins, lag_step, trials)


class MacroAutocorrelation:
    """What MakeAutocorrelation.C writes, from pooled device sums over the last plan.trials slots on the macro's lag
    grid (the engines' MakeAutocorrelation; from_sums is pure).  With n = trials * nchains and y = x - centre:
      bin_centres      [bin], the centres of the bins over [0, maxLag)
      mean[d]          centre + sum / n                                          (meanValues, :132)
      err2[d]          sumsq / n - (sum / n)^2: the "s" error of meanValues, squared (:133)
      autocorr[d][bin] (v / e - (sum / n)^2) / err2, v and e the sums of `lagged` and of `counts` over the lags that
                       fall into the bin (:135-139); a bin no lag falls into is 0/0 = NaN, as in the macro
      average[bin], spread[bin]   mean and population r.m.s. of autocorr over the dimensions (avgCorr, option "S", :146)
    Sums of several ranks add (`+`) when the plan and the centre agree.
    Deviations from the macro, on purpose (include/smcmc.h states them): its ring buffer holds floats, so every value is
    rounded to single precision before it is multiplied, and the values here are doubles; its TH1F sums are floats, and
    these are doubles; it reads one chain, and here the chains are pooled into one sum, so one chain is the macro.  The
    macro's reference point is the origin (centre = None); another centre changes autocorr only through the edges of
    the lagged sums, O(lag / trials)."""

    def __init__(self, plan, total, sumsq, lagged, nchains, centre=None):
        self.plan, self.nchains = plan, int(nchains)
        self.sum, self.sumsq, self.lagged = _f64(total).copy(), _f64(sumsq).copy(), _f64(lagged).copy()
        self.centre = np.zeros(self.sum.size) if centre is None else _f64(centre).copy()
        if (self.sum.ndim != 1 or self.sumsq.shape != self.sum.shape or self.centre.shape != self.sum.shape
                or self.lagged.shape != (plan.lags.size, self.sum.size)):
            raise ValueError("sum[dim], sumsq[dim], centre[dim] and lagged[lag][dim] do not fit the plan")

    @classmethod
    def from_sums(cls, plan, total, sumsq, lagged, nchains, centre=None):
        return cls(plan, total, sumsq, lagged, nchains, centre)

    def __add__(self, other):
        if self.plan != other.plan:
            raise ValueError("sums of different plans do not add")
        if not np.array_equal(self.centre, other.centre):
            raise ValueError("sums about different centres do not add")
        return MacroAutocorrelation(self.plan, self.sum + other.sum, self.sumsq + other.sumsq, self.lagged + other.lagged,
                                    self.nchains + other.nchains, self.centre)

    @property
    def counts(self):
        """[lag]: the macro's fills per lag (`fills <= lag` breaks, :118), times the chains"""
        return (self.plan.trials - self.plan.lags) * float(self.nchains)

    @property
    def bin_centres(self):
        return self.plan.bin_centres

    @property
    def _ymean(self):
        return self.sum / (float(self.plan.trials) * self.nchains)

    @property
    def mean(self):
        return self.centre + self._ymean

    @property
    def err2(self):
        m = self._ymean
        return self.sumsq / (float(self.plan.trials) * self.nchains) - m * m

    @property
    def autocorr(self):
        """[dim][bin]"""
        dim, bins = self.sum.size, self.plan.bins
        v, e = np.zeros((dim, bins)), np.zeros(bins)
        counts = self.counts
        for i, b in enumerate(self.plan.lag_bins):      # lags ascending, as the macro fills them
            v[:, b] += self.lagged[i]
            e[b] += counts[i]
        m = self._ymean
        with np.errstate(divide="ignore", invalid="ignore"):
            return (v / e[None, :] - (m * m)[:, None]) / self.err2[:, None]

    @property
    def average(self):
        return self.autocorr.mean(axis=0)

    @property
    def spread(self):
        return self.autocorr.std(axis=0)


def _make_autocorrelation(lib, check, trace_ptr, nslots, dim, dim_stride, nchains, nchains_padded, centre, stream, plan):
    """The body of the engines' MakeAutocorrelation methods."""
    if plan is None:
        plan = autocorrelation_plan(int(nslots))
    elif plan.entries != int(nslots):
        raise ValueError("the plan is for %d entries, the trace has %d slots" % (plan.entries, int(nslots)))
    first = int(trace_ptr) + 8 * (plan.entries - plan.trials) * dim_stride * nchains_padded   # the last `trials` slots
    g = _autocorrelation_grid(lib, check, first, plan.trials, dim, dim_stride, nchains, nchains_padded, 1, plan.lag_step,
                              plan.lags.size, centre, stream)
    return MacroAutocorrelation.from_sums(plan, g.sum, g.sumsq, g.lagged, nchains, centre)


class Marginals:
    """The marginal distributions of a trace as TestMarginalization.C histograms them, from the device counts of
    smcmc_trace_ranges / smcmc_marginal_histograms (include/smcmc.h has the bin rule):
      lo, hi [dim]                 the ranges of the dimensions over the sampled slots (macro :45-63)
      n1, lo1, hi1 [dim]; counts1 [dim][n1 + 2]               the 1-D axes and counts (0 / n1 + 1: under- / overflow)
      pair_dims [P]; n2, lo2, hi2 [P]; counts2 [P][P][n2 + 2][n2 + 2]   table (p, q): x = pair_dims[p], y = pair_dims[q]
    Counts are unsigned 64-bit integers and exact.  Counts of several ranks filled on identical axes add (`+`); their
    ranges combine beforehand with merge_ranges.  Everything derived here is host-side numpy."""

    def __init__(self, lo, hi, nslots, nchains, lo1=None, hi1=None, counts1=None, pair_dims=None, lo2=None, hi2=None,
                 counts2=None):
        self.lo, self.hi, self.nslots, self.nchains = _f64(lo), _f64(hi), int(nslots), int(nchains)
        self.lo1 = None if lo1 is None else _f64(lo1)
        self.hi1 = None if hi1 is None else _f64(hi1)
        self.counts1 = None if counts1 is None else np.array(counts1, dtype=np.uint64)
        self.pair_dims = None if pair_dims is None else np.array(pair_dims, dtype=np.int32)
        self.lo2 = None if lo2 is None else _f64(lo2)
        self.hi2 = None if hi2 is None else _f64(hi2)
        self.counts2 = None if counts2 is None else np.array(counts2, dtype=np.uint64)

    @property
    def n1(self): return 0 if self.counts1 is None else self.counts1.shape[1] - 2

    @property
    def n2(self): return 0 if self.counts2 is None else self.counts2.shape[2] - 2

    @staticmethod
    def _edges(lo, hi, n):
        return lo[:, None] + (hi - lo)[:, None] * (np.arange(n + 1) / float(n))[None, :]

    @property
    def edges1(self):
        """[dim][n1 + 1]: the bin edges of every 1-D axis (for plotting; the counting used the bin rule, not these)."""
        return None if self.counts1 is None else self._edges(self.lo1, self.hi1, self.n1)

    @property
    def edges2(self):
        """[P][n2 + 1]: the bin edges of the axis of every pair dimension."""
        return None if self.counts2 is None else self._edges(self.lo2, self.hi2, self.n2)

    @staticmethod
    def _same(a, b):
        return (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and np.array_equal(a, b))

    def __add__(self, other):
        if self.nslots != other.nslots:
            raise ValueError("traces of different lengths do not pool")
        for name in ("lo", "hi", "lo1", "hi1", "pair_dims", "lo2", "hi2"):
            if not self._same(getattr(self, name), getattr(other, name)):
                raise ValueError("histograms add only on identical bins and ranges (%s differs)" % name)
        if (self.n1, self.n2) != (other.n1, other.n2):
            raise ValueError("histograms add only on identical bins and ranges (the numbers of bins differ)")
        return Marginals(self.lo, self.hi, self.nslots, self.nchains + other.nchains, self.lo1, self.hi1,
                         None if self.counts1 is None else self.counts1 + other.counts1, self.pair_dims, self.lo2, self.hi2,
                         None if self.counts2 is None else self.counts2 + other.counts2)

    @staticmethod
    def merge_ranges(ranges):
        """(lo, hi) over several ranks' (lo, hi) pairs (or Marginals): the ranges of the whole ensemble."""
        pairs = [(r.lo, r.hi) if isinstance(r, Marginals) else (_f64(r[0]), _f64(r[1])) for r in ranges]
        lo, hi = pairs[0][0].copy(), pairs[0][1].copy()
        for a, b in pairs[1:]:
            lo, hi = np.minimum(lo, a), np.maximum(hi, b)
        return lo, hi

    @staticmethod
    def macro_sample_stride(nslots):
        """The stride of the macro's range loop (`entry += 0.001*entries` on an int, then ++entry; :54-62)."""
        return 1 + int(0.001 * int(nslots))

    @staticmethod
    def macro_axes(lo, hi, pair_dims):
        """The macro's axes from per-dimension ranges: ((absMin, absMax) of :52-53, 59-60, (lo2, hi2) of the pair
        dimensions: the dimension's range widened by 5 % of its width on both sides, :85-89)."""
        lo, hi = _f64(lo), _f64(hi)
        abs_min = min(1e20, float(np.min(lo)))
        abs_max = max(-1e20, float(np.max(hi)))
        p = np.asarray(pair_dims, dtype=np.int64)
        r = 0.05 * (hi[p] - lo[p])
        return (abs_min, abs_max), (lo[p] - r, hi[p] + r)

    def macro_ranges(self, pair_dims=None):
        """macro_axes of this object's ranges (pair_dims: its own, or the macro's first min(dim, 10) dimensions)."""
        if pair_dims is None:
            pair_dims = self.pair_dims if self.pair_dims is not None else np.arange(min(self.lo.size, 10))
        return self.macro_axes(self.lo, self.hi, pair_dims)

    def density(self, d):
        """[n1]: the in-range counts of dimension d over (all points x bin width): a density that integrates to the
        in-range fraction."""
        c = self.counts1[d].astype(np.float64)
        return c[1:-1] / (c.sum() * (self.hi1[d] - self.lo1[d]) / self.n1)

    def quantile(self, d, q):
        """The q-quantile of dimension d from its histogram: linear interpolation inside the bin where the cumulative
        count crosses q x (all points); underflow counts as sitting on lo1[d], overflow on hi1[d].  The resolution is
        one bin."""
        c = self.counts1[d].astype(np.float64)
        n, lo, hi = self.n1, float(self.lo1[d]), float(self.hi1[d])
        target = float(q) * c.sum()
        cum = np.cumsum(c[:-1])                 # cum[k]: points below edge k (the underflow included)
        if target <= cum[0]:
            return lo
        if target > cum[n]:
            return hi
        k = int(np.searchsorted(cum, target, side="left"))     # first edge with cum >= target: inside bin k
        return lo + (hi - lo) * ((k - 1) + (target - cum[k - 1]) / c[k]) / n

    def interval(self, d, level=0.68):
        """The central credible interval of dimension d holding `level` of the points (to one bin)."""
        return self.quantile(d, 0.5 * (1.0 - level)), self.quantile(d, 0.5 * (1.0 + level))


def _marginals(lib, check, trace_ptr, nslots, dim, dim_stride, nchains, nchains_padded, n1, n2, pair_dims, sample_stride,
               ranges, stream):
    """Ranges (unless given) and then the fill with the macro's axes: the body of the engines' Marginals methods."""
    up = C.POINTER(C.c_uint64)
    trace, nslots, st = C.c_void_p(int(trace_ptr)), int(nslots), C.c_void_p(int(stream))
    if pair_dims is None:
        pair_dims = np.arange(min(dim, 10))                        # the macro's "only doing 10" (:39-43)
    pair_dims = np.ascontiguousarray(pair_dims, dtype=np.int32)
    if ranges is None:
        if sample_stride is None:
            sample_stride = Marginals.macro_sample_stride(nslots)
        lo, hi = np.zeros(dim), np.zeros(dim)
        check(lib.smcmc_trace_ranges(trace, nslots, dim, dim_stride, nchains, nchains_padded, int(sample_stride), _ptr(lo),
                                     _ptr(hi), st))
    else:
        lo, hi = _f64(ranges[0]), _f64(ranges[1])
        if lo.shape != (dim,) or hi.shape != (dim,):
            raise ValueError("ranges must be (lo[dim], hi[dim])")
    (abs_min, abs_max), (lo2, hi2) = Marginals.macro_axes(lo, hi, pair_dims)
    lo1, hi1 = np.full(dim, abs_min), np.full(dim, abs_max)
    lo2, hi2 = _f64(lo2), _f64(hi2)
    P = int(pair_dims.size)
    counts1 = np.zeros((dim, n1 + 2), dtype=np.uint64) if n1 else None
    counts2 = np.zeros((P, P, n2 + 2, n2 + 2), dtype=np.uint64) if P else None
    check(lib.smcmc_marginal_histograms(trace, nslots, dim, dim_stride, nchains, nchains_padded, int(n1), _ptr(lo1), _ptr(hi1),
                                        counts1.ctypes.data_as(up) if n1 else None, P,
                                        pair_dims.ctypes.data_as(C.POINTER(C.c_int32)), int(n2), _ptr(lo2), _ptr(hi2),
                                        counts2.ctypes.data_as(up) if P else None, st))
    return Marginals(lo, hi, nslots, nchains, lo1 if n1 else None, hi1 if n1 else None, counts1,
                     pair_dims if P else None, lo2 if P else None, hi2 if P else None, counts2)


class TraceMoments:
    """The mean and covariance of a saved trace as MakeCovariance.C:63-89 takes them, from the raw sums of
    smcmc_trace_moments about `centre`: sum[d] = sum y_d, sumsq[i][j] = sum y_i y_j, y = x - centre, over
    n = nslots * nchains points.
      mean         centre + sum / n
      covariance   sumsq / n - (sum / n)(sum / n)^T: the macro's :84 taken about the centre (a covariance does not
                   depend on the point it is taken about; about a point near the mean the difference cancels less)
      spread       sqrt(diag covariance): the errors of the macro's TProfile in its "S" option (:58-60)
      correlation  covariance / (spread_i spread_j)
    Sums of several ranks add (`+`): the right operand is re-centred on the left one's centre first."""

    def __init__(self, total, sumsq, nslots, nchains, centre=None):
        self.sum, self.sumsq = _f64(total).copy(), _f64(sumsq).copy()
        self.nslots, self.nchains = int(nslots), int(nchains)
        self.centre = np.zeros(self.sum.size) if centre is None else _f64(centre).copy()
        if self.sumsq.shape != (self.sum.size, self.sum.size) or self.centre.shape != self.sum.shape:
            raise ValueError("sum[dim], sumsq[dim][dim] and centre[dim] do not fit together")

    @property
    def n(self):
        return float(self.nslots) * float(self.nchains)

    def about(self, centre):
        """The same sums taken about another point: with s = old centre - new centre, y' = y + s."""
        centre = _f64(centre)
        s, n = self.centre - centre, self.n
        total = self.sum + n * s
        sumsq = self.sumsq + np.outer(s, self.sum) + np.outer(self.sum, s) + n * np.outer(s, s)
        return TraceMoments(total, sumsq, self.nslots, self.nchains, centre)

    def __add__(self, other):
        if self.nslots != other.nslots:
            raise ValueError("traces of different lengths do not pool")
        o = other if np.array_equal(other.centre, self.centre) else other.about(self.centre)
        return TraceMoments(self.sum + o.sum, self.sumsq + o.sumsq, self.nslots, self.nchains + o.nchains, self.centre)

    @property
    def mean(self):
        return self.centre + self.sum / self.n

    @property
    def covariance(self):
        m = self.sum / self.n
        return self.sumsq / self.n - np.outer(m, m)

    @property
    def spread(self):
        return np.sqrt(np.diag(self.covariance))

    @property
    def correlation(self):
        s = self.spread
        return self.covariance / np.outer(s, s)


def _trace_moments(lib, check, trace_ptr, nslots, dim, dim_stride, nchains, nchains_padded, centre, stream):
    """The body of the engines' TraceMoments methods."""
    c = None if centre is None else _f64(centre)
    if c is not None and c.shape != (dim,):
        raise ValueError("centre must be [dim]")
    total, sumsq = np.zeros(dim), np.zeros((dim, dim))
    check(lib.smcmc_trace_moments(C.c_void_p(int(trace_ptr)), int(nslots), dim, dim_stride, nchains, nchains_padded,
                                  None if c is None else _ptr(c), _ptr(total), _ptr(sumsq), C.c_void_p(int(stream))))
    return TraceMoments(total, sumsq, nslots, nchains, c)


class Convergence:
    """Split R-hat and the multi-chain effective sample size of a saved trace, from the raw sums of
    smcmc_trace_convergence (include/smcmc.h has the definition): every chain is cut into segments of L slots, M
    segment-chains in all, y = x - centre, s1_m the sum of segment-chain m and z = y - s1_m / L:
      sum[d] = sum_m s1_m,  sumsq_of_sums[d] = sum_m s1_m^2,  within[k][d] = sum_m sum_{t >= k} z_t z_(t-k)
      W             within[0] / (M (L - 1)): the mean within-chain variance
      var_of_means  (sumsq_of_sums / L^2 - (sum / L)^2 / M) / (M - 1): the variance of the segment means (B / L)
      var_plus      (L - 1) / L W + var_of_means
      rhat()        sqrt(var_plus / W) (Gelman-Rubin; the split form when the segments are halves); NaN where W is 0 or
                    M < 2
      rho()         [lag][dim], 1 - (W - within[k] / (M L)) / var_plus for the lags below min(64, L)
      tau()         Geyer's initial monotone sequence (BDA3 section 11.5, Vehtari et al. 2021): the pairs
                    P_j = rho[2j] + rho[2j + 1] up to the first negative one, P_j = min(P_j, P_(j-1)), -1 + 2 sum P_j
      ess()         M L / tau()
      truncated()   per dimension: the pairs ran out at the last available lag before one turned negative (the
                    autocorrelation outlives the 64 lags, or L): ess() is then an upper bound
      mean()        centre + sum / (M L)
    sumsq_of_sums / L^2 - (sum / L)^2 / M cancels like any E[yy] - E[y]^2: take the sums about a centre near the mean,
    e.g. TraceMoments(...).mean from one earlier pass.  Sums of several ranks add (`+`) when L and the centre agree."""

    def __init__(self, total, sumsq_of_sums, within, L, M, centre=None):
        self.sum, self.sumsq_of_sums, self.within = _f64(total).copy(), _f64(sumsq_of_sums).copy(), _f64(within).copy()
        self.L, self.M = int(L), int(M)
        self.centre = np.zeros(self.sum.size) if centre is None else _f64(centre).copy()
        if (self.sum.ndim != 1 or self.sumsq_of_sums.shape != self.sum.shape or self.centre.shape != self.sum.shape
                or self.within.ndim != 2 or self.within.shape[1] != self.sum.size):
            raise ValueError("sum[dim], sumsq_of_sums[dim], within[lag][dim] and centre[dim] do not fit together")

    def __add__(self, other):
        if self.L != other.L:
            raise ValueError("segments of different lengths do not pool")
        if not np.array_equal(self.centre, other.centre):
            raise ValueError("sums about different centres do not add")
        return Convergence(self.sum + other.sum, self.sumsq_of_sums + other.sumsq_of_sums, self.within + other.within,
                           self.L, self.M + other.M, self.centre)

    @property
    def W(self):
        return self.within[0] / (float(self.M) * (self.L - 1))

    @property
    def var_of_means(self):
        if self.M < 2:
            return np.full(self.sum.size, np.nan)
        L, M = float(self.L), float(self.M)
        return (self.sumsq_of_sums / (L * L) - (self.sum / L) ** 2 / M) / (M - 1.0)

    @property
    def var_plus(self):
        return (self.L - 1.0) / self.L * self.W + self.var_of_means

    def rhat(self):
        W = self.W
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(W == 0.0, np.nan, np.sqrt(self.var_plus / W))

    def rho(self):
        """[lag][dim]"""
        nlag = min(self.within.shape[0], self.L)
        with np.errstate(divide="ignore", invalid="ignore"):
            return 1.0 - (self.W[None, :] - self.within[:nlag] / (float(self.M) * self.L)) / self.var_plus[None, :]

    def _geyer(self):
        """(tau[dim], truncated[dim])"""
        rho = self.rho()
        npairs, dim = rho.shape[0] // 2, rho.shape[1]
        tau, truncated = np.empty(dim), np.zeros(dim, dtype=bool)
        for d in range(dim):
            total, last, j = 0.0, np.inf, 0
            while j < npairs:
                pair = rho[2 * j, d] + rho[2 * j + 1, d]
                if pair < 0.0:
                    break
                last = min(pair, last) if pair == pair else pair           # a NaN pair makes tau NaN
                total += last
                j += 1
            tau[d], truncated[d] = -1.0 + 2.0 * total, j == npairs
        return tau, truncated

    def tau(self):
        return self._geyer()[0]

    def truncated(self):
        return self._geyer()[1]

    def ess(self):
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(self.M) * self.L / self.tau()

    def mean(self):
        return self.centre + self.sum / (float(self.M) * self.L)


def _convergence(lib, check, trace_ptr, nslots, dim, dim_stride, nchains, nchains_padded, nsegments, centre, stream):
    """The body of the engines' Convergence methods."""
    c = None if centre is None else _f64(centre)
    if c is not None and c.shape != (dim,):
        raise ValueError("centre must be [dim]")
    nslots, nsegments = int(nslots), int(nsegments)
    total, sumsq, within = np.zeros(dim), np.zeros(dim), np.zeros((_capi.AUTOCORR_LAGS, dim))
    check(lib.smcmc_trace_convergence(C.c_void_p(int(trace_ptr)), nslots, dim, dim_stride, nchains, nchains_padded,
                                      nsegments, None if c is None else _ptr(c), None, _ptr(total), _ptr(sumsq),
                                      _ptr(within), C.c_void_p(int(stream))))
    return Convergence(total, sumsq, within, nslots // nsegments, nsegments * nchains, c)


class PosteriorPredictive:
    """The posterior-predictive histograms of a saved trace under one of the likelihoods over a simulated event sample
    (LIKE_EVENT_SAMPLE, _TEMPLATE, _SHAPE): what FakeLikelihood::WriteSimulation writes at one point, over every point,
    from the raw sums of smcmc_event_predictive_sums about `centre`: sum[h][b] = sum y, sumsq[h][b] = sum y y,
    y = hist - centre, over n = nslots * nchains points.
      names    the histograms: ("Close", "Separated", "DecayTag"), for the shape "VeryClose" first
      data     [NH][nbins], the observed histograms the simulation is drawn over (the parameter array's)
      mean     [NH][nbins], centre + sum / n
      spread   [NH][nbins], sqrt(sumsq / n - (sum / n)^2): the band around the prediction (about a centre near the mean,
               e.g. the mean of one earlier pass, the difference cancels less)
    Sums of several ranks add (`+`): the right operand is re-centred on the left one's centre first."""

    NAMES = ("VeryClose", "Close", "Separated", "DecayTag")

    def __init__(self, total, sumsq, nslots, nchains, data, centre=None):
        self.data = _f64(data).copy()
        if self.data.ndim != 2 or self.data.shape[0] not in (3, 4) or self.data.shape[1] < 1:
            raise ValueError("data must be [3][nbins] or [4][nbins]")
        shape = self.data.shape
        total, sumsq = _f64(total), _f64(sumsq)
        centre = np.zeros(shape) if centre is None else _f64(centre)
        if total.size != self.data.size or sumsq.size != self.data.size or centre.size != self.data.size:
            raise ValueError("sum, sumsq and centre must hold one value per bin of data[NH][nbins]")
        self.sum, self.sumsq, self.centre = total.reshape(shape).copy(), sumsq.reshape(shape).copy(), centre.reshape(shape).copy()
        self.nslots, self.nchains = int(nslots), int(nchains)
        self.names = self.NAMES[4 - shape[0]:]

    @property
    def n(self):
        return float(self.nslots) * float(self.nchains)

    def about(self, centre):
        """The same sums taken about another point: with s = old centre - new centre, y' = y + s."""
        centre = _f64(centre)
        if centre.size != self.data.size:
            raise ValueError("centre must hold one value per bin of data[NH][nbins]")
        centre = centre.reshape(self.data.shape)
        s, n = self.centre - centre, self.n
        return PosteriorPredictive(self.sum + n * s, self.sumsq + 2.0 * s * self.sum + n * s * s, self.nslots, self.nchains,
                                   self.data, centre)

    def __add__(self, other):
        if self.nslots != other.nslots:
            raise ValueError("traces of different lengths do not pool")
        if self.data.shape != other.data.shape:
            raise ValueError("histograms of different shapes do not pool")
        o = other if np.array_equal(other.centre, self.centre) else other.about(self.centre)
        return PosteriorPredictive(self.sum + o.sum, self.sumsq + o.sumsq, self.nslots, self.nchains + o.nchains, self.data,
                                   self.centre)

    @property
    def mean(self):
        return self.centre + self.sum / self.n

    @property
    def spread(self):
        m = self.sum / self.n
        return np.sqrt(self.sumsq / self.n - m * m)


def _event_data_shape(likelihood, prm):
    """(header, NH, nbins) of a likelihood's parameter array; nbins = 1 where the array does not say (the library
    refuses such an array with its own words)"""
    shape = likelihood == _capi.LIKE_EVENT_SHAPE
    header, nh = (12, 4) if shape else (8, 3)
    max_bins = _capi.EVENT_SHAPE_MAX_BINS if shape else _capi.EVENT_SAMPLE_MAX_BINS
    nbins = int(prm[1]) if prm.size > 1 and np.isfinite(prm[1]) and 1 <= prm[1] <= max_bins else 1
    return header, nh, nbins


def event_predictive(likelihood, params, trace_ptr, nslots, dim_stride, nchains, nchains_padded, centre=None,
                     histograms_ptr=None, logl_ptr=None, stream=0, _lib=None):
    """smcmc_event_predictive_sums: the simulated histograms of LIKE_EVENT_SAMPLE, _TEMPLATE or _SHAPE with the flat
    parameter array `params` at every point of the trace at `trace_ptr` ([nslots][dim_stride][nchains_padded] on the
    device, as StepSave wrote it), summed per bin about `centre` ([NH][nbins]; default: the origin).  histograms_ptr:
    optional device memory [nslots][NH nbins][nchains_padded] that receives every point's histograms; logl_ptr: optional
    device memory [nslots][nchains_padded] that receives every point's log-likelihood.  Returns a PosteriorPredictive.
    (_lib: the library an engine has loaded, for Engine.PosteriorPredictive.)"""
    lib = _lib or _capi.load()
    likelihood = int(likelihood)
    prm = _f64(params).ravel()
    header, nh, nbins = _event_data_shape(likelihood, prm)
    rows = nh * nbins
    c = None if centre is None else _f64(centre).ravel()
    if c is not None and c.size != rows:
        raise ValueError("centre must be [NH][nbins]")
    total, sumsq = np.zeros(rows), np.zeros(rows)
    st = lib.smcmc_event_predictive_sums(likelihood, _ptr(prm), prm.size, C.c_void_p(int(trace_ptr)), int(nslots),
                                         int(dim_stride), int(nchains), int(nchains_padded), None if c is None else _ptr(c),
                                         C.c_void_p(int(histograms_ptr)) if histograms_ptr else None,
                                         C.c_void_p(int(logl_ptr)) if logl_ptr else None, _ptr(total), _ptr(sumsq),
                                         C.c_void_p(int(stream)))
    if st != _capi.OK:
        raise SmcmcError(st, lib.smcmc_event_sample_last_error().decode() or lib.smcmc_status_string(st).decode())
    data = prm[header:header + rows].reshape(nh, nbins)
    return PosteriorPredictive(total, sumsq, nslots, nchains, data, c)


_u64 = np.uint64
_up = C.POINTER(C.c_uint64)


def poisson_draw(seed, chain, slot, row, replica, expectation, _lib=None):
    """smcmc_poisson_draw on the host (no GPU needed): the Poisson variate of include/smcmc_poisson.h at
    (seed, chain, slot, row, replica) -- the global chain and slot -- and `expectation`.  chain, slot, row, replica and
    expectation broadcast against each other; returns doubles of that shape, NaN where the variate is invalid (an
    expectation that is NaN or infinite, or above POISSON_MAX_MEAN)."""
    lib = _lib or _capi.load()
    args = np.broadcast_arrays(np.asarray(chain, dtype=np.uint32), np.asarray(slot, dtype=np.uint32),
                               np.asarray(row, dtype=np.uint32), np.asarray(replica, dtype=np.uint32),
                               np.asarray(expectation, dtype=np.float64))
    out = np.empty(args[0].shape)
    flat = out.reshape(-1)
    y, valid = C.c_double(), C.c_int()
    draw, seed = lib.smcmc_poisson_draw, int(seed)
    for i, (c, t, r, k, e) in enumerate(zip(*(a.ravel().tolist() for a in args))):
        st = draw(seed, c, t, r, k, e, C.byref(y), C.byref(valid))
        if st != _capi.OK:
            raise SmcmcError(st, "poisson_draw: slot < 2^28, row < 2^16 and replica < 2^16")
        flat[i] = y.value
    return out if out.ndim else float(out)


class PredictiveCheck:
    """The posterior-predictive check of a buffer of predicted histograms against the observed ones, from the integer
    counts of smcmc_predictive_check (include/smcmc.h): for every valid posterior point the replicated data
    y_rep ~ Poisson(expectation) were drawn and the likelihood's own bin term summed over them (T_rep) and over the
    observed data (T_obs), per histogram and over all bins.
      names          the histograms: ("Close", "Separated", "DecayTag"), for the shape "VeryClose" first (the groups
                     numbered where the data are not an event likelihood's)
      data           [NH][nbins], the observed histograms
      below, equal   [NH][nbins] uint64: the valid points whose replicate fell below / on the observed count
      stat_counts    [NH + 1][3] uint64: points with T_rep < T_obs, with T_rep == T_obs, and the number compared; the
                     last entry is over all bins
      n, invalid     the valid points, and the points left out (an expectation that is NaN, infinite or above 2^20)
      pvalue, group_pvalues       (less + equal) / compared over all bins, and per histogram as {name: value}: the
                     fraction of replicates that fit no better than the data do (T is a log-likelihood: smaller is worse)
      mid_pvalue, group_mid_pvalues   (less + equal / 2) / compared
      bin_tail()     (P(y_rep <= data), P(y_rep >= data)) per bin, [NH][nbins] each
    Counts of several ranks, of windows of slots and of replicas add (`+`); operands whose data differ are refused."""

    def __init__(self, data, below, equal, stat_counts, invalid, names=None):
        self.data = _f64(data).copy()
        if self.data.ndim != 2:
            raise ValueError("data must be [NH][nbins]")
        shape, nh = self.data.shape, self.data.shape[0]
        self.below = np.array(below, dtype=_u64).reshape(shape)
        self.equal = np.array(equal, dtype=_u64).reshape(shape)
        self.stat_counts = np.array(stat_counts, dtype=_u64).reshape(nh + 1, 3)
        self.invalid = int(invalid)
        if names is None:
            names = PosteriorPredictive.NAMES[4 - nh:] if nh in (3, 4) else tuple("group%d" % g for g in range(nh))
        self.names = tuple(names)
        if len(self.names) != nh:
            raise ValueError("one name per histogram")

    @property
    def n(self):
        return int(self.stat_counts[-1, 2])

    def __add__(self, other):
        if self.data.shape != other.data.shape or not np.array_equal(self.data, other.data):
            raise ValueError("checks against different data do not add")
        return PredictiveCheck(self.data, self.below + other.below, self.equal + other.equal,
                               self.stat_counts + other.stat_counts, self.invalid + other.invalid, self.names)

    def _tail(self, half):
        less, same, n = (self.stat_counts[:, k].astype(np.float64) for k in range(3))
        with np.errstate(invalid="ignore", divide="ignore"):
            return (less + (0.5 if half else 1.0) * same) / n

    @property
    def pvalue(self):
        return float(self._tail(False)[-1])

    @property
    def mid_pvalue(self):
        return float(self._tail(True)[-1])

    @property
    def group_pvalues(self):
        return dict(zip(self.names, self._tail(False)[:-1].tolist()))

    @property
    def group_mid_pvalues(self):
        return dict(zip(self.names, self._tail(True)[:-1].tolist()))

    def bin_tail(self):
        """(P(y_rep <= data), P(y_rep >= data)) of every bin over the valid points"""
        n = float(self.n)
        below, equal = self.below.astype(np.float64), self.equal.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return (below + equal) / n, (n - below) / n


def predictive_check(hist_ptr, nslots, rows, nchains, nchains_padded, data, ngroups, seed, chain_offset=0, slot_offset=0,
                     replica=0, replicates_ptr=None, statistics_ptr=None, stream=0, names=None, _lib=None):
    """smcmc_predictive_check: the posterior-predictive check of the Poisson means at `hist_ptr`
    ([nslots][rows][nchains_padded] on the device, as PosteriorPredictive(histograms_ptr=...) filled it) against
    `data` ([ngroups][rows / ngroups], or flat [rows]).  replicates_ptr: optional device memory
    [nslots][rows][nchains_padded] that receives the replicated data; statistics_ptr: optional device memory
    [nslots][2 (ngroups + 1)][nchains_padded] that receives T_obs and T_rep of every group and of all rows.  Returns a
    PredictiveCheck.  (_lib: the library an engine has loaded, for Engine.PredictiveCheck.)"""
    lib = _lib or _capi.load()
    rows, ngroups = int(rows), int(ngroups)
    d = _f64(data).ravel()
    if d.size != rows:
        raise ValueError("data must hold one value per row")
    below, equal = np.zeros(max(rows, 0), dtype=_u64), np.zeros(max(rows, 0), dtype=_u64)
    stat_counts, invalid = np.zeros((max(ngroups, 0) + 1, 3), dtype=_u64), np.zeros(1, dtype=_u64)
    st = lib.smcmc_predictive_check(C.c_void_p(int(hist_ptr)) if hist_ptr else None, int(nslots), rows, int(nchains),
                                    int(nchains_padded), _ptr(d), ngroups, int(seed), int(chain_offset), int(slot_offset),
                                    int(replica), C.c_void_p(int(replicates_ptr)) if replicates_ptr else None,
                                    C.c_void_p(int(statistics_ptr)) if statistics_ptr else None, below.ctypes.data_as(_up),
                                    equal.ctypes.data_as(_up), stat_counts.ctypes.data_as(_up), invalid.ctypes.data_as(_up),
                                    C.c_void_p(int(stream)))
    if st != _capi.OK:
        raise SmcmcError(st, lib.smcmc_event_sample_last_error().decode() or lib.smcmc_status_string(st).decode())
    return PredictiveCheck(d.reshape(ngroups, rows // ngroups), below, equal, stat_counts, invalid[0], names)


_SIGN, _ONES = _u64(0x8000000000000000), _u64(0xFFFFFFFFFFFFFFFF)


def order_keys(x):
    """key(x) of include/smcmc_order_key.h for an array of doubles: uint64, whose unsigned order is
    -inf < ... < -0 < +0 < ... < +inf < NaN (every NaN the all-ones key)."""
    x = _f64(x)
    b = x.view(_u64)
    return np.where(np.isnan(x), _ONES, b ^ np.where(b >> _u64(63) != 0, _ONES, _SIGN))


def order_values(keys):
    """value(key), the inverse of order_keys (the quiet NaN 0x7FF8000000000000 for the all-ones key)."""
    k = np.ascontiguousarray(keys, dtype=_u64)
    b = np.where(k == _ONES, _u64(0x7FF8000000000000), k ^ np.where(k >> _u64(63) != 0, _SIGN, _ONES))
    return np.ascontiguousarray(b).view(np.float64)


def quantile_ranks(n, q):
    """The distinct ranks, ascending, that the quantiles `q` of n entries interpolate between: floor((n - 1) q) and
    ceil((n - 1) q) for every q in [0, 1]."""
    n = int(n)
    if n < 1:
        raise ValueError("no entries")
    ranks = set()
    for p in np.atleast_1d(_f64(q)):
        if not 0.0 <= p <= 1.0:
            raise ValueError("a quantile's probability lies in [0, 1]")
        h = float(n - 1) * float(p)
        ranks.update((int(np.floor(h)), int(np.ceil(h))))
    return np.array(sorted(ranks), dtype=_u64)


class TraceQuantiles:
    """Exact order statistics of the rows of a saved trace (smcmc_trace_order_statistics; include/smcmc.h has the order)
    and the quantiles between them.  Over the n = nslots * nchains entries of each row:
      ranks  [R]       the zero-based ranks asked for
      values [rows][R] the entry with exactly ranks[r] entries before it: the bits of an entry of the trace
      below  [rows][R] uint64, the entries with a smaller key than that one
      equal  [rows][R] uint64, the entries with the same key (a rejected step repeats a value: ties are the normal case)
      quantile(q)      with h = (n - 1) q, lo = floor(h), hi = ceil(h): v_lo + (h - lo) (v_hi - v_lo), numpy's "linear"
                       method; both ranks must be among `ranks` (Quantiles asks for them)
      median           quantile(0.5)
      interval(level)  the central credible interval holding `level` of the entries: the quantiles (1 -+ level) / 2
    Results have the shape `shape` of the rows ([dim]; [NH][nbins] for the predictive histograms), a sequence of
    probabilities adds a last axis.  Selected values do not add: ranks combine the counts of the passes instead
    (order_statistics_combined)."""

    def __init__(self, ranks, values, below, equal, n, shape=None):
        self.ranks = np.array(ranks, dtype=_u64).ravel()
        self.values = _f64(values).copy()
        self.below, self.equal = np.array(below, dtype=_u64), np.array(equal, dtype=_u64)
        self.n = int(n)
        want = (self.values.shape[0] if self.values.ndim == 2 else -1, self.ranks.size)
        if self.values.shape != want or self.below.shape != want or self.equal.shape != want:
            raise ValueError("ranks[R] and values, below, equal [rows][R] do not fit together")
        self.shape = (want[0],) if shape is None else tuple(int(s) for s in shape)
        if int(np.prod(self.shape)) != want[0]:
            raise ValueError("shape does not hold the rows")
        self._column = {int(r): i for i, r in enumerate(self.ranks)}

    def value_at(self, rank):
        """[rows]: the entry of every row at `rank`"""
        if int(rank) not in self._column:
            raise KeyError("rank %d was not asked for" % int(rank))
        return self.values[:, self._column[int(rank)]]

    def _quantile(self, q):
        q = float(q)
        if not 0.0 <= q <= 1.0:
            raise ValueError("a quantile's probability lies in [0, 1]")
        h = float(self.n - 1) * q
        lo, hi = int(np.floor(h)), int(np.ceil(h))
        v_lo, v_hi = self.value_at(lo), self.value_at(hi)
        return v_lo + (h - lo) * (v_hi - v_lo)

    def quantile(self, q):
        if np.ndim(q) == 0:
            return self._quantile(q).reshape(self.shape)
        return np.stack([self._quantile(p) for p in q], axis=-1).reshape(self.shape + (len(q),))

    @property
    def median(self):
        return self.quantile(0.5)

    def interval(self, level=0.68):
        """(lower, upper): the quantiles (1 - level) / 2 and (1 + level) / 2, the probabilities rounded to twelve decimals so
        that level 0.68 asks for the 0.16 and 0.84 that Quantiles takes by default, not a neighbouring double"""
        return self.quantile(round(0.5 * (1.0 - level), 12)), self.quantile(round(0.5 * (1.0 + level), 12))


def _order_statistics(lib, check, trace_ptr, nslots, dim, dim_stride, nchains, nchains_padded, ranks, stream, shape=None):
    """The body of the engines' OrderStatistics and Quantiles methods: calls of at most ORDER_MAX_RANKS ranks each."""
    ranks = np.ascontiguousarray(ranks, dtype=_u64).ravel()
    if ranks.size < 1:
        raise ValueError("at least one rank")
    nslots = int(nslots)
    values = np.zeros((dim, ranks.size))
    below, equal = np.zeros((dim, ranks.size), dtype=_u64), np.zeros((dim, ranks.size), dtype=_u64)
    for i0 in range(0, ranks.size, _capi.ORDER_MAX_RANKS):
        part = np.ascontiguousarray(ranks[i0:i0 + _capi.ORDER_MAX_RANKS])
        v = np.zeros((dim, part.size))
        b, e = np.zeros((dim, part.size), dtype=_u64), np.zeros((dim, part.size), dtype=_u64)
        check(lib.smcmc_trace_order_statistics(C.c_void_p(int(trace_ptr)), nslots, dim, dim_stride, nchains, nchains_padded,
                                               part.size, part.ctypes.data_as(_up), _ptr(v), b.ctypes.data_as(_up),
                                               e.ctypes.data_as(_up), C.c_void_p(int(stream))))
        values[:, i0:i0 + part.size], below[:, i0:i0 + part.size], equal[:, i0:i0 + part.size] = v, b, e
    return TraceQuantiles(ranks, values, below, equal, nslots * nchains, shape)


def trace_digit_counts(trace_ptr, nslots, dim, dim_stride, nchains, nchains_padded, pass_, prefixes=None, nprefix=None,
                       stream=0, _lib=None, _check=None):
    """smcmc_trace_digit_counts: counts[dim][nprefix][256] of pass `pass_` over the trace at `trace_ptr`
    ([nslots][dim_stride][nchains_padded] on the device), uint64.  prefixes: [dim][nprefix] uint64, the top 8 pass_ bits
    of a key each (None at pass 0; nprefix then says how many copies of the counts to return, default 1)."""
    lib = _lib or _capi.load()
    if prefixes is not None:
        prefixes = np.ascontiguousarray(prefixes, dtype=_u64)
        if prefixes.ndim != 2 or prefixes.shape[0] != dim:
            raise ValueError("prefixes must be [dim][nprefix]")
        nprefix = prefixes.shape[1]
    nprefix = 1 if nprefix is None else int(nprefix)
    counts = np.zeros((dim, max(nprefix, 0), 1 << _capi.ORDER_DIGIT_BITS), dtype=_u64)
    st = lib.smcmc_trace_digit_counts(C.c_void_p(int(trace_ptr)), int(nslots), dim, dim_stride, nchains, nchains_padded,
                                      int(pass_), nprefix, None if prefixes is None else prefixes.ctypes.data_as(_up),
                                      counts.ctypes.data_as(_up), C.c_void_p(int(stream)))
    if _check is not None:
        _check(st)
    elif st != _capi.OK:
        raise SmcmcError(st, lib.smcmc_status_string(st).decode())
    return counts


def order_statistics_combined(count_fn, dim, n, ranks, shape=None):
    """The eight-pass selection of smcmc_trace_order_statistics on the host, from any
    count_fn(pass, prefixes) -> counts[dim][R][256]: prefixes is [dim][R] uint64 (None at pass 0: the counts of the whole
    rows, one copy per rank or one for all), counts what smcmc_trace_digit_counts defines.  Several ranks, each calling
    DigitCounts on its own shard of the chains and adding the arrays (an all-reduce of 256 R dim integers per pass), get
    the ensemble's exact order statistics this way: n is the ensemble's nslots * nchains.  Returns a TraceQuantiles, bit
    for bit what one call over the whole ensemble returns."""
    ranks = np.array(ranks, dtype=_u64).ravel()
    dim, n, R = int(dim), int(n), ranks.size
    if not 1 <= R <= _capi.ORDER_MAX_RANKS:
        raise ValueError("between 1 and %d ranks" % _capi.ORDER_MAX_RANKS)
    if np.any(ranks >= _u64(n)):
        raise ValueError("a rank is zero-based and below n")
    ndigits, bits = 1 << _capi.ORDER_DIGIT_BITS, _u64(_capi.ORDER_DIGIT_BITS)
    prefix = np.zeros((dim, R), dtype=_u64)
    resid = np.tile(ranks, (dim, 1))
    below, equal = np.zeros((dim, R), dtype=_u64), np.zeros((dim, R), dtype=_u64)
    for p in range(_capi.ORDER_PASSES):
        counts = np.asarray(count_fn(p, None if p == 0 else prefix.copy()), dtype=_u64)
        if p == 0 and counts.size == dim * ndigits:
            counts = np.repeat(counts.reshape(dim, 1, ndigits), R, axis=1)
        counts = counts.reshape(dim, R, ndigits)
        cum = np.cumsum(counts, axis=2, dtype=_u64)
        g = (cum <= resid[:, :, None]).sum(axis=2)          # the first digit whose running count exceeds the residual rank
        if np.any(g >= ndigits):
            raise ValueError("pass %d: the counts hold fewer entries than a rank asks for" % p)
        pick = g[:, :, None]
        before = np.take_along_axis(cum - counts, pick, axis=2)[:, :, 0]
        prefix = (prefix << bits) | g.astype(_u64)
        resid, below = resid - before, below + before
        if p == _capi.ORDER_PASSES - 1:
            equal = np.take_along_axis(counts, pick, axis=2)[:, :, 0]
    return TraceQuantiles(ranks, order_values(prefix), below, equal, n, shape)


def cholesky_chain(mean, covariance, nslots, nchains, seed=20240607, chain_offset=0, dim_stride=None, stream=0):
    """The Gaussian stand-in chain of CholeskyChain.C:18-66, filled on the device: covariance = U^T U, every
    (slot, chain) one draw mean + sum_i r_i U(i, :) on the random stream (seed, chain_offset + chain, slot).  Returns
    (trace, U): a torch tensor [nslots][dim_stride][nchains_padded] on the current device (rows >= dim and lanes >=
    nchains are NaN), which the reducers take as it is through trace.data_ptr(), and the decomposition [dim][dim].
    A covariance that is not positive definite raises SmcmcError (SMCMC_ERR_RUNTIME)."""
    import torch
    lib = _capi.load()
    mean, covariance = _f64(mean), _f64(covariance)
    dim = mean.size
    if mean.ndim != 1 or covariance.shape != (dim, dim):
        raise ValueError("mean must be [dim] and covariance [dim][dim]")
    dim_stride = dim if dim_stride is None else int(dim_stride)
    nchains, nslots = int(nchains), int(nslots)
    npad = (nchains + 63) // 64 * 64
    if not torch.cuda.is_available():   # the fill is a device kernel: there is no host version of it
        raise SmcmcError(_capi.ERR_NO_DEVICE, lib.smcmc_status_string(_capi.ERR_NO_DEVICE).decode())
    trace = torch.full((nslots, dim_stride, npad), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    U = np.zeros((dim, dim))
    st = lib.smcmc_cholesky_chain(_ptr(mean), _ptr(covariance), dim, nslots, nchains, npad, dim_stride, int(seed),
                                  int(chain_offset), C.c_void_p(trace.data_ptr()), _ptr(U), C.c_void_p(int(stream)))
    if st != _capi.OK:
        raise SmcmcError(st, lib.smcmc_status_string(st).decode())
    return trace, U
