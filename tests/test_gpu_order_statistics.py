"""smcmc_trace_order_statistics and smcmc_trace_digit_counts on the device.  Order statistics are selected values: the
truth everywhere is np.sort of the uint64 keys of the live entries, bit for bit, for `values`, `below` and `equal`; no
tolerance anywhere.

  1  small shapes (130 of 192 lanes, 3 of 5 rows, 1 / 3 / 17 slots) over every kind of value and every kind of rank list,
     padding lanes and rows >= dim poisoned three ways with identical results
  2  rows that span several workgroups, and rows one entry above and below the chunk one workgroup counts
  3  the pass primitive against a numpy count at passes 0, 1 and 7
  4  two shards of the chains combined on the host (order_statistics_combined) against the single call
  5  end to end: Engine.StepSave -> Quantiles, PosteriorPredictive -> PredictiveQuantiles, HmcEngine and VaatEngine traces
  6  the refusals write nothing with a device present
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu
UP, DP = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
POISONS = (-float("inf"), float("nan"), 1e300)


def _load(name):
    spec = importlib.util.spec_from_file_location("smcmc_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def key_truth(x):
    """the definition of include/smcmc.h, written out here independently of the package"""
    b = bits(x)
    return np.where(np.isnan(x), ONES, b ^ np.where(b >> np.uint64(63) != 0, ONES, np.uint64(0x8000000000000000)))


def value_truth(k):
    b = np.where(k == ONES, np.uint64(0x7FF8000000000000), k ^ np.where(k >> np.uint64(63) != 0, np.uint64(0x8000000000000000), ONES))
    return np.ascontiguousarray(b).view(np.float64)


def row_keys(x):
    """x[slot][dim][chain] (live entries) -> sorted keys [dim][N]"""
    return np.sort(key_truth(np.transpose(x, (1, 0, 2)).reshape(x.shape[1], -1)), axis=1)


def sort_truth(s, ranks):
    """(value bits, below, equal)[dim][R] from the sorted keys s[dim][N]"""
    k = s[:, np.asarray(ranks, dtype=np.int64)]
    lo = np.array([np.searchsorted(s[d], k[d], side="left") for d in range(s.shape[0])]).astype(np.uint64)
    hi = np.array([np.searchsorted(s[d], k[d], side="right") for d in range(s.shape[0])]).astype(np.uint64)
    return bits(value_truth(k)), lo, hi - lo


def device_trace(x, npad, stride, poison):
    """the device trace [slot][stride][npad] of x[slot][dim][chain]; padding lanes and rows >= dim hold `poison`"""
    import torch
    nslots, dim, nchains = x.shape
    trace = torch.full((nslots, stride, npad), poison, dtype=torch.float64, device="cuda")
    trace[:, :dim, :nchains] = torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    torch.cuda.synchronize()
    return trace


def statistics(lib, trace, nslots, dim, stride, nchains, npad, ranks):
    """(status, value bits, below, equal), the outputs prefilled"""
    r = np.array(ranks, dtype=np.uint64)
    v = np.full((dim, r.size), -7.0)
    b, e = np.full((dim, r.size), 7, dtype=np.uint64), np.full((dim, r.size), 7, dtype=np.uint64)
    st = lib.smcmc_trace_order_statistics(C.c_void_p(trace.data_ptr()), nslots, dim, stride, nchains, npad, r.size,
                                          r.ctypes.data_as(UP), v.ctypes.data_as(DP), b.ctypes.data_as(UP), e.ctypes.data_as(UP),
                                          None)
    return st, bits(v), b, e


def check(lib, x, npad, stride, ranks, what, poisons=POISONS[:1]):
    nslots, dim, nchains = x.shape
    want = sort_truth(row_keys(x), ranks)
    for poison in poisons:
        st, v, b, e = statistics(lib, device_trace(x, npad, stride, poison), nslots, dim, stride, nchains, npad, ranks)
        where = "%s, ranks %s, poison %r" % (what, list(ranks)[:4], poison)
        assert st == 0, where
        assert np.array_equal(v, want[0]), where
        assert np.array_equal(b, want[1]) and np.array_equal(e, want[2]), where


def values_of(kind, nslots, dim, nchains, seed):
    rng = np.random.default_rng(seed)
    shape = (nslots, dim, nchains)
    if kind == "gauss":             # sign and exponent shared: pass 0 is one counter
        return rng.normal(76.0, 6.0, shape)
    if kind == "runs":              # entries repeat in runs, as rejected steps leave them
        base = np.round(rng.normal(0.0, 1.0, ((nslots + 3) // 4, dim, nchains)), 1)
        return np.repeat(base, 4, axis=0)[:nslots]
    if kind == "equal":
        return np.full(shape, 3.25)
    if kind == "zeros":             # mixed signs around 0 with both zeros
        x = rng.normal(0.0, 1e-3, shape)
        x[rng.random(shape) < 0.1] = 0.0
        x[rng.random(shape) < 0.1] = -0.0
        return x
    if kind == "lastbyte":          # entries that differ only in the last byte: the last pass decides
        return (np.float64(76.0).view(np.uint64) + rng.integers(0, 256, shape).astype(np.uint64)).view(np.float64)
    assert kind == "special"        # +-inf, denormals and NaNs of both signs among ordinary values
    x = rng.normal(1.0, 2.0, shape)
    odd = np.array([np.inf, -np.inf, 5e-324, -5e-324, 1e-310, -1e-310, np.nan, 0.0], dtype=np.float64)
    odd[7] = np.array([0xFFF8000000000001], dtype=np.uint64).view(np.float64)[0]       # a NaN with the sign set
    pick = rng.random(shape) < 0.15
    x[pick] = odd[rng.integers(0, odd.size, int(pick.sum()))]
    return x


KINDS = ("gauss", "runs", "equal", "zeros", "lastbyte", "special")


def rank_lists(n):
    return ([0, n - 1], [n // 2], [n // 3, n // 3 + 1], [n // 4, n // 4], [int(r) for r in np.linspace(0, n - 1, 32)], [n - 1],
            [n - 1, 0, n // 2, 0])


@pytest.mark.parametrize("nslots", [1, 3, 17])
def test_small_shapes_every_value_and_rank(gpu, nslots):
    lib = gpu.load()
    dim, stride, nchains, npad = 3, 5, 130, 192
    for i, kind in enumerate(KINDS):
        x = values_of(kind, nslots, dim, nchains, 100 * nslots + i)
        assert x.shape == (nslots, dim, nchains)
        for j, ranks in enumerate(rank_lists(nslots * nchains)):
            # every poison on the first and on the fullest rank list of a kind, one on the others
            check(lib, x, npad, stride, ranks, "%s, %d slots" % (kind, nslots), POISONS if j in (0, 4) else POISONS[:1])


def _two_factors(n):
    """(nslots, nchains) with nslots * nchains = n, the chains a few wavefronts wide and no multiple of 64 where n allows"""
    for nchains in list(range(1000, 64, -1)) + [n]:
        if n % nchains == 0 and nchains % 64 != 0:
            return n // nchains, nchains
    return 1, n


def test_rows_over_several_workgroups(gpu):
    lib = gpu.load()
    chunk = lib.smcmc_order_chunk_entries()
    rng = np.random.default_rng(77)
    # 40 x 4 096 entries per row: ten workgroups of the chunk the source derives (asserted, so that the case keeps its point)
    assert 40 * 4096 > 4 * chunk
    x = rng.normal(76.0, 6.0, (40, 2, 4096))
    n = 40 * 4096
    check(lib, x, 4096, 2, [0, n - 1, n // 2, n // 2 + 1, int(0.025 * n), int(0.975 * n)], "40 x 4096 x 2")
    sizes = [_two_factors(chunk + 1), _two_factors(chunk - 1),          # the live entries of a row: chunk +- 1
             (chunk // 64, 64), (chunk // 64 + 1, 64), (chunk // 64 - 1, 64)]          # the whole row: chunk, chunk +- 64
    assert sizes[0][0] * sizes[0][1] == chunk + 1 and sizes[1][0] * sizes[1][1] == chunk - 1
    for nslots, nchains in sizes:
        npad = (nchains + 63) // 64 * 64
        x = np.round(rng.normal(0.0, 30.0, (nslots, 2, nchains)), 2)        # ties included
        n = nslots * nchains
        check(lib, x, npad, 3, [0, 1, n // 2, n - 2, n - 1], "%d x %d" % (nslots, nchains), POISONS[:2])


def numpy_counts(keys, p, prefixes):
    """smcmc_trace_digit_counts in numpy over the keys[dim][N] of the live entries"""
    dim, R = prefixes.shape
    out = np.zeros((dim, R, 256), dtype=np.uint64)
    digit = ((keys >> np.uint64(56 - 8 * p)) & np.uint64(255)).astype(np.int64)
    for d in range(dim):
        for i in range(R):
            hit = np.ones(keys.shape[1], dtype=bool) if p == 0 else (keys[d] >> np.uint64(64 - 8 * p)) == prefixes[d, i]
            out[d, i] = np.bincount(digit[d][hit], minlength=256)
    return out


def test_the_pass_primitive_against_numpy(gpu):
    nslots, dim, stride, nchains, npad = 5, 3, 5, 130, 192
    for kind in ("gauss", "lastbyte", "special"):
        x = values_of(kind, nslots, dim, nchains, 9)
        keys = row_keys(x)
        n = keys.shape[1]
        for poison in POISONS:
            trace = device_trace(x, npad, stride, poison)
            for p in (0, 1, 7):
                shift = np.uint64(64 - 8 * p) if p else np.uint64(0)
                # the prefixes of the smallest, the median and the largest key, one of them twice, one no entry has, and one
                # with a bit above the pass's 8p, which no entry matches
                pre = np.stack([keys[:, 0] >> shift, keys[:, n // 2] >> shift, keys[:, n - 1] >> shift, keys[:, n // 2] >> shift,
                                (keys[:, 0] >> shift) ^ np.uint64(0x55), (keys[:, n // 2] >> shift) | (np.uint64(1) << np.uint64(8 * p))],
                               axis=1) if p else np.zeros((dim, 6), dtype=np.uint64)
                got = gpu.trace_digit_counts(trace.data_ptr(), nslots, dim, stride, nchains, npad, p, pre if p else None,
                                             nprefix=6)
                want = numpy_counts(keys, p, pre)
                assert got.dtype == np.uint64 and np.array_equal(got, want), (kind, poison, p)
                if p == 0:
                    assert int(got[0, 0].sum()) == n
    # pass 7 with every prefix the library takes: 32 of them
    x = values_of("lastbyte", nslots, dim, nchains, 10)
    keys = row_keys(x)
    pre = np.ascontiguousarray(keys[:, np.linspace(0, keys.shape[1] - 1, 32).astype(np.int64)] >> np.uint64(8))
    got = gpu.trace_digit_counts(device_trace(x, npad, stride, POISONS[1]).data_ptr(), nslots, dim, stride, nchains, npad, 7, pre)
    assert np.array_equal(got, numpy_counts(keys, 7, pre))


def test_two_shards_combine_to_the_single_call(gpu):
    lib = gpu.load()
    nslots, dim, nchains = 6, 3, 130
    for kind in ("gauss", "runs", "special"):
        x = values_of(kind, nslots, dim, nchains, 21)
        n = nslots * nchains
        ranks = [0, n // 2, n // 2, n - 1, 17, 18]
        st, v, b, e = statistics(lib, device_trace(x, 192, 5, POISONS[0]), nslots, dim, 5, nchains, 192, ranks)
        assert st == 0
        halves = [device_trace(x[:, :, :65], 128, 4, POISONS[1]), device_trace(x[:, :, 65:], 128, 4, POISONS[2])]

        def count_fn(p, prefixes):
            return sum(gpu.trace_digit_counts(t.data_ptr(), nslots, dim, 4, 65, 128, p, prefixes, nprefix=len(ranks))
                       for t in halves)

        both = gpu.order_statistics_combined(count_fn, dim, n, ranks)
        assert np.array_equal(bits(both.values), v) and np.array_equal(both.below, b) and np.array_equal(both.equal, e), kind
        want = sort_truth(row_keys(x), ranks)
        assert np.array_equal(v, want[0]) and np.array_equal(b, want[1]) and np.array_equal(e, want[2]), kind


def _check_quantiles(tq, x, q, shape=None):
    """tq against numpy on the copied trace x[slot][rows][chain]"""
    s = row_keys(x)
    n = s.shape[1]
    assert tq.n == n
    want = sort_truth(s, tq.ranks)
    assert np.array_equal(bits(tq.values), want[0]) and np.array_equal(tq.below, want[1]) and np.array_equal(tq.equal, want[2])
    sv = value_truth(s)
    for p in q:
        h = (n - 1) * p
        lo, hi = int(np.floor(h)), int(np.ceil(h))
        expect = sv[:, lo] + (h - lo) * (sv[:, hi] - sv[:, lo])
        assert np.array_equal(tq.quantile(p).ravel(), expect)
        assert tq.quantile(p).shape == ((s.shape[0],) if shape is None else shape)


Q = (0.025, 0.16, 0.5, 0.84, 0.975)


def test_engine_trace_quantiles(gpu):
    import torch
    dim, nchains, nslots = 5, 130, 8
    e = gpu.Engine(dim, nchains, seed=9, mode=gpu.MODE_POOLED)
    assert e.Start(np.zeros(dim))
    e.Step(100)
    sx = torch.full((nslots, e.dim_padded, e.nchains_padded), float("nan"), dtype=torch.float64, device="cuda")
    sl = torch.empty((nslots, e.nchains_padded), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    e.StepSave(32, sx.data_ptr(), sl.data_ptr(), stride=4)
    e.sync()
    torch.cuda.synchronize()
    x = sx[:, :dim, :nchains].cpu().numpy()
    assert np.isfinite(x).all() and not np.array_equal(x[0], x[-1])
    tq = e.Quantiles(sx.data_ptr(), nslots)
    _check_quantiles(tq, x, Q)
    lo, hi = tq.interval(0.68)
    assert np.all(lo <= tq.median) and np.all(tq.median <= hi) and np.all(tq.equal >= 1)
    n = nslots * nchains
    os_ = e.OrderStatistics(sx.data_ptr(), nslots, list(range(0, n, n // 40)))       # more than 32 ranks: several calls
    assert os_.ranks.size > 32
    _check_quantiles(os_, x, ())
    e.close()


def test_predictive_quantiles(gpu, oracle):
    import torch
    ref, cases = _load("event_sample_ref"), _load("event_sample_cases")
    params = np.ascontiguousarray(cases.sample(ref, oracle, "64ev_5bins"))
    nchains, nslots, rows = 130, 8, 15
    e = gpu.Engine(9, nchains=nchains, likelihood=gpu.LIKE_EVENT_SAMPLE, likelihood_params=params, seed=20260131,
                   mode=gpu.MODE_FROZEN)
    npad, stride = e.nchains_padded, e.dim_padded
    r = ref._Stream(oracle, 77)
    assert e.Start(np.array([[2.0 * r.uniform() - 1.0 for _ in range(nchains)] for _ in range(9)]))
    x = torch.full((nslots, stride, npad), float("nan"), dtype=torch.float64, device="cuda")
    logl = torch.full((nslots, npad), float("nan"), dtype=torch.float64, device="cuda")
    h = torch.full((nslots, rows, npad), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    e.StepSave(32, x.data_ptr(), logl.data_ptr(), stride=4)
    torch.cuda.synchronize()
    pp = e.PosteriorPredictive(x.data_ptr(), nslots, histograms_ptr=h.data_ptr())
    torch.cuda.synchronize()
    hist = h.cpu().numpy()[:, :, :nchains]
    assert np.isfinite(hist).all() and hist.std(axis=(0, 2)).max() > 0.0
    tq = e.PredictiveQuantiles(h.data_ptr(), nslots)
    _check_quantiles(tq, hist, Q, shape=(3, 5))
    lo, hi = tq.interval(0.95)
    assert lo.shape == pp.mean.shape == (3, 5) and np.all(lo <= tq.median) and np.all(tq.median <= hi)
    e.close()
    gauss = gpu.Engine(9, nchains=64)
    with pytest.raises(gpu.SmcmcError) as err:
        gauss.PredictiveQuantiles(h.data_ptr(), 1)
    assert err.value.status == 2                                             # SMCMC_ERR_LOGIC: not the family's likelihood
    gauss.close()


def test_hmc_and_vaat_traces(gpu):
    """traces whose stride is dim, through the same mixin method"""
    import torch
    dim, nchains, slots = 7, 130, 6
    hm = gpu.HmcEngine(dim, nchains, seed=4)
    hm.SetMeanEpsilon(-0.2)
    hm.SetLeapFrog(5)
    hm.Start(np.random.default_rng(1).normal(size=(dim, nchains)))
    trace = torch.full((slots, dim, hm.nchains_padded), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for k in range(slots):
        hm.Step(1)
        hm.copy_positions(trace[k].data_ptr())
    hm.sync()
    torch.cuda.synchronize()
    _check_quantiles(hm.Quantiles(trace.data_ptr(), slots), trace[:, :, :nchains].cpu().numpy(), Q)
    dim, nchains, steps, stride = 6, 100, 24, 4
    va = gpu.VaatEngine(dim, nchains, seed=2)
    assert va.Start(np.zeros(dim))
    sx = torch.full((steps // stride, dim, va.nchains_padded), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    va.step_save(steps, stride, sx.data_ptr())
    torch.cuda.synchronize()
    _check_quantiles(va.Quantiles(sx.data_ptr(), steps // stride), sx[:, :, :nchains].cpu().numpy(), Q)


def test_refusals_write_nothing_with_a_device(gpu):
    import torch
    lib = gpu.load()
    trace = torch.zeros((4, 5, 192), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def stat(trace_ptr=trace.data_ptr(), nslots=4, dim=3, stride=5, nchains=130, npad=192, nranks=2, ranks=(0, 519),
             give_ranks=True, give_values=True):
        r = np.array(ranks, dtype=np.uint64)
        v = np.full((max(dim, 1), max(nranks, 1)), -7.0)
        b, e = np.full(v.shape, 7, dtype=np.uint64), np.full(v.shape, 7, dtype=np.uint64)
        st = lib.smcmc_trace_order_statistics(C.c_void_p(trace_ptr), nslots, dim, stride, nchains, npad, nranks,
                                              r.ctypes.data_as(UP) if give_ranks else None,
                                              v.ctypes.data_as(DP) if give_values else None, b.ctypes.data_as(UP),
                                              e.ctypes.data_as(UP), None)
        torch.cuda.synchronize()
        return st, bool(np.all(v == -7.0) and np.all(b == 7) and np.all(e == 7))

    def count(trace_ptr=trace.data_ptr(), nslots=4, dim=3, stride=5, nchains=130, npad=192, pass_=1, nprefix=2,
              give_prefixes=True, give_counts=True):
        p = np.zeros((dim, max(nprefix, 1)), dtype=np.uint64)
        c = np.full((dim, max(nprefix, 1), 256), 7, dtype=np.uint64)
        st = lib.smcmc_trace_digit_counts(C.c_void_p(trace_ptr), nslots, dim, stride, nchains, npad, pass_, nprefix,
                                          p.ctypes.data_as(UP) if give_prefixes else None,
                                          c.ctypes.data_as(UP) if give_counts else None, None)
        torch.cuda.synchronize()
        return st, bool(np.all(c == 7))

    refused = (1, True)
    for kw in (dict(trace_ptr=0), dict(give_ranks=False), dict(give_values=False), dict(nranks=0, ranks=(0,)),
               dict(nranks=33, ranks=tuple(range(33))), dict(ranks=(0, 520)), dict(nslots=0), dict(stride=2), dict(nchains=0),
               dict(npad=128), dict(npad=193)):
        assert stat(**kw) == refused, kw
    for kw in (dict(trace_ptr=0), dict(pass_=-1), dict(pass_=8), dict(nprefix=0), dict(nprefix=33), dict(nslots=0),
               dict(stride=2), dict(nchains=0), dict(npad=128), dict(npad=193), dict(give_prefixes=False)):
        assert count(**kw) == refused, kw
    assert stat() == (0, False) and count() == (0, False)                    # and the well-formed calls run
