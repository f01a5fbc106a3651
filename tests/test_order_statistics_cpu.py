"""The order statistics of a saved trace, the parts that need no device: the order of include/smcmc_order_key.h through
its two host entry points, the refusals of smcmc_trace_digit_counts and smcmc_trace_order_statistics, the eight-pass
selection on the host (order_statistics_combined) against an integer sort, and TraceQuantiles.quantile against its own
formula and numpy's "linear" method."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UP, DP = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
INVALID, NO_DEVICE = 1, 7
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
NAMES = ("smcmc_order_key", "smcmc_order_value", "smcmc_order_chunk_entries", "smcmc_trace_digit_counts",
         "smcmc_trace_order_statistics")


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def key_truth(x):
    """the issue's definition, written out here independently of the package"""
    b = bits(x)
    k = b ^ np.where(b >> np.uint64(63) != 0, ONES, np.uint64(0x8000000000000000))
    return np.where(np.isnan(x), ONES, k)


def grid():
    tiny, big = 5e-324, 1.7976931348623157e308
    vals = [0.0, -0.0, tiny, -tiny, 2.2250738585072014e-308, -2.2250738585072014e-308, 2.225073858507201e-308,
            float("inf"), -float("inf"), big, -big, 1.0, -1.0, 76.0, -76.0, 1e-300, -1e-300, 3.5, -3.5, 1e300, -1e300]
    for v in (1.0, -1.0, 76.0, -76.0, 1e300, tiny * 7):
        vals += [np.nextafter(v, np.inf), np.nextafter(v, -np.inf)]
    rng = np.random.default_rng(5)
    vals += list(rng.normal(76.0, 6.0, 40)) + list(rng.normal(0.0, 1.0, 40)) + list(-np.exp(rng.normal(0.0, 30.0, 20)))
    x = np.array(vals, dtype=np.float64)
    nans = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF],
                    dtype=np.uint64).view(np.float64)
    return x, nans


def test_the_entry_points_are_declared_exported_and_bound(smcmc):
    text = open(os.path.join(ROOT, "include", "smcmc.h")).read()
    lib = C.CDLL(smcmc.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", text, flags=re.S)), name
        assert hasattr(lib, name) and name in smcmc.SIGNATURES
    for macro, value in (("SMCMC_ORDER_DIGIT_BITS", 8), ("SMCMC_ORDER_PASSES", 8), ("SMCMC_ORDER_MAX_RANKS", 32)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), text), macro
    lib = smcmc.load()
    assert lib.smcmc_version() >= 101
    chunk = lib.smcmc_order_chunk_entries()
    assert 64 <= chunk < 2 ** 31 and chunk % 64 == 0


def test_key_order_is_the_order_of_the_doubles(smcmc):
    lib = smcmc.load()
    x, nans = grid()
    keys = np.array([lib.smcmc_order_key(float(v)) for v in x], dtype=np.uint64)
    assert np.array_equal(keys, key_truth(x))
    assert np.array_equal(keys, smcmc.order_keys(x))
    back = np.array([lib.smcmc_order_value(int(k)) for k in keys])
    assert np.array_equal(bits(back), bits(x))                      # the round trip: the identity on non-NaN bits
    assert np.array_equal(bits(smcmc.order_values(keys)), bits(x))
    by_key = np.array([lib.smcmc_order_value(int(k)) for k in np.sort(keys)])
    assert np.array_equal(by_key, np.sort(x))                       # under ==
    # -0 before +0, which == does not tell apart
    assert lib.smcmc_order_key(-0.0) + 1 == lib.smcmc_order_key(0.0) == 0x8000000000000000
    zeros = by_key[by_key == 0.0]
    assert zeros.size == 2 and np.signbit(zeros[0]) and not np.signbit(zeros[1])
    # every NaN, of either sign: the all-ones key, after +inf, and back as the canonical quiet NaN
    for v in nans:
        assert lib.smcmc_order_key(float(v)) == 0xFFFFFFFFFFFFFFFF
    assert np.all(smcmc.order_keys(nans) == ONES)
    assert lib.smcmc_order_key(float("inf")) == 0xFFF0000000000000 < 0xFFFFFFFFFFFFFFFF
    assert lib.smcmc_order_key(-float("inf")) == 0x000FFFFFFFFFFFFF
    assert bits(lib.smcmc_order_value(0xFFFFFFFFFFFFFFFF))[0] == 0x7FF8000000000000
    assert bits(smcmc.order_values(np.array([ONES])))[0] == 0x7FF8000000000000
    mixed = np.concatenate([nans[:2], x])
    k = np.sort(np.array([lib.smcmc_order_key(float(v)) for v in mixed], dtype=np.uint64))
    assert np.all(k[-2:] == ONES) and np.all(k[:-2] < ONES)         # NaNs last


def _statistics(lib, trace=0x1000, nslots=4, dim=3, stride=5, nchains=130, npad=192, nranks=2, ranks=(0, 519),
                give_ranks=True, give_values=True):
    r = np.array(ranks, dtype=np.uint64)
    v = np.full((max(dim, 1), max(nranks, 1)), -7.0)
    b, e = np.full(v.shape, 7, dtype=np.uint64), np.full(v.shape, 7, dtype=np.uint64)
    st = lib.smcmc_trace_order_statistics(C.c_void_p(trace), nslots, dim, stride, nchains, npad, nranks,
                                          r.ctypes.data_as(UP) if give_ranks else None,
                                          v.ctypes.data_as(DP) if give_values else None, b.ctypes.data_as(UP),
                                          e.ctypes.data_as(UP), None)
    return st, bool(np.all(v == -7.0) and np.all(b == 7) and np.all(e == 7))


def _counts(lib, trace=0x1000, nslots=4, dim=3, stride=5, nchains=130, npad=192, pass_=1, nprefix=2, give_prefixes=True,
            give_counts=True):
    p = np.zeros((max(dim, 1), max(nprefix, 1)), dtype=np.uint64)
    c = np.full((max(dim, 1), max(nprefix, 1), 256), 7, dtype=np.uint64)
    st = lib.smcmc_trace_digit_counts(C.c_void_p(trace), nslots, dim, stride, nchains, npad, pass_, nprefix,
                                      p.ctypes.data_as(UP) if give_prefixes else None,
                                      c.ctypes.data_as(UP) if give_counts else None, None)
    return st, bool(np.all(c == 7))


def test_refusals_need_no_device(smcmc):
    """SMCMC_ERR_INVALID before a device is looked for, with nothing written; a well-formed call without a device is
    SMCMC_ERR_NO_DEVICE.  (The trace pointer is never followed here.)"""
    lib = smcmc.load()
    refused = (INVALID, True)
    many = tuple(range(33))
    for kw in (dict(trace=0), dict(give_ranks=False), dict(give_values=False), dict(nranks=0, ranks=(0,)),
               dict(nranks=33, ranks=many), dict(ranks=(0, 520)), dict(ranks=(2 ** 63, 0)), dict(nslots=0), dict(dim=0),
               dict(stride=2), dict(nchains=0), dict(npad=128), dict(npad=193), dict(npad=200), dict(dim=65536, stride=65536)):
        assert _statistics(lib, **kw) == refused, kw
    for kw in (dict(trace=0), dict(pass_=-1), dict(pass_=8), dict(nprefix=0), dict(nprefix=33), dict(nslots=0), dict(dim=0),
               dict(stride=2), dict(nchains=0), dict(npad=128), dict(npad=193), dict(give_counts=False),
               dict(give_prefixes=False), dict(dim=65536, stride=65536)):
        assert _counts(lib, **kw) == refused, kw
    import torch
    if torch.cuda.is_available():
        return                               # tests/test_gpu_order_statistics.py has the device's side
    assert _statistics(lib) == (NO_DEVICE, True)
    assert _statistics(lib, nranks=32, ranks=tuple(range(32))) == (NO_DEVICE, True)
    assert _statistics(lib, dim=291, stride=291) == (NO_DEVICE, True)        # not bounded by the kernels' largest dimension
    assert _counts(lib) == (NO_DEVICE, True)
    assert _counts(lib, pass_=0, give_prefixes=False) == (NO_DEVICE, True)   # pass 0 needs no prefixes
    assert _counts(lib, pass_=7, nprefix=32) == (NO_DEVICE, True)


def numpy_count_fn(keys):
    """smcmc_trace_digit_counts in numpy over keys[dim][n]"""
    def count_fn(p, prefixes):
        dim = keys.shape[0]
        R = 1 if prefixes is None else prefixes.shape[1]
        out = np.zeros((dim, R, 256), dtype=np.uint64)
        digit = ((keys >> np.uint64(56 - 8 * p)) & np.uint64(255)).astype(np.int64)
        for d in range(dim):
            for i in range(R):
                hit = np.ones(keys.shape[1], dtype=bool) if p == 0 else (keys[d] >> np.uint64(64 - 8 * p)) == prefixes[d, i]
                out[d, i] = np.bincount(digit[d][hit], minlength=256)
        return out
    return count_fn


def synthetic_rows():
    rng = np.random.default_rng(11)
    n = 1500
    rows = [rng.normal(76.0, 6.0, n),
            np.repeat(rng.normal(0.0, 1.0, n // 10), 10),                               # runs, as rejected steps leave them
            np.full(n, 3.25),
            np.concatenate([rng.normal(0.0, 1e-3, n - 4), [0.0, -0.0, 0.0, -0.0]]),
            (np.float64(76.0).view(np.uint64) + rng.integers(0, 256, n).astype(np.uint64)).view(np.float64)]
    odd = rng.normal(1.0, 2.0, n)
    odd[:8] = [np.inf, -np.inf, 5e-324, -5e-324, np.nan, -np.nan, 1e-310, np.inf]
    odd[8] = np.array([0xFFF8000000000001], dtype=np.uint64).view(np.float64)[0]
    rows.append(odd)
    return np.array(rows)


def sort_truth(keys, ranks):
    """(key, below, equal)[dim][R] from an integer sort"""
    s = np.sort(keys, axis=1)
    k = s[:, np.asarray(ranks, dtype=np.int64)]
    below = np.array([[np.searchsorted(s[d], k[d, r], side="left") for r in range(k.shape[1])] for d in range(k.shape[0])])
    upper = np.array([[np.searchsorted(s[d], k[d, r], side="right") for r in range(k.shape[1])] for d in range(k.shape[0])])
    return k, below.astype(np.uint64), (upper - below).astype(np.uint64)


def test_combined_selection_is_the_integer_sort(smcmc):
    x = synthetic_rows()
    keys = key_truth(x)
    n = x.shape[1]
    for ranks in ([0, n - 1], [n // 2], [7, 8], [5, 5], list(range(0, 32 * 40, 40)), [n - 1, 0, 3, 3, n // 2]):
        got = smcmc.order_statistics_combined(numpy_count_fn(keys), x.shape[0], n, ranks)
        k, below, equal = sort_truth(keys, ranks)
        assert np.array_equal(key_truth(got.values), k), ranks
        assert np.array_equal(bits(got.values), bits(smcmc.order_values(k))), ranks
        assert np.array_equal(got.below, below) and np.array_equal(got.equal, equal), ranks
        assert got.n == n and np.array_equal(got.ranks, np.array(ranks, dtype=np.uint64))
    # one copy of the pass-0 counts for all ranks is taken too
    one = numpy_count_fn(keys)
    got = smcmc.order_statistics_combined(lambda p, pre: one(p, pre) if p else one(0, None)[:, 0], x.shape[0], n, [1, 2, 3])
    assert np.array_equal(key_truth(got.values), sort_truth(keys, [1, 2, 3])[0])
    with pytest.raises(ValueError):
        smcmc.order_statistics_combined(one, x.shape[0], n, [n])
    with pytest.raises(ValueError):
        smcmc.order_statistics_combined(one, x.shape[0], n, list(range(33)))
    with pytest.raises(ValueError):
        smcmc.order_statistics_combined(one, x.shape[0], n + 1, [n])          # the counts hold fewer entries


def _quantiles_of(smcmc, x, q):
    """a TraceQuantiles over the rows of x from a sort"""
    n = x.shape[1]
    ranks = smcmc.quantile_ranks(n, q)
    s = np.sort(x, axis=1)
    z = np.zeros((x.shape[0], ranks.size), dtype=np.uint64)
    return smcmc.TraceQuantiles(ranks, s[:, ranks.astype(np.int64)], z, z + np.uint64(1), n), s


def test_quantile_is_the_stated_formula_and_numpys(smcmc):
    rng = np.random.default_rng(3)
    qs = (0.0, 0.025, 0.16, 0.5, 0.84, 0.975, 1.0, 1.0 / 3.0, 0.999)
    for n in (1, 2, 7, 1040, 4097):
        x = np.array([rng.normal(76.0, 6.0, n), np.exp(rng.normal(0.0, 3.0, n)), -np.exp(rng.normal(5.0, 2.0, n)),
                      rng.normal(0.0, 1.0, n)])
        tq, s = _quantiles_of(smcmc, x, qs)
        assert tq.ranks.size <= 2 * len(qs) and np.all(np.diff(tq.ranks.astype(np.int64)) > 0)
        for q in qs:
            h = (n - 1) * q
            lo, hi = int(np.floor(h)), int(np.ceil(h))
            want = s[:, lo] + (h - lo) * (s[:, hi] - s[:, lo])
            got = tq.quantile(q)
            assert got.shape == (4,) and np.array_equal(got, want), (n, q)
            ref = np.quantile(x, q, axis=1, method="linear")
            tol = 8.0 * 2.0 ** -52 * np.maximum(np.abs(s[:, lo]), np.abs(s[:, hi]))
            assert np.all(np.abs(got - ref) <= tol), (n, q, got - ref, tol)
        both = tq.quantile(qs)
        assert both.shape == (4, len(qs)) and np.array_equal(both[:, 3], tq.median)
        lo68, hi68 = tq.interval(0.68)
        assert np.array_equal(lo68, tq.quantile(0.16)) and np.array_equal(hi68, tq.quantile(0.84))
        lo95, hi95 = tq.interval(0.95)
        assert np.array_equal(lo95, tq.quantile(0.025)) and np.array_equal(hi95, tq.quantile(0.975))
        assert np.all(lo68 <= tq.median) and np.all(tq.median <= hi68)
        with pytest.raises(KeyError):
            tq.value_at(n)                                           # a rank that was not asked for
    shaped = smcmc.TraceQuantiles([0], np.arange(6.0).reshape(6, 1), np.zeros((6, 1)), np.ones((6, 1)), 1, shape=(2, 3))
    assert shaped.median.shape == (2, 3) and shaped.quantile([0.0, 1.0]).shape == (2, 3, 2)
    with pytest.raises(ValueError):
        smcmc.TraceQuantiles([0, 1], np.zeros((3, 1)), np.zeros((3, 1)), np.zeros((3, 1)), 5)
