"""The numpy restatement of TestMarginalization.C (tests/marginal_ref.py) on hand-counted cases, the host-side Marginals
class, and the declaration of the two device entry points.  Nothing here launches a kernel."""
import importlib.util
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_spec = importlib.util.spec_from_file_location("smcmc_marginal_ref", os.path.join(HERE, "marginal_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)


# ---- the restatement ---------------------------------------------------------------------------------------------------

def test_bin_rule_on_hand_counted_values():
    # 4 bins over [0, 8): width 2
    inf, nan = np.inf, np.nan
    x = [0.0, 1.999, 2.0, 3.0, 4.0, 7.999, 8.0, -0.001, 9.0, nan, inf, -inf, -0.0]
    want = [1, 1, 2, 2, 3, 4, 5, 0, 5, 5, 5, 0, 1]
    assert R.bin_index(x, 4, 0.0, 8.0).tolist() == want
    # one bin: everything inside lands in bin 1
    assert R.bin_index([-1.0, 0.0, 0.5, 1.0], 1, 0.0, 1.0).tolist() == [0, 1, 1, 2]
    # an axis that does not start at zero: 10 bins over [-1, 1), edges at -1 + 0.2 k
    assert R.bin_index([-1.0, -0.5, 0.0, 0.5, 0.99], 10, -1.0, 1.0).tolist() == [1, 3, 6, 8, 10]


def test_bin_rule_sends_a_quotient_that_rounds_up_to_the_overflow():
    """The formula's own behaviour, kept: x just below hi whose quotient n (x - lo) / (hi - lo) rounds up to n (or, the
    product having been rounded up before the division, an ulp beyond it) gets n + 1."""
    rng = np.random.default_rng(7)
    hits = 0
    for _ in range(2000):
        lo = rng.normal() * 10.0
        hi = lo + rng.uniform(0.1, 20.0)
        x = np.nextafter(hi, -np.inf)
        b = int(R.bin_index([x], 100, lo, hi)[0])
        q = np.float64(100) * (x - lo) / (hi - lo)
        assert q < 101.0 and b == (101 if q >= 100.0 else 100)
        hits += b == 101
    assert hits > 0          # about one axis in five


def test_hist1_equals_numpy_histogram_clear_of_the_edges():
    rng = np.random.default_rng(3)
    n, lo, hi = 20, -4.0, 6.0                      # width 0.5: edges are exact doubles
    centres = lo + 0.5 * (np.arange(n) + 0.5)
    x = (rng.choice(centres, size=(7, 2, 31)) + rng.uniform(-0.2, 0.2, size=(7, 2, 31)))
    got = R.hist1(x, n, [lo, lo], [hi, hi])
    for d in range(2):
        want, _ = np.histogram(x[:, d, :].ravel(), bins=n, range=(lo, hi))
        assert got[d, 0] == 0 and got[d, n + 1] == 0
        assert np.array_equal(got[d, 1:n + 1], want.astype(np.uint64))
    assert got.dtype == np.uint64


def test_hist2_tables_on_a_hand_counted_trace():
    # two slots, two dimensions, three chains; 2 bins over [0, 2) in both
    x = np.array([[[0.5, 1.5, 2.5], [0.5, 0.5, -1.0]],
                  [[1.0, 0.0, np.nan], [1.5, 1.5, 1.5]]])
    h = R.hist2(x, [0, 1], 2, [0.0, 0.0], [2.0, 2.0])
    b0 = [1, 2, 3, 2, 1, 3]                          # bins of dimension 0 (slot-major)
    b1 = [1, 1, 0, 2, 2, 2]
    want = np.zeros((4, 4), dtype=np.uint64)
    for a, b in zip(b0, b1):
        want[a, b] += 1
    assert np.array_equal(h[0, 1], want) and np.array_equal(h[1, 0], want.T)
    assert np.array_equal(np.diag(h[0, 0]), R.hist1(x, 2, [0.0, 0.0], [2.0, 2.0])[0])
    assert h[0, 0].sum() == 6 and np.count_nonzero(h[0, 0] - np.diag(np.diag(h[0, 0]))) == 0
    # the list may repeat and reorder dimensions: positions index the tables
    g = R.hist2(x, [1, 0, 1], 2, [0.0, 0.0, 0.0], [2.0, 2.0, 2.0])
    assert np.array_equal(g[1, 0], want) and np.array_equal(g[0, 2], g[0, 0])


def test_ranges_subsample_and_ignore_nan():
    x = np.arange(2 * 3 * 10, dtype=np.float64).reshape(10, 2, 3)
    x[0, 0, 0] = np.nan
    x[9, 1, 2] = 1000.0
    lo, hi = R.ranges(x, 1)
    assert lo.tolist() == [1.0, 3.0] and hi.tolist() == [56.0, 1000.0]
    lo, hi = R.ranges(x, 4)                           # slots 0, 4, 8
    assert lo.tolist() == [1.0, 3.0] and hi.tolist() == [50.0, 53.0]
    lo, hi = R.ranges(x, 11)                          # slot 0 alone
    assert lo.tolist() == [1.0, 3.0] and hi.tolist() == [2.0, 5.0]
    lo, hi = R.ranges(np.full((2, 1, 2), np.nan), 1)
    assert lo[0] == np.inf and hi[0] == -np.inf


def _macro_loop_entries(entries):
    """The macro's loop (:54-62) with its int entry: the entries it visits."""
    out, entry = [], 0
    while entry < entries:
        out.append(entry)
        entry = int(entry + 0.001 * entries)          # entry += 0.001*entries on an int
        entry += 1
    return out


@pytest.mark.parametrize("entries", [1, 999, 1000, 1001, 123456])
def test_macro_stride_is_the_macro_loop(smcmc, entries):
    visited = _macro_loop_entries(entries)
    for stride in (R.macro_stride(entries), smcmc.Marginals.macro_sample_stride(entries)):
        assert visited == list(range(0, entries, stride))


def test_macro_restatement_holds_together():
    rng = np.random.default_rng(11)
    x = rng.normal(size=(30, 12, 9)) * np.arange(1, 13)[None, :, None]
    m = R.macro(x)
    assert m["dims"].tolist() == list(range(10))
    assert m["counts1"].shape == (12, 102) and m["counts2"].shape == (10, 10, 52, 52)
    assert np.all(m["counts1"].sum(axis=1) == 30 * 9) and np.all(m["counts2"].sum(axis=(2, 3)) == 30 * 9)
    assert m["abs"] == (x.min(), x.max())             # stride 1 at 30 entries: the full range
    # absMax itself is not below the axis' end: it is counted as overflow (the macro loses it the same way)
    assert m["counts1"][:, 101].sum() == 1 and m["counts1"][:, 0].sum() == 0
    w = m["hi"] - m["lo"]
    assert np.array_equal(m["lo2"], (m["lo"] - 0.05 * w)[:10]) and np.array_equal(m["hi2"], (m["hi"] + 0.05 * w)[:10])


# ---- the host-side class ----------------------------------------------------------------------------------------------

def _marginals(smcmc, counts1, nchains=4, lo1=(0.0,), hi1=(10.0,)):
    counts1 = np.asarray(counts1, dtype=np.uint64)
    dim = counts1.shape[0]
    return smcmc.Marginals(np.zeros(dim), np.ones(dim), 5, nchains, lo1=np.resize(lo1, dim), hi1=np.resize(hi1, dim),
                           counts1=counts1)


def test_marginals_add_and_refuse(smcmc):
    a = _marginals(smcmc, [[1, 2, 3, 4], [0, 5, 5, 0]])
    b = _marginals(smcmc, [[4, 3, 2, 1], [1, 1, 1, 1]], nchains=6)
    s = a + b
    assert s.counts1.tolist() == [[5, 5, 5, 5], [1, 6, 6, 1]] and s.counts1.dtype == np.uint64
    assert s.nchains == 10 and s.nslots == 5 and s.n1 == 2
    with pytest.raises(ValueError):
        a + _marginals(smcmc, [[1, 2, 3, 4], [0, 5, 5, 0]], hi1=(11.0,))        # another axis
    with pytest.raises(ValueError):
        a + _marginals(smcmc, [[1, 2, 3, 4, 5], [0, 5, 5, 0, 0]])              # another number of bins
    c = _marginals(smcmc, [[1, 2, 3, 4], [0, 5, 5, 0]])
    c.lo = np.array([0.0, -1.0])
    with pytest.raises(ValueError):
        a + c                                                                    # other ranges
    c = _marginals(smcmc, [[1, 2, 3, 4], [0, 5, 5, 0]])
    c.nslots = 6
    with pytest.raises(ValueError):
        a + c
    # pair tables add too, and a different list of pair dimensions is refused
    kw = dict(lo2=[0.0, 0.0], hi2=[1.0, 1.0])
    p = smcmc.Marginals([0.0] * 3, [1.0] * 3, 5, 4, pair_dims=[0, 2], counts2=np.ones((2, 2, 3, 3)), **kw)
    q = smcmc.Marginals([0.0] * 3, [1.0] * 3, 5, 4, pair_dims=[0, 2], counts2=2 * np.ones((2, 2, 3, 3)), **kw)
    assert np.all((p + q).counts2 == 3) and (p + q).n2 == 1
    r = smcmc.Marginals([0.0] * 3, [1.0] * 3, 5, 4, pair_dims=[0, 1], counts2=np.ones((2, 2, 3, 3)), **kw)
    with pytest.raises(ValueError):
        p + r


def test_merge_ranges(smcmc):
    lo, hi = smcmc.Marginals.merge_ranges([([0.0, -3.0], [1.0, 2.0]), ([-1.0, -2.0], [0.5, 7.0]), ([0.5, 0.0], [9.0, 0.0])])
    assert lo.tolist() == [-1.0, -3.0] and hi.tolist() == [9.0, 7.0]
    a = smcmc.Marginals([0.0], [1.0], 1, 1)
    b = smcmc.Marginals([-2.0], [0.5], 1, 1)
    lo, hi = smcmc.Marginals.merge_ranges([a, b])
    assert lo.tolist() == [-2.0] and hi.tolist() == [1.0]


def test_quantile_and_interval_at_exact_positions(smcmc):
    # 4 bins of width 2.5 over [0, 10): underflow 8, bins 8 32 8 0, overflow 8: 64 points, every q below a dyadic fraction
    m = _marginals(smcmc, [[8, 8, 32, 8, 0, 8]])
    assert m.quantile(0, 1 / 16) == 0.0 and m.quantile(0, 1 / 8) == 0.0         # inside the underflow: it sits on lo
    assert m.quantile(0, 3 / 16) == 1.25                                        # half way through bin 1
    assert m.quantile(0, 1 / 4) == 2.5                                          # an edge
    assert m.quantile(0, 1 / 2) == 3.75
    assert m.quantile(0, 3 / 4) == 5.0
    assert m.quantile(0, 13 / 16) == 6.25
    assert m.quantile(0, 7 / 8) == 7.5                                          # bin 4 is empty: the first edge that reaches it
    assert m.quantile(0, 15 / 16) == 10.0 and m.quantile(0, 1.0) == 10.0        # inside the overflow: it sits on hi
    assert m.interval(0, 0.625) == (1.25, 6.25)
    assert m.interval(0, 0.0) == (3.75, 3.75)
    d = m.density(0)
    assert d.tolist() == [8 / 160.0, 32 / 160.0, 8 / 160.0, 0.0]                 # counts / (64 points x 2.5)
    assert m.edges1.tolist() == [[0.0, 2.5, 5.0, 7.5, 10.0]]


def test_macro_ranges(smcmc):
    m = smcmc.Marginals([-1.0, 2.0, 0.0], [1.0, 6.0, 0.5], 3, 2)
    (amin, amax), (lo2, hi2) = m.macro_ranges()
    assert (amin, amax) == (-1.0, 6.0)
    assert np.array_equal(lo2, np.array([-1.0 - 0.05 * 2.0, 2.0 - 0.05 * 4.0, 0.0 - 0.05 * 0.5]))
    assert np.array_equal(hi2, np.array([1.0 + 0.05 * 2.0, 6.0 + 0.05 * 4.0, 0.5 + 0.05 * 0.5]))
    (_, _), (lo2, hi2) = m.macro_ranges(pair_dims=[2, 0])
    assert np.array_equal(lo2, np.array([0.0 - 0.05 * 0.5, -1.0 - 0.05 * 2.0]))
    assert np.array_equal(hi2, np.array([0.5 + 0.05 * 0.5, 1.0 + 0.05 * 2.0]))
    # the macro's starting values bound absMin / absMax
    far = smcmc.Marginals([1e30], [-1e30], 1, 1)
    assert far.macro_ranges()[0] == (1e20, -1e20)
    # the same numbers as the restatement
    rng = np.random.default_rng(5)
    lo = rng.normal(size=12)
    hi = lo + rng.uniform(0.1, 3.0, size=12)
    (a, b), (l2, h2) = smcmc.Marginals(lo, hi, 1, 1).macro_ranges()
    (ra, rb), (rl2, rh2) = R.macro_axes(lo, hi, np.arange(10))
    assert (a, b) == (ra, rb) and np.array_equal(l2, rl2) and np.array_equal(h2, rh2)


# ---- the declaration -------------------------------------------------------------------------------------------------

def _declaration(name):
    text = open(os.path.join(ROOT, "include", "smcmc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, "%s is not declared in include/smcmc.h" % name
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_entry_points_are_declared_with_the_documented_arguments(smcmc):
    assert _declaration("smcmc_trace_ranges") == [
        "const double* trace_device", "int nslots", "int dim", "int dim_stride", "int nchains", "int nchains_padded",
        "int sample_stride", "double* lo", "double* hi", "void* stream"]
    assert _declaration("smcmc_marginal_histograms") == [
        "const double* trace_device", "int nslots", "int dim", "int dim_stride", "int nchains", "int nchains_padded",
        "int n1", "const double* lo1", "const double* hi1", "uint64_t* counts1",
        "int npair_dims", "const int32_t* pair_dims", "int n2", "const double* lo2", "const double* hi2",
        "uint64_t* counts2", "void* stream"]
    for name, nargs in (("smcmc_trace_ranges", 10), ("smcmc_marginal_histograms", 17)):
        assert len(smcmc.SIGNATURES[name][1]) == nargs
    text = open(os.path.join(ROOT, "include", "smcmc.h")).read()
    limits = {k: int(v) for k, v in re.findall(r"#define SMCMC_MARGINAL_MAX_(\w+) (\d+)", text)}
    # the macro's own shape is admitted, and at least 256 bins in 1-D
    assert limits["BINS1"] >= 256 and limits["BINS2"] >= 50 and limits["PAIR_DIMS"] >= 10
    _capi = smcmc._capi
    assert (_capi.MARGINAL_MAX_BINS1, _capi.MARGINAL_MAX_BINS2, _capi.MARGINAL_MAX_PAIR_DIMS) == \
        (limits["BINS1"], limits["BINS2"], limits["PAIR_DIMS"])


def test_entry_points_refuse_bad_arguments_before_looking_for_a_device(smcmc):
    """The argument checks come first, so they answer SMCMC_ERR_INVALID on a machine without a GPU as well."""
    import ctypes as C
    lib = smcmc.load()
    dp = C.POINTER(C.c_double)
    lo, hi = np.zeros(2), np.ones(2)
    fake = C.c_void_p(4096)                                                    # never dereferenced: the call is refused
    assert lib.smcmc_trace_ranges(None, 4, 2, 2, 64, 64, 1, lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), None) == 1
    assert lib.smcmc_trace_ranges(fake, 4, 2, 2, 64, 64, 0, lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), None) == 1
    assert lo.tolist() == [0.0, 0.0] and hi.tolist() == [1.0, 1.0]
    c1 = np.full((2, 6), 7, dtype=np.uint64)
    st = lib.smcmc_marginal_histograms(fake, 4, 2, 2, 64, 64, 4, hi.ctypes.data_as(dp), lo.ctypes.data_as(dp),
                                       c1.ctypes.data_as(C.POINTER(C.c_uint64)), 0, None, 0, None, None, None, None)
    assert st == 1 and np.all(c1 == 7)                                          # lo > hi: an empty axis
