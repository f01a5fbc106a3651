"""TestMarginalization.C restated in numpy for the tests of the device histograms (smcmc_trace_ranges,
smcmc_marginal_histograms).  Shares no code with the product.  Traces are x[slot][dim][chain] (live chains only).

The bin rule (include/smcmc.h; ROOT's fixed-width axis as the engine defines it, not checked against ROOT):
    bin(x; n, lo, hi) = 0 if x < lo, n + 1 if !(x < hi), else 1 + (int)(n * (x - lo) / (hi - lo))
evaluated in IEEE double, one rounding per operation, which is what numpy's elementwise operators do."""
import numpy as np

MACRO_BINS1, MACRO_BINS2, MACRO_PAIR_DIMS = 100, 50, 10      # TestMarginalization.C:73, 88-89, 39-43


def bin_index(x, n, lo, hi):
    """Bin numbers (int64, 0 .. n + 1) of the doubles x on the axis of n bins over [lo, hi)."""
    x = np.asarray(x, dtype=np.float64)
    lo, hi = np.float64(lo), np.float64(hi)
    out = np.empty(x.shape, dtype=np.int64)
    under = x < lo
    over = ~(x < hi)                                  # NaN lands here
    inside = ~under & ~over
    out[under] = 0
    out[over] = n + 1
    with np.errstate(all="ignore"):
        q = np.float64(n) * (x[inside] - lo) / (hi - lo)
    out[inside] = 1 + np.trunc(q).astype(np.int64)
    return out


def macro_stride(entries):
    """The stride of `for (entry = 0; entry < entries; ++entry) { ...; entry += 0.001*entries; }` on an int entry."""
    return 1 + int(0.001 * entries)


def ranges(x, stride):
    """(lo[dim], hi[dim]) over the live chains of slots 0, stride, 2 stride, ...; a NaN never replaces a value
    (std::min / std::max); without any comparable value lo = +inf, hi = -inf."""
    s = np.asarray(x, dtype=np.float64)[::stride]
    lo = np.fmin.reduce(np.fmin.reduce(s, axis=2, initial=np.inf), axis=0, initial=np.inf)
    hi = np.fmax.reduce(np.fmax.reduce(s, axis=2, initial=-np.inf), axis=0, initial=-np.inf)
    return lo, hi


def hist1(x, n, lo, hi):
    """counts[dim][n + 2] (uint64): every slot of every chain of dimension d on the axis (n, lo[d], hi[d])."""
    x = np.asarray(x, dtype=np.float64)
    dim = x.shape[1]
    out = np.zeros((dim, n + 2), dtype=np.uint64)
    for d in range(dim):
        out[d] = np.bincount(bin_index(x[:, d, :].ravel(), n, lo[d], hi[d]), minlength=n + 2).astype(np.uint64)
    return out


def hist2(x, dims, n, lo, hi):
    """counts[P][P][n + 2][n + 2] (uint64) for the list `dims` of P dimensions with axes (n, lo[p], hi[p]):
    table (p, q)[a][b] counts the points with bin a in dims[p] and bin b in dims[q]."""
    x = np.asarray(x, dtype=np.float64)
    P, nb = len(dims), n + 2
    idx = [bin_index(x[:, dims[p], :].ravel(), n, lo[p], hi[p]) for p in range(P)]
    out = np.zeros((P, P, nb, nb), dtype=np.uint64)
    for p in range(P):
        for q in range(P):
            out[p, q] = np.bincount(idx[p] * nb + idx[q], minlength=nb * nb).reshape(nb, nb).astype(np.uint64)
    return out


def macro_axes(lo, hi, dims):
    """((absMin, absMax), (lo2[P], hi2[P])): TestMarginalization.C:52-53, 59-60 and :85-89."""
    abs_min = min(1e20, float(np.min(lo)))
    abs_max = max(-1e20, float(np.max(hi)))
    dims = np.asarray(dims, dtype=np.int64)
    r = 0.05 * (hi[dims] - lo[dims])
    return (abs_min, abs_max), (lo[dims] - r, hi[dims] + r)


def macro(x):
    """The macro's three passes with its own constants: dict of lo, hi, abs (absMin, absMax), counts1, dims, lo2, hi2,
    counts2."""
    x = np.asarray(x, dtype=np.float64)
    nslots, dim, _ = x.shape
    lo, hi = ranges(x, macro_stride(nslots))
    dims = np.arange(min(dim, MACRO_PAIR_DIMS))
    (abs_min, abs_max), (lo2, hi2) = macro_axes(lo, hi, dims)
    counts1 = hist1(x, MACRO_BINS1, np.full(dim, abs_min), np.full(dim, abs_max))
    counts2 = hist2(x, dims, MACRO_BINS2, lo2, hi2)
    return dict(lo=lo, hi=hi, abs=(abs_min, abs_max), counts1=counts1, dims=dims, lo2=lo2, hi2=hi2, counts2=counts2)
