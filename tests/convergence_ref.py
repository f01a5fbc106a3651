"""numpy restatement of the convergence sums and statistics (include/smcmc.h, "split R-hat and multi-chain ESS of a saved
trace"; test helper, imported by the test modules), written from the definitions and sharing no code with the kernels or
with engine.py, and the exact sums and rounding bound the device reducer is judged against.

  sums                 the four outputs in doubles: per segment-chain loops, mean, explicit lagged products
  statistics           W, var_of_means, var_plus, rhat, rho, tau, ess, truncated from the sums
  exact_sums           the outputs in exact rational arithmetic
  check_rounding_bound |device - exact| against the bound derived below

The trace is x[slot][dim][chain].  Every chain is cut into S segments of L = nslots // S slots, segment s covering the
slots [r + s L, r + (s + 1) L), r = nslots - S L; M = S * nchains segment-chains.

The rounding bound.  Model of tests/truth.py: u = 2^-53, gamma_m = m u / (1 - m u), a factor 2 for the second-order
terms; nothing is tuned.  Per segment-chain, with y_t = x_t - centre (one rounding) and every sum over its slots:
  s1       L roundings touch a term (the subtraction, L - 1 additions):  |s1~ - s1| <= gamma_L sum |y|
  mean     one more, the division:                                        eps = gamma_(L+1) sum |y| / L
  z_t      = y_t - mean: the roundings of y_t and of z_t, and eps:        e_t = u (|y_t| + |z_t|) + eps
  within[k][d]   a product z_t z_(t-k) is off by |z_t| e_(t-k) + |z_(t-k)| e_t to first order; the n = M (L - k) fused
           multiply-adds and the additions of the partial sums put at most n + 1 roundings on a term:
           2 ( sum_m sum_t (|z_t| e_(t-k) + |z_(t-k)| e_t) + gamma_(n+1) sum |z_t z_(t-k)| )
  sum      M L terms, the subtraction and the additions:                  2 gamma_(ML+1) sum |y|
  sumsq_of_sums  s1^2 is off by 2 |s1| gamma_L sum |y|, then the square's rounding and M additions:
           2 ( sum_m 2 |s1_m| gamma_L sum_t |y_t| + gamma_(M+2) sum_m s1_m^2 )
  chain_sums     gamma_L sum |y| as above (already rigorous: no factor)
The sums of absolute values that scale a bound are taken in doubles and rounded DOWN by 2^-20 relative: an underestimate
keeps the bound honest.
"""
import importlib.util
import os
from fractions import Fraction

import numpy as np

LAGS = 64                    # SMCMC_AUTOCORR_LAGS of include/smcmc.h


def _truth_module():
    spec = importlib.util.spec_from_file_location("smcmc_truth", os.path.join(os.path.dirname(os.path.abspath(__file__)), "truth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_T = _truth_module()
gamma, U, F = _T.gamma, _T.U, _T.F


def layout(nslots, S):
    """(L, r): the segment length and the number of leading slots that are not read."""
    L = nslots // S
    return L, nslots - S * L


# ---- the restatement in doubles ----------------------------------------------------------------------------------------

def sums(x, S=2, centre=None):
    """x[slot][dim][chain] -> dict(sum[dim], sumsq_of_sums[dim], within[LAGS][dim], chain_sums[S][dim][chain], L, M)."""
    x = np.asarray(x, dtype=np.float64)
    nslots, dim, nchains = x.shape
    L, r = layout(nslots, S)
    c = np.zeros(dim) if centre is None else np.asarray(centre, dtype=np.float64)
    total, sumsq, within = np.zeros(dim), np.zeros(dim), np.zeros((LAGS, dim))
    chain_sums = np.zeros((S, dim, nchains))
    for s in range(S):
        for ch in range(nchains):
            for d in range(dim):
                y = x[r + s * L:r + (s + 1) * L, d, ch] - c[d]
                s1 = 0.0
                for v in y:
                    s1 += v
                z = y - s1 / L
                chain_sums[s, d, ch] = s1
                total[d] += s1
                sumsq[d] += s1 * s1
                for k in range(min(LAGS, L)):
                    within[k, d] += float(np.sum(z[k:] * z[:L - k]))
    return dict(sum=total, sumsq_of_sums=sumsq, within=within, chain_sums=chain_sums, L=L, M=S * nchains)


def statistics(total, sumsq_of_sums, within, L, M):
    """The statistics of the definition from the raw sums, one dimension at a time."""
    total, sumsq_of_sums, within = np.asarray(total), np.asarray(sumsq_of_sums), np.asarray(within)
    dim = total.size
    nlag = min(LAGS, L)
    nan = float("nan")
    out = dict(W=np.zeros(dim), var_of_means=np.zeros(dim), var_plus=np.zeros(dim), rhat=np.zeros(dim),
               rho=np.zeros((nlag, dim)), tau=np.zeros(dim), ess=np.zeros(dim), truncated=np.zeros(dim, dtype=bool))
    for d in range(dim):
        W = within[0, d] / (M * (L - 1))
        if M >= 2:
            vm = (sumsq_of_sums[d] / (L * L) - (total[d] / L) * (total[d] / L) / M) / (M - 1)
        else:
            vm = nan
        vp = (L - 1) / L * W + vm
        rhat = nan if (W == 0 or M < 2 or vp != vp or vp / W < 0) else float(np.sqrt(vp / W))
        rho = []
        for k in range(nlag):
            rho.append(nan if (vp != vp or vp == 0) else 1.0 - (W - within[k, d] / (M * L)) / vp)
        pairs = []
        truncated = True
        for j in range(nlag // 2):
            p = rho[2 * j] + rho[2 * j + 1]
            if p < 0:
                truncated = False
                break
            pairs.append(p)
        for j in range(1, len(pairs)):
            if pairs[j] > pairs[j - 1]:
                pairs[j] = pairs[j - 1]
        tau = -1.0 + 2.0 * sum(pairs)
        out["W"][d], out["var_of_means"][d], out["var_plus"][d], out["rhat"][d] = W, vm, vp, rhat
        out["rho"][:, d] = rho
        out["tau"][d], out["truncated"][d] = tau, truncated
        out["ess"][d] = nan if tau != tau else (float("inf") if tau == 0 else M * L / tau)
    return out


# ---- exact sums --------------------------------------------------------------------------------------------------------
# Every double is an integer over a power of two.  With y = Y / D (Y integers, D one power of two for the data set) and
# S1 = sum Y, z = y - s1 / L = Z / (L D) with Z = L Y - S1: all of it integers, put together as Python integers.

def _dyadic(a):
    """doubles -> (object array of Python ints, den) with a = ints / den exactly."""
    a = np.asarray(a, dtype=np.float64)
    pairs = [float(v).as_integer_ratio() for v in a.ravel()]
    den = max([q for _, q in pairs] + [1])
    ints = np.empty(len(pairs), dtype=object)
    for i, (p, q) in enumerate(pairs):
        ints[i] = p * (den // q)
    return ints.reshape(a.shape), den


def _isum(a):
    return sum(np.asarray(a, dtype=object).ravel().tolist(), 0)


def exact_sums(x, S=2, centre=None):
    """The outputs as Fractions (object arrays of the shapes of `sums`), from integer arithmetic."""
    x = np.asarray(x, dtype=np.float64)
    nslots, dim, nchains = x.shape
    L, r = layout(nslots, S)
    X, dx = _dyadic(x[r:])
    C, dc = _dyadic(np.zeros(dim) if centre is None else centre)
    D = max(dx, dc)
    Y = X * (D // dx) - (C * (D // dc))[None, :, None]                 # [S L][dim][chain], y = Y / D
    total = np.empty(dim, dtype=object)
    sumsq = np.empty(dim, dtype=object)
    within = np.empty((LAGS, dim), dtype=object)
    chain_sums = np.empty((S, dim, nchains), dtype=object)
    for d in range(dim):
        t_sum, t_sq, t_w = 0, 0, [0] * LAGS
        for s in range(S):
            Ys = Y[s * L:(s + 1) * L, d, :]                            # [L][chain]
            S1 = Ys.sum(axis=0)                                        # object sums: exact
            Z = Ys * L - S1[None, :]
            t_sum += _isum(S1)
            t_sq += _isum(S1 * S1)
            big = max(abs(v) for v in Z.ravel().tolist())
            if big * big * L * nchains < 2 ** 62:                      # small integers: the same sums in int64
                Z = Z.astype(np.int64)
            for k in range(min(LAGS, L)):
                t_w[k] += int(np.sum(Z[k:] * Z[:L - k]))
            for ch in range(nchains):
                chain_sums[s, d, ch] = Fraction(S1[ch], D)
        total[d] = Fraction(t_sum, D)
        sumsq[d] = Fraction(t_sq, D * D)
        for k in range(LAGS):
            within[k, d] = Fraction(t_w[k], L * L * D * D)
    return dict(sum=total, sumsq_of_sums=sumsq, within=within, chain_sums=chain_sums, L=L, M=S * nchains)


def bounds(x, S=2, centre=None):
    """The rounding bounds of the module docstring as Fractions: dict(sum[dim], sumsq_of_sums[dim], within[LAGS][dim],
    chain_sums[S][dim][chain])."""
    x = np.asarray(x, dtype=np.float64)
    nslots, dim, nchains = x.shape
    L, r = layout(nslots, S)
    M = S * nchains
    c = np.zeros(dim) if centre is None else np.asarray(centre, dtype=np.float64)
    down = 1.0 - 2.0 ** -20
    u = float(U)
    gL, gL1 = float(gamma(L)), float(gamma(L + 1))
    b_sum = np.empty(dim, dtype=object)
    b_sq = np.empty(dim, dtype=object)
    b_w = np.empty((LAGS, dim), dtype=object)
    b_cs = np.empty((S, dim, nchains), dtype=object)
    for d in range(dim):
        abs_y_all, sq_a, sq_b = 0.0, 0.0, 0.0
        first = np.zeros(LAGS)                                         # sum (|z_t| e_(t-k) + |z_(t-k)| e_t)
        prod = np.zeros(LAGS)                                          # sum |z_t z_(t-k)|
        for s in range(S):
            y = x[r + s * L:r + (s + 1) * L, d, :] - c[d]              # [L][chain]
            ay = np.abs(y)
            say = ay.sum(axis=0) * down                                # sum_t |y_t| per chain
            s1 = y.sum(axis=0)
            z = y - s1[None, :] / L
            az = np.abs(z) * down
            e = u * (ay * down + az) + (gL1 * say / L)[None, :]
            abs_y_all += float(say.sum())
            sq_a += float(np.sum(2.0 * np.abs(s1) * down * gL * say))
            sq_b += float(np.sum(s1 * s1)) * down
            for k in range(min(LAGS, L)):
                first[k] += float(np.sum(az[k:] * e[:L - k] + az[:L - k] * e[k:])) * down
                prod[k] += float(np.sum(az[k:] * az[:L - k])) * down
            for ch in range(nchains):
                b_cs[s, d, ch] = gamma(L) * F(say[ch])
        b_sum[d] = 2 * gamma(M * L + 1) * F(abs_y_all * down)
        b_sq[d] = 2 * (F(sq_a * down) + gamma(M + 2) * F(sq_b * down))
        for k in range(LAGS):
            n = M * (L - k)
            b_w[k, d] = 2 * (F(first[k]) + gamma(n + 1) * F(prod[k])) if k < L else Fraction(0)
    return dict(sum=b_sum, sumsq_of_sums=b_sq, within=b_w, chain_sums=b_cs)


def check_rounding_bound(got, x, S=2, centre=None, tag="", exact=None):
    """got: dict with sum, sumsq_of_sums, within and optionally chain_sums (doubles).  Asserts every value within its
    bound of the exact one and returns the worst |error| / bound."""
    exact = exact_sums(x, S, centre) if exact is None else exact
    bound = bounds(x, S, centre)
    worst = 0.0
    for name in ("sum", "sumsq_of_sums", "within", "chain_sums"):
        if name not in got or got[name] is None:
            continue
        g, t, b = np.asarray(got[name]), exact[name], bound[name]
        assert g.shape == t.shape, (tag, name, g.shape, t.shape)
        for idx in np.ndindex(*t.shape):
            v = float(g[idx])
            assert np.isfinite(v), (tag, name, idx, v)
            err = abs(F(v) - t[idx])
            assert err <= b[idx], (tag, name, idx, float(err), float(b[idx]))
            if b[idx]:
                worst = max(worst, float(err / b[idx]))
    return worst


# ---- the pooled lagged sums of one chain (smcmc_autocorrelation_sums), for the comparison of the two reducers ----------

def exact_pooled_lagged(x, centre=None):
    """x[slot][dim][1 chain]: (lagged[LAGS][dim] as Fractions, abs[LAGS][dim] doubles rounded down) of
    lagged[k] = sum_{t >= k} y_t y_(t-k), and the exact within[k] of the same chain rebuilt from them:
    sum (y_t - m)(y_(t-k) - m) = lagged[k] - m (sum_{t >= k} y_t + sum_{t < L-k} y_t) + (L - k) m^2, m the chain's mean."""
    x = np.asarray(x, dtype=np.float64)
    nslots, dim, nchains = x.shape
    assert nchains == 1
    X, dx = _dyadic(x[:, :, 0])
    C, dc = _dyadic(np.zeros(dim) if centre is None else centre)
    D = max(dx, dc)
    Y = X * (D // dx) - (C * (D // dc))[None, :]
    lagged = np.empty((LAGS, dim), dtype=object)
    rebuilt = np.empty((LAGS, dim), dtype=object)
    absl = np.zeros((LAGS, dim))
    y = x[:, :, 0] - (0.0 if centre is None else np.asarray(centre)[None, :])
    for d in range(dim):
        col = Y[:, d]
        m = Fraction(_isum(col), D * nslots)
        for k in range(LAGS):
            if k >= nslots:
                lagged[k, d], rebuilt[k, d] = Fraction(0), Fraction(0)
                continue
            lagged[k, d] = Fraction(_isum(col[k:] * col[:nslots - k]), D * D)
            edges = Fraction(_isum(col[k:]) + _isum(col[:nslots - k]), D)
            rebuilt[k, d] = lagged[k, d] - m * edges + (nslots - k) * m * m
            absl[k, d] = float(np.sum(np.abs(y[k:, d] * y[:nslots - k, d]))) * (1.0 - 2.0 ** -20)
    return lagged, absl, rebuilt
