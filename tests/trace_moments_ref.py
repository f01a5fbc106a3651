"""numpy restatements of the reference's MakeCovariance.C and CholeskyChain.C (test helper, imported by the test
modules), sharing no code with the kernels, and the exact sums the device reducer is judged against.

  make_covariance      MakeCovariance.C:63-89 on an [entries][dim] array
  cholesky_chain       CholeskyChain.C:18-66 with the engine's draws in place of gRandom->Gaus (oracle.cholesky,
                       oracle.draw_block, oracle.det_normal_pair); a numpy multiply followed by an add is the un-fused
                       IEEE pair of :58
  exact_sums           sum y and sum y y^T of y = x - centre in exact integers
  gaussian_round_trip  the statistical assertion of the Cholesky round trip
"""
from fractions import Fraction

import numpy as np

STREAM_CHOLESKY = 4          # SMCMC_STREAM_CHOLESKY of include/smcmc_detmath.h


def make_covariance(accepted):
    """MakeCovariance.C:63-89 on accepted[entries][dim].  The loops over the entries (:64) and over i (:67) are the
    macro's; the loop over j (:70-73) is one numpy row operation, the same multiply and the same add per element.
    TH2D::Fill and TProfile::Fill add in double.  Returns avg (:77), covariance (:84), the raw sums before them, and the
    TProfile's mean and "S" spread (:58-60, 68: sqrt(E[x^2] - E[x]^2))."""
    accepted = np.asarray(accepted, dtype=np.float64)
    entries, dim = accepted.shape
    avg = np.zeros(dim)
    cov = np.zeros((dim, dim))
    for e in range(entries):
        a = accepted[e]
        for i in range(dim):
            avg[i] += a[i]
            cov[i] += a[i] * a
    total, sumsq = avg.copy(), cov.copy()
    for i in range(dim):
        avg[i] /= entries
    for i in range(dim):
        for j in range(dim):
            v = cov[i, j]
            v = v / entries - avg[i] * avg[j]
            cov[i, j] = v
    profile_mean = total / entries
    spread = np.sqrt(np.abs(np.diag(sumsq) / entries - profile_mean * profile_mean))
    return dict(avg=avg, covariance=cov, sum=total, sumsq=sumsq, mean=profile_mean, spread=spread)


def entry_normals(oracle, seed, chain, slot, dim, stream=STREAM_CHOLESKY):
    """r_0 .. r_(dim-1) of one entry: Philox block b of counter (b, chain, slot) gives normals 4b .. 4b + 3, words
    (0, 1) and (2, 3) one pair each."""
    nb = (dim + 3) // 4
    w = np.array([oracle.draw_block(seed, chain, slot, b, stream) for b in range(nb)], dtype=np.float64)   # [nb][4]
    a0, a1 = oracle.det_normal_pair(w[:, 0], w[:, 1])
    b0, b1 = oracle.det_normal_pair(w[:, 2], w[:, 3])
    return np.stack([a0, a1, b0, b1], axis=1).ravel()[:dim]


def cholesky_chain(oracle, mean, covariance, nslots, nchains, seed, chain_offset=0):
    """(trace[nslots][dim][nchains], U) of CholeskyChain.C: U of :39-46 (None and None when it fails, where the macro
    exits), then per entry accepted = mean and, i ascending, accepted[j] += r_i * U(i, j) (:53-60)."""
    mean = np.asarray(mean, dtype=np.float64)
    dim = mean.size
    ok, U = oracle.cholesky(np.asarray(covariance, dtype=np.float64))
    if not ok:
        return None, None
    r = np.empty((nslots, nchains, dim))
    for t in range(nslots):
        for c in range(nchains):
            r[t, c] = entry_normals(oracle, seed, chain_offset + c, t, dim)
    accepted = np.empty((nslots, nchains, dim))
    accepted[:] = mean
    for i in range(dim):
        step = r[:, :, i, None] * U[i][None, None, :]
        accepted = accepted + step
    return np.ascontiguousarray(accepted.transpose(0, 2, 1)), U


# ---- exact sums --------------------------------------------------------------------------------------------------------
# y = x - centre exactly is the pair (hi, lo) of doubles of the error-free subtraction; every double of the pair is an
# integer multiple of 2^emin; cut into signed limbs of 16 bits the sums of limb products over up to 2^20 entries stay
# below 2^53, so a float64 matrix product adds them exactly, and Python integers put the limbs together.

def _two_diff(a, b):
    """(s, e) with a - b = s + e exactly (Knuth's TwoSum on a and -b)."""
    s = a - b
    bb = s - a
    e = (a - (s - bb)) - (b + bb)
    return s, e


def _limbs(parts, emin, nlimbs):
    out = np.zeros((nlimbs,) + parts[0].shape)
    for d in parts:
        t = np.ldexp(d, -emin)
        for k in range(nlimbs - 1, -1, -1):
            q = np.trunc(np.ldexp(t, -16 * k))
            out[k] += q
            t = t - np.ldexp(q, 16 * k)
        assert not t.any()
    return out


def exact_sums(x, centre=None):
    """x[entries][dim] doubles: (total[dim], gram[dim][dim]) as Fractions (object arrays) of y = x - centre, exactly,
    and (abs_total, abs_gram): sum |y| and sum |y_i y_j| as doubles rounded DOWN by 2^-20 relative (they only scale
    the error bound, so an underestimate keeps the bound honest)."""
    x = np.asarray(x, dtype=np.float64)
    entries, dim = x.shape
    assert entries <= 2 ** 19
    c = np.zeros(dim) if centre is None else np.asarray(centre, dtype=np.float64)
    hi, lo = _two_diff(x, np.broadcast_to(c, x.shape))
    nz = np.concatenate([hi[hi != 0].ravel(), lo[lo != 0].ravel()])
    if nz.size == 0:
        zero = np.full((dim, dim), Fraction(0), dtype=object)
        return np.full(dim, Fraction(0), dtype=object), zero, np.zeros(dim), np.zeros((dim, dim))
    _, e = np.frexp(nz)
    emin, emax = int(e.min()) - 53, int(e.max())
    nlimbs = (emax - emin) // 16 + 2
    L = _limbs([hi, lo], emin, nlimbs)                             # [nlimbs][entries][dim], |limb| <= 2^17
    flat = L.transpose(1, 0, 2).reshape(entries, nlimbs * dim)
    P = (flat.T @ flat).reshape(nlimbs, dim, nlimbs, dim)          # exact: < 2^34 * 2^19
    S = flat.sum(axis=0).reshape(nlimbs, dim)
    gram = np.zeros((dim, dim), dtype=object)
    total = np.zeros(dim, dtype=object)
    for a in range(nlimbs):
        total = total + (S[a].astype(np.int64).astype(object) << (16 * a))
        for b in range(nlimbs):
            gram = gram + (P[a, :, b, :].astype(np.int64).astype(object) << (16 * (a + b)))
    scale = Fraction(2) ** emin
    to_fraction = np.frompyfunc(lambda v, s: Fraction(int(v)) * s, 2, 1)
    ay = np.abs(hi + lo)
    down = 1.0 - 2.0 ** -20
    return to_fraction(total, scale), to_fraction(gram, scale * scale), ay.sum(axis=0) * down, (ay.T @ ay) * down


def entries_of(trace):
    """trace[slot][dim][chain] -> [entries][dim], slots outermost as a tree written step by step has them."""
    t = np.asarray(trace)
    return np.ascontiguousarray(t.transpose(0, 2, 1).reshape(-1, t.shape[1]))


def _truth_module():
    """tests/truth.py: u = 2^-53 and gamma_m = m u / (1 - m u), the only constants of the bound."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("smcmc_truth", os.path.join(os.path.dirname(os.path.abspath(__file__)), "truth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gamma = _truth_module().gamma


def check_rounding_bound(total, sumsq, x, centre, tag=""):
    """|error| <= 2 gamma_m sum |y_i y_j| with m = terms + 2 (the two roundings of y in a product, one rounding per fused
    multiply-add), and m = terms + 1 for the plain sum (tests/truth.py has the model and the factor 2).  Returns the
    worst |error| / bound."""
    t_total, t_gram, a_total, a_gram = exact_sums(x, centre)
    entries, dim = np.shape(x)
    worst = 0.0
    for i in range(dim):
        err = abs(Fraction(*float(total[i]).as_integer_ratio()) - t_total[i])
        bound = 2 * gamma(entries + 1) * Fraction(*float(a_total[i]).as_integer_ratio())
        assert err <= bound, (tag, "sum", i, float(err), float(bound))
        worst = max(worst, float(err / bound) if bound else 0.0)
        for j in range(dim):
            err = abs(Fraction(*float(sumsq[i, j]).as_integer_ratio()) - t_gram[i, j])
            bound = 2 * gamma(entries + 2) * Fraction(*float(a_gram[i, j]).as_integer_ratio())
            assert err <= bound, (tag, "sumsq", i, j, float(err), float(bound))
            worst = max(worst, float(err / bound) if bound else 0.0)
    return worst


def gaussian_round_trip(mean_est, cov_est, mean, sigma, n):
    """The moments of n independent draws of N(mean, sigma) within six standard errors: sqrt(sigma_ii / n) for a mean,
    sqrt((sigma_ii sigma_jj + sigma_ij^2) / n) for a covariance entry."""
    mean, sigma = np.asarray(mean), np.asarray(sigma)
    d = np.diag(sigma)
    assert np.all(np.abs(np.asarray(mean_est) - mean) <= 6.0 * np.sqrt(d / n)), np.abs(mean_est - mean) / np.sqrt(d / n)
    se = np.sqrt((np.outer(d, d) + sigma * sigma) / n)
    assert np.all(np.abs(np.asarray(cov_est) - sigma) <= 6.0 * se), np.max(np.abs(cov_est - sigma) / se)


def random_spd(dim, seed, lo=1e-3, hi=1e3):
    """A random symmetric positive definite matrix whose axes have scales lo .. hi (variances lo^2 .. hi^2)."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((dim, dim)))
    s = np.exp(rng.uniform(np.log(lo), np.log(hi), size=dim)) if dim > 1 else np.array([hi])
    a = (q * (s * s)[None, :]) @ q.T
    return 0.5 * (a + a.T)
