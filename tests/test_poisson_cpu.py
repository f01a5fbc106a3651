"""The Poisson variate of the posterior-predictive check on the host (smcmc_poisson_draw, include/smcmc_poisson.h) and the
refusals of smcmc_predictive_check; no GPU.

  A1  smcmc_poisson_draw is tests/poisson_ref.py -- the header's comment restated in Python floats over the oracle's
      Philox block and the host smcmc_exp -- bit for bit: 4 096 draws per mean, and the invalid expectations
  A2  every draw is the index the exact cumulative distribution gives (tests/poisson_truth.py: mpmath at 256 bits, the
      exact mass function term by term), for every uniform farther than 1e-10 from both neighbouring thresholds, with no
      exception; at most 2 draws per mean may lie inside that band (expected: 20 000 * 2e-10 * thresholds <= 0.03).  The
      same check against the truth at mu (1 + 2^-10) reports mismatches: it bites.
  A3  every refusal of smcmc_predictive_check is SMCMC_ERR_INVALID with nothing written, a well-formed call without a
      device SMCMC_ERR_NO_DEVICE
"""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location("smcmc_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


pref, truth = _load("poisson_ref"), _load("poisson_truth")

UP, DP = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
INVALID, NO_DEVICE = 1, 7
SEED = 20260519
MEANS = [-3.0, 0.0, 0.0005, 0.001, 0.7, math.nextafter(16.0, 0.0), 16.0, math.nextafter(16.0, math.inf), 37.25, 200.0,
         1234.5, 1e4, 1e5, 2.0 ** 20]
NOT_DRAWN = [math.nextafter(2.0 ** 20, math.inf), float("nan"), float("inf"), float("-inf")]
N_RESTATED, N_TRUTH, N_TRUTH_LARGEST = 4096, 20000, 2000


def addresses(n, salt):
    """n distinct (chain, slot, row, replica): every field moves, up to its largest value"""
    i = np.arange(n, dtype=np.int64)
    chain = (i * 2654435761 + salt * 97) % (2 ** 32)
    slot = (i * 40503 + salt) % (2 ** 28)
    row = (i * 31 + 7 * salt) % (2 ** 16)
    replica = (i // 5 + salt) % (2 ** 16)
    chain[:2], slot[:2], row[:2], replica[:2] = (0, 2 ** 32 - 1), (0, 2 ** 28 - 1), (0, 2 ** 16 - 1), (0, 2 ** 16 - 1)
    return chain, slot, row, replica


@pytest.fixture(scope="module")
def restated(smcmc, oracle):
    return pref.Restatement(oracle, smcmc)


@pytest.mark.parametrize("k", range(len(MEANS)))
def test_a1_the_library_is_the_restatement(smcmc, restated, k):
    mean = MEANS[k]
    chain, slot, row, replica = addresses(N_RESTATED, k)
    got = smcmc.poisson_draw(SEED + k, chain, slot, row, replica, mean)
    want = np.array([restated.draw(SEED + k, int(c), int(t), int(r), int(j), mean)[0]
                     for c, t, r, j in zip(chain, slot, row, replica)])
    assert np.array_equal(got, want), "mean %r: %d of %d draws differ" % (mean, int((got != want).sum()), N_RESTATED)
    assert np.all(got == np.floor(got)) and np.all(got >= 0)
    if mean >= 200.0:
        assert len(np.unique(got)) > 20      # a spread, not one value


def test_a1_invalid_expectations_draw_nothing(smcmc, restated):
    lib = smcmc.load()
    for e in NOT_DRAWN:
        y, valid = C.c_double(-7.0), C.c_int(-7)
        assert lib.smcmc_poisson_draw(SEED, 3, 4, 5, 6, e, C.byref(y), C.byref(valid)) == 0
        assert math.isnan(y.value) and valid.value == 0
        assert restated.draw(SEED, 3, 4, 5, 6, e)[1] == 0
        assert math.isnan(smcmc.poisson_draw(SEED, 3, 4, 5, 6, e))
    y, valid = C.c_double(-7.0), C.c_int(-7)
    assert lib.smcmc_poisson_draw(SEED, 3, 4, 5, 6, 2.0 ** 20, C.byref(y), C.byref(valid)) == 0 and valid.value == 1
    # the counter's fields: nothing written
    for slot, row, replica in ((2 ** 28, 0, 0), (0, 2 ** 16, 0), (0, 0, 2 ** 16)):
        y, valid = C.c_double(-7.0), C.c_int(-7)
        assert lib.smcmc_poisson_draw(SEED, 0, slot, row, replica, 1.0, C.byref(y), C.byref(valid)) == INVALID
        assert y.value == -7.0 and valid.value == -7
    assert lib.smcmc_poisson_draw(SEED, 0, 0, 0, 0, 1.0, None, C.byref(valid)) == INVALID
    assert lib.smcmc_poisson_draw(SEED, 0, 0, 0, 0, 1.0, C.byref(y), None) == INVALID


def test_a1_vectorised_over_arrays(smcmc):
    e = np.array([[0.5, 20.0, float("nan")], [3.0, 1e3, 2e6]])
    got = smcmc.poisson_draw(SEED, np.arange(3), 9, np.array([[1], [2]]), 0, e)
    assert got.shape == (2, 3) and np.isnan(got[0, 2]) and np.isnan(got[1, 2]) and np.isfinite(got[:, :2]).all()
    assert got[1, 1] == smcmc.poisson_draw(SEED, 1, 9, 2, 0, 1e3)
    assert isinstance(smcmc.poisson_draw(SEED, 1, 9, 2, 0, 1e3), float)


@pytest.mark.parametrize("k", range(len(MEANS)))
def test_a2_every_draw_is_the_exact_distributions(smcmc, restated, k):
    mean = MEANS[k]
    n = N_TRUTH_LARGEST if mean == 2.0 ** 20 else N_TRUTH
    chain, slot, row, replica = addresses(n, 100 + k)
    seed = SEED + 1000 + k
    drawn = smcmc.poisson_draw(seed, chain, slot, row, replica, mean)
    u = np.array([restated.uniform_at(seed, int(c), int(t), int(r), int(j)) for c, t, r, j in zip(chain, slot, row, replica)])
    assert u.min() > 0.0 and u.max() < 1.0 and len(np.unique(u)) == n
    mu = truth.mean_of(mean)
    wrong, left_out, nthresholds = truth.check(u, drawn, mu)
    print("mean %r: %d draws, %d thresholds, %d wrong, %d inside the band" % (mean, n, nthresholds, wrong, left_out))
    assert wrong == 0
    assert left_out <= 2
    # The check bites: the truth of a mean 2^-10 away disagrees.  Its thresholds move by about mu 2^-10 pmf each, so the
    # draws that tell the two apart number about n mu 2^-10 sum(pmf(k) |k - mu| / mu): 12 at mu = 0.7 and more above it,
    # but 0.02 at the clamp's mu = 0.001, where one threshold at exp(-0.001) is all there is -- the four expectations
    # that are drawn at the clamp are counted, not asserted.
    wrong_off, _, _ = truth.check(u, drawn, mu * (1.0 + 2.0 ** -10))
    print("          against mu (1 + 2^-10): %d wrong" % wrong_off)
    if mu >= 0.7:
        assert wrong_off > 0


# ---- A3: the refusals of smcmc_predictive_check ----------------------------------------------------------------------

def call(lib, hist=0x1000, nslots=2, rows=6, nchains=65, npad=128, data=None, ngroups=3, slot_offset=0, replica=0,
         give=("below", "equal", "stat", "invalid"), rep=None, stat=None):
    """(status, untouched): the host outputs are prefilled with 7; `hist` is never followed without a device"""
    n = max(rows, 1)
    d = np.arange(n, dtype=np.float64) if data is None else np.ascontiguousarray(data, dtype=np.float64)
    below, equal = np.full(n, 7, dtype=np.uint64), np.full(n, 7, dtype=np.uint64)
    counts, invalid = np.full(3 * (max(ngroups, 0) + 1), 7, dtype=np.uint64), np.full(1, 7, dtype=np.uint64)
    st = lib.smcmc_predictive_check(C.c_void_p(hist) if hist else None, nslots, rows, nchains, npad,
                                    d.ctypes.data_as(DP) if data is not False else None, ngroups, SEED, 0, slot_offset, replica,
                                    C.c_void_p(rep) if rep else None, C.c_void_p(stat) if stat else None,
                                    below.ctypes.data_as(UP) if "below" in give else None,
                                    equal.ctypes.data_as(UP) if "equal" in give else None,
                                    counts.ctypes.data_as(UP) if "stat" in give else None,
                                    invalid.ctypes.data_as(UP) if "invalid" in give else None, None)
    return st, bool(np.all(below == 7) and np.all(equal == 7) and np.all(counts == 7) and np.all(invalid == 7))


REFUSED = [dict(hist=0), dict(data=False), dict(give=("equal", "stat", "invalid")), dict(give=("below", "stat", "invalid")),
           dict(give=("below", "equal", "invalid")), dict(give=("below", "equal", "stat")),
           dict(nslots=0), dict(nchains=0), dict(npad=64), dict(npad=129), dict(npad=200),
           dict(rows=0, ngroups=1), dict(rows=4097, ngroups=1), dict(rows=-1, ngroups=1),
           dict(ngroups=0), dict(ngroups=9, rows=18), dict(ngroups=4), dict(ngroups=-1),
           dict(data=[0, 1, 2, -1e-300, 4, 5]), dict(data=[0, 1, float("nan"), 3, 4, 5]), dict(data=[0, 1, 2, 3, 4, float("inf")]),
           dict(slot_offset=2 ** 28 - 1), dict(slot_offset=2 ** 28), dict(nslots=2 ** 28 + 1), dict(replica=2 ** 16),
           dict(replica=2 ** 32 - 1)]


def test_a3_refusals_need_no_device(smcmc):
    lib = smcmc.load()
    for kw in REFUSED:
        assert call(lib, **kw) == (INVALID, True), kw
        assert b"smcmc_predictive_check" in lib.smcmc_event_sample_last_error()
    with pytest.raises(smcmc.SmcmcError) as err:
        smcmc.predictive_check(0x1000, 2, 6, 65, 128, np.arange(6.0), 4, SEED)
    assert err.value.status == INVALID and "ngroups" in str(err.value)
    with pytest.raises(ValueError):
        smcmc.predictive_check(0x1000, 2, 6, 65, 128, np.arange(5.0), 3, SEED)
    import torch
    if torch.cuda.is_available():
        return                               # tests/test_gpu_predictive_check.py has the device's side
    for kw in (dict(), dict(rows=4096, ngroups=8), dict(rows=197, ngroups=1), dict(slot_offset=2 ** 28 - 2),
               dict(replica=2 ** 16 - 1), dict(nchains=128), dict(data=[0.0, 0.5, 2.0, 1e300, 4.0, 5.0])):
        assert call(lib, **kw) == (NO_DEVICE, True), kw
        assert lib.smcmc_event_sample_last_error() == b""


def test_a3_counts_add_and_refuse_other_data(smcmc):
    """PredictiveCheck on the host alone: p-values from the counts, addition, the refusal of other data"""
    data = np.array([[1.0, 2.0], [0.0, 5.0], [3.0, 3.0]])
    a = smcmc.PredictiveCheck(data, [[1, 2], [3, 4], [5, 6]], [[1, 0], [0, 1], [2, 2]],
                              [[2, 1, 10], [0, 0, 10], [10, 0, 10], [4, 2, 10]], 1)
    b = smcmc.PredictiveCheck(data, np.ones((3, 2)), np.zeros((3, 2)), [[1, 1, 6], [6, 0, 6], [0, 0, 6], [1, 0, 6]], 0)
    assert a.names == ("Close", "Separated", "DecayTag") and a.n == 10 and a.invalid == 1
    assert a.pvalue == 0.6 and a.mid_pvalue == 0.5
    assert a.group_pvalues == {"Close": 0.3, "Separated": 0.0, "DecayTag": 1.0}
    assert a.group_mid_pvalues["Close"] == 0.25
    le, ge = a.bin_tail()
    assert le[0, 0] == 0.2 and ge[0, 0] == 0.9 and le.shape == (3, 2)
    s = a + b
    assert s.n == 16 and s.invalid == 1 and s.below[2, 1] == 7 and s.below.dtype == np.uint64
    assert np.array_equal(s.stat_counts, np.array([[3, 2, 16], [6, 0, 16], [10, 0, 16], [5, 2, 16]], dtype=np.uint64))
    other = smcmc.PredictiveCheck(data + 1.0, np.ones((3, 2)), np.zeros((3, 2)), np.ones((4, 3)), 0)
    with pytest.raises(ValueError):
        a + other
    assert smcmc.PredictiveCheck(np.ones((2, 2)), np.ones((2, 2)), np.ones((2, 2)), np.ones((3, 3)), 0).names == ("group0", "group1")
