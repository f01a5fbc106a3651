"""smcmc_predictive_check on the device: replicated data, the likelihood's statistic on them and on the observed data, and
the integer counts behind the p-values.

  B1  hand-made buffers of Poisson means (one lane; 63 of 64; 130 of 256 with a whole dead block; 1, 5, 150 and 197 rows
      in 1, 5, 3 and 1 groups), the means of tests/test_poisson_cpu.py dealt so that neighbouring lanes and rows differ, a
      few points with one NaN, one infinite or one too large row, NaN in the padding: the replicates are
      smcmc_poisson_draw's bit for bit, the statistics the ordered sums restated here with the host log bit for bit, the
      counts numpy's integer counts of those arrays, an invalid point NaN in both buffers and counted once, the padding +0.0
  B2  the same integers from a second call without the optional outputs and with other padding; a window of slots with
      its slot_offset and a block of chains with its chain_offset reproduce the whole call's slices; replica 1 differs
      from replica 0 and their counts add as PredictiveCheck.__add__ says
  B3  an engine's own trace: the total T_obs is the saved log-likelihood bit for bit, the replicates' quantiles are
      integers, the p-values carry the histograms' names
  B4  the refusals of tests/test_poisson_cpu.py write nothing with a device present
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


ref, cases = _load("event_sample_ref"), _load("event_sample_cases")
cpu = _load("test_poisson_cpu")

pytestmark = pytest.mark.gpu
UP, DP = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
SEED = 20260520
SHAPES = [(1, 1, 64), (2, 63, 64), (3, 130, 256)]
ROWS = [(1, 1), (5, 5), (150, 3), (197, 1)]
NOT_DRAWN = [float("nan"), float("inf"), float("-inf"), math.nextafter(2.0 ** 20, math.inf)]


def same(a, b):
    """bit for bit (a zero's sign included), NaN compared as NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(((a == b) & (np.signbit(a) == np.signbit(b))) | (np.isnan(a) & np.isnan(b))))


def means(nslots, rows, nchains):
    """[slot][row][chain]: the means dealt from the list, and which points are invalid"""
    t, r, c = np.meshgrid(np.arange(nslots), np.arange(rows), np.arange(nchains), indexing="ij")
    mu = np.array(cpu.MEANS)[(c + 5 * t + 3 * r) % len(cpu.MEANS)]
    bad = np.zeros((nslots, nchains), dtype=bool)
    for k, (tt, cc) in enumerate([(0, 0), (nslots - 1, nchains - 1), (nslots // 2, nchains // 2), (0, min(64, nchains - 1)),
                                  (nslots - 1, nchains // 3)]):
        if nslots * nchains == 1 and k > 0:
            break
        if nslots * nchains == 1 and rows > 1:
            break                                        # the one point of the smallest shape stays valid where it has rows to show
        mu[tt, (7 * k + 3) % rows, cc] = NOT_DRAWN[k % len(NOT_DRAWN)]
        bad[tt, cc] = True
    return mu, bad


def observed(rows):
    return np.array([0.0, 1.0, 16.0, 0.5, 37.0, 200.0, 15.0, 1234.0, 1e4, 2.0, 1e5, 1048600.0, 17.0])[(np.arange(rows) * 5) % 13]


def host_log(gpu, x):
    return gpu.selftest_detmath(0, np.ascontiguousarray(x, dtype=np.float64).ravel(), device=-1).reshape(np.shape(x))


def bin_term(gpu, data, mc):
    """smcmc_es_bin_term over arrays, un-fused, with the host smcmc_log"""
    mc = np.where(mc < 0.001, 0.001, mc)
    v = data - mc
    pos = data > 0.0
    safe = np.where(pos, data, 1.0)
    return np.where(pos, v + data * host_log(gpu, mc / safe), v)


def expected(gpu, mu, bad, data, ngroups, seed, chain_offset=0, slot_offset=0, replica=0):
    """(rep[slot][rows][chain], stat[slot][2 (ngroups + 1)][chain]) of the live lanes, NaN at the invalid points"""
    nslots, rows, nchains = mu.shape
    t, r, c = np.meshgrid(np.arange(nslots), np.arange(rows), np.arange(nchains), indexing="ij")
    rep = gpu.poisson_draw(seed, c + chain_offset, t + slot_offset, r, replica, mu)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mus = np.where(np.isfinite(mu), mu, 1.0)
        t_obs, t_rep = bin_term(gpu, data[None, :, None], mus), bin_term(gpu, np.where(np.isnan(rep), 0.0, rep), mus)
    stat = np.zeros((nslots, 2 * (ngroups + 1), nchains))
    per = rows // ngroups
    for row in range(rows):                              # rows ascending from +0.0: the group's sums and the total's own
        g = row // per
        stat[:, 2 * g] += t_obs[:, row]
        stat[:, 2 * g + 1] += t_rep[:, row]
        stat[:, 2 * ngroups] += t_obs[:, row]
        stat[:, 2 * ngroups + 1] += t_rep[:, row]
    rep[np.broadcast_to(bad[:, None, :], rep.shape)] = np.nan
    stat[np.broadcast_to(bad[:, None, :], stat.shape)] = np.nan
    return rep, stat


def counts_of(rep, stat, bad, data, ngroups):
    good = ~bad
    below = np.array([(good & (rep[:, r] < data[r])).sum() for r in range(rep.shape[1])], dtype=np.uint64)
    equal = np.array([(good & (rep[:, r] == data[r])).sum() for r in range(rep.shape[1])], dtype=np.uint64)
    sc = np.array([[(good & (stat[:, 2 * g + 1] < stat[:, 2 * g])).sum(), (good & (stat[:, 2 * g + 1] == stat[:, 2 * g])).sum(),
                    good.sum()] for g in range(ngroups + 1)], dtype=np.uint64)
    return below, equal, sc, int(bad.sum())


def device_buffer(mu, npad, padding):
    import torch
    nslots, rows, nchains = mu.shape
    h = torch.full((nslots, rows, npad), padding, dtype=torch.float64, device="cuda")
    h[:, :, :nchains] = torch.from_numpy(np.ascontiguousarray(mu)).to("cuda")
    torch.cuda.synchronize()
    return h


def run(gpu, h, nslots, rows, nchains, npad, data, ngroups, seed, outputs=True, ptr=None, **kw):
    """(PredictiveCheck, rep[slot][rows][npad] or None, stat or None); the optional outputs prefilled with -7"""
    import torch
    rep = torch.full((nslots, rows, npad), -7.0, dtype=torch.float64, device="cuda") if outputs else None
    stat = torch.full((nslots, 2 * (ngroups + 1), npad), -7.0, dtype=torch.float64, device="cuda") if outputs else None
    torch.cuda.synchronize()
    pc = gpu.predictive_check(h.data_ptr() if ptr is None else ptr, nslots, rows, nchains, npad, data, ngroups, seed,
                              replicates_ptr=rep.data_ptr() if outputs else None,
                              statistics_ptr=stat.data_ptr() if outputs else None, **kw)
    torch.cuda.synchronize()
    return pc, (rep.cpu().numpy() if outputs else None), (stat.cpu().numpy() if outputs else None)


def same_counts(pc, below, equal, sc, invalid):
    return (np.array_equal(pc.below.ravel(), below) and np.array_equal(pc.equal.ravel(), equal)
            and np.array_equal(pc.stat_counts, sc) and pc.invalid == invalid)


@pytest.mark.parametrize("rows,ngroups", ROWS)
@pytest.mark.parametrize("nslots,nchains,npad", SHAPES)
def test_b1_hand_made_buffers(gpu, nslots, nchains, npad, rows, ngroups):
    mu, bad = means(nslots, rows, nchains)
    data = observed(rows)
    want_rep, want_stat = expected(gpu, mu, bad, data, ngroups, SEED)
    pc, rep, stat = run(gpu, device_buffer(mu, npad, float("nan")), nslots, rows, nchains, npad, data, ngroups, SEED)
    assert same(rep[:, :, :nchains], want_rep)
    assert same(stat[:, :, :nchains], want_stat)
    assert same(rep[:, :, nchains:], np.zeros((nslots, rows, npad - nchains)))           # +0.0
    assert same(stat[:, :, nchains:], np.zeros((nslots, 2 * (ngroups + 1), npad - nchains)))
    below, equal, sc, invalid = counts_of(want_rep, want_stat, bad, data, ngroups)
    assert same_counts(pc, below, equal, sc, invalid)
    assert pc.n + pc.invalid == nslots * nchains and pc.n == int(sc[-1, 2])
    if nslots * nchains > 1:
        assert invalid >= 3 and np.isnan(want_rep[bad.nonzero()[0][0], :, bad.nonzero()[1][0]]).all()
        assert (below + equal).max() > 0 and below.min() < pc.n                          # the counts tell rows apart
    valid_rep = want_rep[~np.isnan(want_rep)]
    assert np.all(valid_rep == np.floor(valid_rep))


def test_b2_repeat_and_slice(gpu):
    import torch
    nslots, nchains, npad, rows, ngroups = 3, 130, 256, 150, 3
    mu, bad = means(nslots, rows, nchains)
    data = observed(rows)
    h = device_buffer(mu, npad, float("nan"))
    pc, rep, stat = run(gpu, h, nslots, rows, nchains, npad, data, ngroups, SEED)
    again, _, _ = run(gpu, device_buffer(mu, npad, 3.0e5), nslots, rows, nchains, npad, data, ngroups, SEED, outputs=False)
    assert same_counts(again, pc.below.ravel(), pc.equal.ravel(), pc.stat_counts, pc.invalid)
    # slots [1, 3) as a call of their own
    window, wrep, wstat = run(gpu, h, 2, rows, nchains, npad, data, ngroups, SEED, slot_offset=1,
                              ptr=h.data_ptr() + 8 * rows * npad)
    assert same(wrep, rep[1:]) and same(wstat, stat[1:])
    first, _, _ = run(gpu, h, 1, rows, nchains, npad, data, ngroups, SEED, outputs=False)
    assert same_counts(first + window, pc.below.ravel(), pc.equal.ravel(), pc.stat_counts, pc.invalid)
    # the second block of chains as a call of its own
    block, brep, bstat = run(gpu, device_buffer(mu[:, :, 64:], 128, float("nan")), nslots, rows, nchains - 64, 128, data,
                             ngroups, SEED, chain_offset=64)
    assert same(brep[:, :, :nchains - 64], rep[:, :, 64:nchains]) and same(bstat[:, :, :nchains - 64], stat[:, :, 64:nchains])
    head, _, _ = run(gpu, device_buffer(mu[:, :, :64], 64, float("nan")), nslots, rows, 64, 64, data, ngroups, SEED,
                     outputs=False)
    assert same_counts(head + block, pc.below.ravel(), pc.equal.ravel(), pc.stat_counts, pc.invalid)
    # another replica: other draws, and the counts add
    other, orep, _ = run(gpu, h, nslots, rows, nchains, npad, data, ngroups, SEED, replica=1)
    want, _ = expected(gpu, mu, bad, data, ngroups, SEED, replica=1)
    assert same(orep[:, :, :nchains], want) and not same(orep, rep)
    both = pc + other
    assert np.array_equal(both.below, pc.below + other.below) and np.array_equal(both.equal, pc.equal + other.equal)
    assert np.array_equal(both.stat_counts, pc.stat_counts + other.stat_counts) and both.invalid == 2 * pc.invalid
    assert both.n == 2 * pc.n
    with pytest.raises(ValueError):
        pc + run(gpu, h, nslots, rows, nchains, npad, data + 1.0, ngroups, SEED, outputs=False)[0]
    del torch


def test_b3_an_engines_own_trace(gpu, oracle):
    import torch
    params = np.ascontiguousarray(cases.sample(ref, oracle, "197ev_50bins"))
    nchains, nslots, rows = 130, 8, 150
    eng = gpu.Engine(9, nchains=nchains, likelihood=gpu.LIKE_EVENT_SAMPLE, likelihood_params=params, seed=SEED,
                     mode=gpu.MODE_FROZEN)
    npad, stride = eng.nchains_padded, eng.dim_padded
    r = ref._Stream(oracle, 77)
    assert eng.Start(np.array([[2.0 * r.uniform() - 1.0 for _ in range(nchains)] for _ in range(9)]))
    x = torch.full((nslots, stride, npad), float("nan"), dtype=torch.float64, device="cuda")
    hist = torch.full((nslots, rows, npad), -7.0, dtype=torch.float64, device="cuda")
    logl = torch.full((nslots, npad), -7.0, dtype=torch.float64, device="cuda")
    rep = torch.full((nslots, rows, npad), -7.0, dtype=torch.float64, device="cuda")
    stat = torch.full((nslots, 8, npad), -7.0, dtype=torch.float64, device="cuda")
    saved = torch.full((nslots, npad), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    eng.StepSave(32, x.data_ptr(), saved.data_ptr(), stride=4)
    torch.cuda.synchronize()
    pp = eng.PosteriorPredictive(x.data_ptr(), nslots, histograms_ptr=hist.data_ptr(), logl_ptr=logl.data_ptr())
    pc = eng.PredictiveCheck(hist.data_ptr(), nslots, replicates_ptr=rep.data_ptr(), statistics_ptr=stat.data_ptr())
    torch.cuda.synchronize()
    stat_h, logl_h, rep_h = stat.cpu().numpy(), logl.cpu().numpy(), rep.cpu().numpy()
    assert np.isfinite(logl_h[:, :nchains]).all()
    assert same(stat_h[:, 6, :nchains], logl_h[:, :nchains])                 # the total T_obs is the likelihood's logl
    assert same(stat_h[:, 6, :nchains], saved.cpu().numpy()[:, :nchains])    # ... the one the step kernel saved
    assert same(stat_h[:, :, nchains:], np.zeros((nslots, 8, npad - nchains)))
    assert pc.n + pc.invalid == 8 * 130 and pc.n == int(pc.stat_counts[-1, 2])
    assert np.array_equal(pc.data, pp.data) and pc.below.shape == pc.equal.shape == (3, 50)
    assert list(pc.group_pvalues) == ["Close", "Separated", "DecayTag"] == list(pc.names)
    assert all(0.0 <= v <= 1.0 for v in pc.group_pvalues.values()) and 0.0 <= pc.mid_pvalue <= pc.pvalue <= 1.0
    le, ge = pc.bin_tail()
    assert le.shape == (3, 50) and np.all(le + ge >= 1.0 - 1e-12) and np.all(le <= 1.0)
    # the replicates are this engine's: its seed and its chains
    hist_h = hist.cpu().numpy()
    assert same(rep_h[0, :, :nchains], gpu.poisson_draw(SEED, np.arange(nchains)[None, :], 0, np.arange(rows)[:, None], 0,
                                                         hist_h[0, :, :nchains]))
    q = eng.PredictiveQuantiles(rep.data_ptr(), nslots)
    assert q.values.shape[0] == rows and np.isfinite(q.values).all() and np.all(q.values == np.floor(q.values))
    lo, hi = q.interval(0.95)
    assert lo.shape == (3, 50) and np.all(lo <= hi)
    eng.close()
    gauss = gpu.Engine(9, nchains=64)
    with pytest.raises(gpu.SmcmcError) as err:
        gauss.PredictiveCheck(hist.data_ptr(), 1)
    assert err.value.status == 2                                             # SMCMC_ERR_LOGIC: not the family's likelihood
    gauss.close()


def test_b4_refusals_write_nothing_with_a_device(gpu):
    import torch
    lib = gpu.load()
    h = torch.ones((2, 6, 128), dtype=torch.float64, device="cuda")
    for kw in cpu.REFUSED:
        rep = torch.full((2, 6, 128), -7.0, dtype=torch.float64, device="cuda")
        stat = torch.full((2, 8, 128), -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        args = dict(hist=h.data_ptr(), rep=rep.data_ptr(), stat=stat.data_ptr())
        args.update(kw)
        assert cpu.call(lib, **args) == (cpu.INVALID, True), kw
        torch.cuda.synchronize()
        assert bool((rep == -7.0).all()) and bool((stat == -7.0).all()), kw
    rep = torch.full((2, 6, 128), -7.0, dtype=torch.float64, device="cuda")
    stat = torch.full((2, 8, 128), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert cpu.call(lib, hist=h.data_ptr(), rep=rep.data_ptr(), stat=stat.data_ptr()) == (0, False)      # the well-formed call runs
    assert lib.smcmc_event_sample_last_error() == b""
    assert not bool((rep == -7.0).any()) and not bool((stat == -7.0).any())
