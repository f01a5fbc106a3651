"""smcmc_hmc_step_recorded, smcmc_hmc_snapshot and smcmc_hmc_rollback (SMCMC_MODE_PER_CHAIN): the per-step record of one
chain is the reference chain stepped one step at a time, and what a second engine reads back after every Step(1)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20240607


def _spd(dim, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((dim, dim)) / np.sqrt(dim)
    return a @ a.T + np.eye(dim)


def _engine(gpu, kind, dim, nchains, mode=None):
    prm = np.linalg.inv(_spd(dim, 3)) if kind == 1 else None
    e = gpu.HmcEngine(dim, nchains, likelihood=kind, likelihood_params=prm, seed=SEED,
                      mode=gpu.MODE_PER_CHAIN if mode is None else mode)
    x0 = np.full(dim, 0.5) if kind == 1 else np.ones(dim)
    e.Start(x0)
    return e, prm, x0


def _fields(gpu, rec, dim):
    out = {"accepted": rec[:, :dim], "average": rec[:, dim:2 * dim]}
    for k, name in enumerate(gpu.HMC_RECORD_FIELDS):
        out[name] = rec[:, 2 * dim + k]
    return out


def _row_of_engine(e, c):
    """what smcmc_hmc_read_state, the lanes and smcmc_hmc_read_chain_tuning return now, in the record's layout"""
    q, m, logl = e.state()
    avg, cov, t = e.chain_tuning(c)
    sc = [-logl[c], -e.lane("logl_proposed")[c], e.lane("acceptance")[c], float(e.lane("last_accept")[c]),
          e.lane("mean_epsilon")[c], float(e.lane("leapfrog")[c]), e.lane("reversal_len")[c], float(e.lane("trials")[c])]
    from root_simple_mcmc_amd import _capi
    return np.concatenate([q[:, c], avg, sc, [t[k] for k in _capi.HMC_TUNING]])


RECORDS = {}


def _record(gpu, kind, dim, nchains, nsteps, chain):
    key = (kind, dim, nchains, nsteps, chain)
    if key not in RECORDS:
        e, prm, x0 = _engine(gpu, kind, dim, nchains)
        assert e.record_stride == 2 * dim + len(gpu.HMC_RECORD_FIELDS)
        rec = e.StepRecorded(nsteps, chain)
        rec.setflags(write=False)
        RECORDS[key] = (rec, prm, x0)
    return RECORDS[key]


SIZES = [(0, 5, 70, 32), (1, 64, 40, 2 * 64 + 6)]


@pytest.mark.parametrize("kind,dim,nchains,nsteps", SIZES)
@pytest.mark.parametrize("last", [False, True])
def test_record_is_the_reference_chain(gpu, oracle, kind, dim, nchains, nsteps, last):
    c = nchains - 1 if last else 0
    rec, prm, x0 = _record(gpu, kind, dim, nchains, nsteps, c)
    f = _fields(gpu, rec, dim)
    h = oracle.Hmc(dim, kind=kind, params=prm, seed=SEED, chain_id=c, potential_from_gradient=True)
    h.start(x0)
    for k in range(nsteps):
        h.step()
        s = h.scalars
        assert np.array_equal(f["accepted"][k], h.accepted), k
        assert np.array_equal(f["average"][k], h.average), k
        for name, want in (("potential", "accepted_potential"), ("proposed_potential", "proposed_potential"),
                           ("acceptance", "current_acceptance"), ("mean_epsilon", "mean_epsilon"),
                           ("leapfrog", "leapfrog_steps"), ("reversal_len", "reversal_len"), ("trace", "trace"),
                           ("orbit", "orbit"), ("updates", "updates"), ("cov_trials", "cov_trials")):
            assert f[name][k] == s[want], (k, name, f[name][k], s[want])
        assert f["step_count"][k] == k + 1
        assert f["last_accept"][k] == s["last_accept"], k
    assert f["updates"].max() >= 1


@pytest.mark.parametrize("kind,dim,nchains,nsteps", SIZES)
@pytest.mark.parametrize("last", [False, True])
def test_record_is_what_a_stepping_engine_reads_back(gpu, kind, dim, nchains, nsteps, last):
    c = nchains - 1 if last else 0
    rec, _, _ = _record(gpu, kind, dim, nchains, nsteps, c)
    e, _, _ = _engine(gpu, kind, dim, nchains)
    for k in range(nsteps):
        e.Step(1)
        row = _row_of_engine(e, c)
        assert np.array_equal(rec[k], row), (k, np.flatnonzero(rec[k] != row))


def _state(e, chains):
    out = list(e.state()) + [e.lane(k) for k in ("logl_proposed", "acceptance", "mean_epsilon", "reversal_len", "naccept",
                                                  "last_accept", "trials", "leapfrog", "contributes")]
    for c in chains:
        avg, cov, t = e.chain_tuning(c)
        out += [avg, cov, np.array([t[k] for k in sorted(t)])]
    return out


def test_snapshot_and_rollback(gpu):
    dim, n = 5, 70
    e, _, _ = _engine(gpu, 0, dim, n)
    ref, _, _ = _engine(gpu, 0, dim, n)
    e.snapshot()
    first = e.StepRecorded(12)
    e.rollback()
    e.Step(5)
    ref.Step(5)
    for a, b in zip(_state(e, (0, 69)), _state(ref, (0, 69))):
        assert np.array_equal(a, b)
    again = e.StepRecorded(7)
    assert np.array_equal(again, first[5:12])
    e.rollback()                                     # a second time, to the same snapshot
    ref2, _, _ = _engine(gpu, 0, dim, n)
    for a, b in zip(_state(e, (0, 69)), _state(ref2, (0, 69))):
        assert np.array_equal(a, b)
    assert np.array_equal(e.StepRecorded(12), first)


def test_refusals(gpu):
    import ctypes as C
    p, _, _ = _engine(gpu, 0, 5, 70, mode=gpu.MODE_POOLED)
    for call in (lambda: p.StepRecorded(3), p.snapshot, p.rollback):
        with pytest.raises(gpu.SmcmcError) as err:
            call()
        assert err.value.status == 5
    e, _, _ = _engine(gpu, 0, 5, 70)
    before = e.state()
    with pytest.raises(gpu.SmcmcError) as err:
        e.StepRecorded(3, chain=70)
    assert err.value.status == 1
    with pytest.raises(gpu.SmcmcError) as err:
        e.StepRecorded(3, chain=-1)
    assert err.value.status == 1
    assert e._lib.smcmc_hmc_step_recorded(e._h, 3, 0, None) == 1
    with pytest.raises(gpu.SmcmcError) as err:
        e.rollback()                                 # no snapshot yet
    assert err.value.status == 2
    fresh = gpu.HmcEngine(5, 70, seed=SEED, mode=gpu.MODE_PER_CHAIN)
    assert fresh._lib.smcmc_hmc_snapshot(fresh._h) == 1 and fresh._lib.smcmc_hmc_rollback(fresh._h) == 1        # not started
    rec = np.zeros((3, fresh.record_stride))
    assert fresh._lib.smcmc_hmc_step_recorded(fresh._h, 3, 0, rec.ctypes.data_as(C.POINTER(C.c_double))) == 1   # not started
    for a, b in zip(before, e.state()):
        assert np.array_equal(a, b)
