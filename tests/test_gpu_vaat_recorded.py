"""smcmc_vaat_step_recorded, smcmc_vaat_snapshot and smcmc_vaat_rollback: the per-step record of one chain is the reference
chain (oracle/vaat_oracle.c) stepped one step at a time and what a second engine reads back after every Step(1); the
rows rebuild the chain's point and per-dimension arrays; the call is Step(n) for every chain.  Bit equality throughout.

70 chains (two wavefronts, the second partial), chain 0 and chain 69, both arithmetic orders, with and without the
explicit UpdateProposal() of SimpleVAAT.C:44 (without it the first row has a refill inside the step; with it the first
ADAPT_INDEX is -1), SetAcceptanceWindow(20) so that widths move within a few visits per dimension, every launch across
at least two queue refills.  No way to make a snapshot fail to allocate at these sizes: SMCMC_ERR_HIP of
smcmc_vaat_snapshot is not exercised here."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 11
N = 70
# (likelihood, dim, nsteps): the smallest and the largest register family (dim 63: 85 KB of LDS), the smallest
# large-kernel shape, the three likelihoods every kernel family is built for
SHAPES = [(0, 5, 4 * 5 + 3), (1, 12, 51), (0, 63, 2 * 63 + 6), (1, 64, 2 * 64 + 6), (2, 100, 207)]
F64 = ("logl", "logl_proposed", "step_rms")
I32 = ("last_accept", "trials", "successes", "naccept", "step_rms_trials")


def _x0(kind, dim):
    rng = np.random.default_rng(kind * 1000 + dim)
    if kind == 2:
        return rng.uniform(0.5, 1.5, size=(dim, N))
    return rng.uniform(-1.0, 1.0, size=(dim, N))                     # SimpleVAAT.C:41


def _params(oracle, kind, dim):
    prm = oracle.like_params(kind, dim)
    return prm if prm.size else None


def _engine(gpu, oracle, kind, dim, exact, explicit):
    e = gpu.VaatEngine(dim, N, likelihood=kind, likelihood_params=_params(oracle, kind, dim), seed=SEED, exact=exact)
    assert e.Start(_x0(kind, dim))
    e.SetAcceptanceWindow(20)                                        # after Start, which makes it 100 (:211)
    if explicit:
        e.UpdateProposal()
    return e


def _reference(oracle, kind, dim, exact, explicit, c):
    """chain c alone: chains share nothing, chain c is the stream (seed, c)"""
    o = oracle.Vaat(1, dim, kind=kind, params=_params(oracle, kind, dim), seed=SEED, chain_offset=c, exact=exact)
    assert o.start(np.ascontiguousarray(_x0(kind, dim)[:, c:c + 1]))
    o.set_acceptance_window(20.0)
    if explicit:
        o.update_proposal()
    return o


def _row(gpu, lane, x, per_dim, adapt_index, total_steps, queue_length):
    """the record's row from what an engine (or the oracle) reads back after a step; adapt_index: fLastIndex before it"""
    f = {name: float(lane(name)) for name in F64 + I32}
    f["index"] = float(lane("last_index"))
    f["proposed_value"] = float(lane("proposed_value"))
    f["accepted_value"] = float(x[int(f["index"])])
    a = int(adapt_index)
    f["adapt_index"] = float(a) if a >= 0 else -1.0
    f["adapt_sigma"] = float(per_dim("sigma")[a]) if a >= 0 else 0.0
    f["adapt_acceptance"] = float(per_dim("acceptance")[a]) if a >= 0 else 0.0
    f["adapt_trials"] = float(per_dim("acceptance_trials")[a]) if a >= 0 else 0.0
    f["total_steps"] = float(total_steps)
    f["queue_length"] = float(queue_length)
    return np.array([f[name] for name in gpu.VAAT_RECORD_FIELDS])


def _state(e):
    qlen = e.queue_length
    out = [e.GetAccepted()]
    out += [e.lane(k) for k in ("logl", "logl_proposed", "step_rms", "proposed_value", "last_value", "trials", "successes",
                                "naccept", "last_accept", "last_index", "step_rms_trials")]
    out += [e.per_dim(k) for k in ("sigma", "acceptance", "acceptance_trials")]
    out += [e.per_dim("queue")[:qlen], np.array([qlen, e.total_steps])]
    return out


RECORDS = {}


def _record(gpu, oracle, kind, dim, nsteps, exact, explicit, c):
    key = (kind, dim, nsteps, exact, explicit, c)
    if key not in RECORDS:
        e = _engine(gpu, oracle, kind, dim, exact, explicit)
        assert e.record_stride == len(gpu.VAAT_RECORD_FIELDS) == 17
        rec = e.StepRecorded(nsteps, c)
        assert rec.shape == (nsteps, 17)
        rec.setflags(write=False)
        RECORDS[key] = (rec, _state(e))
    return RECORDS[key]


CASES = [pytest.param(k, d, n, x, u, c, id=f"like{k}-d{d}-{'exact' if x else 'fused'}-{'explicit' if u else 'bare'}-c{c}")
         for k, d, n in SHAPES for x in (True, False) for u in (True, False) for c in (0, N - 1)]


@pytest.mark.parametrize("kind,dim,nsteps,exact,explicit,c", CASES)
def test_record_is_the_reference_chain(gpu, oracle, kind, dim, nsteps, exact, explicit, c):
    rec, _ = _record(gpu, oracle, kind, dim, nsteps, exact, explicit, c)
    col = {name: k for k, name in enumerate(gpu.VAAT_RECORD_FIELDS)}
    o = _reference(oracle, kind, dim, exact, explicit, c)
    # the reader's side: the state at the start of the launch plus the rows
    x = o.x[:, 0].copy()
    arrays = {k: o.per_dim(k)[:, 0].copy() for k in ("sigma", "acceptance", "acceptance_trials")}
    refills = 0
    for k in range(nsteps):
        before = int(o.lane("last_index")[0])
        refills += int(o.lane("queue_len")[0] == 0)
        o.step(1)
        want = _row(gpu, lambda name: o.lane(name)[0], o.x[:, 0], lambda name: o.per_dim(name)[:, 0], before, k + 1,
                    o.lane("queue_len")[0])
        assert np.array_equal(rec[k], want), (k, [gpu.VAAT_RECORD_FIELDS[i] for i in np.flatnonzero(rec[k] != want)])
        if k == 0:
            assert (rec[0, col["adapt_index"]] == -1.0) and not np.signbit(rec[0, col["adapt_sigma"]:col["adapt_trials"] + 1]).any()
        x[int(rec[k, col["index"]])] = rec[k, col["accepted_value"]]
        a = int(rec[k, col["adapt_index"]])
        if a >= 0:
            arrays["sigma"][a] = rec[k, col["adapt_sigma"]]
            arrays["acceptance"][a] = rec[k, col["adapt_acceptance"]]
            arrays["acceptance_trials"][a] = rec[k, col["adapt_trials"]]
        assert np.array_equal(x, o.x[:, 0]), k                        # no coordinate other than INDEX moved
        for name in arrays:
            assert np.array_equal(arrays[name], o.per_dim(name)[:, 0]), (k, name)   # ... no entry other than ADAPT_INDEX
    assert refills >= 2                                               # steps that found the queue empty (:55)
    assert rec[:, col["last_accept"]].sum() > 0 and not np.all(arrays["sigma"] == 2.34)


@pytest.mark.parametrize("kind,dim,nsteps,exact,explicit,c", CASES)
def test_record_is_what_a_stepping_engine_reads_back(gpu, oracle, kind, dim, nsteps, exact, explicit, c):
    rec, _ = _record(gpu, oracle, kind, dim, nsteps, exact, explicit, c)
    e = _engine(gpu, oracle, kind, dim, exact, explicit)
    for k in range(nsteps):
        before = e.lane("last_index")[c]
        e.Step(1)
        x = e.GetAccepted()[:, c]
        want = _row(gpu, lambda name: e.lane(name)[c], x, lambda name: e.per_dim(name)[:, c], before, e.total_steps,
                    e.queue_length)
        assert np.array_equal(rec[k], want), (k, [gpu.VAAT_RECORD_FIELDS[i] for i in np.flatnonzero(rec[k] != want)])


@pytest.mark.parametrize("kind,dim,nsteps,exact,explicit,c", CASES)
def test_recorded_launch_is_step_for_every_chain(gpu, oracle, kind, dim, nsteps, exact, explicit, c):
    _, after = _record(gpu, oracle, kind, dim, nsteps, exact, explicit, c)
    twin = _engine(gpu, oracle, kind, dim, exact, explicit)
    twin.Step(nsteps)
    for a, b in zip(after, _state(twin)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("kind,dim,nsteps", SHAPES)
@pytest.mark.parametrize("exact", [True, False])
def test_launches_may_be_cut_anywhere(gpu, oracle, kind, dim, nsteps, exact):
    whole, after = _record(gpu, oracle, kind, dim, nsteps, exact, True, N - 1)
    e = _engine(gpu, oracle, kind, dim, exact, True)
    a = dim + dim // 2 + 1                                           # inside the second pass over the queue
    assert 0 < a % dim < dim and a < nsteps
    first, second = e.StepRecorded(a, N - 1), e.StepRecorded(nsteps - a, N - 1)
    assert np.array_equal(np.concatenate([first, second]), whole)
    for x, y in zip(after, _state(e)):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("kind,dim", [(0, 5), (1, 64)])
def test_snapshot_and_rollback(gpu, oracle, kind, dim):
    e = _engine(gpu, oracle, kind, dim, True, True)
    ref = _engine(gpu, oracle, kind, dim, True, True)
    e.snapshot()
    first = e.StepRecorded(12, N - 1)
    e.rollback()
    e.Step(5)
    ref.Step(5)
    for a, b in zip(_state(e), _state(ref)):
        assert np.array_equal(a, b)
    again = e.StepRecorded(7, N - 1)
    assert np.array_equal(again, first[5:12])
    e.rollback()                                                     # a second time, to the same snapshot
    fresh = _engine(gpu, oracle, kind, dim, True, True)
    for a, b in zip(_state(e), _state(fresh)):
        assert np.array_equal(a, b)
    assert np.array_equal(e.StepRecorded(12, N - 1), first)


def test_refusals(gpu, oracle):
    e = _engine(gpu, oracle, 0, 5, True, True)
    e.Step(3)
    before = _state(e)
    for call in (lambda: e.StepRecorded(3, chain=N), lambda: e.StepRecorded(3, chain=-1), lambda: e.StepRecorded(0),
                 lambda: e.StepRecorded(-2)):
        with pytest.raises(gpu.SmcmcError) as err:
            call()
        assert err.value.status == 1
    assert e._lib.smcmc_vaat_step_recorded(e._h, 3, 0, None) == 1
    with pytest.raises(gpu.SmcmcError) as err:
        e.rollback()                                                 # no snapshot yet
    assert err.value.status == 2
    for a, b in zip(before, _state(e)):
        assert np.array_equal(a, b)
    fresh = gpu.VaatEngine(5, N, seed=SEED)                          # not started
    assert fresh._lib.smcmc_vaat_snapshot(fresh._h) == 1 and fresh._lib.smcmc_vaat_rollback(fresh._h) == 1
    rec = np.full((3, fresh.record_stride), -7.0)
    assert fresh._lib.smcmc_vaat_step_recorded(fresh._h, 3, 0, rec.ctypes.data_as(C.POINTER(C.c_double))) == 1
    assert np.all(rec == -7.0) and fresh.total_steps == 0
