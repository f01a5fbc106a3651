"""SMCMC_MODE_PER_CHAIN on the one-chain-per-workgroup kernel (SMCMC_P_PERCHAIN_WORKGROUP, smcmc_perchain_wg.hip.h):
the reference's own mode above dimension 63.  Checked lane by lane, bit for bit, against oracle.Chain with the covariance
adapting: accepted and proposed points, every lane scalar, centre, covariance and decomposition."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F64 = {"logl": "accepted_logl", "logl_proposed": "proposed_logl", "sigma": "sigma", "acceptance": "acceptance",
       "acceptance_trials": "acceptance_trials", "rigidity": "rigidity", "step_rms": "step_rms",
       "center_trials": "central_trials", "covariance_trials": "cov_trials", "sigma_trace": "sigma_trace"}
I32 = {"trials": "trials", "successes": "successes", "next_update": "next_update", "step_rms_trials": "step_rms_trials",
       "chain_steps": "total_steps", "update_count": "update_count", "last_update_path": "last_update_path"}


def _window(o, w):
    (o.SetAcceptanceWindow if hasattr(o, "SetAcceptanceWindow") else o.set_acceptance_window)(w)


def _make(gpu, oracle, dim, n, kind=0, which=None, seed=20240607, offset=0, x0=None, setup=None, dense=False, wave=None):
    prm = oracle.like_params(kind, dim)
    prm = prm if prm.size else None
    if wave is None:
        e = gpu.Engine(dim, n, likelihood=kind, likelihood_params=prm, seed=seed, chain_offset=offset,
                       mode=gpu.MODE_PER_CHAIN, perchain_workgroup=True)
        assert e.get_param("PERCHAIN_WORKGROUP") == 1 and e.get_param("PERCHAIN_WAVE") == 0
    else:
        e = gpu.Engine(dim, n, likelihood=kind, likelihood_params=prm, seed=seed, chain_offset=offset,
                       mode=gpu.MODE_PER_CHAIN)
        e.set_param("PERCHAIN_WAVE", wave)
    if dense:
        e.set_param("DENSE_QUADFORM", 1)
    which = list(range(n)) if which is None else list(which)
    chains = {c: oracle.Chain(dim, kind=kind, params=prm, seed=seed, chain_id=offset + c) for c in which}
    if setup:
        setup(e)
        for c in chains.values():
            setup(c)
    x0 = np.zeros(dim) if x0 is None else np.asarray(x0, dtype=np.float64)
    assert e.Start(x0)
    for c, ch in chains.items():
        assert ch.start(x0 if x0.ndim == 1 else x0[:, c])
    return e, chains


def _both(e, chains, name_e, name_c, *args):
    getattr(e, name_e)(*args)
    for ch in chains.values():
        getattr(ch, name_c)(*args)


def _step(e, chains, n, metropolis=0):
    e.Step(n, metropolis)
    for ch in chains.values():
        if metropolis == 0:
            ch.run_quiet(n)
        else:
            for _ in range(n):
                ch.step(False, metropolis)


def _same(e, chains, tag):
    x = e.GetAccepted()
    lanes = {k: e.lane(k) for k in list(F64) + list(I32)}
    for c, ch in chains.items():
        sc = ch.scalars
        assert np.array_equal(x[:, c], ch.accepted), f"{tag}: chain {c}: accepted point differs"
        for k, ok in F64.items():
            assert lanes[k][c] == sc[ok], f"{tag}: chain {c}: {k} = {lanes[k][c]!r}, reference chain {sc[ok]!r}"
        for k, ok in I32.items():
            assert lanes[k][c] == int(sc[ok]), f"{tag}: chain {c}: {k} = {lanes[k][c]}, reference chain {int(sc[ok])}"
        centre, cov, dec = e.chain_proposal(c)
        assert np.array_equal(centre, ch.center), f"{tag}: chain {c}: centre differs"
        assert np.array_equal(cov, ch.covariance), f"{tag}: chain {c}: covariance differs"
        assert np.array_equal(dec, ch.decomposition), f"{tag}: chain {c}: decomposition differs"
        assert np.array_equal(e.chain(c)["proposed"], ch.proposed), f"{tag}: chain {c}: proposed point differs"


def _max_dim(gpu):
    gpu.load()
    from importlib import import_module
    return int(import_module(gpu.__name__ + "._capi").load().smcmc_max_perchain_dim())


def _schedule(e, chains, steps=300, free=600):
    _same(e, chains, "start")
    _step(e, chains, 1)
    _same(e, chains, "first step")
    updates0 = e.lane("update_count").copy()
    for k in range(4):
        _both(e, chains, "SetNextUpdate", "set_next_update", 12)
        _step(e, chains, steps)
        _same(e, chains, f"forced schedule {k}")
    assert np.median(e.lane("update_count") - updates0) >= 3, "the launches must cross UpdateProposal events"
    _step(e, chains, free)
    _same(e, chains, "free running")


CASES = [(0, 64, 5), (0, 100, 5), (0, 128, 5), (0, 150, 5), (0, "max", 5), (2, "max", 5), (1, 100, 5), ("dense", 64, 5),
         (4, 100, 70), (5, 75, 5), (6, 100, 5)]


@pytest.mark.parametrize("kind,dim,n", CASES, ids=[f"{k}-{d}-{n}" for k, d, n in CASES])
def test_every_lane_is_the_reference_chain(gpu, oracle, kind, dim, n):
    dim = _max_dim(gpu) if dim == "max" else dim
    dense = kind == "dense"
    kind = 1 if dense else kind
    rng = np.random.default_rng(dim + 7 * kind)
    x0 = {2: rng.uniform(0.5, 1.5, size=(dim, n)), 5: rng.uniform(-0.5, 0.5, size=(dim, n)) / np.sqrt(dim),
          6: 76.0 + rng.normal(0.0, 1.0, size=(dim, n))}.get(kind, np.zeros(dim))
    which = range(n) if n <= 5 else (0, 1, 33, 69)
    e, chains = _make(gpu, oracle, dim, n, kind, which=which, x0=x0, dense=dense, setup=lambda o: _window(o, 150))
    _schedule(e, chains, steps=300 if kind not in (2, 5) else 600)


@pytest.mark.parametrize("dim", [5, 50, 63])
def test_three_kernels_one_chain(gpu, oracle, dim):
    """At dim <= 63 the workgroup kernel, the wave kernel and the oracle are the same chain."""
    runs = []
    for wave in (0, 1, None):                                     # one chain per lane, per wavefront, per workgroup
        e, chains = _make(gpu, oracle, dim, 3, 0, which=(0, 2), wave=wave, setup=lambda o: _window(o, 100))
        _both(e, chains, "SetNextUpdate", "set_next_update", 10)
        _step(e, chains, 400)
        _same(e, chains, f"wave={wave}")
        runs.append(e)
    a, b = runs[1], runs[2]
    for other in runs[:2]:
        assert np.array_equal(other.GetAccepted(), b.GetAccepted())
        for c in range(3):
            for u, v in zip(other.chain_proposal(c), b.chain_proposal(c)):
                assert np.array_equal(u, v)
    # the choice may change between launches at dim <= 63
    b.set_param("PERCHAIN_WORKGROUP", 0)
    assert b.get_param("PERCHAIN_WORKGROUP") == 0 and b.get_param("PERCHAIN_WAVE") == 1
    b.Step(50)
    a.Step(50)
    assert np.array_equal(a.GetAccepted(), b.GetAccepted())


def _bad_covariance(e, chains, dim, eigen=False):
    bad = np.eye(dim)
    bad[0, 1] = bad[1, 0] = 1.0 + 1e-3                           # correlation > 1: no Cholesky factor
    if eigen:
        # three correlations of -0.9: no clipping of single correlations repairs that, the eigen rung (:1252-1321) does
        for i, j in ((0, 1), (0, 2), (1, 2)):
            bad[i, j] = bad[j, i] = -0.9
    e.SetCovariance(bad)
    for ch in chains.values():
        ch.set_covariance(bad)
    _both(e, chains, "SetCovarianceWindow", "set_covariance_window", 10 ** 6)
    _both(e, chains, "SetCovarianceTrials", "set_covariance_trials", 1e6)
    _both(e, chains, "SetNextUpdate", "set_next_update", 3)


@pytest.mark.parametrize("per_launch,eigen", [(60, False), (1, False), (60, True)],
                         ids=["inside-a-launch", "last-step-of-a-launch", "eigen-rung"])
def test_the_fallback_ladder(gpu, oracle, per_launch, eigen):
    dim = 100
    e, chains = _make(gpu, oracle, dim, 3, 0)
    _step(e, chains, 50)
    _bad_covariance(e, chains, dim, eigen)
    for _ in range(60 // per_launch):
        _step(e, chains, per_launch)
    assert np.all(e.lane("last_update_path") >= 1), "the ladder must have run in every chain"
    if eigen:      # the full decomposition: the proposal's rows below the diagonal (the kernel's `ufull` path) run on
        assert np.all(e.lane("last_update_path") == 2) and np.all(e.lane("decomp_full") == 1)
    _same(e, chains, "after the ladder")
    _step(e, chains, 200)
    _same(e, chains, "and on")


def test_state_round_trips(gpu, oracle):
    dim = 100
    e, chains = _make(gpu, oracle, dim, 4, 2, which=(3,), x0=np.full(dim, 0.9))
    _both(e, chains, "SetNextUpdate", "set_next_update", 20)
    _step(e, chains, 300)
    st = e.saved_state(3)
    ref = chains[3].saved_state()
    e2, chains2 = _make(gpu, oracle, dim, 2, 2, which=(0, 1), x0=np.full(dim, 0.9))
    e2.Restore(st)
    for ch in chains2.values():
        ch.restore(ref)
    _same(e2, chains2, "restored")
    _step(e2, chains2, 150)
    _same(e2, chains2, "continued")
    _both(e2, chains2, "ResetProposal", "reset_proposal")
    _same(e2, chains2, "after ResetProposal")
    e2.SetCovarianceFrozen(True)
    for ch in chains2.values():
        ch.set_covariance_frozen(1)
    _step(e2, chains2, 100)
    _same(e2, chains2, "frozen covariance")
    e2.SetCovarianceFrozen(False)
    for ch in chains2.values():
        ch.set_covariance_frozen(0)
    _step(e2, chains2, 30, metropolis=1)
    _same(e2, chains2, "metropolis = 1")
    _step(e2, chains2, 5, metropolis=2)
    _same(e2, chains2, "metropolis = 2")
    p = np.linspace(0.8, 1.1, dim)
    e2.ForceStep(p)
    for ch in chains2.values():
        ch.force_step(p)
    _step(e2, chains2, 3)
    _same(e2, chains2, "forced step")


def test_update_proposal_of_a_covariance_without_a_trace(gpu, oracle):
    """A covariance whose trace is not positive (TSimpleMCMC.H:1025-1028, where the reference throws): UpdateProposal
    counts the call, leaves everything else of the chain alone and reports it."""
    dim = 64
    e, chains = _make(gpu, oracle, dim, 2)
    _step(e, chains, 20)
    _both(e, chains, "SetCovariance", "set_covariance", np.zeros((dim, dim)))
    with pytest.raises(gpu.SmcmcError, match="Invalid trace"):
        e.UpdateProposal()
    for ch in chains.values():
        ch.update_proposal()
        assert ch.scalars["failed"] == 1
    _same(e, chains, "UpdateProposal without a trace")
    assert np.all(e.lane("update_status")[:2] == 3)


def test_sharding(gpu, oracle):
    dim, n = 100, 6
    whole, chains = _make(gpu, oracle, dim, n, 0, which=(3, 5))
    part, _ = _make(gpu, oracle, dim, 3, 0, which=(), offset=3)
    for obj in (whole, part):
        obj.SetNextUpdate(10)
    for ch in chains.values():
        ch.set_next_update(10)
    whole.Step(120)
    for _ in range(4):
        part.Step(30)
    for ch in chains.values():
        ch.run_quiet(120)
    _same(whole, chains, "whole")
    assert np.array_equal(part.GetAccepted(), whole.GetAccepted()[:, 3:])
    for c in range(3):
        for a, b in zip(part.chain_proposal(c), whole.chain_proposal(3 + c)):
            assert np.array_equal(a, b)


def test_step_recorded_is_the_chain_step_by_step(gpu, oracle):
    dim, n, nsteps, c = 100, 3, 300, 1
    e, chains = _make(gpu, oracle, dim, n, 0, which=(c,))
    _both(e, chains, "SetNextUpdate", "set_next_update", 7)
    rec = e.StepRecorded(nsteps, chain=c)
    ch = chains[c]
    names = {"logl": "accepted_logl", "logl_proposed": "proposed_logl", "step_rms": "step_rms", "trials": "trials",
             "successes": "successes", "next_update": "next_update", "acceptance": "acceptance",
             "acceptance_trials": "acceptance_trials", "sigma": "sigma", "center_trials": "central_trials",
             "covariance_trials": "cov_trials", "total_steps": "total_steps"}
    for s in range(nsteps):
        moved = ch.step(False, 0)
        sc = ch.scalars
        assert np.array_equal(rec["accepted"][s], ch.accepted), f"step {s}: accepted"
        assert np.array_equal(rec["proposed"][s], ch.proposed), f"step {s}: proposed"
        assert bool(rec["last_accept"][s]) == bool(moved), f"step {s}: accept flag"
        for k, ok in names.items():
            assert rec[k][s] == sc[ok], f"step {s}: {k}"
        assert rec["covariance_trace"][s] == np.add.accumulate(np.diag(ch.covariance))[-1], f"step {s}: trace"
    assert int(ch.scalars["update_count"]) >= 2
    _same(e, chains, "after the recorded launch")


def test_larger_ensemble(gpu, oracle):
    dim, n = _max_dim(gpu), 1024
    e, chains = _make(gpu, oracle, dim, n, 0, which=(0, 511, 1023), setup=lambda o: _window(o, 100))
    _both(e, chains, "SetNextUpdate", "set_next_update", 10)
    _step(e, chains, 250)
    assert np.median(e.lane("update_count")) >= 2
    _same(e, chains, "1 024 chains")


def test_refusals(gpu):
    top = _max_dim(gpu)
    with pytest.raises(gpu.SmcmcError):
        gpu.Engine(top + 1, 2, mode=gpu.MODE_PER_CHAIN, perchain_workgroup=True)
    e = gpu.Engine(100, 2, mode=gpu.MODE_PER_CHAIN, perchain_workgroup=True, exact=False)
    with pytest.raises(gpu.SmcmcError) as err:
        e.Start(np.zeros(100))
    assert err.value.status == 5
    e = gpu.Engine(100, 2, mode=gpu.MODE_PER_CHAIN, perchain_workgroup=True)
    e.SetUniform(2, -1.0, 1.0)
    with pytest.raises(gpu.SmcmcError) as err:
        e.Start(np.zeros(100))
    assert err.value.status == 5
    e = gpu.Engine(100, 2, mode=gpu.MODE_PER_CHAIN, perchain_workgroup=True)
    with pytest.raises(gpu.SmcmcError) as err:
        e.set_param("PERCHAIN_WORKGROUP", 0)                     # above 63 nothing else runs the mode
    assert err.value.status == 5
    e = gpu.Engine(100, 2)
    with pytest.raises(gpu.SmcmcError):
        e._check(e._lib.smcmc_set_mode(e._h, gpu.MODE_PER_CHAIN))  # not asked for: refused as before


def _perchain_wg_snapshot(gpu):
    dim = _max_dim(gpu)
    e = gpu.Engine(dim, 64, mode=gpu.MODE_PER_CHAIN, perchain_workgroup=True)
    assert e.Start(np.zeros(dim))
    e.Step(2)
    e.snapshot()
    e.sync()
    return e


def _pooled_fold_ring(gpu):
    # the ring of per-step states (8 x 100 x 8 192 doubles, 52 MB) behind the fold of a multi-step launch
    e = gpu.Engine(100, 8192, mode=gpu.MODE_POOLED)
    assert e.Start(np.zeros(100))
    e.Step(16)
    e.sync()
    return e


def _perchain_record_ladder(gpu):
    # every chain's adaptive state (10 MB of decompositions), a 5 000-step record (6 MB) and the ladder's staging buffer
    dim = 50
    e = gpu.Engine(dim, 512, mode=gpu.MODE_PER_CHAIN)
    assert e.Start(np.zeros(dim))
    e.StepRecorded(5000, chain=1)
    _bad_covariance(e, {}, dim)
    e.Step(60)
    assert np.all(e.lane("last_update_path") >= 1), "the ladder must have run in every chain"
    return e


def _hmc_pooled(gpu):
    # the pooled tuning's buffers: two 100 x 8 192 images (6.5 MB each), the moments and the fold plan
    e = gpu.HmcEngine(100, 8192)
    e.Start(np.zeros(100))
    e.Step(4)
    e.sync()
    return e


def _hmc_per_chain(gpu):
    # every chain's running covariance: 1 275 x 4 096 doubles (42 MB)
    e = gpu.HmcEngine(50, 4096, mode=gpu.MODE_PER_CHAIN)
    e.Start(np.zeros(50))
    e.Step(2)
    return e


def _vaat(gpu):
    # per-dimension widths, acceptances, trials and queues: 50 x 16 384 each (6.5 MB the widths)
    e = gpu.VaatEngine(50, 16384)
    e.Start(np.zeros(50))
    e.Step(10)
    return e


LIFECYCLES = {"perchain_wg_snapshot": _perchain_wg_snapshot, "pooled_d100_fold_ring": _pooled_fold_ring,
              "perchain_d50_record_ladder": _perchain_record_ladder, "hmc_pooled": _hmc_pooled,
              "hmc_per_chain": _hmc_per_chain, "vaat": _vaat}


@pytest.mark.parametrize("case", list(LIFECYCLES))
def test_destroyed_engines_return_their_memory(gpu, case):
    """create -> Start -> steps -> destroy, five times: every buffer an engine allocated, lazily or not, goes back."""
    import gc
    import torch

    def one():
        e = LIFECYCLES[case](gpu)
        e.close()
        del e

    one()
    gc.collect()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(5):
        one()
        gc.collect()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    # every case holds at least one group of > 5 MB (the snapshot of the first is ~2 x 12 246 x 64 doubles, 13 MB, and
    # more): five leaked ones would be > 24 MB
    assert free0 - free1 < 24 << 20, f"{(free0 - free1) / 2**20:.1f} MiB not returned"
