"""HMC in SMCMC_MODE_PER_CHAIN: every chain keeps its own running covariance and runs UpdateCovariance /
UpdateErrorMatrix (TSimpleHMC.H:665-858) after each of its steps, so chain c of the engine is, bit for bit, the
reference TSimpleHMC chain on the stream (seed, chain_offset + c) -- oracle.Hmc(..., chain_id=chain_offset + c)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 5


def _spd(dim, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((dim, dim)) / np.sqrt(dim)
    return a @ a.T + np.eye(dim)


def _engine(gpu, dim, nchains, kind, params, exact=True, offset=0):
    return gpu.HmcEngine(dim, nchains, likelihood=kind, likelihood_params=params, seed=SEED, chain_offset=offset,
                         exact=exact, mode=gpu.MODE_PER_CHAIN)


def _oracles(oracle, dim, kind, params, x0, chains, exact=True, offset=0):
    out = {}
    for c in chains:
        h = oracle.Hmc(dim, kind=kind, params=params, seed=SEED, chain_id=offset + c, potential_from_gradient=True,
                       fused_gradient=not exact)
        h.start(x0 if x0.ndim == 1 else x0[:, c])
        out[c] = h
    return out


def _same(e, hs, tag):
    q, m, logl = e.state()
    lanes = {k: e.lane(k) for k in ("mean_epsilon", "leapfrog", "reversal_len", "acceptance")}
    for c, h in hs.items():
        s = h.scalars
        assert np.array_equal(q[:, c], h.accepted), f"{tag}, chain {c}: positions"
        assert np.array_equal(m[:, c], h.momentum), f"{tag}, chain {c}: momenta"
        assert logl[c] == -s["accepted_potential"], f"{tag}, chain {c}: potential"
        assert lanes["mean_epsilon"][c] == s["mean_epsilon"], f"{tag}, chain {c}: fMeanEpsilon"
        assert lanes["leapfrog"][c] == s["leapfrog_steps"], f"{tag}, chain {c}: fLeapFrogSteps"
        assert lanes["reversal_len"][c] == s["reversal_len"], f"{tag}, chain {c}: fReversalLen"
        assert lanes["acceptance"][c] == s["current_acceptance"], f"{tag}, chain {c}: fCurrentAcceptance"
        avg, cov, t = e.chain_tuning(c)
        assert np.array_equal(avg, h.average), f"{tag}, chain {c}: fAveragePoint"
        assert np.array_equal(cov, h.covariance), f"{tag}, chain {c}: fEstimatedCovariance"
        for k in ("trace", "orbit", "updates", "cov_trials"):
            assert t[k] == s[k], f"{tag}, chain {c}: {k} {t[k]} != {s[k]}"


def _checked(nchains):
    return sorted({c for c in (0, 1, 63, 64, nchains - 1) if c < nchains})


def _run(e, hs, nsteps, per_step=None):
    """after 1, after 2 and after nsteps steps; per_step(done) may change the configuration first"""
    done = 0
    for chunk in (1, 1, nsteps - 2):
        e.Step(chunk)
        for h in hs.values():
            h.run(chunk)
        done += chunk
        _same(e, hs, f"after {done} steps")


def _tunings(e):
    return [e.chain_tuning(c)[2] for c in range(e.nchains)]


CASES = [  # (kind, dim, nchains, per-chain start points, steps)
    (0, 5, 70, False, 4 * 5 + 12),
    (2, 6, 64, False, 4 * 6 + 12),
    (0, 20, 130, True, 4 * 20 + 12),
    (1, 63, 64, False, 2 * 63 + 6),
    (1, 64, 40, False, 2 * 64 + 6),
    (0, 100, 64, False, 2 * 100 + 6),
]


@pytest.mark.parametrize("kind,dim,nchains,own_start,nsteps", CASES)
def test_hmc_per_chain_default_tuning_is_the_reference_chain(gpu, oracle, kind, dim, nchains, own_start, nsteps):
    """SimpleHMC.C's call sequence (Start, then Step, nothing fixed): every checked chain passes fCovarianceTrials >= 2 dim
    and retunes itself at least once, and is the reference chain throughout."""
    prm = [100.0] if kind == 2 else (np.linalg.inv(_spd(dim, 3)) if kind == 1 else None)
    if own_start:
        x0 = np.random.default_rng(dim).uniform(-1.0, 1.0, (dim, nchains))
    else:
        x0 = np.ones(dim) if kind != 1 else np.full(dim, 0.5)
    e = _engine(gpu, dim, nchains, kind, prm)
    assert e.GetMode() == gpu.MODE_PER_CHAIN
    e.Start(x0)
    hs = _oracles(oracle, dim, kind, prm, x0, _checked(nchains))
    _run(e, hs, nsteps)
    tun = _tunings(e)
    for c in hs:
        assert tun[c]["updates"] >= 1 and tun[c]["cov_trials"] >= 2 * dim
    if nsteps > 4 * dim:
        # the chains retune on their own schedules: a pooled engine cannot show this
        assert (len({t["steps_since_update"] for t in tun}) > 1 or len({t["updates"] for t in tun}) > 1)


@pytest.mark.parametrize("exact", [True, False])
def test_hmc_per_chain_quadratic_form_both_orders(gpu, oracle, exact):
    dim, n = 40, 70
    prm = np.linalg.inv(_spd(dim, 7))
    x0 = np.full(dim, 0.5)
    e = _engine(gpu, dim, n, 1, prm, exact=exact)
    e.Start(x0)
    hs = _oracles(oracle, dim, 1, prm, x0, _checked(n), exact=exact)
    _run(e, hs, 2 * dim + 6)
    assert all(e.chain_tuning(c)[2]["updates"] >= 1 for c in hs)


def test_hmc_per_chain_fixed_leapfrog_tuned_step(gpu, oracle):
    """SetLeapFrog(n) with the step length left to the tuning"""
    dim, n = 20, 70
    prm = np.linalg.inv(_spd(dim, 3))
    x0 = np.full(dim, 0.5)
    e = _engine(gpu, dim, n, 1, prm)
    e.Start(x0)
    e.SetLeapFrog(6)
    hs = _oracles(oracle, dim, 1, prm, x0, _checked(n))
    for h in hs.values():
        h.set_leapfrog(6)
    _run(e, hs, 2 * dim + 10)
    assert np.all(e.lane("leapfrog") == -6)
    assert e.chain_tuning(0)[2]["updates"] >= 1


def test_hmc_per_chain_fixed_step_runs_the_tuning_for_its_outputs(gpu, oracle):
    """SetMeanEpsilon(<0) + SetLeapFrog(n): the states are the fixed-step path's, Trace / Orbit the reference chain's"""
    dim, n, steps = 8, 64, 30
    x0 = np.zeros(dim)
    e = _engine(gpu, dim, n, 0, None)
    f = gpu.HmcEngine(dim, n, seed=SEED)
    for eng in (e, f):
        eng.Start(x0)
        eng.SetMeanEpsilon(-0.2)
        eng.SetLeapFrog(5)
    hs = _oracles(oracle, dim, 0, None, x0, _checked(n))
    for h in hs.values():
        h.set_mean_epsilon(-0.2)
        h.set_leapfrog(5)
    _run(e, hs, steps)
    f.Step(steps)
    for a, b in zip(e.state(), f.state()):
        assert np.array_equal(a, b)
    t = e.chain_tuning(0)[2]
    assert t["updates"] >= 1 and t["orbit"] > 0 and t["trace"] > 0


def test_hmc_per_chain_gradient_types(gpu, oracle):
    """finite differences (3), zero (5) and a switch 0 -> 3 -> 5 -> 0 mid-run, on a likelihood with a gradient"""
    dim, n = 5, 70
    x0 = np.ones(dim)
    for schedule in ([(3, 2 * dim + 6)], [(5, 2 * dim + 6)], [(0, 3), (3, 4), (5, 5), (0, 2 * dim)]):
        e = _engine(gpu, dim, n, 0, None)
        e.Start(x0)
        hs = _oracles(oracle, dim, 0, None, x0, _checked(n))
        done = 0
        for t, steps in schedule:
            e.SetGradientType(t)
            for h in hs.values():
                h.set_gradient_type(t)
            for chunk in ((1, 1, steps - 2) if steps > 2 else (steps,)):
                e.Step(chunk)
                for h in hs.values():
                    h.run(chunk)
                done += chunk
                _same(e, hs, f"types {schedule}, after {done} steps")


def test_hmc_per_chain_refuses_the_covariant_gradient(gpu):
    e = _engine(gpu, 5, 10, 0, None)
    with pytest.raises(gpu.SmcmcError) as err:
        e.SetGradientType(2)
    assert err.value.status == 5
    f = gpu.HmcEngine(5, 10)
    f.SetGradientType(2)
    with pytest.raises(gpu.SmcmcError) as err:
        f.SetMode(gpu.MODE_PER_CHAIN)
    assert err.value.status == 5
    assert f.GetMode() == gpu.MODE_POOLED


def test_hmc_per_chain_chain_offset(gpu, oracle):
    dim, n = 5, 70
    x0 = np.ones(dim)
    e = _engine(gpu, dim, n, 0, None, offset=100)
    e.Start(x0)
    hs = _oracles(oracle, dim, 0, None, x0, _checked(n), offset=100)
    _run(e, hs, 2 * dim + 6)
    # two shards at offsets 0 and n / 2 are one engine of n chains
    whole = _engine(gpu, dim, n, 0, None)
    parts = [_engine(gpu, dim, n // 2, 0, None, offset=o) for o in (0, n // 2)]
    for eng in [whole] + parts:
        eng.Start(x0)
        eng.Step(2 * dim + 6)
    for a, b0, b1 in zip(whole.state(), parts[0].state(), parts[1].state()):
        assert np.array_equal(a, np.concatenate([b0, b1], axis=-1))
    for c in range(n):
        p, k = parts[c // (n // 2)], c % (n // 2)
        for a, b in zip(whole.chain_tuning(c)[:2], p.chain_tuning(k)[:2]):
            assert np.array_equal(a, b)
        assert whole.chain_tuning(c)[2] == p.chain_tuning(k)[2]


def test_hmc_per_chain_surface(gpu, oracle):
    dim, n = 5, 70
    e = gpu.HmcEngine(dim, n, seed=SEED)
    assert e.GetMode() == gpu.MODE_POOLED                       # the default
    with pytest.raises(gpu.SmcmcError) as err:
        e.SetMode(7)
    assert err.value.status == 1
    e.SetMode(gpu.MODE_PER_CHAIN)
    e.SetSyncInterval(3)                                        # accepted, no effect
    e.Start(np.ones(dim))
    with pytest.raises(gpu.SmcmcError) as err:
        e.SetMode(gpu.MODE_POOLED)
    assert err.value.status == 2
    e.Step(2 * dim + 4)
    before = e.state()
    e.sync()                                                    # a no-op
    for a, b in zip(before, e.state()):
        assert np.array_equal(a, b)
    with pytest.raises(gpu.SmcmcError) as err:
        e.reduce_moments()
    assert err.value.status == 2
    avg, cov, t = e.chain_tuning(0)
    assert np.array_equal(e.average, avg) and np.array_equal(e.covariance, cov) and e.tuning == t
    assert t["updates"] >= 1
    # the pooled default is untouched: the ensemble oracle, as before
    p = gpu.HmcEngine(dim, n, seed=SEED)
    o = oracle.HmcEnsemble(n, dim, seed=SEED, group=p.moment_group, sync_every=1, potential_from_gradient=True)
    p.Start(np.ones(dim)); o.start(np.ones(dim))
    p.Step(2 * dim + 4); o.step(2 * dim + 4)
    q, m, logl = p.state()
    oq, om = o.state()
    assert np.array_equal(q, oq) and np.array_equal(m, om)
    assert np.array_equal(p.lane("mean_epsilon"), o.lane("mean_epsilon"))
