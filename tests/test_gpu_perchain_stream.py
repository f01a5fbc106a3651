"""SMCMC_MODE_PER_CHAIN on the streamed one-chain-per-workgroup kernel (SMCMC_P_PERCHAIN_STREAM,
smcmc_perchain_stream.hip.h): the reference's own mode from dimension 64 to 512.  Checked lane by lane, bit for bit,
against oracle.Chain with the covariance adapting: accepted and proposed points, every lane scalar, centre, covariance
and decomposition.  No tolerances: this mode is bit parity or it is wrong.

The dimensions are the smallest at which this kernel can still go wrong: 100 and 156 overlap the register kernel, 157 is
the first only this kernel serves, 200 is BASELINE config 3's, 257 is past every 8-bit and 256-entry assumption of the
register kernel, 511 is odd with a ragged last batch, at 512 every thread owns a coordinate."""
import numpy as np
import pytest

from test_gpu_perchain_workgroup import _bad_covariance, _both, _same, _step, _window

pytestmark = pytest.mark.gpu

UNSUPPORTED = 5


def _error_matrix(dim):
    """QUADFORM's Error matrix of these tests: tridiagonal (three entries a row for the sparse walk), eigenvalues in
    [0.8, 2.2].  With oracle.like_params' header TDummy (eigenvalues 0.5 and 1e6) the reference chain itself accepts fewer
    than 12 moves in 200 steps once it has found the narrow direction: oracle.Chain alone makes 1 - 2 of the schedule's 3
    updates there, at every start tried, so that matrix cannot carry the schedule's own assertion."""
    e = np.diag(1.0 + 0.5 * (np.arange(dim) % 3))
    i = np.arange(dim - 1)
    e[i, i + 1] = e[i + 1, i] = 0.25
    return e.ravel()


def _make(gpu, oracle, dim, n, kind=0, which=None, seed=20240607, offset=0, x0=None, setup=None, dense=False, workgroup=False):
    prm = _error_matrix(dim) if kind == 1 else oracle.like_params(kind, dim)
    prm = prm if prm.size else None
    if workgroup:
        e = gpu.Engine(dim, n, likelihood=kind, likelihood_params=prm, seed=seed, chain_offset=offset,
                       mode=gpu.MODE_PER_CHAIN, perchain_workgroup=True)
        assert e.get_param("PERCHAIN_WORKGROUP") == 1 and e.get_param("PERCHAIN_STREAM") == 0
    else:
        e = gpu.Engine(dim, n, likelihood=kind, likelihood_params=prm, seed=seed, chain_offset=offset,
                       mode=gpu.MODE_PER_CHAIN, perchain_stream=True)
        assert e.get_param("PERCHAIN_STREAM") == 1
        assert e.get_param("PERCHAIN_WORKGROUP") == 0 and e.get_param("PERCHAIN_WAVE") == 0
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


def _start_points(kind, dim, n):
    # (ASYM away from its peak at the origin, where every move is downhill and the reference chain accepts too few moves
    # for the schedule: oracle.Chain alone makes 0 - 1 of its 3 updates from there)
    rng = np.random.default_rng(dim + 7 * kind)
    return {2: rng.uniform(0.5, 1.5, size=(dim, n)), 4: rng.uniform(0.5, 1.5, size=(dim, n)), 5: rng.uniform(-0.5, 0.5, size=(dim, n)) / np.sqrt(dim),
            6: 76.0 + rng.normal(0.0, 1.0, size=(dim, n))}.get(kind, np.zeros(dim))


def _schedule(e, chains):
    _same(e, chains, "start")
    _step(e, chains, 1)
    _same(e, chains, "first step")
    updates0 = e.lane("update_count").copy()
    for k in range(3):
        _both(e, chains, "SetNextUpdate", "set_next_update", 12)
        _step(e, chains, 200)
        _same(e, chains, f"forced schedule {k}")
    grown = np.median(e.lane("update_count") - updates0)
    print("median growth of update_count:", grown)
    assert grown >= 3, "the launches must cross UpdateProposal events"
    _step(e, chains, 200)
    _same(e, chains, "free running")


CASES = [(0, 157, 5), (0, 257, 3), (0, 511, 3), (0, 512, 3), (2, 200, 3), ("dense", 157, 3), (1, 200, 3), (4, 157, 3),
         (5, 157, 3), (6, 157, 3)]


@pytest.mark.parametrize("kind,dim,n", CASES, ids=[f"{k}-{d}-{n}" for k, d, n in CASES])
def test_every_lane_is_the_reference_chain(gpu, oracle, kind, dim, n):
    dense = kind == "dense"
    kind = 1 if dense else kind
    e, chains = _make(gpu, oracle, dim, n, kind, x0=_start_points(kind, dim, n), dense=dense, setup=lambda o: _window(o, 150))
    _schedule(e, chains)


def test_across_a_tile_of_the_images(gpu, oracle):
    """70 chains: the second tile of the wavefront-tiled images and its ragged tail."""
    e, chains = _make(gpu, oracle, 157, 70, 0, which=(0, 63, 64, 69), setup=lambda o: _window(o, 150))
    _schedule(e, chains)


@pytest.mark.parametrize("dim", [100, 156])
def test_three_kernels_one_chain(gpu, oracle, dim):
    """Where the register kernel serves too, the streamed kernel, the register kernel and the oracle are the same chain
    in every image."""
    runs = []
    for workgroup in (True, False):
        e, chains = _make(gpu, oracle, dim, 3, 0, workgroup=workgroup, setup=lambda o: _window(o, 100))
        _both(e, chains, "SetNextUpdate", "set_next_update", 10)
        _step(e, chains, 400)
        _same(e, chains, f"workgroup={workgroup}")
        runs.append(e)
    a, b = runs
    assert np.array_equal(a.GetAccepted(), b.GetAccepted())
    for k in ("logl", "sigma", "acceptance", "update_count", "next_update"):
        assert np.array_equal(a.lane(k), b.lane(k))
    for c in range(3):
        for u, v in zip(a.chain_proposal(c), b.chain_proposal(c)):
            assert np.array_equal(u, v)
    assert np.all(b.lane("update_count") >= 2)


def test_below_its_range_the_default_kernels_run(gpu, oracle):
    """SMCMC_P_PERCHAIN_STREAM at dim 63 changes nothing: the one-chain-per-wavefront kernel runs, and is the chain."""
    dim = 63
    e = gpu.Engine(dim, 3, mode=gpu.MODE_PER_CHAIN, perchain_stream=True)
    assert e.get_param("PERCHAIN_STREAM") == 0 and e.get_param("PERCHAIN_WAVE") == 1
    chains = {c: oracle.Chain(dim, chain_id=c) for c in range(3)}
    assert e.Start(np.zeros(dim))
    for ch in chains.values():
        assert ch.start(np.zeros(dim))
    _both(e, chains, "SetNextUpdate", "set_next_update", 10)
    _step(e, chains, 100)
    _same(e, chains, "dim 63")


@pytest.mark.parametrize("per_launch,eigen", [(60, False), (1, False), (60, True)],
                         ids=["inside-a-launch", "last-step-of-a-launch", "eigen-rung"])
def test_the_fallback_ladder(gpu, oracle, per_launch, eigen):
    """A covariance with no Cholesky factor: a numerical failure the reference handles with its ladder, on the host here."""
    dim = 157
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
    dim = 157
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


def test_snapshot_and_rollback(gpu, oracle):
    """20 steps, snapshot, 30 steps, rollback, 30 steps: the same bits as 50 straight (the working copies are not part of
    a snapshot: every launch reads the images)."""
    dim = 157
    e, chains = _make(gpu, oracle, dim, 3, 0, setup=lambda o: _window(o, 150))
    _both(e, chains, "SetNextUpdate", "set_next_update", 8)
    e.Step(20)
    e.snapshot()
    e.Step(30)
    e.rollback()
    e.Step(30)
    for ch in chains.values():
        ch.run_quiet(50)
    assert np.all(e.lane("update_count") >= 1)
    _same(e, chains, "50 steps through a rollback")


def test_step_recorded_is_the_chain_step_by_step(gpu, oracle):
    dim, n, nsteps, c = 200, 3, 150, 1
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


def test_saved_trace(gpu, oracle):
    """StepSave(6, stride = 2): the slots are the chain's points after steps 2, 4 and 6; the rows from dim on are zero."""
    import torch
    dim, n = 157, 3
    e, chains = _make(gpu, oracle, dim, n, 0)
    npad, dpad = e.nchains_padded, e.dim_padded
    sx = torch.zeros((3, dpad, npad), dtype=torch.float64, device="cuda")
    sl = torch.zeros((3, npad), dtype=torch.float64, device="cuda")
    e.StepSave(6, sx.data_ptr(), sl.data_ptr(), stride=2)
    torch.cuda.synchronize()
    xs, logl = sx.cpu().numpy(), sl.cpu().numpy()
    for slot in range(3):
        for ch in chains.values():
            ch.run_quiet(2)
        for c, ch in chains.items():
            assert np.array_equal(xs[slot, :dim, c], ch.accepted), f"slot {slot} chain {c}"
            assert logl[slot, c] == ch.scalars["accepted_logl"], f"slot {slot} chain {c}: logl"
        assert not xs[slot, dim:, :].any(), f"slot {slot}: rows from dim on"
    _same(e, chains, "after the saved launch")


def test_sharding(gpu, oracle):
    dim, n = 157, 6
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


def test_refusals(gpu):
    with pytest.raises(gpu.SmcmcError) as err:
        gpu.Engine(157, 2, mode=gpu.MODE_PER_CHAIN, perchain_workgroup=True)      # without the parameter: as before
    assert err.value.status == UNSUPPORTED
    with pytest.raises(gpu.SmcmcError):
        gpu.Engine(513, 2, mode=gpu.MODE_PER_CHAIN, perchain_stream=True)         # at create
    e = gpu.Engine(157, 2, mode=gpu.MODE_PER_CHAIN, perchain_stream=True, exact=False)
    with pytest.raises(gpu.SmcmcError) as err:
        e.Start(np.zeros(157))
    assert err.value.status == UNSUPPORTED
    e = gpu.Engine(157, 2, mode=gpu.MODE_PER_CHAIN, perchain_stream=True)
    e.SetUniform(2, -1.0, 1.0)
    with pytest.raises(gpu.SmcmcError) as err:
        e.Start(np.zeros(157))
    assert err.value.status == UNSUPPORTED
    e = gpu.Engine(157, 2, mode=gpu.MODE_PER_CHAIN, perchain_stream=True)
    with pytest.raises(gpu.SmcmcError) as err:
        e.set_param("PERCHAIN_STREAM", 0)                         # above 156 nothing else runs the mode
    assert err.value.status == UNSUPPORTED
    e = gpu.Engine(157, 2)
    with pytest.raises(gpu.SmcmcError):
        e._check(e._lib.smcmc_set_mode(e._h, gpu.MODE_PER_CHAIN))  # not asked for: refused as before


def test_destroyed_engines_return_their_memory(gpu):
    """create -> Start at D = 512 with 64 chains -> 2 steps -> snapshot -> destroy, five times: the tile's images
    (67 MB + 134 MB), their snapshot and the working copies (2.1 MB per chain) all go back."""
    import gc
    import torch

    def one():
        e = gpu.Engine(512, 64, mode=gpu.MODE_PER_CHAIN, perchain_stream=True)
        assert e.Start(np.zeros(512))
        e.Step(2)
        e.snapshot()
        e.sync()
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
    assert free0 - free1 < 24 << 20, f"{(free0 - free1) / 2**20:.1f} MiB not returned"
