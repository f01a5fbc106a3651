"""smcmc_hmc_step_save: an HMC run leaves its trace on the device from the launches that make the steps.  Three engines
with the same seed -- A: Step(1) in a loop with copy_positions and a read of lane "logl" at the save steps, B: one
StepSave, C: Step(nsteps) -- must agree bit for bit: B's trace is A's, the final state and every lane are the same in all
three, and nothing outside the live region of the trace is written (lanes >= nchains, the guard slot)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 20240607
F64_LANES = ("logl", "logl_proposed", "acceptance", "mean_epsilon", "reversal_len")
I32_LANES = ("naccept", "last_accept", "trials", "leapfrog", "contributes")


def _spd(dim, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((dim, dim)) / np.sqrt(dim)
    return a @ a.T + np.eye(dim)


def _params(kind, dim):
    return [100.0] if kind == 2 else (np.linalg.inv(_spd(dim, 3)) if kind == 1 else None)


def _start(kind, dim):
    return np.full(dim, 0.5) if kind == 1 else np.ones(dim)


def _make(gpu, kind, dim, nchains, exact=True, mode=None, fixed=True, gradient_type=0, sync=None):
    e = gpu.HmcEngine(dim, nchains, likelihood=kind, likelihood_params=_params(kind, dim), seed=SEED, exact=exact,
                      mode=gpu.MODE_POOLED if mode is None else mode)
    if sync is not None:
        e.SetSyncInterval(sync)
    e.Start(_start(kind, dim))
    if fixed:
        e.SetMeanEpsilon(-0.1)
        e.SetLeapFrog(3)
    if gradient_type:
        e.SetGradientType(gradient_type)
    return e


def _trace(e, slots):
    """NaN-filled device buffers with one guard slot more than `slots`"""
    x = torch.full((slots + 1, e.dim, e.nchains_padded), float("nan"), dtype=torch.float64, device="cuda")
    l = torch.full((slots + 1, e.nchains_padded), float("nan"), dtype=torch.float64, device="cuda")
    return x, l


def _everything(e):
    q, m, logl = e.state()
    out = {"q": q, "m": m}
    for k in F64_LANES + I32_LANES:
        out[k] = e.lane(k)
    return out


def _assert_same_state(a, b, tag):
    sa, sb = _everything(a), _everything(b)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), f"{tag}: {k}"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _three_engines(make, nsteps, stride):
    a, b, c = make(), make(), make()
    slots = nsteps // stride
    # A: the host loop
    ax, al = _trace(a, slots)
    for s in range(1, nsteps + 1):
        a.Step(1)
        if s % stride == 0 and s // stride <= slots:
            a.copy_positions(ax[s // stride - 1].data_ptr())
            al[s // stride - 1, :a.nchains] = torch.from_numpy(a.lane("logl")).cuda()
    # B: one call
    bx, bl = _trace(b, slots)
    b.StepSave(nsteps, bx.data_ptr(), bl.data_ptr(), stride=stride)
    c.Step(nsteps)
    torch.cuda.synchronize()
    n = a.nchains
    ax, al, bx, bl = (t.cpu().numpy() for t in (ax, al, bx, bl))
    assert slots >= 1
    assert np.array_equal(_bits(bx[:slots, :, :n]), _bits(ax[:slots, :, :n])), "trace"
    assert not np.isnan(bx[:slots, :, :n]).any()
    assert np.array_equal(_bits(bl[:slots, :n]), _bits(al[:slots, :n])), "save_logl"
    assert np.isnan(bx[:, :, n:]).all() and np.isnan(bl[:, n:]).all(), "a lane >= nchains was written"
    assert np.isnan(bx[slots]).all() and np.isnan(bl[slots]).all(), "the guard slot was written"
    _assert_same_state(a, b, "Step(1) loop against StepSave")
    _assert_same_state(c, b, "Step(nsteps) against StepSave")
    return a, b, bx, bl


FAMILIES = {  # kernel family: (likelihood, dim, chains, exact, gradient type)
    "w4": (0, 5, 70, True, 0),                     # two wave groups, ragged tail
    "generic": (0, 5, 70, True, 3),                # the GENERIC instantiation: finite differences
    "mfma1_reference": (1, 20, 64, True, 0),       # hmc_mfma_kernel<1, false>
    "mfma1_fused": (1, 20, 64, False, 0),          # hmc_mfma_kernel<1, true>
    "mfma2_fused": (1, 130, 64, False, 0),         # kMfTI = 2
    "w8": (2, 260, 64, True, 0),
}


@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_step_save_is_the_host_loop(gpu, family, stride):
    kind, dim, nchains, exact, gtype = FAMILIES[family]
    _three_engines(lambda: _make(gpu, kind, dim, nchains, exact=exact, gradient_type=gtype), 11, stride)


@pytest.mark.parametrize("mode", ["pooled_sync1", "pooled_sync4", "per_chain"])
def test_step_save_in_the_tuned_modes(gpu, oracle, mode):
    dim, nchains, nsteps, stride = 5, 70, 30, 3
    per_chain = mode == "per_chain"
    make = lambda: _make(gpu, 0, dim, nchains, fixed=False, mode=gpu.MODE_PER_CHAIN if per_chain else gpu.MODE_POOLED,
                         sync=None if per_chain else int(mode[-1]))
    a, b, bx, bl = _three_engines(make, nsteps, stride)
    if per_chain:
        # chains 0 and 69 of the trace are the reference chains after the same steps
        for c in (0, nchains - 1):
            h = oracle.Hmc(dim, seed=SEED, chain_id=c, potential_from_gradient=True)
            h.start(np.ones(dim))
            for slot in range(nsteps // stride):
                h.run(stride)
                assert np.array_equal(bx[slot, :, c], h.accepted), (c, slot)
                assert bl[slot, c] == -h.scalars["accepted_potential"], (c, slot)
        assert b.chain_tuning(0)[2] == a.chain_tuning(0)[2] and b.chain_tuning(69)[2] == a.chain_tuning(69)[2]


def test_the_phase_restarts_with_every_call(gpu):
    """two calls of 6 steps with stride 4 write one slot each: after steps 4 and 10"""
    make = lambda: _make(gpu, 0, 5, 70)
    a, b = make(), make()
    want = []
    for s in range(1, 13):
        a.Step(1)
        if s in (4, 10):
            want.append(a.state()[0])
    n = b.nchains
    for k in range(2):
        x, l = _trace(b, 1)
        b.StepSave(6, x.data_ptr(), l.data_ptr(), stride=4)
        torch.cuda.synchronize()
        x = x.cpu().numpy()
        assert np.array_equal(x[0, :, :n], want[k]), k
        assert np.isnan(x[1]).all() and np.isnan(l[1].cpu().numpy()).all()
    _assert_same_state(a, b, "two calls")


def test_fewer_steps_than_the_stride_write_nothing(gpu):
    make = lambda: _make(gpu, 0, 5, 70)
    a, b = make(), make()
    x, l = _trace(b, 0)
    b.StepSave(3, x.data_ptr(), None, stride=4)
    a.Step(3)
    torch.cuda.synchronize()
    assert torch.isnan(x).all() and torch.isnan(l).all()
    _assert_same_state(a, b, "3 steps")


def test_save_logl_may_be_null(gpu):
    make = lambda: _make(gpu, 0, 5, 70)
    a, b = make(), make()
    x, _ = _trace(b, 2)
    b.StepSave(5, x.data_ptr(), None, stride=2)
    a.Step(4)
    torch.cuda.synchronize()
    assert np.array_equal(x[1, :, :70].cpu().numpy(), a.state()[0])
    assert torch.isnan(x[2]).all()


def test_argument_errors_launch_nothing(gpu):
    e = _make(gpu, 0, 5, 70)
    e.Step(2)
    before = _everything(e)
    x, l = _trace(e, 2)
    lib, h = e._lib, e._h
    import ctypes as C
    xp, lp = C.c_void_p(x.data_ptr()), C.c_void_p(l.data_ptr())
    assert lib.smcmc_hmc_step_save(h, 2, 1, None, lp) == 1
    assert lib.smcmc_hmc_step_save(h, 2, 0, xp, lp) == 1
    assert lib.smcmc_hmc_step_save(h, -1, 1, xp, lp) == 1
    assert lib.smcmc_hmc_step_save(None, 2, 1, xp, lp) == 1
    fresh = gpu.HmcEngine(5, 70, seed=SEED)
    assert lib.smcmc_hmc_step_save(fresh._h, 2, 1, xp, lp) == 1          # not started
    torch.cuda.synchronize()
    assert torch.isnan(x).all() and torch.isnan(l).all()
    after = _everything(e)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert lib.smcmc_hmc_step_save(h, 0, 1, xp, lp) == 0                 # no steps: nothing to do
    assert torch.isnan(x).all()
