"""The step boundary of the D = 50 iso-Gaussian reference-order step kernels (BOUNDARY in csrc/smcmc_kernels.hip.h), with
and without the moment fold, runs the chains it ran.

Two things moved there, in the kernel with the fold, and neither may change a bit: coordinate 0 of the accepted point
is final before the step loop, and the reload of the accepted point into the proposal registers goes out at the top of a
step, behind the commit of the step before and in front of the scalar half of UpdateState.  The forced first step sets
the proposal itself in front of the loop, and StepSave reads the column behind the commit, with the next step's reload
behind it.  Every case holds the engine to oracle.Ensemble (oracle.Chain where a step is forced: the ensemble oracle has
no ForceStep) bit for bit, at the smallest shapes these paths have: one full wavefront, a ragged second group, the kernel below its padded dimension,
one-step launches, the StepRMS window clamped and off, the two Metropolis overrides, a saved trace."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F64 = ("logl", "sigma", "acceptance", "acceptance_trials", "rigidity", "step_rms", "logl_proposed")
I32 = ("trials", "successes", "next_update", "naccept", "step_rms_trials")


def _pair(gpu, oracle, dim, nchains, mode):
    e = gpu.Engine(dim, nchains, likelihood=0, likelihood_params=None, seed=20240607, chain_offset=0, mode=mode, exact=True)
    o = oracle.Ensemble(nchains, dim, kind=0, params=None, seed=20240607, chain_offset=0, mode=mode, exact=True)
    return e, o


def _assert_same_state(e, o, tag=""):
    assert np.array_equal(e.GetAccepted(), o.x), f"{tag}: accepted points differ"
    for name in F64:
        a, b = e.lane(name), o.lane(name)
        assert np.array_equal(a, b), f"{tag}: lane field {name} differs (max |d| = {np.max(np.abs(a - b))})"
    for name in I32:
        assert np.array_equal(e.lane(name), o.lane(name)), f"{tag}: lane field {name} differs"
    assert np.array_equal(e.lane("last_accept").astype(np.uint8), o.lane("last_accept")), f"{tag}: accept bits"


def _assert_same_moments(e, o, count, tag=""):
    e.reduce_moments()
    m_gpu, m_cpu = e.read_moments(), o.reduce_moments()
    assert np.array_equal(m_gpu, m_cpu), f"{tag}: moments differ, max |d| {np.max(np.abs(m_gpu - m_cpu))}"
    assert m_gpu[-1] == count, f"{tag}: {m_gpu[-1]} points folded, expected {count}"
    return m_cpu


@pytest.mark.parametrize("pooled", [True, False], ids=["pooled", "frozen"])
@pytest.mark.parametrize("dim,nchains", [(50, 64), (50, 100), (48, 70), (49, 70)])
def test_windows_match_oracle(gpu, oracle, dim, nchains, pooled):
    e, o = _pair(gpu, oracle, dim, nchains, gpu.MODE_POOLED if pooled else gpu.MODE_FROZEN)
    assert e.Start(np.zeros(dim)) and o.start(np.zeros(dim))
    for w in range(2):
        e.Step(3)
        o.step(3)
        _assert_same_state(e, o, f"window {w}")
        if pooled:
            m = _assert_same_moments(e, o, 3 * nchains, f"window {w}")
            e.apply_moments()
            o.apply_moments(m)
            assert np.array_equal(e.covariance, o.covariance)
            assert np.array_equal(e.GetEstimatedCenter(), o.center)
            assert np.array_equal(e.decomposition, o.decomposition)
            _assert_same_state(e, o, f"window {w}, after the update")
    e.Step(3)
    o.step(3)
    _assert_same_state(e, o, "after the last window")
    if pooled:
        _assert_same_moments(e, o, 3 * nchains, "after the last window")


def test_one_step_launches_equal_one_launch(gpu, oracle):
    """Step(1) five times = Step(5) = the oracle: every launch is a first and a last step at once, so coordinate 0 and the
    reload cross a launch boundary each time."""
    dim, nchains = 50, 100
    one, o = _pair(gpu, oracle, dim, nchains, gpu.MODE_POOLED)
    five, _ = _pair(gpu, oracle, dim, nchains, gpu.MODE_POOLED)
    assert one.Start(np.zeros(dim)) and five.Start(np.zeros(dim)) and o.start(np.zeros(dim))
    for _ in range(5):
        one.Step(1)
    five.Step(5)
    o.step(5)
    _assert_same_state(one, o, "five launches of one step")
    _assert_same_state(five, o, "one launch of five steps")
    m = _assert_same_moments(one, o, 5 * nchains, "five launches of one step")
    five.reduce_moments()
    assert np.array_equal(five.read_moments(), m)


@pytest.mark.parametrize("pooled", [True, False], ids=["pooled", "frozen"])
def test_step_rms_window_of_two(gpu, oracle, pooled):
    """SetStepRMSWindow(2): the window clamps rms_trials from the second step on."""
    dim, nchains = 50, 100
    e, o = _pair(gpu, oracle, dim, nchains, gpu.MODE_POOLED if pooled else gpu.MODE_FROZEN)
    e.SetStepRMSWindow(2)
    o.set_step_rms_window(2)
    assert e.Start(np.zeros(dim)) and o.start(np.zeros(dim))
    e.Step(5)
    o.step(5)
    _assert_same_state(e, o, "window of two")
    assert (e.lane("step_rms_trials") == 2).all()
    if pooled:
        _assert_same_moments(e, o, 5 * nchains, "window of two")


@pytest.mark.parametrize("pooled", [True, False], ids=["pooled", "frozen"])
def test_step_rms_window_off(gpu, oracle, pooled):
    """SetStepRMSWindow(0): neither the rows are read nor the sum is made; step_rms keeps its start value and nothing
    else notices."""
    dim, nchains = 50, 100
    mode = gpu.MODE_POOLED if pooled else gpu.MODE_FROZEN
    off, o = _pair(gpu, oracle, dim, nchains, mode)
    on, _ = _pair(gpu, oracle, dim, nchains, mode)
    off.SetStepRMSWindow(0)
    o.set_step_rms_window(0)
    assert off.Start(np.zeros(dim)) and on.Start(np.zeros(dim)) and o.start(np.zeros(dim))
    rms0, trials0 = off.lane("step_rms").copy(), off.lane("step_rms_trials").copy()
    off.Step(5)
    on.Step(5)
    o.step(5)
    _assert_same_state(off, o, "window off")
    assert np.array_equal(off.lane("step_rms"), rms0) and np.array_equal(off.lane("step_rms_trials"), trials0)
    assert not np.array_equal(on.lane("step_rms"), rms0)
    assert np.array_equal(off.GetAccepted(), on.GetAccepted())
    for name in F64 + I32 + ("last_accept",):
        if name not in ("step_rms", "step_rms_trials"):
            assert np.array_equal(off.lane(name), on.lane(name)), name
    if pooled:
        m = _assert_same_moments(off, o, 5 * nchains, "window off")
        on.reduce_moments()
        assert np.array_equal(on.read_moments(), m)


@pytest.mark.parametrize("pooled", [True, False], ids=["pooled", "frozen"])
@pytest.mark.parametrize("metropolis", [1, 2])
def test_metropolis_overrides(gpu, oracle, metropolis, pooled):
    """Step(n, 1) turns every downhill proposal away: coordinate 0 is carried and the proposal is reloaded from a column
    nobody wrote.  Step(n, 2) takes every proposal: every step commits."""
    dim, nchains, n = 50, 100, 4
    e, o = _pair(gpu, oracle, dim, nchains, gpu.MODE_POOLED if pooled else gpu.MODE_FROZEN)
    assert e.Start(np.zeros(dim)) and o.start(np.zeros(dim))
    e.Step(3)
    o.step(3)
    before = e.lane("naccept").copy()
    e.Step(n, metropolis=metropolis)
    o.step(n, metropolis)
    _assert_same_state(e, o, f"metropolis {metropolis}")
    taken = e.lane("naccept") - before
    if metropolis == 2:
        assert (taken == n).all()
    else:
        assert (taken < n).any()
    e.Step(2)
    o.step(2)
    _assert_same_state(e, o, f"metropolis {metropolis}, two plain steps later")
    if pooled:
        _assert_same_moments(e, o, (3 + n + 2) * nchains, f"metropolis {metropolis}")


@pytest.mark.parametrize("pooled", [True, False], ids=["pooled", "frozen"])
def test_forced_first_step_of_a_launch(gpu, oracle, pooled):
    """ForceStep, then a launch of four steps: the forced proposal is tested in front of the step loop, and the loop's
    first step reloads what that test left.  A point near the mode, then one far out that every chain turns away.
    oracle.Ensemble has no forced step; before the first update of the proposal a pooled chain is the reference chain
    with a frozen covariance, so both modes are held to oracle.Chain, field by field as _assert_same_state does -- chains
    of both groups, the last lane of the first and the last chain of the ragged one among them.  Two gaps against the
    other cases: next_update is compared in the frozen mode only (a pooled chain does not count it down; the ensemble
    oracle agrees), and of the pooled moments only the number of folded points is checked (a forced step folds nothing):
    their sums are in the matrix instructions' order, which the single-chain oracle does not have."""
    dim, nchains = 50, 100
    e = gpu.Engine(dim, nchains, mode=gpu.MODE_POOLED if pooled else gpu.MODE_FROZEN, exact=True)
    assert e.Start(np.zeros(dim))
    near, far = np.linspace(-0.2, 0.3, dim), np.full(dim, 10.0)
    e.Step(3)
    e.ForceStep(near)
    e.Step(4)
    after_near = e.GetAccepted()
    e.ForceStep(far)
    e.Step(2)
    x = e.GetAccepted()
    assert (e.lane("trials") == 3 + 3 + 1).all()            # a forced step leaves the proposal state alone (:671-678)
    fields = [("logl", "accepted_logl"), ("logl_proposed", "proposed_logl"), ("sigma", "sigma"), ("acceptance", "acceptance"),
              ("acceptance_trials", "acceptance_trials"), ("rigidity", "rigidity"), ("step_rms", "step_rms"),
              ("trials", "trials"), ("successes", "successes"), ("step_rms_trials", "step_rms_trials")]
    if not pooled:
        fields.append(("next_update", "next_update"))
    lanes = {lane: e.lane(lane) for lane, _ in fields}
    naccept, last_accept = e.lane("naccept"), e.lane("last_accept")
    for ch in (0, 63, 64, 99):
        c = oracle.Chain(dim, chain_id=ch)
        c.set_covariance_frozen(1)
        assert c.start(np.zeros(dim))
        taken = [c.step(False, 0) for _ in range(3)]
        c.force_step(near)
        taken += [c.step(False, 0) for _ in range(4)]
        assert np.array_equal(c.accepted, after_near[:, ch]), f"chain {ch}: after the forced step near the mode"
        c.force_step(far)
        taken += [c.step(False, 0) for _ in range(2)]
        assert not taken[7], f"chain {ch}: the oracle takes the point far out"
        assert np.array_equal(c.accepted, x[:, ch]), f"chain {ch}: after the forced step far out"
        sc = c.scalars
        for lane, name in fields:
            assert lanes[lane][ch] == sc[name], f"chain {ch}: {lane}"
        assert naccept[ch] == sum(taken), f"chain {ch}: naccept"
        assert bool(last_accept[ch]) == taken[-1], f"chain {ch}: accept bit of the last step"
    if pooled:
        e.reduce_moments()
        assert e.read_moments()[-1] == (3 + 3 + 1) * nchains


@pytest.mark.parametrize("pooled", [True, False], ids=["pooled", "frozen"])
def test_saved_trace(gpu, oracle, pooled):
    """StepSave(4, stride = 2): the slots hold the oracle's accepted points after steps 2 and 4 (the save reads the column
    behind the commit, with the next step's reload behind it)."""
    import torch
    dim, nchains, steps, stride = 50, 100, 4, 2
    e, o = _pair(gpu, oracle, dim, nchains, gpu.MODE_POOLED if pooled else gpu.MODE_FROZEN)
    assert e.Start(np.zeros(dim)) and o.start(np.zeros(dim))
    npad, dpad = e.nchains_padded, e.dim_padded
    sx = torch.zeros((steps // stride, dpad, npad), dtype=torch.float64, device="cuda")
    sl = torch.zeros((steps // stride, npad), dtype=torch.float64, device="cuda")
    e.StepSave(steps, sx.data_ptr(), sl.data_ptr(), stride=stride)
    torch.cuda.synchronize()
    for slot in range(steps // stride):
        o.step(stride)
        assert np.array_equal(sx[slot, :dim, :nchains].cpu().numpy(), o.x), f"slot {slot}: accepted points"
        assert np.array_equal(sl[slot, :nchains].cpu().numpy(), o.lane("logl")), f"slot {slot}: log-likelihoods"
    _assert_same_state(e, o, "after the saved launch")
    if pooled:
        _assert_same_moments(e, o, steps * nchains, "after the saved launch")
