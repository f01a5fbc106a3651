"""The headline step kernel with the moment fold (D = 50 family, iso-Gaussian, reference order, triangular decomposition)
reads the tile rows past the ones row from the image's zero row (XLayout::ZERO_ROW of csrc/smcmc_step_deal.h) instead of
zeroing them with a select.  That changes no operand and no order: every case holds the engine to oracle.Ensemble bit for
bit (oracle.Chain where a step is forced: the ensemble oracle has no ForceStep).  The cases are the ones written for
the StepRMS terms taken block by block as well (StepRMS windows, a forced first step in front of the loop, the kernel
without the fold); that half was built, passed them, and is not in the kernels (profiles/step_rms_blocks_notes.md) --
they hold whatever takes its place to the same.

Shapes, the smallest that reach the code: D = 48, 49 and 50 are the family's dimensions (at 48 and 49 rows of the last
tile below the ones row are padding, +0; at 49 a padding row shares a pair with a live one).  64 chains are one full
wavefront; 70 leave a second one with 58 idle lanes, whose k-quads fold the zero row and the ones row's +0."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F64 = ("logl", "sigma", "acceptance", "acceptance_trials", "rigidity", "step_rms", "logl_proposed")
I32 = ("trials", "successes", "next_update", "naccept", "step_rms_trials")
SHAPES = [(48, 64), (48, 70), (49, 64), (49, 70), (50, 64), (50, 70)]
MODES = pytest.mark.parametrize("pooled", [True, False], ids=["pooled", "frozen"])


def _pair(gpu, oracle, dim, nchains, pooled):
    mode = gpu.MODE_POOLED if pooled else gpu.MODE_FROZEN
    e = gpu.Engine(dim, nchains, likelihood=0, likelihood_params=None, seed=20250917, chain_offset=0, mode=mode, exact=True)
    o = oracle.Ensemble(nchains, dim, kind=0, params=None, seed=20250917, chain_offset=0, mode=mode, exact=True)
    assert e.dim_padded == 50
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


@MODES
@pytest.mark.parametrize("dim,nchains", SHAPES)
def test_windows_of_six_steps(gpu, oracle, dim, nchains, pooled):
    e, o = _pair(gpu, oracle, dim, nchains, pooled)
    assert e.Start(np.zeros(dim)) and o.start(np.zeros(dim))
    for w in range(2):
        e.Step(6)
        o.step(6)
        _assert_same_state(e, o, f"window {w}")
        if pooled:
            m = _assert_same_moments(e, o, 6 * nchains, f"window {w}")
            e.apply_moments()
            o.apply_moments(m)
            assert np.array_equal(e.covariance, o.covariance)
            assert np.array_equal(e.GetEstimatedCenter(), o.center)
            assert np.array_equal(e.decomposition, o.decomposition)
            _assert_same_state(e, o, f"window {w}, after the update")
    assert 0 < e.lane("naccept").sum() < 12 * nchains
    assert (e.lane("step_rms") > 0).all()   # the default window: every step's sum went in


@MODES
@pytest.mark.parametrize("window", [0, 2, None], ids=["window0", "window2", "default"])
def test_step_rms_window(gpu, oracle, window, pooled):
    """SetStepRMSWindow(0): step_rms and its trial count stay as Start left them; (2): the sum goes in every step, the trial
    count clamped from the second step on; the default window: never clamped in five steps."""
    dim, nchains = 49, 70
    e, o = _pair(gpu, oracle, dim, nchains, pooled)
    if window is not None:
        e.SetStepRMSWindow(window)
        o.set_step_rms_window(window)
    assert e.Start(np.zeros(dim)) and o.start(np.zeros(dim))
    rms0, trials0 = e.lane("step_rms").copy(), e.lane("step_rms_trials").copy()
    e.Step(5)
    o.step(5)
    _assert_same_state(e, o, f"window {window}")
    assert np.array_equal(e.lane("step_rms"), o.lane("step_rms"))
    assert np.array_equal(e.lane("step_rms_trials"), o.lane("step_rms_trials"))
    if window == 0:
        assert np.array_equal(e.lane("step_rms"), rms0) and np.array_equal(e.lane("step_rms_trials"), trials0)
    elif window == 2:
        assert (e.lane("step_rms_trials") == 2).all()
    else:
        assert (e.lane("step_rms_trials") == trials0 + 5).all()
    if pooled:
        _assert_same_moments(e, o, 5 * nchains, f"window {window}")


@pytest.mark.parametrize("dim,nchains", [(48, 70), (49, 70), (50, 70)])
def test_one_step_launches_equal_one_launch(gpu, oracle, dim, nchains):
    one, o = _pair(gpu, oracle, dim, nchains, True)
    five, _ = _pair(gpu, oracle, dim, nchains, True)
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


@MODES
@pytest.mark.parametrize("dim", [49, 50])
def test_saved_trace(gpu, oracle, dim, pooled):
    """StepSave(4, stride = 2): the save path reads the column behind the commit, in front of the next step's operand reads."""
    import torch
    nchains, steps, stride = 70, 4, 2
    e, o = _pair(gpu, oracle, dim, nchains, pooled)
    assert e.Start(np.zeros(dim)) and o.start(np.zeros(dim))
    npad, dpad = e.nchains_padded, e.dim_padded
    sx = torch.zeros((steps // stride, dpad, npad), dtype=torch.float64, device="cuda")
    sl = torch.zeros((steps // stride, npad), dtype=torch.float64, device="cuda")
    e.StepSave(steps, sx.data_ptr(), sl.data_ptr(), stride=stride)
    torch.cuda.synchronize()
    for slot in range(steps // stride):
        o.step(stride)
        assert np.array_equal(sx[slot, :dim, :nchains].cpu().numpy(), o.x), f"slot {slot}: accepted points"
        assert not sx[slot, dim:, :].cpu().numpy().any(), f"slot {slot}: padding rows"
        assert np.array_equal(sl[slot, :nchains].cpu().numpy(), o.lane("logl")), f"slot {slot}: log-likelihoods"
    _assert_same_state(e, o, "after the saved launch")
    if pooled:
        _assert_same_moments(e, o, steps * nchains, "after the saved launch")


@MODES
@pytest.mark.parametrize("dim", [48, 49])
def test_forced_first_step_of_a_launch(gpu, oracle, dim, pooled):
    """ForceStep as the first step of a launch of four: the forced proposal is finished in front of the step loop, and the
    three steps behind it read (and, pooled, fold through the operand reads) the point it committed.  Held to
    oracle.Chain with a frozen covariance (before the first update of the proposal a pooled chain is that chain);
    next_update is compared in the frozen mode only, and of the pooled moments the number of folded points (a forced step
    folds nothing)."""
    nchains = 70
    mode = gpu.MODE_POOLED if pooled else gpu.MODE_FROZEN
    e = gpu.Engine(dim, nchains, mode=mode, exact=True)
    assert e.Start(np.zeros(dim))
    near = np.linspace(-0.2, 0.3, dim)
    e.ForceStep(near)
    e.Step(4)
    x = e.GetAccepted()
    fields = [("logl", "accepted_logl"), ("logl_proposed", "proposed_logl"), ("sigma", "sigma"), ("acceptance", "acceptance"),
              ("acceptance_trials", "acceptance_trials"), ("rigidity", "rigidity"), ("step_rms", "step_rms"),
              ("trials", "trials"), ("successes", "successes"), ("step_rms_trials", "step_rms_trials")]
    if not pooled:
        fields.append(("next_update", "next_update"))
    lanes = {lane: e.lane(lane) for lane, _ in fields}
    naccept, last_accept = e.lane("naccept"), e.lane("last_accept")
    for ch in (0, 63, 64, 69):
        c = oracle.Chain(dim, chain_id=ch)
        c.set_covariance_frozen(1)
        assert c.start(np.zeros(dim))
        c.force_step(near)
        taken = [c.step(False, 0) for _ in range(4)]   # the first of them is the forced one
        assert np.array_equal(c.accepted, x[:, ch]), f"chain {ch}: accepted point"
        sc = c.scalars
        for lane, name in fields:
            assert lanes[lane][ch] == sc[name], f"chain {ch}: {lane}"
        assert bool(last_accept[ch]) == taken[-1], f"chain {ch}: accept bit of the last step"
        assert naccept[ch] == sum(taken), f"chain {ch}: naccept"
    if pooled:
        e.reduce_moments()
        assert e.read_moments()[-1] == 3 * nchains
