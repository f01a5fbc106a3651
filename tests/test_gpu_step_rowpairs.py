"""The headline step kernels (D = 50 family, iso-Gaussian, reference order, triangular decomposition; with and without
the moment fold) keep the accepted point in row pairs in LDS (XLayout of csrc/smcmc_step_deal.h) and take the accept word
from the one Philox block that holds it for every dimension of the family (AcceptBlock).  All of it is data movement and
control: every case holds the engine to oracle.Ensemble bit for bit (oracle.Chain where a step is forced: the ensemble
oracle has no ForceStep).

Shapes, the smallest that reach the new code: D = 48, 49 and 50 are the family's dimensions -- accept words 48, 50 and
50: both word indices inside block 12, and its first word; at D = 49 the point's padding row 49 shares a pair with the
live row 48.  64 chains are one full wavefront; 70 leave a second one with 58 idle lanes, which must fold +0 through the
ones row and the zero row paired with it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F64 = ("logl", "sigma", "acceptance", "acceptance_trials", "rigidity", "step_rms", "logl_proposed")
I32 = ("trials", "successes", "next_update", "naccept", "step_rms_trials")
SHAPES = [(48, 64), (48, 70), (49, 64), (49, 70), (50, 64), (50, 70)]
MODES = pytest.mark.parametrize("pooled", [True, False], ids=["pooled", "frozen"])


def _pair(gpu, oracle, dim, nchains, pooled):
    mode = gpu.MODE_POOLED if pooled else gpu.MODE_FROZEN
    e = gpu.Engine(dim, nchains, likelihood=0, likelihood_params=None, seed=20250311, chain_offset=0, mode=mode, exact=True)
    o = oracle.Ensemble(nchains, dim, kind=0, params=None, seed=20250311, chain_offset=0, mode=mode, exact=True)
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
    # the accept word was drawn: some chains took a downhill proposal on a draw, others turned one away
    assert 0 < e.lane("naccept").sum() < 12 * nchains


@pytest.mark.parametrize("dim,nchains", [(48, 70), (49, 70), (50, 70)])
def test_one_step_launches_equal_one_launch(gpu, oracle, dim, nchains):
    """Step(1) five times = Step(5) = the oracle: the image is written by the prologue and read back by the epilogue of
    every launch."""
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
    """StepSave(4, stride = 2) reads the column back through the layout, row by row, behind the commit."""
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
    """ForceStep as the first step of a launch of four: the forced proposal is tested in front of the step loop (its accept
    word drawn there, by block number), committed through the layout, and the loop's first step reloads it.  Held to
    oracle.Chain with a frozen covariance (before the first update of the proposal a pooled chain is that chain); as in
    test_gpu_step_boundary.py next_update is compared in the frozen mode only, and of the pooled moments the number of
    folded points (a forced step folds nothing)."""
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


@MODES
@pytest.mark.parametrize("window", [0, 2])
def test_step_rms_window(gpu, oracle, window, pooled):
    """SetStepRMSWindow(0): the batch of the accepted point's rows is not read at all; (2): read every step, the trial
    count clamped from the second on."""
    dim, nchains = 49, 70
    e, o = _pair(gpu, oracle, dim, nchains, pooled)
    e.SetStepRMSWindow(window)
    o.set_step_rms_window(window)
    assert e.Start(np.zeros(dim)) and o.start(np.zeros(dim))
    rms0 = e.lane("step_rms").copy()
    e.Step(5)
    o.step(5)
    _assert_same_state(e, o, f"window {window}")
    if window == 0:
        assert np.array_equal(e.lane("step_rms"), rms0)
    else:
        assert (e.lane("step_rms_trials") == 2).all()
    if pooled:
        _assert_same_moments(e, o, 5 * nchains, f"window {window}")
