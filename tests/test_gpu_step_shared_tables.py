"""The headline step kernels (D = 50 family, iso-Gaussian, reference order, triangular decomposition; with and without
the moment fold) run as one workgroup of four wavefronts per CU: wavefront w of block b is chain group 4 b + w with an
LDS image of the accepted point of its own, the decomposition and the tables of the normal transform are held once per
workgroup, the tables in copies that a gather cannot conflict on (StepWorkgroupLds and NormalTableLayout of
csrc/smcmc_step_deal.h).  All of it is placement: every case holds the engine to oracle.Ensemble bit for bit
(oracle.Chain where a step is forced: the ensemble oracle has no ForceStep).

Shapes: D = 48, 49 and 50 are the family's dimensions.  64 and 70 chains are one and two wavefronts of one workgroup (the
other wavefronts lie past the last group: they stage, reach the barrier and end), 256 a full workgroup, 300 and 330 a
second workgroup with one and two live wavefronts, the last of them ragged."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F64 = ("logl", "sigma", "acceptance", "acceptance_trials", "rigidity", "step_rms", "logl_proposed")
I32 = ("trials", "successes", "next_update", "naccept", "step_rms_trials")
CHAINS = [64, 70, 256, 300, 330]
SHAPES = [(d, n) for d in (48, 49, 50) for n in CHAINS]
MODES = pytest.mark.parametrize("pooled", [True, False], ids=["pooled", "frozen"])


def _pair(gpu, oracle, dim, nchains, pooled):
    mode = gpu.MODE_POOLED if pooled else gpu.MODE_FROZEN
    e = gpu.Engine(dim, nchains, likelihood=0, likelihood_params=None, seed=20251021, chain_offset=0, mode=mode, exact=True)
    o = oracle.Ensemble(nchains, dim, kind=0, params=None, seed=20251021, chain_offset=0, mode=mode, exact=True)
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


@pytest.mark.parametrize("nchains", [70, 330])
@pytest.mark.parametrize("dim", [48, 49, 50])
def test_one_step_launches_equal_one_launch(gpu, oracle, dim, nchains):
    """Step(1) five times = Step(5) = the oracle: images, decomposition and tables are staged by every launch."""
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
@pytest.mark.parametrize("dim,nchains", [(49, 70), (50, 330)])
def test_saved_trace(gpu, oracle, dim, nchains, pooled):
    """StepSave(4, stride = 2): every live wavefront writes its own image's rows to the trace."""
    import torch
    steps, stride = 4, 2
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
        assert not sx[slot, :, nchains:].cpu().numpy().any(), f"slot {slot}: idle lanes"
        assert np.array_equal(sl[slot, :nchains].cpu().numpy(), o.lane("logl")), f"slot {slot}: log-likelihoods"
    _assert_same_state(e, o, "after the saved launch")
    if pooled:
        _assert_same_moments(e, o, steps * nchains, "after the saved launch")


@MODES
@pytest.mark.parametrize("dim,nchains", [(48, 70), (49, 330)])
def test_forced_first_step_of_a_launch(gpu, oracle, dim, nchains, pooled):
    """ForceStep as the first step of a launch of four, held to oracle.Chain with a frozen covariance (before the first
    update of the proposal a pooled chain is that chain); as in test_gpu_step_rowpairs.py next_update is compared in the
    frozen mode only, and of the pooled moments the number of folded points (a forced step folds nothing).  The chains
    are the first and last of a wavefront, of a workgroup and of the ensemble."""
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
    for ch in sorted({0, 63, 64, min(255, nchains - 1), min(256, nchains - 1), nchains - 1}):
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
    dim, nchains = 49, 330
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
