"""The headline step kernel with its matrix instructions dealt by plan (csrc/smcmc_step_deal.h) runs the chains it ran.

step_kernel<50, iso-Gaussian, reference order, triangular, moments> issues the 160 matrix instructions of the moment fold
in the plan's order instead of evenly by piece number.  Per accumulator tile the k-quads still ascend, so every sum keeps
its terms and their order: the cases below hold it to oracle.Ensemble bit for bit, as tests/test_gpu_parity.py's
test_pooled_iso_matches_oracle does for the other shapes -- one full wavefront, a ragged second group whose idle lanes
must fold +0, the same kernel below its padded dimension, the accumulators across one-step launches, and the same kernel
without the fold (MODE_FROZEN: no plan)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _pair(gpu, oracle, dim, nchains, mode):
    e = gpu.Engine(dim, nchains, likelihood=0, likelihood_params=None, seed=20240607, chain_offset=0, mode=mode, exact=True)
    o = oracle.Ensemble(nchains, dim, kind=0, params=None, seed=20240607, chain_offset=0, mode=mode, exact=True)
    return e, o


def _assert_same_state(e, o, tag=""):
    assert np.array_equal(e.GetAccepted(), o.x), f"{tag}: accepted points differ"
    for name in ("logl", "sigma", "acceptance", "acceptance_trials", "rigidity", "step_rms", "logl_proposed"):
        a, b = e.lane(name), o.lane(name)
        assert np.array_equal(a, b), f"{tag}: lane field {name} differs (max |d| = {np.max(np.abs(a - b))})"
    for name in ("trials", "successes", "next_update", "naccept", "step_rms_trials"):
        assert np.array_equal(e.lane(name), o.lane(name)), f"{tag}: lane field {name} differs"
    assert np.array_equal(e.lane("last_accept").astype(np.uint8), o.lane("last_accept")), f"{tag}: accept bits"


@pytest.mark.parametrize("dim,nchains,window,nwin", [(50, 64, 3, 2), (50, 100, 3, 2), (48, 70, 3, 2), (49, 64, 2, 2)])
def test_planned_deal_matches_oracle(gpu, oracle, dim, nchains, window, nwin):
    e, o = _pair(gpu, oracle, dim, nchains, gpu.MODE_POOLED)
    assert e.Start(np.zeros(dim)) and o.start(np.zeros(dim))
    for w in range(nwin):
        e.Step(window)
        o.step(window)
        _assert_same_state(e, o, f"window {w}")
        e.reduce_moments()
        m_gpu = e.read_moments()
        m_cpu = o.reduce_moments()
        assert np.array_equal(m_gpu, m_cpu), f"window {w}: moments differ, max |d| {np.max(np.abs(m_gpu - m_cpu))}"
        assert m_gpu[-1] == nchains * window
        e.apply_moments()
        o.apply_moments(m_cpu)
        assert np.array_equal(e.covariance, o.covariance)
        assert np.array_equal(e.GetEstimatedCenter(), o.center)
        assert np.array_equal(e.decomposition, o.decomposition)
        _assert_same_state(e, o, f"window {w}, after the update")
    e.Step(3); o.step(3)
    _assert_same_state(e, o, "after the last sync")


def test_one_step_launches_accumulate_like_one_launch(gpu):
    """Step(1) five times = Step(5): the accumulators leave and re-enter the kernel between launches, and every launch
    is a first and a last step at once."""
    dim, nchains = 50, 100
    one = gpu.Engine(dim, nchains, mode=gpu.MODE_POOLED, exact=True)
    five = gpu.Engine(dim, nchains, mode=gpu.MODE_POOLED, exact=True)
    assert one.Start(np.zeros(dim)) and five.Start(np.zeros(dim))
    for _ in range(5):
        one.Step(1)
    five.Step(5)
    assert np.array_equal(one.GetAccepted(), five.GetAccepted())
    for name in ("logl", "sigma", "step_rms", "naccept"):
        assert np.array_equal(one.lane(name), five.lane(name)), name
    one.reduce_moments(); five.reduce_moments()
    m1, m5 = one.read_moments(), five.read_moments()
    assert m1[-1] == 5 * nchains
    assert np.array_equal(m1, m5)


def test_frozen_kernel_without_the_plan_matches_oracle(gpu, oracle):
    dim, nchains = 50, 100
    e, o = _pair(gpu, oracle, dim, nchains, gpu.MODE_FROZEN)
    assert e.Start(np.zeros(dim)) and o.start(np.zeros(dim))
    for w in range(2):
        e.Step(3)
        o.step(3)
        _assert_same_state(e, o, f"launch {w}")
