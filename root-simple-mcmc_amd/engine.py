"""Host-side mirror of the reference's operator interface for the Step() path.

`Engine` is the many-chain counterpart of sMCMC::TSimpleMCMC<L, TProposeAdaptiveStep>
(reference TSimpleMCMC.H:185-590): the same verbs (Start, Step, SaveStep-style
read back, GetProposeStep()-style setters/getters named as in TSimpleMCMC.H:732-1003)
on top of the C ABI of include/smcmc.h.  All compute happens in the HIP library.
"""
import ctypes as C
import math

import numpy as np

from . import _capi
from ._capi import (LIKE_ASYM, LIKE_CONSTRAINED, LIKE_EVENT_SAMPLE, LIKE_EVENT_SHAPE, LIKE_EVENT_TEMPLATE, LIKE_HORRIFIC, LIKE_ISO_GAUSS, LIKE_QUADFORM, LIKE_ROSENBROCK, LIKE_USER, MODE_FROZEN, MODE_PER_CHAIN, MODE_POOLED, P,  # noqa: F401
                    SmcmcError)
# the reducers over a saved trace live in trace.py; their names stay importable from here
from .trace import (Autocorrelation, AutocorrelationGrid, AutocorrelationPlan, Convergence, MacroAutocorrelation, Marginals,  # noqa: F401
                    PosteriorPredictive, PredictiveCheck, TraceMoments, TraceQuantiles, TraceReducers, autocorrelation_plan,
                    cholesky_chain, event_predictive, order_keys, order_statistics_combined, order_values, poisson_draw,
                    predictive_check, quantile_ranks, trace_digit_counts, _event_data_shape, _f64, _order_statistics, _ptr)


class Engine(TraceReducers):
    """N chains of dimension D advancing in lock step on one GPU."""

    def __init__(self, dim, nchains=1, likelihood=LIKE_ISO_GAUSS, likelihood_params=None, seed=20240607,
                 chain_offset=0, device=0, mode=MODE_POOLED, exact=True, stream=None, library=None, perchain_workgroup=False,
                 perchain_stream=False):
        # library: path of a build that carries a user likelihood (LIKE_USER), see build.py --user-likelihood
        # perchain_workgroup: MODE_PER_CHAIN on the one-chain-per-workgroup kernel (SMCMC_P_PERCHAIN_WORKGROUP), the one
        # that serves dim > 63 (up to smcmc_max_perchain_dim())
        # perchain_stream: MODE_PER_CHAIN on the one-chain-per-workgroup kernel that streams the chain's matrices from
        # device memory (SMCMC_P_PERCHAIN_STREAM), 63 < dim <= smcmc_max_perchain_stream_dim()
        self._lib = _capi.load(library)
        self.dim, self.nchains = int(dim), int(nchains)
        self.seed, self.chain_offset = int(seed), int(chain_offset)
        h = C.c_void_p()
        st = self._lib.smcmc_create(self.dim, self.nchains, likelihood, seed, chain_offset, device, C.byref(h))
        self._h = h
        if st != _capi.OK:
            msg = self._lib.smcmc_last_error(h).decode() if h else self._lib.smcmc_status_string(st).decode()
            if h:
                self._lib.smcmc_destroy(h)
            self._h = None
            raise SmcmcError(st, msg)
        if perchain_workgroup:
            self.set_param("PERCHAIN_WORKGROUP", 1.0)
        if perchain_stream:
            self.set_param("PERCHAIN_STREAM", 1.0)
        self._check(self._lib.smcmc_set_mode(self._h, mode))
        self.mode = mode
        self.set_param("EXACT_ARITHMETIC", 1.0 if exact else 0.0)
        self.likelihood = int(likelihood)
        self._likelihood_params = None
        if likelihood_params is not None:
            prm = _f64(likelihood_params).ravel()
            self._check(self._lib.smcmc_set_likelihood_params(self._h, _ptr(prm), prm.size))
            self._likelihood_params = prm.copy()
        if stream is not None:
            self.set_stream(stream)

    # -- plumbing ---------------------------------------------------------
    def _check(self, st):
        if st != _capi.OK:
            raise SmcmcError(st, self._lib.smcmc_last_error(self._h).decode()
                             or self._lib.smcmc_status_string(st).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.smcmc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _event_histograms(self, who, like, name, evaluate, point):
        """(hist, logl) of one of the likelihoods over a simulated event sample, from its host evaluator"""
        if self.likelihood != like or self._likelihood_params is None:
            raise SmcmcError(_capi.ERR_LOGIC, "%s needs %s and its parameters" % (who, name))
        logl, hist = evaluate(self._likelihood_params, point, histograms=True)
        return hist, logl

    def EventSampleHistograms(self, point):
        """LIKE_EVENT_SAMPLE: the three simulated histograms [3][nbins] (Close, Separated, DecayTag) at `point`, as
        FakeLikelihood::WriteSimulation (example/FakeLikelihood.H:173-179) fills them, and the log-likelihood there:
        (hist, logl).  Evaluated on the host by smcmc_event_sample_evaluate, bit for bit what the device sums."""
        return self._event_histograms("EventSampleHistograms", LIKE_EVENT_SAMPLE, "LIKE_EVENT_SAMPLE", event_sample_evaluate, point)

    def EventTemplateHistograms(self, point):
        """LIKE_EVENT_TEMPLATE: the expectation [3][nbins] (Close, Separated, DecayTag) at `point`, as
        FakeLikelihood::WriteSimulation (example2/FakeLikelihood.H:201-207) fills it, and the log-likelihood there:
        (hist, logl).  Evaluated on the host by smcmc_event_template_evaluate, bit for bit what the device sums."""
        return self._event_histograms("EventTemplateHistograms", LIKE_EVENT_TEMPLATE, "LIKE_EVENT_TEMPLATE", event_template_evaluate, point)

    def EventShapeHistograms(self, point):
        """LIKE_EVENT_SHAPE: the expectation [4][nbins] (VeryClose, Close, Separated, DecayTag) at `point`, as
        FakeLikelihood::WriteSimulation (example3/FakeLikelihood.H:232-239) fills it, and the log-likelihood there:
        (hist, logl).  Evaluated on the host by smcmc_event_shape_evaluate, bit for bit what the device sums."""
        return self._event_histograms("EventShapeHistograms", LIKE_EVENT_SHAPE, "LIKE_EVENT_SHAPE", event_shape_evaluate, point)

    def PosteriorPredictive(self, trace_ptr, nslots, centre=None, histograms_ptr=None, logl_ptr=None, stream=0):
        """LIKE_EVENT_SAMPLE, _TEMPLATE, _SHAPE: the simulated histograms of the engine's likelihood at every point of a
        trace StepSave wrote, taken on the device (smcmc_event_predictive_sums) and summed per bin about `centre`
        ([NH][nbins]; default: the origin): WriteSimulation over the whole posterior, where the *Histograms methods
        above serve one point.  histograms_ptr / logl_ptr: optional device memory [nslots][NH nbins][nchains_padded] /
        [nslots][nchains_padded] that receives every point's histograms / log-likelihood.  Returns a
        PosteriorPredictive: mean and spread per bin, the band around the prediction."""
        if self.likelihood not in (LIKE_EVENT_SAMPLE, LIKE_EVENT_TEMPLATE, LIKE_EVENT_SHAPE) or self._likelihood_params is None:
            raise SmcmcError(_capi.ERR_LOGIC, "PosteriorPredictive needs LIKE_EVENT_SAMPLE, LIKE_EVENT_TEMPLATE or "
                                              "LIKE_EVENT_SHAPE and its parameters")
        return event_predictive(self.likelihood, self._likelihood_params, trace_ptr, nslots, self._trace_dim_stride,
                                self.nchains, self.nchains_padded, centre, histograms_ptr, logl_ptr, stream, _lib=self._lib)

    def PredictiveQuantiles(self, histograms_ptr, nslots, q=(0.025, 0.16, 0.5, 0.84, 0.975), stream=0):
        """The quantile band of every predicted bin: exact order statistics (smcmc_trace_order_statistics) over the
        device buffer [nslots][NH nbins][nchains_padded] that PosteriorPredictive(..., histograms_ptr=...) filled, one
        row per bin.  Returns a TraceQuantiles whose results are [NH][nbins]."""
        if self.likelihood not in (LIKE_EVENT_SAMPLE, LIKE_EVENT_TEMPLATE, LIKE_EVENT_SHAPE) or self._likelihood_params is None:
            raise SmcmcError(_capi.ERR_LOGIC, "PredictiveQuantiles needs LIKE_EVENT_SAMPLE, LIKE_EVENT_TEMPLATE or "
                                              "LIKE_EVENT_SHAPE and its parameters")
        _, nh, nbins = _event_data_shape(self.likelihood, self._likelihood_params)
        rows = nh * nbins
        return _order_statistics(self._lib, self._check, histograms_ptr, nslots, rows, rows, self.nchains, self.nchains_padded,
                                 quantile_ranks(int(nslots) * self.nchains, q), stream, shape=(nh, nbins))

    def PredictiveCheck(self, histograms_ptr, nslots, seed=None, replica=0, slot_offset=0, replicates_ptr=None,
                        statistics_ptr=None, stream=0):
        """The posterior-predictive check (smcmc_predictive_check) of the device buffer [nslots][NH nbins][nchains_padded]
        that PosteriorPredictive(..., histograms_ptr=...) filled, against the likelihood's own data: replicated data
        y_rep ~ Poisson(expectation) at every point, the bin term summed over them and over the data, one group per
        histogram.  seed: of the replicates (default: the engine's); replica: which of 2^16 independent sets; slot_offset:
        the global number of the buffer's first slot, for a window of a longer trace.  replicates_ptr / statistics_ptr:
        optional device memory [nslots][NH nbins][nchains_padded] / [nslots][2 (NH + 1)][nchains_padded] that receives the
        replicates (PredictiveQuantiles takes it: the band the data are expected in) / T_obs and T_rep.  Returns a
        PredictiveCheck: p-values per histogram and overall, and per bin how often the replicate fell below or on the data."""
        if self.likelihood not in (LIKE_EVENT_SAMPLE, LIKE_EVENT_TEMPLATE, LIKE_EVENT_SHAPE) or self._likelihood_params is None:
            raise SmcmcError(_capi.ERR_LOGIC, "PredictiveCheck needs LIKE_EVENT_SAMPLE, LIKE_EVENT_TEMPLATE or "
                                              "LIKE_EVENT_SHAPE and its parameters")
        header, nh, nbins = _event_data_shape(self.likelihood, self._likelihood_params)
        rows = nh * nbins
        return predictive_check(histograms_ptr, nslots, rows, self.nchains, self.nchains_padded,
                                self._likelihood_params[header:header + rows], nh, self.seed if seed is None else seed,
                                self.chain_offset, slot_offset, replica, replicates_ptr, statistics_ptr, stream, _lib=self._lib)

    def set_stream(self, stream):
        """stream: a raw hipStream_t value (e.g. torch.cuda.current_stream().cuda_stream)."""
        self._check(self._lib.smcmc_set_stream(self._h, C.c_void_p(int(stream))))

    @property
    def nchains_padded(self):
        return self._lib.smcmc_nchains_padded(self._h)

    @property
    def dim_padded(self):
        return self._lib.smcmc_dim_padded(self._h)

    @property
    def _trace_dim_stride(self):
        """TraceReducers: a slot StepSave wrote is [dim_padded][nchains_padded]."""
        return self.dim_padded

    # -- GetProposeStep() surface (TSimpleMCMC.H:732-1003) ------------------
    def set_param(self, name, value):
        self._check(self._lib.smcmc_set_param(self._h, P[name], float(value)))

    def get_param(self, name):
        out = C.c_double(0)
        self._check(self._lib.smcmc_get_param(self._h, P[name], C.byref(out)))
        return out.value

    def SetGaussian(self, dim, sigma):
        self._check(self._lib.smcmc_set_gaussian(self._h, dim, sigma))

    def SetUniform(self, dim, minimum, maximum):
        self._check(self._lib.smcmc_set_uniform(self._h, dim, minimum, maximum))

    def SetScanDimension(self, dim):
        self._check(self._lib.smcmc_set_scan_dimension(self._h, dim))

    def SetCorrelation(self, dim1, dim2, correlation):
        self._check(self._lib.smcmc_set_correlation(self._h, dim1, dim2, correlation))

    def ResetCorrelations(self):
        self._check(self._lib.smcmc_reset_correlations(self._h))

    def SetCovarianceWindow(self, w): self.set_param("COVARIANCE_WINDOW", w)
    def GetCovarianceWindow(self): return self.get_param("COVARIANCE_WINDOW")
    def SetCovarianceUpdateDeweighting(self, d): self.set_param("COVARIANCE_DEWEIGHT", d)
    def SetAcceptanceWindow(self, w): self.set_param("ACCEPTANCE_WINDOW", w)
    def GetAcceptanceWindow(self): return self.get_param("ACCEPTANCE_WINDOW")
    def SetAcceptanceUpdateDeweighting(self, d): self.set_param("ACCEPTANCE_DEWEIGHT", d)
    def SetAcceptanceRigidity(self, r): self.set_param("ACCEPTANCE_RIGIDITY", r)
    def GetAcceptanceRigidity(self): return self.get_param("ACCEPTANCE_RIGIDITY")
    def SetTargetAcceptance(self, a): self.set_param("TARGET_ACCEPTANCE", a)
    def GetTargetAcceptance(self): return self.get_param("TARGET_ACCEPTANCE")
    def SetSigma(self, s): self.set_param("SIGMA", s)
    def GetSigma(self, chain=None):
        """fSigma (TSimpleMCMC.H:770): of chain 0 by default, of `chain` otherwise."""
        return self.get_param("SIGMA") if chain is None else float(self.lane("sigma")[chain])
    def SetMaximumCorrelation(self, c): self.set_param("MAXIMUM_CORRELATION", c)
    def SetStepRMSWindow(self, n): self.set_param("STEP_RMS_WINDOW", n)
    def SetNextUpdate(self, n): self.set_param("NEXT_UPDATE", n)
    def GetNextUpdate(self): return self.get_param("NEXT_UPDATE")
    def GetCovarianceTrials(self): return self.get_param("COVARIANCE_TRIALS")
    def SetCovarianceTrials(self, v): self.set_param("COVARIANCE_TRIALS", v)
    def GetEstimatedCenterTrials(self): return self.get_param("CENTER_TRIALS")
    def SetEstimatedCenterTrials(self, v): self.set_param("CENTER_TRIALS", v)
    def GetCovarianceTrace(self): return self.get_param("COVARIANCE_TRACE")

    def UpdateProposal(self):
        self._check(self._lib.smcmc_update_proposal(self._h))

    def ResetProposal(self):
        self._check(self._lib.smcmc_reset_proposal(self._h))

    def ForceStep(self, point):
        point = _f64(point)
        self._check(self._lib.smcmc_force_step(self._h, _ptr(point), int(point.ndim == 1)))

    def GetEstimatedCenter(self):
        out = np.zeros(self.dim)
        self._check(self._lib.smcmc_get_center(self._h, _ptr(out)))
        return out

    def SetEstimatedCenter(self, v):
        v = _f64(v)
        if v.shape != (self.dim,):
            return False
        self._check(self._lib.smcmc_set_center(self._h, _ptr(v)))
        return True

    # -- TSimpleMCMC surface (TSimpleMCMC.H:246-532) ------------------------
    def Start(self, start):
        """start: [dim] (every chain) or [dim][nchains].  False = bad start (:265-268)."""
        start = _f64(start)
        broadcast = int(start.ndim == 1)
        if not broadcast and start.shape != (self.dim, self.nchains):
            raise ValueError("start must be [dim] or [dim][nchains]")
        st = self._lib.smcmc_start(self._h, _ptr(start), broadcast)
        if st == _capi.ERR_BAD_START:
            return False
        self._check(st)
        return True

    def SetCovarianceFrozen(self, frozen=True):
        """SetCovarianceFrozen (TSimpleMCMC.H:937) inside MODE_PER_CHAIN (MODE_FROZEN is the shared-decomposition form)."""
        self.set_param("COVARIANCE_FROZEN", 1.0 if frozen else 0.0)

    def chain(self, c=0):
        """One chain's members (smcmc_read_chain): dict with accepted, proposed (when kept) and every lane by name."""
        x, lf = np.zeros(self.dim), np.zeros(len(_capi.LANE_F64))
        li = np.zeros(len(_capi.LANE_I32), np.int32)
        keep = self.get_param("KEEP_PROPOSED") != 0.0
        prop = np.zeros(self.dim) if keep else None
        self._check(self._lib.smcmc_read_chain(self._h, int(c), _ptr(x), _ptr(prop) if keep else None, _ptr(lf),
                                               li.ctypes.data_as(C.POINTER(C.c_int32))))
        out = dict(accepted=x, proposed=prop)
        out.update({k: float(lf[i]) for k, i in _capi.LANE_F64.items()})
        out.update({k: int(li[i]) for k, i in _capi.LANE_I32.items()})
        return out

    def chain_proposal(self, c=0):
        """(fCentralPoint, fCurrentCov, fDecomposition) of chain c (MODE_PER_CHAIN: its own; else the shared ones)."""
        centre, cov, dec = np.zeros(self.dim), np.zeros((self.dim, self.dim)), np.zeros((self.dim, self.dim))
        self._check(self._lib.smcmc_read_chain_proposal(self._h, int(c), _ptr(centre), _ptr(cov), _ptr(dec)))
        return centre, cov, dec

    def saved_state(self, chain=0):
        """What SaveStep(true) writes for one chain (branches of TSimpleMCMC.H:208-215, 1616-1626):
        its point and scalar state plus the centre and covariance (the chain's own in MODE_PER_CHAIN, else shared)."""
        if self.mode == MODE_PER_CHAIN:
            ch = self.chain(chain)
            centre, cov, _ = self.chain_proposal(chain)
            return dict(accepted=ch["accepted"], log_likelihood=ch["logl"], total_steps=ch["chain_steps"],
                        step_rms=ch["step_rms"], trials=ch["trials"], successes=ch["successes"],
                        next_update=ch["next_update"], acceptance=ch["acceptance"],
                        acceptance_trials=ch["acceptance_trials"], sigma=ch["sigma"], central_point=centre,
                        central_point_trials=ch["center_trials"],
                        covariance=np.array([cov[i, j] for i in range(self.dim) for j in range(i + 1)]),
                        covariance_trials=ch["covariance_trials"])
        cov = self.covariance
        return dict(accepted=self.GetAccepted()[:, chain].copy(),
                    log_likelihood=float(self.GetAcceptedLogLikelihood()[chain]),
                    total_steps=int(self.get_param("TOTAL_STEPS")), step_rms=float(self.lane("step_rms")[chain]),
                    trials=int(self.lane("trials")[chain]), successes=int(self.lane("successes")[chain]),
                    next_update=int(self.lane("next_update")[chain]),
                    acceptance=float(self.lane("acceptance")[chain]),
                    acceptance_trials=float(self.lane("acceptance_trials")[chain]),
                    sigma=float(self.lane("sigma")[chain]), central_point=self.GetEstimatedCenter(),
                    central_point_trials=self.get_param("CENTER_TRIALS"),
                    covariance=np.array([cov[i, j] for i in range(self.dim) for j in range(i + 1)]),
                    covariance_trials=self.get_param("COVARIANCE_TRIALS"))

    def Restore(self, state, accepted=None):
        """Restore(tree) (TSimpleMCMC.H:282-352) from a saved_state() dict; `accepted` ([dim] or
        [dim][nchains]) overrides state["accepted"] as the point(s) to continue from."""
        x = _f64(state["accepted"] if accepted is None else accepted)
        broadcast = int(x.ndim == 1)
        if not broadcast and x.shape != (self.dim, self.nchains):
            raise ValueError("accepted must be [dim] or [dim][nchains]")
        centre, cov = _f64(state["central_point"]), _f64(state["covariance"])
        if centre.size != self.dim or cov.size != self.dim * (self.dim + 1) // 2:
            raise ValueError("saved centre / packed covariance have the wrong size")
        st = _capi.SavedState(state["log_likelihood"], state["total_steps"], state["step_rms"], state["trials"],
                              state["successes"], state["next_update"], state["acceptance"],
                              state["acceptance_trials"], state["sigma"], _ptr(centre),
                              state["central_point_trials"], _ptr(cov), state["covariance_trials"])
        self._check(self._lib.smcmc_restore(self._h, _ptr(x), broadcast, C.byref(st)))

    def Step(self, nsteps=1, metropolis=0):
        """nsteps x Step(save=false, metropolis) of every chain, one launch."""
        self._check(self._lib.smcmc_step(self._h, int(nsteps), int(metropolis)))

    def snapshot(self): self._check(self._lib.smcmc_snapshot(self._h))
    def rollback(self): self._check(self._lib.smcmc_rollback(self._h))

    def StepRecorded(self, nsteps, chain=0, metropolis=0):
        """nsteps x Step(false) in one launch with the per-step record of one chain (smcmc_step_recorded): a dict of
        arrays over the steps -- "accepted" / "proposed" [step][dim] and the scalars of smcmc_record_field."""
        stride = self._lib.smcmc_record_stride(self._h)
        rec = np.zeros((int(nsteps), stride))
        self._check(self._lib.smcmc_step_recorded(self._h, int(nsteps), int(metropolis), int(chain), _ptr(rec)))
        out = {"accepted": rec[:, :self.dim].copy(), "proposed": rec[:, self.dim:2 * self.dim].copy(),
               "covariance_diagonal": rec[:, 2 * self.dim:3 * self.dim].copy()}
        for k, name in enumerate(_capi.RECORD_FIELDS):
            out[name] = rec[:, 3 * self.dim + k].copy()
        # GetCovarianceTrace (TSimpleMCMC.H:961-967): the diagonal added up in index order
        out["covariance_trace"] = np.add.accumulate(out["covariance_diagonal"], axis=1)[:, -1]
        return out

    def StepSave(self, nsteps, save_x_ptr, save_logl_ptr, stride=1, metropolis=0):
        """As Step, also writing the accepted points into device buffers (raw pointers)."""
        self._check(self._lib.smcmc_step_save(self._h, int(nsteps), int(metropolis), int(stride),
                                              C.c_void_p(int(save_x_ptr)), C.c_void_p(int(save_logl_ptr))))

    def GetAccepted(self):
        x = np.zeros((self.dim, self.nchains))
        self._check(self._lib.smcmc_read_state(self._h, _ptr(x), None))
        return x

    def KeepProposed(self, on=True):
        """Leave the proposal of every launch's last step on the device for GetProposed()."""
        self.set_param("KEEP_PROPOSED", 1.0 if on else 0.0)

    def GetProposed(self):
        """fProposed (TSimpleMCMC.H:514) of every chain, [dim][nchains]; needs KeepProposed()."""
        x = np.zeros((self.dim, self.nchains))
        self._check(self._lib.smcmc_read_proposed(self._h, _ptr(x)))
        return x

    def GetAcceptedLogLikelihood(self):
        return self.lane("logl")

    def GetProposedLogLikelihood(self):
        return self.lane("logl_proposed")

    def GetStepRMS(self):
        return self.lane("step_rms")

    def lane(self, name):
        if name in _capi.LANE_F64:
            out = np.zeros(self.nchains)
            self._check(self._lib.smcmc_read_lane_f64(self._h, _capi.LANE_F64[name], _ptr(out)))
            return out
        out = np.zeros(self.nchains, np.int32)
        self._check(self._lib.smcmc_read_lane_i32(self._h, _capi.LANE_I32[name],
                                                  out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    # -- pooled adaptation ---------------------------------------------------
    @property
    def moments_size(self):
        return self._lib.smcmc_moments_size(self._h)

    def reduce_moments(self):
        self._check(self._lib.smcmc_reduce_moments(self._h))

    def export_moments(self, dst_device_ptr):
        self._check(self._lib.smcmc_export_moments(self._h, C.c_void_p(int(dst_device_ptr))))

    def import_moments(self, src_device_ptr):
        self._check(self._lib.smcmc_import_moments(self._h, C.c_void_p(int(src_device_ptr))))

    def apply_moments(self):
        self._check(self._lib.smcmc_apply_moments(self._h))

    # native RCCL communicator (include/smcmc.h): rank 0 makes the id, the caller hands it to the other ranks
    @staticmethod
    def comm_unique_id(library=None):
        buf = C.create_string_buffer(_capi.COMM_ID_BYTES)
        st = _capi.load(library).smcmc_comm_unique_id(buf)
        if st != _capi.OK:
            raise SmcmcError(st, "smcmc_comm_unique_id failed (is librccl.so loadable?)")
        return buf.raw

    def comm_init(self, unique_id, rank, nranks):
        buf = C.create_string_buffer(bytes(unique_id), _capi.COMM_ID_BYTES)
        self._check(self._lib.smcmc_comm_init(self._h, buf, int(rank), int(nranks)))

    def comm_ranks(self):
        """Ranks of the attached RCCL communicator as RCCL reports them (ncclCommCount); 0 without one."""
        return self._lib.smcmc_comm_ranks(self._h)

    def comm_destroy(self):
        self._check(self._lib.smcmc_comm_destroy(self._h))

    def allreduce_moments(self):
        self._check(self._lib.smcmc_allreduce_moments(self._h))

    def sync(self):
        self._check(self._lib.smcmc_sync(self._h))

    def read_moments(self):
        out = np.zeros(self.moments_size)
        self._check(self._lib.smcmc_read_moments(self._h, _ptr(out)))
        return out

    @property
    def covariance(self):
        out = np.zeros((self.dim, self.dim))
        self._check(self._lib.smcmc_get_covariance(self._h, _ptr(out)))
        return out

    def SetCovariance(self, cov):
        """Overwrite fCurrentCov ([dim][dim]); takes effect at the next UpdateProposal (the hook the reference's
        IMPOSE_RANDOM_CORRELATIONS experiment uses through SetCorrelation, SimpleMCMC.C:107-115)."""
        cov = _f64(cov)
        if cov.shape != (self.dim, self.dim):
            raise ValueError("covariance must be [dim][dim]")
        self._check(self._lib.smcmc_set_covariance(self._h, _ptr(cov)))

    @property
    def decomposition(self):
        out = np.zeros((self.dim, self.dim))
        self._check(self._lib.smcmc_get_decomposition(self._h, _ptr(out)))
        return out

    def state_device_ptr(self):
        x, l = C.c_void_p(), C.c_void_p()
        self._check(self._lib.smcmc_state_device_ptr(self._h, C.byref(x), C.byref(l)))
        return x.value, l.value


class PosteriorMoments:
    """Posterior mean / covariance of everything the ensemble visits (the reducers of
    MakeCovariance.C:63-89), fed by the pooled moment sums the device already forms:

        e.Step(window); e.reduce_moments(); acc.add(e); e.apply_moments()

    Each window's packed vector M holds n, sum(x - c0) and sum (x - c0)(x - c0)^T about the centre c0 the
    window ran with; they are re-centred on zero here and added up on the host (a few KB per window)."""

    def __init__(self, dim):
        self.dim = dim
        self.n = 0.0
        self.s1 = np.zeros(dim)
        self.s2 = np.zeros((dim, dim))

    def add(self, engine):
        D = self.dim
        m = engine.read_moments()
        c0 = engine.GetEstimatedCenter()
        tri = np.zeros((D + 1, D + 1))
        tri[np.tril_indices(D + 1)] = m
        n, s1 = tri[D, D], tri[D, :D]
        s2 = tri[:D, :D] + np.tril(tri[:D, :D], -1).T
        self.n += n
        self.s1 += s1 + n * c0
        self.s2 += s2 + np.outer(c0, s1) + np.outer(s1, c0) + n * np.outer(c0, c0)

    @property
    def mean(self):
        return self.s1 / self.n

    @property
    def covariance(self):
        mu = self.mean
        return self.s2 / self.n - np.outer(mu, mu)


def _event_evaluate(entry, what, dim, nh, max_bins, nparts, params, point, histograms, parts):
    """One of the three host evaluators of the likelihoods over a simulated event sample, `entry` of the library: nh
    histograms, a point of `dim` values, nparts doubles of intermediate stages (0: the entry takes none).  Returns
    (logL, nbins, hist or None, raw parts or None)."""
    lib = _capi.load()
    prm = _f64(params).ravel()
    pt = _f64(point).ravel()
    if pt.size != dim:
        raise SmcmcError(_capi.ERR_INVALID, what)
    nbins = int(prm[1]) if prm.size > 1 and np.isfinite(prm[1]) and 1 <= prm[1] <= max_bins else 1
    hist = np.zeros((nh, nbins))
    raw = np.zeros(2 * nh * nbins + nparts)
    logl = C.c_double(0.0)
    args = [_ptr(prm), prm.size, _ptr(pt), C.byref(logl), _ptr(hist) if histograms else None]
    if nparts:
        args.append(_ptr(raw) if parts else None)
    st = getattr(lib, entry)(*args)
    if st != _capi.OK:
        raise SmcmcError(st, lib.smcmc_event_sample_last_error().decode() or lib.smcmc_status_string(st).decode())
    return logl.value, nbins, hist if histograms else None, raw if parts else None


def _event_result(logl, nbins, nh, hist, raw, extra=None):
    """(logL, hist, parts) without what was not asked for; parts: S, B, IS, IB, ws, wb and what extra(tail) adds"""
    out = [logl]
    if hist is not None:
        out.append(hist)
    if raw is not None:
        t = raw[2 * nh * nbins:]
        d = {"S": raw[:nh * nbins].reshape(nh, nbins).copy(), "B": raw[nh * nbins:2 * nh * nbins].reshape(nh, nbins).copy(),
             "IS": float(t[0]), "IB": float(t[1]), "ws": float(t[2]), "wb": float(t[3])}
        if extra:
            d.update(extra(t))
        out.append(d)
    return out[0] if len(out) == 1 else tuple(out)


def event_sample_evaluate(params, point, histograms=False):
    """smcmc_event_sample_evaluate: LIKE_EVENT_SAMPLE at `point` (9 values) on the host, for the exposure ratio and the
    simulated histograms -- never to step a chain.  Returns logL, or (logL, hist[3][nbins]) with histograms=True."""
    logl, nbins, hist, _ = _event_evaluate("smcmc_event_sample_evaluate", "the event sample has nine parameters", 9, 3,
                                           _capi.EVENT_SAMPLE_MAX_BINS, 0, params, point, histograms, False)
    return _event_result(logl, nbins, 3, hist, None)


def event_template_evaluate(params, point, histograms=False, parts=False):
    """smcmc_event_template_evaluate: LIKE_EVENT_TEMPLATE at `point` (9 values) on the host -- never to step a chain.
    Returns logL; with histograms=True also the expectation mc[3][nbins] before the clamp; with parts=True also a dict of
    the intermediate stages: S[3][nbins], B[3][nbins] (the signal's and the background's histograms), IS, IB (their
    integrals), ws, wb (the two normalisations).  The order is (logL, hist, parts), without what was not asked for."""
    logl, nbins, hist, raw = _event_evaluate("smcmc_event_template_evaluate", "the event template has nine parameters", 9, 3,
                                             _capi.EVENT_SAMPLE_MAX_BINS, 4, params, point, histograms, parts)
    return _event_result(logl, nbins, 3, hist, raw)


def event_shape_evaluate(params, point, histograms=False, parts=False):
    """smcmc_event_shape_evaluate: LIKE_EVENT_SHAPE at `point` (31 values) on the host -- never to step a chain.
    Returns logL; with histograms=True also the expectation mc[4][nbins] before the clamp; with parts=True also a dict of
    the intermediate stages: S[4][nbins], B[4][nbins], IS, IB, ws, wb, penB, penS (the two shape penalties) and KinvB[11][11],
    KinvS[13][13] (the inverted kernels).  The order is (logL, hist, parts), without what was not asked for."""
    logl, nbins, hist, raw = _event_evaluate("smcmc_event_shape_evaluate", "the event shape has 31 parameters", 31, 4,
                                             _capi.EVENT_SHAPE_MAX_BINS, 6 + 121 + 169, params, point, histograms, parts)
    return _event_result(logl, nbins, 4, hist, raw, lambda t: {
        "penB": float(t[4]), "penS": float(t[5]), "KinvB": t[6:127].reshape(11, 11).copy(), "KinvS": t[127:296].reshape(13, 13).copy()})


def event_shape_kernel(low, high, n, coherence, sigma=1.0, exponential=False):
    """TFakeGP::GaussianKernel (TFakeGP.H:96-109; exponential=True: ExponentialKernel, :113-126) on n control bins over
    [low, high]: the n x n kernel matrix, entries whose exponent passes 20 exactly zero."""
    bw = (high - low) / n
    c = [low + i * bw + 0.5 * bw for i in range(n)]
    k = np.zeros((n, n))
    for i in range(n):
        for j in range(i, n):
            r = (c[i] - c[j]) / coherence
            r = abs(r) if exponential else 0.5 * r * r
            k[i, j] = k[j, i] = 0.0 if r > 20 else sigma * sigma * math.exp(-r)
    return k


def event_shape_params(events, data, nbins, xmin, xmax, kernel_b=None, kernel_s=None, cut_very_close=50.0, cut_close=100.0,
                       true_fakes=0.05, true_efficiency=0.5, bkg_range=(0.0, 500.0), sig_range=(0.0, 250.0)):
    """The flat parameter array of LIKE_EVENT_SHAPE (include/smcmc.h).  events: [nevents][6] (Mass, Type, Separation, MuDk,
    TrueMass, TrueMassSigma); data: [4][nbins] (VeryClose, Close, Separated, DecayTag); kernel_b [11][11] and kernel_s
    [13][13]: the kernel matrices of the two shapes, by default example3's (SystematicCorrection.H:151-163): Gaussian,
    coherence 100 and sigma 0.7 over the background's range, coherence 50 and sigma 1 over the signal's."""
    events = _f64(events).reshape(-1, 6)
    data = _f64(data).reshape(4, int(nbins))
    kb = event_shape_kernel(bkg_range[0], bkg_range[1], 11, 100.0, 0.7) if kernel_b is None else _f64(kernel_b).reshape(11, 11)
    ks = event_shape_kernel(sig_range[0], sig_range[1], 13, 50.0, 1.0) if kernel_s is None else _f64(kernel_s).reshape(13, 13)
    head = [events.shape[0], int(nbins), xmin, xmax, cut_very_close, cut_close, true_fakes, true_efficiency,
            bkg_range[0], bkg_range[1], sig_range[0], sig_range[1]]
    return np.concatenate([np.asarray(head, dtype=np.float64), data.ravel(), kb.ravel(), ks.ravel(), events.ravel()])


def event_sample_params(events, data, nbins, xmin, xmax, exposure_ratio=None, separation_cut=100.0, true_fakes=0.05,
                        true_efficiency=0.5):
    """The flat parameter array of LIKE_EVENT_SAMPLE (include/smcmc.h).  events: [nevents][6] (Mass, Type, Separation,
    MuDk, TrueMass, TrueMassSigma); data: [3][nbins] (Close, Separated, DecayTag).  exposure_ratio=None takes it as
    FakeLikelihood::Init does (example/FakeLikelihood.H:107-138): the simulated histograms at the origin with a ratio of
    1, then sum(data) / sum(mc), the histograms added up as TH1::Integral does it (bins ascending, Close + Separated +
    DecayTag)."""
    events = _f64(events).reshape(-1, 6)
    data = _f64(data).reshape(3, int(nbins))
    head = [events.shape[0], int(nbins), xmin, xmax, 1.0 if exposure_ratio is None else exposure_ratio, separation_cut,
            true_fakes, true_efficiency]
    prm = np.concatenate([np.asarray(head, dtype=np.float64), data.ravel(), events.ravel()])
    if exposure_ratio is None:
        _, hist = event_sample_evaluate(prm, np.zeros(9), histograms=True)

        def integral(h):
            s = 0.0
            for v in h:
                s += float(v)
            return s
        d = integral(data[0]) + integral(data[1]) + integral(data[2])
        m = integral(hist[0]) + integral(hist[1]) + integral(hist[2])
        prm[4] = d / m
    return prm


def selftest_detmath(kind, x, y=None, device=0):
    lib = _capi.load()
    x = _f64(x)
    out = np.empty_like(x)
    yy = _f64(y) if y is not None else None
    st = lib.smcmc_selftest_detmath(device, kind, x.size, _ptr(x), _ptr(yy) if yy is not None else None, _ptr(out))
    if st != _capi.OK:
        raise SmcmcError(st, lib.smcmc_status_string(st).decode())
    return out


def selftest_mfma(a, b, device=0):
    lib = _capi.load()
    a, b = _f64(a), _f64(b)
    K = a.shape[1]
    c = np.zeros((16, 16))
    st = lib.smcmc_selftest_mfma(device, K, _ptr(a), _ptr(b), _ptr(c))
    if st != _capi.OK:
        raise SmcmcError(st, lib.smcmc_status_string(st).decode())
    return c


def selftest_hmc_error_matrix(cov, est_trace, device=0):
    """UpdateErrorMatrix's eigenvalue step (TSimpleHMC.H:760-830) on one covariance: device >= 0 the per-chain HMC mode's
    device routine, device < 0 the pooled mode's host routine.  Returns (covariance after the repair loop, eigenvalues
    of the last pass, dict of max_scale, min_scale, passes, trace, orbit)."""
    lib = _capi.load()
    cov = _f64(cov)
    d = cov.shape[0]
    out = np.zeros(d * d + d + 5)
    st = lib.smcmc_selftest_hmc_error_matrix(int(device), d, float(est_trace), _ptr(cov), _ptr(out))
    if st != _capi.OK:
        raise SmcmcError(st, lib.smcmc_status_string(st).decode())
    tail = out[d * d + d:]
    return (out[:d * d].reshape(d, d), out[d * d:d * d + d],
            dict(zip(("max_scale", "min_scale", "passes", "trace", "orbit"), tail)))


def selftest_mfma_strip(a, b, device=0):
    lib = _capi.load()
    a, b = _f64(a), _f64(b)
    c = np.zeros((4, 16))
    st = lib.smcmc_selftest_mfma_strip(device, a.shape[1], _ptr(a), _ptr(b), _ptr(c))
    if st != _capi.OK:
        raise SmcmcError(st, lib.smcmc_status_string(st).decode())
    return c


class HmcEngine(TraceReducers):
    """N sMCMC::TSimpleHMC chains (reference TSimpleHMC.H:119-973) with the analytic gradient of a device
    likelihood.  SetMeanEpsilon(negative) + SetLeapFrog(n) fix the step: independent chains, many steps per launch.
    Otherwise every chain retunes its own step length and leapfrog count (:302-345) and the covariance-driven
    retuning (:665-858) is pooled over the ensemble every SetSyncInterval steps (mode=MODE_POOLED, the default) or
    kept by every chain for itself after each step, as the reference chain does (mode=MODE_PER_CHAIN)."""

    def __init__(self, dim, nchains=1, likelihood=LIKE_ISO_GAUSS, likelihood_params=None, seed=20240607,
                 chain_offset=0, device=0, stream=None, exact=True, library=None, mode=MODE_POOLED):
        # library: path of a build that carries a user likelihood (LIKE_USER as an HMC target through gradient type 2 / 3 / 5,
        # and through 0 / 1 / 4 when its header has a gradient: has_gradient)
        self._lib = _capi.load(library)
        self.dim, self.nchains = int(dim), int(nchains)
        h = C.c_void_p()
        st = self._lib.smcmc_hmc_create(self.dim, self.nchains, likelihood, seed, chain_offset, device, C.byref(h))
        self._h = h
        if st != _capi.OK:
            msg = self._lib.smcmc_hmc_last_error(h).decode() if h else self._lib.smcmc_status_string(st).decode()
            if h:
                self._lib.smcmc_hmc_destroy(h)
            self._h = None
            raise SmcmcError(st, msg)
        if likelihood_params is not None:
            prm = _f64(likelihood_params).ravel()
            self._check(self._lib.smcmc_hmc_set_likelihood_params(self._h, _ptr(prm), prm.size))
        if stream is not None:
            self._check(self._lib.smcmc_hmc_set_stream(self._h, C.c_void_p(int(stream))))
        if not exact:
            self._check(self._lib.smcmc_hmc_set_exact_arithmetic(self._h, 0))
        if mode != MODE_POOLED:
            self.SetMode(mode)

    def _check(self, st):
        if st != _capi.OK:
            raise SmcmcError(st, self._lib.smcmc_hmc_last_error(self._h).decode()
                             or self._lib.smcmc_status_string(st).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.smcmc_hmc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def SetAlpha(self, a): self._check(self._lib.smcmc_hmc_set_alpha(self._h, float(a)))
    def SetMeanEpsilon(self, e): self._check(self._lib.smcmc_hmc_set_mean_epsilon(self._h, float(e)))
    def SetLeapFrog(self, n): self._check(self._lib.smcmc_hmc_set_leapfrog(self._h, int(n)))

    def GetMeanEpsilon(self):
        out = C.c_double(0)
        self._check(self._lib.smcmc_hmc_get_mean_epsilon(self._h, C.byref(out)))
        return out.value

    def GetLeapFrog(self):
        """fLeapFrogSteps of chain 0, signed as the reference keeps it (negative = fixed by SetLeapFrog)."""
        out = C.c_int(0)
        self._check(self._lib.smcmc_hmc_get_leapfrog(self._h, C.byref(out)))
        return out.value

    def SetSyncInterval(self, steps): self._check(self._lib.smcmc_hmc_set_sync_interval(self._h, int(steps)))
    def TrackCovariance(self, on=True): self._check(self._lib.smcmc_hmc_set_track_covariance(self._h, int(on)))

    def SetGradientType(self, gradient_type):
        """Step(save, gradientType) of TSimpleHMC.H:279: 0 / 1 / 4 the likelihood's gradient, 2 covariant, 3 finite
        differences, 5 zero (PotentialGradient, :467-532)."""
        self._check(self._lib.smcmc_hmc_set_gradient_type(self._h, int(gradient_type)))

    def GetGradientType(self): return int(self._lib.smcmc_hmc_get_gradient_type(self._h))

    @property
    def has_gradient(self):
        """Are gradient types 0 / 1 / 4 served?  True for ISO_GAUSS, QUADFORM, ROSENBROCK and for a user library whose header
        defines smcmc_user_gradient_at; False for the stress targets and a user library without a gradient."""
        return bool(self._lib.smcmc_hmc_has_gradient(self._h))

    def SetGradientMatrix(self, G=None):
        """LIKE_QUADFORM: gradient types 0 / 1 / 4 compute g = -G q instead of -Error q from the next step on (BadGrad.C's
        GradientError; the potential stays that of Error).  None clears it.  Reference-order arithmetic only."""
        if G is None:
            self._check(self._lib.smcmc_hmc_set_gradient_matrix(self._h, None, 0))
            return
        g = _f64(G).ravel()
        self._check(self._lib.smcmc_hmc_set_gradient_matrix(self._h, _ptr(g), g.size))
    def sync(self): self._check(self._lib.smcmc_hmc_sync(self._h))

    def SetMode(self, mode):
        """MODE_POOLED or MODE_PER_CHAIN, before Start."""
        self._check(self._lib.smcmc_hmc_set_mode(self._h, int(mode)))

    def GetMode(self): return int(self._lib.smcmc_hmc_get_mode(self._h))

    def chain_tuning(self, c):
        """(fAveragePoint, fEstimatedCovariance, tuning dict) of chain c (MODE_PER_CHAIN: its own; else the shared ones)."""
        avg = np.zeros(self.dim)
        cov = np.zeros((self.dim, self.dim))
        tun = np.zeros(len(_capi.HMC_TUNING))
        self._check(self._lib.smcmc_hmc_read_chain_tuning(self._h, int(c), _ptr(avg), _ptr(cov), _ptr(tun)))
        return avg, cov, dict(zip(_capi.HMC_TUNING, tun))

    # the pooled update in pieces (a sharded ensemble adds the ranks' moment vectors between export and import)
    @property
    def moments_size(self): return self._lib.smcmc_hmc_moments_size(self._h)
    def reduce_moments(self): self._check(self._lib.smcmc_hmc_reduce_moments(self._h))
    def export_moments(self, dst_device_ptr): self._check(self._lib.smcmc_hmc_export_moments(self._h, C.c_void_p(int(dst_device_ptr))))
    def import_moments(self, src_device_ptr): self._check(self._lib.smcmc_hmc_import_moments(self._h, C.c_void_p(int(src_device_ptr))))
    def apply_moments(self): self._check(self._lib.smcmc_hmc_apply_moments(self._h))

    @property
    def moment_group(self):
        return self._lib.smcmc_hmc_moment_group(self._h)

    @property
    def tuning(self):
        out = np.zeros(len(_capi.HMC_TUNING))
        self._check(self._lib.smcmc_hmc_get_tuning(self._h, _ptr(out)))
        return dict(zip(_capi.HMC_TUNING, out))

    @property
    def average(self):
        out = np.zeros(self.dim)
        self._check(self._lib.smcmc_hmc_get_average_point(self._h, _ptr(out)))
        return out

    @property
    def covariance(self):
        out = np.zeros((self.dim, self.dim))
        self._check(self._lib.smcmc_hmc_get_covariance(self._h, _ptr(out)))
        return out

    def Start(self, start):
        start = _f64(start)
        broadcast = int(start.ndim == 1)
        if not broadcast and start.shape != (self.dim, self.nchains):
            raise ValueError("start must be [dim] or [dim][nchains]")
        self._check(self._lib.smcmc_hmc_start(self._h, _ptr(start), broadcast))

    def Step(self, nsteps=1, gradient_type=None):
        if gradient_type is not None:
            self.SetGradientType(gradient_type)
        self._check(self._lib.smcmc_hmc_step(self._h, int(nsteps)))

    def StepSave(self, nsteps, save_x_ptr, save_logl_ptr=None, stride=1):
        """As Step, and after every `stride`-th step of the call the accepted points go into the device buffer
        save_x[slot][dim][nchains_padded] and lane "logl" into save_logl[slot][nchains_padded] (raw pointers; save_logl_ptr
        may be None), from the launches that make the steps (smcmc_hmc_step_save)."""
        self._check(self._lib.smcmc_hmc_step_save(self._h, int(nsteps), int(stride), C.c_void_p(int(save_x_ptr)),
                                                  C.c_void_p(int(save_logl_ptr)) if save_logl_ptr else None))

    def snapshot(self): self._check(self._lib.smcmc_hmc_snapshot(self._h))
    def rollback(self): self._check(self._lib.smcmc_hmc_rollback(self._h))

    @property
    def record_stride(self): return self._lib.smcmc_hmc_record_stride(self._h)

    def StepRecorded(self, nsteps, chain=0):
        """nsteps x Step(false) of the ensemble (MODE_PER_CHAIN) with the per-step record of one chain
        (smcmc_hmc_step_recorded): an [nsteps, record_stride] array, a row = [0, dim) fAccepted, [dim, 2 dim) fAveragePoint,
        then the scalars HMC_RECORD_FIELDS, all after the step and the update that follows it."""
        rec = np.zeros((int(nsteps), self.record_stride))
        self._check(self._lib.smcmc_hmc_step_recorded(self._h, int(nsteps), int(chain), _ptr(rec)))
        return rec

    def state(self):
        q = np.zeros((self.dim, self.nchains))
        m = np.zeros((self.dim, self.nchains))
        logl = np.zeros(self.nchains)
        self._check(self._lib.smcmc_hmc_read_state(self._h, _ptr(q), _ptr(m), _ptr(logl)))
        return q, m, logl

    @property
    def nchains_padded(self): return self._lib.smcmc_hmc_nchains_padded(self._h)

    def copy_positions(self, dst_device_ptr):
        """fAccepted of every chain into a device buffer [dim][nchains_padded] (one slot of a trace), on the engine's stream."""
        self._check(self._lib.smcmc_hmc_copy_positions(self._h, C.c_void_p(int(dst_device_ptr))))

    @property
    def _trace_dim_stride(self):
        """TraceReducers: a slot StepSave or copy_positions wrote is [dim][nchains_padded]."""
        return self.dim

    def lane(self, name):
        if name in _capi.HMC_LANE_F64:
            out = np.zeros(self.nchains)
            self._check(self._lib.smcmc_hmc_read_lane_f64(self._h, _capi.HMC_LANE_F64[name], _ptr(out)))
            return out
        out = np.zeros(self.nchains, np.int32)
        self._check(self._lib.smcmc_hmc_read_lane_i32(self._h, _capi.HMC_LANE_I32[name],
                                                      out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out


class VaatEngine(TraceReducers):
    """N independent sMCMC::TSimpleMCMC<L, sMCMC::TProposeVAATStep> chains (reference TProposeVAATStep.H:22-307 driven
    by TSimpleMCMC::Step): one coordinate per step from a shuffled queue of the dimensions, a proposal width per
    dimension adapted to a 44 % acceptance.  Chain c is the reference chain on the random stream (seed, chain_offset + c)."""

    def __init__(self, dim, nchains=1, likelihood=LIKE_ISO_GAUSS, likelihood_params=None, seed=20240607,
                 chain_offset=0, device=0, stream=None, exact=True, library=None):
        # library: path of a build that carries a user likelihood (LIKE_USER), see build.py --user-likelihood
        self._lib = _capi.load(library)
        self.dim, self.nchains = int(dim), int(nchains)
        h = C.c_void_p()
        st = self._lib.smcmc_vaat_create(self.dim, self.nchains, likelihood, seed, chain_offset, device, C.byref(h))
        self._h = h
        if st != _capi.OK:
            msg = self._lib.smcmc_vaat_last_error(h).decode() if h else self._lib.smcmc_status_string(st).decode()
            if h:
                self._lib.smcmc_vaat_destroy(h)
            self._h = None
            raise SmcmcError(st, msg)
        if likelihood_params is not None:
            prm = _f64(likelihood_params).ravel()
            self._check(self._lib.smcmc_vaat_set_likelihood_params(self._h, _ptr(prm), prm.size))
        if stream is not None:
            self._check(self._lib.smcmc_vaat_set_stream(self._h, C.c_void_p(int(stream))))
        if not exact:
            self._check(self._lib.smcmc_vaat_set_exact_arithmetic(self._h, 0))

    def _check(self, st):
        if st != _capi.OK:
            raise SmcmcError(st, self._lib.smcmc_vaat_last_error(self._h).decode()
                             or self._lib.smcmc_status_string(st).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.smcmc_vaat_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- TProposeVAATStep's interface (GetProposeStep() of the reference) ----
    def SetUniform(self, dim, minimum, maximum):
        self._check(self._lib.smcmc_vaat_set_uniform(self._h, int(dim), float(minimum), float(maximum)))

    def SetGaussian(self, dim, sigma): self._check(self._lib.smcmc_vaat_set_gaussian(self._h, int(dim), float(sigma)))
    def SetAcceptanceWindow(self, a): self._check(self._lib.smcmc_vaat_set_acceptance_window(self._h, float(a)))
    def SetAcceptanceRigidity(self, r): self._check(self._lib.smcmc_vaat_set_acceptance_rigidity(self._h, float(r)))
    def SetStepRMSWindow(self, n): self._check(self._lib.smcmc_vaat_set_step_rms_window(self._h, int(n)))
    def UpdateProposal(self): self._check(self._lib.smcmc_vaat_update_proposal(self._h))

    def GetAcceptanceWindow(self):
        out = C.c_double(0)
        self._check(self._lib.smcmc_vaat_get_acceptance_window(self._h, C.byref(out)))
        return out.value

    def GetAcceptanceRigidity(self):
        out = C.c_double(0)
        self._check(self._lib.smcmc_vaat_get_acceptance_rigidity(self._h, C.byref(out)))
        return out.value

    def GetSuccesses(self, chain=0): return int(self.lane("successes")[chain])      # :151
    def GetTrials(self, chain=0): return int(self.lane("trials")[chain])            # :154
    def GetAcceptance(self, chain=0):                                               # :157-165: the mean over the dimensions
        a = self.per_dim("acceptance")[:, chain]
        return float(np.add.reduce(a) / a.size) if a.size else 0.0

    def GetSigma(self, chain=0):                                                    # :168-175
        s = self.per_dim("sigma")[:, chain]
        return float(np.add.reduce(s) / s.size) if s.size else 0.0

    # ---- TSimpleMCMC's interface ----
    def Start(self, start):
        start = _f64(start)
        broadcast = int(start.ndim == 1)
        if not broadcast and start.shape != (self.dim, self.nchains):
            raise ValueError("start must be [dim] or [dim][nchains]")
        st = self._lib.smcmc_vaat_start(self._h, _ptr(start), broadcast)
        if st == _capi.ERR_BAD_START:
            return False
        self._check(st)
        return True

    def Step(self, nsteps=1): self._check(self._lib.smcmc_vaat_step(self._h, int(nsteps)))

    def snapshot(self): self._check(self._lib.smcmc_vaat_snapshot(self._h))
    def rollback(self): self._check(self._lib.smcmc_vaat_rollback(self._h))

    @property
    def record_stride(self): return self._lib.smcmc_vaat_record_stride(self._h)

    def StepRecorded(self, nsteps, chain=0):
        """Step(nsteps) of every chain in one launch with the per-step record of one chain (smcmc_vaat_step_recorded):
        an [nsteps, record_stride] array, a row = the scalars VAAT_RECORD_FIELDS after that step.  A step moves the
        coordinate `index` to `accepted_value` and adapts the width of dimension `adapt_index` only, so the rows and the
        state before the call give the chain after every step."""
        rec = np.zeros((max(int(nsteps), 0), self.record_stride))
        self._check(self._lib.smcmc_vaat_step_recorded(self._h, int(nsteps), int(chain), _ptr(rec)))
        return rec

    def step_save(self, nsteps, stride, save_x_ptr, save_logl_ptr=None):
        self._check(self._lib.smcmc_vaat_step_save(self._h, int(nsteps), int(stride), C.c_void_p(int(save_x_ptr)),
                                                   C.c_void_p(int(save_logl_ptr)) if save_logl_ptr else None))

    @property
    def _trace_dim_stride(self):
        """TraceReducers: a slot step_save wrote is [dim][nchains_padded]."""
        return self.dim

    @property
    def total_steps(self): return self._lib.smcmc_vaat_total_steps(self._h)

    @property
    def queue_length(self): return self._lib.smcmc_vaat_queue_length(self._h)

    @property
    def nchains_padded(self): return self._lib.smcmc_vaat_nchains_padded(self._h)

    def GetAccepted(self):
        x = np.zeros((self.dim, self.nchains))
        self._check(self._lib.smcmc_vaat_read_state(self._h, _ptr(x), None))
        return x

    def lane(self, name):
        if name in _capi.VAAT_LANE_F64:
            out = np.zeros(self.nchains)
            self._check(self._lib.smcmc_vaat_read_lane_f64(self._h, _capi.VAAT_LANE_F64[name], _ptr(out)))
            return out
        out = np.zeros(self.nchains, np.int32)
        self._check(self._lib.smcmc_vaat_read_lane_i32(self._h, _capi.VAAT_LANE_I32[name],
                                                       out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def per_dim(self, name):
        """fSigma / fAcceptance / fAcceptanceTrials / fNextIndex as [dim][chain]."""
        if name in _capi.VAAT_DIM_F64:
            out = np.zeros((self.dim, self.nchains))
            self._check(self._lib.smcmc_vaat_read_dim_f64(self._h, _capi.VAAT_DIM_F64[name], _ptr(out)))
            return out
        out = np.zeros((self.dim, self.nchains), np.int32)
        self._check(self._lib.smcmc_vaat_read_dim_i32(self._h, _capi.VAAT_DIM_I32[name],
                                                      out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def state_device_ptr(self):
        x, logl = C.c_void_p(), C.c_void_p()
        self._check(self._lib.smcmc_vaat_state_device_ptr(self._h, C.byref(x), C.byref(logl)))
        return x.value, logl.value
