"""Host-side mirror of the reference's operator interface for the Step() path.

`Engine` is the many-chain counterpart of sMCMC::TSimpleMCMC<L, TProposeAdaptiveStep>
(reference TSimpleMCMC.H:185-590): the same verbs (Start, Step, SaveStep-style
read back, GetProposeStep()-style setters/getters named as in TSimpleMCMC.H:732-1003)
on top of the C ABI of include/smcmc.h.  All compute happens in the HIP library.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import (LIKE_ASYM, LIKE_CONSTRAINED, LIKE_HORRIFIC, LIKE_ISO_GAUSS, LIKE_QUADFORM, LIKE_ROSENBROCK, LIKE_USER, MODE_FROZEN, MODE_PER_CHAIN, MODE_POOLED, P,  # noqa: F401
                    SmcmcError)

_dp = C.POINTER(C.c_double)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    return a.ctypes.data_as(_dp)


class Engine:
    """N chains of dimension D advancing in lock step on one GPU."""

    def __init__(self, dim, nchains=1, likelihood=LIKE_ISO_GAUSS, likelihood_params=None, seed=20240607,
                 chain_offset=0, device=0, mode=MODE_POOLED, exact=True, stream=None, library=None, perchain_workgroup=False):
        # library: path of a build that carries a user likelihood (LIKE_USER), see build.py --user-likelihood
        # perchain_workgroup: MODE_PER_CHAIN on the one-chain-per-workgroup kernel (SMCMC_P_PERCHAIN_WORKGROUP), the one
        # that serves dim > 63 (up to smcmc_max_perchain_dim())
        self._lib = _capi.load(library)
        self.dim, self.nchains = int(dim), int(nchains)
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
        self._check(self._lib.smcmc_set_mode(self._h, mode))
        self.mode = mode
        self.set_param("EXACT_ARITHMETIC", 1.0 if exact else 0.0)
        if likelihood_params is not None:
            prm = _f64(likelihood_params).ravel()
            self._check(self._lib.smcmc_set_likelihood_params(self._h, _ptr(prm), prm.size))
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

    def set_stream(self, stream):
        """stream: a raw hipStream_t value (e.g. torch.cuda.current_stream().cuda_stream)."""
        self._check(self._lib.smcmc_set_stream(self._h, C.c_void_p(int(stream))))

    @property
    def nchains_padded(self):
        return self._lib.smcmc_nchains_padded(self._h)

    @property
    def dim_padded(self):
        return self._lib.smcmc_dim_padded(self._h)

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

    def AutocorrelationSums(self, trace_ptr, nslots, centre=None, stream=0):
        """Lagged-product sums of a trace StepSave wrote ([slot][dim_padded][nchains_padded] on the device), pooled
        over slots and chains about `centre` (default: the origin, as the macro has it): the inputs of the reference's
        autocorrelation (MakeAutocorrelation.C:108-148).  Returns an Autocorrelation."""
        c = _f64(np.zeros(self.dim) if centre is None else centre)
        s = np.zeros(self.dim)
        lagged = np.zeros((_capi.AUTOCORR_LAGS, self.dim))
        self._check(self._lib.smcmc_autocorrelation_sums(C.c_void_p(int(trace_ptr)), int(nslots), self.dim,
                                                         self.dim_padded, self.nchains, self.nchains_padded, _ptr(c),
                                                         _ptr(s), _ptr(lagged), C.c_void_p(int(stream))))
        return Autocorrelation(s, lagged, int(nslots), self.nchains)

    def AutocorrelationGrid(self, trace_ptr, nslots, lag_first=1, lag_step=1, nlags=64, centre=None, stream=0):
        """The pooled sums of a trace StepSave wrote on the lags lag_first + i lag_step, i < nlags, taken on the device
        (smcmc_autocorrelation_grid_sums): as far back along the chain as the caller asks, where AutocorrelationSums
        stops at lag 63.  More than 512 lags are taken in several calls.  Returns an AutocorrelationGrid."""
        return _autocorrelation_grid(self._lib, self._check, trace_ptr, nslots, self.dim, self.dim_padded, self.nchains,
                                     self.nchains_padded, lag_first, lag_step, nlags, centre, stream)

    def MakeAutocorrelation(self, trace_ptr, nslots, stream=0, centre=None, plan=None):
        """MakeAutocorrelation.C over a trace StepSave wrote: the macro's plan for entries = nslots
        (autocorrelation_plan), the device sums over the last `trials` slots on its lag grid, its bins.  centre: the
        reference point of the sums (default: the origin, as the macro has it).  plan: another AutocorrelationPlan for
        entries = nslots, e.g. autocorrelation_plan(nslots, depth, bins, precision) with constants of the caller's own.
        Returns a MacroAutocorrelation."""
        return _make_autocorrelation(self._lib, self._check, trace_ptr, nslots, self.dim, self.dim_padded, self.nchains,
                                     self.nchains_padded, centre, stream, plan)

    def Marginals(self, trace_ptr, nslots, n1=100, n2=50, pair_dims=None, sample_stride=None, ranges=None, stream=0):
        """The histograms of TestMarginalization.C over a trace StepSave wrote, counted on the device: the ranges of the
        dimensions over every sample_stride-th slot (default: the macro's stride; skipped when `ranges` = (lo, hi) is
        given, e.g. the merged ranges of several ranks), then n1 bins over [absMin, absMax) for every dimension and
        n2 x n2 bins for every ordered pair of pair_dims (default: the first min(dim, 10) dimensions) over the
        dimensions' ranges widened by 5 %.  Returns a Marginals."""
        return _marginals(self._lib, self._check, trace_ptr, nslots, self.dim, self.dim_padded, self.nchains,
                          self.nchains_padded, n1, n2, pair_dims, sample_stride, ranges, stream)

    def TraceMoments(self, trace_ptr, nslots, centre=None, stream=0):
        """The sums behind the mean and covariance of a trace StepSave wrote (MakeCovariance.C:63-89), taken on the
        device over every slot of every chain about `centre` (default: the origin, as the macro has it; the mean of
        the run conditions the covariance better).  Returns a TraceMoments."""
        return _trace_moments(self._lib, self._check, trace_ptr, nslots, self.dim, self.dim_padded, self.nchains,
                              self.nchains_padded, centre, stream)

    def Convergence(self, trace_ptr, nslots, nsegments=2, centre=None, stream=0):
        """The sums behind split R-hat and the multi-chain effective sample size of a trace StepSave wrote
        (smcmc_trace_convergence), taken on the device: every chain cut into `nsegments` segments (2: split R-hat, 1: the
        plain form), each about its own mean.  Pass a `centre` near the mean, e.g. TraceMoments(...).mean from one
        earlier pass: the variance of the segment means cancels like any E[yy] - E[y]^2.  Returns a Convergence."""
        return _convergence(self._lib, self._check, trace_ptr, nslots, self.dim, self.dim_padded, self.nchains,
                            self.nchains_padded, nsegments, centre, stream)

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


class Autocorrelation:
    """a(lag) = (E[x_t x_(t-lag)] - mean^2) / var per dimension (MakeAutocorrelation.C:127-139) from the pooled sums
    of Engine.AutocorrelationSums; sums of several ranks add (`+`)."""

    def __init__(self, total, lagged, nslots, nchains):
        self.sum, self.lagged, self.nslots, self.nchains = np.array(total), np.array(lagged), nslots, nchains

    def __add__(self, other):
        if self.nslots != other.nslots:
            raise ValueError("traces of different lengths do not pool")
        return Autocorrelation(self.sum + other.sum, self.lagged + other.lagged, self.nslots, self.nchains + other.nchains)

    def rho(self):
        """[lag][dim]"""
        nlag = min(self.lagged.shape[0], self.nslots)
        n = (self.nslots - np.arange(nlag))[:, None] * float(self.nchains)
        mean = self.sum / n[0]
        var = self.lagged[0] / n[0] - mean * mean
        return (self.lagged[:nlag] / n - mean * mean) / var

    def tau(self):
        """Integrated autocorrelation time per dimension in slots: 1 + 2 sum rho, the sum cut where a pair of
        consecutive lags turns negative (initial positive sequence)."""
        rho = self.rho()
        out = np.ones(rho.shape[1])
        for d in range(rho.shape[1]):
            for k in range(1, rho.shape[0] - 1, 2):
                pair = rho[k, d] + rho[k + 1, d]
                if pair < 0:
                    break
                out[d] += 2.0 * pair
        return out


class AutocorrelationGrid:
    """The pooled sums of smcmc_autocorrelation_grid_sums (include/smcmc.h) on the lags `lags` = lag_first + i lag_step:
    sum[dim], sumsq[dim] (lag 0) and lagged[lag][dim] about one reference point.
      counts   terms per lag, max(nslots - lag, 0) * nchains
      rho()    [lag][dim], (lagged / counts - mean^2) / (sumsq / n - mean^2); NaN for a lag beyond the trace
    Sums of several ranks add (`+`) when the grid and nslots agree."""

    def __init__(self, lags, total, sumsq, lagged, nslots, nchains):
        self.lags = np.array(lags, dtype=np.int64)
        self.sum, self.sumsq, self.lagged = _f64(total).copy(), _f64(sumsq).copy(), _f64(lagged).copy()
        self.nslots, self.nchains = int(nslots), int(nchains)
        if (self.lags.ndim != 1 or self.sum.ndim != 1 or self.sumsq.shape != self.sum.shape
                or self.lagged.shape != (self.lags.size, self.sum.size)):
            raise ValueError("lags[lag], sum[dim], sumsq[dim] and lagged[lag][dim] do not fit together")

    @property
    def counts(self):
        return np.maximum(self.nslots - self.lags, 0) * float(self.nchains)

    def __add__(self, other):
        if self.nslots != other.nslots:
            raise ValueError("traces of different lengths do not pool")
        if not np.array_equal(self.lags, other.lags):
            raise ValueError("sums on different lag grids do not add")
        return AutocorrelationGrid(self.lags, self.sum + other.sum, self.sumsq + other.sumsq, self.lagged + other.lagged,
                                   self.nslots, self.nchains + other.nchains)

    def rho(self):
        """[lag][dim]"""
        n = float(self.nslots) * self.nchains
        mean = self.sum / n
        var = self.sumsq / n - mean * mean
        with np.errstate(divide="ignore", invalid="ignore"):
            return (self.lagged / self.counts[:, None] - mean * mean) / var


def _autocorrelation_grid(lib, check, trace_ptr, nslots, dim, dim_stride, nchains, nchains_padded, lag_first, lag_step,
                          nlags, centre, stream):
    """The body of the engines' AutocorrelationGrid methods: calls of at most AUTOCORR_GRID_MAX_LAGS lags each, the rows
    concatenated (a row's bits do not depend on the call it is taken in)."""
    c = None if centre is None else _f64(centre)
    if c is not None and c.shape != (dim,):
        raise ValueError("centre must be [dim]")
    nslots, lag_first, lag_step, nlags = int(nslots), int(lag_first), int(lag_step), int(nlags)
    if nlags < 1:
        raise ValueError("nlags must be at least 1")
    total, sumsq, lagged = np.zeros(dim), np.zeros(dim), np.zeros((nlags, dim))
    for i0 in range(0, nlags, _capi.AUTOCORR_GRID_MAX_LAGS):
        n = min(_capi.AUTOCORR_GRID_MAX_LAGS, nlags - i0)
        rows = np.zeros((n, dim))
        check(lib.smcmc_autocorrelation_grid_sums(C.c_void_p(int(trace_ptr)), nslots, dim, dim_stride, nchains,
                                                  nchains_padded, None if c is None else _ptr(c),
                                                  lag_first + i0 * lag_step, lag_step, n, _ptr(total), _ptr(sumsq),
                                                  _ptr(rows), C.c_void_p(int(stream))))
        lagged[i0:i0 + n] = rows
    return AutocorrelationGrid(lag_first + lag_step * np.arange(nlags), total, sumsq, lagged, nslots, nchains)


class AutocorrelationPlan:
    """The constants MakeAutocorrelation.C derives from the number of entries (autocorrelation_plan): entries, depth,
    max_lag, bins, lag_step, trials, lags[lag], lag_bins[lag] (0-based bin of each lag) and bin_centres[bin]."""

    def __init__(self, entries, depth, max_lag, bins, lag_step, trials):
        self.entries, self.depth, self.max_lag, self.bins = entries, depth, max_lag, bins
        self.lag_step, self.trials = lag_step, trials
        self.lags = np.arange(1, max_lag, lag_step, dtype=np.int64)
        # the fixed-width axis of include/smcmc.h over [0, max_lag), filled at lag + 0.5 (:121)
        self.lag_bins = np.array([int(bins * (lag + 0.5) / max_lag) for lag in self.lags], dtype=np.int64)
        self.bin_centres = (np.arange(bins) + 0.5) * (float(max_lag) / bins)

    def __eq__(self, other):
        return (isinstance(other, AutocorrelationPlan)
                and (self.entries, self.depth, self.max_lag, self.bins, self.lag_step, self.trials)
                == (other.entries, other.depth, other.max_lag, other.bins, other.lag_step, other.trials))


def autocorrelation_plan(entries, depth=30000, bins=100, precision=0.01):
    """MakeAutocorrelation.C's constants for a tree of `entries` entries (:62, 70-73, 98-99, 104-106):
      maxLag  = min(int(entries - sqrt(entries)), depth)        bins    = min(bins, maxLag)
      lagStep = max(1, int(0.5 maxLag / bins))                  trials  = min(int(maxLag + 1 / precision^3), entries)
      lags 1, 1 + lagStep, ... < maxLag, each in bin int(bins (lag + 0.5) / maxLag).
    A pure function; returns an AutocorrelationPlan."""
    entries = int(entries)
    max_lag = min(int(entries - np.sqrt(float(entries))), int(depth)) if entries > 0 else 0
    if max_lag < 2:
        raise ValueError("the macro evaluates no lag below 4 entries")
    bins = min(int(bins), max_lag)
    lag_step = max(1, int(0.5 * max_lag / bins))
    trials = min(int(max_lag + 1.0 / (precision * precision * precision)), entries)
    return AutocorrelationPlan(entries, int(depth), max_lag, bins, lag_step, trials)


class MacroAutocorrelation:
    """What MakeAutocorrelation.C writes, from pooled device sums over the last plan.trials slots on the macro's lag
    grid (the engines' MakeAutocorrelation; from_sums is pure).  With n = trials * nchains and y = x - centre:
      bin_centres      [bin], the centres of the bins over [0, maxLag)
      mean[d]          centre + sum / n                                          (meanValues, :132)
      err2[d]          sumsq / n - (sum / n)^2: the "s" error of meanValues, squared (:133)
      autocorr[d][bin] (v / e - (sum / n)^2) / err2, v and e the sums of `lagged` and of `counts` over the lags that
                       fall into the bin (:135-139); a bin no lag falls into is 0/0 = NaN, as in the macro
      average[bin], spread[bin]   mean and population r.m.s. of autocorr over the dimensions (avgCorr, option "S", :146)
    Sums of several ranks add (`+`) when the plan and the centre agree.
    Deviations from the macro, on purpose (include/smcmc.h states them): its ring buffer holds floats, so every value is
    rounded to single precision before it is multiplied, and the values here are doubles; its TH1F sums are floats, and
    these are doubles; it reads one chain, and here the chains are pooled into one sum, so one chain is the macro.  The
    macro's reference point is the origin (centre = None); another centre changes autocorr only through the edges of
    the lagged sums, O(lag / trials)."""

    def __init__(self, plan, total, sumsq, lagged, nchains, centre=None):
        self.plan, self.nchains = plan, int(nchains)
        self.sum, self.sumsq, self.lagged = _f64(total).copy(), _f64(sumsq).copy(), _f64(lagged).copy()
        self.centre = np.zeros(self.sum.size) if centre is None else _f64(centre).copy()
        if (self.sum.ndim != 1 or self.sumsq.shape != self.sum.shape or self.centre.shape != self.sum.shape
                or self.lagged.shape != (plan.lags.size, self.sum.size)):
            raise ValueError("sum[dim], sumsq[dim], centre[dim] and lagged[lag][dim] do not fit the plan")

    @classmethod
    def from_sums(cls, plan, total, sumsq, lagged, nchains, centre=None):
        return cls(plan, total, sumsq, lagged, nchains, centre)

    def __add__(self, other):
        if self.plan != other.plan:
            raise ValueError("sums of different plans do not add")
        if not np.array_equal(self.centre, other.centre):
            raise ValueError("sums about different centres do not add")
        return MacroAutocorrelation(self.plan, self.sum + other.sum, self.sumsq + other.sumsq, self.lagged + other.lagged,
                                    self.nchains + other.nchains, self.centre)

    @property
    def counts(self):
        """[lag]: the macro's fills per lag (`fills <= lag` breaks, :118), times the chains"""
        return (self.plan.trials - self.plan.lags) * float(self.nchains)

    @property
    def bin_centres(self):
        return self.plan.bin_centres

    @property
    def _ymean(self):
        return self.sum / (float(self.plan.trials) * self.nchains)

    @property
    def mean(self):
        return self.centre + self._ymean

    @property
    def err2(self):
        m = self._ymean
        return self.sumsq / (float(self.plan.trials) * self.nchains) - m * m

    @property
    def autocorr(self):
        """[dim][bin]"""
        dim, bins = self.sum.size, self.plan.bins
        v, e = np.zeros((dim, bins)), np.zeros(bins)
        counts = self.counts
        for i, b in enumerate(self.plan.lag_bins):      # lags ascending, as the macro fills them
            v[:, b] += self.lagged[i]
            e[b] += counts[i]
        m = self._ymean
        with np.errstate(divide="ignore", invalid="ignore"):
            return (v / e[None, :] - (m * m)[:, None]) / self.err2[:, None]

    @property
    def average(self):
        return self.autocorr.mean(axis=0)

    @property
    def spread(self):
        return self.autocorr.std(axis=0)


def _make_autocorrelation(lib, check, trace_ptr, nslots, dim, dim_stride, nchains, nchains_padded, centre, stream, plan):
    """The body of the engines' MakeAutocorrelation methods."""
    if plan is None:
        plan = autocorrelation_plan(int(nslots))
    elif plan.entries != int(nslots):
        raise ValueError("the plan is for %d entries, the trace has %d slots" % (plan.entries, int(nslots)))
    first = int(trace_ptr) + 8 * (plan.entries - plan.trials) * dim_stride * nchains_padded   # the last `trials` slots
    g = _autocorrelation_grid(lib, check, first, plan.trials, dim, dim_stride, nchains, nchains_padded, 1, plan.lag_step,
                              plan.lags.size, centre, stream)
    return MacroAutocorrelation.from_sums(plan, g.sum, g.sumsq, g.lagged, nchains, centre)


class Marginals:
    """The marginal distributions of a trace as TestMarginalization.C histograms them, from the device counts of
    smcmc_trace_ranges / smcmc_marginal_histograms (include/smcmc.h has the bin rule):
      lo, hi [dim]                 the ranges of the dimensions over the sampled slots (macro :45-63)
      n1, lo1, hi1 [dim]; counts1 [dim][n1 + 2]               the 1-D axes and counts (0 / n1 + 1: under- / overflow)
      pair_dims [P]; n2, lo2, hi2 [P]; counts2 [P][P][n2 + 2][n2 + 2]   table (p, q): x = pair_dims[p], y = pair_dims[q]
    Counts are unsigned 64-bit integers and exact.  Counts of several ranks filled on identical axes add (`+`); their
    ranges combine beforehand with merge_ranges.  Everything derived here is host-side numpy."""

    def __init__(self, lo, hi, nslots, nchains, lo1=None, hi1=None, counts1=None, pair_dims=None, lo2=None, hi2=None,
                 counts2=None):
        self.lo, self.hi, self.nslots, self.nchains = _f64(lo), _f64(hi), int(nslots), int(nchains)
        self.lo1 = None if lo1 is None else _f64(lo1)
        self.hi1 = None if hi1 is None else _f64(hi1)
        self.counts1 = None if counts1 is None else np.array(counts1, dtype=np.uint64)
        self.pair_dims = None if pair_dims is None else np.array(pair_dims, dtype=np.int32)
        self.lo2 = None if lo2 is None else _f64(lo2)
        self.hi2 = None if hi2 is None else _f64(hi2)
        self.counts2 = None if counts2 is None else np.array(counts2, dtype=np.uint64)

    @property
    def n1(self): return 0 if self.counts1 is None else self.counts1.shape[1] - 2

    @property
    def n2(self): return 0 if self.counts2 is None else self.counts2.shape[2] - 2

    @staticmethod
    def _edges(lo, hi, n):
        return lo[:, None] + (hi - lo)[:, None] * (np.arange(n + 1) / float(n))[None, :]

    @property
    def edges1(self):
        """[dim][n1 + 1]: the bin edges of every 1-D axis (for plotting; the counting used the bin rule, not these)."""
        return None if self.counts1 is None else self._edges(self.lo1, self.hi1, self.n1)

    @property
    def edges2(self):
        """[P][n2 + 1]: the bin edges of the axis of every pair dimension."""
        return None if self.counts2 is None else self._edges(self.lo2, self.hi2, self.n2)

    @staticmethod
    def _same(a, b):
        return (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and np.array_equal(a, b))

    def __add__(self, other):
        if self.nslots != other.nslots:
            raise ValueError("traces of different lengths do not pool")
        for name in ("lo", "hi", "lo1", "hi1", "pair_dims", "lo2", "hi2"):
            if not self._same(getattr(self, name), getattr(other, name)):
                raise ValueError("histograms add only on identical bins and ranges (%s differs)" % name)
        if (self.n1, self.n2) != (other.n1, other.n2):
            raise ValueError("histograms add only on identical bins and ranges (the numbers of bins differ)")
        return Marginals(self.lo, self.hi, self.nslots, self.nchains + other.nchains, self.lo1, self.hi1,
                         None if self.counts1 is None else self.counts1 + other.counts1, self.pair_dims, self.lo2, self.hi2,
                         None if self.counts2 is None else self.counts2 + other.counts2)

    @staticmethod
    def merge_ranges(ranges):
        """(lo, hi) over several ranks' (lo, hi) pairs (or Marginals): the ranges of the whole ensemble."""
        pairs = [(r.lo, r.hi) if isinstance(r, Marginals) else (_f64(r[0]), _f64(r[1])) for r in ranges]
        lo, hi = pairs[0][0].copy(), pairs[0][1].copy()
        for a, b in pairs[1:]:
            lo, hi = np.minimum(lo, a), np.maximum(hi, b)
        return lo, hi

    @staticmethod
    def macro_sample_stride(nslots):
        """The stride of the macro's range loop (`entry += 0.001*entries` on an int, then ++entry; :54-62)."""
        return 1 + int(0.001 * int(nslots))

    @staticmethod
    def macro_axes(lo, hi, pair_dims):
        """The macro's axes from per-dimension ranges: ((absMin, absMax) of :52-53, 59-60, (lo2, hi2) of the pair
        dimensions: the dimension's range widened by 5 % of its width on both sides, :85-89)."""
        lo, hi = _f64(lo), _f64(hi)
        abs_min = min(1e20, float(np.min(lo)))
        abs_max = max(-1e20, float(np.max(hi)))
        p = np.asarray(pair_dims, dtype=np.int64)
        r = 0.05 * (hi[p] - lo[p])
        return (abs_min, abs_max), (lo[p] - r, hi[p] + r)

    def macro_ranges(self, pair_dims=None):
        """macro_axes of this object's ranges (pair_dims: its own, or the macro's first min(dim, 10) dimensions)."""
        if pair_dims is None:
            pair_dims = self.pair_dims if self.pair_dims is not None else np.arange(min(self.lo.size, 10))
        return self.macro_axes(self.lo, self.hi, pair_dims)

    def density(self, d):
        """[n1]: the in-range counts of dimension d over (all points x bin width): a density that integrates to the
        in-range fraction."""
        c = self.counts1[d].astype(np.float64)
        return c[1:-1] / (c.sum() * (self.hi1[d] - self.lo1[d]) / self.n1)

    def quantile(self, d, q):
        """The q-quantile of dimension d from its histogram: linear interpolation inside the bin where the cumulative
        count crosses q x (all points); underflow counts as sitting on lo1[d], overflow on hi1[d].  The resolution is
        one bin."""
        c = self.counts1[d].astype(np.float64)
        n, lo, hi = self.n1, float(self.lo1[d]), float(self.hi1[d])
        target = float(q) * c.sum()
        cum = np.cumsum(c[:-1])                 # cum[k]: points below edge k (the underflow included)
        if target <= cum[0]:
            return lo
        if target > cum[n]:
            return hi
        k = int(np.searchsorted(cum, target, side="left"))     # first edge with cum >= target: inside bin k
        return lo + (hi - lo) * ((k - 1) + (target - cum[k - 1]) / c[k]) / n

    def interval(self, d, level=0.68):
        """The central credible interval of dimension d holding `level` of the points (to one bin)."""
        return self.quantile(d, 0.5 * (1.0 - level)), self.quantile(d, 0.5 * (1.0 + level))


def _marginals(lib, check, trace_ptr, nslots, dim, dim_stride, nchains, nchains_padded, n1, n2, pair_dims, sample_stride,
               ranges, stream):
    """Ranges (unless given) and then the fill with the macro's axes: the body of the engines' Marginals methods."""
    up = C.POINTER(C.c_uint64)
    trace, nslots, st = C.c_void_p(int(trace_ptr)), int(nslots), C.c_void_p(int(stream))
    if pair_dims is None:
        pair_dims = np.arange(min(dim, 10))                        # the macro's "only doing 10" (:39-43)
    pair_dims = np.ascontiguousarray(pair_dims, dtype=np.int32)
    if ranges is None:
        if sample_stride is None:
            sample_stride = Marginals.macro_sample_stride(nslots)
        lo, hi = np.zeros(dim), np.zeros(dim)
        check(lib.smcmc_trace_ranges(trace, nslots, dim, dim_stride, nchains, nchains_padded, int(sample_stride), _ptr(lo),
                                     _ptr(hi), st))
    else:
        lo, hi = _f64(ranges[0]), _f64(ranges[1])
        if lo.shape != (dim,) or hi.shape != (dim,):
            raise ValueError("ranges must be (lo[dim], hi[dim])")
    (abs_min, abs_max), (lo2, hi2) = Marginals.macro_axes(lo, hi, pair_dims)
    lo1, hi1 = np.full(dim, abs_min), np.full(dim, abs_max)
    lo2, hi2 = _f64(lo2), _f64(hi2)
    P = int(pair_dims.size)
    counts1 = np.zeros((dim, n1 + 2), dtype=np.uint64) if n1 else None
    counts2 = np.zeros((P, P, n2 + 2, n2 + 2), dtype=np.uint64) if P else None
    check(lib.smcmc_marginal_histograms(trace, nslots, dim, dim_stride, nchains, nchains_padded, int(n1), _ptr(lo1), _ptr(hi1),
                                        counts1.ctypes.data_as(up) if n1 else None, P,
                                        pair_dims.ctypes.data_as(C.POINTER(C.c_int32)), int(n2), _ptr(lo2), _ptr(hi2),
                                        counts2.ctypes.data_as(up) if P else None, st))
    return Marginals(lo, hi, nslots, nchains, lo1 if n1 else None, hi1 if n1 else None, counts1,
                     pair_dims if P else None, lo2 if P else None, hi2 if P else None, counts2)


class TraceMoments:
    """The mean and covariance of a saved trace as MakeCovariance.C:63-89 takes them, from the raw sums of
    smcmc_trace_moments about `centre`: sum[d] = sum y_d, sumsq[i][j] = sum y_i y_j, y = x - centre, over
    n = nslots * nchains points.
      mean         centre + sum / n
      covariance   sumsq / n - (sum / n)(sum / n)^T: the macro's :84 taken about the centre (a covariance does not
                   depend on the point it is taken about; about a point near the mean the difference cancels less)
      spread       sqrt(diag covariance): the errors of the macro's TProfile in its "S" option (:58-60)
      correlation  covariance / (spread_i spread_j)
    Sums of several ranks add (`+`): the right operand is re-centred on the left one's centre first."""

    def __init__(self, total, sumsq, nslots, nchains, centre=None):
        self.sum, self.sumsq = _f64(total).copy(), _f64(sumsq).copy()
        self.nslots, self.nchains = int(nslots), int(nchains)
        self.centre = np.zeros(self.sum.size) if centre is None else _f64(centre).copy()
        if self.sumsq.shape != (self.sum.size, self.sum.size) or self.centre.shape != self.sum.shape:
            raise ValueError("sum[dim], sumsq[dim][dim] and centre[dim] do not fit together")

    @property
    def n(self):
        return float(self.nslots) * float(self.nchains)

    def about(self, centre):
        """The same sums taken about another point: with s = old centre - new centre, y' = y + s."""
        centre = _f64(centre)
        s, n = self.centre - centre, self.n
        total = self.sum + n * s
        sumsq = self.sumsq + np.outer(s, self.sum) + np.outer(self.sum, s) + n * np.outer(s, s)
        return TraceMoments(total, sumsq, self.nslots, self.nchains, centre)

    def __add__(self, other):
        if self.nslots != other.nslots:
            raise ValueError("traces of different lengths do not pool")
        o = other if np.array_equal(other.centre, self.centre) else other.about(self.centre)
        return TraceMoments(self.sum + o.sum, self.sumsq + o.sumsq, self.nslots, self.nchains + o.nchains, self.centre)

    @property
    def mean(self):
        return self.centre + self.sum / self.n

    @property
    def covariance(self):
        m = self.sum / self.n
        return self.sumsq / self.n - np.outer(m, m)

    @property
    def spread(self):
        return np.sqrt(np.diag(self.covariance))

    @property
    def correlation(self):
        s = self.spread
        return self.covariance / np.outer(s, s)


def _trace_moments(lib, check, trace_ptr, nslots, dim, dim_stride, nchains, nchains_padded, centre, stream):
    """The body of the engines' TraceMoments methods."""
    c = None if centre is None else _f64(centre)
    if c is not None and c.shape != (dim,):
        raise ValueError("centre must be [dim]")
    total, sumsq = np.zeros(dim), np.zeros((dim, dim))
    check(lib.smcmc_trace_moments(C.c_void_p(int(trace_ptr)), int(nslots), dim, dim_stride, nchains, nchains_padded,
                                  None if c is None else _ptr(c), _ptr(total), _ptr(sumsq), C.c_void_p(int(stream))))
    return TraceMoments(total, sumsq, nslots, nchains, c)


class Convergence:
    """Split R-hat and the multi-chain effective sample size of a saved trace, from the raw sums of
    smcmc_trace_convergence (include/smcmc.h has the definition): every chain is cut into segments of L slots, M
    segment-chains in all, y = x - centre, s1_m the sum of segment-chain m and z = y - s1_m / L:
      sum[d] = sum_m s1_m,  sumsq_of_sums[d] = sum_m s1_m^2,  within[k][d] = sum_m sum_{t >= k} z_t z_(t-k)
      W             within[0] / (M (L - 1)): the mean within-chain variance
      var_of_means  (sumsq_of_sums / L^2 - (sum / L)^2 / M) / (M - 1): the variance of the segment means (B / L)
      var_plus      (L - 1) / L W + var_of_means
      rhat()        sqrt(var_plus / W) (Gelman-Rubin; the split form when the segments are halves); NaN where W is 0 or
                    M < 2
      rho()         [lag][dim], 1 - (W - within[k] / (M L)) / var_plus for the lags below min(64, L)
      tau()         Geyer's initial monotone sequence (BDA3 section 11.5, Vehtari et al. 2021): the pairs
                    P_j = rho[2j] + rho[2j + 1] up to the first negative one, P_j = min(P_j, P_(j-1)), -1 + 2 sum P_j
      ess()         M L / tau()
      truncated()   per dimension: the pairs ran out at the last available lag before one turned negative (the
                    autocorrelation outlives the 64 lags, or L): ess() is then an upper bound
      mean()        centre + sum / (M L)
    sumsq_of_sums / L^2 - (sum / L)^2 / M cancels like any E[yy] - E[y]^2: take the sums about a centre near the mean,
    e.g. TraceMoments(...).mean from one earlier pass.  Sums of several ranks add (`+`) when L and the centre agree."""

    def __init__(self, total, sumsq_of_sums, within, L, M, centre=None):
        self.sum, self.sumsq_of_sums, self.within = _f64(total).copy(), _f64(sumsq_of_sums).copy(), _f64(within).copy()
        self.L, self.M = int(L), int(M)
        self.centre = np.zeros(self.sum.size) if centre is None else _f64(centre).copy()
        if (self.sum.ndim != 1 or self.sumsq_of_sums.shape != self.sum.shape or self.centre.shape != self.sum.shape
                or self.within.ndim != 2 or self.within.shape[1] != self.sum.size):
            raise ValueError("sum[dim], sumsq_of_sums[dim], within[lag][dim] and centre[dim] do not fit together")

    def __add__(self, other):
        if self.L != other.L:
            raise ValueError("segments of different lengths do not pool")
        if not np.array_equal(self.centre, other.centre):
            raise ValueError("sums about different centres do not add")
        return Convergence(self.sum + other.sum, self.sumsq_of_sums + other.sumsq_of_sums, self.within + other.within,
                           self.L, self.M + other.M, self.centre)

    @property
    def W(self):
        return self.within[0] / (float(self.M) * (self.L - 1))

    @property
    def var_of_means(self):
        if self.M < 2:
            return np.full(self.sum.size, np.nan)
        L, M = float(self.L), float(self.M)
        return (self.sumsq_of_sums / (L * L) - (self.sum / L) ** 2 / M) / (M - 1.0)

    @property
    def var_plus(self):
        return (self.L - 1.0) / self.L * self.W + self.var_of_means

    def rhat(self):
        W = self.W
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(W == 0.0, np.nan, np.sqrt(self.var_plus / W))

    def rho(self):
        """[lag][dim]"""
        nlag = min(self.within.shape[0], self.L)
        with np.errstate(divide="ignore", invalid="ignore"):
            return 1.0 - (self.W[None, :] - self.within[:nlag] / (float(self.M) * self.L)) / self.var_plus[None, :]

    def _geyer(self):
        """(tau[dim], truncated[dim])"""
        rho = self.rho()
        npairs, dim = rho.shape[0] // 2, rho.shape[1]
        tau, truncated = np.empty(dim), np.zeros(dim, dtype=bool)
        for d in range(dim):
            total, last, j = 0.0, np.inf, 0
            while j < npairs:
                pair = rho[2 * j, d] + rho[2 * j + 1, d]
                if pair < 0.0:
                    break
                last = min(pair, last) if pair == pair else pair           # a NaN pair makes tau NaN
                total += last
                j += 1
            tau[d], truncated[d] = -1.0 + 2.0 * total, j == npairs
        return tau, truncated

    def tau(self):
        return self._geyer()[0]

    def truncated(self):
        return self._geyer()[1]

    def ess(self):
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(self.M) * self.L / self.tau()

    def mean(self):
        return self.centre + self.sum / (float(self.M) * self.L)


def _convergence(lib, check, trace_ptr, nslots, dim, dim_stride, nchains, nchains_padded, nsegments, centre, stream):
    """The body of the engines' Convergence methods."""
    c = None if centre is None else _f64(centre)
    if c is not None and c.shape != (dim,):
        raise ValueError("centre must be [dim]")
    nslots, nsegments = int(nslots), int(nsegments)
    total, sumsq, within = np.zeros(dim), np.zeros(dim), np.zeros((_capi.AUTOCORR_LAGS, dim))
    check(lib.smcmc_trace_convergence(C.c_void_p(int(trace_ptr)), nslots, dim, dim_stride, nchains, nchains_padded,
                                      nsegments, None if c is None else _ptr(c), None, _ptr(total), _ptr(sumsq),
                                      _ptr(within), C.c_void_p(int(stream))))
    return Convergence(total, sumsq, within, nslots // nsegments, nsegments * nchains, c)


def cholesky_chain(mean, covariance, nslots, nchains, seed=20240607, chain_offset=0, dim_stride=None, stream=0):
    """The Gaussian stand-in chain of CholeskyChain.C:18-66, filled on the device: covariance = U^T U, every
    (slot, chain) one draw mean + sum_i r_i U(i, :) on the random stream (seed, chain_offset + chain, slot).  Returns
    (trace, U): a torch tensor [nslots][dim_stride][nchains_padded] on the current device (rows >= dim and lanes >=
    nchains are NaN), which the reducers take as it is through trace.data_ptr(), and the decomposition [dim][dim].
    A covariance that is not positive definite raises SmcmcError (SMCMC_ERR_RUNTIME)."""
    import torch
    lib = _capi.load()
    mean, covariance = _f64(mean), _f64(covariance)
    dim = mean.size
    if mean.ndim != 1 or covariance.shape != (dim, dim):
        raise ValueError("mean must be [dim] and covariance [dim][dim]")
    dim_stride = dim if dim_stride is None else int(dim_stride)
    nchains, nslots = int(nchains), int(nslots)
    npad = (nchains + 63) // 64 * 64
    if not torch.cuda.is_available():   # the fill is a device kernel: there is no host version of it
        raise SmcmcError(_capi.ERR_NO_DEVICE, lib.smcmc_status_string(_capi.ERR_NO_DEVICE).decode())
    trace = torch.full((nslots, dim_stride, npad), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    U = np.zeros((dim, dim))
    st = lib.smcmc_cholesky_chain(_ptr(mean), _ptr(covariance), dim, nslots, nchains, npad, dim_stride, int(seed),
                                  int(chain_offset), C.c_void_p(trace.data_ptr()), _ptr(U), C.c_void_p(int(stream)))
    if st != _capi.OK:
        raise SmcmcError(st, lib.smcmc_status_string(st).decode())
    return trace, U


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


class HmcEngine:
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

    def AutocorrelationSums(self, trace_ptr, nslots, centre=None, stream=0):
        """As Engine.AutocorrelationSums, over a trace of copy_positions slots ([slot][dim][nchains_padded])."""
        c = _f64(np.zeros(self.dim) if centre is None else centre)
        s = np.zeros(self.dim)
        lagged = np.zeros((_capi.AUTOCORR_LAGS, self.dim))
        self._check(self._lib.smcmc_autocorrelation_sums(C.c_void_p(int(trace_ptr)), int(nslots), self.dim, self.dim,
                                                         self.nchains, self.nchains_padded, _ptr(c), _ptr(s), _ptr(lagged),
                                                         C.c_void_p(int(stream))))
        return Autocorrelation(s, lagged, int(nslots), self.nchains)

    def AutocorrelationGrid(self, trace_ptr, nslots, lag_first=1, lag_step=1, nlags=64, centre=None, stream=0):
        """As Engine.AutocorrelationGrid, over a trace of copy_positions slots ([slot][dim][nchains_padded])."""
        return _autocorrelation_grid(self._lib, self._check, trace_ptr, nslots, self.dim, self.dim, self.nchains,
                                     self.nchains_padded, lag_first, lag_step, nlags, centre, stream)

    def MakeAutocorrelation(self, trace_ptr, nslots, stream=0, centre=None, plan=None):
        """As Engine.MakeAutocorrelation, over a trace of copy_positions slots ([slot][dim][nchains_padded])."""
        return _make_autocorrelation(self._lib, self._check, trace_ptr, nslots, self.dim, self.dim, self.nchains,
                                     self.nchains_padded, centre, stream, plan)

    def Marginals(self, trace_ptr, nslots, n1=100, n2=50, pair_dims=None, sample_stride=None, ranges=None, stream=0):
        """As Engine.Marginals, over a trace of copy_positions slots ([slot][dim][nchains_padded])."""
        return _marginals(self._lib, self._check, trace_ptr, nslots, self.dim, self.dim, self.nchains, self.nchains_padded,
                          n1, n2, pair_dims, sample_stride, ranges, stream)

    def TraceMoments(self, trace_ptr, nslots, centre=None, stream=0):
        """As Engine.TraceMoments, over a trace of copy_positions slots ([slot][dim][nchains_padded])."""
        return _trace_moments(self._lib, self._check, trace_ptr, nslots, self.dim, self.dim, self.nchains,
                              self.nchains_padded, centre, stream)

    def Convergence(self, trace_ptr, nslots, nsegments=2, centre=None, stream=0):
        """As Engine.Convergence, over a trace of copy_positions slots ([slot][dim][nchains_padded])."""
        return _convergence(self._lib, self._check, trace_ptr, nslots, self.dim, self.dim, self.nchains,
                            self.nchains_padded, nsegments, centre, stream)

    def lane(self, name):
        if name in _capi.HMC_LANE_F64:
            out = np.zeros(self.nchains)
            self._check(self._lib.smcmc_hmc_read_lane_f64(self._h, _capi.HMC_LANE_F64[name], _ptr(out)))
            return out
        out = np.zeros(self.nchains, np.int32)
        self._check(self._lib.smcmc_hmc_read_lane_i32(self._h, _capi.HMC_LANE_I32[name],
                                                      out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out


class VaatEngine:
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

    def AutocorrelationGrid(self, trace_ptr, nslots, lag_first=1, lag_step=1, nlags=64, centre=None, stream=0):
        """As Engine.AutocorrelationGrid, over a trace step_save wrote ([slot][dim][nchains_padded])."""
        return _autocorrelation_grid(self._lib, self._check, trace_ptr, nslots, self.dim, self.dim, self.nchains,
                                     self.nchains_padded, lag_first, lag_step, nlags, centre, stream)

    def MakeAutocorrelation(self, trace_ptr, nslots, stream=0, centre=None, plan=None):
        """As Engine.MakeAutocorrelation, over a trace step_save wrote ([slot][dim][nchains_padded])."""
        return _make_autocorrelation(self._lib, self._check, trace_ptr, nslots, self.dim, self.dim, self.nchains,
                                     self.nchains_padded, centre, stream, plan)

    def Marginals(self, trace_ptr, nslots, n1=100, n2=50, pair_dims=None, sample_stride=None, ranges=None, stream=0):
        """As Engine.Marginals, over a trace step_save wrote ([slot][dim][nchains_padded])."""
        return _marginals(self._lib, self._check, trace_ptr, nslots, self.dim, self.dim, self.nchains, self.nchains_padded,
                          n1, n2, pair_dims, sample_stride, ranges, stream)

    def TraceMoments(self, trace_ptr, nslots, centre=None, stream=0):
        """As Engine.TraceMoments, over a trace step_save wrote ([slot][dim][nchains_padded])."""
        return _trace_moments(self._lib, self._check, trace_ptr, nslots, self.dim, self.dim, self.nchains,
                              self.nchains_padded, centre, stream)

    def Convergence(self, trace_ptr, nslots, nsegments=2, centre=None, stream=0):
        """As Engine.Convergence, over a trace step_save wrote ([slot][dim][nchains_padded])."""
        return _convergence(self._lib, self._check, trace_ptr, nslots, self.dim, self.dim, self.nchains,
                            self.nchains_padded, nsegments, centre, stream)

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
