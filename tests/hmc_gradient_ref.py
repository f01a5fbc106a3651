"""One fixed-step sMCMC::TSimpleHMC::Step() (reference TSimpleHMC.H:279-401, ProposeMomentum :554-570, LeapFrog :582-651)
of one chain, restated in Python with the gradient and the potential passed in as callables.

It exists so that a chain whose gradient is NOT the gradient of its likelihood (BadGrad.C: TSimpleHMC<L, G> with G's
matrix different from L's) has a yardstick: oracle.Hmc only knows the built-in likelihoods' own gradients.  Everything
random or transcendental comes from what oracle/oracle.py exports (draw_block, det_normal_pair, det_u01, det_log); the
rest is IEEE double arithmetic in the reference's operation order, one Python float operation per C operation.
tests/test_hmc_user_gradient_cpu.py pins it against oracle.Hmc, bit for bit, where the two overlap."""
import math

import numpy as np

STREAM_HMC = 2          # SMCMC_STREAM_HMC, include/smcmc_detmath.h


def accept_word(dim):
    """smcmc_accept_word: the first random word behind the momentum normals (two words per pair of dimensions)."""
    return 2 * ((dim + 1) // 2)


class HmcGradientRef:
    """gradient(q) -> grad log L at q (what the reference functor writes to g, TSimpleHMC.H:87; the step negates it, :486);
    potential(q) -> -log L at q (:411-414).  abs_epsilon and leapfrog are fixed (SetMeanEpsilon(-e), SetLeapFrog(n))."""

    def __init__(self, oracle, dim, gradient, potential, abs_epsilon, leapfrog, alpha=0.0, seed=20240607, chain_id=0):
        assert 0.0 <= alpha and leapfrog >= 1 and abs_epsilon > 0.0
        self._o = oracle
        self.dim, self.gradient, self.potential = int(dim), gradient, potential
        self.abs_epsilon, self.leapfrog, self.alpha = float(abs_epsilon), int(leapfrog), float(alpha)
        self.seed, self.chain_id = int(seed), int(chain_id)
        self.step_count = 0
        self.naccept = 0

    def start(self, x0):                                                  # Start :210-269
        self.step_count = 0
        self.naccept = 0
        self.accepted = [float(v) for v in x0]
        self.momentum = [0.0] * self.dim
        self.accepted_potential = float(self.potential(np.array(self.accepted)))
        self.proposed_potential = self.accepted_potential
        self.acceptance = 0.65                                            # :234-235
        self.last_accept = False

    def _word(self, w):
        return self._o.draw_block(self.seed, self.chain_id, self.step_count, w >> 2, STREAM_HMC)[w & 3]

    def _potential_gradient(self, q):                                     # PotentialGradient type 0 / 1 / 4, :478-491
        g = self.gradient(np.array(q))
        return [-float(v) for v in g]

    def step(self):
        o, n = self._o, self.dim
        self.step_count += 1                                              # :286
        # ProposeMomentum :554-570
        pn = [0.0] * n
        if self.alpha >= 1.0:
            for i in range(n):
                pn[i] = self.momentum[i] / self.alpha
        else:
            mix = math.sqrt(1.0 - self.alpha * self.alpha)
            for i in range(n):
                pr = i >> 1
                n0, n1 = o.det_normal_pair([self._word(2 * pr)], [self._word(2 * pr + 1)])
                r = float(n1[0]) if (i & 1) else float(n0[0])
                pn[i] = self.alpha * self.momentum[i] + mix * r
        ke0 = 0.0                                                         # KineticEnergy :535-542
        for i in range(n):
            ke0 += pn[i] * pn[i] / 2.0
        ew = accept_word(n)
        lo, hi = 0.9 * self.abs_epsilon, 1.1 * self.abs_epsilon
        eps = lo + (hi - lo) * float(o.det_u01([self._word(ew)])[0])      # :297-298
        # LeapFrog :582-651 (steps >= 1)
        qn = list(self.accepted)
        grad = self._potential_gradient(qn)                               # :615
        for j in range(n):
            pn[j] = pn[j] - eps * grad[j] / 2.0                           # :618-620
        for _ in range(self.leapfrog - 1):                                # :623-639 (a fixed count ignores the reversal)
            for j in range(n):
                qn[j] = qn[j] + eps * pn[j]
            grad = self._potential_gradient(qn)
            for j in range(n):
                pn[j] = pn[j] - eps * grad[j]
        for j in range(n):
            qn[j] = qn[j] + eps * pn[j]                                   # :641-643
        grad = self._potential_gradient(qn)
        for j in range(n):
            pn[j] = pn[j] - eps * grad[j] / 2.0                           # :645-648
        ke1 = 0.0
        for i in range(n):
            ke1 += pn[i] * pn[i] / 2.0                                    # :326
        self.proposed_potential = float(self.potential(np.array(qn)))     # :327
        h_prop = self.proposed_potential + ke1                            # :333
        h_acc = self.accepted_potential + ke0                             # :334
        delta = h_prop - h_acc                                            # :346
        trial = -float(o.det_log([float(o.det_u01([self._word(ew + 1)])[0])])[0])   # :347
        if delta > trial or not math.isfinite(delta):                     # :348-368
            self.momentum = [-v for v in self.momentum]
            self.acceptance = (self.acceptance * 4999.0) / 5000.0
            self.last_accept = False
        else:                                                             # :369-387
            self.accepted = qn
            self.momentum = pn
            self.accepted_potential = self.proposed_potential
            self.acceptance = (self.acceptance * 4999.0 + 1.0) / 5000.0
            self.last_accept = True
            self.naccept += 1
        return self.last_accept

    def run(self, nsteps):
        for _ in range(nsteps):
            self.step()
