// The unchanged caller's loop around the variable-at-a-time proposal (SimpleVAAT.C:47-61): chains of
// sMCMC::TSimpleMCMC<L, sMCMC::TProposeVAATStep>, Start(p, false), the explicit UpdateProposal(), then
// `for (...) mcmc.Step(save)` one call at a time, the getters of SimpleVAAT.C's progress line (:54-57) read every
// `verbosity` steps.  The counterpart of StepLoop_amd.C for this proposal.
// argv: dim cycles steps save(0|1) runahead(0|1|2: on, and turned off after the first cycle) [out.csv [chains [likelihood 0|1]]]
//   likelihood 0: iso-Gaussian (default), 1: the header-form TDummyLogLikelihood (SimpleVAAT.C's own, with dim 100)
// Prints "steps_per_s <rate>" for the timed loop, and -- for the parity test -- with out.csv the tree, so that the
// run-ahead Step() can be diffed against Step() one launch at a time: they are the same chain.
#include <chrono>
#include <cstdlib>
#include <iostream>
#include "TSimpleMCMC_amd.H"
#include "TProposeVAATStep_amd.H"

template <typename MCMC>
int Loop(MCMC& mcmc, sMCMC::TreeType& tree, int dim, int cycles, int steps, bool save, int ahead, int chains,
         const char* out) {
    if (ahead == 0) mcmc.SetRunAhead(false);             // 1 / 2: the default, on (a small ensemble)
    mcmc.SetChains(chains);
    mcmc.GetProposeStep().SetDim(dim);
    sMCMC::Vector p((std::size_t)dim);
    for (int i = 0; i < dim; ++i) p[i] = 0.125 * (i % 9) - 0.5;
    if (!mcmc.Start(p, false)) return 1;                                  // SimpleVAAT.C:43
    mcmc.GetProposeStep().UpdateProposal();                               // :44
    const int verbosity = steps * cycles / 100 > 0 ? steps * cycles / 100 : 1;   // :47
    double printed = 0.0;
    int moved = 0, trial = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int cycle = 0; cycle < cycles; ++cycle) {
        for (int i = 0; i < steps; ++i) {
            ++trial;
            moved += mcmc.Step(save) ? 1 : 0;                             // :52
            if (trial % verbosity == 0)                                   // what :54-57 prints
                printed += mcmc.GetProposeStep().GetAcceptance() + mcmc.GetProposeStep().GetSuccesses() +
                           mcmc.GetProposeStep().GetTrials() + mcmc.GetProposeStep().GetSigma();
        }
        if (ahead == 2 && cycle == 0) mcmc.SetRunAhead(false);
    }
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::cout.precision(17);
    std::cout << "steps_per_s " << (double)cycles * steps / dt << " moved " << moved << " entries " << tree.GetEntries()
              << " run_ahead " << (mcmc.GetRunAhead() ? 1 : 0) << " printed " << printed << std::endl;
    if (out) tree.WriteCsv(out);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 6) return 64;
    const int dim = std::atoi(argv[1]), cycles = std::atoi(argv[2]), steps = std::atoi(argv[3]);
    const bool save = std::atoi(argv[4]) != 0;
    const int ahead = std::atoi(argv[5]);
    const char* out = argc > 6 && argv[6][0] ? argv[6] : nullptr;   // "": no tree file
    const int chains = argc > 7 ? std::atoi(argv[7]) : 1;
    const int kind = argc > 8 ? std::atoi(argv[8]) : 0;
    try {
        sMCMC::TreeType tree("SimpleVAAT", "");
        if (kind == 1) {
            sMCMC::TSimpleMCMC<sMCMC::TDummyLogLikelihood, sMCMC::TProposeVAATStep> mcmc(&tree, true);
            mcmc.GetLogLikelihood().SetDim(dim);
            mcmc.GetLogLikelihood().Init();                               // :26
            return Loop(mcmc, tree, dim, cycles, steps, save, ahead, chains, out);
        }
        sMCMC::TSimpleMCMC<sMCMC::TIsoGaussLogLikelihood, sMCMC::TProposeVAATStep> mcmc(&tree, true);
        return Loop(mcmc, tree, dim, cycles, steps, save, ahead, chains, out);
    } catch (const std::exception& e) {
        std::cerr << "vaat_step_loop: " << e.what() << std::endl;
        return 2;
    }
}
