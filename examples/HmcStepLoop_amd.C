// The unchanged caller's loop of SimpleHMC.C: one chain of sMCMC::TSimpleHMC<TIsoGaussLogLikelihood> with per-chain
// adaptation (the reference chain), `for (...) hmc.Step(save)` one call at a time, the getters a caller prints read
// every `verbosity` calls.  argv: dim steps save(0|1) runahead(0|1) [out.csv]
// Prints "steps_per_s <rate>" for the timed loop.  SetRunAhead is called only where the header has it, so the same
// file measures a header from before the run-ahead.
#include <chrono>
#include <cstdlib>
#include <iostream>
#include "TSimpleHMC_amd.H"

int main(int argc, char** argv) {
    if (argc < 5) return 64;
    const int dim = std::atoi(argv[1]), steps = std::atoi(argv[2]);
    const bool save = std::atoi(argv[3]) != 0;
    const bool ahead = std::atoi(argv[4]) != 0;
    try {
        sMCMC::TreeType tree("SimpleHMC", "");
        sMCMC::TSimpleHMC<sMCMC::TIsoGaussLogLikelihood> hmc(&tree);
        hmc.SetPerChainAdaptation(true);
        bool runAhead = false;
#ifdef SMCMC_HMC_RUN_AHEAD
        hmc.SetRunAhead(ahead);
#else
        (void)ahead;
#endif
        sMCMC::Vector p((std::size_t)dim, 1.0);
        hmc.Start(p, save);
#ifdef SMCMC_HMC_RUN_AHEAD
        runAhead = hmc.GetRunAhead();
#endif
        const int verbosity = steps / 5 > 0 ? steps / 5 : 1;
        double printed = 0.0;
        int moved = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < steps; ++i) {
            if ((i + 1) % verbosity == 0)
                printed += hmc.GetAcceptanceRate() + hmc.GetMeanEpsilon() + hmc.GetLeapFrog() + hmc.GetCovarianceTrace() +
                           hmc.GetEstimatedOrbitLength();
            moved += hmc.Step(save) ? 1 : 0;
        }
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::cout << "steps_per_s " << (double)steps / dt << " moved " << moved << " entries " << tree.GetEntries()
                  << " run_ahead " << (runAhead ? 1 : 0) << " potentials " << hmc.GetPotentialCount() << " gradients "
                  << hmc.GetGradientCount() << " printed " << printed << std::endl;
        if (argc > 5) tree.WriteCsv(argv[5]);
    } catch (const std::exception& e) {
        std::cerr << "hmc_step_loop: " << e.what() << std::endl;
        return 2;
    }
    return 0;
}
