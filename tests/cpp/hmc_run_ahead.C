// Test driver: sMCMC::TSimpleHMC<TIsoGaussLogLikelihood>, 64 chains, SetPerChainAdaptation(true), 34 x Step(true) with
// SetAlpha(0.1) after step 11 and GetEstimatedCovariance() after step 23, the tree written as CSV and the potential /
// gradient counts printed.  argv: dim runahead(0|1) out.csv.  tests/test_cpp_hmc_run_ahead.py runs it with the run-ahead
// off and on: the same tree byte for byte, and chain 0's columns are the reference chain's.
#include <cstdlib>
#include <iostream>
#include "TSimpleHMC_amd.H"

int main(int argc, char** argv) {
    if (argc < 4) return 64;
    const int dim = std::atoi(argv[1]);
    const bool ahead = std::atoi(argv[2]) != 0;
    try {
        sMCMC::TreeType tree("SimpleHMC", "");
        sMCMC::TSimpleHMC<sMCMC::TIsoGaussLogLikelihood> hmc(&tree);
        hmc.SetChains(64);
        hmc.SetPerChainAdaptation(true);
        hmc.SetRunAhead(ahead);
        sMCMC::Vector p((std::size_t)dim, 1.0);
        hmc.Start(p, true);
        if (hmc.GetRunAhead() != ahead) { std::cerr << "GetRunAhead\n"; return 3; }
        double covTrace = 0.0;
        for (int s = 1; s <= 34; ++s) {
            hmc.Step(true);
            if (s == 11) hmc.SetAlpha(0.1);
            if (s == 23) {
                const sMCMC::Vector cov = hmc.GetEstimatedCovariance();
                for (int d = 0; d < dim; ++d) covTrace += cov[(std::size_t)d * dim + d];
            }
        }
        std::cout.precision(17);
        std::cout << "entries " << tree.GetEntries() << " potentials " << hmc.GetPotentialCount() << " gradients "
                  << hmc.GetGradientCount() << " cov_trace " << covTrace << " central " << hmc.GetCentralPotential()
                  << " accepted " << hmc.GetAcceptedPotential() << std::endl;
        tree.WriteCsv(argv[3]);
    } catch (const std::exception& e) {
        std::cerr << "hmc_run_ahead: " << e.what() << std::endl;
        return 2;
    }
    return 0;
}
