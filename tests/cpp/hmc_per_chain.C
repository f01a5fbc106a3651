// Test driver: sMCMC::TSimpleHMC<TIsoGaussLogLikelihood> with 64 chains and SetPerChainAdaptation(true), the reference's
// call sequence (Start, then Step(true) nsteps times, nothing fixed), the tree written as CSV.  argv: dim nsteps out.csv.
// tests/test_cpp_hmc_per_chain.py checks chain 0's columns against the CPU restatement of one TSimpleHMC chain.
#include <cstdlib>
#include <iostream>
#include "TSimpleHMC_amd.H"

int main(int argc, char** argv) {
    if (argc < 4) return 64;
    const int dim = std::atoi(argv[1]), nsteps = std::atoi(argv[2]);
    try {
        sMCMC::TreeType tree("SimpleHMC", "");
        sMCMC::TSimpleHMC<sMCMC::TIsoGaussLogLikelihood> hmc(&tree);
        hmc.SetChains(64);
        hmc.SetPerChainAdaptation(true);
        if (!hmc.GetPerChainAdaptation()) return 3;
        sMCMC::Vector p((std::size_t)dim, 1.0);
        hmc.Start(p, true);
        for (int s = 0; s < nsteps; ++s) hmc.Step(true);
        bool refused = false;
        try {
            hmc.SetPerChainAdaptation(false);
        } catch (const std::logic_error&) {
            refused = true;
        }
        if (!refused) { std::cerr << "SetPerChainAdaptation after Start was accepted\n"; return 3; }
        std::cout << "entries " << tree.GetEntries() << std::endl;
        tree.WriteCsv(argv[3]);
    } catch (const std::exception& e) {
        std::cerr << "hmc_per_chain: " << e.what() << std::endl;
        return 2;
    }
    return 0;
}
