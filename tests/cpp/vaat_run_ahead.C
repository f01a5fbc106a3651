// Test driver: sMCMC::TSimpleMCMC<L, sMCMC::TProposeVAATStep>, 70 chains, 40 x Step(true) with the getters of
// SimpleVAAT.C's progress line printed after every step, SetAcceptanceRigidity(0.7) after step 11, UpdateProposal()
// after Start (an empty queue), after step 17 (a queue that is not empty: nothing happens) and after step 21 (empty
// again at dim 7), GetAcceptedAll() after step 29; the tree written as CSV.
// argv: dim likelihood(0 iso-Gaussian | 1 header-form TDummyLogLikelihood) runahead(0 off | 1 on | 2 on, off after step 23) out.csv
// tests/test_cpp_vaat_run_ahead.py runs it in the three modes: the same tree and the same output byte for byte, and
// chain 0's columns are the reference chain's.
#include <cstdlib>
#include <iostream>
#include "TSimpleMCMC_amd.H"
#include "TProposeVAATStep_amd.H"

#if !defined(SMCMC_VAAT_RUN_AHEAD)
#error "TProposeVAATStep_amd.H has no SetRunAhead"
#endif

template <typename L>
int Run(L& like, sMCMC::TSimpleMCMC<L, sMCMC::TProposeVAATStep>& mcmc, sMCMC::TreeType& tree, int dim, int mode,
        const char* out) {
    (void)like;
    mcmc.SetChains(70);
    mcmc.SetRunAhead(mode != 0);
    mcmc.GetProposeStep().SetDim(dim);
    sMCMC::Vector p((std::size_t)dim);
    for (int i = 0; i < dim; ++i) p[i] = 0.125 * (i % 5) - 0.25;
    if (!mcmc.Start(p, true)) return 1;
    if (mcmc.GetRunAhead() != (mode != 0)) { std::cerr << "GetRunAhead after Start\n"; return 3; }
    mcmc.GetProposeStep().SetAcceptanceWindow(20);       // widths move within a few visits per dimension
    mcmc.GetProposeStep().UpdateProposal();              // SimpleVAAT.C:44
    std::cout.precision(17);
    int moved = 0;
    for (int s = 1; s <= 40; ++s) {
        moved += mcmc.Step(true) ? 1 : 0;
        std::cout << "step " << s << " sigma " << mcmc.GetProposeStep().GetSigma() << " acceptance "
                  << mcmc.GetProposeStep().GetAcceptance() << " successes " << mcmc.GetProposeStep().GetSuccesses() << "/"
                  << mcmc.GetProposeStep().GetTrials() << " proposed " << mcmc.GetProposedLogLikelihood() << std::endl;
        if (s == 11) mcmc.GetProposeStep().SetAcceptanceRigidity(0.7);
        if (s == 17 || s == 21) mcmc.GetProposeStep().UpdateProposal();
        if (s == 23 && mode == 2) mcmc.SetRunAhead(false);
        if (s == 29) {
            sMCMC::Vector logl;
            const sMCMC::Vector all = mcmc.GetAcceptedAll(&logl);
            double sum = 0.0;
            for (double v : all) sum += v;
            std::cout << "all chains: sum " << sum << " logl[69] " << logl[69] << " chain 0 "
                      << (all[0] == mcmc.GetAccepted()[0] ? "agrees" : "DIFFERS") << std::endl;
        }
    }
    if (mcmc.GetRunAhead() != (mode == 1)) { std::cerr << "GetRunAhead at the end\n"; return 3; }
    const sMCMC::Vector sigmas = mcmc.GetProposeStep().GetSigmas(), accs = mcmc.GetProposeStep().GetAcceptances();
    double ws = 0.0;
    for (int d = 0; d < dim; ++d) ws += (d + 1) * sigmas[d] + accs[d] / (d + 1);
    std::cout << "entries " << tree.GetEntries() << " moved " << moved << " likelihoods " << mcmc.GetLogLikelihoodCount()
              << " weighted " << ws << " accepted " << mcmc.GetAcceptedLogLikelihood() << std::endl;
    tree.WriteCsv(out);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 5) return 64;
    const int dim = std::atoi(argv[1]), kind = std::atoi(argv[2]), mode = std::atoi(argv[3]);
    try {
        sMCMC::TreeType tree("SimpleVAAT", "");
        if (kind == 1) {
            sMCMC::TSimpleMCMC<sMCMC::TDummyLogLikelihood, sMCMC::TProposeVAATStep> mcmc(&tree, true);
            mcmc.GetLogLikelihood().SetDim(dim);
            mcmc.GetLogLikelihood().Init();
            return Run(mcmc.GetLogLikelihood(), mcmc, tree, dim, mode, argv[4]);
        }
        sMCMC::TSimpleMCMC<sMCMC::TIsoGaussLogLikelihood, sMCMC::TProposeVAATStep> mcmc(&tree, true);
        return Run(mcmc.GetLogLikelihood(), mcmc, tree, dim, mode, argv[4]);
    } catch (const std::exception& e) {
        std::cerr << "vaat_run_ahead: " << e.what() << std::endl;
        return 2;
    }
}
