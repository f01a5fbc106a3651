// FakeMCMC2_amd.C -- the reference's example2/FakeMCMC.C on the MI355X engine: one chain of
// sMCMC::TSimpleMCMC<sMCMC::FakeTemplateLikelihood> (include/FakeTemplateLikelihood_amd.H, SMCMC_LIKE_EVENT_TEMPLATE)
// adapting as the reference does, with the macro's schedule -- Gaussian proposals of sqrt(1 + count) for the two fitted
// counts, a start at the true values with the two counts jittered, two unsaved burn-ins each opened by ResetProposal()
// (the second twice the length of the first, :106-114), then four saved legs each opened by UpdateProposal() -- and its
// WriteSimulation() calls.  Without the drawing: the histograms the macro stacks and prints are kept by name in
// like.Written.  The macro's lengths (10 000 steps of burn-in, legs of 50 000) are the defaults; every size comes from
// the command line so that a test can run it small.
//
//   g++ -std=c++17 -O2 -Iinclude examples/FakeMCMC2_amd.C -Lroot-simple-mcmc_amd/lib -lsmcmc_amd
//       -Wl,-rpath,$PWD/root-simple-mcmc_amd/lib -Wl,-rpath,/opt/rocm/lib -o fake_mcmc2_amd.exe
//   ./fake_mcmc2_amd.exe [dataSignal [dataBackground [mcOversample [burninLength [chainLength [output.csv [params.txt]]]]]]]
// params.txt receives the likelihood's parameter array (smcmc_set_likelihood_params' layout), so that a saved point can
// be checked against smcmc_event_template_evaluate.
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "FakeTemplateLikelihood_amd.H"

const int gBurninCycles = 2;                                                             // FakeMCMC.C:13-17
const int gChainCycles = 4;

int FakeMCMC2(int dataSignal, int dataBackground, double mcOversample, int burninLength, int chainLength,
              const char* outputName, const char* paramsName) {
    std::cout << "Fake Likelihood MCMC Loaded (template fit, MI355X engine)" << std::endl;
    sMCMC::TreeType tree("MCMC", "Tree of accepted points");                             // :28
    sMCMC::TSimpleMCMC<sMCMC::FakeTemplateLikelihood> mcmc(&tree);                       // :30
    sMCMC::FakeTemplateLikelihood& like = mcmc.GetLogLikelihood();
    sMCMC::TProposeAdaptiveStep& proposal = mcmc.GetProposeStep();

    like.Init(dataSignal, dataBackground, mcOversample);                                 // :36
    std::cout << like.SimulatedSample.size() << " simulated events, signal integral " << like.SignalIntegral
              << ", background integral " << like.BackgroundIntegral << std::endl;
    if (paramsName) like.WriteParams(paramsName);
    proposal.SetDim((int)like.GetDim());                                                 // :65
    proposal.SetGaussian(0, std::sqrt(1.0 + like.MCTrueValues[0]));                      // :67
    proposal.SetGaussian(1, std::sqrt(1.0 + like.MCTrueValues[1]));                      // :68

    sMCMC::Vector p(like.MCTrueValues);                                                  // :74-79
    sMCMC::detail::RestoreUniform uniform(20240607);                                     // :80-81, on the host stream
    for (int k = 0; k < 2; ++k) {
        const double r = std::sqrt(-2.0 * std::log(uniform()));
        p[k] += std::sqrt(p[k]) * r * std::cos(6.283185307179586476925 * uniform());
    }
    if (!mcmc.Start(p, false)) {                                                         // :82
        std::cout << "bad starting point" << std::endl;
        return 1;
    }
    like.WriteSimulation(p, "initial");                                                  // :84

    for (int burnin = 0; burnin < gBurninCycles; ++burnin) {                             // :106-116
        proposal.ResetProposal();
        std::ostringstream name;
        name << "burnin" << burnin + 1;
        const int length = burninLength * (burnin + 1) / gBurninCycles;
        std::cout << "Start new burnin phase (" << length << " steps)" << std::endl;
        for (int i = 0; i < length; ++i) mcmc.Step(false);
        like.WriteSimulation(proposal.GetEstimatedCenter(), name.str());
    }

    const auto t0 = std::chrono::steady_clock::now();
    for (int chain = 0; chain < gChainCycles; ++chain) {                                 // :140-146
        proposal.UpdateProposal();
        std::cout << "Start chain " << chain << std::endl;
        for (int i = 0; i < chainLength; ++i) mcmc.Step();
        like.WriteSimulation(proposal.GetEstimatedCenter(), "midway");
    }
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::cout << "steps_per_s " << (double)gChainCycles * chainLength / dt
              << " (the saved legs, their UpdateProposal and WriteSimulation calls included)" << std::endl;

    std::cout << "Finished with " << mcmc.GetLogLikelihoodCount() << " calls, log L " << mcmc.GetAcceptedLogLikelihood()
              << ", " << like.Written.size() << " histograms kept" << std::endl;
    tree.Write();                                                                        // :170
#ifndef SMCMC_HAVE_ROOT
    tree.WriteCsv(outputName);
    std::cout << "wrote " << tree.GetEntries() << " entries to " << outputName << std::endl;
#endif
    return 0;
}

int main(int argc, char** argv) {
    int dataSignal = 1000, dataBackground = 1000;                                        // FakeMCMC.C:36
    double mcOversample = 10.0;
    int burninLength = 10000, chainLength = 50000;                                       // :14, 17
    std::string outputName("FakeMCMC2_amd.csv");
    if (argc > 1) { std::istringstream in(argv[1]); in >> dataSignal; }
    if (argc > 2) { std::istringstream in(argv[2]); in >> dataBackground; }
    if (argc > 3) { std::istringstream in(argv[3]); in >> mcOversample; }
    if (argc > 4) { std::istringstream in(argv[4]); in >> burninLength; }
    if (argc > 5) { std::istringstream in(argv[5]); in >> chainLength; }
    if (argc > 6) outputName = argv[6];
    const char* paramsName = (argc > 7) ? argv[7] : NULL;
    try {
        return FakeMCMC2(dataSignal, dataBackground, mcOversample, burninLength, chainLength, outputName.c_str(), paramsName);
    } catch (const std::exception& e) {
        std::cerr << "FakeMCMC2_amd: " << e.what() << std::endl;
        return 2;
    }
}
