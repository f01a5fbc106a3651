// FakeMCMC_amd.C -- the reference's example/FakeMCMC.C on the MI355X engine: one chain of
// sMCMC::TSimpleMCMC<sMCMC::FakeLikelihood> (include/FakeLikelihood_amd.H, SMCMC_LIKE_EVENT_SAMPLE) adapting as the
// reference does, with the macro's schedule -- a first burn-in of 100 unsaved steps and ResetProposal(), a second of 100
// and UpdateProposal(), then two legs of 500 saved steps -- and its WriteSimulation() calls.  Without the drawing: the
// histograms the macro stacks and prints are kept by name in like.Written.
//
//   g++ -std=c++17 -O2 -Iinclude examples/FakeMCMC_amd.C -Lroot-simple-mcmc_amd/lib -lsmcmc_amd
//       -Wl,-rpath,$PWD/root-simple-mcmc_amd/lib -Wl,-rpath,/opt/rocm/lib -o fake_mcmc_amd.exe
//   ./fake_mcmc_amd.exe [dataSignal [dataBackground [mcOversample [output.csv [params.txt]]]]]
// params.txt receives the likelihood's parameter array (smcmc_set_likelihood_params' layout), so that a saved point can
// be checked against smcmc_event_sample_evaluate.
#include <chrono>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "FakeLikelihood_amd.H"

const int gFirstBurnin = 100;                                                            // FakeMCMC.C:13-15
const int gSecondBurnin = 100;
const int gChainLength = 500;

int FakeMCMC(int dataSignal, int dataBackground, double mcOversample, const char* outputName, const char* paramsName) {
    std::cout << "Fake Likelihood MCMC Loaded (MI355X engine)" << std::endl;
    sMCMC::TreeType tree("MCMC", "Tree of accepted points");                             // :26
    sMCMC::TSimpleMCMC<sMCMC::FakeLikelihood> mcmc(&tree);                               // :28
    sMCMC::FakeLikelihood& like = mcmc.GetLogLikelihood();
    sMCMC::TProposeAdaptiveStep& proposal = mcmc.GetProposeStep();

    like.Init(dataSignal, dataBackground, mcOversample);                                 // :34
    std::cout << "Exposure Ratio " << like.ExposureRatio << " (" << like.SimulatedSample.size() << " simulated events)"
              << std::endl;
    if (paramsName) like.WriteParams(paramsName);
    proposal.SetDim((int)like.GetDim());                                                 // :57

    sMCMC::Vector p(like.GetDim());                                                      // :66-67, on the host stream
    sMCMC::detail::RestoreUniform uniform(20240607);
    for (std::size_t i = 0; i < p.size(); ++i) p[i] = -1.0 + 2.0 * uniform();

    if (!mcmc.Start(p, false)) {                                                         // :69
        std::cout << "bad starting point" << std::endl;
        return 1;
    }
    like.WriteSimulation(p, "initial");                                                  // :71

    for (int i = 0; i < gFirstBurnin; ++i) mcmc.Step(false);                             // :93
    proposal.ResetProposal();
    like.WriteSimulation(proposal.GetEstimatedCenter(), "burnin");

    for (int i = 0; i < gSecondBurnin; ++i) mcmc.Step(false);                            // :118
    proposal.UpdateProposal();
    like.WriteSimulation(proposal.GetEstimatedCenter(), "Start");

    std::cout << "Start the chain" << std::endl;                                         // :142
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < gChainLength; ++i) mcmc.Step();
    like.WriteSimulation(proposal.GetEstimatedCenter(), "midway");
    for (int i = 0; i < gChainLength; ++i) mcmc.Step();                                  // :165
    like.WriteSimulation(proposal.GetEstimatedCenter(), "final");
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::cout << "steps_per_s " << 2.0 * gChainLength / dt << " (the two saved legs, their WriteSimulation calls included)" << std::endl;

    std::cout << "Finished with " << mcmc.GetLogLikelihoodCount() << " calls, log L " << mcmc.GetAcceptedLogLikelihood()
              << ", " << like.Written.size() << " histograms kept" << std::endl;
    tree.Write();                                                                        // :187
#ifndef SMCMC_HAVE_ROOT
    tree.WriteCsv(outputName);
    std::cout << "wrote " << tree.GetEntries() << " entries to " << outputName << std::endl;
#endif
    return 0;
}

int main(int argc, char** argv) {
    int dataSignal = 1000, dataBackground = 1000;                                        // FakeLikelihood.H:86-87
    double mcOversample = 10.0;
    std::string outputName("FakeMCMC_amd.csv");
    if (argc > 1) { std::istringstream in(argv[1]); in >> dataSignal; }
    if (argc > 2) { std::istringstream in(argv[2]); in >> dataBackground; }
    if (argc > 3) { std::istringstream in(argv[3]); in >> mcOversample; }
    if (argc > 4) outputName = argv[4];
    const char* paramsName = (argc > 5) ? argv[5] : NULL;
    try {
        return FakeMCMC(dataSignal, dataBackground, mcOversample, outputName.c_str(), paramsName);
    } catch (const std::exception& e) {
        std::cerr << "FakeMCMC_amd: " << e.what() << std::endl;
        return 2;
    }
}
