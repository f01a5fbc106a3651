// FakeMCMC3_amd.C -- the reference's example3/FakeMCMC.C on the MI355X engine: one chain of
// sMCMC::TSimpleMCMC<sMCMC::FakeShapeLikelihood> (include/FakeShapeLikelihood_amd.H, SMCMC_LIKE_EVENT_SHAPE) adapting as
// the reference does, with the macro's schedule -- Gaussian proposals of sqrt(1 + count) for the two fitted counts, a
// start at the true values with the two counts jittered, five unsaved burn-ins each opened by ResetProposal() (burn-in k
// of k / 5 of the burn-in length, :111-119), then five saved legs each opened by UpdateProposal() -- and its
// WriteSimulation() calls.  Without the drawing: the histograms the macro stacks and prints are kept by name in
// like.Written, the two shapes' control values in like.BackgroundShape and like.SignalShape.  The macro's sizes --
// Init(10000, 100, 10.0), 1 000 steps of burn-in, legs of 10 000 -- are the defaults; every size comes from the command
// line so that a test can run it small.
//
//   g++ -std=c++17 -O2 -Iinclude examples/FakeMCMC3_amd.C -Lroot-simple-mcmc_amd/lib -lsmcmc_amd
//       -Wl,-rpath,$PWD/root-simple-mcmc_amd/lib -Wl,-rpath,/opt/rocm/lib -o fake_mcmc3_amd.exe
//   ./fake_mcmc3_amd.exe [dataSignal [dataBackground [mcOversample [burninLength [chainLength [output.csv [params.txt]]]]]]]
// params.txt receives the likelihood's parameter array (smcmc_set_likelihood_params' layout), so that a saved point can
// be checked against smcmc_event_shape_evaluate.
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "FakeShapeLikelihood_amd.H"

const int gBurninCycles = 5;                                                             // FakeMCMC.C:13-17
const int gChainCycles = 5;

int FakeMCMC3(int dataSignal, int dataBackground, double mcOversample, int burninLength, int chainLength,
              const char* outputName, const char* paramsName) {
    std::cout << "Fake Likelihood MCMC Loaded (template fit with shape weights, MI355X engine)" << std::endl;
    sMCMC::TreeType tree("MCMC", "Tree of accepted points");                             // :28
    sMCMC::TSimpleMCMC<sMCMC::FakeShapeLikelihood> mcmc(&tree);                          // :30
    sMCMC::FakeShapeLikelihood& like = mcmc.GetLogLikelihood();
    sMCMC::TProposeAdaptiveStep& proposal = mcmc.GetProposeStep();

    like.Init(dataSignal, dataBackground, mcOversample);                                 // :36
    std::cout << like.SimulatedSample.size() << " simulated events, signal integral " << like.SignalIntegral
              << ", background integral " << like.BackgroundIntegral << std::endl;
    if (paramsName) like.WriteParams(paramsName);
    proposal.SetDim((int)like.GetDim());                                                 // :69
    proposal.SetGaussian(0, std::sqrt(1.0 + like.MCTrueValues[0]));                      // :71
    proposal.SetGaussian(1, std::sqrt(1.0 + like.MCTrueValues[1]));                      // :72

    sMCMC::Vector p(like.MCTrueValues);                                                  // :78-83
    sMCMC::detail::RestoreUniform uniform(20240607);                                     // :84-85, on the host stream
    for (int k = 0; k < 2; ++k) {
        const double r = std::sqrt(-2.0 * std::log(uniform()));
        p[k] += std::sqrt(p[k]) * r * std::cos(6.283185307179586476925 * uniform());
    }
    if (!mcmc.Start(p, false)) {                                                         // :86
        std::cout << "bad starting point" << std::endl;
        return 1;
    }
    like.WriteSimulation(p, "initial");                                                  // :88

    for (int burnin = 0; burnin < gBurninCycles; ++burnin) {                             // :111-121
        proposal.ResetProposal();
        std::ostringstream name;
        name << "burnin" << burnin + 1;
        const int length = burninLength * (burnin + 1) / gBurninCycles;
        std::cout << "Start new burnin phase (" << length << " steps)" << std::endl;
        for (int i = 0; i < length; ++i) mcmc.Step(false);
        like.WriteSimulation(proposal.GetEstimatedCenter(), name.str());
    }

    const auto t0 = std::chrono::steady_clock::now();
    for (int chain = 0; chain < gChainCycles; ++chain) {                                 // :150-156
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
    tree.Write();                                                                        // :185
#ifndef SMCMC_HAVE_ROOT
    tree.WriteCsv(outputName);
    std::cout << "wrote " << tree.GetEntries() << " entries to " << outputName << std::endl;
#endif
    return 0;
}

int main(int argc, char** argv) {
    int dataSignal = 10000, dataBackground = 100;                                        // FakeMCMC.C:36
    double mcOversample = 10.0;
    int burninLength = 1000, chainLength = 10000;                                        // :14, 17
    std::string outputName("FakeMCMC3_amd.csv");
    if (argc > 1) { std::istringstream in(argv[1]); in >> dataSignal; }
    if (argc > 2) { std::istringstream in(argv[2]); in >> dataBackground; }
    if (argc > 3) { std::istringstream in(argv[3]); in >> mcOversample; }
    if (argc > 4) { std::istringstream in(argv[4]); in >> burninLength; }
    if (argc > 5) { std::istringstream in(argv[5]); in >> chainLength; }
    if (argc > 6) outputName = argv[6];
    const char* paramsName = (argc > 7) ? argv[7] : NULL;
    try {
        return FakeMCMC3(dataSignal, dataBackground, mcOversample, burninLength, chainLength, outputName.c_str(), paramsName);
    } catch (const std::exception& e) {
        std::cerr << "FakeMCMC3_amd: " << e.what() << std::endl;
        return 2;
    }
}
