// Test driver, host only: sMCMC::detail::VaatReplay (include/TProposeVAATStep_amd.H) -- the replay that
// TSimpleMCMC<L, TProposeVAATStep>::Step() serves its caller from while it runs ahead -- fed with rows in the layout of
// smcmc_vaat_step_recorded.  No device, no engine.
// stdin: dim nsteps, then the start state (point[dim], sigma[dim], acceptance[dim], acceptanceTrials[dim]), then nsteps
// rows of SMCMC_VAAT_REC_COUNT_ numbers; every number a hexadecimal float.  stdout, one line per step: point[dim]
// sigma[dim] acceptance[dim] acceptanceTrials[dim] GetSigma GetAcceptance trials successes queueLength, hexadecimal floats.
// tests/test_vaat_record_cpu.py compares them with the CPU restatement of the reference bit for bit.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include "TProposeVAATStep_amd.H"

static double Next() {
    std::string tok;
    if (!(std::cin >> tok)) { std::fprintf(stderr, "vaat_replay_host: input ends early\n"); std::exit(3); }
    return std::strtod(tok.c_str(), nullptr);
}

int main() {
    const int dim = (int)Next(), nsteps = (int)Next();
    if (dim < 1 || nsteps < 0) return 64;
    sMCMC::detail::VaatReplay replay;
    sMCMC::Vector point((std::size_t)dim);
    for (double& v : point) v = Next();
    replay.sigma.resize((std::size_t)dim);
    for (double& v : replay.sigma) v = Next();
    replay.acceptance.resize((std::size_t)dim);
    for (double& v : replay.acceptance) v = Next();
    replay.acceptanceTrials.resize((std::size_t)dim);
    for (int& v : replay.acceptanceTrials) v = (int)Next();
    double row[SMCMC_VAAT_REC_COUNT_];
    for (int s = 0; s < nsteps; ++s) {
        for (double& v : row) v = Next();
        replay.Apply(row, point);
        for (double v : point) std::printf("%a ", v);
        for (double v : replay.sigma) std::printf("%a ", v);
        for (double v : replay.acceptance) std::printf("%a ", v);
        for (int v : replay.acceptanceTrials) std::printf("%a ", (double)v);
        std::printf("%a %a %a %a %a\n", replay.MeanSigma(), replay.MeanAcceptance(), (double)replay.trials,
                    (double)replay.successes, (double)replay.queueLength);
    }
    return 0;
}
