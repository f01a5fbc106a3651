// Prints the deal of the moment fold's matrix instructions over the pieces of a step (csrc/smcmc_step_deal.h) for the
// headline family, DP = 50: the plan and, scored by the same model, the uniform deal of the kernels without a plan.
// tests/test_step_deal_plan_cpu.py reads the output and checks the plan's invariants.
//
//   geometry G NQ NT NT16 PREFETCH
//   <name> score S
//   <name> slot g fill F : kk.tile[p] kk.tile ...      ([p]: the next k-quad's operand prefetch right behind it)
#include <cstdio>

#include "smcmc_step_deal.h"

typedef smcmc::StepDeal<50> SD;

static void print(const char* name, const SD::Plan& p) {
    std::printf("%s score %d\n", name, p.score);
    for (int g = 0; g < SD::G; ++g) {
        std::printf("%s slot %d fill %d :", name, g, p.fill[g]);
        for (int m = p.first[g]; m < p.first[g + 1]; ++m)
            std::printf(" %d.%d%s", p.kk[m], p.tile[m], p.pf_after[m] ? "p" : "");
        std::printf("\n");
    }
}

int main() {
    static_assert(SD::valid(smcmc::kStepDealPlan<50>), "the plan breaks an invariant");
    static_assert(SD::valid(smcmc::kStepDealUniform<50>), "the uniform deal breaks an invariant");
    std::printf("geometry %d %d %d %d %d\n", SD::G, SD::NQ, SD::NT, SD::NT16, SD::PREFETCH);
    print("plan", smcmc::kStepDealPlan<50>);
    print("uniform", smcmc::kStepDealUniform<50>);
    return 0;
}
