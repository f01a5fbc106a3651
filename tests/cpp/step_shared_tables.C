// Prints the LDS of the headline step kernels' workgroup and the replicated tables of the normal transform
// (StepWorkgroupLds, NormalTableLayout of csrc/smcmc_step_deal.h), for tests/test_step_shared_tables_cpu.py to check.
// Plain g++, no HIP.  A gather's address is formed the way step_kernel forms it (smcmc_kernels.hip.h): the lane's part,
// lane_offset, plus the index shifted by SHIFT; a staged slot the way the prologue fills it.
//
//   lds DP MOMENTS IMAGE_BYTES US US_BYTES LOG LOG_BYTES ANGLE ANGLE_BYTES TOTAL LIMIT
//   image DP MOMENTS wave byte                 start of a wavefront's image of the accepted point
//   table name ENTRIES COPIES STRIDE SHIFT BYTES SLOTS
//   lane name lane byte                        the lane's part of a gather's address (from the table's start)
//   entry name copy k byte                     NormalTableLayout::offset(copy, k)
//   slot name s byte source                    the prologue writes entry `source` of the table to 16 bytes at `byte`
//   group block wave group                     chain group of wavefront `wave` of block `block`
//   blocks groups n                            the grid for `groups` chain groups
#include <cstdio>

#include "smcmc_step_deal.h"

template <bool MOMENTS>
static void lds() {
    constexpr int DP = 50;
    typedef smcmc::StepWorkgroupLds<DP, MOMENTS> WL;
    static_assert(WL::IMAGE_BYTES >= smcmc::XLayout<DP, MOMENTS, true>::BYTES, "an image holds the row pairs");
    std::printf("lds %d %d %d %d %d %d %d %d %d %d %d\n", DP, MOMENTS ? 1 : 0, WL::IMAGE_BYTES, WL::US, WL::US_BYTES, WL::LOG,
                smcmc::LogTableLayout::BYTES, WL::ANGLE, smcmc::AngleTableLayout::BYTES, WL::TOTAL, smcmc::kLdsPerCU);
    for (int w = 0; w < smcmc::kStepWaves; ++w) std::printf("image %d %d %d %d\n", DP, MOMENTS ? 1 : 0, w, WL::image(w));
}

template <typename TL>
static void table(const char* name, int entries) {
    std::printf("table %s %d %d %d %d %d %d\n", name, entries, TL::STRIDE / TL::ENTRY_BYTES, TL::STRIDE, TL::SHIFT, TL::BYTES, TL::SLOTS);
    for (int lane = 0; lane < 64; ++lane) std::printf("lane %s %d %d\n", name, lane, TL::lane_offset(lane));
    for (int c = 0; c < TL::STRIDE / TL::ENTRY_BYTES; ++c)
        for (int k = 0; k < entries; ++k) std::printf("entry %s %d %d %d\n", name, c, k, TL::offset(c, k));
    for (int s = 0; s < TL::SLOTS; ++s) std::printf("slot %s %d %d %d\n", name, s, TL::slot_offset(s), TL::slot_entry(s));
}

int main() {
    lds<true>();
    lds<false>();
    table<smcmc::LogTableLayout>("log", 64);
    table<smcmc::AngleTableLayout>("angle", 128);
    for (int b = 0; b < 3; ++b)
        for (int w = 0; w < smcmc::kStepWaves; ++w) std::printf("group %d %d %d\n", b, w, smcmc::step_group_of(b, w));
    for (int g = 1; g <= 9; ++g) std::printf("blocks %d %d\n", g, smcmc::step_blocks_for(g));
    return 0;
}
