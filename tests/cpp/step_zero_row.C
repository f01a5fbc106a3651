// Prints the addresses of the moment fold's operand reads of the headline step kernel, DP = 50, formed the way step_kernel
// (csrc/smcmc_kernels.hip.h) forms them with ZROW: row 16 t + (lane & 15) of chain 4 kk + (lane >> 4), the tile rows past
// the ones row sent to the image's zero row (XLayout::ZERO_ROW of csrc/smcmc_step_deal.h) instead of clamped onto the ones
// row.  tests/test_step_rms_blocks_cpu.py reads the output.  Plain g++, no HIP.
//
//   zero ZERO_ROW ROWS HELD BYTES PAIR_STRIDE
//   slot r c byte                                       the zero row and the ones row, every lane c
//   zoperand t kk lane byte                             ds_read_b64 of tile row t, k-quad kk
//   zstrip kk lane byte                                 ds_read_b64 of the strip rows
#include <cstdio>

#include "smcmc_step_deal.h"

int main() {
    constexpr int DP = 50;
    typedef smcmc::XLayout<DP, true, true> XL;
    typedef smcmc::Geo<DP> G;
    static_assert(XL::ZERO_ROW == DP + 1 && XL::ZERO_ROW < XL::HELD, "the ones row's partner, inside the image");
    static_assert(smcmc::XLayout<DP, false, true>::ZERO_ROW < 0 && smcmc::XLayout<DP, true, false>::ZERO_ROW < 0,
                  "only the image with the fold, in row pairs, has the row");
    std::printf("zero %d %d %d %d %d\n", XL::ZERO_ROW, XL::ROWS, XL::HELD, XL::BYTES, XL::PAIR_STRIDE);
    for (int c = 0; c < 64; ++c) {
        std::printf("slot %d %d %d\n", DP, c, XL::offset(DP, c));
        std::printf("slot %d %d %d\n", XL::ZERO_ROW, c, XL::offset(XL::ZERO_ROW, c));
    }
    constexpr int KQ = 4 * 8 * XL::LANE;
    for (int t = 0; t < G::T; ++t)
        for (int kk = 0; kk < 16; ++kk)
            for (int lane = 0; lane < 64; ++lane) {
                const int r = 16 * t + (lane & 15);
                std::printf("zoperand %d %d %d %d\n", t, kk, lane, XL::offset(r <= DP ? r : XL::ZERO_ROW, lane >> 4) + KQ * kk);
            }
    for (int kk = 0; kk < 16; ++kk)
        for (int lane = 0; lane < 64; ++lane) {
            const int r = 16 * G::T16 + (lane & 3);
            std::printf("zstrip %d %d %d\n", kk, lane, XL::offset(r <= DP ? r : XL::ZERO_ROW, lane >> 4) + KQ * kk);
        }
    return 0;
}
