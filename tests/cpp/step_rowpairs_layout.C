// Prints the row-pair LDS image of the accepted point and the accept block of every step-kernel family
// (csrc/smcmc_step_deal.h), for tests/test_step_rowpairs_layout_cpu.py to check.  Plain g++, no HIP.  The addresses are
// formed the way step_kernel forms them (smcmc_kernels.hip.h): a lane's column by XLayout::row, the fold's operand reads
// by row 16 t + (lane & 15) clamped to the ones row, lane (lane >> 4), plus kk k-quad strides.
//
//   layout DP ROWS HELD BYTES PAIR_STRIDE LANE          (the headline kernel's image: moment fold, row pairs)
//   slot r c byte                                       every held row r, lane c
//   operand t kk lane byte                              ds_read_b64 of tile row t, k-quad kk
//   unclamped t kk lane byte                            the same by the layout's formula alone, rows not clamped
//   strip kk lane byte                                ds_read_b64 of the strip rows
//   plain DP ROWS BYTES r c byte ...                    the other instantiations' image at a few (r, c)
//   accept DP fixed block lowest
//   word d accept_word_of smcmc_accept_word
#include <cstdio>

#include "smcmc_detmath.h"
#include "smcmc_step_deal.h"

template <int DP>
static void accept() {
    typedef smcmc::AcceptBlock<DP> AB;
    std::printf("accept %d %d %d %d\n", DP, AB::FIXED ? 1 : 0, AB::BLOCK, AB::LOWEST);
}

int main() {
    constexpr int DP = 50;
    typedef smcmc::XLayout<DP, true, true> XL;
    typedef smcmc::Geo<DP> G;
    static_assert(XL::offset(7, 5) == (7 >> 1) * (64 * 16 + 32) + 5 * 16 + (7 & 1) * 8, "byte offset of (row, lane)");
    std::printf("layout %d %d %d %d %d %d\n", DP, XL::ROWS, XL::HELD, XL::BYTES, XL::PAIR_STRIDE, XL::LANE);
    for (int r = 0; r < XL::HELD; ++r)
        for (int c = 0; c < 64; ++c) std::printf("slot %d %d %d\n", r, c, XL::offset(r, c));
    constexpr int KQ = 4 * 8 * XL::LANE;
    for (int t = 0; t < G::T; ++t)
        for (int kk = 0; kk < 16; ++kk)
            for (int lane = 0; lane < 64; ++lane) {
                const int r = 16 * t + (lane & 15);
                std::printf("operand %d %d %d %d\n", t, kk, lane, XL::offset(r <= DP ? r : DP, lane >> 4) + KQ * kk);
                // the same read without the clamp (the layout's formula alone; rows past HELD lie outside the image)
                std::printf("unclamped %d %d %d %d\n", t, kk, lane, XL::offset(r, lane >> 4) + KQ * kk);
            }
    for (int kk = 0; kk < 16; ++kk)
        for (int lane = 0; lane < 64; ++lane) {
            const int r = 16 * G::T16 + (lane & 3);
            std::printf("strip %d %d %d\n", kk, lane, XL::offset(r <= DP ? r : DP, lane >> 4) + KQ * kk);
        }
    typedef smcmc::XLayout<DP, true, false> XP;
    std::printf("plain %d %d %d", DP, XP::ROWS, XP::BYTES);
    for (int r = 0; r <= DP; r += 25)
        for (int c = 0; c < 64; c += 21) std::printf(" %d %d %d", r, c, XP::offset(r, c));
    std::printf("\n");
    accept<7>();
    accept<15>();
    accept<31>();
    accept<47>();
    accept<50>();
    accept<63>();
    for (unsigned d = 1; d <= 63; ++d) std::printf("word %u %u %u\n", d, smcmc::accept_word_of(d), smcmc_accept_word(d));
    return 0;
}
