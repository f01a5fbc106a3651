// The index helpers of the streamed per-chain kernel (csrc/smcmc_perchain_stream_index.h), walked on the host: for every
// dimension given and every packed slot, row-major slot <-> (a, b) <-> tile index k round-trips, the slots cover the
// upper triangle exactly once, rows are contiguous, and the kernel's stride-512 walks (st_advance_slot, st_advance_k)
// from every thread's first element land where the direct unpacking says -- and never on an index past the triangle.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "smcmc_perchain_stream_index.h"

using namespace smcmc;

static int failures = 0;
#define EXPECT(cond, ...)                                   \
    do {                                                    \
        if (!(cond)) {                                      \
            if (++failures <= 20) {                         \
                std::printf("FAIL %s: ", #cond);            \
                std::printf(__VA_ARGS__);                   \
                std::printf("\n");                          \
            }                                               \
        }                                                   \
    } while (0)

static void check_dim(int D) {
    const int npk = st_packed(D), threads = 512;
    EXPECT(npk == D * (D + 1) / 2, "D=%d", D);
    std::vector<int> seen_slot((size_t)npk, 0), seen_k((size_t)npk, 0);
    // (a, b) -> slot and k, and back
    int expect_m = 0;
    for (int a = 0; a < D; ++a) {
        EXPECT(st_row_start(a, D) == expect_m, "D=%d row %d starts at %d, expected %d", D, a, st_row_start(a, D), expect_m);
        for (int b = a; b < D; ++b, ++expect_m) {
            const int m = st_slot(a, b, D), k = st_tile_k(a, b);
            EXPECT(m == expect_m, "D=%d (%d, %d): slot %d, rows must be contiguous (%d)", D, a, b, m, expect_m);
            EXPECT(m >= 0 && m < npk && k >= 0 && k < npk, "D=%d (%d, %d): slot %d k %d out of range", D, a, b, m, k);
            if (m < 0 || m >= npk || k < 0 || k >= npk) continue;
            ++seen_slot[(size_t)m];
            ++seen_k[(size_t)k];
            int a2 = -1, b2 = -1, a3 = -1, b3 = -1;
            st_unpack_slot(m, D, a2, b2);
            st_unpack_k(k, a3, b3);
            EXPECT(a2 == a && b2 == b, "D=%d slot %d -> (%d, %d), expected (%d, %d)", D, m, a2, b2, a, b);
            EXPECT(a3 == a && b3 == b, "D=%d k %d -> (%d, %d), expected (%d, %d)", D, k, a3, b3, a, b);
        }
    }
    EXPECT(expect_m == npk, "D=%d: %d slots walked, %d packed", D, expect_m, npk);
    for (int i = 0; i < npk; ++i) {
        EXPECT(seen_slot[(size_t)i] == 1, "D=%d slot %d covered %d times", D, i, seen_slot[(size_t)i]);
        EXPECT(seen_k[(size_t)i] == 1, "D=%d k %d covered %d times", D, i, seen_k[(size_t)i]);
    }
    // the tile index of a slot is that of the lower-triangle element (b, a), row major
    for (int m = 0; m < npk; ++m) {
        int a, b;
        st_unpack_slot(m, D, a, b);
        EXPECT(a >= 0 && a <= b && b < D, "D=%d slot %d -> (%d, %d)", D, m, a, b);
        EXPECT(st_tile_k(a, b) == b * (b + 1) / 2 + a, "D=%d slot %d", D, m);
    }
    // the kernel's walks: thread t starts at element t and goes on in strides of 512
    for (int t = 0; t < threads; ++t) {
        int a, b;
        st_unpack_slot(t, D, a, b);
        for (int m = t; m < npk; m += threads) {
            int a2, b2;
            st_unpack_slot(m, D, a2, b2);
            EXPECT(a == a2 && b == b2, "D=%d thread %d slot %d: walk (%d, %d), direct (%d, %d)", D, t, m, a, b, a2, b2);
            EXPECT(st_tile_k(a, b) < npk, "D=%d thread %d slot %d: k past the triangle", D, t, m);
            st_advance_slot(a, b, D, threads);       // (the last one runs off the end: it must stop)
        }
        EXPECT(a <= D, "D=%d thread %d: the walk went on past row D (%d)", D, t, a);
        int ka, kb;
        st_unpack_k(t, ka, kb);
        for (int k = t; k < npk; k += threads) {
            int a2, b2;
            st_unpack_k(k, a2, b2);
            EXPECT(ka == a2 && kb == b2, "D=%d thread %d k %d: walk (%d, %d), direct (%d, %d)", D, t, k, ka, kb, a2, b2);
            EXPECT(ka <= kb && kb < D, "D=%d thread %d k %d: (%d, %d) outside the matrix", D, t, k, ka, kb);
            st_advance_k(ka, kb, threads);
        }
    }
    // the proposal's and the Cholesky's running slot: st_slot(i + 1, j) = st_slot(i, j) + D - i - 1
    for (int j = 0; j < D; ++j) {
        int s = j;
        for (int i = 0; i <= j; ++i) {
            EXPECT(s == st_slot(i, j, D), "D=%d column %d row %d: running slot %d, direct %d", D, j, i, s, st_slot(i, j, D));
            s += D - i - 1;
        }
    }
}

int main(int argc, char** argv) {
    int ndims = 0;
    for (int i = 1; i < argc; ++i) {
        const int D = std::atoi(argv[i]);
        if (D < kStMinDim || D > kStMaxDim) {
            std::printf("dimension %d is outside [%d, %d]\n", D, kStMinDim, kStMaxDim);
            return 2;
        }
        check_dim(D);
        ++ndims;
    }
    std::printf("dims %d failures %d max_dim %d\n", ndims, failures, kStMaxDim);
    return failures ? 1 : 0;
}
