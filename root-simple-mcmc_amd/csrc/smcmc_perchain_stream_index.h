// smcmc_perchain_stream_index.h -- where the elements of one chain's two matrices lie in the working copies of the
// streamed per-chain kernel (smcmc_perchain_stream.hip.h).  Plain integer arithmetic that compiles with and without
// HIP: tests/cpp/perchain_stream_index.C walks it on the host for every slot of the dimensions the kernel serves.
//
//   wcov[k], k = b (b + 1) / 2 + a, a <= b: the covariance element (b, a) -- the lower triangle row major, the index
//             of the host-visible tiled image (pc_tile_index's k), which is also where that image keeps U(a, b);
//   wU[m],   m = st_row_start(a, D) + (b - a), a <= b: U(a, b) -- the upper triangle row major, so that for a fixed row
//             the threads that own neighbouring columns read neighbouring doubles.
#pragma once

#if defined(__HIPCC__)
#define SMCMC_ST_HD __host__ __device__ inline
#else
#define SMCMC_ST_HD inline
#endif

namespace smcmc {

constexpr int kStMaxDim = 512;               // one thread per coordinate of a workgroup of 512
constexpr int kStMinDim = 64;                // below it the default kernels serve the mode

SMCMC_ST_HD int st_packed(int D) { return D * (D + 1) / 2; }

// start of row a of U in the row-major packing of the upper triangle
SMCMC_ST_HD int st_row_start(int a, int D) { return a * D - a * (a - 1) / 2; }

// slot of U(a, b), a <= b < D
SMCMC_ST_HD int st_slot(int a, int b, int D) { return st_row_start(a, D) + (b - a); }

// index of covariance (b, a) and of U(a, b), a <= b, in the tiled images
SMCMC_ST_HD int st_tile_k(int a, int b) { return b * (b + 1) / 2 + a; }

// (row, column) of U for slot m < st_packed(D)
SMCMC_ST_HD void st_unpack_slot(int m, int D, int& a, int& b) {
    const double t = 2.0 * D + 1.0;
    a = (int)((t - __builtin_sqrt(t * t - 8.0 * (double)m)) * 0.5);
    if (a < 0) a = 0;
    if (a > D - 1) a = D - 1;
    while (a > 0 && st_row_start(a, D) > m) --a;
    while (a + 1 < D && st_row_start(a + 1, D) <= m) ++a;
    b = a + (m - st_row_start(a, D));
}

// (a, b), a <= b, of tile index k = b (b + 1) / 2 + a
SMCMC_ST_HD void st_unpack_k(int k, int& a, int& b) {
    b = (int)((__builtin_sqrt(8.0 * (double)k + 1.0) - 1.0) * 0.5);
    if (b < 0) b = 0;
    while ((b + 1) * (b + 2) / 2 <= k) ++b;
    while (b > 0 && b * (b + 1) / 2 > k) --b;
    a = k - b * (b + 1) / 2;
}

// slot m -> slot m + n: (a, b) of the slot n places on.  Past the last slot it stops at row D (no slot).
SMCMC_ST_HD void st_advance_slot(int& a, int& b, int D, int n) {
    int off = b - a + n;
    while (a < D && off >= D - a) {
        off -= D - a;
        ++a;
    }
    b = a + off;
}

// tile index k -> k + n
SMCMC_ST_HD void st_advance_k(int& a, int& b, int n) {
    a += n;
    while (a > b) {
        a -= b + 1;
        ++b;
    }
}

}  // namespace smcmc
