/* smcmc_order_key.h -- the total order the order statistics of a saved trace are taken in (include/smcmc.h states it
 * under smcmc_trace_order_statistics), one copy for the device kernels (smcmc_order_statistics.hip) and for the host
 * entry points smcmc_order_key / smcmc_order_value.
 *
 * With b the 64 bits of a double,
 *   key(x) = b ^ (b >> 63 ? 0xFFFFFFFFFFFFFFFF : 0x8000000000000000)        every NaN, of either sign: 0xFFFFFFFFFFFFFFFF
 * A non-negative double's bits grow with its value, so setting the sign bit puts them above every negative one; a
 * negative double's bits grow with its magnitude, so inverting them all makes them grow with its value.  Unsigned
 * comparison of keys is then the total order
 *   -inf < ... < -0 < +0 < ... < +inf < NaN.
 * No finite double or infinity has the all-ones key: it would be the bits 0x7FFFFFFFFFFFFFFF, a NaN.  value(key) is
 * the inverse, and the quiet NaN 0x7FF8000000000000 for the all-ones key.  Integer operations only: the same bits on
 * the host and on gfx950.
 */
#ifndef SMCMC_ORDER_KEY_H_SEEN
#define SMCMC_ORDER_KEY_H_SEEN

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SMCMC_ORDER_HD __host__ __device__ __forceinline__
#elif defined(__cplusplus)
#define SMCMC_ORDER_HD inline
#else
#define SMCMC_ORDER_HD static inline
#endif

#define SMCMC_ORDER_KEY_NAN 0xFFFFFFFFFFFFFFFFull

/* the key of the double whose bits are b */
SMCMC_ORDER_HD uint64_t smcmc_order_key_of_bits(uint64_t b) {
    if ((b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return SMCMC_ORDER_KEY_NAN;
    return b ^ ((b >> 63) ? 0xFFFFFFFFFFFFFFFFull : 0x8000000000000000ull);
}

/* the bits of the double whose key is k */
SMCMC_ORDER_HD uint64_t smcmc_order_bits_of_key(uint64_t k) {
    if (k == SMCMC_ORDER_KEY_NAN) return 0x7FF8000000000000ull;
    return k ^ ((k >> 63) ? 0x8000000000000000ull : 0xFFFFFFFFFFFFFFFFull);
}

SMCMC_ORDER_HD uint64_t smcmc_order_key_of(double x) {
    uint64_t b;
    memcpy(&b, &x, sizeof b);
    return smcmc_order_key_of_bits(b);
}

SMCMC_ORDER_HD double smcmc_order_value_of(uint64_t k) {
    const uint64_t b = smcmc_order_bits_of_key(k);
    double x;
    memcpy(&x, &b, sizeof x);
    return x;
}

#endif
