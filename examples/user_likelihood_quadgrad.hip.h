// user_likelihood_quadgrad.hip.h -- a user likelihood WITH a gradient of its own for the MI355X engine: the pair
// BadGrad.C gives to sMCMC::TSimpleHMC<TDummyLogLikelihood, TDummyLogLikelihood> (BadGrad.C:21-41, 176), as device code.
//
//   python root-simple-mcmc_amd/build.py --user-likelihood examples/user_likelihood_quadgrad.hip.h --output-name user_grad
//
// gives lib/libsmcmc_amd_user_grad.so, in which smcmc_hmc_create(..., SMCMC_LIKE_USER, ...) runs gradient types 0 / 1 / 4
// on smcmc_user_gradient_at below instead of refusing them (smcmc_hmc_has_gradient() == 1).
//
// Parameters (smcmc_hmc_set_likelihood_params): Error, row-major, in params[0 .. D*D); GradientError in
// params[D*D .. 2*D*D).  The likelihood reads only the first matrix, the gradient only the second: with two different
// matrices the gradient is wrong on purpose, which HMC tolerates as long as the leapfrog stays reversible
// (TSimpleHMC.H:101-108); with the same matrix twice the chain is the built-in SMCMC_LIKE_QUADFORM chain of the
// reference's own summation order.
#pragma once

// TDummyLogLikelihood.H:24-27 on a point held in registers (dim <= 63): i outer, j inner, one subtraction per term,
//     logLikelihood -= 0.5*point[i]*Error(j,i)*point[j];
// The outer loop stays rolled (63 x 63 unrolled terms would take minutes to compile); point[i] is picked out of the
// register array by a chain of selects so that the array is only ever indexed by constants.
template <int DP>
__device__ __forceinline__ double smcmc_user_loglike(const double (&p)[DP], smcmc::cptr_f64 params, int D) {
    double logLikelihood = 0.0;
#pragma nounroll
    for (int i = 0; i < D; ++i) {
        double pi = 0.0;
#pragma unroll
        for (int k = 0; k < DP; ++k) pi = (k == i) ? p[k] : pi;
#pragma unroll
        for (int j = 0; j < DP; ++j) {
            if (j < D) logLikelihood -= 0.5 * pi * params[j * D + i] * p[j];
        }
    }
    return logLikelihood;
}

// The same sum for any dimension: p[i] reads coordinate i of the chain's point from device memory.
#define SMCMC_USER_LIKELIHOOD_ANY_DIM 1

template <class Point>
__device__ __forceinline__ double smcmc_user_loglike_at(const Point& p, const double* params, int D) {
    double logLikelihood = 0.0;
    for (int i = 0; i < D; ++i) {
        const double pi = p[i];
        for (int j = 0; j < D; ++j) logLikelihood -= 0.5 * pi * params[(size_t)j * D + i] * p[j];
    }
    return logLikelihood;
}

// Component i of the gradient of log L (BadGrad.C:33-41): g[i] = 0.0; g[i] -= GradientError(i,j)*p[j], j ascending.
// The HMC step kernel calls it for the components a wavefront owns, every chain of the wavefront in its own lane; the
// engine negates the result (TSimpleHMC.H:486).  Defining SMCMC_USER_GRADIENT tells the build that it exists.
#define SMCMC_USER_GRADIENT 1

template <class Point>
__device__ __forceinline__ double smcmc_user_gradient_at(const Point& p, const double* params, int D, int i) {
    const double* G = params + (size_t)D * D + (size_t)i * D;
    double g = 0.0;
    for (int j = 0; j < D; ++j) g -= G[j] * p[j];
    return g;
}
