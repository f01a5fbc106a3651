// BadGrad_amd.C -- the reference's approximate-gradient experiment (BadGrad.C) on the MI355X engine: a quadratic-form
// likelihood whose gradient is computed from a DIFFERENT matrix than the likelihood itself, on purpose.  HMC stays
// correct because the leapfrog is reversible whatever the gradient is (TSimpleHMC.H:101-108); a wrong gradient only
// costs acceptance.  As in BadGrad.C:176 the likelihood type is also the OptionalGradient:
//     sMCMC::TSimpleHMC<TBadGradLogLikelihood, TBadGradLogLikelihood>
// and because the type has kDeviceGradientMatrix, Start hands GradientError to smcmc_hmc_set_gradient_matrix: gradient
// types 0 / 1 / 4 compute g = -GradientError q on the device while the potential stays that of Error.
// Schedule of BadGrad.C:186-203: a start point uniform in (-1, 1), no burn-in of its own, `trials` saved steps with
// a progress line every 1000, an optional limit on the likelihood calls.  Differences: dimension (BadGrad.C: 50), chain
// count and seed are arguments; the random numbers that perturb the gradient covariance come from std::mt19937, not
// gRandom; positive definiteness is tested by a Cholesky factorisation instead of the eigenvalues.
//
//   g++ -std=c++17 -O2 -Iinclude examples/BadGrad_amd.C -Lroot-simple-mcmc_amd/lib -lsmcmc_amd
//       -Wl,-rpath,$PWD/root-simple-mcmc_amd/lib -Wl,-rpath,/opt/rocm/lib -o badgrad_amd.exe
//   ./badgrad_amd.exe [maxEvals [trials [output.csv [dim [chains [seed]]]]]]
#include <cmath>
#include <cstdlib>
#include <iostream>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>
#include <utility>

#include "TSimpleHMC_amd.H"

class TBadGradLogLikelihood {
public:
    static constexpr int kDeviceLikelihood = SMCMC_LIKE_QUADFORM;
    static constexpr bool kDeviceGradientMatrix = true;
    void SetDim(std::size_t d) { fDim = d; }
    void SetSeed(unsigned seed) { fSeed = seed; }
    std::size_t GetDim() const { return fDim; }

    double operator()(const sMCMC::Vector& point) const {             // BadGrad.C:20-30
        double logLikelihood = 0.0;
        for (std::size_t i = 0; i < fDim; ++i)
            for (std::size_t j = 0; j < fDim; ++j) logLikelihood -= 0.5 * point[i] * Error[j * fDim + i] * point[j];
        return logLikelihood;
    }
    bool operator()(sMCMC::Vector& g, const sMCMC::Vector& p) const {   // :33-41, the wrong gradient
        for (std::size_t i = 0; i < p.size(); ++i) {
            g[i] = 0.0;
            for (std::size_t j = 0; j < p.size(); ++j) g[i] -= GradientError[i * fDim + j] * p[j];
        }
        return true;
    }

    void Init() {                                                      // :43-150
        const std::size_t n = fDim;
        Covariance.assign(n * n, 0.0);
        for (std::size_t i = 0; i < n; ++i) Covariance[i * n + i] = 1.0;
        for (std::size_t i = 0; i < n; ++i)                            // VERY_CORRELATED, :72-76: the anti-diagonal
            for (std::size_t j = i + 1; j < n; ++j)
                if (i + j == n - 1) Covariance[i * n + j] = Covariance[j * n + i] = 0.900 * (double)(j - i) / (n - 1.0);
        MakePositiveDefinite(Covariance);                              // :82-100
        Error = Inverse(Covariance);
        // a gradient covariance that is wrong on purpose (:104-123): every variance scaled by Gaus(1, 0.1) (at least
        // 0.3), every covariance moved by Gaus(0, 0.3) sigma_i sigma_j
        std::mt19937 rng(fSeed);
        std::normal_distribution<double> gaus(0.0, 1.0);
        GradientCovariance.assign(n * n, 0.0);
        for (std::size_t i = 0; i < n; ++i)
            for (std::size_t j = i; j < n; ++j) {
                double r = Covariance[i * n + j];
                if (i == j) {
                    double e = 1.0 + 0.1 * gaus(rng);
                    while (e < 0.3) e = 1.0 + 0.1 * gaus(rng);
                    r = r * e;
                } else {
                    r = r + 0.3 * gaus(rng) * std::sqrt(Covariance[i * n + i]) * std::sqrt(Covariance[j * n + j]);
                }
                GradientCovariance[i * n + j] = GradientCovariance[j * n + i] = r;
            }
        MakePositiveDefinite(GradientCovariance);                      // :126-143
        GradientError = Inverse(GradientCovariance);
    }

    sMCMC::Vector DeviceParams() const { return Error; }
    sMCMC::Vector DeviceGradientMatrix() const { return GradientError; }
    sMCMC::Vector Covariance, Error, GradientCovariance, GradientError;

private:
    static bool PositiveDefinite(const sMCMC::Vector& a, std::size_t n) {
        sMCMC::Vector l(n * n, 0.0);
        for (std::size_t i = 0; i < n; ++i)
            for (std::size_t j = 0; j <= i; ++j) {
                double s = a[i * n + j];
                for (std::size_t k = 0; k < j; ++k) s -= l[i * n + k] * l[j * n + k];
                if (i == j) {
                    if (!(s > 0.0)) return false;
                    l[i * n + i] = std::sqrt(s);
                } else {
                    l[i * n + j] = s / l[j * n + j];
                }
            }
        return true;
    }
    // shrink the correlations by 0.9 until the matrix is positive definite
    void MakePositiveDefinite(sMCMC::Vector& a) const {
        const std::size_t n = fDim;
        while (!PositiveDefinite(a, n))
            for (std::size_t i = 0; i < n; ++i)
                for (std::size_t j = i + 1; j < n; ++j) a[i * n + j] = a[j * n + i] = 0.9 * a[i * n + j];
    }
    // Gauss-Jordan with partial pivoting
    sMCMC::Vector Inverse(const sMCMC::Vector& m) const {
        const std::size_t n = fDim, w = 2 * n;
        sMCMC::Vector a(n * w, 0.0);
        for (std::size_t i = 0; i < n; ++i) {
            for (std::size_t j = 0; j < n; ++j) a[i * w + j] = m[i * n + j];
            a[i * w + n + i] = 1.0;
        }
        for (std::size_t col = 0; col < n; ++col) {
            std::size_t piv = col;
            for (std::size_t r = col + 1; r < n; ++r)
                if (std::fabs(a[r * w + col]) > std::fabs(a[piv * w + col])) piv = r;
            if (a[piv * w + col] == 0.0) throw std::runtime_error("singular matrix");
            if (piv != col) for (std::size_t k = 0; k < w; ++k) std::swap(a[col * w + k], a[piv * w + k]);
            const double d = a[col * w + col];
            for (std::size_t k = 0; k < w; ++k) a[col * w + k] /= d;
            for (std::size_t r = 0; r < n; ++r) {
                const double f = a[r * w + col];
                if (r == col || f == 0.0) continue;
                for (std::size_t k = 0; k < w; ++k) a[r * w + k] -= f * a[col * w + k];
            }
        }
        sMCMC::Vector inv(n * n, 0.0);
        for (std::size_t i = 0; i < n; ++i)
            for (std::size_t j = 0; j < n; ++j) inv[i * n + j] = a[i * w + n + j];
        return inv;
    }
    std::size_t fDim = 50;                                             // BadGrad.C:15
    unsigned fSeed = 20240607u;
};

int BadGrad(int maxEvals, int trials, const char* outputName, int dim, int chains, unsigned seed) {
    std::cout << "Bad-gradient HMC (MI355X engine) D=" << dim << " chains=" << chains << std::endl;
    sMCMC::TreeType tree("BadGrad", "Tree of accepted points");
    sMCMC::TSimpleHMC<TBadGradLogLikelihood, TBadGradLogLikelihood> hmc(&tree);
    TBadGradLogLikelihood& like = hmc.GetLogLikelihood();
    like.SetDim(dim);
    like.SetSeed(seed);
    like.Init();
    hmc.SetChains(chains);
    hmc.SetSeed(seed);

    std::mt19937 rng(seed + 1u);
    std::uniform_real_distribution<double> uniform(-1.0, 1.0);
    sMCMC::Vector p(like.GetDim());
    for (std::size_t i = 0; i < p.size(); ++i) p[i] = uniform(rng);   // BadGrad.C:187
    hmc.Start(p, false);

    for (int i = 0; i < trials; ++i) {                                  // :192-203
        if (i % 1000 == 0) std::cout << i << " " << hmc.GetPotentialCount() << " " << hmc.GetGradientCount() << std::endl;
        hmc.Step(true);
        if (maxEvals > 0 && hmc.GetPotentialCount() > maxEvals) break;
    }
    std::cout << "Finished " << trials << " requested trials with calls " << hmc.GetPotentialCount() << " + "
              << hmc.GetGradientCount() << " " << 1.0 * hmc.GetGradientCount() / hmc.GetPotentialCount() << ", acceptance "
              << hmc.GetAcceptanceRate() << std::endl;
    tree.Write();
#ifndef SMCMC_HAVE_ROOT
    tree.WriteCsv(outputName);
    std::cout << "wrote " << tree.GetEntries() << " entries to " << outputName << std::endl;
#endif
    return 0;
}

int main(int argc, char** argv) {
    int maxEvals = -1, trials = 1000, dim = 50, chains = 64;
    unsigned seed = 20240607u;
    std::string outputName("BadGrad_amd.csv");
    if (argc > 1) { std::istringstream in(argv[1]); in >> maxEvals; }
    if (argc > 2) { std::istringstream in(argv[2]); in >> trials; }
    if (argc > 3) outputName = argv[3];
    if (argc > 4) { std::istringstream in(argv[4]); in >> dim; }
    if (argc > 5) { std::istringstream in(argv[5]); in >> chains; }
    if (argc > 6) { std::istringstream in(argv[6]); in >> seed; }
    try {
        return BadGrad(maxEvals, trials, outputName.c_str(), dim, chains, seed);
    } catch (const std::exception& e) {
        std::cerr << "BadGrad_amd: " << e.what() << std::endl;
        return 2;
    }
}
