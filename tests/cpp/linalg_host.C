// linalg_host.C -- the host's dense factorisations on matrices read from a file, for tests/test_linalg_truth_cpu.py.
//
// usage: linalg_host.exe IN OUT.  IN holds records, all little-endian: int32 op, int32 n, double p0, double p1, then the
// n x n matrix in row order as raw doubles.  OUT receives raw doubles per record:
//   op 0  SharedProposal::choleskyOnly() on cov:          ok, decomp[n*n]
//   op 1  SharedProposal::finishUpdateOnHost(1.0) on cov (every ptype 0, every param1 0):
//                                                         status, lastPath, decompFull, cov[n*n], decomp[n*n]
//   op 2  HmcShared::finishUpdate() on cov with estTrace = p0, covTrials = p1:
//                                                         cov[n*n], error[n*n], maxScale, minScale, orbitLength, estTrace
#include <cstdint>
#include <cstdio>
#include <vector>

#include "smcmc_hmc_shared.hpp"
#include "smcmc_proposal.hpp"

static void put(std::FILE* f, const std::vector<double>& v) { std::fwrite(v.data(), sizeof(double), v.size(), f); }
static void put(std::FILE* f, double v) { std::fwrite(&v, sizeof(double), 1, f); }

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open the files\n"); return 2; }
    for (;;) {
        int32_t head[2];
        double prm[2];
        if (std::fread(head, sizeof(int32_t), 2, in) != 2) break;
        const int op = head[0], n = head[1];
        if (n < 1 || n > 4096 || std::fread(prm, sizeof(double), 2, in) != 2) { std::fprintf(stderr, "bad record\n"); return 1; }
        std::vector<double> a((size_t)n * n);
        if (std::fread(a.data(), sizeof(double), a.size(), in) != a.size()) { std::fprintf(stderr, "short matrix\n"); return 1; }
        if (op == 0) {
            smcmc::SharedProposal p(n);
            p.cov = a;
            put(out, p.choleskyOnly() ? 1.0 : 0.0);
            put(out, p.decomp);
        } else if (op == 1) {
            smcmc::SharedProposal p(n);
            p.cov = a;
            const smcmc::UpdateStatus st = p.finishUpdateOnHost(1.0);
            put(out, (double)(int)st);
            put(out, (double)p.lastPath);
            put(out, p.decompFull ? 1.0 : 0.0);
            put(out, p.cov);
            put(out, p.decomp);
        } else if (op == 2) {
            smcmc::HmcShared h(n);
            h.cov = a;
            h.estTrace = prm[0];
            h.covTrials = prm[1];
            h.finishUpdate();
            put(out, h.cov);
            put(out, h.error);
            put(out, h.maxScale);
            put(out, h.minScale);
            put(out, h.orbitLength);
            put(out, h.estTrace);
        } else {
            std::fprintf(stderr, "unknown op %d\n", op);
            return 1;
        }
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 1;
}
