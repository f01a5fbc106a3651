// fake_shape_host.C -- sMCMC::TFakeGP (include/TFakeGP_amd.H) and sMCMC::FakeShapeLikelihood
// (include/FakeShapeLikelihood_amd.H) through their host paths alone, for tests/test_cpp_fake_shape.py: Init(),
// DeviceParams() written to argv[4], operator() at a point with every shape parameter set, and TFakeGP::GetValue /
// GetPenalty of the two shapes at that point.
//   ./fake_shape_host.exe dataSignal dataBackground mcOversample params.txt
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "FakeShapeLikelihood_amd.H"

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    try {
        sMCMC::FakeShapeLikelihood like;
        like.Init(std::atoi(argv[1]), std::atoi(argv[2]), std::atof(argv[3]));
        like.WriteParams(argv[4]);
        std::printf("logl_true %.17g\n", like(like.MCTrueValues));
        sMCMC::Vector p(like.MCTrueValues);
        for (std::size_t i = 2; i < p.size(); ++i) p[i] = 0.37 * (double)((int)((i * 7) % 11) - 5);     // every parameter at work
        const double logl = like(p);
        std::size_t signal = 0, below = 0;
        for (const auto& e : like.SimulatedSample) {
            signal += e.Type == 0;
            below += e.Type > 0 && e.Mass < 500.0;
        }
        std::printf("logl %.17g\n", logl);
        std::printf("point");
        for (double v : p) std::printf(" %.17g", v);
        std::printf("\ntrue %.17g %.17g dim %zu\n", like.MCTrueValues[0], like.MCTrueValues[1], like.MCTrueValues.size());
        std::printf("simulated %zu signal %zu background_below_500 %zu\n", like.SimulatedSample.size(), signal, below);
        std::printf("integrals %.17g %.17g norms %.17g %.17g\n", like.SignalIntegral, like.BackgroundIntegral, like.SignalNorm,
                    like.BackgroundNorm);
        // operator() left the point's control values in the two shapes
        std::printf("penalties %.17g %.17g shapes %.17g %.17g\n", like.BackgroundPenalty, like.SignalPenalty,
                    like.BackgroundShape.GetPenalty(), like.SignalShape.GetPenalty());
        const double xs[] = {5.0, 22.727272727272727, 100.0, 135.0, 240.0, 249.0, 260.0, 477.27272727272725, 480.0, 600.0};
        std::printf("values_b");
        for (double x : xs) std::printf(" %.17g", like.BackgroundShape.GetValue(x));
        std::printf("\nvalues_s");
        for (double x : xs) std::printf(" %.17g", like.SignalShape.GetValue(x));
        std::printf("\nbins %g %g centre %.17g %.17g value %.17g %.17g kernel %.17g %.17g\n", like.BackgroundShape.GetBinCount(),
                    like.SignalShape.GetBinCount(), like.BackgroundShape.GetBinCenter(3), like.SignalShape.GetBinCenter(12),
                    like.BackgroundShape.GetBinValue(4), like.SignalShape.GetBinValue(0), like.BackgroundShape.GetKernel(2, 5),
                    like.SignalShape.GetKernel(12, 0));
        sMCMC::TFakeGP far("far", 0.0, 500.0, 11);
        far.ExponentialKernel(2.0, 3.0);
        std::printf("exponential %.17g %.17g %.17g\n", far.GetKernel(0, 0), far.GetKernel(0, 1), far.GetKernel(4, 3));
        like.WriteSimulation(like.MCTrueValues, "nominal");
        std::printf("written %zu\n", like.Written.size());
    } catch (const std::exception& e) {
        std::cerr << "fake_shape_host: " << e.what() << std::endl;
        return 2;
    }
    return 0;
}
