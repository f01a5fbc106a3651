// fake_template_host.C -- sMCMC::FakeTemplateLikelihood (include/FakeTemplateLikelihood_amd.H) through its host path
// alone, for tests/test_cpp_fake_template.py: Init(), DeviceParams() written to argv[4], operator() at MCTrueValues.
//   ./fake_template_host.exe dataSignal dataBackground mcOversample params.txt
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "FakeTemplateLikelihood_amd.H"

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    try {
        sMCMC::FakeTemplateLikelihood like;
        like.Init(std::atoi(argv[1]), std::atoi(argv[2]), std::atof(argv[3]));
        like.WriteParams(argv[4]);
        const double logl = like(like.MCTrueValues);
        std::size_t signal = 0, below = 0;
        for (const auto& e : like.SimulatedSample) {
            signal += e.Type == 0;
            below += e.Type > 0 && e.Mass < 500.0;
        }
        std::printf("logl %.17g\n", logl);
        std::printf("true %.17g %.17g dim %zu\n", like.MCTrueValues[0], like.MCTrueValues[1], like.MCTrueValues.size());
        std::printf("simulated %zu signal %zu background_below_500 %zu\n", like.SimulatedSample.size(), signal, below);
        std::printf("integrals %.17g %.17g norms %.17g %.17g\n", like.SignalIntegral, like.BackgroundIntegral, like.SignalNorm,
                    like.BackgroundNorm);
        std::printf("expectation %.17g\n", sMCMC::FakeTemplateLikelihood::Integral(like.SimulatedClose) +
                                               sMCMC::FakeTemplateLikelihood::Integral(like.SimulatedSeparated) +
                                               sMCMC::FakeTemplateLikelihood::Integral(like.SimulatedDecayTag));
        like.WriteSimulation(like.MCTrueValues, "nominal");
        std::printf("written %zu\n", like.Written.size());
    } catch (const std::exception& e) {
        std::cerr << "fake_template_host: " << e.what() << std::endl;
        return 2;
    }
    return 0;
}
