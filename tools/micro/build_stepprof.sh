# The profiling build of the headline step kernel (SMCMC_STEP_PROFILE: s_memtime stamps per section of the step loop,
# smcmc_kernels.hip.h): root-simple-mcmc_amd/build/prof/libsmcmc_amd_stepprof<level>.so = the plain library's objects with
# inst_dp50_l0.o replaced.  Level 1 stamps the sections, level 2 every piece as well.  Read by tools/micro/stepprof.py
# and tests/test_gpu_step_profile_build.py on the GPU box.
# usage: bash tools/micro/build_stepprof.sh [levels, default "1 2"]   (after the plain build)
set -e
R=$(cd "$(dirname "$0")/../.." && pwd); B=$R/root-simple-mcmc_amd/build; P=$B/prof
mkdir -p $P
OBJS=$(ls $B/*.o | grep -v -e '_frozen_definition\.o$' -e '_user\.o$' -e '_user_grad\.o$' -e '/user_large' -e '/inst_dp50_l0\.o$' -e '/inst_dp[0-9]*_l3\.o$')
for L in ${1:-1 2}; do
    rm -rf $P/tmp$L; mkdir -p $P/tmp$L
    /opt/rocm/bin/hipcc -std=c++17 -O3 -fPIC -ffp-contract=off --offload-arch=gfx950 -fno-gpu-rdc -Wall -Wno-unused-function \
        -I$R/include -I$R/root-simple-mcmc_amd/csrc -DSMCMC_DP=50 -DSMCMC_LIKE=0 -DSMCMC_STEP_PROFILE=$L \
        -save-temps=obj -c $R/root-simple-mcmc_amd/csrc/smcmc_inst.hip -o $P/tmp$L/inst_dp50_l0_prof$L.o
    # the listing check of the plain build (hand-placed LDS reads must not be touched in flight) holds here too
    python3 $R/tools/check_inflight_regs.py $P/tmp$L/*amdgcn*gfx950*.s > $P/inflight$L.txt || { cat $P/inflight$L.txt; exit 1; }
    mv $P/tmp$L/inst_dp50_l0_prof$L.o $P/ && cp $P/tmp$L/*amdgcn*gfx950*.s $P/stepprof$L.s && rm -r $P/tmp$L
    /opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -fno-gpu-rdc $OBJS $P/inst_dp50_l0_prof$L.o -o $P/libsmcmc_amd_stepprof$L.so
    echo built $P/libsmcmc_amd_stepprof$L.so
done
