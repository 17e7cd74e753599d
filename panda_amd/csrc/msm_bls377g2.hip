// msm_bls377g2.hip -- the MSM kernels and driver of msm_impl.h instantiated for BLS12-377 G2 (coordinates in Fq2 = Fq[u] / (u^2 + 5)
// over the 14-limb field, fe29_ext2.h; k_accumulate in its one shipped shape, one wave per SIMD: AccWaves / AccSingleShape).
#define PANDA_MSM_IMPL
#include "msm_impl.h"

namespace panda {

hipError_t msm_execute_bls377_g2(const panda_msm_configuration &cfg, const MsmRegistration *reg, MsmTuning tuning, float *phase_ms, bool *stale,
                                 const MsmPipeline *pipe)
{
    return msm_execute<CurveBls377G2>(cfg, reg, tuning, phase_ms, stale, pipe);
}

hipError_t msm_execute_batch_bls377_g2(const panda_msm_configuration &cfg, const MsmRegistration *reg, unsigned batch, unsigned group_log_max, unsigned timing,
                                       float *phase_ms, bool *stale)
{
    return msm_execute_batch<CurveBls377G2>(cfg, reg, batch, group_log_max, timing, phase_ms, stale);
}

hipError_t msm_build_registration_bls377_g2(MsmRegistration &r, hipStream_t s) { return build_registration<Ext2<Bls377Fq>>(r, s); }

} // namespace panda
