// Host side of the GroupNorm / LayerNorm launches (pf_norm_plan.hip): the environment knob, the constant planner and kernels share,
// and THE plan of a problem -- what pf_groupnorm_stats / _from_partials, pf_groupnorm_bwd / _param_grads and pf_layernorm / _bwd launch
// and what pf_groupnorm_plan, pf_groupnorm_bwd_plan, pf_layernorm_plan and the four size queries report.
#pragma once
#include "pf_common.h"

namespace pf {

// The environment knob of the family with its default, read ONCE per process (norm_tuning()).
struct NormTuning {
    long gn_direct_max = getenv("PF_GN_DIRECT_MAX") ? atol(getenv("PF_GN_DIRECT_MAX")) : 32768;   // direct arm: elements per (image, group); 0 = off (A/B)
};
const NormTuning& norm_tuning();

constexpr int GN_GPB = 8;      // groups per block of k_gn_finalize, and the most of k_gn_finalize_cols

// Each planner applies the shape rules of its entry point first: a refused problem has PF_ERR_ARG, that entry point's message and an
// all-zero plan.  No plan reads a pointer.
// rows0 / rows1: rows per part of the moments attached to the sources (0: none).  Moments on every source that can serve: the plan of
// pf_groupnorm_from_partials; that cannot: the plan of the statistics pass, partials_refused = 1.
pf_status plan_groupnorm(int n_img, int hw, int c0, int c1, int groups, int dtype, int rows0, int rows1, pf_gn_plan* out);
// pf_groupnorm_from_partials itself: refused with ITS message where plan_groupnorm falls back to the statistics pass (one source: c1 = 0, rows1 = rows0)
pf_status plan_groupnorm_partials(int n_img, int hw, int c0, int rows0, int c1, int rows1, int groups, pf_gn_plan* out);
// pf_groupnorm_bwd (with the pf_groupnorm_param_grads of the same tensor), and pf_groupnorm_param_grads alone by its own rules: it knows no
// groups and has half the LDS to fit, the members of pf_groupnorm_bwd are 0
pf_status plan_groupnorm_bwd(int n_img, int hw, int c0, int c1, int groups, pf_gn_bwd_plan* out);
pf_status plan_groupnorm_param_grads(int n_img, int hw, int c0, int c1, pf_gn_bwd_plan* out);
// one plan, by the rules of pf_layernorm or of pf_layernorm_bwd
pf_status plan_layernorm(long rows, int C, pf_ln_plan* out);
pf_status plan_layernorm_bwd(long rows, int C, pf_ln_plan* out);

}  // namespace pf
