// Host side of pf_linear_ws (pf_linear_ws_plan.hip): the environment knobs and THE plan of a problem -- what the launch runs and
// pf_linear_ws_plan / pf_linear_ws_supported report.
#pragma once
#include "pf_common.h"
#include <string.h>

namespace pf {

// Every environment knob of pf_linear_ws (A/B switches for benchmarking) with its default, read ONCE per process (lws_tuning()).
// A flag is off for the literal "0" only.
struct LwsTuning {
    static bool flag(const char* name) { const char* e = getenv(name); return !(e && strcmp(e, "0") == 0); }
    bool ws = flag("PF_LINEAR_WS");                          // 0 = no linear prefers this kernel: all of them on the tile kernel (pf_conv_gemm)
    bool k640 = flag("PF_LINEAR_WS_K640");                   // 0 = the K = 640 layers (32^2 level: FF1, q | k, to_q, V^T) stay on the tile kernel
    bool k1280 = flag("PF_LINEAR_WS_K1280");                 // 0 = the K = 1280 layers (16^2 level) stay on the tile kernel
    bool vt = flag("PF_LINEAR_VT");                          // 0 = V^T projections (PF_LWS_VT) by the operand-swapped tile GEMM
    bool ln = flag("PF_LINEAR_LN");                          // 0 = no LayerNorm epilogue (PF_LWS_F32_LN): projection and LayerNorm as two launches
    int min_rows = env_int("PF_LINEAR_WS_MIN_ROWS", 8192);   // fewer rows: fewer token tiles than workgroups, the tile kernel wins (N = 320: 4 x as many)
    bool counted = env_int("PF_LWS_COUNTED", 1) != 0;        // 0 = k_linear_ws drains vmcnt(0) per tile instead of the counted wait
};
const LwsTuning& lws_tuning();

// THE plan of a problem, from the scalar members of pf_linear_ws_desc alone (rows_per_batch 0: not stated, not checked).
pf_lws_plan plan_linear_ws(long M, int N, int K, int mode, int dtype, int a_ld, int rows_per_batch);

}  // namespace pf
