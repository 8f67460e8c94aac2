// Host side of the attention front ends (pf_attention_plan.hip): the environment knobs, the descriptor checks that pf_attention and
// pf_attention_wide share, and THE plan of a pf_attention problem -- what the launch runs and pf_attention_plan / _workspace_size report;
// below them the same three things for pf_attention_bwd.
#pragma once
#include "pf_common.h"

namespace pf {

// Every environment knob of pf_attention (A/B switches for benchmarking) with its default.  The members are read ONCE per process
// (attn_tuning()); the two that tests switch inside a process are the static accessors below them, read on every call.
struct AttnTuning {
    bool lds = !(getenv("PF_ATTENTION_IMPL") && getenv("PF_ATTENTION_IMPL")[0] == 'd');   // PF_ATTENTION_IMPL=direct: the no-LDS kernel everywhere
    int occ64 = env_int("PF_ATTENTION_OCC", 3);              // D = 64: 3 = one score array, three waves per SIMD; 2 = register-pipelined scores, two waves
    int occ32 = env_int("PF_ATTENTION_OCC32", 4);            // D = 32: 4 | 5 = not pipelined at that occupancy; anything else = register-pipelined, three waves
    int msum = env_int("PF_ATTENTION_MSUM", 1);              // D = 64: softmax row sums as ones-operand MFMAs (nk >= 256, no lse); 0 = on the vector ALU
    int msum32 = env_int("PF_ATTENTION_MSUM32", 0);          // the same for the biased D = 32 kernel in its pipelined form: 168 registers + 3 spilled
    int split_min_tiles = env_int("PF_ATTENTION_SPLIT_MIN_TILES", 8);   // least 64-key tiles per split of the key range
    int pp_role = env_int("PF_ATTENTION_PP_ROLE", 3);        // k_attention_pp: how a wave finds its phase group (AttnParams.pp_role)
    int pp_prio = env_int("PF_ATTENTION_PP_PRIO", 2);        // k_attention_pp: wave priorities (AttnParams.pp_prio)
    int xcd = env_int("PF_ATTENTION_XCD", 1);                // k_attention_lds: 1 = heads pinned to XCDs, 0 = plain block order
    int steady2 = env_int("PF_ATTENTION_STEADY2", 1);        // k_attention_lds, not pipelined: 1 = branch-free two-tile steady-state loop
    // read on every call:
    static int pingpong() { return env_int("PF_ATTENTION_PP", 0); }   // 1 | 2 = the 8-wave ping-pong kernels for the unbiased D = 64 launches (one | two key tiles per phase)
    static int split() { return env_int("PF_ATTENTION_SPLIT", 1); }   // 0 = never split the key range
};
const AttnTuning& attn_tuning();

// How pf_attention.hip -- the kernels -- was built (defined there): the planner follows the kernels it is linked with.
extern const bool attn_build_bufload;      // PF_ATTN_BUFLOAD: k_attention_lds addresses K / V^T tiles with 32-bit byte offsets
extern const bool attn_build_pp_timing;    // PF_ATTN_PP_TIMING: k_attention_pp writes its clock stamps over lse

// The layout rules of pf_attn_desc that both entry points share (include/panfusion_hip.h); `who` names the entry point in the messages.
pf_status validate_attn_desc(const pf_attn_desc* d, const char* who);
// THE plan of a problem.  allow_split: the key-range split's scratch is at hand.
pf_attn_plan plan_attention(const pf_attn_desc* d, bool allow_split);
// ... of THIS launch: split only with the scratch the split plan asks for (pf_attn_desc.workspace: present, large enough, 16-byte aligned).
pf_attn_plan plan_attention_launch(const pf_attn_desc* d);
// Can the grid of plan g be launched?  Each dimension within HIP's limits; 1-D grids: workgroups x threads under 2^32.
bool attn_grid_launchable(const pf_attn_desc* d, const pf_attn_plan& g);

// descriptor -> the operand members the kernel parameter structs have in common (AttnParams, WideParams)
template <typename P> void attn_operands(const pf_attn_desc* d, P& p) {
    p.q = static_cast<const unsigned short*>(d->q); p.k = static_cast<const unsigned short*>(d->k);
    p.vt = static_cast<const unsigned short*>(d->vt); p.out = static_cast<unsigned short*>(d->out);
    p.H = d->H; p.nq = d->nq; p.nk = d->nk;
    p.q_ld = d->q_ld; p.k_ld = d->k_ld; p.vt_ld = d->vt_ld; p.o_ld = d->o_ld;
    p.q_bs = d->q_bs; p.k_bs = d->k_bs; p.vt_bs = d->vt_bs; p.o_bs = d->o_bs;
    p.scale_log2e = d->scale * 1.44269504088896340736f;
}

// ---- pf_attention_bwd (kernels in pf_backward.hip) ----------------------------------------------------------------------------------
// Its two environment knobs, read ONCE per process (attn_bwd_tuning()).
struct AttnBwdTuning {
    bool lds = !(getenv("PF_ATTN_BWD_IMPL") && getenv("PF_ATTN_BWD_IMPL")[0] == 'd');   // PF_ATTN_BWD_IMPL=direct: the no-LDS kernels everywhere
    int qsplit = env_int("PF_ATTN_BWD_QSPLIT", 1);           // 0 = never split the query range of the keys-stationary launch
};
const AttnBwdTuning& attn_bwd_tuning();

// The rules of pf_attn_bwd_desc (include/panfusion_hip.h); `who` names the entry point in the messages.
pf_status validate_attn_bwd_desc(const pf_attn_bwd_desc* d, const char* who);
// THE plan of a problem.  allow_split: the query split's scratch is at hand.
pf_attn_bwd_plan plan_attention_bwd(const pf_attn_bwd_desc* d, bool allow_split);
// Can the three grids of plan g be launched?  y and z within 65535, workgroups x threads in x under 2^32.
bool attn_bwd_grids_launchable(const pf_attn_bwd_plan& g);

// descriptor -> the operand members of the kernel parameter struct (AttnBwdParams)
template <typename P> void attn_bwd_operands(const pf_attn_bwd_desc* d, P& p) {
    auto in = [](const void* v) { return static_cast<const unsigned short*>(v); };
    auto out = [](void* v) { return static_cast<unsigned short*>(v); };
    p.q = in(d->q); p.k = in(d->k); p.v = in(d->v); p.dout = in(d->dout); p.qt = in(d->qt); p.kt = in(d->kt); p.dot = in(d->dot);
    p.dq = out(d->dq); p.dk = out(d->dk); p.dv = out(d->dv);
    p.H = d->H; p.nq = d->nq; p.nk = d->nk;
    p.q_ld = d->q_ld; p.k_ld = d->k_ld; p.v_ld = d->v_ld; p.do_ld = d->do_ld; p.qt_ld = d->qt_ld; p.kt_ld = d->kt_ld; p.dot_ld = d->dot_ld;
    p.dq_ld = d->dq_ld; p.dk_ld = d->dk_ld; p.dv_ld = d->dv_ld;
    p.q_bs = d->q_bs; p.k_bs = d->k_bs; p.v_bs = d->v_bs; p.do_bs = d->do_bs; p.qt_bs = d->qt_bs; p.kt_bs = d->kt_bs; p.dot_bs = d->dot_bs;
    p.dq_bs = d->dq_bs; p.dk_bs = d->dk_bs; p.dv_bs = d->dv_bs;
    p.scale = d->scale; p.scale_log2e = d->scale * 1.44269504088896340736f;
    p.bias = d->bias; p.bias_ld = d->bias_ld; p.flags = d->flags; p.flags_ld = d->flags_ld;
    p.lse = d->lse; p.delta = d->delta;
}

}  // namespace pf
