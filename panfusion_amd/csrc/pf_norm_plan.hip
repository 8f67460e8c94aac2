// Host side of the GroupNorm / LayerNorm launches (no device code): the environment knob, the shape rules of every entry point and THE
// plan of a problem -- arm, chunking, staging layout, grids and workspace -- that pf_elementwise.hip and pf_backward.hip launch and that
// pf_groupnorm_plan, pf_groupnorm_bwd_plan, pf_layernorm_plan and the four size queries report.
#include "pf_norm_plan.h"
#include <algorithm>

namespace pf {

const NormTuning& norm_tuning() {
    static const NormTuning t;
    return t;
}

// The staging layout of k_gn_partial, k_gn_bwd_partial and k_gn_param_partial: the C / 8 octets of a pixel side by side over the 256
// threads (two rounds from 257 octets), pix_par pixels in parallel, `arrays` fp32 [pix_par][C] of dynamic LDS (at most 64 KiB).
static int gn_pix_par(int C) { return 256 / std::min(C / 8, 256); }
static size_t gn_lds_bytes(int arrays, int C) { return static_cast<size_t>(arrays) * gn_pix_par(C) * C * sizeof(float); }
constexpr size_t GN_LDS_MAX = 64 * 1024;

// ---- the sizes the plans and the size queries share (plain arithmetic: no rule, no message) -------------------------------------------
// statistics: pixels per chunk -- ~2048 blocks in flight, 8..64 pixels each, at most 256 chunks per image -- and the chunk partials
static long gn_stats_ppc(int n_img, int hw) {
    return std::min<long>(hw, std::max(cdiv(hw, 256), std::clamp(static_cast<long>(n_img) * hw / 2048, 8L, 64L)));
}
static size_t gn_stats_workspace(int n_img, int hw) {
    return static_cast<size_t>(n_img) * cdiv(hw, gn_stats_ppc(n_img, hw)) * 64 * 2 * sizeof(float);      // up to 64 groups
}
// backward: at least 16 chunks per image, down to 8 pixels each
static int gn_bwd_ppc(int hw) {
    int ppc = 64;
    while (ppc > 8 && cdiv(hw, ppc) < 16) ppc >>= 1;
    return ppc;
}
static long gn_bwd_rows(int n_img, int hw) { return static_cast<long>(n_img) * cdiv(hw, gn_bwd_ppc(hw)); }      // chunks of all images
static size_t gn_bwd_workspace(int n_img, int hw, int groups) {                                                   // chunk partials + statistics
    return (static_cast<size_t>(gn_bwd_rows(n_img, hw)) * groups * 4 + static_cast<size_t>(n_img) * groups * 4) * sizeof(float);
}
static size_t gn_param_partial_bytes(int n_img, int hw, int C) { return static_cast<size_t>(gn_bwd_rows(n_img, hw)) * 2 * C * sizeof(float); }
static size_t gn_param_workspace(int n_img, int hw, int C) {                                                      // ... + pf_colsum's slabs
    return gn_param_partial_bytes(n_img, hw, C) + pf_colsum_workspace_size(gn_bwd_rows(n_img, hw), 2 * C);
}
constexpr int LN_BWD_MAX_PARTS = 512;
static int ln_bwd_parts(long rows) { return static_cast<int>(std::max(1L, std::min<long>(LN_BWD_MAX_PARTS, cdiv(rows, 4)))); }

// ---- GroupNorm statistics ------------------------------------------------------------------------------------------------------
// The rules of pf_groupnorm_from_partials in their order: 0 = the moments serve (then *gpb = groups per block), else the rule that fails.
static int partials_fault(int n_img, int hw, int c0, int rows0, int c1, int rows1, int groups, int* gpb) {
    const int C = c0 + c1;
    if (!(n_img > 0 && hw > 0 && groups > 0 && groups <= 64 && C % groups == 0 && c0 > 0)) return 1;
    if (!(rows0 > 0 && rows1 > 0 && hw % rows0 == 0 && hw % rows1 == 0)) return 2;
    if (!((C / groups) % 2 == 0 && c0 % 2 == 0 && c1 % 2 == 0)) return 3;
    const int ppi = std::max(hw / rows0, hw / rows1), ppg = C / groups / 2;       // parts per image; pairs per group
    *gpb = ppi <= 32 ? GN_GPB : ppi <= 128 ? 4 : ppi <= 512 ? 2 : 1;             // fewer groups per block = more slices walking the parts
    while (*gpb > 1 && *gpb * ppg > 512) *gpb >>= 1;
    return *gpb * ppg <= 512 ? 0 : 4;
}

pf_status plan_groupnorm_partials(int n_img, int hw, int c0, int rows0, int c1, int rows1, int groups, pf_gn_plan* out) {
    *out = pf_gn_plan{};
    const int C = c0 + c1;
    int gpb = 0;
    const int fault = partials_fault(n_img, hw, c0, rows0, c1, rows1, groups, &gpb);
    PF_REQUIRE(fault != 1, "pf_groupnorm_from_partials: bad sizes");
    PF_REQUIRE(fault != 2, "pf_groupnorm_from_partials: an image (%d rows) must be whole runs of %d / %d rows", hw, rows0, rows1);
    PF_REQUIRE(fault != 3, "pf_groupnorm_from_partials: groups and sources must hold even numbers of channels (moments are per column pair)");
    PF_REQUIRE(fault != 4, "pf_groupnorm_from_partials: C=%d too large for %d groups", C, groups);
    out->arm = PF_GN_FROM_PARTIALS;
    out->gpb = gpb;
    out->pairs_per_block = std::min(gpb * (C / groups / 2), C / 2);
    out->slices = out->pairs_per_block <= 128 ? 256 / out->pairs_per_block : 1;
    out->grid_x = n_img;
    out->grid_y = static_cast<unsigned>(cdiv(groups, gpb));
    return PF_OK;
}

pf_status plan_groupnorm(int n_img, int hw, int c0, int c1, int groups, int dtype, int rows0, int rows1, pf_gn_plan* out) {
    const bool offered = rows0 > 0 && (c1 == 0 || rows1 > 0);
    int gpb;
    if (offered && partials_fault(n_img, hw, c0, rows0, c1, c1 ? rows1 : rows0, groups, &gpb) == 0)
        return plan_groupnorm_partials(n_img, hw, c0, rows0, c1, c1 ? rows1 : rows0, groups, out);
    *out = pf_gn_plan{};
    const int C = c0 + c1;
    PF_REQUIRE(n_img > 0 && hw > 0 && groups > 0 && groups <= 64, "pf_groupnorm_stats: bad sizes");
    PF_REQUIRE(C % 8 == 0 && c0 % 8 == 0 && C % groups == 0, "pf_groupnorm_stats: C=%d must be a multiple of 8 and of groups=%d", C, groups);
    PF_REQUIRE(dtype != PF_F32 || (c0 % 4 == 0 && c1 % 4 == 0), "pf_groupnorm_stats: fp32 sources need c0, c1 %% 4 == 0");
    PF_REQUIRE(dtype == PF_BF16 || dtype == PF_F16 || dtype == PF_F32, "pf_groupnorm_stats: dtype must be PF_BF16, PF_F16 or PF_F32");
    pf_gn_plan g{};
    g.partials_refused = offered;
    g.workspace_bytes = gn_stats_workspace(n_img, hw);                       // asked of either arm
    if (static_cast<long>(hw) * (C / groups) <= norm_tuning().gn_direct_max && static_cast<long>(n_img) * hw * C <= (4L << 20)) {
        g.arm = PF_GN_DIRECT;
        g.grid_x = n_img;
        g.grid_y = groups;
    } else {
        PF_REQUIRE(gn_lds_bytes(2, C) <= GN_LDS_MAX, "pf_groupnorm_stats: C=%d too large", C);
        g.arm = PF_GN_TWO_STAGE;
        g.ppc = static_cast<int>(gn_stats_ppc(n_img, hw));
        g.nchunks = static_cast<int>(cdiv(hw, g.ppc));
        g.pix_par = gn_pix_par(C);
        g.lds_bytes = static_cast<unsigned>(gn_lds_bytes(2, C));
        g.grid_x = g.nchunks;
        g.grid_y = n_img;
        g.grid2_x = n_img;
        g.grid2_y = static_cast<unsigned>(cdiv(groups, GN_GPB));
    }
    *out = g;
    return PF_OK;
}

// ---- GroupNorm backward --------------------------------------------------------------------------------------------------------
// what both entry points share: the chunks, the staging layout and the partial kernels' grid, and the parameter gradients' sizes
static pf_gn_bwd_plan gn_bwd_common(int n_img, int hw, int C) {
    pf_gn_bwd_plan g{};
    g.ppc = gn_bwd_ppc(hw);
    g.chunks = static_cast<int>(cdiv(hw, g.ppc));
    g.pix_par = gn_pix_par(C);
    g.partial_grid_x = g.chunks;
    g.partial_grid_y = n_img;
    g.param_lds_bytes = static_cast<unsigned>(gn_lds_bytes(2, C));
    g.param_partial_bytes = gn_param_partial_bytes(n_img, hw, C);
    g.param_workspace_bytes = gn_param_workspace(n_img, hw, C);
    return g;
}

pf_status plan_groupnorm_bwd(int n_img, int hw, int c0, int c1, int groups, pf_gn_bwd_plan* out) {
    *out = pf_gn_bwd_plan{};
    const int C = c0 + c1;
    PF_REQUIRE(n_img > 0 && hw > 0, "pf_groupnorm_bwd: bad arguments");
    PF_REQUIRE(c0 > 0 && c0 % 8 == 0 && c1 % 8 == 0 && groups > 0 && C % groups == 0, "pf_groupnorm_bwd: channels (%d,%d) must be multiples of 8 and divide into %d groups", c0, c1, groups);
    PF_REQUIRE(n_img <= 65535, "pf_groupnorm_bwd: at most 65535 images per call");
    PF_REQUIRE(gn_lds_bytes(4, C) <= GN_LDS_MAX, "pf_groupnorm_bwd: %d channels exceed the 64 KiB staging buffer", C);
    *out = gn_bwd_common(n_img, hw, C);
    out->bwd_lds_bytes = static_cast<unsigned>(gn_lds_bytes(4, C));
    out->finalize_grid_x = n_img;
    out->apply_grid_x = static_cast<unsigned>(cdiv(static_cast<long>(hw) * (C / 8), 256));
    out->apply_grid_y = n_img;
    out->bwd_workspace_bytes = gn_bwd_workspace(n_img, hw, groups);
    return PF_OK;
}

pf_status plan_groupnorm_param_grads(int n_img, int hw, int c0, int c1, pf_gn_bwd_plan* out) {
    *out = pf_gn_bwd_plan{};
    const int C = c0 + c1;
    PF_REQUIRE(n_img > 0 && hw > 0, "pf_groupnorm_param_grads: bad arguments");
    PF_REQUIRE(c0 > 0 && c0 % 8 == 0 && c1 % 8 == 0, "pf_groupnorm_param_grads: channels (%d,%d) must be multiples of 8", c0, c1);
    PF_REQUIRE(n_img <= 65535, "pf_groupnorm_param_grads: at most 65535 images per call");
    PF_REQUIRE(gn_lds_bytes(2, C) <= GN_LDS_MAX, "pf_groupnorm_param_grads: %d channels exceed the 64 KiB staging buffer", C);
    *out = gn_bwd_common(n_img, hw, C);
    return PF_OK;
}

// ---- LayerNorm -----------------------------------------------------------------------------------------------------------------
static pf_ln_plan ln_plan(long rows, int C) {
    pf_ln_plan g{};
    g.rows_per_wave = C <= 512 && rows >= 4096 ? 4 : 1;               // narrow rows: 4 rows per wavefront in flight
    g.grid_x = static_cast<unsigned>(cdiv(rows, 4 * g.rows_per_wave));
    g.bwd_parts = ln_bwd_parts(rows);
    return g;
}

pf_status plan_layernorm(long rows, int C, pf_ln_plan* out) {
    *out = pf_ln_plan{};
    PF_REQUIRE(rows > 0, "pf_layernorm: bad arguments");
    PF_REQUIRE(C % 8 == 0 && C <= 2048, "pf_layernorm: C=%d must be a multiple of 8 and <= 2048", C);
    *out = ln_plan(rows, C);
    return PF_OK;
}

pf_status plan_layernorm_bwd(long rows, int C, pf_ln_plan* out) {
    *out = pf_ln_plan{};
    PF_REQUIRE(rows > 0, "pf_layernorm_bwd: bad arguments");
    PF_REQUIRE(C > 0 && C % 8 == 0 && C <= 2048, "pf_layernorm_bwd: C=%d must be a multiple of 8, at most 2048", C);
    *out = ln_plan(rows, C);
    return PF_OK;
}

}  // namespace pf

using namespace pf;

extern "C" pf_status pf_groupnorm_plan(int n_img, int hw, int c0, int c1, int groups, int dtype, int rows0, int rows1, pf_gn_plan* out) {
    PF_REQUIRE(out, "pf_groupnorm_plan: null pointer");
    return plan_groupnorm(n_img, hw, c0, c1, groups, dtype, rows0, rows1, out);
}

extern "C" pf_status pf_groupnorm_bwd_plan(int n_img, int hw, int c0, int c1, int groups, pf_gn_bwd_plan* out) {
    PF_REQUIRE(out, "pf_groupnorm_bwd_plan: null pointer");
    return groups == 0 ? plan_groupnorm_param_grads(n_img, hw, c0, c1, out) : plan_groupnorm_bwd(n_img, hw, c0, c1, groups, out);
}

extern "C" pf_status pf_layernorm_plan(long rows, int C, pf_ln_plan* out) {
    PF_REQUIRE(out, "pf_layernorm_plan: null pointer");
    const pf_status fwd = plan_layernorm(rows, C, out);                 // what both directions accept
    return fwd != PF_OK ? fwd : plan_layernorm_bwd(rows, C, out);
}

// ---- the size queries: the plans' own sizes for the arguments a query has.  They know no shape rule and write no message, as before the
// planner: a size is stated for every problem with positive arguments, accepted by its launch or not.
extern "C" size_t pf_groupnorm_workspace_size(int n_img, int hw, int C) {
    (void)C;
    return n_img > 0 && hw > 0 ? gn_stats_workspace(n_img, hw) : 0;
}

extern "C" size_t pf_groupnorm_bwd_workspace_size(int n_img, int hw, int groups) {
    return n_img > 0 && hw > 0 && groups > 0 ? gn_bwd_workspace(n_img, hw, groups) : 0;
}

extern "C" size_t pf_groupnorm_param_grads_workspace_size(int n_img, int hw, int C) {
    return n_img > 0 && hw > 0 && C > 0 ? gn_param_workspace(n_img, hw, C) : 0;
}

extern "C" int pf_layernorm_bwd_parts(long rows) { return ln_bwd_parts(rows); }
