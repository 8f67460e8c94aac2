// Host side of pf_linear_ws (no device code): the environment knobs and THE plan of a problem -- whether the kernel can run it, whether
// the linear front ends should send it there, the instantiation (K, channels per workgroup) and the grid split -- that pf_linear_ws
// launches and pf_linear_ws_plan / pf_linear_ws_supported report.  The shape table is the one at pf_linear_ws_desc in
// include/panfusion_hip.h.
#include "pf_linear_ws_plan.h"
#include <algorithm>

namespace pf {

const LwsTuning& lws_tuning() {
    static const LwsTuning t;
    return t;
}

pf_lws_plan plan_linear_ws(long M, int N, int K, int mode, int dtype, int a_ld, int rows_per_batch) {
    const LwsTuning& t = lws_tuning();
    pf_lws_plan g{};
    const bool m16 = mode == PF_LWS_16, geglu = mode == PF_LWS_GEGLU, vt = mode == PF_LWS_VT;
    if (mode < PF_LWS_16 || mode > PF_LWS_VT || N <= 0) return g;
    // ---- can the kernel run it?  (K, mode, N) -> channels per workgroup and the most channel blocks; K -> tokens per tile
    int chb = 0, max_blocks = 32;
    if (K == 320) chb = 320;                                            // every mode
    else if (K == 640) chb = N % 256 == 0 && (m16 || geglu) ? 256 : m16 || vt ? 128 : 0;
    else if (K == 1280 && (m16 || geglu || vt)) { chb = 128; max_blocks = 128; }
    const int tile = K == 320 ? 64 : K == 640 ? 32 : 16;
    if (chb == 0 || N % chb != 0 || N / chb > max_blocks || M < tile) return g;
    if ((mode == PF_LWS_QKV && N != 960) || (mode == PF_LWS_F32_LN && N != 320)) return g;   // q | k | v; a whole row per workgroup
    g.supported = 1;
    g.k = K; g.chb = chb; g.tile_tokens = tile;
    g.nblocks = N / chb;
    g.ntiles = static_cast<int>(cdiv(M, tile));
    g.counted = t.counted;
    // ---- the grid of 256 workgroups: the channel blocks of one token range on one XCD (one L2 fill of the activation tiles) -- unless
    // that leaves too many CUs without a workgroup (20 channel blocks: 160 of 256), then token range b / nblocks, channel block b % nblocks
    const int per_xcd = 32 / g.nblocks;
    if (8 * per_xcd * g.nblocks >= 200) g.splits_per_xcd = per_xcd;
    else g.flat_splits = std::max(1, 256 / g.nblocks);
    // ---- should a linear go here?  The layout the kernel reads, the knobs, enough token tiles to stream (one channel block: 256 token
    // ranges -- under 2 tiles each the tile kernel wins, M = 16384: 0.88 - 0.94 x; q | k | v and FF1 win from 8192 rows,
    // profiles/r4_lws_notes.txt), whole tiles per batch of a transposed output
    const bool layout = (dtype == PF_BF16 || dtype == PF_F16) && a_ld >= K && a_ld % 8 == 0;
    const bool knobs = t.ws && (K != 640 || t.k640) && (K != 1280 || t.k1280) && (!vt || t.vt) && (mode != PF_LWS_F32_LN || t.ln);
    const bool rows = M >= t.min_rows && !(K == 320 && N == 320 && M < 4L * t.min_rows);
    const bool batches = !(vt || mode == PF_LWS_QKV) || rows_per_batch == 0 ||
                         (rows_per_batch > 0 && rows_per_batch % tile == 0 && M % rows_per_batch == 0);
    g.preferred = layout && knobs && rows && batches;
    return g;
}

}  // namespace pf

using namespace pf;

extern "C" pf_status pf_linear_ws_plan(const pf_linear_ws_desc* d, pf_lws_plan* out) {
    PF_REQUIRE(d && out, "pf_linear_ws_plan: null pointer");
    *out = plan_linear_ws(d->M, d->N, d->K, d->mode, d->dtype, d->a_ld, d->rows_per_batch);
    return PF_OK;
}

extern "C" int pf_linear_ws_supported(long M, int N, int K, int mode) {
    return plan_linear_ws(M, N, K, mode, PF_BF16, K, 0).supported;
}
