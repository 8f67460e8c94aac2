// Host side of pf_conv_gemm's planning (no device code): the environment knobs, descriptor -> kernel parameters, and THE plan of a
// problem -- which tile kernel, tile shape, split-K / tail-split layout, GroupNorm-moment rows, scratch -- that pf_conv_gemm launches
// and pf_conv_gemm_plan / _workspace_size / _gn_rows / _kernel_id report.
#include "pf_gemm_params.h"

namespace pf {

const GemmTuning& gemm_tuning() {
    static const GemmTuning t;
    return t;
}

void params_from_desc(const pf_conv_desc* d, GemmParams& p) {
    const int c1 = d->a1 ? d->c1 : 0;
    const int Ctot = d->c0 + c1;
    p.a0 = static_cast<const unsigned short*>(d->a0);
    p.a1 = static_cast<const unsigned short*>(d->a1);
    p.c0 = d->c0; p.c1 = c1; p.a0_ld = d->a0_ld; p.a1_ld = d->a1 ? d->a1_ld : 0;
    p.h_in = d->h_in; p.w_in = d->w_in; p.h_out = d->h_out; p.w_out = d->w_out;
    p.ksize = d->ksize; p.stride = d->stride; p.pad = d->pad; p.up = d->upsample;
    p.wrap = d->wrap_pad; p.crop = d->crop;
    p.w = static_cast<const unsigned short*>(d->w);
    p.rows_per_img = d->h_out * d->w_out;
    p.M = d->n_img * p.rows_per_img; p.N = d->n_out; p.K = d->ksize * d->ksize * Ctot;
    p.bias = d->bias; p.rowvec = d->rowvec; p.rowvec_ld = d->rowvec_ld;
    p.residual = d->residual; p.res_ld = d->res_ld;
    p.res_f32 = d->residual != nullptr && d->res_dtype == PF_F32;
    p.out = d->out; p.out_ld = d->out_ld; p.out_f32 = d->out_dtype == PF_F32;
    p.geglu = d->epilogue == PF_EPILOGUE_GEGLU;
    p.split_out = d->epilogue == PF_EPILOGUE_SPLIT;
    p.a_bs = d->a_bstride; p.w_bs = d->w_bstride; p.out_bs = d->out_bstride; p.res_bs = d->res_bstride;
    p.mtiles = p.ntiles = 0;
    p.prof = nullptr;
    p.s3 = d->split3 != 0;
    p.batch = d->batch;
    p.gn_partial = nullptr; p.gn_rows = 0;
    p.m_begin = 0; p.splits = 1; p.kb_per_split = 0; p.partial = nullptr; p.tickets = nullptr;
    p.a0_bytes = p.a1_bytes = p.w_bytes = 0; p.adv_img = p.adv_y = p.adv_x = 0;
    p.a32 = d->a_src_dtype == PF_F32;
    p.a_scale = p.a32 ? d->a_scale : nullptr; p.a_shift = p.a32 ? d->a_shift : nullptr;
    if (p.a32) { p.c0 = 2 * d->c0; p.c1 = 2 * c1; p.K = 2 * Ctot; }     // pair elements: the problem the planner sees IS the pair form's
    p.subpix = 0;
    p.fastseg = (d->upsample == 0 || d->subpixel) && d->wrap_pad == 0 && GemmTuning::conv_fastseg() ? 1 : 0;
    if (d->subpixel) {
        // nearest x2 + 3x3 conv == four 2x2 convolutions on the low-resolution grid, one per output phase (blockIdx.z): 4 Cin
        // instead of 9 Cin MACs per output value.  Everything below is the LOW-resolution problem; out_row() scatters the rows.
        p.subpix = 1; p.ksize = 2; p.up = 0; p.pad = 0;
        p.h_out = d->h_out / 2; p.w_out = d->w_out / 2;
        p.rows_per_img = p.h_out * p.w_out;
        p.M = d->n_img * p.rows_per_img; p.K = 4 * Ctot;
        p.crop = d->crop / 2;
        p.batch = 4; p.a_bs = 0; p.out_bs = 0; p.res_bs = 0; p.w_bs = static_cast<long>(p.N) * p.K;
    }
}

// ---- the 16x16x32 kernels: tile shape and split-K layout (kernel, mrep, nrep, block_rows, splits, kb_per_split, m_split, tail_*) ----

static pf_conv_plan plan_small(long M, int N, int K, int batch, bool allow_split, bool s3) {
    const GemmTuning& t = gemm_tuning();
    pf_conv_plan g{};
    g.kernel = 0;
    // 160-wide N tiles when they divide N exactly (all UNet widths are multiples of 160), 128-wide
    // otherwise; 64-row M tiles when 128-row tiles would not fill the 256 CUs (2 blocks per CU).
    g.nrep = (N % 160 == 0) ? 5 : 4;
    const long ntiles = cdiv(N, 32 * g.nrep);
    const long tiles128 = cdiv(M, 128) * ntiles * batch;
    g.mrep = tiles128 < 512 ? 2 : 4;
    g.block_rows = 32 * g.mrep;
    const long tiles = cdiv(M, 32 * g.mrep) * ntiles * batch;
    const int nkb = K / 64;
    g.splits = 1;
    g.kb_per_split = nkb;
    // split-K when the grid cannot fill the chip and K is long: aim at ~640 blocks, >= 6 K-blocks each
    // Round 6: a grid of <= 256 blocks runs the four-slot ring, one block per CU (plan_conv_gemm): there the split aims at ONE round of the
    // chip (fewer fp32 slabs for the reduce kernel: 128 tiles x 2 K slices instead of x 5) and a K slice may be as short as 4 steps.
    if (t.deep_ring && !s3 && tiles <= 256) {                        // (the split-precision kernels keep the two-slot ring and its plan)
        long s = allow_split && N % 4 == 0 && nkb >= t.split_min_kb ? 256 / tiles : 1;
        if (s > nkb / 4) s = nkb / 4;
        if (s > 32) s = 32;
        if (s > 1) {
            g.kb_per_split = static_cast<int>(cdiv(nkb, s));
            g.splits = static_cast<int>(cdiv(nkb, g.kb_per_split));
        }
        return g;
    }
    if (allow_split && N % 4 == 0 && tiles <= 320 && nkb >= t.split_min_kb) {
        long s = (640 + tiles - 1) / tiles;
        if (s > nkb / 6) s = nkb / 6;
        if (s > 32) s = 32;
        if (s > 1) {
            g.kb_per_split = static_cast<int>(cdiv(nkb, s));
            g.splits = static_cast<int>(cdiv(nkb, g.kb_per_split));
        }
    }
    return g;
}

static pf_conv_plan plan_big(int nrep, int K) {                    // the 8-wave kernel, unsplit, 256-row blocks
    pf_conv_plan g{};
    g.kernel = 1; g.mrep = 8; g.nrep = nrep; g.block_rows = 256; g.splits = 1; g.kb_per_split = K / 64;
    return g;
}

static pf_conv_plan plan_tiles(long M, int N, int K, int batch, bool allow_split, bool s3) {
    const GemmTuning& t = gemm_tuning();
    const int nrep = (N % 160 == 0) ? 5 : 4;
    const long tiles256 = cdiv(M, 256) * cdiv(N, 32 * nrep) * batch;
    // one 8-wave block per CU: take it only when the tiles fill their rounds of 256 CUs to >= 60 % overall (320
    // tiles would idle for 37 % of the launch; the 4-wave kernel's 2 blocks per CU degrade more gracefully).
    // The threshold was flat at the single-GPU sizes in round 2 (17.4-17.5 steps/s from 50 to 95 %) and was set to 60 on the smaller
    // per-rank GEMMs of 2 / 4 / 8 ranks (tools/sim_rank.py: 37.1 -> 33.9 ms per step at 2 ranks from 88 to 60 %).  Round 6, last sweep
    // on the final kernels (profiles/r6n_ab_plan_knobs.txt): 30-50 read -0.2 ... -0.5 ms per step on three boxes, cfg 4 -0.9 ms, the
    // simulated ranks unchanged (half-filled rounds of the panorama's 64 x 128 level and of the 8 x 8 level now take the persistent kernel): 30.
    const long rounds = cdiv(tiles256, 256);
    const bool filled = tiles256 * 100 >= rounds * 256 * t.big_fill_pct;
    // Tail split: whole rounds of 256 tiles run unsplit; the tile rows left over (a badly filled last round)
    // become a second launch whose K range is split so that it fills the chip once more.  320 tiles then
    // cost 1.25 rounds instead of 2.
    pf_conv_plan tail = plan_big(nrep, K);
    bool tail_ok = false;
    if (t.big_min_tiles > 0 && t.tail_split && allow_split && batch == 1 && N % 4 == 0 && tiles256 > 256 && K >= t.big_min_k &&
        K / 64 >= t.tail_min_kb) {
        const long ntl = cdiv(N, 32 * nrep), mt = cdiv(M, 256);
        const long rows1 = (tiles256 / 256) * 256 / ntl;            // tile rows of the unsplit launch
        const long tiles2 = (mt - rows1) * ntl;
        long sp = tiles2 > 0 ? (256 + tiles2 / 2) / tiles2 : 1;
        if (sp > (K / 64) / 8) sp = (K / 64) / 8;
        if (rows1 > 0 && tiles2 > 0 && sp >= 2 && rows1 * ntl * 100 >= (tiles256 / 256) * 256 * 90) {
            tail.m_split = static_cast<int>(rows1 * 256);
            tail.tail_kb = static_cast<int>(cdiv(K / 64, sp));
            tail.tail_splits = static_cast<int>(cdiv(K / 64, tail.tail_kb));
            tail_ok = true;
        }
    }
    // a badly filled last round of a LONG-K layer (320 tiles of a 16x16-level 3x3 conv = 1.25 rounds) is better spent on a
    // split-K tail launch than on a second full round: the tail split goes first when the fill is under
    // PF_GEMM8_TAIL_FIRST % (same-box A/B on the mixed scheme: 69.7 -> 68.7 ms per step)
    if (tail_ok && tiles256 * 100 < rounds * 256 * t.tail_first_pct) return tail;
    if (t.big_min_tiles > 0 && tiles256 >= t.big_min_tiles && filled && K >= t.big_min_k) return plan_big(nrep, K);
    if (tail_ok) return tail;
    // long-K layers with few output tiles (the 8x8 level, the panorama's inner levels): 256-row tiles
    // re-read the weight panel 2-4x less often than the 64-row tiles of the small kernel; split K so
    // that one round of blocks covers the chip
    const int nkb_all = K / 64;
    if (t.big_min_tiles > 0 && allow_split && N % 4 == 0 && tiles256 >= 32 && tiles256 <= 128 && nkb_all >= 32) {
        long sp = 256 / tiles256;
        if (sp > nkb_all / 16) sp = nkb_all / 16;
        if (sp >= 2) {
            pf_conv_plan g = plan_big(nrep, K);
            g.kb_per_split = static_cast<int>(cdiv(nkb_all, sp));
            g.splits = static_cast<int>(cdiv(nkb_all, g.kb_per_split));
            return g;
        }
    }
    return plan_small(M, N, K, batch, allow_split, s3);
}

// Which plans of the 8-wave kernel run as 128-row blocks, two per CU (k_conv_gemm8<..., BM_ = 128>): PF_GEMM_BM128 = 0 none,
// 1 all of them (A/B), 2 (default) the measured rule: the 128-row blocks win where the tile is ramp / epilogue-bound -- short K
// (K <= PF_GEMM_BM128_MAXK: isolated +7 % at K = 320, +15...22 % at K = 640, +12...16 % at K = 1280; long-K convolutions lose
// 3-5 % to the shorter DMA look-ahead and the doubled weight traffic, profiles/r5a_gemm_bm128.txt): same-box step A/B 62.06 -> 61.39 /
// 61.36 ms (profiles/r5b_ab_gemm_bm128.txt).  PF_GEMM_BM128_ONEROUND=1 also takes every problem that is ONE round of 256-row tiles
// (a CU then runs a single ramp + K loop + epilogue with nothing to overlap -- the per-rank GEMMs of the sharded layouts): measured
// neutral to slightly slower on the simulated ranks (8 ranks 14.35 -> 14.48 ms, 4 ranks 19.9 -> 20.4), so off.
static bool takes_128_row_blocks(const pf_conv_plan& g, long M, int N, int K, int batch) {
    const GemmTuning& t = gemm_tuning();
    if (g.kernel != 1 || g.m_split > 0 || t.bm128 == 0) return false;
    if (t.bm128 == 1) return true;
    const long tiles256 = cdiv(M, 256) * cdiv(N, 32 * g.nrep) * batch * g.splits;
    return t.bm128 == 2 && (K <= t.bm128_max_k || (t.bm128_one_round && tiles256 <= 256));
}

// Rows per GroupNorm-moment part (pf_conv_desc.gn_partial) of this problem under plan g: the fragment rows of one
// wavefront -- or 0 where the moments cannot be produced: split K (the reduce kernel writes the output), a batch,
// images that are not whole parts, or an operand mix that takes the per-fragment (generic) epilogue.
static int gn_rows16(const GemmParams& p, const pf_conv_plan& g, int batch) {
    if ((batch != 1 && !p.subpix) || g.splits > 1 || g.m_split > 0 || p.geglu || p.split_out) return 0;   // (the four sub-pixel phases of an image are contiguous runs: gn_part)
    // Layers with a residual are left to the consumer's statistics pass by default.  Round 3: the moment phase has to read the
    // residual tile a second time, which costs an HBM-bound layer as much as that pass saves (fp32-residual linear at
    // 163840 x 320: 141 -> 171 us, the pass it replaces 42 us; VAE decode 107 -> 122 ms; profiles/archive/r3d_gemm_gn.txt).  Round 4: fp32
    // tiles with an fp32 residual form their moments inside the store loop instead (epilogue_f32_stats: no second read, no extra
    // registers) -- and the step still does not move: 63.17 vs 63.33 / 63.54 ms on one box, 61.23 / 61.40 vs 61.00 on another
    // (profiles/r4ah_ab_gn_moments_residual.txt): ~30 statistics passes of 10-55 us leave the critical stream, the column-block-major
    // store order of the fused epilogue gives as much back.  Off; PF_GN_EPILOGUE_RES=1 enables it (tests run both).
    // Without a residual (resnet conv1 -> norm2, the up-sampling conv) the phase costs 2-3 us against a 25-40 us pass.
    if (p.residual && GemmTuning::gn_epilogue_res() == 0) return 0;
    if (g.kernel == 1 && gemm_tuning().big_waves == 4) return 0;   // (the one-wave-per-SIMD A/B instantiation has no moment variant)
    const int rows = g.kernel == 1 ? 64 : 16 * g.mrep;
    const int BM = g.kernel == 1 ? 256 : 32 * g.mrep;
    if (p.rows_per_img % rows != 0 || p.N % (32 * g.nrep) != 0) return 0;      // whole runs per image, whole N tiles
    if (p.out_f32) {
        const bool ok = !p.rowvec && (p.out_ld & 3) == 0 && (!p.residual || (p.res_f32 && (p.res_ld & 3) == 0));
        return ok ? rows : 0;
    }
    const bool staged = !p.res_f32 && (p.out_ld & 7) == 0 && (p.N & 7) == 0 && !(p.rowvec && p.residual) &&
                        !(p.rowvec && p.rows_per_img < BM);
    return staged ? rows : 0;
}

// ---- the 32x32x16 kernel ------------------------------------------------------------------------------------------------------------

// Which problems take the 32x32x16 kernel of pf_gemm32.hip (256 x 320 tiles, one persistent block per CU): plain (not split-precision)
// layers with N a multiple of 320 and a long K whose tiles fill whole rounds of 256 CUs -- or whole rounds plus a tail that a split-K
// launch spreads over the chip once more (640 tiles = 2 rounds + 128 tiles x 2 K slices; 320 = 1 round + 64 x 4).  OFF by default
// (PF_GEMM32=1 enables it; PF_GEMM32_MINK is the least K, PF_GEMM32_K1=1 also admits 1x1 layers): its K loop needs 1680 clocks per 32-wide
// stage against the 16x16 kernel's 2140 per equal-FLOP step, and on N(0,1) operands it is no faster -- the chip is POWER capped there
// (zero operands: +7 %), v_mfma_f32_32x32x16 draws ~13 % more per FLOP than v_mfma_f32_16x16x32 on random data, and the step is 0.6 ms
// slower with it because of the split-K tails its 2.5 / 1.25 rounds need (profiles/r6_gemm32_power_cap.txt).
// Fills kernel 2's tile shape and tail layout; false: the problem stays on the 16x16x32 kernels.
static bool plan32(const GemmParams& p, int batch, bool allow_split, pf_conv_plan& g) {
    const GemmTuning& t = gemm_tuning();
    if (!GemmTuning::gemm32() || p.s3 || p.subpix || batch != 1 || p.N % 320 != 0 || p.K < t.gemm32_min_k || p.K % 64 != 0 || p.geglu)
        return false;
    if (p.ksize != 3 && !t.gemm32_k1) return false;
    const int nkb = p.K / 64;
    g = pf_conv_plan{};
    g.kernel = 2; g.mrep = 8; g.nrep = 10; g.block_rows = 256; g.splits = 1; g.kb_per_split = nkb;
    const long ntl = p.N / 320, mt = cdiv(p.M, 256), tiles = mt * ntl;
    const long full = tiles / 256 * 256, rest = tiles - full;
    if (rest == 0) return true;
    if (full == 0 || !allow_split || p.N % 4 != 0) return false;
    const long rows1 = full / ntl;                                  // tile rows of the unsplit launch (ntl divides 256)
    long sp = (256 + rest / 2) / rest;
    if (sp > nkb / 8) sp = nkb / 8;
    if (sp < 2 || rest * sp > 256) return false;
    g.m_split = static_cast<int>(rows1 * 256);
    g.tail_kb = static_cast<int>(cdiv(nkb, sp));
    g.tail_splits = static_cast<int>(cdiv(nkb, g.tail_kb));
    return true;
}
// Rows per GroupNorm-moment run of the 32x32 kernel (a wave's 64 rows), or 0: a split-K tail (the reduce kernel writes those rows), a
// residual (left to the consumer's pass, see gn_rows16), a row vector over images that are not whole runs, pair output.
static int gn_rows32(const GemmParams& p, const pf_conv_plan& g) {
    if (g.m_split > 0 || p.residual || p.split_out || p.geglu) return 0;
    if (p.rows_per_img % 64 != 0) return 0;
    const bool ok = p.out_f32 ? (p.out_ld & 3) == 0 : (p.out_ld & 7) == 0;
    return ok ? 64 : 0;
}

// ---- the plan -----------------------------------------------------------------------------------------------------------------------

pf_conv_plan plan_conv_gemm(const GemmParams& p, int batch, bool allow_split, bool want_moments) {
    const GemmTuning& t = gemm_tuning();
    pf_conv_plan g{};
    // moments asked for and the 32x32 plan cannot emit them: the 16x16 plan serves the launch
    if (plan32(p, batch, allow_split, g) && (!want_moments || gn_rows32(p, g) > 0)) {
        g.gn_rows = want_moments ? 64 : 0;
        g.waves = 8; g.ring_slots = 4;
    } else {
        g = plan_tiles(p.M, p.N, p.K, batch, allow_split, p.s3 != 0);
        g.gn_rows = want_moments ? gn_rows16(p, g, batch) : 0;
        if (p.a32 && g.kernel == 1) g.gn_rows = 0;                  // (fp32 sources: the 8-wave kernel has no moment variant -- its staging registers are what that variant spends)
        if (g.kernel == 1) {
            // 128-row blocks: four waves and a two-slot ring, two blocks per CU.  PF_GEMM8_WAVES=4: one 128x80 wave per SIMD (accumulators in AGPRs)
            // is implemented and correct but measured slower (K step 2520 vs 2222 clocks, epilogue 2x): a lone in-order wave exposes every
            // lgkmcnt / vmcnt / barrier wait (A/B: it moves 28 % fewer fragment bytes through the LDS; no split-precision variant).
            if (takes_128_row_blocks(g, p.M, p.N, p.K, batch)) { g.block_rows = 128; g.waves = 4; g.ring_slots = 2; }
            else { g.waves = t.big_waves == 4 && !p.s3 ? 4 : 8; g.ring_slots = 3; }
        } else {
            // a grid of at most one block per CU runs the four-slot ring (one block per CU: nothing to share the CU with anyway); the moment /
            // split-precision variants keep the two-slot form (they are not instantiated with four slots)
            const long blocks = cdiv(p.M, g.block_rows) * cdiv(p.N, 32 * g.nrep) * g.splits * batch;
            const int deep_max = t.deep_ring ? t.deep_ring_max_blocks : 0;
            g.waves = 4;
            g.ring_slots = g.gn_rows == 0 && !p.s3 && blocks <= deep_max && p.K / 64 / g.splits >= 3 ? 4 : 2;
        }
    }
    const long rows2 = p.M - g.m_split;                             // rows of the split launch
    if (g.m_split > 0) g.workspace_bytes = static_cast<size_t>(g.tail_splits) * rows2 * p.N * sizeof(float);
    else if (g.splits > 1) g.workspace_bytes = static_cast<size_t>(g.splits) * batch * p.M * p.N * sizeof(float);
    // (one arrival counter per (batch, tile) of the split launch; the 32x32 kernel's tail is always combined by the reduce kernel)
    if (g.workspace_bytes && g.kernel != 2) g.n_tickets = static_cast<int>(cdiv(rows2, g.block_rows) * cdiv(p.N, 32 * g.nrep) * batch);
    return g;
}

}  // namespace pf

using namespace pf;

extern "C" pf_status pf_conv_gemm_plan(const pf_conv_desc* d, int want_moments, pf_conv_plan* out) {
    PF_REQUIRE(d && out, "pf_conv_gemm_plan: null pointer");
    PF_REQUIRE(d->batch >= 1 && d->n_out >= 1 && d->n_img >= 1, "pf_conv_gemm_plan: batch, n_out and n_img must be >= 1");
    GemmParams p;
    params_from_desc(d, p);
    *out = plan_conv_gemm(p, d->subpixel ? 4 : d->batch, true, want_moments != 0);
    return PF_OK;
}

// The three older queries: projections of the plan.
extern "C" int pf_conv_gemm_gn_rows(const pf_conv_desc* d) {
    pf_conv_plan g;
    return pf_conv_gemm_plan(d, 1, &g) == PF_OK ? g.gn_rows : 0;
}

extern "C" int pf_conv_gemm_kernel_id(const pf_conv_desc* d) {
    pf_conv_plan g;
    return pf_conv_gemm_plan(d, 0, &g) == PF_OK ? g.kernel : -1;
}

extern "C" size_t pf_conv_gemm_workspace_size(const pf_conv_desc* d) {
    pf_conv_plan g0, g1;
    if (pf_conv_gemm_plan(d, 0, &g0) != PF_OK || pf_conv_gemm_plan(d, 1, &g1) != PF_OK) return 0;
    // room for either launch, with or without moments -- except that a layer with a residual whose moment launch cannot emit them
    // (it fails) does not count
    if (d->residual && g1.gn_rows == 0) return g0.workspace_bytes;
    return g0.workspace_bytes > g1.workspace_bytes ? g0.workspace_bytes : g1.workspace_bytes;
}
