// Host side of the attention front ends (no device code): the environment knobs, the descriptor checks pf_attention and
// pf_attention_wide share, and THE plan of a pf_attention problem -- which kernel and instantiation, the split of the key range, grid
// and scratch -- that pf_attention launches and pf_attention_plan / pf_attention_workspace_size report.  The same for pf_attention_bwd
// (kernels in pf_backward.hip): its knobs, its descriptor checks and THE plan behind pf_attention_bwd_plan / _workspace_size.
#include "pf_attention_plan.h"
#include <algorithm>

namespace pf {

const AttnTuning& attn_tuning() {
    static const AttnTuning t;
    return t;
}

pf_status validate_attn_desc(const pf_attn_desc* d, const char* who) {
    PF_REQUIRE(d, "%s: null descriptor", who);
    PF_REQUIRE(d->q && d->k && d->vt && d->out, "%s: null pointer", who);
    PF_REQUIRE(d->B > 0 && d->H > 0 && d->nq > 0 && d->nk > 0, "%s: bad sizes", who);
    PF_REQUIRE(d->q_ld % 8 == 0 && d->k_ld % 8 == 0 && d->o_ld % 4 == 0 && d->vt_ld % 4 == 0,
               "%s: leading dimensions must be multiples of 8 (q,k) / 4 (out, vt)", who);
    const long cols = static_cast<long>(d->H) * d->D;
    PF_REQUIRE(d->q_ld >= cols && d->k_ld >= cols && d->o_ld >= cols, "%s: q_ld, k_ld and o_ld must cover H * D = %ld columns", who, cols);
    PF_REQUIRE(d->vt_ld >= ((d->nk + 31) / 32) * 32, "%s: vt_ld=%d must cover nk=%d rounded up to 32", who, d->vt_ld, d->nk);
    PF_REQUIRE(d->q_bs % 8 == 0 && d->k_bs % 8 == 0 && d->vt_bs % 4 == 0 && d->o_bs % 4 == 0, "%s: batch strides misaligned", who);
    PF_REQUIRE(aligned16(d->q) && aligned16(d->k) && aligned16(d->vt) && aligned16(d->out), "%s: pointers must be 16-byte aligned", who);
    PF_REQUIRE((d->bias == nullptr) == (d->flags == nullptr), "%s: bias and flags come together", who);
    return PF_OK;
}

// ---- the plan -----------------------------------------------------------------------------------------------------------------------

// Workgroups of plan g per grid dimension, in 64 bits (the plan's grid_x / y / z are these, narrowed).  k_attention: (query blocks,
// heads, batches); the LDS kernels: 1-D over (query block, head, batch), decoded in the kernel, the splits of the key range in y.
static void grid_of(const pf_attn_desc* d, const pf_attn_plan& g, long (&n)[3]) {
    const long qb = cdiv(d->nq, g.block_queries);
    if (g.kernel == 0) { n[0] = qb; n[1] = d->H; n[2] = d->B; }
    else { n[0] = qb * d->H * d->B; n[1] = g.splits; n[2] = 1; }
}

bool attn_grid_launchable(const pf_attn_desc* d, const pf_attn_plan& g) {
    const long lim = 0xFFFFFFFFL / g.threads;                                   // HIP refuses grid x block sizes past 2^32 - 1 threads
    if (g.kernel != 0 && static_cast<long>(d->H) * d->B > lim) return false;    // (so that the product below stays in 64 bits)
    long n[3];
    grid_of(d, g, n);
    return n[0] <= lim && n[1] <= 65535 && n[2] <= 65535;
}

// Split of the key range: a launch of the biased D = 32 kernel (EPA) whose query blocks fill less than ~0.95 of the chip's workgroup
// slots (256 CUs x occupancy) with a long key walk is cut into S splits of an even number of key tiles, at least
// PF_ATTENTION_SPLIT_MIN_TILES each, aiming at ~1.9 rounds of workgroups.  Fills splits, split_tiles and workspace_bytes: S normalised
// 16-bit partial outputs [S][B][nq][H * D], then their fp32 log-sum-exps [S][B][H][nq].  (The register-pipelined form walks three LDS
// buffers: never split.)
static void plan_split(const pf_attn_desc* d, pf_attn_plan& g) {
    const AttnTuning& t = attn_tuning();
    if (!AttnTuning::split() || d->lse || d->o_ld % 8 != 0 || d->o_bs % 8 != 0) return;
    const long blocks = cdiv(d->nq, 128) * d->H * d->B, slots = 256L * g.occupancy;
    const int nkt = (d->nk + 63) / 64;
    if (blocks * 20 >= slots * 19) return;
    int S = static_cast<int>((slots * 19 / 10 + blocks / 2) / blocks);
    S = std::min(S, 8);
    S = std::min(S, nkt / std::max(t.split_min_tiles, 2));
    if (S < 2) return;
    int tiles = static_cast<int>(cdiv(nkt, S));
    tiles += tiles & 1;
    S = static_cast<int>(cdiv(nkt, tiles));
    if (S < 2) return;
    g.splits = S; g.split_tiles = tiles;
    const size_t rows = static_cast<size_t>(S) * d->B * d->nq * d->H;
    g.workspace_bytes = rows * d->D * 2 + rows * sizeof(float);
}

pf_attn_plan plan_attention(const pf_attn_desc* d, bool allow_split) {
    const AttnTuning& t = attn_tuning();
    pf_attn_plan g{};
    g.block_queries = 128; g.threads = 256; g.splits = 1;
    // (k_attention_lds addresses K / V^T tiles with 32-bit byte offsets inside one (batch, head) slice)
    const bool fits32 = !attn_build_bufload || (static_cast<long>(d->nk + 64) * d->k_ld * 2 < (1L << 31) && static_cast<long>(d->vt_ld) * (d->D + 1) * 2 < (1L << 31));
    if (t.lds && d->vt_ld % 8 == 0 && d->vt_bs % 8 == 0 && fits32) {
        g.kernel = 1;
        if (d->D == 64 && d->bias) {                       // always pipelined (not pipelined it needs 169 registers at three waves per SIMD)
            g.pipelined = 1; g.occupancy = 2;
        } else if (d->D == 64) {
            // The experimental ping-pong kernels address K and V^T with 32-bit byte offsets inside a (batch, head) slice; the one-tile
            // form takes ragged key counts that are multiples of 8, the two-tile form multiples of 128.  lse = training forward: exact
            // fp32 row sums there (the timing build of the one-tile form writes its stamps over lse instead).
            const bool pp_fits = static_cast<long>(d->nk) * d->k_ld * 2 < (1L << 31) && static_cast<long>(d->vt_ld) * 64 * 2 < (1L << 31);
            const bool pp1_ok = (attn_build_pp_timing || !d->lse) && d->nk % 8 == 0 && d->nk >= 128 && pp_fits;
            const bool pp2_ok = !d->lse && d->nk % 128 == 0 && d->nk >= 256 && pp_fits;
            const int pingpong = AttnTuning::pingpong();
            if (pingpong == 2 && pp2_ok) g.kernel = 3;
            else if (pingpong && pp1_ok) g.kernel = 2;
            else if (t.occ64 == 2) { g.pipelined = 1; g.occupancy = 2; }
            else { g.occupancy = 3; g.msum = t.msum && !d->lse && d->nk >= 256; }     // (77 text keys: the 4 extra MFMAs of two tiles cost 2 %)
            if (g.kernel != 1) { g.block_queries = 256; g.threads = 512; }
        } else if (t.occ32 == 4 || t.occ32 == 5) {
            g.occupancy = t.occ32;
            if (d->bias && allow_split) plan_split(d, g);
        } else {
            g.pipelined = 1; g.occupancy = 3; g.msum = d->bias && t.msum32 && !d->lse;
        }
    }
    long n[3];
    grid_of(d, g, n);
    g.grid_x = static_cast<unsigned>(n[0]); g.grid_y = static_cast<unsigned>(n[1]); g.grid_z = static_cast<unsigned>(n[2]);
    return g;
}

pf_attn_plan plan_attention_launch(const pf_attn_desc* d) {
    const pf_attn_plan g = plan_attention(d, true);
    const bool scratch = d->workspace && d->workspace_bytes >= g.workspace_bytes && aligned16(d->workspace);
    return g.splits > 1 && !scratch ? plan_attention(d, false) : g;
}

// ---- pf_attention_bwd -----------------------------------------------------------------------------------------------------------------

const AttnBwdTuning& attn_bwd_tuning() {
    static const AttnBwdTuning t;
    return t;
}

// Query split of the keys-stationary launch: towards ~512 blocks, at least 8 query tiles (256 queries) per block.  A launch with few
// blocks (the 128 text keys of a cross-attention: H x B blocks walking all queries; one panorama sample) splits the query range over
// several blocks per key block, which leave fp32 partial sums [qsplit][B][nk][H * D] for dK and for dV, added in a fixed order by
// k_attn_bwd_reduce.  (That kernel works on quads of the H * D columns: whole for D in {32, 64}.)
static int plan_qsplit(const pf_attn_bwd_desc* d) {
    const long base = cdiv(d->nk, 128) * d->H * d->B;
    if (base >= 384) return 1;
    return static_cast<int>(std::max<long>(1, std::min<long>(cdiv(512, base), (d->nq / 32) / 8)));
}

pf_attn_bwd_plan plan_attention_bwd(const pf_attn_bwd_desc* d, bool allow_split) {
    const AttnBwdTuning& t = attn_bwd_tuning();
    pf_attn_bwd_plan g{};
    g.threads = 256; g.qsplit = 1;
    const bool tail = d->nq % 32 != 0 || d->nk % 32 != 0;          // ragged token counts: guarded loads, masked tails
    // LDS-staged kernels: whole 32-token tiles, 16-byte rows for the cooperative loads of the transposed tiles
    const bool rows16 = d->qt_ld % 8 == 0 && d->kt_ld % 8 == 0 && d->dot_ld % 8 == 0 && d->qt_bs % 8 == 0 && d->kt_bs % 8 == 0 && d->dot_bs % 8 == 0;
    g.kernel = t.lds && !tail && rows16 ? 2 : tail ? 1 : 0;
    if (g.kernel == 2 && t.qsplit && allow_split) g.qsplit = plan_qsplit(d);
    g.dq_grid_x = static_cast<unsigned>(cdiv(d->nq, 128)); g.dq_grid_y = d->H; g.dq_grid_z = d->B;
    g.dkv_grid_x = static_cast<unsigned>(cdiv(d->nk, 128) * g.qsplit); g.dkv_grid_y = d->H; g.dkv_grid_z = d->B;
    if (g.qsplit > 1) {
        const size_t elems = static_cast<size_t>(d->B) * d->nk * d->H * d->D;
        g.reduce_grid_x = static_cast<unsigned>(cdiv(static_cast<long>(elems / 4), 256)); g.reduce_grid_y = g.reduce_grid_z = 1;
        g.workspace_bytes = 2 * g.qsplit * elems * sizeof(float);
    }
    return g;
}

bool attn_bwd_grids_launchable(const pf_attn_bwd_plan& g) {
    const unsigned lim = 0xFFFFFFFFu / g.threads;                 // HIP refuses grid x block sizes past 2^32 - 1 threads
    auto ok = [lim](unsigned x, unsigned y, unsigned z) { return x <= lim && y <= 65535 && z <= 65535; };
    return ok(g.dq_grid_x, g.dq_grid_y, g.dq_grid_z) && ok(g.dkv_grid_x, g.dkv_grid_y, g.dkv_grid_z) && ok(g.reduce_grid_x, g.reduce_grid_y, g.reduce_grid_z);
}

pf_status validate_attn_bwd_desc(const pf_attn_bwd_desc* d, const char* who) {
    PF_REQUIRE(d, "%s: null descriptor", who);
    PF_REQUIRE(d->q && d->k && d->v && d->dout && d->qt && d->kt && d->dot && d->dq && d->dk && d->dv && d->lse && d->delta, "%s: null pointer", who);
    PF_REQUIRE(d->D == 32 || d->D == 64, "%s: head dim %d unsupported (32 or 64)", who, d->D);
    PF_REQUIRE(d->B > 0 && d->H > 0 && d->nq > 0 && d->nk > 0, "%s: bad sizes", who);
    PF_REQUIRE(d->q_ld % 8 == 0 && d->k_ld % 8 == 0 && d->v_ld % 8 == 0 && d->do_ld % 8 == 0, "%s: row-major leading dimensions must be multiples of 8", who);
    PF_REQUIRE(d->qt_ld % 4 == 0 && d->kt_ld % 4 == 0 && d->dot_ld % 4 == 0 && d->qt_ld >= d->nq && d->dot_ld >= d->nq && d->kt_ld >= d->nk,
               "%s: transposed leading dimensions must be multiples of 4 and cover the token count", who);
    PF_REQUIRE(d->dq_ld % 4 == 0 && d->dk_ld % 4 == 0 && d->dv_ld % 4 == 0, "%s: output leading dimensions must be multiples of 4", who);
    PF_REQUIRE(d->q_bs % 8 == 0 && d->k_bs % 8 == 0 && d->v_bs % 8 == 0 && d->do_bs % 8 == 0 && d->qt_bs % 4 == 0 && d->kt_bs % 4 == 0 &&
               d->dot_bs % 4 == 0 && d->dq_bs % 4 == 0 && d->dk_bs % 4 == 0 && d->dv_bs % 4 == 0, "%s: batch strides misaligned", who);
    PF_REQUIRE(aligned16(d->q) && aligned16(d->k) && aligned16(d->v) && aligned16(d->dout) && aligned16(d->qt) && aligned16(d->kt) &&
               aligned16(d->dot) && aligned16(d->dq) && aligned16(d->dk) && aligned16(d->dv) && aligned16(d->lse) && aligned16(d->delta),
               "%s: pointers must be 16-byte aligned", who);
    PF_REQUIRE((d->bias == nullptr) == (d->flags == nullptr), "%s: bias and flags come together", who);
    if (d->bias) {
        PF_REQUIRE(d->nk % 4 == 0 && d->bias_ld % 4 == 0 && d->bias_ld >= d->nk && aligned16(d->bias), "%s: bias needs nk %% 4 == 0 and an aligned ld >= nk", who);
        PF_REQUIRE(d->flags_ld >= (d->nk + 31) / 32, "%s: flags_ld too small", who);
    }
    const long cols = static_cast<long>(d->H) * d->D;
    PF_REQUIRE(d->q_ld >= cols && d->k_ld >= cols && d->v_ld >= cols && d->do_ld >= cols && d->dq_ld >= cols && d->dk_ld >= cols && d->dv_ld >= cols,
               "%s: q_ld, k_ld, v_ld, do_ld, dq_ld, dk_ld and dv_ld must cover H * D = %ld columns", who, cols);
    PF_REQUIRE(attn_bwd_grids_launchable(plan_attention_bwd(d, true)), "%s: B=%d, H=%d, nq=%d, nk=%d exceed the grid limits of the launch", who, d->B, d->H, d->nq, d->nk);
    return PF_OK;
}

}  // namespace pf

using namespace pf;

extern "C" pf_status pf_attention_plan(const pf_attn_desc* d, pf_attn_plan* out) {
    PF_REQUIRE(d && out, "pf_attention_plan: null pointer");
    PF_REQUIRE(d->B > 0 && d->H > 0 && d->nq > 0 && d->nk > 0, "pf_attention_plan: bad sizes");
    PF_REQUIRE(d->D == 32 || d->D == 64, "pf_attention_plan: head dim %d unsupported (32 or 64)", d->D);
    *out = plan_attention(d, true);
    return PF_OK;
}

extern "C" size_t pf_attention_workspace_size(const pf_attn_desc* d) {
    pf_attn_plan g;
    return pf_attention_plan(d, &g) == PF_OK ? g.workspace_bytes : 0;
}

extern "C" pf_status pf_attention_bwd_plan(const pf_attn_bwd_desc* d, pf_attn_bwd_plan* out) {
    PF_REQUIRE(d && out, "pf_attention_bwd_plan: null pointer");
    PF_REQUIRE(d->B > 0 && d->H > 0 && d->nq > 0 && d->nk > 0, "pf_attention_bwd_plan: bad sizes");
    PF_REQUIRE(d->D == 32 || d->D == 64, "pf_attention_bwd_plan: head dim %d unsupported (32 or 64)", d->D);
    *out = plan_attention_bwd(d, true);
    return PF_OK;
}

extern "C" size_t pf_attention_bwd_workspace_size(const pf_attn_bwd_desc* d) {
    pf_attn_bwd_plan g;
    return pf_attention_bwd_plan(d, &g) == PF_OK ? g.workspace_bytes : 0;
}
