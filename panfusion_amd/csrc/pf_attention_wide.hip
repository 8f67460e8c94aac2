// Flash attention on MFMA for gfx950 (CDNA4) at WIDE heads, D in {128, 256, 512}: the VAE mid-block attention (one head of
// width 512) without its N x N score matrix.
//
//   out[b][i][h*D+:] = softmax_j(scale * q_i.k_j) v_j
//
// A workgroup of 4 wavefronts owns 64 query rows and ALL D output columns; a wavefront owns 16 of the rows and walks the keys in
// tiles of 64 with an online softmax.  Both products are computed TRANSPOSED on v_mfma_f32_16x16x32 so that a lane owns one query
// column (as pf_attention.hip does on the 32x32 shape):
//   S^T = K Q^T   : A = K tile (rows = keys) from LDS, B = Q^T held in registers for the whole walk (D / 8 registers).  Lane
//                   (query l & 15, g = l >> 4) then holds keys 16 a + 4 g + r of score tile a: row max / row sum are local
//                   operations + two lane exchanges (l ^ 16, l ^ 32), no LDS.
//   O^T += V^T P^T: A = V^T tile (rows = head dim, keys contiguous) from LDS, B = P^T straight from the score registers: k-slot
//                   (g, j) of a 32-key step stands for key 4 g + j (j < 4) / 16 + 4 g + j - 4 (j >= 4) in BOTH operands, so P
//                   needs no cross-lane movement (the V^T tile is stored in that key order in LDS: a fragment is one 16-byte read).
// The accumulator O^T is D / 4 registers per lane (128 at D = 512), Q^T D / 8 (64), the staging registers 2 x D / 8 (128): one
// wavefront per SIMD (up to 512 registers per lane, VGPR + AGPR), no redundant work, nothing spilled.
//
// K [64 keys][D] and V^T [D][64 keys] of a step are fetched once per workgroup with coalesced 16-byte loads, staged through
// registers into LDS and shared by the 4 wavefronts (D = 512: 64 KiB + 80 KiB of the CU's 160 KiB, one buffer each).  With one
// workgroup per CU nothing else hides a load, so each tile is requested a WHOLE key tile before it is written to LDS (K and V^T
// have D / 8 staging registers each); three barriers per 64 keys:
//   S = K_j Q^T | A | V_j -> LDS, load V_j+1, softmax | B | O^T += V_j^T P^T, K_j+1 -> LDS, load K_j+2 | C
//   K rows are 2 D bytes; the 16-B chunk index is XOR-swizzled with the key (& 15) so the ds_read_b128 fragment reads of 16
//   different keys land on 16 different 16-B slots of the 256-B bank row.
//   V^T rows are padded to 160 B (ten 16-B slots) and hold the keys of a 32-key step in the MFMA's k-slot order, so a fragment is one
//   ds_read_b128 and the 16 d-rows x 2 k-groups of a lane group land on 16 different slots of the bank row.
//
// Rounding points (those of every forward arm of pf_attention.hip): scores in fp32; online softmax in the exp2 domain, the
// reference point moved at every key tile (no deferred rescale; a tile in which no row of the wave moved its maximum skips the
// products with alpha = 1, which changes no bit); P rounded to the 16-bit type before the second product; fp32
// accumulation; the denominator is the fp32 sum of the UNROUNDED P (not the MSUM form); the output normalised and rounded once.
//
// Addressing: batch strides are 64-bit; INSIDE one (batch, head) slice K and V^T are addressed with 31-bit byte offsets, so
// (nk + 64) * k_ld * 2 and D * vt_ld * 2 must stay under 2^31 (nk = 34 816 at D = 512: 36 MB); q and out rows are 64-bit.  The
// grid is 1-D: ceil(nq / 64) * H * B < 2^31.
//
// Replaces the mid-block Attention(heads = 1, dim_head = C) of diffusers' AutoencoderKL (baddbmm + softmax + bmm), reached from
// models/pano/PanoGenerator.py:213-238 (decode / encode of the panorama and the views).
#include "pf_attention_plan.h"

namespace pf {

struct WideParams {
    const unsigned short* q; const unsigned short* k; const unsigned short* vt; unsigned short* out;
    int H, nq, nk;
    int q_ld, k_ld, vt_ld, o_ld;
    long q_bs, k_bs, vt_bs, o_bs;
    float scale_log2e;
    int v16;                     // 1: V^T rows and batch stride allow 16-byte loads (vt_ld % 8 == 0, vt_bs % 8 == 0); 0: 8-byte loads
};

// v_mfma_f32_16x16x32 on 16-bit operands.  A[row][k]: lane l supplies row l & 15, k = 8 (l >> 4) .. + 7; B[k][col]: col l & 15,
// same k; C[row][col]: lane l holds col l & 15, rows 4 (l >> 4) + r.
template <typename T> struct Mfma16;
template <> struct Mfma16<Bf16> {
    typedef __attribute__((ext_vector_type(8))) __bf16 frag;
    static __device__ __forceinline__ f32x4 run(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <> struct Mfma16<F16> {
    typedef __attribute__((ext_vector_type(8))) _Float16 frag;
    static __device__ __forceinline__ f32x4 run(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};

constexpr int WIDE_KT = 64;                            // keys per tile
constexpr int WIDE_VROW = WIDE_KT + 16;                // elements per padded V^T row in LDS (160 B = ten 16-B slots)
constexpr size_t wide_lds_bytes(int D) { return static_cast<size_t>(WIDE_KT * D + D * WIDE_VROW) * 2; }

template <typename T, int D>
__global__ __launch_bounds__(256, 1) void k_attention_wide(const WideParams p) {
    constexpr int KT = WIDE_KT, VROW = WIDE_VROW;
    constexpr int KS = D / 32;                         // k-steps of the QK^T product
    constexpr int DT = D / 16;                         // 16-row tiles of O^T
    constexpr int KCHUNKS = D / 8;                     // 16-B chunks per K row
    constexpr int NST = D / 32;                        // staged 16-B chunks per thread and tile (K: 64 D / 8 / 256, V^T: D 8 / 256)
    constexpr int K_ELEMS = KT * D;
    typedef typename Mfma16<T>::frag frag;
    extern __shared__ __attribute__((aligned(16))) unsigned short smem[];
    unsigned short* const Ks = smem;
    unsigned short* const Vs = smem + K_ELEMS;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ql = lane & 15, g = lane >> 4;
    const int nqb = (p.nq + 63) / 64;
    const int bh = static_cast<int>(blockIdx.x) / nqb, qb = static_cast<int>(blockIdx.x) - bh * nqb;
    const int h = bh % p.H;
    const long b = bh / p.H;
    const int q0 = qb * 64 + wave * 16;
    const unsigned short* qp = p.q + b * p.q_bs + h * D;
    const unsigned short* kp = p.k + b * p.k_bs + h * D;
    const unsigned short* vp = p.vt + b * p.vt_bs + static_cast<long>(h) * D * p.vt_ld;
    const int qrow = min(q0 + ql, p.nq - 1);           // (rows past nq compute a copy of the last row and store nothing)

    frag qf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s)
        qf[s] = __builtin_bit_cast(frag, *reinterpret_cast<const u16x8*>(qp + static_cast<long>(qrow) * p.q_ld + 32 * s + 8 * g));

    f32x4 o[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) o[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;

    const int nkt = (p.nk + KT - 1) / KT;
    u16x8 kst[NST], vst[NST];                          // staging registers: the K and the V^T tile in flight, each a whole key tile ahead of its use
    // staging ownership (fixed per thread): chunk c = t + 256 i; K -> (key tr + RPP i, chunk tc), V^T -> (d = (t >> 3) + 32 i, keys 8 (t & 7) ..)
    constexpr int RPP = 256 / KCHUNKS;                 // K rows per pass of the 256 threads (4 / 8 / 16)
    const int tr = t / KCHUNKS, tc = t % KCHUNKS;
    // K and V^T tiles come through buffer descriptors (base = this (batch, head)'s K / V^T, SGPR; the launcher checks that a slice fits
    // 31-bit byte offsets) + ONE per-thread 32-bit byte offset + a scalar offset per load: no 64-bit vector address per load (2 x 16 of
    // them at D = 512 pushed the kernel into scratch).  Every offset is kept inside the slice by construction (the last tile clamps its
    // rows / pieces); the descriptors also END with the slice -- K after key nk - 1, V^T after row D - 1.
    typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
    const __amdgpu_buffer_rsrc_t rs_k = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(kp), 0, ((p.nk - 1) * p.k_ld + D) * 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_v = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(vp), 0, D * p.vt_ld * 2, 0x00020000);
    const unsigned kvoff = static_cast<unsigned>(tr * p.k_ld + tc * 8) * 2u;              // bytes
    auto load_k = [&](int j) {
        if (j * KT + KT <= p.nk) {
#pragma unroll
            for (int i = 0; i < NST; ++i) {
                const int so = __builtin_amdgcn_readfirstlane((j * KT + RPP * i) * p.k_ld * 2);
                kst[i] = __builtin_bit_cast(u16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_k, kvoff, so, 0));
            }
        } else {                                       // last tile: rows past nk read key nk - 1 again (their scores are masked below)
#pragma unroll
            for (int i = 0; i < NST; ++i) {
                const int row = min(j * KT + RPP * i + tr, p.nk - 1);
                kst[i] = __builtin_bit_cast(u16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_k, static_cast<unsigned>(row * p.k_ld + tc * 8) * 2u, 0, 0));
            }
        }
    };
    auto store_k = [&]() {
        const int sw0 = tc ^ tr;                       // (row & 15) = tr | (RPP i & 15): tr < RPP <= 16, a power of two
#pragma unroll
        for (int i = 0; i < NST; ++i)
            *reinterpret_cast<u16x8*>(Ks + (tr + RPP * i) * D + ((sw0 ^ ((RPP * i) & 15)) << 3)) = kst[i];
    };
    auto load_v = [&](int j) {
        // a 4- / 8-key piece that would start past the row's end (last tile only: vt_ld covers nk rounded up to 32) reads the row's start
        // instead: all its keys are past nk and store_v zeroes them
        const int key0 = j * KT + (t & 7) * 8;
        if (p.v16) {
            const unsigned vo = static_cast<unsigned>((t >> 3) * p.vt_ld + (key0 < p.vt_ld ? key0 : 0)) * 2u;
#pragma unroll
            for (int i = 0; i < NST; ++i) {
                const int so = __builtin_amdgcn_readfirstlane(32 * i * p.vt_ld * 2);
                vst[i] = __builtin_bit_cast(u16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_v, vo, so, 0));
            }
        } else {                                       // V^T rows that are only 8-byte aligned
            typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
            const unsigned vlo = static_cast<unsigned>((t >> 3) * p.vt_ld + (key0 < p.vt_ld ? key0 : 0)) * 2u;
            const unsigned vup = static_cast<unsigned>((t >> 3) * p.vt_ld + (key0 + 4 < p.vt_ld ? key0 + 4 : 0)) * 2u;
#pragma unroll
            for (int i = 0; i < NST; ++i) {
                const int so = __builtin_amdgcn_readfirstlane(32 * i * p.vt_ld * 2);
                const u32x2 lo = __builtin_amdgcn_raw_buffer_load_b64(rs_v, vlo, so, 0);
                const u32x2 up = __builtin_amdgcn_raw_buffer_load_b64(rs_v, vup, so, 0);
                vst[i] = __builtin_bit_cast(u16x8, u32x4{lo[0], lo[1], up[0], up[1]});
            }
        }
    };
    auto store_v = [&](int j) {
        if (j * KT + KT > p.nk) {                      // last tile: keys past nk are the padding of V^T or the next row, which may hold anything (0 * NaN = NaN)
            const int key0 = j * KT + (t & 7) * 8;
#pragma unroll
            for (int i = 0; i < NST; ++i)
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (key0 + e >= p.nk) vst[i][e] = 0;
        }
        // inside a 32-key step the keys are stored in the order the MFMA consumes them: key 16 h2 + 4 g + r at 8 g + 4 h2 + r, so that
        // a lane's fragment (keys 4 g .. + 3 and 16 + 4 g .. + 3) is ONE 16-byte read.  This thread's keys 8 c .. 8 c + 7 (c = t & 7):
        // s2 = c >> 2, h2 = (c >> 1) & 1, g = 2 (c & 1) for the first four and g + 1 for the rest -> positions pos and pos + 8
        const int c = t & 7, pos = 32 * (c >> 2) + 16 * (c & 1) + 4 * ((c >> 1) & 1);
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            unsigned short* dst = Vs + ((t >> 3) + 32 * i) * VROW + pos;    // 8-byte aligned (160-B rows)
            const u16x8 v = vst[i];
            *reinterpret_cast<u16x4*>(dst) = u16x4{v[0], v[1], v[2], v[3]};
            *reinterpret_cast<u16x4*>(dst + 8) = u16x4{v[4], v[5], v[6], v[7]};
        }
    };

    int kq[4];                                         // swizzled chunk (4 kk + g) ^ ql of the four k-steps inside a 256-B bank row, in elements
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) kq[kk] = ((4 * kk + g) ^ ql) << 3;

    load_k(0);
    store_k();
    load_v(0);
    if (nkt > 1) load_k(1);
    __syncthreads();

    for (int j = 0; j < nkt; ++j) {
        const int k0 = j * KT;
        // ---- S^T = K_j Q^T: four 16-key tiles
        f32x4 s[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) s[a] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const u16x8 kf = *reinterpret_cast<const u16x8*>(Ks + (a * 16 + ql) * D + 128 * (ks >> 2) + kq[ks & 3]);
                s[a] = Mfma16<T>::run(__builtin_bit_cast(frag, kf), qf[ks], s[a]);
            }
        __syncthreads();                               // A: every wave is done with K_j and with V_j-1
        store_v(j);
        if (j + 1 < nkt) load_v(j + 1);

        // ---- online softmax of the tile (exp2 domain)
        float sv[16];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) sv[4 * a + r] = s[a][r] * p.scale_log2e;
        if (k0 + KT > p.nk) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (k0 + 16 * a + 4 * g + r >= p.nk) sv[4 * a + r] = -INFINITY;
        }
        float mt = sv[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mt = fmaxf(mt, sv[r]);
        mt = fmaxf(mt, __shfl_xor(mt, 16));
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        const float m_new = fmaxf(m_run, mt);          // finite: key k0 of a tile always exists
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        float pv[16], ls = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            pv[r] = __builtin_amdgcn_exp2f(sv[r] - m_new);
            ls += pv[r];
        }
        ls += __shfl_xor(ls, 16);
        ls += __shfl_xor(ls, 32);
        l_run = l_run * alpha + ls;
        const float m_old = m_run;
        m_run = m_new;
        // rescale only when some row of this wave moved its maximum (always at the first tile: m_old = -inf, alpha = 0); otherwise
        // alpha == 1 in every lane and skipping the products changes no bit
        if (__builtin_amdgcn_ballot_w64(m_new > m_old) != 0) {
#pragma unroll
            for (int d = 0; d < DT; ++d) o[d] *= alpha;
        }
        u16x8 pb[2];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int e = 0; e < 8; ++e) pb[s2][e] = from_f32<T>(pv[8 * s2 + e]);       // tile 2 s2 (e < 4), tile 2 s2 + 1 (e >= 4)
        __syncthreads();                               // B: V_j is in LDS

        // ---- O^T += V_j^T P^T
#pragma unroll
        for (int d = 0; d < DT; ++d)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const u16x8 vf = *reinterpret_cast<const u16x8*>(Vs + (d * 16 + ql) * VROW + 32 * s2 + 8 * g);
                o[d] = Mfma16<T>::run(__builtin_bit_cast(frag, vf), __builtin_bit_cast(frag, pb[s2]), o[d]);
            }
        if (j + 1 < nkt) store_k();                    // K_j+1, loaded a tile ago (every wave passed A: nobody reads K_j any more)
        if (j + 2 < nkt) load_k(j + 2);
        __syncthreads();                               // C: K_j+1 is in LDS
    }

    if (q0 + ql < p.nq) {
        const float inv = 1.0f / l_run;
        unsigned short* op = p.out + b * p.o_bs + static_cast<long>(q0 + ql) * p.o_ld + h * D;
#pragma unroll
        for (int d = 0; d < DT; ++d) {
            u16x4 w;
#pragma unroll
            for (int r = 0; r < 4; ++r) w[r] = from_f32<T>(o[d][r] * inv);
            *reinterpret_cast<u16x4*>(op + d * 16 + 4 * g) = w;
        }
    }
}

template <typename T, int D>
static pf_status launch_wide(const WideParams& p, unsigned blocks, hipStream_t st) {
    static std::atomic<unsigned long long> done{0};
    constexpr size_t lds = wide_lds_bytes(D);
    const pf_status s = allow_dynamic_lds(reinterpret_cast<const void*>(k_attention_wide<T, D>), lds, done, "pf_attention_wide");
    if (s != PF_OK) return s;
    hipLaunchKernelGGL((k_attention_wide<T, D>), dim3(blocks), dim3(256), lds, st, p);
    return PF_OK;
}

}  // namespace pf

using namespace pf;

extern "C" pf_status pf_attention_wide(const pf_attn_desc* d, void* stream) {
    const pf_status v = validate_attn_desc(d, "pf_attention_wide");
    if (v != PF_OK) return v;
    PF_REQUIRE(d->D == 128 || d->D == 256 || d->D == 512, "pf_attention_wide: head dim %d unsupported (128, 256 or 512)", d->D);
    PF_REQUIRE(!d->bias && !d->flags, "pf_attention_wide: bias and flags must be NULL (no bias at wide heads)");
    PF_REQUIRE(!d->lse, "pf_attention_wide: lse must be NULL (no backward at wide heads)");
    PF_REQUIRE(!d->workspace, "pf_attention_wide: workspace must be NULL (no key-range split at wide heads)");
    // The kernel addresses K and V^T with 31-bit byte offsets inside one (batch, head) slice (batch strides are 64-bit), and its grid is 1-D.
    PF_REQUIRE((static_cast<long>(d->nk) + 64) * d->k_ld * 2 < (1L << 31) && static_cast<long>(d->D) * d->vt_ld * 2 < (1L << 31),
               "pf_attention_wide: per-batch operand too large: (nk + 64) * k_ld * 2 = %ld and D * vt_ld * 2 = %ld bytes must stay under 2^31",
               (static_cast<long>(d->nk) + 64) * d->k_ld * 2, static_cast<long>(d->D) * d->vt_ld * 2);
    const long blocks = cdiv(d->nq, 64) * d->H * d->B;
    PF_REQUIRE(blocks < (1L << 31) && d->nq <= 0x7FFFFFFF - 64,
               "pf_attention_wide: ceil(nq / 64) * H * B = %ld workgroups exceed the 1-D grid (2^31 - 1)", blocks);
    WideParams p;
    attn_operands(d, p);
    p.v16 = d->vt_ld % 8 == 0 && d->vt_bs % 8 == 0;
    hipStream_t st = as_stream(stream);
    pf_status s = PF_OK;
    PF_DISPATCH_16(d->dtype, "pf_attention_wide",
        if (d->D == 512) s = launch_wide<T, 512>(p, static_cast<unsigned>(blocks), st);
        else if (d->D == 256) s = launch_wide<T, 256>(p, static_cast<unsigned>(blocks), st);
        else s = launch_wide<T, 128>(p, static_cast<unsigned>(blocks), st));
    if (s != PF_OK) return s;
    PF_CHECK_LAUNCH("pf_attention_wide");
    return PF_OK;
}
