// MFMA GEMM / implicit-GEMM convolution for gfx950 (CDNA4).
//
//   out[m][n] = sum_k A[m][k] * W[n][k]  (+ bias[n]) (+ rowvec[img(m)][n]) (+ residual[m][n])
//
// A is never materialised for convolutions: row m = (image, yo, xo) and K-block kb = (tap, 64
// channels) address 128 contiguous bytes of the NHWC activation (zero padding, optional nearest
// x2 upsampling, optional channel concat of two sources are folded into the address).
//
// Two tile kernels share the fragment mapping, the LDS image and the block epilogue:
//   k_conv_gemm   256 threads = 4 wavefronts (2 x 2), tile (32*MREP) x (32*NREP), two LDS slots, 2 blocks per CU;
//   k_conv_gemm8  512 threads = 8 wavefronts (4 x 2), tile 256 x (32*NREP), three LDS slots, persistent over tiles.
// K-step 64, v_mfma_f32_16x16x32 (bf16 or f16) with fp32 accumulation.  The weight tile is the MFMA "A"
// operand and the activation tile the "B" operand, so every lane ends up with 4 CONSECUTIVE output channels
// of one output row (float4 bias loads, 8-byte LDS staging writes).  Operands go global -> LDS by LDS-DMA
// (buffer_load_dwordx4 ... lds) through scalar buffer descriptors: zero padding and ragged tiles are offsets
// beyond num_records.  LDS rows are 128 B; the 16-byte chunk index is XOR-swizzled with (row>>1)&7 (applied to
// the per-lane SOURCE offset, the DMA writes lane-linear), which makes the ds_read_b128 fragment reads conflict
// free.  Tile ids are remapped so that the tiles sharing an activation row-panel run on one XCD (private L2).
// Epilogue (epilogue_fast): bias / per-image row vector / residual / GEGLU on the fp32 accumulators, one
// rounding, 16-bit tile staged through LDS and written as whole 16-byte row segments.
//
// Replaces cuDNN / cuBLAS behind diffusers Conv2d / Linear (reference call sites
// models/pano/MVGenModel.py:86-144,174-198,224-294; models/modules/transformer.py:8-74).
#include "pf_common.h"
#include "pf_gemm_params.h"
#include "pf_gemm_walk.h"
#include <stdlib.h>
#include <algorithm>
#include <atomic>
#include <type_traits>

namespace pf {


template <typename T> struct Mfma;
template <> struct Mfma<Bf16> {
    typedef __attribute__((ext_vector_type(8))) __bf16 frag;
    static __device__ __forceinline__ f32x4 run(frag a, frag b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
    // accumulate IN PLACE in the AGPR half of the register file (one wave per SIMD, > 256 registers):
    // with the builtin hipcc copies every AGPR accumulator to a temporary before each MFMA
    static __device__ __forceinline__ void acc_agpr(frag a, frag b, f32x4& c) {
        asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
    }
};
template <> struct Mfma<F16> {
    typedef __attribute__((ext_vector_type(8))) _Float16 frag;
    static __device__ __forceinline__ f32x4 run(frag a, frag b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ void acc_agpr(frag a, frag b, f32x4& c) {
        asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
    }
};

__device__ __forceinline__ int lds_off(int row, int chunk) {   // in 16-bit elements
    return row * 64 + ((chunk ^ ((row >> 1) & 7)) << 3);
}


// GroupNorm moments of the layer's OUTPUT as a by-product of the epilogue (the consumer's statistics pass re-read
// the whole tensor: 210 MB per fp32 stream tensor at 64 x 64 x 320 x 40 views).  A lane holds 4 consecutive
// columns of the rows (lane & 15) + 16 i of its wavefront's fragment rows: per-lane sums over i, then an
// all-reduce over the 16 lanes of a DPP row (row_ror 8 / 4 / 2 / 1: VALU only, no LDS), and lane 0 of every row
// writes its 4 columns.  One partial row per (wavefront row group): [part][2][N], part = first row / gn_rows --
// fixed summation order, no atomics: results do not depend on scheduling.
__device__ __forceinline__ float row16_allreduce(float v) {
#define PF_ROR(n) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x120 + (n), 0xF, 0xF, false))
    v += PF_ROR(8);
    v += PF_ROR(4);
    v += PF_ROR(2);
    v += PF_ROR(1);
#undef PF_ROR
    return v;
}
// Moments are kept per column PAIR (2 c, 2 c + 1): every GroupNorm group of the UNets / VAE has an even number of channels
// and pairs never straddle a group.  They are computed in a phase of their own BEFORE the block epilogue, column block by
// column block, while nothing but the accumulators is live -- folded into the epilogue's own loops the 20 + 20 running sums
// pushed the 8-wave kernel from 244 registers into scratch, and every reload drained the DMA queue of the next tile
// (K loop + 15 %, epilogue x 1.8: profiles/archive/r3c_gemm_gn.txt).  The phase re-reads the tile's residual (the epilogue proper
// reads it again, from L2); bias and the image's time-embedding row are one float4 each per column block -- an image is
// whole runs of gn_rows rows (gn_rows_for), so a wavefront's rows belong to ONE image.
template <typename T, int MREP, int NREP, int RES>            // RES: 0 none, 1 fp32 residual, 2 16-bit residual
__device__ __forceinline__ void gn_moments_phase_r(const GemmParams& p, long bz, const f32x4 (&acc)[MREP][NREP],
                                                   int m0, int n0, int row_base, int col_base, int lane) {
    const int cq4 = 4 * (lane >> 4), rl = lane & 15;
    const int NP = p.N >> 1;
    const int mw = m0 + row_base;                                 // first row of this wavefront
    if (mw >= p.M) return;
    float* base = p.gn_partial + gn_part(p, bz, mw) * 2 * NP;
    const float* rv = p.rowvec ? p.rowvec + static_cast<long>(mw / p.rows_per_img) * p.rowvec_ld : nullptr;
    const int nb = n0 + col_base + cq4;                           // (whole N tiles: gn_rows_for) column of block j: nb + 16 j
    // operands are requested in batches (a few memory latencies for the whole phase, not one per column block): bias + row
    // vector of all column blocks first, then the residual of HALF the fragment rows at a time (40 registers; all 80 at once
    // sent the kernel back to scratch)
    float4 c[NREP];
#pragma unroll
    for (int j = 0; j < NREP; ++j) {
        c[j] = p.bias ? *reinterpret_cast<const float4*>(p.bias + nb + 16 * j) : float4{0.f, 0.f, 0.f, 0.f};
        if (rv) {
            const float4 r = *reinterpret_cast<const float4*>(rv + nb + 16 * j);
            c[j].x += r.x; c[j].y += r.y; c[j].z += r.z; c[j].w += r.w;
        }
    }
    constexpr bool res32 = RES == 1, res16 = RES == 2;
    float sm[NREP][2], sq[NREP][2];
#pragma unroll
    for (int j = 0; j < NREP; ++j) { sm[j][0] = sm[j][1] = 0.f; sq[j][0] = sq[j][1] = 0.f; }
    constexpr int HR = MREP >= 2 ? MREP / 2 : 1;                  // fragment rows per batch
#pragma unroll
    for (int i0 = 0; i0 < MREP; i0 += HR) {
        float4 r32[res32 ? HR : 1][NREP];
        u16x4 r16[res16 ? HR : 1][NREP];
        if constexpr (res32) {
#pragma unroll
            for (int ii = 0; ii < HR; ++ii) {
                const float* rp = static_cast<const float*>(p.residual) + bz * p.res_bs + static_cast<long>(min(mw + (i0 + ii) * 16 + rl, p.M - 1)) * p.res_ld + nb;
#pragma unroll
                for (int j = 0; j < NREP; ++j) r32[ii][j] = *reinterpret_cast<const float4*>(rp + 16 * j);
            }
        } else if constexpr (res16) {
#pragma unroll
            for (int ii = 0; ii < HR; ++ii) {
                const unsigned short* rp = static_cast<const unsigned short*>(p.residual) + bz * p.res_bs + static_cast<long>(min(mw + (i0 + ii) * 16 + rl, p.M - 1)) * p.res_ld + nb;
#pragma unroll
                for (int j = 0; j < NREP; ++j) r16[ii][j] = *reinterpret_cast<const u16x4*>(rp + 16 * j);
            }
        }
#pragma unroll
        for (int ii = 0; ii < HR; ++ii) {
            const int i = i0 + ii;
            const float live = mw + i * 16 + rl < p.M ? 1.f : 0.f;        // (rows past M: clamped copies)
#pragma unroll
            for (int j = 0; j < NREP; ++j) {
                float x0 = acc[i][j][0] + c[j].x, x1 = acc[i][j][1] + c[j].y, x2 = acc[i][j][2] + c[j].z, x3 = acc[i][j][3] + c[j].w;
                if constexpr (res32) { x0 += r32[ii][j].x; x1 += r32[ii][j].y; x2 += r32[ii][j].z; x3 += r32[ii][j].w; }
                else if constexpr (res16) { x0 += to_f32<T>(r16[ii][j][0]); x1 += to_f32<T>(r16[ii][j][1]); x2 += to_f32<T>(r16[ii][j][2]); x3 += to_f32<T>(r16[ii][j][3]); }
                x0 *= live; x1 *= live; x2 *= live; x3 *= live;
                sm[j][0] += x0 + x1; sm[j][1] += x2 + x3;
                sq[j][0] += x0 * x0 + x1 * x1; sq[j][1] += x2 * x2 + x3 * x3;
            }
        }
        __builtin_amdgcn_sched_barrier(0);                        // (one batch of residual registers at a time)
    }
#pragma unroll
    for (int j = 0; j < NREP; ++j) {
        const float s0 = row16_allreduce(sm[j][0]), s1 = row16_allreduce(sm[j][1]);
        const float q0 = row16_allreduce(sq[j][0]), q1 = row16_allreduce(sq[j][1]);
        if (rl == 0) {
            *reinterpret_cast<float2*>(base + ((nb + 16 * j) >> 1)) = float2{s0, s1};
            *reinterpret_cast<float2*>(base + NP + ((nb + 16 * j) >> 1)) = float2{q0, q1};
        }
    }
}

template <typename T, int MREP, int NREP>
__device__ __forceinline__ void gn_moments_phase(const GemmParams& p, long bz, const f32x4 (&acc)[MREP][NREP],
                                                 int m0, int n0, int row_base, int col_base, int lane) {
    if (!p.residual) gn_moments_phase_r<T, MREP, NREP, 0>(p, bz, acc, m0, n0, row_base, col_base, lane);
    else if (p.res_f32) gn_moments_phase_r<T, MREP, NREP, 1>(p, bz, acc, m0, n0, row_base, col_base, lane);
    else gn_moments_phase_r<T, MREP, NREP, 2>(p, bz, acc, m0, n0, row_base, col_base, lane);
}

// Block epilogue.  All arithmetic (bias, per-image row vector, residual, GEGLU) runs in the MFMA
// fragment layout on the fp32 accumulators -- one rounding to 16 bit -- and the finished 16-bit tile is
// staged through LDS so that it leaves as whole 16-byte row segments (a fragment store touches 16
// different rows with 8 bytes each).  fp32 output, ragged N or an unaligned out_ld take the direct
// per-fragment store.  smem16: the block's LDS (the operand ring is dead after the K loop).
// Staged block epilogue, specialised at compile time for the operand mix of the layer (MODE):
//   0 bias | 1 bias + per-image row vector (time embedding) | 2 bias + residual | 3 bias + GEGLU pairing.
// Straight-line code: rows beyond M / quads beyond N are CLAMPED to the last valid one instead of being
// predicated (their results are dropped by the bounds check of the copy-out), the operands of two
// 16-row fragment groups are requested one group ahead of the arithmetic, and nothing in the loop
// waits for memory more than once per group.  The finished 16-bit tile goes through LDS in HALVES row
// slices (every wave stages MREP / HALVES of its fragment rows per slice) and leaves as 16-byte row segments.
template <typename T, int MREP, int NREP, int NT, int BM, int BN, int HALVES, int MODE>
__device__ __forceinline__ void epilogue_fast(const GemmParams& p, long bz, f32x4 (&acc)[MREP][NREP], unsigned short* smem16,
                                              int m0, int n0, int row_base, int col_base, int lane, int t) {
    constexpr int SLD = (MODE == 3 ? BN / 2 : BN) + 8;            // 16-bit elements per staged row (GEGLU: half as many columns)
    constexpr int BMH = BM / HALVES;                              // staged rows per slice
    constexpr int WR = 16 * MREP, WRH = WR / HALVES, IH = MREP / HALVES;
    constexpr int G = 2, NG = MREP / G;                           // fragment rows per operand group
    static_assert(MREP % HALVES == 0 && IH % G == 0, "slices are whole operand groups");
    const int cq = 4 * (lane >> 4), rl = lane & 15;
    const int n_store = MODE == 3 ? p.N >> 1 : p.N;
    int ncl[NREP];
#pragma unroll
    for (int j = 0; j < NREP; ++j) ncl[j] = min(n0 + col_base + j * 16 + cq, p.N - 4);
    float4 bias[NREP];
#pragma unroll
    for (int j = 0; j < NREP; ++j) bias[j] = float4{0.f, 0.f, 0.f, 0.f};
    if (p.bias) {
#pragma unroll
        for (int j = 0; j < NREP; ++j) bias[j] = *reinterpret_cast<const float4*>(p.bias + ncl[j]);
    }
    const unsigned short* resp = MODE == 2 ? static_cast<const unsigned short*>(p.residual) + bz * p.res_bs : nullptr;
    // MODE 1 (requires rows_per_img >= BM: the tile touches two images at most): both candidate row
    // vectors are fetched up front, a row picks one by comparing its offset with the image boundary
    float4 rv0[NREP], rv1[NREP];
    int boundary = 0;                                             // first tile row of the second image
    if (MODE == 1) {
        const int img0 = m0 / p.rows_per_img, img_last = (p.M - 1) / p.rows_per_img;
        boundary = (img0 + 1) * p.rows_per_img - m0;
        const float* r0 = p.rowvec + static_cast<long>(img0) * p.rowvec_ld;
        const float* r1 = p.rowvec + static_cast<long>(min(img0 + 1, img_last)) * p.rowvec_ld;
#pragma unroll
        for (int j = 0; j < NREP; ++j) {
            rv0[j] = *reinterpret_cast<const float4*>(r0 + ncl[j]);
            rv1[j] = *reinterpret_cast<const float4*>(r1 + ncl[j]);
        }
    }
    u16x4 res[2][G][NREP];                                        // residual, requested one group ahead (MODE 2)
    auto request = [&](auto g_tag, auto buf_tag) __attribute__((always_inline)) {
        constexpr int g = decltype(g_tag)::value, bf = decltype(buf_tag)::value;
        if (MODE != 2) return;
#pragma unroll
        for (int ii = 0; ii < G; ++ii) {
            const int mc = min(m0 + row_base + (g * G + ii) * 16 + rl, p.M - 1);
            const unsigned short* rp = resp + static_cast<long>(mc) * p.res_ld;
#pragma unroll
            for (int j = 0; j < NREP; ++j) res[bf][ii][j] = *reinterpret_cast<const u16x4*>(rp + ncl[j]);
        }
    };
    auto arithmetic = [&](auto g_tag, auto buf_tag) __attribute__((always_inline)) {
        constexpr int g = decltype(g_tag)::value, bf = decltype(buf_tag)::value;
#pragma unroll
        for (int ii = 0; ii < G; ++ii) {
            constexpr int i0 = g * G;
            const int i = i0 + ii, h = i0 / IH;
            const int r = row_base / HALVES + (i - h * IH) * 16 + rl;         // staged row <-> tile row row_base + i*16 + rl
#pragma unroll
            for (int j = 0; j < NREP; ++j) {
                const int c = col_base + j * 16 + cq;
                float v[4] = {acc[i][j][0] + bias[j].x, acc[i][j][1] + bias[j].y, acc[i][j][2] + bias[j].z, acc[i][j][3] + bias[j].w};
                if (MODE == 1) {
                    const bool second = row_base + i * 16 + rl >= boundary;
                    v[0] += second ? rv1[j].x : rv0[j].x; v[1] += second ? rv1[j].y : rv0[j].y;
                    v[2] += second ? rv1[j].z : rv0[j].z; v[3] += second ? rv1[j].w : rv0[j].w;
                }
                if (MODE == 2) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] += to_f32<T>(res[bf][ii][j][e]);
                }
                if (MODE == 3) {
                    typedef __attribute__((ext_vector_type(2))) unsigned short u16x2;
                    u16x2 w2;
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const float gt = v[2 * e + 1];
                        w2[e] = from_f32<T>(geglu_value(v[2 * e], gt));
                    }
                    *reinterpret_cast<u16x2*>(smem16 + r * SLD + (c >> 1)) = w2;
                } else {
                    u16x4 w4;
#pragma unroll
                    for (int e = 0; e < 4; ++e) w4[e] = from_f32<T>(v[e]);
                    *reinterpret_cast<u16x4*>(smem16 + r * SLD + c) = w4;
                }
            }
        }
    };
    unsigned short* outp = static_cast<unsigned short*>(p.out) + bz * p.out_bs;
    auto copy_out = [&](int h) __attribute__((always_inline)) {
        constexpr int CPR = MODE == 3 ? BN / 16 : BN / 8;         // 16-byte chunks per tile row
        const int nbase = MODE == 3 ? n0 >> 1 : n0;
#pragma unroll
        for (int k = 0; k < (BMH * CPR + NT - 1) / NT; ++k) {
            const int q = t + k * NT, r = q / CPR, c8 = (q - r * CPR) * 8;
            const int m = m0 + (r / WRH) * WR + h * WRH + r % WRH;
            if (q < BMH * CPR && m < p.M && nbase + c8 < n_store) {
                const u16x8 x = *reinterpret_cast<const u16x8*>(smem16 + r * SLD + c8);
                *reinterpret_cast<u16x8*>(outp + out_row(p, bz, m) * p.out_ld + nbase + c8) = x;
            }
        }
    };
    auto group = [&](auto g_tag) __attribute__((always_inline)) {
        constexpr int g = decltype(g_tag)::value;
        if constexpr (g + 1 < NG) request(std::integral_constant<int, g + 1>(), std::integral_constant<int, (g + 1) & 1>());
        arithmetic(g_tag, std::integral_constant<int, g & 1>());
        if constexpr (((g + 1) * G) % IH == 0) {                  // slice complete
            constexpr int h = (g * G) / IH;
            stamp(p, 6 + 3 * h);
            __syncthreads();
            stamp(p, 7 + 3 * h);
            copy_out(h);
            stamp(p, 8 + 3 * h);
            if constexpr (h + 1 < HALVES) __syncthreads();        // slice read out before the next one is staged
        }
    };
    request(std::integral_constant<int, 0>(), std::integral_constant<int, 0>());
    group(std::integral_constant<int, 0>());
    if constexpr (NG > 1) group(std::integral_constant<int, 1>());
    if constexpr (NG > 2) group(std::integral_constant<int, 2>());
    if constexpr (NG > 3) group(std::integral_constant<int, 3>());
    static_assert(NG <= 4, "unrolled by hand");
}

// fp32 block epilogue of the mixed-precision scheme (the residual stream is fp32): bias (+ fp32 residual)
// on the accumulators, stored straight from the fragments -- a lane owns 4 consecutive fp32 columns
// (16 bytes), the four column groups of a fragment make a 64-byte row segment, so no LDS staging is
// needed.  Straight-line like epilogue_fast: rows / quads beyond the edge are clamped for the loads and
// only the store is predicated; the residual of a group of two fragment rows is requested one group ahead.
template <typename T, int MREP, int NREP, bool RES, bool PAIR = false>
__device__ __forceinline__ void epilogue_f32(const GemmParams& p, long bz, f32x4 (&acc)[MREP][NREP],
                                             int m0, int n0, int row_base, int col_base, int lane) {
    constexpr int G = 1, NG = MREP / G;                           // (two fp32 row groups in flight would spill)
    const int cq = 4 * (lane >> 4), rl = lane & 15;
    int ncl[NREP];
    bool nok[NREP];
#pragma unroll
    for (int j = 0; j < NREP; ++j) {
        const int n4 = n0 + col_base + j * 16 + cq;
        nok[j] = n4 < p.N;
        ncl[j] = min(n4, p.N - 4);
    }
    float4 bias[NREP];
#pragma unroll
    for (int j = 0; j < NREP; ++j) bias[j] = float4{0.f, 0.f, 0.f, 0.f};
    if (p.bias) {
#pragma unroll
        for (int j = 0; j < NREP; ++j) bias[j] = *reinterpret_cast<const float4*>(p.bias + ncl[j]);
    }
    const float* resp = RES ? static_cast<const float*>(p.residual) + bz * p.res_bs : nullptr;
    float* outp = static_cast<float*>(p.out) + bz * p.out_bs;
    unsigned short* outp16 = static_cast<unsigned short*>(p.out) + bz * p.out_bs;    // PAIR: [M][per 32 columns: hi(32) | lo(32)] 16-bit
    float4 res[2][G][NREP];
    auto request = [&](int g, int bf) __attribute__((always_inline)) {
        if (!RES) return;
#pragma unroll
        for (int ii = 0; ii < G; ++ii) {
            const int mc = min(m0 + row_base + (g * G + ii) * 16 + rl, p.M - 1);
            const float* rp = resp + static_cast<long>(mc) * p.res_ld;
#pragma unroll
            for (int j = 0; j < NREP; ++j) res[bf][ii][j] = *reinterpret_cast<const float4*>(rp + ncl[j]);
        }
    };
    request(0, 0);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        if (g + 1 < NG) request(g + 1, (g + 1) & 1);
#pragma unroll
        for (int ii = 0; ii < G; ++ii) {
            const int i = g * G + ii;
            const int m = m0 + row_base + i * 16 + rl;
            float* op = outp + out_row(p, bz, min(m, p.M - 1)) * p.out_ld;
#pragma unroll
            for (int j = 0; j < NREP; ++j) {
                float4 v = float4{acc[i][j][0] + bias[j].x, acc[i][j][1] + bias[j].y, acc[i][j][2] + bias[j].z, acc[i][j][3] + bias[j].w};
                if (RES) {
                    const float4 r = res[g & 1][ii][j];
                    v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
                }
                if (PAIR) {
                    if (m < p.M && nok[j]) {
                        unsigned short* o16 = outp16 + out_row(p, bz, m) * p.out_ld + pair_off(ncl[j]);
                        const float f[4] = {v.x, v.y, v.z, v.w};
                        u16x4 hi, lo;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            hi[e] = from_f32<T>(f[e]);
                            lo[e] = from_f32<T>(f[e] - to_f32<T>(hi[e]));
                        }
                        *reinterpret_cast<u16x4*>(o16) = hi;
                        *reinterpret_cast<u16x4*>(o16 + 32) = lo;
                    }
                } else if (m < p.M && nok[j]) *reinterpret_cast<float4*>(op + ncl[j]) = v;
            }
        }
    }
}

// fp32 tile WITH the GroupNorm moments of the finished output (bias + residual included) from the same registers: column block by
// column block (j outermost), so that only the 4 running sums of ONE block are live next to the two residual buffers (4 fragment rows
// each: 32 registers against the 40 of epilogue_f32; 256 registers, no scratch) -- the separate moment phase above has to read the
// residual tile a second time, which cost a residual layer as much as the consumer's statistics pass saves
// (profiles/archive/r3d_gemm_gn.txt).  (Row group by row group with all 20 sums live -- the store order of epilogue_f32 -- spills 10-73
// registers in the persistent kernel, whichever way the bias and the residual buffer are arranged.)  Whole N tiles (gn_rows_for);
// rows past M are clamped and masked.
template <typename T, int MREP, int NREP, bool RES>
__device__ __forceinline__ void epilogue_f32_stats(const GemmParams& p, long bz, f32x4 (&acc)[MREP][NREP],
                                                   int m0, int n0, int row_base, int col_base, int lane) {
    const int cq = 4 * (lane >> 4), rl = lane & 15;
    const int NP = p.N >> 1;
    const int mw = m0 + row_base;                                 // first row of this wavefront
    if (mw >= p.M) return;
    float* base = p.gn_partial + gn_part(p, bz, mw) * 2 * NP;
    const float* resp = RES ? static_cast<const float*>(p.residual) + bz * p.res_bs : nullptr;
    float* outp = static_cast<float*>(p.out) + bz * p.out_bs;
    const int nb = n0 + col_base + cq;
    float4 res[2][MREP];
    auto request = [&](int j, int bf) __attribute__((always_inline)) {
        if (!RES) return;
#pragma unroll
        for (int i = 0; i < MREP; ++i)
            res[bf][i] = *reinterpret_cast<const float4*>(resp + static_cast<long>(min(mw + i * 16 + rl, p.M - 1)) * p.res_ld + nb + 16 * j);
    };
    request(0, 0);
#pragma unroll
    for (int j = 0; j < NREP; ++j) {
        if (j + 1 < NREP) request(j + 1, (j + 1) & 1);
        const float4 b = p.bias ? *reinterpret_cast<const float4*>(p.bias + nb + 16 * j) : float4{0.f, 0.f, 0.f, 0.f};
        float s0 = 0.f, s1 = 0.f, q0 = 0.f, q1 = 0.f;
#pragma unroll
        for (int i = 0; i < MREP; ++i) {
            const int m = mw + i * 16 + rl;
            float4 v = float4{acc[i][j][0] + b.x, acc[i][j][1] + b.y, acc[i][j][2] + b.z, acc[i][j][3] + b.w};
            if (RES) {
                const float4 r = res[j & 1][i];
                v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
            }
            const bool live = m < p.M;
            if (live) *reinterpret_cast<float4*>(outp + static_cast<long>(m) * p.out_ld + nb + 16 * j) = v;
            const float lf = live ? 1.f : 0.f;
            v.x *= lf; v.y *= lf; v.z *= lf; v.w *= lf;
            s0 += v.x + v.y; s1 += v.z + v.w;
            q0 += v.x * v.x + v.y * v.y; q1 += v.z * v.z + v.w * v.w;
        }
        s0 = row16_allreduce(s0); s1 = row16_allreduce(s1);
        q0 = row16_allreduce(q0); q1 = row16_allreduce(q1);
        if (rl == 0) {
            *reinterpret_cast<float2*>(base + ((nb + 16 * j) >> 1)) = float2{s0, s1};
            *reinterpret_cast<float2*>(base + NP + ((nb + 16 * j) >> 1)) = float2{q0, q1};
        }
    }
}

// Block epilogue.  All arithmetic (bias, per-image row vector, residual, GEGLU) runs in the MFMA
// fragment layout on the fp32 accumulators -- one rounding to 16 bit.  16-bit outputs with 16-byte
// aligned rows take one of the staged specialisations above; everything else (fp32 output, ragged or
// unaligned rows, row vector AND residual together) takes the per-fragment store.  smem16: the LDS
// region the staged tile may use.  HALVES > 1: staged in row slices through a smaller region;
// after_ring() runs right after the barrier that retires the operand ring -- the persistent kernel
// requests the next tile's first stages there, into ring slots the staging region does not overlap.
template <typename T, int MREP, int NREP, int NT, int BM, int BN, int HALVES = 1, bool STATS = false, typename F = NoOp>
__device__ __forceinline__ void epilogue_tile(const GemmParams& p, long bz, f32x4 (&acc)[MREP][NREP],
                                              unsigned short* smem16, int m0, int n0, int row_base, int col_base,
                                              int lane, int t, F after_ring = F()) {
    if constexpr (STATS) {
        // GroupNorm-moment instantiation of the kernel (pf_conv_desc.gn_partial; a separate instantiation so that the
        // default kernels keep their code and register allocation untouched).  Ahead of the ring barrier and of the next
        // tile's DMA requests: the phase's own loads would otherwise queue behind them in vmcnt order (it cost 8 k clocks
        // per tile there), and the waves that arrive early spend their barrier wait on it.
        // (fp32 tiles with an fp32 residual produce their moments inside the store loop instead: epilogue_f32_stats)
        if (!(p.out_f32 && p.residual)) gn_moments_phase<T, MREP, NREP>(p, bz, acc, m0, n0, row_base, col_base, lane);
        __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();                                              // every wave is done reading the operand ring
    stamp(p, 4);
    after_ring();
    stamp(p, 5);
    if constexpr (STATS) {
        if (p.out_f32 && p.residual) {                            // (gn_rows_for admitted it: fp32 residual, aligned rows, no row vector)
            epilogue_f32_stats<T, MREP, NREP, true>(p, bz, acc, m0, n0, row_base, col_base, lane);
            return;
        }
    }
    const int n_store = p.geglu ? p.N >> 1 : p.N;
    if (p.split_out && !p.rowvec && (p.N & 3) == 0 && (p.out_ld & 3) == 0 && p.N >= 4) {
        if (!p.residual) { epilogue_f32<T, MREP, NREP, false, true>(p, bz, acc, m0, n0, row_base, col_base, lane); return; }
        if (p.res_f32 && (p.res_ld & 3) == 0) { epilogue_f32<T, MREP, NREP, true, true>(p, bz, acc, m0, n0, row_base, col_base, lane); return; }
    }
    if (p.out_f32 && !p.geglu && !p.rowvec && (p.N & 3) == 0 && (p.out_ld & 3) == 0 && p.N >= 4) {
        if (!p.residual) { epilogue_f32<T, MREP, NREP, false>(p, bz, acc, m0, n0, row_base, col_base, lane); return; }
        if (p.res_f32 && (p.res_ld & 3) == 0) { epilogue_f32<T, MREP, NREP, true>(p, bz, acc, m0, n0, row_base, col_base, lane); return; }
    }
    const bool staged = !p.out_f32 && !p.res_f32 && !p.split_out && (p.out_ld & 7) == 0 && (n_store & 7) == 0 && (p.N & 3) == 0;
    if (staged && !(p.rowvec && p.residual) && !(p.geglu && (p.rowvec || p.residual))) {
        // GEGLU halves the columns: the whole 256 x 80 tile fits the staging slot at once -- one barrier pair instead of two
        // (the FF1 tile of a K = 320 layer spends 3 x 1.2 k of its 24.6 k clocks waiting at them)
        if (p.geglu) epilogue_fast<T, MREP, NREP, NT, BM, BN, 1, 3>(p, bz, acc, smem16, m0, n0, row_base, col_base, lane, t);
        else if (p.rowvec && p.rows_per_img < BM) goto generic;
        else if (p.rowvec) epilogue_fast<T, MREP, NREP, NT, BM, BN, HALVES, 1>(p, bz, acc, smem16, m0, n0, row_base, col_base, lane, t);
        else if (p.residual) epilogue_fast<T, MREP, NREP, NT, BM, BN, HALVES, 2>(p, bz, acc, smem16, m0, n0, row_base, col_base, lane, t);
        else epilogue_fast<T, MREP, NREP, NT, BM, BN, HALVES, 0>(p, bz, acc, smem16, m0, n0, row_base, col_base, lane, t);
        return;
    }
generic:
    const int cq = 4 * (lane >> 4), rl = lane & 15;
#pragma unroll
    for (int i = 0; i < MREP; ++i) {
        const int m = m0 + row_base + i * 16 + rl;
#pragma unroll
        for (int j = 0; j < NREP; ++j) {
            const int n4 = n0 + col_base + j * 16 + cq;
            float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
            if (m < p.M && n4 < p.N) epilogue_store<T>(p, bz, m, n4, v);
        }
    }
}

// Split-K combine INSIDE the GEMM launch (no second kernel: the 8 x 8 / 16 x 16 levels and the whole panorama branch paid
// one ~8 us launch per split layer, 200+ per step, most of them on the latency-bound chains the branch joins wait for).
// Every K-slice block publishes its fp32 slab and draws a ticket; the block that draws the last one combines the slabs IN
// SPLIT ORDER (the same sums as k_splitk_reduce: results do not depend on arrival order) and runs the epilogue.
// Inter-workgroup visibility (cdna_hip_programming.md section 6 Guideline 16, write-through form): sc1 slab stores ->
// s_waitcnt vmcnt(0) in every wave -> barrier -> lane 0: relaxed agent-scope fetch_add; the last arriver: lane 0
// agent-scope acquire fence (drops this CU's L1) -> barrier -> plain loads.  Nobody waits for anybody:
// no residency assumption, no deadlock.  The last arriver zeroes the counter for the next launch that is handed the slot.

template <typename T, int BM, int BN, int NT>
__device__ __forceinline__ void splitk_finish(const GemmParams& p, long bz, int tile_lin, int m0, int n0, int* flag, int t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // this wave's slab stores have left the wave
    __syncthreads();                                              // (also: every wave is done with the operand ring -> `flag` may live there)
    int* ticket = p.tickets + (bz * p.mtiles * p.ntiles + tile_lin);
    if (t == 0) {                                                 // (write-through slabs + drained stores: no release fence)
        const int drawn = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *flag = drawn == p.splits - 1 ? 1 : 0;
    }
    __syncthreads();
    const bool last = *flag != 0;
    __syncthreads();                                              // (flag read by everyone before the ring is reused)
    if (!last) return;
    if (t == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    __syncthreads();
    constexpr int QPR = BN / 4;
    const int Ms = p.M - p.m_begin;
    const long slab = static_cast<long>(p.batch) * Ms * p.N;
    for (int q = t; q < BM * QPR; q += NT) {
        const int r = q / QPR, m = m0 + r, n4 = n0 + (q - r * QPR) * 4;
        if (m >= p.M || n4 >= p.N) continue;
        const float* src = p.partial + (bz * Ms + (m - p.m_begin)) * p.N + n4;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < p.splits; ++s) {
            const float4 x = *reinterpret_cast<const float4*>(src + s * slab);
            v[0] += x.x; v[1] += x.y; v[2] += x.z; v[3] += x.w;
        }
        epilogue_store<T>(p, bz, m, n4, v);
    }
    if (t == 0) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// STAGES (round 6): ring depth.  2 = the original form, two blocks per CU, ONE K step of DMA look-ahead and a full drain per step -- every
// step then costs a whole L2 round trip (~1 us per 64-wide step measured on the panorama branch's small-M layers: M 1024 N 1280 K 1280
// ran 20 steps in 20.8 us, 0.1 of peak).  4 = one block per CU (115 KB), stage it+3 requested while stage it is multiplied and awaited with a
// COUNTED s_waitcnt that leaves the two younger stages in flight: the launch-latency-bound problems whose grid is one round of the chip
// anyway (180 launches per step; the floor of every sharded rank).
// A32 (pf_conv_desc.a_src_dtype = PF_F32; S3, two slots, 1x1): the activation operand is the fp32 stream itself.  Thread t owns the octet 8 (t & 3) of the
// rows (t >> 2) + 64 u of the tile: the 8 fp32 channels of K block it + 1 are requested into registers (buffer loads: rows past M read as zero -- with a_scale they become the image's shift; such rows are never stored and the moment phase masks them) in front of the
// weight DMA of that block, stay in flight during the MFMAs of block it, and become the two 16-byte pieces hi | lo (affine_f / split8, pf_common.h) that the
// DMA of the pair tensor would have put at lds_off(row, c4) and lds_off(row, c4 + 4) -- written behind the same full drain and in front of the same barrier
// that ends the step.  Fragment reads, MFMA order, split-K and every epilogue are the pair form's: the result is bit-identical.
// This kernel keeps its OWN copy of the operand walk (pf_gemm_walk.h serves k_conv_gemm8 and k_conv_gemm32): folded onto ConvWalk every 16-bit
// instantiation went from 0 to 4-15 spilled SGPRs (TotalSGPRs 79-96 -> 104-106, VGPRs + 1-5, one occupancy 3 -> 2), whichever way the rows, the bounds
// test, the tile remap, the inlining or the launch constants were spelled; with its own text the registers are the ones it always had.  A change to
// the walk is made in pf_gemm_walk.h AND here.  (Its uniform_ptr / lds_dma lambdas are part of that text and kept on purpose.)
template <typename T, int MREP, int NREP, bool STATS = false, bool S3 = false, int STAGES = 2, bool A32 = false>
__global__ __launch_bounds__(256, STAGES > 2 ? 1 : 2) void k_conv_gemm(const GemmParams p) {
    constexpr int BM = 32 * MREP, BN = 32 * NREP;
    static_assert(!A32 || (S3 && STAGES == 2 && MREP % 2 == 0), "fp32-source staging: split-precision walk, two slots");
    extern __shared__ __attribute__((aligned(16))) unsigned short smem[];
    unsigned short* As = smem;                       // [STAGES][BM][64]
    unsigned short* Bs = smem + STAGES * BM * 64;    // [STAGES][BN][64]

    // XCD-aware, bijective remap of the 1-D tile id (8 XCDs, block b runs on XCD b % 8).
    const int ntile_total = p.mtiles * p.ntiles;
    int tid_lin = blockIdx.x;
    {
        const int q = ntile_total / 8, r = ntile_total % 8;
        const int xcd = tid_lin % 8, idx = tid_lin / 8;
        tid_lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int tile_n = tid_lin % p.ntiles, tile_m = tid_lin / p.ntiles;
    const int m0 = p.m_begin + tile_m * BM, n0 = tile_n * BN;
    const long bz = blockIdx.z;
    const unsigned short* a0 = p.a0 + bz * p.a_bs;
    const unsigned short* a1 = p.a1 ? p.a1 + bz * p.a_bs : nullptr;
    const unsigned short* wg = p.w + bz * p.w_bs;

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    // staging ownership: global_load_lds_dwordx4 writes LDS at (wave-uniform base + 16 * lane), i.e.
    // lane l of wave w fills physical chunk l%8 of row 8w + l/8 of a 32-row pass.  The XOR swizzle
    // therefore moves to the SOURCE address: the lane fetches the logical chunk that belongs in its
    // physical slot (same 128-B row segment, coalescing intact).  (row>>1)&7 only depends on lrow.
    const int chunk = t & 7, lrow = t >> 3;
    const int lchunk8 = (chunk ^ ((lrow >> 1) & 7)) * 8;

    // per-thread staging rows: output pixel -> top-left input coordinate
    const int pad_y = p.subpix ? 1 - (static_cast<int>(bz) >> 1) : p.pad, pad_x = p.subpix ? 1 - (static_cast<int>(bz) & 1) : p.pad;   // (sub-pixel phase: pf_gemm_params.h)
    int a_img[MREP], a_y[MREP], a_x[MREP];
#pragma unroll
    for (int i = 0; i < MREP; ++i) {
        const int m = m0 + i * 32 + lrow;
        if (m < p.M) {
            const int img = m / p.rows_per_img, rem = m - img * p.rows_per_img;
            const int yo = rem / p.w_out;
            a_img[i] = img;
            a_y[i] = yo * p.stride - pad_y;
            a_x[i] = (rem - yo * p.w_out + p.crop) * p.stride - pad_x;
        } else {
            a_img[i] = 0; a_y[i] = -(1 << 20); a_x[i] = 0;     // never in range
        }
        if (p.fastseg) seg_pack(a_img[i], a_y[i], a_x[i], p.h_in, p.w_in);      // (pf_gemm_params.h: a_img = pixel index, a_y = validity bits from here on)
    }
    // DMA addressing as in k_conv_gemm8: scalar buffer descriptors + per-thread byte offset (VGPR) +
    // per-stage scalar offset; out-of-range offsets (zero padding, ragged tiles) read as zero.
    constexpr unsigned OOB = 0x80000000u;
    auto uniform_ptr = [](const unsigned short* ptr) {
        const unsigned long long v = reinterpret_cast<unsigned long long>(ptr);
        const unsigned lo = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(v));
        const unsigned hi = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(v >> 32));
        return reinterpret_cast<unsigned short*>(static_cast<unsigned long long>(lo) | (static_cast<unsigned long long>(hi) << 32));
    };
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(wg), 0, __builtin_amdgcn_readfirstlane(p.w_bytes), 0x00020000);
    unsigned w_off[NREP];                                         // bytes
#pragma unroll
    for (int j = 0; j < NREP; ++j) {
        const int n = n0 + j * 32 + lrow;
        w_off[j] = n < p.N ? static_cast<unsigned>(n * p.K + lchunk8) * 2u : OOB;
    }
    const int Ctot = p.c0 + p.c1;
    const int Hl = p.h_in << p.up, Wl = (p.w_in + 2 * p.wrap) << p.up;

    // K walk (wave-uniform state): K-block kb = (tap, source, 64-channel block); no divisions in the loop
    const int nkb = p.K / 64;
    const int kb0 = blockIdx.y * p.kb_per_split;
    const int kb1 = min(nkb, kb0 + p.kb_per_split);
    int kg = kb0 * 64;
    int tap = kg / Ctot, cc = kg - tap * Ctot;
    unsigned a_off[MREP];                                         // bytes, or OOB
    bool seg1 = false;
    auto set_segment = [&]() {
        const int ky = p.ksize == 3 ? tap / 3 : p.ksize == 2 ? tap >> 1 : 0, kx = p.ksize == 3 ? tap - 3 * ky : p.ksize == 2 ? tap & 1 : 0;
        seg1 = __builtin_amdgcn_readfirstlane(cc >= p.c0 ? 1 : 0) != 0;
        const int ld = seg1 ? p.a1_ld : p.a0_ld;
        if constexpr (A32) return;                                // (1x1: a row IS its pixel; a32_load addresses it)
        if (p.fastseg) {
            const unsigned sel = (1u << ky) | (16u << kx);
            const int tap_pix = ky * p.w_in + kx;
#pragma unroll
            for (int i = 0; i < MREP; ++i) {
                const unsigned off = ((static_cast<unsigned>(a_img[i]) + static_cast<unsigned>(tap_pix)) * static_cast<unsigned>(ld) + static_cast<unsigned>(lchunk8)) * 2u;
                a_off[i] = (static_cast<unsigned>(a_y[i]) & sel) == sel ? off : OOB;
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < MREP; ++i) {
            const int yi = a_y[i] + ky, xi = a_x[i] + kx;             // xi: column in the (virtually wrap-padded, upsampled) input
            const bool ok = yi >= 0 && yi < Hl && xi >= 0 && xi < Wl;
            int sx = (xi >> p.up) - p.wrap;                            // source column: the padding is circular
            sx += sx < 0 ? p.w_in : 0;
            sx -= sx >= p.w_in ? p.w_in : 0;
            const int pix = (a_img[i] * p.h_in + (yi >> p.up)) * p.w_in + sx;
            a_off[i] = ok ? static_cast<unsigned>(pix * ld + lchunk8) * 2u : OOB;
        }
    };
    set_segment();

    auto lds_dma = [&](const __amdgpu_buffer_rsrc_t& r, unsigned short* dst, unsigned voff, int soff) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)dst, 16, voff, soff, 0, 0);
    };
    // fp32-source staging (A32): registers of the K block in flight
    constexpr int NP32 = A32 ? MREP / 2 : 1;                      // octets per thread: BM rows x 4 octets over 256 threads
    const int c4 = t & 3, r32 = t >> 2;
    f32x4 xr[NP32][2], sr[NP32][2], hr[NP32][2];
    auto a32_load = [&](const __amdgpu_buffer_rsrc_t& rs_a, int soff_a) {
        const int ld = seg1 ? p.a1_ld : p.a0_ld;
#pragma unroll
        for (int u = 0; u < NP32; ++u) {
            const int m = m0 + 64 * u + r32;
            const unsigned voff = m < p.M ? (static_cast<unsigned>(m) * static_cast<unsigned>(ld) + 8u * c4) * 4u : OOB;
            xr[u][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_a, voff, soff_a, 0));
            xr[u][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_a, voff + 16u, soff_a, 0));
            if (p.a_scale) {
                const long so = static_cast<long>(min(m, p.M - 1) / p.rows_per_img) * (Ctot >> 1) + (cc >> 1) + 8 * c4;
                sr[u][0] = *reinterpret_cast<const f32x4*>(p.a_scale + so); sr[u][1] = *reinterpret_cast<const f32x4*>(p.a_scale + so + 4);
                hr[u][0] = *reinterpret_cast<const f32x4*>(p.a_shift + so); hr[u][1] = *reinterpret_cast<const f32x4*>(p.a_shift + so + 4);
            }
        }
    };
    auto a32_write = [&](int buf) {
#pragma unroll
        for (int u = 0; u < NP32; ++u) {
            float f[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = xr[u][j >> 2][j & 3];
            if (p.a_scale) {
#pragma unroll
                for (int j = 0; j < 8; ++j) f[j] = affine_f(f[j], sr[u][j >> 2][j & 3], hr[u][j >> 2][j & 3]);
            }
            u16x8 hi, lo;
            split8<T>(f, hi, lo);
            unsigned short* dst = As + buf * BM * 64;
            *reinterpret_cast<u16x8*>(dst + lds_off(64 * u + r32, c4)) = hi;
            *reinterpret_cast<u16x8*>(dst + lds_off(64 * u + r32, c4 + 4)) = lo;
        }
    };
    auto dma_stage = [&](int buf) {
        const int soff_a = __builtin_amdgcn_readfirstlane((seg1 ? cc - p.c0 : cc) * 2);      // (A32: pair offset / 2 channels x 4 bytes -- the same number)
        const int soff_w = __builtin_amdgcn_readfirstlane(kg * 2);
        const __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(
            uniform_ptr(seg1 ? a1 : a0), 0, __builtin_amdgcn_readfirstlane(seg1 ? p.a1_bytes : p.a0_bytes), 0x00020000);
        if constexpr (A32) a32_load(rs_a, soff_a);
#pragma unroll
        for (int i = 0; i < (A32 ? 0 : MREP); ++i) {
            unsigned short* dst = As + buf * BM * 64 + (i * 32 + wave * 8) * 64;
            lds_dma(rs_a, dst, a_off[i], soff_a);
        }
#pragma unroll
        for (int j = 0; j < NREP; ++j) {
            unsigned short* dst = Bs + buf * BN * 64 + (j * 32 + wave * 8) * 64;
            lds_dma(rs_w, dst, w_off[j], soff_w);
        }
        kg += 64;
        cc += 64;
        if (cc == Ctot) { cc = 0; ++tap; set_segment(); }
        else if (cc == p.c0) set_segment();
    };

    f32x4 acc[MREP][NREP];
#pragma unroll
    for (int i = 0; i < MREP; ++i)
#pragma unroll
        for (int j = 0; j < NREP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    typedef typename Mfma<T>::frag frag;
    const int frow = lane & 15, fchunk = lane >> 4;
    auto compute = [&](int buf) {
        if constexpr (S3) {
            // split-precision K block: slab 0 = (W_hi, A_hi), slab 1 = (W_lo, A_lo) of the same 32 channels
            frag af[2][MREP], bf[2][NREP];
#pragma unroll
            for (int slab = 0; slab < 2; ++slab) {
#pragma unroll
                for (int i = 0; i < MREP; ++i)
                    af[slab][i] = __builtin_bit_cast(frag, *reinterpret_cast<const u16x8*>(As + buf * BM * 64 + lds_off(wm * 16 * MREP + i * 16 + frow, slab * 4 + fchunk)));
#pragma unroll
                for (int j = 0; j < NREP; ++j)
                    bf[slab][j] = __builtin_bit_cast(frag, *reinterpret_cast<const u16x8*>(Bs + buf * BN * 64 + lds_off(wn * 16 * NREP + j * 16 + frow, slab * 4 + fchunk)));
            }
#pragma unroll
            for (int i = 0; i < MREP; ++i)
#pragma unroll
                for (int j = 0; j < NREP; ++j) {
                    acc[i][j] = Mfma<T>::run(bf[0][j], af[0][i], acc[i][j]);
                    acc[i][j] = Mfma<T>::run(bf[0][j], af[1][i], acc[i][j]);
                    acc[i][j] = Mfma<T>::run(bf[1][j], af[0][i], acc[i][j]);
                }
            return;
        }
#pragma unroll
        for (int slab = 0; slab < 2; ++slab) {
            frag af[MREP], bf[NREP];
#pragma unroll
            for (int i = 0; i < MREP; ++i) {
                const int brow = wm * 16 * MREP + i * 16 + frow;
                u16x8 v = *reinterpret_cast<const u16x8*>(As + buf * BM * 64 + lds_off(brow, slab * 4 + fchunk));
                af[i] = __builtin_bit_cast(frag, v);
            }
#pragma unroll
            for (int j = 0; j < NREP; ++j) {
                const int brow = wn * 16 * NREP + j * 16 + frow;
                u16x8 v = *reinterpret_cast<const u16x8*>(Bs + buf * BN * 64 + lds_off(brow, slab * 4 + fchunk));
                bf[j] = __builtin_bit_cast(frag, v);
            }
#pragma unroll
            for (int i = 0; i < MREP; ++i)
#pragma unroll
                for (int j = 0; j < NREP; ++j) acc[i][j] = Mfma<T>::run(bf[j], af[i], acc[i][j]);
        }
    };

    stamp(p, 0);
    if constexpr (STAGES == 2) {
        dma_stage(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if constexpr (A32) a32_write(0);
        __syncthreads();
        stamp(p, 1);
        for (int kb = kb0, it = 0; kb < kb1; ++kb, ++it) {
            if (kb + 1 < kb1) dma_stage((it + 1) & 1);            // in flight during the MFMAs
            compute(it & 1);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every wave's DMA has landed ...
            if constexpr (A32) { if (kb + 1 < kb1) a32_write((it + 1) & 1); }   // (its fp32 octets too: the slot was retired by the previous barrier;
                                                                  // __syncthreads waits for the ds_writes -- lgkmcnt(0) -- in front of its barrier)
            __syncthreads();                                      // ... before anyone reads the tile
        }
    } else {
        // Deep ring: stages it+1 .. it+STAGES-1 are in flight while stage it is multiplied.  Every wave issues exactly L = MREP + NREP DMA
        // instructions per stage and loads retire in order among themselves, so "at most (STAGES - 2) L outstanding" means stage it+1
        // has landed whatever the younger ones are doing; the last STAGES - 2 steps (nothing left to request) drain fully.
        constexpr int L = MREP + NREP, KEEP = (STAGES - 2) * L;
        const int n_it = kb1 - kb0;
#pragma unroll
        for (int s = 0; s < STAGES - 1; ++s)
            if (s < n_it) dma_stage(s);
        if (n_it >= STAGES - 1) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(KEEP) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        stamp(p, 1);
        int slot = 0, fill = STAGES - 1;                          // slot of stage it; slot stage it+STAGES-1 goes to (= the one step it-1 read)
        for (int it = 0; it < n_it; ++it) {
            const bool more = it + STAGES - 1 < n_it;
            if (more) dma_stage(fill);
            compute(slot);
            if (more) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(KEEP) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();                                      // stage it+1 complete on every wave; slot of stage it free
            slot = slot == STAGES - 1 ? 0 : slot + 1;
            fill = fill == STAGES - 1 ? 0 : fill + 1;
        }
    }
    stamp(p, 2);

    if (p.splits > 1) {          // fp32 slab straight from the fragments (64-byte row segments)
#pragma unroll
        for (int i = 0; i < MREP; ++i) {
            const int m = m0 + wm * 16 * MREP + i * 16 + (lane & 15);
            if (m >= p.M) continue;
#pragma unroll
            for (int j = 0; j < NREP; ++j) {
                const int n4 = n0 + wn * 16 * NREP + j * 16 + 4 * (lane >> 4);
                if (n4 >= p.N) continue;
                slab_store(p, ((static_cast<long>(blockIdx.y) * p.batch + bz) * (p.M - p.m_begin) + (m - p.m_begin)) * p.N + n4, acc[i][j]);
            }
        }
        if (p.tickets) splitk_finish<T, BM, BN, 256>(p, bz, tid_lin, m0, n0, reinterpret_cast<int*>(smem), t);
        return;
    }
    epilogue_tile<T, MREP, NREP, 256, BM, BN, 1, STATS>(p, bz, acc, smem, m0, n0, wm * 16 * MREP, wn * 16 * NREP, lane, t);
    stamp(p, 3);
}

// ---- 8-wave, 3-stage ring variant (the large layers) ---------------------------------------------
// 512 threads = 8 wavefronts (4 x 2), block tile 256 x (32*NREP) in {256x160, 256x128}, one block per
// CU (2 waves per SIMD), persistent: a block walks tiles blockIdx.x, + gridDim.x, ...
// K loop: fragment registers are double buffered and the single raw s_barrier of a K step sits between its
// two 32-k halves.  The last fragments of stage `it` are requested in the first half, so its slot is retired by
// that barrier and stage it+3 is requested into it right behind the barrier: TWO K steps of DMA look-ahead with
// three slots.  Stage it+1 is awaited with a COUNTED s_waitcnt vmcnt(L) (L = DMA instructions of one stage) so
// that stage it+2 stays in flight -- never a full drain inside a tile.  Every wave issues exactly
// L = 4 + ceil(BN/64) DMA instructions per stage (the 32-row remainder pass of the 160-row weight tile is issued
// by the lower 32 lanes of all 8 waves), so one immediate serves all.
// Tile boundary: right after the barrier that retires the ring the block decodes its next tile and requests
// that tile's first two stages into slots 0 / 1; the epilogue runs meanwhile in two row slices through slot 2.
// A32 (pf_conv_desc.a_src_dtype = PF_F32; split-precision 1x1 walk): the activation operand is the fp32 stream itself.  Thread t owns the octet 8 (t & 3) of
// tile rows 2 (t >> 2) + u, u < 2: the four 16-byte buffer loads of its two octets take the places (and the issue slots between the MFMAs of the
// second half) of the four activation DMA pieces of the stage requested there, stay in registers for half a K step, and are turned into the pieces
// hi | lo at lds_off(row, c4) / lds_off(row, c4 + 4) (affine_f / split8, pf_common.h) behind the first MFMA group of the NEXT step -- in front of the
// mid-step barrier that the stage's first fragment reads wait behind (two slots), or one step ahead of it (three).  Counted waits: the octets are
// consumed (the compiler's own vmcnt in front of the conversion) before every explicit wait, so what may stay in flight there is the weight pieces of the
// youngest stage alone: NPIECE - APASS instead of NPIECE; the ds_writes are covered by the lgkmcnt(0) of the mid-step wait.
// AFF (a_scale / a_shift given): the scale / shift octet of a stage is requested behind the (W_lo, A_hi) group of the step that requests the stage -- the
// W_lo fragments are dead from there on -- and the conversion runs in front of the next step's fragment requests, while the second fragment set is dead:
// with the affine registers live next to all four fragment sets the 160-column kernels spilled (108-364 bytes of scratch per lane).
// Cost, stated and not measured in isolation: the four scale / shift loads are YOUNGER than the stage's weight pieces, so the compiler's wait in front of the
// next step's conversion is vmcnt(0) and the youngest weight stage has landed half a step after its request -- on the three-slot 256 x 128 tile that gives up
// the second step of look-ahead the explicit vmcnt(NPIECE - APASS) would leave it (the two-slot blocks drain fully at that point anyway).  Requested in
// front of the weight pieces the octet is live across the (W_lo, A_hi) group and the 160-column kernels spill again.
template <typename T, int NREP, int NW, bool STATS = false, bool S3 = false, int BM_ = 256, bool A32 = false, bool AFF = false>
__global__ __launch_bounds__(64 * NW, BM_ == 128 ? 2 : 1) void k_conv_gemm8(const GemmParams p) {
    // NW = 8: 4 x 2 waves, 64x80 per wave, two waves per SIMD.  NW = 4, BM_ = 256: 2 x 2 waves, 128x80 per wave, ONE wave
    // per SIMD with the whole register file (160 accumulator + 104 fragment registers): twice the MFMAs per
    // LDS read / DMA piece / barrier, and no second wave competing for the issue port.
    // NW = 4, BM_ = 128 (round 5, "two tiles in flight"): 2 x 2 waves with the SAME 64x80 wave tile and K-step schedule, block tile
    // 128 x (32*NREP), a TWO-slot ring (74 KB) so that TWO blocks share a CU: one block's ramp / epilogue overlaps the other's K loop
    // (the 8-wave block idles its CU's matrix pipes for 10-50 % of every tile there).  One K step of DMA look-ahead instead of two --
    // a block that waits for its stage leaves the SIMDs to its neighbour.
    constexpr int NT = 64 * NW, WMG = NW / 2, BM = BM_, BN = 32 * NREP, MREP = BM / (16 * WMG), STAGES = BM_ == 128 ? 2 : 3;
    constexpr bool ONEWAVE = NW == 4 && BM_ == 256;
    static_assert(BM_ == 256 || (BM_ == 128 && NW == 4), "tile shapes: 256 rows (8 or 4 waves) or 128 rows (4 waves, two blocks per CU)");
    constexpr int RPP = NT / 8;                      // tile rows staged by one DMA pass of the block
    constexpr int STAGE = (BM + BN) * 64;            // 16-bit elements per ring slot
    constexpr int BFULL = BN / RPP;                  // full DMA passes of the weight tile
    constexpr bool BHALF = (BN % RPP) != 0;          // + one half pass (BN = 160 with 64-row passes)
    extern __shared__ __attribute__((aligned(16))) unsigned short smem[];

    const int ntile_total = p.mtiles * p.ntiles;
    const long bz = blockIdx.z;
    const unsigned short* a0 = p.a0 + bz * p.a_bs;
    const unsigned short* a1 = p.a1 ? p.a1 + bz * p.a_bs : nullptr;
    const unsigned short* wg = p.w + bz * p.w_bs;
    int m0 = 0, n0 = 0;                              // origin of the tile being multiplied (set_tile)

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int chunk = t & 7, lrow = t >> 3;                       // DMA passes of RPP rows: row = pass*RPP + lrow
    const int lchunk8 = (chunk ^ ((lrow >> 1) & 7)) * 8;
    const int hrow = wave * 4 + (lane >> 3);                      // half pass (lanes 0..31): row = BFULL*64 + hrow
    const int hchunk8 = (chunk ^ ((hrow >> 1) & 7)) * 8;

    constexpr int APASS = BM / RPP;                  // DMA passes of the activation tile
    static_assert(!A32 || (S3 && APASS == 4 && BM * 4 == NT * 2), "fp32-source staging: two octets = four 16-byte loads per thread and stage");
    struct XR { f32x4 x[2][2], s[2], h[2]; int cc; };   // A32: a stage's two fp32 octets (+ the scale / shift of their 8 channels, cc = its pair channel) in flight
    XR xq;
    const int c4 = t & 3, r32 = 2 * (t >> 2);        // A32: octet and first of the two (adjacent) tile rows of this thread -- rows 2 q, 2 q + 1 belong to ONE
                                                     // image (rows per image are even: pf_conv_gemm checks), so one scale / shift octet serves both
    unsigned x_off[2];                               // bytes, or OOB
    int x_sidx = 0;                                  // element of a_scale / a_shift at channel 0 of the octet
    // DMA addressing: buffer descriptors (SGPR) + a per-thread 32-bit byte offset (VGPR) + a per-stage
    // scalar byte offset (soffset), so that a piece costs no vector ALU work per K step -- the kernel is
    // bound by instruction issue, not by the matrix pipe (4 issue slots of a SIMD per 16-clock MFMA,
    // shared by two waves).  Zero padding / ragged tiles: an offset beyond num_records reads as zero.
    // The walk that produces them: pf_gemm_walk.h.
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(wg), 0, __builtin_amdgcn_readfirstlane(p.w_bytes), 0x00020000);
    unsigned w_off[BFULL + 1];                                    // bytes
#ifdef PF_GEMM_BDIRECT        /* experiment: weight fragments straight from L1 / L2 into registers, no weight tile in LDS.
                               * Correct (68 GEMM / conv tests) and 2x SLOWER (3x3 convs 850 -> 440 TF/s): a fragment-shaped load touches 16
                               * half-used cache lines per instruction, four waves fetch the same lines, and the prefetch distance is
                               * half a K step.  Kept as a compile-time record of the measurement. */
    unsigned wb_off[NREP];                                        // bytes: (n of fragment j, this lane's k chunk)
    int kw = 0;                                                   // K offset (elements) of the stage being multiplied
#endif
    // K blocks [kb0, kb1) of this split-K slice
    const int nkb = p.K / 64;
    const int kb0 = blockIdx.y * p.kb_per_split;
    const int kb1 = min(nkb, kb0 + p.kb_per_split);
    const int n_it = kb1 - kb0;
    ConvWalk<APASS, 64, true, true, A32> w;                       // staged rows i * RPP + lrow of the tile
    w.init(p, bz);
    // A32, every new segment: 1x1, a row IS its pixel; rows past M read as zero (and become `shift` under the affine map: never stored, masked in the moments)
    auto a32_rows = [&]() __attribute__((always_inline)) {
        const int ld = w.seg1 ? p.a1_ld : p.a0_ld;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int m = m0 + r32 + u;
            x_off[u] = m < p.M ? (static_cast<unsigned>(m) * static_cast<unsigned>(ld) + 8u * c4) * 4u : GEMM_OOB;
        }
    };
    // Persistent over tiles: a block walks tiles blockIdx.x, + gridDim.x, ...; all per-tile state is set here (this runs once per tile on every thread).
    auto set_tile = [&](int tile) __attribute__((always_inline)) {
        const int tid_lin = xcd_tile(tile, ntile_total);
        const int tile_m = static_cast<unsigned>(tid_lin) / static_cast<unsigned>(p.ntiles), tile_n = tid_lin - tile_m * p.ntiles;
        m0 = p.m_begin + tile_m * BM;
        n0 = tile_n * BN;
        if constexpr (!A32) w.rows_by_advance(p, m0, lrow, RPP);
#pragma unroll
        for (int j = 0; j < BFULL; ++j) w_off[j] = weight_row_offset(p, n0 + j * RPP + lrow, lchunk8);
        w_off[BFULL] = BHALF ? weight_row_offset(p, n0 + BFULL * RPP + hrow, hchunk8) : GEMM_OOB;
        if constexpr (A32 && AFF) x_sidx = (min(m0 + r32, p.M - 1) / p.rows_per_img) * (w.Ctot >> 1) + 8 * c4;
        w.start(p, kb0 * 64, lchunk8, a32_rows);
#ifdef PF_GEMM_BDIRECT
        kw = kb0 * 64;
#pragma unroll
        for (int j = 0; j < NREP; ++j) {
            const int n = n0 + (wave & 1) * 16 * NREP + j * 16 + (lane & 15);
            wb_off[j] = n < p.N ? static_cast<unsigned>(n * p.K + (lane >> 4) * 8) * 2u : GEMM_OOB;
        }
#endif
    };

    // One stage = NPIECE DMA instructions per wave: pieces 0..3 the activation passes, then the weight
    // passes, issued one at a time between MFMAs (a burst of 8 waves x 7 KB stalls every wave at issue
    // for ~900 clocks: the CU's vector-memory pipe moves ~64 B/clk).
    constexpr int NPIECE = APASS + BFULL + (BHALF ? 1 : 0);
    int st_soff_a = 0, st_soff_w = 0;
    auto stage_begin = [&]() __attribute__((always_inline)) { return w.stage_begin(p, a0, a1, st_soff_a, st_soff_w); };
    auto stage_end = [&]() __attribute__((always_inline)) { w.stage_end(p, lchunk8, a32_rows); };
    auto dma_piece = [&](const __amdgpu_buffer_rsrc_t& rs_a, int slot, int k, XR& q) __attribute__((always_inline)) {
        unsigned short* As = smem + slot * STAGE;
        unsigned short* Bs = As + BM * 64;
        if (k < APASS) {
            if constexpr (A32) {                                  // half an fp32 octet into registers (a32_write puts it into the slot)
                const int u = k >> 1, hf = k & 1;
                q.x[u][hf] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_a, x_off[u] + 16u * hf, st_soff_a, 0));
                if (k == 0) q.cc = w.cc;
                return;
            }
            unsigned short* dst = As + (k * RPP + wave * 8) * 64;
            lds_dma16(rs_a, dst, w.off[k], st_soff_a);
#ifdef PF_GEMM_BDIRECT
        } else if (true) {
#endif
        } else if (k < APASS + BFULL) {
            const int j = k - APASS;
            lds_dma16(rs_w, Bs + (j * RPP + wave * 8) * 64, w_off[j], st_soff_w);
        } else if (BHALF) {
            if (lane < 32) lds_dma16(rs_w, Bs + (BFULL * RPP + wave * 4) * 64, w_off[BFULL], st_soff_w);
        }
    };
    auto dma_stage = [&](int slot, XR& q) __attribute__((always_inline)) {
        const __amdgpu_buffer_rsrc_t rs_a = stage_begin();
#pragma unroll
        for (int k = 0; k < NPIECE; ++k) dma_piece(rs_a, slot, k, q);
        stage_end();
    };
    // A32 + AFF: scale / shift of the 8 channels of the stage in q
    auto a32_affine = [&](XR& q) __attribute__((always_inline)) {
        if constexpr (A32 && AFF) {
            const int so = x_sidx + (q.cc >> 1);
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                q.s[hf] = *reinterpret_cast<const f32x4*>(p.a_scale + so + 4 * hf);
                q.h[hf] = *reinterpret_cast<const f32x4*>(p.a_shift + so + 4 * hf);
            }
        }
    };
    // A32: registers of a stage -> its activation image in ring slot `slot`
    auto a32_write = [&](int slot, const XR& q) __attribute__((always_inline)) {
        unsigned short* As = smem + slot * STAGE;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            float f[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = q.x[u][j >> 2][j & 3];
            if constexpr (AFF) {
#pragma unroll
                for (int j = 0; j < 8; ++j) f[j] = affine_f(f[j], q.s[j >> 2][j & 3], q.h[j >> 2][j & 3]);
            }
            u16x8 hi, lo;
            split8<T>(f, hi, lo);
            const int row = r32 + u;
            *reinterpret_cast<u16x8*>(As + lds_off(row, c4)) = hi;
            *reinterpret_cast<u16x8*>(As + lds_off(row, c4 + 4)) = lo;
        }
    };

    f32x4 acc[MREP][NREP];

    typedef typename Mfma<T>::frag frag;
    const int frow = lane & 15, fchunk = lane >> 4;
    // Fragment registers are double buffered (f0 = first 32 k of a stage, f1 = second) and the barrier
    // sits BETWEEN the two halves of a step, so the matrix pipe always has 20 MFMAs queued while LDS
    // reads are in flight (measured: with both halves' reads exposed the K step took 2300 clocks
    // without any DMA, against 1280 of pure MFMA issue):
    //   f1 <- LDS(stage it, k 32..63) | MFMA(f0) | wait DMA(it+1), barrier | f0 <- LDS(stage it+1, k 0..31)
    //   | MFMA(f1) interleaved with the DMA pieces of stage it+2
    frag fa0[MREP], fb0[NREP], fa1[MREP], fb1[NREP];
#ifdef PF_ABL_DUMMY_B
#pragma unroll
    for (int j = 0; j < NREP; ++j) {
        u16x8 z = {1, 2, 3, 4, 5, 6, 7, static_cast<unsigned short>(lane)};
        asm volatile("" : "+v"(z));
        fb0[j] = __builtin_bit_cast(frag, z);
        fb1[j] = __builtin_bit_cast(frag, z);
    }
#endif
    auto load_frags_a = [&](int slot, int slab, frag (&fa)[MREP]) __attribute__((always_inline)) {
        const unsigned short* As = smem + slot * STAGE;
#pragma unroll
        for (int i = 0; i < MREP; ++i)
            fa[i] = __builtin_bit_cast(frag, *reinterpret_cast<const u16x8*>(As + lds_off(wm * 16 * MREP + i * 16 + frow, slab * 4 + fchunk)));
    };
    auto load_frags_b = [&](int slot, int slab, frag (&fb)[NREP], int kadd) __attribute__((always_inline)) {
#ifdef PF_GEMM_BDIRECT
        typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
        const int soff = __builtin_amdgcn_readfirstlane((kw + kadd + slab * 32) * 2);
#pragma unroll
        for (int j = 0; j < NREP; ++j) {
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs_w, wb_off[j], soff, 0);
            fb[j] = __builtin_bit_cast(frag, v);
        }
        return;
#endif
        const unsigned short* Bs = smem + slot * STAGE + BM * 64;
#ifdef PF_ABL_DUMMY_B         /* timing-only: the weight-fragment reads are issued and waited for, but the MFMAs keep their first operands */
#pragma unroll
        for (int j = 0; j < NREP; ++j) {
            u16x8 v = *reinterpret_cast<const u16x8*>(Bs + lds_off(wn * 16 * NREP + j * 16 + frow, slab * 4 + fchunk));
            asm volatile("" :: "v"(v));
        }
        (void)fb;
#else
#pragma unroll
        for (int j = 0; j < NREP; ++j)
            fb[j] = __builtin_bit_cast(frag, *reinterpret_cast<const u16x8*>(Bs + lds_off(wn * 16 * NREP + j * 16 + frow, slab * 4 + fchunk)));
#endif
    };
    auto load_frags = [&](int slot, int slab, frag (&fa)[MREP], frag (&fb)[NREP], int kadd) __attribute__((always_inline)) {   // kadd: 64 for the NEXT stage (PF_GEMM_BDIRECT)
        load_frags_a(slot, slab, fa);
#ifndef PF_ABL_NOLDS_B        /* timing-only: what the weight fragments' share of the LDS reads costs */
        load_frags_b(slot, slab, fb, kadd);
#endif
    };

    auto issue_prologue = [&]() __attribute__((always_inline)) {
        if constexpr (A32 && STAGES == 3) {                // both stages requested, then both written (the fragment registers are dead here)
            XR q0;
            dma_stage(0, q0);
            a32_affine(q0);
            if (n_it > 1) { dma_stage(1, xq); a32_affine(xq); }
            a32_write(0, q0);
            if (n_it > 1) a32_write(1, xq);
        } else if constexpr (A32) {                               // two slots: stage 1 stays in registers, step 0 writes it in front of its barrier
            dma_stage(0, xq);
            a32_affine(xq);
            a32_write(0, xq);
            if (n_it > 1) { dma_stage(1, xq); a32_affine(xq); }
        } else {
            dma_stage(0, xq);
            if (n_it > 1) dma_stage(1, xq);
        }
    };
    const std::true_type YES;
    const std::false_type NO;
    int cur = 0, nx1 = 1, nx2 = 2;
#ifdef PF_GEMM_TIMELINE
    int tl_tile = 0, tl_step = 0;
#endif
    // One K step.  MORE: a next stage exists (wait for it, barrier, prefetch its first fragments);
    // DMA: a stage three ahead exists (issue its pieces between the MFMAs of the second half).  The flags
    // are compile-time so that the steady-state body is branch free and the compiler's s_waitcnt
    // insertion sees exact counts (a conditional around the prefetch made it drain lgkmcnt to 0 right
    // after issuing it, exposing the LDS latency once per step).
    // (-DPF_ABL_NOBARRIER / NODMA / NOLDS: timing-only ablations of this loop -- wrong results -- for tools/gpu_gemm_ablate.sh)
    auto step_l = [&](auto more_tag, auto dma_tag, auto wait_tag, auto flead_tag) __attribute__((always_inline)) {
        constexpr bool MORE = decltype(more_tag)::value, DMA = decltype(dma_tag)::value;
        constexpr int WAIT = decltype(wait_tag)::value;           // DMA instructions that may stay in flight at the mid-step wait
        constexpr int NM = MREP * NREP, LEAD0 = NM - 1 - 2 * (NPIECE - 1), LEAD = LEAD0 < 4 ? LEAD0 : 4, FLEAD = decltype(flead_tag)::value;   // fragment requests go out after FLEAD MFMAs:
        // at every s_waitcnt lgkmcnt the only outstanding LDS reads are then the ones being waited for
        // (the compiler drains to 0, it does not count), and they were issued >= NM - LEAD MFMAs earlier.
#pragma unroll
        for (int idx = 0; idx < NM; ++idx) {
            // (S3: weight-fragment-major order -- the fragment fb0[j] of THIS step was requested j-th during the previous step's last
            // group, so the later ones have time to arrive)
            const int fi = S3 ? idx % MREP : idx / NREP, fj = S3 ? idx / MREP : idx % NREP;
            if constexpr (ONEWAVE) Mfma<T>::acc_agpr(fb0[fj], fa0[fi], acc[fi][fj]);
            else acc[fi][fj] = Mfma<T>::run(fb0[fj], fa0[fi], acc[fi][fj]);
#ifdef PF_GEMM_FLEAD2          /* two bursts: A fragments after FLEAD MFMAs, B fragments after FLEAD2 (A/B build) */
            if (idx == FLEAD - 1) { __builtin_amdgcn_sched_barrier(0); load_frags_a(cur, 1, fa1); __builtin_amdgcn_sched_barrier(0); }
            if (idx == PF_GEMM_FLEAD2 - 1) { __builtin_amdgcn_sched_barrier(0); load_frags_b(cur, 1, fb1, 0); __builtin_amdgcn_sched_barrier(0); }
#else
            if (idx == FLEAD - 1) {
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (A32) {
                    // the octets requested during the previous step (or by the prologue) become stage it + STAGES - 1 in LDS, while the second fragment set is
                    // still dead: three slots -- the steps that still await a younger stage (WAIT != 0) -- into the slot retired one step ago; two slots --
                    // every step that has a successor -- into the other slot
                    constexpr bool PEND = STAGES == 3 ? WAIT != 0 : MORE;
                    if constexpr (PEND) {
                        a32_write(STAGES == 3 ? nx2 : nx1, xq);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
#ifndef PF_ABL_NOLDS
                load_frags(cur, 1, fa1, fb1, 0);
#endif
                __builtin_amdgcn_sched_barrier(0);
            }
#endif
        }
        // (S3: hipcc sank 15 of the first group's 20 MFMAs below the wait -- register-only instructions move across an inline-asm
        // s_waitcnt -- so the wait found the nine f1 reads it had just issued: pinned)
        if constexpr (S3) __builtin_amdgcn_sched_barrier(0);
        if constexpr (MORE) {
            // my pieces of the next stage have landed (the stage after it may still be in flight: WAIT), and my
            // reads of the current slot have returned -- it is refilled right after the barrier
            if constexpr (A32 && WAIT != 0) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "n"(WAIT) : "memory");
            else
#ifdef PF_GEMM_BDIRECT
            if constexpr (true) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#else
            if constexpr (WAIT == 0) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#endif
            else if constexpr (WAIT == 6) asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory");
            else if constexpr (WAIT == 7) asm volatile("s_waitcnt vmcnt(7) lgkmcnt(0)" ::: "memory");
            else if constexpr (WAIT == 8) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
            else if constexpr (WAIT == 9) asm volatile("s_waitcnt vmcnt(9) lgkmcnt(0)" ::: "memory");
            else if constexpr (WAIT == 12) asm volatile("s_waitcnt vmcnt(12) lgkmcnt(0)" ::: "memory");
            else if constexpr (WAIT == 13) asm volatile("s_waitcnt vmcnt(13) lgkmcnt(0)" ::: "memory");
            else static_assert(WAIT == 0, "add the immediate");
#ifndef PF_ABL_NOBARRIER
            __builtin_amdgcn_s_barrier();                         // next stage complete; the current slot no longer read
#endif
            asm volatile("" ::: "memory");
        }
        __amdgpu_buffer_rsrc_t rs_a = rs_w;
        if constexpr (DMA) rs_a = stage_begin();
        if constexpr (S3) {
            // Split-precision step: the stage holds [hi(32) | lo(32)] of 32 channels for both operands, f0 = (W_hi, A_hi),
            // f1 = (W_lo, A_lo).  The first half multiplied W_hi A_hi; here W_lo A_hi (group X, fa0's last use -> the next stage's fa0
            // is requested behind it) and W_hi A_lo (group Y, weight-fragment-major: fb0[j] is re-requested as soon as its four
            // MFMAs are issued).  W_lo A_lo (2^-22) is not formed.  60 MFMAs per 52 KB stage instead of 40: the K' = 3 K walk of
            // rounds 2-3 moved [hi] twice and ran 3 stages per 64 channels, this one 2.
#pragma unroll
            for (int idx = 0; idx < NM; ++idx) {
                acc[idx / NREP][idx % NREP] = Mfma<T>::run(fb1[idx % NREP], fa0[idx / NREP], acc[idx / NREP][idx % NREP]);
                if constexpr (DMA) {
                    const int k = idx - LEAD;
                    if (k >= 0 && (k & 1) == 0 && (k >> 1) < NPIECE) {
                        __builtin_amdgcn_sched_barrier(0);
                        dma_piece(rs_a, cur, k >> 1, xq);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            if constexpr (DMA) { __builtin_amdgcn_sched_barrier(0); a32_affine(xq); }
            if (MORE) { __builtin_amdgcn_sched_barrier(0); load_frags_a(nx1, 0, fa0); __builtin_amdgcn_sched_barrier(0); }
#pragma unroll
            for (int j = 0; j < NREP; ++j) {
#pragma unroll
                for (int i = 0; i < MREP; ++i) acc[i][j] = Mfma<T>::run(fb0[j], fa1[i], acc[i][j]);
                if (MORE) {
                    __builtin_amdgcn_sched_barrier(0);
                    const unsigned short* Bn = smem + nx1 * STAGE + BM * 64;
                    fb0[j] = __builtin_bit_cast(frag, *reinterpret_cast<const u16x8*>(Bn + lds_off(wn * 16 * NREP + j * 16 + frow, fchunk)));
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        } else {
#pragma unroll
        for (int idx = 0; idx < NM; ++idx) {
            if constexpr (ONEWAVE) Mfma<T>::acc_agpr(fb1[idx % NREP], fa1[idx / NREP], acc[idx / NREP][idx % NREP]);
            else acc[idx / NREP][idx % NREP] = Mfma<T>::run(fb1[idx % NREP], fa1[idx / NREP], acc[idx / NREP][idx % NREP]);
#ifdef PF_GEMM_FLEAD2
            if (MORE && idx == FLEAD - 1) { __builtin_amdgcn_sched_barrier(0); load_frags_a(nx1, 0, fa0); __builtin_amdgcn_sched_barrier(0); }
            if (MORE && idx == PF_GEMM_FLEAD2 - 1) { __builtin_amdgcn_sched_barrier(0); load_frags_b(nx1, 0, fb0, 64); __builtin_amdgcn_sched_barrier(0); }
#else
            if (MORE && idx == FLEAD - 1) {
                __builtin_amdgcn_sched_barrier(0);
#ifndef PF_ABL_NOLDS
                load_frags(nx1, 0, fa0, fb0, 64);
#endif
                __builtin_amdgcn_sched_barrier(0);
            }
#endif
            if constexpr (DMA) {
                const int k = idx - LEAD;                         // pieces after MFMA LEAD, LEAD+2, ...
                if (k >= 0 && (k & 1) == 0 && (k >> 1) < NPIECE) {
                    __builtin_amdgcn_sched_barrier(0);
#ifndef PF_ABL_NODMA
#ifdef PF_ABL_NODMA_B         /* timing-only: activation pieces only */
                    if ((k >> 1) < APASS)
#endif
                    dma_piece(rs_a, cur, k >> 1, xq);             // stage it+3 into the slot retired at this step's barrier
#endif
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        }
        static_assert(LEAD >= 0 && LEAD + 2 * (NPIECE - 1) < NM, "DMA pieces must fit behind the MFMAs of the second half");
        if constexpr (DMA) stage_end();
        cur = cur == STAGES - 1 ? 0 : cur + 1;
        nx1 = nx1 == STAGES - 1 ? 0 : nx1 + 1;
        nx2 = nx2 == STAGES - 1 ? 0 : nx2 + 1;
#ifdef PF_GEMM_BDIRECT
        kw += 64;
#endif
#ifdef PF_GEMM_TIMELINE
        PF_TL(p, tl_tile == 1 && tl_step < 8, 15 + tl_step);
        ++tl_step;
#endif
    };
#ifndef PF_GEMM_FLEAD
#define PF_GEMM_FLEAD 4
#endif
    auto step = [&](auto more_tag, auto dma_tag, auto wait_tag) __attribute__((always_inline)) { step_l(more_tag, dma_tag, wait_tag, std::integral_constant<int, PF_GEMM_FLEAD>()); };

    stamp(p, 0);
#ifdef PF_GEMM_SETPRIO
    // static priority for the later-dispatched half of the block (MI355X_MICROARCH.md, "two waves per SIMD", item 4):
    // measured neutral here (-DPF_GEMM_SETPRIO=1 / 3, same-box A/B round 2: 3x3 convs 915 -> 891 / 912 TF/s, step 14.85 vs 14.76):
    // both waves of a SIMD run the same MFMA-dense stream, there is no loader / computer pairing for a priority to help
    if (NW == 8 && wave >= 4) __builtin_amdgcn_s_setprio(PF_GEMM_SETPRIO);
#endif
    int tile = blockIdx.x;
    set_tile(tile);
    issue_prologue();
    bool first = true;
    for (;;) {
        PF_TL(p, tl_tile == 1, 12);
#pragma unroll
        for (int i = 0; i < MREP; ++i)
#pragma unroll
            for (int j = 0; j < NREP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (first && n_it > 1) {                          // stage 0 landed, stage 1 may still fly
            if constexpr (A32) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(NPIECE - APASS) : "memory");   // (its weight pieces: the octets of both stages were consumed or are older)
            else
#ifdef PF_GEMM_BDIRECT
            if constexpr (true) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#else
            if constexpr (NPIECE == 7) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
#endif
            else if constexpr (NPIECE == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            else if constexpr (NPIECE == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else if constexpr (NPIECE == 9) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
            else if constexpr (NPIECE == 13) asm volatile("s_waitcnt vmcnt(13)" ::: "memory");
            else if constexpr (NPIECE == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {                                          // later tiles: the epilogue's stores sit behind the DMAs in vmcnt
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        if constexpr (A32) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the prologue's ds_writes
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (first) stamp(p, 1);
        first = false;
        PF_TL(p, tl_tile == 1, 13);
        if constexpr (STAGES == 3) { if (n_it > 2) { dma_stage(2, xq); a32_affine(xq); } }   // third stage in flight (slot 2 staged the previous tile's epilogue)
        load_frags(0, 0, fa0, fb0, 0);
        cur = 0; nx1 = 1; nx2 = 2 % STAGES;
        PF_TL(p, tl_tile == 1, 14);
        // The slot of stage `it` is retired at the mid-step barrier of step `it` (its last fragments are
        // requested in the first half), and stage it+3 is requested into it right behind that barrier: with
        // three slots a stage has TWO K steps to arrive, the mid-step wait leaves the younger one in flight.
        const std::integral_constant<int, A32 ? NPIECE - APASS : NPIECE> W1;
        const std::integral_constant<int, 0> W0;
        if constexpr (STAGES == 3) {
            for (int it = 0; it + 3 < n_it; ++it) step(YES, YES, W1);
            if (n_it >= 3) step(YES, NO, W1);
            if (n_it >= 2) step(YES, NO, W0);
            step(NO, NO, W0);
        } else {
            // two slots: stage it+2 goes into the slot of stage it right behind the mid-step barrier of step it and is awaited
            // (full drain: nothing younger is in flight) at the mid-step wait of step it+1
            for (int it = 0; it + 2 < n_it; ++it) step(YES, YES, W0);
            if (n_it >= 2) step(YES, NO, W0);
            step(NO, NO, W0);
        }
        if constexpr (ONEWAVE) asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");   // inline-asm MFMA results -> vector ALU reads
        stamp(p, 2);

        const int em0 = m0, en0 = n0;
        const int next = tile + static_cast<int>(gridDim.x);
        const bool has_next = next < ntile_total;
        if (p.splits > 1) {          // fp32 slab straight from the fragments (64-byte row segments)
#pragma unroll
            for (int i = 0; i < MREP; ++i) {
                const int m = em0 + wm * 16 * MREP + i * 16 + (lane & 15);
                if (m >= p.M) continue;
#pragma unroll
                for (int j = 0; j < NREP; ++j) {
                    const int n4 = en0 + wn * 16 * NREP + j * 16 + 4 * (lane >> 4);
                    if (n4 >= p.N) continue;
                    slab_store(p, ((static_cast<long>(blockIdx.y) * p.batch + bz) * (p.M - p.m_begin) + (m - p.m_begin)) * p.N + n4, acc[i][j]);
                }
            }
            if (p.tickets) splitk_finish<T, BM, BN, NT>(p, bz, tile, em0, en0, reinterpret_cast<int*>(smem + (STAGES - 1) * STAGE), t);
            if (!has_next) break;
            __syncthreads();                              // every wave is done reading the operand ring
            set_tile(next);
            issue_prologue();
        } else {
            // epilogue in two 128-row halves through ring slot 2; the next tile's first two stages are
            // requested into slots 0 / 1 right after the barrier that frees the ring, so their latency
            // hides behind the epilogue
            // (laundered lane / thread ids: the epilogue's per-thread addressing would otherwise be hoisted out
            // of the tile loop and stay live -- in registers the K loop has none to spare of)
            int e_lane = lane, e_t = t;
            asm volatile("" : "+v"(e_lane), "+v"(e_t));
            if constexpr (STAGES == 3) {
                epilogue_tile<T, MREP, NREP, NT, BM, BN, 2, STATS>(p, bz, acc, smem + 2 * STAGE, em0, en0, wm * 16 * MREP, wn * 16 * NREP,
                                                            e_lane, e_t, [&]() __attribute__((always_inline)) { if (has_next) { set_tile(next); issue_prologue(); } });
            } else {
                // two slots: the whole 128-row tile is staged through the (dead) ring at once; the next tile's first stages are
                // requested only when every wave has read its rows back out -- the neighbour block owns the matrix pipes meanwhile
                epilogue_tile<T, MREP, NREP, NT, BM, BN, 1, STATS>(p, bz, acc, smem, em0, en0, wm * 16 * MREP, wn * 16 * NREP, e_lane, e_t);
                if (has_next) {
                    __syncthreads();
                    set_tile(next);
                    issue_prologue();
                }
            }
            PF_TL(p, tl_tile == 1, 23);
            if (!has_next) break;
        }
        tile = next;
#ifdef PF_GEMM_TIMELINE
        ++tl_tile; tl_step = 0;
#endif
    }
    stamp(p, 3);
}

// Split-K second pass: sum the fp32 slabs in split order (deterministic) and run the epilogue.
template <typename T>
__global__ __launch_bounds__(256) void k_splitk_reduce(const GemmParams p) {
    const long quads = static_cast<long>(p.N / 4);
    const int Ms = p.M - p.m_begin;
    const long total = static_cast<long>(p.batch) * Ms * quads;
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= total) return;
    const int n4 = static_cast<int>(i % quads) * 4;
    const long bm = i / quads;
    const int ml = static_cast<int>(bm % Ms), m = p.m_begin + ml;
    const long bz = bm / Ms;
    const long slab = static_cast<long>(p.batch) * Ms * p.N;
    const float* src = p.partial + (bz * Ms + ml) * p.N + n4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < p.splits; ++s) {
        const float4 x = *reinterpret_cast<const float4*>(src + s * slab);
        v[0] += x.x; v[1] += x.y; v[2] += x.z; v[3] += x.w;
    }
    epilogue_store<T>(p, bz, m, n4, v);
}

// diagnostics buffer (device) + its capacity, see pf_debug_gemm_profile: published / read as ONE atomic
// snapshot so that concurrent launches from other host threads see either the old or the new pair
struct ProfState { unsigned long long* buf; long blocks; };
static std::atomic<const ProfState*> g_prof_state{nullptr};
static inline ProfState prof_snapshot() {
    const ProfState* s = g_prof_state.load(std::memory_order_acquire);
    return s ? *s : ProfState{nullptr, 0};
}

// The launchers below run ONE pass of a plan's kernel: output rows [p.m_begin, p.M) in p.splits K slices (launch_pass combines the slices).

template <typename T, int MREP, int NREP, bool STATS, bool S3, int STAGES, bool A32 = false>
static pf_status launch_ring(const GemmParams& p, int batch, hipStream_t st) {
    constexpr int BM = 32 * MREP, BN = 32 * NREP;
    const size_t smem = static_cast<size_t>(STAGES) * (BM + BN) * 64 * sizeof(unsigned short);
    static std::atomic<unsigned long long> lds_set{0};
    const pf_status s = allow_dynamic_lds(reinterpret_cast<const void*>(k_conv_gemm<T, MREP, NREP, STATS, S3, STAGES, A32>), smem, lds_set, "pf_conv_gemm");
    if (s != PF_OK) return s;
    hipLaunchKernelGGL((k_conv_gemm<T, MREP, NREP, STATS, S3, STAGES, A32>), dim3(p.mtiles * p.ntiles, p.splits, batch), dim3(256), smem, st, p);
    PF_CHECK_LAUNCH("pf_conv_gemm");
    return PF_OK;
}

template <typename T, int MREP, int NREP, bool STATS = false, bool S3 = false>
static pf_status launch_s(const pf_conv_plan& g, const GemmParams& gp, int batch, hipStream_t st) {
    constexpr int BM = 32 * MREP, BN = 32 * NREP;
    GemmParams p = gp;
    p.mtiles = static_cast<int>(cdiv(p.M - p.m_begin, BM));
    p.ntiles = static_cast<int>(cdiv(p.N, BN));
    const ProfState ps = prof_snapshot();
    p.prof = (ps.buf && static_cast<long>(p.mtiles) * p.ntiles * p.splits * batch <= ps.blocks) ? ps.buf : nullptr;
    // (the four-slot ring is instantiated for the plain kernels only: the plan gives the moment / split-precision variants two slots)
    if constexpr (!STATS && !S3) {
        if (g.ring_slots == 4) return launch_ring<T, MREP, NREP, false, false, 4>(p, batch, st);
    }
    if constexpr (S3) {
        if (p.a32) return launch_ring<T, MREP, NREP, STATS, true, 2, true>(p, batch, st);      // the fp32-source form of the same kernel arm
    }
    return launch_ring<T, MREP, NREP, STATS, S3, 2>(p, batch, st);
}

template <typename T, int MREP, int NREP>
static pf_status launch(const pf_conv_plan& g, const GemmParams& gp, int batch, hipStream_t st) {
    if (gp.s3) return gp.gn_partial ? launch_s<T, MREP, NREP, true, true>(g, gp, batch, st) : launch_s<T, MREP, NREP, false, true>(g, gp, batch, st);
    return gp.gn_partial ? launch_s<T, MREP, NREP, true>(g, gp, batch, st) : launch_s<T, MREP, NREP, false>(g, gp, batch, st);
}

template <typename T, int NREP, int NW, bool STATS = false, bool S3 = false, int BM = 256, bool A32 = false, bool AFF = false>
static pf_status launch8w_s(const GemmParams& gp, int batch, hipStream_t st) {
    constexpr int BN = 32 * NREP, STAGES = BM == 128 ? 2 : 3;
    GemmParams p = gp;
    p.mtiles = static_cast<int>(cdiv(p.M - p.m_begin, BM));
    p.ntiles = static_cast<int>(cdiv(p.N, BN));
    {
        const int rpp = 8 * NW, rem = rpp % p.rows_per_img;       // rows of one DMA pass, as (images, rows, columns)
        p.adv_img = rpp / p.rows_per_img;
        p.adv_y = rem / p.w_out;
        p.adv_x = rem % p.w_out;
    }
    const ProfState ps = prof_snapshot();
    p.prof = (ps.buf && static_cast<long>(p.mtiles) * p.ntiles * p.splits * batch <= ps.blocks) ? ps.buf : nullptr;
    const size_t smem = static_cast<size_t>(STAGES) * (BM + BN) * 64 * sizeof(unsigned short);
    static std::atomic<unsigned long long> lds_set{0};
    const pf_status s = allow_dynamic_lds(reinterpret_cast<const void*>(k_conv_gemm8<T, NREP, NW, STATS, S3, BM, A32, AFF>), smem, lds_set, "pf_conv_gemm (8-wave)");
    if (s != PF_OK) return s;
    // persistent over tiles: one block per CU walks tiles b, b + grid, ... (a multiple of 8 keeps a tile on
    // the XCD its id maps to); PF_GEMM8_PERSIST=0 launches one block per tile
    const int cap1 = gemm_tuning().big_persist;
    const int cap = BM == 128 ? 2 * cap1 : cap1;                  // (two resident 128-row blocks per CU)
    int grid = p.mtiles * p.ntiles;
    if (cap > 0) {
        int gx = std::max(1, cap / (p.splits * batch));           // blockIdx.y / z multiply the resident blocks
        if (gx >= 8) gx = gx / 8 * 8;
        grid = std::min(grid, gx);
    }
    hipLaunchKernelGGL((k_conv_gemm8<T, NREP, NW, STATS, S3, BM, A32, AFF>), dim3(grid, p.splits, batch), dim3(64 * NW), smem, st, p);
    PF_CHECK_LAUNCH("pf_conv_gemm (8-wave)");
    return PF_OK;
}

template <typename T, int NREP, int NW, int BM = 256>
static pf_status launch8w(const GemmParams& gp, int batch, hipStream_t st) {
    if constexpr (NW == 8 || BM == 128) {
        // fp32 sources (pf_conv_gemm has refused what is not instantiated: moments -- the plan gives this kernel none in that mode -- and the affine map on
        // the 256 x 160 tile, whose registers do not hold the scale / shift octet without scratch)
        if (gp.s3 && gp.a32 && gp.a_scale) {
            if constexpr (NREP == 5 && BM == 256) { set_error("pf_conv_gemm: a_scale on the 256 x 160 tile"); return PF_ERR_ARG; }
            else return launch8w_s<T, NREP, NW, false, true, BM, true, true>(gp, batch, st);
        }
        if (gp.s3 && gp.a32) return launch8w_s<T, NREP, NW, false, true, BM, true>(gp, batch, st);
        if (gp.s3) return gp.gn_partial ? launch8w_s<T, NREP, NW, true, true, BM>(gp, batch, st) : launch8w_s<T, NREP, NW, false, true, BM>(gp, batch, st);
        if (gp.gn_partial) return launch8w_s<T, NREP, NW, true, false, BM>(gp, batch, st);
    }
    return launch8w_s<T, NREP, NW, false, false, BM>(gp, batch, st);
}

template <typename T, int NREP>
static pf_status launch8(const pf_conv_plan& g, const GemmParams& gp, int batch, hipStream_t st) {
    if (g.block_rows == 128) return launch8w<T, NREP, 4, 128>(gp, batch, st);       // two 128-row blocks per CU (round 5)
    if (g.waves == 4) return launch8w<T, NREP, 4>(gp, batch, st);                   // (PF_GEMM8_WAVES=4, see plan_conv_gemm)
    return launch8w<T, NREP, 8>(gp, batch, st);
}

// One pass of plan g's kernel over rows [p.m_begin, p.M), then -- split K without arrival counters -- the second kernel that sums the slabs.
static pf_status launch_pass(const pf_conv_plan& g, GemmParams p, int dtype, int batch, hipStream_t st) {
    pf_status s = PF_OK;
    if (g.kernel == 2) {
        const ProfState ps = prof_snapshot();
        p.prof = (ps.buf && ps.blocks >= 256) ? ps.buf : nullptr;
        s = launch_gemm32(p, dtype, batch, st);
    } else if (g.kernel == 1) {
        PF_DISPATCH_16(dtype, "pf_conv_gemm", s = g.nrep == 5 ? launch8<T, 5>(g, p, batch, st) : launch8<T, 4>(g, p, batch, st));
    } else {
        PF_DISPATCH_16(dtype, "pf_conv_gemm",
            if (g.nrep == 5) s = g.mrep == 2 ? launch<T, 2, 5>(g, p, batch, st) : launch<T, 4, 5>(g, p, batch, st);
            else s = g.mrep == 2 ? launch<T, 2, 4>(g, p, batch, st) : launch<T, 4, 4>(g, p, batch, st));
    }
    if (s != PF_OK || p.splits == 1 || p.tickets) return s;
    const long total = static_cast<long>(batch) * (p.M - p.m_begin) * (p.N / 4);
    PF_DISPATCH_16(dtype, "pf_conv_gemm", hipLaunchKernelGGL((k_splitk_reduce<T>), dim3(cdiv(total, 256)), dim3(256), 0, st, p));
    PF_CHECK_LAUNCH("pf_conv_gemm (split-K reduce)");
    return PF_OK;
}

}  // namespace pf

using namespace pf;

extern "C" pf_status pf_conv_gemm(const pf_conv_desc* d, void* stream) {
    PF_REQUIRE(d, "pf_conv_gemm: null descriptor");
    PF_REQUIRE(d->a0 && d->w && d->out, "pf_conv_gemm: null pointer");
    PF_REQUIRE(d->dtype == PF_BF16 || d->dtype == PF_F16, "pf_conv_gemm: dtype must be PF_BF16 or PF_F16");
    PF_REQUIRE(d->out_dtype == d->dtype || d->out_dtype == PF_F32, "pf_conv_gemm: out_dtype must equal dtype or be PF_F32");
    PF_REQUIRE(!d->residual || d->res_dtype == d->dtype || d->res_dtype == PF_F32, "pf_conv_gemm: res_dtype must equal dtype or be PF_F32");
    const int c1 = d->a1 ? d->c1 : 0;
    const bool a32 = d->a_src_dtype == PF_F32;                    // fp32 sources, split while they are staged
    PF_REQUIRE(d->a_src_dtype == 0 || a32, "pf_conv_gemm: a_src_dtype must be 0 (a0 / a1 hold dtype elements) or PF_F32");
    PF_REQUIRE(a32 || (!d->a_scale && !d->a_shift), "pf_conv_gemm: a_scale / a_shift belong to fp32 sources (a_src_dtype = PF_F32)");
    if (a32) {
        PF_REQUIRE(d->split3 && d->ksize == 1 && d->stride == 1 && d->pad == 0 && d->upsample == 0 && d->wrap_pad == 0 && d->crop == 0 && !d->subpixel &&
                   d->batch == 1, "pf_conv_gemm: fp32 sources serve the split-precision 1x1 walk only (split3, ksize 1, stride 1, no padding, batch 1)");
        PF_REQUIRE(d->c0 > 0 && d->c0 % 32 == 0 && c1 % 32 == 0, "pf_conv_gemm: fp32 channel counts (%d,%d) must be multiples of 32", d->c0, c1);
        PF_REQUIRE(d->a0_ld >= d->c0 && d->a0_ld % 4 == 0 && (!d->a1 || (d->a1_ld >= c1 && d->a1_ld % 4 == 0)),
                   "pf_conv_gemm: leading dimensions of fp32 sources must be >= their channels and multiples of 4");
        PF_REQUIRE((d->a_scale != nullptr) == (d->a_shift != nullptr), "pf_conv_gemm: a_scale and a_shift come together");
        PF_REQUIRE((!d->a_scale || aligned16(d->a_scale)) && (!d->a_shift || aligned16(d->a_shift)), "pf_conv_gemm: a_scale / a_shift must be 16-byte aligned");
    } else
    PF_REQUIRE(d->c0 > 0 && d->c0 % 64 == 0 && c1 % 64 == 0, "pf_conv_gemm: channel counts (%d,%d) must be multiples of 64", d->c0, c1);
    PF_REQUIRE(d->ksize == 1 || d->ksize == 3, "pf_conv_gemm: ksize must be 1 or 3");
    PF_REQUIRE(d->stride == 1 || d->stride == 2, "pf_conv_gemm: stride must be 1 or 2");
    PF_REQUIRE(d->pad == 0 || d->pad == 1, "pf_conv_gemm: pad must be 0 or 1");
    PF_REQUIRE(d->upsample == 0 || d->upsample == 1, "pf_conv_gemm: upsample must be 0 or 1");
    PF_REQUIRE(d->n_img > 0 && d->h_in > 0 && d->w_in > 0 && d->h_out > 0 && d->w_out > 0, "pf_conv_gemm: bad spatial sizes");
    // n_out that is not a multiple of 4 is allowed for a bare product (no epilogue operands) when
    // out_ld leaves room for the 4-wide store; the extra columns are written as zeros.
    PF_REQUIRE(d->n_out > 0 && (d->n_out % 4 == 0 || (!d->bias && !d->rowvec && !d->residual && d->out_ld >= (d->n_out + 3) / 4 * 4)),
               "pf_conv_gemm: n_out=%d must be a multiple of 4 (or no epilogue operands and a padded out_ld)", d->n_out);
    PF_REQUIRE(a32 || (d->a0_ld >= d->c0 && d->a0_ld % 8 == 0), "pf_conv_gemm: a0_ld must be >= c0 and a multiple of 8");
    PF_REQUIRE(a32 || !d->a1 || (d->a1_ld >= c1 && d->a1_ld % 8 == 0), "pf_conv_gemm: a1_ld must be >= c1 and a multiple of 8");
    PF_REQUIRE(d->epilogue == PF_EPILOGUE_GEGLU || (d->out_ld >= d->n_out && d->out_ld % 4 == 0), "pf_conv_gemm: out_ld must be >= n_out and a multiple of 4");
    PF_REQUIRE(!d->residual || (d->res_ld >= d->n_out && d->res_ld % 4 == 0), "pf_conv_gemm: res_ld must be >= n_out and a multiple of 4");
    PF_REQUIRE(!d->rowvec || (d->rowvec_ld >= d->n_out && d->rowvec_ld % 4 == 0), "pf_conv_gemm: rowvec_ld must be >= n_out and a multiple of 4");
    PF_REQUIRE(aligned16(d->a0) && aligned16(d->w) && aligned16(d->out) && (!d->a1 || aligned16(d->a1)) &&
               (!d->bias || aligned16(d->bias)) && (!d->rowvec || aligned16(d->rowvec)) &&
               (!d->residual || aligned16(d->residual)), "pf_conv_gemm: pointers must be 16-byte aligned");
    PF_REQUIRE(d->batch >= 1, "pf_conv_gemm: batch must be >= 1");
    PF_REQUIRE(d->epilogue == PF_EPILOGUE_NONE || d->epilogue == PF_EPILOGUE_GEGLU || d->epilogue == PF_EPILOGUE_SPLIT,
               "pf_conv_gemm: unknown epilogue %d", d->epilogue);
    if (d->epilogue == PF_EPILOGUE_SPLIT)
        PF_REQUIRE(d->n_out % 32 == 0 && d->out_dtype == d->dtype && d->out_ld >= 2 * d->n_out && !d->rowvec,
                   "pf_conv_gemm: SPLIT epilogue needs n_out %% 32 == 0 (hi / lo interleave per 32 columns), a 16-bit output with out_ld >= 2 n_out, no row vector");
    if (d->split3 && !a32)
        PF_REQUIRE(!d->a1 && d->c0 % 64 == 0, "pf_conv_gemm: a split-precision walk (split3) takes ONE source of 2 x channels = c0 (hi / lo interleaved per 32)");
    if (d->epilogue == PF_EPILOGUE_GEGLU)
        PF_REQUIRE(d->n_out % 4 == 0 && d->out_dtype == d->dtype && !d->residual && d->out_ld >= d->n_out / 2 && d->out_ld % 2 == 0,
                   "pf_conv_gemm: GEGLU epilogue needs n_out %% 4 == 0, 16-bit output, no residual, out_ld >= n_out/2");
    PF_REQUIRE(d->wrap_pad >= 0 && d->wrap_pad <= 2 && d->crop >= 0 && d->crop <= 2 && d->wrap_pad <= d->w_in,
               "pf_conv_gemm: wrap_pad and crop must be in 0..2");
    {   // the output size must be what the conv arithmetic produces
        const int hl = d->h_in << d->upsample, wl = (d->w_in + 2 * d->wrap_pad) << d->upsample;
        const int ho = (hl + 2 * d->pad - d->ksize) / d->stride + 1, wo = (wl + 2 * d->pad - d->ksize) / d->stride + 1 - 2 * d->crop;
        // one more zero row / column at the bottom / right is allowed (pixels past the input read as zero anyway):
        // diffusers Downsample2D(padding=0) = F.pad(x, (0, 1, 0, 1)) + conv3x3 stride 2 of the VAE encoder
        const int ho1 = (hl + 2 * d->pad + 1 - d->ksize) / d->stride + 1, wo1 = (wl + 2 * d->pad + 1 - d->ksize) / d->stride + 1 - 2 * d->crop;
        PF_REQUIRE((d->h_out == ho && d->w_out == wo) || (d->h_out == ho1 && d->w_out == wo1),
                   "pf_conv_gemm: output size (%d,%d) does not match (%d,%d) [or (%d,%d) with a trailing zero row / column]",
                   d->h_out, d->w_out, ho, wo, ho1, wo1);
    }
    if (d->subpixel)
        PF_REQUIRE(d->ksize == 3 && d->upsample == 1 && d->stride == 1 && d->pad == 1 && d->batch == 1 && !d->residual && !d->rowvec &&
                   d->epilogue == PF_EPILOGUE_NONE && d->h_out % 2 == 0 && d->w_out % 2 == 0 && d->crop % 2 == 0 && d->wrap_pad <= 1,
                   "pf_conv_gemm: subpixel serves nearest x2 + 3x3 stride-1 pad-1 convolutions (bias only; weights packed [4][n_out][2][2][c0 + c1])");
    const int batch = d->subpixel ? 4 : d->batch;
    GemmParams p;
    params_from_desc(d, p);
    const pf_conv_plan g = plan_conv_gemm(p, batch, d->workspace != nullptr, d->gn_partial != nullptr);
    // fp32 sources + affine map: every arm but the 256 x 160 tile of the 8-wave kernel (no registers left for the scale / shift octet: 144 bytes of
    // scratch per lane); the caller runs that problem in the two-launch form (ops.conv_gemm_a32_serves asks the same question of the plan)
    PF_REQUIRE(!(a32 && d->a_scale && g.kernel == 1 && g.block_rows == 256 && g.nrep == 5),
               "pf_conv_gemm: a_scale / a_shift are not available on the 256 x 160 tile of the 8-wave kernel (this problem's plan): use the pair form");
    PF_REQUIRE(!(a32 && d->a_scale) || (d->h_out * d->w_out) % 2 == 0, "pf_conv_gemm: a_scale needs an even number of rows per image");
    if (d->gn_partial) {
        PF_REQUIRE(g.gn_rows > 0, "pf_conv_gemm: gn_partial given but this problem cannot emit GroupNorm moments (ask pf_conv_gemm_gn_rows first)");
        PF_REQUIRE(aligned16(d->gn_partial), "pf_conv_gemm: gn_partial must be 16-byte aligned");
        // (a caller that cached a plan made under other PF_GEMM32 / PF_GN_EPILOGUE_RES settings: its buffer has the wrong number of runs)
        PF_REQUIRE(d->gn_rows == g.gn_rows, "pf_conv_gemm: gn_partial is sized for runs of gn_rows = %d rows, but this launch's plan writes runs of %d rows (ask pf_conv_gemm_plan again)",
                   d->gn_rows, g.gn_rows);
        p.gn_partial = d->gn_partial;
        p.gn_rows = g.gn_rows;
    }
    {   // extents for the buffer descriptors of the 8-wave and 32x32 kernels (32-bit offsets, < 2 GiB)
        const long npix = static_cast<long>(d->n_img) * d->h_in * d->w_in;
        // (fp32 sources: p.c0 / p.c1 count pair elements = 2 x fp32 channels, of 4 bytes each)
        const long a0b = a32 ? ((npix - 1) * p.a0_ld + p.c0 / 2) * 4 : ((npix - 1) * p.a0_ld + p.c0) * 2;
        const long a1b = !p.a1 ? 0 : a32 ? ((npix - 1) * p.a1_ld + p.c1 / 2) * 4 : ((npix - 1) * p.a1_ld + p.c1) * 2;
        const long wb = static_cast<long>(p.N) * p.K * 2;      // (per batch element / sub-pixel phase: the kernels offset the base by w_bs)
        PF_REQUIRE(a0b < (1L << 31) && a1b < (1L << 31) && wb < (1L << 31),
                   "pf_conv_gemm: each operand must be smaller than 2 GiB (32-bit buffer offsets)");
        p.a0_bytes = static_cast<unsigned>(a0b); p.a1_bytes = static_cast<unsigned>(a1b); p.w_bytes = static_cast<unsigned>(wb);
    }
    p.partial = static_cast<float*>(d->workspace);
    // In-launch combine: implemented, bit-identical (tests/test_gpu_kernels.py), and OFF by default -- it does not pay at these
    // tile sizes: the last-arriving workgroup reads splits x 164 KB of slabs through one CU (~65 GB/s per block cross-XCD,
    // MI355X_MICROARCH.md "handoff-payload") while the second kernel spreads the same reads over the whole chip: the step went
    // 65.3 -> 67.8 ms with write-through slabs, -> 72.9 ms with a release fence per workgroup (profiles/archive/r3k_ab_splitk.txt,
    // r3l_ab_splitk.txt).  PF_SPLITK_INKERNEL=1 enables it for A/B (16x16x32 kernels only).
    if (d->tickets && g.kernel != 2 && gemm_tuning().splitk_inkernel && d->workspace_bytes < (1ULL << 32)) {      // (32-bit slab offsets)
        // enough zeroed counters for every (batch, tile) of the split launch?  (tile counts of split plans: <= 320 of the
        // 4-wave kernel, <= 255 of the 8-wave one)
        PF_REQUIRE(d->n_tickets >= g.n_tickets && (reinterpret_cast<uintptr_t>(d->tickets) & 3) == 0,
                   "pf_conv_gemm: %d arrival counters needed, %d given", g.n_tickets, d->n_tickets);
        p.tickets = d->tickets;
    }
    PF_REQUIRE(g.workspace_bytes == 0 || (d->workspace_bytes >= g.workspace_bytes && aligned16(d->workspace)),
               "pf_conv_gemm: workspace of %zu bytes (16-byte aligned) needed, got %zu", g.workspace_bytes, d->workspace_bytes);
    hipStream_t st = as_stream(stream);
    p.splits = g.splits; p.kb_per_split = g.kb_per_split;
    if (g.m_split == 0) return launch_pass(g, p, d->dtype, batch, st);
    // two launches: full rounds unsplit, then the tail rows with split K
    GemmParams p2 = p;
    p.M = g.m_split;
    p2.m_begin = g.m_split; p2.splits = g.tail_splits; p2.kb_per_split = g.tail_kb;
    const pf_status s1 = launch_pass(g, p, d->dtype, batch, st);
    return s1 != PF_OK ? s1 : launch_pass(g, p2, d->dtype, batch, st);
}

extern "C" pf_status pf_debug_gemm_profile(void* device_buffer, long capacity_blocks) {
    // (states are leaked on purpose: a few bytes per call of a diagnostics switch, never freed under a reader)
    const ProfState* s = device_buffer ? new ProfState{static_cast<unsigned long long*>(device_buffer), capacity_blocks} : nullptr;
    g_prof_state.store(s, std::memory_order_release);
    return PF_OK;
}
