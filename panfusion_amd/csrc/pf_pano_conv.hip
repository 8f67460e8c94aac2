// The FAED encoder's convolutions on MFMA for gfx950 (models/faed/modules.py:5-36 CircularPadding + nn.Conv2d(padding = 0), with the
// bias and the evaluation-mode BatchNorm folded into scale / shift): wide kernels (3 .. 9), narrow channels (32 .. 128), columns periodic
// in longitude, zero rows above and below.  Contract: pf_pano_conv_desc in include/panfusion_hip.h.
//
// An implicit GEMM without an im2col operand or a padded copy.  A workgroup of 4 wavefronts owns a tile of TH x 16 output pixels and
// ALL n_out channels; a wavefront owns RW = TH / 4 of the rows: 4 where such tiles still give every CU two workgroups (a weight
// fragment read from LDS then serves 4 MFMAs instead of 2 -- the loop is bound by LDS reads), else 2.  Both forms add in the same
// order, so their results are identical.  The K loop walks  channel block of 32 -> tap row ky -> tap column kx:
//   * per channel block the input tile WITH its halo (((TH - 1) s + k) x (15 s + k) pixels x 32 channels) is staged in LDS once: wrapped
//     columns and zero rows are resolved there, so that the MFMA loop reads plain shifted addresses;
//   * per tap row the weights [n_out][k][32] of that row are staged;
//   * per tap one v_mfma_f32_16x16x32_f16 per (output row, 16 channels), computed TRANSPOSED (weights as the A operand, pixels as B):
//     a lane then holds 4 consecutive channels of ONE pixel, which the epilogue stores as one 8- or 16-byte word.
// The order of a sum depends on nothing but (channel block, ky, kx): a pixel's position in the tile changes the lane, not the order,
// so shifting the panorama in longitude shifts the result bit for bit.  No atomics.
//
// LDS rows are padded by 16 bytes (pixel stride 80 B, weight row stride 64 k + 16 B): the 16 lanes of a ds_read_b128 phase then fall
// into 16 distinct 4-bank groups at stride 1 (2-way at stride 2, where consecutive lanes are two pixels apart).
//
// The image layer (downconv1_rgb, 3 -> 32 at 9 x 9) is a second kernel behind the same entry point: it reads the planar uint8 / fp32
// image, applies v / 127.5 - 1 while staging, and orders K as (ky, c, kx padded to 16) so that a lane's 8 operand values are 8
// neighbouring columns of one LDS row.
#include "pf_common.h"

namespace pf {
namespace {

typedef __attribute__((ext_vector_type(8))) _Float16 h8;

constexpr int PC_TW = 16;                  // output columns of a tile; its rows are 4 RW (8 or 16)
constexpr int PC_CC = 32;                  // channels per K block (one MFMA's K)
constexpr int PC_PIX = PC_CC + 8;          // LDS pixel stride in halves

struct PanoConvParams {
    const unsigned short* x;
    const unsigned short* weight;
    const float* scale;
    const float* shift;
    const unsigned short* residual;
    void* out;
    int h, w, c_in, h_out, w_out, pad, relu;
};

__host__ __device__ constexpr int pc_tile_h(int ks, int s, int th) { return (th - 1) * s + ks; }
__host__ __device__ constexpr int pc_tile_w(int ks, int s) { return (PC_TW - 1) * s + ks; }
__host__ __device__ constexpr int pc_wrow(int ks) { return ks * PC_CC + 8; }
__host__ __device__ constexpr size_t pc_lds_bytes(int ks, int s, int nout, int th) {
    return (static_cast<size_t>(pc_tile_h(ks, s, th)) * pc_tile_w(ks, s) * PC_PIX + static_cast<size_t>(nout) * pc_wrow(ks)) * 2;
}

__device__ __forceinline__ int wrap_col(int x, int w) {
    x %= w;
    return x < 0 ? x + w : x;
}

// The shared epilogue: lane l holds channels n0 .. n0 + 3 of pixel (img, oy, ox).
template <bool OUT32>
__device__ __forceinline__ void pano_store(const f32x4& acc, const float* scale, const float* shift, int relu, const unsigned short* residual,
                                           void* out, long m, int n_out, int n0) {
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        v[r] = __builtin_fmaf(acc[r], scale[n0 + r], shift[n0 + r]);
        if (relu) v[r] = fmaxf(v[r], 0.0f);
    }
    const long o = m * n_out + n0;
    if (residual) {
        const u16x4 rr = *reinterpret_cast<const u16x4*>(residual + o);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += to_f32<F16>(rr[r]);
    }
    if constexpr (OUT32) {
        *reinterpret_cast<f32x4*>(static_cast<float*>(out) + o) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
        u16x4 q;
#pragma unroll
        for (int r = 0; r < 4; ++r) q[r] = from_f32<F16>(v[r]);
        *reinterpret_cast<u16x4*>(static_cast<unsigned short*>(out) + o) = q;
    }
}

// (two wavefronts per SIMD at least: the 4-row, 128-channel form holds 128 accumulator registers and would otherwise take the whole
// register file, leaving a CU one workgroup and nothing to hide its staging behind)
template <int KS, int S, int NOUT, int RW, bool OUT32>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_pano_conv(const PanoConvParams p) {
    constexpr int TH = 4 * RW, TIH = pc_tile_h(KS, S, TH), TIW = pc_tile_w(KS, S), WROW = pc_wrow(KS), NF = NOUT / 16;
    extern __shared__ __attribute__((aligned(16))) unsigned short pc_lds[];
    unsigned short* tile = pc_lds;                          // [TIH][TIW][PC_PIX]
    unsigned short* wl = pc_lds + TIH * TIW * PC_PIX;       // [NOUT][WROW]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int img = blockIdx.z, oy0 = blockIdx.y * TH, ox0 = blockIdx.x * PC_TW;
    const int iy0 = oy0 * S - p.pad, ix0 = ox0 * S - p.pad;
    const int px = lane & 15, g = lane >> 4;

    f32x4 acc[RW][NF];
#pragma unroll
    for (int mf = 0; mf < RW; ++mf)
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) acc[mf][nf] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nchunk = p.c_in / PC_CC;
    for (int ch = 0; ch < nchunk; ++ch) {
        for (int ky = 0; ky < KS; ++ky) {
            __syncthreads();                                // the previous tap row's fragments are read
            if (ky == 0) {
                for (int idx = tid; idx < TIH * TIW * 4; idx += 256) {
                    const int j = idx & 3, pix = idx >> 2, r = pix / TIW, col = pix - r * TIW;
                    const int yy = iy0 + r;
                    u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
                    if (yy >= 0 && yy < p.h) {
                        const int xx = wrap_col(ix0 + col, p.w);
                        v = *reinterpret_cast<const u16x8*>(p.x + ((static_cast<long>(img) * p.h + yy) * p.w + xx) * p.c_in + ch * PC_CC + j * 8);
                    }
                    *reinterpret_cast<u16x8*>(tile + pix * PC_PIX + j * 8) = v;
                }
            }
            for (int idx = tid; idx < NOUT * KS * 4; idx += 256) {
                const int j = idx & 3, t = idx >> 2, n = t / KS, kx = t - n * KS;
                const u16x8 v = *reinterpret_cast<const u16x8*>(p.weight + (static_cast<long>(n * KS + ky) * KS + kx) * p.c_in + ch * PC_CC + j * 8);
                *reinterpret_cast<u16x8*>(wl + n * WROW + kx * PC_CC + j * 8) = v;
            }
            __syncthreads();
            const unsigned short* trow = tile + ((RW * wave * S + ky) * TIW + px * S) * PC_PIX + g * 8;
            const unsigned short* wrow = wl + px * WROW + g * 8;
#pragma unroll
            for (int kx = 0; kx < KS; ++kx) {
                h8 b[RW];
#pragma unroll
                for (int mf = 0; mf < RW; ++mf) b[mf] = *reinterpret_cast<const h8*>(trow + (mf * S * TIW + kx) * PC_PIX);
#pragma unroll
                for (int nf = 0; nf < NF; ++nf) {
                    const h8 a = *reinterpret_cast<const h8*>(wrow + nf * 16 * WROW + kx * PC_CC);
#pragma unroll
                    for (int mf = 0; mf < RW; ++mf) acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b[mf], acc[mf][nf], 0, 0, 0);
                }
            }
        }
    }

    const int ox = ox0 + px;
#pragma unroll
    for (int mf = 0; mf < RW; ++mf) {
        const int oy = oy0 + RW * wave + mf;
        if (oy >= p.h_out || ox >= p.w_out) continue;
        const long m = (static_cast<long>(img) * p.h_out + oy) * p.w_out + ox;
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) pano_store<OUT32>(acc[mf][nf], p.scale, p.shift, p.relu, p.residual, p.out, m, NOUT, nf * 16 + g * 4);
    }
}

// ---- the image layer: planar [n][3][h][w] uint8 / fp32 on the 0 .. 255 scale, 9 x 9, 3 -> 32 ------------------------------------------
constexpr int IM_KS = 9, IM_PAD = 4, IM_NOUT = 32, IM_TH = 8;
constexpr int IM_TIH = IM_TH - 1 + IM_KS, IM_TIW = PC_TW - 1 + IM_KS;       // 16 x 24
constexpr int IM_PAIRS = IM_KS * 3;                                        // (ky, c) pairs, 16 K values each (9 taps + 7 zeros)
constexpr int IM_STEPS = (IM_PAIRS + 1) / 2;                               // MFMA steps of two pairs
constexpr int IM_WROW = IM_STEPS * 32 + 8;

template <typename SRC> __device__ __forceinline__ float image_value(const void* x, long i);
template <> __device__ __forceinline__ float image_value<uint8_t>(const void* x, long i) { return static_cast<float>(static_cast<const uint8_t*>(x)[i]); }
template <> __device__ __forceinline__ float image_value<float>(const void* x, long i) { return static_cast<const float*>(x)[i]; }

template <typename SRC, bool OUT32>
__global__ __launch_bounds__(256) void k_pano_conv_image(const PanoConvParams p) {
    __shared__ __attribute__((aligned(16))) unsigned short img_l[3 * IM_TIH * IM_TIW];
    __shared__ __attribute__((aligned(16))) unsigned short wl[IM_NOUT * IM_WROW];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int img = blockIdx.z, oy0 = blockIdx.y * IM_TH, ox0 = blockIdx.x * PC_TW;
    const int px = lane & 15, g = lane >> 4;

    for (int idx = tid; idx < 3 * IM_TIH * IM_TIW; idx += 256) {
        const int c = idx / (IM_TIH * IM_TIW), rem = idx - c * (IM_TIH * IM_TIW), r = rem / IM_TIW, col = rem - r * IM_TIW;
        const int yy = oy0 - IM_PAD + r;
        float v = 0.0f;
        if (yy >= 0 && yy < p.h) {
            const int xx = wrap_col(ox0 - IM_PAD + col, p.w);
            v = image_value<SRC>(p.x, ((static_cast<long>(img) * 3 + c) * p.h + yy) * p.w + xx) / 127.5f - 1.0f;     // FAED.py:70
        }
        img_l[idx] = from_f32<F16>(v);
    }
    for (int idx = tid; idx < IM_NOUT * IM_STEPS * 32; idx += 256) {
        const int n = idx / (IM_STEPS * 32), k = idx - n * (IM_STEPS * 32), pair = k >> 4, kx = k & 15;
        unsigned short v = 0;
        if (pair < IM_PAIRS && kx < IM_KS) {
            const int ky = pair / 3, c = pair - ky * 3;
            v = p.weight[((n * IM_KS + ky) * IM_KS + kx) * 3 + c];
        }
        wl[n * IM_WROW + k] = v;
    }
    __syncthreads();

    f32x4 acc[2][2];
#pragma unroll
    for (int mf = 0; mf < 2; ++mf)
#pragma unroll
        for (int nf = 0; nf < 2; ++nf) acc[mf][nf] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int s = 0; s < IM_STEPS; ++s) {
        const int pair = 2 * s + (g >> 1), half = g & 1;
        u16x8 b[2];
#pragma unroll
        for (int mf = 0; mf < 2; ++mf) {
            b[mf] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
            if (pair < IM_PAIRS) {
                const int ky = pair / 3, c = pair - ky * 3;
                const unsigned short* src = img_l + (c * IM_TIH + 2 * wave + mf + ky) * IM_TIW + px + half * 8;
                if (half == 0) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) b[mf][j] = src[j];
                } else {
                    b[mf][0] = src[0];                       // kx = 8; kx 9 .. 15 are the zero weights
                }
            }
        }
#pragma unroll
        for (int nf = 0; nf < 2; ++nf) {
            const h8 a = *reinterpret_cast<const h8*>(wl + (nf * 16 + px) * IM_WROW + s * 32 + g * 8);
#pragma unroll
            for (int mf = 0; mf < 2; ++mf) {
                h8 bb;
                __builtin_memcpy(&bb, &b[mf], 16);
                acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bb, acc[mf][nf], 0, 0, 0);
            }
        }
    }

    const int ox = ox0 + px;
#pragma unroll
    for (int mf = 0; mf < 2; ++mf) {
        const int oy = oy0 + 2 * wave + mf;
        if (oy >= p.h_out || ox >= p.w_out) continue;
        const long m = (static_cast<long>(img) * p.h_out + oy) * p.w_out + ox;
#pragma unroll
        for (int nf = 0; nf < 2; ++nf) pano_store<OUT32>(acc[mf][nf], p.scale, p.shift, p.relu, p.residual, p.out, m, IM_NOUT, nf * 16 + g * 4);
    }
}

template <int KS, int S, int NOUT, int RW, bool OUT32>
pf_status launch_pano_conv(const PanoConvParams& p, int n_img, hipStream_t st) {
    static std::atomic<unsigned long long> done{0};
    constexpr size_t lds = pc_lds_bytes(KS, S, NOUT, 4 * RW);
    const pf_status s = allow_dynamic_lds(reinterpret_cast<const void*>(k_pano_conv<KS, S, NOUT, RW, OUT32>), lds, done, "pf_pano_conv");
    if (s != PF_OK) return s;
    const dim3 grid(static_cast<unsigned>(cdiv(p.w_out, PC_TW)), static_cast<unsigned>(cdiv(p.h_out, 4 * RW)), static_cast<unsigned>(n_img));
    hipLaunchKernelGGL((k_pano_conv<KS, S, NOUT, RW, OUT32>), grid, dim3(256), lds, st, p);
    return PF_OK;
}

// Rows per wavefront (THE rule; pf_pano_conv_tile_rows reports it).  4 at stride 1 where 16 x 16 tiles still give each of the 256 CUs
// two workgroups; a stride-2 tile of 16 rows would need 127 KB of LDS, and the 3 x 3 kernel at 128 channels would spill registers in
// that form (10 VGPRs, 44 B of scratch), so neither has it.  PF_PANO_CONV_ROWS = 2 | 4 forces a form where both exist (A/B and tests;
// the results do not differ).
int pano_conv_rows(int ksize, int stride, int n_img, int h_out, int w_out) {
    if (stride != 1 || ksize == 3) return 2;
    const int forced = env_int("PF_PANO_CONV_ROWS", 0);
    if (forced == 2 || forced == 4) return forced;
    return static_cast<long>(cdiv(w_out, PC_TW)) * cdiv(h_out, 16) * n_img >= 512 ? 4 : 2;
}

template <int KS, int S, int NOUT>
pf_status launch_pano_conv_rows(const PanoConvParams& p, bool out32, int n_img, hipStream_t st) {
    if constexpr (S == 1 && KS != 3) {
        if (pano_conv_rows(KS, S, n_img, p.h_out, p.w_out) == 4)
            return out32 ? launch_pano_conv<KS, S, NOUT, 4, true>(p, n_img, st) : launch_pano_conv<KS, S, NOUT, 4, false>(p, n_img, st);
    }
    return out32 ? launch_pano_conv<KS, S, NOUT, 2, true>(p, n_img, st) : launch_pano_conv<KS, S, NOUT, 2, false>(p, n_img, st);
}

template <int KS, int S>
pf_status dispatch_pano_conv(const PanoConvParams& p, int n_out, bool out32, int n_img, hipStream_t st) {
#define PF_PC_ARM(N) \
    if (n_out == N) return launch_pano_conv_rows<KS, S, N>(p, out32, n_img, st)
    PF_PC_ARM(32);
    PF_PC_ARM(64);
    PF_PC_ARM(128);
#undef PF_PC_ARM
    set_error("pf_pano_conv: n_out must be 32, 64 or 128, got %d", n_out);
    return PF_ERR_ARG;
}

__global__ void k_faed_features(const float* x, int n, int h, int w, int C, const float* weight, float* out) {
    const long idx = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (idx >= static_cast<long>(n) * h * C) return;
    const int c = idx % C;
    const long row = idx / C;                 // image * h + y
    const int y = row % h;
    const long i = row / h;
    const float* src = x + row * w * C + c;
    float sum = 0.0f;
    for (int col = 0; col < w; ++col) sum += src[static_cast<long>(col) * C];
    out[i * C * h + static_cast<long>(c) * h + y] = weight[y] * (sum / static_cast<float>(w));
}

}  // namespace
}  // namespace pf

extern "C" pf_status pf_pano_conv(const pf_pano_conv_desc* d, void* stream) {
    using namespace pf;
    PF_REQUIRE(d, "pf_pano_conv: null pointer: desc");
    PF_REQUIRE(d->x, "pf_pano_conv: null pointer: x");
    PF_REQUIRE(d->weight, "pf_pano_conv: null pointer: weight");
    PF_REQUIRE(d->scale, "pf_pano_conv: null pointer: scale");
    PF_REQUIRE(d->shift, "pf_pano_conv: null pointer: shift");
    PF_REQUIRE(d->out, "pf_pano_conv: null pointer: out");
    const bool image = d->x_dtype == PF_U8 || d->x_dtype == PF_F32;
    PF_REQUIRE(image || d->x_dtype == PF_F16, "pf_pano_conv: x_dtype must be PF_F16 (NHWC activations) or PF_U8 / PF_F32 (the planar image), got %d", d->x_dtype);
    PF_REQUIRE(d->out_dtype == PF_F16 || d->out_dtype == PF_F32, "pf_pano_conv: out_dtype must be PF_F16 or PF_F32, got %d", d->out_dtype);
    PF_REQUIRE(d->ksize == 3 || d->ksize == 4 || d->ksize == 5 || d->ksize == 7 || d->ksize == 9, "pf_pano_conv: ksize must be 3, 4, 5, 7 or 9, got %d", d->ksize);
    PF_REQUIRE(d->stride == (d->ksize == 4 ? 2 : 1), "pf_pano_conv: stride must be 2 at ksize 4 and 1 at the odd kernels, got stride %d at ksize %d", d->stride, d->ksize);
    PF_REQUIRE(d->n_out == 32 || d->n_out == 64 || d->n_out == 128, "pf_pano_conv: n_out must be 32, 64 or 128, got %d", d->n_out);
    if (image)
        PF_REQUIRE(d->c_in == 3 && d->ksize == 9 && d->n_out == 32, "pf_pano_conv: the image layer is c_in 3, ksize 9, n_out 32, got c_in %d, ksize %d, n_out %d", d->c_in, d->ksize, d->n_out);
    else
        PF_REQUIRE(d->c_in == 32 || d->c_in == 64 || d->c_in == 128, "pf_pano_conv: c_in must be 32, 64 or 128, got %d", d->c_in);
    PF_REQUIRE(d->n_img >= 1 && d->h >= 1 && d->w >= 1, "pf_pano_conv: n_img, h and w must be positive, got %d, %d, %d", d->n_img, d->h, d->w);
    const int pad = d->stride == 2 ? 1 : (d->ksize - 1) / 2;
    PF_REQUIRE(d->w >= pad, "pf_pano_conv: w = %d is narrower than pad = %d (one period of columns must cover the margin)", d->w, pad);
    PF_REQUIRE(d->stride == 1 || (d->h % 2 == 0 && d->w % 2 == 0), "pf_pano_conv: stride 2 needs even h and w, got %d x %d", d->h, d->w);
    const int h_out = (d->h + 2 * pad - d->ksize) / d->stride + 1, w_out = (d->w + 2 * pad - d->ksize) / d->stride + 1;
    const long long lim = 1LL << 31;
    PF_REQUIRE(static_cast<long long>(d->n_img) * d->h * d->w * d->c_in < lim, "pf_pano_conv: x holds 2^31 elements or more (n_img * h * w * c_in)");
    PF_REQUIRE(static_cast<long long>(d->n_img) * h_out * w_out * d->n_out < lim, "pf_pano_conv: out holds 2^31 elements or more (n_img * h_out * w_out * n_out)");
    PF_REQUIRE(d->n_img <= 65535 && cdiv(h_out, 8) <= 65535, "pf_pano_conv: n_img and h_out / 8 must fit a launch grid (65535)");
    PF_REQUIRE(aligned16(d->weight) && aligned16(d->out) && (image || aligned16(d->x)) && (!d->residual || aligned16(d->residual)),
               "pf_pano_conv: x, weight, residual and out must be 16-byte aligned");

    PanoConvParams p;
    p.x = static_cast<const unsigned short*>(d->x);
    p.weight = static_cast<const unsigned short*>(d->weight);
    p.scale = d->scale;
    p.shift = d->shift;
    p.residual = static_cast<const unsigned short*>(d->residual);
    p.out = d->out;
    p.h = d->h; p.w = d->w; p.c_in = d->c_in; p.h_out = h_out; p.w_out = w_out; p.pad = pad; p.relu = d->relu != 0;
    const dim3 grid(static_cast<unsigned>(cdiv(w_out, PC_TW)), static_cast<unsigned>(cdiv(h_out, IM_TH)), static_cast<unsigned>(d->n_img));   // (the image layer's)
    hipStream_t st = as_stream(stream);
    const bool out32 = d->out_dtype == PF_F32;
    pf_status s = PF_OK;
    if (image) {
        if (d->x_dtype == PF_U8) {
            if (out32) hipLaunchKernelGGL((k_pano_conv_image<uint8_t, true>), grid, dim3(256), 0, st, p);
            else hipLaunchKernelGGL((k_pano_conv_image<uint8_t, false>), grid, dim3(256), 0, st, p);
        } else {
            if (out32) hipLaunchKernelGGL((k_pano_conv_image<float, true>), grid, dim3(256), 0, st, p);
            else hipLaunchKernelGGL((k_pano_conv_image<float, false>), grid, dim3(256), 0, st, p);
        }
    } else {
        switch (d->ksize) {
            case 3: s = dispatch_pano_conv<3, 1>(p, d->n_out, out32, d->n_img, st); break;
            case 4: s = dispatch_pano_conv<4, 2>(p, d->n_out, out32, d->n_img, st); break;
            case 5: s = dispatch_pano_conv<5, 1>(p, d->n_out, out32, d->n_img, st); break;
            case 7: s = dispatch_pano_conv<7, 1>(p, d->n_out, out32, d->n_img, st); break;
            default: s = dispatch_pano_conv<9, 1>(p, d->n_out, out32, d->n_img, st); break;
        }
        if (s != PF_OK) return s;
    }
    PF_CHECK_LAUNCH("pf_pano_conv");
    return PF_OK;
}

extern "C" int pf_pano_conv_tile_rows(int ksize, int stride, int n_img, int h, int w) {
    using namespace pf;
    if (!(ksize == 3 || ksize == 4 || ksize == 5 || ksize == 7 || ksize == 9) || stride != (ksize == 4 ? 2 : 1) || n_img < 1 || h < 1 || w < 1) return 0;
    const int pad = stride == 2 ? 1 : (ksize - 1) / 2;
    if (w < pad || (stride == 2 && (h % 2 || w % 2))) return 0;
    return 4 * pano_conv_rows(ksize, stride, n_img, (h + 2 * pad - ksize) / stride + 1, (w + 2 * pad - ksize) / stride + 1);
}

extern "C" pf_status pf_faed_features(const float* x, int n, int h, int w, int C, const float* weight, float* out, void* stream) {
    using namespace pf;
    PF_REQUIRE(x && weight && out, "pf_faed_features: null pointer");
    PF_REQUIRE(n >= 1 && h >= 1 && w >= 1 && C >= 1, "pf_faed_features: n, h, w and C must be positive, got %d, %d, %d, %d", n, h, w, C);
    PF_REQUIRE(static_cast<long long>(n) * h * w * C < (1LL << 31), "pf_faed_features: x holds 2^31 elements or more");
    const long total = static_cast<long>(n) * h * C;
    hipLaunchKernelGGL(k_faed_features, dim3(static_cast<unsigned>(cdiv(total, 256))), dim3(256), 0, as_stream(stream), x, n, h, w, C, weight, out);
    PF_CHECK_LAUNCH("pf_faed_features");
    return PF_OK;
}
