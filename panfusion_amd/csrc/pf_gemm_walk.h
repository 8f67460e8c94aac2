// The implicit-GEMM operand walk of the persistent tile kernels (k_conv_gemm8: pf_gemm.hip; k_conv_gemm32: pf_gemm32.hip; the 4-wave k_conv_gemm keeps
// a copy of its own, see there): everything
// that turns "output row m, K block kb" into "buffer descriptor + per-thread byte offset + scalar offset, or out of range".  Device code only.
// A K block is (tap, source, BK channels); the per-thread activation offsets change only when the tap or the source changes (a "segment"),
// inside a segment only the scalar offset moves.  Zero padding and ragged tiles are offsets beyond num_records (GEMM_OOB), which read as zero.
// Pipeline decisions (ring slots, counted waits, where a piece is issued between MFMAs) and the fp32-source register staging are the kernels'.
#pragma once
#include "pf_common.h"
#include "pf_gemm_params.h"

namespace pf {

constexpr unsigned GEMM_OOB = 0x80000000u;                        // (the launcher guarantees tensors < 2 GiB)

struct NoOp { __device__ void operator()() const {} };

// XCD-aware, bijective remap of a 1-D tile id (8 XCDs, block b runs on XCD b % 8): the tiles that share an activation row panel run on one XCD.
__device__ __forceinline__ int xcd_tile(int tile, int ntile_total) {
    const int q = ntile_total >> 3, r = ntile_total & 7;
    const int xcd = tile & 7, idx = tile >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}
// Byte offset of 16-byte chunk `chunk8` (in elements) of weight row n, or out of range.
__device__ __forceinline__ unsigned weight_row_offset(const GemmParams& p, int n, int chunk8) {
    return n < p.N ? static_cast<unsigned>(n * p.K + chunk8) * 2u : GEMM_OOB;
}
// SUBPIX: the 2 x 2 taps of a sub-pixel phase exist.
template <bool SUBPIX> __device__ __forceinline__ void tap_yx(const GemmParams& p, int tap, int& ky, int& kx) {
    ky = p.ksize == 3 ? tap / 3 : SUBPIX && p.ksize == 2 ? tap >> 1 : 0;
    kx = p.ksize == 3 ? tap - 3 * ky : SUBPIX && p.ksize == 2 ? tap & 1 : 0;
}

// ROWS: staged activation rows per thread.  BK: channels per K block.  PACKED: p.fastseg may select the packed row state (seg_pack: img = linear pixel
// index, y = validity bits).  SUBPIX: ksize 2 and the phase-dependent pads exist.  A32: the kernel stages fp32 rows through registers and addresses them
// itself -- the walk keeps the K state and the source, and hands every new segment to the kernel's hook.
// The K state is pinned with readfirstlane at every step (pin): integer division runs on the vector ALU, and without the pin hipcc treats the whole walk as
// divergent and puts every stage_end() under exec masks.  The 8-wave kernel had no pins in its own copy; with them every instantiation of it but the
// plain 256 x 128 one (164 -> 180 spilled SGPRs) keeps or lowers its registers, spills and scratch, without them most spill 10-40 SGPRs more.
template <int ROWS, int BK, bool PACKED, bool SUBPIX, bool A32 = false>
struct ConvWalk {
    int Ctot, Hl, Wl, pad_y, pad_x;                               // of the launch
    int kg, tap, cc;                                              // wave-uniform: K element, tap, channel inside the tap's concatenated sources
    bool seg1;                                                    // current source is a1
    int img[ROWS], y[ROWS], x[ROWS];                              // per staged row: image and top-left input coordinate (or the packed form)
    unsigned off[ROWS];                                           // bytes, or GEMM_OOB

    static __device__ __forceinline__ int pin(int v) { return __builtin_amdgcn_readfirstlane(v); }
    __device__ __forceinline__ void init(const GemmParams& p, long bz) {
        Ctot = p.c0 + p.c1;
        Hl = p.h_in << p.up;
        Wl = (p.w_in + 2 * p.wrap) << p.up;
        pad_y = SUBPIX && p.subpix ? 1 - (static_cast<int>(bz) >> 1) : p.pad;      // (sub-pixel phase: pf_gemm_params.h)
        pad_x = SUBPIX && p.subpix ? 1 - (static_cast<int>(bz) & 1) : p.pad;
    }
    __device__ __forceinline__ void put_row(const GemmParams& p, int i, bool ok, int im, int yo, int xo) {
        img[i] = ok ? im : 0;
        y[i] = ok ? yo * p.stride - pad_y : -(1 << 20);           // never in range
        x[i] = (xo + p.crop) * p.stride - pad_x;
        if (PACKED && p.fastseg) seg_pack(img[i], y[i], x[i], p.h_in, p.w_in);
    }
    // output rows m0 + lrow + i row_step -> (image, y, x): two divisions for the first row, then the host-computed advance of row_step rows (p.adv_*) with one carry per level
    __device__ __forceinline__ void rows_by_advance(const GemmParams& p, int m0, int lrow, int row_step) {
        const unsigned m = static_cast<unsigned>(m0 + lrow);
        int im = static_cast<int>(m / static_cast<unsigned>(p.rows_per_img));
        const unsigned rem = m - static_cast<unsigned>(im) * static_cast<unsigned>(p.rows_per_img);
        int yo = static_cast<int>(rem / static_cast<unsigned>(p.w_out));
        int xo = static_cast<int>(rem) - yo * p.w_out;
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            put_row(p, i, m0 + i * row_step + lrow < p.M, im, yo, xo);
            xo += p.adv_x;
            if (xo >= p.w_out) { xo -= p.w_out; ++yo; }
            yo += p.adv_y;
            if (yo >= p.h_out) { yo -= p.h_out; ++im; }
            im += p.adv_img;
        }
    }
    // A new tap or source: the source, and every staged row's offset of its first channel.
    template <typename F = NoOp> __device__ __forceinline__ void set_segment(const GemmParams& p, int lchunk8, F a32_rows = F()) {
        int ky, kx;
        tap_yx<SUBPIX>(p, tap, ky, kx);
        seg1 = __builtin_amdgcn_readfirstlane(cc >= p.c0 ? 1 : 0) != 0;
        const int ld = seg1 ? p.a1_ld : p.a0_ld;
        if constexpr (A32) { a32_rows(); return; }                // (1x1: a row IS its pixel)
        if (PACKED && p.fastseg) {
            const unsigned sel = (1u << ky) | (16u << kx);
            const int tap_pix = ky * p.w_in + kx;
#pragma unroll
            for (int i = 0; i < ROWS; ++i) {
                const unsigned o = ((static_cast<unsigned>(img[i]) + static_cast<unsigned>(tap_pix)) * static_cast<unsigned>(ld) + static_cast<unsigned>(lchunk8)) * 2u;
                off[i] = (static_cast<unsigned>(y[i]) & sel) == sel ? o : GEMM_OOB;
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const int yi = y[i] + ky, xi = x[i] + kx;             // xi: column in the (virtually wrap-padded, upsampled) input
            // (no short-circuit: hipcc keeps && as nested exec-masked branches and sinks the uniform K-walk updates into them)
            const bool ok = (static_cast<unsigned>(yi) < static_cast<unsigned>(Hl)) & (static_cast<unsigned>(xi) < static_cast<unsigned>(Wl));
            int sx = (xi >> p.up) - p.wrap;                       // source column: the padding is circular
            sx += sx < 0 ? p.w_in : 0;
            sx -= sx >= p.w_in ? p.w_in : 0;
            const int pix = (img[i] * p.h_in + (yi >> p.up)) * p.w_in + sx;
            off[i] = ok ? static_cast<unsigned>(pix * ld + lchunk8) * 2u : GEMM_OOB;
        }
    }
    // The walk at K element k_first: the start of a split-K slice may lie at any tap and inside either source.
    template <typename F = NoOp> __device__ __forceinline__ void start(const GemmParams& p, int k_first, int lchunk8, F a32_rows = F()) {
        kg = k_first;
        tap = pin(kg / Ctot);
        cc = pin(kg - tap * Ctot);
        set_segment(p, lchunk8, a32_rows);
    }
    // Scalar offsets of the K block about to be requested and the descriptor of its activation source (rebuilt from scalars at the start of
    // every stage: carried across the loop as a variable it would live in VGPRs).
    __device__ __forceinline__ __amdgpu_buffer_rsrc_t stage_begin(const GemmParams& p, const unsigned short* a0, const unsigned short* a1, int& soff_a, int& soff_w) const {
        soff_a = __builtin_amdgcn_readfirstlane((seg1 ? cc - p.c0 : cc) * 2);
        soff_w = __builtin_amdgcn_readfirstlane(kg * 2);
        return __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(seg1 ? a1 : a0), 0, __builtin_amdgcn_readfirstlane(seg1 ? p.a1_bytes : p.a0_bytes), 0x00020000);
    }
    template <typename F = NoOp> __device__ __forceinline__ void stage_end(const GemmParams& p, int lchunk8, F a32_rows = F()) {
        kg = pin(kg + BK);
        cc = pin(cc + BK);
        tap = pin(tap);                                           // (a no-op in value: it keeps tap scalar across the branch below)
        if (cc == Ctot) { cc = 0; ++tap; set_segment(p, lchunk8, a32_rows); }
        else if (cc == p.c0) set_segment(p, lchunk8, a32_rows);
    }
};

}  // namespace pf
