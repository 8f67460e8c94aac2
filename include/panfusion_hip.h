/*
 * panfusion_hip.h -- C ABI of the MI355X-native (gfx950) PanFusion denoising hot path.
 *
 * Drop-in boundary.  The reference (chengzhag/PanFusion) is pure Python and has
 * no FFI of its own; the arithmetic on its denoising path lives in third-party CUDA wheels reached
 * through the call sites cited on every entry point below (paths relative to the reference tree).
 * This header is what a ctypes / cffi binding on the reference side binds (INTEGRATION.md shows
 * the stub); `panfusion_amd/_lib.py` is that binding for the in-tree Python host.
 *
 * Conventions
 *   - extern "C", plain pointers + sizes, no C++/torch types.  All data pointers are DEVICE
 *     pointers owned by the caller unless the name says `host_`.  Scratch is passed in
 *     (`workspace`, size from the matching *_workspace_size); the library owns NO device memory
 *     (per-camera constants of the geometry calls travel by value in the kernel arguments).
 *   - All work is enqueued on `stream` (a hipStream_t passed as void*); no implicit device sync,
 *     no allocation, host arrays (`host_*`) are consumed before the call returns.
 *   - Activations are token-major / NHWC: [image][y][x][channel]; MFMA operands are 16-bit (PF_BF16 or
 *     PF_F16); in the mixed scheme the residual-stream tensors are PF_F32 (the entry points that take a
 *     stream tensor say so).  Statistics, biases, tables and accumulators are fp32.
 *   - Every function returns pf_status; on failure pf_last_error_string() describes the problem
 *     (thread-local).  Arguments are validated before any launch.  Nothing throws or aborts.
 */
#ifndef PANFUSION_HIP_H
#define PANFUSION_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { PF_OK = 0, PF_ERR_ARG = 1, PF_ERR_LAUNCH = 2, PF_ERR_UNSUPPORTED = 3 } pf_status;
typedef enum { PF_BF16 = 0, PF_F16 = 1, PF_F32 = 2, PF_U8 = 3, PF_F64 = 4 } pf_dtype;

int pf_version(void);
const char* pf_last_error_string(void);

/* ------------------------------------------------------------------------------------------
 * Spherical geometry (replaces external/Perspective_and_Equirectangular/{e2p,p2e}.py and
 * models/pano/utils.py; angles in DEGREES as host doubles, one entry per camera).
 * ------------------------------------------------------------------------------------------ */

/* e2p.py:39-51 map_pers_pix_to_equi for `ncam` cameras: sampling position (pixel units of an
 * (eh,ew) panorama) of every pixel of an (h,w) view.  map_x/map_y: [ncam][h][w] fp32 (the
 * float64 result cast as e2p.py:74-75 does).  lonlat (optional, may be NULL): [ncam][h][w][2]
 * fp32 = e2p.py:9-36 map_pers_coords_to_equi (lon, lat) -- models/pano/utils.py:97-104. */
pf_status pf_e2p_grid(const double* host_fov, const double* host_theta, const double* host_phi,
                      int ncam, int eh, int ew, int h, int w,
                      float* map_x, float* map_y, float* lonlat, void* stream);

/* p2e.py:9-49 map_equi_pix_to_pers: for every pixel of an (h,w) panorama its position in the
 * (ph,pw) view (0 where invisible) and the visibility mask.  [ncam][h][w]. */
pf_status pf_p2e_grid(const double* host_fov, const double* host_theta, const double* host_phi,
                      int ncam, int ph, int pw, int h, int w,
                      float* map_u, float* map_v, uint8_t* mask, void* stream);

/* Dataset-side view cropping, external/py360convert/e2p.py:6-43 (called from utils/pano.py:160-161
 * Equirectangular.to_perspective, dataset/PanoDataset.py:133-140): `ncam` perspective crops (oh, ow) of ONE
 * equirectangular image img [H][W][C] (PF_U8 or PF_F32, channels last like the numpy array) -> out
 * [ncam][oh][ow][C], same dtype.  Per camera (host arrays, DEGREES): horizontal / vertical field of view,
 * yaw u, pitch v, in-plane rotation (may be NULL = 0).  order 0 = nearest, 1 = bilinear; sampling is
 * scipy.ndimage.map_coordinates(mode='wrap') on the pole-padded image (utils.py:120-133), restated bit for bit
 * (double accumulation; PF_U8 rounds half up and clamps like scipy's integer outputs). */
pf_status pf_py360_e2p(const void* img, int dtype, int H, int W, int C, const double* host_hfov,
                       const double* host_vfov, const double* host_u, const double* host_v,
                       const double* host_in_rot, int ncam, int oh, int ow, int order, void* out,
                       void* stream);

/* Cube maps, external/py360convert/e2c.py:6-40 (called from utils/pano.py:146-147 Equirectangular.to_cubemap): `n`
 * equirectangular images img [n][H][W][C] (PF_U8 or PF_F32, channels last) -> out [n][face_w][6 face_w][C], same
 * dtype: the reference's 'horizon' layout, faces F R B L U D side by side.  Rays are utils.py:5-37 xyzcube (float32
 * linspace(-0.5, 0.5, face_w) in-face coordinates); utils.py:82-114 xyz2uv / uv2coor are evaluated in double from
 * those float32 values (the reference evaluates them in float32; DESIGN.md 4.2 bounds the difference).  order 0 =
 * nearest, 1 = bilinear; the sampler is pf_py360_e2p's (pole rows, legacy 'wrap', scipy's uint8 store). */
pf_status pf_py360_e2c(const void* img, int dtype, int n, int H, int W, int C, int face_w, int order,
                       void* out, void* stream);

/* external/py360convert/c2e.py:6-64 (called from utils/pano.py:124-125 Cubemap.to_equirectangular; scripts/
 * stitch_mp3d.py makes every Matterport3D panorama with it): `n` cube maps cube [n][face_w][6 face_w][C] in horizon
 * layout (PF_U8 or PF_F32) -> out [n][h][w][C], w % 8 == 0.  out_dtype PF_F64 is what the reference returns for any
 * input dtype; PF_F32 / PF_U8 are numpy's astype of that result (PF_U8 truncates, as Equirectangular.save does).
 * host_ceil_rows: w / 4 host ints, the per-column U / D boundary rows of utils.py:47-64 equirect_facetype
 * (h // 2 - round(arctan(cos(linspace(-pi, pi, w // 4) / 4)) * h / pi)), computed by the caller with numpy so that
 * a rounding tie falls as in the reference; each must lie in [0, h].  In-face coordinates: c2e.py:40-57 in double
 * from the float32 utils.py:40-44 equirect_uvgrid values.  Sampling: utils.py:135-173 sample_cubefaces (faces R, B
 * flipped left-right, U up-down; two rows then two columns appended from the neighbouring faces; map_coordinates
 * mode='wrap', order 0 / 1) folded into addressing of the unpadded input; the zero-weight tap on the face axis is
 * not read. */
pf_status pf_py360_c2e(const void* cube, int dtype, int n, int face_w, int C, const int* host_ceil_rows,
                       int h, int w, int order, int out_dtype, void* out, void* stream);

/* Integer gather indices of kornia.remap(mode='nearest', align_corners=True) -> F.grid_sample
 * (e2p.py:76): idx[i] = iy*src_w+ix or -1 when the sample falls outside.  n entries. */
pf_status pf_nearest_indices(const float* map_x, const float* map_y, long n, int src_h, int src_w,
                             int32_t* idx, void* stream);

/* kornia.remap == grid_sample(zeros padding, align_corners=True) on NCHW images (e2p.py:76,
 * p2e.py:70-71).  src [B][C][hs][ws], maps [map_batch][ho][wo] (map_batch == B or 1), dst
 * [B][C][ho][wo]; mode 0 = nearest, 1 = bilinear; mask (optional) [map_batch][ho][wo]
 * multiplies the result (p2e.py:71).  dtype: PF_F32 / PF_F16 / PF_BF16 (same in and out). */
pf_status pf_remap(const void* src, int dtype, int B, int C, int hs, int ws,
                   const float* map_x, const float* map_y, const uint8_t* mask, int map_batch,
                   int ho, int wo, int mode, void* dst, void* stream);

/* external/Perspective_and_Equirectangular/mp2e.py:6-28 (called from dataset/PanoDataset.py:208-213 and
 * models/pano/MvDiffusion.py:144,157): `m` perspective views stitched into one panorama in ONE launch,
 *   out = sum_i p2e(img_i) p2e(tent_i) / sum_i p2e(tent_i),   `fill` where the denominator is 0,
 * both samples with the tensor p2e semantics of pf_p2e_grid + pf_remap (grid_sample, align_corners=True, zeros
 * outside, times the visibility mask), summed in fp32 over the cameras in index order: every term is the float
 * pf_remap returns, and the result does not depend on the launch geometry.  tent_i is the view-sized weight image
 * of mp2e.py:14-17, T[x] = float32(linspace(0, 1, pw/2)[x]) on the left half and float32(linspace(1, 0, pw/2)
 * [x - pw/2]) on the right (numpy rules, in double); feather 0 = T[x] (the reference), 1 = float32(T[x] Ty[y]) with Ty
 * the same tent over the rows.  pw must be even, and ph too with feather 1.  mp2e.py:19-21 (a blurred mask that is
 * never used) has no counterpart.
 *   src [B][m][C][ph][pw] (PF_F32 / PF_F16 / PF_BF16), out [B][C][H][W] fp32, weight (optional, may be NULL)
 *   [B][1][H][W] fp32 = the denominator.  Cameras: cam_batch * m host doubles each (degrees, fov in (0, 180)),
 *   cam_batch == B (per batch) or 1 (shared).  mode 0 = nearest, 1 = bilinear.
 * workspace: pf_mp2e_workspace_size(B, m) bytes of device memory, 8-byte aligned (the camera constants). */
size_t pf_mp2e_workspace_size(int B, int m);
pf_status pf_mp2e(const void* src, int dtype, int B, int m, int C, int ph, int pw,
                  const double* host_fov, const double* host_theta, const double* host_phi, int cam_batch,
                  int H, int W, int mode, int feather, float fill, float* out, float* weight,
                  void* workspace, size_t workspace_bytes, void* stream);

/* models/pano/utils.py:92-95: (lon,lat) of every pixel of an (H,W) panorama, [H][W][2] fp32. */
pf_status pf_equi_coords(int H, int W, float* lonlat, void* stream);

/* models/modules/transformer.py:185-201 SphericalPE.forward: coords [n][2] fp32, freq_bands
 * [nfreq] fp32 -> out [n][4*nfreq] fp32 = [sin(lon f) | sin(lat f) | cos(lon f) | cos(lat f)].
 * Full-range accurate sinf/cosf (frequencies reach 2^79). */
pf_status pf_spherical_pe(const float* coords, long n, const float* freq_bands, int nfreq,
                          float* out, void* stream);

/* models/pano/utils.py:10-84 get_masks, restated as shift-invariant tables: bias_x = mask + 1
 * in [0,2] (softmax is shift invariant per query row, and 98-99% of the entries are exactly 0).
 *   bias_e [E][m*P]   panorama pixel queries, keys ordered (view, y, x)   (modules.py:47)
 *   bias_p [m*P][E]   view pixel queries                                   (modules.py:53)
 *   flags_e [ceil(E/32)][ceil(m*P/32)], flags_p [ceil(m*P/32)][ceil(E/32)]: 1 where the 32x32
 *   tile of the table holds any non-zero.  E = eh*ew, P = ph*pw.  m = ncam. */
size_t pf_epa_tables_workspace_size(int ncam, int ph, int pw, int eh, int ew);
pf_status pf_epa_tables_build(const double* host_fov, const double* host_theta,
                              const double* host_phi, int ncam, int ph, int pw, int eh, int ew,
                              float* bias_e, float* bias_p, uint8_t* flags_e, uint8_t* flags_p,
                              void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Normalisation / element-wise (replace torch GroupNorm / LayerNorm / SiLU / GELU / F.pad /
 * torch.cat / torch.roll kernels reached from diffusers ResnetBlock2D, Transformer2DModel and
 * models/modules/transformer.py:151-162).
 * ------------------------------------------------------------------------------------------ */

/* GroupNorm statistics folded with the affine: for x [n_img][hw][C] (C = c0+c1 when two
 * sources are concatenated along channels, MVGenModel.py:231-233) writes scale/shift
 * [n_img][C] fp32 such that GN(x) = x*scale + shift.  workspace: pf_groupnorm_workspace_size.
 * dtype (both sources): PF_BF16 / PF_F16, or PF_F32 for the fp32 residual stream of the mixed scheme. */
size_t pf_groupnorm_workspace_size(int n_img, int hw, int C);
pf_status pf_groupnorm_stats(const void* x0, int c0, const void* x1, int c1, int dtype,
                             int n_img, int hw, int groups, float eps,
                             const float* gamma, const float* beta,
                             float* scale, float* shift, void* workspace, size_t workspace_bytes,
                             void* stream);

/* GroupNorm statistics of the tensor x [n_img][h][w][C] as if its width had been padded circularly by wrap_pad columns first
 * (the first and last wrap_pad columns count twice): what GroupNorm sees inside pad_pano(x, 2) -> ResnetBlock2D -> unpad_pano
 * of the panorama branch (MVGenModel.py:110-115), without the padded copy.  Workspace as pf_groupnorm_stats (hw = h * w). */
pf_status pf_groupnorm_stats_wrap(const void* x0, int c0, const void* x1, int c1, int dtype,
                                  int n_img, int h, int w, int wrap_pad, int groups, float eps,
                                  const float* gamma, const float* beta,
                                  float* scale, float* shift, void* workspace, size_t workspace_bytes,
                                  void* stream);

/* The same scale / shift from the per-column-pair moments a pf_conv_gemm epilogue left in pf_conv_desc.gn_partial: source s
 * is fp32 [n_img * hw / rows_s][2][c_s / 2] (rows_s = pf_conv_gemm_gn_rows of the launch that produced it); part1 = NULL: one
 * source.  (c0 + c1) / groups, c0 and c1 must be even.  No pass over the activation itself. */
pf_status pf_groupnorm_from_partials(const float* part0, int c0, int rows0, const float* part1, int c1, int rows1,
                                     int n_img, int hw, int groups, float eps, const float* gamma, const float* beta,
                                     float* scale, float* shift, void* stream);

/* The whole plan of one GroupNorm statistics problem: which of the three producers runs, with what chunking, grids and workspace. */
enum { PF_GN_DIRECT = 1, PF_GN_TWO_STAGE = 2, PF_GN_FROM_PARTIALS = 3 };
typedef struct {
    int arm;               /* PF_GN_DIRECT: one launch, a block per (image, group), for hw * C / groups <= PF_GN_DIRECT_MAX (32768; 0 = never;
                            * read once per process) and n_img * hw * C <= 4 Mi;  PF_GN_TWO_STAGE: chunk partials, then k_gn_finalize;
                            * PF_GN_FROM_PARTIALS: pf_groupnorm_from_partials;  0: refused -- every other member is 0                        */
    int partials_refused;  /* 1: moments were offered (rows0 > 0, and rows1 > 0 with a second source) but cannot serve -- odd channels per
                            * group or source, an image that is not whole runs of rows0 and rows1 rows, too many pairs per group -- so the
                            * plan is that of the statistics pass                                                                           */
    int ppc;               /* two-stage: pixels per chunk, 8 .. 64 (more where hw > 64 * 256, fewer where hw < 8)                             */
    int nchunks;           /* two-stage: chunks per image, ceil(hw / ppc)                                                                    */
    int pix_par;           /* two-stage: pixels a block reads in parallel, 256 / min(C / 8, 256)                                             */
    unsigned lds_bytes;    /* two-stage: dynamic LDS of k_gn_partial, 2 fp32 arrays [pix_par][C]; refused above 64 KiB                       */
    int gpb;               /* from partials: groups per block, 8 / 4 / 2 / 1 by parts per image, halved until a block holds <= 512 pairs     */
    int pairs_per_block;   /* from partials: column pairs of a full block, gpb * C / groups / 2 (a ragged last block holds fewer)            */
    int slices;            /* from partials: slices of the parts that walk them side by side in a full block, 256 / pairs_per_block
                            * (1 above 128 pairs) -- the number k_gn_finalize_cols derives for itself                                        */
    unsigned grid_x, grid_y;   /* the first launch: (n_img, groups) direct, (nchunks, n_img) two-stage, (n_img, ceil(groups / gpb)) partials */
    unsigned grid2_x, grid2_y; /* two-stage: k_gn_finalize, (n_img, ceil(groups / 8)); otherwise 0                                          */
    size_t workspace_bytes;    /* what pf_groupnorm_stats / _wrap require (of the direct arm too: n_img * nchunks * 128 floats); partials: 0  */
} pf_gn_plan;
/* Reads no pointer and needs no GPU.  rows0 / rows1: rows per part of the moments attached to the sources (0: none; rows1 is not looked
 * at when c1 = 0).  A circular wrap (pf_groupnorm_stats_wrap) changes only the counted pixels: its plan is that of hw = h * w without
 * moments.  PF_ERR_ARG, the launch's own message and an all-zero plan for a problem the launch refuses. */
pf_status pf_groupnorm_plan(int n_img, int hw, int c0, int c1, int groups, int dtype, int rows0, int rows1, pf_gn_plan* out);

/* y = act(x*scale + shift), act 0 = identity, 1 = SiLU (scale = shift = NULL: y = act(x)).  Same concat
 * convention.  dtype = type of the sources (16-bit or PF_F32).  Output:
 *   out_dtype 16-bit, out_split 0:  y [n_img][hw][C]
 *   out_dtype 16-bit, out_split 1:  y [n_img][hw][2C]: per block of 32 channels [hi(32) | lo(32)], hi = round16(v),
 *                                   lo = round16(v - hi) (C %% 32 == 0): the A operand of a split-precision GEMM
 *                                   (pf_conv_desc.split3: A_hi W_hi + A_lo W_hi + A_hi W_lo reproduce the fp32
 *                                   product to ~2^-22)
 *   out_dtype PF_F32:               y [n_img][hw][C] fp32. */
pf_status pf_scale_shift_act(const void* x0, int c0, const void* x1, int c1, int dtype,
                             int n_img, int hw, const float* scale, const float* shift, int act,
                             int out_dtype, int out_split, void* y, void* stream);
/* fp32 sources, 16-bit y as above, PLUS the un-normalised input as the split pair raw_pair [n_img][hw][2C] (same layout)
 * in the same pass (the A operand of a ResnetBlock2D's split-precision conv_shortcut next to norm1 + SiLU of the same
 * tensor: one read of the fp32 stream instead of two). */
pf_status pf_scale_shift_act_pair(const void* x0, int c0, const void* x1, int c1, int n_img, int hw,
                                  const float* scale, const float* shift, int act, int out_dtype, void* y,
                                  void* raw_pair, void* stream);

/* y = LayerNorm(x + pe) * gamma + beta over the last dim; x,y [rows][C]; pe (optional) fp32
 * [pe_rows][C], row r uses pe row (r % pe_rows) (transformer.py:155-158; eps 1e-5).
 * dtype: type of x (16-bit == out_dtype, or PF_F32); out_dtype: 16-bit type of y. */
pf_status pf_layernorm(const void* x, const float* pe, long pe_rows, int dtype, long rows, int C,
                       const float* gamma, const float* beta, float eps, int out_dtype, void* y, void* stream);
/* The plan of pf_layernorm and pf_layernorm_bwd (below) on [rows][C]. */
typedef struct {
    int rows_per_wave;   /* forward: 4 rows per wavefront in flight for C <= 512 and rows >= 4096, else 1                                  */
    unsigned grid_x;     /* forward: blocks of 4 wavefronts, ceil(rows / (4 rows_per_wave))                                               */
    int bwd_parts;       /* backward: blocks, each leaving one row of the [2][bwd_parts][C] partials: ceil(rows / 4), at most 512         */
} pf_ln_plan;
/* Reads no pointer.  PF_ERR_ARG, the launch's message and an all-zero plan for rows <= 0 or a C that either direction refuses. */
pf_status pf_layernorm_plan(long rows, int C, pf_ln_plan* out);

/* Sampling of the VAE posterior (diffusers DiagonalGaussianDistribution.sample, PanoGenerator.py:214-225):
 * moments fp32 NHWC [n][hw][2L] = (mean | logvar), eps fp32 NCHW [n][L][hw] ->
 * z NCHW [n][L][hw] = (mean + exp(0.5 * clamp(logvar, -30, 20)) * eps) * scale. */
pf_status pf_vae_sample(const float* moments, const float* eps, int n, int L, long hw, float scale, float* z, void* stream);

/* out = a * x + b * y on n fp32 elements (scheduler.add_noise of the training step, PanFusion.py:83-84:
 * sqrt(abar_t) * latents + sqrt(1 - abar_t) * noise). */
pf_status pf_axpby(const float* x, const float* y, float a, float b, long n, float* out, void* stream);

/* GEGLU: in [rows][2*inner] = [a | gate] -> out [rows][inner] = a * gelu(gate) (erf GELU). */
pf_status pf_geglu(const void* in, int dtype, long rows, int inner, void* out, void* stream);

/* Sinusoidal timestep features [cos | sin] (diffusers Timesteps, flip_sin_to_cos, shift 0)
 * followed by nothing: t [n] int64 -> out [n][dim] in `dtype`. */
pf_status pf_timestep_features(const int64_t* t, int n, int dim, int out_dtype, void* out, void* stream);
/* The same with the n timesteps t_stride words apart: `timestep[:, 0]` of the (b, m) tensor the reference hands the panorama
 * branch (MVGenModel.py:49-50, :85) read in place -- no strided-copy kernel in the step. */
pf_status pf_timestep_features_strided(const int64_t* t, long t_stride, int n, int dim, int out_dtype, void* out, void* stream);

/* y = silu(x) element-wise, n elements. */
pf_status pf_silu(const void* x, int dtype, long n, void* y, void* stream);

/* Circular width pad (utils/pano.py:74-99) and crop (:102-105) on NHWC: x [n][h][w][C], 16-bit or PF_F32. */
pf_status pf_pad_width(const void* x, int dtype, int n, int h, int w, int C, int pad, void* y, void* stream);
pf_status pf_crop_width(const void* x, int dtype, int n, int h, int w, int C, int crop, void* y, void* stream);

/* The reference's pad_pano on NCHW tensors (utils/pano.py:74-99): x [rows][w] -> y [rows][w+2 pad],
 * circular; elem_bytes 2 or 4. */
pf_status pf_pad_width_rows(const void* x, int elem_bytes, long rows, int w, int pad, void* y, void* stream);
/* torch.roll(x, shift, dims=-1) of rotate_latent (PanoGenerator.py:264-269): y[r][(i+shift) mod w] = x[r][i]. */
pf_status pf_roll_width_rows(const void* x, int elem_bytes, long rows, int w, int shift, void* y, void* stream);

/* Layout/precision converters at the boundary: NCHW (src_dtype) <-> NHWC (dst_dtype). */
pf_status pf_nchw_to_nhwc(const void* x, int src_dtype, int n, int C, int h, int w, int dst_dtype, void* y, void* stream);
pf_status pf_nhwc_to_nchw(const void* x, int src_dtype, int n, int C, int h, int w, int dst_dtype, void* y, void* stream);

/* y = a + b element-wise (ControlNet residual adds, MVGenModel.py:154-170,200-203); a and y of type
 * dtype_a, b of type dtype_b (any of PF_BF16 / PF_F16 / PF_F32). */
pf_status pf_add(const void* a, int dtype_a, const void* b, int dtype_b, long n, void* y, void* stream);

/* Token + position embedding of the CLIP text encoder (transformers CLIPTextEmbeddings, reached from
 * PanoGenerator.py:197-211 encode_text): ids int64 [B][L] -> out [B][Lp][C] (out_dtype 16-bit or PF_F32),
 * out[b][t] = tok[ids[b][t]] + pos[t] for t < L, zero rows for L <= t < Lp (the sequence is padded to a
 * multiple of 4 keys for the masked attention).  tok [vocab][C], pos [>= L][C] fp32. */
pf_status pf_embed_tokens(const int64_t* ids, int B, int L, int Lp, int C, long vocab, const float* tok,
                          const float* pos, int out_dtype, void* out, void* stream);

/* Row softmax of fp32 scores: probs[r][j] = exp(scale (s[r][j] - max_j)) / sum_j, 16-bit out.  The VAE decoder's
 * mid-block attention has ONE head of width 512 (diffusers Attention in AutoencoderKL, reached from
 * PanoGenerator.py:213-220 decode_latent): its scores and the P.V product run on pf_conv_gemm (batched), this
 * kernel sits between them.  scores [rows][scores_ld] fp32, probs [rows][probs_ld] (out_dtype 16-bit). */
pf_status pf_softmax_rows(const float* scores, long rows, int n, long scores_ld, float scale, int out_dtype,
                          void* probs, long probs_ld, void* stream);

/* models/modules/utils.py:9-15 tensor_to_image: x fp32 NCHW in [-1, 1] -> y uint8 NHWC,
 * round((x / 2 + 0.5).clamp(0, 1) * 255) (half to even, like torch.round). */
pf_status pf_tensor_to_image(const float* x, int n, int C, int h, int w, uint8_t* y, void* stream);

/* Fused classifier-free-guidance merge + DDIM update (+ optional width roll of the result):
 * eps = eps_uncond + g*(eps_cond - eps_uncond)                (PanoGenerator.py:253-262)
 * x0 = (x - sqrt(1-a_t) eps)/sqrt(a_t); x' = sqrt(a_prev) x0 + sqrt(1-a_prev) eps  (DDIM eta=0)
 * out[..., (w + roll) mod W] = x'                              (PanoGenerator.py:264-269)
 * x, out: fp32 [n_img][C][H][W]; eps_uncond/eps_cond fp32 same shape. */
pf_status pf_cfg_ddim_step(const float* x, const float* eps_uncond, const float* eps_cond,
                           float guidance, float sqrt_a_t, float sqrt_1m_a_t, float sqrt_a_prev,
                           float sqrt_1m_a_prev, long rows, int W, int roll, float* out, void* stream);

/* The same update as ONE launch per latent with everything the NEXT denoiser call needs (round 5: no torch.cat / copy_ / fill_
 * kernels between two calls of the loop, PanFusion.py:149-162): out may alias x for ANY roll (a block owns whole rows);
 * out2 (or NULL) receives a second copy -- the other half of the CFG pair torch.cat([x] * 2) of PanoGenerator.py:240-251;
 * tstep (or NULL): n_tstep int64 words (n_tstep > 0) set to t_next, the timestep tensor of the next call (PanFusion.py:147).
 *
 * The rules of all four pf_cfg_*_step_pair entry points (one kernel, one launcher; each adds operands to the one before it).
 * Forms: DDIM (x0_out == NULL; x0_prev must be NULL too): one row staged in LDS, W <= 16384; 2M (x0_out != NULL): two rows,
 * W <= 8192.  rows < 2^31.  One block per row reads its rows in full before it writes them: out may alias x, and x0_out may alias
 * x0_prev, for any roll.  Nothing else may overlap: out2 must not alias x / out; out must not alias the predictions; x0_out must
 * not alias x, the predictions, out or out2; x0_prev must not alias out / out2; known / noise / mask (given together or NULL
 * together) must not alias out, out2 or x0_out -- they are read at an offset.  A call that breaks a rule returns PF_ERR_ARG
 * before any launch, with a message that names the entry point called and the argument. */
pf_status pf_cfg_ddim_step_pair(const float* x, const float* eps_uncond, const float* eps_cond,
                                float guidance, float sqrt_a_t, float sqrt_1m_a_t, float sqrt_a_prev,
                                float sqrt_1m_a_prev, long rows, int W, int roll, float* out, float* out2,
                                int64_t* tstep, int n_tstep, int64_t t_next, void* stream);

/* pf_cfg_ddim_step_pair with the DPM-Solver++(2M) multistep update (diffusers DPMSolverMultistepScheduler,
 * algorithm_type="dpmsolver++", solver_order=2, solver_type="midpoint": multistep_dpm_solver_second_order_update) in the
 * loop of PanFusion.py:146-162.  With alpha = sqrt(a), sigma = sqrt(1-a), lambda = log alpha - log sigma, s0 = the current
 * timestep, t = its target, s1 = the previous step's timestep, h = lambda_t - lambda_s0, r0 = (lambda_s0 - lambda_s1) / h:
 *   x_t = (sigma_t/sigma_s0) x - alpha_t (e^-h - 1) D0 - 1/2 alpha_t (e^-h - 1) D1,  D0 = x0, D1 = (x0 - x0_prev) / r0
 * whose first two terms are the DDIM update; the kernel computes
 *   out = DDIM(x, eps) + k (x0 - x0_prev),  k = 1/2 alpha_t (1 - e^-h) / r0  (host: float64, passed as fp32)
 * with eps, x0 and DDIM(x, eps) in the operation sequence of pf_cfg_ddim_step_pair, and writes x0 to x0_out[(w + roll) mod W]
 * -- the history rolls with the state, into the frame of the next call.  x0_prev == NULL: a first-order step (k unused, the
 * history not read), out bit-identical to pf_cfg_ddim_step_pair.  x0_out is required (the 2M form of the rules above);
 * x0_prev / x0_out fp32, the shape of x. */
pf_status pf_cfg_dpmpp_step_pair(const float* x, const float* eps_uncond, const float* eps_cond,
                                 float guidance, float sqrt_a_t, float sqrt_1m_a_t, float sqrt_a_prev,
                                 float sqrt_1m_a_prev, long rows, int W, int roll, float* out, float* out2,
                                 int64_t* tstep, int n_tstep, int64_t t_next, const float* x0_prev, float k,
                                 float* x0_out, void* stream);

/* The loop's update with a known region (inpainting / outpainting at strength 1): diffusers StableDiffusionInpaintPipeline
 * 0.24, the 4-channel branch, in the loop of PanFusion.py:159-162.  After the DDIM update (x0_out == NULL, the operation
 * sequence of pf_cfg_ddim_step_pair) or the 2M update (x0_out != NULL, that of pf_cfg_dpmpp_step_pair, x0 written as there)
 * every element is blended with the known latent z:
 *   v <- fmaf(m, v, (1 - m) * fmaf(ka, z, kb * n)),  (ka, kb) = (sqrt abar(t_next), sqrt(1 - abar(t_next))), (1, 0) at the last step
 * i.e. m v + (1 - m) add_noise(z, n, t_next); m = 1 generates, m = 0 keeps (diffusers' convention); n = the loop's starting
 * latents.  m = 1 gives the unblended value and m = 0 with (1, 0) gives z, bit for bit (finite operands).  The x0 history is
 * the model's x0 of the blended state: the blend does not touch it.
 * Frames: known / noise / mask stay in the caller's frame and are read at column (w - known_roll) mod W -- the panorama passes
 * the sum of the integer rolls its state has gone through before this update (PanoGenerator.py:264-269: (i + 1) shift mod W at
 * step i), the views 0; the blended value is written at (w + roll) mod W as by the other update kernels.
 * known / noise / mask are required (fp32, the shape of x; the host expands a per-pixel mask over the channels); either form
 * of the rules above. */
pf_status pf_cfg_inpaint_step_pair(const float* x, const float* eps_uncond, const float* eps_cond,
                                   float guidance, float sqrt_a_t, float sqrt_1m_a_t, float sqrt_a_prev,
                                   float sqrt_1m_a_prev, long rows, int W, int roll, float* out, float* out2,
                                   int64_t* tstep, int n_tstep, int64_t t_next, const float* x0_prev, float k,
                                   float* x0_out, const float* known, const float* noise, const float* mask,
                                   float ka, float kb, int known_roll, void* stream);

/* Guidance rescale (Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps are Flawed", §3.4; diffusers 0.24
 * pipeline_stable_diffusion.py: rescale_noise_cfg) applied to the merge of PanoGenerator.py:253-262
 * (combine_cls_free_guide_pred) on the tensors of PanFusion.py:156-162, one statistic per sample over all of its views, the
 * panorama a separate one:
 *   eps = f eps_cfg,  f = phi std(eps_cond) / std(eps_cfg) + 1 - phi = phi sqrt(M2_text / M2_cfg) + 1 - phi,
 *   M2(v) = sum (v - mean v)^2  (the N - 1 of torch's unbiased std cancels in the ratio and appears nowhere).
 * pf_cfg_moments is the first of two launches: for each of n_samples samples of sample_elems contiguous fp32 elements it
 * writes n_partials records of PF_CFG_MOMENT_DOUBLES = 4 float64 sums
 *   partials[s][p] = (sum c, sum c^2, sum e, sum e^2),  c = eps_cond, e = fmaf(guidance, c - u, u)
 * -- e is the very fp32 value the update kernels form -- over the elements [p chunk, min((p + 1) chunk, sample_elems)) of
 * sample s, chunk = ceil(sample_elems / n_partials): a function of (sample_elems, n_partials) alone (an empty range gives
 * zeros).  mean = sum / N and M2 = sum v^2 - (sum v)^2 / N follow from the records added in index order.  Plain float64 sums:
 * fp32 squares are exact in float64 and N < 2^31 of them lose < 1e-12 relative, so M2 is good to ~1e-12 (mean / std)^2 --
 * ample for noise predictions, whose mean is a fraction of their std.  Fixed accumulation order (thread t takes elements
 * t, t + 256, ... of its chunk, then a butterfly over the lanes and the wavefronts in index order), no atomics: every launch
 * on the same inputs writes the same bits.  2 <= sample_elems < 2^31, 1 <= n_partials <= PF_CFG_MAX_PARTIALS,
 * 1 <= n_samples <= 65535; partials: caller-owned, n_samples * n_partials * 4 doubles. */
#define PF_CFG_MOMENT_DOUBLES 4
#define PF_CFG_MAX_PARTIALS 256
pf_status pf_cfg_moments(const float* eps_uncond, const float* eps_cond, float guidance, int n_samples, long sample_elems,
                         double* partials, int n_partials, void* stream);

/* The second launch: pf_cfg_inpaint_step_pair's update on the rescaled prediction.  known / noise / mask are given together or
 * are NULL together (NULL: no blend -- pf_cfg_ddim_step_pair with x0_out == NULL, pf_cfg_dpmpp_step_pair otherwise).  The block
 * of row r adds the n_partials records of sample r / sample_rows in index order in float64, forms
 *   f = (float)(phi sqrt(M2_text / M2_cfg) + (1 - phi)),  N = sample_rows W;   M2_cfg <= 0 (a constant prediction): f = 1
 * (diffusers returns NaN there), then eps = f * fmaf(guidance, c - u, u) and the operation sequence of the other update
 * kernels from eps on: x0 (and the 2M history x0_out) is the x0 of the RESCALED eps, as in diffusers, whose scheduler only ever
 * sees the rescaled prediction.  Every block of a sample runs the same float64 operations on the same records, hence
 * multiplies by the same bits of f; phi = 0 gives f = 1 exactly and the outputs of the corresponding existing kernel bit for
 * bit.  factor_out (or NULL): f per sample, rows / sample_rows floats, written by the block of the sample's first row.
 * Refused besides what the rules above refuse: sample_rows not dividing rows, a sample of fewer than 2 elements, phi outside
 * [0, 1] or NaN, partials == NULL, n_partials outside [1, PF_CFG_MAX_PARTIALS]. */
pf_status pf_cfg_rescaled_step_pair(const float* x, const float* eps_uncond, const float* eps_cond,
                                    float guidance, float sqrt_a_t, float sqrt_1m_a_t, float sqrt_a_prev,
                                    float sqrt_1m_a_prev, long rows, int W, int roll, float* out, float* out2,
                                    int64_t* tstep, int n_tstep, int64_t t_next, const float* x0_prev, float k,
                                    float* x0_out, const float* known, const float* noise, const float* mask,
                                    float ka, float kb, int known_roll, const double* partials, int n_partials,
                                    long sample_rows, float phi, float* factor_out, void* stream);

/* The start state of a sampling run in ONE launch (PanFusion.py:30-43,146-149: the noise the loop starts from, its first roll
 * and timestep tensor; PanoGenerator.py:240-251,264-269: the CFG pair [x ; x] and the integer roll), for a start below
 * strength 1 (diffusers' img2img / inpaint pipelines: latents = scheduler.add_noise(image_latents, noise, latent_timestep)) and
 * for re-arming a loop whose captured graphs read the state by address:
 *   out[r][(w + roll) mod W] = fmaf(ka, z[r][w], kb * noise[r][w]),  (ka, kb) = (sqrt abar(t_s), sqrt(1 - abar(t_s)))
 * -- the expression pf_cfg_inpaint_step_pair uses for its blend operand, so a kept pixel starts on the value the blend would
 * write -- and the same value to out2 (or NULL), the other half of the CFG pair.  z == NULL: out = noise rolled, a bit-exact
 * copy (ka, kb unused).  tstep (or NULL): n_tstep int64 words set to t0, the timestep tensor of the first call.
 * One block per row, the row staged in LDS: W <= 16384.  z / noise fp32, rows x W; out / out2 must not alias z, noise or each
 * other. */
pf_status pf_noised_start_pair(const float* z, const float* noise, float ka, float kb, long rows, int W, int roll,
                               float* out, float* out2, int64_t* tstep, int n_tstep, int64_t t0, void* stream);

/* pf_noised_start_pair with z read from a SMALLER source: the start state of the second pass of two-pass high-resolution
 * sampling ("hires fix": compose at the native size, up-sample the latents, re-noise, run the tail of the schedule).
 * z: planes images (n * C) of h_src x w_src, fp32; the output is planes x H x W with H = fh h_src, W = fw w_src, fh and fw
 * integers >= 1 (anything else is an error):
 *   out[p][y][(w + roll) mod W] = fmaf(ka, r, kb * noise[p][y][w]),   r = resize(z[p])[y][w]
 * and the same value to out2 (or NULL); noise == NULL: out = r itself, a pure resize (ka, kb unused).  tstep as above.
 * resize is torch.nn.functional.interpolate(mode = nearest (0) / bilinear (1) / bicubic (2), align_corners=False, no
 * antialiasing, cubic A = -0.75).  Rows clamp at the top and bottom.  wrap = 1: columns are periodic (a panorama latent: the
 * taps of the output columns near 0 and W - 1 come from the other side of the source); wrap = 0: columns clamp (a view).
 * The weights of an output index dst = q f + p depend on its phase p alone -- t = (2p + 1 - f) / (2f), its floor and its
 * fraction, from integers -- so with wrap = 1 a source rolled by k columns gives the output rolled by k fw, bit for bit.  r is a
 * complete fp32 value before the fmaf, the expression pf_noised_start_pair and the inpaint blend use: the result equals
 * pf_noised_start_pair on the resized z bit for bit.
 * One block per output row; the output row and the row-resampled source row are staged in LDS: W <= 2048 (16 KB at the limit).
 * out / out2 must not alias z, noise or each other. */
pf_status pf_upsampled_start_pair(const float* z, const float* noise, float ka, float kb, long planes, int h_src, int w_src,
                                  int H, int W, int mode, int wrap, int roll, float* out, float* out2, int64_t* tstep,
                                  int n_tstep, int64_t t0, void* stream);

/* ------------------------------------------------------------------------------------------
 * MFMA GEMM / implicit-GEMM convolution (replaces cuDNN/cuBLAS behind diffusers Conv2d/Linear:
 * MVGenModel.py:86-144,174-198,224-294 and transformer.py:57-74,8-38).
 *   out[m][n] = sum_k A[m][k] * W[n][k]  (+ bias[n]) (+ rowvec[img(m)][n]) (+ residual[m][n])
 * A is gathered on the fly: m = (img, yo, xo), k = (ky, kx, c); zero padding; optional nearest
 * x2 upsampling of the input (Upsample2D) and optional channel concat of two sources.
 * A plain linear layer is ksize = 1, n_img = 1, h_in = 1, w_in = rows.
 * Requirements: (c0 + c1) % 64 == 0, c0 % 64 == 0; pointers 16-byte aligned; ld's % 8 == 0.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    const void* a0;      /* source 0, [n_img][h_in][w_in][a0_ld]                            */
    const void* a1;      /* source 1 (channel concat after source 0) or NULL                */
    int c0, c1;          /* channels taken from each source                                 */
    int a0_ld, a1_ld;    /* per-pixel stride in elements (>= c0 / c1)                       */
    int n_img, h_in, w_in;
    int h_out, w_out;    /* output spatial size: (h + 2 pad - k) / stride + 1, or that of the input with ONE more zero
                          * row and column at the bottom / right (F.pad(x, (0,1,0,1)) + conv, the VAE encoder's
                          * Downsample2D(padding=0)): pixels past the input read as zero                       */
    int ksize;           /* 1 or 3                                                          */
    int stride;          /* 1 or 2                                                          */
    int pad;             /* 0 or 1 (zeros)                                                  */
    int upsample;        /* 1: input is nearest-upsampled x2 before the convolution         */
    const void* w;       /* [n_out][ksize*ksize*(c0+c1)], k ordered (ky, kx, c)             */
    int n_out;
    const float* bias;   /* [n_out] or NULL                                                 */
    const float* rowvec; /* [n_img][rowvec_ld] added per image (time embedding) or NULL     */
    int rowvec_ld;
    const void* residual;/* [M][res_ld] (res_dtype) or NULL                                 */
    int res_ld;
    int res_dtype;       /* == dtype, or PF_F32: the fp32 residual stream of the mixed scheme */
    void* out;           /* [M][out_ld]                                                     */
    int out_ld;
    int out_dtype;       /* PF_BF16 / PF_F16 (== dtype) or PF_F32                           */
    int dtype;           /* PF_BF16 or PF_F16: A, W, residual                               */
    int batch;           /* >= 1: independent problems, strides below (elements)            */
    long a_bstride, w_bstride, out_bstride, res_bstride;
    int epilogue;        /* PF_EPILOGUE_NONE; PF_EPILOGUE_GEGLU: W rows interleaved (value_j, gate_j),
                          * out [M][n_out/2] = value * gelu(gate) (transformer.py:8-21, erf GELU);
                          * PF_EPILOGUE_SPLIT: out is the 16-bit pair [M][2 n_out] of the fp32 result, per block of 32
                          * columns [hi(32) | lo(32)] (hi = round16(v), lo = round16(v - hi)), out_ld >= 2 n_out,
                          * n_out %% 32 == 0: the A operand of a following split3 GEMM without a separate split pass */
    void* workspace;     /* split-K scratch (may be NULL: no split) of pf_conv_gemm_workspace_size   */
    size_t workspace_bytes;
    float* gn_partial;   /* optional by-product (NULL: none): GroupNorm moments of the OUTPUT for the next layer's
                          * norm (diffusers ResnetBlock2D.norm1 / norm2, Transformer2DModel.norm; call sites
                          * MVGenModel.py:102-144,174-198,224-277), so that no statistics pass re-reads the tensor:
                          * fp32 [M / R][2][n_out / 2] = (sum, sum of squares) of each column PAIR (2 k, 2 k + 1) over each run of R output rows,
                          * R = pf_conv_plan.gn_rows of pf_conv_gemm_plan(desc, 1) (> 0: possible for this problem; images are whole runs).
                          * The caller states the R it sized the buffer for in gn_rows below: a launch whose plan resolves to another
                          * R fails with PF_ERR_ARG before anything is written.
                          * Consumed by pf_groupnorm_from_partials.  Fixed summation order, no atomics.      */
    int wrap_pad;        /* 0..2: the input is read as if its WIDTH had been padded circularly by wrap_pad columns on both
                          * sides first (pad_pano, utils/pano.py:74-99), in pre-upsampling columns; the zero padding `pad`
                          * applies outside that virtual tensor.  No padded copy exists.                              */
    int crop;            /* 0..2: output columns cropped by `crop` on both sides (unpad_pano, utils/pano.py:102-105):
                          * w_out = ((w_in + 2 wrap_pad) << upsample + 2 pad - ksize) / stride + 1 - 2 crop.
                          * Together: pad_pano(x, p) -> conv -> unpad_pano(., c) of the panorama branch in one launch
                          * (MVGenModel.py:110-115 resnets p = c = 2 [conv1: wrap 2 / crop 0, conv2: wrap 0 / crop 2 on the
                          * padded intermediate], :138-144 down-sampling 2 / 1, :272-277 up-sampling 1 / 2).           */
    int* tickets;        /* optional (NULL: the split-K slabs are combined by a second kernel): n_tickets int32 arrival counters,
                          * ALL ZERO when the call is enqueued and zero again when it has run, not shared with a launch that may
                          * run concurrently -- the K-slice workgroup that arrives last combines the slabs inside the launch
                          * (same sums in split order as the second kernel: bit-identical).  n_tickets >= tiles x batch of the
                          * split launch (<= 1024 for every plan this library makes).                                  */
    int n_tickets;
    int split3;          /* split-precision walk: a0 is a PAIR tensor -- per block of 32 channels [hi(32) | lo(32)], c0 = 2 x channels (what
                          * pf_scale_shift_act(out_split) / PF_EPILOGUE_SPLIT write) -- and w holds per tap and block of 32 channels
                          * [W_hi(32) | W_lo(32)]; every 64-element K block is multiplied as W_hi A_hi + W_hi A_lo + W_lo A_hi (2^-22
                          * relative: an fp32-grade product from 16-bit MFMA operands).  a1 must be NULL.                       */
    int subpixel;        /* 1: a nearest-x2-upsampling 3x3 convolution (ksize 3, upsample 1, stride 1, pad 1; diffusers Upsample2D:
                          * F.interpolate(scale_factor=2, mode="nearest") + Conv2d, reference call sites MVGenModel.py:272-277) computed as FOUR 2x2
                          * convolutions on the LOW-resolution grid, one per output phase (a, b) in {0, 1}^2: output pixel (2 y + a, 2 x + b) only
                          * ever reads input rows y - 1 + a, y + a and columns x - 1 + b, x + b, so the nine taps collapse to four with summed
                          * weights -- 4 instead of 9 MACs per (output value, input channel), the same sums in exact arithmetic.  `w` then holds
                          * [4 phases][n_out][2][2][c0 + c1] (phase-major, 16-bit; panfusion_amd.engine._subpixel_weight builds it: row taps of
                          * phase a = 0: {W[0]}, {W[1] + W[2]}; a = 1: {W[0] + W[1]}, {W[2]}; columns alike).  Bias only (no row vector,
                          * residual, GEGLU / pair epilogue; split3 allowed: c0 = 2 x channels per tap), batch 1, h_out / w_out even; wrap_pad 0..1 with crop 2 x wrap_pad is the
                          * panorama's pad 1 / upsample / conv / crop 2.  gn_partial is supported (runs of R LOW-resolution rows).            */
    int gn_rows;         /* with gn_partial: the rows per moment run R that gn_partial was sized for (pf_conv_plan.gn_rows); else unused */
    int a_src_dtype;     /* 0: a0 / a1 hold `dtype` elements (everything above).  PF_F32 (with split3 = 1, ksize = 1, batch = 1): a0 / a1 are the
                          * fp32 stream tensors THEMSELVES, [rows][a0_ld] / [rows][a1_ld] fp32 with c0 / c1 fp32 channels (multiples of 32; a1
                          * allowed: x | skip), and the kernels form the pair in registers while they stage a K block -- v = a, or
                          * v = fma(a, a_scale[img][c], a_shift[img][c]); hi = round16(v), lo = round16(v - hi) -- instead of reading a pair
                          * tensor that pf_scale_shift_act(out_split) wrote.  Same bytes in, no pair tensor; w, the plan (K = 2 (c0 + c1)) and
                          * the result are those of the pair form, bit for bit.                                                            */
    const float* a_scale;/* with a_src_dtype = PF_F32: optional GroupNorm scale [n_img][c0 + c1] fp32 (pf_groupnorm_scale_shift), image of a
                          * row = row / (h_out * w_out); NULL: the sources are split as they are                                         */
    const float* a_shift;/* given exactly when a_scale is                                                                                */
} pf_conv_desc;

enum { PF_EPILOGUE_NONE = 0, PF_EPILOGUE_GEGLU = 1, PF_EPILOGUE_SPLIT = 2 };

/* Bytes of fp32 scratch that let pf_conv_gemm split the K range of a problem whose output grid alone
 * cannot fill the 256 CUs (the 8x8 / 16x16 levels and the whole panorama branch); 0 = not wanted.
 * The slabs are summed in split order by a second kernel: results do not depend on scheduling. */
size_t pf_conv_gemm_workspace_size(const pf_conv_desc* desc);
/* Rows per moment run R of pf_conv_desc.gn_partial for this problem, or 0 when the kernel that serves it cannot emit
 * the moments (split-K plans, batches, GEGLU / pair epilogues, images that are not whole runs of R rows). */
int pf_conv_gemm_gn_rows(const pf_conv_desc* desc);
/* Diagnostics / tests / the benchmark's shape classes: which tile kernel pf_conv_gemm's plan gives this problem --
 * 0 the 4-wave 16x16x32 kernel (2 blocks per CU), 1 the persistent 8-wave 16x16x32 kernel (256 x 160 tiles),
 * 2 the persistent 32x32x16 kernel of round 6 (256 x 320 tiles, pf_gemm32.hip); -1 for a bad descriptor.  Like the two
 * queries above it reflects the plan only (workspace assumed available), it validates nothing.  The cuDNN / cuBLAS
 * heuristics behind diffusers Conv2d / Linear are what it stands in for (MVGenModel.py:102-144,174-198,224-277). */
int pf_conv_gemm_kernel_id(const pf_conv_desc* desc);
/* The whole plan pf_conv_gemm resolves for a problem: everything that selects a kernel instantiation or sizes a buffer.  The three
 * queries above are projections of it (workspace_size: the larger workspace_bytes of the plans with and without moments; gn_rows: that of
 * the plan with moments; kernel_id: the kernel of the plan without). */
typedef struct {
    int kernel;          /* 0 the 4-wave 16x16x32 kernel, 1 the persistent 8-wave 16x16x32 kernel, 2 the persistent 32x32x16 kernel */
    int mrep, nrep;      /* the block's tile is (32 mrep) x (32 nrep) outputs (kernel 0: mrep 2 or 4; 1: 8; 2: 8 x 10)            */
    int block_rows;      /* output rows of a block: 32 mrep; kernel 1 also runs 128-row blocks, two per CU                         */
    int waves;           /* wavefronts per block: 4 (kernel 0, 128-row blocks of kernel 1) or 8                                    */
    int ring_slots;      /* operand stages in LDS: 2, 3 or 4                                                                       */
    int splits;          /* K slices of the launch (1: not split), each of kb_per_split 64-element K blocks                        */
    int kb_per_split;
    int m_split;         /* > 0: rows [0, m_split) run unsplit, then rows [m_split, M) in tail_splits K slices of tail_kb blocks   */
    int tail_splits, tail_kb;
    int gn_rows;         /* rows per GroupNorm-moment run R of pf_conv_desc.gn_partial; 0: no moments (not asked for, or the
                          * kernel serving the problem cannot emit them)                                                           */
    int n_tickets;       /* arrival counters the split launch of this plan needs in pf_conv_desc.tickets (0: nothing is split)     */
    size_t workspace_bytes;  /* split-K scratch of exactly this plan (0: nothing is split)                                         */
} pf_conv_plan;
/* want_moments: the plan of a launch that passes gn_partial (it may take another kernel than the launch without: one that can emit
 * them).  Like the queries it assumes the workspace is available and validates nothing; PF_ERR_ARG for a bad descriptor. */
pf_status pf_conv_gemm_plan(const pf_conv_desc* desc, int want_moments, pf_conv_plan* out);
/* Diagnostics only: while `device_buffer` (capacity_blocks x 32 uint64) is set, every pf_conv_gemm launch
 * with at most capacity_blocks workgroups records 4 shader-clock stamps per workgroup (entry, first
 * operand tile landed, K loop done, exit; the 8-wave kernel adds per-wave K-loop time split into
 * wait+barrier / DMA issue / ds_read+MFMA at [4 + 3*wave + {0,1,2}]).  NULL switches it off (the default). */
pf_status pf_debug_gemm_profile(void* device_buffer, long capacity_blocks);
pf_status pf_conv_gemm(const pf_conv_desc* desc, void* stream);

/* ------------------------------------------------------------------------------------------
 * Weight-stationary linear for the token layers of the two finest levels: the nn.Linear layers of their transformer blocks
 * and EPA blocks (models/modules/transformer.py:57-74 to_q / to_k / to_v / to_out, :8-38 GEGLU FeedForward; diffusers
 * BasicTransformerBlock behind models/pano/MVGenModel.py:104-106).  A workgroup keeps `chb` output channels of the weights in
 * registers and streams tiles of `tile_tokens` rows of `a` through LDS.  The shapes it serves (THE rule: pf_linear_ws_plan below is
 * its one implementation, pf_linear_ws_supported and the launch follow it):
 *     K     modes                                  N a multiple of    chb    tile_tokens    N / chb
 *     320   every mode                             320                320    64             <= 32 (PF_LWS_QKV: 3, PF_LWS_F32_LN: 1)
 *     640   PF_LWS_16, PF_LWS_GEGLU                256                256    32             <= 32
 *     640   PF_LWS_16 (else), PF_LWS_VT            128                128    32             <= 32
 *     1280  PF_LWS_16, PF_LWS_GEGLU, PF_LWS_VT     128                128    16             <= 128
 * and M >= tile_tokens.
 *   PF_LWS_16:    out 16-bit [M][out_ld]      = a w^T + bias
 *   PF_LWS_F32:   out fp32   [M][out_ld]      = a w^T + bias + residual (fp32 [M][res_ld] or NULL)
 *   PF_LWS_GEGLU: out 16-bit [M][out_ld], N/2 columns: w / bias rows interleaved (value_j, gate_j), out = value * gelu(gate)
 *   PF_LWS_QKV:   N == 960 = (q | k | v): out 16-bit [M][out_ld] receives the 640 columns (q | k); V leaves TRANSPOSED as
 *                 out_vt[b][c][key] (b = m / rows_per_batch, key = m % rows_per_batch, row stride vt_ld, batch stride vt_bs):
 *                 the layout pf_attention reads.  rows_per_batch a multiple of tile_tokens that divides M.
 *   PF_LWS_VT:    the whole output TRANSPOSED to out_vt[b][n][key] as in PF_LWS_QKV (the V projection of the 32^2 / 16^2 self-attentions and of
 *                 the EPA blocks: replaces the operand-swapped pf_conv_gemm launch); out unused.  rows_per_batch as for PF_LWS_QKV.
 *   PF_LWS_F32_LN: N == 320: PF_LWS_F32, and the LayerNorm of the result rides along (the norm2 / norm3 that follow the two
 *                 attention output projections of a BasicTransformerBlock): ln_out 16-bit [M][ln_ld] =
 *                 LayerNorm(out; ln_eps) * ln_gamma + ln_beta -- no separate pass over the stream tensor.
 * a 16-bit [M][a_ld]; w 16-bit [N][K]; bias fp32 [N] or NULL. */
typedef struct {
    const void* a; int a_ld;
    const void* w;
    const float* bias;
    const float* residual; int res_ld;
    void* out; int out_ld;
    void* out_vt; int vt_ld; int rows_per_batch; long vt_bs;
    const float* ln_gamma; const float* ln_beta; float ln_eps; void* ln_out; int ln_ld;
    int M, N, K;
    int dtype; int mode;
} pf_linear_ws_desc;
enum { PF_LWS_16 = 0, PF_LWS_F32 = 1, PF_LWS_GEGLU = 2, PF_LWS_QKV = 3, PF_LWS_F32_LN = 4, PF_LWS_VT = 5 };
/* The whole plan of a problem: what pf_linear_ws launches, and whether a linear layer should be sent here at all. */
typedef struct {
    int supported;       /* 1: the kernel can run (M, N, K, mode) -- the table above; 0: it cannot, every other member is 0             */
    int preferred;       /* 1: supported, and the linear front ends send the problem here rather than to pf_conv_gemm: dtype 16-bit,
                          * a_ld >= K and a multiple of 8, rows_per_batch (where stated, PF_LWS_QKV / PF_LWS_VT) a multiple of tile_tokens
                          * that divides M, M >= PF_LINEAR_WS_MIN_ROWS (8192; K = N = 320: 4 x that) and no knob against it:
                          * PF_LINEAR_WS=0 (all), PF_LINEAR_WS_K640=0 / PF_LINEAR_WS_K1280=0 (that K), PF_LINEAR_VT=0 (PF_LWS_VT),
                          * PF_LINEAR_LN=0 (PF_LWS_F32_LN).  The knobs are read once per process.                                        */
    int k;               /* the reduction width: 320, 640 or 1280                                                                      */
    int chb;             /* output channels per workgroup: 320, 256 or 128 -- (k, chb, mode) names the kernel instantiation            */
    int tile_tokens;     /* rows of `a` per LDS ring slot: 64, 32 or 16                                                                */
    int nblocks;         /* channel blocks: N / chb                                                                                    */
    int ntiles;          /* token tiles: ceil(M / tile_tokens), dealt out evenly to the token ranges of the grid                       */
    int splits_per_xcd;  /* > 0: the XCD-grouped grid -- 8 splits_per_xcd token ranges, the nblocks workgroups of a range on one XCD   */
    int flat_splits;     /* > 0: the flat grid -- flat_splits token ranges, workgroup b = (range b / nblocks, channel block b % nblocks);
                          * taken where the grouped grid would fill fewer than 200 of the 256 CUs.  Exactly one of the two is nonzero.   */
    int counted;         /* 1: the kernel waits for a tile's loads by count; 0 (PF_LWS_COUNTED=0): it drains all memory operations     */
} pf_lws_plan;
/* Reads only the scalar members M, N, K, mode, dtype, a_ld, rows_per_batch (0: not stated, not checked) -- never a pointer; PF_ERR_ARG
 * for a NULL argument only: an unsupported problem has a plan with supported = 0. */
pf_status pf_linear_ws_plan(const pf_linear_ws_desc* desc, pf_lws_plan* out);
/* pf_linear_ws_plan's `supported` for (M, N, K, mode). */
int pf_linear_ws_supported(long M, int N, int K, int mode);
/* Launches every supported problem, preferred or not. */
pf_status pf_linear_ws(const pf_linear_ws_desc* desc, void* stream);

/* 3x3 convolutions with 4 input or 4 output channels at the UNet boundary:
 * conv_in  (MVGenModel.py:86,89): x fp32 NCHW [n][cin][h][w] -> y NHWC [n][h][w][cout] (out_dtype 16-bit
 *          or PF_F32), weights fp32 [3][3][cin][cout];
 * conv_out (MVGenModel.py:283,292): x NHWC [n][h][w][cin] (dtype 16-bit or PF_F32) -> y fp32 NCHW
 *          [n][cout][h][w], weights fp32 [cout][3][3][cin], cout <= 8.
 * bias fp32 [cout]; zero padding 1 in y.  wrap = 1: the width axis is circular, which is exactly
 * pad_pano(x,1) -> conv(zero pad) -> unpad_pano(.,1) of the pano branch (MVGenModel.py:87-91,
 * 290-294); wrap = 0: zero padding in x. */
pf_status pf_conv_in(const float* x, int n, int cin, int h, int w, const float* wgt, const float* bias,
                     int cout, int wrap, int out_dtype, void* y, void* stream);
pf_status pf_conv_out(const void* x, int dtype, int n, int cin, int h, int w, const float* wgt,
                      const float* bias, int cout, int wrap, float* y, void* stream);
/* The UNets' head in one launch (MVGenModel.py:279-294: conv_norm_out -> SiLU -> conv_out): x fp32 NHWC
 * [n][h][w][cin] BEFORE the GroupNorm, scale / shift fp32 [n][cin] from pf_groupnorm_* (y = act(x * scale + shift),
 * act 1 = SiLU), wgt_t fp32 [3][3][cin][4] (the conv_out weight transposed, output channels padded to 4 with
 * zeros), cout <= 4, cin % 32 == 0; y fp32 NCHW [n][cout][h][w].  Zero padding / wrap apply to the ACTIVATED
 * tensor, as in pf_conv_out. */
pf_status pf_conv_out_gn(const float* x, int n, int cin, int h, int w, const float* scale, const float* shift, int act,
                         const float* wgt_t, const float* bias, int cout, int wrap, float* y, void* stream);

/* ------------------------------------------------------------------------------------------
 * Flash attention on MFMA (replaces xformers memory_efficient_attention, transformer.py:71,
 * and the diffusers AttnProcessor baddbmm+softmax+bmm inside unet.*.attentions[j]).
 *   out[b][i][h*D + :] = softmax_j(scale * q_i.k_j + bias[i][j]) v_j      D in {32, 64}
 * q [B][nq][q_ld], k [B][nk][k_ld] (head h at column h*D), vt = V transposed:
 * [B][H*D][vt_ld] (keys contiguous), out [B][nq][o_ld].  bias (optional) fp32 [nq][bias_ld]
 * shared by all batches and heads, consulted only for 32x32 tiles whose flag byte is non-zero.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    const void* q; const void* k; const void* vt; void* out;
    int dtype;
    int B, H, D;
    int nq, nk;
    int q_ld, k_ld, vt_ld, o_ld;
    long q_bs, k_bs, vt_bs, o_bs;
    float scale;
    const float* bias; long bias_ld;
    const uint8_t* flags; int flags_ld;
    float* lse;      /* optional fp32 [B][H][nq]: log2 of the softmax denominator in the exp2 domain,
                      * lse = log2(sum_j exp2(log2e * (scale * q.k_j + bias_j))) -- what pf_attention_bwd reads */
    void* workspace; size_t workspace_bytes; /* optional scratch of pf_attention_workspace_size(desc) bytes (round 6): lets a launch with FEW query
                      * blocks and MANY keys (the panorama-query direction of an EPA block: 2048 queries x 20 480 keys, 320-640 workgroups for 1024
                      * slots) split its key range over several workgroups -- normalised 16-bit partial outputs + their log-sum-exps, combined
                      * by a second launch in a fixed order (no atomics).  NULL: never split. */
} pf_attn_desc;

/* Layout rules (pf_attention and pf_attention_wide check them in one place; anything else is PF_ERR_ARG before any launch): q, k, vt, out
 * non-NULL and 16-byte aligned; B, H, nq, nk > 0; q_ld, k_ld multiples of 8, o_ld, vt_ld of 4; q_ld, k_ld and o_ld cover the H * D
 * columns of a row; vt_ld >= nk rounded up to 32; q_bs, k_bs multiples of 8, vt_bs, o_bs of 4; bias and flags come together (with a
 * bias: nk % 4 == 0, bias_ld % 4 == 0, bias_ld >= nk, flags_ld >= ceil(nk / 32)); the planned grid is launchable (each dimension within
 * HIP's limits, workgroups x threads of the 1-D grids under 2^32).  The last two rules refuse only descriptors whose launch would read or
 * write out of bounds or fail at launch. */
pf_status pf_attention(const pf_attn_desc* desc, void* stream);
/* Bytes of pf_attn_desc.workspace that let pf_attention split the key range of this problem (0: it would not split): workspace_bytes
 * of the plan below; 0 for a bad descriptor. */
size_t pf_attention_workspace_size(const pf_attn_desc* desc);
/* The whole plan pf_attention resolves for a problem: everything that selects a kernel instantiation or sizes the grid or the scratch. */
typedef struct {
    int kernel;          /* 0 k_attention (no LDS), 1 k_attention_lds, 2 k_attention_pp, 3 k_attention_pp2 */
    int pipelined;       /* k_attention_lds: its PIPE template argument; 0 for the other kernels */
    int occupancy;       /* k_attention_lds: its OCC template argument; 0 for the other kernels */
    int msum;            /* k_attention_lds: its MSUM template argument; 0 for the other kernels */
    int block_queries;   /* query rows of a workgroup: 128, or 256 for the ping-pong kernels */
    int threads;         /* 256 or 512 */
    int splits;          /* key-range splits S of the launch (1: not split); S > 1 adds the k_attention_merge launch */
    int split_tiles;     /* 64-key tiles per split (even), 0 when splits == 1 */
    unsigned grid_x, grid_y, grid_z;
    size_t workspace_bytes;   /* scratch of exactly this plan, 0 when splits == 1 */
} pf_attn_plan;
/* Looks only at the scalar members of desc and at whether bias and lse are NULL (nothing is dereferenced, no GPU is needed), validates
 * nothing else and reports the plan of a launch that hands over the workspace it asks for (a launch without it runs the same plan
 * unsplit).  PF_ERR_ARG for a NULL pointer, non-positive B, H, nq or nk, or a head dim other than 32 or 64. */
pf_status pf_attention_plan(const pf_attn_desc* desc, pf_attn_plan* out);

/* Flash attention at WIDE heads (replaces the mid-block Attention(heads=1, dim_head=C) of diffusers' AutoencoderKL --
 * baddbmm + softmax + bmm over an N x N score matrix -- reached from models/pano/PanoGenerator.py:213-238):
 *   out[b][i][h*D + :] = softmax_j(scale * q_i.k_j) v_j      D in {128, 256, 512}, H >= 1
 * Operand layout and alignment rules of pf_attention (q, k leading dimensions multiples of 8, out / vt of 4, vt_ld >= nk
 * rounded up to 32, 16-byte aligned pointers, fp16 or bf16).  bias, flags, lse and workspace must be NULL: no bias, no
 * backward and no key-range split at these widths.  Batch strides are 64-bit; INSIDE one (batch, head) slice K and V^T are
 * addressed with 31-bit byte offsets, so the per-batch operand limits are (nk + 64) * k_ld * 2 < 2^31 and
 * D * vt_ld * 2 < 2^31 bytes (16-bit elements); the grid is 1-D: ceil(nq / 64) * H * B < 2^31.  Anything else is
 * PF_ERR_ARG before any launch. */
pf_status pf_attention_wide(const pf_attn_desc* desc, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training: backward of the EPA block (reference models/pano/modules.py:15-59 under autograd;
 * models/modules/transformer.py:77-161 -- the reference recomputes the block in backward,
 * CheckpointFunction, and so does the caller of these entry points).
 * ------------------------------------------------------------------------------------------ */

/* delta[b][h][i] = sum_d dout[b][i][h*D+d] * out[b][i][h*D+d]   (fp32 [B][H][nq]; rows of width ld, batch stride bs). */
pf_status pf_attention_delta(const void* out, const void* dout, int dtype, int B, int H, int D, long nq,
                             int ld, long bs, float* delta, void* stream);

/* Backward of pf_attention given lse (forward) and delta:
 *   P = exp2(log2e * (scale * q.k + bias) - lse),  dV = P^T dO,  dS = P o (dO V^T - delta),
 *   dQ = scale * dS K,  dK = scale * dS^T Q.
 * All of q, k, v, dout are ROW-major ([B][n][ld], head h at column h*D); kt, qt, dot are the transposes of k, q, dout
 * ([B][H*D][*_ld], tokens contiguous) -- the A operands of the products whose reduction runs over tokens.
 * dq [B][nq][dq_ld], dk / dv [B][nk][dk_ld / dv_ld] in `dtype`.  Token counts that are not multiples of 32 take a
 * guarded instantiation (the 4x4 level of a 256^2 view has 16 tokens); with a bias nk % 4 == 0.  Two launches: queries-stationary (dq) and keys-stationary (dk, dv)
 * (+ a reduce launch when the query range was split, see `workspace`); no atomics, results do not depend on scheduling. */
typedef struct {
    const void* q; const void* k; const void* v; const void* dout;
    const void* qt; const void* kt; const void* dot;
    void* dq; void* dk; void* dv;
    int dtype;
    int B, H, D;
    int nq, nk;
    int q_ld, k_ld, v_ld, do_ld;          /* row-major operands */
    int qt_ld, kt_ld, dot_ld;             /* transposed operands */
    int dq_ld, dk_ld, dv_ld;
    long q_bs, k_bs, v_bs, do_bs, qt_bs, kt_bs, dot_bs, dq_bs, dk_bs, dv_bs;
    float scale;
    const float* bias; long bias_ld;      /* as pf_attention: [nq][bias_ld] */
    const uint8_t* flags; int flags_ld;
    const float* lse; const float* delta; /* fp32 [B][H][nq] */
    void* workspace; size_t workspace_bytes; /* optional fp32 scratch of pf_attention_bwd_workspace_size(desc) bytes: lets the
                                              * keys-stationary launch split its query range when it has few blocks (the 128
                                              * text keys of a cross-attention, one panorama sample); partial sums are added in a
                                              * fixed order.  NULL: never split. */
} pf_attn_bwd_desc;

/* Layout rules (anything else is PF_ERR_ARG before any launch): every operand pointer, lse and delta non-NULL and 16-byte aligned; D 32 or
 * 64; B, H, nq, nk > 0; q_ld, k_ld, v_ld, do_ld multiples of 8; qt_ld, kt_ld, dot_ld multiples of 4 that cover the token count; dq_ld,
 * dk_ld, dv_ld multiples of 4; the row-major batch strides multiples of 8, the others of 4; bias and flags come together (with a bias:
 * nk % 4 == 0, bias_ld % 4 == 0, bias_ld >= nk, flags_ld >= ceil(nk / 32)); every row-major leading dimension (q, k, v, do, dq, dk, dv)
 * covers the H * D columns of a row; the planned grids are launchable (H and B at most 65535, grid x within HIP's limit); a non-NULL
 * workspace holds the plan's workspace_bytes, 16-byte aligned.  The cover and the grid rule refuse only descriptors whose launch would
 * read or write out of bounds or fail at launch. */
pf_status pf_attention_bwd(const pf_attn_bwd_desc* desc, void* stream);
/* Bytes of pf_attn_bwd_desc.workspace that let pf_attention_bwd split the query range of this problem (0: it would not split):
 * workspace_bytes of the plan below; 0 for a bad descriptor. */
size_t pf_attention_bwd_workspace_size(const pf_attn_bwd_desc* desc);
/* The whole plan pf_attention_bwd resolves for a problem: the kernel pair, the split of the query range, the grids and the scratch. */
typedef struct {
    int kernel;          /* 0 k_attn_bwd_dq / _dkv<.., false> (whole 32-token tiles, no LDS), 1 the same <.., true> (guarded: ragged
                          * token counts), 2 k_attn_bwd_dq_lds / k_attn_bwd_dkv_lds (LDS-staged) */
    int qsplit;          /* blocks per key block that share the query range of the dkv launch (1: not split); > 1 adds the
                          * k_attn_bwd_reduce launch */
    int threads;         /* 256 */
    unsigned dq_grid_x, dq_grid_y, dq_grid_z;
    unsigned dkv_grid_x, dkv_grid_y, dkv_grid_z;
    unsigned reduce_grid_x, reduce_grid_y, reduce_grid_z;   /* 0 when qsplit == 1 */
    size_t workspace_bytes;   /* scratch of exactly this plan, 0 when qsplit == 1 */
} pf_attn_bwd_plan;
/* Looks only at the scalar members of desc (nothing is dereferenced, no GPU is needed), validates nothing else and reports the plan of a
 * launch that hands over the workspace it asks for (a launch with a NULL workspace runs the same plan unsplit).  PF_ERR_ARG for a NULL
 * pointer, non-positive B, H, nq or nk, or a head dim other than 32 or 64. */
pf_status pf_attention_bwd_plan(const pf_attn_bwd_desc* desc, pf_attn_bwd_plan* out);

/* LayerNorm backward (rows of width C <= 2048, C % 8 == 0).  x (+ pe, as pf_layernorm) is the forward input, dy fp32
 * [rows][C] the gradient of the normalised output, dres (optional fp32 [rows][C]) a gradient that by-passes the norm:
 *   dx = dres + rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dy * gamma.
 * partials: fp32 [2][n_part][C] -- per-block sums of dy * xhat (gamma) and dy (beta) over the block's rows, reduced in
 * a fixed order by pf_colsum afterwards; n_part = pf_layernorm_bwd_parts(rows). */
int pf_layernorm_bwd_parts(long rows);
pf_status pf_layernorm_bwd(const void* x, const float* pe, long pe_rows, int dtype, long rows, int C,
                           const float* gamma, float eps, const float* dy, const float* dres, float* dx,
                           float* partials, void* stream);

/* GroupNorm (+ SiLU) backward for the forward y = act(x * scale + shift) of pf_groupnorm_stats + pf_scale_shift_act:
 * x = channel concat of x0 [n][hw][c0] and x1 [n][hw][c1] (16-bit or PF_F32), scale / shift fp32 [n][c0+c1] as the forward
 * produced them, dy fp32 [n][hw][c0+c1], dres optional fp32 gradient of the same shape added to the result;
 * dx0 [n][hw][c0], dx1 [n][hw][c1] fp32.  gamma / beta take no gradient here (frozen UNet).  act: 0 none, 1 SiLU. */
size_t pf_groupnorm_bwd_workspace_size(int n_img, int hw, int groups);
pf_status pf_groupnorm_bwd(const void* x0, int c0, const void* x1, int c1, int dtype, int n_img, int hw, int groups,
                           float eps, const float* gamma, const float* scale, const float* shift, int act,
                           const float* dy, const float* dres, float* dx0, float* dx1, void* workspace,
                           size_t workspace_bytes, void* stream);

/* Parameter gradients of a TRAINABLE GroupNorm (+ SiLU): the ControlNet's own parameters train when layout conditions
 * are on (reference models/pano/PanoGenerator.py:153-157 `get_cn`: list(cn.parameters()) at lr x 0.1; autograd through
 * diffusers' GroupNorm at MVGenModel.py:68-83).  Forward y = act(x * scale + shift) as for pf_groupnorm_bwd;
 * unit_scale / unit_shift fp32 [n][c0+c1]: the same statistics with gamma = 1, beta = 0 (xhat = x * unit_scale +
 * unit_shift).  dgamma_dbeta fp32 [2 * (c0+c1)] = (sum dz * xhat | sum dz), dz = dy * act'(x * scale + shift), summed
 * over images and pixels in a fixed order. */
size_t pf_groupnorm_param_grads_workspace_size(int n_img, int hw, int C);
pf_status pf_groupnorm_param_grads(const void* x0, int c0, const void* x1, int c1, int dtype, int n_img, int hw,
                                   const float* scale, const float* shift, const float* unit_scale, const float* unit_shift,
                                   int act, const float* dy, float* dgamma_dbeta, void* workspace, size_t workspace_bytes,
                                   void* stream);
/* The plan of pf_groupnorm_bwd and of the pf_groupnorm_param_grads of the same tensor: both walk an image in the same chunks. */
typedef struct {
    int ppc;                      /* pixels per chunk: 64, halved down to 8 while an image has fewer than 16 chunks                        */
    int chunks;                   /* chunks per image, ceil(hw / ppc)                                                                     */
    int pix_par;                  /* pixels a block reads in parallel, 256 / min(C / 8, 256)                                              */
    unsigned bwd_lds_bytes;       /* dynamic LDS of k_gn_bwd_partial, 4 fp32 arrays [pix_par][C]; refused above 64 KiB                     */
    unsigned param_lds_bytes;     /* dynamic LDS of k_gn_param_partial, 2 such arrays; refused above 64 KiB                                */
    unsigned partial_grid_x, partial_grid_y;   /* both partial kernels: (chunks, n_img)                                                  */
    unsigned finalize_grid_x;     /* k_gn_bwd_finalize: n_img                                                                            */
    unsigned apply_grid_x, apply_grid_y;       /* k_gn_bwd_apply: (ceil(hw * C / 8 / 256), n_img)                                         */
    size_t bwd_workspace_bytes;   /* pf_groupnorm_bwd: n_img * (chunks + 1) * groups * 4 floats                                           */
    size_t param_partial_bytes;   /* pf_groupnorm_param_grads: the [n_img * chunks][2 C] fp32 partials at the head of its workspace ...    */
    size_t param_workspace_bytes; /* ... and with the pf_colsum workspace that reduces them behind                                       */
} pf_gn_bwd_plan;
/* Reads no pointer.  groups > 0: both launches; groups = 0: pf_groupnorm_param_grads alone, which knows no groups and has half the LDS
 * to fit (the members of pf_groupnorm_bwd are 0 then).  PF_ERR_ARG, the launch's message and an all-zero plan for a refused problem. */
pf_status pf_groupnorm_bwd_plan(int n_img, int hw, int c0, int c1, int groups, pf_gn_bwd_plan* out);

/* dz = dy * silu'(z), z 16-bit or PF_F32 [n] (a pre-activation the forward kept), dy / dz fp32: the SiLUs of the ControlNet's
 * conditioning embedding and of the timestep embedding under autograd (diffusers ControlNetConditioningEmbedding /
 * TimestepEmbedding, reached from MVGenModel.py:68-83). */
pf_status pf_silu_bwd(const void* z, int dtype, const float* dy, long n, float* dz, void* stream);

/* im2col of a 3x3 / pad 1 convolution, stride 1 or 2: x [n][h][w][C] 16-bit -> y [n*ho*wo][9][C] (tap = 3 ky + kx, zero
 * outside the image; ho = (h-1)/stride+1).  The weight gradient of a trainable convolution (torch autograd through
 * nn.Conv2d in the ControlNet) is then one token-reducing pf_conv_gemm: dW [cout][9 C] = dY^T y. */
pf_status pf_im2col3(const void* x, int dtype, int n, int h, int w, int C, int stride, void* y, void* stream);

/* LoRA fold, once per projection and optimizer step of a training run (the rank-4 LoRA of models/pano/PanoGenerator.py:129-151
 * on q / k / v / out of every attention; diffusers LoRALinearLayer: y = W x + scale * up(down(x))):
 *   out [N][out_ld] (16-bit `dtype`) = W + scale * up @ down,   W fp32 [N][K], up fp32 [N][r], down fp32 [r][K], r <= 64
 * (r = 0: a plain fp32 -> 16-bit conversion).  Optional by-products for the backward, NULL to skip: out_t [K][out_t_ld] the
 * transpose of the folded weight; d_out [r][d_ld] = down and u_out [r][u_ld] = up^T in 16 bit (rows / a block of the
 * stacked matrices the LoRA gradient GEMMs read).  `out` may be a row slice of a larger packed weight. */
pf_status pf_lora_fold(const float* w, const float* up, const float* down, int N, int K, int r, float scale, int dtype,
                       void* out, long out_ld, void* out_t, long out_t_ld, void* d_out, long d_ld, void* u_out, long u_ld,
                       void* stream);

/* Data movement of the backward pass (NHWC):
 *   pf_zero_insert2   y [n][2h][2w][C] = x at the even positions, zero elsewhere (16-bit): the data gradient of a
 *                     stride-2 convolution is the stride-1 convolution of this with the flipped kernel;
 *   pf_sum2x2         y [n][h][w][C] = sums of the 2x2 blocks of x [n][2h][2w][C] (fp32): nearest x2 up-sampling backward;
 *   pf_pad_width_bwd  dy [n][h][w+2pad][C] -> dx [n][h][w][C]: the margins fold back onto the columns they copy (fp32);
 *   pf_crop_width_bwd dy [n][h][w-2crop][C] -> dx [n][h][w][C] with zero margins (fp32). */
pf_status pf_zero_insert2(const void* x, int dtype, int n, int h, int w, int C, void* y, void* stream);
pf_status pf_sum2x2(const float* x, int n, int h, int w, int C, float* y, void* stream);
pf_status pf_pad_width_bwd(const float* dy, int n, int h, int w, int C, int pad, float* dx, void* stream);
pf_status pf_crop_width_bwd(const float* dy, int n, int h, int w, int C, int crop, float* dx, void* stream);

/* x [B][T][C] -> y [B][C][T] (16-bit): the token-contiguous operand layout of the products that reduce over tokens
 * (attention backward, weight gradients).  C % 4 == 0. */
pf_status pf_transpose_tokens(const void* x, int dtype, int B, long T, int C, void* y, void* stream);

/* GEGLU backward: u [rows][2*inner] = [a | gate] (forward input of pf_geglu), dg [rows][inner] ->
 * du [rows][2*inner] = [dg * gelu(gate) | dg * a * gelu'(gate)]. */
pf_status pf_geglu_bwd(const void* u, const void* dg, int dtype, long rows, int inner, void* du, void* stream);

/* Column sums: x [rows][N] (16-bit or PF_F32, row stride ld) -> out fp32 [N], fixed summation order.
 * workspace: fp32 scratch of pf_colsum_workspace_size(rows, N) bytes. */
size_t pf_colsum_workspace_size(long rows, int N);
pf_status pf_colsum(const void* x, int dtype, long rows, int N, long ld, float* out, void* workspace,
                    size_t workspace_bytes, void* stream);

/* Weighted column sums, the token-reducing half of the LoRA gradients (rank-4 LoRA of PanoGenerator.py:129-151 under autograd:
 * d_up = dY^T (X down^T), d_down = (dY up)^T X):  out[r][c] = scale * sum_t w[r][t] * x[t][c]  for x [T][C] 16-bit row-major
 * (row stride ld) and w fp32 [R][w_ld >= T], R a multiple of 4 (the stacked ranks of a
 * projection group: 12 for q / k / v at rank 4, 24 at rank 8).  x is read once per 16 rows of w, as the backward holds it (no transposed copy); partial
 * sums per row slab are added in a fixed order.  scale = host_scale * (*dev_scale if given: the gradient-normalisation factor
 * on the device).  blocks (host, n_blocks x 4 ints (row0, rows, col0, cols), n_blocks <= 4): when given, only these blocks of
 * [R][C] are written, one after the other, block b TRANSPOSED as [cols_b][rows_b] (the [N_i][rank] layout of a LoRA up
 * matrix); else out is [R][C].  workspace: pf_weighted_colsum_workspace_size(T, C, R) bytes. */
size_t pf_weighted_colsum_workspace_size(long T, int C, int R);
pf_status pf_weighted_colsum(const void* x, int dtype, long T, int C, long ld, const float* w, int R, long w_ld,
                             const float* dev_scale, float host_scale, const int* blocks, int n_blocks, float* out,
                             void* workspace, size_t workspace_bytes, void* stream);

/* Gradient normalisation for 16-bit backward operands.  state: 4 floats on the device.
 *   pf_amax_f32: state[0] = max(state[0], max |x|) (reset = 1 clears it first);
 *   pf_pow2_scale: state[1] = 2^-e with amax * 2^-e in [1, 2) (1 when amax is 0 or not finite), state[2] = 2^e;
 *   pf_scale_f32: y = x * state[index]; y fp32 (may alias x) or 16-bit. */
pf_status pf_amax_f32(const float* x, long n, float* state, int reset, void* stream);
pf_status pf_pow2_scale(float* state, void* stream);
pf_status pf_scale_f32(const float* x, long n, const float* state, int index, int out_dtype, void* y, void* stream);

/* ------------------------------------------------------------------------------------------
 * The FAED metric's encoder (models/faed/modules.py Encoder, models/faed/FAED.py get_activation): wide-kernel,
 * narrow-channel convolutions that are periodic in longitude.
 * ------------------------------------------------------------------------------------------ */

/* One convolution of the FAED encoder, CircularPadding + nn.Conv2d(padding = 0) of models/faed/modules.py:5-36 with the bias and the
 * evaluation-mode BatchNorm folded into a per-channel affine map, as an implicit GEMM on MFMA (fp16 operands, fp32 sums):
 *
 *   out[img][y][x][n] = act(fma(sum_{ky,kx,c} x[img][y*stride - pad + ky][(x*stride - pad + kx) mod w][c] * weight[n][ky][kx][c],
 *                               scale[n], shift[n])) (+ residual[img][y][x][n])
 *
 * Geometry: (ksize, stride) is (3 | 5 | 7 | 9, 1) with pad = (ksize - 1) / 2, or (4, 2) with pad = 1 and even h and w.  Columns are
 * periodic (w >= pad), rows outside [0, h) read zero.  h_out = (h + 2 pad - ksize) / stride + 1, w_out likewise.
 * x: PF_F16 NHWC [n_img][h][w][c_in], c_in in {32, 64, 128}.  The image layer (downconv1_rgb) instead takes the evaluation loop's tensor
 *    as delivered: x_dtype PF_U8 or PF_F32, planar [n_img][3][h][w] on the 0..255 scale, c_in = 3, ksize = 9, n_out = 32; v / 127.5 - 1
 *    (FAED.py:70) is applied in fp32 and rounded to fp16 while the tile is staged.
 * weight: fp16 [n_out][ksize][ksize][c_in], n_out in {32, 64, 128}.  scale, shift: fp32 [n_out].  relu: 0 / 1, applied before the
 * residual (fp16 [M][n_out], may be NULL; ResBlock has no activation after its sum).  out: PF_F16 or PF_F32 [M][n_out],
 * M = n_img * h_out * w_out.  No tensor may hold 2^31 elements or more.  A sum's order is the same at every position. */
typedef struct {
    const void* x;
    int x_dtype;
    int n_img, h, w, c_in;
    const void* weight;
    int n_out, ksize, stride;
    const float* scale;
    const float* shift;
    int relu;
    const void* residual;
    void* out;
    int out_dtype;
} pf_pano_conv_desc;
pf_status pf_pano_conv(const pf_pano_conv_desc* desc, void* stream);
/* The output rows of the tile one workgroup of pf_pano_conv owns for this geometry (no launch): 16 at stride 1 with ksize 5, 7 or 9
 * from 512 tiles of 16 x 16 on (two workgroups for each of the chip's 256 CUs), else 8; the environment's PF_PANO_CONV_ROWS = 2 | 4
 * forces 8 | 16 where both forms exist.  The two forms give identical bits.  0: a geometry pf_pano_conv rejects. */
int pf_pano_conv_tile_rows(int ksize, int stride, int n_img, int h, int w);

/* FAED.py:72-77: x fp32 [n][h][w][C] (the encoder's output) -> out fp32 [n][C * h], out[i][c * h + y] = weight[y] * mean_x x[i][y][x][c];
 * the mean is a sum in column order divided by w.  weight: fp32 [h] on the device (the caller's cos(linspace(pi/2, -pi/2, h))). */
pf_status pf_faed_features(const float* x, int n, int h, int w, int C, const float* weight, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PANFUSION_HIP_H */
