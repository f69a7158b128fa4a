/* deflow_amd.h -- C ABI of the MI355X-native DeFlow hot path (libdeflow_amd.so).
 *
 * The reference has no C/FFI plugin interface: its boundary is the Python class contract of
 * `model=deflow` ([REF deflow.py:20-113]) plus two native CUDA ops it builds from
 * `assets/cuda/mmcv` ([REF README.md:38]: dynamic voxelize + dynamic scatter).  This header is
 * what a maintainer binds instead of those ops and instead of the torch/cuDNN calls made by
 * the model blocks; INTEGRATION.md shows the ctypes stub.  Every entry point
 *   - takes raw DEVICE pointers, explicit sizes and a hipStream_t (as void*),
 *   - never allocates, never synchronises, is safe to call from any host thread per stream,
 *   - returns 0 on success, a negative DF_E_* code for a rejected argument, or a positive
 *     hipError_t from the launch.
 * All activations are NHWC ("pixel-major"): element (n,y,x,c) of an image set lives at
 *   ptr + (n % grp_size) * img_stride + (n / grp_size) * grp_off + (y * w + x) * ld + c.
 * A plain [N,H,W,C] tensor has grp_size = N, grp_off = 0, ld = C, img_stride = H*W*C.
 * The (grp_size, grp_off) pair lets the two point clouds' feature maps share one channel-
 * concatenated buffer ([REF deflow.py:93] torch.cat((pc0_img, pc1_img), dim=1)) with no copy.
 */
#ifndef DEFLOW_AMD_H
#define DEFLOW_AMD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DF_OK 0
#define DF_E_SHAPE -1    /* unsupported / inconsistent shape */
#define DF_E_ALIGN -2    /* pointer or stride not 16-byte aligned where required */
#define DF_E_ARG -3      /* bad enum / null pointer */
#define DF_E_WORKSPACE -4

typedef struct df_img {
  void* ptr;
  int32_t n, h, w, c; /* images, rows, cols, channels addressed */
  int32_t ld;         /* elements between consecutive pixels */
  int32_t grp_size;   /* images per group */
  int64_t img_stride; /* elements between images inside a group */
  int64_t grp_off;    /* element offset of group g */
  int32_t elt;        /* element type: 0 = float32 (every entry point), 1 = bfloat16 (bf16-STORAGE training, round 3: only the
                         entry points that say so accept it -- df_conv2d_w16 x / y, df_conv2d_mp y, df_bn_gelu_*_t,
                         df_conv2d_wgrad_bf16; all others return DF_E_ARG), 2 = pre-split fp16x2 "h2" image (round 4: see "PRE-SPLIT
                         tensors" below; only the *_h2p / *_yh2 / *_h2 entry points).  ld / img_stride / grp_off stay in ELEMENTS */
  int32_t reserved;   /* 0 */
} df_img;

int df_version(void);

/* ---------------------------------------------------------------- pillarise (A2-A4) ----
 * Replaces mmcv Voxelization(max_num_points=-1) + DynamicScatter + DynamicPillarFeatureNet +
 * PointPillarsScatter as used by DynamicEmbedder ([REF deflow.py:27-30,82-83]).           */
typedef struct df_pillar_geom {
  float vx, vy, vz;          /* voxel size (fp32, as mmcv's tensors hold it)              */
  float minx, miny, minz;    /* point_cloud_range[:3]                                      */
  float offx, offy, offz;    /* v/2 + min computed in double then rounded (feature net)    */
  int32_t gx, gy, gz;        /* grid = round((max-min)/v); gz must be 1 (pillars)          */
} df_pillar_geom;

/* ---- second generation (csrc/pillar_bands.hip): the path DynamicEmbedder takes.  The grid is cut into bands of R rows
 * (R * gx <= 2048 cells, df_pillar2_rows_per_band); points are bucketed by (sample, band) with a stable counting sort over
 * 1024-point tiles (hist -> scan -> scatter) and each band's workgroup finishes the sort by cell in LDS, runs the feature
 * net and writes its slice of the canvas -- zeros included, every byte once; no separate zero-fill, no library sort.
 * S = number of cloud samples in this call (B, or 2B when both clouds are pillarised together), NB = ceil(gy / R),
 * nblk = ceil(N / df_pillar2_tile()).  Sorted layout: sample s owns sorted positions
 * [sum counts[0..s), + counts[s]), ascending cell key, input order inside a cell; positions past the last valid point are
 * not written. */
int df_pillar2_rows_per_band(int H, int W);   /* 0 if the grid is not supported (W > 2048) */
int df_pillar2_tile(void);
/* hist [S, NB+1, nblk] i32: points of each tile per band; column NB = valid points of the tile */
int df_pillar2_hist(const float* pts, int S, int N, df_pillar_geom g, int rows_per_band, int32_t* hist, void* stream);
/* off (shape of hist): exclusive scan over the tiles of every (sample, column); tot [S, NB+1]; counts [S] = valid points */
int df_pillar2_scan(const int32_t* hist, int S, int ncol, int nblk, int32_t* off, int32_t* tot, int32_t* counts,
                    void* stream);
/* order-preserving compaction (points_c [S,N,3] f32, coords_c [S,N,3] i32 (z,y,x), idx_c [S,N] i64, offs_c [S,N,3] f32, cpos [S*N] i32 = compact position of each original point or -1; rows >= counts[s] untouched) + bucketed key [S*N] u32 / flat index [S*N] u32 / xyz [S*N,3] */
int df_pillar2_scatter(const float* pts, int S, int N, df_pillar_geom g, int rows_per_band, const int32_t* off,
                       const int32_t* tot, float* points_c, int32_t* coords_c, int64_t* idx_c, float* offs_c,
                       int32_t* cpos, uint32_t* bkey, uint32_t* bidx, float* bpts, int32_t* bucket0 /* [S, NB] out */,
                       void* stream);
/* flags: 1 = sort (inputs are the bucketed arrays; writes key_sorted / idx_sorted / pts_sorted), 2 = BatchNorm1d batch
 * statistics partials [S, NB, 32, 2] (finalise with df_pfn_bn_finalize, nblk_stat = NB), 4 = canvas (writes ALL of
 * out [S, gy, gx, 32]).  Valid: 1|4 (inference), 1|2 then 4 (training; the second call takes the SORTED arrays as inputs).
 * cell_rng: optional dense [S*gy*gx, 2] table of sorted [start, end) per cell (written completely). */
int df_pillar2_band(const uint32_t* in_key, const uint32_t* in_idx, const float* in_pts, const int32_t* tot,
                    const int32_t* bucket0 /* from df_pillar2_scatter */, int S,
                    df_pillar_geom g, int rows_per_band, int flags, const float* w_pfn, const float* bn_ss,
                    int bn_sample_stride, int mode, df_img out, uint32_t* key_sorted, uint32_t* idx_sorted,
                    float* pts_sorted, int32_t* cell_rng, float* stats_partial, void* stream);
/* round 5, PERSISTENT canvas: the same canvas-writing call (flags & 4) on a buffer that is zero wherever the previous call with the
 * same (S, grid, rows_per_band, occ) left no pillar -- initially all zero, occ all zero.  Only the occupied cells and the cells that
 * were occupied last time and are empty now are written (the dense form streams 128 B of zeros into every empty cell: 87 % of the
 * stage's bytes); occ [S][bands][64] u32 (one bit per cell of a band) is read and rewritten in place by the band's workgroup.
 * amax_out (optional device scalar, ZERO before the call; several calls into one canvas may share it): receives the maximum of the
 * canvas values written (they are >= 0: the feature net ends in a ReLU) -- the bound an fp16x2 consumer of the canvas scales by.
 * Replaces the zero-initialised canvas of PointPillarsScatter [REF deflow.py:82-83 -> embedder] kept across calls. */
int df_pillar2_band_sp(const uint32_t* in_key, const uint32_t* in_idx, const float* in_pts, const int32_t* tot,
                       const int32_t* bucket0, int S, df_pillar_geom g, int rows_per_band, int flags, const float* w_pfn,
                       const float* bn_ss, int bn_sample_stride, int mode, df_img out, uint32_t* key_sorted,
                       uint32_t* idx_sorted, float* pts_sorted, int32_t* cell_rng, float* stats_partial, uint32_t* occ,
                       float* amax_out, void* stream);

/* (the first-generation forward entry points df_pillar_keys / _scan / _compact / _sort / _gather_sorted / _cells, df_pfn_stats
 * and df_pfn_canvas -- a library radix sort and separate kernels over a zero-filled canvas -- were retired in round 3: the band
 * pipeline above is the only pillariser; its tests compare it with the oracle directly.)
 * finalize (training): per-sample scale/shift/mean/invstd of the feature net's BatchNorm1d from the band kernel's statistics
 * partials (flag 2), sequential running-stat update (one update per sample, as the reference calls feature_net once per sample).
 * counts [B] i32 valid points; bn_ss [B,4,32] f32 = scale, shift, mean, invstd. */
int df_pfn_bn_finalize(float* partial /* clobbered: slot 0 of every sample is reused as scratch */, int B, int nblk_stat, const int32_t* counts, const float* gamma,
                       const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                       float* bn_ss, void* stream);
/* round 4: the same, also leaving an a-priori bound of max |canvas| (from the statistics, the feature net's weights w_pfn [32][9]
 * and the geometry) in *canvas_bound (integer atomic max: zero-initialise it, or pass one slot for both clouds) */
int df_pfn_bn_finalize2(float* partial, int B, int nblk_stat, const int32_t* counts, const float* gamma, const float* beta, float eps,
                        float momentum, float* running_mean, float* running_var, float* bn_ss, const float* w_pfn, df_pillar_geom g,
                        float* canvas_bound, void* stream);
/* Stable counting sort of caller-supplied cell keys (the stand-alone decoder-head call takes arbitrary voxel_coords
 * [REF decoder.py:185-199], not the pillariser's): idx_sorted [n] u32 = indices of the keys < ncells grouped by key, ascending
 * index inside a group (entries past the number of such keys are not written); cell_rng [ncells, 2] i32 = [start, end) per key,
 * written completely.  Keys >= ncells are dropped.  ws: df_cell_sort_ws_bytes(ncells).  In-tree replacement of the rocPRIM radix
 * sort of rounds 1-2 (hist / offsets / scatter with integer atomics, then each group put in ascending order: deterministic). */
int64_t df_cell_sort_ws_bytes(int64_t ncells);
int df_cell_sort(const uint32_t* key, int64_t n, int64_t ncells, uint32_t* idx_sorted, int32_t* cell_rng, void* ws, void* stream);
/* backward of the feature net over the sorted runs (all pfn kernels iterate over occupied pillars = heads of the sorted key
 * runs of sample b = sorted positions [sum counts[0..b), +counts[b])); bn_sample_stride = 128 (per-sample stats) or 0 (shared:
 * eval); mode (0 'avg': every point of a pillar gets g / count; 1 'max': per channel the pillar's
 * first maximal point gets g, mmcv's traceback rule): pass A partial sums [B,nblk_stat,32,2] of (g_hat, g_hat*xhat); finalize -> dgamma, dbeta,
 * coef [B,2,32] = (S1/M_b, S2/M_b); pass B dW partials [B*nblk_stat,32,9] (sum with df_colsum_finalize). */
int df_pfn_bwd_stats(const float* pts_sorted, const int32_t* cell_rng, const uint32_t* key_sorted,
    const int32_t* counts, int B, df_pillar_geom g,
                     const float* w_pfn, const float* bn_ss, int bn_sample_stride, int mode, df_img gout,
                     float* partial, int nblk_stat, void* stream);
int df_pfn_bwd_finalize(const float* partial, int B, int nblk_stat, const int32_t* counts, float* dgamma,
                        float* dbeta, int accumulate, float* coef, void* stream);
int df_pfn_bwd_weights(const float* pts_sorted, const int32_t* cell_rng, const uint32_t* key_sorted,
    const int32_t* counts, int B, df_pillar_geom g,
                       const float* w_pfn, const float* bn_ss, int bn_sample_stride, int mode, const float* coef,
                       df_img gout, float* dw_partial, int nblk_stat, void* stream);

/* (autograd of backbone(pc0_img, pc1_img) [REF deflow.py:87-88] w.r.t. its inputs, which only DynamicEmbedder's pillar
 * features [REF deflow.py:82-83] consume)
 * Gradient of the pillar canvas [B,H,W,32] of one cloud (cloud 0 = pc0 = channels 0..31 of the network input, cloud 1 =
 * pc1) evaluated ONLY at that cloud's occupied cells -- the only cells df_pfn_bwd_* read.  Adds (accumulate != 0) or
 * writes the two conv consumers of the canvas in FastFlow3DUNet: the first encoder conv (3x3, stride 2, 32 -> 64:
 * dy1 [2B,H/2,W/2,64] with image = cloud * B + b, w1 [64,3,3,32]) and the decoder's 1x1 skip conv on the 64-channel
 * input (dskip [B,H,W,64], w3 [64,64]).  Replaces two dense data-gradient convolutions.  Unoccupied cells are untouched. */
int df_pillar_input_grad(const uint32_t* key_sorted, const int32_t* counts, int B, int H, int W, int cloud,
                         const float* dy1, const float* w1, df_img dskip, const float* w3, df_img dcanvas,
                         int accumulate, int nblk, void* stream);

/* (autograd of the integer gather after_pseudoimage[:, y, x] [REF decoder.py:165-168]: the backbone output is read, and
 * its gradient is non-zero, only at the voxel coordinates of pc0's points)
 * Weight (and bias) gradient of a 3x3 stride-1 64 -> 64 conv whose OUTPUT gradient dy [B,H,W,64] is exactly zero outside
 * the occupied cells of a pillarised cloud (the UNet's last conv: dy comes from the decoder's gather backward): sums only
 * over those cells.  ws [nblk*B][64][9][64] / bias_ws [nblk*B][64] partials; finish with
 * df_conv2d_wgrad_reduce(ws, nblk*B, 64, 9, 64, ...) and df_colsum_finalize(bias_ws, nblk*B, 64, 1, ...). */
int df_sparse_wgrad3x3(const uint32_t* key_sorted, const int32_t* counts, int B, df_img x, df_img dy, float* ws,
                       float* bias_ws, int nblk, void* stream);
/* ... with both operands as two bf16 planes (16 significant bits; three v_mfma_f32_16x16x32_bf16 per tile and 32 pixels -- the product of
 * the GRU kernels) instead of the fp32 matrix pipe; x / dy rows 16-byte aligned.  Same arguments and partial layout.  Its pixel lists
 * hold y << 16 | x: H < 32768 and W < 65536, else DF_E_SHAPE and nothing is written (df_sparse_wgrad3x3 has no such bound). */
int df_sparse_wgrad3x3_x2(const uint32_t* key_sorted, const int32_t* counts, int B, df_img x, df_img dy, float* ws,
                          float* bias_ws, int nblk, void* stream);

/* The same conv's forward where only those cells of the OUTPUT are consumed (the `after` image is read by the decoder's
 * gather alone): y[p] = bias + conv3x3(x)[p] for the occupied cells p of the pillarised cloud; other cells of y are not
 * written.  x, y [B,H,W,64]; w [64,3,3,64]. */
int df_sparse_conv3x3(const uint32_t* key_sorted, const int32_t* counts, int B, df_img x, const float* w,
                      const float* bias, df_img y, int nblk, void* stream);
/* ... on the 16-bit matrix pipe as an fp32-accurate fp16x2 product (three v_mfma_f32_16x16x32_f16 per 32-deep k step, as the dense
 * 3x3 layers: df_conv2d_h2): w2 = the [hi | lo] fp16 planes of w scaled by df_h2_scale(*w_amax) (df_split_h2 / df_weight_prep),
 * x_amax = a bound of max |x| (device scalars).  Same cells, same result class as df_sparse_conv3x3. */
int df_sparse_conv3x3_h2(const uint32_t* key_sorted, const int32_t* counts, int B, df_img x, const void* w2,
                         const float* x_amax, const float* w_amax, const float* bias, df_img y, int nblk, void* stream);
/* ... with bf16 operands (the bf16-operand training mode: x and w rounded to bf16 on the way to the matrix pipe, fp32 accumulation). */
int df_sparse_conv3x3_bf16(const uint32_t* key_sorted, const int32_t* counts, int B, df_img x, const float* w,
                           const float* bias, df_img y, int nblk, void* stream);

/* Weight gradient of the first encoder conv (3x3, stride 2, pad 1, 32 -> 64; dy1 [2B,H/2,W/2,64], image = cloud*B + b)
 * summed over the occupied cells of one cloud's canvas [B,H,W,32] only.  ws [nblk*B][64][9][32] partials; finish with
 * df_conv2d_wgrad_reduce(ws, nblk*B, 64, 9, 32, ..., accumulate = cloud).  The cell lists hold y << 16 | x: H < 32768 and W < 65536, else
 * DF_E_SHAPE and nothing is written (the caller then takes the dense weight gradient: deflow_amd/autograd.py). */
int df_sparse_in_wgrad(const uint32_t* key_sorted, const int32_t* counts, int B, int H, int W, int cloud,
                       const float* dy1, df_img canvas, float* ws, int nblk, void* stream);

/* ------------------------------------------------------------- BEV convolutions (A5) ---
 * Replaces torch.nn.Conv2d / BatchNorm2d / GELU / interpolate inside FastFlow3DUNet and
 * ConvWithNorms ([REF decoder.py:202-220]).  fp32 MFMA (v_mfma_f32_32x32x2_f32) implicit GEMM. */

#define DF_CONV_FWD 0   /* y[p] = sum_k x[p*stride + k - pad] w[.,k,.]                 */
#define DF_CONV_DGRAD 1 /* y[p] = sum_k x[(p + pad - k)/stride] w[.,k,.] if divisible  */
#define DF_EPI_BIAS 0   /* y = acc (+ bias)                                            */
#define DF_EPI_STATS 1  /* + per-tile per-channel (sum, sumsq) partials for BatchNorm  */
#define DF_EPI_BN_GELU 2 /* y = gelu((acc + bias) * scale[c] + shift[c]) (eval mode)   */

/* w [Cout, k*k, Cin] f32 (OHWI).  bias/scale/shift may be NULL when unused.
 * stats_partial [tiles_m, Cout, 2] with tile_m = df_conv2d_tile_m(rows per stat group, Cout) rows per tile.
 * accumulate != 0: y += result (used to sum gradients arriving from two consumers). */
int df_conv2d(df_img x, const float* w, const float* bias, df_img y, int ksize, int stride, int pad,
              int mode, int epi, const float* scale, const float* shift, float* stats_partial,
              int accumulate, void* stream);
/* Mixed-precision form (training with BASELINE configs[4]'s "bf16 MFMA"): mfma_bf16 != 0 rounds both MFMA operands to bf16
 * as they leave LDS (v_cvt_pk_bf16_f32, round to nearest even) and multiplies on v_mfma_f32_32x32x16_bf16 with fp32
 * accumulation; every tensor stays fp32 in memory, epilogues unchanged.  mfma_bf16 == 0 is df_conv2d.  (The register-staged kernel --
 * the generic stride-2 data gradient, tensors beyond 32-bit offsets -- rounds the operands on their way INTO LDS and multiplies them
 * on the fp32 MFMA: the same exact products, fp32 accumulation.) */
int df_conv2d_mp(df_img x, const float* w, const float* bias, df_img y, int ksize, int stride, int pad,
                 int mode, int epi, const float* scale, const float* shift, float* stats_partial,
                 int accumulate, int mfma_bf16, void* stream);
int df_conv2d_tile_m(int64_t rows_per_stat_group, int cout); /* row-tile the launcher will pick for DF_EPI_STATS */
/* The bf16-operand conv with PRE-CAST weights: w16 = df_cast_bf16 of the [Cout,kh,kw,Cin] weights (one cast per optimizer
 * step).  Activations in and out stay fp32; the workgroup converts its input halo once on the way into LDS, tiles are bf16 in
 * LDS, every MFMA operand is one 16-byte LDS read.  Exists for the haloed 3x3 stride-1 form only (forward and data gradient,
 * W % 128 == 0, Cin % 32 == 0, Cout % 64 == 0): df_conv2d_w16_ok() == 1 says so for a call, other shapes get DF_E_SHAPE and use
 * df_conv2d_mp.  Results are those of df_conv2d_mp(mfma_bf16 = 1) up to fp32 summation order.
 * [REF decoder.py:202-220 under torch.autocast(bfloat16)] */
int df_conv2d_w16(df_img x, const void* w16, const float* bias, df_img y, int ksize, int stride, int pad, int mode, int epi,
                  const float* scale, const float* shift, float* stats_partial, int accumulate, void* stream);
/* fp32-ACCURATE 3x3 stride-1 convolution on the bf16 matrix pipe (round 3, "bf16x3"): every fp32 operand is the exact sum of
 * three bf16 values, six of the nine bf16 x bf16 products (exact in the fp32 accumulator) reproduce the fp32 product to
 * <= 2^-23 relative -- the same accuracy class as v_mfma_f32_32x32x2_f32 at 16 / 6 of its rate.  w3 = df_split_bf16x3 of
 * the [Cout,3,3,Cin] weights (3 * Cout * 9 * Cin bf16); x, y fp32; arguments / epilogues as df_conv2d.  Replaces the fp32
 * Conv2d of ConvWithNorms / UpsampleSkip [REF decoder.py:205,213] forward and data gradient.  df_conv2d_x3_ok: 1 if the form
 * exists for the call (3x3, stride 1, W % 128 == 0, full 128-row tiles, DMA-addressable tensors; DF_CONV_X3=0 disables). */
int df_conv2d_x3(df_img x, const void* w3, const float* bias, df_img y, int ksize, int stride, int pad, int mode, int epi,
                 const float* scale, const float* shift, float* stats_partial, int accumulate, void* stream);
int df_conv2d_x3_ok(df_img x, df_img y, int ksize, int stride, int mode, int epi);
int df_split_bf16x3(const float* w, void* out3, int64_t n, void* stream);
/* The same convolution through TWO fp16 planes per operand ("fp16x2", round 3; conv_halo_x3_kernel<.., NP = 2>): with power-of-
 * two scales s taken from upper bounds of max|x| and max|w| (device scalars, df_absmax) an fp32 value is x s = hi + lo / 2048 with
 * hi = fp16(x s), lo = fp16((x s - hi) 2048) -- 22 significant bits -- and x w = [hi hi' + (hi lo' + lo hi') / 2048] / (s s') to
 * 3 x 2^-22 relative: THREE fp16 MFMAs (v_mfma_f32_32x32x16_f16, two accumulators) instead of six, still far inside the rounding
 * of the fp32 accumulation over K = 9 Cin terms; elements more than 2^29 below the tensor's maximum lose relative (not absolute)
 * accuracy.  w2 = df_split_h2 of the weights with w_amax = df_absmax of them; shapes: df_conv2d_x3_ok.
 * df_absmax: *amax (a float, ZERO-initialised by the caller) <- max(*amax, max |x|) by an integer atomic max of the bit patterns
 * (exact, order-independent); a bound taken over a larger tensor that contains the operand is as good. */
int df_absmax(df_img x, float* amax, void* stream);
int df_split_h2(const float* w, const float* amax, void* out2, int64_t n, void* stream);
/* y_amax (optional, zero-initialised): the epilogue also leaves max |y| there -- the next fp16x2 kernel's bound, for free.
 * df_conv2d_amax: df_conv2d (the fp32-MFMA kernels: 1x1, stride 2) with the same by-product. */
int df_conv2d_h2(df_img x, const void* w2, const float* x_amax, const float* w_amax, const float* bias, df_img y, int ksize,
                 int stride, int pad, int mode, int epi, const float* scale, const float* shift, float* stats_partial,
                 int accumulate, float* y_amax, void* stream);
int df_conv2d_amax(df_img x, const float* w, const float* bias, df_img y, int ksize, int stride, int pad, int mode, int epi,
                   const float* scale, const float* shift, float* stats_partial, int accumulate, float* y_amax, void* stream);
/* fp16x2 for the convolutions without a haloed form (1x1, stride 2: conv_dma_kernel<.., H2>): the fp32 weights as they are,
 * fragments split in registers; bounds as for df_conv2d_h2 */
int df_conv2d_h2f(df_img x, const float* w, const float* x_amax, const float* w_amax, const float* bias, df_img y, int ksize,
                  int stride, int pad, int mode, int epi, const float* scale, const float* shift, float* stats_partial,
                  int accumulate, float* y_amax, void* stream);
/* ... with the weights also handed over PRE-SPLIT (w2: the [hi | lo] fp16 planes of w s_w from df_split_h2 / df_weight_prep): the
 * weight tiles go to LDS as planes by DMA and no wave splits a weight fragment (conv_dma_kernel<.., H2, BP>).  y.elt = 2: y_bound
 * defines the output planes (as df_conv2d_yh2), else y_amax (optional) receives max |y| (as df_conv2d_h2f).  [REF decoder.py:205-211] */
int df_conv2d_h2f_wp(df_img x, const float* w, const void* w2, const float* x_amax, const float* w_amax, const float* bias, df_img y,
                     const float* y_bound, int ksize, int stride, int pad, int mode, int epi, const float* scale, const float* shift,
                     float* stats_partial, int accumulate, float* y_amax, void* stream);
/* ... for the 1x1 skip convolution of an UpsampleSkip block (forward, bias epilogue; y = the SECOND half of the pre-split concatenation:
 * channels [t.c, 2 t.c) of pixels whose first t.c channels precede y.ptr) that ALSO writes the first half -- the bilinear x2 of
 * t [N, H/2, W/2, C] (fp32, F.interpolate semantics), scaled by *y_bound (>= max |t| too): one kernel writes whole pixels of the
 * concatenation.  Replaces df_upsample2x_h2 + df_conv2d_h2f_wp [REF deflow.py:32 FastFlow3DUNet's UpsampleSkip].  DF_E_SHAPE where
 * the 8-wave DMA kernels with pre-split weights do not cover the call. */
int df_conv2d_h2f_wp_up(df_img x, const float* w, const void* w2, const float* x_amax, const float* w_amax, const float* bias,
                        df_img y, const float* y_bound, df_img t, int align_corners, void* stream);
int df_conv2d_w16_ok(df_img x, df_img y, int ksize, int stride, int mode, int epi);
/* tile variant the launcher picks, as BM * 1000 + BN (for profiling tools) */
int df_conv2d_variant(int64_t rows, int64_t rows_per_stat_group, int cout, int epi);
int df_conv2d_last_dma(void); /* 1 if the previous df_conv2d call launched the LDS-DMA kernel (profiling tools) */
/* What the forward / data-gradient dispatch decides for a call, from its descriptors and the kind of its weights alone (no data
 * pointer is read, nothing is launched; the _ok queries above answer from the same plan).  weights: what the entry point hands over --
 * F32 df_conv2d / _mp / _amax / _yh2 without bounds, B16 df_conv2d_w16, X3 df_conv2d_x3, H2 df_conv2d_h2 / _h2p / _h2p_dgrad_bn, WP
 * df_conv2d_h2f_wp, F32_H2 df_conv2d_h2f / _yh2 with both bounds.  out [DF_CONV_PLAN_LEN]: kernel family (DF_CONV_FAM_*), BM, BN, WM, WN
 * (tile and wave grid), SEG (image rows per tile of the haloed 16-bit forms), DB (weight ring depth of the plane forms), planes per
 * operand (0: fp32 tiles), flags (DF_CONV_PLAN_*), statistics-table rows per tile.  Returns DF_OK, or the code the launch would refuse
 * with (out: family -1). */
#define DF_CONV_W_F32 0     /* fp32 [Cout, k*k, Cin] */
#define DF_CONV_W_B16 1     /* bf16 tiles (df_cast_bf16) */
#define DF_CONV_W_X3 2      /* three bf16 planes (df_split_bf16x3) */
#define DF_CONV_W_H2 3      /* two fp16 planes (df_split_h2) */
#define DF_CONV_W_WP 4      /* fp32 + pre-split planes for the DMA-tile kernel */
#define DF_CONV_W_F32_H2 5  /* fp32, split on the fragments (bounds of max |x| and max |w| given) */
#define DF_CONV_FAM_REG 0       /* conv_kernel: register-staged tiles */
#define DF_CONV_FAM_DMA 1       /* conv_dma_kernel */
#define DF_CONV_FAM_HALO 2      /* conv_halo_kernel: haloed fp32 tiles */
#define DF_CONV_FAM_HALO_W16 3  /* conv_halo_w16_kernel: haloed bf16 tiles */
#define DF_CONV_FAM_HALO_X3 4   /* conv_halo_x3_kernel: haloed planes */
#define DF_CONV_FAM_HALO_X3P 5  /* conv_halo_x3p_kernel: haloed pre-split planes, persistent */
#define DF_CONV_PLAN_XP 1    /* pre-split input */
#define DF_CONV_PLAN_X16 2   /* bf16 input */
#define DF_CONV_PLAN_BWS 4   /* DF_EPI_BWD_STATS epilogue */
#define DF_CONV_PLAN_DMA 8   /* operands by LDS-DMA (32-bit buffer offsets) */
#define DF_CONV_PLAN_CLS 16  /* stride-2 data gradient tiled per output-parity class */
#define DF_CONV_PLAN_LEN 10
int df_conv2d_plan(df_img x, df_img y, int ksize, int stride, int mode, int epi, int weights, int32_t* out);
/* BatchNorm2d training statistics from the partials. groups = stat groups (the shared encoder is
 * applied to pc0 then pc1: two calls => two groups, running stats updated in call order).
 * bn_ss [groups,4,C] = scale, shift, mean, invstd.  Optional two-stage reduction for layers with many tiles:
 * scratch [groups, splits, 2, C] doubles and splits > 1 (NULL / <= 1: single stage). */
int df_bn_finalize(const float* partial, int tiles_per_group, int groups, int C, int64_t count_per_group,
                   const float* gamma, const float* beta, float eps, float momentum,
                   float* running_mean, float* running_var, float* bn_ss, double* scratch, int splits, void* stream);
/* z = gelu(y * scale + shift) ; y plain [n,h,w,C]; imgs_per_group images share one stat group */
int df_bn_gelu_apply(const float* y, const float* bn_ss, int imgs_per_group, df_img z, void* stream);
/* backward of z = gelu(bn(y)): pass 1 partial sums [nblk, C, 2] of (dyh, dyh*xhat) */
int df_bn_gelu_bwd_reduce(df_img dz, const float* y, const float* bn_ss, int imgs_per_group,
                          float* partial, int nblk, void* stream);
/* finalize: dgamma/dbeta += over groups; coef [groups,2,C] = (S1/N, S2/N). partial rows are per group contiguous */
int df_bn_bwd_finalize(const float* partial, int nblk_per_group, int groups, int C, int64_t count_per_group,
                       float* dgamma, float* dbeta, float* coef, void* stream);
/* pass 2: dy = scale * (dyh - c1 - xhat * c2) (plain [n,h,w,C]); dbias partial [nblk, C] */
int df_bn_gelu_bwd_apply(df_img dz, const float* y, const float* bn_ss, const float* coef, int imgs_per_group,
                         float* dy, float* dbias_partial, int nblk, void* stream);
/* generic column sums: out[c] = sum over partial rows (used for conv bias grads etc.) */
/* bf16-STORAGE training (round 3): the same three passes with typed tensors.  *_elt / df_img.elt: 0 = float32, 1 = bfloat16;
 * arithmetic in fp32 registers either way.  df_bn_gelu_bwd_apply_t with dy_elt = 1 takes the bias-gradient column sums from
 * the ROUNDED dy (what the weight- and data-gradient kernels read).  Replaces the BatchNorm2d + GELU of ConvWithNorms and its
 * backward [REF decoder.py:202-220] when activations are kept in bfloat16 (Lightning precision="bf16-mixed" keeps them so). */
/* z_amax / dy_amax (optional, ZERO-initialised float): the pass also leaves max |z| resp. max |dy| there (integer atomic max of the
 * bit patterns, as df_absmax) for the fp16x2 convolution kernels that read the tensor next. */
int df_bn_gelu_apply_t(const void* y, int y_elt, const float* bn_ss, int imgs_per_group, df_img z, float* z_amax, void* stream);
int df_bn_gelu_bwd_reduce_t(df_img dz, const void* y, int y_elt, const float* bn_ss, int imgs_per_group, float* partial, int nblk,
                            void* stream);
int df_bn_gelu_bwd_apply_t(df_img dz, const void* y, int y_elt, const float* bn_ss, const float* coef, int imgs_per_group, void* dy,
                           int dy_elt, float* dbias_partial, int nblk, float* dy_amax, void* stream);
int df_colsum_partial(df_img x, float* partial, int nblk, void* stream);
int df_colsum_finalize(const float* partial, int nblk, int C, int nvals, float* out, int accumulate, void* stream);
/* first stage for very many partial rows: out[g][total] = sum of row group g (rows split evenly into `groups`);
 * finish with df_colsum_finalize(out, groups, ...) */
int df_colsum_stage(const float* partial, int nblk, int total, int groups, float* out, void* stream);
/* weight layout helpers: wt[ci][k][co] = w[co][k][ci] */
int df_weight_transpose(const float* w, float* wt, int cout, int taps, int cin, void* stream);
/* dW[co][k][ci] (row stride ldw elements between co rows... taps*cin when dense) = sum_p dy[p][co] x[p*s+k-pad][ci].
 * ws: splits * Cout * taps * Cin floats, splits = df_conv2d_wgrad_splits(...). */
int df_conv2d_wgrad_splits(df_img x, df_img dy, int ksize, int stride);
/* row_counts (optional, 1x1 with h == 1 only): pixel p is summed only if p % rows_per_seg < row_counts[p / rows_per_seg]
 * (padded per-sample point rows of the decoder).
 * bias_ws (optional) [splits, Cout]: per-split column sums of dy = the conv's bias gradient, produced from the dy tiles
 * the kernel stages anyway (sum its rows with df_colsum_finalize). */
int df_conv2d_wgrad(df_img x, df_img dy, int ksize, int stride, int pad, float* ws, int splits,
                    const int32_t* row_counts, int rows_per_seg, float* bias_ws, void* stream);
int df_conv2d_wgrad_mp(df_img x, df_img dy, int ksize, int stride, int pad, float* ws, int splits,
                       const int32_t* row_counts, int rows_per_seg, float* bias_ws, int mfma_bf16, void* stream);
int df_conv2d_wgrad_reduce(const float* ws, int splits, int cout, int taps, int cin, float* dw, int64_t ld_co,
                           int accumulate, void* stream);
/* the same reduction and the bias partials' (bias_ws [splits, Cout] -> db [Cout], summed in double) in ONE launch:
 * what a ConvWithNorms layer's weight + bias gradient [REF decoder.py:205,213] needs after its split-K pass */
int df_conv2d_wgrad_reduce_bias(const float* ws, int splits, int cout, int taps, int cin, float* dw, int64_t ld_co,
                                int accumulate, const float* bias_ws, float* db, void* stream);
/* fp32-ACCURATE 3x3 stride-1 weight gradient on the bf16 matrix pipe (round 3, "bf16x3", the twin of df_conv2d_x3): fp32 x and
 * dy, each staged element split into three bf16 planes, six exact products per operand pair, transposing LDS reads, fp32
 * accumulation and split-K partials.  splits / ws / bias_ws / df_conv2d_wgrad_reduce as df_conv2d_wgrad_mp.  _ok: 1 if the form
 * exists for the call (3x3, stride 1, W % 32 == 0, DMA-addressable tensors).  [REF decoder.py:205,213] weight gradient. */
int df_conv2d_wgrad_x3(df_img x, df_img dy, int ksize, int stride, int pad, float* ws, int splits, float* bias_ws, void* stream);
int df_conv2d_wgrad_x3_ok(df_img x, df_img dy, int ksize, int stride);
/* its fp16x2 form (wgrad3_x3_kernel<2>): x_amax / dy_amax as for df_conv2d_h2 */
int df_conv2d_wgrad_h2(df_img x, df_img dy, const float* x_amax, const float* dy_amax, int ksize, int stride, int pad, float* ws,
                       int splits, float* bias_ws, void* stream);
/* 1x1 weight gradient of fp32 x and dy with fp16x2 products (round 5, wgrad1_h2_kernel): dW[co, ci] = sum_p dy[p, co] x[p, ci] is a
 * row GEMM over the pixels that reads every operand byte once -- each staged element is split in flight into two scaled fp16 planes
 * (x_amax / dy_amax as for df_conv2d_h2), three MFMAs per product, so that the kernel runs at the memory system's pace instead of the
 * fp32 MFMA's.  _ok: 1 if the form takes the call (same geometry, Cin % 32 == 0, Cout % 64 == 0, DMA-addressable tensors;
 * DF_WGRAD1_H2=0: never); _splits: its split-K count; ws [splits][Cout][Cin], bias_ws [splits][Cout] or NULL, then
 * df_conv2d_wgrad_reduce(_bias) as for df_conv2d_wgrad_mp.  x_amax = dy_amax = NULL: the bf16-MFMA training mode's form (ONE bf16
 * plane per operand, one MFMA per product; also for df_conv2d_wgrad_s2_h2).  [REF decoder.py:205,213] weight gradient of the UNet's 1x1 convolutions
 * (the reference's backbone: scripts/network/models/basic/unet.py UpsampleSkip u1 / u3 through torch autograd). */
int df_conv2d_wgrad1_h2_ok(df_img x, df_img dy);
int df_conv2d_wgrad1_h2_splits(df_img x, df_img dy);
int df_conv2d_wgrad1_h2(df_img x, df_img dy, const float* x_amax, const float* dy_amax, float* ws, int splits, float* bias_ws,
                        void* stream);
/* the 3x3 STRIDE-2 (pad 1) weight gradient of fp32 x and dy with fp16x2 products (round 5, wgrad3s2_h2_kernel): the two
 * downsampling layers' form of df_conv2d_wgrad_h2 -- elements split in flight, input columns de-interleaved in LDS so that a tap's
 * 16 pixels are consecutive rows of the transposing-read image.  _ok / _splits / ws [splits][Cout][9][Cin] / bias_ws / reduce as
 * above (DF_WGRAD_S2_H2=0: never).  [REF decoder.py:205,213] weight gradient of the UNet encoder's stride-2 ConvWithNorms. */
int df_conv2d_wgrad_s2_h2_ok(df_img x, df_img dy);
int df_conv2d_wgrad_s2_h2_splits(df_img x, df_img dy);
int df_conv2d_wgrad_s2_h2(df_img x, df_img dy, const float* x_amax, const float* dy_amax, float* ws, int splits, float* bias_ws,
                          void* stream);
/* bf16-STORAGE training (round 3): the 3x3 stride-1 weight gradient of BFLOAT16 x and dy (df_img.elt = 1 on both; W % 32 == 0):
 * bf16 tiles by LDS-DMA into a four-deep ring, fragments by transposing LDS reads (ds_read_b64_tr_b16), fp32 accumulation and
 * fp32 split-K partials.  splits / ws / bias_ws / df_conv2d_wgrad_reduce exactly as df_conv2d_wgrad_mp.  Replaces the weight
 * gradient autograd takes for the Conv2d of ConvWithNorms [REF decoder.py:205,213] under bf16 autocast. */
int df_conv2d_wgrad_bf16(df_img x, df_img dy, int ksize, int stride, int pad, float* ws, int splits, float* bias_ws, void* stream);
/* bf16 inference convolution (BASELINE configs[4], "bf16 MFMA"): x, w bf16 (NHWC / [Cout,kh,kw,Cin]), fp32 accumulation on
 * v_mfma_f32_32x32x16_bf16, epilogue DF_EPI_BIAS or DF_EPI_BN_GELU in fp32, output bf16 (out_f32 = 0) or fp32.
 * df_img element counts (c, ld, strides) are in elements of the respective type; Cin, Cout multiples of 64.
 * df_cast_bf16: y[row][c] = bf16(x[row*ldx + c]) for c < cin, 0 for cin <= c < cout (channel padding). */
int df_conv2d_bf16(df_img x, const void* w, const float* bias, df_img y, int ksize, int stride, int pad, int epi,
                   const float* scale, const float* shift, int out_f32, void* stream);
int df_cast_bf16(const float* x, void* y, int64_t rows, int cin, int ldx, int cout, void* stream);
int df_upsample2x_bf16(df_img x, df_img y, int align_corners, void* stream); /* bf16 in / out, fp32 lerp */
/* bilinear x2 (PyTorch F.interpolate semantics, align_corners selectable), forward and backward */
int df_upsample2x(df_img x, df_img y, int align_corners, void* stream);
int df_upsample2x_bwd(df_img dy, df_img dx, int align_corners, void* stream);
/* ... into a pre-split dx (dx.elt = 2; "PRE-SPLIT tensors" below), scaled by *dx_bound >= max |dx| (4.5 max |dy| always holds): the
 * planes df_h2_pack makes of df_upsample2x_bwd's output with that bound, bit for bit -- for a dx that is the output gradient of a
 * composed 3x3 layer (df_weight_prep), whose consumers are the pre-split data- and weight-gradient kernels */
int df_upsample2x_bwd_h2(df_img dy, df_img dx, int align_corners, const float* dx_bound, void* stream);

/* ---- PRE-SPLIT ("h2") tensors, round 4: the operands of the fp16x2 kernels written split by their PRODUCERS -------------------
 * df_img.elt = 2: the tensor has the geometry of its fp32 form (4 bytes per element: ld / img_stride / grp_off unchanged), but per
 * pixel and 32-channel chunk the 128-byte line holds [32 x fp16 hi | 32 x fp16 lo] with  x s = hi + lo / 2048,  s = the power of
 * two that puts a BOUND of max |x| into [2^14, 2^15).  The bound is a device scalar known BEFORE the producer writes (BatchNorm
 * statistics, weight norms: below), so nothing synchronises; every consumer takes the SAME scalar.  Requirements: c, ld,
 * img_stride, grp_off multiples of 32, 128-byte aligned base.  What this replaces in the reference: nothing -- it is the storage
 * form of the activations / gradients between `ConvWithNorms` / `UpsampleSkip` layers ([REF decoder.py:202-220]) inside this
 * engine; results stay those of the fp32 tensors to 22 significant bits.
 *   df_conv2d_h2p        df_conv2d_h2 with x and / or y as h2 images (x_amax = the bound that defined x; y_bound defines y)
 *   df_conv2d_yh2        the fp32-input kernels (1x1, stride 2; fp32 MFMA or fp16x2-on-fragments when x_amax / w_amax are given)
 *                        writing an h2 output
 *   df_conv2d_wgrad_h2p  3x3 stride-1 weight gradient of h2 x and dy (LDS-DMA ring, no in-kernel split)
 *   df_bn_finalize2 / df_bn_bwd_finalize2   the finalisations, also leaving the bound of the z / dy their apply pass writes next
 *                        (z_bound / dy_bound: zero-initialised slots, integer atomic max): df_bn_gelu_apply_t with z.elt = 2 and
 *                        df_bn_gelu_bwd_apply_t with dy_elt = 2 take that scalar in their z_amax / dy_amax argument (an INPUT then)
 *   df_upsample2x_h2, df_h2_pack / df_h2_unpack, df_rows_l1max, df_h2_bound   helpers (see csrc/elementwise.hip) */
int df_conv2d_h2p(df_img x, const void* w2, const float* x_amax, const float* w_amax, const float* bias, df_img y, const float* y_bound,
                  int ksize, int stride, int pad, int mode, int epi, const float* scale, const float* shift, float* stats_partial,
                  int accumulate, float* y_amax, void* stream);
int df_conv2d_h2p_ok(df_img x, df_img y, int ksize, int stride, int mode, int epi);
/* the 3x3 stride-1 fp16x2 data gradient whose epilogue also leaves the BatchNorm + GELU backward's partial sums of the layer in front
 * (replaces df_bn_gelu_bwd_reduce's pass over dz and y): see csrc/conv.hip */
int df_conv2d_h2p_dgrad_bn(df_img x, const void* w2, const float* x_amax, const float* w_amax, df_img dz, const float* bn_y,
                           const float* bn_ss, float* bwd_partial, float* dz_amax, void* stream);
int df_conv2d_yh2(df_img x, const float* w, const float* x_amax, const float* w_amax, const float* bias, df_img y, const float* y_bound,
                  int ksize, int stride, int pad, int mode, int epi, const float* scale, const float* shift, float* stats_partial,
                  int accumulate, void* stream);
int df_conv2d_wgrad_h2p(df_img x, df_img dy, const float* x_bound, const float* dy_bound, int ksize, int stride, int pad, float* ws,
                        int splits, float* bias_ws, void* stream);
int df_conv2d_wgrad_h2p_ok(df_img x, df_img dy, int ksize, int stride);
int df_conv2d_wgrad_h2p_splits(df_img x, df_img dy);   /* split-K count for df_conv2d_wgrad_h2p (one resident workgroup per CU) */
int df_bn_finalize2(const float* partial, int tiles_per_group, int groups, int C, int64_t count_per_group, const float* gamma,
                    const float* beta, float eps, float momentum, float* running_mean, float* running_var, float* bn_ss,
                    double* scratch, int splits, const float* y_amax, float* z_bound, void* stream);
int df_bn_bwd_finalize2(const float* partial, int nblk_per_group, int groups, int C, int64_t count_per_group, float* dgamma,
                        float* dbeta, float* coef, const float* bn_ss, const float* dz_amax, const float* y_amax, float* dy_bound,
                        void* stream);
int df_upsample2x_h2(df_img x, df_img y, int align_corners, const float* y_bound, void* stream);
int df_h2_pack(df_img x, const float* bound, df_img y, void* stream);
int df_h2_unpack(df_img x, const float* bound, df_img y, void* stream);
int df_rows_l1max(const float* w, int rows, int row_len, const float* bias, int nbias, float* l1max, float* bmax, void* stream);
int df_h2_bound(float* out, const float* a, const float* l1, const float* b, const float* other, float slack, void* stream);
/* all convolution layers' per-step weight forms in ONE launch: transposed weights, [hi | lo] fp16 planes of both, row L1 norms and
 * max |bias| for the a-priori bounds (replaces ~80 df_weight_transpose / df_split_h2 / df_rows_l1max launches per training step).
 * table: nlayers records {int64 w_off, b_off (elements in `params`; b_off < 0: none), wt_off, w2_off, wt2_off (floats in `out`);
 * int32 cout, taps, cin, split, blk0 (first workgroup of the layer = sum of cout + cin of the layers before), pad};
 * norms [nlayers][3] = (max row L1 of w, of w^T, max |bias|), zero-initialised by the caller; w_amax = max |p| over the arena */
int df_weight_prep(const float* params, const void* table, int nlayers, int total_blocks, const float* w_amax, float* out, float* norms,
                   void* stream);
/* COMPOSED layers (unless DF_FUSE_U5U1=0): a record with pad > 0 is the 3x3 layer  We[o][tap][i] = sum_c W1[o][c] W5[c][tap][i],
 * be[o] = sum_c W1[o][c] b5[c] + b1[o]  of an UpsampleSkip block's last 3x3 convolution (W5, b5) and the next block's 1x1 (W1, b1), which
 * is its only reader [REF deflow.py:32].  Its w_off / b_off address `out` (We [O][taps][I] and be, written by a compose launch inside
 * df_weight_prep before the forms are made); tab[pad], a record past the nlayers ordinary ones, names the sources: w_off = W5, b_off =
 * b5, wt_off = W1, w2_off = b1 (elements in `params`), wt2_off = the index in `norms` (past [nlayers][3], zero-initialised with them)
 * of the slot that receives max |We| -- the scale of the composed layer's planes --, cout = C, taps, cin = I, split = O (O % 8 == 0).
 * df_u5u1_decompose: the four parameter gradients from the composed layer's weight gradient dwe [O][taps][I] and bias sum dbe [O]:
 *   dw5[c][tap][i] = sum_o W1[o][c] dwe[o][tap][i]      dw1[o][c] = sum_{tap,i} dwe[o][tap][i] W5[c][tap][i] + dbe[o] b5[c]
 *   db5[c] = sum_o W1[o][c] dbe[o]                      db1 = dbe
 * (O, C % 16 == 0, I % 64 == 0; sums in ascending index order in double, no float atomics: bit-reproducible) */
int df_u5u1_decompose(const float* w1, const float* w5, const float* b5, const float* dwe, const float* dbe, int O, int C, int taps,
                      int I, float* dw5, float* db5, float* dw1, float* db1, void* stream);
/* The SECOND kind of composed layer (unless DF_FUSE_U3U4=0 or DF_FUSE_U5U1=0): an UpsampleSkip block's 1x1 skip convolution (W3 [lat][lat],
 * b3) folded into the block's first 3x3 (W4 [O][taps][2 lat] = [W4a | W4b], b4, zero padding 1), which is its only reader [REF deflow.py:32]:
 *   We[o][tap][:lat] = W4a[o][tap][:]     We[o][tap][lat + i] = sum_c W4b[o][tap][c] W3[c][i]
 *   beta[o][tap] = sum_c W4b[o][tap][c] b3[c]     be[o] = b4[o] + sum_tap beta[o][tap]
 * The layer then reads [up(t) | b] instead of [up(t) | u3(b)].  Its record has pad > 0 like the first kind; the source record tab[pad]
 * carries pad = 1 and  w_off = W4, b_off = b4, wt_off = W3, w2_off = b3 (elements in `params`), wt2_off = the `norms` slot of max |We|,
 * cout = O (O % 8 == 0), taps, cin = 2 lat, split = lat.  beta [O][taps] is stored in `out` behind be (at b_off + (O rounded up to 64)),
 * and norms[layer][2] also covers max_o (|b4[o]| + sum_tap |beta[o][tap]|): the bias side of the layer's a-priori output bound.
 * At a border pixel the taps outside the image carry no b3 term: df_u3u4_border_fix subtracts  sum_{taps outside} beta[o][tap]  from the
 * border pixels of the layer's output y (an h2 image of O channels with bound *y_bound; taps = 9). */
int df_u3u4_border_fix(df_img y, const float* y_bound, const float* beta, void* stream);
/* whole pixels of that layer's pre-split input cat [N,2h,2w,2 lat] (h2, scale of *cat_bound >= max(max |t|, max |b|)): channels [0, lat) =
 * bilinear x2 of t [N,h,w,lat] (the planes df_upsample2x_h2 writes, bit for bit), channels [lat, 2 lat) = b [N,2h,2w,lat] (the planes
 * df_h2_pack writes); t, b fp32 */
int df_cat_pack_up(df_img t, df_img b, df_img cat, int align_corners, const float* cat_bound, void* stream);
/* the tap sums of the layer's output gradient dy (h2 image [N,H,W,O], bound *dy_bound; dbe [O] = its column sum over all pixels):
 *   T[o][tap] = sum_{p : p + tap inside} dy[o][p]  = dbe less the border row / column the tap excludes, plus the corner taken off twice
 * from the border sums  part[q][n][o] (workspace, 8 N O doubles), q = 0 row 0, 1 row H-1, 2 column 0, 3 column W-1, 4..7 the corners
 * (0,0), (0,W-1), (H-1,0), (H-1,W-1), per image in double; two small launches, every sum in a fixed order.  T [O][9] doubles */
int df_u3u4_border_sums(df_img dy, const float* dy_bound, const float* dbe, double* part, double* T, void* stream);
/* the five parameter gradients from the composed layer's weight gradient dwe [O][9][2 lat] and T:
 *   dw4[o][tap][:lat] = dwe[o][tap][:lat]      dw4[o][tap][lat + c] = sum_i W3[c][i] dwe[o][tap][lat + i] + b3[c] T[o][tap]
 *   dw3[c][i] = sum_{o,tap} W4b[o][tap][c] dwe[o][tap][lat + i]      db3[c] = sum_{o,tap} W4b[o][tap][c] T[o][tap]      db4[o] = T[o][centre]
 * w3t = W3 transposed [i][c] (df_weight_prep's wt).  O % 8 == 0, lat % 16 == 0; sums in a fixed index order in double */
int df_u3u4_decompose(const float* w3t, const float* w4, const float* b3, const float* dwe, const double* T, int O, int lat, float* dw4,
                      float* db4, float* dw3, float* db3, void* stream);

/* ------------------------------------------------------- point decoder (A6-A10) --------
 * Replaces ConvGRUDecoder / LinearDecoder forward_single ([REF decoder.py:72-199]): integer
 * gather of the 2x64 pillar vectors, offset encoder, num_iters GRU steps, MLP head.        */
typedef struct df_gru_weights {
  const float* w_off; const float* b_off;   /* [64,3], [64]                       */
  const float* w_zr;  const float* b_zr;    /* [256,192] (z rows then r rows), [256] */
  const float* w_q;   const float* b_q;     /* [128,192], [128]                   */
  const float* w_1;   const float* b_1;     /* [32,192], [32]                     */
  const float* w_2;   const float* b_2;     /* [3,32], [3]                        */
} df_gru_weights;
/* before/after: n=B images of 64 channels.  coords [B,N,3] i32 (z,y,x), offs [B,N,3], counts [B] (device).
 * flow [B,N,3] (rows >= counts[b] untouched).  save (training, may be NULL):
 *   [5, T, B*N, 128] = h_in, z, r, q, r*h per iteration, then hT [B*N,128]. */
int df_gru_decoder_fwd(df_img before, df_img after, const int32_t* coords, const float* offs,
                       const int32_t* counts, int B, int N, int num_iters, df_gru_weights wts,
                       float* flow, float* save, void* stream);
/* mixed-precision form (Trainer(dtype="bf16")): mfma_bf16 != 0 rounds the operands of every gate / head GEMM to bf16 on the
 * way into v_mfma_f32_16x16x32_bf16; hidden state, gate math and accumulators stay fp32.  The saved planes h_in, z, r, q, r*h
 * (and the gate-gradient planes the backward puts in their place) are then stored as bf16 -- 128 values in the first 256 bytes
 * of each row's 512-byte slot, offsets as in the fp32 layout -- which halves the dominant HBM stream of the three kernels; hT
 * stays fp32.  df_gru_decoder_fwd_mp, df_gru_decoder_bwd_mp and df_gru_wgrad_mp of one step must get the same mfma_bf16 (zero or
 * not).  mfma_bf16 == 2 (forward and backward): the GEMM weights -- wts.w_zr, wts.w_q, wts.w_1 and wtt.wt_zr, wtt.wt_q, wtt.wt_1
 * -- point at bf16 COPIES of the same [rows, cols] arrays (cast once per optimizer step); their tiles are then bf16 in LDS and
 * every weight fragment is one 16-byte read.  All other fields of the weight structs stay fp32.
 * mfma_bf16 == 3 (forward and backward; round 3, the default of fp32 training): "bf16x2" -- both operands of every gate / head
 * GEMM as two bf16 planes (hi + lo: 16 significant bits), three MFMAs per product; planes saved fp32 exactly as with 0 (the
 * weight-gradient pass gets 0).  The same six weight pointers then hold rows of [hi (cols) | lo (cols)] bfloat16
 * (df_split_bf16x2_rows of the [rows, cols] fp32 arrays, once per optimizer step). */
int df_split_bf16x2_rows(const float* w, void* out, int64_t rows, int ld, void* stream);
int df_gru_decoder_fwd_mp(df_img before, df_img after, const int32_t* coords, const float* offs, const int32_t* counts,
                          int B, int N, int num_iters, df_gru_weights wts, float* flow, float* save, int mfma_bf16,
                          void* stream);
typedef struct df_gru_weights_t {          /* transposed copies (df_weight_transpose) for the data-gradient GEMMs */
  const float* wt_zr; /* [192,256] */
  const float* wt_q;  /* [192,128] */
  const float* wt_1;  /* [192,32]  */
} df_gru_weights_t;
/* backward data pass.  Consumes dflow [B,N,3] and the forward's `save`; overwrites save's z, r, q planes with
 * dz_pre, dr_pre, dq_pre (inputs of the weight-gradient GEMMs); writes dh0 [B*N,128], dx [B*N,64], dpre1 [B*N,32],
 * xout [B*N,64] (rows of valid points only), and per-workgroup partial sums of every small gradient:
 * partial [B * ceil(N/64), 772] = d b_z|b_r|b_q (384) | d b_1 (32) | dW_off[64][3] (192) | d b_off (64) | dW_2[3][32] (96) |
 * d b_2 (3) | pad.  `partial` must be zero-filled (workgroups with no valid point do not write); sum its rows with
 * df_colsum_finalize. */
int df_gru_decoder_bwd(const float* dflow, const float* offs, const int32_t* counts, int B, int N, int num_iters,
                       df_gru_weights wts, df_gru_weights_t wtt, float* save, float* dh0, float* dx, float* dpre1,
                       float* xout, float* partial, void* stream);
int df_gru_decoder_bwd_mp(const float* dflow, const float* offs, const int32_t* counts, int B, int N, int num_iters,
                          df_gru_weights wts, df_gru_weights_t wtt, float* save, float* dh0, float* dx, float* dpre1,
                          float* xout, float* bias_partial, int mfma_bf16, void* stream);
/* Weight gradients of the three GRU gate convolutions in one streaming pass over the planes df_gru_decoder_fwd saved
 * and df_gru_decoder_bwd overwrote (replaces autograd's six 1x1 conv weight-gradient GEMMs over [REF decoder.py:139-147]):
 * ws[split][384][192] partial tiles, rows 0..127 dW_z, 128..255 dW_r, 256..383 dW_q, columns [h | x]; sum the splits
 * with df_conv2d_wgrad_reduce(ws, splits, 384, 1, 192, ...).  x = the [B*N,64] offset encoding df_gru_decoder_bwd wrote. */
int df_gru_wgrad_splits(void);
/* round 4: the head's first-layer weight gradient dW1 [32][192] = dpre1^T [hT | x] over the valid rows in one streaming pass
 * (partials ws [nsplit][32][192], summed by df_conv2d_wgrad_reduce); bf16x2 products.  [REF decoder.py:151-153,182] differentiated */
int df_gru_head_wgrad(const float* dpre, const float* hT, const float* x, const int32_t* counts, int B, int N, float* ws, int nsplit,
                      void* stream);
int df_gru_wgrad(const float* save, const float* x, const int32_t* counts, int B, int N, int num_iters, float* ws,
                 int nsplit, void* stream);
int df_gru_wgrad_mp(const float* save, const float* x, const int32_t* counts, int B, int N, int num_iters, float* ws,
                    int nsplit, int mfma_bf16, void* stream);

/* ---- round 5: the "lean" ConvGRU decoder (csrc/decoder4.hip) -- the engine's default; the entries above (the full form: every
 * plane saved) remain as the tested alternate and for saving forwards of 2^31 bytes or more per plane ----
 * Same computation as df_gru_decoder_fwd_mp / _bwd_mp / df_gru_wgrad_mp ([REF decoder.py:123-199] and its derivative), two changes:
 *  (1) x = W_off o + b_off [REF decoder.py:172] is affine in the point's 3 offsets and enters every gate and the head linearly
 *      [REF decoder.py:126-139,151,182], so its contribution is evaluated from a [416][4] table (rows z | r | q | head layer 1:
 *      W[:, 128:] W_off | W[:, 128:] b_off + b) as 3 FMAs per value -- df_gru_xtab builds it from the fp32 parameters once per
 *      optimizer step -- and backwards every x-side product collapses onto [416][4] sums S (plain and offset-weighted column sums of
 *      the gate / head pre-activation gradients) which df_gru_lean_finalize turns into dW[:, 128:], d b, dW_off, d b_off;
 *  (2) the forward saves only the hidden state entering each iteration and h_T, hsave [T + 1][B*N][128] (bf16 modes: planes
 *      0 .. T-1 as bf16 half rows); the backward recomputes z, r, q and writes gplanes [4][T][B*N][128] = dz_pre | dr_pre | dq_pre |
 *      r * h for df_gru_lean_wgrad, which multiplies the 128 h columns only: ws [nsplit][384][128] (reduce with
 *      df_conv2d_wgrad_reduce(ws, nsplit, 384, 1, 128, dW, 192, ...)).  df_gru_lean_head_wgrad: ws [nsplit][32][128] = dpre1^T hT.
 * wts: w_zr, w_q, w_1 (and wtt.*) in the form mfma_bf16 selects, exactly as for the _mp entries; w_2, b_2 fp32; the bias and
 * offset-encoder fields are read by df_gru_xtab / df_gru_lean_finalize only (which take the fp32 struct).
 * partial: [B * ceil(N / 64)][df_gru_lean_partial_width()] zero-filled; its column sums = S [416][4] | dW_2 [3][32] | d b_2 [3] | pad.
 * df_gru_lean_finalize: dW_gates [384][192] and dW1 [32][192] get their columns 128..191; db [416] = d b_z | d b_r | d b_q | d b_1. */
int df_gru_xtab(df_gru_weights wts, float* xtab, void* stream);
int df_gru_lean_partial_width(void);
int df_gru_lean_fwd(df_img before, df_img after, const int32_t* coords, const float* offs, const int32_t* counts, int B, int N,
                    int num_iters, df_gru_weights wts, const float* xtab, float* flow, float* hsave, int mfma_bf16, void* stream);
int df_gru_lean_bwd(const float* dflow, const float* offs, const int32_t* counts, int B, int N, int num_iters, df_gru_weights wts,
                    df_gru_weights_t wtt, const float* xtab, const float* hsave, float* gplanes, float* dh0, float* dpre1,
                    float* partial, int mfma_bf16, void* stream);
int df_gru_lean_wgrad(const float* hsave, const float* gplanes, const int32_t* counts, int B, int N, int num_iters, float* ws,
                      int nsplit, int mfma_bf16, void* stream);
int df_gru_lean_head_wgrad(const float* dpre, const float* hT, const int32_t* counts, int B, int N, float* ws, int nsplit,
                           void* stream);
int df_gru_lean_finalize(const float* sums, df_gru_weights wts, float* dW_gates, float* dW1, float* dW_off, float* db_off, float* db,
                         void* stream);
/* gather backward without atomics: every BEV cell sums the dh0 rows of its own pc0 points (cell_rng / idx_sorted /
 * cpos from the pillarise step).  dbefore / dafter (64 ch each) are fully written (zeros for empty cells) or,
 * with accumulate_* != 0, added to.  dbefore.ptr == NULL skips the `before` image. */
int df_gather_bwd(const float* dh0, const uint32_t* idx_sorted, const int32_t* cell_rng, const int32_t* cpos,
                  int B, int N, df_img dbefore, df_img dafter, int accumulate_before, int accumulate_after,
                  int nblk, void* stream);
/* the same, and amax_after (a ZEROED device scalar) receives max |dafter| of what the call writes: the bound the UNet backward's first
 * fp16x2 data gradient scales dv by, without a pass over the image (round 5).  dafter is written, never added to.  Returns DF_E_SHAPE
 * where only the one-cell-at-a-time kernel applies (>= 2^29 points or >= 2^28 cells per image): call df_gather_bwd + df_absmax then. */
int df_gather_bwd_m(const float* dh0, const uint32_t* idx_sorted, const int32_t* cell_rng, const int32_t* cpos,
                    int B, int N, df_img dbefore, df_img dafter, int accumulate_before, int nblk, float* amax_after, void* stream);
/* partial[blk][i*nb+j] = sum over valid rows of a[row][i] * (b ? b[row][j] : 1); row r is valid iff
 * r % rows_per_seg < counts[(r / rows_per_seg) % nseg].  na*nb <= 256.  Sum with df_colsum_finalize. */
int df_small_outer(const float* a, int lda, int na, const float* b, int ldb, int nb, const int32_t* counts,
                   int rows_per_seg, int nseg, int64_t rows, float* partial, int nblk, void* stream);
/* ConvGRUDecoder forward with the gate GEMMs and the first head layer on bf16 MFMA (inference, BASELINE configs[4]):
 * w_zr [256,192], w_q [128,192], w_1 [32,192] bf16; everything else (images, biases, offset encoder, last layer, state,
 * gate non-linearities, accumulation) fp32. */
int df_gru_decoder_fwd_bf16(df_img before, df_img after, const int32_t* coords, const float* offs, const int32_t* counts,
                            int B, int N, int num_iters, const float* w_off, const float* b_off, const void* w_zr,
                            const float* b_zr, const void* w_q, const float* b_q, const void* w_1, const float* b_1,
                            const float* w_2, const float* b_2, float* flow, void* stream);
/* LinearDecoder ([REF decoder.py:72-120]) forward: w_off [128,3], w_1 [32,256], w_2 [3,32] */
int df_linear_decoder_fwd(df_img before, df_img after, const int32_t* coords, const float* offs,
                          const int32_t* counts, int B, int N, const float* w_off, const float* b_off,
                          const float* w_1, const float* b_1, const float* w_2, const float* b_2,
                          float* flow, void* stream);

/* LinearDecoder backward data pass (recomputes gather + hidden layer).  wt_1 = W1^T [256,32].  Writes
 * vx [B*N,256] = [before|after|offset_enc] rows, dh0 [B*N,128], dxe [B*N,128] (grad of the offset encoding),
 * dpre1 [B*N,32], hid [B*N,32]; weight gradients follow with df_conv2d_wgrad / df_small_outer, image gradients
 * with df_gather_bwd. */
int df_linear_decoder_bwd(df_img before, df_img after, const int32_t* coords, const float* offs, const int32_t* counts,
                          const float* dflow, int B, int N, const float* w_off, const float* b_off, const float* w_1,
                          const float* b_1, const float* w_2, const float* wt_1, float* vx, float* dh0, float* dxe,
                          float* dpre1, float* hid, void* stream);

/* ------------------------------------------------------------ ego motion + loss --------*/
/* [REF deflow.py:60-77]: pc0' = pc0 R^T + t ; pose_flow = pc0' - pc0.  T [B,4,4] row-major. */
int df_ego_transform(const float* pc0, const float* T, int B, int N, float* pc0_t, float* pose_flow, void* stream);
/* deflowLoss over padded per-sample rows (rows < counts[b]): partial [B,nblk,3,2] (sum err, count);
 * finalize -> bins [B,3,2], loss[0] = sum_b sum_bins mean; bwd -> dest = gscale * (*gscale_dev) * dloss/dest. */
int df_deflow_loss_fwd(const float* est, const float* gt, const int32_t* counts, int B, int N,
                       float* bins_partial, int nblk, void* stream);
int df_deflow_loss_finalize(const float* bins_partial, int B, int nblk, float* bins, float* loss, void* stream);
int df_deflow_loss_bwd(const float* est, const float* gt, const int32_t* counts, int B, int N, const float* bins,
                       const float* gscale_dev /*nullable*/, float gscale, float* dest, int nblk, void* stream);
/* the ablation losses of the reference's loss_fn switch (round 5; [REF assets/slurm/1_train.sh:53-60], README.md:68): kind 0 = ff3dLoss
 * (weight 0.1 on background points -- class cls[b, idx_c[b, i]] == 0 of compact row i; cls [B, Ncls] int64 -- 1.0 elsewhere), kind 1 =
 * zeroflowLoss (weight clamp(1.8 * 10 |gt| - 0.8, 0.1, 1.0); cls / idx_c unused): sum over samples of the mean over valid rows of
 * w |est - gt|.  fwd -> partial [B, nblk, 2]; finalize -> bins [B, 2] = (sum w err, rows), loss[0]; bwd -> dest as df_deflow_loss_bwd. */
int df_wloss_fwd(const float* est, const float* gt, const int32_t* counts, int B, int N, int kind, const int64_t* cls,
                 const int64_t* idx_c, int Ncls, float* partial, int nblk, void* stream);
int df_wloss_finalize(const float* partial, int B, int nblk, float* bins, float* loss, void* stream);
int df_wloss_bwd(const float* est, const float* gt, const int32_t* counts, int B, int N, int kind, const int64_t* cls,
                 const int64_t* idx_c, int Ncls, const float* bins, const float* gscale_dev /*nullable*/, float gscale, float* dest,
                 int nblk, void* stream);
/* trainer gt: gt[b,i] = flow[b, idx_c[b,i]] - pose_flow[b, idx_c[b,i]] for i < counts[b] */
int df_gather_gt(const float* flow, const float* pose_flow, const int64_t* idx_c, const int32_t* counts,
                 int B, int N, float* gt, int nblk, void* stream);

/* ------------------------------------------------------------------ chamfer nearest neighbour (SeFlow losses) ----
 * The counterpart of the reference's chamfer3D extension [REF README.md:39] (UNPINNED: its source is in the absent submodule), as a
 * grid search instead of upstream's all-pairs kernel.  Batched and padded: query [B,Nq,3] f32 with qcount [B] i32 valid leading rows,
 * ref [B,Nr,3] f32 with rcount [B]; optional row labels (i32, [B,Nq] / [B,Nr]): when given only rows with label > 0 take part.
 * Non-finite rows do not take part.
 * df_nn_grid_build: the participating ref rows in a uniform xy grid of G x G cells of `cell` metres from (minx, miny) per sample (rows
 *   outside go to the clamped border cells; z is not binned): cell_rng [B*G*G, 2] i32 = [start, end) of each cell in `sorted`
 *   [B*Nr, 4] f32 = (x, y, z, bits of the row index), rows of a cell in ascending row order.  ws: df_nn_grid_ws_bytes(B, Nr, G).
 * df_chamfer_nn: d2 [B,Nq] f32 = smallest squared distance (differences formed in fp32) from each participating query row to a
 *   participating ref row of its sample, idx [B,Nq] i32 = that row (lowest index on equal distances); d2 = +inf, idx = -1 where that
 *   distance exceeds max_dist2 (+inf allowed: exact unbounded search), no ref row participates or the query row does not.
 *   far_count (nullable, i32[1], integer atomic add): queries whose search went past the 3 x 3 cells around their own.
 * df_chamfer_bwd: for d2[i] = |query_i - ref[idx_i]|^2 and g [B,Nq] = d loss / d d2 (rows with idx < 0 are skipped):
 *   dquery [B,Nq,3] += 2 g_i (query_i - ref[idx_i]);  dref [B,Nr,3] += sum over i with idx_i == k of 2 g_i (ref_k - query_i), the
 *   pairs segmented by k and summed in ascending i (no float atomics: repeated calls are bit-identical).  Either output may be
 *   NULL; ws (needed for dref): df_chamfer_bwd_ws_bytes(B, Nq, Nr).
 * B * Nq, B * Nr, B * G * G < 2^30 (32-bit keys and sorted positions), G <= 4096, B <= 65535; violations return DF_E_SHAPE. */
int64_t df_nn_grid_ws_bytes(int B, int Nr, int G);
int df_nn_grid_build(const float* ref, const int32_t* rcount, const int32_t* rlabel /*nullable*/, int B, int Nr, float minx, float miny,
                     float cell, int G, int32_t* cell_rng, float* sorted, void* ws, void* stream);
int df_chamfer_nn(const float* query, const int32_t* qcount, const int32_t* qlabel /*nullable*/, int B, int Nq, const int32_t* cell_rng,
                  const float* sorted, float minx, float miny, float cell, int G, float max_dist2, float* d2, int32_t* idx,
                  int32_t* far_count /*nullable*/, void* stream);
int64_t df_chamfer_bwd_ws_bytes(int B, int Nq, int Nr);
int df_chamfer_bwd(const float* query, const float* ref, const int32_t* idx, const float* g, int B, int Nq, int Nr, float* dquery,
                   float* dref, void* ws, void* stream);

/* ------------------------------------------------------------------ DBSCAN cluster labels (SeFlow mode) ----
 * The cluster labels of the self-supervised mode, computed on the GPU.  UNPINNED: upstream clusters offline on the CPU (process.py:
 * DUFO dynamic flags, then HDBSCAN, whose source is in the absent submodule); this is plain DBSCAN with every choice fixed, so that the
 * result is a pure function of the input.  Per sample of a padded batch points [B,N,3] f32 with count [B] i32:
 *   participating rows  i < count[b], all three coordinates finite, and mask[b,i] != 0 when a mask is given (the grid build's rlabel > 0)
 *   neighbourhood       N(i) = the participating j with |p_i - p_j|^2 <= eps^2, i itself included; differences are formed first and then
 *                       squared, in fp32, as df_chamfer_nn does
 *   core rows           |N(i)| >= min_points
 *   clusters            two core rows within eps are linked; a cluster is a connected component of core rows plus its border rows
 *   border rows         a non-core row with a core row in N(i) joins the cluster of its nearest core row, the lowest row index on equal
 *                       distances (df_chamfer_nn's tie rule)
 *   noise               every other row: label 0, like the rows that do not participate
 *   filters             a cluster of fewer than min_cluster_size members is dropped to 0; with a per-row `dynamic` flag [B,N] i32 a cluster
 *                       is dropped too when flagged members < min_dynamic_frac * members (compared in float64)
 *   numbering           the surviving clusters are 1..K per sample, in ascending order of their lowest core row index
 * Defaults of the Python layer: eps = 0.7 and min_cluster_size = 20 are the recalled arguments of upstream's HDBSCAN call; min_points = 4
 * and min_dynamic_frac = 0.3 are this project's own choices.  All four are arguments.
 * The stages run in this order on one stream and share ws (df_dbscan_ws_bytes(B, N)), after df_nn_grid_build has filed the participating
 * rows (ref = points, rcount = count, rlabel = mask) under a grid with cell >= eps.  Every stage scans the cells that a row's clamped
 * position, in cell units as df_nn_grid_build computes it, +- (eps / cell + 2e-3) covers in x and in y (the 2e-3 cell is df_chamfer_nn's
 * slack for the fp32 rounding of the cell coordinates) -- three cell rows, four for a row within the slack of a cell edge: they hold
 * its whole neighbourhood, rows outside the range included (clamping to the border cells is a contraction per coordinate).  NOT "the
 * 3 x 3 cells around the row's own": at cell == eps, fp32 files two rows a hair less than one cell apart (or exactly one cell apart)
 * two cells apart where the cell coordinate crosses a power of two.  A row farther than eps adds nothing, so the scanned cells never
 * show in the result: any cell >= eps gives the same labels.
 * df_dbscan_core: the core flags.   df_dbscan_link: union-find over the core rows (integer compare-and-swap / min; a root is always the
 *   lowest row of its tree, so the forest's roots do not depend on the launch order).   df_dbscan_finish: border rows, member counts
 *   (integer atomic adds), filters, numbering: labels [B,N] i32 and n_clusters [B] i32, both written completely.
 * status (nullable, i32[1]): every loop of the kernels is bounded (by N or 2 N); a loop that reaches its bound adds 1 here and the
 *   kernel carries on.  It stays 0 on every input the bounds were derived for; the host never waits on it.
 * No float atomics; repeated calls are bit-identical.  Limits as for the chamfer entries (B * N, B * G * G < 2^30, G <= 4096,
 * B <= 65535): violations return DF_E_SHAPE; cell < eps, eps <= 0, min_points < 1, min_cluster_size < 1 return DF_E_ARG.  No launch then. */
int64_t df_dbscan_ws_bytes(int B, int N);
int df_dbscan_core(const int32_t* cell_rng, const float* sorted, int B, int N, float minx, float miny, float cell, int G, float eps,
                   int min_points, void* ws, void* stream);
int df_dbscan_link(const int32_t* cell_rng, int B, int N, float minx, float miny, float cell, int G, float eps,
                   int32_t* status /*nullable*/, void* ws, void* stream);
int df_dbscan_finish(const int32_t* cell_rng, const int32_t* dynamic /*nullable*/, int B, int N, float minx, float miny, float cell, int G,
                     float eps, int min_cluster_size, double min_dynamic_frac, int32_t* labels, int32_t* n_clusters,
                     int32_t* status /*nullable*/, void* ws, void* stream);

/* ------------------------------------------------------------------ void map: ray-cast dynamic flags (SeFlow mode) ----
 * The per-point dynamic flag the online cluster labels start from, computed on the GPU.  UNPINNED: upstream writes `dufo_label` offline
 * on the CPU with DUFOMap (process.py; Duberg et al., RA-L 2024; absent submodule).  This is a DUFOMap-style void map with every choice
 * fixed, so that the map and the flags are a pure integer function of the input; parity with upstream's flags is not claimed.  Space that
 * some sweep has seen through is void; a return that lies in void space is dynamic.
 *   grid            gmin (three fp32), voxel size `voxel`, dims (Gx, Gy, Gz) with Gx % 32 == 0 and Gx * Gy * Gz < 2^31; SUB = 256 sub-voxel
 *                   units per voxel; k = fp32(256 / voxel) is computed on the host and passed as a float
 *   quantisation    the only floating-point step: for a coordinate p, u = fp32(fp32(p - gmin) * k), two separately rounded fp32
 *                   operations, and q = floor(u); the voxel of q is q >> 8 (arithmetic shift: floor).  A row takes part when
 *                   i < count[b], its three coordinates are finite and |u| < 2^30 on every axis.  If a sample's origin fails that rule,
 *                   none of its rays is cast (its rows still mark O)
 *   ray walk        from A (the origin) to E (a participating row), in 64-bit integers.  d = E - A, m = max_k |d_k|.  With
 *                   R = round(max_range / voxel * 256) a ray is truncated when m > R: E <- A + floor_div(d * R, m) per axis and d is
 *                   recomputed (a Chebyshev range cut).  c = A >> 8, e = E >> 8; per axis step_k = sign(d_k), den_k = |d_k|,
 *                   rem_k = |e_k - c_k|, num_k = ((c_k + 1) << 8) - A_k if d_k > 0, else A_k - (c_k << 8).  Visit c; then sum(rem)
 *                   times: among the axes with rem_k > 0 take the one with the smallest num_k / den_k (compared by cross-multiplication;
 *                   on equality the lower axis wins, x before y before z), c_k += step_k, num_k += 256, rem_k -= 1, visit c.  A
 *                   6-connected walk that ends in e.  The loop is bounded by 3 * (R / 256 + 1) steps; a ray that would exceed the bound
 *                   adds 1 to status and stops there (never, for 1 <= R <= 2^24, which the entry requires)
 *   free bits F     a visited voxel inside the grid is set when the ray is truncated, or when its Chebyshev voxel distance to e exceeds
 *                   hit_margin; e is the voxel of the ray's end after any truncation
 *   occupied bits O the voxel of every participating row's ORIGINAL endpoint, when inside the grid, truncated or not
 *   void map V      V |= erode(F & ~O, r): the AND over the (2r+1)^3 Chebyshev neighbourhood, r in {0, 1, 2}; voxels outside the grid
 *                   count as not free.  V persists over any number of sweeps until the caller clears it
 *   flag            1 when the row takes part, its voxel is inside the grid and its bit of V is set; every other row 0
 *   bit layout      u32 words, x fastest: bit = (z * Gy + y) * Gx + x, word bit >> 5, bit bit & 31; F, O, V are [B, Gx*Gy*Gz/32]
 * df_void_cast: points [B,N,3] f32, count [B] i32, origin [B,3] f32 -> F and O of this sweep.  The entry ZEROES F and O itself (an async
 *   memset on the stream) before the rays are cast: the caller only provides the storage.  Bits are set with 32-bit integer atomic OR
 *   after a plain test of the word; the result does not depend on the launch order.  status (nullable, i32[1]) as for DBSCAN.
 * df_void_cast_probe: the same cast for measuring (tools/voidmap_bench.py): attempts (nullable, u64[1]) is increased by the number of
 *   free-bit sets the rays asked for; always_atomic != 0 drops the test before the atomic.  The bits it leaves are df_void_cast's.
 * df_void_merge: V |= erode(F & ~O, erode).   df_void_query: flags [B,N] i32, written completely.
 * B * N < 2^30, B <= 65535, the grid limits above: violations return DF_E_SHAPE; a non-finite gmin, k <= 0, hit_margin < 0, R outside
 * [1, 2^24], erode outside {0, 1, 2} and NULL buffers return DF_E_ARG.  No launch then. */
int df_void_cast(const float* points, const int32_t* count, const float* origin, int B, int N, float gminx, float gminy, float gminz,
                 float k, int Gx, int Gy, int Gz, int hit_margin, int R, uint32_t* F, uint32_t* O, int32_t* status /*nullable*/,
                 void* stream);
int df_void_cast_probe(const float* points, const int32_t* count, const float* origin, int B, int N, float gminx, float gminy,
                       float gminz, float k, int Gx, int Gy, int Gz, int hit_margin, int R, uint32_t* F, uint32_t* O,
                       int32_t* status /*nullable*/, uint64_t* attempts /*nullable*/, int always_atomic, void* stream);
int df_void_merge(const uint32_t* F, const uint32_t* O, uint32_t* V, int B, int Gx, int Gy, int Gz, int erode, void* stream);
int df_void_query(const float* points, const int32_t* count, int B, int N, float gminx, float gminy, float gminz, float k, int Gx, int Gy,
                  int Gz, const uint32_t* V, int32_t* flags, void* stream);

/* ------------------------------------------------------------------ ground segmentation: the per-point ground mask of a raw sweep ----
 * The `ground_mask` the reader needs and collate_fn_pad drops, computed on the GPU.  UNPINNED: upstream writes it offline on the CPU with
 * a line-fit ground segmenter (absent submodule).  This is a height-map segmenter with every choice fixed, so that the maps and the mask
 * are a pure integer function of the input; parity with upstream's masks is not claimed.
 *   grid            (xmin, ymin) fp32, cell size `cell`, dims (Gx, Gy); heights in H levels of z_unit from z_min.  kxy = fp32(1 / cell) and
 *                   kz = fp32(1 / z_unit) are computed on the host and passed as floats
 *   quantisation    the only floating-point step: ux = fp32(fp32(x - xmin) * kxy), uy likewise, uz = fp32(fp32(z - z_min) * kz): two
 *                   separately rounded fp32 operations each; cx = floor(ux), cy = floor(uy), h = floor(uz)
 *   participating   i < count[b], three finite coordinates, 0 <= ux < Gx, 0 <= uy < Gy, 0 <= uz < H (compared on the floats, before the
 *                   floor).  Every other row gets mask 0
 *   cell minima     zmin[b][cy][cx] = the minimum h over the cell's participating rows; EMPTY = 2^31 - 1 when it has none
 *   height map      from the origin cell (ox, oy) (the caller quantises the origin the same way and clamps each index into the grid)
 *                   and seed = floor(fp32(fp32(seed_z - z_min) * kz)).  A cell with offset (dx, dy) from the origin cell and
 *                   r = max(|dx|, |dy|) has the ancestors a_k = (ox + clamp(dx, -k, k), oy + clamp(dy, -k, k)), k = 0 .. r (a_r is the
 *                   cell itself).  Start with g = seed, miss = miss_cap; at step k, z = zmin[a_k], w = WIDEN * min(miss, miss_cap); a_k
 *                   is accepted when z != EMPTY and g - DROP - w <= z <= g + RISE + w: then g = z, miss = 0; otherwise
 *                   miss = min(miss + 1, miss_cap).  height = g after step r; observed = 1 when step r accepted, else 0
 *   mask            a participating row is ground when h <= height[cell] + TOL
 * df_ground_cells: points [B,N,3] f32, count [B] i32 -> zmin i32[B,Gy,Gx].  The entry fills zmin with EMPTY itself (an async 32-bit memset
 *   on the stream): the caller only provides the storage.  32-bit integer atomic min after a plain test of the cell.
 * df_ground_height: zmin -> height i32[B,Gy,Gx], observed u8[B,Gy,Gx], both written completely.
 * df_ground_mask: -> mask u8[B,N], written completely.
 * 1 <= Gx, Gy <= 4096, 1 <= B <= 65535, N >= 1, B * N < 2^30: violations return DF_E_SHAPE.  H outside [1, 2^20], a non-finite xmin /
 * ymin / z_min, kxy or kz not positive and finite, (ox, oy) outside the grid, a negative threshold, miss_cap outside [0, 64] and NULL
 * buffers return DF_E_ARG.  No launch then.  The entries never allocate or synchronise. */
int df_ground_cells(const float* points, const int32_t* count, int B, int N, float xmin, float ymin, float kxy, float z_min, float kz,
                    int Gx, int Gy, int H, int32_t* zmin, void* stream);
int df_ground_height(const int32_t* zmin, int B, int Gx, int Gy, int ox, int oy, int seed, int rise, int drop, int widen, int miss_cap,
                     int32_t* height, uint8_t* observed, void* stream);
int df_ground_mask(const float* points, const int32_t* count, int B, int N, float xmin, float ymin, float kxy, float z_min, float kz,
                   int Gx, int Gy, int H, const int32_t* height, int tol, uint8_t* mask, void* stream);

/* ------------------------------------------------------------------ validation metrics, accumulated on the device ----
 * The tables of deflow_amd/metrics.py OfficialMetrics (leaderboard versions 1 and 2) and the range-free summary of evaluate_batch, fed a
 * whole padded batch per call (what DeFlow.forward_padded leaves on the device) and read back only when the caller reads the state.
 * Inputs: flow [B,N,3] f32 (compact rows i < counts[b]); idx_c [B,N] i64 (compact row -> row of the padded batch); pose_flow, pc0 (the
 * untransformed cloud), gt_flow [B,N,3] f32 and the optional u8 is_valid, eval_mask, cats [B,N], all read at j = idx_c[b,i]; counts [B] i32
 * (clamped to [0, N]).  A j outside [0, N) drops the row and adds 1 to the optional status word.
 *   row arithmetic   est = fp32(pose_flow + flow) per component; from there double, every operation rounded on its own:
 *                    norm(v) = sqrt((x x + y y) + z z); err = norm(est - gt); speed = norm(gt - pose_flow); est_speed = norm(est - pose_flow);
 *                    rel = err / (norm(gt) + 1e-10); strict / relaxed accuracy = err < t or rel < t, t = 0.05 / 0.10; dynamic = speed >= 0.05;
 *                    ok = is_valid and eval_mask (each 1 when absent); cat = min(cats, 30) (0 when absent); finite = the twelve values
 *   version 1        sel = finite, ok, |pc0.x| <= 35, |pc0.y| <= 35; foreground = cat != 0.  Per frame: the mean err of foreground-dynamic,
 *                    foreground-static and background-static rows, tp / (tp + fp + fn) of the dynamic flags (est_speed >= 0.05 against
 *                    dynamic), the means of err, both accuracies and the space-time angle arccos(clamp((est.gt + 0.01) /
 *                    (sqrt(est.est + 0.01) sqrt(gt.gt + 0.01)))) over sel; each value that exists is added to v1_sum, its v1_cnt raised by 1
 *   version 2        finite, ok, sqrt(x x + y y) <= 35 and an evaluated category: cell = meta-class x 51 + (number of edges <= speed), the 50
 *                    edges a host-computed double[50] (k * 2.0 / 50, k = 1 .. 50); err_sum, speed_sum and count per cell
 *   summary          over ok rows with finite est and gt, per sample: mean err, both accuracies, n, the mean err of the three classes
 *                    (foreground = cats != 0, every row when cats is absent) and the mean of those that exist; per call, each key's mean
 *                    over the samples that have it, then tot[key] += mean * B, wsum[key] += B
 *   skip rule        with has_eval_mask [B] u8: a sample without one is left out of everything iff some sample of the call has one
 * df_metrics_rows: rows -> per-block partials in ws (df_metrics_rows_per_block() rows per block; fixed reduction order, no float atomics).
 * df_metrics_accumulate: partials -> per-frame sums (ascending block order) -> the running state (ascending sample order):
 *   state_f double[526] = v1_sum[8] (EPE_FD EPE_FS EPE_BS IoU EPE AccS AccR Angle), err_sum[5][51], speed_sum[5][51], tot[8]
 *   state_i int64[272]  = v1_cnt[8], n, count[5][51], wsum[8]            (summary keys: EPE AccS AccR n EPE_FD EPE_FS EPE_BS EPE_3way)
 * ws: df_metrics_ws_bytes(B, N) bytes, 8-byte aligned (DF_E_ALIGN).  1 <= B <= 65535, N >= 1, B * N < 2^31: violations return DF_E_SHAPE;
 * NULL required buffers return DF_E_ARG.  No launch then.  The entries never allocate or synchronise; two runs are bit-identical. */
int df_metrics_rows_per_block(void);
int64_t df_metrics_ws_bytes(int B, int N);
int df_metrics_rows(const float* flow, const float* pose_flow, const float* pc0, const float* gt_flow, const int64_t* idx_c,
                    const int32_t* counts, const uint8_t* is_valid /*nullable*/, const uint8_t* eval_mask /*nullable*/,
                    const uint8_t* cats /*nullable*/, int B, int N, const double* edges, void* ws, int32_t* status /*nullable*/, void* stream);
int df_metrics_accumulate(const int32_t* counts, const uint8_t* has_eval_mask /*nullable*/, int B, int N, void* ws, double* state_f,
                          int64_t* state_i, void* stream);

/* ------------------------------------------------------------------ whole-sweep flow: what the save command writes per raw row ----
 * UNPINNED: the reference's save.py writes the estimated flow of every sweep into the dataset under the checkpoint's name; its source is
 * absent, so this definition is the project's own.  For sweep k of a scene (rows p_r of `lidar`, N_raw of them), its
 * successor and T = ego_motion or inv(pose1) pose0 exactly as DeFlow.forward_padded forms it:
 *   pose flow       of a raw row: what df_ego_transform computes for it -- per component i, a = fp32(x T[i][0]); a = fp32(a + fp32(y T[i][1]));
 *                   a = fp32(a + fp32(z T[i][2])); a = fp32(a + T[i][3]); pose_flow = fp32(a - p[i]): one rounding per operation
 *   decoded row     not ground, three finite coordinates, inside the model's range: the rows behind idx_c0[b, i], i < counts0[b].
 *                   flow_est = fp32(pose_flow + flow) per component; dynamic = (fp32(fp32(fp32(fx fx) + fp32(fy fy)) + fp32(fz fz)) >=
 *                   0.0025f) on the model's flow alone -- the 0.05 m per frame of the version-1 metrics, compared as squares
 *   other finite    rows (ground, out of range): flow_est = pose_flow, dynamic = 0
 *   non-finite      rows and padded rows r >= count_raw[b]: flow_est = (0, 0, 0), dynamic = 0
 *   half            flow_est rounded to fp16, round to nearest even
 * df_sweep_compact: raw [B,N,3] f32, count_raw [B] i32 (clamped to [0, N]), drop [B,N] u8 (non-zero = ground) -> pc [B,N,3]: the kept rows
 *   (r < count_raw[b], drop == 0) first, in their order and bit for bit, every further row three fp32 NaNs of pattern 0x7FC00000 (what
 *   collate_fn_pad pads with); row_of [B,N] i32: the raw row of each kept row, -1 in the padding; pos_of [B,N] i32: the compact position of
 *   each raw row, -1 for dropped and padded rows; kept [B] i32.  df_sweep_rows_per_block() raw rows per block; ws: df_sweep_compact_ws_bytes
 *   (B, N) bytes.  Every output element is written exactly once.
 * df_flow_compose: raw, count_raw, T [B,4,4] f32, pos_of as above; flow [B,Nc,3] f32, idx_c [B,Nc] i64 (compact position of decoded row i,
 *   no duplicates among the first counts[b]; an entry outside [0, N) is ignored), counts [B] i32 (clamped to [0, Nc]) -> flow_est [B,N,3]
 *   f32 (half = 0) or f16 (half = 1), dynamic [B,N] u8.  ws: df_flow_compose_ws_bytes(B, N) bytes.  Every output element is written exactly
 *   once.
 * ws 4-byte aligned (DF_E_ALIGN).  1 <= B <= 65535, N >= 1 (and Nc >= 1), B * N < 2^31: violations return DF_E_SHAPE (the _ws_bytes
 * functions return it too); NULL buffers and half outside {0, 1} return DF_E_ARG.  No launch then.  The entries never allocate or
 * synchronise and read nothing back; two runs are bit-identical. */
int df_sweep_rows_per_block(void);
int64_t df_sweep_compact_ws_bytes(int B, int N);
int df_sweep_compact(const float* raw, const int32_t* count_raw, const uint8_t* drop, int B, int N, void* ws, float* pc, int32_t* row_of,
                     int32_t* pos_of, int32_t* kept, void* stream);
int64_t df_flow_compose_ws_bytes(int B, int N);
int df_flow_compose(const float* raw, const int32_t* count_raw, const float* T, const int32_t* pos_of, const float* flow,
                    const int64_t* idx_c, const int32_t* counts, int B, int N, int Nc, int half, void* ws, void* flow_est,
                    uint8_t* dynamic, void* stream);

/* ------------------------------------------------------------------ leaderboard submission: the body of one feather file per sweep ----
 * UNPINNED: column names, order and types of the Argoverse-2 scene-flow submission are recalled, and no file written
 * here was ever accepted by the evaluation server.  The benchmark's rows of a sweep are the rows with eval_mask != 0, in raw order:
 * df_sweep_compact with drop = (eval_mask == 0) gives row_of [B,N] and kept [B]; M = kept[b] clamped to [0, N] below.
 * df_submit_pack: flow_est [B,N,3] f32 and dynamic [B,N] u8 (df_flow_compose with half = 0), row_of, kept, version in {1, 2} ->
 *   body [B,S] u8, S = df_submit_body_stride(N): the body of an uncompressed Arrow record batch of M rows and four columns, every buffer
 *   padded with zeros to 8 bytes.  P = pad8(2 M), Q = pad8(ceil(M / 8)), L(M) = 3 P + Q.
 *     version 1: flow_tx_m at 0, flow_ty_m at P, flow_tz_m at 2 P (M fp16 values each), the is_dynamic bits at 3 P
 *     version 2: the is_valid bits at 0 (set for every p < M), the three fp16 columns at Q, Q + P, Q + 2 P
 *   fp16 values: the fp32 component of row row_of[b, p] rounded to nearest even (numpy's astype(float16), overflow to inf included); bit p of
 *   a flag column is bit p & 7 of byte p >> 3 (Arrow's boolean layout); is_dynamic of p is dynamic[row_of[b, p]] != 0.  A row_of entry
 *   outside [0, N) among the first M (df_sweep_compact writes none) packs as a zero row.  Bytes [0, L(M)) of a sample are each written
 *   exactly once; bytes from L(M) on are not touched.
 * df_submit_body_stride(N): L(N) rounded up to 64 (DF_E_SHAPE for N < 1).  No workspace.
 * body 8-byte aligned (DF_E_ALIGN).  1 <= B <= 65535, N >= 1, B * S < 2^31: violations return DF_E_SHAPE; NULL buffers and a version outside
 * {1, 2} return DF_E_ARG.  No launch then.  The grid comes from N, never from a device value; the entry never allocates or synchronises
 * and reads nothing back; no atomics, two runs are bit-identical. */
int64_t df_submit_body_stride(int N);
int df_submit_pack(const float* flow_est, const uint8_t* dynamic, const int32_t* row_of, const int32_t* kept, int B, int N, int version,
                   uint8_t* body, void* stream);

/* ------------------------------------------------------------------ training augmentation of a padded batch ----
 * UNPINNED: upstream's later releases ship RandomFlip / RandomHeight / RandomJitter dataset transforms; the names are recalled, their
 * magnitudes, probabilities and distributions are not (hence arguments), and the jitter bell and the random stream are this project's own
 * (DESIGN.md section 6h).  Everything is a pure function of (seed, epoch, sample id, row): it does not depend on the batch a sample lands in,
 * on its position there, on the world size or on the reader; nothing is read back.
 *   words       Philox4x32-10, standard constants; key (seed & 0xffffffff, epoch & 0xffffffff); counter (id_lo, id_hi, row, purpose), id the
 *               sample's int64 id as two u32.  u(w) = (w >> 8) 2^-24.
 *   per sample  row = 0xffffffff, purpose = 0, words w0..w3: sx = u(w0) < flip_x_p ? -1 : 1; sy = u(w1) < flip_y_p ? -1 : 1;
 *               theta = (2 u(w2) - 1) yaw_max, the product in double (radians); dz = fp32((2 u(w3) - 1) height_max).
 *               c, s = the fp32 roundings of cos / sin of theta evaluated in double.  A: p' = L p + a, L = Rz(theta) diag(sx, sy, 1),
 *               a = (0, 0, dz).
 *   per row     purpose = 1 (pc0 rows) or 2 (pc1 rows), words w0..w3: the jitter of axis k is fp32(n_k sj), n_k = the sum of the four
 *               bytes of w_k minus 510 (an Irwin-Hall bell of unit standard deviation once divided by 147.8, at most 3.46 of them) and
 *               sj = fp32(jitter_sigma / 147.8) formed on the host in double; the row is dropped -- three fp32 NaNs of pattern
 *               0x7FC00000, in place, no compaction -- when u(w3) < drop_p.  Input NaN propagates.
 *   fp32 order  x1 = sx x, y1 = sy y; x2 = c x1 - s y1, y2 = s x1 + c y1 (each may be one FMA), z2 = z + dz; then + jitter (an FMA).
 *               yaw_max == 0: x2 = x1, y2 = y1; jitter_sigma == 0: nothing is added: flips and height are bit-exact.  The per-row
 *               words are drawn only when jitter_sigma > 0 or drop_p > 0.
 *   flow        [B,N0,3], nullable with flow_out: flow' = L flow, the linear part only.
 *   T, poses    [B,4,4] f32 each, nullable with their outputs: T' = A T A^-1, pose' = pose A^-1, composed in double with the double
 *               cos / sin and rounded to fp32 once; A^-1 has linear part diag(sx, sy, 1) Rz(-theta) and translation (0, 0, -dz).
 * df_augment: one launch for both clouds (separate padded lengths N0, N1), the flow and the matrices.  A cloud whose N % 4 == 0 and whose
 *   buffers are 16-byte aligned moves 16 bytes per access; any other takes 4-byte accesses.  The inputs are not modified (an output that
 *   is its input returns DF_E_ARG).
 * df_augment_params: params [B,8] f32 = (sx, sy, c, s, dz, theta, 0, 0) per sample, for logging and tests.
 * 1 <= B <= 65535, N0, N1 >= 1, B * N < 2^31: DF_E_SHAPE; NULL required buffers, an optional buffer without its output, a probability
 * outside [0, 1], a negative or non-finite magnitude: DF_E_ARG.  No launch then.  The entries never allocate or synchronise; no
 * atomics, two runs are bit-identical. */
int df_augment(const float* pc0, const float* pc1, const float* flow /*nullable*/, const int64_t* sample_ids, int B, int N0, int N1,
               int64_t seed, int64_t epoch, float flip_x_p, float flip_y_p, float yaw_max, float height_max, float jitter_sigma,
               float drop_p, const float* T /*nullable*/, const float* pose0 /*nullable*/, const float* pose1 /*nullable*/, float* pc0_out,
               float* pc1_out, float* flow_out, float* T_out, float* pose0_out, float* pose1_out, void* stream);
int df_augment_params(const int64_t* sample_ids, int B, int64_t seed, int64_t epoch, float flip_x_p, float flip_y_p, float yaw_max,
                      float height_max, float jitter_sigma, float drop_p, float* params, void* stream);

/* ------------------------------------------------------------------ bird's-eye-view flow images (the vis command) ----
 * UNPINNED: upstream's viewer (tools/visualization.py) is an interactive window whose source is absent; its colour wheel and camera cannot be
 * compared, so this definition is the project's own.  Every floating-point step below is ONE correctly rounded fp32
 * operation (written fp32(.)), never contracted, so that numpy float32 restates the image byte for byte.
 *   view          (xmin, ymin, inv_res), image W x H.  For a row (x, y, z): fx = floor(fp32(fp32(x - xmin) inv_res)), fy = floor(fp32(fp32(y -
 *                 ymin) inv_res)); the row is drawn when 0 <= fx < W and 0 <= fy < H (compared on the floats); px = fx, py = H - 1 - fy: x to
 *                 the right, y up, line 0 on top
 *   rows          i < count[b] (clamped to [0, N]).  A row is skipped when cls == 0 or when any of its six floats (point and vector) is not
 *                 finite.  cls == 1 draws the colour of its vector; every other non-zero cls (2 by convention: ground) draws grey (128, 128, 128)
 *   colour(vx, vy, vmax)   m = sqrt(fp32(fp32(vx vx) + fp32(vy vy))); s = min(fp32(m / vmax), 1); a = fp32(|vx| + |vy|).  The hue is the
 *                 diamond angle t in [0, 4]: a == 0: t = 0; else
 *                     vy >= 0 and vx >= 0: t = fp32(vy / a)                      vy >= 0 and vx < 0: t = fp32(1 + fp32(-vx / a))
 *                     vy <  0 and vx <  0: t = fp32(2 + fp32(-vy / a))           vy <  0 and vx >= 0: t = fp32(3 + fp32(vx / a))
 *                 (-0.0 >= 0 holds).  h6 = fp32(1.5 t); k = floor(h6), f = fp32(h6 - k), k == 6 counts as 0; p = fp32(1 - s),
 *                 q = fp32(1 - fp32(s f)), u = fp32(1 - fp32(s fp32(1 - f))); (R, G, B) for k = 0 .. 5: (1, u, p), (q, 1, p), (p, 1, u),
 *                 (p, q, 1), (u, p, 1), (1, p, q); each channel c becomes the byte floor(fp32(fp32(c 255) + 0.5)).  +x is red, +y yellow-green,
 *                 -x cyan, -y violet; the zero vector is white, |v| >= vmax fully saturated
 *   word          u64 = [cls == 1 : 1 bit][top 31 bits of key(z)][R G B : 24 bits][0xFF], key(z) = the order-preserving unsigned form of z's
 *                 bits (negative: all bits inverted; otherwise the sign bit set).  Never 0.  The row writes its word into the (2r+1)^2 square
 *                 of pixels around (px, py), clipped to the image, with a 64-bit integer atomic max: coloured rows win over grey ones, within
 *                 a class the highest row wins, equal heights (to 31 bits) are decided by the colour bits.  A maximum does not depend on the
 *                 order it is taken in: two calls are bit-identical
 * df_render_splat: points, vec [B,N,3] f32, cls [B,N] u8, count [B] i32 -> image u64 [B,H,W], which the CALLER zeroes beforehand (0 = empty).
 * df_render_resolve: image -> scanlines u8 [B, H, 1 + 3W]: per line a 0 byte (PNG filter type None), then R G B per pixel; an empty word gives
 *   bg_rgb (0xRRGGBB).  legend = L > 0 draws a colour-wheel disc over whatever lies under it: centre (cx, cy) = (W - 3 - L, L + 2), and a
 *   pixel with integers dx = x - cx, dy = y - cy, dx dx + dy dy <= L L gets colour(dx, -dy, L).  Every output byte is written exactly once.
 * 1 <= B <= 65535, N >= 1, B N < 2^31, 1 <= W, H <= 4096, B H (1 + 3W) < 2^31: violations return DF_E_SHAPE.  NULL buffers, a radius outside
 * [0, 4], vmax or inv_res not positive and finite, a non-finite xmin / ymin, bg_rgb outside [0, 0xFFFFFF], legend < 0 or 2 L + 5 > min(W, H)
 * return DF_E_ARG.  image 8-byte, scanlines 4-byte aligned (DF_E_ALIGN).  No launch then.  The grids come from N, W, H, never from a device
 * value; the entries never allocate or synchronise and read nothing back. */
int df_render_splat(const float* points, const float* vec, const uint8_t* cls, const int32_t* count, int B, int N, float xmin, float ymin,
                    float inv_res, int W, int H, float vmax, int radius, uint64_t* image, void* stream);
int df_render_resolve(const uint64_t* image, int B, int W, int H, int bg_rgb, int legend, uint8_t* scanlines, void* stream);

/* ------------------------------------------------------------------ rigid cluster flow (model=icpflow) ----
 * UNPINNED: the recipe follows ICP-Flow (Lin & Caesar, CVPR'24) -- ego-compensate, cluster both sweeps together, register each cluster
 * rigidly, read the flow off the transform -- but upstream's source is absent and every choice below is this project's own (DESIGN.md
 * section 6j).  Lengths in metres; fp32(.) is one correctly rounded operation.  Per sample: pc0s [N0,3] (first sweep, ground removed, moved
 * into the second sweep's frame by df_ego_transform), pc1 [N1,3], count0 / count1 valid leading rows.  N = N0 + N1.
 *   a. clusters  labels [B,N] i32 of the concatenation (pc0s rows, then pc1 rows): df_dbscan_* with eps = 0.7, min_points = 4,
 *                min_cluster_size = 20 over the valid finite rows (0 = none, 1..K).  Slot k = label - 1 < Kcap = max(N / min_cluster_size, 1).
 *                A slot's SOURCE rows are its rows < N0, its TARGET rows those >= N0, both in ascending row order.
 *   b. status    exactly one per slot, tested in this order: 0 no rows; 2 fewer than min_side (8) source or target rows; 3 more than
 *                max_cluster_points (8192) rows in all; 5 no vote in range (c); 4 / 5 / 1 from (e).
 *   c. vote      a side of n > vote_cap (1024) rows uses entries j * n / vote_cap (integer division, j = 0 .. vote_cap - 1) of its list,
 *                else all.  Every used pair (s, d): ix = floor(fp32(fp32(fp32(d.x - s.x) / vote_bin) + 0.5)), iy alike; R = ceil(max_disp /
 *                vote_bin) on the host (3.4 / 0.2: 17).  |ix| <= R and |iy| <= R adds one to an i32 counter.  Winner: most votes, on equal
 *                counts the lowest (iy + R) (2R + 1) + (ix + R).  t0 = (fp32(ix vote_bin), fp32(iy vote_bin), 0).
 *   d. icp       yaw + translation.  Coordinates relative to the anchor a = the slot's first source row: s' = fp32(s - a), d' = fp32(d - a).
 *                Sides over icp_cap (2048) rows are subsampled by the rule of (c).  theta = 0, t = t0; exactly icp_iters (8) iterations:
 *                p = Rz(theta) s' + t with c = cosf(theta), s = sinf(theta): p.x = fp32(fp32(fp32(c s'.x) - fp32(s s'.y)) + t.x),
 *                p.y = fp32(fp32(fp32(s s'.x) + fp32(c s'.y)) + t.y), p.z = fp32(s'.z + t.z); nearest used target row by
 *                d2 = fp32(fp32(fp32(dx dx) + fp32(dy dy)) + fp32(dz dz)), dx = fp32(p.x - d'.x) ..., the lowest position on equal d2;
 *                inlier when d2 <= fp32(icp_max_dist icp_max_dist) (0.5).  With n >= 3 inliers: ms = sum(s') / n, md = sum(d') / n,
 *                u = s' - ms, v = d' - md, theta = atan2f(sum(u.x v.y - u.y v.x), sum(u.x v.x + u.y v.y)), t = md - Rz(theta) ms
 *                (t.z = md.z - ms.z); with fewer the transform stays.  Sums run in a fixed order (a lane adds its rows in ascending order,
 *                then a fixed tree): two calls are bit-identical.  One more nearest-neighbour pass with the final transform:
 *                inlier_frac = fp32(inliers / used source rows).
 *   e. accept    status 4 unless inlier_frac >= min_inlier_frac (0.6); else status 5 unless |theta| <= max_yaw (0.35) and the centroid c of
 *                the used source rows moves by at most max_disp: |Rz(theta) c + t - c|^2 <= fp32(max_disp max_disp); else status 1.
 *   f. rows      a source row of a status-1 slot: flow = (fp32(p.x - s'.x), fp32(p.y - s'.y), t.z), p as in (d) with the final transform;
 *                rigid_id = its label.  Every other row of pc0s, padded and non-finite ones included: flow = (0, 0, 0), rigid_id = 0.
 * df_rigid_segments: labels -> seg_off [B, 2 Kcap + 1] i32 (list 2k: sources of slot k, 2k + 1: its targets; list l is seg_rows[b][seg_off[l]
 *   .. seg_off[l + 1])), seg_rows [B,N] i32 (rows of the concatenation, -1 behind the last list).  Integer counts, one scan, and a scatter
 *   in which one block per sample walks the rows in order: the lists are stable.  status i32[1] (zeroed by the caller) is added to for a
 *   label outside [0, Kcap] or a row that finds no place.  ws: df_rigid_segments_ws_bytes(B, N0, N1, Kcap) bytes.
 * df_rigid_vote: -> vote [B,Kcap,3] i32 (ix, iy, count; zeros for slots that are not registered); hist (nullable) [B,Kcap,2R+1,2R+1] i32,
 *   the whole histogram, [iy + R][ix + R].  0 <= R <= 64.
 * df_rigid_icp: -> table [B,Kcap,8] f32 = (theta, tx, ty, tz, inlier_frac, n_src, n_dst, status); the first five are 0 for status 0, 2, 3
 *   and for a slot without a vote.  ws: df_rigid_icp_ws_bytes(B, N0, N1) bytes.
 * df_rigid_apply: -> flow [B,N0,3] f32, rigid_id [B,N0] i32, every element written exactly once.
 * 1 <= B <= 65535, N0, N1 >= 1, B * N < 2^31, 1 <= Kcap <= N, R <= 64: violations return DF_E_SHAPE (the _ws_bytes functions return it
 * too); NULL buffers, min_side / max_cluster_points / caps < 1, icp_iters outside [0, 1024], a non-positive or non-finite vote_bin /
 * icp_max_dist, a negative or non-finite max_yaw / max_disp: DF_E_ARG.  ws 4-byte aligned (DF_E_ALIGN).  No launch then.  Grids come from
 * N and Kcap, never from a device value; no float atomics; the entries never allocate or synchronise and read nothing back. */
int64_t df_rigid_segments_ws_bytes(int B, int N0, int N1, int Kcap);
int df_rigid_segments(const int32_t* labels, int B, int N0, int N1, int Kcap, int32_t* seg_off, int32_t* seg_rows, int32_t* status, void* ws,
                      void* stream);
int df_rigid_vote(const float* pc0s, const float* pc1, const int32_t* seg_off, const int32_t* seg_rows, int B, int N0, int N1, int Kcap,
                  int min_side, int max_cluster_points, int vote_cap, float vote_bin, int R, int32_t* vote, int32_t* hist /*nullable*/,
                  void* stream);
int64_t df_rigid_icp_ws_bytes(int B, int N0, int N1);
int df_rigid_icp(const float* pc0s, const float* pc1, const int32_t* seg_off, const int32_t* seg_rows, const int32_t* vote, int B, int N0,
                 int N1, int Kcap, int min_side, int max_cluster_points, int icp_cap, int icp_iters, float vote_bin, float icp_max_dist,
                 float min_inlier_frac, float max_yaw, float max_disp, float* table, void* ws, void* stream);
int df_rigid_apply(const float* pc0s, const int32_t* count0, const int32_t* labels, const int32_t* seg_off, const int32_t* seg_rows,
                   const float* table, int B, int N0, int N1, int Kcap, float* flow, int32_t* rigid_id, void* stream);

/* ------------------------------------------------------------------ per-row coordinate MLP (model=nsfp) ----
 * The hot path of the per-pair neural flow prior.  UNPINNED: upstream's NSFP source is absent; the definition is
 * this project's own.  One net is a map R^3 -> R^3 in fp32, width H = 128 (compile time), `depth` hidden-to-hidden layers (0..15):
 *   a_0 = relu(W_in x + b_in);  a_l = relu(W_l a_{l-1} + b_l), l = 1..depth;  y = W_out a_depth + b_out;  relu'(z) = 1 for z > 0, else 0.
 * Its parameters are one flat fp32 vector of P = (128*3 + 128) + depth * (128*128 + 128) + (3*128 + 3) elements in the order
 * W_in[128][3], b_in[128], then per hidden layer W_l[out][in], b_l, then W_out[3][128], b_out[3].  Nets are batched: sample b of
 * x [B,N,3] uses params + b * param_stride (param_stride >= P, a multiple of 4, params 16-byte aligned), count [B] i32 valid leading rows.
 * Rows >= count[b] contribute nothing; y and dx are written as 0 there (their x and dy are never used: NaN padding is legal); count 0 is legal.
 * df_mlp_fwd: y [B,N,3]; acts (nullable: inference) [B, depth+1, N, 128] f32 = a_0 .. a_depth of every row < N, what df_mlp_bwd reads.
 * df_mlp_bwd: dy [B,N,3] = d loss / d y -> dparams [B] blocks at param_stride floats, EVERY element of a block written (P elements, and the padding up
 *   to the next multiple of 4 as 0; what lies between two blocks of a wider stride is not touched), not accumulated; dx (nullable) [B,N,3] = d loss / d x.  The ReLU masks are acts > 0.  ws: df_mlp_ws_bytes(B, N, depth) bytes, 16-byte
 *   aligned: the pre-activation gradients of every layer [B, depth+1, N, 128] and one partial parameter gradient per sample and split of
 *   1024 rows, which are added in ascending split order (rows inside a split in ascending order too): no float atomics, two calls are
 *   bit-identical, and a sample's dparams depend on neither B nor the other samples of the launch at equal N.
 * The 128 x 128 products (forward, data gradient, weight gradient) run on v_mfma_f32_16x16x4_f32: fp32 operands, fp32 accumulation.
 * 1 <= B <= 65535, N >= 1, 3 B N < 2^31, 0 <= depth <= 15, param_stride as above: else DF_E_SHAPE (df_mlp_ws_bytes returns it too); NULL
 * required pointers: DF_E_ARG; misaligned params / acts / ws: DF_E_ALIGN.  No launch then.  Grids come from B, N and depth only. */
int64_t df_mlp_ws_bytes(int B, int N, int depth);
int df_mlp_fwd(const float* x, const int32_t* count, const float* params, int64_t param_stride, int B, int N, int depth, float* y,
               float* acts /*nullable*/, void* stream);
int df_mlp_bwd(const float* x, const int32_t* count, const float* params, int64_t param_stride, const float* acts, const float* dy, int B,
               int N, int depth, float* dparams, float* dx /*nullable*/, void* ws, void* stream);

/* ------------------------------------------------------------------ distance transform (model=fastnsf) ----
 * The target side of the per-pair flow optimised on a distance transform.  UNPINNED: upstream's FastNSF source
 * is absent; the definition is this project's own.  A grid of GX x GY x GZ voxels of edge `cell` (fp32) starts at the origin (ox, oy, oz)
 * (fp32); R is the truncation radius in voxels, 1..255; every G >= 2 and GX * GY * GZ < 2^31 (offsets across the batch are 64-bit).
 * df_dt_build: ref [B,N,3] f32 with count [B] i32 valid leading rows (clamped to [0, N]; 0 is legal).  A row occupies voxel
 *   floor((p - o) / cell) per axis, in fp32 with an IEEE division; non-finite rows and rows outside the grid occupy nothing.
 *   dt2 [B,GZ,GY,GX] u16 = min(R*R, min over the sample's occupied voxels v' of |v - v'|^2) in integer voxel units: the exact squared
 *   Euclidean distance transform between voxel centres, truncated at R (R*R everywhere for a sample without an occupied voxel).  EVERY
 *   element of dt2 is written.  Clear, mark (plain stores of one constant), then three separable windowed min-plus passes
 *   min over |k| <= R of k*k + prev[. + k] along x, y, z, with partial sums saturated at R*R: integer arithmetic, no atomics, two calls
 *   are bit-identical and a sample's grid depends on neither B nor the other samples.  ws: df_dt_ws_bytes(B, GX, GY, GZ, R) bytes (one
 *   more copy of the grid), 16-byte aligned like dt2.
 * df_dt_lookup: query [B,N,3] f32, count as above -> d [B,N] f32, g [B,N,3] f32, and optionally (nullable) cells [B,N,3] i32 and
 *   clamped [B,N] u8.  Per axis a: u = (q - o) / cell - 0.5 (fp32), clamped to [0, G - 1]; i = min(floor(u), G - 2); t = u - i.
 *   d = the trilinear interpolant of cell * sqrt(dt2) over the corners i .. i + 1 at t (fp32), g = its analytic gradient d d / d q with
 *   component a = 0 where axis a was clamped; cells = (ix, iy, iz), clamped = bit a set where axis a was clamped.  A row >= count gets
 *   d = 0, g = 0, cells = 0, clamped = 0; a counted row with a non-finite coordinate d = R * cell, g = 0, cells = 0, clamped = 0: no
 *   index is formed from it.  All outputs are written for every row.
 * 1 <= B <= 65535, N >= 1, 3 B N < 2^31, the grid limits above: else DF_E_SHAPE (df_dt_ws_bytes returns it too).  NULL required
 * pointers, a cell that is not positive and finite, a NaN origin: DF_E_ARG.  dt2 / ws not 16-byte, the other buffers not 4-byte aligned:
 * DF_E_ALIGN.  No launch then.  Grids come from B, N and the grid extents only; the entries never allocate or synchronise. */
int64_t df_dt_ws_bytes(int B, int GX, int GY, int GZ, int R);
int df_dt_build(const float* ref, const int32_t* count, int B, int N, float ox, float oy, float oz, float cell, int GX, int GY, int GZ, int R,
                uint16_t* dt2, void* ws, void* stream);
int df_dt_lookup(const float* query, const int32_t* count, const uint16_t* dt2, int B, int N, float ox, float oy, float oz, float cell,
                 int GX, int GY, int GZ, int R, float* d, float* g, int32_t* cells /*nullable*/, uint8_t* clamped /*nullable*/, void* stream);

/* ------------------------------------------------------------------ per-cluster rigidity term (model=mbnsf) ----
 * The multi-body regulariser of the flow optimised on a distance transform.  UNPINNED: upstream's MBNSF source is
 * absent and was not read; the definition is this project's own.  x [B,N,3] f32 is the first sweep (non-participating rows as 0), count
 * [B] i32 its valid leading rows (clamped to [0, N]), labels [B,N] i32 its cluster labels (0: none; 1..Kcap), P = the pairs per row, 1..16.
 * Lists.  seg_off [B, 2 Kcap + 1] and seg_rows [B, N + 1] are df_rigid_segments' output for N0 = N, N1 = 1 on the labels followed by one
 *   column of zeros, the labels of rows >= count set to 0 first: list 2k = the rows of cluster k + 1 in ascending order, L[0 .. n-1].  A
 *   cluster is eligible with 2 <= n <= max_cluster_points.  Rows >= count, rows of label 0 or of a label outside 1..Kcap, rows of an
 *   ineligible cluster and rows their list does not hold have no partners.
 * Pairs.  The row at position i of an eligible list has the FORWARD partners L[(i + s_k) mod n], s_k = 1 + floor((k - 1)(n - 1) / P),
 *   k = 1..P (every s_k is in 1..n-1; repeats count as often as they occur), and the BACKWARD partners L[(i - s_k) mod n]: the rows
 *   whose k-th forward partner it is.  M_b = P x (rows of sample b with partners) is the number of pair instances.
 * df_iso_plan: -> nbr [B,N,2P] i32 (entries 0..P-1: the forward partners' rows for k = 1..P, entries P..2P-1: the backward ones; -1 in
 *   all of them for a row without partners), r0 [B,N,2P] f32 (the rest distance |x_a - x_b| of each entry, 0 at -1), pairs [B] i32 = M_b.
 *   Every element is written.  The integers are exact (pairs: one integer atomic add per block of 256 rows); two calls are bit-identical.
 * Distances.  |a - b| = sqrt(fp32(fp32(fp32(dx dx) + fp32(dy dy)) + fp32(dz dz))) with dx = fp32(a.x - b.x) ...: differences first, no
 *   fused multiply-add, so that an instance has the same r0, r1 and e from either of its ends.
 * df_iso_pairs: w [B,N,3] f32 (the warped rows x + F), nbr and r0 as above, delta > 0 -> v [B,N] f32, g [B,N,3] f32.  For an entry with
 *   partner q of row a: r1 = |w_a - w_q|, e = |r1 - r0|, rho(e) = e^2 for e <= delta and delta (2 e - delta) beyond (value and slope are
 *   continuous at delta).  v[a] = the sum of rho over the row's P FORWARD entries in entry order, so that sum_a v[a] counts every instance
 *   once; g[a] = the sum over all 2P entries in entry order of rho'(e) sign(r1 - r0) (w_a - w_q) / r1 (an entry with r1 == 0 adds its
 *   value and no gradient): d (sum of rho over the instances) / d w_a, not normalised.  An entry outside [0, N) is skipped like -1.  One
 *   thread per row; the row's table entries are read with 16-byte loads when P is even.  EVERY element of v and g is written (0 at a
 *   row without partners); no atomics; two calls are bit-identical; g of the two rows of a 2-row cluster are exact negatives.
 * P outside 1..16, B outside 1..65535, N < 1, B N 2P >= 2^31 (df_iso_plan: Kcap < 1 too): DF_E_SHAPE.  NULL pointers, max_cluster_points
 * < 1, a delta that is not positive and finite: DF_E_ARG.  nbr / r0 not 16-byte, the other buffers not 4-byte aligned: DF_E_ALIGN.  No
 * launch then.  Grids come from B and N only; the entries never allocate or synchronise and read nothing back. */
int df_iso_plan(const float* x, const int32_t* count, const int32_t* labels, const int32_t* seg_off, const int32_t* seg_rows, int B, int N,
                int Kcap, int P, int max_cluster_points, int32_t* nbr, float* r0, int32_t* pairs, void* stream);
int df_iso_pairs(const float* w, const int32_t* nbr, const float* r0, int B, int N, int P, float delta, float* v, float* g, void* stream);

/* ------------------------------------------------------------------ flow field on a voxel grid (model=floxels) ----
 * The field of the per-pair flow optimised without a net.  UNPINNED: upstream's Floxels source is absent and was
 * not read; the definition is this project's own.  x [B,N,3] f32 is the first sweep, count [B] i32 its valid leading rows (clamped to
 * [0, N]).  The grid has VX x VY x VZ nodes (each >= 2), node (i, j, k) at origin + voxel (i, j, k); NV = VX VY VZ nodes and
 * NC = (VX-1)(VY-1)(VZ-1) cells per sample.  theta [B,VZ,VY,VX,3] f32: one 3-vector per node, x fastest, the components innermost.
 * Rows.  A counted row with three finite coordinates takes part.  Per axis u = fp32((x - o) / voxel) (IEEE subtraction and division),
 *   clamped to [0, V - 1]; i = min(floor(u), V - 2), t = u - i in [0, 1] (exact); cell = (iz (VY-1) + iy)(VX-1) + ix.  Every other row
 *   has cell = -1 and t = 0, and no index is formed from it.
 * df_vox_plan (once per pair): -> cell [B,N] i32, frac [B,N,3] f32 (tx, ty, tz); the rows that take part grouped by (sample, cell) with
 *   df_cell_sort (key b NC + cell): idx_sorted [B N] i32 holds b N + row, the rows of one cell in ascending order, cell after cell and
 *   sample after sample, and -1 in the slots behind the last grouped row; cell_rng [B NC, 2] i32 = every cell's (first, end) slot,
 *   first == end for an empty cell; active [B,NV] u8 = 1 for the corners of every cell that holds a row (gathered per node from its at
 *   most 8 incident cells' ranges, no atomics), else 0; pairs [B] i32 = M_b, the axis-adjacent node pairs with both ends active (one
 *   integer atomic add per workgroup of 256 nodes after a memset).  Every element of every output is written; all of it is exact; two
 *   calls are bit-identical.  ws: df_vox_plan_ws_bytes(B, N, VX, VY, VZ) bytes, 16-byte aligned (-1 for a refused shape).  The sort's
 *   keys have 30 bits: df_vox_plan (only) also refuses B NC >= 2^30 - 1 with DF_E_SHAPE.
 * Weights.  Corner (a, d, e) of a row's cell has the weight fp32(fp32(wx wy) wz), wx = tx for a = 1 and 1 - tx for a = 0, wy and wz
 *   alike: the same bits in the read and in its transpose.
 * df_vox_sample: theta, cell, frac -> F [B,N,3] f32 = the sum over the 8 corners of weight x theta[node], corners in the order e, d, a
 *   (a fastest).  One thread per row; the two x-neighbours of a corner pair are 24 contiguous bytes.  Every element is written, 0 where
 *   cell is outside [0, NC).
 * df_vox_scatter: dF [B,N,3] f32 (rows that do not take part are never read: they may hold NaN), frac, idx_sorted, cell_rng -> dtheta
 *   [B,NV,3] f32, the exact transpose of the read in gather form: a node sums weight_corner(t_r) dF_r over its at most 8 incident cells
 *   in the order e, d, a (the node is corner (a, d, e) of the cell at (ix - a, iy - d, iz - e)) and over each cell's rows in ascending
 *   order.  One thread per node.  A cell of up to 128 rows is added row by row to the node's running sum, the cells in the order above.  A
 *   cell of more than 128 rows is summed by the node's whole wave after those: lane l adds the rows first + l, first + l + 64, ... in
 *   order, the 64 partial sums are added in a fixed xor butterfly (32, 16, ..., 1; fp32 additions), and that total is added to the node's
 *   sum, the long cells of a node in the order above.  Either way the result is a function of the cell's rows and their order alone: no
 *   float atomics; two calls are bit-identical; a sample's result depends neither on B nor on the other samples.  Every node is written,
 *   0 where nothing is incident.  Ranges are clipped to [0, B N] and entries outside the sample skipped.
 * df_vox_smooth: theta, active -> v [B,NV] f32, g [B,NV,3] f32.  For an active node n and an active axis neighbour q:
 *   d = fp32(theta_n - theta_q) per component, |d|^2 = fp32(fp32(fp32(dx dx) + fp32(dy dy)) + fp32(dz dz)).  v[n] = the sum of |d|^2 over
 *   the FORWARD neighbours x+1, y+1, z+1 in that order, so that sum_n v[n] counts every pair once; g[n] = the sum of 2 d over the
 *   neighbours x-1, x+1, y-1, y+1, z-1, z+1 in that order: d (sum of |d|^2 over the pairs) / d theta_n, not normalised.  No fused
 *   multiply-add.  A node on the grid's face has no neighbour beyond it.  No atomics; every element is written, 0 at an inactive node.
 * B outside 1..65535, N < 1, a V < 2, or 3 B N, 3 B NV or B NC >= 2^31: DF_E_SHAPE.  NULL pointers, a voxel that is not positive and
 * finite, a NaN origin: DF_E_ARG.  Buffers not 4-byte (ws: 16-byte) aligned: DF_E_ALIGN.  No launch then.  Grids come from B, N and the
 * grid's dimensions only; the entries never allocate or synchronise and read nothing back. */
int64_t df_vox_plan_ws_bytes(int B, int N, int VX, int VY, int VZ);
int df_vox_plan(const float* x, const int32_t* count, int B, int N, float ox, float oy, float oz, float voxel, int VX, int VY, int VZ,
                int32_t* cell, float* frac, int32_t* idx_sorted, int32_t* cell_rng, uint8_t* active, int32_t* pairs, void* ws, void* stream);
int df_vox_sample(const float* theta, const int32_t* cell, const float* frac, int B, int N, int VX, int VY, int VZ, float* F, void* stream);
int df_vox_scatter(const float* dF, const float* frac, const int32_t* idx_sorted, const int32_t* cell_rng, int B, int N, int VX, int VY,
                   int VZ, float* dtheta, void* stream);
int df_vox_smooth(const float* theta, const uint8_t* active, int B, int VX, int VY, int VZ, float* v, float* g, void* stream);

/* ------------------------------------------------------------------ per-cluster rigid snap of a model's flow (the refine command) ----
 * UNPINNED: the recipe follows the rigid refinement of Chodosh et al., "Re-evaluating LiDAR scene flow" (WACV'24) -- cluster the first
 * sweep, fit one robust rigid motion per cluster to the flow a model produced, give the rows of an accepted cluster that motion -- but no
 * upstream source was read and every choice below is this project's own.  Lengths in metres; fp32(.) is one
 * correctly rounded operation, no contraction.  Per sample: x [Nc,3] (the decoded rows of the ego-compensated first sweep, compacted),
 * f [Nc,3] (the model's residual flow of those rows), count their valid leading rows (clamped to [0, Nc]).
 *   a. clusters  labels [B,Nc] i32: df_dbscan_* with eps = 0.7, min_points = 4, min_cluster_size = 20 over x (0 = none, 1..K); the labels
 *                of rows >= count set to 0.  Slot k = label - 1 < Kcap = max(Nc / min_cluster_size, 1).  Lists: seg_off [B, 2 Kcap + 1] and
 *                seg_rows [B, Nc + 1] are df_rigid_segments' output for N0 = Nc, N1 = 1 on the labels followed by one column of zeros:
 *                list 2k = the rows of cluster k + 1 in ascending order.
 *   b. rows      a row of a list TAKES PART when it is < count and its x and f are finite.  Status, tested in this order: 0 no rows in the
 *                list; 3 more than max_cluster_points (8192) rows in the list (they are not read); 2 fewer than min_rows (8) rows take part.
 *   c. fit       yaw + translation, iteratively re-weighted least squares with Huber weights.  Anchor a = the list's first row that takes
 *                part; s = fp32(x - a), d = fp32(s + f).  w = 1 in the first fit; exactly iters (4) re-weightings, iters + 1 fits.  One fit:
 *                W = sum w, ms = sum(fp32(w s)) / W, md = sum(fp32(w d)) / W, u = fp32(s - ms), v = fp32(d - md),
 *                theta = atan2f(sum fp32(w fp32(fp32(u.x v.y) - fp32(u.y v.x))), sum fp32(w fp32(fp32(u.x v.x) + fp32(u.y v.y)))),
 *                t = md - Rz(theta) ms with c = cosf(theta), s = sinf(theta): t.x = fp32(md.x - fp32(fp32(c ms.x) - fp32(s ms.y))),
 *                t.y = fp32(md.y - fp32(fp32(s ms.x) + fp32(c ms.y))), t.z = fp32(md.z - ms.z).  Residual of a row under a fit:
 *                p.x = fp32(fp32(fp32(c s.x) - fp32(s s.y)) + t.x), p.y = fp32(fp32(fp32(s s.x) + fp32(c s.y)) + t.y), p.z = fp32(s.z + t.z),
 *                e = fp32(p - d), r2 = fp32(fp32(fp32(e.x e.x) + fp32(e.y e.y)) + fp32(e.z e.z)), r = sqrt(r2) correctly rounded.  The next
 *                fit's w = 1 for r <= delta (0.1), else fp32(delta / r) (0 when r is not finite).  After the last fit, from its residuals:
 *                inlier_frac = fp32(#(r <= inlier_dist (0.2)) / rows that take part), rms = sqrt(fp32(sum r2 / rows that take part)).
 *                Every sum runs in a fixed order: thread t of 256 adds the list positions t, t + 256, ... in ascending order, the 64 lanes
 *                of a wave are added in an xor butterfly (32, 16, ..., 1), then waves 0..3 in order.  Two calls are bit-identical, and a
 *                slot's result depends neither on B nor on the other samples or slots.
 *   d. accept    status 4 unless inlier_frac >= min_inlier_frac (0.5); else 5 unless |theta| <= max_yaw (0.35) and disp <= max_disp (3.4),
 *                disp = |Rz(theta) c + t - c| for the unweighted centroid c = sum(s) / rows of the rows that take part (z: t.z), products
 *                and sums rounded one by one, the root correctly rounded; else 6 (static) when disp <= static_disp (0.05) and |theta| <=
 *                static_yaw (0.02): theta and t are then written as 0, the identity; else 1.
 *   e. check     with f' the flow that (f) would write: d2_before / d2_after [B,Nc] = df_chamfer_nn's squared distances of x + f and
 *                x + f' to the second sweep, max_dist2 = check_trunc^2 (check_trunc 2.0).  Per slot of status 1 or 6, c_before / c_after =
 *                fp32(sum / rows) over the rows that take part of min(sqrt(d2), check_trunc), check_trunc for a row without a neighbour
 *                (inf, NaN, d2 > check_trunc^2), summed in the order of (c).  c_after > fp32(c_before + check_tol) (0.05) turns the status
 *                into 7 and the slot is left alone.  A sample with count1 <= 0 (no second sweep): every slot passes, c_before = c_after = 0.
 *   f. rows      a row that takes part in a status-1 slot: flow = (fp32(p.x - s.x), fp32(p.y - s.y), t.z), p as in (c); in a status-6 slot:
 *                flow = 0; rigid_id = its label for both.  EVERY other row -- label 0 or outside 1..Kcap, another status, rows that do not
 *                take part, rows >= count -- keeps f bit for bit (NaN payloads included) and gets rigid_id = 0.
 * df_refine_fit: -> table [B,Kcap,12] f32 = (theta, tx, ty, tz, inlier_frac, rms, rows used, status, c_before = 0, c_after = 0, 0, 0); the
 *   first six are 0 for status 0, 2, 3; rows used = the rows that take part (status 3: the list's length); anchor [B,Kcap] i32 = the
 *   anchor's row, -1 without one.  Every element of both is written.  One workgroup per (sample, slot), rows re-read from global memory in
 *   every pass, no workspace.
 * df_refine_score: d2_before, d2_after, count1 [B] i32 -> table columns 8, 9 and the status by (e); the other columns are not touched.
 * df_refine_apply: table, anchor -> flow_out [B,Nc,3] f32, rigid_id [B,Nc] i32, every element written exactly once.  It serves both the
 *   provisional f' of (e) and the final output.
 * B outside 1..65535, Nc < 1, B Nc >= 2^31: DF_E_SHAPE.  NULL pointers, Kcap outside [1, Nc], iters outside [0, 64], min_rows or
 * max_cluster_points < 1, a delta / inlier_dist / check_trunc that is not positive and finite, any other threshold negative or not finite:
 * DF_E_ARG.  Buffers not 4-byte aligned: DF_E_ALIGN.  No launch then.  Grids come from B, Nc and Kcap only, never from a device value; no
 * float atomics; the entries never allocate or synchronise and read nothing back. */
int df_refine_fit(const float* x, const float* flow, const int32_t* count, const int32_t* seg_off, const int32_t* seg_rows, int B, int Nc,
                  int Kcap, int min_rows, int max_cluster_points, int iters, float delta, float inlier_dist, float min_inlier_frac,
                  float max_yaw, float max_disp, float static_disp, float static_yaw, float* table, int32_t* anchor, void* stream);
int df_refine_score(const float* x, const float* flow, const int32_t* count, const int32_t* count1, const int32_t* seg_off,
                    const int32_t* seg_rows, const float* d2_before, const float* d2_after, int B, int Nc, int Kcap, float check_trunc,
                    float check_tol, float* table, void* stream);
int df_refine_apply(const float* x, const float* flow, const int32_t* count, const int32_t* labels, const float* table,
                    const int32_t* anchor, int B, int Nc, int Kcap, float* flow_out, int32_t* rigid_id, void* stream);

/* ------------------------------------------------------------------ sweep-to-sweep registration (odometry) ----
 * UNPINNED: this project's own definition, not that of an existing LiDAR odometry; nothing about its accuracy on
 * real sweeps has been measured.  A robust point-to-point ICP of whole clouds in 6 degrees of freedom that never returns to the host:
 * T [B,16] f64 (row-major 4 x 4) with dst ~ R src + t maps the source sweep into the target sweep's frame -- with source = sweep k and
 * target = sweep k + 1 it is the reference's pose_0to1 / ego_motion.  One iteration = df_reg_accumulate, then df_reg_solve.
 *   rows         BOTH clouds are filed by df_nn_grid_build, each under its own grid: a row takes part by that entry's rule (< count,
 *                finite, optional label > 0).  The source is filed so that its rows are walked in cell order and the lanes of a wave search
 *                neighbouring target spans; its grid's range and cell do not enter the result's definition beyond that order.
 *   subsample    stride in [1, 1024]: with [s, e) the span of sample b in the source's cell order (s = the start of its first cell, e =
 *                the end of its last), the record at position p is USED when (p - s) % stride == 0.
 *   row terms    R, t = T rounded to fp32.  q = R s + t in fp32: q.x = fma(R02, s.z, fma(R01, s.y, fma(R00, s.x, t.x))), y and z alike.
 *                (d2, j) = the nearest participating target row of q: df_chamfer_nn's distance expression, tie rule (lowest row on equal
 *                distances) and max_dist2 gate -- the same device function.  A used row with d2 <= max_dist2 is an INLIER with the
 *                Geman-McClure weight w = fp32(u u), u = fp32(k2 / fp32(k2 + d2)), k2 = kernel^2.  Residual r = fp32(q - dst[j]); the
 *                Jacobian of the left perturbation T <- exp(delta) T, delta = (omega, v): J = [ -[q]x , I ].
 *   sums         per inlier, each term formed in fp32 and accumulated in float64; partial[b][block][32] f64 =
 *                  0..20  the upper triangle of H = sum w J^T J, row by row (H00 .. H05, H11 .. H15, ..., H55)
 *                  21..26 g = sum w J^T r = (sum w q x r, sum w r);  27 sum w;  28 sum fp32(w d2);  29 the inliers;  30, 31: 0.
 *                Order: a lane holds its one row, the 64 lanes of a wave are added in an xor butterfly (32, 16, ..., 1), the block's 4
 *                waves in wave order, one slab row per block of 256 cell-ordered positions; df_reg_solve adds the slab rows in ascending
 *                block order.  No float atomics: two calls are bit-identical, and a sample's result depends neither on B nor on the other
 *                samples at equal Ns.
 *   solve        in float64.  planar != 0: rows and columns omega_x, omega_y of H are replaced by identity, their g entries by 0.
 *                status 2: fewer than min_inliers inliers; 3: a Cholesky pivot of a solved-for row <= 1e-9 x the largest diagonal entry
 *                of H (or not finite); T is untouched, bit for bit, in both.  Else 0: delta = -H^-1 g through the Cholesky factor and
 *                T <- exp(delta) T with the closed-form SE(3) exponential: theta = |omega|, R = I + A K + B K^2, t = (I + B K + C K^2) v,
 *                K = [omega]x, A = sin(theta) / theta, B = 2 sin^2(theta / 2) / theta^2, C = (theta - sin(theta)) / theta^3; for
 *                theta < 1e-2 the series of A, B, C up to theta^6.  log [B,4] f32 = (inliers, sum w d2 / sum w (0 when sum w = 0),
 *                |omega|, |v|), the last two 0 unless status 0.
 * df_reg_ws_bytes(B, Ns): the bytes of partial = 256 B ceil(Ns / 256); DF_E_SHAPE (negative) for shapes the entries refuse.
 * df_reg_accumulate: src_rng [B*Gs*Gs, 2] i32 and src_sorted [B*Ns, 4] f32: the source's grid; dst_rng [B*G*G, 2], dst_sorted [B*Nd, 4],
 *   minx, miny, cell, G: the target's.  -> partial, every one of its B ceil(Ns / 256) 32 elements written.  The optional per-row outputs are
 *   indexed by source ROW, not by cell position: q_out [B,Ns,3] f32, idx_out [B,Ns] i32, d2_out [B,Ns] f32, w_out [B,Ns] f32; a row that is
 *   not used gets q = 0, idx = -1, d2 = +inf, w = 0, a used row that is no inlier its q and idx = -1, d2 = +inf, w = 0; every element of a
 *   given output is written.  One thread per cell-ordered source position, 256 per block, grid (ceil(Ns / 256), B).
 * df_reg_solve: partial [B,nblk,32], nblk = ceil(Ns / 256) -> T in place, log [B,4], status [B] i32; one 64-thread block per sample.  T
 *   NULL: nothing is solved, log = (inliers, sum w d2 / sum w, 0, 0), status (then nullable) is not written.
 * B outside 1..65535, Ns < 1, B Ns >= 2^30, Gs or G outside 1..4096, B G^2 >= 2^30, nblk < 1: DF_E_SHAPE.  NULL pointers, stride outside
 * [1, 1024], a max_dist2 / k2 / cell that is not positive and finite, minx / miny not finite, min_inliers < 0: DF_E_ARG.  src_sorted /
 * dst_sorted not 16-byte, partial / T not 8-byte aligned: DF_E_ALIGN.  No launch then.  No grid dimension comes from a device value; the
 * entries never allocate or synchronise and read nothing back.
 *
 * POINT-TO-PLANE (UNPINNED like the rest).  A spinning sensor samples a wall or the ground at positions that move with it, so the nearest
 * target row of a source row is "the same sample", and the point-to-point fit above is pulled towards zero motion.  The plane residual lets
 * a row slide along the surface it lies on: one iteration = df_reg_accumulate_plane, then the SAME df_reg_solve; df_reg_ws_bytes and the
 * slab's layout serve both residuals unchanged.  The target's normals come from df_normals, once per target.
 *   normals      of a cloud filed by df_nn_grid_build (cell_rng, sorted), 0 < radius <= cell.  The NEIGHBOURS of a participating row p
 *                are the participating rows v of its sample, p itself included, with d2 <= fp32(radius radius), d2 = df_chamfer_nn's
 *                distance expression on the fp32 differences x = fp32(v - p).  ALL of them: the entry scans the cells that p's clamped
 *                position, in cell units as df_nn_grid_build computes it, +- (radius / cell + 2e-3) covers in x and in y (the 2e-3 cell
 *                is df_chamfer_nn's slack for the fp32 rounding of the cell coordinates; NOT "the 3 x 3 cells around p's own": at
 *                radius == cell, fp32 files two rows a hair less than one cell apart two cells apart where the cell coordinate
 *                crosses a power of two) -- one span of `sorted` per cell row, three or four of them, walked in ascending position;
 *                a row farther than radius adds nothing, so the scanned span never shows in the result.  m = their number.
 *                S1 = sum x [3] and S2 = sum x x^T [6] are accumulated in float64 in that order; in float64 mean = S1 / m,
 *                C = S2 / m - mean mean^T.
 *                Eigenvectors: cyclic Jacobi in float64, 8 sweeps of the rotations (0,1), (0,2), (1,2) (off-diagonal entries are at
 *                rounding level after 5; a rotation whose off-diagonal entry is exactly 0 is skipped, so rows that share one z get the
 *                axis (0, 0, +-1) exactly).  lambda0 <= lambda1 <= lambda2 (on equal smallest values the later axis), n = the unit
 *                eigenvector of lambda0 rounded to fp32, curv = fp32(max(lambda0 / (lambda0 + lambda1 + lambda2), 0)).  Sign: n . p <= 0
 *                (float64 products of the fp32 values added left to right), on n . p == 0 the first non-zero component is positive; a
 *                zero component is +0.  VALID: m >= min_pts, lambda0 + lambda1 + lambda2 > 0 and curv <= max_curv.
 *   plane terms  q, (d2, j) and the used rows exactly as above.  A used row is an INLIER when d2 <= max_dist2 AND the normal of target
 *                row j is valid (its w >= 0).  n = that normal, r = fp32(q - dst[j]), e = n . r in fp32, the Geman-McClure weight acts
 *                on the plane distance: w = fp32(u u), u = fp32(k2 / fp32(k2 + fp32(e e))) -- sliding along the surface is free, the
 *                Euclidean gate stays on d2.  The row of the normal equations is a = (q x n, n) in fp32.
 *   plane sums   per inlier, each formed in fp32 and accumulated in float64, in the order above; the slab's columns, unchanged:
 *                  0..20  the upper triangle of H = sum w a a^T: fp32(fp32(w a_i) a_j), i <= j, row by row
 *                  21..26 g = sum fp32(fp32(w a_i) e);  27 sum w;  28 sum fp32(fp32(w e) e);  29 the inliers;  30, 31: 0.
 *                Every factor that comes from n changes sign with n and no other does, and no fma joins a term that changes sign with
 *                one that does not: negating the fp32 normals negates a and e exactly and leaves the slab bit for bit.
 * df_normals: cell_rng [B*G*G, 2] i32, sorted [B*N, 4] f32 and minx, miny, cell, G as df_nn_grid_build wrote and took them -> normals
 *   [B,N,4] f32 indexed by ROW: (nx, ny, nz, curv) of a valid row, (0, 0, 0, -1) of every other row of [B,N] (padding, rows that do not
 *   take part, rows that are not valid); m_out [B,N] i32: m, 0 for a row that does not take part.  Every element of both is written (a fill
 *   launch on the same stream, then one thread per cell-ordered position, 256 per block, grid (ceil(N / 256), B)); no atomics.
 * df_reg_accumulate_plane: df_reg_accumulate's arguments and, after dst_sorted, dst_normals [B*Nd, 4] f32 = df_normals' output for the
 *   target, read at row j as one 16-byte load, and Nd after Ns (dst_sorted is [B*Nd, 4]).  -> partial as above.  The optional per-row
 *   outputs as above, and e_out [B,Ns] f32; a row that is not used gets e = 0, and a used row that is gated out OR whose partner has no
 *   valid normal gets its q and idx = -1, d2 = +inf, w = 0, e = 0.
 * B outside 1..65535, N / Ns / Nd < 1, B N (B Ns, B Nd) >= 2^30, G / Gs outside 1..4096, B G^2 >= 2^30: DF_E_SHAPE.  NULL pointers (the
 * nullable ones excepted), radius outside (0, cell], min_pts < 3, max_curv outside (0, 1/3], and df_reg_accumulate's other refusals:
 * DF_E_ARG.  sorted / normals / dst_normals not 16-byte, m_out not 4-byte aligned: DF_E_ALIGN.  No launch then. */
int64_t df_reg_ws_bytes(int B, int Ns);
int df_reg_accumulate(const int32_t* src_rng, const float* src_sorted, int Gs, const int32_t* dst_rng, const float* dst_sorted, float minx,
                      float miny, float cell, int G, int B, int Ns, int stride, const double* T, float max_dist2, float k2, double* partial,
                      float* q_out /*nullable*/, int32_t* idx_out /*nullable*/, float* d2_out /*nullable*/, float* w_out /*nullable*/,
                      void* stream);
int df_reg_solve(const double* partial, int B, int nblk, int min_inliers, int planar, double* T /*nullable*/, float* log,
                 int32_t* status /*nullable*/, void* stream);
int df_normals(const int32_t* cell_rng, const float* sorted, float minx, float miny, float cell, int G, int B, int N, float radius,
               int min_pts, float max_curv, float* normals, int32_t* m_out /*nullable*/, void* stream);
int df_reg_accumulate_plane(const int32_t* src_rng, const float* src_sorted, int Gs, const int32_t* dst_rng, const float* dst_sorted,
                            const float* dst_normals, float minx, float miny, float cell, int G, int B, int Ns, int Nd, int stride,
                            const double* T, float max_dist2, float k2, double* partial, float* q_out /*nullable*/,
                            int32_t* idx_out /*nullable*/, float* d2_out /*nullable*/, float* w_out /*nullable*/,
                            float* e_out /*nullable*/, void* stream);

/* ------------------------------------------------------------------ local map (scan-to-map odometry) ----
 * UNPINNED: this project's own definition.  The target of a scan-to-map registration: world-frame points (the
 * world is the first sweep's frame), at most max_per_voxel = K of them per cubic voxel of edge `voxel`, inside a window of S x S voxel
 * columns, S = 2 W + 1, about the sensor.  State per sample: map [B,cap,3] f64 and count [B] i32, the number of leading rows that hold
 * points.  pose [B,16] f64, row-major 4 x 4 on the device: world = R s + t.  One update = df_map_keys, df_cell_sort with
 * ncells = B S S, df_map_select, df_map_compact; df_map_view makes the dst of df_reg_accumulate's grid.
 * ARITHMETIC: every float64 operation named below is rounded once, on its own (no fma), so numpy float64 reproduces it bit for bit.
 *   candidates   n = cap + N rows per sample: the map's rows 0 .. cap-1 first, then the sweep's rows.  A map row TAKES PART when its
 *                index < count[b]; a sweep row r when r < sweep_count[b], its three coordinates are finite, mask[b,r] > 0 (mask
 *                nullable) and gate is NULL or gate[b] == 0 (gate: the status of the registration that made the pose, so a failed
 *                registration inserts nothing, with nothing read back).
 *   world        of a sweep row (x, y, z): a = R_i0 x; a = a + R_i1 y; a = a + R_i2 z; w_i = a + t_i.  A map row is copied.
 *   voxel        v_i = floor(w_i / voxel).  A row with a w_i that is not finite or a |v_i| >= 2^30 on any axis does not take part (no
 *                float-to-integer conversion is made before that check).  Anchor: a_x = floor(t_x / voxel), a_y likewise, under the
 *                same rule; with an anchor out of range no row of the sample takes part, map rows included.
 *   key          dx = v_x - a_x + W, dy = v_y - a_y + W; with 0 <= dx, dy <= 2 W the key is (b S + dy) S + dx, else -- and for every
 *                row that does not take part -- B S S, which df_cell_sort drops: the window cull.  A row with the drop key has
 *                cand = three float64 NaNs (0x7FF8000000000000) and vz = 0; every other row cand = w, vz = v_z.
 *   select       df_cell_sort is stable: the rows of a column are in candidate order, map rows first.  For the sorted position p with
 *                c = idx_sorted[p]: rank = the number of positions of the same column before p whose vz equals vz[c];
 *                keep[c] = rank < K, and keep = 0 for every candidate that was dropped.  A voxel keeps its first K rows in candidate
 *                order: older rows win, a full voxel refuses every new row, a map row inside the window is never lost.
 *   compact      the kept rows of sample b in sorted order are rows 0 .. of map_out [B,cap,3] (NOT the buffer cand was made from: the
 *                caller double-buffers); kept_b of them.  count_out[b] = min(kept_b, cap); every row from count_out[b] on is three
 *                float64 NaNs.  stat [B,4] i32 = (rows in the window, kept_b, kept rows that came from the sweep -- counted before the
 *                cut at cap --, overflow = max(0, kept_b - cap)).  Block counts, one scan of them per sample, scatter.  Sorted order
 *                is a valid map: the voxel lattice is fixed in the world, rows that share a column always did, their order is their
 *                age and the next stable sort keeps it.
 *   view         d_i = w_i - t_i; o_j = (R_0j d_0 + R_1j d_1) + R_2j d_2 in float64, then rounded to fp32 (nearest even).  dst
 *                [B,cap,3] f32; rows >= count[b] are three fp32 NaNs of pattern 0x7FC00000.
 * Every output element is written exactly once (df_map_select: a fill launch on the same stream first).  No float atomics; no atomics
 * at all outside df_cell_sort.  Two calls are bit-identical; sample b depends neither on B nor on the other samples.  The entries never
 * allocate, synchronise or read back, and no grid dimension comes from a device value.
 * df_map_ws_bytes(B, cap, N): the bytes of df_map_compact's ws = 8 B ceil((cap + N) / 256); DF_E_SHAPE (negative) for refused shapes.
 * df_map_keys: map [B,cap,3] f64, count [B], sweep [B,N,3] f32, sweep_count [B], mask [B,N] i32, gate [B] i32, pose [B,16] f64 ->
 *   cand [B,n,3] f64, key [B n] u32, vz [B n] i32.  One thread per candidate, grid (ceil(n / 256), B).
 * df_map_select: key, vz as above, idx_sorted [B n] u32 and cell_rng [B S S, 2] i32 as df_cell_sort wrote them -> keep [B n] i32.
 * df_map_compact: -> map_out [B,cap,3] f64, count_out [B] i32, stat [B,4] i32.
 * B outside 1..65535, cap / N / n < 1, W outside 1..2047, B n >= 2^30, B S S >= 2^30: DF_E_SHAPE.  NULL pointers (the nullable ones
 * excepted), a voxel that is not positive and finite, max_per_voxel < 1, map_out == cand: DF_E_ARG.  float64 buffers not 8-byte
 * aligned: DF_E_ALIGN.  No launch then.
 *
 * NEAREST-FIRST EVICTION (opt-in; UNPINNED like the rest: this project's own definition).  df_map_compact_near is
 * a second form of the last stage of an update; keys, sort and select are the ones above.  Where kept_b > cap, `compact` loses the end
 * of the sorted order, the columns of the largest dy: one side of the window, whatever the scene.  This form shrinks the window instead.
 *   ring         of a kept candidate with the key (b S + dy) S + dx: r = max(|dx - W|, |dy - W|), the Chebyshev distance of its column
 *                from the anchor column, 0 .. W.  h_b[r] = the kept candidates of ring r; kept_b = their sum.
 *   no overflow  kept_b <= cap: map_out, count_out and stat are bit for bit `compact`'s, and cut[b] = (W + 1, 0).
 *   overflow     R_b = the largest R in 0 .. W with sum_{r < R} h_b[r] <= cap; budget_b = cap - sum_{r < R_b} h_b[r], so
 *                0 <= budget_b < h_b[R_b].  A kept candidate SURVIVES when its ring is < R_b, or when its ring is R_b and fewer than
 *                budget_b kept candidates of ring R_b precede it in sorted order.  The survivors in sorted order are rows 0 .. cap-1 of
 *                map_out; count_out[b] = cap; cut[b] = (R_b, budget_b).  Said another way: the survivors are the first cap kept
 *                candidates under the order (ring, sorted position), emitted in sorted position.
 *   stat, tail   stat [B,4] keeps `compact`'s four meanings exactly (kept rows from the sweep are counted before the cut; overflow =
 *                max(0, kept_b - cap)); every row from count_out[b] on is three float64 NaNs (0x7FF8000000000000).
 * The result is a valid map under `compact`'s argument: survivors keep their sorted order, and all rows of a column share a ring, so a
 * column is kept whole, dropped whole or -- in ring R_b only -- cut after its oldest rows.  What stays arbitrary is the partial ring R_b:
 * it is filled in sorted order, its smallest dy first.  The error is bounded to one ring instead of a slab of the window.
 * Every output element is written exactly once.  No float atomics; the kept rows per (sample, ring) are counted with integer atomicAdd
 * (an LDS histogram per block, then one add per occupied ring into ws after a fill launch), which the statement above that an update
 * runs no atomics outside df_cell_sort does NOT cover.  An integer sum does not depend on the order of its operands, so two calls are
 * still bit-identical, also with ws, cut and map_out pre-filled with anything; sample b depends neither on B nor on the other samples;
 * nothing is allocated, synchronised or read back, and no grid dimension comes from a device value.
 * df_map_compact_near: cand [B,n,3] f64, key [B n] u32, idx_sorted [B n] u32, cell_rng [B S S, 2] i32, keep [B n] i32 -> map_out
 *   [B,cap,3] f64 (NOT the buffer cand was made from), count_out [B] i32, stat [B,4] i32, cut [B,2] i32.  Six launches: fill, ring
 *   counts (ceil(n / 256), B), the cut (B), block counts (ceil(n / 256), B), one scan per sample (B), scatter (ceil(n / 256), B).
 * df_map_near_ws_bytes(B, cap, N, W): the bytes of its ws = 4 B (W + 1 + 4 ceil((cap + N) / 256)): the ring counts [B][W + 1] i32, then
 *   (rows of rings < R, rows of ring R, kept rows, kept rows from the sweep) per block [B][ceil(n / 256)][4] i32; DF_E_SHAPE (negative)
 *   for refused shapes.
 * Shapes, NULL pointers (cut and key included: none is nullable), map_out == cand and alignment are refused as by df_map_compact. */
int64_t df_map_ws_bytes(int B, int cap, int N);
int df_map_keys(const double* map, const int32_t* count, const float* sweep, const int32_t* sweep_count, const int32_t* mask /*nullable*/,
                const int32_t* gate /*nullable*/, const double* pose, int B, int cap, int N, double voxel, int W, double* cand,
                uint32_t* key, int32_t* vz, void* stream);
int df_map_select(const uint32_t* key, const uint32_t* idx_sorted, const int32_t* cell_rng, const int32_t* vz, int B, int n, int W,
                  int max_per_voxel, int32_t* keep, void* stream);
int df_map_compact(const double* cand, const uint32_t* idx_sorted, const int32_t* cell_rng, const int32_t* keep, int B, int cap, int N,
                   int W, double* map_out, int32_t* count_out, int32_t* stat, void* ws, void* stream);
int df_map_view(const double* map, const int32_t* count, const double* pose, int B, int cap, float* dst, void* stream);
int64_t df_map_near_ws_bytes(int B, int cap, int N, int W);
int df_map_compact_near(const double* cand, const uint32_t* key, const uint32_t* idx_sorted, const int32_t* cell_rng, const int32_t* keep,
                        int B, int cap, int N, int W, double* map_out, int32_t* count_out, int32_t* stat, int32_t* cut, void* ws,
                        void* stream);

/* ------------------------------------------------------------------ depth cube: carving seen-through rows out of the local map ----
 * UNPINNED: this project's own definition; every default of its callers is a choice, not a measurement.  A map
 * row is stale when the current sweep sees through it: a return of the sweep lies well behind the row, along the same direction from
 * the sensor.  The sweep is filed in a DEPTH CUBE about the origin of its own frame -- six faces of R x R bins, R even, img [B,6,R,R]
 * u32 -- and the map's view (df_map_view) is tested against it; df_map_drop then compacts the flagged rows away.
 * ARITHMETIC: no transcendental function; every fp32 operation named below is rounded once, on its own (no fma), so numpy float32
 * reproduces every value bit for bit.
 *   face, bin    of a row (x, y, z): ax, ay, az = the absolute values.  The major axis is 0 if ax >= ay and ax >= az, else 1 if
 *                ay >= az, else 2 (on ties the earlier axis wins).  face = 2 axis + (the major coordinate < 0), so -0.0 is on the
 *                positive face.  m = the absolute major coordinate: the row's DEPTH.  (uc, vc) = the other two coordinates in
 *                ascending axis order.  u = uc / m; i = min(R - 1, (int) floor((u + 1) * (R / 2))) (one division, one addition, one
 *                multiplication; R / 2 is exact); j likewise from vc.  The row's bin is img[b][face][j][i].
 *   takes part   a row r with r < count[b], mask[b,r] > 0 (mask nullable), three finite coordinates and m > 0.
 *   build        every bin = 0x7F800000 (+inf: no return), then the integer minimum of the bit patterns of m over the rows that take
 *                part and fall into the bin (positive floats order as their bits).
 *   test         a query row gets flag = 1 (SEEN THROUGH) exactly when it takes part (count_q; there is no mask), max(|x|, |y|) >=
 *                near (rows the sweep's own min_range band hides are left alone), its own bin is not +inf (an empty bin is no
 *                evidence), the whole window i - halo .. i + halo, j - halo .. j + halo lies inside 0 .. R - 1 (on the row's face:
 *                conservative at face edges) and  (m * c) + margin < dmin,  dmin = the smallest depth of the window's bins and
 *                c = 1 + rel in fp32, computed once on the host from the fp32 argument.  Every other row gets flag = 0.  depth_out
 *                [B,M] f32 (nullable) = dmin for a row that takes part and whose window lies on its face, else +inf (0x7F800000).
 * Every element of flag and depth_out is written exactly once; img by a fill launch and then by atomicMin only.  The statement of the
 * local map section that an update runs no atomics outside df_cell_sort does NOT cover df_depth_cube_build: it is one integer atomicMin
 * per row.  An integer minimum does not depend on the order of its operands, so two calls are still bit-identical, and sample b depends
 * neither on B nor on the other samples.  The entries never allocate, synchronise or read back; no grid dimension comes from a device
 * value.
 * df_depth_cube_build: points [B,N,3] f32, count [B] i32, mask [B,N] i32 -> img [B,6,R,R] u32.  Grid (ceil(N / 256), B) after the fill.
 * df_depth_cube_test: query [B,M,3] f32, count_q [B] i32, img -> flag [B,M] i32, depth_out [B,M] f32.  Grid (ceil(M / 256), B).
 * B outside 1..65535, N / M < 1, B N or B M >= 2^30, R odd or outside 2..2048, 6 B R R >= 2^30: DF_E_SHAPE.  NULL pointers (the nullable
 * ones excepted), halo outside 0..4, margin / rel / near negative or not finite: DF_E_ARG.  Buffers not 4-byte aligned: DF_E_ALIGN.
 *
 * df_map_drop: a stable out-of-place compaction of the map -- block counts, one scan per sample and a scatter, df_map_compact's shape.
 *   map [B,cap,3] f64, count [B] i32, flag [B,cap] i32, gate [B] i32 (nullable) -> map_out [B,cap,3] f64 (NOT map: the caller
 *   double-buffers), count_out [B] i32, stat [B,2] i32.  With c_b = count[b] held to 0 .. cap: the rows j < c_b with flag[b,j] == 0 are
 *   rows 0 .. of map_out in their order (relative order is age, all the next stable sort needs: the result is a valid map under the
 *   argument of `compact` above); count_out[b] = their number; every row from count_out[b] on is three float64 NaNs
 *   (0x7FF8000000000000); a flag at j >= c_b is not looked at.  stat = (rows tested = c_b, rows dropped = c_b - count_out[b]).  A sample
 *   with gate[b] != 0 keeps every row j < c_b whatever its flags and has stat = (0, 0).  No atomics; two calls are bit-identical.
 * df_map_drop_ws_bytes(B, cap): the bytes of ws = 4 B ceil(cap / 256); DF_E_SHAPE (negative) for refused shapes.
 * B outside 1..65535, cap < 1, B cap >= 2^30: DF_E_SHAPE.  NULL pointers (gate excepted), map_out == map: DF_E_ARG.  float64 buffers not
 * 8-byte aligned: DF_E_ALIGN.  No launch then. */
int df_depth_cube_build(const float* points, const int32_t* count, const int32_t* mask /*nullable*/, int B, int N, int R, uint32_t* img,
                        void* stream);
int df_depth_cube_test(const float* query, const int32_t* count_q, const uint32_t* img, int B, int M, int R, int halo, float margin,
                       float rel, float near, int32_t* flag, float* depth_out /*nullable*/, void* stream);
int64_t df_map_drop_ws_bytes(int B, int cap);
int df_map_drop(const double* map, const int32_t* count, const int32_t* flag, const int32_t* gate /*nullable*/, int B, int cap,
                double* map_out, int32_t* count_out, int32_t* stat, void* ws, void* stream);

/* ------------------------------------------------------------------ optimiser (A12) ----
 * torch.optim.Adam (defaults: no amsgrad, no weight decay) over ONE flat fp32 arena holding every
 * parameter; grad/exp_avg/exp_avg_sq are arenas of the same layout.  n % 4 == 0. */
int df_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                 float beta1, float beta2, float eps, int step, float grad_scale, void* stream);
/* the same step with the step number read from device memory (*step_dev >= 1, incremented by the caller before the
 * launch): the form that can be captured in a HIP graph and replayed -- nothing about the step is a host-side constant */
int df_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                     float beta1, float beta2, float eps, const int32_t* step_dev, float grad_scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif
