// Validation metrics on the GPU: the Argoverse-2 tables of deflow_amd/metrics.py (OfficialMetrics, both leaderboard versions) and the
// range-free summary of evaluate_batch, accumulated from a whole padded batch per call without a read-back (include/deflow_amd.h,
// DESIGN.md section 6e).
//
//   df_metrics_rows        grid (blocks, samples), MT_ROWS compact rows per block in MT_TILES tiles of 256.  One thread per row: gather by
//                          idx_c, est = pose_flow + flow in fp32 (one rounded add, as the host path adds them), everything after that in
//                          double with every product, sum, root and quotient rounded separately -- so each thresholded (integer) result is
//                          a pure function of the input.  The row's 24 scalar terms stay in registers and are reduced once per block
//                          (xor butterfly inside a wave, the four waves in order).  The 255 (meta-class, speed-bucket) cells: every tile
//                          stages (cell, err, speed) in LDS and thread t adds the rows of cell t in ascending row order (the reads are
//                          broadcasts).  No float atomics: a block's partials are a fixed-order function of its rows.
//   df_metrics_accumulate  (a) per sample, the block partials summed in ascending block order; (b) one block walks the samples in ascending
//                          order: skip rule, per-frame values, running state.
#include <math.h>

#include "common.h"

namespace {

constexpr int MT_THREADS = 256;
constexpr int MT_TILES = 8;
constexpr int MT_ROWS = MT_THREADS * MT_TILES;      // rows per block (df_metrics_rows_per_block)
constexpr int MT_NBKT = 51, MT_CELLS = 5 * MT_NBKT;
constexpr int MT_NCAT = 31;
// a block's (and a frame's) doubles: the scalar sums, then err_sum[255], speed_sum[255]
enum { D_FD, D_FS, D_BS, D_EPE, D_ANG, D_S_EPE, D_S_FD, D_S_FS, D_S_BS, MT_SD };
constexpr int MT_ND = MT_SD + 2 * MT_CELLS;
// ... and its counts: the scalar counts, then count[255]
enum { I_FD, I_FS, I_BS, I_TP, I_FP, I_FN, I_N, I_ACCS, I_ACCR, I_S_N, I_S_ACCS, I_S_ACCR, I_S_FD, I_S_FS, I_S_BS, MT_SI };
constexpr int MT_NI = MT_SI + MT_CELLS;
// running state (see the header): doubles v1_sum[8] err_sum[255] speed_sum[255] tot[8]; int64 v1_cnt[8] n count[255] wsum[8]
constexpr int SF_V1 = 0, SF_ERR = 8, SF_SPD = SF_ERR + MT_CELLS, SF_TOT = SF_SPD + MT_CELLS;
constexpr int SI_V1 = 0, SI_N = 8, SI_CNT = 9, SI_W = SI_CNT + MT_CELLS;
enum { V1_FD, V1_FS, V1_BS, V1_IOU, V1_EPE, V1_ACCS, V1_ACCR, V1_ANG };
enum { SM_EPE, SM_ACCS, SM_ACCR, SM_N, SM_FD, SM_FS, SM_BS, SM_3WAY, SM_KEYS };

constexpr double MT_CLOSE = 35.0, MT_DYN = 0.05;

// av2 label index -> meta-class of the bucketed metric (-1: not evaluated), deflow_amd/metrics.py _META_OF
__device__ const signed char mt_meta_of[MT_NCAT] = {0,  -1, 2,  4, 4, -1, 2, 2, -1, -1, -1, 2, -1, -1, 4, 4,
                                                    3,  3,  2,  1, 2, -1, -1, 3, -1, 2,  2,  2, 3,  4,  4};

struct MtWs {
  double* pd;   // [B][K][MT_ND]
  double* fd;   // [B][MT_ND]
  int32_t* pi;  // [B][K][MT_NI]
  int32_t* fi;  // [B][MT_NI]
};
inline int mt_blocks(int N) { return (N + MT_ROWS - 1) / MT_ROWS; }
inline MtWs mt_carve(void* ws, int B, int N) {
  const int64_t K = mt_blocks(N);
  MtWs w;
  w.pd = reinterpret_cast<double*>(ws);
  w.fd = w.pd + (int64_t)B * K * MT_ND;
  w.pi = reinterpret_cast<int32_t*>(w.fd + (int64_t)B * MT_ND);
  w.fi = w.pi + (int64_t)B * K * MT_NI;
  return w;
}
inline int64_t mt_ws_bytes(int B, int N) { return ((int64_t)B * mt_blocks(N) + B) * (MT_ND * 8 + MT_NI * 4); }
inline bool mt_dims_ok(int B, int N) { return B >= 1 && B <= 65535 && N >= 1 && (int64_t)B * N < 0x80000000ll; }

// sqrt((x x + y y) + z z), every operation rounded on its own whatever -ffp-contract says
__device__ __forceinline__ double mt_norm3(double x, double y, double z) {
  return __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)), __dmul_rn(z, z)));
}
__device__ __forceinline__ double mt_dot3p(double ax, double ay, double az, double bx, double by, double bz) {   // a . b + 0.01
  return __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(ax, bx), __dmul_rn(ay, by)), __dmul_rn(az, bz)), 0.01);
}
__device__ __forceinline__ bool mt_fin3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

__global__ __launch_bounds__(MT_THREADS) void mt_rows_kernel(const float* __restrict__ flow, const float* __restrict__ pose_flow,
                                                             const float* __restrict__ pc0, const float* __restrict__ gt_flow,
                                                             const int64_t* __restrict__ idx_c, const int32_t* __restrict__ counts,
                                                             const uint8_t* __restrict__ is_valid, const uint8_t* __restrict__ eval_mask,
                                                             const uint8_t* __restrict__ cats, int N, const double* __restrict__ edges,
                                                             double* __restrict__ pd, int32_t* __restrict__ pi, int32_t* __restrict__ status) {
  __shared__ double s_edges[MT_NBKT - 1];
  __shared__ int s_cell[MT_THREADS];
  __shared__ double s_err[MT_THREADS], s_spd[MT_THREADS];
  __shared__ double s_wd[MT_THREADS / 64][MT_SD];
  __shared__ int s_wi[MT_THREADS / 64][MT_SI];
  const int tid = threadIdx.x, b = blockIdx.y, k = blockIdx.x;
  const int cnt = min(max(counts[b], 0), N);
  const int row0 = k * MT_ROWS;
  if (row0 >= cnt) return;                      // (uniform) df_metrics_accumulate reads the blocks below ceil(cnt / MT_ROWS) only
  if (tid < MT_NBKT - 1) s_edges[tid] = edges[tid];
  __syncthreads();
  double ad[MT_SD];
  int ai[MT_SI];
#pragma unroll
  for (int q = 0; q < MT_SD; ++q) ad[q] = 0.0;
#pragma unroll
  for (int q = 0; q < MT_SI; ++q) ai[q] = 0;
  double ce = 0.0, cs = 0.0;                    // cell `tid` of this block
  int cc = 0;
  const int64_t sample = (int64_t)b * N;
  for (int tile = 0; tile < MT_TILES; ++tile) {
    const int tile0 = row0 + tile * MT_THREADS;
    if (tile0 >= cnt) break;                    // (uniform)
    const int i = tile0 + tid;
    int cell = -1;
    double err = 0.0, speed = 0.0;
    if (i < cnt) {
      const int64_t j = idx_c[sample + i];
      if (j < 0 || j >= N) {
        if (status) atomicAdd(status, 1);
      } else {
        const int64_t at = sample + j;
        const float* fl = flow + (sample + i) * 3;
        const float *pf = pose_flow + at * 3, *pc = pc0 + at * 3, *gp = gt_flow + at * 3;
        const float rx = pf[0], ry = pf[1], rz = pf[2];
        const float ex = __fadd_rn(rx, fl[0]), ey = __fadd_rn(ry, fl[1]), ez = __fadd_rn(rz, fl[2]);
        const float gx = gp[0], gy = gp[1], gz = gp[2];
        const float px = pc[0], py = pc[1], pz = pc[2];
        const bool ok = (!is_valid || is_valid[at] != 0) && (!eval_mask || eval_mask[at] != 0);
        const int cat = cats ? min((int)cats[at], MT_NCAT - 1) : 0;
        const bool fin_eg = mt_fin3(ex, ey, ez) && mt_fin3(gx, gy, gz);
        const bool fin = fin_eg && mt_fin3(rx, ry, rz) && mt_fin3(px, py, pz);
        err = mt_norm3((double)ex - (double)gx, (double)ey - (double)gy, (double)ez - (double)gz);
        speed = mt_norm3((double)gx - (double)rx, (double)gy - (double)ry, (double)gz - (double)rz);
        const double est_speed = mt_norm3((double)ex - (double)rx, (double)ey - (double)ry, (double)ez - (double)rz);
        const double gtn = mt_norm3(gx, gy, gz);
        const double rel = __ddiv_rn(err, __dadd_rn(gtn, 1e-10));
        const bool acc_s = err < 0.05 || rel < 0.05, acc_r = err < 0.10 || rel < 0.10;
        const bool dyn = speed >= MT_DYN, est_dyn = est_speed >= MT_DYN;
        // ---- the range-free summary (epe_metrics on the rows that pass the masks): foreground = every row when there are no categories
        if (ok && fin_eg) {
          const bool fg = cats ? cat != 0 : true;
          ad[D_S_EPE] += err;
          ai[I_S_N] += 1;
          ai[I_S_ACCS] += acc_s;
          ai[I_S_ACCR] += acc_r;
          if (fg && dyn) { ad[D_S_FD] += err; ai[I_S_FD] += 1; }
          if (fg && !dyn) { ad[D_S_FS] += err; ai[I_S_FS] += 1; }
          if (!fg && !dyn) { ad[D_S_BS] += err; ai[I_S_BS] += 1; }
        }
        // ---- leaderboard version 1: the box |x|, |y| <= 35 m
        const bool sel = fin && ok && fabs((double)px) <= MT_CLOSE && fabs((double)py) <= MT_CLOSE;
        if (sel) {
          const bool fg = cat != 0;
          if (fg && dyn) { ad[D_FD] += err; ai[I_FD] += 1; }
          if (fg && !dyn) { ad[D_FS] += err; ai[I_FS] += 1; }
          if (!fg && !dyn) { ad[D_BS] += err; ai[I_BS] += 1; }
          ai[I_TP] += est_dyn && dyn;
          ai[I_FP] += est_dyn && !dyn;
          ai[I_FN] += !est_dyn && dyn;
          ai[I_N] += 1;
          ai[I_ACCS] += acc_s;
          ai[I_ACCR] += acc_r;
          ad[D_EPE] += err;
          // the angle between the space-time vectors (flow, 0.1): metrics._angle
          const double dot = mt_dot3p(ex, ey, ez, gx, gy, gz);
          const double nn = __dmul_rn(__dsqrt_rn(mt_dot3p(ex, ey, ez, ex, ey, ez)), __dsqrt_rn(mt_dot3p(gx, gy, gz, gx, gy, gz)));
          ad[D_ANG] += acos(fmin(fmax(__ddiv_rn(dot, nn), -1.0), 1.0));
        }
        // ---- leaderboard version 2: the 35 m radius, evaluated categories; bucket = the number of edges <= speed
        const int meta = mt_meta_of[cat];
        const double radius = __dsqrt_rn(__dadd_rn(__dmul_rn((double)px, (double)px), __dmul_rn((double)py, (double)py)));
        if (fin && ok && radius <= MT_CLOSE && meta >= 0) {
          int kb = (int)fmin(speed * 25.0, (double)(MT_NBKT - 1));          // a guess, put right against the edges themselves
          while (kb < MT_NBKT - 1 && speed >= s_edges[kb]) ++kb;
          while (kb > 0 && speed < s_edges[kb - 1]) --kb;
          cell = meta * MT_NBKT + kb;
        }
      }
    }
    s_cell[tid] = cell;
    s_err[tid] = err;
    s_spd[tid] = speed;
    __syncthreads();
    if (tid < MT_CELLS) {
      for (int r = 0; r < MT_THREADS; ++r) {
        if (s_cell[r] == tid) {
          ce += s_err[r];
          cs += s_spd[r];
          cc += 1;
        }
      }
    }
    __syncthreads();
  }
  // ---- the scalar terms: xor butterfly inside each wave, then the waves in order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int q = 0; q < MT_SD; ++q) ad[q] += __shfl_xor(ad[q], o, 64);
#pragma unroll
    for (int q = 0; q < MT_SI; ++q) ai[q] += __shfl_xor(ai[q], o, 64);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int q = 0; q < MT_SD; ++q) s_wd[tid >> 6][q] = ad[q];
#pragma unroll
    for (int q = 0; q < MT_SI; ++q) s_wi[tid >> 6][q] = ai[q];
  }
  __syncthreads();
  double* od = pd + ((int64_t)b * gridDim.x + k) * MT_ND;
  int32_t* oi = pi + ((int64_t)b * gridDim.x + k) * MT_NI;
  if (tid < MT_SD) od[tid] = ((s_wd[0][tid] + s_wd[1][tid]) + s_wd[2][tid]) + s_wd[3][tid];
  if (tid >= 64 && tid < 64 + MT_SI) oi[tid - 64] = s_wi[0][tid - 64] + s_wi[1][tid - 64] + s_wi[2][tid - 64] + s_wi[3][tid - 64];
  if (tid < MT_CELLS) {
    od[MT_SD + tid] = ce;
    od[MT_SD + MT_CELLS + tid] = cs;
    oi[MT_SI + tid] = cc;
  }
}

// (a) a frame's sums: quantity q of sample b over the sample's blocks, ascending
__global__ __launch_bounds__(256) void mt_frame_kernel(const int32_t* __restrict__ counts, int N, int K, const double* __restrict__ pd,
                                                       const int32_t* __restrict__ pi, double* __restrict__ fd, int32_t* __restrict__ fi) {
  const int b = blockIdx.y, q = blockIdx.x * 256 + threadIdx.x;
  if (q >= MT_ND + MT_NI) return;
  const int cnt = min(max(counts[b], 0), N);
  const int nb = (cnt + MT_ROWS - 1) / MT_ROWS;
  if (q < MT_ND) {
    const double* p = pd + (int64_t)b * K * MT_ND + q;
    double s = 0.0;
    for (int k = 0; k < nb; ++k) s += p[(int64_t)k * MT_ND];
    fd[(int64_t)b * MT_ND + q] = s;
  } else {
    const int qi = q - MT_ND;
    const int32_t* p = pi + (int64_t)b * K * MT_NI + qi;
    int32_t s = 0;
    for (int k = 0; k < nb; ++k) s += p[(int64_t)k * MT_NI];
    fi[(int64_t)b * MT_NI + qi] = s;
  }
}

// (b) one block: the samples in ascending order, MT_CHUNK at a time.  Threads 0..254 own one cell each; thread 255 owns the per-frame
// values (their terms are staged in LDS by everybody first)
constexpr int MT_CHUNK = 32;

__global__ __launch_bounds__(256) void mt_state_kernel(const uint8_t* __restrict__ has, int B, const double* __restrict__ fd,
                                                       const int32_t* __restrict__ fi, double* __restrict__ sf, int64_t* __restrict__ si) {
  __shared__ double s_d[MT_CHUNK][MT_SD];
  __shared__ int s_i[MT_CHUNK][MT_SI];
  const int tid = threadIdx.x;
  int mine = 0;
  if (has)
    for (int b = tid; b < B; b += 256) mine |= has[b] != 0;
  const bool any_has = __syncthreads_or(mine) != 0;      // a frame without the benchmark's mask is skipped iff some frame has one
  double ce = 0.0, cs = 0.0;
  int64_t cc = 0;
  if (tid < MT_CELLS) {
    ce = sf[SF_ERR + tid];
    cs = sf[SF_SPD + tid];
    cc = si[SI_CNT + tid];
  }
  double v1s[8], bsum[SM_KEYS];
  int v1c[8], bcnt[SM_KEYS];
  int64_t n_add = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) { v1s[q] = 0.0; v1c[q] = 0; }
#pragma unroll
  for (int q = 0; q < SM_KEYS; ++q) { bsum[q] = 0.0; bcnt[q] = 0; }
  if (tid == 255) {
#pragma unroll
    for (int q = 0; q < 8; ++q) v1s[q] = sf[SF_V1 + q];
  }
  for (int b0 = 0; b0 < B; b0 += MT_CHUNK) {
    const int nb = min(MT_CHUNK, B - b0);
    for (int e = tid; e < nb * (MT_SD + MT_SI); e += 256) {
      const int lb = e / (MT_SD + MT_SI), q = e % (MT_SD + MT_SI);
      if (q < MT_SD) s_d[lb][q] = fd[(int64_t)(b0 + lb) * MT_ND + q];
      else s_i[lb][q - MT_SD] = fi[(int64_t)(b0 + lb) * MT_NI + q - MT_SD];
    }
    __syncthreads();
    if (tid < MT_CELLS) {
      for (int lb = 0; lb < nb; ++lb) {
        const int b = b0 + lb;
        if (any_has && has[b] == 0) continue;
        ce += fd[(int64_t)b * MT_ND + MT_SD + tid];
        cs += fd[(int64_t)b * MT_ND + MT_SD + MT_CELLS + tid];
        cc += fi[(int64_t)b * MT_NI + MT_SI + tid];
      }
    } else if (tid == 255) {
      for (int lb = 0; lb < nb; ++lb) {
        if (any_has && has[b0 + lb] == 0) continue;
        const double* d = s_d[lb];
        const int* c = s_i[lb];
        // ---- version 1: per-frame values, each averaged over the frames that have it
        if (c[I_FD]) { v1s[V1_FD] += d[D_FD] / c[I_FD]; v1c[V1_FD] += 1; }
        if (c[I_FS]) { v1s[V1_FS] += d[D_FS] / c[I_FS]; v1c[V1_FS] += 1; }
        if (c[I_BS]) { v1s[V1_BS] += d[D_BS] / c[I_BS]; v1c[V1_BS] += 1; }
        const int u = c[I_TP] + c[I_FP] + c[I_FN];
        if (u) { v1s[V1_IOU] += (double)c[I_TP] / (double)u; v1c[V1_IOU] += 1; }
        if (c[I_N]) {
          v1s[V1_EPE] += d[D_EPE] / c[I_N];
          v1s[V1_ACCS] += (double)c[I_ACCS] / c[I_N];
          v1s[V1_ACCR] += (double)c[I_ACCR] / c[I_N];
          v1s[V1_ANG] += d[D_ANG] / c[I_N];
          v1c[V1_EPE] += 1; v1c[V1_ACCS] += 1; v1c[V1_ACCR] += 1; v1c[V1_ANG] += 1;
        }
        n_add += c[I_N];
        // ---- the summary of this sample; a key joins the batch mean when its value is not NaN
        bsum[SM_N] += (double)c[I_S_N];
        bcnt[SM_N] += 1;
        if (c[I_S_N]) {
          bsum[SM_EPE] += d[D_S_EPE] / c[I_S_N];
          bsum[SM_ACCS] += (double)c[I_S_ACCS] / c[I_S_N];
          bsum[SM_ACCR] += (double)c[I_S_ACCR] / c[I_S_N];
          bcnt[SM_EPE] += 1; bcnt[SM_ACCS] += 1; bcnt[SM_ACCR] += 1;
        }
        double three = 0.0;
        int nthree = 0;
        if (c[I_S_FD]) { const double v = d[D_S_FD] / c[I_S_FD]; bsum[SM_FD] += v; bcnt[SM_FD] += 1; three += v; nthree += 1; }
        if (c[I_S_FS]) { const double v = d[D_S_FS] / c[I_S_FS]; bsum[SM_FS] += v; bcnt[SM_FS] += 1; three += v; nthree += 1; }
        if (c[I_S_BS]) { const double v = d[D_S_BS] / c[I_S_BS]; bsum[SM_BS] += v; bcnt[SM_BS] += 1; three += v; nthree += 1; }
        if (nthree) { bsum[SM_3WAY] += three / nthree; bcnt[SM_3WAY] += 1; }
      }
    }
    __syncthreads();
  }
  if (tid < MT_CELLS) {
    sf[SF_ERR + tid] = ce;
    sf[SF_SPD + tid] = cs;
    si[SI_CNT + tid] = cc;
  } else if (tid == 255) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      sf[SF_V1 + q] = v1s[q];
      si[SI_V1 + q] += v1c[q];
    }
    si[SI_N] += n_add;
#pragma unroll
    for (int q = 0; q < SM_KEYS; ++q) {
      if (bcnt[q]) {                            // tot += batch mean x batch size, wsum += batch size: what eval.py does with evaluate_batch
        sf[SF_TOT + q] += (bsum[q] / bcnt[q]) * (double)B;
        si[SI_W + q] += B;
      }
    }
  }
}

}  // namespace

extern "C" int df_metrics_rows_per_block(void) { return MT_ROWS; }

extern "C" int64_t df_metrics_ws_bytes(int B, int N) { return mt_dims_ok(B, N) ? mt_ws_bytes(B, N) : (int64_t)DF_E_SHAPE; }

extern "C" int df_metrics_rows(const float* flow, const float* pose_flow, const float* pc0, const float* gt_flow, const int64_t* idx_c,
                               const int32_t* counts, const uint8_t* is_valid, const uint8_t* eval_mask, const uint8_t* cats, int B, int N,
                               const double* edges, void* ws, int32_t* status, void* stream) {
  DF_REQUIRE(flow && pose_flow && pc0 && gt_flow && idx_c && counts && edges && ws, DF_E_ARG);
  DF_REQUIRE(mt_dims_ok(B, N), DF_E_SHAPE);
  DF_REQUIRE((((uintptr_t)ws) & 7u) == 0, DF_E_ALIGN);
  const MtWs w = mt_carve(ws, B, N);
  hipLaunchKernelGGL(mt_rows_kernel, dim3(mt_blocks(N), B), dim3(MT_THREADS), 0, reinterpret_cast<hipStream_t>(stream), flow, pose_flow, pc0,
                     gt_flow, idx_c, counts, is_valid, eval_mask, cats, N, edges, w.pd, w.pi, status);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

extern "C" int df_metrics_accumulate(const int32_t* counts, const uint8_t* has_eval_mask, int B, int N, void* ws, double* state_f,
                                     int64_t* state_i, void* stream) {
  DF_REQUIRE(counts && ws && state_f && state_i, DF_E_ARG);
  DF_REQUIRE(mt_dims_ok(B, N), DF_E_SHAPE);
  DF_REQUIRE((((uintptr_t)ws) & 7u) == 0, DF_E_ALIGN);
  const MtWs w = mt_carve(ws, B, N);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mt_frame_kernel, dim3((MT_ND + MT_NI + 255) / 256, B), dim3(256), 0, s, counts, N, mt_blocks(N), w.pd, w.pi, w.fd, w.fi);
  DF_CHECK_LAUNCH();
  hipLaunchKernelGGL(mt_state_kernel, dim3(1), dim3(256), 0, s, has_eval_mask, B, w.fd, w.fi, state_f, state_i);
  DF_CHECK_LAUNCH();
  return DF_OK;
}
