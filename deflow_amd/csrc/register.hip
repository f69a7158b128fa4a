// Sweep-to-sweep registration (odometry): a robust point-to-point ICP of whole clouds in 6 degrees of freedom that stays on the device.
// UNPINNED -- the definition is this project's own: include/deflow_amd.h, DESIGN.md section 6r.
//
//   df_reg_accumulate   one thread per cell-ordered source position: q = R s + t in fp32, the ring search of df_chamfer_nn (nn_search.h: the
//                       same device function) for its nearest target row, the Geman-McClure weight, and the row's terms of the normal
//                       equations of T <- exp(delta) T.  J = [ -[q]x , I ] makes H = sum w J^T J a function of TEN distinct sums
//                       (w (|q|^2 I - q q^T): 6, w q: 3, w: 1): those, g's 6, sum w d2 and the inlier count -- 18 values -- go through the
//                       wave butterfly and the block's LDS in float64, and the 32-wide slab row is laid out from them (a copy or an exact
//                       negation of a sum, or 0).  One slab row per block, no atomics.
//   df_reg_accumulate_plane   the same thread mapping, transform and search; the residual is e = n . (q - d) with n the matched target
//                       row's normal (normals.hip: df_normals), the row of the normal equations a = (q x n, n).  H = sum w a a^T has no
//                       structure to exploit: its 21 sums, g's 6, sum w, sum w e^2 and the inlier count -- 30 values -- ARE the slab's
//                       columns 0..29 and go through the same butterfly and LDS order.  df_reg_solve serves both.
//   df_reg_solve        one 64-thread block per sample: lanes 0..31 add the slab rows in ascending block order, lane 0 solves the 6 x 6
//                       system by Cholesky in float64 and applies the closed-form SE(3) exponential to T in place.
#include <math.h>

#include "common.h"
#include "nn_search.h"

namespace {

constexpr int REG_NRED = 18;        // values a block reduces
constexpr int REG_SLAB = 32;        // doubles per slab row
constexpr double REG_SERIES_THETA = 1e-2;
constexpr double REG_PIVOT_REL = 1e-9;

// slab column -> (reduced value, sign); sign 0: the column is 0.  Reduced values: 0 w(qy^2+qz^2), 1 -w qx qy, 2 -w qx qz, 3 w(qx^2+qz^2),
// 4 -w qy qz, 5 w(qx^2+qy^2), 6..8 w q, 9 w, 10..12 w q x r, 13..15 w r, 16 w d2, 17 inliers
__device__ const int8_t REG_SRC[REG_SLAB] = {0, 1, 2, 0, 8, 7, 3, 4, 8, 0, 6, 5, 7, 6, 0, 9, 0, 0, 9, 0, 9, 10, 11, 12, 13, 14, 15, 9, 16, 17, 0, 0};
__device__ const int8_t REG_SGN[REG_SLAB] = {1, 1, 1, 0, -1, 1, 1, 1, 1, 0, -1, 1, -1, 1, 0, 1, 0, 0, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0};

// the defaults of the per-row outputs: every element of a given output, before the accumulate kernel writes the used rows
__global__ __launch_bounds__(256) void reg_fill_kernel(int64_t n, float* __restrict__ q_out, int32_t* __restrict__ idx_out,
                                                       float* __restrict__ d2_out, float* __restrict__ w_out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (q_out) {
    q_out[i * 3] = 0.f;
    q_out[i * 3 + 1] = 0.f;
    q_out[i * 3 + 2] = 0.f;
  }
  if (idx_out) idx_out[i] = -1;
  if (d2_out) d2_out[i] = INFINITY;
  if (w_out) w_out[i] = 0.f;
}

__global__ __launch_bounds__(256) void reg_accumulate_kernel(const int32_t* __restrict__ src_rng, const f32x4* __restrict__ src_sorted, int Gs,
                                                             const int32_t* __restrict__ dst_rng, const f32x4* __restrict__ dst_sorted,
                                                             float minx, float miny, float cell, int G, int Ns, int stride,
                                                             const double* __restrict__ T, float max_dist2, float k2,
                                                             double* __restrict__ partial, float* __restrict__ q_out,
                                                             int32_t* __restrict__ idx_out, float* __restrict__ d2_out,
                                                             float* __restrict__ w_out) {
  const int b = blockIdx.y, tid = threadIdx.x, t = blockIdx.x * 256 + tid;
  const int64_t c0 = (int64_t)b * Gs * Gs;
  const int s0 = src_rng[2 * c0], s1 = src_rng[2 * (c0 + (int64_t)Gs * Gs - 1) + 1];     // the sample's span in the source's cell order
  double a[REG_NRED];
#pragma unroll
  for (int k = 0; k < REG_NRED; ++k) a[k] = 0.0;
  const int64_t p = (int64_t)s0 + t;
  // (every thread stays for the reductions below: no early return)
  if (t < Ns && s0 >= 0 && p < (int64_t)s1 && p < (int64_t)gridDim.y * Ns && t % stride == 0) {
    const f32x4 v = src_sorted[p];
    const float vw = v.w;
    const int row = __builtin_bit_cast(int, vw);
    const double* Tb = T + (int64_t)b * 16;
    const float qx = fmaf((float)Tb[2], v.z, fmaf((float)Tb[1], v.y, fmaf((float)Tb[0], v.x, (float)Tb[3])));
    const float qy = fmaf((float)Tb[6], v.z, fmaf((float)Tb[5], v.y, fmaf((float)Tb[4], v.x, (float)Tb[7])));
    const float qz = fmaf((float)Tb[10], v.z, fmaf((float)Tb[9], v.y, fmaf((float)Tb[8], v.x, (float)Tb[11])));
    float best = INFINITY;
    int bi = -1;
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (nn_finite3(qx, qy, qz))
      nn_ring_search<true>(qx, qy, qz, dst_rng + (int64_t)b * G * G * 2, dst_sorted, minx, miny, cell, G, max_dist2, best, bi, bv);
    float w = 0.f;
    if (best <= max_dist2) {
      const float u = k2 / (k2 + best);
      w = u * u;
      const float rx = qx - bv.x, ry = qy - bv.y, rz = qz - bv.z;
      const float wqx = w * qx, wqy = w * qy, wqz = w * qz;
      a[0] = (double)(w * (qy * qy + qz * qz));
      a[1] = (double)(-(wqx * qy));
      a[2] = (double)(-(wqx * qz));
      a[3] = (double)(w * (qx * qx + qz * qz));
      a[4] = (double)(-(wqy * qz));
      a[5] = (double)(w * (qx * qx + qy * qy));
      a[6] = (double)wqx;
      a[7] = (double)wqy;
      a[8] = (double)wqz;
      a[9] = (double)w;
      a[10] = (double)(w * (qy * rz - qz * ry));
      a[11] = (double)(w * (qz * rx - qx * rz));
      a[12] = (double)(w * (qx * ry - qy * rx));
      a[13] = (double)(w * rx);
      a[14] = (double)(w * ry);
      a[15] = (double)(w * rz);
      a[16] = (double)(w * best);
      a[17] = 1.0;
    } else {
      best = INFINITY;
      bi = -1;
    }
    if ((unsigned)row < (unsigned)Ns) {
      const int64_t o = (int64_t)b * Ns + row;
      if (q_out) {
        q_out[o * 3] = qx;
        q_out[o * 3 + 1] = qy;
        q_out[o * 3 + 2] = qz;
      }
      if (idx_out) idx_out[o] = bi;
      if (d2_out) d2_out[o] = best;
      if (w_out) w_out[o] = w;
    }
  }
  // fixed order: the wave's xor butterfly, then the block's waves in wave order
#pragma unroll
  for (int k = 0; k < REG_NRED; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a[k] += __shfl_xor(a[k], o, 64);
  }
  __shared__ double red[4][REG_NRED];
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < REG_NRED; ++k) red[tid >> 6][k] = a[k];
  }
  __syncthreads();
  if (tid < REG_SLAB) {
    const int k = REG_SRC[tid];
    const double s = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    const int sg = REG_SGN[tid];
    partial[((int64_t)b * gridDim.x + blockIdx.x) * REG_SLAB + tid] = sg > 0 ? s : (sg < 0 ? -s : 0.0);
  }
}

// ---- point-to-plane: the same mapping, transform and search; the residual is the distance to the matched row's plane -----------------
constexpr int REG_NRED_PLANE = 30;  // the slab's columns 0..29 themselves: nothing is laid out afterwards

__global__ __launch_bounds__(256) void reg_fill_plane_kernel(int64_t n, float* __restrict__ q_out, int32_t* __restrict__ idx_out,
                                                             float* __restrict__ d2_out, float* __restrict__ w_out,
                                                             float* __restrict__ e_out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (q_out) {
    q_out[i * 3] = 0.f;
    q_out[i * 3 + 1] = 0.f;
    q_out[i * 3 + 2] = 0.f;
  }
  if (idx_out) idx_out[i] = -1;
  if (d2_out) d2_out[i] = INFINITY;
  if (w_out) w_out[i] = 0.f;
  if (e_out) e_out[i] = 0.f;
}

// Every term is a product (or a sum of products) in which each factor that comes from n changes sign with n and nothing else does: the
// rounding of a product, of a sum of two such products and of an fma of them is symmetric, so negating the fp32 n negates a and e
// exactly and leaves w, w a a^T, w a e and w e^2 bit for bit.  (+ 0.0 below: a -0 product enters the sums as +0 whatever n's sign.)
__global__ __launch_bounds__(256) void reg_accumulate_plane_kernel(const int32_t* __restrict__ src_rng, const f32x4* __restrict__ src_sorted,
                                                                   int Gs, const int32_t* __restrict__ dst_rng,
                                                                   const f32x4* __restrict__ dst_sorted, const f32x4* __restrict__ dst_normals,
                                                                   float minx, float miny, float cell, int G, int Ns, int Nd, int stride,
                                                                   const double* __restrict__ T, float max_dist2, float k2,
                                                                   double* __restrict__ partial, float* __restrict__ q_out,
                                                                   int32_t* __restrict__ idx_out, float* __restrict__ d2_out,
                                                                   float* __restrict__ w_out, float* __restrict__ e_out) {
  const int b = blockIdx.y, tid = threadIdx.x, t = blockIdx.x * 256 + tid;
  const int64_t c0 = (int64_t)b * Gs * Gs;
  const int s0 = src_rng[2 * c0], s1 = src_rng[2 * (c0 + (int64_t)Gs * Gs - 1) + 1];     // the sample's span in the source's cell order
  double a[REG_NRED_PLANE];
#pragma unroll
  for (int k = 0; k < REG_NRED_PLANE; ++k) a[k] = 0.0;
  const int64_t p = (int64_t)s0 + t;
  // (every thread stays for the reductions below: no early return)
  if (t < Ns && s0 >= 0 && p < (int64_t)s1 && p < (int64_t)gridDim.y * Ns && t % stride == 0) {
    const f32x4 v = src_sorted[p];
    const float vw = v.w;
    const int row = __builtin_bit_cast(int, vw);
    const double* Tb = T + (int64_t)b * 16;
    const float qx = fmaf((float)Tb[2], v.z, fmaf((float)Tb[1], v.y, fmaf((float)Tb[0], v.x, (float)Tb[3])));
    const float qy = fmaf((float)Tb[6], v.z, fmaf((float)Tb[5], v.y, fmaf((float)Tb[4], v.x, (float)Tb[7])));
    const float qz = fmaf((float)Tb[10], v.z, fmaf((float)Tb[9], v.y, fmaf((float)Tb[8], v.x, (float)Tb[11])));
    float best = INFINITY;
    int bi = -1;
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (nn_finite3(qx, qy, qz))
      nn_ring_search<true>(qx, qy, qz, dst_rng + (int64_t)b * G * G * 2, dst_sorted, minx, miny, cell, G, max_dist2, best, bi, bv);
    float w = 0.f, e = 0.f;
    f32x4 n = {0.f, 0.f, 0.f, -1.f};
    if (best <= max_dist2 && (unsigned)bi < (unsigned)Nd) n = dst_normals[(int64_t)b * Nd + bi];
    if (n.w >= 0.f) {
      const float rx = qx - bv.x, ry = qy - bv.y, rz = qz - bv.z;
      e = n.x * rx + n.y * ry + n.z * rz;
      const float e2 = e * e;
      const float u = k2 / (k2 + e2);
      w = u * u;
      const float av[6] = {qy * n.z - qz * n.y, qz * n.x - qx * n.z, qx * n.y - qy * n.x, n.x, n.y, n.z};
      int c = 0;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const float wa = w * av[i];
#pragma unroll
        for (int j = i; j < 6; ++j) a[c++] = (double)(wa * av[j]) + 0.0;
        a[21 + i] = (double)(wa * e) + 0.0;
      }
      a[27] = (double)w;
      a[28] = (double)((w * e) * e);
      a[29] = 1.0;
    } else {
      best = INFINITY;
      bi = -1;
    }
    if ((unsigned)row < (unsigned)Ns) {
      const int64_t o = (int64_t)b * Ns + row;
      if (q_out) {
        q_out[o * 3] = qx;
        q_out[o * 3 + 1] = qy;
        q_out[o * 3 + 2] = qz;
      }
      if (idx_out) idx_out[o] = bi;
      if (d2_out) d2_out[o] = best;
      if (w_out) w_out[o] = w;
      if (e_out) e_out[o] = e;
    }
  }
  // fixed order: the wave's xor butterfly, then the block's waves in wave order
#pragma unroll
  for (int k = 0; k < REG_NRED_PLANE; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a[k] += __shfl_xor(a[k], o, 64);
  }
  __shared__ double red[4][REG_SLAB];
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < REG_NRED_PLANE; ++k) red[tid >> 6][k] = a[k];
    red[tid >> 6][30] = 0.0;
    red[tid >> 6][31] = 0.0;
  }
  __syncthreads();
  if (tid < REG_SLAB)
    partial[((int64_t)b * gridDim.x + blockIdx.x) * REG_SLAB + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

__global__ __launch_bounds__(64) void reg_solve_kernel(const double* __restrict__ partial, int nblk, int min_inliers, int planar,
                                                       double* __restrict__ T, float* __restrict__ log_out, int32_t* __restrict__ status) {
  const int b = blockIdx.x, tid = threadIdx.x;
  __shared__ double S[REG_SLAB];
  if (tid < REG_SLAB) {
    const double* pb = partial + (int64_t)b * nblk * REG_SLAB + tid;
    double s = 0.0;
    for (int k = 0; k < nblk; ++k) s += pb[(int64_t)k * REG_SLAB];      // ascending block order
    S[tid] = s;
  }
  __syncthreads();
  if (tid != 0) return;
  const double sw = S[27], swr = S[28], inl = S[29];
  const float mean = sw > 0.0 ? (float)(swr / sw) : 0.f;
  float* lg = log_out + (int64_t)b * 4;
  lg[0] = (float)inl;
  lg[1] = mean;
  lg[2] = 0.f;
  lg[3] = 0.f;
  if (!T) return;
  if (!(inl >= (double)min_inliers)) {
    status[b] = 2;
    return;
  }
  double H[6][6], g[6];
  {
    int c = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int j = i; j < 6; ++j) {
        H[i][j] = S[c];
        H[j][i] = S[c];
        ++c;
      }
      g[i] = S[21 + i];
    }
  }
  const int first = planar ? 2 : 0;       // planar: omega_x, omega_y are not solved for
  double dmax = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
    if (i >= first) dmax = fmax(dmax, H[i][i]);
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    if (i < first) {
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        H[i][j] = 0.0;
        H[j][i] = 0.0;
      }
      H[i][i] = 1.0;
      g[i] = 0.0;
    }
  }
  // Cholesky H = L L^T, lower triangle in place
  bool ok = isfinite(dmax);
  const double thr = REG_PIVOT_REL * dmax;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = H[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= H[j][k] * H[j][k];
    if (j >= first && !(d > thr)) ok = false;
    const double l = sqrt(ok ? d : 1.0);
    H[j][j] = l;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = H[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= H[i][k] * H[j][k];
      H[i][j] = s / l;
    }
  }
  if (!ok) {
    status[b] = 3;
    return;
  }
  double y[6], x[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = -g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= H[i][k] * y[k];
    y[i] = s / H[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s -= H[k][i] * x[k];
    x[i] = s / H[i][i];
  }
  bool fin = true;
#pragma unroll
  for (int i = 0; i < 6; ++i) fin = fin && isfinite(x[i]);
  if (!fin) {
    status[b] = 3;
    return;
  }
  // exp(delta): R = I + A K + B K^2, t = (I + B K + C K^2) v, K = [omega]x
  const double ox = x[0], oy = x[1], oz = x[2], vx = x[3], vy = x[4], vz = x[5];
  const double th2 = ox * ox + oy * oy + oz * oz, th = sqrt(th2);
  double A, Bc, C;
  if (th < REG_SERIES_THETA) {
    A = 1.0 + th2 * (-1.0 / 6.0 + th2 * (1.0 / 120.0 - th2 / 5040.0));
    Bc = 0.5 + th2 * (-1.0 / 24.0 + th2 * (1.0 / 720.0 - th2 / 40320.0));
    C = 1.0 / 6.0 + th2 * (-1.0 / 120.0 + th2 * (1.0 / 5040.0 - th2 / 362880.0));
  } else {
    const double sn = sin(th), sh = sin(0.5 * th);
    A = sn / th;
    Bc = 2.0 * sh * sh / th2;
    C = (th - sn) / (th2 * th);
  }
  const double K[3][3] = {{0.0, -oz, oy}, {oz, 0.0, -ox}, {-oy, ox, 0.0}};
  double K2[3][3], Rd[3][3], td[3];
  const double vv[3] = {vx, vy, vz};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) K2[i][j] = K[i][0] * K[0][j] + K[i][1] * K[1][j] + K[i][2] * K[2][j];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Rd[i][j] = (i == j ? 1.0 : 0.0) + A * K[i][j] + Bc * K2[i][j];
      s += ((i == j ? 1.0 : 0.0) + Bc * K[i][j] + C * K2[i][j]) * vv[j];
    }
    td[i] = s;
  }
  double* Tb = T + (int64_t)b * 16;
  double Told[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) Told[i] = Tb[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      Tb[i * 4 + j] = Rd[i][0] * Told[j] + Rd[i][1] * Told[4 + j] + Rd[i][2] * Told[8 + j] + (j == 3 ? td[i] : 0.0);
  }
  Tb[12] = 0.0;
  Tb[13] = 0.0;
  Tb[14] = 0.0;
  Tb[15] = 1.0;
  lg[2] = (float)th;
  lg[3] = (float)sqrt(vx * vx + vy * vy + vz * vz);
  status[b] = 0;
}

inline bool reg_pos_finite(float v) { return isfinite(v) && v > 0.f; }

}  // namespace

extern "C" int64_t df_reg_ws_bytes(int B, int Ns) {
  if (!nn_rows_ok(B, Ns) || B > 65535) return DF_E_SHAPE;
  return (int64_t)B * ((Ns + 255) / 256) * REG_SLAB * 8;
}

extern "C" int df_reg_accumulate(const int32_t* src_rng, const float* src_sorted, int Gs, const int32_t* dst_rng, const float* dst_sorted,
                                 float minx, float miny, float cell, int G, int B, int Ns, int stride, const double* T, float max_dist2,
                                 float k2, double* partial, float* q_out, int32_t* idx_out, float* d2_out, float* w_out, void* stream) {
  DF_REQUIRE(src_rng && src_sorted && dst_rng && dst_sorted && T && partial, DF_E_ARG);
  DF_REQUIRE(nn_rows_ok(B, Ns) && nn_grid_ok(B, G) && nn_grid_ok(B, Gs) && B <= 65535, DF_E_SHAPE);
  DF_REQUIRE(isfinite(minx) && isfinite(miny) && reg_pos_finite(cell) && reg_pos_finite(max_dist2) && reg_pos_finite(k2), DF_E_ARG);
  DF_REQUIRE(stride >= 1 && stride <= 1024, DF_E_ARG);
  DF_REQUIRE(df_aligned16(src_sorted) && df_aligned16(dst_sorted) && (((uintptr_t)partial | (uintptr_t)T) & 7u) == 0, DF_E_ALIGN);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (q_out || idx_out || d2_out || w_out) {
    const int64_t n = (int64_t)B * Ns;
    hipLaunchKernelGGL(reg_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, q_out, idx_out, d2_out, w_out);
    DF_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(reg_accumulate_kernel, dim3((Ns + 255) / 256, B), dim3(256), 0, s, src_rng, reinterpret_cast<const f32x4*>(src_sorted),
                     Gs, dst_rng, reinterpret_cast<const f32x4*>(dst_sorted), minx, miny, cell, G, Ns, stride, T, max_dist2, k2, partial,
                     q_out, idx_out, d2_out, w_out);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

extern "C" int df_reg_accumulate_plane(const int32_t* src_rng, const float* src_sorted, int Gs, const int32_t* dst_rng,
                                       const float* dst_sorted, const float* dst_normals, float minx, float miny, float cell, int G, int B,
                                       int Ns, int Nd, int stride, const double* T, float max_dist2, float k2, double* partial, float* q_out,
                                       int32_t* idx_out, float* d2_out, float* w_out, float* e_out, void* stream) {
  DF_REQUIRE(src_rng && src_sorted && dst_rng && dst_sorted && dst_normals && T && partial, DF_E_ARG);
  DF_REQUIRE(nn_rows_ok(B, Ns) && nn_rows_ok(B, Nd) && nn_grid_ok(B, G) && nn_grid_ok(B, Gs) && B <= 65535, DF_E_SHAPE);
  DF_REQUIRE(isfinite(minx) && isfinite(miny) && reg_pos_finite(cell) && reg_pos_finite(max_dist2) && reg_pos_finite(k2), DF_E_ARG);
  DF_REQUIRE(stride >= 1 && stride <= 1024, DF_E_ARG);
  DF_REQUIRE(df_aligned16(src_sorted) && df_aligned16(dst_sorted) && df_aligned16(dst_normals) &&
                 (((uintptr_t)partial | (uintptr_t)T) & 7u) == 0,
             DF_E_ALIGN);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (q_out || idx_out || d2_out || w_out || e_out) {
    const int64_t n = (int64_t)B * Ns;
    hipLaunchKernelGGL(reg_fill_plane_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, q_out, idx_out, d2_out, w_out, e_out);
    DF_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(reg_accumulate_plane_kernel, dim3((Ns + 255) / 256, B), dim3(256), 0, s, src_rng,
                     reinterpret_cast<const f32x4*>(src_sorted), Gs, dst_rng, reinterpret_cast<const f32x4*>(dst_sorted),
                     reinterpret_cast<const f32x4*>(dst_normals), minx, miny, cell, G, Ns, Nd, stride, T, max_dist2, k2, partial, q_out,
                     idx_out, d2_out, w_out, e_out);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

extern "C" int df_reg_solve(const double* partial, int B, int nblk, int min_inliers, int planar, double* T, float* log, int32_t* status,
                            void* stream) {
  DF_REQUIRE(partial && log && (status || !T), DF_E_ARG);
  DF_REQUIRE(B >= 1 && B <= 65535 && nblk >= 1 && (int64_t)B * nblk < 0x3fffffffll, DF_E_SHAPE);
  DF_REQUIRE(min_inliers >= 0, DF_E_ARG);
  DF_REQUIRE((((uintptr_t)partial | (uintptr_t)T) & 7u) == 0 && (((uintptr_t)log | (uintptr_t)status) & 3u) == 0, DF_E_ALIGN);
  hipLaunchKernelGGL(reg_solve_kernel, dim3(B), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), partial, nblk, min_inliers, planar, T,
                     log, status);
  DF_CHECK_LAUNCH();
  return DF_OK;
}
