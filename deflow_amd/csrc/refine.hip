// Per-cluster rigid snap of a model's flow (the refine command): one robust yaw + translation per cluster of the first sweep, fitted to the
// flow the model produced, checked against the second sweep and written back to the cluster's rows.  UNPINNED -- the recipe is the rigid
// refinement of Chodosh et al. (WACV'24), but no upstream source was read; every choice is this project's own and is written down in
// include/deflow_amd.h and DESIGN.md section 6p, so that tests/helpers/refine_ref.py can restate it.  The labels come from cluster.hip, the
// ordered row lists from df_rigid_segments (N0 = Nc, N1 = 1: list 2k holds the rows of cluster k + 1 in ascending order, seg_rows has
// Nc + 1 entries per sample).
//
//   df_refine_fit    one workgroup per (sample, slot); an empty or too large list leaves at once.  iters + 1 weighted fits in one launch,
//                    the rows re-read from global memory in every pass (a cluster of 8192 rows does not fit in LDS as s and d) and the
//                    Huber weights recomputed from the previous fit's transform, so there is no workspace.  Two passes per fit (weighted
//                    means; centred cross and dot sums), one more pass for the residuals of the last fit.
//   df_refine_score  one workgroup per (sample, slot): the means of the truncated nearest-neighbour distances before and after over the
//                    participating rows of a status 1 / 6 slot, and the status rewritten to 7 where the snap made them worse.
//   df_refine_apply  one thread per row: flow_out and rigid_id, every element written exactly once; rows that get no motion copy f's bits.
// Every sum runs in a fixed order: a thread adds its list positions tid, tid + 256, ... in ascending order, the 64 lanes of a wave are added
// in an xor butterfly (32, 16, ..., 1), then waves 0..3 in order.  No float atomics; every loop's trip count comes from a clamped integer.
#include <math.h>

#include "common.h"

namespace {

constexpr int RF_THREADS = 256;
constexpr int RF_COLS = 12;                   // theta, tx, ty, tz, inlier_frac, rms, rows used, status, c_before, c_after, 0, 0

inline bool rf_dims_ok(int B, int Nc) { return B >= 1 && B <= 65535 && Nc >= 1 && (int64_t)B * Nc < 0x80000000ll; }
inline bool rf_pos(float v) { return isfinite(v) && v > 0.f; }
inline bool rf_nonneg(float v) { return isfinite(v) && v >= 0.f; }
inline bool rf_al4(const void* p) { return (((uintptr_t)p) & 3u) == 0; }

struct RfSeg {
  int lo, n;                                  // the list's start inside seg_rows[b] and its length
};
__device__ __forceinline__ RfSeg rf_seg(const int32_t* __restrict__ seg_off, int b, int k, int Kcap, int Nc) {
  const int32_t* o = seg_off + (int64_t)b * (2 * Kcap + 1) + 2 * k;
  const int a = min(max(o[0], 0), Nc), e = min(max(o[1], a), Nc);
  RfSeg s;
  s.lo = a;
  s.n = e - a;
  return s;
}

__device__ __forceinline__ bool rf_fin3(const float* __restrict__ p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }
// does row r of the sample at x / f take part: inside the count, x and f finite (no address is formed from a row outside [0, n))
__device__ __forceinline__ bool rf_takes_part(const float* __restrict__ x, const float* __restrict__ f, int r, int n) {
  return r >= 0 && r < n && rf_fin3(x + (int64_t)r * 3) && rf_fin3(f + (int64_t)r * 3);
}

struct RfPair {
  float sx, sy, sz, dx, dy, dz;               // s = fp32(x - a), d = fp32(s + f)
};
__device__ __forceinline__ RfPair rf_pair(const float* __restrict__ x, const float* __restrict__ f, int r, float ax, float ay, float az) {
  const float* px = x + (int64_t)r * 3;
  const float* pf = f + (int64_t)r * 3;
  RfPair p;
  p.sx = __fsub_rn(px[0], ax);
  p.sy = __fsub_rn(px[1], ay);
  p.sz = __fsub_rn(px[2], az);
  p.dx = __fadd_rn(p.sx, pf[0]);
  p.dy = __fadd_rn(p.sy, pf[1]);
  p.dz = __fadd_rn(p.sz, pf[2]);
  return p;
}
// |Rz(theta) s + t - d|^2 with every product and sum rounded on its own (section 6j(d)'s p and d2)
__device__ __forceinline__ float rf_res2(const RfPair& p, float c, float sn, float tx, float ty, float tz) {
  const float qx = __fadd_rn(__fsub_rn(__fmul_rn(c, p.sx), __fmul_rn(sn, p.sy)), tx);
  const float qy = __fadd_rn(__fadd_rn(__fmul_rn(sn, p.sx), __fmul_rn(c, p.sy)), ty);
  const float qz = __fadd_rn(p.sz, tz);
  const float ex = __fsub_rn(qx, p.dx), ey = __fsub_rn(qy, p.dy), ez = __fsub_rn(qz, p.dz);
  return __fadd_rn(__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)), __fmul_rn(ez, ez));
}
// Huber weight of a residual: 1 up to delta, delta / r beyond (0 for a residual that is not finite)
__device__ __forceinline__ float rf_weight(float d2, float delta) {
  const float r = __fsqrt_rn(d2);
  return r <= delta ? 1.0f : (isfinite(r) ? __fdiv_rn(delta, r) : 0.0f);
}

// K sums over the block in a fixed order: butterfly inside each wave, then waves 0..3; every thread gets the results.  red: 4 K floats
template <int K>
__device__ __forceinline__ void rf_block_sum(float (&v)[K], float* red) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] = __fadd_rn(v[k], __shfl_xor(v[k], o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[(threadIdx.x >> 6) * K + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = __fadd_rn(__fadd_rn(__fadd_rn(red[k], red[K + k]), red[2 * K + k]), red[3 * K + k]);
  __syncthreads();
}
// integer sum and minimum over the block (exact whatever the order)
__device__ __forceinline__ void rf_block_sum_min(int& sum, int& mn, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o, 64);
    mn = min(mn, __shfl_xor(mn, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = sum;
    red[4 + (threadIdx.x >> 6)] = mn;
  }
  __syncthreads();
  sum = red[0] + red[1] + red[2] + red[3];
  mn = min(min(red[4], red[5]), min(red[6], red[7]));
  __syncthreads();
}

struct RfFit {
  int min_rows, max_pts, iters;
  float delta, inlier_dist, min_inlier_frac, max_yaw, max_disp, static_disp, static_yaw;
};

// ---------------------------------------------------------------------------------------------------------------- fit
__global__ __launch_bounds__(RF_THREADS) void rf_fit_kernel(const float* __restrict__ x, const float* __restrict__ f,
                                                            const int32_t* __restrict__ count, const int32_t* __restrict__ seg_off,
                                                            const int32_t* __restrict__ seg_rows, int Nc, int Kcap, RfFit a,
                                                            float* __restrict__ table, int32_t* __restrict__ anchor) {
  __shared__ float red[4 * 7];
  __shared__ int ired[8];
  const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int64_t slot = (int64_t)b * Kcap + k;
  float* out = table + slot * RF_COLS;
  const RfSeg sg = rf_seg(seg_off, b, k, Kcap, Nc);
  if (sg.n == 0 || sg.n > a.max_pts) {                                      // uniform over the block: 0 no rows, 3 too large (not read)
    if (tid < RF_COLS) out[tid] = tid == 6 ? (float)sg.n : (tid == 7 && sg.n > 0) ? 3.0f : 0.0f;
    if (tid == 0) anchor[slot] = -1;
    return;
  }
  const int n = min(max(count[b], 0), Nc);
  const float* xb = x + (int64_t)b * Nc * 3;
  const float* fb = f + (int64_t)b * Nc * 3;
  const int32_t* rows = seg_rows + (int64_t)b * (Nc + 1) + sg.lo;
  // ---- the rows that take part, and the first of them: the anchor
  int np = 0, first = 0x7fffffff;
  for (int j = tid; j < sg.n; j += RF_THREADS) {
    if (rf_takes_part(xb, fb, rows[j], n)) {
      ++np;
      first = min(first, j);
    }
  }
  rf_block_sum_min(np, first, ired);
  if (np < a.min_rows) {                                                    // 2: too few rows take part
    if (tid < RF_COLS) out[tid] = tid == 6 ? (float)np : tid == 7 ? 2.0f : 0.0f;
    if (tid == 0) anchor[slot] = np > 0 ? rows[first] : -1;
    return;
  }
  const int ar = rows[first];
  const float ax = xb[(int64_t)ar * 3], ay = xb[(int64_t)ar * 3 + 1], az = xb[(int64_t)ar * 3 + 2];
  const float fnp = (float)np;
  float th = 0.f, tx = 0.f, ty = 0.f, tz = 0.f;
  for (int it = 0; it <= a.iters; ++it) {
    // the weights of this fit come from the residuals of the previous one (1 in the first)
    const float c = cosf(th), sn = sinf(th);
    float m[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};                       // W, sum w s, sum w d
    for (int j = tid; j < sg.n; j += RF_THREADS) {
      const int r = rows[j];
      if (!rf_takes_part(xb, fb, r, n)) continue;
      const RfPair p = rf_pair(xb, fb, r, ax, ay, az);
      const float w = it == 0 ? 1.0f : rf_weight(rf_res2(p, c, sn, tx, ty, tz), a.delta);
      m[0] = __fadd_rn(m[0], w);
      m[1] = __fadd_rn(m[1], __fmul_rn(w, p.sx));
      m[2] = __fadd_rn(m[2], __fmul_rn(w, p.sy));
      m[3] = __fadd_rn(m[3], __fmul_rn(w, p.sz));
      m[4] = __fadd_rn(m[4], __fmul_rn(w, p.dx));
      m[5] = __fadd_rn(m[5], __fmul_rn(w, p.dy));
      m[6] = __fadd_rn(m[6], __fmul_rn(w, p.dz));
    }
    rf_block_sum<7>(m, red);
    const float msx = __fdiv_rn(m[1], m[0]), msy = __fdiv_rn(m[2], m[0]), msz = __fdiv_rn(m[3], m[0]);
    const float mdx = __fdiv_rn(m[4], m[0]), mdy = __fdiv_rn(m[5], m[0]), mdz = __fdiv_rn(m[6], m[0]);
    float q[2] = {0.f, 0.f};                                                // sum w (u x v), sum w (u . v), in the xy plane
    for (int j = tid; j < sg.n; j += RF_THREADS) {
      const int r = rows[j];
      if (!rf_takes_part(xb, fb, r, n)) continue;
      const RfPair p = rf_pair(xb, fb, r, ax, ay, az);
      const float w = it == 0 ? 1.0f : rf_weight(rf_res2(p, c, sn, tx, ty, tz), a.delta);
      const float ux = __fsub_rn(p.sx, msx), uy = __fsub_rn(p.sy, msy), vx = __fsub_rn(p.dx, mdx), vy = __fsub_rn(p.dy, mdy);
      q[0] = __fadd_rn(q[0], __fmul_rn(w, __fsub_rn(__fmul_rn(ux, vy), __fmul_rn(uy, vx))));
      q[1] = __fadd_rn(q[1], __fmul_rn(w, __fadd_rn(__fmul_rn(ux, vx), __fmul_rn(uy, vy))));
    }
    rf_block_sum<2>(q, red);
    th = atan2f(q[0], q[1]);
    const float c2 = cosf(th), s2 = sinf(th);
    tx = __fsub_rn(mdx, __fsub_rn(__fmul_rn(c2, msx), __fmul_rn(s2, msy)));
    ty = __fsub_rn(mdy, __fadd_rn(__fmul_rn(s2, msx), __fmul_rn(c2, msy)));
    tz = __fsub_rn(mdz, msz);
  }
  // ---- the last fit's residuals: inliers, rms; the unweighted centroid of the rows that take part
  const float c = cosf(th), sn = sinf(th);
  float g[4] = {0.f, 0.f, 0.f, 0.f};                                        // sum r^2, sum s.x, sum s.y, inliers (a count: exact in fp32)
  for (int j = tid; j < sg.n; j += RF_THREADS) {
    const int r = rows[j];
    if (!rf_takes_part(xb, fb, r, n)) continue;
    const RfPair p = rf_pair(xb, fb, r, ax, ay, az);
    const float d2 = rf_res2(p, c, sn, tx, ty, tz);
    g[0] = __fadd_rn(g[0], d2);
    g[1] = __fadd_rn(g[1], p.sx);
    g[2] = __fadd_rn(g[2], p.sy);
    g[3] = __fadd_rn(g[3], __fsqrt_rn(d2) <= a.inlier_dist ? 1.0f : 0.0f);
  }
  rf_block_sum<4>(g, red);
  if (tid == 0) {
    const float cx = __fdiv_rn(g[1], fnp), cy = __fdiv_rn(g[2], fnp);       // (the z of the centroid moves by tz whatever it is)
    const float mx = __fsub_rn(__fadd_rn(__fsub_rn(__fmul_rn(c, cx), __fmul_rn(sn, cy)), tx), cx);
    const float my = __fsub_rn(__fadd_rn(__fadd_rn(__fmul_rn(sn, cx), __fmul_rn(c, cy)), ty), cy);
    const float disp = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(mx, mx), __fmul_rn(my, my)), __fmul_rn(tz, tz)));
    const float frac = __fdiv_rn(g[3], fnp);
    int status = 1;
    if (!(frac >= a.min_inlier_frac)) status = 4;
    else if (!(fabsf(th) <= a.max_yaw) || !(disp <= a.max_disp)) status = 5;
    else if (disp <= a.static_disp && fabsf(th) <= a.static_yaw) status = 6;
    const bool ident = status == 6;                                         // static: the transform becomes the identity
    out[0] = ident ? 0.f : th;
    out[1] = ident ? 0.f : tx;
    out[2] = ident ? 0.f : ty;
    out[3] = ident ? 0.f : tz;
    out[4] = frac;
    out[5] = __fsqrt_rn(__fdiv_rn(g[0], fnp));
    out[6] = fnp;
    out[7] = (float)status;
    out[8] = out[9] = out[10] = out[11] = 0.f;
    anchor[slot] = ar;
  }
}

// ---------------------------------------------------------------------------------------------------------------- score
__device__ __forceinline__ float rf_trunc_dist(float d2, float trunc, float t2) {
  return (d2 >= 0.f && d2 <= t2) ? fminf(__fsqrt_rn(d2), trunc) : trunc;  // a row with no neighbour (inf, NaN) counts as trunc
}

__global__ __launch_bounds__(RF_THREADS) void rf_score_kernel(const float* __restrict__ x, const float* __restrict__ f,
                                                              const int32_t* __restrict__ count, const int32_t* __restrict__ count1,
                                                              const int32_t* __restrict__ seg_off, const int32_t* __restrict__ seg_rows,
                                                              const float* __restrict__ d2_before, const float* __restrict__ d2_after, int Nc,
                                                              int Kcap, float trunc, float tol, float* __restrict__ table) {
  __shared__ float red[4 * 3];
  const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  float* out = table + ((int64_t)b * Kcap + k) * RF_COLS;
  const float st = out[7];                                                  // (thread 0 writes it behind the block sums' barriers)
  const RfSeg sg = rf_seg(seg_off, b, k, Kcap, Nc);
  if (!(st == 1.0f || st == 6.0f) || count1[b] <= 0 || sg.n == 0) {         // uniform over the block; no second sweep: every slot passes
    if (tid == 0) out[8] = out[9] = 0.f;
    return;
  }
  const int n = min(max(count[b], 0), Nc);
  const float* xb = x + (int64_t)b * Nc * 3;
  const float* fb = f + (int64_t)b * Nc * 3;
  const float* db = d2_before + (int64_t)b * Nc;
  const float* da = d2_after + (int64_t)b * Nc;
  const int32_t* rows = seg_rows + (int64_t)b * (Nc + 1) + sg.lo;
  const float t2 = __fmul_rn(trunc, trunc);
  float s[3] = {0.f, 0.f, 0.f};                                             // sum before, sum after, rows (a count: exact in fp32)
  for (int j = tid; j < sg.n; j += RF_THREADS) {
    const int r = rows[j];
    if (!rf_takes_part(xb, fb, r, n)) continue;
    s[0] = __fadd_rn(s[0], rf_trunc_dist(db[r], trunc, t2));
    s[1] = __fadd_rn(s[1], rf_trunc_dist(da[r], trunc, t2));
    s[2] = __fadd_rn(s[2], 1.0f);
  }
  rf_block_sum<3>(s, red);
  if (tid == 0) {
    const float cb = s[2] > 0.f ? __fdiv_rn(s[0], s[2]) : 0.f, ca = s[2] > 0.f ? __fdiv_rn(s[1], s[2]) : 0.f;
    out[8] = cb;
    out[9] = ca;
    if (ca > __fadd_rn(cb, tol)) out[7] = 7.0f;                             // the snap moved the rows away from the second sweep
  }
}

// ---------------------------------------------------------------------------------------------------------------- apply
__global__ __launch_bounds__(256) void rf_apply_kernel(const float* __restrict__ x, const float* __restrict__ f,
                                                       const int32_t* __restrict__ count, const int32_t* __restrict__ labels,
                                                       const float* __restrict__ table, const int32_t* __restrict__ anchor, int Nc, int Kcap,
                                                       float* __restrict__ flow_out, int32_t* __restrict__ rigid_id) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Nc) return;
  const int64_t row = (int64_t)b * Nc + i;
  const uint32_t* fi = reinterpret_cast<const uint32_t*>(f) + row * 3;      // rows that get no motion keep f bit for bit
  uint32_t o0 = fi[0], o1 = fi[1], o2 = fi[2];
  int id = 0;
  const int l = labels[row];
  const int n = min(max(count[b], 0), Nc);
  if (l >= 1 && l <= Kcap && rf_takes_part(x + (int64_t)b * Nc * 3, f + (int64_t)b * Nc * 3, i, n)) {
    const int64_t slot = (int64_t)b * Kcap + (l - 1);
    const float* t = table + slot * RF_COLS;
    const int ar = anchor[slot];
    if (t[7] == 6.0f) {
      o0 = o1 = o2 = 0u;
      id = l;
    } else if (t[7] == 1.0f && ar >= 0 && ar < Nc) {
      const float* s = x + row * 3;
      const float* an = x + ((int64_t)b * Nc + ar) * 3;
      const float c = cosf(t[0]), sn = sinf(t[0]);
      const float rx = __fsub_rn(s[0], an[0]), ry = __fsub_rn(s[1], an[1]);
      o0 = __builtin_bit_cast(uint32_t, __fsub_rn(__fadd_rn(__fsub_rn(__fmul_rn(c, rx), __fmul_rn(sn, ry)), t[1]), rx));
      o1 = __builtin_bit_cast(uint32_t, __fsub_rn(__fadd_rn(__fadd_rn(__fmul_rn(sn, rx), __fmul_rn(c, ry)), t[2]), ry));
      o2 = __builtin_bit_cast(uint32_t, t[3]);
      id = l;
    }
  }
  uint32_t* o = reinterpret_cast<uint32_t*>(flow_out) + row * 3;
  o[0] = o0;
  o[1] = o1;
  o[2] = o2;
  rigid_id[row] = id;
}

}  // namespace

extern "C" int df_refine_fit(const float* x, const float* flow, const int32_t* count, const int32_t* seg_off, const int32_t* seg_rows, int B,
                             int Nc, int Kcap, int min_rows, int max_cluster_points, int iters, float delta, float inlier_dist,
                             float min_inlier_frac, float max_yaw, float max_disp, float static_disp, float static_yaw, float* table,
                             int32_t* anchor, void* stream) {
  DF_REQUIRE(x && flow && count && seg_off && seg_rows && table && anchor, DF_E_ARG);
  DF_REQUIRE(rf_dims_ok(B, Nc), DF_E_SHAPE);
  DF_REQUIRE(Kcap >= 1 && Kcap <= Nc && iters >= 0 && iters <= 64 && min_rows >= 1 && max_cluster_points >= 1, DF_E_ARG);
  DF_REQUIRE(rf_pos(delta) && rf_pos(inlier_dist) && rf_nonneg(min_inlier_frac) && rf_nonneg(max_yaw) && rf_nonneg(max_disp) &&
                 rf_nonneg(static_disp) && rf_nonneg(static_yaw),
             DF_E_ARG);
  DF_REQUIRE(rf_al4(x) && rf_al4(flow) && rf_al4(count) && rf_al4(seg_off) && rf_al4(seg_rows) && rf_al4(table) && rf_al4(anchor), DF_E_ALIGN);
  RfFit a;
  a.min_rows = min_rows;
  a.max_pts = max_cluster_points;
  a.iters = iters;
  a.delta = delta;
  a.inlier_dist = inlier_dist;
  a.min_inlier_frac = min_inlier_frac;
  a.max_yaw = max_yaw;
  a.max_disp = max_disp;
  a.static_disp = static_disp;
  a.static_yaw = static_yaw;
  hipLaunchKernelGGL(rf_fit_kernel, dim3(Kcap, B), dim3(RF_THREADS), 0, reinterpret_cast<hipStream_t>(stream), x, flow, count, seg_off,
                     seg_rows, Nc, Kcap, a, table, anchor);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

extern "C" int df_refine_score(const float* x, const float* flow, const int32_t* count, const int32_t* count1, const int32_t* seg_off,
                               const int32_t* seg_rows, const float* d2_before, const float* d2_after, int B, int Nc, int Kcap,
                               float check_trunc, float check_tol, float* table, void* stream) {
  DF_REQUIRE(x && flow && count && count1 && seg_off && seg_rows && d2_before && d2_after && table, DF_E_ARG);
  DF_REQUIRE(rf_dims_ok(B, Nc), DF_E_SHAPE);
  DF_REQUIRE(Kcap >= 1 && Kcap <= Nc && rf_pos(check_trunc) && rf_nonneg(check_tol), DF_E_ARG);
  DF_REQUIRE(rf_al4(x) && rf_al4(flow) && rf_al4(count) && rf_al4(count1) && rf_al4(seg_off) && rf_al4(seg_rows) && rf_al4(d2_before) &&
                 rf_al4(d2_after) && rf_al4(table),
             DF_E_ALIGN);
  hipLaunchKernelGGL(rf_score_kernel, dim3(Kcap, B), dim3(RF_THREADS), 0, reinterpret_cast<hipStream_t>(stream), x, flow, count, count1,
                     seg_off, seg_rows, d2_before, d2_after, Nc, Kcap, check_trunc, check_tol, table);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

extern "C" int df_refine_apply(const float* x, const float* flow, const int32_t* count, const int32_t* labels, const float* table,
                               const int32_t* anchor, int B, int Nc, int Kcap, float* flow_out, int32_t* rigid_id, void* stream) {
  DF_REQUIRE(x && flow && count && labels && table && anchor && flow_out && rigid_id, DF_E_ARG);
  DF_REQUIRE(rf_dims_ok(B, Nc), DF_E_SHAPE);
  DF_REQUIRE(Kcap >= 1 && Kcap <= Nc, DF_E_ARG);
  DF_REQUIRE(rf_al4(x) && rf_al4(flow) && rf_al4(count) && rf_al4(labels) && rf_al4(table) && rf_al4(anchor) && rf_al4(flow_out) &&
                 rf_al4(rigid_id),
             DF_E_ALIGN);
  hipLaunchKernelGGL(rf_apply_kernel, dim3((Nc + 255) / 256, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, flow, count, labels,
                     table, anchor, Nc, Kcap, flow_out, rigid_id);
  DF_CHECK_LAUNCH();
  return DF_OK;
}
