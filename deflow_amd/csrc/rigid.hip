// Training-free rigid cluster flow (model=icpflow): per-cluster registration of the first sweep onto the second.  UNPINNED -- upstream's
// ICP-Flow source is absent; every choice is this project's own and is written down in include/deflow_amd.h and DESIGN.md section 6j, so
// that tests/helpers/rigid_ref.py can restate it.  The joint DBSCAN labels of the concatenated rows (pc0s rows first, then pc1 rows) come
// from cluster.hip; cluster slot k = label - 1, list 2k holds its source rows (from pc0s), list 2k + 1 its target rows (from pc1).
//
//   df_rigid_segments  the ordered row lists.  (a) rg_count_kernel, one thread per row: integer atomic add into cnt[b][list] (a count
//                      does not depend on the order it is taken in); (b) rg_scan_kernel, one block per sample: exclusive scan of the
//                      2 Kcap counts -> seg_off, and the running cursor of every list; (c) rg_rank_kernel, one block per tile of 1024
//                      rows: the number of earlier rows of the tile in the same list, and of all of them (counted in LDS);
//                      (d) rg_scatter_kernel, one block per sample walking the tiles IN ORDER: a row's place is its list's cursor plus
//                      that rank, then the first row of every list in the tile moves the cursor on.  One block owns the cursors, so
//                      the lists are stable whatever the launch order.
//   df_rigid_vote      one workgroup per (sample, slot): (2R+1)^2 integer counters in LDS, every used (source, target) pair adds one to
//                      the bin of its rounded xy difference with an LDS integer atomic; block-wide arg-max on (count, lowest bin).
//   df_rigid_icp       one workgroup per (sample, slot): icp_iters + 1 nearest-neighbour passes in one launch; target rows staged in LDS
//                      tiles of float4 (x, y, z relative to the anchor), one source row per lane per pass;
//                      the matches go to a workspace, the closed-form yaw + translation update is reduced in a fixed tree order.
//   df_rigid_apply     one thread per pc0s row: flow and rigid_id, every element written exactly once.
// No float atomics anywhere; every loop's trip count comes from a clamped integer.
#include <math.h>

#include "common.h"

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_SCAT = 1024;                 // rows per tile of the scatter pass (= its block size)
constexpr int RG_RMAX = 64;                   // vote radius in bins: (2 * 64 + 1)^2 counters = 66564 bytes of LDS at most

inline bool rg_dims_ok(int B, int N0, int N1, int Kcap) {
  return B >= 1 && B <= 65535 && N0 >= 1 && N1 >= 1 && (int64_t)B * ((int64_t)N0 + N1) < 0x80000000ll && Kcap >= 1 &&
         (int64_t)Kcap <= (int64_t)N0 + N1 && (int64_t)B * (2 * (int64_t)Kcap + 1) < 0x80000000ll;
}
inline int64_t rg_al16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// ---------------------------------------------------------------------------------------------------------------- segments
__device__ __forceinline__ int rg_list(int label, int row, int N0, int Kcap) {
  return (label >= 1 && label <= Kcap) ? 2 * (label - 1) + (row >= N0 ? 1 : 0) : -1;
}

__global__ __launch_bounds__(256) void rg_count_kernel(const int32_t* __restrict__ labels, int N0, int N, int Kcap, int32_t* __restrict__ cnt,
                                                       int32_t* __restrict__ status) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int l = labels[(int64_t)b * N + i];
  const int k = rg_list(l, i, N0, Kcap);
  if (k >= 0) atomicAdd(cnt + (int64_t)b * 2 * Kcap + k, 1);
  else if (l != 0) atomicAdd(status, 1);            // a label outside [0, Kcap]: not one of cluster.hip's
}

// seg_off[b][0 .. 2 Kcap] = exclusive scan of cnt[b][.]; cnt[b][.] becomes the cursor (= the list's start)
__global__ __launch_bounds__(256) void rg_scan_kernel(int Kcap, int N, int32_t* __restrict__ cnt, int32_t* __restrict__ seg_off) {
  __shared__ int wsum[4];
  __shared__ int carry;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, L = 2 * Kcap;
  int32_t* c = cnt + (int64_t)b * L;
  int32_t* o = seg_off + (int64_t)b * (L + 1);
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < L; base += 256) {
    const int k = base + tid;
    const int v = k < L ? min(max(c[k], 0), N) : 0;
    int s = v;                                       // inclusive scan inside the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(s, d, 64);
      if (lane >= d) s += t;
    }
    if (lane == 63) wsum[w] = s;
    __syncthreads();
    int pre = carry;
    for (int q = 0; q < w; ++q) pre += wsum[q];
    const int excl = min(pre + s - v, N);
    if (k < L) {
      o[k] = excl;
      c[k] = excl;
    }
    __syncthreads();
    if (tid == 255) carry = min(pre + s, N);
    __syncthreads();
  }
  if (tid == 0) o[L] = carry;
}

__device__ __forceinline__ int rg_ld(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void rg_st(int32_t* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// rank[b][i] = (rows of the tile in i's list) << 16 | (those of them before i), -1 for a row of no list: the all-pairs part of the
// scatter, one block per tile of RG_SCAT rows, all tiles at once
__global__ __launch_bounds__(RG_SCAT) void rg_rank_kernel(const int32_t* __restrict__ labels, int N0, int N, int Kcap,
                                                          int32_t* __restrict__ rank) {
  __shared__ int keys[RG_SCAT];
  const int b = blockIdx.y, tid = threadIdx.x, i = blockIdx.x * RG_SCAT + tid;
  const int k = i < N ? rg_list(labels[(int64_t)b * N + i], i, N0, Kcap) : -1;
  keys[tid] = k;
  __syncthreads();
  if (i >= N) return;
  int before = 0, total = 0;
  if (k >= 0) {
    for (int j = 0; j < RG_SCAT; ++j) {
      const int same = keys[j] == k ? 1 : 0;
      total += same;
      before += j < tid ? same : 0;
    }
  }
  rank[(int64_t)b * N + i] = k >= 0 ? (total << 16) | before : -1;
}

// the ordered part: one block per sample walks the tiles in order; a row's place is its list's cursor plus its rank inside the tile,
// then the first row of every list in the tile moves that cursor past the tile's rows
__global__ __launch_bounds__(RG_SCAT) void rg_scatter_kernel(const int32_t* __restrict__ labels, int N0, int N, int Kcap,
                                                             const int32_t* __restrict__ seg_off, const int32_t* __restrict__ rank,
                                                             int32_t* __restrict__ cursor, int32_t* __restrict__ seg_rows,
                                                             int32_t* __restrict__ status) {
  const int b = blockIdx.x, tid = threadIdx.x, L = 2 * Kcap;
  const int32_t* lab = labels + (int64_t)b * N;
  const int32_t* rk = rank + (int64_t)b * N;
  int32_t* cur = cursor + (int64_t)b * L;
  const int32_t* off = seg_off + (int64_t)b * (L + 1);
  int32_t* rows = seg_rows + (int64_t)b * N;
  for (int base = 0; base < N; base += RG_SCAT) {
    const int i = base + tid;
    const int k = i < N ? rg_list(lab[i], i, N0, Kcap) : -1;
    const int r = k >= 0 ? rk[i] : -1;
    int start = 0;
    if (r >= 0) {
      start = rg_ld(cur + k);
      const int at = start + (r & 0xffff);
      if (at >= off[k] && at < off[k + 1] && at < N) rows[at] = i;
      else atomicAdd(status, 1);
    }
    __syncthreads();                                 // every cursor of the tile has been read
    if (r >= 0 && (r & 0xffff) == 0) rg_st(cur + k, start + (r >> 16));
    __threadfence_block();
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------- shared by vote / icp
struct RgSeg {
  int s_lo, ns, d_lo, nd;                            // list starts inside seg_rows[b] and lengths
};
__device__ __forceinline__ RgSeg rg_seg(const int32_t* __restrict__ seg_off, int b, int k, int Kcap, int N) {
  const int32_t* o = seg_off + (int64_t)b * (2 * Kcap + 1) + 2 * k;
  const int a = min(max(o[0], 0), N), m = min(max(o[1], a), N), e = min(max(o[2], m), N);
  RgSeg s;
  s.s_lo = a;
  s.ns = m - a;
  s.d_lo = m;
  s.nd = e - m;
  return s;
}
// 0 empty, 2 one-sided, 3 too large, -1: to be registered
__device__ __forceinline__ int rg_pre_status(const RgSeg& s, int min_side, int max_pts) {
  if (s.ns + s.nd == 0) return 0;
  if (s.ns < min_side || s.nd < min_side) return 2;
  if (s.ns + s.nd > max_pts) return 3;
  return -1;
}
// position in the ordered list of the j-th used row: all rows up to cap, else rows j * n / cap
__device__ __forceinline__ int rg_pick(int j, int n, int cap) { return n > cap ? (int)(((int64_t)j * n) / cap) : j; }

struct RgP {
  float x, y, z;
};
// row r of the concatenation (pc0s rows, then pc1 rows); a row outside it reads as NaN and then takes no part
__device__ __forceinline__ RgP rg_point(const float* __restrict__ p0, const float* __restrict__ p1, int b, int r, int N0, int N1) {
  RgP p = {NAN, NAN, NAN};
  const float* q = nullptr;
  if (r >= 0 && r < N0) q = p0 + ((int64_t)b * N0 + r) * 3;
  else if (r >= N0 && r < N0 + N1) q = p1 + ((int64_t)b * N1 + (r - N0)) * 3;
  if (q) {
    p.x = q[0];
    p.y = q[1];
    p.z = q[2];
  }
  return p;
}

// ---------------------------------------------------------------------------------------------------------------- vote
__global__ __launch_bounds__(RG_THREADS) void rg_vote_kernel(const float* __restrict__ pc0s, const float* __restrict__ pc1,
                                                             const int32_t* __restrict__ seg_off, const int32_t* __restrict__ seg_rows,
                                                             int N0, int N1, int Kcap, int min_side, int max_pts, int vote_cap,
                                                             float vote_bin, int R, int32_t* __restrict__ vote, int32_t* __restrict__ hist) {
  extern __shared__ unsigned char rg_lds[];
  const int W = 2 * R + 1, NB = W * W;
  int* bins = reinterpret_cast<int*>(rg_lds);                              // [NB]
  float* tx = reinterpret_cast<float*>(bins + NB);                         // [RG_THREADS] target tile
  float* ty = tx + RG_THREADS;
  unsigned long long* red = reinterpret_cast<unsigned long long*>(rg_lds + (((size_t)(NB + 2 * RG_THREADS) * 4 + 7) & ~(size_t)7));
  const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, N = N0 + N1;
  const int64_t slot = (int64_t)b * Kcap + k;
  const RgSeg sg = rg_seg(seg_off, b, k, Kcap, N);
  if (rg_pre_status(sg, min_side, max_pts) >= 0) {                         // uniform over the block
    if (tid < 3) vote[slot * 3 + tid] = 0;
    if (hist)
      for (int i = tid; i < NB; i += RG_THREADS) hist[slot * NB + i] = 0;
    return;
  }
  const int32_t* rows = seg_rows + (int64_t)b * N;
  for (int i = tid; i < NB; i += RG_THREADS) bins[i] = 0;
  const int us = min(sg.ns, vote_cap), ud = min(sg.nd, vote_cap);
  const float fR = (float)R;
  for (int s0 = 0; s0 < us; s0 += RG_THREADS) {
    const int js = s0 + tid;
    RgP s = {NAN, NAN, NAN};
    if (js < us) s = rg_point(pc0s, pc1, b, rows[sg.s_lo + rg_pick(js, sg.ns, vote_cap)], N0, N1);
    for (int d0 = 0; d0 < ud; d0 += RG_THREADS) {
      __syncthreads();                                                     // the previous tile has been read (and the bins are zero)
      const int jd = d0 + tid;
      RgP d = {NAN, NAN, NAN};
      if (jd < ud) d = rg_point(pc0s, pc1, b, rows[sg.d_lo + rg_pick(jd, sg.nd, vote_cap)], N0, N1);
      tx[tid] = d.x;
      ty[tid] = d.y;
      __syncthreads();
      const int nt = min(RG_THREADS, ud - d0);
      for (int j = 0; j < nt; ++j) {
        const float qx = floorf(__fadd_rn(__fdiv_rn(__fsub_rn(tx[j], s.x), vote_bin), 0.5f));
        const float qy = floorf(__fadd_rn(__fdiv_rn(__fsub_rn(ty[j], s.y), vote_bin), 0.5f));
        if (fabsf(qx) <= fR && fabsf(qy) <= fR)                            // false for NaN: rows that are absent or not finite
          atomicAdd(bins + ((int)qy + R) * W + ((int)qx + R), 1);
      }
    }
  }
  __syncthreads();
  // arg-max on (count, lowest bin): one 64-bit key per thread, tree over the block
  unsigned long long best = 0;
  for (int i = tid; i < NB; i += RG_THREADS) {
    const unsigned long long key = ((unsigned long long)(unsigned)bins[i] << 32) | (unsigned)(0x7fffffff - i);
    best = key > best ? key : best;
    if (hist) hist[slot * NB + i] = bins[i];
  }
  red[tid] = best;
  __syncthreads();
  for (int o = RG_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] = red[tid + o] > red[tid] ? red[tid + o] : red[tid];
    __syncthreads();
  }
  if (tid == 0) {
    const unsigned long long key = red[0];
    const int cnt = (int)(key >> 32), idx = 0x7fffffff - (int)(key & 0xffffffffu);
    vote[slot * 3 + 0] = cnt > 0 ? idx % W - R : 0;
    vote[slot * 3 + 1] = cnt > 0 ? idx / W - R : 0;
    vote[slot * 3 + 2] = cnt;
  }
}

// ---------------------------------------------------------------------------------------------------------------- icp
// sum over the block in a fixed order: butterfly inside each wave, then waves 0..3; every thread gets the result.  red: 4 floats of LDS
__device__ __forceinline__ float rg_block_sum(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float s = __fadd_rn(__fadd_rn(__fadd_rn(red[0], red[1]), red[2]), red[3]);
  __syncthreads();
  return s;
}

struct RgIcp {
  int icp_cap, icp_iters;
  float vote_bin, max_dist, min_inlier_frac, max_yaw, max_disp;
};

__global__ __launch_bounds__(RG_THREADS) void rg_icp_kernel(const float* __restrict__ pc0s, const float* __restrict__ pc1,
                                                            const int32_t* __restrict__ seg_off, const int32_t* __restrict__ seg_rows,
                                                            const int32_t* __restrict__ vote, int N0, int N1, int Kcap, int min_side,
                                                            int max_pts, RgIcp a, float* __restrict__ table, int32_t* __restrict__ match_ws) {
  __shared__ f32x4 tile[RG_THREADS];
  __shared__ float red[4];
  const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, N = N0 + N1;
  const int64_t slot = (int64_t)b * Kcap + k;
  const RgSeg sg = rg_seg(seg_off, b, k, Kcap, N);
  float* out = table + slot * 8;
  int st = rg_pre_status(sg, min_side, max_pts);
  const int vcnt = vote[slot * 3 + 2];
  if (st < 0 && vcnt <= 0) st = 5;                                          // no pair within max_disp
  if (st >= 0) {
    if (tid == 0) {
      out[0] = out[1] = out[2] = out[3] = out[4] = 0.f;
      out[5] = (float)sg.ns;
      out[6] = (float)sg.nd;
      out[7] = (float)st;
    }
    return;
  }
  const int32_t* rows = seg_rows + (int64_t)b * N;
  int32_t* match = match_ws + (int64_t)b * N + sg.s_lo;                     // one entry per used source row: the clusters' lists are disjoint
  const int us = min(sg.ns, a.icp_cap), ud = min(sg.nd, a.icp_cap);
  const RgP an = rg_point(pc0s, pc1, b, rows[sg.s_lo], N0, N1);             // the anchor: the cluster's first source row
  float th = 0.f, tx = __fmul_rn((float)vote[slot * 3 + 0], a.vote_bin), ty = __fmul_rn((float)vote[slot * 3 + 1], a.vote_bin), tz = 0.f;
  const float md2 = __fmul_rn(a.max_dist, a.max_dist);
  int inl_total = 0;
  for (int it = 0; it <= a.icp_iters; ++it) {
    const float c = cosf(th), s = sinf(th);
    // ---- nearest used target row of every used source row under the current transform
    int inl = 0;
    for (int s0 = 0; s0 < us; s0 += RG_THREADS) {
      const int js = s0 + tid;
      float px = NAN, py = NAN, pz = NAN;
      if (js < us) {
        const RgP p = rg_point(pc0s, pc1, b, rows[sg.s_lo + rg_pick(js, sg.ns, a.icp_cap)], N0, N1);
        const float rx = __fsub_rn(p.x, an.x), ry = __fsub_rn(p.y, an.y), rz = __fsub_rn(p.z, an.z);
        px = __fadd_rn(__fsub_rn(__fmul_rn(c, rx), __fmul_rn(s, ry)), tx);
        py = __fadd_rn(__fadd_rn(__fmul_rn(s, rx), __fmul_rn(c, ry)), ty);
        pz = __fadd_rn(rz, tz);
      }
      float best = INFINITY;
      int bj = -1;
      for (int d0 = 0; d0 < ud; d0 += RG_THREADS) {
        __syncthreads();
        const int jd = d0 + tid;
        f32x4 t = {NAN, NAN, NAN, 0.f};
        if (jd < ud) {
          const RgP d = rg_point(pc0s, pc1, b, rows[sg.d_lo + rg_pick(jd, sg.nd, a.icp_cap)], N0, N1);
          t.x = __fsub_rn(d.x, an.x);
          t.y = __fsub_rn(d.y, an.y);
          t.z = __fsub_rn(d.z, an.z);
        }
        tile[tid] = t;
        __syncthreads();
        const int nt = min(RG_THREADS, ud - d0);
        for (int j = 0; j < nt; ++j) {
          const f32x4 q = tile[j];
          const float dx = __fsub_rn(px, q.x), dy = __fsub_rn(py, q.y), dz = __fsub_rn(pz, q.z);
          const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
          if (d2 < best) {                                                  // ascending j: the lowest row wins on equal distance
            best = d2;
            bj = d0 + j;
          }
        }
      }
      const bool in = js < us && bj >= 0 && best <= md2;
      if (js < us) match[js] = in ? bj : -1;
      inl += in ? 1 : 0;
    }
    const int n_in = (int)rg_block_sum((float)inl, red);                    // (counts up to icp_cap <= 2^24: exact in fp32)
    inl_total = n_in;
    if (it == a.icp_iters) break;
    if (n_in < 3) continue;                                                 // the transform stays as it is
    // ---- means of the inlier pairs, relative to the anchor
    float sx = 0.f, sy = 0.f, sz = 0.f, ex = 0.f, ey = 0.f, ez = 0.f;
    for (int js = tid; js < us; js += RG_THREADS) {
      const int m = match[js];
      if (m < 0 || m >= ud) continue;
      const RgP p = rg_point(pc0s, pc1, b, rows[sg.s_lo + rg_pick(js, sg.ns, a.icp_cap)], N0, N1);
      const RgP d = rg_point(pc0s, pc1, b, rows[sg.d_lo + rg_pick(m, sg.nd, a.icp_cap)], N0, N1);
      sx = __fadd_rn(sx, __fsub_rn(p.x, an.x));
      sy = __fadd_rn(sy, __fsub_rn(p.y, an.y));
      sz = __fadd_rn(sz, __fsub_rn(p.z, an.z));
      ex = __fadd_rn(ex, __fsub_rn(d.x, an.x));
      ey = __fadd_rn(ey, __fsub_rn(d.y, an.y));
      ez = __fadd_rn(ez, __fsub_rn(d.z, an.z));
    }
    const float fn = (float)n_in;
    const float msx = __fdiv_rn(rg_block_sum(sx, red), fn), msy = __fdiv_rn(rg_block_sum(sy, red), fn), msz = __fdiv_rn(rg_block_sum(sz, red), fn);
    const float mdx = __fdiv_rn(rg_block_sum(ex, red), fn), mdy = __fdiv_rn(rg_block_sum(ey, red), fn), mdz = __fdiv_rn(rg_block_sum(ez, red), fn);
    // ---- yaw from the centred pairs
    float cr = 0.f, dt = 0.f;
    for (int js = tid; js < us; js += RG_THREADS) {
      const int m = match[js];
      if (m < 0 || m >= ud) continue;
      const RgP p = rg_point(pc0s, pc1, b, rows[sg.s_lo + rg_pick(js, sg.ns, a.icp_cap)], N0, N1);
      const RgP d = rg_point(pc0s, pc1, b, rows[sg.d_lo + rg_pick(m, sg.nd, a.icp_cap)], N0, N1);
      const float ux = __fsub_rn(__fsub_rn(p.x, an.x), msx), uy = __fsub_rn(__fsub_rn(p.y, an.y), msy);
      const float vx = __fsub_rn(__fsub_rn(d.x, an.x), mdx), vy = __fsub_rn(__fsub_rn(d.y, an.y), mdy);
      cr = __fadd_rn(cr, __fsub_rn(__fmul_rn(ux, vy), __fmul_rn(uy, vx)));
      dt = __fadd_rn(dt, __fadd_rn(__fmul_rn(ux, vx), __fmul_rn(uy, vy)));
    }
    const float scr = rg_block_sum(cr, red), sdt = rg_block_sum(dt, red);
    th = atan2f(scr, sdt);
    const float c2 = cosf(th), s2 = sinf(th);
    tx = __fsub_rn(mdx, __fsub_rn(__fmul_rn(c2, msx), __fmul_rn(s2, msy)));
    ty = __fsub_rn(mdy, __fadd_rn(__fmul_rn(s2, msx), __fmul_rn(c2, msy)));
    tz = __fsub_rn(mdz, msz);
  }
  // ---- accept: inlier fraction, yaw, displacement of the centroid of the used source rows
  float gx = 0.f, gy = 0.f, gz = 0.f;
  for (int js = tid; js < us; js += RG_THREADS) {
    const RgP p = rg_point(pc0s, pc1, b, rows[sg.s_lo + rg_pick(js, sg.ns, a.icp_cap)], N0, N1);
    gx = __fadd_rn(gx, __fsub_rn(p.x, an.x));
    gy = __fadd_rn(gy, __fsub_rn(p.y, an.y));
    gz = __fadd_rn(gz, __fsub_rn(p.z, an.z));
  }
  const float fu = (float)us;
  const float cx = __fdiv_rn(rg_block_sum(gx, red), fu), cy = __fdiv_rn(rg_block_sum(gy, red), fu);
  rg_block_sum(gz, red);                                                    // (the z of the centroid moves by tz whatever it is)
  if (tid == 0) {
    const float c = cosf(th), s = sinf(th);
    const float mx = __fsub_rn(__fadd_rn(__fsub_rn(__fmul_rn(c, cx), __fmul_rn(s, cy)), tx), cx);
    const float my = __fsub_rn(__fadd_rn(__fadd_rn(__fmul_rn(s, cx), __fmul_rn(c, cy)), ty), cy);
    const float m2 = __fadd_rn(__fadd_rn(__fmul_rn(mx, mx), __fmul_rn(my, my)), __fmul_rn(tz, tz));
    const float frac = __fdiv_rn((float)inl_total, fu);
    int status = 1;
    if (!(frac >= a.min_inlier_frac)) status = 4;
    else if (!(fabsf(th) <= a.max_yaw) || !(m2 <= __fmul_rn(a.max_disp, a.max_disp))) status = 5;
    out[0] = th;
    out[1] = tx;
    out[2] = ty;
    out[3] = tz;
    out[4] = frac;
    out[5] = (float)sg.ns;
    out[6] = (float)sg.nd;
    out[7] = (float)status;
  }
}

// ---------------------------------------------------------------------------------------------------------------- apply
__global__ __launch_bounds__(256) void rg_apply_kernel(const float* __restrict__ pc0s, const int32_t* __restrict__ count0,
                                                       const int32_t* __restrict__ labels, const int32_t* __restrict__ seg_off,
                                                       const int32_t* __restrict__ seg_rows, const float* __restrict__ table, int N0, int N1,
                                                       int Kcap, float* __restrict__ flow, int32_t* __restrict__ rigid_id) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N0) return;
  const int N = N0 + N1;
  float f[3] = {0.f, 0.f, 0.f};
  int id = 0;
  const int l = labels[(int64_t)b * N + i];
  if (i < min(max(count0[b], 0), N0) && l >= 1 && l <= Kcap) {
    const float* t = table + ((int64_t)b * Kcap + (l - 1)) * 8;
    const int lo = seg_off[(int64_t)b * (2 * Kcap + 1) + 2 * (l - 1)];
    if (t[7] == 1.0f && lo >= 0 && lo < N) {
      const int ar = seg_rows[(int64_t)b * N + lo];
      if (ar >= 0 && ar < N0) {
        const float* s = pc0s + ((int64_t)b * N0 + i) * 3;
        const float* an = pc0s + ((int64_t)b * N0 + ar) * 3;
        const float c = cosf(t[0]), sn = sinf(t[0]);
        const float rx = __fsub_rn(s[0], an[0]), ry = __fsub_rn(s[1], an[1]);
        f[0] = __fsub_rn(__fadd_rn(__fsub_rn(__fmul_rn(c, rx), __fmul_rn(sn, ry)), t[1]), rx);
        f[1] = __fsub_rn(__fadd_rn(__fadd_rn(__fmul_rn(sn, rx), __fmul_rn(c, ry)), t[2]), ry);
        f[2] = t[3];
        id = l;
      }
    }
  }
  float* o = flow + ((int64_t)b * N0 + i) * 3;
  o[0] = f[0];
  o[1] = f[1];
  o[2] = f[2];
  rigid_id[(int64_t)b * N0 + i] = id;
}

inline size_t rg_vote_lds(int R) {
  const size_t nb = (size_t)(2 * R + 1) * (2 * R + 1);
  return (((nb + 2 * RG_THREADS) * 4 + 7) & ~(size_t)7) + (size_t)RG_THREADS * 8;
}

}  // namespace

extern "C" int64_t df_rigid_segments_ws_bytes(int B, int N0, int N1, int Kcap) {
  return rg_dims_ok(B, N0, N1, Kcap) ? rg_al16((int64_t)B * 2 * Kcap * 4) + rg_al16((int64_t)B * ((int64_t)N0 + N1) * 4) : (int64_t)DF_E_SHAPE;
}

extern "C" int df_rigid_segments(const int32_t* labels, int B, int N0, int N1, int Kcap, int32_t* seg_off, int32_t* seg_rows,
                                 int32_t* status, void* ws, void* stream) {
  DF_REQUIRE(labels && seg_off && seg_rows && status && ws, DF_E_ARG);
  DF_REQUIRE(rg_dims_ok(B, N0, N1, Kcap), DF_E_SHAPE);
  DF_REQUIRE((((uintptr_t)ws) & 3u) == 0, DF_E_ALIGN);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int N = N0 + N1;
  int32_t* cnt = reinterpret_cast<int32_t*>(ws);
  int32_t* rank = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(ws) + rg_al16((int64_t)B * 2 * Kcap * 4));
  hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(cnt), 0, (size_t)B * 2 * Kcap, s);
  if (e != hipSuccess) return (int)e;
  e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(seg_rows), -1, (size_t)B * N, s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(rg_count_kernel, dim3((N + 255) / 256, B), dim3(256), 0, s, labels, N0, N, Kcap, cnt, status);
  DF_CHECK_LAUNCH();
  hipLaunchKernelGGL(rg_scan_kernel, dim3(B), dim3(256), 0, s, Kcap, N, cnt, seg_off);
  DF_CHECK_LAUNCH();
  hipLaunchKernelGGL(rg_rank_kernel, dim3((N + RG_SCAT - 1) / RG_SCAT, B), dim3(RG_SCAT), 0, s, labels, N0, N, Kcap, rank);
  DF_CHECK_LAUNCH();
  hipLaunchKernelGGL(rg_scatter_kernel, dim3(B), dim3(RG_SCAT), 0, s, labels, N0, N, Kcap, seg_off, rank, cnt, seg_rows, status);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

extern "C" int df_rigid_vote(const float* pc0s, const float* pc1, const int32_t* seg_off, const int32_t* seg_rows, int B, int N0, int N1,
                             int Kcap, int min_side, int max_cluster_points, int vote_cap, float vote_bin, int R, int32_t* vote,
                             int32_t* hist, void* stream) {
  DF_REQUIRE(pc0s && pc1 && seg_off && seg_rows && vote, DF_E_ARG);
  DF_REQUIRE(rg_dims_ok(B, N0, N1, Kcap) && R >= 0 && R <= RG_RMAX, DF_E_SHAPE);
  DF_REQUIRE(hist == nullptr || (int64_t)B * Kcap * (2 * R + 1) * (2 * R + 1) < 0x80000000ll, DF_E_SHAPE);
  DF_REQUIRE(min_side >= 1 && max_cluster_points >= 1 && vote_cap >= 1 && vote_cap <= (1 << 20) && isfinite(vote_bin) && vote_bin > 0.f,
             DF_E_ARG);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (rg_vote_lds(R) > 48 * 1024) DF_SET_LDS_ONCE(rg_vote_kernel, rg_vote_lds(RG_RMAX));   // (the default R = 17 needs 9 KB)
  hipLaunchKernelGGL(rg_vote_kernel, dim3(Kcap, B), dim3(RG_THREADS), rg_vote_lds(R), s, pc0s, pc1, seg_off, seg_rows, N0, N1, Kcap, min_side,
                     max_cluster_points, vote_cap, vote_bin, R, vote, hist);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

extern "C" int64_t df_rigid_icp_ws_bytes(int B, int N0, int N1) {
  return rg_dims_ok(B, N0, N1, 1) ? rg_al16((int64_t)B * ((int64_t)N0 + N1) * 4) : (int64_t)DF_E_SHAPE;
}

extern "C" int df_rigid_icp(const float* pc0s, const float* pc1, const int32_t* seg_off, const int32_t* seg_rows, const int32_t* vote, int B,
                            int N0, int N1, int Kcap, int min_side, int max_cluster_points, int icp_cap, int icp_iters, float vote_bin,
                            float icp_max_dist, float min_inlier_frac, float max_yaw, float max_disp, float* table, void* ws, void* stream) {
  DF_REQUIRE(pc0s && pc1 && seg_off && seg_rows && vote && table && ws, DF_E_ARG);
  DF_REQUIRE(rg_dims_ok(B, N0, N1, Kcap), DF_E_SHAPE);
  DF_REQUIRE(min_side >= 1 && max_cluster_points >= 1 && icp_cap >= 1 && icp_cap <= (1 << 20) && icp_iters >= 0 && icp_iters <= 1024, DF_E_ARG);
  DF_REQUIRE(isfinite(vote_bin) && vote_bin > 0.f && isfinite(icp_max_dist) && icp_max_dist > 0.f && isfinite(min_inlier_frac) &&
                 isfinite(max_yaw) && max_yaw >= 0.f && isfinite(max_disp) && max_disp >= 0.f,
             DF_E_ARG);
  DF_REQUIRE((((uintptr_t)ws) & 3u) == 0, DF_E_ALIGN);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  RgIcp a;
  a.icp_cap = icp_cap;
  a.icp_iters = icp_iters;
  a.vote_bin = vote_bin;
  a.max_dist = icp_max_dist;
  a.min_inlier_frac = min_inlier_frac;
  a.max_yaw = max_yaw;
  a.max_disp = max_disp;
  hipLaunchKernelGGL(rg_icp_kernel, dim3(Kcap, B), dim3(RG_THREADS), 0, s, pc0s, pc1, seg_off, seg_rows, vote, N0, N1, Kcap, min_side,
                     max_cluster_points, a, table, reinterpret_cast<int32_t*>(ws));
  DF_CHECK_LAUNCH();
  return DF_OK;
}

extern "C" int df_rigid_apply(const float* pc0s, const int32_t* count0, const int32_t* labels, const int32_t* seg_off,
                              const int32_t* seg_rows, const float* table, int B, int N0, int N1, int Kcap, float* flow, int32_t* rigid_id,
                              void* stream) {
  DF_REQUIRE(pc0s && count0 && labels && seg_off && seg_rows && table && flow && rigid_id, DF_E_ARG);
  DF_REQUIRE(rg_dims_ok(B, N0, N1, Kcap), DF_E_SHAPE);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(rg_apply_kernel, dim3((N0 + 255) / 256, B), dim3(256), 0, s, pc0s, count0, labels, seg_off, seg_rows, table, N0, N1, Kcap,
                     flow, rigid_id);
  DF_CHECK_LAUNCH();
  return DF_OK;
}
