// A voxel-capped local map kept on the device: what the scan-to-map odometry registers a sweep against instead of its predecessor.
// UNPINNED -- the definition is this project's own: include/deflow_amd.h, DESIGN.md section 6t.
//
// One update is  df_map_keys -> df_cell_sort (pillarize.hip, unchanged) -> df_map_select -> df_map_compact;  df_map_view makes the
// target cloud of a registration.  Candidates: n = cap + N rows per sample, the map's cap rows first, then the sweep's N rows.
//
//   df_map_keys     one thread per candidate: world coordinates (float64, every operation rounded once: no fma), the voxel index by
//                   floor, the window column (dy, dx) about the voxel of the pose's translation as the sort key, the z voxel beside it.
//   df_map_select   a fill launch (keep = 0), then one thread per sorted position: its rank among the earlier rows of its column with
//                   the same z voxel -- one dependent load pair per earlier row, stopped once the rank reaches K.  The lanes of a wave
//                   are neighbouring positions of one column (or of neighbouring columns), so their walks have about one length.
//   df_map_compact  block counts of the kept rows, one scan of them per sample, scatter; a row of map_out past the new count gets NaNs
//                   from the thread of the same index.  No look-back, no atomics.
//   df_map_view     the map's rows in the sensor's frame, fp32; NaN rows past the count.
//   df_map_drop     df_map_compact's shape over the map's own rows: block counts of the rows whose flag is 0, one scan per sample,
//                   scatter into the other buffer (the rows the depth cube of visibility.hip saw through).
//   df_map_compact_near  df_map_compact's second form (opt-in): on overflow the rows of the outermost window
//                   rings go, not the end of the sorted order.  A fill launch, the kept rows per (sample, ring), one block per sample
//                   that scans the ring counts into cut = (R, budget), then df_map_compact's three launches with two prefixes carried
//                   together: the rows of rings < R and those of ring R.
//
// No float atomics.  The entries above run no integer atomics (df_cell_sort's are the only ones of an update) and no LDS outside the
// 256-wide scans; df_map_compact_near alone adds an 8 KiB LDS histogram per block and integer atomicAdds into it and into its ring counts
// in ws -- integer sums do not depend on the order of their operands, so its results are as repeatable as the others'.
#include <math.h>

#include "common.h"

namespace {

constexpr double MAP_VOX_LIMIT = 1073741824.0;      // |voxel index| < 2^30 on every axis

__device__ __forceinline__ double map_nan() { return __builtin_bit_cast(double, 0x7ff8000000000000ull); }

// floor(w / voxel) as an integer; false where w is not finite or the index is not inside (-2^30, 2^30).  The conversion is made only
// after the range check, so it is defined for every input.
__device__ __forceinline__ bool map_voxel(double w, double voxel, int* v) {
  const double f = floor(__ddiv_rn(w, voxel));
  if (!(isfinite(w) && fabs(f) < MAP_VOX_LIMIT)) return false;
  *v = (int)f;
  return true;
}

__global__ __launch_bounds__(256) void map_keys_kernel(const double* __restrict__ map, const int32_t* __restrict__ count,
                                                       const float* __restrict__ sweep, const int32_t* __restrict__ sweep_count,
                                                       const int32_t* __restrict__ mask, const int32_t* __restrict__ gate,
                                                       const double* __restrict__ pose, int cap, int N, double voxel, int W,
                                                       double* __restrict__ cand, uint32_t* __restrict__ key, int32_t* __restrict__ vz) {
  const int b = blockIdx.y;
  const int n = cap + N;
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const double* T = pose + (int64_t)b * 16;
  const int S = 2 * W + 1;
  const uint32_t drop = (uint32_t)gridDim.y * (uint32_t)S * (uint32_t)S;
  double w0, w1, w2;
  bool ok;
  if (r < cap) {
    ok = r < count[b];
    const double* m = map + ((int64_t)b * cap + r) * 3;
    w0 = m[0];
    w1 = m[1];
    w2 = m[2];
  } else {
    const int64_t s = (int64_t)b * N + (r - cap);
    ok = (r - cap) < sweep_count[b] && (!mask || mask[s] > 0) && (!gate || gate[b] == 0);
    const float xf = sweep[s * 3], yf = sweep[s * 3 + 1], zf = sweep[s * 3 + 2];
    ok = ok && isfinite(xf) && isfinite(yf) && isfinite(zf);
    const double x = (double)xf, y = (double)yf, z = (double)zf;
    w0 = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(T[0], x), __dmul_rn(T[1], y)), __dmul_rn(T[2], z)), T[3]);
    w1 = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(T[4], x), __dmul_rn(T[5], y)), __dmul_rn(T[6], z)), T[7]);
    w2 = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(T[8], x), __dmul_rn(T[9], y)), __dmul_rn(T[10], z)), T[11]);
  }
  int v0 = 0, v1 = 0, v2 = 0, a0 = 0, a1 = 0;
  ok = ok && map_voxel(T[3], voxel, &a0) && map_voxel(T[7], voxel, &a1);
  ok = ok && map_voxel(w0, voxel, &v0) && map_voxel(w1, voxel, &v1) && map_voxel(w2, voxel, &v2);
  const int64_t dx = (int64_t)v0 - a0 + W, dy = (int64_t)v1 - a1 + W;
  ok = ok && dx >= 0 && dx < S && dy >= 0 && dy < S;
  const int64_t o = (int64_t)b * n + r;
  key[o] = ok ? ((uint32_t)b * (uint32_t)S + (uint32_t)dy) * (uint32_t)S + (uint32_t)dx : drop;
  vz[o] = ok ? v2 : 0;
  cand[o * 3] = ok ? w0 : map_nan();
  cand[o * 3 + 1] = ok ? w1 : map_nan();
  cand[o * 3 + 2] = ok ? w2 : map_nan();
}

__global__ __launch_bounds__(256) void map_fill_i32_kernel(int64_t n, int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = 0;
}

__global__ __launch_bounds__(256) void map_select_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ idx_sorted,
                                                         const int32_t* __restrict__ cell_rng, const int32_t* __restrict__ vz,
                                                         int64_t total_rows, uint32_t ncells, int K, int32_t* __restrict__ keep) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int64_t total = cell_rng[2 * (int64_t)(ncells - 1) + 1];
  if (total > total_rows) total = total_rows;
  if (p >= total) return;
  const uint32_t c = idx_sorted[p];
  if (c >= (uint64_t)total_rows) return;
  const uint32_t cell = key[c];
  if (cell >= ncells) return;
  int64_t q = cell_rng[2 * (int64_t)cell];
  if (q < 0) q = 0;
  const int z = vz[c];
  int rank = 0;
  for (; q < p && rank < K; ++q) {
    const uint32_t d = idx_sorted[q];
    if (d < (uint64_t)total_rows && vz[d] == z) ++rank;
  }
  keep[c] = rank < K ? 1 : 0;
}

// exclusive scan of one int per thread over a block of 256; *total = the block's sum
__device__ __forceinline__ int map_excl_scan256(int v, int* lds, int* total) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int a = t >= o ? lds[t - o] : 0;
    __syncthreads();
    lds[t] += a;
    __syncthreads();
  }
  *total = lds[255];
  const int ex = lds[t] - v;
  __syncthreads();
  return ex;
}

// the sorted positions [s0, e0) of sample b: the start of its first column to the end of its last, held to the buffer's rows
__device__ __forceinline__ void map_span(const int32_t* __restrict__ cell_rng, int b, int S, int n, int64_t total_rows, int64_t* s0,
                                         int64_t* e0) {
  const int64_t cells = (int64_t)S * S;
  int64_t s = cell_rng[2 * (b * cells)], e = cell_rng[2 * ((b + 1) * cells - 1) + 1];
  if (s < 0) s = 0;
  if (e > s + n) e = s + n;
  if (e > total_rows) e = total_rows;
  *s0 = s;
  *e0 = e;
}

// (kept, from the sweep) of the sorted position p of sample b; c: its candidate
__device__ __forceinline__ int map_flag(const uint32_t* __restrict__ idx_sorted, const int32_t* __restrict__ keep, int64_t p, int64_t e0,
                                        int b, int n, int cap, int* from_sweep, int64_t* c_out) {
  *from_sweep = 0;
  *c_out = 0;
  if (p >= e0) return 0;
  const int64_t c = idx_sorted[p];
  const int64_t r = c - (int64_t)b * n;
  if (r < 0 || r >= n || keep[c] <= 0) return 0;
  *from_sweep = r >= cap ? 1 : 0;
  *c_out = c;
  return 1;
}

__global__ __launch_bounds__(256) void map_count_kernel(const uint32_t* __restrict__ idx_sorted, const int32_t* __restrict__ cell_rng,
                                                        const int32_t* __restrict__ keep, int cap, int N, int S,
                                                        int32_t* __restrict__ blk) {
  __shared__ int lds[256];
  const int b = blockIdx.y, n = cap + N;
  int64_t s0, e0, c;
  map_span(cell_rng, b, S, n, (int64_t)gridDim.y * n, &s0, &e0);
  int sw;
  const int f = map_flag(idx_sorted, keep, s0 + (int64_t)blockIdx.x * 256 + threadIdx.x, e0, b, n, cap, &sw, &c);
  int kept, swept;
  map_excl_scan256(f, lds, &kept);
  map_excl_scan256(sw, lds, &swept);
  if (threadIdx.x == 0) {
    int32_t* o = blk + ((int64_t)b * gridDim.x + blockIdx.x) * 2;
    o[0] = kept;
    o[1] = swept;
  }
}

// one block per sample: blk[b][k][0] becomes the number of kept rows before block k; count_out and stat of the sample
__global__ __launch_bounds__(256) void map_scan_kernel(const int32_t* __restrict__ cell_rng, int cap, int N, int S, int nblk,
                                                       int32_t* __restrict__ blk, int32_t* __restrict__ count_out,
                                                       int32_t* __restrict__ stat) {
  __shared__ int lds[256];
  const int b = blockIdx.x, n = cap + N;
  int32_t* mine = blk + (int64_t)b * nblk * 2;
  int carry = 0, swept = 0;
  for (int base = 0; base < nblk; base += 256) {
    const int i = base + threadIdx.x;
    const int v = i < nblk ? mine[2 * i] : 0, s = i < nblk ? mine[2 * i + 1] : 0;
    int total, stotal;
    const int ex = map_excl_scan256(v, lds, &total);
    map_excl_scan256(s, lds, &stotal);
    if (i < nblk) mine[2 * i] = carry + ex;
    carry += total;
    swept += stotal;
  }
  if (threadIdx.x == 0) {
    int64_t s0, e0;
    map_span(cell_rng, b, S, n, (int64_t)gridDim.x * n, &s0, &e0);
    count_out[b] = carry < cap ? carry : cap;
    stat[4 * b] = e0 > s0 ? (int)(e0 - s0) : 0;
    stat[4 * b + 1] = carry;
    stat[4 * b + 2] = swept;
    stat[4 * b + 3] = carry > cap ? carry - cap : 0;
  }
}

__global__ __launch_bounds__(256) void map_scatter_kernel(const double* __restrict__ cand, const uint32_t* __restrict__ idx_sorted,
                                                          const int32_t* __restrict__ cell_rng, const int32_t* __restrict__ keep,
                                                          const int32_t* __restrict__ blk, const int32_t* __restrict__ count_out,
                                                          int cap, int N, int S, double* __restrict__ map_out) {
  __shared__ int lds[256];
  const int b = blockIdx.y, n = cap + N;
  int64_t s0, e0, c;
  map_span(cell_rng, b, S, n, (int64_t)gridDim.y * n, &s0, &e0);
  const int j = blockIdx.x * 256 + threadIdx.x;
  int sw, total;
  const int f = map_flag(idx_sorted, keep, s0 + j, e0, b, n, cap, &sw, &c);
  const int64_t at = (int64_t)blk[((int64_t)b * gridDim.x + blockIdx.x) * 2] + map_excl_scan256(f, lds, &total);
  double* out = map_out + (int64_t)b * cap * 3;
  if (f && at >= 0 && at < cap) {                        // rows below count_out[b]: each kept row has its own `at`
    out[at * 3] = cand[c * 3];
    out[at * 3 + 1] = cand[c * 3 + 1];
    out[at * 3 + 2] = cand[c * 3 + 2];
  }
  if (j < cap && j >= count_out[b]) {                    // rows from count_out[b] on: the thread of the same index
    out[(int64_t)j * 3] = map_nan();
    out[(int64_t)j * 3 + 1] = map_nan();
    out[(int64_t)j * 3 + 2] = map_nan();
  }
}

__global__ __launch_bounds__(256) void map_view_kernel(const double* __restrict__ map, const int32_t* __restrict__ count,
                                                       const double* __restrict__ pose, int cap, float* __restrict__ dst) {
  const int b = blockIdx.y;
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= cap) return;
  float* o = dst + ((int64_t)b * cap + r) * 3;
  if (r >= count[b]) {
    const float none = __builtin_bit_cast(float, 0x7fc00000u);
    o[0] = none;
    o[1] = none;
    o[2] = none;
    return;
  }
  const double* T = pose + (int64_t)b * 16;
  const double* m = map + ((int64_t)b * cap + r) * 3;
  const double d0 = __dsub_rn(m[0], T[3]), d1 = __dsub_rn(m[1], T[7]), d2 = __dsub_rn(m[2], T[11]);
#pragma unroll
  for (int j = 0; j < 3; ++j)                             // R^T d: column j of R
    o[j] = __double2float_rn(__dadd_rn(__dadd_rn(__dmul_rn(T[j], d0), __dmul_rn(T[4 + j], d1)), __dmul_rn(T[8 + j], d2)));
}

// ---- df_map_drop: the stable compaction of df_map_compact over the map's own rows, keyed by a flag instead of a sorted order ----------
// row j of sample b stays: j < count[b] and (the sample is gated or flag[b][j] == 0)
__device__ __forceinline__ int drop_stays(const int32_t* __restrict__ count, const int32_t* __restrict__ flag,
                                          const int32_t* __restrict__ gate, int b, int cap, int j) {
  int cnt = count[b];
  cnt = cnt < 0 ? 0 : (cnt > cap ? cap : cnt);
  if (j >= cnt) return 0;
  if (gate && gate[b] != 0) return 1;
  return flag[(int64_t)b * cap + j] == 0 ? 1 : 0;
}

__global__ __launch_bounds__(256) void drop_count_kernel(const int32_t* __restrict__ count, const int32_t* __restrict__ flag,
                                                         const int32_t* __restrict__ gate, int cap, int32_t* __restrict__ blk) {
  __shared__ int lds[256];
  const int b = blockIdx.y;
  int total;
  map_excl_scan256(drop_stays(count, flag, gate, b, cap, blockIdx.x * 256 + threadIdx.x), lds, &total);
  if (threadIdx.x == 0) blk[(int64_t)b * gridDim.x + blockIdx.x] = total;
}

// one block per sample: blk[b][k] becomes the number of staying rows before block k; count_out and stat of the sample
__global__ __launch_bounds__(256) void drop_scan_kernel(const int32_t* __restrict__ count, const int32_t* __restrict__ gate, int cap,
                                                        int nblk, int32_t* __restrict__ blk, int32_t* __restrict__ count_out,
                                                        int32_t* __restrict__ stat) {
  __shared__ int lds[256];
  const int b = blockIdx.x;
  int32_t* mine = blk + (int64_t)b * nblk;
  int carry = 0;
  for (int base = 0; base < nblk; base += 256) {
    const int i = base + threadIdx.x;
    const int v = i < nblk ? mine[i] : 0;
    int total;
    const int ex = map_excl_scan256(v, lds, &total);
    if (i < nblk) mine[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) {
    int cnt = count[b];
    cnt = cnt < 0 ? 0 : (cnt > cap ? cap : cnt);
    const bool gated = gate && gate[b] != 0;
    count_out[b] = carry;
    stat[2 * b] = gated ? 0 : cnt;
    stat[2 * b + 1] = cnt - carry;
  }
}

__global__ __launch_bounds__(256) void drop_scatter_kernel(const double* __restrict__ map, const int32_t* __restrict__ count,
                                                           const int32_t* __restrict__ flag, const int32_t* __restrict__ gate,
                                                           const int32_t* __restrict__ blk, const int32_t* __restrict__ count_out, int cap,
                                                           double* __restrict__ map_out) {
  __shared__ int lds[256];
  const int b = blockIdx.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  const int f = drop_stays(count, flag, gate, b, cap, j);
  int total;
  const int64_t at = (int64_t)blk[(int64_t)b * gridDim.x + blockIdx.x] + map_excl_scan256(f, lds, &total);
  const double* in = map + ((int64_t)b * cap + j) * 3;
  double* out = map_out + (int64_t)b * cap * 3;
  if (f && at >= 0 && at < cap) {                        // rows below count_out[b]: each staying row has its own `at` <= j
    out[at * 3] = in[0];
    out[at * 3 + 1] = in[1];
    out[at * 3 + 2] = in[2];
  }
  if (j < cap && j >= count_out[b]) {                    // rows from count_out[b] on: the thread of the same index
    out[(int64_t)j * 3] = map_nan();
    out[(int64_t)j * 3 + 1] = map_nan();
    out[(int64_t)j * 3 + 2] = map_nan();
  }
}

// ---- df_map_compact_near: df_map_compact with the window shrunk ring by ring until the kept rows fit -------------
// ring of a kept row of sample b = max(|dx - W|, |dy - W|) of its window column, from its key (b S + dy) S + dx; a key outside the
// sample's columns (no kept row has one: df_map_select keeps only rows of a column) is held to ring W, so every index below is in range
__device__ __forceinline__ int near_ring(uint32_t cell, int b, int S, int W) {
  const uint32_t cells = (uint32_t)S * (uint32_t)S;
  const uint32_t local = cell - (uint32_t)b * cells;
  if (local >= cells) return W;
  const int dy = (int)(local / (uint32_t)S), dx = (int)(local - (uint32_t)dy * (uint32_t)S);
  const int ax = dx > W ? dx - W : W - dx, ay = dy > W ? dy - W : W - dy;
  return ax > ay ? ax : ay;
}

// hist[b][r] += the kept rows of ring r in this block of sorted positions: an LDS histogram, then one integer atomicAdd per occupied ring
__global__ __launch_bounds__(256) void near_ring_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ idx_sorted,
                                                        const int32_t* __restrict__ cell_rng, const int32_t* __restrict__ keep, int cap,
                                                        int N, int S, int W, int32_t* __restrict__ hist) {
  __shared__ int h[2048];
  const int b = blockIdx.y, n = cap + N;
  for (int r = threadIdx.x; r <= W; r += 256) h[r] = 0;
  __syncthreads();
  int64_t s0, e0, c;
  map_span(cell_rng, b, S, n, (int64_t)gridDim.y * n, &s0, &e0);
  int sw;
  if (map_flag(idx_sorted, keep, s0 + (int64_t)blockIdx.x * 256 + threadIdx.x, e0, b, n, cap, &sw, &c))
    atomicAdd(&h[near_ring(key[c], b, S, W)], 1);
  __syncthreads();
  for (int r = threadIdx.x; r <= W; r += 256) {
    const int v = h[r];
    if (v) atomicAdd(hist + (int64_t)b * (W + 1) + r, v);
  }
}

// one block per sample: cut[b] = (R, budget) -- the ring r whose exclusive prefix e of the ring counts has e <= cap < e + hist[r], and
// cap - e; (W + 1, 0) when all kept rows fit.  The prefix does not decrease, so at most one ring meets the condition.
__global__ __launch_bounds__(256) void near_cut_kernel(const int32_t* __restrict__ hist, int cap, int W, int32_t* __restrict__ cut) {
  __shared__ int lds[256];
  const int b = blockIdx.x;
  const int32_t* mine = hist + (int64_t)b * (W + 1);
  int carry = 0;
  for (int base = 0; base <= W; base += 256) {
    const int r = base + threadIdx.x;
    const int v = r <= W ? mine[r] : 0;
    int total;
    const int e = carry + map_excl_scan256(v, lds, &total);
    if (v > 0 && e <= cap && e + v > cap) {
      cut[2 * b] = r;
      cut[2 * b + 1] = cap - e;
    }
    carry += total;
  }
  if (threadIdx.x == 0 && carry <= cap) {
    cut[2 * b] = W + 1;
    cut[2 * b + 1] = 0;
  }
}

// (inner | partial << 16) of the sorted position p of sample b: kept and of a ring < R, kept and of ring R; *kept, *from_sweep, c as map_flag
__device__ __forceinline__ int near_flag(const uint32_t* __restrict__ key, const uint32_t* __restrict__ idx_sorted,
                                         const int32_t* __restrict__ keep, int64_t p, int64_t e0, int b, int n, int cap, int S, int W, int R,
                                         int* kept, int* from_sweep, int64_t* c_out) {
  *kept = map_flag(idx_sorted, keep, p, e0, b, n, cap, from_sweep, c_out);
  if (!*kept) return 0;
  const int ring = near_ring(key[*c_out], b, S, W);
  return ring < R ? 1 : (ring == R ? 1 << 16 : 0);
}

// blk[b][k] = (inner, partial, kept, from the sweep) of block k of sorted positions; two counts of at most 256 share one scan
__global__ __launch_bounds__(256) void near_count_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ idx_sorted,
                                                         const int32_t* __restrict__ cell_rng, const int32_t* __restrict__ keep,
                                                         const int32_t* __restrict__ cut, int cap, int N, int S, int W,
                                                         int32_t* __restrict__ blk) {
  __shared__ int lds[256];
  const int b = blockIdx.y, n = cap + N;
  int64_t s0, e0, c;
  map_span(cell_rng, b, S, n, (int64_t)gridDim.y * n, &s0, &e0);
  int f, sw;
  const int ip = near_flag(key, idx_sorted, keep, s0 + (int64_t)blockIdx.x * 256 + threadIdx.x, e0, b, n, cap, S, W, cut[2 * b], &f, &sw, &c);
  int both, rows;
  map_excl_scan256(ip, lds, &both);
  map_excl_scan256(f | (sw << 16), lds, &rows);
  if (threadIdx.x == 0) {
    int32_t* o = blk + ((int64_t)b * gridDim.x + blockIdx.x) * 4;
    o[0] = both & 0xffff;
    o[1] = both >> 16;
    o[2] = rows & 0xffff;
    o[3] = rows >> 16;
  }
}

// one block per sample: blk[b][k][0], [1] become the inner and the partial rows before block k; count_out and stat of the sample
__global__ __launch_bounds__(256) void near_scan_kernel(const int32_t* __restrict__ cell_rng, int cap, int N, int S, int nblk,
                                                        int32_t* __restrict__ blk, int32_t* __restrict__ count_out,
                                                        int32_t* __restrict__ stat) {
  __shared__ int lds[256];
  const int b = blockIdx.x, n = cap + N;
  int32_t* mine = blk + (int64_t)b * nblk * 4;
  int inner = 0, part = 0, kept = 0, swept = 0;
  for (int base = 0; base < nblk; base += 256) {
    const int i = base + threadIdx.x;
    const bool in = i < nblk;
    const int vi = in ? mine[4 * i] : 0, vp = in ? mine[4 * i + 1] : 0, vk = in ? mine[4 * i + 2] : 0, vs = in ? mine[4 * i + 3] : 0;
    int ti, tp, tk, ts;
    const int ei = map_excl_scan256(vi, lds, &ti);
    const int ep = map_excl_scan256(vp, lds, &tp);
    map_excl_scan256(vk, lds, &tk);
    map_excl_scan256(vs, lds, &ts);
    if (in) {
      mine[4 * i] = inner + ei;
      mine[4 * i + 1] = part + ep;
    }
    inner += ti;
    part += tp;
    kept += tk;
    swept += ts;
  }
  if (threadIdx.x == 0) {
    int64_t s0, e0;
    map_span(cell_rng, b, S, n, (int64_t)gridDim.x * n, &s0, &e0);
    count_out[b] = kept < cap ? kept : cap;
    stat[4 * b] = e0 > s0 ? (int)(e0 - s0) : 0;
    stat[4 * b + 1] = kept;
    stat[4 * b + 2] = swept;
    stat[4 * b + 3] = kept > cap ? kept - cap : 0;
  }
}

__global__ __launch_bounds__(256) void near_scatter_kernel(const double* __restrict__ cand, const uint32_t* __restrict__ key,
                                                           const uint32_t* __restrict__ idx_sorted, const int32_t* __restrict__ cell_rng,
                                                           const int32_t* __restrict__ keep, const int32_t* __restrict__ cut,
                                                           const int32_t* __restrict__ blk, const int32_t* __restrict__ count_out, int cap,
                                                           int N, int S, int W, double* __restrict__ map_out) {
  __shared__ int lds[256];
  const int b = blockIdx.y, n = cap + N;
  int64_t s0, e0, c;
  map_span(cell_rng, b, S, n, (int64_t)gridDim.y * n, &s0, &e0);
  const int j = blockIdx.x * 256 + threadIdx.x;
  const int budget = cut[2 * b + 1];
  int f, sw, total;
  const int ip = near_flag(key, idx_sorted, keep, s0 + j, e0, b, n, cap, S, W, cut[2 * b], &f, &sw, &c);
  const int ex = map_excl_scan256(ip, lds, &total);
  const int32_t* mine = blk + ((int64_t)b * gridDim.x + blockIdx.x) * 4;
  const int before_inner = mine[0] + (ex & 0xffff), before_part = mine[1] + (ex >> 16);
  const bool survives = (ip & 0xffff) != 0 || ((ip >> 16) != 0 && before_part < budget);
  const int64_t at = (int64_t)before_inner + (before_part < budget ? before_part : budget);
  double* out = map_out + (int64_t)b * cap * 3;
  if (survives && at >= 0 && at < cap) {                 // rows below count_out[b]: each survivor has its own `at`
    out[at * 3] = cand[c * 3];
    out[at * 3 + 1] = cand[c * 3 + 1];
    out[at * 3 + 2] = cand[c * 3 + 2];
  }
  if (j < cap && j >= count_out[b]) {                    // rows from count_out[b] on: the thread of the same index
    out[(int64_t)j * 3] = map_nan();
    out[(int64_t)j * 3 + 1] = map_nan();
    out[(int64_t)j * 3 + 2] = map_nan();
  }
}

bool map_shape_ok(int B, int cap, int N, int W) {
  if (B < 1 || B > 65535 || cap < 1 || N < 0 || W < 1 || W > 2047) return false;
  const int64_t S = 2 * (int64_t)W + 1;
  return (int64_t)B * ((int64_t)cap + N) < (1ll << 30) && (int64_t)B * S * S < (1ll << 30);
}

inline bool map_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" int64_t df_map_ws_bytes(int B, int cap, int N) {
  if (!map_shape_ok(B, cap, N, 1) || N < 1) return DF_E_SHAPE;
  return (int64_t)B * (((int64_t)cap + N + 255) / 256) * 2 * (int64_t)sizeof(int32_t);
}

extern "C" int df_map_keys(const double* map, const int32_t* count, const float* sweep, const int32_t* sweep_count, const int32_t* mask,
                           const int32_t* gate, const double* pose, int B, int cap, int N, double voxel, int W, double* cand,
                           uint32_t* key, int32_t* vz, void* stream) {
  DF_REQUIRE(map && count && sweep && sweep_count && pose && cand && key && vz, DF_E_ARG);
  DF_REQUIRE(map_shape_ok(B, cap, N, W) && N >= 1, DF_E_SHAPE);
  DF_REQUIRE(isfinite(voxel) && voxel > 0.0, DF_E_ARG);
  DF_REQUIRE(map_aligned(map, 8) && map_aligned(pose, 8) && map_aligned(cand, 8) && map_aligned(sweep, 4) && map_aligned(key, 4) &&
                 map_aligned(vz, 4), DF_E_ALIGN);
  hipLaunchKernelGGL(map_keys_kernel, dim3((unsigned)((cap + N + 255) / 256), B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), map,
                     count, sweep, sweep_count, mask, gate, pose, cap, N, voxel, W, cand, key, vz);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

extern "C" int df_map_select(const uint32_t* key, const uint32_t* idx_sorted, const int32_t* cell_rng, const int32_t* vz, int B, int n,
                             int W, int max_per_voxel, int32_t* keep, void* stream) {
  DF_REQUIRE(key && idx_sorted && cell_rng && vz && keep, DF_E_ARG);
  DF_REQUIRE(n >= 1 && map_shape_ok(B, n, 0, W), DF_E_SHAPE);
  DF_REQUIRE(max_per_voxel >= 1, DF_E_ARG);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t rows = (int64_t)B * n;
  const int64_t S = 2 * (int64_t)W + 1;
  const dim3 grid((unsigned)((rows + 255) / 256));
  hipLaunchKernelGGL(map_fill_i32_kernel, grid, dim3(256), 0, s, rows, keep);
  DF_CHECK_LAUNCH();
  hipLaunchKernelGGL(map_select_kernel, grid, dim3(256), 0, s, key, idx_sorted, cell_rng, vz, rows, (uint32_t)(B * S * S), max_per_voxel,
                     keep);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

extern "C" int df_map_compact(const double* cand, const uint32_t* idx_sorted, const int32_t* cell_rng, const int32_t* keep, int B, int cap,
                              int N, int W, double* map_out, int32_t* count_out, int32_t* stat, void* ws, void* stream) {
  DF_REQUIRE(cand && idx_sorted && cell_rng && keep && map_out && count_out && stat && ws, DF_E_ARG);
  DF_REQUIRE(map_shape_ok(B, cap, N, W) && N >= 1, DF_E_SHAPE);
  DF_REQUIRE(map_aligned(cand, 8) && map_aligned(map_out, 8) && map_aligned(ws, 4), DF_E_ALIGN);
  DF_REQUIRE(static_cast<const void*>(cand) != static_cast<const void*>(map_out), DF_E_ARG);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int nblk = (cap + N + 255) / 256, S = 2 * W + 1;
  int32_t* blk = reinterpret_cast<int32_t*>(ws);
  hipLaunchKernelGGL(map_count_kernel, dim3(nblk, B), dim3(256), 0, s, idx_sorted, cell_rng, keep, cap, N, S, blk);
  DF_CHECK_LAUNCH();
  hipLaunchKernelGGL(map_scan_kernel, dim3(B), dim3(256), 0, s, cell_rng, cap, N, S, nblk, blk, count_out, stat);
  DF_CHECK_LAUNCH();
  hipLaunchKernelGGL(map_scatter_kernel, dim3(nblk, B), dim3(256), 0, s, cand, idx_sorted, cell_rng, keep, blk, count_out, cap, N, S,
                     map_out);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

// ws of df_map_compact_near: the ring counts [B][W + 1], then (inner, partial, kept, from the sweep) per block [B][nblk][4], all i32
extern "C" int64_t df_map_near_ws_bytes(int B, int cap, int N, int W) {
  if (!map_shape_ok(B, cap, N, W) || N < 1) return DF_E_SHAPE;
  return (int64_t)B * ((int64_t)W + 1 + (((int64_t)cap + N + 255) / 256) * 4) * (int64_t)sizeof(int32_t);
}

extern "C" int df_map_compact_near(const double* cand, const uint32_t* key, const uint32_t* idx_sorted, const int32_t* cell_rng,
                                   const int32_t* keep, int B, int cap, int N, int W, double* map_out, int32_t* count_out, int32_t* stat,
                                   int32_t* cut, void* ws, void* stream) {
  DF_REQUIRE(cand && key && idx_sorted && cell_rng && keep && map_out && count_out && stat && cut && ws, DF_E_ARG);
  DF_REQUIRE(map_shape_ok(B, cap, N, W) && N >= 1, DF_E_SHAPE);
  DF_REQUIRE(map_aligned(cand, 8) && map_aligned(map_out, 8) && map_aligned(ws, 4), DF_E_ALIGN);
  DF_REQUIRE(static_cast<const void*>(cand) != static_cast<const void*>(map_out), DF_E_ARG);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int nblk = (cap + N + 255) / 256, S = 2 * W + 1;
  const int64_t rings = (int64_t)B * (W + 1);
  int32_t* hist = reinterpret_cast<int32_t*>(ws);
  int32_t* blk = hist + rings;
  hipLaunchKernelGGL(map_fill_i32_kernel, dim3((unsigned)((rings + 255) / 256)), dim3(256), 0, s, rings, hist);
  DF_CHECK_LAUNCH();
  hipLaunchKernelGGL(near_ring_kernel, dim3(nblk, B), dim3(256), 0, s, key, idx_sorted, cell_rng, keep, cap, N, S, W, hist);
  DF_CHECK_LAUNCH();
  hipLaunchKernelGGL(near_cut_kernel, dim3(B), dim3(256), 0, s, hist, cap, W, cut);
  DF_CHECK_LAUNCH();
  hipLaunchKernelGGL(near_count_kernel, dim3(nblk, B), dim3(256), 0, s, key, idx_sorted, cell_rng, keep, cut, cap, N, S, W, blk);
  DF_CHECK_LAUNCH();
  hipLaunchKernelGGL(near_scan_kernel, dim3(B), dim3(256), 0, s, cell_rng, cap, N, S, nblk, blk, count_out, stat);
  DF_CHECK_LAUNCH();
  hipLaunchKernelGGL(near_scatter_kernel, dim3(nblk, B), dim3(256), 0, s, cand, key, idx_sorted, cell_rng, keep, cut, blk, count_out, cap,
                     N, S, W, map_out);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

extern "C" int64_t df_map_drop_ws_bytes(int B, int cap) {
  if (!map_shape_ok(B, cap, 0, 1)) return DF_E_SHAPE;
  return (int64_t)B * (((int64_t)cap + 255) / 256) * (int64_t)sizeof(int32_t);
}

extern "C" int df_map_drop(const double* map, const int32_t* count, const int32_t* flag, const int32_t* gate, int B, int cap,
                           double* map_out, int32_t* count_out, int32_t* stat, void* ws, void* stream) {
  DF_REQUIRE(map && count && flag && map_out && count_out && stat && ws, DF_E_ARG);
  DF_REQUIRE(map_shape_ok(B, cap, 0, 1), DF_E_SHAPE);
  DF_REQUIRE(map_aligned(map, 8) && map_aligned(map_out, 8) && map_aligned(flag, 4) && map_aligned(ws, 4), DF_E_ALIGN);
  DF_REQUIRE(static_cast<const void*>(map) != static_cast<const void*>(map_out), DF_E_ARG);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int nblk = (cap + 255) / 256;
  int32_t* blk = reinterpret_cast<int32_t*>(ws);
  hipLaunchKernelGGL(drop_count_kernel, dim3(nblk, B), dim3(256), 0, s, count, flag, gate, cap, blk);
  DF_CHECK_LAUNCH();
  hipLaunchKernelGGL(drop_scan_kernel, dim3(B), dim3(256), 0, s, count, gate, cap, nblk, blk, count_out, stat);
  DF_CHECK_LAUNCH();
  hipLaunchKernelGGL(drop_scatter_kernel, dim3(nblk, B), dim3(256), 0, s, map, count, flag, gate, blk, count_out, cap, map_out);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

extern "C" int df_map_view(const double* map, const int32_t* count, const double* pose, int B, int cap, float* dst, void* stream) {
  DF_REQUIRE(map && count && pose && dst, DF_E_ARG);
  DF_REQUIRE(map_shape_ok(B, cap, 0, 1), DF_E_SHAPE);
  DF_REQUIRE(map_aligned(map, 8) && map_aligned(pose, 8) && map_aligned(dst, 4), DF_E_ALIGN);
  hipLaunchKernelGGL(map_view_kernel, dim3((unsigned)((cap + 255) / 256), B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), map,
                     count, pose, cap, dst);
  DF_CHECK_LAUNCH();
  return DF_OK;
}
