// DBSCAN over a padded batch of clouds: the cluster labels of the self-supervised (SeFlow) mode computed on the GPU.  UNPINNED -- upstream
// clusters offline on the CPU with HDBSCAN (absent submodule); this is plain DBSCAN with every choice fixed (include/deflow_amd.h,
// DESIGN.md section 6b), so that the labels are a pure function of the input.  All three stages walk the grid of df_nn_grid_build
// (chamfer.hip) with cell >= eps: the cells that a row's clamped position +- (eps / cell + 2e-3) covers in x and in y (nn_search.h:
// nn_window) -- one contiguous span of the cell-ordered rows per cell row, three of them, four for a row within the slack of a cell
// edge -- hold every row within eps.  NOT "the 3 x 3 cells around its own": at cell == eps fp32 files two rows a hair less than one
// cell apart two cells apart where the cell coordinate crosses a power of two.  Rows outside the range sit in the clamped border
// cells and still meet all their neighbours (clamping is a contraction).
//
//   df_dbscan_core     one thread per cell-ordered row: counts the rows within eps (stops at min_points) and writes the row again with the
//                      core flag in the top bit of its index word, so that the later passes read one 16-byte record per candidate
//   df_dbscan_link     union-find over the core rows: a core row unites with every core candidate of LOWER row index within eps; the
//                      larger root is hooked under the smaller by an integer compare-and-swap, finds halve their path with an integer
//                      atomic min.  A parent is always a smaller row, so the final root of a component is its lowest row whatever the
//                      launch order: the result is deterministic without a host loop.
//   df_dbscan_finish   roots of the core rows, border rows to the component of their nearest core row (lowest row on equal distances),
//                      members / flagged members per root (integer atomic adds), the two filters, the survivors numbered 1..K in
//                      ascending order of their root by a two-level prefix sum, labels.
//
// Every loop is bounded: cell scans by the sample's rows, walks to a root by N (parents strictly decrease), compare-and-swap retries by
// 2 N (each failed attempt lowers one of the two roots).  A loop that reaches its bound adds 1 to the status word and carries on.
#include <math.h>

#include "common.h"
#include "nn_search.h"

namespace {

constexpr uint32_t CL_CORE = 0x80000000u;     // top bit of a record's index word (row indices stay below 2^30)
constexpr int CL_ROWS = 5;                    // cell rows at the offsets -2 .. 2 from a row's own: the window covers three or four

__device__ __forceinline__ uint32_t cl_bits(const f32x4& v) {
  const float w = v.w;
  return __builtin_bit_cast(uint32_t, w);
}

__device__ __forceinline__ float cl_d2(const f32x4& v, float x, float y, float z) {
  const float dx = v.x - x, dy = v.y - y, dz = v.z - z;
  return dx * dx + dy * dy + dz * dz;
}

// the window of the row (x, y): for each of the cell rows at the FIXED offsets -2 .. 2 from its own one span [s, e) of cell-ordered
// positions, clipped to the sample's own positions [s0, e0); empty for a cell row outside nn_window's ya .. yb (nn_search.h)
struct ClWindow {
  int s[CL_ROWS], e[CL_ROWS];
};
__device__ __forceinline__ ClWindow cl_window(const int32_t* __restrict__ rng, int G, float x, float y, float minx, float miny,
                                              float inv_cell, float reach, int s0, int e0) {
  ClWindow w;
  float px, py;
  nn_cell(x, minx, inv_cell, G, &px);
  const int cy = nn_cell(y, miny, inv_cell, G, &py);
  const NnWindow win = nn_window(px, py, reach, G);
#pragma unroll
  for (int k = 0; k < CL_ROWS; ++k) {
    const int yy = cy - 2 + k;
    int s = 0, e = 0;
    if (yy >= win.ya && yy <= win.yb) {
      const int32_t* rr = rng + (int64_t)yy * G * 2;
      s = max(rr[2 * win.xa], s0);
      e = min(rr[2 * win.xb + 1], e0);
    }
    w.s[k] = s;
    w.e[k] = e;
  }
  return w;
}

// positions of sample b in the cell-ordered rows
__device__ __forceinline__ void cl_sample_span(const int32_t* __restrict__ rng, int G, int N, int* s0, int* e0) {
  const int s = rng[0];
  int e = rng[2 * ((int64_t)G * G - 1) + 1];
  if (e > s + N) e = s + N;
  *s0 = s;
  *e0 = e;
}

__global__ __launch_bounds__(256) void cl_init_kernel(int N, int32_t* __restrict__ parent, int32_t* __restrict__ root,
                                                      int32_t* __restrict__ members, int32_t* __restrict__ flagged) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int64_t g = (int64_t)b * N + i;
  parent[g] = i;
  root[g] = -1;
  members[g] = 0;
  flagged[g] = 0;
}

__global__ __launch_bounds__(256) void cl_core_kernel(const int32_t* __restrict__ cell_rng, const f32x4* __restrict__ sorted, int N,
                                                      float minx, float miny, float inv_cell, int G, float eps2, float reach, int min_points,
                                                      f32x4* __restrict__ rec) {
  const int b = blockIdx.y;
  const int32_t* rng = cell_rng + (int64_t)b * G * G * 2;
  int s0, e0;
  cl_sample_span(rng, G, N, &s0, &e0);
  const int p = s0 + blockIdx.x * 256 + threadIdx.x;
  if (p >= e0) return;
  f32x4 me = sorted[p];
  const ClWindow w = cl_window(rng, G, me.x, me.y, minx, miny, inv_cell, reach, s0, e0);
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < CL_ROWS; ++k) {
    for (int q = w.s[k]; q < w.e[k] && cnt < min_points; ++q) cnt += cl_d2(sorted[q], me.x, me.y, me.z) <= eps2 ? 1 : 0;
  }
  const uint32_t word = (cl_bits(me) & ~CL_CORE) | (cnt >= min_points ? CL_CORE : 0u);
  me.w = __builtin_bit_cast(float, word);
  rec[p] = me;
}

__device__ __forceinline__ int cl_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x with path halving.  Whatever value parent[x] ever held other than x is an ancestor of x for good (trees are only ever hooked
// at their roots), so a late or repeated min only shortens the path.
__device__ __forceinline__ int cl_find(int32_t* __restrict__ par, int x, int bound, int32_t* __restrict__ status) {
  for (int it = 0; it < bound; ++it) {
    const int p = cl_load(par + x);
    if (p == x) return x;
    const int gp = cl_load(par + p);
    if (gp == p) return p;
    atomicMin(par + x, gp);
    x = gp;
  }
  if (status) atomicAdd(status, 1);
  return x;
}

// read-only walk (after the link pass: the forest no longer changes)
__device__ __forceinline__ int cl_root(const int32_t* __restrict__ par, int x, int bound, int32_t* __restrict__ status) {
  for (int it = 0; it < bound; ++it) {
    const int p = par[x];
    if (p == x) return x;
    x = p;
  }
  if (status) atomicAdd(status, 1);
  return x;
}

__device__ __forceinline__ int cl_unite(int32_t* __restrict__ par, int a, int b, int bound, int32_t* __restrict__ status) {
  for (int it = 0; it < 2 * bound; ++it) {
    a = cl_find(par, a, bound, status);
    b = cl_find(par, b, bound, status);
    if (a == b) return a;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomicCAS(par + hi, hi, lo);
    if (old == hi) return lo;
    a = old;                     // somebody hooked hi first: old < hi is its parent now
    b = lo;
  }
  if (status) atomicAdd(status, 1);
  return a < b ? a : b;
}

__global__ __launch_bounds__(256) void cl_link_kernel(const int32_t* __restrict__ cell_rng, const f32x4* __restrict__ rec, int N,
                                                      float minx, float miny, float inv_cell, int G, float eps2, float reach,
                                                      int32_t* __restrict__ parent, int32_t* __restrict__ status) {
  const int b = blockIdx.y;
  const int32_t* rng = cell_rng + (int64_t)b * G * G * 2;
  int s0, e0;
  cl_sample_span(rng, G, N, &s0, &e0);
  const int p = s0 + blockIdx.x * 256 + threadIdx.x;
  if (p >= e0) return;
  const f32x4 me = rec[p];
  const uint32_t mw = cl_bits(me);
  if (!(mw & CL_CORE)) return;
  const int row = (int)(mw & ~CL_CORE);
  if (row >= N) return;
  int32_t* par = parent + (int64_t)b * N;
  const ClWindow w = cl_window(rng, G, me.x, me.y, minx, miny, inv_cell, reach, s0, e0);
  int ra = row;
#pragma unroll
  for (int k = 0; k < CL_ROWS; ++k) {
    for (int q = w.s[k]; q < w.e[k]; ++q) {
      const f32x4 v = rec[q];
      const uint32_t vw = cl_bits(v);
      const int j = (int)(vw & ~CL_CORE);
      if (!(vw & CL_CORE) || j >= row) continue;
      if (cl_d2(v, me.x, me.y, me.z) <= eps2) ra = cl_unite(par, ra, j, N, status);
    }
  }
}

__global__ __launch_bounds__(256) void cl_attach_kernel(const int32_t* __restrict__ cell_rng, const f32x4* __restrict__ rec,
                                                        const int32_t* __restrict__ dynamic, int N, float minx, float miny,
                                                        float inv_cell, int G, float eps2, float reach, const int32_t* __restrict__ parent,
                                                        int32_t* __restrict__ root, int32_t* __restrict__ members,
                                                        int32_t* __restrict__ flagged, int32_t* __restrict__ status) {
  const int b = blockIdx.y;
  const int32_t* rng = cell_rng + (int64_t)b * G * G * 2;
  int s0, e0;
  cl_sample_span(rng, G, N, &s0, &e0);
  const int p = s0 + blockIdx.x * 256 + threadIdx.x;
  if (p >= e0) return;
  const f32x4 me = rec[p];
  const uint32_t mw = cl_bits(me);
  const int row = (int)(mw & ~CL_CORE);
  if (row >= N) return;
  int target = -1;
  if (mw & CL_CORE) {
    target = row;
  } else {
    const ClWindow w = cl_window(rng, G, me.x, me.y, minx, miny, inv_cell, reach, s0, e0);
    float best = INFINITY;
#pragma unroll
    for (int k = 0; k < CL_ROWS; ++k) {
      for (int q = w.s[k]; q < w.e[k]; ++q) {
        const f32x4 v = rec[q];
        const uint32_t vw = cl_bits(v);
        if (!(vw & CL_CORE)) continue;
        const int j = (int)(vw & ~CL_CORE);
        const float d = cl_d2(v, me.x, me.y, me.z);
        if (d <= eps2 && (d < best || (d == best && j < target))) {
          best = d;
          target = j;
        }
      }
    }
  }
  if (target < 0 || target >= N) return;             // noise: root stays -1
  const int64_t base = (int64_t)b * N;
  const int r = cl_root(parent + base, target, N, status);
  root[base + row] = r;
  atomicAdd(members + base + r, 1);
  if (dynamic && dynamic[base + row] != 0) atomicAdd(flagged + base + r, 1);
}

// keep[g] = 1 for the root of a surviving cluster; blk_sum[b, blk] = survivors among the 256 rows of the block
__global__ __launch_bounds__(256) void cl_filter_kernel(int N, const int32_t* __restrict__ members, const int32_t* __restrict__ flagged,
                                                        int use_flag, int min_cluster_size, double min_dynamic_frac,
                                                        int32_t* __restrict__ keep, int32_t* __restrict__ blk_sum) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  int k = 0;
  if (i < N) {
    const int64_t g = (int64_t)b * N + i;
    const int m = members[g];
    k = m > 0 && m >= min_cluster_size;
    if (k && use_flag && (double)flagged[g] < min_dynamic_frac * (double)m) k = 0;      // float64: the comparison the definition states
    keep[g] = k;
  }
  const int total = __syncthreads_count(k);
  if (threadIdx.x == 0) blk_sum[(int64_t)b * gridDim.x + blockIdx.x] = total;
}

// rank[g] = 1-based number of the surviving root g among the survivors of its sample in ascending row order (0 elsewhere)
__global__ __launch_bounds__(256) void cl_rank_kernel(int N, const int32_t* __restrict__ keep, const int32_t* __restrict__ blk_sum,
                                                      int32_t* __restrict__ rank, int32_t* __restrict__ n_clusters) {
  __shared__ int red[4];
  __shared__ int wsum[4];
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t* bs = blk_sum + (int64_t)b * gridDim.x;
  int before = 0;
  for (int k = threadIdx.x; k < (int)blockIdx.x; k += 256) before += bs[k];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
  const int k = i < N ? keep[(int64_t)b * N + i] : 0;
  const unsigned long long m = __ballot(k != 0);
  const int within = __popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) {
    red[wave] = before;
    wsum[wave] = __popcll(m);
  }
  __syncthreads();
  int base = red[0] + red[1] + red[2] + red[3];
  for (int v = 0; v < wave; ++v) base += wsum[v];
  if (i < N) rank[(int64_t)b * N + i] = k ? base + within + 1 : 0;
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0)
    n_clusters[b] = red[0] + red[1] + red[2] + red[3] + wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(256) void cl_label_kernel(int N, const int32_t* __restrict__ root, const int32_t* __restrict__ rank,
                                                       int32_t* __restrict__ labels) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int64_t base = (int64_t)b * N;
  const int r = root[base + i];
  labels[base + i] = (r >= 0 && r < N) ? rank[base + r] : 0;
}

inline int64_t cl_al16(int64_t v) { return (v + 15) & ~(int64_t)15; }
// the same limits as the chamfer entries: 32-bit sorted positions and keys
inline bool cl_rows_ok(int B, int N) { return B > 0 && N > 0 && (int64_t)B * N < 0x3fffffffll && B <= 65535; }
inline bool cl_grid_ok(int B, int G) { return G > 0 && G <= 4096 && (int64_t)B * G * G < 0x3fffffffll; }
inline bool cl_geom_ok(float minx, float miny, float cell, float eps) {
  return isfinite(minx) && isfinite(miny) && isfinite(cell) && isfinite(eps) && eps > 0.f && cell >= eps;
}

// nn_window's reach: eps in cells plus the slack for the fp32 rounding of the cell coordinates (<= 1.002 with cell >= eps)
inline float cl_reach(float eps, float cell) { return eps * (1.0f / cell) + 2e-3f; }

// the workspace the three stages share
struct ClWs {
  f32x4* rec;
  int32_t *parent, *root, *members, *flagged, *keep, *rank, *blk_sum;
};
inline ClWs cl_ws(void* ws, int B, int N) {
  const int64_t n = (int64_t)B * N, a = cl_al16(n * 4);
  char* w = reinterpret_cast<char*>(ws);
  ClWs s;
  s.rec = reinterpret_cast<f32x4*>(w);
  w += cl_al16(n * 16);
  s.parent = reinterpret_cast<int32_t*>(w);
  s.root = reinterpret_cast<int32_t*>(w + a);
  s.members = reinterpret_cast<int32_t*>(w + 2 * a);
  s.flagged = reinterpret_cast<int32_t*>(w + 3 * a);
  s.keep = reinterpret_cast<int32_t*>(w + 4 * a);
  s.rank = reinterpret_cast<int32_t*>(w + 5 * a);
  s.blk_sum = reinterpret_cast<int32_t*>(w + 6 * a);
  return s;
}

}  // namespace

extern "C" int64_t df_dbscan_ws_bytes(int B, int N) {
  if (!cl_rows_ok(B, N)) return 0;
  const int64_t n = (int64_t)B * N;
  return cl_al16(n * 16) + 6 * cl_al16(n * 4) + cl_al16((int64_t)B * ((N + 255) / 256) * 4);
}

extern "C" int df_dbscan_core(const int32_t* cell_rng, const float* sorted, int B, int N, float minx, float miny, float cell, int G,
                              float eps, int min_points, void* ws, void* stream) {
  DF_REQUIRE(cell_rng && sorted && ws, DF_E_ARG);
  DF_REQUIRE(cl_rows_ok(B, N) && cl_grid_ok(B, G), DF_E_SHAPE);
  DF_REQUIRE(cl_geom_ok(minx, miny, cell, eps) && min_points >= 1, DF_E_ARG);
  DF_REQUIRE(df_aligned16(sorted) && df_aligned16(ws), DF_E_ALIGN);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const ClWs w = cl_ws(ws, B, N);
  const dim3 grid((N + 255) / 256, B);
  hipLaunchKernelGGL(cl_init_kernel, grid, dim3(256), 0, s, N, w.parent, w.root, w.members, w.flagged);
  DF_CHECK_LAUNCH();
  hipLaunchKernelGGL(cl_core_kernel, grid, dim3(256), 0, s, cell_rng, reinterpret_cast<const f32x4*>(sorted), N, minx, miny, 1.0f / cell,
                     G, eps * eps, cl_reach(eps, cell), min_points, w.rec);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

extern "C" int df_dbscan_link(const int32_t* cell_rng, int B, int N, float minx, float miny, float cell, int G, float eps,
                              int32_t* status, void* ws, void* stream) {
  DF_REQUIRE(cell_rng && ws, DF_E_ARG);
  DF_REQUIRE(cl_rows_ok(B, N) && cl_grid_ok(B, G), DF_E_SHAPE);
  DF_REQUIRE(cl_geom_ok(minx, miny, cell, eps), DF_E_ARG);
  DF_REQUIRE(df_aligned16(ws), DF_E_ALIGN);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const ClWs w = cl_ws(ws, B, N);
  hipLaunchKernelGGL(cl_link_kernel, dim3((N + 255) / 256, B), dim3(256), 0, s, cell_rng, w.rec, N, minx, miny, 1.0f / cell, G, eps * eps,
                     cl_reach(eps, cell), w.parent, status);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

extern "C" int df_dbscan_finish(const int32_t* cell_rng, const int32_t* dynamic, int B, int N, float minx, float miny, float cell, int G,
                                float eps, int min_cluster_size, double min_dynamic_frac, int32_t* labels, int32_t* n_clusters,
                                int32_t* status, void* ws, void* stream) {
  DF_REQUIRE(cell_rng && labels && n_clusters && ws, DF_E_ARG);
  DF_REQUIRE(cl_rows_ok(B, N) && cl_grid_ok(B, G), DF_E_SHAPE);
  DF_REQUIRE(cl_geom_ok(minx, miny, cell, eps) && min_cluster_size >= 1 && min_dynamic_frac >= 0.0 && isfinite(min_dynamic_frac), DF_E_ARG);
  DF_REQUIRE(df_aligned16(ws), DF_E_ALIGN);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const ClWs w = cl_ws(ws, B, N);
  const dim3 grid((N + 255) / 256, B);
  hipLaunchKernelGGL(cl_attach_kernel, grid, dim3(256), 0, s, cell_rng, w.rec, dynamic, N, minx, miny, 1.0f / cell, G, eps * eps,
                     cl_reach(eps, cell), w.parent, w.root, w.members, w.flagged, status);
  DF_CHECK_LAUNCH();
  hipLaunchKernelGGL(cl_filter_kernel, grid, dim3(256), 0, s, N, w.members, w.flagged, dynamic ? 1 : 0, min_cluster_size, min_dynamic_frac,
                     w.keep, w.blk_sum);
  DF_CHECK_LAUNCH();
  hipLaunchKernelGGL(cl_rank_kernel, grid, dim3(256), 0, s, N, w.keep, w.blk_sum, w.rank, n_clusters);
  DF_CHECK_LAUNCH();
  hipLaunchKernelGGL(cl_label_kernel, grid, dim3(256), 0, s, N, w.root, w.rank, labels);
  DF_CHECK_LAUNCH();
  return DF_OK;
}
