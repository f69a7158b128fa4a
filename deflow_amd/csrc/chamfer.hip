// Nearest-neighbour search of the self-supervised (SeFlow) losses, and its backward: the counterpart of the reference's chamfer3D
// extension ([REF README.md:39]; UNPINNED -- the extension's source is in the absent submodule, the semantics are those of
// include/deflow_amd.h).  Not the all-pairs kernel of upstream (B x Nq x Nr ~ 8e10 pairs at the configs[2] shape) but a grid search:
//
//   df_nn_grid_build   participating ref rows -> uniform xy grid of G x G cells per sample (rows outside the range go to the clamped
//                      border cells, z is not binned): cell keys, then the library's deterministic counting sort (df_cell_sort: rows of a
//                      cell in ascending row order), then the rows copied into cell order as (x, y, z, row) so that a cell -- and a
//                      whole row of adjacent cells -- is one contiguous span
//   df_chamfer_nn      one thread per query: rings of cells around the query's own cell (ring r = the cells at Chebyshev distance r),
//                      until the distance from the query to the edge of the scanned square -- a lower bound for every row not seen yet,
//                      valid without z -- exceeds the best distance found (or max_dist2).  At most G rings: every loop is bounded by the
//                      grid's extent, whatever the input.
//                      The walk itself is nn_search.h's nn_ring_search, which df_reg_accumulate (register.hip) runs too.
//   df_chamfer_bwd     gather part: dquery[i] += 2 g_i (q_i - ref[idx_i]); scatter part: dref[k] += sum over the queries i with
//                      idx_i == k of 2 g_i (ref_k - q_i), the pairs segmented by k with the same counting sort and summed in ascending i
//                      by ONE thread per ref row -- no float atomics, a repeated call is bit-identical.
//
// Non-finite rows never reach a cell index: they do not participate (d2 = +inf, idx = -1).
#include <math.h>

#include "common.h"
#include "nn_search.h"

namespace {

constexpr uint32_t NN_DROP = 0xffffffffu;   // key of a row that does not take part (df_cell_sort drops keys >= ncells)

__global__ __launch_bounds__(256) void nn_keys_kernel(const float* __restrict__ ref, const int32_t* __restrict__ rcount,
                                                      const int32_t* __restrict__ rlabel, int Nr, float minx, float miny, float inv_cell,
                                                      int G, uint32_t* __restrict__ key) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Nr) return;
  const int64_t row = (int64_t)b * Nr + i;
  uint32_t k = NN_DROP;
  if (i < rcount[b] && (!rlabel || rlabel[row] > 0)) {
    const float x = ref[row * 3], y = ref[row * 3 + 1], z = ref[row * 3 + 2];
    if (nn_finite3(x, y, z)) {
      float px, py;
      const int cx = nn_cell(x, minx, inv_cell, G, &px), cy = nn_cell(y, miny, inv_cell, G, &py);
      k = (uint32_t)(((int64_t)b * G + cy) * G + cx);
    }
  }
  key[row] = k;
}

// rows in cell order: sorted[p] = (x, y, z, bits of the row's index inside its sample); p < total = end of the last cell
__global__ __launch_bounds__(256) void nn_gather_kernel(const float* __restrict__ ref, const uint32_t* __restrict__ idx_sorted,
                                                        const int32_t* __restrict__ cell_rng, int64_t ncells, int64_t n, int Nr,
                                                        f32x4* __restrict__ sorted) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n || p >= (int64_t)cell_rng[2 * (ncells - 1) + 1]) return;
  const uint32_t row = idx_sorted[p];
  if ((int64_t)row >= n) return;
  const int local = (int)(row % (uint32_t)Nr);
  f32x4 v;
  v.x = ref[(int64_t)row * 3];
  v.y = ref[(int64_t)row * 3 + 1];
  v.z = ref[(int64_t)row * 3 + 2];
  v.w = __builtin_bit_cast(float, local);
  sorted[p] = v;
}

__global__ __launch_bounds__(256) void chamfer_nn_kernel(const float* __restrict__ query, const int32_t* __restrict__ qcount,
                                                         const int32_t* __restrict__ qlabel, int Nq, const int32_t* __restrict__ cell_rng,
                                                         const f32x4* __restrict__ sorted, float minx, float miny, float cell, int G,
                                                         float max_dist2, float* __restrict__ d2, int32_t* __restrict__ idx,
                                                         int32_t* __restrict__ far_count) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Nq) return;
  const int64_t row = (int64_t)b * Nq + i;
  float best = INFINITY;
  int bi = -1;
  bool part = i < qcount[b] && (!qlabel || qlabel[row] > 0);
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (part) {
    qx = query[row * 3];
    qy = query[row * 3 + 1];
    qz = query[row * 3 + 2];
    part = nn_finite3(qx, qy, qz);
  }
  if (part) {
    f32x4 unused;
    const int r = nn_ring_search<false>(qx, qy, qz, cell_rng + (int64_t)b * G * G * 2, sorted, minx, miny, cell, G, max_dist2, best, bi,
                                        unused);        // (nn_search.h: the walk df_reg_accumulate runs too)
    if (far_count && r >= 2) atomicAdd(far_count, 1);
    if (!(best <= max_dist2)) {
      best = INFINITY;
      bi = -1;
    }
  }
  d2[row] = best;
  idx[row] = bi;
}

__global__ __launch_bounds__(256) void chamfer_bwd_gather_kernel(const float* __restrict__ query, const float* __restrict__ ref,
                                                                 const int32_t* __restrict__ idx, const float* __restrict__ g, int Nq,
                                                                 int Nr, float* __restrict__ dquery, uint32_t* __restrict__ key) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Nq) return;
  const int64_t row = (int64_t)b * Nq + i;
  const int k = idx[row];
  const bool ok = k >= 0 && k < Nr;
  if (key) key[row] = ok ? (uint32_t)((int64_t)b * Nr + k) : NN_DROP;
  if (!ok || !dquery) return;
  const float* q = query + row * 3;
  const float* t = ref + ((int64_t)b * Nr + k) * 3;
  const float s = 2.0f * g[row];
  float* d = dquery + row * 3;
  d[0] += s * (q[0] - t[0]);
  d[1] += s * (q[1] - t[1]);
  d[2] += s * (q[2] - t[2]);
}

// one thread per ref row: its queries, in ascending query index (df_cell_sort's order), summed in that order
__global__ __launch_bounds__(256) void chamfer_bwd_scatter_kernel(const float* __restrict__ query, const float* __restrict__ ref,
                                                                  const float* __restrict__ g, const uint32_t* __restrict__ idx_sorted,
                                                                  const int32_t* __restrict__ rng, int64_t nref, int64_t nq,
                                                                  float* __restrict__ dref) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= nref) return;
  const int s = rng[2 * k], e = rng[2 * k + 1];
  if (e <= s) return;
  const float tx = ref[k * 3], ty = ref[k * 3 + 1], tz = ref[k * 3 + 2];
  float ax = 0.f, ay = 0.f, az = 0.f;
  for (int p = s; p < e; ++p) {
    const int64_t row = (int64_t)idx_sorted[p];
    if (row >= nq) continue;
    const float w = 2.0f * g[row];
    ax += w * (tx - query[row * 3]);
    ay += w * (ty - query[row * 3 + 1]);
    az += w * (tz - query[row * 3 + 2]);
  }
  dref[k * 3] += ax;
  dref[k * 3 + 1] += ay;
  dref[k * 3 + 2] += az;
}

inline int64_t al16(int64_t v) { return (v + 15) & ~(int64_t)15; }

}  // namespace

extern "C" int64_t df_nn_grid_ws_bytes(int B, int Nr, int G) {
  if (!nn_rows_ok(B, Nr) || !nn_grid_ok(B, G)) return 0;
  return 2 * al16((int64_t)B * Nr * 4) + al16(df_cell_sort_ws_bytes((int64_t)B * G * G));
}

extern "C" int df_nn_grid_build(const float* ref, const int32_t* rcount, const int32_t* rlabel, int B, int Nr, float minx, float miny,
                                float cell, int G, int32_t* cell_rng, float* sorted, void* ws, void* stream) {
  DF_REQUIRE(ref && rcount && cell_rng && sorted && ws, DF_E_ARG);
  DF_REQUIRE(nn_rows_ok(B, Nr) && nn_grid_ok(B, G) && B <= 65535, DF_E_SHAPE);
  DF_REQUIRE(isfinite(minx) && isfinite(miny) && isfinite(cell) && cell > 0.f, DF_E_ARG);
  DF_REQUIRE(df_aligned16(sorted) && df_aligned16(ws), DF_E_ALIGN);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t n = (int64_t)B * Nr, ncells = (int64_t)B * G * G;
  char* w = reinterpret_cast<char*>(ws);
  uint32_t* key = reinterpret_cast<uint32_t*>(w);
  uint32_t* idx_sorted = reinterpret_cast<uint32_t*>(w + al16(n * 4));
  void* sort_ws = w + 2 * al16(n * 4);
  hipLaunchKernelGGL(nn_keys_kernel, dim3((Nr + 255) / 256, B), dim3(256), 0, s, ref, rcount, rlabel, Nr, minx, miny, 1.0f / cell, G, key);
  DF_CHECK_LAUNCH();
  const int rc = df_cell_sort(key, n, ncells, idx_sorted, cell_rng, sort_ws, stream);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(nn_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ref, idx_sorted, cell_rng, ncells, n, Nr,
                     reinterpret_cast<f32x4*>(sorted));
  DF_CHECK_LAUNCH();
  return DF_OK;
}

extern "C" int df_chamfer_nn(const float* query, const int32_t* qcount, const int32_t* qlabel, int B, int Nq, const int32_t* cell_rng,
                             const float* sorted, float minx, float miny, float cell, int G, float max_dist2, float* d2, int32_t* idx,
                             int32_t* far_count, void* stream) {
  DF_REQUIRE(query && qcount && cell_rng && sorted && d2 && idx, DF_E_ARG);
  DF_REQUIRE(nn_rows_ok(B, Nq) && nn_grid_ok(B, G) && B <= 65535, DF_E_SHAPE);
  DF_REQUIRE(isfinite(minx) && isfinite(miny) && isfinite(cell) && cell > 0.f && max_dist2 >= 0.f, DF_E_ARG);   // (NaN fails >=)
  DF_REQUIRE(df_aligned16(sorted), DF_E_ALIGN);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(chamfer_nn_kernel, dim3((Nq + 255) / 256, B), dim3(256), 0, s, query, qcount, qlabel, Nq, cell_rng,
                     reinterpret_cast<const f32x4*>(sorted), minx, miny, cell, G, max_dist2, d2, idx, far_count);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

extern "C" int64_t df_chamfer_bwd_ws_bytes(int B, int Nq, int Nr) {
  if (!nn_rows_ok(B, Nq) || !nn_rows_ok(B, Nr)) return 0;
  return 2 * al16((int64_t)B * Nq * 4) + al16((int64_t)B * Nr * 8) + al16(df_cell_sort_ws_bytes((int64_t)B * Nr));
}

extern "C" int df_chamfer_bwd(const float* query, const float* ref, const int32_t* idx, const float* g, int B, int Nq, int Nr,
                              float* dquery, float* dref, void* ws, void* stream) {
  DF_REQUIRE(query && ref && idx && g && (dquery || dref) && (ws || !dref), DF_E_ARG);
  DF_REQUIRE(nn_rows_ok(B, Nq) && nn_rows_ok(B, Nr) && B <= 65535, DF_E_SHAPE);
  DF_REQUIRE(!ws || df_aligned16(ws), DF_E_ALIGN);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t nq = (int64_t)B * Nq, nr = (int64_t)B * Nr;
  char* w = reinterpret_cast<char*>(ws);
  uint32_t* key = dref ? reinterpret_cast<uint32_t*>(w) : nullptr;
  hipLaunchKernelGGL(chamfer_bwd_gather_kernel, dim3((Nq + 255) / 256, B), dim3(256), 0, s, query, ref, idx, g, Nq, Nr, dquery, key);
  DF_CHECK_LAUNCH();
  if (!dref) return DF_OK;
  uint32_t* idx_sorted = reinterpret_cast<uint32_t*>(w + al16(nq * 4));
  int32_t* rng = reinterpret_cast<int32_t*>(w + 2 * al16(nq * 4));
  void* sort_ws = w + 2 * al16(nq * 4) + al16(nr * 8);
  const int rc = df_cell_sort(key, nq, nr, idx_sorted, rng, sort_ws, stream);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(chamfer_bwd_scatter_kernel, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, s, query, ref, g, idx_sorted, rng, nr,
                     nq, dref);
  DF_CHECK_LAUNCH();
  return DF_OK;
}
