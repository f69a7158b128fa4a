// Flow field on a voxel grid of model=floxels (the definition is in include/deflow_amd.h): theta holds one
// 3-vector per grid node, a row reads it trilinearly, and neighbouring active nodes are tied together by a smoothness term.
//   df_vox_plan     once per pair.  vox_coords_kernel, one thread per row: the row's cell, its three fractions and its sort key
//                   b NC + cell (the drop key for a row that does not take part).  df_cell_sort groups the rows by (sample, cell), the
//                   rows of a cell in ascending order.  vox_active_kernel, one thread per node, gathers `active` from the ranges of
//                   the node's at most 8 incident cells; vox_pairs_kernel counts the axis-adjacent active pairs from each pair's
//                   lower end and adds them with ONE integer atomic per workgroup.
//   df_vox_sample   every iteration, one thread per row: the 8 corners of the row's cell (the two x-neighbours of a corner pair are
//                   24 contiguous bytes), weights (wx wy) wz.
//   df_vox_scatter  every iteration, the exact transpose of the read in gather form: one thread per node walks its at most 8 incident
//                   cells in a fixed order and each cell's rows in ascending order; a cell of more than 128 rows is summed by the
//                   node's whole wave in a fixed shape instead (see vox_scatter_kernel).  No atomics: two calls are bit-identical and
//                   a sample's result depends on nothing but the sample.
//   df_vox_smooth   every iteration, one thread per node: the squared differences to the forward neighbours (value) and twice the
//                   differences to all of the up to 6 neighbours (gradient), both ends active.
// The corner weights and the squared lengths are formed with __fmul_rn / __fadd_rn: the file is built with -ffp-contract=on, and a
// fused multiply-add would round differently from the definition (and the read's weights must be the scatter's, bit for bit).
#include <math.h>

#include "common.h"

namespace {

constexpr uint32_t VOX_DROP = 0xffffffffu;   // key of a row that does not take part (df_cell_sort drops keys >= ncells)
constexpr int VOX_LONG = 128;                // a cell with more rows than this is summed by a whole wave in df_vox_scatter

inline int64_t vox_al16(int64_t v) { return (v + 15) & ~(int64_t)15; }
inline int64_t vox_nodes(int VX, int VY, int VZ) { return (int64_t)VX * VY * VZ; }
inline int64_t vox_cells(int VX, int VY, int VZ) { return (int64_t)(VX - 1) * (VY - 1) * (VZ - 1); }

inline bool vox_dims_ok(int B, int N, int VX, int VY, int VZ) {
  if (B < 1 || B > 65535 || N < 1 || VX < 2 || VY < 2 || VZ < 2) return false;
  const int64_t lim = (int64_t)1 << 31;
  if ((int64_t)VX * VY >= lim || vox_nodes(VX, VY, VZ) >= lim) return false;
  return 3 * (int64_t)B * N < lim && 3 * (int64_t)B * vox_nodes(VX, VY, VZ) < lim && (int64_t)B * vox_cells(VX, VY, VZ) < lim;
}
// the plan's sort addresses cells with 30-bit keys (df_cell_sort)
inline bool vox_sort_ok(int B, int VX, int VY, int VZ) { return (int64_t)B * vox_cells(VX, VY, VZ) < 0x3fffffffll; }

struct VoxAxis {
  int i;
  float t;
};

// u = (x - o) / voxel in fp32 with an IEEE division, clamped to [0, V - 1]; i = min(floor(u), V - 2), t = u - i in [0, 1]
__device__ __forceinline__ VoxAxis vox_axis(float x, float o, float voxel, int V) {
  float u = __fdiv_rn(x - o, voxel);
  u = fminf(fmaxf(u, 0.f), (float)(V - 1));
  VoxAxis a;
  a.i = min((int)floorf(u), V - 2);
  a.t = u - (float)a.i;
  return a;
}

__global__ __launch_bounds__(256) void vox_coords_kernel(const float* __restrict__ x, const int32_t* __restrict__ count, int N, float ox,
                                                         float oy, float oz, float voxel, int VX, int VY, int VZ,
                                                         int32_t* __restrict__ cell, float* __restrict__ frac, uint32_t* __restrict__ key) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int64_t row = (int64_t)b * N + i;
  int c = -1;
  float tx = 0.f, ty = 0.f, tz = 0.f;
  if (i < min(max(count[b], 0), N)) {
    const float px = x[row * 3], py = x[row * 3 + 1], pz = x[row * 3 + 2];
    if (isfinite(px) && isfinite(py) && isfinite(pz)) {
      const VoxAxis ax = vox_axis(px, ox, voxel, VX), ay = vox_axis(py, oy, voxel, VY), az = vox_axis(pz, oz, voxel, VZ);
      c = (az.i * (VY - 1) + ay.i) * (VX - 1) + ax.i;
      tx = ax.t, ty = ay.t, tz = az.t;
    }
  }
  cell[row] = c;
  frac[row * 3] = tx, frac[row * 3 + 1] = ty, frac[row * 3 + 2] = tz;
  const int64_t NC = (int64_t)(VX - 1) * (VY - 1) * (VZ - 1);
  key[row] = c < 0 ? VOX_DROP : (uint32_t)((int64_t)b * NC + c);
}

// node n of a sample -> (ix, iy, iz)
__device__ __forceinline__ void vox_node(int n, int VX, int VY, int& ix, int& iy, int& iz) {
  ix = n % VX;
  const int r = n / VX;
  iy = r % VY;
  iz = r / VY;
}

__global__ __launch_bounds__(256) void vox_active_kernel(const int32_t* __restrict__ cell_rng, int VX, int VY, int VZ,
                                                         uint8_t* __restrict__ active) {
  const int b = blockIdx.y;
  const int NV = VX * VY * VZ;
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= NV) return;
  int ix, iy, iz;
  vox_node(n, VX, VY, ix, iy, iz);
  const int64_t NC = (int64_t)(VX - 1) * (VY - 1) * (VZ - 1);
  const int32_t* rng = cell_rng + 2 * (int64_t)b * NC;
  bool on = false;
  for (int e = 0; e < 2; ++e)
    for (int d = 0; d < 2; ++d)
      for (int a = 0; a < 2; ++a) {
        const int cx = ix - a, cy = iy - d, cz = iz - e;
        if (cx < 0 || cy < 0 || cz < 0 || cx > VX - 2 || cy > VY - 2 || cz > VZ - 2) continue;
        const int64_t c = ((int64_t)cz * (VY - 1) + cy) * (VX - 1) + cx;
        on = on || rng[2 * c + 1] > rng[2 * c];
      }
  active[(int64_t)b * NV + n] = on ? 1 : 0;
}

__global__ __launch_bounds__(256) void vox_pairs_kernel(const uint8_t* __restrict__ active, int VX, int VY, int VZ,
                                                        int32_t* __restrict__ pairs) {
  __shared__ int wsum[4];
  const int b = blockIdx.y;
  const int NV = VX * VY * VZ;
  const int n = blockIdx.x * 256 + threadIdx.x;
  const uint8_t* act = active + (int64_t)b * NV;
  int c = 0;
  if (n < NV && act[n]) {
    int ix, iy, iz;
    vox_node(n, VX, VY, ix, iy, iz);
    if (ix + 1 < VX && act[n + 1]) ++c;
    if (iy + 1 < VY && act[n + VX]) ++c;
    if (iz + 1 < VZ && act[n + VX * VY]) ++c;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    if (t) atomicAdd(pairs + b, t);
  }
}

// the weight of corner (a, d, e) of a cell for a row with fractions (tx, ty, tz): (wx wy) wz, every product rounded on its own
__device__ __forceinline__ float vox_weight(float tx, float ty, float tz, int a, int d, int e) {
  const float wx = a ? tx : 1.f - tx, wy = d ? ty : 1.f - ty, wz = e ? tz : 1.f - tz;
  return __fmul_rn(__fmul_rn(wx, wy), wz);
}

__global__ __launch_bounds__(256) void vox_sample_kernel(const float* __restrict__ theta, const int32_t* __restrict__ cell,
                                                         const float* __restrict__ frac, int N, int VX, int VY, int VZ,
                                                         float* __restrict__ F) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int64_t row = (int64_t)b * N + i;
  const int c = cell[row];
  const int NC = (VX - 1) * (VY - 1) * (VZ - 1);
  float fx = 0.f, fy = 0.f, fz = 0.f;
  if (c >= 0 && c < NC) {                                             // -1: the row does not take part (no index is formed from it)
    const int ix = c % (VX - 1), r = c / (VX - 1), iy = r % (VY - 1), iz = r / (VY - 1);
    const float tx = frac[row * 3], ty = frac[row * 3 + 1], tz = frac[row * 3 + 2];
    const float* th = theta + ((int64_t)b * VX * VY * VZ + ((int64_t)iz * VY + iy) * VX + ix) * 3;
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const float* p = th + ((int64_t)e * VY + d) * VX * 3;         // the corner pair (0, d, e), (1, d, e): 6 contiguous floats
        const float w0 = vox_weight(tx, ty, tz, 0, d, e), w1 = vox_weight(tx, ty, tz, 1, d, e);
        fx += w0 * p[0], fy += w0 * p[1], fz += w0 * p[2];
        fx += w1 * p[3], fy += w1 * p[4], fz += w1 * p[5];
      }
  }
  F[row * 3] = fx, F[row * 3 + 1] = fy, F[row * 3 + 2] = fz;
}

// rows p = first, first + step, ... below end of one cell's range, added to (gx, gy, gz) one by one with the weight of corner (a, d, e)
__device__ __forceinline__ void vox_rows(const float* __restrict__ dF, const float* __restrict__ frac, const int32_t* __restrict__ idx_sorted,
                                         int first, int end, int step, int64_t lo, int64_t hi, int a, int d, int e, float& gx, float& gy,
                                         float& gz) {
  for (int p = first; p < end; p += step) {
    const int64_t r = idx_sorted[p];
    if (r < lo || r >= hi) continue;                                  // (never, for df_vox_plan's grouping)
    const float w = vox_weight(frac[r * 3], frac[r * 3 + 1], frac[r * 3 + 2], a, d, e);
    gx += w * dF[r * 3], gy += w * dF[r * 3 + 1], gz += w * dF[r * 3 + 2];
  }
}

// One thread per node.  A cell of up to VOX_LONG rows is walked by the node's own thread.  A longer one (a wall, the rows next to the
// sensor) would leave 63 lanes waiting for one: it is summed by the whole wave instead, lane l taking the rows first + l, first + l + 64,
// ..., and the 64 partial sums are added in a fixed butterfly, so the result is still a function of the cell's rows and their order alone.
__global__ __launch_bounds__(256) void vox_scatter_kernel(const float* __restrict__ dF, const float* __restrict__ frac,
                                                          const int32_t* __restrict__ idx_sorted, const int32_t* __restrict__ cell_rng,
                                                          int B, int N, int VX, int VY, int VZ, float* __restrict__ dtheta) {
  const int b = blockIdx.y;
  const int NV = VX * VY * VZ;
  const int n = blockIdx.x * 256 + threadIdx.x;
  const bool valid = n < NV;                                          // (no early return: the wave's lanes work together below)
  int ix = 0, iy = 0, iz = 0;
  if (valid) vox_node(n, VX, VY, ix, iy, iz);
  const int64_t NC = (int64_t)(VX - 1) * (VY - 1) * (VZ - 1);
  const int32_t* rng = cell_rng + 2 * (int64_t)b * NC;
  const int total = (int)min((int64_t)B * N, (int64_t)0x7fffffff);
  const int64_t lo = (int64_t)b * N, hi = lo + N;
  float gx = 0.f, gy = 0.f, gz = 0.f;
  unsigned longmask = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {                                       // the node is corner (a, d, e) of the cell at (ix - a, iy - d, iz - e)
    const int a = k & 1, d = (k >> 1) & 1, e = k >> 2;
    const int cx = ix - a, cy = iy - d, cz = iz - e;
    if (!valid || cx < 0 || cy < 0 || cz < 0 || cx > VX - 2 || cy > VY - 2 || cz > VZ - 2) continue;
    const int64_t c = ((int64_t)cz * (VY - 1) + cy) * (VX - 1) + cx;
    const int s = max(rng[2 * c], 0), t = min(rng[2 * c + 1], total);
    if (t - s > VOX_LONG) longmask |= 1u << k;
    else vox_rows(dF, frac, idx_sorted, s, t, 1, lo, hi, a, d, e, gx, gy, gz);
  }
  if (__ballot(longmask != 0)) {                                      // (wave-uniform)
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int a = k & 1, d = (k >> 1) & 1, e = k >> 2;
      const bool mine = (longmask >> k) & 1;
      int s = 0, t = 0;
      if (mine) {
        const int64_t c = ((int64_t)(iz - e) * (VY - 1) + (iy - d)) * (VX - 1) + (ix - a);
        s = max(rng[2 * c], 0), t = min(rng[2 * c + 1], total);
      }
      unsigned long long m = __ballot(mine);
      while (m) {                                                     // the lanes with a long cell in this slot, in ascending order
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int ss = __shfl(s, src, 64), tt = __shfl(t, src, 64);
        float px = 0.f, py = 0.f, pz = 0.f;
        vox_rows(dF, frac, idx_sorted, ss + lane, tt, 64, lo, hi, a, d, e, px, py, pz);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          px = __fadd_rn(px, __shfl_xor(px, o, 64)), py = __fadd_rn(py, __shfl_xor(py, o, 64)), pz = __fadd_rn(pz, __shfl_xor(pz, o, 64));
        }
        if (lane == src) gx += px, gy += py, gz += pz;
      }
    }
  }
  if (!valid) return;
  float* o = dtheta + ((int64_t)b * NV + n) * 3;
  o[0] = gx, o[1] = gy, o[2] = gz;
}

struct VoxSm {
  float gx, gy, gz;
};

// the difference theta_n - theta_q to one active neighbour: its doubled components are added to g and its squared length is returned
__device__ __forceinline__ float vox_diff(const float* __restrict__ tn, const float* __restrict__ tq, VoxSm& g) {
  const float dx = tn[0] - tq[0], dy = tn[1] - tq[1], dz = tn[2] - tq[2];
  g.gx = __fadd_rn(g.gx, 2.f * dx), g.gy = __fadd_rn(g.gy, 2.f * dy), g.gz = __fadd_rn(g.gz, 2.f * dz);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

__global__ __launch_bounds__(256) void vox_smooth_kernel(const float* __restrict__ theta, const uint8_t* __restrict__ active, int VX, int VY,
                                                         int VZ, float* __restrict__ v, float* __restrict__ g) {
  const int b = blockIdx.y;
  const int NV = VX * VY * VZ;
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= NV) return;
  const uint8_t* act = active + (int64_t)b * NV;
  const float* th = theta + (int64_t)b * NV * 3;
  float val = 0.f;
  VoxSm a = {0.f, 0.f, 0.f};
  if (act[n]) {
    int ix, iy, iz;
    vox_node(n, VX, VY, ix, iy, iz);
    const float* tn = th + (int64_t)n * 3;
    const int sy = VX, sz = VX * VY;
    // backward, then forward neighbour of every axis; only the forward ones count into the value
    if (ix > 0 && act[n - 1]) vox_diff(tn, tn - 3, a);
    if (ix + 1 < VX && act[n + 1]) val = __fadd_rn(val, vox_diff(tn, tn + 3, a));
    if (iy > 0 && act[n - sy]) vox_diff(tn, tn - (int64_t)sy * 3, a);
    if (iy + 1 < VY && act[n + sy]) val = __fadd_rn(val, vox_diff(tn, tn + (int64_t)sy * 3, a));
    if (iz > 0 && act[n - sz]) vox_diff(tn, tn - (int64_t)sz * 3, a);
    if (iz + 1 < VZ && act[n + sz]) val = __fadd_rn(val, vox_diff(tn, tn + (int64_t)sz * 3, a));
  }
  const int64_t o = (int64_t)b * NV + n;
  v[o] = val;
  g[o * 3] = a.gx, g[o * 3 + 1] = a.gy, g[o * 3 + 2] = a.gz;
}

inline bool vox_al4(const void* p) { return (((uintptr_t)p) & 3u) == 0; }

}  // namespace

extern "C" {

int64_t df_vox_plan_ws_bytes(int B, int N, int VX, int VY, int VZ) {
  if (!vox_dims_ok(B, N, VX, VY, VZ) || !vox_sort_ok(B, VX, VY, VZ)) return -1;
  return vox_al16((int64_t)B * N * 4) + vox_al16(df_cell_sort_ws_bytes((int64_t)B * vox_cells(VX, VY, VZ)));
}

int df_vox_plan(const float* x, const int32_t* count, int B, int N, float ox, float oy, float oz, float voxel, int VX, int VY, int VZ,
                int32_t* cell, float* frac, int32_t* idx_sorted, int32_t* cell_rng, uint8_t* active, int32_t* pairs, void* ws,
                void* stream) {
  DF_REQUIRE(vox_dims_ok(B, N, VX, VY, VZ) && vox_sort_ok(B, VX, VY, VZ), DF_E_SHAPE);
  DF_REQUIRE(x && count && cell && frac && idx_sorted && cell_rng && active && pairs && ws, DF_E_ARG);
  DF_REQUIRE(voxel > 0.f && voxel <= 3.0e38f && ox == ox && oy == oy && oz == oz, DF_E_ARG);      // (NaN fails the comparisons)
  DF_REQUIRE(df_aligned16(ws) && vox_al4(x) && vox_al4(count) && vox_al4(cell) && vox_al4(frac) && vox_al4(idx_sorted) && vox_al4(cell_rng) &&
                 vox_al4(pairs),
             DF_E_ALIGN);
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = (int64_t)B * N, ncells = (int64_t)B * vox_cells(VX, VY, VZ);
  const int NV = (int)vox_nodes(VX, VY, VZ);
  char* w = reinterpret_cast<char*>(ws);
  uint32_t* key = reinterpret_cast<uint32_t*>(w);
  void* sort_ws = w + vox_al16(n * 4);
  hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(pairs), 0, (size_t)B, st);
  if (e != hipSuccess) return (int)e;
  e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(idx_sorted), -1, (size_t)n, st);      // the slots behind the grouped rows: -1
  if (e != hipSuccess) return (int)e;
  vox_coords_kernel<<<dim3((N + 255) / 256, B), 256, 0, st>>>(x, count, N, ox, oy, oz, voxel, VX, VY, VZ, cell, frac, key);
  DF_CHECK_LAUNCH();
  const int rc = df_cell_sort(key, n, ncells, reinterpret_cast<uint32_t*>(idx_sorted), cell_rng, sort_ws, stream);
  if (rc != 0) return rc;
  const dim3 grid((NV + 255) / 256, B);
  vox_active_kernel<<<grid, 256, 0, st>>>(cell_rng, VX, VY, VZ, active);
  DF_CHECK_LAUNCH();
  vox_pairs_kernel<<<grid, 256, 0, st>>>(active, VX, VY, VZ, pairs);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

int df_vox_sample(const float* theta, const int32_t* cell, const float* frac, int B, int N, int VX, int VY, int VZ, float* F, void* stream) {
  DF_REQUIRE(vox_dims_ok(B, N, VX, VY, VZ), DF_E_SHAPE);
  DF_REQUIRE(theta && cell && frac && F, DF_E_ARG);
  DF_REQUIRE(vox_al4(theta) && vox_al4(cell) && vox_al4(frac) && vox_al4(F), DF_E_ALIGN);
  vox_sample_kernel<<<dim3((N + 255) / 256, B), 256, 0, (hipStream_t)stream>>>(theta, cell, frac, N, VX, VY, VZ, F);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

int df_vox_scatter(const float* dF, const float* frac, const int32_t* idx_sorted, const int32_t* cell_rng, int B, int N, int VX, int VY,
                   int VZ, float* dtheta, void* stream) {
  DF_REQUIRE(vox_dims_ok(B, N, VX, VY, VZ), DF_E_SHAPE);
  DF_REQUIRE(dF && frac && idx_sorted && cell_rng && dtheta, DF_E_ARG);
  DF_REQUIRE(vox_al4(dF) && vox_al4(frac) && vox_al4(idx_sorted) && vox_al4(cell_rng) && vox_al4(dtheta), DF_E_ALIGN);
  const int NV = (int)vox_nodes(VX, VY, VZ);
  vox_scatter_kernel<<<dim3((NV + 255) / 256, B), 256, 0, (hipStream_t)stream>>>(dF, frac, idx_sorted, cell_rng, B, N, VX, VY, VZ, dtheta);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

int df_vox_smooth(const float* theta, const uint8_t* active, int B, int VX, int VY, int VZ, float* v, float* g, void* stream) {
  DF_REQUIRE(vox_dims_ok(B, 1, VX, VY, VZ), DF_E_SHAPE);
  DF_REQUIRE(theta && active && v && g, DF_E_ARG);
  DF_REQUIRE(vox_al4(theta) && vox_al4(v) && vox_al4(g), DF_E_ALIGN);
  const int NV = (int)vox_nodes(VX, VY, VZ);
  vox_smooth_kernel<<<dim3((NV + 255) / 256, B), 256, 0, (hipStream_t)stream>>>(theta, active, VX, VY, VZ, v, g);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

}  // extern "C"
