// Truncated squared Euclidean distance transform of a voxelised cloud and its trilinear lookup (model=fastnsf, DESIGN.md section 6l;
// the definition is in include/deflow_amd.h).  Memory-bound stencil and gather kernels:
//   df_dt_build   clear -> mark -> three separable windowed min-plus passes, x then y then z, ping-pong between the workspace and dt2.
//                 Every pass reads and writes u16; the sums k*k + prev are formed in 32-bit registers and saturated at R*R (a partial
//                 above R*R can never reach the result).  Integer arithmetic: the result does not depend on any order.
//   df_dt_lookup  one thread per row: eight 2-byte reads, the interpolant of cell * sqrt(dt2) and its analytic gradient.
// A block is one line tile: DT_TILE consecutive x of one (b, z, y) line, so every access of every pass is coalesced along x and the
// line / axis position of a block is scalar arithmetic.  The x pass stages DT_TILE + 2R values in LDS; the y and z passes read their
// 2R+1 neighbours (other lines at the same x) straight from global memory.
#include "common.h"

namespace {

constexpr int DT_TILE = 256;     // x positions per block (= threads per block)
constexpr int DT_RMAX = 255;     // R*R <= 65025 fits 16 bits

__global__ __launch_bounds__(256) void dt_clear_kernel(uint4* __restrict__ buf, int64_t n16, unsigned sat2) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n16) buf[i] = make_uint4(sat2, sat2, sat2, sat2);
}

// occupancy: voxel floor((p - o) / cell) per axis in fp32 with an IEEE division (the voxeliser's rule); the comparison is made on the
// float, so no index is formed from a row outside the grid or a non-finite row.  Racing stores write the same constant.
__global__ __launch_bounds__(256) void dt_mark_kernel(const float* __restrict__ ref, const int32_t* __restrict__ count, int N, float ox,
                                                      float oy, float oz, float cell, int GX, int GY, int GZ, uint16_t* __restrict__ occ) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int c = min(max(count[b], 0), N);
  if (i >= c) return;
  const float* p = ref + ((int64_t)b * N + i) * 3;
  const float fx = floorf((p[0] - ox) / cell), fy = floorf((p[1] - oy) / cell), fz = floorf((p[2] - oz) / cell);
  if (!(fx >= 0.f && fx < (float)GX && fy >= 0.f && fy < (float)GY && fz >= 0.f && fz < (float)GZ)) return;   // NaN fails every comparison
  occ[(((int64_t)b * GZ + (int)fz) * GY + (int)fy) * GX + (int)fx] = 0;
}

// x pass: dst[line][x] = min(sat, min over |k| <= R of k*k + src[line][x + k]); positions outside the line count as sat
__global__ __launch_bounds__(256) void dt_pass_x_kernel(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, int GX, int tiles, int R,
                                                        int sat) {
  __shared__ uint16_t line_s[DT_TILE + 2 * DT_RMAX];
  const int64_t line = blockIdx.x / tiles;
  const int x0 = (int)(blockIdx.x % tiles) * DT_TILE;
  const uint16_t* s = src + line * GX;
  for (int j = threadIdx.x; j < DT_TILE + 2 * R; j += 256) {          // at most 3 rounds
    const int x = x0 - R + j;
    line_s[j] = (x >= 0 && x < GX) ? s[x] : (uint16_t)sat;
  }
  __syncthreads();
  const int x = x0 + threadIdx.x;
  if (x >= GX) return;
  int m = sat;
  for (int k = -R; k <= R; ++k) m = min(m, k * k + (int)line_s[threadIdx.x + R + k]);
  dst[line * GX + x] = (uint16_t)m;
}

// y pass (div = 1, ext = GY, stride = GX) and z pass (div = GY, ext = GZ, stride = GX * GY): the neighbours are whole lines apart
__global__ __launch_bounds__(256) void dt_pass_line_kernel(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, int GX, int tiles,
                                                           int div, int ext, int64_t stride, int R, int sat) {
  const int64_t line = blockIdx.x / tiles;
  const int x = (int)(blockIdx.x % tiles) * DT_TILE + threadIdx.x;
  if (x >= GX) return;
  const int pos = (int)((line / div) % ext);
  const int lo = max(-R, -pos), hi = min(R, ext - 1 - pos);
  const uint16_t* s = src + line * GX + x;
  int m = sat;
  for (int k = lo; k <= hi; ++k) m = min(m, k * k + (int)s[k * stride]);
  dst[line * GX + x] = (uint16_t)m;
}

struct DtAxis {
  int i;      // lower corner
  float t;    // position inside the cell (0..1 after the clamp)
  bool clamped;
};

__device__ __forceinline__ DtAxis dt_axis(float q, float o, float cell, int G) {
  float u = (q - o) / cell - 0.5f;
  const float top = (float)(G - 1);
  DtAxis a;
  a.clamped = u < 0.f || u > top;
  u = fminf(fmaxf(u, 0.f), top);
  a.i = min((int)floorf(u), G - 2);
  a.t = u - (float)a.i;
  return a;
}

__global__ __launch_bounds__(256) void dt_lookup_kernel(const float* __restrict__ query, const int32_t* __restrict__ count,
                                                        const uint16_t* __restrict__ dt2, int N, float ox, float oy, float oz, float cell,
                                                        int GX, int GY, int GZ, int R, float* __restrict__ d, float* __restrict__ g,
                                                        int32_t* __restrict__ cells, uint8_t* __restrict__ clamped) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int64_t row = (int64_t)b * N + i;
  float dv = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
  int cx = 0, cy = 0, cz = 0, cl = 0;
  if (i < min(max(count[b], 0), N)) {
    const float qx = query[row * 3], qy = query[row * 3 + 1], qz = query[row * 3 + 2];
    if (isfinite(qx) && isfinite(qy) && isfinite(qz)) {
      const DtAxis ax = dt_axis(qx, ox, cell, GX), ay = dt_axis(qy, oy, cell, GY), az = dt_axis(qz, oz, cell, GZ);
      cx = ax.i, cy = ay.i, cz = az.i;
      cl = (ax.clamped ? 1 : 0) | (ay.clamped ? 2 : 0) | (az.clamped ? 4 : 0);
      const uint16_t* p = dt2 + (((int64_t)b * GZ + cz) * GY + cy) * GX + cx;
      const int64_t sy = GX, sz = (int64_t)GX * GY;
      const float v000 = cell * sqrtf((float)p[0]), v100 = cell * sqrtf((float)p[1]);
      const float v010 = cell * sqrtf((float)p[sy]), v110 = cell * sqrtf((float)p[sy + 1]);
      const float v001 = cell * sqrtf((float)p[sz]), v101 = cell * sqrtf((float)p[sz + 1]);
      const float v011 = cell * sqrtf((float)p[sz + sy]), v111 = cell * sqrtf((float)p[sz + sy + 1]);
      const float tx = ax.t, ty = ay.t, tz = az.t, ux = 1.f - tx, uy = 1.f - ty, uz = 1.f - tz;
      // along x, then y, then z
      const float e00 = v000 * ux + v100 * tx, e10 = v010 * ux + v110 * tx, e01 = v001 * ux + v101 * tx, e11 = v011 * ux + v111 * tx;
      const float f0 = e00 * uy + e10 * ty, f1 = e01 * uy + e11 * ty;
      dv = f0 * uz + f1 * tz;
      const float dx0 = (v100 - v000) * uy + (v110 - v010) * ty, dx1 = (v101 - v001) * uy + (v111 - v011) * ty;
      gx = ax.clamped ? 0.f : (dx0 * uz + dx1 * tz) / cell;
      gy = ay.clamped ? 0.f : ((e10 - e00) * uz + (e11 - e01) * tz) / cell;
      gz = az.clamped ? 0.f : (f1 - f0) / cell;
    } else {
      dv = (float)R * cell;
    }
  }
  d[row] = dv;
  g[row * 3] = gx, g[row * 3 + 1] = gy, g[row * 3 + 2] = gz;
  if (cells) cells[row * 3] = cx, cells[row * 3 + 1] = cy, cells[row * 3 + 2] = cz;
  if (clamped) clamped[row] = (uint8_t)cl;
}

inline bool dt_grid_ok(int B, int GX, int GY, int GZ, int R) {
  if (B < 1 || B > 65535 || R < 1 || R > DT_RMAX || GX < 2 || GY < 2 || GZ < 2) return false;
  const int64_t vox = (int64_t)GX * GY * GZ;
  if (vox >= ((int64_t)1 << 31)) return false;
  const int64_t blocks = (int64_t)B * GZ * GY * ((GX + DT_TILE - 1) / DT_TILE);      // one per line tile
  return blocks < ((int64_t)1 << 31) && ((int64_t)B * vox + 7) / 8 / 256 < ((int64_t)1 << 31);
}

inline bool dt_rows_ok(int B, int N) { return N >= 1 && (int64_t)B * N * 3 < ((int64_t)1 << 31); }

inline int64_t dt_buf_bytes(int B, int GX, int GY, int GZ) { return ((int64_t)B * GX * GY * GZ * 2 + 15) / 16 * 16; }

}  // namespace

extern "C" {

int64_t df_dt_ws_bytes(int B, int GX, int GY, int GZ, int R) {
  if (!dt_grid_ok(B, GX, GY, GZ, R)) return DF_E_SHAPE;
  return dt_buf_bytes(B, GX, GY, GZ);
}

int df_dt_build(const float* ref, const int32_t* count, int B, int N, float ox, float oy, float oz, float cell, int GX, int GY, int GZ, int R,
                uint16_t* dt2, void* ws, void* stream) {
  DF_REQUIRE(dt_grid_ok(B, GX, GY, GZ, R) && dt_rows_ok(B, N), DF_E_SHAPE);
  DF_REQUIRE(ref && count && dt2 && ws, DF_E_ARG);
  DF_REQUIRE(cell > 0.f && cell <= 3.0e38f && ox == ox && oy == oy && oz == oz, DF_E_ARG);      // (NaN fails the comparisons)
  DF_REQUIRE(df_aligned16(dt2) && df_aligned16(ws) && ((uintptr_t)ref & 3u) == 0 && ((uintptr_t)count & 3u) == 0, DF_E_ALIGN);
  hipStream_t st = (hipStream_t)stream;
  uint16_t* tmp = (uint16_t*)ws;
  const int sat = R * R;
  const int64_t n16 = dt_buf_bytes(B, GX, GY, GZ) / 16;
  const int tiles = (GX + DT_TILE - 1) / DT_TILE;
  const unsigned blocks = (unsigned)((int64_t)B * GZ * GY * tiles);
  dt_clear_kernel<<<(unsigned)((n16 + 255) / 256), 256, 0, st>>>((uint4*)ws, n16, (unsigned)sat * 0x10001u);
  DF_CHECK_LAUNCH();
  dt_mark_kernel<<<dim3((N + 255) / 256, B), 256, 0, st>>>(ref, count, N, ox, oy, oz, cell, GX, GY, GZ, tmp);
  DF_CHECK_LAUNCH();
  dt_pass_x_kernel<<<blocks, 256, 0, st>>>(tmp, dt2, GX, tiles, R, sat);
  DF_CHECK_LAUNCH();
  dt_pass_line_kernel<<<blocks, 256, 0, st>>>(dt2, tmp, GX, tiles, 1, GY, (int64_t)GX, R, sat);
  DF_CHECK_LAUNCH();
  dt_pass_line_kernel<<<blocks, 256, 0, st>>>(tmp, dt2, GX, tiles, GY, GZ, (int64_t)GX * GY, R, sat);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

int df_dt_lookup(const float* query, const int32_t* count, const uint16_t* dt2, int B, int N, float ox, float oy, float oz, float cell,
                 int GX, int GY, int GZ, int R, float* d, float* g, int32_t* cells, uint8_t* clamped, void* stream) {
  DF_REQUIRE(dt_grid_ok(B, GX, GY, GZ, R) && dt_rows_ok(B, N), DF_E_SHAPE);
  DF_REQUIRE(query && count && dt2 && d && g, DF_E_ARG);
  DF_REQUIRE(cell > 0.f && cell <= 3.0e38f && ox == ox && oy == oy && oz == oz, DF_E_ARG);
  DF_REQUIRE(df_aligned16(dt2) && ((uintptr_t)query & 3u) == 0 && ((uintptr_t)count & 3u) == 0 && ((uintptr_t)d & 3u) == 0 &&
                 ((uintptr_t)g & 3u) == 0 && ((uintptr_t)cells & 3u) == 0,
             DF_E_ALIGN);
  dt_lookup_kernel<<<dim3((N + 255) / 256, B), 256, 0, (hipStream_t)stream>>>(query, count, dt2, N, ox, oy, oz, cell, GX, GY, GZ, R, d, g,
                                                                             cells, clamped);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

}  // extern "C"
