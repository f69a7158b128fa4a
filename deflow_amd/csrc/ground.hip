// Ground segmentation: the per-point `ground_mask` of a raw sweep, computed on the GPU.  UNPINNED -- upstream writes the mask offline on the
// CPU with a line-fit ground segmenter (absent submodule); this is a height-map segmenter with every choice fixed (include/deflow_amd.h,
// DESIGN.md section 6d), so that the maps and the mask are a pure integer function of the input.
//
//   df_ground_cells   fills zmin with EMPTY (an async 32-bit memset on the stream), then one thread per row: quantises the row (the only
//                     floating-point step: per axis one fp32 subtraction and one fp32 product, rounded separately) and lowers its cell's
//                     minimum with a 32-bit integer atomic min.  The cell is read first and the atomic skipped when the row is not lower
//                     (near the sensor many rows share a cell; min is idempotent, so a stale read costs one redundant atomic and never a
//                     wrong value).
//   df_ground_height  one thread per cell: walks the cell's own chain of ancestors from the origin cell outwards (k = 0 .. r, at most
//                     max(Gx, Gy) steps) carrying (g, miss).  No barriers, no dependence between threads.  The chain's addresses do not
//                     depend on the recurrence, so the loads of GH_CHUNK steps are issued together and only the recurrence is serial.
//   df_ground_mask    one thread per row: h <= height[cell] + TOL.
#include <math.h>

#include "common.h"

namespace {

constexpr int GH_EMPTY = 0x7fffffff;
constexpr int GH_CHUNK = 8;                          // chain steps whose loads are in flight together

struct GhGrid {
  float xmin, ymin, kxy, zmin, kz;
  int Gx, Gy, H;
};

// u = fp32(fp32(p - lo) * k): two separately rounded operations whatever -ffp-contract says
__device__ __forceinline__ float gh_quant(float p, float lo, float k) { return __fmul_rn(__fsub_rn(p, lo), k); }

// a participating row's cell index (cy * Gx + cx) and height level h; false for every other row
__device__ __forceinline__ bool gh_row(const float* __restrict__ p, const GhGrid& g, int* cell, int* h) {
  const float x = p[0], y = p[1], z = p[2];
  const float ux = gh_quant(x, g.xmin, g.kxy), uy = gh_quant(y, g.ymin, g.kxy), uz = gh_quant(z, g.zmin, g.kz);
  const bool ok = isfinite(x) && isfinite(y) && isfinite(z) && ux >= 0.f && ux < (float)g.Gx && uy >= 0.f && uy < (float)g.Gy &&
                  uz >= 0.f && uz < (float)g.H;
  if (!ok) return false;
  *cell = (int)floorf(uy) * g.Gx + (int)floorf(ux);
  *h = (int)floorf(uz);
  return true;
}

__global__ __launch_bounds__(256) void gh_cells_kernel(const float* __restrict__ points, const int32_t* __restrict__ count, int N, GhGrid g,
                                                       int32_t* __restrict__ zmin) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N || i >= count[b]) return;
  int cell, h;
  if (!gh_row(points + ((int64_t)b * N + i) * 3, g, &cell, &h)) return;
  int32_t* z = zmin + (int64_t)b * g.Gx * g.Gy + cell;
  if (h < *z) atomicMin(z, h);
}

__device__ __forceinline__ int gh_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

__global__ __launch_bounds__(256) void gh_height_kernel(const int32_t* __restrict__ zmin, int Gx, int Gy, int ox, int oy, int seed, int RISE,
                                                        int DROP, int WIDEN, int miss_cap, int32_t* __restrict__ height,
                                                        uint8_t* __restrict__ observed) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= Gx * Gy) return;
  const int64_t base = (int64_t)blockIdx.y * Gx * Gy;
  const int32_t* zb = zmin + base;
  const int cx = c % Gx, cy = c / Gx;
  const int dx = cx - ox, dy = cy - oy;
  const int r = max(abs(dx), abs(dy));
  int g = seed, miss = miss_cap;
  bool acc = false;
  for (int k0 = 0; k0 <= r; k0 += GH_CHUNK) {
    int z[GH_CHUNK];
#pragma unroll
    for (int j = 0; j < GH_CHUNK; ++j) {                // the chain's addresses are known in advance: GH_CHUNK loads in flight
      const int k = min(k0 + j, r);
      z[j] = zb[(oy + gh_clamp(dy, -k, k)) * Gx + ox + gh_clamp(dx, -k, k)];
    }
#pragma unroll
    for (int j = 0; j < GH_CHUNK; ++j) {
      if (k0 + j <= r) {
        const int64_t w = (int64_t)WIDEN * min(miss, miss_cap);
        acc = z[j] != GH_EMPTY && (int64_t)g - DROP - w <= (int64_t)z[j] && (int64_t)z[j] <= (int64_t)g + RISE + w;
        if (acc) {
          g = z[j];
          miss = 0;
        } else {
          miss = min(miss + 1, miss_cap);
        }
      }
    }
  }
  height[base + c] = g;
  observed[base + c] = acc ? 1 : 0;
}

__global__ __launch_bounds__(256) void gh_mask_kernel(const float* __restrict__ points, const int32_t* __restrict__ count, int N, GhGrid g,
                                                      const int32_t* __restrict__ height, int TOL, uint8_t* __restrict__ mask) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int64_t row = (int64_t)b * N + i;
  int cell, h;
  uint8_t m = 0;
  if (i < count[b] && gh_row(points + row * 3, g, &cell, &h))
    m = (int64_t)h <= (int64_t)height[(int64_t)b * g.Gx * g.Gy + cell] + TOL ? 1 : 0;
  mask[row] = m;
}

inline bool gh_rows_ok(int B, int N) { return B > 0 && B <= 65535 && N > 0 && (int64_t)B * N < 0x3fffffffll; }
inline bool gh_dims_ok(int Gx, int Gy) { return Gx >= 1 && Gx <= 4096 && Gy >= 1 && Gy <= 4096; }
inline bool gh_geom_ok(float xmin, float ymin, float kxy, float zmin, float kz, int H) {
  return isfinite(xmin) && isfinite(ymin) && isfinite(zmin) && isfinite(kxy) && isfinite(kz) && kxy > 0.f && kz > 0.f && H >= 1 &&
         H <= (1 << 20);
}

}  // namespace

extern "C" int df_ground_cells(const float* points, const int32_t* count, int B, int N, float xmin, float ymin, float kxy, float z_min,
                               float kz, int Gx, int Gy, int H, int32_t* zmin, void* stream) {
  DF_REQUIRE(points && count && zmin, DF_E_ARG);
  DF_REQUIRE(gh_rows_ok(B, N) && gh_dims_ok(Gx, Gy), DF_E_SHAPE);
  DF_REQUIRE(gh_geom_ok(xmin, ymin, kxy, z_min, kz, H), DF_E_ARG);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(zmin), GH_EMPTY, (size_t)B * Gx * Gy, s);
  if (e != hipSuccess) return (int)e;
  const GhGrid g{xmin, ymin, kxy, z_min, kz, Gx, Gy, H};
  hipLaunchKernelGGL(gh_cells_kernel, dim3((N + 255) / 256, B), dim3(256), 0, s, points, count, N, g, zmin);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

extern "C" int df_ground_height(const int32_t* zmin, int B, int Gx, int Gy, int ox, int oy, int seed, int rise, int drop, int widen,
                                int miss_cap, int32_t* height, uint8_t* observed, void* stream) {
  DF_REQUIRE(zmin && height && observed, DF_E_ARG);
  DF_REQUIRE(B > 0 && B <= 65535 && gh_dims_ok(Gx, Gy), DF_E_SHAPE);
  DF_REQUIRE(ox >= 0 && ox < Gx && oy >= 0 && oy < Gy && rise >= 0 && drop >= 0 && widen >= 0 && miss_cap >= 0 && miss_cap <= 64, DF_E_ARG);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(gh_height_kernel, dim3((Gx * Gy + 255) / 256, B), dim3(256), 0, s, zmin, Gx, Gy, ox, oy, seed, rise, drop, widen,
                     miss_cap, height, observed);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

extern "C" int df_ground_mask(const float* points, const int32_t* count, int B, int N, float xmin, float ymin, float kxy, float z_min,
                              float kz, int Gx, int Gy, int H, const int32_t* height, int tol, uint8_t* mask, void* stream) {
  DF_REQUIRE(points && count && height && mask, DF_E_ARG);
  DF_REQUIRE(gh_rows_ok(B, N) && gh_dims_ok(Gx, Gy), DF_E_SHAPE);
  DF_REQUIRE(gh_geom_ok(xmin, ymin, kxy, z_min, kz, H) && tol >= 0, DF_E_ARG);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const GhGrid g{xmin, ymin, kxy, z_min, kz, Gx, Gy, H};
  hipLaunchKernelGGL(gh_mask_kernel, dim3((N + 255) / 256, B), dim3(256), 0, s, points, count, N, g, height, tol, mask);
  DF_CHECK_LAUNCH();
  return DF_OK;
}
