// A depth cube about the sensor: the range-image visibility test that carves seen-through rows out of the local map.
// UNPINNED -- the definition is this project's own: include/deflow_amd.h, DESIGN.md section 6u.
//
// A direction from the origin is filed on one of the six faces of a cube, R x R bins per face; a bin holds the smallest depth (the
// absolute major coordinate) of the rows filed there, as the bit pattern of a positive float, +inf where there is none.
//
//   df_depth_cube_build   a fill launch (every bin +inf), then one thread per row: an integer atomicMin of the depth's bits into the
//                         row's bin.  Positive floats order as their bits and an integer minimum does not depend on the order of its
//                         operands, so two calls are bit-identical (ground.hip's zmin is the precedent).
//   df_depth_cube_test    one thread per query row: the smallest depth in the (2 halo + 1)^2 bins about its own, and the flag.
//
// No transcendental function; every fp32 operation is rounded once and named (no fma contraction), so numpy float32 reproduces every
// value bit for bit.  No LDS, no float atomics.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr uint32_t CUBE_EMPTY = 0x7f800000u;        // +inf: a bin without a return

// face, bin and depth of the direction (x, y, z); false where the row does not take part by its coordinates
__device__ __forceinline__ bool cube_bin(float x, float y, float z, int R, int* face, int* i, int* j, float* depth) {
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return false;
  const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
  float major, uc, vc, m;
  int axis;
  if (ax >= ay && ax >= az) {
    axis = 0, major = x, m = ax, uc = y, vc = z;
  } else if (ay >= az) {
    axis = 1, major = y, m = ay, uc = x, vc = z;
  } else {
    axis = 2, major = z, m = az, uc = x, vc = y;
  }
  if (!(m > 0.0f)) return false;
  const float half = (float)(R / 2);
  const float fu = floorf(__fmul_rn(__fadd_rn(__fdiv_rn(uc, m), 1.0f), half));
  const float fv = floorf(__fmul_rn(__fadd_rn(__fdiv_rn(vc, m), 1.0f), half));
  const int iu = (int)fu, iv = (int)fv;             // |u|, |v| <= 1: both lie in [0, R]
  *face = 2 * axis + (major < 0.0f ? 1 : 0);
  *i = iu < 0 ? 0 : (iu > R - 1 ? R - 1 : iu);
  *j = iv < 0 ? 0 : (iv > R - 1 ? R - 1 : iv);
  *depth = m;
  return true;
}

__global__ __launch_bounds__(256) void cube_fill_kernel(int64_t n, uint32_t* __restrict__ img) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) img[i] = CUBE_EMPTY;
}

__global__ __launch_bounds__(256) void cube_build_kernel(const float* __restrict__ points, const int32_t* __restrict__ count,
                                                         const int32_t* __restrict__ mask, int N, int R, uint32_t* __restrict__ img) {
  const int b = blockIdx.y;
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= N || r >= count[b]) return;
  const int64_t s = (int64_t)b * N + r;
  if (mask && !(mask[s] > 0)) return;
  int face, i, j;
  float m;
  if (!cube_bin(points[s * 3], points[s * 3 + 1], points[s * 3 + 2], R, &face, &i, &j, &m)) return;
  atomicMin(img + (((int64_t)b * 6 + face) * R + j) * R + i, __builtin_bit_cast(uint32_t, m));
}

__global__ __launch_bounds__(256) void cube_test_kernel(const float* __restrict__ query, const int32_t* __restrict__ count_q,
                                                        const uint32_t* __restrict__ img, int M, int R, int halo, float margin, float c,
                                                        float near, int32_t* __restrict__ flag, uint32_t* __restrict__ depth_out) {
  const int b = blockIdx.y;
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= M) return;
  const int64_t s = (int64_t)b * M + r;
  const float x = query[s * 3], y = query[s * 3 + 1], z = query[s * 3 + 2];
  int face = 0, i = 0, j = 0;
  float m = 0.0f;
  bool ok = r < count_q[b] && cube_bin(x, y, z, R, &face, &i, &j, &m);
  ok = ok && i - halo >= 0 && i + halo <= R - 1 && j - halo >= 0 && j + halo <= R - 1;
  uint32_t dmin = CUBE_EMPTY, own = CUBE_EMPTY;
  if (ok) {
    const uint32_t* f = img + ((int64_t)b * 6 + face) * R * R;
    own = f[(int64_t)j * R + i];
    for (int dj = -halo; dj <= halo; ++dj)
      for (int di = -halo; di <= halo; ++di) {
        const uint32_t d = f[(int64_t)(j + dj) * R + (i + di)];
        dmin = d < dmin ? d : dmin;
      }
  }
  const bool seen = ok && fmaxf(fabsf(x), fabsf(y)) >= near && own != CUBE_EMPTY &&
                    __fadd_rn(__fmul_rn(m, c), margin) < __builtin_bit_cast(float, dmin);
  flag[s] = seen ? 1 : 0;
  if (depth_out) depth_out[s] = dmin;
}

bool cube_shape_ok(int B, int rows, int R) {
  if (B < 1 || B > 65535 || rows < 1 || R < 2 || R > 2048 || (R & 1)) return false;
  return (int64_t)B * rows < (1ll << 30) && (int64_t)B * 6 * R * R < (1ll << 30);
}

inline bool cube_aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

}  // namespace

extern "C" int df_depth_cube_build(const float* points, const int32_t* count, const int32_t* mask, int B, int N, int R, uint32_t* img,
                                   void* stream) {
  DF_REQUIRE(points && count && img, DF_E_ARG);
  DF_REQUIRE(cube_shape_ok(B, N, R), DF_E_SHAPE);
  DF_REQUIRE(cube_aligned4(points) && cube_aligned4(count) && cube_aligned4(mask) && cube_aligned4(img), DF_E_ALIGN);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t bins = (int64_t)B * 6 * R * R;
  hipLaunchKernelGGL(cube_fill_kernel, dim3((unsigned)((bins + 255) / 256)), dim3(256), 0, s, bins, img);
  DF_CHECK_LAUNCH();
  hipLaunchKernelGGL(cube_build_kernel, dim3((unsigned)((N + 255) / 256), B), dim3(256), 0, s, points, count, mask, N, R, img);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

extern "C" int df_depth_cube_test(const float* query, const int32_t* count_q, const uint32_t* img, int B, int M, int R, int halo,
                                  float margin, float rel, float near, int32_t* flag, float* depth_out, void* stream) {
  DF_REQUIRE(query && count_q && img && flag, DF_E_ARG);
  DF_REQUIRE(cube_shape_ok(B, M, R), DF_E_SHAPE);
  DF_REQUIRE(halo >= 0 && halo <= 4 && isfinite(margin) && margin >= 0.0f && isfinite(rel) && rel >= 0.0f && isfinite(near) && near >= 0.0f,
             DF_E_ARG);
  DF_REQUIRE(cube_aligned4(query) && cube_aligned4(count_q) && cube_aligned4(img) && cube_aligned4(flag) && cube_aligned4(depth_out),
             DF_E_ALIGN);
  const float c = 1.0f + rel;                         // fp32, rounded once, on the host: the kernel multiplies by it
  hipLaunchKernelGGL(cube_test_kernel, dim3((unsigned)((M + 255) / 256), B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), query,
                     count_q, img, M, R, halo, margin, c, near, flag, reinterpret_cast<uint32_t*>(depth_out));
  DF_CHECK_LAUNCH();
  return DF_OK;
}
