// Bird's-eye-view flow images on the GPU (include/deflow_amd.h): what `python -m deflow_amd.vis` draws with.
//
//   df_render_splat    one thread per row i < count[b]: the row's pixel, its colour (the direction of its vector as a hue, its magnitude
//                      as the saturation) and a 64-bit word [coloured : 1][height key : 31][R G B : 24][0xFF]; the word goes into the
//                      (2r+1)^2 square around the pixel, clipped to the image, with a 64-bit integer atomic max on global memory.  The
//                      maximum of a set does not depend on the order it is taken in: two calls are bit-identical.
//   df_render_resolve  one thread per four output bytes of u8 [B, H, 1 + 3W] (PNG scanlines, filter byte 0): an empty word gives the
//                      background, the legend disc overrides what lies under it.  Every output byte is written exactly once.
// Every floating-point step is one correctly rounded fp32 operation (__fmul_rn, __fadd_rn, __fsub_rn, __fdiv_rn, floorf, a correctly rounded
// sqrtf) that the compiler may not contract: tests/helpers/render_ref.py restates the image byte for byte in numpy float32.
#include "common.h"

namespace {

constexpr int RD_THREADS = 256;
constexpr int RD_MAX_SIDE = 4096;
constexpr int RD_MAX_RADIUS = 4;
constexpr uint32_t RD_GREY = 0x808080u;

inline int64_t rd_stride(int W) { return 1 + 3 * (int64_t)W; }
inline bool rd_image_ok(int B, int W, int H) {
  return B >= 1 && B <= 65535 && W >= 1 && W <= RD_MAX_SIDE && H >= 1 && H <= RD_MAX_SIDE && (int64_t)B * H * rd_stride(W) < 0x80000000ll;
}

// the correctly rounded square root: sqrtf under hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt.  NOT __fsqrt_rn: this toolchain's
// header maps that name to the native v_sqrt_f32 (1 ulp), which numpy's sqrt does not restate
__device__ __forceinline__ float rd_sqrt(float x) { return sqrtf(x); }

__device__ __forceinline__ uint32_t rd_byte(float c) { return (uint32_t)(int)floorf(__fadd_rn(__fmul_rn(c, 255.0f), 0.5f)); }

// the colour of a vector, 0xRRGGBB: HSV with V = 1, S = min(|v| / vmax, 1), H = the diamond angle of (vx, vy) scaled to [0, 6]
__device__ __forceinline__ uint32_t rd_colour(float vx, float vy, float vmax) {
  const float m = rd_sqrt(__fadd_rn(__fmul_rn(vx, vx), __fmul_rn(vy, vy)));
  const float s = fminf(__fdiv_rn(m, vmax), 1.0f);
  const float a = __fadd_rn(fabsf(vx), fabsf(vy));
  float t = 0.0f;
  if (a != 0.0f) {
    if (vy >= 0.0f)
      t = vx >= 0.0f ? __fdiv_rn(vy, a) : __fadd_rn(1.0f, __fdiv_rn(-vx, a));
    else
      t = vx >= 0.0f ? __fadd_rn(3.0f, __fdiv_rn(vx, a)) : __fadd_rn(2.0f, __fdiv_rn(-vy, a));
  }
  const float h6 = __fmul_rn(1.5f, t);                       // [0, 6]
  const float fl = floorf(h6);
  const float f = __fsub_rn(h6, fl);
  int k = (int)fl;
  if (k > 5) k = 0;                                          // h6 == 6 (f == 0): the same red as h6 == 0
  const float p = __fsub_rn(1.0f, s);
  const float q = __fsub_rn(1.0f, __fmul_rn(s, f));
  const float u = __fsub_rn(1.0f, __fmul_rn(s, __fsub_rn(1.0f, f)));
  const uint32_t P = rd_byte(p), Q = rd_byte(q), U = rd_byte(u), V = 255u;
  uint32_t r = V, g = U, b = P;                              // sector 0
  if (k == 1) r = Q, g = V, b = P;
  if (k == 2) r = P, g = V, b = U;
  if (k == 3) r = P, g = Q, b = V;
  if (k == 4) r = U, g = P, b = V;
  if (k == 5) r = V, g = P, b = Q;
  return (r << 16) | (g << 8) | b;
}

__global__ __launch_bounds__(RD_THREADS) void rd_splat_kernel(const float* __restrict__ points, const float* __restrict__ vec,
                                                              const uint8_t* __restrict__ cls, const int32_t* __restrict__ count, int N,
                                                              float xmin, float ymin, float inv_res, int W, int H, float vmax, int radius,
                                                              unsigned long long* __restrict__ image) {
  const int b = blockIdx.y, i = blockIdx.x * RD_THREADS + threadIdx.x;
  if (i >= N) return;
  const int cnt = min(max(count[b], 0), N);
  if (i >= cnt) return;
  const int64_t at = (int64_t)b * N + i;
  const uint32_t c = cls[at];
  if (c == 0) return;
  const float* p = points + at * 3;
  const float* v = vec + at * 3;
  const float x = p[0], y = p[1], z = p[2], vx = v[0], vy = v[1], vz = v[2];
  if (!(isfinite(x) && isfinite(y) && isfinite(z) && isfinite(vx) && isfinite(vy) && isfinite(vz))) return;
  const float fx = floorf(__fmul_rn(__fsub_rn(x, xmin), inv_res));
  const float fy = floorf(__fmul_rn(__fsub_rn(y, ymin), inv_res));
  if (!(fx >= 0.0f && fx < (float)W && fy >= 0.0f && fy < (float)H)) return;      // compared on the floats: inf and 2^31 never reach an int
  const int px = (int)fx, py = H - 1 - (int)fy;
  const uint32_t zb = __builtin_bit_cast(uint32_t, z);
  const uint32_t key = (zb & 0x80000000u) ? ~zb : (zb | 0x80000000u);             // unsigned order == float order
  const uint32_t rgb = c == 1 ? rd_colour(vx, vy, vmax) : RD_GREY;
  const unsigned long long word = ((unsigned long long)(c == 1 ? 1u : 0u) << 63) | ((unsigned long long)(key >> 1) << 32) |
                                  ((unsigned long long)rgb << 8) | 0xFFull;
  unsigned long long* img = image + (int64_t)b * H * W;
  const int x0 = max(px - radius, 0), x1 = min(px + radius, W - 1), y0 = max(py - radius, 0), y1 = min(py + radius, H - 1);
  for (int yy = y0; yy <= y1; ++yy)
    for (int xx = x0; xx <= x1; ++xx) atomicMax(img + (int64_t)yy * W + xx, word);
}

// colour of pixel (x, row y) of sample b, 0xRRGGBB
__device__ __forceinline__ uint32_t rd_pixel(const unsigned long long* __restrict__ image, int b, int y, int x, int W, int H, uint32_t bg,
                                             int L) {
  if (L > 0) {
    const int dx = x - (W - 3 - L), dy = y - (L + 2);
    if (dx * dx + dy * dy <= L * L) return rd_colour((float)dx, (float)(-dy), (float)L);
  }
  const unsigned long long w = image[((int64_t)b * H + y) * W + x];
  return w == 0ull ? bg : (uint32_t)(w >> 8) & 0xFFFFFFu;
}

__global__ __launch_bounds__(RD_THREADS) void rd_resolve_kernel(const unsigned long long* __restrict__ image, int W, int H, uint32_t bg,
                                                                int L, uint32_t total, uint8_t* __restrict__ out) {
  const uint32_t o = ((uint32_t)blockIdx.x * RD_THREADS + threadIdx.x) * 4u;      // total < 2^31: no wrap
  if (o >= total) return;
  const uint32_t S = 1u + 3u * (uint32_t)W;
  uint32_t line = o / S, col = o - line * S;                                       // line = b * H + y
  uint32_t b = line / (uint32_t)H, y = line - b * (uint32_t)H;
  const int n = (int)min(4u, total - o);
  uint32_t word = 0, rgb = 0;
  int have = -1;                                                                   // the column rgb was computed for; forgotten at a line's end
  for (int j = 0; j < n; ++j) {
    uint32_t byte = 0;                                                             // col == 0: the scanline's filter byte
    if (col != 0) {
      const int x = (int)((col - 1u) / 3u), ch = (int)((col - 1u) - 3u * (uint32_t)x);
      if (x != have) {
        rgb = rd_pixel(image, (int)b, (int)y, x, W, H, bg, L);
        have = x;
      }
      byte = (rgb >> (8 * (2 - ch))) & 0xFFu;
    }
    word |= byte << (8 * j);
    if (++col == S) {
      col = 0;
      have = -1;
      if (++y == (uint32_t)H) y = 0, ++b;
    }
  }
  if (n == 4) {
    *reinterpret_cast<uint32_t*>(out + o) = word;
  } else {
    for (int j = 0; j < n; ++j) out[o + j] = (uint8_t)(word >> (8 * j));
  }
}

}  // namespace

extern "C" int df_render_splat(const float* points, const float* vec, const uint8_t* cls, const int32_t* count, int B, int N, float xmin,
                               float ymin, float inv_res, int W, int H, float vmax, int radius, uint64_t* image, void* stream) {
  DF_REQUIRE(points && vec && cls && count && image, DF_E_ARG);
  DF_REQUIRE(rd_image_ok(B, W, H) && N >= 1 && (int64_t)B * N < 0x80000000ll, DF_E_SHAPE);
  DF_REQUIRE(radius >= 0 && radius <= RD_MAX_RADIUS && vmax > 0.0f && vmax < INFINITY && inv_res > 0.0f && inv_res < INFINITY &&
                 xmin > -INFINITY && xmin < INFINITY && ymin > -INFINITY && ymin < INFINITY,
             DF_E_ARG);
  DF_REQUIRE((((uintptr_t)image) & 7u) == 0, DF_E_ALIGN);
  hipLaunchKernelGGL(rd_splat_kernel, dim3((N + RD_THREADS - 1) / RD_THREADS, B), dim3(RD_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     points, vec, cls, count, N, xmin, ymin, inv_res, W, H, vmax, radius, reinterpret_cast<unsigned long long*>(image));
  DF_CHECK_LAUNCH();
  return DF_OK;
}

extern "C" int df_render_resolve(const uint64_t* image, int B, int W, int H, int bg_rgb, int legend, uint8_t* scanlines, void* stream) {
  DF_REQUIRE(image && scanlines, DF_E_ARG);
  DF_REQUIRE(rd_image_ok(B, W, H), DF_E_SHAPE);
  DF_REQUIRE(bg_rgb >= 0 && bg_rgb <= 0xFFFFFF && legend >= 0 && (legend == 0 || 2 * (int64_t)legend + 5 <= (W < H ? W : H)), DF_E_ARG);
  DF_REQUIRE((((uintptr_t)image) & 7u) == 0 && (((uintptr_t)scanlines) & 3u) == 0, DF_E_ALIGN);
  const uint32_t total = (uint32_t)((int64_t)B * H * rd_stride(W));
  const uint32_t words = (total + 3u) / 4u;
  hipLaunchKernelGGL(rd_resolve_kernel, dim3((words + RD_THREADS - 1) / RD_THREADS), dim3(RD_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const unsigned long long*>(image), W, H, (uint32_t)bg_rgb, legend, total, scanlines);
  DF_CHECK_LAUNCH();
  return DF_OK;
}
