// Void map: per-point dynamic flags from ray casting, the input of the online cluster labels (cluster.hip) computed on the GPU.  UNPINNED --
// upstream writes its `dufo_label` offline on the CPU with DUFOMap (process.py; absent submodule); this is a DUFOMap-style map with every
// choice fixed (include/deflow_amd.h), so that the map and the flags are a pure integer function of the input.
// Space that some sweep has seen through is void; a return that lies in void space is dynamic.
//
//   df_void_cast    one thread per ray: quantises origin and endpoint to 1/256 voxel (the only floating-point step: one fp32 subtraction
//                   and one fp32 product, rounded separately), walks the voxels from the origin to the endpoint with an integer DDA
//                   (64-bit cross-multiplied comparisons, x before y before z on ties) and sets the free bits F of the voxels it crosses
//                   -- all of them when the ray was cut at the range R, otherwise those further than hit_margin voxels (Chebyshev) from
//                   the end; sets the occupied bit O of the endpoint's voxel.  Bits are set with 32-bit integer atomic OR; the word is
//                   read first and the atomic skipped when the bit is there (every ray of a sweep crosses the same voxels near the
//                   sensor; OR is idempotent, so a stale read costs one redundant atomic and never a wrong bit).
//                   df_void_cast_probe is the same kernel for measuring: it counts the sets the rays ask for and can drop the test.
//   df_void_merge   one thread per word: V |= erode(F & ~O, r); the x neighbours come from shifts with the two adjacent words, the y / z
//                   neighbours from the rows around; voxels outside the grid count as not free.
//   df_void_query   one thread per row: its bit of V.
//
// The Chebyshev distance of the walk's voxel to the end voxel is the largest of the per-axis steps still to do, so an uncut ray stops
// walking once that is <= hit_margin: the rest of its voxels set nothing.  The walk is bounded by 3 * (R / 256 + 1) steps, which a ray
// of at most R sub-voxel units per axis cannot exceed; a ray that would adds 1 to the status word and is cut there.
#include <math.h>

#include "common.h"

namespace {

constexpr int VM_SUB_SHIFT = 8;                       // 256 sub-voxel units per voxel
constexpr float VM_QMAX = 1073741824.0f;              // 2^30: a coordinate takes part when |u| is below it

struct VmGrid {
  float gx, gy, gz, k;
  int Gx, Gy, Gz;
};

// u = fp32(fp32(p - gmin) * k), q = floor(u): two separately rounded operations whatever -ffp-contract says
__device__ __forceinline__ bool vm_quant1(float p, float g, float k, int64_t* q) {
  const float u = __fmul_rn(__fsub_rn(p, g), k);
  *q = (int64_t)floorf(u);
  return isfinite(p) && fabsf(u) < VM_QMAX;
}
__device__ __forceinline__ bool vm_quant(const float* __restrict__ p, const VmGrid& g, int64_t q[3]) {
  const float x = p[0], y = p[1], z = p[2];
  const bool a = vm_quant1(x, g.gx, g.k, &q[0]);
  const bool b = vm_quant1(y, g.gy, g.k, &q[1]);
  const bool c = vm_quant1(z, g.gz, g.k, &q[2]);
  return a && b && c;
}

__device__ __forceinline__ bool vm_inside(const VmGrid& g, int64_t x, int64_t y, int64_t z) {
  return x >= 0 && x < g.Gx && y >= 0 && y < g.Gy && z >= 0 && z < g.Gz;
}
// bit = (z * Gy + y) * Gx + x (< 2^31 by the entry's check); only called for a voxel inside the grid
__device__ __forceinline__ uint32_t vm_bit(const VmGrid& g, int64_t x, int64_t y, int64_t z) {
  return ((uint32_t)z * (uint32_t)g.Gy + (uint32_t)y) * (uint32_t)g.Gx + (uint32_t)x;
}

template <bool TEST>
__device__ __forceinline__ void vm_set(uint32_t* __restrict__ words, uint32_t bit) {
  uint32_t* w = words + (bit >> 5);
  const uint32_t m = 1u << (bit & 31u);
  if (TEST && (*w & m)) return;
  atomicOr(w, m);
}

__device__ __forceinline__ int64_t vm_floor_div(int64_t a, int64_t b) {      // b > 0
  int64_t q = a / b;
  if (a % b < 0) --q;
  return q;
}
__device__ __forceinline__ int64_t vm_abs(int64_t v) { return v < 0 ? -v : v; }

template <bool TEST>
__global__ __launch_bounds__(256) void vm_cast_kernel(const float* __restrict__ points, const int32_t* __restrict__ count,
                                                      const float* __restrict__ origin, int N, VmGrid g, int hit_margin, int R,
                                                      int64_t words_per_sample, uint32_t* __restrict__ F, uint32_t* __restrict__ O,
                                                      int32_t* __restrict__ status, unsigned long long* __restrict__ attempts) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N || i >= count[b]) return;
  int64_t E[3], A[3];
  if (!vm_quant(points + ((int64_t)b * N + i) * 3, g, E)) return;
  uint32_t* Fb = F + (int64_t)b * words_per_sample;
  uint32_t* Ob = O + (int64_t)b * words_per_sample;
  {
    const int64_t ox = E[0] >> VM_SUB_SHIFT, oy = E[1] >> VM_SUB_SHIFT, oz = E[2] >> VM_SUB_SHIFT;
    if (vm_inside(g, ox, oy, oz)) vm_set<TEST>(Ob, vm_bit(g, ox, oy, oz));
  }
  if (!vm_quant(origin + (int64_t)b * 3, g, A)) return;          // no origin: the sample's rows are occupied, none of its rays is cast

  int64_t d[3] = {E[0] - A[0], E[1] - A[1], E[2] - A[2]};
  const int64_t m = max(vm_abs(d[0]), max(vm_abs(d[1]), vm_abs(d[2])));
  const bool cut = m > (int64_t)R;
  if (cut) {                                                        // Chebyshev range cut, in integers
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      E[k] = A[k] + vm_floor_div(d[k] * (int64_t)R, m);
      d[k] = E[k] - A[k];
    }
  }
  int64_t c[3];
  int step[3], rem[3], num[3], den[3];                              // after the cut |d| <= R <= 2^24: these fit 32 bits (num <= R + 768)
  int64_t total = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    c[k] = A[k] >> VM_SUB_SHIFT;
    const int64_t e = E[k] >> VM_SUB_SHIFT;
    step[k] = d[k] > 0 ? 1 : (d[k] < 0 ? -1 : 0);
    den[k] = (int)vm_abs(d[k]);
    const int64_t r = vm_abs(e - c[k]);
    num[k] = (int)(d[k] > 0 ? ((c[k] + 1) << VM_SUB_SHIFT) - A[k] : A[k] - (c[k] << VM_SUB_SHIFT));
    total += r;
    rem[k] = (int)min(r, (int64_t)0x7fffffff);
  }
  const int64_t bound = 3 * ((int64_t)(R >> VM_SUB_SHIFT) + 1);
  if (total > bound) {
    if (status) atomicAdd(status, 1);
    total = bound;
  }
  unsigned long long sets = 0;
  int far = max(rem[0], max(rem[1], rem[2]));                       // Chebyshev voxel distance to the end voxel
  if ((cut || far > hit_margin) && vm_inside(g, c[0], c[1], c[2])) {
    vm_set<TEST>(Fb, vm_bit(g, c[0], c[1], c[2]));
    ++sets;
  }
  for (int64_t it = 0; it < total && (cut || far > hit_margin); ++it) {
    // the axis with the smallest num / den among those with steps left; strict comparisons: the lower axis wins a tie
    int ax = rem[0] > 0 ? 0 : (rem[1] > 0 ? 1 : 2);
    if (ax == 0 && rem[1] > 0 && (int64_t)num[1] * den[0] < (int64_t)num[0] * den[1]) ax = 1;
    if (ax < 2 && rem[2] > 0) {
      const int na = ax == 0 ? num[0] : num[1], da = ax == 0 ? den[0] : den[1];
      if ((int64_t)num[2] * da < (int64_t)na * den[2]) ax = 2;
    }
    // (select by comparison, not by indexing: a dynamically indexed array would go to scratch)
    if (ax == 0) {
      c[0] += step[0]; num[0] += 256; rem[0] -= 1;
    } else if (ax == 1) {
      c[1] += step[1]; num[1] += 256; rem[1] -= 1;
    } else {
      c[2] += step[2]; num[2] += 256; rem[2] -= 1;
    }
    far = max(rem[0], max(rem[1], rem[2]));
    if ((cut || far > hit_margin) && vm_inside(g, c[0], c[1], c[2])) {
      vm_set<TEST>(Fb, vm_bit(g, c[0], c[1], c[2]));
      ++sets;
    }
  }
  if (attempts && sets) atomicAdd(attempts, sets);
}

// x-erosion of one row word: a = the word, l / r = its neighbours in the row (0 outside the grid)
__device__ __forceinline__ uint32_t vm_erode_x(uint32_t l, uint32_t a, uint32_t r, int rad) {
  uint32_t v = a;
  for (int s = 1; s <= rad; ++s) v &= ((a << s) | (l >> (32 - s))) & ((a >> s) | (r << (32 - s)));
  return v;
}

__global__ __launch_bounds__(256) void vm_merge_kernel(const uint32_t* __restrict__ F, const uint32_t* __restrict__ O,
                                                       uint32_t* __restrict__ V, int wx_n, int Gy, int Gz, int rad,
                                                       int64_t words_per_sample) {
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= words_per_sample) return;
  const int64_t base = (int64_t)blockIdx.y * words_per_sample;
  const uint32_t* Fb = F + base;
  const uint32_t* Ob = O + base;
  uint32_t acc = Fb[w] & ~Ob[w];
  if (acc == 0u) return;                                            // the centre is part of every neighbourhood: nothing to add
  if (rad > 0) {
    const int wx = (int)(w % wx_n);
    const int64_t row = w / wx_n;
    const int y = (int)(row % Gy), z = (int)(row / Gy);
    for (int dz = -rad; dz <= rad && acc; ++dz) {
      for (int dy = -rad; dy <= rad && acc; ++dy) {
        const int yy = y + dy, zz = z + dz;
        if (yy < 0 || yy >= Gy || zz < 0 || zz >= Gz) {
          acc = 0u;
          break;
        }
        const int64_t q = ((int64_t)zz * Gy + yy) * wx_n + wx;
        const uint32_t a = Fb[q] & ~Ob[q];
        const uint32_t l = wx > 0 ? Fb[q - 1] & ~Ob[q - 1] : 0u;
        const uint32_t r = wx + 1 < wx_n ? Fb[q + 1] & ~Ob[q + 1] : 0u;
        acc &= vm_erode_x(l, a, r, rad);
      }
    }
    if (acc == 0u) return;
  }
  const uint32_t old = V[base + w];
  if ((old | acc) != old) V[base + w] = old | acc;
}

__global__ __launch_bounds__(256) void vm_query_kernel(const float* __restrict__ points, const int32_t* __restrict__ count, int N, VmGrid g,
                                                       int64_t words_per_sample, const uint32_t* __restrict__ V,
                                                       int32_t* __restrict__ flags) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int64_t row = (int64_t)b * N + i;
  int f = 0;
  int64_t q[3];
  if (i < count[b] && vm_quant(points + row * 3, g, q)) {
    const int64_t x = q[0] >> VM_SUB_SHIFT, y = q[1] >> VM_SUB_SHIFT, z = q[2] >> VM_SUB_SHIFT;
    if (vm_inside(g, x, y, z)) {
      const uint32_t bit = vm_bit(g, x, y, z);
      f = (int)((V[(int64_t)b * words_per_sample + (bit >> 5)] >> (bit & 31u)) & 1u);
    }
  }
  flags[row] = f;
}

inline bool vm_rows_ok(int B, int N) { return B > 0 && N > 0 && (int64_t)B * N < 0x3fffffffll && B <= 65535; }
inline bool vm_dims_ok(int Gx, int Gy, int Gz) {
  return Gx > 0 && Gy > 0 && Gz > 0 && Gx % 32 == 0 && (int64_t)Gx * Gy * Gz < 0x80000000ll;
}
inline bool vm_geom_ok(float gx, float gy, float gz, float k) { return isfinite(gx) && isfinite(gy) && isfinite(gz) && isfinite(k) && k > 0.f; }

}  // namespace

namespace {
int vm_cast(const float* points, const int32_t* count, const float* origin, int B, int N, float gminx, float gminy, float gminz, float k,
            int Gx, int Gy, int Gz, int hit_margin, int R, uint32_t* F, uint32_t* O, int32_t* status, uint64_t* attempts,
            int always_atomic, void* stream) {
  DF_REQUIRE(points && count && origin && F && O, DF_E_ARG);
  DF_REQUIRE(vm_rows_ok(B, N) && vm_dims_ok(Gx, Gy, Gz), DF_E_SHAPE);
  DF_REQUIRE(vm_geom_ok(gminx, gminy, gminz, k) && hit_margin >= 0 && R >= 1 && R <= (1 << 24), DF_E_ARG);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t W = (int64_t)Gx * Gy * Gz / 32;
  hipError_t e = hipMemsetAsync(F, 0, (size_t)B * W * 4, s);
  if (e != hipSuccess) return (int)e;
  e = hipMemsetAsync(O, 0, (size_t)B * W * 4, s);
  if (e != hipSuccess) return (int)e;
  const VmGrid g{gminx, gminy, gminz, k, Gx, Gy, Gz};
  const dim3 grid((N + 255) / 256, B);
  unsigned long long* att = reinterpret_cast<unsigned long long*>(attempts);
  if (always_atomic)
    hipLaunchKernelGGL(vm_cast_kernel<false>, grid, dim3(256), 0, s, points, count, origin, N, g, hit_margin, R, W, F, O, status, att);
  else
    hipLaunchKernelGGL(vm_cast_kernel<true>, grid, dim3(256), 0, s, points, count, origin, N, g, hit_margin, R, W, F, O, status, att);
  DF_CHECK_LAUNCH();
  return DF_OK;
}
}  // namespace

extern "C" int df_void_cast(const float* points, const int32_t* count, const float* origin, int B, int N, float gminx, float gminy,
                            float gminz, float k, int Gx, int Gy, int Gz, int hit_margin, int R, uint32_t* F, uint32_t* O,
                            int32_t* status, void* stream) {
  return vm_cast(points, count, origin, B, N, gminx, gminy, gminz, k, Gx, Gy, Gz, hit_margin, R, F, O, status, nullptr, 0, stream);
}

// the measuring form (tools/voidmap_bench.py, the tests): the same kernel, counting the free-bit sets the rays ask for, and optionally
// without the test before the atomic
extern "C" int df_void_cast_probe(const float* points, const int32_t* count, const float* origin, int B, int N, float gminx, float gminy,
                                  float gminz, float k, int Gx, int Gy, int Gz, int hit_margin, int R, uint32_t* F, uint32_t* O,
                                  int32_t* status, uint64_t* attempts, int always_atomic, void* stream) {
  return vm_cast(points, count, origin, B, N, gminx, gminy, gminz, k, Gx, Gy, Gz, hit_margin, R, F, O, status, attempts, always_atomic, stream);
}

extern "C" int df_void_merge(const uint32_t* F, const uint32_t* O, uint32_t* V, int B, int Gx, int Gy, int Gz, int erode, void* stream) {
  DF_REQUIRE(F && O && V, DF_E_ARG);
  DF_REQUIRE(B > 0 && B <= 65535 && vm_dims_ok(Gx, Gy, Gz), DF_E_SHAPE);
  DF_REQUIRE(erode >= 0 && erode <= 2, DF_E_ARG);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t W = (int64_t)Gx * Gy * Gz / 32;
  hipLaunchKernelGGL(vm_merge_kernel, dim3((unsigned)((W + 255) / 256), B), dim3(256), 0, s, F, O, V, Gx / 32, Gy, Gz, erode, W);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

extern "C" int df_void_query(const float* points, const int32_t* count, int B, int N, float gminx, float gminy, float gminz, float k,
                             int Gx, int Gy, int Gz, const uint32_t* V, int32_t* flags, void* stream) {
  DF_REQUIRE(points && count && V && flags, DF_E_ARG);
  DF_REQUIRE(vm_rows_ok(B, N) && vm_dims_ok(Gx, Gy, Gz), DF_E_SHAPE);
  DF_REQUIRE(vm_geom_ok(gminx, gminy, gminz, k), DF_E_ARG);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const VmGrid g{gminx, gminy, gminz, k, Gx, Gy, Gz};
  hipLaunchKernelGGL(vm_query_kernel, dim3((N + 255) / 256, B), dim3(256), 0, s, points, count, N, g, (int64_t)Gx * Gy * Gz / 32, V, flags);
  DF_CHECK_LAUNCH();
  return DF_OK;
}
