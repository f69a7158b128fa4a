// Per-cluster rigidity term of model=mbnsf (the definition is in include/deflow_amd.h): the distances between rows
// of one cluster of the first sweep should not change under the flow.
//   df_iso_plan   once per pair.  iso_plan_kernel, one thread per row: the row's label names its ordered list (df_rigid_segments'
//                 output), a binary search in that ascending list gives the row's position i, and the 2P partners L[(i +- s_k) mod n]
//                 with their rest distances go into the row's table entries.  The hot kernel then knows nothing of clusters.  The
//                 number of pair instances M_b = P x (rows with partners) is counted per block and added with ONE integer atomic.
//   df_iso_pairs  once per iteration, one thread per row: the row's 2P table entries (contiguous; 16-byte loads when P is even), a
//                 gather of the partners' warped rows, the robust penalty of every instance and its gradient.  Every instance is
//                 evaluated from both of its ends with the same bits (a difference negates exactly, its square does not change), so no
//                 thread writes another row's result: no atomics, two calls are bit-identical.
// The squared lengths are formed with __fmul_rn / __fadd_rn: the file is built with -ffp-contract=on, and a fused multiply-add would
// round differently from the definition's fp32(fp32(fp32(dx dx) + fp32(dy dy)) + fp32(dz dz)).
#include <math.h>

#include "common.h"

namespace {

constexpr int ISO_PMAX = 16;

inline bool iso_dims_ok(int B, int N, int P) {
  return P >= 1 && P <= ISO_PMAX && B >= 1 && B <= 65535 && N >= 1 && (int64_t)B * N * 2 * P < ((int64_t)1 << 31);
}

__device__ __forceinline__ float iso_dist(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
}

// the k-th stride (k = 1..P) of a list of n >= 2 rows: 1 + floor((k - 1)(n - 1) / P), in 1..n-1
__device__ __forceinline__ int iso_stride(int k, int n, int P) { return 1 + (int)(((int64_t)(k - 1) * (n - 1)) / P); }

__global__ __launch_bounds__(256) void iso_plan_kernel(const float* __restrict__ x, const int32_t* __restrict__ count,
                                                       const int32_t* __restrict__ labels, const int32_t* __restrict__ seg_off,
                                                       const int32_t* __restrict__ seg_rows, int N, int Kcap, int P, int max_pts,
                                                       int32_t* __restrict__ nbr, float* __restrict__ r0, int32_t* __restrict__ pairs) {
  __shared__ int wsum[4];
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int32_t* rows = seg_rows + (int64_t)b * (N + 1);           // the lists of the labels followed by one more column
  int start = 0, n = 0, pos = -1;
  if (i < N && i < min(max(count[b], 0), N)) {
    const int l = labels[(int64_t)b * N + i];
    if (l >= 1 && l <= Kcap) {
      const int32_t* off = seg_off + (int64_t)b * (2 * Kcap + 1) + 2 * (l - 1);
      start = off[0];
      n = off[1] - start;
      if (start >= 0 && n >= 2 && n <= max_pts && start + n <= N + 1) {
        int lo = 0, hi = n;                                         // the first position whose row is >= i
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (rows[start + mid] < i) lo = mid + 1;
          else hi = mid;
        }
        if (lo < n && rows[start + lo] == i) pos = lo;              // (a list that does not hold the row: no partners)
      }
    }
  }
  if (i < N) {
    const int64_t base = ((int64_t)b * N + i) * 2 * P;
    const float* xa = x + ((int64_t)b * N + i) * 3;
    for (int e = 0; e < 2 * P; ++e) {
      int q = -1;
      float d = 0.f;
      if (pos >= 0) {
        const int s = iso_stride(e < P ? e + 1 : e - P + 1, n, P);
        const int j = e < P ? pos + s : pos - s;                     // in (-n, 2n)
        q = rows[start + (j < 0 ? j + n : (j >= n ? j - n : j))];
        if (q < 0 || q >= N) q = -1;                                 // (never, for df_rigid_segments' lists)
        else {
          const float* xb = x + ((int64_t)b * N + q) * 3;
          d = iso_dist(xa[0], xa[1], xa[2], xb[0], xb[1], xb[2]);
        }
      }
      nbr[base + e] = q;
      r0[base + e] = d;
    }
  }
  // rows with partners in this block -> one integer add per block
  const unsigned long long m = __ballot(pos >= 0);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int c = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    if (c) atomicAdd(pairs + b, c * P);
  }
}

struct IsoAcc {
  float v, gx, gy, gz;
};

// one table entry of a row at (wx, wy, wz): the instance's penalty (added to v for a forward entry) and its gradient
__device__ __forceinline__ void iso_entry(const float* __restrict__ wb, float wx, float wy, float wz, int q, float rest, bool fwd, float delta,
                                          int N, IsoAcc& a) {
  if (q < 0 || q >= N) return;                                       // -1: no partner (and no index is formed from a bad table)
  const float* p = wb + (int64_t)q * 3;
  const float dx = wx - p[0], dy = wy - p[1], dz = wz - p[2];
  const float r1 = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
  const float diff = r1 - rest;
  const float e = fabsf(diff);
  const bool quad = e <= delta;
  if (fwd) a.v += quad ? e * e : delta * (2.f * e - delta);
  if (r1 > 0.f) {
    const float slope = quad ? 2.f * e : 2.f * delta;                // rho'(e)
    const float c = (diff > 0.f ? slope : (diff < 0.f ? -slope : 0.f)) / r1;
    a.gx += c * dx, a.gy += c * dy, a.gz += c * dz;
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void iso_pairs_kernel(const float* __restrict__ w, const int32_t* __restrict__ nbr, const float* __restrict__ r0,
                                                        int N, int P, float delta, float* __restrict__ v, float* __restrict__ g) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int64_t row = (int64_t)b * N + i;
  const float* wb = w + (int64_t)b * N * 3;
  const float wx = wb[(int64_t)i * 3], wy = wb[(int64_t)i * 3 + 1], wz = wb[(int64_t)i * 3 + 2];
  IsoAcc a = {0.f, 0.f, 0.f, 0.f};
  if (VEC) {                                                         // P even: the row's 8 P bytes of each table are 16-byte aligned
    const int4* nq = reinterpret_cast<const int4*>(nbr + row * 2 * P);
    const f32x4* rq = reinterpret_cast<const f32x4*>(r0 + row * 2 * P);
    for (int c = 0; c < P / 2; ++c) {
      const int4 q = nq[c];
      const f32x4 r = rq[c];
      const int e = 4 * c;
      iso_entry(wb, wx, wy, wz, q.x, r.x, e < P, delta, N, a);
      iso_entry(wb, wx, wy, wz, q.y, r.y, e + 1 < P, delta, N, a);
      iso_entry(wb, wx, wy, wz, q.z, r.z, e + 2 < P, delta, N, a);
      iso_entry(wb, wx, wy, wz, q.w, r.w, e + 3 < P, delta, N, a);
    }
  } else {
    const int32_t* nq = nbr + row * 2 * P;
    const float* rq = r0 + row * 2 * P;
    for (int e = 0; e < 2 * P; ++e) iso_entry(wb, wx, wy, wz, nq[e], rq[e], e < P, delta, N, a);
  }
  v[row] = a.v;
  g[row * 3] = a.gx, g[row * 3 + 1] = a.gy, g[row * 3 + 2] = a.gz;
}

}  // namespace

extern "C" {

int df_iso_plan(const float* x, const int32_t* count, const int32_t* labels, const int32_t* seg_off, const int32_t* seg_rows, int B, int N,
                int Kcap, int P, int max_cluster_points, int32_t* nbr, float* r0, int32_t* pairs, void* stream) {
  DF_REQUIRE(iso_dims_ok(B, N, P) && Kcap >= 1 && (int64_t)B * (2 * (int64_t)Kcap + 1) < ((int64_t)1 << 31), DF_E_SHAPE);
  DF_REQUIRE(x && count && labels && seg_off && seg_rows && nbr && r0 && pairs && max_cluster_points >= 1, DF_E_ARG);
  DF_REQUIRE(df_aligned16(nbr) && df_aligned16(r0) && (((uintptr_t)x | (uintptr_t)count | (uintptr_t)labels | (uintptr_t)seg_off |
                                                        (uintptr_t)seg_rows | (uintptr_t)pairs) & 3u) == 0,
             DF_E_ALIGN);
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(pairs), 0, (size_t)B, st);
  if (e != hipSuccess) return (int)e;
  iso_plan_kernel<<<dim3((N + 255) / 256, B), 256, 0, st>>>(x, count, labels, seg_off, seg_rows, N, Kcap, P, max_cluster_points, nbr, r0,
                                                            pairs);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

int df_iso_pairs(const float* w, const int32_t* nbr, const float* r0, int B, int N, int P, float delta, float* v, float* g, void* stream) {
  DF_REQUIRE(iso_dims_ok(B, N, P), DF_E_SHAPE);
  DF_REQUIRE(w && nbr && r0 && v && g && delta > 0.f && delta <= 3.0e38f, DF_E_ARG);      // (NaN fails the comparison)
  DF_REQUIRE(df_aligned16(nbr) && df_aligned16(r0) && (((uintptr_t)w | (uintptr_t)v | (uintptr_t)g) & 3u) == 0, DF_E_ALIGN);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((N + 255) / 256, B);
  if (P % 2 == 0) iso_pairs_kernel<true><<<grid, 256, 0, st>>>(w, nbr, r0, N, P, delta, v, g);
  else iso_pairs_kernel<false><<<grid, 256, 0, st>>>(w, nbr, r0, N, P, delta, v, g);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

}  // extern "C"
