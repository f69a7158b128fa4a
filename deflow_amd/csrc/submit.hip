// Leaderboard submission bodies on the GPU (include/deflow_amd.h): the step between df_flow_compose and the feather
// files of ``python -m deflow_amd.eval av2_mode=test``.  The benchmark's rows of a sweep are selected by df_sweep_compact with
// drop = (eval_mask == 0); df_submit_pack gathers through its row_of and writes, per sample, the body of an uncompressed Arrow record batch
// byte for byte: three fp16 columns and one bit-packed boolean column, every buffer padded with zeros to a multiple of 8 bytes.
//
//   submit_pack_kernel   grid (ceil(N / 256), samples), one thread per compact position p.  M = kept[b] clamped to [0, N].
//                        p < M: the fp16 roundings of flow_est[row_of[p]] go to the three columns; M <= p < pad4(M): zeros (the columns'
//                        padding).  A wave's __ballot of its 64 flags IS the wave's 8 bytes of the boolean column (bit p & 7 of byte
//                        p >> 3, LSB first): lane 0 stores them as one 64-bit word when they lie below the column's padded length.
// Bytes [0, L(M)) of a sample are each written exactly once, bytes from L(M) on are not touched; no atomics, no scratch memory: the body is
// a pure function of the inputs.
#include <hip/hip_fp16.h>

#include "common.h"

namespace {

constexpr int SB_THREADS = 256;

inline int64_t sb_pad8(int64_t v) { return (v + 7) & ~(int64_t)7; }
// the body length at M rows: three fp16 columns of pad8(2 M) bytes and one bit column of pad8(ceil(M / 8)) bytes
inline int64_t sb_body_len(int64_t M) { return 3 * sb_pad8(2 * M) + sb_pad8((M + 7) / 8); }
inline int64_t sb_stride(int N) { return (sb_body_len(N) + 63) & ~(int64_t)63; }
inline bool sb_dims_ok(int B, int N) { return B >= 1 && B <= 65535 && N >= 1 && (int64_t)B * sb_stride(N) < 0x80000000ll; }

template <int VERSION>
__global__ __launch_bounds__(SB_THREADS) void submit_pack_kernel(const float* __restrict__ flow_est, const uint8_t* __restrict__ dynamic,
                                                                 const int32_t* __restrict__ row_of, const int32_t* __restrict__ kept, int N,
                                                                 int64_t S, uint8_t* __restrict__ body) {
  const int b = blockIdx.y, p = blockIdx.x * SB_THREADS + threadIdx.x, lane = threadIdx.x & 63;
  const int M = min(max(kept[b], 0), N);
  const int P = (2 * M + 7) & ~7;                     // bytes of one fp16 column, padded
  const int Q = (((M + 7) >> 3) + 7) & ~7;            // bytes of the bit column, padded
  const int64_t sample = (int64_t)b * N;
  uint8_t* out = body + (int64_t)b * S;
  const int cols = VERSION == 1 ? 0 : Q;              // version 1: columns, then is_dynamic; version 2: is_valid, then columns
  const int bits = VERSION == 1 ? 3 * P : 0;
  float e0 = 0.f, e1 = 0.f, e2 = 0.f;
  bool flag = false;
  if (p < M) {
    const int r = row_of[sample + p];
    if (r >= 0 && r < N) {                            // a row_of from df_sweep_compact always is; anything else packs as a zero row
      const float* f = flow_est + (sample + r) * 3;
      e0 = f[0];
      e1 = f[1];
      e2 = f[2];
      flag = dynamic[sample + r] != 0;
    }
    if (VERSION == 2) flag = true;
  }
  const unsigned long long m = __ballot(flag);        // every lane of the wave gets here: no return above
  if (p < (P >> 1)) {                                 // p < M: the value; M <= p < pad4(M): the column's zero padding
    __half* c = reinterpret_cast<__half*>(out + cols) + p;
    c[0] = __float2half_rn(e0);
    c[P >> 1] = __float2half_rn(e1);
    c[P] = __float2half_rn(e2);
  }
  // lane 0's p is a multiple of 64 and Q one of 8: p / 8 < Q puts all 8 bytes below Q, at an 8-byte aligned address
  if (lane == 0 && (p >> 3) < Q) *reinterpret_cast<unsigned long long*>(out + bits + (p >> 3)) = m;
}

}  // namespace

extern "C" int64_t df_submit_body_stride(int N) { return N >= 1 ? sb_stride(N) : (int64_t)DF_E_SHAPE; }

extern "C" int df_submit_pack(const float* flow_est, const uint8_t* dynamic, const int32_t* row_of, const int32_t* kept, int B, int N,
                              int version, uint8_t* body, void* stream) {
  DF_REQUIRE(flow_est && dynamic && row_of && kept && body && (version == 1 || version == 2), DF_E_ARG);
  DF_REQUIRE(sb_dims_ok(B, N), DF_E_SHAPE);
  DF_REQUIRE((((uintptr_t)body) & 7u) == 0, DF_E_ALIGN);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((N + SB_THREADS - 1) / SB_THREADS, B);
  const int64_t S = sb_stride(N);
  if (version == 1)
    hipLaunchKernelGGL(submit_pack_kernel<1>, grid, dim3(SB_THREADS), 0, s, flow_est, dynamic, row_of, kept, N, S, body);
  else
    hipLaunchKernelGGL(submit_pack_kernel<2>, grid, dim3(SB_THREADS), 0, s, flow_est, dynamic, row_of, kept, N, S, body);
  DF_CHECK_LAUNCH();
  return DF_OK;
}
