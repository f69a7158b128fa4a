// Whole-sweep flow on the GPU (include/deflow_amd.h): the two steps around the model that the save command needs and
// that collate_fn_pad / the host used to do -- removing the ground rows of a raw sweep, and putting the flow of ALL raw rows together.
//
//   df_sweep_compact   stable compaction of the kept rows (r < count_raw[b], drop == 0) of raw [B,N,3].
//                      (a) sw_count_kernel, grid (blocks, samples), SW_ROWS raw rows per block: the block's number of kept rows
//                          (__ballot / __popcll per wave, the four waves added) -> ws[b][k].
//                      (b) sw_compact_kernel, same grid: a block adds up its predecessors' counts (and all of them: the sample's total),
//                          then per tile of 256 rows a ballot prefix gives each kept row its position.  Position p < total is written by
//                          the one row that lands there, position p >= total (the NaN / -1 padding) by the block whose row range holds p:
//                          every element of pc, row_of, pos_of and kept is written exactly once.
//   df_flow_compose    (a) inv[b][p] = -1 (32-bit memset), (b) inv[b][idx_c[b,i]] = i for i < counts[b] (idx_c holds no duplicates: no two
//                      threads write one element), (c) one thread per raw row: the pose flow with df_ego_transform's operation sequence,
//                      the model's flow through pos_of and inv, the squared-norm flag.  Every output element is written exactly once.
// Integer counts only, no float atomics: the outputs are a pure function of the inputs.
#include <hip/hip_fp16.h>

#include "common.h"

namespace {

constexpr int SW_THREADS = 256;
constexpr int SW_TILES = 4;
constexpr int SW_ROWS = SW_THREADS * SW_TILES;      // raw rows per block (df_sweep_rows_per_block)
constexpr uint32_t SW_NAN = 0x7FC00000u;            // float("nan") as fp32: what collate_fn_pad pads with
constexpr float SW_DYN2 = 0.0025f;                  // (0.05 m per frame)^2

inline int sw_blocks(int N) { return (N + SW_ROWS - 1) / SW_ROWS; }
inline bool sw_dims_ok(int B, int N) { return B >= 1 && B <= 65535 && N >= 1 && (int64_t)B * N < 0x80000000ll; }

// sum of one int per thread over the block's four waves; every thread gets it.  red: 4 ints of LDS, free to reuse after the call
__device__ __forceinline__ int sw_block_sum(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const int s = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return s;
}

__global__ __launch_bounds__(SW_THREADS) void sw_count_kernel(const int32_t* __restrict__ count_raw, const uint8_t* __restrict__ drop, int N,
                                                              int32_t* __restrict__ blk) {
  __shared__ int red[4];
  const int tid = threadIdx.x, b = blockIdx.y, k = blockIdx.x;
  const int cnt = min(max(count_raw[b], 0), N);
  const uint8_t* d = drop + (int64_t)b * N;
  int c = 0;
#pragma unroll
  for (int t = 0; t < SW_TILES; ++t) {
    const int r = k * SW_ROWS + t * SW_THREADS + tid;
    c += (r < cnt && d[r] == 0) ? 1 : 0;
  }
  const int s = sw_block_sum(c, red);
  if (tid == 0) blk[(int64_t)b * gridDim.x + k] = s;
}

__global__ __launch_bounds__(SW_THREADS) void sw_compact_kernel(const uint32_t* __restrict__ raw, const int32_t* __restrict__ count_raw,
                                                                const uint8_t* __restrict__ drop, int N, const int32_t* __restrict__ blk,
                                                                uint32_t* __restrict__ pc, int32_t* __restrict__ row_of,
                                                                int32_t* __restrict__ pos_of, int32_t* __restrict__ kept) {
  __shared__ int red[4];
  __shared__ int s_wc[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, b = blockIdx.y, k = blockIdx.x, K = gridDim.x;
  const int cnt = min(max(count_raw[b], 0), N);
  const int64_t sample = (int64_t)b * N;
  int pre = 0, all = 0;
  for (int j = tid; j < K; j += SW_THREADS) {
    const int v = blk[(int64_t)b * K + j];
    all += v;
    pre += j < k ? v : 0;
  }
  int running = sw_block_sum(pre, red);            // kept rows of the blocks before this one
  const int total = sw_block_sum(all, red);        // kept rows of the sample (<= cnt <= N)
  for (int t = 0; t < SW_TILES; ++t) {
    const int r = k * SW_ROWS + t * SW_THREADS + tid;
    const bool keep = r < cnt && drop[sample + r] == 0;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_wc[w] = __popcll(m);
    __syncthreads();
    int off = running;
#pragma unroll
    for (int q = 0; q < 4; ++q) off += q < w ? s_wc[q] : 0;
    const int tile_total = s_wc[0] + s_wc[1] + s_wc[2] + s_wc[3];
    if (r < N) {
      int p = -1;
      if (keep) {
        p = off + __popcll(m & ((1ull << lane) - 1ull));       // < total: inside the sample
        const uint32_t* src = raw + (sample + r) * 3;
        uint32_t* dst = pc + (sample + p) * 3;
        dst[0] = src[0];
        dst[1] = src[1];
        dst[2] = src[2];
        row_of[sample + p] = r;
      }
      pos_of[sample + r] = p;
      if (r >= total) {                                          // r as a compact position: the padding behind the kept rows
        uint32_t* dst = pc + (sample + r) * 3;
        dst[0] = SW_NAN;
        dst[1] = SW_NAN;
        dst[2] = SW_NAN;
        row_of[sample + r] = -1;
      }
    }
    running += tile_total;
    __syncthreads();
  }
  if (k == 0 && tid == 0) kept[b] = total;
}

__global__ __launch_bounds__(256) void sw_inverse_kernel(const int64_t* __restrict__ idx_c, const int32_t* __restrict__ counts, int N, int Nc,
                                                         int32_t* __restrict__ inv) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const int cnt = min(max(counts[b], 0), Nc);
  if (i >= cnt) return;
  const int64_t j = idx_c[(int64_t)b * Nc + i];
  if (j >= 0 && j < N) inv[(int64_t)b * N + j] = i;
}

template <bool HALF>
__global__ __launch_bounds__(256) void sw_compose_kernel(const float* __restrict__ raw, const int32_t* __restrict__ count_raw,
                                                         const float* __restrict__ T, const int32_t* __restrict__ pos_of,
                                                         const float* __restrict__ flow, const int32_t* __restrict__ inv, int N, int Nc,
                                                         void* __restrict__ flow_est, uint8_t* __restrict__ dynamic) {
  const int b = blockIdx.y, r = blockIdx.x * 256 + threadIdx.x;
  if (r >= N) return;
  const int cnt = min(max(count_raw[b], 0), N);
  const int64_t at = (int64_t)b * N + r;
  float e[3] = {0.f, 0.f, 0.f};
  uint8_t dyn = 0;
  if (r < cnt) {
    const float* p = raw + at * 3;
    const float x = p[0], y = p[1], z = p[2];
    if (isfinite(x) && isfinite(y) && isfinite(z)) {
      const float* M = T + b * 16;
      const float c[3] = {x, y, z};
#pragma unroll
      for (int i = 0; i < 3; ++i) {                 // df_ego_transform's sequence (misc.hip), operation by operation
        float a = __fmul_rn(x, M[i * 4 + 0]);
        a = __fadd_rn(a, __fmul_rn(y, M[i * 4 + 1]));
        a = __fadd_rn(a, __fmul_rn(z, M[i * 4 + 2]));
        a = __fadd_rn(a, M[i * 4 + 3]);
        e[i] = __fsub_rn(a, c[i]);
      }
      const int q = pos_of[at];
      const int i = (q >= 0 && q < N) ? inv[(int64_t)b * N + q] : -1;
      if (i >= 0 && i < Nc) {                        // a row the model decoded
        const float* f = flow + ((int64_t)b * Nc + i) * 3;
        const float fx = f[0], fy = f[1], fz = f[2];
        e[0] = __fadd_rn(e[0], fx);
        e[1] = __fadd_rn(e[1], fy);
        e[2] = __fadd_rn(e[2], fz);
        const float s = __fadd_rn(__fadd_rn(__fmul_rn(fx, fx), __fmul_rn(fy, fy)), __fmul_rn(fz, fz));
        dyn = s >= SW_DYN2 ? 1 : 0;
      }
    }
  }
  if (HALF) {
    __half* o = reinterpret_cast<__half*>(flow_est) + at * 3;
    o[0] = __float2half_rn(e[0]);
    o[1] = __float2half_rn(e[1]);
    o[2] = __float2half_rn(e[2]);
  } else {
    float* o = reinterpret_cast<float*>(flow_est) + at * 3;
    o[0] = e[0];
    o[1] = e[1];
    o[2] = e[2];
  }
  dynamic[at] = dyn;
}

}  // namespace

extern "C" int df_sweep_rows_per_block(void) { return SW_ROWS; }

extern "C" int64_t df_sweep_compact_ws_bytes(int B, int N) {
  return sw_dims_ok(B, N) ? (int64_t)B * sw_blocks(N) * 4 : (int64_t)DF_E_SHAPE;
}

extern "C" int df_sweep_compact(const float* raw, const int32_t* count_raw, const uint8_t* drop, int B, int N, void* ws, float* pc,
                                int32_t* row_of, int32_t* pos_of, int32_t* kept, void* stream) {
  DF_REQUIRE(raw && count_raw && drop && ws && pc && row_of && pos_of && kept, DF_E_ARG);
  DF_REQUIRE(sw_dims_ok(B, N), DF_E_SHAPE);
  DF_REQUIRE((((uintptr_t)ws) & 3u) == 0, DF_E_ALIGN);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int32_t* blk = reinterpret_cast<int32_t*>(ws);
  const dim3 grid(sw_blocks(N), B);
  hipLaunchKernelGGL(sw_count_kernel, grid, dim3(SW_THREADS), 0, s, count_raw, drop, N, blk);
  DF_CHECK_LAUNCH();
  hipLaunchKernelGGL(sw_compact_kernel, grid, dim3(SW_THREADS), 0, s, reinterpret_cast<const uint32_t*>(raw), count_raw, drop, N, blk,
                     reinterpret_cast<uint32_t*>(pc), row_of, pos_of, kept);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

extern "C" int64_t df_flow_compose_ws_bytes(int B, int N) { return sw_dims_ok(B, N) ? (int64_t)B * N * 4 : (int64_t)DF_E_SHAPE; }

extern "C" int df_flow_compose(const float* raw, const int32_t* count_raw, const float* T, const int32_t* pos_of, const float* flow,
                               const int64_t* idx_c, const int32_t* counts, int B, int N, int Nc, int half, void* ws, void* flow_est,
                               uint8_t* dynamic, void* stream) {
  DF_REQUIRE(raw && count_raw && T && pos_of && flow && idx_c && counts && ws && flow_est && dynamic && (half == 0 || half == 1), DF_E_ARG);
  DF_REQUIRE(sw_dims_ok(B, N) && sw_dims_ok(B, Nc), DF_E_SHAPE);
  DF_REQUIRE((((uintptr_t)ws) & 3u) == 0, DF_E_ALIGN);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int32_t* inv = reinterpret_cast<int32_t*>(ws);
  hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(inv), -1, (size_t)B * N, s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sw_inverse_kernel, dim3((Nc + 255) / 256, B), dim3(256), 0, s, idx_c, counts, N, Nc, inv);
  DF_CHECK_LAUNCH();
  const dim3 grid((N + 255) / 256, B);
  if (half)
    hipLaunchKernelGGL(sw_compose_kernel<true>, grid, dim3(256), 0, s, raw, count_raw, T, pos_of, flow, inv, N, Nc, flow_est, dynamic);
  else
    hipLaunchKernelGGL(sw_compose_kernel<false>, grid, dim3(256), 0, s, raw, count_raw, T, pos_of, flow, inv, N, Nc, flow_est, dynamic);
  DF_CHECK_LAUNCH();
  return DF_OK;
}
