// Per-row coordinate MLP (model=nsfp): R^3 -> R^3, width 128, `depth` hidden-to-hidden layers, ReLU, fp32.  Batched over nets: sample b
// reads its own parameter block params + b * param_stride (layout: include/deflow_amd.h).
//
//   df_mlp_fwd   mlp_fwd_kernel, one workgroup (4 waves) per (sample, tile of 64 rows).  The tile's activations [64][128] stay in LDS
//                across all layers of the launch; every hidden layer is 32 x 4 v_mfma_f32_16x16x4_f32 per wave and 16-deep k step, the
//                weights W_l[out][in] streamed from L2 straight into the B fragments (k permutation k = kb + 4 * (lane >> 4) + s, so a
//                fragment fetch is one 16-byte load for W and one ds_read_b128 for the activations).  The 3 -> 128 and 128 -> 3 ends
//                are VALU.  With `acts` the post-ReLU activations of every layer are also written out for the backward.
//   df_mlp_bwd   (1) mlp_dgrad_kernel, same grid: the whole data-gradient chain dz_depth .. dz_0 in one launch, the tile's dz in LDS;
//                da_{l-1} = dz_l W_l runs on the same MFMA with W_l[k = out][n = in] fetched 16 bytes along n (n permutation
//                n = nb + 4 * (lane & 15) + s); every dz_l goes to the workspace, dx (optional) is VALU.
//                (2) mlp_wgrad_kernel, grid (row split, layer, sample): dW_l = dz_l^T a_{l-1} over the split's rows in tiles of 32
//                (MFMA, both operands staged in LDS), db_l = column sums, in ascending row order -> one partial per split.
//                (3) mlp_wreduce_kernel: the partials added in ascending split order; every element of a dparams block written
//                (P elements and the padding up to a multiple of 4, as 0).
// No float atomics; grids come from B, N and depth only; rows >= count[b] contribute nothing and read as x = 0, dy = 0.
#include "common.h"

namespace {

constexpr int MH = 128;          // width
constexpr int MT = 64;           // rows per tile of the forward / data-gradient kernels
constexpr int MLD = 132;         // LDS pitch of an activation tile (floats): 16-byte rows, conflict-free fragment reads
constexpr int MWT = 32;          // rows per tile of the weight-gradient kernel
constexpr int MLDZ = 144;        // LDS pitch of its dz tile (A fragments are read down the rows: 144 % 64 = 16 keeps them apart)
constexpr int MSPLIT = 1024;     // rows per weight-gradient split
constexpr int MLAYER = MH * MH + MH;
constexpr int MIN_SZ = MH * 3 + MH;
constexpr int MOUT_SZ = 3 * MH + 3;

inline int64_t mlp_nparams(int depth) { return (int64_t)MIN_SZ + (int64_t)depth * MLAYER + MOUT_SZ; }
inline int64_t mlp_part_stride(int depth) { return (mlp_nparams(depth) + 3) & ~(int64_t)3; }   // 16-byte partial blocks
inline int mlp_splits(int N) { return (N + MSPLIT - 1) / MSPLIT; }
inline bool mlp_dims_ok(int B, int N, int depth) {
  return B >= 1 && B <= 65535 && N >= 1 && (int64_t)B * N * 3 < 0x7fffffffll && depth >= 0 && depth <= 15;
}

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// ------------------------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(256) void mlp_fwd_kernel(const float* __restrict__ x, const int32_t* __restrict__ count,
                                                      const float* __restrict__ params, int64_t pstride, int N, int depth,
                                                      float* __restrict__ y, float* __restrict__ acts) {
  __shared__ __attribute__((aligned(16))) float As[MT * MLD];
  __shared__ float xs[MT * 4];
  const int b = blockIdx.y, r0 = blockIdx.x * MT, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int cnt = min(max(count[b], 0), N);
  const float* p = params + (int64_t)b * pstride;
  if (tid < MT * 3) {
    const int r = tid / 3, c = tid - 3 * r, row = r0 + r;
    xs[r * 4 + c] = row < cnt ? x[((int64_t)b * N + row) * 3 + c] : 0.f;
  }
  __syncthreads();
  {  // 3 -> 128
    const int o = tid & 127;
    const float w0 = p[o * 3], w1 = p[o * 3 + 1], w2 = p[o * 3 + 2], bb = p[MH * 3 + o];
    float* a0 = acts ? acts + ((int64_t)b * (depth + 1) * N) * MH : nullptr;
#pragma unroll 4
    for (int i = 0; i < MT / 2; ++i) {
      const int r = (tid >> 7) + 2 * i;
      const float z = fmaf(w2, xs[r * 4 + 2], fmaf(w1, xs[r * 4 + 1], fmaf(w0, xs[r * 4], bb)));
      const float a = z > 0.f ? z : 0.f;
      As[r * MLD + o] = a;
      if (a0 && r0 + r < N) a0[(int64_t)(r0 + r) * MH + o] = a;
    }
  }
  for (int l = 1; l <= depth; ++l) {
    const float* W = p + MIN_SZ + (int64_t)(l - 1) * MLAYER;
    const float* bias = W + MH * MH;
    __syncthreads();
    f32x4 acc[4][2];
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[m][0] = acc[m][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* wl = W + (32 * w + (lane & 15)) * MH + (lane >> 4) * 4;
    const float* al = As + (lane & 15) * MLD + (lane >> 4) * 4;
#pragma unroll 2
    for (int kb = 0; kb < MH; kb += 16) {
      const f32x4 b0 = ld4(wl + kb), b1 = ld4(wl + 16 * MH + kb);
      f32x4 a[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) a[m] = ld4(al + m * 16 * MLD + kb);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          acc[m][0] = mfma4(a[m][s], b0[s], acc[m][0]);
          acc[m][1] = mfma4(a[m][s], b1[s], acc[m][1]);
        }
      }
    }
    __syncthreads();
    float* ag = acts ? acts + (((int64_t)b * (depth + 1) + l) * N) * MH : nullptr;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = 32 * w + 16 * j + (lane & 15);
      const float bb = bias[col];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = m * 16 + 4 * (lane >> 4) + r;
          const float z = acc[m][j][r] + bb;
          const float a = z > 0.f ? z : 0.f;
          As[row * MLD + col] = a;
          if (ag && r0 + row < N) ag[(int64_t)(r0 + row) * MH + col] = a;
        }
      }
    }
  }
  __syncthreads();
  if (tid < MT * 3) {  // 128 -> 3
    const int r = tid / 3, c = tid - 3 * r, row = r0 + r;
    const float* wo = p + MIN_SZ + (int64_t)depth * MLAYER + c * MH;
    float s = wo[3 * MH - c * MH + c];   // b_out[c]
    for (int k = 0; k < MH; k += 4) {
      const f32x4 a = ld4(As + r * MLD + k), wv = ld4(wo + k);
      s = fmaf(a[0], wv[0], s);
      s = fmaf(a[1], wv[1], s);
      s = fmaf(a[2], wv[2], s);
      s = fmaf(a[3], wv[3], s);
    }
    if (row < N) y[((int64_t)b * N + row) * 3 + c] = row < cnt ? s : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------------------------ data gradient
__global__ __launch_bounds__(256) void mlp_dgrad_kernel(const int32_t* __restrict__ count, const float* __restrict__ params, int64_t pstride,
                                                        const float* __restrict__ acts, const float* __restrict__ dy, int N, int depth,
                                                        float* __restrict__ dz, float* __restrict__ dx) {
  __shared__ __attribute__((aligned(16))) float Gs[MT * MLD];
  __shared__ float dys[MT * 4];
  const int b = blockIdx.y, r0 = blockIdx.x * MT, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int cnt = min(max(count[b], 0), N);
  const float* p = params + (int64_t)b * pstride;
  const int64_t lay0 = (int64_t)b * (depth + 1) * N;     // row offset of layer 0 of this sample in acts / dz
  if (tid < MT * 3) {
    const int r = tid / 3, c = tid - 3 * r, row = r0 + r;
    dys[r * 4 + c] = row < cnt ? dy[((int64_t)b * N + row) * 3 + c] : 0.f;
  }
  __syncthreads();
  {  // dz_depth = (W_out^T dy) masked by a_depth > 0
    const int o = tid & 127;
    const float* wo = p + MIN_SZ + (int64_t)depth * MLAYER;
    const float w0 = wo[o], w1 = wo[MH + o], w2 = wo[2 * MH + o];
    const int64_t base = (lay0 + (int64_t)depth * N) * MH;
#pragma unroll 4
    for (int i = 0; i < MT / 2; ++i) {
      const int r = (tid >> 7) + 2 * i, row = r0 + r;
      const float da = fmaf(w2, dys[r * 4 + 2], fmaf(w1, dys[r * 4 + 1], w0 * dys[r * 4]));
      float v = 0.f;
      if (row < N) {
        v = acts[base + (int64_t)row * MH + o] > 0.f ? da : 0.f;
        dz[base + (int64_t)row * MH + o] = v;
      }
      Gs[r * MLD + o] = v;
    }
  }
  const int g = w & 1, mh = w >> 1;
  for (int l = depth; l >= 1; --l) {
    const float* W = p + MIN_SZ + (int64_t)(l - 1) * MLAYER;
    __syncthreads();
    f32x4 acc[2][4];
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[0][s] = acc[1][s] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* wl = W + (lane >> 4) * MH + 64 * g + 4 * (lane & 15);
    const float* al = Gs + (mh * 32 + (lane & 15)) * MLD + (lane >> 4);
#pragma unroll 4
    for (int kb = 0; kb < MH; kb += 4) {
      const f32x4 bv = ld4(wl + kb * MH);
      const float a0 = al[kb], a1 = al[16 * MLD + kb];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        acc[0][s] = mfma4(a0, bv[s], acc[0][s]);
        acc[1][s] = mfma4(a1, bv[s], acc[1][s]);
      }
    }
    __syncthreads();
    const int64_t base = (lay0 + (int64_t)(l - 1) * N) * MH;
    const int col = 64 * g + 4 * (lane & 15);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = mh * 32 + m * 16 + 4 * (lane >> 4) + r, row = r0 + rr;
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (row < N) {
          const f32x4 a = ld4(acts + base + (int64_t)row * MH + col);
          v[0] = a[0] > 0.f ? acc[m][0][r] : 0.f;
          v[1] = a[1] > 0.f ? acc[m][1][r] : 0.f;
          v[2] = a[2] > 0.f ? acc[m][2][r] : 0.f;
          v[3] = a[3] > 0.f ? acc[m][3][r] : 0.f;
          st4(dz + base + (int64_t)row * MH + col, v);
        }
        st4(Gs + rr * MLD + col, v);
      }
    }
  }
  __syncthreads();
  if (dx && tid < MT * 3) {  // dx = dz_0 W_in
    const int r = tid / 3, c = tid - 3 * r, row = r0 + r;
    float s = 0.f;
    for (int o = 0; o < MH; ++o) s = fmaf(Gs[r * MLD + o], p[o * 3 + c], s);
    if (row < N) dx[((int64_t)b * N + row) * 3 + c] = row < cnt ? s : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------------------------ weight gradient
// blockIdx: x = split, y = layer (0: input layer, 1..depth: hidden, depth + 1: output layer), z = sample
__global__ __launch_bounds__(256) void mlp_wgrad_kernel(const float* __restrict__ x, const int32_t* __restrict__ count,
                                                        const float* __restrict__ acts, const float* __restrict__ dy,
                                                        const float* __restrict__ dz, int N, int depth, int S, int64_t PS,
                                                        float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float Dz[MWT * MLDZ];
  __shared__ __attribute__((aligned(16))) float Av[MWT * MLD];
  __shared__ float sm[MWT * 4];
  const int s = blockIdx.x, L = blockIdx.y, b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int cnt = min(max(count[b], 0), N);
  const int rs = s * MSPLIT, re = min(rs + MSPLIT, cnt);
  const int64_t lay0 = (int64_t)b * (depth + 1) * N;
  const float* dzl = L <= depth ? dz + (lay0 + (int64_t)L * N) * MH : nullptr;
  const float* avl = L >= 1 ? acts + (lay0 + (int64_t)(L - 1) * N) * MH : nullptr;
  const float* sml = L == 0 ? x : (L == depth + 1 ? dy : nullptr);
  float* out = part + ((int64_t)b * S + s) * PS + (L == 0 ? 0 : MIN_SZ + (int64_t)(L - 1) * MLAYER);
  f32x4 acc[2][2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[m][n][q] = f32x4{0.f, 0.f, 0.f, 0.f};
  float v0 = 0.f, v1 = 0.f, v2 = 0.f;
  for (int t0 = rs; t0 < re; t0 += MWT) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + 256 * i, r = e >> 5, c4 = (e & 31) * 4, row = t0 + r;
      const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
      if (dzl) st4(Dz + r * MLDZ + c4, row < re ? ld4(dzl + (int64_t)row * MH + c4) : z);
      if (avl) st4(Av + r * MLD + c4, row < re ? ld4(avl + (int64_t)row * MH + c4) : z);
    }
    if (sml && tid < MWT * 3) {
      const int r = tid / 3, c = tid - 3 * r, row = t0 + r;
      sm[r * 4 + c] = row < re ? sml[((int64_t)b * N + row) * 3 + c] : 0.f;
    }
    __syncthreads();
    if (L >= 1 && L <= depth) {
      const float* al = Dz + (lane >> 4) * MLDZ + 32 * w + (lane & 15);
      const float* bl = Av + (lane >> 4) * MLD + 4 * (lane & 15);
#pragma unroll 2
      for (int kb = 0; kb < MWT; kb += 4) {
        const float a0 = al[kb * MLDZ], a1 = al[kb * MLDZ + 16];
        const f32x4 b0 = ld4(bl + kb * MLD), b1 = ld4(bl + kb * MLD + 64);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          acc[0][0][q] = mfma4(a0, b0[q], acc[0][0][q]);
          acc[1][0][q] = mfma4(a1, b0[q], acc[1][0][q]);
          acc[0][1][q] = mfma4(a0, b1[q], acc[0][1][q]);
          acc[1][1][q] = mfma4(a1, b1[q], acc[1][1][q]);
        }
      }
      if (tid < MH)
        for (int k = 0; k < MWT; ++k) v0 += Dz[k * MLDZ + tid];
    } else if (L == 0) {
      const int o = tid & 127, h = tid >> 7;
      for (int k = 0; k < MWT; ++k) {
        const float d = Dz[k * MLDZ + o];
        if (h == 0) {
          v0 = fmaf(d, sm[k * 4], v0);
          v1 = fmaf(d, sm[k * 4 + 1], v1);
        } else {
          v0 = fmaf(d, sm[k * 4 + 2], v0);
          v1 += d;
        }
      }
    } else {
      if (tid < MH) {
        for (int k = 0; k < MWT; ++k) {
          const float a = Av[k * MLD + tid];
          v0 = fmaf(sm[k * 4], a, v0);
          v1 = fmaf(sm[k * 4 + 1], a, v1);
          v2 = fmaf(sm[k * 4 + 2], a, v2);
        }
      } else if (tid < MH + 3) {
        for (int k = 0; k < MWT; ++k) v0 += sm[k * 4 + tid - MH];
      }
    }
  }
  if (L >= 1 && L <= depth) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int o = 32 * w + 16 * m + 4 * (lane >> 4) + r, in = 64 * n + 4 * (lane & 15);
          st4(out + o * MH + in, f32x4{acc[m][n][0][r], acc[m][n][1][r], acc[m][n][2][r], acc[m][n][3][r]});
        }
    if (tid < MH) out[MH * MH + tid] = v0;
  } else if (L == 0) {
    const int o = tid & 127;
    if (tid < MH) {
      out[o * 3] = v0;
      out[o * 3 + 1] = v1;
    } else {
      out[o * 3 + 2] = v0;
      out[MH * 3 + o] = v1;
    }
  } else {
    if (tid < MH) {
      out[tid] = v0;
      out[MH + tid] = v1;
      out[2 * MH + tid] = v2;
    } else if (tid < MH + 3) {
      out[3 * MH + tid - MH] = v0;
    }
  }
}

__global__ __launch_bounds__(256) void mlp_wreduce_kernel(const float* __restrict__ part, int S, int64_t P, int64_t PS, int64_t pstride,
                                                          float* __restrict__ dparams) {
  const int b = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= PS) return;          // the block's P elements and its padding up to a multiple of 4 (PS <= pstride)
  float s = 0.f;
  if (i < P) {
    const float* q = part + (int64_t)b * S * PS + i;
    for (int k = 0; k < S; ++k) s += q[(int64_t)k * PS];
  }
  dparams[(int64_t)b * pstride + i] = s;
}

inline int64_t mlp_dz_bytes(int B, int N, int depth) { return (int64_t)B * (depth + 1) * N * MH * 4; }

}  // namespace

extern "C" {

int64_t df_mlp_ws_bytes(int B, int N, int depth) {
  if (!mlp_dims_ok(B, N, depth)) return DF_E_SHAPE;
  return mlp_dz_bytes(B, N, depth) + (int64_t)B * mlp_splits(N) * mlp_part_stride(depth) * 4;
}

int df_mlp_fwd(const float* x, const int32_t* count, const float* params, int64_t param_stride, int B, int N, int depth, float* y,
               float* acts, void* stream) {
  DF_REQUIRE(mlp_dims_ok(B, N, depth), DF_E_SHAPE);
  DF_REQUIRE(x && count && params && y, DF_E_ARG);
  DF_REQUIRE(param_stride >= mlp_nparams(depth) && param_stride % 4 == 0, DF_E_SHAPE);
  DF_REQUIRE(df_aligned16(params) && (!acts || df_aligned16(acts)), DF_E_ALIGN);
  mlp_fwd_kernel<<<dim3((N + MT - 1) / MT, B), 256, 0, (hipStream_t)stream>>>(x, count, params, param_stride, N, depth, y, acts);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

int df_mlp_bwd(const float* x, const int32_t* count, const float* params, int64_t param_stride, const float* acts, const float* dy, int B,
               int N, int depth, float* dparams, float* dx, void* ws, void* stream) {
  DF_REQUIRE(mlp_dims_ok(B, N, depth), DF_E_SHAPE);
  DF_REQUIRE(x && count && params && acts && dy && dparams && ws, DF_E_ARG);
  const int64_t P = mlp_nparams(depth);
  DF_REQUIRE(param_stride >= P && param_stride % 4 == 0, DF_E_SHAPE);
  DF_REQUIRE(df_aligned16(params) && df_aligned16(acts) && df_aligned16(ws), DF_E_ALIGN);
  const int S = mlp_splits(N);
  float* dz = (float*)ws;
  float* part = (float*)((char*)ws + mlp_dz_bytes(B, N, depth));
  hipStream_t st = (hipStream_t)stream;
  mlp_dgrad_kernel<<<dim3((N + MT - 1) / MT, B), 256, 0, st>>>(count, params, param_stride, acts, dy, N, depth, dz, dx);
  DF_CHECK_LAUNCH();
  mlp_wgrad_kernel<<<dim3(S, depth + 2, B), 256, 0, st>>>(x, count, acts, dy, dz, N, depth, S, mlp_part_stride(depth), part);
  DF_CHECK_LAUNCH();
  mlp_wreduce_kernel<<<dim3((unsigned)((mlp_part_stride(depth) + 255) / 256), B), 256, 0, st>>>(part, S, P, mlp_part_stride(depth), param_stride, dparams);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

}  // extern "C"
