// Training augmentation of a padded device batch (include/deflow_amd.h): flip, yaw, height, jitter and point dropout
// of both clouds, the linear part on the flow labels, and the conjugated ego motion / poses -- one launch, nothing read back, every value
// a pure function of (seed, epoch, sample id, row).
//
//   augment_kernel   grid (ceil(N0 / 1024) + ceil(N1 / 1024), B), 256 threads.  The first ceil(N0 / 1024) blocks of a sample take 1024 rows
//                    of pc0 (and of flow) each, the others 1024 rows of pc1.  Thread 0 re-derives the sample's four words (ten Philox
//                    rounds), evaluates sincos in double and leaves the draw in LDS; block (0, b) also writes T', pose0', pose1' (16 threads,
//                    one element each, composed in double).
//                    vector form (the cloud's N % 4 == 0 and its buffers 16-byte aligned, decided on the host): a lane takes four
//                    consecutive rows = 48 bytes = three 16-byte loads and stores; every sample then starts 16-byte aligned and there is
//                    no tail.  scalar form (any other N or alignment): a lane takes rows t, t + 256, t + 512, t + 768 of the block's 1024
//                    with three 4-byte accesses each, neighbouring lanes on neighbouring rows, each row guarded by r < N -- the guard is
//                    the tail.
//   augment_params_kernel   one thread per sample: the draw as eight floats.
// No atomics, no scratch buffers: two runs are bit-identical.  The per-row words are only drawn when jitter or dropout is on.
#include "common.h"

#include "augment_rng.h"

namespace {

constexpr int AG_THREADS = 256;
constexpr int AG_ROWS = 4 * AG_THREADS;     // rows per block
constexpr uint32_t AG_SAMPLE_ROW = 0xffffffffu;

struct ag_cfg {
  uint32_t k0, k1;                          // Philox key: seed, epoch
  float flip_x_p, flip_y_p, yaw_max, height_max, sj /* sigma / 147.8 */, drop_p;
};

struct ag_draw {
  float sx, sy, c, s, dz, theta;
  double cd, sd;                            // cos / sin in double: the matrices are composed with these
};

__device__ __forceinline__ ag_draw ag_sample_draw(int64_t id, const ag_cfg& g) {
  uint32_t w[4];
  df_philox4x32_10((uint32_t)(uint64_t)id, (uint32_t)((uint64_t)id >> 32), AG_SAMPLE_ROW, 0u, g.k0, g.k1, w);
  ag_draw d;
  d.sx = df_u01(w[0]) < g.flip_x_p ? -1.f : 1.f;
  d.sy = df_u01(w[1]) < g.flip_y_p ? -1.f : 1.f;
  const double th = (double)(2.f * df_u01(w[2]) - 1.f) * (double)g.yaw_max;     // (2 u - 1 is exact in fp32)
  d.theta = (float)th;
  double sd = 0.0, cd = 1.0;
  if (g.yaw_max != 0.f) sincos(th, &sd, &cd);
  d.sd = sd;
  d.cd = cd;
  d.c = (float)d.cd;
  d.s = (float)d.sd;
  d.dz = (2.f * df_u01(w[3]) - 1.f) * g.height_max;                              // one fp32 rounding
  return d;
}

struct ag_lds {
  double A[16], Ai[16];
  float sx, sy, c, s, dz;
};

// L (x, y): the flip, then the rotation (contracted to FMAs); rot is uniform
__device__ __forceinline__ void ag_linear(float& x, float& y, const ag_lds& q, bool rot) {
  const float x1 = q.sx * x, y1 = q.sy * y;
  if (rot) {
    x = q.c * x1 - q.s * y1;
    y = q.s * x1 + q.c * y1;
  } else {
    x = x1;
    y = y1;
  }
}

// one row of a cloud: linear part, height, then -- noise is uniform -- the row's own words: jitter and dropout
__device__ __forceinline__ void ag_point(float& x, float& y, float& z, const ag_lds& q, bool rot, bool noise, const ag_cfg& g, uint32_t id_lo,
                                         uint32_t id_hi, uint32_t row, uint32_t purpose) {
  ag_linear(x, y, q, rot);
  z = z + q.dz;
  if (noise) {
    uint32_t w[4];
    df_philox4x32_10(id_lo, id_hi, row, purpose, g.k0, g.k1, w);
    if (g.sj > 0.f) {
      x += df_bell(w[0]) * g.sj;
      y += df_bell(w[1]) * g.sj;
      z += df_bell(w[2]) * g.sj;
    }
    if (df_u01(w[3]) < g.drop_p) x = y = z = __builtin_bit_cast(float, 0x7FC00000u);
  }
}

// element (i, j) of A M A^-1 (conj) or M A^-1, in double.  A = [L a; 0 1], L = Rz(theta) diag(sx, sy, 1), a = (0, 0, dz);
// A^-1 = [Li ai; 0 1], Li = diag(sx, sy, 1) Rz(-theta), ai = (0, 0, -dz): both in LDS, row-major
__device__ __forceinline__ float ag_compose(const float* __restrict__ M, const ag_lds& q, bool conj, int i, int j) {
  double acc = 0;
  for (int k = 0; k < 4; ++k) {
    double p;                                 // (A M)[i][k] or M[i][k]
    if (conj) {
      p = 0;
      for (int l = 0; l < 4; ++l) p += q.A[i * 4 + l] * (double)M[l * 4 + k];
    } else {
      p = (double)M[i * 4 + k];
    }
    acc += p * q.Ai[k * 4 + j];
  }
  return (float)acc;
}

__global__ __launch_bounds__(AG_THREADS) void augment_kernel(const float* __restrict__ pc0, const float* __restrict__ pc1,
                                                             const float* __restrict__ flow, const int64_t* __restrict__ ids, int N0, int N1,
                                                             int nb0, ag_cfg g, int vec0, int vec1, const float* __restrict__ T,
                                                             const float* __restrict__ pose0, const float* __restrict__ pose1,
                                                             float* __restrict__ out0, float* __restrict__ out1, float* __restrict__ flow_out,
                                                             float* __restrict__ T_out, float* __restrict__ pose0_out,
                                                             float* __restrict__ pose1_out) {
  __shared__ ag_lds q;
  const int b = blockIdx.y, t = threadIdx.x;
  const int64_t id = ids[b];
  if (t == 0) {
    const ag_draw d = ag_sample_draw(id, g);
    q.sx = d.sx;
    q.sy = d.sy;
    q.c = d.c;
    q.s = d.s;
    q.dz = d.dz;
    const double sx = d.sx, sy = d.sy, c = d.cd, s = d.sd, dz = d.dz;
    const double A[16] = {c * sx, -s * sy, 0, 0, s * sx, c * sy, 0, 0, 0, 0, 1, dz, 0, 0, 0, 1};
    const double Ai[16] = {sx * c, sx * s, 0, 0, -sy * s, sy * c, 0, 0, 0, 0, 1, -dz, 0, 0, 0, 1};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      q.A[k] = A[k];
      q.Ai[k] = Ai[k];
    }
  }
  __syncthreads();
  if (blockIdx.x == 0 && t < 16) {
    const int64_t m = (int64_t)b * 16;
    if (T) T_out[m + t] = ag_compose(T + m, q, true, t >> 2, t & 3);
    if (pose0) pose0_out[m + t] = ag_compose(pose0 + m, q, false, t >> 2, t & 3);
    if (pose1) pose1_out[m + t] = ag_compose(pose1 + m, q, false, t >> 2, t & 3);
  }
  const bool second = (int)blockIdx.x >= nb0;             // uniform: this block's cloud
  const int N = second ? N1 : N0;
  const float* __restrict__ src = (second ? pc1 : pc0) + (int64_t)b * N * 3;
  float* __restrict__ dst = (second ? out1 : out0) + (int64_t)b * N * 3;
  const float* __restrict__ fsrc = (second || !flow) ? nullptr : flow + (int64_t)b * N * 3;
  float* __restrict__ fdst = flow_out + (fsrc ? (int64_t)b * N * 3 : 0);
  const int row0 = ((int)blockIdx.x - (second ? nb0 : 0)) * AG_ROWS;
  const uint32_t purpose = second ? 2u : 1u, id_lo = (uint32_t)(uint64_t)id, id_hi = (uint32_t)((uint64_t)id >> 32);
  const bool rot = g.yaw_max != 0.f, noise = g.sj > 0.f || g.drop_p > 0.f;
  if (second ? vec1 : vec0) {
    const int r = row0 + 4 * t;                           // N % 4 == 0: all four rows or none
    if (r >= N) return;
    const int64_t e = (int64_t)r * 3;
    float v[12];
    {
      const f32x4 a = ld4(src + e), bq = ld4(src + e + 4), cq = ld4(src + e + 8);
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = bq.x; v[5] = bq.y; v[6] = bq.z; v[7] = bq.w;
      v[8] = cq.x; v[9] = cq.y; v[10] = cq.z; v[11] = cq.w;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) ag_point(v[3 * k], v[3 * k + 1], v[3 * k + 2], q, rot, noise, g, id_lo, id_hi, (uint32_t)(r + k), purpose);
    st4(dst + e, f32x4{v[0], v[1], v[2], v[3]});
    st4(dst + e + 4, f32x4{v[4], v[5], v[6], v[7]});
    st4(dst + e + 8, f32x4{v[8], v[9], v[10], v[11]});
    if (fsrc) {
      const f32x4 a = ld4(fsrc + e), bq = ld4(fsrc + e + 4), cq = ld4(fsrc + e + 8);
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = bq.x; v[5] = bq.y; v[6] = bq.z; v[7] = bq.w;
      v[8] = cq.x; v[9] = cq.y; v[10] = cq.z; v[11] = cq.w;
#pragma unroll
      for (int k = 0; k < 4; ++k) ag_linear(v[3 * k], v[3 * k + 1], q, rot);
      st4(fdst + e, f32x4{v[0], v[1], v[2], v[3]});
      st4(fdst + e + 4, f32x4{v[4], v[5], v[6], v[7]});
      st4(fdst + e + 8, f32x4{v[8], v[9], v[10], v[11]});
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int r = row0 + k * AG_THREADS + t;
      if (r >= N) break;
      const int64_t e = (int64_t)r * 3;
      float x = src[e], y = src[e + 1], z = src[e + 2];
      ag_point(x, y, z, q, rot, noise, g, id_lo, id_hi, (uint32_t)r, purpose);
      dst[e] = x;
      dst[e + 1] = y;
      dst[e + 2] = z;
      if (fsrc) {
        float fx = fsrc[e], fy = fsrc[e + 1];
        ag_linear(fx, fy, q, rot);
        fdst[e] = fx;
        fdst[e + 1] = fy;
        fdst[e + 2] = fsrc[e + 2];
      }
    }
  }
}

__global__ __launch_bounds__(64) void augment_params_kernel(const int64_t* __restrict__ ids, int B, ag_cfg g, float* __restrict__ out) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const ag_draw d = ag_sample_draw(ids[b], g);
  float* o = out + (int64_t)b * 8;
  o[0] = d.sx;
  o[1] = d.sy;
  o[2] = d.c;
  o[3] = d.s;
  o[4] = d.dz;
  o[5] = d.theta;
  o[6] = 0.f;
  o[7] = 0.f;
}

inline bool ag_prob(float p) { return p >= 0.f && p <= 1.f; }            // false for NaN
inline bool ag_size(float v) { return v >= 0.f && v <= 3.0e38f; }        // finite and non-negative
inline bool ag_cfg_ok(float fx, float fy, float yaw, float h, float sg, float dp) {
  return ag_prob(fx) && ag_prob(fy) && ag_prob(dp) && ag_size(yaw) && ag_size(h) && ag_size(sg);
}
inline ag_cfg ag_make(int64_t seed, int64_t epoch, float fx, float fy, float yaw, float h, float sg, float dp) {
  return ag_cfg{(uint32_t)(uint64_t)seed, (uint32_t)(uint64_t)epoch, fx, fy, yaw, h, (float)((double)sg / 147.8), dp};
}

}  // namespace

extern "C" int df_augment(const float* pc0, const float* pc1, const float* flow, const int64_t* sample_ids, int B, int N0, int N1,
                          int64_t seed, int64_t epoch, float flip_x_p, float flip_y_p, float yaw_max, float height_max, float jitter_sigma,
                          float drop_p, const float* T, const float* pose0, const float* pose1, float* pc0_out, float* pc1_out,
                          float* flow_out, float* T_out, float* pose0_out, float* pose1_out, void* stream) {
  DF_REQUIRE(pc0 && pc1 && sample_ids && pc0_out && pc1_out, DF_E_ARG);
  DF_REQUIRE((flow == nullptr) == (flow_out == nullptr) && (T == nullptr) == (T_out == nullptr), DF_E_ARG);
  DF_REQUIRE((pose0 == nullptr) == (pose0_out == nullptr) && (pose1 == nullptr) == (pose1_out == nullptr), DF_E_ARG);
  DF_REQUIRE(pc0 != pc0_out && pc1 != pc1_out && (!flow || flow != flow_out), DF_E_ARG);     // the input batch is never modified
  DF_REQUIRE(ag_cfg_ok(flip_x_p, flip_y_p, yaw_max, height_max, jitter_sigma, drop_p), DF_E_ARG);
  DF_REQUIRE(B >= 1 && B <= 65535 && N0 >= 1 && N1 >= 1, DF_E_SHAPE);
  DF_REQUIRE((int64_t)B * N0 < 0x80000000ll && (int64_t)B * N1 < 0x80000000ll, DF_E_SHAPE);
  const int vec0 = (N0 % 4 == 0) && df_aligned16(pc0) && df_aligned16(pc0_out) && (!flow || (df_aligned16(flow) && df_aligned16(flow_out)));
  const int vec1 = (N1 % 4 == 0) && df_aligned16(pc1) && df_aligned16(pc1_out);
  const int nb0 = (N0 + AG_ROWS - 1) / AG_ROWS, nb1 = (N1 + AG_ROWS - 1) / AG_ROWS;
  hipLaunchKernelGGL(augment_kernel, dim3(nb0 + nb1, B), dim3(AG_THREADS), 0, reinterpret_cast<hipStream_t>(stream), pc0, pc1, flow,
                     sample_ids, N0, N1, nb0, ag_make(seed, epoch, flip_x_p, flip_y_p, yaw_max, height_max, jitter_sigma, drop_p), vec0, vec1,
                     T, pose0, pose1, pc0_out, pc1_out, flow_out, T_out, pose0_out, pose1_out);
  DF_CHECK_LAUNCH();
  return DF_OK;
}

extern "C" int df_augment_params(const int64_t* sample_ids, int B, int64_t seed, int64_t epoch, float flip_x_p, float flip_y_p, float yaw_max,
                                 float height_max, float jitter_sigma, float drop_p, float* params, void* stream) {
  DF_REQUIRE(sample_ids && params, DF_E_ARG);
  DF_REQUIRE(ag_cfg_ok(flip_x_p, flip_y_p, yaw_max, height_max, jitter_sigma, drop_p), DF_E_ARG);
  DF_REQUIRE(B >= 1 && B <= 65535, DF_E_SHAPE);
  hipLaunchKernelGGL(augment_params_kernel, dim3((B + 63) / 64), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), sample_ids, B,
                     ag_make(seed, epoch, flip_x_p, flip_y_p, yaw_max, height_max, jitter_sigma, drop_p), params);
  DF_CHECK_LAUNCH();
  return DF_OK;
}
