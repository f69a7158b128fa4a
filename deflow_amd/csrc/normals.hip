// Per-row surface normals of a cloud filed by df_nn_grid_build: what the point-to-plane residual of the sweep-to-sweep registration
// (register.hip: df_reg_accumulate_plane) reads at the matched target row.  UNPINNED -- the definition is this project's own:
// include/deflow_amd.h, DESIGN.md section 6r.
//
//   df_normals   one thread per cell-ordered position.  The rows within radius of a row lie in the cells that its clamped position
//                +- reach covers in x and in y, reach = radius / cell + nn_ring_search's 2e-3 cell of slack for the fp32 rounding of
//                the cell coordinates (clamped at the border as nn_search.h clamps: rows outside the range sit in the border cells,
//                and clamping is a contraction).  NOT "the 3 x 3 cells around its own": (v - lo) * inv_cell rounds differently on the
//                two sides of a binade edge, so at radius == cell two rows a hair less than one cell apart can be filed two cells
//                apart.  With radius <= cell that is three cell rows, four for a row within the slack of a cell edge (and likewise
//                three or four cells per row) -- one contiguous span of the cell-ordered rows per cell row, walked in ascending
//                position.  The differences from the row itself are formed in fp32 (the distance expression is nn_ring_search's),
//                their 3 first and 6 second moments are accumulated in float64, and the covariance's eigenvectors come from
//                NRM_SWEEPS sweeps of cyclic Jacobi in float64.  A fill launch writes the default (0, 0, 0, -1) / m = 0 to every row
//                first.  No atomics, no LDS.
//
// NRM_SWEEPS = 8.  A sweep is the three rotations (0,1), (0,2), (1,2).  Cyclic Jacobi converges quadratically once the off-diagonal
// norm is below the eigenvalue gap, and a 3 x 3 matrix gets there within two or three sweeps from any start: in float64 the
// off-diagonal entries are at rounding level after five sweeps (the classical count for small matrices is 4 to 6), eight leave a margin
// of three.  A rotation whose off-diagonal entry is exactly 0 is skipped, so a finished matrix costs three compares per sweep and a
// cloud whose rows share one z keeps the axis (0, 0, 1) exactly.
#include <math.h>

#include "common.h"
#include "nn_search.h"

namespace {

constexpr int NRM_SWEEPS = 8;

__global__ __launch_bounds__(256) void normals_fill_kernel(int64_t n, f32x4* __restrict__ normals, int32_t* __restrict__ m_out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const f32x4 none = {0.f, 0.f, 0.f, -1.f};
  normals[i] = none;
  if (m_out) m_out[i] = 0;
}

// one rotation of the symmetric A in the (P, Q) plane, accumulated into the columns P, Q of V; skipped when A[P][Q] is exactly 0
template <int P, int Q>
__device__ __forceinline__ void nrm_rotate(double (&A)[3][3], double (&V)[3][3]) {
  constexpr int R = 3 - P - Q;
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));      // (theta = +-inf: t = 0)
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  A[P][P] -= t * apq;
  A[Q][Q] += t * apq;
  A[P][Q] = 0.0;
  A[Q][P] = 0.0;
  const double arp = A[R][P], arq = A[R][Q];
  A[R][P] = A[P][R] = c * arp - s * arq;
  A[R][Q] = A[Q][R] = s * arp + c * arq;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double vkp = V[k][P], vkq = V[k][Q];
    V[k][P] = c * vkp - s * vkq;
    V[k][Q] = s * vkp + c * vkq;
  }
}

__global__ __launch_bounds__(256) void normals_kernel(const int32_t* __restrict__ cell_rng, const f32x4* __restrict__ sorted, int N,
                                                      float minx, float miny, float inv_cell, int G, float r2, float reach, int min_pts,
                                                      float max_curv, f32x4* __restrict__ normals, int32_t* __restrict__ m_out) {
  const int b = blockIdx.y;
  const int32_t* rng = cell_rng + (int64_t)b * G * G * 2;
  // the sample's positions in the cell-ordered rows, held to the buffer's B N records whatever the ranges say
  const int64_t total = (int64_t)gridDim.y * N;
  const int64_t s0 = rng[0];
  int64_t e0 = rng[2 * ((int64_t)G * G - 1) + 1];
  if (e0 > s0 + N) e0 = s0 + N;
  if (e0 > total) e0 = total;
  const int64_t p = s0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s0 < 0 || p >= e0) return;
  const f32x4 me = sorted[p];
  const float mw = me.w;
  const int row = __builtin_bit_cast(int, mw);
  if ((unsigned)row >= (unsigned)N) return;
  float px, py;
  nn_cell(me.x, minx, inv_cell, G, &px);
  const int cy = nn_cell(me.y, miny, inv_cell, G, &py);
  const NnWindow win = nn_window(px, py, reach, G);         // (nn_search.h: the cells that the clamped position +- reach covers)
  int m = 0;
  double sx = 0.0, sy = 0.0, sz = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
  // ya >= cy - 2 and yb <= cy + 2; the cell rows are walked at a FIXED offset from the row's own, not from ya (nn_search.h says why)
#pragma unroll
  for (int k = -2; k <= 2; ++k) {                          // ascending cell row = ascending position
    const int y = cy + k;
    if (y < win.ya || y > win.yb) continue;
    const int32_t* rr = rng + (int64_t)y * G * 2;
    int64_t s = rr[2 * win.xa], e = rr[2 * win.xb + 1];
    if (s < s0) s = s0;
    if (e > e0) e = e0;
    for (int64_t q = s; q < e; ++q) {
      const f32x4 v = sorted[q];
      const float dx = v.x - me.x, dy = v.y - me.y, dz = v.z - me.z;
      const float d = dx * dx + dy * dy + dz * dz;
      if (d <= r2) {
        const double x = (double)dx, yy = (double)dy, z = (double)dz;
        ++m;
        sx += x;
        sy += yy;
        sz += z;
        sxx += x * x;
        sxy += x * yy;
        sxz += x * z;
        syy += yy * yy;
        syz += yy * z;
        szz += z * z;
      }
    }
  }
  const int64_t o = (int64_t)b * N + row;
  if (m_out) m_out[o] = m;
  if (m < min_pts) return;
  const double inv = 1.0 / (double)m;
  const double mx = sx * inv, my = sy * inv, mz = sz * inv;
  double A[3][3], V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  A[0][0] = sxx * inv - mx * mx;
  A[0][1] = A[1][0] = sxy * inv - mx * my;
  A[0][2] = A[2][0] = sxz * inv - mx * mz;
  A[1][1] = syy * inv - my * my;
  A[1][2] = A[2][1] = syz * inv - my * mz;
  A[2][2] = szz * inv - mz * mz;
#pragma unroll 1
  for (int it = 0; it < NRM_SWEEPS; ++it) {
    nrm_rotate<0, 1>(A, V);
    nrm_rotate<0, 2>(A, V);
    nrm_rotate<1, 2>(A, V);
  }
  const double l0 = A[0][0], l1 = A[1][1], l2 = A[2][2];
  // the smallest eigenvalue; on equal values the later axis
  const int i0 = (l2 <= l0 && l2 <= l1) ? 2 : (l1 <= l0 ? 1 : 0);
  const double lmin = i0 == 2 ? l2 : (i0 == 1 ? l1 : l0);
  const double trace = (l0 + l1) + l2;
  if (!(trace > 0.0)) return;
  const float curv = (float)fmax(lmin / trace, 0.0);      // (a rounding-level negative eigenvalue of a flat neighbourhood: 0)
  if (!(curv <= max_curv)) return;
  float nx = (float)(i0 == 2 ? V[0][2] : (i0 == 1 ? V[0][1] : V[0][0]));
  float ny = (float)(i0 == 2 ? V[1][2] : (i0 == 1 ? V[1][1] : V[1][0]));
  float nz = (float)(i0 == 2 ? V[2][2] : (i0 == 1 ? V[2][1] : V[2][0]));
  // towards the frame's origin: n . p <= 0 (products of fp32 values are exact in float64; added left to right, no fma); on 0 the first
  // non-zero component is positive
  const double dot = __dadd_rn(__dadd_rn(__dmul_rn((double)nx, (double)me.x), __dmul_rn((double)ny, (double)me.y)),
                               __dmul_rn((double)nz, (double)me.z));
  const float lead = nx != 0.f ? nx : (ny != 0.f ? ny : nz);
  if (dot > 0.0 || (dot == 0.0 && lead < 0.f)) {
    nx = 0.f - nx;                                         // (0 - x, not -x: a zero component stays +0)
    ny = 0.f - ny;
    nz = 0.f - nz;
  }
  const f32x4 out = {nx, ny, nz, curv};
  normals[o] = out;
}

}  // namespace

extern "C" int df_normals(const int32_t* cell_rng, const float* sorted, float minx, float miny, float cell, int G, int B, int N,
                          float radius, int min_pts, float max_curv, float* normals, int32_t* m_out, void* stream) {
  DF_REQUIRE(cell_rng && sorted && normals, DF_E_ARG);
  DF_REQUIRE(nn_rows_ok(B, N) && nn_grid_ok(B, G) && B <= 65535, DF_E_SHAPE);
  DF_REQUIRE(isfinite(minx) && isfinite(miny) && isfinite(cell) && cell > 0.f, DF_E_ARG);
  DF_REQUIRE(radius > 0.f && radius <= cell && min_pts >= 3 && max_curv > 0.f && max_curv <= 1.0f / 3.0f, DF_E_ARG);    // (NaN fails)
  DF_REQUIRE(df_aligned16(sorted) && df_aligned16(normals) && ((uintptr_t)m_out & 3u) == 0, DF_E_ALIGN);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t n = (int64_t)B * N;
  const float inv_cell = 1.0f / cell;
  hipLaunchKernelGGL(normals_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, reinterpret_cast<f32x4*>(normals), m_out);
  DF_CHECK_LAUNCH();
  hipLaunchKernelGGL(normals_kernel, dim3((N + 255) / 256, B), dim3(256), 0, s, cell_rng, reinterpret_cast<const f32x4*>(sorted), N, minx,
                     miny, inv_cell, G, radius * radius, radius * inv_cell + 2e-3f, min_pts, max_curv, reinterpret_cast<f32x4*>(normals),
                     m_out);
  DF_CHECK_LAUNCH();
  return DF_OK;
}
