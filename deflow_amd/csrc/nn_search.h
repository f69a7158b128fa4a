// The grid search of df_chamfer_nn as a device function, shared by chamfer.hip (df_chamfer_nn) and register.hip (df_reg_accumulate): the
// cell arithmetic of df_nn_grid_build's grid and the ring walk over it.  ONE body, so that the two entries agree bit for bit on the
// distance expression, the tie rule and the stopping rule.  Also the window of the fixed-radius scans over the same grid (nn_window:
// normals.hip, cluster.hip).
#pragma once
#include <math.h>

#include "common.h"

namespace {

__device__ __forceinline__ bool nn_finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// cell coordinate of a FINITE coordinate: clamped in float first, so that no out-of-range float is ever converted to int
__device__ __forceinline__ int nn_cell(float v, float lo, float inv_cell, int G, float* pos /* clamped position, cell units */) {
  const float f = fminf(fmaxf((v - lo) * inv_cell, 0.f), (float)G);
  *pos = f;
  const int c = (int)f;
  return c > G - 1 ? G - 1 : c;
}

// The cells that hold every row within a FIXED radius of a filed row: those that the row's clamped position (px, py), in cell units as
// nn_cell gives it, +- reach covers in x and in y, reach = radius / cell + the 2e-3 cell of slack that nn_ring_search subtracts from its
// lower bound for the fp32 rounding of the cell coordinates.  NOT "the 3 x 3 cells around the row's own": (v - lo) * inv_cell rounds
// differently on the two sides of a binade edge, so at radius == cell two rows a hair less than one cell apart can be filed two cells
// apart.  Rows outside the range sit in the border cells, and clamping is a contraction, so the clamped window still holds them.  With
// radius <= cell: ya >= cy - 2 and yb <= cy + 2 (three cell rows, four for a row within the slack of a cell edge), likewise in x; one
// cell row's cells xa .. xb are one contiguous span of the cell-ordered rows.  Positions lie in [0, G]: every conversion to int is in
// range.  The fixed-radius scans (normals.hip, cluster.hip) use this; they walk the cell rows at a FIXED offset -2 .. 2 from the row's
// own, not from ya, so that the lanes of a wave that share a cell walk the same cell row in the same iteration whichever of them has
// a fourth one (one lane of a crowded cell that started a row early made its whole wave walk the crowd twice: 1.5 x the launch time
// of df_normals at 640 rows in a cell).
struct NnWindow {
  int xa, xb, ya, yb;
};
__device__ __forceinline__ NnWindow nn_window(float px, float py, float reach, int G) {
  const int top = G - 1;
  NnWindow w;
  w.xa = min((int)fmaxf(px - reach, 0.f), top);
  w.xb = min((int)fminf(px + reach, (float)G), top);
  w.ya = min((int)fmaxf(py - reach, 0.f), top);
  w.yb = min((int)fminf(py + reach, (float)G), top);
  return w;
}

// Nearest row of one sample's grid to the FINITE query (qx, qy, qz): rings of cells around the query's own cell (ring r = the cells at
// Chebyshev distance r) until the distance from the query to the edge of the scanned square -- a lower bound for every row not seen yet,
// valid without z -- exceeds the best distance found (or max_dist2).  rng: the sample's G * G cell ranges; sorted: the rows in cell order,
// (x, y, z, bits of the row index).  -> best = the smallest squared distance (differences formed in fp32) and bi = that row, the lowest
// row on equal distances; +inf / -1 when the grid holds no row.  NOT gated: the caller compares best with max_dist2.  KEEP: bv = the
// best row's record (register.hip forms its residual from it); chamfer.hip compiles the search without it.  Returns the number of
// the last ring scanned.
template <bool KEEP>
__device__ __forceinline__ int nn_ring_search(float qx, float qy, float qz, const int32_t* __restrict__ rng, const f32x4* __restrict__ sorted,
                                              float minx, float miny, float cell, int G, float max_dist2, float& best, int& bi, f32x4& bv) {
  const float inv_cell = 1.0f / cell;
  float px, py;
  const int cx = nn_cell(qx, minx, inv_cell, G, &px), cy = nn_cell(qy, miny, inv_cell, G, &py);
  auto scan = [&](int s, int e) {
    for (int p = s; p < e; ++p) {
      const f32x4 v = sorted[p];
      const float dx = v.x - qx, dy = v.y - qy, dz = v.z - qz;
      const float d = dx * dx + dy * dy + dz * dz;
      const float w = v.w;
      const int j = __builtin_bit_cast(int, w);
      if (d < best || (d == best && j < bi)) {
        best = d;
        bi = j;
        if (KEEP) bv = v;
      }
    }
  };
  int r = 0;
  for (; r <= G; ++r) {                                  // at most G + 1 rings: bounded by the grid's extent
    const int x0 = cx - r, x1 = cx + r, y0 = cy - r, y1 = cy + r;
    const int xa = x0 < 0 ? 0 : x0, xb = x1 > G - 1 ? G - 1 : x1;
    const int ya = y0 < 0 ? 0 : y0, yb = y1 > G - 1 ? G - 1 : y1;
    for (int y = ya; y <= yb; ++y) {
      const int32_t* rr = rng + (int64_t)y * G * 2;
      if (y == y0 || y == y1) {
        scan(rr[2 * xa], rr[2 * xb + 1]);                // a whole row of the ring: adjacent cells are one contiguous span
      } else {
        if (x0 >= 0) scan(rr[2 * x0], rr[2 * x0 + 1]);
        if (x1 <= G - 1) scan(rr[2 * x1], rr[2 * x1 + 1]);
      }
    }
    // every row not seen yet lies in a cell outside the square [x0, x1] x [y0, y1], hence -- border cells hold rows clamped INTO the
    // range, and a query outside it is measured from its clamped position, which only shortens -- at least as far in x or y as the
    // nearest side of the square that still has cells beyond it.  (cells: positions in cell units)
    float lb = INFINITY;
    if (x0 > 0) lb = fminf(lb, px - (float)x0);
    if (x1 < G - 1) lb = fminf(lb, (float)(x1 + 1) - px);
    if (y0 > 0) lb = fminf(lb, py - (float)y0);
    if (y1 < G - 1) lb = fminf(lb, (float)(y1 + 1) - py);
    if (!(lb < INFINITY)) break;                         // the square covers the grid
    lb = fmaxf(lb - 2e-3f, 0.f) * cell;                  // slack for the rounding of the cell coordinates (< 1e-3 cell at G <= 4096)
    const float lb2 = lb * lb;
    if (lb2 > best || lb2 > max_dist2) break;            // (equal: keep going -- an equal distance with a lower row index may follow)
  }
  return r;
}

// rows of one padded tensor are addressed as 32-bit sorted positions and keys: B * N (and, for the grid, B * G * G) must stay below 2^30
inline bool nn_rows_ok(int B, int N) { return B > 0 && N > 0 && (int64_t)B * N < 0x3fffffffll; }
inline bool nn_grid_ok(int B, int G) { return G > 0 && G <= 4096 && (int64_t)B * G * G < 0x3fffffffll; }

}  // namespace
