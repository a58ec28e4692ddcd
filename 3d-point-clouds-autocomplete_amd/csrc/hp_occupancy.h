// The cell decision of the occupancy grid (occupancy.hip): which kept cell centre of the R^3 grid is nearest to a point,
// by Euclidean distance evaluated in fp64 on the fp32 inputs — the answer of an exhaustive fp64 arg-min over the kept
// centres.  One host/device function, so a host program can run the very code
// of the kernel over recorded points.  Exactly equal distances: the lower (i, j) column wins, inside a column the k nearest
// to the point (the lower k if two are equally near).
//
// The grid is described by two host-built tables (hyperpocket_amd/utils/metrics.py builds them from numpy's membership
// test, the device re-derives nothing):
//   axis[R]       the R centre coordinates of one axis, fp32 values widened to fp64
//   columns[R*R]  one word per (i, j) column of cells: the kept cells of a column are k in [klo, khi] (a clipped sphere is
//                 convex in k) and their kept indices are base + (k - klo), row-major over (i, j, k) as the reference lists
//                 them.  Packed klo | khi << 6 | base << 12 (R <= 64, base < 64^3 = 2^18); klo > khi marks an empty column.
//
// Search: the unclipped nearest cell (per-axis nearest centre) is the answer whenever it is kept — it is the minimum over
// a superset.  Otherwise every non-empty column is visited in (i, j) order; inside a column the squared distance
// fma(dz, dz, dxy) is monotone in |dz|, so its minimum sits at the per-axis nearest k clamped into [klo, khi] and no other k
// of the column needs evaluating.  R^2 column visits per searched point instead of one per kept centre (784 against 10 144
// at R = 28).
#pragma once
#include <hip/hip_runtime.h>

namespace hp {

constexpr int kOccupancyMaxR = 64;

__host__ __device__ inline unsigned occupancy_pack_column(int klo, int khi, int base) {
    return (unsigned)klo | (unsigned)khi << 6 | (unsigned)base << 12;
}

// index of the axis centre nearest to p in fp64; the lower index on an exact tie.  p finite.
__host__ __device__ inline int occupancy_axis_nearest(double p, int R, const double* axis) {
    double t = (p + 0.5) * (double)(R - 1) + 0.5;
    t = t < 0.0 ? 0.0 : (t > (double)(R - 1) ? (double)(R - 1) : t);
    int k = (int)t;
    // the estimate is the answer up to the fp32 rounding of the axis; settle it on the axis values themselves
    while (k > 0 && fabs(axis[k - 1] - p) <= fabs(axis[k] - p)) --k;
    while (k < R - 1 && fabs(axis[k + 1] - p) < fabs(axis[k] - p)) ++k;
    return k;
}

// kept index of the cell (column word `col`, axis index k), or -1 if that cell is not kept
__host__ __device__ inline int occupancy_kept_index(unsigned col, int k) {
    const int klo = col & 63, khi = (col >> 6) & 63;
    return (k >= klo && k <= khi) ? (int)(col >> 12) + (k - klo) : -1;
}

// exhaustive fp64 arg-min over the kept cells, column by column; kz = occupancy_axis_nearest(pz)
__host__ __device__ inline int occupancy_search(double px, double py, double pz, int kz, int R, const double* axis,
                                                const unsigned* columns) {
    double best = __builtin_inf();
    int cell = -1;
    for (int i = 0; i < R; ++i) {
        const double dx = axis[i] - px, dx2 = dx * dx;
        for (int j = 0; j < R; ++j) {
            const unsigned col = columns[i * R + j];
            const int klo = col & 63, khi = (col >> 6) & 63;
            if (klo > khi) continue;
            const double dy = axis[j] - py, dxy = __builtin_fma(dy, dy, dx2);
            const int k = kz < klo ? klo : (kz > khi ? khi : kz);
            const double dz = axis[k] - pz, d = __builtin_fma(dz, dz, dxy);
            if (d < best) {      // strict: columns come in kept-index order, the first of equal distances stays
                best = d;
                cell = (int)(col >> 12) + (k - klo);
            }
        }
    }
    return cell;
}

}  // namespace hp
