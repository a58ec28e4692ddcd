// Occupancy-grid histograms of a set of point clouds: the device half of the JSD of the generativity evaluation.
//
// Replaces (behaviour, not code): utils/metrics.py:279-318 of the reference, which fits sklearn's NearestNeighbors on the
// centres of the grid cells kept inside the sphere of radius 0.5 and walks every point of every cloud in Python.
//
// For clouds (S, n, 3) and a grid of resolution R:
//   counters[c]   += 1 for every point whose nearest kept centre is c
//   clouds_hit[c] += 1 for every cloud that has at least one such point
// Both are integer sums: exact, the same bits whatever the launch shape or the order the atomics land in.
//
// Design:
//  * "nearest" is decided in fp64 by hp::occupancy_* (hp_occupancy.h): the per-axis nearest cell when it is kept, else a
//    search of the R^2 cell columns that equals the exhaustive fp64 arg-min over the kept centres.
//  * a workgroup owns a cloud at a time (a grid-stride loop over S, so S is not bounded by a grid dimension) and with it the
//    cloud's bitmap of hit cells in LDS (one bit per kept cell, 32 KB at R = 64): clouds_hit needs no cross-workgroup
//    de-duplication.  Axis (fp64) and column table sit in LDS too: the search reads them as wave-uniform broadcasts, except
//    the one axis[k] gather per column.
//  * points are taken 1024 at a time.  Pass 1 settles every point whose per-axis cell is kept and queues the others in
//    LDS; pass 2 walks the queue with consecutive lanes, so the waves of the search are full whatever share of the points
//    needs it (0 % well inside the ball, 60 % on the sphere's surface, 70 % in a cube of side 1.2).
//  * counters take one global integer atomicAdd per point (no return value used), the bitmap an LDS atomicOr; after the
//    cloud's last point each set bit becomes one global atomicAdd on clouds_hit.  No float atomics anywhere.
//  * a NaN/Inf coordinate sets *nonfinite and the point is left out; the Python caller raises on the flag.
#include "hp_common.h"
#include "hp_occupancy.h"
#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 1024;          // points per pass; the queue's capacity
constexpr int kMaxBlocks = 2048;      // 8 workgroups per CU in flight cover the device; more clouds loop

struct OccArgs {
    const float* clouds;      // (S, n, 3)
    const float* axis;        // (R)
    const unsigned* columns;  // (R*R) packed (hp_occupancy.h)
    int* counters;            // (cells)
    int* clouds_hit;          // (cells)
    int* nonfinite;           // (1)
    int S, n, R, cells;
};

// the range test costs nothing next to the atomics and keeps an inconsistent table from writing outside the outputs
__device__ __forceinline__ void record(const OccArgs& p, unsigned* bitmap, int cell) {
    if ((unsigned)cell >= (unsigned)p.cells) return;
    atomicAdd(&p.counters[cell], 1);
    atomicOr(&bitmap[cell >> 5], 1u << (cell & 31));
}

__global__ __launch_bounds__(kThreads) void occupancy_kernel(const OccArgs p) {
    extern __shared__ double smem[];
    const int R = p.R, words = (p.cells + 31) >> 5;
    double* axis = smem;                                  // R
    unsigned* columns = (unsigned*)(axis + R);            // R*R
    unsigned* bitmap = columns + R * R;                   // words
    int* queue = (int*)(bitmap + words);                  // kChunk
    int* queued = queue + kChunk;                         // 1
    const int tid = threadIdx.x;

    for (int i = tid; i < R; i += kThreads) axis[i] = (double)p.axis[i];
    for (int i = tid; i < R * R; i += kThreads) columns[i] = p.columns[i];
    bool bad = false;

    for (int cloud = blockIdx.x; cloud < p.S; cloud += gridDim.x) {
        const float* pts = p.clouds + (size_t)cloud * p.n * 3;
        for (int w = tid; w < words; w += kThreads) bitmap[w] = 0u;
        for (int c0 = 0; c0 < p.n; c0 += kChunk) {
            if (tid == 0) *queued = 0;
            __syncthreads();      // also: tables and the cleared bitmap are visible
            const int c1 = min(c0 + kChunk, p.n);
            for (int j = c0 + tid; j < c1; j += kThreads) {
                const float x = pts[(size_t)j * 3], y = pts[(size_t)j * 3 + 1], z = pts[(size_t)j * 3 + 2];
                if (!(isfinite(x) && isfinite(y) && isfinite(z))) {
                    bad = true;
                    continue;
                }
                const int ki = hp::occupancy_axis_nearest((double)x, R, axis);
                const int kj = hp::occupancy_axis_nearest((double)y, R, axis);
                const int kz = hp::occupancy_axis_nearest((double)z, R, axis);
                const int cell = hp::occupancy_kept_index(columns[ki * R + kj], kz);
                if (cell >= 0) record(p, bitmap, cell);
                else queue[atomicAdd(queued, 1)] = j;
            }
            __syncthreads();
            const int nq = *queued;
            for (int q = tid; q < nq; q += kThreads) {
                const int j = queue[q];
                const double x = (double)pts[(size_t)j * 3], y = (double)pts[(size_t)j * 3 + 1],
                             z = (double)pts[(size_t)j * 3 + 2];
                const int kz = hp::occupancy_axis_nearest(z, R, axis);
                record(p, bitmap, hp::occupancy_search(x, y, z, kz, R, axis, columns));
            }
            __syncthreads();
        }
        for (int w = tid; w < words; w += kThreads) {
            unsigned bits = bitmap[w];
            while (bits) {
                const int b = __builtin_ctz(bits);
                bits &= bits - 1;
                atomicAdd(&p.clouds_hit[w * 32 + b], 1);
            }
        }
        __syncthreads();          // the bitmap is read out before the next cloud clears it
    }
    if (bad) *p.nonfinite = 1;
}

inline size_t lds_bytes(int R, int cells) {
    return (size_t)R * 8 + (size_t)R * R * 4 + (size_t)((cells + 31) / 32) * 4 + kChunk * 4 + 16;
}

}  // namespace

// ================================================================================================
// C ABI
// ================================================================================================

HP_API int hp_occupancy_grid(int S, int n, const float* clouds, int R, const float* axis, const unsigned* columns,
                             int cells, int* counters, int* clouds_hit, int* nonfinite, hipStream_t stream) {
    HP_CHECK_ARG(S >= 1 && n >= 1 && R >= 2 && R <= hp::kOccupancyMaxR);
    HP_CHECK_ARG((long)S * n < (1L << 31));
    HP_CHECK_ARG(cells >= 1 && cells <= R * R * R);
    HP_CHECK_ARG(clouds && axis && columns && counters && clouds_hit && nonfinite);
    hipError_t e = hipMemsetAsync(counters, 0, (size_t)cells * sizeof(int), stream);
    if (e == hipSuccess) e = hipMemsetAsync(clouds_hit, 0, (size_t)cells * sizeof(int), stream);
    if (e == hipSuccess) e = hipMemsetAsync(nonfinite, 0, sizeof(int), stream);
    if (e != hipSuccess) return (int)e;
    const OccArgs a{clouds, axis, columns, counters, clouds_hit, nonfinite, S, n, R, cells};
    // at most 56 KB at R = 64 (512 B axis, 16 KB columns, 32 KB bitmap, 4 KB queue): under the 64 KB a launch may ask for
    hipLaunchKernelGGL(occupancy_kernel, dim3((unsigned)std::min(S, kMaxBlocks)), dim3(kThreads), lds_bytes(R, cells), stream, a);
    HP_RETURN_LAST_ERROR();
}

// The same cell decision on the host, point by point (hp_occupancy.h compiles for both sides): what the CPU suite holds
// against recorded results without a GPU.  cell_out[i] = kept index of point i's nearest kept centre, -1 for a non-finite point.
HP_API int hp_occupancy_cells_host(long count, const float* points, int R, const float* axis, const unsigned* columns,
                                   int* cell_out) {
    HP_CHECK_ARG(count >= 0 && R >= 2 && R <= hp::kOccupancyMaxR);
    if (count == 0) return 0;
    HP_CHECK_ARG(points && axis && columns && cell_out);
    double ax[hp::kOccupancyMaxR];
    for (int i = 0; i < R; ++i) ax[i] = (double)axis[i];
    for (long i = 0; i < count; ++i) {
        const float x = points[i * 3], y = points[i * 3 + 1], z = points[i * 3 + 2];
        cell_out[i] = -1;
        if (!(std::isfinite(x) && std::isfinite(y) && std::isfinite(z))) continue;
        const int ki = hp::occupancy_axis_nearest(x, R, ax), kj = hp::occupancy_axis_nearest(y, R, ax),
                  kz = hp::occupancy_axis_nearest(z, R, ax);
        const int cell = hp::occupancy_kept_index(columns[ki * R + kj], kz);
        cell_out[i] = cell >= 0 ? cell : hp::occupancy_search(x, y, z, kz, R, ax, columns);
    }
    return 0;
}
