// Voxel-grid thinning of ragged scans: one representative row per occupied cell, so that a sensor scan of
// hundreds of thousands of rows fits the capped neighbour and cluster kernels (knn.hip, clusters.hip) at an even density.
//
// The law, per scan (include/hyperpocket_hip.h and tests/voxel_law.py have it in full):
//   u = p - origin[s] (or p), q_c = floor(u_c / voxel[s]); the row is inside iff -2^20 <= q_c < 2^20 on the three axes;
//   key = ((qx+2^20) << 42) | ((qy+2^20) << 21) | (qz+2^20); m_c = (float(q_c) + 0.5) * voxel[s], d2 = ((dx*dx + dy*dy) + dz*dz)
//   with d = u - m; rank = (bits(d2) << 32 | row) under keep_mode 0, the row under keep_mode 1.  Per cell: label = its smallest
//   row, size = its rows, keep = the row of the smallest rank.
//
// A hash table in the caller's workspace: scan s owns the slots [spr * offsets[s], spr * offsets[s+1]), so scans cannot meet
// and the key needs no scan number.  A slot is (key, best rank) 64-bit and (first row, count) 32-bit, in four arrays: 24 bytes,
// and the three atomics of a crowded cell go to three cache lines (32-byte slots were measured: DESIGN.md 3n).
//   clear    every slot to (all ones, all ones, INT_MAX, 0); kept and beyond to 0.
//   insert   per row: hash the key, probe linearly inside the scan's region (wrapping), claim an empty slot by a 64-bit
//            compare-and-swap on the key word, then min the rank, min the row, add the count.  Before that the lanes of a wave
//            that share a cell fold into one of them — neighbouring rows of a sensor sweep do —, up to 8 cells a wave.
//   resolve  per row: find the slot again (plain loads: the launch boundary made the table visible), write label, size and
//            keep; kept and beyond are summed per wave and added once per (wave, scan).
// Integer atomics only and no flag, fence or float atomic: min and add commute, and which row claimed a slot, or which slot a
// cell landed in, never reaches an output.  A scan has at most as many cells as rows, so with spr >= 1 a probe ends within
// one lap of its region; the loops are bounded by the region's size all the same.
#include "hp_common.h"

namespace {

using hp::finite_bits, hp::kInfBits, hp::scan_of;
constexpr int kScanMaxPoints = 1 << 22;    // = HP_SCAN_MAX_POINTS (include/hyperpocket_hip.h)
constexpr long long kMaxRows = 1ll << 28;  // T at most: 4 slots per row are 2^30 slots, 24 GiB of table
constexpr int kGridHalf = 1 << 20;         // = HP_VOXEL_GRID_HALF: 21 bits per axis
constexpr int kThreads = 256;              // 4 waves per workgroup
constexpr int kRowsPerLane = 4;            // a workgroup covers kThreads * kRowsPerLane consecutive rows of the ragged set
constexpr int kChunk = kThreads * kRowsPerLane;
constexpr int kGrid = 2048;                // workgroups: 8 per compute unit, each strides over the chunks
constexpr unsigned long long kEmpty = ~0ull;

constexpr size_t kSlotBytes = 2 * sizeof(unsigned long long) + 2 * sizeof(int);

struct Table {
    unsigned long long* key;   // the cell, or all ones: empty
    unsigned long long* best;  // the smallest rank of the cell's rows
    int* first;                // the smallest row
    int* count;                // the rows
};

inline Table table_of(void* ws, size_t slots) {
    Table t;
    t.key = static_cast<unsigned long long*>(ws);
    t.best = t.key + slots;
    t.first = reinterpret_cast<int*>(t.best + slots);
    t.count = t.first + slots;
    return t;
}

// What a scan needs to take part: its rows inside [0, T), a length the law allows and a usable cell edge.
__device__ __forceinline__ bool scan_ok(long long lo, long long hi, long long T, float v) {
    return lo >= 0 && hi > lo && hi <= T && hi - lo <= kScanMaxPoints && finite_bits(v) && v > 0.f;
}

__device__ __forceinline__ unsigned long long mix(unsigned long long k) {     // the 64-bit finaliser of MurmurHash3
    k ^= k >> 33;
    k *= 0xFF51AFD7ED558CCDull;
    k ^= k >> 33;
    k *= 0xC4CEB9FE1A85EC53ull;
    k ^= k >> 33;
    return k;
}

// The slot a key's probe starts at, within a region of R slots.
__device__ __forceinline__ unsigned home_of(unsigned long long key, unsigned R) { return __umulhi((unsigned)(mix(key) >> 32), R); }

enum { kAbsent = 0, kBeyond = 1, kInside = 2 };

struct Origin {
    bool given;
    float x, y, z;
};

// The cell and the rank of row g (row `row` of its scan) under the law; kAbsent, kBeyond or kInside.
__device__ __forceinline__ int cell_of(const float* __restrict__ points, long long g, int row, float v, Origin o, int keep_mode,
                                       unsigned long long& key, unsigned long long& rank) {
#pragma clang fp contract(off)
    float ux = points[g * 3], uy = points[g * 3 + 1], uz = points[g * 3 + 2];
    if (!(finite_bits(ux) && finite_bits(uy) && finite_bits(uz))) return kAbsent;
    if (o.given) {
        ux = __fsub_rn(ux, o.x);
        uy = __fsub_rn(uy, o.y);
        uz = __fsub_rn(uz, o.z);
    }
    const float qx = floorf(__fdiv_rn(ux, v)), qy = floorf(__fdiv_rn(uy, v)), qz = floorf(__fdiv_rn(uz, v));
    const float half = (float)kGridHalf;
    // a NaN or an infinite quotient fails a comparison
    if (!(qx >= -half && qx < half && qy >= -half && qy < half && qz >= -half && qz < half)) return kBeyond;
    key = ((unsigned long long)((int)qx + kGridHalf) << 42) | ((unsigned long long)((int)qy + kGridHalf) << 21) |
          (unsigned long long)((int)qz + kGridHalf);
    rank = (unsigned long long)row;
    if (keep_mode == 0) {
        // float(q) + 0.5 is exact (21 bits and one more); q as a float already is float(q), and -0 + 0.5 = 0.5
        const float dx = __fsub_rn(ux, __fmul_rn(__fadd_rn(qx, 0.5f), v));
        const float dy = __fsub_rn(uy, __fmul_rn(__fadd_rn(qy, 0.5f), v));
        const float dz = __fsub_rn(uz, __fmul_rn(__fadd_rn(qz, 0.5f), v));
        const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
        rank |= (unsigned long long)(unsigned)__float_as_int(d2) << 32;      // d2 >= +0 or +inf: its bits order as integers
    }
    return kInside;
}

__device__ __forceinline__ Origin origin_of(const float* __restrict__ origin, int s) {
    Origin o = {origin != nullptr, 0.f, 0.f, 0.f};
    if (o.given) {
        o.x = origin[s * 3];
        o.y = origin[s * 3 + 1];
        o.z = origin[s * 3 + 2];
    }
    return o;
}

__global__ __launch_bounds__(kThreads) void voxel_clear_kernel(int S, size_t slots, Table tab, int* __restrict__ kept,
                                                               int* __restrict__ beyond) {
    const size_t tid = (size_t)blockIdx.x * kThreads + threadIdx.x, step = (size_t)gridDim.x * kThreads;
    for (size_t i = tid; i < slots; i += step) {
        tab.key[i] = kEmpty;
        tab.best[i] = kEmpty;
        tab.first[i] = 0x7FFFFFFF;
        tab.count[i] = 0;
    }
    for (size_t s = tid; s < (size_t)S; s += step) kept[s] = beyond[s] = 0;
}

// (key, rank, row, count) into the region [base, base + R): the cell's slot takes the min of the ranks and of the rows and
// the sum of the counts.
__device__ __forceinline__ void insert(Table tab, size_t base, unsigned R, unsigned long long key, unsigned long long rank,
                                       int row, int count) {
    unsigned idx = home_of(key, R);
    for (unsigned step = 0; step < R; ++step) {
        unsigned long long* kp = tab.key + base + idx;
        // a key word changes once, from empty to a key: whatever a load sees that is not empty is final
        unsigned long long cur = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kEmpty) {
            cur = atomicCAS(kp, kEmpty, key);
            if (cur == kEmpty) cur = key;
        }
        if (cur == key) {
            atomicMin(tab.best + base + idx, rank);
            atomicMin(tab.first + base + idx, row);
            atomicAdd(tab.count + base + idx, count);
            return;
        }
        idx = idx + 1 == R ? 0u : idx + 1;
    }
}

constexpr int kCombineRounds = 8;          // cells a wave folds before its lanes go to memory
constexpr int kCombineMinRuns = 16;        // lanes that sit in the cell of the lane before them, at which folding starts

// The lanes of a wave that share a cell elect a leader, which carries their smallest rank, their smallest row and their number
// to the table in one set of atomics; a wave folds only when its rows come in runs, and lanes it does not reach go alone.
__global__ __launch_bounds__(kThreads) void voxel_insert_kernel(int S, long long T, const float* __restrict__ points,
                                                                const long long* __restrict__ offsets,
                                                                const float* __restrict__ voxel, const float* __restrict__ origin,
                                                                int keep_mode, int spr, Table tab) {
    const int tid = threadIdx.x, lane = tid & (HP_WAVE - 1);
    for (long long row0 = (long long)blockIdx.x * kChunk; row0 < T; row0 += (long long)gridDim.x * kChunk) {
        const long long end = row0 + kChunk < T ? row0 + kChunk : T;
        // every value that steers these loops is uniform over the workgroup
        for (int s = scan_of(offsets, S, row0); s < S && offsets[s] < end; ++s) {
            const long long lo = offsets[s], hi = offsets[s + 1];
            const float v = voxel[s];
            if (!scan_ok(lo, hi, T, v)) continue;
            const long long b0 = lo > row0 ? lo : row0, b1 = hi < end ? hi : end;
            const Origin o = origin_of(origin, s);
            const size_t base = (size_t)spr * (size_t)lo;
            const unsigned R = (unsigned)spr * (unsigned)(hi - lo);
            for (long long g0 = b0; g0 < b1; g0 += kThreads) {             // every lane of a wave takes every step
                const long long g = g0 + tid;
                unsigned long long key = kEmpty, rank = kEmpty;
                int first = (int)(g - lo), count = 1;
                const bool in = g < b1 && cell_of(points, g, first, v, o, keep_mode, key, rank) == kInside;
                bool lead = in;                                            // a lane no round reaches goes alone
                const unsigned long long before = __shfl_up(key, 1, HP_WAVE);
                unsigned long long todo = __ballot(in);
                if (__popcll(__ballot(in && lane > 0 && key == before)) >= kCombineMinRuns) {
                    for (int round = 0; round < kCombineRounds && todo; ++round) {
                        const int leader = __ffsll((long long)todo) - 1;
                        const unsigned long long k = __shfl(key, leader, HP_WAVE);
                        const bool same = in && key == k;
                        const unsigned long long members = __ballot(same);
                        unsigned long long r = same ? rank : kEmpty;
                        int f = same ? first : 0x7FFFFFFF;
#pragma unroll
                        for (int w = 32; w > 0; w >>= 1) {
                            const unsigned long long r2 = __shfl_xor(r, w, HP_WAVE);
                            const int f2 = __shfl_xor(f, w, HP_WAVE);
                            r = r2 < r ? r2 : r;
                            f = f2 < f ? f2 : f;
                        }
                        if (same) {
                            lead = lane == leader;
                            rank = r;
                            first = f;
                            count = __popcll(members);
                        }
                        todo &= ~members;
                    }
                }
                if (lead) insert(tab, base, R, key, rank, first, count);
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void voxel_resolve_kernel(int S, long long T, const float* __restrict__ points,
                                                                 const long long* __restrict__ offsets,
                                                                 const float* __restrict__ voxel, const float* __restrict__ origin,
                                                                 int keep_mode, int spr, Table tab, int* __restrict__ label,
                                                                 int* __restrict__ size, unsigned char* __restrict__ keep,
                                                                 int* __restrict__ kept, int* __restrict__ beyond) {
    const int tid = threadIdx.x;
    for (long long row0 = (long long)blockIdx.x * kChunk; row0 < T; row0 += (long long)gridDim.x * kChunk) {
        const long long end = row0 + kChunk < T ? row0 + kChunk : T;
        for (int s = scan_of(offsets, S, row0); s < S && offsets[s] < end; ++s) {
            const long long lo = offsets[s], hi = offsets[s + 1];
            const long long b0 = lo > row0 ? lo : row0, b1 = hi < end ? hi : end;      // inside the chunk, whatever the offsets
            const float v = voxel[s];
            if (!scan_ok(lo, hi, T, v)) {                  // the empty result
                for (long long g = b0 + tid; g < b1; g += kThreads) {
                    label[g] = -1;
                    size[g] = 0;
                    keep[g] = 0;
                }
                continue;
            }
            const Origin o = origin_of(origin, s);
            const size_t base = (size_t)spr * (size_t)lo;
            const unsigned R = (unsigned)spr * (unsigned)(hi - lo);
            int nk = 0, nb = 0;
            for (long long g = b0 + tid; g < b1; g += kThreads) {
                unsigned long long key = 0, rank = 0;
                const int what = cell_of(points, g, (int)(g - lo), v, o, keep_mode, key, rank);
                int lab = -1, sz = 0, kp = 0;
                if (what == kInside) {
                    unsigned idx = home_of(key, R);
                    for (unsigned step = 0; step < R; ++step) {
                        if (tab.key[base + idx] == key) {
                            lab = tab.first[base + idx];
                            sz = tab.count[base + idx];
                            kp = tab.best[base + idx] == rank;
                            break;
                        }
                        idx = idx + 1 == R ? 0u : idx + 1;
                    }
                }
                label[g] = lab;
                size[g] = sz;
                keep[g] = (unsigned char)kp;
                nk += kp;
                nb += what == kBeyond;
            }
#pragma unroll
            for (int w = 32; w > 0; w >>= 1) {
                nk += __shfl_down(nk, w, HP_WAVE);
                nb += __shfl_down(nb, w, HP_WAVE);
            }
            if ((tid & (HP_WAVE - 1)) == 0) {
                if (nk) atomicAdd(&kept[s], nk);
                if (nb) atomicAdd(&beyond[s], nb);
            }
        }
    }
}

inline bool spr_ok(int spr) { return spr == 1 || spr == 2 || spr == 4; }

}  // namespace

// The geometry of hp_scan_voxels: threads per workgroup and rows per lane (a workgroup covers threads * rows_per_lane
// consecutive rows of the ragged set).  Host only.
HP_API int hp_scan_voxels_plan(int* threads, int* rows_per_lane) {
    HP_CHECK_ARG(threads && rows_per_lane);
    *threads = kThreads;
    *rows_per_lane = kRowsPerLane;
    return 0;
}

// Bytes of hp_scan_voxels' workspace: slots_per_row * T slots of 24 bytes in four arrays.  Host only.
HP_API long hp_scan_voxels_workspace_bytes(long long T, int slots_per_row) {
    if (T < 0 || T > kMaxRows || !spr_ok(slots_per_row)) return -1;
    return (long)(((size_t)T * slots_per_row * kSlotBytes + 15) / 16 * 16 + 16);
}

// One representative row per occupied cell of each of S ragged scans; the law is in include/hyperpocket_hip.h.
HP_API int hp_scan_voxels(int S, long long T, const float* points, const long long* offsets, const float* voxel,
                          const float* origin, int keep_mode, int slots_per_row, int* label, int* size, unsigned char* keep,
                          int* kept, int* beyond, void* ws, hipStream_t stream) {
    HP_CHECK_ARG(S >= 1 && T >= 0 && T <= kMaxRows && points && offsets && voxel && label && size && keep && kept && beyond && ws);
    HP_CHECK_ARG((keep_mode == 0 || keep_mode == 1) && spr_ok(slots_per_row));
    const size_t slots = (size_t)T * slots_per_row;
    const Table tab = table_of(ws, slots);
    const size_t cells = slots > (size_t)S ? slots : (size_t)S;
    const int clear_grid = (int)std::min<size_t>((cells + kChunk - 1) / kChunk, (size_t)kGrid * 4);
    hipLaunchKernelGGL(voxel_clear_kernel, dim3(clear_grid), dim3(kThreads), 0, stream, S, slots, tab, kept, beyond);
    if (T > 0) {
        const int grid = (int)std::min<long long>((T + kChunk - 1) / kChunk, kGrid);
        hipLaunchKernelGGL(voxel_insert_kernel, dim3(grid), dim3(kThreads), 0, stream, S, T, points, offsets, voxel, origin,
                           keep_mode, slots_per_row, tab);
        hipLaunchKernelGGL(voxel_resolve_kernel, dim3(grid), dim3(kThreads), 0, stream, S, T, points, offsets, voxel, origin,
                           keep_mode, slots_per_row, tab, label, size, keep, kept, beyond);
    }
    HP_RETURN_LAST_ERROR();
}
