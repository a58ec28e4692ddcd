// The match sweep of the rigid registration (ICP) steps over ragged sets, stated once: csrc/align.hip (point to
// point) and csrc/align_plane.hip (point to plane) are this sweep with an epilogue of their own, so that the match of the one is
// the match of the other bit for bit.
//
// The shared law, per job (set s, hypothesis h) (include/hyperpocket_hip.h and tests/align_law.py have it in full):
//   p' = [R | t] p, each coordinate ((r0*x + r1*y) + r2*z) + t; a row whose input or p' is not finite is absent for the job
//   best = the finite target row j of set s with the smallest d2 = ((dx*dx + dy*dy) + dz*dz), d = q - p', ties to the lower j
//   a correspondence iff some d2 is below +inf and d2 <= max_dist^2; u, v = trunc(ldexp(p' - anchor, 19 - shift)) and the same
//   of q; clipped (counted, not summed) when a scaled component is not finite or reaches 2^20
// Every float operation is one fp32 rounding in the association written, no contraction.
//
//   fill     only when the caller asks for index / dist2: -1 and +inf over (H,T), so that rows of no valid set are written too.
//   sweep    the hot path.  A work item is (chunk of 512 consecutive source rows of the ragged set, group of G hypotheses);
//            workgroups of 256 lanes stride over the items.  A chunk walks the sets its rows belong to (found by bisection over
//            the offsets; set boundaries fall anywhere in a chunk or a wave).  A lane keeps 2 rows in registers, each moved
//            under the G transforms of the group (read at uniform addresses), and their 2 * G running (d2, j).  The set's
//            targets pass through an LDS tile of 256 float4 that every lane reads at the same address — a broadcast, no bank
//            conflict —, an absent target as NaNs: its d2 is NaN and `d2 < best` fails, as it does for +inf and for an absent
//            source row (its p' is NaN).  Targets arrive in ascending order, so the strict compare keeps the lower j of equals.
//            One LDS read serves 2 * G (row, hypothesis) pairs, eleven VALU operations each.
//            After the tiles, in registers and per hypothesis of the group, the step's epilogue is called; it asks once for
//            each of the lane's 2 rows — index / dist2 are written, then the gate, the matched target row read back once, the
//            quantisation and the clip test give the row as a Pair —, sums what its solve needs over the wave and adds it to
//            the job's moments.  Integer adds only: no order of evaluation can change a bit.  A last group may be partial.
#pragma once
#include "hp_common.h"

namespace hp_align {

constexpr int kMaxPoints = 65536;          // = HP_ALIGN_MAX_POINTS (include/hyperpocket_hip.h): keeps the epilogues' 64-bit sums in range
constexpr int kMaxHyp = 64;                // = HP_ALIGN_MAX_HYPOTHESES
constexpr int kThreads = 256;              // 4 waves per workgroup
constexpr int kRows = 2;                   // source rows a lane keeps in registers (4 at H == 1 was measured: no gain)
constexpr int kChunk = kThreads * kRows;
constexpr int kGroup = 4;                  // hypotheses per work item of the grouped sweep
constexpr int kTile = 256;                 // targets per LDS tile (4 KiB): a tile costs a workgroup ~10^5 cycles, two barriers
constexpr int kMaxGrid = 1 << 16;          // workgroups of a launch; they stride over the items

// What the sweep hands an epilogue for one of the lane's rows under one hypothesis.
enum { kNoPair = 0, kUsed = 1, kClipped = 2 };
struct Pair {
    int state;                             // kUsed: u, v and at hold; kClipped: a correspondence outside the frame; kNoPair: none
    int u[3], v[3];                        // the moved row and its matched target row as integers of the frame, each below 2^20
    int at;                                // the matched row's number within the target set
};

// The set of row: the last s with offsets[s] <= row (0 when there is none).
__device__ __forceinline__ int set_of(const long long* __restrict__ offsets, int S, long long row) {
    int s = 0;
    for (int hi = S; hi - s > 1;) {
        const int mid = (s + hi) >> 1;
        if (offsets[mid] <= row) s = mid;
        else hi = mid;
    }
    return s;
}

// A set takes part iff 0 <= lo < hi <= rows and it holds at most kMaxPoints rows.
__device__ __forceinline__ bool set_ok(long long lo, long long hi, long long rows) {
    return lo >= 0 && lo < hi && hi <= rows && hi - lo <= kMaxPoints;
}

// The body of a step's fill kernel (each step keeps a __global__ of its own name around it).
__device__ __forceinline__ void fill(long long total, int* __restrict__ index, float* __restrict__ dist2) {
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
        index[i] = -1;
        dist2[i] = __int_as_float((int)hp::kInfBits);
    }
}

// The body of a sweep kernel: epilogue(s, h, pair_of) is called by every lane of the workgroup, once per set of the chunk and
// hypothesis h < H of the group.  pair_of(r) writes index / dist2 of the lane's row r < kRows and returns its Pair: an epilogue
// calls it once for every r, in a loop of its own, so that a row's sums follow its quantisation as they did in one kernel.
template <int G, class Epilogue>
__device__ __forceinline__ void align_sweep(int S, int H, long long T, long long U, const float* __restrict__ points,
                                            const long long* __restrict__ offsets, const float* __restrict__ tpoints,
                                            const long long* __restrict__ toffsets, const float* __restrict__ transforms, float g2,
                                            const float* __restrict__ anchor, const int* __restrict__ shift,
                                            int* __restrict__ index, float* __restrict__ dist2, Epilogue epilogue) {
#pragma clang fp contract(off)
    __shared__ float4 tile[kTile];
    const int tid = threadIdx.x;
    const int groups = (H + G - 1) / G;
    const long long chunks = (T + kChunk - 1) / kChunk, items = chunks * groups;
    const float nan = __int_as_float(hp::kNanBits), inf = __int_as_float((int)hp::kInfBits);
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const long long row0 = (item / groups) * kChunk;
        const int h0 = (int)(item % groups) * G;
        float px[kRows], py[kRows], pz[kRows];
        bool have[kRows];
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const long long g = row0 + r * kThreads + tid;
            have[r] = g < T;
            px[r] = py[r] = pz[r] = nan;
            if (have[r]) {
                px[r] = points[g * 3];
                py[r] = points[g * 3 + 1];
                pz[r] = points[g * 3 + 2];
            }
            have[r] = have[r] && hp::finite_bits(px[r]) && hp::finite_bits(py[r]) && hp::finite_bits(pz[r]);
        }
        const long long last = (row0 + kChunk < T ? row0 + kChunk : T) - 1;
        // every value that steers these loops is uniform over the workgroup
        for (int s = set_of(offsets, S, row0); s < S && offsets[s] <= last; ++s) {
            const long long lo = offsets[s], hi = offsets[s + 1], tlo = toffsets[s], thi = toffsets[s + 1];
            if (!set_ok(lo, hi, T) || !set_ok(tlo, thi, U)) continue;          // the empty result: the moments stay 0
            const int m = (int)(thi - tlo);
            const float* Q = tpoints + tlo * 3;
            bool mine[kRows];
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                const long long g = row0 + r * kThreads + tid;
                mine[r] = g >= lo && g < hi;
            }
            float mx[kRows][G], my[kRows][G], mz[kRows][G], best[kRows][G];
            int at[kRows][G];
#pragma unroll
            for (int k = 0; k < G; ++k) {
                const int h = h0 + k < H ? h0 + k : H - 1;                      // a partial group repeats its last transform
                const float* M = transforms + ((size_t)s * H + h) * 12;
#pragma unroll
                for (int r = 0; r < kRows; ++r) {
                    float x = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(M[0], px[r]), __fmul_rn(M[1], py[r])), __fmul_rn(M[2], pz[r])), M[3]);
                    float y = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(M[4], px[r]), __fmul_rn(M[5], py[r])), __fmul_rn(M[6], pz[r])), M[7]);
                    float z = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(M[8], px[r]), __fmul_rn(M[9], py[r])), __fmul_rn(M[10], pz[r])), M[11]);
                    if (!(mine[r] && have[r] && hp::finite_bits(x) && hp::finite_bits(y) && hp::finite_bits(z))) x = y = z = nan;   // absent
                    mx[r][k] = x;
                    my[r][k] = y;
                    mz[r][k] = z;
                    best[r][k] = inf;
                    at[r][k] = -1;
                }
            }
            for (int t0 = 0; t0 < m; t0 += kTile) {
                const int cnt = m - t0 < kTile ? m - t0 : kTile;
                __syncthreads();                                               // the tile before this one has been read
                for (int c = tid; c < cnt; c += kThreads) {
                    float x = Q[(long)(t0 + c) * 3], y = Q[(long)(t0 + c) * 3 + 1], z = Q[(long)(t0 + c) * 3 + 2];
                    if (!(hp::finite_bits(x) && hp::finite_bits(y) && hp::finite_bits(z))) x = y = z = nan;
                    tile[c] = make_float4(x, y, z, 0.f);
                }
                __syncthreads();
#pragma unroll 4
                for (int c = 0; c < cnt; ++c) {
                    const float4 q = tile[c];
                    const int j = t0 + c;
#pragma unroll
                    for (int r = 0; r < kRows; ++r) {
#pragma unroll
                        for (int k = 0; k < G; ++k) {
                            const float dx = __fsub_rn(q.x, mx[r][k]), dy = __fsub_rn(q.y, my[r][k]), dz = __fsub_rn(q.z, mz[r][k]);
                            const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
                            const bool closer = d2 < best[r][k];               // false for a NaN and for +inf
                            best[r][k] = closer ? d2 : best[r][k];
                            at[r][k] = closer ? j : at[r][k];
                        }
                    }
                }
            }
            const float ax = anchor[s * 3], ay = anchor[s * 3 + 1], az = anchor[s * 3 + 2];
            const int up = 19 - shift[s];
#pragma unroll
            for (int k = 0; k < G; ++k) {
                if (h0 + k >= H) continue;                                     // uniform
                // by reference: captured by value, the tile loop above compiles to other, slower code at G == 1
                epilogue(s, h0 + k, [&](int r) {
                    Pair pair = {kNoPair, {0, 0, 0}, {0, 0, 0}, at[r][k]};
                    const long long g = row0 + r * kThreads + tid;
                    if (mine[r] && index) {
                        index[(size_t)(h0 + k) * T + g] = at[r][k];
                        dist2[(size_t)(h0 + k) * T + g] = best[r][k];
                    }
                    if (at[r][k] < 0 || !(best[r][k] <= g2)) return pair;      // at >= 0 only for a present row of this set
                    const float* q = Q + (long)at[r][k] * 3;
                    const float su[3] = {ldexpf(__fsub_rn(mx[r][k], ax), up), ldexpf(__fsub_rn(my[r][k], ay), up),
                                         ldexpf(__fsub_rn(mz[r][k], az), up)};
                    const float sv[3] = {ldexpf(__fsub_rn(q[0], ax), up), ldexpf(__fsub_rn(q[1], ay), up),
                                         ldexpf(__fsub_rn(q[2], az), up)};
                    bool inside = true;
#pragma unroll
                    for (int a = 0; a < 3; ++a) inside = inside && fabsf(su[a]) < 1048576.f && fabsf(sv[a]) < 1048576.f;   // NaN, inf: false
                    pair.state = inside ? kUsed : kClipped;
                    if (!inside) return pair;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        pair.u[a] = (int)su[a];                                // the cast truncates towards zero
                        pair.v[a] = (int)sv[a];
                    }
                    return pair;
                });
            }
        }
    }
}

// The body of a step's entry point: the argument checks, the zeroed moments (`width` per job), the fill when index / dist2 are
// asked for, and sweep(g2), which launches the step's sweep kernel.  `pointers`: none of the step's required pointers is null.
template <class Sweep>
inline int align_step(void (*fill_kernel)(long long, int*, float*), int S, int H, long long T, long long U, bool pointers,
                      float max_dist, long long* moments, int width, int* index, float* dist2, hipStream_t stream, Sweep sweep) {
    HP_CHECK_ARG(S >= 1 && H >= 1 && H <= kMaxHyp && T >= 0 && U >= 0 && T <= (1ll << 40) && U <= (1ll << 40));
    HP_CHECK_ARG(pointers);
    HP_CHECK_ARG((index == nullptr) == (dist2 == nullptr));
    HP_CHECK_ARG(max_dist >= 0.f);                                             // refuses a NaN too; +inf is no gate
    const hipError_t err = hipMemsetAsync(moments, 0, (size_t)S * H * width * sizeof(long long), stream);
    if (err != hipSuccess) return (int)err;
    if (T == 0) return 0;
    if (index) {
        const long long total = (long long)H * T, blocks = (total + kThreads * 8 - 1) / (kThreads * 8);
        hipLaunchKernelGGL(fill_kernel, dim3((unsigned)std::min<long long>(blocks, kMaxGrid)), dim3(kThreads), 0, stream, total, index,
                           dist2);
    }
    sweep(max_dist * max_dist);
    HP_RETURN_LAST_ERROR();
}

// The grid of a sweep at G hypotheses per work item.
inline dim3 sweep_grid(int H, long long T, int G) {
    const long long items = (T + kChunk - 1) / kChunk * ((H + G - 1) / G);
    return dim3((unsigned)std::min<long long>(items, kMaxGrid));
}

}  // namespace hp_align
