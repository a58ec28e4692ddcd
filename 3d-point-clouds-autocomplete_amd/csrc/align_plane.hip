// One step of point-to-plane rigid registration (ICP) over ragged sets: every source row, moved by each of H
// transforms, finds its nearest target row, and the matches leave as the exact integer 6x6 normal system of the linearised
// point-to-plane error (ops.rigid_from_plane_moments on the host) — the error a depth sensor's captures call for: two captures
// of one surface never sample the same points, and only the distance along the target's normal says how far apart they are.
//
// The law, per job (set s, hypothesis h) (include/hyperpocket_hip.h and tests/align_plane_law.py have it in full).  The
// transform, absence, the match, the gate and the quantisation are those of csrc/align.hip, restated here:
//   p' = [R | t] p, each coordinate ((r0*x + r1*y) + r2*z) + t; a row whose input or p' is not finite is absent for the job
//   best = the finite target row j of set s with the smallest d2 = ((dx*dx + dy*dy) + dz*dz), d = q - p', ties to the lower j
//   a correspondence iff some d2 is below +inf and d2 <= max_dist^2; u, v = trunc(ldexp(p' - anchor, 19 - shift)) and the same
//   of q; clipped (counted, not summed) when a scaled component is not finite or reaches 2^20
// and then, with n = tnormals[j] of the matched row:
//   w = trunc(ldexp(n, 9)); without normal (counted, not summed) when a scaled component is not finite or reaches 2^10, when
//   w.w == 0 or when w.w > 2^18 + 2^11;  c = u x w, a = (c, w), b = -(u - v).w: |c_i| < 2^30, |b| < 2^31, both held in 32 bits
//   28 terms: a_i a_j (i <= j, row-major), a_i b, b b, each below 2^62; a term leaves as hi = term >> 31 and lo = term & (2^31 - 1)
//   moments (S,H,60) = [used, clipped, without normal, 0, then (sum hi, sum lo) of the 28 terms]
// Every float operation is one fp32 rounding in the association written, no contraction.
//
//   fill     only when the caller asks for index / dist2: -1 and +inf over (H,T), so that rows of no valid set are written too.
//   sweep    the hot path, the sweep of csrc/align.hip at one hypothesis per work item.  A work item is (chunk of 512 consecutive
//            source rows of the ragged set, hypothesis); workgroups of 256 lanes stride over the items.  A chunk walks the sets
//            its rows belong to (found by bisection over the offsets; set boundaries fall anywhere in a chunk or a wave).  A
//            lane keeps 2 rows in registers, moved under the job's transform (read at uniform addresses), and their running
//            (d2, j).  The set's targets pass through an LDS tile of 256 float4 that every lane reads at the same address — a
//            broadcast, no bank conflict —, an absent target as NaNs: its d2 is NaN and `d2 < best` fails, as it does for +inf
//            and for an absent source row (its p' is NaN).  Targets arrive in ascending order, so the strict compare keeps the
//            lower j of equals.
//   epilogue in registers: the gate, the matched target row and its normal read back once, the quantisation, and the seven
//            32-bit integers (a, b) of each of the lane's two rows — zeros for a row that is not used, so that what follows has
//            no branch.  The 56 sums never exist side by side: one term at a time is formed from those integers (a 32 x 32 -> 64
//            multiply), split, summed over the lane's rows, reduced over the wave by shuffles, and the wave's lane 0 issues one
//            64-bit integer add per non-zero value.  The three counts travel as one packed 64-bit word (21 bits each; a wave
//            holds 128 rows).  Integer adds only: no order of evaluation can change a bit.
// The yaw search stays with the point-to-point step: H > 1 is served, one hypothesis per work item, but not grouped.
#include "hp_common.h"

namespace {

constexpr int kPlaneMaxPoints = 65536;     // = HP_ALIGN_MAX_POINTS (include/hyperpocket_hip.h): keeps the hi and lo sums below 2^48
constexpr int kPlaneMaxHyp = 64;           // = HP_ALIGN_MAX_HYPOTHESES
constexpr int kThreads = 256;              // 4 waves per workgroup
constexpr int kRows = 2;                   // source rows a lane keeps in registers
constexpr int kChunk = kThreads * kRows;
constexpr int kTile = 256;                 // targets per LDS tile (4 KiB)
constexpr int kMaxGrid = 1 << 16;          // workgroups of a launch; they stride over the items
constexpr int kMoments = 60;
constexpr int kNormalBits = 9;
constexpr int kNormalMax = (1 << 18) + (1 << 11);   // w.w of a unit normal is at most 2^18
constexpr unsigned kInfBits = 0x7F800000u;
constexpr int kNanBits = 0x7FC00000;

__device__ __forceinline__ bool finite_bits(float v) { return ((unsigned)__float_as_int(v) & kInfBits) != kInfBits; }

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

// A set takes part iff 0 <= lo < hi <= rows and it holds at most kPlaneMaxPoints rows.
__device__ __forceinline__ bool set_ok(long long lo, long long hi, long long rows) {
    return lo >= 0 && lo < hi && hi <= rows && hi - lo <= kPlaneMaxPoints;
}

__device__ __forceinline__ long long wave_sum(long long w) {
#pragma unroll
    for (int o = HP_WAVE / 2; o > 0; o >>= 1) w += __shfl_down(w, o, HP_WAVE);
    return w;                                                                  // lane 0 holds the wave's sum
}

// The slot of the term a_i a_j, i <= j <= 6 with a_6 = b: the 21 entries of the 6x6 upper triangle row-major, then a_i b, then b b.
__device__ constexpr int slot_of(int i, int j) { return j < 6 ? i * 6 - i * (i - 1) / 2 + (j - i) : 21 + i; }

__global__ __launch_bounds__(kThreads) void align_plane_fill_kernel(long long total, int* __restrict__ index, float* __restrict__ dist2) {
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
        index[i] = -1;
        dist2[i] = __int_as_float((int)kInfBits);
    }
}

__global__ __launch_bounds__(kThreads) void align_plane_sweep_kernel(int S, int H, long long T, long long U,
                                                                     const float* __restrict__ points,
                                                                     const long long* __restrict__ offsets,
                                                                     const float* __restrict__ tpoints,
                                                                     const long long* __restrict__ toffsets,
                                                                     const float* __restrict__ tnormals,
                                                                     const float* __restrict__ transforms, float g2,
                                                                     const float* __restrict__ anchor, const int* __restrict__ shift,
                                                                     long long* __restrict__ moments, int* __restrict__ index,
                                                                     float* __restrict__ dist2) {
#pragma clang fp contract(off)
    __shared__ float4 tile[kTile];
    const int tid = threadIdx.x;
    const long long chunks = (T + kChunk - 1) / kChunk, items = chunks * H;
    const float nan = __int_as_float(kNanBits), inf = __int_as_float((int)kInfBits);
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const long long row0 = (item / H) * kChunk;
        const int h = (int)(item % H);
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
            have[r] = have[r] && finite_bits(px[r]) && finite_bits(py[r]) && finite_bits(pz[r]);
        }
        const long long last = (row0 + kChunk < T ? row0 + kChunk : T) - 1;
        // every value that steers these loops is uniform over the workgroup
        for (int s = set_of(offsets, S, row0); s < S && offsets[s] <= last; ++s) {
            const long long lo = offsets[s], hi = offsets[s + 1], tlo = toffsets[s], thi = toffsets[s + 1];
            if (!set_ok(lo, hi, T) || !set_ok(tlo, thi, U)) continue;          // the empty result: the moments stay 0
            const int m = (int)(thi - tlo);
            const float* Q = tpoints + tlo * 3;
            const float* N = tnormals + tlo * 3;
            const float* M = transforms + ((size_t)s * H + h) * 12;
            bool mine[kRows];
            float mx[kRows], my[kRows], mz[kRows], best[kRows];
            int at[kRows];
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                const long long g = row0 + r * kThreads + tid;
                mine[r] = g >= lo && g < hi;
                float x = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(M[0], px[r]), __fmul_rn(M[1], py[r])), __fmul_rn(M[2], pz[r])), M[3]);
                float y = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(M[4], px[r]), __fmul_rn(M[5], py[r])), __fmul_rn(M[6], pz[r])), M[7]);
                float z = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(M[8], px[r]), __fmul_rn(M[9], py[r])), __fmul_rn(M[10], pz[r])), M[11]);
                if (!(mine[r] && have[r] && finite_bits(x) && finite_bits(y) && finite_bits(z))) x = y = z = nan;   // absent
                mx[r] = x;
                my[r] = y;
                mz[r] = z;
                best[r] = inf;
                at[r] = -1;
            }
            for (int t0 = 0; t0 < m; t0 += kTile) {
                const int cnt = m - t0 < kTile ? m - t0 : kTile;
                __syncthreads();                                               // the tile before this one has been read
                for (int c = tid; c < cnt; c += kThreads) {
                    float x = Q[(long)(t0 + c) * 3], y = Q[(long)(t0 + c) * 3 + 1], z = Q[(long)(t0 + c) * 3 + 2];
                    if (!(finite_bits(x) && finite_bits(y) && finite_bits(z))) x = y = z = nan;
                    tile[c] = make_float4(x, y, z, 0.f);
                }
                __syncthreads();
#pragma unroll 4
                for (int c = 0; c < cnt; ++c) {
                    const float4 q = tile[c];
                    const int j = t0 + c;
#pragma unroll
                    for (int r = 0; r < kRows; ++r) {
                        const float dx = __fsub_rn(q.x, mx[r]), dy = __fsub_rn(q.y, my[r]), dz = __fsub_rn(q.z, mz[r]);
                        const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
                        const bool closer = d2 < best[r];                      // false for a NaN and for +inf
                        best[r] = closer ? d2 : best[r];
                        at[r] = closer ? j : at[r];
                    }
                }
            }
            const float ax = anchor[s * 3], ay = anchor[s * 3 + 1], az = anchor[s * 3 + 2];
            const int up = 19 - shift[s];
            int a[kRows][7];                                                   // (c, w, b) of the lane's rows; zeros where unused
            long long counts = 0;                                              // used | clipped << 21 | without normal << 42
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
#pragma unroll
                for (int i = 0; i < 7; ++i) a[r][i] = 0;
                const long long g = row0 + r * kThreads + tid;
                if (mine[r] && index) {
                    index[(size_t)h * T + g] = at[r];
                    dist2[(size_t)h * T + g] = best[r];
                }
                if (at[r] < 0 || !(best[r] <= g2)) continue;                   // at >= 0 only for a present row of this set
                const float* q = Q + (long)at[r] * 3;
                const float* n = N + (long)at[r] * 3;
                const float su[3] = {ldexpf(__fsub_rn(mx[r], ax), up), ldexpf(__fsub_rn(my[r], ay), up), ldexpf(__fsub_rn(mz[r], az), up)};
                const float sv[3] = {ldexpf(__fsub_rn(q[0], ax), up), ldexpf(__fsub_rn(q[1], ay), up), ldexpf(__fsub_rn(q[2], az), up)};
                const float sn[3] = {ldexpf(n[0], kNormalBits), ldexpf(n[1], kNormalBits), ldexpf(n[2], kNormalBits)};
                bool inside = true, small = true;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    inside = inside && fabsf(su[k]) < 1048576.f && fabsf(sv[k]) < 1048576.f;   // NaN, inf: false
                    small = small && fabsf(sn[k]) < 1024.f;
                }
                if (!inside) {
                    counts += 1ll << 21;
                    continue;
                }
                long long u[3], d[3], w[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    u[k] = (int)su[k];                                         // the cast truncates towards zero
                    d[k] = u[k] - (int)sv[k];
                    w[k] = small ? (int)sn[k] : 0;
                }
                const long long ww = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
                if (!small || ww == 0 || ww > kNormalMax) {
                    counts += 1ll << 42;
                    continue;
                }
                counts += 1;
                a[r][0] = (int)(u[1] * w[2] - u[2] * w[1]);                    // |c_i| < 2^30 and |b| < 2^31: see the law
                a[r][1] = (int)(u[2] * w[0] - u[0] * w[2]);
                a[r][2] = (int)(u[0] * w[1] - u[1] * w[0]);
                a[r][3] = (int)w[0];
                a[r][4] = (int)w[1];
                a[r][5] = (int)w[2];
                a[r][6] = (int)-(d[0] * w[0] + d[1] * w[1] + d[2] * w[2]);
            }
            if (!__any(counts != 0)) continue;                                 // the wave holds no correspondence of this job
            const bool lead = (tid & (HP_WAVE - 1)) == 0;
            unsigned long long* out = reinterpret_cast<unsigned long long*>(moments + ((size_t)s * H + h) * kMoments);
            counts = __shfl(wave_sum(counts), 0, HP_WAVE);                     // every lane holds the wave's three counts
            if (lead) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const unsigned long long c = ((unsigned long long)counts >> (21 * k)) & ((1u << 21) - 1);
                    if (c) atomicAdd(out + k, c);
                }
            }
            if ((counts & ((1 << 21) - 1)) == 0) continue;                     // none of them is used: every term is 0
#pragma unroll
            for (int i = 0; i < 7; ++i) {
#pragma unroll
                for (int j = i; j < 7; ++j) {
                    const int slot = i == 6 ? 27 : slot_of(i, j);
                    long long th = 0, tl = 0;
#pragma unroll
                    for (int r = 0; r < kRows; ++r) {
                        const long long term = (long long)a[r][i] * a[r][j];
                        th += term >> 31;                                      // arithmetic: hi * 2^31 + lo == term
                        tl += term & 0x7FFFFFFFll;
                    }
                    th = wave_sum(th);
                    tl = wave_sum(tl);
                    // two's complement: the unsigned add is the signed one
                    if (lead && th != 0) atomicAdd(out + 4 + 2 * slot, (unsigned long long)th);
                    if (lead && tl != 0) atomicAdd(out + 5 + 2 * slot, (unsigned long long)tl);
                }
            }
        }
    }
}

}  // namespace

// The geometry of hp_scan_align_plane_step for H hypotheses: threads per workgroup, source rows a lane holds (a workgroup covers
// threads * rows_per_lane consecutive rows of the ragged source set), hypotheses per work item (always 1: the yaw search
// stays with hp_scan_align_step) and targets per LDS tile.  Host only.
HP_API int hp_scan_align_plane_plan(int H, int* threads, int* rows_per_lane, int* hypothesis_group, int* tile) {
    HP_CHECK_ARG(H >= 1 && H <= kPlaneMaxHyp && threads && rows_per_lane && hypothesis_group && tile);
    *threads = kThreads;
    *rows_per_lane = kRows;
    *hypothesis_group = 1;
    *tile = kTile;
    return 0;
}

// Bytes of device workspace hp_scan_align_plane_step needs: none — the moments are the only accumulators.  Host only.
HP_API long hp_scan_align_plane_workspace_bytes(int S, int H) {
    if (S < 1 || H < 1 || H > kPlaneMaxHyp) return -1;
    return 0;
}

// One point-to-plane ICP step of S x H jobs: see the law at the top and include/hyperpocket_hip.h.
HP_API int hp_scan_align_plane_step(int S, int H, long long T, const float* points, const long long* offsets, long long U,
                                    const float* tpoints, const long long* toffsets, const float* tnormals,
                                    const float* transforms, float max_dist, const float* anchor, const int* shift,
                                    long long* moments, int* index, float* dist2, hipStream_t stream) {
    HP_CHECK_ARG(S >= 1 && H >= 1 && H <= kPlaneMaxHyp && T >= 0 && U >= 0 && T <= (1ll << 40) && U <= (1ll << 40));
    HP_CHECK_ARG(points && offsets && tpoints && toffsets && tnormals && transforms && anchor && shift && moments);
    HP_CHECK_ARG((index == nullptr) == (dist2 == nullptr));
    HP_CHECK_ARG(max_dist >= 0.f);                                             // refuses a NaN too; +inf is no gate
    const float g2 = max_dist * max_dist;
    const hipError_t err = hipMemsetAsync(moments, 0, (size_t)S * H * kMoments * sizeof(long long), stream);
    if (err != hipSuccess) return (int)err;
    if (T == 0) return 0;
    if (index) {
        const long long total = (long long)H * T, blocks = (total + kThreads * 8 - 1) / (kThreads * 8);
        hipLaunchKernelGGL(align_plane_fill_kernel, dim3((unsigned)std::min<long long>(blocks, kMaxGrid)), dim3(kThreads), 0, stream,
                           total, index, dist2);
    }
    const long long items = (T + kChunk - 1) / kChunk * H;
    hipLaunchKernelGGL(align_plane_sweep_kernel, dim3((unsigned)std::min<long long>(items, kMaxGrid)), dim3(kThreads), 0, stream, S, H,
                       T, U, points, offsets, tpoints, toffsets, tnormals, transforms, g2, anchor, shift, moments, index, dist2);
    HP_RETURN_LAST_ERROR();
}
