// One step of point-to-plane rigid registration (ICP) over ragged sets: every source row, moved by each of H
// transforms, finds its nearest target row, and the matches leave as the exact integer 6x6 normal system of the linearised
// point-to-plane error (ops.rigid_from_plane_moments on the host) — the error a depth sensor's captures call for: two captures
// of one surface never sample the same points, and only the distance along the target's normal says how far apart they are.
//
// The transform, absence, the match, the gate, the quantisation (u, v), the fill and the sweep are csrc/hp_align.h's — the very
// code of csrc/align.hip's step, so index and dist2 are its index and dist2 bit for bit — at one hypothesis per work item: the
// yaw search stays with the point-to-point step, H > 1 is served but not grouped.  This file's own, per job (set s, hypothesis
// h) (include/hyperpocket_hip.h and tests/align_plane_law.py have it in full), with n = tnormals[j] of the matched row:
//   w = trunc(ldexp(n, 9)); without normal (counted, not summed) when a scaled component is not finite or reaches 2^10, when
//   w.w == 0 or when w.w > 2^18 + 2^11;  c = u x w, a = (c, w), b = -(u - v).w: |c_i| < 2^30, |b| < 2^31, both held in 32 bits
//   28 terms: a_i a_j (i <= j, row-major), a_i b, b b, each below 2^62; a term leaves as hi = term >> 31 and lo = term & (2^31 - 1)
//   moments (S,H,60) = [used, clipped, without normal, 0, then (sum hi, sum lo) of the 28 terms]
//
//   epilogue in registers: the matched row's normal read back once, its quantisation, and the seven 32-bit integers (a, b) of
//            each of the lane's two rows — zeros for a row that is not used, so that what follows has no branch.  The 56 sums
//            never exist side by side: one term at a time is formed from those integers (a 32 x 32 -> 64 multiply), split,
//            summed over the lane's rows, reduced over the wave by shuffles, and the wave's lane 0 issues one 64-bit integer add
//            per non-zero value.  The three counts travel as one packed 64-bit word (21 bits each; a wave holds 128 rows).
//            With kMaxPoints rows a set the hi and lo sums stay below 2^48.
#include "hp_align.h"

namespace {

using namespace hp_align;

constexpr int kMoments = 60;
constexpr int kNormalBits = 9;
constexpr int kNormalMax = (1 << 18) + (1 << 11);   // w.w of a unit normal is at most 2^18

// The slot of the term a_i a_j, i <= j <= 6 with a_6 = b: the 21 entries of the 6x6 upper triangle row-major, then a_i b, then b b.
__device__ constexpr int slot_of(int i, int j) { return j < 6 ? i * 6 - i * (i - 1) / 2 + (j - i) : 21 + i; }

__global__ __launch_bounds__(kThreads) void align_plane_fill_kernel(long long total, int* __restrict__ index, float* __restrict__ dist2) {
    fill(total, index, dist2);
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
    align_sweep<1>(S, H, T, U, points, offsets, tpoints, toffsets, transforms, g2, anchor, shift, index, dist2,
                   [=](int s, int h, auto pair_of) {
        const float* N = tnormals + toffsets[s] * 3;
        int a[kRows][7];                                                       // (c, w, b) of the lane's rows; zeros where unused
        long long counts = 0;                                                  // used | clipped << 21 | without normal << 42
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
#pragma unroll
            for (int i = 0; i < 7; ++i) a[r][i] = 0;
            const Pair pair = pair_of(r);
            if (pair.state == kClipped) counts += 1ll << 21;
            if (pair.state != kUsed) continue;
            const float* n = N + (long)pair.at * 3;
            const float sn[3] = {ldexpf(n[0], kNormalBits), ldexpf(n[1], kNormalBits), ldexpf(n[2], kNormalBits)};
            bool small = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) small = small && fabsf(sn[k]) < 1024.f;   // NaN, inf: false
            long long u[3], d[3], w[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                u[k] = pair.u[k];
                d[k] = pair.u[k] - pair.v[k];
                w[k] = small ? (int)sn[k] : 0;                                 // the cast truncates towards zero
            }
            const long long ww = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
            if (!small || ww == 0 || ww > kNormalMax) {
                counts += 1ll << 42;
                continue;
            }
            counts += 1;
            a[r][0] = (int)(u[1] * w[2] - u[2] * w[1]);                        // |c_i| < 2^30 and |b| < 2^31: see the law
            a[r][1] = (int)(u[2] * w[0] - u[0] * w[2]);
            a[r][2] = (int)(u[0] * w[1] - u[1] * w[0]);
            a[r][3] = (int)w[0];
            a[r][4] = (int)w[1];
            a[r][5] = (int)w[2];
            a[r][6] = (int)-(d[0] * w[0] + d[1] * w[1] + d[2] * w[2]);
        }
        if (!__any(counts != 0)) return;                                       // the wave holds no correspondence of this job
        const bool lead = (threadIdx.x & (HP_WAVE - 1)) == 0;
        unsigned long long* out = reinterpret_cast<unsigned long long*>(moments + ((size_t)s * H + h) * kMoments);
        counts = __shfl(hp::wave_sum(counts), 0, HP_WAVE);                     // every lane holds the wave's three counts
        if (lead) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const unsigned long long c = ((unsigned long long)counts >> (21 * k)) & ((1u << 21) - 1);
                if (c) atomicAdd(out + k, c);
            }
        }
        if ((counts & ((1 << 21) - 1)) == 0) return;                           // none of them is used: every term is 0
#pragma unroll
        for (int i = 0; i < 7; ++i) {
#pragma unroll
            for (int j = i; j < 7; ++j) {
                const int slot = i == 6 ? 27 : slot_of(i, j);
                long long th = 0, tl = 0;
#pragma unroll
                for (int r = 0; r < kRows; ++r) {
                    const long long term = (long long)a[r][i] * a[r][j];
                    th += term >> 31;                                          // arithmetic: hi * 2^31 + lo == term
                    tl += term & 0x7FFFFFFFll;
                }
                th = hp::wave_sum(th);
                tl = hp::wave_sum(tl);
                // two's complement: the unsigned add is the signed one
                if (lead && th != 0) atomicAdd(out + 4 + 2 * slot, (unsigned long long)th);
                if (lead && tl != 0) atomicAdd(out + 5 + 2 * slot, (unsigned long long)tl);
            }
        }
    });
}

}  // namespace

// The geometry of hp_scan_align_plane_step for H hypotheses: threads per workgroup, source rows a lane holds (a workgroup covers
// threads * rows_per_lane consecutive rows of the ragged source set), hypotheses per work item (always 1: the yaw search
// stays with hp_scan_align_step) and targets per LDS tile.  Host only.
HP_API int hp_scan_align_plane_plan(int H, int* threads, int* rows_per_lane, int* hypothesis_group, int* tile) {
    HP_CHECK_ARG(H >= 1 && H <= kMaxHyp && threads && rows_per_lane && hypothesis_group && tile);
    *threads = kThreads;
    *rows_per_lane = kRows;
    *hypothesis_group = 1;
    *tile = kTile;
    return 0;
}

// Bytes of device workspace hp_scan_align_plane_step needs: none — the moments are the only accumulators.  Host only.
HP_API long hp_scan_align_plane_workspace_bytes(int S, int H) {
    if (S < 1 || H < 1 || H > kMaxHyp) return -1;
    return 0;
}

// One point-to-plane ICP step of S x H jobs: see the law in csrc/hp_align.h and at the top, and include/hyperpocket_hip.h.
HP_API int hp_scan_align_plane_step(int S, int H, long long T, const float* points, const long long* offsets, long long U,
                                    const float* tpoints, const long long* toffsets, const float* tnormals,
                                    const float* transforms, float max_dist, const float* anchor, const int* shift,
                                    long long* moments, int* index, float* dist2, hipStream_t stream) {
    return align_step(align_plane_fill_kernel, S, H, T, U,
                      points && offsets && tpoints && toffsets && tnormals && transforms && anchor && shift && moments, max_dist,
                      moments, kMoments, index, dist2, stream, [&](float g2) {
        hipLaunchKernelGGL(align_plane_sweep_kernel, sweep_grid(H, T, 1), dim3(kThreads), 0, stream, S, H, T, U, points, offsets,
                           tpoints, toffsets, tnormals, transforms, g2, anchor, shift, moments, index, dist2);
    });
}
