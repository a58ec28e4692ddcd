// One step of point-to-point rigid registration (ICP) over ragged sets: every source row, moved by each of H
// transforms, finds its nearest target row, and the matches leave as the exact integer moments a closed-form rigid fit needs
// (ops.rigid_from_moments on the host) — what poses a cleaned scan against a template, a ground truth or another view.
//
// The transform, absence, the match, the gate, the quantisation, the fill and the sweep are csrc/hp_align.h's.  This file's own:
//   moments (S,H,18) = [used, clipped, sum u (3), sum v (3), sum u_a*v_b (9), sum |u - v|^2]
//   epilogue the 18 sums of a hypothesis are formed over the lane's rows (the eight that are linear in u and v in 32 bits: two
//            rows stay below 2^21), widened, reduced over the wave by shuffles, and the wave's lane 0 issues one 64-bit integer
//            add per non-zero sum.
//   G is 1 for H == 1 (the refinement of one transform per set) and 4 otherwise (the yaw search).
#include "hp_align.h"

namespace {

using namespace hp_align;

__global__ __launch_bounds__(kThreads) void align_fill_kernel(long long total, int* __restrict__ index, float* __restrict__ dist2) {
    fill(total, index, dist2);
}

template <int G>
__global__ __launch_bounds__(kThreads) void align_sweep_kernel(int S, int H, long long T, long long U, const float* __restrict__ points,
                                                               const long long* __restrict__ offsets,
                                                               const float* __restrict__ tpoints,
                                                               const long long* __restrict__ toffsets,
                                                               const float* __restrict__ transforms, float g2,
                                                               const float* __restrict__ anchor, const int* __restrict__ shift,
                                                               long long* __restrict__ moments, int* __restrict__ index,
                                                               float* __restrict__ dist2) {
    align_sweep<G>(S, H, T, U, points, offsets, tpoints, toffsets, transforms, g2, anchor, shift, index, dist2,
                   [=](int s, int h, auto pair_of) {
        int lin[8] = {0, 0, 0, 0, 0, 0, 0, 0};                                 // used, clipped, sum u, sum v of the lane's rows: below 2^21
        long long quad[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};                   // sum u_a*v_b, sum |u - v|^2
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const Pair pair = pair_of(r);
            if (pair.state == kNoPair) continue;
            if (pair.state == kClipped) {
                lin[1] += 1;
                continue;
            }
            const int (&u)[3] = pair.u, (&v)[3] = pair.v;
            lin[0] += 1;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lin[2 + a] += u[a];
                lin[5 + a] += v[a];
#pragma unroll
                for (int b = 0; b < 3; ++b) quad[3 * a + b] += (long long)u[a] * v[b];
                quad[9] += (long long)(u[a] - v[a]) * (u[a] - v[a]);
            }
        }
        if (!__any(lin[0] | lin[1])) return;                                   // the wave holds no correspondence of this job
        long long* out = moments + ((size_t)s * H + h) * 18;
#pragma unroll
        for (int i = 0; i < 18; ++i) {
            const long long w = hp::wave_sum(i < 8 ? (long long)lin[i] : quad[i - 8]);
            // two's complement: the unsigned add is the signed one
            if ((threadIdx.x & (HP_WAVE - 1)) == 0 && w != 0)
                atomicAdd(reinterpret_cast<unsigned long long*>(out + i), (unsigned long long)w);
        }
    });
}

}  // namespace

// The geometry of hp_scan_align_step for H hypotheses: threads per workgroup, source rows a lane holds (a workgroup covers
// threads * rows_per_lane consecutive rows of the ragged source set), hypotheses per work item and targets per LDS tile.
// Host only.
HP_API int hp_scan_align_plan(int H, int* threads, int* rows_per_lane, int* hypothesis_group, int* tile) {
    HP_CHECK_ARG(H >= 1 && H <= kMaxHyp && threads && rows_per_lane && hypothesis_group && tile);
    *threads = kThreads;
    *rows_per_lane = kRows;
    *hypothesis_group = H == 1 ? 1 : kGroup;
    *tile = kTile;
    return 0;
}

// Bytes of device workspace hp_scan_align_step needs: none — the moments are the only accumulators.  Host only.
HP_API long hp_scan_align_workspace_bytes(int S, int H) {
    if (S < 1 || H < 1 || H > kMaxHyp) return -1;
    return 0;
}

// One ICP step of S x H jobs: see the law in csrc/hp_align.h, the moments at the top and include/hyperpocket_hip.h.
HP_API int hp_scan_align_step(int S, int H, long long T, const float* points, const long long* offsets, long long U,
                              const float* tpoints, const long long* toffsets, const float* transforms, float max_dist,
                              const float* anchor, const int* shift, long long* moments, int* index, float* dist2,
                              hipStream_t stream) {
    return align_step(align_fill_kernel, S, H, T, U, points && offsets && tpoints && toffsets && transforms && anchor && shift && moments,
                      max_dist, moments, 18, index, dist2, stream, [&](float g2) {
        if (H == 1)
            hipLaunchKernelGGL(align_sweep_kernel<1>, sweep_grid(H, T, 1), dim3(kThreads), 0, stream, S, H, T, U, points, offsets,
                               tpoints, toffsets, transforms, g2, anchor, shift, moments, index, dist2);
        else
            hipLaunchKernelGGL(align_sweep_kernel<kGroup>, sweep_grid(H, T, kGroup), dim3(kThreads), 0, stream, S, H, T, U, points,
                               offsets, tpoints, toffsets, transforms, g2, anchor, shift, moments, index, dist2);
    });
}
