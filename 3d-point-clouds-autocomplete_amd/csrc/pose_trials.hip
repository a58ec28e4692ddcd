// A rigid start for every set of two ragged sets from given matches, by random sample consensus over matched triples
// (DESIGN.md 3r): the step between the descriptor matches (features.hip) and the refinements (align.hip, align_plane.hip), which
// only converge from a pose that is close already.
//
// The law, per set (include/hyperpocket_hip.h and tests/pose_trials_law.py have it in full):
//   a source row is matched when 0 <= match < m and it and its target row are finite.  Trial h samples the rows
//   r_k = (word[3h+k] * n) >> 32 of Philox4x32-10 (key seed, counter (stream, q, tag 5)).  It is valid iff the three rows are
//   matched and differ, their targets differ, every side agrees in length (fp32: ls2 >= rho2 * lt2 and lt2 >= rho2 * ls2), both
//   triangles have a frame (fp64: e1 = (b - a) / |b - a|, e3 along e1 x (c - a), e2 = e3 x e1; not collinear) and the transform
//   R = Ft Fs^T, t = ct - R cs (c the centroids), rounded to 12 fp32, is finite.  The first `keep` valid trials in ascending h are
//   kept; a kept trial's score is the number of matched rows with |T p - q|^2 <= g2 in align.hip's fp32 formulas; the winner has
//   the most inliers, ties to the lower h.
//
//   draw     one workgroup of 256 lanes per set walks the trials 256 at a time in ascending order: a lane draws and fits one
//            trial, a ballot and a four-entry LDS table give its rank among the valid ones, and it writes its transform and its h
//            at base + rank while that is below `keep` — an ordered compaction, so the kept list is a function of the inputs.
//            Also zeroes the kept trials' counters and writes valid and kept.
//   score    the hot path, plane.hip's shape.  A workgroup holds a chunk of 1024 consecutive source rows in registers, 4 per lane,
//            each with its gathered target row, and for every set the chunk meets walks the kept transforms through an LDS tile of
//            256 x 12 floats that all lanes read at one address; inliers are counted per wave by popcount(ballot), lane u keeps
//            the count of transform u of a group of 64, and the counters take one integer add per (workgroup, set, transform).
//            O(n * kept), not O(n * trials).
//   winner   grid (S): max over ((count + 1) << 12 | 4095 - slot); writes trial, inliers, found and the transform.
// Integer adds and an integer max only: no order of evaluation can change a bit.  Three launches, no host synchronisation.
#include "hp_align.h"
#include "hp_philox.h"

namespace {

using hp::finite_bits, hp::kNanBits;
constexpr int kPoseMaxTrials = 65536;      // = HP_POSE_MAX_TRIALS
constexpr int kPoseMaxKeep = 4096;         // = HP_POSE_MAX_KEEP: 4095 - slot fits the 12 low bits of the winner's key
constexpr uint32_t kTagPose = 5;           // tags 0-2: scan_prep.hip and batch_maker.hip, 3: mesh.hip, 4: plane.hip
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / HP_WAVE;
constexpr int kRowsPerLane = 4;
constexpr int kChunk = kThreads * kRowsPerLane;
constexpr int kTile = 256;                 // transforms per LDS tile (12 KiB); = kThreads: a lane owns one LDS counter
constexpr int kGrid = 2048;
constexpr double kCollinear = 0x1p-24;     // = pose_trials_law.COLLINEAR
constexpr float kFltMax = 3.4028234664e38f;

__device__ __forceinline__ double ddot(const double (&a)[3], const double (&b)[3]) {
#pragma clang fp contract(off)
    return __dadd_rn(__dadd_rn(__dmul_rn(a[0], b[0]), __dmul_rn(a[1], b[1])), __dmul_rn(a[2], b[2]));
}

__device__ __forceinline__ void dcross(const double (&a)[3], const double (&b)[3], double (&out)[3]) {
#pragma clang fp contract(off)
    out[0] = __dsub_rn(__dmul_rn(a[1], b[2]), __dmul_rn(a[2], b[1]));
    out[1] = __dsub_rn(__dmul_rn(a[2], b[0]), __dmul_rn(a[0], b[2]));
    out[2] = __dsub_rn(__dmul_rn(a[0], b[1]), __dmul_rn(a[1], b[0]));
}

__device__ __forceinline__ float len2(const float (&a)[3], const float (&b)[3]) {
#pragma clang fp contract(off)
    const float dx = __fsub_rn(b[0], a[0]), dy = __fsub_rn(b[1], a[1]), dz = __fsub_rn(b[2], a[2]);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// The frame of a triangle: E[k] = e_(k+1), the centroid; false where it has none.
__device__ __forceinline__ bool frame(const float (&p)[3][3], double (&E)[3][3], double (&centre)[3]) {
#pragma clang fp contract(off)
    double u[3], v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        u[c] = __dsub_rn((double)p[1][c], (double)p[0][c]);
        v[c] = __dsub_rn((double)p[2][c], (double)p[0][c]);
        centre[c] = __ddiv_rn(__dadd_rn(__dadd_rn((double)p[0][c], (double)p[1][c]), (double)p[2][c]), 3.0);
    }
    const double l1 = __dsqrt_rn(ddot(u, u));
    if (!(l1 > 0.0)) return false;
#pragma unroll
    for (int c = 0; c < 3; ++c) E[0][c] = __ddiv_rn(u[c], l1);
    double x[3];
    dcross(E[0], v, x);
    const double xx = ddot(x, x);
    if (!(xx > __dmul_rn(kCollinear, ddot(v, v)))) return false;
    const double l3 = __dsqrt_rn(xx);
#pragma unroll
    for (int c = 0; c < 3; ++c) E[2][c] = __ddiv_rn(x[c], l3);
    dcross(E[2], E[0], E[1]);
    return true;
}

__global__ __launch_bounds__(kThreads) void pose_draw_kernel(int trials, int keep, long long T, long long U,
                                                             const float* __restrict__ points, const long long* __restrict__ offsets,
                                                             const float* __restrict__ tpoints, const long long* __restrict__ toffsets,
                                                             const int* __restrict__ match, const long long* __restrict__ streams,
                                                             unsigned long long seed, float rho2, float* __restrict__ hyp,
                                                             int* __restrict__ slot_trial, int* __restrict__ counts,
                                                             int* __restrict__ valid, int* __restrict__ kept) {
#pragma clang fp contract(off)
    __shared__ int sWave[kWaves];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & (HP_WAVE - 1), wave = tid >> 6;
    for (int i = tid; i < keep; i += kThreads) counts[(size_t)s * keep + i] = 0;
    const long long lo = offsets[s], hi = offsets[s + 1], tlo = toffsets[s], thi = toffsets[s + 1];
    int base = 0;
    if (hp_align::set_ok(lo, hi, T) && hp_align::set_ok(tlo, thi, U)) {            // uniform
        const int n = (int)(hi - lo), m = (int)(thi - tlo);
        const unsigned long long sid = streams ? (unsigned long long)streams[s] : (unsigned long long)s;
        const uint2 key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)), stream = make_uint2((uint32_t)sid, (uint32_t)(sid >> 32));
        for (int h0 = 0; h0 < trials; h0 += kThreads) {
            const int h = h0 + tid;
            bool ok = h < trials;
            float M[12];
            if (ok) {
                int r[3], q[3];
                float a[3][3], b[3][3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    r[k] = sample_row(key, stream, h, k, n, kTagPose);
                    q[k] = match[lo + r[k]];
                    ok = ok && q[k] >= 0 && q[k] < m;
                    const int qq = ok ? q[k] : 0;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        a[k][c] = points[(lo + r[k]) * 3 + c];
                        b[k][c] = tpoints[(tlo + qq) * 3 + c];
                        ok = ok && finite_bits(a[k][c]) && finite_bits(b[k][c]);
                    }
                }
                ok = ok && r[0] != r[1] && r[0] != r[2] && r[1] != r[2] && q[0] != q[1] && q[0] != q[2] && q[1] != q[2];
                if (ok) {
#pragma unroll
                    for (int e = 0; e < 3; ++e) {
                        const int i = e == 2 ? 1 : 0, j = e == 0 ? 1 : 2;                  // the sides (0,1), (0,2), (1,2)
                        const float ls = len2(a[i], a[j]), lt = len2(b[i], b[j]);
                        ok = ok && ls <= kFltMax && lt <= kFltMax && ls >= __fmul_rn(rho2, lt) && lt >= __fmul_rn(rho2, ls);
                    }
                }
                if (ok) {
                    double Es[3][3], Et[3][3], cs[3], ct[3];
                    ok = frame(a, Es, cs);
                    ok = frame(b, Et, ct) && ok;
                    if (ok) {
#pragma unroll
                        for (int i = 0; i < 3; ++i) {
                            double R[3];
#pragma unroll
                            for (int j = 0; j < 3; ++j) {
                                R[j] = __dadd_rn(__dadd_rn(__dmul_rn(Et[0][i], Es[0][j]), __dmul_rn(Et[1][i], Es[1][j])),
                                                 __dmul_rn(Et[2][i], Es[2][j]));
                                M[i * 4 + j] = __double2float_rn(R[j]);
                            }
                            M[i * 4 + 3] = __double2float_rn(__dsub_rn(ct[i], ddot(R, cs)));
                        }
#pragma unroll
                        for (int i = 0; i < 12; ++i) ok = ok && finite_bits(M[i]);
                    }
                }
            }
            const unsigned long long vote = __ballot(ok);
            if (lane == 0) sWave[wave] = __popcll(vote);
            __syncthreads();
            int before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                before += w < wave ? sWave[w] : 0;
                total += sWave[w];
            }
            const int pos = base + before + __popcll(vote & ((1ull << lane) - 1ull));
            if (ok && pos < keep) {
                float* out = hyp + ((size_t)s * keep + pos) * 12;
#pragma unroll
                for (int i = 0; i < 12; ++i) out[i] = M[i];
                slot_trial[(size_t)s * keep + pos] = h;
            }
            base += total;
            __syncthreads();                                                   // the table is read before the next round writes it
        }
    }
    if (tid == 0) {
        valid[s] = base;
        kept[s] = base < keep ? base : keep;
    }
}

__global__ __launch_bounds__(kThreads) void pose_score_kernel(int S, int keep, long long T, long long U, const float* __restrict__ points,
                                                              const long long* __restrict__ offsets, const float* __restrict__ tpoints,
                                                              const long long* __restrict__ toffsets, const int* __restrict__ match,
                                                              float g2, const float* __restrict__ hyp, const int* __restrict__ kept,
                                                              int* __restrict__ counts) {
#pragma clang fp contract(off)
    __shared__ float4 tile[kTile * 3];
    __shared__ int sCount[kTile];
    const int tid = threadIdx.x, lane = tid & (HP_WAVE - 1);
    for (long long row0 = (long long)blockIdx.x * kChunk; row0 < T; row0 += (long long)gridDim.x * kChunk) {
        float px[kRowsPerLane], py[kRowsPerLane], pz[kRowsPerLane];
        int mt[kRowsPerLane];
#pragma unroll
        for (int k = 0; k < kRowsPerLane; ++k) {
            const long long g = row0 + k * kThreads + tid;
            px[k] = py[k] = pz[k] = 0.f;
            mt[k] = -1;
            if (g < T) {
                px[k] = points[g * 3];
                py[k] = points[g * 3 + 1];
                pz[k] = points[g * 3 + 2];
                if (finite_bits(px[k]) && finite_bits(py[k]) && finite_bits(pz[k])) mt[k] = match[g];
            }
        }
        const long long last = (row0 + kChunk < T ? row0 + kChunk : T) - 1;
        // every value that steers these loops is uniform over the workgroup
        for (int s = hp_align::set_of(offsets, S, row0); s < S && offsets[s] <= last; ++s) {
            const long long lo = offsets[s], hi = offsets[s + 1], tlo = toffsets[s], thi = toffsets[s + 1];
            if (!hp_align::set_ok(lo, hi, T) || !hp_align::set_ok(tlo, thi, U)) continue;
            const int H = kept[s];
            if (H == 0) continue;
            const int m = (int)(thi - tlo);
            float qx[kRowsPerLane], qy[kRowsPerLane], qz[kRowsPerLane];
            bool mine[kRowsPerLane];
#pragma unroll
            for (int k = 0; k < kRowsPerLane; ++k) {
                const long long g = row0 + k * kThreads + tid;
                mine[k] = g >= lo && g < hi && mt[k] >= 0 && mt[k] < m;
                qx[k] = qy[k] = qz[k] = 0.f;
                if (mine[k]) {
                    const float* Q = tpoints + (tlo + mt[k]) * 3;
                    qx[k] = Q[0];
                    qy[k] = Q[1];
                    qz[k] = Q[2];
                    mine[k] = finite_bits(qx[k]) && finite_bits(qy[k]) && finite_bits(qz[k]);
                }
            }
            const float4* Hs = reinterpret_cast<const float4*>(hyp + (size_t)s * keep * 12);
            for (int t0 = 0; t0 < H; t0 += kTile) {
                const int cnt = H - t0 < kTile ? H - t0 : kTile;
                __syncthreads();                                           // the tile before this one has been read
                for (int i = tid; i < cnt * 3; i += kThreads) tile[i] = Hs[(size_t)t0 * 3 + i];
                sCount[tid] = 0;
                __syncthreads();
                for (int g0 = 0; g0 < cnt; g0 += HP_WAVE) {
                    const int lim = cnt - g0 < HP_WAVE ? cnt - g0 : HP_WAVE;
                    int acc = 0;                                           // lane u: the wave's inliers of transform g0 + u
                    for (int u = 0; u < lim; ++u) {
                        const float4 A = tile[(g0 + u) * 3], B = tile[(g0 + u) * 3 + 1], C = tile[(g0 + u) * 3 + 2];
                        int c = 0;
#pragma unroll
                        for (int k = 0; k < kRowsPerLane; ++k) {
                            const float x = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(A.x, px[k]), __fmul_rn(A.y, py[k])), __fmul_rn(A.z, pz[k])), A.w);
                            const float y = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(B.x, px[k]), __fmul_rn(B.y, py[k])), __fmul_rn(B.z, pz[k])), B.w);
                            const float z = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(C.x, px[k]), __fmul_rn(C.y, py[k])), __fmul_rn(C.z, pz[k])), C.w);
                            const float dx = __fsub_rn(qx[k], x), dy = __fsub_rn(qy[k], y), dz = __fsub_rn(qz[k], z);
                            const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
                            c += __popcll(__ballot(mine[k] && d2 <= g2));      // g2 <= FLT_MAX: false for +inf and a NaN
                        }
                        if (lane == u) acc = c;
                    }
                    if (acc) atomicAdd(&sCount[g0 + lane], acc);
                }
                __syncthreads();
                if (tid < cnt && sCount[tid]) atomicAdd(&counts[(size_t)s * keep + t0 + tid], sCount[tid]);
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void pose_winner_kernel(int keep, int min_inliers, const float* __restrict__ hyp,
                                                               const int* __restrict__ slot_trial, const int* __restrict__ counts,
                                                               const int* __restrict__ kept, int* __restrict__ trial,
                                                               int* __restrict__ inliers, int* __restrict__ found,
                                                               float* __restrict__ transform) {
    __shared__ unsigned long long part[kWaves];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int H = kept[s];
    unsigned long long best = 0ull;                        // (count + 1) << 12 | 4095 - slot: the most inliers, then the lower h
    for (int i = tid; i < H; i += kThreads) {
        const unsigned long long key = ((unsigned long long)(counts[(size_t)s * keep + i] + 1) << 12) | (unsigned long long)(kPoseMaxKeep - 1 - i);
        best = key > best ? key : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, HP_WAVE);
        best = other > best ? other : best;
    }
    if ((tid & (HP_WAVE - 1)) == 0) part[tid >> 6] = best;
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < kWaves; ++w) best = part[w] > best ? part[w] : best;
    int h = -1, count = 0;
    const float nan = __int_as_float(kNanBits);
    float M[12] = {nan, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan, nan};
    if (best) {
        const int slot = kPoseMaxKeep - 1 - (int)(best & (unsigned long long)(kPoseMaxKeep - 1));
        count = (int)(best >> 12) - 1;
        h = slot_trial[(size_t)s * keep + slot];
        for (int i = 0; i < 12; ++i) M[i] = hyp[((size_t)s * keep + slot) * 12 + i];
    }
    trial[s] = h;
    inliers[s] = count;
    found[s] = h >= 0 && count >= min_inliers;
    for (int i = 0; i < 12; ++i) transform[s * 12 + i] = M[i];
}

bool pose_args_ok(int trials, int keep) { return trials >= 1 && trials <= kPoseMaxTrials && keep >= 1 && keep <= kPoseMaxKeep; }

}  // namespace

// The geometry of hp_scan_pose_trials: threads per workgroup, rows a lane of the score kernel holds and transforms per LDS tile.
// Host only.
HP_API int hp_scan_pose_trials_plan(int trials, int keep, int* threads, int* rows_per_lane, int* tile) {
    HP_CHECK_ARG(pose_args_ok(trials, keep) && threads && rows_per_lane && tile);
    *threads = kThreads;
    *rows_per_lane = kRowsPerLane;
    *tile = kTile;
    return 0;
}

// Bytes of hp_scan_pose_trials' workspace: the kept transforms (S,keep,12) fp32, their trials and their counts (S,keep) int32.
// Host only.
HP_API long hp_scan_pose_trials_workspace_bytes(int S, int keep) {
    if (S < 1 || keep < 1 || keep > kPoseMaxKeep) return -1;
    return (long)((size_t)S * keep * (12 * sizeof(float) + 2 * sizeof(int)));
}

// A rigid start of each of S sets from matched triples; the law is in include/hyperpocket_hip.h.
HP_API int hp_scan_pose_trials(int S, long long T, const float* points, const long long* offsets, long long U, const float* tpoints,
                               const long long* toffsets, const int* match, const long long* streams, unsigned long long seed,
                               int trials, int keep, float rho2, float inlier_dist, int min_inliers, int* trial, int* inliers,
                               int* found, float* transform, int* valid, int* kept, void* ws, hipStream_t stream) {
    HP_CHECK_ARG(S >= 1 && T >= 0 && U >= 0 && T <= (1ll << 40) && U <= (1ll << 40) && pose_args_ok(trials, keep));
    HP_CHECK_ARG(offsets && toffsets && trial && inliers && found && transform && valid && kept && ws);
    HP_CHECK_ARG((T == 0 || (points && match)) && (U == 0 || tpoints));
    HP_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 15) == 0);
    HP_CHECK_ARG(rho2 >= 0.f && rho2 <= 1.f && inlier_dist >= 0.f && min_inliers >= 0);      // refuses a NaN too
    const float g2 = std::min(inlier_dist * inlier_dist, kFltMax);                         // +inf: every finite distance passes
    float* hyp = static_cast<float*>(ws);
    int* slot_trial = reinterpret_cast<int*>(hyp + (size_t)S * keep * 12);
    int* counts = slot_trial + (size_t)S * keep;
    hipLaunchKernelGGL(pose_draw_kernel, dim3(S), dim3(kThreads), 0, stream, trials, keep, T, U, points, offsets, tpoints, toffsets,
                       match, streams, seed, rho2, hyp, slot_trial, counts, valid, kept);
    if (T > 0)
        hipLaunchKernelGGL(pose_score_kernel, dim3((unsigned)std::min<long long>((T + kChunk - 1) / kChunk, kGrid)), dim3(kThreads), 0,
                           stream, S, keep, T, U, points, offsets, tpoints, toffsets, match, g2, hyp, kept, counts);
    hipLaunchKernelGGL(pose_winner_kernel, dim3(S), dim3(kThreads), 0, stream, keep, min_inliers, hyp, slot_trial, counts, kept, trial,
                       inliers, found, transform);
    HP_RETURN_LAST_ERROR();
}
