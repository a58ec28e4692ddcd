// The supporting plane of ragged scans by random sample consensus: the floor or table top that joins every
// object of a real scene into one component, fitted and marked before the cluster kernel (clusters.hip) sees the scan.
//
// The law, per scan (include/hyperpocket_hip.h and tests/plane_law.py have it in full):
//   trial h samples rows r_k = (word[3h+k] * n) >> 32 of Philox4x32-10 (key seed, counter (stream, q, tag 4)); with a, b, c the
//   three rows, nrm = (b - a) x (c - a), len2 = |nrm|^2, rhs = threshold^2 * len2, every operation one fp32 rounding; the
//   trial is valid iff n >= 3, len2 finite and > 0, rhs finite.  Row p is an inlier iff e*e <= rhs with e = nrm . (p - a).
//   The winner is the valid trial with the most inliers, ties to the lower h.  Of its inliers: the mask, and the integer
//   moments of q = trunc((p - a) * 2^(19 - e)), e the exponent of the largest |p - a| coordinate.
//
//   hypotheses  grid (S, H / 256): a thread draws one trial, writes its 8 floats (a, nrm, rhs or -1, valid) and zeroes its count.
//   consensus   the hot path.  A workgroup of 256 lanes holds a chunk of 1024 consecutive rows of the ragged set in registers,
//               4 per lane, and for every scan the chunk meets walks that scan's hypotheses through an LDS tile of 256 trials:
//               all lanes read one address (a broadcast, no bank conflict), the inliers of a trial are counted per wave by
//               popcount(ballot), and lane u of a wave keeps the count of trial u of a group of 64, so the LDS counters take one
//               add per wave and 64 trials.  counts (S,H) gets one integer add per (workgroup, scan, trial).
//   winner      grid (S): max over ((count + 1) << 12 | 4095 - h) of the valid trials; writes trial, inliers, found, sample,
//               sample_plane, and resets the scan's moments, shift and maximum.
//   mask        over the rows: the winner's inlier mask and, by an integer max on the bits, the largest |p - a| coordinate.
//   moments     over the rows: q from that maximum, the nine sums per wave by shuffles, one 64-bit integer add per wave and sum.
// Integer adds and an integer max only: no order of evaluation can change a bit.  Five launches, no host synchronisation.
//
//   side        rows against given planes: dist = ((nx*x + ny*y) + nz*z) + d, keep = present and not |dist| <= threshold.
#include "hp_common.h"
#include "hp_philox.h"

namespace {

using hp::finite_bits, hp::kInfBits, hp::kNanBits, hp::scan_of;
constexpr int kScanMaxPoints = 1 << 22;    // = HP_SCAN_MAX_POINTS (include/hyperpocket_hip.h)
constexpr int kPlaneMaxTrials = 4096;      // = HP_PLANE_MAX_TRIALS: 4095 - h fits the 12 low bits of the winner's key
constexpr uint32_t kTagPlane = 4;          // tags 0-2: scan_prep.hip and batch_maker.hip, 3: mesh.hip
constexpr int kThreads = 256;              // 4 waves per workgroup
constexpr int kRowsPerLane = 4;            // rows a lane of the consensus kernel keeps in registers
constexpr int kChunk = kThreads * kRowsPerLane;
constexpr int kTrialTile = 256;            // hypotheses per LDS tile (8 KiB); = kThreads: a lane owns one LDS counter
constexpr int kGrid = 2048;                // workgroups of the row kernels: 8 per compute unit, each strides over the chunks
constexpr int kPassChunk = kThreads * 16;  // rows per workgroup and step of the mask, moment and side kernels

__device__ __forceinline__ uint2 stream_of(const long long* __restrict__ streams, int s) {
    const unsigned long long sid = streams ? (unsigned long long)streams[s] : (unsigned long long)s;
    return make_uint2((uint32_t)sid, (uint32_t)(sid >> 32));
}

// e of the law: ((nx*dx + ny*dy) + nz*dz) with d = p - a.
__device__ __forceinline__ float plane_e(float4 A, float4 B, float x, float y, float z) {
    const float dx = __fsub_rn(x, A.x), dy = __fsub_rn(y, A.y), dz = __fsub_rn(z, A.z);
    return __fadd_rn(__fadd_rn(__fmul_rn(A.w, dx), __fmul_rn(B.x, dy)), __fmul_rn(B.y, dz));
}

__global__ __launch_bounds__(kThreads) void plane_hypotheses_kernel(int H, const float* __restrict__ points,
                                                                    const long long* __restrict__ offsets,
                                                                    const long long* __restrict__ streams, unsigned long long seed,
                                                                    float t2, float4* __restrict__ hyp, int* __restrict__ counts) {
#pragma clang fp contract(off)
    const int s = blockIdx.x, h = blockIdx.y * kThreads + threadIdx.x;
    if (h >= H) return;
    const long long lo = offsets[s], len = offsets[s + 1] - lo;
    float4 A = make_float4(0.f, 0.f, 0.f, 0.f), B = make_float4(0.f, 0.f, -1.f, 0.f);     // an invalid trial: no e*e is <= -1
    if (len >= 3 && len <= kScanMaxPoints) {
        const int n = (int)len;
        const uint2 key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)), stream = stream_of(streams, s);
        const float* P = points + lo * 3;
        float p[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const long r = sample_row(key, stream, h, k, n, kTagPlane);
            p[k][0] = P[r * 3];
            p[k][1] = P[r * 3 + 1];
            p[k][2] = P[r * 3 + 2];
        }
        const float ux = __fsub_rn(p[1][0], p[0][0]), uy = __fsub_rn(p[1][1], p[0][1]), uz = __fsub_rn(p[1][2], p[0][2]);
        const float vx = __fsub_rn(p[2][0], p[0][0]), vy = __fsub_rn(p[2][1], p[0][1]), vz = __fsub_rn(p[2][2], p[0][2]);
        const float nx = __fsub_rn(__fmul_rn(uy, vz), __fmul_rn(uz, vy));
        const float ny = __fsub_rn(__fmul_rn(uz, vx), __fmul_rn(ux, vz));
        const float nz = __fsub_rn(__fmul_rn(ux, vy), __fmul_rn(uy, vx));
        const float len2 = __fadd_rn(__fadd_rn(__fmul_rn(nx, nx), __fmul_rn(ny, ny)), __fmul_rn(nz, nz));
        const float rhs = __fmul_rn(t2, len2);
        if (finite_bits(len2) && len2 > 0.f && finite_bits(rhs)) {
            A = make_float4(p[0][0], p[0][1], p[0][2], nx);
            B = make_float4(ny, nz, rhs, 1.f);
        }
    }
    const size_t at = (size_t)s * H + h;
    hyp[at * 2] = A;
    hyp[at * 2 + 1] = B;
    counts[at] = 0;
}

__global__ __launch_bounds__(kThreads) void plane_consensus_kernel(int S, int H, const float* __restrict__ points,
                                                                   const long long* __restrict__ offsets,
                                                                   const float4* __restrict__ hyp, int* __restrict__ counts) {
#pragma clang fp contract(off)
    __shared__ float4 tile[kTrialTile * 2];
    __shared__ int sCount[kTrialTile];
    const int tid = threadIdx.x, lane = tid & (HP_WAVE - 1);
    const long long T0 = offsets[0], T1 = offsets[S];
    for (long long row0 = T0 + (long long)blockIdx.x * kChunk; row0 < T1; row0 += (long long)gridDim.x * kChunk) {
        float px[kRowsPerLane], py[kRowsPerLane], pz[kRowsPerLane];
        bool ok[kRowsPerLane];
#pragma unroll
        for (int k = 0; k < kRowsPerLane; ++k) {
            const long long g = row0 + k * kThreads + tid;
            px[k] = py[k] = pz[k] = 0.f;
            if (g < T1) {
                px[k] = points[g * 3];
                py[k] = points[g * 3 + 1];
                pz[k] = points[g * 3 + 2];
            }
            ok[k] = g < T1 && finite_bits(px[k]) && finite_bits(py[k]) && finite_bits(pz[k]);
        }
        const long long last = (row0 + kChunk < T1 ? row0 + kChunk : T1) - 1;
        // every value that steers these loops is uniform over the workgroup
        for (int s = scan_of(offsets, S, row0); s < S && offsets[s] <= last; ++s) {
            const long long lo = offsets[s], hi = offsets[s + 1];
            if (hi - lo < 3 || hi - lo > kScanMaxPoints) continue;         // every trial is invalid: the counts stay 0
            bool mine[kRowsPerLane];
#pragma unroll
            for (int k = 0; k < kRowsPerLane; ++k) {
                const long long g = row0 + k * kThreads + tid;
                mine[k] = ok[k] && g >= lo && g < hi;
            }
            const float4* Hs = hyp + (size_t)s * H * 2;
            for (int t0 = 0; t0 < H; t0 += kTrialTile) {
                const int cnt = H - t0 < kTrialTile ? H - t0 : kTrialTile;
                __syncthreads();                                           // the tile before this one has been read
                for (int i = tid; i < cnt * 2; i += kThreads) tile[i] = Hs[(size_t)t0 * 2 + i];
                sCount[tid] = 0;
                __syncthreads();
                for (int g0 = 0; g0 < cnt; g0 += HP_WAVE) {
                    const int lim = cnt - g0 < HP_WAVE ? cnt - g0 : HP_WAVE;
                    int acc = 0;                                           // lane u: the wave's inliers of trial g0 + u
                    for (int u = 0; u < lim; ++u) {
                        const float4 A = tile[(g0 + u) * 2], B = tile[(g0 + u) * 2 + 1];
                        int c = 0;
#pragma unroll
                        for (int k = 0; k < kRowsPerLane; ++k) {
                            const float e = plane_e(A, B, px[k], py[k], pz[k]);
                            c += __popcll(__ballot(mine[k] && __fmul_rn(e, e) <= B.z));
                        }
                        if (lane == u) acc = c;
                    }
                    if (acc) atomicAdd(&sCount[g0 + lane], acc);
                }
                __syncthreads();
                if (tid < cnt && sCount[tid]) atomicAdd(&counts[(size_t)s * H + t0 + tid], sCount[tid]);
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void plane_winner_kernel(int H, const float* __restrict__ points,
                                                                const long long* __restrict__ offsets,
                                                                const long long* __restrict__ streams, unsigned long long seed,
                                                                int min_inliers, float min_share, const float4* __restrict__ hyp,
                                                                const int* __restrict__ counts, int* __restrict__ trial,
                                                                int* __restrict__ inliers, int* __restrict__ found,
                                                                int* __restrict__ sample, float* __restrict__ sample_plane,
                                                                long long* __restrict__ moments, int* __restrict__ shift,
                                                                unsigned* __restrict__ maxbits) {
#pragma clang fp contract(off)
    __shared__ unsigned long long part[kThreads / HP_WAVE];
    const int s = blockIdx.x, tid = threadIdx.x;
    unsigned long long best = 0ull;                        // (count + 1) << 12 | 4095 - h: the most inliers, then the lower h
    for (int h = tid; h < H; h += kThreads) {
        const size_t at = (size_t)s * H + h;
        if (hyp[at * 2 + 1].w != 0.f) {
            const unsigned long long key = ((unsigned long long)(counts[at] + 1) << 12) | (unsigned long long)(kPlaneMaxTrials - 1 - h);
            best = key > best ? key : best;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, HP_WAVE);
        best = other > best ? other : best;
    }
    if ((tid & (HP_WAVE - 1)) == 0) part[tid >> 6] = best;
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < kThreads / HP_WAVE; ++w) best = part[w] > best ? part[w] : best;
    const long long lo = offsets[s], len = offsets[s + 1] - lo;
    const float nan = __int_as_float(kNanBits);
    int h = -1, count = 0, rows[3] = {-1, -1, -1};
    float plane[4] = {nan, nan, nan, nan};
    if (best) {                                            // a valid trial: 3 <= len <= kScanMaxPoints
        h = kPlaneMaxTrials - 1 - (int)(best & (unsigned long long)(kPlaneMaxTrials - 1));
        count = (int)(best >> 12) - 1;
        const uint2 key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)), stream = stream_of(streams, s);
        for (int k = 0; k < 3; ++k) rows[k] = sample_row(key, stream, h, k, (int)len, kTagPlane);
        const float4 A = hyp[((size_t)s * H + h) * 2], B = hyp[((size_t)s * H + h) * 2 + 1];
        plane[0] = A.w;
        plane[1] = B.x;
        plane[2] = B.y;
        plane[3] = -__fadd_rn(__fadd_rn(__fmul_rn(A.w, A.x), __fmul_rn(B.x, A.y)), __fmul_rn(B.y, A.z));
    }
    trial[s] = h;
    inliers[s] = count;
    found[s] = h >= 0 && count >= min_inliers && (double)count >= __dmul_rn((double)min_share, (double)len);
    for (int k = 0; k < 3; ++k) sample[s * 3 + k] = rows[k];
    for (int k = 0; k < 4; ++k) sample_plane[s * 4 + k] = plane[k];
    moments[(size_t)s * 10] = count;
    for (int k = 1; k < 10; ++k) moments[(size_t)s * 10 + k] = 0;
    shift[s] = 0;
    maxbits[s] = 0u;
}

__global__ __launch_bounds__(kThreads) void plane_mask_kernel(int S, int H, const float* __restrict__ points,
                                                              const long long* __restrict__ offsets, const float4* __restrict__ hyp,
                                                              const int* __restrict__ trial, unsigned char* __restrict__ inlier,
                                                              unsigned* __restrict__ maxbits) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const long long T0 = offsets[0], T1 = offsets[S];
    for (long long row0 = T0 + (long long)blockIdx.x * kPassChunk; row0 < T1; row0 += (long long)gridDim.x * kPassChunk) {
        const long long end = row0 + kPassChunk < T1 ? row0 + kPassChunk : T1;
        for (int s = scan_of(offsets, S, row0); s < S && offsets[s] < end; ++s) {
            const long long b0 = offsets[s] > row0 ? offsets[s] : row0, b1 = offsets[s + 1] < end ? offsets[s + 1] : end;
            const int tr = trial[s];
            if (tr < 0) {
                for (long long g = b0 + tid; g < b1; g += kThreads) inlier[g] = 0;
                continue;
            }
            const float4 A = hyp[((size_t)s * H + tr) * 2], B = hyp[((size_t)s * H + tr) * 2 + 1];
            float m = 0.f;
            for (long long g = b0 + tid; g < b1; g += kThreads) {
                const float x = points[g * 3], y = points[g * 3 + 1], z = points[g * 3 + 2];
                const float e = plane_e(A, B, x, y, z);
                const bool hit = finite_bits(x) && finite_bits(y) && finite_bits(z) && __fmul_rn(e, e) <= B.z;
                inlier[g] = hit;
                if (hit)                                   // an inlier's differences are finite: e would not be otherwise
                    m = fmaxf(m, fmaxf(fabsf(__fsub_rn(x, A.x)), fmaxf(fabsf(__fsub_rn(y, A.y)), fabsf(__fsub_rn(z, A.z)))));
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, HP_WAVE));
            // the bits of non-negative floats order as integers
            if ((tid & (HP_WAVE - 1)) == 0 && m > 0.f) atomicMax(&maxbits[s], (unsigned)__float_as_int(m));
        }
    }
}

__global__ __launch_bounds__(kThreads) void plane_moments_kernel(int S, int H, const float* __restrict__ points,
                                                                 const long long* __restrict__ offsets,
                                                                 const float4* __restrict__ hyp, const int* __restrict__ trial,
                                                                 const unsigned char* __restrict__ inlier,
                                                                 const unsigned* __restrict__ maxbits,
                                                                 long long* __restrict__ moments, int* __restrict__ shift) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const long long T0 = offsets[0], T1 = offsets[S];
    for (long long row0 = T0 + (long long)blockIdx.x * kPassChunk; row0 < T1; row0 += (long long)gridDim.x * kPassChunk) {
        const long long end = row0 + kPassChunk < T1 ? row0 + kPassChunk : T1;
        for (int s = scan_of(offsets, S, row0); s < S && offsets[s] < end; ++s) {
            const long long b0 = offsets[s] > row0 ? offsets[s] : row0, b1 = offsets[s + 1] < end ? offsets[s + 1] : end;
            const int tr = trial[s];
            const unsigned mb = maxbits[s];
            if (tr < 0 || mb == 0u || b1 <= b0) continue;  // no plane, or every inlier sits on the sample row: the sums are 0
            const int e = (int)((mb >> 23) & 0xFFu) - 127;
            if (b0 == offsets[s] && tid == 0) shift[s] = e; // the workgroup that holds the scan's first row
            const float4 A = hyp[((size_t)s * H + tr) * 2];
            long long sum[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (long long g = b0 + tid; g < b1; g += kThreads) {
                if (!inlier[g]) continue;
                const long long qx = (int)ldexpf(__fsub_rn(points[g * 3], A.x), 19 - e);       // exact, |q| < 2^20; the cast truncates
                const long long qy = (int)ldexpf(__fsub_rn(points[g * 3 + 1], A.y), 19 - e);
                const long long qz = (int)ldexpf(__fsub_rn(points[g * 3 + 2], A.z), 19 - e);
                sum[0] += qx;
                sum[1] += qy;
                sum[2] += qz;
                sum[3] += qx * qx;
                sum[4] += qx * qy;
                sum[5] += qx * qz;
                sum[6] += qy * qy;
                sum[7] += qy * qz;
                sum[8] += qz * qz;
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                long long v = sum[k];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, HP_WAVE);
                // two's complement: the unsigned add is the signed one
                if ((tid & (HP_WAVE - 1)) == 0 && v != 0)
                    atomicAdd(reinterpret_cast<unsigned long long*>(moments + (size_t)s * 10 + 1 + k), (unsigned long long)v);
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void plane_side_kernel(int S, const float* __restrict__ points,
                                                              const long long* __restrict__ offsets, const float* __restrict__ planes,
                                                              float threshold, float* __restrict__ dist,
                                                              unsigned char* __restrict__ keep, int* __restrict__ kept) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const long long T0 = offsets[0], T1 = offsets[S];
    for (long long row0 = T0 + (long long)blockIdx.x * kPassChunk; row0 < T1; row0 += (long long)gridDim.x * kPassChunk) {
        const long long end = row0 + kPassChunk < T1 ? row0 + kPassChunk : T1;
        for (int s = scan_of(offsets, S, row0); s < S && offsets[s] < end; ++s) {
            const long long b0 = offsets[s] > row0 ? offsets[s] : row0, b1 = offsets[s + 1] < end ? offsets[s + 1] : end;
            const float nx = planes[s * 4], ny = planes[s * 4 + 1], nz = planes[s * 4 + 2], d0 = planes[s * 4 + 3];
            int c = 0;
            for (long long g = b0 + tid; g < b1; g += kThreads) {
                const float x = points[g * 3], y = points[g * 3 + 1], z = points[g * 3 + 2];
                const bool present = finite_bits(x) && finite_bits(y) && finite_bits(z);
                float d = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(nx, x), __fmul_rn(ny, y)), __fmul_rn(nz, z)), d0);
                if (!present || d != d) d = __int_as_float(kNanBits);      // one NaN: the quiet one with no payload
                const bool k = present && !(fabsf(d) <= threshold);
                dist[g] = d;
                keep[g] = k;
                c += k;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, HP_WAVE);
            if ((tid & (HP_WAVE - 1)) == 0 && c) atomicAdd(&kept[s], c);
        }
    }
}

bool threshold_ok(float threshold) {
    if (!(threshold >= 0.f)) return false;                 // refuses a NaN too
    return threshold * threshold <= 3.4028234664e38f;      // a finite square
}

constexpr size_t kHypBytes = 8 * sizeof(float);

}  // namespace

// The geometry of hp_scan_plane: threads per workgroup, rows a lane of the consensus kernel holds (a workgroup covers
// threads * rows_per_lane consecutive rows of the ragged set) and hypotheses per LDS tile.  Host only.
HP_API int hp_scan_plane_plan(int trials, int* threads, int* rows_per_lane, int* trial_tile) {
    HP_CHECK_ARG(trials >= 1 && trials <= kPlaneMaxTrials && threads && rows_per_lane && trial_tile);
    *threads = kThreads;
    *rows_per_lane = kRowsPerLane;
    *trial_tile = kTrialTile;
    return 0;
}

// Bytes of hp_scan_plane's workspace: the hypotheses (S,H,8) fp32, the counts (S,H) int32, the maxima (S) uint32.  Host only.
HP_API long hp_scan_plane_workspace_bytes(int S, int trials) {
    if (S < 1 || trials < 1 || trials > kPlaneMaxTrials) return -1;
    const size_t sh = (size_t)S * trials;
    return (long)((sh * (kHypBytes + sizeof(int)) + (size_t)S * sizeof(unsigned) + 15) / 16 * 16);
}

// The dominant plane of each of S ragged scans by sample consensus; the law is in include/hyperpocket_hip.h.
HP_API int hp_scan_plane(int S, const float* points, const long long* offsets, const long long* streams, unsigned long long seed,
                         int trials, float threshold, int min_inliers, float min_share, int* trial, int* inliers, int* found,
                         int* sample, float* sample_plane, unsigned char* inlier, long long* moments, int* shift, void* ws,
                         hipStream_t stream) {
    HP_CHECK_ARG(S >= 1 && points && offsets && trial && inliers && found && sample && sample_plane && inlier && moments && shift && ws);
    HP_CHECK_ARG(trials >= 1 && trials <= kPlaneMaxTrials && min_inliers >= 3);
    HP_CHECK_ARG(min_share >= 0.f && min_share <= 1.f);    // refuses a NaN too
    HP_CHECK_ARG(threshold_ok(threshold));
    const float t2 = threshold * threshold;
    const size_t sh = (size_t)S * trials;
    float4* hyp = static_cast<float4*>(ws);
    int* counts = reinterpret_cast<int*>(static_cast<char*>(ws) + sh * kHypBytes);
    unsigned* maxbits = reinterpret_cast<unsigned*>(counts + sh);
    hipLaunchKernelGGL(plane_hypotheses_kernel, dim3(S, (trials + kThreads - 1) / kThreads), dim3(kThreads), 0, stream, trials,
                       points, offsets, streams, seed, t2, hyp, counts);
    hipLaunchKernelGGL(plane_consensus_kernel, dim3(kGrid), dim3(kThreads), 0, stream, S, trials, points, offsets, hyp, counts);
    hipLaunchKernelGGL(plane_winner_kernel, dim3(S), dim3(kThreads), 0, stream, trials, points, offsets, streams, seed, min_inliers,
                       min_share, hyp, counts, trial, inliers, found, sample, sample_plane, moments, shift, maxbits);
    hipLaunchKernelGGL(plane_mask_kernel, dim3(kGrid), dim3(kThreads), 0, stream, S, trials, points, offsets, hyp, trial, inlier,
                       maxbits);
    hipLaunchKernelGGL(plane_moments_kernel, dim3(kGrid), dim3(kThreads), 0, stream, S, trials, points, offsets, hyp, trial, inlier,
                       maxbits, moments, shift);
    HP_RETURN_LAST_ERROR();
}

// Rows against given planes (S,4): dist (T), keep (T), kept (S); the law is in include/hyperpocket_hip.h.
HP_API int hp_scan_plane_side(int S, const float* points, const long long* offsets, const float* planes, float threshold,
                              float* dist, unsigned char* keep, int* kept, hipStream_t stream) {
    HP_CHECK_ARG(S >= 1 && points && offsets && planes && dist && keep && kept);
    HP_CHECK_ARG(threshold_ok(threshold));
    const hipError_t err = hipMemsetAsync(kept, 0, (size_t)S * sizeof(int), stream);
    if (err != hipSuccess) return (int)err;
    hipLaunchKernelGGL(plane_side_kernel, dim3(kGrid), dim3(kThreads), 0, stream, S, points, offsets, planes, threshold, dist, keep,
                       kept);
    HP_RETURN_LAST_ERROR();
}
