// Scan preparation: ragged partial scans (points (T,3) + offsets (S+1)) become fixed-size encoder inputs in one chip-wide
// call — the test-time resampling of the reference's datasets (utils/util.py:95-100, datasets/shapenet_3depn.py:18-49) and
// the real-scan dataset's bounding-box normalisation and its inverse (datasets/real_data.py:26-39, :56-67).
//
//   boxes    grid (S), one workgroup per scan: per-axis min / max by wave shuffles, the waves' partials through LDS; no atomics.
//   prepare  grid (B), one workgroup per item.  The index law is a pure function of (seed, streams[b], n, target, replace):
//            Philox4x32-10, key = seed, counter (stream_lo, stream_hi, q, tag); word i of a tag is lane i & 3 of block i >> 2;
//            key_i = word i of tag 0, draw_j = (word j of tag 1 * n) >> 32.
//              n <= target            0..n-1, then draw_0 .. draw_{target-n-1}
//              n >  target, replace   draw_0 .. draw_{target-1}
//              n >  target, subset    the `target` points with the smallest (key_i, i), in ascending i
//            The subset is a radix select on the 32-bit keys — four passes of 8 bits, most significant first, each a
//            histogram (one 256-bin copy per wave in LDS) of the keys that share the prefix chosen so far — which ends with
//            the threshold key K and the number of keys equal to K still to admit; then one order-preserving sweep writes
//            every i with key_i < K and the first admitted ones with key_i == K.  Up to kLdsKeys points the keys are drawn
//            once and kept in LDS, above that each of the five sweeps draws them again; both read the same words.
//   restore  elementwise (c / s_scale) * scale + center.
//
// Every value a test pins comes from explicit single-rounding operations.
#include "hp_common.h"
#include "hp_philox.h"

namespace {

constexpr int kScanMaxPoints = 1 << 22;    // = HP_SCAN_MAX_POINTS (include/hyperpocket_hip.h)
constexpr int kScanMaxTarget = 8192;
constexpr int kThreads = 256;              // 4 waves per workgroup
constexpr int kWaves = kThreads / HP_WAVE;
constexpr int kLdsKeys = 8192;             // keys of a scan of at most this many points stay in LDS (32 KiB)
constexpr int kTagKey = 0, kTagDraw = 1;

__device__ __forceinline__ uint4 word_block(uint2 key, uint2 stream, uint32_t q, uint32_t tag) {
    return philox4x32_10(make_uint4(stream.x, stream.y, q, tag), key);
}

__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
#pragma unroll
    for (int o = 1; o < HP_WAVE; o <<= 1) {
        const int t = __shfl_up(v, o, HP_WAVE);
        if (lane >= o) v += t;
    }
    return v;
}

// Exclusive prefix of v in thread order over the workgroup, the workgroup's sum in `total`.  wsum: kWaves ints of LDS.
__device__ __forceinline__ int block_exclusive_scan(int v, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int inc = wave_inclusive_scan(v, lane);
    if (lane == HP_WAVE - 1) wsum[wid] = inc;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        if (w < wid) off += wsum[w];
        tot += wsum[w];
    }
    __syncthreads();
    total = tot;
    return off + inc - v;
}

__device__ __forceinline__ float wave_min_all(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, HP_WAVE));
    return v;
}

__device__ __forceinline__ float wave_max_all(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, HP_WAVE));
    return v;
}

// real_data.py:26-33 on float32: center = (max + min) / 2 per axis, scale = max over the axes of (max - min), / 0.9f
__global__ __launch_bounds__(kThreads) void scan_boxes_kernel(int S, const float* __restrict__ points,
                                                              const long long* __restrict__ offsets, float* __restrict__ center,
                                                              float* __restrict__ scale) {
#pragma clang fp contract(off)
    __shared__ float part[kWaves][6];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const long long lo = offsets[s], n = offsets[s + 1] - lo;
    const float* P = points + lo * 3;
    const float inf = __int_as_float(0x7F800000);
    float mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
    for (long long i = tid; i < n; i += kThreads) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = P[i * 3 + a];
            mn[a] = fminf(mn[a], v);
            mx[a] = fmaxf(mx[a], v);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        mn[a] = wave_min_all(mn[a]);
        mx[a] = wave_max_all(mx[a]);
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            part[wid][a] = mn[a];
            part[wid][3 + a] = mx[a];
        }
    }
    __syncthreads();
    if (tid == 0) {
        const float nan = __int_as_float(0x7FC00000);
        float ext = 0.f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            float lo_a = part[0][a], hi_a = part[0][3 + a];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) {
                lo_a = fminf(lo_a, part[w][a]);
                hi_a = fmaxf(hi_a, part[w][3 + a]);
            }
            center[s * 3 + a] = n >= 1 ? __fdiv_rn(__fadd_rn(hi_a, lo_a), 2.0f) : nan;
            const float e = __fsub_rn(hi_a, lo_a);
            ext = a == 0 ? e : fmaxf(ext, e);
        }
        scale[s] = n >= 1 ? __fdiv_rn(ext, 0.9f) : nan;    // a scan without points has no box
    }
}

__global__ __launch_bounds__(kThreads) void prepare_scans_kernel(const float* __restrict__ points, const long long* __restrict__ offsets,
                                                                 int S, const int* __restrict__ ids,
                                                                 const long long* __restrict__ streams, unsigned long long seed,
                                                                 int target, int replace, const float* __restrict__ center,
                                                                 const float* __restrict__ scale, float* __restrict__ out,
                                                                 int* __restrict__ index, int* __restrict__ failed) {
    __shared__ __attribute__((aligned(16))) uint32_t skeys[kLdsKeys];
    __shared__ int hist[kWaves * 256];
    __shared__ int wsum[kWaves];
    __shared__ int chosen[2];
    const int b = blockIdx.x, tid = threadIdx.x, wid = tid >> 6;
    float* O = out + (long)b * target * 3;
    int* I = index + (long)b * target;
    const int id = ids[b];
    long long lo = 0, cnt = 0;
    if (id >= 0 && id < S) {
        lo = offsets[id];
        cnt = offsets[id + 1] - lo;
    }
    if (cnt < 1 || cnt > kScanMaxPoints) {                  // no such scan, or one outside the limits: zeros, and counted
        for (int j = tid; j < target; j += kThreads) {
            I[j] = -1;
            O[j * 3] = 0.f;
            O[j * 3 + 1] = 0.f;
            O[j * 3 + 2] = 0.f;
        }
        if (tid == 0) atomicAdd(failed, 1);
        return;
    }
    const int n = (int)cnt;
    const float* P = points + lo * 3;
    const bool normalize = center != nullptr;
    float cx = 0.f, cy = 0.f, cz = 0.f, sc = 1.f;
    if (normalize) {
        cx = center[id * 3];
        cy = center[id * 3 + 1];
        cz = center[id * 3 + 2];
        sc = scale[id];
    }
    auto put = [&](int pos, int i) {
#pragma clang fp contract(off)
        const float x = P[(long)i * 3], y = P[(long)i * 3 + 1], z = P[(long)i * 3 + 2];
        I[pos] = i;
        O[pos * 3] = normalize ? __fdiv_rn(__fsub_rn(x, cx), sc) : x;
        O[pos * 3 + 1] = normalize ? __fdiv_rn(__fsub_rn(y, cy), sc) : y;
        O[pos * 3 + 2] = normalize ? __fdiv_rn(__fsub_rn(z, cz), sc) : z;
    };
    const uint2 key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
    const unsigned long long sid = (unsigned long long)streams[b];
    const uint2 stream = make_uint2((uint32_t)sid, (uint32_t)(sid >> 32));

    if (n <= target || replace) {
        const int head = n <= target ? n : 0;               // the scan itself first, where it fits
        for (int i = tid; i < head; i += kThreads) put(i, i);
        const int nd = target - head;
        for (int q = tid; q * 4 < nd; q += kThreads) {
            const uint4 w = word_block(key, stream, (uint32_t)q, kTagDraw);
            const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (q * 4 + e < nd) put(head + q * 4 + e, (int)__umulhi(ww[e], (uint32_t)n));
        }
        return;
    }

    // ---- the `target` smallest (key_i, i) of n > target
    const int nq = (n + 3) >> 2;                            // Philox blocks that hold the n keys
    const bool in_lds = n <= kLdsKeys;
    if (in_lds) {
        for (int q = tid; q < nq; q += kThreads) reinterpret_cast<uint4*>(skeys)[q] = word_block(key, stream, (uint32_t)q, kTagKey);
    }
    auto keys_of = [&](int q) -> uint4 {
        return in_lds ? reinterpret_cast<const uint4*>(skeys)[q] : word_block(key, stream, (uint32_t)q, kTagKey);
    };
    uint32_t prefix = 0;                                    // the threshold's digits chosen so far
    int rem = target;                                       // points still to take among the keys that start with `prefix`
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) hist[k * 256 + tid] = 0;
        __syncthreads();                                    // also: skeys are written
        for (int q = tid; q < nq; q += kThreads) {
            const uint4 w = keys_of(q);
            const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool mine = q * 4 + e < n && (uint32_t)((uint64_t)ww[e] >> (shift + 8)) == prefix;
                if (mine) atomicAdd(&hist[wid * 256 + ((ww[e] >> shift) & 255u)], 1);
            }
        }
        __syncthreads();
        int c = 0, total;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) c += hist[k * 256 + tid];
        const int before = block_exclusive_scan(c, wsum, total);
        if (before < rem && rem <= before + c) {            // exactly one digit: the keys below it are all taken
            chosen[0] = tid;
            chosen[1] = before;
        }
        __syncthreads();
        prefix = (prefix << 8) | (uint32_t)chosen[0];
        rem -= chosen[1];
        __syncthreads();
    }
    // prefix = K, the largest key taken; `rem` >= 1 of the keys equal to K are taken, the first in index order.
    // Thread t of a sweep holds points 4 * (q0 + t) .. + 3, so thread order is index order.
    int taken_below = 0, ties_seen = 0;
    for (int q0 = 0; q0 < nq; q0 += kThreads) {
        const int q = q0 + tid;
        bool below[4] = {false, false, false, false}, tie[4] = {false, false, false, false};
        int packed = 0;                                     // keys below K in bits 0-15, equal to K in bits 16-31: <= 1024 each
        if (q < nq) {
            const uint4 w = keys_of(q);
            const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool valid = q * 4 + e < n;
                below[e] = valid && ww[e] < prefix;
                tie[e] = valid && ww[e] == prefix;
                packed += (int)below[e] + ((int)tie[e] << 16);
            }
        }
        int total;
        const int ex = block_exclusive_scan(packed, wsum, total);
        int nb = taken_below + (ex & 0xFFFF), nt = ties_seen + (ex >> 16);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (below[e] || (tie[e] && nt < rem)) put(nb + (nt < rem ? nt : rem), q * 4 + e);
            nb += (int)below[e];
            nt += (int)tie[e];
        }
        taken_below += total & 0xFFFF;
        ties_seen += total >> 16;
        if (taken_below + (ties_seen < rem ? ties_seen : rem) >= target) break;      // uniform: all `target` are written
    }
}

__global__ __launch_bounds__(kThreads) void restore_scans_kernel(long total, int N, const float* __restrict__ completions,
                                                                 const float* __restrict__ s_scale, const float* __restrict__ center,
                                                                 const float* __restrict__ scale, float* __restrict__ out) {
#pragma clang fp contract(off)
    const long stride = (long)gridDim.x * kThreads;
    for (long r = (long)blockIdx.x * kThreads + threadIdx.x; r < total; r += stride) {      // r: a point (k, i)
        const long k = r / N;
        const float ss = s_scale[k], sc = scale[k];
#pragma unroll
        for (int a = 0; a < 3; ++a)
            out[r * 3 + a] = __fadd_rn(__fmul_rn(__fdiv_rn(completions[r * 3 + a], ss), sc), center[k * 3 + a]);
    }
}

}  // namespace

// Bounding boxes of S ragged scans (scan s = rows offsets[s] .. offsets[s+1] of points (T,3)): center (S,3), scale (S).
HP_API int hp_scan_boxes(int S, const float* points, const long long* offsets, float* center, float* scale, hipStream_t stream) {
    HP_CHECK_ARG(S >= 1 && points && offsets && center && scale);
    hipLaunchKernelGGL(scan_boxes_kernel, dim3(S), dim3(kThreads), 0, stream, S, points, offsets, center, scale);
    HP_RETURN_LAST_ERROR();
}

// B fixed-size encoder inputs from S ragged scans: see the law at the top and include/hyperpocket_hip.h.
HP_API int hp_prepare_scans(int B, const float* points, const long long* offsets, int S, const int* ids, const long long* streams,
                            unsigned long long seed, int target, int replace, const float* center, const float* scale, float* out,
                            int* index, int* failed, hipStream_t stream) {
    HP_CHECK_ARG(B >= 1 && S >= 1 && target >= 1 && target <= kScanMaxTarget && (replace == 0 || replace == 1));
    HP_CHECK_ARG(points && offsets && ids && streams && out && index && failed);
    HP_CHECK_ARG((center == nullptr) == (scale == nullptr));
    hipLaunchKernelGGL(prepare_scans_kernel, dim3(B), dim3(kThreads), 0, stream, points, offsets, S, ids, streams, seed, target, replace,
                       center, scale, out, index, failed);
    HP_RETURN_LAST_ERROR();
}

// real_data.py:63-67 for K completions of N points: out = (c / s_scale[k]) * scale[k] + center[k].
HP_API int hp_restore_scans(int K, int N, const float* completions, const float* s_scale, const float* center, const float* scale,
                            float* out, hipStream_t stream) {
    HP_CHECK_ARG(K >= 1 && N >= 1 && completions && s_scale && center && scale && out);
    const long total = (long)K * N;
    const long blocks = (total + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(restore_scans_kernel, dim3((unsigned)std::min(blocks, 65535L * 16)), dim3(kThreads), 0, stream, total, N,
                       completions, s_scale, center, scale, out);
    HP_RETURN_LAST_ERROR();
}
