// Farthest-point sampling: k picks out of each of B clouds in one launch — the resampling a density-biased
// scan wants in place of a uniform subset.
//
// The law, per cloud of `count` valid rows, k picks and a start row s (include/hyperpocket_hip.h has it in full):
//   d2(i, j) = ((dx*dx + dy*dy) + dz*dz), every operation one fp32 rounding, no contraction
//   pick_0 = s, mind_i = d2(i, pick_0);  pick_j = argmax_i mind_i (lowest i among equals), mind_i = min(mind_i, d2(i, pick_j))
//   radius2[j] = max_i mind_i after picks 0..j
//
//   grid (B), one workgroup per cloud.  Lane t owns rows t, t + T, .. (R of them): coordinates and running minima stay in
//   registers for all k iterations.  An iteration is: fold the newest pick into the minima, arg-max.  The arg-max runs on one
//   64-bit key per lane — high word the bits of mind (a sum of squares is never negative, so its bits order as an integer),
//   low word ~row, so one signed max gives the value and the lowest row among equals; rows at or beyond `count` hold
//   mind = -1, a negative key that loses to every valid one.  Within a wave the max goes through DPP (rows of 16) and two
//   shuffles; each wave's winning lane leaves (key, its point) in LDS, and after the iteration's only barrier every thread
//   folds the waves' records itself, so all of them know the pick and its coordinates.  Records alternate between two LDS
//   slots: a wave that runs ahead writes the other slot, and cannot write this one again before the next barrier.
//   The same arg-max is radius2[j] and pick_{j+1}.  No atomics on that path, no global scratch.
#include "hp_common.h"

namespace {

constexpr int kFpsMaxPoints = 8192;        // = HP_FPS_MAX_POINTS (include/hyperpocket_hip.h)

struct FpsPlan {
    int max_points, threads, per_lane;
};
// The instance for P is the first with P <= max_points.  Up to 8 rows per lane at 1024 threads (4 waves per SIMD share the
// distance updates); a cloud of at most 1024 rows keeps to 4 waves, whose 4 records fold faster than 16.
constexpr FpsPlan kPlans[] = {{64, 64, 1}, {256, 256, 1}, {1024, 256, 4}, {2048, 1024, 2}, {4096, 1024, 4}, {8192, 1024, 8}};
constexpr int kNumPlans = sizeof(kPlans) / sizeof(kPlans[0]);

__device__ __forceinline__ long long key_max(long long a, long long b) { return a > b ? a : b; }

template <int kCtrl>
__device__ __forceinline__ long long key_dpp(long long v) {
    const int lo = (int)(unsigned long long)v, hi = (int)((unsigned long long)v >> 32);
    const unsigned rlo = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, kCtrl, 0xF, 0xF, false);
    const unsigned rhi = (unsigned)__builtin_amdgcn_update_dpp(hi, hi, kCtrl, 0xF, 0xF, false);
    return (long long)(((unsigned long long)rhi << 32) | rlo);
}

// The wave's largest key, in every lane.
__device__ __forceinline__ long long wave_key_max(long long v) {
    v = key_max(v, key_dpp<0xB1>(v));      // quad_perm [1,0,3,2]: lane ^ 1
    v = key_max(v, key_dpp<0x4E>(v));      // quad_perm [2,3,0,1]: lane ^ 2
    v = key_max(v, key_dpp<0x141>(v));     // row_half_mirror: the other quad of each 8
    v = key_max(v, key_dpp<0x140>(v));     // row_mirror: the other half of each 16
    v = key_max(v, __shfl_xor(v, 16, HP_WAVE));
    v = key_max(v, __shfl_xor(v, 32, HP_WAVE));
    return v;
}

template <int T, int R>
__global__ __launch_bounds__(T) void farthest_points_kernel(int P, const float* __restrict__ clouds, const int* __restrict__ counts,
                                                            const int* __restrict__ start, int k, int* __restrict__ index,
                                                            float* __restrict__ radius2, int* __restrict__ failed) {
#pragma clang fp contract(off)
    constexpr int NW = T / HP_WAVE;
    __shared__ long long skey[2][NW];
    __shared__ float4 spt[2][NW];
    const int b = blockIdx.x, tid = threadIdx.x, wid = tid >> 6;
    int* I = index + (long)b * k;
    float* R2 = radius2 ? radius2 + (long)b * k : nullptr;
    const int count = counts ? counts[b] : P;
    const int s = start ? start[b] : 0;
    if (count < 1 || count > P || s < 0 || s >= count) {    // a bad item is a value: -1 / 0, and counted
        for (int j = tid; j < k; j += T) {
            I[j] = -1;
            if (R2) R2[j] = 0.f;
        }
        if (tid == 0) atomicAdd(failed, 1);
        return;
    }
    const float* C = clouds + (long)b * P * 3;
    float x[R], y[R], z[R], m[R];
#pragma unroll
    for (int e = 0; e < R; ++e) {
        const int i = tid + e * T;
        const bool own = i < count;                         // rows at or beyond count are never read
        x[e] = own ? C[i * 3] : 0.f;
        y[e] = own ? C[i * 3 + 1] : 0.f;
        z[e] = own ? C[i * 3 + 2] : 0.f;
        m[e] = own ? __int_as_float(0x7F800000) : -1.0f;
    }
    int pick = s;
    float px = C[s * 3], py = C[s * 3 + 1], pz = C[s * 3 + 2];
    for (int j = 0; j < k; ++j) {
        if (tid == 0) I[j] = pick;
        float bm = 0.f, bx = 0.f, by = 0.f, bz = 0.f;
        int bi = tid;
#pragma unroll
        for (int e = 0; e < R; ++e) {
            const float dx = __fsub_rn(x[e], px), dy = __fsub_rn(y[e], py), dz = __fsub_rn(z[e], pz);
            const float d = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
            m[e] = fminf(m[e], d);                          // -1 stays -1
            if (e == 0 || m[e] > bm) {                      // rows ascend with e: strict > keeps the lowest row
                bm = m[e];
                bi = tid + e * T;
                bx = x[e];
                by = y[e];
                bz = z[e];
            }
        }
        const long long key = (long long)(((unsigned long long)(unsigned)__float_as_int(bm) << 32) | (unsigned)~bi);
        const long long wmax = wave_key_max(key);
        const int slot = j & 1;
        if (key == wmax) {                                  // one lane per wave: the row is part of the key
            skey[slot][wid] = key;
            spt[slot][wid] = make_float4(bx, by, bz, 0.f);
        }
        __syncthreads();
        long long best = skey[slot][0];
        int bw = 0;
#pragma unroll
        for (int w = 1; w < NW; ++w) {
            const long long other = skey[slot][w];
            if (other > best) {
                best = other;
                bw = w;
            }
        }
        const float4 p = spt[slot][bw];
        pick = (int)~(unsigned)(unsigned long long)best;
        px = p.x;
        py = p.y;
        pz = p.z;
        if (tid == 0 && R2) R2[j] = __int_as_float((int)((unsigned long long)best >> 32));
    }
}

template <int T, int R>
void launch(int B, int P, const float* clouds, const int* counts, const int* start, int k, int* index, float* radius2, int* failed,
            hipStream_t stream) {
    hipLaunchKernelGGL((farthest_points_kernel<T, R>), dim3(B), dim3(T), 0, stream, P, clouds, counts, start, k, index, radius2,
                       failed);
}

const FpsPlan* plan_for(int P) {
    for (int i = 0; i < kNumPlans; ++i)
        if (P <= kPlans[i].max_points) return &kPlans[i];
    return nullptr;
}

}  // namespace

// The instance hp_farthest_points launches for clouds of P rows: threads per workgroup and rows per lane.  Host only.
HP_API int hp_farthest_points_plan(int P, int* threads, int* points_per_lane) {
    HP_CHECK_ARG(P >= 1 && P <= kFpsMaxPoints && threads && points_per_lane);
    const FpsPlan* p = plan_for(P);
    *threads = p->threads;
    *points_per_lane = p->per_lane;
    return 0;
}

// k farthest-point picks out of each of B clouds (B,P,3): see the law at the top and include/hyperpocket_hip.h.
HP_API int hp_farthest_points(int B, int P, const float* clouds, const int* counts, const int* start, int k, int* index,
                              float* radius2, int* failed, hipStream_t stream) {
    HP_CHECK_ARG(B >= 0 && P >= 1 && P <= kFpsMaxPoints && k >= 1 && k <= kFpsMaxPoints);
    HP_CHECK_ARG(clouds && index && failed);
    if (B == 0) return 0;
    const FpsPlan* p = plan_for(P);
#define HP_FPS_CASE(T, R)                                                               \
    if (p->threads == T && p->per_lane == R) {                                          \
        launch<T, R>(B, P, clouds, counts, start, k, index, radius2, failed, stream);   \
        HP_RETURN_LAST_ERROR();                                                         \
    }
    HP_FPS_CASE(64, 1)
    HP_FPS_CASE(256, 1)
    HP_FPS_CASE(256, 4)
    HP_FPS_CASE(1024, 2)
    HP_FPS_CASE(1024, 4)
    HP_FPS_CASE(1024, 8)
#undef HP_FPS_CASE
    return -1;
}
