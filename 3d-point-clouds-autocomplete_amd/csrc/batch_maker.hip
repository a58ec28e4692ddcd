// Batch maker: one chip-wide call turns B items of a device-resident dataset into a training batch
// (existing, missing, gt) — the reference's random-plane slicing law (datasets/utils/dataset_generator.py:6-39) and its
// z-rotation augmentation (datasets/shapenet.py:73-92), with no host synchronisation.
//
//   search     grid (groups, B), 4 waves per workgroup.  Candidate c of item b is a pure function of (seed, streams[b], c):
//              three Philox4x32-10 blocks -> three U[0,1)^3 points -> normal = cross product, bias = +dot(normal, p0).
//              A wave owns whole candidates: its lanes hold the cloud (registers up to 2048 points, LDS above), it draws 64
//              candidate planes at once (one per lane) and then counts each against the cloud with wave ballots.  An
//              accepting candidate does an integer atomicMin on the item's slot; a wave stops once its next candidate is
//              above that minimum, so the final minimum is the first accepted candidate of the sequence whatever the schedule.
//   write-out  grid (B): recomputes the accepted plane from its number, recounts, compacts order-preservingly and rotates.
//
// The search and the write-out classify through the same two functions (candidate_plane, under) built from explicit
// single-rounding operations, so a point is on the same side of a candidate in both.
#include "hp_common.h"
#include "hp_philox.h"

namespace {

using hp::out_row;
constexpr int kMakeMaxPts = 8192;          // = kSliceMaxPts (aux_kernels.hip)
constexpr int kWaves = 4;                  // waves per workgroup
constexpr int kChunk = kWaves * HP_WAVE;   // candidates per chunk: chunk q belongs to group q mod groups, 64 per wave
constexpr int kCheckEvery = 16;            // candidates between two looks at the item's minimum
constexpr unsigned kNone = 0xFFFFFFFFu;    // slot value "nothing accepted yet" (the memset pattern)

struct Plane {
    float nx, ny, nz, bias;
};

// candidate c of the stream: points p0, p1, p2 from Philox blocks k = 0, 1, 2 with counter (stream_lo, stream_hi, c, k)
__device__ __forceinline__ Plane candidate_plane(uint2 key, uint2 stream, uint32_t c) {
#pragma clang fp contract(off)
    const uint4 r0 = philox4x32_10(make_uint4(stream.x, stream.y, c, 0u), key);
    const uint4 r1 = philox4x32_10(make_uint4(stream.x, stream.y, c, 1u), key);
    const uint4 r2 = philox4x32_10(make_uint4(stream.x, stream.y, c, 2u), key);
    constexpr float k2m24 = 1.0f / 16777216.0f;                         // (x >> 8) * 2^-24: exact
    const float p0x = __fmul_rn((float)(r0.x >> 8), k2m24), p0y = __fmul_rn((float)(r0.y >> 8), k2m24),
                p0z = __fmul_rn((float)(r0.z >> 8), k2m24);
    const float ux = __fadd_rn(__fmul_rn((float)(r1.x >> 8), k2m24), -p0x), uy = __fadd_rn(__fmul_rn((float)(r1.y >> 8), k2m24), -p0y),
                uz = __fadd_rn(__fmul_rn((float)(r1.z >> 8), k2m24), -p0z);
    const float vx = __fadd_rn(__fmul_rn((float)(r2.x >> 8), k2m24), -p0x), vy = __fadd_rn(__fmul_rn((float)(r2.y >> 8), k2m24), -p0y),
                vz = __fadd_rn(__fmul_rn((float)(r2.z >> 8), k2m24), -p0z);
    Plane p;
    p.nx = __fmaf_rn(uy, vz, -__fmul_rn(uz, vy));
    p.ny = __fmaf_rn(uz, vx, -__fmul_rn(ux, vz));
    p.nz = __fmaf_rn(ux, vy, -__fmul_rn(uy, vx));
    p.bias = __fmaf_rn(p.nz, p0z, __fmaf_rn(p.ny, p0y, __fmul_rn(p.nx, p0x)));   // HyperPlane(cp, np.dot(cp, points[0]))
    return p;
}

// HyperPlane.check_point's `> 0` (NaN compares false: a NaN pad point is never under)
__device__ __forceinline__ bool under(float x, float y, float z, const Plane& p) {
#pragma clang fp contract(off)
    return __fmaf_rn(z, p.nz, __fmaf_rn(y, p.ny, __fmaf_rn(x, p.nx, p.bias))) > 0.f;
}

__device__ __forceinline__ Plane lane_plane(const Plane& p, int k) {   // lane k's plane, wave-uniform
    Plane q;
    q.nx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p.nx), k));
    q.ny = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p.ny), k));
    q.nz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p.nz), k));
    q.bias = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p.bias), k));
    return q;
}

// PPL > 0: each lane keeps points lane, lane + 64, ... (PPL of them) in registers and tests one candidate per pass.
// PPL == 0: the workgroup stages the cloud in LDS (x[], y[], z[] planes: consecutive lanes, consecutive banks) and a wave tests
// four candidates per pass over it, so the LDS reads are a quarter of the tests.
template <int PPL>
__global__ __launch_bounds__(kWaves* HP_WAVE) void make_batch_search_kernel(int M, int N, int target, const float* __restrict__ clouds,
                                                                            const int* __restrict__ ids,
                                                                            const long long* __restrict__ streams,
                                                                            unsigned long long seed, int max_candidates,
                                                                            unsigned* __restrict__ slots) {
    constexpr int KC = PPL > 0 ? 1 : 4;
    extern __shared__ __attribute__((aligned(16))) float sp[];
    const int b = blockIdx.y, g = blockIdx.x, groups = gridDim.x;
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int id = ids[b];
    if (id < 0 || id >= M) return;                       // the write-out reports it
    const float* P = clouds + (long)id * N * 3;
    const float nan = __int_as_float(0x7FC00000);
    const int npad = (N + 63) & ~63;
    float px[PPL > 0 ? PPL : 1], py[PPL > 0 ? PPL : 1], pz[PPL > 0 ? PPL : 1];
    if constexpr (PPL > 0) {
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
            const int i = j * 64 + lane;
            const bool v = i < N;
            px[j] = v ? P[i * 3] : nan;
            py[j] = v ? P[i * 3 + 1] : nan;
            pz[j] = v ? P[i * 3 + 2] : nan;
        }
    } else {
        for (int i = threadIdx.x; i < npad; i += kWaves * HP_WAVE) {
            const bool v = i < N;
            sp[i] = v ? P[i * 3] : nan;
            sp[npad + i] = v ? P[i * 3 + 1] : nan;
            sp[2 * npad + i] = v ? P[i * 3 + 2] : nan;
        }
        __syncthreads();                                  // the only barrier: the waves go their own way from here
    }
    const uint2 key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
    const unsigned long long sid = (unsigned long long)streams[b];
    const uint2 stream = make_uint2((uint32_t)sid, (uint32_t)(sid >> 32));
    unsigned* slot = slots + b;
    for (long q = g;; q += groups) {
        const long c0 = q * kChunk + wid * HP_WAVE;       // this wave's first candidate of chunk q
        if (c0 >= max_candidates) break;
        if ((unsigned long long)c0 > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        const Plane mine = candidate_plane(key, stream, (uint32_t)(c0 + lane));
        const int nc = (int)((long)max_candidates - c0 < HP_WAVE ? (long)max_candidates - c0 : HP_WAVE);
        bool done = false;
        for (int k = 0; k < nc && !done; k += KC) {
            if (k && (k % kCheckEvery) == 0 &&
                (unsigned long long)(c0 + k) > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                done = true;
                break;
            }
            Plane pl[KC];
            int cnt[KC];
#pragma unroll
            for (int t = 0; t < KC; ++t) {
                pl[t] = lane_plane(mine, (k + t) & 63);
                cnt[t] = 0;
            }
            if constexpr (PPL > 0) {
#pragma unroll
                for (int j = 0; j < PPL; ++j) cnt[0] += __popcll(__ballot(under(px[j], py[j], pz[j], pl[0])));
            } else {
                for (int i = lane; i < npad; i += 64) {
                    const float x = sp[i], y = sp[npad + i], z = sp[2 * npad + i];
#pragma unroll
                    for (int t = 0; t < KC; ++t) cnt[t] += __popcll(__ballot(under(x, y, z, pl[t])));
                }
            }
#pragma unroll
            for (int t = 0; t < KC; ++t) {
                if (!done && k + t < nc && (cnt[t] == target || N - cnt[t] == target)) {
                    if (lane == 0) atomicMin(slot, (unsigned)(c0 + k + t));
                    done = true;                          // this wave's later candidates are all above it
                }
            }
        }
        if (done) break;
    }
}

__global__ __launch_bounds__(256) void make_batch_write_kernel(int M, int N, int target, const float* __restrict__ clouds,
                                                               const int* __restrict__ ids, const long long* __restrict__ streams,
                                                               const int* __restrict__ degrees, const float* __restrict__ rot,
                                                               unsigned long long seed, const unsigned* __restrict__ slots,
                                                               float* __restrict__ existing, float* __restrict__ missing,
                                                               float* __restrict__ gt, float* __restrict__ plane_out,
                                                               int* __restrict__ index, int* __restrict__ failed) {
    __shared__ int wsum[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int id = ids[b];
    const bool have_cloud = id >= 0 && id < M;
    const float* P = clouds + (long)(have_cloud ? id : 0) * N * 3;
    const unsigned m = slots[b];
    bool ok = have_cloud && m != kNone;
    Plane pl = {0.f, 0.f, 0.f, 0.f};
    int side = 0;                                         // +1: the "under" side has `target` points, -1: the other side
    if (ok) {
        const uint2 key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
        const unsigned long long sid = (unsigned long long)streams[b];
        pl = candidate_plane(key, make_uint2((uint32_t)sid, (uint32_t)(sid >> 32)), m);
        int cnt = 0;
        for (int i0 = 0; i0 < N; i0 += 256) {
            const int i = i0 + tid;
            cnt += __popcll(__ballot(i < N && under(P[i * 3], P[i * 3 + 1], P[i * 3 + 2], pl)));
        }
        if (lane == 0) wsum[wid] = cnt;
        __syncthreads();
        cnt = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
        side = cnt == target ? 1 : (N - cnt == target ? -1 : 0);   // the reference tests the "under" side first
        ok = side != 0;                                   // a recount that disagrees with the search: the item has failed
    }
    if (tid == 0) {
        index[b] = ok ? (int)m : -1;
        plane_out[b * 4 + 0] = ok ? pl.nx : 0.f;
        plane_out[b * 4 + 1] = ok ? pl.ny : 0.f;
        plane_out[b * 4 + 2] = ok ? pl.nz : 0.f;
        plane_out[b * 4 + 3] = ok ? pl.bias : 0.f;
        if (!ok) atomicAdd(failed, 1);
    }
    int deg = degrees ? degrees[b] % 360 : 0;
    if (deg < 0) deg += 360;
    const bool rotate = deg != 0;
    const float rc = rotate ? rot[deg * 2] : 1.f, rs = rotate ? rot[deg * 2 + 1] : 0.f;
    // order-preserving compaction, 256 points per pass (as slice_kernel); a failed item falls back to the first `target` points
    float* A = existing + (long)b * target * 3;
    float* Bp = missing + (long)b * (N - target) * 3;
    float* G = gt + (long)b * N * 3;
    int base_a = 0;
    for (int i0 = 0; i0 < N; i0 += 256) {
        const int i = i0 + tid;
        const bool valid = i < N;
        float x = 0.f, y = 0.f, z = 0.f;
        if (valid && have_cloud) {
            x = P[i * 3];
            y = P[i * 3 + 1];
            z = P[i * 3 + 2];
        }
        bool in_a = false;
        if (valid) in_a = ok ? (under(x, y, z, pl) == (side > 0)) : i < target;
        const unsigned long long mask = __ballot(in_a);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wid] = __popcll(mask);
        __syncthreads();
        int woff = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wid) woff += wsum[w];
            tot += wsum[w];
        }
        if (valid) {
            const int pa = base_a + woff + before;
            const int pb = i - pa;                        // points before i that are not in A
            const float3 r = out_row(x, y, z, rotate, rc, rs);
            float* o = in_a ? A + (long)pa * 3 : Bp + (long)pb * 3;
            o[0] = r.x; o[1] = r.y; o[2] = r.z;
            G[(long)i * 3] = r.x; G[(long)i * 3 + 1] = r.y; G[(long)i * 3 + 2] = r.z;
        }
        base_a += tot;
        __syncthreads();
    }
}

}  // namespace

// bytes of `ws` for hp_make_batch: one 32-bit slot per item (the number of its first accepted candidate)
HP_API long hp_make_batch_workspace_bytes(int B, int N) {
    if (B < 1 || N < 1 || N > kMakeMaxPts) return -1;
    return ((long)B * 4 + 255) & ~255L;
}

// One training batch from the resident dataset `clouds` (M,N,3): item b is cloud ids[b], split by the first accepted
// candidate plane of the sequence (seed, streams[b]) and rotated about z by degrees[b] (rot (360,2) = (cos, sin); degrees
// NULL: no rotation).  existing (B,target,3) = the side with `target` points, missing (B,N-target,3) the rest, gt (B,N,3) the
// whole cloud; plane (B,4), index (B) = the accepted plane and its candidate number.  An item with no accepted candidate
// below max_candidates (or an id outside [0,M)) gets index -1, adds 1 to *failed and falls back to first-`target` / rest.
HP_API int hp_make_batch(int M, int N, int target, const float* clouds, int B, const int* ids, const long long* streams,
                         const int* degrees, const float* rot, unsigned long long seed, int max_candidates, int groups,
                         float* existing, float* missing, float* gt, float* plane, int* index, int* failed, void* ws,
                         hipStream_t stream) {
    HP_CHECK_ARG(M >= 1 && B >= 1 && B <= 65535 && N > 0 && N <= kMakeMaxPts && target > 0 && target < N);
    HP_CHECK_ARG(max_candidates > 0 && groups >= 1 && groups <= 65535);
    HP_CHECK_ARG(clouds && ids && streams && existing && missing && gt && plane && index && failed && ws);
    HP_CHECK_ARG(!degrees || rot);
    unsigned* slots = static_cast<unsigned*>(ws);
    const hipError_t e = hipMemsetAsync(slots, 0xFF, (size_t)B * 4, stream);
    if (e != hipSuccess) return (int)e;
    const dim3 grid(groups, B), block(kWaves * HP_WAVE);
#define HP_SEARCH(PPL, LDS) \
    hipLaunchKernelGGL(make_batch_search_kernel<PPL>, grid, block, LDS, stream, M, N, target, clouds, ids, streams, seed, max_candidates, slots)
    if (N <= 128) HP_SEARCH(2, 0);
    else if (N <= 512) HP_SEARCH(8, 0);
    else if (N <= 2048) HP_SEARCH(32, 0);
    else {
        const size_t lds = (size_t)((N + 63) & ~63) * 3 * sizeof(float);
        if (lds > 48 * 1024)
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(make_batch_search_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lds);
        HP_SEARCH(0, lds);
    }
#undef HP_SEARCH
    hipLaunchKernelGGL(make_batch_write_kernel, dim3(B), dim3(256), 0, stream, M, N, target, clouds, ids, streams, degrees, rot, seed,
                       slots, existing, missing, gt, plane, index, failed);
    HP_RETURN_LAST_ERROR();
}
