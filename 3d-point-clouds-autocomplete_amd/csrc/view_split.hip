// Viewpoint batch maker: one launch turns B items of a device-resident dataset into a training batch
// (existing, missing, gt) whose `existing` part is what a depth sensor at the item's viewpoint records — the near side of the
// object, the rest hidden behind it — where batch_maker.hip cuts with a random plane.  Same interface, same house rules: a numpy
// law (tests/view_split_law.py), bit-equality, integer atomics only, no failure mode that needs the host.
//
// The law, per item (include/hyperpocket_hip.h has it in full; every fp64 operation is one rounding, no contraction):
//   c_k = (Q[k,0] x + Q[k,1] y) + Q[k,2] z for the frame's rows k = 0, 1, 2; delta = dist - c_2; z = float(delta);
//   absent: a non-finite coordinate, not (delta > 0), z not finite.  Otherwise u = c_0 / delta, fu = u * scale + 0.5 R,
//   iu = int(floor(clamp(fu, 0, R - 1))), `it` likewise from c_1: a row outside the image lands in a border pixel.
//   A pixel holds the smallest bits(z) of its rows; front = the smallest word within w pixels of the row's own, inside the image;
//   o = z - float(front) in fp32 (+inf for an absent row); the `target` rows lowest in (o, row) are `existing`.
//
// One workgroup per item, the whole item on one compute unit, everything between the cloud and the outputs in LDS:
//   clear    R^2 words of all ones.
//   project  a lane per row: pixel and bits(z) into LDS, integer atomicMin of bits(z) on the row's pixel.  A min commutes: the
//            buffer does not depend on the order the rows arrive in.
//   occlude  a lane per row: (2w+1)^2 LDS reads at most; the ordered uint32 image of o replaces bits(z).
//   select   radix select of the target-th smallest key: four passes of 8 bits, most significant first, each a histogram (one
//            256-bin copy per wave) of the keys that share the prefix chosen so far; it ends with the threshold key K and the
//            number of rows with key == K still to admit, which are the first in row order.
//   write    make_batch_write_kernel's order-preserving compaction (ballot + prefix counts) and hp::out_row.
// Dynamic LDS: 4 R^2 + 6 * roundup(N, 64) bytes — 112 KiB at R = 128, N = 8192 — plus 8.1 KiB static.
#include "hp_common.h"

namespace {

using hp::finite_bits, hp::out_row;
constexpr int kViewMaxPts = 8192;          // = HP_VIEW_SPLIT_MAX_POINTS (include/hyperpocket_hip.h)
constexpr int kMinResolution = 4;          // = HP_VIEW_SPLIT_MIN_RESOLUTION
constexpr int kMaxResolution = 128;        // = HP_VIEW_SPLIT_MAX_RESOLUTION: the image is R^2 words of LDS
constexpr int kMaxWindow = 4;              // = HP_VIEW_SPLIT_MAX_WINDOW
constexpr int kThreads = 512;              // 8 waves per workgroup, two per SIMD: an item is alone on its compute unit
constexpr int kWaves = kThreads / HP_WAVE;
constexpr unsigned kEmpty = 0xFFFFFFFFu;
constexpr unsigned short kNoPixel = 0xFFFF;    // an absent row; a pixel is below 128^2
constexpr unsigned kAbsentKey = 0xFF800000u;   // ordered(+inf): above the key of every finite o

// The pixel coordinate of a ratio: int(floor(clamp((c / delta) * scale + half, 0, R - 1))).  The comparisons send a NaN to 0.
__device__ __forceinline__ int pixel_of(double c, double delta, double scale, double half, double top) {
    const double f = __dadd_rn(__dmul_rn(__ddiv_rn(c, delta), scale), half);
    const double lo = f > 0.0 ? f : 0.0;
    return (int)floor(lo < top ? lo : top);
}

// The uint32 image of an fp32 value whose integer order is the float order, for any value but a NaN (-0 counts as +0).  The law's
// o is never below +0 — the window holds the row's own pixel — but nothing here leans on that.
__device__ __forceinline__ unsigned ordered(float v) {
    const unsigned b = (unsigned)__float_as_int(v);
    if (b == 0x80000000u) return 0x80000000u;
    return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}

__device__ __forceinline__ float unordered(unsigned k) {
    return __int_as_float((int)((k & 0x80000000u) ? k & 0x7FFFFFFFu : ~k));
}

__global__ __launch_bounds__(kThreads) void view_split_kernel(int M, int N, int target, const float* __restrict__ clouds,
                                                              const int* __restrict__ ids, const float* __restrict__ frames,
                                                              const int* __restrict__ degrees, const float* __restrict__ rot,
                                                              double dist, double scale, int R, int w,
                                                              float* __restrict__ existing, float* __restrict__ missing,
                                                              float* __restrict__ gt, unsigned char* __restrict__ side,
                                                              float* __restrict__ occlusion) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned lds[];
    __shared__ int hist[kWaves * 256];
    __shared__ int wsum[kWaves];
    __shared__ int chosen[2];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int npad = (N + 63) & ~63, RR = R * R;
    unsigned* depth = lds;                                                  // R^2 words
    unsigned* keys = lds + RR;                                              // npad words: bits(z), then ordered(o)
    unsigned short* pix = reinterpret_cast<unsigned short*>(keys + npad);   // npad half-words
    float* A = existing + (long)b * target * 3;
    float* Bp = missing + (long)b * (N - target) * 3;
    float* G = gt + (long)b * N * 3;
    const int id = ids[b];
    if (id < 0 || id >= M) {                                // uniform.  No such cloud: zeros, as hp_make_batch serves it
        const float inf = __int_as_float((int)hp::kInfBits);
        for (int i = tid; i < N; i += kThreads) {
            float* o = i < target ? A + (long)i * 3 : Bp + (long)(i - target) * 3;
            o[0] = 0.f; o[1] = 0.f; o[2] = 0.f;
            G[(long)i * 3] = 0.f; G[(long)i * 3 + 1] = 0.f; G[(long)i * 3 + 2] = 0.f;
            if (side) side[(long)b * N + i] = i < target;
            if (occlusion) occlusion[(long)b * N + i] = inf;
        }
        return;
    }
    const float* P = clouds + (long)id * N * 3;
    double q[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) q[k] = (double)frames[(long)b * 9 + k];
    const double half = 0.5 * (double)R, top = (double)(R - 1);             // exact

    for (int p = tid; p < RR; p += kThreads) depth[p] = kEmpty;
    __syncthreads();

    // ---- project: pixel and depth of every row, the nearest depth of every pixel
    for (int i = tid; i < N; i += kThreads) {
        const float fx = P[i * 3], fy = P[i * 3 + 1], fz = P[i * 3 + 2];
        unsigned zb = 0;
        unsigned short px = kNoPixel;
        if (finite_bits(fx) && finite_bits(fy) && finite_bits(fz)) {
            const double x = (double)fx, y = (double)fy, z = (double)fz;
            const double c2 = __dadd_rn(__dadd_rn(__dmul_rn(q[6], x), __dmul_rn(q[7], y)), __dmul_rn(q[8], z));
            const double delta = __dsub_rn(dist, c2);
            const float zf = __double2float_rn(delta);
            if (delta > 0.0 && finite_bits(zf)) {
                const double c0 = __dadd_rn(__dadd_rn(__dmul_rn(q[0], x), __dmul_rn(q[1], y)), __dmul_rn(q[2], z));
                const double c1 = __dadd_rn(__dadd_rn(__dmul_rn(q[3], x), __dmul_rn(q[4], y)), __dmul_rn(q[5], z));
                const int iu = pixel_of(c0, delta, scale, half, top), it = pixel_of(c1, delta, scale, half, top);
                px = (unsigned short)(it * R + iu);                         // 0 <= it, iu <= R - 1 by the clamp
                zb = (unsigned)__float_as_int(zf);                          // z >= 0: its bits order as integers
                atomicMin(&depth[px], zb);
            }
        }
        keys[i] = zb;
        pix[i] = px;
    }
    __syncthreads();

    // ---- occlude: how far behind the front of its window a row lies
    for (int i = tid; i < N; i += kThreads) {
        const unsigned short px = pix[i];
        unsigned key = kAbsentKey;
        if (px != kNoPixel) {
            const int it = px / R, iu = px - it * R;
            unsigned front = kEmpty;                                        // an empty pixel is above every depth
            for (int dy = -w; dy <= w; ++dy) {
                const int y = it + dy;
                if (y < 0 || y >= R) continue;
                for (int dx = -w; dx <= w; ++dx) {
                    const int x = iu + dx;
                    if (x < 0 || x >= R) continue;
                    const unsigned v = depth[y * R + x];
                    front = v < front ? v : front;
                }
            }
            key = ordered(__fsub_rn(__int_as_float((int)keys[i]), __int_as_float((int)front)));
        }
        keys[i] = key;                                                      // a lane reads and writes its own rows only
        if (occlusion) occlusion[(long)b * N + i] = unordered(key);
    }

    // ---- select: K = the target-th smallest key, `rem` of the rows with key == K are taken
    unsigned prefix = 0;
    int rem = target;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int k = tid; k < kWaves * 256; k += kThreads) hist[k] = 0;
        __syncthreads();                                                    // also: the keys are written
        for (int i = tid; i < N; i += kThreads) {
            const unsigned k = keys[i];
            if ((unsigned)((unsigned long long)k >> (shift + 8)) == prefix) atomicAdd(&hist[wid * 256 + ((k >> shift) & 255u)], 1);
        }
        __syncthreads();
        if (wid == 0) {                                                     // lane l owns digits 4l .. 4l+3
            int c[4], sum = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                c[e] = 0;
#pragma unroll
                for (int k = 0; k < kWaves; ++k) c[e] += hist[k * 256 + lane * 4 + e];
                sum += c[e];
            }
            int inc = sum;
#pragma unroll
            for (int o = 1; o < HP_WAVE; o <<= 1) {
                const int t = __shfl_up(inc, o, HP_WAVE);
                if (lane >= o) inc += t;
            }
            int before = inc - sum;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (before < rem && rem <= before + c[e]) {                 // exactly one digit: the keys below it are all taken
                    chosen[0] = lane * 4 + e;
                    chosen[1] = before;
                }
                before += c[e];
            }
        }
        __syncthreads();
        prefix = (prefix << 8) | (unsigned)chosen[0];
        rem -= chosen[1];
    }

    // ---- write: order-preserving compaction, kThreads rows per sweep
    int deg = degrees ? degrees[b] % 360 : 0;
    if (deg < 0) deg += 360;
    const bool rotate = deg != 0;
    const float rc = rotate ? rot[deg * 2] : 1.f, rs = rotate ? rot[deg * 2 + 1] : 0.f;
    int below_seen = 0, ties_seen = 0;                      // over the rows of the sweeps so far
    for (int i0 = 0; i0 < N; i0 += kThreads) {
        const int i = i0 + tid;
        const bool valid = i < N;
        const unsigned k = valid ? keys[i] : kEmpty;
        const bool below = valid && k < prefix, tie = valid && k == prefix;
        const unsigned long long mb = __ballot(below), mt = __ballot(tie), under = (1ull << lane) - 1ull;
        __syncthreads();                                    // the previous sweep has read wsum
        if (lane == 0) wsum[wid] = __popcll(mb) | (__popcll(mt) << 16);     // at most 64 each
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int v = 0; v < kWaves; ++v) {
            if (v < wid) off += wsum[v];
            tot += wsum[v];
        }
        const int nb = below_seen + (off & 0xFFFF) + __popcll(mb & under);  // rows before i below K
        const int nt = ties_seen + (off >> 16) + __popcll(mt & under);      // rows before i equal to K
        if (valid) {
            const bool in_a = below || (tie && nt < rem);
            const int pa = nb + (nt < rem ? nt : rem);      // rows before i in `existing`: < target when in_a
            const int pb = i - pa;                          // ... and in `missing`: < N - target otherwise
            const float3 r = out_row(P[i * 3], P[i * 3 + 1], P[i * 3 + 2], rotate, rc, rs);
            float* o = in_a ? A + (long)pa * 3 : Bp + (long)pb * 3;
            if (in_a ? pa >= target : pb >= N - target) o = G + (long)i * 3;    // never, by the select: no store leaves the item
            o[0] = r.x; o[1] = r.y; o[2] = r.z;
            G[(long)i * 3] = r.x; G[(long)i * 3 + 1] = r.y; G[(long)i * 3 + 2] = r.z;
            if (side) side[(long)b * N + i] = in_a;
        }
        below_seen += tot & 0xFFFF;
        ties_seen += tot >> 16;
    }
}

inline size_t lds_bytes(int N, int R) { return (size_t)R * R * 4 + (size_t)((N + 63) & ~63) * 6; }

}  // namespace

// The geometry of hp_make_view_batch: threads per workgroup (one workgroup per item) and its bytes of dynamic LDS.  Host only.
HP_API int hp_make_view_batch_plan(int N, int R, int* threads, int* lds) {
    HP_CHECK_ARG(N >= 2 && N <= kViewMaxPts && R >= kMinResolution && R <= kMaxResolution && threads && lds);
    *threads = kThreads;
    *lds = (int)lds_bytes(N, R);
    return 0;
}

// One training batch of self-occluded views from the resident dataset `clouds` (M,N,3): the law is at the top and in
// include/hyperpocket_hip.h.
HP_API int hp_make_view_batch(int M, int N, int target, const float* clouds, int B, const int* ids, const float* frames,
                              const int* degrees, const float* rot, double dist, double scale, int R, int w, float* existing,
                              float* missing, float* gt, unsigned char* side, float* occlusion, hipStream_t stream) {
    HP_CHECK_ARG(M >= 1 && B >= 1 && B <= 65535 && N >= 2 && N <= kViewMaxPts && target > 0 && target < N);
    HP_CHECK_ARG(R >= kMinResolution && R <= kMaxResolution && w >= 0 && w <= kMaxWindow);
    HP_CHECK_ARG(dist > 0.0 && dist <= 1.7976931348623157e308 && scale > 0.0 && scale <= 1.7976931348623157e308);
    HP_CHECK_ARG(clouds && ids && frames && existing && missing && gt);
    HP_CHECK_ARG(!degrees || rot);
    const size_t lds = lds_bytes(N, R);
    if (lds > 48 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(view_split_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds);
    hipLaunchKernelGGL(view_split_kernel, dim3(B), dim3(kThreads), lds, stream, M, N, target, clouds, ids, frames, degrees, rot,
                       dist, scale, R, w, existing, missing, gt, side, occlusion);
    HP_RETURN_LAST_ERROR();
}
