// Visibility of ragged scans from their sensor positions: a depth buffer of every scan on a gnomonic cube map
// about its viewpoint, and a test of rows — the scan's own, or a second ragged set's — against it.  What turns a complete cloud
// into the self-occluded view a sensor would record, and what tells a completion that fills the sensor's free space from one
// that stays behind the recorded surface.
//
// The law, per scan (include/hyperpocket_hip.h and tests/visibility_law.py have it in full; every operation is one fp64 rounding):
//   d = double(p) - double(v), a = |d|, m = the largest a (ties to the lowest axis), face = 2m + (d_m < 0),
//   u = d[(m+1)%3] / a_m, t = d[(m+2)%3] / a_m, iu = min(R-1, int(floor((u + 1) * (0.5 R)))), `it` likewise, z = float(a_m);
//   key = bits(z) << 32 | row within the scan; a pixel holds the smallest key, all ones when empty.
//   A query with depth z0 looks at the pixels within w of its own, on its face: tol = margin + (z0 * pitch) * (max(|dx|,|dy|) + 1);
//   3 without a pixel, 2 when some zz + tol < z0, 0 when every zz - tol > z0, 1 otherwise; 4 for a non-finite row, 1 at the viewpoint.
//
// The workspace holds S * 6 * R^2 keys, laid out (scan, face, it, iu): a caller may read it as the scan's range image.
//   memset   the used part to 0xFF: every pixel empty.
//   scatter  one lane per row: atomicMin of the key into the row's pixel.  A min commutes, so the buffer does not depend on the
//            order the rows arrive in; a lane first looks at the pixel and leaves it alone when it already holds a smaller key —
//            a pixel's value only ever falls, so what the lane saw can only have been too large.
//   classify one lane per query: (2w+1)^2 plain loads at most (the launch boundary made the buffer visible), label and winner.
// Integer atomics only, no float atomic and no compare-and-swap; every loop is bounded by the rows, the scans or the window.
#include "hp_common.h"

namespace {

using hp::finite_bits, hp::scan_of;
constexpr int kScanMaxPoints = 1 << 22;    // = HP_SCAN_MAX_POINTS (include/hyperpocket_hip.h): a row fits the key's low word
constexpr int kMinResolution = 4;          // = HP_VISIBILITY_MIN_RESOLUTION
constexpr int kMaxResolution = 1024;       // = HP_VISIBILITY_MAX_RESOLUTION
constexpr int kMaxWindow = 4;              // = HP_VISIBILITY_MAX_WINDOW
constexpr int kThreads = 256;              // 4 waves per workgroup
constexpr int kRowsPerLane = 4;            // a workgroup covers kThreads * kRowsPerLane consecutive rows of the ragged set
constexpr int kChunk = kThreads * kRowsPerLane;
constexpr int kGrid = 2048;                // workgroups at most: 8 per compute unit, each strides over the chunks
constexpr unsigned long long kEmpty = ~0ull;

enum { kSeenThrough = 0, kOnSurface = 1, kHidden = 2, kUnobserved = 3, kAbsent = 4 };
enum { kNoRow = 0, kAtViewpoint = 1, kProjected = 2 };

struct View {
    bool finite;
    double x, y, z;
};

__device__ __forceinline__ View view_of(const float* __restrict__ viewpoints, int s) {
    const float x = viewpoints[s * 3], y = viewpoints[s * 3 + 1], z = viewpoints[s * 3 + 2];
    return {finite_bits(x) && finite_bits(y) && finite_bits(z), (double)x, (double)y, (double)z};
}

// The pixel of a component pair: min(R - 1, int(floor((c / am + 1) * half))).  |c| <= am, so the quotient lies in [-1, 1] and
// the product in [0, R].
__device__ __forceinline__ int pixel_of(double c, double am, double half, int R) {
    const int i = (int)floor(__dmul_rn(__dadd_rn(__ddiv_rn(c, am), 1.0), half));
    return i < R - 1 ? i : R - 1;
}

// Row g of `rows` under the law: kNoRow (a non-finite coordinate), kAtViewpoint or kProjected with the face, the pixel and
// the bits of the depth.
__device__ __forceinline__ int project(const float* __restrict__ rows, long long g, View v, int R, int& face, int& it, int& iu,
                                       unsigned& zbits) {
#pragma clang fp contract(off)
    const float px = rows[g * 3], py = rows[g * 3 + 1], pz = rows[g * 3 + 2];
    if (!(v.finite && finite_bits(px) && finite_bits(py) && finite_bits(pz))) return kNoRow;
    const double d[3] = {__dsub_rn((double)px, v.x), __dsub_rn((double)py, v.y), __dsub_rn((double)pz, v.z)};
    const double ax = fabs(d[0]), ay = fabs(d[1]), az = fabs(d[2]);
    const int m = ax >= ay ? (ax >= az ? 0 : 2) : (ay >= az ? 1 : 2);          // equal maxima: the lowest axis
    const double dm = m == 0 ? d[0] : m == 1 ? d[1] : d[2];
    const double du = m == 0 ? d[1] : m == 1 ? d[2] : d[0];
    const double dt = m == 0 ? d[2] : m == 1 ? d[0] : d[1];
    const double am = fabs(dm);
    if (!(am > 0.0)) return kAtViewpoint;
    const double half = 0.5 * (double)R;                                       // exact
    face = 2 * m + (dm < 0.0);
    iu = pixel_of(du, am, half, R);
    it = pixel_of(dt, am, half, R);
    zbits = (unsigned)__float_as_int(__double2float_rn(am));                   // z > 0 or +inf: its bits order as integers
    return kProjected;
}

// What a scan needs to own a buffer with pixels in it: its rows inside [0, T) and a length the key has room for.
__device__ __forceinline__ bool scan_ok(long long lo, long long hi, long long T) {
    return lo >= 0 && hi > lo && hi <= T && hi - lo <= kScanMaxPoints;
}

__global__ __launch_bounds__(kThreads) void visibility_scatter_kernel(int S, long long T, const float* __restrict__ points,
                                                                      const long long* __restrict__ offsets,
                                                                      const float* __restrict__ viewpoints, int R,
                                                                      unsigned long long* __restrict__ buffer) {
    const int tid = threadIdx.x;
    const size_t per_scan = (size_t)6 * R * R;
    for (long long row0 = (long long)blockIdx.x * kChunk; row0 < T; row0 += (long long)gridDim.x * kChunk) {
        const long long end = row0 + kChunk < T ? row0 + kChunk : T;
        // every value that steers these loops is uniform over the workgroup
        for (int s = scan_of(offsets, S, row0); s < S && offsets[s] < end; ++s) {
            const long long lo = offsets[s], hi = offsets[s + 1];
            if (!scan_ok(lo, hi, T)) continue;
            const long long b0 = lo > row0 ? lo : row0, b1 = hi < end ? hi : end;      // inside the chunk, whatever the offsets
            const View v = view_of(viewpoints, s);
            unsigned long long* pixels = buffer + (size_t)s * per_scan;
            for (long long g = b0 + tid; g < b1; g += kThreads) {
                int face = 0, it = 0, iu = 0;
                unsigned zbits = 0;
                if (project(points, g, v, R, face, it, iu, zbits) != kProjected) continue;
                const unsigned long long key = (unsigned long long)zbits << 32 | (unsigned long long)(g - lo);
                unsigned long long* p = pixels + ((size_t)face * R + it) * R + iu;     // face < 6, it and iu < R
                if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(p, key);
            }
        }
    }
}

// The label of a projected query against its scan's pixels.
__device__ __forceinline__ int classify(const unsigned long long* __restrict__ pixels, int R, int w, double margin, double pitch,
                                        int face, int it, int iu, unsigned zbits) {
#pragma clang fp contract(off)
    const double z0 = (double)__int_as_float((int)zbits);
    const double slant = __dmul_rn(z0, pitch);
    const unsigned long long* plane = pixels + (size_t)face * R * R;
    bool any = false, hidden = false, all_behind = true;
    for (int dy = -w; dy <= w; ++dy) {
        const int y = it + dy;
        if (y < 0 || y >= R) continue;
        for (int dx = -w; dx <= w; ++dx) {
            const int x = iu + dx;
            if (x < 0 || x >= R) continue;
            const unsigned long long k = plane[(size_t)y * R + x];
            if (k == kEmpty) continue;
            const int ring = (dx < 0 ? -dx : dx) > (dy < 0 ? -dy : dy) ? (dx < 0 ? -dx : dx) : (dy < 0 ? -dy : dy);
            const double zz = (double)__int_as_float((int)(unsigned)(k >> 32));
            const double tol = __dadd_rn(margin, __dmul_rn(slant, (double)(ring + 1)));
            any = true;
            hidden |= __dadd_rn(zz, tol) < z0;
            all_behind &= __dsub_rn(zz, tol) > z0;
        }
    }
    return !any ? kUnobserved : hidden ? kHidden : all_behind ? kSeenThrough : kOnSurface;
}

// own: the queries are the scans' rows (qoffsets == offsets, Q == T) and winner, where given, is written too.
__global__ __launch_bounds__(kThreads) void visibility_classify_kernel(int S, long long T, const long long* __restrict__ offsets,
                                                                       const float* __restrict__ viewpoints, int R, int w,
                                                                       double margin, double pitch, long long Q,
                                                                       const float* __restrict__ queries,
                                                                       const long long* __restrict__ qoffsets, bool own,
                                                                       const unsigned long long* __restrict__ buffer,
                                                                       unsigned char* __restrict__ label,
                                                                       unsigned char* __restrict__ winner) {
    const int tid = threadIdx.x;
    const size_t per_scan = (size_t)6 * R * R;
    for (long long row0 = (long long)blockIdx.x * kChunk; row0 < Q; row0 += (long long)gridDim.x * kChunk) {
        const long long end = row0 + kChunk < Q ? row0 + kChunk : Q;
        for (int s = scan_of(qoffsets, S, row0); s < S && qoffsets[s] < end; ++s) {
            const long long qlo = qoffsets[s], qhi = qoffsets[s + 1];
            const long long b0 = qlo > row0 ? qlo : row0, b1 = qhi < end ? qhi : end;
            const long long lo = offsets[s], hi = offsets[s + 1];
            const bool too_long = hi - lo > kScanMaxPoints;                            // no pixel was written: no answer either
            const View v = view_of(viewpoints, s);
            const unsigned long long* pixels = buffer + (size_t)s * per_scan;
            for (long long g = b0 + tid; g < b1; g += kThreads) {
                int face = 0, it = 0, iu = 0;
                unsigned zbits = 0;
                const int kind = too_long ? kNoRow : project(queries, g, v, R, face, it, iu, zbits);
                int lab = kind == kNoRow ? kAbsent : kOnSurface, win = 0;
                if (kind == kProjected) {
                    lab = classify(pixels, R, w, margin, pitch, face, it, iu, zbits);
                    if (own) {
                        const unsigned long long key = (unsigned long long)zbits << 32 | (unsigned long long)(g - qlo);
                        win = pixels[((size_t)face * R + it) * R + iu] == key;
                    }
                }
                label[g] = (unsigned char)lab;
                if (winner != nullptr) winner[g] = (unsigned char)win;
            }
        }
    }
}

inline bool resolution_ok(int R) { return R >= kMinResolution && R <= kMaxResolution; }
inline int groups_of(long long rows) { return (int)std::min<long long>((rows + kChunk - 1) / kChunk, kGrid); }

}  // namespace

// Bytes of hp_scan_visibility's workspace: S * 6 * R^2 keys of 8 bytes, a multiple of 16.  Host only; -1 on bad arguments.
HP_API long long hp_scan_visibility_workspace_bytes(int S, int R) {
    if (S < 1 || !resolution_ok(R)) return -1;
    return (long long)S * 6 * R * R * (long long)sizeof(unsigned long long);
}

// The geometry of hp_scan_visibility over T rows and Q rows to label: threads per workgroup, rows per lane, and the workgroups
// of the scatter and of the classify launch (0: the launch is not made).  Host only.
HP_API int hp_scan_visibility_plan(long long T, long long Q, int* threads, int* rows_per_lane, int* scatter_groups,
                                   int* classify_groups) {
    HP_CHECK_ARG(T >= 0 && Q >= 0 && T <= 0x7FFFFFFFll && Q <= 0x7FFFFFFFll && threads && rows_per_lane && scatter_groups &&
                 classify_groups);
    *threads = kThreads;
    *rows_per_lane = kRowsPerLane;
    *scatter_groups = groups_of(T);
    *classify_groups = groups_of(Q);
    return 0;
}

// The depth buffers of S ragged scans from their viewpoints and the labels of their rows, or of the queries, against them; the
// law is in include/hyperpocket_hip.h.
HP_API int hp_scan_visibility(int S, long long T, const float* points, const long long* offsets, const float* viewpoints, int R,
                              int w, double margin, double pitch, long long Q, const float* queries,
                              const long long* query_offsets, unsigned char* label, unsigned char* winner, void* ws,
                              long long ws_bytes, hipStream_t stream) {
    HP_CHECK_ARG(S >= 1 && T >= 0 && T <= 0x7FFFFFFFll && (points || T == 0) && offsets && viewpoints && label && ws);
    HP_CHECK_ARG(resolution_ok(R) && w >= 0 && w <= kMaxWindow);
    HP_CHECK_ARG(margin >= 0.0 && margin <= 1.7976931348623157e308 && pitch >= 0.0 && pitch <= 1.7976931348623157e308);
    const bool own = queries == nullptr;
    HP_CHECK_ARG(own ? (query_offsets == nullptr && Q == T) : (query_offsets != nullptr && Q >= 0 && Q <= 0x7FFFFFFFll && !winner));
    const long long need = hp_scan_visibility_workspace_bytes(S, R);
    HP_CHECK_ARG(ws_bytes >= need && reinterpret_cast<uintptr_t>(ws) % 16 == 0);
    hipError_t err = hipMemsetAsync(ws, 0xFF, (size_t)need, stream);
    if (err != hipSuccess) return (int)err;
    unsigned long long* buffer = static_cast<unsigned long long*>(ws);
    if (T > 0)
        hipLaunchKernelGGL(visibility_scatter_kernel, dim3(groups_of(T)), dim3(kThreads), 0, stream, S, T, points, offsets,
                           viewpoints, R, buffer);
    if (Q > 0)
        hipLaunchKernelGGL(visibility_classify_kernel, dim3(groups_of(Q)), dim3(kThreads), 0, stream, S, T, offsets, viewpoints,
                           R, w, margin, pitch, Q, own ? points : queries, own ? offsets : query_offsets, own, buffer, label,
                           winner);
    HP_RETURN_LAST_ERROR();
}
