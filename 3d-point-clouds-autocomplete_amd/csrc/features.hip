// Fast point feature histograms of ragged scans from given neighbour lists and normals, and the nearest descriptor of a second
// ragged set: what a global registration matches before it draws its trials (pose_trials.hip).
//
// The law, per scan and per row i (include/hyperpocket_hip.h and tests/feature_law.py have it in full):
//   a row is usable with finite coordinates and a finite non-zero normal; slot t is listed when 0 <= j < n_s, j != i, row j usable;
//   d = p_j - p_i in fp32, then fp64 with one rounding per operation: the end with the larger |n . d| is the source (ties: i),
//   phi = ns . d / |d|, v = (d x ns) / |d x ns|, w = ns x v, alpha = v . nt, theta = the angle of (ns . nt, w . nt); a pair with a
//   non-finite d, d = 0 or d x ns = 0 is skipped.  alpha and phi bin by floor(11 (f + 1) / 2); theta by sign tests of
//   c_k * y - s_k * x against ten tabulated directions: no library function decides a bit.
//   SPFH(i) = 33 counts and m_i, the pairs.  FPFH(i) = SPFH(i) / m_i + (sum_j (w_j / m_j) SPFH(j)) / sum_j w_j, w_j = 1 / |d|^2, over
//   the listed slots with m_j > 0 in list order; each group of 11 bins scaled to trunc(255 F_b / sum F): 36 bytes, the last 3 zero.
//
//   spfh     grid-stride over chunks of 256 consecutive rows, one lane per row, as normals.hip: the list in registers (K = 8, 16 or
//            32 at compile time), the neighbours gathered from global memory.  The 33 counters are bytes of six 64-bit words
//            (bins 0-7 and 8-10 of each feature), so no register is indexed by a value.  Writes 36 bytes a row to the workspace.
//   fpfh     the same walk; a neighbour's record is nine dwords, the 33 fp64 sums are registers.  Writes features and count.
//   match    a work item is a chunk of 512 consecutive source rows; a lane keeps 2 rows' nine dwords.  The set's target
//            descriptors pass through an LDS tile of 256 records of 12 dwords (nine of bytes, |b|^2, two spare) that every lane
//            reads at one address; |a - b|^2 = |a|^2 + |b|^2 - 2 a . b is nine 4 x 8-bit dot products, an exact integer below
//            2^22.  A target without a descriptor carries |b|^2 = 2^30, where the search starts: the strict compare never takes it,
//            and keeps the lower row of equals.
// No atomics, no float accumulation whose order could change: the outputs are a function of the inputs.
#include "hp_align.h"

namespace {

using hp::finite_bits;
constexpr int kFeatMaxK = 32;
constexpr int kThreads = 256;              // rows per chunk
constexpr int kGrid = 2048;
constexpr int kWidth = 36;                 // bytes of a record: 33 bins, m (SPFH) or 0 (FPFH), 0, 0
constexpr int kWords = kWidth / 4;
constexpr int kBins = 11;
constexpr int kMatchRows = 2;              // source rows a lane of the match keeps in registers
constexpr int kMatchChunk = kThreads * kMatchRows;
constexpr int kMatchTile = 256;            // target records per LDS tile (12 KiB)
constexpr int kNoMatch = 1 << 30;          // above every distance (33 * 255^2 < 2^22)

// (cos, sin)(-pi + 2 pi (k + 1) / 11): the ten boundaries of theta's bins = feature_law.THETA, literal for literal.
__device__ constexpr double kThetaC[10] = {-0x1.aeb8c8764f0b9p-1, -0x1.a9628d9c712b4p-2, 0x1.2375f640f44dap-3, 0x1.4f49e7f775887p-1,
                                           0x1.eb42a9bcd5058p-1,  0x1.eb42a9bcd5058p-1,  0x1.4f49e7f775887p-1, 0x1.2375f640f44dap-3,
                                           -0x1.a9628d9c712b1p-2, -0x1.aeb8c8764f0bbp-1};
__device__ constexpr double kThetaS[10] = {-0x1.14cedf8bb580dp-1, -0x1.d1bb48eee2c14p-1, -0x1.fac9e043842efp-1, -0x1.82f19bb3a28a1p-1,
                                           -0x1.207e7fd768dbcp-2, 0x1.207e7fd768dbcp-2,  0x1.82f19bb3a28a1p-1,  0x1.fac9e043842efp-1,
                                           0x1.d1bb48eee2c15p-1,  0x1.14cedf8bb580ap-1};

__device__ __forceinline__ double ddot(double a0, double a1, double a2, double b0, double b1, double b2) {
#pragma clang fp contract(off)
    return __dadd_rn(__dadd_rn(__dmul_rn(a0, b0), __dmul_rn(a1, b1)), __dmul_rn(a2, b2));
}

__device__ __forceinline__ int unit_bin(double f) {
#pragma clang fp contract(off)
    double t = floor(__ddiv_rn(__dmul_rn(11.0, __dadd_rn(f, 1.0)), 2.0));
    t = t < 0.0 ? 0.0 : t > 10.0 ? 10.0 : t;
    return (int)t;
}

__device__ __forceinline__ int theta_bin(double x, double y) {
#pragma clang fp contract(off)
    const bool up = y >= 0.0;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double c = up ? kThetaC[k + 5] : kThetaC[k], s = up ? kThetaS[k + 5] : kThetaS[k];
        cnt += __dsub_rn(__dmul_rn(c, y), __dmul_rn(s, x)) >= 0.0 ? 1 : 0;
    }
    return (x == 0.0 && y == 0.0) ? 5 : up ? 5 + cnt : cnt;
}

__device__ __forceinline__ bool usable_normal(float x, float y, float z) {
    return finite_bits(x) && finite_bits(y) && finite_bits(z) && (x != 0.f || y != 0.f || z != 0.f);
}

// The 11 byte counters of one feature: bins 0-7 in lo, 8-10 in hi.
struct Hist {
    unsigned long long lo, hi;
};
__device__ __forceinline__ void bump(Hist& h, int bin) {
    if (bin < 8) h.lo += 1ull << (8 * bin);
    else h.hi += 1ull << (8 * (bin - 8));
}
__device__ __forceinline__ unsigned hist_byte(const Hist& h, int bin) {     // bin: a compile-time value where it is called
    return bin < 8 ? (unsigned)(h.lo >> (8 * bin)) & 0xFFu : (unsigned)(h.hi >> (8 * (bin - 8))) & 0xFFu;
}

// What the row kernels share: the lane's row of the chunk, its scan s, the scan's first row lo and its length n (clamped to the
// rows that exist).  False for a lane beyond the chunk.
__device__ __forceinline__ bool locate(int S, long long T, const long long* __restrict__ offsets, long long row0, long long& row, int& s,
                                       long long& lo, long long& n) {
    const long long last = (row0 + kThreads < T ? row0 + kThreads : T) - 1;
    const int s0 = hp_align::set_of(offsets, S, row0);
    int s1 = s0;
    for (int hi = S; hi - s1 > 1;) {
        const int mid = (s1 + hi) >> 1;
        if (offsets[mid] <= last) s1 = mid;
        else hi = mid;
    }
    row = row0 + threadIdx.x;
    if (row > last) return false;
    s = s0;
    for (int hi = s1 + 1; hi - s > 1;) {
        const int mid = (s + hi) >> 1;
        if (offsets[mid] <= row) s = mid;
        else hi = mid;
    }
    lo = offsets[s];
    long long end = offsets[s + 1];
    end = end < T ? end : T;
    n = lo >= 0 && lo <= row && row < end ? end - lo : 0;     // a row of no scan lists nothing
    return true;
}

template <int K>
__device__ __forceinline__ void load_list(const int* __restrict__ index, long long row, int k, int vec, int (&idx)[K]) {
    if (vec) {
        const int4* L = reinterpret_cast<const int4*>(index + row * k);
#pragma unroll
        for (int t = 0; t < K / 4; ++t) {
            int4 v = make_int4(-1, -1, -1, -1);
            if (4 * t < k) v = L[t];
            idx[4 * t] = v.x;
            idx[4 * t + 1] = v.y;
            idx[4 * t + 2] = v.z;
            idx[4 * t + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int t = 0; t < K; ++t) idx[t] = t < k ? index[row * k + t] : -1;
    }
}

template <int K>
__global__ __launch_bounds__(kThreads) void spfh_kernel(int S, long long T, const float* __restrict__ points,
                                                        const long long* __restrict__ offsets, const float* __restrict__ normals, int k,
                                                        int vec, const int* __restrict__ index, unsigned* __restrict__ spfh) {
#pragma clang fp contract(off)
    for (long long row0 = (long long)blockIdx.x * kThreads; row0 < T; row0 += (long long)gridDim.x * kThreads) {
        long long row, lo, n;
        int s;
        if (!locate(S, T, offsets, row0, row, s, lo, n)) continue;
        const float px = points[row * 3], py = points[row * 3 + 1], pz = points[row * 3 + 2];
        const float fx = normals[row * 3], fy = normals[row * 3 + 1], fz = normals[row * 3 + 2];
        const bool good = finite_bits(px) && finite_bits(py) && finite_bits(pz) && usable_normal(fx, fy, fz);
        const double nix = fx, niy = fy, niz = fz;
        int idx[K];
        load_list<K>(index, row, k, vec, idx);
        Hist h[3] = {{0ull, 0ull}, {0ull, 0ull}, {0ull, 0ull}};
        unsigned m = 0;
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const long long j = idx[t];
            if (!(good && j >= 0 && j < n && lo + j != row)) continue;
            const float* P = points + (lo + j) * 3;
            const float* N = normals + (lo + j) * 3;
            const float qx = P[0], qy = P[1], qz = P[2], gx = N[0], gy = N[1], gz = N[2];
            if (!(finite_bits(qx) && finite_bits(qy) && finite_bits(qz) && usable_normal(gx, gy, gz))) continue;
            const float ex = __fsub_rn(qx, px), ey = __fsub_rn(qy, py), ez = __fsub_rn(qz, pz);
            if (!(finite_bits(ex) && finite_bits(ey) && finite_bits(ez))) continue;
            double dx = ex, dy = ey, dz = ez;
            const double d2 = ddot(dx, dy, dz, dx, dy, dz);
            if (d2 == 0.0) continue;
            const double njx = gx, njy = gy, njz = gz;
            const bool swap = fabs(ddot(njx, njy, njz, dx, dy, dz)) > fabs(ddot(nix, niy, niz, dx, dy, dz));
            const double sx = swap ? njx : nix, sy = swap ? njy : niy, sz = swap ? njz : niz;
            const double tx = swap ? nix : njx, ty = swap ? niy : njy, tz = swap ? niz : njz;
            dx = swap ? -dx : dx;
            dy = swap ? -dy : dy;
            dz = swap ? -dz : dz;
            const double phi = __ddiv_rn(ddot(sx, sy, sz, dx, dy, dz), __dsqrt_rn(d2));
            double vx = __dsub_rn(__dmul_rn(dy, sz), __dmul_rn(dz, sy)), vy = __dsub_rn(__dmul_rn(dz, sx), __dmul_rn(dx, sz)),
                   vz = __dsub_rn(__dmul_rn(dx, sy), __dmul_rn(dy, sx));
            const double vn = __dsqrt_rn(ddot(vx, vy, vz, vx, vy, vz));
            if (vn == 0.0) continue;
            vx = __ddiv_rn(vx, vn);
            vy = __ddiv_rn(vy, vn);
            vz = __ddiv_rn(vz, vn);
            const double wx = __dsub_rn(__dmul_rn(sy, vz), __dmul_rn(sz, vy)), wy = __dsub_rn(__dmul_rn(sz, vx), __dmul_rn(sx, vz)),
                         wz = __dsub_rn(__dmul_rn(sx, vy), __dmul_rn(sy, vx));
            const double alpha = ddot(vx, vy, vz, tx, ty, tz), y = ddot(wx, wy, wz, tx, ty, tz), x = ddot(sx, sy, sz, tx, ty, tz);
            bump(h[0], theta_bin(x, y));
            bump(h[1], unit_bin(alpha));
            bump(h[2], unit_bin(phi));
            ++m;
        }
        unsigned* out = spfh + row * kWords;
#pragma unroll
        for (int q = 0; q < kWords; ++q) {
            unsigned word = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int b = 4 * q + c;
                const unsigned byte = b < 3 * kBins ? hist_byte(h[b / kBins], b % kBins) : b == 3 * kBins ? m : 0u;
                word |= byte << (8 * c);
            }
            out[q] = word;
        }
    }
}

template <int K>
__global__ __launch_bounds__(kThreads) void fpfh_kernel(int S, long long T, const float* __restrict__ points,
                                                        const long long* __restrict__ offsets, int k, int vec,
                                                        const int* __restrict__ index, const unsigned* __restrict__ spfh,
                                                        unsigned* __restrict__ features, int* __restrict__ count) {
#pragma clang fp contract(off)
    for (long long row0 = (long long)blockIdx.x * kThreads; row0 < T; row0 += (long long)gridDim.x * kThreads) {
        long long row, lo, n;
        int s;
        if (!locate(S, T, offsets, row0, row, s, lo, n)) continue;
        unsigned own[kWords];
#pragma unroll
        for (int q = 0; q < kWords; ++q) own[q] = spfh[row * kWords + q];
        const int mi = (int)((own[kWords - 1] >> 8) & 0xFFu);
        const float px = points[row * 3], py = points[row * 3 + 1], pz = points[row * 3 + 2];
        int idx[K];
        load_list<K>(index, row, k, vec, idx);
        double A[3 * kBins];
#pragma unroll
        for (int b = 0; b < 3 * kBins; ++b) A[b] = 0.0;
        double W = 0.0;
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const long long j = idx[t];
            if (!(mi > 0 && j >= 0 && j < n && lo + j != row)) continue;
            const unsigned* R = spfh + (lo + j) * kWords;
            const int mj = (int)((R[kWords - 1] >> 8) & 0xFFu);
            if (mj == 0) continue;
            const float* P = points + (lo + j) * 3;
            const float ex = __fsub_rn(P[0], px), ey = __fsub_rn(P[1], py), ez = __fsub_rn(P[2], pz);
            if (!(finite_bits(ex) && finite_bits(ey) && finite_bits(ez))) continue;
            const double dx = ex, dy = ey, dz = ez;
            const double d2 = ddot(dx, dy, dz, dx, dy, dz);
            if (d2 == 0.0) continue;
            const double w = __ddiv_rn(1.0, d2), c = __ddiv_rn(w, (double)mj);
            W = __dadd_rn(W, w);
#pragma unroll
            for (int q = 0; q < kWords; ++q) {
                const unsigned word = R[q];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * q + e < 3 * kBins)
                        A[4 * q + e] = __dadd_rn(A[4 * q + e], __dmul_rn(c, (double)((word >> (8 * e)) & 0xFFu)));
            }
        }
        unsigned bytes[kWidth];
#pragma unroll
        for (int b = 0; b < kWidth; ++b) bytes[b] = 0u;
        if (mi > 0) {
            const double m = (double)mi;
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                double F[kBins], tot = 0.0;
#pragma unroll
                for (int b = 0; b < kBins; ++b) {
                    const int at = g * kBins + b;
                    F[b] = __ddiv_rn((double)((own[at >> 2] >> (8 * (at & 3))) & 0xFFu), m);
                    if (W > 0.0) F[b] = __dadd_rn(F[b], __ddiv_rn(A[at], W));
                    tot = b == 0 ? F[0] : __dadd_rn(tot, F[b]);
                }
#pragma unroll
                for (int b = 0; b < kBins; ++b) bytes[g * kBins + b] = (unsigned)(int)__ddiv_rn(__dmul_rn(255.0, F[b]), tot);   // the cast truncates
            }
        }
#pragma unroll
        for (int q = 0; q < kWords; ++q)
            features[row * kWords + q] = bytes[4 * q] | bytes[4 * q + 1] << 8 | bytes[4 * q + 2] << 16 | bytes[4 * q + 3] << 24;
        count[row] = mi;
    }
}

__global__ __launch_bounds__(kThreads) void feature_match_kernel(int S, long long T, long long U, const unsigned* __restrict__ feat,
                                                                 const long long* __restrict__ offsets,
                                                                 const unsigned* __restrict__ tfeat,
                                                                 const long long* __restrict__ toffsets, const int* __restrict__ counts,
                                                                 const int* __restrict__ tcounts, int* __restrict__ match,
                                                                 int* __restrict__ dist) {
    __shared__ uint4 tile[kMatchTile * 3];
    const int tid = threadIdx.x;
    const long long chunks = (T + kMatchChunk - 1) / kMatchChunk;
    for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const long long row0 = chunk * kMatchChunk;
        unsigned a[kMatchRows][kWords];
        int na[kMatchRows];
        bool have[kMatchRows];
#pragma unroll
        for (int r = 0; r < kMatchRows; ++r) {
            const long long g = row0 + r * kThreads + tid;
            have[r] = g < T && counts[g] > 0;
            na[r] = 0;
#pragma unroll
            for (int q = 0; q < kWords; ++q) {
                a[r][q] = have[r] ? feat[g * kWords + q] : 0u;
                na[r] = (int)__builtin_amdgcn_udot4(a[r][q], a[r][q], (unsigned)na[r], false);
            }
            if (g < T) {                                   // the empty result; a row of a valid set with a match writes over it below
                match[g] = -1;
                dist[g] = -1;
            }
        }
        const long long last = (row0 + kMatchChunk < T ? row0 + kMatchChunk : T) - 1;
        // every value that steers these loops is uniform over the workgroup
        for (int s = hp_align::set_of(offsets, S, row0); s < S && offsets[s] <= last; ++s) {
            const long long lo = offsets[s], hi = offsets[s + 1], tlo = toffsets[s], thi = toffsets[s + 1];
            if (!hp_align::set_ok(lo, hi, T) || !hp_align::set_ok(tlo, thi, U)) continue;
            const int m = (int)(thi - tlo);
            int best[kMatchRows], at[kMatchRows];
#pragma unroll
            for (int r = 0; r < kMatchRows; ++r) {
                best[r] = kNoMatch;
                at[r] = -1;
            }
            for (int t0 = 0; t0 < m; t0 += kMatchTile) {
                const int cnt = m - t0 < kMatchTile ? m - t0 : kMatchTile;
                __syncthreads();                                               // the tile before this one has been read
                if (tid < cnt) {
                    const long long u = tlo + t0 + tid;
                    const bool present = tcounts[u] > 0;
                    unsigned b[kWords], nb = 0u;
#pragma unroll
                    for (int q = 0; q < kWords; ++q) {
                        b[q] = present ? tfeat[u * kWords + q] : 0u;
                        nb = __builtin_amdgcn_udot4(b[q], b[q], nb, false);
                    }
                    if (!present) nb = (unsigned)kNoMatch;
                    tile[tid * 3] = make_uint4(b[0], b[1], b[2], b[3]);
                    tile[tid * 3 + 1] = make_uint4(b[4], b[5], b[6], b[7]);
                    tile[tid * 3 + 2] = make_uint4(b[8], nb, 0u, 0u);
                }
                __syncthreads();
#pragma unroll 2
                for (int c = 0; c < cnt; ++c) {
                    const uint4 b0 = tile[c * 3], b1 = tile[c * 3 + 1], b2 = tile[c * 3 + 2];
                    const unsigned b[kWords] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w, b2.x};
#pragma unroll
                    for (int r = 0; r < kMatchRows; ++r) {
                        unsigned ab = 0u;
#pragma unroll
                        for (int q = 0; q < kWords; ++q) ab = __builtin_amdgcn_udot4(a[r][q], b[q], ab, false);
                        const int d = na[r] + (int)b2.y - 2 * (int)ab;
                        const bool closer = d < best[r];
                        best[r] = closer ? d : best[r];
                        at[r] = closer ? t0 + c : at[r];
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < kMatchRows; ++r) {
                const long long g = row0 + r * kThreads + tid;
                if (have[r] && g >= lo && g < hi && at[r] >= 0) {
                    match[g] = at[r];
                    dist[g] = best[r];
                }
            }
        }
    }
}

int features_instance(int k) { return k <= 8 ? 8 : k <= 16 ? 16 : 32; }

}  // namespace

// The instance hp_scan_features launches for k: its compile-time list length, the threads per workgroup (= rows per chunk) and
// the bytes of a descriptor.  Host only.
HP_API int hp_scan_features_plan(int k, int* instance_k, int* threads, int* width) {
    HP_CHECK_ARG(k >= 1 && k <= kFeatMaxK && instance_k && threads && width);
    *instance_k = features_instance(k);
    *threads = kThreads;
    *width = kWidth;
    return 0;
}

// Bytes of hp_scan_features' workspace: one SPFH record a row.  Host only.
HP_API long hp_scan_features_workspace_bytes(long long T) {
    if (T < 0 || T > (1ll << 40)) return -1;
    return (long)(T * kWidth);
}

// Descriptors (T,36) and pair counts (T) of S ragged scans from given lists and normals: see the law at the top and
// include/hyperpocket_hip.h.  Rows at or beyond offsets[S] are written as rows without a descriptor.
HP_API int hp_scan_features(int S, long long T, const float* points, const long long* offsets, const float* normals, int k,
                            const int* index, unsigned char* features, int* count, void* ws, hipStream_t stream) {
    HP_CHECK_ARG(S >= 1 && T >= 0 && T <= (1ll << 40) && k >= 1 && k <= kFeatMaxK);
    HP_CHECK_ARG(points && offsets && normals && index && features && count && ws);
    HP_CHECK_ARG((reinterpret_cast<uintptr_t>(features) & 3) == 0 && (reinterpret_cast<uintptr_t>(ws) & 3) == 0);
    if (T == 0) return 0;
    const int vec = (k & 3) == 0 && (reinterpret_cast<uintptr_t>(index) & 15) == 0;   // every row of the lists starts on 16 bytes
    const unsigned grid = (unsigned)std::min<long long>((T + kThreads - 1) / kThreads, kGrid);
    unsigned* spfh = static_cast<unsigned*>(ws);
    unsigned* out = reinterpret_cast<unsigned*>(features);
#define HP_FEATURES_CASE(KK)                                                                                                       \
    if (k <= KK) {                                                                                                                 \
        hipLaunchKernelGGL((spfh_kernel<KK>), dim3(grid), dim3(kThreads), 0, stream, S, T, points, offsets, normals, k, vec, index, \
                           spfh);                                                                                                  \
        hipLaunchKernelGGL((fpfh_kernel<KK>), dim3(grid), dim3(kThreads), 0, stream, S, T, points, offsets, k, vec, index, spfh, out, \
                           count);                                                                                                 \
        HP_RETURN_LAST_ERROR();                                                                                                    \
    }
    HP_FEATURES_CASE(8)
    HP_FEATURES_CASE(16)
    HP_FEATURES_CASE(32)
#undef HP_FEATURES_CASE
    return -1;
}

// The geometry of hp_scan_feature_match: threads per workgroup, source rows a lane holds and target records per LDS tile.  Host only.
HP_API int hp_scan_feature_match_plan(int* threads, int* rows_per_lane, int* tile) {
    HP_CHECK_ARG(threads && rows_per_lane && tile);
    *threads = kThreads;
    *rows_per_lane = kMatchRows;
    *tile = kMatchTile;
    return 0;
}

// The nearest target descriptor of every source row, set by set: match (T) and dist (T); the law is in include/hyperpocket_hip.h.
HP_API int hp_scan_feature_match(int S, long long T, const unsigned char* features, const long long* offsets, long long U,
                                 const unsigned char* tfeatures, const long long* toffsets, const int* counts, const int* tcounts,
                                 int* match, int* dist, hipStream_t stream) {
    HP_CHECK_ARG(S >= 1 && T >= 0 && U >= 0 && T <= (1ll << 40) && U <= (1ll << 40));
    HP_CHECK_ARG(offsets && toffsets && (T == 0 || (features && counts && match && dist)) && (U == 0 || (tfeatures && tcounts)));
    HP_CHECK_ARG((reinterpret_cast<uintptr_t>(features) & 3) == 0 && (reinterpret_cast<uintptr_t>(tfeatures) & 3) == 0);
    if (T == 0) return 0;
    const unsigned grid = (unsigned)std::min<long long>((T + kMatchChunk - 1) / kMatchChunk, hp_align::kMaxGrid);
    hipLaunchKernelGGL(feature_match_kernel, dim3(grid), dim3(kThreads), 0, stream, S, T, U, reinterpret_cast<const unsigned*>(features),
                       offsets, reinterpret_cast<const unsigned*>(tfeatures), toffsets, counts, tcounts, match, dist);
    HP_RETURN_LAST_ERROR();
}
