// Surface normals and surface variation of ragged scans from given neighbour lists: the smallest eigenvector of
// the scatter of a row's neighbourhood, and the share of the variance along it — what point-to-plane registration and a
// depth-edge filter both start from.
//
// The law, per scan and per row i (include/hyperpocket_hip.h and tests/normals_law.py have it in full):
//   the neighbourhood is row i plus every slot of its list index (T,k) that names a present row of the scan, 0 <= index < n_s;
//   dq = p_j - p_i in fp32; M = the largest |dq_c|; q_c = trunc(ldexp(dq_c, 19 - e)) with e = M's exponent (plane.hip's frame);
//   C_ab = m * S_ab - S_a * S_b over the q's, exact in int64 and, with m <= 33, below 2^53, so exact in fp64 too;
//   a fixed number of cyclic Jacobi sweeps in fp64, one rounding per operation; the column of the smallest diagonal entry,
//   normalised, signed and rounded to fp32, is the normal; max(lambda_min, 0) / trace is the curvature.
//
//   normals  grid-stride over chunks of 256 consecutive rows of the whole ragged set, one lane per row.  The chunk's first and
//            last scan are found once per workgroup (uniform loads), a lane then finds its own between the two.  The lane reads
//            its list with 16-byte loads (when k is a multiple of 4 and the lists are aligned; scalar loads otherwise), gathers
//            the neighbours' coordinates from global memory — a capped scan is 768 KB and lives in L2 — and keeps the K
//            differences in registers (K = 8, 16 or 32 at compile time, as knn.hip) for the two passes the law needs: the
//            maximum, then the quantised sums.  The eigen-solve runs after the differences are dead, so the fp64 state (six
//            matrix entries, nine of V) takes their place in the register file.  No LDS, no atomics, no workspace.
#include "hp_common.h"

namespace {

using hp::finite_bits, hp::kInfBits;
constexpr int kNormalsMaxK = 32;
constexpr int kThreads = 256;              // rows per chunk
constexpr int kGrid = 2048;                // workgroups of a launch: the row count lives on the device (offsets[S])
constexpr int kSweeps = 6;                 // = normals_law.SWEEPS
constexpr unsigned kQuietNaN = 0x7FC00000u;

// One Jacobi rotation of the pair (p, q), r the third index: the law's formulas operation by operation.
__device__ __forceinline__ void rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                       double& v1p, double& v1q, double& v2p, double& v2q) {
#pragma clang fp contract(off)
    if (apq == 0.0) return;
    const double theta = __ddiv_rn(__dsub_rn(aqq, app), __dmul_rn(2.0, apq));
    const double root = __dsqrt_rn(__dadd_rn(__dmul_rn(theta, theta), 1.0));
    const double t = __ddiv_rn(theta >= 0.0 ? 1.0 : -1.0, __dadd_rn(fabs(theta), root));
    const double c = __ddiv_rn(1.0, __dsqrt_rn(__dadd_rn(__dmul_rn(t, t), 1.0)));
    const double s = __dmul_rn(t, c);
    const double h = __dmul_rn(t, apq);
    app = __dsub_rn(app, h);
    aqq = __dadd_rn(aqq, h);
    apq = 0.0;
    const double rp = arp, rq = arq;
    arp = __dsub_rn(__dmul_rn(c, rp), __dmul_rn(s, rq));
    arq = __dadd_rn(__dmul_rn(s, rp), __dmul_rn(c, rq));
    double a = v0p, b = v0q;
    v0p = __dsub_rn(__dmul_rn(c, a), __dmul_rn(s, b));
    v0q = __dadd_rn(__dmul_rn(s, a), __dmul_rn(c, b));
    a = v1p, b = v1q;
    v1p = __dsub_rn(__dmul_rn(c, a), __dmul_rn(s, b));
    v1q = __dadd_rn(__dmul_rn(s, a), __dmul_rn(c, b));
    a = v2p, b = v2q;
    v2p = __dsub_rn(__dmul_rn(c, a), __dmul_rn(s, b));
    v2q = __dadd_rn(__dmul_rn(s, a), __dmul_rn(c, b));
}

template <int K>
__global__ __launch_bounds__(kThreads) void normals_kernel(int S, const float* __restrict__ points,
                                                           const long long* __restrict__ offsets, int k, int vec,
                                                           const int* __restrict__ index, const float* __restrict__ viewpoints,
                                                           float* __restrict__ normal, float* __restrict__ curvature,
                                                           int* __restrict__ count) {
#pragma clang fp contract(off)
    const long long T = offsets[S];
    for (long long row0 = (long long)blockIdx.x * kThreads; row0 < T; row0 += (long long)gridDim.x * kThreads) {
        const long long last = (row0 + kThreads < T ? row0 + kThreads : T) - 1;
        int s0 = 0, s1 = 0;                                // the scans of row0 and of last: the last s with offsets[s] <= row
        for (int hi = S; hi - s0 > 1;) {
            const int mid = (s0 + hi) >> 1;
            if (offsets[mid] <= row0) s0 = mid;
            else hi = mid;
        }
        s1 = s0;
        for (int hi = S; hi - s1 > 1;) {
            const int mid = (s1 + hi) >> 1;
            if (offsets[mid] <= last) s1 = mid;
            else hi = mid;
        }
        const long long row = row0 + threadIdx.x;
        if (row > last) continue;
        int s = s0;
        for (int hi = s1 + 1; hi - s > 1;) {               // this lane's scan, between the two
            const int mid = (s + hi) >> 1;
            if (offsets[mid] <= row) s = mid;
            else hi = mid;
        }
        const long long lo = offsets[s];
        long long end = offsets[s + 1];
        end = end < T ? end : T;                           // nothing at or beyond T is read, whatever the offsets say
        const long long n = lo >= 0 ? end - lo : 0;        // slots are valid in [0, n)

        const float px = points[row * 3], py = points[row * 3 + 1], pz = points[row * 3 + 2];
        const bool present = finite_bits(px) && finite_bits(py) && finite_bits(pz);

        int idx[K];
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

        // pass 1: the differences into registers, their largest magnitude, the neighbourhood's size
        float dx[K], dy[K], dz[K];
        unsigned mbits = 0u;
        int cnt = present ? 1 : 0;
#pragma unroll
        for (int t = 0; t < K; ++t) {
            dx[t] = dy[t] = dz[t] = 0.f;
            const long long j = idx[t];
            if (present && j >= 0 && j < n) {
                const float* P = points + (lo + j) * 3;
                const float x = P[0], y = P[1], z = P[2];
                if (finite_bits(x) && finite_bits(y) && finite_bits(z)) {
                    dx[t] = __fsub_rn(x, px);
                    dy[t] = __fsub_rn(y, py);
                    dz[t] = __fsub_rn(z, pz);
                    ++cnt;
                    const unsigned ax = (unsigned)__float_as_int(dx[t]) & 0x7FFFFFFFu, ay = (unsigned)__float_as_int(dy[t]) & 0x7FFFFFFFu,
                                   az = (unsigned)__float_as_int(dz[t]) & 0x7FFFFFFFu;     // finite or inf: the bits order as the values
                    mbits = ax > mbits ? ax : mbits;
                    mbits = ay > mbits ? ay : mbits;
                    mbits = az > mbits ? az : mbits;
                }
            }
        }
        count[row] = cnt;
        float nx = __int_as_float((int)kQuietNaN), ny = nx, nz = nx, curv = nx;
        if (cnt >= 3 && mbits != 0u && mbits < kInfBits) {
            // pass 2: the quantised sums, exact integers
            const int sh = 19 - ((int)(mbits >> 23) - 127);
            int s1x = 0, s1y = 0, s1z = 0;                 // |sum| <= 32 * 2^20
            long long sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
#pragma unroll
            for (int t = 0; t < K; ++t) {
                const int qx = (int)ldexpf(dx[t], sh), qy = (int)ldexpf(dy[t], sh), qz = (int)ldexpf(dz[t], sh);   // exact; the cast truncates
                s1x += qx;
                s1y += qy;
                s1z += qz;
                sxx += (long long)qx * qx;
                sxy += (long long)qx * qy;
                sxz += (long long)qx * qz;
                syy += (long long)qy * qy;
                syz += (long long)qy * qz;
                szz += (long long)qz * qz;
            }
            const long long m = cnt;
            const long long c00 = m * sxx - (long long)s1x * s1x, c01 = m * sxy - (long long)s1x * s1y,
                            c02 = m * sxz - (long long)s1x * s1z, c11 = m * syy - (long long)s1y * s1y,
                            c12 = m * syz - (long long)s1y * s1z, c22 = m * szz - (long long)s1z * s1z;
            const long long trace = c00 + c11 + c22;       // every one of these below 2^53: the conversions are exact
            if (trace != 0) {
                double a00 = (double)c00, a01 = (double)c01, a02 = (double)c02, a11 = (double)c11, a12 = (double)c12,
                       a22 = (double)c22;
                double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
                for (int sweep = 0; sweep < kSweeps; ++sweep) {
                    rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);     // (0,1), r = 2
                    rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);     // (0,2), r = 1
                    rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);     // (1,2), r = 0
                }
                const bool b1 = a11 < a00;                 // the smallest entry, ties to the lower index
                const double l01 = b1 ? a11 : a00;
                const bool b2 = a22 < l01;
                const double lmin = b2 ? a22 : l01;
                double x = b2 ? v02 : b1 ? v01 : v00, y = b2 ? v12 : b1 ? v11 : v10, z = b2 ? v22 : b1 ? v21 : v20;
                const double len = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)), __dmul_rn(z, z)));
                x = __ddiv_rn(x, len);
                y = __ddiv_rn(y, len);
                z = __ddiv_rn(z, len);
                double lead = x;                           // the component of largest magnitude, ties to the lower axis
                if (fabs(y) > fabs(lead)) lead = y;
                if (fabs(z) > fabs(lead)) lead = z;
                bool flip = lead < 0.0;
                if (viewpoints) {
                    const double wx = __dsub_rn((double)viewpoints[s * 3], (double)px),
                                 wy = __dsub_rn((double)viewpoints[s * 3 + 1], (double)py),
                                 wz = __dsub_rn((double)viewpoints[s * 3 + 2], (double)pz);
                    const double sx = flip ? -x : x, sy = flip ? -y : y, sz = flip ? -z : z;
                    const double dot = __dadd_rn(__dadd_rn(__dmul_rn(sx, wx), __dmul_rn(sy, wy)), __dmul_rn(sz, wz));
                    flip = flip != (dot < 0.0);
                }
                nx = __double2float_rn(flip ? -x : x);
                ny = __double2float_rn(flip ? -y : y);
                nz = __double2float_rn(flip ? -z : z);
                curv = __double2float_rn(__ddiv_rn(lmin > 0.0 ? lmin : 0.0, (double)trace));
            }
        }
        normal[row * 3] = nx;
        normal[row * 3 + 1] = ny;
        normal[row * 3 + 2] = nz;
        curvature[row] = curv;
    }
}

}  // namespace

// The instance hp_scan_normals launches for k: its compile-time list length, threads per workgroup (= rows per chunk) and the
// Jacobi sweeps it runs.  Host only.
HP_API int hp_scan_normals_plan(int k, int* instance_k, int* threads, int* sweeps) {
    HP_CHECK_ARG(k >= 2 && k <= kNormalsMaxK && instance_k && threads && sweeps);
    *instance_k = k <= 8 ? 8 : k <= 16 ? 16 : 32;
    *threads = kThreads;
    *sweeps = kSweeps;
    return 0;
}

// Normals, surface variation and neighbourhood sizes of S ragged scans from given lists: see the law at the top and
// include/hyperpocket_hip.h.
HP_API int hp_scan_normals(int S, const float* points, const long long* offsets, int k, const int* index, const float* viewpoints,
                           float* normal, float* curvature, int* count, hipStream_t stream) {
    HP_CHECK_ARG(S >= 1 && k >= 2 && k <= kNormalsMaxK);
    HP_CHECK_ARG(points && offsets && index && normal && curvature && count);
    const int vec = (k & 3) == 0 && (reinterpret_cast<uintptr_t>(index) & 15) == 0;   // every row of the lists starts on 16 bytes
#define HP_NORMALS_CASE(KK)                                                                                                 \
    if (k <= KK) {                                                                                                          \
        hipLaunchKernelGGL((normals_kernel<KK>), dim3(kGrid), dim3(kThreads), 0, stream, S, points, offsets, k, vec, index, \
                           viewpoints, normal, curvature, count);                                                           \
        HP_RETURN_LAST_ERROR();                                                                                             \
    }
    HP_NORMALS_CASE(8)
    HP_NORMALS_CASE(16)
    HP_NORMALS_CASE(32)
#undef HP_NORMALS_CASE
    return -1;
}
