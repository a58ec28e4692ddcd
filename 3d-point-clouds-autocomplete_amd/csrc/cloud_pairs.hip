// Nearest-neighbour reductions over a list of cloud pairs: the evaluation metrics' kernel (UHD, TMD, all-pairs MMD,
// completeness).
//
// Replaces (behaviour, not code): the reference's evaluation distances, which run on the CPU —
//   utils/evaluation/completeness.py:13-49   directed_hausdorff on a (B,3,N,M) torch tensor, completeness on a KD-tree
//   utils/evaluation/chamfer.py:8-31          compute_trimesh_chamfer on scipy KD-trees (TMD's pair distance)
//
// Design:
//  * a pair (a, b) indexes two clouds A[a] (n points) and B[b] (m points); the caller hands P pairs (P may exceed the
//    65 535 of a grid dimension: the grid is one-dimensional).
//  * the inner loop is nn_distance_kernel's (structural_losses.hip) without the arg-min: R queries per lane in
//    registers, candidates swept through a 12 KB LDS tile as wave-uniform ds_read_b128 broadcasts into packed fp32 ops,
//    each element computing fma(dz,dz,fma(dy,dy,dx*dx)) on the direct differences — every per-point minimum is
//    bit-identical to hp_nndistance's.  One v_min3_f32 per candidate pair carries the running minimum.
//  * a workgroup owns one query tile (256*R points) of one direction and G consecutive pairs; the tile's queries are
//    re-read from memory only when the query cloud changes between those pairs (UHD: one partial input against its k
//    completions; all-pairs MMD: one sample against many references).
//  * deterministic: every workgroup writes its tile's partial (fp64 sum of the fp32 minima, their max, or a count) to
//    its own workspace slot, and a second launch folds each pair's slots in tile order and rounds once.  No atomics.
#include "hp_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 1024;                 // candidates per LDS tile
constexpr int kTileF4 = kTile / 4 * 3;      // float4 per tile (groups of 4 candidates in 3 float4)
constexpr int kUnroll = 8;                  // candidate groups per unrolled step: the tile is padded to 32 candidates

enum Mode { kChamfer = 0, kHausdorff = 1, kCovered = 2 };

using hp::f2, hp::splat2, hp::sqdist2;

struct PairsArgs {
    const float* A;      // (na, n, 3)
    const float* B;      // (nb, m, 3)
    const int* ab;       // (pairs, 2)
    double* ws;          // (pairs, tiles_a + tiles_b) tile partials
    long pairs;
    int na, n, nb, m;
    int tiles_a, tiles_b;  // query tiles of the A->B direction, of the B->A direction (0 unless chamfer)
    int group;             // pairs per workgroup
    double thres2;         // covered: min d^2 < thres^2 in fp64 — exact, the same as sqrt(min d^2) < thres
};

// waves_per_eu(7): without the hint the compiler hoists more of the unrolled LDS reads than it needs and R = 4 lands at
// 104 VGPRs (4 waves per SIMD); with it R = 4 takes 72 VGPRs (7 waves, nn_distance_kernel's figure), R = 2 and R = 1
// ~54 (8 waves), all without scratch.
template <int R, int MODE>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(7))) void cloud_pairs_kernel(const PairsArgs p) {
    __shared__ float4 tile[kTileF4];
    __shared__ double red[kThreads / 64];
    const int tid = threadIdx.x;
    const int tiles = p.tiles_a + p.tiles_b;
    const long grp = blockIdx.x / tiles;
    const int t = blockIdx.x - (int)(grp * tiles);
    const bool second = t >= p.tiles_a;          // B->A: queries from B[b], candidates from A[a]
    const int qt = second ? t - p.tiles_a : t;
    const int nq = second ? p.m : p.n, nc = second ? p.n : p.m;
    const float* Qbase = second ? p.B : p.A;
    const float* Cbase = second ? p.A : p.B;
    const float kInf = __builtin_inff();

    f2 qx[R], qy[R], qz[R];
    int qcloud = -1;
    const long p0 = grp * p.group, p1 = min(p0 + p.group, p.pairs);
    for (long pi = p0; pi < p1; ++pi) {
        const int a = p.ab[pi * 2], b = p.ab[pi * 2 + 1];
        if ((unsigned)a >= (unsigned)p.na || (unsigned)b >= (unsigned)p.nb) continue;   // the finish kernel writes NaN
        const int qc = second ? b : a, cc = second ? a : b;
        if (qc != qcloud) {
            qcloud = qc;
            const float* Q = Qbase + (size_t)qc * nq * 3;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int j = qt * (kThreads * R) + r * kThreads + tid;
                float x = 0.f, y = 0.f, z = 0.f;
                if (j < nq) {
                    x = Q[j * 3 + 0];
                    y = Q[j * 3 + 1];
                    z = Q[j * 3 + 2];
                }
                qx[r] = splat2(x);
                qy[r] = splat2(y);
                qz[r] = splat2(z);
            }
        }
        const float* C = Cbase + (size_t)cc * nc * 3;
        float run[R];
#pragma unroll
        for (int r = 0; r < R; ++r) run[r] = kInf;
        for (int k0 = 0; k0 < nc; k0 += kTile) {
            const int cnt = min(kTile, nc - k0);
            const int groups = (cnt + kUnroll * 4 - 1) / (kUnroll * 4) * kUnroll;   // candidates past nc sit at +inf
            for (int g = tid; g < groups; g += kThreads) {
                float v[12];
#pragma unroll
                for (int u = 0; u < 12; ++u) {
                    const int k = g * 4 + u / 3;
                    v[u] = k < cnt ? C[(size_t)(k0 + k) * 3 + u % 3] : kInf;
                }
                tile[g * 3 + 0] = make_float4(v[0], v[3], v[1], v[4]);
                tile[g * 3 + 1] = make_float4(v[2], v[5], v[6], v[9]);
                tile[g * 3 + 2] = make_float4(v[7], v[10], v[8], v[11]);
            }
            __syncthreads();
            for (int c = 0; c < groups; c += kUnroll) {
#pragma unroll
                for (int g = 0; g < kUnroll; ++g) {
                    const float4 X = tile[(c + g) * 3 + 0], Y = tile[(c + g) * 3 + 1], Z = tile[(c + g) * 3 + 2];
                    const f2 x01{X.x, X.y}, y01{X.z, X.w}, z01{Y.x, Y.y}, x23{Y.z, Y.w}, y23{Z.x, Z.y}, z23{Z.z, Z.w};
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const f2 e = sqdist2(x01 - qx[r], y01 - qy[r], z01 - qz[r]);
                        const f2 f = sqdist2(x23 - qx[r], y23 - qy[r], z23 - qz[r]);
                        run[r] = __builtin_fminf(__builtin_fminf(run[r], e.x), e.y);
                        run[r] = __builtin_fminf(__builtin_fminf(run[r], f.x), f.y);
                    }
                }
            }
            __syncthreads();
        }
        // this tile's partial: an fp64 sum of the minima (chamfer), their max (hausdorff), or a count (covered)
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int j = qt * (kThreads * R) + r * kThreads + tid;
            if (j < nq) {
                if (MODE == kChamfer) s += (double)run[r];
                else if (MODE == kHausdorff) s = fmax(s, (double)run[r]);
                else s += (double)run[r] < p.thres2 ? 1.0 : 0.0;
            }
        }
        double v;
        if (MODE == kHausdorff) {
            float w = hp::wave_max((float)s);    // exact: s is one of the fp32 minima (or 0)
            const int lane = tid & 63, wid = tid >> 6;
            if (lane == 0) red[wid] = (double)w;
            __syncthreads();
            v = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
            __syncthreads();
        } else {
            v = hp::block_sum(s, red);
        }
        if (tid == 0) p.ws[pi * tiles + t] = v;
    }
}

// out[pair] (hausdorff / covered) or out[pair*2 + dir] (chamfer): the pair's tile partials folded in tile order
template <int MODE>
__global__ __launch_bounds__(256) void cloud_pairs_finish_kernel(const PairsArgs p, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int dirs = MODE == kChamfer ? 2 : 1;
    if (i >= p.pairs * dirs) return;
    const long pi = i / dirs;
    const int dir = (int)(i - pi * dirs);
    const int a = p.ab[pi * 2], b = p.ab[pi * 2 + 1];
    if ((unsigned)a >= (unsigned)p.na || (unsigned)b >= (unsigned)p.nb) {
        out[i] = __builtin_nanf("");
        return;
    }
    const int tiles = p.tiles_a + p.tiles_b;
    const int t0 = dir ? p.tiles_a : 0, t1 = dir ? tiles : p.tiles_a;
    const double* w = p.ws + pi * tiles;
    double v = 0.0;
    for (int t = t0; t < t1; ++t) v = MODE == kHausdorff ? fmax(v, w[t]) : v + w[t];
    out[i] = (float)v;
}

inline int tiles_of(int n, int r) { return (n + kThreads * r - 1) / (kThreads * r); }

// Query points per lane: 4 while the launch still has 1024 workgroups (four per CU), else 2, else 1.  Then pairs per
// workgroup: 8, 4 or 2 while 2048 workgroups remain.  Both depend on (mode, n, m, pairs) only, so the workspace query
// and the launch agree.
struct Plan {
    int r, tiles_a, tiles_b, group;
};
inline Plan plan(int mode, int n, int m, long pairs) {
    Plan pl{1, 0, 0, 1};
    for (int r = 4; r >= 1; r >>= 1) {
        pl.r = r;
        pl.tiles_a = tiles_of(n, r);
        pl.tiles_b = mode == kChamfer ? tiles_of(m, r) : 0;
        if (pairs * (pl.tiles_a + pl.tiles_b) >= 1024) break;
    }
    const long tiles = pl.tiles_a + pl.tiles_b;
    for (int g = 8; g > 1; g >>= 1)
        if ((pairs + g - 1) / g * tiles >= 2048) {
            pl.group = g;
            break;
        }
    return pl;
}

template <int MODE>
void launch(const PairsArgs& a, int r, float* out, hipStream_t stream) {
    const long blocks = (a.pairs + a.group - 1) / a.group * (a.tiles_a + a.tiles_b);
    const dim3 grid((unsigned)blocks), block(kThreads);
    if (r == 4) hipLaunchKernelGGL((cloud_pairs_kernel<4, MODE>), grid, block, 0, stream, a);
    else if (r == 2) hipLaunchKernelGGL((cloud_pairs_kernel<2, MODE>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((cloud_pairs_kernel<1, MODE>), grid, block, 0, stream, a);
    const long outs = a.pairs * (MODE == kChamfer ? 2 : 1);
    hipLaunchKernelGGL((cloud_pairs_finish_kernel<MODE>), dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, stream, a, out);
}

}  // namespace

// ================================================================================================
// C ABI
// ================================================================================================

HP_API long hp_cloud_pairs_workspace_floats(int mode, int n, int m, long pairs) {
    if (mode < kChamfer || mode > kCovered || n <= 0 || m <= 0 || pairs < 0) return -1;
    const Plan pl = plan(mode, n, m, pairs);
    return 2 * pairs * (pl.tiles_a + pl.tiles_b);   // one double per (pair, query tile)
}

// What plan() decides for (mode, n, m, pairs): *r = queries per lane of the kernel instance, *group = pairs per workgroup.
// Host only; either pointer may be NULL.
HP_API int hp_cloud_pairs_plan(int mode, int n, int m, long pairs, int* r, int* group) {
    HP_CHECK_ARG(mode >= kChamfer && mode <= kCovered && n > 0 && m > 0 && pairs >= 0);
    const Plan pl = plan(mode, n, m, pairs);
    if (r) *r = pl.r;
    if (group) *group = pl.group;
    return 0;
}

HP_API int hp_cloud_pairs(int mode, int na, int n, const float* A, int nb, int m, const float* B, long pairs,
                          const int* pair_ab, float thres, float* ws, float* out, hipStream_t stream) {
    HP_CHECK_ARG(mode >= kChamfer && mode <= kCovered);
    HP_CHECK_ARG(na > 0 && n > 0 && nb > 0 && m > 0 && pairs >= 0);
    HP_CHECK_ARG(mode != kCovered || (n < (1 << 24) && thres >= 0.f));   // a count below 2^24 is exact in fp32
    if (pairs == 0) return 0;
    HP_CHECK_ARG(A && B && pair_ab && ws && out);
    HP_CHECK_ARG(((uintptr_t)ws & 7) == 0);
    const Plan pl = plan(mode, n, m, pairs);
    HP_CHECK_ARG((pairs + pl.group - 1) / pl.group * (pl.tiles_a + pl.tiles_b) <= 0x7fffffffL);
    PairsArgs a{A, B, pair_ab, (double*)ws, pairs, na, n, nb, m, pl.tiles_a, pl.tiles_b, pl.group,
                (double)thres * thres};
    if (mode == kChamfer) launch<kChamfer>(a, pl.r, out, stream);
    else if (mode == kHausdorff) launch<kHausdorff>(a, pl.r, out, stream);
    else launch<kCovered>(a, pl.r, out, stream);
    HP_RETURN_LAST_ERROR();
}
