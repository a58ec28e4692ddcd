// Euclidean cluster extraction over ragged scans: the connected components of "closer than a radius" — what a
// real scan with a second object or a patch of table needs after outlier removal (knn.hip) has taken the isolated points.
//
// The law, per scan (include/hyperpocket_hip.h and tests/cluster_law.py have it in full):
//   d2(i, j) = ((dx*dx + dy*dy) + dz*dz), every operation one fp32 rounding, no contraction (knn.hip's formula): symmetric bit
//   for bit, and with finite coordinates never NaN.  r2 = radius * radius, one fp32 rounding, finite.
//   a row with a non-finite coordinate is absent.  {i, j} is an edge iff i != j, both present, d2 <= r2.
//   label[i] = the smallest row of i's component (-1 absent), size[i] = its rows (0 absent), clusters[s] = the components,
//   largest[s] = the label of the one with the most rows, ties to the smaller label (-1: no row present).
//   A scan longer than max_points gets the empty result.
//
//   clusters  grid (S), one workgroup of 1024 lanes per scan, a union-find forest parent[n] (int32, rows local to the scan) in
//             LDS behind the candidate tile.  The pair sweep is knn.hip's: a lane owns a row, candidates pass through an LDS
//             tile of 1024 float4 (x, y, z, absent mask) that a wave reads at one address, a group of four ahead in registers.
//             The edge relation is symmetric, so row i visits candidates j < i only: tiles are the outer loop (one load per
//             tile), the blocks of 1024 rows at or behind the tile the inner one, no barrier between them, and on the
//             diagonal a wave stops at its own last row.  The absent mask is or-ed into the bits of d2 (all ones is above
//             every finite r2, and so is +inf), so the test is one unsigned compare.
//             A passing pair whose candidate does not hang right under the lane's last root (one LDS read: the common case
//             once a dense piece has formed) unites the two trees: find both roots, hook the larger under the smaller with a
//             compare-and-swap on the larger's slot.  parent[x] <= x holds at every moment, and a slot that has left the
//             root state (parent[x] < x) never returns to it: the CAS writes only roots, path halving (an atomic min)
//             only lowers.  So every step of a find walk strictly lowers the row it stands on, and every failed CAS hands
//             back a parent below the row it tried: both loops carry the bound n.  Nothing waits for another lane or wave.
//             After a barrier label = find (the root is the smallest row of its tree), sizes are integer adds on the roots'
//             slots of the re-used parent array, clusters a count of roots, largest one max over (size << 16 | 0xFFFF - label).
#include "hp_common.h"

namespace {

using hp::finite_bits, hp::kInfBits;
constexpr int kClusterMaxPoints = 32768;   // = HP_CLUSTER_MAX_POINTS (include/hyperpocket_hip.h)
constexpr int kThreads = 1024;             // rows per block of a scan
constexpr int kTile = 1024;                // candidates per LDS tile (16 KiB); = kThreads, so block b's diagonal tile is tile b
constexpr int kGroup = 4;                  // candidates read ahead; kTile is a multiple
constexpr unsigned kAbsent = 0xFFFFFFFFu;  // the mask of an absent candidate
constexpr size_t kTileBytes = (size_t)(kTile + 2 * kGroup) * sizeof(float4);

__device__ __forceinline__ int peek(const int* slot) {
    return __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The root of x's tree at some moment of the call, halving the path behind it.  Every pass lowers x (gp < p < x): <= n passes.
__device__ __forceinline__ int find(int* parent, int x, int n) {
    for (int pass = 0; pass < n; ++pass) {
        const int p = peek(parent + x);
        if (p == x) break;
        const int gp = peek(parent + p);
        if (gp == p) return p;
        atomicMin(parent + x, gp);
        x = gp;
    }
    return x;
}

// Joins the trees of a and b and returns a row of the joined tree at or below both (its root, unless another lane has hooked
// it since).  The larger of the two rows at hand strictly falls from one pass to the next: a failed CAS hands back that row's
// parent, which lies below it, and the other row lay below it already.  <= n passes.
__device__ __forceinline__ int unite(int* parent, int a, int b, int n) {
    for (int pass = 0; pass < n; ++pass) {
        a = find(parent, a, n);
        b = find(parent, b, n);
        if (a == b) return a;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int was = atomicCAS(parent + hi, hi, lo);
        if (was == hi) return lo;
        a = was;                                           // hi had been hooked meanwhile: go on from where it hangs
        b = lo;
    }
    return a < b ? a : b;
}

__global__ __launch_bounds__(kThreads) void clusters_kernel(const float* __restrict__ points, const long long* __restrict__ offsets,
                                                            float r2, int max_points, int* __restrict__ label,
                                                            int* __restrict__ size, int* __restrict__ clusters,
                                                            int* __restrict__ largest) {
#pragma clang fp contract(off)
    extern __shared__ float4 lds[];
    __shared__ int sRoots;
    __shared__ unsigned sBest;
    float4* tile = lds;                                    // kTile + 2 * kGroup entries
    int* parent = reinterpret_cast<int*>(lds + kTile + 2 * kGroup);     // max_points entries
    const int s = blockIdx.x, tid = threadIdx.x;
    const long long lo = offsets[s], len = offsets[s + 1] - lo;
    int* L = label + lo;
    int* Z = size + lo;
    if (len < 1 || len > max_points) {                     // uniform: no row, or a scan beyond the caller's bound
        for (long long i = tid; i < len; i += kThreads) {
            L[i] = -1;
            Z[i] = 0;
        }
        if (tid == 0) {
            clusters[s] = 0;
            largest[s] = -1;
        }
        return;
    }
    const int n = (int)len;
    const float* P = points + lo * 3;
    const unsigned r2bits = (unsigned)__float_as_int(r2);  // r2 >= 0 finite: the bits of d2 order against it as integers
    const int blocks = (n + kThreads - 1) / kThreads;
    for (int i = tid; i < n; i += kThreads) parent[i] = i;
    if (tid == 0) {
        sRoots = 0;
        sBest = 0u;
    }
    const int wave0 = __builtin_amdgcn_readfirstlane(tid & ~(HP_WAVE - 1));    // the wave's first row within a block
    for (int t = 0; t < blocks; ++t) {
        const int t0 = t * kTile;
        const int cnt = n - t0 < kTile ? n - t0 : kTile;
        __syncthreads();                                   // the tile before this one has been read (first pass: parent is set)
        {
            const int c = tid;                             // kTile == kThreads: a lane loads one candidate
            if (c < cnt) {
                const float x = P[(long)(t0 + c) * 3], y = P[(long)(t0 + c) * 3 + 1], z = P[(long)(t0 + c) * 3 + 2];
                const bool ok = finite_bits(x) && finite_bits(y) && finite_bits(z);
                tile[c] = make_float4(x, y, z, __int_as_float(ok ? 0 : (int)kAbsent));
            }
            if (tid < 2 * kGroup) tile[cnt + tid] = make_float4(0.f, 0.f, 0.f, __int_as_float((int)kAbsent));   // absent padding
        }
        __syncthreads();
        for (int b = t; b < blocks; ++b) {                 // the rows at or behind this tile
            const int i = b * kThreads + tid;
            float qx = 0.f, qy = 0.f, qz = 0.f;
            if (i < n) {
                qx = P[(long)i * 3];
                qy = P[(long)i * 3 + 1];
                qz = P[(long)i * 3 + 2];
            }
            const bool mine = i < n && finite_bits(qx) && finite_bits(qy) && finite_bits(qz);
            if (!__any(mine)) continue;
            // candidates of this tile below row i; on the diagonal (b == t) the wave stops at its last row
            const int below = mine ? (i - t0 < cnt ? i - t0 : cnt) : 0;
            const int reach = b == t ? (wave0 + HP_WAVE - 1 < cnt ? wave0 + HP_WAVE - 1 : cnt) : cnt;
            int at = i;                                    // a row of i's tree at or below i: where the next find starts
            float4 next[kGroup];
#pragma unroll
            for (int u = 0; u < kGroup; ++u) next[u] = tile[u];
            for (int c0 = 0; c0 < reach; c0 += kGroup) {
                float4 p[kGroup];
#pragma unroll
                for (int u = 0; u < kGroup; ++u) {
                    p[u] = next[u];
                    next[u] = tile[c0 + kGroup + u];
                }
                bool hit[kGroup];
                bool some = false;
#pragma unroll
                for (int u = 0; u < kGroup; ++u) {
                    const float dx = __fsub_rn(qx, p[u].x), dy = __fsub_rn(qy, p[u].y), dz = __fsub_rn(qz, p[u].z);
                    const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
                    const unsigned bits = (unsigned)__float_as_int(d2) | (unsigned)__float_as_int(p[u].w);
                    hit[u] = bits <= r2bits && c0 + u < below;
                    some = some || hit[u];
                }
                if (__any(some)) {
#pragma unroll
                    for (int u = 0; u < kGroup; ++u)       // a candidate that hangs right under `at` is in i's tree already
                        if (hit[u] && peek(parent + t0 + c0 + u) != at) at = unite(parent, at, t0 + c0 + u, n);
                }
            }
        }
    }
    __syncthreads();                                       // the forest is complete
    for (int i = tid; i < n; i += kThreads) {
        const float x = P[(long)i * 3], y = P[(long)i * 3 + 1], z = P[(long)i * 3 + 2];
        const bool present = finite_bits(x) && finite_bits(y) && finite_bits(z);
        L[i] = present ? find(parent, i, n) : -1;
    }
    __syncthreads();                                       // every label is out: parent turns into the roots' counters
    for (int i = tid; i < n; i += kThreads) parent[i] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += kThreads) {
        const int l = L[i];                                // this thread's own store
        if (l >= 0) atomicAdd(parent + l, 1);
    }
    __syncthreads();
    int roots = 0;
    unsigned best = 0u;
    for (int i = tid; i < n; i += kThreads) {
        const int l = L[i];
        const int z = l >= 0 ? parent[l] : 0;
        Z[i] = z;
        if (l == i) {                                      // a root: size <= 32768 and label < 32768 share 32 bits
            ++roots;
            const unsigned key = ((unsigned)z << 16) | (0xFFFFu - (unsigned)l);
            best = key > best ? key : best;
        }
    }
    if (roots) atomicAdd(&sRoots, roots);
    if (best) atomicMax(&sBest, best);
    __syncthreads();
    if (tid == 0) {
        clusters[s] = sRoots;
        largest[s] = sBest ? (int)(0xFFFFu - (sBest & 0xFFFFu)) : -1;
    }
}

}  // namespace

// The geometry of hp_scan_clusters for a bound on the longest scan: threads per workgroup (= rows per block), candidates per
// LDS tile, and the dynamic LDS bytes of a workgroup.  Host only.
HP_API int hp_scan_clusters_plan(int max_points, int* threads, int* tile, int* lds_bytes) {
    HP_CHECK_ARG(max_points >= 1 && max_points <= kClusterMaxPoints && threads && tile && lds_bytes);
    *threads = kThreads;
    *tile = kTile;
    *lds_bytes = (int)(kTileBytes + (size_t)max_points * sizeof(int));
    return 0;
}

// Euclidean clusters of S ragged scans: label (T), size (T), clusters (S), largest (S); the law is in include/hyperpocket_hip.h.
HP_API int hp_scan_clusters(int S, const float* points, const long long* offsets, float radius, int max_points, int* label,
                            int* size, int* clusters, int* largest, hipStream_t stream) {
    HP_CHECK_ARG(S >= 1 && points && offsets && label && size && clusters && largest);
    HP_CHECK_ARG(max_points >= 1 && max_points <= kClusterMaxPoints);
    HP_CHECK_ARG(radius >= 0.f);                           // refuses a NaN too
    const float r2 = radius * radius;
    HP_CHECK_ARG(r2 <= 3.4028234664e38f);                  // finite
    const size_t lds = kTileBytes + (size_t)max_points * sizeof(int);
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(clusters_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds);
    hipLaunchKernelGGL(clusters_kernel, dim3(S), dim3(kThreads), lds, stream, points, offsets, r2, max_points, label, size,
                       clusters, largest);
    HP_RETURN_LAST_ERROR();
}
