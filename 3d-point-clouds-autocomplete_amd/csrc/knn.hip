// k nearest neighbours over ragged scans, and statistical outlier removal on top of them — what a real scan
// with flying pixels needs before its bounding box means anything.
//
// The law, per scan (include/hyperpocket_hip.h and tests/knn_law.py have it in full):
//   d2(i, j) = ((dx*dx + dy*dy) + dz*dz), every operation one fp32 rounding, no contraction (fps.hip's formula)
//   a row with a non-finite coordinate is absent: nobody's candidate, and as a query it gets the empty result
//   the candidates of query i — the present rows j of its scan, j != i under exclude_self — ordered by (bits of d2, j); the
//   first k of them are the result, slots beyond the candidates hold index -1 and dist2 +inf
// With finite coordinates d2 is never NaN: a difference is finite or +-inf, a square non-negative, and a sum of non-negative
// terms never meets inf - inf.  So the bits of d2 order as unsigned integers, +inf (an overflow) included.
//
//   knn      grid-stride over chunks of 256 consecutive query rows of the whole ragged set, one lane per query.  A chunk walks
//            the scans its rows belong to (scan boundaries fall anywhere in a chunk or a wave): the scan's candidates pass
//            through an LDS tile of 1024 float4 (x, y, z, absent mask) that every lane reads at the same address — a
//            broadcast, no bank conflicts — and only the lanes whose query is a present row of that scan take part.  A lane
//            keeps its K best (d2 bits, row) sorted in registers.  Candidates arrive in ascending row order, so one with a
//            distance equal to the current worst can never displace it: the test in the sweep is one 32-bit compare
//            `bits < worst`, and the insertion — a chain unrolled over compile-time slots, stable, so equal distances stay in
//            row order — runs only behind it.  The absent mask is or-ed into the bits (all ones: never below any worst), an
//            empty slot holds all ones too (no distance has these bits).
//            A lane passes that test k ln(n/k) times in a sweep, but some lane of a wave passes it at most candidates, and
//            the whole wave would pay the chain each time.  So a candidate that passes is only appended to the lane's queue
//            (8 slots in LDS, indexed at run time — registers could not be) and the wave inserts when a queue could
//            overflow with the next group of 4 candidates, and at the end of a tile: then every lane has work in the chain.
//            The queue keeps row order and every entry is tested again against the worst of that moment, so the list is the
//            one immediate insertion gives; a candidate held back by a stale worst would have failed the fresh one too.
//            The tile is read a group ahead into registers: the next group's four reads are in flight behind this
//            group's work.
//            No atomics, no global scratch.
//            MEAN: instead of the lists the kernel writes m_i, the fp64 mean of the square roots of the list, as fp32.
//   stats    grid (S), one workgroup per scan, over the m_i: M and the participants' count, then the integers q_i, their
//            sums S1 and S2 through 64-bit integer atomics in LDS (no order to depend on), then the threshold in fp64 with
//            one rounding per operation, identically in every thread, and keep / kept.
#include "hp_knn.h"

namespace {

using hp::finite_bits, hp::kInfBits;
using hp_knn::insert, hp_knn::kEmpty;          // hp_knn.h: shared with knn_grid.hip
constexpr int kKnnMaxPoints = 65536;       // = HP_KNN_MAX_POINTS (include/hyperpocket_hip.h)
constexpr int kKnnMaxK = hp_knn::kMaxK;
constexpr int kThreads = 256;              // queries per chunk
constexpr int kTile = 1024;                // candidates per LDS tile (16 KiB)
constexpr int kQueue = 8;                  // candidates a lane can hold back before the wave inserts (16 KiB of LDS)
constexpr int kGroup = 4;                  // candidates between two looks at the queues; kTile is a multiple
constexpr int kGrid = 2048;                // workgroups of a launch: the chunk count lives on the device (offsets[S])
constexpr int kStatThreads = 1024;

template <int K, bool MEAN>
__global__ __launch_bounds__(kThreads) void knn_kernel(int S, const float* __restrict__ points, const long long* __restrict__ offsets,
                                                       const float* __restrict__ queries, const long long* __restrict__ qoffsets,
                                                       int k, int exclude_self, int* __restrict__ index,
                                                       float* __restrict__ dist2, float* __restrict__ mean_dist) {
#pragma clang fp contract(off)
    __shared__ float4 tile[kTile + 2 * kGroup];
    __shared__ uint2 pend[kQueue][kThreads];
    const int tid = threadIdx.x;
    const long long Q = qoffsets[S];
    for (long long row0 = (long long)blockIdx.x * kThreads; row0 < Q; row0 += (long long)gridDim.x * kThreads) {
        const long long q = row0 + tid;
        const bool have = q < Q;
        float qx = 0.f, qy = 0.f, qz = 0.f;
        if (have) {
            qx = queries[q * 3];
            qy = queries[q * 3 + 1];
            qz = queries[q * 3 + 2];
        }
        const bool present = have && finite_bits(qx) && finite_bits(qy) && finite_bits(qz);
        unsigned d[K];
        int j[K];
#pragma unroll
        for (int t = 0; t < K; ++t) {
            d[t] = kEmpty;
            j[t] = -1;
        }
        int pending = 0;                                   // this lane's candidates in pend[0 .. pending)[tid], in row order
        auto drain = [&]() {
            for (int e = 0; __any(e < pending); ++e) {
                if (e < pending) {
                    const uint2 v = pend[e][tid];
                    if (v.x < d[K - 1]) insert<K>(d, j, v.x, (int)v.y);
                }
            }
            pending = 0;
        };
        int s = 0;                                         // the scan of row0: the last s with qoffsets[s] <= row0
        for (int hi = S; hi - s > 1;) {
            const int mid = (s + hi) >> 1;
            if (qoffsets[mid] <= row0) s = mid;
            else hi = mid;
        }
        const long long last = (row0 + kThreads < Q ? row0 + kThreads : Q) - 1;
        for (; s < S && qoffsets[s] <= last; ++s) {        // every value that steers these loops is uniform over the workgroup
            const long long qlo = qoffsets[s], qhi = qoffsets[s + 1];
            const long long plo = offsets[s], cand = offsets[s + 1] - plo;
            if (qhi <= qlo || cand < 1 || cand > kKnnMaxPoints) continue;    // no query, no candidate, or a scan beyond the cap
            const int n = (int)cand;
            const bool mine = present && q >= qlo && q < qhi;
            const int self = mine && exclude_self ? (int)(q - qlo) : -1;
            const float* P = points + plo * 3;
            for (int t0 = 0; t0 < n; t0 += kTile) {
                const int cnt = n - t0 < kTile ? n - t0 : kTile;
                __syncthreads();                           // the tile before this one has been read
                for (int c = tid; c < cnt; c += kThreads) {
                    const float x = P[(long)(t0 + c) * 3], y = P[(long)(t0 + c) * 3 + 1], z = P[(long)(t0 + c) * 3 + 2];
                    tile[c] = make_float4(x, y, z, hp_knn::absent_mask(x, y, z));
                }
                if (tid < 2 * kGroup) tile[cnt + tid] = make_float4(0.f, 0.f, 0.f, __int_as_float((int)kEmpty));   // absent padding
                __syncthreads();
                if (mine) {
                    float4 next[kGroup];                   // a group ahead: the LDS latency hides behind the group at hand
#pragma unroll
                    for (int u = 0; u < kGroup; ++u) next[u] = tile[u];
                    for (int c0 = 0; c0 < cnt; c0 += kGroup) {
                        float4 p[kGroup];
#pragma unroll
                        for (int u = 0; u < kGroup; ++u) {
                            p[u] = next[u];
                            next[u] = tile[c0 + kGroup + u];
                        }
                        if (__any(pending > kQueue - kGroup)) drain();      // room for a whole group in every lane
                        unsigned bits[kGroup];
#pragma unroll
                        for (int u = 0; u < kGroup; ++u) {
                            bits[u] = hp_knn::d2_bits(qx, qy, qz, p[u].x, p[u].y, p[u].z) | (unsigned)__float_as_int(p[u].w);
                        }
#pragma unroll
                        for (int u = 0; u < kGroup; ++u) {
                            if (bits[u] < d[K - 1] && t0 + c0 + u != self) {    // d[K-1]: the worst as of the last drain
                                pend[pending][tid] = make_uint2(bits[u], (unsigned)(t0 + c0 + u));
                                ++pending;
                            }
                        }
                    }
                    drain();
                }
            }
        }
        if (!have) continue;
        if (MEAN) {                                        // m_i: fp64 sum of the roots in slot order, / their number, as fp32
            const float m = hp_knn::mean_root<K>(d, k);
            mean_dist[q] = m;                              // +inf: no neighbour, or an overflowed distance among them
        } else {
#pragma unroll
            for (int t = 0; t < K; ++t) {
                if (t < k) {
                    index[q * k + t] = j[t];
                    dist2[q * k + t] = __int_as_float((int)(d[t] == kEmpty ? kInfBits : d[t]));
                }
            }
        }
    }
}

// Per scan: which rows stay.  m = mean_dist; a row takes part when its m is finite.
__global__ __launch_bounds__(kStatThreads) void outlier_stats_kernel(const float* __restrict__ mean_dist,
                                                                     const long long* __restrict__ offsets, float ratio,
                                                                     unsigned char* __restrict__ keep, int* __restrict__ kept) {
#pragma clang fp contract(off)
    __shared__ unsigned sM;
    __shared__ int sN, sKept;
    __shared__ unsigned long long sS1, sS2;
    const int s = blockIdx.x, tid = threadIdx.x;
    const long long lo = offsets[s], n = offsets[s + 1] - lo;
    const float* m = mean_dist + lo;
    unsigned char* K = keep + lo;
    if (tid == 0) {
        sM = 0u;
        sN = 0;
        sKept = 0;
        sS1 = 0ull;
        sS2 = 0ull;
    }
    __syncthreads();
    unsigned mx = 0u;
    int cnt = 0;
    for (long long i = tid; i < n; i += kStatThreads) {
        const unsigned b = (unsigned)__float_as_int(m[i]);     // m >= 0: the bits order as integers
        if (b < kInfBits) {
            mx = b > mx ? b : mx;
            ++cnt;
        }
    }
    atomicMax(&sM, mx);
    atomicAdd(&sN, cnt);
    __syncthreads();
    const unsigned M = sM;
    const int np = sN;
    if (np <= 1 || M == 0u) {                              // uniform: nothing to compare, every participant stays
        for (long long i = tid; i < n; i += kStatThreads) K[i] = (unsigned)__float_as_int(m[i]) < kInfBits ? 1 : 0;
        if (tid == 0) kept[s] = np;
        return;
    }
    // e = floor(log2 M) from the bits (a subnormal M has its leading bit below 2^-126); q = trunc(m * 2^(23-e)) < 2^24, exact
    const int field = (int)(M >> 23);
    const int e = field ? field - 127 : (31 - __clz((int)(M & 0x7FFFFFu))) - 149;
    const double scale = __longlong_as_double((long long)(1023 + 23 - e) << 52);
    auto quant = [&](float v) { return (unsigned)__dmul_rn((double)v, scale); };
    unsigned long long s1 = 0ull, s2 = 0ull;
    for (long long i = tid; i < n; i += kStatThreads) {
        const float v = m[i];
        if ((unsigned)__float_as_int(v) < kInfBits) {
            const unsigned long long qi = quant(v);
            s1 += qi;
            s2 += qi * qi;
        }
    }
    atomicAdd(&sS1, s1);
    atomicAdd(&sS2, s2);
    __syncthreads();
    const double S1 = __ull2double_rn(sS1), S2 = __ull2double_rn(sS2);
    const double mu = __ddiv_rn(S1, (double)np);
    double var = __ddiv_rn(__dsub_rn(S2, __dmul_rn(mu, S1)), (double)(np - 1));
    var = var > 0.0 ? var : 0.0;
    const double thr = __dadd_rn(mu, __dmul_rn((double)ratio, __dsqrt_rn(var)));
    int stay = 0;
    for (long long i = tid; i < n; i += kStatThreads) {
        const float v = m[i];
        const bool in = (unsigned)__float_as_int(v) < kInfBits && (double)quant(v) <= thr;
        K[i] = in ? 1 : 0;
        stay += (int)in;
    }
    atomicAdd(&sKept, stay);
    __syncthreads();
    if (tid == 0) kept[s] = sKept;
}

template <bool MEAN>
int launch_knn(int S, const float* points, const long long* offsets, const float* queries, const long long* qoffsets, int k,
               int exclude_self, int* index, float* dist2, float* mean_dist, hipStream_t stream) {
#define HP_KNN_CASE(KK)                                                                                                      \
    if (k <= KK) {                                                                                                           \
        hipLaunchKernelGGL((knn_kernel<KK, MEAN>), dim3(kGrid), dim3(kThreads), 0, stream, S, points, offsets, queries, qoffsets, \
                           k, exclude_self, index, dist2, mean_dist);                                                        \
        HP_RETURN_LAST_ERROR();                                                                                              \
    }
    HP_KNN_CASE(8)
    HP_KNN_CASE(16)
    HP_KNN_CASE(32)
#undef HP_KNN_CASE
    return -1;
}

}  // namespace

// The instance hp_knn_points launches for k: its compile-time list length, threads per workgroup (= queries per chunk) and
// candidates per LDS tile.  Host only.
HP_API int hp_knn_points_plan(int k, int* instance_k, int* threads, int* tile) {
    HP_CHECK_ARG(k >= 1 && k <= kKnnMaxK && instance_k && threads && tile);
    *instance_k = k <= 8 ? 8 : k <= 16 ? 16 : 32;
    *threads = kThreads;
    *tile = kTile;
    return 0;
}

// The k nearest rows of its scan for every query of S ragged scans: see the law at the top and include/hyperpocket_hip.h.
HP_API int hp_knn_points(int S, const float* points, const long long* offsets, const float* queries, const long long* query_offsets,
                         int k, int exclude_self, int* index, float* dist2, hipStream_t stream) {
    HP_CHECK_ARG(S >= 1 && k >= 1 && k <= kKnnMaxK && (exclude_self == 0 || exclude_self == 1));
    HP_CHECK_ARG(points && offsets && index && dist2);
    HP_CHECK_ARG((queries == nullptr) == (query_offsets == nullptr));
    const bool own = queries == nullptr || queries == points;
    HP_CHECK_ARG(!own || exclude_self == 1);               // a scan queried with itself: every row would find itself first
    return launch_knn<false>(S, points, offsets, queries ? queries : points, queries ? query_offsets : offsets, k, exclude_self,
                             index, dist2, nullptr, stream);
}

// Statistical outlier removal of S ragged scans: keep (T), mean_dist (T), kept (S); the law is in include/hyperpocket_hip.h.
HP_API int hp_scan_outliers(int S, const float* points, const long long* offsets, int k, float ratio, unsigned char* keep,
                            float* mean_dist, int* kept, hipStream_t stream) {
    HP_CHECK_ARG(S >= 1 && k >= 1 && k <= kKnnMaxK && ratio >= 0.f && ratio <= 3.0e38f);
    HP_CHECK_ARG(points && offsets && keep && mean_dist && kept);
    const int rc = launch_knn<true>(S, points, offsets, points, offsets, k, 1, nullptr, nullptr, mean_dist, stream);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(outlier_stats_kernel, dim3(S), dim3(kStatThreads), 0, stream, mean_dist, offsets, ratio, keep, kept);
    HP_RETURN_LAST_ERROR();
}
