// Exact EMD: the minimum-cost one-to-one matching of two equal-sized clouds, over a list of cloud pairs.
//
// New ground (the reference has only the approximate matching of approxmatch.cu): a forward Jacobi auction with
// eps-scaling held entirely in integers.  The law — costs, bids, tie rules, phases — is tests/assign_law.py, and this
// kernel follows it bit for bit: assignment, cost and the number of rounds.
//
// Design:
//  * one workgroup solves one pair from start to end; workgroups stride over the pair list, so P is not a grid dimension.
//  * everything lives in LDS, 60 bytes per point: both clouds (SoA), the int64 prices, the owner of every object, the two
//    lists of unassigned bidders (this round's, the next round's) and per bidder of the round its bid and its object.
//    No global scratch and no n x n matrix: a bidder recomputes its row of costs in every scan.
//  * a round is four stages between barriers:
//      scan     one wave per unassigned bidder; a lane walks a strided slice of the objects keeping (best value, lowest
//               index) and the second-best value; a butterfly merges the lanes under the same rules
//      raise    price[j] = max(price[j], bid) — a bid exceeds the price it was computed from, so after this stage the price of
//               an object that received bids IS its winning bid (integer LDS atomic max)
//      winner   the lowest bidder among those whose bid equals the new price (integer LDS atomic min)
//      apply    the winner takes the object, its previous owner and every loser go on the next round's list
//    Every rule is a max, a min or a lowest index over integers: no result depends on the order in which waves or lanes arrive
//    (the order inside the unassigned list does vary, and decides only which wave scans for which bidder).
//  * every loop is bounded: the rounds of a pair by max_rounds, its phases by the 42 bits eps can have.
#include "hp_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxPoints = 2048;                // = HP_ASSIGN_MAX_POINTS (include/hyperpocket_hip.h)
constexpr int kTheta = 4;                       // tests/assign_law.py THETA
constexpr float kQMax = 1073741824.f;           // 2^30
constexpr int kMaxPhases = 64;
constexpr int kCUs = 256;                       // MI355X; only sizes the grid, the workgroups stride over the pairs
constexpr size_t kLdsPerCU = 160 * 1024;
constexpr long long kI64Min = (long long)0x8000000000000000ULL;

enum Status { kCapped = -1, kBadPair = -2, kOverflow = -3 };

struct AssignArgs {
    const float* A;        // (na, n, 3)
    const float* B;        // (nb, n, 3)
    const int* ab;         // (pairs, 2)
    int* assignment;       // (pairs, n) or NULL
    long long* cost;       // (pairs)
    int* rounds;           // (pairs)
    long pairs;
    long max_rounds;
    int na, nb, n;
    float scale;           // 2^scale_log2
};

// rint(sqrt_f32(d2) * scale) as a float: the law's q before the integer cast.  Separate roundings, no contraction.
__device__ __forceinline__ float quantised(float ax, float ay, float az, float bx, float by, float bz, float scale) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    return rintf(sqrtf(d2) * scale);
}

struct Best {
    long long v1, v2;
    int j1;
};

// two disjoint sets of objects: the best of both (lowest index among equals) and the second-best of their union
__device__ __forceinline__ Best merge(const Best& a, const Best& b) {
    Best r;
    const bool take_b = b.v1 > a.v1 || (b.v1 == a.v1 && b.j1 < a.j1);
    r.v1 = take_b ? b.v1 : a.v1;
    r.j1 = take_b ? b.j1 : a.j1;
    const long long low = take_b ? a.v1 : b.v1;
    r.v2 = max(max(a.v2, b.v2), low);
    return r;
}

__global__ __launch_bounds__(1024) void assign_pairs_kernel(const AssignArgs p) {
    extern __shared__ long long lds[];
    const int n = p.n, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    long long* price = lds;                     // (n) of every object
    long long* bidval = price + n;              // (n) by position in the round's list
    long long* costsum = bidval + n;            // (1)
    int* small = (int*)(costsum + 1);           // count[2], qmax, overflow
    float* bx = (float*)(small + 4);
    float *by = bx + n, *bz = by + n, *ax = bz + n, *ay = ax + n, *az = ay + n;
    int* owner = (int*)(az + n);                // (n) bidder that holds the object, or -1
    int* winner = owner + n;                    // (n) lowest bidder at the winning bid
    int* bidobj = winner + n;                   // (n) by position in the round's list
    int* list0 = bidobj + n;                    // (n) x 2 unassigned bidders
    const long long np1 = n + 1;

    for (long pair = blockIdx.x; pair < p.pairs; pair += gridDim.x) {
        __syncthreads();                        // the previous pair's LDS is dead
        const int ia = p.ab[pair * 2], ib = p.ab[pair * 2 + 1];
        int status = 0;
        long rounds = 0;
        if ((unsigned)ia >= (unsigned)p.na || (unsigned)ib >= (unsigned)p.nb) status = kBadPair;

        if (!status) {
            const float* a = p.A + (size_t)ia * n * 3;
            const float* b = p.B + (size_t)ib * n * 3;
            for (int i = tid; i < n; i += nt) {
                ax[i] = a[i * 3 + 0];
                ay[i] = a[i * 3 + 1];
                az[i] = a[i * 3 + 2];
                bx[i] = b[i * 3 + 0];
                by[i] = b[i * 3 + 1];
                bz[i] = b[i * 3 + 2];
                price[i] = 0;
            }
            if (tid == 0) {
                small[2] = 0;
                small[3] = 0;
                *costsum = 0;
            }
            __syncthreads();
            // the largest q, and whether any overflows
            int qmax = 0, bad = 0;
            for (int i = wave; i < n; i += nw) {
                const float x = ax[i], y = ay[i], z = az[i];
                for (int j = lane; j < n; j += 64) {
                    const float r = quantised(x, y, z, bx[j], by[j], bz[j], p.scale);
                    if (r <= kQMax) qmax = max(qmax, (int)r);
                    else bad = 1;               // too large, or NaN
                }
            }
            atomicMax(&small[2], qmax);
            if (bad) atomicOr(&small[3], 1);
            __syncthreads();
            if (small[3]) status = kOverflow;
        }

        if (!status) {
            long long eps = max((long long)small[2] * np1 / 2, 1LL);
            for (int phase = 0; phase < kMaxPhases; ++phase) {
                __syncthreads();                // every thread has read the last round's count
                for (int i = tid; i < n; i += nt) {
                    owner[i] = -1;
                    list0[i] = i;
                }
                if (tid == 0) small[0] = n;
                __syncthreads();
                int cur = 0, count = n;
                while (count > 0) {
                    if (rounds >= p.max_rounds) {
                        status = kCapped;
                        break;
                    }
                    ++rounds;
                    const int* list = list0 + cur * n;
                    int* next = list0 + (cur ^ 1) * n;
                    // scan: one wave per bidder
                    for (int k = wave; k < count; k += nw) {
                        const int i = list[k];
                        const float x = ax[i], y = ay[i], z = az[i];
                        Best m{kI64Min, kI64Min, 0x7fffffff};
#pragma unroll 4
                        for (int j = lane; j < n; j += 64) {
                            const int q = (int)quantised(x, y, z, bx[j], by[j], bz[j], p.scale);
                            const long long v = -(long long)q * np1 - price[j];
                            if (v > m.v1) {     // j ascends: an equal value keeps the lower index and becomes the second
                                m.v2 = m.v1;
                                m.v1 = v;
                                m.j1 = j;
                            } else if (v > m.v2) {
                                m.v2 = v;
                            }
                        }
#pragma unroll
                        for (int o = 1; o < 64; o <<= 1) {
                            Best t;
                            t.v1 = __shfl_xor(m.v1, o, 64);
                            t.v2 = __shfl_xor(m.v2, o, 64);
                            t.j1 = __shfl_xor(m.j1, o, 64);
                            m = merge(m, t);
                        }
                        if (lane == 0) {
                            const long long v2 = n > 1 ? m.v2 : m.v1;
                            bidval[k] = price[m.j1] + (m.v1 - v2) + eps;
                            bidobj[k] = m.j1;
                            winner[m.j1] = 0x7fffffff;
                        }
                    }
                    __syncthreads();
                    // raise: the price of an object becomes its highest bid
                    for (int k = tid; k < count; k += nt) atomicMax(&price[bidobj[k]], bidval[k]);
                    if (tid == 0) small[cur ^ 1] = 0;
                    __syncthreads();
                    // winner: the lowest bidder at that bid
                    for (int k = tid; k < count; k += nt) {
                        const int j = bidobj[k];
                        if (bidval[k] == price[j]) atomicMin(&winner[j], list[k]);
                    }
                    __syncthreads();
                    // apply
                    for (int k = tid; k < count; k += nt) {
                        const int i = list[k], j = bidobj[k];
                        int out = i;
                        if (winner[j] == i) {
                            out = owner[j];
                            owner[j] = i;
                        }
                        if (out >= 0) next[atomicAdd(&small[cur ^ 1], 1)] = out;
                    }
                    __syncthreads();
                    cur ^= 1;
                    count = small[cur];
                }
                if (status || eps == 1) break;
                eps = max(eps / kTheta, 1LL);
            }
        }

        if (!status) {
            long long c = 0;
            for (int j = tid; j < n; j += nt) {
                const int i = owner[j];
                if (p.assignment) p.assignment[pair * n + i] = j;
                c += (int)quantised(ax[i], ay[i], az[i], bx[j], by[j], bz[j], p.scale);
            }
            atomicAdd((unsigned long long*)costsum, (unsigned long long)c);
            __syncthreads();
            if (tid == 0) {
                p.cost[pair] = *costsum;
                p.rounds[pair] = (int)rounds;
            }
        } else {
            if (p.assignment)
                for (int i = tid; i < n; i += nt) p.assignment[pair * n + i] = -1;
            if (tid == 0) {
                p.cost[pair] = -1;
                p.rounds[pair] = status;
            }
        }
    }
}

inline size_t lds_bytes(int n) { return (size_t)n * 60 + 8 + 16; }

// 256 threads while several pairs share a CU, more waves per pair once LDS leaves room for one or two workgroups
inline int threads_for(int n) { return n <= 512 ? 256 : n <= 1024 ? 512 : 1024; }

}  // namespace

// ================================================================================================
// C ABI
// ================================================================================================

// The round bound hp_assign_pairs uses for max_rounds = 0: 256 n + 1024.  The law's largest round counts over the host suite's
// families (tests/test_assign_law_host.py derives them) stay below an eighth of it at every n tested: 35.5 k rounds at
// n = 2048 (tie-heavy grid), 19.7 k at 1024, 3.5 k at 256, 1.4 k at 64, 42 at n = 3.
HP_API long hp_assign_default_max_rounds(int n) {
    if (n < 1 || n > kMaxPoints) return -1;
    return 256L * n + 1024;
}

HP_API int hp_assign_pairs(int na, int n, const float* A, int nb, const float* B, long pairs, const int* pair_ab, int scale_log2,
                           long max_rounds, int* assignment, long long* cost, int* rounds, hipStream_t stream) {
    HP_CHECK_ARG(na > 0 && nb > 0 && pairs >= 0);
    HP_CHECK_ARG(n >= 1 && n <= kMaxPoints);
    HP_CHECK_ARG(scale_log2 >= 0 && scale_log2 <= 24);
    HP_CHECK_ARG(max_rounds >= 0 && max_rounds <= 0x7fffffffL);
    if (pairs == 0) return 0;
    HP_CHECK_ARG(A && B && pair_ab && cost && rounds);
    const size_t lds = lds_bytes(n);
    const int threads = threads_for(n);
    const long resident = std::min<long>(kLdsPerCU / lds, 2048 / threads);
    AssignArgs a{A, B, pair_ab, assignment, cost, rounds, pairs, max_rounds ? max_rounds : hp_assign_default_max_rounds(n),
                 na, nb, n, (float)(1 << scale_log2)};
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(assign_pairs_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds);
    hipLaunchKernelGGL(assign_pairs_kernel, dim3((unsigned)std::min<long>(pairs, kCUs * resident)), dim3(threads), lds, stream, a);
    HP_RETURN_LAST_ERROR();
}
