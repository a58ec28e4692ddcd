// Cut by coordinate rank: each of B clouds sorted along one axis and split at row k, in one launch — the
// operation behind the reference's `gt[gt.T[0].argsort()[1024:]]` / `[:1024]`.
//
// The law, per cloud of n rows with c_i the `axis` coordinate of row i (include/hyperpocket_hip.h has it in full):
//   order = the rows sorted by (key(c_i), i) ascending — numpy's float32 order, -0 = +0, NaN after +inf, equal keys by index
//   lower = rows order[0..k), upper = rows order[k..n), every row copied bit for bit
//
//   grid (B), one workgroup per cloud.  A row becomes one 64-bit key: high word the order-preserving uint32 image of c_i
//   (sign bit flipped for c >= 0, all bits for c < 0; -0 first made +0, every NaN made 0xFFFFFFFF), low word i.  Keys of a
//   cloud are distinct, so an unsigned sort of them is total and is the stable sort of the law whatever network does it.
//   The keys sit in LDS, padded to a power of two with ~0 (above every real key: a real low word is below 8192), and go
//   through a bitonic network: log2(N) * (log2(N) + 1) / 2 compare-exchange passes, one barrier each, every thread
//   owning whole pairs so no two threads touch one slot between barriers.  Rank r then holds row order[r] in its low word:
//   the outputs are written as flat floats, consecutive lanes to consecutive addresses, each value fetched from its row
//   of the cloud.  Plain vector loads and stores, no atomics, no global scratch.
#include "hp_common.h"

namespace {

constexpr int kAxisSplitMaxPoints = 8192;  // = HP_AXIS_SPLIT_MAX_POINTS (include/hyperpocket_hip.h)
constexpr int kMaxThreads = 1024;

// numpy's float32 `<` order with -0 = +0 and every NaN last, as an unsigned integer order.
__device__ __forceinline__ unsigned order_image(float c) {
    unsigned u = (unsigned)__float_as_int(c);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;    // NaN, either sign, any payload
    if (u == 0x80000000u) u = 0u;                               // -0 -> +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(kMaxThreads) void axis_split_kernel(int n, int N /* power of two >= n */,
                                                                 const float* __restrict__ clouds, int axis, int k,
                                                                 float* __restrict__ lower, float* __restrict__ upper,
                                                                 int* __restrict__ order) {
    extern __shared__ unsigned long long keys[];                // N of them
    const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    const float* C = clouds + (long)b * n * 3;
    for (int i = tid; i < N; i += T)
        keys[i] = i < n ? ((unsigned long long)order_image(C[i * 3 + axis]) << 32) | (unsigned)i : ~0ull;
    for (int size = 2; size <= N; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = tid; t < (N >> 1); t += T) {
                const int lo = 2 * t - (t & (stride - 1));      // the t-th slot whose `stride` bit is clear
                const int hi = lo + stride;
                const unsigned long long a = keys[lo], c = keys[hi];
                if ((a > c) == ((lo & size) == 0)) {            // ascending runs where the `size` bit is clear
                    keys[lo] = c;
                    keys[hi] = a;
                }
            }
        }
    }
    __syncthreads();
    if (order) {
        int* O = order + (long)b * n;
        for (int r = tid; r < n; r += T) O[r] = (int)(unsigned)keys[r];
    }
    float* L = lower + (long)b * k * 3;
    float* U = upper + (long)b * (n - k) * 3;
    const int cut = 3 * k;
    for (int e = tid; e < 3 * n; e += T) {
        const int r = e / 3;
        const float v = C[(int)(unsigned)keys[r] * 3 + (e - 3 * r)];
        if (e < cut)
            L[e] = v;
        else
            U[e - cut] = v;
    }
}

}  // namespace

// Sort each of B clouds (B,n,3) along `axis` and split it at row k: see the law at the top and include/hyperpocket_hip.h.
HP_API int hp_axis_split(int B, int n, const float* clouds, int axis, int k, float* lower, float* upper, int* order,
                         hipStream_t stream) {
    HP_CHECK_ARG(B >= 0 && n >= 2 && n <= kAxisSplitMaxPoints && k >= 1 && k <= n - 1 && axis >= 0 && axis <= 2);
    HP_CHECK_ARG(clouds && lower && upper);
    if (B == 0) return 0;
    int N = 2;
    while (N < n) N <<= 1;
    const int threads = std::min(std::max(N / 2, HP_WAVE), kMaxThreads);    // a pair per thread, up to 4 at N = 8192
    hipLaunchKernelGGL(axis_split_kernel, dim3(B), dim3(threads), (size_t)N * sizeof(unsigned long long), stream, n, N, clouds,
                       axis, k, lower, upper, order);
    HP_RETURN_LAST_ERROR();
}
