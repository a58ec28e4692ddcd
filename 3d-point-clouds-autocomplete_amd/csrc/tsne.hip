// Exact t-SNE: all-pairs squared distances over long rows, the perplexity calibration, and the O(n^2) gradient
// iterations — the reference's make_tsne_reduction runs scikit-learn's Barnes-Hut t-SNE on the CPU.  The laws are in
// include/hyperpocket_hip.h and, executable, in tests/tsne_law.py.  No float atomics: every sum has one order, two runs
// give the same bits.  -ffp-contract=off: a fused multiply-add is one only where fmaf is written.
//
//   sqdist_kernel       grid (tiles, tiles), upper triangle only.  A workgroup of 256 lanes owns a 64 x 64 tile of pairs, a lane
//                       a 4 x 4 block of it.  Rows are staged k-chunk by k-chunk (64 columns) in LDS, transposed, so a lane reads
//                       its four rows and four columns of one k as two 16-byte words; the next chunk is loaded into registers
//                       meanwhile.  Within a chunk a pair's terms go down one
//                       fmaf chain from +0; the chunk sums are added in chunk order.  Off-diagonal tiles are written twice, as
//                       computed and mirrored; in a diagonal tile (i, j) and (j, i) see negated differences, equal squares and
//                       the same chain, so they hold the same bits, and (i, i) sums zeros.
//   cond_kernel         one workgroup per row.  The row minus its smallest off-diagonal entry sits in LDS across the whole
//                       search; every lane runs the same scalar search on the same block-wide sums, so no lane diverges.
//   cond_total_kernel   the n row sums of C, in row order, in fp64.
//   joint_kernel        32 x 32 tiles through LDS: P_ij = max((C_ij + C_ji) / (2 sum C), eps64), diagonal 0.
//   grad_kernel         one wave per row, 16 rows per workgroup, Y staged in LDS 2048 points at a time; a lane takes
//                       j = lane, lane + 64, ... in ascending order whatever the staging, then a shuffle tree.
//   kl_finish_kernel    KL = sum_i kl_i + log(Z) sum_i p_i in fp64, one workgroup.
//   update_kernel       every workgroup adds the n z_i in the same order in fp64, then the elementwise update.
#include "hp_common.h"

namespace {

constexpr int kMaxN = 16384;            // = HP_TSNE_MAX_POINTS
constexpr int kTile = 64;               // rows and columns of a distance tile
constexpr int kChunk = 64;              // columns of X per staged chunk: the inner level of the two-level sum
constexpr int kPad = kTile + 4;         // LDS row stride: keeps the 16-byte reads aligned
constexpr int kCondThreads = 256;
constexpr int kSearchSteps = 100;
constexpr float kSearchTol = 1e-5f;
constexpr float kEps64 = 2.220446049250313e-16f;
constexpr int kGradRows = 16;           // rows (waves) per workgroup of grad_kernel
constexpr int kGradStage = 2048;        // points of Y in LDS at a time
constexpr int kUpdThreads = 256;
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

// e^x for x <= 0 and log x as the hardware gives them: one v_exp_f32 / v_log_f32 and the one product that changes the base.
__device__ __forceinline__ float hw_exp(float x) { return __builtin_amdgcn_exp2f(x * kLog2e); }
__device__ __forceinline__ float hw_log(float x) { return __builtin_amdgcn_logf(x) * kLn2; }

__global__ __launch_bounds__(256) void sqdist_kernel(int n, int d, const float* __restrict__ X, long ldx, float* __restrict__ D) {
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi) return;                                        // whole workgroup: no barrier is skipped by a part of it
    __shared__ __attribute__((aligned(16))) float As[kChunk][kPad];
    __shared__ __attribute__((aligned(16))) float Bs[kChunk][kPad];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int lc = tid & 63, lr = tid >> 6;
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[r][s] = 0.f;
    // the next chunk travels from memory into registers while the current one is consumed from LDS
    float ra[kTile / 4], rb[kTile / 4];
    auto fetch = [&](int k0) {
        const int k = k0 + lc;
#pragma unroll
        for (int r = 0; r < kTile / 4; ++r) {
            const int gi = bi * kTile + lr + 4 * r, gj = bj * kTile + lr + 4 * r;
            ra[r] = (gi < n && k < d) ? X[(long)gi * ldx + k] : 0.f;           // padding: zero differences, exact +0 terms
            rb[r] = (gj < n && k < d) ? X[(long)gj * ldx + k] : 0.f;
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < d; k0 += kChunk) {
#pragma unroll
        for (int r = 0; r < kTile / 4; ++r) {
            As[lc][lr + 4 * r] = ra[r];
            Bs[lc][lr + 4 * r] = rb[r];
        }
        __syncthreads();
        if (k0 + kChunk < d) fetch(k0 + kChunk);
        float part[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int s = 0; s < 4; ++s) part[r][s] = 0.f;
#pragma unroll 4
        for (int kk = 0; kk < kChunk; ++kk) {
            const float4 a4 = *reinterpret_cast<const float4*>(&As[kk][ty * 4]);
            const float4 b4 = *reinterpret_cast<const float4*>(&Bs[kk][tx * 4]);
            const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float t = a[r] - b[s];
                    part[r][s] = __builtin_fmaf(t, t, part[r][s]);
                }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[r][s] += part[r][s];
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = bi * kTile + ty * 4 + r;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int j = bj * kTile + tx * 4 + s;
            if (i < n && j < n) {
                D[(long)i * n + j] = acc[r][s];
                if (bi != bj) D[(long)j * n + i] = acc[r][s];
            }
        }
    }
}

// Block-wide sum handed to every lane; `scratch` holds blockDim.x / 64 + 1 elements.
template <typename T>
__device__ __forceinline__ T block_sum_all(T v, T* scratch) {
    const T r = hp::block_sum(v, scratch);
    const int nw = (blockDim.x + 63) >> 6;
    if (threadIdx.x == 0) scratch[nw] = r;
    __syncthreads();
    const T out = scratch[nw];
    __syncthreads();
    return out;
}

__global__ __launch_bounds__(kCondThreads) void cond_kernel(int n, const float* __restrict__ D, float log_perp,
                                                            float* __restrict__ C, float* __restrict__ rowsum,
                                                            float* __restrict__ beta_out, int* __restrict__ steps_out) {
    extern __shared__ float row[];                              // n shifted distances
    __shared__ float red[kCondThreads / 64 + 1];
    const int i = blockIdx.x, tid = threadIdx.x;
    const float* Di = D + (long)i * n;
    float m = __builtin_inff();
    for (int j = tid; j < n; j += kCondThreads)
        if (j != i) m = fminf(m, Di[j]);
    m = hp::wave_max(-m);                                       // the minimum, as a maximum of negations: exact either way
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = -fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    for (int j = tid; j < n; j += kCondThreads) row[j] = j == i ? 0.f : Di[j] - m;
    __syncthreads();

    float beta = 1.f, lo = -__builtin_inff(), hi = __builtin_inff(), sum_p = 1.f;
    int steps = 0;
    for (;;) {
        float sp = 0.f, sdp = 0.f;
        for (int j = tid; j < n; j += kCondThreads)
            if (j != i) {
                const float dj = row[j];
                const float p = hw_exp(-(dj * beta));
                sp += p;
                sdp = __builtin_fmaf(dj, p, sdp);
            }
        sum_p = block_sum_all(sp, red);
        const float sum_dp = block_sum_all(sdp, red);
        ++steps;
        const float h = hw_log(sum_p) + (beta * sum_dp) / sum_p;
        const float diff = h - log_perp;
        if (fabsf(diff) <= kSearchTol || steps == kSearchSteps) break;
        if (diff > 0.f) {
            lo = beta;
            beta = hi == __builtin_inff() ? beta * 2.f : (beta + hi) * 0.5f;
        } else {
            hi = beta;
            beta = lo == -__builtin_inff() ? beta * 0.5f : (beta + lo) * 0.5f;
        }
    }
    float rs = 0.f;
    float* Ci = C + (long)i * n;
    for (int j = tid; j < n; j += kCondThreads) {
        const float c = j == i ? 0.f : hw_exp(-(row[j] * beta)) / sum_p;
        Ci[j] = c;
        rs += c;
    }
    rs = hp::block_sum(rs, red);
    if (tid == 0) {
        rowsum[i] = rs;
        beta_out[i] = beta;
        steps_out[i] = steps;
    }
}

__global__ __launch_bounds__(256) void cond_total_kernel(int n, const float* __restrict__ rowsum, float* __restrict__ total) {
    __shared__ double red[256 / 64];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += (double)rowsum[i];
    s = hp::block_sum(s, red);
    if (threadIdx.x == 0) total[0] = (float)(2.0 * s);          // sum over C + C^T
}

__global__ __launch_bounds__(256) void joint_kernel(int n, const float* __restrict__ C, const float* __restrict__ total,
                                                    float* __restrict__ P) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;     // 32 x 8
    const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
    for (int r = ty; r < 32; r += 8) {                          // C[j0 + r][i0 + tx]: the transposed tile
        const int a = j0 + r, b = i0 + tx;
        tile[r][tx] = (a < n && b < n) ? C[(long)a * n + b] : 0.f;
    }
    __syncthreads();
    const float s = total[0];
    for (int r = ty; r < 32; r += 8) {
        const int i = i0 + r, j = j0 + tx;
        if (i < n && j < n) P[(long)i * n + j] = i == j ? 0.f : fmaxf((C[(long)i * n + j] + tile[tx][r]) / s, kEps64);
    }
}

template <bool KL>
__global__ __launch_bounds__(kGradRows * 64) void grad_kernel(int n, const float* __restrict__ P, float ex,
                                                              const float* __restrict__ Y, float* __restrict__ rowacc) {
    __shared__ float2 ys[kGradStage];
    const int tid = threadIdx.x, lane = tid & 63;
    const int i = blockIdx.x * kGradRows + (tid >> 6);
    const bool active = i < n;
    const float2* Y2 = reinterpret_cast<const float2*>(Y);
    const float2 yi = active ? Y2[i] : make_float2(0.f, 0.f);
    const float* Pi = P + (long)(active ? i : 0) * n;
    float ax = 0.f, ay = 0.f, rx = 0.f, ry = 0.f, z = 0.f;
    double kl = 0.0, ps = 0.0;
    for (int j0 = 0; j0 < n; j0 += kGradStage) {
        const int cnt = min(kGradStage, n - j0);
        __syncthreads();
        for (int t = tid; t < cnt; t += kGradRows * 64) ys[t] = Y2[j0 + t];
        __syncthreads();
        if (active)
            for (int jj = lane; jj < cnt; jj += 64) {
                const int j = j0 + jj;
                if (j == i) continue;
                const float2 yj = ys[jj];
                const float p = Pi[j];
                const float dx = yi.x - yj.x, dy = yi.y - yj.y;
                const float w = __builtin_amdgcn_rcpf(1.f + (dx * dx + dy * dy));
                const float pw = (ex * p) * w, w2 = w * w;
                ax = __builtin_fmaf(pw, dx, ax);
                ay = __builtin_fmaf(pw, dy, ay);
                rx = __builtin_fmaf(w2, dx, rx);
                ry = __builtin_fmaf(w2, dy, ry);
                z += w;
                if (KL && p > 0.f) {
                    kl += (double)(p * (hw_log(p) - hw_log(w)));
                    ps += (double)p;
                }
            }
    }
    ax = hp::wave_sum(ax);
    ay = hp::wave_sum(ay);
    rx = hp::wave_sum(rx);
    ry = hp::wave_sum(ry);
    z = hp::wave_sum(z);
    if (KL) {
        kl = hp::wave_sum(kl);
        ps = hp::wave_sum(ps);
    }
    if (active && lane == 0) {
        float* o = rowacc + (long)i * 8;
        o[0] = ax;
        o[1] = ay;
        o[2] = rx;
        o[3] = ry;
        o[4] = z;
        if (KL) {
            o[5] = (float)kl;
            o[6] = (float)ps;
        }
    }
}

__global__ __launch_bounds__(256) void kl_finish_kernel(int n, const float* __restrict__ rowacc, float* __restrict__ out) {
    __shared__ double red[256 / 64];
    double z = 0.0, kl = 0.0, ps = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        z += (double)rowacc[(long)i * 8 + 4];
        kl += (double)rowacc[(long)i * 8 + 5];
        ps += (double)rowacc[(long)i * 8 + 6];
    }
    z = hp::block_sum(z, red);
    kl = hp::block_sum(kl, red);
    ps = hp::block_sum(ps, red);
    if (threadIdx.x == 0) {
        out[0] = (float)(kl + log(z) * ps);
        out[1] = (float)z;
        out[2] = (float)ps;
    }
}

__global__ __launch_bounds__(kUpdThreads) void update_kernel(int n, const float* __restrict__ rowacc, float* __restrict__ Y,
                                                             float* __restrict__ update, float* __restrict__ gains,
                                                             float momentum, float lr, float min_gain,
                                                             float* __restrict__ grad) {
    __shared__ double red[kUpdThreads / 64 + 1];
    double zs = 0.0;
    for (int i = threadIdx.x; i < n; i += kUpdThreads) zs += (double)rowacc[(long)i * 8 + 4];
    const float Z = (float)block_sum_all(zs, red);
    const int i = blockIdx.x * kUpdThreads + threadIdx.x;
    if (i >= n) return;
    const float* a = rowacc + (long)i * 8;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const long e = (long)i * 2 + c;
        const float g = 4.f * (a[c] - a[2 + c] / Z);
        float u = update[e], gn = gains[e];
        const bool inc = u * g < 0.f;
        gn = inc ? gn + 0.2f : gn * 0.8f;
        gn = fmaxf(gn, min_gain);
        u = momentum * u - lr * (g * gn);
        gains[e] = gn;
        update[e] = u;
        Y[e] = Y[e] + u;
        if (grad) grad[e] = g;
    }
}

bool valid_n(int n) { return n >= 2 && n <= kMaxN; }

}  // namespace

HP_API int hp_pairwise_sqdist_plan(int n, int d, int* tile, int* kchunk) {
    HP_CHECK_ARG(valid_n(n) && d >= 1);
    if (tile) *tile = kTile;
    if (kchunk) *kchunk = kChunk;
    return 0;
}

HP_API int hp_pairwise_sqdist(int n, int d, const float* X, long ldx, float* D, hipStream_t stream) {
    HP_CHECK_ARG(valid_n(n) && d >= 1 && ldx >= d && X && D);
    const int tiles = (n + kTile - 1) / kTile;
    hipLaunchKernelGGL(sqdist_kernel, dim3(tiles, tiles), dim3(256), 0, stream, n, d, X, ldx, D);
    HP_RETURN_LAST_ERROR();
}

HP_API long hp_tsne_affinities_workspace_floats(int n) {
    if (!valid_n(n)) return -1;
    return (long)n * n + n + 1;                                 // C, its row sums, their total
}

HP_API int hp_tsne_affinities(int n, const float* D, float perplexity, float* P, float* beta, int* steps, float* ws,
                              hipStream_t stream) {
    HP_CHECK_ARG(valid_n(n) && perplexity > 0.f && perplexity < (float)n && D && P && beta && steps && ws);
    float* C = ws;
    float* rowsum = ws + (long)n * n;
    float* total = rowsum + n;
    const float log_perp = (float)std::log((double)perplexity);
    hipLaunchKernelGGL(cond_kernel, dim3(n), dim3(kCondThreads), (size_t)n * sizeof(float), stream, n, D, log_perp, C, rowsum,
                       beta, steps);
    hipLaunchKernelGGL(cond_total_kernel, dim3(1), dim3(256), 0, stream, n, rowsum, total);
    const int tiles = (n + 31) / 32;
    hipLaunchKernelGGL(joint_kernel, dim3(tiles, tiles), dim3(256), 0, stream, n, C, total, P);
    HP_RETURN_LAST_ERROR();
}

HP_API int hp_tsne_gradient(int n, const float* P, float exaggeration, const float* Y, float* rowacc, float* kl,
                            hipStream_t stream) {
    HP_CHECK_ARG(valid_n(n) && P && Y && rowacc);
    const int blocks = (n + kGradRows - 1) / kGradRows;
    if (kl) {
        hipLaunchKernelGGL(grad_kernel<true>, dim3(blocks), dim3(kGradRows * 64), 0, stream, n, P, exaggeration, Y, rowacc);
        hipLaunchKernelGGL(kl_finish_kernel, dim3(1), dim3(256), 0, stream, n, rowacc, kl);
    } else {
        hipLaunchKernelGGL(grad_kernel<false>, dim3(blocks), dim3(kGradRows * 64), 0, stream, n, P, exaggeration, Y, rowacc);
    }
    HP_RETURN_LAST_ERROR();
}

HP_API int hp_tsne_update(int n, const float* rowacc, float* Y, float* update, float* gains, float momentum, float lr,
                          float min_gain, float* grad, hipStream_t stream) {
    HP_CHECK_ARG(valid_n(n) && rowacc && Y && update && gains);
    hipLaunchKernelGGL(update_kernel, dim3((n + kUpdThreads - 1) / kUpdThreads), dim3(kUpdThreads), 0, stream, n, rowacc, Y,
                       update, gains, momentum, lr, min_gain, grad);
    HP_RETURN_LAST_ERROR();
}

HP_API int hp_tsne_descend(int n, const float* P, float* Y, float* update, float* gains, float* rowacc, int it0, int iters,
                           int explore, float exaggeration, float lr, float* kl_out, hipStream_t stream) {
    HP_CHECK_ARG(valid_n(n) && P && Y && update && gains && rowacc && it0 >= 0 && iters >= 0);
    for (int it = it0; it < it0 + iters; ++it) {
        const bool early = it < explore;
        int rc = hp_tsne_gradient(n, P, early ? exaggeration : 1.f, Y, rowacc, nullptr, stream);
        if (rc) return rc;
        rc = hp_tsne_update(n, rowacc, Y, update, gains, early ? 0.5f : 0.8f, lr, 0.01f, nullptr, stream);
        if (rc) return rc;
    }
    if (kl_out) return hp_tsne_gradient(n, P, 1.f, Y, rowacc, kl_out, stream);
    return 0;
}
