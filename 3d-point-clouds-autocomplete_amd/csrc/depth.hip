// Depth images in, cleaned world points out: the front door of the real-scan chain.  A batch of B depth images of
// H x W pixels with intrinsics, poses and optional instance masks becomes one ragged set — the pixels that are measured, in range,
// masked in and not at a depth edge, back-projected and posed, each with a sensor-facing normal from its four neighbours and
// its pixel number — in image, row, column order.
//
// The law, per pixel (v, u) of image b (include/hyperpocket_hip.h and tests/depth_law.py have it in full; every operation is one
// fp64 rounding, no contraction, the only library function a correctly rounded square root):
//   z = double(d) * scale, measured when finite and > 0; jump(a, b) = |a - b| > jump_abs + jump_rel * min(a, b);
//   kept: measured, near <= z <= far, mask != 0, and no measured pixel within w jumps against it (hp_depth.h, shared with fuse.hip);
//   q = (((u - cx) * z) / fx, ((v - cy) * z) / fy, z); normal = (right - left) x (down - up) over the usable neighbours, turned
//   to the sensor, normalised or zero; p = R q + t, n = R n, cast to fp32 once.
//
// Three launches whatever the images hold.  A chunk is kChunk consecutive row-major pixels of one image; chunks never cross images.
//   count  a workgroup per chunk (grid-stride): the keep test of its pixels, one per lane and slab of kThreads, and their number
//          into ws[chunk] (uint32).
//   scan   one workgroup of kScanThreads lanes walks the chunks kScanThreads at a time: ws[chunk] becomes the number of kept
//          pixels before the chunk, offsets[b] the value at image b's first chunk, offsets[B] the total.
//   emit   the keep test again, then the write position by an order-preserving compaction: a ballot per slab, popcounts below the
//          lane, the waves' and slabs' sums through LDS; a kept lane computes its row and stores it at ws[chunk] + rank.  Kept
//          lanes of a wave hold consecutive positions, so the stores of a wave cover one contiguous span of each output.
// The keep test is recomputed in emit rather than carried as a flag byte through ws: emit loads the centre and its four neighbours
// for the normal anyway, the rest of the window comes out of the same cache lines, and the flag would add a byte written and a
// byte read per pixel and a second layout in ws; the resource report shows emit at 96 VGPRs, free of scratch.
// No atomics at all; positions depend on the input alone, not on the launch geometry.  Rows beyond offsets[B] are never written.
#include "hp_depth.h"

namespace {

constexpr int kScanMaxPoints = 1 << 22;    // = HP_SCAN_MAX_POINTS: the pixels of one image
constexpr int kMaxWindow = 4;              // = HP_DEPTH_MAX_WINDOW
constexpr int kThreads = 256;              // 4 waves per workgroup
constexpr int kWaves = kThreads / HP_WAVE;
constexpr int kPixelsPerLane = 4;          // slabs of kThreads consecutive pixels: lane t has pixels t, t + 256, ... of the chunk
constexpr int kChunk = kThreads * kPixelsPerLane;
constexpr int kGrid = 2048;                // workgroups at most: 8 per compute unit, each strides over the chunks
constexpr int kScanThreads = 1024;         // the scan pass: chunks per round
constexpr int kScanWaves = kScanThreads / HP_WAVE;

// A chunk's place: its image, the image's first pixel and the chunk's first pixel within the image.
struct Chunk {
    int b;
    size_t first;
    int pixel0;
};

__device__ __forceinline__ Chunk chunk_of(const Images& im, long long c) {
    const int b = (int)(c / im.chunks);
    return {b, (size_t)b * im.H * im.W, (int)(c - (long long)b * im.chunks) * kChunk};
}

__global__ __launch_bounds__(kThreads) void depth_count_kernel(Images im, long long chunks, unsigned* __restrict__ count) {
    __shared__ int sWave[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int HW = im.H * im.W;
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const Chunk ch = chunk_of(im, c);
        int n = 0;
#pragma unroll
        for (int k = 0; k < kPixelsPerLane; ++k) {
            const int i = ch.pixel0 + k * kThreads + tid;
            bool keep = false;
            if (i < HW) keep = kept(im, ch.first, i / im.W, i % im.W, depth_at(im, ch.first + i));
            n += __popcll(__ballot(keep));
        }
        if (lane == 0) sWave[wave] = n;
        __syncthreads();
        if (tid == 0) {
            int total = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) total += sWave[w];
            count[c] = (unsigned)total;
        }
        __syncthreads();
    }
}

// ws[c] -> the kept pixels before chunk c; offsets[b] = the value at chunk b * chunks_per_image, offsets[B] = the total.
__global__ __launch_bounds__(kScanThreads) void depth_scan_kernel(long long chunks, int chunks_per_image, int B,
                                                                  unsigned* __restrict__ count, long long* __restrict__ offsets) {
    __shared__ unsigned sWave[kScanWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned carry = 0;                                                        // uniform: the kept pixels of the rounds so far
    for (long long c0 = 0; c0 < chunks; c0 += kScanThreads) {
        const long long c = c0 + tid;
        const unsigned mine = c < chunks ? count[c] : 0u;
        unsigned incl = mine;
#pragma unroll
        for (int o = 1; o < HP_WAVE; o <<= 1) {
            const unsigned up = __shfl_up(incl, o, HP_WAVE);
            if (lane >= o) incl += up;
        }
        if (lane == HP_WAVE - 1) sWave[wave] = incl;
        __syncthreads();
        unsigned before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kScanWaves; ++w) {
            before += w < wave ? sWave[w] : 0u;
            total += sWave[w];
        }
        if (c < chunks) {
            const unsigned base = carry + before + (incl - mine);
            count[c] = base;
            if (c % chunks_per_image == 0) offsets[c / chunks_per_image] = (long long)base;
        }
        carry += total;
        __syncthreads();
    }
    if (tid == 0) offsets[B] = (long long)carry;
}

__device__ __forceinline__ void camera_point(const double (&K)[4], int v, int u, double z, double (&q)[3]) {
#pragma clang fp contract(off)
    q[0] = __ddiv_rn(__dmul_rn(__dsub_rn((double)u, K[2]), z), K[0]);
    q[1] = __ddiv_rn(__dmul_rn(__dsub_rn((double)v, K[3]), z), K[1]);
    q[2] = z;
}

// The camera point of the neighbour (y, x) where it is usable — inside the image, measured, no jump against the centre's z —
// and the centre's q otherwise.
__device__ __forceinline__ void side_point(const Images& im, size_t first, const double (&K)[4], int y, int x, double z,
                                           const double (&q)[3], double (&out)[3]) {
    out[0] = q[0], out[1] = q[1], out[2] = q[2];
    if (y < 0 || y >= im.H || x < 0 || x >= im.W) return;
    const double zz = depth_at(im, first + (size_t)y * im.W + x);
    if (measured(zz) && !jumps(im, z, zz)) camera_point(K, y, x, zz, out);
}

__device__ __forceinline__ double rotate(const double (&M)[12], int k, const double (&x)[3]) {
#pragma clang fp contract(off)
    return __dadd_rn(__dadd_rn(__dmul_rn(M[k * 4], x[0]), __dmul_rn(M[k * 4 + 1], x[1])), __dmul_rn(M[k * 4 + 2], x[2]));
}

// The output row of kept pixel (v, u) with depth z: world point and normal.
__device__ __forceinline__ void emit_row(const Images& im, size_t first, const double (&K)[4], const double (&M)[12], int v, int u,
                                         double z, float* __restrict__ point, float* __restrict__ normal) {
#pragma clang fp contract(off)
    double q[3], right[3], left[3], down[3], up[3];
    camera_point(K, v, u, z, q);
    side_point(im, first, K, v, u + 1, z, q, right);
    side_point(im, first, K, v, u - 1, z, q, left);
    side_point(im, first, K, v + 1, u, z, q, down);
    side_point(im, first, K, v - 1, u, z, q, up);
    double a[3], b[3], n[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] = __dsub_rn(right[c], left[c]), b[c] = __dsub_rn(down[c], up[c]);
    n[0] = __dsub_rn(__dmul_rn(a[1], b[2]), __dmul_rn(a[2], b[1]));
    n[1] = __dsub_rn(__dmul_rn(a[2], b[0]), __dmul_rn(a[0], b[2]));
    n[2] = __dsub_rn(__dmul_rn(a[0], b[1]), __dmul_rn(a[1], b[0]));
    if (__dadd_rn(__dadd_rn(__dmul_rn(n[0], q[0]), __dmul_rn(n[1], q[1])), __dmul_rn(n[2], q[2])) > 0.0)
        n[0] = -n[0], n[1] = -n[1], n[2] = -n[2];
    const double l = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(n[0], n[0]), __dmul_rn(n[1], n[1])), __dmul_rn(n[2], n[2])));
    const bool unit = l > 0.0 && l <= kDoubleMax;
#pragma unroll
    for (int c = 0; c < 3; ++c) n[c] = unit ? __ddiv_rn(n[c], l) : 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        point[k] = __double2float_rn(__dadd_rn(rotate(M, k, q), M[k * 4 + 3]));
        normal[k] = __double2float_rn(rotate(M, k, n));
    }
}

__global__ __launch_bounds__(kThreads) void depth_emit_kernel(Images im, long long chunks, const float* __restrict__ poses,
                                                              const unsigned* __restrict__ base, float* __restrict__ points,
                                                              float* __restrict__ normals, long long* __restrict__ pixel) {
    __shared__ int sWave[kPixelsPerLane][kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int HW = im.H * im.W;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const Chunk ch = chunk_of(im, c);
        double z[kPixelsPerLane];
        int rank[kPixelsPerLane];                                              // among the wave's kept lanes of the slab, -1: not kept
#pragma unroll
        for (int k = 0; k < kPixelsPerLane; ++k) {
            const int i = ch.pixel0 + k * kThreads + tid;
            bool keep = false;
            z[k] = 0.0;
            if (i < HW) {
                z[k] = depth_at(im, ch.first + i);
                keep = kept(im, ch.first, i / im.W, i % im.W, z[k]);
            }
            const unsigned long long vote = __ballot(keep);
            rank[k] = keep ? __popcll(vote & below) : -1;
            if (lane == 0) sWave[k][wave] = __popcll(vote);
        }
        __syncthreads();
        double K[4], M[12];
#pragma unroll
        for (int j = 0; j < 4; ++j) K[j] = im.K[(size_t)ch.b * 4 + j];
#pragma unroll
        for (int j = 0; j < 12; ++j) M[j] = (double)poses[(size_t)ch.b * 12 + j];
        size_t at = base[c];                                                   // uniform: where the slab's first kept pixel goes
#pragma unroll
        for (int k = 0; k < kPixelsPerLane; ++k) {
            int before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                before += w < wave ? sWave[k][w] : 0;
                total += sWave[k][w];
            }
            if (rank[k] >= 0) {
                const int i = ch.pixel0 + k * kThreads + tid;
                const size_t pos = at + before + rank[k];
                emit_row(im, ch.first, K, M, i / im.W, i % im.W, z[k], points + pos * 3, normals + pos * 3);
                pixel[pos] = (long long)(ch.first + i);
            }
            at += total;
        }
        __syncthreads();
    }
}

inline long long chunks_per_image(long long HW) { return (HW + kChunk - 1) / kChunk; }

inline bool shape_ok(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return false;
    const long long HW = (long long)H * W;
    return HW <= kScanMaxPoints && (long long)B * HW <= 0x7FFFFFFFll;
}

}  // namespace

// Bytes of hp_depth_points' workspace: one uint32 per chunk, B * ceil(H * W / 1024) of them, rounded up to a multiple of 16.
// Host only; -1 on bad arguments.
HP_API long long hp_depth_points_workspace_bytes(int B, int H, int W) {
    if (!shape_ok(B, H, W)) return -1;
    return ((long long)B * chunks_per_image((long long)H * W) * (long long)sizeof(unsigned) + 15) / 16 * 16;
}

// The geometry of hp_depth_points over B images of H x W: threads per workgroup, pixels per lane (a chunk is their product),
// chunks per image, the chunks the scan pass takes per round and its rounds.  Host only.
HP_API int hp_depth_points_plan(int B, int H, int W, int* threads, int* pixels_per_lane, int* chunks, int* scan_threads,
                                int* scan_rounds) {
    HP_CHECK_ARG(shape_ok(B, H, W) && threads && pixels_per_lane && chunks && scan_threads && scan_rounds);
    const long long per = chunks_per_image((long long)H * W);
    *threads = kThreads;
    *pixels_per_lane = kPixelsPerLane;
    *chunks = (int)per;
    *scan_threads = kScanThreads;
    *scan_rounds = (int)((B * per + kScanThreads - 1) / kScanThreads);
    return 0;
}

// B depth images -> the ragged set of their kept pixels; the law is in include/hyperpocket_hip.h.
HP_API int hp_depth_points(int B, int H, int W, const void* depth, int depth_is_u16, double scale, const double* K,
                           const float* poses, const unsigned char* mask, double near, double far, double jump_abs,
                           double jump_rel, int w, float* points, float* normals, long long* pixel, long long* offsets, void* ws,
                           long long ws_bytes, hipStream_t stream) {
    HP_CHECK_ARG(shape_ok(B, H, W) && depth && (depth_is_u16 == 0 || depth_is_u16 == 1) && K && poses);
    HP_CHECK_ARG(scale > 0.0 && scale <= kDoubleMax && near >= 0.0 && near <= far);            // far may be +inf; a NaN fails
    HP_CHECK_ARG(jump_abs >= 0.0 && jump_abs <= kDoubleMax && jump_rel >= 0.0 && jump_rel <= kDoubleMax);
    HP_CHECK_ARG(w >= 0 && w <= kMaxWindow && points && normals && pixel && offsets && ws);
    HP_CHECK_ARG(ws_bytes >= hp_depth_points_workspace_bytes(B, H, W) && reinterpret_cast<uintptr_t>(ws) % 16 == 0);
    const long long per = chunks_per_image((long long)H * W), chunks = B * per;
    const Images im = {depth, mask, K, B, H, W, (int)per, depth_is_u16 != 0, scale, near, far, jump_abs, jump_rel, w};
    const int groups = (int)std::min<long long>(chunks, kGrid);
    unsigned* count = static_cast<unsigned*>(ws);
    hipLaunchKernelGGL(depth_count_kernel, dim3(groups), dim3(kThreads), 0, stream, im, chunks, count);
    hipLaunchKernelGGL(depth_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, chunks, (int)per, B, count, offsets);
    hipLaunchKernelGGL(depth_emit_kernel, dim3(groups), dim3(kThreads), 0, stream, im, chunks, poses, count, points, normals,
                       pixel);
    HP_RETURN_LAST_ERROR();
}
