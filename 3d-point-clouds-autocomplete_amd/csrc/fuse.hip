// Posed depth images fused into one surface per volume: volumetric fusion with a truncated signed distance
// function, the sibling of depth.hip — the same images, the same keep test (hp_depth.h), the same ordered compaction.  G volumes
// (groups) of nx x ny x nz voxels, each with its origin and its list of images; every voxel averages, over the images of its group
// that observe it, the signed distance to the surface along the camera's axis cut off at `truncation`; the surface is where that
// average changes sign between two neighbouring voxels.
//
// The law (include/hyperpocket_hip.h and tests/fuse_law.py have it in full; every operation is one fp64 rounding, no contraction):
//   voxel (i, j, k) of group g: c = o + (double(i) + 0.5) * voxel per axis; for each image b of the group in list order:
//     d = c - t; q_a = (R_0a d0 + R_1a d1) + R_2a d2; skip unless q2 > 0; x = ((q0 fx) / q2) + cx, y likewise;
//     u = floor(x + 0.5), v = floor(y + 0.5); skip unless inside the image (compared in fp64) and pixel (v, u) is kept;
//     s = z(v, u) - q2; skip when s < -truncation; f = min(s / truncation, 1); F += f, n += 1.
//     weight = n, tsdf = float(F / double(n)), 1.0f when n = 0.
//   surface: voxel a and its neighbour b = a + e along axis e, both with weight >= min_weight and (fa < 0) != (fb < 0):
//     t = fa / (fa - fb); the point is a's centre with t * voxel added to component e; the normal is the central difference of
//     the field (a missing side takes the centre's value) interpolated between a and b, normalised or zero.
//
// hp_fuse_volume, two launches:
//   keep    the keep test of every pixel once, as ballot words in ws: one bit per pixel, an image padded to a multiple of 64 —
//           a wave per word.  The voxel loop then reads a bit and a depth per image rather than a (2w+1)^2 window.
//   volume  a lane per voxel, x fastest, so both volumes are stored coalesced; a workgroup lies within one group, so the group's
//           image list, intrinsics and poses are uniform and come through scalar loads.  A gather: no atomics.
// hp_fuse_surface, three launches as depth.hip's.  A chunk is kChunk consecutive voxels of one group; chunks never cross groups.
//   count   rows per chunk into ws (uint64: 3 rows a voxel can pass 2^32).
//   scan    one workgroup: ws[chunk] becomes the rows before the chunk, offsets[g] the value at group g's first chunk.
//   emit    the crossings again, then the write position: three ballots a slab, one per axis, the popcounts below the lane, the
//           waves' and slabs' sums through LDS.  Row order: group, k, j, i, then axis x, y, z.  Rows at positions >= capacity are
//           not written; capacity 0 skips the launch.
// No atomics of any kind; positions depend on the input alone, not on the launch geometry.
#include "hp_depth.h"

namespace {

constexpr int kScanMaxPoints = 1 << 22;    // = HP_SCAN_MAX_POINTS: the pixels of one image
constexpr int kMaxWindow = 4;              // = HP_DEPTH_MAX_WINDOW
constexpr int kMaxDim = 1024;              // = HP_FUSE_MAX_DIM
constexpr int kThreads = 256;              // 4 waves per workgroup
constexpr int kWaves = kThreads / HP_WAVE;
constexpr int kVoxelsPerLane = 4;          // slabs of kThreads consecutive voxels: lane t has voxels t, t + 256, ... of the chunk
constexpr int kChunk = kThreads * kVoxelsPerLane;
constexpr int kGrid = 2048;                // workgroups at most of the grid-stride passes
constexpr int kScanThreads = 1024;         // the scan pass: chunks per round
constexpr int kScanWaves = kScanThreads / HP_WAVE;
typedef unsigned long long u64;

// ---- the volume ------------------------------------------------------------------------------------------------------------------
struct Groups {
    const int* images;                     // (L): the images of the groups, group after group
    const int* offsets;                    // (G+1)
    const double* origin;                  // (G,3)
    int G, nx, ny, nz;
    double voxel, truncation;
};

// In Images, `chunks` counts the ballot words of an image here: ceil(H * W / 64).
__global__ __launch_bounds__(kThreads) void fuse_keep_kernel(Images im, long long words, u64* __restrict__ bits) {
    const int lane = threadIdx.x & 63;
    const int HW = im.H * im.W;
    const long long stride = (long long)gridDim.x * kWaves;
    for (long long wd = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); wd < words; wd += stride) {
        const int b = (int)(wd / im.chunks);
        const int i = (int)(wd - (long long)b * im.chunks) * 64 + lane;
        const size_t first = (size_t)b * HW;
        bool keep = false;
        if (i < HW) keep = kept(im, first, i / im.W, i % im.W, depth_at(im, first + i));
        const u64 vote = __ballot(keep);
        if (lane == 0) bits[wd] = vote;
    }
}

__device__ __forceinline__ double centre(double o, int i, double voxel) {
#pragma clang fp contract(off)
    return __dadd_rn(o, __dmul_rn(__dadd_rn((double)i, 0.5), voxel));
}

__global__ __launch_bounds__(kThreads) void fuse_volume_kernel(Images im, Groups gr, int blocks_per_group,
                                                               const float* __restrict__ poses, const u64* __restrict__ bits,
                                                               float* __restrict__ tsdf, int* __restrict__ weight) {
#pragma clang fp contract(off)
    const int g = blockIdx.x / blocks_per_group;                               // uniform: the group's tables come through scalar loads
    const int V = gr.nx * gr.ny * gr.nz;
    const int r = (blockIdx.x - g * blocks_per_group) * kThreads + threadIdx.x;
    if (r >= V) return;
    const int i = r % gr.nx, j = r / gr.nx % gr.ny, k = r / (gr.nx * gr.ny);
    const double c0 = centre(gr.origin[g * 3], i, gr.voxel), c1 = centre(gr.origin[g * 3 + 1], j, gr.voxel),
                 c2 = centre(gr.origin[g * 3 + 2], k, gr.voxel);
    const int HW = im.H * im.W;
    const double umax = (double)(im.W - 1), vmax = (double)(im.H - 1), below = -gr.truncation;
    double F = 0.0;
    int n = 0;
    const int l1 = gr.offsets[g + 1];
    for (int l = gr.offsets[g]; l < l1; ++l) {
        const int b = gr.images[l];
        const float* M = poses + (size_t)b * 12;
        const double* K = im.K + (size_t)b * 4;
        const double d0 = __dsub_rn(c0, (double)M[3]), d1 = __dsub_rn(c1, (double)M[7]), d2 = __dsub_rn(c2, (double)M[11]);
        const double q2 = __dadd_rn(__dadd_rn(__dmul_rn((double)M[2], d0), __dmul_rn((double)M[6], d1)), __dmul_rn((double)M[10], d2));
        if (!(q2 > 0.0)) continue;
        const double q0 = __dadd_rn(__dadd_rn(__dmul_rn((double)M[0], d0), __dmul_rn((double)M[4], d1)), __dmul_rn((double)M[8], d2));
        const double q1 = __dadd_rn(__dadd_rn(__dmul_rn((double)M[1], d0), __dmul_rn((double)M[5], d1)), __dmul_rn((double)M[9], d2));
        const double x = __dadd_rn(__ddiv_rn(__dmul_rn(q0, K[0]), q2), K[2]);
        const double y = __dadd_rn(__ddiv_rn(__dmul_rn(q1, K[1]), q2), K[3]);
        const double uf = floor(__dadd_rn(x, 0.5)), vf = floor(__dadd_rn(y, 0.5));
        if (!(uf >= 0.0 && uf <= umax && vf >= 0.0 && vf <= vmax)) continue;   // in fp64, before any conversion: a NaN is outside
        const int p = (int)vf * im.W + (int)uf;
        if (!((bits[(size_t)b * im.chunks + (p >> 6)] >> (p & 63)) & 1ull)) continue;
        const double s = __dsub_rn(depth_at(im, (size_t)b * HW + p), q2);
        if (s < below) continue;
        const double f = __ddiv_rn(s, gr.truncation);
        F = __dadd_rn(F, f > 1.0 ? 1.0 : f);
        ++n;
    }
    const size_t at = (size_t)g * V + r;
    weight[at] = n;
    tsdf[at] = n > 0 ? __double2float_rn(__ddiv_rn(F, (double)n)) : 1.0f;
}

// ---- the surface -----------------------------------------------------------------------------------------------------------------
struct Volume {
    const float* tsdf;                     // (G, nz, ny, nx)
    const int* weight;
    const double* origin;                  // (G,3)
    int G, nx, ny, nz, chunks;             // chunks per group
    double voxel;
    int min_weight;
};

// The field at voxel (i, j, k) of the group whose first voxel is `first`, where the voxel is usable — inside the grid and observed
// min_weight times; false otherwise, and f is left alone.
__device__ __forceinline__ bool usable(const Volume& vol, size_t first, int i, int j, int k, double& f) {
    if (i < 0 || i >= vol.nx || j < 0 || j >= vol.ny || k < 0 || k >= vol.nz) return false;
    const size_t at = first + ((size_t)k * vol.ny + j) * vol.nx + i;
    if (vol.weight[at] < vol.min_weight) return false;
    f = (double)vol.tsdf[at];
    return true;
}

// Bit e: usable voxel (i, j, k) with field fa has a row along axis e.
__device__ __forceinline__ int crossings(const Volume& vol, size_t first, int i, int j, int k, double fa) {
    int rows = 0;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        double fb = 0.0;
        if (usable(vol, first, i + (e == 0), j + (e == 1), k + (e == 2), fb) && (fa < 0.0) != (fb < 0.0)) rows |= 1 << e;
    }
    return rows;
}

// g_d at voxel (i, j, k) with field fc: a side that is not usable takes the centre's value.
__device__ __forceinline__ double slope(const Volume& vol, size_t first, int i, int j, int k, int d, double fc) {
    double hi = fc, lo = fc;
    usable(vol, first, i + (d == 0), j + (d == 1), k + (d == 2), hi);
    usable(vol, first, i - (d == 0), j - (d == 1), k - (d == 2), lo);
    return __dsub_rn(hi, lo);
}

// A chunk's place: its group, the group's first voxel and the chunk's first voxel within the group.
struct Chunk {
    int g;
    size_t first;
    int voxel0;
};

__device__ __forceinline__ Chunk chunk_of(const Volume& vol, int V, long long c) {
    const int g = (int)(c / vol.chunks);
    return {g, (size_t)g * V, (int)(c - (long long)g * vol.chunks) * kChunk};
}

// The crossings of voxel r of the chunk's group (0 beyond the group or where the voxel is not usable) and its field.
__device__ __forceinline__ int voxel_rows(const Volume& vol, const Chunk& ch, int V, int r, double& fa) {
    fa = 0.0;
    if (r >= V) return 0;
    const int i = r % vol.nx, j = r / vol.nx % vol.ny, k = r / (vol.nx * vol.ny);
    if (!usable(vol, ch.first, i, j, k, fa)) return 0;
    return crossings(vol, ch.first, i, j, k, fa);
}

__global__ __launch_bounds__(kThreads) void fuse_count_kernel(Volume vol, long long chunks, u64* __restrict__ count) {
    __shared__ int sWave[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = vol.nx * vol.ny * vol.nz;
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const Chunk ch = chunk_of(vol, V, c);
        int n = 0;
#pragma unroll
        for (int s = 0; s < kVoxelsPerLane; ++s) {
            double fa;
            const int rows = voxel_rows(vol, ch, V, ch.voxel0 + s * kThreads + tid, fa);
            n += __popcll(__ballot(rows & 1)) + __popcll(__ballot(rows & 2)) + __popcll(__ballot(rows & 4));
        }
        if (lane == 0) sWave[wave] = n;
        __syncthreads();
        if (tid == 0) {
            int total = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) total += sWave[w];
            count[c] = (u64)total;
        }
        __syncthreads();
    }
}

// ws[c] -> the rows before chunk c; offsets[g] = the value at chunk g * chunks_per_group, offsets[G] = the total.
__global__ __launch_bounds__(kScanThreads) void fuse_scan_kernel(long long chunks, int chunks_per_group, int G,
                                                                 u64* __restrict__ count, long long* __restrict__ offsets) {
    __shared__ u64 sWave[kScanWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u64 carry = 0;                                                             // uniform: the rows of the rounds so far
    for (long long c0 = 0; c0 < chunks; c0 += kScanThreads) {
        const long long c = c0 + tid;
        const u64 mine = c < chunks ? count[c] : 0ull;
        u64 incl = mine;
#pragma unroll
        for (int o = 1; o < HP_WAVE; o <<= 1) {
            const u64 up = __shfl_up(incl, o, HP_WAVE);
            if (lane >= o) incl += up;
        }
        if (lane == HP_WAVE - 1) sWave[wave] = incl;
        __syncthreads();
        u64 before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kScanWaves; ++w) {
            before += w < wave ? sWave[w] : 0ull;
            total += sWave[w];
        }
        if (c < chunks) {
            const u64 base = carry + before + (incl - mine);
            count[c] = base;
            if (c % chunks_per_group == 0) offsets[c / chunks_per_group] = (long long)base;
        }
        carry += total;
        __syncthreads();
    }
    if (tid == 0) offsets[G] = (long long)carry;
}

// The row of the crossing between voxel a = (i, j, k), field fa, and its neighbour along axis e.
__device__ __forceinline__ void emit_row(const Volume& vol, const Chunk& ch, int i, int j, int k, int e, double fa,
                                         float* __restrict__ point, float* __restrict__ normal) {
#pragma clang fp contract(off)
    const int bi = i + (e == 0), bj = j + (e == 1), bk = k + (e == 2);
    double fb = fa;
    usable(vol, ch.first, bi, bj, bk, fb);
    const double t = __ddiv_rn(fa, __dsub_rn(fa, fb));
    double p[3] = {centre(vol.origin[ch.g * 3], i, vol.voxel), centre(vol.origin[ch.g * 3 + 1], j, vol.voxel),
                   centre(vol.origin[ch.g * 3 + 2], k, vol.voxel)};
    const double step = __dmul_rn(t, vol.voxel);
    double m[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        if (d == e) p[d] = __dadd_rn(p[d], step);
        const double ga = slope(vol, ch.first, i, j, k, d, fa), gb = slope(vol, ch.first, bi, bj, bk, d, fb);
        m[d] = __dadd_rn(ga, __dmul_rn(t, __dsub_rn(gb, ga)));
    }
    const double l = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(m[0], m[0]), __dmul_rn(m[1], m[1])), __dmul_rn(m[2], m[2])));
    const bool unit = l > 0.0 && l <= kDoubleMax;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        point[d] = __double2float_rn(p[d]);
        normal[d] = __double2float_rn(unit ? __ddiv_rn(m[d], l) : 0.0);
    }
}

__global__ __launch_bounds__(kThreads) void fuse_emit_kernel(Volume vol, long long chunks, const u64* __restrict__ base,
                                                             long long capacity, float* __restrict__ points,
                                                             float* __restrict__ normals, long long* __restrict__ cell) {
    __shared__ int sWave[kVoxelsPerLane][kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = vol.nx * vol.ny * vol.nz;
    const u64 below = (1ull << lane) - 1ull;
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const Chunk ch = chunk_of(vol, V, c);
        double fa[kVoxelsPerLane];
        int rows[kVoxelsPerLane], rank[kVoxelsPerLane];                        // rank: the rows of the wave's lower lanes in the slab
#pragma unroll
        for (int s = 0; s < kVoxelsPerLane; ++s) {
            rows[s] = voxel_rows(vol, ch, V, ch.voxel0 + s * kThreads + tid, fa[s]);
            const u64 vx = __ballot(rows[s] & 1), vy = __ballot(rows[s] & 2), vz = __ballot(rows[s] & 4);
            rank[s] = __popcll(vx & below) + __popcll(vy & below) + __popcll(vz & below);
            if (lane == 0) sWave[s][wave] = __popcll(vx) + __popcll(vy) + __popcll(vz);
        }
        __syncthreads();
        u64 at = base[c];                                                      // uniform: where the slab's first row goes
#pragma unroll
        for (int s = 0; s < kVoxelsPerLane; ++s) {
            int before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                before += w < wave ? sWave[s][w] : 0;
                total += sWave[s][w];
            }
            if (rows[s]) {
                const int r = ch.voxel0 + s * kThreads + tid;
                const int i = r % vol.nx, j = r / vol.nx % vol.ny, k = r / (vol.nx * vol.ny);
                u64 pos = at + before + rank[s];
#pragma unroll
                for (int e = 0; e < 3; ++e)
                    if ((rows[s] >> e) & 1) {
                        if (pos < (u64)capacity) {
                            emit_row(vol, ch, i, j, k, e, fa[s], points + pos * 3, normals + pos * 3);
                            cell[pos] = (long long)(ch.first + r) * 3 + e;
                        }
                        ++pos;
                    }
            }
            at += total;
        }
        __syncthreads();
    }
}

inline bool images_ok(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return false;
    const long long HW = (long long)H * W;
    return HW <= kScanMaxPoints && (long long)B * HW <= 0x7FFFFFFFll;
}

inline bool grid_ok(int G, int nx, int ny, int nz) {
    if (G < 1 || nx < 1 || ny < 1 || nz < 1 || nx > kMaxDim || ny > kMaxDim || nz > kMaxDim) return false;
    return (long long)G * nx * ny * nz <= 0x7FFFFFFFll;
}

inline long long words_per_image(long long HW) { return (HW + 63) / 64; }
inline long long chunks_per_group(long long V) { return (V + kChunk - 1) / kChunk; }
inline bool positive(double x) { return x > 0.0 && x <= kDoubleMax; }           // false for a NaN

}  // namespace

// Bytes of hp_fuse_volume's workspace: one 64-bit ballot word per 64 pixels, B * ceil(H * W / 64) of them (a multiple of 16 after
// rounding up).  Host only; -1 on bad arguments.
HP_API long long hp_fuse_volume_workspace_bytes(int B, int H, int W) {
    if (!images_ok(B, H, W)) return -1;
    return ((long long)B * words_per_image((long long)H * W) * (long long)sizeof(u64) + 15) / 16 * 16;
}

// The geometry of hp_fuse_volume: threads per workgroup of both launches, the ballot words of an image, the workgroups a group's
// voxels take and the workgroups of the volume launch.  Host only.
HP_API int hp_fuse_volume_plan(int B, int H, int W, int G, int nx, int ny, int nz, int* threads, int* words, int* blocks_per_group,
                               int* blocks) {
    HP_CHECK_ARG(images_ok(B, H, W) && grid_ok(G, nx, ny, nz) && threads && words && blocks_per_group && blocks);
    const long long per = ((long long)nx * ny * nz + kThreads - 1) / kThreads;
    *threads = kThreads;
    *words = (int)words_per_image((long long)H * W);
    *blocks_per_group = (int)per;
    *blocks = (int)(G * per);
    return 0;
}

// B posed depth images -> the TSDF and the weights of G volumes; the law is in include/hyperpocket_hip.h.  group_images and
// group_offsets are the device's tables, host_group_images and host_group_offsets the host's copies that the checks read.
HP_API int hp_fuse_volume(int B, int H, int W, const void* depth, int depth_is_u16, double scale, const double* K,
                          const float* poses, const unsigned char* mask, double near, double far, double jump_abs, double jump_rel,
                          int w, int G, int L, const int* group_images, const int* group_offsets, const int* host_group_images,
                          const int* host_group_offsets, const double* origin, int nx, int ny, int nz, double voxel,
                          double truncation, float* tsdf, int* weight, void* ws, long long ws_bytes, hipStream_t stream) {
    HP_CHECK_ARG(images_ok(B, H, W) && depth && (depth_is_u16 == 0 || depth_is_u16 == 1) && K && poses);
    HP_CHECK_ARG(scale > 0.0 && scale <= kDoubleMax && near >= 0.0 && near <= far);            // far may be +inf; a NaN fails
    HP_CHECK_ARG(jump_abs >= 0.0 && jump_abs <= kDoubleMax && jump_rel >= 0.0 && jump_rel <= kDoubleMax);
    HP_CHECK_ARG(w >= 0 && w <= kMaxWindow && grid_ok(G, nx, ny, nz) && L >= 1 && positive(voxel) && positive(truncation));
    HP_CHECK_ARG(group_images && group_offsets && host_group_images && host_group_offsets && origin && tsdf && weight && ws);
    HP_CHECK_ARG(host_group_offsets[0] == 0 && host_group_offsets[G] == L);
    for (int g = 0; g < G; ++g) HP_CHECK_ARG(host_group_offsets[g] < host_group_offsets[g + 1]);   // every group has an image
    for (int l = 0; l < L; ++l) HP_CHECK_ARG(host_group_images[l] >= 0 && host_group_images[l] < B);
    HP_CHECK_ARG(ws_bytes >= hp_fuse_volume_workspace_bytes(B, H, W) && reinterpret_cast<uintptr_t>(ws) % 16 == 0);
    const long long per = words_per_image((long long)H * W), words = B * per;
    const Images im = {depth, mask, K, B, H, W, (int)per, depth_is_u16 != 0, scale, near, far, jump_abs, jump_rel, w};
    const Groups gr = {group_images, group_offsets, origin, G, nx, ny, nz, voxel, truncation};
    u64* bits = static_cast<u64*>(ws);
    const long long keep_blocks = std::min<long long>((words + kWaves - 1) / kWaves, kGrid * 4);
    const long long blocks_per_group = ((long long)nx * ny * nz + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(fuse_keep_kernel, dim3((unsigned)keep_blocks), dim3(kThreads), 0, stream, im, words, bits);
    hipLaunchKernelGGL(fuse_volume_kernel, dim3((unsigned)(G * blocks_per_group)), dim3(kThreads), 0, stream, im, gr,
                       (int)blocks_per_group, poses, bits, tsdf, weight);
    HP_RETURN_LAST_ERROR();
}

// Bytes of hp_fuse_surface's workspace: one uint64 per chunk, G * ceil(nx * ny * nz / 1024) of them, rounded up to a multiple of
// 16.  Host only; -1 on bad arguments.
HP_API long long hp_fuse_surface_workspace_bytes(int G, int nx, int ny, int nz) {
    if (!grid_ok(G, nx, ny, nz)) return -1;
    return ((long long)G * chunks_per_group((long long)nx * ny * nz) * (long long)sizeof(u64) + 15) / 16 * 16;
}

// The geometry of hp_fuse_surface: threads per workgroup, voxels per lane (a chunk is their product), chunks per group, the chunks
// the scan pass takes per round and its rounds.  Host only.
HP_API int hp_fuse_surface_plan(int G, int nx, int ny, int nz, int* threads, int* voxels_per_lane, int* chunks, int* scan_threads,
                                int* scan_rounds) {
    HP_CHECK_ARG(grid_ok(G, nx, ny, nz) && threads && voxels_per_lane && chunks && scan_threads && scan_rounds);
    const long long per = chunks_per_group((long long)nx * ny * nz);
    *threads = kThreads;
    *voxels_per_lane = kVoxelsPerLane;
    *chunks = (int)per;
    *scan_threads = kScanThreads;
    *scan_rounds = (int)((G * per + kScanThreads - 1) / kScanThreads);
    return 0;
}

// G volumes -> the ragged set of their zero crossings; the law is in include/hyperpocket_hip.h.
HP_API int hp_fuse_surface(int G, int nx, int ny, int nz, const float* tsdf, const int* weight, const double* origin, double voxel,
                           int min_weight, long long capacity, float* points, float* normals, long long* cell, long long* offsets,
                           void* ws, long long ws_bytes, hipStream_t stream) {
    HP_CHECK_ARG(grid_ok(G, nx, ny, nz) && tsdf && weight && origin && positive(voxel) && min_weight >= 1 && capacity >= 0);
    HP_CHECK_ARG((capacity == 0 || (points && normals && cell)) && offsets && ws);
    HP_CHECK_ARG(ws_bytes >= hp_fuse_surface_workspace_bytes(G, nx, ny, nz) && reinterpret_cast<uintptr_t>(ws) % 16 == 0);
    const long long per = chunks_per_group((long long)nx * ny * nz), chunks = G * per;
    const Volume vol = {tsdf, weight, origin, G, nx, ny, nz, (int)per, voxel, min_weight};
    const int groups = (int)std::min<long long>(chunks, kGrid);
    u64* count = static_cast<u64*>(ws);
    hipLaunchKernelGGL(fuse_count_kernel, dim3(groups), dim3(kThreads), 0, stream, vol, chunks, count);
    hipLaunchKernelGGL(fuse_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, chunks, (int)per, G, count, offsets);
    if (capacity > 0)
        hipLaunchKernelGGL(fuse_emit_kernel, dim3(groups), dim3(kThreads), 0, stream, vol, chunks, count, capacity, points, normals,
                           cell);
    HP_RETURN_LAST_ERROR();
}
