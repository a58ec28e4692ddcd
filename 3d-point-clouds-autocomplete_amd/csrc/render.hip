// Point-cloud previews: B clouds under V views as depth-buffered splats, one launch (the executable law is
// tests/render_law.py and the kernel follows it bit for bit).
//
//   One workgroup per (cloud, view, tile).  The tile's 64-bit depth keys (zq << 32 | point index) live in LDS, start as all
//   ones, and take every splat pixel that falls inside the tile with an LDS atomicMin on unsigned long long (ds_min_u64: no
//   compare-and-swap loop).  The workgroup streams all n points of its cloud, one point per thread and pass (coalesced 12-byte
//   rows), projects each in fp32 without contraction, and tests the splat's box against the tile before touching LDS; a splat
//   that straddles 2 or 4 tiles is drawn by each of their workgroups.  After a barrier the tile is resolved: a wave per pixel
//   row, a lane per output byte, so the RGB bytes of a row leave as consecutive byte stores, then its ids.
//   Integer keys make the minimum independent of arrival order: no global atomics, no float atomics, no clear or resolve
//   launch, and every output byte is written exactly once.
#include "hp_common.h"

namespace {

constexpr int kMaxLayers = 8;
constexpr int kMaxRadius2 = 64;
constexpr int kMaxSide = 4096;
constexpr int kDefaultTile = 128;         // measured against 32 and 64: a workgroup streams the whole cloud, so fewer tiles win
constexpr unsigned long long kEmpty = ~0ull;

std::atomic<int> g_tile{0};     // 0: the launcher's choice

struct RenderLayers {           // by value in the kernel's arguments
    int count;
    int ends[kMaxLayers];
    int radius2[kMaxLayers];
    int radius[kMaxLayers];     // floor(sqrt(radius2))
    unsigned char rgb[kMaxLayers][4];
    unsigned char background[4];
    int fog;
};

struct RenderPlan {
    int tile_w, tile_h, tiles_x, tiles_y, threads, lds_bytes;
};

RenderPlan plan_for(int W, int H) {
    const int hook = g_tile.load(std::memory_order_relaxed);
    const int T = hook ? hook : kDefaultTile;
    RenderPlan p;
    p.tile_w = std::min(T, W);
    p.tile_h = std::min(T, H);
    p.tiles_x = (W + p.tile_w - 1) / p.tile_w;
    p.tiles_y = (H + p.tile_h - 1) / p.tile_h;
    p.threads = (long)p.tile_w * p.tile_h > 64 * 64 ? 1024 : 256;
    p.lds_bytes = p.tile_w * p.tile_h * (int)sizeof(unsigned long long);
    return p;
}

__device__ __forceinline__ int layer_of(const RenderLayers& lay, unsigned i) {
    int l = 0;
    while (l < lay.count - 1 && (unsigned)lay.ends[l] <= i) ++l;
    return l;
}

__global__ __launch_bounds__(1024) void render_points_kernel(int n, const float* __restrict__ points, int V,
                                                              const float* __restrict__ views, RenderLayers lay, int W, int H,
                                                              int tile_w, int tile_h, int tiles_x, int tiles_y,
                                                              unsigned char* __restrict__ image, int* __restrict__ ids) {
    extern __shared__ unsigned long long zbuf[];            // tile_w x tile_h keys, row stride tile_w
    const unsigned tiles = (unsigned)tiles_x * tiles_y;
    const unsigned tile = blockIdx.x % tiles, bv = blockIdx.x / tiles;      // bv = b * V + v
    const unsigned v = bv % (unsigned)V, b = bv / (unsigned)V;
    const int x0 = (int)(tile % (unsigned)tiles_x) * tile_w, y0 = (int)(tile / (unsigned)tiles_x) * tile_h;
    const int tw = min(tile_w, W - x0), th = min(tile_h, H - y0);          // the part of the tile inside the image

    for (int k = threadIdx.x; k < tile_w * tile_h; k += blockDim.x) zbuf[k] = kEmpty;

    const float* M = views + (size_t)v * 12;
    const float m00 = M[0], m01 = M[1], m02 = M[2], m03 = M[3];
    const float m10 = M[4], m11 = M[5], m12 = M[6], m13 = M[7];
    const float m20 = M[8], m21 = M[9], m22 = M[10], m23 = M[11];
    const float u_hi = __fadd_rn((float)W, 9.0f), v_hi = __fadd_rn((float)H, 9.0f);
    const float* cloud = points + (size_t)b * n * 3;
    __syncthreads();

    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float x = cloud[(size_t)i * 3], y = cloud[(size_t)i * 3 + 1], z = cloud[(size_t)i * 3 + 2];
        // one rounding per operation, left to right (the build passes -ffp-contract=off; the _rn forms say it again)
        const float u = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m00, x), __fmul_rn(m01, y)), __fmul_rn(m02, z)), m03);
        const float vv = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m10, x), __fmul_rn(m11, y)), __fmul_rn(m12, z)), m13);
        const float w = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(m20, x), __fmul_rn(m21, y)), __fmul_rn(m22, z)), m23);
        if (!(__builtin_isfinite(u) && __builtin_isfinite(vv) && __builtin_isfinite(w))) continue;
        if (!(u >= -9.0f && u < u_hi && vv >= -9.0f && vv < v_hi)) continue;
        const int px = (int)floorf(u), py = (int)floorf(vv);               // within [-9, 4105]
        const int l = layer_of(lay, (unsigned)i);
        const int r = lay.radius[l], r2 = lay.radius2[l];
        // the splat's box against the tile, in tile coordinates
        const int cx = px - x0, cy = py - y0;
        const int dx_lo = max(-r, -cx), dx_hi = min(r, tw - 1 - cx);
        const int dy_lo = max(-r, -cy), dy_hi = min(r, th - 1 - cy);
        if (dx_lo > dx_hi || dy_lo > dy_hi) continue;
        const float zf = fminf(fmaxf(floorf(__fmul_rn(w, 16777216.0f)), 0.0f), 16777215.0f);
        const unsigned long long key = ((unsigned long long)(unsigned)(int)zf << 32) | (unsigned)i;
        for (int dy = dy_lo; dy <= dy_hi; ++dy)
            for (int dx = dx_lo; dx <= dx_hi; ++dx)
                if (dx * dx + dy * dy <= r2) atomicMin(&zbuf[(cy + dy) * tile_w + (cx + dx)], key);
    }
    __syncthreads();

    const int lane = threadIdx.x & (HP_WAVE - 1), wave = threadIdx.x / HP_WAVE, waves = blockDim.x / HP_WAVE;
    const size_t image_px = (size_t)bv * H * W;             // first pixel of this (cloud, view) image
    for (int row = wave; row < th; row += waves) {
        const size_t px0 = image_px + (size_t)(y0 + row) * W + x0;
        const unsigned long long* keys = zbuf + row * tile_w;
        for (int k = lane; k < tw * 3; k += HP_WAVE) {
            const int col = k / 3, c = k - col * 3;
            const unsigned long long key = keys[col];
            unsigned out = lay.background[c];
            if (key != kEmpty) {
                const unsigned zq = (unsigned)(key >> 32);
                const unsigned shade = 255u - (((zq >> 16) * (unsigned)lay.fog) >> 8);
                out = ((unsigned)lay.rgb[layer_of(lay, (unsigned)key)][c] * shade + 127u) / 255u;
            }
            image[px0 * 3 + k] = (unsigned char)out;
        }
        if (ids)
            for (int col = lane; col < tw; col += HP_WAVE) {
                const unsigned long long key = keys[col];
                ids[px0 + col] = key == kEmpty ? -1 : (int)(unsigned)key;
            }
    }
}

bool size_ok(int W, int H) { return W >= 1 && H >= 1 && W <= kMaxSide && H <= kMaxSide; }

}  // namespace

// [test hook: process-wide, not read from the environment] the tile side: 8, 16, 32, 64 or 128 pixels, 0 = the launcher's
// choice (default).  Returns the previous setting, -1 (and no change) for any other value.  The image is the same bits under
// every setting.
HP_API int hp_render_points_set_tile(int side) {
    if (side != 0 && side != 8 && side != 16 && side != 32 && side != 64 && side != 128) return -1;
    return g_tile.exchange(side);
}

struct HpRenderPlan {           // = HpRenderPlan (include/hyperpocket_hip.h)
    int tile_w, tile_h, tiles_x, tiles_y, tiles, threads, lds_bytes;
    long long workgroups;
};

// The launch hp_render_points makes for B clouds, V views and a W x H image, under the current hook.  Host only.
HP_API int hp_render_points_plan(int B, int V, int W, int H, HpRenderPlan* plan) {
    HP_CHECK_ARG(B >= 1 && V >= 1 && size_ok(W, H) && plan);
    const RenderPlan p = plan_for(W, H);
    plan->tile_w = p.tile_w;
    plan->tile_h = p.tile_h;
    plan->tiles_x = p.tiles_x;
    plan->tiles_y = p.tiles_y;
    plan->tiles = p.tiles_x * p.tiles_y;
    plan->threads = p.threads;
    plan->lds_bytes = p.lds_bytes;
    plan->workgroups = (long long)B * V * plan->tiles;
    return 0;
}

HP_API int hp_render_points(int B, int n, const float* points, int V, const float* views, int L, const int* layer_ends,
                            const unsigned char* palette, const int* radius2, int fog, const unsigned char* background,
                            int W, int H, unsigned char* image, int* ids, hipStream_t stream) {
    HP_CHECK_ARG(B >= 1 && n >= 1 && V >= 1 && size_ok(W, H));
    HP_CHECK_ARG(L >= 1 && L <= kMaxLayers && fog >= 0 && fog <= 255);
    HP_CHECK_ARG(points && views && layer_ends && palette && radius2 && background && image);
    RenderLayers lay = {};
    lay.count = L;
    lay.fog = fog;
    for (int l = 0, before = 0; l < L; ++l) {
        HP_CHECK_ARG(layer_ends[l] >= before && layer_ends[l] <= n);
        HP_CHECK_ARG(radius2[l] >= 0 && radius2[l] <= kMaxRadius2);
        before = lay.ends[l] = layer_ends[l];
        lay.radius2[l] = radius2[l];
        int r = 0;
        while ((r + 1) * (r + 1) <= radius2[l]) ++r;
        lay.radius[l] = r;
        for (int c = 0; c < 3; ++c) lay.rgb[l][c] = palette[l * 3 + c];
    }
    HP_CHECK_ARG(layer_ends[L - 1] == n);
    for (int c = 0; c < 3; ++c) lay.background[c] = background[c];
    const RenderPlan p = plan_for(W, H);
    const long long groups = (long long)B * V * p.tiles_x * p.tiles_y;
    HP_CHECK_ARG(groups <= 0x7fffffffLL);                   // one grid dimension
    if (p.lds_bytes > 64 * 1024)                            // a 128 x 128 tile: 128 KiB of the CU's 160
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(render_points_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  p.lds_bytes);
    hipLaunchKernelGGL(render_points_kernel, dim3((unsigned)groups), dim3(p.threads), p.lds_bytes, stream, n, points, V, views, lay,
                       W, H, p.tile_w, p.tile_h, p.tiles_x, p.tiles_y, image, ids);
    HP_RETURN_LAST_ERROR();
}
