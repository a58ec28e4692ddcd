// What a batch of depth images is to the kernels that read one, and the keep test of a pixel, stated once for
// depth.hip (back-projection) and fuse.hip (volumetric fusion).  The law, per pixel (v, u) of image b (include/hyperpocket_hip.h
// and tests/depth_law.py have it in full; every operation is one fp64 rounding, no contraction):
//   z = double(d) * scale, measured when finite and > 0; jump(a, b) = |a - b| > jump_abs + jump_rel * min(a, b);
//   kept: measured, near <= z <= far, mask != 0, and no measured pixel within w jumps against it.
// Device inlines of a translation unit each: the unnamed namespace is meant.
#pragma once
#include "hp_common.h"

namespace {

constexpr double kDoubleMax = 1.7976931348623157e308;

struct Images {
    const void* depth;
    const unsigned char* mask;             // or nullptr
    const double* K;                       // (B,4): fx, fy, cx, cy
    int B, H, W, chunks;                   // chunks per image
    bool is_u16;
    double scale, near, far, jump_abs, jump_rel;
    int w;
};

__device__ __forceinline__ double depth_at(const Images& im, size_t g) {
    const double d = im.is_u16 ? (double)static_cast<const unsigned short*>(im.depth)[g]
                               : (double)static_cast<const float*>(im.depth)[g];
    return __dmul_rn(d, im.scale);
}

__device__ __forceinline__ bool measured(double z) { return z > 0.0 && z <= kDoubleMax; }     // false for a NaN

__device__ __forceinline__ bool jumps(const Images& im, double a, double b) {
    return fabs(__dsub_rn(a, b)) > __dadd_rn(im.jump_abs, __dmul_rn(im.jump_rel, a < b ? a : b));
}

// The keep test of pixel (v, u) with depth z of the image whose first pixel is `first`.
__device__ __forceinline__ bool kept(const Images& im, size_t first, int v, int u, double z) {
    if (!(measured(z) && z >= im.near && z <= im.far)) return false;
    if (im.mask != nullptr && im.mask[first + (size_t)v * im.W + u] == 0) return false;
    const int v0 = v - im.w > 0 ? v - im.w : 0, v1 = v + im.w < im.H - 1 ? v + im.w : im.H - 1;
    const int u0 = u - im.w > 0 ? u - im.w : 0, u1 = u + im.w < im.W - 1 ? u + im.w : im.W - 1;
    bool edge = false;
    for (int y = v0; y <= v1; ++y)
        for (int x = u0; x <= u1; ++x) {
            const double zz = depth_at(im, first + (size_t)y * im.W + x);      // the centre never jumps against itself
            edge |= measured(zz) && jumps(im, z, zz);
        }
    return !edge;
}

}  // namespace
