// Philox4x32-10, shared by the kernels that draw on the device (aux_kernels.hip, batch_maker.hip, mesh.hip, plane.hip,
// pose_trials.hip, scan_prep.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// ---- Philox4x32-10 (Salmon et al. 2011), counter-based: reproducible for a (seed, offset) pair
__device__ __forceinline__ uint4 philox4x32_10(uint4 ctr, uint2 key) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(M0, ctr.x), lo0 = M0 * ctr.x;
        const uint32_t hi1 = __umulhi(M1, ctr.z), lo1 = M1 * ctr.z;
        ctr = make_uint4(hi1 ^ ctr.y ^ key.x, lo1, hi0 ^ ctr.w ^ key.y, lo0);
        key.x += W0;
        key.y += W1;
    }
    return ctr;
}

// Sample row k (0..2) of trial h of an n-row scan: word 3h + k of the stream's words under `tag` (plane.hip, pose_trials.hip).
__device__ __forceinline__ int sample_row(uint2 key, uint2 stream, int h, int k, int n, uint32_t tag) {
    const uint32_t i = (uint32_t)(3 * h + k);
    const uint4 w = philox4x32_10(make_uint4(stream.x, stream.y, i >> 2, tag), key);
    const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
    return (int)__umulhi(ww[i & 3u], (uint32_t)n);
}

}  // namespace
