// Shared device helpers for the HyperPocket gfx950 kernels (wave64, CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <atomic>
#include <cstdlib>

#define HP_API extern "C" __attribute__((visibility("default")))

#define HP_WAVE 64

// Launch epilogue: the reference's launchers either check nothing (nndistance.cu:131-160) or throw
// std::runtime_error (approxmatch.cu:334-337).  The C-ABI returns the hipError_t instead.
#define HP_RETURN_LAST_ERROR() return (int)hipGetLastError()

#define HP_CHECK_ARG(cond) \
    do {                   \
        if (!(cond)) return -1; \
    } while (0)

// stream_order.hip: everything enqueued on `to` afterwards starts behind everything enqueued on `from` so far (an event per
// (device, from) under a mutex).  0 or a hipError_t.
int hp_order_streams(hipStream_t from, hipStream_t to);

namespace hp {

// A process-wide switch of the library, kept next to the code it selects.  Read once at load from the environment variable
// `env` (a whole decimal number in [lo, hi]; anything else leaves the default) and held atomically.  set(v): v < 0 restores the
// load-time value, any other v is clamped to [lo, hi]; returns the previous value.  An entry point reads each switch once.
class Switch {
  public:
    Switch(const char* env, int dflt, int lo = 0, int hi = 1) : lo_(lo), hi_(hi), load_(dflt) {
        const char* e = std::getenv(env);
        char* end = nullptr;
        const long v = e ? std::strtol(e, &end, 10) : 0;
        if (e && end != e && *end == '\0' && v >= lo && v <= hi) load_ = (int)v;
        v_.store(load_);
    }
    int get() const { return v_.load(std::memory_order_relaxed); }
    int set(int v) { return v_.exchange(v < 0 ? load_ : std::min(std::max(v, lo_), hi_)); }

  private:
    const int lo_, hi_;
    int load_;
    std::atomic<int> v_;
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, HP_WAVE);
    return v;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, HP_WAVE);
    return v;
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, HP_WAVE);
    return v;                                                                  // lane 0 holds the wave's sum
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_down(v, o, HP_WAVE));
    return v;
}

// Block-wide sum in a fixed order (wave partials combined by wave 0 in wave order): deterministic.
// `scratch` must hold blockDim.x/64 elements.  Result valid in thread 0.
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* scratch) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_sum(v);
    if (lane == 0) scratch[wid] = v;
    __syncthreads();
    T r = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < nw; ++w) r += scratch[w];
    __syncthreads();
    return r;
}

// The scan kernels' test of a coordinate, on its bits: neither an infinity nor a NaN.  A row with such a coordinate is absent.
constexpr unsigned kInfBits = 0x7F800000u;
constexpr int kNanBits = 0x7FC00000;       // the quiet NaN with no payload, what an absent value is written as

__device__ __forceinline__ bool finite_bits(float v) { return ((unsigned)__float_as_int(v) & kInfBits) != kInfBits; }

// The scan of a row of a ragged set: the last s with offsets[s] <= row (scan 0 when there is none: its bounds then refuse the
// row).  At most log2(S) + 1 steps.
__device__ __forceinline__ int scan_of(const long long* __restrict__ offsets, int S, long long row) {
    int s = 0;
    for (int hi = S; hi - s > 1;) {
        const int mid = (s + hi) >> 1;
        if (offsets[mid] <= row) s = mid;
        else hi = mid;
    }
    return s;
}

// One output row of the batch makers (batch_maker.hip, view_split.hip): z-rotation by (c, s) = (cos, sin); `rotate` false
// copies the bits.
__device__ __forceinline__ float3 out_row(float x, float y, float z, bool rotate, float c, float s) {
#pragma clang fp contract(off)
    if (!rotate) return make_float3(x, y, z);
    return make_float3(__fmaf_rn(x, c, __fmul_rn(y, s)), __fmaf_rn(y, c, -__fmul_rn(x, s)), z);
}

// squared distance with the fma chain the oracle uses: fma(dz,dz,fma(dy,dy,dx*dx))
__device__ __forceinline__ float sqdist(float dx, float dy, float dz) {
    return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
}
// ... of two candidates to one point, per element the same chain: packed fp32 ops, two candidates per instruction
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 splat2(float v) { return f2{v, v}; }
__device__ __forceinline__ f2 sqdist2(f2 dx, f2 dy, f2 dz) {
    return __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
}

}  // namespace hp
