// Triangle meshes over one shared face list: n points per mesh drawn uniformly by area in one launch, and
// area-weighted vertex normals.  K meshes are K vertex arrays (K,V,3) decoded from one triangulated sphere; faces (F,3) is theirs
// in common.
//
// The sampling law, per mesh (include/hyperpocket_hip.h has it in full).  Every floating operation is one fp64 rounding:
//   c_f   = (b - a) x (c - a), products rounded, then their difference;  d_f = sqrt((cx*cx + cy*cy) + cz*cz), not finite -> 0
//   e     = the binary exponent of d_max (frexp);  w_f = (uint64) floor(ldexp(d_f, 40 - e)), so w_max is in [2^39, 2^40)
//   P_f   = w_0 + .. + w_f, integers below 2^55: exact in any order, which is what lets a parallel scan state the law
//   r_j   = mulhi64(word0 << 32 | word1, W) of Philox block j (key seed, counter (stream, j, kTagMesh));  face_j = min f: P_f > r_j
//   (u,v) = (word2, word3) * 2^-32, folded to (1-u, 1-v) where u + v > 1;  point_j = (a + u*e1) + v*e2, rounded to fp32 once
//
//   sample   grid (slices, K), one workgroup per (mesh, slice of the n samples).  Every slice builds the mesh's table again — F
//            cross products — so no workgroup waits for another and the launch stands alone.  Pass 1: thread t takes faces t,
//            t + T, .. (consecutive lanes, consecutive face rows), leaves d_f in slot f and the workgroup reduces max d.  Pass 2:
//            thread t takes the contiguous run of ceil(F/T) slots t owns, turns d into w, and one workgroup-wide exclusive
//            scan of the per-thread sums makes every slot its inclusive prefix P_f, in place.  Pass 3: each thread draws its
//            samples, a binary search over the slots each.  The slots (8 bytes a face) are LDS up to kLdsFaces faces and the
//            caller's workspace above, one private run per workgroup.  No atomics, no order of arrival anywhere.
//   normals  one thread per vertex walks its CSR list in ascending face order and sums the faces' c_f again (about six each);
//            one thread per face for the face normals.  No atomics either: the sum has one order.
#include "hp_common.h"
#include "hp_philox.h"

namespace {

constexpr int kMeshMaxFaces = 32768;       // = HP_MESH_MAX_FACES (include/hyperpocket_hip.h)
constexpr int kLdsFaces = 8192;            // the table of a mesh of at most this many faces stays in LDS (64 KiB, of the CU's 160)
constexpr int kMaxSamples = 1 << 24;
constexpr int kMaxSlices = 1024;
constexpr uint32_t kTagMesh = 3;           // tags 0-2 of the (stream, q, tag) counter belong to scan_prep.hip and batch_maker.hip
constexpr int kMaxWaves = 16;
constexpr int kScratchSlots = 2 * kMaxWaves;   // 8-byte slots of LDS ahead of the table: per-wave maxima and sums

// Test hooks (hp_mesh_sample_set_slices / hp_mesh_sample_set_lds_faces): 0 = the launcher's own choice.
std::atomic<int> g_slices{0};
std::atomic<int> g_lds_faces{kLdsFaces};

struct Cross {
    double x, y, z;
};

// The unnormalised normal of face f: (b - a) x (c - a) in fp64, one rounding per operation.
__device__ __forceinline__ Cross face_cross(const float* __restrict__ X, const int* __restrict__ faces, int f, double* a3 = nullptr,
                                            double* e1 = nullptr, double* e2 = nullptr) {
#pragma clang fp contract(off)
    const int ia = faces[f * 3], ib = faces[f * 3 + 1], ic = faces[f * 3 + 2];
    const double ax = X[ia * 3], ay = X[ia * 3 + 1], az = X[ia * 3 + 2];
    const double e1x = __dsub_rn((double)X[ib * 3], ax), e1y = __dsub_rn((double)X[ib * 3 + 1], ay),
                 e1z = __dsub_rn((double)X[ib * 3 + 2], az);
    const double e2x = __dsub_rn((double)X[ic * 3], ax), e2y = __dsub_rn((double)X[ic * 3 + 1], ay),
                 e2z = __dsub_rn((double)X[ic * 3 + 2], az);
    if (a3) {
        a3[0] = ax, a3[1] = ay, a3[2] = az;
        e1[0] = e1x, e1[1] = e1y, e1[2] = e1z;
        e2[0] = e2x, e2[1] = e2y, e2[2] = e2z;
    }
    Cross c;
    c.x = __dsub_rn(__dmul_rn(e1y, e2z), __dmul_rn(e1z, e2y));
    c.y = __dsub_rn(__dmul_rn(e1z, e2x), __dmul_rn(e1x, e2z));
    c.z = __dsub_rn(__dmul_rn(e1x, e2y), __dmul_rn(e1y, e2x));
    return c;
}

__device__ __forceinline__ double cross_length(const Cross& c) {
    return __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(c.x, c.x), __dmul_rn(c.y, c.y)), __dmul_rn(c.z, c.z)));
}

__device__ __forceinline__ bool finite64(double v) {
    return ((unsigned long long)__double_as_longlong(v) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}

__global__ __launch_bounds__(1024) void mesh_sample_kernel(int V, const float* __restrict__ verts, int F, const int* __restrict__ faces,
                                                           int n, int per_slice, unsigned long long seed,
                                                           const long long* __restrict__ streams, float* __restrict__ points,
                                                           int* __restrict__ face, double* __restrict__ area,
                                                           int* __restrict__ failed, unsigned long long* __restrict__ ws) {
    extern __shared__ unsigned long long lds[];            // the waves' partials (kScratchSlots), then the table when it is here
    double* wmax = reinterpret_cast<double*>(lds);
    unsigned long long* wsum = lds + kMaxWaves;
    const int k = blockIdx.y, slice = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    const int lane = tid & 63, wid = tid >> 6, nw = T >> 6;
    const float* X = verts + (long)k * V * 3;
    unsigned long long* slot = ws ? ws + ((long)k * gridDim.x + slice) * F : lds + kScratchSlots;
    const int j0 = slice * per_slice, j1 = min(n, j0 + per_slice);

    // ---- pass 1: d_f, and its maximum.  d >= 0 or NaN-free after the filter, so fmax is exact and order-free
    double dm = 0.0;
    for (int f = tid; f < F; f += T) {
        double d = cross_length(face_cross(X, faces, f));
        if (!finite64(d)) d = 0.0;
        slot[f] = (unsigned long long)__double_as_longlong(d);
        dm = fmax(dm, d);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dm = fmax(dm, __shfl_xor(dm, o, HP_WAVE));
    if (lane == 0) wmax[wid] = dm;
    __syncthreads();                                        // also: every slot is written
    double d_max = wmax[0];
    for (int w = 1; w < nw; ++w) d_max = fmax(d_max, wmax[w]);
    if (d_max == 0.0) {                                     // nothing to draw from: zeros, and said so
        for (int j = j0 + tid; j < j1; j += T) {
            float* P = points + ((long)k * n + j) * 3;
            P[0] = 0.f, P[1] = 0.f, P[2] = 0.f;
            face[(long)k * n + j] = 0;
        }
        if (slice == 0 && tid == 0) {
            area[k] = 0.0;
            failed[k] = 1;
        }
        return;
    }
    int e;
    (void)frexp(d_max, &e);

    // ---- pass 2: the integer weights and their inclusive prefix, in place.  Thread t owns slots [t * run, (t + 1) * run)
    const int run = (F + T - 1) / T;
    const int f0 = min(F, tid * run), f1 = min(F, f0 + run);
    unsigned long long mine = 0;
    for (int f = f0; f < f1; ++f) {
        const unsigned long long w = (unsigned long long)ldexp(__longlong_as_double((long long)slot[f]), 40 - e);
        slot[f] = w;
        mine += w;
    }
    unsigned long long inc = mine;
#pragma unroll
    for (int o = 1; o < HP_WAVE; o <<= 1) {
        const unsigned long long t = __shfl_up(inc, o, HP_WAVE);
        if (lane >= o) inc += t;
    }
    if (lane == HP_WAVE - 1) wsum[wid] = inc;
    __syncthreads();
    unsigned long long before = inc - mine, W = 0;
    for (int w = 0; w < nw; ++w) {
        if (w < wid) before += wsum[w];
        W += wsum[w];
    }
    for (int f = f0; f < f1; ++f) {
        before += slot[f];
        slot[f] = before;
    }
    __syncthreads();
    if (slice == 0 && tid == 0) {
        area[k] = ldexp((double)W, e - 41);
        failed[k] = 0;
    }

    // ---- pass 3: the samples of this slice
    const uint2 key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
    const unsigned long long sid = (unsigned long long)streams[k];
    for (int j = j0 + tid; j < j1; j += T) {
#pragma clang fp contract(off)
        const uint4 w = philox4x32_10(make_uint4((uint32_t)sid, (uint32_t)(sid >> 32), (uint32_t)j, kTagMesh), key);
        const unsigned long long r = __umul64hi(((unsigned long long)w.x << 32) | w.y, W);     // < W = slot[F - 1]
        int lo = 0, hi = F - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (slot[mid] > r)
                hi = mid;
            else
                lo = mid + 1;
        }
        double a[3], e1[3], e2[3];
        face_cross(X, faces, lo, a, e1, e2);
        double u = __dmul_rn((double)w.z, 0x1p-32), v = __dmul_rn((double)w.w, 0x1p-32);
        if (__dadd_rn(u, v) > 1.0) {
            u = __dsub_rn(1.0, u);
            v = __dsub_rn(1.0, v);
        }
        float* P = points + ((long)k * n + j) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) P[c] = (float)__dadd_rn(__dadd_rn(a[c], __dmul_rn(u, e1[c])), __dmul_rn(v, e2[c]));
        face[(long)k * n + j] = lo;
    }
}

__device__ __forceinline__ void store_unit(float* __restrict__ out, double x, double y, double z) {
#pragma clang fp contract(off)
    Cross c{x, y, z};
    const double len = cross_length(c);
    const bool ok = finite64(len) && len != 0.0;
    out[0] = ok ? (float)__ddiv_rn(x, len) : 0.f;
    out[1] = ok ? (float)__ddiv_rn(y, len) : 0.f;
    out[2] = ok ? (float)__ddiv_rn(z, len) : 0.f;
}

__global__ __launch_bounds__(256) void mesh_normals_kernel(int K, int V, const float* __restrict__ verts, int F,
                                                           const int* __restrict__ faces, const int* __restrict__ vf_offsets,
                                                           const int* __restrict__ vf_faces, float* __restrict__ face_normal,
                                                           float* __restrict__ vertex_normal) {
#pragma clang fp contract(off)
    const long per_mesh = (long)V + (face_normal ? F : 0), total = (long)K * per_mesh;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long item = (long)blockIdx.x * blockDim.x + threadIdx.x; item < total; item += stride) {
        const int k = (int)(item / per_mesh), i = (int)(item - (long)k * per_mesh);
        const float* X = verts + (long)k * V * 3;
        if (i < V) {
            double sx = 0.0, sy = 0.0, sz = 0.0;
            for (int p = vf_offsets[i]; p < vf_offsets[i + 1]; ++p) {
                const Cross c = face_cross(X, faces, vf_faces[p]);
                sx = __dadd_rn(sx, c.x);
                sy = __dadd_rn(sy, c.y);
                sz = __dadd_rn(sz, c.z);
            }
            store_unit(vertex_normal + ((long)k * V + i) * 3, sx, sy, sz);
        } else {
            const Cross c = face_cross(X, faces, i - V);
            store_unit(face_normal + ((long)k * F + (i - V)) * 3, c.x, c.y, c.z);
        }
    }
}

struct SamplePlan {
    int threads, slices, per_slice, lds;    // lds: 1 = the table is in LDS, 0 = in the workspace
};

// Slices: enough workgroups for the chip at small K (about four per CU), none with fewer than 256 samples — each slice pays
// for the whole table.  Threads: a face or more per lane, 256 at the least.
SamplePlan plan_for(int K, int F, int n) {
    SamplePlan p;
    p.threads = F <= 1024 ? 256 : F <= 4096 ? 512 : 1024;
    const int forced = g_slices.load(std::memory_order_relaxed);
    int slices = forced > 0 ? forced : std::min((1024 + K - 1) / std::max(K, 1), (n + 255) / 256);
    slices = std::max(1, std::min(std::min(slices, n), kMaxSlices));
    p.per_slice = (n + slices - 1) / slices;
    p.slices = (n + p.per_slice - 1) / p.per_slice;
    p.lds = F <= g_lds_faces.load(std::memory_order_relaxed);
    return p;
}

bool sample_shape_ok(int K, int V, int F, int n) {
    return K >= 0 && K <= 65535 && V >= 1 && V <= (1 << 24) && F >= 1 && F <= kMeshMaxFaces && n >= 1 && n <= kMaxSamples;
}

}  // namespace

// Test hook: s >= 1 forces that many sample slices per mesh (capped by n and 1024), 0 restores the launcher's choice.
// Returns the previous setting, -1 for a value outside [0, 1024] (nothing changes).
HP_API int hp_mesh_sample_set_slices(int s) {
    if (s < 0 || s > kMaxSlices) return -1;
    return g_slices.exchange(s);
}

// Test hook: meshes of more than `faces` faces keep their table in the workspace; 0 <= faces <= 8192, the default 8192.
// Returns the previous setting, -1 for a value outside the range (nothing changes).
HP_API int hp_mesh_sample_set_lds_faces(int faces) {
    if (faces < 0 || faces > kLdsFaces) return -1;
    return g_lds_faces.exchange(faces);
}

// What hp_mesh_sample launches for (K, F, n) under the current hooks.  Host only.
HP_API int hp_mesh_sample_plan(int K, int F, int n, int* threads, int* slices, int* in_lds) {
    HP_CHECK_ARG(sample_shape_ok(K, 1, F, n) && threads && slices && in_lds);
    const SamplePlan p = plan_for(K, F, n);
    *threads = p.threads;
    *slices = p.slices;
    *in_lds = p.lds;
    return 0;
}

// Bytes of `ws` hp_mesh_sample needs for (K, F, n) under the current hooks: 0 while the table fits LDS.  Host only.
HP_API long hp_mesh_sample_workspace_bytes(int K, int F, int n) {
    if (!sample_shape_ok(K, 1, F, n)) return -1;
    const SamplePlan p = plan_for(K, F, n);
    return p.lds ? 0 : (long)K * p.slices * F * (long)sizeof(unsigned long long);
}

// n points per mesh, uniform by area: see the law at the top and include/hyperpocket_hip.h.
HP_API int hp_mesh_sample(int K, int V, const float* verts, int F, const int* faces, int n, unsigned long long seed,
                          const long long* streams, float* points, int* face, double* area, int* failed, void* ws,
                          hipStream_t stream) {
    HP_CHECK_ARG(sample_shape_ok(K, V, F, n));
    HP_CHECK_ARG(verts && faces && streams && points && face && area && failed);
    const SamplePlan p = plan_for(K, F, n);
    HP_CHECK_ARG(p.lds || ws);
    if (K == 0) return 0;
    const size_t lds = ((size_t)kScratchSlots + (p.lds ? F : 0)) * sizeof(unsigned long long);
    if (lds > 64 * 1024)                                    // 8192 faces and the partials: 256 bytes past the default limit
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mesh_sample_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(mesh_sample_kernel, dim3(p.slices, K), dim3(p.threads), lds, stream, V, verts, F, faces, n, p.per_slice, seed, streams, points, face, area, failed,
                       p.lds ? nullptr : (unsigned long long*)ws);
    HP_RETURN_LAST_ERROR();
}

// Unit normals of K meshes: see the top and include/hyperpocket_hip.h.
HP_API int hp_mesh_normals(int K, int V, const float* verts, int F, const int* faces, const int* vf_offsets, const int* vf_faces,
                           float* face_normal, float* vertex_normal, hipStream_t stream) {
    HP_CHECK_ARG(K >= 0 && K <= 65535 && V >= 1 && V <= (1 << 24) && F >= 1 && F <= kMeshMaxFaces);
    HP_CHECK_ARG(verts && faces && vf_offsets && vf_faces && vertex_normal);
    if (K == 0) return 0;
    const long total = (long)K * ((long)V + (face_normal ? F : 0));
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(mesh_normals_kernel, dim3((unsigned)std::min(blocks, 65535L * 16)), dim3(256), 0, stream, K, V, verts, F, faces,
                       vf_offsets, vf_faces, face_normal, vertex_normal);
    HP_RETURN_LAST_ERROR();
}
