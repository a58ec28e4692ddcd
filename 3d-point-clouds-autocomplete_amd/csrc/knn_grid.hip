// k nearest neighbours over ragged scans behind a uniform grid: knn.hip's law, bit for bit, for scans of up to
// 2^22 rows, and statistical outlier removal on top of it with sums that hold 2^22 rows.
//
// The law is knn.hip's (include/hyperpocket_hip.h, tests/knn_law.py): d2 = ((dx*dx + dy*dy) + dz*dz) with one fp32 rounding per
// operation, absent rows, candidates ordered by (bits of d2, row), the first k.  The grid only decides which rows a query
// looks at, and in which order; the key (bits, row) is a total order, so neither shows in the result.
//
//   setup    grid (S), one workgroup per scan: the box of the present rows, a cell edge h — the caller's request, or from the
//            occupied cells of coarse histograms of 32^3, 16^3 and 8^3 cells (scans are surfaces: how the occupied cells
//            multiply with the resolution, not the box volume, says how many rows a cell of edge h holds) aiming at k/2
//            rows per occupied cell — raised by bisection to the smallest
//            edge with at most 1024 cells per axis and at most 2 n_s + 64 cells in all; an axis of zero or overflowed extent
//            has one cell.  It also zeroes the scan's cell counters.
//   cells    edge_c(j) = fl(lo_c + fl(float(j) * h)) is monotone in j.  A coordinate x lies in the largest cell j of
//            [0, G_c) with edge_c(j) <= x, cell 0 if there is none: the first and the last cell are unbounded outwards, and
//            edge_c(j) <= x < edge_c(j + 1) holds for every inner cell by construction (a binary search over the edges, no
//            quotient).  That is what makes the pruning bound below exact in fp32 without an epsilon.
//   bin      count per cell (integer atomics), an exclusive prefix per scan, scatter of (x, y, z, row) as float4 into cell
//            order; queries of a second set get the same treatment with the points' grid.  The order inside a cell is that
//            of the atomics, arbitrary.  Rows that are not searched (absent, or of a scan that is empty, beyond the cap or
//            without a present candidate) get the empty result here.
//   sweep    one wave (a workgroup of 64) per 64 consecutive queries in cell order.  Its lanes are served in groups — the first
//            lane not served yet and the lanes behind it on the same (y, z) line of cells within 16 cells: neighbours in
//            space even where the cell order jumps (the end of a line, a surface that leaves the line).  A group takes the
//            block of cells that covers its queries' cells, grown by r shells, and streams the rows of those cells (one
//            contiguous run per (y, z) line of the block, the run bounds fetched 64 lines at a time, one per lane) through
//            an LDS tile that every lane reads at one address.  A lane keeps its K best keys sorted in registers and
//            inserts on the full key.  A lane is done iff its list is full and its worst d2 is strictly below the smallest of
//            fl(fl(edge_face - q_c)^2) over the block's six faces (a face at the grid's end counts +inf): fp32 subtraction,
//            squaring and the addition of non-negative terms are monotone, so every row outside the block has a d2 of at
//            least that bound, and strictness keeps a tie to a lower row outside from mattering.  While a lane is not done
//            the block grows — doubling until the lists are full, then to the radius the worst distances ask for — and only
//            the new shell is swept.  The whole grid ends every lane; every loop is bounded by the grid.
//   keep     knn.hip's statistics with S2 = sum q^2 held as two sums (the low and the high 32 bits of each square), combined
//            exactly (up to 70 bits) and rounded to fp64 to nearest even by hand; equal to knn.hip's wherever that is defined.
#include "hp_knn.h"

namespace {

using hp::finite_bits, hp::kInfBits, hp::scan_of;
using hp_knn::kEmpty;
constexpr int kGridMaxPoints = 1 << 22;    // = HP_KNN_GRID_MAX_POINTS (include/hyperpocket_hip.h)
constexpr int kMaxCells = 1024;            // per axis
constexpr int kSetupThreads = 1024;
constexpr int kBinThreads = 256;
constexpr int kBinGrid = 2048;
constexpr int kSweepGrid = 8192;           // waves of a launch: the query count lives on the device
constexpr int kTile = 256;                 // candidates per LDS tile (4 KiB per wave)
constexpr int kSpan = 16;                  // cells along x a group of lanes may span
constexpr int kGroup = 4;                  // candidates per look at the lists; kTile is a multiple
constexpr int kStatThreads = 1024;

struct Scan {                              // the grid of one scan, in the workspace; np == 0: nothing to search
    float lo[3], h;
    int G[3], np;
};

struct Layout {
    long long cells_p, sorted_p, cells_q, sorted_q, need;
};

__host__ __device__ inline long long up16(long long v) { return (v + 15) & ~15LL; }

// The workspace for S scans of T rows in all and Q rows of a second query set (Q <= 0: the scans query themselves).
__host__ __device__ inline Layout layout(int S, long long T, long long Q) {
    Layout L;
    const long long cells = up16((2 * T + 65LL * S) * 4);      // per scan 2 n_s + 64 cells and one spare
    long long off = up16((long long)S * (long long)sizeof(Scan));
    L.cells_p = off, off += cells;
    L.sorted_p = off, off += T * 16;
    L.cells_q = off, off += Q > 0 ? cells : 0;
    L.sorted_q = off, off += Q > 0 ? Q * 16 : 0;
    L.need = off;
    return L;
}

__device__ __forceinline__ long long cell_base(const long long* offsets, int s) { return 2 * offsets[s] + 65LL * s; }

__device__ __forceinline__ unsigned ordered(float v) {          // floats as unsigned integers in their order
    const unsigned b = (unsigned)__float_as_int(v);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float unordered(unsigned u) {
    return __int_as_float((int)(u ^ ((u >> 31) ? 0x80000000u : 0xFFFFFFFFu)));
}

__device__ __forceinline__ float edge(float lo, float h, int j) { return __fadd_rn(lo, __fmul_rn((float)j, h)); }

// The largest j of [0, G) with edge(j) <= x, 0 if none.
__device__ __forceinline__ int cell_of(float x, float lo, float h, int G) {
    int a = 0, b = G - 1;
    while (a < b) {
        const int m = (a + b + 1) >> 1;
        if (edge(lo, h, m) <= x) a = m;
        else b = m - 1;
    }
    return a;
}

__global__ __launch_bounds__(kSetupThreads) void grid_setup_kernel(int S, const float* __restrict__ points,
                                                                   const long long* __restrict__ offsets,
                                                                   const long long* __restrict__ qoffsets, const float* __restrict__ cell,
                                                                   int k, char* __restrict__ ws, long long ws_bytes,
                                                                   float* __restrict__ grid_out) {
#pragma clang fp contract(off)
    __shared__ unsigned sLo[3], sHi[3], sOcc[1024];
    __shared__ int sNp, sCells[3];                              // occupied cells of the 32^3, 16^3 and 8^3 histograms
    __shared__ Scan sP;
    const int s = blockIdx.x, tid = threadIdx.x;
    const Layout L = layout(S, offsets[S], qoffsets ? qoffsets[S] : 0);
    const long long plo = offsets[s], n = offsets[s + 1] - plo;
    const bool fits = L.need <= ws_bytes;
    if (!fits || n < 1 || n > kGridMaxPoints) {                 // uniform over the workgroup
        if (tid == 0) {
            if (fits) {
                Scan none = {};
                reinterpret_cast<Scan*>(ws)[s] = none;
            }
            if (grid_out)
                for (int c = 0; c < 4; ++c) grid_out[s * 4 + c] = 0.f;
        }
        return;
    }
    const float* P = points + plo * 3;
    if (tid < 3) sLo[tid] = 0xFFFFFFFFu, sHi[tid] = 0u;
    if (tid == 0) sNp = 0, sCells[0] = sCells[1] = sCells[2] = 0;
    sOcc[tid] = 0u;
    __syncthreads();
    unsigned mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0u, 0u, 0u};
    int cnt = 0;
    for (long long i = tid; i < n; i += kSetupThreads) {
        const float v[3] = {P[i * 3], P[i * 3 + 1], P[i * 3 + 2]};
        if (finite_bits(v[0]) && finite_bits(v[1]) && finite_bits(v[2])) {
            ++cnt;
            for (int c = 0; c < 3; ++c) {
                const unsigned o = ordered(v[c]);
                mn[c] = o < mn[c] ? o : mn[c];
                mx[c] = o > mx[c] ? o : mx[c];
            }
        }
    }
    if (cnt) {
        for (int c = 0; c < 3; ++c) atomicMin(&sLo[c], mn[c]), atomicMax(&sHi[c], mx[c]);
        atomicAdd(&sNp, cnt);
    }
    __syncthreads();
    const int np = sNp;
    float lo[3] = {0.f, 0.f, 0.f}, ext[3] = {0.f, 0.f, 0.f}, emax = 0.f;
    bool good[3] = {false, false, false};
    if (np > 0) {
        for (int c = 0; c < 3; ++c) {
            lo[c] = unordered(sLo[c]);
            ext[c] = __fsub_rn(unordered(sHi[c]), lo[c]);
            good[c] = ext[c] > 0.f && finite_bits(ext[c]);      // zero or overflowed extent: one cell
            if (good[c]) emax = fmaxf(emax, ext[c]);
        }
    }
    const float ask = cell ? cell[s] : 0.f;
    const bool asked = ask > 0.f && finite_bits(ask);
    if (np > 0 && emax > 0.f && !asked) {                       // the occupied cells of a coarse 32^3 grid over the box
        const float inv = 32.f / emax;
        for (long long i = tid; i < n; i += kSetupThreads) {
            const float v[3] = {P[i * 3], P[i * 3 + 1], P[i * 3 + 2]};
            if (finite_bits(v[0]) && finite_bits(v[1]) && finite_bits(v[2])) {
                int bit = 0;
                for (int c = 2; c >= 0; --c) {
                    int q = 0;
                    if (good[c]) {
                        const float t = (v[c] - lo[c]) * inv;
                        q = t < 31.f ? (int)t : 31;
                        q = q < 0 ? 0 : q;
                    }
                    bit = bit * 32 + q;
                }
                atomicOr(&sOcc[bit >> 5], 1u << (bit & 31));
            }
        }
        __syncthreads();
        {                                                       // word w = (z, y) holds the 32 cells along x
            const int c = __popc(sOcc[tid]);
            if (c) atomicAdd(&sCells[0], c);
        }
        if (tid < 256) {                                        // 16^3: 2 x 2 words, then pairs of bits
            const int z = tid >> 4, y = tid & 15;
            unsigned m = 0u;
            for (int u = 0; u < 4; ++u) m |= sOcc[(2 * z + (u >> 1)) * 32 + 2 * y + (u & 1)];
            const int c = __popc((m | (m >> 1)) & 0x55555555u);
            if (c) atomicAdd(&sCells[1], c);
        }
        if (tid < 64) {                                         // 8^3: 4 x 4 words, then fours of bits
            const int z = tid >> 3, y = tid & 7;
            unsigned m = 0u;
            for (int u = 0; u < 16; ++u) m |= sOcc[(4 * z + (u >> 2)) * 32 + 4 * y + (u & 3)];
            const int c = __popc((m | (m >> 1) | (m >> 2) | (m >> 3)) & 0x11111111u);
            if (c) atomicAdd(&sCells[2], c);
        }
    }
    __syncthreads();
    if (tid == 0) {
        Scan p = {};
        p.np = np;
        p.G[0] = p.G[1] = p.G[2] = 1;
        for (int c = 0; c < 3; ++c) p.lo[c] = lo[c];
        p.h = asked ? ask : 1.f;                                // a box without extent: one cell, whatever its edge
        if (np > 0 && emax > 0.f) {
            const long long budget = 2 * n + 64;
            int G[3];
            auto feasible = [&](float h) {
                long long all = 1;
                for (int c = 0; c < 3; ++c) {
                    G[c] = 1;
                    if (!good[c]) continue;
                    const float g = ext[c] / h;
                    if (!(g < (float)kMaxCells)) return false;
                    G[c] = (int)g + 1;
                    all *= G[c];
                }
                return all <= budget;
            };
            float h = ask;
            if (!asked) {
                // How the occupied cells multiply from one histogram to the next finer one is the dimension d of what the
                // scan samples (a curve 1, a surface 2, a volume 3); the pair that shows the larger one is the one the rows
                // still fill.  Occupied cells of edge e split into (e / h)^d occupied cells of edge h: k/2 rows in each.
                const float per = k > 2 ? 0.5f * (float)k : 1.f;
                const float c32 = (float)sCells[0], c16 = (float)sCells[1], c8 = (float)sCells[2];
                const float d32 = log2f(c32 / c16), d16 = log2f(c16 / c8);
                const bool fine = d32 >= d16;
                const float d = fminf(fmaxf(fine ? d32 : d16, 1.f), 3.f);
                h = emax * (fine ? 1.f / 32.f : 1.f / 16.f) * powf((fine ? c32 : c16) * per / (float)np, 1.f / d);
            }
            if (!(h > 0.f) || !finite_bits(h)) h = emax;
            if (!feasible(h)) {                                 // then h < emax; the smallest edge the caps allow: emax itself gives <= 8 cells
                float bad = h, ok = emax;
                for (int it = 0; it < 64; ++it) {
                    const float mid = 0.5f * bad + 0.5f * ok;
                    if (!(mid > bad && mid < ok)) break;
                    if (feasible(mid)) ok = mid;
                    else bad = mid;
                }
                h = ok;
                feasible(h);
            }
            p.h = h;
            for (int c = 0; c < 3; ++c) p.G[c] = G[c];
        }
        sP = p;
        reinterpret_cast<Scan*>(ws)[s] = p;
        if (grid_out) {
            grid_out[s * 4] = np > 0 ? p.h : 0.f;
            for (int c = 0; c < 3; ++c) grid_out[s * 4 + 1 + c] = np > 0 ? (float)p.G[c] : 0.f;
        }
    }
    __syncthreads();
    if (np == 0) return;
    const long long cb = cell_base(offsets, s);
    const int all = sP.G[0] * sP.G[1] * sP.G[2];                // <= 2 n + 64; one spare behind
    int* cp = reinterpret_cast<int*>(ws + L.cells_p) + cb;
    for (int c = tid; c <= all; c += kSetupThreads) cp[c] = 0;
    if (qoffsets && qoffsets[S] > 0) {
        int* cq = reinterpret_cast<int*>(ws + L.cells_q) + cb;
        for (int c = tid; c <= all; c += kSetupThreads) cq[c] = 0;
    }
}

// Rows of one ragged set X (the points, or the queries of a second set) into the cells of the points' grids: the count, or —
// behind the prefix — the scatter into cell order.  fill: the rows are queries, and one that is not searched gets the empty
// result here (the count pass only).
template <bool SCATTER>
__global__ __launch_bounds__(kBinThreads) void grid_bin_kernel(int S, const float* __restrict__ X, const long long* __restrict__ xoff,
                                                               const long long* __restrict__ offsets,
                                                               const long long* __restrict__ qoffsets, int as_queries, int fill, int k,
                                                               int* __restrict__ index, float* __restrict__ dist2,
                                                               float* __restrict__ mean_dist, char* __restrict__ ws, long long ws_bytes) {
#pragma clang fp contract(off)
    const Layout L = layout(S, offsets[S], qoffsets ? qoffsets[S] : 0);
    const bool fits = L.need <= ws_bytes;
    const Scan* scans = reinterpret_cast<const Scan*>(ws);
    int* cells = reinterpret_cast<int*>(ws + (as_queries ? L.cells_q : L.cells_p));
    float4* sorted = reinterpret_cast<float4*>(ws + (as_queries ? L.sorted_q : L.sorted_p));
    const long long R = xoff[S];
    for (long long i = (long long)blockIdx.x * kBinThreads + threadIdx.x; i < R; i += (long long)gridDim.x * kBinThreads) {
        const int s = scan_of(xoff, S, i);
        const float x = X[i * 3], y = X[i * 3 + 1], z = X[i * 3 + 2];
        bool searched = fits && finite_bits(x) && finite_bits(y) && finite_bits(z);
        if (searched) {
            const Scan p = scans[s];
            searched = p.np > 0;
            if (searched) {
                const int cx = cell_of(x, p.lo[0], p.h, p.G[0]), cy = cell_of(y, p.lo[1], p.h, p.G[1]),
                          cz = cell_of(z, p.lo[2], p.h, p.G[2]);
                int* c = cells + cell_base(offsets, s) + ((long long)(cz * p.G[1] + cy) * p.G[0] + cx);
                if (SCATTER) {
                    const int pos = atomicAdd(c, 1);            // the cell's next free place: in the end, the cell's end
                    sorted[xoff[s] + pos] = make_float4(x, y, z, __int_as_float((int)(i - xoff[s])));
                } else {
                    atomicAdd(c, 1);
                }
            }
        }
        if (!SCATTER && fill && !searched) {
            if (mean_dist) mean_dist[i] = __int_as_float((int)kInfBits);
            if (index)
                for (int t = 0; t < k; ++t) index[i * k + t] = -1, dist2[i * k + t] = __int_as_float((int)kInfBits);
        }
    }
}

// Counts -> exclusive starts, in place, per scan (blockIdx.y: the points' cells, the queries' cells).
__global__ __launch_bounds__(1024) void grid_prefix_kernel(int S, const long long* __restrict__ offsets,
                                                           const long long* __restrict__ qoffsets, char* __restrict__ ws,
                                                           long long ws_bytes) {
    __shared__ int sWave[16];
    __shared__ int sCarry;
    const Layout L = layout(S, offsets[S], qoffsets ? qoffsets[S] : 0);
    if (L.need > ws_bytes || (blockIdx.y && !(qoffsets && qoffsets[S] > 0))) return;     // no query row: no query cells
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const Scan p = reinterpret_cast<const Scan*>(ws)[s];
    if (p.np == 0) return;
    int* cells = reinterpret_cast<int*>(ws + (blockIdx.y ? L.cells_q : L.cells_p)) + cell_base(offsets, s);
    const int all = p.G[0] * p.G[1] * p.G[2];
    if (tid == 0) sCarry = 0;
    __syncthreads();
    for (int c0 = 0; c0 < all; c0 += 4096) {
        const int c = c0 + tid * 4;
        int v[4], sum = 0;
        for (int u = 0; u < 4; ++u) {
            v[u] = c + u < all ? cells[c + u] : 0;
            sum += v[u];
        }
        int inc = sum;                                          // inclusive over the wave
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (lane == 63) sWave[wid] = inc;
        __syncthreads();
        int before = sCarry;
        for (int w = 0; w < wid; ++w) before += sWave[w];
        int run = before + inc - sum;
        for (int u = 0; u < 4; ++u) {
            if (c + u < all) cells[c + u] = run;
            run += v[u];
        }
        __syncthreads();
        if (tid == 1023) sCarry = run;
        __syncthreads();
    }
}

__device__ __forceinline__ int wave_max_all(int v) {
    for (int o = 32; o > 0; o >>= 1) {
        const int t = __shfl_xor(v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}

template <int K, bool MEAN>
__global__ __launch_bounds__(64) void grid_sweep_kernel(int S, const long long* __restrict__ offsets,
                                                        const long long* __restrict__ qoffsets_or_null, int k, int exclude_self,
                                                        int* __restrict__ index, float* __restrict__ dist2,
                                                        float* __restrict__ mean_dist, const char* __restrict__ ws, long long ws_bytes) {
#pragma clang fp contract(off)
    __shared__ float4 tile[kTile];
    const bool cross = qoffsets_or_null != nullptr;
    const long long* qoffsets = cross ? qoffsets_or_null : offsets;
    const Layout L = layout(S, offsets[S], cross ? qoffsets[S] : 0);
    if (L.need > ws_bytes) return;                              // the bin pass has written the empty result everywhere
    const int lane = threadIdx.x;
    const Scan* scans = reinterpret_cast<const Scan*>(ws);
    const int* cells_p = reinterpret_cast<const int*>(ws + L.cells_p);
    const int* cells_q = reinterpret_cast<const int*>(ws + L.cells_q);
    const float4* sorted_p = reinterpret_cast<const float4*>(ws + L.sorted_p);
    const float4* sorted_q = cross ? reinterpret_cast<const float4*>(ws + L.sorted_q) : sorted_p;
    const long long Q = qoffsets[S];
    for (long long g0 = (long long)blockIdx.x * 64; g0 < Q; g0 += (long long)gridDim.x * 64) {
        const long long last = (g0 + 64 < Q ? g0 + 64 : Q) - 1;
        for (int s = scan_of(qoffsets, S, g0); s < S && qoffsets[s] <= last; ++s) {      // uniform over the wave
            const Scan P = scans[s];
            if (P.np == 0) continue;
            const int Gx = P.G[0], Gy = P.G[1], Gz = P.G[2], all = Gx * Gy * Gz;
            const long long cb = cell_base(offsets, s), qlo = qoffsets[s];
            const int nq = cross ? cells_q[cb + all - 1] : P.np;                         // the end of the last cell
            const long long g = g0 + lane;
            const bool active = g >= qlo && g < qlo + nq;
            if (!__any(active)) continue;
            const float4 qv = active ? sorted_q[g] : make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
            const float qx = qv.x, qy = qv.y, qz = qv.z;
            const int qrow = __float_as_int(qv.w);
            const int self = active && exclude_self ? qrow : -1;
            const int* cells = cells_p + cb;
            const float4* cand = sorted_p + offsets[s];

            unsigned d[K];
            int j[K];
#pragma unroll
            for (int t = 0; t < K; ++t) {
                d[t] = kEmpty;
                j[t] = -1;
            }
            const int cx = cell_of(qx, P.lo[0], P.h, Gx), cy = cell_of(qy, P.lo[1], P.h, Gy), cz = cell_of(qz, P.lo[2], P.h, Gz);
            // The lanes are served in groups: the first lane not served yet and the lanes behind it on its (y, z) line of
            // cells within kSpan cells — neighbours in space even where the cell order jumps (the end of a line, a surface
            // that leaves the line).  Each lane belongs to one group; the others wait with their lists untouched.
            for (unsigned long long todo = __ballot(active); todo;) {
                const int leader = __ffsll((long long)todo) - 1;
                const int x0 = __shfl(cx, leader, 64), y0 = __shfl(cy, leader, 64), z0 = __shfl(cz, leader, 64), y1 = y0, z1 = z0;
                const bool mine = active && ((todo >> lane) & 1ull) && cy == y0 && cz == z0 && cx >= x0 && cx - x0 < kSpan;
                const int x1 = wave_max_all(mine ? cx : -1);
                todo &= ~__ballot(mine);
                int fill = 0;
                auto flush = [&]() __attribute__((always_inline)) {     // every lane against the tile's rows, all at one address
                    __syncthreads();
                    for (int c0 = 0; c0 < fill; c0 += kGroup) {
                        float4 p[kGroup];
                        unsigned bits[kGroup];
#pragma unroll
                        for (int u = 0; u < kGroup; ++u) p[u] = tile[c0 + u];
#pragma unroll
                        for (int u = 0; u < kGroup; ++u) bits[u] = hp_knn::d2_bits(qx, qy, qz, p[u].x, p[u].y, p[u].z);
#pragma unroll
                        for (int u = 0; u < kGroup; ++u) {
                            const int row = __float_as_int(p[u].w);
                            const bool take =
                                mine && c0 + u < fill && row != self && hp_knn::key_above(d[K - 1], j[K - 1], bits[u], row);
                            if (__any(take)) {
                                if (take) hp_knn::insert_key<K>(d, j, bits[u], row);
                            }
                        }
                    }
                    __syncthreads();
                    fill = 0;
                };
                auto run = [&](int a, int b) __attribute__((always_inline)) {   // rows [a, b) of the scan in cell order; uniform
                    while (a < b) {
                        const int room = kTile - fill, m = b - a < room ? b - a : room;
                        for (int i = lane; i < m; i += 64) tile[fill + i] = cand[a + i];
                        fill += m;
                        a += m;
                        if (fill == kTile) flush();
                    }
                };

                int px0 = 1, px1 = 0, py0 = 1, py1 = 0, pz0 = 1, pz1 = 0;                    // the block swept so far: none
                for (int r = 0;;) {
                    const int bx0 = x0 - r > 0 ? x0 - r : 0, bx1 = x1 + r < Gx - 1 ? x1 + r : Gx - 1;
                    const int by0 = y0 - r > 0 ? y0 - r : 0, by1 = y1 + r < Gy - 1 ? y1 + r : Gy - 1;
                    const int bz0 = z0 - r > 0 ? z0 - r : 0, bz1 = z1 + r < Gz - 1 ? z1 + r : Gz - 1;
                    const int ny = by1 - by0 + 1, lines = ny * (bz1 - bz0 + 1);
                    for (int l0 = 0; l0 < lines; l0 += 64) {        // 64 (y, z) lines of the block, one per lane
                        int a0 = 0, b0 = 0, a1 = 0, b1 = 0;
                        const int l = l0 + lane;
                        if (l < lines) {
                            const int y = by0 + l % ny, z = bz0 + l / ny;
                            const int line = (z * Gy + y) * Gx;
                            auto start = [&](int c) { return c > 0 ? cells[c - 1] : 0; };
                            if (px0 <= px1 && y >= py0 && y <= py1 && z >= pz0 && z <= pz1) {   // swept before: its two ends only
                                if (bx0 < px0) a0 = start(line + bx0), b0 = cells[line + px0 - 1];
                                if (bx1 > px1) a1 = cells[line + px1], b1 = cells[line + bx1];
                            } else {
                                a0 = start(line + bx0), b0 = cells[line + bx1];
                            }
                        }
                        const int cnt = lines - l0 < 64 ? lines - l0 : 64;
                        for (int u = 0; u < cnt; ++u) {
                            run(__builtin_amdgcn_readfirstlane(__shfl(a0, u, 64)), __builtin_amdgcn_readfirstlane(__shfl(b0, u, 64)));
                            run(__builtin_amdgcn_readfirstlane(__shfl(a1, u, 64)), __builtin_amdgcn_readfirstlane(__shfl(b1, u, 64)));
                        }
                    }
                    if (fill) flush();
                    if (bx0 == 0 && bx1 == Gx - 1 && by0 == 0 && by1 == Gy - 1 && bz0 == 0 && bz1 == Gz - 1) break;   // the whole scan
                    // the smallest d2 a row outside the block can have, per lane: fl(fl(face - q)^2) over the faces inside the grid
                    unsigned bound = kInfBits;
                    auto face = [&](float e, float q, bool low) {
                        const float t = low ? __fsub_rn(q, e) : __fsub_rn(e, q);
                        const unsigned b = (unsigned)__float_as_int(__fmul_rn(t, t));
                        bound = b < bound ? b : bound;
                    };
                    if (bx0 > 0) face(edge(P.lo[0], P.h, bx0), qx, true);
                    if (bx1 < Gx - 1) face(edge(P.lo[0], P.h, bx1 + 1), qx, false);
                    if (by0 > 0) face(edge(P.lo[1], P.h, by0), qy, true);
                    if (by1 < Gy - 1) face(edge(P.lo[1], P.h, by1 + 1), qy, false);
                    if (bz0 > 0) face(edge(P.lo[2], P.h, bz0), qz, true);
                    if (bz1 < Gz - 1) face(edge(P.lo[2], P.h, bz1 + 1), qz, false);
                    const bool full = d[K - 1] != kEmpty;
                    const bool open = mine && !(full && d[K - 1] < bound);
                    if (!__any(open)) break;
                    int want = r + 1;
                    if (__any(mine && !full)) {
                        want = r ? 2 * r : 1;
                    } else if (open) {                          // the shells the worst distance reaches over: a guess, the rule decides
                        const float t = __fsqrt_rn(__int_as_float((int)d[K - 1])) / P.h;
                        const int reach = t < (float)(kMaxCells - 1) ? (int)t + 1 : kMaxCells;
                        want = reach > want ? reach : want;
                    }
                    px0 = bx0, px1 = bx1, py0 = by0, py1 = by1, pz0 = bz0, pz1 = bz1;
                    r = wave_max_all(want);
                }
                const long long q = qlo + qrow;
                if (mine && MEAN) mean_dist[q] = hp_knn::mean_root<K>(d, k);
                if (mine && !MEAN) {
#pragma unroll
                    for (int t = 0; t < K; ++t) {
                        if (t < k) {
                            index[q * k + t] = j[t];
                            dist2[q * k + t] = __int_as_float((int)(d[t] == kEmpty ? kInfBits : d[t]));
                        }
                    }
                }
            }
        }
    }
}

// Per scan: which rows stay (knn.hip's statistics, S2 exact up to 2^22 rows).  m = mean_dist; a row takes part when its m is
// finite.
__global__ __launch_bounds__(kStatThreads) void outlier_keep_kernel(const float* __restrict__ mean_dist,
                                                                    const long long* __restrict__ offsets, float ratio,
                                                                    unsigned char* __restrict__ keep, int* __restrict__ kept) {
#pragma clang fp contract(off)
    __shared__ unsigned sM;
    __shared__ int sN, sKept;
    __shared__ unsigned long long sS1, sLow, sHigh;
    const int s = blockIdx.x, tid = threadIdx.x;
    const long long lo = offsets[s], n = offsets[s + 1] - lo;
    const float* m = mean_dist + lo;
    unsigned char* K = keep + lo;
    if (n > kGridMaxPoints) {                                   // beyond the cap: keeps nothing
        for (long long i = tid; i < n; i += kStatThreads) K[i] = 0;
        if (tid == 0) kept[s] = 0;
        return;
    }
    if (tid == 0) {
        sM = 0u;
        sN = 0;
        sKept = 0;
        sS1 = sLow = sHigh = 0ull;
    }
    __syncthreads();
    unsigned mx = 0u;
    int cnt = 0;
    for (long long i = tid; i < n; i += kStatThreads) {
        const unsigned b = (unsigned)__float_as_int(m[i]);     // m >= 0: the bits order as integers
        if (b < kInfBits) {
            mx = b > mx ? b : mx;
            ++cnt;
        }
    }
    atomicMax(&sM, mx);
    atomicAdd(&sN, cnt);
    __syncthreads();
    const unsigned M = sM;
    const int np = sN;
    if (np <= 1 || M == 0u) {                                  // uniform: nothing to compare, every participant stays
        for (long long i = tid; i < n; i += kStatThreads) K[i] = (unsigned)__float_as_int(m[i]) < kInfBits ? 1 : 0;
        if (tid == 0) kept[s] = np;
        return;
    }
    const int field = (int)(M >> 23);
    const int e = field ? field - 127 : (31 - __clz((int)(M & 0x7FFFFFu))) - 149;
    const double scale = __longlong_as_double((long long)(1023 + 23 - e) << 52);
    auto quant = [&](float v) { return (unsigned)__dmul_rn((double)v, scale); };
    unsigned long long s1 = 0ull, low = 0ull, high = 0ull;
    for (long long i = tid; i < n; i += kStatThreads) {
        const float v = m[i];
        if ((unsigned)__float_as_int(v) < kInfBits) {
            const unsigned long long qi = quant(v), sq = qi * qi;      // q < 2^24: the square below 2^48
            s1 += qi;
            low += sq & 0xFFFFFFFFull;                          // each sum below 2^54 over 2^22 rows
            high += sq >> 32;
        }
    }
    atomicAdd(&sS1, s1);
    atomicAdd(&sLow, low);
    atomicAdd(&sHigh, high);
    __syncthreads();
    // S2 = high * 2^32 + low as (top, bot) of 128 bits, then to fp64 by round-to-nearest-even
    const unsigned long long H = sHigh, Lw = sLow, shifted = H << 32, bot = shifted + Lw;
    const unsigned long long top = (H >> 32) + (bot < shifted ? 1ull : 0ull);
    double S2;
    if (top == 0ull) {
        S2 = __ull2double_rn(bot);
    } else {
        const int sh = (64 - __clzll((long long)top)) + 11;    // the bits below the 53 kept: 12 .. 17 here
        unsigned long long mant = (top << (64 - sh)) | (bot >> sh);
        const unsigned long long rem = bot & ((1ull << sh) - 1ull), half = 1ull << (sh - 1);
        if (rem > half || (rem == half && (mant & 1ull))) ++mant;
        S2 = __dmul_rn(__ull2double_rn(mant), __longlong_as_double((long long)(1023 + sh) << 52));      // both exact
    }
    const double S1 = __ull2double_rn(sS1);
    const double mu = __ddiv_rn(S1, (double)np);
    double var = __ddiv_rn(__dsub_rn(S2, __dmul_rn(mu, S1)), (double)(np - 1));
    var = var > 0.0 ? var : 0.0;
    const double thr = __dadd_rn(mu, __dmul_rn((double)ratio, __dsqrt_rn(var)));
    int stay = 0;
    for (long long i = tid; i < n; i += kStatThreads) {
        const float v = m[i];
        const bool in = (unsigned)__float_as_int(v) < kInfBits && (double)quant(v) <= thr;
        K[i] = in ? 1 : 0;
        stay += (int)in;
    }
    atomicAdd(&sKept, stay);
    __syncthreads();
    if (tid == 0) kept[s] = sKept;
}

template <bool MEAN>
int launch_grid(int S, const float* points, const long long* offsets, const float* queries, const long long* qoffsets, int k,
                int exclude_self, const float* cell, int* index, float* dist2, float* mean_dist, float* grid, char* ws,
                long long ws_bytes, hipStream_t stream) {
    const bool cross = queries != nullptr && queries != points;
    const long long* qo = cross ? qoffsets : nullptr;
    hipLaunchKernelGGL(grid_setup_kernel, dim3(S), dim3(kSetupThreads), 0, stream, S, points, offsets, qo, cell, k, ws, ws_bytes, grid);
    hipLaunchKernelGGL((grid_bin_kernel<false>), dim3(kBinGrid), dim3(kBinThreads), 0, stream, S, points, offsets, offsets, qo, 0,
                       cross ? 0 : 1, k, index, dist2, mean_dist, ws, ws_bytes);
    if (cross)
        hipLaunchKernelGGL((grid_bin_kernel<false>), dim3(kBinGrid), dim3(kBinThreads), 0, stream, S, queries, qoffsets, offsets, qo,
                           1, 1, k, index, dist2, mean_dist, ws, ws_bytes);
    hipLaunchKernelGGL(grid_prefix_kernel, dim3(S, cross ? 2 : 1), dim3(1024), 0, stream, S, offsets, qo, ws, ws_bytes);
    hipLaunchKernelGGL((grid_bin_kernel<true>), dim3(kBinGrid), dim3(kBinThreads), 0, stream, S, points, offsets, offsets, qo, 0, 0,
                       k, index, dist2, mean_dist, ws, ws_bytes);
    if (cross)
        hipLaunchKernelGGL((grid_bin_kernel<true>), dim3(kBinGrid), dim3(kBinThreads), 0, stream, S, queries, qoffsets, offsets, qo, 1,
                           0, k, index, dist2, mean_dist, ws, ws_bytes);
#define HP_KNN_GRID_CASE(KK)                                                                                                  \
    if (k <= KK) {                                                                                                            \
        hipLaunchKernelGGL((grid_sweep_kernel<KK, MEAN>), dim3(kSweepGrid), dim3(64), 0, stream, S, offsets, qo, k, exclude_self, \
                           index, dist2, mean_dist, ws, ws_bytes);                                                            \
        HP_RETURN_LAST_ERROR();                                                                                               \
    }
    HP_KNN_GRID_CASE(8)
    HP_KNN_GRID_CASE(16)
    HP_KNN_GRID_CASE(32)
#undef HP_KNN_GRID_CASE
    return -1;
}

}  // namespace

// Bytes of workspace hp_knn_grid needs for S scans of T rows in all and a second query set of Q rows (Q <= 0: none).  Host only.
HP_API long long hp_knn_grid_workspace_bytes(int S, long long T, long long Q) {
    if (S < 1 || T < 0 || T > (1LL << 36) || Q > (1LL << 36)) return -1;
    return layout(S, T, Q).need;
}

// The instance hp_knn_grid launches for k: its compile-time list length, threads per workgroup (one wave = the queries of a
// block of cells) and candidates per LDS tile.  Host only.
HP_API int hp_knn_grid_plan(int k, int* instance_k, int* threads, int* tile) {
    HP_CHECK_ARG(k >= 1 && k <= hp_knn::kMaxK && instance_k && threads && tile);
    *instance_k = k <= 8 ? 8 : k <= 16 ? 16 : 32;
    *threads = 64;
    *tile = kTile;
    return 0;
}

// hp_knn_points' result for scans of up to HP_KNN_GRID_MAX_POINTS rows: see the top and include/hyperpocket_hip.h.
HP_API int hp_knn_grid(int S, const float* points, const long long* offsets, const float* queries, const long long* query_offsets,
                       int k, int exclude_self, const float* cell, int* index, float* dist2, float* mean_dist, float* grid,
                       void* ws, long long ws_bytes, hipStream_t stream) {
    HP_CHECK_ARG(S >= 1 && k >= 1 && k <= hp_knn::kMaxK && (exclude_self == 0 || exclude_self == 1));
    HP_CHECK_ARG(points && offsets && ws && ws_bytes > 0);
    HP_CHECK_ARG((index != nullptr) == (dist2 != nullptr) && (index != nullptr) != (mean_dist != nullptr));   // lists, or m_i
    HP_CHECK_ARG((queries == nullptr) == (query_offsets == nullptr));
    const bool own = queries == nullptr || queries == points;
    HP_CHECK_ARG(!own || exclude_self == 1);               // a scan queried with itself: every row would find itself first
    HP_CHECK_ARG(((uintptr_t)ws & 15) == 0);
    if (mean_dist)
        return launch_grid<true>(S, points, offsets, queries, query_offsets, k, exclude_self, cell, nullptr, nullptr, mean_dist, grid,
                                 (char*)ws, ws_bytes, stream);
    return launch_grid<false>(S, points, offsets, queries, query_offsets, k, exclude_self, cell, index, dist2, nullptr, grid, (char*)ws,
                              ws_bytes, stream);
}

// keep / kept from given m_i by the statistics law, scans of up to HP_KNN_GRID_MAX_POINTS rows.
HP_API int hp_outlier_keep(int S, const float* mean_dist, const long long* offsets, float ratio, unsigned char* keep, int* kept,
                           hipStream_t stream) {
    HP_CHECK_ARG(S >= 1 && ratio >= 0.f && ratio <= 3.0e38f);
    HP_CHECK_ARG(mean_dist && offsets && keep && kept);
    hipLaunchKernelGGL(outlier_keep_kernel, dim3(S), dim3(kStatThreads), 0, stream, mean_dist, offsets, ratio, keep, kept);
    HP_RETURN_LAST_ERROR();
}

// Statistical outlier removal of S ragged scans of up to HP_KNN_GRID_MAX_POINTS rows: hp_scan_outliers' result.
HP_API int hp_scan_outliers_grid(int S, const float* points, const long long* offsets, int k, float ratio, const float* cell,
                                 unsigned char* keep, float* mean_dist, int* kept, void* ws, long long ws_bytes, hipStream_t stream) {
    HP_CHECK_ARG(S >= 1 && k >= 1 && k <= hp_knn::kMaxK && ratio >= 0.f && ratio <= 3.0e38f);
    HP_CHECK_ARG(points && offsets && keep && mean_dist && kept && ws && ws_bytes > 0 && ((uintptr_t)ws & 15) == 0);
    const int rc = launch_grid<true>(S, points, offsets, nullptr, nullptr, k, 1, cell, nullptr, nullptr, mean_dist, nullptr, (char*)ws,
                                     ws_bytes, stream);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(outlier_keep_kernel, dim3(S), dim3(kStatThreads), 0, stream, mean_dist, offsets, ratio, keep, kept);
    HP_RETURN_LAST_ERROR();
}
