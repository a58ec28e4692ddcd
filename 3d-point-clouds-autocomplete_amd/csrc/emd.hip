// Approximate earth-mover matching for gfx950 (replaces approxmatch.cu:34-213 + the match-based
// cost/gradient kernels :215-322 of the reference's utils/pytorch_structural_losses/).
//
// Algorithm: 9 annealing levels, each with three globally dependent phases.  What this file holds:
//   * RECORDS.  Every phase is a chip-wide launch over (cloud, row block); one lane owns one row point and sweeps ALL candidates of
//     the other set.  Candidates are wave-uniform, so they travel on the SCALAR path: packed records (xyz + weights) are fetched with
//     s_load_dwordx8/x16 and used as SGPR operands of the VALU ops — no LDS tile, no barrier, no candidate VGPRs.  They are stored as
//     PAIR records ([x0 x1 | y0 y1 | z0 z1 | w0 w1 ...]) so that the arithmetic of two candidates runs on packed fp32 VALU ops
//     (v_pk_add/mul/fma_f32 with an SGPR pair as one operand); padding records carry zero weights and contribute exact zeros.  Each
//     element still sees the reference's operation sequence as nvcc's default -fmad=true contracts it (distance fma chain, products
//     entering the running sums through an fma, ascending candidate order in the accumulators): the C oracle's `contract` variant 3.
//     Only ~2 waves per SIMD exist, so the SMEM latency is hidden by an explicit two-stage software pipeline: the next stage's
//     s_loads are issued (inline asm, pinned with sched_barrier) before the VALU work on the current stage, and waited for after it.
//     The records of a call are written by ONE writer (write_pair_records), from emd_init_kernel in the caller's point order or
//     from emd_order_kernel in Hilbert order.
//   * THE THREE SWEEP FAMILIES.  Set1-row sweeps (emd_rows1_kernel: phase 3 of level j and phase 1 of level j+1 own the same rows and
//     candidates, so they are ONE launch — distance evaluated once, two exponentials: 19 launches instead of 27; rows1_setup /
//     rows1_finish), set2-row sweeps (emd_rows2_kernel: phase 2; rows2_setup / rows2_finish), and the final sweeps over the "final"
//     records that keep every level's ratioL / ratioR: `match` (API) is produced by one pass that re-evaluates the nine
//     exponentials per pair in level order (emd_match_kernel) — or never: the fused cost / gradient kernels (emd_cost_grad1_kernel,
//     emd_grad2_kernel) consume the records directly, so the (b,m,n) tensor disappears from the training step; they derive four of
//     the nine exponentials as fourth powers of their neighbours (match_entry2; only there — nothing is downstream of those values).
//     The plain kernels are templates over their rows per lane (with_rows picks the instance).
//   * CULLING.  With the records in Hilbert order the sweeps of the first `cull` levels skip the (64-row tile, 8-candidate block)
//     units whose exponentials all underflow to exactly +0 (emd_rows1_cull_kernel, emd_rows2_cull_kernel; one row per lane), and
//     the final gradient sweep leaves those levels' terms out.
//   * COMPACTION.  Set2 points whose remainR is clamped to exactly +0 add only exact zeros from then on: behind each plain level's
//     phase-2 launch emd_compact_kernel lists the live ones and compacts the next launches' rows and candidates, class by class in
//     the full sweep's order, so every sum keeps its bits (the COMPACT instances of the plain kernels; hp_emd_set_compact(1)).
//     FUSED (hp_emd_set_compact(2), the default where MP <= 4096): no compaction launch — each phase-2 launch leaves its live rows
//     in its own segment of the row list and each row's record in a slot fixed by the list the launch started from, and the next
//     phase-2 launch scans that list in its prologue (fused_scan, rows2_finish<R, FUSED>): nothing passes between workgroups.
//     Round 12, the list-driven phase-2 launches (emd_rows2_kernel MODE 1 / 2).  PLACEMENT: a list is dense, so with the row tile in
//     blockIdx.x the live workgroups of every cloud sat on the same few XCDs and the launch took 54-60 us at any row count; they take
//     the cloud from x and the tile from y, one row per lane, and follow their work (45 .. 15 us).  THE ONE EXCEPTION TO THE SCALAR
//     PATH: spread like that they are one wave per SIMD or less, too few to cover a scalar load's round trip, so their workgroups
//     stage the cloud's set1 records in LDS once and the waves read them from there as broadcasts (FEED 1, hp_emd_set_rows2_feed; sets
//     of up to kFeedMaxNP points): the same operations in the same order on VGPR operands, bit-identical.
//   * CHAINS.  The clouds are independent but a launch is not: hp_emd_forward* runs the level sweeps as TWO chains of half the
//     clouds on two streams, enqueued alternately, and one chain's waves cover the other's launch boundaries (LevelChain,
//     emd_forward_impl); the final sweep is one launch over all clouds behind both (emd_final_sweep).
//   * WAVE PRIORITY (round 13).  The kernels of hp_emd_forward* / hp_emd_pairs raise their waves' priority with one s_setprio
//     (emd_wave_prio, HP_EMD_WAVE_PRIO): a caller's older kernel on another stream no longer takes the vector pipes from them.
//   * THE WORKSPACE-FREE PATH.  hp_approxmatch keeps the reference's prototype and data flow (emd_plain_*_kernel): no records.
// How the file came to be, round by round: docs/DESIGN_HISTORY.md.
#include "hp_common.h"
#include <algorithm>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

// (Round 3's derived-exponential experiment — e(j) = e(j+1)^4, -0.08 ms per step, fails the parity bars — lives as a patch in
// tools/micro/emd_derive.patch, not in the shipped library: docs/DESIGN_HISTORY.md 7b.)

namespace {

#ifndef HP_EMD_PARTS
#define HP_EMD_PARTS 4
#endif
// Round 13: the user priority (s_setprio, 0..3) of every wave of the kernels hp_emd_forward* and hp_emd_pairs launch.  VALU issue on
// a SIMD is arbitrated by priority, then by age, and every level launch brings young waves: beside an older resident kernel of
// another stream (the training step's Chamfer forward: 512 workgroups, vector-issue-bound, ~94 us) they got the leftover slots.
// The sweeps are the critical chain and leave most issue slots idle, so their waves go first.  0: no instruction (rounds 1-12);
// 1, 2 and 3 measured alike (profiles/r13_bench_ab.md).
#ifndef HP_EMD_WAVE_PRIO
#define HP_EMD_WAVE_PRIO 1
#endif
// Each of those kernels passes a workgroup id it needs at once (its cloud index; emd_rows2_cull_kernel its row tile) through the
// instruction as the tied operand of a plain asm.  __builtin_amdgcn_s_setprio and `asm volatile` count as writers of memory:
// behind either, the compiler no longer proves the kernels' uniform loads unclobbered and turns them into vector loads (26 of
// the 55 kernels changed registers, spills or loop code).  The tied form is ordered by data flow alone and adds nothing else
// (profiles/r13_emd_isa_compare.md).  Not in emd_grad2_kernel: with 40-61 spilled SGPRs every placement tried moved spill code
// inside its loop, and the final sweep runs behind the join with `after`, with nothing beside it to outrank.
__device__ __forceinline__ unsigned emd_wave_prio(unsigned wg_id) {
#if HP_EMD_WAVE_PRIO
    asm("s_setprio %1" : "+s"(wg_id) : "n"(HP_EMD_WAVE_PRIO));
#endif
    return wg_id;
}
constexpr int kThreads = 64 * HP_EMD_PARTS;   // one wave per candidate range, 64 rows per workgroup
constexpr int kLevels = 9;
constexpr int kStage = 8;   // candidates per software-pipeline stage of the phase kernels (= 4 pair records)
constexpr int kSpare = 8;   // readable zero candidates past the padded range (the prefetch after the last stage)
constexpr float kLog2e = 1.4426950408889634f;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
using hp::f2, hp::splat2, hp::sqdist2;   // a candidate pair to the lane's point, per element hp::sqdist's chain

// Scalar-memory loads the compiler must neither wait for early nor sink (cdna_hip_programming.md §5.7):
// issue -> sched_barrier -> VALU work on the other stage -> one s_waitcnt that names every destination.
#define HP_SLOAD16(dst, ptr, off) asm volatile("s_load_dwordx16 %0, %1, " #off : "=s"(dst) : "s"(ptr) : "memory")
#define HP_SLOAD8(dst, ptr, off) asm volatile("s_load_dwordx8 %0, %1, " #off : "=s"(dst) : "s"(ptr) : "memory")
#define HP_PIN() __builtin_amdgcn_sched_barrier(0)

__host__ __device__ constexpr float level_l2e(int lev) {
    // level = -4^j, j = 7..-1 (approxmatch.cu:55-56), pre-multiplied by log2(e); powers of 4 scale exactly
    return (lev == 0 ? -16384.f : lev == 1 ? -4096.f : lev == 2 ? -1024.f : lev == 3 ? -256.f : lev == 4 ? -64.f
            : lev == 5 ? -16.f : lev == 6 ? -4.f : lev == 7 ? -1.f : -0.25f) * kLog2e;
}
// largest squared distance whose exponential at `lev` is not exactly zero (exp2 of less than -152 is +0 in fp32, denormals
// included; the margin over -150 covers the rounding of the box test and of the kernels' own distance)
__host__ __device__ constexpr float underflow_r2(int lev) { return 152.f / -level_l2e(lev); }

// Only B*N row points exist (2 waves per SIMD at B=64, N=2048): to fill the SIMDs each row's candidate sweep is cut
// into kParts contiguous ranges handled by different waves of the workgroup and added in range order through LDS
// (ordered, deterministic; a reordering of the reference's sequential sum that moves the cost by ~1e-7 relative —
// measured on the oracle — against 1e-5 for the exp formulation).
constexpr int kParts = HP_EMD_PARTS;
constexpr int kRowsPerWg = kThreads / kParts;
inline int pad_up(int x) { return (x + 2 * kStage * kParts - 1) / (2 * kStage * kParts) * (2 * kStage * kParts); }

// per-cloud workspace (floats), every candidate array padded to NP/MP (+kSpare) entries:
//   PLP  pair records of set1 for phase 2:        8 floats per PAIR  [x0 x1 y0 y1 z0 z1 ratioL0 ratioL1]
//   PRP  pair records of set2 for phases 1/3:     8 floats per PAIR  [x0 x1 y0 y1 z0 z1 ratioR0 ratioR1]
//   RR   remainR per candidate of set2 (linear, so pairs are adjacent)
//   FLP / FRP  "final" pair records (32 floats per PAIR): [x0 x1 y0 y1 z0 z1 | r(lev0)0 r(lev0)1 | ... | r(lev8)0 r(lev8)1 | 8 pad]
struct WsLayout {
    int NP, MP;
    long plp, prp, rr, flp, frp, permL, permR, blkL, blkR, tileL, tileR, flag, per_cloud;
};
// Round 6 (ordered / culling sweeps): per set the Hilbert order (position -> original index, int32 in a float slot), the bounding
// boxes of its 8-candidate blocks (SoA: [minx | miny | minz | maxx | maxy | maxz] x NP/8) and of its 64-row tiles (x NP/64), and
// one flag block per cloud: flag[0] != 0: the records are in Hilbert order (0: the caller's order); then flag[1] / flag[2] = the
// final sweep's tier radii under the cull of the forward that wrote the records (emd_order_kernel).
constexpr int kBlk = 8;      // candidates per cull block = one software-pipeline stage of pair records
constexpr int kTile = 64;    // rows per cull tile = the rows one wave owns per row slot
inline WsLayout ws_layout(int n, int m) {
    WsLayout w;
    w.NP = pad_up(n);
    w.MP = pad_up(m);
    w.plp = 0;
    w.prp = w.plp + (long)(w.NP + kSpare) * 4;
    w.rr = w.prp + (long)(w.MP + kSpare) * 4;
    w.flp = w.rr + (long)(w.MP + kSpare);
    w.frp = w.flp + (long)(w.NP + kSpare) * 16;
    w.permL = w.frp + (long)(w.MP + kSpare) * 16;
    w.permR = w.permL + w.NP;
    w.blkL = w.permR + w.MP;
    w.blkR = w.blkL + 6L * (w.NP / kBlk);
    w.tileL = w.blkR + 6L * (w.MP / kBlk);
    w.tileR = w.tileL + 6L * (w.NP / kTile);
    w.flag = w.tileR + 6L * (w.MP / kTile);
    w.per_cloud = w.flag + 16;
    return w;
}

std::mutex g_s2_mu;                            // the library's second-chain stream per device (emd_forward_impl)
std::map<int, hipStream_t> g_s2_streams;
constexpr int kMaxChains = 4;
constexpr int kOrderMaxLog = 12;   // Hilbert order for sets of up to 4096 points (the order kernel's LDS: 19 bytes per point)
// The process-wide switches (hp_emd_set_*): hp_emd_forward* as two chains of half the clouds on two streams (2) or one chain (1);
// the records in Hilbert order and the first `cull` levels' sweeps culling (0: caller's order, no culling); the final cost /
// gradient sweep with derived exponentials (match_entry2<.., DERIVE>); forced rows per lane of the three sweep families (0 = the
// size heuristic).  A call reads them once, at its entry (EmdSwitches).
hp::Switch g_chains("HP_EMD_CHAINS", 2, 1, kMaxChains);
hp::Switch g_cull("HP_EMD_CULL", 3, 0, kLevels);
hp::Switch g_final_derive("HP_EMD_FINAL_DERIVE", 1);
hp::Switch g_rows1("HP_EMD_ROWS1_R", 0, 0, 4), g_rows2("HP_EMD_ROWS2_R", 0, 0, 4), g_grad2("HP_EMD_GRAD2_R", 0, 0, 2);
// the plain level sweeps over the set2 points still alive: 0 = every point, 1 = emd_compact_kernel behind each phase-2 launch, 2 = fused
// (the phase-2 launches list and place the points themselves: fused_scan; where it does not apply a call runs as 1)
hp::Switch g_compact("HP_EMD_COMPACT", 2, 0, 2);
// how the candidates reach the waves of the list-driven phase-2 sweeps: 0 = the scalar path, 1 = staged in LDS (emd_rows2_kernel, FEED)
hp::Switch g_rows2_feed("HP_EMD_ROWS2_FEED", 1);
struct EmdSwitches {
    int chains, cull, rows1, rows2, grad2;
    bool derive;
    int compact, rows2_feed;
};
EmdSwitches read_switches() {
    return {g_chains.get(), g_cull.get(), g_rows1.get(), g_rows2.get(), g_grad2.get(), g_final_derive.get() != 0, g_compact.get(),
            g_rows2_feed.get()};
}

// Round 7: the compaction scratch of a cloud (floats), in `partials` behind the cost partials (hp_emd_partials_floats):
//   REC / W   the phase-3 / phase-1 candidates of the next merged launch, compacted per class (see emd_compact_kernel): pair records
//             as PRP and remainR as RR, (MP + kSpare) candidate slots
//   LIST0/1   the set2 points alive on entry to a level (int32 in float slots, ascending), ping-pong between consecutive levels
//   CNT       [0] / [1]: the lengths of LIST0 / LIST1; [4 + part]: the merged launch's loop iterations of each candidate range
// The fused compaction (round 9, fused_scan) keeps the layout; its lists are MP entries in per-workgroup segments, live points first and
// -1 behind them, and it has no use for CNT[0] / [1].
struct CsLayout {
    long rec, w, list0, list1, cnt, per_cloud;
};
inline long align16(long x) { return (x + 15) / 16 * 16; }      // 64-byte boundaries for the scalar loads of the records
inline CsLayout cs_layout(int m) {
    const int MP = pad_up(m);
    CsLayout s;
    s.rec = 0;
    s.w = align16(s.rec + (long)(MP + kSpare) * 4);
    s.list0 = align16(s.w + MP + kSpare);
    s.list1 = align16(s.list0 + MP);
    s.cnt = align16(s.list1 + MP);
    s.per_cloud = align16(s.cnt + 16);
    return s;
}
inline long cost_partials_floats(int b, int n, int m) { return align16((long)b * ((std::max(n, m) + kRowsPerWg - 1) / kRowsPerWg)); }

struct Ctx {
    int n, m, NP, MP;
    const float* xyz1;
    const float* xyz2;
    float* temp;  // (b, 2(n+m)) : [remainL n | remainR m | ratioL n | ratioR m]  (reference layout, approxmatch.cu:35)
    float* ws;
    int plp, prp, rr, flp, frp, permL, permR, blkL, blkR, tileL, tileR, flag;   // float offsets inside a cloud's workspace (< 2^31)
    long per_cloud;
    float acc_scale = 0.f;   // != 0: emd_grad2_kernel stores grad2[i] += acc_scale * d cost / d xyz2[i] instead of the plain gradient
    float* cs = nullptr;     // compaction scratch (CsLayout) of the chain's first cloud; offsets as for ws
    int cs_rec = 0, cs_w = 0, cs_list0 = 0, cs_list1 = 0, cs_cnt = 0, cs_per_cloud = 0;
};
// The pair form (hp_emd_pairs): cloud i of a call, or of a chain of it, is (xyz1[ab[2i]], xyz2[ab[2i+1]]) with xyz1 (na,n,3) and
// xyz2 (nb,m,3).  ab == NULL: the batched addressing, cloud i is (xyz1[i], xyz2[i]).  An argument of its own of the three kernels
// that read it — the two set-up kernels and the cost finish — and not a part of Ctx: every sweep takes Ctx by value, and a Ctx of
// another size moves their register allocation (SGPR spills of the fused phase-2 instances) for nothing they use.
struct PairList {
    const int* ab = nullptr;
    int na = 0, nb = 0;
};
inline Ctx make_ctx(int n, int m, const float* xyz1, const float* xyz2, float* temp, float* ws) {
    const WsLayout L = ws_layout(n, m);
    Ctx c;
    c.n = n; c.m = m; c.NP = L.NP; c.MP = L.MP;
    c.xyz1 = xyz1; c.xyz2 = xyz2; c.temp = temp; c.ws = ws;
    c.plp = (int)L.plp; c.prp = (int)L.prp; c.rr = (int)L.rr; c.flp = (int)L.flp; c.frp = (int)L.frp;
    c.permL = (int)L.permL; c.permR = (int)L.permR; c.blkL = (int)L.blkL; c.blkR = (int)L.blkR; c.tileL = (int)L.tileL; c.tileR = (int)L.tileR;
    c.flag = (int)L.flag; c.per_cloud = L.per_cloud;
    c.acc_scale = 0.f;
    return c;
}
// ... and the offsets of the compaction scratch (`cs`: that of the first cloud `c` covers)
inline void set_compact_scratch(Ctx& c, float* cs) {
    const CsLayout S = cs_layout(c.m);
    c.cs = cs;
    c.cs_rec = (int)S.rec; c.cs_w = (int)S.w; c.cs_list0 = (int)S.list0; c.cs_list1 = (int)S.list1; c.cs_cnt = (int)S.cnt;
    c.cs_per_cloud = (int)S.per_cloud;
}

// the initial remainL / remainR of every point (approxmatch.cu:37-43; integer division)
inline void multi_lr(int n, int m, float* multiL, float* multiR) {
    *multiL = n >= m ? 1.f : (float)(m / n);
    *multiR = n >= m ? (float)(n / m) : 1.f;
}
// "fills the chip": `clouds` clouds of `rows` row points at r rows per lane still put two waves on every SIMD
inline bool fills_chip(long clouds, int rows, int r) { return clouds * ((rows + r * kRowsPerWg - 1) / (r * kRowsPerWg)) * (kThreads / 64) >= 2048; }
// The launch helper of the sweeps that are templates over their rows per lane: calls f with `rows` (1, 2, or 4 where MAX allows it) as a
// compile-time constant, f(std::integral_constant<int, R>).
template <int MAX = 4, class F>
void with_rows(int rows, F f) {
    if constexpr (MAX >= 4) {
        if (rows == 4) return f(std::integral_constant<int, 4>{});
    }
    if (rows == 2) return f(std::integral_constant<int, 2>{});
    f(std::integral_constant<int, 1>{});
}

// element offsets of candidate i inside the pair-record arrays
__device__ __forceinline__ long pair8(int i, int comp) { return (long)(i >> 1) * 8 + comp * 2 + (i & 1); }            // comp 0..3 = x,y,z,w
__device__ __forceinline__ long pair32(int i, int comp) { return (long)(i >> 1) * 32 + comp * 2 + (i & 1); }          // comp 0..2 = x,y,z ; 3+lev = ratio

// The record writer: everything a call's set-up leaves for pair `pr` (points j0 = 2 pr and j0 + 1) of one set — the 8-float sweep
// record and the 32-float final record as 16-byte stores (the first version wrote 20 scattered dwords per point: 17 us for 26 MB),
// remainL / remainR in `temp`, and RR for set2.  The caller supplies the two points (zeros past the set's count).
__device__ __forceinline__ void write_pair_records(const Ctx& c, float* ws, float* remL, float* remR, bool left, int pr, int cnt, float x0, float y0,
                                                   float z0, float x1, float y1, float z1, float multiL, float multiR) {
    const int j0 = 2 * pr, j1 = j0 + 1;
    const bool ok0 = j0 < cnt, ok1 = j1 < cnt;
    float4* p8 = reinterpret_cast<float4*>(ws + (left ? c.plp : c.prp) + (long)pr * 8);
    float4* p32 = reinterpret_cast<float4*>(ws + (left ? c.flp : c.frp) + (long)pr * 32);
    const float4 a = make_float4(x0, x1, y0, y1), b = make_float4(z0, z1, 0.f, 0.f), zero = make_float4(0.f, 0.f, 0.f, 0.f);
    p8[0] = a;
    p8[1] = b;
    p32[0] = a;
    p32[1] = b;
#pragma unroll
    for (int q = 2; q < 8; ++q) p32[q] = zero;
    if (left) {
        if (ok0) remL[j0] = multiL;
        if (ok1) remL[j1] = multiL;
    } else {
        *reinterpret_cast<float2*>(ws + c.rr + j0) = make_float2(ok0 ? multiR : 0.f, ok1 ? multiR : 0.f);
        if (ok0) remR[j0] = multiR;
        if (ok1) remR[j1] = multiR;
    }
}

// The points of one set of cloud `cloud` as the caller handed them: the set-up kernels' only reads of xyz1 / xyz2.  In the pair form an
// index outside its set is clamped into it (nothing is read out of bounds; emd_cost_finish_kernel writes that pair's cost as NaN).
__device__ __forceinline__ const float* cloud_points(const Ctx& c, const PairList& pl, int cloud, bool left) {
    long idx = cloud;
    if (pl.ab) idx = min(max(pl.ab[2 * (long)cloud + (left ? 0 : 1)], 0), (left ? pl.na : pl.nb) - 1);
    return left ? c.xyz1 + idx * c.n * 3 : c.xyz2 + idx * c.m * 3;
}

// The set-up in the caller's point order: one thread per PAIR of points.
__global__ __launch_bounds__(256) void emd_init_kernel(Ctx c, float multiL, float multiR, PairList pl) {
    const int cloud = emd_wave_prio(blockIdx.y);
    float* ws = c.ws + (long)cloud * c.per_cloud;
    float* remL = c.temp + (long)cloud * (c.n + c.m) * 2;
    float* remR = remL + c.n;
    const float* P = cloud_points(c, pl, cloud, true);
    const float* Q = cloud_points(c, pl, cloud, false);
    const int NPp = (c.NP + kSpare) / 2, MPp = (c.MP + kSpare) / 2;   // pairs per set (NP, MP, kSpare are even)
    if (blockIdx.x == 0 && threadIdx.x == 0) ws[c.flag] = 0.f;        // records in the caller's point order (see emd_order_kernel)
    for (int i = blockIdx.x * 256 + threadIdx.x; i < NPp + MPp; i += gridDim.x * 256) {
        const bool left = i < NPp;
        const int pr = left ? i : i - NPp, j0 = 2 * pr, j1 = j0 + 1;
        const int cnt = left ? c.n : c.m;
        const float* src = left ? P : Q;
        const bool ok0 = j0 < cnt, ok1 = j1 < cnt;
        const float x0 = ok0 ? src[j0 * 3] : 0.f, y0 = ok0 ? src[j0 * 3 + 1] : 0.f, z0 = ok0 ? src[j0 * 3 + 2] : 0.f;
        const float x1 = ok1 ? src[j1 * 3] : 0.f, y1 = ok1 ? src[j1 * 3 + 1] : 0.f, z1 = ok1 ? src[j1 * 3 + 2] : 0.f;
        write_pair_records(c, ws, remL, remR, left, pr, cnt, x0, y0, z0, x1, y1, z1, multiL, multiR);
    }
}

// ------------------------------------------------------------------------------------------------
// Round 6: the records in HILBERT ORDER, so that the level sweeps can skip work that is exactly zero.
// At level -16384 / -4096 / -1024 / -256 the exponential of a pair further apart than 0.080 / 0.160 / 0.321 / 0.641 underflows to
// exactly +0 (exp2 of less than -152): its terms are exact zeros in every phase (approxmatch.cu:86-87,131-132,185-189) and a sweep
// that leaves them out produces the same sums.  Skipping is only possible for whole (wave, pipeline stage) units, so both sets are
// put in an order in which 64 consecutive rows and 8 consecutive candidates are spatially compact: along the Hilbert curve of a
// 16^3 grid over the set's bounding box — consecutive cells of that curve are always neighbours, so ANY run of consecutive points
// is compact, not only the aligned ones (Morton order jumps).  Decidable from the bounding boxes of a (64-row tile, 8-candidate
// block) unit at the first four levels, uniform clouds: 80 / 70 / 47 / 6 % of the units (Morton 69 / 59 / 33 / 3 %; a k-d order —
// median splits, 85 / 76 / 54 / 10 % — needs eight segment sorts instead of one and costs more than it saves:
// tools/study/emd_cull_hilbert.py).  The algorithm is indifferent to the order of either set; a sweep in another
// order is another summation order of the same sums (oracle on re-ordered inputs: cost within 3e-7,
// tools/study/emd_order_sensitivity.py), and the gradient sweeps write through the permutation, so callers see their own order.
//
// One workgroup per (cloud, set): a counting sort by Hilbert cell in LDS (histogram, scan, scatter; the points of a cell in index
// order, so the order is a pure function of the input).  Then the same workgroup writes everything emd_init_kernel writes, in the
// new order, plus the permutation and the block / tile bounding boxes.
// ------------------------------------------------------------------------------------------------
constexpr int kOrderThreads = 1024;   // 16 waves for the load / key / output phases; the sort network runs on the first P2/8 threads
constexpr float kFar = 1e18f;     // an empty box: min = +kFar, max = -kFar (its gap to anything squares to 1e36 > any radius)

// Hilbert index of the cell (x, y, z), `bits` bits per axis (Skilling's transpose form, then interleaved: 3 * bits bits)
__device__ __forceinline__ uint32_t spread3(uint32_t v) {      // bit b -> bit 3b (b < 10)
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
__device__ __forceinline__ uint32_t hilbert3(uint32_t x0, uint32_t x1, uint32_t x2, int bits) {
    const uint32_t M = 1u << (bits - 1);
    for (uint32_t Q = M; Q > 1; Q >>= 1) {
        const uint32_t P = Q - 1;
        if (x0 & Q) x0 ^= P;
        if (x1 & Q) x0 ^= P;
        else {
            const uint32_t t = (x0 ^ x1) & P;
            x0 ^= t;
            x1 ^= t;
        }
        if (x2 & Q) x0 ^= P;
        else {
            const uint32_t t = (x0 ^ x2) & P;
            x0 ^= t;
            x2 ^= t;
        }
    }
    x1 ^= x0;
    x2 ^= x1;
    uint32_t t = 0;
    for (uint32_t Q = M; Q > 1; Q >>= 1)
        if (x2 & Q) t ^= Q - 1;
    x0 ^= t;
    x1 ^= t;
    x2 ^= t;
    return (spread3(x0) << 2) | (spread3(x1) << 1) | spread3(x2);
}
constexpr int kHilbertBits = 4;                        // 16^3 cells: finer grids do not make 8-point runs more compact (emd_cull_hilbert.py)
constexpr int kCells = 1 << (3 * kHilbertBits);

__global__ __launch_bounds__(kOrderThreads) void emd_order_kernel(Ctx c, float multiL, float multiR, int logpL, int logpR, int cull, PairList pl) {
    extern __shared__ float smem[];
    __shared__ float red[6][kOrderThreads / 64];
    __shared__ float gb[3], gscale[3];
    __shared__ uint32_t wsum[kOrderThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const bool left = blockIdx.x == 0;
    const int cloud = emd_wave_prio(blockIdx.y);
    const int cnt = left ? c.n : c.m, NPx = left ? c.NP : c.MP, logp = left ? logpL : logpR, P2 = 1 << logp;
    const float* src = cloud_points(c, pl, cloud, left);
    float* ws = c.ws + (long)cloud * c.per_cloud;
    float* X = smem;
    float* Y = X + P2;
    float* Z = Y + P2;
    uint32_t* hist = reinterpret_cast<uint32_t*>(Z + P2);            // per cell: count -> start -> end of its slot range
    uint16_t* cell = reinterpret_cast<uint16_t*>(hist + kCells);     // per point
    uint16_t* tmp = cell + P2;                                       // slot -> point, arrival order inside a cell
    uint16_t* key = tmp + P2;                                        // position -> point (the order)
    float* box0 = reinterpret_cast<float*>(hist);   // NP/8 block boxes [lo xyz | hi xyz] (the output phase; the histogram is dead by then)

    // the points and their bounding box
    float mn[3] = {kFar, kFar, kFar}, mx[3] = {-kFar, -kFar, -kFar};
    for (int i = tid; i < P2; i += kOrderThreads) {
        float x = 0.f, y = 0.f, z = 0.f;
        if (i < cnt) {
            x = src[i * 3];
            y = src[i * 3 + 1];
            z = src[i * 3 + 2];
            mn[0] = fminf(mn[0], x); mx[0] = fmaxf(mx[0], x);
            mn[1] = fminf(mn[1], y); mx[1] = fmaxf(mx[1], y);
            mn[2] = fminf(mn[2], z); mx[2] = fmaxf(mx[2], z);
        }
        X[i] = x;
        Y[i] = y;
        Z[i] = z;
        key[i] = (uint16_t)i;                       // positions past the count keep the identity
    }
    for (int q = tid; q < kCells; q += kOrderThreads) hist[q] = 0u;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn[a] = fminf(mn[a], __shfl_xor(mn[a], o, 64));
            mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o, 64));
        }
        if (lane == 0) {
            red[a][wid] = mn[a];
            red[3 + a][wid] = mx[a];
        }
    }
    __syncthreads();
    if (tid < 3) {
        float lo = red[tid][0], hi = red[3 + tid][0];
        for (int w = 1; w < kOrderThreads / 64; ++w) {
            lo = fminf(lo, red[tid][w]);
            hi = fmaxf(hi, red[3 + tid][w]);
        }
        gb[tid] = lo;
        gscale[tid] = hi > lo ? (float)(1 << kHilbertBits) * 0.9999f / (hi - lo) : 0.f;
    }
    __syncthreads();
    // A counting sort by Hilbert cell, points of a cell in index order (deterministic: the counts do not depend on the order
    // the atomics execute in, and the arrival order inside a cell is replaced by the index order below).
    for (int i = tid; i < cnt; i += kOrderThreads) {
        const uint32_t cm = (1u << kHilbertBits) - 1u;
        const uint32_t qx = min((uint32_t)((X[i] - gb[0]) * gscale[0]), cm), qy = min((uint32_t)((Y[i] - gb[1]) * gscale[1]), cm),
                       qz = min((uint32_t)((Z[i] - gb[2]) * gscale[2]), cm);
        const uint32_t h = hilbert3(qx, qy, qz, kHilbertBits);
        cell[i] = (uint16_t)h;
        atomicAdd(&hist[h], 1u);
    }
    __syncthreads();
    {   // exclusive scan of the cell counts: kCells / kOrderThreads consecutive cells per thread
        constexpr int kPer = kCells / kOrderThreads;
        uint32_t v[kPer], s = 0;
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            v[q] = hist[tid * kPer + q];
            s += v[q];
        }
        uint32_t inc = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (lane == 63) wsum[wid] = inc;
        __syncthreads();
        uint32_t base = 0;
        for (int w = 0; w < wid; ++w) base += wsum[w];
        uint32_t run = base + inc - s;
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            hist[tid * kPer + q] = run;
            run += v[q];
        }
    }
    __syncthreads();
    for (int i = tid; i < cnt; i += kOrderThreads) tmp[atomicAdd(&hist[cell[i]], 1u)] = (uint16_t)i;    // hist[h]: start -> end
    __syncthreads();
    for (int i = tid; i < cnt; i += kOrderThreads) {
        const uint32_t h = cell[i];
        const uint32_t s0 = h ? hist[h - 1] : 0u, s1 = hist[h];      // the cell's slots (the previous cell's end .. its own)
        uint32_t rank = 0;
        for (uint32_t q = s0; q < s1; ++q) rank += tmp[q] < (uint16_t)i ? 1u : 0u;
        key[s0 + rank] = (uint16_t)i;
    }
    __syncthreads();
    const uint32_t imask = 0xffffu;

    // ---- outputs: the permutation, what emd_init_kernel writes (in the new order), the boxes ----
    int* perm = reinterpret_cast<int*>(ws + (left ? c.permL : c.permR));
    for (int e = tid; e < NPx; e += kOrderThreads) perm[e] = (int)(key[e] & imask);
    float* remL = c.temp + (long)cloud * (c.n + c.m) * 2;
    float* remR = remL + c.n;
    const int pairs = (NPx + kSpare) / 2;
    for (int pr = tid; pr < pairs; pr += kOrderThreads) {
        const int j0 = 2 * pr, j1 = j0 + 1;
        const bool ok0 = j0 < cnt, ok1 = j1 < cnt;
        const uint32_t i0 = ok0 ? (key[j0] & imask) : 0u, i1 = ok1 ? (key[j1] & imask) : 0u;
        const float x0 = ok0 ? X[i0] : 0.f, y0 = ok0 ? Y[i0] : 0.f, z0 = ok0 ? Z[i0] : 0.f;
        const float x1 = ok1 ? X[i1] : 0.f, y1 = ok1 ? Y[i1] : 0.f, z1 = ok1 ? Z[i1] : 0.f;
        write_pair_records(c, ws, remL, remR, left, pr, cnt, x0, y0, z0, x1, y1, z1, multiL, multiR);
    }
    // bounding boxes of the 8-candidate blocks (exact, over the real points) ...
    const int NB = NPx / kBlk, NT = NPx / kTile;
    float* bb = ws + (left ? c.blkL : c.blkR);
    float* lb = box0;                                  // (both box tables are free now: NB * 6 floats = their size)
    for (int g = tid; g < NB; g += kOrderThreads) {
        float lo[3] = {kFar, kFar, kFar}, hi[3] = {-kFar, -kFar, -kFar};
        for (int j = g * kBlk; j < min(g * kBlk + kBlk, cnt); ++j) {
            const uint32_t i = key[j] & imask;
            lo[0] = fminf(lo[0], X[i]); hi[0] = fmaxf(hi[0], X[i]);
            lo[1] = fminf(lo[1], Y[i]); hi[1] = fmaxf(hi[1], Y[i]);
            lo[2] = fminf(lo[2], Z[i]); hi[2] = fmaxf(hi[2], Z[i]);
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            bb[q * NB + g] = lo[q];
            bb[(3 + q) * NB + g] = hi[q];
            lb[g * 6 + q] = lo[q];
            lb[g * 6 + 3 + q] = hi[q];
        }
    }
    __syncthreads();
    // ... and of the 64-row tiles
    float* tb = ws + (left ? c.tileL : c.tileR);
    for (int t = tid; t < NT; t += kOrderThreads) {
        float lo[3] = {kFar, kFar, kFar}, hi[3] = {-kFar, -kFar, -kFar};
        for (int g = t * (kTile / kBlk); g < (t + 1) * (kTile / kBlk); ++g) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                lo[q] = fminf(lo[q], lb[g * 6 + q]);
                hi[q] = fmaxf(hi[q], lb[g * 6 + 3 + q]);
            }
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            tb[q * NT + t] = lo[q];
            tb[(3 + q) * NT + t] = hi[q];
        }
    }
    if (left && tid == 0) {      // Hilbert order, and the underflow radii of levels 1 and 2 where they cull (3e38: that tier of
        ws[c.flag] = 1.f;            // emd_grad2_kernel is off)
        ws[c.flag + 1] = cull > 1 ? underflow_r2(1) : 3.0e38f;
        ws[c.flag + 2] = cull > 2 ? underflow_r2(2) : 3.0e38f;
    }
}

// pair record `u` (0..3) of a stage held in two x16 SGPR groups: component c (0=x,1=y,2=z,3=w) as a float2
// (indices are compile-time constants once the stage loop is unrolled; elements (2i, 2i+1) form an aligned SGPR pair)
#define PAIRC(lo, hi, u, c) \
    ((u) < 2 ? f2{(lo)[(u)*8 + (c)*2], (lo)[(u)*8 + (c)*2 + 1]} : f2{(hi)[((u)-2) * 8 + (c)*2], (hi)[((u)-2) * 8 + (c)*2 + 1]})

__device__ __forceinline__ f2 exp2_2(f2 a) { return f2{__builtin_amdgcn_exp2f(a.x), __builtin_amdgcn_exp2f(a.y)}; }

// Rows = set1.  DO3: phase 3 of level lev3 (remainL update, approxmatch.cu:161-194);
//               DO1: phase 1 of level lev1 (ratioL, :60-93).  Candidates: PRP (+RR) records on the scalar path.
// R rows per lane, as in emd_rows2_kernel.
//
// The set-up of one row of a set1-row sweep: point k of set1 out of its own record (the records are in the order the sweeps run
// in: emd_order_kernel), its ratioL (phase 3), and the two packed accumulators.
template <bool DO3>
__device__ __forceinline__ void rows1_setup(const Ctx& c, const float* ws, const float* ratioL, int k, int part, bool& ok, f2& px2, f2& py2, f2& pz2,
                                            f2& rl2, f2& acc3, f2& acc1) {
    ok = k < c.n;
    float px = 0.f, py = 0.f, pz = 0.f, rl = 0.f;
    if (ok) {
        px = ws[c.plp + pair8(k, 0)];
        py = ws[c.plp + pair8(k, 1)];
        pz = ws[c.plp + pair8(k, 2)];
        if (DO3) rl = ratioL[k];
    }
    px2 = splat2(px);
    py2 = splat2(py);
    pz2 = splat2(pz);
    rl2 = splat2(rl);
    // even / odd candidates accumulate in the two halves of a packed register (one v_pk_add_f32 per pair record
    // instead of two dependent v_add_f32); the halves are added once at the end, then the 4 candidate ranges in order
    acc3 = splat2(0.f);
    acc1 = f2{part == 0 ? 1e-9f : 0.f, 0.f};
}
// The end of a set1-row sweep, R rows per lane: the halves added, the candidate ranges added in range order through LDS, then the
// row's update: remainL (phase 3, approxmatch.cu:190-194) and ratioL (phase 1, :92-93) into `temp`, the sweep and the final record.
template <bool DO3, bool DO1, int R>
__device__ __forceinline__ void rows1_finish(const Ctx& c, float* ws, float* remL, float* ratioL, int lrow, int part, int lev1, const int* k,
                                             const bool* ok, const f2* acc3, const f2* acc1, float (&part3)[kParts][kRowsPerWg * R],
                                             float (&part1)[kParts][kRowsPerWg * R]) {
    float s3[R], s1[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        s3[r] = acc3[r].x + acc3[r].y;
        s1[r] = acc1[r].x + acc1[r].y;
        part3[part][r * kRowsPerWg + lrow] = s3[r];
        part1[part][r * kRowsPerWg + lrow] = s1[r];
    }
    __syncthreads();
    if (part != 0) return;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (!ok[r]) continue;
        float t3 = s3[r], t1 = s1[r];
#pragma unroll
        for (int q2 = 1; q2 < kParts; ++q2) {
            t3 += part3[q2][r * kRowsPerWg + lrow];
            t1 += part1[q2][r * kRowsPerWg + lrow];
        }
        float rem = remL[k[r]];
        if (DO3) {
            rem = fmaxf(0.0f, rem - t3);
            remL[k[r]] = rem;
        }
        if (DO1) {
            const float v = rem / t1;
            ratioL[k[r]] = v;
            ws[c.plp + pair8(k[r], 3)] = v;
            ws[c.flp + pair32(k[r], 3 + lev1)] = v;
        }
    }
}

// COMPACT (round 7): the candidates are the compacted records emd_compact_kernel left in the cloud's scratch — per candidate range
// only the set2 points that can add a non-zero term, each (range, parity) class in ascending order — and the range's wave walks its
// own iteration count (a wave-uniform value from the scratch) instead of the whole range.
template <bool DO3, bool DO1, int R, bool COMPACT = false>
__global__ __launch_bounds__(kThreads) void emd_rows1_kernel(Ctx c, int lev1, float l2e3, float l2e1) {
    __shared__ float part3[kParts][kRowsPerWg * R], part1[kParts][kRowsPerWg * R];
    const int cloud = emd_wave_prio(blockIdx.y);
    const int lrow = threadIdx.x % kRowsPerWg;
    const int part = __builtin_amdgcn_readfirstlane(threadIdx.x / kRowsPerWg);   // wave-uniform
    float* ws = c.ws + (long)cloud * c.per_cloud;
    float* remL = c.temp + (long)cloud * (c.n + c.m) * 2;
    float* ratioL = remL + c.n + c.m;
    int k[R];
    bool ok[R];
    f2 px2[R], py2[R], pz2[R], rl2[R], acc3[R], acc1[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        k[r] = (blockIdx.x * R + r) * kRowsPerWg + lrow;
        rows1_setup<DO3>(c, ws, ratioL, k[r], part, ok[r], px2[r], py2[r], pz2[r], rl2[r], acc3[r], acc1[r]);
    }
    const f2 l3 = splat2(l2e3), l1 = splat2(l2e1);
    const int cand = c.MP / kParts;                                  // candidates of this wave's range
    const float* cs = c.cs + (long)cloud * c.cs_per_cloud;
    const float* p = (COMPACT ? cs + c.cs_rec : ws + c.prp) + (long)part * cand * 4;   // wave-uniform
    const float* q = (COMPACT ? cs + c.cs_w : ws + c.rr) + (long)part * cand;
    // loop iterations (two pipeline stages each) of this wave's range
    const int iters = COMPACT ? __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(cs + c.cs_cnt)[4 + part]) : cand / (2 * kStage);
    f32x16 a0, a1, b0, b1;
    f32x8 w0 = {}, w1 = {};
    auto work = [&](const f32x16& lo, const f32x16& hi, const f32x8& w) {
#pragma unroll
        for (int u = 0; u < kStage / 2; ++u) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const f2 d = sqdist2(PAIRC(lo, hi, u, 0) - px2[r], PAIRC(lo, hi, u, 1) - py2[r], PAIRC(lo, hi, u, 2) - pz2[r]);
                // the running sums take their product through an fma — what nvcc's default -fmad=true makes of the
                // reference's `w=...; suml+=w` (approxmatch.cu:86-87,185-189); the oracle's `contract` variant 3
                if (DO3) {
                    acc3[r] = __builtin_elementwise_fma(exp2_2(l3 * d) * rl2[r], PAIRC(lo, hi, u, 3), acc3[r]);   // (e * ratioL[k]) * ratioR[l]
                }
                if (DO1) {
                    acc1[r] = __builtin_elementwise_fma(exp2_2(l1 * d), f2{w[u * 2], w[u * 2 + 1]}, acc1[r]);   // e * remainR[l]
                }
            }
        }
    };
    HP_SLOAD16(a0, p, 0x0);
    HP_SLOAD16(a1, p, 0x40);
    if (DO1) HP_SLOAD8(w0, q, 0x0);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a0), "+s"(a1), "+s"(w0));
    for (int it = 0; it < iters; ++it) {
        p += kStage * 4;
        q += kStage;
        HP_SLOAD16(b0, p, 0x0);
        HP_SLOAD16(b1, p, 0x40);
        if (DO1) HP_SLOAD8(w1, q, 0x0);
        HP_PIN();
        work(a0, a1, w0);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(b0), "+s"(b1), "+s"(w1), "+v"(acc3[0]), "+v"(acc1[0]), "+v"(acc3[R - 1]), "+v"(acc1[R - 1]));
        p += kStage * 4;
        q += kStage;
        HP_SLOAD16(a0, p, 0x0);      // past the last stage this reads the spare (zero) records
        HP_SLOAD16(a1, p, 0x40);
        if (DO1) HP_SLOAD8(w0, q, 0x0);
        HP_PIN();
        work(b0, b1, w1);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a0), "+s"(a1), "+s"(w0), "+v"(acc3[0]), "+v"(acc1[0]), "+v"(acc3[R - 1]), "+v"(acc1[R - 1]));
    }
    rows1_finish<DO3, DO1, R>(c, ws, remL, ratioL, lrow, part, lev1, k, ok, acc3, acc1, part3, part1);
}

// Rows = set2: phase 2 (ratioR / remainR update, approxmatch.cu:109-142).  Candidates: PLP records.
// R rows per lane (rows l and l + 64, ...): every candidate record fetched on the scalar path serves R rows, so a stage
// carries R times the VALU work behind its s_waitcnt (R independent accumulation chains per lane) at 1/R of the scalar
// traffic.  Per row the arithmetic and its order are those of R = 1.
//
// The set-up of one row of a set2-row sweep: point l of set2 out of its own record, and the packed accumulator (even / odd
// candidates, see rows1_setup).
__device__ __forceinline__ void rows2_setup(const Ctx& c, const float* ws, int l, bool ok, f2& qx2, f2& qy2, f2& qz2, f2& acc2) {
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (ok) {
        qx = ws[c.prp + pair8(l, 0)];
        qy = ws[c.prp + pair8(l, 1)];
        qz = ws[c.prp + pair8(l, 2)];
    }
    qx2 = splat2(qx);
    qy2 = splat2(qy);
    qz2 = splat2(qz);
    acc2 = splat2(0.f);
}
// What a phase-2 launch of the fused compaction (hp_emd_set_compact(2), see fused_scan) leaves for its successors, besides the
// update itself: `lout` the cloud's next row list, `seg` the workgroup's first slot in it; rec / wr the candidate slots of the next
// merged launch.  Not `produce` (the last level): the launch only consumed a list.
struct FusedOut {
    int* lout = nullptr;
    float* rec = nullptr;
    float* wr = nullptr;
    int seg = 0;
    bool produce = false;
};

// The end of a set2-row sweep, R rows per lane: the halves added, the candidate ranges added in range order through LDS, then THE
// phase-2 update of the row's point (approxmatch.cu:138-142) into `temp`, its sweep record, RR and its final record.
// FUSED (round 9) 1: the workgroup also lists its rows that stay alive (remainR != 0) in its own segment of `lout` — ascending, the
// rest of the segment -1 — and writes ratioR = +0 into `temp` for the rows that leave (what the full sweeps write there at every
// later level); 2: and each row writes its record and remainR into its slot sl of the next merged launch's candidates (sl < 0: the
// row was not alive on entry and has none).
template <int R, int FUSED = 0>
__device__ __forceinline__ void rows2_finish(const Ctx& c, float* ws, float* remR, float* ratioR, int lrow, int part, int lev, const int* l,
                                             const bool* ok, const f2* acc2, float (&parts)[kParts][kRowsPerWg * R], const FusedOut& fo = {},
                                             const int* sl = nullptr, const f2* qx2 = nullptr, const f2* qy2 = nullptr, const f2* qz2 = nullptr) {
    float acc[R];
    [[maybe_unused]] float vout[R], remout[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        acc[r] = acc2[r].x + acc2[r].y;
        parts[part][r * kRowsPerWg + lrow] = acc[r];
    }
    __syncthreads();
    if (part != 0) return;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (!ok[r]) continue;
        float a = acc[r];
#pragma unroll
        for (int q2 = 1; q2 < kParts; ++q2) a += parts[q2][r * kRowsPerWg + lrow];
        const float rr = remR[l[r]];
        const float sumr = a * rr;
        const float consumption = fminf(rr / (sumr + 1e-9f), 1.0f);
        const float v = consumption * rr;
        const float rem = fmaxf(0.0f, rr - sumr);
        ratioR[l[r]] = FUSED && fo.produce && rem == 0.f ? 0.f : v;
        remR[l[r]] = rem;
        ws[c.prp + pair8(l[r], 3)] = v;
        ws[c.rr + l[r]] = rem;
        ws[c.frp + pair32(l[r], 3 + lev)] = v;
        if (FUSED) {
            vout[r] = v;
            remout[r] = rem;
        }
    }
    if constexpr (FUSED != 0) {
        if (!fo.produce) return;
        const unsigned long long below = (1ull << lrow) - 1ull;      // (wave 0: lrow is the lane)
        int pos = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const bool live = ok[r] && remout[r] != 0.f;
            const unsigned long long bl = __ballot(live);
            if (live) fo.lout[fo.seg + pos + __popcll(bl & below)] = l[r];
            pos += __popcll(bl);
            if (FUSED == 2 && ok[r] && sl[r] >= 0) {
                const int s = sl[r];
                fo.rec[pair8(s, 0)] = qx2[r].x;
                fo.rec[pair8(s, 1)] = qy2[r].x;
                fo.rec[pair8(s, 2)] = qz2[r].x;
                fo.rec[pair8(s, 3)] = vout[r];
                fo.wr[s] = remout[r];
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = r * kRowsPerWg + lrow;
            if (i >= pos && fo.seg + i < c.MP) fo.lout[fo.seg + i] = -1;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Round 9: the FUSED compaction (hp_emd_set_compact(2)): what emd_compact_kernel computes, without its launch and without any hand-off
// between workgroups.  The candidates of the merged phase-3(j) / phase-1(j+1) launch may be any superset of kept_j = {ratioR_j != 0
// or remainR != 0} as long as each (range, parity) class keeps its ascending order — a point outside kept_j is a zero-weight record
// like the padding —, and L_j, the points alive on entry to level j, is such a superset known BEFORE phase 2 of level j runs.  So
//   * every phase-2 launch with a compacted successor leaves, per workgroup, the rows that stay alive in its own segment of the
//     cloud's list (rows2_finish<R, FUSED>): the segments in order are L_{j+1}, with -1 in the unused slots;
//   * every workgroup of the next phase-2 launch scans that list once (MP int32, L2-resident): the dense count (its grid is sized
//     from the shapes; workgroups past the count fill their segment with -1 and leave), its own rows and, per row, the rank in its
//     class, i.e. the slot sl = range * cand + 2 * rank + parity of emd_compact_kernel's layout, into which the row itself writes
//     its record and remainR when it finishes;
//   * workgroup 0 of the cloud writes the ranges' iteration counts (cnt[4 + part]) and the zero-weight records from each class's
//     count to the end of the padded range (fused_pad): slots no row writes.
// The scan: thread t owns 4 G consecutive list entries (G <= 4 int4 loads: MP <= 4096) and counts them per candidate range in two
// packed words (16 bits per range: all live entries / the odd ones); an inclusive scan over the workgroup then gives every entry its
// dense index and its rank in its class.
// ------------------------------------------------------------------------------------------------
constexpr int kFusedMaxMP = 4 * 4 * kThreads;
static_assert(kParts == 4, "fused_scan packs four 16-bit range counters into a 64-bit word");
struct FusedLds {
    unsigned long long wcnt[kThreads / 64], wodd[kThreads / 64];     // per wave: the inclusive totals
};
__device__ __forceinline__ int fused_field(unsigned long long v, int q) { return (int)((v >> (16 * q)) & 0xffffull); }

// WIN: the size of the workgroup's window, `base` its start.  BY_VALUE: the window is over point indices (the culling sweep: row
// base + i IS point base + i) and row_sl[i] receives the slot of point base + i, or -1; otherwise it is over the dense list (row slot
// base + i takes the (base + i)-th live entry) and row_l / row_sl receive the point and its slot.  Returns the dense count; tcnt /
// todd: the class totals.  Ends with a barrier.
template <int WIN, bool BY_VALUE>
__device__ __forceinline__ int fused_scan(const Ctx& c, const int* lin, int base, FusedLds& lds, int* row_l, int* row_sl, unsigned long long& tcnt,
                                          unsigned long long& todd) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int cand = c.MP / kParts;
    const int groups = c.MP / 4, G = (groups + kThreads - 1) / kThreads;      // int4 groups of the list, per thread
    int e[16];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int idx = tid * G + g;
        int4 v = make_int4(-1, -1, -1, -1);
        if (g < G && idx < groups) v = reinterpret_cast<const int4*>(lin)[idx];
        e[4 * g] = v.x;
        e[4 * g + 1] = v.y;
        e[4 * g + 2] = v.z;
        e[4 * g + 3] = v.w;
    }
    auto live = [&](int x) { return (unsigned)x < (unsigned)c.MP; };
    auto shift = [&](int x) { return 16 * ((x >= cand ? 1 : 0) + (x >= 2 * cand ? 1 : 0) + (x >= 3 * cand ? 1 : 0)); };
    unsigned long long acnt = 0ull, aodd = 0ull;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const unsigned long long one = live(e[q]) ? 1ull << shift(e[q]) : 0ull;
        acnt += one;
        aodd += (e[q] & 1) ? one : 0ull;
    }
    unsigned long long icnt = acnt, iodd = aodd;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t0 = __shfl_up(icnt, o, 64), t1 = __shfl_up(iodd, o, 64);
        if (lane >= o) {
            icnt += t0;
            iodd += t1;
        }
    }
    if (lane == 63) {
        lds.wcnt[wid] = icnt;
        lds.wodd[wid] = iodd;
    }
    if (BY_VALUE)
        for (int i = tid; i < WIN; i += kThreads) row_sl[i] = -1;
    __syncthreads();
    unsigned long long xcnt = icnt - acnt, xodd = iodd - aodd;      // exclusive: the entries before this thread's
    tcnt = 0ull;
    todd = 0ull;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
        const unsigned long long wc = lds.wcnt[w], wo = lds.wodd[w];
        tcnt += wc;
        todd += wo;
        if (w < wid) {
            xcnt += wc;
            xodd += wo;
        }
    }
    int dense = fused_field(xcnt, 0) + fused_field(xcnt, 1) + fused_field(xcnt, 2) + fused_field(xcnt, 3);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        if (!live(e[q])) continue;
        const int sh = shift(e[q]), par = e[q] & 1;
        const int nall = (int)((xcnt >> sh) & 0xffffull), nodd = (int)((xodd >> sh) & 0xffffull);
        const int rank = par ? nodd : nall - nodd;
        const int w = (BY_VALUE ? e[q] : dense) - base;
        if ((unsigned)w < (unsigned)WIN) {
            if (!BY_VALUE) row_l[w] = e[q];
            row_sl[w] = (sh >> 4) * cand + 2 * rank + par;
        }
        xcnt += 1ull << sh;
        xodd += par ? 1ull << sh : 0ull;
        ++dense;
    }
    __syncthreads();
    return fused_field(tcnt, 0) + fused_field(tcnt, 1) + fused_field(tcnt, 2) + fused_field(tcnt, 3);
}
// Workgroup 0 of a cloud: the merged launch's loop iterations per candidate range, and each class padded from its count to whole
// iterations (2 stages = kStage pair records) with zero-weight records at the origin — emd_compact_kernel's last loop.
__device__ __forceinline__ void fused_pad(const Ctx& c, float* cs, unsigned long long tcnt, unsigned long long todd) {
    const int tid = threadIdx.x;
    const int cand = c.MP / kParts;
    float* rec = cs + c.cs_rec;
    float* wr = cs + c.cs_w;
    if (tid < kParts) {
        const int nodd = fused_field(todd, tid), nev = fused_field(tcnt, tid) - nodd;
        reinterpret_cast<int*>(cs + c.cs_cnt)[4 + tid] = (max(nev, nodd) + kStage - 1) / kStage;
    }
    for (int sl = tid; sl < c.MP; sl += kThreads) {
        const int p = (sl >= cand ? 1 : 0) + (sl >= 2 * cand ? 1 : 0) + (sl >= 3 * cand ? 1 : 0), r = (sl - p * cand) >> 1, par = sl & 1;
        const int nodd = fused_field(todd, p), nev = fused_field(tcnt, p) - nodd;
        const int end = (max(nev, nodd) + kStage - 1) / kStage * kStage;
        if (r >= (par ? nodd : nev) && r < end) {
#pragma unroll
            for (int q = 0; q < 4; ++q) rec[pair8(sl, q)] = 0.f;
            wr[sl] = 0.f;
        }
    }
}

// COMPACT (round 7): the rows are the set2 points alive on entry to the level — the list `li` of the cloud's scratch
// (emd_compact_kernel) —, row slot i takes list entry i; the grid is sized from the shapes and the workgroups past the list's
// length leave at once.  Results go to the points' own positions, as before.
// MODE 0: every point a row; 1: COMPACT; 2: FUSED (round 9, fused_scan) — the rows are the live entries of the list the previous phase-2
// launch left (list (lev - 1) & 1), found by the workgroup's own scan, and with `li` != 0 the launch leaves the next list (lev & 1)
// and the next merged launch's candidates; 3: every point a row, and the launch leaves the first list.
//
// FEED (round 12, the list-driven modes 1 and 2 only) — how the candidates reach the waves.  0: the scalar path, as everywhere else in
// this file.  1 (default): through LDS.  A list-driven launch has a fraction of the full sweep's workgroups — spread over the chip
// (PLACEMENT, below) one wave per SIMD or less —, so little covers the scalar loads' round trips.  Here the workgroup copies the
// cloud's PLP records (NP float4, one per candidate) into LDS once, with 16-byte loads that are all in flight together and issued
// ahead of the list scan, and each wave walks its range with wave-uniform (broadcast) 16-byte LDS reads, one stage ahead.  Only
// the operand source changes — VGPRs for SGPRs —: per row and per (range, parity) class the same terms enter the same fma chain
// in the same order (rows2_term), so the feeds agree bit for bit (tests/test_emd_rows2_feed_gpu.py).  The staged block is static LDS,
// so sets of more than kFeedMaxNP (padded) points take the scalar feed (LevelChain).
constexpr int kFeedMaxNP = 2048;                           // 32 KB of LDS; two chains' workgroups share a CU's 160 KB
constexpr int kFeedLoads = kFeedMaxNP / kThreads;          // staging loads per thread
static_assert(kFeedMaxNP % kThreads == 0 && (kFeedMaxNP + kSpare) * sizeof(float4) + 8 * 1024 <= 64 * 1024, "the static LDS of a workgroup");

template <int R, int MODE = 0, int FEED = 0>
__global__ __launch_bounds__(kThreads) void emd_rows2_kernel(Ctx c, int lev, float l2e, int li) {
    constexpr bool COMPACT = MODE == 1, FUSED = MODE == 2, LDS = FEED == 1;
    static_assert(!LDS || COMPACT || FUSED, "the LDS feed serves the list-driven sweeps");
    __shared__ float parts[kParts][kRowsPerWg * R];
    __shared__ FusedLds flds;
    __shared__ int row_l[FUSED ? kRowsPerWg * R : 1], row_sl[FUSED ? kRowsPerWg * R : 1];
    // the cloud's PLP records, one float4 per candidate ([x0 x1 y0 y1] / [z0 z1 w0 w1] of a pair), and kSpare slots nobody fills: the
    // read-ahead past the last range's last stage lands there and is never used
    __shared__ float4 staged[LDS ? kFeedMaxNP + kSpare : 1];
    // PLACEMENT (round 12).  Workgroups are dealt to the 8 XCDs round-robin in launch order, x fastest.  A list is dense, so a cloud's
    // live row tiles are its first k: with the tile in x (the full sweeps' grid) the live workgroups of EVERY cloud land on the same k
    // of 8 XCDs, two or more deep per CU while the other XCDs run the workgroups that leave at once — the launch took 54-60 us at any
    // k (profiles/r12_one_chain_levels.md).  The list-driven launches therefore take the cloud from x and the tile from y
    // (LevelChain::grid_listed): tile t of all clouds before tile t + 1 of any, the live workgroups first and spread over the whole chip.
    constexpr bool LISTED = COMPACT || FUSED;
    const int cloud = emd_wave_prio(LISTED ? blockIdx.x : blockIdx.y), tile = LISTED ? blockIdx.y : blockIdx.x;
    const int lrow = threadIdx.x % kRowsPerWg;
    const int part = __builtin_amdgcn_readfirstlane(threadIdx.x / kRowsPerWg);
    float* ws = c.ws + (long)cloud * c.per_cloud;
    float* remR = c.temp + (long)cloud * (c.n + c.m) * 2 + c.n;
    float* ratioR = remR + c.m + c.n;
    const float* cs = c.cs + (long)cloud * c.cs_per_cloud;
    const int* list = reinterpret_cast<const int*>(cs + (li ? c.cs_list1 : c.cs_list0));
    int rows = COMPACT ? __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(cs + c.cs_cnt)[li]) : c.m;
    if (COMPACT && tile * R * kRowsPerWg >= rows) return;
    // LDS feed: the staging loads first, so that the list scan's and the row set-up's own loads share their round trip
    [[maybe_unused]] float4 st[kFeedLoads];
    if constexpr (LDS) {
        const float4* src = reinterpret_cast<const float4*>(ws + c.plp);
#pragma unroll
        for (int g = 0; g < kFeedLoads; ++g) {
            const int i = g * kThreads + (int)threadIdx.x;
            st[g] = i < c.NP ? src[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    FusedOut fo;
    if constexpr (MODE >= 2) {
        float* csw = c.cs + (long)cloud * c.cs_per_cloud;
        fo.lout = reinterpret_cast<int*>(csw + ((lev & 1) ? c.cs_list1 : c.cs_list0));
        fo.rec = csw + c.cs_rec;
        fo.wr = csw + c.cs_w;
        fo.seg = tile * R * kRowsPerWg;
        fo.produce = li != 0;
        if constexpr (FUSED) {
            unsigned long long tcnt, todd;
            rows = __builtin_amdgcn_readfirstlane(fused_scan<kRowsPerWg * R, false>(
                c, reinterpret_cast<const int*>(csw + ((lev & 1) ? c.cs_list0 : c.cs_list1)), fo.seg, flds, row_l, row_sl, tcnt, todd));
            if (tile == 0 && fo.produce) fused_pad(c, csw, tcnt, todd);
            if (fo.seg >= rows) {
                if (fo.produce)
                    for (int i = threadIdx.x; i < kRowsPerWg * R && fo.seg + i < c.MP; i += kThreads) fo.lout[fo.seg + i] = -1;
                return;
            }
        }
    }
    int l[R];
    [[maybe_unused]] int sl[R];
    bool ok[R];
    f2 qx2[R], qy2[R], qz2[R], acc2[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = (tile * R + r) * kRowsPerWg + lrow;
        ok[r] = i < rows;
        l[r] = COMPACT ? (ok[r] ? list[i] : 0) : FUSED ? (ok[r] ? row_l[r * kRowsPerWg + lrow] : 0) : i;
        if (FUSED) sl[r] = ok[r] ? row_sl[r * kRowsPerWg + lrow] : -1;
        rows2_setup(c, ws, l[r], ok[r], qx2[r], qy2[r], qz2[r], acc2[r]);
    }
    const f2 lv = splat2(l2e);
    const int cand = c.NP / kParts;
    // one candidate pair's term of row r, whichever registers hold the record
    auto rows2_term = [&](int r, f2 x, f2 y, f2 z, f2 w) {
        // the reference evaluates (x2-x1) with x2 the set2 point in every phase (approxmatch.cu:85,131,185)
        const f2 d = sqdist2(qx2[r] - x, qy2[r] - y, qz2[r] - z);
        acc2[r] = __builtin_elementwise_fma(exp2_2(lv * d), w, acc2[r]);   // approxmatch.cu:131-132 contracted
    };
    if constexpr (LDS) {
#pragma unroll
        for (int g = 0; g < kFeedLoads; ++g) {
            const int i = g * kThreads + (int)threadIdx.x;
            if (i < c.NP) staged[i] = st[g];
        }
        __syncthreads();
        const float4* sp = staged + part * cand;      // wave-uniform: every read below is a broadcast
        float4 a[kStage], b[kStage];
        auto fetch = [&](float4(&v)[kStage], int k) {
#pragma unroll
            for (int q = 0; q < kStage; ++q) v[q] = sp[k + q];
        };
        auto work = [&](const float4(&v)[kStage]) {
#pragma unroll
            for (int u = 0; u < kStage / 2; ++u) {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    rows2_term(r, f2{v[2 * u].x, v[2 * u].y}, f2{v[2 * u].z, v[2 * u].w}, f2{v[2 * u + 1].x, v[2 * u + 1].y},
                               f2{v[2 * u + 1].z, v[2 * u + 1].w});
            }
        };
        fetch(a, 0);
        for (int k0 = 0; k0 < cand; k0 += 2 * kStage) {      // the scalar walk's stages in its order, the next one's reads in flight
            fetch(b, k0 + kStage);
            work(a);
            fetch(a, k0 + 2 * kStage);      // (past the last range's end: the spare slots)
            work(b);
        }
    } else {
        const float* p = ws + c.plp + (long)part * cand * 4;
        f32x16 a0, a1, b0, b1;
        auto work = [&](const f32x16& lo, const f32x16& hi) {
#pragma unroll
            for (int u = 0; u < kStage / 2; ++u) {
#pragma unroll
                for (int r = 0; r < R; ++r) rows2_term(r, PAIRC(lo, hi, u, 0), PAIRC(lo, hi, u, 1), PAIRC(lo, hi, u, 2), PAIRC(lo, hi, u, 3));
            }
        };
        HP_SLOAD16(a0, p, 0x0);
        HP_SLOAD16(a1, p, 0x40);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a0), "+s"(a1));
        for (int k0 = 0; k0 < cand; k0 += 2 * kStage) {
            p += kStage * 4;
            HP_SLOAD16(b0, p, 0x0);
            HP_SLOAD16(b1, p, 0x40);
            HP_PIN();
            work(a0, a1);
            if (R == 1) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(b0), "+s"(b1), "+v"(acc2[0]));
            else asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(b0), "+s"(b1), "+v"(acc2[0]), "+v"(acc2[R - 1]));
            p += kStage * 4;
            HP_SLOAD16(a0, p, 0x0);
            HP_SLOAD16(a1, p, 0x40);
            HP_PIN();
            work(b0, b1);
            if (R == 1) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a0), "+s"(a1), "+v"(acc2[0]));
            else asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a0), "+s"(a1), "+v"(acc2[0]), "+v"(acc2[R - 1]));
        }
    }
    if constexpr (MODE >= 2) rows2_finish<R, FUSED ? 2 : 1>(c, ws, remR, ratioR, lrow, part, lev, l, ok, acc2, parts, fo, sl, qx2, qy2, qz2);
    else rows2_finish<R>(c, ws, remR, ratioR, lrow, part, lev, l, ok, acc2, parts);
}

// ------------------------------------------------------------------------------------------------
// Round 7: COMPACTION of the exhausted set2 points.  Phase 2 clamps remainR to exactly +0 once a point is oversubscribed
// (approxmatch.cu:141, the auction itself, not a rounding effect), and then the point stays at +0: its own phase-2 row gives
// ratioR = +0 and remainR = +0 without reading a candidate (sumr = a * 0, consumption = 0 / 1e-9), and as a candidate it adds exact
// zeros — fma(e, remainR = 0, acc) in phase 1, fma(e * ratioL, ratioR = 0, acc) in phase 3 (e <= 1, every sum >= +0).  So after the
// phase-2 launch of level j one workgroup per cloud, in order (no atomics: the lists are pure functions of the values), writes
//   (a) the row list L_{j+1} = {remainR != 0}, ascending, for the next phase-2 launch (emd_rows2_kernel<R, true>);
//   (b) the candidates of the merged phase-3(j) / phase-1(j+1) launch (emd_rows1_kernel<.., true>): the points with ratioR_j != 0 or
//       remainR != 0, compacted per CLASS — the candidate range (wave `part`) and the parity (the even / odd half of the packed
//       accumulator) the point had in the full sweep —, each class in ascending order, paired as [even_i | odd_i] and padded with
//       zero-weight records at the origin to whole loop iterations: every accumulator of every row receives the same non-zero terms in
//       the same order as in the full sweep, so the sums are bit-identical;
//   (c) ratioR = +0 in `temp` for the points that leave (the full sweeps wrote +0 there at every later level).
// The input is L_j (list `li_in`), or every point of the set behind the first plain level's predecessor (`first`: there the test
// ratioR_j != 0 || remainR != 0 over all points is exact on its own).
// ------------------------------------------------------------------------------------------------
constexpr int kCompactThreads = 1024;
constexpr int kClasses = 2 * kParts;       // (candidate range, parity)

__global__ __launch_bounds__(kCompactThreads) void emd_compact_kernel(Ctx c, int first, int li_in, int li_out) {
    __shared__ int wtot[kCompactThreads / 64][kClasses + 1];     // per wave: the class counts, then the live rows
    __shared__ int run[kClasses + 1];                            // the same, over the chunks done
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int cloud = emd_wave_prio(blockIdx.x);
    const float* ws = c.ws + (long)cloud * c.per_cloud;
    float* cs = c.cs + (long)cloud * c.cs_per_cloud;
    float* ratioR = c.temp + (long)cloud * (c.n + c.m) * 2 + 2 * c.n + c.m;
    int* cnt = reinterpret_cast<int*>(cs + c.cs_cnt);
    const int* lin = reinterpret_cast<const int*>(cs + (li_in ? c.cs_list1 : c.cs_list0));
    int* lout = reinterpret_cast<int*>(cs + (li_out ? c.cs_list1 : c.cs_list0));
    float* rec = cs + c.cs_rec;
    float* wr = cs + c.cs_w;
    const int count = first ? c.m : cnt[li_in];
    const int cand = c.MP / kParts;
    const unsigned long long below = (1ull << lane) - 1ull;
    if (tid <= kClasses) run[tid] = 0;
    __syncthreads();
    for (int base = 0; base < count; base += kCompactThreads) {
        const int i = base + tid;
        const bool valid = i < count;
        const int l = valid ? (first ? i : lin[i]) : 0;
        float x = 0.f, y = 0.f, z = 0.f, w = 0.f, rem = 0.f;
        if (valid) {
            x = ws[c.prp + pair8(l, 0)];
            y = ws[c.prp + pair8(l, 1)];
            z = ws[c.prp + pair8(l, 2)];
            w = ws[c.prp + pair8(l, 3)];      // ratioR_j
            rem = ws[c.rr + l];               // remainR after phase 2 of level j
        }
        const bool live = valid && rem != 0.f;
        const bool keep = valid && (w != 0.f || rem != 0.f);
        const int cls = (l / cand) * 2 + (l & 1);
        const unsigned long long bl = __ballot(live);
        if (lane == 0) wtot[wid][kClasses] = __popcll(bl);
        int rank = 0;
#pragma unroll
        for (int q = 0; q < kClasses; ++q) {
            const unsigned long long bq = __ballot(keep && cls == q);
            if (cls == q) rank = __popcll(bq & below);
            if (lane == 0) wtot[wid][q] = __popcll(bq);
        }
        __syncthreads();
        int orow = run[kClasses] + __popcll(bl & below), ocls = run[cls] + rank;
        for (int v = 0; v < wid; ++v) {
            orow += wtot[v][kClasses];
            ocls += wtot[v][cls];
        }
        if (live) lout[orow] = l;
        else if (valid) ratioR[l] = 0.f;
        if (keep) {
            const int sl = (cls >> 1) * cand + 2 * ocls + (cls & 1);      // the class's ocls-th pair record, its half
            rec[pair8(sl, 0)] = x;
            rec[pair8(sl, 1)] = y;
            rec[pair8(sl, 2)] = z;
            rec[pair8(sl, 3)] = w;
            wr[sl] = rem;
        }
        __syncthreads();
        if (tid <= kClasses) {
            int t = 0;
            for (int v = 0; v < kCompactThreads / 64; ++v) t += wtot[v][tid];
            run[tid] += t;
        }
        __syncthreads();
    }
    // each range to whole loop iterations (2 stages = kStage pair records) with zero-weight records at the origin
    for (int sl = tid; sl < c.MP; sl += kCompactThreads) {
        const int p = sl / cand, r = (sl - p * cand) >> 1, par = sl & 1;
        const int end = (max(run[2 * p], run[2 * p + 1]) + kStage - 1) / kStage * kStage;
        if (r >= run[2 * p + par] && r < end) {
#pragma unroll
            for (int q = 0; q < 4; ++q) rec[pair8(sl, q)] = 0.f;
            wr[sl] = 0.f;
        }
    }
    if (tid == 0) cnt[li_out] = run[kClasses];
    if (tid < kParts) cnt[4 + tid] = (max(run[2 * tid], run[2 * tid + 1]) + kStage - 1) / kStage;
}

// ------------------------------------------------------------------------------------------------
// Culling sweeps (records in Hilbert order).  Same rows, same candidates, same arithmetic per (row, candidate) as emd_rows1_kernel /
// emd_rows2_kernel; the candidate set is cut into blocks of 8 (one pipeline stage), block g belongs to the workgroup's wave
// (g mod kParts) — interleaved, so that the blocks near a row tile spread over the 4 waves (8 or 16 waves per row tile were tried for
// the sparse levels and lost: 1.18 -> 1.22 / 1.30 ms per call) —, and a (64-row tile, block) unit is evaluated only if the two
// bounding boxes are closer than the level's underflow radius.  Every skipped term is an exact zero (exp2 of less than -152;
// fma(0, w, acc) == acc), so a row's sum is the sum over its surviving blocks in ascending order — the reference's sum with its zero
// terms left out.  The culling kernels run ONE row per lane whatever the plain kernels' rows per lane are (a launch is one round of
// workgroups and lasts as long as its slowest CU: finer workgroups balance; two rows per lane: +3 % per call), so a row's result does
// not depend on hp_emd_set_rows_per_lane.  Lane i of a wave tests block i of its range (one ballot per row tile = per wave), the
// surviving blocks are walked with s_ff1 on the masks, their records prefetched one block ahead on the scalar path as before.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float box_gap2(const float (&tlo)[3], const float (&thi)[3], float cx0, float cy0, float cz0, float cx1, float cy1,
                                          float cz1) {
    const float gx = fmaxf(0.f, fmaxf(cx0 - thi[0], tlo[0] - cx1));
    const float gy = fmaxf(0.f, fmaxf(cy0 - thi[1], tlo[1] - cy1));
    const float gz = fmaxf(0.f, fmaxf(cz0 - thi[2], tlo[2] - cz1));
    return gx * gx + gy * gy + gz * gz;
}
// tile t's box (uniform address: scalar loads); tiles past the last one are empty
__device__ __forceinline__ void load_tile_box(const float* tb, int NT, int t, float (&lo)[3], float (&hi)[3]) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        lo[q] = t < NT ? tb[q * NT + t] : kFar;
        hi[q] = t < NT ? tb[(3 + q) * NT + t] : -kFar;
    }
}

template <bool DO3, bool DO1>
__global__ __launch_bounds__(kThreads) void emd_rows1_cull_kernel(Ctx c, int lev1, float l2e3, float l2e1, float thr3, float thr1) {
    __shared__ float part3[kParts][kRowsPerWg], part1[kParts][kRowsPerWg];
    const int cloud = emd_wave_prio(blockIdx.y);
    const int lrow = threadIdx.x % kRowsPerWg;
    const int part = __builtin_amdgcn_readfirstlane(threadIdx.x / kRowsPerWg);   // wave-uniform
    float* ws = c.ws + (long)cloud * c.per_cloud;
    float* remL = c.temp + (long)cloud * (c.n + c.m) * 2;
    float* ratioL = remL + c.n + c.m;
    const int k = blockIdx.x * kRowsPerWg + lrow;
    bool ok;
    f2 px2, py2, pz2, rl2, acc3, acc1;
    rows1_setup<DO3>(c, ws, ratioL, k, part, ok, px2, py2, pz2, rl2, acc3, acc1);
    float tlo[3], thi[3];
    load_tile_box(ws + c.tileL, c.NP / kTile, blockIdx.x, tlo, thi);
    const f2 l3 = splat2(l2e3), l1 = splat2(l2e1);
    const int NB = c.MP / kBlk, nblk = (NB + kParts - 1) / kParts;     // blocks of the set, blocks of this wave's range (g = i * kParts + part)
    const float* bb = ws + c.blkR;
    const float* prec = ws + c.prp;
    const float* wrec = ws + c.rr;
    const int lane = threadIdx.x & 63;
    f32x16 a0, a1, b0, b1;
    f32x8 w0 = {}, w1 = {};
    for (int ch = 0; ch < nblk; ch += 64) {
        // which blocks of this chunk can any row of the tile reach at the level of phase 1 (any) / phase 3 (mask3 <= any)
        unsigned long long mask3, any;
        {
            const int i = ch + lane;
            const bool valid = i * kParts + part < NB;
            const int g = valid ? i * kParts + part : 0;
            const float cx0 = bb[g], cy0 = bb[NB + g], cz0 = bb[2 * NB + g], cx1 = bb[3 * NB + g], cy1 = bb[4 * NB + g], cz1 = bb[5 * NB + g];
            const float g2 = box_gap2(tlo, thi, cx0, cy0, cz0, cx1, cy1, cz1);
            mask3 = DO3 ? __ballot(valid && g2 <= thr3) : 0ull;
            any = DO1 ? __ballot(valid && g2 <= thr1) : mask3;
        }
        // one stage for the lane's row (a walked block has its bit in `any`): phase 3 + phase 1, or phase 1 alone where the block is
        // beyond phase 3's radius
        auto work = [&](const f32x16& lo, const f32x16& hi, const f32x8& w, int bi) {
            const bool on3 = DO3 && ((mask3 >> bi) & 1ull);
            if (on3 || !DO1) {
#pragma unroll
                for (int u = 0; u < kStage / 2; ++u) {
                    const f2 d = sqdist2(PAIRC(lo, hi, u, 0) - px2, PAIRC(lo, hi, u, 1) - py2, PAIRC(lo, hi, u, 2) - pz2);
                    acc3 = __builtin_elementwise_fma(exp2_2(l3 * d) * rl2, PAIRC(lo, hi, u, 3), acc3);   // (e * ratioL[k]) * ratioR[l]
                    if (DO1) acc1 = __builtin_elementwise_fma(exp2_2(l1 * d), f2{w[u * 2], w[u * 2 + 1]}, acc1);   // e * remainR[l]
                }
            } else {
#pragma unroll
                for (int u = 0; u < kStage / 2; ++u) {
                    const f2 d = sqdist2(PAIRC(lo, hi, u, 0) - px2, PAIRC(lo, hi, u, 1) - py2, PAIRC(lo, hi, u, 2) - pz2);
                    acc1 = __builtin_elementwise_fma(exp2_2(l1 * d), f2{w[u * 2], w[u * 2 + 1]}, acc1);
                }
            }
        };
        if (any == 0ull) continue;
        int ia = __builtin_ctzll(any), ib = 0;
        any &= any - 1ull;
        {
            const long g = (long)(ch + ia) * kParts + part;
            const float* p = prec + g * (kBlk * 4);
            const float* q = wrec + g * kBlk;
            HP_SLOAD16(a0, p, 0x0);
            HP_SLOAD16(a1, p, 0x40);
            if (DO1) HP_SLOAD8(w0, q, 0x0);
            asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a0), "+s"(a1), "+s"(w0));
        }
        while (true) {
            const bool more_b = any != 0ull;
            if (more_b) {
                ib = __builtin_ctzll(any);
                any &= any - 1ull;
                const long g = (long)(ch + ib) * kParts + part;
                const float* p = prec + g * (kBlk * 4);
                const float* q = wrec + g * kBlk;
                HP_SLOAD16(b0, p, 0x0);
                HP_SLOAD16(b1, p, 0x40);
                if (DO1) HP_SLOAD8(w1, q, 0x0);
            }
            HP_PIN();
            work(a0, a1, w0, ia);
            asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(b0), "+s"(b1), "+s"(w1), "+v"(acc3), "+v"(acc1));
            if (!more_b) break;
            const bool more_a = any != 0ull;
            if (more_a) {
                ia = __builtin_ctzll(any);
                any &= any - 1ull;
                const long g = (long)(ch + ia) * kParts + part;
                const float* p = prec + g * (kBlk * 4);
                const float* q = wrec + g * kBlk;
                HP_SLOAD16(a0, p, 0x0);
                HP_SLOAD16(a1, p, 0x40);
                if (DO1) HP_SLOAD8(w0, q, 0x0);
            }
            HP_PIN();
            work(b0, b1, w1, ib);
            asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a0), "+s"(a1), "+s"(w0), "+v"(acc3), "+v"(acc1));
            if (!more_a) break;
        }
    }
    rows1_finish<DO3, DO1, 1>(c, ws, remL, ratioL, lrow, part, lev1, &k, &ok, &acc3, &acc1, part3, part1);
}

// FUSED (round 9, fused_scan) 1: the launch leaves the first row list (lev & 1); 2: its rows are still all the points, but it
// reads the list the previous launch left for the slots of the alive ones, and leaves the next list and the next merged launch's
// candidates (the last culled level).
template <int FUSED = 0>
__global__ __launch_bounds__(kThreads) void emd_rows2_cull_kernel(Ctx c, int lev, float l2e, float thr) {
    __shared__ float parts[kParts][kRowsPerWg];
    __shared__ FusedLds flds;
    __shared__ int row_sl[FUSED == 2 ? kRowsPerWg : 1];
    const int cloud = blockIdx.y;
    const int lrow = threadIdx.x % kRowsPerWg;
    const int part = __builtin_amdgcn_readfirstlane(threadIdx.x / kRowsPerWg);
    float* ws = c.ws + (long)cloud * c.per_cloud;
    float* remR = c.temp + (long)cloud * (c.n + c.m) * 2 + c.n;
    float* ratioR = remR + c.m + c.n;
    const unsigned seg = emd_wave_prio(blockIdx.x) * kRowsPerWg;
    const int l = seg + lrow;
    const bool ok = l < c.m;
    f2 qx2, qy2, qz2, acc2;
    rows2_setup(c, ws, l, ok, qx2, qy2, qz2, acc2);
    FusedOut fo;
    int sl = -1;
    if constexpr (FUSED != 0) {
        float* csw = c.cs + (long)cloud * c.cs_per_cloud;
        fo.lout = reinterpret_cast<int*>(csw + ((lev & 1) ? c.cs_list1 : c.cs_list0));
        fo.rec = csw + c.cs_rec;
        fo.wr = csw + c.cs_w;
        fo.seg = seg;
        fo.produce = true;
        if constexpr (FUSED == 2) {
            unsigned long long tcnt, todd;
            fused_scan<kRowsPerWg, true>(c, reinterpret_cast<const int*>(csw + ((lev & 1) ? c.cs_list0 : c.cs_list1)), fo.seg, flds, nullptr, row_sl,
                                         tcnt, todd);
            if (blockIdx.x == 0) fused_pad(c, csw, tcnt, todd);
            sl = row_sl[lrow];
        }
    }
    float tlo[3], thi[3];
    load_tile_box(ws + c.tileR, c.MP / kTile, blockIdx.x, tlo, thi);
    const f2 lv = splat2(l2e);
    const int NB = c.NP / kBlk, nblk = (NB + kParts - 1) / kParts;
    const float* bb = ws + c.blkL;
    const float* prec = ws + c.plp;
    const int lane = threadIdx.x & 63;
    f32x16 a0, a1, b0, b1;
    for (int ch = 0; ch < nblk; ch += 64) {
        unsigned long long any;      // the blocks of this chunk some row of the tile can reach
        {
            const int i = ch + lane;
            const bool valid = i * kParts + part < NB;
            const int g = valid ? i * kParts + part : 0;
            const float cx0 = bb[g], cy0 = bb[NB + g], cz0 = bb[2 * NB + g], cx1 = bb[3 * NB + g], cy1 = bb[4 * NB + g], cz1 = bb[5 * NB + g];
            any = __ballot(valid && box_gap2(tlo, thi, cx0, cy0, cz0, cx1, cy1, cz1) <= thr);
        }
        auto work = [&](const f32x16& lo, const f32x16& hi) {
#pragma unroll
            for (int u = 0; u < kStage / 2; ++u) {
                const f2 d = sqdist2(qx2 - PAIRC(lo, hi, u, 0), qy2 - PAIRC(lo, hi, u, 1), qz2 - PAIRC(lo, hi, u, 2));
                acc2 = __builtin_elementwise_fma(exp2_2(lv * d), PAIRC(lo, hi, u, 3), acc2);   // approxmatch.cu:131-132 contracted
            }
        };
        if (any == 0ull) continue;
        int ia = __builtin_ctzll(any), ib;
        any &= any - 1ull;
        {
            const float* p = prec + ((long)(ch + ia) * kParts + part) * (kBlk * 4);
            HP_SLOAD16(a0, p, 0x0);
            HP_SLOAD16(a1, p, 0x40);
            asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a0), "+s"(a1));
        }
        while (true) {
            const bool more_b = any != 0ull;
            if (more_b) {
                ib = __builtin_ctzll(any);
                any &= any - 1ull;
                const float* p = prec + ((long)(ch + ib) * kParts + part) * (kBlk * 4);
                HP_SLOAD16(b0, p, 0x0);
                HP_SLOAD16(b1, p, 0x40);
            }
            HP_PIN();
            work(a0, a1);
            asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(b0), "+s"(b1), "+v"(acc2));
            if (!more_b) break;
            const bool more_a = any != 0ull;
            if (more_a) {
                ia = __builtin_ctzll(any);
                any &= any - 1ull;
                const float* p = prec + ((long)(ch + ia) * kParts + part) * (kBlk * 4);
                HP_SLOAD16(a0, p, 0x0);
                HP_SLOAD16(a1, p, 0x40);
            }
            HP_PIN();
            work(b0, b1);
            asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a0), "+s"(a1), "+v"(acc2));
            if (!more_a) break;
        }
    }
    rows2_finish<1, FUSED>(c, ws, remR, ratioR, lrow, part, lev, &l, &ok, &acc2, parts, fo, &sl, &qx2, &qy2, &qz2);
}

// final pair record (two x16 SGPR groups): component q (0..2 xyz, 3+lev ratio) as a float2
#define FINC(lo, hi, q) ((q) < 8 ? f2{(lo)[(q)*2], (lo)[(q)*2 + 1]} : f2{(hi)[((q)-8) * 2], (hi)[((q)-8) * 2 + 1]})

// M(l,k) for the two candidates of a pair record = sum over levels, in level order, of
//   ROW_IS_L: (exp(level*d) * ratioL_lev[row]) * ratioR_lev[cand]     (row = set1 point, candidates = set2)
//   else    : (exp(level*d) * ratioL_lev[cand]) * ratioR_lev[row]
// DERIVE (the cost / gradient sweeps of the training path; never the `match` the API returns): the levels are exact powers of
// 4 apart — l_j * d = 4 * (l_{j+1} * d) bit for bit — so exp2(l_j d) = exp2(l_{j+1} d)^4, and levels 0, 2, 4, 6 are formed as the
// fourth power (two packed multiplies) of the hardware exponential of levels 1, 3, 5, 7: five v_exp_f32 per pair instead of nine.
// A derived value carries ~5 ulp (4 x the exponential's + the two squarings') instead of 1.  Round 3 tried this in the LEVEL sweeps
// as well and the auction amplified it past the parity bars (docs/DESIGN_HISTORY.md 7b); here nothing is downstream of the value: M moves by
// <= 3.5e-7 relative, cost and gradients by less (tests: the cost error map's bars are unchanged, and the exact form stays
// selectable: hp_emd_set_final_derive).
// SKIP (round 6): the first SKIP levels' exponentials are known to be exactly zero for this (row tile, candidate block) — the
// boxes are further apart than those levels' underflow radius (the culling test of the level sweeps; a derived value is the
// fourth power of a hardware exponential below 2^-38, i.e. below 2^-152: zero as well) — and their terms are left out.
template <bool ROW_IS_L, bool DERIVE, int SKIP = 0>
__device__ __forceinline__ f2 match_entry2(f2 d, const float (&row)[kLevels], const f32x16& lo, const f32x16& hi) {
    f2 acc = splat2(0.f);
    f2 ev[kLevels];
#pragma unroll
    for (int lev = kLevels - 1; lev >= 0; --lev) {
        if (lev < SKIP) continue;      // (an odd level is the source of the even level below it only: nothing kept derives from a skipped one)
        if (!DERIVE || lev == kLevels - 1 || (lev & 1)) {
            ev[lev] = exp2_2(splat2(level_l2e(lev)) * d);
        } else {
            const f2 sq = ev[lev + 1] * ev[lev + 1];
            ev[lev] = sq * sq;
        }
    }
#pragma unroll
    for (int lev = SKIP; lev < kLevels; ++lev) {
        const f2 e = ev[lev];
        const f2 cr = FINC(lo, hi, 3 + lev);
        // the level's term rides on an fma into the running sum (one rounding instead of the reference's two, i.e. a
        // slightly more accurate M; unlike the phase sweeps nothing downstream amplifies it: cost moves by ~1e-7 relative)
        acc = ROW_IS_L ? __builtin_elementwise_fma(e * splat2(row[lev]), cr, acc)
                       : __builtin_elementwise_fma(e * cr, splat2(row[lev]), acc);
    }
    return acc;
}

__device__ __forceinline__ void load_row_final(const float* rec, int i, float& x, float& y, float& z, float (&r)[kLevels]) {
    x = rec[pair32(i, 0)];
    y = rec[pair32(i, 1)];
    z = rec[pair32(i, 2)];
#pragma unroll
    for (int lev = 0; lev < kLevels; ++lev) r[lev] = rec[pair32(i, 3 + lev)];
}

constexpr int kLT = 64;  // match rows (l) per workgroup in the materialising pass
__global__ __launch_bounds__(kThreads) void emd_match_kernel(Ctx c, float* __restrict__ match) {
    const int cloud = blockIdx.z;
    const int k = blockIdx.x * kThreads + threadIdx.x;
    const int l0 = blockIdx.y * kLT;
    const float* ws = c.ws + (long)cloud * c.per_cloud;
    const bool ok = k < c.n;
    float px = 0.f, py = 0.f, pz = 0.f, rL[kLevels] = {};
    if (ok) load_row_final(ws + c.flp, k, px, py, pz, rL);
    const f2 px2 = splat2(px), py2 = splat2(py), pz2 = splat2(pz);
    float* out = match + ((long)cloud * c.m + l0) * c.n + k;
    const int cnt = min(kLT, c.m - l0);          // l0 is even; spare records exist past MP
    const float* p = ws + c.frp + (long)(l0 >> 1) * 32;
    f32x16 a0, a1, b0, b1;
    HP_SLOAD16(a0, p, 0x0);
    HP_SLOAD16(a1, p, 0x40);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a0), "+s"(a1));
    for (int l = 0; l < cnt; l += 4) {
        p += 32;
        HP_SLOAD16(b0, p, 0x0);
        HP_SLOAD16(b1, p, 0x40);
        HP_PIN();
        f2 v = match_entry2<true, false>(sqdist2(FINC(a0, a1, 0) - px2, FINC(a0, a1, 1) - py2, FINC(a0, a1, 2) - pz2), rL, a0, a1);
        if (ok) {
            out[(long)l * c.n] = v.x;
            if (l + 1 < cnt) out[(long)(l + 1) * c.n] = v.y;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(b0), "+s"(b1), "+v"(v));
        p += 32;
        HP_SLOAD16(a0, p, 0x0);
        HP_SLOAD16(a1, p, 0x40);
        HP_PIN();
        v = match_entry2<true, false>(sqdist2(FINC(b0, b1, 0) - px2, FINC(b0, b1, 1) - py2, FINC(b0, b1, 2) - pz2), rL, b0, b1);
        if (ok && l + 2 < cnt) {
            out[(long)(l + 2) * c.n] = v.x;
            if (l + 3 < cnt) out[(long)(l + 3) * c.n] = v.y;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a0), "+s"(a1), "+v"(v));
    }
}

// match-free cost + grad1:  cost_b = sum_{k,l} M(l,k) sqrt(d),  grad1[k] = sum_l M(l,k) (p_k-q_l)/max(|p_k-q_l|,1e-10)
// (approxmatch.cu:215-255, 301-322 without the match tensor).  One lane per k, all l on the scalar path.
template <bool DERIVE>
__global__ __launch_bounds__(kThreads) void emd_cost_grad1_kernel(Ctx c, float* __restrict__ partials, float* __restrict__ grad1) {
    __shared__ float red[kThreads / 64];
    __shared__ float parts[kParts][4][kRowsPerWg];
    const int cloud = emd_wave_prio(blockIdx.y);
    const int lrow = threadIdx.x % kRowsPerWg;
    const int part = __builtin_amdgcn_readfirstlane(threadIdx.x / kRowsPerWg);
    const int k = blockIdx.x * kRowsPerWg + lrow;
    const float* ws = c.ws + (long)cloud * c.per_cloud;
    const bool ok = k < c.n;
    float px = 0.f, py = 0.f, pz = 0.f, rL[kLevels] = {};
    if (ok) load_row_final(ws + c.flp, k, px, py, pz, rL);
    const f2 px2 = splat2(px), py2 = splat2(py), pz2 = splat2(pz);
    f2 cost2 = splat2(0.f), dx2 = splat2(0.f), dy2 = splat2(0.f), dz2 = splat2(0.f);   // even / odd candidates (see rows1_setup)
    auto work = [&](const f32x16& lo, const f32x16& hi) {
        const f2 ex = px2 - FINC(lo, hi, 0), ey = py2 - FINC(lo, hi, 1), ez = pz2 - FINC(lo, hi, 2);   // (x1 - x2), approxmatch.cu:312
        const f2 d2 = sqdist2(ex, ey, ez);       // squares: the sign of the difference does not change a bit
        const f2 mv = match_entry2<true, DERIVE>(d2, rL, lo, hi);
        const f2 w = mv * f2{__builtin_amdgcn_rsqf(fmaxf(d2.x, 1e-20f)), __builtin_amdgcn_rsqf(fmaxf(d2.y, 1e-20f))};
        // M * sqrt(d) as (M / sqrt(d)) * d: the reciprocal root is needed for the gradient anyway (d = 0: w * 0 = 0 = M * sqrt(0))
        cost2 = DERIVE ? __builtin_elementwise_fma(w, d2, cost2)
                       : __builtin_elementwise_fma(mv, f2{__builtin_amdgcn_sqrtf(d2.x), __builtin_amdgcn_sqrtf(d2.y)}, cost2);
        dx2 = __builtin_elementwise_fma(ex, w, dx2);
        dy2 = __builtin_elementwise_fma(ey, w, dy2);
        dz2 = __builtin_elementwise_fma(ez, w, dz2);
    };
    const int cand = c.MP / kParts;
    const float* p = ws + c.frp + (long)part * cand * 16;
    f32x16 a0, a1, b0, b1;
    HP_SLOAD16(a0, p, 0x0);
    HP_SLOAD16(a1, p, 0x40);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a0), "+s"(a1));
    for (int l = 0; l < cand; l += 4) {
        p += 32;
        HP_SLOAD16(b0, p, 0x0);
        HP_SLOAD16(b1, p, 0x40);
        HP_PIN();
        work(a0, a1);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(b0), "+s"(b1), "+v"(cost2), "+v"(dx2), "+v"(dy2), "+v"(dz2));
        p += 32;
        HP_SLOAD16(a0, p, 0x0);
        HP_SLOAD16(a1, p, 0x40);
        HP_PIN();
        work(b0, b1);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a0), "+s"(a1), "+v"(cost2), "+v"(dx2), "+v"(dy2), "+v"(dz2));
    }
    float cost = cost2.x + cost2.y, dx = dx2.x + dx2.y, dy = dy2.x + dy2.y, dz = dz2.x + dz2.y;
    parts[part][0][lrow] = dx;
    parts[part][1][lrow] = dy;
    parts[part][2][lrow] = dz;
    parts[part][3][lrow] = cost;
    __syncthreads();
    if (part == 0) {
#pragma unroll
        for (int q2 = 1; q2 < kParts; ++q2) {
            dx += parts[q2][0][lrow];
            dy += parts[q2][1][lrow];
            dz += parts[q2][2][lrow];
            cost += parts[q2][3][lrow];
        }
        if (ok && grad1) {
            // records in Hilbert order (emd_order_kernel): position k holds the caller's point permL[k]
            const int ko = ws[c.flag] != 0.f ? reinterpret_cast<const int*>(ws + c.permL)[k] : k;
            float* g = grad1 + ((long)cloud * c.n + ko) * 3;
            g[0] = dx;
            g[1] = dy;
            g[2] = dz;
        }
    }
    const float t = hp::block_sum((ok && part == 0) ? cost : 0.f, red);
    if (threadIdx.x == 0) partials[(long)cloud * gridDim.x + blockIdx.x] = t;
}

// match-free grad2[l] = sum_k M(l,k) (q_l-p_k)/max(|q_l-p_k|,1e-10)   (approxmatch.cu:260-300); with WITH_COST the
// same sweep also yields the cost (sum over the same pairs, owned by l instead of k), so a training step that only
// needs d cost / d xyz2 evaluates the match entries once.
template <bool WITH_COST, int R, bool DERIVE>
__global__ __launch_bounds__(kThreads) void emd_grad2_kernel(Ctx c, float* __restrict__ grad2, float* __restrict__ partials) {
    __shared__ float red[kThreads / 64];
    __shared__ float parts[kParts][4][kRowsPerWg * R];
    const int cloud = blockIdx.y;
    const int lrow = threadIdx.x % kRowsPerWg;
    const int part = __builtin_amdgcn_readfirstlane(threadIdx.x / kRowsPerWg);
    const float* ws = c.ws + (long)cloud * c.per_cloud;
    // thr1 / thr2: the underflow radii of levels 1 and 2 where the forward that wrote the records culled those levels (3e38: that
    // tier is off), from the flag block.  Only with the records in Hilbert order: the boxes exist and mean something.  (Loaded,
    // not derived in the kernel: as compile-time constants the radii cost up to two VGPRs.)
    auto uniform = [](float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); };
    const float thr1 = uniform(ws[c.flag + 1]), thr2 = uniform(ws[c.flag + 2]);
    const bool tiers = ws[c.flag] != 0.f && thr1 < 1e38f;
    int l[R];
    bool ok[R];
    float rR[R][kLevels];
    float tlo[R][3], thi[R][3];
    f2 qx2[R], qy2[R], qz2[R], sx2[R], sy2[R], sz2[R], cost2[R];   // sums: even / odd candidates (see rows1_setup)
#pragma unroll
    for (int r = 0; r < R; ++r) {
        l[r] = (blockIdx.x * R + r) * kRowsPerWg + lrow;
        ok[r] = l[r] < c.m;
        float qx = 0.f, qy = 0.f, qz = 0.f;
#pragma unroll
        for (int lev = 0; lev < kLevels; ++lev) rR[r][lev] = 0.f;
        if (ok[r]) load_row_final(ws + c.frp, l[r], qx, qy, qz, rR[r]);
        qx2[r] = splat2(qx);
        qy2[r] = splat2(qy);
        qz2[r] = splat2(qz);
        sx2[r] = sy2[r] = sz2[r] = cost2[r] = splat2(0.f);
        if (tiers) load_tile_box(ws + c.tileR, c.MP / kTile, blockIdx.x * R + r, tlo[r], thi[r]);
    }
    unsigned long long far1[R], far2[R];      // per candidate block of the current chunk: beyond level 1's radius / level 2's
    auto work = [&](const f32x16& lo, const f32x16& hi, int bi) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const f2 ex = qx2[r] - FINC(lo, hi, 0), ey = qy2[r] - FINC(lo, hi, 1), ez = qz2[r] - FINC(lo, hi, 2);
            const f2 d2 = sqdist2(ex, ey, ez);
            f2 mv;
            if ((far2[r] >> bi) & 1ull) mv = match_entry2<false, DERIVE, 3>(d2, rR[r], lo, hi);
            else if ((far1[r] >> bi) & 1ull) mv = match_entry2<false, DERIVE, 2>(d2, rR[r], lo, hi);
            else mv = match_entry2<false, DERIVE, 0>(d2, rR[r], lo, hi);
            const f2 w = mv * f2{__builtin_amdgcn_rsqf(fmaxf(d2.x, 1e-20f)), __builtin_amdgcn_rsqf(fmaxf(d2.y, 1e-20f))};
            if (WITH_COST)
                cost2[r] = DERIVE ? __builtin_elementwise_fma(w, d2, cost2[r])      // (M / sqrt(d)) * d, see emd_cost_grad1_kernel
                                  : __builtin_elementwise_fma(mv, f2{__builtin_amdgcn_sqrtf(d2.x), __builtin_amdgcn_sqrtf(d2.y)}, cost2[r]);
            sx2[r] = __builtin_elementwise_fma(ex, w, sx2[r]);
            sy2[r] = __builtin_elementwise_fma(ey, w, sy2[r]);
            sz2[r] = __builtin_elementwise_fma(ez, w, sz2[r]);
        }
    };
    const int cand = c.NP / kParts, nblk = cand / kBlk;      // this wave's candidates: blocks [part * nblk, (part + 1) * nblk) of set1
    const int NB = c.NP / kBlk;
    const float* bb = ws + c.blkL;
    const int lane = threadIdx.x & 63;
    const float* p = ws + c.flp + (long)part * cand * 16;
    f32x16 a0, a1, b0, b1;
    HP_SLOAD16(a0, p, 0x0);
    HP_SLOAD16(a1, p, 0x40);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a0), "+s"(a1));
    for (int ch = 0; ch < nblk; ch += 64) {
#pragma unroll
        for (int r = 0; r < R; ++r) far1[r] = far2[r] = 0ull;
        if (tiers) {
            const bool valid = ch + lane < nblk;
            const int g = valid ? part * nblk + ch + lane : 0;
            const float cx0 = bb[g], cy0 = bb[NB + g], cz0 = bb[2 * NB + g], cx1 = bb[3 * NB + g], cy1 = bb[4 * NB + g], cz1 = bb[5 * NB + g];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float g2 = box_gap2(tlo[r], thi[r], cx0, cy0, cz0, cx1, cy1, cz1);
                far1[r] = __ballot(valid && g2 > thr1);
                far2[r] = __ballot(valid && g2 > thr2);
            }
        }
        const int nb = min(64, nblk - ch);
        for (int bi = 0; bi < nb; ++bi) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {      // a block = 8 candidates = four pair records
                p += 32;
                HP_SLOAD16(b0, p, 0x0);
                HP_SLOAD16(b1, p, 0x40);
                HP_PIN();
                work(a0, a1, bi);
                asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(b0), "+s"(b1), "+v"(sx2[0]), "+v"(sy2[0]), "+v"(sz2[0]), "+v"(cost2[0]),
                             "+v"(sx2[R - 1]), "+v"(sy2[R - 1]), "+v"(sz2[R - 1]), "+v"(cost2[R - 1]));
                p += 32;
                HP_SLOAD16(a0, p, 0x0);
                HP_SLOAD16(a1, p, 0x40);
                HP_PIN();
                work(b0, b1, bi);
                asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a0), "+s"(a1), "+v"(sx2[0]), "+v"(sy2[0]), "+v"(sz2[0]), "+v"(cost2[0]),
                             "+v"(sx2[R - 1]), "+v"(sy2[R - 1]), "+v"(sz2[R - 1]), "+v"(cost2[R - 1]));
            }
        }
    }
    float sx[R], sy[R], sz[R], cost[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        sx[r] = sx2[r].x + sx2[r].y;
        sy[r] = sy2[r].x + sy2[r].y;
        sz[r] = sz2[r].x + sz2[r].y;
        cost[r] = cost2[r].x + cost2[r].y;
        parts[part][0][r * kRowsPerWg + lrow] = sx[r];
        parts[part][1][r * kRowsPerWg + lrow] = sy[r];
        parts[part][2][r * kRowsPerWg + lrow] = sz[r];
        parts[part][3][r * kRowsPerWg + lrow] = cost[r];
    }
    __syncthreads();
    float total = 0.f;
    if (part == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int q2 = 1; q2 < kParts; ++q2) {   // candidate ranges in ascending order
                sx[r] += parts[q2][0][r * kRowsPerWg + lrow];
                sy[r] += parts[q2][1][r * kRowsPerWg + lrow];
                sz[r] += parts[q2][2][r * kRowsPerWg + lrow];
                cost[r] += parts[q2][3][r * kRowsPerWg + lrow];
            }
            if (ok[r]) {
                const int lo = ws[c.flag] != 0.f ? reinterpret_cast<const int*>(ws + c.permR)[l[r]] : l[r];   // see emd_cost_grad1_kernel
                float* g = grad2 + ((long)cloud * c.m + lo) * 3;
                if (c.acc_scale != 0.f) {   // hp_emd_forward_acc: the caller's running gradient (+= coef * this term)
                    g[0] = __builtin_fmaf(c.acc_scale, sx[r], g[0]);
                    g[1] = __builtin_fmaf(c.acc_scale, sy[r], g[1]);
                    g[2] = __builtin_fmaf(c.acc_scale, sz[r], g[2]);
                } else {
                    g[0] = sx[r];
                    g[1] = sy[r];
                    g[2] = sz[r];
                }
                total += cost[r];
            }
        }
    }
    if (WITH_COST) {
        const float t = hp::block_sum(total, red);
        if (threadIdx.x == 0) partials[(long)cloud * gridDim.x + blockIdx.x] = t;
    }
}

// pairs: the call's pair list (hp_emd_pairs) — a pair outside [0,na) x [0,nb) ran on clamped indices and gets NaN —, or ab == NULL
__global__ __launch_bounds__(256) void emd_cost_finish_kernel(const float* __restrict__ partials, int per_cloud, float* __restrict__ out,
                                                              PairList pairs) {
    __shared__ double red[4];
    const float* p = partials + (long)emd_wave_prio(blockIdx.x) * per_cloud;
    double s = 0;
    for (int i = threadIdx.x; i < per_cloud; i += 256) s += (double)p[i];
    const double t = hp::block_sum(s, red);
    if (threadIdx.x == 0) {
        bool valid = true;
        if (pairs.ab) {
            const int a = pairs.ab[2 * (long)blockIdx.x], b = pairs.ab[2 * (long)blockIdx.x + 1];
            valid = (unsigned)a < (unsigned)pairs.na && (unsigned)b < (unsigned)pairs.nb;
        }
        out[blockIdx.x] = valid ? (float)t : __builtin_nanf("");
    }
}

// final_remainL: also run phase 3 of the last level.  Its only products are the last `match +=` term — which the match pass
// and the cost/gradient sweeps re-evaluate from the final records — and remainL's final value in `temp`: the API path
// (hp_approxmatch_ws) returns that, the match-free training path (hp_emd_forward) has no reader for it and skips the
// launch (one of 28 exponential sweeps, 55 us at B=64, N=2048).
// The level sweeps of `b` clouds as a sequence of launches on one stream, one step at a time: step 0 = the record set-up,
// step 1 = phase 1 of level 0, then per level phase 2 and the merged phase-3 / next-phase-1 launch.  Stepwise so that two
// chains (emd_forward_impl) can be ENQUEUED alternately: the host then feeds both streams at the same pace and the chains
// run side by side from the first launch to the last (enqueued one after the other, the second chain trailed the first by
// the host's ~0.2 ms of launch calls and ran its last sweeps alone on a half-empty chip).
struct LevelChain {
    Ctx c;
    int b;
    hipStream_t stream;
    bool final_remainL;
    float multiL, multiR;
    int rows1_r, rows2_r;
    int cull;                      // > 0: records in Hilbert order, sweeps of levels < cull skip the units that are exactly zero
    bool compact = false;          // the plain sweeps over the live set2 points (emd_compact_kernel behind phase 2 of levels j0..7)
    int j0 = 0;                    // the first compacted level: the last culled one (0 without culling)
    int rows2c_r = 1;              // rows per lane of the compacted phase-2 sweeps
    bool lds_feed = false;         // ... and their candidates staged in LDS (emd_rows2_kernel, FEED 1): sets of up to kFeedMaxNP points
    // Round 9, the fused compaction (fused_scan): no emd_compact_kernel.  Phase 2 of level jf - 1 leaves the first list, phase 2 of
    // levels jf .. 7 read one list and leave the next and the candidates of the merged launch behind them, phase 2 of level 8 reads
    // the last.  With culling jf is the last culled level, as j0 (the culling kernel there takes its rows' slots from the list);
    // without, a list can only exist behind level 0, so jf = 1 and the merged launch (0, 1) sweeps every point.
    bool fused = false;
    int jf = 0;
    int logpL = 0, logpR = 0;      // log2 of the order kernel's sort sizes
    PairList pl;                   // the pair list of the chain's clouds (then c.xyz1 / c.xyz2 are the whole sets), or none

    static int log2_ceil64(int x) {
        int l = 6;
        while ((1 << l) < x) ++l;
        return l;
    }
    float radius2(int lev) const { return lev < cull ? underflow_r2(lev) : 3.0e38f; }
    dim3 grid(int rows, int r) const { return dim3((rows + r * kRowsPerWg - 1) / (r * kRowsPerWg), b); }
    // the list-driven phase-2 launches: the cloud in x, the row tile in y (emd_rows2_kernel, PLACEMENT)
    dim3 grid_listed(int rows, int r) const { return dim3(b, (rows + r * kRowsPerWg - 1) / (r * kRowsPerWg)); }

    // cs: the compaction scratch of the chain's first cloud (CsLayout), or NULL (no compaction)
    LevelChain(int b_, int n, int m, const float* xyz1, const float* xyz2, float* temp, float* ws, float* cs, hipStream_t st, bool frl,
               const EmdSwitches& sw, const PairList& pl_ = {})
        : c(make_ctx(n, m, xyz1, xyz2, temp, ws)), b(b_), stream(st), final_remainL(frl), cull(sw.cull), pl(pl_) {
        // (phase 3 of the last level, final_remainL, would need the list of level 9; the row tiles are a grid's y: grid_listed)
        if (cs && sw.compact && !frl && (m + kRowsPerWg - 1) / kRowsPerWg <= 65535) {
            compact = true;
            set_compact_scratch(c, cs);
        }
        const bool want_fused = compact && sw.compact == 2 && c.MP <= kFusedMaxMP;
        multi_lr(n, m, &multiL, &multiR);
        logpL = log2_ceil64(n);
        logpR = log2_ceil64(m);
        if (logpL > kOrderMaxLog || logpR > kOrderMaxLog) cull = 0;
        // rows per lane: the most that still leaves >= 2 waves per SIMD on the chip (measured at B=64, N=2048 on the whole
        // step: phase 1/3 kernel best at 2 — 4 costs occupancy it needs —, phase 2 at 4: -0.10 ms together; tools/emd_rows_sweep.sh).
        // hp_emd_set_rows_per_lane (or HP_EMD_ROWS1_R / HP_EMD_ROWS2_R at load time) overrides: every instance is a
        // per-row-identical evaluation (tests/test_structural_losses_gpu.py compares them bit for bit and with the oracle).
        auto pick = [&](int rows, int cap) {
            for (int r = cap; r > 1; r >>= 1)
                if (fills_chip(b, rows, r)) return r;
            return 1;
        };
        rows1_r = sw.rows1 ? sw.rows1 : pick(n, 2);
        rows2_r = sw.rows2 ? sw.rows2 : pick(m, 4);
        // The list-driven phase-2 sweeps have a fraction of the rows (0.45 .. 0.02 of them from level 3 on at the bench operating point,
        // profiles/r07_emd_alive_share.json): one row per lane, i.e. the most workgroups, spread over the chip by grid_listed.  While the
        // live workgroups sat two deep on a few XCDs (rounds 7-11) one row or two made no difference (-0.017 ms per step, per pair
        // -0.074 .. +0.027: profiles/r07_bench_ab.md); placed over the whole chip, one row measures -0.026 ms against two under the
        // scalar feed (per pair -0.032 .. -0.020) and -0.048 with the LDS feed (profiles/r12_bench_ab.md).
        rows2c_r = sw.rows2 ? sw.rows2 : 1;
        lds_feed = sw.rows2_feed == 1 && c.NP <= kFeedMaxNP;
        j0 = std::max(cull, 1) - 1;
        jf = std::max(cull - 1, 1);
        fused = want_fused && jf + 1 < kLevels;      // (every level culled: nothing is compacted in either form)
    }

    // phase 3 of level lev3 (D3) merged with phase 1 of level lev1 (D1)
    template <bool D3, bool D1>
    void rows1(int lev3, int lev1) const {
        const float l2e3 = D3 ? level_l2e(lev3) : 0.f, l2e1 = D1 ? level_l2e(lev1) : 0.f;
        // (lev3 < lev1.  A launch whose phase-1 level is past the culling levels visits every block anyway, and then the plain
        // kernel's straight pipeline is faster than skipping half of the phase-3 terms: measured)
        const int clev = D1 ? lev1 : lev3;
        if (cull > 0 && clev < cull) {
            const float t3 = D3 ? radius2(lev3) : 0.f, t1 = D1 ? radius2(lev1) : 0.f;
            hipLaunchKernelGGL((emd_rows1_cull_kernel<D3, D1>), grid(c.n, 1), dim3(kThreads), 0, stream, c, lev1, l2e3, l2e1, t3, t1);
            return;
        }
        // the candidates emd_compact_kernel left behind phase 2 of lev3
        // (the compacted R = 4 instance needs 79 VGPRs against the plain one's 67: 6 waves per SIMD instead of 7; the size heuristic
        // caps rows1 at 2, so only a forced rows1 = 4 runs it)
        const bool compacted = D3 && D1 && compact && lev3 >= (fused ? jf : j0);
        with_rows(rows1_r, [&](auto r) {
            constexpr int R = decltype(r)::value;
            if (compacted) hipLaunchKernelGGL((emd_rows1_kernel<true, true, R, true>), grid(c.n, R), dim3(kThreads), 0, stream, c, lev1, l2e3, l2e1);
            else hipLaunchKernelGGL((emd_rows1_kernel<D3, D1, R>), grid(c.n, R), dim3(kThreads), 0, stream, c, lev1, l2e3, l2e1);
        });
    }
    // a list-driven phase-2 launch (MODE 1 / 2) under the chain's candidate feed
    template <int R, int MODE>
    void rows2_listed(int lev, int li) const {
        if (lds_feed) hipLaunchKernelGGL((emd_rows2_kernel<R, MODE, 1>), grid_listed(c.m, R), dim3(kThreads), 0, stream, c, lev, level_l2e(lev), li);
        else hipLaunchKernelGGL((emd_rows2_kernel<R, MODE, 0>), grid_listed(c.m, R), dim3(kThreads), 0, stream, c, lev, level_l2e(lev), li);
    }
    void rows2(int lev) const {
        if (cull > 0 && lev < cull) {
            const dim3 g = grid(c.m, 1);
            if (fused && lev == jf) hipLaunchKernelGGL(emd_rows2_cull_kernel<2>, g, dim3(kThreads), 0, stream, c, lev, level_l2e(lev), radius2(lev));
            else if (fused && lev == jf - 1) hipLaunchKernelGGL(emd_rows2_cull_kernel<1>, g, dim3(kThreads), 0, stream, c, lev, level_l2e(lev), radius2(lev));
            else hipLaunchKernelGGL(emd_rows2_cull_kernel<0>, g, dim3(kThreads), 0, stream, c, lev, level_l2e(lev), radius2(lev));
            return;
        }
        if (fused && lev >= jf - 1) {      // the first list behind level jf - 1 (= 0 here), then list to list; the last level leaves none
            const bool first = lev == jf - 1;
            with_rows(first ? rows2_r : rows2c_r, [&](auto r) {
                constexpr int R = decltype(r)::value;
                if (first) hipLaunchKernelGGL((emd_rows2_kernel<R, 3>), grid(c.m, R), dim3(kThreads), 0, stream, c, lev, level_l2e(lev), 1);
                else rows2_listed<R, 2>(lev, lev + 1 < kLevels ? 1 : 0);
            });
            return;
        }
        // compacted: the rows of list (lev - 1 - j0) & 1: L_lev, written behind phase 2 of lev - 1
        const bool compacted = compact && lev > j0;
        const int li = compacted ? (lev - 1 - j0) & 1 : 0;
        with_rows(compacted ? rows2c_r : rows2_r, [&](auto r) {
            constexpr int R = decltype(r)::value;
            if (compacted) rows2_listed<R, 1>(lev, li);
            else hipLaunchKernelGGL((emd_rows2_kernel<R, 0>), grid(c.m, R), dim3(kThreads), 0, stream, c, lev, level_l2e(lev), li);
        });
    }
    // behind phase 2 of level lev (j0 <= lev < 8): L_{lev+1} into list (lev - j0) & 1, the candidates of the next merged launch
    void compact_after(int lev) const {
        hipLaunchKernelGGL(emd_compact_kernel, dim3(b), dim3(kCompactThreads), 0, stream, c, lev == j0 ? 1 : 0, (lev - 1 - j0) & 1,
                           (lev - j0) & 1);
    }
    static constexpr int kSteps = 2 + 2 * kLevels;
    void step(int s) const {
        if (s == 0) {
            if (cull > 0) {
                const int lp = std::max(logpL, logpR);
                const size_t lds = ((size_t)18 << lp) + kCells * 4;    // per point x, y, z + cell, slot, order (u16); the cell histogram
                if (lds > 48 * 1024)
                    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(emd_order_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                hipLaunchKernelGGL(emd_order_kernel, dim3(2, b), dim3(kOrderThreads), lds, stream, c, multiL, multiR, logpL, logpR, cull, pl);
            } else {
                hipLaunchKernelGGL(emd_init_kernel, dim3(((c.NP + c.MP + 2 * kSpare) / 2 + 255) / 256, b), dim3(256), 0, stream, c, multiL, multiR, pl);
            }
        } else if (s == 1) {
            rows1<false, true>(0, 0);
        } else {
            const int lev = (s - 2) >> 1;
            if (((s - 2) & 1) == 0) {
                rows2(lev);
                if (compact && !fused && lev >= j0 && lev + 1 < kLevels) compact_after(lev);
            } else if (lev + 1 < kLevels) rows1<true, true>(lev, lev + 1);
            else if (final_remainL) rows1<true, false>(lev, lev);
        }
    }
};

int run_levels(int b, int n, int m, const float* xyz1, const float* xyz2, float* temp, float* ws, float* cs, Ctx* out, hipStream_t stream,
               bool final_remainL, const EmdSwitches& sw, const PairList& pl = {}) {
    const LevelChain ch(b, n, m, xyz1, xyz2, temp, ws, cs, stream, final_remainL, sw, pl);
    for (int s = 0; s < LevelChain::kSteps; ++s) ch.step(s);
    *out = ch.c;
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Workspace-free path: the reference launcher's exact prototype (structural_loss.cpp:11), for callers that own
// nothing but `match` and `temp`.  It keeps the reference's data flow (approxmatch.cu:34-213): the four vectors of
// `temp` are the only state, every phase re-reads the other set's points and one of those vectors through a 16 KB LDS
// tile, phase 3 read-modify-writes `match` once per level.  One lane per row; a row's sum runs over the candidates in
// ascending order in one fp32 accumulator — the reference's per-thread order (:77-93,:125-137,:177-189), which also
// makes this path comparable with the CPU oracle term by term.  ~2.5x the time of the record-based path at B=64,
// N=2048 (it moves the 18 GB the reference moves); a binding that can allocate scratch calls hp_approxmatch_ws.
// ------------------------------------------------------------------------------------------------
constexpr int kPlainTile = 1024;

__global__ __launch_bounds__(kThreads) void emd_plain_init_kernel(int n, int m, float* __restrict__ temp, float multiL, float multiR) {
    float* remL = temp + (long)blockIdx.y * (n + m) * 2;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n + m; i += gridDim.x * kThreads) remL[i] = i < n ? multiL : multiR;
}

// PHASE 1: rows = set1, ratioL[k] = remainL[k] / (1e-9 + sum_l e * remainR[l])                     (:60-93)
// PHASE 2: rows = set2, sumr = remainR[l] * sum_k e * ratioL[k]; ratioR / remainR update            (:109-142)
// PHASE 3: rows = set1, w = (e * ratioL[k]) * ratioR[l]; match[l,k] += w; remainL[k] -= sum_l w    (:161-194)
template <int PHASE>
__global__ __launch_bounds__(kThreads) void emd_plain_kernel(int n, int m, const float* __restrict__ xyz1, const float* __restrict__ xyz2,
                                                             float* __restrict__ temp, float* __restrict__ match, float l2e, int first) {
    __shared__ float4 tile[kPlainTile];
    const int cloud = blockIdx.y, tid = threadIdx.x;
    float* remL = temp + (long)cloud * (n + m) * 2;
    float* remR = remL + n;
    float* ratioL = remR + m;
    float* ratioR = ratioL + n;
    constexpr bool kRowsL = PHASE != 2;
    const int rows = kRowsL ? n : m, cands = kRowsL ? m : n;
    const float* R = (kRowsL ? xyz1 : xyz2) + (long)cloud * rows * 3;
    const float* C = (kRowsL ? xyz2 : xyz1) + (long)cloud * cands * 3;
    const float* cw = PHASE == 1 ? remR : PHASE == 2 ? ratioL : ratioR;
    const int row = blockIdx.x * kThreads + tid;
    const bool ok = row < rows;
    float rx = 0.f, ry = 0.f, rz = 0.f, rl = 0.f;
    if (ok) {
        rx = R[row * 3];
        ry = R[row * 3 + 1];
        rz = R[row * 3 + 2];
        if (PHASE == 3) rl = ratioL[row];
    }
    float sum = PHASE == 1 ? 1e-9f : 0.f;
    float* mcol = match + (long)cloud * m * n + row;
    for (int c0 = 0; c0 < cands; c0 += kPlainTile) {
        const int cnt = min(kPlainTile, cands - c0);
        for (int t = tid; t < cnt; t += kThreads) {
            const float* s = C + (long)(c0 + t) * 3;
            tile[t] = make_float4(s[0], s[1], s[2], cw[c0 + t]);
        }
        __syncthreads();
        if (ok) {
#pragma unroll 4
            for (int t = 0; t < cnt; ++t) {
                const float4 c = tile[t];
                // (x2 - x1) with x2 the set2 point in every phase (approxmatch.cu:85,131,185)
                const float d = kRowsL ? hp::sqdist(c.x - rx, c.y - ry, c.z - rz) : hp::sqdist(rx - c.x, ry - c.y, rz - c.z);
                const float e = __builtin_amdgcn_exp2f(l2e * d);
                // products enter the sums through an fma (nvcc's default -fmad=true contraction of the reference source;
                // oracle `contract` variant 3), as in the packed-record sweeps
                if (PHASE == 3) {
                    const float er = e * rl;
                    float* mp = mcol + (long)(c0 + t) * n;
                    *mp = first ? er * c.w : __builtin_fmaf(er, c.w, *mp);   // level 0 writes (zero fill + first `+=`)
                    sum = __builtin_fmaf(er, c.w, sum);
                } else {
                    sum = __builtin_fmaf(e, c.w, sum);
                }
            }
        }
        __syncthreads();
    }
    if (!ok) return;
    if (PHASE == 1) {
        ratioL[row] = remL[row] / sum;
    } else if (PHASE == 2) {
        const float rr = remR[row];
        const float sumr = sum * rr;
        const float consumption = fminf(rr / (sumr + 1e-9f), 1.0f);
        ratioR[row] = consumption * rr;
        remR[row] = fmaxf(0.0f, rr - sumr);
    } else {
        remL[row] = fmaxf(0.0f, remL[row] - sum);
    }
}

}  // namespace

// ---- tuning hook (no counterpart in the reference) -------------------------------------------------
// Rows per lane of the three sweep families: rows1 (phase 3 + phase 1 kernel) in {0,1,2,4}, rows2 (phase 2) in
// {0,1,2,4}, grad2 (final cost/gradient sweep) in {0,1,2}; 0 = the size heuristic.  Process-wide; every instance
// evaluates each row with the same operations in the same order, so results do not depend on the setting.
HP_API int hp_emd_set_rows_per_lane(int rows1, int rows2, int grad2) {
    auto okv = [](int v, bool four) { return v == 0 || v == 1 || v == 2 || (four && v == 4); };
    HP_CHECK_ARG(okv(rows1, true) && okv(rows2, true) && okv(grad2, false));
    g_rows1.set(rows1);
    g_rows2.set(rows2);
    g_grad2.set(grad2);
    return 0;
}

// The training path's final cost / gradient sweep with four of its nine exponentials per pair derived (1, default) or all nine
// from v_exp_f32 (0); returns the previous setting.  `match` as hp_approxmatch* return it is never derived.
HP_API int hp_emd_set_final_derive(int on) { return g_final_derive.set(on); }

// hp_emd_forward* / hp_emd_forward_acc: the records in Hilbert order and the sweeps of the first `levels` annealing levels skipping
// the (64-row tile, 8-candidate block) units whose terms are all exactly zero (emd_order_kernel, emd_rows*_cull_kernel); 0 = the
// caller's point order, every unit evaluated (rounds 1-5).  Default 3 (HP_EMD_CULL at load time).  Returns the previous setting.
HP_API int hp_emd_set_cull(int levels) {
    HP_CHECK_ARG(levels >= -1 && levels <= kLevels);
    return g_cull.set(levels);
}

// hp_emd_forward* / hp_emd_forward_acc: the plain level sweeps over the set2 points that can still add a non-zero term — listed by
// the phase-2 launches themselves (2, default: fused_scan; sets of up to 4096 points, otherwise as 1) or by emd_compact_kernel behind
// each of them (1) — or over every point (0: rounds 1-6).  Bit-identical results.  Values above 2 count as 2.  Returns the previous
// setting.
HP_API int hp_emd_set_compact(int on) { return g_compact.set(on); }

// hp_emd_forward* / hp_emd_forward_acc: the candidates of the list-driven phase-2 sweeps (hp_emd_set_compact 1 and 2) on the scalar
// path (0) or staged in LDS by the workgroup (1, default; set1 of up to 2048 points, larger ones run as 0).  Bit-identical results.
// Returns the previous setting.
HP_API int hp_emd_set_rows2_feed(int feed) { return g_rows2_feed.set(feed); }

// hp_emd_forward* as two chains of half the clouds on two streams (2, default) or as one chain (1); returns the previous setting.
HP_API int hp_emd_set_chains(int chains) {
    HP_CHECK_ARG(chains == -1 || (chains >= 1 && chains <= kMaxChains));
    return g_chains.set(chains);
}

// replaces approxmatch(...)  structural_loss.cpp:11 / approxmatch.cu:330-338 — the reference's exact argument list:
// match (b,m,n) and temp (b,2(n+m)) are the only buffers.  temp ends as cloud i's [remainL | remainR | ratioL | ratioR].
HP_API int hp_approxmatch(int b, int n, int m, const float* xyz1, const float* xyz2, float* match, float* temp, hipStream_t stream) {
    HP_CHECK_ARG(b >= 0 && n > 0 && m > 0);
    if (b == 0) return 0;
    HP_CHECK_ARG(xyz1 && xyz2 && match && temp && b <= 65535);
    float multiL, multiR;
    multi_lr(n, m, &multiL, &multiR);
    const dim3 blk(kThreads), gL((n + kThreads - 1) / kThreads, b), gR((m + kThreads - 1) / kThreads, b);
    hipLaunchKernelGGL(emd_plain_init_kernel, dim3((n + m + kThreads - 1) / kThreads, b), blk, 0, stream, n, m, temp, multiL, multiR);
    for (int lev = 0; lev < kLevels; ++lev) {
        const float l2e = level_l2e(lev);
        hipLaunchKernelGGL(emd_plain_kernel<1>, gL, blk, 0, stream, n, m, xyz1, xyz2, temp, match, l2e, 0);
        hipLaunchKernelGGL(emd_plain_kernel<2>, gR, blk, 0, stream, n, m, xyz1, xyz2, temp, match, l2e, 0);
        hipLaunchKernelGGL(emd_plain_kernel<3>, gL, blk, 0, stream, n, m, xyz1, xyz2, temp, match, l2e, lev == 0);
    }
    HP_RETURN_LAST_ERROR();
}

// floats of scratch hp_approxmatch_ws / hp_emd_forward need besides `temp` (packed candidate records)
HP_API long hp_approxmatch_workspace_floats(int b, int n, int m) { return (long)b * ws_layout(n, m).per_cloud; }

// The same result through the packed-record sweeps (the fast path): `ws` is scratch of
// hp_approxmatch_workspace_floats floats; `match` is written once instead of read-modify-written nine times.
HP_API int hp_approxmatch_ws(int b, int n, int m, const float* xyz1, const float* xyz2, float* match, float* temp, float* ws,
                             hipStream_t stream) {
    HP_CHECK_ARG(b >= 0 && n > 0 && m > 0);
    if (b == 0) return 0;
    HP_CHECK_ARG(xyz1 && xyz2 && match && temp && ws && b <= 65535);
    Ctx c;
    EmdSwitches sw = read_switches();
    sw.cull = 0;      // `match` and `temp` leave in the caller's order
    int rc = run_levels(b, n, m, xyz1, xyz2, temp, ws, nullptr, &c, stream, true, sw);
    if (rc) return rc;
    hipLaunchKernelGGL(emd_match_kernel, dim3((n + kThreads - 1) / kThreads, (m + kLT - 1) / kLT, b), dim3(kThreads), 0, stream, c,
                       match);
    HP_RETURN_LAST_ERROR();
}

// Match-free EMD forward (what match_cost's forward = ApproxMatch + MatchCost computes, match_cost.py:9-27):
// cost (b,) and, as a by-product of the same sweep, grad1 = d cost / d xyz1 (b,n,3) (may be NULL).
// `ws` keeps the packed records for hp_emd_backward; partials: the final sweep's per-workgroup costs (b*ceil(max(n,m)/64) floats),
// then the compaction scratch of every cloud (CsLayout).
HP_API long hp_emd_partials_floats(int b, int n, int m) { return cost_partials_floats(b, n, m) + (long)b * cs_layout(m).per_cloud; }

// grad1 / grad2 (either may be NULL): gradients to produce in the same call.  With grad2 != NULL the cost rides on the
// grad2 sweep (one evaluation of the match entries serves both); grad1 then costs a second sweep only if requested.
namespace {
int emd_forward_impl(int b, int n, int m, const float* xyz1, const float* xyz2, float* temp, float* ws, float* partials,
                     float* cost, float* grad1, float* grad2, float acc_scale, hipStream_t stream, hipStream_t after, const PairList& pl = {});
}
HP_API int hp_emd_forward(int b, int n, int m, const float* xyz1, const float* xyz2, float* temp, float* ws, float* partials,
                          float* cost, float* grad1, float* grad2, hipStream_t stream) {
    return emd_forward_impl(b, n, m, xyz1, xyz2, temp, ws, partials, cost, grad1, grad2, 0.f, stream, nullptr);
}

// The training step's form: grad2_acc (b,m,3) already holds the other loss terms' gradient with respect to xyz2 (the Chamfer
// term, written on stream `after`, or NULL = same stream) and receives  += scale * d cost / d xyz2  from the gradient sweep
// itself — the caller's separate `g_rec.add_(g_emd, alpha=scale)` launch (core/epoch_loops.py:26-31 forms the sum through
// autograd) is gone.  The sweep launch is ordered behind everything enqueued on `after` so far; scale != 0.
HP_API int hp_emd_forward_acc(int b, int n, int m, const float* xyz1, const float* xyz2, float* temp, float* ws, float* partials,
                              float* cost, float* grad2_acc, float scale, hipStream_t stream, hipStream_t after) {
    HP_CHECK_ARG(grad2_acc && scale != 0.f);
    return emd_forward_impl(b, n, m, xyz1, xyz2, temp, ws, partials, cost, nullptr, grad2_acc, scale, stream, after);
}

namespace {
// emd_grad2_kernel over the b clouds of `c` (partials: WITH_COST).  Rows per lane: `rows` (hp_emd_set_rows_per_lane), else two
// when that still leaves >= 2 waves per SIMD (as in LevelChain; -0.01 ms in the forward's final sweep at B=64, N=2048, and
// round 6's backward took 465 us at one row per lane against ~250 at two).  Returns the row blocks per cloud of the grid.
template <bool WITH_COST>
int launch_grad2(const Ctx& c, int b, float* grad2, float* partials, int rows, bool derive, hipStream_t stream) {
    const int r = rows ? rows : fills_chip(b, c.m, 2) ? 2 : 1;
    const dim3 grid((c.m + r * kRowsPerWg - 1) / (r * kRowsPerWg), b);
    with_rows<2>(r, [&](auto rc) {
        constexpr int R = decltype(rc)::value;
        if (derive) hipLaunchKernelGGL((emd_grad2_kernel<WITH_COST, R, true>), grid, dim3(kThreads), 0, stream, c, grad2, partials);
        else hipLaunchKernelGGL((emd_grad2_kernel<WITH_COST, R, false>), grid, dim3(kThreads), 0, stream, c, grad2, partials);
    });
    return (int)grid.x;
}
// emd_cost_grad1_kernel over the b clouds of `c`
void launch_cost_grad1(const Ctx& c, int b, float* partials, float* grad1, bool derive, hipStream_t stream) {
    const dim3 grid((c.n + kRowsPerWg - 1) / kRowsPerWg, b);
    if (derive) hipLaunchKernelGGL(emd_cost_grad1_kernel<true>, grid, dim3(kThreads), 0, stream, c, partials, grad1);
    else hipLaunchKernelGGL(emd_cost_grad1_kernel<false>, grid, dim3(kThreads), 0, stream, c, partials, grad1);
}

// the cost / gradient sweep(s) of the b clouds of `c` behind their level sweeps
// (pairs: the whole call's pair list, for the NaN of an out-of-range pair)
int emd_final_sweep(Ctx c, int b, float* partials, float* cost, float* grad1, float* grad2, float acc_scale, hipStream_t stream,
                    hipStream_t after, const EmdSwitches& sw, const PairList& pairs) {
    const int n = c.n;
    int rc = 0;
    c.acc_scale = acc_scale;
    if (after && after != stream) {   // the accumulated-into gradient was written on `after`: order the sweep behind it
        rc = hp_order_streams(after, stream);
        if (rc) return rc;
    }
    const int nb = (n + kRowsPerWg - 1) / kRowsPerWg;
    if (grad2) {
        const int gb = launch_grad2<true>(c, b, grad2, partials, sw.grad2, sw.derive, stream);
        hipLaunchKernelGGL(emd_cost_finish_kernel, dim3(b), dim3(256), 0, stream, partials, gb, cost, pairs);
        // (the second sweep's partials are unused: cost was already reduced, in stream order, by the finish kernel)
        if (grad1) launch_cost_grad1(c, b, partials, grad1, sw.derive, stream);
    } else {
        launch_cost_grad1(c, b, partials, grad1, sw.derive, stream);
        hipLaunchKernelGGL(emd_cost_finish_kernel, dim3(b), dim3(256), 0, stream, partials, nb, cost, pairs);
    }
    HP_RETURN_LAST_ERROR();
}

// Round 5: the clouds are independent, but a launch is not — each of the 19 dependent launches pays its ramp, prologue, epilogue
// and tail with every wave of the chip in lockstep (at B = 64 the grid is ONE round of workgroups), ~8 us per launch that the
// same launches on several times the clouds amortise (tools/emd_launch_bound.py: 1.371 ms at 64 clouds, 1.217 per 64 at 576).
// So the call runs as TWO chains of half the clouds on two streams: while one chain's launch ramps up or drains, the other's
// waves hold the vector pipes — what a persistent per-cloud kernel would give, without a flag hand-off and without anything that
// could wait for a workgroup the dispatcher has not placed (docs/DESIGN_HISTORY.md 7b).  Per cloud the arithmetic is that of one chain
// (the halves may run other rows-per-lane instances, which are bit-identical per row): match-free cost within the partials'
// regrouping (2e-6, as between instances), gradients identical.  Measured at B = 64, N = 2048: 1.370 -> 1.280 ms per call.
// The second stream is the library's own, one per device, created on first use (non-blocking, high priority: its own hardware
// queue).  HP_EMD_CHAINS=1 / hp_emd_set_chains(1): one chain (rounds 1-4).

// The library's own stream number `i` (1..kMaxChains-1) on the device `stream` belongs to (the null stream: the current device).
// Created on first use on THAT device — the calling thread's current device may be another one — non-blocking, high
// priority: its own hardware queue.
hipStream_t chain_stream(hipStream_t stream, int i) {
    int cur = 0, dev = 0;
    if (hipGetDevice(&cur) != hipSuccess) return nullptr;
    dev = cur;
    if (stream && hipStreamGetDevice(stream, &dev) != hipSuccess) {
        (void)hipGetLastError();
        dev = cur;
    }
    std::lock_guard<std::mutex> lock(g_s2_mu);
    auto it = g_s2_streams.find(dev * kMaxChains + i);
    if (it != g_s2_streams.end()) return it->second;
    hipStream_t s = nullptr;
    if (dev == cur || hipSetDevice(dev) == hipSuccess) {
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);      // (numerically lowest = highest priority)
        if (hipStreamCreateWithPriority(&s, hipStreamNonBlocking, hi) != hipSuccess) {
            (void)hipGetLastError();
            s = nullptr;
        }
        if (dev != cur) (void)hipSetDevice(cur);
    } else {
        (void)hipGetLastError();
    }
    g_s2_streams[dev * kMaxChains + i] = s;
    return s;
}

int emd_forward_impl(int b, int n, int m, const float* xyz1, const float* xyz2, float* temp, float* ws, float* partials,
                     float* cost, float* grad1, float* grad2, float acc_scale, hipStream_t stream, hipStream_t after, const PairList& pl) {
    HP_CHECK_ARG(b >= 0 && n > 0 && m > 0);
    if (b == 0) return 0;
    HP_CHECK_ARG(xyz1 && xyz2 && temp && ws && partials && cost && b <= 65535);
    const EmdSwitches sw = read_switches();
    // several chains only where each part still fills the chip (>= 2 waves per SIMD at one row per lane) and a capture is not in
    // progress on the caller's stream (a captured call stays on the stream it was captured on)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(stream, &cap);
    int nch = cap == hipStreamCaptureStatusNone ? sw.chains : 1;
    while (nch > 1 && !fills_chip(b / nch, std::min(n, m), 1)) --nch;
    hipStream_t st[kMaxChains] = {stream};
    for (int i = 1; i < nch; ++i) {
        st[i] = chain_stream(stream, i);
        if (!st[i]) nch = 1;
    }
    float* cs = partials + cost_partials_floats(b, n, m);      // the compaction scratch, cloud by cloud
    const long cs_per_cloud = cs_layout(m).per_cloud;
    if (nch <= 1) {      // ONE chain: the 18 level sweeps + the final sweep, launch behind launch on `stream`
        Ctx c;
        const int rc = run_levels(b, n, m, xyz1, xyz2, temp, ws, cs, &c, stream, false, sw, pl);   // temp is scratch here
        return rc ? rc : emd_final_sweep(c, b, partials, cost, grad1, grad2, acc_scale, stream, after, sw, pl);
    }
    const WsLayout L = ws_layout(n, m);
    int rc = 0;
    for (int i = 1; i < nch && !rc; ++i) rc = hp_order_streams(stream, st[i]);      // the inputs are ready on `stream`
    if (rc) return rc;      // (nothing is enqueued on the library's streams yet)
    std::vector<LevelChain> ch;
    ch.reserve(nch);
    for (int i = 0; i < nch; ++i) {
        const int c0 = (int)((long)b * i / nch), c1 = (int)((long)b * (i + 1) / nch);
        // (a chain of the pair form keeps the whole sets and starts its pair list at c0)
        const long s1 = pl.ab ? 0 : (long)c0 * n * 3, s2 = pl.ab ? 0 : (long)c0 * m * 3;
        ch.emplace_back(c1 - c0, n, m, xyz1 + s1, xyz2 + s2, temp + (long)c0 * (n + m) * 2, ws + (long)c0 * L.per_cloud,
                        cs + c0 * cs_per_cloud, st[i], false, sw, PairList{pl.ab ? pl.ab + 2L * c0 : nullptr, pl.na, pl.nb});
    }
    for (int s = 0; s < LevelChain::kSteps; ++s)      // alternately: all streams are fed at the same pace
        for (int i = 0; i < nch; ++i) ch[i].step(s);
    rc = (int)hipGetLastError();
    // the final sweep is ONE launch over all clouds again, behind every chain: it is a single long launch (nothing follows it that
    // could cover its tail), and as two half-size launches the second ran its last ~110 us alone on a half-empty chip
    // (173 + 284 us in the trace against 288 for the whole batch)
    // ... and behind `after` (the stream that wrote the gradient the sweep accumulates into).  Every wait costs the waiting stream a
    // bubble of several microseconds even when the event has long fired, so the caller's stream gets as few as possible: `after` is
    // joined into the last chain's stream first (nothing is queued there behind its chain), the library's streams into one
    // another, and the last one into the caller's.
    const bool ext = after && after != stream && acc_scale != 0.f;
    if (!rc && ext) rc = hp_order_streams(after, st[nch - 1]);
    // On a failure the library's streams are still joined into the caller's (best effort): the caller only knows `stream` and may
    // free or reuse temp / ws / the inputs behind it.
    for (int i = 1; i + 1 < nch; ++i) {
        const int r2 = hp_order_streams(st[i], st[i + 1]);
        if (!rc) rc = r2;
    }
    const int r3 = hp_order_streams(st[nch - 1], stream);
    if (!rc) rc = r3;
    if (rc) return rc;
    Ctx call = ch[0].c;      // the whole batch: chain 0 starts at cloud 0
    return emd_final_sweep(call, b, partials, cost, grad1, grad2, acc_scale, stream, ext ? nullptr : after, sw, pl);
}

}  // namespace

// The match-free cost over a LIST of cloud pairs: cost[p] is what hp_emd_forward writes for cloud p of the batch
// (A[pair_ab[p][0]], B[pair_ab[p][1]]) — the raw match cost, not divided by n — without that batch ever being gathered: the set-up
// kernels (emd_init_kernel / emd_order_kernel) take their source clouds through the pair list and are the only readers of A and B;
// the level sweeps, the chains and the final cost sweep run on the records as for hp_emd_forward(b = pairs), so the bits are its
// bits under the same switches.  No gradients.  temp / ws / partials: hp_emd_forward's at b = pairs.  A pair outside
// [0,na) x [0,nb) reads nothing out of bounds and costs NaN (hp_cloud_pairs' convention); the other pairs are unaffected.
HP_API int hp_emd_pairs(int na, int n, const float* A, int nb, int m, const float* B, int pairs, const int* pair_ab, float* temp,
                        float* ws, float* partials, float* cost, hipStream_t stream) {
    HP_CHECK_ARG(na > 0 && n > 0 && nb > 0 && m > 0 && pairs >= 0);
    if (pairs == 0) return 0;
    HP_CHECK_ARG(A && B && pair_ab && temp && ws && partials && cost && pairs <= 65535);
    return emd_forward_impl(pairs, n, m, A, B, temp, ws, partials, cost, nullptr, nullptr, 0.f, stream, nullptr, PairList{pair_ab, na, nb});
}

// grad2 = d cost / d xyz2 (b,m,3) from the records hp_emd_forward left in `ws` (match_cost.py:35-46 without match)
HP_API int hp_emd_backward(int b, int n, int m, const float* xyz1, const float* xyz2, const float* ws, float* grad2,
                           hipStream_t stream) {
    HP_CHECK_ARG(b >= 0 && n > 0 && m > 0);
    if (b == 0) return 0;
    HP_CHECK_ARG(ws && grad2 && b <= 65535);
    const Ctx c = make_ctx(n, m, xyz1, xyz2, nullptr, const_cast<float*>(ws));
    // (the tiers of the sweep follow the cull the workspace was built under: emd_grad2_kernel reads it there)
    launch_grad2<false>(c, b, grad2, nullptr, g_grad2.get(), g_final_derive.get() != 0, stream);
    HP_RETURN_LAST_ERROR();
}
