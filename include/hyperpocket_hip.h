/*
 * hyperpocket_hip.h — C ABI of libhyperpocket_hip.so (gfx950 / MI355X only).
 *
 * The drop-in boundary for the HyperPocket training-step hot path of
 * gmum/3d-point-clouds-autocomplete.  Plain pointers and sizes; every pointer is a DEVICE
 * pointer unless stated; `stream` is a hipStream_t (NULL = the null stream).  All entry points
 *   - are asynchronous on `stream`, never allocate, free or synchronise (safe under hipGraph
 *     capture; the caller owns every buffer, as the reference binding does with torch::empty —
 *     structural_loss.cpp:32-33,49,64-65,90-93,111-112),
 *   - fully initialise their outputs (callers pass uninitialised memory),
 *   - return 0 on success, -1 on an invalid argument, otherwise the hipError_t of the launch
 *     (the reference throws std::runtime_error("CUDA kernel failed : <code>"),
 *      approxmatch.cu:334-337; its nndistance launchers check nothing, nndistance.cu:131-160).
 * Layouts are the reference's: point sets (b, n, 3) fp32 contiguous, indices int32.
 *
 * TEST HOOKS.  hp_nn_set_queries_per_lane, hp_emd_set_rows_per_lane, hp_emd_set_final_derive, hp_emd_set_chains, hp_emd_set_cull, hp_emd_set_compact, hp_emd_set_rows2_feed, hp_encoder_backward_set_fused, hp_encoder_backward_set_chain_f16, hp_hypernet_set_heads_stream, hp_conv_split_set, hp_skinny_set_enabled,
 * hp_skinny_programs_run (a read-only counter, not a switch),
 * hp_target_fused_set_f16 (and hp_conv_presplit_set below) flip PROCESS-WIDE switches that select between implementations of
 * the same result; they exist so that the parity tests can hold every implementation against the oracle in one process.
 * A production caller never needs them: the defaults are the measured-fastest paths.
 * The switch contract: each switch is an atomic, process-wide value (not per stream or thread), read once from the environment
 * variable named at its hook when the library loads (HP_NN_QUERIES_PER_LANE, HP_EMD_ROWS1_R / HP_EMD_ROWS2_R / HP_EMD_GRAD2_R, HP_EMD_FINAL_DERIVE,
 * HP_EMD_CHAINS, HP_EMD_CULL, HP_EMD_COMPACT, HP_EMD_ROWS2_FEED, HP_ENC_BWD_FUSED, HP_EB_CHAIN16, HP_HEADS_FWD, HP_CONV_SPLIT, HP_CONV_PRESPLIT, HP_SKINNY,
 * HP_TARGET_F16; a value outside the switch's range is ignored).  An entry point reads each switch it depends on once, at entry,
 * so a call runs one consistent combination even if another thread flips a switch meanwhile.  hp_emd_backward follows the
 * workspace: it culls as the hp_emd_forward* call that built `ws` did, whatever hp_emd_set_cull says now.  A one-argument hook
 * returns the previous setting; -1 restores the load-time value.
 */
#ifndef HYPERPOCKET_HIP_H
#define HYPERPOCKET_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* hpStream_t; /* == hipStream_t */

/* ------------------------------------------------------------------------------------------
 * Structural losses — the five launchers the reference's pybind module binds
 * (utils/pytorch_structural_losses/structural_loss.cpp:11-15).
 * ------------------------------------------------------------------------------------------ */

/* nndistance  (structural_loss.cpp:14, nndistance.cu:131-134)
 * result[i,j]  = min_k |xyz[i,j]-xyz2[i,k]|^2, result_i = arg min (smallest k on ties); and the
 * mirrored result2/result2_i over xyz2's points. */
int hp_nndistance(int b, int n, const float* xyz, int m, const float* xyz2, float* result, int* result_i,
                  float* result2, int* result2_i, hpStream_t stream);

/* nn_distance_kernel comes in three instances, R = 1, 2 or 4 query points per lane, picked from (b, n, m) alone; each evaluates
 * every query with the same operations in the same order (distances and indices identical bit for bit;
 * tests/test_nn_instances_gpu.py).  The hook forces one for hp_nndistance AND hp_chamfer_forward: 1, 2 or 4 = that instance at
 * any size, 0 = the size heuristic (default; environment HP_NN_QUERIES_PER_LANE at load time), a negative value restores the
 * load-time value.  Returns the previous setting; any other value returns -1 and leaves the setting alone.  Read once per call. */
/* [test hook: process-wide switch — see the header comment] */
int hp_nn_set_queries_per_lane(int r);
/* The R the size heuristic picks for (b, n, m), whatever the hook says.  Host only (no HIP call). */
int hp_nn_queries_per_lane(int b, int n, int m);

/* nndistancegrad  (structural_loss.cpp:15, nndistance.cu:155-160) */
int hp_nndistancegrad(int b, int n, const float* xyz1, int m, const float* xyz2, const float* grad_dist1,
                      const int* idx1, const float* grad_dist2, const int* idx2, float* grad_xyz1, float* grad_xyz2,
                      hpStream_t stream);

/* approxmatch  (structural_loss.cpp:11, approxmatch.cu:330-338) — the reference's exact argument list.
 * match (b, m, n), temp (b, 2*(n+m)) as in the reference; no other buffer.  Keeps the reference's data flow (the
 * four vectors of temp are the only state, match is read-modify-written once per level) on a chip-wide grid. */
int hp_approxmatch(int b, int n, int m, const float* xyz1, const float* xyz2, float* match, float* temp,
                   hpStream_t stream);
/* The same result ~2.5x faster for a caller that can allocate: `ws` = scratch of
 * hp_approxmatch_workspace_floats(b,n,m) floats (packed candidate records incl. the per-level scaling vectors; lets
 * `match` be written once instead of read-modify-written nine times).  What this repo's Python binding calls. */
long hp_approxmatch_workspace_floats(int b, int n, int m);
int hp_approxmatch_ws(int b, int n, int m, const float* xyz1, const float* xyz2, float* match, float* temp, float* ws,
                      hpStream_t stream);
/* Tuning hook (no counterpart in the reference): rows per lane of the packed-record sweeps — rows1 (phase 3 + phase 1
 * kernel) and rows2 (phase 2) in {0,1,2,4}, grad2 (final cost/gradient sweep) in {0,1,2}; 0 = the size heuristic (environment
 * HP_EMD_ROWS1_R / HP_EMD_ROWS2_R / HP_EMD_GRAD2_R at load time).  Returns 0.  Every setting evaluates each row with the same operations in the same order (results identical bit
 * for bit; tests/test_structural_losses_gpu.py). */
/* [test hook: process-wide switch — see the header comment] */
int hp_emd_set_rows_per_lane(int rows1, int rows2, int grad2);
/* The match-free cost / gradient sweep (hp_emd_forward*, hp_emd_backward) evaluates the nine per-level exponentials of a point
 * pair; the levels are exact powers of 4 apart, so four of them can be formed as the fourth power of their neighbour's (two
 * multiplies instead of v_exp_f32; ~5 ulp instead of 1 on a value nothing is downstream of).  1 (default; environment
 * HP_EMD_FINAL_DERIVE=0 turns it off at load time): derived; 0: all nine from the hardware exponential.  Returns the previous
 * setting.  The level sweeps and the `match` tensor hp_approxmatch / hp_approxmatch_ws return are never derived. */
/* [test hook: process-wide switch — see the header comment] */
int hp_emd_set_final_derive(int on);
/* hp_emd_forward / hp_emd_forward_acc run the clouds as TWO chains of launches — the first half of the batch on the caller's
 * stream, the second half on a stream the library owns (one per device, created on first use), ordered behind everything the
 * caller's stream held at the call and joined back into it before the call returns control of the stream: to the caller it is one
 * asynchronous call on `stream`, as before.  While one chain's launch ramps up or drains, the other's waves hold the vector pipes
 * (B = 64, N = 2048: 1.37 -> 1.28 ms).  Used when each half still fills the chip and `stream` is not being captured; per cloud the
 * results are those of one chain (gradients identical, cost within the 2e-6 of the partial sums' grouping).  2 (default;
 * environment HP_EMD_CHAINS=1 at load time): two chains; 1: one.  Returns the previous setting. */
/* [test hook: process-wide switch — see the header comment] */
int hp_emd_set_chains(int chains);
/* hp_emd_forward / hp_emd_forward_acc put both point sets in a Hilbert order first (one workgroup per cloud and set; a counting sort
 * over 16^3 Hilbert cells, so runs of consecutive positions are compact boxes) and the sweeps of the first `levels` annealing levels skip every (64-row tile, 8-candidate
 * block) unit whose bounding boxes are further apart than the level's underflow radius (d^2 > 152 ln2 / |level|: each of its
 * exponentials is exactly +0 in fp32, so each skipped term of approxmatch.cu:86-87,131-132,185-189 is an exact zero).  Results:
 * the sums of the caller's order with their zero terms left out, accumulated in the Hilbert order (cost within 3e-7 of the same
 * kernels on the caller's order); gradients are written through the permutation, so callers keep their own point order.
 * levels in 0..9; 0 = the caller's order, every unit evaluated (rounds 1-5).  Default 3 (environment HP_EMD_CULL at load time).
 * Sets of more than 4096 points always run in the caller's order.  hp_approxmatch / hp_approxmatch_ws (whose `match` and `temp`
 * are returned in the caller's order) are never re-ordered.  Returns the previous setting. */
/* [test hook: process-wide switch — see the header comment] */
int hp_emd_set_cull(int levels);
/* hp_emd_forward / hp_emd_forward_acc: once a set2 point's remainR is clamped to exactly +0 (the point is oversubscribed,
 * approxmatch.cu:141) it only adds exact zeros, so behind each plain level's phase-2 sweep one workgroup per cloud lists the points
 * still alive and compacts the next sweeps' candidates per (candidate range, parity) class, in order; the plain sweeps then run over
 * those alone.  Every row sums the same non-zero terms in the same order: cost, gradients, temp and the records are bit-identical
 * to the full sweeps.  The lists live in `partials` (hp_emd_partials_floats).  1: compacted, by emd_compact_kernel behind each
 * phase-2 launch; 0: every point (rounds 1-6).  2 (default; environment HP_EMD_COMPACT = 0..2 at load time): FUSED, the same
 * without the compaction launches — each phase-2 workgroup leaves its rows that stay alive in its own segment of the row list (-1
 * in the unused slots) and each row writes its record into a slot fixed by the list the launch started from (a superset of mode 1's
 * candidates: the extra ones carry zero weights), and the next phase-2 launch scans the list in its prologue; same scratch, same
 * bits.  Fused applies to sets of up to 4096 points (MP <= 4096); larger ones run as 1.  Values above 2 count as 2; -1 restores the
 * load-time value.  hp_approxmatch / hp_approxmatch_ws never compact.  Returns the previous setting. */
/* [test hook: process-wide switch — see the header comment] */
int hp_emd_set_compact(int on);
/* The phase-2 sweeps over a row list (hp_emd_set_compact 1 and 2) have a fraction of the full sweep's workgroups, too few waves to cover
 * the round trips of candidate records fetched on the scalar path.  1 (default; environment HP_EMD_ROWS2_FEED=0 at load time): each
 * workgroup stages the cloud's set1 records in LDS once (32 KB at n = 2048) and its waves read them from there; sets of more than
 * 2048 (padded) points run as 0.  0: the scalar path.  The same terms in the same order: results identical bit for bit
 * (tests/test_emd_rows2_feed_gpu.py).  Values above 1 count as 1; -1 restores the load-time value.  Returns the previous setting. */
/* [test hook: process-wide switch — see the header comment] */
int hp_emd_set_rows2_feed(int feed);

/* Match-free EMD (what match_cost.py:9-46 computes through ApproxMatch + MatchCost + MatchCostGrad, without ever
 * writing the (b,m,n) match tensor): cost (b,) plus whichever of grad1 = d cost/d xyz1, grad2 = d cost/d xyz2 the
 * caller asks for (the cost rides on one of those sweeps); hp_emd_backward computes grad2 later from the packed
 * records hp_emd_forward left in `ws` (hp_approxmatch_workspace_floats).
 * partials: hp_emd_partials_floats floats (the final sweep's partial costs, then the compaction scratch of every cloud; query it,
 * its size is not part of the contract).  temp: scratch of hp_approxmatch's size (its remainL block is left one level
 * short: the last level's phase 3 has no reader on this path and is not launched); ws as in hp_approxmatch_ws. */
long hp_emd_partials_floats(int b, int n, int m);
int hp_emd_forward(int b, int n, int m, const float* xyz1, const float* xyz2, float* temp, float* ws, float* partials,
                   float* cost, float* grad1 /* or NULL */, float* grad2 /* or NULL */, hpStream_t stream);
/* The training step's form of hp_emd_forward: grad2_acc (b,m,3) already holds the gradient of the other loss terms with respect
 * to xyz2 (written on stream `after`; NULL = the same stream) and receives += scale * d cost / d xyz2 from the gradient sweep
 * itself (no separate axpy launch); the sweep is ordered behind everything enqueued on `after` so far.  scale != 0. */
int hp_emd_forward_acc(int b, int n, int m, const float* xyz1, const float* xyz2, float* temp, float* ws, float* partials,
                       float* cost, float* grad2_acc, float scale, hpStream_t stream, hpStream_t after);
int hp_emd_backward(int b, int n, int m, const float* xyz1, const float* xyz2, const float* ws, float* grad2,
                    hpStream_t stream);

/* matchcost  (structural_loss.cpp:12, approxmatch.cu:340-347) — the reference's exact argument list: one
 * 1024-thread workgroup per cloud, ordered sums, no scratch. */
int hp_matchcost(int b, int n, int m, const float* xyz1, const float* xyz2, const float* match, float* out,
                 hpStream_t stream);
/* The same sum chip-wide in two ordered stages for a caller that can allocate `partials`
 * (hp_matchcost_workspace_floats floats): 5.9 TB/s at B=64, N=2048 instead of one workgroup per cloud. */
long hp_matchcost_workspace_floats(int b, int n, int m);
int hp_matchcost_ws(int b, int n, int m, const float* xyz1, const float* xyz2, const float* match, float* out,
                    float* partials, hpStream_t stream);

/* matchcostgrad  (structural_loss.cpp:13, approxmatch.cu:349-357) */
int hp_matchcostgrad(int b, int n, int m, const float* xyz1, const float* xyz2, const float* match, float* grad1,
                     float* grad2, hpStream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused Chamfer loss — replaces losses/champfer_loss.py:11-35 (ChamferLoss.forward and its
 * autograd backward) without materialising the (b, n, m) distance tensor.
 * ------------------------------------------------------------------------------------------ */
/* `partials` of hp_chamfer_forward, in floats: sized for one query per lane, so valid under every hp_nn_set_queries_per_lane
 * setting. */
long hp_chamfer_workspace_floats(int b, int n, int m);
int hp_chamfer_forward(int b, int n, const float* preds, int m, const float* gts, float* dist1, int* idx1,
                       float* dist2, int* idx2, float* partials, float* loss /* 1 float */, hpStream_t stream);
int hp_chamfer_backward(int b, int n, const float* preds, int m, const float* gts, const int* idx1, const int* idx2,
                        const float* grad_loss /* device scalar */, float* grad_preds, float* grad_gts,
                        hpStream_t stream);

/* ------------------------------------------------------------------------------------------
 * Nearest-neighbour reductions over a list of cloud pairs — the completion metrics (UHD, TMD,
 * all-pairs MMD, completeness; the reference computes them on the CPU in utils/evaluation/).
 * A (na, n, 3), B (nb, m, 3); pair_ab (pairs, 2) int32 holds (a, b) = (index into A, index into B).
 * Per-point minima are those of hp_nndistance, bit for bit (same direct-difference fma chain).
 *   HP_PAIRS_CHAMFER    out (pairs, 2) = ( sum_i min_j |A[a]_i - B[b]_j|^2 ,  sum_j min_i |A[a]_i - B[b]_j|^2 )
 *                       (fp64 sums of the fp32 minima, rounded once)
 *   HP_PAIRS_HAUSDORFF  out (pairs)    = max_i min_j |A[a]_i - B[b]_j|^2          (A -> B only)
 *   HP_PAIRS_COVERED    out (pairs)    = #{ i : sqrt(min_j |A[a]_i - B[b]_j|^2) < thres }  (A -> B only, exact)
 * Deterministic (no atomics).  `ws`: hp_cloud_pairs_workspace_floats(mode, n, m, pairs) floats, 8-byte aligned.
 * Sizes, NULLs and the mode are checked (-1); pairs == 0 is a no-op; a pair whose index lies outside [0, na) x [0, nb)
 * gets NaN in its outputs.  P is not limited by a grid dimension.
 * ------------------------------------------------------------------------------------------ */
#define HP_PAIRS_CHAMFER 0
#define HP_PAIRS_HAUSDORFF 1
#define HP_PAIRS_COVERED 2
long hp_cloud_pairs_workspace_floats(int mode, int n, int m, long pairs);
/* The launch plan hp_cloud_pairs uses for (mode, n, m, pairs): *r = query points per lane of the kernel instance (1, 2 or 4),
 * *group = pairs per workgroup (1, 2, 4 or 8).  Host only (no HIP call); either pointer may be NULL; -1 on a bad mode or size. */
int hp_cloud_pairs_plan(int mode, int n, int m, long pairs, int* r, int* group);
int hp_cloud_pairs(int mode, int na, int n, const float* A, int nb, int m, const float* B, long pairs,
                   const int* pair_ab, float thres, float* ws, float* out, hpStream_t stream);

/* ------------------------------------------------------------------------------------------
 * Match-free EMD over a list of cloud pairs — the distance matrices of the generative metrics
 * (MMD / coverage / 1-NN accuracy, EMD half) without a gathered or expanded copy of any cloud.
 * A (na, n, 3), B (nb, m, 3); pair_ab (pairs, 2) int32 holds (a, b) = (index into A, index into B).
 *   cost (pairs): cost[p] is what hp_emd_forward writes for cloud p of the batch (A[pair_ab[p][0]], B[pair_ab[p][1]]) —
 *   the raw match cost, not divided by n — bit for bit under the same hp_emd_set_* switches: only the set-up kernels
 *   read A and B, through the pair list; the level sweeps, the chains and the cost sweep are hp_emd_forward's at
 *   b = pairs.  No gradients.  n != m is allowed (hp_approxmatch's multiL / multiR rule).
 * Buffers, all scratch: temp pairs * (n + m) * 2 floats, ws hp_approxmatch_workspace_floats(pairs, n, m) floats,
 * partials hp_emd_partials_floats(pairs, n, m) floats.
 * Sizes, NULLs and pairs > 65535 (a grid dimension, as for hp_emd_forward; callers chunk) are checked (-1) before any HIP
 * call; pairs == 0 is a no-op; a pair whose index lies outside [0, na) x [0, nb) reads nothing out of bounds and gets
 * NaN as its cost, the other pairs are unaffected.
 * ------------------------------------------------------------------------------------------ */
int hp_emd_pairs(int na, int n, const float* A, int nb, int m, const float* B, int pairs, const int* pair_ab,
                 float* temp, float* ws, float* partials, float* cost, hpStream_t stream);

/* ------------------------------------------------------------------------------------------
 * Occupancy-grid histograms of a set of clouds — the device half of the generativity evaluation's
 * JSD (the reference: utils/metrics.py:279-318, sklearn NearestNeighbors on the CPU and a Python
 * loop over every point).  clouds (S, n, 3); a grid of R centres per axis, of which `cells` are kept
 * (all R^3, or those inside the sphere of radius 0.5), numbered row-major over (i, j, k).
 *   counters[c]   = number of points, over all clouds, whose nearest kept centre is c
 *   clouds_hit[c] = number of clouds with at least one such point
 *   *nonfinite    = non-zero if a coordinate was NaN/Inf (such points are counted nowhere)
 * "Nearest" is the Euclidean distance evaluated in fp64 on the fp32 values: the result is that of an
 * exhaustive fp64 arg-min over the kept centres.  Exactly equal distances: the lower (i, j) column wins,
 * inside a column the k nearest to the point.  All three
 * outputs are int32, zeroed by the call on `stream`; integer sums, so bit-identical run to run.
 * The grid comes from the host (hyperpocket_amd.utils.metrics builds it with numpy):
 *   axis (R) fp32 centre coordinates of one axis, ascending;
 *   columns (R*R) one word per (i, j): the kept cells of the column are k in [klo, khi] and their kept
 *   indices base + (k - klo); packed klo | khi << 6 | base << 12, klo > khi for an empty column.
 * Checked before any HIP call (-1): NULLs, S < 1, n < 1, R < 2, R > HP_OCCUPANCY_MAX_R,
 * cells outside [1, R^3], S * n >= 2^31.  S is not limited by a grid dimension.
 * ------------------------------------------------------------------------------------------ */
#define HP_OCCUPANCY_MAX_R 64
int hp_occupancy_grid(int S, int n, const float* clouds, int R, const float* axis, const unsigned int* columns,
                      int cells, int* counters, int* clouds_hit, int* nonfinite, hpStream_t stream);
/* The kernel's cell decision run on the host (one source for both sides), all pointers host memory: cell_out[i] = kept
 * index of the centre nearest to points[i] (count, 3), -1 for a non-finite point.  For checks without a GPU. */
int hp_occupancy_cells_host(long count, const float* points, int R, const float* axis, const unsigned int* columns,
                            int* cell_out);

/* ------------------------------------------------------------------------------------------
 * fp32 matrix-core GEMM family (v_mfma_f32_32x32x2_f32) — the dense contractions PyTorch/cuBLAS
 * perform for the reference's nn.Conv1d(k=1)/nn.Linear/torch.mm calls (model/encoder.py:14-36,
 * model/hyper_network.py:16-43, model/target_network.py:31-38) and their autograd backward.
 *   C[z](i,j) = epi( sum_k A[z](i,k) B[z](k,j) );  epi = (+bias[j]) (+add(i,j)) (ReLU) (*(mask(i,j)>0))
 * ------------------------------------------------------------------------------------------ */
#define HP_GEMM_BIAS 1
#define HP_GEMM_RELU 2
#define HP_GEMM_MASK 4
#define HP_GEMM_ADD 8
#define HP_GEMM_ROWSUM 32 /* also rsum(i) = sum_k A(i,k): the bias gradient rides on the dW = dY^T X contraction */
#define HP_GEMM_COLMAX 16 /* do not store C: per row-tile column max (+bias) and its row -> cmax/cidx (fused max-pool) */

typedef struct HpGemmDesc {
    const float* A;    /* A(i,k) at A + z*sAz + i*sAi + k*sAk (one of sAi,sAk is 1) */
    const float* B;    /* B(k,j) at B + z*sBz + k*sBk + j*sBj (one of sBk,sBj is 1) */
    float* C;          /* C(i,j) at C + z*sCz + i*ldc + j                           */
    const float* bias; /* bias(j) at bias + z*sBiasz + j                            */
    const float* mask; /* mask(i,j) at mask + z*sMaskz + i*ldmask + j               */
    const float* add;  /* add(i,j) at add + z*sAddz + i*ldadd + j                   */
    float* ws;         /* split-K slabs: hp_gemm_workspace_floats(desc) floats       */
    long sAz, sBz, sCz, sBiasz, sMaskz, sAddz;
    long sAi, sAk, sBk, sBj;
    int ldc, ldmask, ldadd;
    int M, N, K, batch;
    int ksplit; /* <=1: no split; >1: ordered (atomic-free) split-K through `ws` */
    int flags;
    /* HP_GEMM_COLMAX: rows come in groups of group_rows (one cloud); cmax/cidx are (M / tile_rows, N) with
     * tile_rows = hp_gemm_tile_rows(desc) dividing group_rows; cidx holds the row index inside its group */
    float* cmax;
    int* cidx;
    int group_rows;
    /* HP_GEMM_ROWSUM: rsum(i) at rsum + z*sRsumz + i ; with split-K the workspace needs batch*ksplit*M more floats */
    float* rsum;
    long sRsumz;
    /* A size known only on the device: dyn_count (device pointer to one int, or NULL) bounds M (dyn_kind 1: rows of
     * A/C beyond it are neither read nor written) or K (dyn_kind 2: the contraction stops there; split-K ranges
     * partition the real K).  M / K of this descriptor stay the static upper bounds the launch is sized for. */
    const int* dyn_count;
    int dyn_kind;
} HpGemmDesc;

long hp_gemm_workspace_floats(const HpGemmDesc* d);
int hp_gemm_tile_rows(const HpGemmDesc* d);
/* Which kernel hp_gemm_f32 would launch for d, answered on the host by the code that launches (no HIP call):
 * *tile = 0: 128x32, 1: 128x128, 2: 64x128, 3: 64x64; *mode = am + 3*bm, the staging loaders of A and B (0 lanes along i/j,
 * 1 16-byte loads along k, 2 4-byte loads along k) after the fall-backs to the instantiated pairs: 0, 1, 2, 3, 4, 7 or 8.
 * Either output may be NULL; both are -1 for a problem with nothing to do.  0, or -1 where hp_gemm_f32 refuses d. */
int hp_gemm_plan(const HpGemmDesc* d, int* tile, int* mode);
int hp_gemm_f32(const HpGemmDesc* d /* host struct */, hpStream_t stream);
/* out[z][j] = sum_i (mask ? (mask(i,j)>0 ? X(i,j) : 0) : X(i,j))  — bias gradients */
long hp_colsum_workspace_floats(int batch, int M, int N);
int hp_colsum_f32(int batch, int M, int N, const float* X, long sXz, int ldx, const float* mask, long sMaskz,
                  int ldmask, float* out, long sOz, float* ws /* or NULL */, hpStream_t stream);

/* ------------------------------------------------------------------------------------------
 * Model entry points.  Parameter tables hold device pointers to tensors laid out exactly as the
 * reference's nn.Module parameters (row-major (out,in); Conv1d weights (out,in,1)).
 * ------------------------------------------------------------------------------------------ */
#define HP_MAX_HEADS 8
#define HP_MAX_TN_LAYERS 8

typedef struct HpEncoderWeights { /* model/encoder.py:14-36: conv 3-64-128-256-512-512, fc 512, mu/std (out,512) */
    const float* conv_w[5];
    const float* conv_b[5];
    const float* fc_w;
    const float* fc_b;
    const float* mu_w;
    const float* mu_b;
    const float* std_w; /* NULL for a non-VAE encoder */
    const float* std_b;
} HpEncoderWeights;

typedef struct HpEncoderGrads {
    float* conv_w[5];
    float* conv_b[5];
    float* fc_w;
    float* fc_b;
    float* mu_w;
    float* mu_b;
    float* std_w;
    float* std_b;
} HpEncoderGrads;

typedef struct HpHyperWeights { /* model/hyper_network.py:16-36 */
    const float* trunk_w[5];
    const float* trunk_b[5];
    int n_heads;
    int head_out[HP_MAX_HEADS];
    const float* head_w[HP_MAX_HEADS];
    const float* head_b[HP_MAX_HEADS];
} HpHyperWeights;

typedef struct HpHyperGrads {
    float* trunk_w[5];
    float* trunk_b[5];
    float* head_w[HP_MAX_HEADS];
    float* head_b[HP_MAX_HEADS];
} HpHyperGrads;

/* Encoder.forward (model/encoder.py:43-53).  x (B,Np,3) contiguous.  Outputs: argidx/g (B,512) the max-pool
 * arg-max / value, f (B,512) the fc activation, mu (B,out); VAE also lv (raw std_layer output), z = eps*exp(lv)+mu,
 * explv = exp(lv) (what the reference returns as "logvar").  ws: hp_encoder_forward_workspace_floats. */
long hp_encoder_forward_workspace_floats(int B, int Np);
int hp_encoder_forward(int B, int Np, const float* x, const HpEncoderWeights* w, int out_size, int is_vae,
                       const float* eps, int* argidx, float* g, float* f, float* mu, float* lv, float* z, float* explv,
                       float* ws, hpStream_t stream);
/* The two encoders of a HyperPocket step (model/full_model.py:106-112: random_encoder on `missing`, real_encoder on
 * `existing`; same conv stack, own weights) in one call: every conv layer is one batched launch over both.  io[0], io[1]
 * carry hp_encoder_forward's arguments; same B, Np, out_size.  Results are those of two hp_encoder_forward calls. */
typedef struct HpEncoderIO {
    const float* x;
    const HpEncoderWeights* w;
    const float* eps; /* VAE only */
    int* argidx;
    float *g, *f, *mu, *lv, *z, *explv, *ws;
    int is_vae;
    int out_ld; /* row stride of the primary output (z of a VAE encoder, mu of a plain one); 0 = out_size (dense).  The two
                   encoders of a pair can so write the halves of one (B, 2*out) latent [z | real mu] directly */
} HpEncoderIO;
int hp_encoder_forward_pair(int B, int Np, int out_size, const HpEncoderIO* io /* [2] */, hpStream_t stream);
/* Layout of the forward workspace: per-point activations h1..h4 (B*Np rows of 64 | 128 | 256 | 512 channels, 4 bytes per value), the
 * slot of h5 (per-tile maxima, tail slabs), then the split area (weight pieces, exponents).  Since round 4 the fast path (whole
 * 128-point tiles per cloud) stores h1..h4 as f16 piece pairs with block exponents ("P-format", csrc/conv_pp.hip) — the operand
 * format of the next layer's matrix-core launch — and says so in a word of the split area; hp_encoder_backward* read either
 * format.  hp_encoder_workspace_to_f32 converts such a workspace to plain fp32 rows in place (idempotent). */
int hp_encoder_workspace_to_f32(int B, int Np, float* ws, hpStream_t stream);
/* [test hook: process-wide switch — see the header comment] 0: the conv stack takes fp32 activations again (round 3's
 * kernels, csrc/conv_split.hip; also: environment HP_CONV_PRESPLIT=0).  Returns the previous setting. */
int hp_conv_presplit_set(int on);
/* The P-format GEMM as a stand-alone primitive (bench.py's roofline leg, tests): C = act(X W^T + b), X (M,K), W (N,K) fp32, N % 128
 * == 0, K % 32 == 0, K <= 512.  prepare packs X (one exponent per 128 rows x xcb channels) and W into ws
 * (hp_gemm_pp_workspace_floats floats); run is the matrix-core launch alone: mode 0 stores C in P-format inside ws
 * (hp_gemm_pp_unpack -> fp32), mode 1 forms per-128-row-tile column maxima of X W^T + b and their rows (hp_gemm_pp_partials). */
long hp_gemm_pp_workspace_floats(long M, int N, int K);
int hp_gemm_pp_prepare(long M, int N, int K, int xcb, const float* X, const float* W, float* ws, hpStream_t stream);
int hp_gemm_pp_run(long M, int N, int K, int xcb, const float* bias, int relu, int mode, int group_rows, float* ws, hpStream_t stream);
int hp_gemm_pp_unpack(long M, int N, int K, const float* ws, float* C, hpStream_t stream);
int hp_gemm_pp_partials(long M, int N, int K, const float* ws, float* cmax, int* cidx, hpStream_t stream);
/* Host-only query (launches nothing): what hp_gemm_pp_run(mode) of an (M, N) problem — or, with n = 2, the encoder pair's layer
 * of that shape — launches, through the function the launch itself calls.  out = {tile columns bn, tile rows bm, column tiles
 * tiles_n, tiles, persistent workgroups, threads per workgroup}: bn / 128 and threads / 256 name the kernel instance.
 * Non-zero where the launch refuses (N no multiple of bn, mode not 0 / 1, M <= 0). */
int hp_gemm_pp_plan(long M, int N, int mode, int n, int out[6]);
/* Gradients of every encoder parameter (autograd of the above).  grad_out = d/dz (VAE) or d/dmu (plain);
 * grad_mu / grad_explv = direct gradients on the VAE outputs (may be NULL).  Only the 512 arg-max points of a
 * cloud carry gradient below the max-pool: their activations are copied out of fwd_ws (the workspace
 * hp_encoder_forward ran in, untouched since) or, with fwd_ws = NULL, recomputed from x.  dedup != 0: channels that
 * peak at the same point share one row (their gradients add), so the layers below run on the DISTINCT critical
 * points, about a third of B*512; same gradients up to fp32 summation order.
 * fwd_ws is declared const because the call never changes the VALUES it holds, but the layered path (dedup == 0, or the fused
 * path switched off) rewrites their REPRESENTATION in place: hidden activations the forward left in the piece format are
 * converted to fp32 rows and the workspace's format word is updated (as hp_encoder_workspace_to_f32 does).  Consequences for a
 * foreign caller: do not run two backward calls over the same workspace concurrently on different streams, and a workspace
 * not produced by hp_encoder_forward* must carry a valid format word (call hp_encoder_workspace_to_f32 semantics: fp32 rows +
 * the word hp_encoder_forward writes).  The autograd bridge (ops.py) uses each workspace for exactly one backward. */
long hp_encoder_backward_workspace_floats(int B, int out_size);
int hp_encoder_backward(int B, int Np, const float* x, const HpEncoderWeights* w, int out_size, int is_vae,
                        const float* eps, const int* argidx, const float* g, const float* f, const float* lv,
                        const float* grad_out, const float* grad_mu, const float* grad_explv, const HpEncoderGrads* grads,
                        float* ws, const float* fwd_ws, int dedup, hpStream_t stream);
/* ... with grad_out a column block of a wider matrix (row stride grad_out_ld >= out_size). */
int hp_encoder_backward_ld(int B, int Np, const float* x, const HpEncoderWeights* w, int out_size, int is_vae,
                           const float* eps, const int* argidx, const float* g, const float* f, const float* lv,
                           const float* grad_out, int grad_out_ld, const float* grad_mu, const float* grad_explv,
                           const HpEncoderGrads* grads, float* ws, const float* fwd_ws, int dedup, hpStream_t stream);
/* Both encoders of a HyperPocket step in one call, on one stream (round 3): with the forward's workspaces at hand and
 * dedup != 0 the two conv stacks share four launches (sort, a row-block chain delta4 -> delta1 on the matrix cores, one
 * grouped launch for every weight/bias gradient, an ordered reduce — csrc/enc_bwd.hip) and the two fc/mu/std tails three.
 * Results are those of two hp_encoder_backward_ld calls, bit for bit.  Autograd of model/encoder.py:14-53 for
 * model/full_model.py:106-112's two encoders. */
typedef struct HpEncoderBwdIO {
    const float* x;              /* (B, Np, 3) */
    const HpEncoderWeights* w;
    const float* eps;            /* VAE only */
    const int* argidx;
    const float *g, *f, *lv;
    const float *grad_out, *grad_mu, *grad_explv;
    const HpEncoderGrads* gr;
    float* ws;                   /* hp_encoder_backward_workspace_floats */
    const float* fwd_ws;         /* the forward's workspace, or NULL */
    int is_vae;
    int grad_out_ld;
} HpEncoderBwdIO;
int hp_encoder_backward_pair(int B, int Np, int out_size, const HpEncoderBwdIO* io /* [2] */, int dedup, hpStream_t stream);
/* Route query: which launches the encoder calls above take for (B, Np, out_size) with n = 1 (hp_encoder_forward,
 * hp_encoder_backward[_ld]) or n = 2 encoders (the _pair calls) under the current switches — decided by the functions those
 * calls decide with, on the host, without a HIP call.  is_vae[n]; ld[n] (NULL or 0: out_size): the row stride of grad_out,
 * and in a pair of the latent a plain encoder's mu is a column block of; aligned != 0: the forward's workspace is at hand
 * and it, the backward's workspace, the conv weights and their gradients start on 16-byte boundaries; dedup as handed to the
 * backward.  A plain encoder is taken to receive grad_out.  Reports
 *   conv_format       HP_ENC_CONV_PFORMAT (f16 piece pairs stored, whole 128-point tiles), HP_ENC_CONV_SPLIT_F32 (f16 pieces
 *                     formed from fp32 activations) or HP_ENC_CONV_GEMM_F32 (hp_conv_split_set(0))
 *   pool_fused        the max-pool is layer 5's epilogue (per-tile partials of tile_rows rows, then colmax over tiles), else h5 is
 *                     written and reduced per cloud
 *   fwd_tails_skinny  fc / mu / std as skinny layer programs (else GEMM launches)
 *   bwd_fused         the conv stack's backward in the fused launches (else the layered sequence), bwd_splits its row ranges (0 when
 *                     layered)
 *   bwd_tails_skinny  per encoder: the tail's backward as a skinny layer program (else GEMM launches)
 * 0, or -1 for shapes the forward or the backward refuses. */
enum { HP_ENC_CONV_PFORMAT = 0, HP_ENC_CONV_SPLIT_F32 = 1, HP_ENC_CONV_GEMM_F32 = 2 };
typedef struct HpEncoderPlan {
    int conv_format;
    int pool_fused;
    int tile_rows;
    int fwd_tails_skinny;
    int bwd_fused;
    int bwd_splits;
    int bwd_tails_skinny[2];
} HpEncoderPlan;
int hp_encoder_plan(int B, int Np, int out_size, int n, const int* is_vae, const int* ld, int aligned, int dedup,
                    HpEncoderPlan* plan);
/* Parity-test switch: 0 sends every encoder backward through round 2's layered launch sequence (sort, gather, a dX GEMM,
 * a dW GEMM and a split-K reduce per layer), 1 (default; environment HP_ENC_BWD_FUSED) through the fused kernels when fwd_ws != NULL
 * and dedup != 0.  Returns the previous setting. */
/* [test hook: process-wide switch — see the header comment] */
int hp_encoder_backward_set_fused(int on);
/* The fused backward's delta chain (delta4 -> delta1 of the critical rows) and its dW launch run on the f16 matrix pipe with split
 * fp32 operands (csrc/enc_bwd_f16.hip; environment HP_EB_CHAIN16, default 1); 0 selects round 3's fp32 MFMA chain and dW launch.
 * Returns the previous setting. */
/* [test hook: process-wide switch — see the header comment] */
int hp_encoder_backward_set_chain_f16(int on);
/* The encoders' conv stack (model/encoder.py:14-28) runs on the f16 matrix pipe with every fp32 operand split into two
 * f16 pieces (three MFMA products per block; as close to fp64 as the fp32 fma chain — csrc/conv_split.hip).  0 sends it
 * through the fp32 MFMA GEMMs instead (also: environment HP_CONV_SPLIT=0).  Returns the previous setting. */
/* [test hook: process-wide switch — see the header comment] */
int hp_conv_split_set(int on);
/* The same split-f16 GEMM as a stand-alone primitive: C = act(X W^T + b), X (M,K) and W (N,K) fp32 of either sign, row-major;
 * N % 128 == 0, K % 32 == 0, K <= 512.  prepare forms max|X| per 128-row tile and the f16 pieces / per-row exponents of W in ws
 * (hp_gemm_f16x2_workspace_floats(M, N, K) floats — inside the encoder stack the producing layer's epilogue and one prep launch
 * per forward do this); run is the GEMM launch alone (bench.py times it).  relu != 0: max(., 0). */
long hp_gemm_f16x2_workspace_floats(long M, int N, int K);
int hp_gemm_f16x2_prepare(long M, int N, int K, const float* X, const float* W, float* ws, hpStream_t stream);
int hp_gemm_f16x2_run(long M, int N, int K, const float* X, const float* bias, float* C, int relu, const float* ws, hpStream_t stream);

/* The heads' forward (theta = t5 . W^T + b at B <= 64, 156 MB of weights) runs as a streaming kernel on the bf16 matrix pipe with
 * every fp32 operand split into three bf16 pieces (exact split, six products: csrc/heads_fwd.hip; environment HP_HEADS_FWD,
 * default 1); 0 selects the tiled fp32 GEMM + split-K reduce.  Returns the previous setting. */
/* [test hook: process-wide switch — see the header comment] */
int hp_hypernet_set_heads_stream(int on);
/* HyperNetwork.forward (model/hyper_network.py:41-43): latent (B,in) -> theta (B,theta_ld); t = saved trunk
 * activations (hp_hypernet_saved_floats floats) for the backward. */
long hp_hypernet_saved_floats(int B);
int hp_hypernet_forward(int B, int in_size, const float* latent, const HpHyperWeights* w, float* t, float* theta,
                        int theta_ld, hpStream_t stream);
long hp_hypernet_backward_workspace_floats(int B);
int hp_hypernet_backward(int B, int in_size, const float* latent, const HpHyperWeights* w, const float* t,
                         const float* grad_theta, int theta_ld, const HpHyperGrads* grads, float* grad_latent /* or NULL */,
                         float* ws, hpStream_t stream);
/* ... with a second stream `after` (may be NULL) ordered behind the last reader of the heads' weights inside the call (d t5 =
 * d theta . W): an in-place update of those weights enqueued on `after` next (hp_hypernet_heads_dw_adam) starts beside the trunk's
 * backward launches instead of behind the whole call. */
int hp_hypernet_backward_ordered(int B, int in_size, const float* latent, const HpHyperWeights* w, const float* t,
                                 const float* grad_theta, int theta_ld, const HpHyperGrads* grads, float* grad_latent /* or NULL */,
                                 float* ws, hpStream_t stream, hpStream_t after);
/* Data-parallel form of the heads' weight gradient (no counterpart in the reference, which has no distributed code:
 * SURVEY 8e).  grads->head_w[0] == NULL makes hp_hypernet_backward skip dW of the heads (bias gradients and d latent are
 * still produced); ranks then all-gather d theta (B x theta_ld) and t5 (B x 2048, hp_hypernet_t5_offset(B) floats into
 * the forward's `t`) and each forms rows [r0, r0+rows) of the GLOBAL gradient of the (19011 x 2048) heads matrix:
 *   dW_rows = dtheta_all[:, r0:r0+rows]^T . t5_all   (contraction over the Kc = world*B gathered clouds). */
long hp_hypernet_t5_offset(int B);
long hp_hypernet_heads_dw_workspace_floats(void);
int hp_hypernet_heads_dw_rows(int Kc, int rows, int r0, const float* dtheta_all, int theta_ld, const float* t5_all,
                              float* dW_rows, float* ws, hpStream_t stream);
/* Route query: which launches the heads take in hp_hypernet_forward, hp_hypernet_backward[_ordered] and hp_hypernet_heads_dw_rows
 * under the current switch — decided by the functions those calls decide with, on the host, without a HIP call; no pointer is
 * followed except w and grads themselves.  B and t as handed to the forward (the heads read the t5 block of t,
 * hp_hypernet_t5_offset(B) floats in, and the stream kernel lays its t5 pieces behind the saved activations: both inherit t's
 * 16-byte phase).  Reports
 *   fwd_route      HP_HEADS_FWD_STREAM (csrc/heads_fwd.hip: contiguous heads, 1 <= B <= 64, 16 rows or more in all, t and the
 *                  weights on 16-byte boundaries, hp_hypernet_set_heads_stream(1)), HP_HEADS_FWD_GEMM (one GEMM over the contiguous
 *                  heads) or HP_HEADS_FWD_PER_HEAD (a GEMM per head: the heads' weights or biases are not back to back)
 *   dw_route       grads != NULL, the backward's weight gradient: HP_HEADS_DW_DIRECT (csrc/hypernet.hip's fragment-direct kernel:
 *                  weights, biases and their gradients back to back, t and grads->head_w[0] on 16-byte boundaries), HP_HEADS_DW_GEMM
 *                  (one GEMM), HP_HEADS_DW_PER_HEAD, or HP_HEADS_DW_SKIPPED (grads->head_w[0] == NULL: column sums only);
 *                  -1 with grads == NULL
 *   dw_rows_route  dW_rows != NULL, hp_hypernet_heads_dw_rows with t5_all = the t5 block of t: HP_HEADS_DW_DIRECT or
 *                  HP_HEADS_DW_GEMM (t5_all or dW_rows off a 16-byte boundary); -1 with dW_rows == NULL
 * 0, or -1 for what the calls refuse (a skipped dW whose heads or bias gradients are not back to back). */
enum { HP_HEADS_FWD_STREAM = 0, HP_HEADS_FWD_GEMM = 1, HP_HEADS_FWD_PER_HEAD = 2 };
enum { HP_HEADS_DW_DIRECT = 0, HP_HEADS_DW_GEMM = 1, HP_HEADS_DW_PER_HEAD = 2, HP_HEADS_DW_SKIPPED = 3 };
typedef struct HpHeadsPlan {
    int fwd_route;
    int dw_route;
    int dw_rows_route;
} HpHeadsPlan;
int hp_hypernet_heads_plan(int B, const HpHyperWeights* w, const HpHyperGrads* grads /* or NULL */, const float* t,
                           const float* dW_rows /* or NULL */, HpHeadsPlan* plan);

/* The heads' weight gradient AND its torch.optim.Adam update in one pass (no counterpart in the reference: PyTorch
 * materialises the 156 MB gradient and the optimiser re-reads it): rows [r0, r0+rows) of the (theta_ld x 2048) heads matrix,
 *   g = dtheta_all[:, r0:r0+rows]^T . t5_all (Kc clouds);  W_rows, m_rows (exp_avg), v_rows (exp_avg_sq) <- Adam(g), in place;
 * g is never written (6 x 156 MB of traffic instead of 8 x).  Pointers address row r0; 16-byte aligned; wd = 0. */
int hp_hypernet_heads_dw_adam(int Kc, int rows, int r0, const float* dtheta_all, int theta_ld, const float* t5_all,
                              float* W_rows, float* m_rows, float* v_rows, float lr, float beta1, float beta2, float eps,
                              int step, hpStream_t stream);
/* ... as a BACKGROUND stream: persistent 16-wave workgroups on `cus` of the 256 CUs (0: 176) — for a caller
 * that runs the pass on its own stream beside latency-built launches which need the other CUs.  Same results. */
int hp_hypernet_heads_dw_adam_bg(int Kc, int rows, int r0, const float* dtheta_all, int theta_ld, const float* t5_all,
                                 float* W_rows, float* m_rows, float* v_rows, float lr, float beta1, float beta2, float eps,
                                 int step, int cus, hpStream_t stream);

/* The M = B <= 64 chains (hypernetwork trunk, encoder fc/mu/std tail) run as skinny layer programs — ONE latency-built
 * launch per phase (layer), ordered by the kernel boundary, no reduce launches: csrc/skinny.hip; the one-persistent-launch
 * variant with a grid-wide barrier was measured and dropped — when their shapes allow, otherwise as tiled GEMM launches.  Diagnostic switch for parity tests: 0 forces the GEMM launches, 1 the layer programs
 * (default; HP_SKINNY=0 in the environment turns it off).  Returns the previous setting.  No reference counterpart. */
/* [test hook: process-wide switch — see the header comment] */
int hp_skinny_set_enabled(int on);
/* [test hook: read-only counter] Layer programs launched since the library was loaded: one per direction of a trunk or an
 * encoder tail (one for both tails of a pair) that the layer programs served; a call whose shapes fall back to the tiled GEMM
 * launches leaves it unchanged.  Monotonic, process-wide, atomic.  The parity tests read it to know which path ran. */
long hp_skinny_programs_run(void);

/* The B per-cloud TargetNetworks of one step at once (model/full_model.py:70-74, model/target_network.py:6-45).
 * theta (B,theta_ld): [W1 b1 | W2 b2 | ... | Wout bout] per cloud; pts (B,N,3) -> y (B,N,3) (rec[b] = y[b]^T).
 * acts: hidden activations kept for the backward (hp_target_saved_floats floats). */
long hp_target_theta_size(int n_hidden, const int* channels);
long hp_target_saved_floats(int B, int N, int n_hidden, const int* channels);
int hp_target_forward(int B, int N, int n_hidden, const int* channels, const float* theta, int theta_ld, const float* pts,
                      float* acts, float* y, hpStream_t stream);
long hp_target_backward_workspace_floats(int B, int N, int n_hidden, const int* channels);
int hp_target_backward(int B, int N, int n_hidden, const int* channels, const float* theta, int theta_ld, const float* pts,
                       const float* acts, const float* grad_y, float* grad_theta, float* ws, hpStream_t stream);

/* The same decoder for the published architecture (n_hidden = 4, channels 32/64/128/64; hp_target_fused_supported
 * says so) as ONE kernel per direction: the cloud's 19 011 weights sit in LDS, activations stay in registers, the
 * backward recomputes the forward (nothing is saved) and writes per-workgroup partial d theta into ws
 * (hp_target_fused_workspace_floats floats), added in order by a second kernel.  Same results as
 * hp_target_forward / hp_target_backward up to fp32 summation order. */
int hp_target_fused_supported(int n_hidden, const int* channels);
long hp_target_fused_workspace_floats(int B, int N);
/* The fused target-network forward computes its hidden layers on the f16 matrix pipe from two f16 pieces per fp32 operand
 * (csrc/target_fused.hip; the arithmetic of csrc/conv_split.hip with per-wave / per-channel scales).  0 selects the fp32 MFMA
 * forward (also: environment HP_TARGET_F16=0).  Returns the previous setting. */
/* [test hook: process-wide switch — see the header comment] */
int hp_target_fused_set_f16(int on);
int hp_target_fused_forward(int B, int N, const float* theta, int theta_ld, const float* pts, float* y, hpStream_t stream);
int hp_target_fused_backward(int B, int N, const float* theta, int theta_ld, const float* pts, const float* grad_y,
                             float* grad_theta, float* ws, hpStream_t stream);

/* ------------------------------------------------------------------------------------------
 * Auxiliary kernels of the step
 * ------------------------------------------------------------------------------------------ */
/* Decoder input points (utils/points.py:8-36 distribution) for total = B*N points, Philox(seed, offset). */
int hp_sample_points(long total, float coef, unsigned long long seed, unsigned long long offset, float* out,
                     hpStream_t stream);
/* Random-plane slicer (datasets/utils/dataset_generator.py:26-39) for B clouds: part_a (B,target,3) is the side of an
 * accepted random plane that holds exactly `target` points, part_b (B,N-target,3) the rest, both in original order;
 * plane (B,4) = normal + bias of the accepted plane; status (B) int: 0 ok, 1 none accepted in max_rounds*4 draws.
 * Candidate c = 4*round + wave of cloud b is drawn from Philox4x32-10 blocks (b, round, wave, 0..2) under key = seed; the
 * FIRST accepted candidate in c order wins, its "under" side (dot + bias > 0 in fp32) if that one holds `target` points.
 * Status is per cloud, and NOTHING is written for a failed cloud: its rows of part_a, part_b and plane (and of
 * hp_slice_clouds_planes' parts) keep what the caller put there; the other clouds of the call are unaffected.
 * N <= 8192 (the cloud is staged in LDS, 12 N bytes); -1 beyond that, before any HIP call. */
int hp_slice_clouds(int B, int N, int target, const float* pts, unsigned long long seed, int max_rounds, float* part_a,
                    float* part_b, float* plane, int* status, hpStream_t stream);
/* The same split with the CALLER's candidate planes: planes (B, R, 4) float64 device memory = (params, bias) of
 * dataset_generator.py:6-8's HyperPlane; cloud i tries planes[i,0..R) in order and classifies every point in float64 exactly
 * as HyperPlane.check_point (:10-11) — with the planes numpy's generator hands the reference, part_a / part_b ARE
 * SlicedDatasetGenerator.generate_item's two return values (tests/golden/slicer.npz).  plane_idx (B): index of the accepted
 * candidate, -1 (and status 1) when none of the R was accepted. */
int hp_slice_clouds_planes(int B, int N, int target, const float* pts, const double* planes, int R, float* part_a,
                           float* part_b, int* plane_idx, int* status, hpStream_t stream);
/* Batch maker (csrc/batch_maker.hip): one training batch from a device-resident dataset clouds (M,N,3), N <= 8192,
 * 0 < target < N, in one chip-wide call and without a host synchronisation.  Item b is cloud ids[b], split by the FIRST
 * accepted candidate plane of its own sequence and rotated about z by degrees[b] (rot (360,2) = (cos, sin) fp32 per degree;
 * degrees NULL: no rotation; x' = x*c + y*s, y' = y*c - x*s as datasets/shapenet.py:73-92, applied after the split).
 * Candidate c of item b is a pure function of (seed, streams[b], c): three Philox4x32-10 blocks, counter
 * (stream_lo, stream_hi, c, k), k = 0,1,2, key = seed, uniforms (x >> 8) * 2^-24 -> three points of [0,1)^3 -> the plane of
 * dataset_generator.py:13-20, accepted when one side holds exactly `target` points ("under" = dot + bias > 0 is tried first).
 * `groups` workgroups per item share the candidates in interleaved chunks; the result does not depend on it.
 * existing (B,target,3) / missing (B,N-target,3): the two sides in the cloud's point order; gt (B,N,3): the cloud; every row
 * of existing and missing is bitwise a row of gt.  plane (B,4), index (B): the accepted plane and its candidate number.
 * No accepted candidate below max_candidates (or an id outside [0,M)) is a value, not an error: index[b] = -1, *failed += 1
 * (never reset here), plane 0, and the outputs fall back to the first `target` points / the rest.
 * ws: hp_make_batch_workspace_bytes(B, N) bytes (-1 on a bad shape). */
long hp_make_batch_workspace_bytes(int B, int N);
int hp_make_batch(int M, int N, int target, const float* clouds, int B, const int* ids, const long long* streams,
                  const int* degrees, const float* rot, unsigned long long seed, int max_candidates, int groups,
                  float* existing, float* missing, float* gt, float* plane, int* index, int* failed, void* ws,
                  hpStream_t stream);
/* Viewpoint batch maker (csrc/view_split.hip): hp_make_batch's interface with another law — `existing` is what a depth sensor at
 * the item's viewpoint records of the cloud, the near side, and `missing` what the object hides from it: the self-occluded input
 * of hp_scan_visibility's virtual scans as a training batch of exact sizes, in one launch and without a host synchronisation.
 * clouds (M,N,3) fp32, 2 <= N <= HP_VIEW_SPLIT_MAX_POINTS, 0 < target < N; item b is cloud ids[b] seen in frames[b] (3,3) fp32
 * row-major = Q, whose rows are the camera's right, up and towards-the-sensor axes (not required to be orthonormal); the sensor
 * sits at dist > 0 along Q's third row; scale = (0.5 R) / h is the caller's, computed once in fp64, h the tangent of the image's
 * half-angle; the image is R x R pixels.  Every floating operation below is one IEEE rounding in the association written, no
 * contraction, no library function (numpy gives the same bits: tests/view_split_law.py).
 *     project    p = double(row); c_k = (Q[k,0] p_x + Q[k,1] p_y) + Q[k,2] p_z, k = 0, 1, 2; delta = dist - c_2;
 *                z = float(delta), round to nearest even.  A row is ABSENT when a coordinate is non-finite, or not (delta > 0), or
 *                z is not finite.  Otherwise u = c_0 / delta, fu = (u * scale) + 0.5 R, iu = int(floor(min(max(fu, 0.0), R - 1.0)))
 *                — max(f, 0.0) is f where f > 0.0 and 0.0 elsewhere, min(f, a) is f where f < a and a elsewhere, so a NaN lands in
 *                pixel 0 —, `it` likewise from c_1; pixel = it * R + iu.  A row outside the image is clamped into a border pixel,
 *                never dropped.
 *     buffer     R^2 uint32 words; an empty word is all ones, another holds the smallest bit pattern of z over the rows that
 *                project to it (z >= 0: bit patterns order as values).
 *     occlusion  front = the smallest word among the pixels (it + dy, iu + dx), |dx|, |dy| <= w, inside the image (the row's own
 *                is never empty, and its word is at most bits(z): o >= +0); o = z - float(front) in fp32, one rounding; +inf
 *                for an absent row.
 *     split      the rows ranked by (o, row) ascending — numpy's float32 `<`; absent rows last, in row order —: the `target`
 *                lowest are `existing`, the rest `missing`, both in the cloud's row order.  There is no failed item: where fewer
 *                than `target` rows project, absent rows fill up in row order.
 *     rotation   degrees / rot as hp_make_batch: x' = x*c + y*s, y' = y*c - x*s, applied to the output rows after the split.
 * existing (B,target,3), missing (B,N-target,3), gt (B,N,3) the whole cloud: every row of existing and missing is bitwise a row
 * of gt.  side (B,N) uint8 or NULL: 1 = existing.  occlusion (B,N) fp32 or NULL: o.  An id outside [0,M) is a value, not an
 * error: the three parts get zeros (side: the first `target` rows, occlusion +inf).
 * An item's result depends on its cloud, its frame and the scalars only — not on B, its place in the batch or the launch geometry.
 * One launch, one workgroup per item; the depth buffer lives in LDS under integer atomicMin — no float atomics, no
 * compare-and-swap, no workspace, no memset, nothing allocated.  The pixel must be about the sample spacing or coarser, or the far
 * side shows through the holes of the near one: R = 32 with w = 1 for 2048 rows.
 * Checked before any HIP call (-1): M >= 1, 1 <= B <= 65535, N and target as above, HP_VIEW_SPLIT_MIN_RESOLUTION <= R <=
 * HP_VIEW_SPLIT_MAX_RESOLUTION, 0 <= w <= HP_VIEW_SPLIT_MAX_WINDOW, dist and scale finite and > 0, pointers not NULL (side and
 * occlusion may be; degrees may be, rot must be given with it).
 *
 * hp_make_view_batch_plan: threads per workgroup and the bytes of dynamic LDS of a call — 4 R^2 + 6 roundup(N, 64).  Host only. */
#define HP_VIEW_SPLIT_MAX_POINTS 8192
#define HP_VIEW_SPLIT_MIN_RESOLUTION 4
#define HP_VIEW_SPLIT_MAX_RESOLUTION 128
#define HP_VIEW_SPLIT_MAX_WINDOW 4
int hp_make_view_batch_plan(int N, int R, int* threads, int* lds);
int hp_make_view_batch(int M, int N, int target, const float* clouds, int B, const int* ids, const float* frames /* (B,3,3) */,
                       const int* degrees, const float* rot, double dist, double scale, int R, int w, float* existing,
                       float* missing, float* gt, unsigned char* side /* (B,N) or NULL */, float* occlusion /* (B,N) or NULL */,
                       hpStream_t stream);
/* Scan preparation (csrc/scan_prep.hip): ragged partial scans -> fixed-size encoder inputs, and back to scene coordinates.
 * A ragged set is points (T,3) fp32 + offsets (S+1) int64, both device memory; scan s is rows offsets[s] .. offsets[s+1].
 * Arguments the host can see are checked before any HIP call (-1): counts >= 1, 1 <= target <= 8192, replace 0 or 1,
 * pointers, center and scale given together.  A scan's length lives on the device and is checked there:
 * 1 <= n_s <= HP_SCAN_MAX_POINTS, otherwise the item counts as failed (hp_prepare_scans) / its box is NaN (hp_scan_boxes).
 *
 * hp_scan_boxes: per scan, in fp32, mn / mx per axis, center (S,3) = (mx + mn) / 2, scale (S) = max_axis(mx - mn) / 0.9f —
 * datasets/real_data.py:26-33 as numpy evaluates it on float32 arrays.  One workgroup per scan, no atomics: the result does
 * not depend on the order of a scan's points.  K completions of N points are the ragged set offsets = arange(K+1) * N.
 *
 * hp_prepare_scans: item b is scan ids[b] resampled to `target` points.  index (B,target): the chosen rows of the scan;
 * out (B,target,3): those rows, bit for bit (center, scale NULL), or (p - center[id]) / scale[id] as one rounded subtraction
 * and one rounded division.  The index law is a pure function of (seed, streams[b], n, target, replace) — not of the item's
 * place in the batch, of B or of the points: Philox4x32-10 with key = seed (lo, hi) and counter (stream_lo, stream_hi, q, tag);
 * word i of a tag is lane i & 3 of block q = i >> 2; key_i = word i of tag 0; draw_j = (uint64(word j of tag 1) * n) >> 32.
 *     n == target              0 .. n-1
 *     n <  target              0 .. n-1, then draw_0 .. draw_{target-n-1}          (utils/util.py:97-100, shapenet_3depn.py:29-39)
 *     n >  target, replace 0   the `target` points with the smallest (key_i, i), in ascending i: a uniform subset without
 *                              replacement, equal keys broken by index (the reference's random order of the subset is not
 *                              kept: the encoder max-pools over the points)
 *     n >  target, replace 1   draw_0 .. draw_{target-1} in draw order                             (shapenet_3depn.py:18-26)
 * The multiply-shift draw is not exactly uniform: a value's probability is off by at most n / 2^32 relative.
 * An id outside [0,S) (or a scan outside the length limits) is a value, not an error: *failed += 1 (never reset here),
 * out rows 0, index -1; nothing is read out of range.
 *
 * hp_restore_scans: out (K,N,3) = (c / s_scale[k]) * scale[k] + center[k], each operation rounded once in that order
 * (real_data.py:63-67); s_scale (K) is hp_scan_boxes' scale of the completions, center (K,3) / scale (K) the scans' boxes. */
#define HP_SCAN_MAX_POINTS (1 << 22)
int hp_scan_boxes(int S, const float* points, const long long* offsets, float* center /* (S,3) */, float* scale /* (S) */,
                  hpStream_t stream);
int hp_prepare_scans(int B, const float* points, const long long* offsets, int S, const int* ids, const long long* streams,
                     unsigned long long seed, int target, int replace, const float* center, const float* scale, float* out,
                     int* index, int* failed, hpStream_t stream);
int hp_restore_scans(int K, int N, const float* completions, const float* s_scale, const float* center, const float* scale,
                     float* out, hpStream_t stream);
/* Farthest-point sampling (csrc/fps.hip): k picks out of each of B clouds (B,P,3) fp32 in one launch, one workgroup per cloud.
 * Per cloud, with count = counts[b] (NULL: P) valid rows p_0 .. p_{count-1} and start row s = start[b] (NULL: 0):
 *     d2(i, j)   = ((dx*dx + dy*dy) + dz*dz), dx = p_i.x - p_j.x etc.; every operation one fp32 rounding in this association,
 *                  no contraction (numpy float32 gives the same bits)
 *     pick_0     = s,                      mind_i = d2(i, pick_0)
 *     pick_j     = argmax_i mind_i, equal values broken by the lowest i;  then mind_i = min(mind_i, d2(i, pick_j))
 *     radius2[j] = max_i mind_i after picks 0..j: the squared covering radius of the first j+1 picks, non-increasing in j
 * count < k needs no special case: once every mind_i is 0 the arg-max is row 0, so the tail is row 0 with radius2 0.
 * index (B,k): the picks, rows of the cloud; radius2 (B,k) or NULL.  A cloud's result depends on its rows below count, on
 * count, s and k only — not on B, on its place in the batch or on the rows at or beyond count, which are never read.
 * Checked before any HIP call (-1): B >= 0 (0: nothing to do), 1 <= P <= HP_FPS_MAX_POINTS, 1 <= k <= 8192, clouds, index and
 * failed not NULL.  counts[b] outside [1,P] or start[b] outside [0,count) is a value, not an error: *failed += 1 (never reset
 * here), the item's index row -1 and its radius2 row 0; nothing is read out of range and the other rows are as without it.
 *
 * hp_farthest_points_plan: the instance the launcher picks for P — threads per workgroup and rows per lane
 * (threads * points_per_lane >= P).  Host only; -1 for P outside [1, HP_FPS_MAX_POINTS] or a NULL pointer. */
#define HP_FPS_MAX_POINTS 8192
int hp_farthest_points(int B, int P, const float* clouds, const int* counts, const int* start, int k, int* index,
                       float* radius2, int* failed, hpStream_t stream);
int hp_farthest_points_plan(int P, int* threads, int* points_per_lane);
/* k nearest neighbours and statistical outlier removal over ragged scans (csrc/knn.hip); a ragged set as for hp_scan_boxes.
 * Everything is per scan: rows of other scans never take part.
 *     d2(i, j)   = ((dx*dx + dy*dy) + dz*dz), dx = q_i.x - p_j.x etc.; every operation one fp32 rounding in this association, no
 *                  contraction (hp_farthest_points' formula).  A NaN d2 counts as +inf; an overflowed +inf is a legal value.
 *     absent     a row with a non-finite coordinate: nobody's candidate, and as a query it gets the empty result.
 *     candidates of query i: the present rows j of the same scan, j != i under exclude_self, ordered by the pair
 *                  (d2 as its uint32 bit pattern, j) ascending — a total order, equal distances go to the lower row.
 *     result     the first k candidates: index (Q,k) int32 rows within the scan, dist2 (Q,k) fp32; slots beyond the number of
 *                  candidates hold index -1 and dist2 +inf.  Both outputs are fully written.
 * hp_knn_points: queries (Q,3) / query_offsets (S+1) are a second ragged set over the same S scans (query i of scan s is row
 * query_offsets[s] + i; under exclude_self it skips candidate row i); both NULL means the scans themselves, and then — or with
 * queries == points — exclude_self must be 1.  Brute force, O(n^2) per scan.  Checked before any HIP call (-1): S >= 1,
 * 1 <= k <= 32, exclude_self 0 or 1, points / offsets / index / dist2 not NULL, queries and query_offsets given together, the
 * rule above.  A scan's length lives on the device: a scan of more than HP_KNN_MAX_POINTS candidates (or fewer than 1) is a
 * value, not an error — its queries get the empty result; nothing is read out of range.
 *
 * hp_knn_points_plan: the compile-time instance that serves k (lists of 8, 16 or 32 slots; a k in between uses the next one
 * and writes its first k slots), threads per workgroup = queries per chunk, and candidates per LDS tile.  Host only; -1 for
 * k outside [1, 32] or a NULL pointer.
 *
 * hp_scan_outliers(k, ratio): with the neighbours above (queries = the scan, exclude_self) and c_i = the valid slots of row i,
 *     m_i        = float32((sum_t sqrt64(float64(dist2_t))) / c_i): the fp64 sum sequential in slot order, sqrt and the division
 *                  correctly rounded.  Rows with c_i = 0 or a non-finite m_i are absent too: never kept, not in the statistics.
 *     M          = the largest m_i of the n_p participating rows.  n_p <= 1 or M == 0: every participating row is kept.
 *     q_i        = trunc(m_i * 2^(23-e)) with e = floor(log2 M) from M's bits: exact, 0 <= q_i < 2^24.
 *     S1, S2     = sum q_i, sum q_i^2 as exact integers (unsigned 64 bits hold them up to HP_KNN_MAX_POINTS rows).
 *     mu         = double(S1) / n_p;  var = max(0, (double(S2) - mu * double(S1)) / (n_p - 1));
 *     thr        = mu + double(ratio) * sqrt(var);  keep row i iff double(q_i) <= thr
 *                  — each a single fp64 operation, one rounding, no fma; integer-to-double conversions round to nearest even.
 * keep (T) uint8; mean_dist (T) fp32 = m_i, +inf for absent rows; kept (S) int32 = the rows kept per scan.  The integer sums make
 * the result independent of any reduction order.  Two launches, no workspace, no host synchronisation.  Checked before any HIP
 * call (-1): S >= 1, 1 <= k <= 32, 0 <= ratio finite, pointers.  A scan beyond HP_KNN_MAX_POINTS keeps nothing (all rows absent). */
#define HP_KNN_MAX_POINTS 65536
int hp_knn_points(int S, const float* points, const long long* offsets, const float* queries, const long long* query_offsets,
                  int k, int exclude_self, int* index /* (Q,k) */, float* dist2 /* (Q,k) */, hpStream_t stream);
int hp_knn_points_plan(int k, int* instance_k, int* threads, int* tile);
int hp_scan_outliers(int S, const float* points, const long long* offsets, int k, float ratio, unsigned char* keep /* (T) */,
                     float* mean_dist /* (T) */, int* kept /* (S) */, hpStream_t stream);
/* The same neighbours and the same outlier removal behind a uniform grid (csrc/knn_grid.hip), for scans of up to
 * HP_KNN_GRID_MAX_POINTS rows.  The law of the lists is hp_knn_points', word for word and bit for bit: d2, absent rows, the
 * order by (bits of d2, row), the first k, -1 and +inf in the slots beyond the candidates.  The grid is an acceleration
 * structure only — no property of it (cell edge, origin, the order of rows inside a cell) shows in any output.
 *     grid       per scan, chosen on the device: lo = the box minimum of the present rows, a cell edge h, G_c <= 1024 cells per
 *                axis and G_x G_y G_z <= 2 n_s + 64 cells in all; an axis of zero or overflowed (inf) extent has one cell.
 *                cell (S) fp32 or NULL: cell[s] > 0 and finite is a request for scan s's edge, raised as far as the two caps
 *                demand; anything else means the default rule (the occupied cells of coarse 32^3, 16^3 and 8^3
 *                histograms estimate what the scan fills — a curve, a surface, a volume; h aims at k/2 rows per occupied cell).
 *     cells      edge_c(j) = fl(lo_c + fl(float(j) * h)); a coordinate lies in the largest cell j with edge_c(j) <= x, cell 0 if
 *                none: the first and the last cell are unbounded outwards, so queries outside the box fall into end cells.
 *     search     64 queries in cell order share a block of cells that covers their cells, grown shell by shell.  A query is
 *                done iff its list is full and its worst d2 is strictly below min over the block's faces inside the grid of
 *                fl(fl(edge_face - q_c)^2): subtraction, squaring and the sum of non-negative terms are monotone in fp32, so
 *                no row outside the block can have a smaller d2, and strictness keeps a tie to a lower row out of it.  The
 *                whole grid ends every query.
 * hp_knn_grid: arguments as hp_knn_points; index / dist2 (both), or mean_dist (Q) alone — then the m_i of the outlier law below
 * are written instead of the lists.  grid (S,4) fp32 or NULL receives (h, G_x, G_y, G_z) per scan, zeros for a scan that is
 * not searched.  ws: hp_knn_grid_workspace_bytes(S, T, Q) bytes, 16-byte aligned (T, Q: the rows of the two sets; Q <= 0
 * without a second set); the lengths live on the device, so a workspace that is too small for them is a value as well — every
 * query then gets the empty result.  Checked before any HIP call (-1): hp_knn_points' conditions, ws and ws_bytes > 0, the
 * alignment, lists or mean_dist but not both.  A scan of more than HP_KNN_GRID_MAX_POINTS candidates, or without a present
 * one, is a value: its queries get the empty result; nothing is read out of range.  Five launches (seven with a second set),
 * integer atomics only, no host synchronisation.
 *
 * hp_knn_grid_plan: as hp_knn_points_plan — the list length of the instance, threads per workgroup (one wave: 64 queries
 * share a block) and candidates per LDS tile.  hp_knn_grid_workspace_bytes: host only; -1 for S < 1 or rows out of range.
 *
 * hp_outlier_keep(ratio): hp_scan_outliers' statistics over given mean_dist (T) for scans of up to HP_KNN_GRID_MAX_POINTS
 * rows.  The law is the one above with S2 an exact integer of up to 70 bits (q_i < 2^24, n_p <= 2^22) — the squares' low and
 * high 32 bits are summed apart and combined exactly — converted to double by round-to-nearest-even; every other line is
 * unchanged, so the result equals hp_scan_outliers' wherever that is defined.  A longer scan keeps nothing.
 * hp_scan_outliers_grid: hp_knn_grid's m_i (the scans themselves, exclude_self) and then hp_outlier_keep. */
#define HP_KNN_GRID_MAX_POINTS (1 << 22)
long long hp_knn_grid_workspace_bytes(int S, long long T, long long Q);
int hp_knn_grid_plan(int k, int* instance_k, int* threads, int* tile);
int hp_knn_grid(int S, const float* points, const long long* offsets, const float* queries, const long long* query_offsets,
                int k, int exclude_self, const float* cell /* (S) or NULL */, int* index /* (Q,k) */, float* dist2 /* (Q,k) */,
                float* mean_dist /* (Q), or NULL */, float* grid /* (S,4) or NULL */, void* ws, long long ws_bytes,
                hpStream_t stream);
int hp_outlier_keep(int S, const float* mean_dist, const long long* offsets, float ratio, unsigned char* keep /* (T) */,
                    int* kept /* (S) */, hpStream_t stream);
int hp_scan_outliers_grid(int S, const float* points, const long long* offsets, int k, float ratio, const float* cell,
                          unsigned char* keep /* (T) */, float* mean_dist /* (T) */, int* kept /* (S) */, void* ws,
                          long long ws_bytes, hpStream_t stream);
/* Euclidean cluster extraction over ragged scans (csrc/clusters.hip): the connected components of "closer than a radius"; a
 * ragged set as for hp_scan_boxes.  Everything is per scan: rows of other scans never take part.
 *     absent     a row with a non-finite coordinate, as above.
 *     d2(i, j)   = ((dx*dx + dy*dy) + dz*dz), hp_knn_points' formula: every operation one fp32 rounding, no contraction.  It is
 *                  symmetric bit for bit (fp32 subtraction is exactly antisymmetric).  A NaN d2 counts as +inf.
 *     r2         = radius * radius, one fp32 rounding.
 *     edge       {i, j} iff i != j, both rows present and d2(i, j) <= r2.  The test is inclusive: exact duplicates are joined
 *                  even at radius 0.  An overflowed +inf distance never joins.
 *     label[i]   the smallest row index within the scan of the connected component of i; -1 for an absent row.
 *     size[i]    the number of rows of that component; 0 for an absent row.
 *     clusters[s] the number of components of scan s.
 *     largest[s] the label of the component with the most rows, equal sizes to the smaller label; -1 when no row is present.
 * The result is a function of the input alone: no order of evaluation can change it.  max_points is the caller's bound on the
 * longest scan, 1 <= max_points <= HP_CLUSTER_MAX_POINTS: it sizes the LDS of a workgroup (one per scan, the forest lives
 * there), and a scan longer than it gets the empty result — every label -1, size 0, clusters 0, largest -1 — which is a value,
 * not an error; nothing is read or written out of range.  All four outputs are fully written.  One launch, no workspace, no
 * host synchronisation, no global and no float atomics.  Brute force over the pairs j < i, O(n^2) per scan.  Checked before
 * any HIP call (-1): S >= 1, pointers not NULL, radius >= 0 with radius * radius finite, max_points in range.
 *
 * hp_scan_clusters_plan: threads per workgroup (= rows per block of a scan), candidates per LDS tile and the dynamic LDS bytes
 * of a workgroup for max_points.  Host only; -1 for max_points out of range or a NULL pointer. */
#define HP_CLUSTER_MAX_POINTS 32768
int hp_scan_clusters(int S, const float* points, const long long* offsets, float radius, int max_points,
                     int* label /* (T) */, int* size /* (T) */, int* clusters /* (S) */, int* largest /* (S) */,
                     hpStream_t stream);
int hp_scan_clusters_plan(int max_points, int* threads, int* tile, int* lds_bytes);
/* The supporting plane of ragged scans by random sample consensus (csrc/plane.hip): the floor or table top that joins every
 * object of a scene into one component, fitted and marked before hp_scan_clusters sees the scan; a ragged set as for
 * hp_scan_boxes.  Everything is per scan: rows of other scans never take part.  Every float operation below is one fp32
 * rounding in the association written, no contraction (numpy float32 gives the same bits).
 *     absent     a row with a non-finite coordinate, as above; never an inlier.
 *     draws      Philox4x32-10 exactly as hp_prepare_scans: key = seed (lo, hi), counter (stream_lo, stream_hi, q, tag), word i of
 *                the tag = lane i & 3 of block q = i >> 2; the tag is 4 (0-2: scan preparation and batches, 3: meshes);
 *                stream = streams[s], or s when streams is NULL.  Trial h < trials samples the rows
 *                r_k = (uint64(word[3h+k]) * n) >> 32, k = 0, 1, 2, of the n rows of the scan.
 *     trial h    a, b, c = rows r_0, r_1, r_2;  u = b - a, v = c - a;
 *                nrm  = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x);   len2 = ((nx*nx + ny*ny) + nz*nz);
 *                t2 = threshold*threshold;   rhs = t2*len2.
 *                The trial is valid iff n >= 3, len2 is finite and > 0, and rhs is finite: a repeated row, collinear
 *                samples and an absent sample row are all refused by this one rule.
 *     inlier     row p of trial h iff e*e <= rhs with e = ((nx*(p.x-a.x) + ny*(p.y-a.y)) + nz*(p.z-a.z)): the test is inclusive
 *                (the sample rows pass at threshold 0), has no root and no division, and a NaN or an overflowed e*e never passes.
 *     winner     count[h] = the inliers of trial h, an exact integer; the winner is the valid trial with the largest count,
 *                ties to the lower h.  trial[s] = that h, or -1 when no trial is valid.
 *                found[s] = count >= min_inliers and double(count) >= double(min_share) * double(n), one fp64 product.
 *     outputs    inliers[s] = the winner's count; sample (S,3) = its rows within the scan; sample_plane (S,4) =
 *                (nx, ny, nz, -((nx*a.x + ny*a.y) + nz*a.z)), not normalised; inlier (T) uint8 = its mask.
 *                With trial -1: inliers 0, found 0, sample -1, sample_plane four quiet NaNs (0x7FC00000), a zero mask.
 *     moments    of the winner's inliers, for a least-squares refit in exact arithmetic: dq = p - a; M = the largest |dq_c|
 *                over the inliers and c = x, y, z; e = M's biased exponent field - 127 (floor(log2 M) for a normal M);
 *                q_c = trunc(ldexp(dq_c, 19 - e)): exact, |q_c| < 2^20.  moments (S,10) int64 =
 *                [cnt, Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz] over the q's with cnt the winner's count — a scan of 2^22 rows
 *                fits without overflow —, shift (S) = e.  M == 0 (every inlier on row a): shift 0, the nine sums 0.
 *                With trial -1: ten zeros and shift 0.
 * The result is a function of the input alone: integer adds and an integer max, no float atomics.  A scan shorter than 3 rows
 * or longer than HP_SCAN_MAX_POINTS gets the empty result (trial -1), which is a value, not an error; nothing is read out of
 * range.  The cost is O(n * trials) per scan.  All outputs are fully written.  Five launches, no host synchronisation.
 * ws: hp_scan_plane_workspace_bytes(S, trials) bytes of device memory, 16-byte aligned (-1 on bad arguments).
 * Checked before any HIP call (-1): S >= 1, pointers not NULL (streams may be), 1 <= trials <= HP_PLANE_MAX_TRIALS,
 * threshold >= 0 with threshold * threshold finite, min_inliers >= 3, 0 <= min_share <= 1.
 *
 * hp_scan_plane_plan: threads per workgroup of the consensus kernel, rows a lane holds (a workgroup covers
 * threads * rows_per_lane consecutive rows of the ragged set) and hypotheses per LDS tile.  Host only; -1 for trials out of
 * range or a NULL pointer.
 *
 * hp_scan_plane_side: every row against a given plane of its scan, planes (S,4) fp32 (nx, ny, nz, d):
 *     dist (T)   = ((nx*p.x + ny*p.y) + nz*p.z) + d; the quiet NaN 0x7FC00000 for an absent row, and for any NaN result.
 *     keep (T)   = 1 iff the row is present and not (|dist| <= threshold): a NaN plane keeps every present row.
 *     kept (S)   = the rows kept per scan.
 * Scans of any length.  Checked before any HIP call (-1): S >= 1, pointers not NULL, the threshold as above. */
#define HP_PLANE_MAX_TRIALS 4096
long hp_scan_plane_workspace_bytes(int S, int trials);
int hp_scan_plane_plan(int trials, int* threads, int* rows_per_lane, int* trial_tile);
int hp_scan_plane(int S, const float* points, const long long* offsets, const long long* streams /* (S) or NULL */,
                  unsigned long long seed, int trials, float threshold, int min_inliers, float min_share,
                  int* trial /* (S) */, int* inliers /* (S) */, int* found /* (S) */, int* sample /* (S,3) */,
                  float* sample_plane /* (S,4) */, unsigned char* inlier /* (T) */, long long* moments /* (S,10) */,
                  int* shift /* (S) */, void* ws, hpStream_t stream);
int hp_scan_plane_side(int S, const float* points, const long long* offsets, const float* planes /* (S,4) */, float threshold,
                       float* dist /* (T) */, unsigned char* keep /* (T) */, int* kept /* (S) */, hpStream_t stream);
/* Voxel-grid thinning of ragged scans (csrc/voxels.hip): one representative row per occupied cell of a regular grid, the stage
 * that brings a sensor scan of hundreds of thousands of rows under HP_KNN_MAX_POINTS and HP_CLUSTER_MAX_POINTS at an even
 * density; a ragged set as for hp_scan_boxes.  Everything is per scan: rows of other scans never take part.  Every float
 * operation below is one fp32 rounding in the association written, no contraction; the division is the correctly rounded one
 * (numpy float32 gives the same bits).
 *     voxel      (S) fp32, the cell edge of each scan.  A scan whose voxel is not finite or not > 0 gets the empty result.
 *     origin     (S,3) fp32 or NULL.  NULL: u = p, no operation at all; otherwise u = p - origin[s], one subtraction per axis.
 *     absent     a row with a non-finite coordinate, as above.
 *     cell       q_c = floor(u_c / voxel[s]) per axis; the row is inside iff -2^20 <= q_c < 2^20 on all three axes (a NaN or
 *                overflowed quotient is not inside).  A present row that is not inside is beyond the grid and takes no part.
 *                key = ((qx + 2^20) << 42) | ((qy + 2^20) << 21) | (qz + 2^20), below 2^63.
 *     centre     m_c = (float(q_c) + 0.5f) * voxel[s]: the convert and the add are exact, the product is rounded once.
 *     d2         ((dx*dx + dy*dy) + dz*dz) with d = u - m — hp_knn_points' formula; an overflowed +inf is a legal value.
 *     rank       keep_mode 0 ("center"): the pair (d2's uint32 bit pattern, row within the scan), ascending;
 *                keep_mode 1 ("first"): the row alone.  Either is a total order.
 *     label (T)  int32: the smallest row within the scan among the inside rows of the row's cell; -1 for absent and beyond rows.
 *     size (T)   int32: the number of inside rows of that cell; 0 for absent and beyond rows.
 *     keep (T)   uint8: 1 iff the row is inside and has the smallest rank of its cell — exactly one row per occupied cell.
 *     kept (S)   int32: the rows kept = the occupied cells.   beyond (S) int32: the present rows outside the grid.
 * A scan that is empty, longer than HP_SCAN_MAX_POINTS or has a bad voxel gets the empty result: every label -1, size 0,
 * keep 0, kept 0, beyond 0 — a value, not an error.  All outputs are fully written.
 * T is the caller's promise of the rows of points, = offsets[S]: it sizes the table, no row at or beyond T is read, and a
 * scan that reaches beyond T gets the empty result.
 * The result is a function of the input alone — not of the launch geometry, of slots_per_row or of which row claimed a slot:
 * a hash table in ws gives scan s the slots [slots_per_row * offsets[s], slots_per_row * offsets[s+1]); a slot is claimed by
 * a 64-bit compare-and-swap on its key and takes an integer min of the ranks, an integer min of the rows and an integer add
 * of the count; no flags, fences or float atomics.  Three launches, no host synchronisation, nothing is allocated.
 * ws: hp_scan_voxels_workspace_bytes(T, slots_per_row) bytes of device memory, 16-byte aligned (-1 on bad arguments).
 * Checked before any HIP call (-1): S >= 1, 0 <= T <= 2^28, keep_mode in {0, 1}, slots_per_row in {1, 2, 4}, pointers not
 * NULL (origin may be).  T == 0 writes kept and beyond as zeros and returns 0.
 *
 * hp_scan_voxels_plan: threads per workgroup and rows per lane (a workgroup covers threads * rows_per_lane consecutive rows
 * of the ragged set).  Host only; -1 for a NULL pointer. */
#define HP_VOXEL_GRID_HALF (1 << 20)
long hp_scan_voxels_workspace_bytes(long long T, int slots_per_row);
int hp_scan_voxels_plan(int* threads, int* rows_per_lane);
int hp_scan_voxels(int S, long long T, const float* points, const long long* offsets, const float* voxel /* (S) */,
                   const float* origin /* (S,3) or NULL */, int keep_mode, int slots_per_row, int* label /* (T) */,
                   int* size /* (T) */, unsigned char* keep /* (T) */, int* kept /* (S) */, int* beyond /* (S) */, void* ws,
                   hpStream_t stream);
/* Visibility of ragged scans from their sensor positions (csrc/visibility.hip): a depth buffer of every scan on a gnomonic cube
 * map about its viewpoint, and the labels of rows against it — what makes the self-occluded view of a complete cloud, and what
 * tells a completion that fills the sensor's free space from one that stays behind the recorded surface; a ragged set as for
 * hp_scan_boxes.  Everything is per scan s with viewpoints[s] (3) fp32: rows of other scans never take part.  Every operation
 * below is one fp64 rounding in the association written, no contraction (numpy float64 gives the same bits); no library function
 * decides a bit.
 *     project    d = double(p) - double(v) per component, a = |d|; the major axis m is the largest a, ties to the lowest axis;
 *                face = 2 m + (d_m < 0); u = d[(m+1) % 3] / a_m and t = d[(m+2) % 3] / a_m by IEEE division;
 *                iu = min(R - 1, int(floor((u + 1.0) * (0.5 * R)))), `it` likewise from t; the depth z = float(a_m), round to
 *                nearest even, +inf where it overflows: the z-depth of the face's pinhole camera, no square root.
 *     absent     a row with a non-finite coordinate, or of a scan whose viewpoint has one: no pixel, label 4, winner 0.
 *     at v       a row with a_m == 0: no pixel, label 1, winner 0.
 *     buffer     ws holds S * 6 * R^2 uint64 keys laid out (scan, face, it, iu) — pixel ((s * 6 + face) * R + it) * R + iu, all
 *                index arithmetic in 64 bits: (z's uint32 bit pattern) << 32 | row within the scan.  A pixel holds the smallest
 *                key of the rows that project to it, all ones when empty: the nearest depth, equal depths to the lowest row.  After
 *                the call it is the scan's range image, the caller's to read.
 *     classify   a query q — a row of the scan, or with queries (Q,3) / query_offsets (S+1) a row of a second ragged set over
 *                the same S scans — has its pixel (face, it, iu) and its depth z0 = double(z) by the rule above.  Over the pixels
 *                (it + dy, iu + dx) of that face with |dx|, |dy| <= w that lie inside the face and are not empty:
 *                zz = double(the pixel's depth), c = max(|dx|, |dy|) + 1, tol = margin + (z0 * pitch) * c — a recorded point
 *                shadows a cone, not a cylinder; pitch = 2 * slope / R is the caller's, computed once in fp64.  Pixels beyond the
 *                face's edge are skipped: a window does not reach across a cube edge.
 *     label      uint8 (T), or (Q) with queries, decided in this order:
 *                  3 unobserved      no such pixel: the ray met nothing the sensor recorded
 *                  2 hidden          some pixel has zz + tol < z0: something recorded is in front
 *                  0 seen through    every pixel has zz - tol > z0: the sensor looked past q, free space is violated
 *                  1 on the surface  otherwise.        A scan's own rows get 1, 2 or 4 only.
 *     winner     uint8 (T) or NULL, without queries only: 1 iff the row's key is the key its pixel holds — one row per pixel.
 * A scan longer than HP_SCAN_MAX_POINTS, or whose offsets are not 0 <= lo <= hi <= T, writes no pixel; the rows and queries of
 * a scan that is too long are labelled 4.  T and Q (at most 2^31 - 1) are the caller's promise of the rows of points and of
 * queries; without queries Q == T.  Nothing is read out of range.
 * The result is a function of the input alone — not of the launch geometry or the order rows arrive in: the scatter is an integer
 * atomic min on 64-bit words, no float atomics and no compare-and-swap.  A memset of the used part of ws to 0xFF and two launches,
 * scatter and classify, on the caller's stream; no host synchronisation, nothing is allocated.
 * ws: hp_scan_visibility_workspace_bytes(S, R) = S * 6 * R^2 * 8 bytes of device memory, 16-byte aligned (-1 on bad arguments).
 * Checked before any HIP call (-1): S >= 1, 0 <= T, Q <= 2^31 - 1, HP_VISIBILITY_MIN_RESOLUTION <= R <= HP_VISIBILITY_MAX_RESOLUTION,
 * 0 <= w <= HP_VISIBILITY_MAX_WINDOW, margin and pitch finite and >= 0, ws_bytes at least the workspace and ws aligned, pointers
 * not NULL (points may be with T == 0; queries and query_offsets come together; winner may be, and must be with queries).
 *
 * hp_scan_visibility_plan: threads per workgroup, rows per lane (a workgroup covers threads * rows_per_lane consecutive rows),
 * and the workgroups of the scatter launch over T rows and of the classify launch over Q rows (0: not launched).  Host only. */
#define HP_VISIBILITY_MIN_RESOLUTION 4
#define HP_VISIBILITY_MAX_RESOLUTION 1024
#define HP_VISIBILITY_MAX_WINDOW 4
long long hp_scan_visibility_workspace_bytes(int S, int R);
int hp_scan_visibility_plan(long long T, long long Q, int* threads, int* rows_per_lane, int* scatter_groups,
                            int* classify_groups);
int hp_scan_visibility(int S, long long T, const float* points, const long long* offsets, const float* viewpoints /* (S,3) */,
                       int R, int w, double margin, double pitch, long long Q, const float* queries /* (Q,3) or NULL */,
                       const long long* query_offsets /* (S+1) or NULL */, unsigned char* label /* (T) or (Q) */,
                       unsigned char* winner /* (T) or NULL */, void* ws, long long ws_bytes, hpStream_t stream);
/* Depth images in, a cleaned ragged set out (csrc/depth.hip): the front door of the scan chain.  B images of H x W pixels,
 * depth (B,H,W) uint16 (depth_is_u16 = 1) or fp32 (0), K (B,4) double (fx, fy, cx, cy) on the device — pixel centres at integer
 * coordinates, the camera looks along +z, x right, y down —, poses (B,3,4) fp32 row-major [R | t] camera-to-world, widened to
 * fp64 (the identity where there is none: one code path), mask (B,H,W) uint8 or NULL.  Every floating operation below is one
 * fp64 rounding in the association written, no contraction (numpy float64 gives the same bits); sqrt is the correctly rounded one.
 * For pixel (v, u) of image b:
 *     depth      z = double(d) * scale.  Measured: z finite and z > 0 — a hole is 0, a NaN, negative or infinite.
 *     jump       between two measured depths, jump(a, b) = |a - b| > jump_abs + jump_rel * min(a, b); equality is no jump.
 *     edge       w > 0, the pixel is measured, and some measured pixel within |dv|, |du| <= w inside the image jumps against it —
 *                in range and masked in or not: the background behind a silhouette is what gives a mixed pixel away.  Both sides go.
 *     kept       measured, near <= z <= far (inclusive), mask != 0 where a mask is given, and not an edge.
 *     camera     q = (((double(u) - cx) * z) / fx, ((double(v) - cy) * z) / fy, z).
 *     normal     a neighbour of the four-neighbourhood is usable when it is inside the image, measured and does not jump against
 *                the centre (at every w).  a = (right usable ? q_right : q) - (left usable ? q_left : q), b the same with down and
 *                up; n = a x b = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0), each product rounded; if (n0 q0 + n1 q1) + n2 q2 > 0
 *                then n = -n: the normal faces the sensor; l = sqrt((n0^2 + n1^2) + n2^2); n = n / l, or (0, 0, 0) when l is 0 or
 *                not finite — a row without a normal is kept.
 *     world      p_k = ((R_k0 q0 + R_k1 q1) + R_k2 q2) + t_k; the normal likewise without t; both cast to fp32, round to nearest.
 *     outputs    the kept pixels in order of image, row, column: points (T,3) fp32, normals (T,3) fp32, pixel (T) int64 =
 *                (b * H + v) * W + u, offsets (B+1) int64.  The caller holds B * H * W rows of each; rows at and beyond
 *                offsets[B] are not written.
 * Three launches whatever the images hold, on the caller's stream, no host synchronisation, nothing allocated, no atomics: count
 * (kept pixels per chunk of threads * pixels_per_lane = 1024 consecutive row-major pixels of one image, into ws), scan (one
 * workgroup, scan_threads = 1024 chunks a round: chunk bases and offsets), emit (the keep test again, an order-preserving
 * compaction by ballot and popcount, the rows).  The result is a function of the input alone, not of the launch geometry.
 * ws: hp_depth_points_workspace_bytes(B, H, W) = roundup(4 * B * ceil(H * W / 1024), 16) bytes of device memory, 16-byte
 * aligned (-1 on bad arguments).
 * Checked before any HIP call (-1): B, H, W >= 1, H * W <= HP_SCAN_MAX_POINTS, B * H * W <= 2^31 - 1, depth_is_u16 0 or 1, scale
 * finite and > 0, 0 <= near <= far (far may be +inf), jump_abs and jump_rel finite and >= 0, 0 <= w <= HP_DEPTH_MAX_WINDOW,
 * ws_bytes at least the workspace and ws aligned, pointers not NULL (mask may be).
 *
 * hp_depth_points_plan: threads per workgroup, pixels per lane (a chunk is their product), chunks per image =
 * ceil(H * W / chunk), the chunks the scan pass takes per round and its rounds = ceil(B * chunks / scan_threads).  Host only. */
#define HP_DEPTH_MAX_WINDOW 4
long long hp_depth_points_workspace_bytes(int B, int H, int W);
int hp_depth_points_plan(int B, int H, int W, int* threads, int* pixels_per_lane, int* chunks, int* scan_threads,
                         int* scan_rounds);
int hp_depth_points(int B, int H, int W, const void* depth, int depth_is_u16, double scale, const double* K /* (B,4) */,
                    const float* poses /* (B,3,4) */, const unsigned char* mask /* (B,H,W) or NULL */, double near, double far,
                    double jump_abs, double jump_rel, int w, float* points /* (B*H*W,3) */, float* normals /* (B*H*W,3) */,
                    long long* pixel /* (B*H*W) */, long long* offsets /* (B+1) */, void* ws, long long ws_bytes,
                    hpStream_t stream);
/* Posed depth images fused into one surface per volume (csrc/fuse.hip): volumetric fusion with a truncated signed distance
 * function (TSDF).  The images, K, poses, mask, scale, near, far, jump_abs, jump_rel and w are hp_depth_points', and so is the
 * keep test of a pixel (csrc/hp_depth.h states it once for both).  G volumes (groups) of nx x ny x nz voxels of edge `voxel`:
 * group_images (L) int32 and group_offsets (G+1) int32 list the images of each group in order — an image may be in several groups
 * or in none, no image is copied or permuted —, origin (G,3) double is the corner of voxel (0, 0, 0).  Every floating operation is
 * one fp64 rounding in the association written, no contraction; floor is exact; sqrt is the correctly rounded one.
 *     voxel      (i, j, k) of group g has the centre c = (ox + (double(i) + 0.5) * voxel, oy + (double(j) + 0.5) * voxel,
 *                oz + (double(k) + 0.5) * voxel).
 *     image      for each image b of the group, in list order, with [R | t] its pose widened to fp64: d = c - t;
 *                q_a = (R_0a d0 + R_1a d1) + R_2a d2 (the inverse of a rotation); skip unless q2 > 0;
 *                x = ((q0 * fx) / q2) + cx, y = ((q1 * fy) / q2) + cy; u = floor(x + 0.5), v = floor(y + 0.5); skip unless
 *                0 <= u <= W - 1 and 0 <= v <= H - 1, compared in fp64 before any conversion (a NaN is outside); skip unless
 *                pixel (v, u) is kept; s = z(v, u) - q2; skip when s < -truncation (equality is kept); f = s / truncation, then
 *                f = 1 when f > 1; F = F + f, n = n + 1.
 *     volume     weight = n (int32); tsdf = float(F / double(n)) when n > 0, else 1.0f.  Layout (G, nz, ny, nx).
 *     usable     a voxel inside the grid with weight >= min_weight.
 *     row        voxel a and axis e in (x, y, z) with b = a + e inside the grid, fa and fb the two fp32 values widened to fp64:
 *                a row when both are usable and (fa < 0) != (fb < 0).  t = fa / (fa - fb); the point is a's centre with
 *                t * voxel added to component e.
 *     normal     g_d(c) = (usable(c + d) ? f(c + d) : f(c)) - (usable(c - d) ? f(c - d) : f(c)) for each axis d;
 *                m_d = g_d(a) + t * (g_d(b) - g_d(a)); l = sqrt((m0^2 + m1^2) + m2^2); the normal is m / l, or zero when l is 0 or
 *                not finite.  It points into free space, towards the sensors.
 *     outputs    rows in order of group, k, j, i, then axis x, y, z: points (capacity,3) fp32, normals (capacity,3) fp32, cell
 *                (capacity) int64 = (((g * nz + k) * ny + j) * nx + i) * 3 + e, offsets (G+1) int64.  offsets always holds the
 *                true counts; rows at positions >= capacity are not written, and neither is anything beyond offsets[G].
 * Both entry points run on the caller's stream, allocate nothing, make no host synchronisation and use no atomics; the result is a
 * function of the input alone, not of the launch geometry.
 * hp_fuse_volume, two launches: the keep test of every pixel once, as ballot words in ws (one bit per pixel, an image padded to a
 * multiple of 64), then a lane per voxel, x fastest.  ws: hp_fuse_volume_workspace_bytes(B, H, W) = roundup(8 * B * ceil(H * W /
 * 64), 16) bytes, 16-byte aligned.  group_images and group_offsets are on the device; host_group_images and host_group_offsets are
 * the same tables on the host, which the checks read.  Checked before any HIP call (-1): what hp_depth_points checks of its
 * arguments; G >= 1, 1 <= nx, ny, nz <= HP_FUSE_MAX_DIM, G * nx * ny * nz <= 2^31 - 1, L >= 1, voxel and truncation finite and > 0,
 * host_group_offsets[0] = 0, host_group_offsets[G] = L, every group non-empty, image indices in [0, B), ws_bytes and the alignment
 * of ws, pointers not NULL (mask may be).
 * hp_fuse_volume_plan: threads per workgroup, words = ceil(H * W / 64), blocks_per_group = ceil(nx * ny * nz / threads), blocks =
 * G * blocks_per_group.
 * hp_fuse_surface, three launches (two when capacity = 0) over chunks of threads * voxels_per_lane = 1024 consecutive voxels of
 * one group: count (rows per chunk into ws), scan (one workgroup, scan_threads = 1024 chunks a round: chunk bases and offsets),
 * emit (three ballots a slab, one per axis, the popcounts below the lane, the waves' and slabs' sums through LDS).
 * ws: hp_fuse_surface_workspace_bytes(G, nx, ny, nz) = roundup(8 * G * ceil(nx * ny * nz / 1024), 16) bytes, 16-byte aligned.
 * Checked before any HIP call (-1): the grid as above, voxel finite and > 0, min_weight >= 1, capacity >= 0, ws_bytes and the
 * alignment of ws, pointers not NULL (points, normals and cell may be when capacity = 0).
 * hp_fuse_surface_plan: threads, voxels_per_lane, chunks per group = ceil(nx * ny * nz / 1024), scan_threads, scan rounds =
 * ceil(G * chunks / scan_threads).  The workspace and plan queries are host only and answer -1 to bad arguments. */
#define HP_FUSE_MAX_DIM 1024
long long hp_fuse_volume_workspace_bytes(int B, int H, int W);
int hp_fuse_volume_plan(int B, int H, int W, int G, int nx, int ny, int nz, int* threads, int* words, int* blocks_per_group,
                        int* blocks);
int hp_fuse_volume(int B, int H, int W, const void* depth, int depth_is_u16, double scale, const double* K /* (B,4) */,
                   const float* poses /* (B,3,4) */, const unsigned char* mask /* (B,H,W) or NULL */, double near, double far,
                   double jump_abs, double jump_rel, int w, int G, int L, const int* group_images /* (L), device */,
                   const int* group_offsets /* (G+1), device */, const int* host_group_images /* (L), host */,
                   const int* host_group_offsets /* (G+1), host */, const double* origin /* (G,3) */, int nx, int ny, int nz,
                   double voxel, double truncation, float* tsdf /* (G,nz,ny,nx) */, int* weight /* (G,nz,ny,nx) */, void* ws,
                   long long ws_bytes, hpStream_t stream);
long long hp_fuse_surface_workspace_bytes(int G, int nx, int ny, int nz);
int hp_fuse_surface_plan(int G, int nx, int ny, int nz, int* threads, int* voxels_per_lane, int* chunks, int* scan_threads,
                         int* scan_rounds);
int hp_fuse_surface(int G, int nx, int ny, int nz, const float* tsdf, const int* weight, const double* origin /* (G,3) */,
                    double voxel, int min_weight, long long capacity, float* points /* (capacity,3) */,
                    float* normals /* (capacity,3) */, long long* cell /* (capacity) */, long long* offsets /* (G+1) */, void* ws,
                    long long ws_bytes, hpStream_t stream);
/* One step of point-to-point rigid registration (ICP) over ragged sets (csrc/align.hip): what poses a cleaned scan against a
 * template, a ground truth or another view of the same object.  Two ragged sets over the same S sets: the sources, points (T,3)
 * fp32 with offsets (S+1), and the targets, tpoints (U,3) fp32 with toffsets (S+1); rows of other sets never take part.  A job is
 * (set s, hypothesis h < H) with transforms[s][h] (12) fp32, row-major [R | t] = r00 r01 r02 tx r10 ...  Every float operation
 * below is one fp32 rounding in the association written, no contraction (numpy float32 gives the same bits).
 *     transform  x' = ((r00*x + r01*y) + r02*z) + tx, likewise y' and z'.  A source row whose coordinates or p' are not all
 *                finite is absent for this job: index -1, dist2 +inf, no correspondence.
 *     match      the candidates are the rows j of target set s with finite coordinates; d = q - p',
 *                d2 = ((dx*dx + dy*dy) + dz*dz) — hp_knn_points' formula; a NaN d2 counts as +inf; best is the smallest d2, ties
 *                to the lower j; with no candidate below +inf (an overflow included): index -1 and dist2 +inf.
 *     gate       g2 = max_dist * max_dist (+inf allowed).  The row is a correspondence iff index >= 0 and d2 <= g2, inclusive.
 *     quantise   u_c = trunc(ldexp(p'_c - anchor[s]_c, 19 - shift[s])), v_c the same of q: one rounding in the subtraction, an
 *                exact scaling, truncation towards zero.  The correspondence is clipped if any of the six scaled components is
 *                not finite or has magnitude >= 2^20: it is counted in [1] and takes part in no sum.
 *     moments    (S,H,18) int64, exact and therefore free of summation order: [0] correspondences used, [1] clipped,
 *                [2:5] sum u, [5:8] sum v, [8:17] sum u_a*v_b row-major, [17] sum |u - v|^2.  With |u|, |v| < 2^20 and at most
 *                HP_ALIGN_MAX_POINTS = 2^16 rows every sum stays below 2^60.
 *     index, dist2  (H,T) int32 / fp32 or both NULL: the best candidate of every source row, as a row within its target set.
 *                Both are written in full: -1 and +inf for every row of no set and of a set with the empty result.
 *     frame      anchor (S,3) fp32 and shift (S) int32 are the caller's; ops.align_frame builds them from hp_scan_boxes of the
 *                targets: anchor = the box centre (0 where it is not finite); with half = double(scale) * 0.45, half the box's
 *                longest side, and x = half + min(double(max_dist), half): shift = the smallest integer e with x < 2^e, clamped
 *                to [-100, 128], 0 when x is NaN.  A component is clipped at 2^(shift + 1), twice that bound: no target row is
 *                ever clipped, and no gated correspondence while max_dist <= 3 * half.
 * A set is a value, not an error, when it is empty on either side, holds more than HP_ALIGN_MAX_POINTS rows on either side, or
 * its offsets are not 0 <= lo <= hi <= T (U for the targets): it gets the empty result — moments 0, index -1, dist2 +inf — and
 * nothing is read out of range.  T and U are the caller's promise of the rows of points and tpoints.
 * The result is a function of the input alone: integer adds only, no float atomics.  A memset and one launch (two with index),
 * on the caller's stream, no host synchronisation, nothing is allocated; hp_scan_align_workspace_bytes is 0 (-1 on bad arguments).
 * The cost is O(n * m * H) per set.  The rigid fit itself is a host function over the moments (ops.rigid_from_moments).
 * Checked before any HIP call (-1): S >= 1, 1 <= H <= HP_ALIGN_MAX_HYPOTHESES, T, U >= 0, pointers not NULL (index and dist2
 * may be, together), max_dist >= 0 and not NaN.
 *
 * hp_scan_align_plan: threads per workgroup, source rows a lane holds (a workgroup covers threads * rows_per_lane consecutive
 * rows of the ragged source set), hypotheses a lane serves per LDS read (1 for H == 1) and targets per LDS tile.  Host only; -1
 * for H out of range or a NULL pointer. */
#define HP_ALIGN_MAX_POINTS 65536
#define HP_ALIGN_MAX_HYPOTHESES 64
long hp_scan_align_workspace_bytes(int S, int H);
int hp_scan_align_plan(int H, int* threads, int* rows_per_lane, int* hypothesis_group, int* tile);
int hp_scan_align_step(int S, int H, long long T, const float* points, const long long* offsets, long long U,
                       const float* tpoints, const long long* toffsets, const float* transforms /* (S,H,12) */, float max_dist,
                       const float* anchor /* (S,3) */, const int* shift /* (S) */, long long* moments /* (S,H,18) */,
                       int* index /* (H,T) or NULL */, float* dist2 /* (H,T) or NULL */, hpStream_t stream);
/* One step of point-to-plane rigid registration over ragged sets (csrc/align_plane.hip): the step of hp_scan_align_step with the
 * error a depth sensor's captures call for — two captures of one surface never sample the same points, so only the distance along
 * the target's normal measures how far apart they are.  The sets, the jobs, and the rules transform, match, gate, quantise and
 * frame are hp_scan_align_step's — one code, csrc/hp_align.h: index and dist2 are its index and dist2 bit for bit.  tnormals (U,3) fp32 is
 * aligned with tpoints (hp_scan_normals' output).  What a correspondence matched to row j contributes:
 *     normal     n = tnormals[j]; w_c = trunc(ldexp(n_c, 9)).  The correspondence is *without normal* when a scaled component is
 *                not finite or has magnitude >= 2^10, when w.w == 0, or when w.w > 2^18 + 2^11 (not a unit vector): it is counted
 *                in [2] and takes part in no sum.  hp_scan_normals' NaN rows are without normal.
 *     order      of a gated correspondence: clipped first (hp_scan_align_step's rule, counted in [1]), then without normal.
 *     terms      d = u - v, c = u x w, a = (c, w) (6 components), b = -d.w.  With |u_c|, |v_c| < 2^20: |u|_2 < sqrt(3) 2^20,
 *                |d|_2 < sqrt(3) 2^21 and |w|_2 <= sqrt(2^18 + 2^11) < 1.004 * 2^9, so by Cauchy-Schwarz |c|_2 < 2^30 and
 *                |b| < 2^31: both fit 32 bits, and every product a_i a_j, a_i b, b b is below 2^62 in magnitude.
 *     sums       28 exact integers: the 21 a_i a_j (i <= j, row-major), the 6 a_i b, then b b.  Over HP_ALIGN_MAX_POINTS = 2^16
 *                rows a sum can reach 2^78, so each leaves as a pair: per row lo = term & (2^31 - 1) and hi = term >> 31
 *                (arithmetic), summed separately — each stays below 2^48 in magnitude — and the host rebuilds
 *                hi * 2^31 + lo in integers of any width.
 *     moments    (S,H,60) int64: [0] used, [1] clipped, [2] without normal, [3] 0, [4 + 2i] and [5 + 2i] the hi and lo of sum i.
 * The host solves A x = g (ops.rigid_from_plane_moments), A = sum a a^T, g = sum a b, x = (omega, t'): the turn omega about the
 * anchor and the shift t' in units of the frame, the Gauss-Newton step of sum ((R p' + t - q).n)^2.
 * Sets with the empty result, T and U, and what is checked before any HIP call (-1, tnormals not NULL among it) are as for
 * hp_scan_align_step.  The result is a function of the input alone: integer adds only, no float atomics.  A memset and one
 * launch (two with index), on the caller's stream, no host synchronisation, nothing is allocated;
 * hp_scan_align_plane_workspace_bytes is 0 (-1 on bad arguments).
 *
 * hp_scan_align_plane_plan: as hp_scan_align_plan; hypothesis_group is 1 for every H — each (chunk, hypothesis) is a work item of
 * its own, the yaw search stays with hp_scan_align_step.  Host only; -1 for H out of range or a NULL pointer. */
long hp_scan_align_plane_workspace_bytes(int S, int H);
int hp_scan_align_plane_plan(int H, int* threads, int* rows_per_lane, int* hypothesis_group, int* tile);
int hp_scan_align_plane_step(int S, int H, long long T, const float* points, const long long* offsets, long long U,
                             const float* tpoints, const long long* toffsets, const float* tnormals /* (U,3) */,
                             const float* transforms /* (S,H,12) */, float max_dist, const float* anchor /* (S,3) */,
                             const int* shift /* (S) */, long long* moments /* (S,H,60) */, int* index /* (H,T) or NULL */,
                             float* dist2 /* (H,T) or NULL */, hpStream_t stream);
/* Surface normals and surface variation of ragged scans by local principal components (csrc/normals.hip): which way the surface
 * faces at every row, and how far the row's neighbourhood is from flat — what point-to-plane registration and a depth-edge
 * filter start from; a ragged set as for hp_scan_boxes.  Everything is per scan, n_s its rows, and per row i, given neighbour
 * lists index (T,k) int32 of rows within the scan: hp_knn_points' output format, taken as given.
 *     absent     a row with a non-finite coordinate, as above.
 *     neighbourhood  row i itself plus every slot t with 0 <= index[i][t] < n_s whose row is present.  Any other slot is empty:
 *                -1, and garbage too — nothing is read out of range.  Duplicates and a slot equal to i count as listed.
 *                count (T) int32 = the size of the neighbourhood; 0 for an absent row i.
 *     dq         = p_j - p_i per component, one fp32 rounding; row i contributes (0, 0, 0).
 *     frame      hp_scan_plane's: M = the largest |dq_c| over the neighbourhood; e = M's biased exponent field - 127;
 *                q_c = trunc(ldexp(dq_c, 19 - e)): exact, |q_c| < 2^20.
 *     scatter    m = count;  S_a = sum q_a, S_ab = sum q_a q_b: exact integers;  C_ab = m S_ab - S_a S_b, exact in int64.
 *                With m <= 33 (k <= 32): m S_ab <= 33 * 32 * (2^20 - 1)^2 < 2^50.05 and |S_a S_b| <= (32 * (2^20 - 1))^2 < 2^50, so
 *                |C_ab| < 2^51.1 and the trace, three terms 0 <= C_aa <= m S_aa, < 2^51.7: every entry and the trace lie
 *                below 2^53 and convert to fp64 exactly.
 *     undefined  count < 3, M == 0, M not finite (an overflowed dq), or trace == 0: normal = three quiet NaNs (0x7FC00000),
 *                curvature = the same NaN.
 *     eigen      cyclic Jacobi on A = double(C) with V = I: 6 sweeps, no convergence exit, pairs (p, q) in the order (0,1),
 *                (0,2), (1,2), r the third index.  A rotation is skipped only where a_pq == 0 exactly; otherwise
 *                    theta = (a_qq - a_pp) / (2 * a_pq);  t = sgn(theta) / (|theta| + sqrt(theta * theta + 1)), sgn(0) = +1;
 *                    c = 1 / sqrt(t * t + 1);  s = t * c;  h = t * a_pq;
 *                    a_pp = a_pp - h;  a_qq = a_qq + h;  a_pq = 0;
 *                    (a_rp, a_rq) = (c * a_rp - s * a_rq,  s * a_rp + c * a_rq);
 *                    (v_kp, v_kq) = (c * v_kp - s * v_kq,  s * v_kp + c * v_kq) for k = 0, 1, 2
 *                — every + - * / sqrt one fp64 rounding in the association written, no fma, a pair's new values from its old
 *                ones.  An overflowed theta * theta gives t = 0, which is a value.
 *     normal (T,3)  the column of V of the smallest diagonal entry after the sweeps (ties to the lower index), divided by its
 *                length sqrt((x*x + y*y) + z*z) in fp64.  Sign: the component of largest magnitude (ties to the lower axis) is
 *                made positive.  Then, with viewpoints (S,3) fp32: w = double(v_s) - double(p_i),
 *                dot = (nx*wx + ny*wy) + nz*wz, and the normal is negated iff dot < 0 (a NaN dot never flips).  Rounded to fp32.
 *     curvature (T)  the surface variation max(lambda_min, 0) / trace in fp64, rounded to fp32; lambda_min is that smallest
 *                diagonal entry, trace the exact integer trace of C (not the rotated one).  0: flat.  1/3: isotropic.
 * The result is a function of the input alone.  Scans of any length: the cap is the neighbour search's, and the lists of a scan
 * beyond it (all -1) give count 1 and the undefined result by the rules above.  All three outputs are fully written.  One
 * launch, no workspace, no atomics, no host synchronisation.  Checked before any HIP call (-1): S >= 1, 2 <= k <= 32, pointers
 * not NULL (viewpoints may be).
 *
 * hp_scan_normals_plan: the compile-time instance that serves k (lists of 8, 16 or 32 slots held in registers; a k in between
 * uses the next one), threads per workgroup = rows per chunk, and the Jacobi sweeps.  Host only; -1 for k outside [2, 32] or a
 * NULL pointer. */
int hp_scan_normals_plan(int k, int* instance_k, int* threads, int* sweeps);
int hp_scan_normals(int S, const float* points, const long long* offsets, int k, const int* index /* (T,k) */,
                    const float* viewpoints /* (S,3) or NULL */, float* normal /* (T,3) */, float* curvature /* (T) */,
                    int* count /* (T) */, hpStream_t stream);
/* Global registration of ragged scans (csrc/features.hip, csrc/pose_trials.hip): descriptors, their nearest
 * matches and a consensus over matched triples — a start for hp_scan_align_step / hp_scan_align_plane_step from any relative
 * pose.  tests/feature_law.py and tests/pose_trials_law.py state the laws in numpy; only IEEE + - * / sqrt, comparisons, floor
 * and trunc appear in them, so no library function decides a bit.
 *
 * hp_scan_features: fast point feature histograms, per scan and per row i, given points, normals (T,3) fp32 row for row and
 * lists index (T,k) int32 of rows within the scan (hp_knn_points' format), 1 <= k <= 32.
 *     usable     a row with finite coordinates and a finite normal that is not (0, 0, 0).  Normals are taken as given.
 *     listed     slot t with 0 <= j = index[i][t] < n_s, j != i and row j usable; any other slot is empty, garbage too.
 *     d          = p_j - p_i per component, one fp32 rounding.  Everything below is fp64, one rounding per operation in the
 *                association written, no fma;  dot(a, b) = (a0*b0 + a1*b1) + a2*b2;  cross(a, b)_0 = a1*b2 - a2*b1 and cyclic.
 *     pair       of a usable row i and a listed j, d2 = dot(d, d); skipped if a component of d is not finite or d2 == 0.  The
 *                source is j iff |dot(n_j, d)| > |dot(n_i, d)|, and then d is negated; ns, nt the source's and target's normal.
 *                    phi = dot(ns, d) / sqrt(d2);  v = cross(d, ns);  vn = sqrt(dot(v, v));  skipped if vn == 0;  v = v / vn;
 *                    w = cross(ns, v);  alpha = dot(v, nt);  y = dot(w, nt);  x = dot(ns, nt)
 *     bins       alpha, phi: floor((11 * (f + 1)) / 2) clamped to [0, 10].  theta, the angle of (x, y) over (-pi, pi] in 11 equal
 *                bins, by sign tests against the ten directions (c_k, s_k) = (cos, sin)(-pi + 2 pi (k + 1) / 11), k = 0..9,
 *                tabulated as hex-float literals in features.hip and feature_law.py: with cr_k = c_k * y - s_k * x the bin is
 *                5 + #{k in 5..9: cr_k >= 0} where y >= 0 (-0.0 is 0) and #{k in 0..4: cr_k >= 0} where y < 0; x = y = 0: bin 5.
 *     SPFH(i)    33 counts (theta, alpha, phi) and m_i, the pairs not skipped: a record of 36 bytes [33 counts, m_i, 0, 0].
 *     FPFH(i)    for m_i > 0, over the slots in list order with 0 <= j < n_s, j != i, m_j > 0, d finite and d2 != 0:
 *                w_j = 1 / d2;  W = W + w_j;  c_j = w_j / m_j;  A_b = A_b + c_j * SPFH(j)_b.  F_b = SPFH(i)_b / m_i + A_b / W (the
 *                second term only where a slot took part); per group of 11 bins, sum = F_0 + .. + F_10 in bin order and
 *                byte_b = trunc((255 * F_b) / sum).
 *     features (T,36) uint8, bytes 33..35 zero; count (T) int32 = m_i.  A row with count 0 — not usable, without a valid pair,
 *                or a row of no scan — has 36 zero bytes and no descriptor.
 * Two launches, one lane per row; ws holds T * 36 bytes (hp_scan_features_workspace_bytes), the SPFH records; no atomics, no
 * LDS.  Checked before any HIP call (-1): S >= 1, T >= 0, 1 <= k <= 32, pointers not NULL, features and ws on 4 bytes.
 * hp_scan_features_plan: the compile-time list length that serves k (8, 16 or 32), threads per workgroup, bytes a descriptor.
 *
 * hp_scan_feature_match: two ragged descriptor sets over the same S sets.  For every source row with counts > 0: the target
 * row of set s with tcounts > 0 at the smallest squared distance over the 36 bytes — an exact integer, at most
 * 33 * 255^2 < 2^22, formed as |a|^2 + |b|^2 - 2 a.b —, ties to the lower row: match (T) int32 the row within the target set,
 * dist (T) int32.  Without a descriptor or a candidate both are -1.  A set is a value, not an error, when it is empty on
 * either side, holds more than HP_ALIGN_MAX_POINTS rows on either side, or its offsets are not 0 <= lo < hi <= rows: the empty
 * result.  One launch.  Checked before any HIP call (-1): S >= 1, T, U >= 0, pointers not NULL (those of an empty side may be),
 * descriptors on 4 bytes.  hp_scan_feature_match_plan: threads, source rows per lane, target records per LDS tile.
 *
 * hp_scan_pose_trials: per set with n source and m target rows, match (T) as above.
 *     matched    a source row with 0 <= match < m whose coordinates and whose target row's are finite.
 *     draws      Philox4x32-10, key = seed, counter (streams[s] lo, hi, q, 5) — hp_scan_plane's scheme under tag 5; streams NULL:
 *                s.  Trial h < trials samples the rows r_k = (word[3h+k] * n) >> 32; a, b, c those rows, a', b', c' their targets.
 *     valid      iff the three rows are matched and differ; their targets differ; for the sides (a,b), (a,c), (b,c), with
 *                l2 = ((dx*dx + dy*dy) + dz*dz) of the fp32 difference: both l2 finite, ls2 >= rho2 * lt2 and lt2 >= rho2 * ls2,
 *                every operation one fp32 rounding, rho2 = fp32(edge_ratio^2) from the caller; both triangles have a frame; the
 *                12 fp32 of the transform are finite.
 *     frame      fp64, one rounding per operation:  u = b - a, v = c - a;  l1 = sqrt(dot(u, u)) > 0;  e1 = u / l1;
 *                x = cross(e1, v), dot(x, x) > 2^-24 * dot(v, v);  e3 = x / sqrt(dot(x, x));  e2 = cross(e3, e1);
 *                centre = ((a + b) + c) / 3.
 *     fit        R_ij = (e1t_i * e1s_j + e2t_i * e2s_j) + e3t_i * e3s_j;  t_i = ct_i - ((R_i0*cs_0 + R_i1*cs_1) + R_i2*cs_2);
 *                [R | t] row-major rounded to fp32: a start, not a least-squares fit.
 *     kept       the first `keep` valid trials in ascending h (an ordered compaction).  valid (S) = the number of valid
 *                trials, kept (S) = min(valid, keep).
 *     score      of a kept trial: the matched rows with d2 <= g2 and d2 finite, p' = hp_scan_align_step's fp32 transform of
 *                the row, d2 = its fp32 squared distance to the row's target; g2 = inlier_dist * inlier_dist in fp32, +inf allowed.
 *     winner     the most inliers, ties to the lower h: trial (S), inliers (S), transform (S,12), found = inliers >= min_inliers.
 *                Without a kept trial: -1, 0, twelve quiet NaNs, 0.  Sets with the empty result: hp_scan_feature_match's.
 * Three launches (draw and compact, score, winner); integer adds and an integer max only.  ws holds
 * hp_scan_pose_trials_workspace_bytes on a 16-byte boundary.  Checked before any HIP call (-1): S >= 1, T, U >= 0,
 * 1 <= trials <= HP_POSE_MAX_TRIALS, 1 <= keep <= HP_POSE_MAX_KEEP, 0 <= rho2 <= 1, inlier_dist >= 0, min_inliers >= 0,
 * pointers not NULL (streams may be, and those of an empty side).
 * hp_scan_pose_trials_plan: threads, source rows per lane of the score kernel, transforms per LDS tile. */
#define HP_POSE_MAX_TRIALS 65536
#define HP_POSE_MAX_KEEP 4096
int hp_scan_features_plan(int k, int* instance_k, int* threads, int* width);
long hp_scan_features_workspace_bytes(long long T);
int hp_scan_features(int S, long long T, const float* points, const long long* offsets, const float* normals /* (T,3) */, int k,
                     const int* index /* (T,k) */, unsigned char* features /* (T,36) */, int* count /* (T) */, void* ws,
                     hpStream_t stream);
int hp_scan_feature_match_plan(int* threads, int* rows_per_lane, int* tile);
int hp_scan_feature_match(int S, long long T, const unsigned char* features /* (T,36) */, const long long* offsets, long long U,
                          const unsigned char* tfeatures /* (U,36) */, const long long* toffsets, const int* counts /* (T) */,
                          const int* tcounts /* (U) */, int* match /* (T) */, int* dist /* (T) */, hpStream_t stream);
int hp_scan_pose_trials_plan(int trials, int keep, int* threads, int* rows_per_lane, int* tile);
long hp_scan_pose_trials_workspace_bytes(int S, int keep);
int hp_scan_pose_trials(int S, long long T, const float* points, const long long* offsets, long long U, const float* tpoints,
                        const long long* toffsets, const int* match /* (T) */, const long long* streams /* (S) or NULL */,
                        unsigned long long seed, int trials, int keep, float rho2, float inlier_dist, int min_inliers,
                        int* trial, int* inliers, int* found, float* transform /* (S,12) */, int* valid, int* kept, void* ws,
                        hpStream_t stream);
/* Cut by coordinate rank (csrc/axis_split.hip): each of B clouds (B,n,3) fp32 sorted along one axis and split at row k, in
 * one launch, one workgroup per cloud — core/experiments.py:149-152 (`gt[gt.T[0].argsort()[1024:]]` / `[:1024]`) for a batch.
 * Per cloud, with c_i the `axis` coordinate of row i:
 *     order      = the permutation that sorts the rows by (key(c_i), i) ascending.  key is numpy's float32 `<` order: -0.0 and
 *                  +0.0 are equal, -inf is first and +inf last among the numbers, every NaN (either sign, any payload) comes
 *                  after +inf; equal keys — NaNs among themselves included — keep ascending i.
 *                  This is np.argsort(c, kind='stable').
 *     lower      = rows order[0..k), upper = rows order[k..n): each output row is bit for bit a row of the cloud, all three
 *                  coordinates, NaN payloads included.
 * order (B,n) int32 or NULL (not written; lower and upper are the same either way).  A cloud's result depends on its own rows,
 * on axis and on k only — not on B or on its place in the batch.  The reference's argsort is numpy's default, not stable: the
 * two agree exactly whenever the coordinate has no duplicates, and the reference leaves the rest unspecified.
 * Checked before any HIP call (-1): B >= 0 (0: nothing to do), 2 <= n <= HP_AXIS_SPLIT_MAX_POINTS, 1 <= k <= n-1, axis in
 * {0,1,2}, clouds, lower and upper not NULL. */
#define HP_AXIS_SPLIT_MAX_POINTS 8192
int hp_axis_split(int B, int n, const float* clouds /* (B,n,3) */, int axis, int k,
                  float* lower /* (B,k,3) */, float* upper /* (B,n-k,3) */, int* order /* (B,n) or NULL */,
                  hpStream_t stream);
/* Triangle meshes (csrc/mesh.hip): K meshes are K vertex arrays verts (K,V,3) fp32 over ONE face list faces (F,3) int32 — what a
 * triangulated sphere gives when it is decoded K times.  1 <= F <= HP_MESH_MAX_FACES; every face index must lie in [0,V): the
 * kernels do not check it (hyperpocket_amd/ops.py does, on the host, when it first sees a face list).
 *
 * hp_mesh_sample: n points per mesh, uniform by area, in one launch.  The law is exact and does not depend on the launch
 * geometry; every floating operation below is ONE IEEE fp64 rounding, no contraction (tests/mesh_law.py states it in numpy
 * and Python integers).  Per mesh k, with a, b, c the corners of face f widened to fp64:
 *     e1 = b - a, e2 = c - a;  cx = e1y*e2z - e1z*e2y, cy = e1z*e2x - e1x*e2z, cz = e1x*e2y - e1y*e2x (products rounded,
 *          then the difference);  d_f = sqrt((cx*cx + cy*cy) + cz*cz), and a d_f that is not finite counts as 0
 *     d_max = max_f d_f.  d_max == 0: failed[k] = 1, area[k] = 0, the mesh's rows of points and face are 0, nothing else is
 *          computed.  Otherwise failed[k] = 0 and, with frexp(d_max) = (m, e):
 *     w_f  = (uint64) floor(ldexp(d_f, 40 - e)), so w_max is in [2^39, 2^40) and W = sum_f w_f < 2^55.  Prefix sums of w are
 *          integer sums, the same in any order: a parallel scan and a sequential one agree to the bit
 *     area[k] = ldexp((double) W, e - 41): the mesh's area to 2^-39 relative per face
 *     sample j: (x0, x1, x2, x3) = Philox4x32-10 with key = seed (lo, hi) and counter (streams[k] lo, streams[k] hi, j, 3) —
 *          the (stream, q, tag) scheme of hp_prepare_scans (tags 0, 1) and hp_make_batch (tags 0-2) under a tag of its own
 *          r = mulhi64(x0 << 32 | x1, W);  face[k,j] = the smallest f whose inclusive prefix w_0 + .. + w_f exceeds r, so a
 *          face is drawn with probability w_f / W up to 2^-64 W and a zero-weight face never
 *          u = x2 * 2^-32, v = x3 * 2^-32; where u + v > 1, u = 1 - u and v = 1 - v (all exact)
 *          points[k,j] = (a + u*e1) + v*e2 per coordinate in fp64, rounded to fp32 once
 * A mesh's result depends on its own vertices, the faces, n, seed and streams[k] only.  Power-of-two scaling of the vertices
 * leaves face unchanged (short of overflow and underflow).  A NaN or infinite vertex zeroes the weight of its faces only.
 * points (K,n,3) fp32, face (K,n) int32, area (K) fp64, failed (K) int32: all written in full.
 * ws: hp_mesh_sample_workspace_bytes(K, F, n) bytes, 8-byte aligned; may be NULL when that is 0 (F <= 8192: the table of
 * weights is in LDS).  Its contents are scratch.
 * Checked before any HIP call (-1): 0 <= K <= 65535 (0: nothing to do), 1 <= V <= 2^24, 1 <= F <= HP_MESH_MAX_FACES,
 * 1 <= n <= 2^24, every pointer but ws not NULL, ws not NULL where the workspace is needed.
 *
 * hp_mesh_sample_plan: threads per workgroup, sample slices per mesh (the grid is slices x K; every slice builds the mesh's
 * table) and whether the table is in LDS (1) or in ws (0), under the current hooks.  Host only.
 * [test hooks: process-wide, not read from the environment] hp_mesh_sample_set_slices(s): 1 <= s <= 1024 forces s slices
 * (capped by n), 0 = the launcher's choice (default).  hp_mesh_sample_set_lds_faces(faces): meshes of more than `faces` faces
 * use ws; 0 <= faces <= 8192 (default 8192; 0 sends every mesh to ws).  Both return the previous setting, -1 (and no change)
 * for a value out of range.  The results are the same bits under every setting: that is what the hooks are there to show.
 *
 * hp_mesh_normals: unit normals.  The (cx, cy, cz) above is face f's area-weighted normal.  vertex_normal (K,V,3): the fp64
 * sum, starting from +0, of the cross products of vertex v's incident faces vf_faces[vf_offsets[v] .. vf_offsets[v+1]) in that
 * order (ascending faces: utils/sphere_mesh.py vertex_faces), each component then divided by the sum's length
 * sqrt((sx*sx + sy*sy) + sz*sz) and rounded to fp32; a zero or non-finite length gives (0,0,0).  No atomics: one order, one
 * result.  face_normal (K,F,3) or NULL: (cx, cy, cz) normalised the same way.  vf_offsets (V+1) int32 ascending from 0,
 * vf_faces (vf_offsets[V]) int32 in [0,F): not checked here either.
 * Checked before any HIP call (-1): K, V, F as above; verts, faces, vf_offsets, vf_faces, vertex_normal not NULL. */
#define HP_MESH_MAX_FACES 32768
int hp_mesh_sample(int K, int V, const float* verts, int F, const int* faces, int n, unsigned long long seed,
                   const long long* streams /* (K) */, float* points /* (K,n,3) */, int* face /* (K,n) */,
                   double* area /* (K) */, int* failed /* (K) */, void* ws, hpStream_t stream);
long hp_mesh_sample_workspace_bytes(int K, int F, int n);
int hp_mesh_sample_plan(int K, int F, int n, int* threads, int* slices, int* in_lds);
int hp_mesh_sample_set_slices(int s);
int hp_mesh_sample_set_lds_faces(int faces);
int hp_mesh_normals(int K, int V, const float* verts, int F, const int* faces, const int* vf_offsets, const int* vf_faces,
                    float* face_normal /* (K,F,3) or NULL */, float* vertex_normal /* (K,V,3) */, hpStream_t stream);
/* KLD term of core/epoch_loops.py:29-30 and its gradients */
int hp_kld_forward(long n, int batch, const float* explv, const float* mu, float* out, hpStream_t stream);
int hp_kld_backward(long n, int batch, const float* explv, const float* mu, const float* grad_out, float* grad_explv,
                    float* grad_mu, hpStream_t stream);
/* TrainEngine glue — the step's scalar loss terms in one launch (core/epoch_loops.py:26-31 + the optional EMD term):
 * out[0] = loss_r = c_cd*cd[0], out[1] = loss_kld = kld[0], out[2] = loss_emd = c_emd * sum_b cost[b], out[3] = their sum.
 * kld / cost may be NULL (term absent). */
int hp_step_losses(int b, const float* cd, const float* kld, const float* cost, float c_cd, float c_emd, float* out /* 4 */,
                   hpStream_t stream);

/* torch.optim.Adam(lr, betas, eps, weight_decay=0, amsgrad=False) over n contiguous fp32 parameters (core/main.py:62-66) */
int hp_adam_step(long n, float* p, const float* g, float* m, float* v, float lr, float beta1, float beta2, float eps,
                 int step, float grad_scale, hpStream_t stream);

/* Exact t-SNE (csrc/tsne.hip; the executable law and its error bars are tests/tsne_law.py).  All five are
 * asynchronous on `stream`, use no float atomics — two runs give the same bits — and check, before any HIP call (-1):
 * 2 <= n <= HP_TSNE_MAX_POINTS, d >= 1, ldx >= d, 0 < perplexity < n, every pointer not marked optional not NULL.
 *
 * hp_pairwise_sqdist: D[i][j] = sum_k (x_ik - x_jk)^2 for X (n, d) with row stride ldx, D (n, n) fp32 — differences first,
 * never the Gram expansion.  In fp32: the terms of k-chunk q (columns q*kchunk .. of hp_pairwise_sqdist_plan) go down one
 * chain s = fmaf(t, t, s) from +0 in column order, and the chunk sums are added in chunk order from +0.  D is bit-symmetric
 * with an exactly zero diagonal; every element is within (kchunk + ceil(d / kchunk) + 4) 2^-24 of the exact sum, relatively.
 * hp_pairwise_sqdist_plan: the tile (rows per workgroup side) and kchunk the launcher uses; host only.
 *
 * hp_tsne_affinities: per row i, with m_i the smallest off-diagonal D[i][j] and e_ij = D[i][j] - m_i (the diagonal left
 * out), the search for beta_i: start at 1; H = log(sum_j p_j) + beta sum_j e_ij p_j / sum_j p_j with p_j = exp(-beta e_ij);
 * stop when |H - log(perplexity)| <= 1e-5 or after 100 evaluations; H too large: beta doubles until a step was too small,
 * then bisects; H too small: beta halves until a step was too large, then bisects.  beta[i] is the beta of the last
 * evaluation, steps[i] the number of evaluations.  C_ij = p_j / sum p; P = max((C + C^T) / sum(C + C^T), 2^-52) with a zero
 * diagonal, (n, n) fp32, bit-symmetric.  ws: hp_tsne_affinities_workspace_floats(n) floats; on return it holds C (n, n), its
 * n row sums and sum(C + C^T).
 *
 * hp_tsne_gradient: one pass over the pairs of the embedding Y (n, 2) under P (n, n), of which only row i is read for row
 * i.  With w_ij = 1 / (1 + |y_i - y_j|^2), j != i, rowacc (n, 8) receives per row [0..1] sum_j (exaggeration P_ij) w_ij
 * (y_i - y_j), [2..3] sum_j w_ij^2 (y_i - y_j), [4] z_i = sum_j w_ij and, with kl not NULL, [5] sum_j P_ij (log P_ij - log
 * w_ij) over P_ij > 0 and [6] sum_j P_ij; [7] is not written.  kl (3) or NULL: KL = sum_i [5] + log(Z) sum_i [6], Z = sum_i
 * z_i, sum P.
 *
 * hp_tsne_update: Z = the n z_i added in one fixed order; g = 4 (attractive - repulsive / Z); then in fp32, each operation
 * rounded once: inc = update * g < 0; gains = inc ? gains + 0.2f : gains * 0.8f; gains = max(gains, min_gain);
 * update = momentum * update - lr * (g * gains); Y += update.  Y, update, gains (n, 2) in place; grad (n, 2) or NULL: g.
 *
 * hp_tsne_descend: iterations it0 .. it0 + iters - 1 as gradient + update launches with min_gain 0.01, no host
 * synchronisation, no convergence test; an iteration below `explore` uses `exaggeration` and momentum 0.5, a later one
 * exaggeration 1 and momentum 0.8.  kl_out (3) or NULL: hp_tsne_gradient's kl of the final Y, at exaggeration 1. */
#define HP_TSNE_MAX_POINTS 16384
int hp_pairwise_sqdist(int n, int d, const float* X, long ldx, float* D /* (n,n) */, hpStream_t stream);
int hp_pairwise_sqdist_plan(int n, int d, int* tile, int* kchunk);
long hp_tsne_affinities_workspace_floats(int n);
int hp_tsne_affinities(int n, const float* D, float perplexity, float* P /* (n,n) */, float* beta /* (n) */,
                       int* steps /* (n) */, float* ws, hpStream_t stream);
int hp_tsne_gradient(int n, const float* P, float exaggeration, const float* Y /* (n,2) */, float* rowacc /* (n,8) */,
                     float* kl /* (3) or NULL */, hpStream_t stream);
int hp_tsne_update(int n, const float* rowacc, float* Y, float* update, float* gains, float momentum, float lr,
                   float min_gain, float* grad /* (n,2) or NULL */, hpStream_t stream);
int hp_tsne_descend(int n, const float* P, float* Y, float* update, float* gains, float* rowacc, int it0, int iters,
                    int explore, float exaggeration, float lr, float* kl_out /* (3) or NULL */, hpStream_t stream);

/* ------------------------------------------------------------------------------------------
 * Exact EMD over a list of cloud pairs: the minimum-cost one-to-one matching of A[a] against B[b]
 * (csrc/assign.hip; the executable law is tests/assign_law.py and the kernel follows it bit for bit).
 * A (na, n, 3), B (nb, n, 3) — equal point counts only; pair_ab (pairs, 2) int32 as for hp_cloud_pairs.
 *   q(i, j)       = rint(sqrt_f32(((dx*dx + dy*dy) + dz*dz)) * 2^scale_log2), every operation one fp32 rounding, the root
 *                   correctly rounded, ties to even; a q that is not <= 2^30 is an overflow
 *   assignment[p] (n) the object j of B[b] matched to every point i of A[a], a permutation that minimises sum_i q(i, j_i);
 *                 NULL: not written
 *   cost[p]       that minimum, int64: the distance sum is cost / 2^scale_log2
 *   rounds[p]     the auction rounds the pair took (> 0), or its status:
 *                   -1 the round bound was exhausted   -2 a pair index lies outside its set (nothing is read out of range)
 *                   -3 a quantised distance overflowed
 *                 with a status, cost[p] = -1 and the assignment row is -1; the other pairs are unaffected.
 * A forward Jacobi auction with eps-scaling (theta = 4) in int64, one workgroup per pair, all state in LDS (60 bytes per
 * point), integer max / min atomics only: a pair's outputs depend on its two clouds, scale_log2 and max_rounds alone, not
 * on its place in the list, on `pairs` or on the launch.  Workgroups stride over the list: pairs is no grid dimension.
 * max_rounds bounds every pair's loop; 0 = hp_assign_default_max_rounds(n) = 256 n + 1024, at least 8 times the largest
 * round count of the law over the families of tests/test_assign_law_host.py (-1 for n outside [1, HP_ASSIGN_MAX_POINTS]).
 * Sizes, NULLs, n outside [1, HP_ASSIGN_MAX_POINTS], scale_log2 outside [0, 24] and max_rounds outside [0, 2^31) are checked
 * (-1) before any HIP call; pairs == 0 is a no-op.
 * ------------------------------------------------------------------------------------------ */
#define HP_ASSIGN_MAX_POINTS 2048
long hp_assign_default_max_rounds(int n); /* host only */
int hp_assign_pairs(int na, int n, const float* A, int nb, const float* B, long pairs, const int* pair_ab, int scale_log2,
                    long max_rounds, int* assignment /* (pairs,n) or NULL */, long long* cost /* (pairs) */,
                    int* rounds /* (pairs) */, hpStream_t stream);

/* ------------------------------------------------------------------------------------------
 * Point-cloud previews: depth-buffered splats (csrc/render.hip; the executable law is tests/render_law.py
 * and the kernel follows it bit for bit).  B clouds points (B,n,3) under V views (V,3,4) fp32 — device memory, shared by all
 * clouds — give image (B,V,H,W,3) uint8 and, unless NULL, ids (B,V,H,W) int32.  The n points of a cloud fall into L <= 8
 * layers by the cumulative ends layer_ends (L), non-decreasing, layer_ends[L-1] == n: point i belongs to the first layer whose
 * end exceeds i; a layer may be empty.  HOST arrays, read before the call returns: layer_ends (L), palette (L,3) uint8,
 * radius2 (L) in [0, HP_RENDER_MAX_RADIUS2], background (3) uint8.  Per image, with M the view:
 *   projection  t_k = ((M[k,0]*x + M[k,1]*y) + M[k,2]*z) + M[k,3], each operation one fp32 rounding -> u, v, w
 *   cull        a point is dropped if u, v or w is not finite, or unless -9 <= u < W+9 and -9 <= v < H+9 (fp32 comparisons)
 *   raster      px = floor(u), py = floor(v), zq = (int)min(max(floor(w * 2^24), 0), 2^24 - 1), clamped in fp32
 *   key         (zq << 32) | i
 *   splat       every (dx,dy) with dx*dx + dy*dy <= radius2[layer(i)]: pixel (px+dx, py+dy), if inside the image, keeps the
 *               smallest key — the nearest depth, and at equal zq the lower index
 *   resolve     no key: background, ids -1.  Otherwise shade = 255 - (((zq >> 16) * fog) >> 8), channel c =
 *               (palette[layer][c] * shade + 127) / 255, ids = i.
 * One launch, one workgroup per (cloud, view, tile) with the tile's keys in LDS and 64-bit integer LDS atomics only: the
 * result depends on the inputs alone, not on the tile size or the launch.  Every output byte is written.
 * Checked before any HIP call (-1): B, n, V, W, H >= 1; W, H <= HP_RENDER_MAX_SIDE; 1 <= L <= HP_RENDER_MAX_LAYERS; layer_ends
 * as above; radius2 and fog (0..255) in range; every pointer but ids not NULL; B * V * tiles < 2^31.
 *
 * hp_render_points_plan: the launch for (B, V, W, H) under the current hook — tile size (the image's own where that is
 * smaller), tiles per image = tiles_x * tiles_y (tile t covers columns (t % tiles_x) * tile_w .. and rows (t / tiles_x) *
 * tile_h .., cut at the image edge), threads per workgroup, workgroups and bytes of LDS per workgroup.  Host only.
 * [test hook: process-wide, not read from the environment] hp_render_points_set_tile(side): side 8, 16, 32, 64 or 128, 0 =
 * the launcher's choice (default).  Returns the previous setting, -1 (and no change) for another value.
 * ------------------------------------------------------------------------------------------ */
#define HP_RENDER_MAX_LAYERS 8
#define HP_RENDER_MAX_RADIUS2 64
#define HP_RENDER_MAX_SIDE 4096
typedef struct HpRenderPlan {
    int tile_w, tile_h, tiles_x, tiles_y, tiles, threads, lds_bytes;
    long long workgroups;
} HpRenderPlan;
int hp_render_points(int B, int n, const float* points, int V, const float* views, int L, const int* layer_ends,
                     const unsigned char* palette, const int* radius2, int fog, const unsigned char* background, int W, int H,
                     unsigned char* image /* (B,V,H,W,3) */, int* ids /* (B,V,H,W) or NULL */, hpStream_t stream);
int hp_render_points_plan(int B, int V, int W, int H, HpRenderPlan* plan);
int hp_render_points_set_tile(int side);

#ifdef __cplusplus
}
#endif
#endif /* HYPERPOCKET_HIP_H */
