/*
 * bm_gar.h — C ABI of libbm_gar.so, the MI355X (gfx950) implementation of the
 * Byzantine-robust gradient-aggregation hot path of LPD-EPFL/ByzantineMomentum.
 *
 * This is the drop-in boundary. Every entry point is what the reference's
 * `native` hook (aggregators/krum.py:22-26,82-96; bulyan.py:22-26,86-100;
 * median.py:22-26,41-49; brute.py:23-27,82-91) or its registry
 * (aggregators/__init__.py:71-86) would bind through an FFI for this path.
 * The reference-side binding (a ctypes stub) is shown in INTEGRATION.md.
 *
 * Conventions
 *   - `rows`   : HOST array of n DEVICE pointers, one per worker gradient
 *                (reference: `gradients: list[Tensor(d)]`, entries may alias,
 *                attacks/identical.py:86). Never written. n <= BM_MAX_ROWS.
 *   - `d`      : coordinates per gradient (fp32, contiguous).
 *   - `out`    : DEVICE pointer, caller-allocated, never aliases an input
 *                (aggregators/__init__.py:19).
 *   - `stream` : hipStream_t of the caller (torch.cuda.current_stream().cuda_stream);
 *                every launch goes there, no entry point synchronises the device.
 *   - return   : 0 on success; a negative value -hipError_t on a HIP failure;
 *                BM_EINVAL for an argument the kernels cannot serve.
 *   - The library owns no memory across calls; workspaces are caller-owned and
 *     sized by bm_workspace_bytes().
 */
#ifndef BM_GAR_H
#define BM_GAR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BM_MAX_ROWS 64
#define BM_EINVAL   (-100000)
#define BM_ENOCOMM  (-100001) /* RCCL is not available in this process      */
#define BM_ECOMM    (-100002) /* an RCCL call failed                        */

/* Column-wise rules (coordinate-per-coordinate over the worker axis). */
enum bm_colwise_op {
  BM_OP_MEDIAN = 0, /* aggregators/median.py:31-39  lower median, rank (n-1)//2      */
  BM_OP_TRMEAN = 1, /* aggregators/trmean.py:24-33  mean of sorted ranks f..n-f-1    */
  BM_OP_PHOCAS = 2, /* aggregators/trmean.py:81-94  n-f closest to the trimmed mean  */
  BM_OP_MEAMED = 3  /* aggregators/trmean.py:96-109 n-f closest to the median        */
};

/* ABI version of this header; bumped on any signature change (23 also covers the additions that say so below). */
int bm_abi_version(void);
/* TEST / MEASUREMENT ONLY — not part of the drop-in surface.  Sets one launch-shape knob by the name of its environment
 * variable (BM_COL_BURST, BM_PAIR_MODE, BM_BRUTE_BUDGET, ...: csrc/bm_common.h, struct Tuning) for the calls that
 * follow, so that an A/B of two settings can alternate inside one process; results never depend on a knob.  The knobs
 * are the library's only process-global mutable state ("no global mutable state besides a workspace
 * cache"): they are read from the environment once, and a production process never calls this.  No locking: the
 * caller must not run it concurrently with any other entry point.  BM_EINVAL for an unknown name. */
int bm_tuning_set(const char* name, int value);

/* Human-readable text for a code returned by any entry point. */
const char* bm_error_string(int code);

/* out[j] = op over {rows[i][j]}_i, 0 <= j < d.  f ignored for BM_OP_MEDIAN. */
int bm_colwise(int op, const float* const* rows, int n, int64_t d, int f,
               float* out, void* stream);

/* Workspace sizes (bytes) for the entry points below. kind: */
enum bm_ws_kind {
  BM_WS_PAIRWISE = 0, /* bm_pairwise_sqdist            */
  BM_WS_AKSEL    = 1, /* bm_aksel_pass1                */
  BM_WS_STATS    = 2, /* bm_stack_stats                */
  BM_WS_DOT      = 3, /* bm_multi_dot                  */
  BM_WS_STEP     = 4, /* bm_momentum_stats             */
  BM_WS_STUDY    = 5  /* bm_study_stats                */
};
int64_t bm_workspace_bytes(int kind, int n, int64_t d);

/* sq[i*n+j] = sum_k (rows[i][k]-rows[j][k])^2 as fp64, full symmetric n x n matrix,
 * zero diagonal.  Replaces the n(n-1)/2 x (sub, norm, .item()) loop of
 * aggregators/krum.py:41-48, bulyan.py:48-54, brute.py:43-45 (which take sqrt on top).
 * Deterministic: bitwise-equal rows give bitwise-equal distances.
 */
int bm_pairwise_sqdist(const float* const* rows, int n, int64_t d,
                       double* sq_nxn, void* ws, void* stream);

/* The same over ONE SHARD of a dimension-partitioned stack: d coordinates here, d_total >= d over
 * all shards.  The partial matrices of the shards add up to the matrix of the whole rows; the precision
 * plan of the pass (how each fp32 value is split for the matrix cores) follows d_total, so a job gives the
 * same plan whatever its world size.  bm_pairwise_sqdist(rows, n, d, ...) is this with d_total = d. */
int bm_pairwise_sqdist_shard(const float* const* rows, int n, int64_t d, int64_t d_total,
                             double* sq_nxn, void* ws, void* stream);

/* Score + stable rank on the device (one workgroup), from the squared distances.
 * mode BM_RANK_KRUM  : score_i = sum of the (n-f-1) smallest distances of row i
 *                      (aggregators/krum.py:50-62)
 * mode BM_RANK_BULYAN: score_i = sum of the m smallest distances of row i
 *                      (aggregators/bulyan.py:56-62)
 * Distances are sqrt(sq) in fp64, non-finite -> +inf (krum.py:46-47); sums are
 * fp64 in ascending order; order_out is the stable (lower index first) argsort of
 * the scores.  scores_out (n doubles) may be NULL. */
enum bm_rank_mode { BM_RANK_KRUM = 0, BM_RANK_BULYAN = 1 };
int bm_krum_rank(const double* sq_nxn, int n, int f, int m, int mode,
                 int32_t* order_out, double* scores_out, void* stream);

/* bm_pairwise_sqdist_shard + bm_krum_rank as one call for a single GPU (nothing to exchange between the two): the
 * third launch of the distance pass — the gated exact pass, which has nothing to do unless the accuracy gate listed
 * rows — ranks the rows from the final distances, so the ranking costs no launch of its own.  Same sq_nxn,
 * order_out, scores_out as the two calls.  ws as bm_pairwise_sqdist. */
int bm_pairwise_rank(const float* const* rows, int n, int64_t d, int64_t d_total, int f, int m, int mode,
                     double* sq_nxn, int32_t* order_out, double* scores_out, void* ws, void* stream);

/* out = (((0 + rows[idx[0]]) + rows[idx[1]]) + ...)/m, sequential fp32 like
 * `sum(...).div_(m)` at aggregators/krum.py:80, brute.py:80, aksel.py:64.
 * idx is a DEVICE array of m int32 (so no host sync between rank and mean).  A NEGATIVE entry means "there is no
 * selection" (bm_brute_select_device, status -2): out is then NaN everywhere. */
int bm_selected_mean(const float* const* rows, int n, const int32_t* idx, int m,
                     int64_t d, float* out, void* stream);

/* Bulyan pass 2 (aggregators/bulyan.py:64-84 with static scores): with
 * m_max = n-f-2, theta = n-2f-2, beta = theta-2f, for every coordinate
 *   sel[i] = mean(rows[order[i .. i+min(m, m_max-i)-1]]),  i < theta
 *   out    = mean of the beta values of sel closest to the lower median of sel.
 * order is the DEVICE output of bm_krum_rank(mode BULYAN). */
int bm_bulyan_pass2(const float* const* rows, int n, const int32_t* order, int f, int m,
                    int64_t d, float* out, void* stream);

/* Aksel pass 1 (aggregators/aksel.py:35-41): coordinate-wise lower median
 * (written to median_out if non-NULL) and sq[i] = sum_j (rows[i][j]-median[j])^2. */
int bm_aksel_pass1(const float* const* rows, int n, int64_t d, float* median_out,
                   double* sq_out, void* ws, void* stream);

/* tools/pytorch.py:97-125 in one pass: avg_out = sequential mean of the k rows;
 * out3 = { sum_j avg_j^2, sum_i sum_j (rows[i][j]-avg_j)^2, max_j |avg_j| }.
 * If scaled_out is non-NULL it receives avg + scale * (-avg) in the same pass, rounded like the
 * reference's `grad_att = grad_avg.neg(); grad_att.mul_(factor); byz = grad_avg.add_(grad_att)`:
 * the Byzantine vector of the "empire" attack with factor = scale (attacks/identical.py:63-86,
 * 129-134) comes for free with the honest-stack statistics the study block needs anyway
 * (attack.py:847).
 * attack_kind selects what scaled_out holds:
 *   BM_ATTACK_EMPIRE  avg + scale * (-avg)                         attacks/identical.py:129-134
 *   BM_ATTACK_LITTLE  avg + scale * sqrt(var_unbiased over rows)   attacks/identical.py:136-141
 *                     (pass a negative scale for the reference's `negative:True`) */
enum bm_attack_kind { BM_ATTACK_EMPIRE = 0, BM_ATTACK_LITTLE = 1,
                      /* OR-ed in: scaled_out = scale * direction only, without the average (what the factor
                       * search of attacks/identical.py:67-77 keeps as `grad_att`)                             */
                      BM_ATTACK_DIRECTION = 16 };
int bm_stack_stats(const float* const* rows, int k, int64_t d, float* avg_out,
                   float* scaled_out, float scale, int attack_kind, double* out3, void* ws,
                   void* stream);

/* The dot products of the study block (attack.py:851-868) in one pass:
 *   out[a*nc+b]   = <core[a], core[b]>   for the nc (<= 4) "core" vectors (symmetric, the
 *                   diagonal holds the squared norms), then
 *   out[nc*nc+e]  = <core[0], extra[e]>  for ne (<= 32) more vectors (the past sampled
 *                   averages of the curvature term, attack.py:863-865).  All fp64. */
int bm_multi_dot(const float* const* core, int nc, const float* const* extra, int ne,
                 int64_t d, double* out, void* ws, void* stream);

/* The study block of a step (attack.py:830,848-868) in ONE pass over the d-sized vectors:
 *   - statistics of the attack stack = f_real copies of byz (tools.compute_avg_dev_max, attack.py:848): the
 *     sequential mean a and the deviations are rebuilt per element from byz with the reference's operations;
 *     a is written to attack_avg_out only if that is non-NULL;
 *   - |defense|^2 and max|defense| (attack.py:851-852);
 *   - the Gram matrix of core = (sampled avg, honest avg, defense, attack avg) behind the six cosines
 *     (attack.py:854-859), <sampled avg, past_newest> (attack.py:861-862) and <sampled avg, curv>, curv being
 *     C = sum_i mu^i past_i: the curvature term mu * sum_i mu^i <s, past_i> of attack.py:863-866 as ONE dot;
 *   - |params - origin|^2 (attack.py:830) when both are non-NULL;
 *   - the update of C for the next step, in place, AFTER its dot product:
 *       curv_mode 0  no curvature term kept (curv, past_* ignored)
 *                 1  first step: C <- sampled avg (no dots with the past)
 *                 2  C <- sampled avg + mu * C
 *                 3  C <- sampled avg + mu * (C + oldest_weight * past_oldest), oldest_weight = -(mu^(P-1)):
 *                    the entry that leaves a full ring of P past averages is taken out first.
 * out (DEVICE, BM_STUDY_SLOTS doubles):
 *   [4a+b] <core_a, core_b> (row/column 3 zero when f_real = 0)   [16] <s, past_newest>   [17] <s, C before the update>
 *   [18] sum avg_a^2   [19] sum_i |a_i - avg_a|^2   [20] max|avg_a|   [21] max|defense|   [22] |params - origin|^2
 * ws: bm_workspace_bytes(BM_WS_STUDY).  f_real = 0: no attack (byz ignored). */
#define BM_STUDY_SLOTS 32
int bm_study_stats(const float* sampled_avg, const float* honest_avg, const float* defense, const float* byz,
                   int f_real, float* attack_avg_out, const float* past_newest, float* curv,
                   const float* past_oldest, int curv_mode, float mu, float oldest_weight, const float* params,
                   const float* origin, int64_t d, double* out, void* ws, void* stream);
/* bm_study_stats that also carries the momentum of the update (attack.py:836-838, `--momentum-at update`, the
 * reference's default placement): update_momentum <- fma(one_minus_damp, defense, momentum_mu * update_momentum), in
 * place, element by element with the bits of bm_multi_fma3(M, M, defense, mu, 1 - damp) — inside the pass that reads
 * the defense vector anyway (2 row units more instead of a 3-unit pass and a launch of its own).  update_momentum
 * NULL: exactly bm_study_stats.  The statistics are those of `defense`, not of the updated momentum. */
int bm_study_stats_update(const float* sampled_avg, const float* honest_avg, const float* defense, const float* byz,
                          int f_real, float* attack_avg_out, const float* past_newest, float* curv,
                          const float* past_oldest, int curv_mode, float mu, float oldest_weight, const float* params,
                          const float* origin, float* update_momentum, float momentum_mu, float one_minus_damp,
                          int64_t d, double* out, void* ws, void* stream);

/* sq_out[i] = |rows[i]|^2 (DEVICE, k doubles), every row read once: the `gradient.norm().item()` of
 * aggregators/cge.py:28-38 and of the clipping at attack.py:776-779,791-794 for all gradients in one call, without a
 * host round trip per gradient.  ws: bm_workspace_bytes(BM_WS_DOT). */
int bm_row_sqnorms(const float* const* rows, int k, int64_t d, double* sq_out, void* ws, void* stream);

/* order_out = stable argsort (ties to the lower index, NaN last) of n fp64 keys that live on
 * the device: the `d.sort(key=...)` of aggregators/aksel.py:48 without a host round trip. */
int bm_stable_argsort(const double* keys, int n, int32_t* order_out, void* stream);

/* The reference's `anticge` attack (attacks/anticge.py:49-78) on the device, for 1 <= f_decl <= h (the reference indexes
 * normed[h - f_decl]).  These three entry points joined ABI 23: additions only, no signature changed.
 *   With maxpos = h - f_decl and g_(0), g_(1), ... the honest rows by increasing norm (a non-finite norm counts as +inf,
 *   ties go to the lower index: anticge.py:44-47 and Python's stable sort):
 *     S   = ((g_(0) + g_(0)) + g_(1)) + ... + g_(maxpos-1)      sequential fp32, the smallest row twice: anticge.py:70-72
 *           (`attack = g_(0).clone()`, then one add_ per selected row, g_(0) first; maxpos = 0 leaves the clone alone)
 *     byz = S * (float)(-nextafter(|g_(maxpos)|, 0) / |S|)      when |S| > 0, else S as it is: anticge.py:68,74-76
 * bm_anticge_sum: row_sq (DEVICE, h doubles) holds the squared norms where bm_row_sqnorms left them — the GLOBAL ones
 *   under sharding, after the caller's all-reduce.  One workgroup ranks the rows; order_out (DEVICE, BM_MAX_ROWS int32,
 *   may be NULL) receives the ranking (the h rows, then zeros) and scal_out[1] the squared norm of g_(maxpos) (+inf when
 *   it is not finite).  One pass over the selected rows then writes S to sum_out (DEVICE, d floats, never an input) and
 *   scal_out[0] = sum_j S_j^2 over the d coordinates given: this shard's part.  fp64 partial sums in a fixed order, no
 *   float atomics, no synchronisation.  scal_out: DEVICE, 2 doubles.  ws: bm_anticge_workspace_bytes(d).
 *   d == 0 is legal (an empty shard: scal_out[0] = 0).
 * bm_anticge_scale: vec *= the multiplier above, in place, formed on the device from scal = { |S|^2, |g_(maxpos)|^2 }
 *   (DEVICE; under sharding after the caller's all-reduce of scal[0]) with the reference's arithmetic: both norms
 *   rounded to fp32 as `.norm().item()` returns them, nextafter and the quotient in double, ONE rounding to fp32
 *   (`mul_` with a Python scalar).  A |S|^2 that is zero or NaN leaves vec untouched. */
int64_t bm_anticge_workspace_bytes(int64_t d);
int bm_anticge_sum(const float* const* rows, int h, int64_t d, int f_decl, const double* row_sq, float* sum_out,
                   int32_t* order_out, double* scal_out, void* ws, void* stream);
int bm_anticge_scale(float* vec, int64_t d, const double* scal, void* stream);

/* The Byzantine vector of the reference's `nan` (attacks/nan.py:36-40), `bulyan` (attacks/identical.py:114-127 with
 * :82-84) and `empire-strict` (attacks/empire.py:61-62) attacks from the honest average, in ONE streaming pass.  This
 * entry point joined ABI 23: an addition, no signature changed.
 *   out[i] = NaN (bits 0x7FC00000) | avg[i] + factor*(i == target) | avg[i] + factor | avg[i]*factor
 * every coordinate computed as written (avg + factor*dir with dir in {0, 1}, never a copy of avg: a -0.0 comes out as
 * the reference's), in fp32.  The `bulyan` attack at a fixed factor: BM_AV_SHIFT_ONE / _ALL with its factor (negated
 * by the caller for negative:True); `empire-strict`: BM_AV_SCALE with factor = -epsilon.
 * factor_dev != NULL: the factor is read from DEVICE memory (a double, rounded to fp32 as bm_multi_fma3_bdev rounds
 *   it) and `factor` is ignored.
 * direction_out != NULL (SHIFT kinds only): the same launch also stores the 0/1 direction vector (d floats).
 * target (BM_AV_SHIFT_ONE; any value of [-1, d) with the other kinds): a coordinate of THIS buffer in [0, d), or -1 =
 *   not in this buffer (under sharding: a rank that does not hold the targeted coordinate).
 * avg may be NULL for BM_AV_NAN only.  out must not overlap avg or direction_out.  d == 0 launches nothing.  No
 * workspace, no atomics, no synchronisation. */
enum bm_attack_vector_kind { BM_AV_NAN = 0, BM_AV_SHIFT_ONE = 1, BM_AV_SHIFT_ALL = 2, BM_AV_SCALE = 3 };
int bm_attack_vector(int kind, const float* avg, int64_t d, int64_t target, float factor, const double* factor_dev,
                     float* out, float* direction_out, void* stream);

/* y[i] = a*y[i] + b*x[i] for k vectors at once: worker momentum
 * `gmtm.mul_(mu).add_(grad, alpha=1-damp)` at attack.py:800-804. */
int bm_multi_axpby(float* const* y, const float* const* x, int k, int64_t d,
                   float a, float b, void* stream);

/* First pass of a simulation step in ONE kernel (attack.py:791-804,846-847 + attacks/identical.py:63-86):
 *   s_i      = clip_factors[i] * sampled[i]                       (clip_factors NULL: s_i = sampled[i])
 *   buffers[i] <- mu * buffers[i] + one_minus_damp * s_i, i < h   worker momentum, in place; these ARE
 *                                                                  the honest gradients the rule sees
 *   sampled_avg, honest_avg = sequential means of the ks sampled rows s_i / the h updated buffers
 *   byz_out  = honest_avg + scale * (-honest_avg)                 BM_ATTACK_EMPIRE
 *            = honest_avg + scale * sqrt(unbiased column variance) BM_ATTACK_LITTLE
 *   out6     = { sum avg_s^2, sum_i ||s_i-avg_s||^2, max|avg_s|,  sum avg_h^2, sum_i ||b_i-avg_h||^2, max|avg_h| }
 * i.e. tools.compute_avg_dev_max of both stacks (tools/pytorch.py:97-125) without re-reading them.
 * ks >= h; any of sampled_avg / honest_avg / byz_out may be NULL.  ws: bm_workspace_bytes(BM_WS_STEP). */
int bm_momentum_stats(const float* const* sampled, int ks, float* const* buffers, int h, int64_t d,
                      float mu, float one_minus_damp, const float* clip_factors, float* sampled_avg,
                      float* honest_avg, float* byz_out, float scale, int attack_kind, double* out6,
                      void* ws, void* stream);

/* The same first pass followed by a coordinate-wise rule over the h updated buffers and n_byz copies of byz_out, i.e.
 * defense_out = GAR(honests + [byz] * n_byz, f = rule_f) of attack.py:821 for rule_op = BM_OP_MEDIAN / TRMEAN / PHOCAS /
 * MEAMED (aggregators/median.py:39, trmean.py:33,81-109), with the results of bm_momentum_stats + bm_colwise (same
 * bits).  For the four rules over ks = h = 20 buffers and 5 Byzantine copies (the reference's n = 25, f = 5), or 14
 * buffers and 11 copies (its n = 25, f = 11), on 16-byte aligned rows, the rule runs INSIDE the first pass, on the
 * values it already holds in registers: the rule's own pass over the n rows disappears (26 of the 97 row passes of such a step).  Any other
 * shape runs the two kernels one after the other.  byz_out and defense_out must be non-NULL, attack_kind without
 * BM_ATTACK_DIRECTION. */
int bm_momentum_stats_colwise(const float* const* sampled, int ks, float* const* buffers, int h, int64_t d,
                              float mu, float one_minus_damp, const float* clip_factors, float* sampled_avg,
                              float* honest_avg, float* byz_out, float scale, int attack_kind, int rule_op,
                              int rule_f, int n_byz, float* defense_out, double* out6, void* ws, void* stream);

/* The same first pass together with the squared distances of the n = h + n_byz rows (the h updated buffers and n_byz
 * copies of byz_out) that Krum / Bulyan / Brute rank next (attack.py:821 with a distance-based rule and worker momentum):
 * sq_nxn as bm_pairwise_sqdist_shard(rows, n, d, d_total, ...) would give it.  For ks = h = 20 with 1..6 Byzantine
 * copies (or 14 with 11) and gradients long enough for the burst form, the centred rows are contracted on the matrix cores INSIDE the first
 * pass, from the registers that hold them: the distance pass never re-reads the n rows (25 of the 115 row passes of
 * such a step).  The distances then differ from the stand-alone pass by its rounding (another centre, another
 * order: both within 1e-5 of fp64); everything else has the bits of bm_momentum_stats.  Any other shape runs the two
 * passes one after the other.  ws: bm_workspace_bytes(BM_WS_STEP); ws_pair: bm_workspace_bytes(BM_WS_PAIRWISE, n, d).
 * attack_kind without BM_ATTACK_DIRECTION. */
int bm_momentum_stats_sqdist(const float* const* sampled, int ks, float* const* buffers, int h, int64_t d,
                             int64_t d_total, float mu, float one_minus_damp, const float* clip_factors,
                             float* sampled_avg, float* honest_avg, float* byz_out, float scale, int attack_kind,
                             int n_byz, double* sq_nxn, double* out6, void* ws, void* ws_pair, void* stream);

/* The same two fusions when there are no momentum buffers: the honest rows are the k sampled rows themselves, as with
 * `--momentum-at update` (the reference's default placement, attack.py:809-810,837-839).  bm_stack_stats (average,
 * Byzantine vector, statistics; tools/pytorch.py:97-125, attacks/identical.py:63-86) together with
 *   bm_stack_stats_colwise: defense_out = rule(rows + [byz] * n_byz, f = rule_f), the rule of bm_colwise;
 *   bm_stack_stats_sqdist : sq_nxn = the squared distances of rows + [byz] * n_byz (n = k + n_byz).
 * For 16-byte aligned rows and d a multiple of 4 it is ONE pass over the k rows — bm_stack_stats_colwise at k = 20 with
 * 5 Byzantine copies or 14 with 11 (the shapes of bm_momentum_stats_colwise), bm_stack_stats_sqdist at k = 20 with
 * 1..6 copies or 14 with 11 and gradients long enough for the burst form; otherwise the stand-alone kernels run one
 * after the other.  out6[0..2] = out6[3..5] = { sum avg^2, sum_i |row_i - avg|^2, max|avg| }. */
int bm_stack_stats_colwise(const float* const* rows, int k, int64_t d, float* avg_out, float* byz_out, float scale,
                           int attack_kind, int rule_op, int rule_f, int n_byz, float* defense_out, double* out6,
                           void* ws, void* stream);
int bm_stack_stats_sqdist(const float* const* rows, int k, int64_t d, int64_t d_total, float* avg_out, float* byz_out,
                          float scale, int attack_kind, int n_byz, double* sq_nxn, double* out6, void* ws,
                          void* ws_pair, void* stream);

/* out[i] = b * q[i] + a * (p_scale[i] * p[i]) for k vectors (p_scale: DEVICE array of k floats or NULL;
 * entries of q may be one shared vector; out[i] may alias p[i]).  Every momentum placement of the loop:
 * worker (attack.py:800-804), server (:805-808), update (:838-839), Nesterov look-ahead (:762,767). */
int bm_multi_fma3(float* const* out, const float* const* p, const float* const* q, int k, int64_t d,
                  float a, float b, const float* p_scale, void* stream);
/* The same with b read from DEVICE memory (one double, rounded to fp32 like the host's conversion of the same number):
 * the Byzantine vector avg + factor * att (identical.py:82-84) from the factor bm_attack_line_search_device left on
 * the device, without a host round trip. */
int bm_multi_fma3_bdev(float* const* out, const float* const* p, const float* const* q, int k, int64_t d,
                       float a, const double* b_dev, const float* p_scale, void* stream);

/* Gradient clipping (attack.py:776-779,791-794) without a host round trip:
 * bm_clip_factors: factors[i] = clip/sqrt(row_sq[i]) if sqrt(row_sq[i]) > clip else 1 (device arrays);
 * bm_multi_scale : y[i] *= factors[i] in place; rows whose factor is 1 are not touched. */
int bm_clip_factors(const double* row_sq, int k, float clip, float* factors_out, void* stream);
int bm_multi_scale(float* const* y, int k, int64_t d, const float* factors, void* stream);

/* Brute subset search on the host (aggregators/brute.py:47-68): over all
 * C(n, n-f) subsets in lexicographic order, first subset of smallest diameter;
 * subsets touching a non-finite distance are skipped.  dist_nxn holds sqrt'ed
 * distances (host memory; entries [x*n + y] with x < y are read).  Writes n-f
 * ascending indices; returns 0, or BM_EINVAL if no finite subset exists.
 * The subsets are not enumerated (bisection over the distances, a search tree of
 * depth <= f per probe): n = 51, f = 12 — 1.6e11 subsets — takes 0.1 ms. */
int bm_brute_select(const double* dist_nxn, int n, int f, int32_t* sel_out);
/* The subset search of bm_brute_select ON THE DEVICE (one workgroup of 16 waves that probe 16 thresholds / 16 rows at
 * a time, csrc/brute.hip), from the SQUARED distances where bm_pairwise_sqdist left them: no copy out, no host search,
 * no copy in — distances -> search -> bm_selected_mean are three launches on one stream, and a HIP graph can record
 * them.  sel_out (DEVICE, BM_MAX_ROWS int32): the n-f rows ascending, then zeros — the index table bm_selected_mean
 * reads.  status (DEVICE, one int32): 0; -1 when every subset touches a non-finite distance (brute.py:56-57,68: the
 * reference then fails its assertion) — sel_out then holds n-f copies of the first row all of whose distances are
 * non-finite, so that the average that follows is non-finite where that row is; -2 when the search gave up on its
 * budget of 2^18 search-tree nodes per wave (the tree is exponential in f in the worst case; a crafted matrix must
 * not hold the stream for seconds) — sel_out then holds n-f times the index -1, which bm_selected_mean answers with
 * NaN in EVERY coordinate (never the average of some rows); bm_brute_select on the host has no such limit and is what
 * the Python host falls back to.
 * Same selections as bm_brute_select (tests/test_gpu_parity_r4.py). */
int bm_brute_select_device(const double* sq_nxn, int n, int f, int32_t* sel_out, int32_t* status, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dim-sharded aggregation: one process per GPU, every rank holds all n rows
 * restricted to its d_local coordinates.  The reference has no counterpart (its aggregation is
 * single-device, attack.py:811-825); these are the entry points a multi-GPU binding would use.
 * RCCL is bound lazily with dlopen (no link-time dependency).  A NULL comm means "one rank".
 */
typedef struct bm_comm bm_comm;

int bm_comm_available(void);                  /* 1 if RCCL could be bound in this process        */
int bm_comm_unique_id(void* id128);           /* rank 0: 128 bytes to hand to every other rank   */
int bm_comm_init(bm_comm** out, int nranks, int rank, const void* id128);  /* collective         */
int bm_comm_destroy(bm_comm* comm);
int bm_comm_size(const bm_comm* comm);

/* In-place sum over the ranks of `count` doubles on the caller's stream (the n x n squared-distance
 * partials, the packed step statistics); no-op for one rank. */
int bm_allreduce_sum_f64(bm_comm* comm, double* buf, int64_t count, void* stream);
/* all[r*count .. (r+1)*count) = rank r's `mine`: the full output vector from the per-rank slices. */
int bm_allgather_f32(bm_comm* comm, const float* mine, float* all, int64_t count_per_rank, void* stream);

/* Multi-Krum / Bulyan of the local slice in ONE call: partial squared distances -> all-reduce ->
 * score + stable rank (identical on every rank) -> selected mean / Bulyan pass 2 of the slice
 * (aggregators/krum.py:31-80, bulyan.py:31-84).  order_out (DEVICE, BM_MAX_ROWS int32, may be NULL)
 * receives the ranking.  ws: bm_sharded_workspace_bytes(n, d_local).  d_total >= d_local is the length of the
 * WHOLE vectors (all shards): the plan of the distance pass follows it, and every rank must state the same number
 * (a short or empty trailing shard then plans exactly like its peers, whatever the world size). */
int64_t bm_sharded_workspace_bytes(int n, int64_t d_local);
int bm_sharded_krum(bm_comm* comm, const float* const* rows, int n, int64_t d_local, int64_t d_total, int f, int m,
                    float* out_local, int32_t* order_out, void* ws, void* stream);
int bm_sharded_bulyan(bm_comm* comm, const float* const* rows, int n, int64_t d_local, int64_t d_total, int f, int m,
                      float* out_local, int32_t* order_out, void* ws, void* stream);

/* The tail of bm_sharded_krum / bm_sharded_bulyan (all-reduce -> rank -> selected mean / pass 2) when the squared
 * distances of the local shard are already in the workspace: bm_momentum_stats_sqdist wrote them to
 * bm_sharded_sq_slot(ws), using bm_sharded_pair_workspace(ws) as its ws_pair.  rule: BM_RULE_KRUM or BM_RULE_BULYAN. */
double* bm_sharded_sq_slot(void* ws);
void* bm_sharded_pair_workspace(void* ws);
/* Where bm_sharded_krum / bm_sharded_bulyan / bm_sharded_rule_from_sq leave their ranking (DEVICE, BM_MAX_ROWS int32,
 * inside ws): valid on the call's stream until the next of these calls with the same ws.  (Added within ABI 23.) */
int32_t* bm_sharded_order_slot(void* ws);
int bm_sharded_rule_from_sq(bm_comm* comm, int rule, const float* const* rows, int n, int64_t d_local, int f, int m,
                            float* out_local, int32_t* order_out, void* ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * One simulation step with worker-side momentum (attack.py:786-868) as ONE call on the caller's stream:
 * [clipping factors] -> bm_momentum_stats -> rule over buffers + [byz] * f_real -> bm_study_stats (attack /
 * defense statistics, study dots, l2 from the origin, curvature combination: one pass) -> one packed exchange.
 * attack_avg_out may be NULL (the attack average is only needed as a vector by callers that want it).
 * comm NULL = one rank; otherwise every collective of the dim-sharded step (row norms when clipping, the
 * n x n squared distances, the packed statistics) goes through it.  d = coordinates of this rank.
 *
 * stats_out (DEVICE, bm_step_stats_count() doubles, identical on every rank):
 *   [0] sum avg_s^2  [1] sum_i |s_i-avg_s|^2  [2] sum avg_h^2  [3] sum_i |b_i-avg_h|^2  [4] |defense|^2
 *   [5] sum avg_a^2  [6] sum_i |a_i-avg_a|^2  [7] |params-origin|^2
 *   [8 + 4a + b] <core_a, core_b>, core = (sampled avg, honest avg, defense, attack avg)
 *   [24] <sampled avg, past_newest>  [25] <sampled avg, curv>   [26..29] max|avg_s|, max|avg_h|, max|defense|, max|avg_a|
 *   [30] BM_RULE_KRUM: how many of the m rows the rule averaged are Byzantine copies (index >= n - f_real), an integer
 *        (bm_accept_count on the rule's ranking; the "Attack acceptation ratio" of attack.py:822 is this over m);
 *        0 for every other rule.  Every rank holds the same ranking: the slot is reduced as a maximum, not summed.
 * curv (in/out, may be NULL when nb_past = 0): C = sum_i mu^i past_i, updated for the NEXT step
 * (C <- s when past_count = 0, else C <- mu * (C + oldest_weight * past_oldest) ... see step.py);
 * past_oldest non-NULL only when the caller's ring of nb_past vectors is full (its last entry).
 */
enum bm_step_rule { BM_RULE_KRUM = 0, BM_RULE_BULYAN = 1, BM_RULE_MEDIAN = 2, BM_RULE_TRMEAN = 3,
                    BM_RULE_PHOCAS = 4, BM_RULE_MEAMED = 5,
                    BM_RULE_BRUTE = 6, BM_RULE_AVERAGE = 7 /* bm_attack_* only, not bm_step_worker */ };
typedef struct bm_step_params {
  int32_t n, f_decl, f_real;  /* workers, declared and real Byzantine ones; honest = n - f_real      */
  int32_t ks;                 /* sampled gradients (>= honest)                                        */
  int32_t rule;               /* bm_step_rule                                                          */
  int32_t m;                  /* Multi-Krum / Bulyan m, 0 = n - f_decl - 2                             */
  int32_t attack_kind;        /* bm_attack_kind                                                        */
  int32_t nb_past;            /* length P of the caller's ring of past sampled averages, 0 = none      */
  int32_t past_count;         /* entries in the ring before this step                                  */
  float attack_scale;         /* factor of the attack                                                  */
  float mu, one_minus_damp;   /* momentum, 1 - dampening                                               */
  float clip;                 /* gradient clipping threshold, <= 0 = off                               */
  float oldest_weight;        /* -(mu^(P-1)): weight that takes the leaving entry out of C              */
} bm_step_params;
int bm_step_stats_count(void);
int64_t bm_step_workspace_bytes(int n, int64_t d_local);
int bm_step_worker(bm_comm* comm, const bm_step_params* p, const float* const* sampled, float* const* buffers,
                   int64_t d, int64_t d_total /* >= d: all shards, as bm_sharded_krum */, float* defense_out,
                   float* sampled_avg_out, float* honest_avg_out, float* byz_out,
                   float* attack_avg_out, const float* past_newest, float* curv, const float* past_oldest,
                   const float* params, const float* origin, double* stats_out, void* ws, void* stream);

/* The numerator of the "Attack acceptation ratio" (attack.py:571,822; krum.py:144-150, brute.py:132-140,
 * aksel.py:97-105, cge.py:88-96) from the selection a rule left in device memory.  With gradients = honests + [byz] *
 * f_real a selected row is an attack exactly when its index is >= h = n - f_real.
 * order (DEVICE, at least `count` int32): row indices — a ranking of bm_krum_rank / bm_stable_argsort, or the subset of
 * bm_brute_select_device.  out (DEVICE, 1 double): the number of entries >= h among the first `count`, an integer
 * (count == 0 writes 0).  One wavefront on the caller's stream, no synchronisation; the caller divides by its
 * denominator on the host, the reference's own `int / int`.  0 <= count <= BM_MAX_ROWS, h >= 0.
 * (Added within ABI 23: a host recognises the leg by the presence of the symbol.) */
int bm_accept_count(const int32_t* order, int count, int h, double* out, void* stream);

/* ONE candidate of the attacks' factor search against the trimmed mean, phocas or meamed, evaluate only
 * (attacks/identical.py:73-76 with aggregators/trmean.py:69-109 as the defense):
 *     out[0] = sum_j ( RULE(honests + [avg + t * dir] * copies)_j - avg_j )^2        (DEVICE, one double)
 * The candidate vector is never written (it is fma(t, dir, avg) in registers, the bits bm_multi_fma3 would store),
 * nor the rule's output: h + 2 rows read, nothing written, against h + 5 read and 2 written by candidate vector +
 * bm_colwise + objective.  Instances exist for n = h + copies in {11, 25, 51} (bm_colwise_eval_supported);
 * ws: bm_colwise_eval_workspace_bytes().  d == 0 is legal (an empty shard: out[0] = 0). */
int bm_colwise_eval_supported(int op, int n);
int64_t bm_colwise_eval_workspace_bytes(void);
int bm_colwise_eval(int op, const float* const* honests, int h, int copies, int64_t d, int f, const float* avg,
                    const float* dir, float t, double* out, void* ws, void* stream);
/* (Also op = BM_OP_MEDIAN with h = 2, copies = 1: the middle of (candidate, honests[0], honests[1]) — the median's own
 * factor search, where the two rows are order statistics of the honest rows formed once per search.)
 * The same with t read from DEVICE memory (one double, rounded to fp32 like the host's conversion of the same number):
 * the factor bm_search_device_next left there. */
int bm_colwise_eval_tdev(int op, const float* const* honests, int h, int copies, int64_t d, int f, const float* avg,
                         const float* dir, const double* t_dev, double* out, void* ws, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The factor search of the "identical" attacks (attacks/identical.py:67-77, the reference's default
 * factor=-16) — HOST functions, no stream (but bm_attack_line_search_device).
 *
 * bm_search_*: the exploration of tools/misc.py:468-514 (best-effort arg-max over x >= 0 within a budget of
 * evaluations; reference defaults: start 0, delta 1, ratio 0.8) as a cursor the CALLER drives:
 *     bm_search_begin(&c, start, delta, ratio);
 *     repeat `evals` times: bm_search_propose(&c, &x); y = <evaluate at x>; bm_search_report(&c, y);
 *     answer: c.best_x
 * The evaluations are the caller's (a rule on the device, or bm_attack_objective on scalars); the library
 * never calls back.  bm_search is plain data owned by the caller.
 *
 * bm_attack_objective / bm_attack_line_search: for a rule whose output is the mean of a selected subset
 * (BM_RULE_KRUM with m, BM_RULE_BRUTE, BM_RULE_AVERAGE), the objective |GAR(honests + [avg + t*att]*k, f)
 * - avg|^2 of identical.py:72-76 evaluated from scalars only.  ext: HOST row-major (h+2) x (h+2) squared
 * distances (bm_pairwise_sqdist) among the h honest rows, their average and average + att.
 * sel_out (may be NULL): the rows the rule averages, indices >= h being Byzantine copies; count_out
 * their number.  bm_attack_line_search runs the whole search (negative: identical.py:70-71) and returns
 * the factor the attack then uses.  No d-sized vector is touched: 16 evaluations cost microseconds. */
typedef struct bm_search {
  double best_x, best_y;  /* incumbent: abscissa and value (valid once evaluations >= 1)           */
  double probe;           /* last abscissa proposed                                                 */
  double step, ratio;     /* current step; contraction factor, 0.5 < ratio < 1                      */
  int32_t phase;          /* 0 first evaluation, 1 growing, 2 shrinking                             */
  int32_t evaluations;    /* values reported so far                                                 */
  int32_t awaiting;       /* 1 between bm_search_propose and bm_search_report                       */
  int32_t reserved;
} bm_search;
int bm_search_begin(bm_search* c, double start, double delta, double ratio);
int bm_search_propose(bm_search* c, double* x_out);
int bm_search_report(bm_search* c, double y);
int bm_attack_objective(const double* ext, int h, int k, int f, int rule, int m, double t, double* y_out,
                        int32_t* sel_out, int32_t* count_out);
int bm_attack_line_search(const double* ext, int h, int k, int f, int rule, int m, int evals, int negative,
                          double* factor_out, double* trace_out);
/* bm_attack_line_search on the DEVICE, for BM_RULE_KRUM and BM_RULE_AVERAGE (BM_EINVAL for BM_RULE_BRUTE: its search
 * is the host form's): ext is the DEVICE matrix where bm_pairwise_sqdist left it, one workgroup evaluates the `evals`
 * candidates (csrc/search_device.hip) and writes out[0] = the factor, out[1 + 2e], out[2 + 2e] = abscissa and objective
 * of evaluation e (out: DEVICE, 1 + 2 * evals doubles).  Same candidates and the same bits as the host form; no copy,
 * no synchronisation — the factor is consumed where it is by bm_multi_fma3_bdev.  (MEASUREMENT ONLY: with
 * BM_SEARCH_TRACE=1 in the environment the kernel also writes 24 phase timestamps per evaluation behind the results and
 * `out` must hold 1 + 26 * evals doubles; scripts/search_kernel_probe.py.) */
int bm_attack_line_search_device(const double* ext, int h, int k, int f, int rule, int m, int evals, int negative,
                                 double* out, void* stream);
/* out[0] = |a - b|^2 (fp64, DEVICE): the objective `aggregated.sub_(grad_avg); aggregated.dot(aggregated)` of
 * identical.py:75-76 for a candidate whose rule was run on the vectors; one pass over the two vectors (the n x n
 * distance pass spends three launches on them).  ws: bm_colwise_eval_workspace_bytes().  Partial sums in a fixed order. */
int bm_sqdist2(const float* a, const float* b, int64_t d, double* out, void* ws, void* stream);
/* bm_attack_ranking on the DEVICE, the factor read from DEVICE memory (one double): order_out[0..63] (int32, DEVICE; the n
 * rows by rank, then zeros) for honests + [avg + t*att] * k, from the matrix where bm_pairwise_sqdist left it.  One
 * workgroup; no copy, no synchronisation.  k >= 1.  mode: BM_RANK_KRUM or BM_RANK_BULYAN (m as for bm_krum_rank). */
int bm_attack_ranking_device(const double* ext, int h, int k, int f, int mode, int m, const double* t_dev,
                             int32_t* order_out, void* stream);
/* out[0] = | pass2(honests + [avg + t * dir] * copies, order) - avg |^2 (fp64, DEVICE): bm_bulyan_pass2 on a stack whose
 * last `copies` rows are ONE candidate of the factor search (identical.py:67-77), evaluate only — the candidate is formed
 * in registers with the arithmetic of bm_multi_fma3, nothing is written.  `order` ranks the n = h + copies rows (indices
 * >= h name a copy), e.g. by bm_attack_ranking.  t from the host, or from DEVICE memory when t_dev != NULL (one double,
 * rounded to fp32).  Instances: (n, f) in {(11, 2), (25, 5), (51, 12)} with m = n - f - 2 (bm_bulyan_pass2_eval_supported),
 * d <= 2^29.  ws: bm_colwise_eval_workspace_bytes(). */
int bm_bulyan_pass2_eval_supported(int n, int f, int m);
int bm_bulyan_pass2_eval(const float* const* honests, int h, int copies, const int32_t* order, int f, int m, int64_t d,
                         const float* avg, const float* dir, float t, const double* t_dev, double* out, void* ws,
                         void* stream);
/* lo[j] = the value of rank il, hi[j] = the value of rank ih (0-based, ascending) among rows[0..h)[j]; a rank below 0 reads
 * -inf, a rank beyond h - 1 reads +inf; a NaN in the column makes both NaN.  One pass over the h rows (h <= 51:
 * bm_order_pair_supported).  With n = h + k, il = (n-1)/2 - k, ih = (n-1)/2 these are the lower medians (median.py:31-39)
 * of the rows with k copies of -inf, resp. +inf — the two vectors between which the median of `rows + [b] * k` moves
 * with b: the median's own factor search (identical.py:67-77) forms them once and evaluates every candidate as the
 * middle of three (bm_colwise_eval with BM_OP_MEDIAN).  Values of the rows, no arithmetic: the bits of the two median
 * calls it replaces. */
int bm_order_pair_supported(int h);
int bm_order_pair(const float* const* rows, int h, int64_t d, int il, int ih, float* lo, float* hi, void* stream);
/* The cursor of bm_search_* kept in DEVICE memory, for the searches whose candidates are evaluated by d-sized kernels
 * (median, trimmed mean, phocas, meamed, any rule): the host queues
 *     bm_search_device_next(state, NULL, negative, 0, start, delta, ratio, t, out)      first candidate
 *     repeat: <evaluation kernels that read t[0]: bm_multi_fma3_bdev, bm_colwise_eval_tdev, the rule, and leave the
 *              objective y[0] on the device>;  bm_search_device_next(state, y, negative, 0, ..., t, out)
 *     bm_search_device_next(state, y_last, negative, 1, ..., NULL, out)                  the factor
 * without waiting for any of them: `state` DEVICE memory of sizeof(bm_search), t DEVICE double (the candidate's signed
 * factor, identical.py:70-71), out DEVICE 1 + 2 * evals doubles laid out like bm_attack_line_search_device's.  Same
 * candidates as the host cursor (one definition, csrc/search_core.h).  start / delta / ratio are read on the first call. */
int bm_search_device_next(void* state, const double* y, int negative, int last, double start, double delta, double ratio,
                          double* t_out, double* out, void* stream);
/* The ranking bm_krum_rank(mode, m) would give for honests + [avg + t*att] * k, from the same scalars (order_out: n
 * int32, indices >= h being Byzantine copies): for the rules whose output needs the vectors but whose ranking does not
 * — Bulyan (aggregators/bulyan.py:48-62 rank, :64-84 second pass): a candidate of the factor search then costs
 * bm_bulyan_pass2 with this ranking instead of a distance pass over the n rows as well.  m <= 0: n - f - 2. */
int bm_attack_ranking(const double* ext, int h, int k, int f, int mode, int m, double t, int32_t* order_out);

/* ---------------------------------------------------------------------------------------------
 * The geometric median (RFA, smoothed Weiszfeld) and centered clipping from ONE distance pass.  These three entry
 * points joined ABI 23: additions only, no signature changed.  Neither rule exists in the reference.
 *
 * Every iterate of both rules is an affine combination v = sum_j c_j p_j (sum c = 1) of the points p_0 .. p_{N-1}: the
 * n rows and, when has_start != 0, a start vector as point n (N = n + has_start <= BM_MAX_ROWS).  With D the N x N
 * squared distances of the points (bm_pairwise_sqdist over rows + [start]),
 *     |p_i - v|^2 = t_i - q / 2,   t_i = sum_j c_j D_ij,   q = sum_i c_i t_i,
 * so the whole iteration runs on the N weights (csrc/center_core.h, one definition for host and device) and the rule
 * costs one distance pass plus one bm_weighted_sum whatever the number of iterations.
 *   usable    point i is unusable when D_ij is non-finite for at least one and at least half of the other points
 *             (cnt >= 1 and 2 cnt >= N - 1): it never gets weight.  No usable ROW: every weight is NaN.  U = the
 *             number of usable rows.
 *   start     c = 1 on the start vector when it is given and usable, else 1 / U on every usable row.
 *   distance  r_i = sqrt(max(0, t_i - q / 2)); terms with c_j == 0 are skipped; a non-finite r_i^2 counts as +inf
 *             (aggregators/krum.py:46-47).
 *   BM_CENTER_GEOMED (param = nu > 0): w_i = 1 / max(nu, r_i) over the usable rows, c <- w / sum w (the start gets 0).
 *   BM_CENTER_CCLIP  (param = tau > 0): s_i = 1 if r_i <= tau else tau / r_i over the usable rows, S = sum s_i,
 *             c <- c * (1 - S / U), then c_i += s_i / U on the rows: v <- v + (1/U) sum_i (x_i - v) min(1, tau / |x_i - v|).
 *   stop      after `iters` iterations (1 .. 64), or earlier once sqrt(move^2) <= tol, move^2 = max(0, -1/2 sum_jk e_j e_k
 *             D_jk) being the squared length of the step (e = the change of c); tol = 0 never stops early.
 * weights_out: BM_MAX_ROWS doubles, the N weights, then zeros.  info_out: 3 doubles = { iterations run, move^2 of the
 * last one, U }.
 * bm_center_weights: HOST function on a HOST matrix, no stream.  bm_center_weights_device: the same on the DEVICE matrix
 * where bm_pairwise_sqdist left it, one workgroup, no copy, no synchronisation; the same bits as the host form.  Both
 * return BM_EINVAL for a bad n, has_start, mode, param, iters or tol before any HIP call. */
enum bm_center_mode { BM_CENTER_GEOMED = 0, BM_CENTER_CCLIP = 1 };
int bm_center_weights(const double* sq_host, int n, int has_start, int mode, double param, int iters, double tol,
                      double* weights_out, double* info_out);
int bm_center_weights_device(const double* sq_dev, int n, int has_start, int mode, double param, int iters, double tol,
                             double* weights_out_dev, double* info_out_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The spectral filtering rules CAF (covariance-bound agnostic filter: Allouah, Guerraoui, Gupta, Rizk, Stephan, NeurIPS
 * 2023) and DnC (Shejwalkar & Houmansadr, NDSS 2021, without its coordinate sub-sampling and repeated draws) from ONE
 * distance pass.  These two entry points joined ABI 23: additions only, no signature changed.  Not in the reference.
 *
 * With weights c >= 0 on the rows x_i (C = sum c), mu = sum c_i x_i / C, y_i = x_i - mu and D the n x n squared distances
 * (bm_pairwise_sqdist), r_i = sum_k c_k D_ik / C and s = sum_i c_i r_i / C give
 *     <y_i, y_j> = K_ij = -1/2 (D_ij - r_i - r_j + s),   |y_i|^2 = r_i - s / 2,
 * so the top eigen-direction of the weighted covariance, every projection on it and every reweighting are computed on
 * scalars (csrc/spectral_core.h, one definition for host and device), and the rule costs one distance pass plus one
 * bm_weighted_sum whatever the number of rounds or power steps.
 *   usable      the predicate of bm_center_weights; unusable rows have weight 0 throughout; U = the usable rows; U = 0:
 *               every weight is NaN.
 *   evaluation  E(c), c = 0 on the rows without weight, which take no part: start v = y_j, j = argmax c_i |y_i|^2 (ties
 *               to the lowest index; a maximum that is not > 0: DEGENERATE); power_iters times w = (1/C) sum c_i <y_i, v>
 *               y_i, v <- w / |w| (a w of no length stops the steps); g_i = <y_i, v / |v|>, tau_i = g_i^2,
 *               lambda = (1/C) sum c_i g_i^2.  power_iters (1 .. 256) is a fixed count: no convergence test.
 *   BM_SPECTRAL_CAF (count = f, 0 <= 2 f < n): c = 1 on the usable rows, best = c / U, best lambda = +inf; while
 *               sum c > n - 2 f, at most n rounds: E(c), stop if degenerate; lambda < best lambda (strictly): best = c / C;
 *               tau_max = max tau over the rows of weight, stop unless > 0; c_i <- c_i (1 - tau_i / tau_max) — the row of
 *               largest tau gets exactly 0.  The weights are `best`.
 *   BM_SPECTRAL_DNC (count = k, 0 <= k < n): one E(c) on c = 1 over the usable rows (degenerate: every tau = 0); the
 *               k' = max(0, k - (n - U)) usable rows of largest tau are removed, the higher index first among equal tau;
 *               1 / (U - k') on every other usable row.
 * weights_out: BM_MAX_ROWS doubles, the n weights (sum 1), then zeros.  info_out: 4 doubles = { evaluations that were
 * not degenerate, the lambda of the weights kept (+inf: none), U, the 0-based round whose weights were kept (-1: none) }.
 * bm_spectral_weights: HOST function on a HOST matrix, no stream.  bm_spectral_weights_device: the same on the DEVICE
 * matrix where bm_pairwise_sqdist left it, one workgroup, no copy, no synchronisation; the same bits as the host form.
 * Both return BM_EINVAL for a null pointer or a bad n, mode, count or power_iters before any HIP call. */
enum bm_spectral_mode { BM_SPECTRAL_CAF = 0, BM_SPECTRAL_DNC = 1 };
int bm_spectral_weights(const double* sq_host, int n, int mode, int count, int power_iters, double* weights_out,
                        double* info_out);
int bm_spectral_weights_device(const double* sq_dev, int n, int mode, int count, int power_iters,
                               double* weights_out_dev, double* info_out_dev, void* stream);

/* out[j] = sum_i w_i rows[i][j] with w_i = (float)weights[i] (weights: DEVICE, n doubles, e.g. where
 * bm_center_weights_device left them): acc = 0, then acc = fmaf(w_i, rows[i][j], acc) over the ACTIVE rows in index order.
 * Rows that are the same pointer form one group: their fp64 weights are added in index order, rounded to fp32 once, and
 * the row is read once, at its first index.  A group whose fp32 weight is exactly 0 is not read (an excluded NaN row
 * cannot poison the sum).  A NaN weight makes out NaN everywhere.  One pass, no workspace, no synchronisation; d == 0
 * launches nothing. */
int bm_weighted_sum(const float* const* rows, int n, const double* weights_dev, int64_t d, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Nearest-neighbour mixing (Allouah, Farhadkhani, Guerraoui, Gupta, Pinot, Stephan, "Fixing by Mixing", AISTATS 2023):
 * every row is replaced by the average of its k = n - f nearest rows, itself included, and any rule runs on the mixed
 * rows.  These five entry points joined ABI 23: additions only, no signature changed.  Not in the reference.
 *
 * Neighbour masks, from the n x n fp64 squared distances D (bm_pairwise_sqdist), 1 <= n <= BM_MAX_ROWS, 0 <= f < n:
 * N_i holds row i itself, whatever D[i][i] is, and the k - 1 OTHER rows of smallest D[i][j]; ties go to the lower
 * index; NaN keys sort last, in index order among themselves (+inf before NaN).  masks[i] has bit j set iff j is in
 * N_i: one 64-bit word per row of the mixing matrix.  BM_MAX_ROWS masks are written, zeros beyond n.
 * bm_nnm_masks: HOST function on a HOST matrix, no stream.  bm_nnm_masks_device: the same on the DEVICE matrix, one
 * workgroup, no copy, no synchronisation; the same masks.  Both return BM_EINVAL for a bad n or f before any HIP call. */
int bm_nnm_masks(const double* sq_host, int n, int f, uint64_t* masks_host);
int bm_nnm_masks_device(const double* sq_dev, int n, int f, uint64_t* masks_dev, void* stream);

/* Mixing: n_out averages over subsets of the n rows, 1 <= n_out <= BM_MAX_ROWS (masks_dev: DEVICE, n_out words; the
 * masks above, or one mask per bucket: bucketing).  Per coordinate and output row r:
 *     acc = +0.0f;  for j = 0 .. n-1 ascending, bit j of masks[r] set:  acc = acc + rows[j] (fp32);
 *     out_rows[r] = acc / (float)popcount(masks[r])     one IEEE division
 * Bits at positions >= n are ignored; an empty mask gives NaN (0 / 0); a row outside the mask does not influence the
 * result even where it holds NaN or inf.  One streaming pass: every column is read once, 4 d (n + n_out) bytes.
 * rows may alias one another; every out_rows[r] must be disjoint from the other outputs and from every input, else
 * BM_EINVAL.  d == 0 launches nothing. */
int bm_mix_rows(const float* const* rows, int n, const uint64_t* masks_dev, int n_out, int64_t d, float* const* out_rows,
                void* stream);

/* out = rule(y_0 .. y_{n-1}), y_r the mixed rows of bm_mix_rows with n_out = n (masks_dev: at least n words), for op =
 * BM_OP_MEDIAN or BM_OP_TRMEAN (f: the trimmed mean's, n >= 2 f + 1), without writing a mixed row: 4 d (n + 1) bytes.
 * The same bits as bm_colwise on the rows bm_mix_rows writes.  Any other op, or n above bm_colwise_mixed_max_rows(),
 * returns BM_EINVAL: the caller then runs bm_mix_rows and bm_colwise. */
int bm_colwise_mixed(int op, const float* const* rows, int n, const uint64_t* masks_dev, int64_t d, int f, float* out,
                     void* stream);
int bm_colwise_mixed_max_rows(void);

/* The same with n_out < n mixed rows — bucketing in front of the coordinate-wise median / trimmed mean without the
 * bucket means.  out = rule(y_0 .. y_{n_out-1}), y_r the rows bm_mix_rows(rows, n, masks_dev, n_out) would write
 * (masks_dev: at least n_out words, general 64-bit masks: they may overlap, an empty one gives a NaN row), for op =
 * BM_OP_MEDIAN or BM_OP_TRMEAN (f: the trimmed mean's on the n_out rows, n_out >= 2 f + 1).  One pass, 4 d (n + 1) bytes
 * where the two kernels move 4 d (n + 2 n_out + 1).  The same bits as bm_colwise on the rows bm_mix_rows writes: the
 * sequential fp32 sum in ascending row order, one IEEE division by the popcount, a row outside a mask without influence
 * on y_r even where it holds NaN or inf.  Instances exist for n_out = ceil(n / 2) and ceil(n / 3), n = 2 .. an internal
 * limit per bucket size, decided by measurement: bm_colwise_bucketed_supported says 1 for those (op, n, n_out), 0
 * otherwise; an
 * unsupported shape returns BM_EINVAL and the caller runs bm_mix_rows and bm_colwise.  A null pointer, n_out outside
 * 1 .. n, a bad f or d < 0: BM_EINVAL before any HIP call.  d == 0 launches nothing.  Joined ABI 23 (additions only). */
int bm_colwise_bucketed_supported(int op, int n, int n_out);
int bm_colwise_bucketed(int op, const float* const* rows, int n, const uint64_t* masks_dev, int n_out, int64_t d, int f,
                        float* out, void* stream);

/* Bucket masks from a counter (bucketing: Karimireddy, He, Jaggi, ICLR 2022): a permutation of 0 .. n-1 that is a
 * function of (n, seed, counter) alone, cut into buckets of s.  All arithmetic is uint64 and wrapping:
 *     mix(x):  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31
 *     u_i    = mix(seed + 0x9E3779B97F4A7C15 * (64 * counter + i))                      i = 1 .. n-1
 *     perm   = (0 .. n-1);  for i = n-1 down to 1:  j = u_i mod (i + 1);  swap(perm[i], perm[j])
 *     bucket b = { perm[b s] .. perm[min(n, b s + s) - 1] },  b < ceil(n / s);  masks[b] has bit j set iff j is in bucket b
 * BM_MAX_ROWS words are written, zeros beyond ceil(n / s).  bm_bucket_masks: HOST function, host array, no stream.
 * bm_bucket_masks_device: one wavefront reads counter_dev[0] (DEVICE), writes the masks of that counter (DEVICE) and
 * stores counter + 1 back with an ordinary store, no atomic — the counter word belongs to one stream of launches — so a
 * recorded graph draws the next permutation at every replay with no host involvement, and every rank of a sharded run
 * draws the same one without a collective.  The same masks from both.  BM_EINVAL for a null pointer, n outside
 * 1 .. BM_MAX_ROWS or s outside 1 .. n, before any HIP call.  Joined ABI 23 (additions only). */
int bm_bucket_masks(int n, int s, uint64_t seed, uint64_t counter, uint64_t* masks_host);
int bm_bucket_masks_device(int n, int s, uint64_t seed, uint64_t* counter_dev, uint64_t* masks_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Distance-based rules on mixed rows WITHOUT the mixed rows.  These four entry points joined ABI 23: additions only.
 *
 * A mixed row is y_a = (1 / c_a) sum_{i in mask_a} x_i, c_a = popcount(mask_a).  With W_a = mask_a / c_a and
 * w = W_a - W_b, |y_a - y_b|^2 = -1/2 w' D w, D the squared distances of the ORIGINAL rows; and a weighted sum (or the
 * mean of a selection) of mixed rows is a weighted sum of the original rows.  So Krum / Multi-Krum, Brute, the
 * geometric median, centered clipping and the average on mixed rows cost the distance pass, kernels on at most
 * 64 x 64 scalars and one bm_weighted_sum: no n x d scratch, and one collective when the coordinates are sharded.
 *
 * bm_mixed_sqdist: sq = the n_in x n_in fp64 matrix as bm_pairwise_sqdist leaves it (possibly all-reduced); masks =
 * n_out words as bm_nnm_masks* write them, or one per bucket; out = n_out x n_out fp64, row-major.  The definition,
 * which fixes the bits (fp64, no contraction):
 *     D_ij (i != j) is read at (min(i, j), max(i, j)); the diagonal is never read and counts as +0; an entry of D
 *       outside every pair of masks is never read;
 *     Q_ib = sum over j in mask_b, j != i, ascending, of D_ij, from +0     (every i < n_in)
 *     P_ab = sum over i in mask_a, ascending, of Q_ib, from +0
 *     a != b, named so that mask_a < mask_b AS UNSIGNED 64-BIT WORDS:
 *       out_ab = P_ab / (c_a c_b) - (1/2) P_aa / c_a^2 - (1/2) P_bb / c_b^2, left to right, a value <= 0 -> +0;
 *       out_ba = out_ab: bitwise symmetric;  out_aa = +0.  (P_ab and P_ba are one sum in two orders and differ in
 *       their last bits: the order comes from the masks, not from the indices, so that an entry is a function of the
 *       two masks alone.  For masks in ascending word order this is "P_ab for a < b".)
 *     mask_a == mask_b: +0 by an explicit test (the pair reads no distance);
 *     an empty mask: NaN in its row and column, the diagonal entry included (bm_mix_rows writes a NaN row there);
 *     P_ab, P_aa or P_bb not finite (any distance read for the pair is not finite): NaN — never clamped to 0.
 * Rows with equal masks get bitwise-equal rows of out; aliased rows, whose rows of D are bitwise equal, keep their ties.
 * bm_mixed_sqdist: HOST function on HOST arrays, no stream.  bm_mixed_sqdist_device: the same on DEVICE arrays, one
 * workgroup, no copy, no synchronisation; the same bits.  Both return BM_EINVAL for a null pointer or n_in / n_out
 * outside 1 .. BM_MAX_ROWS before any HIP call.  A mask with a bit at or above n_in: BM_EINVAL from the host form;
 * the device form, which cannot read the masks before it returns, writes NaN to EVERY entry of out. */
int bm_mixed_sqdist(const double* sq_host, int n_in, const uint64_t* masks_host, int n_out, double* out_host);
int bm_mixed_sqdist_device(const double* sq_dev, int n_in, const uint64_t* masks_dev, int n_out, double* out_dev,
                           void* stream);

/* The weights of the ORIGINAL rows behind sum_r w_r y_r.  Exactly one of w_mixed and sel is non-null, else BM_EINVAL:
 *   w_mixed  fp64[n_out], e.g. what bm_center_weights* leaves;
 *   sel      int32[m], 1 <= m <= BM_MAX_ROWS: the first m entries of a ranking, or a Brute subset; w_r = the sum, one
 *            entry at a time in table order from +0, of 1 / m per entry equal to r (duplicates add up).  An entry
 *            outside 0 .. n_out-1 (-1 after a device Brute search that gave up) makes every w_out[j], j < n_in, NaN,
 *            as bm_selected_mean answers it.
 *   w_out[j] = sum over r ascending, w_r != 0 and bit j of mask_r set, of w_r / c_r   (fp64; a NaN w_r counts)
 * for j < n_in; w_out is fp64[BM_MAX_ROWS] with zeros beyond n_in: what bm_weighted_sum reads.  A mixed row with
 * w_r != 0 and an empty mask is a NaN row: every w_out[j], j < n_in, is NaN.  Same refusals, same treatment of mask
 * bits at or above n_in, and the same bits from the host and the device form as above. */
int bm_mix_weights(const uint64_t* masks_host, int n_in, int n_out, const double* w_mixed, const int32_t* sel, int m,
                   double* w_out_host);
int bm_mix_weights_device(const uint64_t* masks_dev, int n_in, int n_out, const double* w_mixed_dev, const int32_t* sel_dev,
                          int m, double* w_out_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The Min-Max and Min-Sum attacks (Shejwalkar, Houmansadr, "Manipulating the Byzantine", NDSS 2021), closed form.  These
 * entry points joined ABI 23: additions only, no signature changed.
 *
 * Honest rows g_1 .. g_h, 2 <= h <= BM_MAX_ROWS, D_ij = |g_i - g_j|^2 (bm_pairwise_sqdist).  The Byzantine vector is
 * m = avg + gamma p: avg the sequential fp32 mean bm_stack_stats writes (same bits), p a perturbation direction, gamma
 * the largest factor that keeps m as close to the honest rows as they are to each other.  Every distance involved is a
 * quadratic in gamma with scalar coefficients, so gamma has a closed form (the paper halves a step on d-sized vectors).
 *   p      BM_PERTURB_UNIT  -avg                 (the paper's -avg / |avg| unnormalised: same m, gamma in units of |avg|)
 *          BM_PERTURB_STD   -sqrt(q / (h - 1))   q = the column's sum (x - avg)^2 as bm_stack_stats forms it: the bits of
 *                                                its BM_ATTACK_LITTLE | BM_ATTACK_DIRECTION output at scale -1
 *          BM_PERTURB_SIGN  -sign(avg)           sign(+-0) = 0, a NaN stays NaN
 *   b_i = <p, avg - g_i>  (sum of p_c (avg_c - g_ic), not a difference of two dots)    P = |p|^2    N = |avg|^2
 *   a_i = |avg - g_i|^2 = (1/h) sum_j D_ij - (1/(2 h^2)) sum_ij D_ij, from D; a value <= 0 counts as +0
 *   Min-Max  R = max_{i<j} D_ij;  gamma_i = (-b_i + sqrt(b_i^2 + P (R - a_i))) / P;  gamma = min_i gamma_i, ties to the
 *            lower index: the binding row
 *   Min-Sum  S = max_i sum_j D_ij, A = sum_i a_i, B = sum_i b_i (the computed one, analytically 0);
 *            gamma = (-B + sqrt(B^2 + h P (S - A))) / (h P)
 *   degenerate: P not > 0, a scalar the formula reads (or gamma) not finite, or a negative discriminant: gamma = +0 and
 *            the flag is set — the vector is then avg itself.
 * Every fp64 sum runs in plain index order (the row sums of D over j, the sums over the rows over i), on host and
 * device alike.
 *
 * bm_perturb_stats: ONE pass over the h rows (h + 2 row units of traffic): avg_out and dir_out = p (DEVICE, d floats
 *   each, must not overlap each other or a row) and scal_out (DEVICE, BM_PERTURB_SLOTS doubles) = { b_0 .. b_{h-1}, zeros
 *   up to BM_MAX_ROWS, P, N } over the d coordinates given — this shard's part: all are sums over coordinates.  Per-lane
 *   fp32 chains of at most 16 iterations, then fp64: across the wave, per workgroup into ws
 *   (bm_perturb_workspace_bytes(d)), and a finish kernel that adds the workgroups' partials in a fixed order.  No float
 *   atomics, no synchronisation: two calls on the same input give the same bits.  Rows may be separately allocated, of
 *   any 4-byte alignment.  d == 0 is legal (an empty shard): the scalars are zeros.  BM_EINVAL before any HIP call for a
 *   null pointer (avg_out / dir_out may be NULL when d == 0), h outside 2 .. BM_MAX_ROWS, an unknown kind, d < 0 or
 *   overlapping outputs.
 * bm_minmax_factor: HOST function on HOST arrays (sq: h x h doubles, scal: BM_PERTURB_SLOTS doubles), no stream.
 *   bm_minmax_factor_device: the same on the DEVICE arrays where bm_pairwise_sqdist and bm_perturb_stats left them, one
 *   workgroup, D in LDS, no copy, no synchronisation; the same bits (csrc/minmax_core.h, one definition for both).
 *   out: 6 doubles = { gamma, the bound R or S, the binding row (-1: Min-Sum, or degenerate), P, N, degenerate 0 / 1 }.
 *   BM_EINVAL for a null pointer, h outside 2 .. BM_MAX_ROWS or an unknown mode before any HIP call.
 * The vector: bm_multi_fma3_bdev(out, avg, dir, a = 1, b_dev = &out[0]). */
#define BM_PERTURB_SLOTS (BM_MAX_ROWS + 2)
enum bm_perturb_kind { BM_PERTURB_UNIT = 0, BM_PERTURB_STD = 1, BM_PERTURB_SIGN = 2 };
enum bm_minmax_mode { BM_MINMAX = 0, BM_MINSUM = 1 };
int64_t bm_perturb_workspace_bytes(int64_t d);
int bm_perturb_stats(const float* const* rows, int h, int64_t d, int kind, float* avg_out, float* dir_out,
                     double* scal_out, void* ws, void* stream);
int bm_minmax_factor(const double* sq_host, const double* scal_host, int h, int mode, double* out_host);
int bm_minmax_factor_device(const double* sq_dev, const double* scal_dev, int h, int mode, double* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BM_GAR_H */
