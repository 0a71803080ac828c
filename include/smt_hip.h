/*
 * smt_hip.h -- C ABI of libsmt_hip.so, the MI355X (gfx950) kernel library for the
 * VQ-VAE train-step hot path of vliu15/speech-masters-thesis.
 *
 * The reference is pure Python/PyTorch and has NO native/FFI interface
 * (SURVEY.md 8(b)); each entry point therefore cites the reference *Python
 * expression* it replaces (file:line relative to the reference root).  The
 * binding a maintainer would add is a ctypes stub: see INTEGRATION.md.
 *
 * Conventions (all entry points):
 *   - plain C types only: device pointers, sizes, a hipStream_t passed as void*;
 *   - return 0 on success, non-zero on error; smt_last_error() gives the
 *     thread-local message of the last failing call;
 *   - never allocate or free caller-visible memory: scratch is passed in, sized
 *     by the matching *_workspace_bytes() query;
 *   - asynchronous on `stream`; no host synchronisation inside (graph-capturable);
 *   - activations are channels-last: a [B, C, T] reference tensor is held as
 *     [B, T, C] ("NTC") so that one time step's channels are contiguous.
 */
#ifndef SMT_HIP_H
#define SMT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* smt_stream_t; /* hipStream_t */

/* dtype tags for activation / weight buffers of the conv stack */
enum { SMT_F32 = 0, SMT_BF16 = 1 };

const char* smt_last_error(void);
int smt_abi_version(void);

/* ------------------------------------------------------------------ VQ ---- */
/* Per-codebook derived data of the nearest-code search (mean, centred bf16-pair split of the codes, -|k~|^2/2,
 * max |k~|^2), kept in a caller-owned persistent buffer so that it is rebuilt only when the codebook changes:
 * smt_vq_ema_apply refreshes it in the same call that rewrites the codebook; call smt_vq_prepare after any other
 * write to `codebook` (initialisation, checkpoint load). */
size_t smt_vq_prep_bytes(int k_bins, int dim);
int smt_vq_prepare(const float* codebook, int k_bins, int dim, void* prep, size_t prep_bytes, smt_stream_t stream);

/* BottleneckBlock.quantize + dequantize (models/vqvae/bottleneck.py:126-145)
 * and the per-row terms of the commit loss / fit metric (:140, :194).
 *
 *   x        [n_rows, dim]  f32, encoder output rows (NTC flattening, :92-98)
 *   codebook [k_bins, dim]  f32 (buffer `k`)
 *   prep     the buffer smt_vq_prepare / smt_vq_ema_apply filled for THIS codebook content, or NULL (then it is
 *            rebuilt inside the call, in the workspace).  It also carries the call's queue counter (zero between
 *            calls): one forward at a time per prep buffer.
 *   row_mask [n_rows]       f32 0/1 or NULL (= all ones)
 * outputs
 *   idx      [n_rows] int64  exact argmin_j ||x - k_j||^2, lowest j on ties
 *   min_dist [n_rows] f32    ||x - k_idx||^2
 *   x_d      [n_rows, dim]   k[idx] * row_mask   (may be NULL)
 *   sums     [4] f32: {sum_all min_dist, sum_masked min_dist, sum mask,
 *                      number of rows that needed exact (fp64) re-scoring}
 * A row of x that holds a NaN has no finite distance: it gets idx 0, a NaN min_dist and x_d = k[0] * row_mask (what the
 * reference's min over a NaN distance row dequantises, and what the grouped quantiser writes); the sums over it are NaN.
 * dim in {32, 64, 128}; k_bins >= 1. */
size_t smt_vq_forward_workspace_bytes(int64_t n_rows, int k_bins, int dim);
int smt_vq_forward(const float* x, const float* codebook, void* prep, const float* row_mask,
                   int64_t n_rows, int k_bins, int dim,
                   int64_t* idx, float* min_dist, float* x_d, float* sums,
                   void* workspace, size_t workspace_bytes, smt_stream_t stream);

/* Backward of the straight-through estimator + commit loss
 * (bottleneck.py:194-201):  dx = dy*mask + g_commit * 2 (x - x_d) mask / (sum_mask * dim)
 *   x_d       [n_rows, dim] the x_d written by smt_vq_forward (= k[idx] on unmasked rows; masks are 0/1)
 *   dy        [n_rows, dim] grad of the (masked) quantised output, or NULL
 *   g_commit  [1] device scalar: upstream grad of the commit loss, or NULL
 *   sums      the `sums` written by smt_vq_forward (reads sums[2]) */
int smt_vq_backward(const float* x, const float* x_d, const float* row_mask, const float* dy,
                    const float* g_commit, const float* sums, int64_t n_rows, int dim, float* dx,
                    smt_stream_t stream);

/* Codebook EMA statistics, BottleneckBlock.update_k (bottleneck.py:64-68):
 * _k_sum = onehot @ x, _k_elem = onehot.sum(-1) over UNMASKED rows.
 *   stats [k_bins*dim + k_bins] f32: sums then counts; written by this call.
 * The rows are grouped by code first (counting sort, LDS-privatised histograms) and each wave sums a share of the sorted
 * order in registers: one 64-bit fixed-point integer atomic (units of 2^-24) per channel per (share, code) boundary, not per
 * row -- so the time does not depend on how skewed the code usage is, and the sums are bit-reproducible whatever order the
 * rows arrive in.  Exact for |x| < 2^15 on a 2^-24 grid (saturating beyond 2^39 units per element).
 * k_bins <= 16384 runs as described; larger tables (the grouped quantiser below: n_groups * l_bins, up to 262144) run the same
 * counting sort with the histogram in global memory and a multi-workgroup scan, then the same summation: same sums, same
 * bit-reproducibility.  A code outside [0, k_bins) is ignored by the large path. */
size_t smt_vq_ema_accumulate_workspace_bytes(int64_t n_rows, int k_bins, int dim);
int smt_vq_ema_accumulate(const float* x, const int64_t* idx, const float* row_mask,
                          int64_t n_rows, int k_bins, int dim, float* stats, void* workspace, size_t workspace_bytes,
                          smt_stream_t stream);

/* bottleneck.py:78-90: EMA mix, dead-code revival from k_rand, metrics; refreshes `prep` for the new codebook.
 *   stats   as above (after the cross-rank SUM, :74-75)
 *   k_rand  [k_bins, dim] revival candidates (rank 0's, :73)
 *   metrics [4] f32: {entropy, used_curr, usage, dk}
 *   prep    smt_vq_prep_bytes(k_bins, dim) bytes (its previous content is not read) */
int smt_vq_ema_apply(float* codebook, float* k_sum, float* k_elem, const float* stats,
                     const float* k_rand, float mu, float threshold, int k_bins, int dim,
                     float* metrics, void* prep, size_t prep_bytes, smt_stream_t stream);


/* ---- grouped quantiser: the text-conditioned bottleneck of VQTTS (models/vqtts/bottleneck.py:19-77) ----
 * The codebook holds n_groups * l_bins codes; row r searches ONLY the l_bins codes of its group, rows
 * [group[r] * l_bins, (group[r] + 1) * l_bins).  The reference gathers k[x_id] ([n, l_bins, dim]) and calls bmm; here the
 * rows are bucketed by group and tiles of rows of one group sweep that group's codes: no gather, workspace O(n_rows).
 * dim in {32, 64, 128}; l_bins a multiple of 32 in [32, 1024]; 1 <= n_groups <= 256; 0 <= n_rows <= 2^20.  Anything else is
 * an argument error (smt_vq_grouped_prep_bytes then returns 0).
 *
 * smt_vq_grouped_prepare: the per-GROUP derived data (mean of the group's codes, centred bf16-pair split, -|k~|^2/2,
 * max |k~|^2) in a caller-owned persistent buffer; same contract as smt_vq_prepare: smt_vq_grouped_ema_apply refreshes it,
 * call this after any other write to `codebook`. */
size_t smt_vq_grouped_prep_bytes(int n_groups, int l_bins, int dim);
int smt_vq_grouped_prepare(const float* codebook, int n_groups, int l_bins, int dim, void* prep, size_t prep_bytes,
                           smt_stream_t stream);

/* bottleneck.py:24-28: group[b, j] = x_id[b, align_idx[b, j]] and row_mask[b, j] = 1 where frame j has a token, else group 0
 * and mask 0 (what matmul(x_id, attn) and attn.sum(1) give).
 *   x_id      [batch, t_x] int64 token ids; the caller guarantees 0 <= id < n_groups (the kernel clamps, it never faults)
 *   align_idx [batch, t_y] int32, the convention of smt_glow_align_index: the token of frame j, -1 = none
 *   group     [batch * t_y] int32, row_mask [batch * t_y] f32: outputs */
int smt_vq_align_groups(const int64_t* x_id, const int* align_idx, int batch, int t_x, int t_y, int n_groups,
                        int* group, float* row_mask, smt_stream_t stream);

/* Grouped nearest-code search + dequantise (bottleneck.py:38-60).
 *   x [n_rows, dim] f32; group [n_rows] int32 in [0, n_groups) (clamped); codebook [n_groups * l_bins, dim] f32;
 *   prep     the buffer smt_vq_grouped_prepare / smt_vq_grouped_ema_apply filled for THIS codebook content (required);
 *   row_mask [n_rows] f32 0/1 or NULL.  Masked rows ARE searched, in whatever group they carry (smt_vq_align_groups: 0):
 *            the reference's fit sums min_dist over all rows; x_d is zero there.
 * outputs
 *   q_rel    [n_rows] int64  exact argmin over the group's codes of ||x - k_j||^2 (fp32 inputs), lowest index on ties
 *   q_abs    [n_rows] int64  group * l_bins + q_rel
 *   min_dist [n_rows] f32, x_d [n_rows, dim] = codebook[q_abs] * row_mask (may be NULL), sums [4] as smt_vq_forward.
 * x_d, row_mask and sums feed smt_vq_backward unchanged. */
size_t smt_vq_grouped_forward_workspace_bytes(int64_t n_rows);
int smt_vq_grouped_forward(const float* x, const int* group, const float* codebook, void* prep, const float* row_mask,
                           int64_t n_rows, int n_groups, int l_bins, int dim,
                           int64_t* q_rel, int64_t* q_abs, float* min_dist, float* x_d, float* sums,
                           void* workspace, size_t workspace_bytes, smt_stream_t stream);

/* smt_vq_ema_apply for the grouped codebook (k_bins = n_groups * l_bins; stats from smt_vq_ema_accumulate on q_abs):
 * same update and metrics, and `prep` (smt_vq_grouped_prep_bytes) is refreshed per group for the new codebook. */
int smt_vq_grouped_ema_apply(float* codebook, float* k_sum, float* k_elem, const float* stats,
                             const float* k_rand, float mu, float threshold, int n_groups, int l_bins, int dim,
                             float* metrics, void* prep, size_t prep_bytes, smt_stream_t stream);


/* --------------------------------------------------------------- losses ---- */
/* MultiNormReconstructionLoss (models/vqvae/losses.py:73-80) on [batch, t] fp32 signals, d = (y - yh) * [i < lens[b]]:
 * per clip the plain sums and the sum of the `topk` largest d^2 (exact k-th-largest threshold by radix select; the
 * reference materialises d^2 and calls torch.topk).  stats [batch][8] f32 =
 *   {sum d^2, sum |d|, sum of the topk largest d^2, threshold tau, #(d^2 > tau), #(d^2 == tau), 0, 0};
 * loss = l1 * sum_b stats[b][1] / (B t) + l2 * sum_b stats[b][0] / (B t) + linf * sum_b stats[b][2] / B (host side). */
int smt_recon_loss_fwd(const float* y, const float* yh, const int* lens, int batch, int t, int topk, float* stats,
                       smt_stream_t stream);
/* d loss / d yh given the stats of the forward and coef [3] (device) = upstream gradient times
 * {l1 / (B t), 2 l2 / (B t), 2 linf / B}. */
int smt_recon_loss_bwd(const float* y, const float* yh, const int* lens, const float* stats, const float* coef,
                       int batch, int t, int topk, float* dyh, smt_stream_t stream);

/* ------------------------------------------------------------------ MAS ---- */
/* GlowTTS monotonic alignment search, `maximum_path` (models/glow_tts/submodules.py:28-67), on the device instead of the
 * reference's numpy loop on the host: value / mask / path are [batch, t_x, t_y] fp32 (mask 0/1), max_neg_val = -inf in the
 * reference's calls.  path is the 0/1 alignment, bit-identical to the numpy result. */
int smt_maximum_path(const float* value, const float* mask, int batch, int t_x, int t_y, float max_neg_val, float* path,
                     smt_stream_t stream);

/* ------------------------------------------------------ VQTTS alignment ---- */
/* Text-audio alignment of VQTTS (models/vqtts/vqtts.py:133-137, 150-156; ABI 9).  All tensors channels-last fp32:
 * x_enc [batch, t_x, dim] (text encoder means), y_enc [batch, t_q, dim] (audio encoder output), x_lens / q_lens [batch]
 * int32 on the device; nothing synchronises with the host.  Limits of every entry: dim a multiple of 4 up to 256,
 * t_x <= 512, t_q <= 32768, batch <= 65535 -- an argument error that names the limit otherwise.  Inputs are finite.
 *
 * distance: dist[b, i, j] = sqrtf(sum_d (x[b, i, d] - y[b, j, d])^2), the squared differences accumulated with fmaf in
 *   ascending d (no |x|^2 + |y|^2 - 2xy expansion).  Dense; for tests and small shapes.
 * align: the distance fused with the monotonic search, no [batch, t_x, t_q] tensor anywhere.  idx [batch, t_q] int32 =
 *   the token of each frame, -1 = none (the convention of smt_glow_align_index); dur [batch, t_x] = frames per token.
 *   For every item, whatever its lengths (0 and q_len < x_len included), both are bit-identical to
 *   smt_glow_align_index(smt_maximum_path(value = -dist, mask, max_neg_val = -inf)) with dist from smt_vqtts_distance and
 *   mask[b, i, j] = (i < x_lens[b]) (j < q_lens[b]); rows of x_enc / y_enc at or past the lengths are never read.
 *   workspace: smt_vqtts_align_workspace_bytes = batch * t_q * ceil(t_x / 64) * 8 bytes (direction bits), 8-byte aligned.
 * align_loss: frame_dist[b, j] = dist(x[b, idx[b, j]], y[b, j]) (0 where idx < 0), sum[0] = their sum in a fixed order
 *   (equal inputs give equal bits).  bwd with the DEVICE scalar coef = g / denom: dy[b, j] = coef (y_j - x_i) / dist,
 *   dx[b, i] = -(sum of dy over the frames of token i, in frame order; idx must be a monotonic path, as align returns).
 *   A frame with dist == 0 contributes 0 to both (the reference's sqrt backward gives NaN there); idx < 0 gives dy = 0. */
int smt_vqtts_distance(const float* x_enc, const float* y_enc, float* dist, int batch, int t_x, int t_q, int dim,
                       smt_stream_t stream);
size_t smt_vqtts_align_workspace_bytes(int batch, int t_x, int t_q);
int smt_vqtts_align(const float* x_enc, const float* y_enc, const int* x_lens, const int* q_lens, int batch, int t_x, int t_q,
                    int dim, int* idx, float* dur, void* workspace, size_t workspace_bytes, smt_stream_t stream);
int smt_vqtts_align_loss(const float* x_enc, const float* y_enc, const int* idx, int batch, int t_x, int t_q, int dim,
                         float* frame_dist, float* sum, smt_stream_t stream);
int smt_vqtts_align_loss_bwd(const float* x_enc, const float* y_enc, const int* idx, const float* frame_dist, const float* coef,
                             int batch, int t_x, int t_q, int dim, float* dx, float* dy, smt_stream_t stream);

/* ------------------------------------------------------ VQTTS code head ---- */
/* The code predictor's projection fused with its cross-entropy (models/vqtts/vqtts.py:86-87, 142-144, 157, 175-178, 190;
 * ABI 10): logits = h . weight^T + bias are formed tile by tile on the MFMA and never stored, nor is their gradient.
 * h [rows, channels] fp32 channels-last rows, weight [bins, channels] and bias [bins] fp32, target [rows] int64 with
 * target < 0 = "not scored" (the convention of smt_lm_ce_fwd; a scored target must be < bins).  Nothing synchronises with
 * the host.  Limits of every entry: channels a multiple of 16 up to 256, bins a multiple of 32 up to 1024, rows up to
 * 2^31 - 1 -- an argument error that names the limit otherwise.  h, dh and both workspaces are 16-byte aligned.
 *
 * Arithmetic of a logit: every fp32 operand is split into a bf16 pair, hi = bf16(x), lo = bf16(x - hi), and bias +
 *   sum (w_lo h_hi + w_hi h_lo + w_hi h_hi) is accumulated in fp32 by v_mfma_f32_32x32x16_bf16, 16 channels per step in
 *   ascending order -- the same instruction sequence for every column, so equal weight rows give equal logits.
 *   |logit - exact| <= 2^-15 (sum_c |h_c||w_c| + |b|).
 * prepare: splits weight into `workspace` (smt_vqtts_code_head_workspace_bytes = 8 * bins * padded channels, channels
 *   padded to 32 / 64 / 128 / 256); once per weight version, the workspace is read-only afterwards.
 * fwd: per row lse = logsumexp(logits) (online, stable), pred = argmax (lowest index on ties, int32),
 *   row_loss = lse - logit[target] and correct = (pred == target) as 0/1, both 0 on unscored rows; then
 *   sums[0..2] = sum of row_loss, sum of correct, number of scored rows as DOUBLES, added in a fixed order in two stages
 *   (equal inputs give equal bits); `sums` holds 3 + 3 * 256 doubles, the rest is the first stage's partial sums.
 *   target == NULL is the synthesis form: only pred and, if lse != NULL, lse are written.  rows == 0 writes three zeros
 *   (nothing in the synthesis form) and takes NULL for h and the per-row outputs.
 * bwd: with the DEVICE scalar coef = g / count and the saved lse it recomputes the logits with the same arithmetic,
 *   p = exp(logit - lse), G = coef (p - onehot(target)), 0 on unscored rows, and writes dh = G . weight [rows, channels],
 *   dweight = G^T . h [bins, channels], dbias = sum_r G; G's bf16 pair feeds the MFMAs the same way.  dweight / dbias:
 *   one slab per row slice in `scratch` (smt_vqtts_code_head_bwd_workspace_bytes), added in slice order in fp64 -- no
 *   float atomics, equal inputs give equal bits.
 * sample (an addition to ABI 10): the synthesis form with a draw instead of the argmax.  rows = batch * t_q; row r is frame
 *   j = r % t_q of item b = r / t_q; seeds [batch] int32 in device memory.  Per row, with the logits of fwd bit for bit:
 *     key   = fmix32(fmix32((uint32)seeds[b]) + (uint32)j * 0x9E3779B1)          (fmix32 of the dropout spec below)
 *     bits  = fmix32(key + (uint32)v * 0x85EBCA77)                               per bin v
 *     u     = ((bits >> 9) + 0.5) * 2^-23                                        exact in fp32, strictly inside (0, 1)
 *     g     = -logf(-logf(u))                                                    Gumbel noise
 *     score = fmaf(logit, inv_temperature, g)
 *     M = max_v logit_v;  bin v is KEPT iff logit_v >= M + cut (fp32)
 *     pred  = the kept bin with the highest score, lowest index on ties;  n_kept = number of kept bins (may be NULL)
 *   -- a sample of softmax(logit * inv_temperature) restricted to the bins with p_v / p_max >= min_p (min-p), where
 *   cut = T ln(min_p) <= 0 is computed by the host in double and rounded once; cut = -inf keeps every bin (one sweep over
 *   the weight; a finite cut takes two, and the maximum is always kept: n_kept >= 1).  A frame's draw depends on
 *   (seeds[b], j, v) only, not on t_q, the batch position or the launch geometry.  inv_temperature finite and > 0,
 *   t_q >= 1, rows % t_q == 0 -- an argument error otherwise.  One launch, no atomics, no workspace beyond the split;
 *   equal inputs give equal bits.  rows == 0 launches nothing. */
size_t smt_vqtts_code_head_workspace_bytes(int channels, int bins);
int smt_vqtts_code_head_prepare(const float* weight, int channels, int bins, void* workspace, size_t workspace_bytes,
                                smt_stream_t stream);
int smt_vqtts_code_head_fwd(const float* h, const void* workspace, size_t workspace_bytes, const float* bias,
                            const int64_t* target, int64_t rows, int channels, int bins, float* lse, float* row_loss, int* pred,
                            float* correct, double* sums, smt_stream_t stream);
int smt_vqtts_code_head_sample(const float* h, const void* workspace, size_t workspace_bytes, const float* bias,
                               const int* seeds, int64_t rows, int t_q, int channels, int bins, float inv_temperature, float cut,
                               int* pred, int* n_kept, smt_stream_t stream);
size_t smt_vqtts_code_head_bwd_workspace_bytes(int64_t rows, int channels, int bins);
int smt_vqtts_code_head_bwd(const float* h, const void* workspace, size_t workspace_bytes, const float* bias,
                            const int64_t* target, const float* lse, const float* coef, int64_t rows, int channels, int bins,
                            float* dh, float* dweight, float* dbias, void* scratch, size_t scratch_bytes, smt_stream_t stream);

/* ------------------------------------------------------ VQTTS code emission ---- */
/* The synthesis side of the grouped bottleneck (models/vqtts/vqtts.py:170-174; an addition to ABI 10): the predicted
 * relative code of a frame becomes its absolute code and its codebook row.  pred [batch, t_q] int32 (the code head's
 * argmax), x_id [batch, t_x] int64 token ids, idx [batch, t_q] int32 frame -> token (-1 = none), q_lens [batch] int32,
 * codebook [n_vocab * l_bins, dim] fp32; outputs q_abs [batch, t_q] int64 (may be NULL) and y_d [batch, t_q, dim] fp32.
 * Per frame (b, j): i = idx[b, j], tok = x_id[b, i], q = tok * l_bins + pred[b, j].  The frame HAS A CODE iff
 * j < q_lens[b], 0 <= i < t_x, 0 <= tok < n_vocab and 0 <= pred[b, j] < l_bins.  With a code q_abs[b, j] = q and
 * y_d[b, j, :] = codebook[q, :] bit for bit; without one q_abs[b, j] = -1 and the row is exactly 0.0f.  Nothing outside
 * the arrays is read: x_id is not read when i is out of range, codebook is not read when the frame has no code.
 * One launch on `stream`, no host synchronisation, no atomics, no workspace; equal inputs give equal bits.  dim must be
 * a multiple of 4 and codebook / y_d 16-byte aligned (a row moves as 16-byte loads and stores) -- an argument error
 * otherwise.  batch, t_q or dim of 0 is a no-op that returns 0. */
int smt_vqtts_emit(const int* pred, const int64_t* x_id, const int* idx, const int* q_lens, const float* codebook, int batch,
                   int t_x, int t_q, int n_vocab, int l_bins, int dim, int64_t* q_abs, float* y_d, smt_stream_t stream);

/* ------------------------------------------------------------ conv stack ---- */
/* Counter-based dropout ("dropout" spec).  The reference draws dropout masks from torch's global
 * RNG (models/vqvae/resnet.py:22,25), which no other device can reproduce; this build defines a
 * stateless generator so that train mode is parity-testable and backward can recompute the mask:
 *   keep(i) = ((fmix32((uint32)(i >> 1) * 0x9E3779B1 + key) >> (16 * (i & 1))) & 0xFFFF) >= thresh16
 * i = linear channels-last index ((b*T + t)*C + c) of the tensor being dropped, fmix32 = MurmurHash3's
 * finaliser, key = per (step seed, site) 32-bit key, thresh16 = round(p * 65536); kept values are
 * scaled by drop_scale = 1/(1-p).  oracle/vqvae_oracle.py restates it bit-exactly. */

/* Repack an fp32 torch-layout weight into the [taps][n_out][n_in] operand layout (dtype SMT_F32 /
 * SMT_BF16):  dst[tap][o][i] = src[o*stride_out + i*stride_in + tap_map[tap]*stride_tap]. */
int smt_pack_weight(const float* src, void* dst, int dtype, int n_out, int n_in, int taps,
                    int64_t stride_out, int64_t stride_in, int64_t stride_tap, const int* tap_map,
                    int swizzle, smt_stream_t stream);
/* swizzle = 1 (bf16, n_in % 128 == 0): LDS-DMA operand layout -- inside every group of 128 input channels the
 * 8-channel chunk c of row o is stored at chunk position c ^ (o & 15); pass w_swizzled = 1 with it. */

/* The same repack for MANY weights in one launch.  `table_dev` is an array of smt_pack_entry in DEVICE memory (built
 * once by the host: parameter storage is stable across optimiser steps); dst element index of (tap, o, i) is
 * dst_offset + tap*dst_tap_stride + o*dst_row_stride + i' (i' = i, or the swizzled position for swizzle = 1), so several
 * weights can be packed side by side into one operand (K1 of the four branches).  Block b of the launch handles elements
 * [1024*block_local_dev[b], +1024) of table row block_entry_dev[b]. */
typedef struct smt_pack_entry {
  const float* src; void* dst;
  int64_t stride_out, stride_in, stride_tap;
  int64_t dst_offset, dst_tap_stride, dst_row_stride;
  int dtype, n_out, n_in, taps, swizzle;
  int tap_map[16];
} smt_pack_entry;
int smt_pack_weights_batched(const smt_pack_entry* table_dev, const int* block_entry_dev, const int* block_local_dev,
                             int n_blocks, smt_stream_t stream);

/* One implicit-GEMM convolution over channels-last activations (forward, or a data gradient, which
 * is the same computation on repacked weights):
 *   y[b, t*out_stride + out_offset, co] =
 *       epi( bias[co] + sum_{j<taps} sum_ci x[b, t*stride + j*dilation - padding, ci] * w[j][co][ci] )
 *   rows t_in >= lens_in[b] of x read as 0 (the row mask of MaskedConv1d, conv.py:7-10);
 *   epi, in this order: if act_grad: times scale*[u != 0] with u = act_grad_src (the derivative of
 *        relu(dropout(.)) at an activated tensor u that this library produced); rows >= lens_out[b] -> 0;
 *        + res.
 *   if act_out: additionally y_act = relu(dropout(y)) (resnet.py:22-26) with the counter-based
 *        generator below; channel block [s*site_width, (s+1)*site_width) is dropout site s with key
 *        drop_keys[s] and index i = (b*t_y + t)*site_width + (co - s*site_width).  y may be NULL then.
 * Replaces F.conv1d / F.conv_transpose1d of models/vqvae/conv.py:5-18, resnet.py:24,27,205,217 and
 * their autograd data-gradients.  c_in % 16 == 0 (bf16) or % 8 (f32). */
typedef struct smt_conv_desc {
  int dtype;                       /* SMT_F32 | SMT_BF16: x, w, y, y_act, res, act_grad_src */
  int batch, t_in, t_out, t_y;     /* t_out: number of t computed; t_y: rows of y per batch item */
  int c_in, c_out;
  int taps, stride, dilation, padding, out_stride, out_offset;
  int act_out, act_grad, site_width;
  int ld_x, ld_y, ld_res, ld_act, ld_yact;  /* row pitches in elements */
  uint32_t drop_keys[8];
  uint32_t drop_thresh16;
  float drop_scale;
  int64_t bs_x, bs_y, bs_res, bs_act, bs_yact;  /* batch strides in elements */
  const void* x; const void* w; const float* bias; void* y; void* y_act;
  const void* res; const void* act_grad_src;
  const int* lens_in; const int* lens_out;
  int w_swizzled;                  /* w was packed with swizzle = 1: enables the LDS-DMA kernel */
  const void* zero_page;           /* >= 256 zero bytes in device memory (source of out-of-range rows), or NULL.  Since round 3
                                    * the fused streaming entries (smt_conv_k3gate_fwd, smt_conv_k1_bwd, smt_conv_gate_bwd,
                                    * smt_conv1x1_bwd, smt_conv4s2, smt_convt4s2, the K1 activated-output path) address their
                                    * operands through range-checked buffer descriptors and no longer read it; the argument
                                    * stays in their signatures (ABI 3) and must still be non-NULL where it was required. */
  /* Optional second 1x1 term folded into the same output (bf16 1x1 LDS-DMA path only, c_in == 128, c_in2 == 64):
   *   y += bias2[co] + sum_ci2 x2[b, t, ci2] * w2[co][ci2]
   * GatedHiFiBlock adds the branch input h1 = K1(x) + b1 to K3's output (resnet.py:226); K1 being linear, the
   * residual can be recomputed from x inside K3 instead of being written and read back as a 2w-wide tensor. */
  const void* x2; const void* w2;  /* x2 [B, t, c_in2] (pitch ld_x2, batch stride bs_x2); w2 [c_out][c_in2] packed, swizzle 0 */
  const float* bias2;
  const int* lens_in2;             /* rows >= lens_in2[b] of x2 read as 0 (lens_in applies to x only), or NULL */
  int c_in2, ld_x2;
  int64_t bs_x2;
  /* Dropout keys in DEVICE memory (or NULL): site s uses drop_keys_dev[s * drop_keys_dev_stride] instead of drop_keys[s].
   * A captured hipGraph freezes by-value arguments; a graphed train step keeps a table of per-site keys on the device and
   * refreshes it with smt_lm_make_keys (the same derivation as the host's) before the first convolution of every step. */
  const uint32_t* drop_keys_dev;
  int drop_keys_dev_stride;
} smt_conv_desc;
int smt_conv1d_ntc(const smt_conv_desc* desc, smt_stream_t stream);
/* Name of the kernel smt_conv1d_ntc dispatches this descriptor to ("conv_gemm", "conv_gemm_dma", "conv_ws",
 * "conv_ws_pipe", "conv1x1_dma", "conv1x1_fold", "conv_k1act"): for profilers and tests; no device work. */
const char* smt_conv1d_kernel_name(const smt_conv_desc* desc);
/* The plan behind the name "conv_gemm_dma", which covers two tile sizes with and without dilation classes: *tile_rows =
 * output rows per workgroup (128 or 256), *row_classes = number of row classes the launch is split into (the dilation
 * where the class decomposition is on, else 1).  Both are 0 for a descriptor that any other kernel runs (the
 * weight-stationary kernels plan their own tiles).  Answered by the launch's own plan; no device work.  Returns 0. */
int smt_conv1d_dma_plan(const smt_conv_desc* desc, int* tile_rows, int* row_classes);

/* Weight (+ bias) gradient of the same convolution:
 *   dw[j][co][ci] = sum_{b,t} dy[b, t*out_stride + out_offset, co] * x[b, t*stride + j*dil - pad, ci]
 *   db[co]        = sum_{b,t} dy[b, ., co]                                   (if dbias != NULL)
 * written in fp32 to dweight[o*stride_out + i*stride_in + tap_map[tap]*stride_tap] (torch layout).
 * `desc` is the forward descriptor with y := dy (w, bias, res, act_*, y_act unused). */
size_t smt_conv1d_wgrad_workspace_bytes(const smt_conv_desc* desc);
int smt_conv1d_wgrad(const smt_conv_desc* desc, float* dweight, int64_t stride_out, int64_t stride_in,
                     int64_t stride_tap, const int* tap_map, float* dbias, void* workspace,
                     size_t workspace_bytes, smt_stream_t stream);
/* Every weight-gradient entry point (smt_conv1d_wgrad, smt_conv1x1_bwd, smt_conv_k1_bwd, smt_conv_gate_bwd) leaves
 * per-workgroup partial sums in its workspace and then reduces them in a fixed order (bitwise reproducible).  Between
 * smt_wgrad_reduce_defer(1, .) and smt_wgrad_reduce_defer(0, stream) the calls of this thread only QUEUE that reduction
 * (up to 16 per launch, job descriptors travel by value in the kernel arguments): each call must then be handed a workspace
 * of its own that stays untouched until the closing call, which launches the queued reductions on `stream`.  dweight / dbias
 * are valid once that launch has run.  Replaces autograd's per-layer weight gradients of the reference (the convolutions of
 * models/vqvae/resnet.py:205-241): one reduction launch per GatedHiFiBlock instead of ten. */
int smt_wgrad_reduce_defer(int on, smt_stream_t stream);
/* Name of the kernel smt_conv1d_wgrad runs for this descriptor ("conv_wgrad_shift", "conv_wgrad_dma", "conv_wgrad");
 * no device work. */
const char* smt_conv1d_wgrad_kernel_name(const smt_conv_desc* desc);

/* Fused backward of a bf16 128 -> 128 1x1 convolution whose forward input was u = relu(dropout(h)) (K3 of
 * GatedHiFiBlock, resnet.py:218-227): one pass over dy and u yields the masked data gradient AND the weight / bias
 * gradients.  `desc` is the 1x1 DATA-GRADIENT descriptor as for smt_conv1d_ntc (x = dy, y = dx, w = weights packed
 * [ci][co] with swizzle = 1, act_grad = 1 with act_grad_src = u, drop_scale, zero_page; no bias / res / act_out);
 * dweight[co*stride_out + ci*stride_in] = sum_t dy[t,co] * u[t,ci], dbias[co] = sum_t dy[t,co] (fp32, may be NULL). */
size_t smt_conv1x1_bwd_workspace_bytes(const smt_conv_desc* desc);
int smt_conv1x1_bwd(const smt_conv_desc* desc, float* dweight, int64_t stride_out, int64_t stride_in, float* dbias,
                    void* workspace, size_t workspace_bytes, smt_stream_t stream);

/* Fused backward of K1 of GatedHiFiBlock for all branches at once (bf16, 64 -> 512 1x1; resnet.py:205-216 and the
 * block residual resnet.py:241):  dx[t,ci] = keep(t) * sum_co dh[t,co] * W[co][ci] + res[t,ci]  (keep = t < lens[b]),
 * dweight[co*stride_out + ci*stride_in] = sum_t dh[t,co] * x[t,ci] (x rows >= lens[b] read as 0), dbias[co] = sum_t dh.
 * dh [B,t,512], x / res / dx [B,t,64] with explicit pitches; w_packed_bwd = smt_pack_weight(..) layout [ci][co],
 * swizzle 0; zero_page >= 256 zero bytes.  One pass over dh instead of a data-gradient and a weight-gradient pass. */
size_t smt_conv_k1_bwd_workspace_bytes(int batch, int t);
int smt_conv_k1_bwd(const void* dh, int64_t bs_dh, int ld_dh, const void* x, int64_t bs_x, int ld_x,
                    const void* w_packed_bwd, const void* res, int64_t bs_res, int ld_res, void* dx, int64_t bs_dx,
                    int ld_dx, const int* lens, int batch, int t, const void* zero_page, float* dweight,
                    int64_t stride_out, int64_t stride_in, float* dbias, void* workspace, size_t workspace_bytes,
                    smt_stream_t stream);

/* The k = 4 / stride 2 / padding 1 resampling convolutions at width 64 (bf16; conv.py:61-78,111-137) as HBM-streaming kernels:
 *   smt_convt4s2: y[b, 2m]   = bias + W1 x[b, m] + W3 x[b, m-1]        x [B, t_in, 64] -> y [B, 2 t_in, c_out], c_out in {64,128}
 *                 y[b, 2m+1] = bias + W2 x[b, m] + W0 x[b, m+1]        (MaskedConvTranspose1d forward; data gradient of conv4s2)
 *   smt_conv4s2 : y[b, t]    = bias + sum_j Wj x[b, 2t + j - 1]        x [B, t_in, c_in], c_in in {64,128} -> y [B, t_in/2, 64]
 *                                                                      (MaskedConv1d forward; data gradient of convt4s2)
 * w_packed = smt_pack_weight layout [tap][c_out][c_in], swizzle 0; bias fp32 or NULL; x rows >= lens_in[b] read as zero,
 * y rows >= lens_out[b] are written as zero (either may be NULL); zero_page >= 256 zero bytes. */
int smt_convt4s2(const void* x, int64_t bs_x, int ld_x, const void* w_packed, const float* bias, void* y, int64_t bs_y,
                 int ld_y, const int* lens_in, const int* lens_out, int batch, int t_in, int c_out, const void* zero_page,
                 smt_stream_t stream);
int smt_conv4s2(const void* x, int64_t bs_x, int ld_x, const void* w_packed, const float* bias, void* y, int64_t bs_y,
                int ld_y, const int* lens_in, const int* lens_out, int batch, int t_in, int c_in, const void* zero_page,
                smt_stream_t stream);

/* K3 of all four branches of a GatedHiFiBlock + the tanh * softmax gate in one pass (bf16, width 64; resnet.py:224-237):
 *   z[b,t,128 d + c] = b3[d][c] + sum_i W3_d[c][i] u2[b,t,128 d + i]  +  b1[d][c] + sum_j W1_d[c][j] x[b,t,j]     d = 0..3
 *   g[b,t,c]         = sum_d tanh(z[.., 128 d + c]) * softmax_d(z[.., 128 d + 64 + c])                             c < 64
 * u2 / z are [B,t,512], x / g [B,t,64] with explicit pitches; x rows >= lens[b] read as zero (lens may be NULL).
 * w3_packed = the four [128][128] weights stacked, smt_pack_weight layout with swizzle = 1; w1_packed = the four [128][64]
 * weights stacked, swizzle 0; b3 / b1 [4][128] fp32.  g is bit-identical to smt_conv1d_ntc (folded K3) + smt_gate_mix_fwd. */
int smt_conv_k3gate_fwd(const void* u2, int64_t bs_u2, int ld_u2, const void* x, int64_t bs_x, int ld_x,
                        const void* w3_packed, const void* w1_packed, const float* b3, const float* b1, void* z,
                        int64_t bs_z, int ld_z, void* g, int64_t bs_g, int ld_g, const int* lens, int batch, int t,
                        const void* zero_page, smt_stream_t stream);

/* Fused backward of the 64 -> 64 1x1 gate convolution that closes a GatedHiFiBlock (bf16; resnet.py:238-241):
 * dx[t,ci] = keep(t) * sum_co dy[t,co] * W[co][ci] (keep = t < lens[b]), dweight[co*stride_out + ci*stride_in] =
 * sum_t dy[t,co] * g[t,ci] (g rows >= lens[b] read as 0), dbias[co] = sum_t dy[t,co].  dy / g / dx are [B,t,64] with
 * explicit pitches; w_packed_bwd = smt_pack_weight(..) layout [ci][co], swizzle 0; zero_page >= 256 zero bytes. */
size_t smt_conv_gate_bwd_workspace_bytes(int batch, int t);
int smt_conv_gate_bwd(const void* dy, int64_t bs_dy, int ld_dy, const void* g, int64_t bs_g, int ld_g,
                      const void* w_packed_bwd, void* dx, int64_t bs_dx, int ld_dx, const int* lens, int batch, int t,
                      const void* zero_page, float* dweight, int64_t stride_out, int64_t stride_in, float* dbias,
                      void* workspace, size_t workspace_bytes, smt_stream_t stream);

/* sum_d tanh(t_d) * softmax_d(s_d) over `depth` branches laid side by side along the channel axis
 * (z[.., d*2w + c] = t_d, z[.., d*2w + w + c] = s_d) -- GatedHiFiBlock.forward, resnet.py:229-237.  depth <= 8.  The
 * backward exchanges the softmax statistics between lanes when depth and width / (16 bytes) are powers of two whose
 * product divides 64, and holds all branches in one lane otherwise (three branches: VQTTS). */
int smt_gate_mix_fwd(const void* z, void* g, int dtype, int64_t rows, int width, int depth, int ld_z, int ld_g,
                     smt_stream_t stream);
int smt_gate_mix_bwd(const void* z, const void* dg, void* dz, int dtype, int64_t rows, int width, int depth,
                     int ld_z, int ld_g, int ld_dz, smt_stream_t stream);

/* The encoder's first convolution (C_in = 1; conv.py:61 with input_emb_width = 1): x fp32 [B, t_in],
 * weight fp32 [c_out][taps], y [B, t_out, c_out] in `dtype`; rows >= lens[b] of x read as 0. */
int smt_conv_in_fwd(const float* x, const float* weight, const float* bias, const int* lens, void* y, int dtype,
                    int batch, int t_in, int t_out, int c_out, int taps, int stride, int padding,
                    smt_stream_t stream);
size_t smt_conv_in_wgrad_workspace_bytes(int batch, int t_out, int c_out);
int smt_conv_in_wgrad(const float* x, const void* dy, const int* lens, float* dweight, float* dbias, int dtype,
                      int batch, int t_in, int t_out, int c_out, int taps, int stride, int padding, void* workspace,
                      size_t workspace_bytes, smt_stream_t stream);

/* The decoder's final 1x1 projection to one channel on masked rows (encdec.py:61,82):
 * y[b,t] = bias + sum_c x[b,t,c]*mask*w[c], y fp32 [B, t].  bwd writes dx (dtype) and fp32 dw/db. */
int smt_conv_out_fwd(const void* x, const float* weight, const float* bias, const int* lens, float* y, int dtype,
                     int batch, int t, int c_in, smt_stream_t stream);
size_t smt_conv_out_bwd_workspace_bytes(int batch, int t, int c_in);
int smt_conv_out_bwd(const void* x, const float* weight, const int* lens, const float* dy, void* dx, float* dweight,
                     float* dbias, int dtype, int batch, int t, int c_in, void* workspace, size_t workspace_bytes,
                     smt_stream_t stream);

/* -------------------------------------------------------- WaveNet block ---- */
/* The gate and the layer tail of WaveNetBlock (models/vqvae/resnet.py:170-181; additions under ABI 10).  z is [B, t, 2 hidden]:
 * the first `hidden` channels of a row are the tanh half, the last `hidden` the sigmoid half.  Every tensor has an explicit batch
 * stride bs_* and row pitch ld_*, both in elements; lens[b] is the valid length of item b (NULL: every row is valid).  A row at
 * or past lens[b] is WRITTEN as zero and NOT READ in any input.  One launch each, no atomics, no workspace, no host
 * synchronisation; equal inputs give equal bits; batch * t == 0 returns 0 without a launch (pointers may then be NULL).
 * Argument errors, all decided on the host before a launch and named by smt_last_error: hidden (a positive multiple of 8; 64
 * or 128 for the tail), dtype, null pointers, pointers not 16-byte aligned, a pitch smaller than the row width, a pitch or
 * batch stride that is not a multiple of 8 elements, batch * t >= 2^31, an output that overlaps an input.
 *
 *   smt_wavenet_gate_fwd:  a[b,t,c] = tanh(z[b,t,c]) * sigmoid(z[b,t,hidden + c])                         (resnet.py:176-177)
 *   smt_wavenet_gate_bwd:  dz[b,t,c]          = da * sigmoid(s) * (1 - tanh(t)^2)
 *                          dz[b,t,hidden + c] = da * tanh(t) * sigmoid(s) * (1 - sigmoid(s))
 * dtype SMT_F32 or SMT_BF16 (all tensors); arithmetic in fp32, a bf16 result is rounded once. */
int smt_wavenet_gate_fwd(const void* z, int64_t bs_z, int ld_z, void* a, int64_t bs_a, int ld_a, const int* lens, int batch,
                         int t, int hidden, int dtype, smt_stream_t stream);
int smt_wavenet_gate_bwd(const void* z, int64_t bs_z, int ld_z, const void* da, int64_t bs_da, int ld_da, void* dz,
                         int64_t bs_dz, int ld_dz, const int* lens, int batch, int t, int hidden, int dtype,
                         smt_stream_t stream);
/* One layer's tail in one pass (bf16, hidden 64 or 128; resnet.py:176-179):
 *   y[b,t,:] = keep(t) * ( x[b,t,:] + bias + W_g . (tanh(z_t) * sigmoid(z_s)) ),   keep = t < lens[b]
 * z [B,t,2 hidden], x / y [B,t,hidden]; w_packed = smt_pack_weight layout [1][c_out][c_in] of the 1x1 gate convolution with
 * swizzle = 0 (the kernel pads the rows itself when it stages them); bias fp32 [hidden] or NULL.  The gated value is formed in
 * fp32, rounded to bf16 once and fed to the matrix cores from registers: it is never stored.  fp32 accumulation, y rounded
 * once.  4 hidden elements of traffic per row, against 6 hidden for smt_wavenet_gate_fwd + smt_conv1d_ntc with a residual. */
int smt_wavenet_tail_fwd(const void* z, int64_t bs_z, int ld_z, const void* x, int64_t bs_x, int ld_x, const void* w_packed,
                         const float* bias, void* y, int64_t bs_y, int ld_y, const int* lens, int batch, int t, int hidden,
                         smt_stream_t stream);

/* ------------------------------------------------------------- spectral ---- */
/* Windowed STFT magnitude (STFT.forward, datasets/transforms.py:108-123): reflect padding
 * (n_fft - hop)/2, frame every `hop`, window[n_fft] (Hann centre-padded), bins 0..n_fft/2.
 *   x [batch, t] f32;  window [n_fft] f32;  twiddle [n_fft/2] complex f32 = exp(-2 pi i m / n_fft)
 *   mag [batch, n_fft/2+1, frames] f32, frames = smt_stft_num_frames(t, n_fft, hop)
 * n_fft in {256, 512, 1024, 2048}. */
int smt_stft_num_frames(int t, int n_fft, int hop);
int smt_stft_magnitude(const float* x, const float* window, const float* twiddle, float* mag, int batch, int t,
                       int n_fft, int hop, smt_stream_t stream);
/* Fused log-mel (MelSpectrogram.forward, transforms.py:61-65): mel [batch, n_mels, frames] =
 * log(max(mel_basis @ |STFT|, 1e-5)); band[2m], band[2m+1] = first / one-past-last non-zero bin of row m. */
int smt_melspec(const float* x, const float* window, const float* twiddle, const float* mel_basis, const int* band,
                float* mel, int batch, int t, int n_fft, int hop, int n_mels, smt_stream_t stream);
/* Log-mel of a ragged batch in one launch.  Item b is the clip x[b, :L_b], L_b = clamp(lens[b], 0, t) (lens int32 [batch] on
 * the device), transformed as smt_melspec transforms that clip alone: reflected about its own two ends, F_b =
 * smt_stft_num_frames(L_b) frames, or none if L_b <= pad or L_b + 2 pad < n_fft (pad = (n_fft - hop) / 2).  mel [batch,
 * n_mels, frames_out]: columns f < min(F_b, frames_out) hold the frames -- bit for bit what smt_melspec gives on the clip --
 * and every other column holds `fill`; each element is written exactly once and no x[b, i >= L_b] is read.  Errors: null
 * pointer, n_fft outside {256, 512, 1024, 2048}, hop outside [1, n_fft], n_mels < 1, t outside [1, 2^30], frames_out < 0,
 * batch outside [0, 65535].  batch == 0 or frames_out == 0 launches nothing.  No workspace, no atomics. */
int smt_melspec_ragged(const float* x, const int* lens, const float* window, const float* twiddle, const float* mel_basis,
                       const int* band, float* mel, int batch, int t, int n_fft, int hop, int n_mels, int frames_out, float fill,
                       smt_stream_t stream);
/* One resolution of MultiResolutionSpectralLoss (models/vqvae/losses.py:39-55) without materialising
 * the spectra.  fwd: partial [batch, frames, 2] = per-frame sums of ((|Y|-|Yh|) m)^2 and
 * ((log|Y| - log|Yh|) m)^2 (clamp 1e-5), m = frame mask from lens (losses.py:33-37).
 * bwd: dyh [batch, t] = adjoint of dL/dYh with coef [batch, 2] = upstream * 1/(2 B sqrt(S)) per term (written, not
 * accumulated).  The per-frame gradient rows go through `workspace` and are summed per sample in a fixed order: the result
 * is bit-reproducible (no floating-point atomics). */
int smt_stft_loss_fwd(const float* y, const float* yh, const int* lens, const float* window, const float* twiddle,
                      float* partial, int batch, int t, int n_fft, int hop, smt_stream_t stream);
size_t smt_stft_loss_bwd_workspace_bytes(int batch, int t, int n_fft, int hop);
int smt_stft_loss_bwd(const float* y, const float* yh, const int* lens, const float* window, const float* twiddle,
                      const float* coef, float* dyh, int batch, int t, int n_fft, int hop, void* workspace,
                      size_t workspace_bytes, smt_stream_t stream);

/* STFT.inverse (datasets/transforms.py:125-156): magnitude, phase [batch, n_fft/2+1, frames] ->
 * out [batch, (frames - 1) * hop + n_fft - 2 * ((n_fft - hop) / 2)]: inverse real FFT per frame, synthesis window,
 * overlap-add, division by the window sum-square where it exceeds float tiny, pad_amount trimmed on both sides.
 * window / twiddle as for smt_stft_magnitude. */
int smt_stft_inverse(const float* magnitude, const float* phase, const float* window, const float* twiddle, float* out,
                     int batch, int n_fft, int hop, int frames, smt_stream_t stream);

/* Mel magnitudes back to linear magnitudes (the inverse of smt_melspec's basis @ |STFT|): non-negative
 * least squares by multiplicative updates.  Per frame m = exp(mel) if log_input else mel, c_j = sum_k B[j,k]:
 *   num_k = sum_j B[j,k] m_j;  S_k = num_k / sum_j B[j,k] c_j where that is > 0, S_k = 0 for good on a bin no filter covers;
 *   n_iter times: r = B S;  S_k <- S_k num_k / max(sum_j B[j,k] r_j, 1e-30).
 * mel [batch, n_mels, frames] f32 -> mag [batch, n_fft/2+1, frames] f32; mel_basis / band as for smt_melspec; lens int32
 * [batch] on the device (frames per item, clamped to [0, frames]) or NULL for `frames` everywhere.  Columns f >= lens[b] are
 * written as exact zeros and mel is not read there.  One launch, no workspace, no atomics: equal inputs give equal bits.
 * Errors: null pointer, n_fft outside {256, 512, 1024, 2048}, n_mels outside [1, 1024], n_iter < 0, batch outside [0, 65535],
 * frames < 0.  batch == 0 or frames == 0 launches nothing. */
int smt_mel_invert(const float* mel, const int* lens, const float* mel_basis, const int* band, float* mag, int batch, int n_fft,
                   int n_mels, int frames, int n_iter, int log_input, smt_stream_t stream);

/* Fast Griffin-Lim, every iteration queued by this one call.  With alpha = momentum / (1 + momentum),
 * per item:  c = S e^{i phi0}, t = 0;  n_iter times: x = istft(c), R = stft(x), a = R - alpha t, t = R, c = S a / (|a| + 1e-16);
 * wave = istft(c).  istft is smt_stft_inverse on the item's own F_b = lens[b] frames (lens int32 [batch] on the device,
 * clamped to [0, frames], or NULL); stft is the complex spectrum of the item's own T_b = (F_b - 1) hop + n_fft - 2 pad samples,
 * reflected about its own two ends, so an item's waveform does not depend on the batch around it.
 *   mag [batch, n_fft/2+1, frames] f32;  exactly one of phase0 (same shape, radians) and seeds (int32 [batch] on the device):
 *   with seeds, phi0 = 2 pi u in fp32, u = ((bits >> 9) + 0.5) 2^-23, bits = fmix32(fmix32(fmix32(seed_b) + f 0x9E3779B1) +
 *   k 0x85EBCA77) -- a draw depends on (seed_b, f, k) only.  mag and phase0 are not read at f >= F_b.
 *   wave [batch, t_max] f32, t_max = (frames - 1) hop + n_fft - 2 pad: exact zeros at or past T_b; an item with F_b = 0, or too
 *   short to transform (T_b <= pad), is all zeros.
 * workspace (smt_griffin_lim_workspace_bytes): t [batch, frames, K] complex, S transposed [batch, frames, K], the windowed rows
 * [batch, frames, n_fft] and x [batch, t_max], all f32, each rounded up to 256 bytes.  Two launches per iteration, no
 * floating-point atomics: bit-reproducible.  Errors: null pointer, both or neither of phase0 / seeds, n_fft outside {256, 512,
 * 1024, 2048}, hop outside [1, n_fft], n_iter < 0, momentum outside [0, 1), batch outside [0, 65535], frames < 0, t_max above
 * 2^30, workspace too small.  batch == 0 or frames == 0 launches nothing. */
size_t smt_griffin_lim_workspace_bytes(int batch, int n_fft, int hop, int frames);
int smt_griffin_lim(const float* mag, const int* lens, const float* phase0, const int* seeds, const float* window,
                    const float* twiddle, float* wave, int batch, int n_fft, int hop, int frames, int n_iter, float momentum,
                    void* workspace, size_t workspace_bytes, smt_stream_t stream);

/* Test hook (no reference counterpart): the one-wave in-LDS transform of the spectral kernels alone on ONE complex frame.
 * in / out [n_fft][2] f32, twiddle as for smt_stft_magnitude; inverse != 0 uses the conjugate twiddles (no 1/N). */
int smt_fft_selftest(const float* in, const float* twiddle, float* out, int n_fft, int inverse, smt_stream_t stream);

/* ------------------------------------------------------- TransformerLM ---- */
/* The kernels between the dense projections of the causal TransformerLM over VQ codes
 * (models/transformer_lm/transformer_lm.py:32-135: nn.TransformerEncoder, post-norm layers, ReLU feed-forward).
 * Activations are batch-major rows [batch, len, dim] f32 (the reference runs them [len, batch, dim]; the layout is
 * internal to the model).  Every dropout site uses the counter-based generator above on the element's linear index
 * in the tensor being dropped; thresh16 = 0 disables it (eval).  Every entry takes the site key twice: `drop_key` by value
 * and `drop_key_dev`, a DEVICE pointer to one key that overrides it when non-NULL -- a captured hipGraph freezes by-value
 * arguments, so a graphed step keeps its keys in device memory and refreshes them with smt_lm_make_keys. */

/* keys_dev[s] = fmix32(seed_dev[0] * 0x9E3779B1 + s * 0x7F4A7C15 + 1), s < n_sites: the per-site keys of the step whose
 * seed is in device memory (the same derivation the host uses for `drop_key`). */
int smt_lm_make_keys(const uint32_t* seed_dev, uint32_t* keys_dev, int n_sites, smt_stream_t stream);

/* out = (emb[tokens] * mul + pe[position]) * keep   (transformer_lm.py:114-116, PositionalEncoding :27-29);
 * tokens [batch, len] int64, emb [vocab_rows, dim], pe [>= len, dim].  bwd: demb [vocab_rows, dim] is zeroed and
 * accumulated; row padding_idx receives nothing (nn.Embedding(padding_idx=PAD), :42-46). */
int smt_lm_embed_fwd(const int64_t* tokens, const float* emb, const float* pe, float* out, int batch, int len, int dim,
                     float mul, uint32_t drop_key, const uint32_t* drop_key_dev, uint32_t drop_thresh16, float drop_scale, smt_stream_t stream);
int smt_lm_embed_bwd(const int64_t* tokens, const float* dout, float* demb, int batch, int len, int dim, int vocab_rows,
                     float mul, uint32_t drop_key, const uint32_t* drop_key_dev, uint32_t drop_thresh16, float drop_scale, int64_t padding_idx,
                     smt_stream_t stream);

/* Multi-head self-attention core of nn.MultiheadAttention as the reference calls it (:110-111,117: additive causal
 * mask triu(-inf, 1) plus the key-padding mask ~sequence_mask(lens)): head dim 32, len * 3 * heads * 32 < 2^31.
 *   qkv [batch, len, 3*heads*32] = (q | k | v) rows as in_proj produces them;  lens [batch] int32 or NULL
 *   ctx [batch, len, heads*32] = dropout(softmax(q k^T / sqrt(32) + masks)) v;   lse [batch, heads, len]: scratch between
 *   the forward and the backward call (log2 of the sum of 2^(score * log2 e): the kernels work in base 2)
 * key j is visible to query i iff (j <= i or causal == 0) and j < lens[b] -- causal = 0 is what `sample` runs
 * (mask=None, :142); dropout index ((b*heads + h)*len + i)*len + j.
 * bwd writes dqkv [batch, len, 3*heads*32] (every element); delta [batch, heads, len] is scratch it fills and reads. */
int smt_lm_attention_fwd(const float* qkv, const int* lens, float* ctx, float* lse, int batch, int len, int heads,
                         int causal, uint32_t drop_key, const uint32_t* drop_key_dev, uint32_t drop_thresh16, float drop_scale, smt_stream_t stream);
int smt_lm_attention_bwd(const float* qkv, const int* lens, const float* ctx, const float* lse, const float* dctx,
                         float* dqkv, float* delta, int batch, int len, int heads, int causal, uint32_t drop_key,
                         const uint32_t* drop_key_dev, uint32_t drop_thresh16, float drop_scale, smt_stream_t stream);

/* The same two calls with the five (forward: two) 32-channel products on v_mfma_f32_32x32x16_bf16 (model.attention_dtype:
 * bf16).  Tensors, layouts, limits, argument checks, workgroup ownership, merge order, dropout indices and keys are those
 * of the f32 entries above; every tensor stays f32 in memory.  The arithmetic has exactly these rounding points:
 *   operands   q, k, v and dctx are rounded to bf16 (nearest even, v_cvt_pk_bf16_f32) as loaded, unscaled: 1/sqrt(32) and
 *              log2(e) multiply the f32 score accumulator, so a bf16-representable input is used exactly
 *   forward    s = q^ . k^ accumulated in f32;  the running max m, the sum z of the UNROUNDED p = exp2(s - m) and lse are
 *              f32;  the second product's operand is bf16(p * keep * drop_scale), one rounding;  ctx accumulates in f32,
 *              takes the f32 rescale and 1/z, and is stored f32
 *   dq kernel  delta = dctx . ctx in f32 from the unrounded values;  dP = dctx^ . v^;
 *              dS = p (keep * drop_scale * dP - delta) in f32, rounded once to bf16;  dq = (dS^ . k^) / sqrt(32)
 *   dkv kernel dv = bf16(p * keep * drop_scale)^T . dctx^;  dk = (dS^^T . q^) / sqrt(32)
 * (x^ = x rounded to bf16; in the backward p = exp2(s - lse), the normalised weight). */
int smt_lm_attention_bf16_fwd(const float* qkv, const int* lens, float* ctx, float* lse, int batch, int len, int heads,
                              int causal, uint32_t drop_key, const uint32_t* drop_key_dev, uint32_t drop_thresh16, float drop_scale,
                              smt_stream_t stream);
int smt_lm_attention_bf16_bwd(const float* qkv, const int* lens, const float* ctx, const float* lse, const float* dctx,
                              float* dqkv, float* delta, int batch, int len, int heads, int causal, uint32_t drop_key,
                              const uint32_t* drop_key_dev, uint32_t drop_thresh16, float drop_scale, smt_stream_t stream);

/* The attention core at head dim 32 or 64 (the reference's `nhead` with d_model / nhead = 64): the arguments of
 * smt_lm_attention_fwd / _bwd, then head_dim and bf16 (0: the f32 products, non-zero: the bf16 products above).  Every
 * "32" of the two descriptions above reads head_dim: qkv [batch, len, 3*heads*head_dim], head h at channel h*head_dim of
 * each third, ctx [batch, len, heads*head_dim], scale 1/sqrt(head_dim), len * 3 * heads * head_dim < 2^31.  Masks,
 * dropout indices and keys, lse, delta and the rounding points of the bf16 form do not depend on the head dim.
 * head_dim = 32 is exactly the launches of the four entries above (which are calls of these two); any head_dim other than
 * 32 or 64 is an argument error, with no launch. */
int smt_lm_attention_hd_fwd(const float* qkv, const int* lens, float* ctx, float* lse, int batch, int len, int heads,
                            int causal, uint32_t drop_key, const uint32_t* drop_key_dev, uint32_t drop_thresh16, float drop_scale,
                            int head_dim, int bf16, smt_stream_t stream);
int smt_lm_attention_hd_bwd(const float* qkv, const int* lens, const float* ctx, const float* lse, const float* dctx,
                            float* dqkv, float* delta, int batch, int len, int heads, int causal, uint32_t drop_key,
                            const uint32_t* drop_key_dev, uint32_t drop_thresh16, float drop_scale, int head_dim, int bf16,
                            smt_stream_t stream);

/* y = LayerNorm(x + dropout(h + h_bias)) * gamma + beta over the last dim (TransformerEncoderLayer, norm_first = False):
 * h is the bias-free output of out_proj / linear2 and h_bias [dim] that projection's bias (NULL = none), so that the
 * bias gradient falls out of this kernel's backward instead of a separate reduction; with h = NULL the plain final
 * LayerNorm of the encoder (:63-66).  stats [rows, 2] = (mean, rstd).  dim = 64 * {1,2,4,8,12,16,32}.
 * bwd: dx / dh may be NULL (not wanted); dparams [3, dim] = dgamma, dbeta, dh_bias (column sums of dh). */
int smt_lm_add_ln_fwd(const float* x, const float* h, const float* h_bias, const float* gamma, const float* beta, float* y,
                      float* stats, int64_t rows, int dim, float eps, uint32_t drop_key, const uint32_t* drop_key_dev, uint32_t drop_thresh16,
                      float drop_scale, smt_stream_t stream);
size_t smt_lm_add_ln_bwd_workspace_bytes(int64_t rows, int dim);
int smt_lm_add_ln_bwd(const float* x, const float* h, const float* h_bias, const float* dy, const float* gamma,
                      const float* stats, float* dx, float* dh, float* dparams, int64_t rows, int dim, uint32_t drop_key,
                      const uint32_t* drop_key_dev, uint32_t drop_thresh16, float drop_scale, void* workspace,
                      size_t workspace_bytes, smt_stream_t stream);

/* The residual step of a pre-norm stack (TransformerEncoderLayer, norm_first = True), where every residual add is followed
 * by a LayerNorm -- the same layer's norm2, the next layer's norm1 or the encoder's final norm:
 *   s = x + dropout(h + h_bias)              the new residual stream [rows, dim], stored
 *   y = LayerNorm(s) * gamma + beta          the input of the next projection;  stats [rows, 2] = (mean, rstd) of s
 * x and h are both required; h_bias, the dropout index, the key pair and the dim set 64 * {1,2,3,4,8,12,16,32} are those of
 * smt_lm_add_ln_*.  s and y alias neither an input nor each other.
 * bwd takes two incoming gradients, either NULL (= zero): ds of the stream (from everything downstream of it) and dy of the
 * normed output.  With xhat = (s - mean) * rstd recomputed from the stored s (neither x nor h is read) and g = dy * gamma:
 *   dpre = ds + rstd * (g - mean(g) - xhat * mean(g * xhat));   dx = dpre;   dh = dpre * keep      (dx / dh may be NULL)
 *   dparams [3, dim] = dgamma, dbeta, dh_bias (column sums of dh): per-workgroup partials merged in a fixed order, no float
 *   atomics -- equal inputs give equal bits.
 * rows = 0: no launch, bwd zeroes dparams.  A dim outside the built set is an argument error named by smt_last_error. */
int smt_lm_res_ln_fwd(const float* x, const float* h, const float* h_bias, const float* gamma, const float* beta, float* s,
                      float* y, float* stats, int64_t rows, int dim, float eps, uint32_t drop_key, const uint32_t* drop_key_dev,
                      uint32_t drop_thresh16, float drop_scale, smt_stream_t stream);
size_t smt_lm_res_ln_bwd_workspace_bytes(int64_t rows, int dim);
int smt_lm_res_ln_bwd(const float* s, const float* ds, const float* dy, const float* gamma, const float* stats, float* dx,
                      float* dh, float* dparams, int64_t rows, int dim, uint32_t drop_key, const uint32_t* drop_key_dev,
                      uint32_t drop_thresh16, float drop_scale, void* workspace, size_t workspace_bytes, smt_stream_t stream);

/* a = dropout(gelu(h + bias)), gelu(u) = 0.5 u (1 + erf(u / sqrt 2)): the exact form (activation = "gelu"), not the tanh
 * approximation.  Not in place (a != h): h, the bias-free output of linear1, is kept for the backward, which recomputes
 * u = h + bias and gives dh = da * keep * (Phi(u) + u phi(u)) (dh aliases neither h nor da) and dbias [dim] = its column
 * sums in a fixed order.  Element index, key pair and rows = 0 behaviour as smt_lm_bias_relu_*. */
int smt_lm_bias_gelu_fwd(const float* h, const float* bias, float* a, int64_t rows, int dim, uint32_t drop_key,
                         const uint32_t* drop_key_dev, uint32_t drop_thresh16, float drop_scale, smt_stream_t stream);
size_t smt_lm_bias_gelu_bwd_workspace_bytes(int64_t rows, int dim);
int smt_lm_bias_gelu_bwd(const float* h, const float* bias, const float* da, float* dh, float* dbias, int64_t rows, int dim,
                         uint32_t drop_key, const uint32_t* drop_key_dev, uint32_t drop_thresh16, float drop_scale, void* workspace,
                         size_t workspace_bytes, smt_stream_t stream);

/* h <- dropout(relu(h + bias)) in place (linear1 -> activation -> dropout of the feed-forward).  bwd: dh = da * keep *
 * [a != 0] (a = the forward's result; dh may alias da), dbias [dim] = its column sums in a fixed order. */
int smt_lm_bias_relu_fwd(float* h, const float* bias, int64_t rows, int dim, uint32_t drop_key, const uint32_t* drop_key_dev, uint32_t drop_thresh16,
                         float drop_scale, smt_stream_t stream);
size_t smt_lm_bias_relu_bwd_workspace_bytes(int64_t rows, int dim);
int smt_lm_bias_relu_bwd(const float* a, const float* da, float* dh, float* dbias, int64_t rows, int dim, uint32_t drop_key,
                         const uint32_t* drop_key_dev, uint32_t drop_thresh16, float drop_scale, void* workspace,
                         size_t workspace_bytes, smt_stream_t stream);

/* Next-token cross entropy and accuracy (:121-128).  target [rows] int64, < 0 = row not counted (the reference's
 * loss_mask); row_out [rows, 2] = (logsumexp - logit[target] or 0, argmax == target as 0/1, lowest index on ties);
 * lse [rows].  bwd: dlogits = coef[0] * (softmax - onehot) on counted rows, 0 elsewhere; coef is a DEVICE scalar
 * (upstream gradient / number of counted rows). */
int smt_lm_ce_fwd(const float* logits, const int64_t* target, float* row_out, float* lse, int64_t rows, int vocab,
                  smt_stream_t stream);
int smt_lm_ce_bwd(const float* logits, const int64_t* target, const float* lse, const float* coef, float* dlogits,
                  int64_t rows, int vocab, smt_stream_t stream);

/* The other two training losses of the TransformerLM (loss_type focal | mmi, reference models/transformer_lm/losses.py), with
 * the conventions of smt_lm_ce_*: logits [rows, vocab] fp32; target [rows] int64, < 0 = row not scored, a scored target is
 * < vocab (the caller's guarantee); lse [rows]; coef a DEVICE scalar (upstream gradient / number of scored rows).  Nothing
 * synchronises with the host and there are no float atomics: every cross-row sum is merged in a fixed order, so equal
 * inputs give equal bits.  rows = 0 returns 0 and launches nothing; rows < 0, vocab < 1 and a gamma outside the built set
 * are argument errors, returned before any HIP call.  On unscored rows dlogits is exactly 0.
 *
 * Focal, (1 - p_t)^gamma * CE (FocalLoss without class weights), per scored row r with s = logit[r, t_r] - lse[r] = log p_t,
 * p_t = exp(s), q = -expm1(s) (not 1 - exp(s): no cancellation as p_t -> 1):
 *   l_r = -q^gamma s,   c_r = dl_r/ds = gamma q^(gamma-1) p_t s - q^gamma   (gamma = 0: c_r = -1, the cross entropy)
 *   fwd: row_out [rows, 2] = (l_r or 0, argmax == target as 0/1, lowest index on ties), lse, row_coef [rows] = c_r (0 on
 *        unscored rows): the powers are taken once per row here, the backward has none
 *   bwd: dlogits[r, v] = coef[0] * c_r * ([v = t_r] - p_v),  p_v = exp(logit[r, v] - lse[r])
 * gamma = 0 or gamma >= 1, finite; 0 < gamma < 1 (an unbounded derivative at q = 0) is not built. */
int smt_lm_focal_fwd(const float* logits, const int64_t* target, float* row_out, float* lse, float* row_coef, int64_t rows,
                     int vocab, float gamma, smt_stream_t stream);
int smt_lm_focal_bwd(const float* logits, const int64_t* target, const float* lse, const float* row_coef, const float* coef,
                     float* dlogits, int64_t rows, int vocab, smt_stream_t stream);

/* Maximum mutual information (MaximumMutualInformationLoss in its collapsed form), n = count[0] scored rows (a DEVICE float),
 * p_rv = exp(logit[r, v] - lse[r]) on scored rows, m_v = (1/n) sum_r p_rv (two-stage column sums in a fixed order),
 * logm_v = log m_v and 0 where m_v = 0 (every p_rv is 0 there, so the value is never weighed):
 *   loss = log(e + vocab - 1) - (1/n) sum_r p_{r,t_r} + sum_v m_v logm_v
 *   fwd: row_out [rows, 2] = (p_{r,t_r} or 0, correct 0/1), lse, logm [vocab] (kept for bwd), ent [1] = sum_v m_v logm_v;
 *        the constant and the row mean are the caller's.  No scored row: ent is nan.
 *   bwd: dlogits[r, v] = coef[0] * p_rv * (logm_v - [v = t_r] - E_r + p_{r,t_r}),  E_r = sum_v p_rv logm_v  (the exact
 *        gradient: the +1 of d(m log m)/dm cancels against its own row mean)
 * The marginal m is formed over the rows of THIS call: under data parallelism every rank uses the marginal of its own rows,
 * as the reference does under DDP (its loss sees the local batch only).
 * workspace: smt_lm_mmi_workspace_bytes (column-sum partials per block of 16 rows, and the merged sums). */
size_t smt_lm_mmi_workspace_bytes(int64_t rows, int vocab);
int smt_lm_mmi_fwd(const float* logits, const int64_t* target, const float* count, float* row_out, float* lse, float* logm,
                   float* ent, int64_t rows, int vocab, void* workspace, size_t workspace_bytes, smt_stream_t stream);
int smt_lm_mmi_bwd(const float* logits, const int64_t* target, const float* lse, const float* logm, const float* coef,
                   float* dlogits, int64_t rows, int vocab, smt_stream_t stream);

/* The dense projections with bf16 operands (model.compute_dtype: bf16; csrc/lm_linear.hip).  Activations, gradients and the
 * bias stay fp32 in memory: x / dy are rounded to bf16 (round to nearest even, what tensor.to(torch.bfloat16) gives on finite
 * values) as they are loaded, products accumulate in fp32 on the bf16 MFMA, results are stored as fp32.
 *   fwd    y[r, o]  = bias[o] + sum_i bf16(x[r, i]) * w[o][i]                 bias fp32 [n_out] or NULL, added in fp32
 *   dgrad  dx[r, i] = sum_o bf16(dy[r, o]) * w[o][i]
 *   wgrad  dweight[o * n_in + i] = sum_r bf16(dy[r, o]) * bf16(x[r, i]);  dbias[o] = sum_r dy[r, o] in fp32 from the UNROUNDED
 *          dy (NULL = not wanted)
 * w_packed = smt_pack_weight(dtype SMT_BF16, one tap, swizzle 0) of the weight as [n_out][n_in]; w_packed_t = the same weight
 * packed [n_in][n_out] (the pack's n_out / n_in and strides swapped).
 * Shapes: n_in a positive multiple of 32, n_out a positive multiple of 16, rows >= 0 arbitrary (rows beyond `rows` are
 * neither read nor written; columns outside a row's width are neither read nor written).  x / y / dy / dx are rows with an
 * explicit pitch in elements (>= the width, a multiple of 4); dweight [n_out][n_in] and dbias [n_out] are dense.  Every
 * pointer is 16-byte aligned (bias: 4).  Row offsets are formed in 64 bits: rows * pitch may exceed 2^31.
 * Argument errors (a dimension off these rules, a negative rows, a null or misaligned pointer, a pitch below the width or
 * off the multiple, an output that overlaps an input, a workspace below the queried size) return 1 before any HIP call and
 * are named by smt_last_error.  rows = 0 returns 0 without a launch; wgrad then zeroes dweight and dbias (the sum over nothing).
 * No allocation, no host synchronisation, no atomics: wgrad splits the rows over several workgroups per output tile, each
 * writes a slab into `workspace`, and a second launch adds the slabs in slab order, so equal inputs give equal bits. */
int smt_lm_linear_fwd(const float* x, int64_t ld_x, const void* w_packed, const float* bias, float* y, int64_t ld_y,
                      int64_t rows, int n_in, int n_out, smt_stream_t stream);
int smt_lm_linear_dgrad(const float* dy, int64_t ld_dy, const void* w_packed_t, float* dx, int64_t ld_dx, int64_t rows,
                        int n_in, int n_out, smt_stream_t stream);
size_t smt_lm_linear_wgrad_workspace_bytes(int64_t rows, int n_in, int n_out);
int smt_lm_linear_wgrad(const float* x, int64_t ld_x, const float* dy, int64_t ld_dy, float* dweight, float* dbias,
                        int64_t rows, int n_in, int n_out, void* workspace, size_t workspace_bytes, smt_stream_t stream);

/* Incremental decoding (TransformerLM.sample(causal=True)): one new token per step against a key/value cache.  fp32, eval
 * mode (no dropout), head dim 32 (the _hd entries: 32 or 64), batch 1..32.  What changes from step to step -- the position, the tokens, the uniforms --
 * lives in device memory, so a step is a fixed sequence of launches with fixed arguments.  Like the dropout keys above,
 * the position comes twice: `pos` by value and `pos_dev`, a DEVICE pointer that overrides it when non-NULL.  A by-value
 * position outside the buffers is an argument error; with a device position the kernels return without touching memory.
 * Every sum is merged in a fixed order (no float atomics): equal inputs give equal bits. */

/* out[b, :] = emb[tokens[b, pos]] * mul + pe[pos];  tokens [batch, tok_len] int64, emb [vocab_rows, dim], pe [pe_rows, dim],
 * out [batch, dim].  A token outside [0, vocab_rows) gives a NaN row. */
int smt_lm_decode_embed(const int64_t* tokens, const float* emb, const float* pe, float* out, int batch, int tok_len, int dim,
                        int vocab_rows, int pe_rows, float mul, int pos, const int* pos_dev, smt_stream_t stream);

/* out [batch, out_dim] = act(x [batch, in_dim] . w [out_dim, in_dim]^T (+ bias [out_dim] if non-NULL)), act: 0 none, 1 ReLU,
 * 2 exact GELU (0.5 u (1 + erf(u / sqrt 2))); any other value is an argument error.  The weight matrix (an nn.Linear weight
 * as is) is streamed once.  in_dim % 64 == 0, out_dim >= 1; fp32 products and sums. */
int smt_lm_decode_linear(const float* x, const float* w, const float* bias, float* out, int batch, int in_dim, int out_dim, int act,
                         smt_stream_t stream);

/* One layer's attention for the token at `pos`: qkv [batch, 3*heads*32] (q | k | v as in_proj produces them); the k and v
 * rows are stored to cache row pos (k_cache, v_cache [batch, heads, l_max, 32]) and
 * ctx [batch, heads*32] = softmax(q . K[0..pos]^T / sqrt(32)) . V[0..pos].  Cache rows beyond pos are never read.
 * workspace: smt_lm_decode_attention_workspace_bytes (partial softmaxes of the 256-row chunks; 0 when l_max <= 256). */
size_t smt_lm_decode_attention_workspace_bytes(int batch, int heads, int l_max);
int smt_lm_decode_attention(const float* qkv, float* k_cache, float* v_cache, float* ctx, void* workspace, size_t workspace_bytes,
                            int batch, int heads, int l_max, int pos, const int* pos_dev, smt_stream_t stream);

/* The same at head dim 32 or 64: qkv [batch, 3*heads*head_dim], caches [batch, heads, l_max, head_dim], ctx
 * [batch, heads*head_dim], scale 1/sqrt(head_dim); the workspace holds 4 + head_dim floats per (batch, head, chunk), so its
 * size depends on the head dim.  pos / pos_dev as above.  head_dim = 32 is the entry above; any other value than 32 or 64
 * is an argument error (and a workspace size of 0). */
size_t smt_lm_decode_attention_hd_workspace_bytes(int batch, int heads, int l_max, int head_dim);
int smt_lm_decode_attention_hd(const float* qkv, float* k_cache, float* v_cache, float* ctx, void* workspace, size_t workspace_bytes,
                               int batch, int heads, int l_max, int head_dim, int pos, const int* pos_dev, smt_stream_t stream);

/* Rotary positions (model.position: rotary; csrc/lm_rope.hip).  Head dim dh = 32 or 64.  Pair i in [0, dh/2) is
 * channels (2i, 2i+1) of a head -- interleaved, so that a pair never crosses the 4 consecutive channels a lane of the decode
 * attention owns -- in the q and k thirds of qkv [batch, len, 3*heads*dh]; v is untouched.  With theta_i = base^(-2i/dh),
 * absolute position p and a = p * theta_i:
 *     y[2i]   = x[2i] * cos a - x[2i+1] * sin a
 *     y[2i+1] = x[2i] * sin a + x[2i+1] * cos a            (inverse: sin negated)
 * cos a and sin a are read from the table rope [rope_rows, dh/2, 2] fp32 = (cos a, sin a), which the host computes in float64
 * (theta_i = pow(base, -2i/dh), a = p * theta_i, both float64) and rounds once (smt_amd.lm.rope_table); the kernels call no
 * transcendental, and equal inputs give equal bits.  Rounding: y = fma(x0, c, -(x1 * s)) resp. fma(x0, s, x1 * c), so
 * |y - y64| <= 4 * 2^-24 * (|x[2i]| + |x[2i+1]|) against float64 with float64 angles.  The gradient of the rotation is the
 * inverse rotation of the incoming gradient: inverse != 0 is the backward.
 *
 * In place on the q and k thirds of every row; row l uses table row pos0 + l; the v third is neither read nor written.  One
 * launch, 16-byte accesses (qkv and rope 16-byte aligned), no atomics, no workspace; batch * len = 0 returns 0 without a
 * launch.  Argument errors: null pointers, a head dim other than 32 or 64, pos0 < 0 or pos0 + len > rope_rows ("outside the
 * rope table"), len * 3 * heads * head_dim >= 2^31. */
int smt_lm_rope(float* qkv, const float* rope, int batch, int len, int heads, int head_dim, int rope_rows, int pos0, int inverse,
                smt_stream_t stream);

/* smt_lm_decode_attention_hd with rotary positions, in the same launches: the step's q and its own k row are rotated at
 * position pos (table row pos of rope [rope_rows, head_dim/2, 2]) as they are loaded from qkv, before the scale and before the
 * store to cache row pos.  The cache therefore holds rotated keys, cached rows are used as read, qkv is not modified; v is
 * untouched.  Workspace: that of the _hd entry.  rope == NULL is exactly the _hd launch (rope_rows is then ignored).  A
 * by-value pos >= rope_rows is an argument error; a *pos_dev outside the table or the cache makes the launch write nothing. */
int smt_lm_decode_attention_rope(const float* qkv, float* k_cache, float* v_cache, float* ctx, void* workspace, size_t workspace_bytes,
                                 int batch, int heads, int l_max, int head_dim, const float* rope, int rope_rows, int pos,
                                 const int* pos_dev, smt_stream_t stream);

/* Inverse-CDF draw: p_i = exp((logits[b, i] - max_i) * inv_sigma), S = sum p_i, k = the smallest index whose cumulative sum
 * exceeds uniforms[pos, b] * S (if rounding leaves none: the last k with p_k > 0).  logits [batch, vocab], uniforms
 * [n_steps, batch] in [0, 1); writes tokens[b, pos + 1] = k + token_offset (tokens [batch, tok_len] int64) and
 * codes[b, pos] = k (codes [batch, n_steps] int64). */
int smt_lm_decode_sample(const float* logits, const float* uniforms, int64_t* tokens, int64_t* codes, int batch, int vocab,
                         int tok_len, int n_steps, float inv_sigma, int token_offset, int pos, const int* pos_dev, smt_stream_t stream);

/* The same draw over a kept set, the first n codes of the order pi (logit descending, then code index ascending), with
 * w_i = exp((logits[b, i] - max_i) * inv_sigma):
 *   candidates  top_k > 0: the first K = min(top_k, vocab) codes of pi; top_k = 0: all.  W = their total weight.
 *   kept        top_p < 1: the smallest n >= 1 whose first-n weight is >= top_p * W (so top-p acts on the distribution
 *               renormalised over the candidates); top_p = 1: n = the number of candidates.  Equal logits at the cut are
 *               taken lowest index first.  kept (NULL or [n_steps, batch] int32) gets n at row pos.
 *   draw        as smt_lm_decode_sample over the kept codes in code-index order (the others have weight 0 and are never drawn); with top_k = 0
 *               and top_p = 1 the codes are bit-identical to smt_lm_decode_sample.
 * top_k >= 0, 0 < top_p <= 1, vocab <= 4096 (keys and weights of a row sit in 32 KiB of LDS). */
int smt_lm_decode_sample_filtered(const float* logits, const float* uniforms, int64_t* tokens, int64_t* codes, int batch, int vocab,
                                  int tok_len, int n_steps, float inv_sigma, int token_offset, int top_k, float top_p,
                                  int32_t* kept, int pos, const int* pos_dev, smt_stream_t stream);

/* Keys / values of a whole prompt: qkv [batch, len, 3*heads*32] (the batched in-projection, batch-major; 16-byte aligned)
 * -> its k and v thirds into rows 0..len-1 of k_cache / v_cache [batch, heads, l_max, 32]; rows >= len are not touched.
 * 1 <= len <= l_max; batch, heads and l_max bounded as in smt_lm_decode_attention. */
int smt_lm_decode_prefill_kv(const float* qkv, float* k_cache, float* v_cache, int batch, int len, int heads, int l_max,
                             smt_stream_t stream);

/* The same at head dim 32 or 64 (qkv [batch, len, 3*heads*head_dim], caches [batch, heads, l_max, head_dim]). */
int smt_lm_decode_prefill_kv_hd(const float* qkv, float* k_cache, float* v_cache, int batch, int len, int heads, int l_max,
                                int head_dim, smt_stream_t stream);

/* pos_dev[0] += 1: the last launch of a step. */
int smt_lm_decode_advance(int* pos_dev, smt_stream_t stream);

/* ------------------------------------------------------- GlowTTS ---- */
/* SURVEY 8(f4) / BASELINE.json configs[4]: the pieces of the reference's GlowTTS (models/glow_tts/glow_tts.py:59-130,
 * modules.py:134-236, submodules.py:88-512) that are not convolutions; fp32, channels-last rows [batch, t, channels] with
 * prefix row masks (lens[batch], NULL = no mask).  Row reductions are two-stage in a fixed order (reproducible).
 * Workspaces for the column reductions: smt_glow_reduce_workspace_bytes(rows, columns). */
size_t smt_glow_reduce_workspace_bytes(int64_t rows, int cols);
/* ActNorm (submodules.py:237-253): z = (bias + exp(logs) x) mask; reverse: (x - bias) exp(-logs) mask.  bwd: dx (may be NULL),
 * dlogs[c] = sum dz x exp(logs) mask, dbias[c] = sum dz mask; workspace columns = 2 * channels. */
int smt_glow_actnorm_fwd(const float* x, const float* logs, const float* bias, const int* lens, float* z, int batch, int t,
                         int channels, int reverse, smt_stream_t stream);
int smt_glow_actnorm_bwd(const float* x, const float* dz, const float* logs, const int* lens, float* dx, float* dlogs,
                         float* dbias, int batch, int t, int channels, void* workspace, size_t workspace_bytes,
                         smt_stream_t stream);
/* InvConvNear (submodules.py:292-323), n_split = 4: the 4 x 4 weight mixes the channel quadruples (h C/2 + 2 j + k);
 * transpose = 1 applies weight^T (the data gradient).  wgrad: dweight[s'][s] = sum dz[s'] x[s] over rows and groups
 * (workspace columns = 16). */
int smt_glow_invconv(const float* x, const float* weight, const int* lens, float* z, int batch, int t, int channels,
                     int transpose, smt_stream_t stream);
int smt_glow_invconv_wgrad(const float* x, const float* dz, const int* lens, float* dweight, int batch, int t, int channels,
                           void* workspace, size_t workspace_bytes, smt_stream_t stream);
/* WN gate (submodules.py:88-95 fused_add_tanh_sigmoid_multiply after the in_layer's dropout, :213-220):
 * acts[r, c] = tanh(d(a[r, c])) sigmoid(d(a[r, hidden + c])), d = counter dropout over the linear index of a [rows, 2 hidden]. */
int smt_glow_gate_fwd(const float* a, float* acts, int64_t rows, int hidden, uint32_t drop_key, const uint32_t* drop_key_dev,
                      uint32_t drop_thresh16, float drop_scale, smt_stream_t stream);
int smt_glow_gate_bwd(const float* a, const float* dacts, float* da, int64_t rows, int hidden, uint32_t drop_key,
                      const uint32_t* drop_key_dev, uint32_t drop_thresh16, float drop_scale, smt_stream_t stream);
/* WN gate with a speaker condition (WN.forward with g, submodules.py:212-224): a [batch, t, 2 hidden], one vector per item
 * cond[b * cond_stride + 0 .. 2 hidden) added AFTER the dropout of a:
 *   acts[b, t, c] = tanh(d(a[b, t, c]) + cond[b, c]) sigmoid(d(a[b, t, hidden + c]) + cond[b, hidden + c]),
 * d and its counter as in smt_glow_gate_fwd; cond = 0 gives that function's result bit for bit.
 * bwd: one pass writes da (every row) and per-item partial sums, a second launch adds them in a fixed order (no float
 * atomics, bitwise reproducible): dcond[b * dcond_stride + 0 .. 2 hidden) = the sum over the rows t < lens[b] (NULL: all) of
 * the gate's derivative by its argument, without the dropout factor.  cond and dcond are two tensors with two layouts: each
 * pointer has its own item stride, in floats, and both strides must be >= 2 hidden.
 * workspace >= smt_glow_gate_cond_workspace_bytes(batch, t, 2 hidden) = batch * ceil(t / 64) * cols floats. */
size_t smt_glow_gate_cond_workspace_bytes(int batch, int t, int cols);
int smt_glow_gate_cond_fwd(const float* a, const float* cond, int64_t cond_stride, float* acts, int batch, int t, int hidden,
                           uint32_t drop_key, const uint32_t* drop_key_dev, uint32_t drop_thresh16, float drop_scale,
                           smt_stream_t stream);
int smt_glow_gate_cond_bwd(const float* a, const float* dacts, const float* cond, int64_t cond_stride, const int* lens, float* da,
                           float* dcond, int64_t dcond_stride, int batch, int t, int hidden, uint32_t drop_key,
                           const uint32_t* drop_key_dev, uint32_t drop_thresh16, float drop_scale, void* workspace,
                           size_t workspace_bytes, smt_stream_t stream);
/* The duration predictor's input with a speaker (TextEncoder.forward, modules.py:117-129): out [batch, t, width],
 * out[b, t, :] = (x[b, t, 0 .. hidden) | g[b * g_stride + 0 .. gin) | zeros) on the rows t < lens[b] (NULL: all), zero rows
 * after; width >= hidden + gin (the next channel count the convolution takes), g_stride >= gin.
 * item_colsum, its gradient by g (x enters detached): dg[b * dg_stride + j] = sum over t < lens[b] of
 * dout[b, t, col0 + j], j < ncol, rows of width floats, two-stage in a fixed order;
 * workspace >= smt_glow_gate_cond_workspace_bytes(batch, t, ncol). */
int smt_glow_bcast_concat(const float* x, const float* g, int64_t g_stride, const int* lens, float* out, int batch, int t, int hidden,
                          int gin, int width, smt_stream_t stream);
int smt_glow_item_colsum(const float* dout, const int* lens, float* dg, int64_t dg_stride, int batch, int t, int width, int col0,
                         int ncol, void* workspace, size_t workspace_bytes, smt_stream_t stream);
/* Plain dropout over the linear element index: y[i] = x[i] keep(i) (DurationPredictor, submodules.py:629-633). */
int smt_glow_dropout(const float* x, float* y, int64_t n, uint32_t drop_key, const uint32_t* drop_key_dev, uint32_t drop_thresh16,
                     float drop_scale, smt_stream_t stream);
/* Affine coupling (submodules.py:383-405): out = (m | logs) from the `end` convolution, x = (x0 | x1):
 * z = (x0 | (m + exp(logs) x1) mask), logdet[b] = sum logs mask (NULL: not wanted; workspace >= batch * ceil(t / 64) floats);
 * reverse: z1 = (x1 - m) exp(-logs) mask.  bwd: dout = (dm | dlogs), dx = (dz0 | dz1 exp(logs) mask). */
int smt_glow_coupling_fwd(const float* out, const float* x, const int* lens, float* z, float* logdet, int batch, int t,
                          int channels, int sigmoid_scale, int reverse, void* workspace, size_t workspace_bytes,
                          smt_stream_t stream);
int smt_glow_coupling_bwd(const float* out, const float* x, const float* dz, const float* dlogdet, const int* lens,
                          float* dout, float* dx, int batch, int t, int channels, int sigmoid_scale, smt_stream_t stream);
/* Self-attention with relative-position keys and values (AttentionBlock.attention, submodules.py:463-512; window W, the
 * embeddings [2 W + 1, head_dim] shared by the heads): q, k, v, ctx [batch, t, heads * head_dim]; scores of padded queries /
 * keys are FILLED with -1e4 like the reference (a fully padded row is uniform); probs [batch, heads, t, t] = the softmax,
 * kept for the backward; dropout on the probabilities (index = linear index of probs).  Rows of q / k / v at padded positions
 * are never read where the reference's result does not depend on them (they may hold anything, NaN included): the backward
 * takes the same lens, and the score gradient of a padded pair is 0 as masked_fill's backward makes it. */
int smt_glow_attention_fwd(const float* q, const float* k, const float* v, const float* emb_rel_k, const float* emb_rel_v,
                           const int* lens, float* ctx, float* probs, int batch, int t, int heads, int head_dim, int window,
                           uint32_t drop_key, const uint32_t* drop_key_dev, uint32_t drop_thresh16, float drop_scale,
                           smt_stream_t stream);
size_t smt_glow_attention_bwd_workspace_bytes(int batch, int t, int heads, int head_dim, int window);
int smt_glow_attention_bwd(const float* q, const float* k, const float* v, const float* emb_rel_k, const float* emb_rel_v,
                           const float* probs, const int* lens, const float* dctx, float* dq, float* dk, float* dv, float* demb_rel_k,
                           float* demb_rel_v, int batch, int t, int heads, int head_dim, int window, uint32_t drop_key,
                           const uint32_t* drop_key_dev, uint32_t drop_thresh16, float drop_scale, void* workspace,
                           size_t workspace_bytes, smt_stream_t stream);
/* Prior log-likelihood of every (token, frame) pair (glow_tts.py:87-95), the input of smt_maximum_path:
 * x_m, x_logs [batch, t_x, dim] (x_logs NULL = zeros), z [batch, t_y, dim] -> logp [batch, t_x, t_y]. */
int smt_glow_prior_logp(const float* x_m, const float* x_logs, const float* z, float* logp, int batch, int t_x, int t_y,
                        int dim, smt_stream_t stream);
/* Alignment path [batch, t_x, t_y] (0/1) -> idx [batch, t_y] (token of each frame, -1 = none), durations [batch, t_x];
 * gather: z[b, j, :] = x[b, idx[b, j], :] (glow_tts.py:100-101, the matmul with the path); scatter = its adjoint. */
int smt_glow_align_index(const float* path, int* idx, float* durations, int batch, int t_x, int t_y, smt_stream_t stream);
int smt_glow_align_gather(const float* x, const int* idx, float* z, int batch, int t_x, int t_y, int dim, smt_stream_t stream);
int smt_glow_align_scatter(const float* dz, const int* idx, float* dx, int batch, int t_x, int t_y, int dim, smt_stream_t stream);
/* Inference durations (glow_tts.py:148-156, `infer_step`; ABI 5).  logw [batch, t_x], lens [batch] (int32) ->
 * w [batch, t_x] = ceil(exp(logw) length_scale) for t < lens[b], else 0 (logw is never read at or past lens[b]);
 * cum [batch, t_x] (int32) = inclusive prefix sum of w; z_lens[b] = (max(sum w, 1) / n_sqz) n_sqz.  An item with a non-finite
 * w or sum w > 2^24 (where the reference's fp32 cumsum stops being exact) gets z_lens[b] = -1 and cum = 0.
 * duration_index: idx [batch, t_out] (int32) = the token j < lens[b] with cum[b, j - 1] <= f < cum[b, j] for frames
 * f < z_lens[b] (-1 where no token covers f, and past z_lens[b]) -- the frame -> token convention of smt_glow_align_index,
 * so smt_glow_align_gather expands the prior statistics (the reference's generate_path + matmul, :157-163). */
int smt_glow_durations(const float* logw, const int* lens, int batch, int t_x, float length_scale, int n_sqz, float* w,
                       int* z_lens, int* cum, smt_stream_t stream);
int smt_glow_duration_index(const int* cum, const int* lens, const int* z_lens, int batch, int t_x, int t_out, int* idx,
                            smt_stream_t stream);
/* MLE loss pieces (glow_tts.py:115-119): sums[0] = sum z_logs, sums[1] = sum exp(-2 z_logs) (z - z_m)^2 over n elements
 * (z_logs NULL = zeros); bwd with the DEVICE scalar coef: dz = coef exp(-2 zl)(z - zm), dz_m = -dz, dz_logs = coef (1 - ...). */
size_t smt_glow_mle_workspace_bytes(int64_t n);
int smt_glow_mle_sums(const float* z, const float* z_m, const float* z_logs, int64_t n, float* sums, void* workspace,
                      size_t workspace_bytes, smt_stream_t stream);
int smt_glow_mle_bwd(const float* z, const float* z_m, const float* z_logs, const float* coef, int64_t n, float* dz, float* dz_m,
                     float* dz_logs, smt_stream_t stream);
/* Duration loss (glow_tts.py:99, 120): diff[b, t] = (logw - log(1e-8 + durations)) mask, sum[0] = sum diff^2. */
int smt_glow_length_loss(const float* logw, const float* durations, const int* lens, int batch, int t_x, float* diff, float* sum,
                         smt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SMT_HIP_H */
