// Vector-quantiser kernels for gfx950: exact nearest-code search, dequantise,
// commit/fit terms, straight-through backward, codebook EMA statistics and update.
//
// Replaces BottleneckBlock.quantize/dequantize/update_k of the reference
// (models/vqvae/bottleneck.py:60-90, 126-145, 171-201).
//
// Index semantics (oracle/vqvae_oracle.py: vq_argmin_exact): idx = the exact
// argmin_j ||x - k_j||^2 of the fp32 inputs, lowest j on ties.  Implementation:
//   0. prepare     (only when the codebook changes: smt_vq_prepare / smt_vq_ema_apply) codebook mean, centred bf16-pair
//                  split of the codes, -|k~|^2/2, max |k~|^2 -- kept in a persistent `prep` buffer;
//   1. vq_search   one workgroup sweeps ALL codes for its 64 rows on the matrix cores (3 x v_mfma_f32_32x32x16_bf16 per
//                  k-step on the bf16-pair split of the fp32 operands = a FILTER score); best / runner-up never leave
//                  registers; rows whose gap clears the rigorous round-off bound are finished in the same kernel
//                  (idx, min_dist, x_d), the others are queued with their threshold best - 2 err;
//   2. vq_candidates  queued rows only: the same MFMA sweep (code range split over workgroups) collects every code whose
//                  filter score reaches the row's threshold -- the exact argmin is provably among them;
//   3. vq_exact    scores just those in fp64, index order, no contraction (the oracle's arithmetic), lowest index on
//                  ties; a row with too many candidates (degenerate codebooks) scans ALL codes the same way;
//   4. vq_reduce   fixed-order sums (deterministic commit / fit).
// The [N, K] distance matrix is never materialised.
#include <algorithm>

#include "vq_common.h"

namespace smt {

#if VQ_ABL & 16     // phase timestamps of vq_search_kernel (100 MHz wall clock), tools/ablate_vq.sh only
__device__ long long vq_dbg[8192 * 6];
#define VQ_STAMP(k) do { if (threadIdx.x == 0 && blockIdx.x < 8192) vq_dbg[blockIdx.x * 6 + (k)] = wall_clock64(); } while (0)
#else
#define VQ_STAMP(k) do { } while (0)
#endif

// ---------------------------------------------------------------- prepare ---
// Distances are translation invariant, so the filter runs on data centred at the codebook mean mu: trained encoders
// emit rows with a large common offset, and the round-off bound that decides which rows need exact re-scoring scales
// with the NORMS of the operands, not their spread.  Column sums: per-part in index order, parts in index order.
struct VqPrep {
  float* mu;          // [D]
  float* nkhalf;      // [Kpad]   -0.5 |k~_j|^2, -3e38 for the padding codes j >= K
  unsigned* kmax2;    // max_j |k~_j|^2 (float bits); kmax2[32] = number of queued rows of the forward in flight (zero between calls)
  __bf16* kh;         // [Kpad][D] high halves of k~ = k - mu (zero rows for padding)
  __bf16* kl;         // [Kpad][D] low halves
  float* part;        // [ceil(K / VQ_PART)][D] partial column sums
  double* dkpart;     // [ceil(K / VQ_PART)]    partial sums of (k_new - k_old)^2 (EMA apply)
  int kpad, nparts;
};
static size_t vq_prep_layout(int K, int D, void* base, VqPrep* w) {
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return (char*)base + o; };
  const int kpad = (K + VQ_KPAD - 1) / VQ_KPAD * VQ_KPAD, nparts = (K + VQ_PART - 1) / VQ_PART;
  char* p;
  p = take((size_t)D * 4);            if (w) w->mu = (float*)p;
  p = take((size_t)kpad * 4);         if (w) w->nkhalf = (float*)p;
  p = take(256);                      if (w) w->kmax2 = (unsigned*)p;
  p = take((size_t)kpad * D * 2);     if (w) w->kh = (__bf16*)p;
  p = take((size_t)kpad * D * 2);     if (w) w->kl = (__bf16*)p;
  p = take((size_t)nparts * D * 4);   if (w) w->part = (float*)p;
  p = take((size_t)nparts * 8);       if (w) w->dkpart = (double*)p;
  if (w) { w->kpad = kpad; w->nparts = nparts; }
  return off;
}

// (vq_colsum_kernel, the partial column sums: vq_common.h)

// Single workgroup: mu from the partial column sums; with `cnt` also the metrics of update_k (bottleneck.py:85-90),
// all reductions in fixed order.
__global__ __launch_bounds__(1024) void vq_mu_kernel(const float* __restrict__ part, int nparts, int K, int D,
                                                     float* __restrict__ mu, unsigned* __restrict__ kmax2_bits,
                                                     const float* __restrict__ cnt, const float* __restrict__ k_elem,
                                                     const double* __restrict__ dkpart, float threshold,
                                                     float* __restrict__ metrics) {
  if ((int)threadIdx.x < D) {
    float t = 0.f;
#pragma unroll 16
    for (int p = 0; p < nparts; ++p) t += part[(size_t)p * D + threadIdx.x];   // index order; 16 loads in flight
    mu[threadIdx.x] = t / (float)K;
  }
  if (threadIdx.x == 0) { kmax2_bits[0] = 0u; kmax2_bits[32] = 0u; }     // + the queue counter of smt_vq_forward
  if (!cnt) return;                                        // workgroup-uniform
  vq_update_metrics(cnt, k_elem, dkpart, nparts, K, D, threshold, metrics);
}

// k~[j] = k[j] - mu as the bf16 pair (kh, kl) (v = hi + lo + eps, |eps| <= 2^-18 |v|), chunk-swizzled; nkhalf[j] =
// -0.5 |k~[j]|^2 (fp32, index order per lane then wave tree); kmax2 = max_j |k~[j]|^2.  One wave per code, 16 codes per
// workgroup (one atomicMax per workgroup); padding codes get zero rows and -inf.
__global__ __launch_bounds__(1024) void vq_split_kernel(const float* __restrict__ cb, const float* __restrict__ mu, int K,
                                                        int Kpad, int D, __bf16* __restrict__ kh, __bf16* __restrict__ kl,
                                                        float* __restrict__ nkhalf, unsigned* __restrict__ kmax2_bits) {
  __shared__ float wmax[16];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int code = blockIdx.x * 16 + wave;
  float s = 0.f;
  if (code < Kpad) {
    const int sw = vq_swz(code, D);
    for (int i = lane; i < D; i += 64) {
      const float v = code < K ? cb[(size_t)code * D + i] - mu[i] : 0.f;
      const __bf16 hi = (__bf16)v;
      const size_t o = (size_t)code * D + 8 * ((i >> 3) ^ sw) + (i & 7);
      kh[o] = hi;
      kl[o] = (__bf16)(v - (float)hi);
      s = fmaf(v, v, s);
    }
    s = wave_sum(s);
    if (lane == 0) nkhalf[code] = code < K ? -0.5f * s : -3.0e38f;   // padding: never the best, still a finite float
  }
  if (lane == 0) wmax[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = 0.f;
    for (int w = 0; w < 16; ++w) m = fmaxf(m, wmax[w]);
    atomicMax(kmax2_bits, __float_as_uint(m));  // m >= 0: uint order == float order
  }
}

// ---------------------------------------------------------------- search ----
// (operand layout, staging, the filter score and its error bound: vq_common.h)
// Shape: RG = blockDim / 128 column groups of 32 rows, two waves each.  Wave (rg, c) keeps column group rg in
// registers (bf16 pairs of its share of 32 rows) and takes chunks c and c + 2 of every staged 128-code step.  The host
// picks RG = ceil(rows / 32 / 256) (up to VQ_MAXRG) so that ONE round of workgroups covers all rows with at most one
// column group of imbalance, and a workgroup stages the whole codebook exactly once for its rows (LDS-DMA, double
// buffered, 2 x 64.5 KiB for D = 128: one workgroup per CU, 2 RG waves on its four SIMDs).
template <int D>
__global__ __launch_bounds__(128 * VQ_MAXRG) void vq_search_kernel(const float* __restrict__ x, const float* __restrict__ cb,
                                                        const float* __restrict__ row_mask, const float* __restrict__ mu,
                                                        const float* __restrict__ nkhalf, unsigned* __restrict__ kmax2_bits,
                                                        const __bf16* __restrict__ kh, const __bf16* __restrict__ kl,
                                                        long long N, int Kpad, long long* __restrict__ idx,
                                                        float* __restrict__ min_dist, float* __restrict__ x_d,
                                                        int* __restrict__ q_rows, float* __restrict__ q_thr) {
  constexpr int SUP = VQ_SSUP;
  using G = VqGeom<D, SUP>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nw = blockDim.x >> 6, tile = 16 * nw;           // waves, rows per workgroup
  float* m_best = reinterpret_cast<float*>(smem + 2 * G::BUF_BYTES);
  float* m_second = m_best + tile;
  int* m_idx = reinterpret_cast<int*>(m_second + tile);

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int rg = wave >> 1, c = wave & 1;
  const long long row0 = (long long)blockIdx.x * tile;

  char* buf0 = smem;
  char* buf1 = smem + G::BUF_BYTES;
  VQ_STAMP(0);
  vq_stage<D, SUP>(kh, kl, nkhalf, 0, buf0, nw, wave, lane);
  vq_stage<D, SUP>(kh, kl, nkhalf, 1, buf1, nw, wave, lane);
  vq_bf16x8 xh[1][G::NS], xl[1][G::NS];
  float xx;
  {
    const long long row = min(row0 + 32 * rg + j, N - 1);   // rows past the end repeat the last row and are never written
    xx = vq_load_row<D>(x, mu, row, h, xh[0], xl[0]);
    xx += __shfl_xor(xx, 32, 64);
  }
  vm_wait<0>();
  __syncthreads();
  VQ_STAMP(1);

  float best[1] = {-INFINITY}, second[1] = {-INFINITY};
  int bidx[1] = {0x7fffffff};
  const int nsc = Kpad / SUP;                               // even (the prep pads to 256 codes)
  f32x16 acc[1];
  // The running best / runner-up costs VALU issue slots that the matrix pipe cannot hide (measured: it adds to the MFMA
  // time), so it is cut to 3 instructions per score: the score's position r in the chunk is written into its 4 low
  // mantissa bits (error <= 2^-19 |score|, accounted for in vq_filter_err), after which max / med3 on the tagged floats
  // carry the position along; which chunk holds the best is noted once per chunk.
  int bchunk = 0;
  float pinf = INFINITY;
  asm volatile("" : "+v"(pinf));
  auto score_step = [&](const char* buf, int sc) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int chunk = c + 2 * q;
      vq_chunk_scores<D, SUP, 1>(buf, chunk, j, h, xh, xl, acc);
      if (!(VQ_ABL & 4)) {
        const float before = best[0];
#pragma unroll
        for (int r = 0; r < 16; ++r) {            // v_and_or_b32, v_med3_f32, v_med3_f32 (plain builtins: the compiler
          const float t = __int_as_float((__float_as_int(acc[0][r]) & ~15) | r);   // pads the MFMA -> VALU hazards itself)
          second[0] = __builtin_amdgcn_fmed3f(best[0], second[0], t);
          best[0] = __builtin_amdgcn_fmed3f(best[0], t, pinf);                     // = max; pinf is opaque, so it stays one med3
        }
        bchunk = best[0] != before ? sc * (SUP / VQ_CHUNK) + chunk : bchunk;
      } else {
        best[0] += acc[0][0] + acc[0][5] + acc[0][10] + acc[0][15];      // keeps the MFMA chain alive
      }
    }
  };
  for (int sc = 0; sc < nsc; sc += 2) {
    score_step(buf0, sc);
    vm_wait<0>();                                           // step sc + 1 (issued one scoring phase ago) has landed in buf1
    __syncthreads();                                        // buf0 released
    if (sc + 2 < nsc) vq_stage<D, SUP>(kh, kl, nkhalf, sc + 2, buf0, nw, wave, lane);
    score_step(buf1, sc + 1);
    vm_wait<0>();
    __syncthreads();                                        // buf1 released, step sc + 2 landed in buf0
    if (sc + 3 < nsc) vq_stage<D, SUP>(kh, kl, nkhalf, sc + 3, buf1, nw, wave, lane);   // lands while step sc + 2 is scored
  }
  VQ_STAMP(2);
  {  // decode the winner: chunk, position tag, lane half
    const int r = __float_as_int(best[0]) & 15;
    bidx[0] = bchunk * VQ_CHUNK + 8 * (r >> 2) + 4 * h + (r & 3);
  }
  // merge the two lane halves of a row (same row, disjoint codes), then the two chunk waves of the column group
  {
    const float ob = __shfl_xor(best[0], 32, 64), os = __shfl_xor(second[0], 32, 64);
    const int oi = __shfl_xor(bidx[0], 32, 64);
    vq_merge(best[0], second[0], bidx[0], ob, os, oi);
  }
  float b = best[0], s2 = second[0];
  int bi = bidx[0];
  if (c == 1 && h == 0) { m_best[32 * rg + j] = b; m_second[32 * rg + j] = s2; m_idx[32 * rg + j] = bi; }
  __syncthreads();
  if (c == 0 && h == 0) {
    const int r = 32 * rg + j;
    vq_merge(b, s2, bi, m_best[r], m_second[r], m_idx[r]);
    const long long row = row0 + r;
    const float err = vq_filter_err(xx, __uint_as_float(kmax2_bits[0]), D);
    const bool ambiguous = !((b - s2) > 2.0f * err);        // also catches NaN / inf
    int res = bi;
    if (row < N && ambiguous) {
      const int q = atomicAdd(reinterpret_cast<int*>(kmax2_bits + 32), 1);
      q_rows[q] = (int)row;
      q_thr[q] = b - 2.0f * err;
      res = -1;
    }
    m_idx[r] = res;
  }
  __syncthreads();
  VQ_STAMP(3);
  // finish the unambiguous rows: idx, min_dist = |x - k_idx|^2 (fp32 direct form), x_d = k_idx * mask.
  // LPR lanes per row, RPI rows per wave-instruction, 16 rows per wave; loads of a batch are issued together.
  constexpr int RPW = 16, LPR = D / 4, RPI = 64 / LPR, NIT = RPW / RPI, BATCH = NIT < 4 ? NIT : 4;
  const int c4 = lane % LPR;
#pragma unroll 1
  for (int it0 = 0; it0 < ((VQ_ABL & 8) ? 0 : NIT); it0 += BATCH) {
    f32x4 xv[BATCH], kv[BATCH];
    int code[BATCH];
    long long rows[BATCH];
#pragma unroll
    for (int q = 0; q < BATCH; ++q) {
      const int r = RPW * wave + (it0 + q) * RPI + lane / LPR;
      rows[q] = row0 + r;
      code[q] = m_idx[r];
      xv[q] = *reinterpret_cast<const f32x4*>(x + min(rows[q], N - 1) * D + 4 * c4);
      kv[q] = *reinterpret_cast<const f32x4*>(cb + (size_t)max(code[q], 0) * D + 4 * c4);
    }
#pragma unroll
    for (int q = 0; q < BATCH; ++q) {
      const f32x4 df = xv[q] - kv[q];
      float ds = fmaf(df.w, df.w, fmaf(df.z, df.z, fmaf(df.y, df.y, df.x * df.x)));
#pragma unroll
      for (int o = LPR / 2; o > 0; o >>= 1) ds += __shfl_xor(ds, o, 64);
      if (rows[q] < N && code[q] >= 0) {
        if (x_d) {
          const float m = row_mask ? row_mask[rows[q]] : 1.f;
          *reinterpret_cast<f32x4*>(x_d + rows[q] * D + 4 * c4) = kv[q] * m;
        }
        if (c4 == 0) { idx[rows[q]] = code[q]; min_dist[rows[q]] = ds; }
      }
    }
  }
  VQ_STAMP(4);
}

// ---------------------------------------------------------------- candidates
// Queued rows, 32 at a time, the code range cut into `splits` pieces (one workgroup per (row group, piece)): with filter
// scores f_j (|f_j - s_j| <= err against the exact scores s_j) and the first pass's maximum fmax, the exact winner j*
// satisfies f_j* >= s_j* - err >= s_jmax - err >= fmax - 2 err for ANY filter values within err of the truth -- so every
// code whose score here reaches thr = fmax - 2 err is recorded (up to VQ_CAPS per row and piece; the count is recorded
// in full so that vq_exact sees an overflow).
template <int D>
__global__ __launch_bounds__(128) void vq_candidates_kernel(const float* __restrict__ x, const float* __restrict__ mu,
                                                            const float* __restrict__ nkhalf, const unsigned* __restrict__ kmax2_bits,
                                                            const __bf16* __restrict__ kh, const __bf16* __restrict__ kl,
                                                            int Kpad, int splits, const int* __restrict__ q_rows,
                                                            const float* __restrict__ q_thr, int* __restrict__ c_count,
                                                            int* __restrict__ c_codes) {
  constexpr int SUP = VQ_CSUP;
  using G = VqGeom<D, SUP>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int l_cnt[32];
  __shared__ int l_code[32][VQ_CAPS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int n_q = (int)kmax2_bits[32];
  const int nsc = Kpad / SUP, per = nsc / splits;      // staged steps per piece
  const int ntask = ((n_q + 31) / 32) * splits;
  for (int task = blockIdx.x; task < ntask; task += gridDim.x) {
    const int rg = task / splits, sp = task % splits;
    __syncthreads();                                        // the previous task's lists are no longer read
    if (threadIdx.x < 32) l_cnt[threadIdx.x] = 0;
    const int qi = min(rg * 32 + j, n_q - 1);
    const float thr = rg * 32 + j < n_q ? q_thr[qi] : INFINITY;
    vq_stage<D, SUP>(kh, kl, nkhalf, sp * per, smem, 2, wave, lane);
    vq_bf16x8 xh[1][G::NS], xl[1][G::NS];
    (void)vq_load_row<D>(x, mu, (long long)q_rows[qi], h, xh[0], xl[0]);
    vm_wait<0>();
    __syncthreads();
    for (int i = 0; i < per; ++i) {
      const int buf = i & 1, sc = sp * per + i;
      if (i + 1 < per) vq_stage<D, SUP>(kh, kl, nkhalf, sc + 1, smem + (buf ^ 1) * G::BUF_BYTES, 2, wave, lane);
      f32x16 acc[1];
      vq_chunk_scores<D, SUP, 1>(smem + buf * G::BUF_BYTES, wave, j, h, xh, xl, acc);
      const int cbase = sc * SUP + wave * VQ_CHUNK + 4 * h;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (acc[0][r] >= thr) {                             // padding codes score -inf, NaN compares false
          const int pos = atomicAdd(&l_cnt[j], 1);
          if (pos < VQ_CAPS) l_code[j][pos] = cbase + 8 * (r >> 2) + (r & 3);
        }
      }
      vm_wait<0>();
      __syncthreads();
    }
    if (threadIdx.x < 32 && rg * 32 + (int)threadIdx.x < n_q) {
      const size_t slot = (size_t)(rg * 32 + threadIdx.x) * splits + sp;
      c_count[slot] = l_cnt[threadIdx.x];
#pragma unroll
      for (int c = 0; c < VQ_CAPS; ++c) c_codes[slot * VQ_CAPS + c] = l_code[threadIdx.x][c];
    }
  }
}

// ---------------------------------------------------------------- exact -----
// (vq_exact_dist: vq_common.h)  Half a wave per queued row, one lane per candidate slot (splits * VQ_CAPS <= 32); lowest index among equal distances.
// A row with no candidate or an overflowing piece (NaN input, degenerate codebook) scans all K codes the same way.
__global__ __launch_bounds__(256) void vq_exact_kernel(const float* __restrict__ x, const float* __restrict__ cb,
                                                       const float* __restrict__ row_mask, const unsigned* __restrict__ kmax2_bits,
                                                       int K, int D, int splits, const int* __restrict__ q_rows,
                                                       const int* __restrict__ c_count, const int* __restrict__ c_codes,
                                                       long long* __restrict__ idx, float* __restrict__ min_dist,
                                                       float* __restrict__ x_d) {
  const int n_q = (int)kmax2_bits[32];
  const int lane = threadIdx.x & 63, half = lane >> 5, l = lane & 31;
  const int hw0 = (((int)blockIdx.x * 256 + (int)threadIdx.x) >> 6) * 2, nhw = (int)gridDim.x * 8;
  for (int q0 = hw0; q0 < n_q; q0 += nhw) {                  // wave-uniform trip count; the second half may idle
    const int qi = q0 + half;
    const bool rvalid = qi < n_q;
    const long long row = rvalid ? q_rows[qi] : 0;
    const float* xr = x + row * D;
    const int sp = l / VQ_CAPS, c = l % VQ_CAPS;
    int n = 0;
    if (rvalid && sp < splits) n = c_count[(size_t)qi * splits + sp];
    // any piece over capacity, or no candidate at all, anywhere in this half-wave's row?
    const unsigned long long over = __ballot(n > VQ_CAPS), some = __ballot(n > 0);
    const unsigned long long hmask = half ? 0xffffffff00000000ull : 0x00000000ffffffffull;
    const bool full = rvalid && ((over & hmask) != 0 || (some & hmask) == 0);
    double d = INFINITY;
    int code = 0x7fffffff;
    if (rvalid && !full && c < n) {
      code = c_codes[((size_t)qi * splits + sp) * VQ_CAPS + c];
      d = vq_exact_dist(xr, cb + (size_t)code * D, D);
    }
    if (full) {
      for (int c0 = l; c0 < K; c0 += 32) {                   // increasing code order per lane: strict '<' keeps the lowest
        const double dc = vq_exact_dist(xr, cb + (size_t)c0 * D, D);
        if (dc < d) { d = dc; code = c0; }
      }
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
      const double od = __shfl_xor(d, o, 64);
      const int oc = __shfl_xor(code, o, 64);
      if (od < d || (od == d && oc < code)) { d = od; code = oc; }
    }
    if (!rvalid) continue;
    const bool found = code != 0x7fffffff;                   // false on a NaN row: keep the outputs defined (code 0, as
    const int cc = found ? code : 0;                         // vqg_exact_kernel and the reference's min over NaNs do)
    if (x_d) {
      const float m = row_mask ? row_mask[row] : 1.f;
      for (int i = l; i < D; i += 32) x_d[row * D + i] = cb[(size_t)cc * D + i] * m;
    }
    if (l == 0) { idx[row] = cc; min_dist[row] = found ? (float)d : __builtin_nanf(""); }   // the exact distance, rounded once
  }
}

// (vq_reduce_kernel, the fixed-order sums: vq_common.h)
// ---------------------------------------------------------------- backward --
__global__ __launch_bounds__(256) void vq_backward_kernel(const float* __restrict__ x, const float* __restrict__ x_d,
                                                          const float* __restrict__ row_mask, const float* __restrict__ dy,
                                                          const float* __restrict__ g_commit, const float* __restrict__ sums,
                                                          long long N, int D, float* __restrict__ dx) {
  const long long total4 = N * D / 4;
  const float gc = g_commit ? (*g_commit) * 2.0f / (sums[2] * (float)D) : 0.f;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total4;
       e += (long long)gridDim.x * blockDim.x) {
    const long long row = (e * 4) / D;
    const float m = row_mask ? row_mask[row] : 1.f;
    f32x4 xv = *reinterpret_cast<const f32x4*>(x + e * 4);
    f32x4 out = {0.f, 0.f, 0.f, 0.f};
    if (dy) {
      f32x4 g = *reinterpret_cast<const f32x4*>(dy + e * 4);
      out = g * m;
    }
    if (g_commit && m != 0.f) {
      f32x4 kv = *reinterpret_cast<const f32x4*>(x_d + e * 4);      // = k[idx[row]] on unmasked rows (0/1 masks)
      out += (xv - kv) * gc;
    }
    *reinterpret_cast<f32x4*>(dx + e * 4) = out;
  }
}

// ---------------------------------------------------------------- EMA -------
// _k_sum = onehot^T x, _k_elem = column sums of onehot (bottleneck.py:64-68) as a scatter-add.  The sums are accumulated
// in 64-bit FIXED POINT (2^-24 units) with integer atomics: integer addition is associative, so the result does not
// depend on the order in which rows arrive -- bit-reproducible from run to run, which f32 atomics are not -- and is
// converted to f32 once at the end.  A value is exact when it is a multiple of 2^-24 below 2^15 in magnitude (every bf16
// and every f32 encoder output of ordinary size); larger magnitudes saturate at +-2^39 units so that 2^23 rows cannot
// overflow the accumulator.  One wave per row; 512 contiguous bytes per atomic wave-instruction.
constexpr float VQ_FX_SCALE = 16777216.f;            // 2^24
constexpr float VQ_FX_LIMIT = 549755813888.f;        // 2^39

// Round 3: the scatter-add no longer issues one atomic per (row, channel).  Under skewed usage -- a trained codebook
// concentrates on a few codes, a collapsing one on very few -- those atomics pile up on the same lines (measured: 47-400 us
// over four train steps, 548 us in the round-2 driver run, against 75 us on uniform usage).  The rows are first grouped by
// code with a counting sort whose histogram and cursors are privatised in LDS (integer atomics only, at most one global
// atomic per (workgroup, code)), then waves walk equal shares of the sorted order and keep the running sum of the current
// code in registers: one 64-bit integer atomic per channel per (share, code) boundary instead of per row -- 23x fewer on
// uniform usage, and the more skewed the usage, the fewer.  Integer sums: any order gives the same bits.
constexpr int VQ_EMA_HIST_NT = 1024;
// counts[code] += rows of this workgroup's share with that code (masked rows excluded)
__global__ __launch_bounds__(VQ_EMA_HIST_NT) void vq_ema_count_kernel(const long long* __restrict__ idx, const float* __restrict__ row_mask,
                                                                     long long N, int K, int rows_per_wg, int* __restrict__ counts) {
  extern __shared__ int hist[];
  for (int k = threadIdx.x; k < K; k += VQ_EMA_HIST_NT) hist[k] = 0;
  __syncthreads();
  const long long r0 = (long long)blockIdx.x * rows_per_wg, r1 = min(N, r0 + rows_per_wg);
  for (long long r = r0 + threadIdx.x; r < r1; r += VQ_EMA_HIST_NT)
    if (!row_mask || row_mask[r] != 0.f) atomicAdd(&hist[(int)idx[r]], 1);
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += VQ_EMA_HIST_NT)
    if (hist[k]) atomicAdd(&counts[k], hist[k]);
}
// exclusive scan of counts -> cursor (one workgroup; K <= a few thousand); total[0] = number of unmasked rows
__global__ __launch_bounds__(1024) void vq_ema_scan_kernel(const int* __restrict__ counts, int K, int* __restrict__ cursor, int* __restrict__ total) {
  __shared__ int part[1024];
  const int per = (K + 1023) / 1024, k0 = threadIdx.x * per;
  int s = 0;
  for (int k = k0; k < min(K, k0 + per); ++k) s += counts[k];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int v = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  int run = part[threadIdx.x] - s;
  for (int k = k0; k < min(K, k0 + per); ++k) { cursor[k] = run; run += counts[k]; }
  if (threadIdx.x == 1023) total[0] = part[1023];
}
// order[cursor[code]++] = row, with the cursor advanced once per (workgroup, code)
__global__ __launch_bounds__(VQ_EMA_HIST_NT) void vq_ema_scatter_kernel(const long long* __restrict__ idx, const float* __restrict__ row_mask,
                                                                       long long N, int K, int rows_per_wg, int* __restrict__ cursor,
                                                                       int* __restrict__ order) {
  extern __shared__ int sm[];            // hist [K] | base [K]
  int* hist = sm;
  int* base = sm + K;
  for (int k = threadIdx.x; k < K; k += VQ_EMA_HIST_NT) hist[k] = 0;
  __syncthreads();
  const long long r0 = (long long)blockIdx.x * rows_per_wg, r1 = min(N, r0 + rows_per_wg);
  for (long long r = r0 + threadIdx.x; r < r1; r += VQ_EMA_HIST_NT)
    if (!row_mask || row_mask[r] != 0.f) atomicAdd(&hist[(int)idx[r]], 1);
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += VQ_EMA_HIST_NT) {
    base[k] = hist[k] ? atomicAdd(&cursor[k], hist[k]) : 0;
    hist[k] = 0;
  }
  __syncthreads();
  for (long long r = r0 + threadIdx.x; r < r1; r += VQ_EMA_HIST_NT)
    if (!row_mask || row_mask[r] != 0.f) {
      const int code = (int)idx[r];
      order[base[code] + atomicAdd(&hist[code], 1)] = (int)r;
    }
}
// ---- tables of more than VQ_EMA_LDS_BINS codes (the grouped bottleneck: n_vocab * l_bins, tens of thousands) ----
// The histogram no longer fits in LDS and one workgroup no longer scans it, so the same counting sort runs on global
// memory: one integer atomic per unmasked row into counts[K] and one into cursor[K] (with K >> rows per code the atomics
// spread over many lines), and a two-launch scan in blocks of VQ_EMA_SCAN_BLOCK codes.  The sorted order then feeds the
// SAME accumulate / convert kernels as the small path: 64-bit fixed-point sums, any order gives the same bits.  A code
// outside [0, K) is skipped by count and scatter alike (never a write out of range).
constexpr int VQ_EMA_LDS_BINS = 16384;
constexpr int VQ_EMA_MAX_BINS = 1 << 18;
constexpr int VQ_EMA_SCAN_BLOCK = 4096;         // codes per workgroup of the large scan: 4 per thread
__global__ __launch_bounds__(256) void vq_ema_count_large_kernel(const long long* __restrict__ idx, const float* __restrict__ row_mask,
                                                                 long long N, int K, int* __restrict__ counts) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= N || (row_mask && row_mask[r] == 0.f)) return;
  const long long code = idx[r];
  if (code >= 0 && code < K) atomicAdd(&counts[code], 1);
}
// this thread's four codes of block blockIdx.x (zero past K)
__device__ __forceinline__ void vq_ema_load4(const int* __restrict__ counts, int K, int k0, int* c) {
#pragma unroll
  for (int e = 0; e < 4; ++e) c[e] = k0 + e < K ? counts[k0 + e] : 0;
}
__global__ __launch_bounds__(1024) void vq_ema_blocksum_kernel(const int* __restrict__ counts, int K, int* __restrict__ bsum) {
  __shared__ int sh[16];
  int c[4];
  vq_ema_load4(counts, K, blockIdx.x * VQ_EMA_SCAN_BLOCK + 4 * threadIdx.x, c);
  int s = (c[0] + c[1]) + (c[2] + c[3]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < 16; ++w) t += sh[w];
    bsum[blockIdx.x] = t;
  }
}
__global__ __launch_bounds__(1024) void vq_ema_scan_large_kernel(const int* __restrict__ counts, int K, const int* __restrict__ bsum,
                                                                int* __restrict__ cursor, int* __restrict__ total) {
  __shared__ int part[1024];
  __shared__ int base;
  if (threadIdx.x == 0) {
    int t = 0;
    for (int b = 0; b < (int)blockIdx.x; ++b) t += bsum[b];        // at most VQ_EMA_MAX_BINS / VQ_EMA_SCAN_BLOCK = 64 terms
    base = t;
  }
  const int k0 = blockIdx.x * VQ_EMA_SCAN_BLOCK + 4 * threadIdx.x;
  int c[4];
  vq_ema_load4(counts, K, k0, c);
  const int s = (c[0] + c[1]) + (c[2] + c[3]);
  part[threadIdx.x] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int v = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  int run = base + part[threadIdx.x] - s;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (k0 + e < K) cursor[k0 + e] = run;
    run += c[e];
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 1023) total[0] = base + part[1023];
}
__global__ __launch_bounds__(256) void vq_ema_scatter_large_kernel(const long long* __restrict__ idx, const float* __restrict__ row_mask,
                                                                   long long N, int K, int* __restrict__ cursor, int* __restrict__ order) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= N || (row_mask && row_mask[r] == 0.f)) return;
  const long long code = idx[r];
  if (code >= 0 && code < K) order[atomicAdd(&cursor[code], 1)] = (int)r;
}

// one wave per share of VQ_EMA_SHARE sorted rows; PER = ceil(D / 64) channels per lane (D = 32: the upper half of the wave idles)
constexpr int VQ_EMA_SHARE = 64;
// A wave owns 64 consecutive positions of the sorted order.  Lane l fetches the row id and the code of position r0 + l once
// (one coalesced load + one gather); the rows are then read sixteen at a time with wave-uniform row ids (v_readlane), so a
// share costs ~6 memory round trips.  (The first version walked 128 positions four at a time with order -> idx -> x as
// dependent loads: 2 x 32 round trips per wave, 119 us of latency for 19 MB.)
template <int D>
__global__ __launch_bounds__(256) void vq_ema_accumulate_kernel(const float* __restrict__ x, const long long* __restrict__ idx,
                                                                const int* __restrict__ order, const int* __restrict__ total, int K,
                                                                unsigned long long* __restrict__ acc) {
  constexpr int PER = (D + 63) / 64;
  const int lane = threadIdx.x & 63;
  const bool live = lane < D;
  const long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
  const long long r0 = wave * VQ_EMA_SHARE, r1 = min((long long)total[0], r0 + VQ_EMA_SHARE);
  if (r0 >= r1) return;
  const int n = (int)(r1 - r0);
  const int my_row = lane < n ? order[r0 + lane] : 0;
  const int my_code = lane < n ? (int)idx[my_row] : -1;
  long long sum[PER];
#pragma unroll
  for (int q = 0; q < PER; ++q) sum[q] = 0;
  int cur = -1, cnt = 0;
  auto flush = [&]() {
    if (cur < 0) return;
#pragma unroll
    for (int q = 0; q < PER; ++q)
      if (live) atomicAdd(acc + (size_t)cur * D + lane + 64 * q, (unsigned long long)sum[q]);   // two's complement
    if (lane == 0) atomicAdd(acc + (size_t)K * D + cur, (unsigned long long)cnt);
  };
  for (int g = 0; g < n; g += 16) {
    float v[16][PER];
    int code[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int pos = min(g + u, n - 1);                             // wave-uniform
      const int row = __builtin_amdgcn_readlane(my_row, pos);
      code[u] = g + u < n ? __builtin_amdgcn_readlane(my_code, pos) : -1;
#pragma unroll
      for (int q = 0; q < PER; ++q) v[u][q] = live ? x[(size_t)row * D + lane + 64 * q] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      if (code[u] < 0) continue;                                     // uniform
      if (code[u] != cur) {
        flush();
        cur = code[u]; cnt = 0;
#pragma unroll
        for (int q = 0; q < PER; ++q) sum[q] = 0;
      }
#pragma unroll
      for (int q = 0; q < PER; ++q)
        sum[q] += __float2ll_rn(fminf(fmaxf(v[u][q] * VQ_FX_SCALE, -VQ_FX_LIMIT), VQ_FX_LIMIT));
      ++cnt;
    }
  }
  flush();
}
__global__ __launch_bounds__(256) void vq_ema_convert_kernel(const unsigned long long* __restrict__ acc, float* __restrict__ stats,
                                                             int n_sums, int n_total) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n_total) return;
  const long long v = (long long)acc[e];
  stats[e] = e < n_sums ? (float)((double)v * (1.0 / 16777216.0)) : (float)v;
}

// (vq_ema_apply_kernel, the EMA mix + revival: vq_common.h)

struct VqWorkspace { int* q_rows; float* q_thr; int* c_count; int* c_codes; void* prep; };

static size_t vq_layout(long long N, int K, int D, void* base, VqWorkspace* w) {
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return (char*)base + o; };
  char* p;
  p = take((size_t)N * 4); if (w) w->q_rows = (int*)p;
  p = take((size_t)N * 4); if (w) w->q_thr = (float*)p;
  p = take((size_t)N * VQ_SPLITS * 4);           if (w) w->c_count = (int*)p;
  p = take((size_t)N * VQ_SPLITS * VQ_CAPS * 4); if (w) w->c_codes = (int*)p;
  p = take(vq_prep_layout(K, D, nullptr, nullptr)); if (w) w->prep = p;   // used when the caller passes no prep buffer
  return off;
}

// column sums -> mu (-> metrics) -> centred split: the three launches behind smt_vq_prepare and smt_vq_ema_apply
static int vq_finish_prepare(const float* cb, int K, int D, const VqPrep& pr, const float* cnt, const float* k_elem,
                             float threshold, float* metrics, hipStream_t stream) {
  vq_mu_kernel<<<1, 1024, 0, stream>>>(pr.part, pr.nparts, K, D, pr.mu, pr.kmax2, cnt, k_elem, pr.dkpart, threshold, metrics);
  SMT_CHECK_LAUNCH("vq_mu");
  vq_split_kernel<<<(pr.kpad + 15) / 16, 1024, 0, stream>>>(cb, pr.mu, K, pr.kpad, D, pr.kh, pr.kl, pr.nkhalf, pr.kmax2);
  SMT_CHECK_LAUNCH("vq_split");
  return 0;
}

template <int D>
static int vq_launch_search(const float* x, const float* cb, const float* row_mask, const VqPrep& pr, long long N, int K,
                            long long* idx, float* min_dist, float* x_d, const VqWorkspace& w, hipStream_t stream) {
  using GS = VqGeom<D, VQ_SSUP>;
  using GC = VqGeom<D, VQ_CSUP>;
  const long long groups = (N + 31) / 32;
  // column groups per workgroup: one round of at most 256 workgroups when that fits (<= VQ_MAXRG groups each)
  const int rgs = (int)std::min<long long>(VQ_MAXRG, (groups + 255) / 256);
  const size_t lds = 2 * GS::BUF_BYTES + 3 * 32 * rgs * 4;
  (void)hipFuncSetAttribute((const void*)vq_search_kernel<D>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(2 * GS::BUF_BYTES + 3 * 32 * VQ_MAXRG * 4));
  (void)hipFuncSetAttribute((const void*)vq_candidates_kernel<D>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * GC::BUF_BYTES);
  vq_search_kernel<D><<<(unsigned)((groups + rgs - 1) / rgs), 128 * rgs, lds, stream>>>(
      x, cb, row_mask, pr.mu, pr.nkhalf, pr.kmax2, pr.kh, pr.kl, N, pr.kpad, idx, min_dist, x_d, w.q_rows, w.q_thr);
  SMT_CHECK_LAUNCH("vq_search");
  const int nsc = pr.kpad / VQ_CSUP;
  int splits = VQ_SPLITS;
  while (nsc % splits) splits >>= 1;                         // nsc is a multiple of 4
  vq_candidates_kernel<D><<<(unsigned)std::min<long long>(512, groups * splits), 128, 2 * GC::BUF_BYTES, stream>>>(
      x, pr.mu, pr.nkhalf, pr.kmax2, pr.kh, pr.kl, pr.kpad, splits, w.q_rows, w.q_thr, w.c_count, w.c_codes);
  SMT_CHECK_LAUNCH("vq_candidates");
  vq_exact_kernel<<<(unsigned)std::min<long long>(256, (N + 7) / 8), 256, 0, stream>>>(
      x, cb, row_mask, pr.kmax2, K, D, splits, w.q_rows, w.c_count, w.c_codes, idx, min_dist, x_d);
  SMT_CHECK_LAUNCH("vq_exact");
  return 0;
}

}  // namespace smt

using namespace smt;

#if VQ_ABL & 16
extern "C" int smt_vq_debug_dump(long long* host, int n) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(vq_dbg), sizeof(long long) * n);
}
#endif

extern "C" size_t smt_vq_prep_bytes(int k_bins, int dim) { return vq_prep_layout(k_bins, dim, nullptr, nullptr); }

extern "C" int smt_vq_prepare(const float* codebook, int k_bins, int dim, void* prep, size_t prep_bytes, smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SMT_CHECK_ARG(dim == 32 || dim == 64 || dim == 128, "smt_vq_prepare: dim must be 32, 64 or 128 (got %d)", dim);
  SMT_CHECK_ARG(codebook && prep && k_bins >= 1, "smt_vq_prepare: null pointer / bad size");
  SMT_CHECK_ARG(prep_bytes >= vq_prep_layout(k_bins, dim, nullptr, nullptr), "smt_vq_prepare: prep buffer too small");
  VqPrep pr;
  vq_prep_layout(k_bins, dim, prep, &pr);
  vq_colsum_kernel<<<pr.nparts, 128, 0, stream>>>(codebook, k_bins, dim, pr.part);
  SMT_CHECK_LAUNCH("vq_colsum");
  return vq_finish_prepare(codebook, k_bins, dim, pr, nullptr, nullptr, 0.f, nullptr, stream);
}

extern "C" size_t smt_vq_forward_workspace_bytes(int64_t n_rows, int k_bins, int dim) {
  return vq_layout(n_rows, k_bins, dim, nullptr, nullptr);
}

extern "C" int smt_vq_forward(const float* x, const float* codebook, void* prep, const float* row_mask,
                              int64_t n_rows, int k_bins, int dim, int64_t* idx, float* min_dist, float* x_d, float* sums,
                              void* workspace, size_t workspace_bytes, smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SMT_CHECK_ARG(dim == 32 || dim == 64 || dim == 128, "smt_vq_forward: dim must be 32, 64 or 128 (got %d)", dim);
  SMT_CHECK_ARG(k_bins >= 1 && n_rows >= 0, "smt_vq_forward: bad sizes n_rows=%lld k_bins=%d", (long long)n_rows, k_bins);
  SMT_CHECK_ARG(n_rows < (1ll << 31), "smt_vq_forward: n_rows must be < 2^31");
  SMT_CHECK_ARG(codebook && sums && workspace, "smt_vq_forward: null pointer");
  SMT_CHECK_ARG(n_rows == 0 || (x && idx && min_dist), "smt_vq_forward: null pointer");
  SMT_CHECK_ARG(workspace_bytes >= vq_layout(n_rows, k_bins, dim, nullptr, nullptr), "smt_vq_forward: workspace too small");
  VqWorkspace w;
  vq_layout(n_rows, k_bins, dim, workspace, &w);
  if (n_rows == 0) {
    (void)hipMemsetAsync(sums, 0, 16, stream);
    return 0;
  }
  VqPrep pr;
  if (prep) {
    vq_prep_layout(k_bins, dim, prep, &pr);
  } else {                                   // no cached split of this codebook: build one in the workspace
    int rc = smt_vq_prepare(codebook, k_bins, dim, w.prep, vq_prep_layout(k_bins, dim, nullptr, nullptr), stream_);
    if (rc) return rc;
    vq_prep_layout(k_bins, dim, w.prep, &pr);
  }
  int rc;
  if (dim == 128) rc = vq_launch_search<128>(x, codebook, row_mask, pr, n_rows, k_bins, (long long*)idx, min_dist, x_d, w, stream);
  else if (dim == 64) rc = vq_launch_search<64>(x, codebook, row_mask, pr, n_rows, k_bins, (long long*)idx, min_dist, x_d, w, stream);
  else rc = vq_launch_search<32>(x, codebook, row_mask, pr, n_rows, k_bins, (long long*)idx, min_dist, x_d, w, stream);
  if (rc) return rc;
  vq_reduce_kernel<<<1, 1024, 0, stream>>>(min_dist, row_mask, n_rows, pr.kmax2, sums);
  SMT_CHECK_LAUNCH("vq_reduce");
  return 0;
}

extern "C" int smt_vq_backward(const float* x, const float* x_d, const float* row_mask, const float* dy,
                               const float* g_commit, const float* sums, int64_t n_rows, int dim, float* dx,
                               smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SMT_CHECK_ARG(dim % 4 == 0, "smt_vq_backward: dim must be a multiple of 4");
  if (n_rows == 0) return 0;
  SMT_CHECK_ARG(x && x_d && sums && dx, "smt_vq_backward: null pointer");
  long long total4 = n_rows * dim / 4;
  unsigned grid = (unsigned)min((long long)2048, (total4 + 255) / 256);
  vq_backward_kernel<<<grid, 256, 0, stream>>>(x, x_d, row_mask, dy, g_commit, sums, n_rows, dim, dx);
  SMT_CHECK_LAUNCH("vq_backward");
  return 0;
}

// workspace: acc u64 [K D + K] | counts int [K] | cursor int [K] | total int [64] (| bsum int [64]) | order int [N]
static size_t vq_ema_ws_layout(long long N, int K, int D, size_t* off_counts, size_t* off_cursor, size_t* off_total, size_t* off_order) {
  size_t off = align_up(((size_t)K * D + K) * sizeof(unsigned long long), 256);
  if (off_counts) *off_counts = off;
  off += align_up((size_t)K * sizeof(int), 256);
  if (off_cursor) *off_cursor = off;
  off += align_up((size_t)K * sizeof(int), 256);
  if (off_total) *off_total = off;
  off += K > VQ_EMA_LDS_BINS ? 512 : 256;            // total int [64] (+ the large scan's block sums int [64])
  if (off_order) *off_order = off;
  off += align_up((size_t)std::max<long long>(N, 1) * sizeof(int), 256);
  return off;
}

extern "C" size_t smt_vq_ema_accumulate_workspace_bytes(int64_t n_rows, int k_bins, int dim) {
  return vq_ema_ws_layout(n_rows, k_bins, dim, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int smt_vq_ema_accumulate(const float* x, const int64_t* idx, const float* row_mask, int64_t n_rows, int k_bins,
                                     int dim, float* stats, void* workspace, size_t workspace_bytes, smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SMT_CHECK_ARG(stats && workspace && (n_rows == 0 || (x && idx)), "smt_vq_ema_accumulate: null pointer");
  SMT_CHECK_ARG(dim == 64 || dim == 128 || dim == 32, "smt_vq_ema_accumulate: dim must be 32, 64 or 128 (got %d)", dim);
  SMT_CHECK_ARG(n_rows >= 0 && n_rows < (1ll << 31), "smt_vq_ema_accumulate: n_rows must be in [0, 2^31) (got %lld)", (long long)n_rows);
  SMT_CHECK_ARG(k_bins >= 1 && k_bins <= VQ_EMA_MAX_BINS, "smt_vq_ema_accumulate: k_bins must be in [1, %d] (got %d)", VQ_EMA_MAX_BINS, k_bins);
  size_t o_counts, o_cursor, o_total, o_order;
  SMT_CHECK_ARG(workspace_bytes >= vq_ema_ws_layout(n_rows, k_bins, dim, &o_counts, &o_cursor, &o_total, &o_order),
                "smt_vq_ema_accumulate: workspace too small");
  const int n_sums = k_bins * dim, n_total = n_sums + k_bins;
  unsigned long long* acc = (unsigned long long*)workspace;
  int* counts = (int*)((char*)workspace + o_counts);
  int* cursor = (int*)((char*)workspace + o_cursor);
  int* total = (int*)((char*)workspace + o_total);
  int* order = (int*)((char*)workspace + o_order);
  (void)hipMemsetAsync(workspace, 0, o_order, stream);                // accumulators, counts, cursors, total
  if (n_rows > 0 && k_bins > VQ_EMA_LDS_BINS) {
    const unsigned rgrid = (unsigned)((n_rows + 255) / 256), nb = (unsigned)((k_bins + VQ_EMA_SCAN_BLOCK - 1) / VQ_EMA_SCAN_BLOCK);
    int* bsum = total + 64;
    vq_ema_count_large_kernel<<<rgrid, 256, 0, stream>>>((const long long*)idx, row_mask, n_rows, k_bins, counts);
    SMT_CHECK_LAUNCH("vq_ema_count_large");
    vq_ema_blocksum_kernel<<<nb, 1024, 0, stream>>>(counts, k_bins, bsum);
    SMT_CHECK_LAUNCH("vq_ema_blocksum");
    vq_ema_scan_large_kernel<<<nb, 1024, 0, stream>>>(counts, k_bins, bsum, cursor, total);
    SMT_CHECK_LAUNCH("vq_ema_scan_large");
    vq_ema_scatter_large_kernel<<<rgrid, 256, 0, stream>>>((const long long*)idx, row_mask, n_rows, k_bins, cursor, order);
    SMT_CHECK_LAUNCH("vq_ema_scatter_large");
  } else if (n_rows > 0) {
    const int rows_per_wg = (int)std::max<long long>(VQ_EMA_HIST_NT, (n_rows + 255) / 256);
    const unsigned nwg = (unsigned)((n_rows + rows_per_wg - 1) / rows_per_wg);
    vq_ema_count_kernel<<<nwg, VQ_EMA_HIST_NT, (size_t)k_bins * sizeof(int), stream>>>((const long long*)idx, row_mask, n_rows, k_bins, rows_per_wg,
                                                                                      counts);
    SMT_CHECK_LAUNCH("vq_ema_count");
    vq_ema_scan_kernel<<<1, 1024, 0, stream>>>(counts, k_bins, cursor, total);
    SMT_CHECK_LAUNCH("vq_ema_scan");
    vq_ema_scatter_kernel<<<nwg, VQ_EMA_HIST_NT, 2 * (size_t)k_bins * sizeof(int), stream>>>((const long long*)idx, row_mask, n_rows, k_bins,
                                                                                          rows_per_wg, cursor, order);
    SMT_CHECK_LAUNCH("vq_ema_scatter");
  }
  if (n_rows > 0) {
    const long long waves = (n_rows + VQ_EMA_SHARE - 1) / VQ_EMA_SHARE;
    const unsigned grid = (unsigned)((waves + 3) / 4);
    if (dim == 128) vq_ema_accumulate_kernel<128><<<grid, 256, 0, stream>>>(x, (const long long*)idx, order, total, k_bins, acc);
    else if (dim == 64) vq_ema_accumulate_kernel<64><<<grid, 256, 0, stream>>>(x, (const long long*)idx, order, total, k_bins, acc);
    else vq_ema_accumulate_kernel<32><<<grid, 256, 0, stream>>>(x, (const long long*)idx, order, total, k_bins, acc);
    SMT_CHECK_LAUNCH("vq_ema_accumulate");
  }
  vq_ema_convert_kernel<<<(n_total + 255) / 256, 256, 0, stream>>>(acc, stats, n_sums, n_total);
  SMT_CHECK_LAUNCH("vq_ema_convert");
  return 0;
}

extern "C" int smt_vq_ema_apply(float* codebook, float* k_sum, float* k_elem, const float* stats, const float* k_rand,
                                float mu, float threshold, int k_bins, int dim, float* metrics, void* prep,
                                size_t prep_bytes, smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SMT_CHECK_ARG(codebook && k_sum && k_elem && stats && k_rand && metrics && prep, "smt_vq_ema_apply: null pointer");
  SMT_CHECK_ARG(dim == 32 || dim == 64 || dim == 128, "smt_vq_ema_apply: dim must be 32, 64 or 128 (got %d)", dim);
  SMT_CHECK_ARG(prep_bytes >= vq_prep_layout(k_bins, dim, nullptr, nullptr), "smt_vq_ema_apply: prep buffer too small");
  VqPrep pr;
  vq_prep_layout(k_bins, dim, prep, &pr);
  vq_ema_apply_kernel<<<pr.nparts, 256, 0, stream>>>(codebook, k_sum, k_elem, stats, k_rand, mu, threshold, k_bins, dim,
                                                     pr.part, pr.dkpart);
  SMT_CHECK_LAUNCH("vq_ema_apply");
  // the codebook has changed: refresh its centred split for the next forward in the same call
  return vq_finish_prepare(codebook, k_bins, dim, pr, stats + (size_t)k_bins * dim, k_elem, threshold, metrics, stream);
}
