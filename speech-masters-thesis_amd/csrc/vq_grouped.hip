// Text-conditioned grouped vector quantiser for gfx950: a codebook of G * L codes in which every row searches ONLY the
// L codes of its group (the text token its frame is aligned to).
//
// Replaces the quantiser of the reference's VQTTS (models/vqtts/bottleneck.py:27-60), which gathers k[x_id] -- an
// [N, L, D] tensor, 262 KB per row at L = 512, D = 128 -- before a bmm.  Here the gather does not exist in any form:
//   0. prepare    (only when the codebook changes) per GROUP: mean of its L codes, centred bf16-pair split of the codes,
//                 -|k~|^2/2, max |k~|^2 -- a persistent `prep` buffer, the grouped twin of smt_vq_prepare;
//   1. bucket     counting sort of the rows by group (G <= 256 bins: LDS histograms, one global atomic per (workgroup,
//                 group) -- the count / scan / scatter scheme of the EMA path);
//   2. vqg_search one workgroup per tile of 32 rows of ONE group sweeps that group's L codes on the matrix cores with the
//                 flat search's filter (vq_common.h: 3 x v_mfma_f32_32x32x16_bf16 per k-step, LDS-DMA staging, the same
//                 rigorous round-off bound, evaluated with the GROUP's centred norms); rows whose best / runner-up gap
//                 clears the bound are finished in the same kernel, the others are queued;
//   3. vqg_exact  queued rows: all L codes of the row's group in fp64, index order, lowest index on ties (L <= 1024, so
//                 the flat path's candidate collection is not worth its launch here);
//   4. vq_reduce  the flat path's fixed-order sums.
// Index semantics are those of vq.hip: q_rel = the exact argmin over the group's codes on the fp32 inputs.
// Workspace is O(N); the derived data O(G L D).
#include <algorithm>

#include "vq_common.h"

namespace smt {

constexpr int VQG_MAX_GROUPS = 256;
constexpr int VQG_TILE = 32;            // rows per workgroup of the search: one MFMA column group
constexpr int VQG_SUP = VQ_CSUP;        // codes staged per step: one 32-code chunk for each of the two waves
constexpr int VQG_MAX_ROWS = 1 << 20;

// ---------------------------------------------------------------- prepare ---
struct VqgPrep {
  float* mu;          // [G][D]      mean of the group's L codes
  float* nkhalf;      // [G][Lpad]   -0.5 |k~_j|^2, -3e38 for the padding codes j >= L
  unsigned* kmax2;    // [G]         max_j |k~_j|^2 of the group (float bits)
  __bf16* kh;         // [G][Lpad][D] high halves of k~ = k - mu_g (zero rows for padding), chunk-swizzled (vq_swz)
  __bf16* kl;         // [G][Lpad][D] low halves
  float* part;        // [G L / VQ_PART][D] partial column sums (a group's parts are contiguous: L is a multiple of 32)
  double* dkpart;     // [G L / VQ_PART]    partial sums of (k_new - k_old)^2 (EMA apply)
  int lpad, nparts;
};
static size_t vqg_prep_layout(int G, int L, int D, void* base, VqgPrep* w) {
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return (char*)base + o; };
  const int lpad = (L + VQG_SUP - 1) / VQG_SUP * VQG_SUP, nparts = G * (L / VQ_PART);
  char* p;
  p = take((size_t)G * D * 4);             if (w) w->mu = (float*)p;
  p = take((size_t)G * lpad * 4);          if (w) w->nkhalf = (float*)p;
  p = take((size_t)G * 4);                 if (w) w->kmax2 = (unsigned*)p;
  p = take((size_t)G * lpad * D * 2);      if (w) w->kh = (__bf16*)p;
  p = take((size_t)G * lpad * D * 2);      if (w) w->kl = (__bf16*)p;
  p = take((size_t)nparts * D * 4);        if (w) w->part = (float*)p;
  p = take((size_t)nparts * 8);            if (w) w->dkpart = (double*)p;
  if (w) { w->lpad = lpad; w->nparts = nparts; }
  return off;
}

// mu[g] from the group's L / VQ_PART partial column sums, index order; one workgroup per group
__global__ __launch_bounds__(128) void vqg_mu_kernel(const float* __restrict__ part, int L, int D, float* __restrict__ mu,
                                                     unsigned* __restrict__ kmax2_bits) {
  const int g = blockIdx.x, np = L / VQ_PART;
  if (threadIdx.x == 0) kmax2_bits[g] = 0u;
  if ((int)threadIdx.x >= D) return;
  float t = 0.f;
#pragma unroll 16
  for (int p = 0; p < np; ++p) t += part[((size_t)g * np + p) * D + threadIdx.x];
  mu[(size_t)g * D + threadIdx.x] = t / (float)L;
}

// The grouped twin of vq_split_kernel: one wave per padded code, 16 codes (all of one group: Lpad is a multiple of 64)
// per workgroup; the swizzle runs on the index inside the group.
__global__ __launch_bounds__(1024) void vqg_split_kernel(const float* __restrict__ cb, const float* __restrict__ mu, int L, int Lpad,
                                                         int D, __bf16* __restrict__ kh, __bf16* __restrict__ kl,
                                                         float* __restrict__ nkhalf, unsigned* __restrict__ kmax2_bits) {
  __shared__ float wmax[16];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int pcode = blockIdx.x * 16 + wave;                 // < G * Lpad: the grid is exact
  const int g = pcode / Lpad, j = pcode % Lpad;
  const int sw = vq_swz(j, D);
  float s = 0.f;
  for (int i = lane; i < D; i += 64) {
    const float v = j < L ? cb[((size_t)g * L + j) * D + i] - mu[(size_t)g * D + i] : 0.f;
    const __bf16 hi = (__bf16)v;
    const size_t o = (size_t)pcode * D + 8 * ((i >> 3) ^ sw) + (i & 7);
    kh[o] = hi;
    kl[o] = (__bf16)(v - (float)hi);
    s = fmaf(v, v, s);
  }
  s = wave_sum(s);
  if (lane == 0) { nkhalf[pcode] = j < L ? -0.5f * s : -3.0e38f; wmax[wave] = s; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = 0.f;
    for (int w = 0; w < 16; ++w) m = fmaxf(m, wmax[w]);
    atomicMax(kmax2_bits + g, __float_as_uint(m));          // m >= 0: uint order == float order
  }
}

__global__ __launch_bounds__(1024) void vqg_metrics_kernel(const float* __restrict__ cnt, const float* __restrict__ k_elem,
                                                           const double* __restrict__ dkpart, int nparts, int K, int D,
                                                           float threshold, float* __restrict__ metrics) {
  vq_update_metrics(cnt, k_elem, dkpart, nparts, K, D, threshold, metrics);
}

static int vqg_finish_prepare(const float* cb, int G, int L, int D, const VqgPrep& pr, hipStream_t stream) {
  vqg_mu_kernel<<<G, 128, 0, stream>>>(pr.part, L, D, pr.mu, pr.kmax2);
  SMT_CHECK_LAUNCH("vqg_mu");
  vqg_split_kernel<<<G * pr.lpad / 16, 1024, 0, stream>>>(cb, pr.mu, L, pr.lpad, D, pr.kh, pr.kl, pr.nkhalf, pr.kmax2);
  SMT_CHECK_LAUNCH("vqg_split");
  return 0;
}

// ---------------------------------------------------------------- groups ----
// group[b, j] = x_id[b, idx[b, j]], mask = 1 where frame j has a token (idx >= 0), else group 0, mask 0 -- what the
// reference's matmul(x_id, attn) gives (bottleneck.py:24-28).  Ids are clamped into [0, G): the host checks them.
__global__ __launch_bounds__(256) void vqg_align_groups_kernel(const long long* __restrict__ x_id, const int* __restrict__ idx,
                                                               long long total, int t_x, int t_y, int G,
                                                               int* __restrict__ group, float* __restrict__ row_mask) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int i = idx[e];
  const bool live = i >= 0 && i < t_x;
  const long long tok = live ? x_id[(e / t_y) * t_x + i] : 0;
  group[e] = tok < 0 ? 0 : tok >= G ? G - 1 : (int)tok;
  row_mask[e] = live ? 1.f : 0.f;
}

// ---------------------------------------------------------------- bucket ----
__device__ __forceinline__ int vqg_group_of(const int* __restrict__ group, long long r, int G) { return min(max(group[r], 0), G - 1); }

constexpr int VQG_SORT_NT = 1024;
__global__ __launch_bounds__(VQG_SORT_NT) void vqg_count_kernel(const int* __restrict__ group, long long N, int G, int rows_per_wg,
                                                                int* __restrict__ counts) {
  __shared__ int hist[VQG_MAX_GROUPS];
  if (threadIdx.x < VQG_MAX_GROUPS) hist[threadIdx.x] = 0;
  __syncthreads();
  const long long r0 = (long long)blockIdx.x * rows_per_wg, r1 = min(N, r0 + rows_per_wg);
  for (long long r = r0 + threadIdx.x; r < r1; r += VQG_SORT_NT) atomicAdd(&hist[vqg_group_of(group, r, G)], 1);
  __syncthreads();
  if (threadIdx.x < VQG_MAX_GROUPS && hist[threadIdx.x]) atomicAdd(&counts[threadIdx.x], hist[threadIdx.x]);
}
// goff[g] = first sorted position of group g, toff[g] = its first tile (exclusive scans; entry VQG_MAX_GROUPS = totals);
// cursor = goff for the scatter.  One workgroup.
__global__ __launch_bounds__(VQG_MAX_GROUPS) void vqg_scan_kernel(const int* __restrict__ counts, int* __restrict__ cursor,
                                                                 int* __restrict__ goff, int* __restrict__ toff) {
  __shared__ int rs[VQG_MAX_GROUPS], ts[VQG_MAX_GROUPS];
  const int t = threadIdx.x, c = counts[t], nt = (c + VQG_TILE - 1) / VQG_TILE;   // counts beyond G are zero
  rs[t] = c; ts[t] = nt;
  __syncthreads();
  for (int off = 1; off < VQG_MAX_GROUPS; off <<= 1) {
    const int a = t >= off ? rs[t - off] : 0, b = t >= off ? ts[t - off] : 0;
    __syncthreads();
    rs[t] += a; ts[t] += b;
    __syncthreads();
  }
  goff[t] = rs[t] - c; toff[t] = ts[t] - nt; cursor[t] = rs[t] - c;
  if (t == VQG_MAX_GROUPS - 1) { goff[VQG_MAX_GROUPS] = rs[t]; toff[VQG_MAX_GROUPS] = ts[t]; }
}
__global__ __launch_bounds__(VQG_SORT_NT) void vqg_scatter_kernel(const int* __restrict__ group, long long N, int G, int rows_per_wg,
                                                                  int* __restrict__ cursor, int* __restrict__ order) {
  __shared__ int hist[VQG_MAX_GROUPS], base[VQG_MAX_GROUPS];
  if (threadIdx.x < VQG_MAX_GROUPS) hist[threadIdx.x] = 0;
  __syncthreads();
  const long long r0 = (long long)blockIdx.x * rows_per_wg, r1 = min(N, r0 + rows_per_wg);
  for (long long r = r0 + threadIdx.x; r < r1; r += VQG_SORT_NT) atomicAdd(&hist[vqg_group_of(group, r, G)], 1);
  __syncthreads();
  if (threadIdx.x < VQG_MAX_GROUPS) {
    base[threadIdx.x] = hist[threadIdx.x] ? atomicAdd(&cursor[threadIdx.x], hist[threadIdx.x]) : 0;
    hist[threadIdx.x] = 0;
  }
  __syncthreads();
  for (long long r = r0 + threadIdx.x; r < r1; r += VQG_SORT_NT) {
    const int g = vqg_group_of(group, r, G);
    order[base[g] + atomicAdd(&hist[g], 1)] = (int)r;       // the order inside a group varies; no result depends on it
  }
}

// ---------------------------------------------------------------- search ----
// Two waves, 32 rows of one group: wave c takes chunk c of every staged 64-code step (the shape of vq_candidates_kernel),
// double buffered; every lane owns one row and sees 16 codes per chunk in its accumulator, so best / runner-up are
// in-lane work.  The grid is the upper bound ceil(N / 32) + G tiles; a workgroup finds its group by bisection of toff.
template <int D>
__global__ __launch_bounds__(128) void vqg_search_kernel(const float* __restrict__ x, const float* __restrict__ cb,
                                                         const float* __restrict__ row_mask, const float* __restrict__ mu,
                                                         const float* __restrict__ nkhalf, const unsigned* __restrict__ kmax2_bits,
                                                         const __bf16* __restrict__ kh, const __bf16* __restrict__ kl,
                                                         const int* __restrict__ order, const int* __restrict__ goff,
                                                         const int* __restrict__ toff, int L, int Lpad,
                                                         long long* __restrict__ q_rel, long long* __restrict__ q_abs,
                                                         float* __restrict__ min_dist, float* __restrict__ x_d,
                                                         unsigned* __restrict__ ctl, int* __restrict__ q_rows) {
  constexpr int SUP = VQG_SUP;
  using G = VqGeom<D, SUP>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* m_best = reinterpret_cast<float*>(smem + 2 * G::BUF_BYTES);      // all LDS in the dynamic region: its base stays 16-byte aligned
  float* m_second = m_best + VQG_TILE;
  int* m_idx = reinterpret_cast<int*>(m_second + VQG_TILE);
  int* m_row = m_idx + VQG_TILE;
  const int tile = blockIdx.x;
  if (tile >= toff[VQG_MAX_GROUPS]) return;                 // workgroup-uniform
  int lo = 0, hi = VQG_MAX_GROUPS;                          // the group g with toff[g] <= tile < toff[g + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (toff[mid] <= tile) lo = mid; else hi = mid;
  }
  const int g = lo;
  const int pos0 = goff[g] + (tile - toff[g]) * VQG_TILE, nrows = min(VQG_TILE, goff[g + 1] - pos0);   // >= 1
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  const __bf16* gkh = kh + (size_t)g * Lpad * D;
  const __bf16* gkl = kl + (size_t)g * Lpad * D;
  const float* gnk = nkhalf + (size_t)g * Lpad;
  const float* gcb = cb + (size_t)g * L * D;

  vq_stage<D, SUP>(gkh, gkl, gnk, 0, smem, 2, wave, lane);
  const long long my_row = order[pos0 + min(j, nrows - 1)];  // lanes past the end repeat the last row and are never written
  vq_bf16x8 xh[1][G::NS], xl[1][G::NS];
  float xx = vq_load_row<D>(x, mu + (size_t)g * D, my_row, h, xh[0], xl[0]);
  xx += __shfl_xor(xx, 32, 64);
  vm_wait<0>();
  __syncthreads();

  float best = -INFINITY, second = -INFINITY;
  int bidx = 0x7fffffff;
  const int nsc = Lpad / SUP;
  for (int i = 0; i < nsc; ++i) {
    const int buf = i & 1;
    if (i + 1 < nsc) vq_stage<D, SUP>(gkh, gkl, gnk, i + 1, smem + (buf ^ 1) * G::BUF_BYTES, 2, wave, lane);
    f32x16 acc[1];
    vq_chunk_scores<D, SUP, 1>(smem + buf * G::BUF_BYTES, wave, j, h, xh, xl, acc);
    const int cbase = i * SUP + wave * VQ_CHUNK + 4 * h;
#pragma unroll
    for (int r = 0; r < 16; ++r) {                          // codes in increasing order: '>' keeps the lowest index
      const float t = acc[0][r];
      if (t > best) { second = best; best = t; bidx = cbase + 8 * (r >> 2) + (r & 3); }
      else second = fmaxf(second, t);
    }
    vm_wait<0>();
    __syncthreads();
  }
  {  // the two lane halves of a row (same row, disjoint codes), then the two chunk waves
    const float ob = __shfl_xor(best, 32, 64), os = __shfl_xor(second, 32, 64);
    const int oi = __shfl_xor(bidx, 32, 64);
    vq_merge(best, second, bidx, ob, os, oi);
  }
  if (wave == 1 && h == 0) { m_best[j] = best; m_second[j] = second; m_idx[j] = bidx; }
  __syncthreads();
  if (wave == 0 && h == 0) {
    vq_merge(best, second, bidx, m_best[j], m_second[j], m_idx[j]);
    const float err = vq_filter_err(xx, __uint_as_float(kmax2_bits[g]), D);
    const bool ambiguous = !((best - second) > 2.0f * err) || bidx >= L;   // also catches NaN / inf
    if (j < nrows && ambiguous) q_rows[atomicAdd(reinterpret_cast<int*>(ctl + 32), 1)] = (int)my_row;
    m_idx[j] = (ambiguous || j >= nrows) ? -1 : bidx;       // -1: nothing to finish here (queued, or past the tile's end)
    m_row[j] = j < nrows ? (int)my_row : -1;
  }
  __syncthreads();
  // finish the unambiguous rows: indices, min_dist = |x - k|^2 (fp32 direct form), x_d = k * mask
  constexpr int RPW = 16, LPR = D / 4, RPI = 64 / LPR, NIT = RPW / RPI, BATCH = NIT < 4 ? NIT : 4;
  const int c4 = lane % LPR;
#pragma unroll 1
  for (int it0 = 0; it0 < NIT; it0 += BATCH) {
    f32x4 xv[BATCH], kv[BATCH];
    int code[BATCH];
    long long rows[BATCH];
#pragma unroll
    for (int q = 0; q < BATCH; ++q) {
      const int r = RPW * wave + (it0 + q) * RPI + lane / LPR;
      rows[q] = m_row[r];
      code[q] = m_idx[r];
      xv[q] = *reinterpret_cast<const f32x4*>(x + max(rows[q], 0ll) * D + 4 * c4);
      kv[q] = *reinterpret_cast<const f32x4*>(gcb + (size_t)max(code[q], 0) * D + 4 * c4);
    }
#pragma unroll
    for (int q = 0; q < BATCH; ++q) {
      const f32x4 df = xv[q] - kv[q];
      float ds = fmaf(df.w, df.w, fmaf(df.z, df.z, fmaf(df.y, df.y, df.x * df.x)));
#pragma unroll
      for (int o = LPR / 2; o > 0; o >>= 1) ds += __shfl_xor(ds, o, 64);
      if (rows[q] >= 0 && code[q] >= 0) {
        if (x_d) {
          const float m = row_mask ? row_mask[rows[q]] : 1.f;
          *reinterpret_cast<f32x4*>(x_d + rows[q] * D + 4 * c4) = kv[q] * m;
        }
        if (c4 == 0) {
          q_rel[rows[q]] = code[q];
          q_abs[rows[q]] = (long long)g * L + code[q];
          min_dist[rows[q]] = ds;
        }
      }
    }
  }
}

// ---------------------------------------------------------------- exact -----
// Half a wave per queued row: all L codes of the row's group in fp64 (vq_exact_dist: the oracle's arithmetic), lane l
// takes codes l, l + 32, ... in increasing order; lowest index among equal distances.
__global__ __launch_bounds__(256) void vqg_exact_kernel(const float* __restrict__ x, const int* __restrict__ group,
                                                        const float* __restrict__ cb, const float* __restrict__ row_mask,
                                                        const unsigned* __restrict__ ctl, int G, int L, int D,
                                                        const int* __restrict__ q_rows, long long* __restrict__ q_rel,
                                                        long long* __restrict__ q_abs, float* __restrict__ min_dist,
                                                        float* __restrict__ x_d) {
  const int n_q = (int)ctl[32];
  const int lane = threadIdx.x & 63, half = lane >> 5, l = lane & 31;
  const int hw0 = (((int)blockIdx.x * 256 + (int)threadIdx.x) >> 6) * 2, nhw = (int)gridDim.x * 8;
  for (int q0 = hw0; q0 < n_q; q0 += nhw) {                  // wave-uniform trip count; the second half may idle
    const int qi = q0 + half;
    const bool rvalid = qi < n_q;
    const long long row = rvalid ? q_rows[qi] : 0;
    const int g = rvalid ? vqg_group_of(group, row, G) : 0;
    const float* xr = x + row * D;
    const float* gcb = cb + (size_t)g * L * D;
    double d = INFINITY;
    int code = 0x7fffffff;
    if (rvalid) {
      for (int c0 = l; c0 < L; c0 += 32) {
        const double dc = vq_exact_dist(xr, gcb + (size_t)c0 * D, D);
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
    const bool found = code != 0x7fffffff;                   // false on a NaN row: keep the outputs defined
    const int cc = found ? code : 0;
    if (x_d) {
      const float m = row_mask ? row_mask[row] : 1.f;
      for (int i = l; i < D; i += 32) x_d[row * D + i] = gcb[(size_t)cc * D + i] * m;
    }
    if (l == 0) {
      q_rel[row] = cc;
      q_abs[row] = (long long)g * L + cc;
      min_dist[row] = found ? (float)d : __builtin_nanf("");  // the exact distance, rounded once
    }
  }
}

// workspace: ctl u32 [64] (ctl[32] = queued rows) | counts int [256] | cursor int [256] | goff int [257 -> 320] |
//            toff int [320] | order int [N] | q_rows int [N]
struct VqgWorkspace { unsigned* ctl; int *counts, *cursor, *goff, *toff, *order, *q_rows; size_t zero_bytes; };
static size_t vqg_layout(long long N, void* base, VqgWorkspace* w) {
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return (char*)base + o; };
  const size_t n = (size_t)std::max<long long>(N, 1);
  char* p;
  p = take(256);                       if (w) w->ctl = (unsigned*)p;
  p = take(VQG_MAX_GROUPS * 4);        if (w) w->counts = (int*)p;
  p = take(VQG_MAX_GROUPS * 4);        if (w) w->cursor = (int*)p;
  if (w) w->zero_bytes = off;
  p = take(320 * 4);                   if (w) w->goff = (int*)p;
  p = take(320 * 4);                   if (w) w->toff = (int*)p;
  p = take(n * 4);                     if (w) w->order = (int*)p;
  p = take(n * 4);                     if (w) w->q_rows = (int*)p;
  return off;
}

template <int D>
static int vqg_launch_search(const float* x, const int* group, const float* cb, const float* row_mask, const VqgPrep& pr,
                             long long N, int G, int L, long long* q_rel, long long* q_abs, float* min_dist, float* x_d,
                             const VqgWorkspace& w, hipStream_t stream) {
  using GS = VqGeom<D, VQG_SUP>;
  const int lds = 2 * GS::BUF_BYTES + 4 * VQG_TILE * 4;                      // two staging buffers + the per-row merge arrays
  (void)hipFuncSetAttribute((const void*)vqg_search_kernel<D>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  const unsigned tiles = (unsigned)((N + VQG_TILE - 1) / VQG_TILE + G);      // upper bound: one partial tile per group
  vqg_search_kernel<D><<<tiles, 128, lds, stream>>>(x, cb, row_mask, pr.mu, pr.nkhalf, pr.kmax2, pr.kh, pr.kl,
                                                                  w.order, w.goff, w.toff, L, pr.lpad, q_rel, q_abs,
                                                                  min_dist, x_d, w.ctl, w.q_rows);
  SMT_CHECK_LAUNCH("vqg_search");
  vqg_exact_kernel<<<(unsigned)std::min<long long>(256, (N + 7) / 8), 256, 0, stream>>>(x, group, cb, row_mask, w.ctl, G, L, D,
                                                                                      w.q_rows, q_rel, q_abs, min_dist, x_d);
  SMT_CHECK_LAUNCH("vqg_exact");
  return 0;
}

static bool vqg_shape_ok(int G, int L, int D) {
  return (D == 32 || D == 64 || D == 128) && L >= 32 && L <= 1024 && L % 32 == 0 && G >= 1 && G <= VQG_MAX_GROUPS;
}

}  // namespace smt

using namespace smt;

#define VQG_CHECK_SHAPE(fn)                                                                                            \
  do {                                                                                                                 \
    SMT_CHECK_ARG(dim == 32 || dim == 64 || dim == 128, fn ": dim must be 32, 64 or 128 (got %d)", dim);               \
    SMT_CHECK_ARG(l_bins >= 32 && l_bins <= 1024 && l_bins % 32 == 0,                                                   \
                  fn ": l_bins must be a multiple of 32 in [32, 1024] (got %d)", l_bins);                               \
    SMT_CHECK_ARG(n_groups >= 1 && n_groups <= VQG_MAX_GROUPS, fn ": n_groups must be in [1, %d] (got %d)",             \
                  VQG_MAX_GROUPS, n_groups);                                                                            \
  } while (0)

extern "C" size_t smt_vq_grouped_prep_bytes(int n_groups, int l_bins, int dim) {
  if (!vqg_shape_ok(n_groups, l_bins, dim)) return 0;
  return vqg_prep_layout(n_groups, l_bins, dim, nullptr, nullptr);
}

extern "C" int smt_vq_grouped_prepare(const float* codebook, int n_groups, int l_bins, int dim, void* prep, size_t prep_bytes,
                                      smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VQG_CHECK_SHAPE("smt_vq_grouped_prepare");
  SMT_CHECK_ARG(codebook && prep, "smt_vq_grouped_prepare: null pointer");
  SMT_CHECK_ARG(prep_bytes >= vqg_prep_layout(n_groups, l_bins, dim, nullptr, nullptr), "smt_vq_grouped_prepare: prep buffer too small");
  VqgPrep pr;
  vqg_prep_layout(n_groups, l_bins, dim, prep, &pr);
  vq_colsum_kernel<<<pr.nparts, 128, 0, stream>>>(codebook, n_groups * l_bins, dim, pr.part);
  SMT_CHECK_LAUNCH("vq_colsum");
  return vqg_finish_prepare(codebook, n_groups, l_bins, dim, pr, stream);
}

extern "C" int smt_vq_align_groups(const int64_t* x_id, const int* align_idx, int batch, int t_x, int t_y, int n_groups,
                                   int* group, float* row_mask, smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SMT_CHECK_ARG(batch >= 0 && t_x >= 1 && t_y >= 0, "smt_vq_align_groups: bad sizes batch=%d t_x=%d t_y=%d", batch, t_x, t_y);
  SMT_CHECK_ARG(n_groups >= 1 && n_groups <= VQG_MAX_GROUPS, "smt_vq_align_groups: n_groups must be in [1, %d] (got %d)",
                VQG_MAX_GROUPS, n_groups);
  const long long total = (long long)batch * t_y;
  if (total == 0) return 0;
  SMT_CHECK_ARG(total < (1ll << 31), "smt_vq_align_groups: batch * t_y must be < 2^31");
  SMT_CHECK_ARG(x_id && align_idx && group && row_mask, "smt_vq_align_groups: null pointer");
  vqg_align_groups_kernel<<<(unsigned)((total + 255) / 256), 256, 0, stream>>>((const long long*)x_id, align_idx, total, t_x, t_y,
                                                                              n_groups, group, row_mask);
  SMT_CHECK_LAUNCH("vqg_align_groups");
  return 0;
}

extern "C" size_t smt_vq_grouped_forward_workspace_bytes(int64_t n_rows) { return vqg_layout(n_rows, nullptr, nullptr); }

extern "C" int smt_vq_grouped_forward(const float* x, const int* group, const float* codebook, void* prep, const float* row_mask,
                                      int64_t n_rows, int n_groups, int l_bins, int dim, int64_t* q_rel, int64_t* q_abs,
                                      float* min_dist, float* x_d, float* sums, void* workspace, size_t workspace_bytes,
                                      smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VQG_CHECK_SHAPE("smt_vq_grouped_forward");
  SMT_CHECK_ARG(n_rows >= 0 && n_rows <= VQG_MAX_ROWS, "smt_vq_grouped_forward: n_rows must be in [0, %d] (got %lld)", VQG_MAX_ROWS,
                (long long)n_rows);
  SMT_CHECK_ARG(codebook && prep && sums && workspace, "smt_vq_grouped_forward: null pointer");
  SMT_CHECK_ARG(n_rows == 0 || (x && group && q_rel && q_abs && min_dist), "smt_vq_grouped_forward: null pointer");
  SMT_CHECK_ARG(workspace_bytes >= vqg_layout(n_rows, nullptr, nullptr), "smt_vq_grouped_forward: workspace too small");
  if (n_rows == 0) {
    (void)hipMemsetAsync(sums, 0, 16, stream);
    return 0;
  }
  VqgWorkspace w;
  vqg_layout(n_rows, workspace, &w);
  VqgPrep pr;
  vqg_prep_layout(n_groups, l_bins, dim, prep, &pr);
  (void)hipMemsetAsync(workspace, 0, w.zero_bytes, stream);           // queue counter, counts, cursors
  const int rows_per_wg = (int)std::max<long long>(VQG_SORT_NT, (n_rows + 255) / 256);
  const unsigned nwg = (unsigned)((n_rows + rows_per_wg - 1) / rows_per_wg);
  vqg_count_kernel<<<nwg, VQG_SORT_NT, 0, stream>>>(group, n_rows, n_groups, rows_per_wg, w.counts);
  SMT_CHECK_LAUNCH("vqg_count");
  vqg_scan_kernel<<<1, VQG_MAX_GROUPS, 0, stream>>>(w.counts, w.cursor, w.goff, w.toff);
  SMT_CHECK_LAUNCH("vqg_scan");
  vqg_scatter_kernel<<<nwg, VQG_SORT_NT, 0, stream>>>(group, n_rows, n_groups, rows_per_wg, w.cursor, w.order);
  SMT_CHECK_LAUNCH("vqg_scatter");
  int rc;
  if (dim == 128) rc = vqg_launch_search<128>(x, group, codebook, row_mask, pr, n_rows, n_groups, l_bins, (long long*)q_rel, (long long*)q_abs, min_dist, x_d, w, stream);
  else if (dim == 64) rc = vqg_launch_search<64>(x, group, codebook, row_mask, pr, n_rows, n_groups, l_bins, (long long*)q_rel, (long long*)q_abs, min_dist, x_d, w, stream);
  else rc = vqg_launch_search<32>(x, group, codebook, row_mask, pr, n_rows, n_groups, l_bins, (long long*)q_rel, (long long*)q_abs, min_dist, x_d, w, stream);
  if (rc) return rc;
  vq_reduce_kernel<<<1, 1024, 0, stream>>>(min_dist, row_mask, n_rows, w.ctl, sums);
  SMT_CHECK_LAUNCH("vq_reduce");
  return 0;
}

extern "C" int smt_vq_grouped_ema_apply(float* codebook, float* k_sum, float* k_elem, const float* stats, const float* k_rand,
                                        float mu, float threshold, int n_groups, int l_bins, int dim, float* metrics, void* prep,
                                        size_t prep_bytes, smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  VQG_CHECK_SHAPE("smt_vq_grouped_ema_apply");
  SMT_CHECK_ARG(codebook && k_sum && k_elem && stats && k_rand && metrics && prep, "smt_vq_grouped_ema_apply: null pointer");
  SMT_CHECK_ARG(prep_bytes >= vqg_prep_layout(n_groups, l_bins, dim, nullptr, nullptr), "smt_vq_grouped_ema_apply: prep buffer too small");
  VqgPrep pr;
  vqg_prep_layout(n_groups, l_bins, dim, prep, &pr);
  const int K = n_groups * l_bins;
  vq_ema_apply_kernel<<<pr.nparts, 256, 0, stream>>>(codebook, k_sum, k_elem, stats, k_rand, mu, threshold, K, dim, pr.part, pr.dkpart);
  SMT_CHECK_LAUNCH("vq_ema_apply");
  vqg_metrics_kernel<<<1, 1024, 0, stream>>>(stats + (size_t)K * dim, k_elem, pr.dkpart, pr.nparts, K, dim, threshold, metrics);
  SMT_CHECK_LAUNCH("vqg_metrics");
  return vqg_finish_prepare(codebook, n_groups, l_bins, dim, pr, stream);   // the codebook has changed: refresh its split
}
