// Device functions shared by the flat (vq.hip) and the grouped (vq_grouped.hip) nearest-code search: the bf16-pair MFMA
// filter with its round-off bound, the LDS-DMA staging of the split codebook, the fp64 distance of the exact re-scoring,
// and the kernels both paths launch as they are (`static`: one copy per translation unit): the fixed-order reduction of the
// per-row distances, the partial column sums, the EMA mix + revival and the metrics of update_k.
#pragma once
#include "conv_common.h"

#ifndef VQ_ABL
#define VQ_ABL 0      // timing experiments (tools/ablate_vq.sh, results invalid): 1 no MFMAs, 2 no re-staging of the codebook,
#endif                // 4 no best/runner-up folding, 8 no epilogue, 16 phase timestamps (tools/vq_phases.py), 32 no fragment reads

namespace smt {

constexpr int VQ_MAXRG = 5;           // 32-row MFMA column groups per workgroup of the search kernel (two waves each)
constexpr int VQ_SSUP = 128;          // codes staged per step of the search kernel: two 32-code chunks per wave
constexpr int VQ_CSUP = 64;           // ... of the candidates kernel: one chunk for each of its two waves
constexpr int VQ_KPAD = 256;          // the prep pads the codebook to a multiple of this (two search steps)
constexpr int VQ_CHUNK = 32;
constexpr int VQ_SPLITS = 8;          // code-range splits of the candidate sweep (one workgroup each)
constexpr int VQ_CAPS = 4;            // candidate codes kept per queued row and split
constexpr int VQ_PART = 8;            // codes per partial column sum (prepare)

typedef __bf16 vq_bf16x8 __attribute__((ext_vector_type(8)));

// Position of dim i of code j inside its [D] row of the kh / kl tiles: rows are NOT padded (they are copied to LDS by
// linear LDS-DMA), so the 16-byte chunk index is XORed with the row index instead -- the 32 lanes of an MFMA A-fragment
// read (32 consecutive codes, same chunk) then fall into 16 different 16-byte bank groups.
__host__ __device__ __forceinline__ int vq_swz(int j, int D) { return (j / (128 / D)) & (D / 8 - 1); }

// ---------------------------------------------------------------- search ----
// The codebook is the MFMA A operand (code on the row index i), x the B operand (row on the column index j = lane & 31),
// so every lane owns ONE x row per column group and sees 16 codes per chunk in its accumulator registers: the running
// best / runner-up is pure in-lane work.  Each fp32 operand is split into a bf16 pair and x~.k~ is evaluated as
// kl.xh + kh.xl + kh.xh with fp32 accumulation on top of -|k~|^2/2 -- 3 bf16 MFMAs (16x the fp32-MFMA rate each)
// instead of 8 fp32 MFMAs.  The score is only a FILTER: its error bound (vq_filter_err) decides which rows are
// re-scored exactly, so the index semantics stay exact.
//
// Shape: 2 waves, 64 rows.  Each wave keeps BOTH 32-row column groups of the tile in registers (bf16 pairs of its
// share of the rows) and takes one of the two 32-code chunks of every staged 64-code step, so one A fragment read from
// LDS feeds 6 MFMAs and a workgroup stages the whole codebook exactly once for its 64 rows.  LDS: two stages of
// [hi | lo][64][D + 8] bf16 + 64 floats.
template <int D, int SUP> struct VqGeom {
  static constexpr int NS = D / 16;                       // k-steps per chunk
  static constexpr int TILE_BYTES = SUP * D * 2;          // one staged tile (hi or lo)
  static constexpr int NDMA = TILE_BYTES / 1024;          // 1-KiB LDS-DMA wave-instructions per tile
  static constexpr int BUF_BYTES = 2 * TILE_BYTES + SUP * 4;
};

__device__ __forceinline__ void vq_dma16(const void* gsrc, void* lds_dst_wave_base) {
  __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)gsrc,
                                   (void __attribute__((address_space(3)))*)lds_dst_wave_base, 16, 0, 0);
}
__device__ __forceinline__ void vq_dma4(const void* gsrc, void* lds_dst_wave_base) {
  __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)gsrc,
                                   (void __attribute__((address_space(3)))*)lds_dst_wave_base, 4, 0, 0);
}
// Stage step `sc` (SUP codes: hi tile, lo tile, -|k~|^2/2) into `buf` with LDS-DMA, no register round trip: the nw
// waves of the workgroup issue the 1-KiB pieces in turn.  The data has landed after every issuing wave's
// `s_waitcnt vmcnt(0)` + a barrier.
template <int D, int SUP>
__device__ __forceinline__ void vq_stage(const __bf16* kh, const __bf16* kl, const float* nkhalf, int sc, char* buf,
                                         int nw, int wave, int lane) {
  using G = VqGeom<D, SUP>;
  if ((VQ_ABL & 2) && sc > 1) return;
  for (int q = wave; q < 2 * G::NDMA; q += nw) {
    const int which = q / G::NDMA, piece = q % G::NDMA;
    const __bf16* src = (which ? kl : kh) + (size_t)sc * SUP * D + piece * 512 + lane * 8;
    vq_dma16(src, buf + which * G::TILE_BYTES + piece * 1024);
  }
  if (wave == nw - 1) {
#pragma unroll
    for (int i = 0; i < SUP / 64; ++i) vq_dma4(nkhalf + sc * SUP + 64 * i + lane, buf + 2 * G::TILE_BYTES + 256 * i);
  }
}

// this lane's share of row `row` (dims 16 s + 8 h .. + 7 for every k-step s), centred and split; returns its share of
// |x~|^2.  All loads are issued before the first use (callers pass a row index that is always in range).
template <int D>
__device__ __forceinline__ float vq_load_row(const float* __restrict__ x, const float* __restrict__ mu, long long row,
                                             int h, vq_bf16x8* xh, vq_bf16x8* xl) {
  constexpr int NS = D / 16, HB = NS < 4 ? NS : 4;           // k-steps per batch of loads (bounds the live registers)
  float xx = 0.f;
#pragma unroll
  for (int s0 = 0; s0 < NS; s0 += HB) {
    f32x4 v[HB][2], m[HB][2];
#pragma unroll
    for (int s = 0; s < HB; ++s) {
      const f32x4* src = reinterpret_cast<const f32x4*>(x + row * D + 16 * (s0 + s) + 8 * h);
      const f32x4* msrc = reinterpret_cast<const f32x4*>(mu + 16 * (s0 + s) + 8 * h);
      v[s][0] = src[0]; v[s][1] = src[1]; m[s][0] = msrc[0]; m[s][1] = msrc[1];
    }
#pragma unroll
    for (int s = 0; s < HB; ++s) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float c = v[s][e >> 2][e & 3] - m[s][e >> 2][e & 3];
        const __bf16 hi = (__bf16)c;
        xh[s0 + s][e] = hi;
        xl[s0 + s][e] = (__bf16)(c - (float)hi);
        xx = fmaf(c, c, xx);
      }
    }
  }
  return xx;
}

// Error of the filter score against the exact acc = x~.k~ - |k~|^2/2 on the centred operands (norms are the centred
// ones, Cauchy-Schwarz turns sums of products into norm products):
//   bf16-pair split, three of the four partial products kept:  <= 3.01 * 2^-18 |x~| |k~|
//   fp32 accumulation of 3D exact products + the initial term:  <= 1.05 (3D+2) 2^-24 (|x~||k~| + |k~|^2/2)
//   fp32 rounding of khalf and of the centring x - mu, k - mu:  <= 2^-24 ((D+2)|k~|^2/2 + (|x~| + |k~|)^2)
//   position tag in the 4 low mantissa bits of a score (vq_search_kernel):   <= 2^-19 (|x~||k~| + |k~|^2/2)
// with |k~| <= |k~|max; a factor 1.25 of slack covers the MFMA's internal summation order and the fp32 rounding of xx.
__device__ __forceinline__ float vq_filter_err(float xx, float kmax2, int D) {
  const float xk = sqrtf(xx * kmax2);
  const float u24 = 5.9604645e-8f;
  return 1.25f * (3.01f * 64.f * u24 * xk + (1.05f * (float)(3 * D + 2) + 32.f) * u24 * (xk + 0.5f * kmax2) +
                  u24 * (0.5f * (float)(D + 2) * kmax2 + xx + 2.f * xk + kmax2));
}

// One 32-code chunk against NG column groups: acc[g] = -|k~|^2/2 + sum_s (kl.xh + kh.xl + kh.xh), small terms first.
template <int D, int SUP, int NG>
__device__ __forceinline__ void vq_chunk_scores(const char* buf, int chunk, int j, int h, const vq_bf16x8 (*xh)[D / 16],
                                                const vq_bf16x8 (*xl)[D / 16], f32x16* acc) {
  using G = VqGeom<D, SUP>;
  constexpr int NS = D / 16;
  const float* nk = reinterpret_cast<const float*>(buf + 2 * G::TILE_BYTES) + chunk * VQ_CHUNK + 4 * h;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(nk + 8 * q);       // codes 8 q + 4 h + e of the chunk
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      acc[g][4 * q + 0] = v.x; acc[g][4 * q + 1] = v.y; acc[g][4 * q + 2] = v.z; acc[g][4 * q + 3] = v.w;
    }
  }
  const int rowi = chunk * VQ_CHUNK + j, sw = vq_swz(rowi, D);
  const char* ah = buf + rowi * (2 * D);
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int so = (VQ_ABL & 32) ? 0 : s;
    const vq_bf16x8 fh = *reinterpret_cast<const vq_bf16x8*>(ah + 16 * ((2 * so + h) ^ sw));
    const vq_bf16x8 fl = *reinterpret_cast<const vq_bf16x8*>(ah + G::TILE_BYTES + 16 * ((2 * so + h) ^ sw));
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if (!(VQ_ABL & 1)) {
        acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fl, xh[g][s], acc[g], 0, 0, 0);
        acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh, xl[g][s], acc[g], 0, 0, 0);
        acc[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh, xh[g][s], acc[g], 0, 0, 0);
      }
    }
  }
}

// top-2 merge of (best, second, idx) with another candidate triple; equal scores keep the lower index (the gap is then
// zero and the row is re-scored exactly anyway)
__device__ __forceinline__ void vq_merge(float& best, float& second, int& bidx, float ob, float os, int oi) {
  if (ob > best || (ob == best && oi < bidx)) {
    second = fmaxf(best, os); best = ob; bidx = oi;
  } else {
    second = fmaxf(second, ob);
  }
}

// ---------------------------------------------------------------- exact -----
// d_j = sum_i (x_i - k_ji)^2 in fp64, index order, no fma contraction (the numpy float64 loop of the oracle)
__device__ __forceinline__ double vq_exact_dist(const float* __restrict__ xr, const float* __restrict__ kr, int D) {
  double d = 0.0;
#pragma unroll 4
  for (int i = 0; i < D; i += 4) {
    const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + i), kv = *reinterpret_cast<const f32x4*>(kr + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double df = __dsub_rn((double)xv[e], (double)kv[e]);
      d = __dadd_rn(d, __dmul_rn(df, df));
    }
  }
  return d;
}

// ---------------------------------------------------------------- reduce ----
// Single workgroup, fixed order: sums[0] = sum_all min_dist, sums[1] = sum_masked, sums[2] = sum mask,
// sums[3] = rows that were re-scored exactly.  Resets the queue counter for the next forward.
static __global__ __launch_bounds__(1024) void vq_reduce_kernel(const float* __restrict__ min_dist,
                                                         const float* __restrict__ row_mask, long long N,
                                                         unsigned* __restrict__ kmax2_bits, float* __restrict__ sums) {
  __shared__ double sh[3][16];
  double a = 0.0, b = 0.0, c = 0.0;
  constexpr int U = 10;                                     // 16-byte loads in flight per thread: 40,960 rows per pass
  for (long long r0 = 4ll * threadIdx.x; r0 < N; r0 += 4096ll * U) {
    f32x4 d[U], m[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long r = r0 + 4096ll * u;
      const f32x4 z = {0.f, 0.f, 0.f, 0.f}, one = {1.f, 1.f, 1.f, 1.f};
      if (r + 3 < N) {
        d[u] = *reinterpret_cast<const f32x4*>(min_dist + r);
        m[u] = row_mask ? *reinterpret_cast<const f32x4*>(row_mask + r) : one;
      } else {
        d[u] = z; m[u] = z;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (r + e < N) { d[u][e] = min_dist[r + e]; m[u][e] = row_mask ? row_mask[r + e] : 1.f; }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) { a += d[u][e]; b += (m[u][e] != 0.f) ? d[u][e] : 0.f; c += m[u][e]; }
  }
  a = wave_sum_d(a); b = wave_sum_d(b); c = wave_sum_d(c);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { sh[0][wave] = a; sh[1][wave] = b; sh[2][wave] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double ta = 0, tb = 0, tc = 0;
    for (int w = 0; w < 16; ++w) { ta += sh[0][w]; tb += sh[1][w]; tc += sh[2][w]; }
    sums[0] = (float)ta; sums[1] = (float)tb; sums[2] = (float)tc; sums[3] = (float)kmax2_bits[32];
    kmax2_bits[32] = 0u;
  }
}

// part[p][i] = sum of k[j][i] over the codes j of part p (index order)
static __global__ __launch_bounds__(128) void vq_colsum_kernel(const float* __restrict__ cb, int K, int D, float* __restrict__ part) {
  const int i = threadIdx.x;
  if (i >= D) return;
  const int j0 = blockIdx.x * VQ_PART;
  float s = 0.f;
  for (int j = j0; j < min(K, j0 + VQ_PART); ++j) s += cb[(size_t)j * D + i];
  part[(size_t)blockIdx.x * D + i] = s;
}

// The metrics of update_k (bottleneck.py:85-90) from the batch counts `cnt`, the mixed `k_elem` and the partial sums of
// (k_new - k_old)^2 that vq_ema_apply_kernel left: every thread of a SINGLE workgroup calls it; all reductions in fixed order.
__device__ __forceinline__ void vq_update_metrics(const float* __restrict__ cnt, const float* __restrict__ k_elem,
                                                  const double* __restrict__ dkpart, int nparts, int K, int D, float threshold,
                                                  float* __restrict__ metrics) {
  __shared__ double sh[16];
  __shared__ double bc;
  auto block_sum = [&](double v) -> double {
    v = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0;
      for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += sh[w];
      bc = t;
    }
    __syncthreads();
    return bc;
  };
  double tot = 0.0;
  for (int j = threadIdx.x; j < K; j += blockDim.x) tot += cnt[j];
  const float total = (float)block_sum(tot);
  double ent = 0.0, used = 0.0, usage_n = 0.0, dk2 = 0.0;
  for (int j = threadIdx.x; j < K; j += blockDim.x) {
    const float c = cnt[j];
    const float prob = c / total;
    ent += -(double)(prob * logf(fmaxf(prob, 1e-5f)));
    used += (c >= threshold) ? 1.0 : 0.0;
    usage_n += (k_elem[j] >= threshold) ? 1.0 : 0.0;       // k_elem already holds the mixed value
  }
  for (int p = threadIdx.x; p < nparts; p += blockDim.x) dk2 += dkpart[p];
  ent = block_sum(ent);
  used = block_sum(used);
  usage_n = block_sum(usage_n);
  dk2 = block_sum(dk2);
  if (threadIdx.x == 0) {
    metrics[0] = (float)ent;
    metrics[1] = (float)used;
    metrics[2] = (float)usage_n;
    metrics[3] = (float)(sqrt(dk2) / sqrt((double)K * D));
  }
}

// EMA mix + revival for VQ_PART codes per workgroup (bottleneck.py:78-84); leaves the partial column sums of the NEW
// codebook and the partial sums of (k_new - k_old)^2 for vq_mu_kernel, which finishes the metrics in fixed order.
static __global__ __launch_bounds__(256) void vq_ema_apply_kernel(float* __restrict__ cb, float* __restrict__ k_sum,
                                                           float* __restrict__ k_elem, const float* __restrict__ stats,
                                                           const float* __restrict__ k_rand, float mu, float threshold,
                                                           int K, int D, float* __restrict__ part, double* __restrict__ dkpart) {
  __shared__ float slab[VQ_PART * 128];
  __shared__ double red[4];
  const int j0 = blockIdx.x * VQ_PART;
  const int n = min(VQ_PART, K - j0) * D;
  const float* cnt = stats + (size_t)K * D;
  double dk2 = 0.0;
  for (int e = threadIdx.x; e < n; e += 256) {
    const int j = j0 + e / D;
    const size_t ge = (size_t)j0 * D + e;
    const float ne = mu * k_elem[j] + (1.f - mu) * cnt[j];   // k_elem is rewritten only after the barrier below
    const float ns = mu * k_sum[ge] + (1.f - mu) * stats[ge];
    const float usage = (ne >= threshold) ? 1.f : 0.f;
    const float nk = usage * (ns / ne) + (1.f - usage) * k_rand[ge];
    const float d = nk - cb[ge];
    dk2 += (double)d * d;
    k_sum[ge] = ns;
    cb[ge] = nk;
    slab[e] = nk;
  }
  dk2 = wave_sum_d(dk2);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = dk2;
  __syncthreads();
  if ((int)threadIdx.x < min(VQ_PART, K - j0)) {
    const int j = j0 + threadIdx.x;
    k_elem[j] = mu * k_elem[j] + (1.f - mu) * cnt[j];
  }
  if (threadIdx.x == 0) dkpart[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
  if ((int)threadIdx.x < D) {
    float t = 0.f;
    for (int q = 0; q < min(VQ_PART, K - j0); ++q) t += slab[q * D + threadIdx.x];
    part[(size_t)blockIdx.x * D + threadIdx.x] = t;
  }
}

}  // namespace smt
