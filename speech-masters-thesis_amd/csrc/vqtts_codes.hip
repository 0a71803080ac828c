// Code head of VQTTS (reference models/vqtts/vqtts.py:86-87, 142-144, 157, 175-178, 190): the projection of the frames to
// l_bins logits fused with the cross-entropy against the quantiser's codes (training) or with the argmax (synthesis).
// No logit and no dlogit is ever stored in global memory.
//
//   ch_split_kernel        weight [V, C] fp32 -> bf16 pairs hi = bf16(w), lo = bf16(w - hi), zero-padded to CP channels, in
//                          both orientations ([V][CP] for the logits, [CP][V] for dh), once per weight version.
//   ch_rows_kernel<false>  forward: CH_ROWS rows per workgroup, one row per MFMA lane (32 per wave), V on the accumulator's
//                          row index.  The weight is staged CH_VT rows at a time in LDS; per staged tile a lane sees 32 of
//                          its row's logits in registers and folds them into the running maximum / sum / argmax.
//   ch_rows_kernel<true>   data gradient: the same logits (ch_logits2, the ONE place a logit is computed with V on the
//                          accumulator), p = exp(logit - lse), G = coef (p - onehot); the G tile is the B operand of the
//                          next MFMAs as it stands (it sums over V, the accumulator's row index): dh^T = W^T G.
//   ch_sample_kernel<TRUNC> synthesis with a draw: the forward's geometry and logits; per logit a counter-based Gumbel noise,
//                          the running argmax of logit / T + g is a sample of softmax(logit / T).  TRUNC (min-p): a first
//                          sweep for the row maximum, the draw among the bins within `cut` of it in a second.
//   ch_dw_kernel           weight gradient: one workgroup = CH_VCOLS columns of V and a slice of rows.  It recomputes its
//                          columns' logits with the ROW on the accumulator's row index (same split, same three products in
//                          the same order), so G sums over the accumulator's row index again: dW = G^T h with h^T staged
//                          in LDS.  One slab per slice, ch_dw_reduce_kernel adds the slabs in slice order in fp64.
//   ch_fwd_partial_kernel, ch_fwd_final_kernel   loss sum, correct count and scored count in a fixed order (the scheme of
//                          vq_reduce_kernel, in two stages: up to CH_SUM_PARTS workgroups add a chunk of rows each, one adds
//                          their partial sums).
// No float atomics anywhere: equal inputs give equal bits.
#include "vq_common.h"

namespace smt {

constexpr int CH_ROWS = 128;          // rows per workgroup of the row kernels: 32 per wave, one per MFMA lane
constexpr int CH_VT = 64;             // weight rows staged in LDS per step of the row kernels (two 32-row MFMA chunks)
constexpr int CH_VCOLS = 64;          // columns of V owned by one workgroup of the weight-gradient kernel (32 past 128 channels)
constexpr int CH_SLICE = 4096;        // rows per slice of the weight-gradient kernel (more once CH_MAX_SLICES is reached)
constexpr int CH_MAX_SLICES = 256;    // slabs the reduce adds at most
constexpr int CH_SUM_PARTS = 256;     // partial sums of the forward's reduce at most: `sums` holds 3 + 3 * CH_SUM_PARTS doubles
constexpr int CH_SUM_ROWS = 4096;     // rows per partial sum (more once CH_SUM_PARTS is reached)
constexpr int CH_MAX_C = 256;
constexpr int CH_MAX_V = 1024;
constexpr int CH_TP = 36;             // pitch (bf16) of a 32-row line of the transposed h tile: 8-byte aligned, conflict-free
constexpr int CH_WTP = 68;            // ... of a CH_VT-column line of the transposed weight tile

// channels are padded with zeros to the next of 32, 64, 128, 256 (one kernel instance each); zeros add nothing to a sum
__host__ __device__ static inline int ch_pad(int C) { return C <= 32 ? 32 : C <= 64 ? 64 : C <= 128 ? 128 : 256; }

// row of the 32x32 accumulator tile that register q of a lane in half hf holds
__device__ __forceinline__ int ch_accrow(int q, int hf) { return (q & 3) + 8 * (q >> 2) + 4 * hf; }

__global__ __launch_bounds__(256) void ch_split_kernel(const float* __restrict__ w, int V, int C, int CP, __bf16* __restrict__ wh,
                                                       __bf16* __restrict__ wl, __bf16* __restrict__ wth, __bf16* __restrict__ wtl) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= V * CP) return;
  const int v = e / CP, c = e - v * CP;
  const float x = c < C ? w[(size_t)v * C + c] : 0.f;
  const __bf16 hi = (__bf16)x;
  const __bf16 lo = (__bf16)(x - (float)hi);
  wh[e] = hi;
  wl[e] = lo;
  wth[(size_t)c * V + v] = hi;
  wtl[(size_t)c * V + v] = lo;
}

// this lane's share of row `row` (channels 16 s + 8 hf .. + 7 of every k-step s), split; k-steps past C are zero
template <int NS>
__device__ __forceinline__ void ch_load_row(const float* __restrict__ h, int C, long long row, int hf, vq_bf16x8* xh, vq_bf16x8* xl) {
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
    if (16 * s < C) {
      const f32x4* src = reinterpret_cast<const f32x4*>(h + row * C + 16 * s + 8 * hf);
      v0 = src[0];
      v1 = src[1];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float c = e < 4 ? v0[e & 3] : v1[e & 3];
      const __bf16 hi = (__bf16)c;
      xh[s][e] = hi;
      xl[s][e] = (__bf16)(c - (float)hi);
    }
  }
}

// G registers 8 s2 .. 8 s2 + 7 of an accumulator tile as the bf16-pair fragment of k-step s2 of the next product
__device__ __forceinline__ void ch_split_g(const f32x16& g, vq_bf16x8 (&gh)[2], vq_bf16x8 (&gl)[2]) {
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float v = g[8 * s2 + e];
      const __bf16 hi = (__bf16)v;
      gh[s2][e] = hi;
      gl[s2][e] = (__bf16)(v - (float)hi);
    }
}

// th / tl of ch_dw_kernel are private to a wave, and a wave's LDS operations execute in order: its writes and the fragment
// reads of its other lanes need the compiler's ordering only, no workgroup barrier
__device__ __forceinline__ void ch_wave_sync() {
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
}

union ChFrag {
  vq_bf16x8 v;
  uint2 h[2];
};

// logits of the two 32-row chunks of the staged weight tile against this lane's row: acc = b + sum_s (wl.xh + wh.xl + wh.xh),
// small terms first, the same instruction sequence for every column
template <int CP>
__device__ __forceinline__ void ch_logits2(const char* wt, const float* bl, int j, int hf, const vq_bf16x8* xh, const vq_bf16x8* xl,
                                           f32x16 (&acc)[2]) {
  constexpr int NS = CP / 16, PITCH = 2 * CP + 16, TILE = CH_VT * PITCH;
#pragma unroll
  for (int ch = 0; ch < 2; ++ch)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[ch][q] = bl[32 * ch + ch_accrow(q, hf)];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      const char* a = wt + (32 * ch + j) * PITCH + 16 * (2 * s + hf);
      const vq_bf16x8 fh = *reinterpret_cast<const vq_bf16x8*>(a);
      const vq_bf16x8 fl = *reinterpret_cast<const vq_bf16x8*>(a + TILE);
      acc[ch] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fl, xh[s], acc[ch], 0, 0, 0);
      acc[ch] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh, xl[s], acc[ch], 0, 0, 0);
      acc[ch] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh, xh[s], acc[ch], 0, 0, 0);
    }
  }
}

template <int CP, bool BWD>
struct ChRowsLds {
  static constexpr int PITCH = 2 * CP + 16, TILE = CH_VT * PITCH;
  static constexpr int BIAS = CH_MAX_V * 4;                       // bias, zero-filled past V
  static constexpr int WT = BIAS, WTT = WT + 2 * TILE;            // [hi | lo][CH_VT][PITCH]; then [hi | lo][CP][CH_WTP] bf16
  static constexpr int TTILE = CP * CH_WTP * 2;
  static constexpr int TOTAL = WTT + (BWD ? 2 * TTILE : 0);
};

template <int CP, bool BWD>
__global__ __launch_bounds__(256) void ch_rows_kernel(const float* __restrict__ h, const __bf16* __restrict__ wh,
                                                      const __bf16* __restrict__ wl, const __bf16* __restrict__ wth,
                                                      const __bf16* __restrict__ wtl, const float* __restrict__ bias,
                                                      const long long* __restrict__ target, const float* __restrict__ lse_in,
                                                      const float* __restrict__ coef, long long N, int C, int V,
                                                      float* __restrict__ lse_out, float* __restrict__ row_loss,
                                                      int* __restrict__ pred, float* __restrict__ correct, float* __restrict__ dh) {
  using L = ChRowsLds<CP, BWD>;
  constexpr int NS = CP / 16, NCB = CP / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* bl = reinterpret_cast<float*>(smem);
  char* wt = reinterpret_cast<char*>(smem) + L::WT;
  char* wtt = reinterpret_cast<char*>(smem) + L::WTT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, hf = lane >> 5;
  const long long row = (long long)blockIdx.x * CH_ROWS + wave * 32 + j;
  const long long rowc = row < N ? row : N - 1;                  // a row past the end reads the last one and stores nothing

  vq_bf16x8 xh[NS], xl[NS];
  ch_load_row<NS>(h, C, rowc, hf, xh, xl);
  for (int i = tid; i < CH_MAX_V; i += 256) bl[i] = i < V ? bias[i] : 0.f;
  const long long t = target ? target[rowc] : -1;
  const bool scored = target && t >= 0 && row < N;

  const float NEG_INF = -__builtin_huge_valf();
  float m = NEG_INF, ssum = 0.f, best = NEG_INF, lt = 0.f;
  int bidx = 0;
  bool found = false;
  float lser = 0.f, k = 0.f;
  f32x16 dacc[NCB];
  if (BWD) {
    lser = lse_in[rowc];
    k = coef[0];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
      for (int q = 0; q < 16; ++q) dacc[cb][q] = 0.f;
  }

  for (int v0 = 0; v0 < V; v0 += CH_VT) {
    const bool two = v0 + CH_VT <= V;                            // V is a multiple of 32: the last tile may hold one chunk
    __syncthreads();                                             // the previous tile is consumed
    for (int p = tid; p < CH_VT * (CP / 8); p += 256) {
      const int r = p / (CP / 8), pc = p - r * (CP / 8);
      uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
      if (v0 + r < V) {
        a = *reinterpret_cast<const uint4*>(wh + (size_t)(v0 + r) * CP + 8 * pc);
        b = *reinterpret_cast<const uint4*>(wl + (size_t)(v0 + r) * CP + 8 * pc);
      }
      *reinterpret_cast<uint4*>(wt + r * L::PITCH + 16 * pc) = a;
      *reinterpret_cast<uint4*>(wt + L::TILE + r * L::PITCH + 16 * pc) = b;
    }
    if (BWD) {
      for (int p = tid; p < CP * (CH_VT / 8); p += 256) {
        const int c = p / (CH_VT / 8), pc = p - c * (CH_VT / 8);
        uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
        if (v0 + 8 * pc < V) {                                   // V % 32 == 0: a piece of 8 columns is inside or outside
          a = *reinterpret_cast<const uint4*>(wth + (size_t)c * V + v0 + 8 * pc);
          b = *reinterpret_cast<const uint4*>(wtl + (size_t)c * V + v0 + 8 * pc);
        }
        char* d = wtt + c * (CH_WTP * 2) + 16 * pc;              // 8-byte aligned lines: two 8-byte stores
        *reinterpret_cast<uint2*>(d) = make_uint2(a.x, a.y);
        *reinterpret_cast<uint2*>(d + 8) = make_uint2(a.z, a.w);
        *reinterpret_cast<uint2*>(d + L::TTILE) = make_uint2(b.x, b.y);
        *reinterpret_cast<uint2*>(d + L::TTILE + 8) = make_uint2(b.z, b.w);
      }
    }
    __syncthreads();

    f32x16 acc[2];
    ch_logits2<CP>(wt, bl + v0, j, hf, xh, xl, acc);

    if (!BWD) {
#pragma unroll
      for (int ch = 0; ch < 2; ++ch) {
        if (ch == 0 || two) {
          float cm = acc[ch][0];
#pragma unroll
          for (int q = 1; q < 16; ++q) cm = fmaxf(cm, acc[ch][q]);
          const float mn = fmaxf(m, cm);
          float ps = 0.f;
#pragma unroll
          for (int q = 0; q < 16; ++q) ps += expf(acc[ch][q] - mn);
          ssum = ssum * expf(m - mn) + ps;
          m = mn;
#pragma unroll
          for (int q = 0; q < 16; ++q) {                         // ascending index inside a lane: '>' keeps the lowest
            const int vi = v0 + 32 * ch + ch_accrow(q, hf);
            const float a = acc[ch][q];
            if (a > best) { best = a; bidx = vi; }
            if ((long long)vi == t) { lt = a; found = true; }
          }
        }
      }
    } else {
#pragma unroll
      for (int ch = 0; ch < 2; ++ch) {
        f32x16 g;
        const bool live = scored && (ch == 0 || two);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int vi = v0 + 32 * ch + ch_accrow(q, hf);
          const float p = expf(acc[ch][q] - lser);
          g[q] = live ? k * (p - ((long long)vi == t ? 1.f : 0.f)) : 0.f;
        }
        vq_bf16x8 gh[2], gl[2];
        ch_split_g(g, gh, gl);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
          for (int cb = 0; cb < NCB; ++cb) {
            // A = W^T: lane = channel 32 cb + j, element e = weight row 32 ch + 16 s2 + 8 (e >> 2) + 4 hf + (e & 3), the
            // row of the G tile that element e of the B fragment holds
            const char* a = wtt + (32 * cb + j) * (CH_WTP * 2) + 2 * (32 * ch + 16 * s2 + 4 * hf);
            ChFrag fh, fl;
            fh.h[0] = *reinterpret_cast<const uint2*>(a);
            fh.h[1] = *reinterpret_cast<const uint2*>(a + 16);
            fl.h[0] = *reinterpret_cast<const uint2*>(a + L::TTILE);
            fl.h[1] = *reinterpret_cast<const uint2*>(a + L::TTILE + 16);
            dacc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fl.v, gh[s2], dacc[cb], 0, 0, 0);
            dacc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh.v, gl[s2], dacc[cb], 0, 0, 0);
            dacc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh.v, gh[s2], dacc[cb], 0, 0, 0);
          }
        }
      }
    }
  }

  if (!BWD) {
    // the two lane halves hold interleaved columns of the same row; both compute the same sum (a + b == b + a)
    const float om = __shfl_xor(m, 32, 64), os = __shfl_xor(ssum, 32, 64), ob = __shfl_xor(best, 32, 64);
    const int oi = __shfl_xor(bidx, 32, 64);
    const float olt = __shfl_xor(lt, 32, 64);
    const float M = fmaxf(m, om);
    const float S = ssum * expf(m - M) + os * expf(om - M);
    if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
    const float ltv = found ? lt : olt;                          // the other half found it (or the target is out of range: 0)
    const float lse = M + logf(S);
    if (hf == 0 && row < N) {
      if (lse_out) lse_out[row] = lse;
      pred[row] = bidx;
      if (target) {
        row_loss[row] = scored ? lse - ltv : 0.f;
        correct[row] = (scored && (long long)bidx == t) ? 1.f : 0.f;
      }
    }
  } else {
    if (row < N) {
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          const int c0 = 32 * cb + 8 * q4 + 4 * hf;
          if (c0 < C) {
            const f32x4 v = {dacc[cb][4 * q4], dacc[cb][4 * q4 + 1], dacc[cb][4 * q4 + 2], dacc[cb][4 * q4 + 3]};
            *reinterpret_cast<f32x4*>(dh + row * C + c0) = v;
          }
        }
    }
  }
}

// ---- sampling ("VQTTS code head" of the header, smt_vqtts_code_head_sample) ---------------------------------------------
constexpr unsigned CH_NOISE_ROW = 0x9E3779B1u;   // odd multiplier of the frame index in a row's key
constexpr unsigned CH_NOISE_BIN = 0x85EBCA77u;   // ... of the bin index in a logit's counter

// Gumbel noise of bin v under the row's key: u = ((bits >> 9) + 0.5) 2^-23 is exact in fp32 and strictly inside (0, 1)
__device__ __forceinline__ float ch_gumbel(unsigned key, int v) {
  const unsigned bits = fmix32(key + (unsigned)v * CH_NOISE_BIN);
  const float u = ((float)(bits >> 9) + 0.5f) * 1.1920928955078125e-07f;
  return -logf(-logf(u));
}

// The staging step of ch_rows_kernel: weight rows v0 .. v0 + CH_VT - 1 (zeros past V) into [hi | lo][CH_VT][PITCH].  A copy,
// not a shared helper: factoring the loop out of ch_rows_kernel changes that kernel's register allocation.
template <int CP>
__device__ __forceinline__ void ch_stage_w(const __bf16* __restrict__ wh, const __bf16* __restrict__ wl, int v0, int V, int tid,
                                           char* wt) {
  constexpr int PITCH = 2 * CP + 16, TILE = CH_VT * PITCH;
  for (int p = tid; p < CH_VT * (CP / 8); p += 256) {
    const int r = p / (CP / 8), pc = p - r * (CP / 8);
    uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
    if (v0 + r < V) {
      a = *reinterpret_cast<const uint4*>(wh + (size_t)(v0 + r) * CP + 8 * pc);
      b = *reinterpret_cast<const uint4*>(wl + (size_t)(v0 + r) * CP + 8 * pc);
    }
    *reinterpret_cast<uint4*>(wt + r * PITCH + 16 * pc) = a;
    *reinterpret_cast<uint4*>(wt + TILE + r * PITCH + 16 * pc) = b;
  }
}

// One draw per row from softmax(logit / T) by Gumbel-max, in the forward's geometry (one row per MFMA lane, V on the
// accumulator's row index, the logits of ch_logits2 bit for bit).  TRUNC: a first sweep finds the row's maximum M, the second
// recomputes the logits -- the same instructions on the same operands, so M itself is met again and kept -- and only the
// bins with logit >= M + cut compete.  The winner is the kept bin with the highest score = fma(logit, 1/T, g), lowest index
// on ties: ascending index inside a lane, the tie rule across the two lane halves.
template <int CP, bool TRUNC>
__global__ __launch_bounds__(256) void ch_sample_kernel(const float* __restrict__ h, const __bf16* __restrict__ wh,
                                                        const __bf16* __restrict__ wl, const float* __restrict__ bias,
                                                        const int* __restrict__ seeds, long long N, int t_q, int C, int V,
                                                        float inv_t, float cut, int* __restrict__ pred, int* __restrict__ n_kept) {
  using L = ChRowsLds<CP, false>;
  constexpr int NS = CP / 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* bl = reinterpret_cast<float*>(smem);
  char* wt = reinterpret_cast<char*>(smem) + L::WT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, hf = lane >> 5;
  const long long row = (long long)blockIdx.x * CH_ROWS + wave * 32 + j;
  const long long rowc = row < N ? row : N - 1;                  // a row past the end reads the last one and stores nothing

  vq_bf16x8 xh[NS], xl[NS];
  ch_load_row<NS>(h, C, rowc, hf, xh, xl);
  for (int i = tid; i < CH_MAX_V; i += 256) bl[i] = i < V ? bias[i] : 0.f;
  const int item = (int)(rowc / t_q), frame = (int)(rowc - (long long)item * t_q);
  const unsigned key = fmix32(fmix32((unsigned)seeds[item]) + (unsigned)frame * CH_NOISE_ROW);

  const float NEG_INF = -__builtin_huge_valf();
  float thr = NEG_INF;
  if (TRUNC) {
    float m = NEG_INF;
    for (int v0 = 0; v0 < V; v0 += CH_VT) {
      const bool two = v0 + CH_VT <= V;
      __syncthreads();                                           // the previous tile is consumed
      ch_stage_w<CP>(wh, wl, v0, V, tid, wt);
      __syncthreads();
      f32x16 acc[2];
      ch_logits2<CP>(wt, bl + v0, j, hf, xh, xl, acc);
#pragma unroll
      for (int ch = 0; ch < 2; ++ch)
        if (ch == 0 || two) {
#pragma unroll
          for (int q = 0; q < 16; ++q) m = fmaxf(m, acc[ch][q]);
        }
    }
    thr = fmaxf(m, __shfl_xor(m, 32, 64)) + cut;
  }

  float best = NEG_INF;
  int bidx = 0, kept = 0;
  for (int v0 = 0; v0 < V; v0 += CH_VT) {
    const bool two = v0 + CH_VT <= V;                            // V is a multiple of 32: the last tile may hold one chunk
    __syncthreads();
    ch_stage_w<CP>(wh, wl, v0, V, tid, wt);
    __syncthreads();
    f32x16 acc[2];
    ch_logits2<CP>(wt, bl + v0, j, hf, xh, xl, acc);
#pragma unroll
    for (int ch = 0; ch < 2; ++ch)
      if (ch == 0 || two) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {                           // ascending index inside a lane: '>' keeps the lowest
          const int vi = v0 + 32 * ch + ch_accrow(q, hf);
          const float a = acc[ch][q];
          if (!TRUNC || a >= thr) {
            const float s = fmaf(a, inv_t, ch_gumbel(key, vi));
            ++kept;
            if (s > best) { best = s; bidx = vi; }
          }
        }
      }
  }
  // the two lane halves hold interleaved columns of the same row; a half that kept nothing stands at -inf
  const float ob = __shfl_xor(best, 32, 64);
  const int oi = __shfl_xor(bidx, 32, 64), ok = __shfl_xor(kept, 32, 64);
  if (ob > best || (ob == best && oi < bidx)) bidx = oi;
  if (hf == 0 && row < N) {
    pred[row] = bidx;
    if (n_kept) n_kept[row] = kept + ok;
  }
}

// The forward's three sums as doubles, in two stages with a fixed order.  Stage 1: workgroup p owns rows [p chunk, (p + 1) chunk),
// thread t adds its rows t, t + 256, ... in that order, then a fixed tree; part[3 p ..] = sum of row_loss, sum of correct, rows
// with target >= 0.
__global__ __launch_bounds__(256) void ch_fwd_partial_kernel(const float* __restrict__ row_loss, const float* __restrict__ correct,
                                                             const long long* __restrict__ target, long long N, long long chunk,
                                                             double* __restrict__ part) {
  __shared__ double sh[3][4];
  const long long begin = (long long)blockIdx.x * chunk;
  const long long end = begin + chunk < N ? begin + chunk : N;
  double a = 0.0, b = 0.0, c = 0.0;
#pragma unroll 4
  for (long long r = begin + threadIdx.x; r < end; r += 256) {
    a += row_loss[r];
    b += correct[r];
    c += target[r] >= 0 ? 1.0 : 0.0;
  }
  a = wave_sum_d(a); b = wave_sum_d(b); c = wave_sum_d(c);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { sh[0][wave] = a; sh[1][wave] = b; sh[2][wave] = c; }
  __syncthreads();
  if (threadIdx.x < 3) part[3 * blockIdx.x + threadIdx.x] = ((sh[threadIdx.x][0] + sh[threadIdx.x][1]) + sh[threadIdx.x][2]) + sh[threadIdx.x][3];
}

// Stage 2: one workgroup, thread t holds partial t (0 past `parts`), the same tree.  parts = 0 (no rows) gives three zeros.
__global__ __launch_bounds__(CH_SUM_PARTS) void ch_fwd_final_kernel(const double* __restrict__ part, int parts, double* __restrict__ sums) {
  __shared__ double sh[3][CH_SUM_PARTS / 64];
  const int t = threadIdx.x;
  double a = t < parts ? part[3 * t] : 0.0, b = t < parts ? part[3 * t + 1] : 0.0, c = t < parts ? part[3 * t + 2] : 0.0;
  a = wave_sum_d(a); b = wave_sum_d(b); c = wave_sum_d(c);
  const int lane = t & 63, wave = t >> 6;
  if (lane == 0) { sh[0][wave] = a; sh[1][wave] = b; sh[2][wave] = c; }
  __syncthreads();
  if (t < 3) {
    double s = 0.0;
    for (int w = 0; w < CH_SUM_PARTS / 64; ++w) s += sh[t][w];
    sums[t] = s;
  }
}

template <int CP>
struct ChDwLds {
  static constexpr int VCN = CP > 128 ? 1 : 2;                    // 32-column chunks per workgroup: CH_VCOLS / 32, one at 256
                                                                  // channels (the accumulators are VCN * CP / 2 registers)
  static constexpr int TTILE = CP * CH_TP * 2;                    // one wave's transposed h tile, hi or lo
  static constexpr int WAVE = 2 * TTILE;
  static constexpr int Z = CH_VCOLS * CP * 4;                     // the cross-wave sum reuses the tiles
  static constexpr int DB = 4 * WAVE > Z ? 4 * WAVE : Z;
  static constexpr int TOTAL = DB + 4 * CH_VCOLS * 8;
};

template <int CP>
__global__ __launch_bounds__(256) void ch_dw_kernel(const float* __restrict__ h, const __bf16* __restrict__ wh,
                                                    const __bf16* __restrict__ wl, const float* __restrict__ bias,
                                                    const long long* __restrict__ target, const float* __restrict__ lse,
                                                    const float* __restrict__ coef, long long N, int C, int V,
                                                    long long slice_rows, float* __restrict__ slab, double* __restrict__ dbslab) {
  using L = ChDwLds<CP>;
  constexpr int NS = CP / 16, NCB = CP / 32, VCN = ChDwLds<CP>::VCN, VCOLS = 32 * VCN;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, hf = lane >> 5;
  __bf16* th = reinterpret_cast<__bf16*>(smem + wave * L::WAVE);  // [CP][CH_TP]: channel-major, this wave's 32 rows
  __bf16* tl = reinterpret_cast<__bf16*>(smem + wave * L::WAVE + L::TTILE);
  float* zb = reinterpret_cast<float*>(smem);
  double* dbs = reinterpret_cast<double*>(smem + L::DB);          // [4][CH_VCOLS]
  const int v0 = blockIdx.x * VCOLS;
  const long long r_begin = (long long)blockIdx.y * slice_rows;
  const long long r_end = r_begin + slice_rows < N ? r_begin + slice_rows : N;
  const float k = coef[0];

  f32x16 z[VCN][NCB];
#pragma unroll
  for (int vc = 0; vc < VCN; ++vc)
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
      for (int q = 0; q < 16; ++q) z[vc][cb][q] = 0.f;
  double dbacc[VCN];
#pragma unroll
  for (int vc = 0; vc < VCN; ++vc) dbacc[vc] = 0.0;

  const long long ntiles = (r_end - r_begin + 31) / 32;
  const long long iters = (ntiles + 3) / 4;
  for (long long it = 0; it < iters; ++it) {
    const long long r0 = r_begin + (it * 4 + wave) * 32;          // may lie past r_end: every row is then unscored
    const long long row = r0 + j;
    const long long rowc = row < N ? row : N - 1;
    vq_bf16x8 xh[NS], xl[NS];
    ch_load_row<NS>(h, C, rowc, hf, xh, xl);
    ch_wave_sync();                                               // the previous tile's fragment reads are done
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = 16 * s + 8 * hf + e;
        th[c * CH_TP + j] = xh[s][e];
        tl[c * CH_TP + j] = xl[s][e];
      }
    ch_wave_sync();
    float lq[16];
    int tq[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const long long rq = r0 + ch_accrow(q, hf);
      const bool in = rq < r_end;
      lq[q] = in ? lse[rq] : 0.f;
      const long long tt = in ? target[rq] : -1;
      tq[q] = tt < 0 ? -1 : (tt < V ? (int)tt : V);               // an out-of-range target matches no column
    }
#pragma unroll
    for (int vc = 0; vc < VCN; ++vc) {
      const int vcol = v0 + 32 * vc + j;
      const bool vin = vcol < V;
      const int vcl = vin ? vcol : V - 1;
      const float bv = bias[vcl];
      f32x16 acc;
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[q] = bv;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const vq_bf16x8 fh = *reinterpret_cast<const vq_bf16x8*>(wh + (size_t)vcl * CP + 16 * s + 8 * hf);
        const vq_bf16x8 fl = *reinterpret_cast<const vq_bf16x8*>(wl + (size_t)vcl * CP + 16 * s + 8 * hf);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh[s], fl, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xl[s], fh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh[s], fh, acc, 0, 0, 0);
      }
      f32x16 g;
      double dsum = 0.0;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const float p = expf(acc[q] - lq[q]);
        g[q] = (tq[q] >= 0 && vin) ? k * (p - (tq[q] == vcol ? 1.f : 0.f)) : 0.f;
        dsum += (double)g[q];
      }
      dbacc[vc] += dsum;
      vq_bf16x8 gh[2], gl[2];
      ch_split_g(g, gh, gl);
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
          // B = h: lane = channel 32 cb + j, element e = row 16 s2 + 8 (e >> 2) + 4 hf + (e & 3) of the tile
          const __bf16* b = th + (32 * cb + j) * CH_TP + 16 * s2 + 4 * hf;
          ChFrag fh, fl;
          fh.h[0] = *reinterpret_cast<const uint2*>(b);
          fh.h[1] = *reinterpret_cast<const uint2*>(b + 8);
          fl.h[0] = *reinterpret_cast<const uint2*>(b + L::TTILE / 2);
          fl.h[1] = *reinterpret_cast<const uint2*>(b + L::TTILE / 2 + 8);
          z[vc][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gl[s2], fh.v, z[vc][cb], 0, 0, 0);
          z[vc][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh[s2], fl.v, z[vc][cb], 0, 0, 0);
          z[vc][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh[s2], fh.v, z[vc][cb], 0, 0, 0);
        }
      }
    }
  }

  // db: the two lane halves of a wave hold different rows of the same column
#pragma unroll
  for (int vc = 0; vc < VCN; ++vc) {
    const double d = dbacc[vc] + __shfl_xor(dbacc[vc], 32, 64);
    if (hf == 0) dbs[wave * CH_VCOLS + 32 * vc + j] = d;
  }
  // dW: waves 0..3 add their accumulators into one LDS image in that order
  for (int w = 0; w < 4; ++w) {
    __syncthreads();
    if (wave == w) {
#pragma unroll
      for (int vc = 0; vc < VCN; ++vc)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            float* d = zb + (32 * vc + ch_accrow(q, hf)) * CP + 32 * cb + j;
            *d = w == 0 ? z[vc][cb][q] : *d + z[vc][cb][q];
          }
    }
  }
  __syncthreads();
  float* out = slab + (size_t)blockIdx.y * V * C;
  for (int e = tid; e < VCOLS * C; e += 256) {
    const int v = e / C, c = e - v * C;
    if (v0 + v < V) out[(size_t)(v0 + v) * C + c] = zb[v * CP + c];
  }
  if (tid < VCOLS && v0 + tid < V)
    dbslab[(size_t)blockIdx.y * V + v0 + tid] = ((dbs[tid] + dbs[CH_VCOLS + tid]) + dbs[2 * CH_VCOLS + tid]) + dbs[3 * CH_VCOLS + tid];
}

// dW[e] = sum over the slabs in slice order (fp64), db likewise: one thread per element
__global__ __launch_bounds__(256) void ch_dw_reduce_kernel(const float* __restrict__ slab, const double* __restrict__ dbslab,
                                                           int nslices, int V, int C, float* __restrict__ dw, float* __restrict__ db) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int vc = V * C;
  if (e < vc) {
    double s = 0.0;
    for (int sl = 0; sl < nslices; ++sl) s += (double)slab[(size_t)sl * vc + e];
    dw[e] = (float)s;
  } else if (e < vc + V) {
    double s = 0.0;
    for (int sl = 0; sl < nslices; ++sl) s += dbslab[(size_t)sl * V + (e - vc)];
    db[e - vc] = (float)s;
  }
}

struct ChSlices {
  long long rows;
  int n;
};
static ChSlices ch_slices(long long N) {
  ChSlices s;
  s.rows = CH_SLICE;
  if ((N + s.rows - 1) / s.rows > CH_MAX_SLICES) s.rows = ((N + CH_MAX_SLICES - 1) / CH_MAX_SLICES + 127) / 128 * 128;
  s.n = (int)((N + s.rows - 1) / s.rows);
  return s;
}

}  // namespace smt

using namespace smt;

#define CH_CHECK_SHAPE(name)                                                                                                   \
  SMT_CHECK_ARG(rows >= 0 && rows <= 2147483647ll, name ": rows=%lld must be between 0 and 2^31 - 1", (long long)rows);         \
  SMT_CHECK_ARG(channels > 0 && channels % 16 == 0 && channels <= CH_MAX_C, name ": channels=%d must be a multiple of 16 up to %d", \
                channels, CH_MAX_C);                                                                                            \
  SMT_CHECK_ARG(bins > 0 && bins % 32 == 0 && bins <= CH_MAX_V, name ": bins=%d must be a multiple of 32 up to %d", bins, CH_MAX_V)

#define CH_DISPATCH(CP_, STMT)            \
  switch (CP_) {                          \
    case 32: { constexpr int CP = 32; STMT; } break;   \
    case 64: { constexpr int CP = 64; STMT; } break;   \
    case 128: { constexpr int CP = 128; STMT; } break; \
    default: { constexpr int CP = 256; STMT; } break;  \
  }

extern "C" size_t smt_vqtts_code_head_workspace_bytes(int channels, int bins) {
  if (channels <= 0 || bins <= 0) return 0;
  return (size_t)8 * bins * ch_pad(channels);                    // hi and lo, both orientations, 2 bytes each
}

extern "C" int smt_vqtts_code_head_prepare(const float* weight, int channels, int bins, void* workspace, size_t workspace_bytes,
                                           smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const long long rows = 0;
  CH_CHECK_SHAPE("smt_vqtts_code_head_prepare");
  SMT_CHECK_ARG(weight && workspace, "smt_vqtts_code_head_prepare: null pointer");
  const size_t need = smt_vqtts_code_head_workspace_bytes(channels, bins);
  SMT_CHECK_ARG(workspace_bytes >= need, "smt_vqtts_code_head_prepare: workspace of %zu B, %zu B needed", workspace_bytes, need);
  SMT_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "smt_vqtts_code_head_prepare: workspace must be 16-byte aligned");
  const int CP = ch_pad(channels);
  __bf16* wh = reinterpret_cast<__bf16*>(workspace);
  const size_t n = (size_t)bins * CP;
  ch_split_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(weight, bins, channels, CP, wh, wh + n, wh + 2 * n, wh + 3 * n);
  SMT_CHECK_LAUNCH("ch_split");
  return 0;
}

// the dynamic-LDS limit of a kernel is set once per device, not per launch
static void ch_allow_lds(const void* kernel, int bytes, unsigned long long* done_on) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64 || !((*done_on >> dev) & 1ull)) {
    (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (dev >= 0 && dev < 64) *done_on |= 1ull << dev;
  }
}

template <int CP, bool BWD>
static void ch_launch_rows(hipStream_t stream, const float* h, const __bf16* ws, const float* bias, const long long* target,
                           const float* lse_in, const float* coef, long long N, int C, int V, float* lse_out, float* row_loss,
                           int* pred, float* correct, float* dh) {
  using L = ChRowsLds<CP, BWD>;
  const size_t n = (size_t)V * CP;
  static unsigned long long allowed = 0;                          // one bit per device, one word per kernel instance
  ch_allow_lds((const void*)ch_rows_kernel<CP, BWD>, L::TOTAL, &allowed);
  ch_rows_kernel<CP, BWD><<<(unsigned)((N + CH_ROWS - 1) / CH_ROWS), 256, L::TOTAL, stream>>>(
      h, ws, ws + n, ws + 2 * n, ws + 3 * n, bias, target, lse_in, coef, N, C, V, lse_out, row_loss, pred, correct, dh);
}

template <int CP>
static void ch_launch_dw(hipStream_t stream, dim3 grid, const float* h, const __bf16* wh, const __bf16* wl, const float* bias,
                         const long long* target, const float* lse, const float* coef, long long N, int C, int V,
                         long long slice_rows, float* slab, double* dbslab) {
  static unsigned long long allowed = 0;
  ch_allow_lds((const void*)ch_dw_kernel<CP>, ChDwLds<CP>::TOTAL, &allowed);
  ch_dw_kernel<CP><<<grid, 256, ChDwLds<CP>::TOTAL, stream>>>(h, wh, wl, bias, target, lse, coef, N, C, V, slice_rows, slab, dbslab);
}

extern "C" int smt_vqtts_code_head_fwd(const float* h, const void* workspace, size_t workspace_bytes, const float* bias,
                                       const int64_t* target, int64_t rows, int channels, int bins, float* lse, float* row_loss,
                                       int* pred, float* correct, double* sums, smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CH_CHECK_SHAPE("smt_vqtts_code_head_fwd");
  SMT_CHECK_ARG(workspace && bias && (pred || rows == 0), "smt_vqtts_code_head_fwd: null pointer");
  SMT_CHECK_ARG(!target || (lse && row_loss && correct && sums), "smt_vqtts_code_head_fwd: null pointer (a target needs every output)");
  SMT_CHECK_ARG(workspace_bytes >= smt_vqtts_code_head_workspace_bytes(channels, bins),
                "smt_vqtts_code_head_fwd: workspace of %zu B, %zu B needed", workspace_bytes,
                smt_vqtts_code_head_workspace_bytes(channels, bins));
  SMT_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)h & 15) == 0, "smt_vqtts_code_head_fwd: h and workspace must be 16-byte aligned");
  const __bf16* ws = reinterpret_cast<const __bf16*>(workspace);
  const long long* tg = reinterpret_cast<const long long*>(target);
  if (rows > 0) {
    SMT_CHECK_ARG(h, "smt_vqtts_code_head_fwd: null pointer");
    CH_DISPATCH(ch_pad(channels), (ch_launch_rows<CP, false>(stream, h, ws, bias, tg, nullptr, nullptr, rows, channels, bins, lse,
                                                             row_loss, pred, correct, nullptr)));
    SMT_CHECK_LAUNCH("ch_rows_fwd");
  }
  if (target) {
    long long chunk = CH_SUM_ROWS;
    if ((rows + chunk - 1) / chunk > CH_SUM_PARTS) chunk = (rows + CH_SUM_PARTS - 1) / CH_SUM_PARTS;
    const int parts = (int)((rows + chunk - 1) / chunk);
    double* part = sums + 3;
    if (parts > 0) {
      ch_fwd_partial_kernel<<<parts, 256, 0, stream>>>(row_loss, correct, tg, rows, chunk, part);
      SMT_CHECK_LAUNCH("ch_fwd_partial");
    }
    ch_fwd_final_kernel<<<1, CH_SUM_PARTS, 0, stream>>>(part, parts, sums);
    SMT_CHECK_LAUNCH("ch_fwd_final");
  }
  return 0;
}

template <int CP, bool TRUNC>
static void ch_launch_sample(hipStream_t stream, const float* h, const __bf16* ws, const float* bias, const int* seeds, long long N,
                             int t_q, int C, int V, float inv_t, float cut, int* pred, int* n_kept) {
  using L = ChRowsLds<CP, false>;
  const size_t n = (size_t)V * CP;
  static unsigned long long allowed = 0;
  ch_allow_lds((const void*)ch_sample_kernel<CP, TRUNC>, L::TOTAL, &allowed);
  ch_sample_kernel<CP, TRUNC><<<(unsigned)((N + CH_ROWS - 1) / CH_ROWS), 256, L::TOTAL, stream>>>(h, ws, ws + n, bias, seeds, N, t_q, C,
                                                                                               V, inv_t, cut, pred, n_kept);
}

extern "C" int smt_vqtts_code_head_sample(const float* h, const void* workspace, size_t workspace_bytes, const float* bias,
                                          const int* seeds, int64_t rows, int t_q, int channels, int bins, float inv_temperature,
                                          float cut, int* pred, int* n_kept, smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CH_CHECK_SHAPE("smt_vqtts_code_head_sample");
  SMT_CHECK_ARG(t_q >= 1, "smt_vqtts_code_head_sample: t_q=%d must be at least 1", t_q);
  SMT_CHECK_ARG(rows % t_q == 0, "smt_vqtts_code_head_sample: rows=%lld must be a multiple of t_q=%d", (long long)rows, t_q);
  SMT_CHECK_ARG(inv_temperature > 0.f && inv_temperature <= 3.402823466e38f,
                "smt_vqtts_code_head_sample: inv_temperature=%g must be finite and > 0", (double)inv_temperature);
  SMT_CHECK_ARG(cut <= 0.f, "smt_vqtts_code_head_sample: cut=%g must be <= 0 (T ln(min_p); -inf = no truncation)", (double)cut);
  SMT_CHECK_ARG(workspace && bias && ((seeds && pred) || rows == 0), "smt_vqtts_code_head_sample: null pointer");
  SMT_CHECK_ARG(workspace_bytes >= smt_vqtts_code_head_workspace_bytes(channels, bins),
                "smt_vqtts_code_head_sample: workspace of %zu B, %zu B needed", workspace_bytes,
                smt_vqtts_code_head_workspace_bytes(channels, bins));
  SMT_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)h & 15) == 0,
                "smt_vqtts_code_head_sample: h and workspace must be 16-byte aligned");
  if (rows == 0) return 0;
  SMT_CHECK_ARG(h, "smt_vqtts_code_head_sample: null pointer");
  const __bf16* ws = reinterpret_cast<const __bf16*>(workspace);
  if (cut >= -3.402823466e38f) {                                  // a finite cut: two sweeps
    CH_DISPATCH(ch_pad(channels), (ch_launch_sample<CP, true>(stream, h, ws, bias, seeds, rows, t_q, channels, bins, inv_temperature,
                                                              cut, pred, n_kept)));
  } else {
    CH_DISPATCH(ch_pad(channels), (ch_launch_sample<CP, false>(stream, h, ws, bias, seeds, rows, t_q, channels, bins,
                                                               inv_temperature, cut, pred, n_kept)));
  }
  SMT_CHECK_LAUNCH("ch_sample");
  return 0;
}

extern "C" size_t smt_vqtts_code_head_bwd_workspace_bytes(int64_t rows, int channels, int bins) {
  if (rows <= 0 || channels <= 0 || bins <= 0) return 0;
  const ChSlices s = ch_slices(rows);
  return (size_t)s.n * bins * ((size_t)channels * 4 + 8);
}

extern "C" int smt_vqtts_code_head_bwd(const float* h, const void* workspace, size_t workspace_bytes, const float* bias,
                                       const int64_t* target, const float* lse, const float* coef, int64_t rows, int channels,
                                       int bins, float* dh, float* dweight, float* dbias, void* scratch, size_t scratch_bytes,
                                       smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CH_CHECK_SHAPE("smt_vqtts_code_head_bwd");
  SMT_CHECK_ARG(workspace && bias && coef && dweight && dbias, "smt_vqtts_code_head_bwd: null pointer");
  SMT_CHECK_ARG(workspace_bytes >= smt_vqtts_code_head_workspace_bytes(channels, bins),
                "smt_vqtts_code_head_bwd: workspace of %zu B, %zu B needed", workspace_bytes,
                smt_vqtts_code_head_workspace_bytes(channels, bins));
  SMT_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)h & 15) == 0 && ((uintptr_t)dh & 15) == 0,
                "smt_vqtts_code_head_bwd: h, dh and workspace must be 16-byte aligned");
  if (rows == 0) {
    if (hipMemsetAsync(dweight, 0, (size_t)bins * channels * 4, stream) != hipSuccess ||
        hipMemsetAsync(dbias, 0, (size_t)bins * 4, stream) != hipSuccess)
      SMT_CHECK_ARG(false, "smt_vqtts_code_head_bwd: memset failed");
    return 0;
  }
  SMT_CHECK_ARG(h && target && lse && dh && scratch, "smt_vqtts_code_head_bwd: null pointer");
  const size_t need = smt_vqtts_code_head_bwd_workspace_bytes(rows, channels, bins);
  SMT_CHECK_ARG(scratch_bytes >= need, "smt_vqtts_code_head_bwd: scratch of %zu B, %zu B needed", scratch_bytes, need);
  SMT_CHECK_ARG(((uintptr_t)scratch & 15) == 0, "smt_vqtts_code_head_bwd: scratch must be 16-byte aligned");
  const __bf16* ws = reinterpret_cast<const __bf16*>(workspace);
  const long long* tg = reinterpret_cast<const long long*>(target);
  const int CPr = ch_pad(channels);
  CH_DISPATCH(CPr, (ch_launch_rows<CP, true>(stream, h, ws, bias, tg, lse, coef, rows, channels, bins, nullptr, nullptr, nullptr,
                                             nullptr, dh)));
  SMT_CHECK_LAUNCH("ch_rows_bwd");
  const ChSlices s = ch_slices(rows);
  double* dbslab = reinterpret_cast<double*>(scratch);            // [n][V] doubles first (8-byte aligned), then the slabs
  float* slab = reinterpret_cast<float*>(dbslab + (size_t)s.n * bins);
  const int vcols = CPr > 128 ? 32 : CH_VCOLS;
  const dim3 grid((bins + vcols - 1) / vcols, s.n);
  const size_t n = (size_t)bins * CPr;
  CH_DISPATCH(CPr, (ch_launch_dw<CP>(stream, grid, h, ws, ws + n, bias, tg, lse, coef, rows, channels, bins, s.rows, slab, dbslab)));
  SMT_CHECK_LAUNCH("ch_dw");
  const int total = bins * channels + bins;
  ch_dw_reduce_kernel<<<(total + 255) / 256, 256, 0, stream>>>(slab, dbslab, s.n, bins, channels, dweight, dbias);
  SMT_CHECK_LAUNCH("ch_dw_reduce");
  return 0;
}
