// Incremental decoding of the causal TransformerLM (TransformerLM.sample(causal=True)): one new token per step against a
// key/value cache, batch 1..32, fp32, eval mode (no dropout anywhere), head dim 32 or 64.
//
//   lm_decode_embed      emb[tokens[b, pos]] * sqrt(d) + pe[pos]
//   lm_decode_linear     out[B, N] = x[B, K] W[N, K]^T (+ bias) (ReLU): the weights are streamed once, B <= 32 rows ride along
//   lm_decode_attention  this step's k / v rows into the cache, softmax(q K[0..pos]^T / sqrt(dh)) V[0..pos]
//   lm_decode_sample     inverse-CDF draw from softmax(logits / sigma) with a uniform number from device memory
//   lm_decode_sample_filtered  the same draw over the top-k / nucleus (top-p) prefix of the codes ordered by logit
//   lm_decode_prefill_kv the keys / values of a whole prompt (batched in-projection) into cache rows 0..len-1
//   lm_decode_advance    pos += 1
//
// Everything that changes from step to step -- the position, the tokens, the uniforms -- lives in device memory: a step is
// a fixed sequence of launches with fixed arguments (what a captured graph replays).  `pos` follows the convention of the
// dropout keys of lm.hip: by value, overridden by *pos_dev when that pointer is non-NULL.  A position outside the buffers
// (which the host cannot check when it sits in device memory) makes a kernel return without touching memory.
// Sums are merged in fixed orders: no float atomics, the same inputs give the same bits.
#include <algorithm>

#include "lm_rope.h"

namespace smt {

constexpr int DEC_CHUNK = 256;               // cache rows per workgroup of the attention kernel
constexpr int dec_part(int dh) { return 4 + dh; }   // floats per partial softmax: m, z, 2 unused, o[dh] (16-byte aligned)
static inline bool dec_dh_ok(int dh) { return dh == 32 || dh == 64; }   // head dims, as in lm.hip
constexpr int DEC_ROWS = 8;                  // output columns per workgroup of the linear kernel
constexpr int DEC_KW = 128;                  // contraction elements per wave of the linear kernel (two per lane)
constexpr int DEC_KMAX = 16 * DEC_KW;        // ... and per launch (16 waves)
constexpr float DEC_LOG2E = 1.4426950408889634f;

typedef float f32x2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------------------ embedding
__global__ __launch_bounds__(256) void lm_decode_embed_kernel(const long long* __restrict__ tok, const float* __restrict__ emb,
                                                              const float* __restrict__ pe, float* __restrict__ out, int L_tok,
                                                              int D, int vocab_rows, int pe_rows, float mul, int pos,
                                                              const int* __restrict__ pos_dev) {
  if (pos_dev) pos = *pos_dev;
  if (pos < 0 || pos >= L_tok || pos >= pe_rows) return;
  const int b = blockIdx.x;
  const long long t = tok[(long long)b * L_tok + pos];
  const bool ok = t >= 0 && t < vocab_rows;                   // a token outside the table: NaN, never a read past it
  for (int c = threadIdx.x; c < D; c += 256)
    out[(size_t)b * D + c] = ok ? emb[t * D + c] * mul + pe[(size_t)pos * D + c] : NAN;
}

// ------------------------------------------------------------------------------------------------ skinny linear
// Sum 32 values per lane over the 64 lanes of a wave, leaving the total of value (lane >> 1) in v[0]: five
// halving exchanges (a lane keeps the half its lane bit selects and sends the other) and one plain exchange -- 32 shuffles
// instead of the 192 of 32 separate wave sums.  The order of the additions is fixed by the lane numbers.
template <int CNT>
__device__ __forceinline__ void dec_halve(float (&v)[32], int lane, int off) {
  const bool up = (lane & off) != 0;
#pragma unroll
  for (int i = 0; i < CNT / 2; ++i) {
    const float send = up ? v[i] : v[i + CNT / 2];
    const float keep = up ? v[i + CNT / 2] : v[i];
    v[i] = keep + __shfl_xor(send, off, 64);
  }
}
__device__ __forceinline__ void dec_reduce32(float (&v)[32], int lane) {
  dec_halve<32>(v, lane, 32);
  dec_halve<16>(v, lane, 16);
  dec_halve<8>(v, lane, 8);
  dec_halve<4>(v, lane, 4);
  dec_halve<2>(v, lane, 2);
  v[0] += __shfl_xor(v[0], 1, 64);
}

// A workgroup owns DEC_ROWS consecutive output columns n and all BP (>= B, a power of two) batch rows.  The contraction is
// split over its waves, DEC_KW elements each: a lane keeps its two x elements of every batch row in registers (2 BP) and
// streams two elements of each of the eight weight rows -- a wave reads 512 contiguous bytes per weight row, all eight
// loads in flight before the first product.  The 8 * BP per-lane products-of-two are summed over the lanes 32 at a
// time (dec_reduce32), then over the waves through LDS in wave order; bias and the activation (act: 0 none, 1 ReLU, 2 exact
// GELU) on the way out.  Products and sums are fp32 FMAs.  accumulate != 0 adds to `out` (the second and later launches of a contraction longer than DEC_KMAX).
template <int BP, int MAXT>
__global__ __launch_bounds__(MAXT) void lm_decode_linear_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                                const float* __restrict__ bias, float* out, int B, int N, int kc,
                                                                int ldx, int ldw, int act, int accumulate) {
  constexpr int R = 32 / BP;                                  // weight rows per group of 32 values
  __shared__ float red[MAXT / 64][DEC_ROWS * BP];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  const int k = w * DEC_KW + 2 * lane;
  const bool live = k < kc;
  const int n0 = blockIdx.x * DEC_ROWS;
  f32x2 wr[DEC_ROWS], xr[BP];
#pragma unroll
  for (int r = 0; r < DEC_ROWS; ++r) {
    const int n = min(n0 + r, N - 1);
    wr[r] = live ? *(const f32x2*)(W + (size_t)n * ldw + k) : f32x2{0.f, 0.f};
  }
#pragma unroll
  for (int b = 0; b < BP; ++b) xr[b] = (live && b < B) ? *(const f32x2*)(x + (size_t)b * ldx + k) : f32x2{0.f, 0.f};
#pragma unroll
  for (int g = 0; g < DEC_ROWS / R; ++g) {
    float v[32];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int b = 0; b < BP; ++b) v[r * BP + b] = fmaf(wr[g * R + r].x, xr[b].x, wr[g * R + r].y * xr[b].y);
    dec_reduce32(v, lane);
    if ((lane & 1) == 0) red[w][g * 32 + (lane >> 1)] = v[0];
  }
  __syncthreads();
  for (int t = threadIdx.x; t < DEC_ROWS * BP; t += blockDim.x) {
    const int n = n0 + t / BP, b = t % BP;
    float s = red[0][t];
    for (int ww = 1; ww < nw; ++ww) s += red[ww][t];
    if (n < N && b < B) {
      float* dst = out + (size_t)b * N + n;
      if (accumulate) s += *dst;
      if (bias) s += bias[n];
      *dst = act == 1 ? fmaxf(s, 0.f) : act == 2 ? 0.5f * s * (1.f + erff(s * 0.70710678118654752f)) : s;
    }
  }
}

// ------------------------------------------------------------------------------------------------ attention over the cache
// One (batch, head) scans contiguous rows of K and V [B, H, l_max, DH] (128 bytes at DH = 32, 256 at 64).  Workgroup (s, bh)
// takes cache rows [256 s, 256 s + 256) up to pos; LPR = DH / 4 lanes share a row, 16 bytes each, so a wave loads
// G = 64 / LPR rows = 1 KiB per instruction whatever the head dim, and takes 32 rows per trip: U = 32 / G K loads and as
// many V loads in flight (4 + 4 at DH = 32, 8 + 8 at 64).  A score costs log2 LPR shuffles and the V row needs none; every
// lane group keeps its own running maximum / sum / four output channels, merged over the G groups of a wave by shuffles,
// over the four waves through LDS in wave order, and over the workgroups by lm_decode_attn_merge_kernel in chunk order.
// (DH = 64 with 8 lanes per row and two f32x4 each would keep the shuffle counts of DH = 32, but a lane would then read
// 32 bytes at a 256-byte stride and carry eight output channels through every merge; 16 lanes keep the per-lane state,
// the 16-byte contiguous-per-lane load and the 1 KiB per instruction, for one more score shuffle and one fewer group merge.)
// The step's own k / v rows come from qkv (one wave stores them to the cache; no value read from cache row pos is used in
// this launch), rows beyond pos are never read.
// ROPE (model.position: rotary): the step's q and k are rotated at position pos as they are loaded -- a lane's four channels
// are two whole pairs, its (cos, sin, cos, sin) are 16 bytes of table row pos -- before the scale and before the store, so the
// cache holds rotated keys and cached rows are used as read.  A position outside the table: nothing is written, as for l_max.
struct DecAcc { float m, z; f32x4 o; };
__device__ __forceinline__ void dec_merge(DecAcc& a, float m2, float z2, const f32x4& o2) {
  const float mn = fmaxf(a.m, m2), ms = (mn == -INFINITY) ? 0.f : mn;
  const float e1 = __builtin_amdgcn_exp2f(a.m - ms), e2 = __builtin_amdgcn_exp2f(m2 - ms);
  a.z = a.z * e1 + z2 * e2;
  a.o = a.o * e1 + o2 * e2;
  a.m = mn;
}

template <int DH, bool ROPE>
__global__ __launch_bounds__(256) void lm_decode_attn_kernel(const float* __restrict__ qkv, float* kcache, float* vcache,
                                                             float* __restrict__ ctx, float* __restrict__ part, int H, int l_max,
                                                             int nsplit, const float* __restrict__ rope, int rope_rows, int pos,
                                                             const int* __restrict__ pos_dev) {
  constexpr int LPR = DH / 4, G = 64 / LPR, U = 32 / G;        // lanes per row, rows per load instruction, loads per trip
  if (pos_dev) pos = *pos_dev;
  if (pos < 0 || pos >= l_max) return;
  if (ROPE && pos >= rope_rows) return;
  const int s = blockIdx.x, bh = blockIdx.y, b = bh / H, h = bh % H, d = H * DH;
  const int c0 = s * DEC_CHUNK;
  if (c0 > pos) return;                                       // uniform: no visible row in this chunk (the merge skips it too)
  __shared__ float red[4][LPR][6];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane / LPR, c = lane % LPR;
  const float* qrow = qkv + (size_t)b * 3 * d + h * DH + 4 * c;
  f32x4 qn = *(const f32x4*)qrow, kn = *(const f32x4*)(qrow + d);
  const f32x4 vn = *(const f32x4*)(qrow + 2 * d);
  if (ROPE) {
    const f32x4 cs = *(const f32x4*)(rope + (size_t)pos * DH + 4 * c);
    qn = rope_rotate4(qn, cs, false);
    kn = rope_rotate4(kn, cs, false);
  }
  const f32x4 q = qn * (rsqrtf((float)DH) * DEC_LOG2E);        // base-2 scores: exp2 is one instruction
  float* kb = kcache + (size_t)bh * l_max * DH + 4 * c;
  float* vb = vcache + (size_t)bh * l_max * DH + 4 * c;
  if (pos - c0 < DEC_CHUNK && w == 0 && g == 0) {             // the chunk that holds row pos
    *(f32x4*)(kb + (size_t)pos * DH) = kn;
    *(f32x4*)(vb + (size_t)pos * DH) = vn;
  }
  const int end = min(pos, c0 + DEC_CHUNK - 1);               // last visible row of this chunk
  const int before = max(pos - 1, 0);
  DecAcc a{-INFINITY, 0.f, f32x4{0.f, 0.f, 0.f, 0.f}};
  for (int r0 = c0 + 32 * w; r0 <= end; r0 += 128) {
    f32x4 kf[U], vf[U];
    float sc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int row = min(r0 + G * u + g, end);
      const size_t off = (size_t)(row == pos ? before : row) * DH;   // row pos: a load that is thrown away, from a row < pos (or row 0)
      kf[u] = *(const f32x4*)(kb + off);
      vf[u] = *(const f32x4*)(vb + off);
      if (row == pos) { kf[u] = kn; vf[u] = vn; }
    }
    float mloc = -INFINITY;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float t = fmaf(q.x, kf[u].x, fmaf(q.y, kf[u].y, fmaf(q.z, kf[u].z, q.w * kf[u].w)));
#pragma unroll
      for (int off = 1; off < LPR; off <<= 1) t += __shfl_xor(t, off, 64);
      sc[u] = (r0 + G * u + g <= end) ? t : -INFINITY;
      mloc = fmaxf(mloc, sc[u]);
    }
    const float mn = fmaxf(a.m, mloc), ms = (mn == -INFINITY) ? 0.f : mn;
    const float corr = __builtin_amdgcn_exp2f(a.m - ms);       // a.m = -inf: 0
    a.z *= corr;
    a.o *= corr;
    a.m = mn;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float p = __builtin_amdgcn_exp2f(sc[u] - ms);     // masked: exp2(-inf) = 0
      a.z += p;
      a.o += vf[u] * p;
    }
  }
#pragma unroll
  for (int off = LPR; off < 64; off <<= 1) {
    const float m2 = __shfl_xor(a.m, off, 64), z2 = __shfl_xor(a.z, off, 64);
    f32x4 o2;
    o2.x = __shfl_xor(a.o.x, off, 64); o2.y = __shfl_xor(a.o.y, off, 64);
    o2.z = __shfl_xor(a.o.z, off, 64); o2.w = __shfl_xor(a.o.w, off, 64);
    dec_merge(a, m2, z2, o2);
  }
  if (g == 0) {
    float* r = red[w][c];
    r[0] = a.m; r[1] = a.z; r[2] = a.o.x; r[3] = a.o.y; r[4] = a.o.z; r[5] = a.o.w;
  }
  __syncthreads();
  if (w == 0 && g == 0) {
    DecAcc t{red[0][c][0], red[0][c][1], f32x4{red[0][c][2], red[0][c][3], red[0][c][4], red[0][c][5]}};
#pragma unroll
    for (int ww = 1; ww < 4; ++ww)
      dec_merge(t, red[ww][c][0], red[ww][c][1], f32x4{red[ww][c][2], red[ww][c][3], red[ww][c][4], red[ww][c][5]});
    if (nsplit == 1) {
      *(f32x4*)(ctx + (size_t)b * d + h * DH + 4 * c) = t.o * (1.f / t.z);    // row 0 is always visible: z > 0
    } else {
      float* dst = part + ((size_t)bh * nsplit + s) * dec_part(DH);
      if (c == 0) { dst[0] = t.m; dst[1] = t.z; }
      *(f32x4*)(dst + 4 + 4 * c) = t.o;
    }
  }
}

// ctx = sum over the chunks 0 .. pos / 256, in chunk order, of the partial softmaxes; a thread per (batch, head, channel)
template <int DH>
__global__ __launch_bounds__(256) void lm_decode_attn_merge_kernel(const float* __restrict__ part, float* __restrict__ ctx, int BH,
                                                                   int l_max, int nsplit, int pos, const int* __restrict__ pos_dev) {
  constexpr int PART = dec_part(DH);
  if (pos_dev) pos = *pos_dev;
  if (pos < 0 || pos >= l_max) return;
  const int t = blockIdx.x * 256 + threadIdx.x, bh = t / DH, c = t % DH;
  if (bh >= BH) return;
  const int ns = min(nsplit, pos / DEC_CHUNK + 1);
  const float* p = part + (size_t)bh * nsplit * PART;
  float mm = -INFINITY;
  for (int s = 0; s < ns; ++s) mm = fmaxf(mm, p[s * PART]);
  float z = 0.f, o = 0.f;
  for (int s = 0; s < ns; ++s) {
    const float e = __builtin_amdgcn_exp2f(p[s * PART] - mm);
    z = fmaf(p[s * PART + 1], e, z);
    o = fmaf(p[s * PART + 4 + c], e, o);
  }
  ctx[(size_t)bh * DH + c] = o / z;                           // [B, H * DH]: (b H + h) * DH + c
}

// ------------------------------------------------------------------------------------------------ sampler
// One wave per batch row; lane i owns the contiguous codes [i ch, (i + 1) ch), ch = ceil(V / 64).  p = exp((l - max) /
// sigma); the cumulative sum runs lane by lane (an inclusive scan of the lanes' totals, then along the lane's own codes),
// S is the scan's last element.  The code is the smallest k whose cumulative sum exceeds u S; if rounding leaves none
// (u S >= the last cumulative sum), the last k with p > 0.  FILTER: a code i with keep[i] == 0 has p = 0 and is never the
// answer (keep: LDS, one word per code, written by the filtered kernel below); nothing else differs, so "everything kept"
// draws the same code.
template <bool FILTER>
__device__ __forceinline__ int dec_draw(const float* __restrict__ l, const float* __restrict__ u, const unsigned* keep, int V,
                                        float inv_sigma, int lane) {
  const int ch = (V + 63) / 64, lo = min(V, lane * ch), hi = min(V, lo + ch);
  float m = -INFINITY;
  for (int i = lo; i < hi; ++i) m = fmaxf(m, l[i]);
  m = wave_max(m);
  float t = 0.f;
  int last = -1;
  for (int i = lo; i < hi; ++i) {
    float p = expf((l[i] - m) * inv_sigma);
    if (FILTER) p = keep[i] ? p : 0.f;
    t += p;
    if (p > 0.f) last = i;
  }
  float inc = t;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  const float thr = *u * __shfl(inc, 63, 64);
  float cum = __shfl_up(inc, 1, 64);
  if (lane == 0) cum = 0.f;
  int k = 0x7fffffff;
  for (int i = lo; i < hi; ++i) {
    float p = expf((l[i] - m) * inv_sigma);
    bool in = true;                                           // the scan's sums are not monotone to the last bit: a lane behind
    if (FILTER) {                                             // the kept codes may hold a sum above thr, and must not answer
      in = keep[i] != 0u;
      p = in ? p : 0.f;
    }
    cum += p;
    if (cum > thr && in && k == 0x7fffffff) k = i;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    k = min(k, __shfl_xor(k, o, 64));
    last = max(last, __shfl_xor(last, o, 64));
  }
  if (k == 0x7fffffff) k = max(last, 0);
  return k;
}

__global__ __launch_bounds__(256) void lm_decode_sample_kernel(const float* __restrict__ logits, const float* __restrict__ uni,
                                                               long long* __restrict__ tokens, long long* __restrict__ codes, int B,
                                                               int V, int L_tok, int n_steps, float inv_sigma, int token_offset,
                                                               int pos, const int* __restrict__ pos_dev) {
  if (pos_dev) pos = *pos_dev;
  if (pos < 0 || pos >= n_steps || pos + 1 >= L_tok) return;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= B) return;
  const int k = dec_draw<false>(logits + (size_t)b * V, uni + (size_t)pos * B + b, nullptr, V, inv_sigma, lane);
  if (lane == 0) {
    tokens[(size_t)b * L_tok + pos + 1] = k + token_offset;
    codes[(size_t)b * n_steps + pos] = k;
  }
}

// The same draw restricted to a kept set: the first n codes of the order pi (logit descending, then code index ascending).
//   candidates  the first K = min(top_k, V) codes of pi (top_k = 0: all V); W = their total weight w = exp((l - max) / sigma)
//   kept        top_p < 1: the smallest n >= 1 whose first-n weight is >= top_p W; else n = the number of candidates
// A prefix of pi is { key > T } plus the first r codes, by index, of { key == T }, where key is an order-preserving 32-bit
// image of the logit -- so no sort: T is found bit by bit, from the top, as the largest value whose count (top-k: >= K) or
// weight (top-p: >= top_p W) of { key >= T } still suffices; 32 passes each over the keys and weights in LDS (code i belongs
// to lane i % 64 here: conflict-free, and a lane reads back only what it wrote), a wave reduction after each pass.  Tied
// codes at T have one weight wT, so r is the smallest count with A + r wT >= top_p W (A: the weight above T), found by
// bisection; their ranks by index come from ballots, 64 codes at a time.  Every sum runs lane-locally in index order and
// then through the same xor butterfly: a sum over fewer codes is never larger, which is what the bitwise search relies on.
constexpr int DEC_VMAX = 4096;               // vocabulary cap of the filtered sampler: 32 KiB of LDS per wave

__device__ __forceinline__ unsigned dec_key(float x) {
  const unsigned u = __float_as_uint(x + 0.f);                // -0 -> +0: equal logits, equal keys
  return max((u & 0x80000000u) ? ~u : (u | 0x80000000u), 1u); // 0 is kept free: it marks a code outside the candidates
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// weight resp. number of the codes with key >= t (ge) or key > t (!ge)
__device__ __forceinline__ float dec_mass(const unsigned* key, const float* wt, int V, int lane, unsigned t, bool ge) {
  float s = 0.f;
  for (int i = lane; i < V; i += 64) s += (ge ? key[i] >= t : key[i] > t) ? wt[i] : 0.f;
  return wave_sum(s);
}
__device__ __forceinline__ int dec_count(const unsigned* key, int V, int lane, unsigned t, bool ge) {
  int c = 0;
  for (int i = lane; i < V; i += 64) c += (ge ? key[i] >= t : key[i] > t) ? 1 : 0;
  return wave_sum_i(c);
}
// key[i] = 0 for every code outside { key > t } + the first r, by index, of { key == t }; `flag`: 1 for the codes inside
__device__ __forceinline__ void dec_cut(unsigned* key, float* wt, int V, int lane, unsigned t, int r, bool flag) {
  int seen = 0;
  for (int i0 = 0; i0 < V; i0 += 64) {                        // uniform trip count: the ballot needs the whole wave
    const int i = i0 + lane;
    const unsigned kv = i < V ? key[i] : 0u;
    const bool eq = i < V && kv == t;
    const unsigned long long tied = __ballot(eq);
    const int rank = seen + __popcll(tied & ((1ull << lane) - 1ull));
    seen += __popcll(tied);
    if (i < V) {
      const bool in = kv > t || (eq && rank < r);
      key[i] = in ? (flag ? 1u : kv) : 0u;
      if (!in) wt[i] = 0.f;
    }
  }
}

__global__ __launch_bounds__(64) void lm_decode_sample_filtered_kernel(const float* __restrict__ logits, const float* __restrict__ uni,
                                                                       long long* __restrict__ tokens, long long* __restrict__ codes,
                                                                       int* __restrict__ kept, int B, int V, int L_tok, int n_steps,
                                                                       float inv_sigma, int token_offset, int top_k, float top_p, int pos,
                                                                       const int* __restrict__ pos_dev) {
  if (pos_dev) pos = *pos_dev;
  if (pos < 0 || pos >= n_steps || pos + 1 >= L_tok) return;
  __shared__ unsigned key[DEC_VMAX];
  __shared__ float wt[DEC_VMAX];
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* l = logits + (size_t)b * V;
  float m = -INFINITY;
  for (int i = lane; i < V; i += 64) m = fmaxf(m, l[i]);
  m = wave_max(m);
  for (int i = lane; i < V; i += 64) {
    key[i] = dec_key(l[i]);
    wt[i] = expf((l[i] - m) * inv_sigma);
  }
  int n = V;
  if (top_k > 0 && top_k < V) {                               // T = the top_k-th largest key
    unsigned t = 0u;
    for (unsigned bit = 0x80000000u; bit; bit >>= 1)
      if (dec_count(key, V, lane, t | bit, true) >= top_k) t |= bit;
    dec_cut(key, wt, V, lane, t, top_k - dec_count(key, V, lane, t, false), false);
    n = top_k;
  }
  if (top_p < 1.f) {
    const float target = top_p * dec_mass(key, wt, V, lane, 0u, true);      // top_p W: a code outside the candidates has weight 0
    unsigned t = 0u;
    for (unsigned bit = 0x80000000u; bit; bit >>= 1)
      if (dec_mass(key, wt, V, lane, t | bit, true) >= target) t |= bit;
    const float above = dec_mass(key, wt, V, lane, t, false);
    const int n_above = dec_count(key, V, lane, t, false), n_tied = dec_count(key, V, lane, t, true) - n_above;
    float w_tied = 0.f;
    for (int i = lane; i < V; i += 64) w_tied = fmaxf(w_tied, key[i] == t ? wt[i] : 0.f);
    w_tied = wave_max(w_tied);
    int lo = 1, hi = max(n_tied, 1);                          // the smallest r in 1..n_tied with above + r w_tied >= target, else n_tied
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (fmaf((float)mid, w_tied, above) >= target) hi = mid; else lo = mid + 1;
    }
    dec_cut(key, wt, V, lane, t, lo, true);
    n = n_above + lo;
  } else {
    for (int i = lane; i < V; i += 64) key[i] = key[i] != 0u;
  }
  __syncthreads();                                            // the draw reads the flags of contiguous codes: other lanes' words
  const int k = dec_draw<true>(l, uni + (size_t)pos * B + b, key, V, inv_sigma, lane);
  if (lane == 0) {
    tokens[(size_t)b * L_tok + pos + 1] = k + token_offset;
    codes[(size_t)b * n_steps + pos] = k;
    if (kept) kept[(size_t)pos * B + b] = n;
  }
}

// ------------------------------------------------------------------------------------------------ prompt keys / values
// The k and v thirds of qkv [B, L, 3 H DH] (what the batched in-projection of a prompt produces) into rows 0..L-1 of the caches
// [B, H, l_max, DH]: a thread moves 16 bytes of k and 16 of v, DH / 4 threads a row; consecutive threads write consecutive
// 16 bytes of a (batch, head)'s cache rows (a wave stores 1 KiB contiguous) and read 4 DH-byte pieces of the qkv rows.
// Rows >= L are not touched.
template <int DH>
__global__ __launch_bounds__(256) void lm_decode_prefill_kv_kernel(const float* __restrict__ qkv, float* __restrict__ kcache,
                                                                   float* __restrict__ vcache, int L, int H, int l_max) {
  constexpr int LPR = DH / 4;
  const int t = blockIdx.x * 256 + threadIdx.x, row = t / LPR, c = t % LPR;
  if (row >= L) return;
  const int bh = blockIdx.y, b = bh / H, h = bh % H, d = H * DH;
  const float* src = qkv + ((size_t)b * L + row) * 3 * d + d + h * DH + 4 * c;
  const size_t dst = ((size_t)bh * l_max + row) * DH + 4 * c;
  const f32x4 kk = *(const f32x4*)src, vv = *(const f32x4*)(src + d);
  *(f32x4*)(kcache + dst) = kk;
  *(f32x4*)(vcache + dst) = vv;
}

__global__ void lm_decode_advance_kernel(int* pos_dev) {
  if (threadIdx.x == 0 && blockIdx.x == 0) pos_dev[0] += 1;
}

static int dec_splits(int l_max) { return (l_max + DEC_CHUNK - 1) / DEC_CHUNK; }

template <int BP>
static void dec_linear_launch(const float* x, const float* w, const float* bias, float* out, int B, int N, int kc, int ld, int act,
                              int accumulate, hipStream_t stream) {
  const int nw = (kc + DEC_KW - 1) / DEC_KW, grid = (N + DEC_ROWS - 1) / DEC_ROWS;
  if (nw <= 4)
    lm_decode_linear_kernel<BP, 256><<<grid, 64 * nw, 0, stream>>>(x, w, bias, out, B, N, kc, ld, ld, act, accumulate);
  else
    lm_decode_linear_kernel<BP, 1024><<<grid, 64 * nw, 0, stream>>>(x, w, bias, out, B, N, kc, ld, ld, act, accumulate);
}

}  // namespace smt

using namespace smt;

extern "C" int smt_lm_decode_embed(const int64_t* tokens, const float* emb, const float* pe, float* out, int batch, int tok_len,
                                   int dim, int vocab_rows, int pe_rows, float mul, int pos, const int* pos_dev, smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SMT_CHECK_ARG(tokens && emb && pe && out, "smt_lm_decode_embed: null pointer");
  SMT_CHECK_ARG(batch >= 1 && batch <= 32 && tok_len >= 1 && dim >= 1 && vocab_rows >= 1 && pe_rows >= 1,
                "smt_lm_decode_embed: batch must be 1..32 and every size positive (batch %d)", batch);
  SMT_CHECK_ARG(pos_dev || (pos >= 0 && pos < tok_len && pos < pe_rows), "smt_lm_decode_embed: pos %d outside the token buffer (%d) or the position table (%d)",
                pos, tok_len, pe_rows);
  lm_decode_embed_kernel<<<batch, 256, 0, stream>>>((const long long*)tokens, emb, pe, out, tok_len, dim, vocab_rows, pe_rows, mul, pos, pos_dev);
  SMT_CHECK_LAUNCH("lm_decode_embed");
  return 0;
}

extern "C" int smt_lm_decode_linear(const float* x, const float* w, const float* bias, float* out, int batch, int in_dim, int out_dim,
                                    int act, smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SMT_CHECK_ARG(x && w && out, "smt_lm_decode_linear: null pointer");
  SMT_CHECK_ARG(batch >= 1 && batch <= 32, "smt_lm_decode_linear: batch must be 1..32 (got %d)", batch);
  SMT_CHECK_ARG(in_dim >= 64 && in_dim % 64 == 0 && out_dim >= 1, "smt_lm_decode_linear: in_dim must be a positive multiple of 64, out_dim >= 1 (got %d, %d)",
                in_dim, out_dim);
  SMT_CHECK_ARG(act >= 0 && act <= 2, "smt_lm_decode_linear: act must be 0 (none), 1 (ReLU) or 2 (GELU) (got %d)", act);
  for (int k0 = 0; k0 < in_dim; k0 += DEC_KMAX) {
    const int kc = std::min(DEC_KMAX, in_dim - k0), last = k0 + kc == in_dim;
    const float* bl = last ? bias : nullptr;
    const int rl = last ? act : 0, acc = k0 > 0;
    if (batch <= 4) dec_linear_launch<4>(x + k0, w + k0, bl, out, batch, out_dim, kc, in_dim, rl, acc, stream);
    else if (batch <= 8) dec_linear_launch<8>(x + k0, w + k0, bl, out, batch, out_dim, kc, in_dim, rl, acc, stream);
    else if (batch <= 16) dec_linear_launch<16>(x + k0, w + k0, bl, out, batch, out_dim, kc, in_dim, rl, acc, stream);
    else dec_linear_launch<32>(x + k0, w + k0, bl, out, batch, out_dim, kc, in_dim, rl, acc, stream);
    SMT_CHECK_LAUNCH("lm_decode_linear");
  }
  return 0;
}

extern "C" size_t smt_lm_decode_attention_hd_workspace_bytes(int batch, int heads, int l_max, int head_dim) {
  if (batch <= 0 || heads <= 0 || l_max <= 0 || !dec_dh_ok(head_dim) || dec_splits(l_max) == 1) return 0;
  return (size_t)batch * heads * dec_splits(l_max) * dec_part(head_dim) * sizeof(float);
}
extern "C" size_t smt_lm_decode_attention_workspace_bytes(int batch, int heads, int l_max) {
  return smt_lm_decode_attention_hd_workspace_bytes(batch, heads, l_max, 32);
}

// rope == NULL: the kernel without the rotation (the launch of smt_lm_decode_attention_hd).  The merge kernel uses its row
// limit for nothing but the "write nothing" rule, so with a table it gets min(l_max, rope_rows).
template <int DH>
static int dec_attention_launch(const float* qkv, float* k_cache, float* v_cache, float* ctx, void* workspace, int batch, int heads,
                                int l_max, int nsplit, const float* rope, int rope_rows, int pos, const int* pos_dev, hipStream_t stream) {
  const dim3 grid(nsplit, batch * heads);
  if (rope)
    lm_decode_attn_kernel<DH, true><<<grid, 256, 0, stream>>>(qkv, k_cache, v_cache, ctx, (float*)workspace, heads, l_max, nsplit, rope, rope_rows, pos, pos_dev);
  else
    lm_decode_attn_kernel<DH, false><<<grid, 256, 0, stream>>>(qkv, k_cache, v_cache, ctx, (float*)workspace, heads, l_max, nsplit, nullptr, 0, pos, pos_dev);
  SMT_CHECK_LAUNCH("lm_decode_attention");
  if (nsplit > 1) {
    const int limit = rope ? std::min(l_max, rope_rows) : l_max;
    lm_decode_attn_merge_kernel<DH><<<(batch * heads * DH + 255) / 256, 256, 0, stream>>>((const float*)workspace, ctx, batch * heads, limit, nsplit, pos, pos_dev);
    SMT_CHECK_LAUNCH("lm_decode_attention_merge");
  }
  return 0;
}

extern "C" int smt_lm_decode_attention_rope(const float* qkv, float* k_cache, float* v_cache, float* ctx, void* workspace,
                                            size_t workspace_bytes, int batch, int heads, int l_max, int head_dim, const float* rope,
                                            int rope_rows, int pos, const int* pos_dev, smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SMT_CHECK_ARG(dec_dh_ok(head_dim), "smt_lm_decode_attention: head dim must be 32 or 64 (got %d)", head_dim);
  SMT_CHECK_ARG(qkv && k_cache && v_cache && ctx, "smt_lm_decode_attention: null pointer");
  SMT_CHECK_ARG(batch >= 1 && batch <= 32 && heads >= 1 && l_max >= 1, "smt_lm_decode_attention: batch must be 1..32, heads and l_max positive");
  SMT_CHECK_ARG((long long)batch * heads <= 65535 && (long long)l_max * head_dim < (1ll << 31),
                "smt_lm_decode_attention: batch * heads <= 65535, l_max * head dim < 2^31");
  SMT_CHECK_ARG(pos_dev || (pos >= 0 && pos < l_max), "smt_lm_decode_attention: pos %d outside the cache (%d rows)", pos, l_max);
  SMT_CHECK_ARG(!rope || (rope_rows >= 1 && (uintptr_t)rope % 16 == 0), "smt_lm_decode_attention: the rope table needs rope_rows >= 1 and a 16-byte aligned address");
  SMT_CHECK_ARG(!rope || pos_dev || pos < rope_rows, "smt_lm_decode_attention: pos %d outside the rope table (%d rows)", pos, rope_rows);
  const int nsplit = dec_splits(l_max);
  SMT_CHECK_ARG(nsplit == 1 || (workspace && workspace_bytes >= smt_lm_decode_attention_hd_workspace_bytes(batch, heads, l_max, head_dim)),
                "smt_lm_decode_attention: workspace too small");
  return head_dim == 32 ? dec_attention_launch<32>(qkv, k_cache, v_cache, ctx, workspace, batch, heads, l_max, nsplit, rope, rope_rows, pos, pos_dev, stream)
                        : dec_attention_launch<64>(qkv, k_cache, v_cache, ctx, workspace, batch, heads, l_max, nsplit, rope, rope_rows, pos, pos_dev, stream);
}
extern "C" int smt_lm_decode_attention_hd(const float* qkv, float* k_cache, float* v_cache, float* ctx, void* workspace,
                                          size_t workspace_bytes, int batch, int heads, int l_max, int head_dim, int pos,
                                          const int* pos_dev, smt_stream_t stream) {
  return smt_lm_decode_attention_rope(qkv, k_cache, v_cache, ctx, workspace, workspace_bytes, batch, heads, l_max, head_dim, nullptr, 0, pos,
                                      pos_dev, stream);
}
extern "C" int smt_lm_decode_attention(const float* qkv, float* k_cache, float* v_cache, float* ctx, void* workspace,
                                       size_t workspace_bytes, int batch, int heads, int l_max, int pos, const int* pos_dev,
                                       smt_stream_t stream) {
  return smt_lm_decode_attention_hd(qkv, k_cache, v_cache, ctx, workspace, workspace_bytes, batch, heads, l_max, 32, pos, pos_dev, stream);
}

extern "C" int smt_lm_decode_sample(const float* logits, const float* uniforms, int64_t* tokens, int64_t* codes, int batch, int vocab,
                                    int tok_len, int n_steps, float inv_sigma, int token_offset, int pos, const int* pos_dev,
                                    smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SMT_CHECK_ARG(logits && uniforms && tokens && codes, "smt_lm_decode_sample: null pointer");
  SMT_CHECK_ARG(batch >= 1 && batch <= 32 && vocab >= 1 && n_steps >= 1 && tok_len >= 2, "smt_lm_decode_sample: batch must be 1..32, vocab and n_steps positive");
  SMT_CHECK_ARG(inv_sigma > 0.f, "smt_lm_decode_sample: 1 / sigma must be positive");
  SMT_CHECK_ARG(pos_dev || (pos >= 0 && pos < n_steps && pos + 1 < tok_len), "smt_lm_decode_sample: pos %d outside the uniforms (%d rows) or the token buffer (%d)",
                pos, n_steps, tok_len);
  lm_decode_sample_kernel<<<(batch + 3) / 4, 256, 0, stream>>>(logits, uniforms, (long long*)tokens, (long long*)codes, batch, vocab, tok_len, n_steps,
                                                             inv_sigma, token_offset, pos, pos_dev);
  SMT_CHECK_LAUNCH("lm_decode_sample");
  return 0;
}

extern "C" int smt_lm_decode_sample_filtered(const float* logits, const float* uniforms, int64_t* tokens, int64_t* codes, int batch,
                                             int vocab, int tok_len, int n_steps, float inv_sigma, int token_offset, int top_k,
                                             float top_p, int32_t* kept, int pos, const int* pos_dev, smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SMT_CHECK_ARG(logits && uniforms && tokens && codes, "smt_lm_decode_sample_filtered: null pointer");
  SMT_CHECK_ARG(batch >= 1 && batch <= 32 && vocab >= 1 && n_steps >= 1 && tok_len >= 2,
                "smt_lm_decode_sample_filtered: batch must be 1..32, vocab and n_steps positive");
  SMT_CHECK_ARG(vocab <= DEC_VMAX, "smt_lm_decode_sample_filtered: vocab %d above the cap of %d", vocab, DEC_VMAX);
  SMT_CHECK_ARG(inv_sigma > 0.f, "smt_lm_decode_sample_filtered: 1 / sigma must be positive");
  SMT_CHECK_ARG(top_k >= 0, "smt_lm_decode_sample_filtered: top_k must be >= 0 (0 = off; got %d)", top_k);
  SMT_CHECK_ARG(top_p > 0.f && top_p <= 1.f, "smt_lm_decode_sample_filtered: top_p must lie in (0, 1] (1 = off; got %g)", (double)top_p);
  SMT_CHECK_ARG(pos_dev || (pos >= 0 && pos < n_steps && pos + 1 < tok_len),
                "smt_lm_decode_sample_filtered: pos %d outside the uniforms (%d rows) or the token buffer (%d)", pos, n_steps, tok_len);
  lm_decode_sample_filtered_kernel<<<batch, 64, 0, stream>>>(logits, uniforms, (long long*)tokens, (long long*)codes, kept, batch, vocab, tok_len,
                                                             n_steps, inv_sigma, token_offset, top_k, top_p, pos, pos_dev);
  SMT_CHECK_LAUNCH("lm_decode_sample_filtered");
  return 0;
}

extern "C" int smt_lm_decode_prefill_kv_hd(const float* qkv, float* k_cache, float* v_cache, int batch, int len, int heads, int l_max,
                                           int head_dim, smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SMT_CHECK_ARG(dec_dh_ok(head_dim), "smt_lm_decode_prefill_kv: head dim must be 32 or 64 (got %d)", head_dim);
  SMT_CHECK_ARG(qkv && k_cache && v_cache, "smt_lm_decode_prefill_kv: null pointer");
  SMT_CHECK_ARG(batch >= 1 && batch <= 32 && heads >= 1 && l_max >= 1, "smt_lm_decode_prefill_kv: batch must be 1..32, heads and l_max positive");
  SMT_CHECK_ARG((long long)batch * heads <= 65535 && (long long)l_max * head_dim < (1ll << 31),
                "smt_lm_decode_prefill_kv: batch * heads <= 65535, l_max * head dim < 2^31");
  SMT_CHECK_ARG(len >= 1 && len <= l_max, "smt_lm_decode_prefill_kv: len %d outside 1..l_max = %d", len, l_max);
  const dim3 grid((unsigned)(((long long)len * (head_dim / 4) + 255) / 256), batch * heads);
  if (head_dim == 32) lm_decode_prefill_kv_kernel<32><<<grid, 256, 0, stream>>>(qkv, k_cache, v_cache, len, heads, l_max);
  else lm_decode_prefill_kv_kernel<64><<<grid, 256, 0, stream>>>(qkv, k_cache, v_cache, len, heads, l_max);
  SMT_CHECK_LAUNCH("lm_decode_prefill_kv");
  return 0;
}
extern "C" int smt_lm_decode_prefill_kv(const float* qkv, float* k_cache, float* v_cache, int batch, int len, int heads, int l_max,
                                        smt_stream_t stream) {
  return smt_lm_decode_prefill_kv_hd(qkv, k_cache, v_cache, batch, len, heads, l_max, 32, stream);
}

extern "C" int smt_lm_decode_advance(int* pos_dev, smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SMT_CHECK_ARG(pos_dev, "smt_lm_decode_advance: null pointer");
  lm_decode_advance_kernel<<<1, 64, 0, stream>>>(pos_dev);
  SMT_CHECK_LAUNCH("lm_decode_advance");
  return 0;
}
