// WaveNet block (reference models/vqvae/resnet.py:123-181): the gate a = tanh(t) * sigmoid(s) and the fused tail of one layer.
//   * wavenet_gate_fwd / _bwd   elementwise over z [B, T, 2H] (t = first half of a row, s = second half), fp32 and bf16:
//                               one pass with 16-byte accesses along the channel axis, rows >= lens[b] written as 0, never read
//   * wavenet_tail_fwd          bf16, H in {64, 128}:  y = keep * (x + bias + W_g . (tanh t * sigmoid s)) in one pass.  One wave
//                               owns 32 rows; lane (r, hh) loads the 16-byte pieces 2s + hh of the two halves of row r of z, gates
//                               them in fp32 and rounds once to bf16: that IS the B fragment of k-step s of
//                               mfma_f32_32x32x16_bf16 (B[k = 8 hh + j][col r]), so `a` never touches LDS or memory.  W_g is the A
//                               operand (transposed product, y^T = W_g a^T), staged once per workgroup in LDS with a padded pitch;
//                               the accumulator starts at x + bias, and the transposed 32 x 32 result is paired up across lane
//                               halves (pair_up8) and stored in 16-byte pieces.
// No atomics, no workspace, one launch each; the result of an element depends on its own row alone (bitwise reproducible).
#include "conv_common.h"

namespace smt {

// tanh(t) * sigmoid(s) and the two factors.  E = exp(-2t), S = exp(-s) on the hardware exp2 (v_exp_f32, 1 ulp):
//   tanh t = (1 - E) / (1 + E),  sigmoid s = 1 / (1 + S).
// t is clamped at -15 (tanh(-15) rounds to -1 in fp32) so that E stays finite; below |t| = 1/16 the numerator 1 - E cancels,
// so tanh is taken from its series t (1 - t^2 / 3) there (truncation 2 t^4 / 15 <= 2.1e-6 relative): the result keeps a small
// RELATIVE error for small t, which the bf16 bound needs.  DESIGN.md section 20 derives the error bounds from this text.
constexpr float WN_LOG2E = 1.4426950408889634f;
constexpr float WN_SMALL_T = 0.0625f;

struct WnParts { float num, e1; };     // tanh t = num / e1 with e1 = 1 + E
__device__ __forceinline__ WnParts wn_tanh_parts(float t) {
  const float e = __builtin_amdgcn_exp2f(fmaxf(t, -15.f) * (-2.f * WN_LOG2E));
  const float e1 = 1.f + e;
  const float series = t * (1.f - t * t * (1.f / 3.f)) * e1;
  return {fabsf(t) < WN_SMALL_T ? series : 1.f - e, e1};
}
// forward: ONE reciprocal for both factors (three transcendentals per element instead of four)
__device__ __forceinline__ float wn_gate(float t, float s) {
  const WnParts p = wn_tanh_parts(t);
  const float s1 = 1.f + __builtin_amdgcn_exp2f(s * -WN_LOG2E);
  return p.num * __builtin_amdgcn_rcpf(p.e1 * s1);
}
__device__ __forceinline__ void wn_gate_grad(float t, float s, float da, float& dt, float& ds) {
  const WnParts p = wn_tanh_parts(t);
  const float th = p.num * __builtin_amdgcn_rcpf(p.e1);
  const float sg = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(s * -WN_LOG2E));
  dt = da * (sg * (1.f - th * th));
  ds = da * (th * (sg * (1.f - sg)));
}

struct WnArgs {
  const void* z; const void* da; void* out;      // out = a (forward) or dz (backward)
  long long bs_z, bs_da, bs_out;
  int ld_z, ld_da, ld_out;
  const int* lens;
  int batch, t, hidden;
};

// one lane per 16-byte vector of the H-wide side (a, da); BWD writes both halves of the dz row
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void wavenet_gate_kernel(WnArgs p) {
  constexpr int EPV = Tr<T>::EPV;
  typedef Vec<T, EPV> V;
  const int vpr = p.hidden / EPV;
  const long long total = (long long)p.batch * p.t * vpr;
  const T* z = (const T*)p.z;
  const T* da = (const T*)p.da;
  T* out = (T*)p.out;
  for (long long f = (long long)blockIdx.x * 256 + threadIdx.x; f < total; f += (long long)gridDim.x * 256) {
    const int row = (int)(f / vpr);
    const int c = (int)(f - (long long)row * vpr) * EPV;
    const int b = row / p.t, tt = row - b * p.t;
    const bool keep = p.lens == nullptr || tt < p.lens[b];
    const long long oz = b * p.bs_z + (long long)tt * p.ld_z + c;
    const long long oo = b * p.bs_out + (long long)tt * p.ld_out + c;
    V o0, o1;
    if (keep) {
      const V tv = *reinterpret_cast<const V*>(z + oz);
      const V sv = *reinterpret_cast<const V*>(z + oz + p.hidden);
      if constexpr (BWD) {
        const V dv = *reinterpret_cast<const V*>(da + b * p.bs_da + (long long)tt * p.ld_da + c);
#pragma unroll
        for (int e = 0; e < EPV; ++e) {
          float dt, ds;
          wn_gate_grad((float)tv.v[e], (float)sv.v[e], (float)dv.v[e], dt, ds);
          o0.v[e] = (T)dt; o1.v[e] = (T)ds;
        }
      } else {
#pragma unroll
        for (int e = 0; e < EPV; ++e) o0.v[e] = (T)wn_gate((float)tv.v[e], (float)sv.v[e]);
      }
    } else {
#pragma unroll
      for (int e = 0; e < EPV; ++e) { o0.v[e] = (T)0.f; o1.v[e] = (T)0.f; }
    }
    *reinterpret_cast<V*>(out + oo) = o0;
    if constexpr (BWD) *reinterpret_cast<V*>(out + oo + p.hidden) = o1;
  }
}

// ------------------------------------------------------------------------------------------------ fused tail
struct WnTailArgs {
  const __bf16* z; const __bf16* x; const __bf16* w; const float* bias; __bf16* y;
  long long bs_z, bs_x, bs_y;
  int ld_z, ld_x, ld_y;
  const int* lens;
  int batch, t, tiles_per_item, ntiles;
};

constexpr int WT_ROWS = 32;      // rows per wave tile (the N side of the transposed 32 x 32 MFMA)
constexpr int WT_WAVES = 4;

template <int H>
__global__ __launch_bounds__(64 * WT_WAVES) void wavenet_tail_kernel(WnTailArgs p) {
  constexpr int LDW = H + 8;     // LDS pitch of W_g: 16 bytes of padding per row spread the 32 rows of a fragment read over the banks
  constexpr int KS = H / 16;     // k-steps
  constexpr int NB = H / 32;     // 32-channel output blocks
  __shared__ __attribute__((aligned(16))) __bf16 w_lds[H * LDW];
  __shared__ __attribute__((aligned(16))) float b_lds[H];
  for (int v = threadIdx.x; v < H * H / 8; v += 64 * WT_WAVES) {
    const int o = v / (H / 8), c = v - o * (H / 8);
    *reinterpret_cast<bf16x8*>(&w_lds[o * LDW + 8 * c]) = reinterpret_cast<const bf16x8*>(p.w)[v];
  }
  for (int i = threadIdx.x; i < H; i += 64 * WT_WAVES) b_lds[i] = p.bias ? p.bias[i] : 0.f;
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, hh = lane >> 5;
  for (long long tile = blockIdx.x * WT_WAVES + wave; tile < p.ntiles; tile += gridDim.x * WT_WAVES) {
    const int b = __builtin_amdgcn_readfirstlane((int)(tile / p.tiles_per_item));
    const int t0 = __builtin_amdgcn_readfirstlane((int)(tile - (long long)b * p.tiles_per_item) * WT_ROWS);
    const int len = p.lens ? min(p.lens[b], p.t) : p.t;
    const int row = t0 + r;
    const bool live = row < len;             // rows at or past lens[b]: z and x are not read, y = 0
    const bool inside = row < p.t;
    __bf16* yrow = p.y + b * p.bs_y + (long long)row * p.ld_y + 8 * hh;
    if (t0 >= len) {                         // wave-uniform: nothing of this tile is valid
      if (inside) {
        const i32x4v zero = {0, 0, 0, 0};
#pragma unroll
        for (int n = 0; n < NB; ++n) {
          *reinterpret_cast<i32x4v*>(yrow + 32 * n) = zero;
          *reinterpret_cast<i32x4v*>(yrow + 32 * n + 16) = zero;
        }
      }
      continue;
    }
    const __bf16* zrow = p.z + b * p.bs_z + (long long)row * p.ld_z + 8 * hh;
    const __bf16* xrow = p.x + b * p.bs_x + (long long)row * p.ld_x + 4 * hh;
    bf16x8 zt[KS], zs[KS];
    bf16x4 xv[NB][4];
    if (live) {
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        zt[s] = *reinterpret_cast<const bf16x8*>(zrow + 16 * s);
        zs[s] = *reinterpret_cast<const bf16x8*>(zrow + H + 16 * s);
      }
#pragma unroll
      for (int n = 0; n < NB; ++n)
#pragma unroll
        for (int g = 0; g < 4; ++g) xv[n][g] = *reinterpret_cast<const bf16x4*>(xrow + 32 * n + 8 * g);
    } else {
#pragma unroll
      for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) { zt[s][j] = (__bf16)0.f; zs[s][j] = (__bf16)0.f; }
#pragma unroll
      for (int n = 0; n < NB; ++n)
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int i = 0; i < 4; ++i) xv[n][g][i] = (__bf16)0.f;
    }
    // accumulator element e of block n is channel 32 n + 8 (e >> 2) + 4 hh + (e & 3) of row r: start it at x + bias
    f32x16 acc[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(&b_lds[32 * n + 8 * g + 4 * hh]);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[n][4 * g + i] = (float)xv[n][g][i] + bv[i];
      }
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      bf16x8 a;                                 // gated in fp32, rounded to bf16 once: the B fragment of k-step s
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = (__bf16)wn_gate((float)zt[s][j], (float)zs[s][j]);
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        const bf16x8 wf = *reinterpret_cast<const bf16x8*>(&w_lds[(32 * n + r) * LDW + 16 * s + 8 * hh]);
        acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, a, acc[n], 0, 0, 0);
      }
    }
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      unsigned v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = live ? pack_bf16x2(acc[n][2 * q], acc[n][2 * q + 1]) : 0u;
      pair_up8(v);                              // lane r: channels 0-7 | 16-23 of the block, lane r + 32: 8-15 | 24-31
      if (inside) {
        *reinterpret_cast<i32x4v*>(yrow + 32 * n) = i32x4v{(int)v[0], (int)v[1], (int)v[2], (int)v[3]};
        *reinterpret_cast<i32x4v*>(yrow + 32 * n + 16) = i32x4v{(int)v[4], (int)v[5], (int)v[6], (int)v[7]};
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ host side
struct WnTensor { const char* name; const void* p; long long bs; int ld; int width; bool output; };

static bool wn_overlap(const WnTensor& a, const WnTensor& b, long long batch, long long t, size_t esz) {
  const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
  const uintptr_t a1 = a0 + (uintptr_t)(((batch - 1) * a.bs + (t - 1) * a.ld + a.width) * (long long)esz);
  const uintptr_t b1 = b0 + (uintptr_t)(((batch - 1) * b.bs + (t - 1) * b.ld + b.width) * (long long)esz);
  return a0 < b1 && b0 < a1;
}

// The limits every entry of this file shares, decided before any launch.  Returns 0 (go on), 1 (argument error) or -1 (no rows).
static int wn_check(const char* fn, const WnTensor* ts, int n, int batch, int t, int hidden, int dtype, bool tail) {
  if (tail) SMT_CHECK_ARG(hidden == 64 || hidden == 128, "%s: hidden=%d must be 64 or 128", fn, hidden);
  else SMT_CHECK_ARG(hidden >= 8 && hidden % 8 == 0, "%s: hidden=%d must be a positive multiple of 8", fn, hidden);
  SMT_CHECK_ARG(dtype == SMT_F32 || dtype == SMT_BF16, "%s: dtype=%d must be SMT_F32 (0) or SMT_BF16 (1)", fn, dtype);
  SMT_CHECK_ARG(batch >= 0 && t >= 0, "%s: batch=%d and t=%d must not be negative", fn, batch, t);
  SMT_CHECK_ARG((long long)batch * t < (1ll << 31), "%s: batch * t = %lld rows must be at most 2^31 - 1", fn,
                (long long)batch * t);
  if ((long long)batch * t == 0) return -1;
  const size_t esz = dtype == SMT_BF16 ? 2 : 4;
  for (int i = 0; i < n; ++i) {
    const WnTensor& a = ts[i];
    SMT_CHECK_ARG(a.p != nullptr, "%s: null pointer (%s)", fn, a.name);
    SMT_CHECK_ARG(((uintptr_t)a.p & 15) == 0, "%s: %s must be 16-byte aligned", fn, a.name);
    SMT_CHECK_ARG(a.ld >= a.width, "%s: pitch ld_%s=%d is smaller than the row width %d", fn, a.name, a.ld, a.width);
    SMT_CHECK_ARG(a.ld % 8 == 0, "%s: pitch ld_%s=%d must be a multiple of 8 elements", fn, a.name, a.ld);
    SMT_CHECK_ARG(a.bs >= 0 && a.bs % 8 == 0, "%s: batch stride bs_%s=%lld must be a non-negative multiple of 8 elements", fn,
                  a.name, a.bs);
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j)
      if (ts[i].output && i != j)
        SMT_CHECK_ARG(!wn_overlap(ts[i], ts[j], batch, t, esz), "%s: %s must not alias %s", fn, ts[i].name, ts[j].name);
  return 0;
}

static int wn_grid(long long work_items) {
  return (int)std::min<long long>((work_items + 255) / 256, 256 * 16);
}

}  // namespace smt

using namespace smt;

extern "C" int smt_wavenet_gate_fwd(const void* z, int64_t bs_z, int ld_z, void* a, int64_t bs_a, int ld_a, const int* lens,
                                    int batch, int t, int hidden, int dtype, smt_stream_t stream_) {
  static const char* fn = "smt_wavenet_gate_fwd";
  const WnTensor ts[2] = {{"z", z, bs_z, ld_z, 2 * hidden, false}, {"a", a, bs_a, ld_a, hidden, true}};
  const int st = wn_check(fn, ts, 2, batch, t, hidden, dtype, false);
  if (st) return st < 0 ? 0 : st;
  hipStream_t stream = (hipStream_t)stream_;
  WnArgs p{z, nullptr, a, bs_z, 0, bs_a, ld_z, 0, ld_a, lens, batch, t, hidden};
  const int grid = wn_grid((long long)batch * t * (hidden / (dtype == SMT_BF16 ? 8 : 4)));
  if (dtype == SMT_BF16) wavenet_gate_kernel<__bf16, false><<<grid, 256, 0, stream>>>(p);
  else wavenet_gate_kernel<float, false><<<grid, 256, 0, stream>>>(p);
  SMT_CHECK_LAUNCH(fn);
  return 0;
}

extern "C" int smt_wavenet_gate_bwd(const void* z, int64_t bs_z, int ld_z, const void* da, int64_t bs_da, int ld_da, void* dz,
                                    int64_t bs_dz, int ld_dz, const int* lens, int batch, int t, int hidden, int dtype,
                                    smt_stream_t stream_) {
  static const char* fn = "smt_wavenet_gate_bwd";
  const WnTensor ts[3] = {{"z", z, bs_z, ld_z, 2 * hidden, false}, {"da", da, bs_da, ld_da, hidden, false},
                          {"dz", dz, bs_dz, ld_dz, 2 * hidden, true}};
  const int st = wn_check(fn, ts, 3, batch, t, hidden, dtype, false);
  if (st) return st < 0 ? 0 : st;
  hipStream_t stream = (hipStream_t)stream_;
  WnArgs p{z, da, dz, bs_z, bs_da, bs_dz, ld_z, ld_da, ld_dz, lens, batch, t, hidden};
  const int grid = wn_grid((long long)batch * t * (hidden / (dtype == SMT_BF16 ? 8 : 4)));
  if (dtype == SMT_BF16) wavenet_gate_kernel<__bf16, true><<<grid, 256, 0, stream>>>(p);
  else wavenet_gate_kernel<float, true><<<grid, 256, 0, stream>>>(p);
  SMT_CHECK_LAUNCH(fn);
  return 0;
}

extern "C" int smt_wavenet_tail_fwd(const void* z, int64_t bs_z, int ld_z, const void* x, int64_t bs_x, int ld_x,
                                    const void* w_packed, const float* bias, void* y, int64_t bs_y, int ld_y, const int* lens,
                                    int batch, int t, int hidden, smt_stream_t stream_) {
  static const char* fn = "smt_wavenet_tail_fwd";
  const WnTensor ts[3] = {{"z", z, bs_z, ld_z, 2 * hidden, false}, {"x", x, bs_x, ld_x, hidden, false},
                          {"y", y, bs_y, ld_y, hidden, true}};
  const int st = wn_check(fn, ts, 3, batch, t, hidden, SMT_BF16, true);
  if (st) return st < 0 ? 0 : st;
  SMT_CHECK_ARG(w_packed != nullptr, "%s: null pointer (w_packed)", fn);
  SMT_CHECK_ARG(((uintptr_t)w_packed & 15) == 0, "%s: w_packed must be 16-byte aligned", fn);
  SMT_CHECK_ARG(bias == nullptr || ((uintptr_t)bias & 3) == 0, "%s: bias must be 4-byte aligned", fn);
  hipStream_t stream = (hipStream_t)stream_;
  const int tiles_per_item = (t + WT_ROWS - 1) / WT_ROWS;
  const long long ntiles = (long long)tiles_per_item * batch;      // < 2^31 / 32 + batch
  WnTailArgs p{(const __bf16*)z, (const __bf16*)x, (const __bf16*)w_packed, bias, (__bf16*)y, bs_z, bs_x, bs_y,
               ld_z, ld_x, ld_y, lens, batch, t, tiles_per_item, (int)ntiles};
  // every workgroup stages W_g once: give it at least four tiles per wave where there are that many, at most 4 WGs per CU
  const int grid = (int)std::max<long long>(1, std::min<long long>((ntiles + 4 * WT_WAVES - 1) / (4 * WT_WAVES), 256 * 4));
  if (hidden == 64) wavenet_tail_kernel<64><<<grid, 64 * WT_WAVES, 0, stream>>>(p);
  else wavenet_tail_kernel<128><<<grid, 64 * WT_WAVES, 0, stream>>>(p);
  SMT_CHECK_LAUNCH(fn);
  return 0;
}
