// Channels-last 1-D convolution as an implicit GEMM on the gfx950 matrix cores.
//
// Replaces F.conv1d / F.conv_transpose1d under MaskedConv1d, MaskedConvTranspose1d, ResLayer and
// GatedHiFiBlock of the reference (models/vqvae/conv.py:5-18, resnet.py:16-36, 184-241) -- forward
// and data-gradient (the data-gradient of a convolution is a convolution with repacked weights).
//
//   y[b, t*os + oo, co] = epi( sum_j sum_ci pro(x)[b, t*stride + j*dil - pad, ci] * w[j][co][ci] )
//
// Activations are [B, T, C] with an explicit row pitch, so channel slices of a wider tensor are
// operands without copies.  One workgroup (4 waves, 2x2) computes BM output rows x BN output
// channels:  the haloed input tile is staged ONCE into LDS (the prologue -- row mask, ReLU,
// counter-based dropout -- is applied while staging, once per element, not once per tap) and every
// tap reads it at a row offset; weight chunks [BN x KC] stream through a double buffer.
//   bf16: v_mfma_f32_32x32x16_bf16, fp32 accumulate.   fp32: v_mfma_f32_32x32x2_f32 (exact fp32 fma
//   chains; the parity path).  Both read 16-byte fragments with ds_read_b128 from rows padded by
//   16 B (conflict-free, cdna guide G4).
// The accumulator tile goes back through LDS so that the epilogue (bias, activation gradient, row
// mask, residual) and the stores are fully coalesced 16-byte accesses.
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "smt_common.h"
#include "conv_common.h"

namespace smt {

template <typename T>
__device__ __forceinline__ void mma_step(const T* a, const T* b, f32x16& acc);
template <>
__device__ __forceinline__ void mma_step<__bf16>(const __bf16* a, const __bf16* b, f32x16& acc) {
  bf16x8 av = *reinterpret_cast<const bf16x8*>(a);
  bf16x8 bv = *reinterpret_cast<const bf16x8*>(b);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc, 0, 0, 0);
}
template <>
__device__ __forceinline__ void mma_step<float>(const float* a, const float* b, f32x16& acc) {
  f32x4 av = *reinterpret_cast<const f32x4*>(a);
  f32x4 bv = *reinterpret_cast<const f32x4*>(b);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc, 0, 0, 0);
}

// Waves are arranged 2 (rows) x WN (cols): NT = 256 threads -> WN = 2, NT = 512 -> WN = 4 (two waves per
// SIMD, so one wave's staging / address arithmetic hides under the other's MFMAs).
template <typename T, int BN, int NT>
__global__ __launch_bounds__(NT) void conv_gemm_kernel(ConvArgs p) {
  constexpr int EPV = Tr<T>::EPV, CCH = Tr<T>::CCH, KC = Tr<T>::KC, BM = Tr<T>::BM;
  constexpr int MW = BM / 64;           // 32-row tiles per wave (bf16: 2, fp32: 1)
  constexpr int WN = NT / 128;          // wave columns
  constexpr int NW = BN / (32 * WN);    // 32-col tiles per wave
  constexpr int PITCH_W = KC + EPV;
  constexpr int PITCH_C = BN + EPV;
  constexpr int WVEC = BN * KC / EPV;   // 16-byte vectors per weight chunk
  constexpr int WST = WVEC / NT;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int r = lane & 31, hh = lane >> 5;
  // XCD-aware mapping (cdna guide T1): workgroups b and b+8 share an XCD/L2, so give every XCD a
  // CONTIGUOUS run of row tiles -- neighbouring tiles share their halo rows and the weights in L2.
  const int ntiles = p.tiles_per_batch * p.B;
  const int per_xcd = (ntiles + 7) / 8;
  const int tile = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
  if (tile >= ntiles) return;
  if (p.dbg & 16) return;
  const int b = tile / p.tiles_per_batch;
  const int t0 = (tile % p.tiles_per_batch) * BM;
  const int n0 = blockIdx.y * BN;

  const int rows_in = (BM - 1) * p.stride + (p.taps - 1) * p.dil + 1;
  const int cch_max = min(p.Cin, CCH);
  const int pitch_a = cch_max + EPV;
  T* lds_a = reinterpret_cast<T*>(smem);
  const size_t a_bytes = align_up((size_t)max(rows_in * pitch_a, BM * PITCH_C) * sizeof(T), 16);
  T* lds_w = reinterpret_cast<T*>(smem + a_bytes);
  T* lds_c = lds_a;

  const T* xg = reinterpret_cast<const T*>(p.x) + (long long)b * p.x_bs;
  const T* wg = reinterpret_cast<const T*>(p.w);
  const int len_in = p.lens_in ? min(p.lens_in[b], p.Tin) : p.Tin;
  const int tin0 = t0 * p.stride - p.pad;

  f32x16 acc[MW][NW];
#pragma unroll
  for (int i = 0; i < MW; ++i)
#pragma unroll
    for (int n = 0; n < NW; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][n][e] = 0.f;

  // weight chunk staging: two register sets so that chunk s+2 is in flight while chunk s is consumed
  Vec<T, EPV> wst0[WST], wst1[WST];
  auto w_load = [&](Vec<T, EPV>* wst, int j, int ci0) {  // chunk rows co = n0.., cols ci = ci0..ci0+KC
#pragma unroll
    for (int s = 0; s < WST; ++s) {
      int f = tid + NT * s;
      int co = f / (KC / EPV), cv = f % (KC / EPV);
      int ci = ci0 + cv * EPV;
      Vec<T, EPV> v;
#pragma unroll
      for (int e = 0; e < EPV; ++e) v.v[e] = (T)0.f;
      if (n0 + co < p.Cout && ci < p.Cin && !(p.dbg & 2))
        v = *reinterpret_cast<const Vec<T, EPV>*>(wg + ((size_t)j * p.Cout + n0 + co) * p.Cin + ci);
      wst[s] = v;
    }
  };
  auto w_store = [&](const Vec<T, EPV>* wst, int buf) {
#pragma unroll
    for (int s = 0; s < WST; ++s) {
      int f = tid + NT * s;
      int co = f / (KC / EPV), cv = f % (KC / EPV);
      if (!(p.dbg & 128)) *reinterpret_cast<Vec<T, EPV>*>(lds_w + (size_t)buf * BN * PITCH_W + co * PITCH_W + cv * EPV) = wst[s];
    }
  };

  for (int cc = 0; cc < p.Cin; cc += CCH) {
    const int cch = min(CCH, p.Cin - cc);
    __syncthreads();  // previous chunk's readers are done with lds_a / lds_w
    // ---- stage the haloed input tile (this channel chunk), prologue applied once per element
    const int vpr = cch / EPV;
    const int vshift = 31 - __builtin_clz(vpr);   // vpr is a power of two (checked on the host)
    {
      // batches of UB independent 16-byte loads per thread, THEN the LDS stores: a load->store loop
      // would expose one full memory latency per vector
      constexpr int UB = 8;
      const int total = rows_in * vpr;
      for (int f0 = tid; f0 < total; f0 += NT * UB) {
        Vec<T, EPV> v[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
          const int f = f0 + NT * u;
          const int row = f >> vshift, cv = f & (vpr - 1);
          const int tin = tin0 + row;
#pragma unroll
          for (int e = 0; e < EPV; ++e) v[u].v[e] = (T)0.f;
          if (f < total && tin >= 0 && tin < len_in && !(p.dbg & 1))
            v[u] = *reinterpret_cast<const Vec<T, EPV>*>(xg + (long long)tin * p.ldx + cc + cv * EPV);
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
          const int f = f0 + NT * u;
          const int row = f >> vshift, cv = f & (vpr - 1);
          if (f < total && !(p.dbg & 64)) *reinterpret_cast<Vec<T, EPV>*>(lds_a + row * pitch_a + cv * EPV) = v[u];
        }
      }
    }
    // ---- K loop: taps x K-chunks.  LDS weight buffers alternate; global loads run two chunks ahead
    const int nkc = (cch + KC - 1) / KC;
    const int nsteps = p.taps * nkc;
    auto compute = [&](int s) {
      const int j = s / nkc, kc = s % nkc;
      const int kvalid = min(KC, cch - kc * KC);
      const T* abase = lds_a + (wm * (BM / 2) * p.stride + j * p.dil + r * p.stride) * pitch_a + kc * KC + hh * EPV;
      const T* bbase = lds_w + (size_t)(s & 1) * BN * PITCH_W + (wn * (BN / WN) + r) * PITCH_W + hh * EPV;
      const int a_step = 32 * p.stride * pitch_a;
      if (p.dbg & 4) return;
      if (kvalid == KC) {  // full chunk: constant trip count so the LDS reads are scheduled ahead of the MFMAs
#pragma unroll
        for (int kk = 0; kk < KC; kk += 2 * EPV) {
#pragma unroll
          for (int i = 0; i < MW; ++i)
#pragma unroll
            for (int n = 0; n < NW; ++n)
              mma_step<T>(abase + i * a_step + kk, bbase + n * 32 * PITCH_W + kk, acc[i][n]);
        }
      } else {
        for (int kk = 0; kk < kvalid; kk += 2 * EPV) {
#pragma unroll
          for (int i = 0; i < MW; ++i)
#pragma unroll
            for (int n = 0; n < NW; ++n)
              mma_step<T>(abase + i * a_step + kk, bbase + n * 32 * PITCH_W + kk, acc[i][n]);
        }
      }
    };
    w_load(wst0, 0, cc);
    if (nsteps > 1) w_load(wst1, 1 / nkc, cc + (1 % nkc) * KC);
    w_store(wst0, 0);
    __syncthreads();
    for (int s = 0; s < nsteps; s += 2) {
      // even step: chunk s is in LDS[0]; chunk s+1 sits in wst1; fetch chunk s+2 into wst0
      if (s + 2 < nsteps) w_load(wst0, (s + 2) / nkc, cc + ((s + 2) % nkc) * KC);
      compute(s);
      if (s + 1 < nsteps) w_store(wst1, 1);
      __syncthreads();
      if (s + 1 >= nsteps) break;
      // odd step: chunk s+1 is in LDS[1]; chunk s+2 sits in wst0; fetch chunk s+3 into wst1
      if (s + 3 < nsteps) w_load(wst1, (s + 3) / nkc, cc + ((s + 3) % nkc) * KC);
      compute(s + 1);
      if (s + 2 < nsteps) w_store(wst0, 0);
      __syncthreads();
    }
  }

  if (p.dbg & 32) return;
  // ---- accumulators -> LDS (element type T) -> coalesced epilogue
  float bvals[NW];
#pragma unroll
  for (int n = 0; n < NW; ++n) {
    const int col = n0 + wn * (BN / WN) + n * 32 + r;
    bvals[n] = (p.bias && col < p.Cout) ? p.bias[col] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < MW; ++i)
#pragma unroll
    for (int n = 0; n < NW; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = wm * (BM / 2) + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
        const int col = wn * (BN / WN) + n * 32 + r;
        // bias joins in fp32 before the (single, for residual-free layers) rounding to T
        lds_c[row * PITCH_C + col] = (T)(acc[i][n][e] + bvals[n]);
      }
  __syncthreads();
  T* yg = p.y ? reinterpret_cast<T*>(p.y) + (long long)b * p.y_bs : nullptr;
  const T* rg = p.res ? reinterpret_cast<const T*>(p.res) + (long long)b * p.res_bs : nullptr;
  const T* hg = p.epi_act ? reinterpret_cast<const T*>(p.gate_h) + (long long)b * p.gh_bs : nullptr;
  const int len_out = p.lens_out ? p.lens_out[b] : 0x7fffffff;
  constexpr int CV = BN / EPV;
  constexpr int NE = BM * CV / NT;    // vectors per thread
  // A full tile (the overwhelmingly common case) needs no per-vector bounds logic: every condition
  // below is then wave-uniform and the eight vectors of a thread are independent straight-line code.
  const bool full = (t0 + BM <= p.Tout) && (n0 + BN <= p.Cout) && ((t0 + BM - 1) * p.out_stride + p.out_offset < p.Ty);
  const int cv0 = tid % CV, row0 = tid / CV;      // this thread's column vector; rows row0 + it*(NT/CV)
  const int col = n0 + cv0 * EPV;
  Vec<T, EPV> rv[NE], uv[NE];
  bool okv[NE];
#pragma unroll
  for (int it = 0; it < NE; ++it) {
    const int t = t0 + row0 + it * (NT / CV);
    const int ty = t * p.out_stride + p.out_offset;
    okv[it] = full || ((t < p.Tout) && (col < p.Cout) && (ty < p.Ty));
#pragma unroll
    for (int e = 0; e < EPV; ++e) { rv[it].v[e] = (T)0.f; uv[it].v[e] = (T)0.f; }
    if (rg && okv[it]) rv[it] = *reinterpret_cast<const Vec<T, EPV>*>(rg + (long long)ty * p.ldr + col);
    if (p.epi_act && okv[it]) uv[it] = *reinterpret_cast<const Vec<T, EPV>*>(hg + (long long)ty * p.ldgh + col);
  }
  const int site = p.act_out ? col / p.site_width : 0;
  const unsigned key = site_key(p, site);
  const int cs = col - site * (p.act_out ? p.site_width : 0);
#pragma unroll
  for (int it = 0; it < NE; ++it) {
    const int row = row0 + it * (NT / CV);
    const int ty = (t0 + row) * p.out_stride + p.out_offset;
    Vec<T, EPV> c = *reinterpret_cast<const Vec<T, EPV>*>(lds_c + row * PITCH_C + cv0 * EPV);
    float o[EPV];
#pragma unroll
    for (int e = 0; e < EPV; ++e) o[e] = (float)c.v[e];
    if (p.epi_act) {  // d relu(dropout(h))/dh = scale * [u != 0] with u the stored activated tensor
#pragma unroll
      for (int e = 0; e < EPV; ++e) o[e] = ((float)uv[it].v[e] != 0.f) ? o[e] * p.drop_scale : 0.f;
    }
    const float keep_row = (ty >= len_out) ? 0.f : 1.f;
    if (rg) {
#pragma unroll
      for (int e = 0; e < EPV; ++e) o[e] = fmaf(o[e], keep_row, (float)rv[it].v[e]);
    } else {
#pragma unroll
      for (int e = 0; e < EPV; ++e) o[e] *= keep_row;
    }
    if (yg && okv[it] && !(p.dbg & 8)) {
      Vec<T, EPV> out;
#pragma unroll
      for (int e = 0; e < EPV; ++e) out.v[e] = (T)o[e];
      *reinterpret_cast<Vec<T, EPV>*>(yg + (long long)ty * p.ldy + col) = out;
    }
    if (p.act_out && okv[it]) {  // u = relu(dropout(y)), counter-based mask, applied in fp32 before rounding
      const unsigned long long base = ((unsigned long long)b * p.Ty + ty) * p.site_width + cs;
      Vec<T, EPV> ua;
#pragma unroll
      for (int e = 0; e < EPV; e += 2) {   // base is even: elements (e, e+1) share one hash
        const unsigned h = fmix32((unsigned)((base + e) >> 1) * 0x9E3779B1u + key);
        const bool k0 = (h & 0xFFFFu) >= p.drop_thresh16, k1 = (h >> 16) >= p.drop_thresh16;
        ua.v[e] = (T)((k0 && o[e] > 0.f) ? o[e] * p.drop_scale : 0.f);
        ua.v[e + 1] = (T)((k1 && o[e + 1] > 0.f) ? o[e + 1] * p.drop_scale : 0.f);
      }
      *reinterpret_cast<Vec<T, EPV>*>(reinterpret_cast<T*>(p.y_act) + (long long)b * p.ya_bs + (long long)ty * p.ldya + col) = ua;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// LDS-DMA variant (bf16, C_in % 128 == 0, C_out % 128 == 0, stride 1): both operands go HBM/L2 -> LDS
// with global_load_lds_dwordx4 (no VGPR round trip, no ds_write, no staging arithmetic in the loop).
// A DMA wave-instruction writes 64 x 16 B linearly, so rows cannot be padded; bank conflicts are
// avoided by an XOR swizzle of the 16-byte chunk index with the row index instead:
//   activations: applied on the per-lane SOURCE address while staging, undone by the fragment reads;
//   weights    : pre-swizzled in global memory by smt_pack_weight(swizzle = 1), copied linearly.
// Rows outside [0, len) are fetched from a zero page.
constexpr int DMA_BM = 128, DMA_BN = 128, DMA_KC = 128, DMA_NT = 512;

// MW = 32-row tiles per wave: BM = 64 * MW rows per workgroup.  MW = 4 (256 rows) halves the weight
// stream per output row -- the L2 -> LDS weight DMA (taps x 32 KiB per tile) is what bounds this kernel.
template <int MW>
__global__ __launch_bounds__(DMA_NT) void conv_gemm_dma_kernel(ConvArgs p, const __bf16* __restrict__ zero_page) {
  typedef __bf16 T;
  constexpr int EPV = 8, BM = 64 * MW, BN = DMA_BN, KC = DMA_KC, NT = DMA_NT;
  constexpr int WN = 4;                         // waves 2 (rows) x 4 (cols); wave tile (32 MW) x 32
  constexpr int ROWB = KC * 2;                  // 256 bytes per LDS row (128 channels)
  constexpr int PITCH_C = BN + EPV;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int r = lane & 31, hh = lane >> 5;

  const int ntiles = p.tiles_per_batch * p.B * p.rs;
  const int per_xcd = (ntiles + 7) / 8;
  const int tile = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
  if (tile >= ntiles) return;
  // Dilation classes: a conv with dilation d >= 8 is run as d independent DENSE convs over the row
  // classes t = cls (mod d) (rs = d, taps at distance 1 in the class domain), so the halo of a 128-row
  // tile is (taps - 1) rows instead of (taps - 1) * d.  Each class row is still a whole 256-byte
  // segment for the DMA.  rs == 1 is the plain case.
  const int rs = p.rs;
  const int bb = tile / p.tiles_per_batch;
  const int b = bb / rs, cls = bb - b * rs;
  const int t0 = (tile % p.tiles_per_batch) * BM;
  const int n0 = blockIdx.y * BN;
  const int Tc = (p.Tout - cls + rs - 1) / rs;          // rows of this class
  if (t0 >= Tc) return;

  const int rows_in = (BM - 1) + (p.taps - 1) * p.dil + 1;
  const int rows_pad = (rows_in + 3) & ~3;      // DMA granularity: 4 rows (1 KiB) per wave-instruction
  unsigned char* lds_a = smem;
  const size_t a_bytes = align_up((size_t)max(rows_pad * ROWB, BM * PITCH_C * 2), 1024);
  unsigned char* lds_w = smem + a_bytes;        // 2 x [BN rows][256 B]
  T* lds_c = reinterpret_cast<T*>(smem);

  const T* xg = reinterpret_cast<const T*>(p.x) + (long long)b * p.x_bs + (long long)cls * p.ldx;
  const long long ldx = (long long)p.ldx * rs;
  const unsigned char* wg = reinterpret_cast<const unsigned char*>(p.w);
  const int len_full = p.lens_in ? min(p.lens_in[b], p.Tin) : p.Tin;
  const int len_in = max(0, (len_full - cls + rs - 1) / rs);
  const int tin0 = t0 - p.pad;
  const int ncc = p.Cin / KC;

  f32x16 acc[MW];
#pragma unroll
  for (int i = 0; i < MW; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

  // epilogue operands (residual, activation source) are requested NOW so that they arrive under the GEMM
  constexpr int CV = BN / EPV, NE = BM * CV / NT;
  const int cv0 = tid % CV, row0 = tid / CV;
  const int col = n0 + cv0 * EPV;
  const T* rg = p.res ? reinterpret_cast<const T*>(p.res) + (long long)b * p.res_bs : nullptr;
  const T* hg = p.epi_act ? reinterpret_cast<const T*>(p.gate_h) + (long long)b * p.gh_bs : nullptr;
  Vec<T, EPV> rv[NE], uv[NE];
  bool okv[NE];
#pragma unroll
  for (int it = 0; it < NE; ++it) {
    const int tc = t0 + row0 + it * (NT / CV);
    okv[it] = (tc < Tc);
    const long long t = cls + (long long)rs * tc;          // actual row
#pragma unroll
    for (int e = 0; e < EPV; ++e) { rv[it].v[e] = (T)0.f; uv[it].v[e] = (T)0.f; }
    if (rg && okv[it]) rv[it] = *reinterpret_cast<const Vec<T, EPV>*>(rg + t * p.ldr + col);
    if (p.epi_act && okv[it]) uv[it] = *reinterpret_cast<const Vec<T, EPV>*>(hg + t * p.ldgh + col);
  }

  const int lrow = lane >> 4, lch = lane & 15;  // this lane's (row within the 4-row group, chunk) of a DMA instruction
  auto stage_w = [&](int j, int cc, int buf) {  // 32 KiB = 32 wave-instructions, 4 per wave
#pragma unroll
    for (int q = 0; q < (BN / 4) / (NT / 64); ++q) {
      const int g = wave + (NT / 64) * q;       // 4-row group index 0..31
      const int co = n0 + 4 * g + lrow;
      const unsigned char* src = wg + (((size_t)j * p.Cout + co) * ncc + cc) * ROWB + lch * 16;
      lds_dma16(src, lds_w + (size_t)buf * BN * ROWB + g * 1024);
    }
  };

  for (int cc = 0; cc < ncc; ++cc) {
    __syncthreads();  // previous chunk's readers are done with lds_a / lds_w
    for (int g = wave; g < rows_pad / 4; g += NT / 64) {
      const int row = 4 * g + lrow;
      const int tin = tin0 + row;
      const bool ok = (row < rows_in) && (tin >= 0) && (tin < len_in);
      const T* src = ok ? xg + (long long)tin * ldx + cc * KC + ((lch ^ (row & 15)) * EPV) : zero_page + lch * EPV;
      lds_dma16(src, lds_a + g * 1024);
    }
    stage_w(0, cc, 0);
    vm_wait<0>();
    __syncthreads();
    const int nsteps = p.taps;
    for (int s = 0; s < nsteps; ++s) {
      if (s + 1 < nsteps) stage_w(s + 1, cc, (s + 1) & 1);
      const unsigned char* wb = lds_w + (size_t)(s & 1) * BN * ROWB + (wn * 32 + r) * ROWB;
      const int bsw = (wn * 32 + r) & 15;
      const int arow0 = wm * (BM / 2) + s * p.dil + r;
#pragma unroll
      for (int kk = 0; kk < KC / 16; ++kk) {
        const int ch = 2 * kk + hh;
        const bf16x8 bv = *reinterpret_cast<const bf16x8*>(wb + ((ch ^ bsw) << 4));
#pragma unroll
        for (int i = 0; i < MW; ++i) {
          const int ar = arow0 + 32 * i;
          const bf16x8 av = *reinterpret_cast<const bf16x8*>(lds_a + ar * ROWB + ((ch ^ (ar & 15)) << 4));
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc[i], 0, 0, 0);
        }
      }
      vm_wait<0>();
      __syncthreads();
    }
  }

  // ---- epilogue: identical to conv_gemm_kernel<bf16, 128, 512>
  const float bval = (p.bias && n0 + wn * 32 + r < p.Cout) ? p.bias[n0 + wn * 32 + r] : 0.f;
#pragma unroll
  for (int i = 0; i < MW; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = wm * (BM / 2) + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
      lds_c[row * PITCH_C + wn * 32 + r] = (T)(acc[i][e] + bval);
    }
  __syncthreads();
  T* yg = p.y ? reinterpret_cast<T*>(p.y) + (long long)b * p.y_bs : nullptr;
  const int len_out = p.lens_out ? p.lens_out[b] : 0x7fffffff;
  const int site = p.act_out ? col / p.site_width : 0;
  const unsigned key = site_key(p, site);
  const int cs = col - site * (p.act_out ? p.site_width : 0);
#pragma unroll
  for (int it = 0; it < NE; ++it) {
    const int row = row0 + it * (NT / CV);
    const int ty = cls + rs * (t0 + row);                  // actual output row
    Vec<T, EPV> c = *reinterpret_cast<const Vec<T, EPV>*>(lds_c + row * PITCH_C + cv0 * EPV);
    float o[EPV];
#pragma unroll
    for (int e = 0; e < EPV; ++e) o[e] = (float)c.v[e];
    if (p.epi_act) {
#pragma unroll
      for (int e = 0; e < EPV; ++e) o[e] = ((float)uv[it].v[e] != 0.f) ? o[e] * p.drop_scale : 0.f;
    }
    const float keep_row = (ty >= len_out) ? 0.f : 1.f;
    if (rg) {
#pragma unroll
      for (int e = 0; e < EPV; ++e) o[e] = fmaf(o[e], keep_row, (float)rv[it].v[e]);
    } else {
#pragma unroll
      for (int e = 0; e < EPV; ++e) o[e] *= keep_row;
    }
    if (yg && okv[it]) {
      Vec<T, EPV> out;
#pragma unroll
      for (int e = 0; e < EPV; ++e) out.v[e] = (T)o[e];
      *reinterpret_cast<Vec<T, EPV>*>(yg + (long long)ty * p.ldy + col) = out;
    }
    if (p.act_out && okv[it]) {
      const unsigned long long base = ((unsigned long long)b * p.Ty + ty) * p.site_width + cs;
      Vec<T, EPV> ua;
#pragma unroll
      for (int e = 0; e < EPV; e += 2) {
        const unsigned h = fmix32((unsigned)((base + e) >> 1) * 0x9E3779B1u + key);
        const bool k0 = (h & 0xFFFFu) >= p.drop_thresh16, k1 = (h >> 16) >= p.drop_thresh16;
        ua.v[e] = (T)((k0 && o[e] > 0.f) ? o[e] * p.drop_scale : 0.f);
        ua.v[e + 1] = (T)((k1 && o[e + 1] > 0.f) ? o[e + 1] * p.drop_scale : 0.f);
      }
      *reinterpret_cast<Vec<T, EPV>*>(reinterpret_cast<T*>(p.y_act) + (long long)b * p.ya_bs + (long long)ty * p.ldya + col) = ua;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Persistent 1x1 variant (bf16, C_in == 128, C_out % 128 == 0): an HBM-bound layer.  Each workgroup keeps
// its 128 x 128 weight block in REGISTERS (32 VGPRs per lane) for its whole run of row tiles, streams the
// activation tiles through an LDS double buffer by LDS-DMA (tile i+1 is in flight while tile i is
// multiplied, staged and stored) and requests the epilogue operands of a tile before its MFMAs.
constexpr int P1_BUF = 35 * 1024;   // 128 rows x 256 B operand tile, reused as the 128 x 272 B output staging tile

__global__ __launch_bounds__(DMA_NT) void conv1x1_dma_kernel(ConvArgs p, const __bf16* __restrict__ zero_page,
                                                             int tiles_per_wg) {
  typedef __bf16 T;
  constexpr int EPV = 8, BM = DMA_BM, BN = DMA_BN, KC = DMA_KC, NT = DMA_NT;
  constexpr int WN = 4, MW = 2, ROWB = KC * 2, PITCH_C = BN + EPV;
  constexpr int CV = BN / EPV, NE = BM * CV / NT;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int r = lane & 31, hh = lane >> 5;
  const int lrow = lane >> 4, lch = lane & 15;
  const int n0 = blockIdx.y * BN;

  int wg, tile_begin, tile_end;
  if (!wg_tile_run(p.tiles_per_batch * p.B, tiles_per_wg, wg, tile_begin, tile_end)) return;

  // weight fragments -> registers (weights are packed swizzled: chunk c of row co sits at c ^ (co & 15))
  bf16x8 wfrag[KC / 16];
  {
    const int co = n0 + wn * 32 + r;
    load_wfrags(wfrag, reinterpret_cast<const unsigned char*>(p.w) + (size_t)co * ROWB, hh, co & 15);
  }
  const float bval = p.bias ? p.bias[n0 + wn * 32 + r] : 0.f;
  const int cv0 = tid % CV, row0 = tid / CV;
  const int col = n0 + cv0 * EPV;
  const int site = p.act_out ? col / p.site_width : 0;
  const unsigned key = site_key(p, site);
  const int cs = col - site * (p.act_out ? p.site_width : 0);

  auto stage_a = [&](int tile, int buf) {
    const int b = tile / p.tiles_per_batch;
    const int t0 = (tile % p.tiles_per_batch) * BM;
    const T* xg = reinterpret_cast<const T*>(p.x) + (long long)b * p.x_bs;
    const int len_in = p.lens_in ? min(p.lens_in[b], p.Tin) : p.Tin;
#pragma unroll
    for (int q = 0; q < (BM / 4) / (NT / 64); ++q) {
      const int g = wave + (NT / 64) * q;
      const int row = 4 * g + lrow;
      const int tin = t0 + row;
      const T* src = (tin < len_in) ? xg + (long long)tin * p.ldx + ((lch ^ (row & 15)) * EPV) : zero_page + lch * EPV;
      lds_dma16(src, smem + (size_t)buf * P1_BUF + g * 1024);
    }
  };

  stage_a(tile_begin, 0);
  for (int tile = tile_begin; tile < tile_end; ++tile) {
    const int buf = (tile - tile_begin) & 1;
    const int b = tile / p.tiles_per_batch;
    const int t0 = (tile % p.tiles_per_batch) * BM;
    vm_wait<0>();                                       // this tile's operand has landed (and older stores retired)
    __syncthreads();                                    // ... for every wave; the other buffer is free again
    if (tile + 1 < tile_end) stage_a(tile + 1, buf ^ 1);
    // epilogue operands of THIS tile: requested before the MFMAs
    const T* rg = p.res ? reinterpret_cast<const T*>(p.res) + (long long)b * p.res_bs : nullptr;
    const T* hg = p.epi_act ? reinterpret_cast<const T*>(p.gate_h) + (long long)b * p.gh_bs : nullptr;
    Vec<T, EPV> rv[NE], uv[NE];
    bool okv[NE];
#pragma unroll
    for (int it = 0; it < NE; ++it) {
      const int t = t0 + row0 + it * (NT / CV);
      okv[it] = (t < p.Tout);
#pragma unroll
      for (int e = 0; e < EPV; ++e) { rv[it].v[e] = (T)0.f; uv[it].v[e] = (T)0.f; }
      if (rg && okv[it]) rv[it] = *reinterpret_cast<const Vec<T, EPV>*>(rg + (long long)t * p.ldr + col);
      if (p.epi_act && okv[it]) uv[it] = *reinterpret_cast<const Vec<T, EPV>*>(hg + (long long)t * p.ldgh + col);
    }
    const unsigned char* lds_a = smem + (size_t)buf * P1_BUF;
    f32x16 acc[MW];
#pragma unroll
    for (int i = 0; i < MW; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
#pragma unroll
    for (int kk = 0; kk < KC / 16; ++kk) {
      const int ch = 2 * kk + hh;
#pragma unroll
      for (int i = 0; i < MW; ++i) {
        const int ar = wm * 64 + 32 * i + r;
        bf16x8 av = *reinterpret_cast<const bf16x8*>(lds_a + ar * ROWB + ((ch ^ (ar & 15)) << 4));
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, wfrag[kk], acc[i], 0, 0, 0);
      }
    }
    __syncthreads();   // every wave is done reading the operand tile: reuse it as the output staging tile
    T* lds_c = reinterpret_cast<T*>(smem + (size_t)buf * P1_BUF);
#pragma unroll
    for (int i = 0; i < MW; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
        lds_c[row * PITCH_C + wn * 32 + r] = (T)(acc[i][e] + bval);
      }
    __syncthreads();
    T* yg = p.y ? reinterpret_cast<T*>(p.y) + (long long)b * p.y_bs : nullptr;
    const int len_out = p.lens_out ? p.lens_out[b] : 0x7fffffff;
#pragma unroll
    for (int it = 0; it < NE; ++it) {
      const int row = row0 + it * (NT / CV);
      const int ty = t0 + row;
      Vec<T, EPV> c = *reinterpret_cast<const Vec<T, EPV>*>(lds_c + row * PITCH_C + cv0 * EPV);
      float o[EPV];
#pragma unroll
      for (int e = 0; e < EPV; ++e) o[e] = (float)c.v[e];
      if (p.epi_act) {
#pragma unroll
        for (int e = 0; e < EPV; ++e) o[e] = ((float)uv[it].v[e] != 0.f) ? o[e] * p.drop_scale : 0.f;
      }
      const float keep_row = (ty >= len_out) ? 0.f : 1.f;
      if (rg) {
#pragma unroll
        for (int e = 0; e < EPV; ++e) o[e] = fmaf(o[e], keep_row, (float)rv[it].v[e]);
      } else {
#pragma unroll
        for (int e = 0; e < EPV; ++e) o[e] *= keep_row;
      }
      if (yg && okv[it]) {
        Vec<T, EPV> out;
#pragma unroll
        for (int e = 0; e < EPV; ++e) out.v[e] = (T)o[e];
        *reinterpret_cast<Vec<T, EPV>*>(yg + (long long)ty * p.ldy + col) = out;
      }
      if (p.act_out && okv[it]) {
        const unsigned long long base = ((unsigned long long)b * p.Ty + ty) * p.site_width + cs;
        Vec<T, EPV> ua;
#pragma unroll
        for (int e = 0; e < EPV; e += 2) {
          const unsigned h = fmix32((unsigned)((base + e) >> 1) * 0x9E3779B1u + key);
          const bool k0 = (h & 0xFFFFu) >= p.drop_thresh16, k1 = (h >> 16) >= p.drop_thresh16;
          ua.v[e] = (T)((k0 && o[e] > 0.f) ? o[e] * p.drop_scale : 0.f);
          ua.v[e + 1] = (T)((k1 && o[e + 1] > 0.f) ? o[e + 1] * p.drop_scale : 0.f);
        }
        *reinterpret_cast<Vec<T, EPV>*>(reinterpret_cast<T*>(p.y_act) + (long long)b * p.ya_bs + (long long)ty * p.ldya + col) = ua;
      }
    }
    // the next iteration's top barrier orders these LDS reads before the buffer is overwritten by a DMA
  }
}
// ------------------------------------------------------------------------------------------------
// 1x1 conv with a folded second 1x1 term (bf16, C_in == 128, C_in2 == 64):
//   y = W u + b  +  W2 x2 + b2
// K3 of GatedHiFiBlock adds the branch input h1 = K1(x) + b1 (resnet.py:226).  K1 is linear, so the residual is
// recomputed here from the 64-channel block input instead of being written by K1 and read back as a 128-channel
// tensor: per row 384 B in / 256 B out instead of 512 B in / 256 B out here and 256 B less written by K1.
// Same structure as conv1x1_bwd_kernel: persistent workgroups, both operand tiles through an LDS-DMA double
// buffer, transposed MFMA tiles (A = weights in registers, B = rows) stored straight from registers.
constexpr int FO_ROWS = 128, FO_NT = 512, FO_U = FO_ROWS * 256, FO_X = FO_ROWS * 128, FO_STAGE = FO_U + FO_X;

__global__ __launch_bounds__(FO_NT) void conv1x1_fold_kernel(ConvArgs p, const __bf16* __restrict__ zero_page,
                                                              int tiles_per_wg) {
  typedef __bf16 T;
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];   // 2 x [u tile 32 KiB | x2 tile 16 KiB]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;          // rows 64 wm.., output channels n0 + 32 wn..
  const int r = lane & 31, hh = lane >> 5;
  const int n0 = blockIdx.y * 128;

  int wg, tile_begin, tile_end;
  if (!wg_tile_run(p.tiles_per_batch * p.B, tiles_per_wg, wg, tile_begin, tile_end)) return;

  bf16x8 wfrag[8], w2frag[4];
  {
    const int co = n0 + wn * 32 + r;
    load_wfrags(wfrag, reinterpret_cast<const unsigned char*>(p.w) + (size_t)co * 256, hh, co & 15);
    load_wfrags(w2frag, reinterpret_cast<const unsigned char*>(p.w2) + (size_t)co * 128, hh);
  }
  // accumulator element 4g + k of a lane = output channel col0 + 8g + k
  const int col0 = n0 + wn * 32 + 4 * hh;
  float bval[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int c = col0 + 8 * (e >> 2) + (e & 3);
    bval[e] = (p.bias ? p.bias[c] : 0.f) + (p.bias2 ? p.bias2[c] : 0.f);
  }

  auto stage = [&](int tile, int buf) {
    const int b = tile / p.tiles_per_batch;
    const int t0 = (tile - b * p.tiles_per_batch) * FO_ROWS;
    const T* ug = reinterpret_cast<const T*>(p.x) + (long long)b * p.x_bs;
    const T* xg = reinterpret_cast<const T*>(p.x2) + (long long)b * p.x2_bs;
    const int len_in = p.lens_in ? min(p.lens_in[b], p.Tin) : p.Tin;
    const int len_in2 = p.lens_in2 ? min(p.lens_in2[b], p.Tin) : p.Tin;
    unsigned char* base = smem + (size_t)buf * FO_STAGE;
#pragma unroll
    for (int q = 0; q < (FO_ROWS / 4) / (FO_NT / 64); ++q) {     // u: 4 rows x 16 chunks per instruction
      const int g = wave + (FO_NT / 64) * q;
      const int row = 4 * g + (lane >> 4), pos = lane & 15;
      const int t = t0 + row;
      lds_dma16(t < len_in ? ug + (long long)t * p.ldx + ((pos ^ swz256_row(row)) * 8) : zero_page + pos * 8, base + g * 1024);
    }
#pragma unroll
    for (int q = 0; q < (FO_ROWS / 8) / (FO_NT / 64); ++q) {     // x2: 8 rows x 8 chunks per instruction
      const int g = wave + (FO_NT / 64) * q;
      const int row = 8 * g + (lane >> 3), pos = lane & 7;
      const int t = t0 + row;
      lds_dma16(t < len_in2 ? xg + (long long)t * p.ldx2 + ((pos ^ swz128_row(row)) * 8) : zero_page + pos * 8,
                base + FO_U + g * 1024);
    }
  };

  stage(tile_begin, 0);
  for (int tile = tile_begin; tile < tile_end; ++tile) {
    const int buf = (tile - tile_begin) & 1;
    const int b = tile / p.tiles_per_batch;
    const int t0 = (tile - b * p.tiles_per_batch) * FO_ROWS;
    vm_wait<0>();                                       // this tile has landed
    __syncthreads();                                    // ... for every wave; the other buffer is free again
    if (tile + 1 < tile_end) stage(tile + 1, buf ^ 1);
    const unsigned char* ut = smem + (size_t)buf * FO_STAGE;
    const unsigned char* xt = ut + FO_U;

    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = wm * 64 + 32 * i + r;
        bf16x8 bv = lds_row_frag(ut, row, 256, kk, hh, swz256_row(row));
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wfrag[kk], bv, acc[i], 0, 0, 0);
      }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = wm * 64 + 32 * i + r;
        bf16x8 bv = lds_row_frag(xt, row, 128, kk, hh, swz128_row(row));
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2frag[kk], bv, acc[i], 0, 0, 0);
      }

    T* yg = reinterpret_cast<T*>(p.y) + (long long)b * p.y_bs;
    const int len_out = p.lens_out ? p.lens_out[b] : 0x7fffffff;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int t = t0 + wm * 64 + 32 * i + r;
      const float keep_row = (t >= len_out) ? 0.f : 1.f;
      unsigned yp[8];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = (acc[i][4 * g + k] + bval[4 * g + k]) * keep_row;
        yp[2 * g] = pack_bf16x2(o[0], o[1]);
        yp[2 * g + 1] = pack_bf16x2(o[2], o[3]);
      }
      pair_up8(yp);
      if (t < p.Tout) {
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        T* dst = yg + (long long)t * p.ldy + n0 + wn * 32 + 8 * hh;
        *reinterpret_cast<u32x4*>(dst) = u32x4{yp[0], yp[1], yp[2], yp[3]};
        *reinterpret_cast<u32x4*>(dst + 16) = u32x4{yp[4], yp[5], yp[6], yp[7]};
      }
    }
  }
}

static int launch_conv1x1_fold(ConvArgs p, const void* zero_page, hipStream_t stream) {
  p.tiles_per_batch = (p.Tout + FO_ROWS - 1) / FO_ROWS;
  const StreamGrid sg = plan_stream((long long)p.tiles_per_batch * p.B, 256, 2);     // one workgroup per CU (96 KiB of LDS)
  dim3 grid((unsigned)sg.nwg, (unsigned)(p.Cout / 128));
  (void)hipFuncSetAttribute((const void*)conv1x1_fold_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  conv1x1_fold_kernel<<<grid, FO_NT, 2 * FO_STAGE, stream>>>(p, (const __bf16*)zero_page, sg.tiles_per_wg);
  SMT_CHECK_LAUNCH("conv1x1_fold");
  return 0;
}

// ------------------------------------------------------------------------------------------------
// K1 of GatedHiFiBlock for all branches at once when only the ACTIVATED output is wanted (bf16, C_in = 64,
// C_out = 512, y == NULL):  u = relu(dropout(W x + b)) -- 128 B in, 1 KiB out per row, an HBM-write-bound
// layer.  Persistent workgroups; the 512 x 64 weight block lives in registers (wave w owns output channels
// 64 w .. 64 w + 63); x tiles come through an LDS-DMA double buffer; transposed MFMA tiles, dropout hash and
// ReLU on the accumulators, v_permlane32_swap pairing, 16-byte stores straight from registers.
constexpr int K1_ROWS = 128, K1_NT = 512, K1_X = K1_ROWS * 128, K1_COUT = 512;
constexpr int K1_STORES = (K1_ROWS / 32) * 2 * 2;      // stores per wave and tile: row groups x 2 channel tiles x 2

__global__ __launch_bounds__(K1_NT) void conv_k1act_kernel(ConvArgs p, const __bf16* __restrict__ zero_page,
                                                           int tiles_per_wg) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];   // 2 x [128 rows][128 B]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;

  int wg, tile_begin, tile_end;
  if (!wg_tile_run(p.tiles_per_batch * p.B, tiles_per_wg, wg, tile_begin, tile_end)) return;

  bf16x8 wfrag[2][4];
  float bval[2][16];
  unsigned keys[2];
  int cs[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int co = wave * 64 + 32 * c + r;
    const unsigned char* wrow = reinterpret_cast<const unsigned char*>(p.w) + (size_t)co * 128;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) wfrag[c][kk] = *reinterpret_cast<const bf16x8*>(wrow + ((2 * kk + hh) << 4));
    // accumulator element 4g + k of a lane = output channel col0 + 8g + k
    const int col0 = wave * 64 + 32 * c + 4 * hh;
#pragma unroll
    for (int e = 0; e < 16; ++e) bval[c][e] = p.bias ? p.bias[col0 + 8 * (e >> 2) + (e & 3)] : 0.f;
    const int site = col0 / p.site_width;            // a 32-channel tile never straddles a site (site_width % 32 == 0)
    keys[c] = site_key(p, site);
    cs[c] = col0 - site * p.site_width;
  }

  // the tile loop of conv_stream.h; the counted wait is vmcnt(16 stores): the 128 KiB a workgroup writes per tile drain
  // under the next tile instead of in front of it
  auto decode = [&](int tile, int& b, int& t0) { tile_decode<K1_ROWS>(tile, p.tiles_per_batch, b, t0); };
  const unsigned pitch_x = (unsigned)p.ldx * 2u, pitch_u = (unsigned)p.ldya * 2u;
  const int xrow = 8 * wave + (lane >> 3);                        // group wave + 8 q: rows 8 wave + .. + 64 q, swizzle independent of q
  const unsigned xoff0 = (unsigned)xrow * pitch_x + (unsigned)(((lane & 7) ^ swz128_row(xrow)) << 4);
  auto stage = [&](int tile, int buf) {
    int b, t0;
    decode(tile, b, t0);
    const int len_in = p.lens_in ? min(scalar_load_i32(p.lens_in + b), p.Tin) : p.Tin;
    const UntrackedRsrc rx = untracked_rsrc(p.x, (long long)b * p.x_bs * 2, (unsigned)len_in * pitch_x);
    unsigned vo = xoff0 + (unsigned)t0 * pitch_x;
#pragma unroll
    for (int q = 0; q < (K1_ROWS / 8) / (K1_NT / 64); ++q) {     // 8 rows x 8 chunks per instruction; rows >= len_in read as zero
      untracked_dma16(rx, vo, smem + (size_t)buf * K1_X + (wave + (K1_NT / 64) * q) * 1024);
      vo += 64u * pitch_x;
    }
  };

  stage(tile_begin, 0);
  // the first tile, weights and biases (pinned, so that the compiler does not re-wait for them in the loop); later tiles:
  // counted wait at the END
  vm_wait<0>(wfrag, bval);
  for (int tile = tile_begin; tile < tile_end; ++tile) {
    const int buf = (tile - tile_begin) & 1;
    int b, t0;
    decode(tile, b, t0);
    lgkm_wait<0>();
    __builtin_amdgcn_s_barrier();                       // every wave's part of this tile landed; the other buffer is free again
    if (tile + 1 < tile_end) stage(tile + 1, buf ^ 1);
    const unsigned char* xt = smem + (size_t)buf * K1_X;
    const __amdgpu_buffer_rsrc_t ru = ws_rsrc(p.y_act, (long long)b * p.ya_bs * 2, (unsigned)p.Tout * pitch_u);
    const int len_out = p.lens_out ? scalar_load_i32(p.lens_out + b) : 0x7fffffff;
#pragma unroll 1
    for (int i = 0; i < K1_ROWS / 32; ++i) {
      const int row = 32 * i + r;
      f32x16 acc[2];
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[c][e] = 0.f;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        bf16x8 bv = lds_row_frag(xt, row, 128, kk, hh, swz128_row(row));
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wfrag[c][kk], bv, acc[c], 0, 0, 0);
      }
      const int t = t0 + row;
      const float srow = (t >= len_out) ? 0.f : p.drop_scale;       // row mask folded into the dropout scale
      const unsigned thr_m1 = (unsigned)(p.drop_thresh16 - 1) * 0x10001u;
      // dropout hash input of element pair (g, k): ((rowbase + cs + 8 g + k) >> 1) * C + key.  rowbase, cs, 8 g and k are
      // all even (site_width % 32 == 0), so the shift distributes and the product is linear mod 2^32: ONE quarter-rate
      // multiply per (row, column block) instead of eight, the rest are adds of compile-time multiples of C
      const unsigned rowhalf = (unsigned)((((unsigned long long)b * p.Ty + t) * p.site_width) >> 1);
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        unsigned up[8];
        const unsigned hbase = (rowhalf + (unsigned)(cs[c] >> 1)) * 0x9E3779B1u + keys[c];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            // h = bf16(acc + bias), two elements per conversion; u = relu(dropout(h)): scale, round, then ReLU and the keep
            // mask on the packed pair (same arithmetic, element by element, as the generic epilogue)
            const unsigned hp = pack_bf16x2(acc[c][4 * g + 2 * j] + bval[c][4 * g + 2 * j], acc[c][4 * g + 2 * j + 1] + bval[c][4 * g + 2 * j + 1]);
            unsigned w = pk_relu_bf16(pack_bf16x2(__builtin_bit_cast(float, hp << 16) * srow, __builtin_bit_cast(float, hp & 0xffff0000u) * srow));
            if (p.drop_thresh16) w &= pk_keep_mask(fmix32(hbase + (unsigned)(4 * g + j) * 0x9E3779B1u), thr_m1);
            up[2 * g + j] = w;
          }
        pair_up8(up);
        {                                               // rows >= Tout: out of range, dropped -- but ISSUED
          const unsigned vo = (unsigned)t * pitch_u + (unsigned)(wave * 64 + 32 * c + 8 * hh) * 2u;
          store_paired(up, ru, vo);
        }
      }
    }
    // the next tile's DMA is older than this tile's stores
    step_end_wait<K1_STORES>();
  }
}

static bool conv_k1act_eligible(const smt_conv_desc* d) {
  return d->dtype == SMT_BF16 && d->taps == 1 && d->c_in == 64 && d->c_out == K1_COUT && d->stride == 1 &&
         d->out_stride == 1 && d->out_offset == 0 && d->t_y == d->t_out && d->t_in == d->t_out && !d->y && d->act_out &&
         d->y_act && !d->res && !d->act_grad && !d->x2 && d->zero_page && !d->w_swizzled && d->site_width % 32 == 0;
}

static int launch_conv_k1act(ConvArgs p, const void* zero_page, hipStream_t stream) {
  p.tiles_per_batch = (p.Tout + K1_ROWS - 1) / K1_ROWS;
  const StreamGrid sg = plan_stream((long long)p.tiles_per_batch * p.B, 512, 2);     // two workgroups per CU (32 KiB of LDS each)
  conv_k1act_kernel<<<sg.nwg, K1_NT, 2 * K1_X, stream>>>(p, (const __bf16*)zero_page, sg.tiles_per_wg);
  SMT_CHECK_LAUNCH("conv_k1act");
  return 0;
}

// ------------------------------------------------------------------------------------------------
// The gate conv of GatedHiFiBlock, forward (reference models/vqvae/resnet.py:238-241): out = W g + b + x, a 64 -> 64 1 x 1
// conv with the block input as residual -- 128 B + 128 B in, 128 B out per row.  It ran on the generic register-staged
// kernel (1.07 ms/step over the 14 blocks; now 0.8 ms = 4.7 TB/s at the top level).  Same machine as conv_k1act: persistent
// workgroups (four waves, 64-row tiles, up to four per CU), the 64 x 64 weight block in registers (wave w: output channels
// 32 (w & 1).., rows 32 (w >> 1)..),
// g and x tiles through an untracked LDS-DMA double buffer, transposed MFMA tile, the generic epilogue's arithmetic element
// by element -- out = bf16(bf16(acc + b) * keep_row + x) -- v_permlane32_swap pairing, 16-byte stores through a V#, one
// counted wait per tile.
constexpr int C64_ROWS = 64, C64_NT = 256, C64_TILE = C64_ROWS * 128;   // four waves: 32 output channels x 32 rows each
constexpr int C64_STORES = 2;                                              // stores per wave and tile

__global__ __launch_bounds__(C64_NT) void conv1x1_c64_kernel(ConvArgs p, int tiles_per_wg) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];   // 2 x [g tile | x tile], 64 rows x 128 B each
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int ct = wave & 1, rg = wave >> 1;

  int wg, tile_begin, tile_end;
  if (!wg_tile_run(p.tiles_per_batch * p.B, tiles_per_wg, wg, tile_begin, tile_end)) return;

  bf16x8 wfrag[4];
  float bval[16];
  {
    const int co = 32 * ct + r;
    load_wfrags(wfrag, reinterpret_cast<const unsigned char*>(p.w) + (size_t)co * 128, hh);
    // accumulator element 4g + k of a lane = output channel 32 ct + 4 hh + 8g + k
#pragma unroll
    for (int e = 0; e < 16; ++e) bval[e] = p.bias ? p.bias[32 * ct + 4 * hh + 8 * (e >> 2) + (e & 3)] : 0.f;
  }

  auto decode = [&](int tile, int& b, int& t0) { tile_decode<C64_ROWS>(tile, p.tiles_per_batch, b, t0); };
  const unsigned pitch_x = (unsigned)p.ldx * 2u, pitch_r = (unsigned)p.ldr * 2u, pitch_y = (unsigned)p.ldy * 2u;
  const int srow = 8 * wave + (lane >> 3);                         // group wave + 8 q: rows 8 wave + .. + 64 q
  const unsigned schunk = (unsigned)(((lane & 7) ^ swz128_row(srow)) << 4);
  auto stage = [&](int tile, int buf) {
    int b, t0;
    decode(tile, b, t0);
    const int len_in = p.lens_in ? min(scalar_load_i32(p.lens_in + b), p.Tin) : p.Tin;
    const UntrackedRsrc rx = untracked_rsrc(p.x, (long long)b * p.x_bs * 2, (unsigned)len_in * pitch_x);
    const UntrackedRsrc rr = untracked_rsrc(p.res, (long long)b * p.res_bs * 2, (unsigned)p.Tout * pitch_r);
    unsigned char* base = smem + (size_t)buf * 2 * C64_TILE + wave * 1024;
#pragma unroll
    for (int q = 0; q < (C64_ROWS / 8) / (C64_NT / 64); ++q) {     // 8 rows x 8 chunks per instruction
      untracked_dma16(rx, (unsigned)(t0 + srow + 8 * (C64_NT / 64) * q) * pitch_x + schunk, base + q * (C64_NT / 64) * 1024);
      untracked_dma16(rr, (unsigned)(t0 + srow + 8 * (C64_NT / 64) * q) * pitch_r + schunk, base + C64_TILE + q * (C64_NT / 64) * 1024);
    }
  };

  stage(tile_begin, 0);
  vm_wait<0>(wfrag, bval);                              // the first tile, weights and biases; later tiles: counted wait at the END
  for (int tile = tile_begin; tile < tile_end; ++tile) {
    const int buf = (tile - tile_begin) & 1;
    int b, t0;
    decode(tile, b, t0);
    lgkm_wait<0>();
    __builtin_amdgcn_s_barrier();                       // every wave's part of this tile landed; the other buffer is free again
    if (tile + 1 < tile_end) stage(tile + 1, buf ^ 1);
    const unsigned char* gt = smem + (size_t)buf * 2 * C64_TILE;
    const unsigned char* xt = gt + C64_TILE;
    const __amdgpu_buffer_rsrc_t ry = ws_rsrc(p.y, (long long)b * p.y_bs * 2, (unsigned)p.Tout * pitch_y);
    const int len_out = p.lens_out ? scalar_load_i32(p.lens_out + b) : 0x7fffffff;
    const int row = 32 * rg + r;
    const int swz = swz128_row(row);
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const bf16x8 bv = lds_row_frag(gt, row, 128, kk, hh, swz);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wfrag[kk], bv, acc, 0, 0, 0);
    }
    const int t = t0 + row;
    const float keep_row = (t >= len_out) ? 0.f : 1.f;
    unsigned yp[8];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      // residual channels 32 ct + 8 g + 4 hh + 0..3 of this row: half of the 16-byte chunk 4 ct + g
      const uint2 rv = *reinterpret_cast<const uint2*>(xt + row * 128 + (((4 * ct + g) ^ swz) << 4) + 8 * hh);
      const unsigned h01 = pack_bf16x2(acc[4 * g] + bval[4 * g], acc[4 * g + 1] + bval[4 * g + 1]);
      const unsigned h23 = pack_bf16x2(acc[4 * g + 2] + bval[4 * g + 2], acc[4 * g + 3] + bval[4 * g + 3]);
      yp[2 * g] = pack_bf16x2(fmaf(__builtin_bit_cast(float, h01 << 16), keep_row, __builtin_bit_cast(float, rv.x << 16)),
                              fmaf(__builtin_bit_cast(float, h01 & 0xffff0000u), keep_row, __builtin_bit_cast(float, rv.x & 0xffff0000u)));
      yp[2 * g + 1] = pack_bf16x2(fmaf(__builtin_bit_cast(float, h23 << 16), keep_row, __builtin_bit_cast(float, rv.y << 16)),
                                  fmaf(__builtin_bit_cast(float, h23 & 0xffff0000u), keep_row, __builtin_bit_cast(float, rv.y & 0xffff0000u)));
    }
    // lane pairing (written out: as a call to pair_up8 this kernel compiles to a different instruction order)
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        auto sw = __builtin_amdgcn_permlane32_swap(yp[4 * h2 + d], yp[4 * h2 + 2 + d], false, false);
        yp[4 * h2 + d] = sw[0]; yp[4 * h2 + 2 + d] = sw[1];
      }
    store_paired(yp, ry, (unsigned)t * pitch_y + (unsigned)(32 * ct + 8 * hh) * 2u);   // rows >= Tout: dropped -- but ISSUED
    step_end_wait<C64_STORES>();                        // the next tile's DMA is older than this tile's stores
  }
}

static bool conv1x1_c64_eligible(const smt_conv_desc* d) {
  static const bool off = getenv("SMT_NO_C64") != nullptr;
  return !off && d->dtype == SMT_BF16 && d->taps == 1 && d->c_in == 64 && d->c_out == 64 && d->stride == 1 && d->out_stride == 1 &&
         d->out_offset == 0 && d->t_y == d->t_out && d->t_in == d->t_out && d->y && d->res && !d->act_out && !d->act_grad &&
         !d->x2 && !d->w_swizzled && d->zero_page && d->ld_x % 8 == 0 && d->ld_res % 8 == 0 && d->ld_y % 8 == 0;
}

static int launch_conv1x1_c64(ConvArgs p, hipStream_t stream) {
  p.tiles_per_batch = (p.Tout + C64_ROWS - 1) / C64_ROWS;
  const StreamGrid sg = plan_stream((long long)p.tiles_per_batch * p.B, 1024, 2);    // four workgroups per CU (32 KiB of LDS, four waves each)
  (void)hipFuncSetAttribute((const void*)conv1x1_c64_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * C64_TILE);
  conv1x1_c64_kernel<<<sg.nwg, C64_NT, 4 * C64_TILE, stream>>>(p, sg.tiles_per_wg);
  SMT_CHECK_LAUNCH("conv1x1_c64");
  return 0;
}

static int launch_conv1x1_dma(ConvArgs p, const void* zero_page, hipStream_t stream) {
  p.tiles_per_batch = (p.Tout + DMA_BM - 1) / DMA_BM;
  // two workgroups per CU (70 KB of LDS each); at least 2 tiles per workgroup so that the pipeline pays
  const StreamGrid sg = plan_stream((long long)p.tiles_per_batch * p.B, 512, 2);
  dim3 grid((unsigned)sg.nwg, (unsigned)(p.Cout / DMA_BN));
  const size_t lds = 2 * P1_BUF;
  (void)hipFuncSetAttribute((const void*)conv1x1_dma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  conv1x1_dma_kernel<<<grid, DMA_NT, lds, stream>>>(p, (const __bf16*)zero_page, sg.tiles_per_wg);
  SMT_CHECK_LAUNCH("conv1x1_dma");
  return 0;
}

static bool conv_dma_eligible(const smt_conv_desc* d) {
  return d->dtype == SMT_BF16 && d->w_swizzled && d->c_in % 128 == 0 && d->c_out % 128 == 0 && d->stride == 1 &&
         d->out_stride == 1 && d->out_offset == 0 && d->t_y == d->t_out && d->zero_page != nullptr;
}

// Plan of the LDS-DMA family for one conv: dilation classes, then weight-stationary / 256-row / 128-row tiles.
struct DmaPlan { bool ws; WsPlan wsp; bool big; size_t lds; dim3 grid; };
static bool plan_conv_dma(ConvArgs& p, DmaPlan& pl) {
  // Dilation classes (see conv_gemm_dma_kernel) for same-size convs whose padding is a multiple of a large
  // dilation, as long as a class still has enough rows to fill tiles.
  p.rs = 1;
  if (p.dil >= 8 && p.taps > 1 && p.pad % p.dil == 0 && p.Tin == p.Tout && p.Tout / p.dil >= class_min_rows()) {
    p.rs = p.dil; p.pad /= p.dil; p.dil = 1;
  }
  const int tc_max = (p.Tout + p.rs - 1) / p.rs;
  pl.ws = plan_conv_ws(p, pl.wsp);    // the weight-stationary persistent kernels (conv_ws.hip)
  if (pl.ws) return true;
  auto lds_for = [&](int bm) {
    const int rows_in = (bm - 1) + (p.taps - 1) * p.dil + 1;
    const int rows_pad = (rows_in + 3) & ~3;
    const size_t a_bytes = align_up((size_t)std::max(rows_pad * 256, bm * (DMA_BN + 8) * 2), 1024);
    return a_bytes + (size_t)(p.taps > 1 ? 2 : 1) * DMA_BN * 256;   // one weight buffer suffices for 1x1
  };
  // 256-row tiles when they fit in LDS and there are enough rows to keep every CU busy
  pl.big = p.taps > 1 && lds_for(256) <= 160 * 1024 && (long long)tc_max * p.B * p.rs >= 256LL * 256 * 2;
  const int bm = pl.big ? 256 : 128;
  pl.lds = lds_for(bm);
  if (pl.lds > 160 * 1024) return false;
  p.tiles_per_batch = (tc_max + bm - 1) / bm;
  const int ntiles = p.tiles_per_batch * p.B * p.rs;
  pl.grid = dim3((unsigned)(8 * ((ntiles + 7) / 8)), (unsigned)(p.Cout / DMA_BN));
  return true;
}

static int launch_conv_dma(ConvArgs p, const void* zero_page, hipStream_t stream) {
  DmaPlan pl;
  SMT_CHECK_ARG(plan_conv_dma(p, pl), "conv_gemm_dma: tile needs %zu B of LDS", pl.lds);
  if (pl.ws) {
    launch_conv_ws(p, pl.wsp, zero_page, stream);
    SMT_CHECK_LAUNCH("conv_ws");
    return 0;
  }
  if (pl.big) {
    (void)hipFuncSetAttribute((const void*)conv_gemm_dma_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    conv_gemm_dma_kernel<4><<<pl.grid, DMA_NT, pl.lds, stream>>>(p, (const __bf16*)zero_page);
  } else {
    (void)hipFuncSetAttribute((const void*)conv_gemm_dma_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    conv_gemm_dma_kernel<2><<<pl.grid, DMA_NT, pl.lds, stream>>>(p, (const __bf16*)zero_page);
  }
  SMT_CHECK_LAUNCH("conv_gemm_dma");
  return 0;
}

template <typename T>
static size_t conv_gemm_lds_bytes(const ConvArgs& p, int BN) {
  constexpr int EPV = Tr<T>::EPV, CCH = Tr<T>::CCH, KC = Tr<T>::KC, BM = Tr<T>::BM;
  int rows_in = (BM - 1) * p.stride + (p.taps - 1) * p.dil + 1;
  int pitch_a = std::min(p.Cin, CCH) + EPV;
  size_t a = align_up((size_t)std::max(rows_in * pitch_a, BM * (BN + EPV)) * sizeof(T), 16);
  const int nsteps = p.taps * ((std::min(p.Cin, CCH) + KC - 1) / KC);
  return a + (size_t)(nsteps > 1 ? 2 : 1) * BN * (KC + EPV) * sizeof(T);
}

template <typename T>
static int launch_conv_gemm(ConvArgs p, hipStream_t stream) {
  constexpr int BM = Tr<T>::BM;
  const int BN = (p.Cout > 64) ? 128 : 64;
  p.tiles_per_batch = (p.Tout + BM - 1) / BM;
  const int ntiles = p.tiles_per_batch * p.B;
  dim3 grid((unsigned)(8 * ((ntiles + 7) / 8)), (unsigned)((p.Cout + BN - 1) / BN));
  size_t lds = conv_gemm_lds_bytes<T>(p, BN);
  SMT_CHECK_ARG(lds <= 160 * 1024, "conv_gemm: tile needs %zu B of LDS (taps=%d dil=%d stride=%d Cin=%d)", lds,
                p.taps, p.dil, p.stride, p.Cin);
  // two waves per SIMD (512 threads) for the 128-wide bf16 tiles; everything else keeps 256
  if (BN == 128) {
    constexpr int NT = sizeof(T) == 2 ? 512 : 256;
    (void)hipFuncSetAttribute((const void*)conv_gemm_kernel<T, 128, NT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    conv_gemm_kernel<T, 128, NT><<<grid, NT, lds, stream>>>(p);
  } else {
    (void)hipFuncSetAttribute((const void*)conv_gemm_kernel<T, 64, 256>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    conv_gemm_kernel<T, 64, 256><<<grid, 256, lds, stream>>>(p);
  }
  SMT_CHECK_LAUNCH("conv_gemm");
  return 0;
}

// ---- weight repacking: dst[tap][o][i] (act dtype) = src[o*so + i*si + jmap[tap]*sj] (fp32) ------------
struct PackArgs {
  const float* src; void* dst; int O, I, taps; long long so, si, sj; int jmap[16]; int swizzle;
};
template <typename T>
__global__ __launch_bounds__(256) void pack_weight_kernel(PackArgs p) {
  const long long total = (long long)p.taps * p.O * p.I;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    int i = (int)(e % p.I);
    int o = (int)((e / p.I) % p.O);
    int tap = (int)(e / ((long long)p.I * p.O));
    long long dst = e;
    if (p.swizzle) {  // LDS-DMA layout: within every 128-channel group the 8-channel chunk index is XORed with (o & 15)
      const int chunk = (i >> 3) & 15;
      dst = e - ((long long)chunk << 3) + ((long long)(chunk ^ (o & 15)) << 3);
    }
    reinterpret_cast<T*>(p.dst)[dst] = (T)p.src[o * p.so + i * p.si + p.jmap[tap] * p.sj];
  }
}

// Table-driven repack of MANY weights in one launch (the table lives in device memory and is built once by the
// host; parameter storage is stable across optimiser steps).  block_entry[b] = table row of block b,
// block_local[b] = its index among that row's blocks; 1024 elements per block.
__global__ __launch_bounds__(256) void pack_weights_batched_kernel(const smt_pack_entry* __restrict__ table,
                                                                   const int* __restrict__ block_entry,
                                                                   const int* __restrict__ block_local) {
  const smt_pack_entry e = table[block_entry[blockIdx.x]];
  const long long total = (long long)e.taps * e.n_out * e.n_in;
  const long long base = (long long)block_local[blockIdx.x] * 1024;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long long idx = base + u * 256 + threadIdx.x;
    if (idx >= total) break;
    const int i = (int)(idx % e.n_in);
    const int o = (int)((idx / e.n_in) % e.n_out);
    const int tap = (int)(idx / ((long long)e.n_in * e.n_out));
    int ipos = i;
    if (e.swizzle) ipos = (i & ~127) | ((((i >> 3) & 15) ^ (o & 15)) << 3) | (i & 7);
    const float v = e.src[o * e.stride_out + i * e.stride_in + e.tap_map[tap] * e.stride_tap];
    const long long d = e.dst_offset + (long long)tap * e.dst_tap_stride + (long long)o * e.dst_row_stride + ipos;
    if (e.dtype == SMT_BF16) reinterpret_cast<__bf16*>(e.dst)[d] = (__bf16)v;
    else reinterpret_cast<float*>(e.dst)[d] = v;
  }
}

}  // namespace smt

using namespace smt;

extern "C" int smt_pack_weights_batched(const smt_pack_entry* table_dev, const int* block_entry_dev,
                                        const int* block_local_dev, int n_blocks, smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_blocks <= 0) return 0;
  SMT_CHECK_ARG(table_dev && block_entry_dev && block_local_dev, "smt_pack_weights_batched: null pointer");
  pack_weights_batched_kernel<<<(unsigned)n_blocks, 256, 0, stream>>>(table_dev, block_entry_dev, block_local_dev);
  SMT_CHECK_LAUNCH("pack_weights_batched");
  return 0;
}

extern "C" int smt_pack_weight(const float* src, void* dst, int dtype, int n_out, int n_in, int taps,
                               int64_t stride_out, int64_t stride_in, int64_t stride_tap, const int* tap_map,
                               int swizzle, smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SMT_CHECK_ARG(src && dst && tap_map, "smt_pack_weight: null pointer");
  SMT_CHECK_ARG(taps >= 1 && taps <= 16, "smt_pack_weight: taps must be in [1, 16]");
  PackArgs p;
  p.src = src; p.dst = dst; p.O = n_out; p.I = n_in; p.taps = taps;
  p.so = stride_out; p.si = stride_in; p.sj = stride_tap;
  for (int t = 0; t < taps; ++t) p.jmap[t] = tap_map[t];
  SMT_CHECK_ARG(!swizzle || (n_in % 128 == 0 && dtype == SMT_BF16), "smt_pack_weight: swizzle needs bf16 and n_in %% 128 == 0");
  p.swizzle = swizzle;
  long long total = (long long)taps * n_out * n_in;
  unsigned grid = (unsigned)std::min<long long>(1024, (total + 255) / 256);
  if (dtype == SMT_BF16) pack_weight_kernel<__bf16><<<grid, 256, 0, stream>>>(p);
  else if (dtype == SMT_F32) pack_weight_kernel<float><<<grid, 256, 0, stream>>>(p);
  else SMT_CHECK_ARG(false, "smt_pack_weight: bad dtype %d", dtype);
  SMT_CHECK_LAUNCH("pack_weight");
  return 0;
}

static void conv_args_from_desc(const smt_conv_desc* d, ConvArgs& p) {
  p.x = d->x; p.w = d->w; p.bias = d->bias; p.y = d->y; p.res = d->res; p.gate_h = d->act_grad_src;
  p.lens_in = d->lens_in; p.lens_out = d->lens_out;
  p.x_bs = d->bs_x; p.y_bs = d->bs_y; p.res_bs = d->bs_res; p.gh_bs = d->bs_act;
  p.ldx = d->ld_x; p.ldy = d->ld_y; p.ldr = d->ld_res; p.ldgh = d->ld_act;
  p.B = d->batch; p.Tin = d->t_in; p.Tout = d->t_out; p.Cin = d->c_in; p.Cout = d->c_out;
  p.taps = d->taps; p.stride = d->stride; p.dil = d->dilation; p.pad = d->padding;
  p.out_stride = d->out_stride; p.out_offset = d->out_offset; p.Ty = d->t_y;
  p.y_act = d->y_act; p.ya_bs = d->bs_yact; p.ldya = d->ld_yact;
  p.act_out = d->act_out; p.epi_act = d->act_grad;
  for (int i = 0; i < 8; ++i) p.drop_keys[i] = d->drop_keys[i];
  p.drop_keys_dev = d->drop_keys_dev; p.drop_keys_dev_stride = d->drop_keys_dev_stride;
  p.site_width = d->site_width; p.drop_thresh16 = d->drop_thresh16; p.drop_scale = d->drop_scale;
  p.tiles_per_batch = 0;
  p.rs = 1;
  p.x2 = d->x2; p.w2 = d->w2; p.bias2 = d->bias2; p.lens_in2 = d->lens_in2; p.x2_bs = d->bs_x2; p.ldx2 = d->ld_x2;
  { static int dbg = getenv("SMT_CONV_DBG") ? atoi(getenv("SMT_CONV_DBG")) : 0; p.dbg = dbg; }
}

enum ConvKernelKind { K_GENERIC, K_1X1, K_DMA, K_WS, K_FOLD, K_K1ACT, K_C64 };
static bool conv_fold_eligible(const smt_conv_desc* d) {
  return d->x2 && d->w2 && d->c_in2 == 64 && d->taps == 1 && d->c_in == 128 && !d->res && !d->act_grad && !d->act_out &&
         d->y && d->ld_x2 % 8 == 0;
}
// the one dispatch rule (smt_conv1d_ntc and smt_conv1d_kernel_name both use it)
static ConvKernelKind pick_kernel(const smt_conv_desc* d, const ConvArgs& p0) {
  if (conv_k1act_eligible(d)) return K_K1ACT;
  if (conv1x1_c64_eligible(d)) return K_C64;
  if (!conv_dma_eligible(d)) return K_GENERIC;
  if (d->x2) return conv_fold_eligible(d) ? K_FOLD : K_GENERIC;
  if (d->taps == 1 && d->c_in == 128) return K_1X1;
  ConvArgs p = p0;
  DmaPlan pl;
  if (!plan_conv_dma(p, pl)) return K_GENERIC;
  return pl.ws ? K_WS : K_DMA;
}

extern "C" int smt_conv1d_ntc(const smt_conv_desc* d, smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SMT_CHECK_ARG(d && d->x && d->w && (d->y || d->y_act), "smt_conv1d_ntc: null pointer");
  const int epv = d->dtype == SMT_BF16 ? 8 : 4;
  SMT_CHECK_ARG(d->dtype == SMT_BF16 || d->dtype == SMT_F32, "smt_conv1d_ntc: bad dtype");
  SMT_CHECK_ARG(d->c_in % (2 * epv) == 0, "smt_conv1d_ntc: c_in=%d must be a multiple of %d", d->c_in, 2 * epv);
  SMT_CHECK_ARG(d->c_out % epv == 0, "smt_conv1d_ntc: c_out=%d must be a multiple of %d", d->c_out, epv);
  {
    const int cch = d->dtype == SMT_BF16 ? 128 : 64;
    const int first = d->c_in < cch ? d->c_in : cch;
    SMT_CHECK_ARG((first & (first - 1)) == 0 && (d->c_in <= cch || d->c_in % cch == 0),
                  "smt_conv1d_ntc: c_in=%d must be a power of two up to %d or a multiple of it", d->c_in, cch);
    SMT_CHECK_ARG(!d->act_out || d->site_width % 2 == 0, "smt_conv1d_ntc: site_width must be even");
  }
  SMT_CHECK_ARG(d->ld_x % epv == 0 && d->ld_y % epv == 0 && (!d->res || d->ld_res % epv == 0) &&
                    (!d->act_grad_src || d->ld_act % epv == 0),
                "smt_conv1d_ntc: row pitches must keep 16-byte alignment");
  SMT_CHECK_ARG(d->taps >= 1 && d->stride >= 1 && d->dilation >= 1 && d->out_stride >= 1, "smt_conv1d_ntc: bad geometry");
  SMT_CHECK_ARG(!d->act_grad || d->act_grad_src, "smt_conv1d_ntc: act_grad needs act_grad_src");
  SMT_CHECK_ARG(!d->act_out || (d->y_act && d->site_width > 0 && d->site_width % epv == 0 && d->ld_yact % epv == 0 &&
                                (d->c_out + d->site_width - 1) / d->site_width <= 8),
                "smt_conv1d_ntc: act_out needs y_act and 1..8 sites of site_width channels");
  if (d->batch == 0 || d->t_out == 0) return 0;
  ConvArgs p;
  conv_args_from_desc(d, p);
  const ConvKernelKind kind = pick_kernel(d, p);
  SMT_CHECK_ARG(!d->x2 || kind == K_FOLD,
                "smt_conv1d_ntc: the folded second term needs the bf16 1x1 LDS-DMA path (c_in 128, c_in2 64, no other epilogue)");
  switch (kind) {
    case K_FOLD: return launch_conv1x1_fold(p, d->zero_page, stream);
    case K_K1ACT: return launch_conv_k1act(p, d->zero_page, stream);
    case K_C64: return launch_conv1x1_c64(p, stream);
    case K_1X1: return launch_conv1x1_dma(p, d->zero_page, stream);
    case K_DMA: case K_WS: return launch_conv_dma(p, d->zero_page, stream);
    default: break;
  }
  SMT_CHECK_ARG(!d->w_swizzled, "smt_conv1d_ntc: swizzled weights need the LDS-DMA path (bf16, stride 1, channels %% 128)");
  if (d->dtype == SMT_BF16) return launch_conv_gemm<__bf16>(p, stream);
  return launch_conv_gemm<float>(p, stream);
}

extern "C" const char* smt_conv1d_kernel_name(const smt_conv_desc* d) {
  if (!d) return "";
  ConvArgs p;
  conv_args_from_desc(d, p);
  switch (pick_kernel(d, p)) {
    case K_1X1: return "conv1x1_dma";
    case K_FOLD: return "conv1x1_fold";
    case K_K1ACT: return "conv_k1act";
    case K_C64: return "conv1x1_c64";
    case K_WS: return conv_ws_variant_name(p);
    case K_DMA: return "conv_gemm_dma";
    default: return "conv_gemm";
  }
}

// What plan_conv_dma decided for a descriptor that pick_kernel sends to conv_gemm_dma_kernel: the tile's rows and the
// number of dilation classes.  Zeros for every other kernel.
extern "C" int smt_conv1d_dma_plan(const smt_conv_desc* d, int* tile_rows, int* row_classes) {
  if (tile_rows) *tile_rows = 0;
  if (row_classes) *row_classes = 0;
  if (!d) return 0;
  ConvArgs p;
  conv_args_from_desc(d, p);
  if (pick_kernel(d, p) != K_DMA) return 0;
  DmaPlan pl;
  plan_conv_dma(p, pl);                      // sets p.rs and pl.big, as in launch_conv_dma
  if (tile_rows) *tile_rows = pl.big ? 256 : 128;
  if (row_classes) *row_classes = p.rs;
  return 0;
}
