// Weight / bias gradients of the channels-last convolutions (autograd of F.conv1d /
// F.conv_transpose1d in the reference, models/vqvae/conv.py, resnet.py) on the matrix cores.
//
//   dw[j][co][ci] = sum_{b,t} dy[b, t*os + oo, co] * pro(x)[b, t*stride + j*dil - pad, ci]
//
// The contraction runs over ROWS (time), which is the slow axis of both channels-last operands.
// Tiles are staged row-major into LDS exactly as in the forward kernel (same prologue) and the MFMA
// fragments are read TRANSPOSED:  bf16 with ds_read_b64_tr_b16 (4 rows x 16 channels per 16-lane
// group, delivered channel-major -- the hardware transpose), fp32 with plain ds_read_b32 (one scalar
// per lane per MFMA at the fp32 rate).  A row shift for tap j only moves the row index, so no
// alignment constraint arises from odd dilations.
//
// Decomposition: workgroup = 4 waves (2x2) = a 64(co) x 64(ci) block of dw for ALL taps (<= 9 taps x 16
// accumulator registers) over one chunk of rows; partial blocks go to a slab and a second kernel
// reduces the chunks in fixed order (deterministic) into the fp32 torch-layout gradient.  The bias
// gradient rides along as one extra "tap" whose x operand is the constant 1.
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "conv_common.h"

namespace smt {

struct WgradArgs {
  const void* x; const void* dy; float* slab;
  const int* lens_in;
  long long x_bs, dy_bs;
  int ldx, ldy;
  int B, Tin, Tout, Ty, Cin, Cout;
  int taps, stride, dil, pad, out_stride, out_offset;
  int rows_per_chunk, chunks_per_batch, nblk_ci, nblk_co, with_bias;
};

// R = rows per staged tile; CIB = input channels per workgroup (CIB/32 wave columns, 2 wave rows);
// pitches chosen so that the transposed reads are bank-conflict-free: for ds_read_b64_tr_b16 a
// 32-lane half touches 4 rows x 2 16-column blocks, which need row pitch == 16 dwords (mod 64).
template <typename T> struct WTr;
template <> struct WTr<__bf16> {
  static constexpr int R = 128;
  static constexpr int pitch(int ch) { return ch + 32; }   // 64 ch: 192 B == 48 dwords; 128 ch: 320 B == 16 (mod 64)
};
template <> struct WTr<float> {
  static constexpr int R = 64;
  static constexpr int pitch(int ch) { return ch + 4; }
};

// Transposed fragments (ds_read_b64_tr_b16): element e of lane (n = lane&31, hh = lane>>5) is tile[row + 8*hh + e][col + n].
// A lane addresses row tr_lane_row, column tr_lane_col of the 16 x 32 block and reads twice, four rows apart.
__device__ __forceinline__ int tr_lane_row(int lane) { return 8 * (lane >> 5) + ((lane & 15) >> 2); }
__device__ __forceinline__ int tr_lane_col(int lane) { return 16 * ((lane >> 4) & 1) + 4 * (lane & 3); }
__device__ __forceinline__ bf16x8 tr_read2(const void* a0, int step4_bytes) {
  const unsigned char* a = reinterpret_cast<const unsigned char*>(a0);
  return lds_tr2(a, a + step4_bytes);
}
__device__ __forceinline__ bf16x8 frag_tr_bf16(const __bf16* tile, int pitch, int row0, int col0, int lane) {
  return tr_read2(tile + (row0 + tr_lane_row(lane)) * pitch + col0 + tr_lane_col(lane), 4 * pitch * 2);
}

// Workgroup -> (global chunk index cgl, block blk of the nblk 64 x CIB blocks of dw).  XCD-aware order: the blocks of one row
// chunk run back to back on the same XCD (ids == mod 8), so the second reader of a chunk's rows hits L2.
struct WgBlock { int nblk, blk, cgl; };
__device__ __forceinline__ WgBlock wgrad_block(int nblk_ci, int nblk_co) {
  WgBlock w;
  w.nblk = nblk_ci * nblk_co;
  const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
  w.blk = q % w.nblk;
  w.cgl = (q / w.nblk) * 8 + xcd;
  return w;
}

#ifndef SMT_WGRAD_STAMP
#define SMT_WGRAD_STAMP 0   // diagnostic build (tools/wgrad_phases.sh): per-wave cycle sums of the phases of conv_wgrad_kernel and conv_wgrad_shift_kernel
#endif
#if SMT_WGRAD_STAMP
// [workgroup < 256][wave][barrier | stage | k-loop | slab store | tiles]: written here, read by smt_wgrad_debug_dump only
__device__ unsigned long long wg_dbg[256 * 8 * 8];
__device__ __forceinline__ unsigned long long wg_stamp() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
// the sums stay in scalar registers during the tile loop and leave the kernel once, after the slab store
#define WG_SUMS unsigned long long wg_sum[5] = {0, 0, 0, 0, 0}
#define WG_T(var) const unsigned long long var = wg_stamp()
#define WG_ACC(k, a, b) wg_sum[k] += (b) - (a)
#define WG_DUMP do { if (lane == 0 && blockIdx.x < 256) for (int k_ = 0; k_ < 5; ++k_) wg_dbg[(blockIdx.x * 8 + wave) * 8 + k_] += wg_sum[k_]; } while (0)
#else
#define WG_SUMS do {} while (0)
#define WG_T(var) do {} while (0)
#define WG_ACC(k, a, b) do {} while (0)
#define WG_DUMP do {} while (0)
#endif

// Quotient by a divisor fixed for the launch: q = n / s as one v_mul_hi_u32 with magic = ceil(2^32 / s); exact while
// n * s < 2^32 (here n is a staged row, below 1,000)
__device__ __forceinline__ unsigned div_magic(int s) { return 0xffffffffu / (unsigned)s + 1u; }

// NT = accumulator planes (taps + bias plane); CIB = input channels per workgroup; STRIDED = stride > 1
//
// The tile loop overlaps staging with the k-loop through a register prefetch: the global loads of tile i+1 are issued
// right before the k-loop of tile i and retired into LDS after it, behind the barrier that frees the (single) LDS buffer.
// A thread keeps the dy tile and the first XS slots of the x tile that way (9 or 13 16-byte vectors at 64 channels), which is
// the whole tile for a halo of up to 32 rows at stride 1 and for the k = 4 stride-2 conv; what a wider halo adds is loaded
// at the store, as the whole tile used to be.  (On the flagship's 64-channel resampling convs the prefetch is worth 2-4 % at
// the largest level and nothing measurable below it; the k-loop changes carry the gain: profiles/wgrad_generic_ab.txt.)
//
// bf16, STRIDED: the haloed x rows are staged into `stride` planes by row residue (plane q holds the staged rows
// == q mod stride, in order; the planes follow each other, so the tile takes the same rows_x rows of LDS).  The x row of
// (k, tap j), k * stride + j * dil, is then row k + (j * dil) / stride of plane (j * dil) % stride: 16 consecutive k are 16
// consecutive LDS rows, and the B fragment of a tap is the same pair of transposed reads as at stride 1.
//
// Per instance: whether the prefetch is on, and the waves per SIMD the register allocation must leave room for
// (profiles/wgrad_generic_ab.txt has the table these come from).
#ifndef SMT_WGRAD_PREFETCH
#define SMT_WGRAD_PREFETCH -1   // diagnostic builds: 0 / 1 = the prefetch off / on in every instance
#endif
#ifndef SMT_WGRAD_WAVES
#define SMT_WGRAD_WAVES 0       // diagnostic builds: waves per SIMD of every instance
#endif
constexpr bool wgrad_prefetch(int esz, int nt, int cib, bool strided) {
  if (SMT_WGRAD_PREFETCH >= 0) return SMT_WGRAD_PREFETCH != 0;
  return true;                                        // every instance holds it without scratch at the occupancy below
}
// The most waves the LDS tile admits anyway (three 49 KB workgroups of 64 bf16 channels at stride 1; two at stride 2) that
// the accumulators, the prefetch and two fragment requests fit without scratch.
constexpr int wgrad_waves_per_simd(int esz, int nt, int cib, bool strided) {
  if (SMT_WGRAD_WAVES > 0) return SMT_WGRAD_WAVES;
  if (cib == 128) return 2;                           // 8 waves per workgroup
  if (esz == 2) return (!strided && nt <= 4) ? 3 : 2;
  return nt <= (strided ? 4 : 5) ? 3 : 2;
}
template <typename T, int NT, int CIB, bool STRIDED>
__global__ __launch_bounds__(CIB * 4) __attribute__((amdgpu_waves_per_eu(wgrad_waves_per_simd(sizeof(T), NT, CIB, STRIDED))))
void conv_wgrad_kernel(WgradArgs p) {
  constexpr int EPV = Tr<T>::EPV;
  constexpr int R = WTr<T>::R;          // rows per staged tile
  constexpr int CB = 64;                // output channels per block
  constexpr int WNC = CIB / 32;         // wave columns
  constexpr int NTHR = 128 * WNC;
  constexpr int PITCH_DY = WTr<T>::pitch(CB), PITCH_X = WTr<T>::pitch(CIB);
  constexpr bool PLANES = STRIDED && sizeof(T) == 2;
  constexpr bool PREFETCH = wgrad_prefetch(sizeof(T), NT, CIB, STRIDED);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WNC, wn = wave % WNC;
  const int r = lane & 31, hh = lane >> 5;

  const WgBlock w = wgrad_block(p.nblk_ci, p.nblk_co);
  if (w.cgl >= p.B * p.chunks_per_batch) return;
  const int co0 = (w.blk / p.nblk_ci) * CB, ci0 = (w.blk % p.nblk_ci) * CIB;
  const int b = w.cgl / p.chunks_per_batch;
  const int chunk = w.cgl % p.chunks_per_batch;
  const int t_begin = chunk * p.rows_per_chunk;
  const int t_end = min(p.Tout, t_begin + p.rows_per_chunk);

  const int rows_x = (R - 1) * p.stride + (p.taps - 1) * p.dil + 1;
  T* lds_dy = reinterpret_cast<T*>(smem);                 // [R][PITCH_DY]
  T* lds_x = lds_dy + R * PITCH_DY;                       // [rows_x][PITCH_X]
  const T* xg = reinterpret_cast<const T*>(p.x) + (long long)b * p.x_bs;
  const T* dyg = reinterpret_cast<const T*>(p.dy) + (long long)b * p.dy_bs;
  const int len_in = p.lens_in ? min(p.lens_in[b], p.Tin) : p.Tin;
  const bool bias_plane = p.with_bias && (ci0 == 0);

  // LDS row of staged x row `row` (0 <= row < rows_x): planes 0 .. rows_x % stride - 1 hold one row more than the others
  const unsigned s_magic = PLANES ? div_magic(p.stride) : 0u;
  const int plane_q = PLANES ? rows_x / p.stride : 0, plane_rem = PLANES ? rows_x % p.stride : 0;
  auto lds_row_x = [&](int row) {
    if constexpr (!PLANES) return row;
    const int q = (int)__umulhi((unsigned)row, s_magic), pl = row - q * p.stride;
    return pl * plane_q + min(pl, plane_rem) + q;
  };

  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;

  // Staging: a thread moves one 16-byte vector per slot, always the same channels; a slot is RPS_DY rows of the dy tile (rows
  // t0.., channels co0..co0+64) or RPS_X rows of the haloed x tile.  Rows >= t_end, ty >= Ty, tin outside [0, len_in) and
  // channels beyond Cin / Cout are zeros.  Slots 0 .. DYS-1 (dy) and the first XS of x are prefetched.
  typedef Vec<T, EPV> V;
  constexpr int VPR_DY = CB / EPV, VPR_X = CIB / EPV;
  constexpr int RPS_DY = NTHR / VPR_DY, RPS_X = NTHR / VPR_X;
  constexpr int DYS = R / RPS_DY;
  constexpr int XS = STRIDED ? 9 : 5;    // 5: a halo of up to 32 (fp32: 16) rows at stride 1; 9: k = 4 at stride 2
  constexpr int UB = 4;                  // beyond them: loads in flight per thread
  static_assert(R % RPS_DY == 0, "whole slots");
  const int rd = tid / VPR_DY, cd = (tid % VPR_DY) * EPV, rx = tid / VPR_X, cx = (tid % VPR_X) * EPV;
  const bool cd_ok = co0 + cd < p.Cout, cx_ok = ci0 + cx < p.Cin;
  auto fetch_dy = [&](int t0, int slot_row) {
    V v;
#pragma unroll
    for (int e = 0; e < EPV; ++e) v.v[e] = (T)0.f;
    const int t = t0 + slot_row + rd;
    const int ty = t * p.out_stride + p.out_offset;
    if (t < t_end && ty < p.Ty && cd_ok) v = *reinterpret_cast<const V*>(dyg + (long long)ty * p.ldy + co0 + cd);
    return v;
  };
  auto fetch_x = [&](int t0, int slot_row) {
    V v;
#pragma unroll
    for (int e = 0; e < EPV; ++e) v.v[e] = (T)0.f;
    const int row = slot_row + rx;
    const int tin = t0 * p.stride - p.pad + row;
    if (row < rows_x && tin >= 0 && tin < len_in && cx_ok) v = *reinterpret_cast<const V*>(xg + (long long)tin * p.ldx + ci0 + cx);
    return v;
  };
  auto put_dy = [&](int slot_row, const V& v) { *reinterpret_cast<V*>(lds_dy + (slot_row + rd) * PITCH_DY + cd) = v; };
  auto put_x = [&](int slot_row, const V& v) {
    const int row = slot_row + rx;
    if (row < rows_x) *reinterpret_cast<V*>(lds_x + lds_row_x(row) * PITCH_X + cx) = v;
  };
  V pf_dy[DYS], pf_x[XS];
  auto prefetch = [&](int t0) {
#pragma unroll
    for (int u = 0; u < DYS; ++u) pf_dy[u] = fetch_dy(t0, u * RPS_DY);
#pragma unroll
    for (int u = 0; u < XS; ++u) pf_x[u] = fetch_x(t0, u * RPS_X);
  };

  // bf16: per-lane LDS byte addresses of the transposed fragments of k-step 0 (dy, and x per tap)
  static_assert(NT >= 2, "at least one tap and the bias plane");
  constexpr int NB = NT - 1;                // taps: the launch picks the instance with NT == taps + 1 (SMT_WG_BY_PLANES)
  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  struct Frags { u32x2 a0, a1, b0[NB], b1[NB]; };
  constexpr int NREAD = 2 + 2 * NB;         // ds_read instructions per request
  static_assert(NREAD <= 15, "lgkmcnt counts up to 15");
  unsigned a_addr = 0, x_addr[NB];
  if constexpr (sizeof(T) == 2) {
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
    a_addr = lds0 + (unsigned)(tr_lane_row(lane) * PITCH_DY + wm * 32 + tr_lane_col(lane)) * 2u;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int row_j = lds_row_x(j * p.dil);
      x_addr[j] = lds0 + (unsigned)(R * PITCH_DY + (row_j + tr_lane_row(lane)) * PITCH_X + wn * 32 + tr_lane_col(lane)) * 2u;
    }
  }
  // The fragments of k-step k+1 are requested (asm, so that the requests stay where they are written) before the MFMAs of
  // k-step k; `s_waitcnt lgkmcnt(NREAD)` then retires exactly the older request (LDS returns in order), and the wait
  // pins the fragments so that nothing that uses them can be scheduled above it.  Two requests are in flight at most:
  // hoisting the reads of all eight k-steps would spill.
  // (the k-step arrives as a type, so that its row offset goes into the instructions' offset fields)
  auto request = [&](Frags& f, auto ks_) {
    constexpr int KS = decltype(ks_)::value;
    const unsigned pa = a_addr;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(f.a0) : "v"(pa), "n"(KS * 16 * PITCH_DY * 2));
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(f.a1) : "v"(pa), "n"((KS * 16 + 4) * PITCH_DY * 2));
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const unsigned px = x_addr[j];
      asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(f.b0[j]) : "v"(px), "n"(KS * 16 * PITCH_X * 2));
      asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(f.b1[j]) : "v"(px), "n"((KS * 16 + 4) * PITCH_X * 2));
    }
  };
  static_assert((R + 4) * PITCH_X * 2 < 65536, "the k-step offsets fit the 16-bit offset field");
  bf16x8 ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;
  Frags fr[2];
  auto k_step = [&](auto ks_) {
    constexpr int KS = decltype(ks_)::value;
    Frags& f = fr[KS & 1];
    if constexpr (KS + 1 < R / 16) {
      request(fr[(KS + 1) & 1], std::integral_constant<int, KS + 1>{});
      lgkm_wait<NREAD>(f.a0, f.a1, f.b0, f.b1);
    } else {
      lgkm_wait<0>(f.a0, f.a1, f.b0, f.b1);
    }
    const u32x4 aw = {f.a0[0], f.a0[1], f.a1[0], f.a1[1]};
    const bf16x8 a = __builtin_bit_cast(bf16x8, aw);               // A[co][k] = dy[k][co]
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      if (j < NB) {
        const int jb = j < NB ? j : 0;
        const u32x4 bw = {f.b0[jb][0], f.b0[jb][1], f.b1[jb][0], f.b1[jb][1]};   // B[k][ci] = x[k * stride + j * dil][ci]
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, bw), acc[j], 0, 0, 0);
      }
    }
    if (bias_plane) acc[NB] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, ones, acc[NB], 0, 0, 0);
  };

  WG_SUMS;
  if constexpr (PREFETCH) prefetch(t_begin);
  for (int t0 = t_begin; t0 < t_end; t0 += R) {
    WG_T(c0);
    __syncthreads();                       // every wave has left the k-loop of the previous tile: the LDS tile is free
    WG_T(c1);
    if constexpr (!PREFETCH) prefetch(t0);   // no overlap: all loads of the tile, then the stores
#pragma unroll
    for (int u = 0; u < DYS; ++u) put_dy(u * RPS_DY, pf_dy[u]);
#pragma unroll
    for (int u = 0; u < XS; ++u) put_x(u * RPS_X, pf_x[u]);
    for (int row0 = XS * RPS_X; row0 < rows_x; row0 += UB * RPS_X) {   // a wider halo: what is not prefetched
      V v[UB];
#pragma unroll
      for (int u = 0; u < UB; ++u) v[u] = fetch_x(t0, row0 + u * RPS_X);
      // every path waits for these loads here: left to the stores, the wait sits in a branch that rows beyond the halo skip,
      // and the compiler would then wait for ALL vector memory -- the prefetch included -- at the first k-step
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        f32x4 t = __builtin_bit_cast(f32x4, v[u]);
        pin_v(t);
        v[u] = __builtin_bit_cast(V, t);
      }
#pragma unroll
      for (int u = 0; u < UB; ++u) put_x(row0 + u * RPS_X, v[u]);
    }
    WG_T(c2);
    __syncthreads();
    WG_T(c3);
    if constexpr (PREFETCH)
      if (t0 + R < t_end) prefetch(t0 + R);   // in flight during the k-loop

    if constexpr (sizeof(T) == 2) {
      static_assert(sizeof(T) != 2 || R == 128, "eight k-steps, written out");
      __builtin_amdgcn_sched_barrier(0);   // the lgkmcnt counts of the k-steps must see these LDS reads only
      request(fr[0], std::integral_constant<int, 0>{});
      k_step(std::integral_constant<int, 0>{}); k_step(std::integral_constant<int, 1>{});
      k_step(std::integral_constant<int, 2>{}); k_step(std::integral_constant<int, 3>{});
      k_step(std::integral_constant<int, 4>{}); k_step(std::integral_constant<int, 5>{});
      k_step(std::integral_constant<int, 6>{}); k_step(std::integral_constant<int, 7>{});
      __builtin_amdgcn_sched_barrier(0);
    } else {
      const float* dyt = reinterpret_cast<const float*>(lds_dy);
      const float* xt = reinterpret_cast<const float*>(lds_x);
#pragma unroll 2
      for (int k0 = 0; k0 < R; k0 += 2) {
        const float a = dyt[(k0 + hh) * PITCH_DY + wm * 32 + r];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          if (j < NB) {
            const float bv = xt[((k0 + hh) * p.stride + j * p.dil) * PITCH_X + wn * 32 + r];
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc[j], 0, 0, 0);
          }
        }
        if (bias_plane) acc[NB] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, 1.0f, acc[NB], 0, 0, 0);
      }
    }
    WG_T(c4);
    WG_ACC(0, c0, c1); WG_ACC(0, c2, c3); WG_ACC(1, c1, c2); WG_ACC(2, c3, c4); WG_ACC(4, c0, c0 + 1);
  }
  WG_T(c5);
  // partial block -> slab[chunk_global][blk][plane][co 64][ci CIB]
  // (the slab layout always carries the bias plane: zeros when not requested)
  float* out = p.slab + ((size_t)w.cgl * w.nblk + w.blk) * (size_t)NT * CB * CIB;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;  // co
      const int col = wn * 32 + r;                                 // ci
      out[((size_t)j * CB + row) * CIB + col] = acc[j][e];
    }
  }
  WG_T(c6);
  WG_ACC(3, c5, c6);
  WG_DUMP;
}

// ------------------------------------------------------------------------------------------------
// LDS-DMA variant (bf16, stride 1, C_in % 128 == 0, C_out % 64 == 0): the dy / x row tiles go
// HBM/L2 -> LDS with buffer_load ... lds into a DOUBLE buffer (tile i+1 lands while tile i is
// multiplied), rows unpadded.  The transposed reads stay conflict-free through an XOR swizzle of the
// 16-byte chunk index, applied on the source address while staging:
//   x  rows (256 B): chunk ^ ((row & 3) << 2)        dy rows (128 B): chunk ^ (((row >> 1) & 1) << 2)
// (a 32-lane half of ds_read_b64_tr_b16 touches 4 rows x 64 B; the swizzles put those on 4 distinct
// 64-byte slots of the 256-byte bank row).
__device__ __forceinline__ int swz_dy(int row) { return ((row >> 1) & 1) << 2; }
__device__ __forceinline__ int swz_x(int row) { return (row & 3) << 2; }
// byte offset of bf16 column `col` of a swizzled row (swz = swz_dy / swz_x of that row)
__device__ __forceinline__ int swz_col_bytes(int col, int swz) { return (((col >> 3) ^ swz) << 4) + (col & 7) * 2; }

template <int NT>
__global__ __launch_bounds__(512) void conv_wgrad_dma_kernel(WgradArgs p) {
  typedef __bf16 T;
  constexpr int R = 128, CB = 64, CIB = 128, WNC = 4, NTHR = 512;
  constexpr int DYB = CB * 2, XB = CIB * 2;         // row bytes
  constexpr int DY_BYTES = R * DYB;                 // 16 KiB
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WNC, wn = wave % WNC;
  const int r = lane & 31, hh = lane >> 5;

  const WgBlock w = wgrad_block(p.nblk_ci, p.nblk_co);
  if (w.cgl >= p.B * p.chunks_per_batch) return;
  const int co0 = (w.blk / p.nblk_ci) * CB, ci0 = (w.blk % p.nblk_ci) * CIB;
  const int b = w.cgl / p.chunks_per_batch;
  const int chunk = w.cgl % p.chunks_per_batch;
  const int t_begin = chunk * p.rows_per_chunk;
  const int t_end = min(p.Tout, t_begin + p.rows_per_chunk);

  const int rows_x = (R - 1) + (p.taps - 1) * p.dil + 1;
  const int rows_x_pad = (rows_x + 3) & ~3;
  const size_t buf_bytes = (size_t)DY_BYTES + (size_t)rows_x_pad * XB;
  const T* xg = reinterpret_cast<const T*>(p.x) + (long long)b * p.x_bs;
  const T* dyg = reinterpret_cast<const T*>(p.dy) + (long long)b * p.dy_bs;
  const int len_in = max(0, p.lens_in ? min(p.lens_in[b], p.Tin) : p.Tin);
  const bool bias_plane = p.with_bias && (ci0 == 0);
  const int ntaps = p.taps;

  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;

  // Untracked LDS-DMA through range-checked V#s (conv_stream.h): the compiler used to put a wait for the NEXT tile's
  // prefetch in front of the first transposed read of the current tile, so nothing overlapped.  An offset of ~0 is out of
  // range of any descriptor: such lanes read zero (rows past the chunk, before the item, past the valid length).
  const UntrackedRsrc rdy = untracked_rsrc(dyg + co0, 0, (unsigned)min((long long)0xfffffff0ll, (long long)p.Tout * p.ldy * 2));
  const UntrackedRsrc rxx = untracked_rsrc(xg + ci0, 0, (unsigned)min((long long)0xfffffff0ll, (long long)len_in * p.ldx * 2));
  const unsigned pdy = (unsigned)(p.ldy * 2), pxx = (unsigned)(p.ldx * 2);
  auto stage = [&](int t0, int buf) {
    unsigned char* base = smem + (size_t)buf * buf_bytes;
    // dy: 128 rows x 8 chunks; one wave-instruction = 8 rows
    for (int g = wave; g < R / 8; g += NTHR / 64) {
      const int row = 8 * g + (lane >> 3), pos = lane & 7;
      const int t = t0 + row;
      const int ch = pos ^ swz_dy(row);
      untracked_dma16(rdy, t < t_end ? (unsigned)t * pdy + (unsigned)(ch << 4) : 0xffffff00u, base + g * 1024);
    }
    // x: rows_x_pad rows x 16 chunks; one wave-instruction = 4 rows
    const int tin0 = t0 - p.pad;
    for (int g = wave; g < rows_x_pad / 4; g += NTHR / 64) {
      const int row = 4 * g + (lane >> 4), pos = lane & 15;
      const int ch = pos ^ swz_x(row);
      const int tin = tin0 + row;
      const bool ok = (row < rows_x) && (tin >= 0) && (tin < len_in);
      untracked_dma16(rxx, ok ? (unsigned)tin * pxx + (unsigned)(ch << 4) : 0xffffff00u, base + DY_BYTES + g * 1024);
    }
  };

  bf16x8 ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;

  // Per-lane fragment offsets, computed ONCE: the k-step advances rows by 16 (a multiple of 4), so the
  // swizzle term of a lane depends only on the tap.  Inside the loop every transposed read is then
  // "base + lane offset + compile-time immediate" -- no address arithmetic between the MFMAs.
  const int lrow = tr_lane_row(lane);
  const int coly = wm * 32 + tr_lane_col(lane), colx = wn * 32 + tr_lane_col(lane);
  const int dyoff = lrow * DYB + swz_col_bytes(coly, swz_dy(lrow));
  int xoff[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int rj = lrow + j * p.dil;
    xoff[j] = rj * XB + swz_col_bytes(colx, swz_x(rj));
  }

  stage(t_begin, 0);
  vm_wait<0>();
  int buf = 0;
  for (int t0 = t_begin; t0 < t_end; t0 += R, buf ^= 1) {
    lgkm_wait<0>();
    __builtin_amdgcn_s_barrier();          // this tile has landed for every wave (each waited at the end of the previous
                                           // iteration); the buffer read in the previous iteration is free
    if (t0 + R < t_end) stage(t0 + R, buf ^ 1);
    const unsigned char* dyt = smem + (size_t)buf * buf_bytes + dyoff;
    const unsigned char* xbase = smem + (size_t)buf * buf_bytes + DY_BYTES;
#pragma unroll
    for (int k0 = 0; k0 < R; k0 += 16) {
      const bf16x8 a = tr_read2(dyt + k0 * DYB, 4 * DYB);
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        if (j < ntaps) {
          const bf16x8 bfrag = tr_read2(xbase + xoff[j] + k0 * XB, 4 * XB);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bfrag, acc[j], 0, 0, 0);
        } else if (j == ntaps && bias_plane) {
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, ones, acc[j], 0, 0, 0);
        }
      }
    }
    step_end_wait<0>();                    // the next tile must have landed
  }
  const int planes = ntaps + 1;
  float* out = p.slab + ((size_t)w.cgl * w.nblk + w.blk) * (size_t)planes * CB * CIB;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    if (j >= planes) break;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
      const int col = wn * 32 + r;
      out[((size_t)j * CB + row) * CIB + col] = acc[j][e];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Shifted-fragment variant for the dilated 128-channel convs (bf16, stride 1, <= 9 taps at distance 1 in the
// row domain -- natively, or after the dilation-class decomposition of conv_gemm_dma_kernel: rows t = cls (mod
// dilation) form `rs` independent dense problems).  The x operand of tap s is the x operand of tap 0 moved down
// s rows, and an MFMA B fragment holds 8 consecutive rows per lane, so all taps of a k-step are windows of ONE
// 16-row register window W = [P | Q] (P: rows 16 k0 + 8 hh + 0..7, Q: the next 8):
//     even s: B_s = dwords s/2 .. s/2+3 of W (register renaming, free)
//     odd  s: B_s[i] = v_alignbit(W[(s+1)/2 + i], W[(s-1)/2 + i], 16)
// Per k-step a wave reads 3 fragments from LDS (dy^T, P, Q) for up to 9 (+1 bias) MFMAs, where the per-tap
// kernel above reads one per MFMA -- that kernel is LDS-bandwidth bound.  All taps are handled in one launch
// (accumulators: 10 planes x 16 registers), and a workgroup walks a contiguous range of 128-row tiles across
// (batch, class) items, so the number of partial slabs does not grow with the number of classes.
struct ShiftArgs {
  const void* x; const void* dy; float* slab; const int* lens_in;
  long long x_bs, dy_bs;
  int ldx, ldy;
  int B, Tin, Tout, pad, rs;
  int tiles_per_item, tiles_per_wg, n_chunks, nblk_ci, nblk_co, with_bias;
};

constexpr int SH_R = 128, SH_XROWS = SH_R + 8, SH_DY = SH_R * 128, SH_X = SH_XROWS * 256, SH_STAGE = SH_DY + SH_X;

template <int NTAPS>
__global__ __launch_bounds__(512) void conv_wgrad_shift_kernel(ShiftArgs p, const __bf16* __restrict__ zero_page) {
  constexpr int CB = 64, CIB = 128, WNC = 4, DYB = CB * 2, XB = CIB * 2, PLANES = NTAPS + 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // scalar: the LDS base of a piece goes to M0 without a VALU detour
  const int wm = wave / WNC, wn = wave % WNC;
  const int r = lane & 31, hh = lane >> 5;

  const WgBlock w = wgrad_block(p.nblk_ci, p.nblk_co);
  if (w.cgl >= p.n_chunks) return;
  const int co0 = (w.blk / p.nblk_ci) * CB, ci0 = (w.blk % p.nblk_ci) * CIB;
  const int ntiles = p.tiles_per_item * p.B * p.rs;
  const int tile_begin = w.cgl * p.tiles_per_wg;
  const int tile_end = min(ntiles, tile_begin + p.tiles_per_wg);
  const int rs = p.rs;
  const bool bias_plane = p.with_bias && (ci0 == 0);

  f32x16 acc[PLANES];
#pragma unroll
  for (int j = 0; j < PLANES; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;

  // Staging through range-checked V#s (conv_stream.h: ws_rsrc / ws_dma16), as in conv_ws.hip: one descriptor per operand
  // and tile covers the valid class-domain rows of the tile's item (dy: Tc rows, x: len_in rows), a lane's source is a 32-bit
  // byte offset = tile-invariant lane part + a scalar per tile, and whatever lies outside -- rows before the item (the offset
  // wraps to ~4 GiB), rows at or past Tc / len_in, rows no tap reads -- is out of range and lands in LDS as zero.  (The plan
  // keeps every in-range offset below 2^31.)  A wave stages SH_PIECES pieces per tile, each one DMA instruction = 1 KiB:
  //   pieces 0, 1: dy rows 8 wave + 64 i + (lane >> 3), 8 chunks of 16 B per row
  //   pieces 2..5: x rows 4 wave + 32 (i - 2) + (lane >> 4), 16 chunks per row;  piece 6: x rows 128 + ..., waves 0 and 1 only
  constexpr int SH_PIECES = 7;
  // pieces per k-step of the k-loop: two, behind the first two MFMAs of k-steps 0..3, so that the last piece has half a tile
  // to land (one per k-step measured the same at 7 and 9 taps and 2-5 % slower per tile at 3 and 5: the wait at the top of
  // the next tile grows)
  constexpr int SH_PPS = 2;
  static_assert(SH_PPS <= NTAPS && SH_PPS * (SH_R / 16) >= SH_PIECES, "the pieces fit the k-loop");
  const unsigned pdy = (unsigned)p.ldy * rs * 2u, pxx = (unsigned)p.ldx * rs * 2u;      // byte pitches of the class-domain rows
  const int dyrow = 8 * wave + (lane >> 3), xrow = 4 * wave + (lane >> 4);              // + 64 i / + 32 i: the swizzle terms stay
  const unsigned voff_dy = (unsigned)dyrow * pdy + (unsigned)(((lane & 7) ^ swz_dy(dyrow)) << 4);
  const unsigned voff_x = (unsigned)xrow * pxx + (unsigned)(((lane & 15) ^ swz_x(xrow)) << 4);
  const unsigned voff_x6 = (128 + xrow < SH_R + NTAPS - 1) ? voff_x + 128u * pxx : 0x80000000u;   // rows no tap reads: out of range
  struct Src { __amdgpu_buffer_rsrc_t rdy, rxx; unsigned sdy, sx; };
  // The descriptors change with the (batch, class) item only -- a workgroup's run of tiles crosses few item borders -- so
  // the divisions and the scalar load of lens_in[b] are paid per item; per tile only the two scalar offsets move.
  auto item_source = [&](int item, Src& s) {
    const int b = item / rs, cls = item - b * rs;
    const int Tc = (p.Tout - cls + rs - 1) / rs;
    const int len_full = p.lens_in ? min(scalar_load_i32(p.lens_in + b), p.Tin) : p.Tin;
    const int len_in = max(0, (len_full - cls + rs - 1) / rs);
    s.rdy = ws_rsrc(p.dy, ((long long)b * p.dy_bs + (long long)cls * p.ldy + co0) * 2, (unsigned)Tc * pdy);
    s.rxx = ws_rsrc(p.x, ((long long)b * p.x_bs + (long long)cls * p.ldx + ci0) * 2, (unsigned)len_in * pxx);
  };
  auto tile_source = [&](int t0, Src& s) {
    s.sdy = (unsigned)t0 * pdy;
    s.sx = (unsigned)(t0 - p.pad) * pxx;
  };
  auto piece = [&](const Src& s, int i, int buf) {       // i is a compile-time constant wherever this is called
    unsigned char* base = smem + (size_t)buf * SH_STAGE;
    if (i < 2) ws_dma16(s.rdy, voff_dy + s.sdy + (unsigned)(64 * i) * pdy, base + (wave + 8 * i) * 1024);
    else if (i < 6) ws_dma16(s.rxx, voff_x + s.sx + (unsigned)(32 * (i - 2)) * pxx, base + SH_DY + (wave + 8 * (i - 2)) * 1024);
    else if (wave < 2) ws_dma16(s.rxx, voff_x6 + s.sx, base + SH_DY + (wave + 32) * 1024);
  };

  bf16x8 ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;

  // per-lane fragment offsets: the k-step advances rows by 16, which keeps both swizzle terms
  // (written out: through tr_lane_row / swz_col_bytes the compiler schedules this kernel differently)
  const int tg = lane >> 4, tq = (lane & 15) >> 2, tp = lane & 3, thh = tg >> 1;
  const int coly = wm * 32 + 16 * (tg & 1) + 4 * tp, colx = wn * 32 + 16 * (tg & 1) + 4 * tp;
  const int lrow = 8 * thh + tq;
  const int dyoff = lrow * DYB + (((coly >> 3) ^ (((lrow >> 1) & 1) << 2)) << 4) + (coly & 7) * 2;
  const int xoff = SH_DY + lrow * XB + (((colx >> 3) ^ ((lrow & 3) << 2)) << 4) + (colx & 7) * 2;
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  // The three fragments of k-step k0+1 are requested (asm, so that the request stays where it is written) before the
  // MFMAs of k-step k0; `s_waitcnt lgkmcnt(SH_NREAD)` then retires exactly the older six reads (LDS returns in order).  The
  // fragments are pinned by the wait so that nothing that uses them can be scheduled above it.
  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
  struct Frags { u32x2 a0, a1, p0, p1, q0, q1; };
  constexpr int SH_NREAD = 6;                      // ds_read instructions per request
  auto request = [&](Frags& f, unsigned base, int k0) {
    const unsigned pa = base + dyoff + k0 * 16 * DYB, px = base + xoff + k0 * 16 * XB;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(f.a0) : "v"(pa));
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(f.a1) : "v"(pa), "n"(4 * DYB));
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(f.p0) : "v"(px));
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(f.p1) : "v"(px), "n"(4 * XB));
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(f.q0) : "v"(px), "n"(8 * XB));
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(f.q1) : "v"(px), "n"(12 * XB));
  };

  WG_SUMS;
  // (item, first row) of the tile staged next, and its source
  const int item_rows = p.tiles_per_item * SH_R;
  int n_item = tile_begin / p.tiles_per_item, n_t0 = (tile_begin - n_item * p.tiles_per_item) * SH_R;
  Src sn;
  sn.rdy = sn.rxx = ws_rsrc(p.x, 0, 0);
  if (tile_begin < tile_end) {
    item_source(n_item, sn);
    tile_source(n_t0, sn);
#pragma unroll
    for (int i = 0; i < SH_PIECES; ++i) piece(sn, i, 0);
  }
  for (int tile = tile_begin; tile < tile_end; ++tile) {
    const int buf = (tile - tile_begin) & 1;
    WG_T(c0);
    vm_wait<0>();
    __syncthreads();                       // this tile has landed for every wave; the other buffer is free
    WG_T(c1);
    // The next tile's pieces go out behind the MFMAs of the k-loop (as one burst here, with both waves of a SIMD in lockstep
    // and the matrix pipe idle, the 6-7 pieces with their 64-bit addresses cost 2,100-2,200 cycles per tile:
    // profiles/dma_placement_phases.txt).  Descriptors, lens_in[b] and scalar offsets are ready before the k-loop, whose
    // lgkmcnt counts must see LDS reads only.  The last tile issues the same pieces through descriptors of zero records,
    // which the range check drops (zeros land in the idle buffer): one code path.
    const bool more = tile + 1 < tile_end;
    n_t0 += SH_R;
    if (n_t0 == item_rows) {
      n_t0 = 0; ++n_item;
      if (more) item_source(n_item, sn);
    }
    if (!more) sn.rdy = sn.rxx = ws_rsrc(p.x, 0, 0);
    tile_source(n_t0, sn);
    WG_T(c2);
    const unsigned base = lds0 + (unsigned)buf * SH_STAGE;
    Frags fr[2];
    request(fr[0], base, 0);
#pragma unroll
    for (int k0 = 0; k0 < SH_R / 16; ++k0) {
      Frags& f = fr[k0 & 1];
      if (k0 + 1 < SH_R / 16) {
        request(fr[(k0 + 1) & 1], base, k0 + 1);
        lgkm_wait<SH_NREAD>(f.a0, f.a1, f.p0, f.p1, f.q0, f.q1);
      } else {
        lgkm_wait<0>(f.a0, f.a1, f.p0, f.p1, f.q0, f.q1);
      }
      const u32x4 aw = {f.a0[0], f.a0[1], f.a1[0], f.a1[1]};
      const bf16x8 a = __builtin_bit_cast(bf16x8, aw);
      const unsigned w[8] = {f.p0[0], f.p0[1], f.p1[0], f.p1[1], f.q0[0], f.q0[1], f.q1[0], f.q1[1]};
#pragma unroll
      for (int s = 0; s < NTAPS; ++s) {
        const int m = s >> 1;
        u32x4 bw;
        if (s & 1) {
#pragma unroll
          for (int i = 0; i < 4; ++i) bw[i] = __builtin_amdgcn_alignbit(w[m + i + 1], w[m + i], 16);
        } else {
          bw = u32x4{w[m], w[m + 1], w[m + 2], w[m + 3]};
        }
        acc[s] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, bw), acc[s], 0, 0, 0);
        if (s < SH_PPS && SH_PPS * k0 + s < SH_PIECES) {   // fenced, so that the piece stays behind this MFMA
          __builtin_amdgcn_sched_barrier(0);
          piece(sn, SH_PPS * k0 + s, buf ^ 1);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      // bias gradient: the four waves of a row share the k-steps (each column block of the bias plane then holds a
      // PARTIAL sum; the reduce kernel adds columns 0, 32, 64, 96)
      if (bias_plane && (k0 & 3) == wn) acc[NTAPS] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, ones, acc[NTAPS], 0, 0, 0);
    }
    WG_T(c3);
    WG_ACC(0, c0, c1); WG_ACC(1, c1, c2); WG_ACC(2, c2, c3); WG_ACC(4, c0, c0 + 1);
  }
  vm_wait<0>();                            // the last tile's dropped pieces still write (zeros) to this workgroup's LDS
  WG_T(c4);
  float* out = p.slab + ((size_t)w.cgl * w.nblk + w.blk) * (size_t)PLANES * CB * CIB;
#pragma unroll
  for (int j = 0; j < PLANES; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
      out[((size_t)j * CB + row) * CIB + wn * 32 + r] = acc[j][e];
    }
  WG_T(c5);
  WG_ACC(3, c4, c5);
  WG_DUMP;
}

// plan of the shifted-fragment variant; false = not applicable
struct ShiftPlan { int rs, pad, tiles_per_item, tiles_per_wg, n_chunks, nblk_co, nblk_ci; };
static bool wgrad_shift_plan(const smt_conv_desc* d, ShiftPlan* pl) {
  static const bool off = getenv("SMT_WGRAD_NO_SHIFT") != nullptr;
  if (off || d->dtype != SMT_BF16 || d->stride != 1 || d->out_stride != 1 || d->out_offset != 0 || !d->zero_page ||
      d->c_in % 128 != 0 || d->c_out % 64 != 0 || d->taps < 3 || d->taps > 9 || !(d->taps & 1) || d->t_in != d->t_out)
    return false;
  int rs = 1, pad = d->padding;
  if (d->dilation > 1) {
    if (d->padding % d->dilation != 0 || d->t_out / d->dilation < class_min_rows()) return false;
    rs = d->dilation; pad = d->padding / d->dilation;
  }
  if (pad < 0 || pad > d->taps - 1) return false;
  const long long tc_max = (d->t_out + rs - 1) / rs;
  // 32-bit buffer offsets: an item's rows plus a tile beyond them stay below 2^31 bytes, so that rows before the item
  // (offsets that wrap) and the out-of-range marker of the kernel are beyond every descriptor's range
  const long long span = (tc_max + 2 * SH_R) * rs * 2;
  if (span * d->ld_x >= (1ll << 31) || span * d->ld_y >= (1ll << 31)) return false;
  const int tpi = (int)((tc_max + SH_R - 1) / SH_R);
  const long long ntiles = (long long)tpi * d->batch * rs;
  static const int min_tiles = getenv("SMT_SHIFT_MIN_TILES") ? atoi(getenv("SMT_SHIFT_MIN_TILES")) : 256;
  if (ntiles < min_tiles) return false;                 // small levels: the per-tap kernel wastes less
  const int nco = d->c_out / 64, nci = d->c_in / 128;
  // one workgroup per CU, but at least `min_tpw` tiles per workgroup: every workgroup leaves a (taps + 1) x 32 KiB slab
  // that the reduce kernel reads back, which at the small levels would rival the operand traffic
  static const int min_tpw = getenv("SMT_SHIFT_MIN_TPW") ? atoi(getenv("SMT_SHIFT_MIN_TPW")) : 2;   // measured: 66.9 -> 66.3 ms/step
  const long long chunks_target =
      std::max<long long>(8, std::min<long long>(256 / (nco * nci), ntiles / std::max(1, min_tpw)));
  const int tpw = (int)((ntiles + chunks_target - 1) / chunks_target);
  pl->rs = rs; pl->pad = pad; pl->tiles_per_item = tpi; pl->tiles_per_wg = tpw;
  pl->n_chunks = (int)((ntiles + tpw - 1) / tpw); pl->nblk_co = nco; pl->nblk_ci = nci;
  return true;
}

// ---- fixed-order reduction of the partial slabs -------------------------------------------------------------------
// One job = one weight (+ bias) gradient: slab[chunk][blk][plane][64 co][cib ci] -> dw (torch layout), db.  Jobs travel BY
// VALUE in the kernel arguments (no table upload, capturable in a hipGraph); up to WR_MAXJ jobs share one launch, so a
// GatedHiFi block's ten weight gradients cost one reduce launch instead of ten (smt_wgrad_reduce_defer / _flush).
struct WreduceJob {
  const float* slab; float* dw; float* db;
  long long so, si, sj;
  int n_chunks, nblk, nblk_ci, planes, taps, Cin, Cout, cib, bias_cols;
  int block0;                      // first workgroup of this job inside the launch
  int wblocks;                     // workgroups of the weight part (the bias part follows)
  signed char jmap[16];
};
constexpr int WR_MAXJ = 16;
struct WreduceBatch { int n_jobs, total_blocks; WreduceJob job[WR_MAXJ]; };

// Weight part: a workgroup owns 64 float4 outputs (256 consecutive ci of one (plane, co) row ... up to row ends) x 4 chunk
// slices: thread (o, s) sums chunks s, s+4, ... in index order (four independent 16-byte loads in flight; eight measured the same), the four slice
// sums are then added in slice order -- a fixed summation tree: bitwise reproducible.  (Round 3: a wave now reads ONE
// 1 KiB run of one slab per load instruction; the first layout -- 32 outputs x 8 slices, two 512-byte runs of two slabs per
// instruction -- read the slabs at 2.5-3 TB/s.)  Bias part: one thread per output channel and slice (32 x 8), columns 0, 32, ..
__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(WreduceBatch bt) {
  __shared__ f32x4 part[4][64];
  int j = 0;
#pragma unroll 1
  for (int k = 1; k < bt.n_jobs; ++k)
    if ((int)blockIdx.x >= bt.job[k].block0) j = k;
  const WreduceJob& p = bt.job[j];
  const int lb = blockIdx.x - p.block0;
  const size_t blk_elems = (size_t)p.planes * 64 * p.cib;
  const size_t cstride = (size_t)p.nblk * blk_elems;
  if (lb < p.wblocks) {
    const int o = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int cin4 = p.Cin >> 2;
    const long long total4 = (long long)p.taps * p.Cout * cin4;
    const long long e4 = (long long)lb * 64 + o;
    const bool live = e4 < total4;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    int ci = 0, co = 0, plane = 0;
    if (live) {
      ci = (int)(e4 % cin4) * 4; co = (int)((e4 / cin4) % p.Cout); plane = (int)(e4 / ((long long)cin4 * p.Cout));
      const int blk = (co / 64) * p.nblk_ci + (ci / p.cib);
      const float* src = p.slab + (size_t)blk * blk_elems + ((size_t)plane * 64 + (co % 64)) * p.cib + (ci % p.cib);
      int c = sl;
      for (; c + 12 < p.n_chunks; c += 16) {
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(src + (size_t)c * cstride);
        const f32x4 v1 = *reinterpret_cast<const f32x4*>(src + (size_t)(c + 4) * cstride);
        const f32x4 v2 = *reinterpret_cast<const f32x4*>(src + (size_t)(c + 8) * cstride);
        const f32x4 v3 = *reinterpret_cast<const f32x4*>(src + (size_t)(c + 12) * cstride);
        s += v0; s += v1; s += v2; s += v3;
      }
      for (; c < p.n_chunks; c += 4) s += *reinterpret_cast<const f32x4*>(src + (size_t)c * cstride);
    }
    part[sl][o] = s;
    __syncthreads();
    if (sl == 0 && live) {
      f32x4 t = part[0][o];
#pragma unroll
      for (int k = 1; k < 4; ++k) t += part[k][o];
      float* dst = p.dw + co * p.so + ci * p.si + p.jmap[plane] * p.sj;
      dst[0] = t[0]; dst[p.si] = t[1]; dst[2 * p.si] = t[2]; dst[3 * p.si] = t[3];
    }
  } else {
    float* part1 = reinterpret_cast<float*>(&part[0][0]);      // [8][32]
    const int o = threadIdx.x & 31, sl = threadIdx.x >> 5;
    const int co = (lb - p.wblocks) * 32 + o;
    const bool live = co < p.Cout && p.db != nullptr;
    float s = 0.f;
    if (live) {
      // bias plane: column 0 of every ci block holds db[co] (or partial sums in columns 0, 32, .. of the first block)
      const int blk = (co / 64) * p.nblk_ci;
      const float* src = p.slab + (size_t)blk * blk_elems + ((size_t)p.taps * 64 + (co % 64)) * p.cib;
      for (int c = sl; c < p.n_chunks; c += 8) {
        const float* q = src + (size_t)c * cstride;
        float part_sum = q[0];
        for (int k = 1; k < p.bias_cols; ++k) part_sum += q[32 * k];
        s += part_sum;
      }
    }
    part1[sl * 32 + o] = s;
    __syncthreads();
    if (sl == 0 && live) {
      float t = part1[o];
#pragma unroll
      for (int k = 1; k < 8; ++k) t += part1[k * 32 + o];
      p.db[co] = t;
    }
  }
}

static thread_local bool g_reduce_defer = false;
static thread_local WreduceBatch g_reduce_batch = {0, 0, {}};

static int reduce_flush(hipStream_t stream) {
  if (g_reduce_batch.n_jobs > 0 && g_reduce_batch.total_blocks > 0) {
    conv_wgrad_reduce_kernel<<<(unsigned)g_reduce_batch.total_blocks, 256, 0, stream>>>(g_reduce_batch);
    g_reduce_batch.n_jobs = 0; g_reduce_batch.total_blocks = 0;
    SMT_CHECK_LAUNCH("conv_wgrad_reduce");
  }
  g_reduce_batch.n_jobs = 0; g_reduce_batch.total_blocks = 0;
  return 0;
}

int launch_wgrad_reduce(const float* slab, float* dw, float* db, int n_chunks, int nblk_co, int nblk_ci, int taps,
                        int c_in, int c_out, int cib, long long so, long long si, long long sj, const int* jmap,
                        hipStream_t stream, int bias_cols) {
  SMT_CHECK_ARG(c_in % 4 == 0 && cib % 4 == 0 && taps <= 16, "conv_wgrad_reduce: c_in and the ci block must be multiples of 4");
  if (g_reduce_batch.n_jobs == WR_MAXJ) {
    int rc = reduce_flush(stream);
    if (rc) return rc;
  }
  WreduceJob& r = g_reduce_batch.job[g_reduce_batch.n_jobs];
  r.bias_cols = bias_cols;
  r.slab = slab; r.dw = dw; r.db = db;
  r.n_chunks = n_chunks; r.nblk = nblk_co * nblk_ci; r.nblk_ci = nblk_ci; r.planes = taps + 1; r.taps = taps;
  r.Cin = c_in; r.Cout = c_out; r.cib = cib;
  r.so = so; r.si = si; r.sj = sj;
  for (int t = 0; t < 16; ++t) r.jmap[t] = (signed char)(t < taps ? jmap[t] : 0);
  const long long total4 = (long long)taps * c_out * (c_in / 4);
  r.wblocks = (int)((total4 + 63) / 64);
  r.block0 = g_reduce_batch.total_blocks;
  g_reduce_batch.total_blocks += r.wblocks + (db ? (c_out + 31) / 32 : 0);
  g_reduce_batch.n_jobs += 1;
  return g_reduce_defer ? 0 : reduce_flush(stream);
}

}  // namespace smt

using namespace smt;

#if SMT_WGRAD_STAMP
extern "C" int smt_wgrad_debug_dump(unsigned long long* host, int n, int reset) {
  int rc = (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(wg_dbg), sizeof(unsigned long long) * n);
  if (reset) { static unsigned long long z[256 * 8 * 8]; rc |= (int)hipMemcpyToSymbol(HIP_SYMBOL(wg_dbg), z, sizeof(z)); }
  return rc;
}
#endif

extern "C" int smt_wgrad_reduce_defer(int on, smt_stream_t stream_) {
  // on = 1: the weight-gradient calls that follow on this thread (smt_conv1d_wgrad, smt_conv1x1_bwd, smt_conv_k1_bwd,
  // smt_conv_gate_bwd) queue their slab reductions instead of launching them; every call must then be given a workspace
  // of its own, which has to stay untouched until the flush.  on = 0: launch what is queued (one launch per 16 jobs).
  g_reduce_defer = on != 0;
  return on ? 0 : reduce_flush((hipStream_t)stream_);
}

// ---- the plan: which kernel runs for a descriptor, with what launch geometry, over how much workspace -----------------
// smt_conv1d_wgrad launches what the plan says, smt_conv1d_wgrad_kernel_name and _workspace_bytes report it.
//
// Shift: all taps in one launch (conv_wgrad_shift_kernel).  Otherwise tap groups: more than 5 taps would need more
// accumulator registers than two waves per SIMD allow, so wide kernels are processed as consecutive groups of <= 5 taps (a
// group of taps j0.. is the same convolution with padding reduced by j0*dilation), each on the LDS-DMA or the generic kernel.
constexpr int WG_GROUP = 5, WG_MAX_TAPS = 16, WG_MAX_GROUPS = (WG_MAX_TAPS + WG_GROUP - 1) / WG_GROUP;
constexpr size_t WG_MAX_LDS = 160 * 1024;
enum WgradVariant { WG_GENERIC, WG_DMA, WG_SHIFT };
static const char* const kWgradName[] = {"conv_wgrad", "conv_wgrad_dma", "conv_wgrad_shift"};

struct WgradLaunch {
  WgradVariant variant;
  int j0, taps, pad;                     // tap group (shift: all taps) and its left padding
  int cib;                               // input channels per workgroup = slab block width
  int rows_per_chunk, chunks_per_batch;  // generic / LDS-DMA chunking (shift: see ShiftPlan)
  int n_chunks, nblk_co, nblk_ci;        // partial slabs and their (co, ci) blocks
  unsigned grid; size_t lds;
  size_t ws_off, ws_bytes;               // this launch's region of the workspace (256-byte aligned)
};
struct WgradPlan {
  int n; WgradLaunch l[WG_MAX_GROUPS];   // launches in order; the first one names the conv
  ShiftPlan sh;                          // valid when l[0].variant == WG_SHIFT
  size_t ws_bytes;
};

static unsigned wgrad_grid(const WgradLaunch& l) { return (unsigned)(8 * ((l.n_chunks + 7) / 8) * l.nblk_co * l.nblk_ci); }
static size_t wgrad_slab_bytes(const WgradLaunch& l) {
  return (size_t)l.n_chunks * l.nblk_co * l.nblk_ci * (l.taps + 1) * 64 * l.cib * sizeof(float);
}

// one tap group on the LDS-DMA or the generic kernel
static WgradLaunch wgrad_group_plan(const smt_conv_desc* d, int j0, int taps) {
  WgradLaunch l = {};
  const bool bf = d->dtype == SMT_BF16;
  l.j0 = j0; l.taps = taps; l.pad = d->padding - j0 * d->dilation;
  // input channels per workgroup: 128 (8 waves, two per SIMD) while the accumulator planes fit in the 256-register
  // budget of that occupancy, else 64 (4 waves, one per SIMD, 512 registers)
  l.cib = (bf && d->c_in > 64 && d->stride == 1) ? 128 : 64;
  l.nblk_co = (d->c_out + 63) / 64;
  l.nblk_ci = (d->c_in + l.cib - 1) / l.cib;
  const int R = bf ? 128 : 64;
  const long long target_wgs = 512;   // two rounds of one workgroup per CU: keeps the partial slabs small
  long long rows = ((long long)d->batch * d->t_out * l.nblk_co * l.nblk_ci + target_wgs - 1) / target_wgs;
  rows = std::min<long long>((rows + R - 1) / R * R, ((long long)d->t_out + R - 1) / R * R);
  rows = std::max<long long>(R, rows);
  l.rows_per_chunk = (int)rows;
  l.chunks_per_batch = (int)((d->t_out + rows - 1) / rows);
  l.n_chunks = d->batch * l.chunks_per_batch;
  l.grid = wgrad_grid(l);
  // (dilation classes, as in conv_gemm_dma_kernel, were measured slower for these kernels: 2.04 vs 1.79 ms at k = 9, dilation 27)
  const int rows_x = (R - 1) * d->stride + (taps - 1) * d->dilation + 1;
  const size_t lds_dma = 2 * ((size_t)128 * 128 + (size_t)((rows_x + 3) & ~3) * 256);
  const bool dma = bf && l.cib == 128 && d->zero_page && d->c_in % 128 == 0 && d->c_out % 64 == 0 && d->out_stride == 1 &&
                   d->out_offset == 0 && lds_dma <= WG_MAX_LDS;
  l.variant = dma ? WG_DMA : WG_GENERIC;
  l.lds = dma ? lds_dma
        : bf  ? ((size_t)R * WTr<__bf16>::pitch(64) + (size_t)rows_x * WTr<__bf16>::pitch(l.cib)) * 2
              : ((size_t)R * WTr<float>::pitch(64) + (size_t)rows_x * WTr<float>::pitch(l.cib)) * 4;
  l.ws_bytes = align_up(wgrad_slab_bytes(l), 256);
  return l;
}

static bool wgrad_plan(const smt_conv_desc* d, WgradPlan* pl) {
  if (!d || d->taps < 1 || d->taps > WG_MAX_TAPS) return false;
  size_t groups_ws = 0;
  pl->n = 0;
  for (int j0 = 0; j0 < d->taps; j0 += WG_GROUP) {
    WgradLaunch& l = pl->l[pl->n++];
    l = wgrad_group_plan(d, j0, std::min(WG_GROUP, d->taps - j0));
    l.ws_off = groups_ws;            // consecutive regions: the groups' reductions may be deferred (smt_wgrad_reduce_defer)
    groups_ws += l.ws_bytes;
  }
  pl->ws_bytes = groups_ws;
  if (wgrad_shift_plan(d, &pl->sh)) {
    WgradLaunch l = {};
    l.variant = WG_SHIFT; l.taps = d->taps; l.pad = pl->sh.pad; l.cib = 128;
    l.n_chunks = pl->sh.n_chunks; l.nblk_co = pl->sh.nblk_co; l.nblk_ci = pl->sh.nblk_ci;
    l.grid = wgrad_grid(l); l.lds = 2 * SH_STAGE;
    l.ws_bytes = wgrad_slab_bytes(l);
    pl->n = 1; pl->l[0] = l;
    pl->ws_bytes = std::max(l.ws_bytes, groups_ws);   // callers size their workspace for either choice
  }
  return true;
}

extern "C" size_t smt_conv1d_wgrad_workspace_bytes(const smt_conv_desc* d) {
  WgradPlan pl;
  return wgrad_plan(d, &pl) ? pl.ws_bytes : 0;
}

extern "C" const char* smt_conv1d_wgrad_kernel_name(const smt_conv_desc* d) {
  WgradPlan pl;
  return wgrad_plan(d, &pl) ? kWgradName[pl.l[0].variant] : "";
}

// every kernel here takes its tiles in dynamic LDS beyond the 64 KiB default
template <typename... P, typename... A>
static void launch_lds(void (*kernel)(P...), unsigned grid, unsigned threads, size_t lds, hipStream_t stream, A... args) {
  (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)WG_MAX_LDS);
  kernel<<<dim3(grid), dim3(threads), lds, stream>>>(args...);
}

typedef void (*WgradKernel)(WgradArgs);
static_assert(WG_GROUP == 5, "the kernels are instantiated for 2 .. 6 accumulator planes (1 .. 5 taps + bias)");
#define SMT_WG_BY_PLANES(planes, K) \
  ((planes) == 2 ? K(2) : (planes) == 3 ? K(3) : (planes) == 4 ? K(4) : (planes) == 5 ? K(5) : K(6))
template <typename T, int CIB, bool STRIDED> static WgradKernel generic_kernel(int planes) {
#define SMT_WG_K(NT) (WgradKernel)conv_wgrad_kernel<T, NT, CIB, STRIDED>
  return SMT_WG_BY_PLANES(planes, SMT_WG_K);
#undef SMT_WG_K
}
static WgradKernel dma_kernel(int planes) {
#define SMT_WG_K(NT) (WgradKernel)conv_wgrad_dma_kernel<NT>
  return SMT_WG_BY_PLANES(planes, SMT_WG_K);
#undef SMT_WG_K
}

extern "C" int smt_conv1d_wgrad(const smt_conv_desc* d, float* dweight, int64_t stride_out, int64_t stride_in,
                                int64_t stride_tap, const int* tap_map, float* dbias, void* workspace,
                                size_t workspace_bytes, smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SMT_CHECK_ARG(d && tap_map, "smt_conv1d_wgrad: null pointer");
  SMT_CHECK_ARG(d->taps >= 1 && d->taps <= WG_MAX_TAPS, "smt_conv1d_wgrad: taps must be in [1, 16]");
  SMT_CHECK_ARG(d->x && d->y && dweight && workspace, "smt_conv1d_wgrad: null pointer");
  SMT_CHECK_ARG(d->dtype == SMT_BF16 || d->dtype == SMT_F32, "smt_conv1d_wgrad: bad dtype");
  const bool bf = d->dtype == SMT_BF16;
  const int epv = bf ? 8 : 4;
  SMT_CHECK_ARG(d->c_in % epv == 0 && d->c_out % epv == 0 && d->ld_x % epv == 0 && d->ld_y % epv == 0,
                "smt_conv1d_wgrad: channels / pitches must keep 16-byte alignment");
  WgradPlan pl;
  wgrad_plan(d, &pl);
  SMT_CHECK_ARG(workspace_bytes >= pl.ws_bytes, "smt_conv1d_wgrad: workspace too small");
  const bool empty = d->batch <= 0 || d->t_out <= 0;
  for (int i = 0; i < pl.n; ++i) {
    const WgradLaunch& l = pl.l[i];
    float* slab = reinterpret_cast<float*>((char*)workspace + l.ws_off);
    float* db = i == 0 ? dbias : nullptr;
    if (l.variant == WG_SHIFT) {      // fragments shifted in registers
      ShiftArgs a;
      a.x = d->x; a.dy = d->y; a.slab = slab; a.lens_in = d->lens_in;
      a.x_bs = d->bs_x; a.dy_bs = d->bs_y; a.ldx = d->ld_x; a.ldy = d->ld_y;
      a.B = d->batch; a.Tin = d->t_in; a.Tout = d->t_out; a.pad = l.pad; a.rs = pl.sh.rs;
      a.tiles_per_item = pl.sh.tiles_per_item; a.tiles_per_wg = pl.sh.tiles_per_wg; a.n_chunks = l.n_chunks;
      a.nblk_ci = l.nblk_ci; a.nblk_co = l.nblk_co; a.with_bias = db ? 1 : 0;
      const __bf16* zp = (const __bf16*)d->zero_page;
      switch (d->taps) {
        case 3: launch_lds(conv_wgrad_shift_kernel<3>, l.grid, 512, l.lds, stream, a, zp); break;
        case 5: launch_lds(conv_wgrad_shift_kernel<5>, l.grid, 512, l.lds, stream, a, zp); break;
        case 7: launch_lds(conv_wgrad_shift_kernel<7>, l.grid, 512, l.lds, stream, a, zp); break;
        default: launch_lds(conv_wgrad_shift_kernel<9>, l.grid, 512, l.lds, stream, a, zp); break;
      }
      SMT_CHECK_LAUNCH(kWgradName[l.variant]);
    } else if (!empty) {
      SMT_CHECK_ARG(l.lds <= WG_MAX_LDS, "conv_wgrad: tile needs %zu B of LDS", l.lds);
      WgradArgs a;
      a.x = d->x; a.dy = d->y; a.slab = slab; a.lens_in = d->lens_in;
      a.x_bs = d->bs_x; a.dy_bs = d->bs_y; a.ldx = d->ld_x; a.ldy = d->ld_y;
      a.B = d->batch; a.Tin = d->t_in; a.Tout = d->t_out; a.Ty = d->t_y; a.Cin = d->c_in; a.Cout = d->c_out;
      a.taps = l.taps; a.stride = d->stride; a.dil = d->dilation; a.pad = l.pad;
      a.out_stride = d->out_stride; a.out_offset = d->out_offset;
      a.rows_per_chunk = l.rows_per_chunk; a.chunks_per_batch = l.chunks_per_batch;
      a.nblk_ci = l.nblk_ci; a.nblk_co = l.nblk_co; a.with_bias = db ? 1 : 0;
      const bool strided = d->stride > 1;
      const int planes = l.taps + 1;
      const WgradKernel k = l.variant == WG_DMA ? dma_kernel(planes)
                          : bf && l.cib == 128  ? generic_kernel<__bf16, 128, false>(planes)
                          : bf ? (strided ? generic_kernel<__bf16, 64, true>(planes) : generic_kernel<__bf16, 64, false>(planes))
                               : (strided ? generic_kernel<float, 64, true>(planes) : generic_kernel<float, 64, false>(planes));
      launch_lds(k, l.grid, l.variant == WG_DMA ? 512 : l.cib * 4, l.lds, stream, a);
      SMT_CHECK_LAUNCH(kWgradName[l.variant]);
    }
    const int bias_cols = l.variant == WG_SHIFT ? 4 : 1;   // the shift kernel leaves four partial bias columns
    int rc = launch_wgrad_reduce(slab, dweight, db, empty ? 0 : l.n_chunks, l.nblk_co, l.nblk_ci, l.taps, d->c_in, d->c_out,
                                 l.cib, stride_out, stride_in, stride_tap, tap_map + l.j0, stream, bias_cols);
    if (rc) return rc;
  }
  return 0;
}
