// Pieces shared by the convolution kernels: element traits, 16-byte vectors, counter-based dropout.
#pragma once
#include <algorithm>
#include <cstdlib>

#include "smt_common.h"

namespace smt {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

// ---- counter-based dropout (spec: include/smt_hip.h "dropout") -------------------------------
__device__ __forceinline__ unsigned fmix32(unsigned h) {
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}
// keep-bit of linear element index i: 16 random bits per element, two elements per hash
__device__ __forceinline__ bool drop_keep(unsigned long long i, unsigned key, unsigned thresh16) {
  unsigned h = fmix32((unsigned)(i >> 1) * 0x9E3779B1u + key);
  unsigned bits = (h >> (16 * (unsigned)(i & 1))) & 0xFFFFu;
  return bits >= thresh16;
}

template <typename T> struct Tr;
template <> struct Tr<__bf16> {
  static constexpr int EPV = 8;      // elements per 16-byte vector
  static constexpr int CCH = 128;    // input channels staged per LDS A chunk
  static constexpr int KC = 128;     // K per weight chunk (one barrier per tap for 128 input channels)
  static constexpr int BM = 128;
};
template <> struct Tr<float> {
  static constexpr int EPV = 4;
  static constexpr int CCH = 64;
  static constexpr int KC = 64;
  static constexpr int BM = 64;
};

template <typename T, int EPV> struct Vec { T v[EPV]; } __attribute__((aligned(16)));

__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  bf16x2 v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(unsigned, v);
}

typedef short s16x2v __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2v __attribute__((ext_vector_type(2)));
// relu on a packed bf16 pair: a negative bf16 is a negative int16 (v_pk_max_i16)
__device__ __forceinline__ unsigned pk_relu_bf16(unsigned w) {
  return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2v, w), s16x2v{0, 0}));
}
// 0xFFFF per 16-bit half of h that is >= thr (thr_m1 = thr - 1 in both halves, thr >= 1): saturating subtract, min 1, negate
__device__ __forceinline__ unsigned pk_keep_mask(unsigned h, unsigned thr_m1) {
  u16x2v d = __builtin_elementwise_sub_sat(__builtin_bit_cast(u16x2v, h), __builtin_bit_cast(u16x2v, thr_m1));
  d = __builtin_elementwise_min(d, u16x2v{1, 1});
  return __builtin_bit_cast(unsigned, (u16x2v)(u16x2v{0, 0} - d));
}

// tanh for the gate (resnet.py:233): 1 - 2 / (exp(2x) + 1) on the hardware exp2 / rcp -- 5 instructions instead of the
// ~40 of tanhf; absolute error <= 2e-7 (the gate's output is O(1) and is stored in bf16 on the fast path), exact limits
// +-1 at +-inf.  Every gate kernel (forward, fused forward, backward) uses this one function, so they stay consistent.
__device__ __forceinline__ float gate_tanh(float x) {
  const float e = __builtin_amdgcn_exp2f(x * 2.885390081777927f);        // exp(2x) = 2^(2x log2 e)
  return 1.f - 2.f * __builtin_amdgcn_rcpf(e + 1.f);
}

// LDS-DMA: one wave-instruction copies 64 x 16 B (per-lane global source) to 1 KiB of LDS at a wave-uniform base
__device__ __forceinline__ void lds_dma16(const void* gsrc, void* lds_dst_wave_base) {
  __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)gsrc,
                                   (void __attribute__((address_space(3)))*)lds_dst_wave_base, 16, 0, 0);
}

// Buffer addressing for the streaming kernels: a range-checked V# over `bytes` bytes from base + byte_off -- per-lane
// offsets are 32-bit, loads beyond the range return zero and stores beyond it are dropped (no per-lane bounds selects, no
// zero page), and every such instruction IS issued, so `s_waitcnt vmcnt(N)` counts stay compile-time constants.
typedef int i32x4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t ws_rsrc(const void* base, long long byte_off, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(base)) + byte_off, 0, (int)bytes, 0x00020000);
}
// LDS-DMA through a V#: 64 x 16 B (per-lane byte offset) to 1 KiB of LDS at a wave-uniform base
__device__ __forceinline__ void ws_dma16(__amdgpu_buffer_rsrc_t rs, unsigned voff, void* lds_wave_base) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds_wave_base, 16, (int)voff, 0, 0, 0);
}
// Persistent workgroups: every workgroup takes a contiguous run of tiles_per_wg tiles, and the runs of workgroups b, b + 8, ..
// (one XCD, one L2) are adjacent -- neighbouring tiles share their halo rows and the weights in L2.  False: no tile left.
__device__ __forceinline__ bool wg_tile_run(int ntiles, int tiles_per_wg, int& wg, int& tile_begin, int& tile_end) {
  const int nwg = gridDim.x;
  wg = (blockIdx.x & 7) * (nwg >> 3) + (blockIdx.x >> 3);
  tile_begin = wg * tiles_per_wg;
  tile_end = min(ntiles, tile_begin + tiles_per_wg);
  return tile_begin < tile_end;
}

// Output of a TRANSPOSED 32 x 32 MFMA tile (A = weights, B = rows), packed to bf16 pairs v[2g + h] = channels 8g + 4hh + 2h, +1:
// lanes r and r + 32 hold channels {0-3, 8-11, 16-19, 24-27} and {4-7, 12-15, 20-23, 28-31} of the same row: swap so that
// lane r owns 0-7 | 16-23 and lane r + 32 owns 8-15 | 24-31 (16-byte pieces) ...
__device__ __forceinline__ void pair_up8(unsigned (&v)[8]) {
#pragma unroll
  for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      auto sw = __builtin_amdgcn_permlane32_swap(v[4 * h2 + d], v[4 * h2 + 2 + d], false, false);
      v[4 * h2 + d] = sw[0]; v[4 * h2 + 2 + d] = sw[1];
    }
}
// ... and store them straight from registers: vo = byte offset of this lane's first piece (row, channel 8 hh of the tile)
__device__ __forceinline__ void store_paired(const unsigned (&v)[8], __amdgpu_buffer_rsrc_t rs, unsigned vo) {
  __builtin_amdgcn_raw_buffer_store_b128(i32x4v{(int)v[0], (int)v[1], (int)v[2], (int)v[3]}, rs, (int)vo, 0, 0);
  __builtin_amdgcn_raw_buffer_store_b128(i32x4v{(int)v[4], (int)v[5], (int)v[6], (int)v[7]}, rs, (int)(vo + 32u), 0, 0);
}

// The same instruction as inline asm, for loops that own their vmcnt waits: the compiler tracks LDS-DMA builtins and puts a
// wait for every DMA in flight in front of the first LDS intrinsic it cannot disambiguate (ds_read_b64_tr_b16: measured in
// conv1x1_bwd, a vmcnt wait for the NEXT tile's prefetch in the middle of the current tile) and answers the first use of
// any ordinary load with vmcnt(0).  Untracked, nothing is inserted; the caller's counted waits are the only ones.
struct UntrackedRsrc { i32x4v w; };
__device__ __forceinline__ UntrackedRsrc untracked_rsrc(const void* base, long long byte_off, unsigned bytes) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(base) + (unsigned long long)byte_off;
  UntrackedRsrc r;
  r.w = i32x4v{__builtin_amdgcn_readfirstlane((int)(unsigned)a), __builtin_amdgcn_readfirstlane((int)((a >> 32) & 0xffffu)),
               __builtin_amdgcn_readfirstlane((int)bytes), 0x00020000};
  return r;
}
__device__ __forceinline__ void untracked_dma16(const UntrackedRsrc& rs, unsigned voff, const void* lds_wave_base) {
  const unsigned m0v = __builtin_amdgcn_readfirstlane(
      (int)(unsigned)reinterpret_cast<size_t>((__attribute__((address_space(3))) const void*)lds_wave_base));
  // Hazards the compiler pads for its own instructions but not inside inline asm: an SALU write of M0 needs one wait state
  // before an LDS-DMA reads it, and an SGPR written by the VALU (v_readfirstlane: the descriptor words, the LDS address) needs
  // five before a vector-memory instruction reads it.  s_nop 4 after the M0 write covers both.
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 4\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds" : : "v"(voff), "s"(rs.w), "s"(m0v) : "memory");
}

// A 16-byte global load the COMPILER DOES NOT TRACK (scalar base + 32-bit lane offset).  While LDS-DMA is in flight hipcc
// answers the first use of any ordinary load result with s_waitcnt vmcnt(0), which also drains the DMA of the NEXT tile and
// serialises a double-buffered stream (measured in round 3 on conv_k3gate: every step waited for its own prefetch).  The
// caller owns the wait: s_waitcnt vmcnt(N) with N = the vector-memory instructions issued after this one.
__device__ __forceinline__ i32x4v untracked_load16(const void* sbase, unsigned voff) {
  i32x4v v;
  asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %1, %2" : "=v"(v) : "v"(voff), "s"(sbase) : "memory");   // s_nop: see untracked_dma16
  return v;
}

typedef unsigned u32x2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u32x2v untracked_load8(const void* sbase, unsigned voff) {
  u32x2v v;
  asm volatile("s_nop 4\n\tglobal_load_dwordx2 %0, %1, %2" : "=v"(v) : "v"(voff), "s"(sbase) : "memory");
  return v;
}

// ---- counted waits: the one spelling of "wait, then these registers hold their data" ---------------------------------
// The untracked loads above are invisible to hipcc's wait bookkeeping, so the kernels that use them wait themselves:
// vm_wait<N> is `s_waitcnt vmcnt(N)`, N = the vector-memory instructions this wave issued after the newest one that must
// have completed.  An asm load's destination counts as written when its statement ends, so every register an untracked load
// filled must be listed here: each is pinned ("+v") right after the wait, and no instruction that reads, copies or spills it
// can be scheduled above the wait.  lgkm_wait<N> is the same for the LDS / scalar-memory counter.  untracked_dma16 writes
// M0, which cannot be declared as a clobber (reserved: an "m0" clobber only draws a warning), so it writes M0 in the same
// statement that reads it; do not mix it with the ws_dma16 builtin in one kernel.
template <typename T> __device__ __forceinline__ void pin_v(T& x) { asm volatile("" : "+v"(x)); }
template <typename T, int N> __device__ __forceinline__ void pin_v(T (&a)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) pin_v(a[i]);
}
template <int N, typename... R> __device__ __forceinline__ void vm_wait(R&... regs) {
  static_assert(0 <= N && N <= 63, "vmcnt is a 6-bit field on gfx9");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
  (pin_v(regs), ...);
}
template <int N, typename... R> __device__ __forceinline__ void lgkm_wait(R&... regs) {
  static_assert(0 <= N && N <= 15, "lgkmcnt is a 4-bit field on gfx9");
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
  (pin_v(regs), ...);
}
// Where the younger instructions are issued only on some paths (the last tile has no prefetch): vmcnt(N) if `counted`,
// else vmcnt(0); the registers are pinned after either.
template <int N, typename... R> __device__ __forceinline__ void vm_wait_or_drain(bool counted, R&... regs) {
  if (counted) vm_wait<N>();
  else vm_wait<0>();
  (pin_v(regs), ...);
}
// End of a tile or step: nothing the compiler placed above may sink below the wait (and vice versa), then the wait.
template <int N, typename... R> __device__ __forceinline__ void step_end_wait(R&... regs) {
  __builtin_amdgcn_sched_barrier(0);
  vm_wait<N>(regs...);
}

// lens[b] as a SCALAR load (the compiler picks a vector load for a pointer the kernel may also write through, tracks it,
// and waits vmcnt(0) for it -- draining the LDS-DMA in flight); the address must be wave-uniform.
__device__ __forceinline__ int scalar_load_i32(const int* ptr) {
  int v;
  asm volatile("s_nop 4\n\ts_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(ptr) : "memory");   // s_nop: the address may
                                                        // come from v_readfirstlane (VALU-written SGPR read by a memory instruction)
  return v;
}

// ---- arguments of the smt_conv1d_ntc kernels (conv.hip, conv_ws.hip) ---------------------------------------------------
struct ConvArgs {
  const void* x; const void* w; const float* bias; void* y; const void* res; const void* gate_h; void* y_act;
  const int* lens_in; const int* lens_out;
  long long x_bs, y_bs, res_bs, gh_bs, ya_bs;  // batch strides (elements)
  int ldx, ldy, ldr, ldgh, ldya;               // row pitches (elements)
  int B, Tin, Tout, Cin, Cout;          // Tout = output rows PER LAUNCH INDEX t (before os/oo)
  int taps, stride, dil, pad;
  int out_stride, out_offset, Ty;       // output row = t*out_stride + out_offset, Ty rows in y per batch
  int act_out, epi_act;                 // relu+dropout of the OUTPUT (second store) / its derivative as epilogue
  unsigned drop_keys[8]; int site_width; unsigned drop_thresh16; float drop_scale;
  const unsigned* drop_keys_dev; int drop_keys_dev_stride;   // keys in device memory (graph replay): override drop_keys
  int tiles_per_batch;
  int rs;   // row stride of the dilation-class decomposition (LDS-DMA kernel), 1 = off
  const void* x2; const void* w2; const float* bias2; const int* lens_in2; long long x2_bs; int ldx2;   // folded second 1x1 term (conv1x1_fold)
  int dbg;  // ablation switches (SMT_CONV_DBG): 1 no A loads, 2 no W loads, 4 no MFMA, 8 no stores
};

// dropout key of site s of this launch: by value, or from device memory when the caller keeps its keys there
__device__ __forceinline__ unsigned site_key(const ConvArgs& p, int site) {
  return p.drop_keys_dev ? p.drop_keys_dev[(site & 7) * p.drop_keys_dev_stride] : p.drop_keys[site & 7];
}

// ---- the weight-stationary family (conv_ws.hip) as conv.hip's dispatch sees it -----------------------------------------
struct WsPlan { int buf_bytes; size_t lds; int tiles_per_wg; dim3 grid; };
// Plan the weight-stationary launch of p (dilation classes already applied: p.rs, p.dil, p.pad), or say that p is not
// eligible.  On success p.tiles_per_batch is set.
bool plan_conv_ws(ConvArgs& p, WsPlan& pl);
void launch_conv_ws(const ConvArgs& p, const WsPlan& pl, const void* zero_page, hipStream_t stream);
// the name smt_conv1d_kernel_name reports for the variant that launch_conv_ws picks for p
const char* conv_ws_variant_name(const ConvArgs& p);

// Tiles a persistent workgroup of the fused backward kernels takes at least (SMT_FUSED_MIN_TPW): every workgroup leaves a
// partial weight-gradient slab that the reduce kernel reads back, so at the small levels of the model fewer, longer
// workgroups cost less than the slabs of 256 short ones.
inline int fused_min_tpw() {
  static const int v = [] { const char* e = getenv("SMT_FUSED_MIN_TPW"); return e ? std::max(1, atoi(e)) : 2; }();
  return v;
}

// Rows a dilation class must have for the class decomposition to pay (SMT_CLASS_MIN_ROWS): tile quantisation wastes
// ceil(Tc/128)*128 - Tc rows per class.  Read by the forward / data-gradient plan (conv.hip) and the shift weight gradient.
inline int class_min_rows() {
  static const int v = [] { const char* e = getenv("SMT_CLASS_MIN_ROWS"); return e ? atoi(e) : 128; }();
  return v;
}

// Fixed-order reduction of weight-gradient partial slabs (conv_wgrad.hip): slab[chunk][blk = co/64 * nblk_ci + ci/cib]
// [plane = tap | bias][64 co][cib ci] -> dw[co*so + ci*si + jmap[tap]*sj], db[co] (column 0 of the bias plane).
int launch_wgrad_reduce(const float* slab, float* dw, float* db, int n_chunks, int nblk_co, int nblk_ci, int taps,
                        int c_in, int c_out, int cib, long long so, long long si, long long sj, const int* jmap,
                        hipStream_t stream, int bias_cols = 1);   // bias_cols > 1: db = sum of columns 0, 32, .. of the bias plane

}  // namespace smt
