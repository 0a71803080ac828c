// The vocabulary of the persistent, double-buffered "streaming" convolution kernels: conv1x1_fold / conv_k1act / conv1x1_c64 /
// conv1x1_dma (conv.hip), conv_k3gate, conv1x1_bwd, conv_k1_bwd, conv_gate_bwd, convt4s2 / conv4s2 (conv_resample.hip) and the
// weight-stationary kernels (conv_ws.hip).  conv_common.h includes this file at its end; it uses the vector typedefs from there.
// A helper is used in a kernel only where the compiled kernel stayed instruction-identical; the other sites keep the
// hand-written form (profiles/stream_helpers_isa.txt).
//
// THE TILE-LOOP PROTOCOL.  The host plans the grid (plan_stream); a workgroup takes one contiguous run of tiles (tile_run)
// and keeps its weights in registers for the whole run.  Per run:
//
//     stage(first tile, buffer 0);  vm_wait<0>(weights, biases ..);            // prologue: the only full drain
//     for (tile in run) {
//       tile_decode(tile) -> b, t0 as SCALARS (they feed V#s, which must live in SGPRs)
//       lgkm_wait<0>(); s_barrier;      // every wave's pieces of this tile are in LDS; the other buffer is free again
//       stage(tile + 1, other buffer)   // untracked LDS-DMA through a range-checked V#: rows outside the item read as zero,
//                                       //   and every instruction IS issued, whatever the tile's position
//       body: LDS fragments -> transposed 32 x 32 MFMA tiles (A = weights, B = rows) -> epilogue in registers ->
//             pair_up8 -> store_paired through a V# (rows beyond the item are dropped by the range check, but ISSUED)
//       step_end_wait<S>();             // S = the stores this wave issued in the body
//     }
//
// Vector memory completes in issue order.  The next tile's DMA is issued BEFORE the body's stores, so vmcnt(S) at the end of
// a tile says "everything older than my S stores is done": the prefetched tile has landed, while the stores drain under the
// next tile.  S must be a compile-time count of instructions that are issued on every path, which is why loads and stores
// go through range-checked V#s instead of per-lane bounds tests.  Whatever the body itself needs from global memory
// (residual rows, the next step's weights) is issued before or with the prefetch and is covered by a counted wait of its
// own.  The compiler must place none of these waits: it answers the first use of any load it tracks with vmcnt(0), which
// also drains the prefetch -- hence the untracked_* loads (inline asm), scalar lens loads, raw s_barrier + lgkm_wait<0>
// instead of __syncthreads(), and the register pins of vm_wait.  The order stage / barrier / body / wait and every
// sched_barrier stay written out in each kernel: these kernels are register-tight and their instruction order is the product.
#pragma once
#include <algorithm>
#include <cstdlib>

#include "smt_common.h"

namespace smt {

// ---- host: the launch plan ---------------------------------------------------------------------------------------------
// At least min_tpw tiles per workgroup (so that the double buffer pays), at most `cap` workgroups (CUs x workgroups per CU),
// whole XCD octets (tile_run deals the runs out by XCD).
struct StreamGrid { int nwg, tiles_per_wg; };
inline StreamGrid plan_stream(long long ntiles, int cap, int min_tpw) {
  long long nwg = std::min<long long>(cap, std::max<long long>(8, (ntiles + min_tpw - 1) / min_tpw));
  nwg = (nwg + 7) / 8 * 8;
  return {(int)nwg, (int)((ntiles + nwg - 1) / nwg)};
}

// Tiles a persistent workgroup of the fused backward kernels takes at least (SMT_FUSED_MIN_TPW): every workgroup leaves a
// partial weight-gradient slab that the reduce kernel reads back, so at the small levels of the model fewer, longer
// workgroups cost less than the slabs of 256 short ones.
inline int fused_min_tpw() {
  static const int v = [] { const char* e = getenv("SMT_FUSED_MIN_TPW"); return e ? std::max(1, atoi(e)) : 2; }();
  return v;
}

// ---- the run of a workgroup --------------------------------------------------------------------------------------------
// Workgroup `block` of nwg (a multiple of 8) takes tiles [begin, end): tiles_per_wg consecutive tiles, and the runs of
// blocks b, b + 8, .. (one XCD, one L2) are adjacent -- neighbouring tiles share their halo rows and the weights in L2.
// begin >= end: no tile left for this workgroup; with clamp_begin an empty run is begin == end == ntiles.
struct TileRun { int wg, begin, end; };
__host__ __device__ inline TileRun tile_run(int nwg, unsigned block, int ntiles, int tiles_per_wg, bool clamp_begin = false) {
  TileRun t;
  t.wg = (int)((block & 7) * (nwg >> 3) + (block >> 3));
  t.begin = t.wg * tiles_per_wg;
  if (clamp_begin && ntiles < t.begin) t.begin = ntiles;
  t.end = ntiles < t.begin + tiles_per_wg ? ntiles : t.begin + tiles_per_wg;
  return t;
}
// The run of this workgroup; false: no tile, the kernel returns.  (The fused backward kernels call tile_run themselves and
// do NOT return: a workgroup without tiles still writes its zero partial slab, which the reducer reads.)
__device__ __forceinline__ bool wg_tile_run(int ntiles, int tiles_per_wg, int& wg, int& tile_begin, int& tile_end) {
  const TileRun t = tile_run(gridDim.x, blockIdx.x, ntiles, tiles_per_wg);
  wg = t.wg; tile_begin = t.begin; tile_end = t.end;
  return tile_begin < tile_end;
}
// tile -> (batch item, first row of the tile), as SCALARS: the V#s built from them must live in SGPRs (a divergent-looking
// descriptor costs a waterfall loop per DMA instruction, and a vector load of lens[b] would be a tracked load again)
template <int ROWS>
__device__ __forceinline__ void tile_decode(int tile, int tiles_per_batch, int& b, int& t0) {
  b = __builtin_amdgcn_readfirstlane(tile / tiles_per_batch);
  t0 = __builtin_amdgcn_readfirstlane((tile - b * tiles_per_batch) * ROWS);
}

// ---- buffer addressing -------------------------------------------------------------------------------------------------
// A range-checked V# over `bytes` bytes from base + byte_off -- per-lane offsets are 32-bit, loads beyond the range return
// zero and stores beyond it are dropped (no per-lane bounds selects, no zero page), and every such instruction IS issued, so
// `s_waitcnt vmcnt(N)` counts stay compile-time constants.
typedef int i32x4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t ws_rsrc(const void* base, long long byte_off, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(base)) + byte_off, 0, (int)bytes, 0x00020000);
}
// LDS-DMA through a V#: 64 x 16 B (per-lane byte offset) to 1 KiB of LDS at a wave-uniform base
__device__ __forceinline__ void ws_dma16(__amdgpu_buffer_rsrc_t rs, unsigned voff, void* lds_wave_base) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds_wave_base, 16, (int)voff, 0, 0, 0);
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
// serialises a double-buffered stream (measured on conv_k3gate: every step waited for its own prefetch).  The caller owns
// the wait: s_waitcnt vmcnt(N) with N = the vector-memory instructions issued after this one.
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

// ---- LDS layouts: the 16-byte chunk c of staged row `row` sits at chunk c ^ swz(row) -----------------------------------
// 128-byte rows read as row fragments (b128 per lane, 32 consecutive rows): two rows share a 256-byte bank window
__device__ __forceinline__ int swz128_row(int row) { return (row >> 1) & 7; }
// 128-byte rows that are also read transposed (ds_read_b64_tr_b16): transposed fragments conflict-free, row fragments 2-way
__device__ __forceinline__ int swz128_tr(int row) { return ((row >> 1) & 3) << 1; }
// 256-byte rows read as row fragments: 16 consecutive rows hit 16 different chunks
__device__ __forceinline__ int swz256_row(int row) { return row & 15; }
// 256-byte / 1-KiB rows read both ways: 16 consecutive rows hit 16 different chunks (row fragments) and 4 consecutive rows
// are 64 B apart (transposed fragments, 4 rows x 32 B per 16-lane group)
__device__ __forceinline__ int swz256_tr(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }

// B-operand fragment of k-step kk: 8 consecutive channels 16 kk + 8 hh.. of staged row `row` (swz = the layout's swz(row))
__device__ __forceinline__ bf16x8 lds_row_frag(const unsigned char* tile, int row, int row_bytes, int kk, int hh, int swz) {
  return *reinterpret_cast<const bf16x8*>(tile + row * row_bytes + (((2 * kk + hh) ^ swz) << 4));
}
// Transposed fragment: two ds_read_b64_tr_b16, four rows apart (pa, pb = this lane's addresses in the two row groups)
__device__ __forceinline__ bf16x8 lds_tr2(const unsigned char* pa, const unsigned char* pb) {
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)pa);
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)pb);
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}

// ---- operands kept in registers for the run ----------------------------------------------------------------------------
// A-operand fragments of one packed weight row (this lane's output channel), k-steps 0 .. N - 1; swz = 0 for the plain
// packed layout, co & 15 for the swizzled one (chunk c of row co sits at c ^ (co & 15))
template <int N>
__device__ __forceinline__ void load_wfrags(bf16x8 (&w)[N], const unsigned char* wrow, int hh, int swz = 0) {
#pragma unroll
  for (int kk = 0; kk < N; ++kk) w[kk] = *reinterpret_cast<const bf16x8*>(wrow + (((2 * kk + hh) ^ swz) << 4));
}

// ---- the way out -------------------------------------------------------------------------------------------------------
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
// ... and store them straight from registers: vo = byte offset of this lane's first piece (row, channel 8 hh of the tile),
// the second piece `second` bytes on (16 channels; conv_k3gate's s half sits 64 channels on)
__device__ __forceinline__ void store_paired(const unsigned (&v)[8], __amdgpu_buffer_rsrc_t rs, unsigned vo, unsigned second = 32u) {
  __builtin_amdgcn_raw_buffer_store_b128(i32x4v{(int)v[0], (int)v[1], (int)v[2], (int)v[3]}, rs, (int)vo, 0, 0);
  __builtin_amdgcn_raw_buffer_store_b128(i32x4v{(int)v[4], (int)v[5], (int)v[6], (int)v[7]}, rs, (int)(vo + second), 0, 0);
}

}  // namespace smt
