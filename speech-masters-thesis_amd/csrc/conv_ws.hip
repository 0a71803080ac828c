// Weight-stationary convolution kernels (bf16, C_in == 128, 3..9 taps), the dilated 128 -> 128 convs of the GatedHiFi block:
// the k x 128 x 128 weight block of a dilated conv
// is at most 288 KiB -- too large for LDS, but it fits the REGISTER FILE of one CU.  Four waves (one per
// SIMD, up to 512 VGPRs each) each own 32 output channels and keep that slice of every tap in registers
// for the whole run of a persistent workgroup, so nothing but activations moves through LDS:
//   * activation tiles (128 rows + halo) arrive by LDS-DMA into a double buffer: tile i+1 and the epilogue
//     operands of tile i are in flight while tile i is multiplied, and the stores of tile i-1 drain;
//   * ONE barrier per tile (the buffer swap); the tap loop has none;
//   * the MFMA computes the TRANSPOSED tile (A = weights, B = activations), so a lane ends up with 4
//     consecutive output channels of one row; a v_permlane32_swap pairs them to 16-byte pieces that are stored
//     straight from registers -- no LDS staging of the output, no epilogue barrier;
//   * each wave DMAs its own 64-byte column slice of the residual / activation-source rows to LDS and reads
//     only that back, so the epilogue operands need neither registers during the tap loop nor a barrier.
// Measured motivation (ablation build, tools/ablate_dma.sh of commit 29a7cd8): the streaming kernel spends as long
// waiting for HBM (tile in, tile out) as it does in MFMAs, and with one workgroup per CU the two never overlap.
// Buffer addressing (raw V#, byte offsets): rows outside [0, valid rows) fall outside num_records and read as zero /
// are not stored -- the hardware's range check replaces the per-lane bounds tests and zero-page selects, and a per-lane
// 32-bit offset replaces the 64-bit address arithmetic (both were VALU work serial with the MFMAs: tools/ws_phases.py
// measured 1,100-2,000 cycles per tile for the issue of ~5 DMA instructions per wave).
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "smt_common.h"
#include "conv_common.h"

namespace smt {

#ifndef SMT_WS_STAMP
#define SMT_WS_STAMP 0   // diagnostic build (tools/ws_phases.sh): per-wave cycle sums of the phases of the three kernels
#endif
#if SMT_WS_STAMP
__device__ unsigned long long ws_dbg[256 * 8 * 8];
#define WS_T(var) const unsigned long long var = __builtin_readcyclecounter()
#define WS_ACC(k, a, b) do { if (lane == 0 && wg < 256) ws_dbg[(wg * 8 + wave) * 8 + (k)] += (b) - (a); } while (0)
#else
#define WS_T(var) do {} while (0)
#define WS_ACC(k, a, b) do {} while (0)
#endif
constexpr int WS_AGPR_TAPS = 8;   // taps whose weights are pinned to AccVGPRs (8 x 32 = all 256)
constexpr int WS_BM = 128, WS_BN = 128, WS_NT = 256, WS_EPI = 128 * 256;   // rows, output channels per tile, threads, epilogue-operand tile bytes
constexpr int WS_KC = 128, WS_ROWB = WS_KC * 2, WS_KSTEPS = WS_KC / 16;     // input channels, bytes per LDS row, 16-channel k-steps per tap

template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// ---- the pieces the three kernels share: one definition each ----------------------------------------------------------
// The kernels are sensitive to code shape (register classes, issue order), so each piece was accepted only where the
// compiled kernels stayed instruction-identical.  Pieces that did not pass that check are still written out per kernel: the
// loops of the weight-slice load, of the activation staging (stage_a) and of the epilogue-operand staging (stage_epi), and
// in conv_ws2_kernel the tap bases and the lane pairing.  (The persistent tile split and the lane pairing with its stores
// are in conv_stream.h: wg_tile_run, pair_up8, store_paired.)

// weight fragment kk of output channel co (row wrow of the packed block; packed swizzled: chunk c of row co sits at
// c ^ (co & 15)): a wave keeps its 32 output channels of every tap in registers
__device__ __forceinline__ bf16x8 ws_wfrag(const unsigned char* wrow, int kk, int hh, int co) {
  return *reinterpret_cast<const bf16x8*>(wrow + (((2 * kk + hh) ^ (co & 15)) << 4));
}

// tile -> (batch, class, first class row)
__device__ __forceinline__ void ws_decode(int tiles_per_batch, int rs, int tile, int& b, int& cls, int& t0) {
  const int bb = tile / tiles_per_batch;
  b = bb / rs; cls = bb - b * rs;
  t0 = (tile - bb * tiles_per_batch) * WS_BM;
}

// fragment address of step (s, kk) = tap_base[s] ^ (32 kk): buffers are 1 KiB-aligned, so the XOR swizzle of the 16-byte
// chunk index (bits 4..7) can be applied after the buffer base has been added.  ar = lane row + tap offset: rows
// ar + 32 i share the swizzle term (ar & 15).
__device__ __forceinline__ unsigned ws_tap_base(unsigned abase, int ar, int hh) { return abase + ar * WS_ROWB + ((hh ^ swz256_row(ar)) << 4); }
template <int NTAPS>
__device__ __forceinline__ unsigned ws_frag_addr(const unsigned (&tap_base)[NTAPS], int q) {
  return tap_base[q / WS_KSTEPS] ^ (32u * (q % WS_KSTEPS));
}

// The MFMA pipeline over the NTAPS x 8 k-steps is written as asm so that it stays a pipeline: the fragments of a later
// step are requested before the MFMAs of step q (one or two waves per SIMD -- nothing else hides the LDS latency) and a
// counted `s_waitcnt lgkmcnt` retires exactly the older reads (LDS returns in order; a stray scalar load in flight only makes
// the wait more conservative).  The asm also pins the register classes: the first taps of the weight block live in AccVGPRs
// and are read directly as an operand, the rest and the accumulators in VGPRs.  Left to itself the compiler keeps all 288
// weight registers in the 256 VGPRs, spills to AccVGPRs, and serialises every ds_read behind the previous MFMA.
template <int MW>
__device__ __forceinline__ void ws_read_frags(bf16x8 (&afr)[MW], unsigned ap) {   // rows 32 i of this lane, one k-step
#pragma unroll
  for (int i = 0; i < MW; ++i)
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(afr[i]) : "v"(ap), "n"(i * 32 * WS_ROWB));
}
// first use of an accumulator: the compiler may have initialised it with a VALU move in the instruction just before, and
// it cannot see that an MFMA follows (VALU write -> MFMA SrcC needs wait states)
__device__ __forceinline__ void ws_first_use(f32x16& acc) { asm volatile("s_nop 4" : "+v"(acc)); }
__device__ __forceinline__ void ws_first_use(f32x16& acc0, f32x16& acc1) { asm volatile("s_nop 4" : "+v"(acc0), "+v"(acc1)); }
// D^T = W * A^T: operand A = weights [32 co x 16 k], operand B = activations [16 k x 32 rows]
__device__ __forceinline__ void ws_mfma(f32x16& acc, const bf16x8& w, const bf16x8& a, bool w_in_agpr) {
  if (w_in_agpr) asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "a"(w), "v"(a));
  else asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(w), "v"(a));
}
// The hazard recogniser does not see MFMAs inside asm: let the last ones drain before VALU reads acc.  The accumulators
// are operands of the nops so that no reader of acc can be scheduled above them.
template <int MW>
__device__ __forceinline__ void ws_drain(f32x16 (&acc)[MW]) {
  static_assert(MW == 2 || MW == 4, "the drain names two or four accumulators");
#define WS_DRAIN_NOPS "s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15"
  if constexpr (MW == 4) asm volatile(WS_DRAIN_NOPS : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]));
  else asm volatile(WS_DRAIN_NOPS : "+v"(acc[0]), "+v"(acc[1]));
#undef WS_DRAIN_NOPS
}

// MODE fixes the epilogue at compile time (straight-line code instead of ~85 branches in the unrolled epilogue, which
// a single wave per SIMD cannot hide): 1 = activated output only (K2 forward), 2 = y with activation-gradient mask and
// residual (K2 data gradient), 0 = whatever the descriptor asks for.
template <int NTAPS, int MODE>
__global__ __launch_bounds__(WS_NT) void conv_ws_kernel(ConvArgs p, const __bf16* __restrict__ zero_page,
                                                        int tiles_per_wg, int buf_bytes) {
  const bool has_y = MODE == 0 ? (p.y != nullptr) : (MODE == 2);
  const bool has_act_out = MODE == 0 ? (p.act_out != 0) : (MODE == 1);
  const bool has_res = MODE == 0 ? (p.res != nullptr) : (MODE == 2);
  const bool has_epi_act = MODE == 0 ? (p.epi_act != 0) : (MODE == 2);
  typedef __bf16 T;
  constexpr int BM = WS_BM, BN = WS_BN, KC = WS_KC, NT = WS_NT, MW = BM / 32, ROWB = WS_ROWB;
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int lrow = lane >> 4, lch = lane & 15;
  const int n0 = blockIdx.y * BN;
  const int rs = p.rs;

  int wg, tile_begin, tile_end;
  if (!wg_tile_run(p.tiles_per_batch * p.B * rs, tiles_per_wg, wg, tile_begin, tile_end)) return;

  // epilogue-operand tiles: per wave [128 rows][64 B] (its 32 output channels), 16-byte chunks XOR-swizzled
  unsigned char* lds_res = smem + 2 * (size_t)buf_bytes + wave * (WS_EPI / 4);
  unsigned char* lds_act = lds_res + WS_EPI;
  const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;

  // this wave's 32 output channels of every tap -> registers
  bf16x8 wfrag[NTAPS][KC / 16];
  {
    const int co = n0 + wave * 32 + r;
#pragma unroll
    for (int s = 0; s < NTAPS; ++s) {
      const unsigned char* wrow = reinterpret_cast<const unsigned char*>(p.w) + ((size_t)s * p.Cout + co) * ROWB;
#pragma unroll
      for (int kk = 0; kk < KC / 16; ++kk)
        wfrag[s][kk] = ws_wfrag(wrow, kk, hh, co);
    }
  }
  // accumulator element 4g + k of a lane = output channel col0 + 8g + k (this lane's row: 32 i + r)
  const int col0 = n0 + wave * 32 + 4 * hh;
  float bval[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) bval[e] = p.bias ? p.bias[col0 + 8 * (e >> 2) + (e & 3)] : 0.f;
  const int rows_in = BM + (NTAPS - 1) * p.dil;
  const int rows_pad = (rows_in + 3) & ~3;

  auto decode = [&](int tile, int& b, int& cls, int& t0) { ws_decode(p.tiles_per_batch, rs, tile, b, cls, t0); };
  // buffer addressing (ws_rsrc / ws_dma16): per-lane byte offsets are tile-invariant up to a scalar; rows outside
  // [0, valid rows) are out of range of the V# and read as zero.  Group g = wave + 4 j covers rows 16 j + 4 wave + lrow,
  // so the swizzle term (row & 15) does not depend on j.
  const unsigned pitch_x = (unsigned)p.ldx * rs * 2u;
  const unsigned voff_a0 = (unsigned)(4 * wave + lrow) * pitch_x + (unsigned)((lch ^ swz256_row(4 * wave + lrow)) << 4);
  const int ngroups = rows_pad >> 2;
  auto stage_a = [&](int tile, int buf) {
    int b, cls, t0;
    decode(tile, b, cls, t0);
    const int len_full = p.lens_in ? min(scalar_load_i32(p.lens_in + b), p.Tin) : p.Tin;
    const int len_in = max(0, (len_full - cls + rs - 1) / rs);
    const __amdgpu_buffer_rsrc_t rx = ws_rsrc(p.x, ((long long)b * p.x_bs + (long long)cls * p.ldx) * 2, (unsigned)len_in * pitch_x);
    unsigned vo = voff_a0 + (unsigned)(t0 - p.pad) * pitch_x;      // rows before the item wrap to huge offsets: zero
    unsigned char* dst = smem + (size_t)buf * buf_bytes + wave * 1024;
    for (int g = wave; g < ngroups; g += NT / 64) {
      ws_dma16(rx, vo, dst);
      vo += 16u * pitch_x; dst += 4096;
    }
  };
  // this wave's slice of an epilogue operand: one DMA instruction = 16 rows x 64 B; slot c of row n holds the
  // 16-byte chunk c ^ ((n >> 2) & 3) of the slice (keeps the 8-byte fragment reads at <= 2-way bank conflicts)
  const unsigned echunk = (unsigned)(((lane & 3) ^ ((lane >> 4) & 3)) << 4);
  auto stage_epi = [&](const void* base, long long bs, int ld, int b, int cls, int t0, int Tc, unsigned char* dst) {
    const unsigned pitch = (unsigned)ld * rs * 2u;
    const __amdgpu_buffer_rsrc_t re = ws_rsrc(base, ((long long)b * bs + (long long)cls * ld + n0 + wave * 32) * 2, (unsigned)Tc * pitch);
    unsigned vo = (unsigned)(t0 + (lane >> 2)) * pitch + echunk;
#pragma unroll
    for (int q = 0; q < BM / 16; ++q) {
      ws_dma16(re, vo, dst + q * 1024);
      vo += 16u * pitch;
    }
  };

  stage_a(tile_begin, 0);
  vm_wait<0>();
  for (int tile = tile_begin; tile < tile_end; ++tile) {
    const int buf = (tile - tile_begin) & 1;
    int b, cls, t0;
    decode(tile, b, cls, t0);
    const int Tc = (p.Tout - cls + rs - 1) / rs;
    // tile `tile` is in LDS for every wave (each waited for its own DMAs before its previous epilogue) and
    // every wave is done reading the other buffer
    WS_T(c0);
    __syncthreads();
    WS_T(c1);
    // MODE 2 (the data gradient) issues none of its pieces here: issued as one burst, with the matrix pipe idle, a piece
    // cost 140-190 cycles of issue time (profiles/dma_placement_phases.txt), so they go out one per k-step behind that
    // step's first MFMA (dma_slot below).  What the burst built per tile is built here: descriptors, lens_in[b] (a scalar
    // load, which must not sit inside the counted lgkmcnt pipeline) and the per-lane offsets, which then advance by scalars.
    // The last tile of the run has no next tile: n_in = 0 skips its input pieces.
    __amdgpu_buffer_rsrc_t rx_n = ws_rsrc(p.x, 0, 0), re_res = rx_n, re_act = rx_n;
    unsigned vo_in = 0, vo_res = 0, vo_act = 0, pitch_res = 0, pitch_act = 0;
    int n_in = 0;
    // the wave index as a SCALAR: with the per-lane value in a descriptor's base the compiler keeps the descriptor in
    // VGPRs and wraps every piece in a waterfall loop (four v_readfirstlane and a branch per piece: what stage_epi pays)
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    if constexpr (MODE == 2) {
      if (tile + 1 < tile_end) {
        int nb, ncls, nt0;
        decode(tile + 1, nb, ncls, nt0);
        const int len_full = p.lens_in ? min(scalar_load_i32(p.lens_in + nb), p.Tin) : p.Tin;
        const int len_in = max(0, (len_full - ncls + rs - 1) / rs);
        rx_n = ws_rsrc(p.x, ((long long)nb * p.x_bs + (long long)ncls * p.ldx) * 2, (unsigned)len_in * pitch_x);
        vo_in = voff_a0 + (unsigned)(nt0 - p.pad) * pitch_x;
        n_in = ngroups;
      }
      pitch_res = (unsigned)p.ldr * rs * 2u; pitch_act = (unsigned)p.ldgh * rs * 2u;
      re_res = ws_rsrc(p.res, ((long long)b * p.res_bs + (long long)cls * p.ldr + n0 + wave_s * 32) * 2, (unsigned)Tc * pitch_res);
      re_act = ws_rsrc(p.gate_h, ((long long)b * p.gh_bs + (long long)cls * p.ldgh + n0 + wave_s * 32) * 2, (unsigned)Tc * pitch_act);
      vo_res = (unsigned)(t0 + (lane >> 2)) * pitch_res + echunk;
      vo_act = (unsigned)(t0 + (lane >> 2)) * pitch_act + echunk;
    } else {
      if (tile + 1 < tile_end) stage_a(tile + 1, buf ^ 1);
    }
    WS_T(c2);
    if constexpr (MODE != 2) {
      if (has_res) stage_epi(p.res, p.res_bs, p.ldr, b, cls, t0, Tc, lds_res);
      if (has_epi_act) stage_epi(p.gate_h, p.gh_bs, p.ldgh, b, cls, t0, Tc, lds_act);
    }
    // slot q of the tap loop: the 8 + 8 epilogue-operand pieces first (the epilogue reads them right after the loop), then
    // up to WS_IN_SLOTS input pieces of the next tile (12 = 192 rows, more than the LDS budget of the plan allows)
    constexpr int WS_EPI_SLOTS = BM / 16, WS_IN_SLOTS = 12, WS_SLOTS = 2 * WS_EPI_SLOTS + WS_IN_SLOTS;
    static_assert(MODE != 2 || WS_SLOTS <= NTAPS * (KC / 16), "one piece per k-step");
    unsigned char* const dst_in = smem + (size_t)(buf ^ 1) * buf_bytes + wave_s * 1024;
    unsigned char* const dst_res = smem + 2 * (size_t)buf_bytes + wave_s * (WS_EPI / 4), * const dst_act = dst_res + WS_EPI;   // = lds_res, lds_act
    auto dma_slot = [&](int s) {
      if (s < WS_EPI_SLOTS) ws_dma16(re_res, vo_res + (unsigned)(16 * s) * pitch_res, dst_res + s * 1024);
      else if (s < 2 * WS_EPI_SLOTS) ws_dma16(re_act, vo_act + (unsigned)(16 * (s - WS_EPI_SLOTS)) * pitch_act, dst_act + (s - WS_EPI_SLOTS) * 1024);
      else {
        const int j = s - 2 * WS_EPI_SLOTS;
        if (wave_s + 4 * j < n_in) ws_dma16(rx_n, vo_in + (unsigned)(16 * j) * pitch_x, dst_in + j * 4096);
      }
    };

    WS_T(c4);
    f32x16 acc[MW];
#pragma unroll
    for (int i = 0; i < MW; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    // the MFMA pipeline (see ws_read_frags), one step ahead; all of WS_AGPR_TAPS taps pinned to AccVGPRs
    const unsigned abase = lds_base + (unsigned)buf * (unsigned)buf_bytes;
    unsigned tap_base[NTAPS];
#pragma unroll
    for (int s = 0; s < NTAPS; ++s) tap_base[s] = ws_tap_base(abase, r + s * p.dil, hh);
    auto frag_addr = [&](int q) -> unsigned { return ws_frag_addr(tap_base, q); };
    bf16x8 afr[2][MW];
    ws_read_frags(afr[0], frag_addr(0));
#pragma unroll
    for (int q = 0; q < NTAPS * (KC / 16); ++q) {
      if (q + 1 < NTAPS * (KC / 16)) {
        ws_read_frags(afr[(q + 1) & 1], frag_addr(q + 1));
        lgkm_wait<MW>();                            // the MW reads of step q are done, those of step q + 1 in flight
      } else {
        lgkm_wait<0>();
      }
#pragma unroll
      for (int i = 0; i < MW; ++i) {
        if (q == 0) ws_first_use(acc[i]);
        ws_mfma(acc[i], wfrag[q / (KC / 16)][q % (KC / 16)], afr[q & 1][i], q / (KC / 16) < WS_AGPR_TAPS);
        if (MODE == 2 && i == 0 && q < WS_SLOTS) {   // one piece behind the step's first MFMA, fenced so that it stays there
          __builtin_amdgcn_sched_barrier(0);
          dma_slot(q);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    ws_drain(acc);
    WS_T(c5);
    // next tile + this tile's epilogue operands have landed (issued a whole tap loop ago); older stores retired
    vm_wait<0>();
    WS_T(c6);

    // ---- epilogue straight from the accumulators; same arithmetic as the other kernels: bf16(acc + bias) first.
    // Stores go through range-checked buffer descriptors (rows >= Tc are dropped by the hardware, 32-bit offsets).
    const int len_out = p.lens_out ? scalar_load_i32(p.lens_out + b) : 0x7fffffff;
    const unsigned pitch_y = (unsigned)p.ldy * rs * 2u, pitch_u = (unsigned)p.ldya * rs * 2u;
    const __amdgpu_buffer_rsrc_t ry = ws_rsrc(has_y ? p.y : p.x, has_y ? ((long long)b * p.y_bs + (long long)cls * p.ldy + n0 + (MODE == 2 ? wave_s : wave) * 32) * 2 : 0,
                                              has_y ? (unsigned)Tc * pitch_y : 0u);
    const __amdgpu_buffer_rsrc_t ru = ws_rsrc(has_act_out ? p.y_act : p.x,
                                              has_act_out ? ((long long)b * p.ya_bs + (long long)cls * p.ldya + n0 + wave * 32) * 2 : 0,
                                              has_act_out ? (unsigned)Tc * pitch_u : 0u);
    if constexpr (MODE == 2) {
      // dx = y * scale * [u != 0] * row mask + residual, written for few VALU instructions (tools/ws_phases.py: at one wave
      // per SIMD the epilogue and the DMA issue are serial with the tap loop).  The eight LDS reads of a row block are
      // issued together, so their latency is paid once per row block.  (Tried and dropped in round 3: loading the two
      // operands straight into registers in the store layout after touching their lines before the tap loop -- the 4-byte
      // touches, 64 lines per instruction, slowed the tap loop by 20 %: 826 vs 775 us at 9 taps.)
#pragma unroll
      for (int i = 0; i < MW; ++i) {
        const int row = 32 * i + r;
        const int tc = t0 + row;
        const float srow = (cls + rs * tc >= len_out) ? 0.f : p.drop_scale;     // row mask and 1 / (1 - p) in one factor
        const int swz = (row >> 2) & 3;
        uint2 uv[4], rv[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int eoff = row * 64 + ((g ^ swz) << 4) + 8 * hh;
          uv[g] = *reinterpret_cast<const uint2*>(lds_act + eoff);
          rv[g] = *reinterpret_cast<const uint2*>(lds_res + eoff);
        }
        unsigned yp[8];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const unsigned uvp[2] = {uv[g].x, uv[g].y}, rvp[2] = {rv[g].x, rv[g].y};
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const unsigned ypk = pack_bf16x2(acc[i][4 * g + 2 * j] + bval[4 * g + 2 * j], acc[i][4 * g + 2 * j + 1] + bval[4 * g + 2 * j + 1]);
            const float o0 = __builtin_bit_cast(float, ypk << 16), o1 = __builtin_bit_cast(float, ypk & 0xffff0000u);
            const float v0 = (uvp[j] & 0x7fffu) ? o0 * srow : 0.f, v1 = (uvp[j] & 0x7fff0000u) ? o1 * srow : 0.f;
            yp[2 * g + j] = pack_bf16x2(v0 + __builtin_bit_cast(float, rvp[j] << 16), v1 + __builtin_bit_cast(float, rvp[j] & 0xffff0000u));
          }
        }
        pair_up8(yp);
        store_paired(yp, ry, (unsigned)tc * pitch_y + (unsigned)hh * 16u);
      }
    } else {
#pragma unroll
    for (int i = 0; i < MW; ++i) {
      const int row = 32 * i + r;
      const int tc = t0 + row;
      const int ty = cls + rs * tc;                          // actual output row
      const float keep_row = (ty >= len_out) ? 0.f : 1.f;
      const int swz = (row >> 2) & 3;
      unsigned yp[8], up[8];
      {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = (float)(T)(acc[i][4 * g + k] + bval[4 * g + k]);
        const int eoff = row * 64 + ((g ^ swz) << 4) + 8 * hh;
        if (has_epi_act) {
          const bf16x4 uv = *reinterpret_cast<const bf16x4*>(lds_act + eoff);
#pragma unroll
          for (int k = 0; k < 4; ++k) o[k] = ((float)uv[k] != 0.f) ? o[k] * p.drop_scale : 0.f;
        }
        if (has_res) {
          const bf16x4 rv = *reinterpret_cast<const bf16x4*>(lds_res + eoff);
#pragma unroll
          for (int k = 0; k < 4; ++k) o[k] = fmaf(o[k], keep_row, (float)rv[k]);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) o[k] *= keep_row;
        }
        yp[2 * g] = pack_bf16x2(o[0], o[1]);
        yp[2 * g + 1] = pack_bf16x2(o[2], o[3]);
        if (has_act_out) {
          const int col = col0 + 8 * g;
          const int site = col / p.site_width;
          const unsigned key = site_key(p, site);
          const unsigned long long base = ((unsigned long long)b * p.Ty + ty) * p.site_width + (col - site * p.site_width);
#pragma unroll
          for (int k = 0; k < 4; k += 2) {
            const unsigned h = fmix32((unsigned)((base + k) >> 1) * 0x9E3779B1u + key);
            const bool k0 = (h & 0xFFFFu) >= p.drop_thresh16, k1 = (h >> 16) >= p.drop_thresh16;
            up[2 * g + (k >> 1)] = pack_bf16x2((k0 && o[k] > 0.f) ? o[k] * p.drop_scale : 0.f,
                                               (k1 && o[k + 1] > 0.f) ? o[k + 1] * p.drop_scale : 0.f);
          }
        }
      }
      }
      if (has_y) {
        pair_up8(yp);
        store_paired(yp, ry, (unsigned)tc * pitch_y + (unsigned)hh * 16u);
      }
      if (has_act_out) {
        pair_up8(up);
        store_paired(up, ru, (unsigned)tc * pitch_u + (unsigned)hh * 16u);
      }
    }
    }
    WS_T(c7);
    WS_ACC(0, c0, c1); WS_ACC(1, c1, c2); WS_ACC(3, c2, c4); WS_ACC(4, c4, c5); WS_ACC(5, c5, c6); WS_ACC(6, c6, c7); WS_ACC(7, c0, c0 + 1);
  }
}

// ------------------------------------------------------------------------------------------------
// Weight-stationary kernel with the epilogue of tile i-1 hidden in the MFMA gaps of tile i (K2 forward: only the
// activated output u = relu(dropout(y)) is written).  One wave per SIMD issues strictly in order, so the epilogue of
// conv_ws_kernel (~1000 VALU instructions per tile at 4 cycles each) runs while the matrix core idles; but an
// MFMA holds the vector issue port for only 8 of its 32 cycles, which leaves room for ~5 other instructions per MFMA.
// Here the finished accumulators are packed to bf16 (32 registers) and the rest of the epilogue -- dropout hash,
// ReLU, scaling, lane pairing, stores -- is cut into micro-steps of 2..10 instructions, one behind each MFMA of the
// next tile (sched_barrier keeps them where they are written).  Taps 0..7 of the weight block are pinned to
// AccVGPRs.  Same arithmetic as conv_ws_kernel: bit-identical outputs.
template <int NTAPS>
__global__ __launch_bounds__(WS_NT) void conv_ws_pipe_kernel(ConvArgs p, const __bf16* __restrict__ zero_page,
                                                             int tiles_per_wg, int buf_bytes) {
  constexpr int BM = WS_BM, BN = WS_BN, KC = WS_KC, NT = WS_NT, MW = BM / 32, ROWB = WS_ROWB;
  constexpr int NSTEP = NTAPS * (KC / 16), NGAP = NSTEP * MW;
  constexpr int PH_UNIT = 12, PH_ROW = 4 * PH_UNIT + 2, PH_TILE = MW * PH_ROW;
  constexpr int AGPR_TAPS = NTAPS < 8 ? NTAPS : 8;
  static_assert(MW == 4, "four accumulators");
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int lrow = lane >> 4, lch = lane & 15;
  const int n0 = blockIdx.y * BN;
  const int rs = p.rs;

  int wg, tile_begin, tile_end;
  if (!wg_tile_run(p.tiles_per_batch * p.B * rs, tiles_per_wg, wg, tile_begin, tile_end)) return;
  const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;

  bf16x8 wfrag[NTAPS][KC / 16];
  {
    const int co = n0 + wave * 32 + r;
#pragma unroll
    for (int s = 0; s < NTAPS; ++s) {
      const unsigned char* wrow = reinterpret_cast<const unsigned char*>(p.w) + ((size_t)s * p.Cout + co) * ROWB;
#pragma unroll
      for (int kk = 0; kk < KC / 16; ++kk)
        wfrag[s][kk] = ws_wfrag(wrow, kk, hh, co);
    }
  }
  // accumulator element 4g + k of a lane = output channel col0 + 8g + k (this lane's row: 32 i + r)
  const int col0 = n0 + wave * 32 + 4 * hh;
  float bval[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) bval[e] = p.bias ? p.bias[col0 + 8 * (e >> 2) + (e & 3)] : 0.f;
  unsigned keyg[4], cshalf[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int col = col0 + 8 * g;
    const int site = col / p.site_width;
    keyg[g] = site_key(p, site);
    cshalf[g] = (unsigned)(col - site * p.site_width) >> 1;
  }
  const int rows_in = BM + (NTAPS - 1) * p.dil;
  const int rows_pad = (rows_in + 3) & ~3;

  auto decode = [&](int tile, int& b, int& cls, int& t0) { ws_decode(p.tiles_per_batch, rs, tile, b, cls, t0); };
  // buffer addressing as in conv_ws_kernel: one per-lane offset, a scalar per tile, out-of-range rows read as zero
  const unsigned pitch_x = (unsigned)p.ldx * rs * 2u;
  const unsigned voff_a0 = (unsigned)(4 * wave + lrow) * pitch_x + (unsigned)((lch ^ swz256_row(4 * wave + lrow)) << 4);
  const int ngroups = rows_pad >> 2;
  auto stage_a = [&](int tile, int buf) {
    int b, cls, t0;
    decode(tile, b, cls, t0);
    const int len_full = p.lens_in ? min(scalar_load_i32(p.lens_in + b), p.Tin) : p.Tin;
    const int len_in = max(0, (len_full - cls + rs - 1) / rs);
    const __amdgpu_buffer_rsrc_t rx = ws_rsrc(p.x, ((long long)b * p.x_bs + (long long)cls * p.ldx) * 2, (unsigned)len_in * pitch_x);
    unsigned vo = voff_a0 + (unsigned)(t0 - p.pad) * pitch_x;
    unsigned char* dst = smem + (size_t)buf * buf_bytes + wave * 1024;
    for (int g = wave; g < ngroups; g += NT / 64) {
      ws_dma16(rx, vo, dst);
      vo += 16u * pitch_x; dst += 4096;
    }
  };

  // ---- state of the tile whose epilogue is pending
  unsigned pc[MW][8];                 // bf16 pairs of (acc + bias): pc[i][2g + h] = elements 4g + 2h, 4g + 2h + 1
  int p_b = 0, p_cls = 0, p_t0 = 0, p_Tc = 0, p_len = 0;
  __amdgpu_buffer_rsrc_t p_ru = ws_rsrc(p.y_act, 0, 0);      // output rows of the pending item (set at the hand-over)
  // ---- scratch of the micro-steps (live across MFMAs)
  float o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f, u0 = 0.f, u1 = 0.f, u2 = 0.f, u3 = 0.f, keepf = 1.f;
  unsigned h0 = 0, h1 = 0, rh = 0, up[8];
  int ty = 0;
  auto fbits = [](unsigned v) { return __builtin_bit_cast(float, v); };
  auto epi = [&](auto M) {           // micro-step M of the pending epilogue (M is a compile-time constant)
    constexpr int m = decltype(M)::value;
    constexpr int i = m / PH_ROW, rem = m % PH_ROW;
    if constexpr (rem < 4 * PH_UNIT) {
      constexpr int g = rem / PH_UNIT, ph = rem % PH_UNIT;
      if constexpr (ph == 0) {
        if constexpr (g == 0) {
          const int tc = p_t0 + 32 * i + r;
          ty = (tc < p_Tc) ? p_cls + rs * tc : -1;
          keepf = (ty >= p_len) ? 0.f : 1.f;
          rh = (unsigned)((((unsigned long long)p_b * p.Ty + (unsigned)max(ty, 0)) * (unsigned)p.site_width) >> 1);
        }
      } else if constexpr (ph == 1) {
        o0 = fbits(pc[i][2 * g] << 16) * keepf; o1 = fbits(pc[i][2 * g] & 0xffff0000u) * keepf;
      } else if constexpr (ph == 2) {
        o2 = fbits(pc[i][2 * g + 1] << 16) * keepf; o3 = fbits(pc[i][2 * g + 1] & 0xffff0000u) * keepf;
      } else if constexpr (ph == 3) {
        h0 = (rh + cshalf[g]) * 0x9E3779B1u + keyg[g]; h1 = h0 + 0x9E3779B1u;
      } else if constexpr (ph == 4) {
        h0 ^= h0 >> 16; h0 *= 0x85EBCA6Bu; h1 ^= h1 >> 16; h1 *= 0x85EBCA6Bu;
      } else if constexpr (ph == 5) {
        h0 ^= h0 >> 13; h0 *= 0xC2B2AE35u; h1 ^= h1 >> 13; h1 *= 0xC2B2AE35u;
      } else if constexpr (ph == 6) {
        h0 ^= h0 >> 16; h1 ^= h1 >> 16;
      } else if constexpr (ph == 7) {
        u0 = ((h0 & 0xFFFFu) >= p.drop_thresh16 && o0 > 0.f) ? o0 * p.drop_scale : 0.f;
      } else if constexpr (ph == 8) {
        u1 = ((h0 >> 16) >= p.drop_thresh16 && o1 > 0.f) ? o1 * p.drop_scale : 0.f;
      } else if constexpr (ph == 9) {
        u2 = ((h1 & 0xFFFFu) >= p.drop_thresh16 && o2 > 0.f) ? o2 * p.drop_scale : 0.f;
      } else if constexpr (ph == 10) {
        u3 = ((h1 >> 16) >= p.drop_thresh16 && o3 > 0.f) ? o3 * p.drop_scale : 0.f;
      } else {
        up[2 * g] = pack_bf16x2(u0, u1); up[2 * g + 1] = pack_bf16x2(u2, u3);
      }
    } else if constexpr (rem == 4 * PH_UNIT) {
      pair_up8(up);
    } else {
      if (ty >= 0) {      // 32-bit offset from the pending item's base (a scalar); the V# covers the whole output tensor
        store_paired(up, p_ru, (unsigned)ty * ((unsigned)p.ldya * 2u) + (unsigned)hh * 16u);
      }
    }
  };

  stage_a(tile_begin, 0);
  vm_wait<0>();
  // the wave index as a SCALAR for what goes into descriptors and LDS bases (a per-lane value there puts the descriptor in
  // VGPRs and a waterfall loop around every instruction that uses it)
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
#pragma unroll
  for (int i = 0; i < MW; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) pc[i][e] = 0;
  for (int tile = tile_begin; tile < tile_end; ++tile) {
    const int buf = (tile - tile_begin) & 1;
    int b, cls, t0;
    decode(tile, b, cls, t0);
    WS_T(c0);
    __syncthreads();                 // tile `tile` is in LDS for every wave; every wave is done with the other buffer
    WS_T(c1);
    // The next tile's input pieces go out behind the first MFMA of every second k-step (as in conv_ws_kernel<.., 2>: one
    // burst here cost 105-155 cycles of issue time per piece, profiles/dma_placement_phases.txt); descriptor, lens_in[b]
    // and the per-lane offset are ready before the loop.  No next tile: n_in = 0 skips every piece.
    __amdgpu_buffer_rsrc_t rx_n = ws_rsrc(p.x, 0, 0);
    unsigned vo_in = 0;
    int n_in = 0;
    if (tile + 1 < tile_end) {
      int nb, ncls, nt0;
      decode(tile + 1, nb, ncls, nt0);
      const int len_full = p.lens_in ? min(scalar_load_i32(p.lens_in + nb), p.Tin) : p.Tin;
      const int len_in = max(0, (len_full - ncls + rs - 1) / rs);
      rx_n = ws_rsrc(p.x, ((long long)nb * p.x_bs + (long long)ncls * p.ldx) * 2, (unsigned)len_in * pitch_x);
      vo_in = voff_a0 + (unsigned)(nt0 - p.pad) * pitch_x;
      n_in = ngroups;
    }
    unsigned char* const dst_in = smem + (size_t)(buf ^ 1) * buf_bytes + wave_s * 1024;
    constexpr int WS_IN_SLOTS = 12, WS_IN_EVERY = 2;      // 12 pieces = 192 rows, more than the LDS budget of the plan allows
    static_assert(WS_IN_SLOTS * WS_IN_EVERY <= NSTEP, "the pieces fit the tap loop");
    WS_T(c2);

    f32x16 acc[MW];
#pragma unroll
    for (int i = 0; i < MW; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    const unsigned abase = lds_base + (unsigned)buf * (unsigned)buf_bytes;
    unsigned tap_base[NTAPS];
#pragma unroll
    for (int s = 0; s < NTAPS; ++s) tap_base[s] = ws_tap_base(abase, r + s * p.dil, hh);
    auto frag_addr = [&](int q) -> unsigned { return ws_frag_addr(tap_base, q); };
    bf16x8 afr[2][MW];

    // the MFMA pipeline of conv_ws_kernel with micro-step 4q + i of the pending epilogue behind MFMA (q, i).  (The
    // first tile runs the micro-steps on an empty pending tile -- p_Tc = 0 suppresses its stores -- so that there is
    // ONE copy of the loop: with two, the allocator no longer keeps the pinned weights in AccVGPRs.)
    ws_read_frags(afr[0], frag_addr(0));
    static_for<0, NSTEP>([&](auto Q) {
      constexpr int q = decltype(Q)::value;
      if constexpr (q + 1 < NSTEP) {
        ws_read_frags(afr[(q + 1) & 1], frag_addr(q + 1));
        lgkm_wait<MW>();
      } else {
        lgkm_wait<0>();
      }
      static_for<0, MW>([&](auto I) {
        constexpr int i = decltype(I)::value;
        if constexpr (q == 0) ws_first_use(acc[i]);
        ws_mfma(acc[i], wfrag[q / (KC / 16)][q % (KC / 16)], afr[q & 1][i], q / (KC / 16) < AGPR_TAPS);
        if constexpr (i == 0 && q % WS_IN_EVERY == 0 && q / WS_IN_EVERY < WS_IN_SLOTS) {
          constexpr int j = q / WS_IN_EVERY;
          __builtin_amdgcn_sched_barrier(0);
          if (wave_s + 4 * j < n_in) ws_dma16(rx_n, vo_in + (unsigned)(16 * j) * pitch_x, dst_in + j * 4096);
          __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (4 * q + i < PH_TILE) {
          __builtin_amdgcn_sched_barrier(0);
          epi(std::integral_constant<int, 4 * q + i>{});
          __builtin_amdgcn_sched_barrier(0);
        }
      });
    });
    static_for<(NGAP < PH_TILE ? NGAP : PH_TILE), PH_TILE>(epi);   // micro-steps that did not fit behind this tile's MFMAs
    ws_drain(acc);
    WS_T(c5);
    vm_wait<0>();                                       // next tile has landed; older stores retired
    WS_T(c6);
    // hand the tile over: y = bf16(acc + bias), packed
#pragma unroll
    for (int i = 0; i < MW; ++i)
#pragma unroll
      for (int e = 0; e < 16; e += 2) pc[i][e >> 1] = pack_bf16x2(acc[i][e] + bval[e], acc[i][e + 1] + bval[e + 1]);
    p_b = b; p_cls = cls; p_t0 = t0;
    p_ru = ws_rsrc(p.y_act, ((long long)b * p.ya_bs + n0 + wave_s * 32) * 2, (unsigned)p.Ty * ((unsigned)p.ldya * 2u));
    p_Tc = (p.Tout - cls + rs - 1) / rs;
    p_len = p.lens_out ? scalar_load_i32(p.lens_out + b) : 0x7fffffff;
    WS_T(c7);
    WS_ACC(0, c0, c1); WS_ACC(1, c1, c2); WS_ACC(4, c2, c5); WS_ACC(5, c5, c6); WS_ACC(6, c6, c7); WS_ACC(7, c0, c0 + 1);
  }
  static_for<0, PH_TILE>(epi);                          // epilogue of the last tile
}

// ------------------------------------------------------------------------------------------------
// Weight-stationary kernel with TWO waves per SIMD (3 and 5 taps: 96 / 160 weight registers per wave leave room for a
// second wave in the 512-entry register file).  conv_ws_kernel runs one wave per SIMD, and a wave issues in order: its
// epilogue (VALU), its LDS-DMA issue and its barrier wait are all serial with its own MFMAs -- at 3 taps the matrix pipe
// is busy 30 % of the time (profiles/r02_pmc_mfma.txt).  Here a 512-thread workgroup splits the 128-row tile into two
// 64-row halves: waves w and w + 4 share a SIMD, own the SAME 32 output channels (both hold that weight slice) and
// different halves of the rows.  The two run the same program with one barrier per tile, but STAGGERED
// (MI355X_MICROARCH.md, "Two waves per SIMD", item 9): waves 0-3 multiply tile n and then write it out, waves 4-7 first
// write out tile n-1 (its sums stay in the accumulators across the barrier) and then multiply tile n -- so on every SIMD
// one wave's MFMA segment always sits beside its partner's epilogue segment (matrix beside VALU / memory, the pairing
// that nets).  Same arithmetic per output as conv_ws_kernel: bit-identical results.
// MODE 1 = activated output only (K2 forward), 2 = y with activation-gradient mask and residual (K2 data gradient).
constexpr int WS2_NT = 512;
// conv_ws2_kernel is dispatched up to this tap count.  Five taps compile (4 taps in AccVGPRs + 1 in VGPRs) but spill 7-24
// registers to scratch in the epilogue and run slower than the one-wave kernels (r03: 638 vs 490 us at the top level).
constexpr int WS2_MAX_TAPS = 3;

template <int NTAPS, int MODE>
__global__ __launch_bounds__(WS2_NT) void conv_ws2_kernel(ConvArgs p, const __bf16* __restrict__ zero_page,
                                                          int tiles_per_wg, int buf_bytes) {
  constexpr int BM = WS_BM, BN = WS_BN, KC = WS_KC, MW = 2, ROWB = WS_ROWB;
  constexpr int NSTEP = NTAPS * (KC / 16), NG = 5;          // NG: 4-row staging groups per wave (<= 160 rows per tile)
  static_assert(MODE == 1 || MODE == 2, "two epilogues");
  // Register budget at two waves per SIMD: 256 per lane, which the compiler splits 128 AccVGPRs / 128 VGPRs as soon as a
  // kernel names AccVGPRs (telling it to take 160 through an "a159" clobber leaves the VGPR side at 128 and the kernel
  // at one wave per SIMD): four taps (128 registers) are pinned there, a fifth lives in VGPRs, and what else is live
  // (32 accumulators, 24 fragment registers, offsets) has to fit beside it -- the bias values come from LDS for that.
  constexpr int AGPR_TAPS = NTAPS < 4 ? NTAPS : 4;
  static_assert(NTAPS <= 5, "weights of more than five taps do not fit two waves per SIMD");
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cw = wave & 3, rhalf = wave >> 2;              // column group (32 output channels), row half = phase
  const int r = lane & 31, hh = lane >> 5;
  const int n0 = blockIdx.y * BN;
  const int rs = p.rs;

  int wg, tile_begin, tile_end;
  if (!wg_tile_run(p.tiles_per_batch * p.B * rs, tiles_per_wg, wg, tile_begin, tile_end)) return;

  // fp32 bias of the 128 output channels, then (MODE 2) the epilogue-operand slices: per wave [64 rows][64 B] (its 32
  // channels of its row half), 16-byte chunks swizzled
  float* lds_bias = reinterpret_cast<float*>(smem + 2 * (size_t)buf_bytes);
  unsigned char* lds_res = smem + 2 * (size_t)buf_bytes + 1024 + wave * (WS_EPI / 8);
  unsigned char* lds_act = lds_res + WS_EPI;
  const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
  if (tid < BN) lds_bias[tid] = p.bias ? p.bias[n0 + tid] : 0.f;       // visible after the first barrier of the tile loop

  bf16x8 wfrag[NTAPS][KC / 16];
  {
    const int co = n0 + cw * 32 + r;
#pragma unroll
    for (int s = 0; s < NTAPS; ++s) {
      const unsigned char* wrow = reinterpret_cast<const unsigned char*>(p.w) + ((size_t)s * p.Cout + co) * ROWB;
#pragma unroll
      for (int kk = 0; kk < KC / 16; ++kk)
        wfrag[s][kk] = ws_wfrag(wrow, kk, hh, co);
    }
  }
  // accumulator element 4g + k of a lane = output channel col0 + 8g + k (this lane's row: 64 rhalf + 32 i + r)
  const int col0 = n0 + cw * 32 + 4 * hh;
  // dropout (MODE 1): hash input of the pair (row, col0 + 8g + 2j ..+1) = rowh + kc[g] + j C, with
  // rowh = ((b Ty + ty) site_width / 2) C (mod 2^32) = scalar part + lane part, kc[g] = (column / 2) C + key
  const unsigned HC = 0x9E3779B1u;
  const unsigned swh = (unsigned)p.site_width >> 1;
  unsigned kc[4];
  unsigned rowh_lane = 0;
  const unsigned thr_m1 = (p.drop_thresh16 - 1u) * 0x00010001u;
  if (MODE == 1) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int col = col0 + 8 * g;
      const int site = col / p.site_width;
      kc[g] = ((unsigned)(col - site * p.site_width) >> 1) * HC + site_key(p, site);
    }
    rowh_lane = HC * swh * (unsigned)(rs * r);
  }
  const int rows_in = BM + (NTAPS - 1) * p.dil;
  const int ngroups = (rows_in + 3) >> 2;

  // ---- byte pitches of the class-domain rows and the tile-invariant per-lane offsets
  const unsigned pitch_x = (unsigned)p.ldx * rs * 2u;
  unsigned voff_a[NG];
#pragma unroll
  for (int j = 0; j < NG; ++j) {
    const int row = 4 * (wave + 8 * j) + (lane >> 4);
    voff_a[j] = (unsigned)row * pitch_x + (unsigned)(((lane & 15) ^ swz256_row(row)) << 4);
  }
  const unsigned pitch_o = (MODE == 2 ? (unsigned)p.ldy : (unsigned)p.ldya) * rs * 2u;    // output rows
  const unsigned voff_o = (unsigned)(64 * rhalf + r) * pitch_o + (unsigned)hh * 16u;      // row block i: + 32 i pitch_o
  const unsigned pitch_r = (unsigned)p.ldr * rs * 2u, pitch_g = (unsigned)p.ldgh * rs * 2u;
  const int elr = 64 * rhalf + (lane >> 2);                                                 // + 16 q: staged row of the slices
  const unsigned echunk = (unsigned)(((lane & 3) ^ ((lane >> 4) & 3)) << 4);                // chunk (lane & 3) ^ ((row >> 2) & 3)

  auto decode = [&](int tile, int& b, int& cls, int& t0) { ws_decode(p.tiles_per_batch, rs, tile, b, cls, t0); };
  auto stage_a = [&](int tile, int buf) {
    int b, cls, t0;
    decode(tile, b, cls, t0);
    const int len_full = p.lens_in ? min(scalar_load_i32(p.lens_in + b), p.Tin) : p.Tin;
    const int len_in = max(0, (len_full - cls + rs - 1) / rs);
    const __amdgpu_buffer_rsrc_t rx = ws_rsrc(p.x, ((long long)b * p.x_bs + (long long)cls * p.ldx) * 2, (unsigned)len_in * pitch_x);
    const unsigned s0 = (unsigned)(t0 - p.pad) * pitch_x;       // rows before the item wrap to huge offsets: out of range, zero
    unsigned char* dst = smem + (size_t)buf * buf_bytes + wave * 1024;
#pragma unroll
    for (int j = 0; j < NG; ++j)
      if (wave + 8 * j < ngroups) ws_dma16(rx, voff_a[j] + s0, dst + j * 8192);
  };
  // this wave's slice of an epilogue operand: one DMA instruction = 16 rows x 64 B; slot c of local row n holds the
  // 16-byte chunk c ^ ((n >> 2) & 3) of the slice
  auto stage_epi = [&](const void* base, long long bs, int ld, unsigned pitch, int b, int cls, int t0, int Tc, unsigned char* dst) {
    const __amdgpu_buffer_rsrc_t re = ws_rsrc(base, ((long long)b * bs + (long long)cls * ld + n0 + cw * 32) * 2, (unsigned)Tc * pitch);
#pragma unroll
    for (int q = 0; q < 4; ++q) ws_dma16(re, (unsigned)(t0 + elr + 16 * q) * pitch + echunk, dst + q * 1024);
  };

  f32x16 acc[MW];
  // ---- epilogue of one tile half straight from the accumulators (the arithmetic of conv_ws_kernel, written for few VALU
  //      instructions: the epilogue, not the matrix pipe, bounds this kernel at 3 taps)
  auto epilogue = [&](int b, int cls, int t0, int Tc) {
    const int len_out = p.lens_out ? scalar_load_i32(p.lens_out + b) : 0x7fffffff;
    const __amdgpu_buffer_rsrc_t ry =
        MODE == 2 ? ws_rsrc(p.y, ((long long)b * p.y_bs + (long long)cls * p.ldy + n0 + cw * 32) * 2, (unsigned)Tc * pitch_o)
                  : ws_rsrc(p.y_act, ((long long)b * p.ya_bs + (long long)cls * p.ldya + n0 + cw * 32) * 2, (unsigned)Tc * pitch_o);
    const unsigned so = (unsigned)t0 * pitch_o;
    const unsigned rowh_s = MODE == 1 ? HC * swh * ((unsigned)b * (unsigned)p.Ty + (unsigned)cls + (unsigned)rs * (unsigned)(t0 + 64 * rhalf)) : 0u;
#pragma unroll
    for (int i = 0; i < MW; ++i) {
      const int lr = 32 * i + r;                                // row inside this wave's half
      const int ty = cls + rs * (t0 + 64 * rhalf + lr);         // actual output row
      const float srow = (ty >= len_out) ? 0.f : p.drop_scale;  // row mask and 1 / (1 - p) in one factor
      const int swz = (lr >> 2) & 3;
      unsigned yp[8];
      const unsigned rowh = rowh_s + rowh_lane + HC * swh * (unsigned)(rs * 32 * i);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(lds_bias + cw * 32 + 4 * hh + 8 * g);
        unsigned uvp[2] = {0, 0}, rvp[2] = {0, 0};
        if (MODE == 2) {
          const int eoff = lr * 64 + ((g ^ swz) << 4) + 8 * hh;
          const uint2 uv = *reinterpret_cast<const uint2*>(lds_act + eoff);
          const uint2 rv = *reinterpret_cast<const uint2*>(lds_res + eoff);
          uvp[0] = uv.x; uvp[1] = uv.y; rvp[0] = rv.x; rvp[1] = rv.y;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          // y = bf16(acc + bias), two elements per conversion
          const unsigned ypk = pack_bf16x2(acc[i][4 * g + 2 * j] + bv[2 * j], acc[i][4 * g + 2 * j + 1] + bv[2 * j + 1]);
          const float o0 = __builtin_bit_cast(float, ypk << 16), o1 = __builtin_bit_cast(float, ypk & 0xffff0000u);
          if (MODE == 1) {
            // u = relu(dropout(y)): scale (row mask folded in), round, relu + keep mask on the packed pair
            unsigned w = pk_relu_bf16(pack_bf16x2(o0 * srow, o1 * srow));
            if (p.drop_thresh16) w &= pk_keep_mask(fmix32(rowh + kc[g] + (unsigned)j * HC), thr_m1);
            yp[2 * g + j] = w;
          } else {
            // dx = y * scale * [u != 0] * row mask + residual
            const unsigned u2 = uvp[j], r2 = rvp[j];
            const float v0 = (u2 & 0x7fffu) ? o0 * srow : 0.f, v1 = (u2 & 0x7fff0000u) ? o1 * srow : 0.f;
            yp[2 * g + j] = pack_bf16x2(v0 + __builtin_bit_cast(float, r2 << 16), v1 + __builtin_bit_cast(float, r2 & 0xffff0000u));
          }
        }
      }
      // lanes r and r + 32 hold channels {0-3, 8-11, 16-19, 24-27} and {4-7, 12-15, 20-23, 28-31} of the same
      // row: swap so that lane r owns 0-7 | 16-23 and lane r + 32 owns 8-15 | 24-31 (16-byte pieces)
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          auto sw = __builtin_amdgcn_permlane32_swap(yp[4 * h2 + d], yp[4 * h2 + 2 + d], false, false);
          yp[4 * h2 + d] = sw[0]; yp[4 * h2 + 2 + d] = sw[1];
        }
      store_paired(yp, ry, voff_o + so + (unsigned)(32 * i) * pitch_o);    // rows >= Tc are out of range: dropped by the hardware
    }
  };

  stage_a(tile_begin, 0);
  vm_wait<0>();
  int pb = 0, pcls = 0, pt0 = 0, pTc = 0;        // the tile whose sums waves 4-7 still hold
  for (int tile = tile_begin; tile < tile_end; ++tile) {
    const int buf = (tile - tile_begin) & 1;
    int b, cls, t0;
    decode(tile, b, cls, t0);
    const int Tc = (p.Tout - cls + rs - 1) / rs;
    // tile `tile` is in LDS for every wave (each waited for its own DMAs before arriving here) and every wave is done
    // reading the other buffer
    WS_T(c0);
    __syncthreads();
    WS_T(c1);
    if (tile + 1 < tile_end) stage_a(tile + 1, buf ^ 1);
    WS_T(c2);
    if (rhalf == 1 && tile > tile_begin) epilogue(pb, pcls, pt0, pTc);
    WS_T(c3);
    if (MODE == 2) {                         // this wave's slices are free: its previous epilogue is done
      stage_epi(p.res, p.res_bs, p.ldr, pitch_r, b, cls, t0, Tc, lds_res);
      stage_epi(p.gate_h, p.gh_bs, p.ldgh, pitch_g, b, cls, t0, Tc, lds_act);
    }
    WS_T(c4);
#pragma unroll
    for (int i = 0; i < MW; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
    // MFMA pipeline over the NTAPS x 8 k-steps: the fragments of step q + 2 are requested before the MFMAs of step q
    // (two MFMAs = 64 cycles per step would not cover the LDS latency with a distance of one)
    const unsigned abase = lds_base + (unsigned)buf * (unsigned)buf_bytes + (unsigned)(64 * rhalf) * ROWB;
    unsigned tap_base[NTAPS];
#pragma unroll
    for (int s = 0; s < NTAPS; ++s) {
      const int ar = r + s * p.dil;                 // rows ar + 32 i (+ 64 rhalf) share the swizzle term (ar & 15)
      tap_base[s] = abase + ar * ROWB + ((hh ^ swz256_row(ar)) << 4);
    }
    auto frag_addr = [&](int q) -> unsigned { return ws_frag_addr(tap_base, q); };
    bf16x8 afr[3][MW];
#pragma unroll
    for (int q0 = 0; q0 < 2; ++q0) {
      const unsigned ap = frag_addr(q0);          // (a named temporary here and below: folded into the call, the MODE 2 kernel compiles differently)
      ws_read_frags(afr[q0], ap);
    }
    static_for<0, NSTEP>([&](auto Q) {
      constexpr int q = decltype(Q)::value;
      if constexpr (q + 2 < NSTEP) {
        const unsigned ap = frag_addr(q + 2);
        ws_read_frags(afr[(q + 2) % 3], ap);
        lgkm_wait<2 * MW>();                    // steps q + 1 and q + 2 in flight
      } else if constexpr (q + 1 < NSTEP) {
        lgkm_wait<MW>();
      } else {
        lgkm_wait<0>();
      }
      static_assert(MW == 2, "two accumulators per wave");
      if constexpr (q == 0) ws_first_use(acc[0], acc[1]);
      ws_mfma(acc[0], wfrag[q / (KC / 16)][q % (KC / 16)], afr[q % 3][0], q / (KC / 16) < AGPR_TAPS);
      ws_mfma(acc[1], wfrag[q / (KC / 16)][q % (KC / 16)], afr[q % 3][1], q / (KC / 16) < AGPR_TAPS);
    });
    ws_drain(acc);
    WS_T(c5);
    // next tile + this tile's epilogue operands have landed; older stores retired
    vm_wait<0>();
    WS_T(c6);
    if (rhalf == 0) epilogue(b, cls, t0, Tc);
    WS_T(c7);
    WS_ACC(0, c0, c1); WS_ACC(1, c1, c2); WS_ACC(2, c2, c3); WS_ACC(3, c3, c4); WS_ACC(4, c4, c5); WS_ACC(5, c5, c6);
    WS_ACC(6, c6, c7); WS_ACC(7, c0, c0 + 1);
    pb = b; pcls = cls; pt0 = t0; pTc = Tc;
  }
  if (rhalf == 1) epilogue(pb, pcls, pt0, pTc);
}

// ---- host side: eligibility and plan, the one variant rule, launch --------------------------------------------------
#ifndef SMT_WS_AB
#define SMT_WS_AB 0   // A/B build (tools/ablate_ws.sh): SMT_CONV_NO_WS2 / SMT_CONV_NO_PIPE and the kernels only they can reach
#endif

// tiles a launch must have for the persistent weight-stationary kernel (it loads the weight block once per workgroup)
static int ws_min_tiles() {
  static const int v = getenv("SMT_WS_MIN_TILES") ? atoi(getenv("SMT_WS_MIN_TILES")) : 512;
  return v;
}

// 128 input channels, odd tap counts 3..9, enough tiles per workgroup
bool plan_conv_ws(ConvArgs& p, WsPlan& pl) {
  static const bool no_ws = getenv("SMT_CONV_NO_WS") != nullptr;
  const int tc_max = (p.Tout + p.rs - 1) / p.rs;
  const int rows_pad = (WS_BM + (p.taps - 1) * p.dil + 3) & ~3;
  const int buf_bytes = (int)align_up((size_t)std::max(rows_pad * 256, WS_BM * (WS_BN + 8) * 2), 1024);
  const size_t lds = 2 * (size_t)buf_bytes + 2 * WS_EPI;
  const int tpb = (tc_max + WS_BM - 1) / WS_BM;
  const long long ntiles = (long long)tpb * p.B * p.rs;
  if (no_ws || p.Cin != 128 || p.taps < 3 || p.taps > 9 || !(p.taps & 1) || lds > 160 * 1024 || ntiles < ws_min_tiles()) return false;
  p.tiles_per_batch = tpb;
  const int nwg = 256;
  pl.buf_bytes = buf_bytes; pl.lds = lds;
  pl.tiles_per_wg = (int)((ntiles + nwg - 1) / nwg);
  pl.grid = dim3((unsigned)nwg, (unsigned)(p.Cout / WS_BN));
  return true;
}

// The one variant rule (launch_conv_ws and conv_ws_variant_name both use it): two waves per SIMD up to WS2_MAX_TAPS for the
// two epilogues of the GatedHiFi block; above that the pipelined kernel for the activated-output epilogue (K2 forward), the
// MODE 2 kernel for the data gradient; the generic epilogue for everything else.
enum WsVariant { WS2_FWD, WS2_DGRAD, WS_PIPE, WS_MODE1, WS_MODE2, WS_GENERIC };
static WsVariant ws_variant(const ConvArgs& p) {
  const bool y = p.y != nullptr, ao = p.act_out != 0, res = p.res != nullptr, ea = p.epi_act != 0;
  const bool fwd = !y && ao && !res && !ea, dgrad = y && !ao && res && ea;
#if SMT_WS_AB
  static const bool no_ws2 = getenv("SMT_CONV_NO_WS2") != nullptr, no_pipe = getenv("SMT_CONV_NO_PIPE") != nullptr;
#else
  constexpr bool no_ws2 = false, no_pipe = false;
#endif
  if (p.taps <= WS2_MAX_TAPS && !no_ws2 && (fwd || dgrad)) return fwd ? WS2_FWD : WS2_DGRAD;
  if (fwd) return no_pipe ? WS_MODE1 : WS_PIPE;
  return dgrad ? WS_MODE2 : WS_GENERIC;
}

const char* conv_ws_variant_name(const ConvArgs& p) {
  switch (ws_variant(p)) {
    case WS2_FWD: case WS2_DGRAD: return "conv_ws2";
    case WS_PIPE: return "conv_ws_pipe";
    default: return "conv_ws";
  }
}

template <typename K>
static void launch_ws_kernel(K kernel, int nt, size_t lds, const ConvArgs& p, const WsPlan& pl, const void* zero_page, hipStream_t stream) {
  (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  kernel<<<pl.grid, nt, lds, stream>>>(p, (const __bf16*)zero_page, pl.tiles_per_wg, pl.buf_bytes);
}

// Only the variants that ws_variant can return for NTAPS are instantiated: without SMT_WS_AB the two-wave kernels take both
// epilogues up to WS2_MAX_TAPS and the pipelined kernel always takes the forward.
template <int NTAPS>
static void launch_ws(const ConvArgs& p, const WsPlan& pl, const void* zero_page, hipStream_t stream) {
  constexpr bool ws2 = NTAPS <= WS2_MAX_TAPS, one_wave = SMT_WS_AB || !ws2;
  const WsVariant v = ws_variant(p);
  if constexpr (ws2) {
    // (the forward needs no epilogue-operand tiles)
    if (v == WS2_FWD) return launch_ws_kernel(conv_ws2_kernel<NTAPS, 1>, WS2_NT, 2 * (size_t)pl.buf_bytes + 1024, p, pl, zero_page, stream);
    if (v == WS2_DGRAD) return launch_ws_kernel(conv_ws2_kernel<NTAPS, 2>, WS2_NT, pl.lds + 1024, p, pl, zero_page, stream);
  }
  if constexpr (one_wave) {
    if (v == WS_PIPE) return launch_ws_kernel(conv_ws_pipe_kernel<NTAPS>, WS_NT, pl.lds, p, pl, zero_page, stream);
    if (v == WS_MODE2) return launch_ws_kernel(conv_ws_kernel<NTAPS, 2>, WS_NT, pl.lds, p, pl, zero_page, stream);
  }
  if constexpr (SMT_WS_AB) {
    if (v == WS_MODE1) return launch_ws_kernel(conv_ws_kernel<NTAPS, 1>, WS_NT, pl.lds, p, pl, zero_page, stream);
  }
  launch_ws_kernel(conv_ws_kernel<NTAPS, 0>, WS_NT, pl.lds, p, pl, zero_page, stream);
}

void launch_conv_ws(const ConvArgs& p, const WsPlan& pl, const void* zero_page, hipStream_t stream) {
  switch (p.taps) {
    case 3: return launch_ws<3>(p, pl, zero_page, stream);
    case 5: return launch_ws<5>(p, pl, zero_page, stream);
    case 7: return launch_ws<7>(p, pl, zero_page, stream);
    default: return launch_ws<9>(p, pl, zero_page, stream);
  }
}

}  // namespace smt

using namespace smt;

#if SMT_WS_STAMP
extern "C" int smt_ws_debug_dump(unsigned long long* host, int n, int reset) {
  int rc = (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(ws_dbg), sizeof(unsigned long long) * n);
  if (reset) { static unsigned long long z[256 * 8 * 8]; rc |= (int)hipMemcpyToSymbol(HIP_SYMBOL(ws_dbg), z, sizeof(z)); }
  return rc;
}
#endif
