// Pieces shared by the convolution kernels: element traits, 16-byte vectors, counter-based dropout; the streaming
// kernels' building blocks are in conv_stream.h (included at the end).
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

// tile runs, V# addressing, untracked loads, counted waits, LDS layouts, lane pairing and stores of the streaming kernels
#include "conv_stream.h"
