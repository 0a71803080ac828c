// Dense projections of the TransformerLM with bf16 operands (include/smt_hip.h "TransformerLM", smt_lm_linear_*).
//   * lm_linear_nt_kernel     C[m, n] = bias[n] + sum_k bf16(A[m, k]) * B[n][k]: A fp32 rows with a pitch, B a packed bf16
//                             weight [N][K].  It is the forward (A = x, B = w [n_out][n_in]) and the data gradient (A = dy,
//                             B = the same weight packed [n_in][n_out]): both sum over the fast axis of both operands.
//   * lm_linear_wgrad_kernel  dW[o, i] = sum_r bf16(dy[r, o]) * bf16(x[r, i]): the sum runs over the slow axis of both
//                             operands, so the staging pass transposes: a thread loads an 8-row x 4-column piece (eight 16-byte
//                             loads), rounds it and writes four 16-byte k-runs, one per column.  After that both kernels read
//                             the same LDS image [row of the product][k] and share one MFMA loop.  The column sums of the
//                             UNROUNDED dy (dbias) fall out of the same registers.  The rows are split over `splits`
//                             workgroups per output tile; each writes a slab, lm_linear_reduce_kernel adds the slabs in
//                             slab order (no atomics: equal inputs give equal bits).
// Tile: 64 RM x 64 RN outputs per workgroup of 4 waves (2 x 2), 64 k per step, mfma_f32_32x32x16_bf16 with RM x RN
// accumulators per wave.  LDS rows are 64 bf16 + 8 of padding (144 bytes): the 16-byte fragment reads of 16 consecutive rows
// start 36 dwords apart and cover the 64 banks once.  The next k-step's global loads are issued before the MFMAs of the
// current one and written to LDS after them (one LDS buffer, two barriers per step).
// fp32 -> bf16 is the compiler's conversion (v_cvt_pk_bf16_f32, round to nearest even).  Row offsets are 64-bit.
#include <algorithm>

#include "conv_common.h"

namespace smt {

constexpr int LL_BK = 64;             // k per step
constexpr int LL_PITCH = LL_BK + 8;   // LDS row pitch in bf16 elements
constexpr int LL_THREADS = 256;

struct LlNtArgs {
  const float* a; long long ld_a;
  const __bf16* b;                    // [n][k], dense
  const float* bias;                  // [n] or NULL
  float* c; long long ld_c;
  long long m; int n, k;
};

__device__ __forceinline__ bf16x8 ll_round8(const float4& lo, const float4& hi) {
  return bf16x8{(__bf16)lo.x, (__bf16)lo.y, (__bf16)lo.z, (__bf16)lo.w, (__bf16)hi.x, (__bf16)hi.y, (__bf16)hi.z, (__bf16)hi.w};
}

// The MFMA loop over one staged k-step: wave (wm, wn) owns rows wm*32*RM.. of sa and rows wn*32*RN.. of sb.
template <int RM, int RN>
__device__ __forceinline__ void ll_mma_step(const __bf16* sa, const __bf16* sb, int wm, int wn, int lane, f32x16 (&acc)[RM][RN]) {
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int ks = 0; ks < LL_BK / 16; ++ks) {
    bf16x8 af[RM], bf[RN];
#pragma unroll
    for (int i = 0; i < RM; ++i) af[i] = *(const bf16x8*)(sa + (wm * 32 * RM + i * 32 + r) * LL_PITCH + ks * 16 + h * 8);
#pragma unroll
    for (int j = 0; j < RN; ++j) bf[j] = *(const bf16x8*)(sb + (wn * 32 * RN + j * 32 + r) * LL_PITCH + ks * 16 + h * 8);
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
      for (int j = 0; j < RN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
  }
}

// Store the accumulators: element (reg, lane) of acc[i][j] is row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), column lane & 31.
template <int RM, int RN>
__device__ __forceinline__ void ll_store(float* c, long long ld_c, long long m0, long long m_end, int n0, int n_end,
                                         const float* bias, int wm, int wn, int lane, const f32x16 (&acc)[RM][RN]) {
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int j = 0; j < RN; ++j) {
    const int col = n0 + wn * 32 * RN + j * 32 + r;
    if (col >= n_end) continue;
    const float bv = bias ? bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const long long row = m0 + wm * 32 * RM + i * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        if (row < m_end) c[row * ld_c + col] = acc[i][j][reg] + bv;
      }
  }
}

template <int RM, int RN>
__global__ __launch_bounds__(LL_THREADS) void lm_linear_nt_kernel(LlNtArgs p) {
  constexpr int BM = 64 * RM, BN = 64 * RN;
  constexpr int A_PER = BM * 8 / LL_THREADS, B_PER = BN * 8 / LL_THREADS;     // 8-element chunks per thread
  __shared__ __attribute__((aligned(16))) __bf16 lds[(BM + BN) * LL_PITCH];
  __bf16* sa = lds;
  __bf16* sb = lds + BM * LL_PITCH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const long long m0 = (long long)blockIdx.y * BM;
  const int n0 = blockIdx.x * BN;

  float4 ra[A_PER][2];
  uint4 rb[B_PER];
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
      const int c = tid + i * LL_THREADS, row = c >> 3, kk = k0 + (c & 7) * 8;
      const long long gr = m0 + row;
      if (gr < p.m && kk < p.k) {
        const float4* src = (const float4*)(p.a + gr * p.ld_a + kk);
        ra[i][0] = src[0];
        ra[i][1] = src[1];
      } else {
        ra[i][0] = float4{0.f, 0.f, 0.f, 0.f};
        ra[i][1] = float4{0.f, 0.f, 0.f, 0.f};
      }
    }
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
      const int c = tid + i * LL_THREADS, row = c >> 3, kk = k0 + (c & 7) * 8;
      const int gn = n0 + row;
      rb[i] = uint4{0u, 0u, 0u, 0u};
      if (gn < p.n && kk < p.k) rb[i] = *(const uint4*)(p.b + (long long)gn * p.k + kk);
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
      const int c = tid + i * LL_THREADS;
      *(bf16x8*)(sa + (c >> 3) * LL_PITCH + (c & 7) * 8) = ll_round8(ra[i][0], ra[i][1]);
    }
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
      const int c = tid + i * LL_THREADS;
      *(uint4*)(sb + (c >> 3) * LL_PITCH + (c & 7) * 8) = rb[i];
    }
  };

  f32x16 acc[RM][RN];
#pragma unroll
  for (int i = 0; i < RM; ++i)
#pragma unroll
    for (int j = 0; j < RN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  load(0);
  for (int k0 = 0; k0 < p.k; k0 += LL_BK) {
    stage();
    __syncthreads();
    if (k0 + LL_BK < p.k) load(k0 + LL_BK);
    ll_mma_step<RM, RN>(sa, sb, wm, wn, lane, acc);
    __syncthreads();
  }
  ll_store<RM, RN>(p.c, p.ld_c, m0, p.m, n0, p.n, p.bias, wm, wn, lane, acc);
}

struct LlWgArgs {
  const float* x; long long ld_x;
  const float* dy; long long ld_dy;
  float* out;                         // dweight (splits == 1) or the slabs [splits][n_out][n_in]
  float* out_bias;                    // dbias (splits == 1) or [splits][n_out]; NULL = not wanted
  long long rows; int n_in, n_out;
  int rows_per_split;                 // a multiple of LL_BK
};

// 128 x 128 outputs (o x i) per workgroup; blockIdx.z = the split (a run of rows_per_split rows).
__global__ __launch_bounds__(LL_THREADS) void lm_linear_wgrad_kernel(LlWgArgs p) {
  constexpr int BM = 128, BN = 128;
  __shared__ __attribute__((aligned(16))) __bf16 lds[(BM + BN) * LL_PITCH];
  __bf16* sa = lds;                   // [o][r]
  __bf16* sb = lds + BM * LL_PITCH;   // [i][r]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int o0 = blockIdx.y * BM, i0 = blockIdx.x * BN;
  const long long r_begin = (long long)blockIdx.z * p.rows_per_split;
  const long long r_end = r_begin + p.rows_per_split < p.rows ? r_begin + p.rows_per_split : p.rows;
  // thread -> rows 8 rg .. 8 rg + 7 of the step, columns 4 cg .. 4 cg + 3 of the tile: eight neighbouring lanes read one
  // 16-byte column piece of eight row groups and write one whole 128-byte LDS row
  const int rg = tid & 7, cg = tid >> 3;
  const bool o_in = o0 + cg * 4 < p.n_out, i_in = i0 + cg * 4 < p.n_in;

  float4 rdy[8], rx[8];
  float4 bsum = {0.f, 0.f, 0.f, 0.f};
  auto load = [&](long long r0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const long long r = r0 + rg * 8 + q;
      const bool in = r < r_end;
      rdy[q] = (in && o_in) ? *(const float4*)(p.dy + r * p.ld_dy + o0 + cg * 4) : float4{0.f, 0.f, 0.f, 0.f};
      rx[q] = (in && i_in) ? *(const float4*)(p.x + r * p.ld_x + i0 + cg * 4) : float4{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto stage = [&]() {
    __bf16* da = sa + (cg * 4) * LL_PITCH + rg * 8;
    __bf16* db = sb + (cg * 4) * LL_PITCH + rg * 8;
    *(bf16x8*)(da) = bf16x8{(__bf16)rdy[0].x, (__bf16)rdy[1].x, (__bf16)rdy[2].x, (__bf16)rdy[3].x,
                            (__bf16)rdy[4].x, (__bf16)rdy[5].x, (__bf16)rdy[6].x, (__bf16)rdy[7].x};
    *(bf16x8*)(da + LL_PITCH) = bf16x8{(__bf16)rdy[0].y, (__bf16)rdy[1].y, (__bf16)rdy[2].y, (__bf16)rdy[3].y,
                                       (__bf16)rdy[4].y, (__bf16)rdy[5].y, (__bf16)rdy[6].y, (__bf16)rdy[7].y};
    *(bf16x8*)(da + 2 * LL_PITCH) = bf16x8{(__bf16)rdy[0].z, (__bf16)rdy[1].z, (__bf16)rdy[2].z, (__bf16)rdy[3].z,
                                           (__bf16)rdy[4].z, (__bf16)rdy[5].z, (__bf16)rdy[6].z, (__bf16)rdy[7].z};
    *(bf16x8*)(da + 3 * LL_PITCH) = bf16x8{(__bf16)rdy[0].w, (__bf16)rdy[1].w, (__bf16)rdy[2].w, (__bf16)rdy[3].w,
                                           (__bf16)rdy[4].w, (__bf16)rdy[5].w, (__bf16)rdy[6].w, (__bf16)rdy[7].w};
    *(bf16x8*)(db) = bf16x8{(__bf16)rx[0].x, (__bf16)rx[1].x, (__bf16)rx[2].x, (__bf16)rx[3].x,
                            (__bf16)rx[4].x, (__bf16)rx[5].x, (__bf16)rx[6].x, (__bf16)rx[7].x};
    *(bf16x8*)(db + LL_PITCH) = bf16x8{(__bf16)rx[0].y, (__bf16)rx[1].y, (__bf16)rx[2].y, (__bf16)rx[3].y,
                                       (__bf16)rx[4].y, (__bf16)rx[5].y, (__bf16)rx[6].y, (__bf16)rx[7].y};
    *(bf16x8*)(db + 2 * LL_PITCH) = bf16x8{(__bf16)rx[0].z, (__bf16)rx[1].z, (__bf16)rx[2].z, (__bf16)rx[3].z,
                                           (__bf16)rx[4].z, (__bf16)rx[5].z, (__bf16)rx[6].z, (__bf16)rx[7].z};
    *(bf16x8*)(db + 3 * LL_PITCH) = bf16x8{(__bf16)rx[0].w, (__bf16)rx[1].w, (__bf16)rx[2].w, (__bf16)rx[3].w,
                                           (__bf16)rx[4].w, (__bf16)rx[5].w, (__bf16)rx[6].w, (__bf16)rx[7].w};
#pragma unroll
    for (int q = 0; q < 8; ++q) {     // rows in ascending order: a fixed order of additions
      bsum.x += rdy[q].x; bsum.y += rdy[q].y; bsum.z += rdy[q].z; bsum.w += rdy[q].w;
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  load(r_begin);
  for (long long r0 = r_begin; r0 < r_end; r0 += LL_BK) {
    stage();
    __syncthreads();
    if (r0 + LL_BK < r_end) load(r0 + LL_BK);
    ll_mma_step<2, 2>(sa, sb, wm, wn, lane, acc);
    __syncthreads();
  }
  const size_t slab = (size_t)blockIdx.z * p.n_out * p.n_in;
  ll_store<2, 2>(p.out + slab, p.n_in, o0, p.n_out, i0, p.n_in, nullptr, wm, wn, lane, acc);
  if (p.out_bias && blockIdx.x == 0) {          // uniform over the workgroup; the eight row groups are lanes 8 cg .. 8 cg + 7
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
      bsum.x += __shfl_xor(bsum.x, o, 64); bsum.y += __shfl_xor(bsum.y, o, 64);
      bsum.z += __shfl_xor(bsum.z, o, 64); bsum.w += __shfl_xor(bsum.w, o, 64);
    }
    if (rg == 0 && o_in) *(float4*)(p.out_bias + (size_t)blockIdx.z * p.n_out + o0 + cg * 4) = bsum;
  }
}

// out[e] = slabs[0][e] + slabs[1][e] + ... in slab order, four elements per thread (n is a multiple of 4)
__global__ __launch_bounds__(256) void lm_linear_reduce_kernel(const float* slabs, float* out, long long n, int splits) {
  const long long e = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e >= n) return;
  float4 s = *(const float4*)(slabs + e);
  for (int k = 1; k < splits; ++k) {
    const float4 v = *(const float4*)(slabs + (long long)k * n + e);
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  *(float4*)(out + e) = s;
}

// ------------------------------------------------------------------------------------------------ host side
struct LlTensor { const char* name; const void* p; long long ld; int width; bool output; };

static bool ll_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}
static size_t ll_span(const LlTensor& t, long long rows) { return (size_t)((rows - 1) * t.ld + t.width) * sizeof(float); }

// The limits the three entries share, decided before any HIP call.  Returns 0 (go on) or 1 (argument error).
static int ll_check(const char* fn, const LlTensor* ts, int n, long long rows, int n_in, int n_out) {
  SMT_CHECK_ARG(n_in >= 32 && n_in % 32 == 0, "%s: n_in=%d must be a positive multiple of 32", fn, n_in);
  SMT_CHECK_ARG(n_out >= 16 && n_out % 16 == 0, "%s: n_out=%d must be a positive multiple of 16", fn, n_out);
  SMT_CHECK_ARG(rows >= 0, "%s: rows=%lld must not be negative", fn, rows);
  for (int i = 0; i < n; ++i) {
    const LlTensor& a = ts[i];
    SMT_CHECK_ARG(a.p != nullptr, "%s: null pointer (%s)", fn, a.name);
    SMT_CHECK_ARG(((uintptr_t)a.p & 15) == 0, "%s: %s must be 16-byte aligned", fn, a.name);
    SMT_CHECK_ARG(a.ld >= a.width, "%s: pitch ld_%s=%lld is smaller than the row width %d", fn, a.name, a.ld, a.width);
    SMT_CHECK_ARG(a.ld % 4 == 0, "%s: pitch ld_%s=%lld must be a multiple of 4 elements", fn, a.name, a.ld);
  }
  return 0;
}

static int ll_check_alias(const char* fn, const char* out_name, const void* out, size_t out_bytes, const char* in_name,
                          const void* in, size_t in_bytes) {
  SMT_CHECK_ARG(!ll_overlap(out, out_bytes, in, in_bytes), "%s: %s must not alias %s", fn, out_name, in_name);
  return 0;
}

// C[m, n] = A[m, k] B[n][k]^T: 128 x 128 tiles where they give every CU of the chip a workgroup, else 64 x 64
static void ll_launch_nt(const LlNtArgs& p, hipStream_t stream) {
  const long long big = ((p.m + 127) / 128) * ((p.n + 127) / 128);
  if (big >= 256) {
    lm_linear_nt_kernel<2, 2><<<dim3((p.n + 127) / 128, (unsigned)((p.m + 127) / 128)), LL_THREADS, 0, stream>>>(p);
  } else {
    lm_linear_nt_kernel<1, 1><<<dim3((p.n + 63) / 64, (unsigned)((p.m + 63) / 64)), LL_THREADS, 0, stream>>>(p);
  }
}

// splits of the rows per output tile: enough workgroups for the chip, at least one k-step each, at most 32 slabs
static int ll_wgrad_splits(long long rows, int n_in, int n_out) {
  const long long tiles = (long long)((n_in + 127) / 128) * ((n_out + 127) / 128);
  const long long steps = (rows + LL_BK - 1) / LL_BK;
  return (int)std::max<long long>(1, std::min<long long>({steps, (256 + tiles - 1) / tiles, 32}));
}

}  // namespace smt

using namespace smt;

extern "C" int smt_lm_linear_fwd(const float* x, int64_t ld_x, const void* w_packed, const float* bias, float* y, int64_t ld_y,
                                 int64_t rows, int n_in, int n_out, smt_stream_t stream_) {
  static const char* fn = "smt_lm_linear_fwd";
  const LlTensor ts[2] = {{"x", x, ld_x, n_in, false}, {"y", y, ld_y, n_out, true}};
  if (ll_check(fn, ts, 2, rows, n_in, n_out)) return 1;
  SMT_CHECK_ARG(w_packed != nullptr, "%s: null pointer (w_packed)", fn);
  SMT_CHECK_ARG(((uintptr_t)w_packed & 15) == 0, "%s: w_packed must be 16-byte aligned", fn);
  SMT_CHECK_ARG(bias == nullptr || ((uintptr_t)bias & 3) == 0, "%s: bias must be 4-byte aligned", fn);
  SMT_CHECK_ARG((rows + 127) / 128 <= 65535, "%s: rows=%lld exceeds 65535 row tiles", fn, (long long)rows);
  if (rows == 0) return 0;
  const size_t y_bytes = ll_span(ts[1], rows), w_bytes = (size_t)n_in * n_out * 2;
  if (ll_check_alias(fn, "y", y, y_bytes, "x", x, ll_span(ts[0], rows))) return 1;
  if (ll_check_alias(fn, "y", y, y_bytes, "w_packed", w_packed, w_bytes)) return 1;
  if (bias && ll_check_alias(fn, "y", y, y_bytes, "bias", bias, (size_t)n_out * 4)) return 1;
  ll_launch_nt(LlNtArgs{x, ld_x, (const __bf16*)w_packed, bias, y, ld_y, rows, n_out, n_in}, (hipStream_t)stream_);
  SMT_CHECK_LAUNCH(fn);
  return 0;
}

extern "C" int smt_lm_linear_dgrad(const float* dy, int64_t ld_dy, const void* w_packed_t, float* dx, int64_t ld_dx,
                                   int64_t rows, int n_in, int n_out, smt_stream_t stream_) {
  static const char* fn = "smt_lm_linear_dgrad";
  const LlTensor ts[2] = {{"dy", dy, ld_dy, n_out, false}, {"dx", dx, ld_dx, n_in, true}};
  if (ll_check(fn, ts, 2, rows, n_in, n_out)) return 1;
  SMT_CHECK_ARG(w_packed_t != nullptr, "%s: null pointer (w_packed_t)", fn);
  SMT_CHECK_ARG(((uintptr_t)w_packed_t & 15) == 0, "%s: w_packed_t must be 16-byte aligned", fn);
  SMT_CHECK_ARG((rows + 127) / 128 <= 65535, "%s: rows=%lld exceeds 65535 row tiles", fn, (long long)rows);
  if (rows == 0) return 0;
  const size_t dx_bytes = ll_span(ts[1], rows);
  if (ll_check_alias(fn, "dx", dx, dx_bytes, "dy", dy, ll_span(ts[0], rows))) return 1;
  if (ll_check_alias(fn, "dx", dx, dx_bytes, "w_packed_t", w_packed_t, (size_t)n_in * n_out * 2)) return 1;
  ll_launch_nt(LlNtArgs{dy, ld_dy, (const __bf16*)w_packed_t, nullptr, dx, ld_dx, rows, n_in, n_out}, (hipStream_t)stream_);
  SMT_CHECK_LAUNCH(fn);
  return 0;
}

extern "C" size_t smt_lm_linear_wgrad_workspace_bytes(int64_t rows, int n_in, int n_out) {
  if (rows <= 0 || n_in <= 0 || n_out <= 0) return 0;
  const int splits = ll_wgrad_splits(rows, n_in, n_out);
  return splits == 1 ? 0 : (size_t)splits * ((size_t)n_out * n_in + n_out) * sizeof(float);
}

extern "C" int smt_lm_linear_wgrad(const float* x, int64_t ld_x, const float* dy, int64_t ld_dy, float* dweight, float* dbias,
                                   int64_t rows, int n_in, int n_out, void* workspace, size_t workspace_bytes,
                                   smt_stream_t stream_) {
  static const char* fn = "smt_lm_linear_wgrad";
  const LlTensor ts[3] = {{"x", x, ld_x, n_in, false}, {"dy", dy, ld_dy, n_out, false}, {"dweight", dweight, n_in, n_in, true}};
  if (ll_check(fn, ts, 3, rows, n_in, n_out)) return 1;
  SMT_CHECK_ARG(dbias == nullptr || ((uintptr_t)dbias & 15) == 0, "%s: dbias must be 16-byte aligned", fn);
  const size_t dw_bytes = (size_t)n_out * n_in * 4, db_bytes = (size_t)n_out * 4;
  const size_t x_bytes = rows ? ll_span(ts[0], rows) : 0, dy_bytes = rows ? ll_span(ts[1], rows) : 0;
  // dweight on an input is named before dbias inside dweight: a dweight pointer that sits on x or dy spans n_out * n_in
  // floats from there, which may also cover a correctly placed dbias -- which of the two is reported must not depend on
  // where the caller's allocator put the buffers
  if (rows) {
    if (ll_check_alias(fn, "dweight", dweight, dw_bytes, "x", x, x_bytes)) return 1;
    if (ll_check_alias(fn, "dweight", dweight, dw_bytes, "dy", dy, dy_bytes)) return 1;
  }
  SMT_CHECK_ARG(dbias == nullptr || !ll_overlap(dbias, db_bytes, dweight, dw_bytes), "%s: dbias must not alias dweight", fn);
  hipStream_t stream = (hipStream_t)stream_;
  if (rows == 0) {                      // the sum over nothing
    if (hipMemsetAsync(dweight, 0, dw_bytes, stream) != hipSuccess || (dbias && hipMemsetAsync(dbias, 0, db_bytes, stream) != hipSuccess)) {
      set_error("%s: hipMemsetAsync failed", fn);
      return 2;
    }
    return 0;
  }
  if (dbias && ll_check_alias(fn, "dbias", dbias, db_bytes, "x", x, x_bytes)) return 1;
  if (dbias && ll_check_alias(fn, "dbias", dbias, db_bytes, "dy", dy, dy_bytes)) return 1;
  const int splits = ll_wgrad_splits(rows, n_in, n_out);
  const size_t need = smt_lm_linear_wgrad_workspace_bytes(rows, n_in, n_out);
  SMT_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %zu bytes is smaller than the %zu needed", fn, workspace_bytes, need);
  if (need) {
    SMT_CHECK_ARG(workspace != nullptr, "%s: null pointer (workspace)", fn);
    SMT_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "%s: workspace must be 16-byte aligned", fn);
    if (ll_check_alias(fn, "workspace", workspace, need, "x", x, x_bytes)) return 1;
    if (ll_check_alias(fn, "workspace", workspace, need, "dy", dy, dy_bytes)) return 1;
    if (ll_check_alias(fn, "workspace", workspace, need, "dweight", dweight, dw_bytes)) return 1;
    if (dbias && ll_check_alias(fn, "workspace", workspace, need, "dbias", dbias, db_bytes)) return 1;
  }
  const long long steps = (rows + LL_BK - 1) / LL_BK;
  const int rows_per_split = (int)((steps + splits - 1) / splits) * LL_BK;
  const int z = (int)((rows + rows_per_split - 1) / rows_per_split);          // every split holds at least one row
  float* slabs = (float*)workspace;
  float* bias_slabs = slabs + (size_t)splits * n_out * n_in;
  const bool direct = z == 1;
  LlWgArgs p{x, ld_x, dy, ld_dy, direct ? dweight : slabs, dbias ? (direct ? dbias : bias_slabs) : nullptr, rows, n_in, n_out,
             rows_per_split};
  lm_linear_wgrad_kernel<<<dim3((n_in + 127) / 128, (n_out + 127) / 128, z), LL_THREADS, 0, stream>>>(p);
  SMT_CHECK_LAUNCH(fn);
  if (!direct) {
    const long long n = (long long)n_out * n_in;
    lm_linear_reduce_kernel<<<(unsigned)((n / 4 + 255) / 256), 256, 0, stream>>>(slabs, dweight, n, z);
    SMT_CHECK_LAUNCH(fn);
    if (dbias) {
      // the bias slabs are [z][n_out] behind `splits` weight slabs: same kernel, slab stride n_out
      lm_linear_reduce_kernel<<<(n_out / 4 + 255) / 256, 256, 0, stream>>>(bias_slabs, dbias, n_out, z);
      SMT_CHECK_LAUNCH(fn);
    }
  }
  return 0;
}
