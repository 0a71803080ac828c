// VQTTS code emission (include/smt_hip.h, "VQTTS code emission"): the predicted relative code of every frame becomes the
// absolute code token * l_bins + pred and the frame's codebook row in one pass -- the synthesis side of the grouped
// bottleneck (reference models/vqtts/vqtts.py:170-174).  The kernel moves 2 * batch * t_q * dim * 4 bytes (each row read once, written once) and computes only
// indices, so the work is laid out for the memory system alone: one thread per 16 bytes of output, consecutive threads on
// consecutive 16-byte pieces of consecutive rows, so a wave is full whatever dim / 4 is and its stores are contiguous.
#include "smt_common.h"

namespace {

constexpr int EM_NT = 256;          // threads per workgroup: 256 * 16 B = 4 KiB of rows (16 rows at dim 64) per sweep
constexpr int EM_MAX_BLOCKS = 2048; // grid cap (256 CUs x 8 workgroups); the sweep is grid-strided past it

// The frame's code, or -1: j < q_lens[b], 0 <= idx < t_x, 0 <= token < n_vocab, 0 <= pred < l_bins.  x_id is read only
// with an index in range.
__device__ __forceinline__ long long em_code(const int* __restrict__ pred, const int64_t* __restrict__ x_id,
                                             const int* __restrict__ idx, const int* __restrict__ q_lens, long long row, int t_x,
                                             int t_q, int n_vocab, int l_bins) {
  const int b = (int)(row / t_q), j = (int)(row - (long long)b * t_q);
  if (j >= q_lens[b]) return -1;
  const int i = idx[row];
  if (i < 0 || i >= t_x) return -1;
  const long long tok = x_id[(size_t)b * t_x + i];
  if (tok < 0 || tok >= n_vocab) return -1;
  const int p = pred[row];
  if (p < 0 || p >= l_bins) return -1;
  return tok * l_bins + p;
}

__global__ __launch_bounds__(EM_NT) void em_emit_kernel(const int* __restrict__ pred, const int64_t* __restrict__ x_id,
                                                        const int* __restrict__ idx, const int* __restrict__ q_lens,
                                                        const smt::f32x4* __restrict__ codebook, long long rows, int t_x, int t_q,
                                                        int n_vocab, int l_bins, int dim4, int64_t* __restrict__ q_abs,
                                                        smt::f32x4* __restrict__ y_d) {
  const long long total = rows * dim4;
  for (long long e = (long long)blockIdx.x * EM_NT + threadIdx.x; e < total; e += (long long)gridDim.x * EM_NT) {
    const long long row = e / dim4;
    const int c = (int)(e - row * dim4);
    const long long q = em_code(pred, x_id, idx, q_lens, row, t_x, t_q, n_vocab, l_bins);
    smt::f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (q >= 0) v = codebook[(size_t)q * dim4 + c];
    y_d[e] = v;
    if (c == 0 && q_abs) q_abs[row] = q;
  }
}

}  // namespace

extern "C" int smt_vqtts_emit(const int* pred, const int64_t* x_id, const int* idx, const int* q_lens, const float* codebook,
                              int batch, int t_x, int t_q, int n_vocab, int l_bins, int dim, int64_t* q_abs, float* y_d,
                              smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SMT_CHECK_ARG(batch >= 0 && t_x >= 0 && t_q >= 0 && n_vocab >= 0 && l_bins >= 0 && dim >= 0, "smt_vqtts_emit: negative size");
  SMT_CHECK_ARG(dim % 4 == 0, "smt_vqtts_emit: dim %d is not a multiple of 4 (a row moves as 16-byte pieces)", dim);
  if (batch == 0 || t_q == 0 || dim == 0) return 0;
  SMT_CHECK_ARG(pred && idx && q_lens && y_d, "smt_vqtts_emit: null pointer");
  SMT_CHECK_ARG((x_id || t_x == 0) && (codebook || (long long)n_vocab * l_bins == 0), "smt_vqtts_emit: null x_id / codebook");
  SMT_CHECK_ARG((((uintptr_t)codebook | (uintptr_t)y_d) & 15) == 0, "smt_vqtts_emit: codebook and y_d must be 16-byte aligned");
  const long long rows = (long long)batch * t_q;
  const int dim4 = dim / 4;
  const long long blocks = (rows * dim4 + EM_NT - 1) / EM_NT;
  const int grid = (int)(blocks < EM_MAX_BLOCKS ? blocks : EM_MAX_BLOCKS);
  em_emit_kernel<<<grid, EM_NT, 0, stream>>>(pred, x_id, idx, q_lens, (const smt::f32x4*)codebook, rows, t_x, t_q, n_vocab, l_bins,
                                             dim4, q_abs, (smt::f32x4*)y_d);
  SMT_CHECK_LAUNCH("vqtts_emit");
  return 0;
}
