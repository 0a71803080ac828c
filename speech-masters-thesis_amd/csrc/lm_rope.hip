// Rotary positions of the TransformerLM (model.position: rotary; include/smt_hip.h "Rotary positions"): the q and k thirds of
// qkv [B, L, 3 H DH] rotated in place, pair (2i, 2i + 1) of every head by the angle of table row pos0 + l.  The v third is
// neither read nor written.  The gradient of a rotation is the inverse rotation of the incoming gradient (inverse != 0: the
// sine negated), so this one kernel is the forward (training, logits, prefill) and the backward.
//
// A thread owns 16 bytes = two pairs: the q and k thirds of a row are its first 2 H DH floats, H DH / 2 threads a row, one
// 16-byte load of the row, one of the table (L2-resident: L * DH floats, shared by the batch and the heads), one 16-byte
// store.  No transcendental, no atomics, no workspace: 2 * B * L * 2 H DH * 4 bytes of traffic per call.
#include "lm_rope.h"

namespace smt {

template <int DH>
__global__ __launch_bounds__(256) void lm_rope_kernel(float* __restrict__ qkv, const float* __restrict__ rope, long long total, int L,
                                                      int d, int pos0, int inverse) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int per_row = d / 2;                                   // 16-byte pieces of the q and k thirds of one row
  const long long row = t / per_row;
  const int col = 4 * (int)(t % per_row);                      // float offset in the row, < 2 d
  const int l = (int)(row % L);
  float* p = qkv + (size_t)row * 3 * d + col;
  const f32x4 cs = *(const f32x4*)(rope + (size_t)(pos0 + l) * DH + col % DH);
  *(f32x4*)p = rope_rotate4(*(const f32x4*)p, cs, inverse != 0);
}

}  // namespace smt

using namespace smt;

extern "C" int smt_lm_rope(float* qkv, const float* rope, int batch, int len, int heads, int head_dim, int rope_rows, int pos0,
                           int inverse, smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SMT_CHECK_ARG(head_dim == 32 || head_dim == 64, "smt_lm_rope: head dim must be 32 or 64 (got %d)", head_dim);
  SMT_CHECK_ARG(batch >= 0 && len >= 0 && heads >= 1 && rope_rows >= 0, "smt_lm_rope: negative size (batch %d, len %d, heads %d, rope_rows %d)",
                batch, len, heads, rope_rows);
  if (batch == 0 || len == 0) return 0;
  SMT_CHECK_ARG(qkv && rope, "smt_lm_rope: null pointer");
  SMT_CHECK_ARG(((uintptr_t)qkv | (uintptr_t)rope) % 16 == 0, "smt_lm_rope: qkv and the table must be 16-byte aligned");
  SMT_CHECK_ARG(pos0 >= 0 && (long long)pos0 + len <= rope_rows, "smt_lm_rope: positions %d..%lld outside the rope table (%d rows)", pos0,
                (long long)pos0 + len - 1, rope_rows);
  SMT_CHECK_ARG((long long)len * 3 * heads * head_dim < (1ll << 31), "smt_lm_rope: len * 3 * heads * head dim must stay below 2^31");
  const int d = heads * head_dim;
  const long long total = (long long)batch * len * (d / 2), blocks = (total + 255) / 256;
  SMT_CHECK_ARG(blocks < (1ll << 31), "smt_lm_rope: batch * len * heads * head dim too large for one launch");
  if (head_dim == 32) lm_rope_kernel<32><<<(unsigned)blocks, 256, 0, stream>>>(qkv, rope, total, len, d, pos0, inverse);
  else lm_rope_kernel<64><<<(unsigned)blocks, 256, 0, stream>>>(qkv, rope, total, len, d, pos0, inverse);
  SMT_CHECK_LAUNCH("lm_rope");
  return 0;
}
