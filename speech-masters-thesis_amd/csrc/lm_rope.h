// The rotary rotation shared by csrc/lm_rope.hip (whole rows: training, logits, prefill) and csrc/lm_decode.hip (the step's q and
// k inside the one-token attention): both paths round at the same points, so a key rotated by the prefill and the same key
// rotated by a decoding step have the same bits.  include/smt_hip.h "Rotary positions" has the definition.
#pragma once
#include "smt_common.h"

namespace smt {

// Four consecutive channels 4j .. 4j + 3 of a head = pairs 2j and 2j + 1; cs = the table's (cos, sin, cos, sin) of those two
// pairs at the row's position (16 bytes at float offset pos * dh + 4j of the table: a table row is dh floats).  One product is
// rounded, the other goes into the FMA: y = fma(x0, c, -(x1 s)), fma(x0, s, x1 c).
__device__ __forceinline__ f32x4 rope_rotate4(const f32x4& x, const f32x4& cs, bool inverse) {
  const float s0 = inverse ? -cs.y : cs.y, s1 = inverse ? -cs.w : cs.w;
  f32x4 y;
  y.x = fmaf(x.x, cs.x, -(x.y * s0));
  y.y = fmaf(x.x, s0, x.y * cs.x);
  y.z = fmaf(x.z, cs.z, -(x.w * s1));
  y.w = fmaf(x.z, s1, x.w * cs.z);
  return y;
}

}  // namespace smt
