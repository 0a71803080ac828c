// Text-audio alignment of VQTTS (reference models/vqtts/vqtts.py:133-137, 150-156): the Euclidean distance of every
// (token, frame) pair feeds a monotonic alignment search, and the distances on the found path are the alignment loss.
// The reference materialises a [B, D, Tx, Tq] broadcast and runs the search in numpy on the host; Tq is the audio
// encoder's frame count (18,176 for the training clip), far past what maximum_path_kernel's LDS bitmaps hold (mas.hip).
//
//   vqtts_distance_kernel   dense dist [B, Tx, Tq], for tests and small shapes.
//   vqtts_align_kernel      the product path: one workgroup per batch item computes the distances of a slab of ALIGN_SLAB
//                           columns into LDS (dist_cols, the same function the dense kernel calls, so the same bits), runs
//                           the recurrence of maximum_path_kernel over the slab (v in an LDS double buffer, one barrier
//                           per column, one ballot per 64 rows) and streams the direction words to a global workspace.
//                           The backtrack stages ALIGN_CHUNK columns of direction words in LDS at a time; wave 0 walks
//                           them ALIGN_WALK columns per step: lane l holds the 64 rows [p - 63, p] of column j - l (the path
//                           climbs at most one row per column, so nothing else can be read) and the walk itself is 64
//                           readlane + scalar steps with no memory access in the chain.
//   vqtts_frame_dist_kernel / vqtts_sum_kernel / vqtts_loss_dy_kernel / vqtts_loss_dx_kernel   the loss on the path and its
//                           gradients; the frames of a token are contiguous, so dx is a sum in frame order, no atomics.
#include <algorithm>

#include "smt_common.h"

namespace smt {

constexpr int VA_NT = 512;            // threads of the fused search = its row limit (one row per thread)
constexpr int VA_SLAB = 32;           // columns whose distances are computed before their recurrence runs
constexpr int VA_CHUNK = 512;         // columns of direction words staged in LDS per backtrack chunk
constexpr int VA_WALK = 64;           // columns one walk step consumes (one per lane of wave 0)
constexpr int VA_NC = 4;              // columns per thread in dist_cols
constexpr int VA_MAX_D = 256, VA_MAX_TX = VA_NT, VA_MAX_TQ = 32768, VA_MAX_B = 65535;
constexpr size_t VA_LDS_LIMIT = 160 * 1024 - 64;

// sqrt(sum_d (x[d] - y_c[d])^2) of one x row against NC y rows (y0 + c * ystride): squared differences accumulated with
// fmaf in ascending d.  The ONE place a distance is computed: every kernel below calls it, so they agree bit for bit.
template <int NC>
__device__ __forceinline__ void dist_cols(const float* __restrict__ xr, const float* __restrict__ y0, int ystride, int D,
                                          float (&out)[NC]) {
  float acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.f;
  for (int d = 0; d < D; d += 4) {
    const float4 xv = *reinterpret_cast<const float4*>(xr + d);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const float4 yv = *reinterpret_cast<const float4*>(y0 + (size_t)c * ystride + d);
      float t = xv.x - yv.x;
      acc[c] = fmaf(t, t, acc[c]);
      t = xv.y - yv.y;
      acc[c] = fmaf(t, t, acc[c]);
      t = xv.z - yv.z;
      acc[c] = fmaf(t, t, acc[c]);
      t = xv.w - yv.w;
      acc[c] = fmaf(t, t, acc[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) out[c] = sqrtf(acc[c]);
}

// dist [B, Tx, Tq]: thread = one row i and VA_NC consecutive columns; blockIdx.y = i, blockIdx.z = b
__global__ __launch_bounds__(256) void vqtts_distance_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                             float* __restrict__ dist, int Tx, int Tq, int D) {
  const int b = blockIdx.z, i = blockIdx.y;
  const int j = (blockIdx.x * 256 + threadIdx.x) * VA_NC;
  if (j >= Tq) return;
  const int jl = min(j, Tq - VA_NC);                          // a tail group is moved back inside the row (Tq >= VA_NC) ...
  float out[VA_NC];
  const float* xr = x + ((size_t)b * Tx + i) * D;
  float* o = dist + ((size_t)b * Tx + i) * Tq;
  if (Tq >= VA_NC) {
    dist_cols<VA_NC>(xr, y + ((size_t)b * Tq + jl) * D, D, D, out);
#pragma unroll
    for (int c = 0; c < VA_NC; ++c) o[jl + c] = out[c];      // ... and rewrites up to VA_NC - 1 values with the same bits
  } else {
    for (int c = 0; c < Tq; ++c) {                            // fewer than VA_NC columns: one at a time (stride 0)
      dist_cols<VA_NC>(xr, y + ((size_t)b * Tq + c) * D, 0, D, out);
      o[c] = out[0];
    }
  }
}

struct AlignLds {                     // byte offsets of the fused search's LDS regions
  int vp, tp, xp, words;
  size_t v, cnt, ys, tile, xs, total;
  bool x_in_lds;
};

__host__ __device__ static inline AlignLds align_lds(int Tx, int D) {
  AlignLds L;
  L.words = (Tx + 63) / 64;
  L.vp = (Tx + 3) / 4 * 4;
  L.tp = L.vp;
  L.xp = D + 4;                                               // row pitch of x in LDS: b128 reads of 8 consecutive rows hit 8 bank groups
  if (L.xp % 32 == 0) L.xp += 4;
  L.v = 0;
  L.cnt = L.v + 2 * (size_t)L.vp * 4;
  L.ys = L.cnt + (size_t)L.vp * 4;
  L.tile = L.ys + (size_t)VA_SLAB * D * 4;
  const size_t tile_bytes = std::max((size_t)VA_SLAB * L.tp * 4, (size_t)VA_CHUNK * L.words * 8);
  L.xs = L.tile + tile_bytes;
  const size_t with_x = L.xs + (size_t)Tx * L.xp * 4;
  L.x_in_lds = with_x <= VA_LDS_LIMIT;
  L.total = L.x_in_lds ? with_x : L.xs;
  return L;
}

__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}

template <bool XLDS>
__global__ __launch_bounds__(VA_NT) void vqtts_align_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                            const int* __restrict__ x_lens, const int* __restrict__ q_lens,
                                                            int Tx, int Tq, int D, unsigned long long* __restrict__ ws,
                                                            int* __restrict__ idx, float* __restrict__ dur) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const AlignLds L = align_lds(Tx, D);
  float* vb = reinterpret_cast<float*>(smem + L.v);          // [2][vp]
  int* cnt = reinterpret_cast<int*>(smem + L.cnt);           // [Tx] frames per token
  float* ys = reinterpret_cast<float*>(smem + L.ys);         // [VA_SLAB][D]
  float* dt = reinterpret_cast<float*>(smem + L.tile);       // [VA_SLAB][tp] distances of the slab, column-major ...
  unsigned long long* cb = reinterpret_cast<unsigned long long*>(smem + L.tile);   // ... reused as [VA_CHUNK][words] in the backtrack
  float* xs = reinterpret_cast<float*>(smem + L.xs);         // [Tx][xp] when XLDS
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int words = L.words, vp = L.vp, tp = L.tp, xp = L.xp;
  const int xl = min(max(x_lens[b], 0), Tx), ql = min(max(q_lens[b], 0), Tq);
  const float* xg = x + (size_t)b * Tx * D;
  const float* yg = y + (size_t)b * Tq * D;
  unsigned long long* wsb = ws + (size_t)b * Tq * words;
  int* idxb = idx + (size_t)b * Tq;
  const float NEG_INF = -__builtin_huge_valf();
  const int d4 = D / 4;

  for (int i = tid; i < vp; i += VA_NT) { vb[i] = 0.f; cnt[i] = 0; }
  for (int j = ql + tid; j < Tq; j += VA_NT) idxb[j] = -1;
  const bool live = xl > 0 && ql > 0;                         // otherwise the mask is empty: no frame has a token
  if (!live) {
    for (int j = tid; j < ql; j += VA_NT) idxb[j] = -1;
    for (int i = tid; i < Tx; i += VA_NT) dur[(size_t)b * Tx + i] = 0.f;
    return;
  }
  if (XLDS) {
    for (int e = tid; e < xl * d4; e += VA_NT) {
      const int i = e / d4, c = e - i * d4;
      *reinterpret_cast<float4*>(xs + (size_t)i * xp + 4 * c) = *reinterpret_cast<const float4*>(xg + (size_t)i * D + 4 * c);
    }
  }
  // the next slab's y rows wait in registers while the current slab's recurrence runs: VA_SLAB * D / 4 float4 over VA_NT threads
  constexpr int PRE = VA_SLAB * VA_MAX_D / 4 / VA_NT;
  float4 pre[PRE];
#define VA_PREFETCH(j0_)                                                                                   \
  {                                                                                                        \
    const int n4_ = min(VA_SLAB, ql - (j0_)) * d4;                                                         \
    _Pragma("unroll") for (int r = 0; r < PRE; ++r) {                                                      \
      const int e = tid + r * VA_NT;                                                                       \
      pre[r] = e < n4_ ? *reinterpret_cast<const float4*>(yg + (size_t)(j0_) * D + 4 * (size_t)e)          \
                       : make_float4(0.f, 0.f, 0.f, 0.f);                                                  \
    }                                                                                                      \
  }
  VA_PREFETCH(0);

  int cur = 0;
  for (int j0 = 0; j0 < ql; j0 += VA_SLAB) {
    const int jn = min(VA_SLAB, ql - j0);
    {
      const int n4 = jn * d4;
#pragma unroll
      for (int r = 0; r < PRE; ++r) {
        const int e = tid + r * VA_NT;
        if (e < n4) *reinterpret_cast<float4*>(ys + 4 * (size_t)e) = pre[r];
      }
    }
    __syncthreads();                                          // ys (and, the first time, xs / vb / cnt) written
    if (j0 + VA_SLAB < ql) VA_PREFETCH(j0 + VA_SLAB);
    // distances of the slab: task = (group of VA_NC columns, row); consecutive lanes take consecutive rows
    const int ngroups = (jn + VA_NC - 1) / VA_NC;
    for (int t = tid; t < ngroups * xl; t += VA_NT) {
      const int cg = t / xl, i = t - cg * xl;
      const int c0 = cg * VA_NC;
      float out[VA_NC];
      // a tail group shorter than VA_NC reads ys rows past jn: stale but inside ys, and never stored
      const float* xr = XLDS ? xs + (size_t)i * xp : xg + (size_t)i * D;
      dist_cols<VA_NC>(xr, ys + (size_t)c0 * D, D, D, out);
#pragma unroll
      for (int c = 0; c < VA_NC; ++c)
        if (c0 + c < jn) dt[(size_t)(c0 + c) * tp + i] = out[c];
    }
    __syncthreads();
    // recurrence of maximum_path_kernel with value = -dist, mask = 1 on the xl x ql lattice
    const int xrow = tid;
    const bool in = xrow < xl;
    for (int jj = 0; jj < jn; ++jj) {
      const int j = j0 + jj;
      const float* vc = vb + cur * vp;
      float* vn = vb + (cur ^ 1) * vp;
      const float v1 = in ? vc[xrow] : 0.f;
      const float vprev = (in && xrow > 0) ? vc[xrow - 1] : NEG_INF;
      const bool keep = v1 >= vprev;
      const float vmax = keep ? v1 : vprev;
      if (in) vn[xrow] = (xrow <= j) ? vmax - dt[(size_t)jj * tp + xrow] : NEG_INF;
      const unsigned long long kb = __ballot(in && keep);
      if (lane == 0 && wave < words) wsb[(size_t)j * words + wave] = kb;
      cur ^= 1;
      __syncthreads();
    }
  }

#undef VA_PREFETCH

  // backtrack from (xl - 1, ql - 1)
  int p = xl - 1;
  for (int jhi = ql; jhi > 0; jhi -= VA_CHUNK) {
    const int jlo = max(0, jhi - VA_CHUNK);
    const int nw = (jhi - jlo) * words;
    __syncthreads();                                          // the previous chunk's walk (or the last column's stores) is done
    for (int e = tid; e < nw; e += VA_NT) cb[e] = wsb[(size_t)jlo * words + e];
    __syncthreads();
    if (wave == 0) {
      for (int jt = jhi - 1; jt >= jlo; jt -= VA_WALK) {
        const int col = jt - lane;
        const bool valid = col >= jlo;
        const int lo_row = p - 63;                            // lane's window = rows [p - 63, p] of its column
        const int wlo = lo_row >> 6, s = lo_row & 63;
        unsigned long long a = ~0ull, hi = ~0ull;             // rows outside the lattice and columns outside the chunk: "stay"
        if (valid) {
          const unsigned long long* cw = cb + (size_t)(col - jlo) * words;
          if (wlo >= 0 && wlo < words) a = cw[wlo];
          if (wlo + 1 >= 0 && wlo + 1 < words) hi = cw[wlo + 1];
        }
        const unsigned long long win = s ? (a >> s) | (hi << (64 - s)) : a;
        int off = 0, myp = p;
#pragma unroll
        for (int l = 0; l < VA_WALK; ++l) {
          const unsigned long long w = readlane_u64(win, l);
          if (lane == l) myp = p - off;
          off += 1 - (int)((w >> (63 - off)) & 1ull);
        }
        if (valid) {
          idxb[col] = myp >= 0 ? myp : -1;
          if (myp >= 0) atomicAdd(&cnt[myp], 1);
        }
        p -= off;
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < Tx; i += VA_NT) dur[(size_t)b * Tx + i] = (float)cnt[i];
}

// fd[b, j] = dist(x[b, idx[b, j]], y[b, j]), 0 where the frame has no token
__global__ __launch_bounds__(256) void vqtts_frame_dist_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                               const int* __restrict__ idx, float* __restrict__ fd, long long rows,
                                                               int Tx, int Tq, int D) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const int tok = idx[r];
  float out[1] = {0.f};
  if (tok >= 0 && tok < Tx) dist_cols<1>(x + ((size_t)(r / Tq) * Tx + tok) * D, y + (size_t)r * D, 0, D, out);
  fd[r] = out[0];
}

// sum[0] = sum of v[0..n): thread t adds v[t], v[t + 1024], ... in that order, then a fixed tree -- the same bits every run
__global__ __launch_bounds__(1024) void vqtts_sum_kernel(const float* __restrict__ v, long long n, float* __restrict__ sum) {
  __shared__ float part[1024];
  float s = 0.f;
  for (long long e = threadIdx.x; e < n; e += 1024) s += v[e];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) sum[0] = part[0];
}

// dy[b, j, :] = coef (y_j - x_i) / dist, 0 where the frame has no token or dist == 0
__global__ __launch_bounds__(256) void vqtts_loss_dy_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                            const int* __restrict__ idx, const float* __restrict__ fd,
                                                            const float* __restrict__ coef, float* __restrict__ dy, long long total4,
                                                            int Tx, int Tq, int D) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total4) return;
  const int d4 = D / 4;
  const long long r = e / d4;
  const int c = (int)(e - r * d4);
  const int tok = idx[r];
  const float dist = fd[r];
  float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
  if (tok >= 0 && tok < Tx && dist > 0.f) {
    const float k = coef[0];
    const float4 yv = *reinterpret_cast<const float4*>(y + (size_t)r * D + 4 * c);
    const float4 xv = *reinterpret_cast<const float4*>(x + ((size_t)(r / Tq) * Tx + tok) * D + 4 * c);
    g.x = k * (yv.x - xv.x) / dist;
    g.y = k * (yv.y - xv.y) / dist;
    g.z = k * (yv.z - xv.z) / dist;
    g.w = k * (yv.w - xv.w) / dist;
  }
  *reinterpret_cast<float4*>(dy + (size_t)r * D + 4 * c) = g;
}

// dx[b, i, :] = -(sum of dy[b, j, :] over the frames of token i, in frame order).  On a monotonic path idx is
// non-decreasing over the frames that have a token and -1 after them, so the frames of token i are [lower(i), lower(i + 1)).
__global__ __launch_bounds__(64) void vqtts_loss_dx_kernel(const int* __restrict__ idx, const float* __restrict__ dy,
                                                           float* __restrict__ dx, int Tx, int Tq, int D) {
  const int b = blockIdx.y, i = blockIdx.x;
  const int* ib = idx + (size_t)b * Tq;
  auto lower = [&](int key) {                                 // first frame whose token is >= key (no token = past every key)
    int lo = 0, hi = Tq;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const int t = ib[mid];
      if (t >= 0 && t < key) lo = mid + 1; else hi = mid;
    }
    return lo;
  };
  const int start = lower(i), end = lower(i + 1);
  const int c = threadIdx.x;
  if (4 * c >= D) return;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int j = start; j < end; ++j) {
    if (ib[j] != i) continue;                                 // only on an index that is not a monotonic path
    const float4 g = *reinterpret_cast<const float4*>(dy + ((size_t)b * Tq + j) * D + 4 * c);
    s.x += g.x; s.y += g.y; s.z += g.z; s.w += g.w;
  }
  *reinterpret_cast<float4*>(dx + ((size_t)b * Tx + i) * D + 4 * c) = make_float4(-s.x, -s.y, -s.z, -s.w);
}

}  // namespace smt

using namespace smt;

#define VA_CHECK_SHAPE(name)                                                                                            \
  SMT_CHECK_ARG(dim > 0 && dim % 4 == 0 && dim <= VA_MAX_D, name ": dim=%d must be a multiple of 4 up to %d", dim, VA_MAX_D); \
  SMT_CHECK_ARG(t_x <= VA_MAX_TX, name ": t_x=%d exceeds the limit of %d tokens", t_x, VA_MAX_TX);                      \
  SMT_CHECK_ARG(t_q <= VA_MAX_TQ, name ": t_q=%d exceeds the limit of %d frames", t_q, VA_MAX_TQ);                      \
  SMT_CHECK_ARG(batch <= VA_MAX_B, name ": batch=%d exceeds the limit of %d items", batch, VA_MAX_B)

extern "C" int smt_vqtts_distance(const float* x_enc, const float* y_enc, float* dist, int batch, int t_x, int t_q, int dim,
                                  smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SMT_CHECK_ARG(batch >= 0 && t_x >= 0 && t_q >= 0, "smt_vqtts_distance: negative size");
  VA_CHECK_SHAPE("smt_vqtts_distance");
  if (batch == 0 || t_x == 0 || t_q == 0) return 0;
  SMT_CHECK_ARG(x_enc && y_enc && dist, "smt_vqtts_distance: null pointer");
  const dim3 grid((t_q + 256 * VA_NC - 1) / (256 * VA_NC), t_x, batch);
  vqtts_distance_kernel<<<grid, 256, 0, stream>>>(x_enc, y_enc, dist, t_x, t_q, dim);
  SMT_CHECK_LAUNCH("vqtts_distance");
  return 0;
}

extern "C" size_t smt_vqtts_align_workspace_bytes(int batch, int t_x, int t_q) {
  if (batch <= 0 || t_x <= 0 || t_q <= 0) return 0;
  return (size_t)batch * t_q * ((t_x + 63) / 64) * 8;
}

extern "C" int smt_vqtts_align(const float* x_enc, const float* y_enc, const int* x_lens, const int* q_lens, int batch, int t_x,
                               int t_q, int dim, int* idx, float* dur, void* workspace, size_t workspace_bytes,
                               smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SMT_CHECK_ARG(batch >= 0 && t_x >= 0 && t_q >= 0, "smt_vqtts_align: negative size");
  VA_CHECK_SHAPE("smt_vqtts_align");
  if (batch == 0) return 0;
  if (t_x == 0 || t_q == 0) {                                 // an empty lattice: no frame has a token
    if (t_q > 0) {
      SMT_CHECK_ARG(idx, "smt_vqtts_align: null pointer");
      if (hipMemsetAsync(idx, 0xFF, (size_t)batch * t_q * sizeof(int), stream) != hipSuccess) SMT_CHECK_ARG(false, "smt_vqtts_align: memset failed");
    }
    if (t_x > 0) {
      SMT_CHECK_ARG(dur, "smt_vqtts_align: null pointer");
      if (hipMemsetAsync(dur, 0, (size_t)batch * t_x * sizeof(float), stream) != hipSuccess) SMT_CHECK_ARG(false, "smt_vqtts_align: memset failed");
    }
    return 0;
  }
  SMT_CHECK_ARG(x_enc && y_enc && x_lens && q_lens && idx && dur && workspace, "smt_vqtts_align: null pointer");
  const size_t need = smt_vqtts_align_workspace_bytes(batch, t_x, t_q);
  SMT_CHECK_ARG(workspace_bytes >= need, "smt_vqtts_align: workspace of %zu B, %zu B needed", workspace_bytes, need);
  SMT_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "smt_vqtts_align: workspace must be 8-byte aligned");
  const AlignLds L = align_lds(t_x, dim);
  SMT_CHECK_ARG(L.total <= VA_LDS_LIMIT, "smt_vqtts_align: t_x=%d dim=%d needs %zu B of LDS (limit 160 KiB)", t_x, dim, L.total);
  unsigned long long* ws = reinterpret_cast<unsigned long long*>(workspace);
  if (L.x_in_lds) {
    (void)hipFuncSetAttribute((const void*)vqtts_align_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.total);
    vqtts_align_kernel<true><<<batch, VA_NT, L.total, stream>>>(x_enc, y_enc, x_lens, q_lens, t_x, t_q, dim, ws, idx, dur);
  } else {
    (void)hipFuncSetAttribute((const void*)vqtts_align_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.total);
    vqtts_align_kernel<false><<<batch, VA_NT, L.total, stream>>>(x_enc, y_enc, x_lens, q_lens, t_x, t_q, dim, ws, idx, dur);
  }
  SMT_CHECK_LAUNCH("vqtts_align");
  return 0;
}

extern "C" int smt_vqtts_align_loss(const float* x_enc, const float* y_enc, const int* idx, int batch, int t_x, int t_q, int dim,
                                    float* frame_dist, float* sum, smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SMT_CHECK_ARG(batch >= 0 && t_x >= 0 && t_q >= 0, "smt_vqtts_align_loss: negative size");
  VA_CHECK_SHAPE("smt_vqtts_align_loss");
  SMT_CHECK_ARG(sum, "smt_vqtts_align_loss: null pointer");
  const long long rows = (long long)batch * t_q;
  if (rows > 0) {
    SMT_CHECK_ARG(y_enc && idx && frame_dist && (x_enc || t_x == 0), "smt_vqtts_align_loss: null pointer");
    vqtts_frame_dist_kernel<<<(unsigned)((rows + 255) / 256), 256, 0, stream>>>(x_enc, y_enc, idx, frame_dist, rows, t_x, t_q, dim);
    SMT_CHECK_LAUNCH("vqtts_frame_dist");
  }
  vqtts_sum_kernel<<<1, 1024, 0, stream>>>(frame_dist, rows, sum);
  SMT_CHECK_LAUNCH("vqtts_sum");
  return 0;
}

extern "C" int smt_vqtts_align_loss_bwd(const float* x_enc, const float* y_enc, const int* idx, const float* frame_dist,
                                        const float* coef, int batch, int t_x, int t_q, int dim, float* dx, float* dy,
                                        smt_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SMT_CHECK_ARG(batch >= 0 && t_x >= 0 && t_q >= 0, "smt_vqtts_align_loss_bwd: negative size");
  VA_CHECK_SHAPE("smt_vqtts_align_loss_bwd");
  if (batch == 0) return 0;
  const long long total4 = (long long)batch * t_q * (dim / 4);
  if (total4 > 0) {
    SMT_CHECK_ARG(y_enc && idx && frame_dist && coef && dy && (x_enc || t_x == 0), "smt_vqtts_align_loss_bwd: null pointer");
    vqtts_loss_dy_kernel<<<(unsigned)((total4 + 255) / 256), 256, 0, stream>>>(x_enc, y_enc, idx, frame_dist, coef, dy, total4, t_x, t_q, dim);
    SMT_CHECK_LAUNCH("vqtts_loss_dy");
  }
  if (t_x > 0) {
    SMT_CHECK_ARG(dx && (t_q == 0 || (idx && dy)), "smt_vqtts_align_loss_bwd: null pointer");
    vqtts_loss_dx_kernel<<<dim3(t_x, batch), 64, 0, stream>>>(idx, dy, dx, t_x, t_q, dim);
    SMT_CHECK_LAUNCH("vqtts_loss_dx");
  }
  return 0;
}
