// Host run of the streaming kernels' launch plan and tile split (csrc/conv_stream.h: plan_stream, tile_run).  Built and run
// by tests/test_stream_plan_cpu.py with hipcc (no GPU needed: only host code executes).
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../speech-masters-thesis_amd/csrc/conv_common.h"

static int fails = 0;
#define CHECK(cond, ...)                        \
  do {                                          \
    if (!(cond)) {                              \
      ++fails;                                  \
      std::printf("FAIL %s: ", #cond);          \
      std::printf(__VA_ARGS__);                 \
      std::printf("\n");                        \
    }                                           \
  } while (0)

static void run_case(long long ntiles, int cap, int min_tpw) {
  const smt::StreamGrid g = smt::plan_stream(ntiles, cap, min_tpw);
  // the closed formula: nwg = min(cap, max(8, ceil(ntiles / min_tpw))) rounded up to a multiple of 8, tpw = ceil(ntiles / nwg)
  long long nwg = (ntiles + min_tpw - 1) / min_tpw;
  if (nwg < 8) nwg = 8;
  if (nwg > cap) nwg = cap;
  nwg = (nwg + 7) / 8 * 8;
  const long long tpw = (ntiles + nwg - 1) / nwg;
  CHECK(g.nwg == nwg && g.tiles_per_wg == tpw, "ntiles %lld cap %d min_tpw %d: plan (%d, %d), formula (%lld, %lld)", ntiles, cap,
        min_tpw, g.nwg, g.tiles_per_wg, nwg, tpw);
  CHECK(g.nwg % 8 == 0 && g.nwg >= 8, "ntiles %lld cap %d min_tpw %d: nwg %d", ntiles, cap, min_tpw, g.nwg);
  CHECK((long long)g.nwg * g.tiles_per_wg >= ntiles, "ntiles %lld cap %d min_tpw %d: %d x %d tiles", ntiles, cap, min_tpw, g.nwg,
        g.tiles_per_wg);
  for (int clamp = 0; clamp < 2; ++clamp) {
    std::vector<int> owner(ntiles, -1), seen(g.nwg, 0);
    for (int block = 0; block < g.nwg; ++block) {
      const smt::TileRun t = smt::tile_run(g.nwg, (unsigned)block, (int)ntiles, g.tiles_per_wg, clamp != 0);
      CHECK(0 <= t.wg && t.wg < g.nwg, "block %d: wg %d of %d", block, t.wg, g.nwg);
      if (0 <= t.wg && t.wg < g.nwg) ++seen[t.wg];
      CHECK(t.end <= ntiles && t.end - t.begin <= g.tiles_per_wg, "block %d: run [%d, %d)", block, t.begin, t.end);
      if (clamp) CHECK(t.begin <= t.end, "block %d: clamped run [%d, %d)", block, t.begin, t.end);
      for (int tile = std::max(t.begin, 0); tile < t.end; ++tile) {
        CHECK(owner[tile] == -1, "tile %d in the runs of blocks %d and %d", tile, owner[tile], block);   // pairwise disjoint
        owner[tile] = block;
      }
    }
    for (long long tile = 0; tile < ntiles; ++tile) CHECK(owner[tile] >= 0, "tile %lld in no run", tile);   // exact cover
    for (int w = 0; w < g.nwg; ++w) CHECK(seen[w] == 1, "wg %d taken %d times", w, seen[w]);                  // a permutation
  }
  std::printf("case ntiles %lld cap %d min_tpw %d -> nwg %d tiles_per_wg %d\n", ntiles, cap, min_tpw, g.nwg, g.tiles_per_wg);
}

int main() {
  const long long ntiles[] = {0, 1, 7, 8, 9, 15, 16, 17, 511, 512, 513, 1025, 2049, 100000};
  // (cap, min_tpw) of the kernels: k3gate / resampling (256, 1); fold, k1_bwd, 1x1_bwd (256, 2); k1act, 1x1_dma, gate_bwd
  // (512, 2); c64 (1024, 2); gate_bwd with SMT_FUSED_MIN_TPW=1 (512, 1)
  const int plans[][2] = {{256, 1}, {256, 2}, {512, 2}, {1024, 2}, {512, 1}};
  for (long long n : ntiles)
    for (const auto& pl : plans) run_case(n, pl[0], pl[1]);
  std::printf("failures %d\n", fails);
  return fails ? 1 : 0;
}
