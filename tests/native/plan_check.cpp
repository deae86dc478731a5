// Host-side property check of a train step's plan (plenoctree_amd/csrc/pxo_common.h: wgrad_split, plan_step): what the step
// decides from one tuning snapshot before its first launch.  Compiled and run by
// tests/test_host_cpu.py::test_step_plan_properties (hipcc, host code only - no device is touched).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pxo_common.h"

using namespace pxo;

static long g_bad = 0;
#define CHECK(cond)                                                                                                    \
  do {                                                                                                                 \
    if (!(cond)) {                                                                                                     \
      if (g_bad < 10)                                                                                                  \
        std::printf("FAIL %s  (M_c=%lld M_f=%lld ncu=%d prec=%d skip_zero_rows=%d tuning=%d,%d,%d,%d,%d)\n", #cond,     \
                    (long long)M_c, (long long)M_f, ncu, cfg.mlp_precision, cfg.skip_zero_rows, tu.tile_sched,          \
                    tu.wgrad_ranges, tu.wgrad_skinny_ranges, tu.coarse_stream, tu.x6_wgrad);                             \
      ++g_bad;                                                                                                         \
    }                                                                                                                  \
  } while (0)

static bool same(const WgradSplit& a, const WgradSplit& b) {
  return a.rpw_main == b.rpw_main && a.P_main == b.P_main && a.rpw_skinny == b.rpw_skinny && a.P_skinny == b.P_skinny;
}
static bool fits(const WgradSplit& w) {
  return w.rpw_main <= (int64_t)kMaxLiveChunks * kLiveRows && w.rpw_skinny <= (int64_t)kMaxLiveChunks * kLiveRows;
}
// the ranges cover [0, M) exactly, in whole kKC-row granules, and there are never more of them than the workspace has slabs
// for (wgrad_workspace_bytes: ncu slab sets of the 256x256 products, 2 ncu of the skinny ones)
static bool covers(const WgradSplit& w, int64_t M, int ncu) {
  if (M == 0) return w.P_main == 0 && w.P_skinny == 0;
  return w.rpw_main % kKC == 0 && w.rpw_skinny % kKC == 0 && w.P_main >= 1 && w.P_main <= ncu && w.P_skinny >= 1 &&
         w.P_skinny <= 2 * ncu && w.P_main * w.rpw_main >= M && (w.P_main - 1) * w.rpw_main < M &&
         w.P_skinny * w.rpw_skinny >= M && (w.P_skinny - 1) * w.rpw_skinny < M;
}

static StepPlan check(const PxoCfg& cfg, int64_t M_c, int64_t M_f, int ncu, const Tuning& tu) {
  const StepPlan p = plan_step(cfg, M_c, M_f, ncu, tu);
  // the splits the launchers receive are the ones the skip decision was made on
  const WgradSplit wc = wgrad_split(M_c, ncu, tu), wf = wgrad_split(M_f, ncu, tu);
  CHECK(same(p.split_c, wc) && same(p.split_f, wf));
  CHECK(covers(p.split_c, M_c, ncu) && covers(p.split_f, M_f, ncu));
  // skipping only where every range of both passes fits a live-chunk list -- and then always, when asked for
  if (p.skip) CHECK(fits(p.split_c) && fits(p.split_f));
  CHECK(p.skip == (cfg.skip_zero_rows != 0 && fits(wc) && (M_f == 0 || fits(wf))));
  const bool x6 = cfg.mlp_precision == PXO_MLP_BF16X6 && tu.x6_wgrad != 0;
  CHECK(p.x6_main == x6 && p.bias_from_wgrad == x6);
  CHECK(p.dyn == (tu.tile_sched != 0));
  CHECK(p.fork == (M_f > 0 && tu.coarse_stream != 0));
  return p;
}

int main() {
  long cases = 0, skipping = 0, dense_fallback = 0;
  std::vector<int64_t> Ms;
  for (int64_t M = 1; M <= 9000000; M += 2999) Ms.push_back(M);
  for (int64_t M : {1, 31, 32, 33, 38400, 115977, 262144, 786432, 796432, 8388608, 9000000}) Ms.push_back(M);
  // around the live-list limit: ranges of exactly 32,768 rows and one granule more, for 1 .. 512 ranges
  for (int64_t r : {1, 2, 3, 73, 100, 104, 146, 256, 274, 304, 512})
    for (int64_t d : {-kKC, -1, 0, 1, kKC}) Ms.push_back(r * kMaxLiveChunks * kLiveRows + d);
  const int ncus[] = {1, 8, 32, 80, 104, 256, 304, 512};
  PxoCfg cfg = {};
  for (int ncu : ncus)
    for (int64_t M : Ms)
      for (int64_t M_f : {(int64_t)0, 3 * M + 777, M / 3})
        for (int ranges : {0, 1, 2, 73, ncu})
          for (int skinny : {0, 1, 100, 2 * ncu}) {
            if (ranges > ncu || skinny > 2 * ncu) continue;        // pxo_set_tuning's bounds
            for (int prec : {PXO_MLP_F32, PXO_MLP_BF16X6})
              for (int bits = 0; bits < 16; ++bits) {
                cfg.mlp_precision = prec;
                cfg.skip_zero_rows = bits & 1;
                const Tuning tu{(bits >> 1) & 1, ranges, skinny, (bits >> 2) & 1, (bits >> 3) & 1};
                const StepPlan p = check(cfg, M, M_f, ncu, tu);
                ++cases;
                if (cfg.skip_zero_rows) ++(p.skip ? skipping : dense_fallback);
              }
          }
  std::printf("cases %ld bad %ld skipping %ld dense_fallback %ld kMaxLiveChunks %d kLiveRows %d\n", cases, g_bad, skipping,
              dense_fallback, kMaxLiveChunks, kLiveRows);
  return g_bad ? 1 : 0;
}
