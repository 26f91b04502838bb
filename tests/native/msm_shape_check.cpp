// Prints msm_shape's decision for a fixed list of cases, one line each (tests/test_msm_shape_host.py holds the expected values, which were
// derived by hand from the launcher that msm_shape replaced).  No HIP: g++ -O2 -std=c++17 -I vimz_amd/csrc.
#include <cstdio>
#include "msm_shape.hpp"

using namespace vz;

struct Case {
  int id; size_t n; int bits = 254, c_override = 0, split_ones = 0;
  MsmTableDesc tb; MsmGroupDesc rg; MsmTuning tune; bool no_small = false;
};

static MsmTableDesc tables(int c, int K, int own, size_t n_total, bool mult = false) {
  MsmTableDesc t; t.present = true; t.c = c; t.K = K; t.own = own; t.n_total = n_total; t.mult = mult; return t;
}
static MsmGroupDesc group(uint32_t G, uint32_t n_extra = 0) { MsmGroupDesc g; g.grouped = true; g.G = G; g.n_extra = n_extra; return g; }

static void run(const Case& k, const char* tag = "") {
  MsmShape s;
  const int rc = msm_shape(s, k.n, k.bits, k.c_override, k.split_ones, k.tb, k.rg, k.tune, k.no_small);
  static const char* const RC[] = {"ok", "invalid", "not-supported"};
  static const char* const PATH[] = {"FIXED", "SMALL", "LARGE"};
  if (rc != MSM_SHAPE_OK) { printf("case %d%s: %s\n", k.id, tag, RC[rc]); return; }
  const MsmPlan& p = s.plan;
  printf("case %d%s: ok path=%s c=%d K=%d nbw=%u nb=%u split_ones=%d tabled=%d Q=%u chunk=%u Qf=%u lds_sort=%d own=%d shared=%d planes=%d sub=%u entries=%zu max_subs=%zu "
         "sort_blocks=%u lane_bits=%u heavy_min=%u bstride=%u pstride=%u vw=%u V=%d Pl=%u Gp=%u kout=%d sums=%d max_windows=%d\n",
         k.id, tag, PATH[s.path], p.c, p.K, p.nbw, p.nb, p.split_ones, p.tabled, s.Q, s.chunk, s.Qf, (int)s.lds_sort, (int)s.own, (int)s.shared, (int)s.planes, s.sub, s.entries,
         s.max_subs, s.sort_blocks, s.lane_bits, s.heavy_min, s.bstride, s.pstride, s.vw, s.V, s.Pl, s.Gp, s.kout, msm_sums_out(p), MSM_MAX_WINDOWS);
}
// the same case as one row group of G rows
static void run_grouped(Case k, uint32_t G = 4) { k.rg = group(G); run(k, "g"); }

int main() {
  const MsmTableDesc shared15 = tables(15, 17, 0, 313321), own11 = tables(11, 24, 1, 40000), small7 = tables(7, 37, 0, 8000);
  Case k;
  k = Case{1, 1536}; run(k);
  k = Case{2, 1537}; run(k);
  k = Case{3, 30720}; run(k);
  k = Case{4, 30721}; run(k);
  k = Case{5, 30721}; k.no_small = true; run(k);
  k = Case{6, 1000}; k.no_small = true; run(k);
  k = Case{7, 305185}; k.tb = shared15; run(k);
  k = Case{8, 305185}; k.tb = shared15; k.split_ones = 1; run(k);
  k = Case{9, 305185}; k.tb = shared15; k.tune.reduce_planes = 1; run(k); run_grouped(k);
  k = Case{10, 305185}; k.tb = shared15; k.tune.sort_blocks = 40; k.tune.combine_lane_bits = 2; run(k);
  k = Case{11, 305185}; k.tb = shared15; k.tune.sort_blocks = 300; run(k);
  k = Case{12, 3000}; k.c_override = 16; run(k); run_grouped(k);
  k = Case{13, 3000}; k.c_override = 10; run(k);
  k = Case{14, 3000}; k.c_override = 13; run(k);
  k = Case{15, 32768}; k.tb = own11; run(k); run_grouped(k);
  k = Case{16, 30000}; k.tb = own11; run(k);
  k = Case{17, 5000}; k.tb = small7; run(k);
  k = Case{18, 5000}; k.tb = small7; k.tb.mult = true; run(k);
  k = Case{19, 30721}; k.tb = small7; k.tb.n_total = 40000; run(k);
  k = Case{20, 5000}; k.tb = small7; k.tb.K = 36; run(k);
  k = Case{21, 5000}; k.tb = small7; k.c_override = 9; run(k);
  k = Case{22, 524287}; k.split_ones = 1; run(k);
  k = Case{23, 524288}; k.split_ones = 1; run(k);
  k = Case{24, 0}; run(k);
  k = Case{25, (size_t)1 << 31}; run(k);
  k = Case{26, 305185}; k.tb = shared15; k.rg = group(17); run(k);
  k = Case{27, 305185}; k.tb = shared15; k.rg = group(4, 2); run(k);
  k = Case{28, 5000}; k.rg = group(4); run(k);
  k = Case{29, 1000}; k.bits = 255; run(k);
  k = Case{30, (size_t)1 << 17}; k.bits = 255; run(k);
  return 0;
}
