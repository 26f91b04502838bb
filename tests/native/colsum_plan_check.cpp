// The column sums and the h query of vimz_amd/csrc/g16_powers.hip on the CPU: the host plan (g16_colsum_plan.hpp: colsum_plan) of every case in the file named
// on the command line, its invariants asserted here, and the very functions the kernels call with their thread index (g16_point_stage.hpp: colsum_run, pt_diff)
// looped over every thread of every level, over G1 with the canonical Fp fields.  The file holds, a case:
//     CASE name n_rows n_cols n_dict          ROWPTR n_rows + 1 numbers          COL nnz numbers          COEF nnz numbers
//     DICT n_dict hex coefficients below r    SCALARS n_rows hex scalars s_r: the points are [s_r]G
// and  HQ name n dinv s_0 .. s_(2n-2)  for an h query.  Judged here: the plan's invariants, and the looped functions' outputs against plain sums (every entry's
// c·P by double-and-add over all 254 bits, added up).  Printed for tests/test_colsum_plan_host.py: the outputs' coordinates (OUT name x y ..; canonical, hex; the
// identity as zeros) and the plan (MAGS, ENTRIES, LEVEL lines), which that test evaluates on scalars.  No HIP: g++ -std=c++17 -fsanitize=address,undefined -I vimz_amd/csrc.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "g16_point_stage.hpp"

using namespace vz;
typedef Fp<BnFr> Fr;
typedef Fp<BnFq> Fq;
typedef Affine<Fq> Pt;

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "colsum_plan_check: %s: ", name.c_str()); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); exit(1); } } while (0)

template <class F>
static F from_hex(const std::string& h) {      // canonical words of a hex integer below 2^256
  F c = F::zero();
  int bit = 0;
  for (size_t i = h.size(); i-- > 0; bit += 4) {
    const char ch = h[i];
    const uint32_t d = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : 16;
    if (d > 15 || bit >= 256) { fprintf(stderr, "bad hex %s\n", h.c_str()); exit(2); }
    c.v[bit >> 5] |= d << (bit & 31);
  }
  return c;
}
static void print_fq(const Fq& m) {
  const Fq c = Fq::from_mont(m);
  putchar(' ');
  for (int i = 7; i >= 0; i--) printf("%08x", c.v[i]);
}
static Pt generator() { Pt g; g.x = Fq::one(); g.y = Fq::dbl(Fq::one()); return g; }
static bool same(const Pt& a, const Pt& b) { return a.x.eq(b.x) && a.y.eq(b.y); }

template <class T>
static std::vector<T> numbers(std::istream& in, const char* tag, size_t n) {
  std::string line, t;
  if (!std::getline(in, line)) { fprintf(stderr, "missing %s\n", tag); exit(2); }
  std::istringstream ls(line);
  ls >> t;
  if (t != tag) { fprintf(stderr, "expected %s, read %s\n", tag, t.c_str()); exit(2); }
  std::vector<T> v;
  while (ls >> t) { if constexpr (std::is_same<T, Fr>::value) v.push_back(from_hex<Fr>(t)); else v.push_back((T)std::stoul(t)); }
  if (v.size() != n) { fprintf(stderr, "%s: %zu values, expected %zu\n", tag, v.size(), n); exit(2); }
  return v;
}

// The plan's invariants.  part_rows: row_base of the matrix's rows; units: the extra entries of coefficient one.
static void check_plan(const std::string& name, const ColsumPlan& P, const std::vector<uint32_t>& row_ptr, const std::vector<uint32_t>& col, const std::vector<uint32_t>& coef,
                       const std::vector<Fr>& dict, uint32_t row_base, const std::vector<ColsumUnit>& units) {
  const size_t n_rows = row_ptr.size() - 1, n_lv = P.levels.size();
  CHECK(n_lv >= 1 && P.mags.size() >= 8 && P.mags[0] == 1, "no level 0 or no magnitude one");
  // every run: its bounds, the order within its level, a slot of its own
  for (size_t lv = 0; lv < n_lv; lv++) {
    const ColsumLevel& L = P.levels[lv];
    const size_t n_src = lv ? P.levels[lv - 1].n_partials : P.entries.size();
    std::vector<uint32_t> read(n_src, 0), written(L.n_partials, 0);
    for (size_t t = 0; t < L.runs.size(); t++) {
      const ColsumRun& r = L.runs[t];
      CHECK(r.len >= 1 && r.len <= COLSUM_CHUNK, "level %zu run %zu holds %u entries", lv, t, r.len);
      CHECK(r.bits >= 1 && r.bits <= 253 && 8 * (size_t)r.mag < P.mags.size(), "level %zu run %zu: magnitude", lv, t);
      CHECK(lv == 0 || (r.mag == 0 && r.bits == 1), "level %zu run %zu has a coefficient", lv, t);
      CHECK((size_t)r.off + r.len <= n_src, "level %zu run %zu reads past its source", lv, t);
      if (t) { const ColsumRun& q = L.runs[t - 1]; CHECK(q.bits > r.bits || (q.bits == r.bits && q.len >= r.len), "level %zu: run %zu out of order", lv, t); }
      for (uint32_t k = 0; k < r.len; k++) read[r.off + k]++;
      if (r.dst & COLSUM_FINAL) CHECK((r.dst & ~COLSUM_FINAL) < P.n_cols, "level %zu run %zu: column", lv, t);
      else { CHECK(r.dst < L.n_partials, "level %zu run %zu: slot", lv, t); written[r.dst]++; }
    }
    for (uint32_t x : read) CHECK(x == 1, "level %zu reads an entry or a partial %u times", lv, x);
    for (uint32_t x : written) CHECK(x == 1, "level %zu writes a slot %u times", lv, x);
  }
  CHECK(P.levels[n_lv - 1].n_partials == 0, "the last level leaves partials");
  // a run's column: where its sum ends — from the last level down
  std::vector<std::vector<uint32_t>> col_of(n_lv);
  std::vector<uint32_t> finals(P.n_cols, 0);
  for (size_t lv = n_lv; lv-- > 0;) {
    const ColsumLevel& L = P.levels[lv];
    std::vector<uint32_t> col_of_slot(L.n_partials, 0);
    if (lv + 1 < n_lv) for (size_t t = 0; t < P.levels[lv + 1].runs.size(); t++) { const ColsumRun& r = P.levels[lv + 1].runs[t]; for (uint32_t k = 0; k < r.len; k++) col_of_slot[r.off + k] = col_of[lv + 1][t]; }
    col_of[lv].resize(L.runs.size());
    for (size_t t = 0; t < L.runs.size(); t++) {
      const ColsumRun& r = L.runs[t];
      if (r.dst & COLSUM_FINAL) { col_of[lv][t] = r.dst & ~COLSUM_FINAL; finals[col_of[lv][t]]++; } else col_of[lv][t] = col_of_slot[r.dst];
    }
    // the slots of a column lie side by side: no column comes back after another
    std::vector<bool> closed(P.n_cols, false);
    for (size_t s = 0; s < col_of_slot.size(); s++) {
      CHECK(!closed[col_of_slot[s]], "level %zu: the slots of column %u are not contiguous", lv, col_of_slot[s]);
      if (s + 1 < col_of_slot.size() && col_of_slot[s + 1] != col_of_slot[s]) closed[col_of_slot[s]] = true;
    }
  }
  // level 0 against the matrix: every non-zero entry in exactly one run, of its column and its magnitude
  struct Want { uint32_t word; Fr mag; bool used; };
  std::vector<std::vector<Want>> want(P.n_cols);
  for (size_t r = 0; r < n_rows; r++) for (uint32_t k = row_ptr[r]; k < row_ptr[r + 1]; k++) {
    const Fr c = dict[coef[k]], neg = Fr::neg(c);
    if (c.is_zero()) continue;
    bool minus = false;
    for (int i = 7; i >= 0; i--) if (neg.v[i] != c.v[i]) { minus = neg.v[i] < c.v[i]; break; }
    want[col[k]].push_back({(uint32_t)((row_base + r) << 1) | (minus ? 1u : 0u), minus ? neg : c, false});
  }
  Fr one = Fr::zero(); one.v[0] = 1;
  for (const ColsumUnit& u : units) want[u.col].push_back({u.row << 1, one, false});
  size_t n_want = 0;
  for (const auto& w : want) n_want += w.size();
  CHECK(n_want == P.entries.size(), "%zu entries planned, %zu non-zero in the matrix", P.entries.size(), n_want);
  for (size_t t = 0; t < P.levels[0].runs.size(); t++) {
    const ColsumRun& r = P.levels[0].runs[t];
    int bits = 0;
    for (int i = 7; i >= 0 && !bits; i--) if (P.mags[8 * r.mag + i]) bits = 32 * i + 32 - __builtin_clz(P.mags[8 * r.mag + i]);
    CHECK((int)r.bits == bits, "level 0 run %zu: bits %u of a magnitude of %d", t, r.bits, bits);
    for (uint32_t k = 0; k < r.len; k++) {
      bool found = false;
      for (Want& w : want[col_of[0][t]]) if (!w.used && w.word == P.entries[r.off + k] && !memcmp(w.mag.v, &P.mags[8 * r.mag], 32)) { w.used = found = true; break; }
      CHECK(found, "level 0 run %zu: entry %u is not one of column %u with the run's magnitude", t, k, col_of[0][t]);
    }
  }
  for (uint32_t j = 0; j < P.n_cols; j++) CHECK(finals[j] == (want[j].empty() ? 0u : 1u), "column %u is written %u times", j, finals[j]);
}

static std::vector<Pt> run_levels(const ColsumPlan& P, const std::vector<Pt>& pts) {
  std::vector<Pt> out(P.n_cols), part[2];
  for (Pt& p : out) { p.x = Fq::zero(); p.y = Fq::zero(); }
  for (size_t lv = 0; lv < P.levels.size(); lv++) {
    const ColsumLevel& L = P.levels[lv];
    part[lv & 1].assign(L.n_partials, Pt{Fq::zero(), Fq::zero()});
    const Pt* src = lv ? part[(lv - 1) & 1].data() : pts.data();
    for (size_t t = 0; t < L.runs.size(); t++) colsum_run<Fq>(t, L.runs.data(), lv ? nullptr : P.entries.data(), P.mags.data(), src, part[lv & 1].data(), out.data());
  }
  return out;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: colsum_plan_check CASES.txt\n"); return 2; }
  std::ifstream in(argv[1]);
  if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  const Pt g = generator();
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string tag, name;
    if (!(ls >> tag >> name)) continue;
    if (tag == "HQ") {
      size_t n; std::string t;
      ls >> n >> t;
      const Fr dinv = from_hex<Fr>(t);
      std::vector<Pt> pts;
      while (ls >> t) pts.push_back(to_affine(pt_scalar_mul(g, from_hex<Fr>(t).v)));
      CHECK(n >= 2 && pts.size() == 2 * n - 1, "h query: %zu points for n = %zu", pts.size(), n);
      std::vector<Pt> out(n - 1);
      for (size_t j = 0; j + 1 < n; j++) { pt_diff(j, n, pts.data(), out.data()); out[j] = to_affine(pt_scalar_mul(out[j], dinv.v)); }
      printf("OUT %s", name.c_str());
      for (const Pt& p : out) { print_fq(p.x); print_fq(p.y); }
      putchar('\n');
      continue;
    }
    if (tag != "CASE") { fprintf(stderr, "bad line: %s\n", tag.c_str()); return 2; }
    size_t n_rows, n_cols, n_dict;
    ls >> n_rows >> n_cols >> n_dict;
    const std::vector<uint32_t> row_ptr = numbers<uint32_t>(in, "ROWPTR", n_rows + 1);
    const size_t nnz = row_ptr.back();
    const std::vector<uint32_t> col = numbers<uint32_t>(in, "COL", nnz), coef = numbers<uint32_t>(in, "COEF", nnz);
    const std::vector<Fr> dict = numbers<Fr>(in, "DICT", n_dict), sc = numbers<Fr>(in, "SCALARS", n_rows);
    ColsumPlan P; std::string err;
    const ColsumPart part{row_ptr.data(), col.data(), coef.data(), (uint32_t)n_rows, 0u};
    CHECK(colsum_plan(&part, 1, nullptr, 0, (const uint32_t*)dict.data(), n_dict, BnFr::MOD.w, (uint32_t)n_cols, (uint32_t)n_rows, &P, &err), "%s", err.c_str());
    check_plan(name, P, row_ptr, col, coef, dict, 0u, {});
    std::vector<Pt> pts(n_rows);
    for (size_t r = 0; r < n_rows; r++) pts[r] = to_affine(pt_scalar_mul(g, sc[r].v));
    const std::vector<Pt> out = run_levels(P, pts);
    // plain sums: every entry's c·P over all 254 bits, added up
    std::vector<XYZZ<Fq>> sum(n_cols, XYZZ<Fq>::identity());
    for (size_t r = 0; r < n_rows; r++) for (uint32_t k = row_ptr[r]; k < row_ptr[r + 1]; k++) { const XYZZ<Fq> t = pt_scalar_mul(pts[r], dict[coef[k]].v); add_full(sum[col[k]], t); }
    for (size_t j = 0; j < n_cols; j++) CHECK(same(out[j], to_affine(sum[j])), "column %zu differs from the plain sum", j);
    // the plan with a part at a row offset and unit entries: the same sums shifted, plus the named points
    { std::vector<Pt> shifted(n_rows + 3, Pt{Fq::zero(), Fq::zero()});
      for (size_t r = 0; r < n_rows; r++) shifted[r + 3] = pts[r];
      shifted[1] = g;
      const ColsumPart part3{row_ptr.data(), col.data(), coef.data(), (uint32_t)n_rows, 3u};
      const ColsumUnit units[2] = {{1u, 0u}, {1u, (uint32_t)n_cols - 1}};
      ColsumPlan P3;
      CHECK(colsum_plan(&part3, 1, units, 2, (const uint32_t*)dict.data(), n_dict, BnFr::MOD.w, (uint32_t)n_cols, (uint32_t)n_rows + 3, &P3, &err), "%s", err.c_str());
      check_plan(name, P3, row_ptr, col, coef, dict, 3u, {units[0], units[1]});
      const std::vector<Pt> out3 = run_levels(P3, shifted);
      add_mixed(sum[0], g); add_mixed(sum[n_cols - 1], g);
      for (size_t j = 0; j < n_cols; j++) CHECK(same(out3[j], to_affine(sum[j])), "with unit entries: column %zu differs from the plain sum", j);
    }
    printf("OUT %s", name.c_str());
    for (const Pt& p : out) { print_fq(p.x); print_fq(p.y); }
    printf("\nMAGS %s", name.c_str());
    for (size_t k = 0; k < P.mags.size(); k += 8) { putchar(' '); for (int i = 7; i >= 0; i--) printf("%08x", P.mags[k + i]); }
    printf("\nENTRIES %s", name.c_str());
    for (uint32_t e : P.entries) printf(" %u", e);
    putchar('\n');
    for (size_t lv = 0; lv < P.levels.size(); lv++) {
      printf("LEVEL %s %zu %u", name.c_str(), lv, P.levels[lv].n_partials);
      for (const ColsumRun& r : P.levels[lv].runs) printf(" %u %u %u %u %u", r.off, r.len, r.mag, r.bits, r.dst);
      putchar('\n');
    }
  }
  return 0;
}
