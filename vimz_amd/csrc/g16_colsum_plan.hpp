// The host plan of the column sums of a Groth16 set-up from a powers-of-tau string (g16_powers.hpp: g16_column_sums):
//     Q_j = Σ_{r, k: col[k] = j} dict[coef[k]] · P_r        over the entries of a CSR matrix of the builder (cb::Csr: row_ptr, col, coef) and points P_r
// as LEVELS of RUNS, one thread of k_col_runs per run (g16_point_stage.hpp: colsum_run).  A pure function of the matrix: it never reads a point, and every loop
// bound of the kernel is a number written here.  No HIP, no field arithmetic: the dictionary comes as canonical words, the group's order as 8 words.
//
// Level 0 cuts every column's entries into runs of ONE column and ONE coefficient magnitude |c| = min(c, r − c), the sign kept per entry, COLSUM_CHUNK entries at
// the most: the thread sums ±P over its entries and multiplies ONCE by |c| over exactly bitlen(|c|) bits — nothing when |c| = 1.  Entries whose coefficient
// is 0 are dropped.  Level k >= 1 sums the partials of level k − 1 per column in segments of at most COLSUM_CHUNK, until every column has one partial; a run
// that is its column's only one writes the OUTPUT (dst = COLSUM_FINAL | column), the others the level's partial array, a column's slots side by side so that
// the next level reads them as one range.  Columns without entries are in no run: the caller presets the output to the identity.
// Within a level the runs are ordered by (bitlen(|c|), length) descending: the 64 consecutive threads of a wave do alike work.
#pragma once
#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

namespace vz {

constexpr uint32_t COLSUM_CHUNK = 1024;            // entries (level 0) or partials (above) of a run, at the most
constexpr uint32_t COLSUM_FINAL = 0x80000000u;     // in ColsumRun::dst: the run writes the output of the column in the low bits

// one thread's work.  Level 0: entries[off .. off + len) name the points; above: the previous level's partials off .. off + len.  mag: the index of |c| in
// the magnitude table (0: one), bits = bitlen(|c|) >= 1; above level 0 both are (0, 1).  dst: a slot of this level's partials, or COLSUM_FINAL | column.
struct ColsumRun { uint32_t off, len, mag, bits, dst; };

struct ColsumPart {              // a matrix whose row r multiplies the point row_base + r
  const uint32_t *row_ptr, *col, *coef; uint32_t n_rows, row_base;
};
struct ColsumUnit { uint32_t row, col; };      // an extra entry with coefficient one: point `row` into column `col`

struct ColsumLevel { std::vector<ColsumRun> runs; uint32_t n_partials = 0; };
struct ColsumPlan {
  uint32_t n_cols = 0, n_points = 0;           // outputs; points the entries may name
  std::vector<uint32_t> entries;               // level 0's permuted entries: point << 1 | sign
  std::vector<uint32_t> mags;                  // 8 canonical words a magnitude; entry 0 is one
  std::vector<ColsumLevel> levels;
  uint32_t max_col_runs = 0;                   // the level-0 runs of the column that has the most (for the record: profiles/decider_powers.txt)
  size_t max_partials() const { size_t m = 0; for (const ColsumLevel& l : levels) m = std::max<size_t>(m, l.n_partials); return m; }
};

namespace colsum_detail {
inline int bitlen256(const uint32_t* w) { for (int i = 7; i >= 0; i--) if (w[i]) return 32 * i + 32 - __builtin_clz(w[i]); return 0; }
inline bool less256(const uint32_t* a, const uint32_t* b) { for (int i = 7; i >= 0; i--) if (a[i] != b[i]) return a[i] < b[i]; return false; }
// runs of one level in the order the kernel takes them, and the partial slots: a column's side by side, in column order
inline void finish_level(ColsumLevel& lv, std::vector<uint32_t>& col_of_run, std::vector<std::pair<uint32_t, uint32_t>>& next /* column -> (first slot, slots) of those with more than one */) {
  next.clear();
  uint32_t slot = 0;
  for (size_t i = 0; i < lv.runs.size();) {      // (runs arrive grouped by column)
    size_t j = i;
    while (j < lv.runs.size() && col_of_run[j] == col_of_run[i]) j++;
    if (j - i == 1) lv.runs[i].dst = COLSUM_FINAL | col_of_run[i];
    else { next.push_back({col_of_run[i], slot}); for (size_t k = i; k < j; k++) lv.runs[k].dst = slot++; }
    i = j;
  }
  lv.n_partials = slot;
  std::stable_sort(lv.runs.begin(), lv.runs.end(), [](const ColsumRun& a, const ColsumRun& b) { return a.bits != b.bits ? a.bits > b.bits : a.len > b.len; });
}
}  // namespace colsum_detail

// false (and why in *err): an entry names a column, a coefficient or a point out of range, a coefficient is not below r, or the sizes exceed 31 bits
inline bool colsum_plan(const ColsumPart* parts, size_t n_parts, const ColsumUnit* units, size_t n_units, const uint32_t* dict_canon, size_t n_dict,
                        const uint32_t r_mod[8], uint32_t n_cols, uint32_t n_points, ColsumPlan* out, std::string* err) {
  using namespace colsum_detail;
  auto fail = [&](const char* m) { if (err) *err = m; return false; };
  if (n_cols >= COLSUM_FINAL || n_points >= COLSUM_FINAL) return fail("column sums: more than 2^31 columns or points");
  ColsumPlan P; P.n_cols = n_cols; P.n_points = n_points;
  // coefficient -> magnitude, sign, bit length (0: dropped)
  struct Coef { uint32_t mag, sign, bits; };
  std::vector<Coef> cf(n_dict);
  std::map<std::array<uint32_t, 8>, uint32_t> seen;
  { std::array<uint32_t, 8> one{}; one[0] = 1; seen[one] = 0; P.mags.assign(one.begin(), one.end()); }
  for (size_t i = 0; i < n_dict; i++) {
    const uint32_t* c = dict_canon + 8 * i;
    if (!less256(c, r_mod)) return fail("column sums: a coefficient is not below the group's order");
    std::array<uint32_t, 8> neg, mag; uint64_t br = 0;
    for (int k = 0; k < 8; k++) { const uint64_t d = (uint64_t)r_mod[k] - c[k] - br; neg[k] = (uint32_t)d; br = (d >> 32) & 1; }
    const bool minus = less256(neg.data(), c);
    for (int k = 0; k < 8; k++) mag[k] = minus ? neg[k] : c[k];
    cf[i].bits = (uint32_t)bitlen256(mag.data()); cf[i].sign = minus ? 1u : 0u; cf[i].mag = 0;
    if (!cf[i].bits) continue;
    auto it = seen.find(mag);
    if (it == seen.end()) { it = seen.emplace(mag, (uint32_t)(P.mags.size() / 8)).first; P.mags.insert(P.mags.end(), mag.begin(), mag.end()); }
    cf[i].mag = it->second;
  }
  // the entries by column (a counting sort), then by magnitude inside a column
  std::vector<uint64_t> start((size_t)n_cols + 1, 0);
  uint64_t total = 0;
  for (size_t p = 0; p < n_parts; p++) {
    const ColsumPart& M = parts[p];
    if ((uint64_t)M.row_base + M.n_rows > n_points) return fail("column sums: a row names a point beyond the array");
    for (uint32_t r = 0; r < M.n_rows; r++) {
      if (M.row_ptr[r + 1] < M.row_ptr[r]) return fail("column sums: row_ptr decreases");
      for (uint32_t k = M.row_ptr[r]; k < M.row_ptr[r + 1]; k++) {
        if (M.col[k] >= n_cols) return fail("column sums: a column index is out of range");
        if (M.coef[k] >= n_dict) return fail("column sums: a coefficient index is out of range");
        if (cf[M.coef[k]].bits) { start[M.col[k] + 1]++; total++; }
      }
    }
  }
  for (size_t u = 0; u < n_units; u++) {
    if (units[u].col >= n_cols || units[u].row >= n_points) return fail("column sums: a unit entry is out of range");
    start[units[u].col + 1]++; total++;
  }
  if (total >= COLSUM_FINAL) return fail("column sums: more than 2^31 entries");
  for (size_t j = 0; j < n_cols; j++) start[j + 1] += start[j];
  struct Ent { uint32_t mag, word; };
  std::vector<Ent> ent(total);
  { std::vector<uint64_t> at(start.begin(), start.end() - 1);
    for (size_t p = 0; p < n_parts; p++) {
      const ColsumPart& M = parts[p];
      for (uint32_t r = 0; r < M.n_rows; r++) for (uint32_t k = M.row_ptr[r]; k < M.row_ptr[r + 1]; k++) {
        const Coef& c = cf[M.coef[k]];
        if (c.bits) ent[at[M.col[k]]++] = {c.mag, ((M.row_base + r) << 1) | c.sign};
      }
    }
    for (size_t u = 0; u < n_units; u++) ent[at[units[u].col]++] = {0u, units[u].row << 1};
  }
  std::vector<uint32_t> bits_of(P.mags.size() / 8);
  for (size_t k = 0; k < bits_of.size(); k++) bits_of[k] = (uint32_t)bitlen256(&P.mags[8 * k]);
  P.entries.resize(total);
  P.levels.emplace_back();
  std::vector<uint32_t> col_of_run;
  for (uint32_t j = 0; j < n_cols; j++) {
    const uint64_t lo = start[j], hi = start[j + 1];
    std::stable_sort(ent.begin() + lo, ent.begin() + hi, [](const Ent& a, const Ent& b) { return a.mag < b.mag; });
    const size_t runs_before = P.levels[0].runs.size();
    for (uint64_t i = lo; i < hi;) {
      uint64_t e = i;
      while (e < hi && ent[e].mag == ent[i].mag && e - i < COLSUM_CHUNK) e++;
      P.levels[0].runs.push_back({(uint32_t)i, (uint32_t)(e - i), ent[i].mag, bits_of[ent[i].mag], 0u});
      col_of_run.push_back(j);
      i = e;
    }
    P.max_col_runs = std::max<uint32_t>(P.max_col_runs, (uint32_t)(P.levels[0].runs.size() - runs_before));
  }
  for (uint64_t i = 0; i < total; i++) P.entries[i] = ent[i].word;
  std::vector<std::pair<uint32_t, uint32_t>> multi;      // columns with more than one partial: (column, first slot); its slots end where the next one's begin
  finish_level(P.levels[0], col_of_run, multi);
  while (!multi.empty()) {
    const uint32_t n_prev = P.levels.back().n_partials;
    ColsumLevel lv; col_of_run.clear();
    for (size_t c = 0; c < multi.size(); c++) {
      const uint32_t lo = multi[c].second, hi = c + 1 < multi.size() ? multi[c + 1].second : n_prev;
      for (uint32_t i = lo; i < hi; i += COLSUM_CHUNK) { lv.runs.push_back({i, std::min<uint32_t>(COLSUM_CHUNK, hi - i), 0u, 1u, 0u}); col_of_run.push_back(multi[c].first); }
    }
    finish_level(lv, col_of_run, multi);
    P.levels.push_back(std::move(lv));
  }
  *out = std::move(P);
  return true;
}

}  // namespace vz
