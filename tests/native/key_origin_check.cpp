// The scalar kernels of the origin check of a key (vimz_amd/csrc/g16_key_origin.hip) on the CPU: the functions k_spmv3_dict and k_origin_vec call with their thread
// index (g16_key_origin_stage.hpp: spmv_dict_row, ko_expand, ko_unit, ko_h_scalar, ko_add) looped over every thread of their grids under the kernels' guards, every
// array a heap block of its exact size.  Reads lines from the file named on the command line (numbers decimal, field elements hex below r, canonical):
//     SPMV LABEL m n_c n n_dict  dict..  v(m)..  then for A, B, C:  nnz  row_ptr(n_c + 1)..  col(nnz)..  coef(nnz)..
//         the three products as g16_spmv3_dict queues them — blocks of KO_BLOCK threads over n rows, the matrix in the grid's second dimension —, the outputs checked
//         after EVERY thread: only that thread's slot may have changed; then each against a naive dense product (the matrix expanded to n_c x m, duplicates added up).
//         Prints LABEL and the 3n outputs.
//     EXPAND LABEL count lo hi scale  rho(count)..      ko_expand over count threads; prints the count elements
//     UNITS LABEL n_c n_pub n  u(n)..  v(n_pub + 1)..   ko_unit over n_pub + 1 threads; prints u
//     HSCALARS LABEL n  rho(n − 1)..                    ko_h_scalar over 2n − 1 threads; prints them
//     ADD LABEL n  a(n)..  b(n)..                       ko_add; prints the sums
// Nothing else is judged here: tests/test_key_origin_host.py compares with Python integers.  No HIP: g++ -std=c++17 -fsanitize=address,undefined -I vimz_amd/csrc.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "g16_key_origin_stage.hpp"

using namespace vz;

static KoFr from_hex(const std::string& h) {      // canonical words of a hex integer below 2^256
  KoFr c = KoFr::zero();
  int bit = 0;
  for (size_t i = h.size(); i-- > 0; bit += 4) {
    const char ch = h[i];
    const uint32_t d = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : 16;
    if (d > 15 || bit >= 256) { fprintf(stderr, "bad hex %s\n", h.c_str()); exit(2); }
    c.v[bit >> 5] |= d << (bit & 31);
  }
  return c;
}
static void print_fe(const KoFr& mont) { const KoFr c = KoFr::from_mont(mont); putchar(' '); for (int i = 7; i >= 0; i--) printf("%08x", c.v[i]); }
static bool take(std::istringstream& ls, size_t* out) { return (bool)(ls >> *out); }
// count elements as Montgomery words, in a block of exactly that size
static bool elements(std::istringstream& ls, size_t count, std::vector<uint32_t>* out) {
  out->assign(8 * count, 0);
  std::string tok;
  for (size_t i = 0; i < count; i++) { if (!(ls >> tok)) return false; ko_store(out->data(), i, KoFr::to_mont(from_hex(tok))); }
  return true;
}
// count scalars of 128 bits as 4 words each
static bool rhos(std::istringstream& ls, size_t count, std::vector<uint32_t>* out) {
  out->assign(4 * count, 0);
  std::string tok;
  for (size_t i = 0; i < count; i++) { if (!(ls >> tok) || tok.size() > 32) return false; const KoFr c = from_hex(tok); memcpy(out->data() + 4 * i, c.v, 16); }
  return true;
}
static bool indices(std::istringstream& ls, size_t count, std::vector<uint32_t>* out) {
  out->assign(count, 0);
  for (size_t i = 0; i < count; i++) { size_t x; if (!take(ls, &x)) return false; (*out)[i] = (uint32_t)x; }
  return true;
}
static void print_vector(const std::string& label, const std::vector<uint32_t>& v) {
  fputs(label.c_str(), stdout);
  for (size_t i = 0; i < v.size() / 8; i++) print_fe(ko_load(v.data(), i));
  putchar('\n');
}

static int spmv(const std::string& label, std::istringstream& ls) {
  size_t m, n_c, n, n_dict;
  if (!take(ls, &m) || !take(ls, &n_c) || !take(ls, &n) || !take(ls, &n_dict) || n < n_c || !m || m > 4096 || n > 4096) { fprintf(stderr, "bad SPMV\n"); return 2; }
  std::vector<uint32_t> dict, v, row_ptr[3], col[3], coef[3];
  if (!elements(ls, n_dict, &dict) || !elements(ls, m, &v)) { fprintf(stderr, "%s: too few elements\n", label.c_str()); return 2; }
  for (int q = 0; q < 3; q++) {
    size_t nnz;
    if (!take(ls, &nnz) || !indices(ls, n_c + 1, &row_ptr[q]) || !indices(ls, nnz, &col[q]) || !indices(ls, nnz, &coef[q])) { fprintf(stderr, "%s: matrix %d\n", label.c_str(), q); return 2; }
    for (size_t k = 0; k < nnz; k++) if (col[q][k] >= m || coef[q][k] >= n_dict) { fprintf(stderr, "%s: an index out of bounds (the host refuses such a matrix)\n", label.c_str()); return 2; }
  }
  std::vector<uint32_t> out(8 * 3 * n, 0xa5a5a5a5u), seen = out;
  const size_t blocks = (n + KO_BLOCK - 1) / KO_BLOCK;
  for (unsigned q = 0; q < 3; q++)
    for (size_t t = 0; t < blocks * KO_BLOCK; t++) {
      if (t < n) spmv_dict_row(t, (uint32_t)n_c, row_ptr[q].data(), col[q].data(), coef[q].data(), dict.data(), v.data(), out.data() + 8 * n * q);      // (the kernel's guard)
      for (size_t k = 0; k < 3 * n; k++) {
        const bool own = t < n && k == q * n + t, same = !memcmp(&out[8 * k], &seen[8 * k], 32);
        if (own == same) { fprintf(stderr, "%s: thread (%zu, %u) %s slot %zu\n", label.c_str(), t, q, own ? "left its own" : "wrote", k); return 1; }
      }
      memcpy(&seen[8 * (q * n + (t < n ? t : 0))], &out[8 * (q * n + (t < n ? t : 0))], 32);
    }
  for (int q = 0; q < 3; q++) {      // the naive dense product
    std::vector<KoFr> dense(n_c * m, KoFr::zero());
    for (size_t r = 0; r < n_c; r++) for (uint32_t k = row_ptr[q][r]; k < row_ptr[q][r + 1]; k++) dense[r * m + col[q][k]] = KoFr::add(dense[r * m + col[q][k]], ko_load(dict.data(), coef[q][k]));
    for (size_t r = 0; r < n; r++) {
      KoFr acc = KoFr::zero();
      if (r < n_c) for (size_t j = 0; j < m; j++) acc = KoFr::add(acc, KoFr::mul(dense[r * m + j], ko_load(v.data(), j)));
      if (!acc.eq(ko_load(out.data(), q * n + r))) { fprintf(stderr, "%s: matrix %d row %zu differs from the dense product\n", label.c_str(), q, r); return 1; }
    }
  }
  print_vector(label, out);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: key_origin_check CASES.txt\n"); return 2; }
  std::ifstream in(argv[1]);
  if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string what, label;
    if (!(ls >> what)) continue;
    if (!(ls >> label)) { fprintf(stderr, "a line without a label\n"); return 2; }
    if (what == "SPMV") { const int rc = spmv(label, ls); if (rc) return rc; continue; }
    size_t a = 0, b = 0, c = 0;
    std::vector<uint32_t> x, y, out;
    std::string tok;
    if (what == "EXPAND") {
      if (!take(ls, &a) || !take(ls, &b) || !take(ls, &c) || !(ls >> tok) || !rhos(ls, a, &x)) { fprintf(stderr, "bad EXPAND\n"); return 2; }
      const KoFr scale_r2 = KoFr::to_mont(KoFr::to_mont(from_hex(tok)));
      out.assign(8 * a, 0xa5a5a5a5u);
      for (size_t i = 0; i < a; i++) ko_expand(i, b, c, x.data(), scale_r2, out.data());
    } else if (what == "UNITS") {
      size_t n = 0;
      if (!take(ls, &a) || !take(ls, &b) || !take(ls, &n) || a + b + 1 > n || !elements(ls, n, &out) || !elements(ls, b + 1, &x)) { fprintf(stderr, "bad UNITS\n"); return 2; }
      for (size_t i = 0; i <= b; i++) ko_unit(i, (uint32_t)a, x.data(), out.data());
    } else if (what == "HSCALARS") {
      if (!take(ls, &a) || a < 2 || !rhos(ls, a - 1, &x)) { fprintf(stderr, "bad HSCALARS\n"); return 2; }
      out.assign(8 * (2 * a - 1), 0xa5a5a5a5u);
      for (size_t k = 0; k < 2 * a - 1; k++) ko_h_scalar(k, a, x.data(), KoFr::r2(), out.data());
    } else if (what == "ADD") {
      if (!take(ls, &a) || !elements(ls, a, &x) || !elements(ls, a, &y)) { fprintf(stderr, "bad ADD\n"); return 2; }
      out.assign(8 * a, 0xa5a5a5a5u);
      for (size_t i = 0; i < a; i++) ko_add(i, x.data(), y.data(), out.data());
    } else { fprintf(stderr, "bad line: %s\n", what.c_str()); return 2; }
    print_vector(label, out);
  }
  return 0;
}
