// A contribution to a powers-of-tau string (vimz_amd/csrc/g16_powers_contrib.hip and .hpp) on the CPU: the functions k_power_vec and k_scale_points_by call with their
// thread index (g16_point_stage.hpp: pt_power, pt_scale_by) looped over every thread, and the host's record maker, record checker and record parser
// (g16_powers_contrib.hpp), with the canonical Fp fields.  Reads lines from the file named on the command line:
//     POWER LABEL COUNT w                        the power vector of COUNT entries (w: hex below r) from a heap block of exactly 32·COUNT bytes — every thread of the grid
//                                                (blocks of PT_BLOCK) under the kernel's guard, the block checked after EVERY thread: only that thread's slot may have
//                                                changed.  Prints LABEL and w^i as canonical hex.
//     SCALE LABEL GROUP N INPLACE w c s_0 ..     the points P_i = [s_i]G of G1 (GROUP 1) or G2 (2) (hex below r; 0: the identity) from a heap block of exactly N points,
//                                                scaled by c·w^i — into another block of N points, or with INPLACE = 1 where they lie —, checked the same way after every
//                                                thread.  Prints LABEL and the N points (canonical hex coordinates; the identity as zeros).
//     RECORD LABEL b_tau b_alpha b_beta s_tau s_alpha s_beta k_tau k_alpha k_beta
//                                                make_powers_record over the points [b]G1: prints LABEL, the record's 488 bytes as hex, then what powers_record_knowledge
//                                                says of it (0), of it with z_s + 1 for s = tau', alpha', beta' (1, 2, 4), and of it over another base (7).
//     PARSE LABEL HEX                            powers_records_layout over exactly those bytes (a heap block of that very size): prints LABEL ok N, or LABEL err J MESSAGE.
// Nothing else is judged here: tests/test_powers_contrib_host.py compares.  No HIP: g++ -std=c++17 -fsanitize=address,undefined -I vimz_amd/csrc.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "g16_powers_contrib.hpp"

using namespace vz;
using namespace vz::powc;
using vz::pairing::Fq2;

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
static Fq fq_hex(const std::string& h) { return Fq::to_mont(from_hex<Fq>(h)); }
static void generator(G1A* g) { g->x = Fq::one(); g->y = Fq::dbl(Fq::one()); }
static void generator(G2A* g) {      // the generator of G2 every BN254 library uses (EIP-197)
  g->x.c0 = fq_hex("1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed"); g->x.c1 = fq_hex("198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2");
  g->y.c0 = fq_hex("12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa"); g->y.c1 = fq_hex("090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b");
}
static void print_words(const uint32_t* v) { putchar(' '); for (int i = 7; i >= 0; i--) printf("%08x", v[i]); }
template <class A>
static void print_point(const A& p) {
  const Fq* c = (const Fq*)&p;
  for (size_t k = 0; k < sizeof(A) / sizeof(Fq); k++) print_words(Fq::from_mont(c[k]).v);
}

// heap blocks of exactly the size the threads may touch: the sanitizer sees a read or write past them
template <class T>
struct Block {
  T* p; size_t n;
  explicit Block(size_t count) : p((T*)malloc(count * sizeof(T))), n(count) { memset((void*)p, 0xa5, count * sizeof(T)); }
  ~Block() { free(p); }
  Block(const Block&) = delete;
};

// after thread t (own = it ran under the guard) only slot t of `now` may differ from `seen`, and must when its value changes; `seen` is brought up to date
template <class T>
static bool only_own_slot(const std::string& label, const T* now, std::vector<T>& seen, size_t t, bool own, bool must_change) {
  for (size_t k = 0; k < seen.size(); k++) {
    const bool same = !memcmp((const void*)&now[k], (const void*)&seen[k], sizeof(T));
    if (!(own && k == t) && !same) { fprintf(stderr, "%s: thread %zu wrote slot %zu\n", label.c_str(), t, k); return false; }
    if (own && k == t && must_change && same) { fprintf(stderr, "%s: thread %zu left its own slot\n", label.c_str(), t); return false; }
  }
  if (own) memcpy((void*)&seen[t], (const void*)&now[t], sizeof(T));
  return true;
}

static int bitlen(size_t v) { int b = 0; while (v) { b++; v >>= 1; } return b; }
struct Pw { uint32_t w[8]; };

static int power(const std::string& label, size_t count, const std::string& w_hex) {
  const Fr w = Fr::to_mont(from_hex<Fr>(w_hex));
  Block<Pw> pw(count);
  std::vector<Pw> seen(pw.p, pw.p + count);
  const size_t blocks = (count + PT_BLOCK - 1) / PT_BLOCK;
  for (size_t t = 0; t < blocks * PT_BLOCK; t++) {
    if (t < count) pt_power(t, bitlen(count - 1), w, (uint32_t*)pw.p);      // (the kernel's guard)
    if (!only_own_slot(label, pw.p, seen, t, t < count, true)) return 1;
  }
  fputs(label.c_str(), stdout);
  for (size_t i = 0; i < count; i++) { Fr m; memcpy(m.v, pw.p[i].w, 32); print_words(Fr::from_mont(m).v); }
  putchar('\n');
  return 0;
}

template <class A>
static int scale(const std::string& label, size_t n, bool in_place, const std::string& w_hex, const std::string& c_hex, std::istringstream& ls) {
  const Fr w = Fr::to_mont(from_hex<Fr>(w_hex)), c = Fr::to_mont(from_hex<Fr>(c_hex));
  A g; generator(&g);
  Block<A> in(n), other(in_place ? 1 : n);
  std::string tok;
  for (size_t i = 0; i < n; i++) {
    if (!(ls >> tok)) { fprintf(stderr, "%s: too few scalars\n", label.c_str()); return 2; }
    in.p[i] = to_affine(pt_scalar_mul(g, from_hex<Fr>(tok).v));
  }
  Block<Pw> pw(n);
  for (size_t t = 0; t < n; t++) pt_power(t, bitlen(n - 1), w, (uint32_t*)pw.p);
  A* out = in_place ? in.p : other.p;
  std::vector<A> seen(out, out + n), seen_in(in.p, in.p + n);
  // (in place a slot need not change: the identity stays, and c·w^i may be one)
  const size_t blocks = (n + PT_BLOCK - 1) / PT_BLOCK;
  for (size_t t = 0; t < blocks * PT_BLOCK; t++) {
    if (t < n) pt_scale_by(t, (const A*)in.p, (const uint32_t*)pw.p, c, out);
    if (!only_own_slot(label, out, seen, t, t < n, !in_place)) return 1;
    if (!in_place && !only_own_slot(label + " (input)", in.p, seen_in, t, false, false)) return 1;
  }
  fputs(label.c_str(), stdout);
  for (size_t i = 0; i < n; i++) print_point(out[i]);
  putchar('\n');
  return 0;
}

static int record(const std::string& label, std::istringstream& ls) {
  std::string tok[9];
  for (auto& t : tok) if (!(ls >> t)) { fprintf(stderr, "bad RECORD\n"); return 2; }
  G1A g; generator(&g);
  G1A before[3], after[3], T[3];
  Fr secrets[3], nonces[3];
  for (int s = 0; s < 3; s++) {
    before[s] = to_affine(pt_scalar_mul(g, from_hex<Fr>(tok[s]).v));
    secrets[s] = Fr::to_mont(from_hex<Fr>(tok[3 + s])); nonces[s] = Fr::to_mont(from_hex<Fr>(tok[6 + s]));
  }
  uint64_t before_words[24];
  for (int s = 0; s < 3; s++) put_g1(before_words + 8 * s, before[s]);
  std::vector<uint64_t> rec(RECORD_WORDS);      // (a heap block of the record's exact size)
  make_powers_record(before, secrets, nonces, rec.data());
  fputs(label.c_str(), stdout); putchar(' ');
  for (size_t i = 0; i < 8 * RECORD_WORDS; i++) printf("%02x", ((const uint8_t*)rec.data())[i]);
  for (int s = 0; s < 3; s++)
    if (!get_g1(rec.data() + REC_A + 8 * s, &after[s]) || !get_g1(rec.data() + REC_T + 8 * s, &T[s])) { fprintf(stderr, "%s: the record's points\n", label.c_str()); return 1; }
  printf(" %u", powers_record_knowledge(before_words, before, after, T, rec.data()));
  for (int s = 0; s < 3; s++) {
    std::vector<uint64_t> off = rec; off[REC_Z + 4 * s] += 1;
    printf(" %u", powers_record_knowledge(before_words, before, after, T, off.data()));
  }
  uint64_t other_words[24];
  for (int s = 0; s < 3; s++) put_g1(other_words + 8 * s, after[s]);
  printf(" %u\n", powers_record_knowledge(other_words, after, after, T, rec.data()));
  return 0;
}

static void parse(const std::string& label, const std::string& hex) {
  std::vector<uint8_t> b;
  if (hex != "-") for (size_t i = 0; i + 1 < hex.size(); i += 2) b.push_back((uint8_t)std::stoul(hex.substr(i, 2), nullptr, 16));
  uint8_t* exact = (uint8_t*)malloc(b.size() ? b.size() : 1);
  if (!b.empty()) memcpy(exact, b.data(), b.size());
  size_t n = 0;
  const char* why = powers_records_layout(exact, b.size(), &n);
  if (why) printf("%s err %zu %s\n", label.c_str(), n, why); else printf("%s ok %zu\n", label.c_str(), n);
  free(exact);
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: powers_contrib_check CASES.txt\n"); return 2; }
  std::ifstream in(argv[1]);
  if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  if (!vz::pairing::consts().ok) { fprintf(stderr, "pairing constants\n"); return 1; }
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string what, label;
    if (!(ls >> what)) continue;
    if (!(ls >> label)) { fprintf(stderr, "a line without a label\n"); return 2; }
    int rc = 0;
    if (what == "POWER") { size_t n = 0; std::string w; if (!(ls >> n >> w) || !n || n > 4096) { fprintf(stderr, "bad POWER\n"); return 2; } rc = power(label, n, w); }
    else if (what == "SCALE") {
      int group = 0, in_place = 0; size_t n = 0; std::string w, c;
      if (!(ls >> group >> n >> in_place >> w >> c) || (group != 1 && group != 2) || !n || n > 4096) { fprintf(stderr, "bad SCALE\n"); return 2; }
      rc = group == 1 ? scale<G1A>(label, n, in_place != 0, w, c, ls) : scale<G2A>(label, n, in_place != 0, w, c, ls);
    }
    else if (what == "RECORD") rc = record(label, ls);
    else if (what == "PARSE") { std::string hex; if (!(ls >> hex)) { fprintf(stderr, "bad PARSE\n"); return 2; } parse(label, hex); }
    else { fprintf(stderr, "bad line: %s\n", what.c_str()); return 2; }
    if (rc) return rc;
  }
  return 0;
}
