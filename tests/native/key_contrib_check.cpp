// Further delta contributions to a saved decider key (vimz_amd/csrc/g16_key_contrib.hip and .hpp) on the CPU: the function k_ratio_rlc calls with its thread index
// (g16_point_stage.hpp: pt_ratio_chunk, then colsum_run over ratio_sum_plan's plan of two columns) looped over every thread of both grid rows, and the host's blob
// parser, record maker and record checker (g16_key_contrib.hpp), with the canonical Fp fields.  Reads lines from the file named on the command line:
//     RATIO LABEL N b_0 .. a_0 .. rho_0 ..   the points before_i = [b_i]G1, after_i = [a_i]G1 (hex below r; 0: the identity) and N scalars rho (hex below 2^128): S and S' as
//                                            g16_ratio_rlc queues them — every thread of the grid (blocks of PT_BLOCK, rows 0 and 1) under the kernel's guard, the chunk
//                                            sums' array checked after EVERY thread: only that thread's slot may have changed —, then the plan's levels run by run.
//                                            Prints LABEL, S, S', then the 2·n_chunks chunk sums (canonical hex coordinates x y; the identity as zeros).
//     PARSE LABEL HEX                        key_layout over exactly those bytes (a heap block of that very size: the sanitizer sees a read past a truncated blob).
//                                            Prints LABEL ok WORDS OFF_LH N_LH, or LABEL err MESSAGE.
//     RECORD LABEL HEAD_HEX s delta k        make_record over the head's 88 bytes with delta1 = [s]G1, delta2 = [s]G2: prints LABEL, the record's 296 bytes as hex, and
//                                            what record_knowledge says of it, of it with z + 1, and of it over another base — "1 0 0".
// Nothing else is judged here: tests/test_key_contrib_host.py compares.  No HIP: g++ -std=c++17 -fsanitize=address,undefined -I vimz_amd/csrc.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "g16_key_contrib.hpp"

using namespace vz;
using namespace vz::keyc;

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
static std::vector<uint8_t> bytes_of(const std::string& h) {
  if (h == "-") return {};
  if (h.size() & 1) { fprintf(stderr, "odd hex\n"); exit(2); }
  std::vector<uint8_t> b(h.size() / 2);
  for (size_t i = 0; i < b.size(); i++) b[i] = (uint8_t)std::stoul(h.substr(2 * i, 2), nullptr, 16);
  return b;
}
static void print_point(const G1A& p) {
  for (const Fq* m : {&p.x, &p.y}) { const Fq c = Fq::from_mont(*m); putchar(' '); for (int i = 7; i >= 0; i--) printf("%08x", c.v[i]); }
}
static Fq fq_hex(const std::string& h) { return Fq::to_mont(from_hex<Fq>(h)); }
static G1A g1() { G1A g; g.x = Fq::one(); g.y = Fq::dbl(Fq::one()); return g; }
static G2A g2() {      // the generator of G2 every BN254 library uses (EIP-197)
  G2A g;
  g.x.c0 = fq_hex("1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed"); g.x.c1 = fq_hex("198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2");
  g.y.c0 = fq_hex("12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa"); g.y.c1 = fq_hex("090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b");
  return g;
}

static int ratio(const std::string& label, size_t n, std::istringstream& ls) {
  std::vector<G1A> before(n), after(n);
  std::vector<uint32_t> rho;
  std::string tok;
  for (std::vector<G1A>* arr : {&before, &after})
    for (size_t i = 0; i < n; i++) { if (!(ls >> tok)) { fprintf(stderr, "%s: too few scalars\n", label.c_str()); return 2; } (*arr)[i] = to_affine(pt_scalar_mul(g1(), from_hex<Fr>(tok).v)); }
  for (size_t i = 0; i < n; i++) {
    if (!(ls >> tok) || tok.size() > 32) { fprintf(stderr, "%s: a rho is missing or above 128 bits\n", label.c_str()); return 2; }
    const Fr r = from_hex<Fr>(tok); rho.insert(rho.end(), r.v, r.v + 4);
  }
  const size_t n_chunks = (n + RLC_CHUNK - 1) / RLC_CHUNK, blocks = (n_chunks + PT_BLOCK - 1) / PT_BLOCK;
  // sentinels no sum can be: a thread that writes another's slot, or leaves its own, shows
  G1A mark; memset((void*)&mark, 0xa5, sizeof(mark));
  std::vector<G1A> chunks(2 * n_chunks, mark), seen = chunks;
  for (unsigned row = 0; row < 2; row++)
    for (size_t t = 0; t < blocks * PT_BLOCK; t++) {
      if (t < n_chunks) pt_ratio_chunk(t, row, (const G1A*)before.data(), (const G1A*)after.data(), n, n_chunks, rho.data(), chunks.data());      // (the kernel's guard)
      for (size_t k = 0; k < chunks.size(); k++) {
        const bool own = t < n_chunks && k == row * n_chunks + t;
        const bool same = !memcmp((const void*)&chunks[k], (const void*)&seen[k], sizeof(G1A));
        if (own == same) { fprintf(stderr, "%s: thread (%zu, %u) %s slot %zu\n", label.c_str(), t, row, own ? "left its own" : "wrote", k); return 1; }
      }
      seen = chunks;
    }
  ColsumPlan plan;
  if (!ratio_sum_plan(n_chunks, &plan)) { fprintf(stderr, "%s: no plan\n", label.c_str()); return 1; }
  std::vector<G1A> out(2), partials[2];
  memset((void*)out.data(), 0, 2 * sizeof(G1A));
  for (size_t k = 0; k < plan.levels.size(); k++) {
    const ColsumLevel& lv = plan.levels[k];
    partials[k & 1].assign(lv.n_partials, G1A());
    const G1A* src = k ? partials[(k - 1) & 1].data() : chunks.data();
    for (size_t t = 0; t < lv.runs.size(); t++) colsum_run(t, lv.runs.data(), k ? nullptr : plan.entries.data(), plan.mags.data(), src, partials[k & 1].data(), out.data());
  }
  fputs(label.c_str(), stdout);
  for (const G1A& p : out) print_point(p);
  for (const G1A& p : chunks) print_point(p);
  putchar('\n');
  return 0;
}

static void parse(const std::string& label, const std::string& hex) {
  const std::vector<uint8_t> b = bytes_of(hex);
  uint8_t* exact = (uint8_t*)malloc(b.size() ? b.size() : 1);      // of exactly that size, 8-byte aligned as a caller's buffer is
  if (!b.empty()) memcpy(exact, b.data(), b.size());
  KeyLayout L;
  const char* why = key_layout(exact, b.size(), &L);
  if (why) printf("%s err %s\n", label.c_str(), why); else printf("%s ok %zu %zu %zu\n", label.c_str(), L.words, L.off_lh, L.n_lh);
  free(exact);
}

static int record(const std::string& label, std::istringstream& ls) {
  std::string head_hex, s, d, k;
  if (!(ls >> head_hex >> s >> d >> k)) { fprintf(stderr, "bad RECORD\n"); return 2; }
  const std::vector<uint8_t> hb = bytes_of(head_hex);
  if (hb.size() != 8 * KEY_HEAD_WORDS) { fprintf(stderr, "%s: the head is 88 bytes\n", label.c_str()); return 2; }
  uint64_t head[KEY_HEAD_WORDS]; memcpy(head, hb.data(), sizeof(head));
  const Fr sc = from_hex<Fr>(s);
  G1A d1 = to_affine(pt_scalar_mul(g1(), sc.v)); G2A d2 = to_affine(pt_scalar_mul(g2(), sc.v));
  const G1A before = d1;
  uint64_t before_words[8]; put_g1(before_words, before);
  std::vector<uint64_t> rec(RECORD_WORDS);      // (a heap block of the record's exact size)
  make_record(head, &d1, &d2, Fr::to_mont(from_hex<Fr>(d)), Fr::to_mont(from_hex<Fr>(k)), rec.data());
  fputs(label.c_str(), stdout); putchar(' ');
  for (size_t i = 0; i < 8 * RECORD_WORDS; i++) printf("%02x", ((const uint8_t*)rec.data())[i]);
  G1A after, T;
  if (!get_g1(rec.data() + REC_DELTA1, &after) || !get_g1(rec.data() + REC_T, &T) || !same_point(after, d1)) { fprintf(stderr, "%s: the record's points\n", label.c_str()); return 1; }
  const bool good = record_knowledge(head, before_words, before, after, T, rec.data());
  std::vector<uint64_t> off = rec; off[REC_Z] += 1;
  const bool bad_z = record_knowledge(head, before_words, before, after, T, off.data());
  uint64_t other_words[8]; put_g1(other_words, after);
  const bool bad_base = record_knowledge(head, other_words, after, after, T, rec.data());
  printf(" %d %d %d\n", (int)good, (int)bad_z, (int)bad_base);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: key_contrib_check CASES.txt\n"); return 2; }
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
    if (what == "RATIO") { size_t n = 0; if (!(ls >> n) || !n || n > 4096) { fprintf(stderr, "bad RATIO\n"); return 2; } rc = ratio(label, n, ls); }
    else if (what == "PARSE") { std::string hex; if (!(ls >> hex)) { fprintf(stderr, "bad PARSE\n"); return 2; } parse(label, hex); }
    else if (what == "RECORD") rc = record(label, ls);
    else { fprintf(stderr, "bad line: %s\n", what.c_str()); return 2; }
    if (rc) return rc;
  }
  return 0;
}
