// Judging a powers-of-tau string (vimz_amd/csrc/g16_powers_verify.hip) on the CPU: the very functions its kernels call with their thread index
// (g16_point_stage.hpp: pt_flags, pt_rlc_chunk, and colsum_run over rlc_sum_plan's plan) looped over every index of every launch, with the canonical Fp fields.
// Reads lines from the file named on the command line:
//     BASE GROUP N a d [i:s ..]         the points the RLC lines after it use: P_k = [a + k·d]G for k < N, then P_i = [s]G for every override (hex below r)
//     RLC LABEL GROUP PAIRS rho_0 ..    S = Σ rho_k·P_k, S' = Σ rho_k·P_(k+1) over k < PAIRS (rho: hex below 2^128) as g16_powers_rlc queues them: one pt_rlc_chunk per
//                                       chunk, then the plan's levels run by run, for shift 0 and 1.  Prints LABEL, S, S', then the chunk sums of shift 0.
//     FLAGS LABEL GROUP tok ..          tok = s:HEX (the point [HEX]G) or p:c,c[,c,c] (canonical coordinates, hex, below q).  Prints LABEL and pt_flags of every point.
// Points print as canonical hex coordinates (G1: x y, G2: x.c0 x.c1 y.c0 y.c1; the identity as zeros).  Nothing is judged here: tests/test_powers_verify_host.py
// compares.  No HIP: g++ -std=c++17 -fsanitize=address,undefined -I vimz_amd/csrc.
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
static void print_canon(const Fq& m) { const Fq c = Fq::from_mont(m); putchar(' '); for (int i = 7; i >= 0; i--) printf("%08x", c.v[i]); }

static Fq fq_hex(const std::string& h) { return Fq::to_mont(from_hex<Fq>(h)); }
template <class F> static Affine<F> generator();
template <> Affine<Fq> generator<Fq>() { Affine<Fq> g; g.x = Fq::one(); g.y = Fq::dbl(Fq::one()); return g; }
template <> Affine<Fq2> generator<Fq2>() {      // the generator of G2 every BN254 library uses (EIP-197)
  Affine<Fq2> g;
  g.x.c0 = fq_hex("1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed"); g.x.c1 = fq_hex("198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2");
  g.y.c0 = fq_hex("12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa"); g.y.c1 = fq_hex("090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b");
  return g;
}
static Fq curve_b(const Affine<Fq>*) { return vz::pairing::fq_u64(3); }
static Fq2 curve_b(const Affine<Fq2>*) { return vz::pairing::consts().twist_b; }
static void coords(Affine<Fq>& p, const std::vector<std::string>& c) { if (c.size() != 2) { fprintf(stderr, "G1 points have two coordinates\n"); exit(2); } p.x = fq_hex(c[0]); p.y = fq_hex(c[1]); }
static void coords(Affine<Fq2>& p, const std::vector<std::string>& c) {
  if (c.size() != 4) { fprintf(stderr, "G2 points have four coordinates\n"); exit(2); }
  p.x.c0 = fq_hex(c[0]); p.x.c1 = fq_hex(c[1]); p.y.c0 = fq_hex(c[2]); p.y.c1 = fq_hex(c[3]);
}

template <class F>
struct Group {
  std::vector<Affine<F>> base;

  void make_base(size_t n, const Fr& a, const Fr& d, std::istringstream& ls) {
    const Affine<F> g = generator<F>();
    const Affine<F> step = to_affine(pt_scalar_mul(g, d.v));
    base.assign(n, Affine<F>());
    XYZZ<F> acc = pt_scalar_mul(g, a.v);
    for (size_t k = 0; k < n; k++) { base[k] = to_affine(acc); add_mixed(acc, step); }
    std::string tok;
    while (ls >> tok) {
      const size_t colon = tok.find(':');
      const size_t i = std::stoul(tok.substr(0, colon));
      if (colon == std::string::npos || i >= n) { fprintf(stderr, "bad override %s\n", tok.c_str()); exit(2); }
      base[i] = to_affine(pt_scalar_mul(g, from_hex<Fr>(tok.substr(colon + 1)).v));
    }
  }

  // what g16_powers_rlc queues, launch by launch, every thread in turn
  void rlc(const std::string& label, size_t n_pairs, const std::vector<uint32_t>& rho) {
    if (n_pairs + 1 > base.size()) { fprintf(stderr, "%s: more pairs than the base has\n", label.c_str()); exit(2); }
    const size_t n_chunks = (n_pairs + RLC_CHUNK - 1) / RLC_CHUNK;
    ColsumPlan plan;
    if (!rlc_sum_plan(n_chunks, &plan)) { fprintf(stderr, "%s: no plan\n", label.c_str()); exit(1); }
    const std::vector<Affine<F>> points(base.begin(), base.begin() + n_pairs + 1);      // (a copy of its exact length: the sanitizer sees a read past the last pair)
    std::vector<Affine<F>> chunks0, out(2);
    for (unsigned shift = 0; shift < 2; shift++) {
      std::vector<Affine<F>> chunks(n_chunks);
      for (size_t t = 0; t < n_chunks; t++) pt_rlc_chunk(t, points.data(), n_pairs, rho.data(), shift, chunks.data());
      if (!shift) chunks0 = chunks;
      std::vector<Affine<F>> partials[2];
      for (size_t k = 0; k < plan.levels.size(); k++) {
        const ColsumLevel& lv = plan.levels[k];
        partials[k & 1].assign(lv.n_partials, Affine<F>());
        const Affine<F>* src = k ? partials[(k - 1) & 1].data() : chunks.data();
        for (size_t t = 0; t < lv.runs.size(); t++) colsum_run(t, lv.runs.data(), k ? nullptr : plan.entries.data(), plan.mags.data(), src, partials[k & 1].data(), out.data() + shift);
      }
    }
    fputs(label.c_str(), stdout);
    for (const Affine<F>& p : out) { const Fq* c = (const Fq*)&p; for (size_t i = 0; i < sizeof(Affine<F>) / sizeof(Fq); i++) print_canon(c[i]); }
    for (const Affine<F>& p : chunks0) { const Fq* c = (const Fq*)&p; for (size_t i = 0; i < sizeof(Affine<F>) / sizeof(Fq); i++) print_canon(c[i]); }
    putchar('\n');
  }

  void flags(const std::string& label, std::istringstream& ls) {
    const Affine<F> g = generator<F>();
    std::vector<Affine<F>> pts;
    std::string tok;
    while (ls >> tok) {
      Affine<F> p;
      if (tok.rfind("s:", 0) == 0) p = to_affine(pt_scalar_mul(g, from_hex<Fr>(tok.substr(2)).v));
      else if (tok.rfind("p:", 0) == 0) {
        std::vector<std::string> c; std::istringstream cs(tok.substr(2)); std::string one;
        while (std::getline(cs, one, ',')) c.push_back(one);
        coords(p, c);
      } else { fprintf(stderr, "bad point %s\n", tok.c_str()); exit(2); }
      pts.push_back(p);
    }
    std::vector<uint32_t> f(pts.size(), 0xdeadu);
    const F b = curve_b(pts.data());
    for (size_t i = 0; i < pts.size(); i++) pt_flags(i, pts.data(), b, sizeof(F) == sizeof(Fq) ? (const uint32_t*)nullptr : BnFr::MOD.w, f.data());
    fputs(label.c_str(), stdout);
    for (uint32_t x : f) printf(" %u", x);
    putchar('\n');
  }
};

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: pt_verify_check CASES.txt\n"); return 2; }
  std::ifstream in(argv[1]);
  if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  if (!vz::pairing::consts().ok) { fprintf(stderr, "pairing constants\n"); return 1; }
  Group<Fq> g1; Group<Fq2> g2;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string what, label, tok;
    int group = 0;
    if (!(ls >> what)) continue;
    if (what == "BASE") {
      size_t n = 0; std::string a, d;
      if (!(ls >> group >> n >> a >> d) || (group != 1 && group != 2) || !n || n > 4096) { fprintf(stderr, "bad BASE\n"); return 2; }
      if (group == 1) g1.make_base(n, from_hex<Fr>(a), from_hex<Fr>(d), ls); else g2.make_base(n, from_hex<Fr>(a), from_hex<Fr>(d), ls);
    } else if (what == "RLC") {
      size_t n_pairs = 0;
      if (!(ls >> label >> group >> n_pairs) || (group != 1 && group != 2) || !n_pairs) { fprintf(stderr, "bad RLC\n"); return 2; }
      std::vector<uint32_t> rho;
      while (ls >> tok) { if (tok.size() > 32) { fprintf(stderr, "%s: a rho above 128 bits\n", label.c_str()); return 2; } const Fr r = from_hex<Fr>(tok); rho.insert(rho.end(), r.v, r.v + 4); }
      if (rho.size() != 4 * n_pairs) { fprintf(stderr, "%s: %zu rho for %zu pairs\n", label.c_str(), rho.size() / 4, n_pairs); return 2; }
      if (group == 1) g1.rlc(label, n_pairs, rho); else g2.rlc(label, n_pairs, rho);
    } else if (what == "FLAGS") {
      if (!(ls >> label >> group) || (group != 1 && group != 2)) { fprintf(stderr, "bad FLAGS\n"); return 2; }
      if (group == 1) g1.flags(label, ls); else g2.flags(label, ls);
    } else { fprintf(stderr, "bad line: %s\n", what.c_str()); return 2; }
  }
  return 0;
}
