// The point transform of vimz_amd/csrc/g16_powers.hip on the CPU: the very functions its kernels call with their thread index (g16_point_stage.hpp:
// pt_twiddle, pt_bitrev_swap, pt_butterfly, pt_scalar_mul) looped over every index of every launch, with the canonical Fp fields.  Reads the runs from the file
// named on the command line, one a line:
//     LABEL GROUP LOGN OPS s_0 .. s_(n-1)        GROUP 1 | 2;  OPS a string of f (forward), i (inverse, unscaled), I (inverse, times 1/n), n (nothing: the input);  s_k hex, below r
// takes [s_k]G as the input and prints "LABEL" and the outputs' coordinates (canonical, hex; G1: x y, G2: x.c0 x.c1 y.c0 y.c1; the identity as zeros) on one
// line.  Nothing is judged here: tests/test_point_transform_host.py compares.  No HIP: g++ -std=c++17 -fsanitize=address,undefined -I vimz_amd/csrc.
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
static void print_fq(const Fq& m) {
  const Fq c = Fq::from_mont(m);
  putchar(' ');
  for (int i = 7; i >= 0; i--) printf("%08x", c.v[i]);
}
static void print_point(const Affine<Fq>& p) { print_fq(p.x); print_fq(p.y); }
static void print_point(const Affine<Fq2>& p) { print_fq(p.x.c0); print_fq(p.x.c1); print_fq(p.y.c0); print_fq(p.y.c1); }

static Fq fq_hex(const char* h) { return Fq::to_mont(from_hex<Fq>(h)); }
template <class F> static Affine<F> generator();
template <> Affine<Fq> generator<Fq>() { Affine<Fq> g; g.x = Fq::one(); g.y = Fq::dbl(Fq::one()); return g; }
template <> Affine<Fq2> generator<Fq2>() {      // the generator of G2 every BN254 library uses (EIP-197)
  Affine<Fq2> g;
  g.x.c0 = fq_hex("1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed"); g.x.c1 = fq_hex("198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2");
  g.y.c0 = fq_hex("12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa"); g.y.c1 = fq_hex("090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b");
  return g;
}

// a primitive 2^k-th root of unity of Fr: 5^((r − 1) / 2^k)
static Fr root_of_unity(int k) {
  uint32_t e[8]; uint64_t br = 1;
  for (int i = 0; i < 8; i++) { const uint64_t d = (uint64_t)BnFr::MOD.w[i] - br; e[i] = (uint32_t)d; br = (d >> 32) & 1; }
  for (int s = 0; s < k; s++) for (int i = 0; i < 8; i++) e[i] = (e[i] >> 1) | (i < 7 ? e[i + 1] << 31 : 0u);
  Fr five = Fr::zero(); five.v[0] = 5; five = Fr::to_mont(five);
  Fr acc = Fr::one();
  for (int i = 255; i >= 0; i--) { acc = Fr::sqr(acc); if ((e[i >> 5] >> (i & 31)) & 1u) acc = Fr::mul(acc, five); }
  return acc;
}

// what g16_point_transform queues, launch by launch, every thread in turn
template <class F>
static void transform(std::vector<Affine<F>>& pts, int logn, bool inverse, bool scaled) {
  const size_t n = (size_t)1 << logn, n_half = n / 2;
  Fr w = root_of_unity(logn);
  if (inverse) w = Fr::pow_pm2(w);
  std::vector<uint32_t> tw(8 * n_half);
  for (size_t k = 0; k < n_half; k++) pt_twiddle(k, logn - 1, w, tw.data());
  for (size_t i = 0; i < n; i++) pt_bitrev_swap(i, logn, pts.data());
  for (size_t half = 1; half < n; half *= 2)
    for (size_t t = 0; t < n_half; t++) pt_butterfly(t, half, n_half, pts.data(), tw.data());
  if (scaled) {
    Fr nn = Fr::zero(); nn.v[0] = (uint32_t)n;
    const Fr ninv = Fr::from_mont(Fr::pow_pm2(Fr::to_mont(nn)));
    for (size_t i = 0; i < n; i++) pts[i] = to_affine(pt_scalar_mul(pts[i], ninv.v));
  }
}

template <class F>
static void run(const std::string& label, int logn, const std::string& ops, const std::vector<Fr>& s) {
  std::vector<Affine<F>> pts(s.size());
  const Affine<F> g = generator<F>();
  for (size_t k = 0; k < s.size(); k++) pts[k] = to_affine(pt_scalar_mul(g, s[k].v));
  for (char op : ops) if (op != 'n') transform(pts, logn, op != 'f', op == 'I');
  fputs(label.c_str(), stdout);
  for (const Affine<F>& p : pts) print_point(p);
  putchar('\n');
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: pt_stage_check RUNS.txt\n"); return 2; }
  std::ifstream in(argv[1]);
  if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string label, ops, tok;
    int group = 0, logn = 0;
    if (!(ls >> label >> group >> logn >> ops)) continue;
    std::vector<Fr> s;
    while (ls >> tok) s.push_back(from_hex<Fr>(tok));
    if ((group != 1 && group != 2) || logn < 1 || logn > 10 || s.size() != (size_t)1 << logn || ops.find_first_not_of("fiIn") != std::string::npos) {
      fprintf(stderr, "bad run: %s\n", label.c_str()); return 2;
    }
    if (group == 1) run<Fq>(label, logn, ops, s); else run<Fq2>(label, logn, ops, s);
  }
  return 0;
}
