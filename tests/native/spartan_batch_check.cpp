// Host check of the GPU-free pieces of the batched compressed-proof verifier (vimz_amd/csrc/spartan_batch_plan.hpp) against the definitions they stand for, on
// both scalar fields: the half-tables' per-thread body (what one thread of k_half_tables computes) against ipa_verify's s-vector loop and the eq table's doubling;
// k_svec_accum's index map against load_bases(shifted) and its mask against k_mask_public's rule; the unrolled coefficients against the round-by-round update
// P <- R + x·P + x²·L with field elements standing in for points; the chunk plan.  Every table lives in a heap block of exactly its size.  Built with
// -fsanitize=address,undefined and run by tests/test_spartan_batch_plan_host.py; prints one line a loop and "done".
#include <cstdio>
#include <random>
#include "spartan_batch_plan.hpp"
using namespace vz;

template <class F>
static F rnd(std::mt19937_64& rng, int mode) {
  if (mode == 0) return F::zero();
  if (mode == 1) return F::neg(F::one());
  F x; for (int i = 0; i < 8; i++) x.v[i] = (uint32_t)rng();
  x.v[7] &= 0x0fffffffu;
  return F::to_mont(x);
}

template <class F>
static int check_tables(const char* name) {
  std::mt19937_64 rng(11);
  int bad = 0, runs = 0;
  for (uint32_t nv : {1u, 2u, 7u, 9u, 10u, 11u, 13u}) {
    for (int kind = 0; kind < 2; kind++) {
      std::vector<F> pt(nv);
      for (uint32_t q = 0; q < nv; q++) pt[q] = rnd<F>(rng, q == nv / 2 ? kind : (q == 0 ? 1 : 2));      // a 0 (or r − 1) among the variables
      const size_t n = (size_t)1 << nv;
      // the definitions: ipa_verify's s-vector (round 0 = the top bit) and eq_table's doubling
      std::vector<F> want(n);
      want[0] = F::one();
      size_t len = 1;
      for (uint32_t q = nv; q-- > 0;) {
        for (size_t i = 0; i < len; i++) {
          if (kind == 0) want[i + len] = F::mul(want[i], pt[q]);
          else { const F hi = F::mul(want[i], pt[q]); want[i + len] = hi; want[i] = F::sub(want[i], hi); }
        }
        len <<= 1;
      }
      const sb::HalfLayout L = sb::half_layout(nv, nv);
      const uint32_t hl = L.hl[0];
      std::vector<F> lo((size_t)1 << hl), hi((size_t)1 << (nv - hl));
      auto var = [&](uint32_t q) { return pt.at(q); };
      for (uint32_t e = 0; e < lo.size(); e++) lo[e] = sb::half_entry<F>(var, nv, hl, false, (uint32_t)kind, e);
      for (uint32_t e = 0; e < hi.size(); e++) hi[e] = sb::half_entry<F>(var, nv, hl, true, (uint32_t)kind, e);
      if (L.off[1] != lo.size() || L.off[2] != lo.size() + hi.size() || L.elems != 2 * (lo.size() + hi.size())) bad++;
      for (size_t i = 0; i < n; i++)
        if (!F::mul(lo.at(i & (((size_t)1 << hl) - 1)), hi.at(i >> hl)).eq(want[i])) bad++;
      runs++;
    }
  }
  printf("%s/tables runs=%d bad=%d\n", name, runs, bad);
  return bad;
}

static int check_index_map() {
  int bad = 0, runs = 0;
  for (size_t n : {(size_t)2, (size_t)4, (size_t)8, (size_t)1024}) {
    // load_bases(shifted): G[0] = ck[n − 1], G[i] = ck[i − 1]
    std::vector<size_t> G(n);
    G[0] = n - 1;
    for (size_t i = 1; i < n; i++) G[i] = i - 1;
    std::vector<int> hit(n, 0);
    for (size_t j = 0; j < n; j++) {
      const size_t i = sb::svec_index(j, n, true);
      if (i >= n || G[i] != j) bad++; else hit[i]++;
      if (sb::svec_index(j, n, false) != j) bad++;
    }
    for (size_t i = 0; i < n; i++) if (hit[i] != 1) bad++;          // a permutation: every index serves exactly one slot
    for (uint32_t n_pub : {1u, 2u, 7u})
      for (uint32_t n_w : {(uint32_t)n, (uint32_t)(n / 2 + 1)}) {
        if (n_w < n_pub + 2) continue;
        for (size_t i = 0; i < n; i++) {
          const bool rule = i == 0 || i + n_pub >= n_w;            // k_mask_public
          if (sb::svec_masked(i, n_pub, n_w) != rule) bad++;
          if (sb::svec_masked(i, n_pub, 0)) bad++;
        }
        runs++;
      }
  }
  printf("index_map runs=%d bad=%d\n", runs, bad);
  return bad;
}

template <class F>
static int check_unroll(const char* name) {
  std::mt19937_64 rng(5);
  int bad = 0, runs = 0;
  for (size_t rounds : {(size_t)1, (size_t)2, (size_t)3, (size_t)19, (size_t)21}) {
    for (int it = 0; it < 8; it++) {
      std::vector<F> xs(rounds), Ls(rounds), Rs(rounds);
      for (size_t j = 0; j < rounds; j++) { xs[j] = rnd<F>(rng, it == 0 && j == rounds / 2 ? 0 : 2); Ls[j] = rnd<F>(rng, 2); Rs[j] = rnd<F>(rng, 2); }
      const F comm = rnd<F>(rng, 2), claim = rnd<F>(rng, it == 1 ? 0 : 2), r0 = rnd<F>(rng, 2), U = rnd<F>(rng, 2);
      F P = F::add(comm, F::mul(F::mul(claim, r0), U));
      for (size_t j = 0; j < rounds; j++) P = F::add(F::add(Rs[j], F::mul(xs[j], P)), F::mul(F::sqr(xs[j]), Ls[j]));
      std::vector<F> c; F g0;
      sb::ipa_unroll<F>(xs, claim, r0, c, &g0);
      if (c.size() != 2 * rounds + 1) { bad++; continue; }
      F got = F::add(F::mul(c.at(0), comm), F::mul(g0, U));
      for (size_t j = 0; j < rounds; j++) got = F::add(got, F::add(F::mul(c.at(1 + 2 * j), Rs[j]), F::mul(c.at(2 + 2 * j), Ls[j])));
      if (!got.eq(P)) bad++;
      runs++;
    }
  }
  printf("%s/unroll runs=%d bad=%d\n", name, runs, bad);
  return bad;
}

static int check_chunks() {
  int bad = 0, runs = 0;
  for (size_t n = 0; n <= 100; n++)
    for (size_t chunk = 0; chunk <= 40; chunk++) {
      const auto plan = sb::chunk_plan(n, chunk);
      const size_t want = chunk ? chunk : sb::DEFAULT_CHUNK;
      size_t at = 0;
      for (const auto& s : plan) {
        if (s.first != at || s.second <= s.first || s.second - s.first > want || s.second > n) bad++;
        if (s.second != n && s.second - s.first != want) bad++;          // only the last chunk may be short
        at = s.second;
      }
      if (at != n || plan.size() != (n + want - 1) / want) bad++;
      runs++;
    }
  printf("chunks runs=%d bad=%d\n", runs, bad);
  return bad;
}

int main() {
  int bad = check_tables<Fp<BnFr>>("fr") + check_tables<Fp<BnFq>>("fq") + check_index_map() + check_unroll<Fp<BnFr>>("fr") + check_unroll<Fp<BnFq>>("fq") + check_chunks();
  printf("done bad=%d\n", bad);
  return bad ? 1 : 0;
}
