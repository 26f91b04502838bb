// The multilinear KZG opening (vimz_amd/csrc/mlkzg_stage.hpp, mlkzg_verify.hpp) on the CPU: the very functions its kernels call with their thread index looped over
// every index from heap blocks of exact size, against a naive Horner, a naive division and the fold's definition; then a prover made of those loops with a tau this
// program knows, and the host verifier and parser over its proofs, again from heap blocks of exact size.  Prints
//     stage/NAME/N ok      after each comparison (any mismatch ends the program with status 1)
//     proof/L/N W0 W1 ..   the words of the proof for the fixed statement of that shape (tests/test_mlkzg_native_host.py compares them with tests/_mlkzg_ref.py's)
//     verdict/NAME V       what verify() says of the untouched and of the tampered proofs
// No HIP: g++ -std=c++17 -fsanitize=address,undefined -I vimz_amd/csrc.
#include <cstdio>
#include <cstdlib>
#include "mlkzg_verify.hpp"

using namespace vz;
using namespace vz::mlk;

static void fail(const char* what, size_t n) { fprintf(stderr, "mlkzg_check: %s (n = %zu)\n", what, n); exit(1); }
static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t next64() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return g_state; }
static Fr random_fr() { uint64_t w[4] = {next64(), next64(), next64(), next64() >> 3}; Fr c; memcpy(c.v, w, 32); return Fr::to_mont(c); }      // below 2^253 < r
static Fr fr_small(uint64_t v) { return dv::fr_u64(v); }
static Fr minus_one() { return Fr::neg(Fr::one()); }

static Fr naive_horner(const std::vector<Fr>& p, const Fr& u) { Fr a = Fr::zero(); for (size_t i = p.size(); i-- > 0;) a = Fr::add(Fr::mul(a, u), p[i]); return a; }
static int bitlen(size_t v) { int b = 0; while (v) { b++; v >>= 1; } return b; }
static Fr pow_u(Fr b, unsigned e) { Fr a = Fr::one(); for (; e; e >>= 1) { if (e & 1u) a = Fr::mul(a, b); b = Fr::sqr(b); } return a; }

// the evaluation at r, −r, r² as k_poly_eval3 + k_eval3_sum do it: chunk by chunk, block by block
static void eval3_loops(const std::vector<Fr>& p, const Fr& r, Fr out[3]) {
  const size_t len = p.size(), nb = n_blocks(len);
  const Fr w = Fr::sqr(r), wh = pow_u(w, ML_CHUNK / 2);
  const int bits = bitlen(n_chunks(len) - 1);
  std::vector<Fr> part(3 * nb);
  for (size_t b = 0; b < nb; b++) {
    Fr s[3] = {Fr::zero(), Fr::zero(), Fr::zero()};
    for (size_t t = b * ML_BLOCK; t < (b + 1) * ML_BLOCK; t++) {      // every thread of the block, those past the end too
      Fr v[3]; eval3_chunk(t, p.data(), len, w, wh, bits, v);
      for (int i = 0; i < 3; i++) s[i] = Fr::add(s[i], v[i]);
    }
    for (int i = 0; i < 3; i++) part[3 * b + i] = s[i];
  }
  eval3_finish(part.data(), nb, r, out);
}
// the division as the three launches do it; quot has len − 1 elements exactly
static Fr divide_loops(const std::vector<Fr>& b, const Fr& u, std::vector<Fr>& quot) {
  const size_t len = b.size(), nc = n_chunks(len), nb = n_blocks(len);
  const Fr uc = pow_u(u, ML_CHUNK), ubc = pow_u(uc, ML_BLOCK);
  std::vector<Fr> z(nc), cin(nc), zb(nb), ib(nb);
  quot.assign(len - 1, Fr::zero());
  Fr rem = Fr::zero();
  for (size_t t = 0; t < nc; t++) div_carry(t, b.data(), len, u, z.data());
  for (size_t k = 0; k < nb; k++) div_block_carry(k, z.data(), nc, uc, zb.data());
  div_block_scan(zb.data(), nb, ubc, ib.data());
  for (size_t k = 0; k < nb; k++) div_chunk_carries(k, z.data(), nc, uc, ib.data(), cin.data());
  for (size_t t = 0; t < nc; t++) div_chunk(t, b.data(), len, u, cin.data(), quot.data(), &rem);
  return rem;
}

static void stages_at(size_t n) {
  std::vector<Fr> p(n);
  for (auto& c : p) c = random_fr();
  if (n > 2) { p[1] = Fr::zero(); p[n - 1] = minus_one(); }
  const Fr us[4] = {Fr::zero(), Fr::one(), minus_one(), random_fr()};
  for (const Fr& u : us) {
    Fr got[3];
    eval3_loops(p, u, got);
    if (!got[0].eq(naive_horner(p, u)) || !got[1].eq(naive_horner(p, Fr::neg(u))) || !got[2].eq(naive_horner(p, Fr::sqr(u)))) fail("eval3 differs from Horner", n);
    std::vector<Fr> quot;
    const Fr rem = divide_loops(p, u, quot);
    if (!rem.eq(naive_horner(p, u))) fail("the remainder is not p(u)", n);
    Fr carry = Fr::zero();      // the plain recurrence, walking down
    for (size_t i = n; i-- > 0;) {
      carry = Fr::add(Fr::mul(carry, u), p[i]);
      if (i && !quot[i - 1].eq(carry)) fail("a quotient coefficient differs from the recurrence", n);
    }
  }
  printf("stage/eval3_divide/%zu ok\n", n);
}

// the levels side by side, by fold_one over every index
static std::vector<Fr> fold_loops(const std::vector<Fr>& v, const std::vector<Fr>& x) {
  const unsigned logn = (unsigned)x.size();
  const size_t N = (size_t)1 << logn;
  std::vector<Fr> levels(level_offset(N, logn + 1));
  for (size_t i = 0; i < N; i++) levels[i] = i < v.size() ? v[i] : Fr::zero();
  for (unsigned k = 0; k < logn; k++)
    for (size_t j = 0; j < (N >> (k + 1)); j++) fold_one(j, levels.data() + level_offset(N, k), x[k], levels.data() + level_offset(N, k + 1));
  return levels;
}
static void fold_batch_at(unsigned logn, int kind) {
  const size_t N = (size_t)1 << logn;
  std::vector<Fr> v(N), x(logn);
  for (auto& c : v) c = random_fr();
  for (unsigned k = 0; k < logn; k++) x[k] = kind == 0 ? Fr::zero() : kind == 1 ? Fr::one() : random_fr();
  const std::vector<Fr> levels = fold_loops(v, x);
  if (levels.size() != 2 * N - 1) fail("levels' length", N);
  if (logn <= 10) {      // y by its definition
    Fr y = Fr::zero();
    for (size_t i = 0; i < N; i++) {
      Fr e = v[i];
      for (unsigned k = 0; k < logn; k++) e = Fr::mul(e, (i >> k) & 1u ? x[k] : Fr::sub(Fr::one(), x[k]));
      y = Fr::add(y, e);
    }
    if (!levels[2 * N - 2].eq(y)) fail("the last level is not the multilinear evaluation", N);
  }
  if (kind == 0 && !levels[2 * N - 2].eq(v[0])) fail("x = 0 does not pick v[0]", N);
  if (kind == 1 && !levels[2 * N - 2].eq(v[N - 1])) fail("x = 1 does not pick v[N − 1]", N);
  const Fr q = random_fr();
  std::vector<Fr> B(N);
  for (size_t j = 0; j < N; j++) batch_one(j, levels.data(), N, logn, q, B.data());
  for (size_t j = 0; j < N; j++) {
    Fr want = Fr::zero(), qk = Fr::one();
    for (unsigned k = 0; k < logn; k++, qk = Fr::mul(qk, q)) if (j < (N >> k)) want = Fr::add(want, Fr::mul(qk, levels[level_offset(N, k) + j]));
    if (!B[j].eq(want)) fail("a batched coefficient", N);
  }
  printf("stage/fold_batch/%u/%d ok\n", logn, kind);
}

// ---- a prover out of the loops above, with a known tau ------------------------------------------------------------------------------------------------------------
static G1A commit(const std::vector<Fr>& p, const Fr& tau) { const Fr s = Fr::from_mont(naive_horner(p, tau)); return to_affine(pt_scalar_mul(g1_generator(), s.v)); }
static void put_g1(uint64_t* dst, const G1A& p) { const Fq x = Fq::from_mont(p.x), y = Fq::from_mont(p.y); memcpy(dst, x.v, 32); memcpy(dst + 4, y.v, 32); }

struct Statement { std::vector<uint64_t> vk, comm, point, eval, proof; uint32_t logn; };
static Statement prove(uint32_t logn, size_t n, uint64_t seed) {
  const size_t N = (size_t)1 << logn;
  const Fr tau = fr_small(0x5555aaaa7ull + seed);
  std::vector<Fr> v(n), x(logn);
  for (size_t i = 0; i < n; i++) v[i] = fr_small(1000 * seed + 3 * i + 1);
  for (uint32_t k = 0; k < logn; k++) x[k] = fr_small(7 * seed + 11 * k + 2);
  const std::vector<Fr> levels = fold_loops(v, x);
  auto level = [&](uint32_t k) { return std::vector<Fr>(levels.begin() + level_offset(N, k), levels.begin() + level_offset(N, k + 1)); };
  Statement S; S.logn = logn;
  S.vk.assign(16, 0); S.comm.assign(8, 0); S.point.assign(4 * logn, 0); S.eval.assign(4, 0); S.proof.assign(proof_words(logn), 0);      // heap blocks of exact size
  { const Fr t = Fr::from_mont(tau); const G2A k = to_affine(pt_scalar_mul(g2_generator(), t.v));
    const Fq c[4] = {k.x.c0, k.x.c1, k.y.c0, k.y.c1};
    for (int i = 0; i < 4; i++) { const Fq w = Fq::from_mont(c[i]); memcpy(&S.vk[4 * i], w.v, 32); } }
  put_g1(S.comm.data(), commit(level(0), tau));
  for (uint32_t k = 0; k < logn; k++) put_fr(&S.point[4 * k], x[k]);
  put_fr(S.eval.data(), levels[2 * N - 2]);
  for (uint32_t k = 1; k < logn; k++) put_g1(&S.proof[at_ck(logn) + 8 * (k - 1)], commit(level(k), tau));
  Rounds R;
  const Fr r = R.round_r(logn, S.comm.data(), S.point.data(), S.eval.data(), S.proof.data() + at_ck(logn));
  if (r.is_zero()) fail("r = 0", n);
  std::vector<Fr> E(3 * logn);
  for (uint32_t k = 0; k < logn; k++) { Fr o[3]; eval3_loops(level(k), r, o); for (int u = 0; u < 3; u++) E[u * logn + k] = o[u]; }
  for (size_t i = 0; i < E.size(); i++) put_fr(&S.proof[at_evals(logn) + 4 * i], E[i]);
  const Fr q = R.round_q(logn, S.proof.data() + at_evals(logn));
  std::vector<Fr> B(N);
  for (size_t j = 0; j < N; j++) batch_one(j, levels.data(), N, logn, q, B.data());
  const Fr us[3] = {r, Fr::neg(r), Fr::sqr(r)};
  for (int j = 0; j < 3; j++) {
    std::vector<Fr> quot;
    const Fr rem = divide_loops(B, us[j], quot);
    Fr b = Fr::zero();
    for (uint32_t k = logn; k-- > 0;) b = Fr::add(Fr::mul(b, q), E[j * logn + k]);
    if (!b.eq(rem)) fail("the remainder rule", n);
    put_g1(&S.proof[at_w(logn) + 8 * j], commit(quot, tau));
  }
  return S;
}
static uint32_t verdict(const Statement& S) { return verify(S.vk.data(), S.comm.data(), S.logn, S.point.data(), S.eval.data(), S.proof.data(), S.proof.size()); }

int main() {
  if (!pairing::consts().ok) fail("pairing constants", 0);
  const size_t bc = (size_t)ML_BLOCK * ML_CHUNK;
  for (size_t n : {(size_t)1, (size_t)2, (size_t)ML_CHUNK - 1, (size_t)ML_CHUNK, (size_t)ML_CHUNK + 1, bc - 1, bc, bc + 1, 2 * bc + 3}) stages_at(n);
  unsigned big = 1;
  while (((size_t)1 << big) <= bc) big++;
  for (unsigned logn : {1u, 2u, 3u, big}) for (int kind = 0; kind < 3; kind++) fold_batch_at(logn, kind);
  printf("shape %u %u\n", ML_BLOCK, ML_CHUNK);
  for (uint32_t logn : {1u, 2u, 3u, 5u})
    for (size_t n : {(size_t)1, ((size_t)1 << logn) - 1, (size_t)1 << logn}) {
      const Statement S = prove(logn, n, logn);
      printf("proof/%u/%zu", logn, n);
      for (uint64_t w : S.proof) printf(" %016llx", (unsigned long long)w);
      putchar('\n');
      printf("verdict/%u/%zu %u\n", logn, n, verdict(S));
    }
  { Statement S = prove(3, 7, 3), T;
    T = S; T.proof.pop_back(); printf("verdict/short %u\n", verdict(T));
    T = S; T.proof[at_evals(3)] += 1; printf("verdict/fold %u\n", verdict(T));
    T = S; T.proof[at_evals(3) + 8 * 3] += 1; printf("verdict/pairing %u\n", verdict(T));
    T = S; T.proof[at_w(3)] += 1; printf("verdict/off_curve %u\n", verdict(T));
    T = S; memcpy(&T.eval[0], BnFr::MOD.w, 32); printf("verdict/element_r %u\n", verdict(T));
    T = S; memcpy(&T.comm[4], BnFq::MOD.w, 32); printf("verdict/coordinate_q %u\n", verdict(T));
    T = S; T.logn = 0; Parsed P; printf("parse/logn_0 %d\n", (int)parse(T.vk.data(), T.comm.data(), 0, T.point.data(), T.eval.data(), T.proof.data(), T.proof.size(), &P)); }
  puts("done");
  return 0;
}
