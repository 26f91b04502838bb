// The batched decider verifier (vimz_amd/csrc/decider_batch.hpp, pairing_stage.hpp, decider_verify.hpp) on the CPU: the very functions its kernels call with their
// thread index (g1_lincomb_thread, miller_thread) looped over every index at n = 1, 2, 65 from heap blocks of exact size — checking after every thread that it wrote
// its own slot and no other —, and the host path of vimz_decider_verify_batch (HostStages) on a small synthetic key whose trapdoor this program knows, so that it can
// make proofs the single verifier accepts.  Prints
//     miller/N/i  the 96 canonical words of thread i's Miller value for P_i = [3 + 5i]G1, Q_i = [7 + 11i]G2 (i ≡ 1 mod 7: P the identity, i ≡ 2 mod 7: Q the identity)
//     lincomb/N/i x y of a_i + k_i·b_i for the cases of lincomb_case() below
//     batch/NAME  the results of verify_batch beside verify_words' for each proof
// tests/test_decider_batch_host.py compares.  No HIP: g++ -std=c++17 -fsanitize=address,undefined -I vimz_amd/csrc.
#include <cstdio>
#include <cstdlib>
#include "decider_batch.hpp"

using namespace vz;
using namespace vz::dvb;
using pairing::Fq12;

static G1A gen1() { G1A g; g.x = Fq::one(); g.y = Fq::dbl(Fq::one()); return g; }
static Fq fq_hex(const char* h) {
  Fq c = Fq::zero(); int bit = 0;
  for (size_t i = strlen(h); i-- > 0; bit += 4) { const char ch = h[i]; const uint32_t d = ch <= '9' ? ch - '0' : ch - 'a' + 10; c.v[bit >> 5] |= d << (bit & 31); }
  return Fq::to_mont(c);
}
static G2A gen2() {      // the generator of G2 every BN254 library uses (EIP-197)
  G2A g;
  g.x.c0 = fq_hex("1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed"); g.x.c1 = fq_hex("198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2");
  g.y.c0 = fq_hex("12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa"); g.y.c1 = fq_hex("090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b");
  return g;
}
template <class F> static Affine<F> mul(const Affine<F>& p, const Fr& k_mont) { const Fr c = Fr::from_mont(k_mont); return to_affine(pt_scalar_mul(p, c.v)); }
static void print_fq(const Fq& m) { const Fq c = Fq::from_mont(m); putchar(' '); for (int i = 7; i >= 0; i--) printf("%08x", c.v[i]); }
static void fail(const char* what) { fprintf(stderr, "decider_batch_check: %s\n", what); exit(1); }

static void miller_at(size_t n) {
  std::vector<G1A> P(n); std::vector<G2A> Q(n);
  for (size_t i = 0; i < n; i++) {
    P[i] = mul(gen1(), fr_u64(3 + 5 * i)); Q[i] = mul(gen2(), fr_u64(7 + 11 * i));
    if (i % 7 == 1) memset((void*)&P[i], 0, sizeof(G1A));
    if (i % 7 == 2) memset((void*)&Q[i], 0, sizeof(G2A));
  }
  const pairing::Consts& C = pairing::consts();
  std::vector<Fq12> out(n);
  memset((void*)out.data(), 0x5a, sizeof(Fq12) * n);
  for (size_t t = 0; t < n; t++) {
    const std::vector<Fq12> before = out;
    pairing::miller_thread(t, P.data(), Q.data(), C.twist_b, C.g12, C.g13, out.data());
    for (size_t i = 0; i < n; i++) if (i != t && memcmp((const void*)&before[i], (const void*)&out[i], sizeof(Fq12))) fail("a Miller thread wrote another thread's slot");
  }
  for (size_t i = 0; i < n; i++) {
    if (n == 65 && i > 3 && i < 62) continue;      // (the edges and the special cases are printed; every thread ran)
    printf("miller/%zu/%zu", n, i);
    const Fq* c = (const Fq*)&out[i];
    for (int k = 0; k < 12; k++) print_fq(c[k]);
    putchar('\n');
  }
  // P and −P against one Q: the product is one after the final exponentiation
  if (n >= 1) {
    const G1A p = mul(gen1(), fr_u64(12345)); const G2A q = mul(gen2(), fr_u64(777));
    const Fq12 f = Fq12::mul(miller_one(p, q), miller_one(g1_negate(p), q));
    if (!pairing::fq12_pow(f, C.final_exp).is_one()) fail("e(P, Q)·e(−P, Q) is not one");
    if (n == 1 && pairing::fq12_pow(miller_one(p, q), C.final_exp).is_one()) fail("e(P, Q) is one");
  }
}

// case i: 0 a the identity, 1 b the identity, 2 k = 0, 3 k = r − 1 with a = b (the sum is the identity), 4.. a walk of 1, 128, 254 bits in turn
static void lincomb_at(size_t n) {
  std::vector<G1A> a(n), b(n), out(n);
  std::vector<uint32_t> k(8 * n, 0), bits(n);
  for (size_t i = 0; i < n; i++) {
    a[i] = mul(gen1(), fr_u64(1000 + i)); b[i] = mul(gen1(), fr_u64(2000 + 3 * i));
    const uint64_t kw[4] = {0x9e3779b97f4a7c15ull * (i + 1), 0xc2b2ae3d27d4eb4full ^ i, 0x165667b19e3779f9ull + i, 0x2fffffffffffffffull};      // 254 bits, below r
    Fr s = reduce256(kw);
    static const uint32_t widths[3] = {1, 128, 254};
    bits[i] = widths[i % 3];
    switch (i % 5 == i ? i : 4) {
      case 0: memset((void*)&a[i], 0, sizeof(G1A)); break;
      case 1: memset((void*)&b[i], 0, sizeof(G1A)); break;
      case 2: s = Fr::zero(); break;
      case 3: { a[i] = b[i]; uint64_t br = 1; for (int q = 0; q < 8; q++) { const uint64_t d = (uint64_t)BnFr::MOD.w[q] - br; s.v[q] = (uint32_t)d; br = (d >> 32) & 1; } bits[i] = 254; } break;
      default: break;
    }
    memcpy(&k[8 * i], s.v, 32);
  }
  memset((void*)out.data(), 0x5a, sizeof(G1A) * n);
  for (size_t t = 0; t < n; t++) {
    const std::vector<G1A> before = out;
    pairing::g1_lincomb_thread(t, a.data(), k.data(), bits.data(), b.data(), out.data());
    for (size_t i = 0; i < n; i++) if (i != t && memcmp((const void*)&before[i], (const void*)&out[i], sizeof(G1A))) fail("a lincomb thread wrote another thread's slot");
  }
  for (size_t i = 0; i < n; i++) {
    if (n == 65 && i > 6 && i < 62) continue;
    printf("lincomb/%zu/%zu %u", n, i, bits[i]);
    for (int q = 7; q >= 0; q--) printf(q == 7 ? " %08x" : "%08x", k[8 * i + q]);
    print_fq(out[i].x); print_fq(out[i].y); putchar('\n');
  }
}

// ---- a synthetic key with a known trapdoor, and proofs made with it ------------------------------------------------------------------------------------------------
struct Trapdoor { Fr alpha, beta, gamma, delta, tau; std::vector<Fr> ic; };
static void put_fq(uint64_t* dst, const Fq& m) { const Fq c = Fq::from_mont(m); memcpy(dst, c.v, 32); }
static void put_fr(uint64_t* dst, const Fr& m) { const Fr c = Fr::from_mont(m); memcpy(dst, c.v, 32); }
static void put_g1(uint64_t* dst, const G1A& p) { put_fq(dst, p.x); put_fq(dst + 4, p.y); }

static void make_key(uint32_t len_z, Trapdoor* T, VerifierKey* K) {
  T->alpha = fr_u64(0x1234567); T->beta = fr_u64(0x7654321); T->gamma = fr_u64(0xabcdef1); T->delta = fr_u64(0x1fedcba); T->tau = fr_u64(0x5555aaaa7);
  K->pp_hash = fr_u64(0xdecade); K->len_z = len_z;
  K->alpha = mul(gen1(), T->alpha); K->beta = mul(gen2(), T->beta); K->gamma = mul(gen2(), T->gamma); K->delta = mul(gen2(), T->delta);
  T->ic.resize(n_public(len_z) + 1); K->ic.resize(T->ic.size());
  for (size_t k = 0; k < T->ic.size(); k++) { T->ic[k] = fr_u64(0x10001 + 977 * k); K->ic[k] = mul(gen1(), T->ic[k]); }
  K->kzg_g1 = gen1(); K->kzg_g2 = gen2(); K->kzg_vk = mul(gen2(), T->tau);
}
// 25 words the single verifier accepts for (steps, z0, zi) under the key of T; `salt` varies the proof
static void make_proof(const Trapdoor& T, const VerifierKey& K, uint64_t steps, const uint64_t* z0, const uint64_t* zi, uint64_t salt, uint64_t* w) {
  memset(w, 0, 800);
  const Fr uw = fr_u64(11 + salt), ue = fr_u64(13 + salt), lw = fr_u64(17 + salt), t = fr_u64(19 + salt), a = fr_u64(23 + salt), b = fr_u64(29 + salt), piw = fr_u64(31 + salt), pie = fr_u64(37 + salt);
  const uint64_t two128[4] = {0, 0, 1, 0};
  const Fr r = Fr::add(fr_u64(salt + 5), Fr::to_mont(fr_of_words(two128, 4))), xw = fr_u64(41 + salt), xe = fr_u64(43 + salt);
  put_g1(w, mul(gen1(), uw)); put_g1(w + 8, mul(gen1(), ue)); put_g1(w + 16, mul(gen1(), lw)); put_g1(w + 24, mul(gen1(), t));
  put_fr(w + 32, r);
  put_g1(w + 36, mul(gen1(), a));
  { const G2A B = mul(gen2(), b); put_fq(w + 44, B.x.c1); put_fq(w + 48, B.x.c0); put_fq(w + 52, B.y.c1); put_fq(w + 56, B.y.c0); }
  put_g1(w + 60, gen1());      // C: a placeholder on the curve until the public inputs are known
  put_fr(w + 68, xw); put_fr(w + 72, xe);
  // y = c + x·p − p·tau opens the commitment [c]G at x with the proof [p]G
  const Fr cw = Fr::add(uw, Fr::mul(r, lw)), ce = Fr::add(ue, Fr::mul(r, t));
  put_fr(w + 76, Fr::sub(Fr::add(cw, Fr::mul(xw, piw)), Fr::mul(piw, T.tau))); put_fr(w + 80, Fr::sub(Fr::add(ce, Fr::mul(xe, pie)), Fr::mul(pie, T.tau)));
  put_g1(w + 84, mul(gen1(), piw)); put_g1(w + 92, mul(gen1(), pie));
  Proof p;
  if (!parse_proof(K, steps, z0, zi, w, true, &p)) fail("the synthetic proof does not parse");
  finish_public(p, w, mul(gen1(), cw), mul(gen1(), ce));
  Fr x = T.ic[0];
  for (size_t k = 0; k < p.pub.size(); k++) x = Fr::add(x, Fr::mul(p.pub[k], T.ic[k + 1]));
  // a·b = alpha·beta + x·gamma + c·delta
  const Fr c = Fr::mul(Fr::sub(Fr::sub(Fr::mul(a, b), Fr::mul(T.alpha, T.beta)), Fr::mul(x, T.gamma)), Fr::pow_pm2(T.delta));
  put_g1(w + 60, mul(gen1(), c));
}

static void batch_case(const char* name, const VerifierKey& K, size_t n, const std::vector<uint64_t>& steps, const std::vector<uint64_t>& z0, const std::vector<uint64_t>& zi,
                       const std::vector<uint64_t>& words, size_t chunk, const uint64_t* given) {
  // heap blocks of exact size
  std::vector<uint32_t> res(n, 0xdeadu);
  double sec[6];
  HostStages st(4);
  const int rc = verify_batch(K, n, steps.data(), z0.data(), zi.data(), words.data(), chunk, given, st, 4, res.data(), sec);
  printf("batch/%s %d", name, rc);
  for (size_t i = 0; i < n; i++) printf(" %u:%u", res[i], verify_words(K, steps[i], z0.data() + 4 * K.len_z * i, zi.data() + 4 * K.len_z * i, words.data() + 100 * i));
  putchar('\n');
}

int main() {
  if (!pairing::consts().ok) fail("pairing constants");
  for (size_t n : {(size_t)1, (size_t)2, (size_t)65}) { miller_at(n); lincomb_at(n); }
  Trapdoor T; VerifierKey K;
  make_key(1, &T, &K);
  const size_t n = 5;
  std::vector<uint64_t> steps(n), z0(4 * n, 0), zi(4 * n, 0), words(100 * n);
  for (size_t i = 0; i < n; i++) { steps[i] = 2 + i; z0[4 * i] = 100 + i; zi[4 * i] = 200 + i; make_proof(T, K, steps[i], &z0[4 * i], &zi[4 * i], 1000 * i, &words[100 * i]); }
  batch_case("good", K, n, steps, z0, zi, words, 2, nullptr);
  batch_case("one_chunk", K, n, steps, z0, zi, words, 256, nullptr);
  { std::vector<uint64_t> w = words, s = steps, zz = zi;
    w[100 * 1 + 76] ^= 1;                                    // proof 1: eval_W
    { Fq y; memcpy(y.v, &w[100 * 2 + 64], 32); y = Fq::neg(Fq::to_mont(y)); put_fq(&w[100 * 2 + 64], y); }      // proof 2: −C
    w[100 * 3 + 0] ^= 1;                                     // proof 3: U.cmW off the curve
    s[4] = 1;                                                // proof 4: steps = 1
    batch_case("mixed", K, n, s, z0, zi, w, 2, nullptr);
    memset(&zz[4 * 0], 0xff, 32);                            // proof 0: z_i not below r
    batch_case("noncanonical", K, n, s, z0, zz, w, 3, nullptr); }
  { // two proofs with their C points swapped: the sums cannot see it when every multiplier is one; the OS's multipliers do
    std::vector<uint64_t> w(words.begin(), words.begin() + 200), ones(12, 0);
    for (int q = 0; q < 8; q++) std::swap(w[60 + q], w[160 + q]);
    for (int q = 0; q < 6; q++) ones[2 * q] = 1;
    const std::vector<uint64_t> s2(steps.begin(), steps.begin() + 2), a0(z0.begin(), z0.begin() + 8), ai(zi.begin(), zi.begin() + 8);
    batch_case("swapped_ones", K, 2, s2, a0, ai, w, 2, ones.data());
    batch_case("swapped", K, 2, s2, a0, ai, w, 2, nullptr);
    std::vector<uint64_t> zero = ones; zero[2] = 0;
    batch_case("zero_multiplier", K, 2, s2, a0, ai, w, 2, zero.data()); }
  batch_case("none", K, 0, {}, {}, {}, {}, 2, nullptr);
  return 0;
}
