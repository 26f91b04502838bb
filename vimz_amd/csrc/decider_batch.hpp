// vimz_decider_verify_batch without its device: many decider proofs under ONE key, judged by one product of Miller values and one final exponentiation a chunk.
// No HIP in this file — decider_batch.hip supplies the device stages, HostStages below loops the same per-thread functions (pairing_stage.hpp, g16_point_stage.hpp)
// on the process's threads, and tests/native/decider_batch_check.cpp runs this path under the host sanitizers.
//
// Under multipliers rho_i, sigma_i, sigma'_i of 128 bits from the OS, with cmW_i = U_i.cmW + r_i·u_i.cmW and cmE_i = U_i.cmE + r_i·cmT_i, a chunk S is accepted iff
//     Π_{i∈S} ML(−rho_i·A_i, B_i) · ML((Σrho_i)·alpha, beta) · ML((Σrho_i)·IC_0 + Σ_k (Σ_i rho_i·pub_{i,k})·IC_{k+1}, gamma) · ML(Σrho_i·C_i, delta)
//       · ML(Σ(sigma_i·piW_i + sigma'_i·piE_i), VK) · ML(Σ(−sigma_i·xW_i·piW_i − sigma_i·cmW_i − sigma'_i·xE_i·piE_i − sigma'_i·cmE_i) + (Σ(sigma_i·yW_i + sigma'_i·yE_i))·G_1, G_2)
// is one after ONE final exponentiation: the 3·|S| equations of the single verifier (decider_verify.hpp: verify_words) in a random combination, wrong with probability
// about 2^-128 when one of them fails.  What every proof brings of its own is B_i, so one Miller loop a proof remains; B_i enters only after it has passed "on the
// twist" and r·B_i = O BY ITSELF — a sum cannot see a component in the twist's small cofactor subgroups (g16_powers_verify.hip says the same of a string's points).
// An accepted chunk gives its members their DV_STEPS bit.  A refused chunk is BISECTED (batch_bisect.hpp): the same equation is asked of halves, every member
// under the multipliers it had, from the rows and Miller values that are already there — a subset costs its column sums (one device pass a level, over all refused
// chunks), the product of its Miller values, the five fixed-G2 loops and one final exponentiation, and the subsets of a level are judged side by side on the
// host's threads.  A member is accepted only inside a subset whose equation was evaluated and held; a refused subset of at most `leaf` members is judged member by
// member by verify_words, which gives the exact bits with no second implementation of them.  At most 2·(|S| − 1) subsets are asked of a refused chunk S.
// BATCH_NO_BISECT sends a refused chunk to verify_words whole (|S| single verifications).  profiles/batch_bisect.txt has the measured costs behind DEFAULT_LEAF.
//
// Stages (what `Stages` abstracts; one thread an element in each):
//   point_flags   pt_flags over the 8 G1 points and the B of every proof the parse let through
//   lincomb       ROWS rows a proof of out = a + k·b (g1_lincomb_thread) — the folded commitments, −rho·A, rho·C and the eight KZG terms —, the folded commitments back
//                 to the host (it needs their limbs), the other rows summed per chunk by colsum_run over batch_sum_plan's plan; the rows stay where they are
//   subset_sums   the same three column sums over any list of ranges of the resident rows (range_sum_plan): what a bisection level asks
//   miller        miller_thread over (−rho_i·A_i, B_i)
#pragma once
#include <sys/random.h>
#include <chrono>
#include <functional>
#include <thread>
#include "batch_bisect.hpp"
#include "decider_verify.hpp"
#include "pairing_stage.hpp"

namespace vz {
namespace dvb {

using namespace dv;
using pairing::Fq12;

constexpr size_t DEFAULT_CHUNK = 256;      // (a refused chunk without bisection: 256 single verifications of 0.03 s each, over the threads — about half a second)
// the default leaf: the smallest power of two >= 8·kappa, kappa = (one subset evaluation at chunk/2) / (a single verification as the fallback schedules it, 1.87 ms
// over 16 threads).  Measured (profiles/batch_bisect.txt): 20.9 ms an evaluation on the device path (kappa 11.2), 13.3 ms on the host path (kappa 7.1)
constexpr size_t DEFAULT_LEAF = 128, DEFAULT_LEAF_HOST = 64;
constexpr uint32_t BATCH_NO_BISECT = 1;    // flags bit 0 (VIMZ_BATCH_NO_BISECT)
constexpr uint32_t MULT_BITS = 128, FULL_BITS = 254;
// the rows of one proof; row `kind` of survivor j is element kind·m + j of the arrays (a kind's rows side by side: the Miller stage reads kind R_NA as its P)
enum { R_CMW = 0, R_CME, R_NA, R_RC, R_SPIW, R_SPIE, R_XPIW, R_XPIE, R_SUW, R_SLW, R_SUE, R_ST, ROWS };
constexpr uint32_t SUMS = 3;               // columns a chunk: Σ rho·C;  the G1 side of the VK pairing;  that of the G_2 pairing before y·G_1
inline uint32_t row_column(int kind) { return kind == R_RC ? 0u : kind <= R_SPIE ? 1u : 2u; }

// the plan (g16_colsum_plan.hpp) of the sums over the ROWS·m rows of m proofs for a list of ranges [lo, hi) of them: column SUMS·r + s takes the rows of its kind
// of range r's members, coefficient one.  The rows R_CMW, R_CME, R_NA are in no column.  Ranges may be any (a bisection level's are disjoint); an empty list is refused.
inline bool range_sum_plan(size_t m, const bb::Subset* ranges, size_t n_ranges, ColsumPlan* plan) {
  if (!m || !n_ranges || m >= ((size_t)1 << 26) || n_ranges >= ((size_t)1 << 26)) return false;
  std::vector<ColsumUnit> units;
  for (size_t r = 0; r < n_ranges; r++) {
    if (ranges[r].lo >= ranges[r].hi || ranges[r].hi > m) return false;
    for (int kind = R_RC; kind < ROWS; kind++)
      for (size_t j = ranges[r].lo; j < ranges[r].hi; j++) units.push_back({(uint32_t)(kind * m + j), (uint32_t)(SUMS * r + row_column(kind))});
  }
  return colsum_plan(nullptr, 0, units.data(), units.size(), nullptr, 0, BnFr::MOD.w, (uint32_t)(SUMS * n_ranges), (uint32_t)(ROWS * m), plan, nullptr);
}
// the per-chunk sums of m proofs cut into chunks of `chunk`: the ranges are the chunks
inline bool batch_sum_plan(size_t m, size_t chunk, ColsumPlan* plan) {
  if (!m || !chunk) return false;
  std::vector<bb::Subset> ranges;
  for (size_t lo = 0; lo < m; lo += chunk) ranges.push_back({lo, std::min(m, lo + chunk), 1u});
  return range_sum_plan(m, ranges.data(), ranges.size(), plan);
}

struct Stages {
  virtual ~Stages() {}
  // flags1[i], flags2[i] = pt_flags of g1[i] (no order) and of g2[i] (order r); false: the stage failed (the device's error is the context's)
  virtual bool point_flags(const G1A* g1, size_t n1, const G2A* g2, size_t n2, uint32_t* flags1, uint32_t* flags2) = 0;
  // rows = a + k·b over ROWS·m rows; cm <- rows [0, 2m); sums <- the plan's columns.  The rows stay where miller finds them.  k is the caller's to wipe
  virtual bool lincomb(size_t m, const G1A* a, const uint32_t* k, const uint32_t* bits, const G1A* b, const ColsumPlan& plan, G1A* cm, G1A* sums) = 0;
  // out[j] = the Miller value of (rows[R_NA·m + j], B[j])
  virtual bool miller(size_t m, const G2A* B, Fq12* out) = 0;
  // sums <- the columns of a plan of range_sum_plan over the rows lincomb left (m: as lincomb's)
  virtual bool subset_sums(size_t m, const ColsumPlan& plan, G1A* sums) = 0;
};

// fn(lo, hi) over [0, n) on up to `threads` threads
inline void parallel_for(size_t n, unsigned threads, const std::function<void(size_t, size_t)>& fn) {
  const unsigned TH = (unsigned)std::max<size_t>(1, std::min<size_t>(threads, n));
  std::vector<std::thread> th;
  for (unsigned t = 1; t < TH; t++) th.emplace_back(fn, n * t / TH, n * (t + 1) / TH);
  fn(0, n / TH);
  for (auto& x : th) x.join();
}

// every stage as the host's loop over the kernels' per-thread functions
struct HostStages : Stages {
  unsigned threads;
  std::vector<G1A> rows;
  explicit HostStages(unsigned th) : threads(th) {}
  bool point_flags(const G1A* g1, size_t n1, const G2A* g2, size_t n2, uint32_t* flags1, uint32_t* flags2) override {
    const Fq b1 = pairing::fq_u64(3); const Fq2 b2 = pairing::consts().twist_b;
    parallel_for(n1, threads, [&](size_t lo, size_t hi) { for (size_t i = lo; i < hi; i++) pt_flags(i, g1, b1, (const uint32_t*)nullptr, flags1); });
    parallel_for(n2, threads, [&](size_t lo, size_t hi) { for (size_t i = lo; i < hi; i++) pt_flags(i, g2, b2, BnFr::MOD.w, flags2); });
    return true;
  }
  bool lincomb(size_t m, const G1A* a, const uint32_t* k, const uint32_t* bits, const G1A* b, const ColsumPlan& plan, G1A* cm, G1A* sums) override {
    rows.assign(ROWS * m, G1A());
    parallel_for(ROWS * m, threads, [&](size_t lo, size_t hi) { for (size_t t = lo; t < hi; t++) pairing::g1_lincomb_thread(t, a, k, bits, b, rows.data()); });
    memcpy((void*)cm, (const void*)rows.data(), sizeof(G1A) * 2 * m);
    return subset_sums(m, plan, sums);
  }
  bool subset_sums(size_t m, const ColsumPlan& plan, G1A* sums) override {
    if (rows.size() != ROWS * m || plan.n_points != ROWS * m) return false;
    memset((void*)sums, 0, sizeof(G1A) * plan.n_cols);
    std::vector<G1A> partials[2];
    for (size_t lv = 0; lv < plan.levels.size(); lv++) {
      const ColsumLevel& L = plan.levels[lv];
      partials[lv & 1].assign(L.n_partials, G1A());
      const G1A* src = lv ? partials[(lv - 1) & 1].data() : rows.data();
      G1A* dst = partials[lv & 1].data();
      parallel_for(L.runs.size(), threads, [&](size_t lo, size_t hi) {
        for (size_t t = lo; t < hi; t++) colsum_run(t, L.runs.data(), lv ? (const uint32_t*)nullptr : plan.entries.data(), plan.mags.data(), src, dst, sums);
      });
    }
    return true;
  }
  bool miller(size_t m, const G2A* B, Fq12* out) override {
    const pairing::Consts& C = pairing::consts();
    const G1A* P = rows.data() + (size_t)R_NA * m;
    parallel_for(m, threads, [&](size_t lo, size_t hi) { for (size_t j = lo; j < hi; j++) pairing::miller_thread(j, P, B, C.twist_b, C.g12, C.g13, out); });
    return true;
  }
};

inline double since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
inline Fr fr_of_words(const uint64_t* w, int n64) { Fr c = Fr::zero(); memcpy(c.v, w, 8 * n64); return c; }      // canonical
// any 256 bits -> the canonical residue below r (2^256 < 6r)
inline Fr reduce256(const uint64_t* w) {
  Fr c = fr_of_words(w, 4);
  while (!c.is_reduced()) { uint64_t br = 0; for (int i = 0; i < 8; i++) { const uint64_t d = (uint64_t)c.v[i] - BnFr::MOD.w[i] - br; c.v[i] = (uint32_t)d; br = (d >> 32) & 1; } }
  return c;
}
inline bool os_random_bytes(void* buf, size_t n) {
  uint8_t* p = (uint8_t*)buf;
  while (n) { const ssize_t g = getrandom(p, n < 256 ? n : 256, 0); if (g <= 0) return false; p += g; n -= (size_t)g; }
  return true;
}
inline Fq12 miller_one(const G1A& P, const G2A& Q) {
  const pairing::Consts& C = pairing::consts();
  Fq12 f; pairing::miller_thread(0, &P, &Q, C.twist_b, C.g12, C.g13, &f);
  return f;
}

enum { BATCH_OK = 0, BATCH_NO_RANDOMNESS = 1, BATCH_ZERO_MULTIPLIER = 2, BATCH_STAGE_FAILED = 3, BATCH_TOO_MANY = 4 };

// results[i] = what verify_words gives for proof i alone.  steps: n; z0, zi: n·len_z·4 words; words: n·100.  chunk >= 1.  given: NULL — the multipliers are drawn
// from the OS — or 3n multipliers of 2 words (rho_i, sigma_i, sigma'_i of proof i; a test's: with known multipliers a chunk can be forged).  seconds[6] (optional):
// parse + per-proof host work, per-proof stage, Miller loops, host sums + fixed-G2 loops + final exponentiations, fallback (the subset equations of refused chunks
// and the single verifications), total.  flags: BATCH_NO_BISECT.  leaf >= 1.  stats[4] (optional): chunks refused, subset equations evaluated after a refusal,
// single verifications run, members of refused chunks accepted by a subset equation.
inline int verify_batch(const VerifierKey& K, size_t n, const uint64_t* steps, const uint64_t* z0, const uint64_t* zi, const uint64_t* words, size_t chunk,
                        const uint64_t* given, Stages& st, unsigned threads, uint32_t* results, double* seconds, uint32_t flags = 0, size_t leaf = DEFAULT_LEAF,
                        uint64_t* stats = nullptr) {
  if (stats) memset(stats, 0, 8 * bb::ST_N);
  const auto t_all = std::chrono::steady_clock::now();
  double sec[6] = {0, 0, 0, 0, 0, 0};
  auto done = [&](int rc) { sec[5] = since(t_all); if (seconds) memcpy(seconds, sec, sizeof(sec)); return rc; };
  if (!n) return done(BATCH_OK);
  if (n >= ((size_t)1 << 26)) return done(BATCH_TOO_MANY);
  const size_t lz = K.len_z;
  auto z0_of = [&](size_t i) { return z0 + 4 * lz * i; };
  auto zi_of = [&](size_t i) { return zi + 4 * lz * i; };
  auto w_of = [&](size_t i) { return words + 100 * i; };

  // 1. the shared parse; "on its curve" and "killed by r" are the per-point stage's
  auto t0 = std::chrono::steady_clock::now();
  std::vector<Proof> proofs(n);
  std::vector<uint8_t> alive(n, 0);
  parallel_for(n, threads, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) { alive[i] = parse_proof(K, steps[i], z0_of(i), zi_of(i), w_of(i), false, &proofs[i]) ? 1 : 0; results[i] = proofs[i].res; }
  });
  std::vector<size_t> idx;
  for (size_t i = 0; i < n; i++) if (alive[i]) idx.push_back(i);
  sec[0] += since(t0);
  if (idx.empty()) return done(BATCH_OK);

  // 2. the per-point stage
  t0 = std::chrono::steady_clock::now();
  {
    const size_t m = idx.size();
    std::vector<G1A> g1(8 * m); std::vector<G2A> g2(m); std::vector<uint32_t> f1(8 * m, 0), f2(m, 0);
    for (size_t j = 0; j < m; j++) { for (int k = 0; k < 8; k++) g1[8 * j + k] = proofs[idx[j]].P[k]; g2[j] = proofs[idx[j]].B; }
    if (!st.point_flags(g1.data(), g1.size(), g2.data(), m, f1.data(), f2.data())) return done(BATCH_STAGE_FAILED);
    std::vector<size_t> keep;
    for (size_t j = 0; j < m; j++) {
      uint32_t f = f2[j];
      for (int k = 0; k < 8; k++) f |= f1[8 * j + k];
      if (f & (PV_OFF_CURVE | PV_SUBGROUP)) results[idx[j]] |= DV_MALFORMED; else keep.push_back(idx[j]);      // (the identity is a point of either group)
    }
    idx.swap(keep);
  }
  sec[1] += since(t0);
  if (idx.empty()) return done(BATCH_OK);
  const size_t m = idx.size(), n_chunks = (m + chunk - 1) / chunk;

  // 3. the multipliers and the rows; everything that holds a multiplier is wiped when this scope goes
  t0 = std::chrono::steady_clock::now();
  struct Secrets {
    std::vector<uint64_t> mult; std::vector<uint32_t> k;
    ~Secrets() { if (!mult.empty()) explicit_bzero(mult.data(), 8 * mult.size()); if (!k.empty()) explicit_bzero(k.data(), 4 * k.size()); }
  } S;
  S.mult.resize(6 * m);      // rho, sigma, sigma' of survivor j: 2 words each
  if (given) { for (size_t j = 0; j < m; j++) memcpy(&S.mult[6 * j], given + 6 * idx[j], 48); }
  else if (!os_random_bytes(S.mult.data(), 8 * S.mult.size())) return done(BATCH_NO_RANDOMNESS);
  for (size_t q = 0; q < 3 * m; q++) {
    int tries = 0;
    while (!(S.mult[2 * q] | S.mult[2 * q + 1])) { if (given || ++tries > 8 || !os_random_bytes(&S.mult[2 * q], 16)) return done(given ? BATCH_ZERO_MULTIPLIER : BATCH_NO_RANDOMNESS); }
  }
  std::vector<G1A> a(ROWS * m), b(ROWS * m);
  std::vector<uint32_t> bits(ROWS * m);
  S.k.assign(8 * ROWS * m, 0);
  memset((void*)a.data(), 0, sizeof(G1A) * a.size());
  parallel_for(m, threads, [&](size_t lo, size_t hi) {
    for (size_t j = lo; j < hi; j++) {
      const Proof& p = proofs[idx[j]]; const uint64_t* w = w_of(idx[j]);
      const Fr r = reduce256(w + 4 * 8), rm = Fr::to_mont(r);
      const Fr rho = fr_of_words(&S.mult[6 * j], 2), sg[2] = {fr_of_words(&S.mult[6 * j + 2], 2), fr_of_words(&S.mult[6 * j + 4], 2)};
      auto row = [&](int kind, const G1A& base, const Fr& k_canon, uint32_t nbits) { b[kind * m + j] = base; memcpy(&S.k[8 * (kind * m + j)], k_canon.v, 32); bits[kind * m + j] = nbits; };
      a[R_CMW * m + j] = p.P[P_UW]; row(R_CMW, p.P[P_LW], r, FULL_BITS);
      a[R_CME * m + j] = p.P[P_UE]; row(R_CME, p.P[P_T], r, FULL_BITS);
      row(R_NA, g1_negate(p.P[P_A]), rho, MULT_BITS);
      row(R_RC, p.P[P_C], rho, MULT_BITS);
      for (int e = 0; e < 2; e++) {      // the opening of cmW under sigma, that of cmE under sigma'
        const Fr sm = Fr::to_mont(sg[e]);
        const Fr x = Fr::to_mont(fr_of_words(w + 4 * (17 + e), 4));      // (below r: the parse has seen to it)
        const G1A& pi = p.P[e ? P_PIE : P_PIW];
        row(e ? R_SPIE : R_SPIW, pi, sg[e], MULT_BITS);
        row(e ? R_XPIE : R_XPIW, g1_negate(pi), Fr::from_mont(Fr::mul(sm, x)), FULL_BITS);
        row(e ? R_SUE : R_SUW, g1_negate(p.P[e ? P_UE : P_UW]), sg[e], MULT_BITS);
        row(e ? R_ST : R_SLW, g1_negate(p.P[e ? P_T : P_LW]), Fr::from_mont(Fr::mul(sm, rm)), FULL_BITS);
      }
    }
  });
  ColsumPlan plan;
  if (!batch_sum_plan(m, chunk, &plan)) return done(BATCH_TOO_MANY);
  sec[0] += since(t0);

  t0 = std::chrono::steady_clock::now();
  std::vector<G1A> cm(2 * m), sums(SUMS * n_chunks);
  if (!st.lincomb(m, a.data(), S.k.data(), bits.data(), b.data(), plan, cm.data(), sums.data())) return done(BATCH_STAGE_FAILED);
  sec[1] += since(t0);

  // 4. the Miller loops of the proofs' own pairs
  t0 = std::chrono::steady_clock::now();
  std::vector<G2A> Bs(m);
  for (size_t j = 0; j < m; j++) Bs[j] = proofs[idx[j]].B;
  std::vector<Fq12> mv(m);
  if (!st.miller(m, Bs.data(), mv.data())) return done(BATCH_STAGE_FAILED);
  sec[2] += since(t0);

  // 5. the public inputs are finished from the folded commitments, and the chunks judged side by side
  t0 = std::chrono::steady_clock::now();
  parallel_for(m, threads, [&](size_t lo, size_t hi) { for (size_t j = lo; j < hi; j++) finish_public(proofs[idx[j]], w_of(idx[j]), cm[R_CMW * m + j], cm[R_CME * m + j]); });
  sec[0] += since(t0);
  t0 = std::chrono::steady_clock::now();
  const size_t n_pub = K.ic.size() - 1;
  // the equation over the members [lo, hi) with their three column sums: the chunks' body, and a bisection's subsets'
  auto judge = [&](size_t lo, size_t hi, const G1A* sum3) {
    Fr rho_sum = Fr::zero(), y_sum = Fr::zero();
    std::vector<Fr> pub_sum(n_pub, Fr::zero());
    Fq12 f = Fq12::one();
    for (size_t j = lo; j < hi; j++) {
      const Proof& p = proofs[idx[j]]; const uint64_t* w = w_of(idx[j]);
      Fr rho = Fr::to_mont(fr_of_words(&S.mult[6 * j], 2));
      rho_sum = Fr::add(rho_sum, rho);
      for (size_t k = 0; k < n_pub; k++) pub_sum[k] = Fr::add(pub_sum[k], Fr::mul(rho, p.pub[k]));
      for (int e = 0; e < 2; e++) {
        Fr sm = Fr::to_mont(fr_of_words(&S.mult[6 * j + 2 + 2 * e], 2));
        y_sum = Fr::add(y_sum, Fr::mul(sm, Fr::to_mont(fr_of_words(w + 4 * (19 + e), 4))));
        explicit_bzero(&sm, sizeof(sm));
      }
      explicit_bzero(&rho, sizeof(rho));
      f = Fq12::mul(f, mv[j]);
    }
    auto mul = [](const G1A& p, const Fr& k_mont) { const Fr c = Fr::from_mont(k_mont); return pt_scalar_mul(p, c.v); };
    G1X vkx = mul(K.ic[0], rho_sum);
    for (size_t k = 0; k < n_pub; k++) { if (pub_sum[k].is_zero() || aff_is_identity(K.ic[k + 1])) continue; const G1X t = mul(K.ic[k + 1], pub_sum[k]); add_full(vkx, t); }
    G1X g2side = mul(K.kzg_g1, y_sum);
    add_mixed(g2side, sum3[2]);
    f = Fq12::mul(f, miller_one(to_affine(mul(K.alpha, rho_sum)), K.beta));
    f = Fq12::mul(f, miller_one(to_affine(vkx), K.gamma));
    f = Fq12::mul(f, miller_one(sum3[0], K.delta));
    f = Fq12::mul(f, miller_one(sum3[1], K.kzg_vk));
    f = Fq12::mul(f, miller_one(to_affine(g2side), K.kzg_g2));
    const bool ok = pairing::fq12_pow(f, pairing::consts().final_exp).is_one();
    explicit_bzero(&rho_sum, sizeof(rho_sum)); explicit_bzero(&y_sum, sizeof(y_sum));
    if (n_pub) explicit_bzero((void*)pub_sum.data(), sizeof(Fr) * n_pub);
    return ok;
  };
  std::vector<uint8_t> accepted(n_chunks, 0);
  parallel_for(n_chunks, threads, [&](size_t clo, size_t chi) {
    for (size_t c = clo; c < chi; c++) accepted[c] = judge(c * chunk, std::min(m, c * chunk + chunk), &sums[SUMS * c]) ? 1 : 0;
  });
  sec[3] += since(t0);

  // 6. a refused chunk: bisected over the rows and Miller values that are there, its refused leaves member by member (an accepted member keeps its DV_STEPS bit)
  t0 = std::chrono::steady_clock::now();
  std::vector<bb::Subset> roots;
  for (size_t c = 0; c < n_chunks; c++) if (!accepted[c]) roots.push_back({c * chunk, std::min(m, c * chunk + chunk), 1u});
  bb::Outcome out;
  if (flags & BATCH_NO_BISECT) { out.singles = roots; }
  else {
    const bool ok = bb::bisect(roots, leaf, [&](const std::vector<bb::Subset>& ask, std::vector<uint32_t>& held) {
      ColsumPlan sub;
      if (!range_sum_plan(m, ask.data(), ask.size(), &sub)) return false;
      std::vector<G1A> ss(SUMS * ask.size());
      if (!st.subset_sums(m, sub, ss.data())) return false;
      parallel_for(ask.size(), threads, [&](size_t lo, size_t hi) { for (size_t k = lo; k < hi; k++) held[k] = judge(ask[k].lo, ask[k].hi, &ss[SUMS * k]) ? 1u : 0u; });
      return true;
    }, &out);
    if (!ok) return done(BATCH_STAGE_FAILED);
  }
  std::vector<size_t> again;
  for (const bb::Subset& sgl : out.singles) for (size_t j = sgl.lo; j < sgl.hi; j++) again.push_back(idx[j]);
  parallel_for(again.size(), threads, [&](size_t lo, size_t hi) {
    for (size_t q = lo; q < hi; q++) { const size_t i = again[q]; results[i] = verify_words(K, steps[i], z0_of(i), zi_of(i), w_of(i)); }
  });
  if (stats) { stats[bb::ST_REFUSED] = roots.size(); stats[bb::ST_EQUATIONS] = out.equations; stats[bb::ST_SINGLES] = again.size(); stats[bb::ST_ACCEPTED] = out.accepted; }
  sec[4] += since(t0);
  return done(BATCH_OK);
}

}  // namespace dvb
}  // namespace vz
