// Judging a powers-of-tau string before a set-up trusts it (vimz_powers_verify) — what snarkjs's `powersoftau verify` does to a ceremony's
// file, for the arrays a set-up reads: tau_g1 [tau^k]G1, tau_g2 [tau^k]G2, alpha_g1 [alpha·tau^k]G1, beta_g1 [beta·tau^k]G1, and beta_g2.
//
// Stage A, per point (k_powers_flags, one thread per point, 4 bytes of flags in the thread's own slot): not the identity, on its curve, and for the points of
// G2 killed by r — the double-and-add of k_scale_points with the scalar r, decided POINT BY POINT: the twist's cofactor 2q − r has the small factors 10069 and
// 5864401, so a random combination of the points would let a component of such an order through once in ten thousand tries.  (Coordinates below q: the host's
// conversion.)  The host scans the flags for the first one.
// Stage B, per array (k_powers_rlc): S = Σ rho_i·P_i and S' = Σ rho_i·P_(i+1) over the pairs of neighbours, rho_i of 128 bits from the OS.  Thread t owns RLC_CHUNK
// consecutive pairs and walks the 128 bit positions once (g16_point_stage.hpp: pt_rlc_chunk), S and S' are two launches of the same kernel (one accumulator a
// thread: the footprint of k_scale_points), and the chunk sums go through g16_column_sums with a plan of one column: no atomics, no flag another workgroup reads.
// Stage C, on the host (pairing.hpp): S' = tau·S for each array — e(S', G2) = e(S, tau_g2[1]), in G2 e(G1, D') = e(tau_g1[1], D) — which holds for a string of one
// tau and, for any other, with probability at most 2^-128 over the rho; that the two halves share their tau and beta_g1 its beta with beta_g2; the first points.
// A stage runs only when the ones before it found nothing: sums over bad points mean nothing.  Arrays go to the device one at a time.
#include <chrono>
#include <thread>
#include "g16_powers.hpp"
#ifdef VIMZ_TESTING
#include "../../include/vimz_hip_testing.h"
#endif

namespace {

using vz::pairing::Fq2;
static_assert(VIMZ_POWERS_OFF_CURVE == PV_OFF_CURVE && VIMZ_POWERS_IDENTITY == PV_IDENTITY && VIMZ_POWERS_SUBGROUP == PV_SUBGROUP, "the kernel's flags are the verdict's bits");

// thread i is point i (g16_point_stage.hpp: pt_flags)
template <class F>
__global__ void __launch_bounds__(PT_BLOCK) k_powers_flags(const Affine<F>* __restrict__ points, size_t n, F b, const uint32_t* __restrict__ order, uint32_t* __restrict__ flags) {
  const size_t i = blockIdx.x * (size_t)PT_BLOCK + threadIdx.x;
  if (i < n) pt_flags(i, points, b, order, flags);
}
// thread t is chunk t of the combination (pt_rlc_chunk): it writes out[t] alone
template <class F>
__global__ void __launch_bounds__(PT_BLOCK) k_powers_rlc(const Affine<F>* __restrict__ points, size_t n_pairs, size_t n_chunks, const uint32_t* __restrict__ rho, unsigned shift,
                                                         Affine<F>* __restrict__ out) {
  const size_t t = blockIdx.x * (size_t)PT_BLOCK + threadIdx.x;
  if (t < n_chunks) pt_rlc_chunk(t, points, n_pairs, rho, shift, out);
}

unsigned pv_blocks(size_t threads) { return (unsigned)((threads + PT_BLOCK - 1) / PT_BLOCK); }
Fq curve_b(const G1Aff*) { return vz::pairing::fq_u64(3); }
Fq2 curve_b(const G2PowAff*) { return vz::pairing::consts().twist_b; }

template <class F>
hipError_t powers_flags(hipStream_t s, const Affine<F>* points, size_t n, const uint32_t* order, uint32_t* flags) {
  if (!n) return hipSuccess;
  constexpr bool cofactor = !std::is_same<F, Fq>::value;      // G1's is one: on the curve is in the group
  if (!points || !flags || (cofactor && !order) || n > ((size_t)1 << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_powers_flags<F>, dim3(pv_blocks(n)), dim3(PT_BLOCK), 0, s, points, n, curve_b(points), cofactor ? order : (const uint32_t*)nullptr, flags);
  return hipGetLastError();
}
template <class F>
hipError_t powers_rlc(hipStream_t s, const Affine<F>* points, size_t n_pairs, const uint32_t* rho, const ColsumDevice& sum, Affine<F>* chunks, Affine<F>* out) {
  const size_t n_chunks = g16_powers_rlc_chunks(n_pairs);
  if (!points || !rho || !chunks || !out || !n_pairs || n_pairs >= ((size_t)1 << 31) || sum.n_cols != 1 || sum.n_points != n_chunks) return hipErrorInvalidValue;
  for (unsigned shift = 0; shift < 2; shift++) {
    hipLaunchKernelGGL(k_powers_rlc<F>, dim3(pv_blocks(n_chunks)), dim3(PT_BLOCK), 0, s, points, n_pairs, n_chunks, rho, shift, chunks);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = g16_column_sums(s, sum, (const Affine<F>*)chunks, out + shift);      // (the stream orders it before the next pass overwrites the chunks)
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

hipError_t g16_powers_flags(hipStream_t s, const G1Aff* points, size_t n, const uint32_t* order_canon, uint32_t* flags) { return powers_flags<Fq>(s, points, n, order_canon, flags); }
hipError_t g16_powers_flags(hipStream_t s, const G2PowAff* points, size_t n, const uint32_t* order_canon, uint32_t* flags) { return powers_flags<Fq2>(s, points, n, order_canon, flags); }
hipError_t g16_powers_rlc(hipStream_t s, const G1Aff* points, size_t n_pairs, const uint32_t* rho, const ColsumDevice& sum, G1Aff* chunks, G1Aff* out) {
  return powers_rlc<Fq>(s, points, n_pairs, rho, sum, chunks, out);
}
hipError_t g16_powers_rlc(hipStream_t s, const G2PowAff* points, size_t n_pairs, const uint32_t* rho, const ColsumDevice& sum, G2PowAff* chunks, G2PowAff* out) {
  return powers_rlc<Fq2>(s, points, n_pairs, rho, sum, chunks, out);
}
#ifdef VIMZ_TESTING
hipError_t g16_powers_rlc_pass(hipStream_t s, const G1Aff* points, size_t n_pairs, const uint32_t* rho, unsigned shift, G1Aff* chunks) {
  if (!points || !rho || !chunks || !n_pairs || n_pairs >= ((size_t)1 << 31) || shift > 1) return hipErrorInvalidValue;
  const size_t n_chunks = g16_powers_rlc_chunks(n_pairs);
  hipLaunchKernelGGL(k_powers_rlc<Fq>, dim3(pv_blocks(n_chunks)), dim3(PT_BLOCK), 0, s, points, n_pairs, n_chunks, rho, shift, chunks);
  return hipGetLastError();
}
#endif
namespace {

double pv_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

// n points as words (form = VIMZ_FORM_*) -> Montgomery coordinates, on up to 16 threads.  A point with a coordinate not below q becomes zeros and
// hflags[i] = VIMZ_POWERS_COORD: the device's flag for that slot is then not looked at.
template <class A>
void points_in(const uint64_t* words, size_t n, int form, A* out, uint32_t* hflags) {
  const size_t per = sizeof(A) / sizeof(Fq);
  const unsigned TH = (unsigned)std::max<size_t>(1, std::min<size_t>({16, usable_cpus(), n / 4096 + 1}));
  auto work = [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) {
      Fq* c = (Fq*)(out + i);
      bool ok = true;
      for (size_t k = 0; k < per; k++) {
        Fq x; memcpy(x.v, words + 4 * (per * i + k), 32);
        ok = ok && x.is_reduced();
        c[k] = form == VIMZ_FORM_MONTGOMERY ? x : Fq::to_mont(x);
      }
      hflags[i] = ok ? 0u : (uint32_t)VIMZ_POWERS_COORD;
      if (!ok) memset((void*)c, 0, sizeof(A));
    }
  };
  std::vector<std::thread> th;
  for (unsigned t = 1; t < TH; t++) th.emplace_back(work, n * t / TH, n * (t + 1) / TH);
  work(0, n / TH);
  for (auto& x : th) x.join();
}

// what judging one array leaves
template <class A>
struct Judged {
  std::vector<uint32_t> flags;      // per point: VIMZ_POWERS_COORD .. _SUBGROUP, 0 = fine
  uint32_t bits = 0;                // their union
  size_t first = 0;                 // the first flagged index (when bits != 0)
  A head[2];                        // points 0 and 1 (Montgomery; the second only when n > 1)
  A sums[2];                        // S, S' (Montgomery, reduced; when the combination ran)
};

// One array of a string on the context's stream (the caller holds the lock and has set the device): stage A, and — when rho is given and the array is clean —
// stage B.  d_order: r's 8 words on the device; d_rho: 4 words a pair, n − 1 pairs or more, or NULL.  seconds[0..2] are added to.
template <class A>
int judge_array(vimz_ctx* ctx, const uint64_t* words, size_t n, int form, const uint32_t* d_order, const uint32_t* d_rho, Judged<A>* out, double seconds[4]) {
  hipStream_t s = ctx->stream;
  auto t0 = std::chrono::steady_clock::now();
  std::vector<A> pts(n);
  std::vector<uint32_t> hflags(n);
  points_in<A>(words, n, form, pts.data(), hflags.data());
  seconds[0] += pv_since(t0);
  out->head[0] = pts[0]; out->head[1] = pts[n > 1 ? 1 : 0];

  t0 = std::chrono::steady_clock::now();
  struct Dev { A *pts = nullptr, *chunks = nullptr, *sums = nullptr; uint32_t* flags = nullptr; ColsumDevice sum;
               ~Dev() { for (void* p : {(void*)pts, (void*)chunks, (void*)sums, (void*)flags}) if (p) hipFree(p); g16_colsum_free(sum); } } d;
  P_TRY(hipMalloc((void**)&d.pts, sizeof(A) * n)); P_TRY(hipMalloc((void**)&d.flags, 4 * n));
  P_TRY(hipMemcpyAsync(d.pts, pts.data(), sizeof(A) * n, hipMemcpyHostToDevice, s));
  P_TRY(g16_powers_flags(s, (const A*)d.pts, n, d_order, d.flags));
  out->flags.resize(n);
  P_TRY(hipMemcpyAsync(out->flags.data(), d.flags, 4 * n, hipMemcpyDeviceToHost, s));
  P_TRY(hipStreamSynchronize(s));
  out->bits = 0;
  for (size_t i = n; i-- > 0;) {
    if (hflags[i]) out->flags[i] = hflags[i];
    if (out->flags[i]) { out->bits |= out->flags[i]; out->first = i; }
  }
  seconds[1] += pv_since(t0);
  if (out->bits || !d_rho || n < 2) return VIMZ_OK;

  t0 = std::chrono::steady_clock::now();
  const size_t n_pairs = n - 1, n_chunks = g16_powers_rlc_chunks(n_pairs);
  ColsumPlan plan;
  if (!rlc_sum_plan(n_chunks, &plan)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_powers_verify: the array is too long");
  P_TRY(g16_colsum_upload(plan, sizeof(A), &d.sum));
  P_TRY(hipMalloc((void**)&d.chunks, sizeof(A) * n_chunks)); P_TRY(hipMalloc((void**)&d.sums, sizeof(A) * 2));
  P_TRY(g16_powers_rlc(s, (const A*)d.pts, n_pairs, d_rho, d.sum, d.chunks, d.sums));
  P_TRY(hipMemcpyAsync(out->sums, d.sums, sizeof(A) * 2, hipMemcpyDeviceToHost, s));
  P_TRY(hipStreamSynchronize(s));
  seconds[2] += pv_since(t0);
  return VIMZ_OK;
}

// r's words and the pairs' scalars on the device; the scalars are wiped on both sides when this goes
struct Scalars {
  std::vector<uint32_t> rho; uint32_t *d_order = nullptr, *d_rho = nullptr; hipStream_t s = nullptr;
  ~Scalars() {
    if (!rho.empty()) explicit_bzero(rho.data(), 4 * rho.size());
    if (d_rho) { hipMemsetAsync(d_rho, 0, 4 * rho.size(), s); hipStreamSynchronize(s); hipFree(d_rho); }
    if (d_order) hipFree(d_order);
  }
  hipError_t upload(hipStream_t stream) {
    s = stream;
    hipError_t e = hipMalloc((void**)&d_order, 32);
    if (e == hipSuccess) e = hipMemcpyAsync(d_order, BnFr::MOD.w, 32, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && !rho.empty()) e = hipMalloc((void**)&d_rho, 4 * rho.size());
    if (e == hipSuccess && !rho.empty()) e = hipMemcpyAsync(d_rho, rho.data(), 4 * rho.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e;
  }
};

G1Aff g1_neg(G1Aff p) { if (!aff_is_identity(p)) p.y = Fq::neg(p.y); return p; }
bool same_point(const G1Aff& p, const G1Aff& q) { return p.x.eq(q.x) && p.y.eq(q.y); }
bool same_point(const G2PowAff& p, const G2PowAff& q) { return p.x.eq(q.x) && p.y.eq(q.y); }

}  // namespace

extern "C" int vimz_powers_verify(vimz_ctx* ctx, const uint64_t* tau_g1, size_t n_tau_g1, const uint64_t* tau_g2, const uint64_t* alpha_g1, const uint64_t* beta_g1, size_t n_pow,
                                  const uint64_t beta_g2[16], int form, uint32_t* result, uint64_t first_bad[2], double seconds[4]) {
  if (!ctx || !tau_g1 || !tau_g2 || !alpha_g1 || !beta_g1 || !beta_g2 || !result || !first_bad) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_powers_verify: NULL argument");
  if (form != VIMZ_FORM_CANONICAL && form != VIMZ_FORM_MONTGOMERY) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_powers_verify: form is VIMZ_FORM_*");
  if (n_pow < 2 || n_tau_g1 < n_pow) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_powers_verify: needs n_pow >= 2 and n_tau_g1 >= n_pow");
  if (!vz::pairing::consts().ok) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_powers_verify: pairing constants");
  double sec[4] = {0, 0, 0, 0};
  *result = 0; first_bad[0] = first_bad[1] = 0;
  Judged<G1Aff> tau1, alpha, beta; Judged<G2PowAff> tau2, beta2;
  {
    std::lock_guard<std::mutex> g(ctx->mu);
    P_TRY(hipSetDevice(ctx->device));
    Scalars sc;
    sc.rho.resize(4 * (n_tau_g1 - 1));      // one vector for the four arrays: each equation is wrong with probability at most 2^-128 on its own
    if (!g16_os_random(sc.rho.data(), 4 * sc.rho.size())) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_powers_verify: no randomness from the OS");
    P_TRY(sc.upload(ctx->stream));
    // beta_g2 first (one point), so that no sum is made of a string it spoils; the arrays then in their order, each alone on the device
    int rc = judge_array<G2PowAff>(ctx, beta_g2, 1, form, sc.d_order, nullptr, &beta2, sec);
    const uint32_t* rho = beta2.bits ? nullptr : sc.d_rho;
    uint32_t bits = 0; uint64_t which = 0, where = 0;
    auto found = [&](uint32_t b, uint64_t array, size_t index) { if (b && !bits) { bits = b; which = array; where = index; } };
    if (!rc) { rc = judge_array<G1Aff>(ctx, tau_g1, n_tau_g1, form, sc.d_order, rho, &tau1, sec); found(tau1.bits, 1, tau1.first); }
    if (!rc && !bits) { rc = judge_array<G2PowAff>(ctx, tau_g2, n_pow, form, sc.d_order, rho, &tau2, sec); found(tau2.bits, 2, tau2.first); }
    if (!rc && !bits) { rc = judge_array<G1Aff>(ctx, alpha_g1, n_pow, form, sc.d_order, rho, &alpha, sec); found(alpha.bits, 3, alpha.first); }
    if (!rc && !bits) { rc = judge_array<G1Aff>(ctx, beta_g1, n_pow, form, sc.d_order, rho, &beta, sec); found(beta.bits, 4, beta.first); }
    if (rc) return rc;
    found(beta2.bits, 5, 0);
    if (!bits) {
      if (!same_point(tau1.head[0], g16_g1_generator())) found(VIMZ_POWERS_FIRST, 1, 0);
      else if (!same_point(tau2.head[0], g16_g2_generator())) found(VIMZ_POWERS_FIRST, 2, 0);
    }
    if (bits) {
      *result = bits; first_bad[0] = which; first_bad[1] = where;
      if (seconds) memcpy(seconds, sec, sizeof(sec));
      return VIMZ_OK;
    }
  }
  // stage C: six products of two pairings, side by side
  const auto t0 = std::chrono::steady_clock::now();
  const G1Aff g1 = g16_g1_generator(); const G2PowAff g2 = g16_g2_generator();
  typedef std::vector<std::pair<G1Aff, G2PowAff>> Pairs;
  auto ratio_g1 = [&](const Judged<G1Aff>& a) { return Pairs{{a.sums[1], g2}, {g1_neg(a.sums[0]), tau2.head[1]}}; };
  const struct { Pairs pairs; uint32_t bit; } eqs[6] = {
      {ratio_g1(tau1), VIMZ_POWERS_RATIO_TAU_G1}, {ratio_g1(alpha), VIMZ_POWERS_RATIO_ALPHA_G1}, {ratio_g1(beta), VIMZ_POWERS_RATIO_BETA_G1},
      {Pairs{{g1, tau2.sums[1]}, {g1_neg(tau1.head[1]), tau2.sums[0]}}, VIMZ_POWERS_RATIO_TAU_G2},
      {Pairs{{tau1.head[1], g2}, {g1_neg(g1), tau2.head[1]}}, VIMZ_POWERS_HALVES},
      {Pairs{{beta.head[0], g2}, {g1_neg(g1), beta2.head[0]}}, VIMZ_POWERS_BETA}};
  bool holds[6];
  { std::vector<std::thread> th;
    for (int k = 0; k < 6; k++) th.emplace_back([&eqs, &holds, k] { holds[k] = vz::pairing::product_is_one(eqs[k].pairs); });
    for (auto& x : th) x.join(); }
  for (int k = 0; k < 6; k++) if (!holds[k]) *result |= eqs[k].bit;
  sec[3] = pv_since(t0);
  if (seconds) memcpy(seconds, sec, sizeof(sec));
  return VIMZ_OK;
}

#ifdef VIMZ_TESTING
namespace {
template <class A>
int test_flags(vimz_ctx* ctx, const uint64_t* points, size_t n, int form, uint32_t* flags) {
  double sec[4] = {0, 0, 0, 0};
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  Judged<A> j; Scalars sc;
  P_TRY(sc.upload(ctx->stream));
  const int rc = judge_array<A>(ctx, points, n, form, sc.d_order, nullptr, &j, sec);
  if (rc) return rc;
  memcpy(flags, j.flags.data(), 4 * n);
  return VIMZ_OK;
}
template <class A>
int test_rlc(vimz_ctx* ctx, const uint64_t* points, size_t n, const uint64_t* rho, int form, uint64_t* out) {
  double sec[4] = {0, 0, 0, 0};
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  Judged<A> j; Scalars sc;
  sc.rho.resize(4 * (n - 1)); memcpy(sc.rho.data(), rho, 16 * (n - 1));
  P_TRY(sc.upload(ctx->stream));
  const int rc = judge_array<A>(ctx, points, n, form, sc.d_order, sc.d_rho, &j, sec);
  if (rc) return rc;
  if (j.bits) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_powers_rlc: a point is flagged");
  const Fq* c = (const Fq*)j.sums;
  for (size_t k = 0; k < 2 * sizeof(A) / sizeof(Fq); k++) { const Fq w = form == VIMZ_FORM_MONTGOMERY ? c[k] : Fq::from_mont(c[k]); memcpy(out + 4 * k, w.v, 32); }
  return VIMZ_OK;
}
}  // namespace

extern "C" int vimz_test_powers_flags(vimz_ctx* ctx, int group, const uint64_t* points, size_t n, int form, uint32_t* flags) {
  if (!ctx || !points || !flags || (group != 1 && group != 2) || (form != VIMZ_FORM_CANONICAL && form != VIMZ_FORM_MONTGOMERY) || !n || n > (1u << 26))
    return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_powers_flags: bad argument");
  return group == 1 ? test_flags<G1Aff>(ctx, points, n, form, flags) : test_flags<G2PowAff>(ctx, points, n, form, flags);
}
extern "C" int vimz_test_powers_rlc(vimz_ctx* ctx, int group, const uint64_t* points, size_t n, const uint64_t* rho, int form, uint64_t* out) {
  if (!ctx || !points || !rho || !out || (group != 1 && group != 2) || (form != VIMZ_FORM_CANONICAL && form != VIMZ_FORM_MONTGOMERY) || n < 2 || n > (1u << 26))
    return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_powers_rlc: bad argument");
  return group == 1 ? test_rlc<G1Aff>(ctx, points, n, rho, form, out) : test_rlc<G2PowAff>(ctx, points, n, rho, form, out);
}
#endif
