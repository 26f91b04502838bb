// A contribution to a powers-of-tau string, and the check of a chain of them (vimz_powers_contribute, vimz_powers_verify_contributions): phase 1
// of a ceremony — snarkjs's `powersoftau contribute` and the chain half of `powersoftau verify` — on the arrays vimz_powers_verify takes.  The host side (the record
// and its three proofs of knowledge): g16_powers_contrib.hpp.
//
// Contribute: tau', alpha', beta' and three nonces from the OS; the record on the host; then ONE power vector pw[k] = tau'^k of n_tau_g1 entries on the device
// (k_power_vec, Montgomery words) and four launches of k_scale_points_by that differ in the kernel argument c alone — out[k] = (c·pw[k])·P[k] with c = 1 for tau_g1
// and tau_g2, alpha' for alpha_g1, beta' for beta_g1 —, each array alone in one device buffer that is reused: peak device memory is one array and the vector.  beta_g2
// is one multiplication on the host.  The vector is overwritten before it is freed on every path (struct Dev), as 1/delta' is in g16_key_contrib.hip; c and tau'
// travel as kernel arguments.  Outputs are written once everything has succeeded.
// Both kernels: PT_BLOCK threads, one thread per element, a thread writes its own slot alone, no atomics, no LDS, nothing another workgroup writes is read, every
// loop bound (the power's bit count) from the host.  In k_scale_points_by the lanes of a wave walk DIFFERENT scalars, so a wave diverges on the additions as
// k_pt_stage does: every one of the 254 steps runs the doubling once and the addition once for the lanes whose bit is set (about half of them); the cost a point is
// that of k_pt_stage's multiplication, not of k_scale_points' uniform walk.  The walk over a secret's bits is not constant-time.
// Verify, stage by stage, a stage only when the ones before it found nothing (host, but for the last):
//   points     the origin's three points and every record's nine have coordinates below q, are on the curve and are not the identity.
//   knowledge  per record z_s·B_s = T_s + c_s·A_s for s in (tau', alpha', beta') over the points of the record before it; the last record's points are the final
//              string's tau_g1[1], alpha_g1[0], beta_g1[0].  Records side by side on host threads.
//   string     vimz_powers_verify on the final string as it stands: that call's verdict decides, and ties every other point of the string to those three.
#include <atomic>
#include <chrono>
#include <thread>
#include "g16_powers.hpp"
#include "g16_powers_contrib.hpp"
#ifdef VIMZ_TESTING
#include "../../include/vimz_hip_testing.h"
#endif

namespace {

using namespace vz::powc;
static_assert(VIMZ_POWCHAIN_RECORD_WORDS == RECORD_WORDS, "the record's size is part of the ABI");
static_assert(VIMZ_POWCHAIN_COORD == VIMZ_POWERS_COORD && VIMZ_POWCHAIN_OFF_CURVE == VIMZ_POWERS_OFF_CURVE && VIMZ_POWCHAIN_IDENTITY == VIMZ_POWERS_IDENTITY, "one meaning a bit");
static_assert(VIMZ_POWCHAIN_AT_STRING_TAU_G1 == VIMZ_POWCHAIN_AT_RECORD + 1 && VIMZ_POWCHAIN_AT_STRING_BETA_G2 == VIMZ_POWCHAIN_AT_RECORD + 5, "2 + the array's number");

// thread i is power i (g16_point_stage.hpp: pt_power)
__global__ void __launch_bounds__(PT_BLOCK) k_power_vec(uint32_t* __restrict__ pw, size_t count, int bits, Fe w) {
  const size_t i = blockIdx.x * (size_t)PT_BLOCK + threadIdx.x;
  if (i < count) pt_power(i, bits, w, pw);
}
// thread i is point i (pt_scale_by): it reads in[i] and pw[i] and writes out[i] alone
template <class F>
__global__ void __launch_bounds__(PT_BLOCK) k_scale_points_by(const Affine<F>* in, size_t n, const uint32_t* __restrict__ pw, Fe c, Affine<F>* out /* may be in */) {
  const size_t i = blockIdx.x * (size_t)PT_BLOCK + threadIdx.x;
  if (i < n) pt_scale_by(i, in, pw, c, out);
}

unsigned pc_blocks(size_t threads) { return (unsigned)((threads + PT_BLOCK - 1) / PT_BLOCK); }
int pc_bitlen(size_t v) { int b = 0; while (v) { b++; v >>= 1; } return b; }
double pc_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

template <class F>
hipError_t scale_points_by(hipStream_t s, const Affine<F>* in, size_t n, const uint32_t* pw, const Fe& c, Affine<F>* out) {
  if (!n) return hipSuccess;
  if (!in || !out || !pw || n > ((size_t)1 << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_scale_points_by<F>, dim3(pc_blocks(n)), dim3(PT_BLOCK), 0, s, in, n, pw, c, out);
  return hipGetLastError();
}

}  // namespace

hipError_t g16_power_vec(hipStream_t s, uint32_t* pw, size_t count, const Fe& w) {
  if (!count) return hipSuccess;
  if (!pw || count > ((size_t)1 << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_power_vec, dim3(pc_blocks(count)), dim3(PT_BLOCK), 0, s, pw, count, pc_bitlen(count - 1), w);
  return hipGetLastError();
}
hipError_t g16_scale_points_by(hipStream_t s, const G1Aff* in, size_t n, const uint32_t* pw, const Fe& c, G1Aff* out) { return scale_points_by<Fq>(s, in, n, pw, c, out); }
hipError_t g16_scale_points_by(hipStream_t s, const G2PowAff* in, size_t n, const uint32_t* pw, const Fe& c, G2PowAff* out) { return scale_points_by<vz::pairing::Fq2>(s, in, n, pw, c, out); }

namespace {

bool pc_on_curve(const G1Aff& p) { return vz::pairing::g1_on_curve(p); }
bool pc_on_curve(const G2PowAff& p) { return vz::pairing::g2_on_curve(p); }

// n points as words (form = VIMZ_FORM_*) -> Montgomery coordinates on up to 16 threads.  The result: 0 fine, VIMZ_POWCHAIN_COORD when a coordinate is not below q,
// _OFF_CURVE when a point is not on its curve (the identity, zeros, is on both).
template <class A>
uint32_t pc_points_in(const uint64_t* words, size_t n, int form, A* out) {
  const size_t per = sizeof(A) / sizeof(Fq);
  const unsigned TH = (unsigned)std::max<size_t>(1, std::min<size_t>({16, usable_cpus(), n / 4096 + 1}));
  std::vector<uint32_t> found(TH, 0);
  auto work = [&](unsigned t, size_t lo, size_t hi) {
    uint32_t f = 0;
    for (size_t i = lo; i < hi; i++) {
      Fq* c = (Fq*)(out + i);
      bool ok = true;
      for (size_t k = 0; k < per; k++) {
        Fq x; memcpy(x.v, words + 4 * (per * i + k), 32);
        ok = ok && x.is_reduced();
        c[k] = form == VIMZ_FORM_MONTGOMERY ? x : Fq::to_mont(x);
      }
      if (!ok) f |= VIMZ_POWCHAIN_COORD; else if (!pc_on_curve(out[i])) f |= VIMZ_POWCHAIN_OFF_CURVE;
    }
    found[t] = f;
  };
  std::vector<std::thread> th;
  for (unsigned t = 1; t < TH; t++) th.emplace_back(work, t, n * t / TH, n * (t + 1) / TH);
  work(0, 0, n / TH);
  for (auto& x : th) x.join();
  uint32_t all = 0;
  for (uint32_t f : found) all |= f;
  return all;
}
template <class A>
void pc_points_out(const A* pts, size_t n, int form, uint64_t* words) {
  const size_t per = sizeof(A) / sizeof(Fq);
  const unsigned TH = (unsigned)std::max<size_t>(1, std::min<size_t>({16, usable_cpus(), n / 4096 + 1}));
  auto work = [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) {
      const Fq* c = (const Fq*)(pts + i);
      for (size_t k = 0; k < per; k++) { const Fq x = form == VIMZ_FORM_MONTGOMERY ? c[k] : Fq::from_mont(c[k]); memcpy(words + 4 * (per * i + k), x.v, 32); }
    }
  };
  std::vector<std::thread> th;
  for (unsigned t = 1; t < TH; t++) th.emplace_back(work, n * t / TH, n * (t + 1) / TH);
  work(0, n / TH);
  for (auto& x : th) x.join();
}

// a non-zero element of Fr from the OS (rejection sampling over 254 bits), Montgomery
bool pc_fr_nonzero_random(Fe* out) {
  for (;;) {
    Fe c;
    if (!g16_os_random(c.v, 32)) return false;
    c.v[7] &= 0x3fffffffu;
    if (c.is_reduced() && !c.is_zero()) { *out = Fe::to_mont(c); explicit_bzero(&c, sizeof(c)); return true; }
  }
}

// the power vector and the one buffer the arrays take turns in; the vector is overwritten before it is freed, whichever way the call ends
struct ContribDev {
  uint32_t* pw = nullptr; size_t pw_bytes = 0; void* pts = nullptr; hipStream_t s = nullptr;
  ~ContribDev() {
    if (pw) { hipMemsetAsync(pw, 0, pw_bytes, s); hipStreamSynchronize(s); hipFree(pw); }
    if (pts) hipFree(pts);
  }
};
template <class A>
int scale_array(vimz_ctx* ctx, ContribDev& d, std::vector<A>& pts, const Fe& c) {
  A* dp = (A*)d.pts;
  P_TRY(hipMemcpyAsync(dp, pts.data(), sizeof(A) * pts.size(), hipMemcpyHostToDevice, d.s));
  P_TRY(g16_scale_points_by(d.s, (const A*)dp, pts.size(), d.pw, c, dp));
  P_TRY(hipMemcpyAsync(pts.data(), dp, sizeof(A) * pts.size(), hipMemcpyDeviceToHost, d.s));
  P_TRY(hipStreamSynchronize(d.s));
  return VIMZ_OK;
}

// given: the test hook's secrets tau', alpha', beta' and nonces (Montgomery); NULL: drawn from the OS.  seconds (optional) = {host, device, total}
int powers_contribute_impl(vimz_ctx* ctx, const char* who, const uint64_t* tau_g1, size_t n_tau_g1, const uint64_t* tau_g2, const uint64_t* alpha_g1, const uint64_t* beta_g1, size_t n_pow,
                           const uint64_t* beta_g2, int form, uint64_t* tau_g1_out, uint64_t* tau_g2_out, uint64_t* alpha_g1_out, uint64_t* beta_g1_out, uint64_t* beta_g2_out,
                           uint64_t* record_out, const Fe* secrets_given, const Fe* nonces_given, double seconds[3]) {
  auto bad = [&](const char* m) { return vz_fail(ctx, VIMZ_ERR_INVALID, (std::string(who) + ": " + m).c_str()); };
  if (!ctx) return VIMZ_ERR_INVALID;
  if (!tau_g1 || !tau_g2 || !alpha_g1 || !beta_g1 || !beta_g2 || !tau_g1_out || !tau_g2_out || !alpha_g1_out || !beta_g1_out || !beta_g2_out || !record_out) return bad("NULL argument");
  if (form != VIMZ_FORM_CANONICAL && form != VIMZ_FORM_MONTGOMERY) return bad("form is VIMZ_FORM_*");
  if (n_pow < 2 || n_tau_g1 < n_pow || n_tau_g1 > ((size_t)1 << 28)) return bad("needs n_pow >= 2 and n_tau_g1 >= n_pow");
  if (!vz::pairing::consts().ok) return bad("pairing constants");
  const auto t_all = std::chrono::steady_clock::now();
  std::vector<G1Aff> tau1(n_tau_g1), alpha(n_pow), beta(n_pow);
  std::vector<G2PowAff> tau2(n_pow), beta2(1);
  { const uint32_t f = pc_points_in(tau_g1, n_tau_g1, form, tau1.data()) | pc_points_in(tau_g2, n_pow, form, tau2.data()) | pc_points_in(alpha_g1, n_pow, form, alpha.data()) |
                       pc_points_in(beta_g1, n_pow, form, beta.data()) | pc_points_in(beta_g2, 1, form, beta2.data());
    if (f & VIMZ_POWCHAIN_COORD) return bad("a coordinate is not below q");
    if (f & VIMZ_POWCHAIN_OFF_CURVE) return bad("a point is not on its curve"); }
  const G1Aff before[3] = {tau1[1], alpha[0], beta[0]};
  for (const G1Aff& p : before) if (aff_is_identity(p)) return bad("tau_g1[1], alpha_g1[0] or beta_g1[0] is the identity");
  // tau', alpha', beta' and the nonces: this party's secrets, wiped on every path
  struct Secret { Fe s[3], k[3], beta_canon; ~Secret() { explicit_bzero(this, sizeof(*this)); } } sec;
  for (int i = 0; i < 3; i++) {
    if (secrets_given) sec.s[i] = secrets_given[i]; else if (!pc_fr_nonzero_random(&sec.s[i])) return bad("no randomness from the OS");
    if (nonces_given) sec.k[i] = nonces_given[i]; else if (!pc_fr_nonzero_random(&sec.k[i])) return bad("no randomness from the OS");
    if (sec.s[i].is_zero()) return bad("a secret is zero");
  }
  uint64_t record[RECORD_WORDS];
  make_powers_record(before, sec.s, sec.k, record);
  sec.beta_canon = Fe::from_mont(sec.s[2]);
  beta2[0] = to_affine(pt_scalar_mul(beta2[0], sec.beta_canon.v));
  const auto t_dev = std::chrono::steady_clock::now();
  {
    std::lock_guard<std::mutex> g(ctx->mu);
    P_TRY(hipSetDevice(ctx->device));
    ContribDev d;
    d.s = ctx->stream;
    d.pw_bytes = 32 * n_tau_g1;
    P_TRY(hipMalloc((void**)&d.pw, d.pw_bytes));
    P_TRY(hipMalloc(&d.pts, std::max(sizeof(G1Aff) * n_tau_g1, sizeof(G2PowAff) * n_pow)));
    P_TRY(g16_power_vec(d.s, d.pw, n_tau_g1, sec.s[0]));
    int rc = scale_array(ctx, d, tau1, Fe::one());
    if (!rc) rc = scale_array(ctx, d, tau2, Fe::one());
    if (!rc) rc = scale_array(ctx, d, alpha, sec.s[1]);
    if (!rc) rc = scale_array(ctx, d, beta, sec.s[2]);
    if (rc) return rc;
  }
  const double t_device = pc_since(t_dev);
  // nothing was written so far: the outputs may be the inputs
  pc_points_out(tau1.data(), n_tau_g1, form, tau_g1_out); pc_points_out(tau2.data(), n_pow, form, tau_g2_out);
  pc_points_out(alpha.data(), n_pow, form, alpha_g1_out); pc_points_out(beta.data(), n_pow, form, beta_g1_out);
  pc_points_out(beta2.data(), 1, form, beta_g2_out);
  memcpy(record_out, record, sizeof(record));
  if (seconds) { seconds[2] = pc_since(t_all); seconds[1] = t_device; seconds[0] = seconds[2] - t_device; }
  return VIMZ_OK;
}

// what is wrong with a G1 point given as canonical words (VIMZ_POWCHAIN_* bits; 0: nothing)
uint32_t pc_point_bits(const uint64_t* words, G1Aff* p) {
  if (!get_g1(words, p)) return VIMZ_POWCHAIN_COORD;
  if (aff_is_identity(*p)) return VIMZ_POWCHAIN_IDENTITY;
  return vz::pairing::g1_on_curve(*p) ? 0u : (uint32_t)VIMZ_POWCHAIN_OFF_CURVE;
}

}  // namespace

extern "C" int vimz_powers_contribute(vimz_ctx* ctx, const uint64_t* tau_g1, size_t n_tau_g1, const uint64_t* tau_g2, const uint64_t* alpha_g1, const uint64_t* beta_g1, size_t n_pow,
                                      const uint64_t beta_g2[16], int form, uint64_t* tau_g1_out, uint64_t* tau_g2_out, uint64_t* alpha_g1_out, uint64_t* beta_g1_out,
                                      uint64_t beta_g2_out[16], uint64_t record_out[VIMZ_POWCHAIN_RECORD_WORDS], double seconds[3]) {
  return powers_contribute_impl(ctx, "vimz_powers_contribute", tau_g1, n_tau_g1, tau_g2, alpha_g1, beta_g1, n_pow, beta_g2, form, tau_g1_out, tau_g2_out, alpha_g1_out, beta_g1_out,
                                beta_g2_out, record_out, nullptr, nullptr, seconds);
}

extern "C" int vimz_powers_verify_contributions(vimz_ctx* ctx, const uint64_t origin_points[24], const uint64_t* tau_g1, size_t n_tau_g1, const uint64_t* tau_g2, const uint64_t* alpha_g1,
                                                const uint64_t* beta_g1, size_t n_pow, const uint64_t beta_g2[16], int form, const uint64_t* records, size_t n_records,
                                                uint32_t* result, uint32_t* string_result, uint64_t first_bad[2], double seconds[3]) {
  auto bad = [&](const std::string& m) { return vz_fail(ctx, VIMZ_ERR_INVALID, ("vimz_powers_verify_contributions: " + m).c_str()); };
  if (!ctx) return VIMZ_ERR_INVALID;
  if (!origin_points || !tau_g1 || !tau_g2 || !alpha_g1 || !beta_g1 || !beta_g2 || !result || !string_result || !first_bad || (n_records && !records)) return bad("NULL argument");
  if (form != VIMZ_FORM_CANONICAL && form != VIMZ_FORM_MONTGOMERY) return bad("form is VIMZ_FORM_*");
  if (n_pow < 2 || n_tau_g1 < n_pow) return bad("needs n_pow >= 2 and n_tau_g1 >= n_pow");
  { size_t j = 0;
    if (n_records > ((size_t)1 << 32)) return bad("too many records");
    if (const char* why = powers_records_layout(records, 8 * RECORD_WORDS * n_records, &j)) return bad("record " + std::to_string(j) + ": " + why); }
  double sec[3] = {0, 0, 0};
  *result = 0; *string_result = 0; first_bad[0] = first_bad[1] = 0;
  auto verdict = [&](uint32_t bits, uint64_t what, uint64_t where) {
    *result = bits; first_bad[0] = what; first_bad[1] = where;
    if (seconds) memcpy(seconds, sec, sizeof(sec));
    return VIMZ_OK;
  };
  // ---- the points ----
  auto t0 = std::chrono::steady_clock::now();
  struct Rec { G1Aff A[3], T[3]; };
  G1Aff origin[3];
  std::vector<Rec> recs(n_records);
  for (unsigned s = 0; s < 3; s++) if (const uint32_t b = pc_point_bits(origin_points + 8 * s, &origin[s])) return verdict(b, VIMZ_POWCHAIN_AT_ORIGIN, s);
  for (size_t j = 0; j < n_records; j++) {
    const uint64_t* r = records + RECORD_WORDS * j;
    uint32_t b = 0;
    for (unsigned s = 0; s < 3; s++) b |= pc_point_bits(r + REC_A + 8 * s, &recs[j].A[s]) | pc_point_bits(r + REC_T + 8 * s, &recs[j].T[s]);
    if (b) return verdict(b, VIMZ_POWCHAIN_AT_RECORD, j);
  }
  sec[0] = pc_since(t0);
  // ---- knowledge ----
  t0 = std::chrono::steady_clock::now();
  std::vector<unsigned> failed(n_records, 0);
  { std::atomic<size_t> next{0};
    auto work = [&] {
      for (size_t j; (j = next.fetch_add(1)) < n_records;)
        failed[j] = powers_record_knowledge(j ? records + RECORD_WORDS * (j - 1) + REC_A : origin_points, j ? recs[j - 1].A : origin, recs[j].A, recs[j].T, records + RECORD_WORDS * j);
    };
    std::vector<std::thread> th;
    for (size_t t = 1; t < std::min<size_t>({16, usable_cpus(), n_records}); t++) th.emplace_back(work);
    work();
    for (auto& x : th) x.join(); }
  uint32_t bits = 0; uint64_t what = 0, where = 0;
  for (size_t j = n_records; j-- > 0;) {
    if (failed[j] & 1u) bits |= VIMZ_POWCHAIN_KNOWLEDGE_TAU;
    if (failed[j] & 2u) bits |= VIMZ_POWCHAIN_KNOWLEDGE_ALPHA;
    if (failed[j] & 4u) bits |= VIMZ_POWCHAIN_KNOWLEDGE_BETA;
    if (failed[j]) { what = VIMZ_POWCHAIN_AT_RECORD; where = j; }
  }
  { // the last record's points, in the string's form, beside the string's own words
    const uint64_t* last = n_records ? records + RECORD_WORDS * (n_records - 1) + REC_A : origin_points;
    const uint64_t* theirs[3] = {tau_g1 + 8, alpha_g1, beta_g1};
    for (unsigned s = 0; s < 3; s++) {
      uint64_t mine[8];
      for (unsigned k = 0; k < 2; k++) {
        Fq c; memcpy(c.v, last + 8 * s + 4 * k, 32);      // (below q: the points stage)
        if (form == VIMZ_FORM_MONTGOMERY) c = Fq::to_mont(c);
        memcpy(mine + 4 * k, c.v, 32);
      }
      if (memcmp(mine, theirs[s], 64)) bits |= VIMZ_POWCHAIN_LAST;
    } }
  sec[1] = pc_since(t0);
  if (bits) return verdict(bits, what, where);
  // ---- the string ----
  t0 = std::chrono::steady_clock::now();
  uint64_t fb[2] = {0, 0};
  const int rc = vimz_powers_verify(ctx, tau_g1, n_tau_g1, tau_g2, alpha_g1, beta_g1, n_pow, beta_g2, form, string_result, fb, nullptr);
  if (rc) return rc;
  sec[2] = pc_since(t0);
  if (*string_result) return verdict(VIMZ_POWCHAIN_STRING, fb[0] ? VIMZ_POWCHAIN_AT_RECORD + fb[0] : 0, fb[1]);
  return verdict(0, 0, 0);
}

#ifdef VIMZ_TESTING
namespace {
bool pc_fr_given(const uint64_t w[4], Fe* out) { Fe c; memcpy(c.v, w, 32); if (!c.is_reduced()) return false; *out = Fe::to_mont(c); explicit_bzero(&c, sizeof(c)); return true; }

template <class A>
int test_scale_by(vimz_ctx* ctx, const uint64_t* points, size_t n, const Fe& w, const Fe& c, int form, uint64_t* out) {
  std::vector<A> pts(n);
  const uint32_t f = pc_points_in(points, n, form, pts.data());
  if (f & VIMZ_POWCHAIN_COORD) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_scale_points_by: a coordinate is not below q");
  if (f) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_scale_points_by: a point is not on its curve");
  { std::lock_guard<std::mutex> g(ctx->mu);
    P_TRY(hipSetDevice(ctx->device));
    ContribDev d;
    d.s = ctx->stream; d.pw_bytes = 32 * n;
    P_TRY(hipMalloc((void**)&d.pw, d.pw_bytes)); P_TRY(hipMalloc(&d.pts, sizeof(A) * n));
    P_TRY(g16_power_vec(d.s, d.pw, n, w));
    const int rc = scale_array(ctx, d, pts, c);
    if (rc) return rc; }
  pc_points_out(pts.data(), n, form, out);
  return VIMZ_OK;
}
}  // namespace

extern "C" int vimz_testing_powers_contribute_secrets(vimz_ctx* ctx, const uint64_t* tau_g1, size_t n_tau_g1, const uint64_t* tau_g2, const uint64_t* alpha_g1, const uint64_t* beta_g1,
                                                      size_t n_pow, const uint64_t beta_g2[16], int form, uint64_t* tau_g1_out, uint64_t* tau_g2_out, uint64_t* alpha_g1_out,
                                                      uint64_t* beta_g1_out, uint64_t beta_g2_out[16], uint64_t record_out[61], const uint64_t secrets[12], const uint64_t nonces[12],
                                                      double seconds[3]) {
  if (!ctx) return VIMZ_ERR_INVALID;
  struct Given { Fe s[3], k[3]; ~Given() { explicit_bzero(this, sizeof(*this)); } } gv;
  bool ok = secrets && nonces;
  for (int i = 0; ok && i < 3; i++) ok = pc_fr_given(secrets + 4 * i, &gv.s[i]) && pc_fr_given(nonces + 4 * i, &gv.k[i]) && !gv.s[i].is_zero();
  if (!ok) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_testing_powers_contribute_secrets: the secrets and the nonces are 4 canonical words below r each, the secrets non-zero");
  return powers_contribute_impl(ctx, "vimz_powers_contribute", tau_g1, n_tau_g1, tau_g2, alpha_g1, beta_g1, n_pow, beta_g2, form, tau_g1_out, tau_g2_out, alpha_g1_out, beta_g1_out, beta_g2_out,
                                record_out, gv.s, gv.k, seconds);
}
extern "C" int vimz_test_power_vec(vimz_ctx* ctx, const uint64_t w[4], size_t count, uint64_t* out) {
  Fe wm;
  if (!ctx || !w || !out || !count || count > (1u << 26) || !pc_fr_given(w, &wm)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_power_vec: bad argument");
  std::vector<Fe> pw(count);
  { std::lock_guard<std::mutex> g(ctx->mu);
    P_TRY(hipSetDevice(ctx->device));
    ContribDev d;
    d.s = ctx->stream; d.pw_bytes = 32 * count;
    P_TRY(hipMalloc((void**)&d.pw, d.pw_bytes));
    P_TRY(g16_power_vec(d.s, d.pw, count, wm));
    P_TRY(hipMemcpyAsync(pw.data(), d.pw, d.pw_bytes, hipMemcpyDeviceToHost, d.s));
    P_TRY(hipStreamSynchronize(d.s)); }
  for (size_t i = 0; i < count; i++) { const Fe c = Fe::from_mont(pw[i]); memcpy(out + 4 * i, c.v, 32); }
  return VIMZ_OK;
}
extern "C" int vimz_test_scale_points_by(vimz_ctx* ctx, int group, const uint64_t* points, size_t n, const uint64_t w[4], const uint64_t c[4], int form, uint64_t* out) {
  Fe wm, cm;
  if (!ctx || !points || !w || !c || !out || (group != 1 && group != 2) || (form != VIMZ_FORM_CANONICAL && form != VIMZ_FORM_MONTGOMERY) || !n || n > (1u << 26) || !pc_fr_given(w, &wm) ||
      !pc_fr_given(c, &cm))
    return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_scale_points_by: bad argument");
  if (!vz::pairing::consts().ok) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_scale_points_by: pairing constants");
  return group == 1 ? test_scale_by<G1Aff>(ctx, points, n, wm, cm, form, out) : test_scale_by<G2PowAff>(ctx, points, n, wm, cm, form, out);
}
#endif
