// Further delta contributions to a saved decider key, and the check of a chain of them (vimz_decider_key_contribute, vimz_decider_key_verify_contributions; DESIGN.md
// §8 item 5): phase 2 of a Groth16 ceremony — snarkjs's `zkey contribute` and `zkey verify` — on key BYTES (groth16.hip: vimz_decider_key_save's layout, parsed from
// its own header: a contributor needs a context, not a prover).  The host side (the blob's layout, the record and its proof of knowledge): g16_key_contrib.hpp.
//
// Contribute: delta' and a nonce from the OS; delta1, delta2 <- delta'·(delta1, delta2) on the host; the l and h queries, side by side in the blob, go to the device
// as ONE array, are multiplied in place by 1/delta' (g16_scale_points) and come back; every other byte is copied.
// Verify, stage by stage, a stage only when the ones before it found nothing:
//   points     every delta1_j, delta2_j, T_j and every point of l‖h of both keys has coordinates below q (host) and is on its curve; delta points are not the identity,
//              delta2_j is killed by r (host: g2_in_subgroup, one per record); l‖h of BOTH keys is one array on the device and k_powers_flags runs over it once — the
//              host reads the identity flag pairwise: an identity is fine where the other key has one too.
//   fixed part origin and final are the same words outside delta1, delta2, l and h.
//   equations  per record e(delta1_j, G2) = e(G1, delta2_j) and z_j·delta1_(j−1) = T_j + c_j·delta1_j; the last record's delta points are the final key's; and the
//              same-ratio check of the END points only — S = Σ rho_i·P_i over the origin's l‖h, S' = Σ rho_i·P'_i over the final's, rho_i of 128 bits from the OS, then
//              e(S', delta2_final) = e(S, delta2_origin) — so a chain of n contributions costs one pass over the arrays, not n.  The products run side by side on host threads.
// k_ratio_rlc forms S and S' in ONE launch over a grid of (chunks, 2): blockIdx.y picks the array, thread t of a row sums chunk t under the shared rho into its own
// slot (g16_point_stage.hpp: pt_ratio_chunk), and the 2·n_chunks chunk sums go through g16_column_sums with a plan of two columns.  No atomics, no flag another
// workgroup reads, every loop bound from the host.  Why one launch and not k_powers_rlc twice, and what that measured: profiles/key_contrib.txt.
#include <atomic>
#include <chrono>
#include <thread>
#include "g16_powers.hpp"
#include "g16_key_contrib.hpp"
#ifdef VIMZ_TESTING
#include "../../include/vimz_hip_testing.h"
#endif

namespace {

using namespace vz::keyc;
static_assert(VIMZ_KEYCHAIN_OFF_CURVE == PV_OFF_CURVE && VIMZ_KEYCHAIN_IDENTITY == PV_IDENTITY, "the kernel's flags are the verdict's bits");
static_assert(VIMZ_KEYCHAIN_RECORD_WORDS == RECORD_WORDS, "the record's size is part of the ABI");

// thread t of row blockIdx.y is chunk t of that row's array (pt_ratio_chunk): it writes out[row·n_chunks + t] alone
__global__ void __launch_bounds__(PT_BLOCK) k_ratio_rlc(const G1Aff* __restrict__ before, const G1Aff* __restrict__ after, size_t n, size_t n_chunks, const uint32_t* __restrict__ rho,
                                                        G1Aff* __restrict__ out) {
  const size_t t = blockIdx.x * (size_t)PT_BLOCK + threadIdx.x;
  if (t < n_chunks) pt_ratio_chunk(t, blockIdx.y, before, after, n, n_chunks, rho, out);
}

double kc_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

// n G1 points as canonical words -> Montgomery coordinates on up to 16 threads; bad[i] = 1 where a coordinate is not below q (the point is then zeros)
void g1_points_in(const uint64_t* words, size_t n, G1Aff* out, uint8_t* bad) {
  const unsigned TH = (unsigned)std::max<size_t>(1, std::min<size_t>({16, usable_cpus(), n / 4096 + 1}));
  auto work = [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) {
      bad[i] = get_g1(words + 8 * i, out + i) ? 0 : 1;
      if (bad[i]) memset((void*)(out + i), 0, sizeof(G1Aff));
    }
  };
  std::vector<std::thread> th;
  for (unsigned t = 1; t < TH; t++) th.emplace_back(work, n * t / TH, n * (t + 1) / TH);
  work(0, n / TH);
  for (auto& x : th) x.join();
}
void g1_points_out(const G1Aff* pts, size_t n, uint64_t* words) {
  const unsigned TH = (unsigned)std::max<size_t>(1, std::min<size_t>({16, usable_cpus(), n / 4096 + 1}));
  auto work = [&](size_t lo, size_t hi) { for (size_t i = lo; i < hi; i++) put_g1(words + 8 * i, pts[i]); };
  std::vector<std::thread> th;
  for (unsigned t = 1; t < TH; t++) th.emplace_back(work, n * t / TH, n * (t + 1) / TH);
  work(0, n / TH);
  for (auto& x : th) x.join();
}

// a non-zero element of Fr from the OS (rejection sampling over 254 bits), Montgomery
bool fr_nonzero_random(Fe* out) {
  for (;;) {
    Fe c;
    if (!g16_os_random(c.v, 32)) return false;
    c.v[7] &= 0x3fffffffu;
    if (c.is_reduced() && !c.is_zero()) { *out = Fe::to_mont(c); explicit_bzero(&c, sizeof(c)); return true; }
  }
}

}  // namespace

hipError_t g16_ratio_rlc(hipStream_t s, const G1Aff* before, const G1Aff* after, size_t n, const uint32_t* rho, const ColsumDevice& sum, G1Aff* chunks, G1Aff* out) {
  const size_t n_chunks = g16_powers_rlc_chunks(n);
  if (!before || !after || !rho || !chunks || !out || !n || n >= ((size_t)1 << 31) || sum.n_cols != 2 || sum.n_points != 2 * n_chunks) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ratio_rlc, dim3((unsigned)((n_chunks + PT_BLOCK - 1) / PT_BLOCK), 2), dim3(PT_BLOCK), 0, s, before, after, n, n_chunks, rho, chunks);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = g16_column_sums(s, sum, (const G1Aff*)chunks, out);
  return e;
}

namespace {

#ifdef VIMZ_TESTING
// the same two sums through two launches of k_powers_rlc (shift 0 each): what the single launch is measured against (profiles/key_contrib.txt), in the testing library alone
hipError_t ratio_rlc_two_launches(hipStream_t s, const G1Aff* before, const G1Aff* after, size_t n, const uint32_t* rho, const ColsumDevice& sum, G1Aff* chunks, G1Aff* out) {
  const size_t n_chunks = g16_powers_rlc_chunks(n);
  if (sum.n_cols != 2 || sum.n_points != 2 * n_chunks) return hipErrorInvalidValue;
  hipError_t e = g16_powers_rlc_pass(s, before, n, rho, 0, chunks);
  if (e == hipSuccess) e = g16_powers_rlc_pass(s, after, n, rho, 0, chunks + n_chunks);
  if (e == hipSuccess) e = g16_column_sums(s, sum, (const G1Aff*)chunks, out);
  return e;
}
#endif

// Two arrays of n points each, side by side on the device (`both`: before, then after; Montgomery): the per-point flags of all 2n, and — when rho is given — S and
// S'.  The caller holds the context's lock and has set the device.  launches = 1: k_ratio_rlc (the product's only form); 2, in the testing library: the two-launch form it is measured against; the
// combination is queued `reps` times, each timed from its first launch to the stream's synchronise into rep_seconds (optional).  rho (host, 4 words a point) is
// wiped on the device before it is freed.
struct RatioDev {
  G1Aff *pts = nullptr, *chunks = nullptr, *sums = nullptr; uint32_t *flags = nullptr, *rho = nullptr; size_t rho_bytes = 0; hipStream_t s = nullptr; ColsumDevice sum;
  ~RatioDev() {
    if (rho) { hipMemsetAsync(rho, 0, rho_bytes, s); hipStreamSynchronize(s); }
    for (void* p : {(void*)pts, (void*)chunks, (void*)sums, (void*)flags, (void*)rho}) if (p) hipFree(p);
    g16_colsum_free(sum);
  }
};
int ratio_upload_and_flags(vimz_ctx* ctx, RatioDev& d, const G1Aff* both, size_t n, uint32_t* flags_out) {
  d.s = ctx->stream;
  P_TRY(hipMalloc((void**)&d.pts, sizeof(G1Aff) * 2 * n)); P_TRY(hipMalloc((void**)&d.flags, 4 * 2 * n));
  P_TRY(hipMemcpyAsync(d.pts, both, sizeof(G1Aff) * 2 * n, hipMemcpyHostToDevice, d.s));
  P_TRY(g16_powers_flags(d.s, (const G1Aff*)d.pts, 2 * n, nullptr, d.flags));
  P_TRY(hipMemcpyAsync(flags_out, d.flags, 4 * 2 * n, hipMemcpyDeviceToHost, d.s));
  P_TRY(hipStreamSynchronize(d.s));
  return VIMZ_OK;
}
int ratio_combine(vimz_ctx* ctx, RatioDev& d, size_t n, const uint32_t* rho_host, int launches, int reps, G1Aff sums[2], double* rep_seconds) {
  const size_t n_chunks = g16_powers_rlc_chunks(n);
  ColsumPlan plan;
  if (!ratio_sum_plan(n_chunks, &plan)) return vz_fail(ctx, VIMZ_ERR_INVALID, "the same-ratio check: the arrays are too long");
  P_TRY(g16_colsum_upload(plan, sizeof(G1Aff), &d.sum));
  P_TRY(hipMalloc((void**)&d.chunks, sizeof(G1Aff) * 2 * n_chunks)); P_TRY(hipMalloc((void**)&d.sums, sizeof(G1Aff) * 2));
  d.rho_bytes = 16 * n;
  P_TRY(hipMalloc((void**)&d.rho, d.rho_bytes));
  P_TRY(hipMemcpyAsync(d.rho, rho_host, d.rho_bytes, hipMemcpyHostToDevice, d.s));
  P_TRY(hipStreamSynchronize(d.s));
  for (int r = 0; r < reps; r++) {
    const auto t0 = std::chrono::steady_clock::now();
#ifdef VIMZ_TESTING
    if (launches == 2) P_TRY(ratio_rlc_two_launches(d.s, d.pts, d.pts + n, n, d.rho, d.sum, d.chunks, d.sums));
    else
#endif
    P_TRY(g16_ratio_rlc(d.s, d.pts, d.pts + n, n, d.rho, d.sum, d.chunks, d.sums));
    P_TRY(hipStreamSynchronize(d.s));
    if (rep_seconds) rep_seconds[r] = kc_since(t0);
  }
  P_TRY(hipMemcpyAsync(sums, d.sums, sizeof(G1Aff) * 2, hipMemcpyDeviceToHost, d.s));
  P_TRY(hipStreamSynchronize(d.s));
  return VIMZ_OK;
}

G1Aff kc_g1_neg(G1Aff p) { if (!aff_is_identity(p)) p.y = Fq::neg(p.y); return p; }

// delta_given, nonce_given: the test hook's (Montgomery); NULL: drawn from the OS.  seconds (optional) = {host (parsing, conversions, the record), device (upload,
// scaling, download), total}
int64_t key_contribute_impl(vimz_ctx* ctx, const void* key_in, size_t len, void* key_out, size_t cap, uint64_t* record_out, const Fe* delta_given, const Fe* nonce_given, double seconds[3]) {
  auto bad = [&](const char* m) { return (int64_t)vz_fail(ctx, VIMZ_ERR_INVALID, (std::string("vimz_decider_key_contribute: ") + m).c_str()); };
  if (!ctx) return VIMZ_ERR_INVALID;
  if (!key_in || !record_out) return bad("NULL argument");
  const auto t_all = std::chrono::steady_clock::now();
  KeyLayout L;
  if (const char* why = key_layout(key_in, len, &L)) return bad(why);
  if (!key_out || cap < len) return (int64_t)len;
  const uint64_t* w = (const uint64_t*)key_in;
  G1Aff d1; G2PowAff d2;
  if (!get_g1(w + KEY_DELTA1, &d1) || !get_g2(w + KEY_DELTA2, &d2)) return bad("a coordinate is not below q");
  if (!vz::pairing::g1_on_curve(d1) || !vz::pairing::g2_on_curve(d2)) return bad("a delta point is not on its curve");
  if (aff_is_identity(d1) || aff_is_identity(d2)) return bad("a delta point is the identity");
  if (!vz::pairing::g2_in_subgroup(d2)) return bad("delta2 is outside the subgroup");
  std::vector<G1Aff> pts(L.n_lh);
  { std::vector<uint8_t> range(L.n_lh);
    g1_points_in(w + L.off_lh, L.n_lh, pts.data(), range.data());
    for (uint8_t b : range) if (b) return bad("a coordinate is not below q"); }
  // delta' and the nonce: this party's secrets, wiped on every path
  struct Secret { Fe delta, k, dinv_canon; ~Secret() { explicit_bzero(this, sizeof(*this)); } } sec;
  if (delta_given) sec.delta = *delta_given; else if (!fr_nonzero_random(&sec.delta)) return bad("no randomness from the OS");
  if (nonce_given) sec.k = *nonce_given; else if (!fr_nonzero_random(&sec.k)) return bad("no randomness from the OS");
  if (sec.delta.is_zero()) return bad("delta' is zero");
  sec.dinv_canon = Fe::from_mont(Fe::pow_pm2(sec.delta));
  uint64_t head[KEY_HEAD_WORDS], record[RECORD_WORDS];
  memcpy(head, w, sizeof(head));
  make_record(head, &d1, &d2, sec.delta, sec.k, record);
  const auto t_dev = std::chrono::steady_clock::now();
  if (L.n_lh) {
    std::lock_guard<std::mutex> g(ctx->mu);
    P_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    struct Dev { G1Aff* pts = nullptr; uint32_t* dinv = nullptr;
                 ~Dev() { if (dinv) { hipMemset(dinv, 0, 32); hipFree(dinv); }      // (an error path between 1/delta's upload and its wipe ends here)
                          if (pts) hipFree(pts); } } D;
    P_TRY(hipMalloc((void**)&D.pts, sizeof(G1Aff) * L.n_lh)); P_TRY(hipMalloc((void**)&D.dinv, 32));
    P_TRY(hipMemcpyAsync(D.pts, pts.data(), sizeof(G1Aff) * L.n_lh, hipMemcpyHostToDevice, s));
    P_TRY(hipMemcpyAsync(D.dinv, sec.dinv_canon.v, 32, hipMemcpyHostToDevice, s));
    P_TRY(g16_scale_points(s, (const G1Aff*)D.pts, L.n_lh, D.dinv, D.pts));
    P_TRY(hipMemsetAsync(D.dinv, 0, 32, s));
    P_TRY(hipMemcpyAsync(pts.data(), D.pts, sizeof(G1Aff) * L.n_lh, hipMemcpyDeviceToHost, s));
    P_TRY(hipStreamSynchronize(s));
  }
  const double t_device = kc_since(t_dev);
  // nothing was written so far: key_out may be key_in
  uint64_t* o = (uint64_t*)key_out;
  if (key_out != key_in) memmove(key_out, key_in, len);
  put_g1(o + KEY_DELTA1, d1); put_g2(o + KEY_DELTA2, d2);
  g1_points_out(pts.data(), L.n_lh, o + L.off_lh);
  memcpy(record_out, record, sizeof(record));
    if (seconds) { seconds[2] = kc_since(t_all); seconds[1] = t_device; seconds[0] = seconds[2] - t_device; }
  return (int64_t)len;
}

// what is wrong with a G1 / G2 point given as canonical words (VIMZ_KEYCHAIN_* bits; 0: nothing); may_be_identity: T of a record
uint32_t g1_point_bits(const uint64_t* words, bool may_be_identity, G1Aff* p) {
  if (!get_g1(words, p)) return VIMZ_KEYCHAIN_COORD;
  if (aff_is_identity(*p)) return may_be_identity ? 0u : (uint32_t)VIMZ_KEYCHAIN_IDENTITY;
  return vz::pairing::g1_on_curve(*p) ? 0u : (uint32_t)VIMZ_KEYCHAIN_OFF_CURVE;
}
uint32_t g2_point_bits(const uint64_t* words, G2PowAff* p) {
  if (!get_g2(words, p)) return VIMZ_KEYCHAIN_COORD;
  if (aff_is_identity(*p)) return VIMZ_KEYCHAIN_IDENTITY;
  if (!vz::pairing::g2_on_curve(*p)) return VIMZ_KEYCHAIN_OFF_CURVE;
  return vz::pairing::g2_in_subgroup(*p) ? 0u : (uint32_t)VIMZ_KEYCHAIN_SUBGROUP;
}

}  // namespace

extern "C" int64_t vimz_decider_key_contribute(vimz_ctx* ctx, const void* key_in, size_t len, void* key_out, size_t cap, uint64_t record_out[37], double seconds[3]) {
  return key_contribute_impl(ctx, key_in, len, key_out, cap, record_out, nullptr, nullptr, seconds);
}

extern "C" int vimz_decider_key_verify_contributions(vimz_ctx* ctx, const void* origin, size_t origin_len, const void* final_key, size_t final_len, const uint64_t* records, size_t n_records,
                                                     uint32_t* result, uint64_t first_bad[2], double seconds[4]) {
  auto bad = [&](const std::string& m) { return vz_fail(ctx, VIMZ_ERR_INVALID, ("vimz_decider_key_verify_contributions: " + m).c_str()); };
  if (!ctx) return VIMZ_ERR_INVALID;
  if (!origin || !final_key || !result || !first_bad || (n_records && !records)) return bad("NULL argument");
  if (!vz::pairing::consts().ok) return bad("pairing constants");
  KeyLayout Lo, Lf;
  if (const char* why = key_layout(origin, origin_len, &Lo)) return bad(std::string("the origin key: ") + why);
  if (const char* why = key_layout(final_key, final_len, &Lf)) return bad(std::string("the final key: ") + why);
  for (size_t j = 0; j < n_records; j++) if (records[RECORD_WORDS * j] != RECORD_MAGIC) return bad("record " + std::to_string(j) + " is not a contribution record");
  const uint64_t *wo = (const uint64_t*)origin, *wf = (const uint64_t*)final_key;
  double sec[4] = {0, 0, 0, 0};
  *result = 0; first_bad[0] = first_bad[1] = 0;
  auto verdict = [&](uint32_t bits, uint64_t what, uint64_t where) {
    *result = bits; first_bad[0] = what; first_bad[1] = where;
    if (seconds) memcpy(seconds, sec, sizeof(sec));
    return VIMZ_OK;
  };
  // keys of other sizes have nothing to compare point by point: that is a difference of the fixed part, at the first header word that differs
  if (Lo.words != Lf.words || memcmp(wo, wf, 8 * 7)) {
    size_t k = 0;
    while (k < 7 && wo[k] == wf[k]) k++;
    return verdict(VIMZ_KEYCHAIN_FIXED_PART, VIMZ_KEYCHAIN_AT_FIXED_PART, k);
  }
  const size_t n = Lo.n_lh;
  // ---- the points ----
  auto t0 = std::chrono::steady_clock::now();
  struct Rec { G1Aff d1, T; G2PowAff d2; };
  G1Aff d1o, d1f; G2PowAff d2o, d2f;
  std::vector<Rec> recs(n_records);
  { const struct { const uint64_t* w; G1Aff* d1; G2PowAff* d2; uint64_t what; } keys[2] = {{wo, &d1o, &d2o, VIMZ_KEYCHAIN_AT_ORIGIN_DELTA}, {wf, &d1f, &d2f, VIMZ_KEYCHAIN_AT_FINAL_DELTA}};
    for (const auto& k : keys) {
      const uint32_t b1 = g1_point_bits(k.w + KEY_DELTA1, false, k.d1), b2 = g2_point_bits(k.w + KEY_DELTA2, k.d2);
      if (b1 | b2) return verdict(b1 | b2, k.what, b1 ? 0 : 1);
    }
    // (delta2_j's membership is 254 doublings over Fq2 a record: side by side on the host's threads)
    std::vector<uint32_t> rbits(n_records, 0);
    std::atomic<size_t> next{0};
    auto work = [&] {
      for (size_t j; (j = next.fetch_add(1)) < n_records;) {
        const uint64_t* r = records + RECORD_WORDS * j;
        rbits[j] = g1_point_bits(r + REC_DELTA1, false, &recs[j].d1) | g2_point_bits(r + REC_DELTA2, &recs[j].d2) | g1_point_bits(r + REC_T, true, &recs[j].T);
      }
    };
    std::vector<std::thread> th;
    for (size_t t = 1; t < std::min<size_t>({16, usable_cpus(), n_records}); t++) th.emplace_back(work);
    work();
    for (auto& x : th) x.join();
    for (size_t j = 0; j < n_records; j++) if (rbits[j]) return verdict(rbits[j], VIMZ_KEYCHAIN_AT_RECORD, j); }
  std::vector<G1Aff> both(2 * n);
  std::vector<uint8_t> range(2 * n);
  g1_points_in(wo + Lo.off_lh, n, both.data(), range.data());
  g1_points_in(wf + Lf.off_lh, n, both.data() + n, range.data() + n);
  sec[0] = kc_since(t0);
  std::unique_lock<std::mutex> lock(ctx->mu, std::defer_lock);      // (declared before what it guards: the device buffers go while it is still held)
  std::unique_ptr<RatioDev> dev(new RatioDev());
  if (n) {
    t0 = std::chrono::steady_clock::now();
    lock.lock();
    P_TRY(hipSetDevice(ctx->device));
    std::vector<uint32_t> flags(2 * n);
    { const int rc = ratio_upload_and_flags(ctx, *dev, both.data(), n, flags.data()); if (rc) return rc; }
    // origin's findings first, then the final's; an identity is one only where the other key's point is none
    for (int side = 0; side < 2; side++) {
      uint32_t bits = 0; size_t first = 0;
      for (size_t i = n; i-- > 0;) {
        const size_t me = side * n + i, other = (1 - side) * n + i;
        uint32_t f = range[me] ? (uint32_t)VIMZ_KEYCHAIN_COORD : flags[me];
        if (f == VIMZ_KEYCHAIN_IDENTITY && (range[other] || flags[other] == VIMZ_KEYCHAIN_IDENTITY)) f = 0;
        if (f) { bits |= f; first = i; }
      }
      if (bits) { sec[1] = kc_since(t0); return verdict(bits, side ? VIMZ_KEYCHAIN_AT_FINAL_LH : VIMZ_KEYCHAIN_AT_ORIGIN_LH, first); }
    }
    sec[1] = kc_since(t0);
  }
  // ---- the fixed part ----
  { const size_t cut[4][2] = {{KEY_DELTA1, KEY_DELTA1 + 8}, {KEY_DELTA2, KEY_DELTA2 + 16}, {Lo.off_lh, Lo.off_lh + 8 * n}, {Lo.words, Lo.words}};
    size_t k = 0;
    for (const auto& c : cut) {
      for (; k < c[0]; k++) if (wo[k] != wf[k]) return verdict(VIMZ_KEYCHAIN_FIXED_PART, VIMZ_KEYCHAIN_AT_FIXED_PART, k);
      k = c[1];
    } }
  // ---- the equations ----
  G1Aff sums[2]; memset((void*)sums, 0, sizeof(sums));
  if (n) {
    t0 = std::chrono::steady_clock::now();
    struct Rho { std::vector<uint32_t> w; ~Rho() { if (!w.empty()) explicit_bzero(w.data(), 4 * w.size()); } } rho;
    rho.w.resize(4 * n);
    if (!g16_os_random(rho.w.data(), 4 * rho.w.size())) return bad("no randomness from the OS");
    { const int rc = ratio_combine(ctx, *dev, n, rho.w.data(), 1, 1, sums, nullptr); if (rc) return rc; }
    dev.reset();
    lock.unlock();
    sec[2] = kc_since(t0);
  }
  t0 = std::chrono::steady_clock::now();
  const G1Aff g1 = g16_g1_generator(); const G2PowAff g2 = g16_g2_generator();
  std::vector<uint8_t> halves(n_records, 0), knows(n_records, 0);
  bool ratio = false;
  { std::atomic<size_t> next{0};
    const size_t jobs = 2 * n_records + 1;
    auto work = [&] {
      for (size_t job; (job = next.fetch_add(1)) < jobs;) {
        const size_t j = job / 2;
        if (job == 2 * n_records) ratio = vz::pairing::product_is_one({{sums[1], d2f}, {kc_g1_neg(sums[0]), d2o}});
        else if (job & 1) halves[j] = vz::pairing::product_is_one({{recs[j].d1, g2}, {kc_g1_neg(g1), recs[j].d2}});
        else knows[j] = record_knowledge(wo, j ? records + RECORD_WORDS * (j - 1) + REC_DELTA1 : wo + KEY_DELTA1, j ? recs[j - 1].d1 : d1o, recs[j].d1, recs[j].T, records + RECORD_WORDS * j);
      }
    };
    std::vector<std::thread> th;
    for (size_t t = 1; t < std::min<size_t>({16, usable_cpus(), jobs}); t++) th.emplace_back(work);
    work();
    for (auto& x : th) x.join(); }
  uint32_t bits = 0; uint64_t what = 0, where = 0;
  for (size_t j = n_records; j-- > 0;) {
    if (!halves[j]) bits |= VIMZ_KEYCHAIN_DELTA_HALVES;
    if (!knows[j]) bits |= VIMZ_KEYCHAIN_KNOWLEDGE;
    if (!halves[j] || !knows[j]) { what = VIMZ_KEYCHAIN_AT_RECORD; where = j; }
  }
  const uint64_t* last = n_records ? records + RECORD_WORDS * (n_records - 1) : nullptr;
  if (memcmp(last ? last + REC_DELTA1 : wo + KEY_DELTA1, wf + KEY_DELTA1, 64) || memcmp(last ? last + REC_DELTA2 : wo + KEY_DELTA2, wf + KEY_DELTA2, 128)) bits |= VIMZ_KEYCHAIN_LAST;
  if (!ratio) bits |= VIMZ_KEYCHAIN_RATIO;
  sec[3] = kc_since(t0);
  return verdict(bits, what, where);
}

#ifdef VIMZ_TESTING
namespace {
bool fr_given(const uint64_t w[4], Fe* out) { Fe c; memcpy(c.v, w, 32); if (!c.is_reduced()) return false; *out = Fe::to_mont(c); explicit_bzero(&c, sizeof(c)); return true; }

int test_ratio(vimz_ctx* ctx, const char* who, const uint64_t* before, const uint64_t* after, size_t n, const uint64_t* rho, int form, int launches, int reps, uint64_t* out, double* rep_seconds) {
  if (!ctx || !before || !after || !rho || !out || (form != VIMZ_FORM_CANONICAL && form != VIMZ_FORM_MONTGOMERY) || !n || n > (1u << 26) || (launches != 1 && launches != 2) || reps < 1)
    return vz_fail(ctx, VIMZ_ERR_INVALID, (std::string(who) + ": bad argument").c_str());
  std::vector<G1Aff> both(2 * n);
  for (size_t i = 0; i < 2 * n; i++) {
    const uint64_t* w = (i < n ? before : after - 8 * n) + 8 * i;
    Fq* c = (Fq*)&both[i];
    for (int k = 0; k < 2; k++) {
      Fq x; memcpy(x.v, w + 4 * k, 32);
      if (!x.is_reduced()) return vz_fail(ctx, VIMZ_ERR_INVALID, (std::string(who) + ": a coordinate is not below q").c_str());
      c[k] = form == VIMZ_FORM_MONTGOMERY ? x : Fq::to_mont(x);
    }
  }
  G1Aff sums[2];
  { std::lock_guard<std::mutex> g(ctx->mu);
    P_TRY(hipSetDevice(ctx->device));
    RatioDev dev;
    std::vector<uint32_t> flags(2 * n);
    int rc = ratio_upload_and_flags(ctx, dev, both.data(), n, flags.data());
    if (rc) return rc;
    for (uint32_t f : flags) if (f & VIMZ_KEYCHAIN_OFF_CURVE) return vz_fail(ctx, VIMZ_ERR_INVALID, (std::string(who) + ": a point is not on the curve").c_str());
    if ((rc = ratio_combine(ctx, dev, n, (const uint32_t*)rho, launches, reps, sums, rep_seconds))) return rc; }
  const Fq* c = (const Fq*)sums;
  for (size_t k = 0; k < 4; k++) { const Fq x = form == VIMZ_FORM_MONTGOMERY ? c[k] : Fq::from_mont(c[k]); memcpy(out + 4 * k, x.v, 32); }
  return VIMZ_OK;
}
}  // namespace

extern "C" int64_t vimz_testing_decider_key_contribute_delta(vimz_ctx* ctx, const void* key_in, size_t len, void* key_out, size_t cap, uint64_t record_out[37], const uint64_t delta[4],
                                                             const uint64_t nonce[4], double seconds[3]) {
  if (!ctx) return VIMZ_ERR_INVALID;
  struct Given { Fe delta, k; ~Given() { explicit_bzero(this, sizeof(*this)); } } gv;
  if (!delta || !nonce || !fr_given(delta, &gv.delta) || !fr_given(nonce, &gv.k) || gv.delta.is_zero())
    return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_testing_decider_key_contribute_delta: delta' and the nonce are 4 canonical words below r, delta' non-zero");
  return key_contribute_impl(ctx, key_in, len, key_out, cap, record_out, &gv.delta, &gv.k, seconds);
}
extern "C" int vimz_test_ratio_rlc(vimz_ctx* ctx, const uint64_t* before, const uint64_t* after, size_t n, const uint64_t* rho, int form, uint64_t* out) {
  return test_ratio(ctx, "vimz_test_ratio_rlc", before, after, n, rho, form, 1, 1, out, nullptr);
}
extern "C" int vimz_test_ratio_rlc_forms(vimz_ctx* ctx, const uint64_t* before, const uint64_t* after, size_t n, const uint64_t* rho, int form, int launches, int reps, uint64_t* out,
                                         double* rep_seconds) {
  return test_ratio(ctx, "vimz_test_ratio_rlc_forms", before, after, n, rho, form, launches, reps, out, rep_seconds);
}
#endif
