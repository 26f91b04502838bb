// Judging a decider key that someone else hands over (vimz_decider_key_verify_origin): is it the key vimz_decider_setup_from_powers derives from
// THIS powers-of-tau string for THIS circuit, for the delta its delta points commit to — what snarkjs's `zkey verify` checks against an r1cs and a ptau.  The
// recipient does not know delta (it is the toxic waste) and derives nothing again: every query is LINEAR in the string's Lagrange basis, so a random combination of a
// query equals a sparse product of the circuit's matrices with the random vector, one inverse NTT over Fr and one MSM over the string's own powers.
//
//   m wires, n_pub public inputs (wire 0 the constant), n_c constraints, domain n = 2^logn; P = wires 0..n_pub, Q = the rest; rho in (128 bits)^m and rho' in
//   (128 bits)^(n−1) from the OS; for X in {A, B, C}, S in {P, Q}:  u_X^S = X·rho^S padded to n (plus the unit rows u_A^P[n_c + i] += rho_i, i <= n_pub),
//   c_X^S = iNTT(u_X^S) with its 1/n, c_X = c_X^P + c_X^Q,  K(S) = MSM(beta_g1, c_A^S) + MSM(alpha_g1, c_B^S) + MSM(tau_g1, c_C^S) over the first n powers.
//     a   Σ rho_i·a_i  = MSM(tau_g1, c_A)           b1  Σ rho_i·b1_i = MSM(tau_g1, c_B)           b2  Σ rho_i·b2_i = MSM_G2(tau_g2, c_B)
//     ic  Σ_P rho_i·ic_i = K(P)   (gamma = 1)        l   e(Σ_Q rho_i·l_i, delta2) = e(K(Q), G2)
//     h   e(Σ rho'_j·h_j, delta2) = e(MSM(tau_g1[:2n−1], s), G2),  s_k = −rho'_k (k < n − 1) + rho'_(k−n) (k >= n)
//   and delta1, delta2 on their curves, not the identity, delta2 killed by r, e(delta1, G2) = e(G1, delta2).  A wrong query point passes an equation with probability
//   at most 2^-128.  tests/_key_origin_ref.py states all of it on plain integers.
//
// Stages, each only when the ones before it found nothing:
//   (i)   the blob's layout (g16_key_contrib.hpp: key_layout — every size against the length before anything is indexed), its header against the circuit, the fixed
//         words against the string: alpha1 = alpha_g1[0], beta1 = beta_g1[0], beta2 = beta_g2, gamma2 = G2, the KZG point = tau_g2[1].  Host.
//   (ii)  the delta conditions (host), then array by array ic, a, b1, l, h, b2: coordinates below q (host), on the curve and — b2 — killed by r POINT BY POINT
//         (g16_powers_flags; the identity is allowed: vimz_decider_key_save writes zeros for the columns nobody touches).  While a clean array is still on the device
//         its combination is formed: ONE array of the key sits there at a time, and none is uploaded twice.
//   (iii) the circuit side — k_origin_vec expands rho masked to P, then to Q; k_spmv3_dict forms the three products of each; the six inverse NTTs; five MSMs through
//         vz_msm_device over ONE resident array beta_g1[:n] ‖ alpha_g1[:n] ‖ tau_g1[:2n−1] (K(S) is a single MSM of 3n points) and the bit-plane MSM over tau_g2 —
//         then the comparisons and three products of pairings on host threads, all evaluated.
// The key side is the 128-bit chunked combination of the string's and the chains' checks (g16_point_stage.hpp: pt_rlc_chunk, eight points a thread, reduced by
// g16_column_sums over rlc_sum_plan's one column) in a launch of its own, k_origin_rlc: g16_powers_rlc and g16_ratio_rlc form TWO sums a call, and here every array
// has one.
//
// k_spmv3_dict: blockIdx.y is the matrix, a THREAD owns a row from its first term to its store; rows n_c..n−1 are written as zero by the same launch.  No atomics, no
// flag another workgroup reads, the trip count is the host's row_ptr, whose offsets, wire numbers and coefficient indices the host has checked (csr_is_sound).  One
// path, not a short/long split with a wave per long row: the decider's long rows (bit sums, Horner rows) are a few thousand among millions, the product is launched
// twice a call, and the whole of it is well under a hundredth of the call (profiles/key_origin.txt: the histogram and the time) — a second path would buy nothing
// that could be measured and would add a host plan and a threshold to test.
//
// Peak device memory (stage iii; n the domain, m the wires, z the non-zeros): the string's 4n − 1 points of G1 twice while they are converted (64 B and the MSM's form),
// tau_g2 (128 n), the vectors (32·(m + 10 n)), the matrices (8 z + 12 n_c) and the dictionary, rho and rho' (16·(m + n)), the MSM's workspace for 3n points and the G2 MSM's
// 133 MB of plane partials.  Stage (ii) adds one array of the key (at most 128 m), its flags and its chunk sums.
#include <atomic>
#include <chrono>
#include <thread>
#include "g16_key_origin.hpp"
#ifdef VIMZ_TESTING
#include "../../include/vimz_hip_testing.h"
#endif

namespace {

using namespace vz::keyc;
static_assert(VIMZ_KEYORIGIN_OFF_CURVE == PV_OFF_CURVE && VIMZ_KEYORIGIN_SUBGROUP == PV_SUBGROUP, "the kernel's flags are the verdict's bits");

struct SpmvArgs { const uint32_t *row_ptr[3], *col[3], *coef[3], *dict; uint32_t* out[3]; uint32_t n_c; };

// thread i of row blockIdx.y is row i of that matrix (g16_key_origin_stage.hpp: spmv_dict_row): it writes out[matrix][i] alone
__global__ void __launch_bounds__(KO_BLOCK) k_spmv3_dict(SpmvArgs a, const uint32_t* __restrict__ v, size_t n) {
  const size_t row = blockIdx.x * (size_t)KO_BLOCK + threadIdx.x;
  const unsigned q = blockIdx.y;
  if (row < n) spmv_dict_row(row, a.n_c, a.row_ptr[q], a.col[q], a.coef[q], a.dict, v, a.out[q]);
}
// the elementwise steps around it, thread i element i (ko_expand, ko_unit, ko_h_scalar, ko_add): mode = KO_*; p0, p1 the mode's two sizes
__global__ void __launch_bounds__(KO_BLOCK) k_origin_vec(uint32_t mode, size_t count, size_t p0, size_t p1, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, KoFr k,
                                                         uint32_t* out) {
  const size_t i = blockIdx.x * (size_t)KO_BLOCK + threadIdx.x;
  if (i >= count) return;
  if (mode == KO_EXPAND) ko_expand(i, p0, p1, a, k, out);
  else if (mode == KO_UNITS) ko_unit(i, (uint32_t)p0, a, out);
  else if (mode == KO_H_SCALARS) ko_h_scalar(i, p0, a, k, out);
  else ko_add(i, a, b, out);
}
// thread t is chunk t of ONE combination Σ rho_i·P_i (pt_rlc_chunk with shift 0): it writes out[t] alone
template <class F>
__global__ void __launch_bounds__(PT_BLOCK) k_origin_rlc(const Affine<F>* __restrict__ points, size_t n, size_t n_chunks, const uint32_t* __restrict__ rho, Affine<F>* __restrict__ out) {
  const size_t t = blockIdx.x * (size_t)PT_BLOCK + threadIdx.x;
  if (t < n_chunks) pt_rlc_chunk(t, points, n, rho, 0u, out);
}

unsigned ko_blocks(size_t threads) { return (unsigned)((threads + KO_BLOCK - 1) / KO_BLOCK); }
double ko_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

hipError_t origin_vec(hipStream_t s, uint32_t mode, size_t count, size_t p0, size_t p1, const uint32_t* a, const uint32_t* b, const KoFr& k, uint32_t* out) {
  if (!count) return hipSuccess;
  hipLaunchKernelGGL(k_origin_vec, dim3(ko_blocks(count)), dim3(KO_BLOCK), 0, s, mode, count, p0, p1, a, b, k, out);
  return hipGetLastError();
}

// every offset, wire number and coefficient index a kernel will follow, before it is uploaded
bool csr_is_sound(const G16CircuitView& c, std::string* why) {
  static const char* names[3] = {"A", "B", "C"};
  for (int q = 0; q < 3; q++) {
    auto bad = [&](const char* m) { if (why) *why = std::string("matrix ") + names[q] + ": " + m; return false; };
    if (!c.row_ptr[q] || c.n_row_ptr[q] != (size_t)c.n_c + 1) return bad("not one row a constraint");
    if (c.nnz[q] >= ((size_t)1 << 32) || (c.nnz[q] && (!c.col[q] || !c.coef[q]))) return bad("its entries");
    if (c.row_ptr[q][0] != 0 || c.row_ptr[q][c.n_c] != c.nnz[q]) return bad("its offsets do not span its entries");
    for (uint32_t r = 0; r < c.n_c; r++) if (c.row_ptr[q][r] > c.row_ptr[q][r + 1]) return bad("its offsets decrease");
    for (size_t k = 0; k < c.nnz[q]; k++) if (c.col[q][k] >= c.m || c.coef[q][k] >= c.n_dict) return bad("a wire number or a coefficient index is out of bounds");
  }
  if (!c.dict && c.n_dict) { if (why) *why = "no dictionary"; return false; }
  return true;
}

}  // namespace

hipError_t g16_spmv_upload(const G16CircuitView& c, SpmvDevice* dev, std::string* why) {
  if (!csr_is_sound(c, why)) return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  auto up = [&](uint32_t** dst, const uint32_t* src, size_t words) {
    if (e != hipSuccess) return;
    e = hipMalloc((void**)dst, 4 * std::max<size_t>(words, 1));
    if (e == hipSuccess && words) e = hipMemcpy(*dst, src, 4 * words, hipMemcpyHostToDevice);
  };
  for (int q = 0; q < 3; q++) { up(&dev->row_ptr[q], c.row_ptr[q], (size_t)c.n_c + 1); up(&dev->col[q], c.col[q], c.nnz[q]); up(&dev->coef[q], c.coef[q], c.nnz[q]); }
  up(&dev->dict, c.dict, 8 * c.n_dict);
  dev->m = c.m; dev->n_c = c.n_c;
  if (e != hipSuccess) { g16_spmv_free(*dev); if (why) *why = "the upload of the matrices"; }
  return e;
}
void g16_spmv_free(SpmvDevice& dev) {
  for (int q = 0; q < 3; q++) for (uint32_t** p : {&dev.row_ptr[q], &dev.col[q], &dev.coef[q]}) { if (*p) hipFree(*p); *p = nullptr; }
  if (dev.dict) hipFree(dev.dict); dev.dict = nullptr;
}
hipError_t g16_spmv3_dict(hipStream_t s, const SpmvDevice& dev, const uint32_t* v, size_t n, uint32_t* out_a, uint32_t* out_b, uint32_t* out_c) {
  if (!v || !out_a || !out_b || !out_c || !dev.dict || n < dev.n_c || !n || n > ((size_t)1 << 31)) return hipErrorInvalidValue;
  SpmvArgs a;
  for (int q = 0; q < 3; q++) { a.row_ptr[q] = dev.row_ptr[q]; a.col[q] = dev.col[q]; a.coef[q] = dev.coef[q]; }
  a.dict = dev.dict; a.out[0] = out_a; a.out[1] = out_b; a.out[2] = out_c; a.n_c = dev.n_c;
  hipLaunchKernelGGL(k_spmv3_dict, dim3(ko_blocks(n), 3), dim3(KO_BLOCK), 0, s, a, v, n);
  return hipGetLastError();
}

namespace {

G1Aff ko_g1_neg(G1Aff p) { if (!aff_is_identity(p)) p.y = Fq::neg(p.y); return p; }
bool same_g1(const G1Aff& p, const G1Aff& q) { return Fq::from_mont(p.x).eq(Fq::from_mont(q.x)) && Fq::from_mont(p.y).eq(Fq::from_mont(q.y)); }
bool same_g2(const G2PowAff& p, const G2PowAff& q) {
  const Fq* a = (const Fq*)&p; const Fq* b = (const Fq*)&q;
  for (int k = 0; k < 4; k++) if (!Fq::from_mont(a[k]).eq(Fq::from_mont(b[k]))) return false;
  return true;
}
Fq2 origin_curve_b(const G2PowAff*) { return vz::pairing::consts().twist_b; }
Fq origin_curve_b(const G1Aff*) { return vz::pairing::fq_u64(3); }

// n points of the key as canonical words -> Montgomery coordinates on up to 16 threads; bad[i] = 1 where a coordinate is not below q (the point is then zeros)
template <class A>
void key_points_in(const uint64_t* words, size_t n, A* out, uint8_t* bad) {
  const size_t per = sizeof(A) / sizeof(Fq);
  const unsigned TH = (unsigned)std::max<size_t>(1, std::min<size_t>({16, usable_cpus(), n / 4096 + 1}));
  auto work = [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) {
      Fq* c = (Fq*)(out + i);
      bool ok = true;
      for (size_t k = 0; k < per; k++) ok = get_fq(words + 4 * (per * i + k), c + k) && ok;
      bad[i] = ok ? 0 : 1;
      if (!ok) memset((void*)c, 0, sizeof(A));
    }
  };
  std::vector<std::thread> th;
  for (unsigned t = 1; t < TH; t++) th.emplace_back(work, n * t / TH, n * (t + 1) / TH);
  work(0, n / TH);
  for (auto& x : th) x.join();
}

// what judging one array of the key leaves
template <class A>
struct KeyArray { uint32_t bits = 0; size_t first = 0; A sum; };

// One array of the key on the context's stream (the caller holds the lock and has set the device): coordinates, per-point flags (the identity allowed), and — when
// clean and rho is given — its combination Σ rho_i·P_i, Montgomery.  d_order: r's 8 words on the device; d_rho: 4 words a point.  sec: {conversion, flags, combination}
// are added to.
template <class A>
int judge_key_array(vimz_ctx* ctx, const uint64_t* words, size_t n, const uint32_t* d_order, const uint32_t* d_rho, KeyArray<A>* out, double sec[3]) {
  hipStream_t s = ctx->stream;
  memset((void*)&out->sum, 0, sizeof(A));
  out->bits = 0; out->first = 0;
  if (!n) return VIMZ_OK;
  auto t0 = std::chrono::steady_clock::now();
  std::vector<A> pts(n);
  std::vector<uint8_t> range(n);
  key_points_in<A>(words, n, pts.data(), range.data());
  sec[0] += ko_since(t0);
  t0 = std::chrono::steady_clock::now();
  struct Dev { A *pts = nullptr, *chunks = nullptr, *sum = nullptr; uint32_t* flags = nullptr; ColsumDevice plan;
               ~Dev() { for (void* p : {(void*)pts, (void*)chunks, (void*)sum, (void*)flags}) if (p) hipFree(p); g16_colsum_free(plan); } } d;
  P_TRY(hipMalloc((void**)&d.pts, sizeof(A) * n)); P_TRY(hipMalloc((void**)&d.flags, 4 * n));
  P_TRY(hipMemcpyAsync(d.pts, pts.data(), sizeof(A) * n, hipMemcpyHostToDevice, s));
  P_TRY(g16_powers_flags(s, (const A*)d.pts, n, d_order, d.flags));
  std::vector<uint32_t> flags(n);
  P_TRY(hipMemcpyAsync(flags.data(), d.flags, 4 * n, hipMemcpyDeviceToHost, s));
  P_TRY(hipStreamSynchronize(s));
  for (size_t i = n; i-- > 0;) {
    const uint32_t f = range[i] ? (uint32_t)VIMZ_KEYORIGIN_COORD : flags[i] & ~(uint32_t)PV_IDENTITY;
    if (f) { out->bits |= f; out->first = i; }
  }
  sec[1] += ko_since(t0);
  if (out->bits || !d_rho) return VIMZ_OK;
  t0 = std::chrono::steady_clock::now();
  const size_t n_chunks = g16_powers_rlc_chunks(n);
  ColsumPlan plan;
  if (!rlc_sum_plan(n_chunks, &plan)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_decider_key_verify_origin: an array is too long");
  P_TRY(g16_colsum_upload(plan, sizeof(A), &d.plan));
  P_TRY(hipMalloc((void**)&d.chunks, sizeof(A) * n_chunks)); P_TRY(hipMalloc((void**)&d.sum, sizeof(A)));
  typedef typename std::remove_reference<decltype(pts[0].x)>::type F;
  hipLaunchKernelGGL(k_origin_rlc<F>, dim3((unsigned)((n_chunks + PT_BLOCK - 1) / PT_BLOCK)), dim3(PT_BLOCK), 0, s, (const A*)d.pts, n, n_chunks, d_rho, d.chunks);
  P_TRY(hipGetLastError());
  P_TRY(g16_column_sums(s, d.plan, (const A*)d.chunks, d.sum));
  P_TRY(hipMemcpyAsync(&out->sum, d.sum, sizeof(A), hipMemcpyDeviceToHost, s));
  P_TRY(hipStreamSynchronize(s));
  sec[2] += ko_since(t0);
  return VIMZ_OK;
}

// r's words, rho and rho' on the device; the scalars are wiped on both sides when this goes
struct OriginScalars {
  std::vector<uint32_t> rho; uint32_t *d_order = nullptr, *d_rho = nullptr; hipStream_t s = nullptr;
  ~OriginScalars() {
    if (!rho.empty()) explicit_bzero(rho.data(), 4 * rho.size());
    if (d_rho) { hipMemsetAsync(d_rho, 0, 4 * rho.size(), s); hipStreamSynchronize(s); hipFree(d_rho); }
    if (d_order) hipFree(d_order);
  }
  hipError_t upload(hipStream_t stream) {
    s = stream;
    hipError_t e = hipMalloc((void**)&d_order, 32);
    if (e == hipSuccess) e = hipMemcpyAsync(d_order, BnFr::MOD.w, 32, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMalloc((void**)&d_rho, 4 * rho.size());
    if (e == hipSuccess) e = hipMemcpyAsync(d_rho, rho.data(), 4 * rho.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e;
  }
};

struct StringSide { G1Aff a, b1, kp, kq, h; G2PowAff b2; };
// the string as the equations read it: beta_g1[:n] ‖ alpha_g1[:n] ‖ tau_g1[:2n−1], and tau_g2[:n] (Montgomery, on their curves)
struct StringPoints { std::vector<G1Aff> g1; std::vector<G2PowAff> tau2; G2PowAff beta2; };

// Stage (iii)'s circuit side, on the context's stream under its lock.  d_rho: rho (4 m words), then rho' (4 (n − 1) words).  stats: the product's time on stderr.
int string_side(vimz_ctx* ctx, const G16CircuitView& cv, const StringPoints& S, const uint32_t* d_rho, bool stats, StringSide* out) {
  hipStream_t s = ctx->stream;
  const size_t n = (size_t)1 << cv.logn, m = cv.m;
  struct Dev {
    SpmvDevice mats; G16Domain* dom = nullptr; vimz_bases* bases = nullptr; G1Aff* raw = nullptr; G2PowAff* tau2 = nullptr; uint32_t *v = nullptr, *u = nullptr, *ab = nullptr, *hs = nullptr, *idx = nullptr;
    hipStream_t s = nullptr; size_t v_bytes = 0, u_bytes = 0, ab_bytes = 0, hs_bytes = 0;
    ~Dev() {      // (the vectors are rho's images: wiped before they are freed)
      const struct { uint32_t* p; size_t bytes; } secret[4] = {{v, v_bytes}, {u, u_bytes}, {ab, ab_bytes}, {hs, hs_bytes}};
      for (const auto& x : secret) if (x.p) hipMemsetAsync(x.p, 0, x.bytes, s);
      if (s) hipStreamSynchronize(s);
      g16_spmv_free(mats); g16_domain_free(dom); g16_bases_free_raw(bases);
      for (void* p : {(void*)raw, (void*)tau2, (void*)v, (void*)u, (void*)ab, (void*)hs, (void*)idx}) if (p) hipFree(p);
    }
  } D;
  D.s = s;
  { std::string why;
    const hipError_t e = g16_spmv_upload(cv, &D.mats, &why);
    if (e == hipErrorInvalidValue) return vz_fail(ctx, VIMZ_ERR_INVALID, ("vimz_decider_key_verify_origin: " + why).c_str());
    P_TRY(e); }
  { const int rc = g16_domain_new(ctx, s, cv.logn, &D.dom); if (rc) return rc; }
  P_TRY(hipMalloc((void**)&D.raw, sizeof(G1Aff) * S.g1.size()));
  P_TRY(hipMemcpy(D.raw, S.g1.data(), sizeof(G1Aff) * S.g1.size(), hipMemcpyHostToDevice));
  { const int rc = g16_bases_from_device(ctx, D.raw, S.g1.size(), &D.bases); if (rc) return rc; }
  hipFree(D.raw); D.raw = nullptr;
  P_TRY(hipMalloc((void**)&D.tau2, sizeof(G2PowAff) * n));
  P_TRY(hipMemcpy(D.tau2, S.tau2.data(), sizeof(G2PowAff) * n, hipMemcpyHostToDevice));
  D.v_bytes = 32 * m; D.u_bytes = 32 * 6 * n; D.ab_bytes = 32 * 2 * n; D.hs_bytes = 32 * (2 * n - 1);
  P_TRY(hipMalloc((void**)&D.v, D.v_bytes)); P_TRY(hipMalloc((void**)&D.u, D.u_bytes)); P_TRY(hipMalloc((void**)&D.ab, D.ab_bytes)); P_TRY(hipMalloc((void**)&D.hs, D.hs_bytes));
  { std::vector<uint32_t> idx(n);
    for (size_t i = 0; i < n; i++) idx[i] = (uint32_t)i;
    P_TRY(hipMalloc((void**)&D.idx, 4 * n)); P_TRY(hipMemcpy(D.idx, idx.data(), 4 * n, hipMemcpyHostToDevice)); }
  // u_X^S, the 1/n of the inverse transforms already in rho's image
  KoFr n_inv; g16_domain_n_inv(D.dom, n_inv.v);
  const KoFr scale = KoFr::to_mont(n_inv);
  const auto t_spmv = std::chrono::steady_clock::now();
  for (int S2 = 0; S2 < 2; S2++) {
    uint32_t* u = D.u + 8 * 3 * n * S2;
    P_TRY(origin_vec(s, KO_EXPAND, m, S2 ? (size_t)cv.n_pub + 1 : 0, S2 ? m : (size_t)cv.n_pub + 1, d_rho, nullptr, scale, D.v));
    P_TRY(g16_spmv3_dict(s, D.mats, D.v, n, u, u + 8 * n, u + 16 * n));
    if (!S2) P_TRY(origin_vec(s, KO_UNITS, (size_t)cv.n_pub + 1, cv.n_c, 0, D.v, nullptr, scale, u));
  }
  if (stats) { P_TRY(hipStreamSynchronize(s)); fprintf(stderr, "key origin: k_origin_vec + k_spmv3_dict for P and Q (2 x 3 products of %u rows, domain %zu): %.3f ms\n", cv.n_c, n, 1e3 * ko_since(t_spmv)); }
  for (int q = 0; q < 6; q++) P_TRY(g16_domain_intt_unscaled(s, D.u + 8 * n * q, D.dom));
  for (int q = 0; q < 2; q++) P_TRY(origin_vec(s, KO_ADD, n, 0, 0, D.u + 8 * n * q, D.u + 8 * n * (3 + q), scale, D.ab + 8 * n * q));
  P_TRY(origin_vec(s, KO_H_SCALARS, 2 * n - 1, n, 0, d_rho + 4 * m, nullptr, KoFr::r2(), D.hs));
  P_TRY(hipStreamSynchronize(s));
  auto msm = [&](size_t base_offset, const uint32_t* sc, size_t count, G1Aff* p) -> int {
    uint64_t pt[8];
    const int rc = vz_msm_device(ctx, D.bases, base_offset, sc, count, 1, 0, pt, VIMZ_FORM_MONTGOMERY);
    if (!rc) { memcpy(p->x.v, pt, 32); memcpy(p->y.v, pt + 4, 32); }
    return rc;
  };
  int rc;
  if ((rc = msm(2 * n, D.ab, n, &out->a)) || (rc = msm(2 * n, D.ab + 8 * n, n, &out->b1)) || (rc = msm(0, D.u, 3 * n, &out->kp)) || (rc = msm(0, D.u + 8 * 3 * n, 3 * n, &out->kq)) ||
      (rc = msm(2 * n, D.hs, 2 * n - 1, &out->h))) return rc;
  XYZZ<Fq2> b2;      // (D.u is spent: its first n elements are the G2 MSM's canonical scalars)
  if ((rc = g16_g2_msm(ctx, s, D.tau2, D.ab + 8 * n, D.idx, (uint32_t)n, D.u, &b2))) return rc;
  out->b2 = to_affine(b2);
  return VIMZ_OK;
}

struct OriginVerdict { uint32_t result = 0; uint64_t first_bad[2] = {0, 0}; double sec[5] = {0, 0, 0, 0, 0}; bool have_points = false; G1Aff key_g1[5], str_g1[5]; G2PowAff key_b2, str_b2; };

struct PowersArrays { const uint64_t* tau_g1; size_t n_tau_g1; const uint64_t *tau_g2, *alpha_g1, *beta_g1; size_t n_pow; const uint64_t* beta_g2; int form; };

// The check itself for a circuit given as a view (the decider's, or a test's).  rho_given: m + n − 1 scalars of 4 words (the test hook's); NULL: from the OS.
int key_origin_core(vimz_ctx* ctx, const G16CircuitView& cv, const void* key, size_t len, const PowersArrays& S, const uint32_t* rho_given, OriginVerdict* V) {
  auto bad = [&](const std::string& msg) { return vz_fail(ctx, VIMZ_ERR_INVALID, ("vimz_decider_key_verify_origin: " + msg).c_str()); };
  if (!vz::pairing::consts().ok) return bad("pairing constants");
  KeyLayout L;
  if (const char* why = key_layout(key, len, &L)) return bad(why);
  const uint64_t* w = (const uint64_t*)key;
  auto verdict = [&](uint32_t bits, uint64_t what, uint64_t where) { V->result = bits; V->first_bad[0] = what; V->first_bad[1] = where; return VIMZ_OK; };
  auto t0 = std::chrono::steady_clock::now();
  // ---- (i) the header and the fixed words ----
  const size_t n = (size_t)1 << cv.logn, m = cv.m, n_l = m - cv.n_pub - 1;
  { const uint64_t want[10] = {cv.m, cv.n_pub, cv.n_c, (uint64_t)n, cv.len_z, cv.mode, cv.pp_hash[0], cv.pp_hash[1], cv.pp_hash[2], cv.pp_hash[3]};
    for (int k = 0; k < 10; k++) if (w[1 + k] != want[k] && (cv.whole_header || (k != 4 && k != 5))) return verdict(VIMZ_KEYORIGIN_HEADER, VIMZ_KEYORIGIN_AT_HEADER, 1 + k); }
  if (cv.logn < 1) return bad("the circuit's domain is a single point");
  if (S.n_pow < n || S.n_tau_g1 < 2 * n - 1) return bad("the string is shorter than the key's domain: n powers are needed, and 2n - 1 of tau in G1");
  StringPoints P;
  P.g1.resize(4 * n - 1); P.tau2.resize(n);
  { const struct { const uint64_t* src; size_t cnt; G1Aff* dst; } g1s[3] = {{S.beta_g1, n, P.g1.data()}, {S.alpha_g1, n, P.g1.data() + n}, {S.tau_g1, 2 * n - 1, P.g1.data() + 2 * n}};
    int rc = 0;
    for (const auto& a : g1s) if (!rc) rc = string_points_in<G1Aff>(a.src, a.cnt, S.form, a.dst);
    if (!rc) rc = string_points_in<G2PowAff>(S.tau_g2, n, S.form, P.tau2.data());
    if (!rc) rc = string_points_in<G2PowAff>(S.beta_g2, 1, S.form, &P.beta2);
    if (rc) return bad(rc == 1 ? "the string: a coordinate is not below the modulus" : "the string: a point is not on its curve"); }
  G1Aff alpha1, beta1, delta1; G2PowAff kzg, beta2, gamma2, delta2;
  { // range first (a finding of its own), then the comparisons
    const bool ok[7] = {get_g2(w + KEY_HEAD_WORDS, &kzg), get_g1(w + 27, &alpha1), get_g1(w + 35, &beta1), get_g2(w + 51, &beta2), get_g2(w + 67, &gamma2), get_g1(w + KEY_DELTA1, &delta1), get_g2(w + KEY_DELTA2, &delta2)};
    for (int k = 0; k < 7; k++) if (!ok[k]) return verdict(VIMZ_KEYORIGIN_COORD, k < 5 ? VIMZ_KEYORIGIN_AT_FIXED : VIMZ_KEYORIGIN_AT_DELTA, k < 5 ? k : k - 5);
    const bool same[5] = {same_g2(kzg, P.tau2[1]), same_g1(alpha1, P.g1[n]), same_g1(beta1, P.g1[0]), same_g2(beta2, P.beta2), same_g2(gamma2, g16_g2_generator())};
    for (int k = 0; k < 5; k++) if (!same[k]) return verdict(VIMZ_KEYORIGIN_FIXED_POINTS, VIMZ_KEYORIGIN_AT_FIXED, k); }
  V->sec[1] += ko_since(t0);
  // ---- (ii) the points: delta's on the host, the arrays one at a time on the device ----
  t0 = std::chrono::steady_clock::now();
  if (!vz::pairing::g1_on_curve(delta1)) return verdict(VIMZ_KEYORIGIN_OFF_CURVE, VIMZ_KEYORIGIN_AT_DELTA, 0);
  if (aff_is_identity(delta1)) return verdict(VIMZ_KEYORIGIN_DELTA, VIMZ_KEYORIGIN_AT_DELTA, 0);
  if (!vz::pairing::g2_on_curve(delta2)) return verdict(VIMZ_KEYORIGIN_OFF_CURVE, VIMZ_KEYORIGIN_AT_DELTA, 1);
  if (aff_is_identity(delta2)) return verdict(VIMZ_KEYORIGIN_DELTA, VIMZ_KEYORIGIN_AT_DELTA, 1);
  if (!vz::pairing::g2_in_subgroup(delta2)) return verdict(VIMZ_KEYORIGIN_SUBGROUP, VIMZ_KEYORIGIN_AT_DELTA, 1);
  V->sec[2] += ko_since(t0);
  KeyArray<G1Aff> ic, a, b1, l, h; KeyArray<G2PowAff> b2;
  StringSide str;
  {
    std::lock_guard<std::mutex> g(ctx->mu);
    P_TRY(hipSetDevice(ctx->device));
    OriginScalars sc;
    sc.rho.resize(4 * (m + n - 1));
    if (rho_given) memcpy(sc.rho.data(), rho_given, 4 * sc.rho.size());
    else if (!g16_os_random(sc.rho.data(), 4 * sc.rho.size())) return bad("no randomness from the OS");
    P_TRY(sc.upload(ctx->stream));
    const size_t off_a = KEY_IC + 8 * ((size_t)cv.n_pub + 1), off_b1 = off_a + 8 * m, off_l = L.off_lh, off_h = off_l + 8 * n_l, off_b2 = off_h + 8 * (n - 1);
    double sec3[3] = {0, 0, 0};
    uint32_t bits = 0; uint64_t which = 0, where = 0;
    auto found = [&](uint32_t b, uint64_t array, size_t index) { if (b && !bits) { bits = b; which = array; where = index; } };
    int rc = judge_key_array<G1Aff>(ctx, w + KEY_IC, (size_t)cv.n_pub + 1, sc.d_order, sc.d_rho, &ic, sec3); found(ic.bits, VIMZ_KEYORIGIN_AT_IC, ic.first);
    if (!rc && !bits) { rc = judge_key_array<G1Aff>(ctx, w + off_a, m, sc.d_order, sc.d_rho, &a, sec3); found(a.bits, VIMZ_KEYORIGIN_AT_A, a.first); }
    if (!rc && !bits) { rc = judge_key_array<G1Aff>(ctx, w + off_b1, m, sc.d_order, sc.d_rho, &b1, sec3); found(b1.bits, VIMZ_KEYORIGIN_AT_B1, b1.first); }
    if (!rc && !bits) { rc = judge_key_array<G1Aff>(ctx, w + off_l, n_l, sc.d_order, sc.d_rho + 4 * ((size_t)cv.n_pub + 1), &l, sec3); found(l.bits, VIMZ_KEYORIGIN_AT_L, l.first); }
    if (!rc && !bits) { rc = judge_key_array<G1Aff>(ctx, w + off_h, n - 1, sc.d_order, sc.d_rho + 4 * m, &h, sec3); found(h.bits, VIMZ_KEYORIGIN_AT_H, h.first); }
    if (!rc && !bits) { rc = judge_key_array<G2PowAff>(ctx, w + off_b2, m, sc.d_order, sc.d_rho, &b2, sec3); found(b2.bits, VIMZ_KEYORIGIN_AT_B2, b2.first); }
    V->sec[1] += sec3[0]; V->sec[2] += sec3[1]; V->sec[4] += sec3[2];
    if (rc) return rc;
    if (bits) return verdict(bits, which, where);
    // ---- (iii) the circuit side ----
    t0 = std::chrono::steady_clock::now();
    if ((rc = string_side(ctx, cv, P, sc.d_rho, getenv("VIMZ_KEY_ORIGIN_STATS") != nullptr, &str))) return rc;
    V->sec[3] += ko_since(t0);
  }
  // ---- the equations, all evaluated ----
  t0 = std::chrono::steady_clock::now();
  const G1Aff g1 = g16_g1_generator(); const G2PowAff g2 = g16_g2_generator();
  typedef std::vector<std::pair<G1Aff, G2PowAff>> Pairs;
  const struct { Pairs pairs; uint32_t bit; } eqs[3] = {{Pairs{{l.sum, delta2}, {ko_g1_neg(str.kq), g2}}, VIMZ_KEYORIGIN_L}, {Pairs{{h.sum, delta2}, {ko_g1_neg(str.h), g2}}, VIMZ_KEYORIGIN_H},
                                                       {Pairs{{delta1, g2}, {ko_g1_neg(g1), delta2}}, VIMZ_KEYORIGIN_DELTA}};
  bool holds[3];
  { std::vector<std::thread> th;
    for (int k = 0; k < 3; k++) th.emplace_back([&eqs, &holds, k] { holds[k] = vz::pairing::product_is_one(eqs[k].pairs); });
    for (auto& x : th) x.join(); }
  uint32_t bits = 0;
  for (int k = 0; k < 3; k++) if (!holds[k]) bits |= eqs[k].bit;
  if (!same_g1(a.sum, str.a)) bits |= VIMZ_KEYORIGIN_A;
  if (!same_g1(b1.sum, str.b1)) bits |= VIMZ_KEYORIGIN_B1;
  if (!same_g2(b2.sum, str.b2)) bits |= VIMZ_KEYORIGIN_B2;
  if (!same_g1(ic.sum, str.kp)) bits |= VIMZ_KEYORIGIN_IC;
  V->sec[4] += ko_since(t0);
  V->have_points = true;
  const G1Aff kg[5] = {a.sum, b1.sum, ic.sum, l.sum, h.sum}, sg[5] = {str.a, str.b1, str.kp, str.kq, str.h};
  memcpy((void*)V->key_g1, (const void*)kg, sizeof(kg)); memcpy((void*)V->str_g1, (const void*)sg, sizeof(sg));
  V->key_b2 = b2.sum; V->str_b2 = str.b2;
  return verdict(bits, 0, 0);
}

bool origin_args_ok(const void* key, const uint64_t* tau_g1, const uint64_t* tau_g2, const uint64_t* alpha_g1, const uint64_t* beta_g1, const uint64_t* beta_g2, const uint32_t* result, const uint64_t* first_bad) {
  return key && tau_g1 && tau_g2 && alpha_g1 && beta_g1 && beta_g2 && result && first_bad;
}

}  // namespace

extern "C" int vimz_decider_key_verify_origin(vimz_cf* prover, const void* key, size_t len, const uint64_t* tau_g1, size_t n_tau_g1, const uint64_t* tau_g2, const uint64_t* alpha_g1,
                                              const uint64_t* beta_g1, size_t n_pow, const uint64_t beta_g2[16], int form, uint32_t* result, uint64_t first_bad[2], double seconds[5]) {
  if (!prover) return VIMZ_ERR_INVALID;
  vimz_ctx* ctx = prover->ctx;
  auto bad = [&](const std::string& msg) { return vz_fail(ctx, VIMZ_ERR_INVALID, ("vimz_decider_key_verify_origin: " + msg).c_str()); };
  if (!origin_args_ok(key, tau_g1, tau_g2, alpha_g1, beta_g1, beta_g2, result, first_bad)) return bad("NULL argument");
  if (form != VIMZ_FORM_CANONICAL && form != VIMZ_FORM_MONTGOMERY) return bad("form is VIMZ_FORM_*");
  KeyLayout L;
  if (const char* why = key_layout(key, len, &L)) return bad(why);
  *result = 0; first_bad[0] = first_bad[1] = 0;
  // the circuit of the mode the blob names
  const auto t0 = std::chrono::steady_clock::now();
  struct Hold { vimz_decider* d; ~Hold() { g16_decider_delete(d); } } hold{g16_decider_new()};
  { const int rc = decider_setup_head(prover, nullptr, ((const uint64_t*)key)[6] == 1, *hold.d); if (rc) return rc; }
  G16CircuitView cv;
  g16_decider_circuit(*hold.d, &cv);
  OriginVerdict V;
  V.sec[0] = ko_since(t0);
  if (getenv("VIMZ_KEY_ORIGIN_STATS")) {      // (read per call) the row-length histogram profiles/key_origin.txt keeps, by bitlen(length)
    static const char* names[3] = {"A", "B", "C"};
    for (int q = 0; q < 3; q++) {
      size_t hist[33] = {}; uint32_t longest = 0;
      for (uint32_t r = 0; r < cv.n_c; r++) { const uint32_t ln = cv.row_ptr[q][r + 1] - cv.row_ptr[q][r]; longest = std::max(longest, ln); int b = 0; while (b < 32 && (ln >> b)) b++; hist[b]++; }
      fprintf(stderr, "key origin: matrix %s of the %s decider: %u rows, %zu entries, longest row %u; rows by bitlen(length) [0: empty, 1: one term, 2: 2-3, 3: 4-7, ..]:", names[q], cv.mode ? "light" : "full", cv.n_c, cv.nnz[q], longest);
      for (int b = 0; b < 33; b++) if (hist[b]) fprintf(stderr, " %d:%zu", b, hist[b]);
      fputc('\n', stderr);
    }
    fprintf(stderr, "key origin: host_spmv3 of the same three matrices with ONE vector, on the host's threads: %.3f ms\n", 1e3 * g16_decider_host_spmv3_seconds(*hold.d));
  }
  const int rc = key_origin_core(ctx, cv, key, len, PowersArrays{tau_g1, n_tau_g1, tau_g2, alpha_g1, beta_g1, n_pow, beta_g2, form}, nullptr, &V);
  if (rc) return rc;
  *result = V.result; first_bad[0] = V.first_bad[0]; first_bad[1] = V.first_bad[1];
  if (seconds) memcpy(seconds, V.sec, sizeof(V.sec));
  return VIMZ_OK;
}

#ifdef VIMZ_TESTING
extern "C" int vimz_test_g16_spmv_dict(vimz_ctx* ctx, const uint32_t* const csr[9], const size_t nnz[3], const uint64_t* dict, size_t n_dict, size_t m, size_t n_c, size_t n, const uint64_t* v,
                                       uint64_t* out_a, uint64_t* out_b, uint64_t* out_c) {
  if (!ctx) return VIMZ_ERR_INVALID;
  auto bad = [&](const std::string& msg) { return vz_fail(ctx, VIMZ_ERR_INVALID, ("vimz_test_g16_spmv_dict: " + msg).c_str()); };
  if (!csr || !nnz || !dict || !v || !out_a || !out_b || !out_c || !n_dict || !m || !n || n < n_c || m >= ((size_t)1 << 31) || n > ((size_t)1 << 26) || n_dict > ((size_t)1 << 26)) return bad("bad argument");
  std::vector<KoFr> dm(n_dict), vm(m);
  auto in = [&](const uint64_t* src, std::vector<KoFr>& dst) { for (size_t i = 0; i < dst.size(); i++) { KoFr c; memcpy(c.v, src + 4 * i, 32); if (!c.is_reduced()) return false; dst[i] = KoFr::to_mont(c); } return true; };
  if (!in(dict, dm) || !in(v, vm)) return bad("an element is not below r");
  G16CircuitView cv{};
  for (int q = 0; q < 3; q++) { cv.row_ptr[q] = csr[q]; cv.col[q] = csr[3 + q]; cv.coef[q] = csr[6 + q]; cv.nnz[q] = nnz[q]; cv.n_row_ptr[q] = n_c + 1; }
  cv.dict = (const uint32_t*)dm.data(); cv.n_dict = n_dict; cv.m = (uint32_t)m; cv.n_c = (uint32_t)n_c;
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  struct Dev { SpmvDevice mats; uint32_t *v = nullptr, *out = nullptr; ~Dev() { g16_spmv_free(mats); if (v) hipFree(v); if (out) hipFree(out); } } D;
  { std::string why;
    const hipError_t e = g16_spmv_upload(cv, &D.mats, &why);
    if (e == hipErrorInvalidValue) return bad(why);
    P_TRY(e); }
  P_TRY(hipMalloc((void**)&D.v, 32 * m)); P_TRY(hipMalloc((void**)&D.out, 32 * 3 * n));
  P_TRY(hipMemcpyAsync(D.v, vm.data(), 32 * m, hipMemcpyHostToDevice, s));
  P_TRY(hipMemsetAsync(D.out, 0xa5, 32 * 3 * n, s));      // (a row the kernel leaves shows)
  P_TRY(g16_spmv3_dict(s, D.mats, D.v, n, D.out, D.out + 8 * n, D.out + 16 * n));
  std::vector<KoFr> res(3 * n);
  P_TRY(hipMemcpyAsync(res.data(), D.out, 32 * 3 * n, hipMemcpyDeviceToHost, s));
  P_TRY(hipStreamSynchronize(s));
  uint64_t* outs[3] = {out_a, out_b, out_c};
  for (int q = 0; q < 3; q++) for (size_t i = 0; i < n; i++) { const KoFr c = KoFr::from_mont(res[q * n + i]); memcpy(outs[q] + 4 * i, c.v, 32); }
  return VIMZ_OK;
}

extern "C" int vimz_test_key_origin(vimz_ctx* ctx, const uint32_t* const csr[9], const size_t nnz[3], const uint64_t* dict, size_t n_dict, size_t m, size_t n_pub, size_t n_c, int logn,
                                    const uint64_t pp_hash[4], const void* key, size_t len, const uint64_t* tau_g1, size_t n_tau_g1, const uint64_t* tau_g2, const uint64_t* alpha_g1,
                                    const uint64_t* beta_g1, size_t n_pow, const uint64_t beta_g2[16], int form, const uint64_t* rho, uint32_t* result, uint64_t first_bad[2],
                                    uint64_t points_out[112]) {
  if (!ctx) return VIMZ_ERR_INVALID;
  auto bad = [&](const std::string& msg) { return vz_fail(ctx, VIMZ_ERR_INVALID, ("vimz_test_key_origin: " + msg).c_str()); };
  if (!csr || !nnz || !dict || !pp_hash || !rho || !points_out || !origin_args_ok(key, tau_g1, tau_g2, alpha_g1, beta_g1, beta_g2, result, first_bad)) return bad("NULL argument");
  if (form != VIMZ_FORM_CANONICAL && form != VIMZ_FORM_MONTGOMERY) return bad("form is VIMZ_FORM_*");
  if (logn < 1 || logn > 20 || !m || m > (1u << 20) || n_pub >= m || !n_dict || n_dict > (1u << 20) || n_c + n_pub + 1 > ((size_t)1 << logn)) return bad("sizes");
  std::vector<KoFr> dm(n_dict);
  for (size_t i = 0; i < n_dict; i++) { KoFr c; memcpy(c.v, dict + 4 * i, 32); if (!c.is_reduced()) return bad("a coefficient is not below r"); dm[i] = KoFr::to_mont(c); }
  G16CircuitView cv{};
  for (int q = 0; q < 3; q++) { cv.row_ptr[q] = csr[q]; cv.col[q] = csr[3 + q]; cv.coef[q] = csr[6 + q]; cv.nnz[q] = nnz[q]; cv.n_row_ptr[q] = n_c + 1; }
  cv.dict = (const uint32_t*)dm.data(); cv.n_dict = n_dict; cv.m = (uint32_t)m; cv.n_pub = (uint32_t)n_pub; cv.n_c = (uint32_t)n_c; cv.logn = logn;
  memcpy(cv.pp_hash, pp_hash, 32); cv.whole_header = false;
  *result = 0; first_bad[0] = first_bad[1] = 0;
  memset(points_out, 0, 8 * 112);
  OriginVerdict V;
  const int rc = key_origin_core(ctx, cv, key, len, PowersArrays{tau_g1, n_tau_g1, tau_g2, alpha_g1, beta_g1, n_pow, beta_g2, form}, (const uint32_t*)rho, &V);
  if (rc) return rc;
  *result = V.result; first_bad[0] = V.first_bad[0]; first_bad[1] = V.first_bad[1];
  if (V.have_points) {      // key side a, b1, b2, ic, l, h, then the string side a, b1, b2, K(P), K(Q), the h combination — canonical
    uint64_t* o = points_out;
    for (int side = 0; side < 2; side++) {
      const G1Aff* g = side ? V.str_g1 : V.key_g1;
      put_g1(o, g[0]); put_g1(o + 8, g[1]); put_g2(o + 16, side ? V.str_b2 : V.key_b2); put_g1(o + 32, g[2]); put_g1(o + 40, g[3]); put_g1(o + 48, g[4]);
      o += 56;
    }
  }
  return VIMZ_OK;
}
#endif
