// Point kernels of a Groth16 set-up from a powers-of-tau string (g16_powers.hpp), each a template over the coordinate field: Fq for G1, Fq2 for G2.
//
// k_scale_points: out_i = k·P_i for ONE scalar k — the step that applies 1/delta to the l and h queries, whose points come from group operations and so have
// no known scalar for k_fixed_mul's window table; and the 1/n of the inverse transform below.
// One thread per point, double-and-add from the top bit over the XYZZ accumulator of ec.hpp with the affine input as the addend (a mixed addition: 8M + 2S
// against the 12M + 2S of a full one).  Every thread walks the same bits, so a wave never diverges on them: the scalar's word is a uniform load, the only
// data-dependent branches are add_mixed's own (identity, doubling, cancellation).  Coordinates stay in the 8 x 32 Montgomery form the points arrive and leave
// in, as in k_fixed_mul; one inversion per point ends the thread (380 of its ~4 300 products).
//
// The transform over points, out_j = Σ_k w^(jk)·P_k (g16_point_transform): k_pt_twiddles writes the table w^k, k < n/2, k_pt_bitrev permutes, and k_pt_stage
// runs ONCE PER STAGE with one thread per butterfly, (u, v) -> (u + w·v, u − w·v): the same double-and-add with a per-thread scalar (a wave diverges on the
// additions), two mixed additions and two inversions.  What a thread does is g16_point_stage.hpp's, which the CPU suite loops over every index
// (tests/native/pt_stage_check.cpp).  A thread touches its own two slots only and no kernel waits on another workgroup: the stream orders the stages.
#include "g16_powers.hpp"
#ifdef VIMZ_TESTING
#include "../../include/vimz_hip_testing.h"
#endif

namespace {

using vz::pairing::Fq2;
constexpr unsigned SCALE_BLOCK = PT_BLOCK;      // one wave per workgroup: 190 VGPRs (G1) hold two waves on a SIMD, and small queries still spread over the CUs

template <class F>
__global__ void __launch_bounds__(SCALE_BLOCK) k_scale_points(const Affine<F>* in, size_t n, const uint32_t* __restrict__ k_canon, Affine<F>* out /* may be in */) {
  const size_t i = blockIdx.x * (size_t)SCALE_BLOCK + threadIdx.x;
  if (i >= n) return;
  const Affine<F> p = in[i];
  out[i] = to_affine(pt_scalar_mul(p, k_canon));
}

// the transform's table: w^k for k < n_half = 2^bits, then 1/n, canonical
__global__ void __launch_bounds__(PT_BLOCK) k_pt_twiddles(uint32_t* __restrict__ twiddles, size_t n_half, int bits, Fe w, Fe n_inv_canon) {
  const size_t k = blockIdx.x * (size_t)PT_BLOCK + threadIdx.x;
  if (k < n_half) pt_twiddle(k, bits, w, twiddles);
  else if (k == n_half) for (int i = 0; i < 8; i++) twiddles[8 * n_half + i] = n_inv_canon.v[i];
}
template <class F>
__global__ void __launch_bounds__(PT_BLOCK) k_pt_bitrev(Affine<F>* points, size_t n, int logn) {
  const size_t i = blockIdx.x * (size_t)PT_BLOCK + threadIdx.x;
  if (i < n) pt_bitrev_swap(i, logn, points);
}
// one stage: thread t is butterfly t on the slots lo, lo + half (g16_point_stage.hpp) — no two threads share a slot
template <class F>
__global__ void __launch_bounds__(PT_BLOCK) k_pt_stage(Affine<F>* points, size_t n_half, size_t half, const uint32_t* __restrict__ twiddles) {
  const size_t t = blockIdx.x * (size_t)PT_BLOCK + threadIdx.x;
  if (t < n_half) pt_butterfly(t, half, n_half, points, twiddles);
}

// the column sums: thread t is run t of one level of the plan (g16_point_stage.hpp: colsum_run) — it writes its own slot and reads nothing written in this launch
template <class F>
__global__ void __launch_bounds__(PT_BLOCK) k_col_runs(const ColsumRun* __restrict__ runs, uint32_t n_runs, const uint32_t* __restrict__ entries, const uint32_t* __restrict__ mags,
                                                       const Affine<F>* __restrict__ src, Affine<F>* __restrict__ partials, Affine<F>* __restrict__ out) {
  const size_t t = blockIdx.x * (size_t)PT_BLOCK + threadIdx.x;
  if (t < n_runs) colsum_run(t, runs, entries, mags, src, partials, out);
}
// the h query before 1/delta: thread j writes out[j] = P[j + n] − P[j]
template <class F>
__global__ void __launch_bounds__(PT_BLOCK) k_point_diff(const Affine<F>* __restrict__ points, size_t n, Affine<F>* __restrict__ out) {
  const size_t j = blockIdx.x * (size_t)PT_BLOCK + threadIdx.x;
  if (j + 1 < n) pt_diff(j, n, points, out);
}

unsigned pt_blocks(size_t threads) { return (unsigned)((threads + PT_BLOCK - 1) / PT_BLOCK); }

template <class F>
hipError_t scale_points(hipStream_t s, const Affine<F>* in, size_t n, const uint32_t* k_canon, Affine<F>* out) {
  if (!n) return hipSuccess;
  if (!in || !out || !k_canon || n > ((size_t)1 << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_scale_points<F>, dim3(pt_blocks(n)), dim3(SCALE_BLOCK), 0, s, in, n, k_canon, out);
  return hipGetLastError();
}

template <class F>
hipError_t point_transform(hipStream_t s, Affine<F>* points, int logn, bool inverse, bool scaled, uint32_t* twiddles) {
  if (!points || !twiddles || logn < 1 || logn > 26) return hipErrorInvalidValue;
  const size_t n = (size_t)1 << logn, n_half = n / 2;
  Fe w = fr_root_of_unity(logn);
  if (inverse) w = Fe::pow_pm2(w);
  const Fe n_inv = Fe::from_mont(Fe::pow_pm2(cb::f_from_u64<Fe>(n)));
  hipLaunchKernelGGL(k_pt_twiddles, dim3(pt_blocks(n_half + 1)), dim3(PT_BLOCK), 0, s, twiddles, n_half, logn - 1, w, n_inv);
  hipLaunchKernelGGL(k_pt_bitrev<F>, dim3(pt_blocks(n)), dim3(PT_BLOCK), 0, s, points, n, logn);
  for (size_t half = 1; half < n; half *= 2)
    hipLaunchKernelGGL(k_pt_stage<F>, dim3(pt_blocks(n_half)), dim3(PT_BLOCK), 0, s, points, n_half, half, (const uint32_t*)twiddles);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && scaled) e = scale_points<F>(s, points, n, twiddles + 8 * n_half, points);
  return e;
}

template <class F>
hipError_t column_sums(hipStream_t s, const ColsumDevice& dev, const Affine<F>* points, Affine<F>* out) {
  if (!dev.n_cols) return hipSuccess;
  if (!points || !out || dev.point_bytes != sizeof(Affine<F>)) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(out, 0, sizeof(Affine<F>) * (size_t)dev.n_cols, s);      // columns without entries: the identity
  for (size_t k = 0; k < dev.levels.size() && e == hipSuccess; k++) {
    const ColsumDevice::Level& lv = dev.levels[k];
    if (!lv.n_runs) continue;
    const Affine<F>* src = k ? (const Affine<F>*)dev.partials[(k - 1) & 1] : points;
    hipLaunchKernelGGL(k_col_runs<F>, dim3(pt_blocks(lv.n_runs)), dim3(PT_BLOCK), 0, s, (const ColsumRun*)(dev.runs + lv.first), lv.n_runs,
                       (const uint32_t*)(k ? nullptr : dev.entries), (const uint32_t*)dev.mags, src, (Affine<F>*)dev.partials[k & 1], out);
    e = hipGetLastError();
  }
  return e;
}

}  // namespace

hipError_t g16_colsum_upload(const ColsumPlan& plan, size_t point_bytes, ColsumDevice* dev) {
  ColsumDevice d;
  d.n_cols = plan.n_cols; d.n_points = plan.n_points; d.point_bytes = point_bytes;
  std::vector<ColsumRun> runs;
  for (const ColsumLevel& lv : plan.levels) { d.levels.push_back({runs.size(), (uint32_t)lv.runs.size(), lv.n_partials}); runs.insert(runs.end(), lv.runs.begin(), lv.runs.end()); }
  hipError_t e = hipSuccess;
  auto up = [&](void** dst, const void* src, size_t bytes) {
    if (e != hipSuccess) return;
    e = hipMalloc(dst, std::max<size_t>(bytes, 4));
    if (e == hipSuccess && bytes) e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
  };
  up((void**)&d.entries, plan.entries.data(), 4 * plan.entries.size());
  up((void**)&d.mags, plan.mags.data(), 4 * plan.mags.size());
  up((void**)&d.runs, runs.data(), sizeof(ColsumRun) * runs.size());
  // partials: level k's in buffer k & 1
  size_t need[2] = {0, 0};
  for (size_t k = 0; k < plan.levels.size(); k++) need[k & 1] = std::max<size_t>(need[k & 1], plan.levels[k].n_partials);
  for (int b = 0; b < 2 && e == hipSuccess; b++) if (need[b]) e = hipMalloc(&d.partials[b], point_bytes * need[b]);
  if (e != hipSuccess) { g16_colsum_free(d); return e; }
  *dev = d;
  return hipSuccess;
}
void g16_colsum_free(ColsumDevice& d) {
  for (void* p : {(void*)d.entries, (void*)d.mags, (void*)d.runs, d.partials[0], d.partials[1]}) if (p) hipFree(p);
  d = ColsumDevice();
}
hipError_t g16_column_sums(hipStream_t s, const ColsumDevice& dev, const G1Aff* points, G1Aff* out) { return column_sums<Fq>(s, dev, points, out); }
hipError_t g16_column_sums(hipStream_t s, const ColsumDevice& dev, const G2PowAff* points, G2PowAff* out) { return column_sums<Fq2>(s, dev, points, out); }
hipError_t g16_h_query(hipStream_t s, const G1Aff* tau_g1, size_t n, const uint32_t* dinv_canon, G1Aff* out) {
  if (n < 2) return hipSuccess;
  if (!tau_g1 || !dinv_canon || !out || n > ((size_t)1 << 26)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_point_diff<Fq>, dim3(pt_blocks(n - 1)), dim3(PT_BLOCK), 0, s, tau_g1, n, out);
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? e : scale_points<Fq>(s, out, n - 1, dinv_canon, out);
}

hipError_t g16_scale_points(hipStream_t s, const G1Aff* in, size_t n, const uint32_t* k_canon, G1Aff* out) { return scale_points<Fq>(s, in, n, k_canon, out); }
hipError_t g16_scale_points(hipStream_t s, const G2PowAff* in, size_t n, const uint32_t* k_canon, G2PowAff* out) { return scale_points<Fq2>(s, in, n, k_canon, out); }
hipError_t g16_point_transform(hipStream_t s, G1Aff* points, int logn, bool inverse, bool scaled, uint32_t* twiddles) {
  return point_transform<Fq>(s, points, logn, inverse, scaled, twiddles);
}
hipError_t g16_point_transform(hipStream_t s, G2PowAff* points, int logn, bool inverse, bool scaled, uint32_t* twiddles) {
  return point_transform<Fq2>(s, points, logn, inverse, scaled, twiddles);
}

// ---- the Lagrange basis of a string's points: vimz_powers_lagrange, and the hook that reaches every direction of the transform ----------------------
namespace {

// n_coord coordinates of 4 words into Montgomery form; false: one is not below q
bool coords_in(const uint64_t* words, size_t n_coord, int form, Fq* out) {
  for (size_t i = 0; i < n_coord; i++) {
    Fq c; memcpy(c.v, words + 4 * i, 32);
    if (!c.is_reduced()) return false;
    out[i] = form == VIMZ_FORM_MONTGOMERY ? c : Fq::to_mont(c);
  }
  return true;
}
void coords_out(const Fq* in, size_t n_coord, int form, uint64_t* words) {
  for (size_t i = 0; i < n_coord; i++) { const Fq c = form == VIMZ_FORM_MONTGOMERY ? in[i] : Fq::from_mont(in[i]); memcpy(words + 4 * i, c.v, 32); }
}
bool on_curve(const G1Aff& p) { return aff_on_curve(p); }
bool on_curve(const G2PowAff& p) { return vz::pairing::g2_on_curve(p); }
double since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

// words of 2^logn points -> the transform on the context's stream, under its lock -> words.  seconds (optional) = {host conversion and checks, device}
template <class A>
int transform_words(vimz_ctx* ctx, const char* who, const uint64_t* points, int form, int logn, bool inverse, bool scaled, uint64_t* out, double seconds[2]) {
  const size_t n = (size_t)1 << logn, per = sizeof(A) / sizeof(Fq);
  auto t0 = std::chrono::steady_clock::now();
  std::vector<A> pts(n);
  if (!coords_in(points, n * per, form, (Fq*)pts.data())) return vz_fail(ctx, VIMZ_ERR_INVALID, (std::string(who) + ": a coordinate is not below the modulus").c_str());
  for (size_t i = 0; i < n; i++) if (!on_curve(pts[i])) return vz_fail(ctx, VIMZ_ERR_INVALID, (std::string(who) + ": a point is not on the curve").c_str());
  double host_s = since(t0), dev_s = 0;
  {
    std::lock_guard<std::mutex> g(ctx->mu);
    t0 = std::chrono::steady_clock::now();
    P_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    A* d_pts = nullptr; uint32_t* d_tw = nullptr;
    struct Free { A** p; uint32_t** t; ~Free() { if (*p) hipFree(*p); if (*t) hipFree(*t); } } fr{&d_pts, &d_tw};
    P_TRY(hipMalloc((void**)&d_pts, sizeof(A) * n)); P_TRY(hipMalloc((void**)&d_tw, 4 * g16_point_transform_words(logn)));
    P_TRY(hipMemcpyAsync(d_pts, pts.data(), sizeof(A) * n, hipMemcpyHostToDevice, s));
    P_TRY(g16_point_transform(s, d_pts, logn, inverse, scaled, d_tw));
    P_TRY(hipMemcpyAsync(pts.data(), d_pts, sizeof(A) * n, hipMemcpyDeviceToHost, s));
    P_TRY(hipStreamSynchronize(s));
    dev_s = since(t0);
  }
  t0 = std::chrono::steady_clock::now();
  coords_out((const Fq*)pts.data(), n * per, form, out);
  host_s += since(t0);
  if (seconds) { seconds[0] = host_s; seconds[1] = dev_s; }
  return VIMZ_OK;
}

}  // namespace

extern "C" int vimz_powers_lagrange(vimz_ctx* ctx, int group, const uint64_t* points, size_t n_points, int form, int logn, uint64_t* out, double seconds[2]) {
  if (!ctx || !points || !out) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_powers_lagrange: NULL argument");
  if ((group != 1 && group != 2) || (form != VIMZ_FORM_CANONICAL && form != VIMZ_FORM_MONTGOMERY)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_powers_lagrange: group is 1 or 2, form VIMZ_FORM_*");
  if (logn < 1 || logn > 26 || n_points < ((size_t)1 << logn)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_powers_lagrange: needs 1 <= logn <= 26 and 2^logn points");
  return group == 1 ? transform_words<G1Aff>(ctx, "vimz_powers_lagrange", points, form, logn, true, true, out, seconds)
                    : transform_words<G2PowAff>(ctx, "vimz_powers_lagrange", points, form, logn, true, true, out, seconds);
}

#ifdef VIMZ_TESTING
extern "C" int vimz_test_g16_scale_points(vimz_ctx* ctx, const uint64_t* points_xy, size_t n, const uint64_t scalar[4], uint64_t* out_xy) {
  if (!ctx || !points_xy || !scalar || !out_xy || !n || n > (1u << 26)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_g16_scale_points: bad argument");
  Fe k; memcpy(k.v, scalar, 32);
  if (!k.is_reduced()) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_g16_scale_points: the scalar is not below the modulus");
  std::vector<G1Aff> pts(n);
  for (size_t i = 0; i < n; i++) {
    Fq x, y; memcpy(x.v, points_xy + 8 * i, 32); memcpy(y.v, points_xy + 8 * i + 4, 32);
    if (!x.is_reduced() || !y.is_reduced()) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_g16_scale_points: a coordinate is not below the modulus");
    pts[i].x = Fq::to_mont(x); pts[i].y = Fq::to_mont(y);
    if (!aff_on_curve(pts[i])) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_g16_scale_points: a point is not on the curve");
  }
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  G1Aff* d_pts = nullptr; uint32_t* d_k = nullptr;
  struct Free { G1Aff** p; uint32_t** k; ~Free() { if (*p) hipFree(*p); if (*k) hipFree(*k); } } fr{&d_pts, &d_k};
  P_TRY(hipMalloc((void**)&d_pts, sizeof(G1Aff) * n)); P_TRY(hipMalloc((void**)&d_k, 32));
  P_TRY(hipMemcpyAsync(d_pts, pts.data(), sizeof(G1Aff) * n, hipMemcpyHostToDevice, s));
  P_TRY(hipMemcpyAsync(d_k, k.v, 32, hipMemcpyHostToDevice, s));
  P_TRY(g16_scale_points(s, d_pts, n, d_k, d_pts));      // in place, as the set-up scales a query where it lies
  P_TRY(hipMemsetAsync(d_k, 0, 32, s));                  // (the caller's duty: the scalar's device copy does not outlive its use)
  P_TRY(hipMemcpyAsync(pts.data(), d_pts, sizeof(G1Aff) * n, hipMemcpyDeviceToHost, s));
  P_TRY(hipStreamSynchronize(s));
  for (size_t i = 0; i < n; i++) {
    const Fq x = Fq::from_mont(pts[i].x), y = Fq::from_mont(pts[i].y);
    memcpy(out_xy + 8 * i, x.v, 32); memcpy(out_xy + 8 * i + 4, y.v, 32);
  }
  return VIMZ_OK;
}

extern "C" int vimz_test_g16_point_transform(vimz_ctx* ctx, int group, int logn, int inverse, int scaled, const uint64_t* points, uint64_t* out) {
  if (!ctx || !points || !out || (group != 1 && group != 2) || logn < 1 || logn > 26) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_g16_point_transform: bad argument");
  return group == 1 ? transform_words<G1Aff>(ctx, "vimz_test_g16_point_transform", points, VIMZ_FORM_CANONICAL, logn, inverse != 0, scaled != 0, out, nullptr)
                    : transform_words<G2PowAff>(ctx, "vimz_test_g16_point_transform", points, VIMZ_FORM_CANONICAL, logn, inverse != 0, scaled != 0, out, nullptr);
}

namespace {
// the hook's column sums for one group: the plan of the caller's matrix, uploaded, g16_column_sums on the context's stream
template <class A>
int column_sums_words(vimz_ctx* ctx, const uint32_t* row_ptr, const uint32_t* col, const uint32_t* coef, size_t n_rows, size_t n_cols, const uint64_t* dict, size_t n_dict,
                      const uint64_t* points, int form, uint64_t* out) {
  const char* who = "vimz_test_g16_column_sums";
  const size_t per = sizeof(A) / sizeof(Fq);
  std::vector<A> pts(std::max<size_t>(n_rows, 1)), res(n_cols);
  if (!coords_in(points, n_rows * per, form, (Fq*)pts.data())) return vz_fail(ctx, VIMZ_ERR_INVALID, (std::string(who) + ": a coordinate is not below the modulus").c_str());
  for (size_t i = 0; i < n_rows; i++) if (!on_curve(pts[i])) return vz_fail(ctx, VIMZ_ERR_INVALID, (std::string(who) + ": a point is not on the curve").c_str());
  ColsumPlan plan; std::string err;
  const ColsumPart part{row_ptr, col, coef, (uint32_t)n_rows, 0u};
  if (!colsum_plan(&part, 1, nullptr, 0, (const uint32_t*)dict, n_dict, BnFr::MOD.w, (uint32_t)n_cols, (uint32_t)n_rows, &plan, &err)) return vz_fail(ctx, VIMZ_ERR_INVALID, (std::string(who) + ": " + err).c_str());
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  ColsumDevice dev; A *d_pts = nullptr, *d_out = nullptr;
  struct Free { ColsumDevice* d; A **p, **o; ~Free() { g16_colsum_free(*d); if (*p) hipFree(*p); if (*o) hipFree(*o); } } fr{&dev, &d_pts, &d_out};
  P_TRY(g16_colsum_upload(plan, sizeof(A), &dev));
  P_TRY(hipMalloc((void**)&d_pts, sizeof(A) * pts.size())); P_TRY(hipMalloc((void**)&d_out, sizeof(A) * n_cols));
  P_TRY(hipMemcpyAsync(d_pts, pts.data(), sizeof(A) * n_rows, hipMemcpyHostToDevice, s));
  P_TRY(g16_column_sums(s, dev, (const A*)d_pts, d_out));
  P_TRY(hipMemcpyAsync(res.data(), d_out, sizeof(A) * n_cols, hipMemcpyDeviceToHost, s));
  P_TRY(hipStreamSynchronize(s));
  coords_out((const Fq*)res.data(), n_cols * per, form, out);
  return VIMZ_OK;
}
}  // namespace

extern "C" int vimz_test_g16_column_sums(vimz_ctx* ctx, int group, const uint32_t* row_ptr, const uint32_t* col, const uint32_t* coef, size_t n_rows, size_t n_cols,
                                         const uint64_t* dict, size_t n_dict, const uint64_t* points, int form, uint64_t* out) {
  if (!ctx || !row_ptr || !col || !coef || !dict || !points || !out || (group != 1 && group != 2) || (form != VIMZ_FORM_CANONICAL && form != VIMZ_FORM_MONTGOMERY)
      || !n_cols || n_cols > (1u << 26) || n_rows > (1u << 26) || !n_dict || n_dict > (1u << 26))
    return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_g16_column_sums: bad argument");
  return group == 1 ? column_sums_words<G1Aff>(ctx, row_ptr, col, coef, n_rows, n_cols, dict, n_dict, points, form, out)
                    : column_sums_words<G2PowAff>(ctx, row_ptr, col, coef, n_rows, n_cols, dict, n_dict, points, form, out);
}

extern "C" int vimz_test_g16_h_query(vimz_ctx* ctx, const uint64_t* tau_g1_xy, size_t n, const uint64_t delta_inv[4], uint64_t* out_xy) {
  if (!ctx || !tau_g1_xy || !delta_inv || !out_xy || n < 2 || n > (1u << 24)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_g16_h_query: bad argument");
  Fe k; memcpy(k.v, delta_inv, 32);
  if (!k.is_reduced()) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_g16_h_query: the scalar is not below the modulus");
  const size_t n_in = 2 * n - 1, n_out = n - 1;
  std::vector<G1Aff> pts(n_in);
  if (!coords_in(tau_g1_xy, 2 * n_in, VIMZ_FORM_CANONICAL, (Fq*)pts.data())) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_g16_h_query: a coordinate is not below the modulus");
  for (size_t i = 0; i < n_in; i++) if (!aff_on_curve(pts[i])) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_g16_h_query: a point is not on the curve");
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  G1Aff *d_pts = nullptr, *d_out = nullptr; uint32_t* d_k = nullptr;
  struct Free { G1Aff **p, **o; uint32_t** k; ~Free() { if (*p) hipFree(*p); if (*o) hipFree(*o); if (*k) hipFree(*k); } } fr{&d_pts, &d_out, &d_k};
  P_TRY(hipMalloc((void**)&d_pts, sizeof(G1Aff) * n_in)); P_TRY(hipMalloc((void**)&d_out, sizeof(G1Aff) * n_out)); P_TRY(hipMalloc((void**)&d_k, 32));
  P_TRY(hipMemcpyAsync(d_pts, pts.data(), sizeof(G1Aff) * n_in, hipMemcpyHostToDevice, s));
  P_TRY(hipMemcpyAsync(d_k, k.v, 32, hipMemcpyHostToDevice, s));
  P_TRY(g16_h_query(s, d_pts, n, d_k, d_out));
  P_TRY(hipMemsetAsync(d_k, 0, 32, s));
  P_TRY(hipMemcpyAsync(pts.data(), d_out, sizeof(G1Aff) * n_out, hipMemcpyDeviceToHost, s));
  P_TRY(hipStreamSynchronize(s));
  coords_out((const Fq*)pts.data(), 2 * n_out, VIMZ_FORM_CANONICAL, out_xy);
  return VIMZ_OK;
}
#endif
