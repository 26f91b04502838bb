// vimz_decider_verify_batch: many decider proofs under one key in one call (decider_batch.hpp has the equation, the chunk and fallback rule and the host path;
// DESIGN.md §5d).  This file is the device side: the part of a batch that grows with it — per proof the curve and subgroup checks of its points, twelve G1 scalar
// multiplications and ONE Miller loop, because every proof brings its own B — as three stages on the context's stream:
//   k_powers_flags (g16_powers_verify.hip)   the 8 G1 points and the B of every proof the host's parse let through; the flags are read on the host
//   k_g1_lincomb                             out[t] = a[t] + k[t]·b[t], one thread a row (pairing_stage.hpp: g1_lincomb_thread), then g16_column_sums per chunk
//   k_miller                                 thread t: the Miller value of (−rho_t·A_t, B_t) into its own 96 words (pairing_stage.hpp: miller_thread)
// Every kernel has the point kernels' shape: one thread an element, a thread writes its own slot, no atomics, no flag another workgroup reads, every loop bound
// from the host (k_miller's is the constant 64), PT_BLOCK threads a block.  The host multiplies the Miller values per chunk with its five fixed-G2 loops and
// exponentiates once a chunk.  The multipliers' copies are wiped on both sides.
#include "g16_powers.hpp"
#include "decider_batch.hpp"
#ifdef VIMZ_TESTING
#include "../../include/vimz_hip_testing.h"
#endif

namespace {

using namespace vz::dvb;
using vz::pairing::Fq12;
using vz::pairing::Fq2;
typedef vz::dv::G1A G1A;
typedef vz::dv::G2A G2A;

__global__ void __launch_bounds__(PT_BLOCK) k_g1_lincomb(const G1A* __restrict__ a, const uint32_t* __restrict__ k, const uint32_t* __restrict__ bits, const G1A* __restrict__ b, size_t n,
                                                         G1A* __restrict__ out) {
  const size_t t = blockIdx.x * (size_t)PT_BLOCK + threadIdx.x;
  if (t < n) vz::pairing::g1_lincomb_thread(t, a, k, bits, b, out);
}
__global__ void __launch_bounds__(PT_BLOCK) k_miller(const G1A* __restrict__ P, const G2A* __restrict__ Q, size_t n, Fq2 twist_b, Fq2 g12, Fq2 g13, Fq12* __restrict__ out) {
  const size_t t = blockIdx.x * (size_t)PT_BLOCK + threadIdx.x;
  if (t < n) vz::pairing::miller_thread(t, P, Q, twist_b, g12, g13, out);
}
unsigned db_blocks(size_t threads) { return (unsigned)((threads + PT_BLOCK - 1) / PT_BLOCK); }

hipError_t launch_lincomb(hipStream_t s, const G1A* a, const uint32_t* k, const uint32_t* bits, const G1A* b, size_t n, G1A* out) {
  if (!n) return hipSuccess;
  if (!a || !k || !bits || !b || !out || n > ((size_t)1 << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_g1_lincomb, dim3(db_blocks(n)), dim3(PT_BLOCK), 0, s, a, k, bits, b, n, out);
  return hipGetLastError();
}
hipError_t launch_miller(hipStream_t s, const G1A* P, const G2A* Q, size_t n, Fq12* out) {
  if (!n) return hipSuccess;
  if (!P || !Q || !out || n > ((size_t)1 << 31)) return hipErrorInvalidValue;
  const vz::pairing::Consts& C = vz::pairing::consts();
  hipLaunchKernelGGL(k_miller, dim3(db_blocks(n)), dim3(PT_BLOCK), 0, s, P, Q, n, C.twist_b, C.g12, C.g13, out);
  return hipGetLastError();
}

// the three stages on the context's stream; the caller holds the context's lock and has set the device.  A failed call leaves its error in `err`.
struct DeviceStages : Stages {
  vimz_ctx* ctx; hipStream_t s; hipError_t err = hipSuccess; const char* what = "";
  G1A* d_rows = nullptr; size_t rows_m = 0;
  explicit DeviceStages(vimz_ctx* c) : ctx(c), s(c->stream) {}
  ~DeviceStages() override { if (d_rows) hipFree(d_rows); }
#define DB_TRY(x) do { err = (x); if (err != hipSuccess) { what = #x; return false; } } while (0)
  struct Buf { void* p = nullptr; ~Buf() { if (p) hipFree(p); } hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); } template <class T> T* as() { return (T*)p; } };

  bool point_flags(const G1A* g1, size_t n1, const G2A* g2, size_t n2, uint32_t* flags1, uint32_t* flags2) override {
    Buf p1, p2, f, order;
    DB_TRY(p1.alloc(sizeof(G1A) * n1)); DB_TRY(p2.alloc(sizeof(G2A) * n2)); DB_TRY(f.alloc(4 * (n1 + n2))); DB_TRY(order.alloc(32));
    DB_TRY(hipMemcpyAsync(p1.p, g1, sizeof(G1A) * n1, hipMemcpyHostToDevice, s)); DB_TRY(hipMemcpyAsync(p2.p, g2, sizeof(G2A) * n2, hipMemcpyHostToDevice, s));
    DB_TRY(hipMemcpyAsync(order.p, BnFr::MOD.w, 32, hipMemcpyHostToDevice, s));
    DB_TRY(g16_powers_flags(s, (const G1Aff*)p1.p, n1, order.as<uint32_t>(), f.as<uint32_t>()));
    DB_TRY(g16_powers_flags(s, (const G2PowAff*)p2.p, n2, order.as<uint32_t>(), f.as<uint32_t>() + n1));
    DB_TRY(hipMemcpyAsync(flags1, f.p, 4 * n1, hipMemcpyDeviceToHost, s)); DB_TRY(hipMemcpyAsync(flags2, f.as<uint32_t>() + n1, 4 * n2, hipMemcpyDeviceToHost, s));
    DB_TRY(hipStreamSynchronize(s));
    return true;
  }
  bool lincomb(size_t m, const G1A* a, const uint32_t* k, const uint32_t* bits, const G1A* b, const ColsumPlan& plan, G1A* cm, G1A* sums) override {
    const size_t rows = (size_t)ROWS * m;
    Buf da, db, dk, dbits, dsums;
    struct Plan { ColsumDevice d; ~Plan() { g16_colsum_free(d); } } P;
    if (d_rows) { hipFree(d_rows); d_rows = nullptr; }
    DB_TRY(hipMalloc((void**)&d_rows, sizeof(G1A) * rows)); rows_m = m;
    DB_TRY(da.alloc(sizeof(G1A) * rows)); DB_TRY(db.alloc(sizeof(G1A) * rows)); DB_TRY(dk.alloc(32 * rows)); DB_TRY(dbits.alloc(4 * rows)); DB_TRY(dsums.alloc(sizeof(G1A) * plan.n_cols));
    // (from here the scalars are on the device: every way out passes the wipe)
    auto wipe = [&] { hipMemsetAsync(dk.p, 0, 32 * rows, s); hipStreamSynchronize(s); };
    bool ok = [&] {
      DB_TRY(hipMemcpyAsync(da.p, a, sizeof(G1A) * rows, hipMemcpyHostToDevice, s)); DB_TRY(hipMemcpyAsync(db.p, b, sizeof(G1A) * rows, hipMemcpyHostToDevice, s));
      DB_TRY(hipMemcpyAsync(dk.p, k, 32 * rows, hipMemcpyHostToDevice, s)); DB_TRY(hipMemcpyAsync(dbits.p, bits, 4 * rows, hipMemcpyHostToDevice, s));
      DB_TRY(launch_lincomb(s, da.as<G1A>(), dk.as<uint32_t>(), dbits.as<uint32_t>(), db.as<G1A>(), rows, d_rows));
      DB_TRY(g16_colsum_upload(plan, sizeof(G1A), &P.d));
      DB_TRY(g16_column_sums(s, P.d, (const G1Aff*)d_rows, (G1Aff*)dsums.p));
      DB_TRY(hipMemcpyAsync(cm, d_rows, sizeof(G1A) * 2 * m, hipMemcpyDeviceToHost, s));
      DB_TRY(hipMemcpyAsync(sums, dsums.p, sizeof(G1A) * plan.n_cols, hipMemcpyDeviceToHost, s));
      return true;
    }();
    wipe();
    return ok;
  }
  // (no multiplier is uploaded here: the plan names rows, the rows are points)
  bool subset_sums(size_t m, const ColsumPlan& plan, G1A* sums) override {
    if (!d_rows || m != rows_m || plan.n_points != (size_t)ROWS * m) { err = hipErrorInvalidValue; what = "subset sums before the rows"; return false; }
    Buf dsums;
    struct Plan { ColsumDevice d; ~Plan() { g16_colsum_free(d); } } P;
    DB_TRY(dsums.alloc(sizeof(G1A) * plan.n_cols));
    DB_TRY(g16_colsum_upload(plan, sizeof(G1A), &P.d));
    DB_TRY(g16_column_sums(s, P.d, (const G1Aff*)d_rows, (G1Aff*)dsums.p));
    DB_TRY(hipMemcpyAsync(sums, dsums.p, sizeof(G1A) * plan.n_cols, hipMemcpyDeviceToHost, s));
    DB_TRY(hipStreamSynchronize(s));
    return true;
  }
  bool miller(size_t m, const G2A* B, Fq12* out) override {
    if (!d_rows || m != rows_m) { err = hipErrorInvalidValue; what = "the Miller stage before the rows"; return false; }
    Buf dq, dout;
    DB_TRY(dq.alloc(sizeof(G2A) * m)); DB_TRY(dout.alloc(sizeof(Fq12) * m));
    DB_TRY(hipMemcpyAsync(dq.p, B, sizeof(G2A) * m, hipMemcpyHostToDevice, s));
    DB_TRY(launch_miller(s, d_rows + (size_t)R_NA * m, dq.as<G2A>(), m, dout.as<Fq12>()));
    DB_TRY(hipMemcpyAsync(out, dout.p, sizeof(Fq12) * m, hipMemcpyDeviceToHost, s));
    DB_TRY(hipStreamSynchronize(s));
    return true;
  }
#undef DB_TRY
};

unsigned batch_threads() { return std::max(1u, std::min(16u, usable_cpus())); }      // as the decider's host code sizes its pools (g16_powers_verify.hip: points_in)

int batch_entry(const char* name, vimz_ctx* ctx, const uint64_t* key_words, size_t n_key_words, uint32_t len_z, size_t n, const uint64_t* steps, const uint64_t* z0, const uint64_t* zi,
                const uint64_t* words, size_t chunk, const uint64_t* given, uint32_t* results, double seconds[6], uint32_t flags, size_t leaf, uint64_t* stats) {
  auto bad = [&](const char* why) { const std::string m = std::string(name) + ": " + why; return vz_fail(ctx, VIMZ_ERR_INVALID, m.c_str()); };
  if (!key_words) return bad("NULL key");
  if (n && (!steps || !z0 || !zi || !words || !results)) return bad("NULL argument");
  if (!vz::pairing::consts().ok) return bad("pairing constants");
  VerifierKey K;
  if (!parse_key(key_words, n_key_words, &K)) return bad("malformed key");
  if (K.len_z != len_z) return bad("len_z disagrees with the key");
  if (flags & ~BATCH_NO_BISECT) return bad("unknown flag");
  if (!chunk) chunk = DEFAULT_CHUNK;
  if (!leaf) leaf = ctx ? DEFAULT_LEAF : DEFAULT_LEAF_HOST;
  int rc;
  if (!ctx) { HostStages st(batch_threads()); rc = verify_batch(K, n, steps, z0, zi, words, chunk, given, st, batch_threads(), results, seconds, flags, leaf, stats); }
  else {
    std::lock_guard<std::mutex> g(ctx->mu);
    P_TRY(hipSetDevice(ctx->device));
    DeviceStages st(ctx);
    rc = verify_batch(K, n, steps, z0, zi, words, chunk, given, st, batch_threads(), results, seconds, flags, leaf, stats);
    if (rc == BATCH_STAGE_FAILED) return vz_fail(ctx, VIMZ_ERR_HIP, st.what, st.err);
  }
  switch (rc) {
    case BATCH_OK: return VIMZ_OK;
    case BATCH_NO_RANDOMNESS: return bad("no randomness from the OS");
    case BATCH_ZERO_MULTIPLIER: return bad("a multiplier is zero");
    case BATCH_TOO_MANY: return bad("more than 2^26 proofs");
    default: return bad("a stage failed");
  }
}

}  // namespace

extern "C" int vimz_decider_verify_batch(vimz_ctx* ctx, const uint64_t* key_words, size_t n_key_words, uint32_t len_z, size_t n, const uint64_t* steps, const uint64_t* z0,
                                         const uint64_t* zi, const uint64_t* words, size_t chunk, uint32_t* results, double seconds[6]) {
  return vimz_decider_verify_batch_ex(ctx, key_words, n_key_words, len_z, n, steps, z0, zi, words, chunk, results, seconds, 0, 0, nullptr);
}
extern "C" int vimz_decider_verify_batch_ex(vimz_ctx* ctx, const uint64_t* key_words, size_t n_key_words, uint32_t len_z, size_t n, const uint64_t* steps, const uint64_t* z0,
                                            const uint64_t* zi, const uint64_t* words, size_t chunk, uint32_t* results, double seconds[6], uint32_t flags, size_t leaf,
                                            uint64_t stats[4]) {
  return batch_entry("vimz_decider_verify_batch", ctx, key_words, n_key_words, len_z, n, steps, z0, zi, words, chunk, nullptr, results, seconds, flags, leaf, stats);
}

#ifdef VIMZ_TESTING
extern "C" int vimz_testing_decider_verify_batch_scalars(vimz_ctx* ctx, const uint64_t* key_words, size_t n_key_words, uint32_t len_z, size_t n, const uint64_t* steps, const uint64_t* z0,
                                                         const uint64_t* zi, const uint64_t* words, size_t chunk, const uint64_t* multipliers, uint32_t* results, double seconds[6]) {
  return vimz_testing_decider_verify_batch_scalars_ex(ctx, key_words, n_key_words, len_z, n, steps, z0, zi, words, chunk, multipliers, results, seconds, 0, 0, nullptr);
}
extern "C" int vimz_testing_decider_verify_batch_scalars_ex(vimz_ctx* ctx, const uint64_t* key_words, size_t n_key_words, uint32_t len_z, size_t n, const uint64_t* steps,
                                                            const uint64_t* z0, const uint64_t* zi, const uint64_t* words, size_t chunk, const uint64_t* multipliers,
                                                            uint32_t* results, double seconds[6], uint32_t flags, size_t leaf, uint64_t stats[4]) {
  if (n && !multipliers) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_testing_decider_verify_batch_scalars: NULL multipliers");
  return batch_entry("vimz_testing_decider_verify_batch_scalars", ctx, key_words, n_key_words, len_z, n, steps, z0, zi, words, chunk, multipliers, results, seconds, flags, leaf,
                     stats);
}

extern "C" int vimz_test_miller_loops(vimz_ctx* ctx, const uint64_t* g1_xy, const uint64_t* g2_xy, size_t n, uint32_t* out) {
  if (!ctx || !g1_xy || !g2_xy || !out || !n || n > (1u << 20)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_miller_loops: bad argument");
  if (!vz::pairing::consts().ok) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_miller_loops: pairing constants");
  std::vector<G1A> P(n); std::vector<G2A> Q(n);
  for (size_t i = 0; i < n; i++)
    if (!vz::dv::get_g1(g1_xy + 8 * i, &P[i]) || !vz::dv::get_g2(g2_xy + 16 * i, &Q[i])) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_miller_loops: a coordinate is not below q");
  std::vector<Fq12> f(n);
  {
    std::lock_guard<std::mutex> g(ctx->mu);
    P_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    struct Dev { G1A* p = nullptr; G2A* q = nullptr; Fq12* f = nullptr; ~Dev() { for (void* x : {(void*)p, (void*)q, (void*)f}) if (x) hipFree(x); } } d;
    P_TRY(hipMalloc((void**)&d.p, sizeof(G1A) * n)); P_TRY(hipMalloc((void**)&d.q, sizeof(G2A) * n)); P_TRY(hipMalloc((void**)&d.f, sizeof(Fq12) * n));
    P_TRY(hipMemcpyAsync(d.p, P.data(), sizeof(G1A) * n, hipMemcpyHostToDevice, s)); P_TRY(hipMemcpyAsync(d.q, Q.data(), sizeof(G2A) * n, hipMemcpyHostToDevice, s));
    P_TRY(launch_miller(s, d.p, d.q, n, d.f));
    P_TRY(hipMemcpyAsync(f.data(), d.f, sizeof(Fq12) * n, hipMemcpyDeviceToHost, s));
    P_TRY(hipStreamSynchronize(s));
  }
  static_assert(sizeof(Fq12) == 12 * sizeof(Fq), "an Fq12 is twelve coordinates");
  for (size_t i = 0; i < n; i++) { const Fq* c = (const Fq*)&f[i]; for (int k = 0; k < 12; k++) { const Fq w = Fq::from_mont(c[k]); memcpy(out + 96 * i + 8 * k, w.v, 32); } }
  return VIMZ_OK;
}

extern "C" int vimz_test_g1_lincomb(vimz_ctx* ctx, const uint64_t* a_xy, const uint64_t* k, const uint32_t* bits, const uint64_t* b_xy, size_t n, uint64_t* out_xy) {
  if (!ctx || !a_xy || !k || !bits || !b_xy || !out_xy || !n || n > (1u << 20)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_g1_lincomb: bad argument");
  std::vector<G1A> a(n), b(n), o(n);
  for (size_t i = 0; i < n; i++) {
    if (!vz::dv::get_g1(a_xy + 8 * i, &a[i]) || !vz::dv::get_g1(b_xy + 8 * i, &b[i])) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_g1_lincomb: a coordinate is not below q");
    if (!vz::pairing::g1_on_curve(a[i]) || !vz::pairing::g1_on_curve(b[i])) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_g1_lincomb: a point is off the curve");
    if (bits[i] > 256) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_g1_lincomb: more than 256 bits");
  }
  {
    std::lock_guard<std::mutex> g(ctx->mu);
    P_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    struct Dev { G1A *a = nullptr, *b = nullptr, *o = nullptr; uint32_t *k = nullptr, *bits = nullptr; ~Dev() { for (void* x : {(void*)a, (void*)b, (void*)o, (void*)k, (void*)bits}) if (x) hipFree(x); } } d;
    P_TRY(hipMalloc((void**)&d.a, sizeof(G1A) * n)); P_TRY(hipMalloc((void**)&d.b, sizeof(G1A) * n)); P_TRY(hipMalloc((void**)&d.o, sizeof(G1A) * n));
    P_TRY(hipMalloc((void**)&d.k, 32 * n)); P_TRY(hipMalloc((void**)&d.bits, 4 * n));
    P_TRY(hipMemcpyAsync(d.a, a.data(), sizeof(G1A) * n, hipMemcpyHostToDevice, s)); P_TRY(hipMemcpyAsync(d.b, b.data(), sizeof(G1A) * n, hipMemcpyHostToDevice, s));
    P_TRY(hipMemcpyAsync(d.k, k, 32 * n, hipMemcpyHostToDevice, s)); P_TRY(hipMemcpyAsync(d.bits, bits, 4 * n, hipMemcpyHostToDevice, s));
    P_TRY(launch_lincomb(s, d.a, d.k, d.bits, d.b, n, d.o));
    P_TRY(hipMemcpyAsync(o.data(), d.o, sizeof(G1A) * n, hipMemcpyDeviceToHost, s));
    P_TRY(hipStreamSynchronize(s));
  }
  for (size_t i = 0; i < n; i++) { const Fq x = Fq::from_mont(o[i].x), y = Fq::from_mont(o[i].y); memcpy(out_xy + 8 * i, x.v, 32); memcpy(out_xy + 8 * i + 4, y.v, 32); }
  return VIMZ_OK;
}
#endif
