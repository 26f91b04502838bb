// Packed curve points and packed decider keys (vimz_points_pack / _unpack, vimz_decider_key_pack / _unpack): the encoding, what one thread does
// and the packed key's layout are g16_point_pack.hpp's.
//
// k_points_pack and k_points_unpack, for G1 and G2: PT_BLOCK threads, one thread per point, a thread writes its own output slot and its own 4-byte flag word; no
// atomics, no LDS, nothing another workgroup writes is read, every loop bound is a constant or comes from the host.  The square root's exponent (q + 1)/4 is a
// constant, so the lanes of a wave walk it together: an unpacked G1 point is one exponentiation, a G2 point three (the norm's root, the root's and an inversion).
// Arrays go through the device in chunks of at most VIMZ_PACK_CHUNK points — upload, kernel, download of points and flags, the host scans the flags for the first
// finding as vimz_powers_verify does — so peak device memory is one chunk whatever the array's size.  The host converts nothing: range checks, the change of form and
// the on-curve check when packing are the thread's.  Outputs are collected on the host and written once everything was judged.
// A key: the seven fixed points on the host through the same per-thread functions, IC‖a‖b1‖l‖h as ONE run of G1, b2 as one run of G2.
#include <chrono>
#include "g16_powers.hpp"
#include "g16_point_pack.hpp"
#ifdef VIMZ_TESTING
#include "../../include/vimz_hip_testing.h"
#endif

namespace {

using namespace vz::keyc;
static_assert(VIMZ_PACK_CHUNK <= (1u << 24), "a chunk's grid is a 32-bit count of blocks");

// thread i is point i (g16_point_pack.hpp: pt_pack, pt_unpack): it writes packed[i] / points[i] and flags[i] alone
template <class F>
__global__ void __launch_bounds__(PT_BLOCK) k_points_pack(const Affine<F>* __restrict__ points, size_t n, int mont, F b, uint32_t* __restrict__ packed, uint32_t* __restrict__ flags) {
  const size_t i = blockIdx.x * (size_t)PT_BLOCK + threadIdx.x;
  if (i < n) pt_pack(i, points, mont != 0, b, packed, flags);
}
template <class F>
__global__ void __launch_bounds__(PT_BLOCK) k_points_unpack(const uint32_t* __restrict__ packed, size_t n, F b, int mont, Affine<F>* __restrict__ points, uint32_t* __restrict__ flags) {
  const size_t i = blockIdx.x * (size_t)PT_BLOCK + threadIdx.x;
  if (i < n) pt_unpack(i, packed, b, mont != 0, points, flags);
}

unsigned pk_blocks(size_t threads) { return (unsigned)((threads + PT_BLOCK - 1) / PT_BLOCK); }
double pk_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
Fq pk_curve_b(const Fq*) { return vz::pairing::fq_u64(3); }
Fq2 pk_curve_b(const Fq2*) { return vz::pairing::consts().twist_b; }
bool pk_overlap(const void* a, size_t na, const void* b, size_t nb) { return (const char*)a < (const char*)b + nb && (const char*)b < (const char*)a + na; }

// one chunk's buffers: the unpacked points, the packed ones, the flags
struct PackDev {
  void *points = nullptr, *packed = nullptr; uint32_t* flags = nullptr;
  ~PackDev() { for (void* p : {points, packed, (void*)flags}) if (p) hipFree(p); }
};
// room for chunks of either group, for runs of up to n1 points of G1 and n2 of G2.  The caller holds the context's lock and has set the device.
int pack_dev_alloc(vimz_ctx* ctx, PackDev& d, size_t n1, size_t n2) {
  const size_t c1 = std::min<size_t>(n1, VIMZ_PACK_CHUNK), c2 = std::min<size_t>(n2, VIMZ_PACK_CHUNK), pts = std::max(64 * c1, 128 * c2);
  if (!pts) return VIMZ_OK;
  P_TRY(hipMalloc(&d.points, pts)); P_TRY(hipMalloc(&d.packed, pts / 2)); P_TRY(hipMalloc((void**)&d.flags, 4 * std::max(c1, c2)));
  return VIMZ_OK;
}

// A run of n points of F's group, chunk by chunk, from `in` to `out` (host; a point is 2·sizeof(F) bytes, a packed one sizeof(F)).  *bits = 0, or the findings of
// the first point that has one, its index in *first; the run stops at that chunk.
template <class F>
int pack_run(vimz_ctx* ctx, PackDev& d, bool packing, const uint64_t* in, size_t n, bool mont, uint64_t* out, uint32_t* bits, size_t* first) {
  hipStream_t s = ctx->stream;
  const size_t pt = 2 * sizeof(F), pk = sizeof(F), in_b = packing ? pt : pk, out_b = packing ? pk : pt;
  const F b = pk_curve_b((const F*)nullptr);
  std::vector<uint32_t> flags(std::min<size_t>(n, VIMZ_PACK_CHUNK));
  *bits = 0; *first = 0;
  for (size_t lo = 0; lo < n; lo += VIMZ_PACK_CHUNK) {
    const size_t c = std::min<size_t>(n - lo, VIMZ_PACK_CHUNK);
    void *d_in = packing ? d.points : d.packed, *d_out = packing ? d.packed : d.points;
    P_TRY(hipMemcpyAsync(d_in, (const char*)in + in_b * lo, in_b * c, hipMemcpyHostToDevice, s));
    if (packing) hipLaunchKernelGGL(k_points_pack<F>, dim3(pk_blocks(c)), dim3(PT_BLOCK), 0, s, (const Affine<F>*)d.points, c, (int)mont, b, (uint32_t*)d.packed, d.flags);
    else hipLaunchKernelGGL(k_points_unpack<F>, dim3(pk_blocks(c)), dim3(PT_BLOCK), 0, s, (const uint32_t*)d.packed, c, b, (int)mont, (Affine<F>*)d.points, d.flags);
    P_TRY(hipGetLastError());
    P_TRY(hipMemcpyAsync((char*)out + out_b * lo, d_out, out_b * c, hipMemcpyDeviceToHost, s));
    P_TRY(hipMemcpyAsync(flags.data(), d.flags, 4 * c, hipMemcpyDeviceToHost, s));
    P_TRY(hipStreamSynchronize(s));
    for (size_t i = 0; i < c; i++) if (flags[i]) { *bits = flags[i]; *first = lo + i; return VIMZ_OK; }
  }
  return VIMZ_OK;
}

int points_call(vimz_ctx* ctx, const char* who, bool packing, int group, const uint64_t* in, size_t n, int form, uint64_t* out, uint32_t* result, uint64_t* first_bad, double seconds[2]) {
  auto bad = [&](const char* m) { return vz_fail(ctx, VIMZ_ERR_INVALID, (std::string(who) + ": " + m).c_str()); };
  if (!ctx) return VIMZ_ERR_INVALID;
  if (!in || !out || !result || !first_bad) return bad("NULL argument");
  if (group != 1 && group != 2) return bad("group is 1 (G1) or 2 (G2)");
  if (form != VIMZ_FORM_CANONICAL && form != VIMZ_FORM_MONTGOMERY) return bad("form is VIMZ_FORM_*");
  if (n > ((size_t)1 << 32)) return bad("too many points");
  if (group == 2 && !vz::pairing::consts().ok) return bad("pairing constants");
  const auto t_all = std::chrono::steady_clock::now();
  const size_t pk = group == 1 ? 32 : 64, in_b = (packing ? 2 * pk : pk) * n, out_b = (packing ? pk : 2 * pk) * n;
  if (n && !(packing && (const void*)in == (const void*)out) && pk_overlap(in, in_b, out, out_b)) return bad("the output overlaps the input");
  *result = 0; *first_bad = 0;
  double t_device = 0;
  if (n) {
    std::vector<uint64_t> tmp(out_b / 8);
    uint32_t bits = 0; size_t first = 0;
    const auto t_dev = std::chrono::steady_clock::now();
    { std::lock_guard<std::mutex> g(ctx->mu);
      P_TRY(hipSetDevice(ctx->device));
      PackDev d;
      int rc = pack_dev_alloc(ctx, d, group == 1 ? n : 0, group == 2 ? n : 0);
      if (!rc) rc = group == 1 ? pack_run<Fq>(ctx, d, packing, in, n, form == VIMZ_FORM_MONTGOMERY, tmp.data(), &bits, &first)
                               : pack_run<Fq2>(ctx, d, packing, in, n, form == VIMZ_FORM_MONTGOMERY, tmp.data(), &bits, &first);
      if (rc) return rc; }
    t_device = pk_since(t_dev);
    if (bits) { *result = bits; *first_bad = first; }
    else memcpy(out, tmp.data(), out_b);
  }
  if (seconds) { seconds[1] = t_device; seconds[0] = pk_since(t_all) - t_device; }
  return VIMZ_OK;
}

// the seven fixed points of a key, in words of the key and of the packed key: {group, key offset, packed offset}
struct FixedPoint { int group; size_t off, poff; };
const FixedPoint FIXED[7] = {{2, KEY_KZG, PKEY_KZG},          {1, KEY_ALPHA1, PKEY_ALPHA1},     {1, KEY_ALPHA1 + 8, PKEY_ALPHA1 + 4}, {1, KEY_ALPHA1 + 16, PKEY_ALPHA1 + 8},
                             {2, KEY_BETA2, PKEY_BETA2},      {2, KEY_BETA2 + 16, PKEY_BETA2 + 8}, {2, KEY_BETA2 + 32, PKEY_BETA2 + 16}};
static_assert(KEY_ALPHA1 + 16 == KEY_DELTA1 && KEY_BETA2 + 32 == KEY_DELTA2 && KEY_DELTA2 + 16 == KEY_IC && PKEY_BETA2 + 24 == PKEY_IC, "one layout");

int64_t key_call(vimz_ctx* ctx, const char* who, bool packing, const void* in, size_t len, void* out, size_t cap, uint32_t* result, uint64_t first_bad[2]) {
  auto bad = [&](const char* m) { return (int64_t)vz_fail(ctx, VIMZ_ERR_INVALID, (std::string(who) + ": " + m).c_str()); };
  if (!ctx) return VIMZ_ERR_INVALID;
  if (!in || !result || !first_bad) return bad("NULL argument");
  KeyRuns R;
  if (const char* why = packing ? plain_key_runs(in, len, &R) : packed_key_layout(in, len, &R)) return bad(why);
  if (!vz::pairing::consts().ok) return bad("pairing constants");
  const size_t out_words = packing ? R.pwords : R.words, size = 8 * out_words;
  if (!out || cap < size) return (int64_t)size;
  if (in != out && pk_overlap(in, len, out, size)) return bad("the output overlaps the input");
  *result = 0; first_bad[0] = first_bad[1] = 0;
  const uint64_t* w = (const uint64_t*)in;
  std::vector<uint64_t> tmp(out_words);
  uint64_t* o = tmp.data();
  auto verdict = [&](uint32_t bits, size_t word) { *result = bits; first_bad[0] = word; first_bad[1] = bits; return (int64_t)size; };
  o[0] = packing ? PACKED_KEY_MAGIC : KEY_MAGIC;
  memcpy(o + 1, w + 1, 8 * (KEY_HEAD_WORDS - 1));
  const Fq b1 = pk_curve_b((const Fq*)nullptr); const Fq2 b2 = pk_curve_b((const Fq2*)nullptr);
  for (const FixedPoint& p : FIXED) {
    uint32_t f = 0;
    const size_t src = packing ? p.off : p.poff, dst = packing ? p.poff : p.off;
    if (packing) { if (p.group == 1) pt_pack(0, (const Affine<Fq>*)(w + src), false, b1, (uint32_t*)(o + dst), &f); else pt_pack(0, (const Affine<Fq2>*)(w + src), false, b2, (uint32_t*)(o + dst), &f); }
    else { if (p.group == 1) pt_unpack(0, (const uint32_t*)(w + src), b1, false, (Affine<Fq>*)(o + dst), &f); else pt_unpack(0, (const uint32_t*)(w + src), b2, false, (Affine<Fq2>*)(o + dst), &f); }
    if (f) return verdict(f, src);
  }
  { std::lock_guard<std::mutex> g(ctx->mu);
    P_TRY(hipSetDevice(ctx->device));
    PackDev d;
    uint32_t bits = 0; size_t first = 0;
    int rc = pack_dev_alloc(ctx, d, R.n_g1, R.n_g2);
    if (rc) return rc;
    const size_t s1 = packing ? R.off_g1 : R.poff_g1, d1 = packing ? R.poff_g1 : R.off_g1, s2 = packing ? R.off_g2 : R.poff_g2, d2 = packing ? R.poff_g2 : R.off_g2;
    if ((rc = pack_run<Fq>(ctx, d, packing, w + s1, R.n_g1, false, o + d1, &bits, &first))) return rc;
    if (bits) return verdict(bits, s1 + (packing ? 8 : 4) * first);
    if ((rc = pack_run<Fq2>(ctx, d, packing, w + s2, R.n_g2, false, o + d2, &bits, &first))) return rc;
    if (bits) return verdict(bits, s2 + (packing ? 16 : 8) * first); }
  memmove(out, o, size);
  return (int64_t)size;
}

}  // namespace

extern "C" int vimz_points_pack(vimz_ctx* ctx, int group, const uint64_t* points, size_t n, int form, uint64_t* packed_out, uint32_t* result, uint64_t* first_bad, double seconds[2]) {
  return points_call(ctx, "vimz_points_pack", true, group, points, n, form, packed_out, result, first_bad, seconds);
}
extern "C" int vimz_points_unpack(vimz_ctx* ctx, int group, const uint64_t* packed, size_t n, int form, uint64_t* points_out, uint32_t* result, uint64_t* first_bad, double seconds[2]) {
  return points_call(ctx, "vimz_points_unpack", false, group, packed, n, form, points_out, result, first_bad, seconds);
}
extern "C" int64_t vimz_decider_key_pack(vimz_ctx* ctx, const void* key, size_t len, void* out, size_t cap, uint32_t* result, uint64_t first_bad[2]) {
  return key_call(ctx, "vimz_decider_key_pack", true, key, len, out, cap, result, first_bad);
}
extern "C" int64_t vimz_decider_key_unpack(vimz_ctx* ctx, const void* packed, size_t len, void* out, size_t cap, uint32_t* result, uint64_t first_bad[2]) {
  return key_call(ctx, "vimz_decider_key_unpack", false, packed, len, out, cap, result, first_bad);
}

#ifdef VIMZ_TESTING
namespace {
// thread i takes the root of values[i] (Montgomery in, Montgomery out) and says whether it is one
__global__ void __launch_bounds__(PT_BLOCK) k_test_fq2_sqrt(const Fq2* __restrict__ values, size_t n, Fq2* __restrict__ roots, uint32_t* __restrict__ is_square) {
  const size_t i = blockIdx.x * (size_t)PT_BLOCK + threadIdx.x;
  if (i >= n) return;
  Fq2 r;
  is_square[i] = vz::pack::fq2_sqrt(values[i], &r) ? 1u : 0u;
  roots[i] = r;
}
}  // namespace

extern "C" int vimz_test_fq2_sqrt(vimz_ctx* ctx, const uint64_t* values, size_t n, uint64_t* roots_out, uint32_t* is_square_out) {
  if (!ctx) return VIMZ_ERR_INVALID;
  if (!values || !roots_out || !is_square_out || !n || n > VIMZ_PACK_CHUNK) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_fq2_sqrt: bad argument");
  std::vector<Fq2> v(n);
  for (size_t i = 0; i < n; i++) {
    Fq* c = (Fq*)&v[i];
    for (int k = 0; k < 2; k++) {
      Fq x; memcpy(x.v, values + 8 * i + 4 * k, 32);
      if (!x.is_reduced()) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_fq2_sqrt: a coordinate is not below q");
      c[k] = Fq::to_mont(x);
    }
  }
  { std::lock_guard<std::mutex> g(ctx->mu);
    P_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    PackDev d;
    P_TRY(hipMalloc(&d.points, sizeof(Fq2) * n)); P_TRY(hipMalloc(&d.packed, sizeof(Fq2) * n)); P_TRY(hipMalloc((void**)&d.flags, 4 * n));
    P_TRY(hipMemcpyAsync(d.points, v.data(), sizeof(Fq2) * n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_test_fq2_sqrt, dim3(pk_blocks(n)), dim3(PT_BLOCK), 0, s, (const Fq2*)d.points, n, (Fq2*)d.packed, d.flags);
    P_TRY(hipGetLastError());
    P_TRY(hipMemcpyAsync(v.data(), d.packed, sizeof(Fq2) * n, hipMemcpyDeviceToHost, s));
    P_TRY(hipMemcpyAsync(is_square_out, d.flags, 4 * n, hipMemcpyDeviceToHost, s));
    P_TRY(hipStreamSynchronize(s)); }
  for (size_t i = 0; i < n; i++) {
    const Fq* c = (const Fq*)&v[i];
    for (int k = 0; k < 2; k++) { const Fq x = Fq::from_mont(c[k]); memcpy(roots_out + 8 * i + 4 * k, x.v, 32); }
  }
  return VIMZ_OK;
}
#endif
