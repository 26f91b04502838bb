// C ABI (include/vimz_hip.h) over the gfx950 kernels.  One translation unit: the kernels are templates
// over the four curves / fields and are instantiated from here.
#include <hip/hip_runtime.h>
#include <mutex>
#include <new>
#include <string>
#include <cstring>
#include <cstdio>

#include "internal.hpp"
#define HIP_TRY(c, x) do { hipError_t _e = (x); if (_e != hipSuccess) return vz::vz_fail(c, VIMZ_ERR_HIP, #x, _e); } while (0)
#include "vecops_api.hpp"
#include "ckgen.hpp"

using namespace vz;

static thread_local std::string g_err_noctx;

namespace vz {
int vz_fail(vimz_ctx* c, int code, const char* what, hipError_t e) {
  std::string m = what;
  if (e != hipSuccess) { m += ": "; m += hipGetErrorString(e); }
  static std::mutex err_mu;          // (host threads of one call may fail side by side: vimz_*_verify_compressed_batch's per-proof pass)
  std::lock_guard<std::mutex> g(err_mu);
  if (c) c->err = m; else g_err_noctx = m;
  return code;
}
}  // namespace vz
static int fail(vimz_ctx* c, int code, const char* what, hipError_t e = hipSuccess) { return vz::vz_fail(c, code, what, e); }

namespace vz {
int vz_ensure_scratch(vimz_ctx* c, size_t bytes) {
  if (bytes <= c->scratch_bytes) return VIMZ_OK;
  if (c->scratch) hipFree(c->scratch);
  c->scratch = nullptr; c->scratch_bytes = 0;
  HIP_TRY(c, hipMalloc(&c->scratch, bytes));
  c->scratch_bytes = bytes;
  return VIMZ_OK;
}
}  // namespace vz
static int ensure_scratch(vimz_ctx* c, size_t bytes) { return vz::vz_ensure_scratch(c, bytes); }

template <class Fn>
static int field_dispatch(int field, Fn fn) {
  switch (field) {
    case VIMZ_FIELD_BN254_FR: return fn(Fp<BnFr>());
    case VIMZ_FIELD_BN254_FQ: return fn(Fp<BnFq>());
    case VIMZ_FIELD_PALLAS_FP: return fn(Fp<PallasFp>());
    case VIMZ_FIELD_VESTA_FQ: return fn(Fp<VestaFq>());
  }
  return VIMZ_ERR_INVALID;
}
template <class Fn>
static int curve_dispatch(int curve, Fn fn) {
  switch (curve) {
    case VIMZ_CURVE_BN254_G1: return fn(BnG1());
    case VIMZ_CURVE_GRUMPKIN: return fn(Grumpkin());
    case VIMZ_CURVE_PALLAS: return fn(Pallas());
    case VIMZ_CURVE_VESTA: return fn(Vesta());
  }
  return VIMZ_ERR_INVALID;
}
static int curve_base_field(int curve) {
  switch (curve) {
    case VIMZ_CURVE_BN254_G1: return VIMZ_FIELD_BN254_FQ;
    case VIMZ_CURVE_GRUMPKIN: return VIMZ_FIELD_BN254_FR;
    case VIMZ_CURVE_PALLAS: return VIMZ_FIELD_PALLAS_FP;
    default: return VIMZ_FIELD_VESTA_FQ;
  }
}
static int curve_scalar_field(int curve) {
  switch (curve) {
    case VIMZ_CURVE_BN254_G1: return VIMZ_FIELD_BN254_FR;
    case VIMZ_CURVE_GRUMPKIN: return VIMZ_FIELD_BN254_FQ;
    case VIMZ_CURVE_PALLAS: return VIMZ_FIELD_VESTA_FQ;
    default: return VIMZ_FIELD_PALLAS_FP;
  }
}

namespace vz {
int vz_msm_device(vimz_ctx* c, const vimz_bases* bases, size_t base_offset, const uint32_t* d_scalars, size_t n,
                      int scalars_mont, int window_bits, uint64_t out_xy[8], int out_form, int split_ones) {
  return curve_dispatch(bases->curve, [&](auto cv) {
    typedef decltype(cv) C;
    typedef typename C::Base F;
    Affine<F> r;
    BaseTables tb = bases->tb(base_offset);
    bool have_tb = bases->tables != nullptr;
    if (n <= MSM_SMALL_MAX && window_bits <= 0 && !split_ones) {      // a fixed slice with small-MSM tables (vimz_bases_precompute(7), or an IVC's slices)
      vimz_bases* bm = const_cast<vimz_bases*>(bases);
      std::lock_guard<std::mutex> g(bm->small_mu);
      for (auto& t : bm->small)
        if (t.offset <= base_offset && base_offset + n <= t.offset + t.n) { tb = BaseTables{t.rows, t.n, base_offset - t.offset, t.c, t.K, 0, t.mult}; have_tb = true; break; }
    }
    hipError_t e = msm_run<C>(c->stream, c->msm_ws, bases->d + (size_t)AFFINE_WORDS * base_offset, d_scalars, n, scalars_mont, window_bits, &r,
                              &c->last_msm, c->profiling ? c->ev : nullptr, split_ones, have_tb ? &tb : nullptr);
    if (e != hipSuccess) return vz_fail(c, VIMZ_ERR_HIP, "msm", e);
    if (c->profiling && n) {
      for (int i = 0; i < 6; i++) c->msm_tot_ms[i] += c->last_msm.ms[i];
      c->msm_tot_calls++; c->msm_tot_points += n; c->msm_tot_entries += c->last_msm.entries;
    }
    if (out_form == VIMZ_FORM_CANONICAL) { r.x = F::from_mont(r.x); r.y = F::from_mont(r.y); }
    memcpy(out_xy, r.x.v, 32); memcpy(out_xy + 4, r.y.v, 32);
    return VIMZ_OK;
  });
}

// core of vimz_kzg_open on a device-resident vector of Montgomery elements (caller holds c->mu and has set the device)
int vz_kzg_open_device(vimz_ctx* c, const vimz_bases* srs, size_t base_offset, int field, const uint32_t* d_vec, size_t n, const uint64_t z[4], int form,
                       uint64_t eval_out[4], uint64_t proof_xy[8]) {
  if (n == 0 || base_offset + n > srs->n) return vz_fail(c, VIMZ_ERR_INVALID, "kzg open: the SRS is shorter than the vector");
  std::vector<uint32_t> host(8 * n);
  hipError_t e;
  if ((e = hipMemcpyAsync(host.data(), d_vec, 32 * n, hipMemcpyDeviceToHost, c->stream)) != hipSuccess || (e = hipStreamSynchronize(c->stream)) != hipSuccess)
    return vz_fail(c, VIMZ_ERR_HIP, "kzg open: download", e);
  int rc = field_dispatch(field, [&](auto f) {
    typedef decltype(f) F;
    F zz; memcpy(zz.v, z, 32);
    if (!zz.is_reduced()) return vz_fail(c, VIMZ_ERR_INVALID, "kzg open: z not below the modulus");
    if (form == VIMZ_FORM_CANONICAL) zz = F::to_mont(zz);
    F* a = reinterpret_cast<F*>(host.data());       // Montgomery, as resident
    F carry = F::zero();                              // q_i, walking down; the last carry is p(z)
    for (size_t i = n; i-- > 0;) { const F cur = F::add(a[i], F::mul(zz, carry)); a[i] = carry; carry = cur; }      // a[i] <- q_i  (q_{n-1} = 0)
    const F ev = form == VIMZ_FORM_CANONICAL ? F::from_mont(carry) : carry;
    memcpy(eval_out, ev.v, 32);
    return VIMZ_OK;
  });
  if (rc) return rc;
  if (n == 1) { memset(proof_xy, 0, 64); return VIMZ_OK; }      // a constant: the quotient is zero, its commitment the identity
  rc = vz_ensure_scratch(c, 32 * (n - 1)); if (rc) return rc;
  if ((e = hipMemcpyAsync(c->scratch, host.data(), 32 * (n - 1), hipMemcpyHostToDevice, c->stream)) != hipSuccess) return vz_fail(c, VIMZ_ERR_HIP, "kzg open: upload", e);
  return vz_msm_device(c, srs, base_offset, (const uint32_t*)c->scratch, n - 1, 1, 0, proof_xy, form);
}
int vz_small_tables(vimz_ctx* c, vimz_bases* b, size_t offset, size_t n, bool with_mult, BaseTables* out) {
  *out = BaseTables{nullptr, 0, 0, 0, 0};
  if (!n || n > MSM_SMALL_MAX || offset + n > b->n) return VIMZ_OK;
  std::lock_guard<std::mutex> g(b->small_mu);
  vimz_small_tables* t = nullptr;
  for (auto& e : b->small) if (e.offset == offset && e.n == n) t = &e;
  return curve_dispatch(b->curve, [&](auto cv) {
    typedef decltype(cv) C;
    const int K = (C::Scalar::Params::BITS + SMALL_C) / SMALL_C;
    hipError_t e = hipSuccess;
    if (!t) {
      vimz_small_tables nt; nt.offset = offset; nt.n = n; nt.c = SMALL_C; nt.K = K;
      if ((e = hipMalloc((void**)&nt.rows, 4 * (size_t)AFFINE_WORDS * n * K)) != hipSuccess) return vz_fail(c, VIMZ_ERR_HIP, "small-MSM window tables", e);
      if ((e = build_tables<C>(c->stream, b->d + (size_t)AFFINE_WORDS * offset, n, SMALL_C, K, nt.rows)) != hipSuccess) { hipFree(nt.rows); return vz_fail(c, VIMZ_ERR_HIP, "small-MSM window tables", e); }
      b->small.push_back(nt);
      t = &b->small.back();
    }
    if (with_mult && !t->mult) {
      const size_t nm = (size_t)1 << (SMALL_C - 1);
      if ((e = hipMalloc((void**)&t->mult, 4 * (size_t)AFFINE_WORDS * n * K * nm)) != hipSuccess) return vz_fail(c, VIMZ_ERR_HIP, "small-MSM multiples tables (1.5 GB per 7.7 k points)", e);
      if ((e = build_multiples<C>(c->stream, t->rows, n, SMALL_C, K, t->mult)) != hipSuccess) { hipFree(t->mult); t->mult = nullptr; return vz_fail(c, VIMZ_ERR_HIP, "small-MSM multiples tables", e); }
    }
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return vz_fail(c, VIMZ_ERR_HIP, "small-MSM tables", e);
    out->d = t->rows; out->n_total = n; out->offset = 0; out->c = SMALL_C; out->K = K; out->mult = with_mult ? t->mult : nullptr;
    return VIMZ_OK;
  });
}
}  // namespace vz
static int msm_device(vimz_ctx* c, const vimz_bases* bases, size_t base_offset, const uint32_t* d_scalars, size_t n,
                      int scalars_mont, int window_bits, uint64_t out_xy[8], int out_form) {
  return vz::vz_msm_device(c, bases, base_offset, d_scalars, n, scalars_mont, window_bits, out_xy, out_form);
}

// Input pipeline: packing of pixels into field elements on the device — ten pixels per element, pixel k in
// bits [24k, 24k + 24) with R in the low byte (a grey value alone in the low byte), rows padded with zero pixels: what
// pyvimz/pyvimz/img/ops.py:4-33 (compress_by_rows) and :36-70 (compress_by_blocks, 40 x 40 blocks -> 160 elements) produce as hex
// strings.  One thread per packed element; the output is canonical little-endian limbs, i.e. the 30 pixel bytes followed by two zeros.
static __global__ void __launch_bounds__(256) k_pack_pixels(const uint8_t* __restrict__ px, uint32_t h, uint32_t w, uint32_t ch, uint32_t block,
                                                            uint32_t n_out, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_out) return;
  uint32_t row, col0, run;       // first pixel of this element and how many pixels of the row / block row are left
  if (!block) {
    const uint32_t per = (w + 9) / 10;
    row = i / per; col0 = (i % per) * 10; run = w - col0;
  } else {
    const uint32_t bw = (w + block - 1) / block, per_row = (block + 9) / 10, per_blk = block * per_row;
    const uint32_t b = i / per_blk, e = i % per_blk, br = b / bw, bc = b % bw, r = e / per_row, c = e % per_row;
    row = br * block + r; col0 = bc * block + c * 10;
    const uint32_t end = min(w, (bc + 1) * block);
    run = row < h && col0 < end ? end - col0 : 0;
  }
  uint32_t words[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const uint32_t np = run < 10 ? run : 10;
  for (uint32_t k = 0; k < np; k++)
    for (uint32_t c = 0; c < 3; c++) {
      const uint32_t v = c < ch ? px[((size_t)row * w + col0 + k) * ch + c] : 0u;
      const uint32_t byte = 3 * k + c;
      words[byte >> 2] |= v << (8 * (byte & 3));
    }
  uint4* o = reinterpret_cast<uint4*>(out + 8 * (size_t)i);
  o[0] = make_uint4(words[0], words[1], words[2], words[3]);
  o[1] = make_uint4(words[4], words[5], words[6], words[7]);
}

extern "C" {

const char* vimz_version(void) { return "vimz-hip 0.1 (gfx950)"; }

int vimz_ctx_create(int device, vimz_ctx** out) {
  if (!out) return fail(nullptr, VIMZ_ERR_INVALID, "out is NULL");
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count == 0) return fail(nullptr, VIMZ_ERR_NO_DEVICE, "no HIP device visible", e);
  if (device < 0 || device >= count) return fail(nullptr, VIMZ_ERR_INVALID, "device index out of range");
  vimz_ctx* c = new (std::nothrow) vimz_ctx();
  if (!c) return fail(nullptr, VIMZ_ERR_INVALID, "out of host memory");
  c->device = device;
  // the context's stream carries the latency-critical sequential chain of a fold: give it the highest priority so the
  // batch producer (a second stream inside the prover) cannot delay it
  int prio_lo = 0, prio_hi = 0;
  hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
  if ((e = hipSetDevice(device)) != hipSuccess || (e = hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio_hi)) != hipSuccess ||
      (e = hipEventCreate(&c->t0)) != hipSuccess || (e = hipEventCreate(&c->t1)) != hipSuccess) {
    delete c; return fail(nullptr, VIMZ_ERR_HIP, "context setup", e);
  }
  for (int i = 0; i < 7; i++) if ((e = hipEventCreate(&c->ev[i])) != hipSuccess) { delete c; return fail(nullptr, VIMZ_ERR_HIP, "event", e); }
  *out = c;
  return VIMZ_OK;
}

void vimz_ctx_destroy(vimz_ctx* c) {
  if (!c) return;
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  c->msm_ws.release();
  if (c->scratch) hipFree(c->scratch);
  if (c->image_hash_tables) hipFree(c->image_hash_tables);
  if (c->image_hash_buf) hipFree(c->image_hash_buf);
  for (void* p : c->image_hash_retired) hipFree(p);
  if (c->image_edit_buf) hipFree(c->image_edit_buf);
  for (void* p : c->image_edit_retired) hipFree(p);
  for (int i = 0; i < 7; i++) if (c->ev[i]) hipEventDestroy(c->ev[i]);
  hipEventDestroy(c->t0); hipEventDestroy(c->t1);
  for (auto& ps : c->spare_streams) hipStreamDestroy(ps.second);
  hipStreamDestroy(c->stream);
  delete c;
}

const char* vimz_last_error(const vimz_ctx* c) { return c ? c->err.c_str() : g_err_noctx.c_str(); }

int vimz_device_info(vimz_ctx* c, char* name, size_t name_len, int* cus, uint64_t* hbm_bytes) {
  if (!c) return VIMZ_ERR_INVALID;
  hipDeviceProp_t p;
  HIP_TRY(c, hipGetDeviceProperties(&p, c->device));
  if (name && name_len) { snprintf(name, name_len, "%s (%s)", p.name, p.gcnArchName); }
  if (cus) *cus = p.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = p.totalGlobalMem;
  return VIMZ_OK;
}

size_t vimz_pack_count(size_t height, size_t width, int block) {
  if (!block) return height * ((width + 9) / 10);
  const size_t b = (size_t)block;
  return ((height + b - 1) / b) * ((width + b - 1) / b) * b * ((b + 9) / 10);
}
int vimz_pack_pixels(vimz_ctx* c, const uint8_t* pixels, size_t height, size_t width, int channels, int block, uint64_t* out) {
  // (each dimension is bounded before anything is multiplied: the kernel indexes with 32-bit products)
  if (!c || !pixels || !out || !height || !width || (channels != 1 && channels != 3) || block < 0 || block > 4096 || height > (1ull << 20) || width > (1ull << 20) ||
      height * width > (1ull << 30))
    return fail(c, VIMZ_ERR_INVALID, "vimz_pack_pixels: bad argument (at most 2^20 per dimension, 2^30 pixels, blocks of at most 4096)");
  const size_t n = vimz_pack_count(height, width, block), in_bytes = height * width * (size_t)channels;
  if (n >= (1ull << 31)) return fail(c, VIMZ_ERR_INVALID, "vimz_pack_pixels: output too large");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  int rc = ensure_scratch(c, 32 * n + in_bytes + 64);
  if (rc) return rc;
  uint8_t* d_in = (uint8_t*)c->scratch + 32 * n;
  HIP_TRY(c, hipMemcpyAsync(d_in, pixels, in_bytes, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_pack_pixels, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t*)d_in, (uint32_t)height, (uint32_t)width,
                     (uint32_t)channels, (uint32_t)block, (uint32_t)n, (uint32_t*)c->scratch);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(out, c->scratch, 32 * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VIMZ_OK;
}

int vimz_sync(vimz_ctx* c) {
  if (!c) return VIMZ_ERR_INVALID;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VIMZ_OK;
}

// A marker in a profiler's kernel trace: an empty kernel named k_trace_marker with `id` workgroups on the context's stream, waited for.
// bench.py brackets its timed region with markers 1 and 2 so that tools/trace_busy.py measures the fold itself, not the set-up,
// the compression and the extras around it.
namespace vz { __global__ void k_trace_marker() {} }
int vimz_trace_marker(vimz_ctx* c, int id) {
  if (!c || id < 1 || id > 1024) return VIMZ_ERR_INVALID;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(vz::k_trace_marker, dim3((unsigned)id), dim3(64), 0, c->stream);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VIMZ_OK;
}

int vimz_timer_start(vimz_ctx* c) {
  if (!c) return VIMZ_ERR_INVALID;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipEventRecord(c->t0, c->stream));
  return VIMZ_OK;
}
int vimz_timer_stop(vimz_ctx* c, float* ms) {
  if (!c || !ms) return VIMZ_ERR_INVALID;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipEventRecord(c->t1, c->stream));
  HIP_TRY(c, hipEventSynchronize(c->t1));
  HIP_TRY(c, hipEventElapsedTime(ms, c->t0, c->t1));
  return VIMZ_OK;
}
int vimz_set_profiling(vimz_ctx* c, int enabled) { if (!c) return VIMZ_ERR_INVALID; c->profiling = enabled != 0; return VIMZ_OK; }
int vimz_msm_last_profile(vimz_ctx* c, float ms[6], uint32_t info[4]) {
  if (!c) return VIMZ_ERR_INVALID;
  if (ms) memcpy(ms, c->last_msm.ms, sizeof(float) * 6);
  if (info) { info[0] = c->last_msm.c; info[1] = c->last_msm.K; info[2] = c->last_msm.subs; info[3] = c->last_msm.entries; }
  return VIMZ_OK;
}

int vimz_msm_profile_totals(vimz_ctx* c, double ms[6], uint64_t counts[3], int reset) {
  if (!c) return VIMZ_ERR_INVALID;
  std::lock_guard<std::mutex> g(c->mu);
  if (ms) memcpy(ms, c->msm_tot_ms, sizeof(double) * 6);
  if (counts) { counts[0] = c->msm_tot_calls; counts[1] = c->msm_tot_points; counts[2] = c->msm_tot_entries; }
  if (reset) { memset(c->msm_tot_ms, 0, sizeof(c->msm_tot_ms)); c->msm_tot_calls = c->msm_tot_points = c->msm_tot_entries = 0; }
  return VIMZ_OK;
}

// ---- commitment key ----------------------------------------------------------------------------------
int vimz_bases_upload(vimz_ctx* c, int curve, const uint64_t* xy, size_t n, int form, vimz_bases** out) {
  if (!c || !out || (!xy && n) || curve < 0 || curve > 3) return fail(c, VIMZ_ERR_INVALID, "vimz_bases_upload: bad argument");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  vimz_bases* b = new vimz_bases(); b->curve = curve; b->n = n; b->d = nullptr;
  if (n) {
    int rc = ensure_scratch(c, 64 * n); if (rc) { delete b; return rc; }
    hipError_t e = hipMalloc(&b->d, 4 * (size_t)AFFINE_WORDS * n);
    if (e != hipSuccess) { delete b; return fail(c, VIMZ_ERR_HIP, "hipMalloc(bases)", e); }
    e = hipMemcpyAsync(c->scratch, xy, 64 * n, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) { hipFree(b->d); delete b; return fail(c, VIMZ_ERR_HIP, "copy bases", e); }
    // resident form: 9 x 29-bit Montgomery coordinates (fp29.hpp)
    field_dispatch(curve_base_field(curve), [&](auto f) { typedef decltype(f) F; launch_points_to_internal<F>(c->stream, (const uint32_t*)c->scratch, form == VIMZ_FORM_CANONICAL, b->d, n); return VIMZ_OK; });
    e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { hipFree(b->d); delete b; return fail(c, VIMZ_ERR_HIP, "bases sync", e); }
  }
  *out = b;
  return VIMZ_OK;
}
int vimz_bases_generate(vimz_ctx* c, int curve, const char* label, size_t label_len, size_t n, vimz_bases** out) {
  if (!c || !out || (!label && label_len) || label_len > 64 || curve < 0 || curve > 3) return fail(c, VIMZ_ERR_INVALID, "vimz_bases_generate: bad argument");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  vimz_bases* b = new vimz_bases(); b->curve = curve; b->n = n; b->d = nullptr;
  if (n) {
    int rcs = ensure_scratch(c, 64 * n); if (rcs) { delete b; return rcs; }
    hipError_t e = hipMalloc(&b->d, 4 * (size_t)AFFINE_WORDS * n);
    if (e != hipSuccess) { delete b; return fail(c, VIMZ_ERR_HIP, "hipMalloc(bases)", e); }
    CkLabel L; memset(&L, 0, sizeof(L)); memcpy(L.bytes, label, label_len); L.len = (int)label_len;
    static const int B_COEF[4] = {3, -17, 5, 5};
    int rc = field_dispatch(curve_base_field(curve), [&](auto f) {
      typedef decltype(f) F;
      hipError_t e2 = ckgen_run<F>(c->stream, L, B_COEF[curve], 0, n, (uint32_t*)c->scratch);
      if (e2 == hipSuccess) { launch_points_to_internal<F>(c->stream, (const uint32_t*)c->scratch, 0, b->d, n); e2 = hipStreamSynchronize(c->stream); }
      return e2 == hipSuccess ? VIMZ_OK : fail(c, VIMZ_ERR_HIP, "ckgen", e2);
    });
    if (rc) { hipFree(b->d); delete b; return rc; }
  }
  *out = b;
  return VIMZ_OK;
}
int vimz_bases_download(vimz_ctx* c, const vimz_bases* b, size_t offset, uint64_t* xy, size_t n, int form) {
  if (!c || !b || (!xy && n) || offset + n > b->n) return fail(c, VIMZ_ERR_INVALID, "vimz_bases_download: bad argument");
  if (!n) return VIMZ_OK;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  int rc = ensure_scratch(c, 64 * n); if (rc) return rc;
  field_dispatch(curve_base_field(b->curve), [&](auto f) { typedef decltype(f) F; launch_points_from_internal<F>(c->stream, b->d + (size_t)AFFINE_WORDS * offset, form == VIMZ_FORM_CANONICAL, (uint32_t*)c->scratch, n); return VIMZ_OK; });
  HIP_TRY(c, hipMemcpyAsync(xy, c->scratch, 64 * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VIMZ_OK;
}
size_t vimz_bases_len(const vimz_bases* b) { return b ? b->n : 0; }
void vimz_bases_free(vimz_ctx* c, vimz_bases* b) {
  if (!b) return;
  if (c) {
    std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device); hipStreamSynchronize(c->stream);
    if (b->d) hipFree(b->d);
    if (b->tables) hipFree(b->tables);
    for (auto& t : b->small) { if (t.rows) hipFree(t.rows); if (t.mult) hipFree(t.mult); }
  }
  delete b;
}
// Window tables T_j[i] = 2^(c j) P_i for the whole key (c = window_bits, 0 -> 16): K x the key's size in HBM
// (0.67 GB for 2^19 points).  Afterwards MSMs over this key with window_bits = 0 use one shared bucket set.
int vimz_bases_precompute(vimz_ctx* c, vimz_bases* b, int window_bits) {
  if (!c || !b) return fail(c, VIMZ_ERR_INVALID, "vimz_bases_precompute: bad argument");
  const int cw = window_bits > 0 ? window_bits : 16;
  if (cw == SMALL_C) {       // the small-MSM form: rows 2^(7w)·P_i and every multiple of them (keys of at most MSM_SMALL_MAX points)
    if (b->n > MSM_SMALL_MAX) return fail(c, VIMZ_ERR_INVALID, "vimz_bases_precompute: window_bits 7 (tables of multiples) is for keys of at most 30720 points");
    std::lock_guard<std::mutex> g(c->mu);
    HIP_TRY(c, hipSetDevice(c->device));
    BaseTables t;
    return vz_small_tables(c, b, 0, b->n, true, &t);
  }
  if (cw < 10 || cw > 16) return fail(c, VIMZ_ERR_INVALID, "vimz_bases_precompute: window_bits must be 7 or in [10, 16]");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  if (b->tables) { hipFree(b->tables); b->tables = nullptr; }
  if (!b->n) return VIMZ_OK;
  return curve_dispatch(b->curve, [&](auto cv) {
    typedef decltype(cv) C;
    const int K = (C::Scalar::Params::BITS + 1 + cw - 1) / cw;
    hipError_t e = hipMalloc(&b->tables, 4 * (size_t)AFFINE_WORDS * b->n * K);
    if (e != hipSuccess) return fail(c, VIMZ_ERR_HIP, "hipMalloc(window tables)", e);
    e = build_tables<C>(c->stream, b->d, b->n, cw, K, b->tables);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { hipFree(b->tables); b->tables = nullptr; return fail(c, VIMZ_ERR_HIP, "build_tables", e); }
    b->table_c = cw; b->table_K = K;
    return VIMZ_OK;
  });
}

// ---- device vectors ----------------------------------------------------------------------------------
int vimz_vec_alloc(vimz_ctx* c, int field, size_t n, vimz_vec** out) {
  if (!c || !out || field < 0 || field > 3) return fail(c, VIMZ_ERR_INVALID, "vimz_vec_alloc: bad argument");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  vimz_vec* v = new vimz_vec{field, n, nullptr};
  if (n) {
    hipError_t e = hipMalloc(&v->d, 32 * n);
    if (e != hipSuccess) { delete v; return fail(c, VIMZ_ERR_HIP, "hipMalloc(vec)", e); }
    e = hipMemsetAsync(v->d, 0, 32 * n, c->stream);
    if (e != hipSuccess) { hipFree(v->d); delete v; return fail(c, VIMZ_ERR_HIP, "memset(vec)", e); }
  }
  *out = v;
  return VIMZ_OK;
}
int vimz_vec_upload(vimz_ctx* c, vimz_vec* v, size_t offset, const uint64_t* host, size_t n, int form) {
  if (!c || !v || (!host && n) || offset + n > v->n) return fail(c, VIMZ_ERR_INVALID, "vimz_vec_upload: bad argument");
  if (!n) return VIMZ_OK;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  uint32_t* dst = v->d + 8 * offset;
  HIP_TRY(c, hipMemcpyAsync(dst, host, 32 * n, hipMemcpyHostToDevice, c->stream));
  if (form == VIMZ_FORM_CANONICAL)
    field_dispatch(v->field, [&](auto f) { typedef decltype(f) F; launch_to_mont<F>(c->stream, dst, n); return VIMZ_OK; });
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // host buffer may be reused by the caller
  return VIMZ_OK;
}
int vimz_vec_download(vimz_ctx* c, const vimz_vec* v, size_t offset, uint64_t* host, size_t n, int form) {
  if (!c || !v || (!host && n) || offset + n > v->n) return fail(c, VIMZ_ERR_INVALID, "vimz_vec_download: bad argument");
  if (!n) return VIMZ_OK;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  const uint32_t* src = v->d + 8 * offset;
  if (form == VIMZ_FORM_CANONICAL) {
    int rc = ensure_scratch(c, 32 * n); if (rc) return rc;
    field_dispatch(v->field, [&](auto f) { typedef decltype(f) F; launch_from_mont<F>(c->stream, src, (uint32_t*)c->scratch, n); return VIMZ_OK; });
    src = (const uint32_t*)c->scratch;
  }
  HIP_TRY(c, hipMemcpyAsync(host, src, 32 * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VIMZ_OK;
}
size_t vimz_vec_len(const vimz_vec* v) { return v ? v->n : 0; }
void vimz_vec_free(vimz_ctx* c, vimz_vec* v) {
  if (!v) return;
  if (c) { std::lock_guard<std::mutex> g(c->mu); hipSetDevice(c->device); hipStreamSynchronize(c->stream); if (v->d) hipFree(v->d); }
  delete v;
}

// ---- MSM ---------------------------------------------------------------------------------------------
int vimz_msm(vimz_ctx* c, const vimz_bases* bases, const uint64_t* scalars, size_t n, int form, int window_bits,
             uint64_t out_xy[8], int out_form) {
  if (!c || !bases || !out_xy || (!scalars && n) || n > bases->n) return fail(c, VIMZ_ERR_INVALID, "vimz_msm: bad argument");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  if (n) {
    int rc = ensure_scratch(c, 32 * n); if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->scratch, scalars, 32 * n, hipMemcpyHostToDevice, c->stream));
  }
  return msm_device(c, bases, 0, (const uint32_t*)c->scratch, n, form == VIMZ_FORM_MONTGOMERY, window_bits, out_xy, out_form);
}

int vimz_msm_vec(vimz_ctx* c, const vimz_bases* bases, size_t base_offset, const vimz_vec* v, size_t offset, size_t n,
                 int window_bits, uint64_t out_xy[8], int out_form) {
  if (!c || !bases || !v || !out_xy || offset + n > v->n || base_offset + n > bases->n)
    return fail(c, VIMZ_ERR_INVALID, "vimz_msm_vec: bad argument");
  if (v->field != curve_scalar_field(bases->curve)) return fail(c, VIMZ_ERR_INVALID, "vimz_msm_vec: vector is not over the curve's scalar field");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  return msm_device(c, bases, base_offset, v->d + 8 * offset, n, 1, window_bits, out_xy, out_form);
}

int vimz_msm_vec_ex(vimz_ctx* c, const vimz_bases* bases, size_t base_offset, const vimz_vec* v, size_t offset, size_t n,
                    int window_bits, int flags, uint64_t out_xy[8], int out_form) {
  if (!c || !bases || !v || !out_xy || offset + n > v->n || base_offset + n > bases->n)
    return fail(c, VIMZ_ERR_INVALID, "vimz_msm_vec_ex: bad argument");
  if (v->field != curve_scalar_field(bases->curve)) return fail(c, VIMZ_ERR_INVALID, "vimz_msm_vec_ex: vector is not over the curve's scalar field");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  return vz::vz_msm_device(c, bases, base_offset, v->d + 8 * offset, n, 1, window_bits, out_xy, out_form, (flags & VIMZ_MSM_SPLIT_ONES) ? 1 : 0);
}

// KZG opening of a committed vector at a point (the `KZG::prove` the Sonobe decider calls for the final commitments, reached from
// vimz/src/sonobe_backend/decider.rs:13-21): with the SRS's G1 powers as bases, comm = Σ v_i·[τ^i]G commits to p(X) = Σ v_i X^i;
// the opening at z is  eval = p(z)  and  proof = commit((p(X) − p(z)) / (X − z)) — the quotient's coefficients by synthetic division
// (q_{n-2} = v_{n-1}, q_{i-1} = v_i + z·q_i; a serial recurrence of n multiplications: host, ≈ 10 ms at 3·10^5), then the same MSM as the
// commitment, one point shorter.  The pairing check e(proof, [τ − z]H) = e(comm − eval·G, H) is the on-chain verifier's (no G2 arithmetic here).
int vimz_kzg_open(vimz_ctx* c, const vimz_bases* srs, size_t base_offset, const vimz_vec* v, size_t offset, size_t n, const uint64_t z[4], int form,
                  uint64_t eval_out[4], uint64_t proof_xy[8]) {
  if (!c || !srs || !v || !z || !eval_out || !proof_xy || n == 0 || offset + n > v->n || base_offset + n > srs->n) return fail(c, VIMZ_ERR_INVALID, "vimz_kzg_open: bad argument");
  if (v->field != curve_scalar_field(srs->curve)) return fail(c, VIMZ_ERR_INVALID, "vimz_kzg_open: vector is not over the curve's scalar field");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  return vz::vz_kzg_open_device(c, srs, base_offset, v->field, v->d + 8 * offset, n, z, form, eval_out, proof_xy);
}

// ---- probes ------------------------------------------------------------------------------------------
int vimz_field_op(vimz_ctx* c, int field, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  if (!c || !a || !out || op < 0 || op > 3 || (op != 3 && !b)) return fail(c, VIMZ_ERR_INVALID, "vimz_field_op: bad argument");
  if (!n) return VIMZ_OK;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  int rc = ensure_scratch(c, 96 * n); if (rc) return rc;
  uint32_t* da = (uint32_t*)c->scratch; uint32_t* db = da + 8 * n; uint32_t* dout = db + 8 * n;
  HIP_TRY(c, hipMemcpyAsync(da, a, 32 * n, hipMemcpyHostToDevice, c->stream));
  if (b) HIP_TRY(c, hipMemcpyAsync(db, b, 32 * n, hipMemcpyHostToDevice, c->stream));
  rc = field_dispatch(field, [&](auto f) { typedef decltype(f) F; launch_field_probe<F>(c->stream, op, da, db, dout, n); return VIMZ_OK; });
  if (rc) return fail(c, rc, "vimz_field_op: bad field");
  HIP_TRY(c, hipMemcpyAsync(out, dout, 32 * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VIMZ_OK;
}

int vimz_curve_add(vimz_ctx* c, int curve, const uint64_t* p, const uint64_t* q, uint64_t* out, size_t n) {
  if (!c || !p || !q || !out) return fail(c, VIMZ_ERR_INVALID, "vimz_curve_add: bad argument");
  if (!n) return VIMZ_OK;
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  int rc = ensure_scratch(c, 192 * n); if (rc) return rc;
  uint32_t* dp = (uint32_t*)c->scratch; uint32_t* dq = dp + 16 * n; uint32_t* dout = dq + 16 * n;
  HIP_TRY(c, hipMemcpyAsync(dp, p, 64 * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(dq, q, 64 * n, hipMemcpyHostToDevice, c->stream));
  rc = curve_dispatch(curve, [&](auto cv) { typedef typename decltype(cv)::Base F; launch_curve_add_probe<F>(c->stream, dp, dq, dout, n); return VIMZ_OK; });
  if (rc) return fail(c, rc, "vimz_curve_add: bad curve");
  HIP_TRY(c, hipMemcpyAsync(out, dout, 64 * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VIMZ_OK;
}

}  // extern "C"

#ifdef VIMZ_TESTING
// ---- test hook (include/vimz_hip_testing.h): in libvimz_hip_testing.so only ----------------------------------------------------------------------
#include "../../include/vimz_hip_testing.h"
extern "C" int vimz_test_msm_rows(vimz_ctx* c, const vimz_bases* bases, const uint64_t* scalars, size_t n, size_t row_stride, size_t G, int form, int use_tables,
                                  size_t n_ones, int calls, uint64_t* out_xy, uint64_t* s1_xy, uint64_t* s1_ref_xy) {
  if (!c || !bases || !scalars || !out_xy || !n || !G || G > MSM_ROWS_MAX || row_stride < n || n > bases->n || n_ones > n || calls < 1 || bases->curve != VIMZ_CURVE_BN254_G1 ||
      (n_ones && (!s1_xy || !s1_ref_xy)) || (use_tables && !bases->tables))
    return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_rows: bad argument");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  typedef BnG1::Base FS;
  const size_t pin_stride = 4 * (size_t)XYZZ_WORDS * MSM_MAX_WINDOWS, s1_slot = 4 * (size_t)XYZZ_WORDS * (MSM_MAX_WINDOWS - 1);
  const int mont = form == VIMZ_FORM_MONTGOMERY;
  int rc = ensure_scratch(c, 32 * G * row_stride); if (rc) return rc;
  char* pin = nullptr;
  MsmWorkspace ws;
  hipError_t e = hipHostMalloc((void**)&pin, G * pin_stride);
  if (e == hipSuccess) e = hipMemcpyAsync(c->scratch, scalars, 32 * ((G - 1) * row_stride + n), hipMemcpyHostToDevice, c->stream);
  const uint32_t* ds = (const uint32_t*)c->scratch;
  const BaseTables tb = bases->tb(0);
  auto affine_out = [&](const Affine<FS>& a, uint64_t* o) { const FS x = FS::from_mont(a.x), y = FS::from_mont(a.y); memcpy(o, x.v, 32); memcpy(o + 4, y.v, 32); };
  for (int call = 0; call < calls && e == hipSuccess; call++) {
    memset(pin, 0xff, G * pin_stride);      // (nothing of an earlier call may pass for this one's result)
    OnesDesc s1[MSM_ROWS_MAX];
    for (size_t r = 0; r < G; r++) s1[r] = OnesDesc{ds + 8 * r * row_stride, bases->d, reinterpret_cast<uint32_t*>(pin + r * pin_stride + s1_slot), n_ones};
    MsmPlan pl;
    e = msm_launch_rows<BnG1>(c->stream, ws, bases->d, ds, n, row_stride, (uint32_t)G, mont, pin, pin_stride, &pl, 1, use_tables ? &tb : nullptr, s1, n_ones ? (uint32_t)G : 0u, (uint32_t)G);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) break;
    for (size_t r = 0; r < G; r++) {
      affine_out(msm_finish<BnG1>(pl, pin + r * pin_stride), out_xy + 8 * ((size_t)call * G + r));
      if (n_ones) affine_out(to_affine(ones_finish<BnG1>(pin + r * pin_stride + s1_slot)), s1_xy + 8 * ((size_t)call * G + r));
    }
  }
  for (size_t r = 0; r < G && n_ones && e == hipSuccess; r++) {      // the same sums by the per-row launches
    memset(pin, 0xff, 4 * (size_t)XYZZ_WORDS);
    e = ones_launch<BnG1>(c->stream, ws, bases->d, ds + 8 * r * row_stride, n_ones, mont, pin);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) affine_out(to_affine(ones_finish<BnG1>(pin)), s1_ref_xy + 8 * r);
  }
  hipStreamSynchronize(c->stream);
  ws.release();
  if (pin) hipHostFree(pin);
  if (e != hipSuccess) return vz_fail(c, VIMZ_ERR_HIP, "vimz_test_msm_rows", e);
  return VIMZ_OK;
}

// ---- the MSM's tail stages on a caller's arrays (tests/test_gpu_msm_tail.py): every launch through the launcher the product calls (msm.hpp) ------------------
#include "msm.hpp"
namespace {
// device arrays of one hook call: freed on every way out
struct TailBufs {
  std::vector<void*> all;
  ~TailBufs() { for (void* p : all) hipFree(p); }
  hipError_t get(uint32_t** p, size_t words, int fill = -1) {
    *p = nullptr;
    hipError_t e = hipMalloc((void**)p, 4 * (words ? words : 1));
    if (e != hipSuccess) return e;
    all.push_back(*p);
    if (fill >= 0) { e = hipMemset(*p, fill, 4 * (words ? words : 1)); if (e == hipSuccess) e = hipStreamSynchronize(nullptr); }      // (a null-stream fill: msm_api.hpp)
    return e;
  }
};
static hipError_t tail_up(vimz_ctx* c, uint32_t* d, const uint32_t* h, size_t words) { return words ? hipMemcpyAsync(d, h, 4 * words, hipMemcpyHostToDevice, c->stream) : hipSuccess; }
static hipError_t tail_down(vimz_ctx* c, uint32_t* h, const uint32_t* d, size_t words) { return words ? hipMemcpyAsync(h, d, 4 * words, hipMemcpyDeviceToHost, c->stream) : hipSuccess; }
// offsets of nb buckets: monotone, the last one inside an array of n_slots
static bool tail_offsets_ok(const uint32_t* off, size_t nb, size_t n_slots) {
  for (size_t b = 0; b < nb; b++) if (off[b] > off[b + 1]) return false;
  return off[nb] <= n_slots;
}
constexpr uint32_t TAIL_HEAVY_GUARD = 64;      // words after the heavy list that a scan must leave alone
constexpr uint32_t QUAD_LEVEL_WORDS = 129;     // a level of vimz_test_quad_level: count, dst[64], src[64]

// TEST-ONLY kernel: workgroup s loads slots [256 s, 256 s + 256) into LDS, applies the caller's levels through quad_level — the tables are read by the lambdas —
// or quad_tree256, and stores all 256 slots.
template <class F>
__global__ void __launch_bounds__(256) k_test_quad_level(const uint32_t* __restrict__ in, const uint32_t* __restrict__ levels, uint32_t n_levels, int tree, uint32_t* __restrict__ out) {
  __shared__ XYZZ<F> sh[256];
  const uint32_t t = threadIdx.x;
  sh[t] = load_xyzz<F>(in, (size_t)blockIdx.x * 256 + t);
  __syncthreads();
  if (tree) quad_tree256<F>(sh);
  else for (uint32_t l = 0; l < n_levels; l++) {
    const uint32_t* L = levels + (size_t)QUAD_LEVEL_WORDS * l;
    quad_level<F>(sh, L[0], [L](uint32_t e) { return L[1 + e]; }, [L](uint32_t e) { return L[65 + e]; });
  }
  store_xyzz(out, (size_t)blockIdx.x * 256 + t, sh[t]);
}
}  // namespace
#define TAIL_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) { hipStreamSynchronize(c->stream); return vz_fail(c, VIMZ_ERR_HIP, #x, _e); } } while (0)

extern "C" int vimz_test_msm_scan(vimz_ctx* c, const uint32_t* block_hist, size_t blocks, size_t nb, uint32_t sub, uint32_t heavy_min, int lds, int calls, uint32_t* counts_out,
                                  uint32_t* bucket_off_out, uint32_t* sub_off_out, uint32_t totals_out[4], uint32_t* heavy_out, uint32_t* block_hist_out) {
  if (!c || !block_hist || !counts_out || !bucket_off_out || !sub_off_out || !totals_out || !heavy_out || (lds != 0 && lds != 1) || (lds && !block_hist_out) || calls < 1)
    return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_scan: bad argument");
  if (!blocks || blocks > SORT_BLOCKS || !nb || nb >= (1u << 24) || !sub) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_scan: blocks in 1..256, nb in 1..2^24 - 1, sub >= 1");
  std::vector<uint32_t> sum(nb, 0u);
  uint64_t total = 0;
  for (size_t k = 0; k < blocks; k++) for (size_t g = 0; g < nb; g++) { sum[g] += block_hist[k * nb + g]; total += block_hist[k * nb + g]; }
  if (total >= (1ull << 31)) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_scan: more than 2^31 - 1 entries");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  TailBufs B;
  uint32_t *hist, *counts, *boff, *soff, *totals, *heavy;
  const size_t heavy_words = 1 + (size_t)MSM_HEAVY_CAP + TAIL_HEAVY_GUARD;
  TAIL_TRY(B.get(&hist, blocks * nb)); TAIL_TRY(B.get(&counts, nb)); TAIL_TRY(B.get(&boff, nb + 1, 0xff)); TAIL_TRY(B.get(&soff, nb + 1, 0xff));
  TAIL_TRY(B.get(&totals, MSM_TOTALS_WORDS, 0)); TAIL_TRY(B.get(&heavy, heavy_words, 0xff));
  for (int call = 0; call < calls; call++) {
    if (lds) {
      TAIL_TRY(tail_up(c, hist, block_hist, blocks * nb));
      launch_prefix_scan(c->stream, hist, (uint32_t)nb, counts, (uint32_t)blocks, heavy, boff, soff, totals, sub, heavy_min, MsmRowStrides(), 1);
    } else {      // (the fallback sort zeroes the list's count itself: launch_sort)
      TAIL_TRY(tail_up(c, counts, sum.data(), nb));
      TAIL_TRY(hipMemsetAsync(heavy, 0, 4, c->stream));
      launch_scan(c->stream, counts, (uint32_t)nb, boff, soff, totals, sub, heavy, heavy_min);
    }
    TAIL_TRY(hipGetLastError());
    TAIL_TRY(hipStreamSynchronize(c->stream));
  }
  TAIL_TRY(tail_down(c, counts_out, counts, nb)); TAIL_TRY(tail_down(c, bucket_off_out, boff, nb + 1)); TAIL_TRY(tail_down(c, sub_off_out, soff, nb + 1));
  TAIL_TRY(tail_down(c, totals_out, totals, 4)); TAIL_TRY(tail_down(c, heavy_out, heavy, heavy_words));
  if (lds) TAIL_TRY(tail_down(c, block_hist_out, hist, blocks * nb));
  TAIL_TRY(hipStreamSynchronize(c->stream));
  return VIMZ_OK;
}

extern "C" int vimz_test_msm_combine(vimz_ctx* c, int curve, uint32_t* partial, size_t n_slots, const uint32_t* sub_off, size_t nb, const uint32_t* heavy, size_t n_ids, int lane_bits,
                                     uint32_t heavy_min, size_t rows, int calls) {
  if (!c || !partial || !sub_off || !heavy || calls < 1 || !nb || nb >= (1u << 24) || n_slots >= (1u << 24)) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_combine: bad argument");
  if (curve < VIMZ_CURVE_BN254_G1 || curve > VIMZ_CURVE_VESTA) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_combine: bad curve");
  if (lane_bits < 0 || lane_bits > 4) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_combine: lane_bits outside 0..4");
  if (!rows || rows > MSM_ROWS_MAX) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_combine: rows outside 1..16");
  if (n_ids > MSM_HEAVY_CAP) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_combine: more ids than the heavy list holds");
  for (size_t r = 0; r < rows; r++) {
    const uint32_t* off = sub_off + r * (nb + 1); const uint32_t* hv = heavy + r * (1 + n_ids);
    if (!tail_offsets_ok(off, nb, n_slots)) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_combine: sub_off not monotone or outside partial");
    if (hv[0] > MSM_HEAVY_CAP) continue;      // an overflowed list is not read
    if (hv[0] > n_ids) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_combine: the heavy count exceeds the ids given");
    std::vector<bool> seen(nb, false);
    for (uint32_t h = 0; h < hv[0]; h++) {
      const uint32_t b = hv[1 + h];
      if (b >= nb) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_combine: a heavy bucket id not below nb");
      if (seen[b] || off[b + 1] - off[b] <= heavy_min) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_combine: a heavy bucket listed twice or not above heavy_min");
      seen[b] = true;
    }
  }
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  const uint32_t G = (uint32_t)rows;
  const MsmRowStrides rs = msm_row_strides(G, 0, (uint32_t)nb, 0, n_slots, 0);
  TailBufs B;
  uint32_t *dp, *doff, *dheavy, *dscr, *ddone;
  TAIL_TRY(B.get(&dp, rows * XYZZ_WORDS * n_slots)); TAIL_TRY(B.get(&doff, rows * (nb + 1))); TAIL_TRY(B.get(&dheavy, rows * ((size_t)MSM_HEAVY_CAP + 1), 0xff));
  TAIL_TRY(B.get(&dscr, rows * MsmWorkspace::HEAVY_SCRATCH_WORDS, 0xff)); TAIL_TRY(B.get(&ddone, rows * (size_t)MSM_HEAVY_DONE_WORDS, 0));
  TAIL_TRY(tail_up(c, doff, sub_off, rows * (nb + 1)));
  for (size_t r = 0; r < rows; r++) TAIL_TRY(tail_up(c, dheavy + r * ((size_t)MSM_HEAVY_CAP + 1), heavy + r * (1 + n_ids), 1 + n_ids));
  const int rc = curve_dispatch(curve, [&](auto cv) {
    typedef typename decltype(cv)::Coord F;
    for (int call = 0; call < calls; call++) {      // every call folds the caller's partials anew; the tickets are whatever the call before left
      TAIL_TRY(tail_up(c, dp, partial, rows * XYZZ_WORDS * n_slots));
      launch_combine<F>(c->stream, dp, doff, (uint32_t)nb, dheavy, dscr, (uint32_t)lane_bits, heavy_min, ddone, rs, G);
      TAIL_TRY(hipGetLastError());
      TAIL_TRY(hipStreamSynchronize(c->stream));
    }
    return (int)VIMZ_OK;
  });
  if (rc) return rc;
  TAIL_TRY(tail_down(c, partial, dp, rows * XYZZ_WORDS * n_slots));
  TAIL_TRY(hipStreamSynchronize(c->stream));
  return VIMZ_OK;
}

extern "C" int vimz_test_msm_reduce(vimz_ctx* c, int curve, const uint32_t* partial, size_t n_slots, const uint32_t* counts, const uint32_t* sub_off, uint32_t nbw, size_t windows,
                                    int mode, size_t rows, int calls, uint32_t* sums_out) {
  if (!c || !partial || !counts || !sub_off || !sums_out || calls < 1 || mode < 0 || mode > 2 || n_slots >= (1u << 24)) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_reduce: bad argument");
  if (curve < VIMZ_CURVE_BN254_G1 || curve > VIMZ_CURVE_VESTA) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_reduce: bad curve");
  if (nbw < 2 || nbw > 32768 || (nbw & (nbw - 1))) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_reduce: nbw not a power of two in 2..32768");
  if (!rows || rows > MSM_ROWS_MAX) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_reduce: rows outside 1..16");
  uint32_t Pl = 0, Gp = 0;
  const bool planes_fit = msm_plane_shape(nbw, Pl, Gp);
  if (!windows || windows > (size_t)MSM_MAX_WINDOWS / 2 || (mode == 2 && (windows != 1 || rows != 1 || !planes_fit)))
    return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_reduce: windows outside 1..48, or bit planes over anything but one row of one bucket set of 1024 buckets or more");
  const size_t nb = (size_t)nbw * windows;
  for (size_t r = 0; r < rows; r++) {
    const uint32_t* off = sub_off + r * (nb + 1);
    if (!tail_offsets_ok(off, nb, n_slots)) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_reduce: sub_off not monotone or outside partial");
    for (size_t b = 0; b < nb; b++) if (counts[r * nb + b] && off[b] >= n_slots) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_reduce: a filled bucket's slot outside partial");
  }
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  const uint32_t G = (uint32_t)rows;
  const size_t kout = mode == 2 ? Pl + 2 : mode == 1 ? 2 * windows : windows;
  const MsmRowStrides rs = msm_row_strides(G, 0, (uint32_t)nb, 0, n_slots, (size_t)XYZZ_WORDS * kout);
  TailBufs B;
  uint32_t *dp, *dcnt, *doff, *dout, *dstage, *dtot;
  TAIL_TRY(B.get(&dp, rows * XYZZ_WORDS * n_slots)); TAIL_TRY(B.get(&dcnt, rows * nb)); TAIL_TRY(B.get(&doff, rows * (nb + 1))); TAIL_TRY(B.get(&dout, rows * XYZZ_WORDS * kout));
  TAIL_TRY(B.get(&dstage, (size_t)XYZZ_WORDS * 256, 0xff)); TAIL_TRY(B.get(&dtot, MSM_TOTALS_WORDS, 0));
  TAIL_TRY(tail_up(c, dp, partial, rows * XYZZ_WORDS * n_slots)); TAIL_TRY(tail_up(c, dcnt, counts, rows * nb)); TAIL_TRY(tail_up(c, doff, sub_off, rows * (nb + 1)));
  const int rc = curve_dispatch(curve, [&](auto cv) {
    typedef typename decltype(cv)::Coord F;
    for (int call = 0; call < calls; call++) {
      TAIL_TRY(hipMemsetAsync(dout, 0xff, 4 * rows * XYZZ_WORDS * kout, c->stream));      // (nothing of an earlier call may pass for this one's result)
      if (mode == 2) launch_reduce_planes<F>(c->stream, dp, dcnt, doff, nbw, Pl, Gp, dstage, dtot + 3, dout);
      else launch_reduce<F>(c->stream, dp, dcnt, doff, nbw, (uint32_t)windows, dout, mode == 1 ? dout + (size_t)XYZZ_WORDS * windows : (uint32_t*)nullptr, rs, G);
      TAIL_TRY(hipGetLastError());
      TAIL_TRY(hipStreamSynchronize(c->stream));
    }
    return (int)VIMZ_OK;
  });
  if (rc) return rc;
  TAIL_TRY(tail_down(c, sums_out, dout, rows * XYZZ_WORDS * kout));
  TAIL_TRY(hipStreamSynchronize(c->stream));
  return VIMZ_OK;
}

extern "C" int vimz_test_msm_tree(vimz_ctx* c, int curve, const uint32_t* points, size_t m, size_t count, uint32_t* out) {
  if (!c || !points || !out || !m) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_tree: bad argument");
  if (curve < VIMZ_CURVE_BN254_G1 || curve > VIMZ_CURVE_VESTA) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_tree: bad curve");
  if (count > MSM_ROWS_MAX) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_tree: more than 16 sums");
  if (count ? m > 256 : m > 65536) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_tree: more points than the trees take (256 a sum; 65536 for one sum)");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t sums = count ? count : 1;
  TailBufs B;
  uint32_t *din, *dtmp, *dout;
  TAIL_TRY(B.get(&din, sums * m * XYZZ_WORDS)); TAIL_TRY(B.get(&dtmp, (size_t)XYZZ_WORDS * 256, 0xff)); TAIL_TRY(B.get(&dout, sums * XYZZ_WORDS, 0xff));
  TAIL_TRY(tail_up(c, din, points, sums * m * XYZZ_WORDS));
  curve_dispatch(curve, [&](auto cv) {
    typedef typename decltype(cv)::Coord F;
    if (!count) launch_tree256<F>(c->stream, din, (uint32_t)m, dtmp, dout);
    else {
      OnesDescs ds;
      for (size_t i = 0; i < 2 * MSM_ROWS_MAX; i++) ds.d[i] = OnesDesc{nullptr, nullptr, i < count ? dout + (size_t)XYZZ_WORDS * i : nullptr, 0};
      launch_tree_rows<F>(c->stream, din, (uint32_t)m, ds, (uint32_t)count);
    }
    return (int)VIMZ_OK;
  });
  TAIL_TRY(hipGetLastError());
  TAIL_TRY(tail_down(c, out, dout, sums * XYZZ_WORDS));
  TAIL_TRY(hipStreamSynchronize(c->stream));
  return VIMZ_OK;
}

extern "C" int vimz_test_quad_level(vimz_ctx* c, int curve, const uint32_t* slots, size_t sets, const uint32_t* levels, size_t n_levels, int tree, uint32_t* out) {
  if (!c || !slots || !out || !sets || sets > 4096 || (!tree && (!levels || !n_levels)) || n_levels > 64) return fail(c, VIMZ_ERR_INVALID, "vimz_test_quad_level: bad argument");
  if (curve < VIMZ_CURVE_BN254_G1 || curve > VIMZ_CURVE_VESTA) return fail(c, VIMZ_ERR_INVALID, "vimz_test_quad_level: bad curve");
  for (size_t l = 0; !tree && l < n_levels; l++) {
    const uint32_t* L = levels + QUAD_LEVEL_WORDS * l;
    if (L[0] > 64) return fail(c, VIMZ_ERR_INVALID, "vimz_test_quad_level: more than 64 additions in a level");
    bool seen[256] = {};
    for (uint32_t e = 0; e < L[0]; e++) {
      if (L[1 + e] >= 256 || L[65 + e] >= 256) return fail(c, VIMZ_ERR_INVALID, "vimz_test_quad_level: an index not below 256");
      if (seen[L[1 + e]]) return fail(c, VIMZ_ERR_INVALID, "vimz_test_quad_level: a destination twice in one level");
      seen[L[1 + e]] = true;
    }
  }
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t words = sets * 256 * XYZZ_WORDS, lw = tree ? 0 : QUAD_LEVEL_WORDS * n_levels;
  TailBufs B;
  uint32_t *din, *dlv, *dout;
  TAIL_TRY(B.get(&din, words)); TAIL_TRY(B.get(&dlv, lw)); TAIL_TRY(B.get(&dout, words, 0xff));
  TAIL_TRY(tail_up(c, din, slots, words)); TAIL_TRY(tail_up(c, dlv, levels, lw));
  curve_dispatch(curve, [&](auto cv) {
    typedef typename decltype(cv)::Coord F;
    hipLaunchKernelGGL(k_test_quad_level<F>, dim3((unsigned)sets), dim3(256), 0, c->stream, (const uint32_t*)din, (const uint32_t*)dlv, (uint32_t)(tree ? 0 : n_levels), tree, dout);
    return (int)VIMZ_OK;
  });
  TAIL_TRY(hipGetLastError());
  TAIL_TRY(tail_down(c, out, dout, words));
  TAIL_TRY(hipStreamSynchronize(c->stream));
  return VIMZ_OK;
}

// ---- the MSM's head stages on a caller's input (tests/test_gpu_msm_head.py; the reference and the cases: tests/_msm_head_ref.py): launch_sort, launch_small and
// launch_fixed with an MsmCall and an MsmShape filled by hand on a workspace of the hook's own; launch_accum, launch_ones, ones_launch_rows on arrays of its own --------
namespace {
struct WorkspaceGuard {      // the hook's own workspace: released on every way out
  MsmWorkspace ws;
  ~WorkspaceGuard() { ws.release(); }
};
struct PinnedGuard {
  void* p = nullptr;
  ~PinnedGuard() { if (p) hipHostFree(p); }
};
// the tables vimz_bases_precompute(7) made for the whole key (rows 2^(7w)·P_i, every multiple of them), or nullptr
static const vimz_small_tables* head_small_tables(const vimz_bases* b) {
  vimz_bases* bm = const_cast<vimz_bases*>(b);
  std::lock_guard<std::mutex> g(bm->small_mu);
  for (auto& t : bm->small) if (t.offset == 0 && t.n == b->n && t.rows) return &t;
  return nullptr;
}
static int head_small_windows(int curve) {
  int K = 0;
  curve_dispatch(curve, [&](auto cv) { typedef decltype(cv) C; K = (C::Scalar::Params::BITS + SMALL_C) / SMALL_C; return (int)VIMZ_OK; });
  return K;
}
}  // namespace

extern "C" int vimz_test_msm_sort(vimz_ctx* c, int field, const uint64_t* scalars, size_t n, int form, int skip_ones, int sgn, int window_bits, int K, int shared, uint32_t pstride,
                                  int lds, uint32_t sort_blocks, uint32_t sub, uint32_t heavy_min, int calls, uint32_t* counts_out, uint32_t* bucket_off_out, uint32_t* sub_off_out,
                                  uint32_t* totals_out, uint32_t* sorted_out, size_t sorted_len) {
  if (!c || !scalars || !counts_out || !bucket_off_out || !sub_off_out || !totals_out || !sorted_out || calls < 1 || (lds != 0 && lds != 1) || (shared != 0 && shared != 1) ||
      (form != VIMZ_FORM_CANONICAL && form != VIMZ_FORM_MONTGOMERY))
    return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_sort: bad argument");
  if (field < VIMZ_FIELD_BN254_FR || field > VIMZ_FIELD_VESTA_FQ) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_sort: bad field");
  if (window_bits < 2 || window_bits > 16) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_sort: window bits outside 2..16");
  if (K < 1 || K > 128 || !n || n >= (1u << 24) || !sub) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_sort: K in 1..128, n in 1..2^24 - 1, sub >= 1");
  if (!sort_blocks || sort_blocks > SORT_BLOCKS) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_sort: sort_blocks outside 1..256");
  const uint32_t nbw = 1u << (window_bits - 1);
  const size_t nb = shared ? nbw : (size_t)nbw * K;
  if (lds && nb * 4 > 144 * 1024) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_sort: the counters of the LDS sort do not fit 144 KiB");
  if (sorted_len < (size_t)K * n || sorted_len >= (1u << 31)) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_sort: `sorted` shorter than K·n entries (or 2^31 and more)");
  if (n + (size_t)K * pstride >= (1u << 31)) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_sort: an entry would not fit 31 bits");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  WorkspaceGuard W;
  TailBufs B;
  uint32_t* dsc;
  TAIL_TRY(W.ws.reserve((uint32_t)nb, sorted_len, 1));
  TAIL_TRY(B.get(&dsc, 8 * n));
  TAIL_TRY(tail_up(c, dsc, reinterpret_cast<const uint32_t*>(scalars), 8 * n));
  MsmShape sh;
  sh.plan.c = window_bits; sh.plan.K = K; sh.plan.nbw = nbw; sh.plan.nb = (uint32_t)nb; sh.plan.split_ones = skip_ones; sh.plan.tabled = 0;
  sh.lds_sort = lds != 0; sh.shared = shared != 0; sh.sub = sub; sh.entries = sorted_len; sh.max_subs = 1; sh.sort_blocks = sort_blocks; sh.heavy_min = heavy_min;
  sh.bstride = shared ? 0u : nbw; sh.pstride = pstride;
  const MsmCall a{c->stream, W.ws, nullptr, dsc, n, form == VIMZ_FORM_MONTGOMERY, sgn, skip_ones, nullptr, nullptr, nullptr, nullptr};
  return field_dispatch(field, [&](auto f) {
    typedef decltype(f) S;
    for (int call = 0; call < calls; call++) {      // every call sorts the caller's scalars anew; the ticket (totals[2]) is whatever the call before left
      TAIL_TRY(hipMemsetAsync(W.ws.sorted, 0xff, 4 * sorted_len, c->stream));
      TAIL_TRY(launch_sort<S>(a, sh, MsmRowStrides(), 1));
      TAIL_TRY(hipGetLastError());
      TAIL_TRY(tail_down(c, counts_out + (size_t)call * nb, W.ws.counts, nb)); TAIL_TRY(tail_down(c, bucket_off_out + (size_t)call * (nb + 1), W.ws.bucket_off, nb + 1));
      TAIL_TRY(tail_down(c, sub_off_out + (size_t)call * (nb + 1), W.ws.sub_off, nb + 1)); TAIL_TRY(tail_down(c, totals_out + 4 * (size_t)call, W.ws.totals, 4));
      TAIL_TRY(tail_down(c, sorted_out + (size_t)call * sorted_len, W.ws.sorted, sorted_len));
      TAIL_TRY(hipStreamSynchronize(c->stream));
    }
    return (int)VIMZ_OK;
  });
}

extern "C" int vimz_test_msm_accum(vimz_ctx* c, const vimz_bases* bases, const uint32_t* sorted, size_t entries, const uint32_t* bucket_off, const uint32_t* sub_off,
                                   const uint32_t* totals, size_t nb, uint32_t sub, size_t rows, uint32_t* partial, size_t n_slots) {
  if (!c || !bases || !bases->n || !sorted || !bucket_off || !sub_off || !totals || !partial || !nb || nb >= (1u << 24) || !sub || !entries || entries >= (1u << 31) || !n_slots ||
      n_slots >= (1u << 24))
    return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_accum: bad argument");
  if (!rows || rows > MSM_ROWS_MAX) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_accum: rows outside 1..16");
  for (size_t r = 0; r < rows; r++) {
    const uint32_t* bo = bucket_off + r * (nb + 1); const uint32_t* so = sub_off + r * (nb + 1); const uint32_t* srt = sorted + r * entries;
    if (bo[0] || so[0] || !tail_offsets_ok(bo, nb, entries) || !tail_offsets_ok(so, nb, n_slots))
      return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_accum: offsets that do not start at zero, are not monotone or end outside their array");
    for (size_t b = 0; b < nb; b++)
      if (so[b + 1] - so[b] != (bo[b + 1] - bo[b] + sub - 1) / sub) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_accum: sub_off is not the scan of ceil(bucket size / sub)");
    if (totals[r * MSM_TOTALS_WORDS] > so[nb]) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_accum: totals[0] above the number of sub-buckets");
    for (uint32_t e = 0; e < bo[nb]; e++) if ((srt[e] & 0x7fffffffu) >= bases->n) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_accum: an entry's point outside the key");
  }
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  const uint32_t G = (uint32_t)rows;
  const MsmRowStrides rs = msm_row_strides(G, 0, (uint32_t)nb, entries, n_slots, 0);
  TailBufs B;
  uint32_t *dsrt, *dbo, *dso, *dtot, *dp;
  TAIL_TRY(B.get(&dsrt, rows * entries)); TAIL_TRY(B.get(&dbo, rows * (nb + 1))); TAIL_TRY(B.get(&dso, rows * (nb + 1))); TAIL_TRY(B.get(&dtot, rows * MSM_TOTALS_WORDS));
  TAIL_TRY(B.get(&dp, rows * XYZZ_WORDS * n_slots));
  TAIL_TRY(tail_up(c, dsrt, sorted, rows * entries)); TAIL_TRY(tail_up(c, dbo, bucket_off, rows * (nb + 1))); TAIL_TRY(tail_up(c, dso, sub_off, rows * (nb + 1)));
  TAIL_TRY(tail_up(c, dtot, totals, rows * MSM_TOTALS_WORDS)); TAIL_TRY(tail_up(c, dp, partial, rows * XYZZ_WORDS * n_slots));
  curve_dispatch(bases->curve, [&](auto cv) {
    typedef typename decltype(cv)::Coord F;
    launch_accum<F>(c->stream, bases->d, dsrt, dbo, dso, (uint32_t)nb, dtot, dp, sub, n_slots, rs, G);
    return (int)VIMZ_OK;
  });
  TAIL_TRY(hipGetLastError());
  TAIL_TRY(tail_down(c, partial, dp, rows * XYZZ_WORDS * n_slots));
  TAIL_TRY(hipStreamSynchronize(c->stream));
  return VIMZ_OK;
}

// what the two fused hooks share: the scalars up, `calls` launches by `launch` into a pinned buffer of the hook's own (as the product's callers hand one in), K sums a call out
template <class Launch>
static int head_fused_run(vimz_ctx* c, const uint64_t* scalars, size_t n, int K, int calls, uint32_t* sums_out, Launch launch) {
  WorkspaceGuard W;
  TailBufs B;
  PinnedGuard pin;
  uint32_t* dsc;
  const size_t out_words = (size_t)XYZZ_WORDS * K;
  TAIL_TRY(hipHostMalloc(&pin.p, 4 * out_words));
  TAIL_TRY(B.get(&dsc, 8 * n));
  TAIL_TRY(tail_up(c, dsc, reinterpret_cast<const uint32_t*>(scalars), 8 * n));
  for (int call = 0; call < calls; call++) {      // every call on the caller's scalars again; the windows' tickets are whatever the call before left
    TAIL_TRY(hipStreamSynchronize(c->stream));
    memset(pin.p, 0xff, 4 * out_words);           // (nothing of an earlier call may pass for this one's result)
    TAIL_TRY(launch(W.ws, dsc, reinterpret_cast<uint32_t*>(pin.p)));
    TAIL_TRY(hipStreamSynchronize(c->stream));
    memcpy(sums_out + (size_t)call * out_words, pin.p, 4 * out_words);
  }
  return VIMZ_OK;
}

extern "C" int vimz_test_msm_small(vimz_ctx* c, const vimz_bases* bases, int use_tables, size_t base_offset, const uint64_t* scalars, size_t n, int form, int sgn, uint32_t Q,
                                   uint32_t chunk, int tail, int calls, uint32_t* sums_out) {
  if (!c || !bases || !scalars || !sums_out || !n || calls < 1 || (tail != 0 && tail != 1) || (form != VIMZ_FORM_CANONICAL && form != VIMZ_FORM_MONTGOMERY))
    return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_small: bad argument");
  if (base_offset > bases->n || n > bases->n - base_offset) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_small: the scalars reach past the key");
  if (!Q || Q > SMALL_MAXQ) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_small: Q outside 1..32");
  if (!chunk || chunk > SMALL_CHUNK) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_small: chunk outside 1..1536");
  if ((size_t)chunk * (Q - 1) >= n || n > (size_t)chunk * Q) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_small: not chunk·(Q - 1) < n <= chunk·Q");
  const vimz_small_tables* st = use_tables ? head_small_tables(bases) : nullptr;
  if (use_tables && !st) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_small: the key has no tables of the fused path (vimz_bases_precompute(7))");
  const int K = head_small_windows(bases->curve);
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  MsmShape sh;
  sh.path = MSM_PATH_SMALL; sh.plan.c = SMALL_C; sh.plan.K = K; sh.plan.nbw = SMALL_NBW; sh.plan.nb = SMALL_NBW * (uint32_t)K; sh.plan.split_ones = 0; sh.plan.tabled = st ? 2 : 0;
  sh.Q = Q; sh.chunk = chunk; sh.kout = K;
  BaseTables tb{nullptr, 0, 0, 0, 0};
  if (st) tb = BaseTables{st->rows, st->n, base_offset, st->c, st->K, 0, st->mult};
  return curve_dispatch(bases->curve, [&](auto cv) {
    typedef decltype(cv) C;
    return head_fused_run(c, scalars, n, K, calls, sums_out, [&](MsmWorkspace& ws, const uint32_t* dsc, uint32_t* pinned) {
      const MsmCall a{c->stream, ws, bases->d + (size_t)AFFINE_WORDS * base_offset, dsc, n, form == VIMZ_FORM_MONTGOMERY, sgn, 0, pinned, nullptr, st ? &tb : nullptr, nullptr};
      return launch_small<C>(a, sh, tail != 0);
    });
  });
}

extern "C" int vimz_test_msm_fixed(vimz_ctx* c, const vimz_bases* bases, size_t base_offset, const uint64_t* scalars, size_t n, int form, int sgn, int calls, uint32_t* sums_out) {
  if (!c || !bases || !scalars || !sums_out || !n || calls < 1 || (form != VIMZ_FORM_CANONICAL && form != VIMZ_FORM_MONTGOMERY))
    return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_fixed: bad argument");
  if (base_offset > bases->n || n > bases->n - base_offset) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_fixed: the scalars reach past the key");
  if (n > (size_t)FIXED_CHUNK * FIXED_MAXQ) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_fixed: more than 64 workgroups a window");
  const vimz_small_tables* st = head_small_tables(bases);
  if (!st || !st->mult) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_fixed: the key has no tables of multiples (vimz_bases_precompute(7))");
  const int K = head_small_windows(bases->curve);
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  MsmShape sh;
  sh.path = MSM_PATH_FIXED; sh.plan.c = SMALL_C; sh.plan.K = K; sh.plan.nbw = SMALL_NBW; sh.plan.nb = SMALL_NBW * (uint32_t)K; sh.plan.split_ones = 0; sh.plan.tabled = 2;
  sh.Qf = (uint32_t)((n + FIXED_CHUNK - 1) / FIXED_CHUNK); sh.kout = K;
  const BaseTables tb{st->rows, st->n, base_offset, st->c, st->K, 0, st->mult};
  return curve_dispatch(bases->curve, [&](auto cv) {
    typedef decltype(cv) C;
    return head_fused_run(c, scalars, n, K, calls, sums_out, [&](MsmWorkspace& ws, const uint32_t* dsc, uint32_t* pinned) {
      const MsmCall a{c->stream, ws, bases->d + (size_t)AFFINE_WORDS * base_offset, dsc, n, form == VIMZ_FORM_MONTGOMERY, sgn, 0, pinned, nullptr, &tb, nullptr};
      return launch_fixed<C>(a, sh);
    });
  });
}

extern "C" int vimz_test_msm_ones(vimz_ctx* c, const vimz_bases* bases, const uint64_t* scalars, size_t n, size_t row_stride, size_t rows, int form, int kind, uint32_t* out) {
  if (!c || !bases || !scalars || !out || !n || row_stride < n || kind < 0 || kind > 2 || (form != VIMZ_FORM_CANONICAL && form != VIMZ_FORM_MONTGOMERY))
    return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_ones: bad argument");
  if (n > bases->n || n >= (1u << 31)) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_ones: more scalars than the key has points");
  if (!rows || rows > (kind == 2 ? 2 * MSM_ROWS_MAX : 1u)) return fail(c, VIMZ_ERR_INVALID, "vimz_test_msm_ones: rows outside 1..32 (kinds 0 and 1: one row)");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  const int mont = form == VIMZ_FORM_MONTGOMERY;
  const size_t sc_words = 8 * ((rows - 1) * row_stride + n);
  WorkspaceGuard W;
  TailBufs B;
  uint32_t *dsc, *dlvl, *dout;
  TAIL_TRY(B.get(&dsc, sc_words)); TAIL_TRY(B.get(&dlvl, (size_t)XYZZ_WORDS * (ONES_THREADS + ONES_THREADS / 256), 0xff)); TAIL_TRY(B.get(&dout, rows * XYZZ_WORDS, 0xff));
  TAIL_TRY(tail_up(c, dsc, reinterpret_cast<const uint32_t*>(scalars), sc_words));
  const int rc = curve_dispatch(bases->curve, [&](auto cv) {
    typedef decltype(cv) C;
    typedef typename C::Coord F;
    typedef typename C::Scalar S;
    if (kind == 2) {
      OnesDesc ds[2 * MSM_ROWS_MAX];
      for (size_t r = 0; r < rows; r++) ds[r] = OnesDesc{dsc + 8 * r * row_stride, bases->d, dout + (size_t)XYZZ_WORDS * r, n};
      TAIL_TRY(ones_launch_rows<C>(c->stream, W.ws, ds, (uint32_t)rows, mont));
    } else {      // the partial sums, then the tree the product runs over them
      launch_ones<S, F>(c->stream, kind == 1, dsc, bases->d, n, mont, dlvl);
      launch_tree256<F>(c->stream, dlvl, ONES_THREADS, dlvl + (size_t)XYZZ_WORDS * ONES_THREADS, dout);
    }
    return (int)VIMZ_OK;
  });
  if (rc) return rc;
  TAIL_TRY(hipGetLastError());
  TAIL_TRY(tail_down(c, out, dout, rows * XYZZ_WORDS));
  TAIL_TRY(hipStreamSynchronize(c->stream));
  return VIMZ_OK;
}

extern "C" int vimz_test_bases_tables(vimz_ctx* c, const vimz_bases* bases, int window_bits, int which, const uint32_t* wim, size_t count, uint64_t* out_xy) {
  if (!c || !bases || !wim || !out_xy || !count || count > 4096 || (which != 0 && which != 1)) return fail(c, VIMZ_ERR_INVALID, "vimz_test_bases_tables: bad argument");
  const vimz_small_tables* st = window_bits == SMALL_C ? head_small_tables(bases) : nullptr;
  const uint32_t* src = nullptr; size_t n = bases->n; int K = 0;
  if (window_bits == SMALL_C) { if (st) { src = which ? st->mult : st->rows; K = st->K; } }
  else if (!which && bases->tables && bases->table_c == window_bits) { src = bases->tables; K = bases->table_K; }
  if (!src) return fail(c, VIMZ_ERR_INVALID, "vimz_test_bases_tables: the key has no such tables (window tables of window_bits; multiples: window_bits 7 only)");
  for (size_t k = 0; k < count; k++)
    if (wim[3 * k] >= (uint32_t)K || wim[3 * k + 1] >= n || (which && (!wim[3 * k + 2] || wim[3 * k + 2] > SMALL_NBW)))
      return fail(c, VIMZ_ERR_INVALID, "vimz_test_bases_tables: an entry outside the tables (w below K, i below n, m in 1..64)");
  std::lock_guard<std::mutex> g(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  TailBufs B;
  uint32_t *dsel, *dstd;
  TAIL_TRY(B.get(&dsel, (size_t)AFFINE_WORDS * count)); TAIL_TRY(B.get(&dstd, 16 * count));
  for (size_t k = 0; k < count; k++) {
    size_t idx = (size_t)wim[3 * k] * n + wim[3 * k + 1];
    if (which) idx = idx * SMALL_NBW + (wim[3 * k + 2] - 1);
    TAIL_TRY(hipMemcpyAsync(dsel + (size_t)AFFINE_WORDS * k, src + (size_t)AFFINE_WORDS * idx, 4 * (size_t)AFFINE_WORDS, hipMemcpyDeviceToDevice, c->stream));
  }
  field_dispatch(curve_base_field(bases->curve), [&](auto f) { typedef decltype(f) F; launch_points_from_internal<F>(c->stream, dsel, 1, dstd, count); return (int)VIMZ_OK; });
  TAIL_TRY(hipGetLastError());
  TAIL_TRY(tail_down(c, reinterpret_cast<uint32_t*>(out_xy), dstd, 16 * count));
  TAIL_TRY(hipStreamSynchronize(c->stream));
  return VIMZ_OK;
}
#undef TAIL_TRY
#endif  // VIMZ_TESTING
