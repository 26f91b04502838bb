// k_scale_points: out_i = k·P_i over points of BN254 G1 for ONE scalar k (g16_powers.hpp) — the step of a Groth16 set-up from a powers-of-tau string that
// applies 1/delta to the l and h queries, whose points come from group operations and so have no known scalar for k_fixed_mul's window table.
//
// One thread per point, double-and-add from the top bit over the XYZZ accumulator of ec.hpp with the affine input as the addend (a mixed addition: 8M + 2S
// against the 12M + 2S of a full one).  Every thread walks the same bits, so a wave never diverges on them: the scalar's word is a uniform load, the only
// data-dependent branches are add_mixed's own (identity, doubling, cancellation).  Coordinates stay in the 8 x 32 Montgomery form the points arrive and leave
// in, as in k_fixed_mul; one inversion per point ends the thread (380 of its ~4 300 products).
#include "g16_powers.hpp"
#ifdef VIMZ_TESTING
#include "../../include/vimz_hip_testing.h"
#endif

namespace {

constexpr unsigned SCALE_BLOCK = 64;      // one wave per workgroup: 190 VGPRs hold two waves on a SIMD, and small queries still spread over the CUs
constexpr int SCALAR_BITS = 254;      // r < 2^254

__global__ void __launch_bounds__(SCALE_BLOCK) k_scale_points(const G1Aff* in, size_t n, const uint32_t* __restrict__ k_canon, G1Aff* out /* may be in */) {
  const size_t i = blockIdx.x * (size_t)SCALE_BLOCK + threadIdx.x;
  if (i >= n) return;
  const G1Aff p = in[i];
  XYZZ<Fq> acc = XYZZ<Fq>::identity();
#pragma unroll 1
  for (int b = SCALAR_BITS - 1; b >= 0; b--) {
    acc = dbl(acc);                                     // (the identity until the scalar's top bit: a compare and a branch)
    if ((k_canon[b >> 5] >> (b & 31)) & 1u) add_mixed(acc, p);
  }
  out[i] = to_affine(acc);
}

}  // namespace

hipError_t g16_scale_points(hipStream_t s, const G1Aff* in, size_t n, const uint32_t* k_canon, G1Aff* out) {
  if (!n) return hipSuccess;
  if (!in || !out || !k_canon || n > ((size_t)1 << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_scale_points, dim3((unsigned)((n + SCALE_BLOCK - 1) / SCALE_BLOCK)), dim3(SCALE_BLOCK), 0, s, in, n, k_canon, out);
  return hipGetLastError();
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
#endif
