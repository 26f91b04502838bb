// Multilinear KZG openings of committed vectors over a KZG SRS (vimz_mlkzg_open, vimz_mlkzg_verify): a vector v of n <= N = 2^ℓ elements of BN254 Fr,
// committed as C = Σ v[i]·[tau^i]G1, is opened as the multilinear polynomial whose evaluations over {0,1}^ℓ it lists (bit k of the index = variable k) at a point
// x of Fr^ℓ.  The protocol, the transcript and the verifier are mlkzg_verify.hpp's; what one thread of each kernel does is mlkzg_stage.hpp's.
//
// The kernels work on Fr alone, ML_BLOCK threads a block; a thread writes the slots of its own index, there are no atomics and nothing one workgroup writes is read
// by another workgroup of the same launch: what crosses workgroups crosses a launch.  Every loop bound is an argument.
//   k_mle_fold        one level of the fold, one thread per output; the ℓ + 1 levels lie side by side in one buffer of 2N − 1 elements
//   k_poly_eval3      P_k at r, −r and r² for every level in ONE launch (the level in blockIdx.y): a thread walks ML_CHUNK coefficients once — Horner in r² over the
//                     even ones, the odd ones and all of them — and scales by the power of its chunk's start; the block sums through LDS and writes three partials;
//   k_eval3_sum       one thread per level sums the level's partials and forms E_r = Pe + r·Po, E_(−r) = Pe − r·Po, E_(r²)
//   k_batch_levels    B[j] = Σ_{k: j < N/2^k} q^k·P_k[j], one thread per j
//   k_div_carry, k_div_scan, k_div_chunk      the division of B by (X − u) for the three u (blockIdx.y) as a chunked scan of q_(i−1) = b_i + u·q_i: each chunk's
//                     carry-out with a zero carry-in; ONE workgroup per u that carries across the chunks of a block and across the blocks; the chunks again with
//                     their carry-in, writing Q_u and the remainder B(u)
// The commitments C, C_1 .. C_(ℓ−1), W_r, W_(−r), W_(r²) are vz_msm_device's as it stands.
#include <chrono>
#include "internal.hpp"
#include "mlkzg_verify.hpp"
#ifdef VIMZ_TESTING
#include "../../include/vimz_hip_testing.h"
#include "proof_io.hpp"      // (the hook that holds mlkzg_verify.hpp's Chain against this file's Transcript)
#endif

namespace {

using namespace vz::mlk;
using vz::vz_fail;

#define ML_TRY(x) do { hipError_t _e = (x); if (_e != hipSuccess) return vz_fail(ctx, VIMZ_ERR_HIP, #x, _e); } while (0)

__global__ void __launch_bounds__(ML_BLOCK) k_mle_fold(const Fr* __restrict__ in, size_t n_out, Fr x, Fr* __restrict__ out) {
  const size_t j = blockIdx.x * (size_t)ML_BLOCK + threadIdx.x;
  if (j < n_out) fold_one(j, in, x, out);
}

// grid (n_blocks(n0), levels): block (bx, k) sums the chunks bx·ML_BLOCK .. of level k into part[3·(k·stride + bx) ..]; a block past its level's end leaves at once
__global__ void __launch_bounds__(ML_BLOCK) k_poly_eval3(const Fr* __restrict__ levels, size_t n0, Fr w, Fr wh, int bits, size_t stride, Fr* __restrict__ part) {
  __shared__ Fr sh[3][ML_BLOCK];
  const unsigned k = blockIdx.y, tid = threadIdx.x;
  const size_t len = n0 >> k;
  if ((size_t)blockIdx.x * ML_BLOCK * ML_CHUNK >= len) return;      // (the same for the whole block: before any barrier)
  Fr v[3];
  eval3_chunk(blockIdx.x * (size_t)ML_BLOCK + tid, levels + level_offset(n0, k), len, w, wh, bits, v);
  sh[0][tid] = v[0]; sh[1][tid] = v[1]; sh[2][tid] = v[2];
  __syncthreads();
  for (unsigned s = ML_BLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) { sh[0][tid] = Fr::add(sh[0][tid], sh[0][tid + s]); sh[1][tid] = Fr::add(sh[1][tid], sh[1][tid + s]); sh[2][tid] = Fr::add(sh[2][tid], sh[2][tid + s]); }
    __syncthreads();
  }
  if (tid < 3) part[3 * ((size_t)k * stride + blockIdx.x) + tid] = sh[tid][0];
}
// thread k: evals[u·levels + k] for u = r, −r, r²
__global__ void __launch_bounds__(64) k_eval3_sum(const Fr* __restrict__ part, size_t n0, size_t stride, unsigned nlevels, Fr r, Fr* __restrict__ evals) {
  const unsigned k = threadIdx.x;
  if (k >= nlevels) return;
  Fr o[3];
  eval3_finish(part + 3 * (size_t)k * stride, n_blocks(n0 >> k), r, o);
  evals[k] = o[0]; evals[nlevels + k] = o[1]; evals[2 * nlevels + k] = o[2];
}

__global__ void __launch_bounds__(ML_BLOCK) k_batch_levels(const Fr* __restrict__ levels, size_t n0, unsigned nlevels, Fr q, Fr* __restrict__ out) {
  const size_t j = blockIdx.x * (size_t)ML_BLOCK + threadIdx.x;
  if (j < n0) batch_one(j, levels, n0, nlevels, q, out);
}

// the three points of a division as kernel arguments: u, u^ML_CHUNK, u^(ML_CHUNK·ML_BLOCK); a kernel takes its row's (blockIdx.y) by comparison, not by an index
struct DivPts { Fr u[3], uc[3], ubc[3]; };
__device__ __forceinline__ Fr div_pick(const Fr a[3], unsigned row) { return row == 0 ? a[0] : row == 1 ? a[1] : a[2]; }

__global__ void __launch_bounds__(ML_BLOCK) k_div_carry(const Fr* __restrict__ b, size_t len, size_t nchunks, DivPts pts, Fr* __restrict__ z) {
  const size_t t = blockIdx.x * (size_t)ML_BLOCK + threadIdx.x;
  if (t < nchunks) div_carry(t, b, len, div_pick(pts.u, blockIdx.y), z + blockIdx.y * nchunks);
}
// grid (1, 3): ONE workgroup per u.  Its threads take the blocks of chunks in turn; between the three passes the workgroup's own barrier orders what its threads wrote.
__global__ void __launch_bounds__(ML_BLOCK) k_div_scan(const Fr* __restrict__ z, size_t nchunks, size_t nblocks, DivPts pts, Fr* zb, Fr* ib, Fr* __restrict__ cin) {
  const unsigned row = blockIdx.y;
  const Fr uc = div_pick(pts.uc, row), ubc = div_pick(pts.ubc, row);
  z += row * nchunks; cin += row * nchunks; zb += row * nblocks; ib += row * nblocks;
  for (size_t blk = threadIdx.x; blk < nblocks; blk += ML_BLOCK) div_block_carry(blk, z, nchunks, uc, zb);
  __syncthreads();
  if (threadIdx.x == 0) div_block_scan(zb, nblocks, ubc, ib);
  __syncthreads();
  for (size_t blk = threadIdx.x; blk < nblocks; blk += ML_BLOCK) div_chunk_carries(blk, z, nchunks, uc, ib, cin);
}
__global__ void __launch_bounds__(ML_BLOCK) k_div_chunk(const Fr* __restrict__ b, size_t len, size_t nchunks, DivPts pts, const Fr* __restrict__ cin,
                                                        Fr* __restrict__ quot, size_t quot_stride, Fr* __restrict__ rem) {
  const size_t t = blockIdx.x * (size_t)ML_BLOCK + threadIdx.x;
  if (t < nchunks) div_chunk(t, b, len, div_pick(pts.u, blockIdx.y), cin + blockIdx.y * nchunks, quot + blockIdx.y * quot_stride, rem + blockIdx.y);
}

unsigned ml_grid(size_t threads) { return (unsigned)((threads + ML_BLOCK - 1) / ML_BLOCK); }
int bitlen(size_t v) { int b = 0; while (v) { b++; v >>= 1; } return b; }
Fr pow_small(Fr base, unsigned e) { Fr acc = Fr::one(); for (; e; e >>= 1) { if (e & 1u) acc = Fr::mul(acc, base); base = Fr::sqr(base); } return acc; }
double since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

// the device buffers of one opening (or of one hook call), ONE allocation carved into arrays of elements; freed when this goes out of scope
struct MlDev {
  Fr* base = nullptr;
  Fr *levels = nullptr, *bv = nullptr, *quot = nullptr, *z = nullptr, *cin = nullptr, *zb = nullptr, *ib = nullptr, *part = nullptr, *evals = nullptr, *rem = nullptr;
  size_t n0 = 0, nchunks = 0, nblocks = 0;
  ~MlDev() { if (base) hipFree(base); }
  // levels_len elements of levels; everything else sized for polynomials of up to n0 coefficients and nlevels levels
  hipError_t alloc(size_t levels_len, size_t n0_, unsigned nlevels) {
    n0 = n0_; nchunks = n_chunks(n0); nblocks = n_blocks(n0);
    const size_t sizes[10] = {levels_len, n0, 3 * n0, 3 * nchunks, 3 * nchunks, 3 * nblocks, 3 * nblocks, 3 * nblocks * nlevels, 3 * (size_t)nlevels, 3};
    size_t total = 0;
    for (size_t s : sizes) total += s;
    hipError_t e = hipMalloc((void**)&base, sizeof(Fr) * total);
    if (e != hipSuccess) { base = nullptr; return e; }
    Fr** slots[10] = {&levels, &bv, &quot, &z, &cin, &zb, &ib, &part, &evals, &rem};
    Fr* p = base;
    for (int i = 0; i < 10; i++) { *slots[i] = p; p += sizes[i]; }
    return hipSuccess;
  }
};

// ---- the stages, queued on the context's stream (the caller holds its lock and has set the device) ---------------------------------------------------------------
// levels k = 1 .. nlevels from level 0 (n0 = 2^nlevels elements at d.levels) and the point x (Montgomery)
int run_folds(vimz_ctx* ctx, MlDev& d, unsigned nlevels, const Fr* x) {
  for (unsigned k = 0; k < nlevels; k++) {
    const size_t n_out = d.n0 >> (k + 1);
    hipLaunchKernelGGL(k_mle_fold, dim3(ml_grid(n_out)), dim3(ML_BLOCK), 0, ctx->stream, (const Fr*)(d.levels + level_offset(d.n0, k)), n_out, x[k], d.levels + level_offset(d.n0, k + 1));
    ML_TRY(hipGetLastError());
  }
  return VIMZ_OK;
}
// d.evals[u·nlevels + k] = P_k(u) for u = r, −r, r² over the levels at d.levels (level k: n0 >> k >= 1 coefficients)
int run_eval3(vimz_ctx* ctx, MlDev& d, unsigned nlevels, const Fr& r) {
  const Fr w = Fr::sqr(r), wh = pow_small(w, ML_CHUNK / 2);
  hipLaunchKernelGGL(k_poly_eval3, dim3((unsigned)d.nblocks, nlevels), dim3(ML_BLOCK), 0, ctx->stream, (const Fr*)d.levels, d.n0, w, wh, bitlen(d.nchunks - 1), d.nblocks, d.part);
  ML_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_eval3_sum, dim3(1), dim3(64), 0, ctx->stream, (const Fr*)d.part, d.n0, d.nblocks, nlevels, r, d.evals);
  ML_TRY(hipGetLastError());
  return VIMZ_OK;
}
int run_batch(vimz_ctx* ctx, MlDev& d, unsigned nlevels, const Fr& q) {
  hipLaunchKernelGGL(k_batch_levels, dim3(ml_grid(d.n0)), dim3(ML_BLOCK), 0, ctx->stream, (const Fr*)d.levels, d.n0, nlevels, q, d.bv);
  ML_TRY(hipGetLastError());
  return VIMZ_OK;
}
// d.quot[j·n0 ..] = (B − B(u_j)) / (X − u_j) and d.rem[j] = B(u_j) for the polynomial of `len` <= n0 coefficients at d.bv
int run_divide(vimz_ctx* ctx, MlDev& d, size_t len, const Fr u[3]) {
  DivPts pts;
  for (int j = 0; j < 3; j++) { pts.u[j] = u[j]; pts.uc[j] = pow_small(u[j], ML_CHUNK); pts.ubc[j] = pow_small(pts.uc[j], ML_BLOCK); }
  const size_t nchunks = n_chunks(len), nblocks = n_blocks(len);
  hipLaunchKernelGGL(k_div_carry, dim3(ml_grid(nchunks), 3), dim3(ML_BLOCK), 0, ctx->stream, (const Fr*)d.bv, len, nchunks, pts, d.z);
  ML_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_div_scan, dim3(1, 3), dim3(ML_BLOCK), 0, ctx->stream, (const Fr*)d.z, nchunks, nblocks, pts, d.zb, d.ib, d.cin);
  ML_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_div_chunk, dim3(ml_grid(nchunks), 3), dim3(ML_BLOCK), 0, ctx->stream, (const Fr*)d.bv, len, nchunks, pts, (const Fr*)d.cin, d.quot, d.n0, d.rem);
  ML_TRY(hipGetLastError());
  return VIMZ_OK;
}

}  // namespace

namespace vz {
int vz_mlkzg_open_device(vimz_ctx* ctx, const vimz_bases* srs, int field, const uint32_t* d_vec, size_t n, uint32_t logn, const uint64_t* point,
                         uint64_t comm_out[8], uint64_t eval_out[4], uint64_t* proof, size_t cap_words, double seconds[4]) {
  auto bad = [&](const char* m) { return vz_fail(ctx, VIMZ_ERR_INVALID, (std::string("mlkzg open: ") + m).c_str()); };
  if (logn == 0 || logn > (uint32_t)ML_MAX_LOGN) return bad("logn is 1 .. 26");
  const size_t N = (size_t)1 << logn;
  if (n == 0 || n > N) return bad("the vector has 1 .. 2^logn elements");
  if (field != VIMZ_FIELD_BN254_FR || srs->curve != VIMZ_CURVE_BN254_G1) return bad("the vector is over BN254 Fr and the key on BN254 G1");
  if (srs->n < N) return bad("the SRS is shorter than 2^logn");
  if (cap_words < proof_words(logn)) return bad("the proof buffer is shorter than vimz_mlkzg_proof_words(logn)");
  std::vector<Fr> x(logn);
  for (uint32_t k = 0; k < logn; k++) if (!get_fr(point + 4 * k, &x[k])) return bad("a point element is not below r");
  hipStream_t s = ctx->stream;
  MlDev d;
  ML_TRY(d.alloc(level_offset(N, logn + 1), N, logn));

  // 1. the levels and their commitments
  auto t0 = std::chrono::steady_clock::now();
  ML_TRY(hipMemcpyAsync(d.levels, d_vec, sizeof(Fr) * n, hipMemcpyDeviceToDevice, s));
  if (n < N) ML_TRY(hipMemsetAsync(d.levels + n, 0, sizeof(Fr) * (N - n), s));
  int rc = run_folds(ctx, d, logn, x.data());
  if (rc) return rc;
  if ((rc = vz_msm_device(ctx, srs, 0, d_vec, n, 1, 0, comm_out, VIMZ_FORM_CANONICAL))) return rc;
  for (uint32_t k = 1; k < logn; k++)
    if ((rc = vz_msm_device(ctx, srs, 0, (const uint32_t*)(d.levels + level_offset(N, k)), N >> k, 1, 0, proof + at_ck(logn) + 8 * (k - 1), VIMZ_FORM_CANONICAL))) return rc;
  Fr y;
  ML_TRY(hipMemcpyAsync(&y, d.levels + level_offset(N, logn), sizeof(Fr), hipMemcpyDeviceToHost, s));
  ML_TRY(hipStreamSynchronize(s));
  put_fr(eval_out, y);
  if (seconds) seconds[0] = since(t0);

  // 2. the evaluations at r, −r, r²
  t0 = std::chrono::steady_clock::now();
  Rounds R;
  const Fr r = R.round_r(logn, comm_out, point, eval_out, proof + at_ck(logn));
  if (r.is_zero()) return bad("the challenge r is zero");
  if ((rc = run_eval3(ctx, d, logn, r))) return rc;
  std::vector<Fr> E(3 * (size_t)logn);
  ML_TRY(hipMemcpyAsync(E.data(), d.evals, sizeof(Fr) * E.size(), hipMemcpyDeviceToHost, s));
  ML_TRY(hipStreamSynchronize(s));
  for (size_t i = 0; i < E.size(); i++) put_fr(proof + at_evals(logn) + 4 * i, E[i]);
  if (seconds) seconds[1] = since(t0);

  // 3. B = Σ q^k·P_k and its three quotients
  t0 = std::chrono::steady_clock::now();
  const Fr q = R.round_q(logn, proof + at_evals(logn));
  if ((rc = run_batch(ctx, d, logn, q))) return rc;
  const Fr u[3] = {r, Fr::neg(r), Fr::sqr(r)};
  Fr rem[3];
  if ((rc = run_divide(ctx, d, N, u))) return rc;
  ML_TRY(hipMemcpyAsync(rem, d.rem, sizeof(rem), hipMemcpyDeviceToHost, s));
  ML_TRY(hipStreamSynchronize(s));
  for (int j = 0; j < 3; j++) {
    Fr b = Fr::zero();
    for (uint32_t k = logn; k-- > 0;) b = Fr::add(Fr::mul(b, q), E[(size_t)j * logn + k]);
    if (!b.eq(rem[j])) return bad("a division's remainder is not the batched evaluation");
  }
  if (seconds) seconds[2] = since(t0);

  // 4. W_u = commit(Q_u) over N − 1 powers
  t0 = std::chrono::steady_clock::now();
  for (int j = 0; j < 3; j++)
    if ((rc = vz_msm_device(ctx, srs, 0, (const uint32_t*)(d.quot + (size_t)j * N), N - 1, 1, 0, proof + at_w(logn) + 8 * j, VIMZ_FORM_CANONICAL))) return rc;
  if (seconds) seconds[3] = since(t0);
  return VIMZ_OK;
}
int vz_mlkzg_open_exact(vimz_ctx* ctx, const vimz_bases* srs, const uint32_t* d_vec, size_t n, uint32_t logn, const uint64_t* point, uint64_t comm_out[8],
                        uint64_t eval_out[4], uint64_t* proof, size_t cap_words, double seconds[4]) {
  uint32_t least = 1;
  while (least < (uint32_t)ML_MAX_LOGN && ((size_t)1 << least) < n) least++;
  if (logn != least) return vz_fail(ctx, VIMZ_ERR_INVALID, "mlkzg open: logn is not the least with 2^logn >= the vector's length");
  return vz_mlkzg_open_device(ctx, srs, VIMZ_FIELD_BN254_FR, d_vec, n, logn, point, comm_out, eval_out, proof, cap_words, seconds);
}
}  // namespace vz

extern "C" size_t vimz_mlkzg_proof_words(uint32_t logn) { return logn == 0 || logn > (uint32_t)ML_MAX_LOGN ? 0 : proof_words(logn); }

extern "C" int vimz_mlkzg_open(vimz_ctx* ctx, const vimz_bases* srs, const vimz_vec* vec, size_t offset, size_t n, uint32_t logn, const uint64_t* point, uint64_t comm_out[8],
                               uint64_t eval_out[4], uint64_t* proof, size_t cap_words, double seconds[4]) {
  if (!ctx) return VIMZ_ERR_INVALID;
  if (!srs || !vec || !point || !comm_out || !eval_out || !proof) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_mlkzg_open: NULL argument");
  if (offset > vec->n || n > vec->n - offset) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_mlkzg_open: offset + n is past the vector's end");
  std::lock_guard<std::mutex> g(ctx->mu);
  ML_TRY(hipSetDevice(ctx->device));
  return vz::vz_mlkzg_open_device(ctx, srs, vec->field, vec->d + 8 * offset, n, logn, point, comm_out, eval_out, proof, cap_words, seconds);
}

extern "C" int vimz_mlkzg_verify(const uint64_t vk_g2[16], const uint64_t comm[8], uint32_t logn, const uint64_t* point, const uint64_t eval[4], const uint64_t* proof,
                                 size_t n_words, uint32_t* result) {
  if (!vk_g2 || !comm || !point || !eval || !proof || !result || logn == 0) return VIMZ_ERR_INVALID;
  *result = verify(vk_g2, comm, logn, point, eval, proof, n_words);
  return VIMZ_OK;
}

#ifdef VIMZ_TESTING
namespace {
// n canonical elements below r from the host to Montgomery on the device, and back
bool hook_in(const uint64_t* src, size_t n, std::vector<Fr>& out) {
  out.resize(n);
  for (size_t i = 0; i < n; i++) if (!get_fr(src + 4 * i, &out[i])) return false;
  return true;
}
int hook_out(vimz_ctx* ctx, const Fr* dev, size_t n, uint64_t* dst) {
  if (!n || !dst) return VIMZ_OK;
  std::vector<Fr> h(n);
  ML_TRY(hipMemcpyAsync(h.data(), dev, sizeof(Fr) * n, hipMemcpyDeviceToHost, ctx->stream));
  ML_TRY(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < n; i++) put_fr(dst + 4 * i, h[i]);
  return VIMZ_OK;
}
int hook_bad(vimz_ctx* ctx, const char* who) { return vz_fail(ctx, VIMZ_ERR_INVALID, (std::string(who) + ": bad argument").c_str()); }
}  // namespace

extern "C" int vimz_test_mlkzg_shape(uint32_t out[2]) {
  if (!out) return VIMZ_ERR_INVALID;
  out[0] = ML_BLOCK; out[1] = ML_CHUNK;
  return VIMZ_OK;
}
extern "C" int vimz_test_mlkzg_chains(const char* label, const char* tag, const uint8_t* data, size_t n, uint64_t out[4]) {
  if (!label || !tag || (!data && n) || !out) return VIMZ_ERR_INVALID;
  Transcript a(label); vz::mlk::Chain b(label);
  uint32_t ca[4];
  for (int round = 0; round < 2; round++) {      // two absorptions and two challenges: the state carries over
    a.absorb_bytes(tag, data, n); b.absorb_bytes(tag, data, n);
    a.challenge(ca);
    const Fr cb = Fr::from_mont(b.challenge());
    memcpy(out, ca, 16); memcpy(out + 2, cb.v, 16);
    if (memcmp(out, out + 2, 16)) return VIMZ_OK;      // (the caller sees the first pair that differs)
  }
  return VIMZ_OK;
}
extern "C" int vimz_test_mlkzg_fold(vimz_ctx* ctx, const uint64_t* vec, uint32_t logn, const uint64_t* point, uint64_t* levels_out) {
  if (!ctx) return VIMZ_ERR_INVALID;
  std::vector<Fr> v, x;
  if (!vec || !point || !levels_out || logn == 0 || logn > 20 || !hook_in(vec, (size_t)1 << logn, v) || !hook_in(point, logn, x)) return hook_bad(ctx, "vimz_test_mlkzg_fold");
  const size_t N = (size_t)1 << logn;
  std::lock_guard<std::mutex> g(ctx->mu);
  ML_TRY(hipSetDevice(ctx->device));
  MlDev d;
  ML_TRY(d.alloc(level_offset(N, logn + 1), N, logn));
  ML_TRY(hipMemcpyAsync(d.levels, v.data(), sizeof(Fr) * N, hipMemcpyHostToDevice, ctx->stream));
  if (int rc = run_folds(ctx, d, logn, x.data())) return rc;
  return hook_out(ctx, d.levels, level_offset(N, logn + 1), levels_out);
}
extern "C" int vimz_test_mlkzg_eval3(vimz_ctx* ctx, const uint64_t* levels, size_t n0, uint32_t nlevels, const uint64_t r[4], uint64_t* evals_out) {
  if (!ctx) return VIMZ_ERR_INVALID;
  std::vector<Fr> v, rr;
  if (!levels || !r || !evals_out || nlevels == 0 || nlevels > 21 || n0 == 0 || n0 > ((size_t)1 << 20) || (n0 >> (nlevels - 1)) == 0 ||
      !hook_in(levels, level_offset(n0, nlevels), v) || !hook_in(r, 1, rr)) return hook_bad(ctx, "vimz_test_mlkzg_eval3");
  std::lock_guard<std::mutex> g(ctx->mu);
  ML_TRY(hipSetDevice(ctx->device));
  MlDev d;
  ML_TRY(d.alloc(v.size(), n0, nlevels));
  ML_TRY(hipMemcpyAsync(d.levels, v.data(), sizeof(Fr) * v.size(), hipMemcpyHostToDevice, ctx->stream));
  if (int rc = run_eval3(ctx, d, nlevels, rr[0])) return rc;
  return hook_out(ctx, d.evals, 3 * (size_t)nlevels, evals_out);
}
extern "C" int vimz_test_mlkzg_batch(vimz_ctx* ctx, const uint64_t* levels, size_t n0, uint32_t nlevels, const uint64_t q[4], uint64_t* out) {
  if (!ctx) return VIMZ_ERR_INVALID;
  std::vector<Fr> v, qq;
  if (!levels || !q || !out || nlevels == 0 || nlevels > 21 || n0 == 0 || n0 > ((size_t)1 << 20) || (n0 >> (nlevels - 1)) == 0 ||
      !hook_in(levels, level_offset(n0, nlevels), v) || !hook_in(q, 1, qq)) return hook_bad(ctx, "vimz_test_mlkzg_batch");
  std::lock_guard<std::mutex> g(ctx->mu);
  ML_TRY(hipSetDevice(ctx->device));
  MlDev d;
  ML_TRY(d.alloc(v.size(), n0, nlevels));
  ML_TRY(hipMemcpyAsync(d.levels, v.data(), sizeof(Fr) * v.size(), hipMemcpyHostToDevice, ctx->stream));
  if (int rc = run_batch(ctx, d, nlevels, qq[0])) return rc;
  return hook_out(ctx, d.bv, n0, out);
}
extern "C" int vimz_test_mlkzg_divide(vimz_ctx* ctx, const uint64_t* coeffs, size_t n, const uint64_t u[12], uint64_t* quot_out, uint64_t rem_out[12], uint64_t* carry_out,
                                      uint64_t* carry_in_out) {
  if (!ctx) return VIMZ_ERR_INVALID;
  std::vector<Fr> v, uu;
  if (!coeffs || !u || !quot_out || !rem_out || n == 0 || n > ((size_t)1 << 20) || !hook_in(coeffs, n, v) || !hook_in(u, 3, uu)) return hook_bad(ctx, "vimz_test_mlkzg_divide");
  std::lock_guard<std::mutex> g(ctx->mu);
  ML_TRY(hipSetDevice(ctx->device));
  MlDev d;
  ML_TRY(d.alloc(0, n, 1));
  ML_TRY(hipMemcpyAsync(d.bv, v.data(), sizeof(Fr) * n, hipMemcpyHostToDevice, ctx->stream));
  if (int rc = run_divide(ctx, d, n, uu.data())) return rc;
  for (int j = 0; j < 3; j++) if (int rc = hook_out(ctx, d.quot + (size_t)j * n, n - 1, quot_out + 4 * (size_t)j * (n - 1))) return rc;
  if (int rc = hook_out(ctx, d.rem, 3, rem_out)) return rc;
  if (int rc = hook_out(ctx, d.z, 3 * d.nchunks, carry_out)) return rc;
  return hook_out(ctx, d.cin, 3 * d.nchunks, carry_in_out);
}
#endif
