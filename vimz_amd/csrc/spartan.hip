// CompressedSNARK::{prove, verify} for the Nova IVC object (reference call sites
// vimz/src/nova_snark_backend/mod.rs:52-67: `CompressedSNARK::<_, _, _, _, S<G1>, S<G2>>::{setup, prove, verify}` with
// nova_scotia::S = nova-snark 0.23.0's `spartan::snark::RelaxedR1CSSNARK<G, ipa_pc::EvaluationEngine<G>>`).  README.md:196 counts
// this step into the total proof time; after folding takes seconds it is the larger part of it (≈13 s on the reference's CPU).
//
// nova-snark is not vendored, so — like the augmented circuits — this is our own statement of the same
// construction, NOT byte-compatible with the crate's proof object: Spartan's two sum-checks for relaxed R1CS followed by
// inner-product-argument openings of the committed vectors, made non-interactive over a SHA3-256 transcript.  An independent
// verifier written against this description lives in tests/_spartan.py (the oracle side); the product's own verifier is below.
//
// For one relaxed instance  U = (comm_W, comm_E, u, X0, X1)  with witness vectors Z (n wires: u at wire 0, X at the last two) and
// E (m rows) over shape (A, B, C), padded to M = 2^s rows and N = 2^t columns:
//   1. tau in F^s from the transcript;  outer sum-check (degree 3, s rounds, top variable first) of
//        sum_x eq(tau, x) · (Az(x)·Bz(x) − u·Cz(x) − E(x)) = 0          -> point rx, claims va, vb, vc, ve (= Az, Bz, Cz, E at rx)
//   2. rho from the transcript;  inner sum-check (degree 2, t rounds) of
//        va + rho·vb + rho²·vc = sum_y M(y)·Z(y),   M(y) = sum_x eq(rx, x)·(A + rho·B + rho²·C)(x, y)      -> point ry
//      the verifier evaluates M(ry) from the sparse matrices itself and needs Z(ry) = W'(ry) + u·eq(ry,0) + X0·eq(ry,n−2) + X1·eq(ry,n−1),
//      W' = Z with the three public entries zeroed — the vector comm_W commits to (bases: wire i ↦ ck[i−1]);
//   3. inner-product arguments:  <W', eq(ry,·)> = eval_W under comm_W  and  <E, eq(rx,·)> = ve under comm_E.
// IPA (Bulletproofs, inverse-free folding): P = <a,G> + <a,b>·U';  per round  L = <a_L,G_R> + <a_L,b_R>·U',  R = <a_R,G_L> + <a_R,b_L>·U',
// challenge x,  a' = x·a_L + a_R,  b' = b_L + x·b_R,  G' = G_L + x·G_R,  P' = R + x·P + x²·L;  final check P = a·G + a·b·U'.
// All challenges are 128 bits.  The compressed proof of an IVC = the two running instances, the last fresh secondary instance and
// one such argument for each of the three (the fresh one with u = 1, E = 0), plus (steps, z_0, z_n) for the hash checks.
//
// GPU work: (A,B,C)·Z and the transposed products by the SpMV kernels of the fold (r1cs_ops.hpp), the sum-check rounds by
// reduction + bind kernels over vectors resident in HBM (one 96-byte read-back per round), the IPA rounds by the Pippenger MSM
// of the fold (msm.hpp) and a per-point double-and-add kernel for the generator folding.
#include "ivc_internal.hpp"
#include "ec_mem.hpp"
#include "proof_io.hpp"
#include "merge_internal.hpp"
#include "cyclefold_merge_internal.hpp"
#include "cf_compressed_parse.hpp"
#ifdef VIMZ_TESTING
#include "../../include/vimz_hip_testing.h"
#endif

namespace {

// ---- kernels -------------------------------------------------------------------------------------------------------------------------
template <class F, int K>
__device__ __forceinline__ void block_reduce_store(F (&acc)[K], uint32_t* __restrict__ partial) {
  __shared__ uint32_t sh[K * 256 * 8];
  const uint32_t t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < K; k++)
#pragma unroll
    for (int w = 0; w < 8; w++) sh[(k * 256 + t) * 8 + w] = acc[k].v[w];
  __syncthreads();
  for (uint32_t d = 128; d > 0; d >>= 1) {
    if (t < d) {
#pragma unroll
      for (int k = 0; k < K; k++) {
        F a, b;
#pragma unroll
        for (int w = 0; w < 8; w++) { a.v[w] = sh[(k * 256 + t) * 8 + w]; b.v[w] = sh[(k * 256 + t + d) * 8 + w]; }
        a = F::add(a, b);
#pragma unroll
        for (int w = 0; w < 8; w++) sh[(k * 256 + t) * 8 + w] = a.v[w];
      }
    }
    __syncthreads();
  }
  if (t == 0)
#pragma unroll
    for (int k = 0; k < K; k++) { F a; for (int w = 0; w < 8; w++) a.v[w] = sh[(k * 256) * 8 + w]; store_fe(partial, (size_t)blockIdx.x * K + k, a); }
}

// out[k] = sum over blocks of partial[blk][k]   (one workgroup)
template <class F, int K>
__global__ void __launch_bounds__(256) k_sum_partials(const uint32_t* __restrict__ partial, uint32_t nblocks, uint32_t* __restrict__ out) {
  F acc[K];
  for (int k = 0; k < K; k++) acc[k] = F::zero();
  for (uint32_t b = threadIdx.x; b < nblocks; b += 256)
    for (int k = 0; k < K; k++) acc[k] = F::add(acc[k], load_fe<F>(partial, (size_t)b * K + k));
  block_reduce_store<F, K>(acc, out);
}

// eq table doubling: the newly processed variable becomes the top bit of the index
template <class F>
__global__ void __launch_bounds__(256) k_eq_step(uint32_t* __restrict__ tab, size_t len, F tau) {
  VZ_GRID_STRIDE(i, len) { const F lo = load_fe<F>(tab, i), hi = F::mul(lo, tau); store_fe(tab, i + len, hi); store_fe(tab, i, F::sub(lo, hi)); }
}

// outer round: evaluations at 0, 2, 3 of the round polynomial (pairs (i, i + half): the top remaining variable is bound)
template <class F>
__global__ void __launch_bounds__(256) k_sc_outer(const uint32_t* __restrict__ eq, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                  const uint32_t* __restrict__ c, const uint32_t* __restrict__ e, size_t half, F u, uint32_t* __restrict__ partial) {
  F acc[3] = {F::zero(), F::zero(), F::zero()};
  VZ_GRID_STRIDE(i, half) {
    F q0 = load_fe<F>(eq, i), a0 = load_fe<F>(a, i), b0 = load_fe<F>(b, i), c0 = load_fe<F>(c, i), e0 = e ? load_fe<F>(e, i) : F::zero();
    const F q1 = load_fe<F>(eq, i + half), a1 = load_fe<F>(a, i + half), b1 = load_fe<F>(b, i + half), c1 = load_fe<F>(c, i + half), e1 = e ? load_fe<F>(e, i + half) : F::zero();
    const F dq = F::sub(q1, q0), da = F::sub(a1, a0), db = F::sub(b1, b0), dc = F::sub(c1, c0), de = F::sub(e1, e0);
    acc[0] = F::add(acc[0], F::mul(q0, F::sub(F::sub(F::mul(a0, b0), F::mul(u, c0)), e0)));
    q0 = F::add(q1, dq); a0 = F::add(a1, da); b0 = F::add(b1, db); c0 = F::add(c1, dc); e0 = F::add(e1, de);      // t = 2
    acc[1] = F::add(acc[1], F::mul(q0, F::sub(F::sub(F::mul(a0, b0), F::mul(u, c0)), e0)));
    q0 = F::add(q0, dq); a0 = F::add(a0, da); b0 = F::add(b0, db); c0 = F::add(c0, dc); e0 = F::add(e0, de);      // t = 3
    acc[2] = F::add(acc[2], F::mul(q0, F::sub(F::sub(F::mul(a0, b0), F::mul(u, c0)), e0)));
  }
  block_reduce_store<F, 3>(acc, partial);
}
// inner round: evaluations at 0 and 2 of m(t)·z(t)
template <class F>
__global__ void __launch_bounds__(256) k_sc_inner(const uint32_t* __restrict__ m, const uint32_t* __restrict__ z, size_t half, uint32_t* __restrict__ partial) {
  F acc[2] = {F::zero(), F::zero()};
  VZ_GRID_STRIDE(i, half) {
    const F m0 = load_fe<F>(m, i), z0 = load_fe<F>(z, i), m1 = load_fe<F>(m, i + half), z1 = load_fe<F>(z, i + half);
    acc[0] = F::add(acc[0], F::mul(m0, z0));
    acc[1] = F::add(acc[1], F::mul(F::add(m1, F::sub(m1, m0)), F::add(z1, F::sub(z1, z0))));
  }
  block_reduce_store<F, 2>(acc, partial);
}
struct BindSet { uint32_t* p[5]; int n; };
template <class F>
__global__ void __launch_bounds__(256) k_bind(BindSet s, size_t half, F r) {
  for (int v = 0; v < s.n; v++) {
    uint32_t* x = s.p[v];
    if (!x) continue;
    VZ_GRID_STRIDE(i, half) { const F lo = load_fe<F>(x, i), hi = load_fe<F>(x, i + half); store_fe(x, i, F::add(lo, F::mul(r, F::sub(hi, lo)))); }
  }
}
// <a_L, b_R> and <a_R, b_L>
template <class F>
__global__ void __launch_bounds__(256) k_dot2(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, size_t half, uint32_t* __restrict__ partial) {
  F acc[2] = {F::zero(), F::zero()};
  VZ_GRID_STRIDE(i, half) {
    acc[0] = F::add(acc[0], F::mul(load_fe<F>(a, i), load_fe<F>(b, i + half)));
    acc[1] = F::add(acc[1], F::mul(load_fe<F>(a, i + half), load_fe<F>(b, i)));
  }
  block_reduce_store<F, 2>(acc, partial);
}
template <class F>
__global__ void __launch_bounds__(256) k_ipa_fold_vec(uint32_t* __restrict__ a, uint32_t* __restrict__ b, size_t half, F x) {
  VZ_GRID_STRIDE(i, half) {
    store_fe(a, i, F::add(F::mul(x, load_fe<F>(a, i)), load_fe<F>(a, i + half)));
    store_fe(b, i, F::add(load_fe<F>(b, i), F::mul(x, load_fe<F>(b, i + half))));
  }
}
// G[i] <- G[i] + x·G[i + half]   (x: 128 bits; affine points in the resident 9x29 form, identity = (0,0))
template <class G>
__global__ void __launch_bounds__(256) k_ipa_fold_bases(uint32_t* __restrict__ bases, size_t half, uint4 xw) {
  const uint32_t x[4] = {xw.x, xw.y, xw.z, xw.w};
  VZ_GRID_STRIDE(i, half) {
    const Affine<G> lo = load_affine<G>(bases, (uint32_t)i), hi = load_affine<G>(bases, (uint32_t)(i + half));
    XYZZ<G> acc = XYZZ<G>::identity();
    for (int bit = 127; bit >= 0; bit--) {
      acc = dbl(acc);
      if ((x[bit >> 5] >> (bit & 31)) & 1u) add_mixed(acc, hi);
    }
    add_mixed(acc, lo);
    const Affine<G> r = to_affine(acc);
    store_affine<G>(bases, i, r);
  }
}
// out = x + r·y + r2·z
template <class F>
__global__ void __launch_bounds__(256) k_combine3(size_t n, const uint32_t* __restrict__ x, const uint32_t* __restrict__ y, const uint32_t* __restrict__ z, F r, F r2, uint32_t* __restrict__ out) {
  VZ_GRID_STRIDE(i, n) store_fe(out, i, F::add(load_fe<F>(x, i), F::add(F::mul(r, load_fe<F>(y, i)), F::mul(r2, load_fe<F>(z, i)))));
}
// out[0..N): the committed part of Z (public entries — wire 0 and the last n_pub wires — zeroed), zero-padded
template <class F>
__global__ void __launch_bounds__(256) k_committed_part(const uint32_t* __restrict__ Z, size_t nw, size_t n_pub, size_t N, uint32_t* __restrict__ out) {
  VZ_GRID_STRIDE(i, N) store_fe(out, i, (i == 0 || i + n_pub >= nw) ? F::zero() : load_fe<F>(Z, i));
}

// b of the W opening: eq(ry, ·) with the public slots (wire 0 = u, the last n_pub wires = X0, X1, ...) and the padding above the last wire
// zeroed.  Those positions of the opened vector are NOT part of what comm_W may say about Z: their generators are live and honest
// commitments never use them, so without the mask a prover could hide a correction of (u, X) there and prove the relation for
// a z whose public entries differ from the instance's.
template <class F>
__global__ void __launch_bounds__(256) k_mask_public(uint32_t* __restrict__ b, size_t nw, size_t n_pub, size_t N) {
  VZ_GRID_STRIDE(i, N) if (i == 0 || i + n_pub >= nw) store_fe(b, i, F::zero());
}

// ---- per-side resident data -----------------------------------------------------------------------------------------------------------
struct SideDev {
  CsrDev A{}, B{}, C{}; const uint32_t* dict = nullptr; const uint32_t* items = nullptr; uint32_t n_long = 0, n_med = 0;     // the shape
  CsrDev At{}, Bt{}, Ct{}; const uint32_t* items_t = nullptr; uint32_t n_long_t = 0, n_med_t = 0;                            // its transpose
  uint32_t n_w = 0, n_c = 0, s = 0, t = 0;
  size_t M = 0, N = 0;
  uint32_t *eq = nullptr, *va = nullptr, *vb = nullptr, *vc = nullptr, *ve = nullptr, *vm = nullptr, *vz = nullptr;   // max(M, N) elements each
  uint32_t* G = nullptr;        // max(M, N) affine points, folded in place by the IPA
  uint32_t* partial = nullptr;  // reduction scratch
  uint32_t* pin = nullptr;      // pinned read-back (a few elements)
};
struct SpartanCache { SideDev side[2]; std::vector<void*> owned; MsmWorkspace ws; G1Aff ipa_u1; G2Aff ipa_u2; bool ready = false; };

constexpr unsigned RED_BLOCKS = 512;

// scratch of one side for padded shapes of up to `big` = max(M, N) elements
hipError_t side_alloc(SideDev& S, size_t big, std::vector<void*>& owned) {
  hipError_t e;
  uint32_t** vecs[] = {&S.eq, &S.va, &S.vb, &S.vc, &S.ve, &S.vm, &S.vz};
  for (auto pv : vecs) { if ((e = hipMalloc((void**)pv, 32 * big)) != hipSuccess) return e; owned.push_back(*pv); }
  if ((e = hipMalloc((void**)&S.G, 4 * (size_t)AFFINE_WORDS * big)) != hipSuccess) return e; owned.push_back(S.G);
  if ((e = hipMalloc((void**)&S.partial, 32 * 3 * (RED_BLOCKS + 1))) != hipSuccess) return e; owned.push_back(S.partial);
  return hipHostMalloc((void**)&S.pin, 32 * 8);
}

uint32_t ceil_log2(size_t x) { uint32_t k = 0; while (((size_t)1 << k) < x) k++; return k; }

template <class F>
hipError_t build_transpose(const cb::Csr* M3[3], uint32_t n_rows, uint32_t n_cols, SideDev& S, std::vector<void*>& owned) {
  std::vector<uint32_t> items;
  std::vector<std::vector<uint32_t>> cnts(3);
  for (int m = 0; m < 3; m++) {
    const cb::Csr& Mx = *M3[m];
    std::vector<uint32_t> ptr(n_cols + 1, 0), col(Mx.col.size()), coef(Mx.col.size());
    for (uint32_t c : Mx.col) ptr[c + 1]++;
    for (uint32_t c = 0; c < n_cols; c++) ptr[c + 1] += ptr[c];
    std::vector<uint32_t> cur(ptr.begin(), ptr.end() - 1);
    for (uint32_t r = 0; r < n_rows; r++)
      for (uint32_t k = Mx.row_ptr[r]; k < Mx.row_ptr[r + 1]; k++) { const uint32_t pos = cur[Mx.col[k]]++; col[pos] = r; coef[pos] = Mx.coef[k]; }
    for (uint32_t c = 0; c < n_cols; c++) if (ptr[c + 1] - ptr[c] > SPMV_LONG) items.push_back(((uint32_t)m << 30) | c);
    cnts[m].resize(n_cols);
    for (uint32_t c = 0; c < n_cols; c++) cnts[m][c] = ptr[c + 1] - ptr[c];
    CsrDev& D = m == 0 ? S.At : m == 1 ? S.Bt : S.Ct;
    hipError_t e;
    if ((e = upload(ptr, &D.row_ptr)) != hipSuccess) return e; owned.push_back((void*)D.row_ptr);
    if ((e = upload(col, &D.col)) != hipSuccess) return e; if (D.col) owned.push_back((void*)D.col);
    if ((e = upload(coef, &D.coef)) != hipSuccess) return e; if (D.coef) owned.push_back((void*)D.coef);
  }
  S.n_med_t = spmv_sort_items(items, [&](uint32_t it) { return cnts[it >> 30][it & 0x3fffffffu]; });
  S.n_long_t = (uint32_t)items.size();
  hipError_t e = upload(items, &S.items_t);
  if (S.items_t) owned.push_back((void*)S.items_t);
  return e;
}

template <class F>
void spmv_any(hipStream_t s, const CsrDev& A, const CsrDev& B, const CsrDev& C, const uint32_t* dict, const uint32_t* items, uint32_t n_long, uint32_t n_med,
              size_t nrows, const uint32_t* z, uint32_t* az, uint32_t* bz, uint32_t* cz) {
  hipLaunchKernelGGL(k_spmv3<F>, dim3(stream_grid(3 * nrows)), dim3(256), 0, s, A, B, C, dict, nrows, z, az, bz, cz);
  if (n_long) hipLaunchKernelGGL(k_spmv_long<F>, dim3(spmv_long_blocks(n_long, n_med)), dim3(256), 0, s, A, B, C, dict, items, n_long, n_med, z, az, bz, cz);
}

void cache_release(vimz_ctx* ctx, void** slot) {
  auto* c = (SpartanCache*)*slot;
  if (!c) return;
  if (ctx) {
    std::lock_guard<std::mutex> g(ctx->mu);
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    for (void* d : c->owned) hipFree(d);
    for (auto& s : c->side) if (s.pin) hipHostFree(s.pin);
    c->ws.release();
  }
  delete c;
  *slot = nullptr;
}
void spartan_release(vimz_ivc* v) { cache_release(v->ctx, &v->spartan_cache); }
void spartan_release_cf(vimz_cf* v) { cache_release(v->ctx, &v->spartan_cache); }

// an independent generator for the inner-product term (nobody knows its discrete log with respect to the key)
template <class C>
int derive_ipa_u(vimz_ctx* ctx, int curve, Affine<typename C::Base>* out) {
  vimz_bases* b = nullptr;
  int rc = vimz_bases_generate(ctx, curve, "vimz-ipa-u", 10, 1, &b);
  if (rc) return rc;
  uint64_t xy[8];
  rc = vimz_bases_download(ctx, b, 0, xy, 1, VIMZ_FORM_MONTGOMERY);
  vimz_bases_free(ctx, b);
  if (rc) return rc;
  memcpy(out->x.v, xy, 32); memcpy(out->y.v, xy + 4, 32);
  return VIMZ_OK;
}

// CompressedSNARK::setup: transposed shapes and scratch on the device (caller does NOT hold the lock).  Side 0: the prover's circuit over Fr with ck1,
// side 1: `sec` over Fq with ck2 (the Nova IVC's secondary circuit, or the CycleFold circuit of a vimz_cf).
int spartan_setup_sides(vimz_ctx* ctx, vimz_prover* p, const cb::Builder& b1, const SecDev& sec, const cb::BuilderT<Fq>& b2, const vimz_bases* ck1, const vimz_bases* ck2,
                        void** slot, SpartanCache** out) {
  if (*slot) { *out = (SpartanCache*)*slot; return VIMZ_OK; }
  std::unique_ptr<SpartanCache> c(new SpartanCache());
  int rc;
  if ((rc = derive_ipa_u<BnG1>(ctx, VIMZ_CURVE_BN254_G1, &c->ipa_u1))) return rc;
  if ((rc = derive_ipa_u<Grumpkin>(ctx, VIMZ_CURVE_GRUMPKIN, &c->ipa_u2))) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  struct FreeOnFail { SpartanCache* c; bool armed = true; ~FreeOnFail() { if (armed) { for (void* d : c->owned) hipFree(d); for (auto& s : c->side) if (s.pin) hipHostFree(s.pin); } } } guard{c.get()};
  for (int side = 0; side < 2; side++) {
    SideDev& S = c->side[side];
    if (side == 0) {
      S.A = p->A; S.B = p->B; S.C = p->C; S.dict = p->dict; S.n_w = p->n_wires; S.n_c = p->n_c;
      const cb::Csr* M3[3] = {&b1.A, &b1.B, &b1.C};
      P_TRY(build_transpose<Fe>(M3, S.n_c, S.n_w, S, c->owned));
    } else {
      S.A = sec.A; S.B = sec.B; S.C = sec.C; S.dict = sec.dict; S.items = sec.long_items; S.n_long = sec.n_long; S.n_med = sec.n_med;
      S.n_w = sec.n_w; S.n_c = sec.n_c;
      const cb::Csr* M3[3] = {&b2.A, &b2.B, &b2.C};
      P_TRY(build_transpose<Fq>(M3, S.n_c, S.n_w, S, c->owned));
    }
    S.s = ceil_log2(S.n_c); S.t = ceil_log2(S.n_w); S.M = (size_t)1 << S.s; S.N = (size_t)1 << S.t;
    const size_t big = std::max(S.M, S.N);
    if ((side == 0 ? ck1->n : ck2->n) < big) return vz_fail(ctx, VIMZ_ERR_INVALID, "compress: the commitment key is shorter than the padded shape (needs next_pow2(max(wires, constraints)) generators)");
    P_TRY(side_alloc(S, big, c->owned));
  }
  guard.armed = false;
  *out = c.get();
  *slot = c.release();
  return VIMZ_OK;
}
int spartan_setup(vimz_ivc* v, SpartanCache** out) {
  const int rc = spartan_setup_sides(v->ctx, v->pri, v->circ1->build->b, v->sec, v->c2.b, v->ck1, v->ck2, &v->spartan_cache, out);
  if (!rc && v->spartan_free != spartan_release) v->spartan_free = spartan_release;      // (written once: the batch's host threads pass here too)
  return rc;
}
int spartan_setup_cf(vimz_cf* v, SpartanCache** out) {
  const int rc = spartan_setup_sides(v->ctx, v->pri, v->circ->build->b, v->sec, v->cf.b, v->ck1, v->ck2, &v->spartan_cache, out);
  if (!rc && v->spartan_free != spartan_release_cf) v->spartan_free = spartan_release_cf;
  return rc;
}

template <class F>
F interp_cubic(const F& s0, const F& s1, const F& s2, const F& s3, const F& r) {     // Lagrange through t = 0, 1, 2, 3
  const F one = F::one(), two = F::dbl(one), three = F::add(two, one);
  const F inv2 = F::pow_pm2(two), inv6 = F::pow_pm2(F::mul(two, three));
  const F r1 = F::sub(r, one), r2 = F::sub(r, two), r3 = F::sub(r, three);
  const F l0 = F::neg(F::mul(F::mul(F::mul(r1, r2), r3), inv6));                  // (r−1)(r−2)(r−3)/(−6)
  const F l1 = F::mul(F::mul(F::mul(r, r2), r3), inv2);                           // r(r−2)(r−3)/2
  const F l2 = F::neg(F::mul(F::mul(F::mul(r, r1), r3), inv2));                   // r(r−1)(r−3)/(−2)
  const F l3 = F::mul(F::mul(F::mul(r, r1), r2), inv6);                           // r(r−1)(r−2)/6
  return F::add(F::add(F::mul(l0, s0), F::mul(l1, s1)), F::add(F::mul(l2, s2), F::mul(l3, s3)));
}
template <class F>
F interp_quad(const F& s0, const F& s1, const F& s2, const F& r) {                  // through t = 0, 1, 2
  const F one = F::one(), two = F::dbl(one), inv2 = F::pow_pm2(two);
  const F r1 = F::sub(r, one), r2 = F::sub(r, two);
  const F l0 = F::mul(F::mul(r1, r2), inv2), l1 = F::neg(F::mul(r, r2)), l2 = F::mul(F::mul(r, r1), inv2);
  return F::add(F::add(F::mul(l0, s0), F::mul(l1, s1)), F::mul(l2, s2));
}

// One relaxed instance of one side, as the prover and the verifier see it: n_pub >= 1 public elements X[0 .. n_pub) at the last n_pub wires of Z
// (wire 0 = u).  The augmented circuits of the IVC and F' have two, a CycleFold instance CF_IO = 7.
constexpr uint32_t MAX_PUB = 8;
template <class F, class FS>
struct Instance { Affine<FS> cW, cE; F u, X[MAX_PUB]; uint32_t n_pub = 2; bool has_E; };
template <class F, class FS>
Instance<F, FS> instance2(const Affine<FS>& cW, const Affine<FS>& cE, const F& u, const F& X0, const F& X1, bool has_E) {
  Instance<F, FS> I; I.cW = cW; I.cE = cE; I.u = u; I.X[0] = X0; I.X[1] = X1; I.n_pub = 2; I.has_E = has_E; return I;
}

template <class F, class FS>
void absorb_instance(Transcript& tr, const F& digest, const Instance<F, FS>& I, uint32_t side_tag) {
  const uint64_t tag = side_tag; tr.absorb_words("side", &tag, 1);
  tr.absorb_fe("digest", digest);
  tr.absorb_fe("cWx", I.cW.x); tr.absorb_fe("cWy", I.cW.y); tr.absorb_fe("cEx", I.cE.x); tr.absorb_fe("cEy", I.cE.y);
  tr.absorb_fe("u", I.u);
  for (uint32_t k = 0; k < I.n_pub; k++) { char tag[8]; snprintf(tag, sizeof(tag), "X%u", k); tr.absorb_fe(tag, I.X[k]); }      // ("X0", "X1" for the two of the IVC)
}

// ---- the bodies of the prover's loops (spartan_prove / ipa_prove and the test hooks of include/vimz_hip_testing.h run these very functions) --------
// tab[0 .. 2^k) = eq(pt, ·), pt[0] = the top bit of the index
template <class F>
hipError_t eq_build(hipStream_t s, uint32_t* tab, const std::vector<F>& pt) {
  const F one = F::one();
  hipError_t e;
  if ((e = hipMemcpyAsync(tab, one.v, 32, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
  const uint32_t k = (uint32_t)pt.size();
  for (uint32_t q = k; q-- > 0;) hipLaunchKernelGGL(k_eq_step<F>, dim3(stream_grid((size_t)1 << (k - 1 - q))), dim3(256), 0, s, tab, (size_t)1 << (k - 1 - q), pt[q]);
  return hipSuccess;
}

inline unsigned red_grid(size_t half) { return (unsigned)std::min<size_t>(RED_BLOCKS, (half + 255) / 256); }

// one outer round over eq, va, vb, vc (ve) of 2·half elements: the three evaluations, `next(s0, s2, s3)` -> the round's challenge r, then the bind at r
template <class F, class Next>
hipError_t outer_round(SideDev& S, hipStream_t s, size_t half, bool has_E, const F& u, Next next) {
  const unsigned gb = red_grid(half);
  hipLaunchKernelGGL(k_sc_outer<F>, dim3(gb), dim3(256), 0, s, (const uint32_t*)S.eq, (const uint32_t*)S.va, (const uint32_t*)S.vb, (const uint32_t*)S.vc,
                     has_E ? (const uint32_t*)S.ve : (const uint32_t*)nullptr, half, u, S.partial);
  hipLaunchKernelGGL((k_sum_partials<F, 3>), dim3(1), dim3(256), 0, s, (const uint32_t*)S.partial, gb, S.partial + 8 * 3 * RED_BLOCKS);
  hipError_t e;
  if ((e = hipMemcpyAsync(S.pin, S.partial + 8 * 3 * RED_BLOCKS, 96, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
  F s0, s2, s3; memcpy(s0.v, S.pin, 32); memcpy(s2.v, S.pin + 8, 32); memcpy(s3.v, S.pin + 16, 32);
  const F r = next(s0, s2, s3);
  BindSet bs{{S.eq, S.va, S.vb, S.vc, has_E ? S.ve : nullptr}, 5};
  hipLaunchKernelGGL(k_bind<F>, dim3(stream_grid(half)), dim3(256), 0, s, bs, half, r);
  return hipSuccess;
}

// one inner round over vm, vz: the two evaluations, `next(s0, s2)` -> r, then the bind
template <class F, class Next>
hipError_t inner_round(SideDev& S, hipStream_t s, size_t half, Next next) {
  const unsigned gb = red_grid(half);
  hipLaunchKernelGGL(k_sc_inner<F>, dim3(gb), dim3(256), 0, s, (const uint32_t*)S.vm, (const uint32_t*)S.vz, half, S.partial);
  hipLaunchKernelGGL((k_sum_partials<F, 2>), dim3(1), dim3(256), 0, s, (const uint32_t*)S.partial, gb, S.partial + 8 * 3 * RED_BLOCKS);
  hipError_t e;
  if ((e = hipMemcpyAsync(S.pin, S.partial + 8 * 3 * RED_BLOCKS, 64, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
  F s0, s2; memcpy(s0.v, S.pin, 32); memcpy(s2.v, S.pin + 8, 32);
  const F r = next(s0, s2);
  BindSet bs{{S.vm, S.vz, nullptr, nullptr, nullptr}, 2};
  hipLaunchKernelGGL(k_bind<F>, dim3(stream_grid(half)), dim3(256), 0, s, bs, half, r);
  return hipSuccess;
}

// the vector side of one IPA round over a, b of 2·half elements: (<a_L,b_R>, <a_R,b_L>) queued into the pinned buffer, then `next(pin, &x)` — which must
// synchronise the stream before it reads the two elements (the prover's MSMs do) — gives the challenge, then the fold of a and b
template <class F, class Next>
hipError_t ipa_vec_round(SideDev& S, hipStream_t s, uint32_t* a, uint32_t* b, size_t half, Next next) {
  const unsigned gb = red_grid(half);
  hipLaunchKernelGGL(k_dot2<F>, dim3(gb), dim3(256), 0, s, (const uint32_t*)a, (const uint32_t*)b, half, S.partial);
  hipLaunchKernelGGL((k_sum_partials<F, 2>), dim3(1), dim3(256), 0, s, (const uint32_t*)S.partial, gb, S.partial + 8 * 3 * RED_BLOCKS);
  hipError_t e;
  if ((e = hipMemcpyAsync(S.pin, S.partial + 8 * 3 * RED_BLOCKS, 64, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
  F x;
  if ((e = next((const uint32_t*)S.pin, &x)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_ipa_fold_vec<F>, dim3(stream_grid(half)), dim3(256), 0, s, a, b, half, x);
  return hipSuccess;
}

template <class G>
void ipa_fold_bases(hipStream_t s, uint32_t* bases, size_t half, const uint32_t xw[4]) {
  hipLaunchKernelGGL(k_ipa_fold_bases<G>, dim3(stream_grid(half)), dim3(256), 0, s, bases, half, make_uint4(xw[0], xw[1], xw[2], xw[3]));
}

// ---- prover ----------------------------------------------------------------------------------------------------------------------------
template <class F, class C>
int ipa_prove(vimz_ctx* ctx, SpartanCache& cache, SideDev& S, hipStream_t s, Transcript& tr, const Affine<typename C::Base>& Ugen, uint32_t* a, uint32_t* b,
              uint32_t rounds, const Affine<typename C::Base>& comm, const F& claim, Writer& out) {
  typedef typename C::Base FS;
  typedef typename C::Coord G;
  tr.absorb_fe("ipaP.x", comm.x); tr.absorb_fe("ipaP.y", comm.y); tr.absorb_fe("ipaC", claim);
  uint32_t r0[4]; tr.challenge(r0);
  const Affine<FS> Up = to_affine(host_mul<FS>(Ugen, r0, 128));
  size_t len = (size_t)1 << rounds;
  for (uint32_t j = 0; j < rounds; j++) {
    const size_t half = len >> 1;
    uint32_t xw[4];
    auto group_side = [&](const uint32_t* pin, F* x) -> hipError_t {
      hipError_t e;
      Affine<FS> Lg, Rg;
      if ((e = msm_run<C>(s, cache.ws, S.G + (size_t)AFFINE_WORDS * half, a, half, 1, 0, &Lg, nullptr, nullptr, 0, nullptr)) != hipSuccess) return e;          // <a_L, G_R>
      if ((e = msm_run<C>(s, cache.ws, S.G, a + 8 * half, half, 1, 0, &Rg, nullptr, nullptr, 0, nullptr)) != hipSuccess) return e;                             // <a_R, G_L>
      F cl, cr; memcpy(cl.v, pin, 32); memcpy(cr.v, pin + 8, 32);              // (the MSMs synchronised the stream)
      XYZZ<FS> L = from_affine(Lg); { XYZZ<FS> t = host_mul_fe<FS, F>(Up, cl); add_full(L, t); }
      XYZZ<FS> R = from_affine(Rg); { XYZZ<FS> t = host_mul_fe<FS, F>(Up, cr); add_full(R, t); }
      const Affine<FS> La = to_affine(L), Ra = to_affine(R);
      out.point(La); out.point(Ra);
      tr.absorb_fe("L.x", La.x); tr.absorb_fe("L.y", La.y); tr.absorb_fe("R.x", Ra.x); tr.absorb_fe("R.y", Ra.y);
      tr.challenge(xw);
      F xc = F::zero(); for (int k = 0; k < 4; k++) xc.v[k] = xw[k];
      *x = F::to_mont(xc);
      return hipSuccess;
    };
    P_TRY(ipa_vec_round<F>(S, s, a, b, half, group_side));
    ipa_fold_bases<G>(s, S.G, half, xw);
    P_TRY(hipGetLastError());
    len = half;
  }
  F afin;
  P_TRY(hipMemcpyAsync(S.pin, a, 32, hipMemcpyDeviceToHost, s));
  P_TRY(hipStreamSynchronize(s));
  memcpy(afin.v, S.pin, 32);
  out.fe(afin);
  tr.absorb_fe("a", afin);
  return VIMZ_OK;
}

// bases of the W opening: index i (wire i) -> ck[i-1], index 0 -> ck[N-1]; of the E opening: ck[0..M)
hipError_t load_bases(hipStream_t s, uint32_t* G, const vimz_bases* ck, size_t n, bool shifted) {
  if (!shifted) return hipMemcpyAsync(G, ck->d, 4 * (size_t)AFFINE_WORDS * n, hipMemcpyDeviceToDevice, s);
  hipError_t e = hipMemcpyAsync(G + AFFINE_WORDS, ck->d, 4 * (size_t)AFFINE_WORDS * (n - 1), hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return e;
  return hipMemcpyAsync(G, ck->d + (size_t)AFFINE_WORDS * (n - 1), 4 * (size_t)AFFINE_WORDS, hipMemcpyDeviceToDevice, s);
}

template <class F, class C, class Fwd>
int spartan_prove(vimz_ctx* ctx, SpartanCache& cache, SideDev& S, hipStream_t s, const vimz_bases* ck, const Affine<typename C::Base>& Ugen, const F& digest,
                  const Instance<F, typename C::Base>& I, const uint32_t* Z, const uint32_t* E, uint32_t side_tag, Transcript& tr, Writer& out, Fwd fwd,
                  bool forge_public_slot = false) {
  const size_t M = S.M, N = S.N, big = std::max(M, N);
  if (I.n_pub < 1 || I.n_pub > MAX_PUB || S.n_w < I.n_pub + 2) return vz_fail(ctx, VIMZ_ERR_INVALID, "spartan: an instance needs 1..8 public elements and at least one committed wire");
  absorb_instance(tr, digest, I, side_tag);
  // vectors: (A,B,C)·Z padded to M, E padded to M
  P_TRY(hipMemsetAsync(S.va, 0, 32 * big, s)); P_TRY(hipMemsetAsync(S.vb, 0, 32 * big, s)); P_TRY(hipMemsetAsync(S.vc, 0, 32 * big, s)); P_TRY(hipMemsetAsync(S.ve, 0, 32 * big, s));
  fwd(Z, S.va, S.vb, S.vc);
  if (E) P_TRY(hipMemcpyAsync(S.ve, E, 32 * (size_t)S.n_c, hipMemcpyDeviceToDevice, s));
  // eq(tau, ·)
  std::vector<F> tau(S.s);
  for (auto& x : tau) x = tr.challenge_fe<F>();
  P_TRY(eq_build<F>(s, S.eq, tau));
  // outer sum-check
  F claim = F::zero();
  std::vector<F> rx(S.s);
  size_t len = M;
  for (uint32_t j = 0; j < S.s; j++) {
    const size_t half = len >> 1;
    P_TRY(outer_round<F>(S, s, half, E != nullptr, I.u, [&](const F& s0, const F& s2, const F& s3) {
      out.fe(s0); out.fe(s2); out.fe(s3);
      tr.absorb_fe("o0", s0); tr.absorb_fe("o2", s2); tr.absorb_fe("o3", s3);
      const F r = tr.challenge_fe<F>();
      rx[j] = r;
      claim = interp_cubic(s0, F::sub(claim, s0), s2, s3, r);
      return r;
    }));
    len = half;
  }
  F cl[4];
  { uint32_t* src[4] = {S.va, S.vb, S.vc, S.ve};
    for (int k = 0; k < 4; k++) P_TRY(hipMemcpyAsync(S.pin + 8 * k, src[k], 32, hipMemcpyDeviceToHost, s));
    P_TRY(hipStreamSynchronize(s));
    for (int k = 0; k < 4; k++) memcpy(cl[k].v, S.pin + 8 * k, 32);
    if (!E) cl[3] = F::zero(); }
  for (int k = 0; k < 4; k++) { out.fe(cl[k]); tr.absorb_fe("claim", cl[k]); }
  const F rho = tr.challenge_fe<F>(), rho2 = F::sqr(rho);
  // eq(rx, ·) over the rows, then M = A^T e + rho B^T e + rho^2 C^T e over the columns
  P_TRY(eq_build<F>(s, S.eq, rx));
  spmv_any<F>(s, S.At, S.Bt, S.Ct, S.dict, S.items_t, S.n_long_t, S.n_med_t, S.n_w, S.eq, S.va, S.vb, S.vc);
  P_TRY(hipMemsetAsync(S.vm, 0, 32 * big, s)); P_TRY(hipMemsetAsync(S.vz, 0, 32 * big, s));
  hipLaunchKernelGGL(k_combine3<F>, dim3(stream_grid(S.n_w)), dim3(256), 0, s, (size_t)S.n_w, (const uint32_t*)S.va, (const uint32_t*)S.vb, (const uint32_t*)S.vc, rho, rho2, S.vm);
  P_TRY(hipMemcpyAsync(S.vz, Z, 32 * (size_t)S.n_w, hipMemcpyDeviceToDevice, s));
  claim = F::add(cl[0], F::add(F::mul(rho, cl[1]), F::mul(rho2, cl[2])));
  std::vector<F> ry(S.t);
  len = N;
  for (uint32_t j = 0; j < S.t; j++) {
    const size_t half = len >> 1;
    P_TRY(inner_round<F>(S, s, half, [&](const F& s0, const F& s2) {
      out.fe(s0); out.fe(s2);
      tr.absorb_fe("i0", s0); tr.absorb_fe("i2", s2);
      const F r = tr.challenge_fe<F>();
      ry[j] = r;
      claim = interp_quad(s0, F::sub(claim, s0), s2, r);
      return r;
    }));
    len = half;
  }
  // Z(ry) is what the bound vector holds; the committed part's evaluation is Z(ry) minus the public entries' share
  F zr;
  P_TRY(hipMemcpyAsync(S.pin, S.vz, 32, hipMemcpyDeviceToHost, s));
  P_TRY(hipStreamSynchronize(s));
  memcpy(zr.v, S.pin, 32);
  auto eq_at = [&](const std::vector<F>& pt, size_t idx) {          // eq(pt, idx), pt[0] = the top bit
    F acc = F::one();
    const size_t k = pt.size();
    for (size_t q = 0; q < k; q++) { const bool bit = (idx >> (k - 1 - q)) & 1; acc = F::mul(acc, bit ? pt[q] : F::sub(F::one(), pt[q])); }
    return acc;
  };
  F pub = F::mul(I.u, eq_at(ry, 0));
  for (uint32_t k = 0; k < I.n_pub; k++) pub = F::add(pub, F::mul(I.X[k], eq_at(ry, S.n_w - I.n_pub + k)));
  const F evalW = F::sub(zr, pub);
  out.fe(evalW);
  tr.absorb_fe("evalW", evalW);
  // opening of the committed part of Z at ry:  a = W' (into va), b = eq(ry, ·) (into vb), bases shifted by one wire
  int rc;
  hipLaunchKernelGGL(k_committed_part<F>, dim3(stream_grid(N)), dim3(256), 0, s, Z, (size_t)S.n_w, (size_t)I.n_pub, N, S.va);
  P_TRY(eq_build<F>(s, S.vb, ry));
  hipLaunchKernelGGL(k_mask_public<F>, dim3(stream_grid(N)), dim3(256), 0, s, S.vb, (size_t)S.n_w, (size_t)I.n_pub, N);
  if (forge_public_slot) {      // test hook (vimz_ivc_compress): the opened vector carries X0 − X0' = −1 in the slot of wire n−2
    const F m1 = F::neg(F::one());
    P_TRY(hipMemcpyAsync(S.va + 8 * (size_t)(S.n_w - 2), m1.v, 32, hipMemcpyHostToDevice, s)); P_TRY(hipStreamSynchronize(s));
  }
  P_TRY(load_bases(s, S.G, ck, N, true));
  if ((rc = ipa_prove<F, C>(ctx, cache, S, s, tr, Ugen, S.va, S.vb, S.t, I.cW, evalW, out))) return rc;
  // opening of E at rx
  if (E) {
    P_TRY(hipMemsetAsync(S.va, 0, 32 * M, s));
    P_TRY(hipMemcpyAsync(S.va, E, 32 * (size_t)S.n_c, hipMemcpyDeviceToDevice, s));
    P_TRY(eq_build<F>(s, S.vb, rx));
    P_TRY(load_bases(s, S.G, ck, M, false));
    if ((rc = ipa_prove<F, C>(ctx, cache, S, s, tr, Ugen, S.va, S.vb, S.s, I.cE, cl[3], out))) return rc;
  }
  P_TRY(hipGetLastError());
  return VIMZ_OK;
}

// ---- verifier (host arithmetic; one MSM per opening on the GPU) ----------------------------------------------------------------------------
template <class F>
std::vector<F> eq_table(const std::vector<F>& pt) {       // eq(pt, ·), pt[0] = the top bit of the index
  const size_t k = pt.size();
  std::vector<F> tab((size_t)1 << k);
  tab[0] = F::one();
  size_t len = 1;
  for (size_t q = k; q-- > 0;) { for (size_t i = 0; i < len; i++) { const F hi = F::mul(tab[i], pt[q]); tab[i + len] = hi; tab[i] = F::sub(tab[i], hi); } len <<= 1; }
  return tab;
}

template <class F, class C>
bool ipa_verify(vimz_ctx* ctx, SpartanCache& cache, SideDev& S, hipStream_t s, Transcript& tr, const Affine<typename C::Base>& Ugen, const vimz_bases* ck, bool shifted,
                const std::vector<F>& b, uint32_t rounds, const Affine<typename C::Base>& comm, const F& claim, Reader& in) {
  typedef typename C::Base FS;
  tr.absorb_fe("ipaP.x", comm.x); tr.absorb_fe("ipaP.y", comm.y); tr.absorb_fe("ipaC", claim);
  uint32_t r0[4]; tr.challenge(r0);
  const Affine<FS> Up = to_affine(host_mul<FS>(Ugen, r0, 128));
  XYZZ<FS> P = from_affine(comm); { XYZZ<FS> t = host_mul_fe<FS, F>(Up, claim); add_full(P, t); }
  std::vector<F> xs(rounds);
  for (uint32_t j = 0; j < rounds; j++) {
    const Affine<FS> L = in.point<FS>(), R = in.point<FS>();
    if (!in.ok) return false;
    tr.absorb_fe("L.x", L.x); tr.absorb_fe("L.y", L.y); tr.absorb_fe("R.x", R.x); tr.absorb_fe("R.y", R.y);
    uint32_t xw[4]; tr.challenge(xw);
    F xc = F::zero(); for (int k = 0; k < 4; k++) xc.v[k] = xw[k];
    xs[j] = F::to_mont(xc);
    // P <- R + x·P + x²·L
    const Affine<FS> Pa = to_affine(P);
    XYZZ<FS> acc = from_affine(R);
    { XYZZ<FS> t = host_mul<FS>(Pa, xw, 128); add_full(acc, t); }
    { XYZZ<FS> t = host_mul_fe<FS, F>(L, F::sqr(xs[j])); add_full(acc, t); }
    P = acc;
  }
  const F afin = in.fe<F>();
  if (!in.ok) return false;
  tr.absorb_fe("a", afin);
  // s_i = product of the challenges of the rounds in which index i sat in the right half (round 0 = top bit)
  const size_t n = (size_t)1 << rounds;
  std::vector<F> sv(n);
  sv[0] = F::one();
  size_t len = 1;
  for (uint32_t q = rounds; q-- > 0;) { for (size_t i = 0; i < len; i++) sv[i + len] = F::mul(sv[i], xs[q]); len <<= 1; }
  F bfin = F::zero();
  for (size_t i = 0; i < n; i++) bfin = F::add(bfin, F::mul(sv[i], b[i]));
  Affine<FS> Gfin;
  if (hipMemcpyAsync(S.va, sv.data(), 32 * n, hipMemcpyHostToDevice, s) != hipSuccess) return false;
  if (load_bases(s, S.G, ck, n, shifted) != hipSuccess) return false;
  if (msm_run<C>(s, cache.ws, S.G, S.va, n, 1, 0, &Gfin, nullptr, nullptr, 0, nullptr) != hipSuccess) return false;
  XYZZ<FS> rhs = host_mul_fe<FS, F>(Gfin, afin);
  { XYZZ<FS> t = host_mul_fe<FS, F>(Up, F::mul(afin, bfin)); add_full(rhs, t); }
  const Affine<FS> lhs_a = to_affine(P), rhs_a = to_affine(rhs);
  return lhs_a.x.eq(rhs_a.x) && lhs_a.y.eq(rhs_a.y);
}

template <class F, class C, class B>
bool spartan_verify(vimz_ctx* ctx, SpartanCache& cache, SideDev& S, hipStream_t s, const vimz_bases* ck, const Affine<typename C::Base>& Ugen, const F& digest,
                    const Instance<F, typename C::Base>& I, const B& shape /* host builder: A, B, C as CSR + dict */, uint32_t side_tag, Transcript& tr, Reader& in) {
  if (I.n_pub < 1 || I.n_pub > MAX_PUB || S.n_w < I.n_pub + 2) return false;
  absorb_instance(tr, digest, I, side_tag);
  std::vector<F> tau(S.s);
  for (auto& x : tau) x = tr.challenge_fe<F>();
  F claim = F::zero();
  std::vector<F> rx(S.s);
  for (uint32_t j = 0; j < S.s; j++) {
    const F s0 = in.fe<F>(), s2 = in.fe<F>(), s3 = in.fe<F>();
    if (!in.ok) return false;
    tr.absorb_fe("o0", s0); tr.absorb_fe("o2", s2); tr.absorb_fe("o3", s3);
    rx[j] = tr.challenge_fe<F>();
    claim = interp_cubic(s0, F::sub(claim, s0), s2, s3, rx[j]);
  }
  F cl[4];
  for (int k = 0; k < 4; k++) cl[k] = in.fe<F>();
  if (!in.ok) return false;
  if (!I.has_E && !cl[3].is_zero()) return false;
  {
    F e = F::one();
    for (uint32_t k = 0; k < S.s; k++) e = F::mul(e, F::add(F::mul(tau[k], rx[k]), F::mul(F::sub(F::one(), tau[k]), F::sub(F::one(), rx[k]))));
    const F want = F::mul(e, F::sub(F::sub(F::mul(cl[0], cl[1]), F::mul(I.u, cl[2])), cl[3]));
    if (!want.eq(claim)) return false;
  }
  for (int k = 0; k < 4; k++) tr.absorb_fe("claim", cl[k]);
  const F rho = tr.challenge_fe<F>(), rho2 = F::sqr(rho);
  claim = F::add(cl[0], F::add(F::mul(rho, cl[1]), F::mul(rho2, cl[2])));
  std::vector<F> ry(S.t);
  for (uint32_t j = 0; j < S.t; j++) {
    const F s0 = in.fe<F>(), s2 = in.fe<F>();
    if (!in.ok) return false;
    tr.absorb_fe("i0", s0); tr.absorb_fe("i2", s2);
    ry[j] = tr.challenge_fe<F>();
    claim = interp_quad(s0, F::sub(claim, s0), s2, ry[j]);
  }
  const F evalW = in.fe<F>();
  if (!in.ok) return false;
  tr.absorb_fe("evalW", evalW);
  const std::vector<F> ex = eq_table(rx), ey = eq_table(ry);
  // M(ry) = sum over the non-zeros of (A + rho B + rho^2 C) of eq(rx, row) · eq(ry, col) · value
  F vm = F::zero();
  {
    const cb::Csr* Ms[3] = {&shape.A, &shape.B, &shape.C};
    const F w[3] = {F::one(), rho, rho2};
    for (int m = 0; m < 3; m++) {
      F acc = F::zero();
      for (uint32_t r = 0; r + 1 < Ms[m]->row_ptr.size(); r++) {
        F row = F::zero();
        for (uint32_t k = Ms[m]->row_ptr[r]; k < Ms[m]->row_ptr[r + 1]; k++) row = F::add(row, F::mul(shape.dict[Ms[m]->coef[k]], ey[Ms[m]->col[k]]));
        acc = F::add(acc, F::mul(row, ex[r]));
      }
      vm = F::add(vm, F::mul(w[m], acc));
    }
  }
  F vz = F::add(evalW, F::mul(I.u, ey[0]));
  for (uint32_t k = 0; k < I.n_pub; k++) vz = F::add(vz, F::mul(I.X[k], ey[S.n_w - I.n_pub + k]));
  if (!F::mul(vm, vz).eq(claim)) return false;
  {   // the W opening is over the committed positions only: b = eq(ry, ·) with the public slots and the padding zeroed (k_mask_public)
    std::vector<F> eyW(ey);
    for (size_t i = 0; i < eyW.size(); i++) if (i == 0 || i + I.n_pub >= S.n_w) eyW[i] = F::zero();
    if (!ipa_verify<F, C>(ctx, cache, S, s, tr, Ugen, ck, true, eyW, S.t, I.cW, evalW, in)) return false;
  }
  if (I.has_E && !ipa_verify<F, C>(ctx, cache, S, s, tr, Ugen, ck, false, ex, S.s, I.cE, cl[3], in)) return false;
  return true;
}

// How the four verifier entries below judge an argument: SingleVerify is spartan_verify under the context's lock; DeferredVerify (spartan_batch.hpp) replays it on
// the host and leaves the device and group work to the batch.  Every other line of an entry's body is the same code for both.
struct SingleVerify {
  typedef std::lock_guard<std::mutex> Lock;
  static constexpr bool on_device = true;
  template <class F, class C, class B>
  bool arg(vimz_ctx* ctx, SpartanCache& cache, SideDev& S, hipStream_t s, const vimz_bases* ck, const Affine<typename C::Base>& Ugen, const F& digest,
           const Instance<F, typename C::Base>& I, const B& shape, uint32_t side_tag, Transcript& tr, Reader& in) {
    return spartan_verify<F, C>(ctx, cache, S, s, ck, Ugen, digest, I, shape, side_tag, tr, in);
  }
};

const uint64_t CSNARK_MAGIC = 0x314e5343565aull;   // "ZVCSN1"

struct Loaded {          // the instances a compressed proof is about, as both provers and verifiers hold them
  RelaxedInst<Fq> U1; RelaxedInst<Fe> U2; FreshInst<Fe> u2;
  Fe u1_run; Fq u2_run;
};

void bind_statement(Transcript& tr, uint64_t steps, const std::vector<Fe>& z0, const std::vector<Fe>& zn) {
  tr.absorb_words("steps", &steps, 1);
  for (auto& z : z0) tr.absorb_fe("z0", z);
  for (auto& z : zn) tr.absorb_fe("zn", z);
}

template <class F> F u256_to_fe(const U256w& x) { return from_u256<F>(x); }

Instance<Fe, Fq> inst_primary(const Loaded& L) { return instance2<Fe, Fq>(L.U1.W, L.U1.E, L.u1_run, u256_to_fe<Fe>(L.U1.X0), u256_to_fe<Fe>(L.U1.X1), true); }
Instance<Fq, Fe> inst_secondary(const Loaded& L) { return instance2<Fq, Fe>(L.U2.W, L.U2.E, L.u2_run, u256_to_fe<Fq>(L.U2.X0), u256_to_fe<Fq>(L.U2.X1), true); }
Instance<Fq, Fe> inst_fresh(const Loaded& L) {
  G2Aff none; none.x = none.y = Fe::zero();
  return instance2<Fq, Fe>(L.u2.W, none, Fq::one(), cross_field<Fq>(L.u2.x0), cross_field<Fq>(L.u2.x1), false);
}

}  // namespace

extern "C" {

// words of a compressed proof for this IVC's shapes
size_t vimz_ivc_compressed_size(vimz_ivc* v) {
  if (!v) return 0;
  const uint32_t s1 = ceil_log2(v->pri->n_c), t1 = ceil_log2(v->pri->n_wires), s2 = ceil_log2(v->sec.n_c), t2 = ceil_log2(v->sec.n_w);
  auto words = [](size_t s, size_t t, bool e) { return 4 * (3 * s + 4 + 2 * t + 1) + 4 * (4 * t + 1) + (e ? 4 * (4 * s + 1) : 0); };
  return 8 * (8 + 4 * 2 * (size_t)v->pri->len_z + 4 * (7 + 7 + 4) + words(s1, t1, true) + words(s2, t2, true) + words(s2, t2, false));
}

// CompressedSNARK::prove (mod.rs:56-59): blob receives vimz_ivc_compressed_size(v) bytes.  seconds (optional): {setup, prove}.
#ifdef VIMZ_TESTING
static std::atomic<bool> g_forge_public_slot{false};
void vimz_test_forge_public_slot(int on) { g_forge_public_slot.store(on != 0); }
#endif
int vimz_ivc_compress(vimz_ivc* v, uint8_t* blob, size_t cap, double seconds[2]) {
  if (!v || !blob) return VIMZ_ERR_INVALID;
  vimz_ctx* ctx = v->ctx;
  if (cap < vimz_ivc_compressed_size(v)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_ivc_compress: buffer too small");
  if (v->i == 0) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_ivc_compress: nothing has been folded");
  double t0 = now_s();
  SpartanCache* cache = nullptr;
  int rc = spartan_setup(v, &cache);
  if (rc) return rc;
  const double t_setup = now_s() - t0;
  t0 = now_s();
  // Test hook for the negative test of the public-slot binding (tests/test_gpu_compress.py): a cheating prover that claims x0 + 1 for
  // the last fresh instance and hides the difference in the generator of that wire's slot.  Exists only in libvimz_hip_testing.so
  // (vimz_test_forge_public_slot, include/vimz_hip_testing.h); the product library has no such prover.
#ifdef VIMZ_TESTING
  const bool forge = g_forge_public_slot.load();
#else
  const bool forge = false;
#endif
  G2Aff forge_gen; forge_gen.x = forge_gen.y = Fe::zero();
  if (forge) {
    uint64_t xy[8];
    if ((rc = vimz_bases_download(ctx, v->ck2, v->sec.n_w - 3, xy, 1, VIMZ_FORM_MONTGOMERY))) return rc;
    memcpy(forge_gen.x.v, xy, 32); memcpy(forge_gen.y.v, xy + 4, 32);
  }
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  P_TRY(hipStreamSynchronize(s));
  vimz_prover* p = v->pri;
  Loaded L; L.U1 = v->U1; L.U2 = v->U2; L.u2 = v->u2; L.u1_run = v->u1_run; L.u2_run = v->u2_run;
  if (forge) {      // comm' = comm − ck[n−3] commits to the same W with −1 in the slot of wire n−2;  x0' = x0 + 1
    G2 a = from_affine(L.u2.W); G2Aff neg = forge_gen; neg.y = Fe::neg(neg.y); add_mixed(a, neg); L.u2.W = to_affine(a);
    L.u2.x0 = Fe::add(L.u2.x0, Fe::one());
  }
  Writer out;
  out.word(CSNARK_MAGIC); out.word(v->i); out.word(p->len_z); out.word(cache->side[0].s); out.word(cache->side[0].t); out.word(cache->side[1].s); out.word(cache->side[1].t); out.word(0);
  for (auto& z : v->z0) out.fe(z);
  for (auto& z : p->z_cur) out.fe(z);
  out.point(L.U1.W); out.point(L.U1.E); out.fe(L.U1.u); out.u256(L.U1.X0); out.u256(L.U1.X1);
  out.point(L.U2.W); out.point(L.U2.E); out.fe(L.U2.u); out.u256(L.U2.X0); out.u256(L.U2.X1);
  out.point(L.u2.W); out.fe(L.u2.x0); out.fe(L.u2.x1);
  Transcript tr("vimz-compressed-snark-v1");
  bind_statement(tr, v->i, v->z0, p->z_cur);
  tr.absorb_words("inst", out.w.data() + 8 + 8 * p->len_z, 4 * (7 + 7 + 4));
  auto fwd1 = [&](const uint32_t* z, uint32_t* az, uint32_t* bz, uint32_t* cz) { launch_spmv(p, s, z, az, bz, cz, 0); };
  auto fwd2 = [&](const uint32_t* z, uint32_t* az, uint32_t* bz, uint32_t* cz) { sec_spmv<Fq>(v->sec, s, z, az, bz, cz); };
  if ((rc = spartan_prove<Fe, BnG1>(ctx, *cache, cache->side[0], s, v->ck1, cache->ipa_u1, v->c1->digest, inst_primary(L), p->Zrun, p->E, 1, tr, out, fwd1))) return rc;
  if ((rc = spartan_prove<Fq, Grumpkin>(ctx, *cache, cache->side[1], s, v->ck2, cache->ipa_u2, v->c2.digest, inst_secondary(L), v->sec.Zrun, v->sec.E, 2, tr, out, fwd2))) return rc;
  if ((rc = spartan_prove<Fq, Grumpkin>(ctx, *cache, cache->side[1], s, v->ck2, cache->ipa_u2, v->c2.digest, inst_fresh(L), v->sec.z2, nullptr, 3, tr, out, fwd2, forge))) return rc;
  if (8 * out.w.size() != vimz_ivc_compressed_size(v)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_ivc_compress: internal size mismatch");
  memcpy(blob, out.w.data(), 8 * out.w.size());
  if (seconds) { seconds[0] = t_setup; seconds[1] = now_s() - t0; }
  return VIMZ_OK;
}

// CompressedSNARK::verify(vk, num_steps, z0_primary, z0_secondary) (mod.rs:63-67).  `v` supplies the verifier key: an IVC object
// created for the same step circuit and commitment keys (its folding state is neither read nor changed).
// result: 0 = accepted; bit 0 / 1 the primary / secondary chain hash; bit 2 / 3 / 4 the argument for the primary running /
// secondary running / last fresh secondary instance; bit 12 the statement (steps, z0) differs; bit 13 malformed proof.
}  // extern "C"
namespace {
template <class V>
int ivc_verify_compressed_impl(V& vf, vimz_ivc* v, const uint8_t* blob, size_t len, uint64_t num_steps, const uint64_t* z0, uint32_t* result) {
  if (!v || !blob || !z0 || !result) return VIMZ_ERR_INVALID;
  vimz_ctx* ctx = v->ctx;
  SpartanCache* cache = nullptr;
  int rc = spartan_setup(v, &cache);
  if (rc) return rc;
  if (len != vimz_ivc_compressed_size(v) || (len & 7)) { *result = 8192; return VIMZ_OK; }
  std::vector<uint64_t> words(len / 8); memcpy(words.data(), blob, len);
  Reader in{words.data(), words.size()};
  vimz_prover* p = v->pri;
  uint32_t res = 0;
  const uint64_t magic = in.word(), steps = in.word(), lz = in.word(), s1 = in.word(), t1 = in.word(), s2 = in.word(), t2 = in.word(); in.word();
  if (magic != CSNARK_MAGIC || lz != p->len_z || s1 != cache->side[0].s || t1 != cache->side[0].t || s2 != cache->side[1].s || t2 != cache->side[1].t) { *result = 8192; return VIMZ_OK; }
  std::vector<Fe> z0p(lz), zn(lz), z0c(lz);
  for (auto& z : z0p) z = in.fe<Fe>();
  for (auto& z : zn) z = in.fe<Fe>();
  for (uint32_t k = 0; k < lz; k++) { Fe c; memcpy(c.v, z0 + 4 * k, 32); if (!c.is_reduced()) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_ivc_verify_compressed: z0 element not below the modulus"); z0c[k] = Fe::to_mont(c); }
  if (steps != num_steps || steps == 0) res |= 4096;
  for (uint32_t k = 0; k < lz; k++) if (!z0c[k].eq(z0p[k])) res |= 4096;
  Loaded L;
  L.U1.W = in.point<Fq>(); L.U1.E = in.point<Fq>(); L.U1.u = in.fe<Fq>(); L.U1.X0 = in.u256(); L.U1.X1 = in.u256();
  L.U2.W = in.point<Fe>(); L.U2.E = in.point<Fe>(); L.U2.u = in.fe<Fe>(); L.U2.X0 = in.u256(); L.U2.X1 = in.u256();
  L.u2.W = in.point<Fe>(); L.u2.x0 = in.fe<Fe>(); L.u2.x1 = in.fe<Fe>();
  if (!in.ok) { *result = 8192; return VIMZ_OK; }
  L.u1_run = cross_field<Fe>(L.U1.u); L.u2_run = cross_field<Fq>(L.U2.u);      // u is a small integer: the same in both fields
  // the two chain hashes, recomputed from the verifier's own digests and the CLAIMED z0
  {
    Fe h1 = instance_hash_native<BnFr>(v->c1->digest, steps, z0c, zn, L.U2);
    if (!h1.eq(L.u2.x0)) res |= 1;
    std::vector<Fq> zq = {Fq::zero()};
    Fq h2 = instance_hash_native<BnFq>(v->c2.digest, steps, zq, zq, L.U1);
    if (!cross_field<Fe>(h2).eq(L.u2.x1)) res |= 2;
  }
  typename V::Lock g(ctx->mu);
  if (V::on_device) P_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  Transcript tr("vimz-compressed-snark-v1");
  bind_statement(tr, steps, z0p, zn);
  tr.absorb_words("inst", words.data() + 8 + 8 * lz, 4 * (7 + 7 + 4));
  const cb::Builder& b1 = v->circ1->build->b; const cb::BuilderT<Fq>& b2 = v->c2.b;
  bool ok1 = false, ok2 = false, ok3 = false;
  try {
    ok1 = vf.template arg<Fe, BnG1>(ctx, *cache, cache->side[0], s, v->ck1, cache->ipa_u1, v->c1->digest, inst_primary(L), b1, 1, tr, in);
    ok2 = ok1 && vf.template arg<Fq, Grumpkin>(ctx, *cache, cache->side[1], s, v->ck2, cache->ipa_u2, v->c2.digest, inst_secondary(L), b2, 2, tr, in);
    ok3 = ok2 && vf.template arg<Fq, Grumpkin>(ctx, *cache, cache->side[1], s, v->ck2, cache->ipa_u2, v->c2.digest, inst_fresh(L), b2, 3, tr, in);
  } catch (const std::exception& e) { return vz_fail(ctx, VIMZ_ERR_INVALID, e.what()); }
  if (!ok1) res |= 4;
  if (ok1 && !ok2) res |= 8;
  if (ok1 && ok2 && !ok3) res |= 16;
  if (!in.ok || (ok3 && in.pos != in.n)) res |= 8192;
  *result = res;
  return VIMZ_OK;
}
}  // namespace
extern "C" {
int vimz_ivc_verify_compressed(vimz_ivc* v, const uint8_t* blob, size_t len, uint64_t num_steps, const uint64_t* z0, uint32_t* result) {
  SingleVerify vf;
  return ivc_verify_compressed_impl(vf, v, blob, len, num_steps, z0, result);
}

// ---- CompressedSNARK for a merged proof (merge.hip): one argument for the folded primary instance, one for the folded secondary one.
// Blob: {magic, words of the records} ‖ records (segments' statements and instances, the fold tree's cross-term commitments) ‖ the two
// arguments.  The verifier replays the records (every segment's hash checks, adjacency, the folds) and verifies the arguments for the
// instances IT computed.
static const uint64_t CMERGED_MAGIC = 0x31474d43565aull;   // "ZVCMG1"

static size_t arg_words(size_t s, size_t t, bool e) { return 4 * (3 * s + 4 + 2 * t + 1) + 4 * (4 * t + 1) + (e ? 4 * (4 * s + 1) : 0); }

size_t vimz_ivc_merged_compressed_size(const vimz_ivc_merged* m) {
  if (!m || !m->vk) return 0;
  const vimz_ivc* v = m->vk;
  const uint32_t s1 = ceil_log2(v->pri->n_c), t1 = ceil_log2(v->pri->n_wires), s2 = ceil_log2(v->sec.n_c), t2 = ceil_log2(v->sec.n_w);
  return 8 * (2 + records_words(m) + arg_words(s1, t1, true) + arg_words(s2, t2, true));
}

int vimz_ivc_merged_compress(vimz_ivc_merged* m, uint8_t* blob, size_t cap, double seconds[2]) {
  if (!m || !blob || !m->vk || m->broken) return VIMZ_ERR_INVALID;
  vimz_ivc* v = m->vk; vimz_ctx* ctx = v->ctx;
  if (cap < vimz_ivc_merged_compressed_size(m)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_ivc_merged_compress: buffer too small");
  double t0 = now_s();
  SpartanCache* cache = nullptr;
  int rc = spartan_setup(v, &cache);
  if (rc) return rc;
  const double t_setup = now_s() - t0;
  t0 = now_s();
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  P_TRY(hipStreamSynchronize(s));
  vimz_prover* p = v->pri;
  Writer out;
  out.word(CMERGED_MAGIC); out.word(records_words(m));
  write_records(m, out);
  Transcript tr("vimz-merged-compressed-v1");
  tr.absorb_words("records", out.w.data() + 2, out.w.size() - 2);
  const Instance<Fe, Fq> I1 = instance2<Fe, Fq>(m->acc.P.cW, m->acc.P.cE, m->acc.P.u, m->acc.P.X0, m->acc.P.X1, true);
  const Instance<Fq, Fe> I2 = instance2<Fq, Fe>(m->acc.Q.cW, m->acc.Q.cE, m->acc.Q.u, m->acc.Q.X0, m->acc.Q.X1, true);
  auto fwd1 = [&](const uint32_t* z, uint32_t* az, uint32_t* bz, uint32_t* cz) { launch_spmv(p, s, z, az, bz, cz, 0); };
  auto fwd2 = [&](const uint32_t* z, uint32_t* az, uint32_t* bz, uint32_t* cz) { sec_spmv<Fq>(v->sec, s, z, az, bz, cz); };
  if ((rc = spartan_prove<Fe, BnG1>(ctx, *cache, cache->side[0], s, v->ck1, cache->ipa_u1, v->c1->digest, I1, m->Zp, m->Ep, 1, tr, out, fwd1))) return rc;
  if ((rc = spartan_prove<Fq, Grumpkin>(ctx, *cache, cache->side[1], s, v->ck2, cache->ipa_u2, v->c2.digest, I2, m->Zq, m->Eq, 2, tr, out, fwd2))) return rc;
  if (8 * out.w.size() != vimz_ivc_merged_compressed_size(m)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_ivc_merged_compress: internal size mismatch");
  memcpy(blob, out.w.data(), 8 * out.w.size());
  if (seconds) { seconds[0] = t_setup; seconds[1] = now_s() - t0; }
  return VIMZ_OK;
}

// verify(vk, num_steps, z0) of a compressed merged proof.  result: 0 = accepted; bit 0 / 1 a segment's primary / secondary chain hash;
// bit 2 / 3 the argument for the folded primary / secondary instance; bit 12 statement (steps, z0, adjacency); bit 13 malformed.
}  // extern "C"
namespace {
template <class V>
int ivc_verify_merged_compressed_impl(V& vf, vimz_ivc* v, const uint8_t* blob, size_t len, uint64_t num_steps, const uint64_t* z0, uint32_t* result) {
  if (!v || !blob || !z0 || !result) return VIMZ_ERR_INVALID;
  vimz_ctx* ctx = v->ctx;
  SpartanCache* cache = nullptr;
  int rc = spartan_setup(v, &cache);
  if (rc) return rc;
  if ((len & 7) || len < 16) { *result = 8192; return VIMZ_OK; }
  std::vector<uint64_t> words(len / 8); memcpy(words.data(), blob, len);
  Reader in{words.data(), words.size()};
  const uint64_t magic = in.word(), rw = in.word();
  if (magic != CMERGED_MAGIC || rw > words.size() - 2) { *result = 8192; return VIMZ_OK; }
  std::vector<MSeg> segs; std::vector<MOp> ops;
  if (!read_records(in, v, segs, ops) || in.pos != 2 + rw) { *result = 8192; return VIMZ_OK; }
  const uint32_t s1 = cache->side[0].s, t1 = cache->side[0].t, s2 = cache->side[1].s, t2 = cache->side[1].t;
  if (words.size() != 2 + rw + arg_words(s1, t1, true) + arg_words(s2, t2, true)) { *result = 8192; return VIMZ_OK; }
  uint32_t res = 0;
  MAcc R;
  if (!merged_replay(v, segs, ops, &R, &res)) { *result = res | 8192; return VIMZ_OK; }
  vimz_prover* p = v->pri;
  if (R.n != num_steps) res |= 4096;
  for (uint32_t k = 0; k < p->len_z; k++) {
    Fe c; memcpy(c.v, z0 + 4 * k, 32);
    if (!c.is_reduced()) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_ivc_verify_merged_compressed: z0 element not below the modulus");
    if (!Fe::to_mont(c).eq(R.zs[k])) res |= 4096;
  }
  typename V::Lock g(ctx->mu);
  if (V::on_device) P_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  Transcript tr("vimz-merged-compressed-v1");
  tr.absorb_words("records", words.data() + 2, rw);
  const Instance<Fe, Fq> I1 = instance2<Fe, Fq>(R.P.cW, R.P.cE, R.P.u, R.P.X0, R.P.X1, true);
  const Instance<Fq, Fe> I2 = instance2<Fq, Fe>(R.Q.cW, R.Q.cE, R.Q.u, R.Q.X0, R.Q.X1, true);
  const cb::Builder& b1 = v->circ1->build->b; const cb::BuilderT<Fq>& b2 = v->c2.b;
  bool ok1 = false, ok2 = false;
  try {
    ok1 = vf.template arg<Fe, BnG1>(ctx, *cache, cache->side[0], s, v->ck1, cache->ipa_u1, v->c1->digest, I1, b1, 1, tr, in);
    ok2 = ok1 && vf.template arg<Fq, Grumpkin>(ctx, *cache, cache->side[1], s, v->ck2, cache->ipa_u2, v->c2.digest, I2, b2, 2, tr, in);
  } catch (const std::exception& e) { return vz_fail(ctx, VIMZ_ERR_INVALID, e.what()); }
  if (!ok1) res |= 4;
  if (ok1 && !ok2) res |= 8;
  if (!in.ok || (ok2 && in.pos != in.n)) res |= 8192;
  *result = res;
  return VIMZ_OK;
}
}  // namespace
extern "C" {
int vimz_ivc_verify_merged_compressed(vimz_ivc* v, const uint8_t* blob, size_t len, uint64_t num_steps, const uint64_t* z0, uint32_t* result) {
  SingleVerify vf;
  return ivc_verify_merged_compressed_impl(vf, v, blob, len, num_steps, z0, result);
}


// ---- CompressedSNARK for the Nova + CycleFold proofs (cyclefold.hip, cyclefold_merge.hip) ---------------------------------------------------------
// One chain: the statement of vimz_cf_verify with every "this witness satisfies this instance" replaced by an argument — U_n (relaxed, over F' on
// BN254 G1), u_n (the last instance of F': strict, no E) and cfU_n (relaxed, CF_IO public elements, over the CycleFold circuit on Grumpkin).
// Merged: the records and one argument for each of the two folded instances.  Framing of both blobs: cf_compressed_parse.hpp.
}  // extern "C"
namespace {
cfz::Shapes cf_shapes(const vimz_cf* v) {
  cfz::Shapes sh{};
  sh.len_z = v->pri->len_z; sh.n_w1 = v->pri->n_wires; sh.n_c1 = v->pri->n_c; sh.n_w2 = v->sec.n_w; sh.n_c2 = v->sec.n_c;
  sh.s1 = ceil_log2(sh.n_c1); sh.t1 = ceil_log2(sh.n_w1); sh.s2 = ceil_log2(sh.n_c2); sh.t2 = ceil_log2(sh.n_w2);
  return sh;
}
struct CfLoaded { CfMainRelaxed U; G1Aff UW, UE; CfMainFresh u; G1Aff uW; CfRelaxed cfU; };
Instance<Fe, Fq> cf_inst_running(const CfLoaded& L) { return instance2<Fe, Fq>(L.UW, L.UE, L.U.u, L.U.x0, L.U.x1, true); }
Instance<Fe, Fq> cf_inst_fresh(const CfLoaded& L) { return instance2<Fe, Fq>(L.uW, g1_identity(), Fe::one(), L.u.x0, L.u.x1, false); }
Instance<Fq, Fe> cf_inst_cyclefold(const G2Aff& cW, const G2Aff& cE, const Fq& u, const Fq* x) {
  static_assert(CF_IO <= (int)MAX_PUB, "a CycleFold instance's public elements must fit an Instance");
  Instance<Fq, Fe> I; I.cW = cW; I.cE = cE; I.u = u; I.n_pub = CF_IO; I.has_E = true;
  for (int k = 0; k < CF_IO; k++) I.X[k] = x[k];
  return I;
}
Instance<Fq, Fe> cf_inst_cyclefold(const CfLoaded& L) {
  Fq x[CF_IO];
  for (int k = 0; k < CF_IO; k++) x[k] = from_u256<Fq>(L.cfU.x[k]);
  return cf_inst_cyclefold(L.cfU.W, L.cfU.E, cross_field<Fq>(L.cfU.u), x);      // u is a small integer: the same in both fields
}
}  // namespace
extern "C" {

size_t vimz_cf_compressed_size(vimz_cf* v) {
  if (!v) return 0;
  return 8 * cfz::chain_words(cf_shapes(v));
}

int vimz_cf_compress(vimz_cf* v, uint8_t* blob, size_t cap, double seconds[2]) {
  if (!v || !blob) return VIMZ_ERR_INVALID;
  vimz_ctx* ctx = v->ctx;
  if (cap < vimz_cf_compressed_size(v)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_cf_compress: buffer too small");
  if (v->broken) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_cf_compress: this IVC failed in the middle of a step");
  if (v->i == 0) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_cf_compress: nothing has been folded");
  double t0 = now_s();
  SpartanCache* cache = nullptr;
  int rc = spartan_setup_cf(v, &cache);
  if (rc) return rc;
  const double t_setup = now_s() - t0;
  t0 = now_s();
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  P_TRY(hipStreamSynchronize(s));
  vimz_prover* p = v->pri;
  const cfz::Shapes sh = cf_shapes(v);
  CfLoaded L; L.U = v->U; L.UW = v->UW; L.UE = v->UE; L.u = v->u; L.uW = v->uW; L.cfU = v->cfU;
  Writer out;
  out.word(cfz::CHAIN_MAGIC); out.word(v->i); out.word(p->len_z); out.word(sh.s1); out.word(sh.t1); out.word(sh.s2); out.word(sh.t2); out.word(0);
  for (auto& z : v->z0) out.fe(z);
  for (auto& z : p->z_cur) out.fe(z);
  out.point(L.UW); out.point(L.UE); out.fe(L.U.u); out.fe(L.U.x0); out.fe(L.U.x1);
  out.point(L.uW); out.fe(L.u.x0); out.fe(L.u.x1);
  out.point(L.cfU.W); out.point(L.cfU.E); out.fe(L.cfU.u); for (auto& e : L.cfU.x) out.u256(e);
  Transcript tr("vimz-cf-compressed-v1");
  bind_statement(tr, v->i, v->z0, p->z_cur);
  tr.absorb_words("inst", out.w.data() + 8 + 8 * p->len_z, cfz::CHAIN_INSTANCE_WORDS);
  auto fwd1 = [&](const uint32_t* z, uint32_t* az, uint32_t* bz, uint32_t* cz) { launch_spmv(p, s, z, az, bz, cz, 0); };
  auto fwd2 = [&](const uint32_t* z, uint32_t* az, uint32_t* bz, uint32_t* cz) { sec_spmv<Fq>(v->sec, s, z, az, bz, cz); };
  const Fq cf_digest = cross_field<Fq>(v->c1->digest);      // (SHA3 of BOTH shapes, 250 bits: the same integer in either field)
  if ((rc = spartan_prove<Fe, BnG1>(ctx, *cache, cache->side[0], s, v->ck1, cache->ipa_u1, v->c1->digest, cf_inst_running(L), p->Zrun, p->E, 1, tr, out, fwd1))) return rc;
  if ((rc = spartan_prove<Fe, BnG1>(ctx, *cache, cache->side[0], s, v->ck1, cache->ipa_u1, v->c1->digest, cf_inst_fresh(L), v->Zl, nullptr, 3, tr, out, fwd1))) return rc;
  if ((rc = spartan_prove<Fq, Grumpkin>(ctx, *cache, cache->side[1], s, v->ck2, cache->ipa_u2, cf_digest, cf_inst_cyclefold(L), v->sec.Zrun, v->sec.E, 2, tr, out, fwd2))) return rc;
  if (8 * out.w.size() != vimz_cf_compressed_size(v)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_cf_compress: internal size mismatch");
  memcpy(blob, out.w.data(), 8 * out.w.size());
  if (seconds) { seconds[0] = t_setup; seconds[1] = now_s() - t0; }
  return VIMZ_OK;
}

// verify(vk, num_steps, z0).  `vk`: any vimz_cf created for the same step circuit and commitment keys (its folding state is neither read nor changed).
// result: 0 = accepted; bit 0 / 1 the hash x0 / x1 carried by u_n; bit 2 / 3 / 4 the argument for U_n / cfU_n / u_n; bit 12 the statement (steps, z0)
// differs; bit 13 malformed proof (also: a blob of another kind).
}  // extern "C"
namespace {
template <class V>
int cf_verify_compressed_impl(V& vf, vimz_cf* v, const uint8_t* blob, size_t len, uint64_t num_steps, const uint64_t* z0, uint32_t* result) {
  if (!v || !blob || !z0 || !result) return VIMZ_ERR_INVALID;
  vimz_ctx* ctx = v->ctx;
  SpartanCache* cache = nullptr;
  int rc = spartan_setup_cf(v, &cache);
  if (rc) return rc;
  if (len & 7) { *result = 8192; return VIMZ_OK; }
  std::vector<uint64_t> words(len / 8); if (len) memcpy(words.data(), blob, len);
  const cfz::Shapes sh = cf_shapes(v);
  cfz::ChainFrame fr;
  if (!cfz::parse_chain(words.data(), words.size(), sh, &fr)) { *result = 8192; return VIMZ_OK; }
  Reader in{words.data(), words.size()};
  in.pos = fr.z0_at;
  vimz_prover* p = v->pri;
  const size_t lz = p->len_z;
  const uint64_t steps = fr.steps;
  uint32_t res = 0;
  std::vector<Fe> z0p(lz), zn(lz), z0c(lz);
  for (auto& z : z0p) z = in.fe<Fe>();
  for (auto& z : zn) z = in.fe<Fe>();
  for (uint32_t k = 0; k < lz; k++) { Fe c; memcpy(c.v, z0 + 4 * k, 32); if (!c.is_reduced()) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_cf_verify_compressed: z0 element not below the modulus"); z0c[k] = Fe::to_mont(c); }
  if (steps != num_steps || steps == 0) res |= 4096;
  for (uint32_t k = 0; k < lz; k++) if (!z0c[k].eq(z0p[k])) res |= 4096;
  CfLoaded L;
  L.UW = in.point<Fq>(); L.UE = in.point<Fq>(); L.U.u = in.fe<Fe>(); L.U.x0 = in.fe<Fe>(); L.U.x1 = in.fe<Fe>();
  L.uW = in.point<Fq>(); L.u.x0 = in.fe<Fe>(); L.u.x1 = in.fe<Fe>();
  L.cfU.W = in.point<Fe>(); L.cfU.E = in.point<Fe>(); L.cfU.u = in.fe<Fe>();
  for (auto& e : L.cfU.x) { e = in.u256(); Fq c; memcpy(c.v, e.w, 32); if (!c.is_reduced()) in.ok = false; }
  if (!in.ok || in.pos != fr.args_at) { *result = 8192; return VIMZ_OK; }
  L.U.W = nn_point(L.UW); L.U.E = nn_point(L.UE); L.u.W = nn_point(L.uW);
  // the two hashes u_n carries, recomputed from the verifier's own digest and the CLAIMED z0
  if (!cf_hash_main(v->c1->digest, steps, z0c, zn.data(), L.U).eq(L.u.x0)) res |= 1;
  if (!cf_hash_cf(v->c1->digest, L.cfU).eq(L.u.x1)) res |= 2;
  typename V::Lock g(ctx->mu);
  if (V::on_device) P_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  Transcript tr("vimz-cf-compressed-v1");
  bind_statement(tr, steps, z0p, zn);
  tr.absorb_words("inst", words.data() + fr.inst_at, cfz::CHAIN_INSTANCE_WORDS);
  const cb::Builder& b1 = v->circ->build->b; const cb::BuilderT<Fq>& b2 = v->cf.b;
  const Fq cf_digest = cross_field<Fq>(v->c1->digest);
  bool ok1 = false, ok3 = false, ok2 = false;
  try {
    ok1 = vf.template arg<Fe, BnG1>(ctx, *cache, cache->side[0], s, v->ck1, cache->ipa_u1, v->c1->digest, cf_inst_running(L), b1, 1, tr, in);
    ok3 = ok1 && vf.template arg<Fe, BnG1>(ctx, *cache, cache->side[0], s, v->ck1, cache->ipa_u1, v->c1->digest, cf_inst_fresh(L), b1, 3, tr, in);
    ok2 = ok3 && vf.template arg<Fq, Grumpkin>(ctx, *cache, cache->side[1], s, v->ck2, cache->ipa_u2, cf_digest, cf_inst_cyclefold(L), b2, 2, tr, in);
  } catch (const std::exception& e) { return vz_fail(ctx, VIMZ_ERR_INVALID, e.what()); }
  if (!ok1) res |= 4;
  if (ok1 && !ok3) res |= 16;
  if (ok1 && ok3 && !ok2) res |= 8;
  if (!in.ok || (ok2 && in.pos != in.n)) res |= 8192;
  *result = res;
  return VIMZ_OK;
}
}  // namespace
extern "C" {
int vimz_cf_verify_compressed(vimz_cf* v, const uint8_t* blob, size_t len, uint64_t num_steps, const uint64_t* z0, uint32_t* result) {
  SingleVerify vf;
  return cf_verify_compressed_impl(vf, v, blob, len, num_steps, z0, result);
}

size_t vimz_cf_merged_compressed_size(const vimz_cf_merged* m) {
  if (!m || !m->vk) return 0;
  const cfz::Shapes sh = cf_shapes(m->vk);
  return 8 * (2 + cfz::records_words(sh, m->segs.size(), m->run_start.size()) + cfz::arg_words(sh.s1, sh.t1, true) + cfz::arg_words(sh.s2, sh.t2, true));
}

int vimz_cf_merged_compress(vimz_cf_merged* m, uint8_t* blob, size_t cap, double seconds[2]) {
  if (!m || !blob) return VIMZ_ERR_INVALID;
  if (!m->vk || !m->dev) return vz_fail(nullptr, VIMZ_ERR_INVALID, "vimz_cf_merged_compress: the prover this object was made with has been freed");
  vimz_cf* v = m->vk; vimz_ctx* ctx = v->ctx;
  if (m->broken || m->segs.empty()) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_cf_merged_compress: this object failed in the middle of a merge");
  if (cap < vimz_cf_merged_compressed_size(m)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_cf_merged_compress: buffer too small");
  double t0 = now_s();
  SpartanCache* cache = nullptr;
  int rc = spartan_setup_cf(v, &cache);
  if (rc) return rc;
  const double t_setup = now_s() - t0;
  t0 = now_s();
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  P_TRY(hipStreamSynchronize(s));
  vimz_prover* p = v->pri;
  const std::vector<uint64_t> rec = vz::cf_merged_records_words(m);
  Writer out;
  out.word(cfz::MERGED_MAGIC); out.word(rec.size());
  out.w.insert(out.w.end(), rec.begin(), rec.end());
  Transcript tr("vimz-cf-merged-compressed-v1");
  tr.absorb_words("records", out.w.data() + 2, out.w.size() - 2);
  const Instance<Fe, Fq> I1 = instance2<Fe, Fq>(m->acc.cW, m->acc.cE, m->acc.u, m->acc.x0, m->acc.x1, true);
  const Instance<Fq, Fe> I2 = cf_inst_cyclefold(m->acc.qW, m->acc.qE, m->acc.qu, m->acc.qx);
  auto fwd1 = [&](const uint32_t* z, uint32_t* az, uint32_t* bz, uint32_t* cz) { launch_spmv(p, s, z, az, bz, cz, 0); };
  auto fwd2 = [&](const uint32_t* z, uint32_t* az, uint32_t* bz, uint32_t* cz) { sec_spmv<Fq>(v->sec, s, z, az, bz, cz); };
  if ((rc = spartan_prove<Fe, BnG1>(ctx, *cache, cache->side[0], s, v->ck1, cache->ipa_u1, v->c1->digest, I1, m->Zp, m->Ep, 1, tr, out, fwd1))) return rc;
  if ((rc = spartan_prove<Fq, Grumpkin>(ctx, *cache, cache->side[1], s, v->ck2, cache->ipa_u2, cross_field<Fq>(v->c1->digest), I2, m->Zq, m->Eq, 2, tr, out, fwd2))) return rc;
  if (8 * out.w.size() != vimz_cf_merged_compressed_size(m)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_cf_merged_compress: internal size mismatch");
  memcpy(blob, out.w.data(), 8 * out.w.size());
  if (seconds) { seconds[0] = t_setup; seconds[1] = now_s() - t0; }
  return VIMZ_OK;
}

// verify(vk, num_steps, z0) of a compressed merged Nova + CycleFold proof.  result: 0 = accepted; bit 0 / 1 a segment's main / CycleFold hash; bit 2 / 3
// the argument for the folded main / CycleFold instance; bit 12 statement (steps, z0, adjacency); bit 13 malformed (also: a blob of another kind).
}  // extern "C"
namespace {
template <class V>
int cf_verify_merged_compressed_impl(V& vf, vimz_cf* v, const uint8_t* blob, size_t len, uint64_t num_steps, const uint64_t* z0, uint32_t* result) {
  if (!v || !blob || !z0 || !result) return VIMZ_ERR_INVALID;
  vimz_ctx* ctx = v->ctx;
  SpartanCache* cache = nullptr;
  int rc = spartan_setup_cf(v, &cache);
  if (rc) return rc;
  if (len & 7) { *result = 8192; return VIMZ_OK; }
  std::vector<uint64_t> words(len / 8); if (len) memcpy(words.data(), blob, len);
  const cfz::Shapes sh = cf_shapes(v);
  cfz::MergedFrame fr;
  if (!cfz::parse_merged(words.data(), words.size(), sh, &fr)) { *result = 8192; return VIMZ_OK; }
  std::vector<CfSegRec> segs; std::vector<uint32_t> run_start; std::vector<CfJunction> junctions;
  if (!vz::cf_merged_read_records(v, words.data() + fr.rec_at, fr.rec_words, segs, run_start, junctions)) { *result = 8192; return VIMZ_OK; }
  uint32_t res = 0, fl = 0;
  CfAcc R;
  if (!vz::cf_merged_replay(v, segs, run_start, junctions, R, &fl)) { *result = 8192; return VIMZ_OK; }
  if (fl & 1) res |= 1;
  if (fl & 2) res |= 2;
  if (fl & 4) res |= 4096;
  vimz_prover* p = v->pri;
  if (R.n != num_steps) res |= 4096;
  for (uint32_t k = 0; k < p->len_z; k++) {
    Fe c; memcpy(c.v, z0 + 4 * k, 32);
    if (!c.is_reduced()) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_cf_verify_merged_compressed: z0 element not below the modulus");
    if (!Fe::to_mont(c).eq(R.zs[k])) res |= 4096;
  }
  typename V::Lock g(ctx->mu);
  if (V::on_device) P_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  Transcript tr("vimz-cf-merged-compressed-v1");
  tr.absorb_words("records", words.data() + fr.rec_at, fr.rec_words);
  const Instance<Fe, Fq> I1 = instance2<Fe, Fq>(R.cW, R.cE, R.u, R.x0, R.x1, true);
  const Instance<Fq, Fe> I2 = cf_inst_cyclefold(R.qW, R.qE, R.qu, R.qx);
  const cb::Builder& b1 = v->circ->build->b; const cb::BuilderT<Fq>& b2 = v->cf.b;
  Reader in{words.data(), words.size()};
  in.pos = fr.args_at;
  bool ok1 = false, ok2 = false;
  try {
    ok1 = vf.template arg<Fe, BnG1>(ctx, *cache, cache->side[0], s, v->ck1, cache->ipa_u1, v->c1->digest, I1, b1, 1, tr, in);
    ok2 = ok1 && vf.template arg<Fq, Grumpkin>(ctx, *cache, cache->side[1], s, v->ck2, cache->ipa_u2, cross_field<Fq>(v->c1->digest), I2, b2, 2, tr, in);
  } catch (const std::exception& e) { return vz_fail(ctx, VIMZ_ERR_INVALID, e.what()); }
  if (!ok1) res |= 4;
  if (ok1 && !ok2) res |= 8;
  if (!in.ok || (ok2 && in.pos != in.n)) res |= 8192;
  *result = res;
  return VIMZ_OK;
}
}  // namespace
extern "C" {
int vimz_cf_verify_merged_compressed(vimz_cf* v, const uint8_t* blob, size_t len, uint64_t num_steps, const uint64_t* z0, uint32_t* result) {
  SingleVerify vf;
  return cf_verify_merged_compressed_impl(vf, v, blob, len, num_steps, z0, result);
}

}  // extern "C"

// ---- many compressed proofs in one call ---------------------------------------------------------------------------------------------------------------------
#include "spartan_batch.hpp"
namespace {
uint64_t first_word(const uint8_t* blob, size_t len) { uint64_t w = 0; if (blob && len >= 8) memcpy(&w, blob, 8); return w; }

int ivc_compressed_batch(const char* who, vimz_ivc* vk, size_t n, const uint8_t* const* blobs, const size_t* lens, const uint64_t* steps, const uint64_t* z0, size_t chunk,
                         const uint64_t* given, uint32_t* results, double seconds[6], BatchProbe* probe, uint32_t flags, size_t leaf, uint64_t* stats) {
  if (!vk) return VIMZ_ERR_INVALID;
  vimz_ctx* ctx = vk->ctx;
  if (n && (!blobs || !lens || !steps || !z0 || !results)) return vz_fail(ctx, VIMZ_ERR_INVALID, "compressed batch: NULL argument");
  for (size_t i = 0; i < n; i++) if (!blobs[i]) return vz_fail(ctx, VIMZ_ERR_INVALID, "compressed batch: NULL blob");
  SpartanCache* cache = nullptr;
  int rc = spartan_setup(vk, &cache);
  if (rc) return rc;
  const size_t lz = vk->pri->len_z;
  // what a caller can get wrong is refused here, on the calling thread, before any result is written (the single entries refuse it proof by proof)
  for (size_t k = 0; k < 4 * lz * n; k += 4) { Fe c; memcpy(c.v, z0 + k, 32); if (!c.is_reduced()) return vz_fail(ctx, VIMZ_ERR_INVALID, "compressed batch: z0 element not below the modulus"); }
  auto kind = [&](size_t i) { const uint64_t w = first_word(blobs[i], lens[i]); return w == CSNARK_MAGIC ? 1 : w == CMERGED_MAGIC ? 2 : 0; };
  auto run = [&](auto& vf, size_t i, uint32_t* res) -> int {
    switch (kind(i)) {
      case 1: return ivc_verify_compressed_impl(vf, vk, blobs[i], lens[i], steps[i], z0 + 4 * lz * i, res);
      case 2: return ivc_verify_merged_compressed_impl(vf, vk, blobs[i], lens[i], steps[i], z0 + 4 * lz * i, res);
      default: *res = 8192; return VIMZ_OK;      // neither kind of this family
    }
  };
  return compressed_batch(who, ctx, cache, vk->ck1, vk->ck2, n, chunk, given, [&](size_t i, DeferredVerify& vf, uint32_t* res) { return run(vf, i, res); },
                          [&](size_t i, uint32_t* res) { SingleVerify vf; return run(vf, i, res); }, results, seconds, probe, flags, leaf, stats);
}

int cf_compressed_batch(const char* who, vimz_cf* vk, size_t n, const uint8_t* const* blobs, const size_t* lens, const uint64_t* steps, const uint64_t* z0, size_t chunk,
                        const uint64_t* given, uint32_t* results, double seconds[6], BatchProbe* probe, uint32_t flags, size_t leaf, uint64_t* stats) {
  if (!vk) return VIMZ_ERR_INVALID;
  vimz_ctx* ctx = vk->ctx;
  if (n && (!blobs || !lens || !steps || !z0 || !results)) return vz_fail(ctx, VIMZ_ERR_INVALID, "compressed batch: NULL argument");
  for (size_t i = 0; i < n; i++) if (!blobs[i]) return vz_fail(ctx, VIMZ_ERR_INVALID, "compressed batch: NULL blob");
  SpartanCache* cache = nullptr;
  int rc = spartan_setup_cf(vk, &cache);
  if (rc) return rc;
  const size_t lz = vk->pri->len_z;
  // what a caller can get wrong is refused here, on the calling thread, before any result is written (the single entries refuse it proof by proof)
  for (size_t k = 0; k < 4 * lz * n; k += 4) { Fe c; memcpy(c.v, z0 + k, 32); if (!c.is_reduced()) return vz_fail(ctx, VIMZ_ERR_INVALID, "compressed batch: z0 element not below the modulus"); }
  auto kind = [&](size_t i) { const uint64_t w = first_word(blobs[i], lens[i]); return w == cfz::CHAIN_MAGIC ? 1 : w == cfz::MERGED_MAGIC ? 2 : 0; };
  auto run = [&](auto& vf, size_t i, uint32_t* res) -> int {
    switch (kind(i)) {
      case 1: return cf_verify_compressed_impl(vf, vk, blobs[i], lens[i], steps[i], z0 + 4 * lz * i, res);
      case 2: return cf_verify_merged_compressed_impl(vf, vk, blobs[i], lens[i], steps[i], z0 + 4 * lz * i, res);
      default: *res = 8192; return VIMZ_OK;
    }
  };
  return compressed_batch(who, ctx, cache, vk->ck1, vk->ck2, n, chunk, given, [&](size_t i, DeferredVerify& vf, uint32_t* res) { return run(vf, i, res); },
                          [&](size_t i, uint32_t* res) { SingleVerify vf; return run(vf, i, res); }, results, seconds, probe, flags, leaf, stats);
}
}  // namespace

extern "C" {

// Many compressed proofs under one verifier key in one call.  blobs[i] / lens[i]: what vimz_ivc_compress or vimz_ivc_merged_compress wrote (the first word tells
// which; the two kinds may be mixed; anything else — a Nova + CycleFold blob among them — gets bit 13); steps[i] and z0 + 4·len_z·i: the statement of proof i.
// results[i] = the word vimz_ivc_verify_compressed / vimz_ivc_verify_merged_compressed gives for proof i alone.  chunk: proofs an equation (0 = 32); a refused
// chunk is bisected down to refused subsets of `leaf` members, which the single verifier judges member by member (spartan_batch.hpp).  n = 0 is accepted.
// seconds[6] (optional): parse + host checks, half-tables, matrix evaluation, s-vector accumulation, MSMs, fallback.  flags, leaf, stats: include/vimz_hip.h.
int vimz_ivc_verify_compressed_batch(vimz_ivc* vk, size_t n, const uint8_t* const* blobs, const size_t* lens, const uint64_t* steps, const uint64_t* z0, size_t chunk,
                                     uint32_t* results, double seconds[6]) {
  return vimz_ivc_verify_batch_compressed_ex(vk, n, blobs, lens, steps, z0, chunk, results, seconds, 0, 0, nullptr);
}
int vimz_ivc_verify_batch_compressed_ex(vimz_ivc* vk, size_t n, const uint8_t* const* blobs, const size_t* lens, const uint64_t* steps, const uint64_t* z0, size_t chunk,
                                        uint32_t* results, double seconds[6], uint32_t flags, size_t leaf, uint64_t stats[4]) {
  return ivc_compressed_batch("vimz_ivc_verify_compressed_batch", vk, n, blobs, lens, steps, z0, chunk, nullptr, results, seconds, nullptr, flags, leaf, stats);
}
// The same for what vimz_cf_compress / vimz_cf_merged_compress wrote; results[i] = vimz_cf_verify_compressed's / vimz_cf_verify_merged_compressed's word.
int vimz_cf_verify_compressed_batch(vimz_cf* vk, size_t n, const uint8_t* const* blobs, const size_t* lens, const uint64_t* steps, const uint64_t* z0, size_t chunk,
                                    uint32_t* results, double seconds[6]) {
  return vimz_cf_verify_batch_compressed_ex(vk, n, blobs, lens, steps, z0, chunk, results, seconds, 0, 0, nullptr);
}
int vimz_cf_verify_batch_compressed_ex(vimz_cf* vk, size_t n, const uint8_t* const* blobs, const size_t* lens, const uint64_t* steps, const uint64_t* z0, size_t chunk,
                                       uint32_t* results, double seconds[6], uint32_t flags, size_t leaf, uint64_t stats[4]) {
  return cf_compressed_batch("vimz_cf_verify_compressed_batch", vk, n, blobs, lens, steps, z0, chunk, nullptr, results, seconds, nullptr, flags, leaf, stats);
}

}  // extern "C"

#ifdef VIMZ_TESTING
// ---- test hooks (include/vimz_hip_testing.h): in libvimz_hip_testing.so only.  Every launch below goes through the functions the prover runs. ----------------
#include "r1cs_handle.hpp"

namespace {

struct TestSide {          // one side's scratch (and, for a whole instance, its shape) for the length of a hook
  SpartanCache cache;
  SideDev& S = cache.side[0];
  ~TestSide() { for (void* d : cache.owned) hipFree(d); if (S.pin) hipHostFree(S.pin); cache.ws.release(); }
};

template <class F>
bool canon_in(const uint64_t* src, size_t n, std::vector<F>& out) {        // canonical words -> Montgomery elements; false: one is not below the modulus
  out.resize(n);
  for (size_t i = 0; i < n; i++) { F c; memcpy(c.v, src + 4 * i, 32); if (!c.is_reduced()) return false; out[i] = F::to_mont(c); }
  return true;
}
template <class F>
void canon_out(uint64_t* dst, const F& mont) { const F c = F::from_mont(mont); memcpy(dst, c.v, 32); }

template <class F>
hipError_t vec_up(hipStream_t s, uint32_t* d, const std::vector<F>& v) { return hipMemcpyAsync(d, v.data(), 32 * v.size(), hipMemcpyHostToDevice, s); }
template <class F>
hipError_t elem_down(hipStream_t s, const uint32_t* d, F* out) {
  hipError_t e = hipMemcpyAsync(out->v, d, 32, hipMemcpyDeviceToHost, s);
  return e != hipSuccess ? e : hipStreamSynchronize(s);
}

template <class Fn>
int scalar_field_dispatch(int field, Fn fn) {
  if (field == VIMZ_FIELD_BN254_FR) return fn(Fe());
  if (field == VIMZ_FIELD_BN254_FQ) return fn(Fq());
  return VIMZ_ERR_INVALID;
}

template <class F>
int test_eq(vimz_ctx* ctx, const uint64_t* point, size_t k, uint64_t* table_out) {
  std::vector<F> pt;
  if (!canon_in(point, k, pt)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_eq: element not below the modulus");
  const size_t n = (size_t)1 << k;
  TestSide T; hipStream_t s = ctx->stream;
  P_TRY(side_alloc(T.S, n, T.cache.owned));
  P_TRY(eq_build<F>(s, T.S.eq, pt));
  launch_from_mont<F>(s, T.S.eq, T.S.va, n);
  P_TRY(hipGetLastError());
  P_TRY(hipMemcpyAsync(table_out, T.S.va, 32 * n, hipMemcpyDeviceToHost, s));
  P_TRY(hipStreamSynchronize(s));
  return VIMZ_OK;
}

template <class F>
int test_sumcheck(vimz_ctx* ctx, int kind, size_t k, const uint64_t* const vecs[5], const uint64_t u[4], const uint64_t* challenges, uint64_t* msgs_out, uint64_t* finals_out) {
  const size_t n = (size_t)1 << k;
  const int nv = kind == 0 ? 5 : 2;
  const bool has_E = kind == 0 && vecs[4];
  std::vector<F> r, uu;
  if (!canon_in(challenges, k, r) || (kind == 0 && !canon_in(u, 1, uu))) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_sumcheck: element not below the modulus");
  TestSide T; SideDev& S = T.S; hipStream_t s = ctx->stream;
  P_TRY(side_alloc(S, n, T.cache.owned));
  uint32_t* dst[5] = {kind == 0 ? S.eq : S.vm, kind == 0 ? S.va : S.vz, S.vb, S.vc, S.ve};
  {
    std::vector<F> v;
    for (int q = 0; q < nv; q++) {
      if (!vecs[q]) continue;
      if (!canon_in(vecs[q], n, v)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_sumcheck: element not below the modulus");
      P_TRY(vec_up(s, dst[q], v));
      P_TRY(hipStreamSynchronize(s));
    }
  }
  size_t len = n;
  for (size_t j = 0; j < k; j++) {
    const size_t half = len >> 1;
    if (kind == 0)
      P_TRY(outer_round<F>(S, s, half, has_E, uu[0], [&](const F& s0, const F& s2, const F& s3) { canon_out(msgs_out + 12 * j, s0); canon_out(msgs_out + 12 * j + 4, s2); canon_out(msgs_out + 12 * j + 8, s3); return r[j]; }));
    else
      P_TRY(inner_round<F>(S, s, half, [&](const F& s0, const F& s2) { canon_out(msgs_out + 8 * j, s0); canon_out(msgs_out + 8 * j + 4, s2); return r[j]; }));
    len = half;
  }
  P_TRY(hipGetLastError());
  for (int q = 0; q < nv; q++) {
    F x = F::zero();
    if (q < 4 || has_E) P_TRY(elem_down(s, dst[q], &x));
    canon_out(finals_out + 4 * q, x);
  }
  return VIMZ_OK;
}

template <class F>
int test_ipa_vec(vimz_ctx* ctx, size_t k, const uint64_t* a, const uint64_t* b, const uint64_t* challenges, uint64_t* dots_out, uint64_t* finals_out) {
  const size_t n = (size_t)1 << k;
  std::vector<F> r, va, vb;
  if (!canon_in(challenges, k, r) || !canon_in(a, n, va) || !canon_in(b, n, vb)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_ipa_vec: element not below the modulus");
  TestSide T; SideDev& S = T.S; hipStream_t s = ctx->stream;
  P_TRY(side_alloc(S, n, T.cache.owned));
  P_TRY(vec_up(s, S.va, va)); P_TRY(vec_up(s, S.vb, vb));
  P_TRY(hipStreamSynchronize(s));
  size_t len = n;
  for (size_t j = 0; j < k; j++) {
    const size_t half = len >> 1;
    auto read_dots = [&](const uint32_t* pin, F* x) -> hipError_t {
      const hipError_t e = hipStreamSynchronize(s);
      if (e != hipSuccess) return e;
      F cl, cr; memcpy(cl.v, pin, 32); memcpy(cr.v, pin + 8, 32);
      canon_out(dots_out + 8 * j, cl); canon_out(dots_out + 8 * j + 4, cr);
      *x = r[j];
      return hipSuccess;
    };
    P_TRY(ipa_vec_round<F>(S, s, S.va, S.vb, half, read_dots));
    len = half;
  }
  P_TRY(hipGetLastError());
  F fa, fb;
  P_TRY(elem_down(s, S.va, &fa)); P_TRY(elem_down(s, S.vb, &fb));
  canon_out(finals_out, fa); canon_out(finals_out + 4, fb);
  return VIMZ_OK;
}

// canonical affine points (8 words each) -> Montgomery; 0: good, 1: a coordinate not below the modulus, 2: a point off the curve
template <class FS>
int points_in(const uint64_t* xy, size_t n, std::vector<Affine<FS>>& out) {
  out.resize(n);
  for (size_t i = 0; i < n; i++) {
    FS x, y; memcpy(x.v, xy + 8 * i, 32); memcpy(y.v, xy + 8 * i + 4, 32);
    if (!x.is_reduced() || !y.is_reduced()) return 1;
    out[i].x = FS::to_mont(x); out[i].y = FS::to_mont(y);
    if (!aff_on_curve(out[i])) return 2;
  }
  return 0;
}

template <class C>
int test_fold_bases(vimz_ctx* ctx, const uint64_t* points_xy, size_t half, const uint64_t x128[2], uint64_t* out_xy) {
  typedef typename C::Base FS;
  typedef typename C::Coord G;
  std::vector<Affine<FS>> pts;
  if (points_in(points_xy, 2 * half, pts)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_fold_bases: a coordinate not below the modulus, or a point off the curve");
  hipStream_t s = ctx->stream;
  uint32_t *raw = nullptr, *gd = nullptr;
  P_TRY(hipMalloc((void**)&raw, 64 * 2 * half));
  hipError_t e = hipMalloc((void**)&gd, 4 * (size_t)AFFINE_WORDS * 2 * half);
  if (e == hipSuccess) e = hipMemcpyAsync(raw, pts.data(), 64 * 2 * half, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    launch_points_to_internal<FS>(s, raw, 0, gd, 2 * half);
    const uint32_t xw[4] = {(uint32_t)x128[0], (uint32_t)(x128[0] >> 32), (uint32_t)x128[1], (uint32_t)(x128[1] >> 32)};
    ipa_fold_bases<G>(s, gd, half, xw);
    launch_points_from_internal<FS>(s, gd, 1, raw, half);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out_xy, raw, 64 * half, hipMemcpyDeviceToHost, s);
  const hipError_t e2 = hipStreamSynchronize(s);
  hipFree(raw); hipFree(gd);
  if (e != hipSuccess) return vz_fail(ctx, VIMZ_ERR_HIP, "vimz_test_spartan_fold_bases", e);
  if (e2 != hipSuccess) return vz_fail(ctx, VIMZ_ERR_HIP, "vimz_test_spartan_fold_bases: synchronize", e2);
  return VIMZ_OK;
}

// the shape of a whole-instance hook: the seam's upload for the forward side, its CSR read back for build_transpose and the verifier
template <class F>
struct TestShape { cb::Csr A, B, C; std::vector<F> dict; };

template <class F>
int test_side_build(vimz_ctx* ctx, const vimz_r1cs* R, const vimz_bases* ck, TestSide& T, TestShape<F>& H) {
  SideDev& S = T.S;
  cb::Csr* Ms[3] = {&H.A, &H.B, &H.C};
  for (int m = 0; m < 3; m++) {
    Ms[m]->row_ptr.assign(R->nrows + 1, 0); Ms[m]->col.resize(R->nnz[m]); Ms[m]->coef.resize(R->nnz[m]);
    P_TRY(hipMemcpy(Ms[m]->row_ptr.data(), R->M[m].row_ptr, 4 * (R->nrows + 1), hipMemcpyDeviceToHost));
    if (R->nnz[m]) { P_TRY(hipMemcpy(Ms[m]->col.data(), R->M[m].col, 4 * R->nnz[m], hipMemcpyDeviceToHost)); P_TRY(hipMemcpy(Ms[m]->coef.data(), R->M[m].coef, 4 * R->nnz[m], hipMemcpyDeviceToHost)); }
  }
  {
    std::vector<F> dd(2 * R->ndict);
    if (R->ndict) P_TRY(hipMemcpy(dd.data(), R->dict, 32 * dd.size(), hipMemcpyDeviceToHost));
    H.dict.resize(R->ndict);
    for (size_t i = 0; i < R->ndict; i++) H.dict[i] = dd[2 * i];
  }
  S.A = R->M[0]; S.B = R->M[1]; S.C = R->M[2]; S.dict = R->dict; S.items = R->long_items; S.n_long = R->n_long; S.n_med = R->n_med;
  S.n_w = (uint32_t)R->ncols; S.n_c = (uint32_t)R->nrows;
  const cb::Csr* M3[3] = {&H.A, &H.B, &H.C};
  P_TRY(build_transpose<F>(M3, S.n_c, S.n_w, S, T.cache.owned));
  S.s = ceil_log2(S.n_c); S.t = ceil_log2(S.n_w); S.M = (size_t)1 << S.s; S.N = (size_t)1 << S.t;
  if (ck->n < std::max(S.M, S.N)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_instance: the commitment key is shorter than the padded shape");
  P_TRY(side_alloc(S, std::max(S.M, S.N), T.cache.owned));
  return VIMZ_OK;
}

template <class F, class C>
int64_t test_instance(vimz_ctx* ctx, int curve, const vimz_r1cs* R, const uint64_t* Zc, const uint64_t* Ec, const vimz_bases* ck, const uint64_t digest[4],
                      uint32_t side_tag, const char* label, uint32_t n_pub, void* buf, size_t cap) {
  typedef typename C::Base FS;
  std::vector<F> Z, E, dg;
  if (!canon_in(Zc, R->ncols, Z) || (Ec && !canon_in(Ec, R->nrows, E)) || !canon_in(digest, 1, dg)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_instance: element not below the modulus");
  Affine<FS> Ugen;
  int rc = derive_ipa_u<C>(ctx, curve, &Ugen);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  TestSide T; TestShape<F> H; SideDev& S = T.S;
  if ((rc = test_side_build<F>(ctx, R, ck, T, H))) return rc;
  uint32_t *Zd = nullptr, *Ed = nullptr;
  P_TRY(hipMalloc((void**)&Zd, 32 * Z.size())); T.cache.owned.push_back(Zd);
  P_TRY(vec_up(s, Zd, Z));
  if (Ec) { P_TRY(hipMalloc((void**)&Ed, 32 * E.size())); T.cache.owned.push_back(Ed); P_TRY(vec_up(s, Ed, E)); }
  P_TRY(hipStreamSynchronize(s));
  Instance<F, FS> I;
  I.u = Z[0]; I.n_pub = n_pub; I.has_E = Ec != nullptr;
  for (uint32_t k = 0; k < n_pub; k++) I.X[k] = Z[S.n_w - n_pub + k];
  I.cE.x = I.cE.y = FS::zero();
  P_TRY(msm_run<C>(s, T.cache.ws, ck->d, Zd + 8, (size_t)S.n_w - 1 - n_pub, 1, 0, &I.cW, nullptr, nullptr, 0, nullptr));          // wire i -> ck[i − 1], the committed wires 1 .. n_w − 1 − n_pub
  if (Ec) P_TRY(msm_run<C>(s, T.cache.ws, ck->d, Ed, (size_t)S.n_c, 1, 0, &I.cE, nullptr, nullptr, 0, nullptr));
  Transcript tr(label);
  Writer out;
  out.point(I.cW); out.point(I.cE);
  auto fwd = [&](const uint32_t* z, uint32_t* az, uint32_t* bz, uint32_t* cz) { spmv_any<F>(s, S.A, S.B, S.C, S.dict, S.items, S.n_long, S.n_med, S.n_c, z, az, bz, cz); };
  if ((rc = spartan_prove<F, C>(ctx, T.cache, S, s, ck, Ugen, dg[0], I, Zd, Ed, side_tag, tr, out, fwd))) return rc;
  P_TRY(hipStreamSynchronize(s));
  const size_t bytes = 8 * out.w.size();
  if (buf && cap >= bytes) memcpy(buf, out.w.data(), bytes);
  return (int64_t)bytes;
}

template <class F, class C>
int test_instance_verify(vimz_ctx* ctx, int curve, const vimz_r1cs* R, const vimz_bases* ck, const uint64_t digest[4], uint32_t side_tag, const char* label,
                         const uint64_t* inst, uint32_t n_pub, int has_E, const uint64_t* words, size_t n_words) {
  typedef typename C::Base FS;
  std::vector<F> sc, dg;
  std::vector<Affine<FS>> pts;
  if (!canon_in(inst + 16, 1 + n_pub, sc) || !canon_in(digest, 1, dg)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_instance_verify: element not below the modulus");
  const int bad = points_in(inst, 2, pts);
  if (bad == 1) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_instance_verify: coordinate not below the modulus");
  if (bad == 2) return 0;          // (a commitment off the curve: rejected, as Reader::point rejects one inside a proof)
  Affine<FS> Ugen;
  int rc = derive_ipa_u<C>(ctx, curve, &Ugen);
  if (rc) return rc;
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  TestSide T; TestShape<F> H;
  if ((rc = test_side_build<F>(ctx, R, ck, T, H))) return rc;
  Instance<F, FS> I;
  I.cW = pts[0]; I.cE = pts[1]; I.u = sc[0]; I.n_pub = n_pub; I.has_E = has_E != 0;
  for (uint32_t k = 0; k < n_pub; k++) I.X[k] = sc[1 + k];
  Transcript tr(label);
  Reader in{words, n_words};
  bool ok = false;
  try { ok = spartan_verify<F, C>(ctx, T.cache, T.S, s, ck, Ugen, dg[0], I, H, side_tag, tr, in); }
  catch (const std::exception& e) { return vz_fail(ctx, VIMZ_ERR_INVALID, e.what()); }
  P_TRY(hipStreamSynchronize(s));
  return ok && in.ok && in.pos == in.n ? 1 : 0;
}

template <class Fn>
int64_t instance_dispatch(vimz_ctx* ctx, int curve, size_t n_c, size_t n_w, uint32_t n_pub, const vimz_coo* A, const vimz_coo* B, const vimz_coo* C, const vimz_bases* ck, const char* who, Fn fn) {
  if (curve != VIMZ_CURVE_BN254_G1 && curve != VIMZ_CURVE_GRUMPKIN) return vz_fail(ctx, VIMZ_ERR_INVALID, who);
  if (n_pub < 1 || n_pub > MAX_PUB || n_w < (size_t)n_pub + 2) return vz_fail(ctx, VIMZ_ERR_INVALID, who);
  if (n_c < 2 || n_c > ((size_t)1 << 21) || n_w > ((size_t)1 << 21) || ck->curve != curve) return vz_fail(ctx, VIMZ_ERR_INVALID, who);
  size_t big = 1; while (big < std::max(n_c, n_w)) big <<= 1;
  if (ck->n < big) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_instance: the commitment key is shorter than the padded shape");
  vimz_r1cs* R = nullptr;
  const int rc = vimz_r1cs_upload(ctx, curve == VIMZ_CURVE_BN254_G1 ? VIMZ_FIELD_BN254_FR : VIMZ_FIELD_BN254_FQ, n_c, n_w, A, B, C, VIMZ_FORM_CANONICAL, &R);
  if (rc) return rc;
  int64_t out;
  try { out = fn(R); } catch (const std::exception& e) { out = vz_fail(ctx, VIMZ_ERR_INVALID, e.what()); }
  vimz_r1cs_free(ctx, R);
  return out;
}

// ---- the batch's kernels and its chunk logic on a caller's data (spartan_batch.hpp) ------------------------------------------------------------------------
template <class F>
int test_mat_eval(vimz_ctx* ctx, const vimz_r1cs* R, size_t n, const uint64_t* rx, const uint64_t* ry, const uint64_t* w, uint64_t* out) {
  SideDev S;
  S.A = R->M[0]; S.B = R->M[1]; S.C = R->M[2]; S.dict = R->dict; S.n_w = (uint32_t)R->ncols; S.n_c = (uint32_t)R->nrows;
  S.s = ceil_log2(S.n_c); S.t = ceil_log2(S.n_w); S.M = (size_t)1 << S.s; S.N = (size_t)1 << S.t;
  std::vector<std::vector<F>> px(n), py(n), pw(n);
  std::vector<const std::vector<F>*> qx(n), qy(n); std::vector<const F*> qw(n);
  for (size_t i = 0; i < n; i++) {
    if (!canon_in(rx + 4 * S.s * i, S.s, px[i]) || !canon_in(ry + 4 * S.t * i, S.t, py[i]) || !canon_in(w + 12 * i, 3, pw[i]))
      return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_mat_eval: element not below the modulus");
    qx[i] = &px[i]; qy[i] = &py[i]; qw[i] = pw[i].data();
  }
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  BatchDev D;
  P_TRY(D.alloc());
  std::vector<F> vm;
  P_TRY(batch_mat_eval<F>(ctx->stream, S, D, qx, qy, qw, vm, nullptr));
  for (size_t i = 0; i < n; i++) canon_out(out + 4 * i, vm[i]);
  return VIMZ_OK;
}

template <class F>
int test_svec_accum(vimz_ctx* ctx, uint32_t rounds, size_t n, const uint64_t* xs, const uint64_t* pts, const uint64_t* coefs, const uint32_t* shifted, const uint32_t* n_pub,
                    const uint32_t* n_w, uint64_t* acc_out, uint64_t* dots_out) {
  std::vector<std::vector<F>> px(n), pp(n); std::vector<F> cf;
  if (!canon_in(coefs, n, cf)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_svec_accum: element not below the modulus");
  std::vector<SvecItem<F>> items(n);
  for (size_t i = 0; i < n; i++) {
    if (!canon_in(xs + 4 * (size_t)rounds * i, rounds, px[i]) || !canon_in(pts + 4 * (size_t)rounds * i, rounds, pp[i]))
      return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_svec_accum: element not below the modulus");
    items[i] = SvecItem<F>{&px[i], &pp[i], cf[i], shifted[i] ? 1u : 0u, n_pub[i], n_w[i]};
  }
  const size_t len = (size_t)1 << rounds;
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  BatchDev D;
  P_TRY(D.alloc());
  struct Dev { uint32_t *a = nullptr, *b = nullptr; ~Dev() { hipFree(a); hipFree(b); } } d;
  P_TRY(hipMalloc((void**)&d.a, 32 * len)); P_TRY(hipMalloc((void**)&d.b, 32 * len));
  P_TRY(hipMemsetAsync(d.a, 0, 32 * len, s));
  std::vector<F> bfin;
  P_TRY(batch_svec_accum<F>(s, D, rounds, items, d.a, bfin, nullptr));
  launch_from_mont<F>(s, d.a, d.b, len);
  P_TRY(hipGetLastError());
  P_TRY(hipMemcpyAsync(acc_out, d.b, 32 * len, hipMemcpyDeviceToHost, s));
  P_TRY(hipStreamSynchronize(s));
  for (size_t i = 0; i < n; i++) canon_out(dots_out + 4 * i, bfin[i]);
  return VIMZ_OK;
}

// one instance's word (1 = accepted) under either policy: what test_instance_verify computes
template <class F, class C, class V>
int test_instance_word(V& vf, vimz_ctx* ctx, TestSide& T, SideDev& S, const TestShape<F>& H, const vimz_bases* ck, const Affine<typename C::Base>& Ugen, const F& dg,
                       uint32_t side_tag, const char* label, const uint64_t* inst, uint32_t n_pub, int has_E, const uint64_t* words, size_t n_words, uint32_t* res) {
  typedef typename C::Base FS;
  std::vector<F> sc;
  std::vector<Affine<FS>> pts;
  if (!canon_in(inst + 16, 1 + n_pub, sc)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_instance_batch: element not below the modulus");
  const int bad = points_in(inst, 2, pts);
  if (bad == 1) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_instance_batch: coordinate not below the modulus");
  if (bad == 2) { *res = 0; return VIMZ_OK; }
  Instance<F, FS> I;
  I.cW = pts[0]; I.cE = pts[1]; I.u = sc[0]; I.n_pub = n_pub; I.has_E = has_E != 0;
  for (uint32_t k = 0; k < n_pub; k++) I.X[k] = sc[1 + k];
  typename V::Lock g(ctx->mu);
  if (V::on_device) P_TRY(hipSetDevice(ctx->device));
  Transcript tr(label);
  Reader in{words, n_words};
  const bool ok = vf.template arg<F, C>(ctx, T.cache, S, ctx->stream, ck, Ugen, dg, I, H, side_tag, tr, in);
  if (V::on_device) P_TRY(hipStreamSynchronize(ctx->stream));
  *res = ok && in.ok && in.pos == in.n ? 1u : 0u;
  return VIMZ_OK;
}

template <class F, class C>
int test_instance_batch(vimz_ctx* ctx, int curve, const vimz_r1cs* R, const vimz_bases* ck, const uint64_t digest[4], uint32_t side_tag, const char* label, uint32_t n_pub,
                        size_t n, const uint64_t* inst, const int* has_E, const uint64_t* const* words, const size_t* n_words, size_t chunk, const uint64_t* multipliers,
                        uint32_t* results, double seconds[6], uint64_t* acc_out, uint32_t flags, size_t leaf, uint64_t* stats) {
  typedef typename C::Base FS;
  std::vector<F> dg;
  if (!canon_in(digest, 1, dg)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_instance_batch: element not below the modulus");
  Affine<FS> Ugen;
  int rc = derive_ipa_u<C>(ctx, curve, &Ugen);
  if (rc) return rc;
  TestSide T; TestShape<F> H;
  {
    std::lock_guard<std::mutex> g(ctx->mu);
    P_TRY(hipSetDevice(ctx->device));
    if ((rc = test_side_build<F>(ctx, R, ck, T, H))) return rc;
  }
  const int side = std::is_same<F, Fe>::value ? 0 : 1;
  if (side == 1) T.cache.side[1] = T.cache.side[0];      // (the Fq side of a batch is side[1]; TestSide frees the scratch through side[0] alone)
  memcpy(side == 0 ? (void*)&T.cache.ipa_u1 : (void*)&T.cache.ipa_u2, &Ugen, sizeof(Ugen));
  SideDev& S = T.cache.side[side];
  const size_t stride = 16 + 4 * (size_t)(1 + n_pub);
  // a test's multipliers: two an instance (its W opening, its E opening) -> the batch's six a proof
  std::vector<uint64_t> given;
  if (multipliers) {
    given.assign(2 * BATCH_MAX_OPENINGS * n, 1);
    for (size_t i = 0; i < n; i++) memcpy(&given[2 * BATCH_MAX_OPENINGS * i], multipliers + 4 * i, 32);
  }
  BatchProbe probe;
  if (side == 0) probe.acc[0] = acc_out; else probe.acc[1] = acc_out;
  auto run = [&](auto& vf, size_t i, uint32_t* res) {
    return test_instance_word<F, C>(vf, ctx, T, S, H, ck, Ugen, dg[0], side_tag, label, inst + stride * i, n_pub, has_E[i], words[i], n_words[i], res);
  };
  return compressed_batch("vimz_test_spartan_instance_batch", ctx, &T.cache, ck, ck, n, chunk, multipliers ? given.data() : nullptr,
                          [&](size_t i, DeferredVerify& vf, uint32_t* res) { return run(vf, i, res); },
                          [&](size_t i, uint32_t* res) { SingleVerify vf; return run(vf, i, res); }, results, seconds, acc_out ? &probe : nullptr, flags, leaf, stats);
}

}  // namespace

extern "C" {

int vimz_test_spartan_batch_group(void) { return (int)BATCH_GROUP; }
int vimz_test_spartan_batch_split(void) { return (int)BATCH_SPLIT_H; }

int vimz_test_spartan_mat_eval(vimz_ctx* ctx, int curve, size_t n_c, size_t n_w, const vimz_coo* A, const vimz_coo* B, const vimz_coo* C, size_t n, const uint64_t* rx,
                               const uint64_t* ry, const uint64_t* w, uint64_t* out) {
  if (!ctx || !A || !B || !C || !n || !rx || !ry || !w || !out || (curve != VIMZ_CURVE_BN254_G1 && curve != VIMZ_CURVE_GRUMPKIN) || n_c < 2 || n_w < 2 ||
      n_c > ((size_t)1 << 21) || n_w > ((size_t)1 << 21) || n > 4096)
    return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_mat_eval: bad argument");
  vimz_r1cs* R = nullptr;
  int rc = vimz_r1cs_upload(ctx, curve == VIMZ_CURVE_BN254_G1 ? VIMZ_FIELD_BN254_FR : VIMZ_FIELD_BN254_FQ, n_c, n_w, A, B, C, VIMZ_FORM_CANONICAL, &R);
  if (rc) return rc;
  try { rc = curve == VIMZ_CURVE_BN254_G1 ? test_mat_eval<Fe>(ctx, R, n, rx, ry, w, out) : test_mat_eval<Fq>(ctx, R, n, rx, ry, w, out); }
  catch (const std::exception& e) { rc = vz_fail(ctx, VIMZ_ERR_INVALID, e.what()); }
  vimz_r1cs_free(ctx, R);
  return rc;
}

int vimz_test_spartan_svec_accum(vimz_ctx* ctx, int field, uint32_t rounds, size_t n, const uint64_t* xs, const uint64_t* points, const uint64_t* coefs, const uint32_t* shifted,
                                 const uint32_t* n_pub, const uint32_t* n_w, uint64_t* acc_out, uint64_t* dots_out) {
  if (!ctx || !n || n > 4096 || !xs || !points || !coefs || !shifted || !n_pub || !n_w || !acc_out || !dots_out || rounds < 1 || rounds > 21)
    return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_svec_accum: bad argument");
  const int rc = scalar_field_dispatch(field, [&](auto f) { typedef decltype(f) F; return test_svec_accum<F>(ctx, rounds, n, xs, points, coefs, shifted, n_pub, n_w, acc_out, dots_out); });
  return rc == VIMZ_ERR_INVALID && field != VIMZ_FIELD_BN254_FR && field != VIMZ_FIELD_BN254_FQ ? vz_fail(ctx, rc, "vimz_test_spartan_svec_accum: bad argument") : rc;
}

int vimz_test_spartan_instance_batch(vimz_ctx* ctx, int curve, size_t n_c, size_t n_w, uint32_t n_pub, const vimz_coo* A, const vimz_coo* B, const vimz_coo* C,
                                     const vimz_bases* ck, const uint64_t digest[4], uint32_t side_tag, const char* label, size_t n, const uint64_t* inst, const int* has_E,
                                     const uint64_t* const* words, const size_t* n_words, size_t chunk, const uint64_t* multipliers, uint32_t* results, double seconds[6],
                                     uint64_t* acc_out) {
  return vimz_test_spartan_instance_batch_ex(ctx, curve, n_c, n_w, n_pub, A, B, C, ck, digest, side_tag, label, n, inst, has_E, words, n_words, chunk, multipliers, results, seconds,
                                             acc_out, 0, 0, nullptr);
}
int vimz_test_spartan_instance_batch_ex(vimz_ctx* ctx, int curve, size_t n_c, size_t n_w, uint32_t n_pub, const vimz_coo* A, const vimz_coo* B, const vimz_coo* C,
                                        const vimz_bases* ck, const uint64_t digest[4], uint32_t side_tag, const char* label, size_t n, const uint64_t* inst, const int* has_E,
                                        const uint64_t* const* words, const size_t* n_words, size_t chunk, const uint64_t* multipliers, uint32_t* results, double seconds[6],
                                        uint64_t* acc_out, uint32_t flags, size_t leaf, uint64_t stats[4]) {
  if (!ctx || !A || !B || !C || !ck || !digest || !label || (n && (!inst || !has_E || !words || !n_words || !results)))
    return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_instance_batch: bad argument");
  for (size_t i = 0; i < n; i++) if (!words[i] && n_words[i]) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_instance_batch: bad argument");
  return (int)instance_dispatch(ctx, curve, n_c, n_w, n_pub, A, B, C, ck, "vimz_test_spartan_instance_batch: bad argument", [&](const vimz_r1cs* R) -> int64_t {
    return curve == VIMZ_CURVE_BN254_G1
             ? test_instance_batch<Fe, BnG1>(ctx, curve, R, ck, digest, side_tag, label, n_pub, n, inst, has_E, words, n_words, chunk, multipliers, results, seconds, acc_out, flags, leaf, stats)
             : test_instance_batch<Fq, Grumpkin>(ctx, curve, R, ck, digest, side_tag, label, n_pub, n, inst, has_E, words, n_words, chunk, multipliers, results, seconds, acc_out, flags, leaf, stats);
  });
}

int vimz_testing_ivc_verify_compressed_batch_scalars(vimz_ivc* vk, size_t n, const uint8_t* const* blobs, const size_t* lens, const uint64_t* steps, const uint64_t* z0,
                                                     size_t chunk, const uint64_t* multipliers, uint32_t* results, double seconds[6]) {
  return vimz_testing_ivc_verify_batch_compressed_scalars_ex(vk, n, blobs, lens, steps, z0, chunk, multipliers, results, seconds, 0, 0, nullptr);
}
int vimz_testing_ivc_verify_batch_compressed_scalars_ex(vimz_ivc* vk, size_t n, const uint8_t* const* blobs, const size_t* lens, const uint64_t* steps, const uint64_t* z0,
                                                        size_t chunk, const uint64_t* multipliers, uint32_t* results, double seconds[6], uint32_t flags, size_t leaf,
                                                        uint64_t stats[4]) {
  if (n && !multipliers) return vz_fail(vk ? vk->ctx : nullptr, VIMZ_ERR_INVALID, "vimz_testing_ivc_verify_compressed_batch_scalars: NULL multipliers");
  return ivc_compressed_batch("vimz_testing_ivc_verify_compressed_batch_scalars", vk, n, blobs, lens, steps, z0, chunk, multipliers, results, seconds, nullptr, flags, leaf, stats);
}
int vimz_testing_cf_verify_compressed_batch_scalars(vimz_cf* vk, size_t n, const uint8_t* const* blobs, const size_t* lens, const uint64_t* steps, const uint64_t* z0,
                                                    size_t chunk, const uint64_t* multipliers, uint32_t* results, double seconds[6]) {
  return vimz_testing_cf_verify_batch_compressed_scalars_ex(vk, n, blobs, lens, steps, z0, chunk, multipliers, results, seconds, 0, 0, nullptr);
}
int vimz_testing_cf_verify_batch_compressed_scalars_ex(vimz_cf* vk, size_t n, const uint8_t* const* blobs, const size_t* lens, const uint64_t* steps, const uint64_t* z0,
                                                       size_t chunk, const uint64_t* multipliers, uint32_t* results, double seconds[6], uint32_t flags, size_t leaf,
                                                       uint64_t stats[4]) {
  if (n && !multipliers) return vz_fail(vk ? vk->ctx : nullptr, VIMZ_ERR_INVALID, "vimz_testing_cf_verify_compressed_batch_scalars: NULL multipliers");
  return cf_compressed_batch("vimz_testing_cf_verify_compressed_batch_scalars", vk, n, blobs, lens, steps, z0, chunk, multipliers, results, seconds, nullptr, flags, leaf, stats);
}

int vimz_test_spartan_eq(vimz_ctx* ctx, int field, const uint64_t* point, size_t k, uint64_t* table_out) {
  if (!ctx || !point || !table_out || k < 1 || k > 21) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_eq: bad argument");
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  const int rc = scalar_field_dispatch(field, [&](auto f) { typedef decltype(f) F; return test_eq<F>(ctx, point, k, table_out); });
  return rc == VIMZ_ERR_INVALID ? vz_fail(ctx, rc, "vimz_test_spartan_eq: bad argument") : rc;
}

int vimz_test_spartan_sumcheck(vimz_ctx* ctx, int field, int kind, size_t k, const uint64_t* const vecs[5], const uint64_t u[4], const uint64_t* challenges,
                               uint64_t* msgs_out, uint64_t* finals_out) {
  if (!ctx || !vecs || !challenges || !msgs_out || !finals_out || k < 1 || k > 21 || kind < 0 || kind > 1) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_sumcheck: bad argument");
  for (int q = 0; q < (kind == 0 ? 4 : 2); q++) if (!vecs[q]) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_sumcheck: NULL vector");
  if (kind == 0 && !u) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_sumcheck: the outer check needs u");
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  const int rc = scalar_field_dispatch(field, [&](auto f) { typedef decltype(f) F; return test_sumcheck<F>(ctx, kind, k, vecs, u, challenges, msgs_out, finals_out); });
  return rc == VIMZ_ERR_INVALID ? vz_fail(ctx, rc, "vimz_test_spartan_sumcheck: bad argument") : rc;
}

int vimz_test_spartan_ipa_vec(vimz_ctx* ctx, int field, size_t k, const uint64_t* a, const uint64_t* b, const uint64_t* challenges, uint64_t* dots_out, uint64_t finals_out[8]) {
  if (!ctx || !a || !b || !challenges || !dots_out || !finals_out || k < 1 || k > 21) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_ipa_vec: bad argument");
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  const int rc = scalar_field_dispatch(field, [&](auto f) { typedef decltype(f) F; return test_ipa_vec<F>(ctx, k, a, b, challenges, dots_out, finals_out); });
  return rc == VIMZ_ERR_INVALID ? vz_fail(ctx, rc, "vimz_test_spartan_ipa_vec: bad argument") : rc;
}

int vimz_test_spartan_fold_bases(vimz_ctx* ctx, int curve, const uint64_t* points_xy, size_t half, const uint64_t x128[2], uint64_t* out_xy) {
  if (!ctx || !points_xy || !x128 || !out_xy || half < 1 || half > ((size_t)1 << 20) || (curve != VIMZ_CURVE_BN254_G1 && curve != VIMZ_CURVE_GRUMPKIN))
    return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_fold_bases: bad argument");
  std::lock_guard<std::mutex> g(ctx->mu);
  P_TRY(hipSetDevice(ctx->device));
  return curve == VIMZ_CURVE_BN254_G1 ? test_fold_bases<BnG1>(ctx, points_xy, half, x128, out_xy) : test_fold_bases<Grumpkin>(ctx, points_xy, half, x128, out_xy);
}

int64_t vimz_test_spartan_instance(vimz_ctx* ctx, int curve, size_t n_c, size_t n_w, const vimz_coo* A, const vimz_coo* B, const vimz_coo* C, const uint64_t* Z,
                                   const uint64_t* E, const vimz_bases* ck, const uint64_t digest[4], uint32_t side_tag, const char* label, void* buf, size_t cap) {
  if (!ctx || !A || !B || !C || !Z || !ck || !digest || !label) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_instance: bad argument");
  return vimz_test_spartan_instance_pub(ctx, curve, n_c, n_w, 2, A, B, C, Z, E, ck, digest, side_tag, label, buf, cap);
}

int64_t vimz_test_spartan_instance_pub(vimz_ctx* ctx, int curve, size_t n_c, size_t n_w, uint32_t n_pub, const vimz_coo* A, const vimz_coo* B, const vimz_coo* C,
                                       const uint64_t* Z, const uint64_t* E, const vimz_bases* ck, const uint64_t digest[4], uint32_t side_tag, const char* label, void* buf,
                                       size_t cap) {
  if (!ctx || !A || !B || !C || !Z || !ck || !digest || !label) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_instance: bad argument");
  return instance_dispatch(ctx, curve, n_c, n_w, n_pub, A, B, C, ck, "vimz_test_spartan_instance: bad argument", [&](const vimz_r1cs* R) -> int64_t {
    return curve == VIMZ_CURVE_BN254_G1 ? test_instance<Fe, BnG1>(ctx, curve, R, Z, E, ck, digest, side_tag, label, n_pub, buf, cap)
                                        : test_instance<Fq, Grumpkin>(ctx, curve, R, Z, E, ck, digest, side_tag, label, n_pub, buf, cap);
  });
}

int vimz_test_spartan_instance_verify(vimz_ctx* ctx, int curve, size_t n_c, size_t n_w, const vimz_coo* A, const vimz_coo* B, const vimz_coo* C, const vimz_bases* ck,
                                      const uint64_t digest[4], uint32_t side_tag, const char* label, const uint64_t inst[28], int has_E, const uint64_t* words,
                                      size_t n_words) {
  if (!ctx || !A || !B || !C || !ck || !digest || !label || !inst || (!words && n_words)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_instance_verify: bad argument");
  return vimz_test_spartan_instance_pub_verify(ctx, curve, n_c, n_w, 2, A, B, C, ck, digest, side_tag, label, inst, has_E, words, n_words);
}

int vimz_test_spartan_instance_pub_verify(vimz_ctx* ctx, int curve, size_t n_c, size_t n_w, uint32_t n_pub, const vimz_coo* A, const vimz_coo* B, const vimz_coo* C,
                                          const vimz_bases* ck, const uint64_t digest[4], uint32_t side_tag, const char* label, const uint64_t* inst, int has_E,
                                          const uint64_t* words, size_t n_words) {
  if (!ctx || !A || !B || !C || !ck || !digest || !label || !inst || (!words && n_words)) return vz_fail(ctx, VIMZ_ERR_INVALID, "vimz_test_spartan_instance_verify: bad argument");
  return (int)instance_dispatch(ctx, curve, n_c, n_w, n_pub, A, B, C, ck, "vimz_test_spartan_instance_verify: bad argument", [&](const vimz_r1cs* R) -> int64_t {
    return curve == VIMZ_CURVE_BN254_G1 ? test_instance_verify<Fe, BnG1>(ctx, curve, R, ck, digest, side_tag, label, inst, n_pub, has_E, words, n_words)
                                        : test_instance_verify<Fq, Grumpkin>(ctx, curve, R, ck, digest, side_tag, label, inst, n_pub, has_E, words, n_words);
  });
}

}  // extern "C"
#endif  // VIMZ_TESTING
