// Many compressed proofs in one call (vimz_ivc_verify_compressed_batch, vimz_cf_verify_compressed_batch).  Part of spartan.hip's translation unit: included
// after spartan_verify / ipa_verify, whose twins live here.
//
// THE DEFERRED VERIFIER.  spartan_verify_deferred replays an argument's transcript and makes every scalar check spartan_verify makes at O(log n) cost on the
// host (the two sum-check chains, the cl[3] == 0 rule of a strict instance, the outer claim; the eq(ry, ·) values of Z(ry) by the product formula), and leaves
//   vm = Σ_m w_m Σ_nonzeros dict[coef]·eq(rx, row)·eq(ry, col)      to k_mat_eval  (the inner claim vm·vz == claim is judged when vm comes back),
//   bfin = <s, b> of every opening                                  to k_svec_accum,
// and does NO group work: ipa_verify's update P <- R + x·P + x²·L unrolls to
//   P_fin = (Π_j x_j)·P_0 + Σ_j (Π_{i>j} x_i)·(R_j + x_j²·L_j),   P_0 = comm + claim·r0·Ugen,
// so the opening's equation P_fin = afin·<s, G> + afin·bfin·r0·Ugen is LINEAR in the 2·rounds + 1 points the proof brings, Ugen and the key's points:
//   Σ_k c_k·Q_k + g·Ugen − afin·<s, G> = O,   c(comm) = Π x,  c(R_j) = Π_{i>j} x_i,  c(L_j) = x_j²·Π_{i>j} x_i,  g = (Π x)·claim·r0 − afin·bfin·r0.
//
// THE BATCH EQUATION.  Every opening o gets a non-zero 128-bit multiplier ρ_o from the OS.  Per curve a chunk is accepted iff
//   Σ_o ρ_o·[Σ_k c_{o,k}·Q_{o,k}] + (Σ_o ρ_o·g_o)·Ugen = <acc, ck>,   acc[j] = Σ_o ρ_o·afin_o·s_o[i],  j = i for an E opening, j = (i − 1) mod n for a W opening
// (load_bases(shifted): slot 0 of a W opening is ck[n − 1], slot i is ck[i − 1]) — one MSM over the key and one over the chunk's own points per curve, both by
// msm_run.  A failing opening survives with probability about 2^-128.  An accepted chunk adds no argument bits.  Every proof whose deferred pass fails anywhere
// inside an argument goes to the single verifier (so the bits are the single verifier's, with no second implementation of them).
//
// A REFUSED CHUNK IS BISECTED (batch_bisect.hpp).  What a proof costs — the parse, the transcript replay, k_mat_eval, the DefArg objects — is there already, so
// the equation of a curve is asked again of halves of the chunk: batch_side_equation over the arguments of the members of [lo, hi), every opening under the
// multiplier it had, i.e. k_svec_accum and the two msm_run calls again and nothing else.  A half is asked only on the curves its parent was refused on; a member
// is accepted only inside a subset whose equations were evaluated and held; a refused subset of at most `leaf` members (default 1) goes to the single verifier.
// At most 2·(c − 1) subsets are asked of a refused chunk of c members; one bad proof among 32 costs 5 to 10 subset equations and ONE single verification where
// it cost 32 (profiles/batch_bisect.txt).  VIMZ_BATCH_NO_BISECT sends the refused chunk to the single verifier whole.
//
// Kernels: one thread an element or a row, every thread writes slots it owns, no atomics, no flag another workgroup reads, every loop bound from the host (or the
// uploaded CSR), partials reduced by a second launch.
#pragma once
#include <sys/random.h>
#include <array>
#include <chrono>
#include <functional>
#include <thread>
#include "batch_bisect.hpp"
#include "spartan_batch_plan.hpp"

namespace {

// (spartan_batch_plan.hpp: the GPU-free pieces, with their host check)
constexpr uint32_t BATCH_GROUP = sb::GROUP, BATCH_SPLIT_H = sb::SPLIT_H, BATCH_MAX_VARS = sb::MAX_VARS;
constexpr size_t BATCH_DEFAULT_CHUNK = sb::DEFAULT_CHUNK, BATCH_DEFAULT_LEAF = sb::DEFAULT_LEAF;
constexpr uint32_t BATCH_NO_BISECT = 1;      // flags bit 0 (VIMZ_BATCH_NO_BISECT)

// ---- kernels ---------------------------------------------------------------------------------------------------------------------------------------------
// per member g of a group two points t = 0, 1 of nv[t] variables each (vars[(2g + t)·BATCH_MAX_VARS + q], q = 0 the TOP bit of the index); four tables, member-
// interleaved: tabs[(off[2t + half] + e)·G + g].  kind 1: eq(point, ·);  kind 0: the monomials Π_{bit set} x (the s-vector of an opening).  Bit p of an index
// selects variable nv − 1 − p.  Members g >= n_members get zero tables: they add nothing anywhere.
struct HalfTabs { uint32_t nv[2], kind[2], hl[2], off[4], n_members, total; };
template <class F, int G>
__global__ void __launch_bounds__(256) k_half_tables(HalfTabs a, const uint32_t* __restrict__ vars, uint32_t* __restrict__ tabs) {
  VZ_GRID_STRIDE(id, (size_t)a.total) {
    const uint32_t e = (uint32_t)(id / G), g = (uint32_t)(id % G);
    const uint32_t tt = (e >= a.off[1] ? 1u : 0u) + (e >= a.off[2] ? 1u : 0u) + (e >= a.off[3] ? 1u : 0u);
    const uint32_t t = tt >> 1, hi = tt & 1u, local = e - a.off[tt];
    const size_t base = (size_t)(2 * g + t) * BATCH_MAX_VARS;
    const F x = sb::half_entry<F>([&](uint32_t q) { return load_fe<F>(vars, base + q); }, a.nv[t], a.hl[t], hi != 0, a.kind[t], local);
    store_fe(tabs, (size_t)e * G + g, g < a.n_members ? x : F::zero());
  }
}

// each of the G sums of a workgroup's 256 threads -> partial[blockIdx.x·G + g].  (block_reduce_store<F, G> of spartan.hip has the same layout but stages all G
// sums at once: 32 KB of LDS a workgroup at G = 4 against 8 KB here — k_mat_eval is latency-bound on gathers and lives on resident waves; k_sum_groups is its
// second stage, one workgroup a member, so that it takes any number of first-stage workgroups.)
template <class F, int G>
__device__ __forceinline__ void block_reduce_each(F (&acc)[G], uint32_t* __restrict__ partial) {
  __shared__ uint32_t sh[256 * 8];
  const uint32_t t = threadIdx.x;
#pragma unroll
  for (int g = 0; g < G; g++) {
#pragma unroll
    for (int w = 0; w < 8; w++) sh[t * 8 + w] = acc[g].v[w];
    __syncthreads();
    for (uint32_t d = 128; d > 0; d >>= 1) {
      if (t < d) {
        F x, y;
#pragma unroll
        for (int w = 0; w < 8; w++) { x.v[w] = sh[t * 8 + w]; y.v[w] = sh[(t + d) * 8 + w]; }
        x = F::add(x, y);
#pragma unroll
        for (int w = 0; w < 8; w++) sh[t * 8 + w] = x.v[w];
      }
      __syncthreads();
    }
    if (t == 0) { F x; for (int w = 0; w < 8; w++) x.v[w] = sh[w]; store_fe(partial, (size_t)blockIdx.x * G + g, x); }
    __syncthreads();
  }
}
// out[g] = Σ_blocks partial[b·G + g]: workgroup g of G
template <class F>
__global__ void __launch_bounds__(256) k_sum_groups(const uint32_t* __restrict__ partial, uint32_t nblocks, uint32_t G, uint32_t* __restrict__ out) {
  F acc[1] = {F::zero()};
  for (uint32_t b = threadIdx.x; b < nblocks; b += 256) acc[0] = F::add(acc[0], load_fe<F>(partial, (size_t)b * G + blockIdx.x));
  block_reduce_store<F, 1>(acc, out);
}

// vm_g = Σ_m w[m][g] Σ_rows eq(rx_g, row) Σ_k dict[coef_k]·eq(ry_g, col_k) for the G members of a group in ONE pass over the CSR: a row's columns and
// coefficients are read once and serve every member; eq(·) = lo[idx & mask]·hi[idx >> h] from the member-interleaved half-tables (G elements side by side: one
// 128-byte line a gather at G = 4; 48 KB a member at 2^19, resident in L2).  One thread a (matrix, row), matrix-major as k_spmv3; rows of any length (the
// 240-term rows of a bit decomposition are a few hundred among 1.5 M: the pass ends when its longest row does, about as k_spmv3's would without its item list —
// SideDev carries that list for the secondary side only).
struct MatTabs { uint32_t xlo, xhi, ylo, yhi, hx, hy; };
template <class F, int G>
__global__ void __launch_bounds__(256) k_mat_eval(CsrDev A, CsrDev B, CsrDev C, const uint32_t* __restrict__ dict, size_t nrows, MatTabs T, const uint32_t* __restrict__ tabs,
                                                  const uint32_t* __restrict__ w, uint32_t* __restrict__ partial) {
  F tot[G];
#pragma unroll
  for (int g = 0; g < G; g++) tot[g] = F::zero();
  const uint32_t mx = (1u << T.hx) - 1u, my = (1u << T.hy) - 1u;
  VZ_GRID_STRIDE(i, 3 * nrows) {
    const uint32_t m = (uint32_t)(i / nrows);
    const size_t r = i - (size_t)m * nrows;
    const CsrDev M = m == 0 ? A : (m == 1 ? B : C);
    const uint32_t lo = M.row_ptr[r], hi = M.row_ptr[r + 1];
    if (hi == lo) continue;
    F row[G];
#pragma unroll
    for (int g = 0; g < G; g++) row[g] = F::zero();
    for (uint32_t k = lo; k < hi; k++) {
      const uint32_t col = M.col[k];
      const F d = load_fe<F>(dict, 2 * (size_t)M.coef[k]);
      const size_t ylo = (size_t)(T.ylo + (col & my)) * G, yhi = (size_t)(T.yhi + (col >> T.hy)) * G;
#pragma unroll
      for (int g = 0; g < G; g++) row[g] = F::add(row[g], F::mul(d, F::mul(load_fe<F>(tabs, ylo + g), load_fe<F>(tabs, yhi + g))));
    }
    const size_t xlo = (size_t)(T.xlo + ((uint32_t)r & mx)) * G, xhi = (size_t)(T.xhi + ((uint32_t)r >> T.hx)) * G;
#pragma unroll
    for (int g = 0; g < G; g++) {
      const F x = F::mul(load_fe<F>(tabs, xlo + g), load_fe<F>(tabs, xhi + g));
      tot[g] = F::add(tot[g], F::mul(load_fe<F>(w, (size_t)m * G + g), F::mul(x, row[g])));
    }
  }
  block_reduce_each<F, G>(tot, partial);
}

// A group of G openings of one (curve, rounds), n = 2^rounds.  The thread of accumulator slot j takes, of member g, index i = j (an E opening) or (j + 1) mod n (a W
// opening: slot j is ck[j], which load_bases(shifted) puts at index j + 1, ck[n − 1] at index 0):  acc[j] += Σ_g coef_g·s_g[i],  s_g[i] = lo_g[i & mask]·hi_g[i >> h],
// and dot_g += s_g[i]·b_g[i] with b_g = eq(point_g, ·) from its own half-tables, zero where n_w != 0 and (i == 0 || i + n_pub >= n_w) — k_mask_public's rule.
// (Consecutive threads read consecutive lo entries and one hi entry a workgroup: coalesced as they stand, so the tables stay in L2 and no LDS copy is made.)
template <int G> struct SvecArgs { uint32_t rounds, hl, slo, shi, blo, bhi; uint32_t shifted[G], n_pub[G], n_w[G]; };
template <class F, int G>
__global__ void __launch_bounds__(256) k_svec_accum(SvecArgs<G> a, const uint32_t* __restrict__ tabs, const uint32_t* __restrict__ coef, uint32_t* __restrict__ acc,
                                                    uint32_t* __restrict__ partial) {
  const size_t n = (size_t)1 << a.rounds;
  const uint32_t mask = (1u << a.hl) - 1u;
  F dot[G], cf[G];
#pragma unroll
  for (int g = 0; g < G; g++) { dot[g] = F::zero(); cf[g] = load_fe<F>(coef, g); }
  VZ_GRID_STRIDE(j, n) {
    F sum = load_fe<F>(acc, j);
#pragma unroll
    for (int g = 0; g < G; g++) {
      const size_t i = sb::svec_index(j, n, a.shifted[g] != 0);
      const size_t lo = (size_t)((uint32_t)i & mask) * G + g, hi = (size_t)(i >> a.hl) * G + g;
      const F s = F::mul(load_fe<F>(tabs, (size_t)a.slo * G + lo), load_fe<F>(tabs, (size_t)a.shi * G + hi));
      sum = F::add(sum, F::mul(cf[g], s));
      const bool masked = sb::svec_masked(i, a.n_pub[g], a.n_w[g]);
      const F b = F::mul(load_fe<F>(tabs, (size_t)a.blo * G + lo), load_fe<F>(tabs, (size_t)a.bhi * G + hi));
      if (!masked) dot[g] = F::add(dot[g], F::mul(s, b));
    }
    store_fe(acc, j, sum);
  }
  block_reduce_each<F, G>(dot, partial);
}

// ---- what a deferred argument leaves behind ------------------------------------------------------------------------------------------------------------------
template <class F, class FS>
struct DefOpening {
  bool shifted = false; uint32_t rounds = 0, n_pub = 0, n_w = 0;      // n_w = 0: no mask (an E opening)
  std::vector<F> xs, pt;                                              // the challenges, round 0 (the top bit) first; b = eq(pt, ·)
  F afin, r0, g0;                                                     // the coefficient on Ugen is g0 − afin·bfin·r0
  std::vector<Affine<FS>> Q; std::vector<F> c;                        // comm, R_0, L_0, R_1, L_1, ... and their coefficients
};
template <class F, class FS>
struct DefArg { std::vector<F> rx, ry; F w[3]; F claim, vz; uint32_t n_open = 0; DefOpening<F, FS> op[2]; };

template <class F>
F eq_at(const std::vector<F>& pt, size_t idx) {          // eq(pt, idx), pt[0] = the top bit: the product formula, no table
  F acc = F::one();
  const size_t k = pt.size();
  for (size_t q = 0; q < k; q++) { const bool bit = (idx >> (k - 1 - q)) & 1; acc = F::mul(acc, bit ? pt[q] : F::sub(F::one(), pt[q])); }
  return acc;
}

// ipa_verify's transcript and reads; the group equation as coefficients
template <class F, class FS>
bool ipa_deferred(Transcript& tr, bool shifted, const std::vector<F>& pt, uint32_t n_pub, uint32_t n_w, uint32_t rounds, const Affine<FS>& comm, const F& claim, Reader& in,
                  DefOpening<F, FS>& O) {
  tr.absorb_fe("ipaP.x", comm.x); tr.absorb_fe("ipaP.y", comm.y); tr.absorb_fe("ipaC", claim);
  uint32_t r0[4]; tr.challenge(r0);
  { F c = F::zero(); for (int k = 0; k < 4; k++) c.v[k] = r0[k]; O.r0 = F::to_mont(c); }
  O.shifted = shifted; O.rounds = rounds; O.n_pub = n_pub; O.n_w = n_w; O.pt = pt;
  O.xs.resize(rounds);
  std::vector<Affine<FS>> Ls(rounds), Rs(rounds);
  for (uint32_t j = 0; j < rounds; j++) {
    Ls[j] = in.point<FS>(); Rs[j] = in.point<FS>();
    if (!in.ok) return false;
    tr.absorb_fe("L.x", Ls[j].x); tr.absorb_fe("L.y", Ls[j].y); tr.absorb_fe("R.x", Rs[j].x); tr.absorb_fe("R.y", Rs[j].y);
    uint32_t xw[4]; tr.challenge(xw);
    F xc = F::zero(); for (int k = 0; k < 4; k++) xc.v[k] = xw[k];
    O.xs[j] = F::to_mont(xc);
  }
  O.afin = in.fe<F>();
  if (!in.ok) return false;
  tr.absorb_fe("a", O.afin);
  O.Q.assign(2 * (size_t)rounds + 1, comm);
  for (uint32_t j = 0; j < rounds; j++) { O.Q[1 + 2 * j] = Rs[j]; O.Q[2 + 2 * j] = Ls[j]; }
  sb::ipa_unroll<F>(O.xs, claim, O.r0, O.c, &O.g0);
  return true;
}

// spartan_verify without its device and group work: false = a check the single verifier makes on the host has failed (or the words ran out)
template <class F, class C>
bool spartan_verify_deferred(const SideDev& S, const F& digest, const Instance<F, typename C::Base>& I, uint32_t side_tag, Transcript& tr, Reader& in,
                             DefArg<F, typename C::Base>& D) {
  typedef typename C::Base FS;
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
  F vz = F::add(evalW, F::mul(I.u, eq_at(ry, 0)));
  for (uint32_t k = 0; k < I.n_pub; k++) vz = F::add(vz, F::mul(I.X[k], eq_at(ry, (size_t)S.n_w - I.n_pub + k)));
  D.rx = rx; D.ry = ry; D.w[0] = F::one(); D.w[1] = rho; D.w[2] = rho2; D.claim = claim; D.vz = vz;      // vm·vz == claim: judged when k_mat_eval's vm is back
  D.n_open = 0;
  if (!ipa_deferred<F, FS>(tr, true, ry, I.n_pub, S.n_w, S.t, I.cW, evalW, in, D.op[0])) return false;
  D.n_open = 1;
  if (I.has_E) {
    if (!ipa_deferred<F, FS>(tr, false, rx, 0, 0, S.s, I.cE, cl[3], in, D.op[1])) return false;
    D.n_open = 2;
  }
  return true;
}

// ---- the device side of a batch ------------------------------------------------------------------------------------------------------------------------------
// first-stage workgroups of k_mat_eval: one thread a (matrix, row) up to this many workgroups (8 a CU on 256 CUs: the kernel waits on gathers, so it wants every
// wave slot a SIMD has), grid-stride beyond; RED_BLOCKS (512) stays the cap of k_svec_accum, which streams
constexpr unsigned MAT_BLOCKS = 2048;
inline unsigned mat_grid(size_t items) { return (unsigned)std::max<size_t>(1, std::min<size_t>(MAT_BLOCKS, (items + 255) / 256)); }

struct BatchDev {          // scratch of one call (a few MB whatever n is; the accumulator is the side's own vm vector)
  uint32_t *tabs = nullptr, *vars = nullptr, *small = nullptr /* w (3G) | coef (G) | out (G) */, *partial = nullptr;
  uint32_t *pts_raw = nullptr, *pts = nullptr, *scal = nullptr; size_t cap_pts = 0;
  static constexpr size_t TAB_ELEMS = 4 * ((size_t)1 << 11) * BATCH_GROUP;          // four half-tables of at most 2^max(H, 21 − H) entries a member
  hipError_t alloc() {
    hipError_t e;
    if ((e = hipMalloc((void**)&tabs, 32 * TAB_ELEMS)) != hipSuccess) return e;
    if ((e = hipMalloc((void**)&vars, 32 * 2 * (size_t)BATCH_MAX_VARS * BATCH_GROUP)) != hipSuccess) return e;
    if ((e = hipMalloc((void**)&small, 32 * 5 * (size_t)BATCH_GROUP)) != hipSuccess) return e;
    return hipMalloc((void**)&partial, 32 * (size_t)BATCH_GROUP * (MAT_BLOCKS + 1));
  }
  void release() { hipFree(tabs); hipFree(vars); hipFree(small); hipFree(partial); hipFree(pts_raw); hipFree(pts); hipFree(scal); tabs = vars = small = partial = pts_raw = pts = scal = nullptr; cap_pts = 0; }
  hipError_t reserve_points(size_t n) {
    if (n <= cap_pts) return hipSuccess;
    hipFree(pts_raw); hipFree(pts); hipFree(scal); pts_raw = pts = scal = nullptr; cap_pts = 0;
    hipError_t e;
    if ((e = hipMalloc((void**)&pts_raw, 64 * n)) != hipSuccess) return e;
    if ((e = hipMalloc((void**)&pts, 4 * (size_t)AFFINE_WORDS * n)) != hipSuccess) return e;
    if ((e = hipMalloc((void**)&scal, 32 * n)) != hipSuccess) return e;
    cap_pts = n;
    return hipSuccess;
  }
  uint32_t* w() const { return small; }
  uint32_t* coef() const { return small + 8 * 3 * BATCH_GROUP; }
  uint32_t* out() const { return small + 8 * 4 * BATCH_GROUP; }
  ~BatchDev() { release(); }
};

inline double batch_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

// the four half-tables of up to G members with points p0[g] (kind k0) and p1[g] (kind k1); both points of a member have nv0 / nv1 variables
template <class F>
hipError_t batch_half_tables(hipStream_t s, BatchDev& D, uint32_t members, const std::vector<F>* const* p0, uint32_t nv0, uint32_t k0, const std::vector<F>* const* p1,
                             uint32_t nv1, uint32_t k1, HalfTabs* out, std::vector<F>& stage) {
  constexpr uint32_t G = BATCH_GROUP;
  if (members < 1 || members > G || nv0 < 1 || nv1 < 1 || nv0 > BATCH_MAX_VARS || nv1 > BATCH_MAX_VARS) return hipErrorInvalidValue;
  HalfTabs a{};
  a.nv[0] = nv0; a.nv[1] = nv1; a.kind[0] = k0; a.kind[1] = k1;
  const sb::HalfLayout L = sb::half_layout(nv0, nv1);
  for (int k = 0; k < 2; k++) a.hl[k] = L.hl[k];
  for (int k = 0; k < 4; k++) a.off[k] = L.off[k];
  const size_t elems = L.elems;
  if (elems * G > BatchDev::TAB_ELEMS) return hipErrorInvalidValue;
  a.n_members = members; a.total = (uint32_t)(elems * G);
  stage.assign(2 * (size_t)BATCH_MAX_VARS * G, F::zero());
  for (uint32_t g = 0; g < members; g++) {
    if (p0[g]->size() != nv0 || p1[g]->size() != nv1) return hipErrorInvalidValue;
    std::copy(p0[g]->begin(), p0[g]->end(), stage.begin() + (size_t)(2 * g) * BATCH_MAX_VARS);
    std::copy(p1[g]->begin(), p1[g]->end(), stage.begin() + (size_t)(2 * g + 1) * BATCH_MAX_VARS);
  }
  hipError_t e;
  if ((e = hipMemcpyAsync(D.vars, stage.data(), 32 * stage.size(), hipMemcpyHostToDevice, s)) != hipSuccess) return e;
  hipLaunchKernelGGL((k_half_tables<F, (int)G>), dim3(stream_grid(a.total)), dim3(256), 0, s, a, (const uint32_t*)D.vars, D.tabs);
  *out = a;
  return hipGetLastError();
}

// vm of every (rx, ry, w) over one side's shape, BATCH_GROUP at a time.  sec (optional): [0] += tables, [1] += the passes
template <class F>
hipError_t batch_mat_eval(hipStream_t s, const SideDev& S, BatchDev& D, const std::vector<const std::vector<F>*>& rx, const std::vector<const std::vector<F>*>& ry,
                          const std::vector<const F*>& w, std::vector<F>& vm, double* sec) {
  constexpr uint32_t G = BATCH_GROUP;
  vm.assign(rx.size(), F::zero());
  hipError_t e;
  std::vector<F> stage, wst, got(G);
  for (size_t at = 0; at < rx.size(); at += G) {
    const uint32_t members = (uint32_t)std::min<size_t>(G, rx.size() - at);
    auto t0 = std::chrono::steady_clock::now();
    HalfTabs h;
    if ((e = batch_half_tables<F>(s, D, members, rx.data() + at, S.s, 1, ry.data() + at, S.t, 1, &h, stage)) != hipSuccess) return e;
    wst.assign(3 * (size_t)G, F::zero());
    for (uint32_t g = 0; g < members; g++) for (int m = 0; m < 3; m++) wst[(size_t)m * G + g] = w[at + g][m];
    if ((e = hipMemcpyAsync(D.w(), wst.data(), 32 * wst.size(), hipMemcpyHostToDevice, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    if (sec) sec[0] += batch_since(t0);
    t0 = std::chrono::steady_clock::now();
    const MatTabs T{h.off[0], h.off[1], h.off[2], h.off[3], h.hl[0], h.hl[1]};
    const unsigned gb = mat_grid(3 * (size_t)S.n_c);
    hipLaunchKernelGGL((k_mat_eval<F, (int)G>), dim3(gb), dim3(256), 0, s, S.A, S.B, S.C, S.dict, (size_t)S.n_c, T, (const uint32_t*)D.tabs, (const uint32_t*)D.w(), D.partial);
    hipLaunchKernelGGL(k_sum_groups<F>, dim3(G), dim3(256), 0, s, (const uint32_t*)D.partial, gb, G, D.out());
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(got.data(), D.out(), 32 * (size_t)G, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    for (uint32_t g = 0; g < members; g++) vm[at + g] = got[g];
    if (sec) sec[1] += batch_since(t0);
  }
  return hipSuccess;
}

// one opening as k_svec_accum takes it
template <class F>
struct SvecItem { const std::vector<F>* xs; const std::vector<F>* pt; F coef; uint32_t shifted, n_pub, n_w; };

// acc (2^rounds slots of the caller's, NOT cleared here) += Σ coef_o·s_o under the index map; bfin[o] = <s_o, b_o>.  Every item has `rounds` challenges.
template <class F>
hipError_t batch_svec_accum(hipStream_t s, BatchDev& D, uint32_t rounds, const std::vector<SvecItem<F>>& items, uint32_t* acc, std::vector<F>& bfin, double* sec) {
  constexpr uint32_t G = BATCH_GROUP;
  bfin.assign(items.size(), F::zero());
  hipError_t e = hipSuccess;
  std::vector<F> stage, cst(G), got(G);
  for (size_t at = 0; at < items.size() && e == hipSuccess; at += G) {
    const uint32_t members = (uint32_t)std::min<size_t>(G, items.size() - at);
    auto t0 = std::chrono::steady_clock::now();
    const std::vector<F>* p0[G]; const std::vector<F>* p1[G];
    SvecArgs<(int)G> a{};
    for (uint32_t g = 0; g < G; g++) {
      const bool on = g < members;
      cst[g] = on ? items[at + g].coef : F::zero();
      if (on) { p0[g] = items[at + g].xs; p1[g] = items[at + g].pt; a.shifted[g] = items[at + g].shifted; a.n_pub[g] = items[at + g].n_pub; a.n_w[g] = items[at + g].n_w; }
    }
    HalfTabs h;
    if ((e = batch_half_tables<F>(s, D, members, p0, rounds, 0, p1, rounds, 1, &h, stage)) != hipSuccess) break;
    if ((e = hipMemcpyAsync(D.coef(), cst.data(), 32 * (size_t)G, hipMemcpyHostToDevice, s)) != hipSuccess) break;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) break;
    if (sec) sec[0] += batch_since(t0);
    t0 = std::chrono::steady_clock::now();
    a.rounds = rounds; a.hl = h.hl[0]; a.slo = h.off[0]; a.shi = h.off[1]; a.blo = h.off[2]; a.bhi = h.off[3];
    const unsigned gb = red_grid((size_t)1 << rounds);
    hipLaunchKernelGGL((k_svec_accum<F, (int)G>), dim3(gb), dim3(256), 0, s, a, (const uint32_t*)D.tabs, (const uint32_t*)D.coef(), acc, D.partial);
    hipLaunchKernelGGL(k_sum_groups<F>, dim3(G), dim3(256), 0, s, (const uint32_t*)D.partial, gb, G, D.out());
    if ((e = hipGetLastError()) != hipSuccess) break;
    if ((e = hipMemcpyAsync(got.data(), D.out(), 32 * (size_t)G, hipMemcpyDeviceToHost, s)) != hipSuccess) break;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) break;
    for (uint32_t g = 0; g < members; g++) bfin[at + g] = got[g];
    if (sec) sec[1] += batch_since(t0);
  }
  explicit_bzero((void*)cst.data(), sizeof(F) * cst.size());          // (multiplier-derived)
  hipMemsetAsync(D.coef(), 0, 32 * (size_t)G, s);
  return e;
}

inline bool batch_os_random(void* buf, size_t n) {
  uint8_t* p = (uint8_t*)buf;
  while (n) { const ssize_t g = getrandom(p, n < 256 ? n : 256, 0); if (g <= 0) return false; p += g; n -= (size_t)g; }
  return true;
}
inline unsigned batch_threads() { return std::max(1u, std::min(16u, usable_cpus())); }
inline void batch_parallel_for(size_t n, unsigned threads, const std::function<void(size_t, size_t)>& fn) {
  const unsigned TH = (unsigned)std::max<size_t>(1, std::min<size_t>(threads, n));
  std::vector<std::thread> th;
  for (unsigned t = 1; t < TH; t++) th.emplace_back(fn, n * t / TH, n * (t + 1) / TH);
  fn(0, n / TH);
  for (auto& x : th) x.join();
}

// The MSM's workspace after a run over multiplier-derived scalars: the sorted digit entries, the bucket counts and offsets, every partial sum and the pinned
// window sums are overwritten with zeros (the zero-between-launches words — totals, tickets, the small path's counters — are zero already and stay so).
inline void batch_wipe_msm(hipStream_t s, MsmWorkspace& ws) {
  const size_t R = ws.cap_rows;
  if (ws.counts) hipMemsetAsync(ws.counts, 0, 4 * R * ws.cap_nb, s);
  if (ws.cursor) hipMemsetAsync(ws.cursor, 0, 4 * R * ws.cap_nb, s);
  if (ws.bucket_off) hipMemsetAsync(ws.bucket_off, 0, 4 * R * (ws.cap_nb + 1), s);
  if (ws.sub_off) hipMemsetAsync(ws.sub_off, 0, 4 * R * (ws.cap_nb + 1), s);
  if (ws.sorted) hipMemsetAsync(ws.sorted, 0, 4 * R * ws.cap_entries, s);
  if (ws.partial) hipMemsetAsync(ws.partial, 0, 4 * (size_t)XYZZ_WORDS * R * ws.cap_subs, s);
  if (ws.block_hist) hipMemsetAsync(ws.block_hist, 0, 4 * R * ws.cap_block_hist, s);
  if (ws.heavy_scratch) hipMemsetAsync(ws.heavy_scratch, 0, 4 * R * MsmWorkspace::HEAVY_SCRATCH_WORDS, s);
  if (ws.plane_scratch) hipMemsetAsync(ws.plane_scratch, 0, 4 * (size_t)XYZZ_WORDS * 256, s);
  if (ws.ones_partial) hipMemsetAsync(ws.ones_partial, 0, 4 * (size_t)XYZZ_WORDS * (16384 + 64 + 512), s);
  if (ws.small_buf) hipMemsetAsync((uint8_t*)ws.small_buf + 512, 0, 4 * (size_t)XYZZ_WORDS * MSM_MAX_WINDOWS * SMALL_MAXQ * (1u << (SMALL_C - 1)), s);
  hipStreamSynchronize(s);
  if (ws.host_pinned) explicit_bzero(ws.host_pinned, 4 * (size_t)XYZZ_WORDS * MSM_MAX_WINDOWS);
}

// The batch equation of one side of a chunk.  args: the chunk's arguments on this side, every one with vm·vz == claim already judged good; rho: 2 words an
// opening in the order (argument, W then E), all non-zero.  *holds: the equation's verdict.  probe_acc (a test's, optional): the accumulator, `big` canonical elements.
template <class F, class C>
hipError_t batch_side_equation(hipStream_t s, SpartanCache& cache, SideDev& S, BatchDev& D, const vimz_bases* ck, const Affine<typename C::Base>& Ugen,
                               const std::vector<const DefArg<F, typename C::Base>*>& args, const uint64_t* rho, bool* holds, double* sec_tab_svec, double* sec_msm,
                               uint64_t* probe_acc) {
  typedef typename C::Base FS;
  *holds = true;
  if (args.empty()) return hipSuccess;
  const size_t big = std::max(S.M, S.N);
  hipError_t e;
  struct Secrets {
    std::vector<F> rho, scal; std::vector<SvecItem<F>> it[2];
    ~Secrets() {
      if (!rho.empty()) explicit_bzero((void*)rho.data(), sizeof(F) * rho.size());
      if (!scal.empty()) explicit_bzero((void*)scal.data(), sizeof(F) * scal.size());
      for (auto& v : it) if (!v.empty()) explicit_bzero((void*)v.data(), sizeof(SvecItem<F>) * v.size());
    }
  } X;
  // every device copy of a multiplier-derived value goes however this function is left: the accumulator, the points' scalars, the MSM's workspace
  struct Wipe {
    hipStream_t s; uint32_t* vm; size_t big; BatchDev& D; MsmWorkspace& ws;
    ~Wipe() {
      hipMemsetAsync(vm, 0, 32 * big, s);
      if (D.scal) hipMemsetAsync(D.scal, 0, 32 * D.cap_pts, s);
      hipMemsetAsync(D.coef(), 0, 32 * (size_t)BATCH_GROUP, s);
      batch_wipe_msm(s, ws);
    }
  } wipe{s, S.vm, big, D, cache.ws};
  // the accumulator: the side's vm vector (nothing else runs on this context while its lock is held)
  if ((e = hipMemsetAsync(S.vm, 0, 32 * big, s)) != hipSuccess) return e;
  std::vector<const DefOpening<F, FS>*> ops[2];          // [0] W openings (rounds t), [1] E openings (rounds s)
  for (const auto* A : args)
    for (uint32_t q = 0; q < A->n_open; q++) {
      const DefOpening<F, FS>& O = A->op[q];
      F r = F::zero(); memcpy(r.v, rho + 2 * X.rho.size(), 16);
      X.rho.push_back(F::to_mont(r));
      const int cls = O.shifted ? 0 : 1;
      ops[cls].push_back(&O);
      X.it[cls].push_back(SvecItem<F>{&O.xs, &O.pt, F::mul(X.rho.back(), O.afin), O.shifted ? 1u : 0u, O.n_pub, O.n_w});
    }
  std::vector<F> bfin[2];
  for (int cls = 0; cls < 2; cls++) {
    if (ops[cls].empty()) continue;
    if ((e = batch_svec_accum<F>(s, D, ops[cls][0]->rounds, X.it[cls], S.vm, bfin[cls], sec_tab_svec)) != hipSuccess) return e;
  }
  auto t0 = std::chrono::steady_clock::now();
  // the chunk's own points under rho·c, and Ugen under Σ rho·g
  std::vector<Affine<FS>> pts;
  F gsum = F::zero();
  {
    size_t at[2] = {0, 0}, o = 0;
    for (const auto* A : args)
      for (uint32_t q = 0; q < A->n_open; q++, o++) {
        const DefOpening<F, FS>& O = A->op[q];
        const int cls = O.shifted ? 0 : 1;
        const F& r = X.rho[o];
        const F g = F::sub(O.g0, F::mul(O.afin, F::mul(bfin[cls][at[cls]++], O.r0)));
        gsum = F::add(gsum, F::mul(r, g));
        for (size_t k = 0; k < O.Q.size(); k++) {
          if (O.Q[k].x.is_zero() && O.Q[k].y.is_zero()) continue;          // the identity adds nothing
          pts.push_back(O.Q[k]); X.scal.push_back(F::mul(r, O.c[k]));
        }
      }
    pts.push_back(Ugen); X.scal.push_back(gsum);
  }
  if ((e = D.reserve_points(pts.size())) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(D.pts_raw, pts.data(), 64 * pts.size(), hipMemcpyHostToDevice, s)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(D.scal, X.scal.data(), 32 * X.scal.size(), hipMemcpyHostToDevice, s)) != hipSuccess) return e;
  launch_points_to_internal<FS>(s, D.pts_raw, 0, D.pts, pts.size());
  if ((e = hipGetLastError()) != hipSuccess) return e;
  Affine<FS> lhs, rhs;
  if ((e = msm_run<C>(s, cache.ws, D.pts, D.scal, pts.size(), 1, 0, &lhs, nullptr, nullptr, 0, nullptr)) != hipSuccess) return e;
  if ((e = msm_run<C>(s, cache.ws, ck->d, S.vm, big, 1, 0, &rhs, nullptr, nullptr, 0, nullptr)) != hipSuccess) return e;
  *holds = lhs.x.eq(rhs.x) && lhs.y.eq(rhs.y);
  if (probe_acc) {
    launch_from_mont<F>(s, S.vm, S.vz, big);
    if ((e = hipMemcpyAsync(probe_acc, S.vz, 32 * big, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    hipMemsetAsync(S.vz, 0, 32 * big, s);
  }
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
  if (sec_msm) *sec_msm += batch_since(t0);
  return hipSuccess;
}

// ---- the policies behind the verifier entries' templates ------------------------------------------------------------------------------------------------------
// DeferredVerify stands where SingleVerify (spartan.hip) stands in the four verifiers' bodies: every statement, hash and record check runs as it does for one
// proof; an argument is replayed on the host and kept.
struct DeferredVerify {
  struct Lock { explicit Lock(std::mutex&) {} };
  static constexpr bool on_device = false;
  std::vector<DefArg<Fe, Fq>> a1; std::vector<DefArg<Fq, Fe>> a2;
  uint32_t calls = 0; bool failed = false;
  std::vector<DefArg<Fe, Fq>>& list(const Fe*) { return a1; }
  std::vector<DefArg<Fq, Fe>>& list(const Fq*) { return a2; }
  template <class F, class C, class B>
  bool arg(vimz_ctx*, SpartanCache&, SideDev& S, hipStream_t, const vimz_bases*, const Affine<typename C::Base>&, const F& digest, const Instance<F, typename C::Base>& I,
           const B&, uint32_t side_tag, Transcript& tr, Reader& in) {
    calls++;
    auto& L = list((const F*)nullptr);
    L.emplace_back();
    const bool ok = spartan_verify_deferred<F, C>(S, digest, I, side_tag, tr, in, L.back());
    if (!ok) failed = true;
    return ok;
  }
  size_t openings() const { size_t n = 0; for (auto& a : a1) n += a.n_open; for (auto& a : a2) n += a.n_open; return n; }
};

constexpr size_t BATCH_MAX_OPENINGS = 6;      // a proof brings at most three arguments of two openings: the layout of a test's multipliers

// What a batch entry is made of.  deferred(i, vf, &res): the single verifier's body under the DeferredVerify policy (an error code ends the call);
// single(i, &res): the single entry itself.  given: NULL, or BATCH_MAX_OPENINGS multipliers of 2 words a proof (a test's).  seconds[6]: parse + host checks,
// tables, matrix evaluation, s-vector accumulation, MSMs, fallback (the subset equations of refused chunks and the single verifications).  probe (a test's):
// receives the accumulators of the LAST chunk's full equation (never a subset's), side 0 then side 1.  flags: BATCH_NO_BISECT; leaf: 0 = the default;
// stats[4] (optional): chunks refused, side equations evaluated after a refusal, single verifications run, members of refused chunks accepted by a subset equation.
// An error code — a member's deferred pass or single verification returning one, no randomness, a HIP error — ends the whole call with that code; `results` is
// then unspecified (the entries check what a caller can get wrong, a z0 element not below the modulus, before anything is written).
struct BatchProbe { uint64_t* acc[2] = {nullptr, nullptr}; };
inline int compressed_batch(const char* who, vimz_ctx* ctx, SpartanCache* cache, const vimz_bases* ck1, const vimz_bases* ck2, size_t n, size_t chunk, const uint64_t* given,
                            const std::function<int(size_t, DeferredVerify&, uint32_t*)>& deferred, const std::function<int(size_t, uint32_t*)>& single, uint32_t* results,
                            double seconds[6], BatchProbe* probe, uint32_t flags = 0, size_t leaf = 0, uint64_t* stats = nullptr) {
  double sec[6] = {0, 0, 0, 0, 0, 0};
  uint64_t cnt[bb::ST_N] = {0, 0, 0, 0};
  if (stats) memset(stats, 0, sizeof(cnt));
  auto done = [&](int rc) { if (seconds) memcpy(seconds, sec, sizeof(sec)); if (stats) memcpy(stats, cnt, sizeof(cnt)); return rc; };
  auto bad = [&](const char* why) { const std::string m = std::string(who) + ": " + why; return done(vz_fail(ctx, VIMZ_ERR_INVALID, m.c_str())); };
  if (flags & ~BATCH_NO_BISECT) return bad("unknown flag");
  if (!n) return done(VIMZ_OK);
  if (!chunk) chunk = BATCH_DEFAULT_CHUNK;
  if (!leaf) leaf = BATCH_DEFAULT_LEAF;
  if (given)
    for (size_t q = 0; q < BATCH_MAX_OPENINGS * n; q++) if (!(given[2 * q] | given[2 * q + 1])) return bad("a multiplier is zero");
  // 1. every proof's own bits and its deferred arguments, on the process's threads
  auto t0 = std::chrono::steady_clock::now();
  std::vector<DeferredVerify> vf(n);
  std::vector<int> rcs(n, VIMZ_OK);
  batch_parallel_for(n, batch_threads(), [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) {
      try { rcs[i] = deferred(i, vf[i], &results[i]); } catch (const std::exception&) { rcs[i] = VIMZ_ERR_INVALID; }
    }
  });
  for (size_t i = 0; i < n; i++) if (rcs[i]) return done(rcs[i]);
  std::vector<size_t> pending, again;
  for (size_t i = 0; i < n; i++) {
    if (!vf[i].calls) continue;                                  // judged before any argument: the word is final
    (vf[i].failed ? again : pending).push_back(i);
  }
  sec[0] += batch_since(t0);
  // 2. the chunks (the device scratch: allocated at the first, freed under the lock when the call is left)
  BatchDev D;
  bool have_dev = false;
  struct FreeDev { vimz_ctx* ctx; BatchDev& D; ~FreeDev() { std::lock_guard<std::mutex> g(ctx->mu); hipSetDevice(ctx->device); D.release(); } } free_dev{ctx, D};
  for (const auto& span : sb::chunk_plan(pending.size(), chunk)) {
    const size_t c0 = span.first, c1 = span.second;
    t0 = std::chrono::steady_clock::now();
    struct Secrets { std::vector<uint64_t> rho; ~Secrets() { if (!rho.empty()) explicit_bzero(rho.data(), 8 * rho.size()); } } X;
    size_t n_open = 0;
    for (size_t q = c0; q < c1; q++) n_open += vf[pending[q]].openings();
    X.rho.assign(2 * n_open, 0);
    if (!given) {
      if (!batch_os_random(X.rho.data(), 8 * X.rho.size())) return bad("no randomness from the OS");
      for (size_t o = 0; o < n_open; o++) {
        int tries = 0;
        while (!(X.rho[2 * o] | X.rho[2 * o + 1])) if (++tries > 8 || !batch_os_random(&X.rho[2 * o], 16)) return bad("no randomness from the OS");
      }
    }
    sec[0] += batch_since(t0);
    std::vector<uint8_t> good(c1 - c0, 1);
    bool holds[2] = {true, true};
    {
      std::lock_guard<std::mutex> g(ctx->mu);
      { const hipError_t e0 = hipSetDevice(ctx->device); if (e0 != hipSuccess) return done(vz_fail(ctx, VIMZ_ERR_HIP, who, e0)); }
      hipStream_t s = ctx->stream;
      hipError_t e = have_dev ? hipSuccess : D.alloc();
      if (e != hipSuccess) return done(vz_fail(ctx, VIMZ_ERR_HIP, who, e));
      have_dev = true;
      // 2a. vm of every argument; a proof with vm·vz != claim leaves the chunk for the single verifier
      auto mat = [&](auto* tag, SideDev& S) -> hipError_t {
        typedef typename std::remove_pointer<decltype(tag)>::type F;
        std::vector<const std::vector<F>*> rx, ry; std::vector<const F*> w; std::vector<size_t> owner;
        for (size_t q = c0; q < c1; q++)
          for (auto& A : vf[pending[q]].list((const F*)nullptr)) { rx.push_back(&A.rx); ry.push_back(&A.ry); w.push_back(A.w); owner.push_back(q - c0); }
        if (rx.empty()) return hipSuccess;
        std::vector<F> vm;
        double st[2] = {0, 0};
        const hipError_t e2 = batch_mat_eval<F>(s, S, D, rx, ry, w, vm, st);
        sec[1] += st[0]; sec[2] += st[1];
        if (e2 != hipSuccess) return e2;
        size_t k = 0;
        for (size_t q = c0; q < c1; q++)
          for (auto& A : vf[pending[q]].list((const F*)nullptr)) { if (!F::mul(vm[k], A.vz).eq(A.claim)) good[q - c0] = 0; k++; }
        return hipSuccess;
      };
      if ((e = mat((Fe*)nullptr, cache->side[0])) != hipSuccess) return done(vz_fail(ctx, VIMZ_ERR_HIP, who, e));
      if ((e = mat((Fq*)nullptr, cache->side[1])) != hipSuccess) return done(vz_fail(ctx, VIMZ_ERR_HIP, who, e));
      // 2b. the equation of each curve over the openings of the proofs still in.  A member keeps its arguments and its multipliers (its Fe arguments' openings
      // in order, then its Fq arguments') for every subset it appears in; the copies are wiped when the chunk is settled, on every way out
      struct Member { size_t q; std::vector<const DefArg<Fe, Fq>*> a1; std::vector<const DefArg<Fq, Fe>*> a2; std::vector<uint64_t> r1, r2; };
      struct Members {
        std::vector<Member> v;
        static void wipe(Member& M) { if (!M.r1.empty()) explicit_bzero(M.r1.data(), 8 * M.r1.size()); if (!M.r2.empty()) explicit_bzero(M.r2.data(), 8 * M.r2.size()); }
        ~Members() { for (Member& M : v) wipe(M); }
      } in;
      in.v.reserve(c1 - c0);
      {
        size_t o = 0;
        for (size_t q = c0; q < c1; q++) {
          DeferredVerify& V = vf[pending[q]];
          Member M; M.q = q;
          size_t k = 0;
          auto take = [&](std::vector<uint64_t>& dst, uint32_t cnt_open) {
            for (uint32_t j = 0; j < cnt_open; j++, k++, o++) {
              const uint64_t* src = given ? given + 2 * (BATCH_MAX_OPENINGS * pending[q] + k) : &X.rho[2 * o];
              dst.push_back(src[0]); dst.push_back(src[1]);
            }
          };
          for (auto& A : V.a1) { take(M.r1, A.n_open); M.a1.push_back(&A); }
          for (auto& A : V.a2) { take(M.r2, A.n_open); M.a2.push_back(&A); }
          if (good[q - c0]) in.v.push_back(std::move(M)); else Members::wipe(M);
        }
      }
      // one curve's equation over the members [lo, hi) of `in`: the chunk's, and a bisection's subsets'
      auto side_eq = [&](size_t lo, size_t hi, int side, bool* ok, double* st, double* sec_msm, uint64_t* probe_acc) -> hipError_t {
        std::vector<uint64_t> r;
        hipError_t e2;
        if (side == 0) {
          std::vector<const DefArg<Fe, Fq>*> a;
          for (size_t p = lo; p < hi; p++) { a.insert(a.end(), in.v[p].a1.begin(), in.v[p].a1.end()); r.insert(r.end(), in.v[p].r1.begin(), in.v[p].r1.end()); }
          e2 = batch_side_equation<Fe, BnG1>(s, *cache, cache->side[0], D, ck1, cache->ipa_u1, a, r.data(), ok, st, sec_msm, probe_acc);
        } else {
          std::vector<const DefArg<Fq, Fe>*> a;
          for (size_t p = lo; p < hi; p++) { a.insert(a.end(), in.v[p].a2.begin(), in.v[p].a2.end()); r.insert(r.end(), in.v[p].r2.begin(), in.v[p].r2.end()); }
          e2 = batch_side_equation<Fq, Grumpkin>(s, *cache, cache->side[1], D, ck2, cache->ipa_u2, a, r.data(), ok, st, sec_msm, probe_acc);
        }
        if (!r.empty()) explicit_bzero(r.data(), 8 * r.size());
        return e2;
      };
      double st[2] = {0, 0};
      e = side_eq(0, in.v.size(), 0, &holds[0], st, &sec[4], probe ? probe->acc[0] : nullptr);
      if (e == hipSuccess) e = side_eq(0, in.v.size(), 1, &holds[1], st, &sec[4], probe ? probe->acc[1] : nullptr);
      sec[1] += st[0]; sec[3] += st[1];
      if (e != hipSuccess) return done(vz_fail(ctx, VIMZ_ERR_HIP, who, e));
      // 2c. a refused chunk: the same equations over halves, on the curves that refused (an accepted member keeps the word of step 1)
      if (!(holds[0] && holds[1])) {
        const auto tb = std::chrono::steady_clock::now();
        const std::vector<bb::Subset> roots{{0, in.v.size(), (holds[0] ? 0u : 1u) | (holds[1] ? 0u : 2u)}};
        bb::Outcome out;
        if (flags & BATCH_NO_BISECT) out.singles = roots;
        else {
          const bool ok = bb::bisect(roots, leaf, [&](const std::vector<bb::Subset>& ask, std::vector<uint32_t>& held) {
            for (size_t k = 0; k < ask.size(); k++)
              for (int side = 0; side < 2; side++) {
                if (!((ask[k].sides >> side) & 1u)) continue;
                bool ok2 = false;
                if ((e = side_eq(ask[k].lo, ask[k].hi, side, &ok2, nullptr, nullptr, nullptr)) != hipSuccess) return false;
                if (ok2) held[k] |= 1u << side;
              }
            return true;
          }, &out);
          if (!ok) return done(vz_fail(ctx, VIMZ_ERR_HIP, who, e));
        }
        for (const bb::Subset& sgl : out.singles) for (size_t p = sgl.lo; p < sgl.hi; p++) again.push_back(pending[in.v[p].q]);
        cnt[bb::ST_REFUSED]++; cnt[bb::ST_EQUATIONS] += out.equations; cnt[bb::ST_ACCEPTED] += out.accepted;
        sec[5] += batch_since(tb);
      }
    }
    for (size_t q = c0; q < c1; q++) if (!good[q - c0]) again.push_back(pending[q]);
  }
  // 3. the single verifier for what the deferred pass or a chunk refused
  t0 = std::chrono::steady_clock::now();
  for (size_t i : again) { const int rc = single(i, &results[i]); if (rc) return done(rc); cnt[bb::ST_SINGLES]++; }
  sec[5] += batch_since(t0);
  return done(VIMZ_OK);
}

}  // namespace
