/* vimz_hip_testing.h — test hooks of the MI355X Nova-folding library.
 *
 * NOT part of the product ABI: libvimz_hip.so is built without them (tests/test_abi.py checks that it exports none of these symbols).
 * They are compiled under -DVIMZ_TESTING into vimz_amd/libvimz_hip_testing.so (the same sources otherwise) and, with the host passes
 * under ThreadSanitizer / AddressSanitizer, into vimz_amd/csrc/build/libvimz_hip_{tsan,asan}.so for the GPU-free ones
 * (tests/native/host_sanitize.cpp, run by the CPU suite).
 */
#ifndef VIMZ_HIP_TESTING_H
#define VIMZ_HIP_TESTING_H
#include "vimz_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* overwrite one element (canonical) of a witness vector on the device — which = 0 running main Z, 1 last fresh main Z, 2 running CycleFold Z,
 * 3 running main E, 4 running CycleFold E (soundness tests flip wires and expect vimz_cf_verify and the oracle-side verifier to reject) */
int vimz_cf_poke(vimz_cf* v, int which, size_t index, const uint64_t value[4]);
/* host only, no GPU — `steps` steps of the Nova + CycleFold recursion over the trivial step circuit with made-up commitments, every witness
 * checked against its R1CS and every in-circuit fold against field / curve arithmetic (result 0 = good; counts: F' wires, constraints,
 * CycleFold wires, constraints, then of the last step's flip test — every wire incremented by one must violate a row — wires of F'
 * flipped, unnoticed, wires of the CycleFold circuit flipped, unnoticed). */
int vimz_cf_selfcheck(int steps, uint32_t* result, uint64_t counts[8]);
/* the LAST step of the same host-only run, for an outside restatement of the relation F' enforces: digest, z_0 (one element), then the words of
 * VIMZ_IX_LAST_STEP.  Returns the byte size (copies when buf is large enough); negative on error or when the self-check itself fails. */
int64_t vimz_cf_selfcheck_last_step(int steps, void* buf, size_t cap);
/* host only: two runs of made-up, self-consistent segment records replayed by the library; output = digest, word count + records, the
 * accumulator arrived at (layout: cyclefold_merge.hip) — for an outside replay of the merge transcript in the CPU suite.  Returns the byte size. */
int64_t vimz_cf_selfcheck_merge(int segs_run0, int segs_run1, void* buf, size_t cap);
/* host only: `jobs` trivial jobs posted to and awaited from one helper thread of the verifier circuits' witness generators; returns how many
 * ran.  With VIMZ_WORKER_SPIN_US=0 the helper sleeps between jobs, so that every post is a wake-up (a lost one hangs the call). */
int64_t vimz_worker_selftest(int jobs);
/* host only: the canonical bit decomposition of hash outputs (aug/cs.hpp: bits_strict) against the ALIASED witness — the bits of h + p for
 * hash values h with h + p below 2^254 — on the gadget alone and inside F' (field 0 = BN254 Fr, 1 = Fq).  out[0] = values tried,
 * out[1] = of them aliasable, out[2] = aliased witnesses that satisfy the plain gadget's rows (must equal out[1]: the attack is real),
 * out[3] = aliased witnesses whose only violated rows are rows of the comparison with p - 1 (must equal out[1]: the fix is what stops it),
 * out[4] = honest witnesses that violate a row (must be 0), out[5] = steps of F' run with aliased challenge decompositions,
 * out[6] = of them left satisfiable (must be 0), out[7] = steps in which an alias existed. */
int vimz_strict_bits_selfcheck(int field, int values, uint64_t out[8]);
/* the negative test of the compressed proof's public-slot binding (tests/test_gpu_compress.py): while on, vimz_ivc_compress plays a cheating
 * prover that claims x0 + 1 for the last fresh instance and hides the difference under the generator of that wire's slot */
void vimz_test_forge_public_slot(int on);
/* deterministic TEST setups of the decider path (vimz_kzg_setup / vimz_decider_setup with the toxic waste derived from `seed`: anyone who knows the
 * seed can forge) — for reproducible keys in tests and benchmarks only */
/* host only, no GPU: the decider circuit over `steps` steps of the Nova + CycleFold recursion of the trivial step circuit (made-up commitments, the running
 * witness folded on the host), its final fold, witness and R1CS; full != 0: the FULL decider, over real CycleFold instances kept on the host; result 0 = good
 * (bits: vimz_amd/csrc/groth16.hip); counts = {decider constraints, wires, public inputs, main constraints} */
int vimz_decider_selfcheck(int steps, int full, uint32_t* result, uint64_t counts[4]);
int vimz_testing_kzg_setup_seeded(vimz_ctx* ctx, const uint8_t* seed, size_t seed_len, size_t n, vimz_bases** srs_out, uint64_t vk_g2_out[16]);
int vimz_testing_decider_setup_seeded(vimz_cf* prover, const uint64_t kzg_vk_g2[16], int light, const uint8_t* seed, size_t seed_len, vimz_decider** out, double seconds[4]);

/* ONE operation of the lazily reduced 9 x 29-bit field (vimz_amd/csrc/fp29.hpp) on raw operands, per element on the device: a, b, c, d and out are HOST
 * arrays of n slots of 9 words, limbs as they stand (no conversion on the way in or out; values of the 8 x 32 side in the first eight words; predicates
 * write 0 / 1).  field = VIMZ_FIELD_*, op = the codes of vimz_amd/csrc/fp29_probe.hpp — the same function tests/native/fp29_probe_host.cpp runs on the
 * host.  Operands must be inside the operation's contract (tests/_fp29_ref.py). */
int vimz_test_fp29_probe(vimz_ctx* ctx, int field, int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out, size_t n);
/* the fused products + cross term kernel of the verifier circuits' rows (k_spmv_cross16) on a caller's shape: rows [row0, row0 + nrows) of (A,B,C)·z into
 * az, bz, cz and, when az1 is given, T = az1∘bz + az∘bz1 − u1·cz − u2·cz1 of those rows (az1 NULL = step 0: products only; T may then be NULL).  Every
 * vector holds at least the shape's rows (z its columns); rows outside the range are left as they were. */
int vimz_test_spmv_cross16(vimz_ctx* ctx, const vimz_r1cs* S, size_t row0, size_t nrows, const vimz_vec* z, vimz_vec* az, vimz_vec* bz, vimz_vec* cz,
                           const vimz_vec* az1, const vimz_vec* bz1, const vimz_vec* cz1, const uint64_t u1[4], const uint64_t u2[4], int form, vimz_vec* T);
/* k_cross_term over n elements with its boolean-row form: T as ever and, when Tm is given, the vector the dense MSM of a step takes — for i < nb twice T_i
 * where az2_i is one, zero where it is zero, T_i + az1_i where it is anything else; T_i from nb on (instance 2 is the fresh one). */
int vimz_test_cross_term_masked(vimz_ctx* ctx, size_t n, const vimz_vec* az1, const vimz_vec* bz1, const vimz_vec* cz1, const uint64_t u1[4], const vimz_vec* az2,
                                const vimz_vec* bz2, const vimz_vec* cz2, const uint64_t u2[4], int form, vimz_vec* T, vimz_vec* Tm, size_t nb);
/* The element-wise kernels of a fold step (vimz_amd/csrc/r1cs_ops.hpp) on a caller's vectors, each through the product's kernel template with the product's block size
 * (tests/test_gpu_fold_kernels.py; the reference and the cases: tests/_fold_ref.py).  All four fields; scalars: 4 words, form = VIMZ_FORM_*.  blocks = 0: the product's
 * grid — stream_grid(n) for k_fold_cross and k_fresh_cross_neg, 2048 for k_fold5 —, blocks in 1..2048: that grid, so that a few hundred elements reach the grid stride.
 * Every length, field and alias is checked before anything is launched (VIMZ_ERR_INVALID with a message).
 * _fold_cross: k_fold_cross over n elements — (AZ, BZ, CZ) += r·(az, bz, cz); with fold_E: E += r·(Tin − hasB·r_prev·negB), E left alone where that vector is zero; with
 *   out: out = AZ'∘bzn + BZ'∘azn − u1_new·czn − u2·CZ' of the folded products and, with outm, its boolean-row form over the first nb elements (as
 *   vimz_test_cross_term_masked's Tm).  Tin may be NULL without fold_E, negB unless fold_E and hasB; out NULL: no cross term (azn, bzn, czn, outm then unused).  out
 *   may be the very vector passed as Tin — what the lookahead does —; every other vector written must be one of its own, outm differ from out.
 * _fold5: k_fold5 over five groups: x1[v][off1[v] .. + n[v]) += r·x2[v][off2[v] .. + n[v]), offsets in elements; x1[v] NULL: the group is skipped (the error vector at
 *   step 0).  A range written must overlap no other range of the call.
 * _fresh_cross_neg: k_fresh_cross_neg over n elements of two fresh product triples: out = cz0 + cz1 − az0∘bz1 − az1∘bz0.
 * _count: one of the counting kernels that guard imported and merged proofs, over the first n elements, on a counter the hook zeroes: what = 0, k_count_unreduced —
 *   the elements of a whose words as they lie are not below the modulus (upload them with VIMZ_FORM_MONTGOMERY: copied as they are) —; what = 1, k_count_diff — the
 *   elements at which a and b differ in any word. */
int vimz_test_fold_cross(vimz_ctx* ctx, size_t n, vimz_vec* AZ, vimz_vec* BZ, vimz_vec* CZ, vimz_vec* E, const vimz_vec* Tin, int fold_E, const uint64_t r[4], int hasB,
                         const uint64_t r_prev[4], const vimz_vec* negB, const uint64_t u1_new[4], const vimz_vec* az, const vimz_vec* bz, const vimz_vec* cz, vimz_vec* out,
                         const vimz_vec* azn, const vimz_vec* bzn, const vimz_vec* czn, const uint64_t u2[4], int form, vimz_vec* outm, size_t nb, unsigned blocks);
int vimz_test_fold5(vimz_ctx* ctx, vimz_vec* const x1[5], const size_t off1[5], const vimz_vec* const x2[5], const size_t off2[5], const size_t n[5], const uint64_t r[4], int form,
                    unsigned blocks);
int vimz_test_fresh_cross_neg(vimz_ctx* ctx, size_t n, const vimz_vec* az0, const vimz_vec* bz0, const vimz_vec* cz0, const vimz_vec* az1, const vimz_vec* bz1, const vimz_vec* cz1,
                              vimz_vec* out, unsigned blocks);
int vimz_test_count(vimz_ctx* ctx, int what, size_t n, const vimz_vec* a, const vimz_vec* b, uint64_t* count);
/* msm_launch_rows (vimz_amd/csrc/msm.hpp) on a caller's rows: G (<= 16) vectors of n scalars each, row r at scalars + 4·r·row_stride words of 64 bits (host;
 * form = VIMZ_FORM_*), committed over the first n points of a BN254 G1 key as ONE chain of launches with the unit scalars split off — with the key's shared-bucket
 * window tables (use_tables != 0; vimz_bases_precompute first) or without — `calls` times over on ONE fresh workspace.  out_xy: calls·G affine points
 * (canonical, 8 words each, the identity as zeros), call after call.  n_ones != 0: every row's unit sum over its first n_ones scalars rides along as the
 * producer's S_1 sums do (s1_xy, calls·G points) and is computed again by one ones_launch per row (s1_ref_xy, G points). */
int vimz_test_msm_rows(vimz_ctx* ctx, const vimz_bases* bases, const uint64_t* scalars, size_t n, size_t row_stride, size_t G, int form, int use_tables,
                       size_t n_ones, int calls, uint64_t* out_xy, uint64_t* s1_xy, uint64_t* s1_ref_xy);
/* The tail stages of the large MSM (vimz_amd/csrc/msm.hpp) and the four-lane additions under them (ec_mem.hpp) on a caller's arrays, each through the launcher the
 * product calls (tests/test_gpu_msm_tail.py; the reference and the cases: tests/_msm_tail_ref.py).  curve = VIMZ_CURVE_*, all four.  Points are raw XYZZ slots in the
 * resident layout of store_xyzz / load_xyzz — 40 words a point: X, Y, ZZ, ZZZ of nine 29-bit limbs in ten words each, Montgomery radix 2^261 — limbs as they stand, no
 * conversion on the way in or out: any representative inside ec.hpp's bounds (X < 5.3 p, Y < 3.4 p, ZZ, ZZZ < 1.5 p; ZZ = 0: the identity) goes in, the kernel's own
 * comes back.  Every layout is validated before anything is launched (VIMZ_ERR_INVALID with a message).  calls: that many runs on ONE set of tickets (totals[2],
 * totals[3], heavy_done), each on the caller's input again; the last run's output comes back.
 * _scan: blocks (1..256) per-workgroup histograms of nb counters; lds = 1: k_prefix_scan over them (block_hist_out: the exclusive prefixes per block it leaves), lds = 0:
 * their sums through k_scan.  counts_out nb, bucket_off_out and sub_off_out nb + 1 words, totals_out = totals[0..3] (sub-buckets, entries, the two tickets), heavy_out:
 * 1 + 65536 + 64 words — the count, the ids (as many as the count, or the cap, says; the rest 0xffffffff), 64 guard words that must come back 0xffffffff.
 * _combine: k_combine in place over rows (1..16) x n_slots slots of `partial`, sub_off rows x (nb + 1), heavy rows x (1 + n_ids) words: the count word — above 65536: a
 * list that overflowed — and the ids (each below nb, listed once, of a bucket with more than heavy_min partials), at the product's row strides on the device.
 * _reduce: mode 0 k_reduce, `windows` sums of nbw buckets each; 1 the same with the plain sums after them (2·windows points a row); 2 k_reduce_planes over one row of
 * one bucket set, log2(nbw) + 2 sums, the planes' shape from msm_plane_shape.  counts rows x nb, sub_off rows x (nb + 1), nb = nbw·windows.
 * _tree: count = 0: the sum of m <= 65536 points by k_tree256, level after level as the unit sums chain it (one point out); count 1..16: that many sums of m <= 256
 * points each by k_tree_rows (count points out).
 * vimz_test_quad_level: a TEST-ONLY kernel — workgroup s loads slots [256 s, 256 s + 256) into LDS, applies n_levels levels through quad_level (a level: 129 words — count
 * <= 64, dst[64], src[64]; indices below 256, the dst of a level distinct) or, tree != 0, quad_tree256, and stores all 256 slots to out. */
int vimz_test_msm_scan(vimz_ctx* ctx, const uint32_t* block_hist, size_t blocks, size_t nb, uint32_t sub, uint32_t heavy_min, int lds, int calls, uint32_t* counts_out,
                       uint32_t* bucket_off_out, uint32_t* sub_off_out, uint32_t totals_out[4], uint32_t* heavy_out, uint32_t* block_hist_out);
int vimz_test_msm_combine(vimz_ctx* ctx, int curve, uint32_t* partial, size_t n_slots, const uint32_t* sub_off, size_t nb, const uint32_t* heavy, size_t n_ids, int lane_bits,
                          uint32_t heavy_min, size_t rows, int calls);
int vimz_test_msm_reduce(vimz_ctx* ctx, int curve, const uint32_t* partial, size_t n_slots, const uint32_t* counts, const uint32_t* sub_off, uint32_t nbw, size_t windows,
                         int mode, size_t rows, int calls, uint32_t* sums_out);
int vimz_test_msm_tree(vimz_ctx* ctx, int curve, const uint32_t* points, size_t m, size_t count, uint32_t* out);
int vimz_test_quad_level(vimz_ctx* ctx, int curve, const uint32_t* slots, size_t sets, const uint32_t* levels, size_t n_levels, int tree, uint32_t* out);
/* The head stages of the MSM (vimz_amd/csrc/msm.hpp) — the digit producers, both counting sorts, k_accum, the unit sums, the two fused paths, the table builders — each
 * through the function the product calls (tests/test_gpu_msm_head.py; the reference and the cases: tests/_msm_head_ref.py).  Scalars are HOST arrays of 4 words of 64
 * bits, taken AS THEY LIE in form = VIMZ_FORM_* (no conversion on the way in: a Montgomery word is the caller's own s·2^256 mod p).  Points come back as raw XYZZ slots
 * (40 words, as in the tail hooks above).  Every layout is validated before anything is launched (VIMZ_ERR_INVALID with a message).  calls: that many runs on ONE
 * workspace of the hook's own — counters and tickets included —, each on the caller's input again; outputs hold `calls` results, call after call.
 * _sort: launch_sort over n scalars of `field` (all four) — skip_ones, sgn as load_scalar takes them; window_bits 2..16 and K windows; shared = 0: a bucket set of
 *   2^(window_bits - 1) buckets per window, 1: one set for all windows; entries are (index + window·pstride) | negative << 31.  lds = 1: k_hist_lds, k_prefix_scan,
 *   k_scatter_lds over sort_blocks (1..256) workgroups — refused where the nb counters exceed 144 KiB, as msm_shape refuses it; lds = 0: k_hist, k_scan, k_scatter.
 *   counts_out nb, bucket_off_out and sub_off_out nb + 1, totals_out 4 words (sub-buckets, entries, the two tickets), sorted_out sorted_len >= K·n words a call,
 *   filled with 0xffffffff before every call.
 * _accum: launch_accum over rows (1..16) of sorted (rows x entries), bucket_off and sub_off (rows x (nb + 1)) and totals (rows x 16 words; [0]: the sub-buckets to
 *   accumulate) at the product's row strides, over the points of `bases` (any curve); partial: rows x n_slots slots, in place — the caller's fill shows where nothing was
 *   written.  Refused: offsets not monotone or outside their arrays, a sub_off that is not the scan of ceil(size / sub), an entry outside the key.
 * _small: launch_small (k_msm_small; tail = 0: the ticket merge inside it, 1: k_msm_small_sum) over n scalars of the curve's scalar field and the points
 *   [base_offset, base_offset + n) of the key — use_tables != 0: through the rows 2^(7w)·P_i that vimz_bases_precompute(7) made, row length the key's —, Q chunks of
 *   `chunk` points: chunk·(Q - 1) < n <= chunk·Q, chunk <= 1536, Q <= 32.  sums_out: K = ceil((bits + 1) / 7) window sums a call.
 * _fixed: launch_fixed (k_msm_fixed, ceil(n / 1024) workgroups a window) over the key's tables of multiples (vimz_bases_precompute(7)).  sums_out as _small.
 * _ones: the sum of the points whose scalar is the unit.  kind 0: k_ones_partial, 1: k_ones_dense — launch_ones, then launch_tree256 as the product chains them, one
 *   row; 2: ones_launch_rows (k_ones_dense_rows + k_tree_rows) over rows (1..32) vectors, row r at scalars + 4·r·row_stride words.  out: one slot a row.
 * vimz_test_bases_tables: `count` entries of a key's tables, canonical affine, 8 words each, the identity as zeros.  wim: (w, i, m) a entry.  which = 0: point i of
 *   row w of the window tables made by vimz_bases_precompute(window_bits) (k_build_tables; m ignored); 1: m·(row w, point i), m in 1..64 (k_build_multiples;
 *   window_bits 7 only). */
int vimz_test_msm_sort(vimz_ctx* ctx, int field, const uint64_t* scalars, size_t n, int form, int skip_ones, int sgn, int window_bits, int K, int shared, uint32_t pstride, int lds,
                       uint32_t sort_blocks, uint32_t sub, uint32_t heavy_min, int calls, uint32_t* counts_out, uint32_t* bucket_off_out, uint32_t* sub_off_out, uint32_t* totals_out,
                       uint32_t* sorted_out, size_t sorted_len);
int vimz_test_msm_accum(vimz_ctx* ctx, const vimz_bases* bases, const uint32_t* sorted, size_t entries, const uint32_t* bucket_off, const uint32_t* sub_off, const uint32_t* totals,
                        size_t nb, uint32_t sub, size_t rows, uint32_t* partial, size_t n_slots);
int vimz_test_msm_small(vimz_ctx* ctx, const vimz_bases* bases, int use_tables, size_t base_offset, const uint64_t* scalars, size_t n, int form, int sgn, uint32_t Q, uint32_t chunk,
                        int tail, int calls, uint32_t* sums_out);
int vimz_test_msm_fixed(vimz_ctx* ctx, const vimz_bases* bases, size_t base_offset, const uint64_t* scalars, size_t n, int form, int sgn, int calls, uint32_t* sums_out);
int vimz_test_msm_ones(vimz_ctx* ctx, const vimz_bases* bases, const uint64_t* scalars, size_t n, size_t row_stride, size_t rows, int form, int kind, uint32_t* out);
int vimz_test_bases_tables(vimz_ctx* ctx, const vimz_bases* bases, int window_bits, int which, const uint32_t* wim, size_t count, uint64_t* out_xy);
/* The decider's kernels (vimz_amd/csrc/groth16.hip) on a caller's shapes, through the functions the set-up and the prover call (tests/test_gpu_g16_kernels.py).
 * The domain of n = 2^logn points, logn in 1..26, with the constants and twiddle tables a key holds: a, b, c and out are HOST arrays of n scalars of 4 words
 * (form = VIMZ_FORM_*, out in the same form).  what = 0: the forward NTT of a; 1: the inverse NTT of a, UNSCALED (n times the inverse); 2: a's evaluations
 * over the coset 5·H (inverse, scale by 5^i / n, forward); 3: the n coefficients of h = (A·B − C) / Z for the evaluations a, b, c (b, c: only here). */
int vimz_test_g16_domain(vimz_ctx* ctx, int logn, int what, const uint64_t* a, const uint64_t* b, const uint64_t* c, int form, uint64_t* out);
/* s_i·G for n >= 1 canonical scalars below r as the set-up makes its key points (the host's window table, k_fixed_mul): group = 1 the generator of G1, out_xy 8
 * words per point (x, y); group = 2 the generator of G2, 16 words per point (x.c0, x.c1, y.c0, y.c1).  Canonical; the identity as zeros. */
int vimz_test_g16_fixed_mul(vimz_ctx* ctx, int group, const uint64_t* scalars, size_t n, uint64_t* out_xy);
/* the proof's G2 multi-scalar multiplication on a caller's query: sum of wires[idx[i]]·P_i over n >= 1 points of G2 (canonical, 16 words each, the identity as
 * zeros), m >= n wire values of 4 words (form = VIMZ_FORM_*) and n wire numbers below m.  out_xy: the affine sum, canonical, the identity as zeros. */
int vimz_test_g16_g2_msm(vimz_ctx* ctx, const uint64_t* bases_xy, size_t n, const uint64_t* wires, size_t m, int form, const uint32_t* idx, uint64_t out_xy[16]);
/* The same-scalar multiplication of a set-up from a powers-of-tau string (vimz_amd/csrc/g16_powers.hip: g16_scale_points, k_scale_points), in place as the
 * set-up uses it: out_i = scalar · P_i for n >= 1 points of G1 (canonical, 8 words each, the identity as zeros; each on the curve) and one canonical scalar
 * below r.  out_xy: n affine points, canonical, the identity as zeros. */
int vimz_test_g16_scale_points(vimz_ctx* ctx, const uint64_t* points_xy, size_t n, const uint64_t scalar[4], uint64_t* out_xy);
/* The transform over points of the same set-up (g16_point_transform: k_pt_twiddles, k_pt_bitrev, one k_pt_stage per stage, k_scale_points), in place on the
 * device as vimz_powers_lagrange runs it, in every direction: out_j = sum_k w^(jk)·P_k over the 2^logn points, logn in 1..26, w the domain's root of unity
 * (tests/_g16_ref.omega) or, with inverse != 0, its inverse; with scaled != 0 times 1/n.  group = 1: points of G1, 8 words each; 2: of G2, 16 words (x.c0, x.c1,
 * y.c0, y.c1).  Canonical on both sides, the identity as zeros; every input below q and on its curve. */
int vimz_test_g16_point_transform(vimz_ctx* ctx, int group, int logn, int inverse, int scaled, const uint64_t* points, uint64_t* out);
/* The column sums of the same set-up (g16_colsum_plan.hpp: colsum_plan, then g16_column_sums: one k_col_runs launch per level of the plan — the very two calls
 * vimz_decider_setup_from_powers makes): out_j = sum over the entries (r, k) with col[k] = j of dict[coef[k]]·P_r for a CSR matrix of n_rows rows (row_ptr: n_rows
 * + 1 offsets) and n_cols >= 1 columns, n_dict >= 1 canonical coefficients below r of 4 words, and n_rows points.  group = 1: points of G1, 8 words each; 2: of
 * G2, 16 words.  form = VIMZ_FORM_* of the points' coordinates, out (n_cols points) in the same form; the identity as zeros; every input below q and on its curve. */
int vimz_test_g16_column_sums(vimz_ctx* ctx, int group, const uint32_t* row_ptr, const uint32_t* col, const uint32_t* coef, size_t n_rows, size_t n_cols,
                              const uint64_t* dict, size_t n_dict, const uint64_t* points, int form, uint64_t* out);
/* The h query of the same set-up (g16_h_query: k_point_diff, then k_scale_points in place): out_j = delta_inv·(P_(j+n) − P_j) for j < n − 1 over 2n − 1 points of
 * G1, n >= 2, and one canonical scalar below r.  Canonical on both sides, 8 words a point, the identity as zeros. */
int vimz_test_g16_h_query(vimz_ctx* ctx, const uint64_t* tau_g1_xy, size_t n, const uint64_t delta_inv[4], uint64_t* out_xy);
/* The two device stages of vimz_powers_verify (vimz_amd/csrc/g16_powers_verify.hip) on a caller's points, through the function the product runs on each array of a
 * string.  group = 1: points of G1, 8 words each; 2: of G2, 16 words (x.c0, x.c1, y.c0, y.c1); form = VIMZ_FORM_*; the identity as zeros.
 * _flags: flags[i] = 0 or the VIMZ_POWERS_COORD / _OFF_CURVE / _IDENTITY / _SUBGROUP finding of point i (k_powers_flags; the coordinates' range on the host), n >= 1.
 * _rlc: out = S = sum rho_i·P_i, then S' = sum rho_i·P_(i+1), over i < n − 1 (k_powers_rlc twice, each reduced by g16_column_sums), n >= 2 points none of which
 * is flagged, rho: 2 words of 64 bits a pair (any 128-bit value), out: 2 points in the form of the input. */
int vimz_test_powers_flags(vimz_ctx* ctx, int group, const uint64_t* points, size_t n, int form, uint32_t* flags);
int vimz_test_powers_rlc(vimz_ctx* ctx, int group, const uint64_t* points, size_t n, const uint64_t* rho, int form, uint64_t* out);
/* The two set-ups a test compares byte for byte (vimz_decider_key_save): the trapdoor set-up (decider_setup_impl) with a GIVEN trapdoor — tau, alpha, beta, gamma,
 * delta: 4 canonical words each, non-zero, below r — and vimz_decider_setup_from_powers with a given delta.  Whoever knows these scalars can forge. */
int vimz_testing_decider_setup_trapdoor(vimz_cf* prover, const uint64_t kzg_vk_g2[16], int light, const uint64_t td[20] /* tau, alpha, beta, gamma, delta */,
                                        vimz_decider** out, double seconds[4]);
int vimz_testing_decider_setup_from_powers_delta(vimz_cf* prover, int light, const uint64_t* tau_g1, size_t n_tau_g1, const uint64_t* tau_g2, const uint64_t* alpha_g1,
                                                 const uint64_t* beta_g1, size_t n_pow, const uint64_t beta_g2[16], int form, const uint64_t delta[4], vimz_decider** out,
                                                 double seconds[6]);
/* vimz_decider_key_contribute (vimz_amd/csrc/g16_key_contrib.hip) with a GIVEN delta' and nonce — 4 canonical words each, below r, delta' non-zero — so that a test
 * compares the key and the record byte for byte.  Whoever knows delta' can undo the contribution. */
int64_t vimz_testing_decider_key_contribute_delta(vimz_ctx* ctx, const void* key_in, size_t len, void* key_out, size_t cap, uint64_t record_out[37], const uint64_t delta[4],
                                                  const uint64_t nonce[4], double seconds[3]);
/* The device stage of vimz_decider_key_verify_contributions' same-ratio check on a caller's points, through the functions the product runs: out = S = sum rho_i·before_i,
 * then S' = sum rho_i·after_i over i < n (k_ratio_rlc: one launch over both arrays, reduced by g16_column_sums over a plan of two columns).  n >= 1 points of G1 each,
 * 8 words a point, form = VIMZ_FORM_*, the identity as zeros, every point on the curve; rho: 2 words of 64 bits a point (any 128-bit value); out: 2 points in the form
 * of the input.  _forms: the same with launches = 1, or launches = 2 — the two sums through two launches of k_powers_rlc (shift 0 each), what the single launch is
 * measured against (profiles/key_contrib.txt) —, the combination queued `reps` times on the uploaded arrays, rep_seconds[r] (optional) = launch to synchronise. */
int vimz_test_ratio_rlc(vimz_ctx* ctx, const uint64_t* before, const uint64_t* after, size_t n, const uint64_t* rho, int form, uint64_t* out /* S, S' */);
int vimz_test_ratio_rlc_forms(vimz_ctx* ctx, const uint64_t* before, const uint64_t* after, size_t n, const uint64_t* rho, int form, int launches, int reps, uint64_t* out,
                              double* rep_seconds);
/* vimz_powers_contribute (vimz_amd/csrc/g16_powers_contrib.hip) with GIVEN secrets tau', alpha', beta' and nonces k_tau, k_alpha, k_beta — 4 canonical words each, below
 * r, the secrets non-zero — so that a test compares the string and the record word for word.  Whoever knows the secrets can undo the contribution. */
int vimz_testing_powers_contribute_secrets(vimz_ctx* ctx, const uint64_t* tau_g1, size_t n_tau_g1, const uint64_t* tau_g2, const uint64_t* alpha_g1, const uint64_t* beta_g1,
                                           size_t n_pow, const uint64_t beta_g2[16], int form, uint64_t* tau_g1_out, uint64_t* tau_g2_out, uint64_t* alpha_g1_out,
                                           uint64_t* beta_g1_out, uint64_t beta_g2_out[16], uint64_t record_out[61], const uint64_t secrets[12], const uint64_t nonces[12],
                                           double seconds[3]);
/* The two kernels of that contribution on a caller's shapes, through the functions the product queues.
 * _power_vec: out[i] = w^i for i < count, 1 <= count <= 2^26 (k_power_vec over bitlen(count − 1) bits); w: 4 canonical words below r; out: 4 canonical words each.
 * _scale_points_by: out[i] = (c·w^i)·P_i for n >= 1 points (k_power_vec, then k_scale_points_by with c as its argument); group = 1: points of G1, 8 words each; 2: of
 * G2, 16 words (x.c0, x.c1, y.c0, y.c1); form = VIMZ_FORM_* of the coordinates, out in the same form and possibly `points`; the identity as zeros; w, c: 4 canonical
 * words below r, zero allowed (the production entry never passes one); every input below q and on its curve. */
int vimz_test_power_vec(vimz_ctx* ctx, const uint64_t w[4], size_t count, uint64_t* out);
int vimz_test_scale_points_by(vimz_ctx* ctx, int group, const uint64_t* points, size_t n, const uint64_t w[4], const uint64_t c[4], int form, uint64_t* out);
/* The origin check of a key (vimz_amd/csrc/g16_key_origin.hip) on a caller's shapes, through the functions the product calls.  csr = {row_ptr of A, B, C; col of A, B, C;
 * coef of A, B, C}: a builder's CSRs as they are (row_ptr: n_c + 1 offsets; col: a wire number below m; coef: an index into dict), nnz their entries; dict: n_dict
 * canonical coefficients below r of 4 words.  An offset, wire number or index out of bounds is VIMZ_ERR_INVALID with a message: nothing is launched.
 * _spmv_dict: g16_spmv_upload, then ONE g16_spmv3_dict launch (k_spmv3_dict): out_q[i] = (row i of matrix q)·v for i < n_c, zero for n_c <= i < n; v: m canonical
 * elements of 4 words, out_a, out_b, out_c: n >= n_c canonical elements each.
 * _key_origin: vimz_decider_key_verify_origin's driver on that R1CS instead of the decider's — m wires, n_pub public inputs, n_c constraints, the domain 2^logn >=
 * n_c + n_pub + 1, the header's pp_hash words (len_z and mode are not compared: such a circuit has neither) — with a GIVEN rho ‖ rho': m + 2^logn - 1 scalars of 2
 * words (any 128-bit values).  The product call is this same function with the decider's circuit and the OS's randomness.  points_out (zeros unless the equations
 * were reached): the key-side sums of a (8 words), b1 (8), b2 (16), ic (8), l (8), h (8), then the string-side a (8), b1 (8), b2 (16), K(P) (8), K(Q) (8) and the h
 * combination (8) — canonical, the identity as zeros. */
int vimz_test_g16_spmv_dict(vimz_ctx* ctx, const uint32_t* const csr[9], const size_t nnz[3], const uint64_t* dict, size_t n_dict, size_t m, size_t n_c, size_t n, const uint64_t* v,
                            uint64_t* out_a, uint64_t* out_b, uint64_t* out_c);
int vimz_test_key_origin(vimz_ctx* ctx, const uint32_t* const csr[9], const size_t nnz[3], const uint64_t* dict, size_t n_dict, size_t m, size_t n_pub, size_t n_c, int logn,
                         const uint64_t pp_hash[4], const void* key, size_t len, const uint64_t* tau_g1, size_t n_tau_g1, const uint64_t* tau_g2, const uint64_t* alpha_g1,
                         const uint64_t* beta_g1, size_t n_pow, const uint64_t beta_g2[16], int form, const uint64_t* rho, uint32_t* result, uint64_t first_bad[2],
                         uint64_t points_out[112]);
/* The chains of the full decider's check 5 (vimz_amd/csrc/aug/decider_cf.hpp: every scalar walks the 127 two-bit windows of its generator's table by affine
 * additions from the derived generator H) over a caller's generators and scalars, through the functions the prover calls: where = 0 the host's
 * (cf_open_chains_host; ctx may be NULL), where = 1 the device's (k_cf_open_chains, the scalars uploaded in Montgomery form as the prover holds them, both
 * openings of one launch filled with them).  gens_xy: n_gens affine points of Grumpkin, canonical, 8 words each (the key is built by CfOpeningKey::build);
 * scalars: cnt <= n_gens canonical scalars below q, scalar k over generator k.  wires_out: cnt·127·4 elements (b0·b1, slope, x, y per window), ends_out: cnt
 * points, h_out: H — all canonical.  *bad_out = 1: an addition met two points with the same x (the wires are then unspecified). */
int vimz_test_decider_chains(vimz_ctx* ctx, int where, const uint64_t* gens_xy, size_t n_gens, const uint64_t* scalars, size_t cnt, uint64_t* wires_out,
                             uint64_t* ends_out, uint64_t h_out[8], int* bad_out);
/* the full assignment z (canonical, 4 words per wire) of the decider circuit as vimz_decider_prove builds it for the proof `ivc` holds, check 5's chains from
 * the host (chains_on_gpu = 0) or from the device.  Returns the byte size (copies when buf is large enough); negative: vimz_decider_prove's error codes. */
int64_t vimz_testing_decider_witness(vimz_decider* d, vimz_cf* ivc, int chains_on_gpu, void* buf, size_t cap);
/* The two kernels of vimz_decider_verify_batch (vimz_amd/csrc/decider_batch.hip) on a caller's points, through the functions the product queues.
 * _miller_loops: out[96·t ..] = the Miller value of (P_t, Q_t) over 6t + 2 with the two Frobenius steps (k_miller, pairing_stage.hpp's projective steps — NOT
 * pairing.hpp's affine ones: the two differ by factors the final exponentiation removes; the word-for-word reference is tests/_miller_ref.py): the 12 Fq
 * coefficients c0.c0.c0, c0.c0.c1, c0.c1.c0, .. c1.c2.c1, canonical, 8 words of 32 bits each; one when either point is the identity.  g1_xy: n >= 1 points of G1,
 * 8 words of 64 bits each; g2_xy: n points of G2, 16 words (x.c0, x.c1, y.c0, y.c1); canonical, below q, the identity as zeros.
 * _g1_lincomb: out_t = a_t + k_t·b_t (k_g1_lincomb) over exactly bits[t] <= 256 bits of k_t (4 words of 64 bits; the bits above are not read); points canonical, on
 * the curve, the identity as zeros on both sides. */
int vimz_test_miller_loops(vimz_ctx* ctx, const uint64_t* g1_xy, const uint64_t* g2_xy, size_t n, uint32_t* out);
int vimz_test_g1_lincomb(vimz_ctx* ctx, const uint64_t* a_xy, const uint64_t* k, const uint32_t* bits, const uint64_t* b_xy, size_t n, uint64_t* out_xy);
/* vimz_decider_verify_batch with GIVEN multipliers: 3n of 2 words (rho_i, sigma_i, sigma'_i of proof i; any non-zero 128-bit values, a zero is VIMZ_ERR_INVALID).
 * Whoever knows the multipliers can make a chunk of wrong proofs pass: two proofs with their C points swapped pass under multipliers that are all one. */
int vimz_testing_decider_verify_batch_scalars(vimz_ctx* ctx, const uint64_t* key_words, size_t n_key_words, uint32_t len_z, size_t n, const uint64_t* steps, const uint64_t* z0,
                                              const uint64_t* zi, const uint64_t* words, size_t chunk, const uint64_t* multipliers, uint32_t* results, double seconds[6]);
/* the same with vimz_decider_verify_batch_ex's flags, leaf and stats */
int vimz_testing_decider_verify_batch_scalars_ex(vimz_ctx* ctx, const uint64_t* key_words, size_t n_key_words, uint32_t len_z, size_t n, const uint64_t* steps,
                                                 const uint64_t* z0, const uint64_t* zi, const uint64_t* words, size_t chunk, const uint64_t* multipliers,
                                                 uint32_t* results, double seconds[6], uint32_t flags, size_t leaf, uint64_t stats[4]);

/* The compressed proof's kernels (vimz_amd/csrc/spartan.hip) on a caller's vectors, through the functions spartan_prove and ipa_prove run for every round
 * (tests/test_gpu_spartan_kernels.py).  field = VIMZ_FIELD_BN254_FR or _FQ, curve = VIMZ_CURVE_BN254_G1 or _GRUMPKIN (anything else: VIMZ_ERR_INVALID); elements are
 * canonical on both sides, 4 words each, points canonical affine, 8 words, the identity as zeros; an element not below its modulus: VIMZ_ERR_INVALID.
 * _eq: table_out[0 .. 2^k) = eq(point, ·), point[0] the top bit of the index, 1 <= k <= 21 (eq_build: k_eq_step level by level).
 * _sumcheck: k rounds over vectors of 2^k elements, 1 <= k <= 21, round j bound at challenges[j] (any field element).  kind = 0, the outer check: vecs = {eq, a, b,
 * c, e}, e NULL for a strict instance; msgs_out: 3 elements a round (the evaluations at 0, 2, 3 of sum eq·(a·b − u·c − e)); finals_out: the 5 bound elements (e's
 * zero when absent).  kind = 1, the inner check: vecs = {m, z}; 2 elements a round (evaluations at 0, 2 of sum m·z); finals_out: 2 elements.
 * _ipa_vec: the vector side of k IPA rounds over a, b of 2^k elements: dots_out 2 elements a round (<a_L,b_R>, <a_R,b_L>), then a' = x·a_L + a_R,
 * b' = b_L + x·b_R at challenges[j]; finals_out: a, b.
 * _fold_bases: out_i = P_i + x·P_(i+half) over 2·half >= 2 points on the curve, x = x128[0] + 2^64·x128[1] (k_ipa_fold_bases). */
int vimz_test_spartan_eq(vimz_ctx* ctx, int field, const uint64_t* point, size_t k, uint64_t* table_out);
int vimz_test_spartan_sumcheck(vimz_ctx* ctx, int field, int kind, size_t k, const uint64_t* const vecs[5], const uint64_t u[4], const uint64_t* challenges,
                               uint64_t* msgs_out, uint64_t* finals_out);
int vimz_test_spartan_ipa_vec(vimz_ctx* ctx, int field, size_t k, const uint64_t* a, const uint64_t* b, const uint64_t* challenges, uint64_t* dots_out,
                              uint64_t finals_out[8]);
int vimz_test_spartan_fold_bases(vimz_ctx* ctx, int curve, const uint64_t* points_xy, size_t half, const uint64_t x128[2], uint64_t* out_xy);
/* spartan_prove for ONE relaxed instance over a caller's R1CS: triplets as vimz_r1cs_upload takes them (canonical values) of n_c >= 2 rows and n_w >= 4 columns over
 * the curve's scalar field; Z: n_w elements (u at wire 0, X0 and X1 at the last two); E: n_c elements, or NULL for a strict instance; ck: a key on `curve` of at least
 * next_pow2(max(n_w, n_c)) points (shorter, or a shape below those sizes: VIMZ_ERR_INVALID).  The forward products are the seam's k_spmv3 / k_spmv_long on the uploaded
 * shape, the transpose build_transpose's, the inner-product generator derive_ipa_u's; W' and E are committed with the library's MSM; the transcript starts from
 * Transcript(label).  buf receives cW, cE (8 words each, cE zeros without E), then the argument's words.  Returns the byte size (copies when cap suffices), or a
 * negative error code.
 * _verify: the product's spartan_verify over the same shape on the caller's instance — inst = cW, cE (8 words each), u, X0, X1 (4 words each) — and argument words
 * (both possibly tampered with).  Returns 1 (accepted), 0 (rejected) or a negative error code. */
int64_t vimz_test_spartan_instance(vimz_ctx* ctx, int curve, size_t n_c, size_t n_w, const vimz_coo* A, const vimz_coo* B, const vimz_coo* C, const uint64_t* Z,
                                   const uint64_t* E, const vimz_bases* ck, const uint64_t digest[4], uint32_t side_tag, const char* label, void* buf, size_t cap);
int vimz_test_spartan_instance_verify(vimz_ctx* ctx, int curve, size_t n_c, size_t n_w, const vimz_coo* A, const vimz_coo* B, const vimz_coo* C, const vimz_bases* ck,
                                      const uint64_t digest[4], uint32_t side_tag, const char* label, const uint64_t inst[28], int has_E, const uint64_t* words,
                                      size_t n_words);
/* The same pair for an instance with n_pub >= 1 public elements at the LAST n_pub wires of Z (wire 0 stays u): 1 <= n_pub <= 8, n_w >= n_pub + 2 (at least one
 * committed wire), anything else VIMZ_ERR_INVALID.  comm_W covers wires 1 .. n_w - 1 - n_pub (wire i over ck[i - 1]); inst = cW, cE (8 words each), u, then
 * X[0 .. n_pub) (4 words each).  At n_pub = 2 every byte is the pair's above (tests/test_gpu_spartan_pub.py). */
int64_t vimz_test_spartan_instance_pub(vimz_ctx* ctx, int curve, size_t n_c, size_t n_w, uint32_t n_pub, const vimz_coo* A, const vimz_coo* B, const vimz_coo* C,
                                       const uint64_t* Z, const uint64_t* E, const vimz_bases* ck, const uint64_t digest[4], uint32_t side_tag, const char* label, void* buf,
                                       size_t cap);
int vimz_test_spartan_instance_pub_verify(vimz_ctx* ctx, int curve, size_t n_c, size_t n_w, uint32_t n_pub, const vimz_coo* A, const vimz_coo* B, const vimz_coo* C,
                                          const vimz_bases* ck, const uint64_t digest[4], uint32_t side_tag, const char* label, const uint64_t* inst, int has_E,
                                          const uint64_t* words, size_t n_words);

/* The batched compressed-proof verifier (vimz_amd/csrc/spartan_batch.hpp) piece by piece (tests/test_gpu_spartan_batch.py).  Elements canonical, 4 words each.
 * _batch_group: members one pass of either kernel serves (a compile-time constant);  _batch_split: the half-table split h.
 * _mat_eval: out[i] = Σ_m w[i][m] Σ_nonzeros value·eq(rx_i, row)·eq(ry_i, col) over the uploaded shape (triplets as vimz_r1cs_upload takes them, n_c, n_w >= 2) for
 * n >= 1 members, rx: n·ceil_log2(n_c) elements, ry: n·ceil_log2(n_w), w: n·3 (k_half_tables, k_mat_eval, k_sum_groups, a group at a time).
 * _svec_accum: n >= 1 openings of `rounds` challenges each (xs, round 0 = the top bit) and a point each; acc_out[j] = Σ_o coefs[o]·s_o[i] over 2^rounds slots,
 * i = j where shifted[o] = 0, (j + 1) mod 2^rounds where it is not; dots_out[o] = <s_o, eq(point_o, ·)> with the entries i == 0 || i + n_pub[o] >= n_w[o] left out
 * where n_w[o] != 0 (k_half_tables, k_svec_accum, k_sum_groups).
 * _instance_batch: n instances over ONE caller's shape, key and digest (as _instance_pub_verify takes one): inst = n × (16 + 4·(1 + n_pub)) words, has_E[i],
 * words[i] / n_words[i] the argument of instance i.  results[i] = what _instance_pub_verify returns for instance i alone (1 accepted, 0 rejected).  chunk as the
 * entry points'.  multipliers: NULL (from the OS) or 2 of 2 words an instance (its W opening's, its E opening's; a zero one: VIMZ_ERR_INVALID).  acc_out
 * (optional): the accumulator of the LAST chunk, next_pow2(max(n_c, n_w)) elements.
 * _batch_scalars: the two entry points with GIVEN multipliers, 6 of 2 words a proof (the openings of its BN254 arguments in order, W before E, then those of its
 * Grumpkin arguments; the unused ones must be non-zero too).  Whoever knows the multipliers can make a chunk of wrong proofs pass.
 * The _ex twins of _instance_batch and _batch_scalars add flags, leaf and stats[4] as the _ex entry points take them (include/vimz_hip.h); acc_out stays the
 * accumulator of the last chunk's FULL equation, not of a subset. */
int vimz_test_spartan_batch_group(void);
int vimz_test_spartan_batch_split(void);
int vimz_test_spartan_mat_eval(vimz_ctx* ctx, int curve, size_t n_c, size_t n_w, const vimz_coo* A, const vimz_coo* B, const vimz_coo* C, size_t n, const uint64_t* rx,
                               const uint64_t* ry, const uint64_t* w, uint64_t* out);
int vimz_test_spartan_svec_accum(vimz_ctx* ctx, int field, uint32_t rounds, size_t n, const uint64_t* xs, const uint64_t* points, const uint64_t* coefs, const uint32_t* shifted,
                                 const uint32_t* n_pub, const uint32_t* n_w, uint64_t* acc_out, uint64_t* dots_out);
int vimz_test_spartan_instance_batch(vimz_ctx* ctx, int curve, size_t n_c, size_t n_w, uint32_t n_pub, const vimz_coo* A, const vimz_coo* B, const vimz_coo* C,
                                     const vimz_bases* ck, const uint64_t digest[4], uint32_t side_tag, const char* label, size_t n, const uint64_t* inst, const int* has_E,
                                     const uint64_t* const* words, const size_t* n_words, size_t chunk, const uint64_t* multipliers, uint32_t* results, double seconds[6],
                                     uint64_t* acc_out);
int vimz_testing_ivc_verify_compressed_batch_scalars(vimz_ivc* vk, size_t n, const uint8_t* const* blobs, const size_t* lens, const uint64_t* steps, const uint64_t* z0,
                                                     size_t chunk, const uint64_t* multipliers, uint32_t* results, double seconds[6]);
int vimz_test_spartan_instance_batch_ex(vimz_ctx* ctx, int curve, size_t n_c, size_t n_w, uint32_t n_pub, const vimz_coo* A, const vimz_coo* B, const vimz_coo* C,
                                        const vimz_bases* ck, const uint64_t digest[4], uint32_t side_tag, const char* label, size_t n, const uint64_t* inst, const int* has_E,
                                        const uint64_t* const* words, const size_t* n_words, size_t chunk, const uint64_t* multipliers, uint32_t* results, double seconds[6],
                                        uint64_t* acc_out, uint32_t flags, size_t leaf, uint64_t stats[4]);
int vimz_testing_ivc_verify_batch_compressed_scalars_ex(vimz_ivc* vk, size_t n, const uint8_t* const* blobs, const size_t* lens, const uint64_t* steps, const uint64_t* z0,
                                                        size_t chunk, const uint64_t* multipliers, uint32_t* results, double seconds[6], uint32_t flags, size_t leaf,
                                                        uint64_t stats[4]);
int vimz_testing_cf_verify_batch_compressed_scalars_ex(vimz_cf* vk, size_t n, const uint8_t* const* blobs, const size_t* lens, const uint64_t* steps, const uint64_t* z0,
                                                       size_t chunk, const uint64_t* multipliers, uint32_t* results, double seconds[6], uint32_t flags, size_t leaf,
                                                       uint64_t stats[4]);
int vimz_testing_cf_verify_compressed_batch_scalars(vimz_cf* vk, size_t n, const uint8_t* const* blobs, const size_t* lens, const uint64_t* steps, const uint64_t* z0,
                                                    size_t chunk, const uint64_t* multipliers, uint32_t* results, double seconds[6]);
int vimz_test_spartan_instance_batch_ex(vimz_ctx* ctx, int curve, size_t n_c, size_t n_w, uint32_t n_pub, const vimz_coo* A, const vimz_coo* B, const vimz_coo* C,
                                        const vimz_bases* ck, const uint64_t digest[4], uint32_t side_tag, const char* label, size_t n, const uint64_t* inst, const int* has_E,
                                        const uint64_t* const* words, const size_t* n_words, size_t chunk, const uint64_t* multipliers, uint32_t* results, double seconds[6],
                                        uint64_t* acc_out, uint32_t flags, size_t leaf, uint64_t stats[4]);
int vimz_testing_ivc_verify_batch_compressed_scalars_ex(vimz_ivc* vk, size_t n, const uint8_t* const* blobs, const size_t* lens, const uint64_t* steps, const uint64_t* z0,
                                                        size_t chunk, const uint64_t* multipliers, uint32_t* results, double seconds[6], uint32_t flags, size_t leaf,
                                                        uint64_t stats[4]);
int vimz_testing_cf_verify_batch_compressed_scalars_ex(vimz_cf* vk, size_t n, const uint8_t* const* blobs, const size_t* lens, const uint64_t* steps, const uint64_t* z0,
                                                       size_t chunk, const uint64_t* multipliers, uint32_t* results, double seconds[6], uint32_t flags, size_t leaf,
                                                       uint64_t stats[4]);

/* The device's square root over Fq2 (vimz_amd/csrc/g16_point_pack.hpp: fq2_sqrt), one thread per value (tests/test_gpu_point_pack.py): values: n elements of Fq2,
 * c0 then c1, canonical, 4 words each (one not below q: VIMZ_ERR_INVALID); roots_out: the same layout, is_square_out[i] = 1 when roots_out[i] squares to values[i],
 * 0 when values[i] is no square (the root is then unspecified).  Reaches the branch for c1 = 0, which no curve point one can craft cheaply takes.  1 <= n <= 2^20. */
int vimz_test_fq2_sqrt(vimz_ctx* ctx, const uint64_t* values, size_t n, uint64_t* roots_out, uint32_t* is_square_out);

/* The multilinear KZG opening's kernels (vimz_amd/csrc/mlkzg.hip) on a caller's vectors (tests/test_gpu_mlkzg_kernels.py).  Elements are canonical, 4 words each,
 * below r (else VIMZ_ERR_INVALID); sizes up to 2^20.  The levels of a polynomial of n0 coefficients lie side by side, level k with n0 >> k elements.
 *   shape    out = {threads of a block, coefficients of one thread}: the sizes at which the evaluation and the division change path
 *   fold     k_mle_fold logn times over vec (2^logn elements) at point: levels_out receives all logn + 1 levels, 2^(logn+1) - 1 elements
 *   eval3    k_poly_eval3 + k_eval3_sum over nlevels levels (n0 >> (nlevels - 1) >= 1): evals_out[u·nlevels + k] = P_k at r, -r, r² for u = 0, 1, 2
 *   batch    k_batch_levels: out[j] = Σ_{k: j < n0 >> k} q^k·P_k[j], n0 elements
 *   divide   the three launches of the division of n coefficients by (X - u_j), j < 3: quot_out[j·(n-1) ..] the n - 1 quotient coefficients, rem_out[j] the
 *            remainder, and what the first and the second launch leave, ceil(n / coefficients of a thread) elements a row (optional): carry_out each chunk's
 *            carry-out with a zero carry-in, carry_in_out the carry into each chunk
 *   chains   host only: label, then (tag, n bytes of data) absorbed and a challenge drawn, twice over, by proof_io.hpp's Transcript (out[0..2)) and by
 *            mlkzg_verify.hpp's restatement of it (out[2..4)): the 128-bit challenges of the last round, or of the first round in which they differ */
int vimz_test_mlkzg_chains(const char* label, const char* tag, const uint8_t* data, size_t n, uint64_t out[4]);
int vimz_test_mlkzg_shape(uint32_t out[2]);
int vimz_test_mlkzg_fold(vimz_ctx* ctx, const uint64_t* vec, uint32_t logn, const uint64_t* point, uint64_t* levels_out);
int vimz_test_mlkzg_eval3(vimz_ctx* ctx, const uint64_t* levels, size_t n0, uint32_t nlevels, const uint64_t r[4], uint64_t* evals_out);
int vimz_test_mlkzg_batch(vimz_ctx* ctx, const uint64_t* levels, size_t n0, uint32_t nlevels, const uint64_t q[4], uint64_t* out);
int vimz_test_mlkzg_divide(vimz_ctx* ctx, const uint64_t* coeffs, size_t n, const uint64_t u[12], uint64_t* quot_out, uint64_t rem_out[12], uint64_t* carry_out,
                           uint64_t* carry_in_out);

#ifdef __cplusplus
}
#endif
#endif
