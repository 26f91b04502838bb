/* vimz_hip.h — C ABI of the MI355X (gfx950) Nova-folding accelerator for VIMz.
 *
 * This is the drop-in boundary: the entry points a patched nova-snark 0.23.0 / nova-scotia 0.5.0 would
 * bind over FFI in place of its CPU arithmetic (INTEGRATION.md shows the Rust stubs).
 * The reference has no FFI seam today — the seam is cut inside the third-party crates reached from
 *   vimz/src/nova_snark_backend/folding.rs:22-23  (load_r1cs, create_public_params)
 *   vimz/src/nova_snark_backend/folding.rs:35-41  (create_recursive_circuit -> RecursiveSNARK::prove_step)
 *   vimz/src/nova_snark_backend/folding.rs:53-55  (RecursiveSNARK::verify)
 * Each function below names the crate interface it replaces.
 *
 * Conventions
 *  - Plain C: opaque handles, pointers and sizes.  No C++/torch types cross this boundary.
 *  - A field element is 4 x uint64_t little-endian limbs (32 bytes).  `form` says whether a buffer holds
 *    canonical integers (VIMZ_FORM_CANONICAL, what .r1cs/.wtns/JSON carry) or Montgomery residues with
 *    R = 2^256 (VIMZ_FORM_MONTGOMERY, the in-memory layout of halo2curves / pasta_curves field types, so
 *    Rust slices can be passed without conversion).
 *  - An affine point is {x, y} = 8 limbs (64 bytes); the identity is (0, 0).
 *  - The caller owns every host buffer; the library owns device memory behind handles (explicit *_free).
 *  - Every function returns VIMZ_OK (0) or a negative error code and never throws or aborts;
 *    vimz_last_error() returns a description for the calling context.
 *  - One vimz_ctx per GPU.  Entry points are thread-safe (serialised per context); work is issued on the
 *    context's own HIP stream.
 *  - Results are exact field / group elements: outputs are bit-identical to the CPU reference.
 */
#ifndef VIMZ_HIP_H
#define VIMZ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VIMZ_OK 0
#define VIMZ_ERR_INVALID (-1)  /* bad argument */
#define VIMZ_ERR_HIP (-2)      /* HIP runtime failure (see vimz_last_error) */
#define VIMZ_ERR_NO_DEVICE (-3)/* no gfx950 device / extension cannot run */
#define VIMZ_ERR_UNSAT (-4)    /* witness does not satisfy the step relation */

#define VIMZ_FORM_CANONICAL 0
#define VIMZ_FORM_MONTGOMERY 1

/* curves: coordinate field / scalar field */
#define VIMZ_CURVE_BN254_G1 0 /* Fq / Fr : primary curve of the reference (nova_snark_backend/mod.rs:19) */
#define VIMZ_CURVE_GRUMPKIN 1 /* Fr / Fq : secondary curve (nova_snark_backend/mod.rs:20) */
#define VIMZ_CURVE_PALLAS 2
#define VIMZ_CURVE_VESTA 3

#define VIMZ_FIELD_BN254_FR 0
#define VIMZ_FIELD_BN254_FQ 1
#define VIMZ_FIELD_PALLAS_FP 2
#define VIMZ_FIELD_VESTA_FQ 3

typedef struct vimz_ctx vimz_ctx;
typedef struct vimz_bases vimz_bases; /* commitment key resident in HBM */
typedef struct vimz_vec vimz_vec;     /* vector of field elements resident in HBM (Montgomery form) */

/* ---- context ------------------------------------------------------------------------------------- */
int vimz_ctx_create(int device, vimz_ctx** out);
void vimz_ctx_destroy(vimz_ctx* ctx);
const char* vimz_last_error(const vimz_ctx* ctx);
const char* vimz_version(void);
/* name: caller buffer; cus / hbm_bytes may be NULL */
int vimz_device_info(vimz_ctx* ctx, char* name, size_t name_len, int* cus, uint64_t* hbm_bytes);
int vimz_sync(vimz_ctx* ctx);

/* A marker for a profiler's kernel trace: an empty kernel `k_trace_marker` of `id` (1..1024) workgroups on the context's stream, waited for
 * (bench.py brackets its timed region with ids 1 and 2; tools/trace_busy.py cuts the trace there). */
int vimz_trace_marker(vimz_ctx* ctx, int id);
/* Rows of a short fold call whose Poseidon chains are evaluated on the host (the "head batch"; the proof is bit-identical either way): rows >= 0 pins
 * the number for every later call of this process (0: every row's witness entirely on the GPU), -1 restores the library's policy (24 for calls of at
 * most 24 rows — for the segments of one proof: proofs of at most 28 rows in all — on six or more host cores, else 0).  Returns the previous setting. */
long vimz_set_head_rows(long rows);
/* Row groups of the batch producer: the most rows of a batch whose witness commitments (and S_1 sums) are issued as ONE chain of kernel launches, the row in a
 * grid dimension (the proof is bit-identical whatever the value): rows >= 0 pins it for every later call of this process (0 or 1: one chain per row; at most 16),
 * -1 restores the default (4, or VIMZ_TUNE's rows_group).  Returns the previous setting. */
long vimz_set_rows_group(long rows);
/* A fingerprint of the host a benchmark line was measured on: out[0] = µs per Poseidon permutation (t = 9) on one host core, out[1] = µs per
 * empty kernel launch + stream synchronise (median of 200), out[2] = host cores this process may use, out[3] = µs per event record + synchronise. */
int vimz_host_fingerprint(vimz_ctx* ctx, double out[4]);
/* Stream-ordered timing with HIP events on the context's stream (used by bench.py for the roofline). */
int vimz_timer_start(vimz_ctx* ctx);
int vimz_timer_stop(vimz_ctx* ctx, float* ms_out);
/* When enabled, vimz_msm* record per-kernel HIP-event durations, readable with vimz_msm_last_profile. */
int vimz_set_profiling(vimz_ctx* ctx, int enabled);
/* ms[6] = {hist, scan, scatter, accumulate, combine, reduce}; info[4] = {window bits, windows, sub-buckets, entries} */
int vimz_msm_last_profile(vimz_ctx* ctx, float ms[6], uint32_t info[4]);
/* sums over every profiled MSM of the context since the last reset (the large MSM(T) launches of a fold, on the stream they run on):
 * ms[6] as above; counts[3] = {MSM calls, points, bucket entries (= mixed additions)} */
int vimz_msm_profile_totals(vimz_ctx* ctx, double ms[6], uint64_t counts[3], int reset);

/* ---- commitment key (replaces the `ck: Vec<G::PreprocessedGroupElement>` of nova-snark's
 *      CommitmentKey, built by PublicParams::setup reached from folding.rs:23) ------------------------- */
int vimz_bases_upload(vimz_ctx* ctx, int curve, const uint64_t* xy, size_t n, int form, vimz_bases** out);
/* Derive n generators on the GPU: ck_i = try-and-increment(SHAKE256(label || LE64(i) || LE32(ctr))), see
 * vimz_amd/csrc/ckgen.hpp (the role of nova-snark's `CommitmentKey::setup(b"ck", n)`; not byte-compatible with it). */
int vimz_bases_generate(vimz_ctx* ctx, int curve, const char* label, size_t label_len, size_t n, vimz_bases** out);
int vimz_bases_download(vimz_ctx* ctx, const vimz_bases* b, size_t offset, uint64_t* xy, size_t n, int form);
/* Precompute window tables T_j[i] = 2^(window_bits*j) * P_i (window_bits 0 -> 16; K x the key's footprint in HBM).  The key
 * is fixed for a whole proof, so every later MSM over it (with window_bits = 0) uses them:
 *   window_bits 12..16: ONE bucket set shared by all windows — fewer digits per scalar, one bucket reduction, no Horner;
 *   window_bits 11 (the window a large MSM uses anyway): the usual per-window bucket sets, whose sums the host then only adds
 *   (no Horner: ~0.1 ms less on the host per MSM).  MSMs too small for that window ignore such tables.
 *   window_bits 7 (keys of at most 30720 points): EVERY multiple m·2^(7w)·P_i, m = 1..64 (189 KB per point): a digit selects its point,
 *   the MSM is one sum without buckets — what the per-step commitments over the verifier circuits' fixed key slices use.
 * Results are unchanged. */
int vimz_bases_precompute(vimz_ctx* ctx, vimz_bases* b, int window_bits);
size_t vimz_bases_len(const vimz_bases* b);
void vimz_bases_free(vimz_ctx* ctx, vimz_bases* b);

/* ---- input pipeline: pixel packing on the device (replaces pyvimz's compress_by_rows / compress_by_blocks,
 *      pyvimz/pyvimz/img/ops.py:4-70, whose hex strings `VIMzInput` carries, vimz/src/input.rs:9-62).  pixels: height x width x
 *      channels bytes (channels 3 = RGB, 1 = grey).  block = 0: one output row of ceil(width/10) elements per image row;
 *      block = 40: 40 x 40 blocks of 160 elements, blocks row-major (the redact input).  out: vimz_pack_count(...) canonical
 *      elements (4 x u64 each). ---------------------------------------------------------------------------------------------- */
size_t vimz_pack_count(size_t height, size_t width, int block);
int vimz_pack_pixels(vimz_ctx* ctx, const uint8_t* pixels, size_t height, size_t width, int channels, int block, uint64_t* out);

/* ---- image hashes: the running Poseidon hash the circuits keep of an image (circuits/src/utils/hashers.circom,
 *      image_running_hash.circom; what pyvimz's image-hasher writes to marketplace/image-data/ .hash files and what a proof's final
 *      state holds in z_n[0] / z_n[1]).  Per unit (a row, or a block x block square) d = ArrayHasher(L)(unit elements); then
 *      acc_0 = 0, acc_{i+1} = PairHasher(acc_i, d_i), or PairHasher(acc_i, 0) for a unit whose `drop` flag is set (redact's target).
 *      Units are packed as vimz_pack_pixels packs them.  The unit digests of all n images go to the GPU in one launch; the serial
 *      chain over them runs on the host, one image per thread.  out: n hashes, canonical (4 x u64 each). ---------------------- */
typedef struct {
  const uint8_t* pixels;      /* height x width x channels bytes; channels 1 (grey, in the R slot), 3 (RGB) or 4 (RGBA, alpha ignored) ... */
  size_t height, width;
  int channels;
  const uint64_t* units;      /* ... or, pixels == NULL: n_units x unit_len pre-packed canonical elements (each below the modulus) */
  size_t n_units, unit_len;
  int block;                  /* 0: row-wise; 40: 40 x 40 blocks as vimz_pack_pixels(block = 40) (redact).  0 for pre-packed units */
  size_t max_units;           /* 0: every unit; else only the first max_units rows / blocks (at most as many as the image has) */
  const uint8_t* drop;        /* optional, one flag per hashed unit: nonzero -> that unit's digest is replaced by 0 */
} vimz_image_desc;
int vimz_image_hash(vimz_ctx* ctx, const vimz_image_desc* imgs, size_t n, uint64_t* out);
/* wall-clock milliseconds of the context's last vimz_image_hash: ms[0] the digests (uploads, kernel, download), ms[1] the host chains */
int vimz_image_hash_last_profile(vimz_ctx* ctx, double ms[2]);

/* ---- image edits: pyvimz's image-editor transformations (pyvimz/pyvimz/img/transformations.py, restated bit-exactly by
 *      vimz_amd/image_editor.py) on the device, with the packing of the prover's input fused in.  One call runs n edit descriptors in
 *      order on the context's stream; a descriptor's source is host pixels or the edited image of an earlier descriptor of the same call
 *      (which stays on the device).  Outputs, each optional:
 *        out_pixels  the edited image, height x width x channels bytes as vimz_image_edit_shapes reports them
 *        out_source  the source packed as vimz_amd.image_editor.build_input's "original": rows of ceil(width/10) elements; blur and
 *                    sharpness add one zero row above and one below; redact packs 40 x 40 blocks (height and width multiples of 40)
 *        out_target  the edited image packed as build_input's "transformed" (rows, or blocks for redact; none for VIMZ_EDIT_HASH)
 *      Packed elements are canonical, 4 x u64 each.  Sources of 4 channels have their alpha ignored; an RGB edit of them has 3 channels.
 *      Grey sources (1 channel) are accepted by hash, crop and redact only. ---------------------------------------------------- */
#define VIMZ_EDIT_HASH 0        /* no edit: the source's packing (and a copy of its pixels) */
#define VIMZ_EDIT_GRAYSCALE 1   /* (19595 R + 38470 G + 7471 B + 32768) >> 16, one channel */
#define VIMZ_EDIT_BRIGHTNESS 2  /* clip(c * factor, 0, 255) truncated, in float64 */
#define VIMZ_EDIT_CONTRAST 3    /* clip((c - 128.0) * factor + 128.0, 0, 255) truncated, in float64 */
#define VIMZ_EDIT_BLUR 4        /* 3 x 3 box, zero padding, sum / 9 */
#define VIMZ_EDIT_SHARPNESS 5   /* 5c - up - down - left - right, zero padding, clamped */
#define VIMZ_EDIT_RESIZE 6      /* to new_width x new_height: image_editor.resize_image's float64 interpolation */
#define VIMZ_EDIT_CROP 7        /* the new_width x new_height window at (x, y), inside the image */
#define VIMZ_EDIT_REDACT 8      /* zero the flagged full 40 x 40 blocks */
typedef struct {
  int op;                     /* VIMZ_EDIT_* */
  const uint8_t* pixels;      /* the source: height x width x channels bytes (channels 1, 3 or 4) ... */
  size_t height, width;
  int channels;
  int64_t source;             /* ... or, pixels == NULL: the index of an earlier descriptor of the call, whose edited image is the source */
  double factor;              /* brightness, contrast (finite) */
  size_t x, y;                /* crop: the window's top-left corner */
  size_t new_width, new_height;     /* crop: the window's size; resize: the target size */
  const uint8_t* redact;      /* redact: NULL (with n_redact = 0) for pyvimz's checkerboard (block (by, bx) when by + bx is odd), or one flag per
                                 full block, row-major (non-NULL even when there are no full blocks) */
  size_t n_redact;            /* the number of flags: (height / 40) * (width / 40); any other count is refused, 0 included */
  uint8_t* out_pixels;        /* optional outputs (NULL: not wanted), sized by vimz_image_edit_shapes */
  uint64_t* out_source;
  uint64_t* out_target;
} vimz_edit_desc;
typedef struct {
  size_t height, width;       /* the edited image */
  int channels;               /* 1 or 3 */
  size_t source_units, source_unit_len;     /* out_source: source_units x source_unit_len elements (rows, or 40 x 40 blocks of 160) */
  size_t target_units, target_unit_len;     /* out_target (0 x 0 for hash) */
} vimz_edit_shape;
/* n: 1 to 4096 descriptors per call (VIMZ_ERR_INVALID otherwise) */
#define VIMZ_EDIT_MAX_DESCS 4096
/* checks the n descriptors as vimz_image_edit does (their outputs may be NULL) and writes each one's shapes to out[i] */
int vimz_image_edit_shapes(vimz_ctx* ctx, const vimz_edit_desc* descs, size_t n, vimz_edit_shape* out);
int vimz_image_edit(vimz_ctx* ctx, const vimz_edit_desc* descs, size_t n);
/* wall-clock milliseconds of the context's last vimz_image_edit: ms[0] uploads, ms[1] the kernels, ms[2] downloads */
int vimz_image_edit_last_profile(vimz_ctx* ctx, double ms[3]);

/* ---- device vectors -------------------------------------------------------------------------------- */
int vimz_vec_alloc(vimz_ctx* ctx, int field, size_t n, vimz_vec** out); /* zero-filled */
int vimz_vec_upload(vimz_ctx* ctx, vimz_vec* v, size_t offset, const uint64_t* host, size_t n, int form);
int vimz_vec_download(vimz_ctx* ctx, const vimz_vec* v, size_t offset, uint64_t* host, size_t n, int form);
size_t vimz_vec_len(const vimz_vec* v);
void vimz_vec_free(vimz_ctx* ctx, vimz_vec* v);

/* ---- MSM: replaces `G::vartime_multiscalar_mul(scalars, bases)` behind `CE::commit(ck, v)`
 *      (nova-snark 0.23.0 provider).  Computes sum_i scalars[i] * bases[i]
 *      over the first n bases.  window_bits = 0 lets the library choose.  out_xy: affine, `out_form`. ---- */
int vimz_msm(vimz_ctx* ctx, const vimz_bases* bases, const uint64_t* scalars, size_t n, int form,
             int window_bits, uint64_t out_xy[8], int out_form);
/* same, scalars already resident: elements [offset, offset+n) of v against bases [base_offset, base_offset+n) */
int vimz_msm_vec(vimz_ctx* ctx, const vimz_bases* bases, size_t base_offset, const vimz_vec* v, size_t offset,
                 size_t n, int window_bits, uint64_t out_xy[8], int out_form);

/* flags: VIMZ_MSM_SPLIT_ONES sums the bases of unit scalars with a dedicated tree kernel instead of the bucket sort
 * (witness vectors are ~80 % bits); the result is identical. */
#define VIMZ_MSM_SPLIT_ONES 1
int vimz_msm_vec_ex(vimz_ctx* ctx, const vimz_bases* bases, size_t base_offset, const vimz_vec* v, size_t offset,
                    size_t n, int window_bits, int flags, uint64_t out_xy[8], int out_form);

/* ---- sparse R1CS mat-vec and the cross-term commitment for a CALLER-SUPPLIED shape (SURVEY.md §8b seam 2): replaces
 *      `R1CSShape::multiply_vec(&self, z) -> (Az, Bz, Cz)` and `R1CSShape::commit_T(ck, U1, W1, U2, W2) -> (T, comm_T)` of
 *      nova-snark 0.23.0, reached from NIFS::prove / is_sat* inside RecursiveSNARK::{prove_step, verify}
 *      (vimz/src/nova_snark_backend/folding.rs:35-41, 53-55).  The matrices are handed over as nova-snark holds them: three lists
 *      of (row, col, value) triplets, in any order; they stay resident behind the handle (CSR + coefficient dictionary). ------- */
typedef struct vimz_r1cs vimz_r1cs;
typedef struct { const uint32_t* row; const uint32_t* col; const uint64_t* val /* nnz x 4 limbs */; size_t nnz; } vimz_coo;
/* field: the shape's scalar field (VIMZ_FIELD_*); ncols = length of z = [W, u, X] as the caller orders it */
int vimz_r1cs_upload(vimz_ctx* ctx, int field, size_t nrows, size_t ncols, const vimz_coo* A, const vimz_coo* B, const vimz_coo* C, int form,
                     vimz_r1cs** out);
void vimz_r1cs_free(vimz_ctx* ctx, vimz_r1cs* shape);
/* info = {rows, cols, nnz A, nnz B, nnz C, distinct coefficients, long rows, field} */
int vimz_r1cs_info(const vimz_r1cs* shape, uint64_t info[8]);
/* (Az, Bz, Cz) = (A, B, C)·z; every vector a vimz_vec of the shape's field (z: >= ncols elements, outputs: >= nrows) */
int vimz_spmv3(vimz_ctx* ctx, const vimz_r1cs* shape, const vimz_vec* z, vimz_vec* az, vimz_vec* bz, vimz_vec* cz);
/* T = AZ1∘BZ2 + AZ2∘BZ1 − u1·CZ2 − u2·CZ1 (written to T_out, nrows elements) and comm_T = Σ T_i·ck_i (affine, out_form).
 * z1 / z2: the full assignment vectors of the two instances (running and fresh); u1 / u2: their relaxation scalars in `form`
 * (u2 = 1 for a fresh instance).  ck: at least nrows generators on the curve whose scalar field is the shape's field. */
int vimz_commit_T(vimz_ctx* ctx, const vimz_r1cs* shape, const vimz_bases* ck, const vimz_vec* z1, const uint64_t u1[4], const vimz_vec* z2,
                  const uint64_t u2[4], int form, vimz_vec* T_out, uint64_t comm_T[8], int out_form);
/* R1CSShape::is_sat_relaxed for a resident assignment z = [W, u-slot, X] with relaxation scalar u (in `form`) and error vector E (NULL = 0):
 * bad_rows = number of rows with (A·z)∘(B·z) != u·(C·z) + E, first_bad = the first of them (all ones if none).  nova-snark 0.23.0,
 * reached from RecursiveSNARK::verify (folding.rs:53-55). */
int vimz_r1cs_check_relaxed(vimz_ctx* ctx, const vimz_r1cs* shape, const vimz_vec* z, const uint64_t u[4], int form, const vimz_vec* E,
                            uint64_t* bad_rows, uint64_t* first_bad);
/* x1 <- x1 + r * x2 over the first n elements (r in `form`): the fold of a resident vector — RelaxedR1CSWitness::fold for W and E,
 * nova-snark 0.23.0 (reached from NIFS::prove, folding.rs:35-41).  Both vectors of the same field, x1 != x2. */
int vimz_vec_axpy(vimz_ctx* ctx, vimz_vec* x1, const uint64_t r[4], int form, const vimz_vec* x2, size_t n);

/* ---- step circuits: R1CS shape + witness program (replaces the `.r1cs` that nova_scotia::circom::reader::load_r1cs
 *      reads at vimz/src/nova_snark_backend/folding.rs:22 and the circom witness generator named by
 *      Config::witness_generator_file(), folding.rs:36).  Host-only: usable without a GPU. -------------------- */
typedef struct vimz_circuit vimz_circuit;
/* (all nine step circuits, crop included, have GPU witness programs; circuits loaded from an .r1cs have none and are folded from
 * supplied witnesses with vimz_prover_fold_witness / vimz_ivc_fold_witness.)
 * transformation ids follow the reference's enum order (vimz/src/transformation.rs:7-18) */
#define VIMZ_T_BLUR 0
#define VIMZ_T_BRIGHTNESS 1
#define VIMZ_T_CONTRAST 2
#define VIMZ_T_CROP 3
#define VIMZ_T_GRAYSCALE 4
#define VIMZ_T_HASH 5
#define VIMZ_T_REDACT 6
#define VIMZ_T_RESIZE 7
#define VIMZ_T_SHARPNESS 8
/* width = packed elements per original row (128 HD / 384 4K / 768 8K; 160 for redact blocks);
 * width2 / rows_in / rows_out: resize geometry (64,3,2 at HD; w/2,2,1 at 4K/8K); crop_height: crop only. */
int vimz_circuit_build(int transformation, int width, int width2, int rows_in, int rows_out, int crop_height,
                       vimz_circuit** out);
void vimz_circuit_free(vimz_circuit* c);
const char* vimz_circuit_last_error(void);
/* iden3 binary formats: load a circom-built `.r1cs` (BN254 Fr, as many public outputs as inputs — a Nova step circuit), and
 * read a `.wtns`.  A loaded circuit has no witness program; fold it with vimz_prover_fold_witness. */
int vimz_circuit_load_r1cs(const uint8_t* data, size_t len, vimz_circuit** out);
int vimz_wtns_load(const uint8_t* data, size_t len, uint64_t* out, size_t cap_elems, size_t* n_out);
#define VIMZ_CIRCUIT_INFO_LEN 16
/* info = {wires, constraints (incl. linear), linear constraints, len_z, private inputs, nnz A, nnz B, nnz C,
 *         dictionary size, decomposition groups, lane groups, lane instructions, lane rows, hash jobs, chains, field ops} */
/* Optional, host only: synthesises ahead of time what vimz_ivc_create needs of this circuit — the augmented primary circuit (the step circuit with Nova's
 * verifier circuit appended, nova-snark's `circuit_primary` of `PublicParams::setup`, reached from vimz/src/nova_snark_backend/folding.rs:20-25) and its digest —
 * and keeps it with the circuit object; the IVCs of a proof made as several segments then share one synthesis.  Call it on the thread that built the circuit. */
int vimz_circuit_prepare_ivc(const vimz_circuit* c);
int vimz_circuit_info(const vimz_circuit* c, uint64_t info[VIMZ_CIRCUIT_INFO_LEN]);
/* raw tables (CSR of A,B,C with a coefficient dictionary; witness-program tables of vimz_amd/csrc/circuit/program.hpp) */
#define VIMZ_CX_A_ROWPTR 0
#define VIMZ_CX_A_COL 1
#define VIMZ_CX_A_COEF 2
#define VIMZ_CX_B_ROWPTR 3
#define VIMZ_CX_B_COL 4
#define VIMZ_CX_B_COEF 5
#define VIMZ_CX_C_ROWPTR 6
#define VIMZ_CX_C_COL 7
#define VIMZ_CX_C_COEF 8
#define VIMZ_CX_DICT_MONT 9
#define VIMZ_CX_DICT_CANON 10
#define VIMZ_CX_DECOMP 11
#define VIMZ_CX_LANE_GROUPS 12
#define VIMZ_CX_LANE_INSTR 13
#define VIMZ_CX_LANE_ROWS 14
#define VIMZ_CX_JOBS 15
#define VIMZ_CX_CHAINS 16
#define VIMZ_CX_FOPS 17
#define VIMZ_CX_ZOUT 18
#define VIMZ_CX_LC_TERMS 19
/* returns the table's size in bytes (copies it when buf != NULL and cap is large enough), negative on error */
int64_t vimz_circuit_export(const vimz_circuit* c, int what, void* buf, size_t cap);

/* ---- folding prover: the body of `fold_input` (vimz/src/nova_snark_backend/folding.rs:27-43), i.e. the per-row loop of
 *      nova_scotia::create_recursive_circuit around nova-snark's RecursiveSNARK::prove_step, with W, E and the running
 *      (A,B,C)·Z resident in HBM.  This is the NIFS *accumulator* over the step circuit's own instances, X = (z_{i+1}, z_i):
 *      accumulators of different row segments merge (vimz_prover_merge), which is the multi-GPU sharding of BASELINE.json's
 *      north_star.  RecursiveSNARK::prove_step in full — augmented verifier circuits on both curves — is vimz_ivc_* below. ------------------------ */
typedef struct vimz_prover vimz_prover;
/* ck must be on BN254 G1 with at least max(wires, constraints) generators; max_batch = rows whose witnesses are
 * generated together (memory: max_batch * wires * 32 bytes). */
int vimz_prover_create(vimz_ctx* ctx, const vimz_circuit* circuit, const vimz_bases* ck, size_t max_batch, vimz_prover** out);
void vimz_prover_free(vimz_prover* p);
/* z0: len_z canonical elements (Transformation::ivc_initial_state, vimz/src/transformation.rs:25-40) */
int vimz_prover_reset(vimz_prover* p, const uint64_t* z0);
/* step_inputs: nsteps x private-input-count canonical elements in the per-step order of
 * vimz/src/nova_snark_backend/input.rs:57-96.  Returns VIMZ_ERR_UNSAT if a row violates the step relation. */
int vimz_prover_fold(vimz_prover* p, const uint64_t* step_inputs, size_t nsteps);
/* Same fold, but the witnesses come from outside (circom's generator): witnesses = nsteps x wires canonical elements in
 * iden3 wire order; step i's public inputs must equal step i-1's public outputs (checked). */
int vimz_prover_fold_witness(vimz_prover* p, const uint64_t* witnesses, size_t nsteps);
/* verify_folded_proof (folding.rs:45-56): 0 = accepted; bit0 relation, bit1 comm_W, bit2 comm_E, bit3 running products */
int vimz_prover_verify(vimz_prover* p, uint32_t* result);
int vimz_prover_instance(vimz_prover* p, uint64_t comm_W[8], uint64_t comm_E[8], uint64_t u[4], uint64_t* z_current, uint64_t* steps);
int vimz_prover_running(vimz_prover* p, uint64_t* z_run, uint64_t* E);
/* IVC state chain only: zs_out = (nsteps+1) x len_z canonical elements starting at z_start (one hash-only GPU pass over the
 * rows + the host pair-hash chain).  Lets a multi-GPU driver find the state at which each row segment starts. */
int vimz_prover_state_chain(vimz_prover* p, const uint64_t* z_start, const uint64_t* step_inputs, size_t nsteps, uint64_t* zs_out);
/* The chain in its two parts, for proofs sharded over GPUs: (1) the ROW DIGESTS (the state-independent row hashes: the expensive part,
 * one GPU pass) of any run of rows — every rank hashes its own rows side by side —, (2) the serial chain over rows whose digests are
 * known (host only, ≈ 12-25 µs per row).  stride = elements per row of the digests (opaque Montgomery limbs); 0 for a circuit whose
 * digests depend on the state (crop): use vimz_prover_state_chain there. */
size_t vimz_prover_digest_stride(const vimz_prover* p);
int vimz_prover_row_digests(vimz_prover* p, const uint64_t* step_inputs, size_t nsteps, uint64_t* digests_out /* nsteps x stride x 4 */);
int vimz_prover_chain_from_digests(vimz_prover* p, const uint64_t* z_start, const uint64_t* step_inputs, const uint64_t* digests, size_t nsteps, uint64_t* zs_out);
/* Host-side final fold of row segments folded on different GPUs (north_star: "host-side sequential final fold"):
 * export one prover's running relaxed instance as a byte blob, merge it into another's (NIFS for two relaxed instances). */
size_t vimz_prover_export_size(const vimz_prover* p);
int vimz_prover_export(vimz_prover* p, uint8_t* blob, size_t cap);
int vimz_prover_merge(vimz_prover* p, const uint8_t* blob, size_t len);
/* the same final fold between two provers on the same GPU (segments folded concurrently on one device), no host copy */
int vimz_prover_merge_prover(vimz_prover* p, vimz_prover* src);
/* seconds[9]/counts[9]: witness, state chain (host), spmv, msm(W), cross term, msm(T), RO (host), fold, host EC */
int vimz_prover_profile(const vimz_prover* p, double seconds[9], uint64_t counts[9]);
/* parity hooks: GPU witness generation alone (replaces the circom witness generator process) and
 * the GPU sparse mat-vec alone (R1CSShape::multiply_vec; row V1).  All buffers canonical. */
int vimz_prover_witness(vimz_prover* p, const uint64_t* inputs, size_t rows, uint64_t* z_wires_out, uint64_t* zs_out, uint32_t* status_out);
int vimz_prover_spmv(vimz_prover* p, const uint64_t* z, uint64_t* az, uint64_t* bz, uint64_t* cz);

/* ---- Nova IVC: RecursiveSNARK::{new, prove_step, verify} in full, with the augmented verifier circuits on the
 *      BN254 / Grumpkin cycle (reference entry vimz/src/nova_snark_backend/folding.rs:27-56,
 *      curves nova_snark_backend/mod.rs:19-20).  nova-snark 0.23.0's own circuit is not vendored: the circuits here
 *      (vimz_amd/csrc/aug/) state the same relation — see DESIGN.md §5 — and are NOT byte-compatible with its proof object.
 *
 *      Per step: the step circuit's witness / commitment / (A,B,C)·z come from the batch producer exactly as in
 *      vimz_prover_fold; the verifier circuit's ~7.6 k wires are computed on the host (as in the reference), committed and
 *      multiplied on the GPU; the secondary circuit (7.6 k constraints over BN254 Fq, commitments on Grumpkin) is folded on
 *      the GPU with the same kernels instantiated for that field/curve. ---------------------------------------------------- */
typedef struct vimz_ivc vimz_ivc;
/* ck_primary on BN254 G1 (>= max(wires, constraints) of the augmented step circuit), ck_secondary on Grumpkin (>= 8192). */
int vimz_ivc_create(vimz_ctx* ctx, const vimz_circuit* step_circuit, const vimz_bases* ck_primary, const vimz_bases* ck_secondary,
                    size_t max_batch, vimz_ivc** out);
void vimz_ivc_free(vimz_ivc* v);
int vimz_ivc_reset(vimz_ivc* v, const uint64_t* z0);
/* One proof on several GPUs: every step's large cross-term commitment MSM(T) is split by base range between this
 * IVC's GPU and the registered helpers (at most 7); each returns one partial point, the host adds them.  helper_ctx: a context on
 * another device; ck_on_helper: a replica of ck_primary resident there (same generators).  The proof is unchanged. */
int vimz_ivc_add_msm_helper(vimz_ivc* v, vimz_ctx* helper_ctx, const vimz_bases* ck_on_helper);
/* same inputs as vimz_prover_fold / vimz_prover_fold_witness */
int vimz_ivc_fold(vimz_ivc* v, const uint64_t* step_inputs, size_t nsteps);
int vimz_ivc_fold_witness(vimz_ivc* v, const uint64_t* witnesses, size_t nsteps);
/* RecursiveSNARK::verify(pp, num_steps, z0_primary, z0_secondary) (reached from folding.rs:53-55): the proof must be about exactly
 * `num_steps` steps from the initial state `z0` (len_z canonical elements; the secondary's z0 is the constant [0]); both output
 * hashes (recomputed from the CLAIMED z0), is_sat_relaxed of both running instances, is_sat of the last secondary instance,
 * every commitment re-opened.  result: 0 = accepted; bit 12 the proof's step count or initial state differ from the claimed ones; bit 0/1 hash of the primary/secondary chain; bit 2 primary relaxed relation;
 * bit 3 primary comm_W; bit 4 primary comm_E; bit 5 secondary relaxed relation; bit 6/7 secondary comm_W/comm_E; bit 8 last
 * secondary instance's relation; bit 9 its comm_W; bit 10 instance scalars differ from the witness vectors; bit 11 the running products (A,B,C)·Z kept for the next
 * fold violate the relation (prover-side bookkeeping, not part of the proof). */
int vimz_ivc_verify(vimz_ivc* v, uint64_t num_steps, const uint64_t* z0, uint32_t* result);
/* info[0..11]: steps, primary wires, primary constraints, step wires, step constraints, secondary wires, secondary constraints,
 * len_z, verifier-circuit wires (primary), nnz(A+B+C) primary, nnz secondary, rows of the last fold call whose Poseidon chains ran on the host */
int vimz_ivc_info(const vimz_ivc* v, uint64_t info[12]);
int vimz_ivc_state(const vimz_ivc* v, uint64_t* z_current /* len_z x 4 */, uint64_t* steps);
/* IVC state chain only (as vimz_prover_state_chain): where a row segment proven by another IVC starts */
int vimz_ivc_state_chain(vimz_ivc* v, const uint64_t* z_start, const uint64_t* step_inputs, size_t nsteps, uint64_t* zs_out);
/* the same in its two parts (see vimz_prover_row_digests): what vimz_amd/distributed.py::prove_sharded uses across ranks */
size_t vimz_ivc_digest_stride(const vimz_ivc* v);
int vimz_ivc_row_digests(vimz_ivc* v, const uint64_t* step_inputs, size_t nsteps, uint64_t* digests_out);
int vimz_ivc_chain_from_digests(vimz_ivc* v, const uint64_t* z_start, const uint64_t* step_inputs, const uint64_t* digests, size_t nsteps, uint64_t* zs_out);
/* seconds[8]/counts[8]: verifier-circuit witness primary (host), secondary (host), wait for secondary MSMs, wait for primary MSMs,
 * uploads+launches, producer wait, GPU time of the secondary half on the main stream (only while profiling is on), total */
int vimz_ivc_profile(const vimz_ivc* v, double seconds[8], uint64_t counts[8]);
/* The proof as an object of its own (RecursiveSNARK serialisation; checkpoint / resume): everything vimz_ivc_verify reads and the
 * next vimz_ivc_fold needs.  Import into a vimz_ivc created for the same step circuit and keys, then verify or keep folding. */
size_t vimz_ivc_proof_size(const vimz_ivc* v);
int vimz_ivc_proof_export(vimz_ivc* v, uint8_t* blob, size_t cap);
int vimz_ivc_proof_import(vimz_ivc* v, const uint8_t* blob, size_t len);
/* ---- CompressedSNARK::{setup, prove, verify} (vimz/src/nova_snark_backend/mod.rs:52-67: Spartan relaxed-R1CS SNARK with
 *      inner-product-argument openings over both curves; README.md:196 counts it into the total proof time).  Our own statement of
 *      the construction (vimz_amd/csrc/spartan.hip), NOT byte-compatible with nova-snark's proof object.  The proof covers the two
 *      running instances and the last fresh secondary instance of the IVC and carries (steps, z_0, z_n). ---------------------------- */
size_t vimz_ivc_compressed_size(vimz_ivc* v);                    /* bytes of a compressed proof for this IVC's shapes */
/* prove: blob receives vimz_ivc_compressed_size(v) bytes; seconds (optional) = {setup (first call only), prove} */
int vimz_ivc_compress(vimz_ivc* v, uint8_t* blob, size_t cap, double seconds[2]);
/* verify(vk, num_steps, z0): `v` supplies the verifier key — any vimz_ivc created for the same step circuit and commitment keys;
 * its folding state is neither read nor changed.  result: 0 = accepted; bit 0 / 1 primary / secondary chain hash; bit 2 / 3 / 4 the
 * argument for the primary running / secondary running / last fresh secondary instance; bit 12 statement mismatch; bit 13 malformed. */
int vimz_ivc_verify_compressed(vimz_ivc* v, const uint8_t* blob, size_t len, uint64_t num_steps, const uint64_t* z0, uint32_t* result);

/* KZG opening of a committed, device-resident vector (the `KZG::prove` of Sonobe's decider for the final commitments, reached from
 * vimz/src/sonobe_backend/decider.rs:13-21; calldata words kzg_*: vimz_amd/calldata.py): `srs` = the SRS's G1 powers [τ^i]G as bases
 * (vimz_bases_upload), so that vimz_msm_vec over them commits to p(X) = Σ v_i X^i.  eval_out = p(z); proof_xy = the commitment to
 * (p(X) − p(z)) / (X − z) (affine, `form`; the identity as zeros).  z and eval_out in `form`.  The pairing check belongs to the verifier. */
int vimz_kzg_open(vimz_ctx* ctx, const vimz_bases* srs, size_t base_offset, const vimz_vec* v, size_t offset, size_t n, const uint64_t z[4], int form,
                  uint64_t eval_out[4], uint64_t proof_xy[8]);

/* Multilinear KZG opening of a committed, device-resident vector over the same SRS: v of n <= N = 2^logn elements of BN254 Fr, read as
 * zero-padded to N, is the multilinear polynomial with v[i] at the corner whose k-th coordinate is the k-th LOWEST bit of i; comm_out = Σ v[i]·srs[i] (what
 * vimz_msm_vec gives), eval_out = its value at point (logn elements), proof = vimz_mlkzg_proof_words(logn) = 20·logn + 16 words.  Everything canonical.
 * seconds (optional) = {folds and their commitments, evaluations, batching and divisions, the three quotient commitments}.  Refused with a message: logn = 0 or
 * above 26, n = 0 or above 2^logn, an SRS shorter than 2^logn, a vector not over BN254 Fr or a key not on BN254 G1, a point element not below r, a short cap_words. */
size_t vimz_mlkzg_proof_words(uint32_t logn);      /* 0 for a logn out of range */
int vimz_mlkzg_open(vimz_ctx* ctx, const vimz_bases* srs, const vimz_vec* v, size_t offset, size_t n, uint32_t logn, const uint64_t* point, uint64_t comm_out[8],
                    uint64_t eval_out[4], uint64_t* proof, size_t cap_words, double seconds[4]);
/* The verifier: host only, no context, no GPU.  vk_g2 = [tau]G2 (x.c0, x.c1, y.c0, y.c1).  *result = 0 accepted, else ONE of VIMZ_MLKZG_* — each stage runs
 * only if the earlier ones found nothing.  A NULL pointer or logn = 0 is VIMZ_ERR_INVALID; everything else is a verdict. */
#define VIMZ_MLKZG_MALFORMED 1u      /* wrong word count, logn out of range, an element not below r, a coordinate not below q */
#define VIMZ_MLKZG_OFF_CURVE 2u      /* comm, a C_k or a W off the curve (vk_g2 off the twist or outside the subgroup) */
#define VIMZ_MLKZG_FOLD 4u           /* a fold equation between the claimed evaluations fails, or the challenge r is zero */
#define VIMZ_MLKZG_PAIRING 8u        /* the batched pairing equation fails */
int vimz_mlkzg_verify(const uint64_t vk_g2[16], const uint64_t comm[8], uint32_t logn, const uint64_t* point, const uint64_t eval[4], const uint64_t* proof,
                      size_t n_words, uint32_t* result);

/* ---- Nova + CycleFold IVC: the `prove_step` loop of the reference's Sonobe backend (vimz/src/sonobe_backend/folding.rs:52-66; scheme
 *      `Nova<G1, G2, C, KZG<Bn254>, Pedersen<G2>, false>`, folding.rs:22) — SURVEY.md §8 row N1.  The main circuit F' (step circuit + our
 *      statement of CycleFold's augmented circuit, vimz_amd/csrc/aug/cyclefold.hpp) is committed on BN254 G1 — ck_main may be a KZG SRS's
 *      G1 powers (vimz_bases_upload) or any other generators —, the CycleFold circuit (1.4 k constraints over Fq) on Grumpkin.  Sonobe is
 *      not vendored with the reference: NOT byte-compatible with its proof object, and the decider (Groth16 + KZG, decider.rs:13-21) is
 *      not built; the calldata layout of its output is vimz_amd/calldata.py.  One proof = (U_n, W_n), (u_n, w_n), (cfU_n, cfW_n). ---------- */
typedef struct vimz_cf vimz_cf;
int vimz_cf_create(vimz_ctx* ctx, const vimz_circuit* step_circuit, const vimz_bases* ck_main, const vimz_bases* ck_cyclefold, size_t max_batch, vimz_cf** out);
void vimz_cf_free(vimz_cf* v);
int vimz_cf_reset(vimz_cf* v, const uint64_t* z0);
/* Folding::prove_step for every row (same inputs as vimz_ivc_fold) */
int vimz_cf_fold(vimz_cf* v, const uint64_t* step_inputs, size_t nsteps);
/* Folding::verify(vp, ivc_proof) (folding.rs:69-75) for the claimed statement: 0 = accepted; bit 0 / 1 the hash of the main / CycleFold running
 * instance carried by the last instance of F'; bit 2 main relaxed relation; bit 3 / 4 main comm_W / comm_E; bit 5 CycleFold relaxed relation;
 * bit 6 / 7 its comm_W / comm_E; bit 8 the last instance of F' (strict); bit 9 its comm_W; bit 10 instance scalars differ from the witness
 * vectors; bit 11 prover-side running products; bit 12 the proof's step count or initial state differ from the claimed ones. */
int vimz_cf_verify(vimz_cf* v, uint64_t num_steps, const uint64_t* z0, uint32_t* result);
/* info[0..12): steps, main wires, main constraints, step wires, step constraints, CycleFold wires, CycleFold constraints, len_z,
 * F' wires, nnz main, nnz CycleFold, public elements of a CycleFold instance */
int vimz_cf_info(const vimz_cf* v, uint64_t info[12]);
int vimz_cf_state(const vimz_cf* v, uint64_t* z_current, uint64_t* steps);
/* seconds[8]/counts[8]: cross term + MSM(T), the two CycleFold instances, F' on the host, fresh instance (upload, verifier rows,
 * commitment), producer wait, total, and — parts of the fresh-instance phase — the wait for the producer's row, for the verifier wires' commitment */
int vimz_cf_profile(const vimz_cf* v, double seconds[8], uint64_t counts[8]);
/* side 0 = main circuit, 1 = CycleFold circuit; what = VIMZ_CX_* (R1CS tables), VIMZ_IX_INFO, VIMZ_IX_INSTANCE (side 0: comm_W.x, comm_W.y,
 * comm_E.x, comm_E.y, u, x0, x1; side 1: comm_W.x, comm_W.y, comm_E.x, comm_E.y, u, x[0..7)), VIMZ_IX_FRESH_INSTANCE (side 0: comm_W.x,
 * comm_W.y, x0, x1), VIMZ_IX_PARAMS (side 0: digest, z0..., z_i...), VIMZ_IX_RUNNING_Z, VIMZ_IX_RUNNING_E, VIMZ_IX_FRESH_Z (side 0),
 * VIMZ_IX_LAST_STEP (side 0: inputs and outputs of the last step's F', for an independent restatement of the step relation) */
int64_t vimz_cf_export(vimz_cf* v, int side, int what, void* buf, size_t cap);
/* KZG openings of the running main instance's commitments at z (vimz_kzg_open over ck_main as the SRS): which = 0 comm_W (coefficients = the witness
 * wires [1, wires - 2) of the running vector), 1 comm_E.  Canonical in and out. */
int vimz_cf_kzg_open(vimz_cf* v, int which, const uint64_t z[4], uint64_t eval_out[4], uint64_t proof_xy[8]);
/* ... and their multilinear openings at `point` (vimz_mlkzg_open over the same two vectors): logn must be the least with 2^logn >= the vector's length
 * (wires - 3 for which = 0, the constraints for 1); comm_out is the instance's comm_W / comm_E. */
int vimz_cf_mlkzg_open(vimz_cf* v, int which, const uint64_t* point, uint32_t logn, uint64_t comm_out[8], uint64_t eval_out[4], uint64_t* proof, size_t cap_words,
                       double seconds[4]);
/* The proof as an object of its own (Sonobe's `ivc_proof()` / `from_ivc_proof`; checkpoint / resume): everything vimz_cf_verify reads and the
 * next vimz_cf_fold needs.  Import into a vimz_cf created for the same step circuit and keys, then verify or keep folding. */
size_t vimz_cf_proof_size(const vimz_cf* v);
int vimz_cf_proof_export(vimz_cf* v, uint8_t* blob, size_t cap);
int vimz_cf_proof_import(vimz_cf* v, const uint8_t* blob, size_t len);
/* ONE proof object out of several row segments' CycleFold proofs (the north_star's "host-side sequential final fold" for this scheme; what
 * vimz_ivc_merge* is for the Nova IVC): segments folded concurrently — each a vimz_cf of its own on the same device — are folded in row order
 * by out-of-circuit NIFS: the running main instances pairwise (two relaxed instances), each segment's last instance of F' (strict), the
 * running CycleFold instances pairwise on Grumpkin.  The verifier replays the segment records (hashes from each segment's statement,
 * adjacency, folds of the instances) and checks ONE main and ONE CycleFold relaxed instance.  Protocol: vimz_amd/csrc/cyclefold_merge.hip, ours. */
typedef struct vimz_cf_merged vimz_cf_merged;
/* the merged proof of one segment; `first` is left unchanged, supplies shapes / keys / context and must outlive the object */
int vimz_cf_merged_create(vimz_cf* first, vimz_cf_merged** out);
void vimz_cf_merged_free(vimz_cf_merged* m);
/* fold the proof of the NEXT row segment in (same device; read in place, left unchanged): it must start at the state m ends in */
int vimz_cf_merge(vimz_cf_merged* m, vimz_cf* next_segment);
/* fold another merged object — ONE run of segments, e.g. what another GPU made of its rows (north_star's sharding) — in, as a whole: two relaxed
 * accumulators on each side.  It must start at the state m ends in; read in place, left unchanged; afterwards m takes no more single segments. */
int vimz_cf_merge_merged(vimz_cf_merged* m, vimz_cf_merged* other);
/* the object as bytes (records + the folded witnesses and running products), and back — into the context of `vk`, any vimz_cf for the same step
 * circuit and keys; untrusted input: ranges, curve membership, the accumulator recomputed from the records */
size_t vimz_cf_merged_size(const vimz_cf_merged* m);
int vimz_cf_merged_save(vimz_cf_merged* m, uint8_t* blob, size_t cap);
int vimz_cf_merged_load(vimz_cf* vk, const uint8_t* blob, size_t len, vimz_cf_merged** out);
/* the hand-over between two processes of one node without the host round trip, as vimz_ivc_merged_share / _open_shared: a ticket (records + HIP IPC
 * handle), a device-to-device copy of the ten vectors on the receiving side */
int64_t vimz_cf_merged_share(vimz_cf_merged* m, void* ticket, size_t cap);
int vimz_cf_merged_open_shared(vimz_cf* vk, const uint8_t* ticket, size_t len, vimz_cf_merged** out);
/* result: 0 = accepted; bit 0 / 1 a segment's main / CycleFold hash; bit 2 / 3 / 4 main relaxed relation / comm_W / comm_E; bit 5 / 6 / 7 the
 * same of the CycleFold instance; bit 10 instance scalars differ from the vectors; bit 12 statement (step count, initial state, adjacency);
 * bit 13 the stored folded instances differ from the replay of the records */
int vimz_cf_merged_verify(vimz_cf_merged* m, uint64_t num_steps, const uint64_t* z0, uint32_t* result);
/* info[0..8): steps, segments, len_z, main wires, main constraints, CycleFold wires, CycleFold constraints, broken */
int vimz_cf_merged_info(const vimz_cf_merged* m, uint64_t info[8]);
int vimz_cf_merged_state(const vimz_cf_merged* m, uint64_t* z_start, uint64_t* z_end, uint64_t* steps);
int vimz_cf_merged_profile(const vimz_cf_merged* m, double seconds[4]);   /* cross terms + commitments, folds, host, total */
/* the statement part as canonical little-endian 64-bit words (layout: cyclefold_merge.hip); returns the byte size */
int64_t vimz_cf_merged_records(const vimz_cf_merged* m, void* buf, size_t cap);
/* side 0 / 1; what = VIMZ_IX_RUNNING_Z, VIMZ_IX_RUNNING_E, VIMZ_IX_INSTANCE (side 0: 7 elements, side 1: 12 — as vimz_cf_export) of the folded instances */
int64_t vimz_cf_merged_export(vimz_cf_merged* m, int side, int what, void* buf, size_t cap);
/* KZG openings (vimz_kzg_open over ck_main as the SRS) of the FOLDED main instance: which = 0 comm_W, 1 comm_E.  For a merged proof of one segment the
 * folded instance is U_{i+1} = NIFS(U_i, u_i), the one Sonobe's decider opens (decider.rs:13-21).  Canonical in and out. */
int vimz_cf_merged_kzg_open(vimz_cf_merged* m, int which, const uint64_t z[4], uint64_t eval_out[4], uint64_t proof_xy[8]);
/* ... and their multilinear openings, as vimz_cf_mlkzg_open */
int vimz_cf_merged_mlkzg_open(vimz_cf_merged* m, int which, const uint64_t* point, uint32_t logn, uint64_t comm_out[8], uint64_t eval_out[4], uint64_t* proof,
                              size_t cap_words, double seconds[4]);
/* IVC state chain only (as vimz_ivc_state_chain): the state at which a row segment proven by another vimz_cf starts */
int vimz_cf_state_chain(vimz_cf* v, const uint64_t* z_start, const uint64_t* step_inputs, size_t nsteps, uint64_t* zs_out);
/* ... in its two parts, as vimz_ivc_row_digests / vimz_ivc_chain_from_digests */
size_t vimz_cf_digest_stride(const vimz_cf* v);
int vimz_cf_row_digests(vimz_cf* v, const uint64_t* step_inputs, size_t nsteps, uint64_t* digests_out);
int vimz_cf_chain_from_digests(vimz_cf* v, const uint64_t* z_start, const uint64_t* step_inputs, const uint64_t* digests, size_t nsteps, uint64_t* zs_out);
/* CompressedSNARK for the Nova + CycleFold proofs (vimz_amd/csrc/spartan.hip; framing of the blobs: vimz_amd/csrc/cf_compressed_parse.hpp): a few
 * kilobytes a third party checks with the verifier key alone — any vimz_cf created for the same step circuit and commitment keys, whose folding
 * state is neither read nor changed.  Needs ck_main of at least next_pow2(max(wires, constraints)) of F + F' and ck_cyclefold of as many for the
 * CycleFold circuit (shorter: VIMZ_ERR_INVALID).  seconds (optional) = {set-up (first call on this object only), prove}.
 * One chain: the statement of vimz_cf_verify, with an argument in place of every witness check — U_n (relaxed), u_n (strict) over F + F' on BN254 G1,
 * cfU_n (relaxed, 7 public elements) over the CycleFold circuit on Grumpkin; carries (steps, z_0, z_n).  An object with no steps is refused.
 * result: 0 = accepted; bit 0 / 1 the hash x0 / x1 that u_n carries; bit 2 / 3 / 4 the argument for U_n / cfU_n / u_n; bit 12 statement (steps, z0)
 * differs; bit 13 malformed (a blob of another kind included). */
size_t vimz_cf_compressed_size(vimz_cf* v);
int vimz_cf_compress(vimz_cf* v, uint8_t* blob, size_t cap, double seconds[2]);
int vimz_cf_verify_compressed(vimz_cf* vk, const uint8_t* blob, size_t len, uint64_t num_steps, const uint64_t* z0, uint32_t* result);
/* Merged: the records (vimz_cf_merged_records) and one argument each for the folded main and the folded CycleFold instance.  The verifier replays the
 * records as vimz_cf_merged_verify does and verifies the arguments for the instances IT computed.  A broken or orphaned object is refused.
 * result: 0 = accepted; bit 0 / 1 a segment's main / CycleFold hash; bit 2 / 3 the argument for the folded main / CycleFold instance; bit 12 statement
 * (steps, z0, adjacency); bit 13 malformed. */
size_t vimz_cf_merged_compressed_size(const vimz_cf_merged* m);
int vimz_cf_merged_compress(vimz_cf_merged* m, uint8_t* blob, size_t cap, double seconds[2]);
int vimz_cf_verify_merged_compressed(vimz_cf* vk, const uint8_t* blob, size_t len, uint64_t num_steps, const uint64_t* z0, uint32_t* result);
/* (test hooks — vimz_cf_poke, the host-only self-checks — are declared in vimz_hip_testing.h and exist only in libvimz_hip_testing.so) */

/* ---- the decider of the Nova + CycleFold path: `Decider::preprocess` / `Decider::prove` / `Decider::verify` of the Sonobe backend
 *      (vimz/src/sonobe_backend/mod.rs:72-80; `DeciderEth<.., Groth16<Bn254>, ..>`, decider.rs:13-21; verify_final_proof, decider.rs:31-50) — the 25 words
 *      `contracts/<T>Verifier.sol::verifyOpaqueNovaProofWithInputs` takes (ContrastVerifier.sol:785-810; solidity.rs:13-27).  Groth16 over BN254 as
 *      published, with the PUBLIC-INPUT LAYOUT of the reference's contracts (pp_hash, i, z_0, z_i, the folded commitments and cmT as 5 x 55-bit
 *      limbs per coordinate, the KZG challenges and evaluations: ContrastVerifier.sol:700-772) — pinned: tests/_novadecider.py restates the
 *      contract, accepts the reference's six committed proofs with the reference's keys, and accepts this library's words with this library's
 *      key.  The circuit's CONSTRAINTS (vimz_amd/csrc/aug/decider.hpp, decider_cf.hpp) are ours, parity unpinned: Sonobe's circuit and keys come out
 *      of crates that are not vendored, so the committed `.proof` bytes cannot be reproduced.  Two variants, as in the reference: the FULL decider
 *      (decider.rs:13-21: also opens the running CycleFold instance's two commitments and checks its relaxed relation inside the circuit — natively over
 *      Grumpkin, non-natively over Fq; ≈ 2.75 M constraints on top of the step circuit's) and the LIGHT one (the opt-in `light-test` feature,
 *      vimz/Cargo.toml:56-59, vimz/Makefile:1-2, the contracts under contracts/light-test/: the CycleFold instance bound by its hash only).  Same public inputs, same
 *      25 words.  NTTs, the G1 / G2 multi-scalar multiplications, the final fold, the KZG openings and the keys' fixed-base multiplications run on
 *      the GPU; verification of ONE proof is host code (pairing.hpp), verification of MANY under one key (vimz_decider_verify_batch) runs its per-proof part —
 *      point checks, scalar multiplications, Miller loops — on the GPU.  The 25-word layout is the reference contracts' INTERFACE, not by itself a sound on-chain
 *      decider: U_i's and u_i's commitments and the fold's r reach the contract as unconstrained calldata (aug/decider.hpp). ---------- */
typedef struct vimz_decider vimz_decider;
/* KZG::setup (inside `prepare_folding`, vimz/src/sonobe_backend/folding.rs:36-48): srs = [tau^i]G1 for i < n as a commitment key (use it as
 * ck_main of vimz_cf_create), vk_g2_out = [tau]G2 (x.c0, x.c1, y.c0, y.c1 canonical).  tau comes from the OS's randomness and is forgotten. */
int vimz_kzg_setup(vimz_ctx* ctx, size_t n, vimz_bases** srs_out, uint64_t vk_g2_out[16]);
/* The Lagrange basis of a powers-of-tau string's points (what snarkjs's `powersoftau prepare phase2` computes; the first step of a Groth16 set-up that draws no
 * trapdoor): out[j] = L_j = 1/n · sum_k w^(−jk)·points[k] over the first n = 2^logn points, w the primitive n-th root of unity
 * 5^((r−1)/n) of Fr — [L_j(tau)]G when points[k] = [tau^k]G, so that sum_j e_j·out[j] commits to the polynomial with the evaluations e_j.  group = 1: points of
 * BN254 G1, 8 words each (x, y); group = 2: of G2, 16 words (x.c0, x.c1, y.c0, y.c1).  form = VIMZ_FORM_* of the coordinates, `out` in the same form; the identity
 * is zeros on both sides.  The inverse transform over points runs on the GPU (radix 2, one launch per stage, logn·n/2 scalar multiplications), on the
 * context's stream and under the context's lock like every call on a context: it does not overlap a fold on the same context (a set-up that must run under a
 * fold needs a stream of its own).  VIMZ_ERR_INVALID: a NULL pointer, a group other than 1 or 2, logn outside 1..26, n_points < 2^logn, a coordinate not below
 * q, a point not on its curve.  Membership of the order-r subgroup of G2 and that the points are the powers of one tau (the same-ratio check of the string) are
 * judged by vimz_powers_verify, which is opt-in: this call does not run it.  seconds (optional) = {host conversion and checks, device (upload, transform, download)}. */
int vimz_powers_lagrange(vimz_ctx* ctx, int group /* 1: G1, 8 words a point; 2: G2, 16 words: x.c0 x.c1 y.c0 y.c1 */, const uint64_t* points, size_t n_points,
                         int form, int logn, uint64_t* out, double seconds[2]);
/* Judges a powers-of-tau string before a set-up trusts it — what snarkjs's `powersoftau verify` does to a ceremony's file, for the arrays vimz_decider_setup_from_powers,
 * vimz_powers_lagrange and hip.kzg_from_powers read (same layout and form): tau_g1 n_tau_g1 points, tau_g2, alpha_g1, beta_g1 n_pow points each, beta_g2 one.  On the GPU:
 * every point is on its curve and not the identity, every point of G2 is killed by r (decided point by point: the twist's cofactor has small factors a sum would
 * miss), and per array two random combinations S = sum rho_i·P_i, S' = sum rho_i·P_(i+1) over the pairs of neighbours, rho_i of 128 bits from the OS, wiped after use.  On
 * the host six pairing equations: e(S', G2) = e(S, tau_g2[1]) for tau_g1, alpha_g1, beta_g1; e(G1, S') = e(tau_g1[1], S) for tau_g2 — each array is the powers of the ONE
 * tau of tau_g2[1] up to a factor, wrongly accepted with probability at most 2^-128 —; e(tau_g1[1], G2) = e(G1, tau_g2[1]); e(beta_g1[0], G2) = e(G1, beta_g2); and the
 * first points of tau_g1 and tau_g2 are the generators.  A stage runs only when the ones before it found nothing.
 * Returns VIMZ_OK whenever the string was judged: a bad string is a verdict, not an error.  *result = 0: accepted; otherwise VIMZ_POWERS_* bits.  first_bad = {array: 1
 * tau_g1, 2 tau_g2, 3 alpha_g1, 4 beta_g1, 5 beta_g2; index} of the first per-point finding (VIMZ_POWERS_COORD .. _FIRST) of the first array that has one — *result then holds
 * that array's findings alone —, {0, 0} when there is none: a ratio that fails names its array by its bit only.  seconds (optional) = {host conversion, per-point flags
 * (upload included), combinations, pairings}.  VIMZ_ERR_INVALID: a NULL pointer (seconds apart), n_pow < 2, n_tau_g1 < n_pow, an unknown form.  Runs on the context's stream
 * under the context's lock, one array on the device at a time: the peak device memory is one array, its flags and the scalars (16 bytes a pair of tau_g1). */
#define VIMZ_POWERS_COORD 0x1u           /* a coordinate is not below q */
#define VIMZ_POWERS_OFF_CURVE 0x2u       /* a point is not on its curve */
#define VIMZ_POWERS_IDENTITY 0x4u        /* a point is the identity */
#define VIMZ_POWERS_SUBGROUP 0x8u        /* a point of G2 is outside the subgroup of order r */
#define VIMZ_POWERS_FIRST 0x10u          /* tau_g1[0] or tau_g2[0] is not the generator */
#define VIMZ_POWERS_RATIO_TAU_G1 0x20u   /* tau_g1 is not the powers of tau_g2[1]'s tau */
#define VIMZ_POWERS_RATIO_ALPHA_G1 0x40u
#define VIMZ_POWERS_RATIO_BETA_G1 0x80u
#define VIMZ_POWERS_RATIO_TAU_G2 0x100u  /* tau_g2 is not the powers of tau_g1[1]'s tau */
#define VIMZ_POWERS_HALVES 0x200u        /* tau_g1[1] and tau_g2[1] are not of one tau */
#define VIMZ_POWERS_BETA 0x400u          /* beta_g1[0] and beta_g2 are not of one beta */
int vimz_powers_verify(vimz_ctx* ctx, const uint64_t* tau_g1, size_t n_tau_g1, const uint64_t* tau_g2, const uint64_t* alpha_g1, const uint64_t* beta_g1, size_t n_pow,
                       const uint64_t beta_g2[16], int form, uint32_t* result, uint64_t first_bad[2], double seconds[4]);
/* A contribution to a powers-of-tau string (phase 1 of a ceremony; what snarkjs calls `powersoftau contribute`), on the arrays vimz_powers_verify takes (same layout and
 * form): tau', alpha', beta' != 0 and three nonces come from the OS and are wiped on every path, host and device; tau_g1[k] and tau_g2[k] become tau'^k times themselves,
 * alpha_g1[k] alpha'·tau'^k times, beta_g1[k] beta'·tau'^k times — one scalar multiplication a point with a DIFFERENT scalar at every point, on the GPU: ONE vector of
 * the n_tau_g1 powers of tau' is made on the device, each array goes there alone, is scaled and comes back, and the vector is overwritten before it is freed (peak device
 * memory: one array and 32 bytes a point of tau_g1) — and beta_g2 becomes beta'·beta_g2 on the host.  The string of (tau, alpha, beta) leaves as the string of
 * (tau·tau', alpha·alpha', beta·beta').  The *_out arrays have the inputs' sizes and form and may be the inputs; nothing is written unless everything succeeded.
 * record_out: VIMZ_POWCHAIN_RECORD_WORDS little-endian words — this project's own format (vimz_amd/csrc/g16_powers_contrib.hpp), NOT snarkjs's transcript: magic
 * "VPOTCTR1", then as canonical words tau_g1[1], alpha_g1[0], beta_g1[0] AFTER the contribution (8 each), T_tau, T_alpha, T_beta (8 each), z_tau, z_alpha, z_beta (4
 * each): three Schnorr proofs of knowledge of tau', alpha', beta' over the same points BEFORE the contribution, each bound to all six points.  Records are kept apart from
 * the string, one after another.  The walk over a secret scalar's bits is NOT constant-time, on host or device.  seconds (optional) = {host (conversion, checks, the
 * record, beta_g2), device (power vector, uploads, scaling, downloads), total}.  VIMZ_ERR_INVALID with a message: a NULL pointer (seconds apart), n_pow < 2, n_tau_g1 <
 * n_pow, an unknown form, a coordinate not below q, a point off its curve, tau_g1[1], alpha_g1[0] or beta_g1[0] the identity.  The string is otherwise NOT judged —
 * subgroup membership in G2, that it is a string at all: vimz_powers_verify's matter. */
#define VIMZ_POWCHAIN_RECORD_WORDS 61
int vimz_powers_contribute(vimz_ctx* ctx, const uint64_t* tau_g1, size_t n_tau_g1, const uint64_t* tau_g2, const uint64_t* alpha_g1, const uint64_t* beta_g1, size_t n_pow,
                           const uint64_t beta_g2[16], int form, uint64_t* tau_g1_out, uint64_t* tau_g2_out, uint64_t* alpha_g1_out, uint64_t* beta_g1_out, uint64_t beta_g2_out[16],
                           uint64_t record_out[VIMZ_POWCHAIN_RECORD_WORDS], double seconds[3]);
/* Judges a chain of such contributions: the final string (arrays as above) is what n_records contributions (`records`, 61 words each, in order; n_records may be 0) made
 * of a string whose tau_g1[1], alpha_g1[0], beta_g1[0] were origin_points (24 canonical words; for a new string three times the generator).  Returns VIMZ_OK whenever
 * the chain was judged: a bad chain is a verdict, not an error.  *result = 0: accepted; otherwise VIMZ_POWCHAIN_* bits.  Stage by stage, a stage only when the ones
 * before it found nothing:  the POINTS — the origin's three and every record's nine points have coordinates below q, are on the curve and not the identity (the bits
 * of the first place that has a finding);  KNOWLEDGE, all evaluated — z_s·B_s = T_s + c_s·A_s for the three secrets of every record, B the points of the record
 * before it (of the origin for the first), and the last record's points (the origin's, without records) are the final string's tau_g1[1], alpha_g1[0], beta_g1[0];
 * the STRING — the final string goes through vimz_powers_verify as it stands; a refusal sets _STRING, *string_result holds that call's VIMZ_POWERS_* bits (0 otherwise).
 * first_bad = {VIMZ_POWCHAIN_AT_*, index}: _AT_ORIGIN with the point's number (0 tau, 1 alpha, 2 beta), _AT_RECORD with the first bad record's number,
 * _AT_STRING_<array> with vimz_powers_verify's index; {0, 0} when only _LAST fails or the string fails by its equations alone.
 * An accepted chain means: the final string is the powers of ONE tau with consistent alpha and beta, and tau, alpha, beta are unknown to everyone if ANY ONE contributor
 * forgot their secrets, whatever the origin was — every record holder knew the factor between its points and the ones before, and the string's own check ties every
 * other point to those three.  It does NOT give: a random beacon (the last contributor can still try secrets until the result suits them), nor compatibility with
 * snarkjs's transcript, challenge files or response files.  seconds (optional) = {points, knowledge, the string's verdict}.  VIMZ_ERR_INVALID: a NULL pointer
 * (seconds apart; records when n_records is 0), a record with the wrong magic, and what vimz_powers_verify answers it to. */
#define VIMZ_POWCHAIN_COORD 0x1u            /* a coordinate is not below q */
#define VIMZ_POWCHAIN_OFF_CURVE 0x2u        /* a point is not on its curve */
#define VIMZ_POWCHAIN_IDENTITY 0x4u         /* a point is the identity */
#define VIMZ_POWCHAIN_KNOWLEDGE_TAU 0x8u    /* a record's proof of knowledge of tau' fails over the points before it */
#define VIMZ_POWCHAIN_KNOWLEDGE_ALPHA 0x10u
#define VIMZ_POWCHAIN_KNOWLEDGE_BETA 0x20u
#define VIMZ_POWCHAIN_LAST 0x40u            /* the last record's points are not the final string's tau_g1[1], alpha_g1[0], beta_g1[0] */
#define VIMZ_POWCHAIN_STRING 0x80u          /* vimz_powers_verify refuses the final string: its bits are in *string_result */
#define VIMZ_POWCHAIN_AT_ORIGIN 1
#define VIMZ_POWCHAIN_AT_RECORD 2
#define VIMZ_POWCHAIN_AT_STRING_TAU_G1 3    /* 2 + vimz_powers_verify's array number */
#define VIMZ_POWCHAIN_AT_STRING_TAU_G2 4
#define VIMZ_POWCHAIN_AT_STRING_ALPHA_G1 5
#define VIMZ_POWCHAIN_AT_STRING_BETA_G1 6
#define VIMZ_POWCHAIN_AT_STRING_BETA_G2 7
int vimz_powers_verify_contributions(vimz_ctx* ctx, const uint64_t origin_points[24], const uint64_t* tau_g1, size_t n_tau_g1, const uint64_t* tau_g2, const uint64_t* alpha_g1,
                                     const uint64_t* beta_g1, size_t n_pow, const uint64_t beta_g2[16], int form, const uint64_t* records, size_t n_records, uint32_t* result,
                                     uint32_t* string_result, uint64_t first_bad[2], double seconds[3]);
/* Decider::preprocess.  prover: supplies shapes, keys and context (must outlive the object).  kzg_vk_g2 (optional): [tau]G2 of the SRS the prover's
 * ck_main is made of (needed by vimz_decider_verify; part of vimz_decider_vk; checked against that SRS: e(srs[1], G2) = e(G1, [tau]G2)).
 * light: 0 = the full decider (the reference's default), non-zero = the `light-test` variant.  The full decider bakes the first generators of the
 * prover's CycleFold commitment key into the circuit.  The Groth16 trapdoor comes from the OS's randomness and is wiped after use (a locally trusted
 * setup; seeded test setups exist only in libvimz_hip_testing.so).  seconds (optional) = {circuit synthesis, QAP evaluation at the trapdoor, key
 * points on the GPU, total} */
int vimz_decider_setup(vimz_cf* prover, const uint64_t kzg_vk_g2[16], int light, vimz_decider** out, double seconds[4]);
/* Decider::preprocess from a powers-of-tau string (iden3.read_ptau's arrays: tau_g1 2n − 1 or more points [tau^k]G1, tau_g2, alpha_g1, beta_g1 n or more points
 * each — n_pow of them —, beta_g2 one point; G1 points 8 words, G2 points 16 (x.c0, x.c1, y.c0, y.c1); form = VIMZ_FORM_* of the coordinates), n the circuit's domain
 * (vimz_decider_info).  The Groth16 key is derived by group operations on the GPU — the four Lagrange bases by the inverse transform over points, the a, b and K
 * queries as column sums of the matrices over them, l and h scaled by 1/delta — so tau, alpha and beta are the string's and never in this process; gamma = 1;
 * delta comes from the OS's randomness and is wiped after use: the key's trust rests on the string plus this one local delta.  The KZG verifying key is the
 * string's tau_g2[1], so the prover's ck_main must be the SRS of the same string (hip.kzg_from_powers).  VIMZ_ERR_INVALID with a message: a NULL pointer,
 * n_pow < n or n_tau_g1 < 2n − 1, a coordinate not below q, a point not on its curve, tau_g1[0] or tau_g2[0] not the generator, beta_g2 or tau_g2[1] outside
 * the subgroup, e(tau_g1[1], G2) != e(G1, tau_g2[1]), e(beta_g1[0], G2) != e(G1, beta_g2), tau_g2[1] not matching the prover's SRS.  The
 * same-ratio property of the whole string (that every point is the next power of ONE tau, alpha·, beta· included) and subgroup membership of the other points of
 * tau_g2 are judged by vimz_powers_verify, which is opt-in (hip.Decider(verify_powers=True) runs it first): this call does not.  The resulting object is an ordinary decider (prove, verify, vk, key_save).
 * seconds (optional) = {circuit synthesis, checks + upload, transforms, column sums, l/h scaling + key tables, total}. */
int vimz_decider_setup_from_powers(vimz_cf* prover, int light, const uint64_t* tau_g1, size_t n_tau_g1, const uint64_t* tau_g2, const uint64_t* alpha_g1,
                                   const uint64_t* beta_g1, size_t n_pow, const uint64_t beta_g2[16], int form, vimz_decider** out, double seconds[6]);
/* the domain n (vimz_decider_info's info[3]) a set-up of this prover's decider would work over, by synthesising the circuit alone (host; no key is made): what a
 * caller needs to judge the prefix of a string (vimz_powers_verify: n_pow = n, n_tau_g1 = 2n − 1) BEFORE vimz_decider_setup_from_powers reads it */
int vimz_decider_domain(vimz_cf* prover, int light, uint64_t* domain);
void vimz_decider_free(vimz_decider* d);
/* info = {constraints, wires, public inputs (36 + 2 len_z), domain size, non-zeros of A, B, C, rows of the CycleFold checks (0: light decider)} */
int vimz_decider_info(const vimz_decider* d, uint64_t info[8]);
/* the verifying key — the constants of a contract generated for this circuit — as canonical words: pp_hash (4), len_z (1), alpha (G1: x, y), beta,
 * gamma, delta (G2: x.c0, x.c1, y.c0, y.c1), the number of IC points, the IC points, KZG G_1 (G1), G_2, VK (G2); returns the byte size (copies
 * when cap suffices) */
int64_t vimz_decider_vk(const vimz_decider* d, void* buf, size_t cap);
/* The key pair at rest (bytes; layout: vimz_amd/csrc/groth16.hip): a set-up made once per circuit, or a key made elsewhere in this layout (the library then never
 * sees its trapdoor).  vimz_decider_setup_from_powers makes such a key from a ceremony's powers of tau with one local delta; further
 * delta contributions to a saved key: vimz_decider_key_contribute below.  _save returns the byte size (copies when cap suffices); _load checks sizes, the public-parameter hash and the
 * verifying part's points, and takes the queries as they are (a loaded key is trusted like any common reference string). */
int64_t vimz_decider_key_save(vimz_decider* d, void* buf, size_t cap);
int vimz_decider_key_load(vimz_cf* prover, const void* buf, size_t len, vimz_decider** out);
/* A further delta contribution to a saved key (phase 2 of a Groth16 ceremony; what snarkjs calls `zkey contribute`), on key BYTES: the layout is read from the blob's
 * own header, so a contributor needs a context and no prover.  delta' != 0 and a nonce come from the OS and are wiped on every path, host and device; delta1 and delta2
 * become delta'·delta1 and delta'·delta2 (host); the l and h queries, side by side in the blob, are multiplied by 1/delta' on the GPU as one array; every other byte is
 * copied.  key_out may be key_in.  Returns the byte size (= len; nothing is written, and no delta' drawn, when key_out is NULL or cap is short), or VIMZ_ERR_INVALID with a
 * message: a blob with the wrong magic or length, a coordinate (of delta1, delta2, l or h) not below q, a delta point off its curve or the identity, delta2 outside
 * the subgroup.  record_out: VIMZ_KEYCHAIN_RECORD_WORDS little-endian words — this project's own format (vimz_amd/csrc/g16_key_contrib.hpp), NOT a section of snarkjs's
 * `.zkey`: magic "VG16CTR1", delta1 after (8), delta2 after (16), T (8), z (4), a Schnorr proof of knowledge of delta' over the base delta1_before bound to the key's
 * header and pp_hash.  Records are kept apart from the key, one after another: the key format is unchanged.  seconds (optional) = {host, device (upload, scaling,
 * download), total}. */
#define VIMZ_KEYCHAIN_RECORD_WORDS 37
int64_t vimz_decider_key_contribute(vimz_ctx* ctx, const void* key_in, size_t len, void* key_out, size_t cap, uint64_t record_out[37], double seconds[3]);
/* Judges a chain of contributions (`zkey verify`): `final_key` is `origin` after the n_records contributions of `records` (37 words each, in order; n_records may be 0).
 * Returns VIMZ_OK whenever the chain was judged: a bad chain is a verdict, not an error.  *result = 0: accepted; otherwise VIMZ_KEYCHAIN_* bits.  Stage by stage, a stage
 * only when the ones before it found nothing:  the POINTS — every delta1_j, delta2_j, T_j and every point of l‖h of both keys has coordinates below q and is on its curve,
 * delta points are not the identity, every delta2_j is killed by r, a point of l‖h is the identity only where the other key's is too (per-point work on l‖h: the GPU);
 * the FIXED PART — the keys are the same words outside delta1, delta2, l and h;  the EQUATIONS, all evaluated — e(delta1_j, G2) = e(G1, delta2_j) and
 * z_j·delta1_(j−1) = T_j + c_j·delta1_j for every record, the last record's delta points (the origin's, without records) are the final key's, and the same-ratio
 * check of the end points: S = sum rho_i·P_i over the origin's l‖h, S' = sum rho_i·P'_i over the final's (one GPU pass under rho_i of 128 bits from the OS, wiped),
 * e(S', delta2_final) = e(S, delta2_origin) — wrongly accepted with probability at most 2^-128.
 * first_bad = {VIMZ_KEYCHAIN_AT_*, index}: the first finding's place — for _ORIGIN_DELTA / _FINAL_DELTA the index is 0 (delta1) or 1 (delta2); for _RECORD the record's
 * number; for _ORIGIN_LH / _FINAL_LH the point's index in l‖h; for _FIXED_PART the offset in 64-bit words of the first difference; {0, 0} when only _LAST or _RATIO fail.
 * A verified chain means: the final key is sound if the origin key is and ANY ONE contributor forgot their delta'.  That the origin key derives from a given
 * string and circuit is judged by vimz_decider_key_verify_origin; there is no random beacon.  seconds (optional) = {host conversion and host point checks, per-point flags (upload included),
 * combination, equations}.  VIMZ_ERR_INVALID: a NULL pointer (seconds apart), a key or a record with the wrong magic or length. */
#define VIMZ_KEYCHAIN_COORD 0x1u          /* a coordinate is not below q */
#define VIMZ_KEYCHAIN_OFF_CURVE 0x2u      /* a point is not on its curve */
#define VIMZ_KEYCHAIN_IDENTITY 0x4u       /* a delta point is the identity, or a point of l‖h is in one key only */
#define VIMZ_KEYCHAIN_SUBGROUP 0x8u       /* a delta2 is outside the subgroup of order r */
#define VIMZ_KEYCHAIN_FIXED_PART 0x10u    /* the keys differ outside delta1, delta2, l and h */
#define VIMZ_KEYCHAIN_DELTA_HALVES 0x20u  /* a record's delta1 and delta2 are not of one delta */
#define VIMZ_KEYCHAIN_KNOWLEDGE 0x40u     /* a record's proof of knowledge fails over the delta1 before it */
#define VIMZ_KEYCHAIN_LAST 0x80u          /* the last record's delta points are not the final key's */
#define VIMZ_KEYCHAIN_RATIO 0x100u        /* l‖h of the final key is not l‖h of the origin over the ratio of their delta2 */
#define VIMZ_KEYCHAIN_AT_ORIGIN_DELTA 1
#define VIMZ_KEYCHAIN_AT_FINAL_DELTA 2
#define VIMZ_KEYCHAIN_AT_RECORD 3
#define VIMZ_KEYCHAIN_AT_ORIGIN_LH 4
#define VIMZ_KEYCHAIN_AT_FINAL_LH 5
#define VIMZ_KEYCHAIN_AT_FIXED_PART 6
int vimz_decider_key_verify_contributions(vimz_ctx* ctx, const void* origin, size_t origin_len, const void* final_key, size_t final_len, const uint64_t* records, size_t n_records,
                                          uint32_t* result, uint64_t first_bad[2], double seconds[4]);
/* Judges a key someone else hands over (what snarkjs's `zkey verify` checks against an r1cs and a ptau): `key` (vimz_decider_key_save's bytes) is the key
 * vimz_decider_setup_from_powers would derive from THIS string for THIS prover's decider circuit, for the delta that its delta1/delta2 commit to.  delta is never
 * known and nothing is derived again: every query is linear in the string's Lagrange basis, so under rho in (128 bits)^m and rho' in (128 bits)^(n-1) from the OS (wiped
 * on host and device on every path) the combination of a query equals sparse products of the circuit's matrices with rho (on the GPU), inverse NTTs over Fr and MSMs over
 * the string's own powers — sum rho_i·a_i = MSM(tau_g1, c_A), the same for b1 and, in G2 over tau_g2, for b2; sum over the public wires rho_i·ic_i = K(P) (gamma = 1);
 * e(sum over the private wires rho_i·l_i, delta2) = e(K(Q), G2); e(sum rho'_j·h_j, delta2) = e(MSM(tau_g1[:2n-1], s), G2) (vimz_amd/csrc/g16_key_origin.hip states c_X, K
 * and s) — each wrongly accepted with probability at most 2^-128.  The mode, light or full, is read from the blob and the circuit is synthesised for it.  Stage by
 * stage, a stage only when the ones before it found nothing:  the HEADER's (m, n_pub, n_c, n, len_z, mode) and pp_hash are this prover's decider circuit's, and the
 * FIXED WORDS are the string's: alpha1 = alpha_g1[0], beta1 = beta_g1[0], beta2 = beta_g2, gamma2 = G2, the KZG point = tau_g2[1];  the POINTS — delta1, delta2 on
 * their curves, not the identity, delta2 killed by r (host); every coordinate below q, every point of ic, a, b1, l, h on the curve and every non-identity point of b2 on
 * the twist and killed by r, point by point (GPU; the identity is allowed in the queries: _save writes zeros for wires no matrix touches);  the EQUATIONS, all
 * evaluated, with e(delta1, G2) = e(G1, delta2).
 * An accepted key is sound if the string is: it is that set-up's key for SOME delta, whoever knows it — so a key that has had contributions passes too, checked
 * directly against string and circuit; who contributed is vimz_decider_key_verify_contributions' matter.  NOT judged: the string itself (vimz_powers_verify;
 * hip.verify_key_origin(verify_powers=True) runs it first) and who knows delta.
 * Returns VIMZ_OK whenever the key was judged: a bad key is a verdict, not an error.  *result = 0: accepted; otherwise VIMZ_KEYORIGIN_* bits.  first_bad =
 * {VIMZ_KEYORIGIN_AT_*, index}: for _HEADER the header word (1 m .. 6 mode, 7..10 pp_hash); for _FIXED 0 the KZG point, 1 alpha1, 2 beta1, 3 beta2, 4 gamma2; for _DELTA 0
 * delta1, 1 delta2; for an array the first flagged point of the first array that has one (*result then holds that array's findings alone); {0, 0} when only
 * equations fail.  seconds (optional) = {circuit synthesis, host conversion + fixed words, per-point flags (uploads included), circuit side (products, NTTs, MSMs),
 * key-side combinations + pairings}.  VIMZ_ERR_INVALID with a message: a NULL pointer (seconds apart), a blob with the wrong magic or length, n_pow < n or n_tau_g1 <
 * 2n - 1 for the key's domain n, an unknown form, a point of the STRING with a coordinate not below q or off its curve (the string's fault, not the key's).  Runs on the
 * context's stream under the context's lock; one array of the key is on the device at a time (peak device memory: g16_key_origin.hip). */
#define VIMZ_KEYORIGIN_COORD 0x1u         /* a coordinate is not below q */
#define VIMZ_KEYORIGIN_OFF_CURVE 0x2u     /* a point is not on its curve */
#define VIMZ_KEYORIGIN_DELTA 0x4u         /* a delta point is the identity, or delta1 and delta2 are not of one delta */
#define VIMZ_KEYORIGIN_SUBGROUP 0x8u      /* delta2 or a point of b2 is outside the subgroup of order r */
#define VIMZ_KEYORIGIN_HEADER 0x10u       /* sizes, mode or pp_hash are not this prover's decider circuit's */
#define VIMZ_KEYORIGIN_FIXED_POINTS 0x20u /* alpha1, beta1, beta2, gamma2 or the KZG point is not the string's */
#define VIMZ_KEYORIGIN_A 0x40u            /* the a query is not the string's and circuit's */
#define VIMZ_KEYORIGIN_B1 0x80u
#define VIMZ_KEYORIGIN_B2 0x100u
#define VIMZ_KEYORIGIN_IC 0x200u
#define VIMZ_KEYORIGIN_L 0x400u           /* ... for the delta of delta2 */
#define VIMZ_KEYORIGIN_H 0x800u
#define VIMZ_KEYORIGIN_AT_HEADER 1
#define VIMZ_KEYORIGIN_AT_FIXED 2
#define VIMZ_KEYORIGIN_AT_DELTA 3
#define VIMZ_KEYORIGIN_AT_IC 4
#define VIMZ_KEYORIGIN_AT_A 5
#define VIMZ_KEYORIGIN_AT_B1 6
#define VIMZ_KEYORIGIN_AT_L 7
#define VIMZ_KEYORIGIN_AT_H 8
#define VIMZ_KEYORIGIN_AT_B2 9
int vimz_decider_key_verify_origin(vimz_cf* prover, const void* key, size_t len, const uint64_t* tau_g1, size_t n_tau_g1, const uint64_t* tau_g2, const uint64_t* alpha_g1,
                                   const uint64_t* beta_g1, size_t n_pow, const uint64_t beta_g2[16], int form, uint32_t* result, uint64_t first_bad[2], double seconds[5]);
/* Packed curve points: x and one bit of y, y recovered on the GPU as a square root of x^3 + b when the point is read — half the bytes of a saved key or of a
 * powers-of-tau string outside snarkjs's container, and a point that unpacks is on its curve by construction.  The encoding is this project's own and canonical, ONE
 * encoding per point (vimz_amd/csrc/g16_point_pack.hpp).  G1, 4 little-endian words: x as an integer below q; bit 63 of word 3 is INF, bit 62 SIGN = 1 iff the
 * canonical y is greater than (q - 1)/2; the identity is INF alone (word 3 = 2^63, every other bit 0).  G2, 8 words: x.c0 then x.c1, the flags in the top bits of word
 * 7, the top two bits of word 3 zero; SIGN = 1 iff y is the larger of (y, -y): y.c1 > (q - 1)/2 when y.c1 != 0, y.c0 > (q - 1)/2 otherwise.  The unpacked side is the
 * affine layout every other point call takes (G1: x, y in 8 words; G2: x.c0, x.c1, y.c0, y.c1 in 16; the identity as zeros) in `form`; the packed side is always
 * canonical.  Membership of G2's subgroup of order r is NOT judged here — a point that unpacks is on the twist, no more; it stays where it is judged today
 * (vimz_decider_key_load for the verifying part, vimz_powers_verify, vimz_decider_key_verify_origin).
 * _pack / _unpack: n points of `group` (1: G1, 2: G2) through the device in chunks of at most VIMZ_PACK_CHUNK points, one thread per point (peak device memory: one
 * chunk of input, output and flags — 100 MB for G1, 200 MB for G2).  Return VIMZ_OK whenever the points were judged: a finding is a verdict, not an error.  *result = 0:
 * done; otherwise the VIMZ_PACK_* bits of the point of lowest index that has a finding, that index in *first_bad, and NOTHING is written to the output.  _COORD: a
 * coordinate is not below q (when packing, y included);  _FLAGS: INF together with any other bit, or a stray top bit in a G2 word 3;  _OFF_CURVE: x^3 + b is no
 * square (unpacking), y^2 != x^3 + b (packing).  n = 0 is fine.  The output is written once everything was judged; packed_out may be `points` itself (it is the
 * smaller); any other overlap of input and output is refused.  seconds (optional) = {host, device with its copies}.  VIMZ_ERR_INVALID: a NULL pointer (seconds
 * apart; n = 0 included), an unknown group or form, overlapping buffers. */
#define VIMZ_PACK_CHUNK 1048576
#define VIMZ_PACK_COORD 0x1u
#define VIMZ_PACK_FLAGS 0x2u
#define VIMZ_PACK_OFF_CURVE 0x4u
int vimz_points_pack(vimz_ctx* ctx, int group, const uint64_t* points, size_t n, int form, uint64_t* packed_out, uint32_t* result, uint64_t* first_bad, double seconds[2]);
int vimz_points_unpack(vimz_ctx* ctx, int group, const uint64_t* packed, size_t n, int form, uint64_t* points_out, uint32_t* result, uint64_t* first_bad, double seconds[2]);
/* A saved decider key in half the bytes, and back, on key BYTES (a context is enough, as for vimz_decider_key_contribute).  The packed key: magic "VG16KPK1", words 1..10
 * of the key verbatim (m, n_pub, n_c, n, len_z, mode, pp_hash), then every point of the key in the key's own order, packed: the KZG [tau]G2, alpha1, beta1, delta1,
 * beta2, gamma2, delta2, IC, a, b1, l, h, b2 — 55 + 4·((n_pub + 1) + 2m + (m - n_pub - 1) + (n - 1)) + 8m words, 11 + (the key's words - 11)/2; the size follows from the
 * header alone and is checked against `len` before anything is indexed.  IC‖a‖b1‖l‖h go through the device as one run of G1, b2 as one run of G2; the seven fixed
 * points are the host's.  unpack(pack(k)) == k byte for byte for every key vimz_decider_key_save writes (zero slots of b2 and of untouched wires included: the
 * identity packs as INF), and pack(unpack(p)) == p for every packed blob that unpacks.
 * Return the byte size of the output, or a negative error.  A NULL `out` or a short `cap` returns the size and writes nothing.  *result = 0: done; otherwise the
 * VIMZ_PACK_* bits of the first point (in the blob's order) that has a finding, first_bad = {the point's offset in 64-bit words in the SOURCE blob, those bits}, and
 * nothing is written.  `out` may be the input itself (cap says it is large enough); any other overlap is refused.  VIMZ_ERR_INVALID with a message: a NULL pointer,
 * a blob with the wrong magic or length, overlapping buffers.  vimz_decider_key_save's layout and every call that takes it are unchanged. */
int64_t vimz_decider_key_pack(vimz_ctx* ctx, const void* key, size_t len, void* out, size_t cap, uint32_t* result, uint64_t first_bad[2]);
int64_t vimz_decider_key_unpack(vimz_ctx* ctx, const void* packed, size_t len, void* out, size_t cap, uint32_t* result, uint64_t first_bad[2]);
/* Decider::prove for the IVC proof `ivc` holds (same shapes and keys as the decider's prover; left unchanged; at least one step): final fold, KZG
 * openings, Groth16 proof.  words_out: the 25 calldata words (vimz_amd/calldata.py names them), public_out: the info[2] public inputs; canonical,
 * 4 little-endian limbs each.  VIMZ_ERR_UNSAT when the proof does not satisfy the decider's statement (full decider: including a running CycleFold
 * witness that violates its relation or does not open its commitments).
 * seconds (optional) = {final fold + KZG openings, witness + sparse products on the host, NTTs, multi-scalar multiplications, total, 0} */
int vimz_decider_prove(vimz_decider* d, vimz_cf* ivc, uint64_t* public_out, uint64_t words_out[100], double seconds[6]);
/* Decider::verify (verify_final_proof, decider.rs:31-50): the checks of contracts/ContrastVerifier.sol:685-783 on (steps, z_0, z_i, 25 words).
 * *result = 0: accepted; else bits: 1 fewer than two steps, 2 KZG opening of cmW, 4 of cmE, 8 Groth16, 16 a word pair is not a curve point. */
int vimz_decider_verify(const vimz_decider* d, uint64_t steps, const uint64_t* z0, const uint64_t* zi, const uint64_t words[100], uint32_t* result);
/* the same against a key given as words (vimz_decider_vk's layout): no context, no GPU */
int vimz_decider_verify_key(const uint64_t* key_words, size_t n_key_words, uint64_t steps, const uint64_t* z0, const uint64_t* zi, uint32_t len_z,
                            const uint64_t words[100], uint32_t* result);
/* MANY proofs under one key in one call — the receiving side of a decider proof: a contract's marketplace, an indexer that refuses bad calldata before it pays
 * gas.  key_words: vimz_decider_vk's layout; steps: n; z0, zi: n·len_z elements; words: n·25 elements (4 little-endian limbs each).  results[i] is what
 * vimz_decider_verify_key returns in *result for proof i alone, for every input: the same bits, its early returns included (malformed words give 16 and nothing
 * else, a public element not below r gives 8 without the KZG bits, steps < 2 gives bit 1 and the checks go on).
 * Proofs that pass the per-proof stage are cut into chunks of `chunk` (0: 256).  Under three 128-bit multipliers a proof from the OS, wiped after use on host
 * and device, a chunk is accepted iff ONE product of Miller values is one after ONE final exponentiation (vimz_amd/csrc/decider_batch.hpp states it; wrong with
 * probability about 2^-128); a refused chunk is bisected: the same equation is asked of halves from the rows and Miller values that are already there, a member is
 * accepted only inside a subset whose equation was evaluated and held, and a refused subset of at most `leaf` members is judged member by member by the single
 * verifier on the host's threads (at most 2·(chunk − 1) subset equations a refused chunk; vimz_decider_verify_batch_ex has the switches and the counts).
 * Every proof's B passes "on the twist" and r·B = O by itself before it enters a product.
 * ctx != NULL: what grows with the batch runs on the GPU — the curve and subgroup flags of every point (k_powers_flags), twelve G1 scalar multiplications a proof
 * and the per-chunk sums (k_g1_lincomb, k_col_runs), one Miller loop a proof (k_miller: homogeneous projective steps, sparse line products) —, the five
 * fixed-G2 Miller loops and the final exponentiation of each chunk on the host.  ctx == NULL: every device stage is its host loop over the same per-thread
 * functions on up to 16 threads — the path of a machine without a GPU.  n == 0 is VIMZ_OK.  A NULL pointer, an unparsable key or a len_z that is not the key's:
 * VIMZ_ERR_INVALID with a message (vimz_last_error(ctx); of the calling thread when ctx is NULL).
 * seconds (optional) = {parse + per-proof host work, per-proof device stage, Miller loops, host sums + fixed-G2 loops + final exponentiations, fallback (the
 * subset equations of refused chunks and the single verifications), total} */
int vimz_decider_verify_batch(vimz_ctx* ctx, const uint64_t* key_words, size_t n_key_words, uint32_t len_z, size_t n, const uint64_t* steps, const uint64_t* z0,
                              const uint64_t* zi, const uint64_t* words, size_t chunk, uint32_t* results, double seconds[6]);
/* The batch verifiers' _ex entries: the entry of the same name with
 *   flags  VIMZ_BATCH_NO_BISECT: a refused chunk goes member by member to the single verifier, whole (any other bit: VIMZ_ERR_INVALID);
 *   leaf   a refused subset of at most `leaf` members goes to the single verifier; 0: the default (decider 128 on the device and 64 with
 *          ctx == NULL, compressed 1: profiles/batch_bisect.txt has the measurements behind them);
 *   stats  (optional) = {chunks refused, subset equations evaluated after a refusal (one a side asked: the compressed verifiers have two curves, and a subset is
 *          asked only on the sides its parent was refused on), single verifications run, members of refused chunks accepted by a subset equation}.
 * `results` are the same words whatever flags and leaf are: a member is accepted by an evaluated equation over a subset it lies in, or judged by the single
 * verifier (vimz_amd/csrc/batch_bisect.hpp).  The entries without _ex are these with flags = 0, leaf = 0, stats = NULL.  The compressed verifiers' twins are
 * vimz_ivc_verify_batch_compressed_ex and vimz_cf_verify_batch_compressed_ex ("verify_batch" as the decider's entry has it). */
#define VIMZ_BATCH_NO_BISECT 1u
int vimz_decider_verify_batch_ex(vimz_ctx* ctx, const uint64_t* key_words, size_t n_key_words, uint32_t len_z, size_t n, const uint64_t* steps, const uint64_t* z0,
                                 const uint64_t* zi, const uint64_t* words, size_t chunk, uint32_t* results, double seconds[6], uint32_t flags, size_t leaf,
                                 uint64_t stats[4]);

/* ---- ONE proof object out of several row segments: the "host-side sequential final fold" of BASELINE.json's north_star for IVC proofs.
 *      fold_input returns ONE RecursiveSNARK (vimz/src/nova_snark_backend/folding.rs:27-43); row segments of an image folded
 *      concurrently (S proofs on one GPU, or one per GPU) are merged into one verifiable object by out-of-circuit NIFS on both curves —
 *      the final fold CompressedSNARK::prove performs on the last fresh secondary instance (mod.rs:56-59), extended to S segments
 *      (protocol: vimz_amd/csrc/merge_internal.hpp; ours, like the augmented circuits).  The verifier replays the
 *      segments' hash checks, their adjacency and the fold tree from the records, then checks ONE primary and ONE secondary relaxed
 *      instance (or one compressed argument each).  The cross terms, their commitments and the vector folds run on the GPU. -------- */
typedef struct vimz_ivc_merged vimz_ivc_merged;
/* the merged proof of one segment; `segment` is left unchanged and supplies shapes / keys / context: keep it alive while the object is
 * in use (freeing it first orphans the object: its buffers are released, every later call on it fails, freeing it stays safe) */
int vimz_ivc_merged_create(vimz_ivc* segment, vimz_ivc_merged** out);
void vimz_ivc_merged_free(vimz_ivc_merged* m);
/* fold the proof of the NEXT row segment in (same device; read in place, left unchanged): it must start at the state m ends in */
int vimz_ivc_merge(vimz_ivc_merged* m, vimz_ivc* next_segment);
/* the same for two merged proofs of adjacent runs of segments (e.g. one per GPU, brought over with vimz_ivc_merged_save / _load) */
int vimz_ivc_merge_merged(vimz_ivc_merged* m, vimz_ivc_merged* next);
/* fold_input in ONE call (folding.rs:27-43): `nsteps` rows from state z0 proven as n_segments contiguous segments — segment k by
 * segments[k]: IVCs of the same circuits, each on a context of its own on one device; they are reset by this call —, folded concurrently
 * (a host thread each) and merged into one object.  The segments' start states come from the state chain in its two parts: the row
 * digests of all but the last segment at once, each on its successor's context, then short serial host chains.
 * seconds (optional) = {waiting for start states, merge, total}. */
int vimz_ivc_fold_segments(vimz_ivc* const* segments, size_t n_segments, const uint64_t* z0, const uint64_t* step_inputs, size_t nsteps,
                           vimz_ivc_merged** out, double seconds[3]);
/* the same when the caller already holds the rows' digests (vimz_ivc_row_digests over exactly these rows, e.g. a rank of a sharded
 * proof that has just exchanged them with the other ranks); digests == NULL: as above */
int vimz_ivc_fold_segments_dg(vimz_ivc* const* segments, size_t n_segments, const uint64_t* z0, const uint64_t* step_inputs, size_t nsteps,
                              const uint64_t* digests, vimz_ivc_merged** out, double seconds[3]);
/* fold_input for a run of rows whose START STATE is not known yet — a rank of a sharded proof: the segments' fold calls begin at once, the rows' digests (what
 * vimz_ivc_row_digests returns for them) are handed out as soon as the calls' own chain passes have produced them, the caller exchanges digests with the other
 * ranks, chains over the rows before its own (vimz_ivc_chain_from_digests) and provides the state; every row is hashed once.  _digests blocks; _finish joins the
 * folds, merges them into ONE object and frees the handle (out == NULL, or no start state given: cancels).  Circuits whose digests depend on the state: refused.
 * Between _begin and _start the segments hold their contexts (their folds wait for the state inside their calls): call nothing else on those IVCs meanwhile
 * (vimz_ivc_chain_from_digests is host-only and takes no context: fine). */
typedef struct vimz_ivc_pending vimz_ivc_pending;
int vimz_ivc_fold_segments_begin(vimz_ivc* const* segs, size_t n_seg, const uint64_t* step_inputs, size_t nsteps, vimz_ivc_pending** out);
int vimz_ivc_pending_digests(vimz_ivc_pending* p, uint64_t* digests_out);
int vimz_ivc_pending_start(vimz_ivc_pending* p, const uint64_t* z_start);
int vimz_ivc_pending_finish(vimz_ivc_pending* p, vimz_ivc_merged** out, double seconds[3]);
/* rows of a fold call of `nsteps` rows whose Poseidon chains the library would evaluate on the host (its policy, or what vimz_set_head_rows pinned) */
size_t vimz_head_rows_policy(size_t nsteps);
/* the same for a proof of `nsteps` rows made as concurrent segments (vimz_ivc_fold_segments): non-zero while its segments take head batches */
size_t vimz_head_rows_policy_segments(size_t nsteps);
/* RecursiveSNARK::verify(pp, num_steps, z0) for the merged object.  result: 0 = accepted; bit 0 / 1 a segment's primary / secondary chain
 * hash; bit 2 primary relaxed relation; bit 3 / 4 primary comm_W / comm_E; bit 5 secondary relation; bit 6 / 7 secondary comm_W / comm_E;
 * bit 10 public entries of a witness vector differ from the instance; bit 11 kept running products (bookkeeping for further merges);
 * bit 12 statement (total steps, initial state, or segments not adjacent); bit 13 malformed. */
int vimz_ivc_merged_verify(vimz_ivc_merged* m, uint64_t num_steps, const uint64_t* z0, uint32_t* result);
/* info = {steps, segments, ops, len_z, primary wires, primary constraints, secondary wires, secondary constraints} */
int vimz_ivc_merged_info(const vimz_ivc_merged* m, uint64_t info[8]);
int vimz_ivc_merged_state(const vimz_ivc_merged* m, uint64_t* z_start, uint64_t* z_end, uint64_t* steps);
/* seconds = {leaf work, wait for the cross-term commitments, folds + host instance arithmetic, total} */
int vimz_ivc_merged_profile(const vimz_ivc_merged* m, double seconds[4]);
/* The proof as bytes: records ‖ folded witnesses.  vimz_ivc_merged_load takes `vk` = any vimz_ivc created for the same step circuit
 * and keys (neither read nor changed; must outlive the object); the blob is untrusted (range and curve checks; instances recomputed). */
size_t vimz_ivc_merged_size(const vimz_ivc_merged* m);
int vimz_ivc_merged_save(vimz_ivc_merged* m, uint8_t* blob, size_t cap);
int vimz_ivc_merged_load(vimz_ivc* vk, const uint8_t* blob, size_t len, vimz_ivc_merged** out);
/* The same hand-over between two processes of ONE node without the host round trip (one rank per GPU; the ranks' final fold as a tree,
 * the counterpart of benchmark.sh:25-58's processes ending in one proof): _share writes a ticket — the records and a HIP IPC handle of
 * the object's device allocation (returns its size; copies when cap suffices) — that travels as a small message; _open_shared maps the
 * allocation, copies the folded witnesses AND the running products device-to-device (over xGMI between GPUs) into an object of its own
 * and unmaps it.  Records are checked as in _load; the products are taken as they are (vimz_ivc_merged_verify recomputes them).  The
 * sharing process keeps its object until the receiver is done.  Fails with VIMZ_ERR_HIP where IPC / peer access is unavailable: use
 * _save / _load then. */
int64_t vimz_ivc_merged_share(vimz_ivc_merged* m, void* ticket, size_t cap);
int vimz_ivc_merged_open_shared(vimz_ivc* vk, const uint8_t* ticket, size_t len, vimz_ivc_merged** out);
/* what an independent verifier replays: header {magic, segments, ops, len_z, n_w1, n_c1, n_w2, n_c2}, per segment {n, z_start, z_end,
 * U1 (W, E, u, X0, X1), U2, u2 (W, x0, x1), T}, per op {kind, leaf [, T_p, T_q]} — canonical little-endian words; returns the byte size */
int64_t vimz_ivc_merged_records(const vimz_ivc_merged* m, void* buf, size_t cap);
/* side 0 / 1; what = VIMZ_IX_RUNNING_Z, VIMZ_IX_RUNNING_E (canonical), VIMZ_IX_INSTANCE (comm_W, comm_E, u, X0, X1 of the folded instance) */
int64_t vimz_ivc_merged_export(vimz_ivc_merged* m, int side, int what, void* buf, size_t cap);
/* CompressedSNARK::{prove, verify} for the merged object: one argument for the folded primary and one for the folded secondary
 * instance (vimz_amd/csrc/spartan.hip); the blob carries the records.  result bits as vimz_ivc_verify_compressed, bit 2 / 3 = the
 * primary / secondary argument. */
size_t vimz_ivc_merged_compressed_size(const vimz_ivc_merged* m);
int vimz_ivc_merged_compress(vimz_ivc_merged* m, uint8_t* blob, size_t cap, double seconds[2]);
int vimz_ivc_verify_merged_compressed(vimz_ivc* vk, const uint8_t* blob, size_t len, uint64_t num_steps, const uint64_t* z0, uint32_t* result);

/* MANY compressed proofs under one verifier key in one call (vimz_amd/csrc/spartan_batch.hpp).  blobs[i] / lens[i]: a compressed proof of this family — the
 * first word tells its kind, one chain or merged, and the two may be mixed; a blob of the other family (or of neither) gets bit 13.  steps[i] and the len_z
 * elements at z0 + 4·len_z·i are proof i's statement.  results[i] is EXACTLY the word the matching single entry (vimz_ivc_verify_compressed /
 * vimz_ivc_verify_merged_compressed; vimz_cf_verify_compressed / vimz_cf_verify_merged_compressed) gives for proof i alone.
 * How: statement, chain hashes, record replay and every scalar check of an argument run per proof on the host's threads, by the single verifiers' own code; the
 * matrix evaluations M(ry) and the openings' s-vectors run on the GPU for groups of proofs; the openings' final group equations — linear in the proof's points,
 * the generator U and the key — are summed under non-zero 128-bit multipliers from the OS into ONE equation a curve a chunk: one MSM over the key, one over the
 * chunk's own points.  chunk: proofs an equation (0 = 32).  An accepted chunk adds no argument bits; a refused chunk, and any proof whose scalar checks fail
 * inside an argument, goes to the single verifier — the refused chunk through a bisection: the two equations are asked again of halves of the chunk, every
 * member under the multipliers it had and from the arguments already replayed (nothing is recomputed per proof), a half only on the curves its parent was refused
 * on; a member is accepted only inside a subset whose equations were evaluated and held, and a refused subset of at most `leaf` members is judged member by member
 * by the single verifier.  At most 2·(chunk − 1) subsets are asked of a refused chunk.  The _ex entries (see vimz_decider_verify_batch_ex) have the switches.
 * An error code ends the whole call and leaves `results` unspecified: a z0 element not below the modulus (checked for every member before anything is written),
 * no randomness from the OS, a HIP error.  n = 0 is accepted.  seconds[6] (optional): parse + host checks, half-tables, matrix evaluation, s-vector
 * accumulation, MSMs, fallback (the subset equations of refused chunks and the single verifications). */
int vimz_ivc_verify_compressed_batch(vimz_ivc* vk, size_t n, const uint8_t* const* blobs, const size_t* lens, const uint64_t* steps, const uint64_t* z0, size_t chunk,
                                     uint32_t* results, double seconds[6]);
int vimz_cf_verify_compressed_batch(vimz_cf* vk, size_t n, const uint8_t* const* blobs, const size_t* lens, const uint64_t* steps, const uint64_t* z0, size_t chunk,
                                    uint32_t* results, double seconds[6]);
int vimz_ivc_verify_batch_compressed_ex(vimz_ivc* vk, size_t n, const uint8_t* const* blobs, const size_t* lens, const uint64_t* steps, const uint64_t* z0, size_t chunk,
                                        uint32_t* results, double seconds[6], uint32_t flags, size_t leaf, uint64_t stats[4]);
int vimz_cf_verify_batch_compressed_ex(vimz_cf* vk, size_t n, const uint8_t* const* blobs, const size_t* lens, const uint64_t* steps, const uint64_t* z0, size_t chunk,
                                       uint32_t* results, double seconds[6], uint32_t flags, size_t leaf, uint64_t stats[4]);

/* Everything an independent verifier needs, canonical little-endian 4 x u64 per element (the parity tests hand these to the
 * CPU oracle's verifier).  side 0 = primary (BN254 Fr / G1), 1 = secondary (BN254 Fq / Grumpkin).
 *   what = VIMZ_CX_{A,B,C}_{ROWPTR,COL,COEF}, VIMZ_CX_DICT_CANON : the augmented circuit's R1CS
 *   what = VIMZ_IX_*  below.  Returns the byte size (copies when buf is large enough). */
#define VIMZ_IX_RUNNING_Z 100   /* running witness vector [u | W | X0 X1] (wire order) */
#define VIMZ_IX_RUNNING_E 101
#define VIMZ_IX_FRESH_Z 102     /* side 1 only: the last fresh secondary witness vector */
#define VIMZ_IX_INSTANCE 103    /* running instance: comm_W.x, comm_W.y, comm_E.x, comm_E.y, u, X0, X1  (7 elements; coordinates in the
                                   commitment curve's base field, u/X in this side's scalar field) */
#define VIMZ_IX_FRESH_INSTANCE 104  /* side 1 only: comm_W.x, comm_W.y, x0, x1 */
#define VIMZ_IX_LAST_STEP 107   /* vimz_cf_export, side 0: what the last step's F' was given and returned (layout: cyclefold.hip) */
#define VIMZ_IX_INFO 106        /* u64[4]: wires, constraints, step wires, step constraints */
#define VIMZ_IX_PARAMS 105      /* digest, z0..., z_i...  (1 + 2 len_z elements of this side's field; secondary len_z = 1) */
int64_t vimz_ivc_export(vimz_ivc* v, int side, int what, void* buf, size_t cap);
/* Host-only hooks for the parity tests of the verifier circuit itself (no GPU): build the augmented circuit of one side over a
 * trivial step circuit (z_out = z_in, arity 1), export it, and run its witness generator on given inputs.
 *   inputs (canonical elements): digest, i, z_0, z_i, U = (W.x, W.y, E.x, E.y, u, X0, X1), u = (W.x, W.y, x0, x1), T = (x, y)   -> 17 elements
 *   wires_out: n_wires elements (the full witness incl. the constant and the trivial step)
 *   outputs: U_new (7), rho (1), x0, x1 (2), flag (1: 1 = some range check failed)                                      -> 11 elements */
typedef struct vimz_augcircuit vimz_augcircuit;
int vimz_augcircuit_build(int side, vimz_augcircuit** out);
void vimz_augcircuit_free(vimz_augcircuit* c);
int64_t vimz_augcircuit_export(const vimz_augcircuit* c, int what, void* buf, size_t cap);   /* VIMZ_CX_* R1CS codes, VIMZ_IX_INFO */
int vimz_augcircuit_witness(const vimz_augcircuit* c, const uint64_t* inputs, uint64_t* wires_out, uint64_t* outputs);

/* ---- field-arithmetic probes (element-wise on the GPU; used by the parity tests to pin the device
 *      Montgomery arithmetic against the oracle).  op: 0 add, 1 sub, 2 mul, 3 inverse (b ignored). -------- */
int vimz_field_op(vimz_ctx* ctx, int field, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
/* group probes: out[i] = p[i] + q[i] (affine canonical in/out), through the device XYZZ formulas */
int vimz_curve_add(vimz_ctx* ctx, int curve, const uint64_t* p_xy, const uint64_t* q_xy, uint64_t* out_xy, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* VIMZ_HIP_H */
