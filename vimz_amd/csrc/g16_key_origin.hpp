// Judging that a saved decider key derives from a powers-of-tau string and the decider circuit (vimz_decider_key_verify_origin; g16_key_origin.hip; DESIGN.md §8
// item 5): what that file shares with groth16.hip — the set-up head and the string's conversion, which it calls and does not copy — and what other files call of it.
#pragma once
#include "g16_powers.hpp"
#include "g16_key_contrib.hpp"
#include "g16_key_origin_stage.hpp"

struct vimz_decider;
struct vimz_cf;

// ---- defined in groth16.hip -------------------------------------------------------------------------------------------------------------------------------
// what every set-up begins with: the decider circuit for the prover's shapes (light or full), the key's sizes, the domain's constants
int decider_setup_head(vimz_cf* v, const uint64_t kzg_vk_g2[16], bool light, vimz_decider& d);
// n points of a string as words (form = VIMZ_FORM_*) -> Montgomery coordinates.  0: fine; 1: a coordinate is not below q; 2: a point is not on its curve
template <class A> int string_points_in(const uint64_t* words, size_t n, int form, A* out);
// an empty decider for decider_setup_head to fill, and its end (vimz_decider is groth16.hip's)
vimz_decider* g16_decider_new();
void g16_decider_delete(vimz_decider* d);
// A circuit as the origin check reads it: the builder's three CSRs as they are (host), the dictionary in Montgomery form (8 words an entry), the sizes, and what
// the key's header must say.  whole_header: len_z and mode are compared too (the decider's circuit; a test's synthetic one has neither).
struct G16CircuitView {
  const uint32_t *row_ptr[3], *col[3], *coef[3]; size_t n_row_ptr[3], nnz[3];
  const uint32_t* dict; size_t n_dict;
  uint32_t m, n_pub, n_c; int logn;
  uint64_t len_z, mode, pp_hash[4]; bool whole_header;
};
void g16_decider_circuit(const vimz_decider& d, G16CircuitView* out);
// seconds of ONE host_spmv3 (the prover's sparse products on the host's threads) over that circuit's three matrices: recorded beside k_spmv3_dict's time
double g16_decider_host_spmv3_seconds(const vimz_decider& d);
// the domain of 2^logn points with the twiddle tables a key holds (device; made on `s` under the context's lock) and its UNSCALED inverse transform over scalars,
// in place on n Montgomery elements: the launches of the prover's ntt(.., inverse)
struct G16Domain;
int g16_domain_new(vimz_ctx* ctx, hipStream_t s, int logn, G16Domain** out);
void g16_domain_free(G16Domain* D);
void g16_domain_n_inv(const G16Domain* D, uint32_t out[8]);      // 1/n, Montgomery
hipError_t g16_domain_intt_unscaled(hipStream_t s, uint32_t* d, const G16Domain* D);
// device points (standard Montgomery coordinates) -> a key in the MSM's resident form, for vz_msm_device (synchronises the context's stream); freed without the
// context's lock, which the caller holds
int g16_bases_from_device(vimz_ctx* ctx, const G1Aff* d_pts, size_t n, vimz_bases** out);
void g16_bases_free_raw(vimz_bases* b);
// Σ wires[idx_i]·bases_i over n points of G2, bit plane by bit plane (groth16.hip: g2_msm): all on the device, wires in Montgomery form, canon 8 n words of scratch
int g16_g2_msm(vimz_ctx* ctx, hipStream_t s, const G2PowAff* bases, const uint32_t* wires, const uint32_t* idx, uint32_t n, uint32_t* canon, XYZZ<vz::pairing::Fq2>* out);

// ---- defined in g16_key_origin.hip ------------------------------------------------------------------------------------------------------------------------
// A circuit's three CSRs and its dictionary on the device: uploaded once per call by g16_spmv_upload (blocking copies; false with a message when an offset, a
// wire number or a coefficient index is out of its bounds — nothing is then on the device), freed by g16_spmv_free on every path.
struct SpmvDevice {
  uint32_t *row_ptr[3] = {nullptr, nullptr, nullptr}, *col[3] = {nullptr, nullptr, nullptr}, *coef[3] = {nullptr, nullptr, nullptr}, *dict = nullptr;
  uint32_t m = 0, n_c = 0;
};
hipError_t g16_spmv_upload(const G16CircuitView& c, SpmvDevice* dev, std::string* why);
void g16_spmv_free(SpmvDevice& dev);
// Queues on `s`: out_q[i] = (row i of matrix q)·v for q = A, B, C and i < n_c, zero for n_c <= i < n — ONE launch of k_spmv3_dict over a grid of (rows, 3):
// blockIdx.y picks the matrix, a thread owns its row (g16_key_origin_stage.hpp: spmv_dict_row).  v: m elements; out_q: n >= n_c elements each; Montgomery.
hipError_t g16_spmv3_dict(hipStream_t s, const SpmvDevice& dev, const uint32_t* v, size_t n, uint32_t* out_a, uint32_t* out_b, uint32_t* out_c);
