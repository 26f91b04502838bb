// TESTING ONLY: one operation of the lazily reduced field (fp29.hpp) on raw operands, the same function on the host (tests/native/fp29_probe_host.cpp,
// compiled with g++) and on the device (vimz_test_fp29_probe in the testing library).  Operands and result are nine 29-bit limbs exactly as they stand —
// no conversion on the way in or out — so a test can hand over any representative an operation's contract admits and read back the representative it
// returns (tests/_fp29_ref.py holds the integer reference and the vectors).  Values of the 8 x 32 side (fp.hpp's form) use the first eight words of a
// slot; predicates write 0 / 1.  A slot is FP29_PROBE_WORDS words.
#pragma once
#include "fp29.hpp"

namespace vz {

constexpr int FP29_PROBE_WORDS = 9;
enum Fp29ProbeOp : int {
  FP29_OP_MUL = 0, FP29_OP_SQR = 1, FP29_OP_MUL_ADD2 = 2, FP29_OP_ADD = 3, FP29_OP_NEG = 4, FP29_OP_DBL = 5, FP29_OP_WEAK_REDUCE = 6, FP29_OP_CANON = 7,
  FP29_OP_IS_ZERO_MOD = 8, FP29_OP_UNPACK = 9 /* 9 limbs -> 8 words */, FP29_OP_PACK = 10 /* 8 words -> 9 limbs */, FP29_OP_FROM_STD = 11, FP29_OP_TO_STD = 12,
  FP29_OP_R29_OF = 13, FP29_OP_FE_OF29 = 14, FP29_OP_PACK_UNPACK = 15 /* pack(unpack(a)): the limbs again */,
  FP29_OP_SUB = 100 /* + K, for every K the tree instantiates */
};

// returns 0, or -1 for an operation it does not know (out is zeroed)
template <class P>
VZ_HD int fp29_probe(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* out) {
  typedef Fp29<P> G; typedef Fp<P> S;
  G x, y, z, w, r = G::zero();
  for (int i = 0; i < 9; i++) { x.v[i] = a[i]; y.v[i] = b[i]; z.v[i] = c[i]; w.v[i] = d[i]; }
  S s; for (int i = 0; i < 8; i++) s.v[i] = a[i];
  uint32_t w8[8]; bool words = false; int rc = 0;
  switch (op) {
    case FP29_OP_MUL: r = G::mul(x, y); break;
    case FP29_OP_SQR: r = G::sqr(x); break;
    case FP29_OP_MUL_ADD2: r = G::mul_add2(x, y, z, w); break;
    case FP29_OP_ADD: r = G::add(x, y); break;
    case FP29_OP_NEG: r = G::neg(x); break;
    case FP29_OP_DBL: r = G::dbl(x); break;
    case FP29_OP_WEAK_REDUCE: r = x.weak_reduce(); break;
    case FP29_OP_CANON: r = x.canon(); break;
    case FP29_OP_IS_ZERO_MOD: r.v[0] = x.is_zero_mod() ? 1u : 0u; break;
    case FP29_OP_UNPACK: x.unpack(w8); words = true; break;
    case FP29_OP_PACK: r = G::pack(a); break;
    case FP29_OP_FROM_STD: r = G::from_std(s); break;
    case FP29_OP_TO_STD: { const S t = x.to_std(); for (int i = 0; i < 8; i++) w8[i] = t.v[i]; words = true; break; }
    case FP29_OP_R29_OF: r = r29_of<S>(s); break;
    case FP29_OP_FE_OF29: { const S t = fe_of29<S>(x); for (int i = 0; i < 8; i++) w8[i] = t.v[i]; words = true; break; }
    case FP29_OP_PACK_UNPACK: x.unpack(w8); r = G::pack(w8); break;
    case FP29_OP_SUB + 1: r = G::template sub<1>(x, y); break;
    case FP29_OP_SUB + 2: r = G::template sub<2>(x, y); break;
    case FP29_OP_SUB + 3: r = G::template sub<3>(x, y); break;
    case FP29_OP_SUB + 4: r = G::template sub<4>(x, y); break;
    case FP29_OP_SUB + 6: r = G::template sub<6>(x, y); break;
    default: rc = -1; break;
  }
  if (words) { for (int i = 0; i < 8; i++) out[i] = w8[i]; out[8] = 0; }
  else for (int i = 0; i < 9; i++) out[i] = r.v[i];
  return rc;
}

template <class Fn>
inline int fp29_probe_field(int field, Fn fn) {
  switch (field) {
    case 0: return fn(BnFr());
    case 1: return fn(BnFq());
    case 2: return fn(PallasFp());
    case 3: return fn(VestaFq());
  }
  return -1;
}

}  // namespace vz
