// points.hpp -- device helpers of point decompression and validation
// (points.hip; the sqrt test hooks of testhooks.hip run the same functions):
// square roots in Fq and Fq2, the sort-flag predicate of the zcash / ark
// compressed encodings and the prime-order subgroup tests ([r]P == O, and the
// endomorphism criteria of the proof decoder), one lane per point.
//
// Everything here runs a few thousand field products per point in loops over
// the bits of a fixed exponent or scalar.  The loops stay rolled and every
// product is a call of one out-of-line function per field (FqC / Fq2C below),
// so a kernel is a few KB of code around four product bodies instead of
// hundreds of KB of inlined multiplies; the exponent words are wave-uniform
// scalar loads.
#pragma once
#include "../../include/zkp.h"
#include "curve.hpp"

namespace zk {
// lanes per block of the one-lane-per-point kernels (points.hip, hash.hip)
constexpr int PT_BLOCK = 128;
}  // namespace zk

// ---- out-of-line products ------------------------------------------------
// Fq operands and results travel in VGPRs (24 argument registers); the Fq2
// product's 48 argument registers exceed the calling convention's 32, so the
// G2 kernels pass part of them through scratch (stated in DESIGN.md 2.10).
static __device__ __noinline__ Fq pt_fq_mul(Fq a, Fq b) { return fq_mul(a, b); }
static __device__ __noinline__ Fq pt_fq_sqr(Fq a) { return fp_sqr(a); }
static __device__ __noinline__ Fq2 pt_fq2_mul(Fq2 a, Fq2 b) { return fq2_mul(a, b); }
static __device__ __noinline__ Fq2 pt_fq2_sqr(Fq2 a) { return fq2_sqr(a); }

// Field types whose products are those calls, with the f_* shims of ff.hpp,
// so curve.hpp's XYZZ formulas are reused as they are.
struct FqC {
  Fq v;
};
struct Fq2C {
  Fq2 v;
};
ZK_DI FqC f_add(const FqC& a, const FqC& b) { return {fp_add(a.v, b.v)}; }
ZK_DI FqC f_sub(const FqC& a, const FqC& b) { return {fp_sub(a.v, b.v)}; }
ZK_DI FqC f_neg(const FqC& a) { return {fp_neg(a.v)}; }
ZK_DI FqC f_mul(const FqC& a, const FqC& b) { return {pt_fq_mul(a.v, b.v)}; }
ZK_DI FqC f_sqr(const FqC& a) { return {pt_fq_sqr(a.v)}; }
ZK_DI FqC f_mul_sub(const FqC& a, const FqC& b, const FqC& c, const FqC& d) {
  return {fp_sub(pt_fq_mul(a.v, b.v), pt_fq_mul(c.v, d.v))};
}
ZK_DI bool f_is_zero(const FqC& a) { return fp_is_zero(a.v); }
ZK_DI bool f_eq(const FqC& a, const FqC& b) { return fp_eq(a.v, b.v); }
ZK_DI void f_set_zero(FqC& a) { a.v = fp_zero<FqParams>(); }
ZK_DI void f_set_one(FqC& a) { a.v = fp_one<FqParams>(); }

ZK_DI Fq2C f_add(const Fq2C& a, const Fq2C& b) { return {fq2_add(a.v, b.v)}; }
ZK_DI Fq2C f_sub(const Fq2C& a, const Fq2C& b) { return {fq2_sub(a.v, b.v)}; }
ZK_DI Fq2C f_neg(const Fq2C& a) { return {fq2_neg(a.v)}; }
ZK_DI Fq2C f_mul(const Fq2C& a, const Fq2C& b) { return {pt_fq2_mul(a.v, b.v)}; }
ZK_DI Fq2C f_sqr(const Fq2C& a) { return {pt_fq2_sqr(a.v)}; }
ZK_DI Fq2C f_mul_sub(const Fq2C& a, const Fq2C& b, const Fq2C& c, const Fq2C& d) {
  return {fq2_sub(pt_fq2_mul(a.v, b.v), pt_fq2_mul(c.v, d.v))};
}
ZK_DI bool f_is_zero(const Fq2C& a) { return fq2_is_zero(a.v); }
ZK_DI bool f_eq(const Fq2C& a, const Fq2C& b) { return fp_eq(a.v.c0, b.v.c0) && fp_eq(a.v.c1, b.v.c1); }
ZK_DI void f_set_zero(Fq2C& a) { a.v = fq2_zero(); }
ZK_DI void f_set_one(Fq2C& a) { a.v = fq2_one(); }

// ---- canonical-value predicates -------------------------------------------
// c >= p (c any 384-bit value)
ZK_DI bool pt_fq_geq_p(const Fq& c) {
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i < 12; i++) (void)__builtin_subc(c.v[i], FqParams::MOD[i], br, &br);
  return br == 0;
}
// The encodings' sort flag on a CANONICAL value: c > (p - 1) / 2
ZK_DI bool pt_fq_largest(const Fq& c) {
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i < 12; i++) (void)__builtin_subc(FQ_PM1_DIV2_32[i], c.v[i], br, &br);
  return br != 0;
}
// Fq2: the same test on c1, or on c0 when c1 == 0 (canonical coefficients)
ZK_DI bool pt_fq2_largest(const Fq2& c) { return fp_is_zero(c.c1) ? pt_fq_largest(c.c0) : pt_fq_largest(c.c1); }

ZK_DI Fq pt_to_mont(const Fq& c) { return pt_fq_mul(c, fp_from_const<FqParams>(FqParams::R2)); }
ZK_DI Fq pt_from_mont(const Fq& a) {
  Fq one = fp_zero<FqParams>();
  one.v[0] = 1;
  return pt_fq_mul(a, one);
}

// ---- exponentiation ---------------------------------------------------------
// a^e for a fixed 384-bit exponent e (12 little-endian words, the same for
// every lane): square and multiply from the top bit, rolled.
template <class F>
ZK_DI F pt_pow(const F& a, const uint32_t* e) {
  F acc;
  f_set_one(acc);
  for (int b = 383; b >= 0; b--) {
    acc = f_sqr(acc);
    if ((e[b >> 5] >> (b & 31)) & 1) acc = f_mul(acc, a);
  }
  return acc;
}

// ---- square roots (Montgomery form in and out) ------------------------------
// p = 3 mod 4: a^((p+1)/4) is a root when a is a square
ZK_DI bool pt_fq_sqrt(const Fq& a, Fq& out) {
  out = pt_pow(FqC{a}, FQ_SQRT_EXP32).v;
  return fp_eq(pt_fq_sqr(out), a);
}
// Fq2: the "complex method" (Adj and Rodriguez-Henriquez, "Square root
// computation over even extension fields", Algorithm 9), as host_pairing.hpp's
// sqrt_fq2: a1 = a^((p-3)/4), alpha = a1^2 a, x0 = a1 a;  alpha^(p+1) = -1: no
// root;  alpha = -1: u x0;  else (1 + alpha)^((p-1)/2) x0.
ZK_DI bool pt_fq2_sqrt(const Fq2& a, Fq2& out) {
  const Fq2C a1 = pt_pow(Fq2C{a}, FQ_PM3_DIV4_32);
  const Fq2C x0 = f_mul(a1, Fq2C{a});
  const Fq2C alpha = f_mul(a1, x0);
  const Fq minus_one = fp_neg(fp_one<FqParams>());
  // conj(alpha) alpha = c0^2 + c1^2, an element of Fq
  const Fq norm = fp_add(pt_fq_sqr(alpha.v.c0), pt_fq_sqr(alpha.v.c1));
  if (fp_eq(norm, minus_one)) return false;
  if (fp_eq(alpha.v.c0, minus_one) && fp_is_zero(alpha.v.c1)) {
    out = {fp_neg(x0.v.c1), x0.v.c0};
  } else {
    Fq2C t = alpha;
    t.v.c0 = fp_add(t.v.c0, fp_one<FqParams>());
    out = f_mul(pt_pow(t, FQ_PM1_DIV2_32), x0).v;
  }
  return f_eq(f_sqr(Fq2C{out}), Fq2C{a});
}

// ---- curve and subgroup -------------------------------------------------------
// y^2 = x^3 + b: b = 4 (G1), 4 (1 + u) (G2)
ZK_DI FqC pt_curve_b(const FqC&) {
  const Fq two = fp_dbl(fp_one<FqParams>());
  return {fp_dbl(two)};
}
ZK_DI Fq2C pt_curve_b(const Fq2C&) {
  const Fq four = fp_dbl(fp_dbl(fp_one<FqParams>()));
  return {{four, four}};
}
template <class F>
ZK_DI F pt_curve_rhs(const F& x) { return f_add(f_mul(f_sqr(x), x), pt_curve_b(x)); }

// [r]P == O by double-and-add over the bits of r (the contract of ark's
// Validate::Yes, host_pairing.hpp's in_subgroup): every lane walks the same
// bits, so the loop does not diverge; the additions are mixed (P stays
// affine) and madd's own branches cover the accumulator reaching O, P or -P
// on the way (points of small order).  P: on the curve, not the identity.
template <class F>
ZK_DI bool pt_in_subgroup(const Affine<F>& P) {
  XYZZ<F> acc = xyzz_from_aff(P);   // bit 254 of r
  for (int b = 253; b >= 0; b--) {
    acc = xyzz_dbl(acc);
    if ((FR_MOD32[b >> 5] >> (b & 31)) & 1) acc = xyzz_madd(acc, P);
  }
  return xyzz_is_inf(acc);
}

// ---- subgroup by endomorphism (the proof decoder, points.hip) -------------------
// Scott, "A note on group membership tests for G1, G2 and GT on BLS
// pairing-friendly curves": for P on the curve, with x = -BLS_X_ABS,
//   G1: P in G1 iff phi(P) = -[x^2] P,  phi(x, y) = (beta x, y)
//   G2: P in G2 iff psi(P) = [x] P = -[|x|] P,  psi(x, y) = (conj(x) PSI_X, conj(y) PSI_Y)
// (constants and their generator identities: gen_constants.py).  Equivalent
// to [r]P == O above, with 2 x 63 (G1) / 63 (G2) doublings and 5 additions per
// pass instead of 254 and 133.
//
// [|x|] B for B affine (mixed additions) or XYZZ (the second pass of G1,
// whose base is the first pass's result): bit 63 of |x| is the start value,
// the other 63 bits a rolled loop over the wave-uniform word.  The formulas'
// own branches cover an accumulator meeting O, B or -B (small-order points).
template <class F>
ZK_DI XYZZ<F> pt_endo_start(const Affine<F>& b) { return xyzz_from_aff(b); }
template <class F>
ZK_DI XYZZ<F> pt_endo_start(const XYZZ<F>& b) { return b; }
template <class F>
ZK_DI XYZZ<F> pt_endo_add(const XYZZ<F>& a, const Affine<F>& b) { return xyzz_madd(a, b); }
template <class F>
ZK_DI XYZZ<F> pt_endo_add(const XYZZ<F>& a, const XYZZ<F>& b) { return xyzz_add(a, b); }
template <class F, class B>
__device__ __noinline__ XYZZ<F> pt_mul_x_abs(const B* base) {
  static_assert(BLS_X_ABS >> 63, "the loop starts below the top bit of |x|");
  XYZZ<F> acc = pt_endo_start(*base);
#pragma unroll 1
  for (int b = 62; b >= 0; b--) {
    acc = xyzz_dbl(acc);
    if ((BLS_X_ABS >> b) & 1) acc = pt_endo_add(acc, *base);
  }
  return acc;
}
// (px, py) == -Q without an inversion: px ZZ == X, py ZZZ == -Y, Q finite.
// Q == O means "not in the subgroup": the affine P that reaches the test is
// never the identity, and |x|, x^2 are not multiples of r.
template <class F>
ZK_DI bool pt_eq_neg(const F& px, const F& py, const XYZZ<F>& Q) {
  if (xyzz_is_inf(Q)) return false;
  return f_eq(f_mul(px, Q.ZZ), Q.X) && f_is_zero(f_add(f_mul(py, Q.ZZZ), Q.Y));
}
// P: on the curve, not the identity (as pt_in_subgroup)
ZK_DI bool pt_in_subgroup_endo(const Affine<FqC>& P) {
  const XYZZ<FqC> t = pt_mul_x_abs<FqC>(&P);
  if (xyzz_is_inf(t)) return false;
  const XYZZ<FqC> q = pt_mul_x_abs<FqC>(&t);   // [x^2] P
  return pt_eq_neg(f_mul(P.x, FqC{fp_from_const<FqParams>(ENDO_BETA32)}), P.y, q);
}
ZK_DI bool pt_in_subgroup_endo(const Affine<Fq2C>& P) {
  const XYZZ<Fq2C> q = pt_mul_x_abs<Fq2C>(&P);   // [|x|] P = -[x] P
  const Fq2C cx = {{P.x.v.c0, fp_neg(P.x.v.c1)}}, cy = {{P.y.v.c0, fp_neg(P.y.v.c1)}};
  const Fq2C kx = {{fp_from_const<FqParams>(ENDO_PSI_X32[0]), fp_from_const<FqParams>(ENDO_PSI_X32[1])}};
  const Fq2C ky = {{fp_from_const<FqParams>(ENDO_PSI_Y32[0]), fp_from_const<FqParams>(ENDO_PSI_Y32[1])}};
  return pt_eq_neg(f_mul(cx, kx), f_mul(cy, ky), q);
}
