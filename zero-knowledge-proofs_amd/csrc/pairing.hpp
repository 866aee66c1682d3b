// pairing.hpp -- the BLS12-381 optimal ate pairing on the device, one lane per
// pairing product (pairing.hip; the tower hooks of testhooks.hip run the same
// functions).  The pairing is host_pairing.hpp's: the tower
//   Fq2 = Fq[u]/(u^2 + 1), Fq6 = Fq2[v]/(v^3 - xi), xi = 1 + u, Fq12 = Fq6[w]/(w^2 - v),
// coefficients in the host's order (c0.c0.c0, c0.c0.c1, c0.c1.c0, ...), G2 on
// the M-type twist, loop parameter x = -BLS_X_ABS.
//
// Shape.  Every Fq2 product is one of points.hpp's out-of-line bodies
// (Fq2C), every Fq6 / Fq12 operation is an out-of-line function on pointers,
// and all loops (the 63 bits of |x|, the exponent of the Fq inversion) stay
// rolled with wave-uniform loop words, so a kernel is a few tens of KB of
// code.  An Fq12 is 144 dwords: f and the temporaries of the tower live in
// the lane's private (scratch) memory and only Fq2 operands are in registers
// (DESIGN.md 2.11).
//
// Lines.  A line has the sparse shape of host_pairing.hpp's line_eval:
//   l = l[0] + l[1] v + l[2] v w        (c0.c0, c0.c1, c1.c1).
// The on-the-fly lines of a variable G2 point are projective: the host's
// affine line times an Fq2 factor (2 U ZZZ for a doubling, P ZZZ for an
// addition, in the XYZZ formulas' names).  Fq2 is a proper subfield of Fq12,
// so the factor vanishes in the final exponentiation, like the w^3 the host
// line already carries.
//
// Final exponentiation.  Easy part f^((p^6 - 1)(p^2 + 1)), then the hard part
// as the x-power chain
//   (x - 1)^2 (x + p) (x^2 + p^2 - 1) + 3 = 3 (p^4 - p^2 + 1) / r
// (asserted by gen_constants.py), with Granger-Scott cyclotomic squarings.
// The device therefore computes f^(PR_FINAL_EXP_C (p^12 - 1) / r) with
// PR_FINAL_EXP_C = 3; 3 is coprime to r, so "== 1" is the host's verdict.
#pragma once
#include <vector>

#include "points.hpp"

constexpr int PR_FINAL_EXP_C = 3;
constexpr int PR_STEPS = 68;   // 63 doubling and 5 addition steps of the Miller loop

using F2 = Fq2C;
struct F6 {
  F2 c0, c1, c2;
};
struct F12 {
  F6 c0, c1;
};
// position k of coefficient j (memory order) in powers of w: a = sum_j co[j] w^PR_WPOW[j]
static constexpr int PR_WPOW[6] = {0, 2, 4, 1, 3, 5};

// ---- Fq2 helpers -------------------------------------------------------------
ZK_DI F2 f2_mul_xi(const F2& a) { return {{fp_sub(a.v.c0, a.v.c1), fp_add(a.v.c0, a.v.c1)}}; }   // (1 + u) a
ZK_DI F2 f2_dbl(const F2& a) { return f_add(a, a); }
ZK_DI F2 f2_conj(const F2& a) { return {{a.v.c0, fp_neg(a.v.c1)}}; }
ZK_DI F2 f2_mul_fq(const F2& a, const Fq& k) { return {{pt_fq_mul(a.v.c0, k), pt_fq_mul(a.v.c1, k)}}; }
ZK_DI Fq pr_fq_inv(const Fq& a) { return pt_pow(FqC{a}, FQ_INV_EXP32).v; }   // a^(p - 2), 0 -> 0
ZK_DI F2 f2_inv(const F2& a) {
  const Fq n = pr_fq_inv(fp_add(pt_fq_sqr(a.v.c0), pt_fq_sqr(a.v.c1)));
  return {{pt_fq_mul(a.v.c0, n), fp_neg(pt_fq_mul(a.v.c1, n))}};
}
ZK_DI F2 f2_load(const uint32_t* w) {
  F2 r;
#pragma unroll
  for (int i = 0; i < 12; i++) {
    r.v.c0.v[i] = w[i];
    r.v.c1.v[i] = w[12 + i];
  }
  return r;
}
ZK_DI Fq pr_fq_load(const uint32_t* w) {
  Fq r;
#pragma unroll
  for (int i = 0; i < 12; i++) r.v[i] = w[i];
  return r;
}

// ---- Fq6 ---------------------------------------------------------------------
// (results may alias operands: every operand is read before the first store)
static __device__ __noinline__ void f6_add(F6* r, const F6* a, const F6* b) {
  const F2 t0 = f_add(a->c0, b->c0), t1 = f_add(a->c1, b->c1), t2 = f_add(a->c2, b->c2);
  r->c0 = t0; r->c1 = t1; r->c2 = t2;
}
static __device__ __noinline__ void f6_sub(F6* r, const F6* a, const F6* b) {
  const F2 t0 = f_sub(a->c0, b->c0), t1 = f_sub(a->c1, b->c1), t2 = f_sub(a->c2, b->c2);
  r->c0 = t0; r->c1 = t1; r->c2 = t2;
}
static __device__ __noinline__ void f6_neg(F6* r, const F6* a) {
  const F2 t0 = f_neg(a->c0), t1 = f_neg(a->c1), t2 = f_neg(a->c2);
  r->c0 = t0; r->c1 = t1; r->c2 = t2;
}
// v a
ZK_DI void f6_mul_v(F6* r, const F6* a) {
  const F2 t0 = f2_mul_xi(a->c2), t1 = a->c0, t2 = a->c1;
  r->c0 = t0; r->c1 = t1; r->c2 = t2;
}
// Karatsuba over Fq2: 6 products
static __device__ __noinline__ void f6_mul(F6* r, const F6* a, const F6* b) {
  const F2 v0 = f_mul(a->c0, b->c0), v1 = f_mul(a->c1, b->c1), v2 = f_mul(a->c2, b->c2);
  const F2 t0 = f_mul(f_add(a->c1, a->c2), f_add(b->c1, b->c2));
  const F2 t1 = f_mul(f_add(a->c0, a->c1), f_add(b->c0, b->c1));
  const F2 t2 = f_mul(f_add(a->c0, a->c2), f_add(b->c0, b->c2));
  r->c0 = f_add(v0, f2_mul_xi(f_sub(f_sub(t0, v1), v2)));
  r->c1 = f_add(f_sub(f_sub(t1, v0), v1), f2_mul_xi(v2));
  r->c2 = f_add(f_sub(f_sub(t2, v0), v2), v1);
}
// a (x + y v): 6 products
static __device__ __noinline__ void f6_mul_01(F6* r, const F6* a, const F2* x, const F2* y) {
  const F2 t0 = f_add(f_mul(a->c0, *x), f2_mul_xi(f_mul(a->c2, *y)));
  const F2 t1 = f_add(f_mul(a->c1, *x), f_mul(a->c0, *y));
  const F2 t2 = f_add(f_mul(a->c2, *x), f_mul(a->c1, *y));
  r->c0 = t0; r->c1 = t1; r->c2 = t2;
}
// a (z v): 3 products
static __device__ __noinline__ void f6_mul_1(F6* r, const F6* a, const F2* z) {
  const F2 t0 = f2_mul_xi(f_mul(a->c2, *z)), t1 = f_mul(a->c0, *z), t2 = f_mul(a->c1, *z);
  r->c0 = t0; r->c1 = t1; r->c2 = t2;
}
// 1 / a through the norm to Fq2, then to Fq (one Fermat inversion)
static __device__ __noinline__ void f6_inv(F6* r, const F6* a) {
  const F2 t0 = f_sub(f_sqr(a->c0), f2_mul_xi(f_mul(a->c1, a->c2)));
  const F2 t1 = f_sub(f2_mul_xi(f_sqr(a->c2)), f_mul(a->c0, a->c1));
  const F2 t2 = f_sub(f_sqr(a->c1), f_mul(a->c0, a->c2));
  const F2 n = f_add(f_mul(a->c0, t0), f2_mul_xi(f_add(f_mul(a->c2, t1), f_mul(a->c1, t2))));
  const F2 ni = f2_inv(n);
  r->c0 = f_mul(t0, ni);
  r->c1 = f_mul(t1, ni);
  r->c2 = f_mul(t2, ni);
}

// ---- Fq12 --------------------------------------------------------------------
ZK_DI void f12_set_one(F12* r) {
  F2 z, o;
  f_set_zero(z);
  f_set_one(o);
  r->c0.c0 = o; r->c0.c1 = z; r->c0.c2 = z;
  r->c1.c0 = z; r->c1.c1 = z; r->c1.c2 = z;
}
ZK_DI bool f12_is_one(const F12* a) {
  F2 o;
  f_set_one(o);
  return f_eq(a->c0.c0, o) && f_is_zero(a->c0.c1) && f_is_zero(a->c0.c2) && f_is_zero(a->c1.c0) &&
         f_is_zero(a->c1.c1) && f_is_zero(a->c1.c2);
}
// a^(p^6)
static __device__ __noinline__ void f12_conj(F12* r, const F12* a) {
  r->c0 = a->c0;
  f6_neg(&r->c1, &a->c1);
}
// Karatsuba over Fq6: 18 Fq2 products
static __device__ __noinline__ void f12_mul(F12* r, const F12* a, const F12* b) {
  F6 t0, t1, s, u;
  f6_mul(&t0, &a->c0, &b->c0);
  f6_mul(&t1, &a->c1, &b->c1);
  f6_add(&s, &a->c0, &a->c1);
  f6_add(&u, &b->c0, &b->c1);
  f6_mul(&s, &s, &u);
  f6_sub(&s, &s, &t0);
  f6_sub(&r->c1, &s, &t1);
  f6_mul_v(&t1, &t1);
  f6_add(&r->c0, &t0, &t1);
}
// complex squaring: 12 Fq2 products
static __device__ __noinline__ void f12_sqr(F12* r, const F12* a) {
  F6 t, s, u;
  f6_mul(&t, &a->c0, &a->c1);
  f6_add(&s, &a->c0, &a->c1);
  f6_mul_v(&u, &a->c1);
  f6_add(&u, &u, &a->c0);
  f6_mul(&s, &s, &u);          // (a0 + a1)(a0 + v a1) = a0^2 + v a1^2 + (1 + v) a0 a1
  f6_sub(&s, &s, &t);
  f6_mul_v(&u, &t);
  f6_sub(&r->c0, &s, &u);
  f6_add(&r->c1, &t, &t);
}
static __device__ __noinline__ void f12_inv(F12* r, const F12* a) {
  F6 t0, t1;
  f6_mul(&t0, &a->c0, &a->c0);
  f6_mul(&t1, &a->c1, &a->c1);
  f6_mul_v(&t1, &t1);
  f6_sub(&t0, &t0, &t1);       // a0^2 - v a1^2
  f6_inv(&t0, &t0);
  f6_mul(&t1, &a->c1, &t0);
  f6_mul(&r->c0, &a->c0, &t0);
  f6_neg(&r->c1, &t1);
}
// f (l[0] + l[1] v + l[2] v w): 15 Fq2 products
static __device__ __noinline__ void f12_mul_line(F12* f, const F2* l) {
  F6 t0, t1, s;
  const F2 bc = f_add(l[1], l[2]);
  f6_mul_01(&t0, &f->c0, &l[0], &l[1]);
  f6_mul_1(&t1, &f->c1, &l[2]);
  f6_add(&s, &f->c0, &f->c1);
  f6_mul_01(&s, &s, &l[0], &bc);
  f6_sub(&s, &s, &t0);
  f6_sub(&f->c1, &s, &t1);
  f6_mul_v(&t1, &t1);
  f6_add(&f->c0, &t0, &t1);
}
// a^p: coefficient j of w^k becomes conj(a_j) xi^(k (p - 1) / 6)
static __device__ __noinline__ void f12_frob1(F12* r, const F12* a) {
  const F2* s = &a->c0.c0;
  F2* d = &r->c0.c0;
#pragma unroll 1
  for (int j = 0; j < 6; j++) d[j] = f_mul(f2_conj(s[j]), f2_load(FROB1_32[PR_WPOW[j]]));
}
// a^(p^2): the coefficients xi^(k (p^2 - 1) / 6) lie in Fq
static __device__ __noinline__ void f12_frob2(F12* r, const F12* a) {
  const F2* s = &a->c0.c0;
  F2* d = &r->c0.c0;
#pragma unroll 1
  for (int j = 0; j < 6; j++) d[j] = f2_mul_fq(s[j], pr_fq_load(FROB2_32[PR_WPOW[j]]));
}
// (x + y s)^2 in Fq4 = Fq2[s]/(s^2 - xi): re = x^2 + xi y^2, im = 2 x y
ZK_DI void pr_fq4_sqr(const F2& x, const F2& y, F2& re, F2& im) {
  const F2 x2 = f_sqr(x), y2 = f_sqr(y);
  im = f_sub(f_sub(f_sqr(f_add(x, y)), x2), y2);
  re = f_add(x2, f2_mul_xi(y2));
}
// a^2 for a in the cyclotomic subgroup (Granger-Scott): 9 Fq2 squarings
static __device__ __noinline__ void f12_cyc_sqr(F12* r, const F12* a) {
  F2 t0, t1, t2, t3, t4, t5;
  pr_fq4_sqr(a->c0.c0, a->c1.c1, t0, t1);
  pr_fq4_sqr(a->c1.c0, a->c0.c2, t2, t3);
  pr_fq4_sqr(a->c0.c1, a->c1.c2, t4, t5);
  const F2 x5 = f2_mul_xi(t5);
  const F2 z0 = f_add(f2_dbl(f_sub(t0, a->c0.c0)), t0);    // 3 t0 - 2 a
  const F2 z1 = f_add(f2_dbl(f_add(t1, a->c1.c1)), t1);    // 3 t1 + 2 a
  const F2 z2 = f_add(f2_dbl(f_add(x5, a->c1.c0)), x5);
  const F2 z3 = f_add(f2_dbl(f_sub(t4, a->c0.c2)), t4);
  const F2 z4 = f_add(f2_dbl(f_sub(t2, a->c0.c1)), t2);
  const F2 z5 = f_add(f2_dbl(f_add(t3, a->c1.c2)), t3);
  r->c0.c0 = z0; r->c0.c1 = z4; r->c0.c2 = z3;
  r->c1.c0 = z2; r->c1.c1 = z1; r->c1.c2 = z5;
}
// a^x for cyclotomic a (x negative: the conjugate of a^|x|)
static __device__ __noinline__ void f12_cyc_pow_x(F12* r, const F12* a) {
  F12 acc = *a;   // bit 63 of |x|
#pragma unroll 1
  for (int i = 62; i >= 0; i--) {
    f12_cyc_sqr(&acc, &acc);
    if ((BLS_X_ABS32[i >> 5] >> (i & 31)) & 1) f12_mul(&acc, &acc, a);
  }
  f12_conj(r, &acc);
}
// f^(3 (p^12 - 1) / r)
static __device__ __noinline__ void f12_final_exp(F12* f) {
  F12 m, u, y0, y1;
  f12_inv(&m, f);
  f12_conj(&u, f);
  f12_mul(&m, &u, &m);          // f^(p^6 - 1)
  f12_frob2(&u, &m);
  f12_mul(&m, &u, &m);          // ^(p^2 + 1): cyclotomic from here, 1 / a = conj(a)
  f12_cyc_pow_x(&y0, &m);
  f12_conj(&u, &m);
  f12_mul(&y0, &y0, &u);        // m^(x - 1)
  f12_cyc_pow_x(&y1, &y0);
  f12_conj(&u, &y0);
  f12_mul(&y1, &y1, &u);        // ^(x - 1)
  f12_cyc_pow_x(&y0, &y1);
  f12_frob1(&u, &y1);
  f12_mul(&y1, &y0, &u);        // ^(x + p)
  f12_cyc_pow_x(&y0, &y1);
  f12_cyc_pow_x(&y0, &y0);
  f12_frob2(&u, &y1);
  f12_mul(&y0, &y0, &u);
  f12_conj(&u, &y1);
  f12_mul(&y0, &y0, &u);        // ^(x^2 + p^2 - 1)
  f12_cyc_sqr(&u, &m);
  f12_mul(&u, &u, &m);
  f12_mul(f, &y0, &u);          // m^3
}

// ---- ABI points --------------------------------------------------------------
ZK_DI Fq pr_read_fq(const uint64_t* w) {
  Fq c;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    c.v[2 * i] = (uint32_t)w[i];
    c.v[2 * i + 1] = (uint32_t)(w[i] >> 32);
  }
  return c;
}
ZK_DI void pr_write_fq(uint64_t* w, const Fq& c) {
#pragma unroll
  for (int i = 0; i < 6; i++) w[i] = (uint64_t)c.v[2 * i] | ((uint64_t)c.v[2 * i + 1] << 32);
}
// What verify.hip's load() checks: a set infinity byte is the identity
// whatever the coordinates hold; else coordinates below p and the point on
// its curve.  Montgomery coordinates out.
static __device__ __noinline__ bool pr_load_g1(const uint64_t* w, Affine<FqC>* P, bool* inf) {
  *inf = (w[12] & 0xff) != 0;
  f_set_zero(P->x);
  f_set_zero(P->y);
  if (*inf) return true;
  const Fq x = pr_read_fq(w), y = pr_read_fq(w + 6);
  if (pt_fq_geq_p(x) || pt_fq_geq_p(y)) return false;
  P->x = {pt_to_mont(x)};
  P->y = {pt_to_mont(y)};
  return f_eq(f_sqr(P->y), pt_curve_rhs(P->x));
}
static __device__ __noinline__ bool pr_load_g2(const uint64_t* w, Affine<F2>* P, bool* inf) {
  *inf = (w[24] & 0xff) != 0;
  f_set_zero(P->x);
  f_set_zero(P->y);
  if (*inf) return true;
  Fq c[4];
  bool in_range = true;
#pragma unroll 1
  for (int k = 0; k < 4; k++) {
    c[k] = pr_read_fq(w + 6 * k);
    in_range = in_range && !pt_fq_geq_p(c[k]);
  }
  if (!in_range) return false;
#pragma unroll 1
  for (int k = 0; k < 4; k++) c[k] = pt_to_mont(c[k]);
  P->x = {{c[0], c[1]}};
  P->y = {{c[2], c[3]}};
  return f_eq(f_sqr(P->y), pt_curve_rhs(P->x));
}

// ---- Miller loop -----------------------------------------------------------------
// Doubling step on T (XYZZ: x = X / ZZ, y = Y / ZZZ) with the tangent at T
// evaluated at P = (xp, yp).  With dbl-2008-s-1's U = 2Y, V = U^2, W = U V,
// S = X V, M = 3 X^2 the slope is M ZZ / (U ZZZ), and the host line times
// 2 U ZZZ is
//   l[0] = 2 M X - V,  l[1] = -2 M ZZ xp,  l[2] = 2 U ZZZ yp.
static __device__ __noinline__ void pr_dbl_step(XYZZ<F2>* T, const Fq* xp, const Fq* yp, F2* l) {
  const F2 U = f2_dbl(T->Y);
  const F2 V = f_sqr(U);
  const F2 W = f_mul(U, V);
  const F2 S = f_mul(T->X, V);
  const F2 X2 = f_sqr(T->X);
  const F2 M = f_add(f2_dbl(X2), X2);
  l[0] = f_sub(f2_dbl(f_mul(M, T->X)), V);
  l[1] = f_neg(f2_mul_fq(f2_dbl(f_mul(M, T->ZZ)), *xp));
  l[2] = f2_mul_fq(f2_dbl(f_mul(U, T->ZZZ)), *yp);
  const F2 X3 = f_sub(f_sqr(M), f2_dbl(S));
  const F2 Y3 = f_sub(f_mul(M, f_sub(S, X3)), f_mul(W, T->Y));
  T->ZZ = f_mul(V, T->ZZ);
  T->ZZZ = f_mul(W, T->ZZZ);
  T->X = X3;
  T->Y = Y3;
}
// Addition step T + Q (Q affine) with the chord through T and Q evaluated at
// P.  With madd-2008-s's U2 = xq ZZ, S2 = yq ZZZ, P' = U2 - X, R = S2 - Y the
// slope is R ZZ / (P' ZZZ), and the host line (taken at Q) times P' ZZZ is
//   l[0] = R U2 - P' S2,  l[1] = -R ZZ xp,  l[2] = P' ZZZ yp.
static __device__ __noinline__ void pr_add_step(XYZZ<F2>* T, const Affine<F2>* Q, const Fq* xp, const Fq* yp, F2* l) {
  const F2 U2 = f_mul(Q->x, T->ZZ), S2 = f_mul(Q->y, T->ZZZ);
  const F2 Pd = f_sub(U2, T->X), R = f_sub(S2, T->Y);
  l[0] = f_sub(f_mul(R, U2), f_mul(Pd, S2));
  l[1] = f_neg(f2_mul_fq(f_mul(R, T->ZZ), *xp));
  l[2] = f2_mul_fq(f_mul(Pd, T->ZZZ), *yp);
  *T = xyzz_madd(*T, *Q);
}

// The pairs of one shared-squaring Miller loop: pair 0 has a variable G2
// point (lines on the fly), pairs 1 and 2 fixed G2 points whose PR_STEPS
// lines come from a per-call table (pairing.hip): per step the affine slope
// lambda' and lambda' x' - y', 48 words, read wave-uniformly.  A pair that is
// off (an infinite point on either side) contributes 1.
struct PrPairs {
  bool on[3];
  Fq xp[3], yp[3];          // the G1 points
  Affine<F2> Q;             // pair 0
  const uint32_t* tab[2];   // pairs 1, 2
};
ZK_DI void pr_fixed_line(F12* f, const PrPairs* in, int j, int step) {
  const uint32_t* t = in->tab[j - 1] + 48 * step;
  F2 l[3];
  l[0] = f2_load(t + 24);
  l[1] = f_neg(f2_mul_fq(f2_load(t), in->xp[j]));
  l[2] = {{in->yp[j], fp_zero<FqParams>()}};
  f12_mul_line(f, l);
}
// f = prod_j f_{|x|, Q_j}(P_j), NOT yet conjugated for the negative x
static __device__ __noinline__ void pr_miller(F12* f, const PrPairs* in) {
  f12_set_one(f);
  XYZZ<F2> T = xyzz_from_aff(in->Q);
  F2 l[3];
  int step = 0;
#pragma unroll 1
  for (int i = 62; i >= 0; i--) {
    f12_sqr(f, f);
    if (in->on[0]) {
      pr_dbl_step(&T, &in->xp[0], &in->yp[0], l);
      f12_mul_line(f, l);
    }
#pragma unroll 1
    for (int j = 1; j < 3; j++)
      if (in->on[j]) pr_fixed_line(f, in, j, step);
    step++;
    if ((BLS_X_ABS32[i >> 5] >> (i & 31)) & 1) {
      if (in->on[0]) {
        pr_add_step(&T, &in->Q, &in->xp[0], &in->yp[0], l);
        f12_mul_line(f, l);
      }
#pragma unroll 1
      for (int j = 1; j < 3; j++)
        if (in->on[j]) pr_fixed_line(f, in, j, step);
      step++;
    }
  }
}

// ---- what the kernels of pairing.hip and verify_all.hip share ----------------------
namespace zk {

constexpr int PR_BLOCK = 64;
constexpr size_t PROOF_WORDS = sizeof(zk_proof) / 8, G1W = sizeof(zk_g1_affine) / 8, G2W = sizeof(zk_g2_affine) / 8;
static_assert(PROOF_WORDS == 51 && G1W == 13 && G2W == 25, "ABI point sizes");
ZK_DI void pr_use_g1(PrPairs& in, int j, const Affine<FqC>& P, bool on) {
  in.on[j] = on;
  in.xp[j] = P.x.v;
  in.yp[j] = P.y.v;
}

// k P for a 64-bit k: double-and-add from the top bit, mixed additions
static __device__ __noinline__ XYZZ<FqC> pr_g1_mul64(const Affine<FqC>* P, uint64_t k) {
  XYZZ<FqC> t;
  xyzz_set_inf(t);
#pragma unroll 1
  for (int b = 63; b >= 0; b--) {
    t = xyzz_dbl(t);
    if ((k >> b) & 1) t = xyzz_madd(t, *P);
  }
  return t;
}
// k P for a whole scalar k < r (sound mode): k = 4 u64 limbs in device memory,
// 255 bits from the top, the same rolled double-and-add
static __device__ __noinline__ XYZZ<FqC> pr_g1_mul255(const Affine<FqC>* P, const uint64_t* k) {
  XYZZ<FqC> t;
  xyzz_set_inf(t);
#pragma unroll 1
  for (int b = 254; b >= 0; b--) {
    t = xyzz_dbl(t);
    if ((k[b >> 6] >> (b & 63)) & 1) t = xyzz_madd(t, *P);
  }
  return t;
}
// a 4-limb public input is a reduced Fr (< r)
static __device__ __forceinline__ bool pr_fr_reduced(const uint64_t* k) {
#pragma unroll
  for (int i = 3; i >= 0; i--)
    if (k[i] != FR_MOD64[i]) return k[i] < FR_MOD64[i];
  return false;
}
// x = X / ZZ, y = Y / ZZZ with one inversion: 1 / ZZ = (ZZ / ZZZ)^2
ZK_DI Affine<FqC> pr_g1_affine(const XYZZ<FqC>& p) {
  const FqC i3 = {pr_fq_inv(p.ZZZ.v)};
  const FqC i2 = f_sqr(f_mul(p.ZZ, i3));
  return {f_mul(p.X, i2), f_mul(p.Y, i3)};
}

// ---- the per-key words the verify kernels read (pairing.hip, prepared.hip) ------------
// 32-bit words, device Montgomery:
//   [VK_AB, +144)                   the Miller value of (-alpha, beta), tower order
//   [VK_TAB, +2 x 48 PR_STEPS)      the lines of gamma, then of delta
//   [VK_ON, +4)                     gamma finite, delta finite
//   [VK_IC, +24 (n_inputs + 1))     ic_g1: x, y; an identity entry is (0, 0)
constexpr size_t VK_AB = 0, VK_TAB = 144, VK_ON = VK_TAB + 2 * 48 * PR_STEPS, VK_IC = VK_ON + 4;
// Those words for a key, made on the host (pairing.hip).  Every point of the
// key is validated -- canonical and on its curve -- alpha, beta, gamma, delta
// and all ic_len entries: false for a malformed one.
bool pairing_tables(const zk_vk& vk, size_t n_inputs, std::vector<uint32_t>& out);

}  // namespace zk
