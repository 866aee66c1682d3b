// ceremony.hpp -- n G1 points times ONE scalar, one lane per point: the hot
// path of a phase-2 key contribution (ceremony.hip), which rescales every
// ic_g1 and h_g1 entry of a sound proving key by the same 1 / d.
//
// Two walks over XYZZ with the formulas of curve.hpp, both rolled and built
// on the out-of-line products of points.hpp; the scalar is the same in every
// lane, so neither diverges:
//   plain  the 255-bit double-and-add of pairing.hpp's pr_g1_mul255 from the
//          top set bit: one doubling per bit, one mixed addition per set bit
//   endo   k = e2 x^2 + e1 with x = BLS_X_ABS, e1, e2 < 2^128 (r = x^4 - x^2 + 1),
//          and phi(x, y) = (beta x, y) = -[x^2] P (ENDO_BETA32, the identity the
//          proof decoder's subgroup test rests on), so k P = e1 P + e2 Q with
//          Q = -phi(P) = (beta x, -y): both halves walked jointly, 128
//          doublings, one addition per non-zero bit pair from {P, Q, P + Q}.
//          P and Q are affine (mixed additions); P + Q stays an XYZZ value
//          added by the full formula (DESIGN.md 2.15 says why).
// The library ships the endo walk (ceremony.hip); the plain one is the test
// library's cross-check and timing baseline (testhooks.hip).  Both leave XYZZ
// values that g1_mul_finish normalises (batch_normalize, msm.hip) and writes
// as canonical ABI words.
#pragma once
#include <algorithm>

#include "ctx.hpp"
#include "points.hpp"

namespace zk {

constexpr int CM_BLOCK = 128;

// What a walk reads of the scalar, as kernel arguments (wave-uniform).
// plain: w = the four limbs of k.  endo: w[0..1] = e1, w[2..3] = e2.
// top: bits to walk -- the bit length of k, or of e1 | e2.
struct CmScalar {
  uint64_t w[4];
  int top;
};

ZK_DI Fq cm_read_fq(const uint64_t* w) {
  Fq c;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    c.v[2 * i] = (uint32_t)w[i];
    c.v[2 * i + 1] = (uint32_t)(w[i] >> 32);
  }
  return c;
}
// ABI point -> Montgomery affine; false for a set infinity byte.  Unchecked:
// the callers' points are canonical, on the curve and in the subgroup.
ZK_DI bool cm_load(const uint64_t* w, Affine<FqC>& P) {
  if (w[12] & 0xff) return false;
  P.x = {pt_to_mont(cm_read_fq(w))};
  P.y = {pt_to_mont(cm_read_fq(w + 6))};
  return true;
}
ZK_DI void cm_store(G1X* out, const XYZZ<FqC>& p) {
  G1X q;
  q.X = p.X.v; q.Y = p.Y.v; q.ZZ = p.ZZ.v; q.ZZZ = p.ZZZ.v;
  st_vec(out, q);
}
ZK_DI XYZZ<FqC> cm_fetch(const G1X* in) {
  const G1X q = ld_vec(in);
  return {{q.X}, {q.Y}, {q.ZZ}, {q.ZZZ}};
}

// k P, k = s.w below 2^s.top.  madd's own branches cover the accumulator at O
// (the first set bit) and at +-P.
ZK_DI XYZZ<FqC> cm_walk_plain(const Affine<FqC>& P, const CmScalar& s) {
  XYZZ<FqC> acc;
  xyzz_set_inf(acc);
#pragma unroll 1
  for (int b = s.top - 1; b >= 0; b--) {
    acc = xyzz_dbl(acc);
    const int j = b >> 6;
    const uint64_t w = j == 0 ? s.w[0] : j == 1 ? s.w[1] : j == 2 ? s.w[2] : s.w[3];
    if ((w >> (b & 63)) & 1) acc = xyzz_madd(acc, P);
  }
  return acc;
}

// e1 P + e2 Q, Q = -phi(P) = [x^2] P.  P is in the prime-order subgroup and
// not the identity, so Q and P + Q are not the identity either; the
// accumulator meets O or +- a table entry only near the ends of the walk
// (k = x^2 - 1, x^2, x^2 + 1, r - 1 ...), which madd's and add's branches cover.
ZK_DI FqC cm_fetch_fq(const Fq* p) { return {ld_vec(p)}; }
// p + *q by add-2008-s (curve.hpp's xyzz_add), with q's coordinates fetched one
// at a time where the formula uses them (ZZ and ZZZ twice): at most one of
// them is live beside p and the formula's own values, which is what keeps the
// walk below at two waves per SIMD.
ZK_DI XYZZ<FqC> cm_add_slot(const XYZZ<FqC>& p, const G1X* q) {
  if (f_is_zero(cm_fetch_fq(&q->ZZ))) return p;
  if (xyzz_is_inf(p)) return cm_fetch(q);
  const FqC U1 = f_mul(p.X, cm_fetch_fq(&q->ZZ));
  ZK_SB();
  const FqC P = f_sub(f_mul(cm_fetch_fq(&q->X), p.ZZ), U1);
  ZK_SB();
  const FqC S1 = f_mul(p.Y, cm_fetch_fq(&q->ZZZ));
  ZK_SB();
  const FqC R = f_sub(f_mul(cm_fetch_fq(&q->Y), p.ZZZ), S1);
  ZK_SB();
  if (f_is_zero(P)) {
    if (f_is_zero(R)) return xyzz_dbl(p);
    XYZZ<FqC> r; xyzz_set_inf(r); return r;
  }
  XYZZ<FqC> r;
  const FqC PP = f_sqr(P);
  ZK_SB();
  r.ZZ = f_mul(p.ZZ, cm_fetch_fq(&q->ZZ));
  ZK_SB();
  r.ZZ = f_mul(r.ZZ, PP);
  ZK_SB();
  const FqC PPP = f_mul(P, PP);
  ZK_SB();
  r.ZZZ = f_mul(p.ZZZ, cm_fetch_fq(&q->ZZZ));
  ZK_SB();
  r.ZZZ = f_mul(r.ZZZ, PPP);
  ZK_SB();
  const FqC Q = f_mul(U1, PP);
  ZK_SB();
  r.X = f_sub(f_sub(f_sqr(R), PPP), f_add(Q, Q));
  ZK_SB();
  r.Y = f_mul_sub(R, f_sub(Q, r.X), S1, PPP);
  ZK_SB();
  return r;
}

// P + Q waits in the lane's result slot `slot` between the steps that add it
// (a quarter of them), not in 48 registers: the slot is written once, read
// back through the cache and overwritten by the result after the walk.
ZK_DI XYZZ<FqC> cm_walk_endo(const Affine<FqC>& P, const CmScalar& s, G1X* slot) {
  const FqC qx = f_mul(P.x, FqC{fp_from_const<FqParams>(ENDO_BETA32)});
  cm_store(slot, xyzz_madd(xyzz_from_aff(P), Affine<FqC>{qx, f_neg(P.y)}));
  XYZZ<FqC> acc;
  xyzz_set_inf(acc);
#pragma unroll 1
  for (int b = s.top - 1; b >= 0; b--) {
    acc = xyzz_dbl(acc);
    const uint64_t w1 = (b & 64) ? s.w[1] : s.w[0], w2 = (b & 64) ? s.w[3] : s.w[2];
    const uint32_t d = (uint32_t)((w1 >> (b & 63)) & 1) | ((uint32_t)((w2 >> (b & 63)) & 1) << 1);
    if (d == 3) {
      acc = cm_add_slot(acc, slot);
    } else if (d) {   // one madd body for P and Q: the choice is wave-uniform
      Affine<FqC> B = P;
      if (d == 2) B = {qx, f_neg(P.y)};
      acc = xyzz_madd(acc, B);
    }
  }
  return acc;
}

template <bool ENDO>
ZK_DI void cm_mul_point(const uint64_t* __restrict__ in, size_t n, const CmScalar& s, G1X* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * CM_BLOCK + threadIdx.x;
  if (i >= n) return;
  Affine<FqC> P;
  XYZZ<FqC> acc;
  if (!cm_load(in + 13 * i, P)) xyzz_set_inf(acc);
  else acc = ENDO ? cm_walk_endo(P, s, &out[i]) : cm_walk_plain(P, s);
  cm_store(&out[i], acc);
}

// (e2, e1) = divmod(k, x^2) into s.w[2..3], s.w[0..1], and the bits to walk.
// false when k >= r.
bool cm_split_scalar(const zk_fr& k, CmScalar& s);
// the plain walk's view of k; false when k >= r
bool cm_plain_scalar(const zk_fr& k, CmScalar& s);

// m XYZZ values on the device -> m canonical zk_g1_affine in d_out (the
// identity: zero coordinates, infinity byte 1), through d_pre (m Fq) and
// d_aff (m G1A), on st
void g1_mul_finish(const G1X* d_x, size_t m, Fq* d_pre, G1A* d_aff, uint64_t* d_out, hipStream_t st);

// One call of n points through a walk: the array crosses the GPU in chunks of
// ctx->point_chunk points on the main stream, as points_run's does, with
// buffers that belong to the call.  launch(grid, st, d_in, m, d_x) starts the
// walk's kernel over m ABI points -> m XYZZ values.  out == pts is allowed: a
// chunk's results are written after its points were read.
template <class Launch>
int g1_mul_scalar_run(zk_ctx* ctx, const zk_g1_affine* pts, size_t n, zk_g1_affine* out, const char* phase,
                      Launch&& launch) {
  if (!n) return ZK_OK;
  hipStream_t st = ctx->stream;
  const size_t chunk = std::min<size_t>(ctx->point_chunk, n);
  DevBuf d_io, d_x, d_pre, d_aff;
  d_io.ensure(sizeof(zk_g1_affine) * chunk);
  d_x.ensure(sizeof(G1X) * chunk);
  d_pre.ensure(sizeof(Fq) * chunk);
  d_aff.ensure(sizeof(G1A) * chunk);
  for (size_t lo = 0; lo < n; lo += chunk) {
    const size_t m = std::min(chunk, n - lo);
    ZK_HIP(hipMemcpyAsync(d_io.p, pts + lo, sizeof(zk_g1_affine) * m, hipMemcpyHostToDevice, st));
    int pi = ctx->prof.begin(st, phase, m);
    launch(dim3(ceil_div(m, CM_BLOCK)), st, d_io.as<uint64_t>(), m, d_x.as<G1X>());
    ZK_LAUNCH_CHECK();
    ctx->prof.end(st, pi);
    pi = ctx->prof.begin(st, "g1_mul_finish", m);
    g1_mul_finish(d_x.as<G1X>(), m, d_pre.as<Fq>(), d_aff.as<G1A>(), d_io.as<uint64_t>(), st);
    ctx->prof.end(st, pi);
    ZK_HIP(hipMemcpyAsync(out + lo, d_io.p, sizeof(zk_g1_affine) * m, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));   // the next chunk reuses the buffers
  }
  if (ctx->prof.on) ctx->prof.collect();
  return ZK_OK;
}

}  // namespace zk
