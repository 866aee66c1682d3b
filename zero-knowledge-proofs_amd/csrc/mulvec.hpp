// mulvec.hpp -- n points times n DIFFERENT scalars, one lane per point, for
// both groups: the hot path of a phase-1 contribution to a powers-of-tau
// string (zk_srs_contribute, srs.hip), which multiplies entry i of every
// array by s^i times a constant.
//
// ceremony.hpp's walks share one scalar among the lanes of a wave, so none of
// their branches diverges.  Here every lane has digits of its own: a branch
// on a digit is taken by some lane at nearly every step and the wave runs
// every side.  So the digit selects an ADDRESS instead: each lane keeps a
// small table of base combinations in global memory and adds the entry its
// digit names through srs.hpp's gn_add_mem (the entry fetched a coordinate at
// a time) -- one doubling and one add body per step for the whole wave, the
// lanes whose digit is 0 masked.  The trip count is fixed (128 / 64), so the
// loop length does not diverge either.
//
// With x = BLS_X_ABS and r = x^4 - x^2 + 1 < x^4, every k < r has four base-x
// digits k = d0 + d1 x + d2 x^2 + d3 x^3, each below x < 2^64 (mv_split).
//   G1  e1 = d0 + d1 x, e2 = d2 + d3 x, (e2, e1) = divmod(k, x^2), both below
//       2^128, and k P = e1 P + e2 Q with Q = -phi(P) = (beta x, -y)
//       (cm_walk_endo's identity).  Table {P, Q, P + Q}, entry m = the bit of
//       e1 | the bit of e2 << 1: 128 doublings, up to 128 additions.
//       3 x 192 B per lane: 576 MiB for a chunk of 2^20 points.
//   G2  psi(P) = [-x] P on G2 (points.hpp's subgroup test), so the bases
//       B_j = (-1)^j psi^j (P) = [x^j] P are affine for two constant products
//       each, and k P = sum d_j B_j.  Table of the 15 non-empty subset sums of
//       B_0 .. B_3, entry m = the bits of d_0 .. d_3: 64 doublings, up to 64
//       additions, 11 additions to build it.  15 x 384 B per lane: 5.6 GiB for
//       a chunk of 2^20 points -- size ZK_OPT_POINT_CHUNK by that.
// The subset sums of {1, x, x^2, x^3} are distinct, non-zero mod r and no two
// are negatives of each other (tests/test_srs_contribute_host.py), so for P in
// the subgroup and not the identity no table entry is the identity and
// building a table never meets the doubling case.  The accumulator meets O or
// +- an entry only near the ends of a walk; gn_add_mem's own branches cover it.
//
// The plain walks (srs.hpp's gn_walk_aff over the lane's own 255 bits, every
// lane from bit 254) are the cross-check and the timing baseline
// (zk_test_g*_mul_scalars_plain).
#pragma once
#include "srs.hpp"

namespace zk {

constexpr int MV_BLOCK = 128;
constexpr int MV_TAB_G1 = 3, MV_TAB_G2 = 15;

enum MvWalk { MV_TABLE = 0, MV_PLAIN = 1 };

// w (nw words) <- w / x, returns w mod x: binary long division, x just below
// 2^64, so the remainder's shift can carry out: the carry joins the compare
// (as cm_split_scalar).
ZK_DI uint64_t mv_divmod_x(uint64_t (&w)[4]) {
  uint64_t rem = 0;
#pragma unroll 1
  for (int b = 255; b >= 0; b--) {
    const int j = b >> 6;
    const uint64_t wj = j == 0 ? w[0] : j == 1 ? w[1] : j == 2 ? w[2] : w[3];
    const bool carry = (rem >> 63) != 0;
    rem = (rem << 1) | ((wj >> (b & 63)) & 1);
    // the bit read is replaced by the quotient's
    const bool q = carry || rem >= BLS_X_ABS;
    if (q) rem -= BLS_X_ABS;
    const uint64_t m = 1ull << (b & 63);
    const uint64_t nw = q ? (wj | m) : (wj & ~m);
    if (j == 0) w[0] = nw; else if (j == 1) w[1] = nw; else if (j == 2) w[2] = nw; else w[3] = nw;
  }
  return rem;
}
// The four base-x digits of a canonical k < r.
ZK_DI void mv_split(const uint64_t* k, uint64_t (&d)[4]) {
  uint64_t w[4] = {k[0], k[1], k[2], k[3]};
  d[0] = mv_divmod_x(w);
  d[1] = mv_divmod_x(w);
  d[2] = mv_divmod_x(w);
  d[3] = w[0];   // k < x^4
}
// lo + hi x, below x^2 < 2^128, as two words
ZK_DI void mv_join(uint64_t lo, uint64_t hi, uint64_t* e) {
  const uint64_t pl = hi * BLS_X_ABS, ph = __umul64hi(hi, BLS_X_ABS);
  e[0] = pl + lo;
  e[1] = ph + (e[0] < pl ? 1 : 0);
}

// ---- G1: {P, Q, P + Q} at tab[m n + i], m < 3 ------------------------------
ZK_DI XYZZ<FqC> mv_walk_g1(const Affine<FqC>& P, const uint64_t* k, G1X* tab, size_t n) {
  uint64_t d[4], e[4];
  mv_split(k, d);
  mv_join(d[0], d[1], e);
  mv_join(d[2], d[3], e + 2);
  {
    const Affine<FqC> Q = {f_mul(P.x, FqC{fp_from_const<FqParams>(ENDO_BETA32)}), f_neg(P.y)};
    gn_store(&tab[0], xyzz_from_aff(P));
    gn_store(&tab[n], xyzz_from_aff(Q));
    gn_store(&tab[2 * n], xyzz_madd(xyzz_from_aff(P), Q));
  }
  XYZZ<FqC> acc;
  xyzz_set_inf(acc);
#pragma unroll 1
  for (int b = 127; b >= 0; b--) {
    acc = xyzz_dbl(acc);
    const uint64_t w1 = (b & 64) ? e[1] : e[0], w2 = (b & 64) ? e[3] : e[2];
    const uint32_t m = (uint32_t)((w1 >> (b & 63)) & 1) | ((uint32_t)((w2 >> (b & 63)) & 1) << 1);
    if (m) acc = gn_add_mem(acc, &tab[(size_t)(m - 1) * n]);
  }
  return acc;
}

// ---- G2: the 15 subset sums of B_0 .. B_3 at tab[(m - 1) n + i] ------------
// -psi(B) = [x] B: (conj(x) PSI_X, -conj(y) PSI_Y)
ZK_DI Affine<Fq2C> mv_next_base(const Affine<Fq2C>& B) {
  const Fq2C cx = {{B.x.v.c0, fp_neg(B.x.v.c1)}}, cy = {{B.y.v.c0, fp_neg(B.y.v.c1)}};
  const Fq2C kx = {{fp_from_const<FqParams>(ENDO_PSI_X32[0]), fp_from_const<FqParams>(ENDO_PSI_X32[1])}};
  const Fq2C ky = {{fp_from_const<FqParams>(ENDO_PSI_Y32[0]), fp_from_const<FqParams>(ENDO_PSI_Y32[1])}};
  return {f_mul(cx, kx), f_neg(f_mul(cy, ky))};
}
ZK_DI XYZZ<Fq2C> mv_walk_g2(const Affine<Fq2C>& P, const uint64_t* k, G2X* tab, size_t n) {
  uint64_t d[4];
  mv_split(k, d);
  {
    Affine<Fq2C> B = P;
#pragma unroll 1
    for (int j = 0; j < 4; j++) {
      gn_store(&tab[(size_t)((1u << j) - 1) * n], xyzz_from_aff(B));
      if (j < 3) B = mv_next_base(B);
    }
  }
  // entry m = entry (m without its lowest bit) + entry (that bit), both made
#pragma unroll 1
  for (uint32_t m = 3; m < 16; m++) {
    const uint32_t low = m & (0u - m);
    if (low == m) continue;
    gn_store(&tab[(size_t)(m - 1) * n],
             gn_add_mem(gn_fetch<Fq2C>(&tab[(size_t)(m - low - 1) * n]), &tab[(size_t)(low - 1) * n]));
  }
  XYZZ<Fq2C> acc;
  xyzz_set_inf(acc);
#pragma unroll 1
  for (int b = 63; b >= 0; b--) {
    acc = xyzz_dbl(acc);
    const uint32_t m = (uint32_t)((d[0] >> b) & 1) | ((uint32_t)((d[1] >> b) & 1) << 1) |
                       ((uint32_t)((d[2] >> b) & 1) << 2) | ((uint32_t)((d[3] >> b) & 1) << 3);
    if (m) acc = gn_add_mem(acc, &tab[(size_t)(m - 1) * n]);
  }
  return acc;
}

// ---- host side (mulvec.hip) --------------------------------------------------
// first index with k[i] >= r, or n
size_t mv_first_not_below_r(const zk_fr* k, size_t n);
// out[i] = k[i] pts[i] for n ABI points (F = FqC: zk_g1_affine, Fq2C:
// zk_g2_affine) in host memory, through the table walk or the plain one.  The
// scalars are canonical words below r (UNCHECKED here), from host memory
// (k_host) or, when k_host is null, from the device array d_k (4 n words,
// ready on the ctx's main stream).  The arrays cross the GPU in chunks of
// ctx->point_chunk points on the main stream with buffers that belong to the
// call; out == pts is allowed.  phase: the profiler's name of the walk kernel.
template <class F>
int mv_mul_scalars(zk_ctx* ctx, const void* pts, size_t n, const zk_fr* k_host, const uint64_t* d_k, void* out,
                   MvWalk walk, const char* phase);
// what the library ships for F's group (the ship rule of DESIGN.md 2.17)
template <class F>
MvWalk mv_shipped();
// the device decomposition alone: n canonical scalars below r -> n x 4 words
// (e1, e2) and n x 4 digits, in host memory (either may be null)
int mv_split_host(zk_ctx* ctx, const zk_fr* k, size_t n, uint64_t* g1_out, uint64_t* g2_out);

// n device affine points -> canonical ABI words on the device (srs.hip)
template <class F>
void gn_points_to_abi(const Affine<typename GnField<F>::Raw>* d_in, size_t n, uint64_t* d_out, hipStream_t st);

}  // namespace zk
