// hash.hpp -- the hash to G2 of the ceremony's proofs of knowledge
// (ZKAMD-H2G2-V1: include/zkp.h), one lane per message, on
// points.hpp's out-of-line products.  hash.hip holds the kernel, the host twin
// and the C ABI; the try-cap hook of testhooks.hip runs the same kernel.
//
//   m0 = SHA-256("ZKAMD-H2G2-V1" | byte(len(dst)) | dst | msg)
//   try ctr = 0, 1, ..: d_j = SHA-256(m0 | byte(ctr) | byte(j)), j = 0..4;
//     x = (d_0 | d_1 mod p) + (d_2 | d_3 mod p) u;  t = x^3 + 4 (1 + u)
//     t == 0 or not a square: next ctr;  y = the root whose sort flag is d_4[31] & 1
//     Q = [x^2 - x - 1] P + [x - 1] psi(P) + psi^2([2] P),  P = (x, y);  Q == O: next ctr
//
// Shape of a lane's work.  The try loop is the only part whose length depends
// on the lane, so it holds as little as it can: five compressions, three
// products per coordinate to enter Fq, the curve's right side and ONE Fq power
// -- t is a square in Fq2 exactly when its norm c0^2 + c1^2 is a square in Fq
// (Euler's criterion; a zero norm is t == 0), about 570 products a try.  The
// square root (two Fq2 powers), the cofactor clearing (two [|x|] passes) and
// the inversion to affine form come after the loop, once per lane.
//
// The loop is scalar control flow: one counter for the wave, left when a
// ballot says every lane has its x (or at the cap).  A lane that is done keeps
// computing and discards the result; the wave would wait for its slowest lane
// anyway, and a loop whose trip count is a per-lane value is the shape that
// went wrong in DESIGN.md 2.17.
#pragma once
#include "points.hpp"
#include "sha256.hpp"

namespace zk {

constexpr uint32_t H2_MAX_TRIES = 256;
constexpr uint8_t H2_NO_POINT = 0xff;      // the tries byte of a message without a point
constexpr size_t H2_TAG_LEN = 13, H2_PREFIX = H2_TAG_LEN + 1;
static constexpr uint8_t H2_TAG[H2_TAG_LEN + 1] = "ZKAMD-H2G2-V1";

// byte pos of tag | byte(dst_len) | dst | msg
struct H2Source {
  const uint8_t* dst;
  size_t dst_len;
  const uint8_t* msg;
  ZK_SHA_HD uint8_t operator()(size_t pos) const {
    if (pos < H2_TAG_LEN) return H2_TAG[pos];
    if (pos == H2_TAG_LEN) return (uint8_t)dst_len;
    pos -= H2_PREFIX;
    return pos < dst_len ? dst[pos] : msg[pos - dst_len];
  }
};
// d_j = SHA-256(m0 | byte(ctr) | byte(j)): 34 bytes, one block
ZK_SHA_HD void h2_digest(const uint32_t m0[8], uint32_t ctr, uint32_t j, uint32_t d[8]) {
  sha256_init(d);
  sha256_compress(d, {m0[0], m0[1], m0[2], m0[3], m0[4], m0[5], m0[6], m0[7], (ctr << 24) | (j << 16) | 0x8000u, 0, 0,
                      0, 0, 0, 0, 34 * 8});
}

#if defined(__HIPCC__)
// m0 travels by value (eight VGPRs), so it never needs an address
struct H2Seed {
  uint32_t w[8];
};
// a digest as a 256-bit big-endian integer -> canonical words (below 2^256 < p)
ZK_DI Fq h2_fq_of_digest(const uint32_t d[8]) {
  Fq c = fp_zero<FqParams>();
#pragma unroll
  for (int i = 0; i < 8; i++) c.v[i] = d[7 - i];
  return c;
}
// int_be(d_a | d_b) mod p in Montgomery form: hi 2^256 + lo
static __device__ __noinline__ Fq h2_fq_of_pair(H2Seed m0, uint32_t ctr, uint32_t ja) {
  uint32_t d[8];
  h2_digest(m0.w, ctr, ja, d);
  const Fq hi = pt_to_mont(h2_fq_of_digest(d));
  h2_digest(m0.w, ctr, ja + 1, d);
  const Fq lo = pt_to_mont(h2_fq_of_digest(d));
  return fp_add(pt_fq_mul(hi, fp_from_const<FqParams>(FQ_TWO256_32)), lo);
}

// psi on XYZZ coordinates: x = X / ZZ and y = Y / ZZZ, conjugation is a field
// automorphism, so (conj(X) PSI_X, conj(Y) PSI_Y, conj(ZZ), conj(ZZZ))
ZK_DI Fq2C h2_conj(const Fq2C& a) { return {{a.v.c0, fp_neg(a.v.c1)}}; }
static __device__ __noinline__ void h2_psi(XYZZ<Fq2C>* p) {
  const Fq2C kx = {{fp_from_const<FqParams>(ENDO_PSI_X32[0]), fp_from_const<FqParams>(ENDO_PSI_X32[1])}};
  const Fq2C ky = {{fp_from_const<FqParams>(ENDO_PSI_Y32[0]), fp_from_const<FqParams>(ENDO_PSI_Y32[1])}};
  p->X = f_mul(h2_conj(p->X), kx);
  p->Y = f_mul(h2_conj(p->Y), ky);
  p->ZZ = h2_conj(p->ZZ);
  p->ZZZ = h2_conj(p->ZZZ);
}
// r = a + b, out of line: one body for the four additions of the clearing
static __device__ __noinline__ void h2_add(XYZZ<Fq2C>* r, const XYZZ<Fq2C>* a, const XYZZ<Fq2C>* b) {
  *r = xyzz_add(*a, *b);
}
// Budroni-Pintore: [h_eff] P = [x^2 - x - 1] P + [x - 1] psi(P) + psi^2([2] P), x = -|x|, so
//   [x^2 - x - 1] P = [|x|]([|x|] P) + [|x|] P - P
//   [x - 1] psi(P)  = -psi([|x|] P + P)        (psi commutes with [k])
// P: on the twist, not the identity
static __device__ __noinline__ void h2_clear_cofactor(const Affine<Fq2C>* P, XYZZ<Fq2C>* out) {
  XYZZ<Fq2C> t1 = pt_mul_x_abs<Fq2C>(P);          // [|x|] P
  XYZZ<Fq2C> acc = pt_mul_x_abs<Fq2C>(&t1);       // [x^2] P
  h2_add(&acc, &acc, &t1);
  const Affine<Fq2C> nP = aff_neg(*P);
  acc = xyzz_madd(acc, nP);                       // [x^2 - x - 1] P
  t1 = xyzz_madd(t1, *P);
  h2_psi(&t1);
  t1.Y = f_neg(t1.Y);                             // [x - 1] psi(P)
  h2_add(&acc, &acc, &t1);
  t1 = aff_dbl(*P);
  h2_psi(&t1);
  h2_psi(&t1);                                    // psi^2([2] P)
  h2_add(out, &acc, &t1);
}
// 1 / a in Fq2 through the norm (one Fermat inversion in Fq); a != 0
ZK_DI Fq2C h2_fq2_inv(const Fq2C& a) {
  const Fq n = pt_pow(FqC{fp_add(pt_fq_sqr(a.v.c0), pt_fq_sqr(a.v.c1))}, FQ_INV_EXP32).v;
  return {{pt_fq_mul(a.v.c0, n), fp_neg(pt_fq_mul(a.v.c1, n))}};
}
ZK_DI void h2_write_fq(uint64_t* w, const Fq& c) {
#pragma unroll
  for (int i = 0; i < 6; i++) w[i] = (uint64_t)c.v[2 * i] | ((uint64_t)c.v[2 * i + 1] << 32);
}

// One lane's hash.  Every lane of a wave must call this together (the loop's
// exit is a ballot); a lane past the end of the batch is given the last
// message and store = false.  out: 25 words (zk_g2_affine), tries: one byte.
ZK_DI void h2_hash_lane(const uint8_t* msg, size_t msg_len, const uint8_t* dst, uint32_t dst_len, uint32_t max_tries,
                        bool store, uint64_t* out, uint8_t* tries) {
  H2Seed m0;
  sha256_of(H2Source{dst, dst_len, msg}, H2_PREFIX + dst_len + msg_len, m0.w);
  Affine<Fq2C> P;
  XYZZ<Fq2C> Q;
  f_set_zero(P.x);
  xyzz_set_inf(Q);
  uint32_t start = 0, found_at = H2_NO_POINT;
  bool done = false;
  // A second pass happens only when a cleared point is the identity (P in the
  // cofactor's torsion: probability about 2^-255); it starts the wave's
  // counter again and the lane takes no x below `start`.
#pragma unroll 1
  for (;;) {
    bool have = false;
    uint32_t sign = 0;
#pragma unroll 1
    for (uint32_t ctr = 0; ctr < max_tries; ctr++) {
      if (__ballot(!(done || have)) == 0) break;
      const Fq2C x = {{h2_fq_of_pair(m0, ctr, 0), h2_fq_of_pair(m0, ctr, 2)}};
      const Fq2C t = pt_curve_rhs(x);
      const Fq norm = fp_add(pt_fq_sqr(t.v.c0), pt_fq_sqr(t.v.c1));
      const bool square = fp_eq(pt_pow(FqC{norm}, FQ_PM1_DIV2_32).v, fp_one<FqParams>());
      uint32_t d4[8];
      h2_digest(m0.w, ctr, 4, d4);
      if (square && !done && !have && ctr >= start) {
        have = true;
        P.x = x;
        sign = d4[7] & 1;
        found_at = ctr;
      }
    }
    // Every lane from here, whether it has an x or not: a lane without one
    // works on whatever P.x holds and its result is dropped.
    Fq2C y;
    pt_fq2_sqrt(pt_curve_rhs(P.x).v, y.v);
    const Fq2 yc = {pt_from_mont(y.v.c0), pt_from_mont(y.v.c1)};
    P.y = (pt_fq2_largest(yc) ? 1u : 0u) == sign ? y : f_neg(y);
    XYZZ<Fq2C> Qn;
    h2_clear_cofactor(&P, &Qn);
    if (!done) {
      if (!have) {
        done = true;                                // no point within the cap: found_at says so
      } else if (!xyzz_is_inf(Qn)) {
        Q = Qn;
        done = true;
      } else {
        start = found_at + 1;
        found_at = H2_NO_POINT;
      }
    }
    if (__ballot(!done) == 0) break;
  }
  const bool ok = found_at != H2_NO_POINT;
  Fq c[4];
#pragma unroll
  for (int k = 0; k < 4; k++) c[k] = fp_zero<FqParams>();
  if (ok) {
    const Fq2C i3 = h2_fq2_inv(Q.ZZZ);
    const Fq2C i2 = f_sqr(f_mul(Q.ZZ, i3));
    const Fq2C ax = f_mul(Q.X, i2), ay = f_mul(Q.Y, i3);
    c[0] = pt_from_mont(ax.v.c0); c[1] = pt_from_mont(ax.v.c1);
    c[2] = pt_from_mont(ay.v.c0); c[3] = pt_from_mont(ay.v.c1);
  }
  if (store) {
#pragma unroll
    for (int k = 0; k < 4; k++) h2_write_fq(out + 6 * k, c[k]);
    out[24] = 0;
    *tries = (uint8_t)found_at;
  }
}
#endif  // __HIPCC__

}  // namespace zk

// ---- host side (hash.hip) ----------------------------------------------------
struct zk_ctx;
namespace zk {
// zk_hash_to_g2 with a try cap (the public call: H2_MAX_TRIES); the test hook
// zk_test_hash_to_g2_capped runs the same kernel with a smaller one.
int hash_to_g2_run(zk_ctx* ctx, const uint8_t* msgs, size_t n, size_t msg_len, const uint8_t* dst, size_t dst_len,
                   uint32_t max_tries, zk_g2_affine* out, uint8_t* tries);
}  // namespace zk
