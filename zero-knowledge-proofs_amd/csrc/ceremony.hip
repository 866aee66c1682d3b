// ceremony.hip -- the phase-2 step of a Groth16 ceremony for SOUND keys: a
// participant rescales delta by a secret share d (zk_groth16_contribute_sound)
// and anyone checks that the new key is the old one with only delta changed
// (zk_groth16_verify_contribution_sound).  No reference counterpart: the
// reference's `ceremony` works over its truncated scalars.
//
// With e = 1 / d mod r, by the sound-mode formulas of include/zkp.h:
//   delta_g1, delta_g2 <- d delta_g1, d delta_g2
//   ic_g1[i], h_g1[i]  <- e ic_g1[i], e h_g1[i]     (both are "... / delta")
// and nothing else moves.  The two delta points go through the host curve
// code; the arrays -- millions of G1 points times the same scalar -- through
// the kernel below (ceremony.hpp), one lane per point.
#include <cstring>
#include <vector>

#include "ceremony.hpp"
#include "host_pairing.hpp"

namespace zk {

const char* point_status_text(int st);   // points.hip

__global__ void __launch_bounds__(CM_BLOCK) k_g1_mul_endo(const uint64_t* __restrict__ in, size_t n, CmScalar s,
                                                          G1X* __restrict__ out) {
  cm_mul_point<true>(in, n, s, out);
}

// device affine (Montgomery, (0, 0) = infinity) -> canonical ABI words
__global__ void __launch_bounds__(CM_BLOCK) k_g1_mul_to_abi(const G1A* __restrict__ in, size_t n,
                                                            uint64_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * CM_BLOCK + threadIdx.x;
  if (i >= n) return;
  const G1A a = ld_vec(&in[i]);
  const bool inf = aff_is_inf(a);
  const Fq x = inf ? a.x : pt_from_mont(a.x), y = inf ? a.y : pt_from_mont(a.y);
  uint64_t* w = out + 13 * i;
#pragma unroll
  for (int k = 0; k < 6; k++) {
    w[k] = (uint64_t)x.v[2 * k] | ((uint64_t)x.v[2 * k + 1] << 32);
    w[6 + k] = (uint64_t)y.v[2 * k] | ((uint64_t)y.v[2 * k + 1] << 32);
  }
  w[12] = inf ? 1 : 0;
}

void g1_mul_finish(const G1X* d_x, size_t m, Fq* d_pre, G1A* d_aff, uint64_t* d_out, hipStream_t st) {
  if (!m) return;
  batch_normalize<G1>(d_x, m, d_pre, d_aff, st);
  k_g1_mul_to_abi<<<ceil_div(m, CM_BLOCK), CM_BLOCK, 0, st>>>(d_aff, m, d_out);
  ZK_LAUNCH_CHECK();
}

static bool fr_below_r(const zk_fr& a) {
  for (int i = 3; i >= 0; i--)
    if (a.l[i] != FR_MOD64[i]) return a.l[i] < FR_MOD64[i];
  return false;
}
static bool fr_zero(const zk_fr& a) { return (a.l[0] | a.l[1] | a.l[2] | a.l[3]) == 0; }
static int bit_length(const uint64_t* w, int nw) {
  for (int i = nw - 1; i >= 0; i--)
    if (w[i]) return 64 * i + 64 - __builtin_clzll(w[i]);
  return 0;
}

bool cm_plain_scalar(const zk_fr& k, CmScalar& s) {
  if (!fr_below_r(k)) return false;
  std::memcpy(s.w, k.l, 32);
  s.top = bit_length(s.w, 4);
  return true;
}

// Binary long division of k < r by x^2 (just below 2^128, so the running
// remainder's shift can carry out of 128 bits: the carry joins the compare).
bool cm_split_scalar(const zk_fr& k, CmScalar& s) {
  if (!fr_below_r(k)) return false;
  typedef unsigned __int128 u128;
  const u128 x2 = (u128)BLS_X_ABS * BLS_X_ABS;
  u128 rem = 0, q = 0;   // q < x^2: r = x^4 - x^2 + 1 < x^4
  for (int b = 255; b >= 0; b--) {
    const bool carry = (rem >> 127) != 0;
    rem = (rem << 1) | ((k.l[b >> 6] >> (b & 63)) & 1);
    q <<= 1;
    if (carry || rem >= x2) {
      rem -= x2;
      q |= 1;
    }
  }
  s.w[0] = (uint64_t)rem; s.w[1] = (uint64_t)(rem >> 64);
  s.w[2] = (uint64_t)q;   s.w[3] = (uint64_t)(q >> 64);
  const uint64_t m[2] = {s.w[0] | s.w[2], s.w[1] | s.w[3]};
  s.top = bit_length(m, 2);
  return true;
}

// out[i] = k pts[i] through the shipped (endomorphism) walk
static int g1_mul_scalar(zk_ctx* ctx, const zk_g1_affine* pts, size_t n, const zk_fr* k, zk_g1_affine* out) {
  CmScalar s;
  if (!cm_split_scalar(*k, s)) {
    ctx->err = "g1_mul_scalar: the scalar is not below r";
    return ZK_ERR_ARG;
  }
  return g1_mul_scalar_run(ctx, pts, n, out, "g1_mul_scalar",
                           [&](dim3 grid, hipStream_t st, const uint64_t* d_in, size_t m, G1X* d_x) {
                             k_g1_mul_endo<<<grid, CM_BLOCK, 0, st>>>(d_in, m, s, d_x);
                           });
}

// ---- host helpers of the two calls below ---------------------------------
static void fq_words(const host::Fq& m, uint64_t* w) {
  const host::Fq c = host::from_mont(m);
  std::memcpy(w, c.l, 48);
}
// the point's words without the struct padding
static bool same(const zk_g1_affine& a, const zk_g1_affine& b) {
  return !std::memcmp(a.x, b.x, 48) && !std::memcmp(a.y, b.y, 48) && a.infinity == b.infinity;
}
static bool same(const zk_g2_affine& a, const zk_g2_affine& b) {
  return !std::memcmp(a.x, b.x, 96) && !std::memcmp(a.y, b.y, 96) && a.infinity == b.infinity;
}
template <class P>
static bool same(const P* a, const P* b, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!same(a[i], b[i])) return false;
  return true;
}
// -P; false when P is not canonical or off the curve
static bool negated(const zk_g1_affine& p, zk_g1_affine& out) {
  host::A1 a;
  if (!host::load(p, a)) return false;
  out = p;
  if (!a.inf) fq_words(host::neg(a.y), out.y);
  return true;
}

}  // namespace zk

using namespace zk;

#define ZK_CGUARD(ctx, ...)                                   \
  try {                                                       \
    ZK_HIP(hipSetDevice((ctx)->device));                      \
    __VA_ARGS__                                               \
  } catch (const zk::Error& e) {                              \
    (ctx)->err = e.what();                                    \
    return e.code;                                            \
  } catch (const std::exception& e) {                         \
    (ctx)->err = e.what();                                    \
    return ZK_ERR_DEVICE;                                     \
  }

int zk_g1_mul_scalar(zk_ctx* ctx, const zk_g1_affine* pts, size_t n, const zk_fr* k, zk_g1_affine* out) {
  if (!ctx || !k || (n && (!pts || !out))) return ZK_ERR_ARG;
  ZK_CGUARD(ctx, { return g1_mul_scalar(ctx, pts, n, k, out); })
}

int zk_groth16_contribute_sound(zk_ctx* ctx, zk_pk* pk, zk_vk* vk, const zk_fr* d) {
  if (!ctx || !pk || !d) return ZK_ERR_ARG;
  if (fr_zero(*d) || !fr_below_r(*d)) {
    ctx->err = "contribute: the share must be non-zero and below r";
    return ZK_ERR_ARG;
  }
  if ((pk->ic_len && !pk->ic_g1) || (pk->h_len && !pk->h_g1)) return ZK_ERR_ARG;
  if (vk && !same(vk->delta_g2, pk->delta_g2)) {
    ctx->err = "contribute: vk.delta_g2 is not pk.delta_g2";
    return ZK_ERR_ARG;
  }
  ZK_CGUARD(ctx, {
    host::A1 d1;
    host::A2 d2;
    if (!host::load(pk->delta_g1, d1) || !host::load(pk->delta_g2, d2)) {
      ctx->err = "contribute: a delta point is not canonical or off its curve";
      return ZK_ERR_ARG;
    }
    zk_fr e;
    host::fr_from_mont(host::fr_inv(host::fr_to_mont(d->l)), e.l);
    // everything into scratch: the key changes only once nothing can fail any more
    const size_t nic = pk->ic_len, nh = pk->h_len;
    std::vector<zk_g1_affine> pts(nic + nh);
    if (nic) std::memcpy(pts.data(), pk->ic_g1, sizeof(zk_g1_affine) * nic);
    if (nh) std::memcpy(pts.data() + nic, pk->h_g1, sizeof(zk_g1_affine) * nh);
    const int rc = g1_mul_scalar(ctx, pts.data(), pts.size(), &e, pts.data());
    if (rc != ZK_OK) return rc;
    zk_g1_affine nd1;
    zk_g2_affine nd2;
    std::memset(&nd1, 0, sizeof nd1);
    std::memset(&nd2, 0, sizeof nd2);
    host_to_abi<G1>(host::mul_scalar(host::from_affine(d1.x, d1.y, d1.inf), d->l), reinterpret_cast<uint64_t*>(&nd1));
    host_to_abi<G2>(host::mul_scalar(host::from_affine(d2.x, d2.y, d2.inf), d->l), reinterpret_cast<uint64_t*>(&nd2));
    pk->delta_g1 = nd1;
    pk->delta_g2 = nd2;
    if (vk) vk->delta_g2 = nd2;
    if (nic) std::memcpy(pk->ic_g1, pts.data(), sizeof(zk_g1_affine) * nic);
    if (nh) std::memcpy(pk->h_g1, pts.data() + nic, sizeof(zk_g1_affine) * nh);
    return ZK_OK;
  })
}

// One array of `after` through zk_g1_validate; true when every point is valid.
// rc: ZK_OK, or the call's own failure (not an invalid point).
static bool valid_g1(zk_ctx* ctx, const char* name, const zk_g1_affine* pts, size_t n, int& rc) {
  std::vector<uint8_t> st(n);
  size_t bad = n;
  rc = zk_g1_validate(ctx, pts, n, st.data(), &bad);
  if (rc == ZK_OK) return true;
  if (rc != ZK_ERR_ARG || bad >= n) return false;
  rc = ZK_OK;
  ctx->err = std::string("after.") + name + "[" + std::to_string(bad) + "]: " + point_status_text(st[bad]);
  return false;
}

int zk_groth16_verify_contribution_sound(zk_ctx* ctx, const zk_pk* before, const zk_vk* vk_before, const zk_pk* after,
                                         const zk_vk* vk_after, const zk_fr* coeffs, size_t n_coeffs, int* status) {
  if (!ctx || !before || !vk_before || !after || !vk_after || !status || (n_coeffs && !coeffs)) return ZK_ERR_ARG;
  const zk_pk &B = *before, &A = *after;
  const zk_vk &VB = *vk_before, &VA = *vk_after;
  *status = ZK_CONTRIB_SHAPE;
  if (A.a_len != B.a_len || A.b_len != B.b_len || A.b2_len != B.b2_len || A.ic_len != B.ic_len ||
      A.h_len != B.h_len || A.num_public != B.num_public || VA.ic_len != VB.ic_len ||
      VA.num_public != VB.num_public || n_coeffs != B.h_len + B.ic_len)
    return ZK_OK;
  if ((B.a_len && (!A.a_g1 || !B.a_g1)) || (B.b_len && (!A.b_g1 || !B.b_g1)) || (B.b2_len && (!A.b_g2 || !B.b_g2)) ||
      (B.ic_len && (!A.ic_g1 || !B.ic_g1)) || (B.h_len && (!A.h_g1 || !B.h_g1)) ||
      (VB.ic_len && (!VA.ic_g1 || !VB.ic_g1)))
    return ZK_ERR_ARG;
  for (size_t i = 0; i < n_coeffs; i++)
    if (fr_zero(coeffs[i]) || coeffs[i].l[2] || coeffs[i].l[3]) {
      ctx->err = "verify_contribution: coefficient " + std::to_string(i) + " must be non-zero and below 2^128";
      return ZK_ERR_ARG;
    }
  ZK_CGUARD(ctx, {
    *status = ZK_CONTRIB_FIXED_PART;
    if (!same(A.alpha_g1, B.alpha_g1) || !same(A.beta_g1, B.beta_g1) || !same(A.beta_g2, B.beta_g2) ||
        !same(A.a_g1, B.a_g1, B.a_len) || !same(A.b_g1, B.b_g1, B.b_len) || !same(A.b_g2, B.b_g2, B.b2_len) ||
        !same(VA.alpha_g1, VB.alpha_g1) || !same(VA.beta_g2, VB.beta_g2) || !same(VA.gamma_g2, VB.gamma_g2) ||
        !same(VA.ic_g1, VB.ic_g1, VB.ic_len) || !same(VA.delta_g2, A.delta_g2) || !same(VB.delta_g2, B.delta_g2))
      return ZK_OK;

    *status = ZK_CONTRIB_POINT;
    int rc = ZK_OK;
    if (!valid_g1(ctx, "delta_g1", &A.delta_g1, 1, rc) || !valid_g1(ctx, "ic_g1", A.ic_g1, A.ic_len, rc) ||
        !valid_g1(ctx, "h_g1", A.h_g1, A.h_len, rc))
      return rc;
    uint8_t st2 = 0;
    rc = zk_g2_validate(ctx, &A.delta_g2, 1, &st2, nullptr);
    if (rc != ZK_OK) {
      if (rc != ZK_ERR_ARG || st2 == ZK_POINT_OK) return rc;
      ctx->err = std::string("after.delta_g2[0]: ") + point_status_text(st2);
      return ZK_OK;
    }

    *status = ZK_CONTRIB_DELTA;
    if (A.delta_g1.infinity || A.delta_g2.infinity) return ZK_OK;
    zk_g1_affine g1[2];
    zk_g2_affine g2[2];
    int one = 0;
    g1[0] = A.delta_g1;
    g2[0] = B.delta_g2;
    g2[1] = A.delta_g2;
    if (!negated(B.delta_g1, g1[1]) || zk_pairing_product_is_one(g1, g2, 2, &one) != ZK_OK) {
      ctx->err = "verify_contribution: a delta point of the old key is not canonical or off its curve";
      return ZK_ERR_ARG;
    }
    if (!one) return ZK_OK;

    *status = ZK_CONTRIB_RATIO;
    // S = sum rho_i h_g1[i] + sum rho_{h_len + j} ic_g1[j] over either key
    std::vector<zk_g1_affine> cat(n_coeffs);
    zk_g1_affine S[2];
    for (int side = 0; side < 2; side++) {
      const zk_pk& K = side ? A : B;
      if (K.h_len) std::memcpy(cat.data(), K.h_g1, sizeof(zk_g1_affine) * K.h_len);
      if (K.ic_len) std::memcpy(cat.data() + K.h_len, K.ic_g1, sizeof(zk_g1_affine) * K.ic_len);
      rc = zk_msm_g1(ctx, cat.data(), n_coeffs, coeffs, n_coeffs, 255, &S[side]);
      if (rc != ZK_OK) return rc;
    }
    g1[0] = S[1];
    g2[0] = A.delta_g2;
    g2[1] = B.delta_g2;
    if (!negated(S[0], g1[1]) || zk_pairing_product_is_one(g1, g2, 2, &one) != ZK_OK) {
      ctx->err = "verify_contribution: the old key's points are not canonical or off the curve";
      return ZK_ERR_ARG;
    }
    if (!one) return ZK_OK;
    *status = ZK_CONTRIB_OK;
    return ZK_OK;
  })
}
