// keycheck.hip -- is this sound key the key of this circuit over this
// powers-of-tau string?  (zk_groth16_verify_key_srs_sound, include/zkp.h;
// DESIGN.md 2.20.)  No reference counterpart.
//
// Over random coefficients rho (one per variable) and sigma (one per domain
// row) every query of the key is compared with what the string gives for the
// same combination of the circuit's columns, without a group transform:
//   u^{M,part}_j = sum_i M[j][i] rho^part_i     sparse row products, k_csr_dot_split
//   m^{M,part}   = iNTT_n(u^{M,part})           the coefficients of sum_i rho^part_i M_i(x)
//   sum_i rho_i a_g1[i] = sum_k m^A_k tau_g1[k] an MSM over the key against one over the string
// and likewise for b_g1, b_g2, the two ic arrays (over alpha_tau, beta_tau and
// tau at once) and h_g1 (over tau_g1[0, 2n) with the scalars of k_h_scalars).
// The string's G1 arrays cross PCIe once, into one base vector
//   [alpha_tau_g1[0, n) | beta_tau_g1[0, n) | tau_g1[0, 2n)]
// so that every G1 sum is an MSM over a contiguous range of it.  The MSMs, the
// transforms, the point validation and the host pairing are the library's own.
#include <cstring>
#include <string>
#include <vector>

#include "host_pairing.hpp"
#include "keycheck.hpp"
#include "prove.hpp"
#include "quotient.hpp"
#include "srs.hpp"

namespace zk {

const char* point_status_text(int st);   // points.hip

// ------------------------------------------------------------- kernels ---
// Row `row` of one matrix times rho, split at column l: pub takes the columns
// <= l, priv the rest.  rho is Montgomery, val canonical, so a product comes
// out canonical (rho R * v / R) while a unit entry adds rho R itself: the sums
// of a matrix with values go to Montgomery form at the end.  Duplicate
// (row, col) entries add; a column >= V is skipped, as in row_dot.
ZK_DI void row_dot_split(const uint64_t* __restrict__ rp, const uint32_t* __restrict__ col,
                         const Fr* __restrict__ val, uint64_t row, const Fr* __restrict__ rho, uint64_t V,
                         uint64_t l, Fr& pub, Fr& priv) {
  const uint64_t e = rp[row + 1];
  for (uint64_t k = rp[row]; k < e; k++) {
    const uint32_t c = col[k];
    if (c >= V) continue;
    Fr t = ld_vec(&rho[c]);
    if (val) t = fp_mul(t, ld_vec(&val[k]));
    if (c <= l) pub = fp_add(pub, t);
    else priv = fp_add(priv, t);
  }
  if (val) {
    pub = fp_to_mont(pub);
    priv = fp_to_mont(priv);
  }
}

// One lane per domain row j < n: out[(2 k + part) n + j] = u^{M_k,part}_j
// (Montgomery), k = 0, 1, 2 for A, B, C, part 0 pub and 1 priv; rows >= nc are
// zero padding.
__global__ void __launch_bounds__(256) k_csr_dot_split(CsrArgs m, const Fr* __restrict__ rho, uint64_t nc, uint64_t V,
                                                       uint64_t l, uint64_t n, Fr* __restrict__ out) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
#pragma unroll 1
  for (int k = 0; k < 3; k++) {
    Fr pub = fp_zero<FrParams>(), priv = pub;
    if (j < nc) row_dot_split(m.rp[k], m.col[k], m.val[k], j, rho, V, l, pub, priv);
    st_vec(&out[(2 * k) * n + j], pub);
    st_vec(&out[(2 * k + 1) * n + j], priv);
  }
}

// out[i] = a[i] + b[i], i < n
__global__ void __launch_bounds__(256) k_fr_add(const Fr* __restrict__ a, const Fr* __restrict__ b, size_t n,
                                                Fr* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) st_vec(&out[i], fp_add(ld_vec(&a[i]), ld_vec(&b[i])));
}

// The scalars of sum_i sigma_i (tau_g1[i + n] - tau_g1[i]) over tau_g1[0, 2n):
// d[k] = -sigma_k mod r, d[k + n] = sigma_k, k < n.  sigma and d are canonical
// four-word scalars.
__global__ void __launch_bounds__(256) k_h_scalars(const Fr* __restrict__ sigma, size_t n, Fr* __restrict__ d) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const Fr s = ld_vec(&sigma[k]);
  st_vec(&d[k], fp_neg(s));
  st_vec(&d[k + n], s);
}

// ------------------------------------------------- the coefficient side ---
void key_srs_coeffs_device(zk_ctx* ctx, const zk_r1cs_csr* q, uint64_t num_public, const zk_fr* rho, uint32_t log_n,
                           Fr* d_out, KeySrsScratch& keep) {
  hipStream_t st = ctx->stream;
  const uint64_t V = q->num_variables, nc = q->num_constraints, n = 1ull << log_n;
  const uint64_t* rps[3] = {q->a_rowptr, q->b_rowptr, q->c_rowptr};
  const uint32_t* cols[3] = {q->a_col, q->b_col, q->c_col};
  const zk_fr* vals[3] = {q->a_val, q->b_val, q->c_val};
  CsrArgs m;
  for (int k = 0; k < 3; k++) {
    // the kernel walks [rp[j], rp[j + 1]) of every row: the pointers must ascend to rp[nc]
    for (uint64_t j = 0; j < nc; j++)
      if (rps[k][j] > rps[k][j + 1]) throw Error(ZK_ERR_ARG, "verify_key_srs: a matrix's row pointers do not ascend");
    const uint64_t nnz = nc ? rps[k][nc] : 0;
    keep.rp[k].ensure(8 * (nc + 1));
    keep.col[k].ensure(4 * std::max<uint64_t>(nnz, 1));
    if (nc) ZK_HIP(hipMemcpyAsync(keep.rp[k].p, rps[k], 8 * (nc + 1), hipMemcpyHostToDevice, st));
    if (nnz) ZK_HIP(hipMemcpyAsync(keep.col[k].p, cols[k], 4 * nnz, hipMemcpyHostToDevice, st));
    if (vals[k] && nnz) {
      keep.val[k].ensure(sizeof(zk_fr) * nnz);
      ZK_HIP(hipMemcpyAsync(keep.val[k].p, vals[k], sizeof(zk_fr) * nnz, hipMemcpyHostToDevice, st));
    }
    m.rp[k] = keep.rp[k].as<uint64_t>();
    m.col[k] = keep.col[k].as<uint32_t>();
    m.val[k] = vals[k] && nnz ? keep.val[k].as<Fr>() : nullptr;
  }
  keep.rho.ensure(sizeof(Fr) * V);
  ZK_HIP(hipMemcpyAsync(keep.rho.p, rho, sizeof(zk_fr) * V, hipMemcpyHostToDevice, st));
  fr_to_mont(keep.rho.as<uint64_t>(), keep.rho.as<Fr>(), V, st);

  int ph = ctx->prof.begin(st, "keysrs_split", n);
  k_csr_dot_split<<<ceil_div(n, 256), 256, 0, st>>>(m, keep.rho.as<Fr>(), nc, V, num_public, n, d_out);
  ZK_LAUNCH_CHECK();
  ctx->prof.end(st, ph);
  if (log_n == 0) return;   // a size-1 transform is the identity
  ph = ctx->prof.begin(st, "keysrs_transforms", 6 * n);
  NttDomain& dom = ctx->domain(log_n);
  keep.tmp.ensure(sizeof(Fr) * n);
  Fr ninv;
  const host::Fr nd = host::fr_to_dev(host::fr_inv(host::fr_from_u64(n)));
  std::memcpy(ninv.v, nd.l, 32);
  for (int k = 0; k < 6; k++)
    ntt_natural(d_out + k * n, d_out + k * n, keep.tmp.as<Fr>(), dom, true, st, &ctx->prof, nullptr, nullptr, &ninv);
  ctx->prof.end(st, ph);
}

int key_srs_coeffs_host(zk_ctx* ctx, const zk_r1cs_csr* q, uint64_t num_public, const zk_fr* rho, zk_fr* out) {
  const uint64_t V = q->num_variables, nc = q->num_constraints;
  if (num_public >= V) return ZK_ERR_SETUP_PARAMS;
  if (nc > (1ull << 32)) return ZK_ERR_DOMAIN;
  uint64_t n = 1;
  while (n < nc) n <<= 1;
  for (uint64_t i = 0; i < V; i++)
    if (!fr_canonical(rho[i])) return ZK_ERR_ARG;
  KeySrsScratch keep;
  DevBuf co;
  co.ensure(sizeof(Fr) * 6 * n);
  key_srs_coeffs_device(ctx, q, num_public, rho, (uint32_t)__builtin_ctzll(n), co.as<Fr>(), keep);
  fr_from_mont(co.as<Fr>(), co.as<uint64_t>(), 6 * n, ctx->stream);
  ZK_HIP(hipMemcpyAsync(out, co.p, sizeof(zk_fr) * 6 * n, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  if (ctx->prof.on) ctx->prof.collect();
  return ZK_OK;
}

// ------------------------------------------------------------- helpers ---
// One array of the key through the point validation (the identity is legal: a
// variable absent from a matrix has one).  true when every entry is valid; rc:
// ZK_OK or the call's own failure.  names: one per entry, else name[index].
template <class P>
static bool key_valid(zk_ctx* ctx, const char* name, const char* const* names, const P* pts, size_t n, int& rc) {
  rc = ZK_OK;
  if (!n) return true;
  std::vector<uint8_t> st(n);
  size_t bad = n;
  if constexpr (sizeof(P) == sizeof(zk_g1_affine)) rc = zk_g1_validate(ctx, pts, n, st.data(), &bad);
  else rc = zk_g2_validate(ctx, pts, n, st.data(), &bad);
  if (rc == ZK_OK) return true;
  if (rc != ZK_ERR_ARG || bad >= n) return false;
  rc = ZK_OK;
  ctx->err = (names ? std::string(names[bad]) : std::string(name) + "[" + std::to_string(bad) + "]") + ": " +
             point_status_text(st[bad]);
  return false;
}

static zk_g1_affine identity_g1() {
  zk_g1_affine p;
  std::memset(&p, 0, sizeof p);
  p.infinity = 1;
  return p;
}

// sum k_i P_i over n device bases and n canonical four-word device scalars
template <class C, class ABI>
static ABI msm_sum(zk_ctx* ctx, const typename C::A* d_bases, const uint64_t* d_scal, size_t n) {
  hipStream_t st = ctx->stream;
  MsmWork& w = ctx->msm[0];
  msm_launch<C>(w, d_bases, d_scal, 4, (uint32_t)n, 255, st);
  msm_download<C>(w, st);
  ZK_HIP(hipStreamSynchronize(st));
  ctx->prof.collect();
  ABI out;
  std::memset(&out, 0, sizeof out);
  host_to_abi<C>(msm_finish<C>(w), reinterpret_cast<uint64_t*>(&out));
  return out;
}
// sum k_i P_i over host points and host scalars (the public MSM); n = 0 is the identity
static int key_sum(zk_ctx* ctx, const zk_g1_affine* pts, const zk_fr* k, size_t n, zk_g1_affine& out) {
  HostPhase hp(ctx->prof, "keysrs_msm_key");
  if (!n) {
    out = identity_g1();
    return ZK_OK;
  }
  return zk_msm_g1(ctx, pts, n, k, n, 255, &out);
}

// --------------------------------------------------------- the verdict ---
static int verify_key_srs(zk_ctx* ctx, const zk_r1cs_csr* q, const zk_srs* srs, const zk_pk* pk, const zk_vk* vk,
                          const zk_fr* coeffs, uint32_t log_n, int* status) {
  Range range("zk_verify_key_srs");
  hipStream_t st = ctx->stream;
  const uint64_t V = q->num_variables, l = pk->num_public, n = 1ull << log_n;
  const zk_fr *rho = coeffs, *sigma = coeffs + V;
  int rc = ZK_OK;

  *status = ZK_KEYSRS_POINT;
  {
    HostPhase hp(ctx->prof, "keysrs_validate");
    const zk_g1_affine p1[4] = {pk->alpha_g1, pk->beta_g1, pk->delta_g1, vk->alpha_g1};
    const char* const n1[4] = {"pk.alpha_g1", "pk.beta_g1", "pk.delta_g1", "vk.alpha_g1"};
    const zk_g2_affine p2[5] = {pk->beta_g2, pk->delta_g2, vk->beta_g2, vk->gamma_g2, vk->delta_g2};
    const char* const n2[5] = {"pk.beta_g2", "pk.delta_g2", "vk.beta_g2", "vk.gamma_g2", "vk.delta_g2"};
    if (!key_valid(ctx, nullptr, n1, p1, 4, rc) || !key_valid(ctx, nullptr, n2, p2, 5, rc) ||
        !key_valid(ctx, "pk.a_g1", nullptr, pk->a_g1, pk->a_len, rc) ||
        !key_valid(ctx, "pk.b_g1", nullptr, pk->b_g1, pk->b_len, rc) ||
        !key_valid(ctx, "pk.b_g2", nullptr, pk->b_g2, pk->b2_len, rc) ||
        !key_valid(ctx, "pk.ic_g1", nullptr, pk->ic_g1, pk->ic_len, rc) ||
        !key_valid(ctx, "pk.h_g1", nullptr, pk->h_g1, pk->h_len, rc) ||
        !key_valid(ctx, "vk.ic_g1", nullptr, vk->ic_g1, vk->ic_len, rc))
      return rc;
  }

  *status = ZK_KEYSRS_FIXED;
  zk_g1_affine g1;
  zk_g2_affine g2;
  generators(ctx, g1, g2);
  if (!same_g1(pk->alpha_g1, srs->alpha_tau_g1[0]) || !same_g1(vk->alpha_g1, srs->alpha_tau_g1[0]) ||
      !same_g1(pk->beta_g1, srs->beta_tau_g1[0]) || !same_g2(pk->beta_g2, srs->beta_g2) ||
      !same_g2(vk->beta_g2, srs->beta_g2) || !same_g2(vk->gamma_g2, g2) || !same_g2(vk->delta_g2, pk->delta_g2))
    return ZK_OK;

  *status = ZK_KEYSRS_DELTA;
  if (pk->delta_g1.infinity || pk->delta_g2.infinity) return ZK_OK;
  {
    HostPhase hp(ctx->prof, "keysrs_pairing");
    if (!pairs_equal(pk->delta_g1, g2, g1, pk->delta_g2)) return ZK_OK;
  }

  // ---- the coefficient vectors, and the scalars of the string's MSMs ----
  KeySrsScratch keep;
  DevBuf co, sum, scal, sig;
  co.ensure(sizeof(Fr) * 6 * n);
  key_srs_coeffs_device(ctx, q, l, rho, log_n, co.as<Fr>(), keep);
  const Fr* mv = co.as<Fr>();   // A pub, A priv, B pub, B priv, C pub, C priv
  int ph = ctx->prof.begin(st, "keysrs_scalars", 10 * n);
  // m^A and m^B whole, as scalars: sc_ab = [m^A | m^B]
  sum.ensure(sizeof(Fr) * 2 * n);
  for (int k = 0; k < 2; k++) {
    k_fr_add<<<ceil_div(n, 256), 256, 0, st>>>(mv + 2 * k * n, mv + (2 * k + 1) * n, n, sum.as<Fr>() + k * n);
    ZK_LAUNCH_CHECK();
  }
  // sc_ab, then per part [m^B | m^A | m^C] against [alpha_tau | beta_tau | tau], then the h scalars
  scal.ensure(sizeof(zk_fr) * 10 * n);
  uint64_t* sc_ab = scal.as<uint64_t>();
  uint64_t* sc_t[2] = {sc_ab + 4 * 2 * n, sc_ab + 4 * 5 * n};
  uint64_t* sc_h = sc_ab + 4 * 8 * n;
  fr_to_scalars(sum.as<Fr>(), 2 * n, 4, sc_ab, st);
  for (int part = 0; part < 2; part++) {
    fr_to_scalars(mv + (2 + part) * n, n, 4, sc_t[part], st);
    fr_to_scalars(mv + (0 + part) * n, n, 4, sc_t[part] + 4 * n, st);
    fr_to_scalars(mv + (4 + part) * n, n, 4, sc_t[part] + 4 * 2 * n, st);
  }
  sig.ensure(sizeof(zk_fr) * n);
  ZK_HIP(hipMemcpyAsync(sig.p, sigma, sizeof(zk_fr) * n, hipMemcpyHostToDevice, st));
  k_h_scalars<<<ceil_div(n, 256), 256, 0, st>>>(sig.as<Fr>(), n, reinterpret_cast<Fr*>(sc_h));
  ZK_LAUNCH_CHECK();
  ctx->prof.end(st, ph);

  // ---- the string, once: [alpha_tau | beta_tau | tau[0, 2n)] and tau_g2[0, n) ----
  DevBuf raw, b1, b2;
  raw.ensure(std::max(sizeof(zk_g1_affine) * 4 * n, sizeof(zk_g2_affine) * n));
  b1.ensure(sizeof(G1A) * 4 * n);
  b2.ensure(sizeof(G2A) * n);
  ph = ctx->prof.begin(st, "keysrs_upload", 5 * n);
  char* r8 = raw.as<char>();
  chunked_copy(ctx, r8, srs->alpha_tau_g1, n, sizeof(zk_g1_affine), hipMemcpyHostToDevice);
  chunked_copy(ctx, r8 + sizeof(zk_g1_affine) * n, srs->beta_tau_g1, n, sizeof(zk_g1_affine), hipMemcpyHostToDevice);
  chunked_copy(ctx, r8 + sizeof(zk_g1_affine) * 2 * n, srs->tau_g1, 2 * n, sizeof(zk_g1_affine), hipMemcpyHostToDevice);
  convert_bases<G1>(raw.as<uint64_t>(), b1.as<G1A>(), 4 * n, st);
  chunked_copy(ctx, r8, srs->tau_g2, n, sizeof(zk_g2_affine), hipMemcpyHostToDevice);
  convert_bases<G2>(raw.as<uint64_t>(), b2.as<G2A>(), n, st);
  ctx->prof.end(st, ph);
  const G1A *alpha_tau = b1.as<G1A>(), *tau = alpha_tau + 2 * n;

  auto srs_sum_g1 = [&](const G1A* bases, const uint64_t* sc, size_t cnt) {
    HostPhase hp(ctx->prof, "keysrs_msm_srs");
    return msm_sum<G1, zk_g1_affine>(ctx, bases, sc, cnt);
  };
  zk_g1_affine key, str;

  *status = ZK_KEYSRS_QUERY_A;
  if ((rc = key_sum(ctx, pk->a_g1, rho, V, key)) != ZK_OK) return rc;
  str = srs_sum_g1(tau, sc_ab, n);
  if (!same_g1(key, str)) return ZK_OK;

  *status = ZK_KEYSRS_QUERY_B1;
  if ((rc = key_sum(ctx, pk->b_g1, rho, V, key)) != ZK_OK) return rc;
  str = srs_sum_g1(tau, sc_ab + 4 * n, n);
  if (!same_g1(key, str)) return ZK_OK;

  *status = ZK_KEYSRS_QUERY_B2;
  {
    zk_g2_affine key2, str2;
    {
      HostPhase hp(ctx->prof, "keysrs_msm_key");
      if ((rc = zk_msm_g2(ctx, pk->b_g2, V, rho, V, 255, &key2)) != ZK_OK) return rc;
    }
    {
      HostPhase hp(ctx->prof, "keysrs_msm_srs");
      str2 = msm_sum<G2, zk_g2_affine>(ctx, b2.as<G2A>(), sc_ab + 4 * n, n);
    }
    if (!same_g2(key2, str2)) return ZK_OK;
  }

  *status = ZK_KEYSRS_IC_VK;   // gamma = 1: the vk's entries are undivided
  if ((rc = key_sum(ctx, vk->ic_g1, rho, l + 1, key)) != ZK_OK) return rc;
  str = srs_sum_g1(alpha_tau, sc_t[0], 3 * n);
  if (!same_g1(key, str)) return ZK_OK;

  *status = ZK_KEYSRS_IC_PK;
  if ((rc = key_sum(ctx, pk->ic_g1, rho + l + 1, V - l - 1, key)) != ZK_OK) return rc;
  str = srs_sum_g1(alpha_tau, sc_t[1], 3 * n);
  {
    HostPhase hp(ctx->prof, "keysrs_pairing");
    if (!pairs_equal(key, pk->delta_g2, str, g2)) return ZK_OK;
  }

  *status = ZK_KEYSRS_H;
  if ((rc = key_sum(ctx, pk->h_g1, sigma, n, key)) != ZK_OK) return rc;
  str = srs_sum_g1(tau, sc_h, 2 * n);
  {
    HostPhase hp(ctx->prof, "keysrs_pairing");
    if (!pairs_equal(key, pk->delta_g2, str, g2)) return ZK_OK;
  }
  *status = ZK_KEYSRS_OK;
  return ZK_OK;
}

}  // namespace zk

using namespace zk;

#define ZK_KGUARD(ctx, ...)                                   \
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

int zk_groth16_verify_key_srs_sound(zk_ctx* ctx, const zk_r1cs_csr* qap, const zk_srs* srs, const zk_pk* pk,
                                    const zk_vk* vk, const zk_fr* coeffs, size_t n_coeffs, int* status) {
  if (!ctx || !qap || !srs || !pk || !vk || !status || (n_coeffs && !coeffs)) return ZK_ERR_ARG;
  if (!srs->tau_g1 || !srs->tau_g2 || !srs->alpha_tau_g1 || !srs->beta_tau_g1) return ZK_ERR_ARG;
  // the circuit against the string, with the codes of zk_groth16_setup_srs_sound
  const uint64_t V = qap->num_variables, nc = qap->num_constraints, l = pk->num_public;
  if (l >= V) return ZK_ERR_SETUP_PARAMS;
  if (nc > (1ull << 32) || srs->log_n > 31) return ZK_ERR_DOMAIN;
  uint64_t n = 1;
  while (n < nc) n <<= 1;
  const uint64_t N = 1ull << srs->log_n;
  if (n > N || srs->tau_g1_len < 2 * N || srs->tau_g2_len < N || srs->alpha_len < N || srs->beta_len < N) {
    ctx->err = "verify_key_srs: the circuit's domain is " + std::to_string(n) + ", the string serves " +
               std::to_string(N) + " (or its arrays are shorter than log_n states)";
    return ZK_ERR_DOMAIN;
  }
  // an MSM counts its bases in 31 bits: 3 n for the ic sums
  if (V >= 0x80000000ull || n > 0x20000000ull) return ZK_ERR_ARG;

  *status = ZK_KEYSRS_SHAPE;
  if (pk->a_len != V || pk->b_len != V || pk->b2_len != V || pk->ic_len != V - l - 1 || pk->h_len != n ||
      vk->ic_len != l + 1 || vk->num_public != l || n_coeffs != V + n)
    return ZK_OK;
  if (!pk->a_g1 || !pk->b_g1 || !pk->b_g2 || !pk->h_g1 || !vk->ic_g1 || (pk->ic_len && !pk->ic_g1)) return ZK_ERR_ARG;
  for (size_t i = 0; i < n_coeffs; i++)
    if (!(coeffs[i].l[0] | coeffs[i].l[1]) || coeffs[i].l[2] || coeffs[i].l[3]) {
      ctx->err = "verify_key_srs: coefficient " + std::to_string(i) + " must be non-zero and below 2^128";
      return ZK_ERR_ARG;
    }
  ZK_KGUARD(ctx, {
    const int rc = verify_key_srs(ctx, qap, srs, pk, vk, coeffs, (uint32_t)__builtin_ctzll(n), status);
    if (ctx->prof.on) ctx->prof.collect();
    return rc;
  })
}
