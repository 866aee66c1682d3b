// lagrange.hip -- prepared powers-of-tau strings (include/zkp.h, "prepared
// powers-of-tau strings").  No reference counterpart.
//
//   zk_srs_prepare                        the upper half of zk_groth16_setup_srs_sound
//                                         (srs.hip), kept on the device: zk_srs_dev
//   zk_srs_dev_export / _import           the handle <-> canonical host points
//   zk_srs_lagrange_verify                a prepared string against its monomial
//                                         string: MSMs under random coefficients
//   zk_groth16_setup_prepared_sound       the lower half, reading the handle
//   zk_groth16_setup_prepared_sound_dev   the same sums straight into a zk_pk_dev
//
// The transforms, the column sums and the differences are srs.hip's kernels,
// launched through the halves srs.hpp declares.  What is new on the device is
// the filling of a key slot from device affine points: one byte per point says
// whether it is the identity, the host picks the kept positions as for every
// other key (shard_positions), and a gather compacts them into the slot.
#include <cstring>
#include <string>
#include <vector>

#include "key.hpp"
#include "prove.hpp"
#include "srs.hpp"

struct zk_srs_dev {
  int device = 0;
  uint32_t log_n = 0;
  zk::DevBuf L1, L2, H;   // [L | alpha L | beta L]_1 (3 n), [L]_2 (n), tau_g1[i + n] - tau_g1[i] (n): device affine
  zk_g1_affine alpha_g1, beta_g1;
  zk_g2_affine beta_g2;
  uint64_t n() const { return 1ull << log_n; }
};

namespace zk {

// ------------------------------------------------------------- kernels ---
// out[i] = 1 where in[i] is the identity ((0, 0)), else 0
template <class A>
ZK_DI void lag_identity(const A* __restrict__ in, size_t n, uint8_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * GN_BLOCK + threadIdx.x;
  if (i >= n) return;
  out[i] = aff_is_inf(ld_vec(&in[i])) ? 1 : 0;
}
__global__ void __launch_bounds__(GN_BLOCK) k_lag_identity_g1(const G1A* __restrict__ in, size_t n,
                                                              uint8_t* __restrict__ out) {
  lag_identity(in, n, out);
}
__global__ void __launch_bounds__(GN_BLOCK) k_lag_identity_g2(const G2A* __restrict__ in, size_t n,
                                                              uint8_t* __restrict__ out) {
  lag_identity(in, n, out);
}
// out[k] = in[pos[k]], k < cnt (pos[k] < the length of in: shard_positions)
template <class A>
ZK_DI void lag_gather(const A* __restrict__ in, const uint32_t* __restrict__ pos, size_t cnt, A* __restrict__ out) {
  const size_t k = (size_t)blockIdx.x * GN_BLOCK + threadIdx.x;
  if (k >= cnt) return;
  st_vec(&out[k], ld_vec(&in[pos[k]]));
}
__global__ void __launch_bounds__(GN_BLOCK) k_lag_gather_g1(const G1A* __restrict__ in, const uint32_t* __restrict__ pos,
                                                            size_t cnt, G1A* __restrict__ out) {
  lag_gather(in, pos, cnt, out);
}
__global__ void __launch_bounds__(GN_BLOCK) k_lag_gather_g2(const G2A* __restrict__ in, const uint32_t* __restrict__ pos,
                                                            size_t cnt, G2A* __restrict__ out) {
  lag_gather(in, pos, cnt, out);
}

// ------------------------------------------------------------- prepare ---
static int srs_prepare(zk_ctx* ctx, const zk_srs* srs, uint32_t log_n, zk_srs_dev** out) {
  Range range("zk_srs_prepare");
  if (srs->log_n > 31) return ZK_ERR_DOMAIN;
  const uint64_t N = 1ull << srs->log_n;
  if (log_n > srs->log_n || srs->tau_g1_len < 2 * N || srs->tau_g2_len < N || srs->alpha_len < N || srs->beta_len < N) {
    ctx->err = "srs_prepare: the domain asked for is 2^" + std::to_string(log_n) + ", the string serves " +
               std::to_string(N) + " (or its arrays are shorter than log_n states)";
    return ZK_ERR_DOMAIN;
  }
  const uint64_t n = 1ull << log_n;
  // three blocks of n rows in one u32 index (the mixed ic sum)
  if (n > 0x40000000ull) return ZK_ERR_ARG;
  if (same_g1(srs->tau_g1[n], srs->tau_g1[0])) {
    ctx->err = "sound setup: tau lies on the evaluation domain (Z(tau) = 0)";
    return ZK_ERR_SETUP_PARAMS;
  }
  std::unique_ptr<zk_srs_dev> d(new zk_srs_dev());
  d->device = ctx->device;
  d->log_n = log_n;
  d->alpha_g1 = srs->alpha_tau_g1[0];
  d->beta_g1 = srs->beta_tau_g1[0];
  d->beta_g2 = srs->beta_g2;
  DevBuf d_abi;
  d_abi.ensure(std::max(sizeof(zk_g1_affine) * 2 * n, sizeof(zk_g2_affine) * n));
  d->L1.ensure(sizeof(G1A) * 3 * n);
  d->L2.ensure(sizeof(G2A) * n);
  d->H.ensure(sizeof(G1A) * n);
  srs_lagrange_transforms(ctx, srs, log_n, d_abi.p, d->L1.as<G1A>(), d->L2.as<G2A>());
  srs_hdiff(ctx, srs->tau_g1, n, d_abi.p, d->H.as<G1A>());
  if (ctx->prof.on) ctx->prof.collect();
  *out = d.release();
  return ZK_OK;
}

// ---------------------------------------------------- export and import ---
static int srs_dev_export(zk_ctx* ctx, const zk_srs_dev* p, zk_srs_lagrange* out) {
  const uint64_t n = p->n();
  const G1A* L1 = p->L1.as<G1A>();
  affine_to_host<FqC>(ctx, L1, n, out->l_g1);
  affine_to_host<FqC>(ctx, L1 + n, n, out->alpha_l_g1);
  affine_to_host<FqC>(ctx, L1 + 2 * n, n, out->beta_l_g1);
  affine_to_host<Fq2C>(ctx, p->L2.as<G2A>(), n, out->l_g2);
  affine_to_host<FqC>(ctx, p->H.as<G1A>(), n, out->h_g1);
  out->log_n = p->log_n;
  out->alpha_g1 = p->alpha_g1;
  out->beta_g1 = p->beta_g1;
  out->beta_g2 = p->beta_g2;
  return ZK_OK;
}

static int srs_dev_import(zk_ctx* ctx, const zk_srs_lagrange* lag, zk_srs_dev** out) {
  hipStream_t st = ctx->stream;
  const uint64_t n = 1ull << lag->log_n;
  std::unique_ptr<zk_srs_dev> d(new zk_srs_dev());
  d->device = ctx->device;
  d->log_n = lag->log_n;
  d->alpha_g1 = lag->alpha_g1;
  d->beta_g1 = lag->beta_g1;
  d->beta_g2 = lag->beta_g2;
  DevBuf raw;
  raw.ensure(sizeof(zk_g2_affine) * n);
  d->L1.ensure(sizeof(G1A) * 3 * n);
  d->L2.ensure(sizeof(G2A) * n);
  d->H.ensure(sizeof(G1A) * n);
  const zk_g1_affine* src[4] = {lag->l_g1, lag->alpha_l_g1, lag->beta_l_g1, lag->h_g1};
  G1A* dst[4] = {d->L1.as<G1A>(), d->L1.as<G1A>() + n, d->L1.as<G1A>() + 2 * n, d->H.as<G1A>()};
  for (int k = 0; k < 4; k++) {
    chunked_copy(ctx, raw.p, src[k], n, sizeof(zk_g1_affine), hipMemcpyHostToDevice);
    convert_bases<G1>(raw.as<uint64_t>(), dst[k], n, st);
  }
  chunked_copy(ctx, raw.p, lag->l_g2, n, sizeof(zk_g2_affine), hipMemcpyHostToDevice);
  convert_bases<G2>(raw.as<uint64_t>(), d->L2.as<G2A>(), n, st);
  ZK_HIP(hipStreamSynchronize(st));   // raw dies here
  *out = d.release();
  return ZK_OK;
}

// -------------------------------------------------------------- verify ---
static int lagrange_verify(zk_ctx* ctx, const zk_srs* srs, const zk_srs_lagrange* lag, const zk_fr* rho, int* status) {
  Range range("zk_srs_lagrange_verify");
  const uint64_t n = 1ull << lag->log_n;
  int rc = ZK_OK;
  *status = ZK_LAG_POINT;
  {
    HostPhase hp(ctx->prof, "lag_validate");
    if (!srs_valid(ctx, "l_g1", lag->l_g1, n, rc) || !srs_valid(ctx, "alpha_l_g1", lag->alpha_l_g1, n, rc) ||
        !srs_valid(ctx, "beta_l_g1", lag->beta_l_g1, n, rc) || !srs_valid(ctx, "l_g2", lag->l_g2, n, rc) ||
        !srs_valid(ctx, "h_g1", lag->h_g1, n, rc) || !srs_valid(ctx, "alpha_g1", &lag->alpha_g1, 1, rc) ||
        !srs_valid(ctx, "beta_g1", &lag->beta_g1, 1, rc) || !srs_valid(ctx, "beta_g2", &lag->beta_g2, 1, rc))
      return rc;
  }
  *status = ZK_LAG_FIXED;
  if (!same_g1(lag->alpha_g1, srs->alpha_tau_g1[0]) || !same_g1(lag->beta_g1, srs->beta_tau_g1[0]) ||
      !same_g2(lag->beta_g2, srs->beta_g2))
    return ZK_OK;

  // c = the inverse transform of rho: sum_i rho_i [L_i] = sum_k c_k [tau^k]
  std::vector<zk_fr> c(rho, rho + n);
  {
    HostPhase hp(ctx->prof, "lag_scalars");
    if ((rc = zk_ntt_fr(ctx, c.data(), lag->log_n, -1, nullptr)) != ZK_OK) return rc;
  }
  const zk_g1_affine* lag1[3] = {lag->l_g1, lag->alpha_l_g1, lag->beta_l_g1};
  const zk_g1_affine* srs1[3] = {srs->tau_g1, srs->alpha_tau_g1, srs->beta_tau_g1};
  const int st1[3] = {ZK_LAG_LAGRANGE_G1, ZK_LAG_ALPHA, ZK_LAG_BETA};
  for (int k = 0; k < 3; k++) {
    *status = st1[k];
    zk_g1_affine a, b;
    {
      HostPhase hp(ctx->prof, "lag_msm_lagrange");
      if ((rc = zk_msm_g1(ctx, lag1[k], n, rho, n, 128, &a)) != ZK_OK) return rc;
    }
    {
      HostPhase hp(ctx->prof, "lag_msm_srs");
      if ((rc = zk_msm_g1(ctx, srs1[k], n, c.data(), n, 255, &b)) != ZK_OK) return rc;
    }
    if (!same_g1(a, b)) return ZK_OK;
  }
  *status = ZK_LAG_LAGRANGE_G2;
  {
    zk_g2_affine a, b;
    {
      HostPhase hp(ctx->prof, "lag_msm_lagrange");
      if ((rc = zk_msm_g2(ctx, lag->l_g2, n, rho, n, 128, &a)) != ZK_OK) return rc;
    }
    {
      HostPhase hp(ctx->prof, "lag_msm_srs");
      if ((rc = zk_msm_g2(ctx, srs->tau_g2, n, c.data(), n, 255, &b)) != ZK_OK) return rc;
    }
    if (!same_g2(a, b)) return ZK_OK;
  }
  *status = ZK_LAG_H;
  {
    DevBuf d_abi, d_aff;
    d_abi.ensure(sizeof(zk_g1_affine) * 2 * n);
    d_aff.ensure(sizeof(G1A) * n);
    std::vector<zk_g1_affine> h(n);
    srs_hdiff(ctx, srs->tau_g1, n, d_abi.p, d_aff.as<G1A>());
    affine_to_host<FqC>(ctx, d_aff.as<G1A>(), n, h.data());
    for (uint64_t i = 0; i < n; i++)
      if (!same_g1(h[i], lag->h_g1[i])) {
        ctx->err = "h_g1[" + std::to_string(i) + "]: not tau_g1[i + n] - tau_g1[i]";
        return ZK_OK;
      }
  }
  *status = ZK_LAG_OK;
  return ZK_OK;
}

// ------------------------------------------------------------ the keys ---
// The circuit against the handle, with the codes of zk_groth16_setup_srs_sound
static int prepared_checks(zk_ctx* ctx, const zk_r1cs_csr* q, const zk_srs_dev* p, uint64_t num_public) {
  const uint64_t V = q->num_variables, nc = q->num_constraints;
  if (num_public >= V) return ZK_ERR_SETUP_PARAMS;
  if (nc > (1ull << 32)) return ZK_ERR_DOMAIN;
  uint64_t n = 1;
  while (n < nc) n <<= 1;
  if (n != p->n()) {
    ctx->err = "setup from a prepared string: the circuit's domain is " + std::to_string(n) +
               ", the string was prepared for " + std::to_string(p->n()) + " (a Lagrange basis serves one size)";
    return ZK_ERR_DOMAIN;
  }
  if (V >= 0x80000000ull || n > 0x40000000ull) return ZK_ERR_ARG;
  if (p->device != ctx->device) {
    ctx->err = "setup from a prepared string: the handle belongs to another device";
    return ZK_ERR_ARG;
  }
  return ZK_OK;
}

static int setup_prepared(zk_ctx* ctx, const zk_r1cs_csr* q, const zk_srs_dev* p, uint64_t num_public, zk_pk* pk,
                          zk_vk* vk) {
  Range range("zk_setup_prepared");
  const int rc = prepared_checks(ctx, q, p, num_public);
  if (rc != ZK_OK) return rc;
  const uint64_t V = q->num_variables, n = p->n();
  // everything into scratch: the keys change only once nothing can fail
  SrsHostKey key(V, n);
  srs_column_sums(ctx, q, n, p->L1.as<G1A>(), p->L2.as<G2A>(), [&](int which, const void* d) {
    HostPhase hp(ctx->prof, "prepared_download");
    key.take(ctx, which, d);
  });
  {
    HostPhase hp(ctx->prof, "prepared_download");
    affine_to_host<FqC>(ctx, p->H.as<G1A>(), n, key.h.data());
  }
  zk_g1_affine g1;
  zk_g2_affine g2;
  generators(ctx, g1, g2);
  if (ctx->prof.on) ctx->prof.collect();
  HostPhase hp(ctx->prof, "prepared_fill_host");
  key.fill(p->alpha_g1, p->beta_g1, p->beta_g2, g1, g2, num_public, pk, vk);
  return ZK_OK;
}

// One slot of a device key from `len` device affine points: the identity
// bytes, the kept positions, the gather.
template <class A>
static void fill_slot_from_points(zk_ctx* ctx, zk_pk_dev& pk, const SlotShape& sh, const A* d_src, const KeyExtras& ex) {
  constexpr bool IS_G2 = sizeof(A) == sizeof(G2A);
  HostPhase hp(ctx->prof, "prepared_dev_fill");
  hipStream_t st = ctx->stream;
  const size_t len = sh.len;
  std::vector<uint8_t> ident(std::max<size_t>(len, 1));
  if (len) {
    DevBuf d_id;
    d_id.ensure(len);
    if constexpr (IS_G2) k_lag_identity_g2<<<ceil_div(len, GN_BLOCK), GN_BLOCK, 0, st>>>(d_src, len, d_id.as<uint8_t>());
    else k_lag_identity_g1<<<ceil_div(len, GN_BLOCK), GN_BLOCK, 0, st>>>(d_src, len, d_id.as<uint8_t>());
    ZK_LAUNCH_CHECK();
    ZK_HIP(hipMemcpyAsync(ident.data(), d_id.p, len, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));   // d_id dies here
  }
  const std::vector<uint32_t> pos = shard_positions(sh, 0, 1, {}, ident.data(), 1);
  pk_fill_slot(pk, sh, pos, ex, st, [&](const std::vector<uint32_t>& kept, void* d_out) {
    DevBuf dpos;
    dpos.ensure(sizeof(uint32_t) * kept.size());
    ZK_HIP(hipMemcpyAsync(dpos.p, kept.data(), sizeof(uint32_t) * kept.size(), hipMemcpyHostToDevice, st));
    if constexpr (IS_G2)
      k_lag_gather_g2<<<ceil_div(kept.size(), GN_BLOCK), GN_BLOCK, 0, st>>>(d_src, dpos.as<uint32_t>(), kept.size(),
                                                                            static_cast<G2A*>(d_out));
    else
      k_lag_gather_g1<<<ceil_div(kept.size(), GN_BLOCK), GN_BLOCK, 0, st>>>(d_src, dpos.as<uint32_t>(), kept.size(),
                                                                            static_cast<G1A*>(d_out));
    ZK_LAUNCH_CHECK();
    ZK_HIP(hipStreamSynchronize(st));   // dpos dies here
  });
}

static int setup_prepared_dev(zk_ctx* ctx, const zk_r1cs_csr* q, const zk_srs_dev* p, uint64_t num_public,
                              zk_pk_dev** pk_out, zk_vk* vk) {
  Range range("zk_setup_prepared_dev");
  const int rc = prepared_checks(ctx, q, p, num_public);
  if (rc != ZK_OK) return rc;
  hipStream_t st = ctx->stream;
  const uint64_t V = q->num_variables, n = p->n(), nvk = num_public + 1, nic = V - nvk;
  zk_g1_affine g1;
  zk_g2_affine g2;
  generators(ctx, g1, g2);
  std::unique_ptr<zk_pk_dev> d;
  {
    HostPhase hp(ctx->prof, "prepared_dev_create");
    d = pk_create(ctx, q, num_public, 0, 1, true);
  }
  const KeyExtras ex = key_extras(0, p->alpha_g1, p->beta_g1, g1, p->beta_g2, g2, true);
  std::vector<zk_g1_affine> vk_ic(vk ? nvk : 0);
  srs_column_sums(ctx, q, n, p->L1.as<G1A>(), p->L2.as<G2A>(), [&](int which, const void* dp) {
    const G1A* p1 = static_cast<const G1A*>(dp);
    if (which == SRS_SUM_A) {
      fill_slot_from_points(ctx, *d, {MSM_A, V, 0, false}, p1, ex);
    } else if (which == SRS_SUM_B1) {
      fill_slot_from_points(ctx, *d, {MSM_B1, V, 0, false}, p1, ex);
    } else if (which == SRS_SUM_B2) {
      fill_slot_from_points(ctx, *d, {MSM_B2, V, 0, false}, static_cast<const G2A*>(dp), ex);
    } else {
      if (vk) affine_to_host<FqC>(ctx, p1, nvk, vk_ic.data());
      fill_slot_from_points(ctx, *d, {MSM_IC, nic, nvk, false}, p1 + nvk, ex);
    }
  });
  fill_slot_from_points(ctx, *d, {MSM_H, n, 0, true}, p->H.as<G1A>(), ex);
  {
    HostPhase hp(ctx->prof, "prepared_dev_finish");
    pk_finish(ctx, *d, q, {}, st);
  }
  if (ctx->prof.on) ctx->prof.collect();
  if (vk) {
    srs_key_header(p->alpha_g1, p->beta_g1, p->beta_g2, g1, g2, V, n, num_public, nullptr, vk);
    std::memcpy(vk->ic_g1, vk_ic.data(), sizeof(zk_g1_affine) * nvk);
  }
  *pk_out = d.release();
  return ZK_OK;
}

}  // namespace zk

using namespace zk;

#define ZK_LGUARD(ctx, ...)                                   \
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

int zk_srs_prepare(zk_ctx* ctx, const zk_srs* srs, uint32_t log_n, zk_srs_dev** out) {
  if (!ctx || !srs || !out || !srs->tau_g1 || !srs->tau_g2 || !srs->alpha_tau_g1 || !srs->beta_tau_g1) return ZK_ERR_ARG;
  ZK_LGUARD(ctx, { return srs_prepare(ctx, srs, log_n, out); })
}

void zk_srs_dev_free(zk_srs_dev* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  delete p;
}

int zk_srs_dev_log_n(const zk_srs_dev* p, uint32_t* log_n) {
  if (!p || !log_n) return ZK_ERR_ARG;
  *log_n = p->log_n;
  return ZK_OK;
}

int zk_srs_dev_bytes(const zk_srs_dev* p, uint64_t* bytes) {
  if (!p || !bytes) return ZK_ERR_ARG;
  *bytes = p->L1.bytes + p->L2.bytes + p->H.bytes;
  return ZK_OK;
}

int zk_srs_dev_export(zk_ctx* ctx, const zk_srs_dev* p, zk_srs_lagrange* out) {
  if (!ctx || !p || !out) return ZK_ERR_ARG;
  if (!out->l_g1 || !out->alpha_l_g1 || !out->beta_l_g1 || !out->h_g1 || !out->l_g2 || out->len < p->n()) {
    ctx->err = "srs_dev_export: every array must hold 2^log_n entries";
    return ZK_ERR_ARG;
  }
  if (p->device != ctx->device) return ZK_ERR_ARG;
  ZK_LGUARD(ctx, { return srs_dev_export(ctx, p, out); })
}

int zk_srs_dev_import(zk_ctx* ctx, const zk_srs_lagrange* lag, zk_srs_dev** out) {
  if (!ctx || !lag || !out) return ZK_ERR_ARG;
  if (lag->log_n > 31) return ZK_ERR_DOMAIN;
  if (!lag->l_g1 || !lag->alpha_l_g1 || !lag->beta_l_g1 || !lag->h_g1 || !lag->l_g2 ||
      lag->len < (1ull << lag->log_n)) {
    ctx->err = "srs_dev_import: every array must hold 2^log_n entries";
    return ZK_ERR_ARG;
  }
  if ((1ull << lag->log_n) > 0x40000000ull) return ZK_ERR_ARG;
  ZK_LGUARD(ctx, { return srs_dev_import(ctx, lag, out); })
}

int zk_srs_lagrange_verify(zk_ctx* ctx, const zk_srs* srs, const zk_srs_lagrange* lag, const zk_fr* coeffs,
                           size_t n_coeffs, int* status) {
  if (!ctx || !srs || !lag || !status || (n_coeffs && !coeffs)) return ZK_ERR_ARG;
  *status = ZK_LAG_SHAPE;
  if (srs->log_n > 31 || lag->log_n > srs->log_n) return ZK_OK;
  const uint64_t N = 1ull << srs->log_n, n = 1ull << lag->log_n;
  if (srs->tau_g1_len < 2 * N || srs->tau_g2_len < N || srs->alpha_len < N || srs->beta_len < N || lag->len < n ||
      n_coeffs != n)
    return ZK_OK;
  if (!srs->tau_g1 || !srs->tau_g2 || !srs->alpha_tau_g1 || !srs->beta_tau_g1 || !lag->l_g1 || !lag->alpha_l_g1 ||
      !lag->beta_l_g1 || !lag->h_g1 || !lag->l_g2)
    return ZK_ERR_ARG;
  for (size_t i = 0; i < n_coeffs; i++)
    if (!(coeffs[i].l[0] | coeffs[i].l[1]) || coeffs[i].l[2] || coeffs[i].l[3]) {
      ctx->err = "srs_lagrange_verify: coefficient " + std::to_string(i) + " must be non-zero and below 2^128";
      return ZK_ERR_ARG;
    }
  ZK_LGUARD(ctx, {
    const int rc = lagrange_verify(ctx, srs, lag, coeffs, status);
    if (ctx->prof.on) ctx->prof.collect();
    return rc;
  })
}

int zk_groth16_setup_prepared_sound(zk_ctx* ctx, const zk_r1cs_csr* qap, const zk_srs_dev* p, uint64_t num_public,
                                    zk_pk* pk, zk_vk* vk) {
  if (!ctx || !qap || !p || !pk) return ZK_ERR_ARG;
  if (!pk->a_g1 || !pk->b_g1 || !pk->b_g2 || !pk->h_g1 || (vk && !vk->ic_g1)) return ZK_ERR_ARG;
  if (qap->num_variables > num_public + 1 && !pk->ic_g1) return ZK_ERR_ARG;
  ZK_LGUARD(ctx, { return setup_prepared(ctx, qap, p, num_public, pk, vk); })
}

int zk_groth16_setup_prepared_sound_dev(zk_ctx* ctx, const zk_r1cs_csr* qap, const zk_srs_dev* p, uint64_t num_public,
                                        zk_pk_dev** pk_out, zk_vk* vk) {
  if (!ctx || !qap || !p || !pk_out || (vk && !vk->ic_g1)) return ZK_ERR_ARG;
  ZK_LGUARD(ctx, { return setup_prepared_dev(ctx, qap, p, num_public, pk_out, vk); })
}
