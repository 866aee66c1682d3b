// prepared.hip -- prepared verification keys (prepared.hpp; include/zkp.h
// "prepared verification keys").
//
//   zk_vk_prepare              validate every point of the key (subgroup
//                              included), make pairing.hip's per-key words once,
//                              build the window table of ic_g1[1 ..] on the GPU
//   zk_groth16_prepare_inputs  IC = ic[0] + sum x_k ic[k + 1] for n rows of inputs
//
// The sums are fixed-base work: input k's window w selects one table entry
// [d 2^(b w)] ic[k + 1] by the digit d of x_k, so a proof's sum is at most
// T = num_public W mixed additions.  They hang on nobody's critical chain, so
// they are cut into runs of L consecutive terms, one lane per run
// (k_prep_runs), and a second level adds a proof's runs (k_prep_fold) -- the
// shape of srs.hip's column sums, with its helpers (srs.hpp).  Digits are read
// from the input words; no index array exists.  Every trip count is a kernel
// argument, the same in every lane: a term past the end, a
// zero digit and an identity entry are selected away after the addition
// instead of branched around.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "mulvec.hpp"
#include "pairing.hpp"
#include "prepared.hpp"

namespace zk {

const char* point_status_text(int st);   // points.hip

uint64_t prep_words(uint64_t num_public) { return VK_IC + 24 * (num_public + 1); }

// ------------------------------------------------------------- kernels ---
// c ? a : b, word by word
ZK_DI XYZZ<FqC> prep_select(bool c, const XYZZ<FqC>& a, const XYZZ<FqC>& b) {
  XYZZ<FqC> o;
  const uint32_t* pa = reinterpret_cast<const uint32_t*>(&a);
  const uint32_t* pb = reinterpret_cast<const uint32_t*>(&b);
  uint32_t* po = reinterpret_cast<uint32_t*>(&o);
#pragma unroll
  for (int k = 0; k < (int)(sizeof(XYZZ<FqC>) / 4); k++) po[k] = c ? pa[k] : pb[k];
  return o;
}

// The table of nb bases, before normalisation: lane (k, w) writes
// out[(k W + w) E + j - 1] = [j 2^(b w)] base[k], j = 1 .. E = 2^b - 1.  The
// base is doubled b w times (every lane runs the top window's b (W - 1) steps
// and keeps its value once its own are done), then added to itself E - 1 times
// from its slot in memory; the first of those additions is a doubling, which
// gn_add_mem handles.  An identity base gives identity entries.
__global__ void __launch_bounds__(GN_BLOCK) k_prep_table(const G1A* __restrict__ base, uint64_t nb, int b, int W,
                                                         G1X* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * GN_BLOCK + threadIdx.x;
  if (t >= nb * (uint64_t)W) return;
  const uint64_t k = t / (uint64_t)W;
  const int w = (int)(t % (uint64_t)W);
  const uint32_t E = (1u << b) - 1;
  G1X* slot = out + t * E;
  Affine<FqC> P;
  XYZZ<FqC> acc;
  xyzz_set_inf(acc);
  if (gn_fetch_aff<FqC>(&base[k], P)) acc = xyzz_from_aff(P);
  const int mine = b * w, steps = b * (W - 1);
#pragma unroll 1
  for (int s = 0; s < steps; s++) acc = prep_select(s < mine, xyzz_dbl(acc), acc);
  gn_store<FqC>(&slot[0], acc);
#pragma unroll 1
  for (uint32_t j = 1; j < E; j++) {
    acc = gn_add_mem<FqC>(acc, &slot[0]);
    gn_store<FqC>(&slot[j], acc);
  }
}

// First level of the sums: lane (i, q) adds terms [q L, (q + 1) L) of proof i,
// term t = (input t / W, window t % W), into part[i R + q]; run 0 starts from
// ic[0] and says whether every input of the row is below r (SOUND; reference
// mode reads lo64 only and accepts every row).  T = npub W > 0 terms.
template <bool SOUND>
__global__ void __launch_bounds__(GN_BLOCK) k_prep_runs(const uint64_t* __restrict__ inputs, uint64_t npub,
                                                        const G1A* __restrict__ ic0, const G1A* __restrict__ table,
                                                        int b, int W, uint32_t L, uint32_t R, uint64_t m,
                                                        G1X* __restrict__ part, uint8_t* __restrict__ ok) {
  const uint64_t id = (uint64_t)blockIdx.x * GN_BLOCK + threadIdx.x;
  if (id >= m * R) return;
  const uint64_t i = id / R;
  const uint32_t q = (uint32_t)(id % R);
  const uint64_t* row = inputs + 4 * npub * i;
  const uint32_t T = (uint32_t)npub * (uint32_t)W, E = (1u << b) - 1;
  XYZZ<FqC> acc;
  xyzz_set_inf(acc);
  if (q == 0) {
    Affine<FqC> P;
    if (gn_fetch_aff<FqC>(ic0, P)) acc = xyzz_from_aff(P);
    bool good = true;
    if constexpr (SOUND) {
#pragma unroll 1
      for (uint64_t k = 0; k < npub; k++) good = pr_fr_reduced(row + 4 * k) && good;
    }
    ok[i] = good ? 1 : 0;
  }
#pragma unroll 1
  for (uint32_t j = 0; j < L; j++) {
    const uint32_t t = q * L + j;
    const bool live = t < T;
    const uint32_t tt = live ? t : 0;
    const uint32_t k = tt / (uint32_t)W, w = tt % (uint32_t)W;
    const uint32_t bit = w * (uint32_t)b;
    const uint32_t d = (uint32_t)(row[4 * (uint64_t)k + (bit >> 6)] >> (bit & 63)) & E;
    Affine<FqC> e;
    const bool finite = gn_fetch_aff<FqC>(&table[(uint64_t)tt * E + (d ? d - 1 : 0)], e);
    acc = prep_select(live && d != 0 && finite, xyzz_madd(acc, e), acc);
  }
  gn_store<FqC>(&part[id], acc);
}
// second level: sum[i] = part[i R] + .. + part[i R + R - 1]
__global__ void __launch_bounds__(GN_BLOCK) k_prep_fold(const G1X* __restrict__ part, uint32_t R, uint64_t m,
                                                        G1X* __restrict__ sum) {
  const uint64_t i = (uint64_t)blockIdx.x * GN_BLOCK + threadIdx.x;
  if (i >= m) return;
  XYZZ<FqC> acc = gn_fetch<FqC>(&part[i * R]);
#pragma unroll 1
  for (uint32_t q = 1; q < R; q++) acc = gn_add_mem<FqC>(acc, &part[i * R + q]);
  gn_store<FqC>(&sum[i], acc);
}

// ------------------------------------------------------------- drivers ---
void prepared_sums_launch(zk_ctx* ctx, hipStream_t st, const zk_vk_dev* pvk, const uint64_t* d_in, size_t m,
                          PrepWork& w) {
  if (!m) return;
  const uint64_t np = pvk->num_public, T = np * (uint64_t)pvk->windows;
  uint64_t L = ctx->prep_run ? ctx->prep_run : prep_run_len(m, np, pvk->windows);
  L = std::min<uint64_t>(std::max<uint64_t>(L, 1), std::max<uint64_t>(T, 1));
  const uint64_t R = T ? (T + L - 1) / L : 1;
  const G1A* ic0 = reinterpret_cast<const G1A*>(pvk->words.as<uint32_t>() + VK_IC);
  w.part.ensure(sizeof(G1X) * m * R);
  w.pre.ensure(sizeof(Fq) * m);
  w.ic.ensure(sizeof(G1A) * m);
  w.ok.ensure(m);
  const int pi = ctx->prof.begin(st, "prepare_inputs", m * T);
  const uint32_t blocks = ceil_div(m * R, GN_BLOCK), Lk = T ? (uint32_t)L : 0;
  if (pvk->sound)
    k_prep_runs<true><<<blocks, GN_BLOCK, 0, st>>>(d_in, np, ic0, pvk->table.as<G1A>(), pvk->width, pvk->windows, Lk,
                                                   (uint32_t)R, m, w.part.as<G1X>(), w.ok.as<uint8_t>());
  else
    k_prep_runs<false><<<blocks, GN_BLOCK, 0, st>>>(d_in, np, ic0, pvk->table.as<G1A>(), pvk->width, pvk->windows, Lk,
                                                    (uint32_t)R, m, w.part.as<G1X>(), w.ok.as<uint8_t>());
  ZK_LAUNCH_CHECK();
  const G1X* src = w.part.as<G1X>();
  if (R > 1) {
    w.sum.ensure(sizeof(G1X) * m);
    k_prep_fold<<<ceil_div(m, GN_BLOCK), GN_BLOCK, 0, st>>>(w.part.as<G1X>(), (uint32_t)R, m, w.sum.as<G1X>());
    ZK_LAUNCH_CHECK();
    src = w.sum.as<G1X>();
  }
  batch_normalize<G1>(src, m, w.pre.as<Fq>(), w.ic.as<G1A>(), st);
  ctx->prof.end(st, pi);
}

static int prepare_inputs_run(zk_ctx* ctx, const zk_vk_dev* pvk, const zk_fr* inputs, size_t n_inputs, size_t n,
                              zk_g1_affine* ic, uint8_t* ok) {
  if (n_inputs != pvk->num_public) return ZK_ERR_INVALID_WITNESS;
  if (pvk->device != ctx->device) {
    ctx->err = "prepared verification key: made on another device";
    return ZK_ERR_ARG;
  }
  if (!n) return ZK_OK;
  hipStream_t st = ctx->stream;
  const size_t chunk = std::min<size_t>(ctx->verify_chunk, n), in_sz = sizeof(zk_fr) * n_inputs;
  DevBuf d_in, d_abi;
  PrepWork w;
  d_in.ensure(std::max<size_t>(in_sz * chunk, 16));
  d_abi.ensure(sizeof(zk_g1_affine) * chunk);
  std::vector<uint8_t> good(chunk);
  for (size_t lo = 0; lo < n; lo += chunk) {
    const size_t m = std::min(chunk, n - lo);
    if (in_sz) ZK_HIP(hipMemcpyAsync(d_in.p, inputs + n_inputs * lo, in_sz * m, hipMemcpyHostToDevice, st));
    prepared_sums_launch(ctx, st, pvk, d_in.as<uint64_t>(), m, w);
    gn_points_to_abi<FqC>(w.ic.as<G1A>(), m, d_abi.as<uint64_t>(), st);
    ZK_HIP(hipMemcpyAsync(ic + lo, d_abi.p, sizeof(zk_g1_affine) * m, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipMemcpyAsync(good.data(), w.ok.p, m, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));   // the next chunk reuses the buffers
    for (size_t j = 0; j < m; j++)
      if (!good[j]) std::memset(ic + lo + j, 0, sizeof(zk_g1_affine));
    if (ok) std::memcpy(ok + lo, good.data(), m);
  }
  if (ctx->prof.on) ctx->prof.collect();
  return ZK_OK;
}

// n points of the key through the point validation (canonical, on the curve,
// in the subgroup; the identity passes).  false with zk_last_error naming the
// point; rc: ZK_ERR_ARG then, or the call's own failure.
template <class P>
static bool vk_points_valid(zk_ctx* ctx, const char* name, const P* pts, size_t n, bool indexed, int& rc) {
  std::vector<uint8_t> st(n);
  size_t bad = n;
  if constexpr (sizeof(P) == sizeof(zk_g1_affine)) rc = zk_g1_validate(ctx, pts, n, st.data(), &bad);
  else rc = zk_g2_validate(ctx, pts, n, st.data(), &bad);
  if (rc == ZK_OK) return true;
  if (rc == ZK_ERR_ARG && bad < n)
    ctx->err = std::string("verification key: ") + name + (indexed ? "[" + std::to_string(bad) + "]" : std::string()) +
               ": " + point_status_text(st[bad]);
  return false;
}

static int vk_prepare(zk_ctx* ctx, const zk_vk* vk, bool sound, zk_vk_dev** out) {
  const uint64_t np = vk->num_public;
  if (!vk->ic_g1 || vk->ic_len < np + 1) {
    ctx->err = "verification key: ic_g1 shorter than the public inputs";
    return ZK_ERR_ARG;
  }
  int rc = ZK_OK;
  if (!vk_points_valid(ctx, "alpha_g1", &vk->alpha_g1, 1, false, rc) ||
      !vk_points_valid(ctx, "beta_g2", &vk->beta_g2, 1, false, rc) ||
      !vk_points_valid(ctx, "gamma_g2", &vk->gamma_g2, 1, false, rc) ||
      !vk_points_valid(ctx, "delta_g2", &vk->delta_g2, 1, false, rc) ||
      !vk_points_valid(ctx, "ic_g1", vk->ic_g1, vk->ic_len, true, rc))
    return rc;
  const int b = ctx->prep_width ? ctx->prep_width : prep_width(sound, np);
  if (!b || prep_table_bytes(sound, np, b) > PREP_TABLE_MAX) {
    ctx->err = "verification key: too many public inputs for a prepared key's window table";
    return ZK_ERR_ARG;
  }
  std::vector<uint32_t> words;
  if (!pairing_tables(*vk, np, words)) {
    ctx->err = "verification key: a point is not canonical or not on its curve";
    return ZK_ERR_ARG;
  }
  hipStream_t st = ctx->stream;
  std::unique_ptr<zk_vk_dev> k(new zk_vk_dev);
  k->device = ctx->device;
  k->sound = sound;
  k->num_public = np;
  k->width = b;
  k->windows = prep_windows(sound, b);
  k->bytes = 4 * words.size() + prep_table_bytes(sound, np, b);
  k->words.ensure(4 * words.size());
  ZK_HIP(hipMemcpyAsync(k->words.p, words.data(), 4 * words.size(), hipMemcpyHostToDevice, st));
  if (np) {
    // in passes of as many bases as PREP_BUILD_MAX lets wait for their normalisation
    const uint64_t per = (uint64_t)k->windows * ((1ull << b) - 1);
    const uint64_t fit = PREP_BUILD_MAX / (per * (sizeof(G1X) + sizeof(Fq)));
    const uint64_t pass = std::min<uint64_t>(np, std::max<uint64_t>(fit, 1));
    DevBuf d_x, d_pre;
    k->table.ensure(sizeof(G1A) * per * np);
    d_x.ensure(sizeof(G1X) * per * pass);
    d_pre.ensure(sizeof(Fq) * per * pass);
    const G1A* base = reinterpret_cast<const G1A*>(k->words.as<uint32_t>() + VK_IC) + 1;
    const int pi = ctx->prof.begin(st, "vk_prepare_table", per * np);
    for (uint64_t k0 = 0; k0 < np; k0 += pass) {
      const uint64_t nb = std::min(pass, np - k0);
      k_prep_table<<<ceil_div(nb * k->windows, GN_BLOCK), GN_BLOCK, 0, st>>>(base + k0, nb, b, k->windows,
                                                                             d_x.as<G1X>());
      ZK_LAUNCH_CHECK();
      batch_normalize<G1>(d_x.as<G1X>(), nb * per, d_pre.as<Fq>(), k->table.as<G1A>() + k0 * per, st);
    }
    ctx->prof.end(st, pi);
  }
  ZK_HIP(hipStreamSynchronize(st));   // the host words and the build's buffers die here
  if (ctx->prof.on) ctx->prof.collect();
  *out = k.release();
  return ZK_OK;
}

}  // namespace zk

using namespace zk;

#define ZK_VGUARD(ctx, ...)                                   \
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

int zk_vk_prepare(zk_ctx* ctx, const zk_vk* vk, int sound, zk_vk_dev** out) {
  if (!ctx || !vk || !out) return ZK_ERR_ARG;
  *out = nullptr;
  ZK_VGUARD(ctx, { return vk_prepare(ctx, vk, sound != 0, out); })
}
void zk_vk_dev_free(zk_vk_dev* pvk) {
  if (!pvk) return;
  (void)hipSetDevice(pvk->device);
  delete pvk;
}
int zk_vk_dev_bytes(const zk_vk_dev* pvk, uint64_t* bytes) {
  if (!pvk || !bytes) return ZK_ERR_ARG;
  *bytes = pvk->bytes;
  return ZK_OK;
}
int zk_vk_dev_is_sound(const zk_vk_dev* pvk) { return pvk && pvk->sound ? 1 : 0; }

int zk_groth16_prepare_inputs(zk_ctx* ctx, const zk_vk_dev* pvk, const zk_fr* public_inputs, size_t n_inputs,
                              size_t n, zk_g1_affine* ic, uint8_t* ok) {
  if (!ctx || !pvk || (n && (!ic || (n_inputs && !public_inputs)))) return ZK_ERR_ARG;
  ZK_VGUARD(ctx, { return prepare_inputs_run(ctx, pvk, public_inputs, n_inputs, n, ic, ok); })
}
