// digest.hip -- the V2 tree digests of a powers-of-tau string and of a sound
// key (include/zkp.h, "tree digests"): leaves of 256 points
// hashed one lane per leaf on the GPU (digest.hpp), a host twin of the same
// definition over zk_g1_compress / zk_g2_compress and Sha256, and the short
// host hash over the leaf digests.  The V1 digests stay in hash.hip.  No
// reference counterpart.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "digest.hpp"

namespace zk {

__global__ void __launch_bounds__(DG_BLOCK) k_g1_leaf_digest(const uint64_t* __restrict__ pts, size_t n,
                                                             uint8_t* __restrict__ out) {
  const size_t leaf = (size_t)blockIdx.x * DG_BLOCK + threadIdx.x;
  if (DIGEST_LEAF * leaf < n) dg_leaf_lane<1>(pts, n, leaf, out);
}
__global__ void __launch_bounds__(DG_BLOCK) k_g2_leaf_digest(const uint64_t* __restrict__ pts, size_t n,
                                                             uint8_t* __restrict__ out) {
  const size_t leaf = (size_t)blockIdx.x * DG_BLOCK + threadIdx.x;
  if (DIGEST_LEAF * leaf < n) dg_leaf_lane<2>(pts, n, leaf, out);
}

static size_t leaf_count(size_t n) { return (n + DIGEST_LEAF - 1) / DIGEST_LEAF; }

// The chunk loop of points_run (points.hip) with chunks of whole leaves:
// ctx->point_chunk rounded down to a multiple of 256, at least 256, so a
// chunk's first point starts a leaf (and lies on a 16-byte boundary of the
// device buffer).  32 bytes per leaf come back.
int leaf_digests_run(zk_ctx* ctx, bool g2, const void* pts, size_t n, uint8_t* out) {
  if (!n) return ZK_OK;
  const size_t sz = g2 ? sizeof(zk_g2_affine) : sizeof(zk_g1_affine);
  hipStream_t st = ctx->stream;
  const size_t whole = std::max<size_t>(ctx->point_chunk / DIGEST_LEAF * DIGEST_LEAF, DIGEST_LEAF);
  const size_t chunk = std::min(whole, leaf_count(n) * DIGEST_LEAF);
  DevBuf d_in, d_out;
  d_in.ensure(sz * std::min(chunk, n));
  d_out.ensure(32 * leaf_count(chunk));
  for (size_t lo = 0; lo < n; lo += chunk) {
    const size_t m = std::min(chunk, n - lo), leaves = leaf_count(m);
    int pi = ctx->prof.begin(st, "leaf_upload", sz * m);
    ZK_HIP(hipMemcpyAsync(d_in.p, static_cast<const uint8_t*>(pts) + sz * lo, sz * m, hipMemcpyHostToDevice, st));
    ctx->prof.end(st, pi);
    pi = ctx->prof.begin(st, g2 ? "leaf_digest_g2" : "leaf_digest_g1", m);
    if (g2) k_g2_leaf_digest<<<ceil_div(leaves, DG_BLOCK), DG_BLOCK, 0, st>>>(d_in.as<uint64_t>(), m, d_out.as<uint8_t>());
    else k_g1_leaf_digest<<<ceil_div(leaves, DG_BLOCK), DG_BLOCK, 0, st>>>(d_in.as<uint64_t>(), m, d_out.as<uint8_t>());
    ZK_LAUNCH_CHECK();
    ctx->prof.end(st, pi);
    ZK_HIP(hipMemcpyAsync(out + 32 * (lo / DIGEST_LEAF), d_out.p, 32 * leaves, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));   // the next chunk reuses the buffers
  }
  if (ctx->prof.on) ctx->prof.collect();
  return ZK_OK;
}

// ---- host twin: the definition in plain C++ ------------------------------------------
void leaf_digests_host(bool g2, const void* pts, size_t n, uint8_t* out) {
  const size_t enc = g2 ? 96 : 48;
  std::vector<uint8_t> buf(enc * DIGEST_LEAF);
  for (size_t lo = 0; lo < n; lo += DIGEST_LEAF) {
    const size_t m = std::min(DIGEST_LEAF, n - lo);
    uint8_t b0[64] = {};
    std::memcpy(b0, DG_TAG, DG_TAG_LEN);
    b0[13] = g2 ? 2 : 1;
    b0[14] = (uint8_t)(m >> 8);
    b0[15] = (uint8_t)m;
    if (g2) zk_g2_compress(static_cast<const zk_g2_affine*>(pts) + lo, m, buf.data());
    else zk_g1_compress(static_cast<const zk_g1_affine*>(pts) + lo, m, buf.data());
    Sha256 h;
    h.update(b0, 64);
    h.update(buf.data(), enc * m);
    h.final(out + 32 * (lo / DIGEST_LEAF));
  }
}

static int leaf_digests_any(zk_ctx* ctx, bool g2, const void* pts, size_t n, uint8_t* out) {
  if (ctx) return leaf_digests_run(ctx, g2, pts, n, out);
  leaf_digests_host(g2, pts, n, out);
  return ZK_OK;
}

// The top hash of a V2 digest: header and single points straight into it, an
// array as its leaf digests (GPU with a ctx, host twin without).
struct TopHash {
  zk_ctx* ctx;
  Sha256 h;
  std::vector<uint8_t> buf;
  double host_ms = 0;
  void point(const zk_g1_affine& p) {
    uint8_t e[48];
    zk_g1_compress(&p, 1, e);
    h.update(e, 48);
  }
  void point(const zk_g2_affine& p) {
    uint8_t e[96];
    zk_g2_compress(&p, 1, e);
    h.update(e, 96);
  }
  void leaves(bool g2, const void* arr, size_t n) {
    buf.resize(32 * leaf_count(n));
    leaf_digests_any(ctx, g2, arr, n, buf.data());
    const auto t0 = std::chrono::steady_clock::now();
    h.update(buf.data(), buf.size());
    host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  void final(uint8_t out[32]) {
    h.final(out);
    if (ctx) ctx->prof.add_host("digest_top_hash", host_ms);
  }
};

static void srs_digest_v2(zk_ctx* ctx, const zk_srs* srs, uint8_t out[32]) {
  TopHash t{ctx};
  t.h.update("ZKAMD-SRS-V2", 12);
  t.h.update_u64be(srs->log_n);
  t.h.update_u64be(srs->tau_g1_len);
  t.h.update_u64be(srs->tau_g2_len);
  t.h.update_u64be(srs->alpha_len);
  t.h.update_u64be(srs->beta_len);
  t.point(srs->beta_g2);
  t.leaves(false, srs->tau_g1, srs->tau_g1_len);
  t.leaves(true, srs->tau_g2, srs->tau_g2_len);
  t.leaves(false, srs->alpha_tau_g1, srs->alpha_len);
  t.leaves(false, srs->beta_tau_g1, srs->beta_len);
  t.final(out);
}

static void key_digest_v2(zk_ctx* ctx, const zk_pk* pk, const zk_vk* vk, uint8_t out[32]) {
  TopHash t{ctx};
  t.h.update("ZKAMD-KEY-V2", 12);
  t.h.update_u64be(pk->a_len);
  t.h.update_u64be(pk->b_len);
  t.h.update_u64be(pk->b2_len);
  t.h.update_u64be(pk->ic_len);
  t.h.update_u64be(pk->h_len);
  t.h.update_u64be(pk->num_public);
  t.h.update_u64be(vk->ic_len);
  t.point(pk->alpha_g1);
  t.point(pk->beta_g1);
  t.point(pk->delta_g1);
  t.point(pk->beta_g2);
  t.point(pk->delta_g2);
  t.point(vk->gamma_g2);
  t.leaves(false, pk->a_g1, pk->a_len);
  t.leaves(false, pk->b_g1, pk->b_len);
  t.leaves(true, pk->b_g2, pk->b2_len);
  t.leaves(false, pk->ic_g1, pk->ic_len);
  t.leaves(false, pk->h_g1, pk->h_len);
  t.leaves(false, vk->ic_g1, vk->ic_len);
  t.final(out);
}

}  // namespace zk

using namespace zk;

// ctx == NULL: the host twin, nothing to guard
#define ZK_DGUARD(ctx, ...)                                   \
  if (!(ctx)) {                                               \
    __VA_ARGS__                                               \
  }                                                           \
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

int zk_g1_leaf_digests(zk_ctx* ctx, const zk_g1_affine* pts, size_t n, uint8_t* out) {
  if (n && (!pts || !out)) return ZK_ERR_ARG;
  ZK_DGUARD(ctx, { return leaf_digests_any(ctx, false, pts, n, out); })
}

int zk_g2_leaf_digests(zk_ctx* ctx, const zk_g2_affine* pts, size_t n, uint8_t* out) {
  if (n && (!pts || !out)) return ZK_ERR_ARG;
  ZK_DGUARD(ctx, { return leaf_digests_any(ctx, true, pts, n, out); })
}

int zk_srs_digest_v2(zk_ctx* ctx, const zk_srs* srs, uint8_t out[32]) {
  if (!srs || !out) return ZK_ERR_ARG;
  if ((srs->tau_g1_len && !srs->tau_g1) || (srs->tau_g2_len && !srs->tau_g2) || (srs->alpha_len && !srs->alpha_tau_g1) ||
      (srs->beta_len && !srs->beta_tau_g1))
    return ZK_ERR_ARG;
  ZK_DGUARD(ctx, {
    srs_digest_v2(ctx, srs, out);
    return ZK_OK;
  })
}

int zk_groth16_key_digest_v2_sound(zk_ctx* ctx, const zk_pk* pk, const zk_vk* vk, uint8_t out[32]) {
  if (!pk || !vk || !out) return ZK_ERR_ARG;
  if ((pk->a_len && !pk->a_g1) || (pk->b_len && !pk->b_g1) || (pk->b2_len && !pk->b_g2) ||
      (pk->ic_len && !pk->ic_g1) || (pk->h_len && !pk->h_g1) || (vk->ic_len && !vk->ic_g1))
    return ZK_ERR_ARG;
  ZK_DGUARD(ctx, {
    key_digest_v2(ctx, pk, vk, out);
    return ZK_OK;
  })
}
