// hash.hip -- the hash to G2 and what a ceremony's transcript builds on it
// (include/zkp.h, "proofs of knowledge"): the hash for a batch
// of messages on the GPU, one lane per message (hash.hpp), its host twin,
// SHA-256 digests of a string and of a key, Schnorr-style proofs of knowledge
// of a share in the pairing setting (Bowe, Gabizon, Miers) and their batch
// check -- validation, hash and pairing product in one device pass.  No
// reference counterpart.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.hpp"
#include "hash.hpp"
#include "host_pairing.hpp"

namespace zk {

constexpr size_t G1W = sizeof(zk_g1_affine) / 8, G2W = sizeof(zk_g2_affine) / 8;
static_assert(G1W == 13 && G2W == 25, "ABI point sizes");
constexpr size_t POK_MSG = 32 + 48 + 1;   // challenge | compress(s_g1) | byte(role)
static const char POK_DST[] = "ZKAMD-POK-V1";
constexpr size_t POK_DST_LEN = sizeof(POK_DST) - 1;

// One lane per message.  Every lane of the last wave stays active (the try
// loop leaves on a ballot): a lane past the end hashes the last message and
// stores nothing.  out: message i's 25 words at out + out_stride i.
__global__ void __launch_bounds__(PT_BLOCK) k_hash_to_g2(const uint8_t* __restrict__ msgs, size_t n, size_t msg_len,
                                                         const uint8_t* __restrict__ dst, uint32_t dst_len,
                                                         uint32_t max_tries, uint64_t* __restrict__ out,
                                                         size_t out_stride, uint8_t* __restrict__ tries) {
  const size_t gid = (size_t)blockIdx.x * PT_BLOCK + threadIdx.x;
  const size_t i = gid < n ? gid : n - 1;
  h2_hash_lane(msgs + msg_len * i, msg_len, dst, dst_len, max_tries, gid < n, out + out_stride * i, tries + i);
}

// The pairs of the products that check m proofs of knowledge, from what the
// stages before left in device memory: per proof
//   product 0: (s_g1, R), (-g1, s_r)
//   product 1 (link != NULL): (s_g1, g2), (-g1, link)
// cst: -g1 (13 words), then the G2 generator (25 words).
__global__ void __launch_bounds__(PT_BLOCK) k_pok_pairs(const uint64_t* __restrict__ s_g1, const uint64_t* __restrict__ s_r,
                                                        const uint64_t* __restrict__ R, const uint64_t* __restrict__ link,
                                                        const uint64_t* __restrict__ cst, size_t m,
                                                        uint64_t* __restrict__ g1, uint64_t* __restrict__ g2) {
  const size_t i = (size_t)blockIdx.x * PT_BLOCK + threadIdx.x;
  if (i >= m) return;
  const size_t per = link ? 2 : 1;
  for (size_t q = 0; q < per; q++) {
    const size_t j = per * i + q;
    uint64_t* a = g1 + 2 * G1W * j;
    uint64_t* b = g2 + 2 * G2W * j;
    const uint64_t* q0 = q == 0 ? R + G2W * i : cst + G1W;
    const uint64_t* q1 = q == 0 ? s_r + G2W * i : link + G2W * i;
    for (size_t w = 0; w < G1W; w++) {
      a[w] = s_g1[G1W * i + w];
      a[G1W + w] = cst[w];
    }
    for (size_t w = 0; w < G2W; w++) {
      b[w] = q0[w];
      b[G2W + w] = q1[w];
    }
  }
}

static void hash_to_g2_launch(zk_ctx* ctx, hipStream_t st, const uint8_t* d_msgs, size_t m, size_t msg_len,
                              const uint8_t* d_dst, size_t dst_len, uint32_t max_tries, uint64_t* d_out,
                              uint8_t* d_tries) {
  if (!m) return;
  const int pi = ctx->prof.begin(st, "hash_to_g2", m);
  k_hash_to_g2<<<ceil_div(m, PT_BLOCK), PT_BLOCK, 0, st>>>(d_msgs, m, msg_len, d_dst, (uint32_t)dst_len, max_tries,
                                                           d_out, G2W, d_tries);
  ZK_LAUNCH_CHECK();
  ctx->prof.end(st, pi);
}

int hash_to_g2_run(zk_ctx* ctx, const uint8_t* msgs, size_t n, size_t msg_len, const uint8_t* dst, size_t dst_len,
                   uint32_t max_tries, zk_g2_affine* out, uint8_t* tries) {
  if (!n) return ZK_OK;
  hipStream_t st = ctx->stream;
  const size_t chunk = std::min<size_t>(ctx->point_chunk, n);
  DevBuf d_msgs, d_dst, d_out, d_tr;
  d_msgs.ensure(std::max<size_t>(msg_len * chunk, 16));
  d_dst.ensure(std::max<size_t>(dst_len, 16));
  d_out.ensure(sizeof(zk_g2_affine) * chunk);
  d_tr.ensure(chunk);
  if (dst_len) ZK_HIP(hipMemcpyAsync(d_dst.p, dst, dst_len, hipMemcpyHostToDevice, st));
  for (size_t lo = 0; lo < n; lo += chunk) {
    const size_t m = std::min(chunk, n - lo);
    if (msg_len) ZK_HIP(hipMemcpyAsync(d_msgs.p, msgs + msg_len * lo, msg_len * m, hipMemcpyHostToDevice, st));
    hash_to_g2_launch(ctx, st, d_msgs.as<uint8_t>(), m, msg_len, d_dst.as<uint8_t>(), dst_len, max_tries,
                      d_out.as<uint64_t>(), d_tr.as<uint8_t>());
    ZK_HIP(hipMemcpyAsync(out + lo, d_out.p, sizeof(zk_g2_affine) * m, hipMemcpyDeviceToHost, st));
    if (tries) ZK_HIP(hipMemcpyAsync(tries + lo, d_tr.p, m, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));   // the next chunk reuses the buffers
  }
  if (ctx->prof.on) ctx->prof.collect();
  return ZK_OK;
}

// ---- host twin ---------------------------------------------------------------------
namespace host {

static X<Fq> g1_gen() {
  X<Fq> p{{}, {}, one(), one()};
  std::memcpy(p.X_.l, G1_GEN_HOSTM, 48);
  std::memcpy(p.Y.l, G1_GEN_HOSTM + 12, 48);
  return p;
}
static X<Fq2> g2_gen() {
  X<Fq2> p{{}, {}, f_one<Fq2>(), f_one<Fq2>()};
  std::memcpy(p.X_.c0.l, G2_GEN_HOSTM, 48);
  std::memcpy(p.X_.c1.l, G2_GEN_HOSTM + 12, 48);
  std::memcpy(p.Y.c0.l, G2_GEN_HOSTM + 24, 48);
  std::memcpy(p.Y.c1.l, G2_GEN_HOSTM + 36, 48);
  return p;
}
// 32 big-endian bytes -> a canonical value below 2^256 < p
static Fq fq_of_digest(const uint8_t* d) {
  Fq c{};
  for (int i = 0; i < 32; i++) c.l[(31 - i) / 8] |= (uint64_t)d[i] << (8 * ((31 - i) % 8));
  return c;
}
static void digest_of(const uint8_t m0[32], unsigned ctr, unsigned j, uint8_t out[32]) {
  Sha256 h;
  const uint8_t tail[2] = {(uint8_t)ctr, (uint8_t)j};
  h.update(m0, 32);
  h.update(tail, 2);
  h.final(out);
}
// int_be(d_a | d_b) mod p, Montgomery form
static Fq fq_of_pair(const uint8_t m0[32], unsigned ctr, unsigned ja) {
  uint8_t d[32];
  Fq two256{};
  two256.l[4] = 1;
  digest_of(m0, ctr, ja, d);
  const Fq hi = to_mont(fq_of_digest(d));
  digest_of(m0, ctr, ja + 1, d);
  return add(mul(hi, to_mont(two256)), to_mont(fq_of_digest(d)));
}
static bool fq2_largest(const Fq2& y) {
  const Fq c0 = from_mont(y.c0), c1 = from_mont(y.c1);
  return is_zero(c1) ? fq_canonical_largest(c0.l) : fq_canonical_largest(c1.l);
}
static X<Fq2> psi(const X<Fq2>& p) {
  const Fq2 kx = {to_host(fq_const(ENDO_PSI_X32[0])), to_host(fq_const(ENDO_PSI_X32[1]))};
  const Fq2 ky = {to_host(fq_const(ENDO_PSI_Y32[0])), to_host(fq_const(ENDO_PSI_Y32[1]))};
  return {mul(conj(p.X_), kx), mul(conj(p.Y), ky), conj(p.ZZ), conj(p.ZZZ)};
}
static X<Fq2> negx(X<Fq2> p) {
  p.Y = neg(p.Y);
  return p;
}
// [x^2 - x - 1] P + [x - 1] psi(P) + psi^2([2] P), x = -BLS_X_ABS
static X<Fq2> clear_cofactor(const X<Fq2>& P) {
  const uint64_t k[4] = {BLS_X_ABS, 0, 0, 0};
  const X<Fq2> t1 = mul_scalar(P, k), t2 = mul_scalar(t1, k);
  const X<Fq2> a = addp(addp(t2, t1), negx(P));
  const X<Fq2> b = negx(psi(addp(t1, P)));
  return addp(addp(a, b), psi(psi(dbl(P))));
}
// false: no point after H2_MAX_TRIES tries
static bool hash_to_g2(const uint8_t* msg, size_t msg_len, const uint8_t* dst, size_t dst_len, X<Fq2>& Q,
                       uint8_t& tries) {
  uint8_t m0[32];
  {
    Sha256 h;
    const uint8_t len = (uint8_t)dst_len;
    h.update(H2_TAG, H2_TAG_LEN);
    h.update(&len, 1);
    h.update(dst, dst_len);
    h.update(msg, msg_len);
    h.final(m0);
  }
  for (unsigned ctr = 0; ctr < H2_MAX_TRIES; ctr++) {
    const Fq2 x = {fq_of_pair(m0, ctr, 0), fq_of_pair(m0, ctr, 2)};
    const Fq2 t = add(mul(sqr(x), x), g2_b());
    Fq2 y;
    if (is_zero(t) || !sqrt_fq2(t, y)) continue;
    uint8_t d4[32];
    digest_of(m0, ctr, 4, d4);
    if (fq2_largest(y) != ((d4[31] & 1) != 0)) y = neg(y);
    Q = clear_cofactor(from_affine(x, y, false));
    if (is_inf(Q)) continue;
    tries = (uint8_t)ctr;
    return true;
  }
  return false;
}

}  // namespace host

static bool fr_share_ok(const zk_fr& a) {
  if (!(a.l[0] | a.l[1] | a.l[2] | a.l[3])) return false;
  for (int i = 3; i >= 0; i--)
    if (a.l[i] != FR_MOD64[i]) return a.l[i] < FR_MOD64[i];
  return false;
}
static void pok_message(const uint8_t challenge[32], const zk_g1_affine& s_g1, uint8_t role, uint8_t* msg) {
  std::memcpy(msg, challenge, 32);
  serialize_g1_compressed(s_g1, msg + 32);
  msg[80] = role;
}
// a proof's point as the checks want it: canonical, on its curve, in the
// subgroup, not the identity
template <class A, class P>
static bool pok_point(const A& abi, P& p) {
  return host::load(abi, p) && !p.inf && host::in_subgroup(p);
}

static int pok_verify_host(const zk_pok* pok, uint8_t role, const uint8_t challenge[32], int* status) {
  host::A1 s1, g1n;
  host::A2 sr, R;
  *status = ZK_POK_POINT;
  if (!pok_point(pok->s_g1, s1) || !pok_point(pok->s_r, sr)) return ZK_OK;
  uint8_t msg[POK_MSG], tries;
  pok_message(challenge, pok->s_g1, role, msg);
  host::X<host::Fq2> Rx;
  *status = ZK_POK_HASH;
  if (!host::hash_to_g2(msg, POK_MSG, reinterpret_cast<const uint8_t*>(POK_DST), POK_DST_LEN, Rx, tries)) return ZK_OK;
  R.inf = !host::to_affine(Rx, R.x, R.y);
  const host::X<host::Fq> g = host::g1_gen();
  g1n = {g.X_, host::neg(g.Y), false};
  *status = host::pairing_product_is_one({s1, g1n}, {R, sr}) ? ZK_POK_OK : ZK_POK_REJECT;
  return ZK_OK;
}

// n proofs through the GPU in chunks of ctx->verify_chunk: the proofs' points
// are validated by zk_g1_validate / zk_g2_validate's kernels, the challenges
// hashed to R by k_hash_to_g2 into device memory, and the products taken by
// zk_pairing_products' kernel from pairs that k_pok_pairs puts together there:
// R never visits the host.  links (may be NULL): per proof a G2 point whose
// product e(s_g1, g2) e(-g1, link) must be 1 as well.
static int pok_verify_many_run(zk_ctx* ctx, const zk_pok* poks, const uint8_t* roles, const uint8_t* challenges,
                               const zk_g2_affine* links, size_t n, uint8_t* status, size_t* first_bad) {
  if (first_bad) *first_bad = n;
  if (!n) return ZK_OK;
  hipStream_t st = ctx->stream;
  const size_t chunk = std::min<size_t>(ctx->verify_chunk, n), per = links ? 2 : 1;
  DevBuf d_s1, d_sr, d_link, d_msgs, d_dst, d_cst, d_R, d_tr, d_v1, d_v2, d_g1, d_g2, d_pst;
  d_s1.ensure(sizeof(zk_g1_affine) * chunk);
  d_sr.ensure(sizeof(zk_g2_affine) * chunk);
  if (links) d_link.ensure(sizeof(zk_g2_affine) * chunk);
  d_msgs.ensure(POK_MSG * chunk);
  d_dst.ensure(16);
  d_cst.ensure(8 * (G1W + G2W));
  d_R.ensure(sizeof(zk_g2_affine) * chunk);
  d_tr.ensure(chunk);
  d_v1.ensure(chunk);
  d_v2.ensure(chunk);
  d_g1.ensure(sizeof(zk_g1_affine) * 2 * per * chunk);
  d_g2.ensure(sizeof(zk_g2_affine) * 2 * per * chunk);
  d_pst.ensure(per * chunk);
  uint64_t cst[G1W + G2W];
  host::X<host::Fq> g = host::g1_gen();
  g.Y = host::neg(g.Y);
  host_to_abi<G1>(g, cst);
  host_to_abi<G2>(host::g2_gen(), cst + G1W);
  ZK_HIP(hipMemcpyAsync(d_cst.p, cst, sizeof cst, hipMemcpyHostToDevice, st));
  ZK_HIP(hipMemcpyAsync(d_dst.p, POK_DST, POK_DST_LEN, hipMemcpyHostToDevice, st));
  std::vector<zk_g1_affine> s1(chunk);
  std::vector<zk_g2_affine> sr(chunk);
  std::vector<uint8_t> msgs(POK_MSG * chunk), v1(chunk), v2(chunk), tr(chunk), pst(per * chunk);
  for (size_t lo = 0; lo < n; lo += chunk) {
    const size_t m = std::min(chunk, n - lo);
    for (size_t i = 0; i < m; i++) {
      s1[i] = poks[lo + i].s_g1;
      sr[i] = poks[lo + i].s_r;
      pok_message(challenges + 32 * (lo + i), s1[i], roles[lo + i], &msgs[POK_MSG * i]);
    }
    ZK_HIP(hipMemcpyAsync(d_s1.p, s1.data(), sizeof(zk_g1_affine) * m, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_sr.p, sr.data(), sizeof(zk_g2_affine) * m, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_msgs.p, msgs.data(), POK_MSG * m, hipMemcpyHostToDevice, st));
    if (links) ZK_HIP(hipMemcpyAsync(d_link.p, links + lo, sizeof(zk_g2_affine) * m, hipMemcpyHostToDevice, st));
    points_validate_launch(ctx, st, false, d_s1.as<uint64_t>(), m, d_v1.as<uint8_t>());
    points_validate_launch(ctx, st, true, d_sr.as<uint64_t>(), m, d_v2.as<uint8_t>());
    hash_to_g2_launch(ctx, st, d_msgs.as<uint8_t>(), m, POK_MSG, d_dst.as<uint8_t>(), POK_DST_LEN, H2_MAX_TRIES,
                      d_R.as<uint64_t>(), d_tr.as<uint8_t>());
    k_pok_pairs<<<ceil_div(m, PT_BLOCK), PT_BLOCK, 0, st>>>(d_s1.as<uint64_t>(), d_sr.as<uint64_t>(), d_R.as<uint64_t>(),
                                                            links ? d_link.as<uint64_t>() : nullptr,
                                                            d_cst.as<uint64_t>(), m, d_g1.as<uint64_t>(),
                                                            d_g2.as<uint64_t>());
    ZK_LAUNCH_CHECK();
    pairing_products_launch(ctx, st, d_g1.as<uint64_t>(), d_g2.as<uint64_t>(), 2, per * m, d_pst.as<uint8_t>());
    ZK_HIP(hipMemcpyAsync(v1.data(), d_v1.p, m, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipMemcpyAsync(v2.data(), d_v2.p, m, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipMemcpyAsync(tr.data(), d_tr.p, m, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipMemcpyAsync(pst.data(), d_pst.p, per * m, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));   // the next chunk reuses the buffers
    for (size_t i = 0; i < m; i++) {
      uint8_t s = ZK_POK_OK;
      if (v1[i] != ZK_POINT_OK || v2[i] != ZK_POINT_OK || s1[i].infinity || sr[i].infinity) s = ZK_POK_POINT;
      else if (tr[i] == H2_NO_POINT) s = ZK_POK_HASH;
      else
        for (size_t q = 0; q < per; q++)
          if (pst[per * i + q] != ZK_VERIFY_ACCEPT) s = ZK_POK_REJECT;
      status[lo + i] = s;
    }
  }
  if (ctx->prof.on) ctx->prof.collect();
  for (size_t i = 0; i < n; i++)
    if (status[i] != ZK_POK_OK) {
      if (first_bad) *first_bad = i;
      break;
    }
  return ZK_OK;
}

// ---- digests ---------------------------------------------------------------------------
constexpr size_t DIGEST_PIECE = 256;   // points encoded at a time
static void digest_g1(Sha256& h, const zk_g1_affine* p, size_t n) {
  uint8_t buf[48 * DIGEST_PIECE];
  for (size_t lo = 0; lo < n; lo += DIGEST_PIECE) {
    const size_t m = std::min(DIGEST_PIECE, n - lo);
    zk_g1_compress(p + lo, m, buf);
    h.update(buf, 48 * m);
  }
}
static void digest_g2(Sha256& h, const zk_g2_affine* p, size_t n) {
  uint8_t buf[96 * DIGEST_PIECE];
  for (size_t lo = 0; lo < n; lo += DIGEST_PIECE) {
    const size_t m = std::min(DIGEST_PIECE, n - lo);
    zk_g2_compress(p + lo, m, buf);
    h.update(buf, 96 * m);
  }
}

}  // namespace zk

using namespace zk;

#define ZK_HGUARD(ctx, ...)                                   \
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

int zk_sha256(const uint8_t* msg, size_t len, uint8_t out[32]) {
  if (!out || (len && !msg)) return ZK_ERR_ARG;
  Sha256 h;
  h.update(msg, len);
  h.final(out);
  return ZK_OK;
}

int zk_hash_to_g2_host(const uint8_t* msg, size_t msg_len, const uint8_t* dst, size_t dst_len, zk_g2_affine* out,
                       uint8_t* tries) {
  if (!out || (msg_len && !msg) || (dst_len && !dst) || dst_len > 255) return ZK_ERR_ARG;
  std::memset(out, 0, sizeof *out);
  host::X<host::Fq2> Q;
  uint8_t t = H2_NO_POINT;
  const bool ok = host::hash_to_g2(msg, msg_len, dst, dst_len, Q, t);
  if (tries) *tries = ok ? t : H2_NO_POINT;
  if (!ok) return ZK_ERR_ARG;
  host_to_abi<G2>(Q, reinterpret_cast<uint64_t*>(out));
  return ZK_OK;
}

int zk_hash_to_g2(zk_ctx* ctx, const uint8_t* msgs, size_t n, size_t msg_len, const uint8_t* dst, size_t dst_len,
                  zk_g2_affine* out, uint8_t* tries) {
  if (!ctx || (n && (!out || (msg_len && !msgs))) || (dst_len && !dst)) return ZK_ERR_ARG;
  if (dst_len > 255) {
    ctx->err = "hash_to_g2: dst longer than 255 bytes";
    return ZK_ERR_ARG;
  }
  ZK_HGUARD(ctx, { return hash_to_g2_run(ctx, msgs, n, msg_len, dst, dst_len, H2_MAX_TRIES, out, tries); })
}

int zk_pok_make(const zk_fr* s, uint8_t role, const uint8_t challenge[32], zk_pok* out) {
  if (!s || !challenge || !out || role > ZK_POK_DELTA || !fr_share_ok(*s)) return ZK_ERR_ARG;
  std::memset(out, 0, sizeof *out);
  host_to_abi<G1>(host::mul_scalar(host::g1_gen(), s->l), reinterpret_cast<uint64_t*>(&out->s_g1));
  uint8_t msg[POK_MSG], tries;
  pok_message(challenge, out->s_g1, role, msg);
  host::X<host::Fq2> R;
  if (!host::hash_to_g2(msg, POK_MSG, reinterpret_cast<const uint8_t*>(POK_DST), POK_DST_LEN, R, tries))
    return ZK_ERR_ARG;
  host_to_abi<G2>(host::mul_scalar(R, s->l), reinterpret_cast<uint64_t*>(&out->s_r));
  return ZK_OK;
}

int zk_pok_verify(const zk_pok* pok, uint8_t role, const uint8_t challenge[32], int* status) {
  if (!pok || !challenge || !status || role > ZK_POK_DELTA) return ZK_ERR_ARG;
  return pok_verify_host(pok, role, challenge, status);
}

static int pok_roles_ok(zk_ctx* ctx, const uint8_t* roles, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (roles[i] > ZK_POK_DELTA) {
      ctx->err = "pok_verify_many: proof " + std::to_string(i) + " has no role " + std::to_string(roles[i]);
      return ZK_ERR_ARG;
    }
  return ZK_OK;
}

int zk_pok_verify_many(zk_ctx* ctx, const zk_pok* poks, const uint8_t* roles, const uint8_t* challenges, size_t n,
                       uint8_t* status, size_t* first_bad) {
  if (!ctx || (n && (!poks || !roles || !challenges || !status))) return ZK_ERR_ARG;
  if (pok_roles_ok(ctx, roles, n) != ZK_OK) return ZK_ERR_ARG;
  ZK_HGUARD(ctx, { return pok_verify_many_run(ctx, poks, roles, challenges, nullptr, n, status, first_bad); })
}

int zk_srs_digest(const zk_srs* srs, uint8_t out[32]) {
  if (!srs || !out) return ZK_ERR_ARG;
  if ((srs->tau_g1_len && !srs->tau_g1) || (srs->tau_g2_len && !srs->tau_g2) || (srs->alpha_len && !srs->alpha_tau_g1) ||
      (srs->beta_len && !srs->beta_tau_g1))
    return ZK_ERR_ARG;
  Sha256 h;
  h.update("ZKAMD-SRS-V1", 12);
  h.update_u64be(srs->log_n);
  h.update_u64be(srs->tau_g1_len);
  h.update_u64be(srs->tau_g2_len);
  h.update_u64be(srs->alpha_len);
  h.update_u64be(srs->beta_len);
  digest_g1(h, srs->tau_g1, srs->tau_g1_len);
  digest_g2(h, srs->tau_g2, srs->tau_g2_len);
  digest_g1(h, srs->alpha_tau_g1, srs->alpha_len);
  digest_g1(h, srs->beta_tau_g1, srs->beta_len);
  digest_g2(h, &srs->beta_g2, 1);
  h.final(out);
  return ZK_OK;
}

int zk_groth16_key_digest_sound(const zk_pk* pk, const zk_vk* vk, uint8_t out[32]) {
  if (!pk || !vk || !out) return ZK_ERR_ARG;
  if ((pk->a_len && !pk->a_g1) || (pk->b_len && !pk->b_g1) || (pk->b2_len && !pk->b_g2) ||
      (pk->ic_len && !pk->ic_g1) || (pk->h_len && !pk->h_g1) || (vk->ic_len && !vk->ic_g1))
    return ZK_ERR_ARG;
  Sha256 h;
  h.update("ZKAMD-KEY-V1", 12);
  h.update_u64be(pk->a_len);
  h.update_u64be(pk->b_len);
  h.update_u64be(pk->b2_len);
  h.update_u64be(pk->ic_len);
  h.update_u64be(pk->h_len);
  h.update_u64be(pk->num_public);
  h.update_u64be(vk->ic_len);
  digest_g1(h, &pk->alpha_g1, 1);
  digest_g1(h, &pk->beta_g1, 1);
  digest_g1(h, &pk->delta_g1, 1);
  digest_g2(h, &pk->beta_g2, 1);
  digest_g2(h, &pk->delta_g2, 1);
  digest_g1(h, pk->a_g1, pk->a_len);
  digest_g1(h, pk->b_g1, pk->b_len);
  digest_g2(h, pk->b_g2, pk->b2_len);
  digest_g1(h, pk->ic_g1, pk->ic_len);
  digest_g1(h, pk->h_g1, pk->h_len);
  digest_g2(h, &vk->gamma_g2, 1);
  digest_g1(h, vk->ic_g1, vk->ic_len);
  h.final(out);
  return ZK_OK;
}

int zk_srs_prove_contribution(const zk_srs* before, const zk_fr* s, const zk_fr* a, const zk_fr* b,
                              zk_srs_contribution_proof* out) {
  if (!before || !s || !a || !b || !out) return ZK_ERR_ARG;
  uint8_t ch[32];
  int rc = zk_srs_digest(before, ch);
  if (rc == ZK_OK) rc = zk_pok_make(s, ZK_POK_TAU, ch, &out->tau);
  if (rc == ZK_OK) rc = zk_pok_make(a, ZK_POK_ALPHA, ch, &out->alpha);
  if (rc == ZK_OK) rc = zk_pok_make(b, ZK_POK_BETA, ch, &out->beta);
  return rc;
}

int zk_srs_verify_contribution_proofs(zk_ctx* ctx, const uint8_t* before_digests, const zk_srs_share* shares,
                                      const zk_srs_contribution_proof* proofs, size_t m, uint8_t* status) {
  if (!ctx || (m && (!before_digests || !shares || !proofs || !status))) return ZK_ERR_ARG;
  // the 3 m proofs, roles, challenges and share points as flat arrays: the
  // structs are three zk_pok / three zk_g2_affine back to back
  static_assert(sizeof(zk_srs_contribution_proof) == 3 * sizeof(zk_pok) && sizeof(zk_srs_share) == 3 * sizeof(zk_g2_affine),
                "a contribution's proofs and shares are arrays of three");
  std::vector<uint8_t> roles(3 * m), ch(32 * 3 * m);
  for (size_t i = 0; i < 3 * m; i++) {
    roles[i] = (uint8_t)(i % 3);   // ZK_POK_TAU, ZK_POK_ALPHA, ZK_POK_BETA
    std::memcpy(&ch[32 * i], before_digests + 32 * (i / 3), 32);
  }
  ZK_HGUARD(ctx, {
    return pok_verify_many_run(ctx, reinterpret_cast<const zk_pok*>(proofs), roles.data(), ch.data(),
                               reinterpret_cast<const zk_g2_affine*>(shares), 3 * m, status, nullptr);
  })
}
