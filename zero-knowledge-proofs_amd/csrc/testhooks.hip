// testhooks.hip -- libzkp_amd_test.so: the diagnostic entry points of
// include/zkp_test.h, built as a separate library on top of libzkp_amd.so so
// that the shipped ABI (include/zkp.h) holds no way to inject a failure or to
// drive the virtual-rank path.  Only the GPU tests load it.
#include <algorithm>
#include <cstring>
#include <vector>

#include "ceremony.hpp"
#include "ctx.hpp"
#include "hash.hpp"
#include "keycheck.hpp"
#include "msm.hpp"
#include "mulvec.hpp"
#include "pairing.hpp"
#include "points.hpp"
#include "prepared.hpp"
#include "prove.hpp"
#include "setup.hpp"
#include "verify_all.hpp"
#include "../../include/zkp_test.h"

using namespace zk;

#define ZK_TGUARD(ctx, ...)                                   \
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

int zk_test_prove_virtual_shards(zk_ctx* ctx, const zk_pk_dev* const* shards, uint32_t nshards, const void* d_z,
                                 size_t zlen, size_t num_public, const zk_fr* r, const zk_fr* s, zk_proof* out) {
  if (!ctx || !shards || !d_z || !r || !s || !out) return ZK_ERR_ARG;
  ZK_TGUARD(ctx, { return prove_virtual_shards_impl(ctx, shards, nshards, d_z, zlen, num_public, r, s, out); })
}

int zk_test_exchange(zk_ctx* ctx, size_t chunk_bytes, int32_t status, int32_t* out_max) {
  if (!ctx || !out_max || !chunk_bytes || chunk_bytes > ((size_t)1 << 30)) return ZK_ERR_ARG;
  ZK_TGUARD(ctx, {
    if (!ctx->exch) throw Error(ZK_ERR_ARG, "test_exchange: no exchange attached");
    Exchange& ex = *ctx->exch;
    const size_t W = (size_t)ex.world, bytes = chunk_bytes * W;
    std::vector<uint8_t> h(bytes);
    for (size_t k = 0; k < W; k++)
      for (size_t i = 0; i < chunk_bytes; i++) h[k * chunk_bytes + i] = (uint8_t)((ex.rank * 31 + k * 7 + i) & 0xff);
    DevBuf send, recv;
    send.ensure(bytes);
    recv.ensure(bytes);
    ZK_HIP(hipMemcpyAsync(send.p, h.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
    ZK_HIP(hipMemsetAsync(recv.p, 0, bytes, ctx->stream));
    ex.all_to_all(send.p, recv.p, chunk_bytes, ctx->stream);
    *out_max = ex.agree_max(status, ctx->stream);
    ZK_HIP(hipMemcpyAsync(h.data(), recv.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    for (size_t s = 0; s < W; s++)   // chunk s came from rank s, which filled its chunk `rank` for us
      for (size_t i = 0; i < chunk_bytes; i++)
        if (h[s * chunk_bytes + i] != (uint8_t)((s * 31 + (size_t)ex.rank * 7 + i) & 0xff)) return ZK_ERR_RCCL;
    return ZK_OK;
  })
}

int zk_test_fault_after_exchange(zk_ctx* ctx, int k) {
  if (!ctx || k < 0 || k > 3 || !ctx->exch) return ZK_ERR_ARG;
  ctx->exch->fault_after = k;
  return ZK_OK;
}

int zk_test_pk_bases(zk_ctx* ctx, const zk_pk_dev* pk, int slot, int window, uint32_t* idx_out, uint64_t* words_out,
                     size_t cap, size_t* count, size_t* nextras) {
  if (!ctx || !pk || !count || !nextras || slot < 0 || slot >= NUM_MSM || window < 0 || window >= pk->copies)
    return ZK_ERR_ARG;
  const size_t cnt = pk->count[slot], nex = pk->extras[slot], tot = cnt + nex;
  *count = cnt;
  *nextras = nex;
  if (!cap) return ZK_OK;
  if (cap < tot || !idx_out || !words_out) return ZK_ERR_ARG;
  ZK_TGUARD(ctx, {
    const bool g2 = slot == MSM_B2;
    const size_t asz = g2 ? sizeof(G2A) : sizeof(G1A);
    // IC and H share one window buffer (bases[MSM_H]: each window [IC | H])
    const bool ich = slot == MSM_IC || slot == MSM_H;
    const int bslot = ich ? MSM_H : slot;
    const size_t step = pk->stride[bslot] ? pk->stride[bslot] : asz;
    const size_t wtot = ich ? pk->ich_tot() : tot;
    const size_t skip = slot == MSM_H ? (size_t)pk->count[MSM_IC] + pk->extras[MSM_IC] : 0;
    const char* base = static_cast<const char*>(pk->bases[bslot].p) + ((size_t)window * wtot + skip) * step;
    if (cnt) ZK_HIP(hipMemcpyAsync(idx_out, pk->idx[slot].p, sizeof(uint32_t) * cnt, hipMemcpyDeviceToHost, ctx->stream));
    bases_to_abi_host(g2, base, pk->stride[bslot], tot, words_out, ctx->stream);
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    return ZK_OK;
  })
}

// ---- the 255-bit fixed-base kernel of a sound setup on its own ------------
int zk_test_fixed_base_g1(zk_ctx* ctx, const zk_fr* scalars, size_t n, zk_g1_affine* out) {
  if (!ctx || (n && (!scalars || !out))) return ZK_ERR_ARG;
  ZK_TGUARD(ctx, { return fixed_base_wide_host(ctx, false, scalars, n, reinterpret_cast<uint64_t*>(out)); })
}
int zk_test_fixed_base_g2(zk_ctx* ctx, const zk_fr* scalars, size_t n, zk_g2_affine* out) {
  if (!ctx || (n && (!scalars || !out))) return ZK_ERR_ARG;
  ZK_TGUARD(ctx, { return fixed_base_wide_host(ctx, true, scalars, n, reinterpret_cast<uint64_t*>(out)); })
}

// ---- n G1 points times one scalar by the plain 255-bit walk ----------------
namespace zk {
__global__ void __launch_bounds__(CM_BLOCK) k_g1_mul_plain(const uint64_t* __restrict__ in, size_t n, CmScalar s,
                                                           G1X* __restrict__ out) {
  cm_mul_point<false>(in, n, s, out);
}
}  // namespace zk
int zk_test_g1_mul_scalar_plain(zk_ctx* ctx, const zk_g1_affine* pts, size_t n, const zk_fr* k, zk_g1_affine* out) {
  if (!ctx || !k || (n && (!pts || !out))) return ZK_ERR_ARG;
  ZK_TGUARD(ctx, {
    CmScalar s;
    if (!cm_plain_scalar(*k, s)) return ZK_ERR_ARG;
    return g1_mul_scalar_run(ctx, pts, n, out, "g1_mul_scalar_plain",
                             [&](dim3 grid, hipStream_t st, const uint64_t* d_in, size_t m, G1X* d_x) {
                               k_g1_mul_plain<<<grid, CM_BLOCK, 0, st>>>(d_in, m, s, d_x);
                             });
  })
}

// ---- n points times n scalars: either walk of mulvec.hpp, and its split ----
namespace zk {
bool mv_scalars_ok(zk_ctx* ctx, const char* name, const zk_fr* k, size_t n);   // mulvec.hip
template <class F>
static int test_mul_scalars(zk_ctx* ctx, const void* pts, size_t n, const zk_fr* k, void* out, MvWalk walk,
                            const char* phase) {
  if (!ctx || (n && (!pts || !k || !out))) return ZK_ERR_ARG;
  if (!mv_scalars_ok(ctx, phase, k, n)) return ZK_ERR_ARG;
  ZK_TGUARD(ctx, { return mv_mul_scalars<F>(ctx, pts, n, k, nullptr, out, walk, phase); })
}
}  // namespace zk
int zk_test_g1_mul_scalars_plain(zk_ctx* ctx, const zk_g1_affine* pts, size_t n, const zk_fr* k, zk_g1_affine* out) {
  return test_mul_scalars<FqC>(ctx, pts, n, k, out, MV_PLAIN, "g1_mul_scalars_plain");
}
int zk_test_g2_mul_scalars_plain(zk_ctx* ctx, const zk_g2_affine* pts, size_t n, const zk_fr* k, zk_g2_affine* out) {
  return test_mul_scalars<Fq2C>(ctx, pts, n, k, out, MV_PLAIN, "g2_mul_scalars_plain");
}
int zk_test_g1_mul_scalars_table(zk_ctx* ctx, const zk_g1_affine* pts, size_t n, const zk_fr* k, zk_g1_affine* out) {
  return test_mul_scalars<FqC>(ctx, pts, n, k, out, MV_TABLE, "g1_mul_scalars_table");
}
int zk_test_g2_mul_scalars_table(zk_ctx* ctx, const zk_g2_affine* pts, size_t n, const zk_fr* k, zk_g2_affine* out) {
  return test_mul_scalars<Fq2C>(ctx, pts, n, k, out, MV_TABLE, "g2_mul_scalars_table");
}
int zk_test_split_scalars(zk_ctx* ctx, const zk_fr* k, size_t n, uint64_t* g1_out, uint64_t* g2_out) {
  if (!ctx || (n && !k)) return ZK_ERR_ARG;
  if (!mv_scalars_ok(ctx, "test_split_scalars", k, n)) return ZK_ERR_ARG;
  ZK_TGUARD(ctx, { return mv_split_host(ctx, k, n, g1_out, g2_out); })
}

// ---- the per-lane walks of srs.hpp on their own ----------------------------
// One lane per point, every lane from its OWN top bit, as gn_stage and
// gn_col_runs call the helpers (the trip count differs between the lanes of a
// wave); mv_mul_scalars' chunking.  MEM: the base waits in slot[i] as XYZZ and
// is fetched a coordinate at a time (gn_walk_mem), else mixed additions
// (gn_walk_aff).
namespace zk {
template <class F, bool MEM>
ZK_DI void tw_point(const uint64_t* __restrict__ in, size_t n, const uint64_t* __restrict__ k,
                    XYZZ<typename GnField<F>::Raw>* __restrict__ slot,
                    XYZZ<typename GnField<F>::Raw>* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * GN_BLOCK + threadIdx.x;
  if (i >= n) return;
  Affine<F> P;
  XYZZ<F> acc;
  const GnScalar s = gn_scalar(k + 4 * i);
  if (!gn_load_abi(in + GnField<F>::W * i, P) || s.top == 0) {
    xyzz_set_inf(acc);
  } else if constexpr (!MEM) {
    acc = gn_walk_aff(P, s);
  } else {
    gn_store(&slot[i], xyzz_from_aff(P));
    acc = gn_walk_mem<F>(&slot[i], s);
  }
  gn_store(&out[i], acc);
}
__global__ void __launch_bounds__(GN_BLOCK) k_test_gn_walk_aff_g1(const uint64_t* __restrict__ in, size_t n,
                                                                  const uint64_t* __restrict__ k,
                                                                  G1X* __restrict__ out) {
  tw_point<FqC, false>(in, n, k, nullptr, out);
}
__global__ void __launch_bounds__(GN_BLOCK) k_test_gn_walk_aff_g2(const uint64_t* __restrict__ in, size_t n,
                                                                  const uint64_t* __restrict__ k,
                                                                  G2X* __restrict__ out) {
  tw_point<Fq2C, false>(in, n, k, nullptr, out);
}
__global__ void __launch_bounds__(GN_BLOCK) k_test_gn_walk_mem_g1(const uint64_t* __restrict__ in, size_t n,
                                                                  const uint64_t* __restrict__ k,
                                                                  G1X* __restrict__ slot, G1X* __restrict__ out) {
  tw_point<FqC, true>(in, n, k, slot, out);
}
__global__ void __launch_bounds__(GN_BLOCK) k_test_gn_walk_mem_g2(const uint64_t* __restrict__ in, size_t n,
                                                                  const uint64_t* __restrict__ k,
                                                                  G2X* __restrict__ slot, G2X* __restrict__ out) {
  tw_point<Fq2C, true>(in, n, k, slot, out);
}
static void tw_launch(FqC, bool mem, const uint64_t* in, size_t m, const uint64_t* k, G1X* slot, G1X* out,
                      hipStream_t st) {
  if (mem) k_test_gn_walk_mem_g1<<<ceil_div(m, GN_BLOCK), GN_BLOCK, 0, st>>>(in, m, k, slot, out);
  else k_test_gn_walk_aff_g1<<<ceil_div(m, GN_BLOCK), GN_BLOCK, 0, st>>>(in, m, k, out);
}
static void tw_launch(Fq2C, bool mem, const uint64_t* in, size_t m, const uint64_t* k, G2X* slot, G2X* out,
                      hipStream_t st) {
  if (mem) k_test_gn_walk_mem_g2<<<ceil_div(m, GN_BLOCK), GN_BLOCK, 0, st>>>(in, m, k, slot, out);
  else k_test_gn_walk_aff_g2<<<ceil_div(m, GN_BLOCK), GN_BLOCK, 0, st>>>(in, m, k, out);
}

template <class F>
static int test_gn_walk(zk_ctx* ctx, bool mem, const void* pts, size_t n, const zk_fr* k, void* out) {
  using Raw = typename GnField<F>::Raw;
  using X = XYZZ<Raw>;
  using A = Affine<Raw>;
  constexpr size_t SZ = 8 * GnField<F>::W;
  hipStream_t st = ctx->stream;
  const size_t chunk = std::min<size_t>(std::max<size_t>(ctx->point_chunk, 1), n);
  DevBuf d_io, d_k, d_slot, d_x, d_pre, d_aff;
  d_io.ensure(SZ * chunk);
  d_k.ensure(sizeof(zk_fr) * chunk);
  if (mem) d_slot.ensure(sizeof(X) * chunk);
  d_x.ensure(sizeof(X) * chunk);
  d_pre.ensure(sizeof(Raw) * chunk);
  d_aff.ensure(sizeof(A) * chunk);
  for (size_t lo = 0; lo < n; lo += chunk) {
    const size_t m = std::min(chunk, n - lo);
    ZK_HIP(hipMemcpyAsync(d_io.p, static_cast<const char*>(pts) + SZ * lo, SZ * m, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_k.p, k + lo, sizeof(zk_fr) * m, hipMemcpyHostToDevice, st));
    tw_launch(F{}, mem, d_io.as<uint64_t>(), m, d_k.as<uint64_t>(), d_slot.as<X>(), d_x.as<X>(), st);
    ZK_LAUNCH_CHECK();
    batch_normalize<typename GnField<F>::C>(d_x.as<X>(), m, d_pre.as<Raw>(), d_aff.as<A>(), st);
    gn_points_to_abi<F>(d_aff.as<A>(), m, d_io.as<uint64_t>(), st);
    ZK_HIP(hipMemcpyAsync(static_cast<char*>(out) + SZ * lo, d_io.p, SZ * m, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));   // the next chunk reuses the buffers
  }
  return ZK_OK;
}
}  // namespace zk
int zk_test_gn_walk(zk_ctx* ctx, int g2, int mem, const void* pts, size_t n, const zk_fr* k, void* out) {
  if (!ctx || (g2 != 0 && g2 != 1) || (mem != 0 && mem != 1) || (n && (!pts || !k || !out))) return ZK_ERR_ARG;
  if (!mv_scalars_ok(ctx, "test_gn_walk", k, n)) return ZK_ERR_ARG;
  if (!n) return ZK_OK;
  ZK_TGUARD(ctx, {
    return g2 ? test_gn_walk<Fq2C>(ctx, mem != 0, pts, n, k, out) : test_gn_walk<FqC>(ctx, mem != 0, pts, n, k, out);
  })
}

// ---- the square roots of points.hpp on their own ---------------------------
namespace zk {
// K = 1: Fq, K = 2: Fq2 (c0 then c1); canonical words in and out
template <int K>
__global__ void __launch_bounds__(128) k_test_sqrt(const uint64_t* __restrict__ in, size_t n,
                                                   uint64_t* __restrict__ out, uint8_t* __restrict__ ok,
                                                   uint8_t* __restrict__ largest) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fq a[K], r[K];
#pragma unroll
  for (int k = 0; k < K; k++) {
    Fq c;
#pragma unroll
    for (int j = 0; j < 6; j++) {
      const uint64_t w = in[6 * (K * i + k) + j];
      c.v[2 * j] = (uint32_t)w;
      c.v[2 * j + 1] = (uint32_t)(w >> 32);
    }
    a[k] = pt_to_mont(c);
  }
  bool good;
  if constexpr (K == 1) {
    good = pt_fq_sqrt(a[0], r[0]);
  } else {
    Fq2 root;
    good = pt_fq2_sqrt(Fq2{a[0], a[1]}, root);
    r[0] = root.c0;
    r[1] = root.c1;
  }
#pragma unroll
  for (int k = 0; k < K; k++) r[k] = good ? pt_from_mont(r[k]) : fp_zero<FqParams>();
  bool big;
  if constexpr (K == 1) big = pt_fq_largest(r[0]);
  else big = pt_fq2_largest(Fq2{r[0], r[1]});
#pragma unroll
  for (int k = 0; k < K; k++)
#pragma unroll
    for (int j = 0; j < 6; j++)
      out[6 * (K * i + k) + j] = (uint64_t)r[k].v[2 * j] | ((uint64_t)r[k].v[2 * j + 1] << 32);
  ok[i] = good ? 1 : 0;
  largest[i] = (good && big) ? 1 : 0;
}

template <int K>
int test_sqrt(zk_ctx* ctx, const uint64_t* in, size_t n, uint64_t* out, uint8_t* ok, uint8_t* largest) {
  if (!n) return ZK_OK;
  const size_t words = 6 * K * n;
  DevBuf d_in, d_out, d_ok, d_big;
  d_in.ensure(8 * words);
  d_out.ensure(8 * words);
  d_ok.ensure(n);
  d_big.ensure(n);
  hipStream_t st = ctx->stream;
  ZK_HIP(hipMemcpyAsync(d_in.p, in, 8 * words, hipMemcpyHostToDevice, st));
  k_test_sqrt<K><<<ceil_div(n, 128), 128, 0, st>>>(d_in.as<uint64_t>(), n, d_out.as<uint64_t>(), d_ok.as<uint8_t>(),
                                                   d_big.as<uint8_t>());
  ZK_LAUNCH_CHECK();
  ZK_HIP(hipMemcpyAsync(out, d_out.p, 8 * words, hipMemcpyDeviceToHost, st));
  ZK_HIP(hipMemcpyAsync(ok, d_ok.p, n, hipMemcpyDeviceToHost, st));
  ZK_HIP(hipMemcpyAsync(largest, d_big.p, n, hipMemcpyDeviceToHost, st));
  ZK_HIP(hipStreamSynchronize(st));
  return ZK_OK;
}
}  // namespace zk

int zk_test_fq_sqrt(zk_ctx* ctx, const uint64_t* in, size_t n, uint64_t* out, uint8_t* ok, uint8_t* largest) {
  if (!ctx || (n && (!in || !out || !ok || !largest))) return ZK_ERR_ARG;
  ZK_TGUARD(ctx, { return test_sqrt<1>(ctx, in, n, out, ok, largest); })
}
int zk_test_fq2_sqrt(zk_ctx* ctx, const uint64_t* in, size_t n, uint64_t* out, uint8_t* ok, uint8_t* largest) {
  if (!ctx || (n && (!in || !out || !ok || !largest))) return ZK_ERR_ARG;
  ZK_TGUARD(ctx, { return test_sqrt<2>(ctx, in, n, out, ok, largest); })
}

// ---- the Fq12 tower and the pairing of pairing.hpp on their own -----------
namespace zk {
__device__ __forceinline__ void t_read_f12(const uint64_t* w, F12* a) {
  F2* co = &a->c0.c0;
#pragma unroll 1
  for (int j = 0; j < 6; j++) co[j] = {{pt_to_mont(pr_read_fq(w + 12 * j)), pt_to_mont(pr_read_fq(w + 12 * j + 6))}};
}
__device__ __forceinline__ void t_write_f12(uint64_t* w, const F12* a) {
  const F2* co = &a->c0.c0;
#pragma unroll 1
  for (int j = 0; j < 6; j++) {
    pr_write_fq(w + 12 * j, pt_from_mont(co[j].v.c0));
    pr_write_fq(w + 12 * j + 6, pt_from_mont(co[j].v.c1));
  }
}
__global__ void __launch_bounds__(64) k_test_fq12(int op, const uint64_t* __restrict__ a, const uint64_t* __restrict__ b,
                                                  size_t n, uint64_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  F12 x, y, r;
  t_read_f12(a + 72 * i, &x);
  if (op == ZK_TEST_FQ12_MUL || op == ZK_TEST_FQ12_LINE_MUL) t_read_f12(b + 72 * i, &y);
  switch (op) {
    case ZK_TEST_FQ12_MUL: f12_mul(&r, &x, &y); break;
    case ZK_TEST_FQ12_SQR: f12_sqr(&r, &x); break;
    case ZK_TEST_FQ12_INV: f12_inv(&r, &x); break;
    case ZK_TEST_FQ12_CONJ: f12_conj(&r, &x); break;
    case ZK_TEST_FQ12_FROB1: f12_frob1(&r, &x); break;
    case ZK_TEST_FQ12_FROB2: f12_frob2(&r, &x); break;
    case ZK_TEST_FQ12_CYC_SQR: f12_cyc_sqr(&r, &x); break;
    case ZK_TEST_FQ12_LINE_MUL: {
      const F2 l[3] = {y.c0.c0, y.c0.c1, y.c1.c1};
      r = x;
      f12_mul_line(&r, l);
      break;
    }
    default: r = x; f12_final_exp(&r); break;
  }
  t_write_f12(out + 72 * i, &r);
}
__global__ void __launch_bounds__(64) k_test_pairing_gt(const uint64_t* __restrict__ g1, const uint64_t* __restrict__ g2,
                                                        size_t n, uint64_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  PrPairs in;
  Affine<FqC> P;
  bool p_inf, q_inf;
  bool ok = pr_load_g1(g1 + 13 * i, &P, &p_inf);
  ok = pr_load_g2(g2 + 25 * i, &in.Q, &q_inf) && ok;
  in.on[0] = ok && !p_inf && !q_inf;
  in.on[1] = in.on[2] = false;
  in.xp[0] = P.x.v;
  in.yp[0] = P.y.v;
  in.tab[0] = in.tab[1] = nullptr;
  F12 f;
  pr_miller(&f, &in);
  f12_conj(&f, &f);
  f12_final_exp(&f);
  t_write_f12(out + 72 * i, &f);
}
}  // namespace zk

int zk_test_fq12(zk_ctx* ctx, int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out) {
  const bool two = op == ZK_TEST_FQ12_MUL || op == ZK_TEST_FQ12_LINE_MUL;
  if (!ctx || op < ZK_TEST_FQ12_MUL || op > ZK_TEST_FQ12_FINAL_EXP || (n && (!a || !out || (two && !b))))
    return ZK_ERR_ARG;
  if (!n) return ZK_OK;
  ZK_TGUARD(ctx, {
    DevBuf d_a, d_b, d_out;
    const size_t bytes = 8 * 72 * n;
    d_a.ensure(bytes);
    d_b.ensure(bytes);
    d_out.ensure(bytes);
    hipStream_t st = ctx->stream;
    ZK_HIP(hipMemcpyAsync(d_a.p, a, bytes, hipMemcpyHostToDevice, st));
    if (two) ZK_HIP(hipMemcpyAsync(d_b.p, b, bytes, hipMemcpyHostToDevice, st));
    k_test_fq12<<<ceil_div(n, 64), 64, 0, st>>>(op, d_a.as<uint64_t>(), d_b.as<uint64_t>(), n, d_out.as<uint64_t>());
    ZK_LAUNCH_CHECK();
    ZK_HIP(hipMemcpyAsync(out, d_out.p, bytes, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    return ZK_OK;
  })
}
int zk_test_pairing_gt(zk_ctx* ctx, const zk_g1_affine* g1, const zk_g2_affine* g2, size_t n, uint64_t* out) {
  if (!ctx || (n && (!g1 || !g2 || !out))) return ZK_ERR_ARG;
  if (!n) return ZK_OK;
  ZK_TGUARD(ctx, {
    DevBuf d_g1, d_g2, d_out;
    d_g1.ensure(sizeof(zk_g1_affine) * n);
    d_g2.ensure(sizeof(zk_g2_affine) * n);
    d_out.ensure(8 * 72 * n);
    hipStream_t st = ctx->stream;
    ZK_HIP(hipMemcpyAsync(d_g1.p, g1, sizeof(zk_g1_affine) * n, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_g2.p, g2, sizeof(zk_g2_affine) * n, hipMemcpyHostToDevice, st));
    k_test_pairing_gt<<<ceil_div(n, 64), 64, 0, st>>>(d_g1.as<uint64_t>(), d_g2.as<uint64_t>(), n, d_out.as<uint64_t>());
    ZK_LAUNCH_CHECK();
    ZK_HIP(hipMemcpyAsync(out, d_out.p, 8 * 72 * n, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    return ZK_OK;
  })
}

// ---- the three folds of the sound batch check on their own --------------------
namespace zk {
// one lane on the accumulators (slot 0) that verify_all_accumulate leaves
__global__ void __launch_bounds__(64) k_test_verify_all_parts(const F12* __restrict__ F, const XYZZ<FqC>* __restrict__ g,
                                                              const Fr* __restrict__ s, size_t W,
                                                              uint64_t* __restrict__ sum_c, uint64_t* __restrict__ scal,
                                                              uint64_t* __restrict__ gt) {
  if (blockIdx.x || threadIdx.x) return;
  F12 f = F[0];
  f12_conj(&f, &f);
  f12_final_exp(&f);
  t_write_f12(gt, &f);
  const XYZZ<FqC> sc = g[0];
  const bool inf = xyzz_is_inf(sc);
  Affine<FqC> P;
  f_set_zero(P.x);
  f_set_zero(P.y);
  if (!inf) P = pr_g1_affine(sc);
  pr_write_fq(sum_c, inf ? P.x.v : pt_from_mont(P.x.v));
  pr_write_fq(sum_c + 6, inf ? P.y.v : pt_from_mont(P.y.v));
  sum_c[12] = inf ? 1 : 0;
#pragma unroll 1
  for (size_t j = 0; j < W; j++) {
    const Fr c = fp_from_mont(s[j]);
#pragma unroll
    for (int k = 0; k < 4; k++) scal[4 * j + k] = (uint64_t)c.v[2 * k] | ((uint64_t)c.v[2 * k + 1] << 32);
  }
}
}  // namespace zk

int zk_test_verify_all_parts(zk_ctx* ctx, const zk_vk* vk, const zk_proof* proofs, const zk_fr* public_inputs,
                             size_t n_inputs, size_t n_proofs, const zk_fr* coeffs, zk_g1_affine* sum_c, zk_fr* scal,
                             uint64_t* gt) {
  if (!ctx || !vk || !sum_c || !scal || !gt || (n_proofs && (!proofs || !coeffs || (n_inputs && !public_inputs))))
    return ZK_ERR_ARG;
  ZK_TGUARD(ctx, {
    VerifyAll S;
    size_t first_bad = n_proofs;
    const int rc = verify_all_accumulate(ctx, vk, proofs, nullptr, public_inputs, n_inputs, n_proofs, coeffs,
                                         &first_bad, nullptr, S);
    if (ctx->prof.on) ctx->prof.collect();
    if (rc != ZK_OK) return rc;
    if (first_bad < n_proofs) {
      ctx->err = "proof " + std::to_string(first_bad) + " is malformed";
      return ZK_ERR_ARG;
    }
    const size_t W = S.W;
    DevBuf d_out;
    d_out.ensure(8 * (13 + 4 * W + 72));
    uint64_t* o = d_out.as<uint64_t>();
    hipStream_t st = ctx->stream;
    k_test_verify_all_parts<<<1, 64, 0, st>>>(S.F(), S.G(), S.S(), W, o, o + 13, o + 13 + 4 * W);
    ZK_LAUNCH_CHECK();
    ZK_HIP(hipMemcpyAsync(sum_c, o, 8 * 13, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipMemcpyAsync(scal, o + 13, 32 * W, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipMemcpyAsync(gt, o + 13 + 4 * W, 8 * 72, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    return ZK_OK;
  })
}

// ---- one field operation / one point formula of ff.hpp / curve.hpp per element --
// Raw device words in and out (no Montgomery conversion).  Blocks of one wave;
// a lane past the last element computes on the last element and skips only its
// store, so every lane of a pair / quad stays active through the arithmetic
// (the precondition of the lane-cooperative forms).
namespace zk {
constexpr int TF_BLOCK = 64;
// W: words of one element in memory; LANES: lanes that share it
template <class F>
struct TfLay {
  static constexpr int W = sizeof(F) / 4, LANES = 1;
};
template <>
struct TfLay<Fq2h> {
  static constexpr int W = 24, LANES = 2;
};
template <class F>
__device__ __forceinline__ F tf_load(const uint32_t* p) {
  F r;
  uint32_t* d = reinterpret_cast<uint32_t*>(&r);
#pragma unroll
  for (int k = 0; k < (int)(sizeof(F) / 4); k++) d[k] = p[k];
  return r;
}
template <class F>
__device__ __forceinline__ void tf_store(uint32_t* p, const F& v) {
  const uint32_t* s = reinterpret_cast<const uint32_t*>(&v);
#pragma unroll
  for (int k = 0; k < (int)(sizeof(F) / 4); k++) p[k] = s[k];
}

template <int OP, class P>
__device__ __forceinline__ Fp<P> tf_op(const Fp<P>& a, const Fp<P>& b, const Fp<P>& c, const Fp<P>& d) {
  if constexpr (OP == ZK_TEST_FOP_MUL) return fp_mul(a, b);
  else if constexpr (OP == ZK_TEST_FOP_SQR) return fp_sqr(a);
  else if constexpr (OP == ZK_TEST_FOP_ADD) return fp_add(a, b);
  else if constexpr (OP == ZK_TEST_FOP_SUB) return fp_sub(a, b);
  else if constexpr (OP == ZK_TEST_FOP_NEG) return fp_neg(a);
  else if constexpr (OP == ZK_TEST_FOP_DBL) return fp_dbl(a);
  else if constexpr (OP == ZK_TEST_FOP_INV) return fp_inv(a);
  else if constexpr (OP == ZK_TEST_FOP_TO_MONT) return fp_to_mont(a);
  else if constexpr (OP == ZK_TEST_FOP_FROM_MONT) return fp_from_mont(a);
  else if constexpr (OP == ZK_TEST_FOP_MUL_LAZY) return fp_mul<P, false>(a, b);
  else if constexpr (OP == ZK_TEST_FOP_MUL_SUB) return fq_mul_sub(a, b, c, d);
  else return fq_inv(a);
}
template <int OP>
__device__ __forceinline__ Fq2 tf_op(const Fq2& a, const Fq2& b, const Fq2& c, const Fq2& d) {
  if constexpr (OP == ZK_TEST_FOP_MUL) return fq2_mul(a, b);
  else if constexpr (OP == ZK_TEST_FOP_SQR) return fq2_sqr(a);
  else if constexpr (OP == ZK_TEST_FOP_INV) return fq2_inv(a);
  else if constexpr (OP == ZK_TEST_FOP_ADD) return fq2_add(a, b);
  else if constexpr (OP == ZK_TEST_FOP_SUB) return fq2_sub(a, b);
  else if constexpr (OP == ZK_TEST_FOP_NEG) return fq2_neg(a);
  else return f_mul_sub(a, b, c, d);
}
template <int OP>
__device__ __forceinline__ Fq2h tf_op(const Fq2h& a, const Fq2h& b, const Fq2h& c, const Fq2h& d) {
  if constexpr (OP == ZK_TEST_FOP_MUL) return f_mul(a, b);
  else if constexpr (OP == ZK_TEST_FOP_SQR) return f_sqr(a);
  else if constexpr (OP == ZK_TEST_FOP_MUL_SUB) return f_mul_sub(a, b, c, d);
  else if constexpr (OP == ZK_TEST_FOP_ADD) return f_add(a, b);
  else if constexpr (OP == ZK_TEST_FOP_SUB) return f_sub(a, b);
  else if constexpr (OP == ZK_TEST_FOP_NEG) return f_neg(a);
  else {
    Fq2h r;
    f_set_zero(r);
    r.v.v[0] = f_is_zero(a) ? 1u : 0u;
    return r;
  }
}
constexpr bool tf_reads_b(int op) {
  return op == ZK_TEST_FOP_MUL || op == ZK_TEST_FOP_ADD || op == ZK_TEST_FOP_SUB || op == ZK_TEST_FOP_MUL_LAZY ||
         op == ZK_TEST_FOP_MUL_SUB;
}

template <class F, int OP>
__global__ void __launch_bounds__(TF_BLOCK) k_test_field(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                         const uint32_t* __restrict__ c, const uint32_t* __restrict__ d,
                                                         size_t n, uint32_t* __restrict__ out) {
  constexpr int W = TfLay<F>::W, L = TfLay<F>::LANES, S = sizeof(F) / 4;
  const size_t gid = (size_t)blockIdx.x * TF_BLOCK + threadIdx.x;
  const size_t e = gid / L, h = gid % L;
  const bool live = e < n;
  const size_t off = (live ? e : n - 1) * W + h * S;
  const F x = tf_load<F>(a + off);
  F y = x, z = x, w = x;
  if constexpr (tf_reads_b(OP)) y = tf_load<F>(b + off);
  if constexpr (OP == ZK_TEST_FOP_MUL_SUB) {
    z = tf_load<F>(c + off);
    w = tf_load<F>(d + off);
  }
  const F r = tf_op<OP>(x, y, z, w);
  if (live) tf_store(out + off, r);
}

template <class F, int OP>
void tf_launch(zk_ctx* ctx, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, size_t n,
               uint32_t* out) {
  const size_t bytes = 4 * (size_t)TfLay<F>::W * n;
  DevBuf d_in[4], d_out;
  const uint32_t* h[4] = {a, tf_reads_b(OP) ? b : nullptr, OP == ZK_TEST_FOP_MUL_SUB ? c : nullptr,
                          OP == ZK_TEST_FOP_MUL_SUB ? d : nullptr};
  hipStream_t st = ctx->stream;
  for (int k = 0; k < 4; k++) {
    if (!h[k]) continue;
    d_in[k].ensure(bytes);
    ZK_HIP(hipMemcpyAsync(d_in[k].p, h[k], bytes, hipMemcpyHostToDevice, st));
  }
  d_out.ensure(bytes);
  k_test_field<F, OP><<<ceil_div(n * TfLay<F>::LANES, (size_t)TF_BLOCK), TF_BLOCK, 0, st>>>(
      d_in[0].as<uint32_t>(), d_in[1].as<uint32_t>(), d_in[2].as<uint32_t>(), d_in[3].as<uint32_t>(), n,
      d_out.as<uint32_t>());
  ZK_LAUNCH_CHECK();
  ZK_HIP(hipMemcpyAsync(out, d_out.p, bytes, hipMemcpyDeviceToHost, st));
  ZK_HIP(hipStreamSynchronize(st));
}

// lanes per element of a formula: the field's own, or four for the quad / duo adds
template <class F, int OP>
constexpr int tc_lanes() {
  return (OP == ZK_TEST_COP_ADD_QUAD || OP == ZK_TEST_COP_ADD_DUO) ? 4 : TfLay<F>::LANES;
}
template <class F, int OP>
__global__ void __launch_bounds__(TF_BLOCK) k_test_curve(const uint32_t* __restrict__ p, const uint32_t* __restrict__ q,
                                                         size_t n, uint32_t* __restrict__ out) {
  constexpr int W = TfLay<F>::W, L = TfLay<F>::LANES, S = sizeof(F) / 4, LPE = tc_lanes<F, OP>();
  constexpr bool AFF = OP == ZK_TEST_COP_MADD || OP == ZK_TEST_COP_AFF_DBL;
  constexpr bool ONE = OP == ZK_TEST_COP_DBL || OP == ZK_TEST_COP_DBL_CALL;
  const size_t gid = (size_t)blockIdx.x * TF_BLOCK + threadIdx.x;
  const size_t e = gid / LPE, h = gid % L;
  const bool live = e < n;
  const size_t ec = live ? e : n - 1;
  XYZZ<F> P, Q, r;
  Affine<F> A;
  if constexpr (OP != ZK_TEST_COP_AFF_DBL) {
    const uint32_t* s = p + ec * 4 * W + h * S;
    P.X = tf_load<F>(s);
    P.Y = tf_load<F>(s + W);
    P.ZZ = tf_load<F>(s + 2 * W);
    P.ZZZ = tf_load<F>(s + 3 * W);
  }
  if constexpr (AFF) {
    const uint32_t* s = q + ec * 2 * W + h * S;
    A.x = tf_load<F>(s);
    A.y = tf_load<F>(s + W);
  } else if constexpr (!ONE) {
    const uint32_t* s = q + ec * 4 * W + h * S;
    Q.X = tf_load<F>(s);
    Q.Y = tf_load<F>(s + W);
    Q.ZZ = tf_load<F>(s + 2 * W);
    Q.ZZZ = tf_load<F>(s + 3 * W);
  }
  if constexpr (OP == ZK_TEST_COP_DBL) r = xyzz_dbl(P);
  else if constexpr (OP == ZK_TEST_COP_DBL_CALL) r = xyzz_dbl_call(P);
  else if constexpr (OP == ZK_TEST_COP_AFF_DBL) r = aff_dbl(A);
  else if constexpr (OP == ZK_TEST_COP_MADD) r = xyzz_madd(P, A);
  else if constexpr (OP == ZK_TEST_COP_ADD) r = xyzz_add(P, Q);
  else if constexpr (OP == ZK_TEST_COP_ADD_ILP) r = xyzz_add_ilp(P, Q);
  else if constexpr (OP == ZK_TEST_COP_ADD_QUAD) r = xyzz_add_quad(P, Q);
  else r = xyzz_add_duo(P, Q);
  if (live) {   // one result per lane (quad), per lane pair (duo), else per element
    uint32_t* o = out + (gid / L) * 4 * W + h * S;
    tf_store(o, r.X);
    tf_store(o + W, r.Y);
    tf_store(o + 2 * W, r.ZZ);
    tf_store(o + 3 * W, r.ZZZ);
  }
}

template <class F, int OP>
void tc_launch(zk_ctx* ctx, const uint32_t* p, const uint32_t* q, size_t n, uint32_t* out) {
  constexpr int W = TfLay<F>::W, L = TfLay<F>::LANES, LPE = tc_lanes<F, OP>();
  constexpr bool AFF = OP == ZK_TEST_COP_MADD || OP == ZK_TEST_COP_AFF_DBL;
  const size_t pb = 16 * (size_t)W * n, qb = (AFF ? 8 : 16) * (size_t)W * n, ob = pb * (LPE / L);
  DevBuf d_p, d_q, d_out;
  hipStream_t st = ctx->stream;
  if (p) {
    d_p.ensure(pb);
    ZK_HIP(hipMemcpyAsync(d_p.p, p, pb, hipMemcpyHostToDevice, st));
  }
  if (q) {
    d_q.ensure(qb);
    ZK_HIP(hipMemcpyAsync(d_q.p, q, qb, hipMemcpyHostToDevice, st));
  }
  d_out.ensure(ob);
  k_test_curve<F, OP><<<ceil_div(n * LPE, (size_t)TF_BLOCK), TF_BLOCK, 0, st>>>(d_p.as<uint32_t>(), d_q.as<uint32_t>(), n,
                                                                               d_out.as<uint32_t>());
  ZK_LAUNCH_CHECK();
  ZK_HIP(hipMemcpyAsync(out, d_out.p, ob, hipMemcpyDeviceToHost, st));
  ZK_HIP(hipStreamSynchronize(st));
}
// the six formulas every field takes
template <class F>
bool tc_common(zk_ctx* ctx, int op, const uint32_t* p, const uint32_t* q, size_t n, uint32_t* out) {
  switch (op) {
    case ZK_TEST_COP_DBL: tc_launch<F, ZK_TEST_COP_DBL>(ctx, p, nullptr, n, out); return true;
    case ZK_TEST_COP_DBL_CALL: tc_launch<F, ZK_TEST_COP_DBL_CALL>(ctx, p, nullptr, n, out); return true;
    case ZK_TEST_COP_AFF_DBL: tc_launch<F, ZK_TEST_COP_AFF_DBL>(ctx, nullptr, q, n, out); return true;
    case ZK_TEST_COP_MADD: tc_launch<F, ZK_TEST_COP_MADD>(ctx, p, q, n, out); return true;
    case ZK_TEST_COP_ADD: tc_launch<F, ZK_TEST_COP_ADD>(ctx, p, q, n, out); return true;
    case ZK_TEST_COP_ADD_ILP: tc_launch<F, ZK_TEST_COP_ADD_ILP>(ctx, p, q, n, out); return true;
    default: return false;
  }
}
}  // namespace zk

#define TF_CASE(F, OP) \
  case OP: tf_launch<F, OP>(ctx, a, b, c, d, n, out); return ZK_OK;
int zk_test_field(zk_ctx* ctx, int field, int op, const uint32_t* a, const uint32_t* b, const uint32_t* c,
                  const uint32_t* d, size_t n, uint32_t* out) {
  if (!ctx || field < ZK_TEST_FIELD_FR || field > ZK_TEST_FIELD_FQ2H || op < ZK_TEST_FOP_MUL ||
      op > ZK_TEST_FOP_IS_ZERO)
    return ZK_ERR_ARG;
  const bool prime = field == ZK_TEST_FIELD_FR || field == ZK_TEST_FIELD_FQ;
  bool known;
  switch (op) {
    case ZK_TEST_FOP_DBL: case ZK_TEST_FOP_TO_MONT: case ZK_TEST_FOP_FROM_MONT: known = prime; break;
    case ZK_TEST_FOP_INV: known = field != ZK_TEST_FIELD_FQ2H; break;
    case ZK_TEST_FOP_MUL_LAZY: known = field == ZK_TEST_FIELD_FR; break;
    case ZK_TEST_FOP_MUL_SUB: known = field != ZK_TEST_FIELD_FR; break;
    case ZK_TEST_FOP_FQ_INV: known = field == ZK_TEST_FIELD_FQ; break;
    case ZK_TEST_FOP_IS_ZERO: known = field == ZK_TEST_FIELD_FQ2H; break;
    default: known = true; break;
  }
  if (!known) return ZK_ERR_ARG;
  if (n && (!a || !out || (tf_reads_b(op) && !b) || (op == ZK_TEST_FOP_MUL_SUB && (!c || !d)))) return ZK_ERR_ARG;
  if (!n) return ZK_OK;
  ZK_TGUARD(ctx, {
    switch (field) {
      case ZK_TEST_FIELD_FR:
        switch (op) {
          TF_CASE(Fr, ZK_TEST_FOP_MUL) TF_CASE(Fr, ZK_TEST_FOP_SQR) TF_CASE(Fr, ZK_TEST_FOP_ADD)
          TF_CASE(Fr, ZK_TEST_FOP_SUB) TF_CASE(Fr, ZK_TEST_FOP_NEG) TF_CASE(Fr, ZK_TEST_FOP_DBL)
          TF_CASE(Fr, ZK_TEST_FOP_INV) TF_CASE(Fr, ZK_TEST_FOP_TO_MONT) TF_CASE(Fr, ZK_TEST_FOP_FROM_MONT)
          TF_CASE(Fr, ZK_TEST_FOP_MUL_LAZY)
        }
        break;
      case ZK_TEST_FIELD_FQ:
        switch (op) {
          TF_CASE(Fq, ZK_TEST_FOP_MUL) TF_CASE(Fq, ZK_TEST_FOP_SQR) TF_CASE(Fq, ZK_TEST_FOP_ADD)
          TF_CASE(Fq, ZK_TEST_FOP_SUB) TF_CASE(Fq, ZK_TEST_FOP_NEG) TF_CASE(Fq, ZK_TEST_FOP_DBL)
          TF_CASE(Fq, ZK_TEST_FOP_INV) TF_CASE(Fq, ZK_TEST_FOP_TO_MONT) TF_CASE(Fq, ZK_TEST_FOP_FROM_MONT)
          TF_CASE(Fq, ZK_TEST_FOP_MUL_SUB) TF_CASE(Fq, ZK_TEST_FOP_FQ_INV)
        }
        break;
      case ZK_TEST_FIELD_FQ2:
        switch (op) {
          TF_CASE(Fq2, ZK_TEST_FOP_MUL) TF_CASE(Fq2, ZK_TEST_FOP_SQR) TF_CASE(Fq2, ZK_TEST_FOP_INV)
          TF_CASE(Fq2, ZK_TEST_FOP_ADD) TF_CASE(Fq2, ZK_TEST_FOP_SUB) TF_CASE(Fq2, ZK_TEST_FOP_NEG)
          TF_CASE(Fq2, ZK_TEST_FOP_MUL_SUB)
        }
        break;
      default:
        switch (op) {
          TF_CASE(Fq2h, ZK_TEST_FOP_MUL) TF_CASE(Fq2h, ZK_TEST_FOP_SQR) TF_CASE(Fq2h, ZK_TEST_FOP_MUL_SUB)
          TF_CASE(Fq2h, ZK_TEST_FOP_ADD) TF_CASE(Fq2h, ZK_TEST_FOP_SUB) TF_CASE(Fq2h, ZK_TEST_FOP_NEG)
          TF_CASE(Fq2h, ZK_TEST_FOP_IS_ZERO)
        }
        break;
    }
    return ZK_ERR_ARG;
  })
}
#undef TF_CASE

int zk_test_curve(zk_ctx* ctx, int field, int op, const uint32_t* p, const uint32_t* q, size_t n, uint32_t* out) {
  if (!ctx || field < ZK_TEST_FIELD_FQ || field > ZK_TEST_FIELD_FQ2C || op < ZK_TEST_COP_DBL ||
      op > ZK_TEST_COP_ADD_DUO)
    return ZK_ERR_ARG;
  if (op == ZK_TEST_COP_ADD_QUAD && field != ZK_TEST_FIELD_FQ) return ZK_ERR_ARG;
  if (op == ZK_TEST_COP_ADD_DUO && field != ZK_TEST_FIELD_FQ2H) return ZK_ERR_ARG;
  const bool reads_p = op != ZK_TEST_COP_AFF_DBL, reads_q = op != ZK_TEST_COP_DBL && op != ZK_TEST_COP_DBL_CALL;
  if (n && (!out || (reads_p && !p) || (reads_q && !q))) return ZK_ERR_ARG;
  if (!n) return ZK_OK;
  ZK_TGUARD(ctx, {
    bool done;
    if (op == ZK_TEST_COP_ADD_QUAD) {
      tc_launch<Fq, ZK_TEST_COP_ADD_QUAD>(ctx, p, q, n, out);
      done = true;
    } else if (op == ZK_TEST_COP_ADD_DUO) {
      tc_launch<Fq2h, ZK_TEST_COP_ADD_DUO>(ctx, p, q, n, out);
      done = true;
    } else {
      switch (field) {
        case ZK_TEST_FIELD_FQ: done = tc_common<Fq>(ctx, op, p, q, n, out); break;
        case ZK_TEST_FIELD_FQ2: done = tc_common<Fq2>(ctx, op, p, q, n, out); break;
        case ZK_TEST_FIELD_FQ2H: done = tc_common<Fq2h>(ctx, op, p, q, n, out); break;
        case ZK_TEST_FIELD_FQC: done = tc_common<FqC>(ctx, op, p, q, n, out); break;
        default: done = tc_common<Fq2C>(ctx, op, p, q, n, out); break;
      }
    }
    return done ? ZK_OK : ZK_ERR_ARG;
  })
}

int zk_test_pk_info(const zk_pk_dev* pk,uint32_t* win, uint32_t* win_c, uint32_t* shard, uint32_t* nshards) {
  if (!pk || !win || !win_c || !shard || !nshards) return ZK_ERR_ARG;
  *win = (uint32_t)pk->win;
  *win_c = (uint32_t)pk->win_c;
  *shard = pk->shard;
  *nshards = pk->nshards;
  return ZK_OK;
}

int zk_test_pk_plan(const zk_pk_dev* pk, uint32_t* copies, uint32_t* sets) {
  if (!pk || !copies || !sets) return ZK_ERR_ARG;
  *copies = (uint32_t)pk->copies;
  *sets = (uint32_t)((pk->win + pk->copies - 1) / pk->copies);
  return ZK_OK;
}

// ---- the hash to G2 under a try cap (hash.hip's kernel, unchanged) ----
int zk_test_hash_to_g2_capped(zk_ctx* ctx, const uint8_t* msgs, size_t n, size_t msg_len, const uint8_t* dst,
                              size_t dst_len, uint32_t max_tries, zk_g2_affine* out, uint8_t* tries) {
  if (!ctx || (n && (!out || (msg_len && !msgs))) || (dst_len && !dst) || dst_len > 255 || max_tries < 1 ||
      max_tries > H2_MAX_TRIES)
    return ZK_ERR_ARG;
  ZK_TGUARD(ctx, { return hash_to_g2_run(ctx, msgs, n, msg_len, dst, dst_len, max_tries, out, tries); })
}

// ---- prepared verification keys: the rules, and their overrides ----
int zk_test_prepared_plan(int sound, uint64_t num_public, int force_width, uint32_t* width, uint32_t* windows,
                          uint64_t* table_bytes, uint64_t* dev_bytes, uint64_t* bound) {
  if (!width || !windows || !table_bytes || !dev_bytes || !bound) return ZK_ERR_ARG;
  if (force_width != 0 && force_width != 1 && force_width != 2 && force_width != 4 && force_width != 8) return ZK_ERR_ARG;
  const int b = force_width ? force_width : prep_width(sound != 0, num_public);
  *width = (uint32_t)b;
  *windows = b ? (uint32_t)prep_windows(sound != 0, b) : 0;
  *table_bytes = b ? prep_table_bytes(sound != 0, num_public, b) : 0;
  *dev_bytes = 4 * prep_words(num_public) + *table_bytes;
  *bound = PREP_TABLE_MAX;
  return ZK_OK;
}
int zk_test_prepared_run(uint64_t m, uint64_t num_public, uint32_t windows, uint64_t* run, uint64_t* fill) {
  if (!run || !fill) return ZK_ERR_ARG;
  *run = prep_run_len(m, num_public, (int)windows);
  *fill = PREP_FILL;
  return ZK_OK;
}
int zk_test_prepared_force(zk_ctx* ctx, int width, uint32_t run) {
  if (!ctx || (width != 0 && width != 1 && width != 2 && width != 4 && width != 8)) return ZK_ERR_ARG;
  ctx->prep_width = width;
  ctx->prep_run = run;
  return ZK_OK;
}
int zk_test_prepared_info(const zk_vk_dev* pvk, uint32_t* width, uint32_t* windows) {
  if (!pvk || !width || !windows) return ZK_ERR_ARG;
  *width = (uint32_t)pvk->width;
  *windows = (uint32_t)pvk->windows;
  return ZK_OK;
}

// ---- MSM chunking: the accumulate units and the fixup threshold under a
// test's control, and readbacks of what the last MSM of a workspace did ----
namespace zk {
// works 0..4: ctx->msm[], 5: part_g2[0], 6: part_abi[0]
static MsmWork* test_msm_work(zk_ctx* ctx, int which) {
  if (which >= 0 && which < NUM_MSM) return &ctx->msm[which];
  if (which == NUM_MSM) return &ctx->part_g2[0];
  if (which == NUM_MSM + 1) return &ctx->part_abi[0];
  return nullptr;
}
// every stream an MSM of this ctx may still run on
static void test_msm_sync(zk_ctx* ctx) {
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < NUM_SIDE; k++)
    if (ctx->side[k]) ZK_HIP(hipStreamSynchronize(ctx->side[k]));
}
// a workspace that has run an MSM: its plan and its device arrays exist
static bool test_msm_ran(const MsmWork& w) { return w.plan.G && w.off.p && w.nbig.p && w.key.p && w.ent.p; }
}  // namespace zk

int zk_test_msm_force(zk_ctx* ctx, uint32_t T, uint32_t fix_max) {
  if (!ctx || T > (1u << 22)) return ZK_ERR_ARG;
  for (int k = 0; k < NUM_MSM; k++) {
    ctx->msm[k].force_T = T;
    ctx->msm[k].force_fix_max = fix_max;
  }
  for (int k = 0; k < HOST_PARTS - 1; k++) {
    ctx->part_g2[k].force_T = ctx->part_abi[k].force_T = T;
    ctx->part_g2[k].force_fix_max = ctx->part_abi[k].force_fix_max = fix_max;
  }
  return ZK_OK;
}

int zk_test_msm_info(zk_ctx* ctx, int which, int g2, uint32_t* info) {
  if (!ctx || !info || (g2 != 0 && g2 != 1)) return ZK_ERR_ARG;
  MsmWork* w = test_msm_work(ctx, which);
  if (!w) return ZK_ERR_ARG;
  ZK_TGUARD(ctx, {
    if (!test_msm_ran(*w)) throw Error(ZK_ERR_ARG, "test_msm_info: no MSM has run on this workspace");
    const MsmPlan& p = w->plan;
    test_msm_sync(ctx);
    uint32_t M = 0, nbig = 0;
    ZK_HIP(hipMemcpy(&M, w->off.as<uint32_t>() + p.G, sizeof(uint32_t), hipMemcpyDeviceToHost));
    ZK_HIP(hipMemcpy(&nbig, w->nbig.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
    info[ZK_TEST_MSM_C] = (uint32_t)p.c;
    info[ZK_TEST_MSM_NWIN] = (uint32_t)p.nwin;
    info[ZK_TEST_MSM_BITS] = (uint32_t)p.bits;
    info[ZK_TEST_MSM_SW] = (uint32_t)p.sw;
    info[ZK_TEST_MSM_SHARED] = (uint32_t)p.shared;
    info[ZK_TEST_MSM_COPIES] = (uint32_t)p.copies;
    info[ZK_TEST_MSM_NRED] = p.nred;
    info[ZK_TEST_MSM_NSEG] = (uint32_t)p.nseg;
    info[ZK_TEST_MSM_SEGSHIFT] = p.segshift;
    info[ZK_TEST_MSM_G] = p.G;
    info[ZK_TEST_MSM_T] = p.T;
    info[ZK_TEST_MSM_FIX_MAX] = p.fix_max;
    info[ZK_TEST_MSM_M] = M;
    info[ZK_TEST_MSM_NBIG] = nbig;
    info[ZK_TEST_MSM_NATURAL_T] = g2 ? msm_accum_units<G2>() : msm_accum_units<G1>();
    info[ZK_TEST_MSM_N] = p.n;
    return ZK_OK;
  })
}

int zk_test_msm_grouping(zk_ctx* ctx, int which, uint32_t* off_out, uint32_t* key_out, uint32_t* ent_out, size_t cap,
                         size_t* G, size_t* M) {
  if (!ctx || !G || !M) return ZK_ERR_ARG;
  MsmWork* w = test_msm_work(ctx, which);
  if (!w) return ZK_ERR_ARG;
  ZK_TGUARD(ctx, {
    if (!test_msm_ran(*w)) throw Error(ZK_ERR_ARG, "test_msm_grouping: no MSM has run on this workspace");
    const uint32_t g = w->plan.G;
    test_msm_sync(ctx);
    uint32_t m = 0;
    ZK_HIP(hipMemcpy(&m, w->off.as<uint32_t>() + g, sizeof(uint32_t), hipMemcpyDeviceToHost));
    *G = g;
    *M = m;
    if (!cap) return ZK_OK;
    if (cap < (size_t)g + 1 || cap < m || !off_out || !key_out || !ent_out) return ZK_ERR_ARG;
    // off[G] never exceeds the entries the front sized key / ent for
    if (sizeof(uint32_t) * (size_t)m > w->key.bytes || sizeof(uint32_t) * (size_t)m > w->ent.bytes ||
        sizeof(uint32_t) * ((size_t)g + 1) > w->off.bytes)
      throw Error(ZK_ERR_DEVICE, "test_msm_grouping: off[G] exceeds the workspace");
    ZK_HIP(hipMemcpy(off_out, w->off.p, sizeof(uint32_t) * ((size_t)g + 1), hipMemcpyDeviceToHost));
    if (m) {
      ZK_HIP(hipMemcpy(key_out, w->key.p, sizeof(uint32_t) * m, hipMemcpyDeviceToHost));
      ZK_HIP(hipMemcpy(ent_out, w->ent.p, sizeof(uint32_t) * m, hipMemcpyDeviceToHost));
    }
    return ZK_OK;
  })
}

int zk_test_msm_scrub(zk_ctx* ctx) {
  if (!ctx) return ZK_ERR_ARG;
  ZK_TGUARD(ctx, {
    test_msm_sync(ctx);
    for (int which = 0; which < NUM_MSM + 2; which++) {
      MsmWork* w = test_msm_work(ctx, which);
      for (DevBuf* b : {&w->buckets, &w->partials, &w->partials2, &w->rc, &w->res})
        if (b->p && b->bytes) ZK_HIP(hipMemset(b->p, 0xA5, b->bytes));
    }
    ZK_HIP(hipDeviceSynchronize());
    return ZK_OK;
  })
}

// ---- the coefficient side of zk_groth16_verify_key_srs_sound on its own ----
int zk_test_key_srs_coeffs(zk_ctx* ctx, const zk_r1cs_csr* qap, uint64_t num_public, const zk_fr* rho, zk_fr* out) {
  if (!ctx || !qap || !rho || !out) return ZK_ERR_ARG;
  ZK_TGUARD(ctx, { return key_srs_coeffs_host(ctx, qap, num_public, rho, out); })
}
