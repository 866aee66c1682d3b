// mulvec.hip -- n points times n different scalars on the GPU, both groups
// (include/zkp.h, "phase-1 contributions"; the walks and their algebra:
// mulvec.hpp).  No reference counterpart.
#include <algorithm>
#include <string>

#include "msm.hpp"
#include "mulvec.hpp"

namespace zk {

// One lane per point: ABI point i times the canonical scalar k[4 i ..] -> XYZZ.
// tab: the lanes' tables, entry m of lane i at tab[m n + i] (TABLE only).
template <class F, bool TABLE>
ZK_DI void mv_point(const uint64_t* __restrict__ in, size_t n, const uint64_t* __restrict__ k,
                    XYZZ<typename GnField<F>::Raw>* __restrict__ tab,
                    XYZZ<typename GnField<F>::Raw>* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * MV_BLOCK + threadIdx.x;
  if (i >= n) return;
  Affine<F> P;
  XYZZ<F> acc;
  GnScalar s = gn_scalar(k + 4 * i);
  const bool zero = s.top == 0;
  // The plain walk from bit 254 in every lane, not from the lane's own top
  // bit: leading zero bits double the identity.  With per-lane trip counts the
  // G1 kernel (two waves per SIMD) gave wrong lanes that changed from run to
  // run once a launch had more than 256 blocks; with one trip count it is exact
  // (DESIGN.md 2.17).
  s.top = 255;
  if (!gn_load_abi(in + GnField<F>::W * i, P) || zero) xyzz_set_inf(acc);
  else if constexpr (!TABLE) acc = gn_walk_aff(P, s);
  else if constexpr (GnField<F>::W == 13) acc = mv_walk_g1(P, k + 4 * i, tab + i, n);
  else acc = mv_walk_g2(P, k + 4 * i, tab + i, n);
  gn_store(&out[i], acc);
}
__global__ void __launch_bounds__(MV_BLOCK) k_g1_mul_scalars(const uint64_t* __restrict__ in, size_t n,
                                                             const uint64_t* __restrict__ k, G1X* __restrict__ tab,
                                                             G1X* __restrict__ out) {
  mv_point<FqC, true>(in, n, k, tab, out);
}
__global__ void __launch_bounds__(MV_BLOCK) k_g2_mul_scalars(const uint64_t* __restrict__ in, size_t n,
                                                             const uint64_t* __restrict__ k, G2X* __restrict__ tab,
                                                             G2X* __restrict__ out) {
  mv_point<Fq2C, true>(in, n, k, tab, out);
}
__global__ void __launch_bounds__(MV_BLOCK) k_g1_mul_scalars_plain(const uint64_t* __restrict__ in, size_t n,
                                                                   const uint64_t* __restrict__ k,
                                                                   G1X* __restrict__ out) {
  mv_point<FqC, false>(in, n, k, nullptr, out);
}
__global__ void __launch_bounds__(MV_BLOCK) k_g2_mul_scalars_plain(const uint64_t* __restrict__ in, size_t n,
                                                                   const uint64_t* __restrict__ k,
                                                                   G2X* __restrict__ out) {
  mv_point<Fq2C, false>(in, n, k, nullptr, out);
}
// the decomposition alone: g1[4 i ..] = e1, e2; g2[4 i ..] = d0 .. d3
__global__ void __launch_bounds__(MV_BLOCK) k_mv_split(const uint64_t* __restrict__ k, size_t n,
                                                       uint64_t* __restrict__ g1, uint64_t* __restrict__ g2) {
  const size_t i = (size_t)blockIdx.x * MV_BLOCK + threadIdx.x;
  if (i >= n) return;
  uint64_t d[4];
  mv_split(k + 4 * i, d);
  mv_join(d[0], d[1], g1 + 4 * i);
  mv_join(d[2], d[3], g1 + 4 * i + 2);
#pragma unroll
  for (int j = 0; j < 4; j++) g2[4 * i + j] = d[j];
}

template <class F>
struct MvLaunch;
template <>
struct MvLaunch<FqC> {
  using C = G1;
  static constexpr size_t TAB = MV_TAB_G1;
  static void walk(MvWalk w, const uint64_t* in, size_t m, const uint64_t* k, G1X* tab, G1X* out, hipStream_t st) {
    if (w == MV_TABLE) k_g1_mul_scalars<<<ceil_div(m, MV_BLOCK), MV_BLOCK, 0, st>>>(in, m, k, tab, out);
    else k_g1_mul_scalars_plain<<<ceil_div(m, MV_BLOCK), MV_BLOCK, 0, st>>>(in, m, k, out);
  }
};
template <>
struct MvLaunch<Fq2C> {
  using C = G2;
  static constexpr size_t TAB = MV_TAB_G2;
  static void walk(MvWalk w, const uint64_t* in, size_t m, const uint64_t* k, G2X* tab, G2X* out, hipStream_t st) {
    if (w == MV_TABLE) k_g2_mul_scalars<<<ceil_div(m, MV_BLOCK), MV_BLOCK, 0, st>>>(in, m, k, tab, out);
    else k_g2_mul_scalars_plain<<<ceil_div(m, MV_BLOCK), MV_BLOCK, 0, st>>>(in, m, k, out);
  }
};

// The ship rule of DESIGN.md 2.17: the table walk ships where it measured
// faster than the plain per-lane walk at 2^20 points.
template <>
MvWalk mv_shipped<FqC>() { return MV_TABLE; }
template <>
MvWalk mv_shipped<Fq2C>() { return MV_TABLE; }

size_t mv_first_not_below_r(const zk_fr* k, size_t n) {
  for (size_t i = 0; i < n; i++) {
    bool below = false;
    for (int j = 3; j >= 0; j--)
      if (k[i].l[j] != FR_MOD64[j]) {
        below = k[i].l[j] < FR_MOD64[j];
        break;
      }
    if (!below) return i;
  }
  return n;
}

template <class F>
int mv_mul_scalars(zk_ctx* ctx, const void* pts, size_t n, const zk_fr* k_host, const uint64_t* d_k, void* out,
                   MvWalk walk, const char* phase) {
  using Raw = typename GnField<F>::Raw;
  using X = XYZZ<Raw>;
  using A = Affine<Raw>;
  using L = MvLaunch<F>;
  constexpr size_t SZ = 8 * GnField<F>::W;
  if (!n) return ZK_OK;
  hipStream_t st = ctx->stream;
  const size_t chunk = std::min<size_t>(ctx->point_chunk, n);
  DevBuf d_io, d_kc, d_tab, d_x, d_pre, d_aff;
  d_io.ensure(SZ * chunk);
  if (k_host) d_kc.ensure(sizeof(zk_fr) * chunk);
  if (walk == MV_TABLE) d_tab.ensure(sizeof(X) * L::TAB * chunk);
  d_x.ensure(sizeof(X) * chunk);
  d_pre.ensure(sizeof(Raw) * chunk);
  d_aff.ensure(sizeof(A) * chunk);
  for (size_t lo = 0; lo < n; lo += chunk) {
    const size_t m = std::min(chunk, n - lo);
    ZK_HIP(hipMemcpyAsync(d_io.p, static_cast<const char*>(pts) + SZ * lo, SZ * m, hipMemcpyHostToDevice, st));
    const uint64_t* kc = d_k + 4 * lo;
    if (k_host) {
      ZK_HIP(hipMemcpyAsync(d_kc.p, k_host + lo, sizeof(zk_fr) * m, hipMemcpyHostToDevice, st));
      kc = d_kc.as<uint64_t>();
    }
    int pi = ctx->prof.begin(st, phase, m);
    L::walk(walk, d_io.as<uint64_t>(), m, kc, d_tab.as<X>(), d_x.as<X>(), st);
    ZK_LAUNCH_CHECK();
    ctx->prof.end(st, pi);
    pi = ctx->prof.begin(st, "mul_scalars_finish", m);
    batch_normalize<typename L::C>(d_x.as<X>(), m, d_pre.as<Raw>(), d_aff.as<A>(), st);
    gn_points_to_abi<F>(d_aff.as<A>(), m, d_io.as<uint64_t>(), st);
    ctx->prof.end(st, pi);
    ZK_HIP(hipMemcpyAsync(static_cast<char*>(out) + SZ * lo, d_io.p, SZ * m, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));   // the next chunk reuses the buffers
  }
  if (ctx->prof.on) ctx->prof.collect();
  return ZK_OK;
}
template int mv_mul_scalars<FqC>(zk_ctx*, const void*, size_t, const zk_fr*, const uint64_t*, void*, MvWalk,
                                 const char*);
template int mv_mul_scalars<Fq2C>(zk_ctx*, const void*, size_t, const zk_fr*, const uint64_t*, void*, MvWalk,
                                  const char*);

int mv_split_host(zk_ctx* ctx, const zk_fr* k, size_t n, uint64_t* g1_out, uint64_t* g2_out) {
  if (!n) return ZK_OK;
  hipStream_t st = ctx->stream;
  DevBuf d_k, d_1, d_2;
  d_k.ensure(32 * n);
  d_1.ensure(32 * n);
  d_2.ensure(32 * n);
  ZK_HIP(hipMemcpyAsync(d_k.p, k, 32 * n, hipMemcpyHostToDevice, st));
  k_mv_split<<<ceil_div(n, MV_BLOCK), MV_BLOCK, 0, st>>>(d_k.as<uint64_t>(), n, d_1.as<uint64_t>(), d_2.as<uint64_t>());
  ZK_LAUNCH_CHECK();
  if (g1_out) ZK_HIP(hipMemcpyAsync(g1_out, d_1.p, 32 * n, hipMemcpyDeviceToHost, st));
  if (g2_out) ZK_HIP(hipMemcpyAsync(g2_out, d_2.p, 32 * n, hipMemcpyDeviceToHost, st));
  ZK_HIP(hipStreamSynchronize(st));
  return ZK_OK;
}

// the public calls' argument check: every scalar below r
bool mv_scalars_ok(zk_ctx* ctx, const char* name, const zk_fr* k, size_t n) {
  const size_t bad = mv_first_not_below_r(k, n);
  if (bad == n) return true;
  ctx->err = std::string(name) + ": scalar " + std::to_string(bad) + " is not below r";
  return false;
}

}  // namespace zk

using namespace zk;

#define ZK_MGUARD(ctx, ...)                                   \
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

int zk_g1_mul_scalars(zk_ctx* ctx, const zk_g1_affine* pts, size_t n, const zk_fr* k, zk_g1_affine* out) {
  if (!ctx || (n && (!pts || !k || !out))) return ZK_ERR_ARG;
  if (!mv_scalars_ok(ctx, "g1_mul_scalars", k, n)) return ZK_ERR_ARG;
  ZK_MGUARD(ctx, { return mv_mul_scalars<FqC>(ctx, pts, n, k, nullptr, out, mv_shipped<FqC>(), "g1_mul_scalars"); })
}
int zk_g2_mul_scalars(zk_ctx* ctx, const zk_g2_affine* pts, size_t n, const zk_fr* k, zk_g2_affine* out) {
  if (!ctx || (n && (!pts || !k || !out))) return ZK_ERR_ARG;
  if (!mv_scalars_ok(ctx, "g2_mul_scalars", k, n)) return ZK_ERR_ARG;
  ZK_MGUARD(ctx, { return mv_mul_scalars<Fq2C>(ctx, pts, n, k, nullptr, out, mv_shipped<Fq2C>(), "g2_mul_scalars"); })
}
