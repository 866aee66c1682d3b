// srs.hip -- a sound proving key from a powers-of-tau string (include/zkp.h,
// "sound keys from a powers-of-tau string").  No reference
// counterpart: the reference's setup takes the scalars themselves.
//
//   zk_g1_ntt / zk_g2_ntt        the radix-2 transform over group elements
//   zk_groth16_setup_srs_sound   [L_i(tau)] by inverse transforms of the powers,
//                                the key's queries by sparse column sums over
//                                points, h_g1 by differences
//   zk_srs_generate              a string from known secrets (fr_powers and the
//                                sound setup's fixed-base kernel)
//   zk_srs_verify                consistency of a string, from the public MSMs,
//                                the point validation and the host pairing
//
// Transform: log n radix-2 decimation-in-time stages over an XYZZ array that
// stays in HBM, alternating between two arrays (a stage reads one and writes
// the other, so no lane ever reads what another lane of the stage wrote); the
// first stage gathers from bit-reversed positions.  One lane per butterfly
// (u, v) -> (u + w v, u - w v): w v is a double-and-add walk over the bits of
// the canonical twiddle with v left in memory (srs.hpp), skipped for w = 1.
// The array is normalised once at the end (batch_normalize).
#include <algorithm>
#include <cstring>
#include <functional>
#include <vector>

#include "host_pairing.hpp"
#include "prove.hpp"
#include "setup.hpp"
#include "mulvec.hpp"
#include "srs.hpp"

namespace zk {

const char* point_status_text(int st);   // points.hip

// ------------------------------------------------------------- kernels ---
// ABI points -> XYZZ, times s when SCALE (the inverse transform's 1 / n, the
// same in every lane): G1 by ceremony.hpp's endomorphism walk over the lane's
// own output slot, G2 by the plain walk.
template <class F, bool SCALE>
ZK_DI void gn_load_point(const uint64_t* __restrict__ in, size_t n, const CmScalar& s,
                         XYZZ<typename GnField<F>::Raw>* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * GN_BLOCK + threadIdx.x;
  if (i >= n) return;
  Affine<F> P;
  XYZZ<F> acc;
  if (!gn_load_abi(in + GnField<F>::W * i, P)) {
    xyzz_set_inf(acc);
  } else if constexpr (!SCALE) {
    acc = xyzz_from_aff(P);
  } else if constexpr (GnField<F>::W == 13) {
    acc = cm_walk_endo(P, s, &out[i]);
  } else {
    GnScalar g;
    g.w[0] = s.w[0]; g.w[1] = s.w[1]; g.w[2] = s.w[2]; g.w[3] = s.w[3];
    g.top = s.top;
    acc = gn_walk_aff(P, g);
  }
  gn_store(&out[i], acc);
}
__global__ void __launch_bounds__(GN_BLOCK) k_gn_load_g1(const uint64_t* __restrict__ in, size_t n, G1X* __restrict__ out) {
  gn_load_point<FqC, false>(in, n, CmScalar{}, out);
}
__global__ void __launch_bounds__(GN_BLOCK) k_gn_load_g2(const uint64_t* __restrict__ in, size_t n, G2X* __restrict__ out) {
  gn_load_point<Fq2C, false>(in, n, CmScalar{}, out);
}
__global__ void __launch_bounds__(GN_BLOCK) k_gn_load_scale_g1(const uint64_t* __restrict__ in, size_t n, CmScalar s,
                                                               G1X* __restrict__ out) {
  gn_load_point<FqC, true>(in, n, s, out);
}
__global__ void __launch_bounds__(GN_BLOCK) k_gn_load_scale_g2(const uint64_t* __restrict__ in, size_t n, CmScalar s,
                                                               G2X* __restrict__ out) {
  gn_load_point<Fq2C, true>(in, n, s, out);
}

// Stage s (half-size h = 2^s) of the n / 2 butterflies of a transform, src ->
// dst (src != dst).  Butterfly (g, j), g < n / 2h, j < h: elements g 2h + j and
// g 2h + j + h, twiddle w^(j n / 2h) = tw[j << (log_n - 1 - s)], four canonical
// words.  share: lane t takes (g, j) = (t mod n/2h, t div n/2h), so the lanes of
// a wave hold one j wherever n / 2h >= 64 and neither the walk's length nor its
// additions diverge; else (g, j) = (t div h, t mod h), consecutive twiddles.
// The first stage reads bit-reversed positions (its twiddle is 1).
template <class F>
ZK_DI void gn_stage(const XYZZ<typename GnField<F>::Raw>* __restrict__ src,
                    XYZZ<typename GnField<F>::Raw>* __restrict__ dst, uint32_t log_n, uint32_t s,
                    const uint64_t* __restrict__ tw, int share) {
  const uint64_t t = (uint64_t)blockIdx.x * GN_BLOCK + threadIdx.x;
  if (t >= (1ull << (log_n - 1))) return;
  const uint32_t lg = log_n - 1 - s;   // log2 of the butterflies per twiddle
  const uint64_t g = share ? (t & ((1ull << lg) - 1)) : (t >> s);
  const uint64_t j = share ? (t >> lg) : (t & ((1ull << s) - 1));
  const uint64_t i0 = (g << (s + 1)) + j, i1 = i0 + (1ull << s);
  const uint64_t s0 = s == 0 ? bitrev32((uint32_t)i0, log_n) : i0, s1 = s == 0 ? bitrev32((uint32_t)i1, log_n) : i1;
  XYZZ<F> wv;
  if (j == 0) wv = gn_fetch<F>(&src[s1]);
  else wv = gn_walk_mem<F>(&src[s1], gn_scalar(tw + 4 * (j << lg)));
  // w v waits in dst[i1] while u + w v is formed, then comes back negated
  gn_store(&dst[i1], wv);
  gn_store(&dst[i0], gn_add_mem(wv, &src[s0]));
  gn_store(&dst[i1], gn_add_mem(gn_neg(gn_fetch<F>(&dst[i1])), &src[s0]));
}
__global__ void __launch_bounds__(GN_BLOCK) k_gn_stage_g1(const G1X* __restrict__ src, G1X* __restrict__ dst,
                                                          uint32_t log_n, uint32_t s, const uint64_t* __restrict__ tw,
                                                          int share) {
  gn_stage<FqC>(src, dst, log_n, s, tw, share);
}
__global__ void __launch_bounds__(GN_BLOCK) k_gn_stage_g2(const G2X* __restrict__ src, G2X* __restrict__ dst,
                                                          uint32_t log_n, uint32_t s, const uint64_t* __restrict__ tw,
                                                          int share) {
  gn_stage<Fq2C>(src, dst, log_n, s, tw, share);
}

// device affine (Montgomery, (0, 0) = infinity) -> canonical ABI words
ZK_DI void gn_put_fq(uint64_t* w, const Fq& m, bool inf) {
  const Fq c = inf ? fp_zero<FqParams>() : pt_from_mont(m);
#pragma unroll
  for (int k = 0; k < 6; k++) w[k] = (uint64_t)c.v[2 * k] | ((uint64_t)c.v[2 * k + 1] << 32);
}
__global__ void __launch_bounds__(GN_BLOCK) k_gn_to_abi_g1(const G1A* __restrict__ in, size_t n, uint64_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * GN_BLOCK + threadIdx.x;
  if (i >= n) return;
  const G1A a = ld_vec(&in[i]);
  const bool inf = aff_is_inf(a);
  uint64_t* w = out + 13 * i;
  gn_put_fq(w, a.x, inf);
  gn_put_fq(w + 6, a.y, inf);
  w[12] = inf ? 1 : 0;
}
__global__ void __launch_bounds__(GN_BLOCK) k_gn_to_abi_g2(const G2A* __restrict__ in, size_t n, uint64_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * GN_BLOCK + threadIdx.x;
  if (i >= n) return;
  const G2A a = ld_vec(&in[i]);
  const bool inf = aff_is_inf(a);
  uint64_t* w = out + 25 * i;
  gn_put_fq(w, a.x.c0, inf);
  gn_put_fq(w + 6, a.x.c1, inf);
  gn_put_fq(w + 12, a.y.c0, inf);
  gn_put_fq(w + 18, a.y.c1, inf);
  w[24] = inf ? 1 : 0;
}

// Column sums, first level: run k = entries [rb[k], rb[k + 1]) of one column,
// part[k] = sum val_e L[row_e].  val == nullptr: every coefficient is 1.
// Coefficient 1 is a mixed addition, r - 1 one of -L, anything else a walk from
// its top set bit, the sum so far waiting in part[k] meanwhile.
template <class F>
ZK_DI void gn_col_runs(const uint64_t* __restrict__ rb, uint64_t nruns, const uint32_t* __restrict__ row,
                       const uint64_t* __restrict__ val, const Affine<typename GnField<F>::Raw>* __restrict__ L,
                       XYZZ<typename GnField<F>::Raw>* __restrict__ part) {
  const uint64_t k = (uint64_t)blockIdx.x * GN_BLOCK + threadIdx.x;
  if (k >= nruns) return;
  XYZZ<F> acc;
  xyzz_set_inf(acc);
#pragma unroll 1
  for (uint64_t e = rb[k]; e < rb[k + 1]; e++) {
    Affine<F> P;
    if (!gn_fetch_aff(&L[row[e]], P)) continue;
    bool unit = true;
    if (val) {
      const GnScalar c = gn_scalar(val + 4 * e);
      if (c.top == 0) continue;
      if (c.w[0] == FR_MOD64[0] - 1 && c.w[1] == FR_MOD64[1] && c.w[2] == FR_MOD64[2] && c.w[3] == FR_MOD64[3]) {
        P.y = f_neg(P.y);
      } else if (c.top > 1) {
        unit = false;
        gn_store(&part[k], acc);
        acc = gn_add_mem(gn_walk_aff(P, c), &part[k]);
      }
    }
    if (unit) acc = xyzz_madd(acc, P);
  }
  gn_store(&part[k], acc);
}
// second level: out[j] = sum of column j's runs part[cfr[j] .. cfr[j + 1])
template <class F>
ZK_DI void gn_col_cols(const uint64_t* __restrict__ cfr, uint64_t V,
                       const XYZZ<typename GnField<F>::Raw>* __restrict__ part,
                       XYZZ<typename GnField<F>::Raw>* __restrict__ out) {
  const uint64_t j = (uint64_t)blockIdx.x * GN_BLOCK + threadIdx.x;
  if (j >= V) return;
  XYZZ<F> acc;
  xyzz_set_inf(acc);
#pragma unroll 1
  for (uint64_t k = cfr[j]; k < cfr[j + 1]; k++) acc = gn_add_mem(acc, &part[k]);
  gn_store(&out[j], acc);
}
__global__ void __launch_bounds__(GN_BLOCK) k_gn_col_runs_g1(const uint64_t* __restrict__ rb, uint64_t nruns,
                                                             const uint32_t* __restrict__ row,
                                                             const uint64_t* __restrict__ val,
                                                             const G1A* __restrict__ L, G1X* __restrict__ part) {
  gn_col_runs<FqC>(rb, nruns, row, val, L, part);
}
__global__ void __launch_bounds__(GN_BLOCK) k_gn_col_runs_g2(const uint64_t* __restrict__ rb, uint64_t nruns,
                                                             const uint32_t* __restrict__ row,
                                                             const uint64_t* __restrict__ val,
                                                             const G2A* __restrict__ L, G2X* __restrict__ part) {
  gn_col_runs<Fq2C>(rb, nruns, row, val, L, part);
}
__global__ void __launch_bounds__(GN_BLOCK) k_gn_col_cols_g1(const uint64_t* __restrict__ cfr, uint64_t V,
                                                             const G1X* __restrict__ part, G1X* __restrict__ out) {
  gn_col_cols<FqC>(cfr, V, part, out);
}
__global__ void __launch_bounds__(GN_BLOCK) k_gn_col_cols_g2(const uint64_t* __restrict__ cfr, uint64_t V,
                                                             const G2X* __restrict__ part, G2X* __restrict__ out) {
  gn_col_cols<Fq2C>(cfr, V, part, out);
}

// out[i] = pts[i + n] - pts[i], i < n (ABI points): h_g1[i] = [tau^i (tau^n - 1)]_1
__global__ void __launch_bounds__(GN_BLOCK) k_gn_hdiff(const uint64_t* __restrict__ pts, size_t n, G1X* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * GN_BLOCK + threadIdx.x;
  if (i >= n) return;
  Affine<FqC> P, Q;
  XYZZ<FqC> acc;
  xyzz_set_inf(acc);
  if (gn_load_abi(pts + 13 * (i + n), P)) acc = xyzz_from_aff(P);
  if (gn_load_abi(pts + 13 * i, Q)) acc = xyzz_madd(acc, aff_neg(Q));
  gn_store(&out[i], acc);
}

// ------------------------------------------------------------- helpers ---
template <class F>
struct GnLaunch;
template <>
struct GnLaunch<FqC> {
  static void load(const uint64_t* in, size_t n, const CmScalar* s, G1X* out, hipStream_t st) {
    if (s) k_gn_load_scale_g1<<<ceil_div(n, GN_BLOCK), GN_BLOCK, 0, st>>>(in, n, *s, out);
    else k_gn_load_g1<<<ceil_div(n, GN_BLOCK), GN_BLOCK, 0, st>>>(in, n, out);
  }
  static void stage(const G1X* src, G1X* dst, uint32_t log_n, uint32_t s, const uint64_t* tw, int share, hipStream_t st) {
    k_gn_stage_g1<<<ceil_div(1ull << (log_n - 1), GN_BLOCK), GN_BLOCK, 0, st>>>(src, dst, log_n, s, tw, share);
  }
  static void to_abi(const G1A* in, size_t n, uint64_t* out, hipStream_t st) {
    k_gn_to_abi_g1<<<ceil_div(n, GN_BLOCK), GN_BLOCK, 0, st>>>(in, n, out);
  }
  static void col_runs(const uint64_t* rb, uint64_t nruns, const uint32_t* row, const uint64_t* val, const G1A* L,
                       G1X* part, hipStream_t st) {
    k_gn_col_runs_g1<<<ceil_div(nruns, GN_BLOCK), GN_BLOCK, 0, st>>>(rb, nruns, row, val, L, part);
  }
  static void col_cols(const uint64_t* cfr, uint64_t V, const G1X* part, G1X* out, hipStream_t st) {
    k_gn_col_cols_g1<<<ceil_div(V, GN_BLOCK), GN_BLOCK, 0, st>>>(cfr, V, part, out);
  }
};
template <>
struct GnLaunch<Fq2C> {
  static void load(const uint64_t* in, size_t n, const CmScalar* s, G2X* out, hipStream_t st) {
    if (s) k_gn_load_scale_g2<<<ceil_div(n, GN_BLOCK), GN_BLOCK, 0, st>>>(in, n, *s, out);
    else k_gn_load_g2<<<ceil_div(n, GN_BLOCK), GN_BLOCK, 0, st>>>(in, n, out);
  }
  static void stage(const G2X* src, G2X* dst, uint32_t log_n, uint32_t s, const uint64_t* tw, int share, hipStream_t st) {
    k_gn_stage_g2<<<ceil_div(1ull << (log_n - 1), GN_BLOCK), GN_BLOCK, 0, st>>>(src, dst, log_n, s, tw, share);
  }
  static void to_abi(const G2A* in, size_t n, uint64_t* out, hipStream_t st) {
    k_gn_to_abi_g2<<<ceil_div(n, GN_BLOCK), GN_BLOCK, 0, st>>>(in, n, out);
  }
  static void col_runs(const uint64_t* rb, uint64_t nruns, const uint32_t* row, const uint64_t* val, const G2A* L,
                       G2X* part, hipStream_t st) {
    k_gn_col_runs_g2<<<ceil_div(nruns, GN_BLOCK), GN_BLOCK, 0, st>>>(rb, nruns, row, val, L, part);
  }
  static void col_cols(const uint64_t* cfr, uint64_t V, const G2X* part, G2X* out, hipStream_t st) {
    k_gn_col_cols_g2<<<ceil_div(V, GN_BLOCK), GN_BLOCK, 0, st>>>(cfr, V, part, out);
  }
};

template <class F>
void gn_points_to_abi(const Affine<typename GnField<F>::Raw>* d_in, size_t n, uint64_t* d_out, hipStream_t st) {
  GnLaunch<F>::to_abi(d_in, n, d_out, st);
  ZK_LAUNCH_CHECK();
}
template void gn_points_to_abi<FqC>(const G1A*, size_t, uint64_t*, hipStream_t);
template void gn_points_to_abi<Fq2C>(const G2A*, size_t, uint64_t*, hipStream_t);

static Fr fr_words(const uint32_t (&c)[8]) {
  Fr a;
  for (int i = 0; i < 8; i++) a.v[i] = c[i];
  return a;
}

template <class F>
void gntt_device(zk_ctx* ctx, const uint64_t* d_abi, uint32_t log_n, bool inverse,
                 Affine<typename GnField<F>::Raw>* d_out, const char* phase) {
  using Raw = typename GnField<F>::Raw;
  using C = typename GnField<F>::C;
  using X = XYZZ<Raw>;
  hipStream_t st = ctx->stream;
  const size_t n = (size_t)1 << log_n;
  DevBuf a, b, tw, pre;
  a.ensure(sizeof(X) * n);
  const int pi = ctx->prof.begin(st, phase, n);
  CmScalar ninv;
  const bool scale = inverse && log_n > 0;
  if (scale) {
    zk_fr k;
    host::fr_from_mont(host::fr_inv(host::fr_from_u64((uint64_t)n)), k.l);
    // G1: the endomorphism walk's two halves; G2: the plain walk's four words
    const bool ok = GnField<F>::W == 13 ? cm_split_scalar(k, ninv) : cm_plain_scalar(k, ninv);
    if (!ok) throw Error(ZK_ERR_ARG, "group transform: 1 / n is not below r");
  }
  GnLaunch<F>::load(d_abi, n, scale ? &ninv : nullptr, a.as<X>(), st);
  ZK_LAUNCH_CHECK();
  X *src = a.as<X>(), *dst = nullptr;
  if (log_n > 0) {
    b.ensure(sizeof(X) * n);
    dst = b.as<X>();
    // tw[j] = w^(+-j), j < n / 2, as canonical words
    tw.ensure(sizeof(Fr) * (n / 2));
    fr_powers(tw.as<Fr>(), fr_words(inverse ? FR_ROOTS_INV[log_n] : FR_ROOTS[log_n]), fr_words(FrParams::ONE), n / 2, st);
    fr_from_mont(tw.as<Fr>(), tw.as<uint64_t>(), n / 2, st);
  }
  for (uint32_t s = 0; s < log_n; s++) {
    const int share = ctx->gntt_map != 0 && (log_n - 1 - s) >= 6;
    GnLaunch<F>::stage(src, dst, log_n, s, tw.as<uint64_t>(), share, st);
    ZK_LAUNCH_CHECK();
    std::swap(src, dst);
  }
  pre.ensure(sizeof(Raw) * n);
  batch_normalize<C>(src, n, pre.as<Raw>(), d_out, st);
  ctx->prof.end(st, pi);
  ZK_HIP(hipStreamSynchronize(st));   // the call's buffers die here
}

// host array <-> device, in pieces of ctx->point_chunk points
void chunked_copy(zk_ctx* ctx, void* dst, const void* src, size_t n, size_t sz, hipMemcpyKind kind) {
  const size_t chunk = std::max<size_t>(ctx->point_chunk, 1);
  for (size_t lo = 0; lo < n; lo += chunk) {
    const size_t m = std::min(chunk, n - lo);
    ZK_HIP(hipMemcpyAsync(static_cast<char*>(dst) + sz * lo, static_cast<const char*>(src) + sz * lo, sz * m, kind,
                          ctx->stream));
  }
}

// n device affine points -> canonical ABI words in host memory
template <class F>
void affine_to_host(zk_ctx* ctx, const Affine<typename GnField<F>::Raw>* d_in, size_t n, void* host_out) {
  if (!n) return;
  constexpr size_t SZ = 8 * GnField<F>::W;
  DevBuf w;
  w.ensure(SZ * n);
  GnLaunch<F>::to_abi(d_in, n, w.as<uint64_t>(), ctx->stream);
  ZK_LAUNCH_CHECK();
  chunked_copy(ctx, host_out, w.p, n, SZ, hipMemcpyDeviceToHost);
  ZK_HIP(hipStreamSynchronize(ctx->stream));
}
template void affine_to_host<FqC>(zk_ctx*, const G1A*, size_t, void*);
template void affine_to_host<Fq2C>(zk_ctx*, const G2A*, size_t, void*);

template <class F, class ABI>
static int gntt_host(zk_ctx* ctx, ABI* pts, uint32_t log_n, int dir) {
  static_assert(sizeof(ABI) == 8 * GnField<F>::W, "ABI point layout");
  using A = Affine<typename GnField<F>::Raw>;
  const size_t n = (size_t)1 << log_n;
  DevBuf d_abi, d_aff;
  d_abi.ensure(sizeof(ABI) * n);
  d_aff.ensure(sizeof(A) * n);
  chunked_copy(ctx, d_abi.p, pts, n, sizeof(ABI), hipMemcpyHostToDevice);
  gntt_device<F>(ctx, d_abi.as<uint64_t>(), log_n, dir < 0, d_aff.as<A>(), GnField<F>::W == 13 ? "g1_ntt" : "g2_ntt");
  affine_to_host<F>(ctx, d_aff.as<A>(), n, pts);
  if (ctx->prof.on) ctx->prof.collect();
  return ZK_OK;
}

// out[j] = sum over column j of val_e L[row_e], j < V, as device affine points
// handed to sink, which returns with the stream idle (the host vectors and the
// buffers die after it).  cp / row / cval: the matrix in CSC (cval empty: all
// ones).
template <class F>
static void colsum_points(zk_ctx* ctx, uint64_t V, const std::vector<uint64_t>& cp, const std::vector<uint32_t>& row,
                          const std::vector<zk_fr>& cval, bool unit, const Affine<typename GnField<F>::Raw>* d_L,
                          const char* phase, const std::function<void(const void*)>& sink) {
  using Raw = typename GnField<F>::Raw;
  using X = XYZZ<Raw>;
  using A = Affine<Raw>;
  hipStream_t st = ctx->stream;
  const uint64_t nnz = cp[V];
  uint64_t run = ctx->srs_run;
  if (!run) {
    uint64_t longest = 0;
    for (uint64_t j = 0; j < V; j++) longest = std::max(longest, cp[j + 1] - cp[j]);
    for (run = SRS_RUN_MIN; run * run < longest; run <<= 1) {}
  }
  // every column cut into runs of at most `run` entries
  std::vector<uint64_t> rb, cfr(V + 1);
  for (uint64_t j = 0; j < V; j++) {
    cfr[j] = rb.size();
    for (uint64_t e = cp[j]; e < cp[j + 1]; e += run) rb.push_back(e);
  }
  cfr[V] = rb.size();
  const uint64_t nruns = rb.size();
  rb.push_back(nnz);
  DevBuf d_rb, d_cfr, d_row, d_val, d_part, d_out, d_pre, d_aff;
  d_rb.ensure(8 * rb.size());
  d_cfr.ensure(8 * cfr.size());
  d_row.ensure(4 * std::max<uint64_t>(nnz, 1));
  ZK_HIP(hipMemcpyAsync(d_rb.p, rb.data(), 8 * rb.size(), hipMemcpyHostToDevice, st));
  ZK_HIP(hipMemcpyAsync(d_cfr.p, cfr.data(), 8 * cfr.size(), hipMemcpyHostToDevice, st));
  if (nnz) ZK_HIP(hipMemcpyAsync(d_row.p, row.data(), 4 * nnz, hipMemcpyHostToDevice, st));
  if (!unit && nnz) {
    d_val.ensure(sizeof(zk_fr) * nnz);
    ZK_HIP(hipMemcpyAsync(d_val.p, cval.data(), sizeof(zk_fr) * nnz, hipMemcpyHostToDevice, st));
  }
  d_part.ensure(sizeof(X) * std::max<uint64_t>(nruns, 1));
  d_out.ensure(sizeof(X) * V);
  d_pre.ensure(sizeof(Raw) * V);
  d_aff.ensure(sizeof(A) * V);
  const int pi = ctx->prof.begin(st, phase, nnz);
  if (nruns) {
    GnLaunch<F>::col_runs(d_rb.as<uint64_t>(), nruns, d_row.as<uint32_t>(), unit ? nullptr : d_val.as<uint64_t>(), d_L,
                          d_part.as<X>(), st);
    ZK_LAUNCH_CHECK();
  }
  GnLaunch<F>::col_cols(d_cfr.as<uint64_t>(), V, d_part.as<X>(), d_out.as<X>(), st);
  ZK_LAUNCH_CHECK();
  batch_normalize<typename GnField<F>::C>(d_out.as<X>(), V, d_pre.as<Raw>(), d_aff.as<A>(), st);
  ctx->prof.end(st, pi);
  sink(d_aff.p);
}

bool same_g1(const zk_g1_affine& a, const zk_g1_affine& b) {
  return !std::memcmp(a.x, b.x, 48) && !std::memcmp(a.y, b.y, 48) && a.infinity == b.infinity;
}
bool same_g2(const zk_g2_affine& a, const zk_g2_affine& b) {
  return !std::memcmp(a.x, b.x, 96) && !std::memcmp(a.y, b.y, 96) && a.infinity == b.infinity;
}
static bool fr_is0(const zk_fr& a) { return (a.l[0] | a.l[1] | a.l[2] | a.l[3]) == 0; }

// the generators as ABI points, through the fixed-base kernel
void generators(zk_ctx* ctx, zk_g1_affine& g1, zk_g2_affine& g2) {
  const zk_fr one = {{1, 0, 0, 0}};
  std::memset(&g1, 0, sizeof g1);
  std::memset(&g2, 0, sizeof g2);
  if (fixed_base_wide_host(ctx, false, &one, 1, reinterpret_cast<uint64_t*>(&g1)) != ZK_OK ||
      fixed_base_wide_host(ctx, true, &one, 1, reinterpret_cast<uint64_t*>(&g2)) != ZK_OK)
    throw Error(ZK_ERR_DEVICE, "generators: the fixed-base kernel refused the scalar 1");
}

// ------------------------------------------------------------ the key ---
// The halves of zk_groth16_setup_srs_sound, shared with the prepared strings
// (lagrange.hip).  Upper half, circuit-independent:
void srs_lagrange_transforms(zk_ctx* ctx, const zk_srs* srs, uint32_t log_n, void* d_abi, G1A* L1, G2A* L2) {
  const uint64_t n = 1ull << log_n;
  const zk_g1_affine* g1src[3] = {srs->tau_g1, srs->alpha_tau_g1, srs->beta_tau_g1};
  const char* g1name[3] = {"srs_ntt_g1_tau", "srs_ntt_g1_alpha", "srs_ntt_g1_beta"};
  for (int k = 0; k < 3; k++) {
    chunked_copy(ctx, d_abi, g1src[k], n, sizeof(zk_g1_affine), hipMemcpyHostToDevice);
    gntt_device<FqC>(ctx, static_cast<const uint64_t*>(d_abi), log_n, true, L1 + k * n, g1name[k]);
  }
  chunked_copy(ctx, d_abi, srs->tau_g2, n, sizeof(zk_g2_affine), hipMemcpyHostToDevice);
  gntt_device<Fq2C>(ctx, static_cast<const uint64_t*>(d_abi), log_n, true, L2, "srs_ntt_g2");
}

void srs_hdiff(zk_ctx* ctx, const zk_g1_affine* tau_g1, uint64_t n, void* d_abi, G1A* d_out) {
  hipStream_t st = ctx->stream;
  DevBuf d_x, d_pre;
  d_x.ensure(sizeof(G1X) * n);
  d_pre.ensure(sizeof(Fq) * n);
  chunked_copy(ctx, d_abi, tau_g1, 2 * n, sizeof(zk_g1_affine), hipMemcpyHostToDevice);
  const int pi = ctx->prof.begin(st, "srs_hdiff", n);
  k_gn_hdiff<<<ceil_div(n, GN_BLOCK), GN_BLOCK, 0, st>>>(static_cast<const uint64_t*>(d_abi), n, d_x.as<G1X>());
  ZK_LAUNCH_CHECK();
  batch_normalize<G1>(d_x.as<G1X>(), n, d_pre.as<Fq>(), d_out, st);
  ctx->prof.end(st, pi);
  ZK_HIP(hipStreamSynchronize(st));   // d_x / d_pre die here
}

// Lower half: the four column sums of the circuit over the Lagrange points.
void srs_column_sums(zk_ctx* ctx, const zk_r1cs_csr* q, uint64_t n, const G1A* L1, const G2A* L2,
                     const SrsSumSink& sink) {
  const uint64_t V = q->num_variables, nc = q->num_constraints;
  {
    std::vector<uint64_t> cp;
    std::vector<uint32_t> row;
    std::vector<zk_fr> cval;
    {
      HostPhase hp(ctx->prof, "srs_csc_host");
      csr_to_csc(nc, V, q->a_rowptr, q->a_col, q->a_val, cp, row, cval);
    }
    colsum_points<FqC>(ctx, V, cp, row, cval, !q->a_val, L1, "srs_colsum_a_g1",
                       [&](const void* d) { sink(SRS_SUM_A, d); });
    {
      HostPhase hp(ctx->prof, "srs_csc_host");
      csr_to_csc(nc, V, q->b_rowptr, q->b_col, q->b_val, cp, row, cval);
    }
    colsum_points<FqC>(ctx, V, cp, row, cval, !q->b_val, L1, "srs_colsum_b_g1",
                       [&](const void* d) { sink(SRS_SUM_B1, d); });
    colsum_points<Fq2C>(ctx, V, cp, row, cval, !q->b_val, L2, "srs_colsum_b_g2",
                        [&](const void* d) { sink(SRS_SUM_B2, d); });
  }
  {
    // ic: one matrix of 3 n rows over [L | alpha L | beta L] -- C's rows, then
    // B's from n, then A's from 2 n
    const uint64_t* rps[3] = {q->c_rowptr, q->b_rowptr, q->a_rowptr};
    const uint32_t* cols[3] = {q->c_col, q->b_col, q->a_col};
    const zk_fr* vals[3] = {q->c_val, q->b_val, q->a_val};
    const bool unit = !vals[0] && !vals[1] && !vals[2];
    std::vector<uint64_t> cp;
    std::vector<uint32_t> row;
    std::vector<zk_fr> cval;
    {
      HostPhase hp(ctx->prof, "srs_csc_host");
      std::vector<uint64_t> rp(3 * n + 1, 0);
      std::vector<uint32_t> col;
      std::vector<zk_fr> val;
      const zk_fr one = {{1, 0, 0, 0}};
      for (int m = 0; m < 3; m++) {
        const uint64_t nnz = nc ? rps[m][nc] : 0;
        for (uint64_t i = 0; i < n; i++) rp[m * n + i + 1] = col.size() + (nc ? rps[m][std::min(i + 1, nc)] : 0);
        col.insert(col.end(), cols[m], cols[m] + nnz);
        if (!unit) {
          if (vals[m]) val.insert(val.end(), vals[m], vals[m] + nnz);
          else val.insert(val.end(), nnz, one);
        }
      }
      csr_to_csc(3 * n, V, rp.data(), col.data(), unit ? nullptr : val.data(), cp, row, cval);
    }
    colsum_points<FqC>(ctx, V, cp, row, cval, unit, L1, "srs_colsum_ic", [&](const void* d) { sink(SRS_SUM_IC, d); });
  }
}

// the fixed points and lengths of a key from a string (delta = gamma = 1)
void srs_key_header(const zk_g1_affine& alpha_g1, const zk_g1_affine& beta_g1, const zk_g2_affine& beta_g2,
                    const zk_g1_affine& g1, const zk_g2_affine& g2, uint64_t V, uint64_t n, uint64_t num_public,
                    zk_pk* pk, zk_vk* vk) {
  if (vk) {
    vk->alpha_g1 = alpha_g1;
    vk->beta_g2 = beta_g2;
    vk->gamma_g2 = g2;
    vk->delta_g2 = g2;
    vk->num_public = num_public;
    vk->ic_len = num_public + 1;
  }
  if (pk) {
    pk->alpha_g1 = alpha_g1;
    pk->beta_g1 = beta_g1;
    pk->delta_g1 = g1;
    pk->beta_g2 = beta_g2;
    pk->delta_g2 = g2;
    pk->num_public = num_public;
    pk->a_len = V;
    pk->b_len = V;
    pk->b2_len = V;
    pk->ic_len = V - num_public - 1;
    pk->h_len = n;
  }
}

void SrsHostKey::take(zk_ctx* ctx, int which, const void* d) {
  if (which == SRS_SUM_B2) {
    affine_to_host<Fq2C>(ctx, static_cast<const G2A*>(d), b2.size(), b2.data());
    return;
  }
  std::vector<zk_g1_affine>& out = which == SRS_SUM_A ? a1 : which == SRS_SUM_B1 ? b1 : ic;
  affine_to_host<FqC>(ctx, static_cast<const G1A*>(d), out.size(), out.data());
}
void SrsHostKey::fill(const zk_g1_affine& alpha_g1, const zk_g1_affine& beta_g1, const zk_g2_affine& beta_g2,
                      const zk_g1_affine& g1, const zk_g2_affine& g2, uint64_t num_public, zk_pk* pk, zk_vk* vk) const {
  const uint64_t V = a1.size(), n = h.size(), nic = V - num_public - 1, nvk = num_public + 1;
  srs_key_header(alpha_g1, beta_g1, beta_g2, g1, g2, V, n, num_public, pk, vk);
  if (vk) std::memcpy(vk->ic_g1, ic.data(), sizeof(zk_g1_affine) * nvk);
  std::memcpy(pk->a_g1, a1.data(), sizeof(zk_g1_affine) * V);
  std::memcpy(pk->b_g1, b1.data(), sizeof(zk_g1_affine) * V);
  std::memcpy(pk->b_g2, b2.data(), sizeof(zk_g2_affine) * V);
  if (nic) std::memcpy(pk->ic_g1, ic.data() + nvk, sizeof(zk_g1_affine) * nic);
  std::memcpy(pk->h_g1, h.data(), sizeof(zk_g1_affine) * n);
}

static int setup_srs(zk_ctx* ctx, const zk_r1cs_csr* q, const zk_srs* srs, uint64_t num_public, zk_pk* pk, zk_vk* vk) {
  Range range("zk_setup_srs");
  const uint64_t V = q->num_variables, nc = q->num_constraints;
  if (num_public >= V) return ZK_ERR_SETUP_PARAMS;
  if (nc > (1ull << 32) || srs->log_n > 31) return ZK_ERR_DOMAIN;
  uint64_t n = 1;
  while (n < nc) n <<= 1;
  const uint32_t log_n = (uint32_t)__builtin_ctzll(n);
  const uint64_t N = 1ull << srs->log_n;
  if (n > N || srs->tau_g1_len < 2 * N || srs->tau_g2_len < N || srs->alpha_len < N || srs->beta_len < N) {
    ctx->err = "setup from a string: the circuit's domain is " + std::to_string(n) + ", the string serves " +
               std::to_string(N) + " (or its arrays are shorter than log_n states)";
    return ZK_ERR_DOMAIN;
  }
  // three blocks of n rows in one u32 index (the mixed ic sum)
  if (V >= 0x80000000ull || n > 0x40000000ull) return ZK_ERR_ARG;
  if (same_g1(srs->tau_g1[n], srs->tau_g1[0])) {
    ctx->err = "sound setup: tau lies on the evaluation domain (Z(tau) = 0)";
    return ZK_ERR_SETUP_PARAMS;
  }

  // ---- [L_i]_1, [alpha L_i]_1, [beta L_i]_1 back to back, and [L_i]_2 ----
  DevBuf d_abi, L1, L2;
  d_abi.ensure(std::max(sizeof(zk_g1_affine) * 2 * n, sizeof(zk_g2_affine) * n));
  L1.ensure(sizeof(G1A) * 3 * n);
  L2.ensure(sizeof(G2A) * n);
  srs_lagrange_transforms(ctx, srs, log_n, d_abi.p, L1.as<G1A>(), L2.as<G2A>());

  // ---- everything into scratch: the keys change only once nothing can fail ----
  SrsHostKey key(V, n);
  srs_column_sums(ctx, q, n, L1.as<G1A>(), L2.as<G2A>(), [&](int which, const void* d) { key.take(ctx, which, d); });
  {
    DevBuf d_aff;
    d_aff.ensure(sizeof(G1A) * n);
    srs_hdiff(ctx, srs->tau_g1, n, d_abi.p, d_aff.as<G1A>());
    affine_to_host<FqC>(ctx, d_aff.as<G1A>(), n, key.h.data());
  }
  zk_g1_affine g1;
  zk_g2_affine g2;
  generators(ctx, g1, g2);
  if (ctx->prof.on) ctx->prof.collect();
  key.fill(srs->alpha_tau_g1[0], srs->beta_tau_g1[0], srs->beta_g2, g1, g2, num_public, pk, vk);
  return ZK_OK;
}

// ---------------------------------------------------------- the string ---
// out[i] = [scale tau^i]_g, i < cnt
static int powers_to_points(zk_ctx* ctx, bool g2, const host::Fr& tau, const host::Fr& scale, size_t cnt, void* out) {
  hipStream_t st = ctx->stream;
  DevBuf tp;
  tp.ensure(sizeof(Fr) * cnt);
  Fr t, s;
  const host::Fr td = host::fr_to_dev(tau), sd = host::fr_to_dev(scale);
  std::memcpy(t.v, td.l, 32);
  std::memcpy(s.v, sd.l, 32);
  fr_powers(tp.as<Fr>(), t, s, cnt, st);
  fr_from_mont(tp.as<Fr>(), tp.as<uint64_t>(), cnt, st);
  std::vector<zk_fr> sc(cnt);
  ZK_HIP(hipMemcpyAsync(sc.data(), tp.p, sizeof(zk_fr) * cnt, hipMemcpyDeviceToHost, st));
  ZK_HIP(hipStreamSynchronize(st));
  return fixed_base_wide_host(ctx, g2, sc.data(), cnt, static_cast<uint64_t*>(out));
}

static int srs_generate(zk_ctx* ctx, uint32_t log_n, const zk_fr* tau, const zk_fr* alpha, const zk_fr* beta,
                        zk_srs* out) {
  const size_t N = (size_t)1 << log_n;
  const host::Fr t = host::fr_to_mont(tau->l), a = host::fr_to_mont(alpha->l), b = host::fr_to_mont(beta->l);
  int rc = powers_to_points(ctx, false, t, host::fr_one(), 2 * N, out->tau_g1);
  if (rc == ZK_OK) rc = powers_to_points(ctx, true, t, host::fr_one(), N, out->tau_g2);
  if (rc == ZK_OK) rc = powers_to_points(ctx, false, t, a, N, out->alpha_tau_g1);
  if (rc == ZK_OK) rc = powers_to_points(ctx, false, t, b, N, out->beta_tau_g1);
  std::memset(&out->beta_g2, 0, sizeof out->beta_g2);
  if (rc == ZK_OK) rc = fixed_base_wide_host(ctx, true, beta, 1, reinterpret_cast<uint64_t*>(&out->beta_g2));
  if (rc != ZK_OK) return rc;
  out->log_n = log_n;
  out->tau_g1_len = 2 * N;
  out->tau_g2_len = N;
  out->alpha_len = N;
  out->beta_len = N;
  return ZK_OK;
}

// ------------------------------------------------------------- verify ---
// One array through the point validation; the identity is refused too.  true
// when every entry is valid; rc: ZK_OK or the call's own failure.
template <class P>
bool srs_valid(zk_ctx* ctx, const char* name, const P* pts, size_t n, int& rc) {
  std::vector<uint8_t> st(n);
  size_t bad = n;
  if constexpr (sizeof(P) == sizeof(zk_g1_affine)) rc = zk_g1_validate(ctx, pts, n, st.data(), &bad);
  else rc = zk_g2_validate(ctx, pts, n, st.data(), &bad);
  if (rc != ZK_OK) {
    if (rc != ZK_ERR_ARG || bad >= n) return false;
    rc = ZK_OK;
    ctx->err = std::string(name) + "[" + std::to_string(bad) + "]: " + point_status_text(st[bad]);
    return false;
  }
  for (size_t i = 0; i < n; i++)
    if (pts[i].infinity) {
      ctx->err = std::string(name) + "[" + std::to_string(i) + "]: the identity";
      return false;
    }
  return true;
}
template bool srs_valid<zk_g1_affine>(zk_ctx*, const char*, const zk_g1_affine*, size_t, int&);
template bool srs_valid<zk_g2_affine>(zk_ctx*, const char*, const zk_g2_affine*, size_t, int&);
static bool negated_g1(const zk_g1_affine& p, zk_g1_affine& out) {
  host::A1 a;
  if (!host::load(p, a)) return false;
  out = p;
  if (!a.inf) {
    const host::Fq c = host::from_mont(host::neg(a.y));
    std::memcpy(out.y, c.l, 48);
  }
  return true;
}
// e(a, p) == e(b, q)
bool pairs_equal(const zk_g1_affine& a, const zk_g2_affine& p, const zk_g1_affine& b, const zk_g2_affine& q) {
  zk_g1_affine g1[2];
  zk_g2_affine g2[2] = {p, q};
  int one = 0;
  g1[0] = a;
  if (!negated_g1(b, g1[1]) || zk_pairing_product_is_one(g1, g2, 2, &one) != ZK_OK) return false;
  return one != 0;
}

static int srs_verify(zk_ctx* ctx, const zk_srs* s, const zk_fr* rho, int* status) {
  const size_t N = (size_t)1 << s->log_n;
  int rc = ZK_OK;
  *status = ZK_SRS_POINT;
  if (!srs_valid(ctx, "tau_g1", s->tau_g1, 2 * N, rc) || !srs_valid(ctx, "tau_g2", s->tau_g2, N, rc) ||
      !srs_valid(ctx, "alpha_tau_g1", s->alpha_tau_g1, N, rc) || !srs_valid(ctx, "beta_tau_g1", s->beta_tau_g1, N, rc) ||
      !srs_valid(ctx, "beta_g2", &s->beta_g2, 1, rc))
    return rc;
  *status = ZK_SRS_GENERATOR;
  zk_g1_affine g1;
  zk_g2_affine g2;
  generators(ctx, g1, g2);
  if (!same_g1(s->tau_g1[0], g1) || !same_g2(s->tau_g2[0], g2)) return ZK_OK;

  zk_g1_affine lo1, hi1, sa, sb;
  zk_g2_affine lo2, hi2, sn;
  // (a string for N = 1 holds no tau_g2[1]: its tau_g1[1] cannot be checked)
  *status = ZK_SRS_POWERS_G1;
  if (N > 1) {
    if ((rc = zk_msm_g1(ctx, s->tau_g1, 2 * N - 1, rho, 2 * N - 1, 255, &lo1)) != ZK_OK ||
        (rc = zk_msm_g1(ctx, s->tau_g1 + 1, 2 * N - 1, rho, 2 * N - 1, 255, &hi1)) != ZK_OK)
      return rc;
    if (!pairs_equal(hi1, g2, lo1, s->tau_g2[1])) return ZK_OK;
  }
  *status = ZK_SRS_POWERS_G2;
  if (N > 1) {
    if ((rc = zk_msm_g2(ctx, s->tau_g2, N - 1, rho, N - 1, 255, &lo2)) != ZK_OK ||
        (rc = zk_msm_g2(ctx, s->tau_g2 + 1, N - 1, rho, N - 1, 255, &hi2)) != ZK_OK)
      return rc;
    if (!pairs_equal(s->tau_g1[1], lo2, g1, hi2)) return ZK_OK;
  }
  if ((rc = zk_msm_g2(ctx, s->tau_g2, N, rho, N, 255, &sn)) != ZK_OK) return rc;
  *status = ZK_SRS_ALPHA;
  if ((rc = zk_msm_g1(ctx, s->alpha_tau_g1, N, rho, N, 255, &sa)) != ZK_OK) return rc;
  if (!pairs_equal(sa, g2, s->alpha_tau_g1[0], sn)) return ZK_OK;
  *status = ZK_SRS_BETA;
  if ((rc = zk_msm_g1(ctx, s->beta_tau_g1, N, rho, N, 255, &sb)) != ZK_OK) return rc;
  if (!pairs_equal(sb, g2, s->beta_tau_g1[0], sn)) return ZK_OK;
  if (!pairs_equal(s->beta_tau_g1[0], g2, g1, s->beta_g2)) return ZK_OK;
  *status = ZK_SRS_OK;
  return ZK_OK;
}

// ------------------------------------------------------- contribution ---
static bool fr_share_ok(const zk_fr& a) { return !fr_is0(a) && fr_canonical(a); }
// k P through the host curve code, as canonical ABI words
static zk_g2_affine host_mul_g2(const host::A2& p, const zk_fr& k) {
  zk_g2_affine out;
  std::memset(&out, 0, sizeof out);
  host_to_abi<G2>(host::mul_scalar(host::from_affine(p.x, p.y, p.inf), k.l), reinterpret_cast<uint64_t*>(&out));
  return out;
}

// Entry i of every array times s^i (times a, b for the alpha and beta
// arrays): the scalars are geometric progressions made on the device
// (fr_powers) and handed to mulvec.hpp's walks as a device array.
static int srs_contribute(zk_ctx* ctx, zk_srs* srs, const zk_fr* s, const zk_fr* a, const zk_fr* b,
                          zk_srs_share* share) {
  Range range("zk_srs_contribute");
  hipStream_t st = ctx->stream;
  const size_t N = (size_t)1 << srs->log_n;
  host::A2 b2, gen2;
  zk_g1_affine g1;
  zk_g2_affine g2;
  generators(ctx, g1, g2);
  if (!host::load(srs->beta_g2, b2) || !host::load(g2, gen2)) {
    ctx->err = "srs_contribute: beta_g2 is not canonical or off its curve";
    return ZK_ERR_ARG;
  }
  // everything into scratch: the string changes only once nothing can fail any more
  std::vector<zk_g1_affine> t1(2 * N), al(N), be(N);
  std::vector<zk_g2_affine> t2(N);
  DevBuf pw;
  pw.ensure(sizeof(Fr) * 2 * N);
  const host::Fr sm = host::fr_to_mont(s->l);
  auto powers = [&](const host::Fr& scale, size_t cnt) {
    Fr base, sc;
    const host::Fr bd = host::fr_to_dev(sm), sd = host::fr_to_dev(scale);
    std::memcpy(base.v, bd.l, 32);
    std::memcpy(sc.v, sd.l, 32);
    fr_powers(pw.as<Fr>(), base, sc, cnt, st);
    fr_from_mont(pw.as<Fr>(), pw.as<uint64_t>(), cnt, st);
  };
  powers(host::fr_one(), 2 * N);
  int rc = mv_mul_scalars<FqC>(ctx, srs->tau_g1, 2 * N, nullptr, pw.as<uint64_t>(), t1.data(), mv_shipped<FqC>(),
                               "srs_contribute_tau_g1");
  if (rc == ZK_OK)
    rc = mv_mul_scalars<Fq2C>(ctx, srs->tau_g2, N, nullptr, pw.as<uint64_t>(), t2.data(), mv_shipped<Fq2C>(),
                              "srs_contribute_tau_g2");
  if (rc != ZK_OK) return rc;
  powers(host::fr_to_mont(a->l), N);
  rc = mv_mul_scalars<FqC>(ctx, srs->alpha_tau_g1, N, nullptr, pw.as<uint64_t>(), al.data(), mv_shipped<FqC>(),
                           "srs_contribute_alpha_g1");
  if (rc != ZK_OK) return rc;
  powers(host::fr_to_mont(b->l), N);
  rc = mv_mul_scalars<FqC>(ctx, srs->beta_tau_g1, N, nullptr, pw.as<uint64_t>(), be.data(), mv_shipped<FqC>(),
                           "srs_contribute_beta_g1");
  if (rc != ZK_OK) return rc;
  const zk_g2_affine nb2 = host_mul_g2(b2, *b);
  if (share) {
    share->tau_g2 = host_mul_g2(gen2, *s);
    share->alpha_g2 = host_mul_g2(gen2, *a);
    share->beta_g2 = host_mul_g2(gen2, *b);
  }
  std::memcpy(srs->tau_g1, t1.data(), sizeof(zk_g1_affine) * 2 * N);
  std::memcpy(srs->tau_g2, t2.data(), sizeof(zk_g2_affine) * N);
  std::memcpy(srs->alpha_tau_g1, al.data(), sizeof(zk_g1_affine) * N);
  std::memcpy(srs->beta_tau_g1, be.data(), sizeof(zk_g1_affine) * N);
  srs->beta_g2 = nb2;
  return ZK_OK;
}

static int srs_verify_contribution(zk_ctx* ctx, const zk_srs* before, const zk_srs* after, const zk_srs_share* share,
                                   const zk_fr* coeffs, size_t n_coeffs, int* status, int* srs_status) {
  *status = ZK_SRSC_SHARE;
  const zk_g2_affine sh[3] = {share->tau_g2, share->alpha_g2, share->beta_g2};
  int rc = ZK_OK;
  if (!srs_valid(ctx, "share", sh, 3, rc)) return rc;
  *status = ZK_SRSC_STRING;
  rc = zk_srs_verify(ctx, after, coeffs, n_coeffs, srs_status);
  if (rc != ZK_OK || *srs_status != ZK_SRS_OK) return rc;
  zk_g1_affine g1;
  zk_g2_affine g2;
  generators(ctx, g1, g2);
  *status = ZK_SRSC_TAU;
  if (!pairs_equal(after->tau_g1[1], g2, before->tau_g1[1], share->tau_g2)) return ZK_OK;
  *status = ZK_SRSC_ALPHA;
  if (!pairs_equal(after->alpha_tau_g1[0], g2, before->alpha_tau_g1[0], share->alpha_g2)) return ZK_OK;
  *status = ZK_SRSC_BETA;
  if (!pairs_equal(after->beta_tau_g1[0], g2, before->beta_tau_g1[0], share->beta_g2)) return ZK_OK;
  *status = ZK_SRSC_OK;
  return ZK_OK;
}

}  // namespace zk

using namespace zk;

#define ZK_SGUARD(ctx, ...)                                   \
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

int zk_g1_ntt(zk_ctx* ctx, zk_g1_affine* pts, uint32_t log_n, int dir) {
  if (!ctx || !pts || (dir != 1 && dir != -1)) return ZK_ERR_ARG;
  if (log_n > 32) return ZK_ERR_DOMAIN;
  ZK_SGUARD(ctx, { return gntt_host<FqC>(ctx, pts, log_n, dir); })
}
int zk_g2_ntt(zk_ctx* ctx, zk_g2_affine* pts, uint32_t log_n, int dir) {
  if (!ctx || !pts || (dir != 1 && dir != -1)) return ZK_ERR_ARG;
  if (log_n > 32) return ZK_ERR_DOMAIN;
  ZK_SGUARD(ctx, { return gntt_host<Fq2C>(ctx, pts, log_n, dir); })
}

int zk_groth16_setup_srs_sound(zk_ctx* ctx, const zk_r1cs_csr* qap, const zk_srs* srs, uint64_t num_public, zk_pk* pk,
                               zk_vk* vk) {
  if (!ctx || !qap || !srs || !pk || !srs->tau_g1 || !srs->tau_g2 || !srs->alpha_tau_g1 || !srs->beta_tau_g1)
    return ZK_ERR_ARG;
  if (!pk->a_g1 || !pk->b_g1 || !pk->b_g2 || !pk->h_g1 || (vk && !vk->ic_g1)) return ZK_ERR_ARG;
  if (qap->num_variables > num_public + 1 && !pk->ic_g1) return ZK_ERR_ARG;
  ZK_SGUARD(ctx, { return setup_srs(ctx, qap, srs, num_public, pk, vk); })
}

int zk_srs_generate(zk_ctx* ctx, uint32_t log_n, const zk_fr* tau, const zk_fr* alpha, const zk_fr* beta, zk_srs* out) {
  if (!ctx || !tau || !alpha || !beta || !out) return ZK_ERR_ARG;
  if (log_n > 31) return ZK_ERR_DOMAIN;
  const uint64_t N = 1ull << log_n;
  if (!out->tau_g1 || !out->tau_g2 || !out->alpha_tau_g1 || !out->beta_tau_g1 || out->tau_g1_len < 2 * N ||
      out->tau_g2_len < N || out->alpha_len < N || out->beta_len < N)
    return ZK_ERR_ARG;
  if (fr_is0(*tau) || fr_is0(*alpha) || fr_is0(*beta)) return ZK_ERR_SETUP_PARAMS;
  if (!fr_canonical(*tau) || !fr_canonical(*alpha) || !fr_canonical(*beta)) {
    ctx->err = "srs_generate: a parameter is not a canonical Fr (>= r)";
    return ZK_ERR_ARG;
  }
  ZK_SGUARD(ctx, { return srs_generate(ctx, log_n, tau, alpha, beta, out); })
}

int zk_srs_verify(zk_ctx* ctx, const zk_srs* srs, const zk_fr* coeffs, size_t n_coeffs, int* status) {
  if (!ctx || !srs || !status || (n_coeffs && !coeffs)) return ZK_ERR_ARG;
  *status = ZK_SRS_SHAPE;
  if (srs->log_n > 31) return ZK_OK;
  const uint64_t N = 1ull << srs->log_n;
  if (srs->tau_g1_len != 2 * N || srs->tau_g2_len != N || srs->alpha_len != N || srs->beta_len != N ||
      n_coeffs != 2 * N)
    return ZK_OK;
  if (!srs->tau_g1 || !srs->tau_g2 || !srs->alpha_tau_g1 || !srs->beta_tau_g1) return ZK_ERR_ARG;
  for (size_t i = 0; i < n_coeffs; i++)
    if (fr_is0(coeffs[i]) || coeffs[i].l[2] || coeffs[i].l[3]) {
      ctx->err = "srs_verify: coefficient " + std::to_string(i) + " must be non-zero and below 2^128";
      return ZK_ERR_ARG;
    }
  ZK_SGUARD(ctx, { return srs_verify(ctx, srs, coeffs, status); })
}

// the lengths that log_n states
static bool srs_shape_ok(const zk_srs* s) {
  if (s->log_n > 31) return false;
  const uint64_t N = 1ull << s->log_n;
  return s->tau_g1_len == 2 * N && s->tau_g2_len == N && s->alpha_len == N && s->beta_len == N;
}

int zk_srs_contribute(zk_ctx* ctx, zk_srs* srs, const zk_fr* s, const zk_fr* a, const zk_fr* b, zk_srs_share* share) {
  if (!ctx || !srs || !s || !a || !b) return ZK_ERR_ARG;
  if (!fr_share_ok(*s) || !fr_share_ok(*a) || !fr_share_ok(*b)) {
    ctx->err = "srs_contribute: every share must be non-zero and below r";
    return ZK_ERR_ARG;
  }
  if (!srs_shape_ok(srs)) {
    ctx->err = "srs_contribute: an array's length is not what log_n states";
    return ZK_ERR_ARG;
  }
  if (!srs->tau_g1 || !srs->tau_g2 || !srs->alpha_tau_g1 || !srs->beta_tau_g1) return ZK_ERR_ARG;
  ZK_SGUARD(ctx, { return srs_contribute(ctx, srs, s, a, b, share); })
}

int zk_srs_verify_contribution(zk_ctx* ctx, const zk_srs* before, const zk_srs* after, const zk_srs_share* share,
                               const zk_fr* coeffs, size_t n_coeffs, int* status, int* srs_status) {
  if (!ctx || !before || !after || !share || !status || !srs_status || (n_coeffs && !coeffs)) return ZK_ERR_ARG;
  *status = ZK_SRSC_SHAPE;
  *srs_status = ZK_SRS_OK;
  if (before->log_n != after->log_n || !srs_shape_ok(before) || !srs_shape_ok(after) ||
      n_coeffs != 2 * after->tau_g2_len)
    return ZK_OK;
  if (!before->tau_g1 || !before->alpha_tau_g1 || !before->beta_tau_g1 || !after->tau_g1 || !after->tau_g2 ||
      !after->alpha_tau_g1 || !after->beta_tau_g1)
    return ZK_ERR_ARG;
  ZK_SGUARD(ctx, { return srs_verify_contribution(ctx, before, after, share, coeffs, n_coeffs, status, srs_status); })
}
