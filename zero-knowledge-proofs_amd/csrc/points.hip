// points.hip -- batch decompression and validation of G1 / G2 points on the
// GPU: ark-serialize CanonicalDeserialize (compressed, Validate::Yes) of
// G1Affine / G2Affine, and the same checks on points that arrive in affine
// form.  What verify.hip's decode_g1 / decode_g2 do for the three points of a
// proof on the host, one point at a time, these kernels do for the millions
// of points of a proving key, one lane per point (points.hpp).  The proof
// decoder (zk_proofs_deserialize_compressed, and the first stage of
// zk_groth16_verify_many_bytes in pairing.hip) is the same decompression over
// the 192-byte records of a proof batch: ark CanonicalDeserialize
// (compressed, Validate::Yes) on n Proof.
//
// Status per point (zk_point_status): the first failing check in
// decode_g1 / decode_g2's order.  An invalid point's output words are zero.
#include <algorithm>
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "points.hpp"

namespace zk {

// 48 big-endian bytes (16-byte aligned) -> 12 little-endian words
__device__ __forceinline__ Fq read_be48(const uint8_t* p) {
  const uint4* s = reinterpret_cast<const uint4*>(p);
  uint32_t w[12];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const uint4 u = s[k];
    w[4 * k] = u.x; w[4 * k + 1] = u.y; w[4 * k + 2] = u.z; w[4 * k + 3] = u.w;
  }
  Fq c;
#pragma unroll
  for (int i = 0; i < 12; i++) c.v[i] = __builtin_bswap32(w[11 - i]);
  return c;
}
__device__ __forceinline__ Fq read_words(const uint64_t* w) {
  Fq c;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    c.v[2 * i] = (uint32_t)w[i];
    c.v[2 * i + 1] = (uint32_t)(w[i] >> 32);
  }
  return c;
}
__device__ __forceinline__ void write_words(uint64_t* w, const Fq& c) {
#pragma unroll
  for (int i = 0; i < 6; i++) w[i] = (uint64_t)c.v[2 * i] | ((uint64_t)c.v[2 * i + 1] << 32);
}

// Per group: the field behind the out-of-line products, coordinates as
// arrays of Fq (1 for G1, 2 for G2; the encoding carries the LAST coefficient
// first: x.c1 with the flags, then x.c0).
struct PG1 {
  using F = FqC;
  static constexpr int K = 1;
  static __device__ __forceinline__ F make(const Fq* c) { return {c[0]}; }
  static __device__ __forceinline__ void split(const F& a, Fq* c) { c[0] = a.v; }
  static __device__ __forceinline__ bool sqrt(const F& a, F& out) { return pt_fq_sqrt(a.v, out.v); }
};
struct PG2 {
  using F = Fq2C;
  static constexpr int K = 2;
  static __device__ __forceinline__ F make(const Fq* c) { return {{c[0], c[1]}}; }
  static __device__ __forceinline__ void split(const F& a, Fq* c) { c[0] = a.v.c0; c[1] = a.v.c1; }
  static __device__ __forceinline__ bool sqrt(const F& a, F& out) { return pt_fq2_sqrt(a.v, out.v); }
};
// the sort flag of canonical coefficients: the highest non-zero one decides
template <int K>
__device__ __forceinline__ bool largest(const Fq* c) {
  if (K == 2 && !fp_is_zero(c[K - 1])) return pt_fq_largest(c[K - 1]);
  return pt_fq_largest(c[0]);
}

// Where point i of a launch lies: the byte offset of its encoding, the word
// offset of its affine words and the index of its status byte.
template <int K>
struct Packed {   // an array of points (zk_g1/g2_decompress)
  static __device__ __forceinline__ size_t in(size_t i) { return 48 * K * i; }
  static __device__ __forceinline__ size_t out(size_t i) { return (12 * K + 1) * i; }
  static __device__ __forceinline__ size_t st(size_t i) { return i; }
};
// The points of 192-byte compressed proofs a | b | c -> the 13 + 25 + 13
// words of zk_proof records, status 3 k + j for point j of proof k.  G1: one
// launch over 2 n points, a of proof i / 2 on even i and c on odd i; G2: b of
// proof i.  Offsets 0, 48 and 144 of a 192-byte stride keep read_be48's
// 16-byte alignment.
struct ProofG1 {
  static __device__ __forceinline__ size_t in(size_t i) { return 192 * (i >> 1) + 144 * (i & 1); }
  static __device__ __forceinline__ size_t out(size_t i) { return 51 * (i >> 1) + 38 * (i & 1); }
  static __device__ __forceinline__ size_t st(size_t i) { return 3 * (i >> 1) + 2 * (i & 1); }
};
struct ProofG2 {
  static __device__ __forceinline__ size_t in(size_t i) { return 192 * i + 48; }
  static __device__ __forceinline__ size_t out(size_t i) { return 51 * i + 13; }
  static __device__ __forceinline__ size_t st(size_t i) { return 3 * i + 1; }
};

// ENDO: the subgroup test by endomorphism (pt_in_subgroup_endo) instead of [r]P == O
template <class G, class L, bool ENDO>
__device__ __forceinline__ void decompress_point(const uint8_t* __restrict__ in, size_t n, uint64_t* __restrict__ out,
                                                 uint8_t* __restrict__ status) {
  constexpr int K = G::K, W = 12 * K + 1;
  using F = typename G::F;
  const size_t i = (size_t)blockIdx.x * PT_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint8_t* enc = in + L::in(i);
  Fq x[K], y[K];
#pragma unroll
  for (int k = 0; k < K; k++) {
    x[k] = read_be48(enc + 48 * (K - 1 - k));
    y[k] = fp_zero<FqParams>();
  }
  const uint32_t flags = x[K - 1].v[11] >> 29;   // 4 compressed, 2 infinity, 1 sort
  x[K - 1].v[11] &= 0x1fffffffu;
  bool zero_x = true, in_range = true;
#pragma unroll
  for (int k = 0; k < K; k++) {
    zero_x = zero_x && fp_is_zero(x[k]);
    in_range = in_range && !pt_fq_geq_p(x[k]);
  }
  uint32_t st = ZK_POINT_OK;
  bool inf = false;
  if (!(flags & 4)) {
    st = ZK_POINT_ENCODING;
  } else if (flags & 2) {
    if ((flags & 1) || !zero_x) st = ZK_POINT_ENCODING;
    else inf = true;
  } else if (!in_range) {
    st = ZK_POINT_NOT_CANONICAL;
  } else {
    Fq xm[K];
#pragma unroll
    for (int k = 0; k < K; k++) xm[k] = pt_to_mont(x[k]);
    Affine<F> P;
    P.x = G::make(xm);
    if (!G::sqrt(pt_curve_rhs(P.x), P.y)) {
      st = ZK_POINT_NOT_ON_CURVE;
    } else {
      Fq ym[K];
      G::split(P.y, ym);
#pragma unroll
      for (int k = 0; k < K; k++) y[k] = pt_from_mont(ym[k]);
      if (largest<K>(y) != ((flags & 1) != 0)) {
        P.y = f_neg(P.y);
#pragma unroll
        for (int k = 0; k < K; k++) y[k] = fp_neg(y[k]);   // p - y, or 0
      }
      if (!(ENDO ? pt_in_subgroup_endo(P) : pt_in_subgroup(P))) st = ZK_POINT_NOT_IN_SUBGROUP;
    }
  }
  uint64_t* o = out + L::out(i);
  const bool coords = st == ZK_POINT_OK && !inf;
#pragma unroll
  for (int k = 0; k < K; k++) {
    write_words(o + 6 * k, coords ? x[k] : fp_zero<FqParams>());
    write_words(o + 6 * (K + k), coords ? y[k] : fp_zero<FqParams>());
  }
  o[W - 1] = (st == ZK_POINT_OK && inf) ? 1 : 0;
  status[L::st(i)] = (uint8_t)st;
}

template <class G>
__device__ __forceinline__ void validate_point(const uint64_t* __restrict__ in, size_t n, uint8_t* __restrict__ status) {
  constexpr int K = G::K, W = 12 * K + 1;
  using F = typename G::F;
  const size_t i = (size_t)blockIdx.x * PT_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint64_t* w = in + W * i;
  uint32_t st = ZK_POINT_OK;
  if (!(w[W - 1] & 0xff)) {   // a set infinity byte is the identity whatever the coordinates hold
    Fq x[K], y[K];
    bool in_range = true;
#pragma unroll
    for (int k = 0; k < K; k++) {
      x[k] = read_words(w + 6 * k);
      y[k] = read_words(w + 6 * (K + k));
      in_range = in_range && !pt_fq_geq_p(x[k]) && !pt_fq_geq_p(y[k]);
    }
    if (!in_range) {
      st = ZK_POINT_NOT_CANONICAL;
    } else {
#pragma unroll
      for (int k = 0; k < K; k++) {
        x[k] = pt_to_mont(x[k]);
        y[k] = pt_to_mont(y[k]);
      }
      Affine<F> P;
      P.x = G::make(x);
      P.y = G::make(y);
      if (!f_eq(f_sqr(P.y), pt_curve_rhs(P.x))) st = ZK_POINT_NOT_ON_CURVE;
      else if (!pt_in_subgroup(P)) st = ZK_POINT_NOT_IN_SUBGROUP;
    }
  }
  status[i] = (uint8_t)st;
}

__global__ void __launch_bounds__(PT_BLOCK) k_g1_decompress(const uint8_t* __restrict__ in, size_t n,
                                                            uint64_t* __restrict__ out, uint8_t* __restrict__ status) {
  decompress_point<PG1, Packed<1>, false>(in, n, out, status);
}
__global__ void __launch_bounds__(PT_BLOCK) k_g2_decompress(const uint8_t* __restrict__ in, size_t n,
                                                            uint64_t* __restrict__ out, uint8_t* __restrict__ status) {
  decompress_point<PG2, Packed<2>, false>(in, n, out, status);
}
__global__ void __launch_bounds__(PT_BLOCK) k_g1_validate(const uint64_t* __restrict__ in, size_t n,
                                                          uint8_t* __restrict__ status) {
  validate_point<PG1>(in, n, status);
}
__global__ void __launch_bounds__(PT_BLOCK) k_g2_validate(const uint64_t* __restrict__ in, size_t n,
                                                          uint8_t* __restrict__ status) {
  validate_point<PG2>(in, n, status);
}
// The proof decoder (zk_proofs_deserialize_compressed, zk_groth16_verify_many_bytes):
// the same decompression over the records of a proof batch, G1 and G2 in
// launches of their own (a G2 point costs several G1 points; one wave of both
// would wait for its G2 lanes), with the subgroup test by endomorphism.
__global__ void __launch_bounds__(PT_BLOCK) k_proof_g1_decode(const uint8_t* __restrict__ in, size_t n_points,
                                                              uint64_t* __restrict__ out, uint8_t* __restrict__ status) {
  decompress_point<PG1, ProofG1, true>(in, n_points, out, status);
}
__global__ void __launch_bounds__(PT_BLOCK) k_proof_g2_decode(const uint8_t* __restrict__ in, size_t n_points,
                                                              uint64_t* __restrict__ out, uint8_t* __restrict__ status) {
  decompress_point<PG2, ProofG2, true>(in, n_points, out, status);
}

const char* point_status_text(int st) {
  switch (st) {
    case ZK_POINT_OK: return "valid";
    case ZK_POINT_ENCODING: return "bad encoding flags";
    case ZK_POINT_NOT_CANONICAL: return "coordinate not below p";
    case ZK_POINT_NOT_ON_CURVE: return "not on the curve";
    case ZK_POINT_NOT_IN_SUBGROUP: return "not in the prime-order subgroup";
    default: return "unknown status";
  }
}

// One call: the array goes through the GPU in chunks of ctx->point_chunk
// points on the ctx's main stream.  Buffers belong to the call (freed on
// every exit path by DevBuf).  first_bad comes from a host scan of the
// statuses, so it is the lowest failing index whatever the chunking.
template <class G, bool DECOMPRESS>
int points_run(zk_ctx* ctx, const void* in, size_t n, void* out, uint8_t* status, size_t* first_bad) {
  constexpr size_t W = 12 * G::K + 1, ENC = 48 * G::K;
  constexpr size_t in_sz = DECOMPRESS ? ENC : 8 * W;
  if (first_bad) *first_bad = n;
  if (!n) return ZK_OK;
  hipStream_t st = ctx->stream;
  const size_t chunk = std::min<size_t>(ctx->point_chunk, n);
  DevBuf d_in, d_out, d_st;
  d_in.ensure(in_sz * chunk);
  d_st.ensure(chunk);
  if (DECOMPRESS) d_out.ensure(8 * W * chunk);
  std::vector<uint8_t> own;
  if (!status) {
    own.resize(n);
    status = own.data();
  }
  for (size_t lo = 0; lo < n; lo += chunk) {
    const size_t m = std::min(chunk, n - lo);
    ZK_HIP(hipMemcpyAsync(d_in.p, static_cast<const uint8_t*>(in) + in_sz * lo, in_sz * m, hipMemcpyHostToDevice, st));
    const int pi = ctx->prof.begin(st, G::K == 1 ? "points_g1" : "points_g2", m);
    const dim3 grid(ceil_div(m, PT_BLOCK)), block(PT_BLOCK);
    if (DECOMPRESS && G::K == 1)
      k_g1_decompress<<<grid, block, 0, st>>>(d_in.as<uint8_t>(), m, d_out.as<uint64_t>(), d_st.as<uint8_t>());
    else if (DECOMPRESS)
      k_g2_decompress<<<grid, block, 0, st>>>(d_in.as<uint8_t>(), m, d_out.as<uint64_t>(), d_st.as<uint8_t>());
    else if (G::K == 1)
      k_g1_validate<<<grid, block, 0, st>>>(d_in.as<uint64_t>(), m, d_st.as<uint8_t>());
    else
      k_g2_validate<<<grid, block, 0, st>>>(d_in.as<uint64_t>(), m, d_st.as<uint8_t>());
    ZK_LAUNCH_CHECK();
    ctx->prof.end(st, pi);
    if (DECOMPRESS)
      ZK_HIP(hipMemcpyAsync(static_cast<uint8_t*>(out) + 8 * W * lo, d_out.p, 8 * W * m, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipMemcpyAsync(status + lo, d_st.p, m, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));   // the next chunk reuses the buffers
  }
  if (ctx->prof.on) ctx->prof.collect();
  for (size_t i = 0; i < n; i++) {
    if (status[i] == ZK_POINT_OK) continue;
    if (first_bad) *first_bad = i;
    ctx->err = std::string(G::K == 1 ? "G1" : "G2") + " point " + std::to_string(i) + ": " +
               point_status_text(status[i]);
    return ZK_ERR_ARG;
  }
  return ZK_OK;
}

// m ABI points in device memory -> m point statuses in device memory, on st
void points_validate_launch(zk_ctx* ctx, hipStream_t st, bool g2, const uint64_t* d_pts, size_t m, uint8_t* d_st) {
  if (!m) return;
  const int pi = ctx->prof.begin(st, g2 ? "points_g2" : "points_g1", m);
  if (g2) k_g2_validate<<<ceil_div(m, PT_BLOCK), PT_BLOCK, 0, st>>>(d_pts, m, d_st);
  else k_g1_validate<<<ceil_div(m, PT_BLOCK), PT_BLOCK, 0, st>>>(d_pts, m, d_st);
  ZK_LAUNCH_CHECK();
  ctx->prof.end(st, pi);
}

// m compressed proofs in device memory (192 m bytes) -> m zk_proof records and
// 3 m point statuses in device memory, on st: one G1 launch over the 2 m
// points a and c, one G2 launch over the m points b.
void proofs_decode_launch(zk_ctx* ctx, hipStream_t st, const uint8_t* d_in, size_t m, uint64_t* d_out, uint8_t* d_pst) {
  int pi = ctx->prof.begin(st, "proof_decode_g1", 2 * m);
  k_proof_g1_decode<<<ceil_div(2 * m, PT_BLOCK), PT_BLOCK, 0, st>>>(d_in, 2 * m, d_out, d_pst);
  ZK_LAUNCH_CHECK();
  ctx->prof.end(st, pi);
  pi = ctx->prof.begin(st, "proof_decode_g2", m);
  k_proof_g2_decode<<<ceil_div(m, PT_BLOCK), PT_BLOCK, 0, st>>>(d_in, m, d_out, d_pst);
  ZK_LAUNCH_CHECK();
  ctx->prof.end(st, pi);
}

// The lowest invalid point of 3 n proof point statuses into ctx->err: false when there is none
static bool proofs_first_bad(zk_ctx* ctx, const uint8_t* pst, size_t n) {
  for (size_t i = 0; i < 3 * n; i++) {
    if (pst[i] == ZK_POINT_OK) continue;
    ctx->err = "proof " + std::to_string(i / 3) + " point " + "abc"[i % 3] + ": " + point_status_text(pst[i]);
    return true;
  }
  return false;
}

// As points_run, in chunks of ctx->verify_chunk proofs (the records of one
// launch of the verification that zk_groth16_verify_many_bytes puts behind
// the same decode).
static int proofs_run(zk_ctx* ctx, const uint8_t* in, size_t n, zk_proof* out, uint8_t* pst) {
  if (!n) return ZK_OK;
  hipStream_t st = ctx->stream;
  const size_t chunk = std::min<size_t>(ctx->verify_chunk, n);
  DevBuf d_in, d_out, d_st;
  d_in.ensure(192 * chunk);
  d_out.ensure(sizeof(zk_proof) * chunk);
  d_st.ensure(3 * chunk);
  std::vector<uint8_t> own;
  if (!pst) {
    own.resize(3 * n);
    pst = own.data();
  }
  for (size_t lo = 0; lo < n; lo += chunk) {
    const size_t m = std::min(chunk, n - lo);
    ZK_HIP(hipMemcpyAsync(d_in.p, in + 192 * lo, 192 * m, hipMemcpyHostToDevice, st));
    proofs_decode_launch(ctx, st, d_in.as<uint8_t>(), m, d_out.as<uint64_t>(), d_st.as<uint8_t>());
    ZK_HIP(hipMemcpyAsync(out + lo, d_out.p, sizeof(zk_proof) * m, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipMemcpyAsync(pst + 3 * lo, d_st.p, 3 * m, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));   // the next chunk reuses the buffers
  }
  if (ctx->prof.on) ctx->prof.collect();
  return proofs_first_bad(ctx, pst, n) ? ZK_ERR_ARG : ZK_OK;
}

}  // namespace zk

using namespace zk;

#define ZK_PGUARD(ctx, ...)                                   \
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

int zk_g1_decompress(zk_ctx* ctx, const uint8_t* in, size_t n, zk_g1_affine* out, uint8_t* status,
                     size_t* first_bad) {
  if (!ctx || (n && (!in || !out))) return ZK_ERR_ARG;
  ZK_PGUARD(ctx, { return points_run<PG1, true>(ctx, in, n, out, status, first_bad); })
}
int zk_g2_decompress(zk_ctx* ctx, const uint8_t* in, size_t n, zk_g2_affine* out, uint8_t* status,
                     size_t* first_bad) {
  if (!ctx || (n && (!in || !out))) return ZK_ERR_ARG;
  ZK_PGUARD(ctx, { return points_run<PG2, true>(ctx, in, n, out, status, first_bad); })
}
int zk_proofs_deserialize_compressed(zk_ctx* ctx, const uint8_t* in, size_t n, zk_proof* out, uint8_t* point_status) {
  if (!ctx || (n && (!in || !out))) return ZK_ERR_ARG;
  ZK_PGUARD(ctx, { return proofs_run(ctx, in, n, out, point_status); })
}
int zk_g1_validate(zk_ctx* ctx, const zk_g1_affine* pts, size_t n, uint8_t* status, size_t* first_bad) {
  if (!ctx || (n && !pts)) return ZK_ERR_ARG;
  ZK_PGUARD(ctx, { return points_run<PG1, false>(ctx, pts, n, nullptr, status, first_bad); })
}
int zk_g2_validate(zk_ctx* ctx, const zk_g2_affine* pts, size_t n, uint8_t* status, size_t* first_bad) {
  if (!ctx || (n && !pts)) return ZK_ERR_ARG;
  ZK_PGUARD(ctx, { return points_run<PG2, false>(ctx, pts, n, nullptr, status, first_bad); })
}
