// srs.hpp -- device helpers of the group transform and the sparse column
// sums over points (srs.hip): a sound key from a powers-of-tau string.
//
// Everything is written once over the field behind the out-of-line products
// of points.hpp (FqC for G1, Fq2C for G2) and curve.hpp's XYZZ formulas.  A
// point that a long walk adds again and again stays in memory and is fetched a
// coordinate at a time where the formula uses it (ceremony.hpp's cm_add_slot,
// here for both groups): beside the accumulator only the formula's own values
// are live, which is what lets the G2 walk fit without spills.
#pragma once
#include <chrono>
#include <functional>
#include <vector>

#include "ceremony.hpp"

namespace zk {

constexpr int GN_BLOCK = 128;
// Column sums over points: the fewest entries of one column that one lane of
// the first level adds.  Unless ZK_OPT_SRS_RUN says otherwise the run length is
// the power of two at or above the square root of the longest column, from
// here up: a lane of either level then adds about as many points in sequence
// (DESIGN.md 2.16).
constexpr uint64_t SRS_RUN_MIN = 32;

template <class F>
struct GnField;
template <>
struct GnField<FqC> {
  using Raw = Fq;
  using C = G1;
  static constexpr int W = 13;
};
template <>
struct GnField<Fq2C> {
  using Raw = Fq2;
  using C = G2;
  static constexpr int W = 25;
};

ZK_DI FqC gn_ld(const Fq* p) { return {ld_vec(p)}; }
ZK_DI Fq2C gn_ld(const Fq2* p) { return {ld_vec(p)}; }
template <class F>
ZK_DI XYZZ<F> gn_fetch(const XYZZ<typename GnField<F>::Raw>* p) {
  return {gn_ld(&p->X), gn_ld(&p->Y), gn_ld(&p->ZZ), gn_ld(&p->ZZZ)};
}
template <class F>
ZK_DI void gn_store(XYZZ<typename GnField<F>::Raw>* p, const XYZZ<F>& v) {
  st_vec(&p->X, v.X.v); st_vec(&p->Y, v.Y.v); st_vec(&p->ZZ, v.ZZ.v); st_vec(&p->ZZZ, v.ZZZ.v);
}
// device affine (Montgomery, (0, 0) = infinity); false for the identity
template <class F>
ZK_DI bool gn_fetch_aff(const Affine<typename GnField<F>::Raw>* p, Affine<F>& P) {
  P.x = gn_ld(&p->x);
  P.y = gn_ld(&p->y);
  return !aff_is_inf(P);
}
// ABI words -> Montgomery affine; false for a set infinity byte (unchecked
// otherwise, as cm_load)
ZK_DI bool gn_load_abi(const uint64_t* w, Affine<FqC>& P) { return cm_load(w, P); }
ZK_DI bool gn_load_abi(const uint64_t* w, Affine<Fq2C>& P) {
  if (w[24] & 0xff) return false;
  P.x = {{pt_to_mont(cm_read_fq(w)), pt_to_mont(cm_read_fq(w + 6))}};
  P.y = {{pt_to_mont(cm_read_fq(w + 12)), pt_to_mont(cm_read_fq(w + 18))}};
  return true;
}
template <class F>
ZK_DI XYZZ<F> gn_neg(XYZZ<F> p) {
  p.Y = f_neg(p.Y);
  return p;
}

// p + *q by add-2008-s, q's coordinates fetched where the formula uses them
template <class F>
ZK_DI XYZZ<F> gn_add_mem(const XYZZ<F>& p, const XYZZ<typename GnField<F>::Raw>* q) {
  if (f_is_zero(gn_ld(&q->ZZ))) return p;
  if (xyzz_is_inf(p)) return gn_fetch<F>(q);
  const F U1 = f_mul(p.X, gn_ld(&q->ZZ));
  ZK_SB();
  const F P = f_sub(f_mul(gn_ld(&q->X), p.ZZ), U1);
  ZK_SB();
  const F S1 = f_mul(p.Y, gn_ld(&q->ZZZ));
  ZK_SB();
  const F R = f_sub(f_mul(gn_ld(&q->Y), p.ZZZ), S1);
  ZK_SB();
  if (f_is_zero(P)) {
    if (f_is_zero(R)) return xyzz_dbl(p);
    XYZZ<F> r; xyzz_set_inf(r); return r;
  }
  XYZZ<F> r;
  const F PP = f_sqr(P);
  ZK_SB();
  r.ZZ = f_mul(p.ZZ, gn_ld(&q->ZZ));
  ZK_SB();
  r.ZZ = f_mul(r.ZZ, PP);
  ZK_SB();
  const F PPP = f_mul(P, PP);
  ZK_SB();
  r.ZZZ = f_mul(p.ZZZ, gn_ld(&q->ZZZ));
  ZK_SB();
  r.ZZZ = f_mul(r.ZZZ, PPP);
  ZK_SB();
  const F Q = f_mul(U1, PP);
  ZK_SB();
  r.X = f_sub(f_sub(f_sqr(R), PPP), f_add(Q, Q));
  ZK_SB();
  r.Y = f_mul_sub(R, f_sub(Q, r.X), S1, PPP);
  ZK_SB();
  return r;
}

// The scalar of a walk: four canonical little-endian words and the bits to walk
struct GnScalar {
  uint64_t w[4];
  int top;
};
ZK_DI GnScalar gn_scalar(const uint64_t* k) {
  GnScalar s;
  s.w[0] = k[0]; s.w[1] = k[1]; s.w[2] = k[2]; s.w[3] = k[3];
  s.top = s.w[3] ? 256 - __builtin_clzll(s.w[3])
        : s.w[2] ? 192 - __builtin_clzll(s.w[2])
        : s.w[1] ? 128 - __builtin_clzll(s.w[1])
        : s.w[0] ? 64 - __builtin_clzll(s.w[0]) : 0;
  return s;
}
ZK_DI bool gn_bit(const GnScalar& s, int b) {
  const int j = b >> 6;
  const uint64_t w = j == 0 ? s.w[0] : j == 1 ? s.w[1] : j == 2 ? s.w[2] : s.w[3];
  return (w >> (b & 63)) & 1;
}
// The steps of a walk: the largest `top` among the wave's active lanes, found
// bit by bit through ballots, so the count is one value for the wave and the
// walk's loop is scalar control flow.  A lane with a shorter scalar doubles the
// identity through its leading zero bits (gn_bit is 0 there), which costs the
// wave nothing: it runs its longest lane's steps either way.  A loop whose
// trip count is a per-lane value went wrong at two waves per SIMD once a launch
// had more than 256 blocks.
ZK_DI int gn_wave_top(int top) {
  int m = 0;
#pragma unroll
  for (int bit = 8; bit >= 0; bit--) {
    const int cand = m | (1 << bit);
    if (__ballot(top >= cand) != 0) m = cand;
  }
  return __builtin_amdgcn_readfirstlane(m);
}
// k * (*base), base an XYZZ value in memory: double-and-add from the top set
// bit of the wave's longest scalar, one doubling per bit and one full addition
// per set bit
template <class F>
ZK_DI XYZZ<F> gn_walk_mem(const XYZZ<typename GnField<F>::Raw>* base, const GnScalar& s) {
  XYZZ<F> acc;
  xyzz_set_inf(acc);
  const int steps = gn_wave_top(s.top);
#pragma unroll 1
  for (int b = steps - 1; b >= 0; b--) {
    acc = xyzz_dbl(acc);
    if (gn_bit(s, b)) acc = gn_add_mem(acc, base);
  }
  return acc;
}
// k P for an affine P (not the identity): mixed additions
template <class F>
ZK_DI XYZZ<F> gn_walk_aff(const Affine<F>& P, const GnScalar& s) {
  XYZZ<F> acc;
  xyzz_set_inf(acc);
  const int steps = gn_wave_top(s.top);
#pragma unroll 1
  for (int b = steps - 1; b >= 0; b--) {
    acc = xyzz_dbl(acc);
    if (gn_bit(s, b)) acc = xyzz_madd(acc, P);
  }
  return acc;
}

// ---- host side (srs.hip) ---------------------------------------------------
// In-place transform of n = 2^log_n device ABI points (zk_g1_affine /
// zk_g2_affine words) -> n device affine points (Montgomery) in d_out, on the
// ctx's main stream; inverse: with 1 / n.  phase: the profiler's name.
template <class F>
void gntt_device(zk_ctx* ctx, const uint64_t* d_abi, uint32_t log_n, bool inverse,
                 Affine<typename GnField<F>::Raw>* d_out, const char* phase);

// Shared with keycheck.hip: n elements of sz bytes between host and device in
// pieces of ctx->point_chunk (not synchronised); a point's words without the
// struct padding; the generators as ABI points; e(a, p) == e(b, q) through the
// host pairing.
void chunked_copy(zk_ctx* ctx, void* dst, const void* src, size_t n, size_t sz, hipMemcpyKind kind);
bool same_g1(const zk_g1_affine& a, const zk_g1_affine& b);
bool same_g2(const zk_g2_affine& a, const zk_g2_affine& b);
void generators(zk_ctx* ctx, zk_g1_affine& g1, zk_g2_affine& g2);
bool pairs_equal(const zk_g1_affine& a, const zk_g2_affine& p, const zk_g1_affine& b, const zk_g2_affine& q);

// wall time of a host-side phase into the profiler
struct HostPhase {
  Prof& prof;
  const char* name;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  HostPhase(Prof& p, const char* nm) : prof(p), name(nm) {}
  ~HostPhase() {
    prof.add_host(name, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
};

// ---- the halves of zk_groth16_setup_srs_sound, shared with the prepared
// strings (lagrange.hip) ------------------------------------------------------
// n device affine points -> canonical ABI words in host memory, through
// gn_points_to_abi and chunked_copy (synchronises)
template <class F>
void affine_to_host(zk_ctx* ctx, const Affine<typename GnField<F>::Raw>* d_in, size_t n, void* host_out);
// One array through the point validation; the identity is refused too (srs.hip)
template <class P>
bool srs_valid(zk_ctx* ctx, const char* name, const P* pts, size_t n, int& rc);
// Upper half: the four inverse transforms of the string's first n = 2^log_n
// powers -> L1 = [L | alpha L | beta L]_1 (3 n points), L2 = [L]_2.  d_abi:
// device scratch of max(2 n G1, n G2) ABI points.
void srs_lagrange_transforms(zk_ctx* ctx, const zk_srs* srs, uint32_t log_n, void* d_abi, G1A* L1, G2A* L2);
// d_out[i] = tau_g1[i + n] - tau_g1[i], i < n, affine (d_abi as above; synchronises)
void srs_hdiff(zk_ctx* ctx, const zk_g1_affine* tau_g1, uint64_t n, void* d_abi, G1A* d_out);
// Lower half: the circuit's column sums over L1 / L2, num_variables device
// affine points each, handed to sink one after the other (A, B1, B2 in G2, IC:
// vk entries first); sink returns with the stream idle, the points die after it.
enum { SRS_SUM_A = 0, SRS_SUM_B1, SRS_SUM_B2, SRS_SUM_IC };
using SrsSumSink = std::function<void(int which, const void* d_points)>;
void srs_column_sums(zk_ctx* ctx, const zk_r1cs_csr* q, uint64_t n, const G1A* L1, const G2A* L2,
                     const SrsSumSink& sink);
// the fixed points and the lengths of a key from a string (gamma = delta = 1);
// pk, vk: either may be null
void srs_key_header(const zk_g1_affine& alpha_g1, const zk_g1_affine& beta_g1, const zk_g2_affine& beta_g2,
                    const zk_g1_affine& g1, const zk_g2_affine& g2, uint64_t V, uint64_t n, uint64_t num_public,
                    zk_pk* pk, zk_vk* vk);
// A host key in scratch: the caller's keys change only once nothing can fail
struct SrsHostKey {
  std::vector<zk_g1_affine> a1, b1, ic, h;
  std::vector<zk_g2_affine> b2;
  SrsHostKey(uint64_t V, uint64_t n) : a1(V), b1(V), ic(V), h(n), b2(V) {}
  void take(zk_ctx* ctx, int which, const void* d_points);   // one of srs_column_sums' results
  void fill(const zk_g1_affine& alpha_g1, const zk_g1_affine& beta_g1, const zk_g2_affine& beta_g2,
            const zk_g1_affine& g1, const zk_g2_affine& g2, uint64_t num_public, zk_pk* pk, zk_vk* vk) const;
};

}  // namespace zk
