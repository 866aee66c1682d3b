// verify_all.hip -- sound batch verification on the GPU: ONE pairing check for
// n Groth16 proofs against one sound verification key
// (zk_groth16_verify_all_sound, zk_groth16_verify_all_bytes_sound).  With
// coefficients c_k (non-zero, below 2^128) the random-linear-combination check
//   s = sum c_k,  t_i = sum c_k x_{k,i},  IC* = s ic_0 + sum t_i ic_{i+1},  S_C = sum c_k C_k
//   F = prod_k f_{|x|,B_k}(c_k A_k)                                   (unconjugated Miller values)
//   finalexp(conj(F f(-s alpha, beta) f(-IC*, gamma) f(-S_C, delta))) == 1
// holds for every choice of c_k when all proofs verify, fails for every c_k
// when exactly one well-formed proof does not, and otherwise fails except with
// probability about 2^-127 over independent uniform c_k.  The
// argument needs A, B, C in the prime-order subgroup, so the subgroup is
// checked here: by the proof decoder for wire bytes, by points.hpp's
// endomorphism test in the Miller kernel for zk_proof records.
//
// Per proof the device pays one single-pair Miller loop, two 128-bit G1
// multiplications and a few Fr products (k_verify_all_miller, one lane per
// proof); halving folds reduce the lanes' Fq12, XYZZ and Fr values into the
// call's running accumulators (slot 0 of the arrays, verify_all.hpp); after
// the last chunk one lane per term multiplies s alpha, s ic_0, t_i ic_{i+1},
// and one lane runs the last three-pair Miller loop and the only final
// exponentiation of the call.  Every field operation is exact, so the result
// does not depend on the fold order or the chunking.
#include <algorithm>
#include <cstring>
#include <vector>

#include "verify_all.hpp"

namespace zk {

// the per-call words of the verification key (32-bit, device Montgomery):
//   [VA_TAB, +2 x 48 PR_STEPS)      the lines of gamma, then of delta
//   [VA_ON, +4)                     gamma finite, delta finite
//   [VA_ALPHA, +24)                 alpha: x, y; the identity is (0, 0)
//   [VA_BETA, +48)                  beta: x, y (Fq2 each); the identity is (0, 0)
//   [VA_IC, +24 (n_inputs + 1))     ic_g1: x, y; an identity entry is (0, 0)
constexpr size_t VA_TAB = 0, VA_ON = 2 * 48 * PR_STEPS, VA_ALPHA = VA_ON + 4, VA_BETA = VA_ALPHA + 24,
                 VA_IC = VA_BETA + 48;
constexpr int FR_BLOCK = 256;

static __device__ __noinline__ Fr va_fr_mul(Fr a, Fr b) { return fp_mul(a, b); }
ZK_DI Fr va_fr_read(const uint64_t* w) {
  Fr c;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    c.v[2 * i] = (uint32_t)w[i];
    c.v[2 * i + 1] = (uint32_t)(w[i] >> 32);
  }
  return c;
}
ZK_DI Fr va_fr_to_mont(const Fr& c) { return va_fr_mul(c, fp_from_const<FrParams>(FrParams::R2)); }

// k P for a coefficient k < 2^128: the rolled double-and-add of pr_g1_mul255
static __device__ __noinline__ XYZZ<FqC> va_g1_mul128(const Affine<FqC>* P, uint64_t lo, uint64_t hi) {
  XYZZ<FqC> t;
  xyzz_set_inf(t);
#pragma unroll 1
  for (int b = 127; b >= 0; b--) {
    t = xyzz_dbl(t);
    if (((b < 64 ? lo : hi) >> (b & 63)) & 1) t = xyzz_madd(t, *P);
  }
  return t;
}

// Slot 0 of the three arrays: 1, the identity and W zeros
__global__ void k_verify_all_init(F12* __restrict__ f, XYZZ<FqC>* __restrict__ g, Fr* __restrict__ s, size_t W) {
  if (blockIdx.x || threadIdx.x) return;
  F12 one;
  f12_set_one(&one);
  f[0] = one;
  XYZZ<FqC> o;
  xyzz_set_inf(o);
  g[0] = o;
  for (size_t j = 0; j < W; j++) s[j] = fp_zero<FrParams>();
}

// One lane per proof.  The lane checks its proof as zk_groth16_verify_many_sound
// does (coordinates below p, on the curve, inputs below r) and, for SUBGROUP,
// the subgroup of A, B and C (for wire bytes the decoder has done that, and an
// invalid point arrives as (0, 0), which is on neither curve).  It writes
//   fo[i] = f_{|x|,B}(c A)   (1 when A or B is the identity),
//   go[i] = c C,   so[W i] = c,  so[W i + 1 + k] = c x_k   (Montgomery Fr),
// and for a malformed proof bad[i] = 1 with 1, the identity and zeros.
template <bool SUBGROUP>
__global__ void __launch_bounds__(PR_BLOCK) k_verify_all_miller(const uint64_t* __restrict__ proofs,
                                                                const uint64_t* __restrict__ inputs, size_t n_inputs,
                                                                const uint64_t* __restrict__ coeffs, size_t n,
                                                                F12* __restrict__ fo, XYZZ<FqC>* __restrict__ go,
                                                                Fr* __restrict__ so, uint8_t* __restrict__ bad) {
  const size_t i = (size_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (i >= n) return;
  const size_t W = n_inputs + 1;
  const uint64_t* w = proofs + PROOF_WORDS * i;
  PrPairs in;
  Affine<FqC> A, Cp;
  bool a_inf, b_inf, c_inf;
  bool ok = pr_load_g1(w, &A, &a_inf);
  ok = pr_load_g2(w + G1W, &in.Q, &b_inf) && ok;
  ok = pr_load_g1(w + G1W + G2W, &Cp, &c_inf) && ok;
#pragma unroll 1
  for (size_t k = 0; k < n_inputs; k++) ok = ok && pr_fr_reduced(inputs + 4 * (n_inputs * i + k));
  if constexpr (SUBGROUP) {
    if (ok && !a_inf) ok = pt_in_subgroup_endo(A);
    if (ok && !c_inf) ok = pt_in_subgroup_endo(Cp);
    if (ok && !b_inf) ok = pt_in_subgroup_endo(in.Q);
  }
  bad[i] = ok ? 0 : 1;
  F12 f;
  XYZZ<FqC> cC;
  xyzz_set_inf(cC);
  if (!ok) {
    f12_set_one(&f);
    fo[i] = f;
    go[i] = cC;
#pragma unroll 1
    for (size_t k = 0; k < W; k++) so[W * i + k] = fp_zero<FrParams>();
    return;
  }
  const uint64_t c_lo = coeffs[4 * i], c_hi = coeffs[4 * i + 1];
  bool on = !a_inf && !b_inf;
  if (on) {
    const XYZZ<FqC> cA = va_g1_mul128(&A, c_lo, c_hi);
    on = !xyzz_is_inf(cA);
    if (on) A = pr_g1_affine(cA);
  }
  if (on) {
    pr_use_g1(in, 0, A, true);
    in.on[1] = in.on[2] = false;
    in.tab[0] = in.tab[1] = nullptr;
    pr_miller(&f, &in);
  } else {
    f12_set_one(&f);
  }
  fo[i] = f;
  if (!c_inf) cC = va_g1_mul128(&Cp, c_lo, c_hi);
  go[i] = cC;
  const Fr cm = va_fr_to_mont(va_fr_read(coeffs + 4 * i));
  so[W * i] = cm;
#pragma unroll 1
  for (size_t k = 0; k < n_inputs; k++)
    so[W * i + 1 + k] = va_fr_mul(cm, va_fr_to_mont(va_fr_read(inputs + 4 * (n_inputs * i + k))));
}

// One halving pass of a fold over cnt elements, half = ceil(cnt / 2):
// a[i] = a[i] op a[i + half] for i < cnt - half, which leaves half elements.
// Right for any cnt; the host repeats it until one element is left.
__global__ void __launch_bounds__(PR_BLOCK) k_verify_all_fold_f12(F12* a, size_t half, size_t cnt) {
  const size_t i = (size_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (i >= cnt - half) return;
  F12 x = a[i], y = a[i + half], r;
  f12_mul(&r, &x, &y);
  a[i] = r;
}
// xyzz_add covers equal operands (its doubling branch), inverse operands and the identity
__global__ void __launch_bounds__(PR_BLOCK) k_verify_all_fold_g1(XYZZ<FqC>* a, size_t half, size_t cnt) {
  const size_t i = (size_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (i >= cnt - half) return;
  const XYZZ<FqC> x = a[i], y = a[i + half];
  a[i] = xyzz_add(x, y);
}
// W Fr per slot: the same pass over the flattened array (half, cnt in Fr)
__global__ void __launch_bounds__(FR_BLOCK) k_verify_all_fold_fr(Fr* a, size_t half, size_t cnt) {
  const size_t i = (size_t)blockIdx.x * FR_BLOCK + threadIdx.x;
  if (i >= cnt - half) return;
  a[i] = fp_add(a[i], a[i + half]);
}

// One lane per term of the finish, W + 1 of them: lane 0 s alpha, lane 1
// s ic_0, lane 2 + i t_i ic_{i+1}.  The lane writes its canonical scalar to
// scal[4 j] (the words pr_g1_mul255 then walks) and its product to terms[j];
// a zero scalar or an identity base gives the identity without the loop.
__global__ void __launch_bounds__(PR_BLOCK) k_verify_all_terms(const Fr* __restrict__ s, const uint32_t* __restrict__ vk,
                                                               size_t W, uint64_t* scal, XYZZ<FqC>* __restrict__ terms) {
  const size_t j = (size_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (j > W) return;
  const Fr c = fp_from_mont(s[j ? j - 1 : 0]);
#pragma unroll
  for (int k = 0; k < 4; k++) scal[4 * j + k] = (uint64_t)c.v[2 * k] | ((uint64_t)c.v[2 * k + 1] << 32);
  const uint32_t* bw = j ? vk + VA_IC + 24 * (j - 1) : vk + VA_ALPHA;
  Affine<FqC> base;
  base.x = {pr_fq_load(bw)};
  base.y = {pr_fq_load(bw + 12)};
  XYZZ<FqC> t;
  xyzz_set_inf(t);
  if (!fp_is_zero(c) && !aff_is_inf(base)) t = pr_g1_mul255(&base, scal + 4 * j);
  terms[j] = t;
}

// One lane: the three-pair Miller loop of (-s alpha, beta) on the fly,
// (-IC*, gamma) and (-S_C, delta) from the tables, times F, conjugated once
// for the negative x, the final exponentiation, and the verdict byte.
__global__ void __launch_bounds__(PR_BLOCK) k_verify_all_final(const F12* __restrict__ F, const XYZZ<FqC>* __restrict__ g,
                                                               const XYZZ<FqC>* __restrict__ terms,
                                                               const uint32_t* __restrict__ vk, uint8_t* __restrict__ out) {
  if (blockIdx.x || threadIdx.x) return;
  PrPairs in;
  in.Q.x = f2_load(vk + VA_BETA);
  in.Q.y = f2_load(vk + VA_BETA + 24);
  const XYZZ<FqC> sa = terms[0], ic = terms[1], sc = g[0];
  Affine<FqC> P;
  f_set_zero(P.x);
  f_set_zero(P.y);
  bool on = !xyzz_is_inf(sa) && !aff_is_inf(in.Q);
  pr_use_g1(in, 0, on ? aff_neg(pr_g1_affine(sa)) : P, on);
  on = !xyzz_is_inf(ic) && vk[VA_ON] != 0;
  pr_use_g1(in, 1, on ? aff_neg(pr_g1_affine(ic)) : P, on);
  on = !xyzz_is_inf(sc) && vk[VA_ON + 1] != 0;
  pr_use_g1(in, 2, on ? aff_neg(pr_g1_affine(sc)) : P, on);
  in.tab[0] = vk + VA_TAB;
  in.tab[1] = vk + VA_TAB + 48 * PR_STEPS;
  F12 f, acc;
  pr_miller(&f, &in);
  acc = F[0];
  f12_mul(&f, &f, &acc);
  f12_conj(&f, &f);
  f12_final_exp(&f);
  out[0] = f12_is_one(&f) ? 1 : 0;
}

// ---- per-call data (host) ------------------------------------------------------
// Every point of the key is validated (as pairing.hip's pairing_tables): false
// for a malformed one.  No host Miller loop: (-s alpha, beta) runs on the device.
static bool verify_all_tables(const zk_vk& vk, size_t n_inputs, std::vector<uint32_t>& out) {
  host::A1 alpha, p;
  host::A2 beta, gamma, delta;
  if (!host::load(vk.alpha_g1, alpha) || !host::load(vk.beta_g2, beta) || !host::load(vk.gamma_g2, gamma) ||
      !host::load(vk.delta_g2, delta))
    return false;
  out.assign(VA_IC + 24 * (n_inputs + 1), 0);
  if (!gamma.inf) line_table(gamma, &out[VA_TAB]);
  if (!delta.inf) line_table(delta, &out[VA_TAB + 48 * PR_STEPS]);
  out[VA_ON] = gamma.inf ? 0 : 1;
  out[VA_ON + 1] = delta.inf ? 0 : 1;
  if (!alpha.inf) {
    put_fq(&out[VA_ALPHA], alpha.x);
    put_fq(&out[VA_ALPHA + 12], alpha.y);
  }
  if (!beta.inf) {
    put_fq(&out[VA_BETA], beta.x.c0);
    put_fq(&out[VA_BETA + 12], beta.x.c1);
    put_fq(&out[VA_BETA + 24], beta.y.c0);
    put_fq(&out[VA_BETA + 36], beta.y.c1);
  }
  for (size_t k = 0; k < vk.ic_len; k++) {
    if (!host::load(vk.ic_g1[k], p)) return false;
    if (k > n_inputs || p.inf) continue;
    put_fq(&out[VA_IC + 24 * k], p.x);
    put_fq(&out[VA_IC + 24 * k + 12], p.y);
  }
  return true;
}

// ---- drivers -------------------------------------------------------------------------
// cnt elements of the three arrays (slot 0 the accumulators) down to slot 0
static void fold_launch(hipStream_t st, F12* f, XYZZ<FqC>* g, Fr* s, size_t W, size_t cnt) {
  while (cnt > 1) {
    const size_t half = (cnt + 1) / 2, m = cnt - half;
    if (f) k_verify_all_fold_f12<<<ceil_div(m, PR_BLOCK), PR_BLOCK, 0, st>>>(f, half, cnt);
    k_verify_all_fold_g1<<<ceil_div(m, PR_BLOCK), PR_BLOCK, 0, st>>>(g, half, cnt);
    if (s) k_verify_all_fold_fr<<<ceil_div(W * m, FR_BLOCK), FR_BLOCK, 0, st>>>(s, W * half, W * cnt);
    ZK_LAUNCH_CHECK();
    cnt = half;
  }
}

int verify_all_accumulate(zk_ctx* ctx, const zk_vk* vk, const zk_proof* proofs, const uint8_t* bytes,
                          const zk_fr* inputs, size_t n_inputs, size_t n, const zk_fr* coeffs, size_t* first_bad,
                          uint8_t* point_status, VerifyAll& S) {
  *first_bad = n;
  if (n_inputs != vk->num_public) return ZK_ERR_INVALID_WITNESS;
  if (!vk->ic_g1 || vk->ic_len < n_inputs + 1) {
    ctx->err = "verification key: ic_g1 shorter than the public inputs";
    return ZK_ERR_ARG;
  }
  for (size_t k = 0; k < n; k++) {
    const uint64_t* c = coeffs[k].l;
    if (!(c[0] | c[1]) || (c[2] | c[3])) {
      ctx->err = "coefficient " + std::to_string(k) + ": " + (c[2] | c[3] ? "not below 2^128" : "zero");
      return ZK_ERR_ARG;
    }
  }
  std::vector<uint32_t> tables;
  if (!verify_all_tables(*vk, n_inputs, tables)) {
    ctx->err = "verification key: a point is not canonical or not on its curve";
    return ZK_ERR_ARG;
  }
  hipStream_t st = ctx->stream;
  const size_t W = n_inputs + 1, chunk = std::max<size_t>(std::min<size_t>(ctx->verify_chunk, n), 1);
  const size_t in_sz = sizeof(zk_fr) * n_inputs;
  S.W = W;
  S.vk.ensure(4 * tables.size());
  S.proofs.ensure(sizeof(zk_proof) * chunk);
  S.in.ensure(std::max<size_t>(in_sz * chunk, 16));
  S.co.ensure(sizeof(zk_fr) * chunk);
  S.bad.ensure(chunk);
  S.f12.ensure(sizeof(F12) * (chunk + 1));
  S.g1.ensure(sizeof(XYZZ<FqC>) * (chunk + 1));
  S.fr.ensure(sizeof(Fr) * W * (chunk + 1));
  if (bytes) {
    S.bytes.ensure(192 * chunk);
    S.pst.ensure(3 * chunk);
  }
  ZK_HIP(hipMemcpyAsync(S.vk.p, tables.data(), 4 * tables.size(), hipMemcpyHostToDevice, st));
  k_verify_all_init<<<1, 1, 0, st>>>(S.F(), S.G(), S.S(), W);
  ZK_LAUNCH_CHECK();
  std::vector<uint8_t> bad(chunk);
  for (size_t lo = 0; lo < n; lo += chunk) {
    const size_t m = std::min(chunk, n - lo);
    if (bytes) {
      ZK_HIP(hipMemcpyAsync(S.bytes.p, bytes + 192 * lo, 192 * m, hipMemcpyHostToDevice, st));
      proofs_decode_launch(ctx, st, S.bytes.as<uint8_t>(), m, S.proofs.as<uint64_t>(), S.pst.as<uint8_t>());
    } else {
      ZK_HIP(hipMemcpyAsync(S.proofs.p, proofs + lo, sizeof(zk_proof) * m, hipMemcpyHostToDevice, st));
    }
    if (in_sz) ZK_HIP(hipMemcpyAsync(S.in.p, inputs + n_inputs * lo, in_sz * m, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(S.co.p, coeffs + lo, sizeof(zk_fr) * m, hipMemcpyHostToDevice, st));
    int pi = ctx->prof.begin(st, "verify_all_miller", m);
    if (bytes)
      k_verify_all_miller<false><<<ceil_div(m, PR_BLOCK), PR_BLOCK, 0, st>>>(
          S.proofs.as<uint64_t>(), S.in.as<uint64_t>(), n_inputs, S.co.as<uint64_t>(), m, S.F() + 1, S.G() + 1,
          S.S() + W, S.bad.as<uint8_t>());
    else
      k_verify_all_miller<true><<<ceil_div(m, PR_BLOCK), PR_BLOCK, 0, st>>>(
          S.proofs.as<uint64_t>(), S.in.as<uint64_t>(), n_inputs, S.co.as<uint64_t>(), m, S.F() + 1, S.G() + 1,
          S.S() + W, S.bad.as<uint8_t>());
    ZK_LAUNCH_CHECK();
    ctx->prof.end(st, pi);
    pi = ctx->prof.begin(st, "verify_all_fold", m);
    fold_launch(st, S.F(), S.G(), S.S(), W, m + 1);
    ctx->prof.end(st, pi);
    ZK_HIP(hipMemcpyAsync(bad.data(), S.bad.p, m, hipMemcpyDeviceToHost, st));
    if (point_status) ZK_HIP(hipMemcpyAsync(point_status + 3 * lo, S.pst.p, 3 * m, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));   // the next chunk reuses the buffers
    if (*first_bad == n) {
      const uint8_t* hit = static_cast<const uint8_t*>(std::memchr(bad.data(), 1, m));
      if (hit) *first_bad = lo + (size_t)(hit - bad.data());
    }
  }
  return ZK_OK;
}

// The finish on the accumulators of S: the W + 1 scalar multiplications, the
// fold of the IC terms into terms[1], the last Miller loop and the verdict.
static int verify_all_finish(zk_ctx* ctx, VerifyAll& S, int* valid) {
  hipStream_t st = ctx->stream;
  const size_t W = S.W;
  S.scal.ensure(32 * (W + 1));
  S.terms.ensure(sizeof(XYZZ<FqC>) * (W + 1));
  S.verdict.ensure(16);
  const int pi = ctx->prof.begin(st, "verify_all_finish", W + 1);
  k_verify_all_terms<<<ceil_div(W + 1, PR_BLOCK), PR_BLOCK, 0, st>>>(S.S(), S.vk.as<uint32_t>(), W,
                                                                    S.scal.as<uint64_t>(), S.terms.as<XYZZ<FqC>>());
  ZK_LAUNCH_CHECK();
  fold_launch(st, nullptr, S.terms.as<XYZZ<FqC>>() + 1, nullptr, 0, W);
  k_verify_all_final<<<1, PR_BLOCK, 0, st>>>(S.F(), S.G(), S.terms.as<XYZZ<FqC>>(), S.vk.as<uint32_t>(),
                                            S.verdict.as<uint8_t>());
  ZK_LAUNCH_CHECK();
  ctx->prof.end(st, pi);
  uint8_t v = 0;
  ZK_HIP(hipMemcpyAsync(&v, S.verdict.p, 1, hipMemcpyDeviceToHost, st));
  ZK_HIP(hipStreamSynchronize(st));
  *valid = v ? 1 : 0;
  return ZK_OK;
}

static int verify_all_run(zk_ctx* ctx, const zk_vk* vk, const zk_proof* proofs, const uint8_t* bytes,
                          const zk_fr* inputs, size_t n_inputs, size_t n, const zk_fr* coeffs, int* valid,
                          size_t* first_malformed, uint8_t* point_status) {
  VerifyAll S;
  size_t first_bad = n;
  int rc = verify_all_accumulate(ctx, vk, proofs, bytes, inputs, n_inputs, n, coeffs, &first_bad, point_status, S);
  if (rc == ZK_OK) {
    if (first_malformed) *first_malformed = first_bad;
    if (!n) *valid = 1;
    else if (first_bad < n) *valid = 0;   // no verdict to compute: a malformed proof decides
    else rc = verify_all_finish(ctx, S, valid);
  }
  if (ctx->prof.on) ctx->prof.collect();
  return rc;
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

int zk_groth16_verify_all_sound(zk_ctx* ctx, const zk_vk* vk, const zk_proof* proofs, const zk_fr* public_inputs,
                                size_t n_inputs, size_t n_proofs, const zk_fr* coeffs, int* valid,
                                size_t* first_malformed) {
  if (!ctx || !vk || !valid || (n_proofs && (!proofs || !coeffs || (n_inputs && !public_inputs)))) return ZK_ERR_ARG;
  ZK_PGUARD(ctx, {
    return verify_all_run(ctx, vk, proofs, nullptr, public_inputs, n_inputs, n_proofs, coeffs, valid, first_malformed,
                          nullptr);
  })
}
int zk_groth16_verify_all_bytes_sound(zk_ctx* ctx, const zk_vk* vk, const uint8_t* proofs, const zk_fr* public_inputs,
                                      size_t n_inputs, size_t n_proofs, const zk_fr* coeffs, int* valid,
                                      size_t* first_malformed, uint8_t* point_status) {
  if (!ctx || !vk || !valid || (n_proofs && (!proofs || !coeffs || (n_inputs && !public_inputs)))) return ZK_ERR_ARG;
  ZK_PGUARD(ctx, {
    return verify_all_run(ctx, vk, nullptr, proofs, public_inputs, n_inputs, n_proofs, coeffs, valid, first_malformed,
                          point_status);
  })
}
