// pairing.hip -- pairings on the GPU, one lane per pairing product
// (pairing.hpp): n Groth16 proofs against one verification key with one
// verdict per proof (zk_groth16_verify_many), and n products of k pairings
// each (zk_pairing_products).  What verify.hip's zk_groth16_verify and
// zk_pairing_product_is_one do for one proof or product on a host core, these
// kernels do for a batch; the host code stays the reference.
// zk_groth16_verify_many_bytes puts points.hip's proof decoder in front of
// the same kernel: ark CanonicalDeserialize (compressed, Validate::Yes) on
// Proof, then Verifier::verify, from the proofs' 192 wire bytes.
// zk_groth16_verify_many_prepared / _bytes_prepared run the same drivers with a
// key prepared once (prepared.hip): its words are on the device already and
// its window table gives every proof's IC ahead of the verify kernel.
//
// Per call the host prepares what every lane shares (pairing_tables): the
// Miller value of (-alpha, beta), and for gamma and delta the PR_STEPS affine
// lines of host_pairing.hpp's loop.  Affine host lines and the projective
// device lines of B differ by Fq2 factors only, which the final
// exponentiation removes.
#include <algorithm>
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "host_pairing.hpp"
#include "pairing.hpp"
#include "prepared.hpp"
#include "verify_all.hpp"

namespace zk {

// One lane per proof: Verifier::verify (verify.hip's zk_groth16_verify) with
// the four Miller loops sharing their squarings.  SOUND
// (zk_groth16_verify_sound): every x_k whole -- one >= r makes the proof
// MALFORMED -- instead of its lo64.
template <bool SOUND>
__global__ void __launch_bounds__(PR_BLOCK) k_groth16_verify(const uint64_t* __restrict__ proofs,
                                                             const uint64_t* __restrict__ inputs, size_t n_inputs,
                                                             const uint32_t* __restrict__ vk, size_t n,
                                                             uint8_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint64_t* w = proofs + PROOF_WORDS * i;
  PrPairs in;
  Affine<FqC> A, Cp;
  bool a_inf, b_inf, c_inf;
  bool ok = pr_load_g1(w, &A, &a_inf);
  ok = pr_load_g2(w + G1W, &in.Q, &b_inf) && ok;
  ok = pr_load_g1(w + G1W + G2W, &Cp, &c_inf) && ok;
  if constexpr (SOUND) {
#pragma unroll 1
    for (size_t k = 0; k < n_inputs; k++) ok = ok && pr_fr_reduced(inputs + 4 * (n_inputs * i + k));
  }
  if (!ok) {
    status[i] = ZK_VERIFY_MALFORMED;
    return;
  }
  // IC = ic[0] + sum lo64(x_k) ic[k + 1] over the non-zero lo64(x_k)  (SOUND: the whole x_k)
  Affine<FqC> ic;
  ic.x = {pr_fq_load(vk + VK_IC)};
  ic.y = {pr_fq_load(vk + VK_IC + 12)};
  XYZZ<FqC> acc = xyzz_from_aff(ic);
#pragma unroll 1
  for (size_t k = 0; k < n_inputs; k++) {
    const uint64_t* xw = inputs + 4 * (n_inputs * i + k);
    const uint64_t x = SOUND ? (xw[0] | xw[1] | xw[2] | xw[3]) : xw[0];
    ic.x = {pr_fq_load(vk + VK_IC + 24 * (k + 1))};
    ic.y = {pr_fq_load(vk + VK_IC + 24 * (k + 1) + 12)};
    if (!x || aff_is_inf(ic)) continue;
    if constexpr (SOUND) acc = xyzz_add(acc, pr_g1_mul255(&ic, xw));
    else acc = xyzz_add(acc, pr_g1_mul64(&ic, x));
  }
  const bool ic_inf = xyzz_is_inf(acc);
  if (!ic_inf) ic = pr_g1_affine(acc);
  // e(A, B) e(-IC, gamma) e(-C, delta), then the constant e(-alpha, beta)
  pr_use_g1(in, 0, A, !a_inf && !b_inf);
  pr_use_g1(in, 1, aff_neg(ic), !ic_inf && vk[VK_ON] != 0);
  pr_use_g1(in, 2, aff_neg(Cp), !c_inf && vk[VK_ON + 1] != 0);
  in.tab[0] = vk + VK_TAB;
  in.tab[1] = vk + VK_TAB + 48 * PR_STEPS;
  F12 f, g;
  pr_miller(&f, &in);
  f12_conj(&f, &f);
  F2* gc = &g.c0.c0;
#pragma unroll 1
  for (int j = 0; j < 6; j++) gc[j] = f2_load(vk + VK_AB + 24 * j);
  f12_mul(&f, &f, &g);
  f12_final_exp(&f);
  status[i] = f12_is_one(&f) ? ZK_VERIFY_ACCEPT : ZK_VERIFY_REJECT;
}

// The same check with IC given (a prepared key, prepared.hip): IC is not summed
// here but read from sums[i] -- 24 words, (0, 0) the identity -- and in_ok[i] = 0
// (an input out of range) makes the proof MALFORMED.  A kernel of its own and not
// a second instance of the one above: with the body shared through an inlined
// template the compiler laid out k_groth16_verify's scratch differently and
// its code changed (tools/kernel_same.py), which this feature must not do.
__global__ void __launch_bounds__(PR_BLOCK) k_groth16_verify_given(const uint64_t* __restrict__ proofs,
                                                                   const G1A* __restrict__ sums,
                                                                   const uint8_t* __restrict__ in_ok,
                                                                   const uint32_t* __restrict__ vk, size_t n,
                                                                   uint8_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint64_t* w = proofs + PROOF_WORDS * i;
  PrPairs in;
  Affine<FqC> A, Cp, ic;
  bool a_inf, b_inf, c_inf;
  bool ok = pr_load_g1(w, &A, &a_inf);
  ok = pr_load_g2(w + G1W, &in.Q, &b_inf) && ok;
  ok = pr_load_g1(w + G1W + G2W, &Cp, &c_inf) && ok;
  if (!ok || !in_ok[i]) {
    status[i] = ZK_VERIFY_MALFORMED;
    return;
  }
  const uint32_t* sw = reinterpret_cast<const uint32_t*>(sums + i);
  ic.x = {pr_fq_load(sw)};
  ic.y = {pr_fq_load(sw + 12)};
  pr_use_g1(in, 0, A, !a_inf && !b_inf);
  pr_use_g1(in, 1, aff_neg(ic), !aff_is_inf(ic) && vk[VK_ON] != 0);
  pr_use_g1(in, 2, aff_neg(Cp), !c_inf && vk[VK_ON + 1] != 0);
  in.tab[0] = vk + VK_TAB;
  in.tab[1] = vk + VK_TAB + 48 * PR_STEPS;
  F12 f, g;
  pr_miller(&f, &in);
  f12_conj(&f, &f);
  F2* gc = &g.c0.c0;
#pragma unroll 1
  for (int j = 0; j < 6; j++) gc[j] = f2_load(vk + VK_AB + 24 * j);
  f12_mul(&f, &f, &g);
  f12_final_exp(&f);
  status[i] = f12_is_one(&f) ? ZK_VERIFY_ACCEPT : ZK_VERIFY_REJECT;
}

// One lane per product of k pairings, each through the on-the-fly loop
__global__ void __launch_bounds__(PR_BLOCK) k_pairing_products(const uint64_t* __restrict__ g1,
                                                               const uint64_t* __restrict__ g2, size_t k, size_t n,
                                                               uint8_t* __restrict__ status) {
  const size_t i = (size_t)blockIdx.x * PR_BLOCK + threadIdx.x;
  if (i >= n) return;
  PrPairs in;
  in.on[1] = in.on[2] = false;
  in.tab[0] = in.tab[1] = nullptr;
  F12 f, g;
  f12_set_one(&f);
  bool ok = true;
#pragma unroll 1
  for (size_t j = 0; j < k; j++) {
    Affine<FqC> P;
    bool p_inf, q_inf;
    bool good = pr_load_g1(g1 + G1W * (k * i + j), &P, &p_inf);
    good = pr_load_g2(g2 + G2W * (k * i + j), &in.Q, &q_inf) && good;
    ok = ok && good;
    if (!good || p_inf || q_inf) continue;
    pr_use_g1(in, 0, P, true);
    pr_miller(&g, &in);
    f12_mul(&f, &f, &g);
  }
  if (!ok) {
    status[i] = ZK_VERIFY_MALFORMED;
    return;
  }
  f12_conj(&f, &f);
  f12_final_exp(&f);
  status[i] = f12_is_one(&f) ? ZK_VERIFY_ACCEPT : ZK_VERIFY_REJECT;
}

// ---- per-call data (host) ------------------------------------------------------
void put_fq(uint32_t* out, const host::Fq& m) {
  const host::Fq d = host::to_dev(m);
  std::memcpy(out, d.l, 48);
}
static void put_fq2(uint32_t* out, const host::Fq2& m) {
  put_fq(out, m.c0);
  put_fq(out + 12, m.c1);
}
// The slopes of host_pairing.hpp's miller_loop for Q, step by step: lambda'
// and lambda' x' - y' (line_eval's c0.c0), 48 words per step.
void line_table(const host::A2& Q, uint32_t* out) {
  host::Fq2 tx = Q.x, ty = Q.y;
  int step = 0;
  for (int i = 62; i >= 0; i--) {
    const host::Fq2 x2 = sqr(tx);
    const host::Fq2 lam = mul(add(add(x2, x2), x2), inv(add(ty, ty)));
    put_fq2(out + 48 * step, lam);
    put_fq2(out + 48 * step + 24, sub(mul(lam, tx), ty));
    step++;
    const host::Fq2 nx = sub(sub(sqr(lam), tx), tx);
    ty = sub(mul(lam, sub(tx, nx)), ty);
    tx = nx;
    if ((BLS_X_ABS >> i) & 1) {
      const host::Fq2 la = mul(sub(Q.y, ty), inv(sub(Q.x, tx)));
      put_fq2(out + 48 * step, la);
      put_fq2(out + 48 * step + 24, sub(mul(la, tx), ty));
      step++;
      const host::Fq2 ax = sub(sub(sqr(la), tx), Q.x);
      ty = sub(mul(la, sub(tx, ax)), ty);
      tx = ax;
    }
  }
  if (step != PR_STEPS) throw Error(ZK_ERR_DEVICE, "pairing line table: step count");
}
// Every point of the key is validated here (alpha, beta, gamma, delta and all
// ic_len entries): false for a malformed one.
bool pairing_tables(const zk_vk& vk, size_t n_inputs, std::vector<uint32_t>& out) {
  host::A1 alpha, p;
  host::A2 beta, gamma, delta;
  if (!host::load(vk.alpha_g1, alpha) || !host::load(vk.beta_g2, beta) || !host::load(vk.gamma_g2, gamma) ||
      !host::load(vk.delta_g2, delta))
    return false;
  out.assign(VK_IC + 24 * (n_inputs + 1), 0);
  if (!alpha.inf) alpha.y = host::neg(alpha.y);
  const host::Fq12 ab = host::miller_loop(alpha, beta);
  const host::Fq2* co = &ab.c0.c0;
  for (int j = 0; j < 6; j++) put_fq2(&out[VK_AB + 24 * j], co[j]);
  if (!gamma.inf) line_table(gamma, &out[VK_TAB]);
  if (!delta.inf) line_table(delta, &out[VK_TAB + 48 * PR_STEPS]);
  out[VK_ON] = gamma.inf ? 0 : 1;
  out[VK_ON + 1] = delta.inf ? 0 : 1;
  for (size_t k = 0; k < vk.ic_len; k++) {
    if (!host::load(vk.ic_g1[k], p)) return false;
    if (k > n_inputs || p.inf) continue;
    put_fq(&out[VK_IC + 24 * k], p.x);
    put_fq(&out[VK_IC + 24 * k + 12], p.y);
  }
  return true;
}

// ---- drivers -------------------------------------------------------------------------
// As points_run: the batch crosses the GPU in chunks of ctx->verify_chunk
// proofs (products) on the ctx's main stream; buffers belong to the call.
// bytes (zk_groth16_verify_many_bytes): the chunk goes up as 192-byte
// compressed proofs and the proof decoder (points.hip) writes the zk_proof
// records into the buffer the verify kernel reads -- decoded proofs never
// visit the host.  An invalid point's words are all zero, infinity word
// included, and (0, 0) is on neither curve: pr_load_g1 / pr_load_g2 refuse it,
// which makes the proof MALFORMED with the verify kernel unchanged (it does
// not read the point statuses).
// pvk (vk then unused): a prepared key.  Its words are on the device already,
// its mode is the call's, and per chunk prepared.hip's sum kernels run ahead of
// the verify kernel, which reads IC instead of summing it.
static int verify_many_run(zk_ctx* ctx, const zk_vk* vk, const zk_vk_dev* pvk, const zk_proof* proofs,
                           const uint8_t* bytes, const zk_fr* inputs, size_t n_inputs, size_t n, uint8_t* status,
                           uint8_t* point_status, bool sound) {
  if (n_inputs != (pvk ? pvk->num_public : vk->num_public)) return ZK_ERR_INVALID_WITNESS;
  std::vector<uint32_t> tables;
  if (!pvk) {
    if (!vk->ic_g1 || vk->ic_len < n_inputs + 1) {
      ctx->err = "verification key: ic_g1 shorter than the public inputs";
      return ZK_ERR_ARG;
    }
    if (!pairing_tables(*vk, n_inputs, tables)) {
      ctx->err = "verification key: a point is not canonical or not on its curve";
      return ZK_ERR_ARG;
    }
  } else if (pvk->device != ctx->device) {
    ctx->err = "prepared verification key: made on another device";
    return ZK_ERR_ARG;
  }
  if (!n) return ZK_OK;
  hipStream_t st = ctx->stream;
  const size_t chunk = std::min<size_t>(ctx->verify_chunk, n), in_sz = sizeof(zk_fr) * n_inputs;
  DevBuf d_vk, d_proofs, d_in, d_st, d_bytes, d_pst;
  PrepWork sums;
  if (!pvk) d_vk.ensure(4 * tables.size());
  d_proofs.ensure(sizeof(zk_proof) * chunk);
  d_in.ensure(std::max<size_t>(in_sz * chunk, 16));
  d_st.ensure(chunk);
  if (bytes) {
    d_bytes.ensure(192 * chunk);
    d_pst.ensure(3 * chunk);
  }
  if (!pvk) ZK_HIP(hipMemcpyAsync(d_vk.p, tables.data(), 4 * tables.size(), hipMemcpyHostToDevice, st));
  for (size_t lo = 0; lo < n; lo += chunk) {
    const size_t m = std::min(chunk, n - lo);
    if (bytes) {
      ZK_HIP(hipMemcpyAsync(d_bytes.p, bytes + 192 * lo, 192 * m, hipMemcpyHostToDevice, st));
      proofs_decode_launch(ctx, st, d_bytes.as<uint8_t>(), m, d_proofs.as<uint64_t>(), d_pst.as<uint8_t>());
    } else {
      ZK_HIP(hipMemcpyAsync(d_proofs.p, proofs + lo, sizeof(zk_proof) * m, hipMemcpyHostToDevice, st));
    }
    if (in_sz) ZK_HIP(hipMemcpyAsync(d_in.p, inputs + n_inputs * lo, in_sz * m, hipMemcpyHostToDevice, st));
    if (pvk) prepared_sums_launch(ctx, st, pvk, d_in.as<uint64_t>(), m, sums);
    const int pi = ctx->prof.begin(st, "verify", m);
    if (pvk)
      k_groth16_verify_given<<<ceil_div(m, PR_BLOCK), PR_BLOCK, 0, st>>>(
          d_proofs.as<uint64_t>(), sums.ic.as<G1A>(), sums.ok.as<uint8_t>(), pvk->words.as<uint32_t>(), m,
          d_st.as<uint8_t>());
    else if (sound)
      k_groth16_verify<true><<<ceil_div(m, PR_BLOCK), PR_BLOCK, 0, st>>>(
          d_proofs.as<uint64_t>(), d_in.as<uint64_t>(), n_inputs, d_vk.as<uint32_t>(), m, d_st.as<uint8_t>());
    else
      k_groth16_verify<false><<<ceil_div(m, PR_BLOCK), PR_BLOCK, 0, st>>>(
          d_proofs.as<uint64_t>(), d_in.as<uint64_t>(), n_inputs, d_vk.as<uint32_t>(), m, d_st.as<uint8_t>());
    ZK_LAUNCH_CHECK();
    ctx->prof.end(st, pi);
    ZK_HIP(hipMemcpyAsync(status + lo, d_st.p, m, hipMemcpyDeviceToHost, st));
    if (point_status) ZK_HIP(hipMemcpyAsync(point_status + 3 * lo, d_pst.p, 3 * m, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));   // the next chunk reuses the buffers
  }
  if (ctx->prof.on) ctx->prof.collect();
  return ZK_OK;
}

// m products of k pairs each in device memory -> m statuses in device memory, on st
void pairing_products_launch(zk_ctx* ctx, hipStream_t st, const uint64_t* d_g1, const uint64_t* d_g2, size_t k,
                             size_t m, uint8_t* d_st) {
  if (!m) return;
  const int pi = ctx->prof.begin(st, "verify", m);
  k_pairing_products<<<ceil_div(m, PR_BLOCK), PR_BLOCK, 0, st>>>(d_g1, d_g2, k, m, d_st);
  ZK_LAUNCH_CHECK();
  ctx->prof.end(st, pi);
}

static int pairing_products_run(zk_ctx* ctx, const zk_g1_affine* g1, const zk_g2_affine* g2, size_t k, size_t n,
                                uint8_t* status) {
  if (!n) return ZK_OK;
  hipStream_t st = ctx->stream;
  const size_t chunk = std::min<size_t>(ctx->verify_chunk, n);
  DevBuf d_g1, d_g2, d_st;
  d_g1.ensure(std::max<size_t>(sizeof(zk_g1_affine) * k * chunk, 16));
  d_g2.ensure(std::max<size_t>(sizeof(zk_g2_affine) * k * chunk, 16));
  d_st.ensure(chunk);
  for (size_t lo = 0; lo < n; lo += chunk) {
    const size_t m = std::min(chunk, n - lo);
    if (k) {
      ZK_HIP(hipMemcpyAsync(d_g1.p, g1 + k * lo, sizeof(zk_g1_affine) * k * m, hipMemcpyHostToDevice, st));
      ZK_HIP(hipMemcpyAsync(d_g2.p, g2 + k * lo, sizeof(zk_g2_affine) * k * m, hipMemcpyHostToDevice, st));
    }
    const int pi = ctx->prof.begin(st, "verify", m);
    k_pairing_products<<<ceil_div(m, PR_BLOCK), PR_BLOCK, 0, st>>>(d_g1.as<uint64_t>(), d_g2.as<uint64_t>(), k, m,
                                                                   d_st.as<uint8_t>());
    ZK_LAUNCH_CHECK();
    ctx->prof.end(st, pi);
    ZK_HIP(hipMemcpyAsync(status + lo, d_st.p, m, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
  }
  if (ctx->prof.on) ctx->prof.collect();
  return ZK_OK;
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

int zk_groth16_verify_many(zk_ctx* ctx, const zk_vk* vk, const zk_proof* proofs, const zk_fr* public_inputs,
                           size_t n_inputs, size_t n_proofs, uint8_t* status) {
  if (!ctx || !vk || (n_proofs && (!proofs || !status || (n_inputs && !public_inputs)))) return ZK_ERR_ARG;
  ZK_PGUARD(ctx, {
    return verify_many_run(ctx, vk, nullptr, proofs, nullptr, public_inputs, n_inputs, n_proofs, status, nullptr,
                           false);
  })
}
int zk_groth16_verify_many_sound(zk_ctx* ctx, const zk_vk* vk, const zk_proof* proofs, const zk_fr* public_inputs,
                                 size_t n_inputs, size_t n_proofs, uint8_t* status) {
  if (!ctx || !vk || (n_proofs && (!proofs || !status || (n_inputs && !public_inputs)))) return ZK_ERR_ARG;
  ZK_PGUARD(ctx, {
    return verify_many_run(ctx, vk, nullptr, proofs, nullptr, public_inputs, n_inputs, n_proofs, status, nullptr, true);
  })
}
int zk_groth16_verify_many_bytes(zk_ctx* ctx, const zk_vk* vk, const uint8_t* proofs, const zk_fr* public_inputs,
                                 size_t n_inputs, size_t n_proofs, uint8_t* status, uint8_t* point_status) {
  if (!ctx || !vk || (n_proofs && (!proofs || !status || (n_inputs && !public_inputs)))) return ZK_ERR_ARG;
  ZK_PGUARD(ctx, {
    return verify_many_run(ctx, vk, nullptr, nullptr, proofs, public_inputs, n_inputs, n_proofs, status, point_status,
                           false);
  })
}
int zk_groth16_verify_many_bytes_sound(zk_ctx* ctx, const zk_vk* vk, const uint8_t* proofs, const zk_fr* public_inputs,
                                       size_t n_inputs, size_t n_proofs, uint8_t* status, uint8_t* point_status) {
  if (!ctx || !vk || (n_proofs && (!proofs || !status || (n_inputs && !public_inputs)))) return ZK_ERR_ARG;
  ZK_PGUARD(ctx, {
    return verify_many_run(ctx, vk, nullptr, nullptr, proofs, public_inputs, n_inputs, n_proofs, status, point_status,
                           true);
  })
}
// the same drivers with a prepared key: the mode is the key's
int zk_groth16_verify_many_prepared(zk_ctx* ctx, const zk_vk_dev* pvk, const zk_proof* proofs,
                                    const zk_fr* public_inputs, size_t n_inputs, size_t n_proofs, uint8_t* status) {
  if (!ctx || !pvk || (n_proofs && (!proofs || !status || (n_inputs && !public_inputs)))) return ZK_ERR_ARG;
  ZK_PGUARD(ctx, {
    return verify_many_run(ctx, nullptr, pvk, proofs, nullptr, public_inputs, n_inputs, n_proofs, status, nullptr,
                           pvk->sound);
  })
}
int zk_groth16_verify_many_bytes_prepared(zk_ctx* ctx, const zk_vk_dev* pvk, const uint8_t* proofs,
                                          const zk_fr* public_inputs, size_t n_inputs, size_t n_proofs,
                                          uint8_t* status, uint8_t* point_status) {
  if (!ctx || !pvk || (n_proofs && (!proofs || !status || (n_inputs && !public_inputs)))) return ZK_ERR_ARG;
  ZK_PGUARD(ctx, {
    return verify_many_run(ctx, nullptr, pvk, nullptr, proofs, public_inputs, n_inputs, n_proofs, status,
                           point_status, pvk->sound);
  })
}
int zk_pairing_products(zk_ctx* ctx, const zk_g1_affine* g1, const zk_g2_affine* g2, size_t pairs_per_product,
                        size_t n_products, uint8_t* status) {
  if (!ctx || (n_products && (!status || (pairs_per_product && (!g1 || !g2))))) return ZK_ERR_ARG;
  ZK_PGUARD(ctx, { return pairing_products_run(ctx, g1, g2, pairs_per_product, n_products, status); })
}
