// prove.hip -- Groth16 prove() orchestration on one GPU.
//
// Restates Prover::prove (crates/groth16-core/src/lib.rs:139-272) with the
// reference's arithmetic, quirks included:
//   w_i = lo64(z_i)                                         core:156-161
//   pi_A = alpha_1 + sum w_i a_g1[i] + r delta_1            core:164-179
//   pi_B = beta_2  + sum w_i b_g2[i] + s delta_2            core:182-197
//   H    = (A B - C) / (x^n - 1), h_i = lo64(H_i)           core:200-208, qap:225-271
//   H_1  = sum h_i h_g1[i]                                  core:211-221
//   B_1  = beta_1  + sum w_i b_g1[i]                        core:246-255
//   pi_C = sum_{i>l} w_i ic_g1[i-l-1] + H_1 + s pi_A + r B_1  core:224-265
// Every sum is one device MSM with 64-bit scalars: the full-width terms
// r*delta_1 and s*delta_2 are split as sum_k r_k (2^(64k) delta) over four
// precomputed bases (appended when the key is built, key.hip), identity bases
// are compacted away there (they contribute nothing), and only s*pi_A + r*B_1 -- which
// depend on this proof's own MSM outputs -- are formed on the host.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <thread>

#include "dist.hpp"
#include "prove.hpp"
#include "quotient.hpp"

namespace zk {

// (Az)_j, (Bz)_j, (Cz)_j for every domain row (rows >= nc are zero padding,
// qap:155-164) plus the witness checks:
//   flags bit 0: row vrow unsatisfied      -> InvalidWitness (core:121-128: the
//                reference checks A(w)B(w) = C(w) at w = omega, i.e. row 1,
//                or row 0 when n == 1)
//   flags bit 1: some row unsatisfied      -> PolynomialDivisionFailed (qap:266)
//   flags bit 2: z_0 != 1                  -> InvalidWitness (core:89-93)
__global__ void __launch_bounds__(256) k_csr_eval(CsrArgs m, const Fr* __restrict__ zc, uint64_t nc, uint64_t V,
                                                  uint64_t n, uint64_t vrow, Fr* __restrict__ qa,
                                                  Fr* __restrict__ qb, Fr* __restrict__ qc,
                                                  uint32_t* __restrict__ flags) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j == 0) {
    Fr z0 = ld_vec(&zc[0]);
    bool one = z0.v[0] == 1;
#pragma unroll
    for (int i = 1; i < 8; i++) one = one && z0.v[i] == 0;
    if (!one) atomicOr(flags, 4u);
  }
  if (j >= n) return;
  Fr a = fp_zero<FrParams>(), b = a, c = a;
  if (j < nc) {
    a = row_dot(m.rp[0], m.col[0], m.val[0], j, zc, V);
    b = row_dot(m.rp[1], m.col[1], m.val[1], j, zc, V);
    c = row_dot(m.rp[2], m.col[2], m.val[2], j, zc, V);
    if (!fp_eq(fp_mul(a, b), c)) atomicOr(flags, j == vrow ? 3u : 2u);
  }
  st_vec(&qa[j], a);
  st_vec(&qb[j], b);
  st_vec(&qc[j], c);
}

__global__ void __launch_bounds__(256) k_quot_pointwise(Fr* __restrict__ qa, const Fr* __restrict__ qb,
                                                        const Fr* __restrict__ qc, const Fr* __restrict__ zinv,
                                                        size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fr t = fp_sub(fp_mul(ld_vec(&qa[i]), ld_vec(&qb[i])), ld_vec(&qc[i]));
  st_vec(&qa[i], fp_mul(t, ld_vec(zinv)));
}

__device__ __forceinline__ uint32_t brev(uint32_t x, uint32_t log_n) {
  return log_n ? (__builtin_bitreverse32(x) >> (32 - log_n)) : 0;
}

// The kernels below write MSM scalars of SW u64 words: 1, the lo64 of the
// reference (core:156-161, 203-208), or 4, whole, for a sound key
// (zk_pk_dev::sound).  st_scal<SW> (quotient.hpp) is the only difference.
//
// H_i = n^-1 g^-i * (bit-reversed iNTT output)[i] as a scalar: the
// element-wise gather path for domains that stay in the MALL
template <int SW>
__global__ void __launch_bounds__(256) k_h_final(const Fr* __restrict__ hb, const Fr* __restrict__ gipow,
                                                 uint32_t log_n, uint64_t* __restrict__ h) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >> log_n) return;
  st_scal<SW>(h, i, fp_mul(ld_vec(&hb[brev((uint32_t)i, log_n)]), ld_vec(&gipow[i])));
}
static void h_final(const Fr* hb, const Fr* gipow, uint32_t log_n, int sw, uint64_t* h, hipStream_t st) {
  const uint32_t nb = ceil_div((size_t)1 << log_n, 256);
  if (sw == 1) k_h_final<1><<<nb, 256, 0, st>>>(hb, gipow, log_n, h);
  else k_h_final<4><<<nb, 256, 0, st>>>(hb, gipow, log_n, h);
  ZK_LAUNCH_CHECK();
}

// n Montgomery Fr -> scalars (the quotient's natural-order path, where
// n^-1 g^-i is already applied; setup's tau powers)
template <int SW>
__global__ void __launch_bounds__(256) k_fr_scalars(const Fr* __restrict__ in, size_t n, uint64_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) st_scal<SW>(out, i, ld_vec(&in[i]));
}
void fr_to_scalars(const Fr* d_in, size_t n, int sw, uint64_t* d_out, hipStream_t st) {
  if (!n) return;
  if (sw == 1) k_fr_scalars<1><<<ceil_div(n, 256), 256, 0, st>>>(d_in, n, d_out);
  else k_fr_scalars<4><<<ceil_div(n, 256), 256, 0, st>>>(d_in, n, d_out);
  ZK_LAUNCH_CHECK();
}

// out[k] = scalar idx[k] / div of src (canonical).  SW = 1: its low word, the
// scalars stride_words apart (4: a witness, 1: lo64(H)); div > 1: a
// distributed-quotient rank holds H_(rank + div d) at position d.  SW = 4:
// whole canonical Fr; a sound key is never sharded (div = 1).
template <int SW>
__global__ void __launch_bounds__(256) k_gather(const uint64_t* __restrict__ src, int stride_words,
                                                const uint32_t* __restrict__ idx, uint32_t div, uint32_t count,
                                                uint64_t* __restrict__ out) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  if constexpr (SW == 1) out[k] = src[(size_t)(idx[k] / div) * stride_words];
  else st_vec(reinterpret_cast<Fr*>(out) + k, ld_vec(reinterpret_cast<const Fr*>(src) + idx[k]));
}
static void gather_scalars(const uint64_t* src, int stride_words, const uint32_t* idx, uint32_t div, uint32_t count,
                           int sw, uint64_t* out, hipStream_t st) {
  if (!count) return;
  if (sw == 1) k_gather<1><<<ceil_div(count, 256), 256, 0, st>>>(src, stride_words, idx, div, count, out);
  else k_gather<4><<<ceil_div(count, 256), 256, 0, st>>>(src, stride_words, idx, div, count, out);
  ZK_LAUNCH_CHECK();
}

// an MSM's extras' scalars: 1, then r or s -- as five one-word scalars
// [1, r0..r3], or as two whole ones [1,0,0,0, r0..r3]
struct Extras {
  uint64_t v[8];
};
__global__ void k_set_extras(uint64_t* __restrict__ dst, Extras e, uint32_t nwords) {
  if (threadIdx.x < nwords) dst[threadIdx.x] = e.v[threadIdx.x];
}

// flags bit 3: some z_i >= r.  The reference's assignment is a vector of
// reduced Fr (core:40-44), so a non-canonical limb vector has no reference
// meaning (its lo64 would differ from the reduced value's): ZK_ERR_ARG.
__global__ void __launch_bounds__(256) k_check_canonical(const Fr* __restrict__ z, uint64_t n,
                                                         uint32_t* __restrict__ flags) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (!fr_lt_r(ld_vec(&z[i]))) atomicOr(flags, 8u);
}

void check_canonical(const void* d_z, uint64_t n, uint32_t* d_flags, hipStream_t st) {
  if (!n) return;
  k_check_canonical<<<ceil_div(n, 256), 256, 0, st>>>(reinterpret_cast<const Fr*>(d_z), n, d_flags);
  ZK_LAUNCH_CHECK();
}

bool fr_canonical(const zk_fr& a) {
  for (int i = 3; i >= 0; i--)
    if (a.l[i] != FR_MOD64[i]) return a.l[i] < FR_MOD64[i];
  return false;
}

// ---------------------------------------------------------------- prove ---
// Partial accumulators of one shard (host XYZZ, Montgomery).  SC = s A + r B1
// of this shard's A / B1 sums: by linearity the shards' SC add up to the
// s pi_A + r B_1 of pi_C (core:224-265), so each rank pays for its own two
// scalar multiplications while its H MSM is still running.
struct Partial {
  host::X<host::Fq> A, B1, IC, H, SC;
  host::X<host::Fq2> B2;
  int32_t status;
};
static_assert(sizeof(Partial) <= ZK_PARTIAL_BYTES, "partial size");

// h_out: H_i as scalars of sw words per coefficient (1: lo64(H_i), 4: the
// whole canonical H_i)
static void quotient(zk_ctx* ctx, const zk_pk_dev* pk, const uint64_t* d_z, int sw, hipStream_t st, uint64_t* h_out) {
  const uint64_t n = pk->n;
  NttDomain& dom = ctx->domain(pk->log_n);
  ctx->qabc.ensure(sizeof(Fr) * 3 * n);
  Fr* v[3] = {ctx->qabc.as<Fr>(), ctx->qabc.as<Fr>() + n, ctx->qabc.as<Fr>() + 2 * n};
  const CsrArgs m = csr_args(pk->csr);
  const uint64_t vrow = n > 1 ? 1 : 0;
  Prof* pf = &ctx->prof;
  int ph = pf->begin(st, "quotient_eval", n);
  k_csr_eval<<<ceil_div(n, 256), 256, 0, st>>>(m, reinterpret_cast<const Fr*>(d_z), pk->nc, pk->V, n, vrow,
                                                v[0], v[1], v[2], ctx->flags.as<uint32_t>());
  ZK_LAUNCH_CHECK();
  pf->end(st, ph);
  // per polynomial: iNTT (coefficients * n, bit-reversed), * n^-1 g^i, NTT
  // (evaluations on the coset g<w>, natural order).  Fused into one tile
  // kernel below 2^LARGE_Q_LOG; from there the three steps run as separate
  // passes, and the final coset iNTT runs in natural order (ntt_natural)
  // instead of a DIF plus an element-wise bit-reversed gather.  Same-box
  // A/B, overlapped prove: 2^24 fused 122.8 / separate 118.6 ms; 2^20 the
  // gather path 9.89 / natural 10.01 ms (profiles/r02_ab_quot.txt).  One
  // launch per pass for all three polynomials (nb = 3) lost 0.2 ms in the
  // overlapped prove (profiles/r03_ab_batchq_fan8_rcw4_rejected.txt).
  // zk_ctx_set_option(ZK_OPT_QUOTIENT_PATH) forces either path (tests).
  constexpr uint32_t LARGE_Q_LOG = 23;
  const bool large = ctx->quot_path >= 0 ? ctx->quot_path == 1 : pk->log_n >= LARGE_Q_LOG;
  for (int k = 0; k < 3; k++) {
    if (!large) {
      ntt_coset_shift(v[k], dom, domain_gpow_br(dom, st), st, pf);
      continue;
    }
    ntt_dif(v[k], dom, /*inverse twiddles*/ true, st, pf);
    ph = pf->begin(st, "quotient_misc", n);
    fr_scale_table(v[k], domain_gpow_br(dom, st), pk->log_n, false, st);
    pf->end(st, ph);
    ntt_dit(v[k], dom, false, st, pf);
  }
  ph = pf->begin(st, "quotient_misc", n);
  k_quot_pointwise<<<ceil_div(n, 256), 256, 0, st>>>(v[0], v[1], v[2], dom.zinv.as<Fr>(), n);
  ZK_LAUNCH_CHECK();
  pf->end(st, ph);
  // coset iNTT: small domains run a DIF and gather its bit-reversed output
  // element by element (k_h_final, all in the MALL); large ones run it in
  // natural order (the bit reversal is the first pass's tiled gather,
  // n^-1 g^-i fused into the last pass's store) into v[1], v[2] as scratch,
  // since beyond the MALL every gathered 32-B element was its own line/page
  ctx->tmp_scal.ensure(sizeof(uint64_t) * sw * n);
  if (!large) {
    ntt_dif(v[0], dom, true, st, pf);
    ph = pf->begin(st, "quotient_misc", n);
    h_final(v[0], domain_gipow(dom, st), pk->log_n, sw, h_out, st);
    pf->end(st, ph);
    return;
  }
  Fr* h = v[1];
  if (pk->log_n == 0) {   // a size-1 transform is the identity: only the factor
    fr_scale_table(v[0], domain_gipow(dom, st), 0, false, st);
    h = v[0];
  } else {
    ntt_natural(v[1], v[0], v[2], dom, true, st, pf, nullptr, domain_gipow(dom, st), nullptr);
  }
  ph = pf->begin(st, "quotient_misc", n);
  fr_to_scalars(h, n, sw, h_out, st);
  pf->end(st, ph);
}

// A sharded key whose ctx is attached to the matching exchange (an RCCL
// communicator, or a host-staged one) computes its quotient distributed
// (three all-to-alls per proof).
// zk_ctx_set_option(ZK_OPT_DIST_QUOTIENT, 0) turns it off: every rank then
// computes the whole quotient (bench.py's replicated-quotient comparison).
// exchange_matches: such an exchange is attached, whatever the option -- the
// ranks then agree on the mode before every proof (prove_partial_common).
static bool exchange_matches(const zk_ctx* ctx, const zk_pk_dev* pk) {
  return pk->nshards > 1 && ctx->exch && ctx->exch->world == (int)pk->nshards &&
         ctx->exch->rank == (int)pk->shard && dist_quotient_ok(pk->n, (int)pk->nshards);
}
static bool uses_dist_quotient(const zk_ctx* ctx, const zk_pk_dev* pk) {
  return ctx->dist_quotient != 0 && exchange_matches(ctx, pk);
}

// a proof's status from its witness-check flags (k_csr_eval, k_check_canonical)
static int status_from_flags(uint32_t flags) {
  if (flags & 8u) return ZK_ERR_ARG;
  if (flags & 5u) return ZK_ERR_INVALID_WITNESS;
  if (flags & 2u) return ZK_ERR_QAP_DIVISION;
  return ZK_OK;
}

// The G1 MSMs run as two groups: A and B1, which need only z, start with the
// witness; IC and H -- both terms of pi_C = IC + H_1 + s pi_A + r B_1
// (core:224-265), so ONE MSM over the bases [ic_g1 | h_g1] with the scalars
// [z_i | H_i] -- follows the quotient.  One bucket set for IC and H: a bucket
// reduction fewer per proof than IC in the first group and H alone.
// The key's mode enters as sw, the u64 words of a scalar: 1 (lo64, the
// reference) or 4 (whole, a sound key), with the key's scalar_bits and window
// copies.  The same groups on the same streams either way; how a group's
// slots become MSMs -- at sw = 1 one batch (msm_launch_batch: one sort,
// accumulate, merge and bucket reduction, so the latency-bound tails cost one
// tree depth per group) -- is ProveRun::launch_g1's decision alone.
static const int G1_AB[2] = {MSM_A, MSM_B1};
static const int G2_B[1] = {MSM_B2}, G1_ICH[1] = {MSM_H};
static const int WAITS[3] = {MSM_B2, MSM_A, MSM_H};   // MSM_A: the A + B1 group, MSM_H: IC + H
// per-MSM profiling prefixes of the slots (MSM_H: [IC | H]); "AB/": A + B1 as one batch
static const char* const SLOT_TAG[5] = {"A/", "B2/", "B1/", "IC/", "ICH/"};

// What one shard's proof is made from, beside the key, r and s: the device witness d_z, and
// h_given (virtual-rank tests): this shard's lo64(H_(shard + nshards d)) is
// already on the device, with the witness-check flags of all ranks.
// ranges: only these [lo, hi) entries of d_z are valid (a witness slice),
// else all of [0, V).
// early (the one-GPU prove): pi_A and pi_B in their affine ABI form as soon
// as those MSMs are done, while H is still on the GPU -- each conversion is
// a field inversion (~40 us on one core) that would otherwise follow the
// last MSM.
// z_host (the drop-in host-witness prove): d_z is the ctx's device copy,
// filled here in HOST_PARTS parts (pk_part_cuts) -- and the G2 and A+B1+IC
// MSMs run split the same way: part k's keys, sort and accumulate start as
// soon as its slice of z has landed, while the next slice is still crossing
// PCIe; each later part adds the previous part's completed buckets
// (msm_batch_back ACCUM / COMBINE) and the last one reduces once.
struct ProveInput {
  const uint64_t* d_z = nullptr;
  const uint64_t* h_given = nullptr;
  uint32_t given_flags = 0;
  const std::vector<uint64_t>* ranges = nullptr;
  zk_proof* early = nullptr;
  const zk_fr* z_host = nullptr;
};

using clk = std::chrono::steady_clock;
static double ms_since(clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); }

// One prove_partial call: what it decides up front, then its steps in order.
struct ProveRun {
  const clk::time_point t_start = clk::now();
  Range range_prove{"zk_prove"};
  zk_ctx* const ctx;
  const zk_pk_dev* const pk;
  const zk_fr *const r, *const s;
  const ProveInput in;
  const hipStream_t st;
  const bool split;   // a host witness, uploaded in parts
  // Streams (<= GPU_MAX_HW_QUEUES = 4, so no two share a hardware queue):
  // main (high priority) runs the quotient and then the IC+H group that
  // depends on it; side[0] (high) the G2 MSM, the longest chain; side[1] the
  // A + B1 group and IC's gather.  The latency-bound phases of one MSM overlap the throughput-bound
  // accumulation of another.  Schedule 3 runs everything in order on main.
  const bool serial;
  const hipStream_t s_g2, s_abi;
  // u64 words and bits of every scalar: 1 and 64 (its lo64), or 4 and 255 for
  // a sound key (whole, over the key's window copies)
  const int sw, bits;
  // The quotient: local (every coefficient), distributed over the ranks of
  // a sharded key (this rank's coefficients i = shard mod N), or given
  // (virtual-rank tests).
  const bool dist;
  const uint64_t* h_src;
  const uint32_t h_div;
  // IC+H scalars: [nic z_i | H_i], sw words each, H's straight from the quotient when h_direct
  const uint32_t nic;
  const bool h_direct;
  // IC's scalars need only z: gathered ahead of the quotient on the A+B1
  // stream (ev_ic), so that the IC+H grouping starts right after the quotient
  bool ic_ready = false;
  int ph_span = -1;
  bool flags_agreed = false;
  clk::time_point t_quot;

  ProveRun(zk_ctx* c, const zk_pk_dev* k, const zk_fr* r_, const zk_fr* s_, const ProveInput& i)
      : ctx(c), pk(k), r(r_), s(s_), in(i), st(c->stream), split(i.z_host != nullptr), serial(c->sched == 3),
        s_g2(serial ? st : c->side[0]), s_abi(serial ? st : c->side[1]),
        sw(k->sound() ? 4 : 1), bits((int)k->scalar_bits), dist(!i.h_given && uses_dist_quotient(c, k)),
        h_src(i.h_given ? i.h_given : c->tmp_scal.as<uint64_t>()), h_div((i.h_given || dist) ? k->nshards : 1),
        nic(k->count[MSM_IC]), h_direct(k->h_ident && !dist && !i.h_given) {
    // the split upload's parts are batches of one-word scalars (launch_part):
    // prove_impl sends a sound key's host witness up whole instead
    if (split && sw != 1) throw Error(ZK_ERR_ARG, "a split witness upload needs a reference-mode key");
  }

  uint32_t* flags() const { return ctx->flags.as<uint32_t>(); }
  uint64_t* scal(int slot) const { return ctx->scal[slot].as<uint64_t>(); }

  // part k of a host witness: variables [vcut[k], vcut[k+1]) to the device,
  // every z_i < r, else ZK_ERR_ARG (the host thread waits for a pageable copy)
  void upload_part(int k) {
    const uint64_t lo = pk->vcut[k], hi = pk->vcut[k + 1];
    if (hi > lo)
      ZK_HIP(hipMemcpyAsync(const_cast<uint64_t*>(in.d_z) + 4 * lo, in.z_host + lo, sizeof(zk_fr) * (hi - lo),
                            hipMemcpyHostToDevice, st));
    check_canonical(in.d_z + 4 * lo, hi - lo, flags(), st);
  }

  // flags reset, every z_i this proof reads < r (else ZK_ERR_ARG): ev_scal
  void check_witness() {
    ctx->flags.ensure(16);
    ctx->flags_host.ensure(16);
    ctx->prof.mark_origin(st);
    ph_span = ctx->prof.begin(st, "prove_gpu_span", pk->n);   // first kernel .. last MSM done
    ZK_HIP(hipMemsetAsync(ctx->flags.p, 0, 16, st));
    if (split) upload_part(0);
    else if (!in.ranges) check_canonical(in.d_z, pk->V, flags(), st);
    else
      for (size_t k = 0; k + 1 < in.ranges->size(); k += 2)
        check_canonical(reinterpret_cast<const Fr*>(in.d_z) + (*in.ranges)[k], (*in.ranges)[k + 1] - (*in.ranges)[k],
                        flags(), st);
    ZK_HIP(hipEventRecord(ctx->ev_scal, st));                     // z (and flags reset) ready
  }

  // ---- scalars of one MSM, sw words each: its variables' z (or H
  // coefficients), then the extras' scalars: 1 for alpha_1 / beta_2 / beta_1,
  // then r (delta_1) or s (delta_2) -- at sw = 1 its four u64 limbs, one each
  // for the key's bases 2^(64k) delta; at sw = 4 one whole scalar
  void set_extras(int slot, hipStream_t ss) {
    const uint32_t nex = pk->extras[slot];
    if (!nex) return;
    const zk_fr* whole = slot == MSM_A ? r : slot == MSM_B2 ? s : nullptr;
    Extras ex{};
    ex.v[0] = 1;
    if (whole) for (int k = 0; k < 4; k++) ex.v[sw + k] = whole->l[k];
    k_set_extras<<<1, 64, 0, ss>>>(scal(slot) + (size_t)sw * pk->count[slot], ex, sw * nex);
    ZK_LAUNCH_CHECK();
  }
  // z behind compacted positions [lo, hi) of an A / B2 / B1 slot ([0, count): all), and the extras
  void gather(int slot, uint32_t lo, uint32_t hi, bool extras, hipStream_t ss) {
    ctx->scal[slot].ensure(sizeof(uint64_t) * sw * std::max<uint32_t>(pk->count[slot] + pk->extras[slot], 1));
    if (hi > lo)
      gather_scalars(in.d_z, 4, pk->idx[slot].as<uint32_t>() + lo, 1u, hi - lo, sw, scal(slot) + (size_t)sw * lo, ss);
    if (extras) set_extras(slot, ss);
  }
  void gather_ic(hipStream_t ss) {
    gather_scalars(in.d_z, 4, pk->idx[MSM_IC].as<uint32_t>(), 1u, nic, sw, scal(MSM_H), ss);
  }
  void gather_ic_early() {
    gather_ic(s_abi);
    ZK_HIP(hipEventRecord(ctx->ev_ic, s_abi));
    ic_ready = true;
  }
  void gather_ich(hipStream_t ss) {
    if (!ic_ready) gather_ic(ss);
    // H's scalars sit sw words apart, a shard's H_(shard + h_div d) at d (a sound key: h_div = 1)
    if (!h_direct)
      gather_scalars(h_src, sw, pk->idx[MSM_H].as<uint32_t>(), h_div, pk->count[MSM_H], sw,
                     scal(MSM_H) + (size_t)sw * nic, ss);
  }
  // the scalars of a whole slot (MSM_H: [IC | H])
  void gather_slot(int slot, hipStream_t ss) {
    if (slot == MSM_H) gather_ich(ss);
    else gather(slot, 0, pk->count[slot], true, ss);
  }
  // points (and scalars) of a slot (MSM_H: the [IC | H] vector)
  uint32_t slot_len(int slot) const { return slot == MSM_H ? pk->ich_tot() : pk->count[slot] + pk->extras[slot]; }
  // One MSM over a slot's window copies (all of them, or the grouped-window
  // plan over those the key kept), downloaded
  template <class C>
  void launch_grouped(int slot, hipStream_t gs) {
    MsmWork& w = ctx->msm[slot];
    w.tag = serial ? SLOT_TAG[slot] : "";
    msm_launch_grouped<C>(w, pk->bases[slot].as<typename C::A>(), scal(slot), sw, slot_len(slot), bits, pk->win_c,
                          pk->copies, gs, pk->stride[slot]);
    msm_download<C>(w, gs);
  }
  // n points from compacted position lo of a slot's window-shifted bases, one-word scalars (a batch's segment)
  MsmSeg seg(int slot, uint32_t lo, uint32_t n) const {
    MsmSeg sg{pk->bases[slot].p, scal(slot) + lo, n, pk->stride[slot]};
    sg.wstride = slot_len(slot);
    sg.ioff = lo;
    return sg;
  }

  // ---- the MSMs that need only z
  // Part `part` of one group (G2: pi_B; G1: A + B1): compacted positions
  // [pcut[part], pcut[part+1]) of every slot, the extras with the last part.
  // Part 0 completes its buckets (FIXUP), every later part adds the previous
  // part's (ACCUM), and the last one reduces (COMBINE) into msm[slots[0]].
  template <class C>
  void launch_part(int part, const int* slots, int k, MsmWork* parts, const char* range_name, const char* tag,
                   const char* tag_part, hipStream_t gs) {
    Range range(range_name);
    const bool last = part == HOST_PARTS - 1;
    const int mode = part == 0 ? MSM_BACK_FIXUP : last ? MSM_BACK_COMBINE : MSM_BACK_ACCUM;
    MsmSeg segs[MSM_MAXSEG];
    for (int i = 0; i < k; i++) {
      const int sl = slots[i];
      const uint32_t lo = pk->pcut[part][sl], hi = pk->pcut[part + 1][sl];
      gather(sl, lo, hi, last, gs);
      segs[i] = seg(sl, lo, (last ? hi + pk->extras[sl] : hi) - lo);
    }
    MsmWork& w = last ? ctx->msm[slots[0]] : parts[part];
    w.tag = serial ? (last ? tag : tag_part) : "";
    msm_batch_front<C>(w, segs, k, 64, pk->win_c, gs);
    msm_batch_back<C>(w, gs, mode, part ? &parts[part - 1] : nullptr);
    if (last) {
      msm_download<C>(w, gs);
      ZK_HIP(hipEventRecord(ctx->ev_done[slots[0]], gs));
    }
  }
  // a host witness: part k's MSMs, then part k+1 of z (the host thread waits
  // for the pageable copy while the GPU runs the parts already there)
  void launch_split() {
    for (int k = 0; k < HOST_PARTS; k++) {
      if (k) {
        upload_part(k);
        ZK_HIP(hipEventRecord(ctx->ev_scal, st));
      }
      if (!serial) {
        ZK_HIP(hipStreamWaitEvent(s_g2, ctx->ev_scal, 0));
        ZK_HIP(hipStreamWaitEvent(s_abi, ctx->ev_scal, 0));
        if (k == HOST_PARTS - 1) gather_ic_early();   // all of z is here: IC's scalars off the critical path too
      }
      launch_part<G2>(k, G2_B, 1, ctx->part_g2, "msm_g2_part", "B2/", "B2p/", s_g2);
      launch_part<G1>(k, G1_AB, 2, ctx->part_abi, "msm_g1_a_b1_part", "AB/", "ABp/", s_abi);
    }
  }
  // A G1 group over whole slots (A + B1, or IC+H alone), its gathers included;
  // ev_done[slots[0]] stands for the group.  One-word scalars run the group
  // as ONE batch (msm_launch_batch: one sort, merge and bucket reduction);
  // whole scalars run one grouped-window MSM per slot, in order:
  // msm_front_impl batches one-word scalars only, and A and B1 as one batch at
  // sw = 4 measured slower in the overlapped prove (DESIGN.md 2.8,
  // profiles/sound_ab_batch_rejected.txt).  finish_g1 reads the result back
  // by the same rule; nothing else in a proof depends on it.
  bool g1_batched() const { return sw == 1; }
  void launch_g1(const int* slots, int k, const char* range_name, const char* tag, hipStream_t gs) {
    Range range(range_name);
    if (g1_batched()) {
      MsmSeg segs[MSM_MAXSEG];
      for (int i = 0; i < k; i++) {
        gather_slot(slots[i], gs);
        segs[i] = seg(slots[i], 0, slot_len(slots[i]));
      }
      MsmWork& w = ctx->msm[slots[0]];
      w.tag = serial ? tag : "";
      msm_launch_batch<G1>(w, segs, k, 64, pk->win_c, gs);
      msm_download<G1>(w, gs);
    } else {
      for (int i = 0; i < k; i++) {
        gather_slot(slots[i], gs);
        launch_grouped<G1>(slots[i], gs);
      }
    }
    ZK_HIP(hipEventRecord(ctx->ev_done[slots[0]], gs));
  }
  // the sum of slot slots[i] of a finished group
  host::X<host::Fq> finish_g1(const int* slots, int i) const {
    return g1_batched() ? msm_finish_seg<G1>(ctx->msm[slots[0]], i) : msm_finish<G1>(ctx->msm[slots[i]]);
  }
  // a device witness: G2 (pi_B), then A + B1 + IC, both starting with it
  void launch_whole() {
    if (!serial) ZK_HIP(hipStreamWaitEvent(s_g2, ctx->ev_scal, 0));
    {
      Range range("msm_g2");
      gather_slot(MSM_B2, s_g2);
      launch_grouped<G2>(MSM_B2, s_g2);
      ZK_HIP(hipEventRecord(ctx->ev_done[MSM_B2], s_g2));
    }
    if (!serial) {
      ZK_HIP(hipStreamWaitEvent(s_abi, ctx->ev_scal, 0));
      gather_ic_early();
    }
    launch_g1(G1_AB, 2, "msm_g1_a_b1", "AB/", s_abi);
  }

  // ---- the quotient, then IC + H on the main stream
  void run_quotient() {
    if (in.h_given) return;
    Range range(dist ? "quotient_distributed" : "quotient");
    if (dist) {
      ctx->tmp_scal.ensure(sizeof(uint64_t) * (pk->n / pk->nshards));
      dist_quotient(ctx, pk, in.d_z, *ctx->exch, ctx->dq, flags(), ctx->tmp_scal.as<uint64_t>(), st);
    } else {
      // (Az, Bz, Cz) -> H's scalars: in place in the IC+H scalars, else in
      // tmp_scal (sized here, before its pointer is taken)
      ctx->tmp_scal.ensure(sizeof(uint64_t) * sw * pk->n);
      quotient(ctx, pk, in.d_z, sw, st, h_direct ? scal(MSM_H) + (size_t)sw * nic : ctx->tmp_scal.as<uint64_t>());
    }
    h_src = ctx->tmp_scal.as<uint64_t>();
  }
  // everything onto the streams
  void launch() {
    // the IC+H scalar vector, sized once before any stream writes it (IC's
    // gather on the A+B1 stream, H's lo64 from the quotient when h_direct)
    ctx->scal[MSM_H].ensure(sizeof(uint64_t) * sw *
                            std::max<uint64_t>({(uint64_t)pk->ich_tot(), (uint64_t)nic + pk->n, 1}));
    // MSMs first, then the quotient (enqueueing the quotient first measured
    // 0.37 ms slower: profiles/r03_ab_quotient_first_rejected.txt).  With
    // ZK_OPT_EXCHANGE_FIRST a distributed quotient goes first and the side
    // streams wait for it, so its all-to-alls find free CUs on every rank.
    // (Split uploads are single-GPU only: the quotient needs all of z.)
    const bool xfirst = dist && ctx->exchange_first == 1 && !serial && !split;
    if (xfirst) {
      run_quotient();
      ZK_HIP(hipEventRecord(ctx->ev_quot, st));
      ZK_HIP(hipStreamWaitEvent(s_g2, ctx->ev_quot, 0));
      ZK_HIP(hipStreamWaitEvent(s_abi, ctx->ev_quot, 0));
    }
    if (split) launch_split();
    else launch_whole();
    if (!xfirst) run_quotient();
    // the exchange watchdog of finish() counts from here: a host-staged
    // exchange has finished its all-to-alls inside run_quotient, and only
    // local GPU work (RCCL: the enqueued collectives) is left
    t_quot = clk::now();
    // A distributed proof's witness checks are spread over the ranks (each
    // checks its slice and its quotient rows): every rank takes the max of the
    // flag words, so all return the status combine() would give -- flags are
    // ORs of 8 (z_i >= r), 4 / 3 (InvalidWitness) and 2 (division), and the
    // max keeps that precedence.  RCCL: on the stream, no host round trip.
    flags_agreed = dist && ctx->exch->agree_max_dev(flags(), st);
    ZK_HIP(hipMemcpyAsync(ctx->flags_host.p, ctx->flags.p, 4, hipMemcpyDeviceToHost, st));
    if (ic_ready) ZK_HIP(hipStreamWaitEvent(st, ctx->ev_ic, 0));
    launch_g1(G1_ICH, 1, "msm_g1_ic_h", "ICH/", st);
    if (ph_span >= 0) {
      for (int sl : WAITS) ZK_HIP(hipStreamWaitEvent(st, ctx->ev_done[sl], 0));
      ctx->prof.end(st, ph_span);
    }
    ctx->prof.add_host("host_launch", ms_since(t_start));
  }

  // ---- host tails (Horner over each MSM's partials, then s A + r B1) run as
  // each MSM's stream reaches its event, overlapping the MSMs still on the
  // GPU.  t_fin: the host time they took.
  Partial collect_msms(double& t_fin) {
    Partial p{};
    bool done[3] = {false, false, false};
    bool sc_done = false, ab_done = false;
    for (int left = 3; left > 0;) {
      // the H MSM waits for the peers' quotient stages: a dead peer must end
      // this proof (ZK_ERR_RCCL, the exchange aborted) instead of hanging it
      if (dist && (ctx->exch->async_error() || ms_since(t_quot) > ctx->exch->timeout_ms))
        throw Error(ZK_ERR_RCCL, "distributed quotient: a peer did not answer within the exchange timeout");
      bool progressed = false;
      for (int wi = 0; wi < 3; wi++) {
        if (done[wi]) continue;
        const int slot = WAITS[wi];
        const hipError_t q = hipEventQuery(ctx->ev_done[slot]);
        if (q == hipErrorNotReady) continue;
        ZK_HIP(q);
        const auto t_f = clk::now();
        if (slot == MSM_B2) {
          p.B2 = msm_finish<G2>(ctx->msm[slot]);
          if (in.early) host_to_abi<G2>(p.B2, reinterpret_cast<uint64_t*>(&in.early->b));
        } else if (slot == MSM_A) {
          p.A = finish_g1(G1_AB, 0);
          p.B1 = finish_g1(G1_AB, 1);
          ab_done = true;
        } else {
          p.IC = finish_g1(G1_ICH, 0);   // IC + H_1
          p.H = host::inf<host::Fq>();
        }
        done[wi] = progressed = true;
        left--;
        if (!sc_done && ab_done) {
          p.SC = host::mul2_scalar(p.A, s->l, p.B1, r->l);
          if (in.early) host_to_abi<G1>(p.A, reinterpret_cast<uint64_t*>(&in.early->a));
          sc_done = true;
        }
        t_fin += ms_since(t_f);
        if (left == 0) ctx->prof.add_host("host_tail_after_last", ms_since(t_f));
      }
      if (!progressed) std::this_thread::yield();
    }
    return p;
  }
  Partial finish() {
    Range range_tail("host_tail");
    double t_fin = 0;
    Partial p = collect_msms(t_fin);
    for (int k = 0; k < NUM_SIDE; k++) ZK_HIP(hipStreamSynchronize(ctx->side[k]));
    ZK_HIP(hipStreamSynchronize(st));
    ctx->prof.add_host("host_finish", t_fin);
    // host wall time of the whole call up to here, against prove_gpu_span
    ctx->prof.add_host("host_prove_total", ms_since(t_start));
    ctx->prof.collect();
    uint32_t flags = in.h_given ? in.given_flags : *ctx->flags_host.as<uint32_t>();
    if (dist && !flags_agreed) flags = (uint32_t)ctx->exch->agree_max((int)flags, st);
    p.status = status_from_flags(flags);
    return p;
  }
};

static Partial prove_partial(zk_ctx* ctx, const zk_pk_dev* pk, const zk_fr* r, const zk_fr* s, const ProveInput& in) {
  ProveRun run(ctx, pk, r, s, in);
  run.check_witness();
  run.launch();
  return run.finish();
}

static int combine(const Partial* parts, size_t k, zk_proof* out) {
  // the witness checks are spread over the ranks' rows: a non-canonical
  // input (ZK_ERR_ARG) first, then InvalidWitness (core:83-98, 124-128)
  // wins over the division failure (qap:266)
  for (size_t i = 0; i < k; i++)
    if (parts[i].status == ZK_ERR_ARG) return ZK_ERR_ARG;
  for (size_t i = 0; i < k; i++)
    if (parts[i].status == ZK_ERR_INVALID_WITNESS) return ZK_ERR_INVALID_WITNESS;
  for (size_t i = 0; i < k; i++)
    if (parts[i].status != ZK_OK) return parts[i].status;
  auto A = host::inf<host::Fq>(), C = A;
  auto B2 = host::inf<host::Fq2>();
  for (size_t i = 0; i < k; i++) {
    A = host::addp(A, parts[i].A);
    B2 = host::addp(B2, parts[i].B2);
    // pi_C = IC + H_1 + s pi_A + r B_1 (core:224-265; identity terms add nothing)
    C = host::addp(C, host::addp(host::addp(parts[i].IC, parts[i].H), parts[i].SC));
  }
  host_to_abi<G1>(A, reinterpret_cast<uint64_t*>(&out->a));
  host_to_abi<G2>(B2, reinterpret_cast<uint64_t*>(&out->b));
  host_to_abi<G1>(C, reinterpret_cast<uint64_t*>(&out->c));
  return ZK_OK;
}

int prove_impl(zk_ctx* ctx, const zk_pk_dev* pk, const void* d_z, size_t zlen, size_t num_public,
               const zk_fr* r, const zk_fr* s, zk_proof* out, const zk_fr* z_host) {
  // Witness::new (core:81-99) and the length check of validate (core:113-118)
  if (!fr_canonical(*r) || !fr_canonical(*s)) return ZK_ERR_ARG;   // Fr::rand draws are reduced
  if (num_public >= zlen) return ZK_ERR_INVALID_WITNESS;
  if (zlen != pk->V) return ZK_ERR_INVALID_WITNESS;
  if (pk->nshards != 1) return ZK_ERR_ARG;
  zk_proof ab{};
  ProveInput in{reinterpret_cast<const uint64_t*>(d_z)};
  in.early = &ab;
  in.z_host = z_host;
  // How a host witness reaches the device is decided here, once.  A reference
  // key takes the split path (ProveRun::launch_split: z goes up in parts under
  // the MSMs of the parts already there, which are batches of one-word
  // scalars).  A sound key's goes up whole first and then takes the device
  // path, like a device witness.
  if (pk->sound() && z_host) {
    ZK_HIP(hipMemcpyAsync(const_cast<void*>(d_z), z_host, sizeof(zk_fr) * zlen, hipMemcpyHostToDevice, ctx->stream));
    in.z_host = nullptr;
  }
  Partial p = prove_partial(ctx, pk, r, s, in);
  if (p.status != ZK_OK) return p.status;
  // combine() for one part: pi_A, pi_B already converted; pi_C = IC + H + s A + r B1
  out->a = ab.a;
  out->b = ab.b;
  host_to_abi<G1>(host::addp(host::addp(p.IC, p.H), p.SC), reinterpret_cast<uint64_t*>(&out->c));
  return ZK_OK;
}

// a host witness slice to its places in the ctx's device copy of z
static const uint64_t* upload_slice(zk_ctx* ctx, const zk_pk_dev* pk, const zk_fr* z_host,
                                    const std::vector<uint64_t>& ranges) {
  ctx->z_canon.ensure(sizeof(zk_fr) * std::max<size_t>(pk->V, 1));
  size_t off = 0;
  for (size_t k = 0; k + 1 < ranges.size(); k += 2) {
    const uint64_t lo = ranges[k], len = ranges[k + 1] - lo;
    ZK_HIP(hipMemcpyAsync(static_cast<zk_fr*>(ctx->z_canon.p) + lo, z_host + off, sizeof(zk_fr) * len,
                          hipMemcpyHostToDevice, ctx->stream));
    off += len;
  }
  return ctx->z_canon.as<uint64_t>();
}

// z_host / ranges: a host witness slice (zk_groth16_prove_partial_host) to
// upload first, after the ranks agreed, instead of the device witness d_z.
// bad_slice: the host slice does not match the ranges (ZK_ERR_ARG) -- with a
// distributed quotient it goes into the status agreement like every other
// input error, so the peers return with this rank instead of waiting in the
// first all-to-all.
static int prove_partial_common(zk_ctx* ctx, const zk_pk_dev* pk, const void* d_z, const zk_fr* z_host,
                                const std::vector<uint64_t>* ranges, size_t zlen, size_t num_public,
                                const zk_fr* r, const zk_fr* s, zk_prove_partial* out, bool bad_slice = false) {
  std::memset(out, 0, sizeof *out);
  if (pk->sound()) {
    ctx->err = "a sound proving key is never sharded: use zk_groth16_prove / zk_groth16_prove_dev";
    return ZK_ERR_ARG;
  }
  Partial p{};
  int local = ZK_OK;
  if (bad_slice || !fr_canonical(*r) || !fr_canonical(*s)) local = ZK_ERR_ARG;
  else if (num_public >= zlen || zlen != pk->V) local = ZK_ERR_INVALID_WITNESS;
  const bool attached = exchange_matches(ctx, pk);
  const bool dist = uses_dist_quotient(ctx, pk);
  if (attached && ctx->exch->broken) {
    ctx->err = "the exchange was aborted by an earlier failed proof; attach a new one (or detach it)";
    return ZK_ERR_RCCL;
  }
  hipStream_t st = ctx->stream;
  auto prove = [&]() {
    ProveInput in{z_host ? upload_slice(ctx, pk, z_host, *ranges) : reinterpret_cast<const uint64_t*>(d_z)};
    in.ranges = ranges;
    return prove_partial(ctx, pk, r, s, in);
  };
  if (!attached) {
    if (local == ZK_OK) p = prove();
    else p.status = local;
    std::memcpy(out->bytes, &p, sizeof p);
    return p.status;
  }
  // An exchange of the key's shape is attached.  Every allocation a
  // distributed quotient needs is made first, then the ranks agree on the
  // host-side checks and on the quotient mode before the first all-to-all (a
  // rank that bailed out alone, or one set to ZK_OPT_DIST_QUOTIENT 0 while
  // its peers are not, would leave them blocked in the collective): one
  // all-reduce of {any rank distributed, 2 status + any rank replicated}.
  // A failure after the agreement -- a transport error, a device error, a
  // peer that stopped answering -- aborts the exchange, so the peers'
  // pending transfers fail too, and marks it dead.  A replicated proof after
  // the agreement uses no exchange: its failures leave the exchange alone.
  bool in_exchange = true;
  try {
    if (local == ZK_OK && dist) {
      try {
        dq_prepare(ctx, pk, (int)pk->nshards, ctx->dq, st);
        ctx->tmp_scal.ensure(sizeof(uint64_t) * (pk->n / pk->nshards));
        if (z_host) ctx->z_canon.ensure(sizeof(zk_fr) * std::max<size_t>(pk->V, 1));
      } catch (const Error& e) {
        local = e.code;
        ctx->err = e.what();
      }
    }
    int32_t v[2] = {dist ? 1 : 0, local * 2 + (dist ? 0 : 1)};
    ctx->exch->agree_max2(v, st);
    if (local == ZK_OK) local = v[1] >> 1;
    if (local == ZK_OK && v[0] == 1 && (v[1] & 1)) {
      local = ZK_ERR_ARG;
      ctx->err = "ranks disagree on ZK_OPT_DIST_QUOTIENT: set it identically on every rank";
    }
    if (local != ZK_OK) {
      p.status = local;
    } else {
      in_exchange = dist;
      p = prove();
    }
  } catch (...) {
    if (in_exchange) {
      ctx->exch->broken = true;
      ctx->exch->abort();
    }
    throw;
  }
  std::memcpy(out->bytes, &p, sizeof p);
  return p.status;
}

int prove_partial_impl(zk_ctx* ctx, const zk_pk_dev* pk, const void* d_z, size_t zlen, size_t num_public,
                       const zk_fr* r, const zk_fr* s, zk_prove_partial* out) {
  return prove_partial_common(ctx, pk, d_z, nullptr, nullptr, zlen, num_public, r, s, out);
}

// The ranges a shard reads on this ctx: wr_dist with a distributed quotient,
// else the whole witness.
std::vector<uint64_t> witness_ranges(const zk_ctx* ctx, const zk_pk_dev* pk) {
  if (uses_dist_quotient(ctx, pk)) return pk->wr_dist;
  return {0, pk->V};
}

int prove_partial_host_impl(zk_ctx* ctx, const zk_pk_dev* pk, const zk_fr* z_slice, size_t slice_len, size_t zlen,
                            size_t num_public, const zk_fr* r, const zk_fr* s, zk_prove_partial* out) {
  const std::vector<uint64_t> ranges = witness_ranges(ctx, pk);
  size_t want = 0;
  for (size_t k = 0; k + 1 < ranges.size(); k += 2) want += ranges[k + 1] - ranges[k];
  const bool bad = slice_len != want || (want && !z_slice);
  if (bad)
    ctx->err = "witness slice length " + std::to_string(slice_len) + " != " + std::to_string(want) +
               " (zk_groth16_witness_ranges)";
  return prove_partial_common(ctx, pk, nullptr, z_slice, &ranges, zlen, num_public, r, s, out, bad);
}

// N virtual ranks of a sharded key on ONE device: the distributed quotient's
// stages run rank by rank, its three all-to-alls become device copies, then
// each rank's MSMs and the fold.  Exercises exactly the per-rank code and
// index maps the RCCL path runs (tests; the RCCL path needs N devices).
int prove_virtual_shards_impl(zk_ctx* ctx, const zk_pk_dev* const* pks, uint32_t N, const void* d_z, size_t zlen,
                              size_t num_public, const zk_fr* r, const zk_fr* s, zk_proof* out) {
  if (N < 2) return ZK_ERR_ARG;
  for (uint32_t k = 0; k < N; k++)
    if (!pks[k] || pks[k]->shard != k || pks[k]->nshards != N || pks[k]->n != pks[0]->n) return ZK_ERR_ARG;
  const zk_pk_dev* pk0 = pks[0];
  if (!fr_canonical(*r) || !fr_canonical(*s)) return ZK_ERR_ARG;
  if (num_public >= zlen || zlen != pk0->V) return ZK_ERR_INVALID_WITNESS;
  if (!dist_quotient_ok(pk0->n, (int)N)) return ZK_ERR_ARG;
  hipStream_t st = ctx->stream;
  const uint64_t* z = reinterpret_cast<const uint64_t*>(d_z);
  const uint64_t m = pk0->n / N;
  std::vector<DistQ> dq(N);
  std::vector<DevBuf> hb(N);
  DevBuf flags;
  flags.ensure(sizeof(uint32_t) * N);
  ZK_HIP(hipMemsetAsync(flags.p, 0, sizeof(uint32_t) * N, st));
  check_canonical(d_z, zlen, flags.as<uint32_t>(), st);
  auto exchange = [&](int which) {
    const size_t chunk = dq_chunk_bytes(pk0, (int)N, which);
    for (uint32_t a = 0; a < N; a++)
      for (uint32_t b = 0; b < N; b++) {
        const DevBuf& src = which == 1 ? dq[b].s1 : which == 2 ? dq[b].s2 : dq[b].s3;
        DevBuf& dst = which == 1 ? dq[a].r1 : which == 2 ? dq[a].r2 : dq[a].r3;
        ZK_HIP(hipMemcpyAsync(static_cast<char*>(dst.p) + b * chunk, static_cast<const char*>(src.p) + a * chunk,
                              chunk, hipMemcpyDeviceToDevice, st));
      }
  };
  for (uint32_t k = 0; k < N; k++) dq_stage_a(ctx, pks[k], z, (int)k, (int)N, dq[k], flags.as<uint32_t>() + k, st);
  exchange(1);
  for (uint32_t k = 0; k < N; k++) dq_stage_b(ctx, pks[k], (int)k, (int)N, dq[k], st);
  exchange(2);
  for (uint32_t k = 0; k < N; k++) dq_stage_c(ctx, pks[k], (int)k, (int)N, dq[k], st);
  exchange(3);
  for (uint32_t k = 0; k < N; k++) {
    hb[k].ensure(sizeof(uint64_t) * m);
    dq_stage_d(ctx, pks[k], (int)k, (int)N, dq[k], hb[k].as<uint64_t>(), st);
  }
  std::vector<uint32_t> hf(N);
  ZK_HIP(hipMemcpyAsync(hf.data(), flags.p, sizeof(uint32_t) * N, hipMemcpyDeviceToHost, st));
  ZK_HIP(hipStreamSynchronize(st));
  uint32_t all = 0;
  for (uint32_t f : hf) all |= f;
  if (status_from_flags(all) == ZK_ERR_ARG) return ZK_ERR_ARG;
  std::vector<Partial> parts(N);
  for (uint32_t k = 0; k < N; k++)
    parts[k] = prove_partial(ctx, pks[k], r, s, ProveInput{z, hb[k].as<uint64_t>(), all});
  return combine(parts.data(), N, out);
}

int combine_impl(const zk_prove_partial* parts, size_t k, const zk_fr* r, const zk_fr* s, zk_proof* out) {
  std::vector<Partial> ps(k);
  for (size_t i = 0; i < k; i++) std::memcpy(&ps[i], parts[i].bytes, sizeof(Partial));
  (void)r;
  (void)s;
  return combine(ps.data(), k, out);
}

}  // namespace zk
