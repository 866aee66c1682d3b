// setup.hip -- CRS::generate_from_qap (crates/groth16-setup/src/lib.rs:141-268)
// on the GPU, with the reference's exact scalar semantics:
//   a~,b~,g~,d~,t~ = lo64(alpha..tau)                         setup:155-159
//   alpha_1 .. delta_2 = generator * FULL param               setup:166-171
//   A_i(t~), B_i(t~), C_i(t~)                                 setup:174-182
//   a_g1[i] = G1 lo64(A_i), b_g1/b_g2[i] = G lo64(B_i)        setup:185-207
//   pk ic[i-l-1] = G1 lo64((b~A_i + a~B_i + C_i)/d~), i > l    setup:210-218
//   vk ic[i]     = G1 lo64((b~A_i + a~B_i + C_i)/g~), i <= l   setup:221-229
//   h[i] = G1 lo64(t~^i / d~), i < qap.degree() = n           setup:232-241
// A_i(t) is evaluated from the sparse matrices as sum_j M[j][i] L_j(t) with
// the Lagrange basis of the size-n domain -- the same value as evaluating the
// interpolated polynomial of qap:143-170, without materialising it.
// The per-point work (64-bit fixed-base multiplications on 8-bit window
// tables, batch affine normalisation) is data-parallel on the GPU; the six
// full-width generator multiples are a few hundred sequential group ops and
// run on the host (host_ec.hpp).
#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "key.hpp"
#include "prove.hpp"
#include "quotient.hpp"
#include "setup.hpp"

namespace zk {

// ---------------------------------------------------- fixed-base tables ---
// T[w][d] = d * 2^(8w) * G, w < W, d < 256 (affine, Montgomery); T[w][0] unused.
// W = 8 byte windows for the reference's 64-bit scalars, 32 for the whole
// scalars of a sound setup (8 160 entries: 0.8 MB for G1, 1.6 MB for G2).
constexpr int FB_WIN64 = 8, FB_WIN255 = 32;
template <class C>
struct FbTable {
  std::vector<typename C::A> host;
  DevBuf dev;
};

static host::X<host::Fq> g1_gen_host() {
  host::X<host::Fq> p{{}, {}, host::one(), host::one()};
  std::memcpy(p.X_.l, G1_GEN_HOSTM, 48);
  std::memcpy(p.Y.l, G1_GEN_HOSTM + 12, 48);
  return p;
}
static host::X<host::Fq2> g2_gen_host() {
  host::X<host::Fq2> p{{}, {}, host::f_one<host::Fq2>(), host::f_one<host::Fq2>()};
  std::memcpy(p.X_.c0.l, G2_GEN_HOSTM, 48);
  std::memcpy(p.X_.c1.l, G2_GEN_HOSTM + 12, 48);
  std::memcpy(p.Y.c0.l, G2_GEN_HOSTM + 24, 48);
  std::memcpy(p.Y.c1.l, G2_GEN_HOSTM + 36, 48);
  return p;
}

template <class HF, class DA>
static void build_table(const host::X<HF>& G, int W, std::vector<DA>& out) {
  using HX = host::X<HF>;
  std::vector<HX> pts(W * 256);
  HX base = G;
  for (int w = 0; w < W; w++) {
    pts[w * 256] = host::inf<HF>();
    for (int d = 1; d < 256; d++) pts[w * 256 + d] = host::addp(pts[w * 256 + d - 1], base);
    for (int k = 0; k < 8; k++) base = host::dbl(base);
  }
  out.resize(W * 256);
  for (int i = 0; i < W * 256; i++) {
    HF x, y;
    if (!host::to_affine(pts[i], x, y)) { x = host::f_zero<HF>(); y = host::f_zero<HF>(); }
    x = host::to_dev(x);   // device Montgomery radix (constants.hpp)
    y = host::to_dev(y);
    static_assert(sizeof(HF) * 2 == sizeof(DA), "layout");
    std::memcpy(&out[i], &x, sizeof(HF));
    std::memcpy(reinterpret_cast<char*>(&out[i]) + sizeof(HF), &y, sizeof(HF));
  }
}

// ------------------------------------------------------------- kernels ---
// Lagrange basis at t over the size-n domain, per-thread batch inversion:
// L_j = w^j (t^n - 1) / (n (t - w^j)); k = (t^n - 1)/n precomputed.
constexpr int LAG_CHUNK = 32;
__global__ void __launch_bounds__(256) k_lagrange(const Fr* __restrict__ wpow, Fr t, Fr k, size_t n,
                                                  Fr* __restrict__ L) {
  const size_t c0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * LAG_CHUNK;
  if (c0 >= n) return;
  const size_t c1 = min(c0 + LAG_CHUNK, n);
  Fr run = fp_one<FrParams>();
  for (size_t j = c0; j < c1; j++) {               // L[j] <- prefix product
    st_vec(&L[j], run);
    run = fp_mul(run, fp_sub(t, ld_vec(&wpow[j])));
  }
  // Fermat inverse of the chunk product
  uint32_t e[8];
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) e[i] = __builtin_subc(FrParams::MOD[i], i == 0 ? 2u : 0u, br, &br);
  Fr inv = fp_one<FrParams>();
#pragma unroll
  for (int i = 7; i >= 0; i--)
    for (int b = 31; b >= 0; b--) {
      inv = fp_mul(inv, inv);
      if ((e[i] >> b) & 1) inv = fp_mul(inv, run);
    }
  for (size_t j = c1; j-- > c0;) {
    const Fr wj = ld_vec(&wpow[j]);
    const Fr d = fp_sub(t, wj);
    const Fr dinv = fp_mul(inv, ld_vec(&L[j]));
    inv = fp_mul(inv, d);
    st_vec(&L[j], fp_mul(fp_mul(dinv, wj), k));
  }
}
// t is a domain point (t^n = 1): L_j = [w^j == t]
__global__ void __launch_bounds__(256) k_lagrange_point(const Fr* __restrict__ wpow, Fr t, size_t n,
                                                        Fr* __restrict__ L) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  st_vec(&L[j], fp_eq(ld_vec(&wpow[j]), t) ? fp_one<FrParams>() : fp_zero<FrParams>());
}

// Column sums over CSC: out[i] = sum_k val_k L[row_k] (cols >= V dropped by construction)
__global__ void __launch_bounds__(256) k_colsum(const uint64_t* __restrict__ cp, const uint32_t* __restrict__ row,
                                                const Fr* __restrict__ val, const Fr* __restrict__ L, uint64_t V,
                                                Fr* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= V) return;
  Fr acc = fp_zero<FrParams>();
  for (uint64_t k = cp[i]; k < cp[i + 1]; k++) {
    Fr x = ld_vec(&L[row[k]]);
    if (val) x = fp_mul(x, ld_vec(&val[k]));
    acc = fp_add(acc, x);
  }
  st_vec(&out[i], acc);
}

struct SetupConsts {
  Fr al, be, dinv, ginv;  // Montgomery: a~, b~, d~^-1, g~^-1 (sound: the full-width alpha, beta, delta^-1, gamma^-1)
  uint64_t V, num_public;
};
// per variable i: the scalars for a_g1, b_g1 (= b_g2), pk ic (i > l) / vk ic
// (i <= l), SW words each (st_scal: 1 = lo64, the reference; 4 = whole, a
// sound setup, where nothing is truncated)
template <int SW>
__global__ void __launch_bounds__(256) k_setup_scalars(const Fr* __restrict__ av, const Fr* __restrict__ bv,
                                                       const Fr* __restrict__ cv, SetupConsts k,
                                                       uint64_t* __restrict__ sa, uint64_t* __restrict__ sb,
                                                       uint64_t* __restrict__ sic, uint64_t* __restrict__ svk) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= k.V) return;
  const Fr a = ld_vec(&av[i]), b = ld_vec(&bv[i]), c = ld_vec(&cv[i]);
  st_scal<SW>(sa, i, a);
  st_scal<SW>(sb, i, b);
  const Fr t = fp_add(fp_add(fp_mul(k.be, a), fp_mul(k.al, b)), c);
  if (i > k.num_public) st_scal<SW>(sic, i - k.num_public - 1, fp_mul(t, k.dinv));
  else st_scal<SW>(svk, i, fp_mul(t, k.ginv));
}
static void setup_scalars(const Fr* av, const Fr* bv, const Fr* cv, const SetupConsts& k, int sw, uint64_t* sa,
                          uint64_t* sb, uint64_t* sic, uint64_t* svk, hipStream_t st) {
  if (sw == 1) k_setup_scalars<1><<<ceil_div(k.V, 256), 256, 0, st>>>(av, bv, cv, k, sa, sb, sic, svk);
  else k_setup_scalars<4><<<ceil_div(k.V, 256), 256, 0, st>>>(av, bv, cv, k, sa, sb, sic, svk);
  ZK_LAUNCH_CHECK();
}

// XYZZ = sum_w T[w][byte_w(k)]  (<= 8 mixed additions), k = scal[idx ? idx[i] : i]
template <class C>
__global__ void __launch_bounds__(128) k_fixed_base(const typename C::A* __restrict__ T,
                                                    const uint64_t* __restrict__ scal,
                                                    const uint32_t* __restrict__ idx, size_t n,
                                                    typename C::X* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = scal[idx ? idx[i] : i];
  typename C::X acc;
  xyzz_set_inf(acc);
  for (int w = 0; w < 8; w++) {
    const uint32_t d = (uint32_t)(k >> (8 * w)) & 255u;
    if (d) acc = xyzz_madd(acc, ld_vec(&T[w * 256 + d]));
  }
  st_vec(&out[i], acc);
}
// The same for a whole canonical scalar k < r of 4 u64 limbs (sound setup):
// XYZZ = sum_w T[w][byte_w(k)] over 32 byte windows, <= 32 mixed additions.
// The partial sum before window w is (k mod 2^(8w)) G, below every entry
// d 2^(8w) G of that window and the total below r G: never the doubling or the
// cancelling case of the mixed addition.  The loop stays rolled and reads the
// scalar a byte at a time (its little-endian bytes are the windows): beside
// the accumulator only a pointer and a counter live across an addition, which
// the G2 variant at 256 VGPRs needs.
template <class C>
__global__ void __launch_bounds__(128) k_fixed_base_wide(const typename C::A* __restrict__ T,
                                                         const uint64_t* __restrict__ scal,
                                                         const uint32_t* __restrict__ idx, size_t n,
                                                         typename C::X* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t* k = reinterpret_cast<const uint8_t*>(scal + 4 * (size_t)(idx ? idx[i] : i));
  typename C::X acc;
  xyzz_set_inf(acc);
#pragma unroll 1
  for (int w = 0; w < FB_WIN255; w++) {
    const uint32_t d = k[w];
    if (d) acc = xyzz_madd(acc, ld_vec(&T[w * 256 + d]));
  }
  st_vec(&out[i], acc);
}

// device affine (Montgomery, (0,0) = infinity) -> canonical ABI words
__device__ __forceinline__ void st_canon(uint64_t* w, const Fq& m) {
  Fq c = fp_from_mont(m);
#pragma unroll
  for (int i = 0; i < 6; i++) w[i] = (uint64_t)c.v[2 * i] | ((uint64_t)c.v[2 * i + 1] << 32);
}
__global__ void __launch_bounds__(256) k_to_abi_g1(const G1A* __restrict__ in, size_t n, uint64_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const G1A a = ld_vec(&in[i]);
  uint64_t* w = out + i * 13;
  if (aff_is_inf(a)) {
    for (int k = 0; k < 12; k++) w[k] = 0;
    w[12] = 1;
    return;
  }
  st_canon(w, a.x);
  st_canon(w + 6, a.y);
  w[12] = 0;
}
__global__ void __launch_bounds__(256) k_to_abi_g2(const G2A* __restrict__ in, size_t n, uint64_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const G2A a = ld_vec(&in[i]);
  uint64_t* w = out + i * 25;
  if (aff_is_inf(a)) {
    for (int k = 0; k < 24; k++) w[k] = 0;
    w[24] = 1;
    return;
  }
  st_canon(w, a.x.c0);
  st_canon(w + 6, a.x.c1);
  st_canon(w + 12, a.y.c0);
  st_canon(w + 18, a.y.c1);
  w[24] = 0;
}

// ------------------------------------------------------------- helpers ---
static std::mutex g_tab_mu;
template <class C>
static FbTable<C>& fb_table(int device, int W, hipStream_t st) {
  static std::map<std::pair<int, int>, FbTable<C>> tabs;   // one per group, device and window count
  std::lock_guard<std::mutex> lk(g_tab_mu);
  FbTable<C>& t = tabs[{device, W}];
  if (t.host.empty()) {
    if constexpr (C::ABI_WORDS == 13) build_table(g1_gen_host(), W, t.host);
    else build_table(g2_gen_host(), W, t.host);
    t.dev.ensure(sizeof(typename C::A) * t.host.size());
    ZK_HIP(hipMemcpyAsync(t.dev.p, t.host.data(), sizeof(typename C::A) * t.host.size(), hipMemcpyHostToDevice, st));
    ZK_HIP(hipStreamSynchronize(st));
  }
  return t;
}

// out[i] = G * scal[idx ? idx[i] : i], affine Montgomery; a scalar is sw u64
// words: 1 (below 2^64) or 4 (a whole canonical Fr)
template <class C>
static void fixed_base(zk_ctx* ctx, const uint64_t* d_scal, const uint32_t* d_idx, size_t n,
                       typename C::A* d_out, hipStream_t st, int sw = 1) {
  if (!n) return;
  FbTable<C>& T = fb_table<C>(ctx->device, sw == 1 ? FB_WIN64 : FB_WIN255, st);
  DevBuf xs, pre;
  xs.ensure(sizeof(typename C::X) * n);
  pre.ensure(sizeof(typename C::F) * n);
  if (sw == 1)
    k_fixed_base<C><<<ceil_div(n, 128), 128, 0, st>>>(T.dev.template as<typename C::A>(), d_scal, d_idx, n,
                                                       xs.template as<typename C::X>());
  else
    k_fixed_base_wide<C><<<ceil_div(n, 128), 128, 0, st>>>(T.dev.template as<typename C::A>(), d_scal, d_idx, n,
                                                            xs.template as<typename C::X>());
  ZK_LAUNCH_CHECK();
  batch_normalize<C>(xs.template as<typename C::X>(), n, pre.template as<typename C::F>(), d_out, st);
  ZK_HIP(hipStreamSynchronize(st));  // xs / pre die here
}

template <class C>
static void to_abi(const typename C::A* d_in, size_t n, void* host_out, hipStream_t st) {
  if (!n) return;
  DevBuf w;
  w.ensure(sizeof(uint64_t) * C::ABI_WORDS * n);
  if (C::ABI_WORDS == 13)
    k_to_abi_g1<<<ceil_div(n, 256), 256, 0, st>>>(reinterpret_cast<const G1A*>(d_in), n, w.as<uint64_t>());
  else
    k_to_abi_g2<<<ceil_div(n, 256), 256, 0, st>>>(reinterpret_cast<const G2A*>(d_in), n, w.as<uint64_t>());
  ZK_LAUNCH_CHECK();
  ZK_HIP(hipMemcpyAsync(host_out, w.p, sizeof(uint64_t) * C::ABI_WORDS * n, hipMemcpyDeviceToHost, st));
  ZK_HIP(hipStreamSynchronize(st));
}

// n device affine points (Montgomery) `stride` bytes apart (0 = packed) ->
// canonical ABI words in host memory (the test library's key readback)
void bases_to_abi_host(bool g2, const void* d_in, uint32_t stride, size_t n, uint64_t* host_out, hipStream_t st) {
  if (!n) return;
  const size_t asz = g2 ? sizeof(G2A) : sizeof(G1A);
  DevBuf packed;
  const void* src = d_in;
  if (stride && stride != asz) {
    packed.ensure(asz * n);
    ZK_HIP(hipMemcpy2DAsync(packed.p, asz, d_in, stride, asz, n, hipMemcpyDeviceToDevice, st));
    src = packed.p;
  }
  if (g2) to_abi<G2>(static_cast<const G2A*>(src), n, host_out, st);
  else to_abi<G1>(static_cast<const G1A*>(src), n, host_out, st);
}

// out[i] = G * scalars[i] for n whole canonical scalars through the 255-bit
// fixed-base kernel, as canonical ABI words in host memory (the test library)
int fixed_base_wide_host(zk_ctx* ctx, bool g2, const zk_fr* scalars, size_t n, uint64_t* host_out) {
  for (size_t i = 0; i < n; i++)
    if (!fr_canonical(scalars[i])) return ZK_ERR_ARG;
  if (!n) return ZK_OK;
  hipStream_t st = ctx->stream;
  DevBuf sc, o;
  sc.ensure(sizeof(zk_fr) * n);
  o.ensure((g2 ? sizeof(G2A) : sizeof(G1A)) * n);
  ZK_HIP(hipMemcpyAsync(sc.p, scalars, sizeof(zk_fr) * n, hipMemcpyHostToDevice, st));
  if (g2) {
    fixed_base<G2>(ctx, sc.as<uint64_t>(), nullptr, n, o.as<G2A>(), st, 4);
    to_abi<G2>(o.as<G2A>(), n, host_out, st);
  } else {
    fixed_base<G1>(ctx, sc.as<uint64_t>(), nullptr, n, o.as<G1A>(), st, 4);
    to_abi<G1>(o.as<G1A>(), n, host_out, st);
  }
  return ZK_OK;
}

// host-side generator multiple by a full-width canonical scalar -> ABI
template <class C, class HX>
static void gen_mul_abi(const HX& G, const zk_fr& k, void* out) {
  host_to_abi<C>(host::mul_scalar(G, k.l), reinterpret_cast<uint64_t*>(out));
}

static bool fr_canon_zero(const zk_fr& a) { return (a.l[0] | a.l[1] | a.l[2] | a.l[3]) == 0; }

// CSR (rows) -> CSC (columns < V) for one matrix
void csr_to_csc(uint64_t nc, uint64_t V, const uint64_t* rp, const uint32_t* col, const zk_fr* val,
                       std::vector<uint64_t>& cp, std::vector<uint32_t>& row, std::vector<zk_fr>& cval) {
  cp.assign(V + 1, 0);
  const uint64_t nnz = nc ? rp[nc] : 0;
  for (uint64_t k = 0; k < nnz; k++)
    if (col[k] < V) cp[col[k] + 1]++;
  for (uint64_t i = 0; i < V; i++) cp[i + 1] += cp[i];
  row.resize(std::max<uint64_t>(cp[V], 1));
  if (val) cval.resize(std::max<uint64_t>(cp[V], 1));
  std::vector<uint64_t> cur(cp.begin(), cp.end() - 1);
  for (uint64_t j = 0; j < nc; j++)
    for (uint64_t k = rp[j]; k < rp[j + 1]; k++) {
      if (col[k] >= V) continue;
      const uint64_t p = cur[col[k]]++;
      row[p] = (uint32_t)j;
      if (val) cval[p] = val[k];
    }
}

static Fr fr_dev(const host::Fr& h) {
  Fr d;
  const host::Fr v = host::fr_to_dev(h);
  std::memcpy(d.v, v.l, 32);
  return d;
}
// Z(t) = t^n - 1 over the size-2^log_n domain
static host::Fr vanishing_at(const host::Fr& t, uint32_t log_n) {
  host::Fr tn = t;
  for (uint32_t i = 0; i < log_n; i++) tn = host::fr_mul(tn, tn);
  return host::fr_sub(tn, host::fr_one());
}
// wpow[j] = w^j and L[j] = L_j(t), j < n = 2^log_n
static void lagrange_at(const host::Fr& t, uint32_t log_n, DevBuf& wpow, DevBuf& L, hipStream_t st) {
  const uint64_t n = 1ull << log_n;
  const host::Fr zt = vanishing_at(t, log_n);
  wpow.ensure(sizeof(Fr) * n);
  L.ensure(sizeof(Fr) * n);
  Fr one_d, w_d;
  for (int i = 0; i < 8; i++) one_d.v[i] = FrParams::ONE[i];
  for (int i = 0; i < 8; i++) w_d.v[i] = FR_ROOTS[log_n][i];
  fr_powers(wpow.as<Fr>(), w_d, one_d, n, st);
  if (host::fr_is_zero(zt)) {
    k_lagrange_point<<<ceil_div(n, 256), 256, 0, st>>>(wpow.as<Fr>(), fr_dev(t), n, L.as<Fr>());
  } else {
    const host::Fr kk = host::fr_mul(zt, host::fr_inv(host::fr_from_u64(n)));
    k_lagrange<<<ceil_div(ceil_div(n, LAG_CHUNK), 256), 256, 0, st>>>(wpow.as<Fr>(), fr_dev(t), fr_dev(kk), n,
                                                                      L.as<Fr>());
  }
  ZK_LAUNCH_CHECK();
}

// ---------------------------------------------------------------- setup ---
int setup_impl(zk_ctx* ctx, const zk_r1cs_csr* q, const zk_setup_params* P, uint64_t num_public, uint32_t shard,
               uint32_t nshards, zk_pk* pk_host, zk_pk_dev** pk_dev, zk_vk* vk, bool sound) {
  Range range("zk_setup");
  hipStream_t st = ctx->stream;
  const uint64_t V = q->num_variables, nc = q->num_constraints;
  // SetupParams::validate (setup:128-136) and num_public < V (setup:148-152)
  if (fr_canon_zero(P->alpha) || fr_canon_zero(P->beta) || fr_canon_zero(P->gamma) || fr_canon_zero(P->delta))
    return ZK_ERR_SETUP_PARAMS;
  if (num_public >= V) return ZK_ERR_SETUP_PARAMS;
  // truncated copies (setup:155-159); the reference unwraps inverse(d~), inverse(g~)
  const uint64_t al = P->alpha.l[0], be = P->beta.l[0], ga = P->gamma.l[0], de = P->delta.l[0], ta = P->tau.l[0];
  if (!sound && (de == 0 || ga == 0)) return ZK_ERR_SETUP_PARAMS;
  if (nc > (1ull << 32)) return ZK_ERR_DOMAIN;
  uint64_t n = 1;
  while (n < nc) n <<= 1;
  const uint32_t log_n = (uint32_t)__builtin_ctzll(n);
  if (log_n > 32) return ZK_ERR_DOMAIN;
  if (V >= 0x80000000ull || n >= 0x80000000ull) return ZK_ERR_ARG;

  // Sound mode (no reference counterpart: the reference truncates) takes every
  // parameter whole, and h_g1[i] = [tau^i Z(tau) / delta]_1: hk = Z(tau) / delta
  // scales the tau powers.  tau on the domain gives Z(tau) = 0 and a key whose
  // H query is all identity: ZK_ERR_SETUP_PARAMS.
  const int sw = sound ? 4 : 1;   // u64 words per setup scalar
  host::Fr t, alf, bef, dinv, ginv, hk;
  if (sound) {
    if (!fr_canonical(P->alpha) || !fr_canonical(P->beta) || !fr_canonical(P->gamma) || !fr_canonical(P->delta) ||
        !fr_canonical(P->tau)) {
      ctx->err = "sound setup: a parameter is not a canonical Fr (>= r)";
      return ZK_ERR_ARG;
    }
    if (nshards != 1) return ZK_ERR_ARG;
    t = host::fr_to_mont(P->tau.l);
    alf = host::fr_to_mont(P->alpha.l);
    bef = host::fr_to_mont(P->beta.l);
    dinv = host::fr_inv(host::fr_to_mont(P->delta.l));
    ginv = host::fr_inv(host::fr_to_mont(P->gamma.l));
    const host::Fr zt = vanishing_at(t, log_n);
    if (host::fr_is_zero(zt)) {
      ctx->err = "sound setup: tau lies on the evaluation domain (Z(tau) = 0)";
      return ZK_ERR_SETUP_PARAMS;
    }
    hk = host::fr_mul(zt, dinv);
  } else {
    t = host::fr_from_u64(ta);
    alf = host::fr_from_u64(al);
    bef = host::fr_from_u64(be);
    dinv = host::fr_inv(host::fr_from_u64(de));
    ginv = host::fr_inv(host::fr_from_u64(ga));
    hk = dinv;
  }

  // ---- Lagrange basis at tau~ and A_i, B_i, C_i (device) ----
  DevBuf wpow, L, abc[3];
  lagrange_at(t, log_n, wpow, L, st);
  const uint64_t* rps[3] = {q->a_rowptr, q->b_rowptr, q->c_rowptr};
  const uint32_t* cols[3] = {q->a_col, q->b_col, q->c_col};
  const zk_fr* vals[3] = {q->a_val, q->b_val, q->c_val};
  for (int m = 0; m < 3; m++) {
    std::vector<uint64_t> cp;
    std::vector<uint32_t> row;
    std::vector<zk_fr> cval;
    csr_to_csc(nc, V, rps[m], cols[m], vals[m], cp, row, cval);
    DevBuf dcp, drow, draw, dval;
    dcp.ensure(sizeof(uint64_t) * (V + 1));
    drow.ensure(sizeof(uint32_t) * row.size());
    ZK_HIP(hipMemcpyAsync(dcp.p, cp.data(), sizeof(uint64_t) * (V + 1), hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(drow.p, row.data(), sizeof(uint32_t) * row.size(), hipMemcpyHostToDevice, st));
    if (vals[m]) {
      draw.ensure(sizeof(zk_fr) * cval.size());
      dval.ensure(sizeof(Fr) * cval.size());
      ZK_HIP(hipMemcpyAsync(draw.p, cval.data(), sizeof(zk_fr) * cval.size(), hipMemcpyHostToDevice, st));
      fr_to_mont(draw.as<uint64_t>(), dval.as<Fr>(), cval.size(), st);
    }
    abc[m].ensure(sizeof(Fr) * std::max<uint64_t>(V, 1));
    k_colsum<<<ceil_div(V, 256), 256, 0, st>>>(dcp.as<uint64_t>(), drow.as<uint32_t>(),
                                               vals[m] ? dval.as<Fr>() : nullptr, L.as<Fr>(), V, abc[m].as<Fr>());
    ZK_LAUNCH_CHECK();
    ZK_HIP(hipStreamSynchronize(st));  // host vectors / staging die here
  }

  // ---- lo64 scalars (sound: whole canonical scalars, 4 words each) ----
  const uint64_t nic = V - num_public - 1, nvk = num_public + 1;
  DevBuf sa, sb, sic, svk, sh, tp;
  sa.ensure(8 * sw * V);
  sb.ensure(8 * sw * V);
  sic.ensure(8 * sw * std::max<uint64_t>(nic, 1));
  svk.ensure(8 * sw * nvk);
  sh.ensure(8 * sw * n);
  tp.ensure(sizeof(Fr) * n);
  SetupConsts K;
  K.al = fr_dev(alf);
  K.be = fr_dev(bef);
  K.dinv = fr_dev(dinv);
  K.ginv = fr_dev(ginv);
  K.V = V;
  K.num_public = num_public;
  setup_scalars(abc[0].as<Fr>(), abc[1].as<Fr>(), abc[2].as<Fr>(), K, sw, sa.as<uint64_t>(), sb.as<uint64_t>(),
                sic.as<uint64_t>(), svk.as<uint64_t>(), st);
  fr_powers(tp.as<Fr>(), fr_dev(t), fr_dev(hk), n, st);   // t~^i / d~ (sound: tau^i Z(tau) / delta)
  fr_to_scalars(tp.as<Fr>(), n, sw, sh.as<uint64_t>(), st);

  // ---- full-width generator multiples (host; setup:166-171) ----
  const auto G1h = g1_gen_host();
  const auto G2h = g2_gen_host();
  zk_g1_affine alpha_g1, beta_g1, delta_g1;
  zk_g2_affine beta_g2, gamma_g2, delta_g2;
  gen_mul_abi<G1>(G1h, P->alpha, &alpha_g1);
  gen_mul_abi<G1>(G1h, P->beta, &beta_g1);
  gen_mul_abi<G1>(G1h, P->delta, &delta_g1);
  gen_mul_abi<G2>(G2h, P->beta, &beta_g2);
  gen_mul_abi<G2>(G2h, P->delta, &delta_g2);
  gen_mul_abi<G2>(G2h, P->gamma, &gamma_g2);

  if (vk) {
    vk->alpha_g1 = alpha_g1;
    vk->beta_g2 = beta_g2;
    vk->gamma_g2 = gamma_g2;
    vk->delta_g2 = delta_g2;
    vk->num_public = num_public;
    vk->ic_len = nvk;
    DevBuf o;
    o.ensure(sizeof(G1A) * nvk);
    fixed_base<G1>(ctx, svk.as<uint64_t>(), nullptr, nvk, o.as<G1A>(), st, sw);
    to_abi<G1>(o.as<G1A>(), nvk, vk->ic_g1, st);
  }

  if (pk_host) {
    // full vectors, canonical, into caller arrays
    pk_host->alpha_g1 = alpha_g1;
    pk_host->beta_g1 = beta_g1;
    pk_host->delta_g1 = delta_g1;
    pk_host->beta_g2 = beta_g2;
    pk_host->delta_g2 = delta_g2;
    pk_host->num_public = num_public;
    pk_host->a_len = V;
    pk_host->b_len = V;
    pk_host->b2_len = V;
    pk_host->ic_len = nic;
    pk_host->h_len = n;
    DevBuf o;
    o.ensure(sizeof(G2A) * std::max<uint64_t>(V, n));
    fixed_base<G1>(ctx, sa.as<uint64_t>(), nullptr, V, o.as<G1A>(), st, sw);
    to_abi<G1>(o.as<G1A>(), V, pk_host->a_g1, st);
    fixed_base<G1>(ctx, sb.as<uint64_t>(), nullptr, V, o.as<G1A>(), st, sw);
    to_abi<G1>(o.as<G1A>(), V, pk_host->b_g1, st);
    fixed_base<G2>(ctx, sb.as<uint64_t>(), nullptr, V, o.as<G2A>(), st, sw);
    to_abi<G2>(o.as<G2A>(), V, pk_host->b_g2, st);
    fixed_base<G1>(ctx, sic.as<uint64_t>(), nullptr, nic, o.as<G1A>(), st, sw);
    to_abi<G1>(o.as<G1A>(), nic, pk_host->ic_g1, st);
    fixed_base<G1>(ctx, sh.as<uint64_t>(), nullptr, n, o.as<G1A>(), st, sw);
    to_abi<G1>(o.as<G1A>(), n, pk_host->h_g1, st);
    return ZK_OK;
  }

  // ---- device-resident (optionally sharded) proving key ----
  std::unique_ptr<zk_pk_dev> d = pk_create(ctx, q, num_public, shard, nshards, sound);
  // host copies of the scalar vectors decide which bases are the identity
  // (scalar 0 <=> identity, since every scalar is < 2^64 < r; sound: a whole
  // canonical scalar < r, sw words of it)
  std::vector<uint64_t> ha(V * sw), hb(V * sw), hic(nic * sw), hh(n * sw);
  ZK_HIP(hipMemcpyAsync(ha.data(), sa.p, 8 * sw * V, hipMemcpyDeviceToHost, st));
  ZK_HIP(hipMemcpyAsync(hb.data(), sb.p, 8 * sw * V, hipMemcpyDeviceToHost, st));
  if (nic) ZK_HIP(hipMemcpyAsync(hic.data(), sic.p, 8 * sw * nic, hipMemcpyDeviceToHost, st));
  ZK_HIP(hipMemcpyAsync(hh.data(), sh.p, 8 * sw * n, hipMemcpyDeviceToHost, st));
  ZK_HIP(hipStreamSynchronize(st));
  const std::vector<uint8_t> own = var_owner(q, n, nshards);
  const KeyExtras ex = key_extras(shard, alpha_g1, beta_g1, delta_g1, beta_g2, delta_g2, sound);
  // one base vector: G * (the device scalars at this shard's positions)
  auto build_slot = [&](const SlotShape& shape, const std::vector<uint64_t>& hs, const DevBuf& ds) {
    std::vector<uint8_t> zero(hs.size() / sw);
    for (size_t i = 0; i < zero.size(); i++) {
      uint64_t any = 0;
      for (int k = 0; k < sw; k++) any |= hs[i * sw + k];
      zero[i] = any == 0;
    }
    const std::vector<uint32_t> pos = shard_positions(shape, shard, nshards, own, zero.data(), 1);
    pk_fill_slot(*d, shape, pos, ex, st, [&](const std::vector<uint32_t>& kept, void* d_out) {
      DevBuf dpos;
      dpos.ensure(sizeof(uint32_t) * kept.size());
      ZK_HIP(hipMemcpyAsync(dpos.p, kept.data(), sizeof(uint32_t) * kept.size(), hipMemcpyHostToDevice, st));
      if (shape.slot == MSM_B2)
        fixed_base<G2>(ctx, ds.as<uint64_t>(), dpos.as<uint32_t>(), kept.size(), static_cast<G2A*>(d_out), st, sw);
      else
        fixed_base<G1>(ctx, ds.as<uint64_t>(), dpos.as<uint32_t>(), kept.size(), static_cast<G1A*>(d_out), st, sw);
      ZK_HIP(hipStreamSynchronize(st));  // dpos dies here
    });
  };
  build_slot({MSM_A, V, 0, false}, ha, sa);
  build_slot({MSM_B2, V, 0, false}, hb, sb);
  build_slot({MSM_B1, V, 0, false}, hb, sb);
  build_slot({MSM_IC, nic, num_public + 1, false}, hic, sic);
  build_slot({MSM_H, n, 0, true}, hh, sh);
  pk_finish(ctx, *d, q, own, st);
  *pk_dev = d.release();
  return ZK_OK;
}

// ---------------------------------------------------- QAP::evaluate_at ---
// A(t) = sum_i z_i A_i(t) = sum_j (Az)_j L_j(t) (A_i interpolates column i of
// the constraint matrix over the domain, qap:143-170; columns >= V dropped,
// qap:122-124), likewise B, C; Z(t) = t^n - 1 (qap:173-176, 211).
__global__ void __launch_bounds__(256) k_eval_rows(CsrArgs m, const Fr* __restrict__ zc, uint64_t nc, uint64_t V,
                                                   const Fr* __restrict__ L, Fr* __restrict__ out) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nc) return;
  const Fr l = ld_vec(&L[j]);
#pragma unroll
  for (int k = 0; k < 3; k++) st_vec(&out[k * nc + j], fp_mul(row_dot(m.rp[k], m.col[k], m.val[k], j, zc, V), l));
}
// out[b] = sum of in[i] over i = b, b + stride, ... (per block b: one LDS tree)
__global__ void __launch_bounds__(256) k_fr_sum(const Fr* __restrict__ in, uint64_t n, Fr* __restrict__ out) {
  __shared__ Fr part[256];
  Fr acc = fp_zero<FrParams>();
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    acc = fp_add(acc, ld_vec(&in[i]));
  part[threadIdx.x] = acc;
  __syncthreads();
  for (unsigned h = 128; h > 0; h >>= 1) {
    if (threadIdx.x < h) part[threadIdx.x] = fp_add(part[threadIdx.x], part[threadIdx.x + h]);
    __syncthreads();
  }
  if (threadIdx.x == 0) st_vec(&out[blockIdx.x], part[0]);
}

// sum of n device Fr (Montgomery) -> host canonical
static void fr_sum_to_host(const Fr* d_in, uint64_t n, zk_fr* out, hipStream_t st) {
  DevBuf part;
  const uint32_t nb = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(ceil_div(n, 256), 1), 1024);
  part.ensure(sizeof(Fr) * (nb + 1));
  k_fr_sum<<<nb, 256, 0, st>>>(d_in, n, part.as<Fr>());
  ZK_LAUNCH_CHECK();
  k_fr_sum<<<1, 256, 0, st>>>(part.as<Fr>(), nb, part.as<Fr>() + nb);
  ZK_LAUNCH_CHECK();
  fr_from_mont(part.as<Fr>() + nb, reinterpret_cast<uint64_t*>(part.as<Fr>() + nb), 1, st);
  ZK_HIP(hipMemcpyAsync(out, part.as<Fr>() + nb, sizeof(zk_fr), hipMemcpyDeviceToHost, st));
  ZK_HIP(hipStreamSynchronize(st));
}

int qap_evaluate_impl(zk_ctx* ctx, const zk_r1cs_csr* q, const zk_fr* point, const zk_fr* z, size_t zlen,
                      zk_fr out[4]) {
  hipStream_t st = ctx->stream;
  const uint64_t V = q->num_variables, nc = q->num_constraints;
  if (zlen != V) return ZK_ERR_DIMENSION;   // qap:191-198
  if (!fr_canonical(*point)) return ZK_ERR_ARG;
  for (size_t i = 0; i < zlen; i++)
    if (!fr_canonical(z[i])) return ZK_ERR_ARG;
  if (nc > (1ull << 32)) return ZK_ERR_DOMAIN;   // Fr 2-adicity 32 (qap:101-105); also keeps the loop finite
  uint64_t n = 1;
  while (n < nc) n <<= 1;
  const uint32_t log_n = (uint32_t)__builtin_ctzll(n);
  const host::Fr t = host::fr_to_mont(point->l);
  host::fr_from_mont(vanishing_at(t, log_n), out[3].l);
  for (int k = 0; k < 3; k++) std::memset(out[k].l, 0, 32);
  if (nc == 0) return ZK_OK;
  DevBuf wpow, L, dz, rows;
  CsrDev csr;
  csr_upload(csr, q, st);
  lagrange_at(t, log_n, wpow, L, st);
  dz.ensure(sizeof(zk_fr) * std::max<size_t>(zlen, 1));
  if (zlen) ZK_HIP(hipMemcpyAsync(dz.p, z, sizeof(zk_fr) * zlen, hipMemcpyHostToDevice, st));
  rows.ensure(sizeof(Fr) * 3 * nc);
  k_eval_rows<<<ceil_div(nc, 256), 256, 0, st>>>(csr_args(csr), dz.as<Fr>(), nc, V, L.as<Fr>(), rows.as<Fr>());
  ZK_LAUNCH_CHECK();
  for (int k = 0; k < 3; k++) fr_sum_to_host(rows.as<Fr>() + k * nc, nc, &out[k], st);
  return ZK_OK;
}
}  // namespace zk
