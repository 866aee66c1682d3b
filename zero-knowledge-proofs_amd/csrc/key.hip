// key.hip -- the device proving key (zk_pk_dev, key.hpp): the constraint
// matrices, each shard's compacted bases and extras (prove.hip says why), the
// window-shifted copies, the witness ranges and the part cuts.
#include <algorithm>
#include <cstring>

#include "host_pairing.hpp"
#include "key.hpp"

namespace zk {

// ------------------------------------------------------------------ CSR ---
__global__ void __launch_bounds__(256) k_u64_to_fr_mont(const uint64_t* __restrict__ in, Fr* __restrict__ out,
                                                        size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  st_vec(&out[i], fp_to_mont(ld_vec(reinterpret_cast<const Fr*>(in) + i)));
}

void csr_upload(CsrDev& d, const zk_r1cs_csr* q, hipStream_t st) {
  d.nc = q->num_constraints;
  d.V = q->num_variables;
  const uint64_t* rps[3] = {q->a_rowptr, q->b_rowptr, q->c_rowptr};
  const uint32_t* cols[3] = {q->a_col, q->b_col, q->c_col};
  const zk_fr* vals[3] = {q->a_val, q->b_val, q->c_val};
  for (int m = 0; m < 3; m++) {
    const uint64_t nnz = d.nc ? rps[m][d.nc] : 0;
    d.rp[m].ensure(sizeof(uint64_t) * (d.nc + 1));
    ZK_HIP(hipMemcpyAsync(d.rp[m].p, rps[m], sizeof(uint64_t) * (d.nc + 1), hipMemcpyHostToDevice, st));
    d.col[m].ensure(sizeof(uint32_t) * std::max<uint64_t>(nnz, 1));
    if (nnz) ZK_HIP(hipMemcpyAsync(d.col[m].p, cols[m], sizeof(uint32_t) * nnz, hipMemcpyHostToDevice, st));
    d.unit[m] = vals[m] == nullptr;
    if (!d.unit[m] && nnz) {
      DevBuf tmp;
      tmp.ensure(sizeof(zk_fr) * nnz);
      ZK_HIP(hipMemcpyAsync(tmp.p, vals[m], sizeof(zk_fr) * nnz, hipMemcpyHostToDevice, st));
      d.val[m].ensure(sizeof(Fr) * nnz);
      k_u64_to_fr_mont<<<ceil_div(nnz, 256), 256, 0, st>>>(tmp.as<uint64_t>(), d.val[m].as<Fr>(), nnz);
      ZK_LAUNCH_CHECK();
      ZK_HIP(hipStreamSynchronize(st));  // tmp dies here
    }
  }
}

std::unique_ptr<zk_pk_dev> pk_create(zk_ctx* ctx, const zk_r1cs_csr* q, uint64_t num_public, uint32_t shard,
                                     uint32_t nshards, bool sound) {
  if (sound && nshards != 1) throw Error(ZK_ERR_ARG, "a sound proving key cannot be sharded");
  std::unique_ptr<zk_pk_dev> d(new zk_pk_dev());
  d->device = ctx->device;
  d->scalar_bits = sound ? 255 : 64;
  d->V = q->num_variables;
  d->nc = q->num_constraints;
  if (d->nc > (1ull << 32)) throw Error(ZK_ERR_DOMAIN, "more than 2^32 constraints (Fr 2-adicity 32)");
  d->n = 1;
  while (d->n < d->nc) d->n <<= 1;
  d->log_n = (uint32_t)__builtin_ctzll(d->n);
  d->num_public = num_public;
  d->shard = shard;
  d->nshards = nshards;
  csr_upload(d->csr, q, ctx->stream);
  return d;
}

// ---------------------------------------------------------------- slots ---
std::vector<uint32_t> shard_positions(const SlotShape& sh, uint32_t shard, uint32_t nshards,
                                      const std::vector<uint8_t>& own, const uint8_t* identity, size_t stride) {
  const bool by_owner = !sh.strided && !own.empty();
  uint64_t lo = 0, hi = sh.len, step = 1;
  if (sh.strided) {
    lo = std::min<uint64_t>(shard, sh.len);
    step = nshards;
  } else if (!by_owner) {
    lo = sh.len * shard / nshards;
    hi = sh.len * (shard + 1) / nshards;
  }
  std::vector<uint32_t> pos;
  for (uint64_t i = lo; i < hi; i += step)
    if (!identity[i * stride] && (!by_owner || own[i + sh.idx_offset] == shard)) pos.push_back((uint32_t)i);
  return pos;
}

// [P, 2^64 P, 2^128 P, 2^192 P] in ABI form
template <class C, class ABI>
static void pow64_chain(const host::X<typename C::HF>& P, ABI* out) {
  host::X<typename C::HF> q = P;
  for (int k = 0; k < 4; k++) {
    host_to_abi<C>(q, reinterpret_cast<uint64_t*>(&out[k]));
    for (int d = 0; d < 64; d++) q = host::dbl(q);
  }
}

KeyExtras key_extras(uint32_t shard, const zk_g1_affine& alpha_g1, const zk_g1_affine& beta_g1,
                     const zk_g1_affine& delta_g1, const zk_g2_affine& beta_g2, const zk_g2_affine& delta_g2,
                     bool sound) {
  KeyExtras ex;
  if (shard != 0) return ex;
  if (sound) {   // whole scalars: 1 alpha_1 + r delta_1, 1 beta_2 + s delta_2, 1 beta_1
    ex.a = {alpha_g1, delta_g1};
    ex.b2 = {beta_g2, delta_g2};
    ex.b1 = {beta_g1};
    return ex;
  }
  ex.a.resize(5);
  ex.a[0] = alpha_g1;
  pow64_chain<G1>(host::x_from_abi(delta_g1), &ex.a[1]);
  ex.b2.resize(5);
  ex.b2[0] = beta_g2;
  pow64_chain<G2>(host::x_from_abi(delta_g2), &ex.b2[1]);
  ex.b1.push_back(beta_g1);
  return ex;
}

template <class C, class ABI>
static void append_extras(zk_pk_dev& pk, int slot, const std::vector<ABI>& extras, hipStream_t st) {
  const uint32_t nex = (uint32_t)extras.size();
  if (!nex) return;
  DevBuf ex;
  ex.ensure(sizeof(ABI) * nex);
  ZK_HIP(hipMemcpyAsync(ex.p, extras.data(), sizeof(ABI) * nex, hipMemcpyHostToDevice, st));
  convert_bases<C>(ex.as<uint64_t>(), pk.bases[slot].as<typename C::A>() + pk.count[slot], nex, st);
  ZK_HIP(hipStreamSynchronize(st));  // ex dies here
}

void pk_fill_slot(zk_pk_dev& pk, const SlotShape& sh, const std::vector<uint32_t>& pos, const KeyExtras& ex,
                  hipStream_t st, const WriteBases& write_bases) {
  const int slot = sh.slot;
  const uint32_t cnt = (uint32_t)pos.size();
  const uint32_t nex = (uint32_t)(slot == MSM_A ? ex.a.size() : slot == MSM_B2 ? ex.b2.size()
                                                             : slot == MSM_B1 ? ex.b1.size() : 0);
  std::vector<uint32_t> gidx(cnt);
  for (uint32_t k = 0; k < cnt; k++) gidx[k] = (uint32_t)(pos[k] + sh.idx_offset);
  if (slot == MSM_H) {
    pk.h_ident = true;
    for (uint32_t k = 0; k < cnt; k++) pk.h_ident = pk.h_ident && gidx[k] == k;
  }
  pk.count[slot] = cnt;
  pk.extras[slot] = nex;
  pk.bases[slot].ensure((slot == MSM_B2 ? sizeof(G2A) : sizeof(G1A)) * std::max<uint64_t>((uint64_t)cnt + nex, 1));
  pk.idx[slot].ensure(sizeof(uint32_t) * std::max<uint32_t>(cnt, 1));
  if (cnt) {
    ZK_HIP(hipMemcpyAsync(pk.idx[slot].p, gidx.data(), sizeof(uint32_t) * cnt, hipMemcpyHostToDevice, st));
    write_bases(pos, pk.bases[slot].p);
  }
  if (slot == MSM_A) append_extras<G1>(pk, slot, ex.a, st);
  else if (slot == MSM_B2) append_extras<G2>(pk, slot, ex.b2, st);
  else if (slot == MSM_B1) append_extras<G1>(pk, slot, ex.b1, st);
  ZK_HIP(hipStreamSynchronize(st));  // gidx dies here
}

// ------------------------------------------------------------- pk upload ---
// One base vector of a host key: its non-identity points at this shard's
// positions, compacted and converted.
template <class C, class ABI>
static void upload_slot(zk_pk_dev& d, const SlotShape& sh, const ABI* v, const std::vector<uint8_t>& own,
                        const KeyExtras& ex, hipStream_t st) {
  const std::vector<uint32_t> pos =
      shard_positions(sh, d.shard, d.nshards, own, v ? &v->infinity : nullptr, sizeof(ABI));
  pk_fill_slot(d, sh, pos, ex, st, [&](const std::vector<uint32_t>& kept, void* d_out) {
    std::vector<ABI> pts;
    pts.reserve(kept.size());
    for (uint32_t i : kept) pts.push_back(v[i]);
    DevBuf raw;
    raw.ensure(sizeof(ABI) * pts.size());
    ZK_HIP(hipMemcpyAsync(raw.p, pts.data(), sizeof(ABI) * pts.size(), hipMemcpyHostToDevice, st));
    convert_bases<C>(raw.as<uint64_t>(), static_cast<typename C::A*>(d_out), pts.size(), st);
    ZK_HIP(hipStreamSynchronize(st));  // pts / raw die here
  });
}

zk_pk_dev* pk_upload(zk_ctx* ctx, const zk_pk* pk, const zk_r1cs_csr* q, uint32_t shard, uint32_t nshards,
                     bool sound) {
  hipStream_t st = ctx->stream;
  std::unique_ptr<zk_pk_dev> d = pk_create(ctx, q, pk->num_public, shard, nshards, sound);
  const KeyExtras ex = key_extras(shard, pk->alpha_g1, pk->beta_g1, pk->delta_g1, pk->beta_g2, pk->delta_g2, sound);
  const uint64_t V = d->V, first_private = pk->num_public + 1;
  const std::vector<uint8_t> own = var_owner(q, d->n, nshards);
  // the a/b vectors may be shorter than V (core:171 `i < pk.a_g1.len()`): indices stay < V.
  upload_slot<G1>(*d, {MSM_A, std::min<uint64_t>(pk->a_len, V), 0, false}, pk->a_g1, own, ex, st);     // core:171
  upload_slot<G2>(*d, {MSM_B2, std::min<uint64_t>(pk->b2_len, V), 0, false}, pk->b_g2, own, ex, st);   // core:189
  upload_slot<G1>(*d, {MSM_B1, std::min<uint64_t>(pk->b_len, V), 0, false}, pk->b_g1, own, ex, st);    // core:250
  // ic_g1[k] pairs with variable k + num_public + 1 (core:227-231)
  upload_slot<G1>(*d, {MSM_IC, std::min<uint64_t>(pk->ic_len, V > first_private ? V - first_private : 0),
                       first_private, false}, pk->ic_g1, own, ex, st);
  // h_g1[i] pairs with H coefficient i (zip, core:211-215); H has n coefficients
  upload_slot<G1>(*d, {MSM_H, std::min<uint64_t>(pk->h_len, d->n), 0, true}, pk->h_g1, own, ex, st);
  pk_finish(ctx, *d, q, own, st);
  return d.release();
}

// -------------------------------------------------------------- the rest ---
// out[k] = first position of idx[0, count) holding a value >= key (the idx
// vectors ascend: compaction keeps variable order)
__global__ void k_lower_bound(const uint32_t* __restrict__ idx, uint32_t count, uint64_t key, uint32_t* __restrict__ out) {
  uint32_t lo = 0, hi = count;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if ((uint64_t)idx[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  *out = lo;
}

// The parts of a host witness grow geometrically, ZK_HOST_PART_RATIO times
// each (2 parts, ratio 2: the first third, then the rest): the MSM work of
// the parts already on the device outlasts the copy of the next one.  Every
// part costs its own sort, bucket fixup and combine on the G2 and A+B1+IC
// streams, so more, smaller parts lose what the smaller exposed first copy
// saves.  Host-witness minus device-witness prove at 2^20 (tools/pcie_ab.py,
// medians of 4 alternating processes, profiles/r05_ab_host_parts.txt): 2
// parts +0.864 ms, 3 parts (ratio 3) +1.042, 4 parts (ratio 2.5) +1.231;
// round 4 with 2 parts, first part 1/2 +1.33, 1/3 +0.84, 1/4 +0.86, 1/6 +1.29
// (profiles/r04_ab_host_split.txt).  (ZK_HOST_PARTS / ZK_HOST_PART_RATIO:
// A/B builds only.)
#ifndef ZK_HOST_PART_RATIO
#define ZK_HOST_PART_RATIO 2
#endif
static void pk_part_cuts(zk_pk_dev& pk, hipStream_t st) {
  double w = 1, tot = 0;
  double f[HOST_PARTS];
  for (int k = 0; k < HOST_PARTS; k++, w *= ZK_HOST_PART_RATIO) tot += (f[k] = w);
  double acc = 0;
  pk.vcut[0] = 0;
  for (int k = 1; k < HOST_PARTS; k++) {
    acc += f[k - 1] / tot;
    pk.vcut[k] = std::max<uint64_t>(pk.vcut[k - 1], (uint64_t)(acc * (double)pk.V));
  }
  pk.vcut[HOST_PARTS] = pk.V;
  DevBuf d;
  d.ensure(sizeof(uint32_t) * NUM_MSM * (HOST_PARTS + 1));
  ZK_HIP(hipMemsetAsync(d.p, 0, sizeof(uint32_t) * NUM_MSM * (HOST_PARTS + 1), st));
  for (int k = 1; k < HOST_PARTS; k++)
    for (int slot : {MSM_A, MSM_B2, MSM_B1, MSM_IC})
      if (pk.count[slot]) {
        k_lower_bound<<<1, 1, 0, st>>>(pk.idx[slot].as<uint32_t>(), pk.count[slot], pk.vcut[k],
                                       d.as<uint32_t>() + k * NUM_MSM + slot);
        ZK_LAUNCH_CHECK();
      }
  ZK_HIP(hipMemcpyAsync(pk.pcut, d.p, sizeof(uint32_t) * NUM_MSM * (HOST_PARTS + 1), hipMemcpyDeviceToHost, st));
  ZK_HIP(hipStreamSynchronize(st));
  for (int slot = 0; slot < NUM_MSM; slot++) pk.pcut[HOST_PARTS][slot] = pk.count[slot];
}

// With a distributed quotient possible (nshards 2, 4 or 8, n % nshards^2 ==
// 0) a variable belongs to the shard whose quotient rows first reference it,
// so a rank's MSM variables are the ones its quotient rows read anyway and
// its witness slice is ~1/nshards of z; unreferenced variables by range.
std::vector<uint8_t> var_owner(const zk_r1cs_csr* q, uint64_t n, uint32_t N) {
  std::vector<uint8_t> own;
  if (N < 2 || !dist_quotient_ok(n, (int)N)) return own;
  const uint64_t V = q->num_variables, nc = q->num_constraints, m = n / N, qq = m / N;
  own.assign(V, 0xff);
  const uint64_t* rps[3] = {q->a_rowptr, q->b_rowptr, q->c_rowptr};
  const uint32_t* cols[3] = {q->a_col, q->b_col, q->c_col};
  for (uint64_t j = 0; j < nc; j++) {   // rank of row j: its column b = j mod m lies in [rank q, rank q + q)
    const uint8_t rk = (uint8_t)((j % m) / qq);
    for (int mtx = 0; mtx < 3; mtx++)
      for (uint64_t e = rps[mtx][j]; e < rps[mtx][j + 1]; e++) {
        const uint32_t c = cols[mtx][e];
        if (c < V && own[c] == 0xff) own[c] = rk;
      }
  }
  for (uint64_t v = 0; v < V; v++)
    if (own[v] == 0xff) own[v] = (uint8_t)(v * N / V);
  return own;
}

// Exactly the z entries a shard reads when its quotient is distributed:
// z_0 (the constant check, core:89-93), the variables behind its compacted
// A / B2 / B1 / IC bases (the idx vectors) and the columns of the rows its
// column slice evaluates (dist.hip stage A: rows a m + rank q + b', a < N,
// b' < q), plus the variables var_owner gives this shard: a variable no row
// references and whose bases are all the identity is read by no stage, but
// it must still be checked canonical by some rank (the one-GPU prove rejects
// z_i >= r anywhere).  For a variable rows do reference, its owner's rows
// read it anyway.  Sorted, merged into ranges.
static void pk_witness_ranges(zk_pk_dev& pk, const zk_r1cs_csr* q, const std::vector<uint8_t>& own, hipStream_t st) {
  pk.wr_dist.clear();
  if (pk.nshards < 2 || !dist_quotient_ok(pk.n, (int)pk.nshards)) return;
  std::vector<uint32_t> vars;
  for (int slot : {MSM_A, MSM_B2, MSM_B1, MSM_IC}) {
    const size_t k = vars.size();
    vars.resize(k + pk.count[slot]);
    if (pk.count[slot])
      ZK_HIP(hipMemcpyAsync(vars.data() + k, pk.idx[slot].p, sizeof(uint32_t) * pk.count[slot],
                            hipMemcpyDeviceToHost, st));
  }
  ZK_HIP(hipStreamSynchronize(st));
  vars.push_back(0);
  for (uint64_t v = 0; v < own.size(); v++)
    if (own[v] == pk.shard) vars.push_back((uint32_t)v);
  const uint64_t N = pk.nshards, m = pk.n / N, qq = m / N;
  const uint64_t* rps[3] = {q->a_rowptr, q->b_rowptr, q->c_rowptr};
  const uint32_t* cols[3] = {q->a_col, q->b_col, q->c_col};
  for (uint64_t a = 0; a < N; a++)
    for (uint64_t b = 0; b < qq; b++) {
      const uint64_t j = a * m + pk.shard * qq + b;
      if (j >= pk.nc) continue;
      for (int mtx = 0; mtx < 3; mtx++)
        for (uint64_t e = rps[mtx][j]; e < rps[mtx][j + 1]; e++)
          if (cols[mtx][e] < pk.V) vars.push_back(cols[mtx][e]);   // columns >= V are ignored (qap:122-124)
    }
  std::sort(vars.begin(), vars.end());
  vars.erase(std::unique(vars.begin(), vars.end()), vars.end());
  for (uint32_t v : vars) {
    if (!pk.wr_dist.empty() && pk.wr_dist.back() == v) pk.wr_dist.back() = (uint64_t)v + 1;
    else {
      pk.wr_dist.push_back(v);
      pk.wr_dist.push_back((uint64_t)v + 1);
    }
  }
}

// The prove MSMs all take 64-bit scalars (lo64, core:156-161 / 203-208, and
// the u64 limbs of r, s against 2^(64k) delta): c = 16 gives 4 windows whose
// shifted bases 2^16 P, 2^32 P, 2^48 P are computed once here, so each MSM
// sums into one set of 2^16 buckets instead of 3 x 2^15 + 2^16.
// c = 22 gives 3 windows over 2^21 buckets per MSM instead: 25 % fewer
// accumulate adds against a 32x larger bucket reduction (~12 ms per proof).
// Measured (window sweep): 2x slower at 2^20 constraints, 7 %
// faster at 2^24 -- so 22 from 2^24 constraints per key shard up.
// zk_ctx_set_option(ZK_OPT_PROVE_WIN_C) forces 16 or 22 (tests).
static int prove_win_c(const zk_ctx* ctx, const zk_pk_dev& pk) {
  if (ctx->prove_win_c) return ctx->prove_win_c;
  return pk.n / std::max<uint64_t>(pk.nshards, 1) >= (1ull << 24) ? 22 : 16;
}

// A sound key's MSMs take whole 255-bit scalars: ceil(255 / c) shifted copies,
// 16 at c = 16 (2^15 buckets per MSM), 13 at c = 20 (2^19), 12 at c = 22
// (2^21).  The sweep behind the default is in DESIGN.md 2.12.
// zk_ctx_set_option(ZK_OPT_SOUND_WIN_C) forces 16, 20 or 22.
constexpr int SOUND_WIN_C_DEFAULT = 20;
static int sound_win_c(const zk_ctx* ctx) { return ctx->sound_win_c ? ctx->sound_win_c : SOUND_WIN_C_DEFAULT; }

// The `copies` window copies of one MSM slot's bases (MSM_H: of [IC | H]),
// padded to whole lines, in place of the bases themselves.
static void pk_precompute_slot(zk_ctx* ctx, zk_pk_dev& pk, int slot, int win_c, int copies) {
  hipStream_t st = ctx->stream;
  const size_t n = slot == MSM_H ? pk.ich_tot() : (size_t)pk.count[slot] + pk.extras[slot];
  const size_t asz = slot == MSM_B2 ? sizeof(G2A) : sizeof(G1A);
  // every entry of an MSM indexes a base of one of the copies in 31 bits (msm.hip)
  if ((uint64_t)n * copies >= MSM_DUMMY)
    throw Error(ZK_ERR_ARG, "proving key: " + std::to_string(n) + " bases x " + std::to_string(copies) +
                                " window copies exceed the 2^31 window bases of one MSM");
  DevBuf big;
  big.ensure(asz * std::max<size_t>(n * copies, 1));
  if (slot == MSM_H) {   // [IC | H]
    const size_t nic = (size_t)pk.count[MSM_IC] + pk.extras[MSM_IC], nh = n - nic;
    if (nic) ZK_HIP(hipMemcpyAsync(big.p, pk.bases[MSM_IC].p, asz * nic, hipMemcpyDeviceToDevice, st));
    if (nh)
      ZK_HIP(hipMemcpyAsync(static_cast<char*>(big.p) + asz * nic, pk.bases[MSM_H].p, asz * nh,
                            hipMemcpyDeviceToDevice, st));
    ZK_HIP(hipStreamSynchronize(st));
    pk.bases[MSM_IC].release();
  } else if (n) {
    ZK_HIP(hipMemcpyAsync(big.p, pk.bases[slot].p, asz * n, hipMemcpyDeviceToDevice, st));
  }
  if (slot == MSM_B2) msm_precompute_windows<G2>(big.as<G2A>(), n, copies, win_c, st);
  else msm_precompute_windows<G1>(big.as<G1A>(), n, copies, win_c, st);
  ZK_HIP(hipStreamSynchronize(st));
  pk.stride[slot] = slot == MSM_B2 ? msm_pad_bases<G2>(big, n * copies, st) : msm_pad_bases<G1>(big, n * copies, st);
  pk.bases[slot] = std::move(big);
}

// zk_ctx_set_option(ZK_OPT_SOUND_COPIES) keeps only the first S of a sound
// key's W copies: its MSMs then sum window w over copy w mod S into bucket
// set w / S (msm_make_plan_grouped) -- S / W of the base memory against
// ceil(W / S) bucket reductions per MSM.  A reference-mode
// key keeps every copy: its batched MSMs own one bucket set each.
static void pk_precompute_windows(zk_ctx* ctx, zk_pk_dev& pk) {
  const int PROVE_WIN_C = pk.sound() ? sound_win_c(ctx) : prove_win_c(ctx, pk);
  const int PROVE_WIN = ((int)pk.scalar_bits + PROVE_WIN_C - 1) / PROVE_WIN_C;
  const int COPIES = pk.sound() && ctx->sound_copies ? std::min(ctx->sound_copies, PROVE_WIN) : PROVE_WIN;
  for (int slot = 0; slot < NUM_MSM; slot++) {
    if (slot == MSM_IC) continue;   // windowed together with H (zk_pk_dev::ich_tot)
    try {
      pk_precompute_slot(ctx, pk, slot, PROVE_WIN_C, COPIES);
    } catch (const Error& e) {
      if (e.code != ZK_ERR_DEVICE || !pk.sound()) throw;
      // most likely a key that does not fit: say which knob shrinks it
      throw Error(ZK_ERR_DEVICE, std::string(e.what()) + " (a sound key holding " + std::to_string(COPIES) + " of " +
                                     std::to_string(PROVE_WIN) +
                                     " window copies of every base: ZK_OPT_SOUND_COPIES keeps fewer)");
    }
  }
  pk.win = PROVE_WIN;
  pk.win_c = PROVE_WIN_C;
  pk.copies = COPIES;
}

void pk_finish(zk_ctx* ctx, zk_pk_dev& pk, const zk_r1cs_csr* q, const std::vector<uint8_t>& own, hipStream_t st) {
  pk_precompute_windows(ctx, pk);
  pk_witness_ranges(pk, q, own, st);
  pk_part_cuts(pk, st);
}

}  // namespace zk
