// key.hpp -- building a device proving key (zk_pk_dev, ctx.hpp): pk_upload
// from a host key's ABI points, setup_impl (setup.hip) from the setup scalars
// on the device.  Which bases a shard keeps is decided here, once.
#pragma once
#include <functional>
#include <memory>
#include <vector>

#include "ctx.hpp"

namespace zk {

void csr_upload(CsrDev& d, const zk_r1cs_csr* q, hipStream_t st);
// An empty key: header fields and the constraint matrices on the device.
std::unique_ptr<zk_pk_dev> pk_create(zk_ctx* ctx, const zk_r1cs_csr* q, uint64_t num_public, uint32_t shard,
                                     uint32_t nshards, bool sound = false);

// One base vector: position i < len pairs with the scalar of variable
// i + idx_offset (H: coefficient i).  strided: a shard keeps positions
// i = shard mod nshards (H, where the distributed quotient leaves its
// coefficients); else its variables by var_owner, or without owners the
// contiguous range [len shard / nshards, len (shard + 1) / nshards).
struct SlotShape {
  int slot;
  uint64_t len, idx_offset;
  bool strided;
};
// The positions this shard keeps, ascending: its share by the rule above,
// without the identity bases (byte identity[i * stride] set: an ABI point's
// `infinity`, or a flag per zero setup scalar); they contribute nothing.
std::vector<uint32_t> shard_positions(const SlotShape& sh, uint32_t shard, uint32_t nshards,
                                      const std::vector<uint8_t>& own, const uint8_t* identity, size_t stride);

// What follows the compacted bases on shard 0 (other shards: nothing): pi_A
// gets alpha_1 (scalar 1) and 2^(64k) delta_1 (scalar r_k); pi_B gets beta_2
// and 2^(64k) delta_2 (s_k); B_1 gets beta_1.  A sound key takes whole
// scalars, so delta_1 (scalar r) and delta_2 (s) stand alone, without the
// 2^(64k) copies.
struct KeyExtras {
  std::vector<zk_g1_affine> a, b1;
  std::vector<zk_g2_affine> b2;
};
KeyExtras key_extras(uint32_t shard, const zk_g1_affine& alpha_g1, const zk_g1_affine& beta_g1,
                     const zk_g1_affine& delta_g1, const zk_g2_affine& beta_g2, const zk_g2_affine& delta_g2,
                     bool sound = false);

// Fill one slot from its kept positions: count, extras, idx (position +
// idx_offset), h_ident (H).  write_bases(pos, d_out) puts the compacted bases
// at d_out and returns with the stream idle; the slot's extras follow them.
using WriteBases = std::function<void(const std::vector<uint32_t>& pos, void* d_out)>;
void pk_fill_slot(zk_pk_dev& pk, const SlotShape& sh, const std::vector<uint32_t>& pos, const KeyExtras& ex,
                  hipStream_t st, const WriteBases& write_bases);
// Every slot filled: window copies, witness ranges, part cuts.
void pk_finish(zk_ctx* ctx, zk_pk_dev& pk, const zk_r1cs_csr* q, const std::vector<uint8_t>& own, hipStream_t st);

// The shard holding each variable's A / B1 / B2 / IC bases; empty: by range.
std::vector<uint8_t> var_owner(const zk_r1cs_csr* q, uint64_t n, uint32_t nshards);
zk_pk_dev* pk_upload(zk_ctx* ctx, const zk_pk* pk, const zk_r1cs_csr* q, uint32_t shard, uint32_t nshards,
                     bool sound = false);

}  // namespace zk
