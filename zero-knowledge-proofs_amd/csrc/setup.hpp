// setup.hpp -- what setup.hip gives the C ABI (capi.hip, util.hip) and the
// test library (testhooks.hip).
#pragma once
#include "ctx.hpp"

namespace zk {
// pk_host: the whole key into the caller's arrays; else *pk_dev: this shard's
// device key.  vk (optional) either way.  sound: whole scalars and Z(tau) in
// the H query (zk_groth16_setup_sound) instead of the reference's lo64 ones.
int setup_impl(zk_ctx* ctx, const zk_r1cs_csr* q, const zk_setup_params* P, uint64_t num_public, uint32_t shard,
               uint32_t nshards, zk_pk* pk_host, zk_pk_dev** pk_dev, zk_vk* vk, bool sound = false);
// G * scalars[i] through the 255-bit fixed-base kernel (ZK_ERR_ARG for a scalar >= r)
int fixed_base_wide_host(zk_ctx* ctx, bool g2, const zk_fr* scalars, size_t n, uint64_t* host_out);
int qap_evaluate_impl(zk_ctx* ctx, const zk_r1cs_csr* q, const zk_fr* point, const zk_fr* z, size_t zlen,
                      zk_fr out[4]);
// CSR (nc rows) -> CSC over the columns < V: cp[V + 1], the entries' rows and
// (val != nullptr) their values, column by column in row order
void csr_to_csc(uint64_t nc, uint64_t V, const uint64_t* rp, const uint32_t* col, const zk_fr* val,
                std::vector<uint64_t>& cp, std::vector<uint32_t>& row, std::vector<zk_fr>& cval);
void bases_to_abi_host(bool g2, const void* d_in, uint32_t stride, size_t n, uint64_t* host_out, hipStream_t st);
}  // namespace zk
