// prove.hpp -- the prove entry points behind the C ABI (prove.hip).
#pragma once
#include <vector>

#include "ctx.hpp"

namespace zk {

// canonical-input checks: a < r on the host; on the device, flags |= 8 when
// some of the n canonical Fr at d_z is >= r
bool fr_canonical(const zk_fr& a);
void check_canonical(const void* d_z, uint64_t n, uint32_t* d_flags, hipStream_t st);

// n device Fr (Montgomery) -> MSM scalars of sw u64 words each: the low 64
// bits of the canonical value (sw = 1) or all of it (sw = 4)
void fr_to_scalars(const Fr* d_in, size_t n, int sw, uint64_t* d_out, hipStream_t st);

// z_host: the witness is still on the host (d_z: the ctx's device copy of it)
int prove_impl(zk_ctx* ctx, const zk_pk_dev* pk, const void* d_z, size_t zlen, size_t num_public, const zk_fr* r,
               const zk_fr* s, zk_proof* out, const zk_fr* z_host = nullptr);
int prove_partial_impl(zk_ctx* ctx, const zk_pk_dev* pk, const void* d_z, size_t zlen, size_t num_public,
                       const zk_fr* r, const zk_fr* s, zk_prove_partial* out);
int prove_partial_host_impl(zk_ctx* ctx, const zk_pk_dev* pk, const zk_fr* z_slice, size_t slice_len, size_t zlen,
                            size_t num_public, const zk_fr* r, const zk_fr* s, zk_prove_partial* out);
int prove_virtual_shards_impl(zk_ctx* ctx, const zk_pk_dev* const* pks, uint32_t N, const void* d_z, size_t zlen,
                              size_t num_public, const zk_fr* r, const zk_fr* s, zk_proof* out);
int combine_impl(const zk_prove_partial* parts, size_t k, const zk_fr* r, const zk_fr* s, zk_proof* out);
std::vector<uint64_t> witness_ranges(const zk_ctx* ctx, const zk_pk_dev* pk);

}  // namespace zk
