// keycheck.hpp -- a sound key audited against the powers-of-tau string it
// claims to come from (keycheck.hip; include/zkp.h, "a key against its
// string").
#pragma once
#include "ctx.hpp"

namespace zk {

// The six coefficient vectors m^{M,part} = iNTT_n(rows of M times rho^part),
// M in {A, B, C}, part in {pub, priv} (rho split at column num_public), as
// 6 n Montgomery Fr in d_out: A pub, A priv, B pub, B priv, C pub, C priv.
// rho: num_variables canonical values.  On the ctx's main stream, not
// synchronised; the CSR's device copy lives in `keep` until the caller has
// synchronised.  ZK_ERR_ARG (an Error) for row pointers that do not ascend.
struct KeySrsScratch {
  DevBuf rp[3], col[3], val[3], rho, tmp;
};
void key_srs_coeffs_device(zk_ctx* ctx, const zk_r1cs_csr* q, uint64_t num_public, const zk_fr* rho, uint32_t log_n,
                           Fr* d_out, KeySrsScratch& keep);
// the same as canonical values in host memory (the test library's hook)
int key_srs_coeffs_host(zk_ctx* ctx, const zk_r1cs_csr* q, uint64_t num_public, const zk_fr* rho, zk_fr* out);

}  // namespace zk
