// verify_all.hpp -- the host side that pairing.hip and verify_all.hip share, and
// the device state of one sound batch check (verify_all.hip), which the test
// hook zk_test_verify_all_parts (testhooks.hip) reads after the same chunked
// Miller and fold path.
#pragma once
#include "ctx.hpp"
#include "host_pairing.hpp"
#include "pairing.hpp"

namespace zk {

// pairing.hip: a host field element as 12 device Montgomery words, and the
// PR_STEPS affine lines of a fixed G2 point (48 words per step)
void put_fq(uint32_t* out, const host::Fq& m);
void line_table(const host::A2& Q, uint32_t* out);

// The arrays of one zk_groth16_verify_all_sound call.  Slot 0 of f12, g1 and
// fr holds the call's running accumulators
//   F = prod f(c_k A_k, B_k),  S_C = sum c_k C_k,  (s, t_0 .. t_{l-1})
// and slots 1 .. chunk the lanes of the chunk in flight; a fold leaves the
// new accumulators in slot 0.  fr: W = n_inputs + 1 Montgomery Fr per slot.
struct VerifyAll {
  DevBuf vk, proofs, in, co, bytes, pst, bad, f12, g1, fr, scal, terms, verdict;
  size_t W = 1;
  F12* F() const { return f12.as<F12>(); }
  XYZZ<FqC>* G() const { return g1.as<XYZZ<FqC>>(); }
  Fr* S() const { return fr.as<Fr>(); }
};

// Argument checks, tables, then every chunk through the Miller and fold
// kernels: the accumulators of the whole batch in slot 0 of S.  *first_bad:
// the lowest malformed proof, or n.  proofs or bytes, as verify_many_run.
int verify_all_accumulate(zk_ctx* ctx, const zk_vk* vk, const zk_proof* proofs, const uint8_t* bytes,
                          const zk_fr* inputs, size_t n_inputs, size_t n, const zk_fr* coeffs, size_t* first_bad,
                          uint8_t* point_status, VerifyAll& S);

}  // namespace zk
