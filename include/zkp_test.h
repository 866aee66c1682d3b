/*
 * zkp_test.h -- diagnostic entry points of libzkp_amd_test.so, a separate
 * library built on top of libzkp_amd.so for the GPU tests.  None of these is
 * part of the drop-in ABI (include/zkp.h) and none has a reference
 * counterpart: they reach paths a one-GPU box cannot reach through the
 * product ABI (N ranks on one device) and inject failures.
 */
#ifndef ZKP_TEST_H
#define ZKP_TEST_H
#include "zkp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nshards virtual ranks of one key on this ctx's single device (the
 * distributed quotient's all-to-alls become device copies) -- checks the
 * distributed path's arithmetic and index maps without N devices. */
int zk_test_prove_virtual_shards(zk_ctx *ctx, const zk_pk_dev *const *shards, uint32_t nshards,
                                 const void *d_z, size_t zlen, size_t num_public, const zk_fr *r,
                                 const zk_fr *s, zk_proof *out);
/* The attached exchange's two operations on their own, on the ctx's stream
 * -- one all-to-all of chunk_bytes per rank over a device buffer whose chunk
 * k holds bytes (rank * 31 + k * 7 + i) & 0xff, then the status agreement of
 * `status`.  *out_max = the agreed maximum; ZK_OK when every received chunk
 * s equals what rank s sent, ZK_ERR_RCCL otherwise (or on a transport
 * error).  Runs ncclAllToAll / ncclAllReduce themselves on a world-1 RCCL
 * communicator, where a one-GPU box can reach them. */
int zk_test_exchange(zk_ctx *ctx, size_t chunk_bytes, int32_t status, int32_t *out_max);
/* k = 1..3: the next distributed-quotient proof on this ctx fails right
 * after its k-th all-to-all, as a rank-local error would (tests of the abort
 * path); 0 clears it.  ZK_ERR_ARG without an attached exchange. */
int zk_test_fault_after_exchange(zk_ctx *ctx, int k);
/* Readback of a device proving key (setup parity at size): slot 0 pi_A
 * (a_g1), 1 pi_B (b_g2), 2 B_1 (b_g1), 3 IC (ic_g1), 4 H (h_g1); window w
 * of the window-shifted copies (w = 0: the bases themselves, w: 2^(win_c w)
 * times them).  *count = compacted non-identity bases of this shard,
 * *nextras = extra bases appended after them (shard 0: alpha_1 and
 * 2^(64k) delta_1 / beta_2 and 2^(64k) delta_2 / beta_1; a sound key:
 * alpha_1, delta_1 / beta_2, delta_2 / beta_1, and ceil(255 / win_c)
 * windows).  window < the copies the key holds (zk_test_pk_plan: every
 * window unless the key was made under ZK_OPT_SOUND_COPIES).  With cap >=
 * count + nextras: idx_out[k] = the variable (H: coefficient) index of base
 * k < count, words_out = all count + nextras bases as canonical ABI words
 * (13 per G1, 25 per G2 point).  cap = 0 only queries the counts. */
int zk_test_pk_bases(zk_ctx *ctx, const zk_pk_dev *pk, int slot, int window, uint32_t *idx_out,
                     uint64_t *words_out, size_t cap, size_t *count, size_t *nextras);
/* The key's window plan and shard: win copies of c = win_c bits. */
int zk_test_pk_info(const zk_pk_dev *pk, uint32_t *win, uint32_t *win_c, uint32_t *shard, uint32_t *nshards);
/* The copies of every base the key holds (win unless ZK_OPT_SOUND_COPIES
 * kept fewer) and the bucket sets of each of its prove MSMs,
 * ceil(win / copies). */
int zk_test_pk_plan(const zk_pk_dev *pk, uint32_t *copies, uint32_t *sets);
/* The 255-bit fixed-base kernel of a sound setup (csrc/setup.hip,
 * k_fixed_base_wide) on its own, one lane per scalar: out[i] = scalars[i] G
 * for n whole canonical scalars, G the G1 generator.  A scalar >= r is
 * ZK_ERR_ARG. */
int zk_test_fixed_base_g1(zk_ctx *ctx, const zk_fr *scalars, size_t n, zk_g1_affine *out);
/* Same with the G2 generator. */
int zk_test_fixed_base_g2(zk_ctx *ctx, const zk_fr *scalars, size_t n, zk_g2_affine *out);
/* zk_g1_mul_scalar through the plain 255-bit double-and-add walk
 * (csrc/ceremony.hpp, cm_walk_plain) instead of the endomorphism walk the
 * library ships: the on-GPU cross-check of that walk and its timing baseline
 * (profiler phase g1_mul_scalar_plain).  Same arguments, errors and chunking. */
int zk_test_g1_mul_scalar_plain(zk_ctx *ctx, const zk_g1_affine *pts, size_t n, const zk_fr *k,
                                zk_g1_affine *out);
/* zk_g1_mul_scalars / zk_g2_mul_scalars through the plain per-lane 255-bit
 * double-and-add walk (csrc/srs.hpp, gn_walk_aff, every lane from bit 254)
 * instead of the table walks of csrc/mulvec.hpp: their on-GPU cross-check and
 * timing baseline (profiler phases g1_mul_scalars_plain, g2_mul_scalars_plain).
 * Same arguments, errors and chunking. */
int zk_test_g1_mul_scalars_plain(zk_ctx *ctx, const zk_g1_affine *pts, size_t n, const zk_fr *k,
                                 zk_g1_affine *out);
int zk_test_g2_mul_scalars_plain(zk_ctx *ctx, const zk_g2_affine *pts, size_t n, const zk_fr *k,
                                 zk_g2_affine *out);
/* The table walks themselves (profiler phases g1_mul_scalars_table,
 * g2_mul_scalars_table), whichever walk the public calls ship. */
int zk_test_g1_mul_scalars_table(zk_ctx *ctx, const zk_g1_affine *pts, size_t n, const zk_fr *k,
                                 zk_g1_affine *out);
int zk_test_g2_mul_scalars_table(zk_ctx *ctx, const zk_g2_affine *pts, size_t n, const zk_fr *k,
                                 zk_g2_affine *out);
/* The device decomposition of those walks alone, one lane per scalar: for n
 * canonical scalars below r (else ZK_ERR_ARG), g1_out[4 i ..] = e1 (two words),
 * e2 (two words) with (e2, e1) = divmod(k[i], x^2), g2_out[4 i ..] = the four
 * base-x digits of k[i], x = 0xd201000000010000. */
int zk_test_split_scalars(zk_ctx *ctx, const zk_fr *k, size_t n, uint64_t *g1_out, uint64_t *g2_out);
/* The per-lane double-and-add walks of csrc/srs.hpp on their own, one lane per
 * point in blocks of 128 lanes: out[i] = k[i] pts[i], every lane handing the
 * helper the top set bit of ITS OWN scalar -- the lengths differ between the
 * lanes of a wave, exactly as the group transform's stages (gn_stage) and the
 * column sums (gn_col_runs) call these helpers, and unlike
 * zk_test_g*_mul_scalars_plain, which walk every lane from bit 254 (the helper
 * itself walks a wave from its longest lane's top bit).
 * g2 = 0: pts and out are zk_g1_affine,
 * 1: zk_g2_affine.  mem = 0: gn_walk_aff (mixed additions of the affine point);
 * mem = 1: gn_walk_mem, the point stored as XYZZ in a slot of the lane's own
 * first and fetched a coordinate at a time inside the full addition.  An
 * identity point or a zero scalar gives the identity; the points are taken as
 * valid.  A scalar >= r is ZK_ERR_ARG (zk_last_error names the index), as is
 * g2 or mem outside {0, 1}.  Chunking as zk_g1_mul_scalars
 * (ZK_OPT_POINT_CHUNK); n = 0 does nothing. */
int zk_test_gn_walk(zk_ctx *ctx, int g2, int mem, const void *pts, size_t n, const zk_fr *k, void *out);
/* The device square roots behind point decompression (csrc/points.hpp), one
 * lane per element: in = n canonical Fq (6 words each), out = a canonical
 * root where ok[i] = 1 (zeros where the input has none), largest[i] = the
 * encodings' sort-flag predicate on that root (out > (p - 1) / 2).  Curve
 * points never reach the rare branches (0, -1, roots with a zero
 * coefficient, an Fq non-residue inside Fq2); these hooks do. */
int zk_test_fq_sqrt(zk_ctx *ctx, const uint64_t *in, size_t n, uint64_t *out, uint8_t *ok, uint8_t *largest);
/* Same in Fq2: 12 words per element (c0 then c1); largest looks at c1, or at
 * c0 when c1 == 0. */
int zk_test_fq2_sqrt(zk_ctx *ctx, const uint64_t *in, size_t n, uint64_t *out, uint8_t *ok, uint8_t *largest);
/* The device Fq12 tower behind the pairing kernels (csrc/pairing.hpp), one
 * lane per element.  An Fq12 crosses as 72 canonical words in tower order
 * (c0.c0.c0, c0.c0.c1, c0.c1.c0, ...).  out[i] = op(a[i]) or op(a[i], b[i]);
 * b is read by MUL and LINE_MUL only (else it may be NULL).  LINE_MUL takes
 * b's c0.c0, c0.c1 and c1.c1 as the three coefficients of a line (its other
 * coefficients are ignored); CYC_SQR expects a in the cyclotomic subgroup;
 * FINAL_EXP is a^(3 (p^12 - 1) / r) (the documented c = 3). */
enum { ZK_TEST_FQ12_MUL = 0, ZK_TEST_FQ12_SQR = 1, ZK_TEST_FQ12_INV = 2, ZK_TEST_FQ12_CONJ = 3,
       ZK_TEST_FQ12_FROB1 = 4, ZK_TEST_FQ12_FROB2 = 5, ZK_TEST_FQ12_CYC_SQR = 6,
       ZK_TEST_FQ12_LINE_MUL = 7, ZK_TEST_FQ12_FINAL_EXP = 8 };
int zk_test_fq12(zk_ctx *ctx, int op, const uint64_t *a, const uint64_t *b, size_t n, uint64_t *out);
/* The device's final-exponentiated e(g1[i], g2[i]) (on-the-fly Miller loop,
 * then FINAL_EXP) as n Fq12 of 72 words.  Points must be canonical and on
 * their curves; an infinite point gives 1. */
int zk_test_pairing_gt(zk_ctx *ctx, const zk_g1_affine *g1, const zk_g2_affine *g2, size_t n, uint64_t *out);
/* The three folds of zk_groth16_verify_all_sound on their own: the same
 * chunked Miller and fold path (ZK_OPT_VERIFY_CHUNK), then instead of the
 * finish sum_c = S_C = sum c_k C_k in affine form, scal = the n_inputs + 1
 * canonical scalars (s, t_0 .. t_{l-1}), and gt = FINAL_EXP of conj(F),
 * F = prod f(c_k A_k, B_k), as 72 canonical words in zk_test_fq12's layout.
 * Arguments and return codes as the product call; a malformed proof is
 * ZK_ERR_ARG here. */
int zk_test_verify_all_parts(zk_ctx *ctx, const zk_vk *vk, const zk_proof *proofs, const zk_fr *public_inputs,
                             size_t n_inputs, size_t n_proofs, const zk_fr *coeffs, zk_g1_affine *sum_c,
                             zk_fr *scal, uint64_t *gt);
/* One device field operation of csrc/ff.hpp per element, on operands exactly
 * as the device holds them: raw 32-bit little-endian limbs in the device's
 * Montgomery domain (R = 2^392 for Fq, 2^261 for Fr), with no conversion on
 * the way in or out, so a caller sets every bit.  An element is 8 words (Fr),
 * 12 (Fq) or 24 (Fq2 and Fq2h: c0 then c1); a, b, c, d and out hold n
 * elements.  Fq2 runs one lane per element; Fq2h runs the lane-pair form,
 * element i on lanes 2i (c0) and 2i + 1 (c1).  Every lane of the last wave
 * stays active (a lane past the end computes on the last element and only its
 * store is skipped).  b is read by MUL, ADD, SUB, MUL_LAZY and MUL_SUB, c and
 * d by MUL_SUB only (else they may be NULL).
 *   Fr, Fq:  MUL SQR ADD SUB NEG DBL INV TO_MONT FROM_MONT
 *            (INV = fp_inv; TO_MONT = a R, FROM_MONT = a / R)
 *   Fr only: MUL_LAZY (fp_mul<FrParams, false>: the result is below 2r and
 *            not reduced further)
 *   Fq only: MUL_SUB (fq_mul_sub: (a b - c d) / R), FQ_INV (fq_inv)
 *   Fq2:     MUL SQR INV ADD SUB NEG MUL_SUB
 *   Fq2h:    MUL SQR MUL_SUB ADD SUB NEG IS_ZERO (out: each lane's verdict,
 *            0 or 1, as word 0 of its half, the other words 0)
 * What an operation requires of its operands: ADD, SUB, NEG, DBL, INV and
 * every Fq2 / Fq2h operation (their products subtract: MUL_SUB, the c0 of a
 * product) take coefficients below the modulus; the Fr / Fq MUL, SQR,
 * MUL_LAZY, TO_MONT and FROM_MONT take any words.  Every result but
 * MUL_LAZY's is below the modulus; INV of 0 is 0.
 * ZK_ERR_ARG: a null ctx, a needed operand or out missing (n > 0), or a
 * (field, op) pair not listed.  n = 0 does nothing. */
enum { ZK_TEST_FIELD_FR = 0, ZK_TEST_FIELD_FQ = 1, ZK_TEST_FIELD_FQ2 = 2, ZK_TEST_FIELD_FQ2H = 3,
       ZK_TEST_FIELD_FQC = 4, ZK_TEST_FIELD_FQ2C = 5 };
enum { ZK_TEST_FOP_MUL = 0, ZK_TEST_FOP_SQR = 1, ZK_TEST_FOP_ADD = 2, ZK_TEST_FOP_SUB = 3, ZK_TEST_FOP_NEG = 4,
       ZK_TEST_FOP_DBL = 5, ZK_TEST_FOP_INV = 6, ZK_TEST_FOP_TO_MONT = 7, ZK_TEST_FOP_FROM_MONT = 8,
       ZK_TEST_FOP_MUL_LAZY = 9, ZK_TEST_FOP_MUL_SUB = 10, ZK_TEST_FOP_FQ_INV = 11, ZK_TEST_FOP_IS_ZERO = 12 };
int zk_test_field(zk_ctx *ctx, int field, int op, const uint32_t *a, const uint32_t *b, const uint32_t *c,
                  const uint32_t *d, size_t n, uint32_t *out);
/* One point formula of csrc/curve.hpp per element, on the same raw words.  A
 * coordinate is one field element as above; p and out are XYZZ points (X, Y,
 * ZZ, ZZZ: 48 words over Fq, 96 over Fq2), q is an XYZZ point for the adds
 * and an affine point (x, y: 24 / 48 words) for MADD and AFF_DBL.
 *   DBL xyzz_dbl(p)   DBL_CALL xyzz_dbl_call(p)   AFF_DBL aff_dbl(q)
 *   MADD xyzz_madd(p, q)   ADD xyzz_add(p, q)   ADD_ILP xyzz_add_ilp(p, q)
 *   ADD_QUAD xyzz_add_quad(p, q)   ADD_DUO xyzz_add_duo(p, q)
 * field is FQ, FQ2 (one lane per element), FQ2H (a lane pair per element),
 * or FQC / FQ2C (the call-based fields of csrc/points.hpp through the same
 * templates); all take DBL .. ADD_ILP.  ADD_QUAD runs on FQ only and ADD_DUO
 * on FQ2H only, both with four lanes per element that hold the same p and q;
 * there out holds every lane's result: 4 n points (ADD_QUAD, one per lane)
 * or 2 n points (ADD_DUO, one per lane pair), element i first.  Every lane of
 * the last wave stays active as in zk_test_field.  p is not read by AFF_DBL
 * and q not by DBL / DBL_CALL (they may be NULL).
 * Coordinates must be below p; the point at infinity is any point with
 * ZZ = 0; MADD and AFF_DBL need q not at infinity (AFF_DBL of a point with
 * y = 0 gives ZZ = 0); nothing is required to lie on the curve.
 * ZK_ERR_ARG as zk_test_field. */
enum { ZK_TEST_COP_DBL = 0, ZK_TEST_COP_DBL_CALL = 1, ZK_TEST_COP_AFF_DBL = 2, ZK_TEST_COP_MADD = 3,
       ZK_TEST_COP_ADD = 4, ZK_TEST_COP_ADD_ILP = 5, ZK_TEST_COP_ADD_QUAD = 6, ZK_TEST_COP_ADD_DUO = 7 };
int zk_test_curve(zk_ctx *ctx, int field, int op, const uint32_t *p, const uint32_t *q, size_t n, uint32_t *out);
/* zk_hash_to_g2 through the same kernel with a cap on the tries: a message
 * that needs more than max_tries (1 .. 256, else ZK_ERR_ARG) comes back as
 * tries = 0xff with zero words.  Shows the loop leaving at the cap and the
 * lanes that found a point earlier keeping it. */
int zk_test_hash_to_g2_capped(zk_ctx *ctx, const uint8_t *msgs, size_t n, size_t msg_len, const uint8_t *dst,
                              size_t dst_len, uint32_t max_tries, zk_g2_affine *out, uint8_t *tries);
/* Prepared verification keys (csrc/prepared.hpp).  The rules as pure host
 * functions, no GPU: for a key of the mode and num_public, *width = the window
 * width b the library chooses (0: no table fits the bound), *windows = W,
 * *table_bytes = the window table, *dev_bytes = what zk_vk_dev_bytes reports,
 * *bound = the table's byte bound.  With force_width in {1, 2, 4, 8} the same
 * figures for that width instead of the chosen one (0: the rule). */
int zk_test_prepared_plan(int sound, uint64_t num_public, int force_width, uint32_t *width, uint32_t *windows,
                          uint64_t *table_bytes, uint64_t *dev_bytes, uint64_t *bound);
/* *run = table additions per first-level lane of the sums for a chunk of m
 * proofs of a key with num_public inputs and `windows` windows; *fill = the
 * proof count from which a lane takes a whole proof. */
int zk_test_prepared_run(uint64_t m, uint64_t num_public, uint32_t windows, uint64_t *run, uint64_t *fill);
/* Force the window width of the keys this ctx prepares from now on (1, 2, 4,
 * 8; 0: the rule) and the run length of every sum it computes (0: the rule).
 * ZK_ERR_ARG for another width. */
int zk_test_prepared_force(zk_ctx *ctx, int width, uint32_t run);
/* The (width, windows) a prepared key holds. */
int zk_test_prepared_info(const zk_vk_dev *pvk, uint32_t *width, uint32_t *windows);
/* MSM chunking (csrc/msm.hip).  The accumulate splits the M grouped entries
 * of an MSM over T units, chunks of K = ceil(M / T) rounded up to a multiple
 * of 4 (4 when M = 0); a bucket over more than fix_max chunks goes to the merge
 * levels instead of the serial fixup.  T is by rule one full-occupancy round
 * of the chip, so small inputs only ever see K = 4.  Force both for every MSM
 * this ctx launches from now on -- its five prove workspaces and the two of
 * the first part of a host witness: T = 0 the rule, else 1 .. 2^22 units;
 * fix_max = 0 the rule (8), else >= 1.  Host values only, the kernels are the
 * shipped ones.  ZK_ERR_ARG for a T above 2^22.  A test restores (0, 0). */
int zk_test_msm_force(zk_ctx *ctx, uint32_t T, uint32_t fix_max);
/* What the last finished MSM of workspace `which` ran with: which = 0 .. 4 the
 * prove slots (pi_A, pi_B, B1, IC, H; zk_msm_* use 0; the A + B1 batch is 0,
 * IC + H is 4), 5 and 6 the G2 and the A + B1 workspace of a host witness's
 * first part.  info[ZK_TEST_MSM_*], ZK_TEST_MSM_WORDS words: the plan (C window
 * bits, NWIN, BITS, SW words per scalar, SHARED, COPIES, NRED reduction
 * windows, NSEG, SEGSHIFT, G buckets, T, FIX_MAX, N points), and read back
 * from the device M = off[G], the grouped entries (a per-window plan: the
 * non-zero digits), and NBIG = the buckets the fixup left to the merge
 * (zeroed by the grouping, counted by the fixup, not written after it).
 * NATURAL_T = the rule's T for the curve g2 (0: G1, 1: G2), whatever is
 * forced.  Waits for the ctx's streams.  ZK_ERR_ARG for a workspace no MSM
 * has run on. */
enum { ZK_TEST_MSM_C = 0, ZK_TEST_MSM_NWIN = 1, ZK_TEST_MSM_BITS = 2, ZK_TEST_MSM_SW = 3, ZK_TEST_MSM_SHARED = 4,
       ZK_TEST_MSM_COPIES = 5, ZK_TEST_MSM_NRED = 6, ZK_TEST_MSM_NSEG = 7, ZK_TEST_MSM_SEGSHIFT = 8,
       ZK_TEST_MSM_G = 9, ZK_TEST_MSM_T = 10, ZK_TEST_MSM_FIX_MAX = 11, ZK_TEST_MSM_M = 12, ZK_TEST_MSM_NBIG = 13,
       ZK_TEST_MSM_NATURAL_T = 14, ZK_TEST_MSM_N = 15, ZK_TEST_MSM_WORDS = 16 };
int zk_test_msm_info(zk_ctx *ctx, int which, int g2, uint32_t *info);
/* The grouping of that MSM (csrc/group.hip) as the accumulate read it: *G and
 * *M as above, and with cap >= max(*G + 1, *M): off_out[0 .. G] = the first
 * entry of every bucket (off[G] = M), key_out[0 .. M) = the sorted bucket of
 * every entry, ent_out[0 .. M) = its base index with the digit's sign in bit
 * 31 (0x7fffffff: the dummy entry of a zero digit in a shared plan).  cap = 0
 * only queries the sizes. */
int zk_test_msm_grouping(zk_ctx *ctx, int which, uint32_t *off_out, uint32_t *key_out, uint32_t *ent_out,
                         size_t cap, size_t *G, size_t *M);
/* Overwrite what the MSMs of this ctx left in their workspaces -- buckets,
 * chunk partials, merge slots, row/column sums and quantities of the seven
 * workspaces above -- with the byte 0xA5: no coordinate is below p and no
 * point is the identity.  An MSM writes every value it later reads, so this
 * changes no result; a test calls it before an MSM so that a bucket or a
 * partial the MSM fails to write cannot pass on the right value an earlier
 * MSM of the same inputs left there.  Waits for the ctx's streams. */
int zk_test_msm_scrub(zk_ctx *ctx);
/* The coefficient side of zk_groth16_verify_key_srs_sound on its own
 * (csrc/keycheck.hip: the split row products, then the six inverse
 * transforms): out = the six vectors m^{M,part} of that call's description as
 * 6 n canonical zk_fr, n the circuit's domain -- A pub, A priv, B pub, B priv,
 * C pub, C priv -- for rho = num_variables canonical values (any values below
 * r, not only below 2^128; else ZK_ERR_ARG) split at column num_public.
 * num_public >= num_variables is ZK_ERR_SETUP_PARAMS. */
int zk_test_key_srs_coeffs(zk_ctx *ctx, const zk_r1cs_csr *qap, uint64_t num_public, const zk_fr *rho,
                           zk_fr *out);

#ifdef __cplusplus
}
#endif
#endif /* ZKP_TEST_H */
