/*
 * zkp.h -- C ABI of the MI355X-native Groth16 prover hot path
 *          (BLS12-381; G1/G2 Pippenger MSM + radix-2 Fr NTT on gfx950).
 *
 * Drop-in boundary for vats98754/zero-knowledge-proofs (Rust, arkworks 0.4):
 * every entry point below names the reference interface it replaces.  The
 * Rust-side binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - Field elements cross the ABI in CANONICAL (non-Montgomery) form,
 *     little-endian u64 limbs: Fr = 4 limbs, Fq = 6, Fq2 = c0 then c1.
 *     (ark's in-memory BigInt layout; Montgomery conversion is internal.)
 *   - Affine points carry an explicit infinity byte, like ark's
 *     G1Affine{x, y, infinity}.  x = y = 0 when infinity is set.
 *   - All host buffers are caller-owned.  A zk_ctx owns its device memory
 *     and any uploaded proving key; calls on one ctx are serialised by the
 *     caller; distinct ctxs are independent.  No callbacks, no exceptions.
 *   - Every function returns a zk_status; zk_last_error() gives detail.
 */
#ifndef ZKP_H
#define ZKP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Error kinds map 1:1 onto the reference's error enums:
 *   GrothError::MSMError            crates/groth16-core/src/lib.rs:75-76,282-283
 *   GrothError::InvalidWitness      crates/groth16-core/src/lib.rs:63-64,83-98,113-128
 *   QAPError::PolynomialDivisionFailed crates/groth16-qap/src/lib.rs:76-77,266-268
 *   QAPError::DomainTooSmall        crates/groth16-qap/src/lib.rs:67-73,101-105
 *   SetupError::InvalidParams       crates/groth16-setup/src/lib.rs:107-108,128-152 */
typedef enum {
  ZK_OK = 0,
  ZK_ERR_MSM_LEN = 1,
  ZK_ERR_INVALID_WITNESS = 2,
  ZK_ERR_QAP_DIVISION = 3,
  ZK_ERR_DOMAIN = 4,
  ZK_ERR_SETUP_PARAMS = 5,
  ZK_ERR_DEVICE = 6,
  ZK_ERR_RCCL = 7,
  ZK_ERR_ARG = 8,          /* bad argument: NULL, out of range, non-canonical field element */
  ZK_ERR_DIMENSION = 9     /* FieldError::DimensionMismatch (crates/groth16-field/src/lib.rs:127-129),
                              as returned by QAP::evaluate_at (crates/groth16-qap/src/lib.rs:190-198) */
} zk_status;

typedef struct { uint64_t l[4]; } zk_fr;                                   /* 32 B  */
typedef struct { uint64_t x[6], y[6]; uint8_t infinity, _pad[7]; } zk_g1_affine;   /* 104 B */
typedef struct { uint64_t x[12], y[12]; uint8_t infinity, _pad[7]; } zk_g2_affine; /* 200 B */

/* Proof (crates/groth16-core/src/lib.rs:27-36) */
typedef struct { zk_g1_affine a; zk_g2_affine b; zk_g1_affine c; } zk_proof;

/* Constraint system in CSR form, rows = constraints.  Replaces the dense
 * a/b/c_evals matrices of QAP::from_r1cs (crates/groth16-qap/src/lib.rs:114-140)
 * and the per-variable polynomials of struct QAP (qap:31-46): the same
 * matrices, never materialised densely.  Columns >= num_variables are
 * ignored (qap:122-124).  *_val == NULL means every coefficient is 1. */
typedef struct {
  uint64_t num_constraints;
  uint64_t num_variables;
  const uint64_t *a_rowptr; const uint32_t *a_col; const zk_fr *a_val;
  const uint64_t *b_rowptr; const uint32_t *b_col; const zk_fr *b_val;
  const uint64_t *c_rowptr; const uint32_t *c_col; const zk_fr *c_val;
} zk_r1cs_csr;

/* SetupParams (crates/groth16-setup/src/lib.rs:82-93); tau is the field
 * the reference calls `s`. */
typedef struct { zk_fr alpha, beta, gamma, delta, tau; } zk_setup_params;

/* ProvingKey (crates/groth16-setup/src/lib.rs:27-52) minus the embedded
 * QAP, which is passed as a zk_r1cs_csr.  Arrays are caller-allocated:
 * a_g1, b_g1, b_g2: num_variables; ic_g1: num_variables - num_public - 1;
 * h_g1: qap.degree() = domain size n. */
typedef struct {
  zk_g1_affine alpha_g1, beta_g1, delta_g1;
  zk_g2_affine beta_g2, delta_g2;
  zk_g1_affine *a_g1;  uint64_t a_len;
  zk_g1_affine *b_g1;  uint64_t b_len;
  zk_g2_affine *b_g2;  uint64_t b2_len;
  zk_g1_affine *ic_g1; uint64_t ic_len;
  zk_g1_affine *h_g1;  uint64_t h_len;
  uint64_t num_public;
} zk_pk;

/* VerificationKey (crates/groth16-setup/src/lib.rs:56-69); ic_g1: num_public + 1 */
typedef struct {
  zk_g1_affine alpha_g1;
  zk_g2_affine beta_g2, gamma_g2, delta_g2;
  zk_g1_affine *ic_g1; uint64_t ic_len;
  uint64_t num_public;
} zk_vk;

typedef struct zk_ctx zk_ctx;          /* one GPU, its streams and workspaces */
typedef struct zk_pk_dev zk_pk_dev;    /* proving key resident in HBM        */

/* ---------------------------------------------------------------- ctx --- */
/* device: HIP ordinal.  NULL on failure (no GPU, HIP error). */
zk_ctx *zk_ctx_create(int device);
void zk_ctx_destroy(zk_ctx *ctx);
const char *zk_last_error(const zk_ctx *ctx);
int zk_ctx_synchronize(zk_ctx *ctx);
/* Live kernel timing: HIP events recorded on the launching stream around
 * each kernel phase (msm_sort, msm_accum_g1, msm_accum_g2, msm_merge,
 * msm_bucket_sum, ntt, quotient_eval, quotient_misc).  enable: 0 off (and
 * clear), 1 on, 2 on plus a per-launch stream timeline.  No reference
 * counterpart (measurement). */
int zk_ctx_profile(zk_ctx *ctx, int enable);
/* names: '\0'-separated phase names; per phase: total ms, launches, work
 * units (scalar-point pairs for msm_*, elements for ntt/quotient). */
int zk_ctx_profile_read(zk_ctx *ctx, char *names, size_t names_cap, double *ms,
                        uint64_t *launches, uint64_t *units, size_t max_phases,
                        size_t *nphases);
/* The timeline of zk_ctx_profile(ctx, 2): one text line per profiled launch
 * ("phase stream start_ms end_ms", times from the start of its proof) and
 * "--" after each proof.  *len = its length; with buf (cap > len) the text is
 * copied NUL-terminated and the timeline cleared. */
int zk_ctx_timeline_read(zk_ctx *ctx, char *buf, size_t cap, size_t *len);

/* Build provenance: "<git HEAD>[-dirty] src:<16 hex of sha256 over the
 * sources in zero-knowledge-proofs_amd/csrc/ *.hip and *.hpp (sorted) and
 * include/zkp.h>".  __graft_entry__.smoke() recomputes the source hash from
 * the tree it runs in and refuses a library built from other sources.  No
 * reference counterpart. */
const char *zk_build_id(void);
/* Prove stream schedule (measurement): -1 or 0 the overlapped four-stream
 * schedule (default), 3 every kernel in order on one stream (isolated kernel
 * durations).  Results never depend on it.  ZK_ERR_ARG for anything else.
 * No reference counterpart. */
int zk_ctx_set_schedule(zk_ctx *ctx, int schedule);

/* Explicit path choices of a ctx, for tests and A/B measurement.  The
 * library reads nothing from the environment; without these calls it picks
 * by size.  No value changes a result: each is covered by a bit-exact GPU
 * test.  ZK_ERR_ARG for an unknown option or value.  No reference
 * counterpart.
 *   ZK_OPT_QUOTIENT_PATH  -1 by domain size (default: small-domain below
 *                         2^23), 0 small-domain (fused iNTT/coset/NTT tile
 *                         kernel, gathered final), 1 large-domain (separate
 *                         passes, natural-order final coset iNTT)
 *   ZK_OPT_PROVE_WIN_C    0 by size (default: 16, or 22 from 2^24 constraints
 *                         per key shard), 16 or 22: digit window width of
 *                         the prove MSMs of keys uploaded / set up after the
 *                         call; governs 64-bit (reference-mode) keys only
 *   ZK_OPT_SOUND_WIN_C    0 the default (20), 16, 20 or 22: digit window width
 *                         of the 255-bit prove MSMs of sound keys
 *                         (zk_groth16_setup_sound_dev, zk_pk_upload_sound)
 *                         made after the call: ceil(255 / c) window copies
 *                         of every base; independent of ZK_OPT_PROVE_WIN_C
 *   ZK_OPT_SOUND_COPIES   0 (default): a sound key made after the call keeps
 *                         all W = ceil(255 / c) window copies of every base;
 *                         k >= 1: it keeps min(k, W) of them and its MSMs sum
 *                         window w over copy w mod k into bucket set w / k --
 *                         k / W of the base memory against ceil(W / k) bucket
 *                         reductions per MSM (zk_pk_device_bytes shows the
 *                         key's size); negative: ZK_ERR_ARG.  Independent of
 *                         ZK_OPT_SOUND_WIN_C; no effect on reference-mode keys
 *   ZK_OPT_EXCHANGE_TIMEOUT_MS  watchdog of the attached exchange (default
 *                         60000, >= 1): a distributed-quotient proof whose
 *                         peers do not answer within it fails with
 *                         ZK_ERR_RCCL and aborts the exchange
 *   ZK_OPT_DIST_QUOTIENT  -1 (default): a sharded key's quotient is
 *                         distributed whenever the ctx has an exchange of the
 *                         key's (shard, nshards) attached; 0: never -- every
 *                         rank computes the whole quotient and reads the
 *                         whole witness (the replicated alternative, for
 *                         measuring one against the other on one node)
 *   ZK_OPT_EXCHANGE_FIRST 0 (default): a distributed-quotient proof starts
 *                         its G2 and A+B1+IC MSMs with the witness, beside
 *                         the quotient and its three all-to-alls; 1: those
 *                         MSMs wait until the quotient (all-to-alls
 *                         included) is done, so the collectives never queue
 *                         behind a full-occupancy accumulate (for measuring
 *                         one order against the other on one node; no
 *                         effect without a distributed quotient or under
 *                         schedule 3, where everything runs in order)
 *   ZK_OPT_POINT_CHUNK    points per kernel launch and device buffer of the
 *                         point decompression / validation calls and of
 *                         zk_g1_mul_scalar (default 2^20, >= 1)
 *   ZK_OPT_VERIFY_CHUNK   proofs (products) per kernel launch and device
 *                         buffer of zk_groth16_verify_many /
 *                         zk_pairing_products (default 65536: one lane per
 *                         proof, a full wave on every SIMD; >= 1)
 *   ZK_OPT_GNTT_MAP       lanes of a group transform stage (zk_g1_ntt / zk_g2_ntt):
 *                         -1 or 1 (default) consecutive lanes take the
 *                         butterflies of ONE twiddle, so a wave walks one scalar
 *                         in every stage with 64 or more butterflies per
 *                         twiddle; 0 consecutive lanes take consecutive
 *                         twiddles in every stage
 *   ZK_OPT_SRS_RUN        entries of one column that one lane of the column
 *                         sums of zk_groth16_setup_srs_sound adds before a second
 *                         level sums the runs (<= 2^20; 0 the default: the power
 *                         of two at or above the square root of the longest
 *                         column, at least 32)
 * (Test hooks -- the virtual-rank prove, the bare exchange, fault injection
 * -- live in a separate library, include/zkp_test.h.) */
enum { ZK_OPT_QUOTIENT_PATH = 1, ZK_OPT_PROVE_WIN_C = 2, ZK_OPT_EXCHANGE_TIMEOUT_MS = 3,
       ZK_OPT_DIST_QUOTIENT = 5, ZK_OPT_EXCHANGE_FIRST = 6, ZK_OPT_POINT_CHUNK = 7,
       ZK_OPT_VERIFY_CHUNK = 8, ZK_OPT_SOUND_WIN_C = 9, ZK_OPT_SOUND_COPIES = 10,
       ZK_OPT_GNTT_MAP = 12, ZK_OPT_SRS_RUN = 13 };
int zk_ctx_set_option(zk_ctx *ctx, int option, int64_t value);

/* ---------------------------------------------------------------- MSM --- */
/* Sum_i scalars[i] * bases[i], normalised to affine.  Replaces
 * Prover::multi_scalar_mult_g1 -> G1Projective::msm (ark-ec 0.4.2
 * VariableBaseMSM::msm), crates/groth16-core/src/lib.rs:275-286.
 * nbases != nscalars -> ZK_ERR_MSM_LEN (ark's Err(min_len)).
 * scalar_bits: 64 when every scalar is < 2^64 (the prove path's lo64
 * scalars), else 255.  Infinity bases and zero scalars are allowed.
 * A scalar >= r (ark's Fr is always reduced) or wider than scalar_bits is
 * ZK_ERR_ARG -- checked on the host for host scalars, by a device flag for
 * the *_dev entry points. */
int zk_msm_g1(zk_ctx *ctx, const zk_g1_affine *bases, size_t nbases,
              const zk_fr *scalars, size_t nscalars, uint32_t scalar_bits,
              zk_g1_affine *out);
/* Same for G2: crates/groth16-core/src/lib.rs:289-300. */
int zk_msm_g2(zk_ctx *ctx, const zk_g2_affine *bases, size_t nbases,
              const zk_fr *scalars, size_t nscalars, uint32_t scalar_bits,
              zk_g2_affine *out);

/* Device-resident MSM (benchmarks, and callers that keep bases in HBM).
 * zk_msm_g1_upload converts bases once into the device layout; the scalars
 * pointer of zk_msm_g1_dev is DEVICE memory holding n canonical zk_fr. */
typedef struct zk_msm_bases zk_msm_bases;
int zk_msm_g1_upload(zk_ctx *ctx, const zk_g1_affine *bases, size_t n, zk_msm_bases **out);
int zk_msm_g2_upload(zk_ctx *ctx, const zk_g2_affine *bases, size_t n, zk_msm_bases **out);
/* Same, plus ceil(scalar_bits / c) window-shifted copies 2^(c w) P of every
 * base (c = 16 up to 64-bit scalars, else 20; scalar_bits = 0 -> 255):
 * later zk_msm_*_dev calls with scalars of at most scalar_bits bits sum every
 * digit window into ONE bucket set (one bucket reduction, no per-window
 * Horner).  Costs ceil(scalar_bits / c) x the base memory (points padded to
 * whole 128-byte lines) and a one-time precomputation.  No reference counterpart
 * (fixed-base preprocessing of bases reused across MSMs, as in the prover). */
int zk_msm_g1_upload_windows(zk_ctx *ctx, const zk_g1_affine *bases, size_t n, uint32_t scalar_bits,
                             zk_msm_bases **out);
int zk_msm_g2_upload_windows(zk_ctx *ctx, const zk_g2_affine *bases, size_t n, uint32_t scalar_bits,
                             zk_msm_bases **out);
/* Same, keeping only the first min(copies, W) of the W = ceil(scalar_bits / c)
 * copies (copies = 0: all W, which is zk_msm_*_upload_windows).  Later
 * zk_msm_*_dev calls sum digit window w over copy w mod copies into bucket
 * set w / copies: ceil(W / copies) bucket sets and reductions instead of one,
 * for copies x the base memory instead of W x.  The sum is the same element
 * whatever the number of copies.  No reference counterpart. */
int zk_msm_g1_upload_copies(zk_ctx *ctx, const zk_g1_affine *bases, size_t n, uint32_t scalar_bits,
                            uint32_t copies, zk_msm_bases **out);
int zk_msm_g2_upload_copies(zk_ctx *ctx, const zk_g2_affine *bases, size_t n, uint32_t scalar_bits,
                            uint32_t copies, zk_msm_bases **out);
void zk_msm_bases_free(zk_msm_bases *b);
int zk_msm_g1_dev(zk_ctx *ctx, const zk_msm_bases *bases, const void *d_scalars, size_t n,
                  uint32_t scalar_bits, zk_g1_affine *out);
int zk_msm_g2_dev(zk_ctx *ctx, const zk_msm_bases *bases, const void *d_scalars, size_t n,
                  uint32_t scalar_bits, zk_g2_affine *out);

/* ---------------------------------------------------------------- NTT --- */
/* In-place radix-2 transform over Fr of size 2^log_n, natural order in and
 * out.  Replaces Radix2EvaluationDomain::{fft, ifft, coset_fft, coset_ifft}
 * (ark-poly 0.4.2) as used at crates/groth16-qap/src/lib.rs:101,167-169,260.
 * dir: +1 forward (evaluations X_k = sum_j x_j w^jk), -1 inverse (scaled by
 * n^-1).  coset: NULL, or the shift g (forward evaluates on g*<w>; inverse
 * undoes it).  log_n <= 32 else ZK_ERR_DOMAIN (Fr 2-adicity is 32). */
int zk_ntt_fr(zk_ctx *ctx, zk_fr *data, uint32_t log_n, int dir, const zk_fr *coset);
/* Same on DEVICE memory holding canonical zk_fr. */
int zk_ntt_fr_dev(zk_ctx *ctx, void *d_data, uint32_t log_n, int dir, const zk_fr *coset);

/* -------------------------------------------------------------- setup --- */
/* CRS::generate_from_qap (crates/groth16-setup/src/lib.rs:141-268) with the
 * reference's exact semantics (low-64-bit truncation of every derived scalar,
 * h_g1 = [lo64(tau~^i / delta~)]_1 for i < n).  Fills caller-allocated pk / vk
 * arrays (sizes as documented on zk_pk / zk_vk). */
int zk_groth16_setup(zk_ctx *ctx, const zk_r1cs_csr *qap, const zk_setup_params *params,
                     uint64_t num_public, zk_pk *pk, zk_vk *vk);
/* Same, but the proving key stays in HBM (no host round trip); vk may be NULL. */
int zk_groth16_setup_dev(zk_ctx *ctx, const zk_r1cs_csr *qap, const zk_setup_params *params,
                         uint64_t num_public, zk_pk_dev **pk_out, zk_vk *vk);

/* --------------------------------------------------------- sound mode --- */
/* The reference truncates every derived scalar to its low 64 bits and leaves
 * Z(tau) out of h_g1, so its proofs verify only when every derived scalar is
 * below 2^64.  Sound mode is textbook Groth16 in the
 * reference's own arrangement of pi_C, nothing truncated: with l = num_public,
 * Z(tau) = tau^n - 1,
 *   a_g1[i] = [A_i(tau)]_1, b_g1[i] = [B_i(tau)]_1, b_g2[i] = [B_i(tau)]_2
 *   pk ic_g1[i-l-1] = [(beta A_i + alpha B_i + C_i)(tau) / delta]_1, l < i < V
 *   vk ic_g1[i]     = [(beta A_i + alpha B_i + C_i)(tau) / gamma]_1, i <= l
 *   h_g1[i] = [tau^i Z(tau) / delta]_1, i < n
 *   pi_A = alpha_1 + sum z_i a_g1[i] + r delta_1
 *   pi_B = beta_2 + sum z_i b_g2[i] + s delta_2,  B_1 = beta_1 + sum z_i b_g1[i]
 *   pi_C = sum_{i>l} z_i ic_g1[i-l-1] + sum H_i h_g1[i] + s pi_A + r B_1
 * with the whole z_i and the whole quotient coefficients H_i; array lengths,
 * struct layouts and error rules are those of the reference mode.  A key
 * carries its mode: the two never mix.
 *
 * zk_groth16_setup in sound mode.  Beyond its errors: a parameter >= r is
 * ZK_ERR_ARG, tau on the evaluation domain (tau^n = 1, so Z(tau) = 0) is
 * ZK_ERR_SETUP_PARAMS.  No reference counterpart: the reference truncates. */
int zk_groth16_setup_sound(zk_ctx *ctx, const zk_r1cs_csr *qap, const zk_setup_params *params,
                           uint64_t num_public, zk_pk *pk, zk_vk *vk);
/* zk_groth16_setup_dev in sound mode: the device key holds S window copies
 * of every base, S = W = ceil(255 / c) by default (ZK_OPT_SOUND_WIN_C; c = 20:
 * 13 copies, 128 B per G1 and 256 B per G2 point -- 1024 n S bytes for n
 * constraints of the synthetic circuit, about 14 GB at 2^20) or fewer under
 * ZK_OPT_SOUND_COPIES, which is how a key too large for the device with all
 * its copies (2^24 constraints: 224 GB) is made to fit.  A key that still
 * does not fit comes back as ZK_ERR_DEVICE with the failed allocation and
 * that option named in zk_last_error; more than 2^31 copied bases in one MSM
 * as ZK_ERR_ARG.  Never sharded.  No reference counterpart: the reference
 * truncates. */
int zk_groth16_setup_sound_dev(zk_ctx *ctx, const zk_r1cs_csr *qap, const zk_setup_params *params,
                               uint64_t num_public, zk_pk_dev **pk_out, zk_vk *vk);
/* zk_pk_upload for a key made by zk_groth16_setup_sound.  zk_groth16_prove and
 * zk_groth16_prove_dev then prove with whole scalars: the device key decides
 * the mode (a host witness is uploaded whole before the first kernel).
 * zk_groth16_prove_partial, zk_groth16_prove_partial_host and
 * zk_groth16_witness_ranges return ZK_ERR_ARG for such a key.  No reference
 * counterpart: the reference truncates. */
int zk_pk_upload_sound(zk_ctx *ctx, const zk_pk *pk, const zk_r1cs_csr *qap, zk_pk_dev **out);
/* 1 for a sound device key, 0 for a reference-mode one (or NULL).  No
 * reference counterpart. */
int zk_pk_is_sound(const zk_pk_dev *pk);
/* Device memory a key of either mode holds, in bytes: its (window copies of
 * the) bases, their variable indices and the constraint matrices.  What
 * ZK_OPT_SOUND_COPIES trades is read here.  ZK_ERR_ARG for a NULL argument.
 * No reference counterpart. */
int zk_pk_device_bytes(const zk_pk_dev *pk, uint64_t *bytes);

/* -------------------------------------------------------------- prove --- */
/* Upload a proving key + its constraint system once; it stays resident.
 * The CSR is required because the reference's ProvingKey embeds the QAP as
 * dense per-variable polynomials (pk.qap, crates/groth16-setup/src/lib.rs:51,
 * built by QAP::from_r1cs, crates/groth16-qap/src/lib.rs:143-170): a Rust
 * caller passes the R1CS it built the QAP from (its A/B/C rows, the same
 * matrices the polynomials interpolate) instead of those polynomials, which
 * are infeasible beyond ~2^12 constraints.  This is the one
 * change to the drop-in contract of prove(pk, witness, rng). */
int zk_pk_upload(zk_ctx *ctx, const zk_pk *pk, const zk_r1cs_csr *qap, zk_pk_dev **out);
void zk_pk_free(zk_pk_dev *pk);

/* Prover::prove (crates/groth16-core/src/lib.rs:139-272), bit-exact:
 * z = full assignment [1 | public | witness] (Witness::assignment), zlen its
 * length, num_public = Witness::num_public.  r and s are the two Fr::rand
 * draws of core:152-153, made explicit so proofs are reproducible.
 * Errors: ZK_ERR_INVALID_WITNESS (Witness::new / validate), ZK_ERR_QAP_DIVISION;
 * ZK_ERR_ARG when r, s or some z_i is >= r (a device flag over z). */
int zk_groth16_prove(zk_ctx *ctx, const zk_pk_dev *pk, const zk_fr *z, size_t zlen,
                     size_t num_public, const zk_fr *r, const zk_fr *s, zk_proof *out);
/* Same with z in DEVICE memory (zlen canonical zk_fr). */
int zk_groth16_prove_dev(zk_ctx *ctx, const zk_pk_dev *pk, const void *d_z, size_t zlen,
                         size_t num_public, const zk_fr *r, const zk_fr *s, zk_proof *out);

/* ---- multi-GPU: MSM sharded by base range (one process per GPU) ---- */
/* Upload only shard `shard` of `nshards` contiguous ranges of every base
 * vector (and the H bases i = shard mod nshards).  The constraint system
 * stays whole on every rank: each computes the whole quotient unless its ctx
 * is attached to an exchange of the key's (shard, nshards), in which case
 * the quotient is distributed (zk_ctx_attach_rccl below). */
int zk_pk_upload_shard(zk_ctx *ctx, const zk_pk *pk, const zk_r1cs_csr *qap,
                       uint32_t shard, uint32_t nshards, zk_pk_dev **out);
int zk_groth16_setup_dev_shard(zk_ctx *ctx, const zk_r1cs_csr *qap, const zk_setup_params *params,
                               uint64_t num_public, uint32_t shard, uint32_t nshards,
                               zk_pk_dev **pk_out);
/* Opaque per-GPU partial accumulators (Montgomery XYZZ), exchanged by ONE
 * all-gather over RCCL/xGMI and folded by zk_groth16_prove_combine. */
#define ZK_PARTIAL_BYTES 1536
typedef struct { uint8_t bytes[ZK_PARTIAL_BYTES]; } zk_prove_partial;
int zk_groth16_prove_partial(zk_ctx *ctx, const zk_pk_dev *pk_shard, const void *d_z, size_t zlen,
                             size_t num_public, const zk_fr *r, const zk_fr *s,
                             zk_prove_partial *out);
/* The witness entries a key shard reads on this ctx: *nranges half-open
 * index ranges [ranges[2k], ranges[2k+1]) of z, ascending and disjoint (at
 * most cap are written).  With a distributed quotient (an exchange of the
 * key's shape attached) that is z_0, the variables of the shard's MSM bases
 * and those its quotient rows reference, plus the variables var_owner gives
 * the shard (so every z entry is read, and checked canonical, by some rank)
 * -- 1/N of the witness plus z_0 for the synthetic circuit (3n/N + 1
 * entries), since a shard's MSM variables are those its quotient rows first
 * reference; otherwise all of [0, zlen).  No reference counterpart. */
int zk_groth16_witness_ranges(zk_ctx *ctx, const zk_pk_dev *pk_shard, uint64_t *ranges, size_t cap,
                              size_t *nranges);
/* zk_groth16_prove_partial from a HOST witness slice -- the sharded form of
 * the drop-in prove(pk, witness, rng) (crates/groth16-core/src/lib.rs:139-147),
 * each rank receiving only its part: z_slice holds z[lo..hi) of every range
 * of zk_groth16_witness_ranges, concatenated in order (slice_len entries in
 * all, else ZK_ERR_ARG -- with a distributed quotient on every rank at once,
 * through the ranks' status agreement, so no peer is left waiting in an
 * all-to-all); zlen is the length of the whole witness (the
 * Witness::validate length check, core:113-118). */
int zk_groth16_prove_partial_host(zk_ctx *ctx, const zk_pk_dev *pk_shard, const zk_fr *z_slice,
                                  size_t slice_len, size_t zlen, size_t num_public, const zk_fr *r,
                                  const zk_fr *s, zk_prove_partial *out);
int zk_groth16_prove_combine(const zk_prove_partial *parts, size_t nparts,
                             const zk_fr *r, const zk_fr *s, zk_proof *out);

/* The quotient of a sharded key, distributed: ranks attached to one RCCL
 * communicator split every transform of compute_quotient_polynomial
 * (crates/groth16-qap/src/lib.rs:225-271) four-step over xGMI -- three
 * all-to-alls per proof -- instead of each recomputing it; shard k's H
 * bases are the coefficients i = k mod nshards.  Used by
 * zk_groth16_prove_partial when the ctx's communicator matches the key's
 * (shard, nshards) and nshards is 2, 4 or 8; otherwise every rank computes
 * the whole quotient.  No reference counterpart (multi-GPU). */
int zk_rccl_unique_id(uint8_t out[128]);   /* one rank makes it, all attach with it */
/* The communicator is created non-blocking and polled under the ctx's
 * exchange watchdog (ZK_OPT_EXCHANGE_TIMEOUT_MS): a peer that never attaches
 * makes this return ZK_ERR_RCCL after the timeout instead of hanging. */
int zk_ctx_attach_rccl(zk_ctx *ctx, const uint8_t unique_id[128], int rank, int world);
/* The same distributed quotient over a host-staged exchange: each of the
 * three all-to-alls brings this rank's world chunks of chunk_bytes (chunk k
 * for rank k) to pinned host memory and calls all_to_all, which must fill
 * recv (chunk s from rank s) through the caller's transport -- e.g.
 * torch.distributed over gloo, or any network -- and return 0;
 * all_reduce_max replaces *value by its maximum over the ranks (the status
 * agreement before the first exchange).  Non-zero from either callback ->
 * ZK_ERR_RCCL.  abort (may be NULL) is called when this rank fails after
 * the ranks agreed to start, so the caller can make its peers' pending
 * transfers fail (e.g. by tearing the process group down).  Callbacks run on
 * the thread that called the prove.  No reference counterpart. */
typedef struct {
  int (*all_to_all)(void *user, const void *send, void *recv, size_t chunk_bytes);
  int (*all_reduce_max)(void *user, int32_t *value);
  void (*abort)(void *user);
  void *user;
} zk_exchange_ops;
int zk_ctx_attach_exchange(zk_ctx *ctx, const zk_exchange_ops *ops, int rank, int world);
/* Drop the ctx's exchange (RCCL: ncclCommAbort, local -- every rank is
 * expected to detach too); later proofs of sharded keys compute the whole
 * quotient on every rank.  A caller whose attach or first distributed proof
 * failed on some rank detaches everywhere and carries on replicated.  No-op
 * without an exchange.  No reference counterpart. */
int zk_ctx_detach_exchange(zk_ctx *ctx);
/* ---------------------------------------------------------------- QAP --- */
/* QAP::evaluate_at (crates/groth16-qap/src/lib.rs:190-220): out[0..2] =
 * A(point), B(point), C(point) = sum_i z_i A_i(point) etc., out[3] = Z(point)
 * = point^n - 1, from the sparse matrices (sum_j (Az)_j L_j(point) with the
 * domain's Lagrange basis -- the value the dense interpolants give).
 * zlen != num_variables -> ZK_ERR_DIMENSION (FieldError::DimensionMismatch).
 * QAP::verify_evaluation (qap:274-282) is a*b == c on these values. */
int zk_qap_evaluate_at(zk_ctx *ctx, const zk_r1cs_csr *qap, const zk_fr *point, const zk_fr *z, size_t zlen,
                       zk_fr out[4]);
/* utils::batch_evaluate (crates/groth16-qap/src/lib.rs:315-322): out[p] =
 * poly_p(point) for npolys dense polynomials in coefficient form, poly p's
 * coefficients (lowest degree first) at coeffs[offsets[p] .. offsets[p+1]). */
int zk_poly_evaluate_batch(zk_ctx *ctx, const zk_fr *coeffs, const uint64_t *offsets, size_t npolys,
                           const zk_fr *point, zk_fr *out);

/* Synthetic data for benchmarks: the witness of the groth16-cli circuit
 * n x (x*y = z) (crates/groth16-cli/src/lib.rs:57-70), z = [1, x_0, y_0,
 * x_0 y_0, ...], 3n+1 canonical zk_fr written to DEVICE memory d_z, with
 * x_j, y_j < 2^254 drawn from a counter-based splitmix64 stream of `seed`. */
int zk_synthetic_witness_dev(zk_ctx *ctx, uint64_t n, uint64_t seed, void *d_z);

/* ------------------------------------------------------ serialization --- */
/* ark-serialize CanonicalSerialize, compressed (zcash flag bits), for
 * Proof (crates/groth16-core/src/lib.rs:28): a(48) | b(96) | c(48). */
int zk_proof_serialize_compressed(const zk_proof *proof, uint8_t out[192]);
/* CanonicalDeserialize, compressed, with ark's Validate::Yes checks: the
 * compression flag, infinity without the sort flag, x < p, a point on the
 * curve with the flagged root, in the prime-order subgroup.  Anything else
 * -> ZK_ERR_ARG (ark's SerializationError). */
int zk_proof_deserialize_compressed(const uint8_t in[192], zk_proof *out);

/* ------------------------------------------------- points of a key file --- */
/* The same compressed encoding for whole arrays of points, as a proving or
 * verification key file holds them: 48 bytes per G1 and 96 per G2 point
 * (x.c1 with the flag bits, then x.c0) instead of the 104 / 200 of the affine
 * structs.  These calls replace ark CanonicalSerialize / CanonicalDeserialize
 * (compressed, Validate::Yes) on G1Affine / G2Affine.  They have no reference
 * counterpart at key level: the reference CLI writes JSON placeholders for
 * its keys (crates/groth16-cli/src/lib.rs:157-219).
 *
 * What a decompressed or validated point can be, per point: the first check
 * that fails, in the order of the proof decoder above. */
typedef enum {
  ZK_POINT_OK = 0,               /* valid (the identity included) */
  ZK_POINT_ENCODING = 1,         /* compression flag clear; or the infinity flag with the sort
                                    flag or any other x bit set (one identity encoding only) */
  ZK_POINT_NOT_CANONICAL = 2,    /* a coordinate >= p */
  ZK_POINT_NOT_ON_CURVE = 3,     /* x^3 + b has no square root / y^2 != x^3 + b */
  ZK_POINT_NOT_IN_SUBGROUP = 4   /* [r]P != O */
} zk_point_status;
/* CanonicalSerialize::serialize_compressed of n points: 48 n bytes out.  Host
 * only, no ctx; writes the encoding of whatever it is given (no validation). */
int zk_g1_compress(const zk_g1_affine *pts, size_t n, uint8_t *out);
/* Same for G2Affine: 96 n bytes out. */
int zk_g2_compress(const zk_g2_affine *pts, size_t n, uint8_t *out);
/* CanonicalDeserialize::deserialize_compressed (Validate::Yes) of n G1Affine
 * on the GPU, one lane per point: square root, flagged sign, [r]P == O.
 * status (n bytes of zk_point_status) and first_bad (the lowest failing
 * index, n when there is none) may be NULL.  ZK_OK when every point is valid;
 * ZK_ERR_ARG when any is not -- out (zeros for an invalid point), status and
 * *first_bad are still filled; ZK_ERR_DEVICE on a HIP error.  n == 0 -> ZK_OK.
 * The array crosses the GPU in chunks of ZK_OPT_POINT_CHUNK points. */
int zk_g1_decompress(zk_ctx *ctx, const uint8_t *in, size_t n, zk_g1_affine *out, uint8_t *status,
                     size_t *first_bad);
/* Same for G2Affine (Fq2 square root). */
int zk_g2_decompress(zk_ctx *ctx, const uint8_t *in, size_t n, zk_g2_affine *out, uint8_t *status,
                     size_t *first_bad);
/* The checks of Validate::Yes on n G1Affine already in affine form (what
 * G1Affine::check does after an uncompressed read): coordinates < p, on the
 * curve (else ZK_POINT_NOT_ON_CURVE), in the subgroup.  A set infinity byte is
 * the identity whatever the coordinates hold.  Returns as the decompression
 * does.  zk_pk_upload itself stays unchecked: a caller that does not trust its
 * key runs this first. */
int zk_g1_validate(zk_ctx *ctx, const zk_g1_affine *pts, size_t n, uint8_t *status, size_t *first_bad);
/* Same for G2Affine. */
int zk_g2_validate(zk_ctx *ctx, const zk_g2_affine *pts, size_t n, uint8_t *status, size_t *first_bad);

/* -------------------------------------------------------------- verify --- */
/* Host-only (no GPU): a handful of sequential pairings per call. */
/* Verifier::verify (crates/groth16-core/src/lib.rs:308-355): *valid = 1 iff
 * e(A,B) e(-alpha,beta) e(-IC,gamma) e(-C,delta) == 1 with
 * IC = ic_g1[0] + sum_i lo64(public_inputs[i]) ic_g1[i+1] (core:322-338).
 * n_inputs != vk->num_public -> ZK_ERR_INVALID_WITNESS (core:315-320).  The
 * reference's own proofs fail this check unless every derived setup scalar is
 * below 2^64 (lo64 truncation) -- mirrored, not fixed. */
int zk_groth16_verify(const zk_vk *vk, const zk_proof *proof, const zk_fr *public_inputs,
                      size_t n_inputs, int *valid);
/* The same check for a sound key: IC = ic_g1[0] + sum_i x_i ic_g1[i+1] with
 * every x_i whole.  A public input >= r is ZK_ERR_ARG (the reference mode
 * ignores the upper limbs; sound mode must not), checked after the input
 * count.  No reference counterpart: the reference truncates. */
int zk_groth16_verify_sound(const zk_vk *vk, const zk_proof *proof, const zk_fr *public_inputs,
                            size_t n_inputs, int *valid);
/* BatchVerifier::verify_batch (core:360-432) with its Fr::rand coefficients
 * made explicit (coeffs[k] for proof k, canonical): ONE pairing check on
 * sum c_k A_k, sum c_k B_k, sum c_k IC_k, sum c_k C_k -- the reference's rule
 * as written.  n_proofs == 0 -> *valid = 1. */
int zk_groth16_verify_batch(const zk_vk *vk, const zk_proof *proofs, const zk_fr *const *public_inputs,
                            const size_t *n_inputs, size_t n_proofs, const zk_fr *coeffs, int *valid);
/* prod_i e(g1[i], g2[i]) == 1 -> *result = 1 (Bls12_381::multi_pairing(..)
 * .is_zero(), core:352).  Points must be canonical and on their curves. */
int zk_pairing_product_is_one(const zk_g1_affine *g1, const zk_g2_affine *g2, size_t n, int *result);

/* ------------------------------------------------------ verify on the GPU --- */
/* What a proof (or a pairing product) of a batch call can be. */
typedef enum {
  ZK_VERIFY_REJECT = 0,      /* the pairing product is not 1 */
  ZK_VERIFY_ACCEPT = 1,      /* it is 1 */
  ZK_VERIFY_MALFORMED = 2    /* a point has a coordinate >= p or is off its curve */
} zk_verify_status;
/* n_proofs independent Verifier::verify calls (core:308-355) against one vk on
 * the GPU, one lane per proof (gfx950 pairing kernel, csrc/pairing.hip);
 * public_inputs is n_proofs x n_inputs, row k for proof k.  status[k] (a
 * zk_verify_status) is what zk_groth16_verify gives for proof k alone:
 * *valid = 1 -> ACCEPT, *valid = 0 -> REJECT, ZK_ERR_ARG for a point of the
 * proof -> MALFORMED.  Returns ZK_OK whenever every proof got a status,
 * whatever the statuses are; n_inputs != vk->num_public ->
 * ZK_ERR_INVALID_WITNESS; a malformed vk point or ic_len < n_inputs + 1 ->
 * ZK_ERR_ARG; a HIP error -> ZK_ERR_DEVICE; n_proofs == 0 -> ZK_OK.  Every
 * vk point (alpha, beta, gamma, delta and all ic_len entries of ic_g1) is
 * validated first -- slightly stricter than zk_groth16_verify, which loads
 * only the ic_g1 entries whose input is non-zero.  As in the reference and the
 * host verifier no subgroup check is made (a caller that needs one runs
 * zk_g1_validate / zk_g2_validate first); for on-curve points outside the
 * r-torsion the status is unspecified (0 or 1) and the call still returns
 * normally.  The batch crosses the GPU in chunks of ZK_OPT_VERIFY_CHUNK
 * proofs.  No reference counterpart at batch level: BatchVerifier gives one
 * bit for the whole batch. */
int zk_groth16_verify_many(zk_ctx *ctx, const zk_vk *vk, const zk_proof *proofs,
                           const zk_fr *public_inputs, size_t n_inputs, size_t n_proofs,
                           uint8_t *status);
/* zk_groth16_verify_many for a sound key: status[k] is what
 * zk_groth16_verify_sound gives for proof k alone, a public input >= r making
 * that proof MALFORMED.  No reference counterpart: the reference truncates. */
int zk_groth16_verify_many_sound(zk_ctx *ctx, const zk_vk *vk, const zk_proof *proofs,
                                 const zk_fr *public_inputs, size_t n_inputs, size_t n_proofs,
                                 uint8_t *status);
/* n proofs of 192 bytes each (a | b | c, the encoding of
 * zk_proof_serialize_compressed) -> n zk_proof, decoded on the GPU: ark
 * CanonicalDeserialize (compressed, Validate::Yes) on n Proof, what
 * zk_proof_deserialize_compressed does for one on the host.  point_status:
 * 3 n bytes of zk_point_status, entry 3k + j for point a, b, c of proof k (may
 * be NULL).  All three points of every proof are decoded and get their own
 * status (no early exit inside a proof); an invalid point's words are zero.
 * ZK_OK when every point is valid, ZK_ERR_ARG when any is not (out and
 * point_status still filled, zk_last_error names the first: proof index, which
 * point, status text), ZK_ERR_DEVICE on a HIP error, n == 0 -> ZK_OK.  The
 * subgroup test is Scott's endomorphism criterion (phi(P) = -[x^2]P on G1,
 * psi(P) = [x]P on G2), equivalent to [r]P == O for points on the curve.  The
 * batch crosses the GPU in chunks of ZK_OPT_VERIFY_CHUNK proofs. */
int zk_proofs_deserialize_compressed(zk_ctx *ctx, const uint8_t *in, size_t n, zk_proof *out,
                                     uint8_t *point_status);
/* zk_groth16_verify_many from wire bytes: proofs is n_proofs x 192 bytes, and
 * decode, curve check, subgroup check and pairing check all run on the GPU in
 * one call (the decoded proofs never visit the host).  It replaces ark
 * CanonicalDeserialize (compressed, Validate::Yes) on Proof followed by
 * Verifier::verify.  status[k]: ZK_VERIFY_MALFORMED where
 * zk_proof_deserialize_compressed refuses proof k's 192 bytes (encoding,
 * range, curve, SUBGROUP), else what zk_groth16_verify gives for the decoded
 * proof.  point_status as in zk_proofs_deserialize_compressed (may be NULL).
 * Return codes, vk validation and chunking exactly as zk_groth16_verify_many
 * (ZK_OK whatever the statuses are).  Because the decoder checks the subgroup,
 * the "unspecified status" clause of zk_groth16_verify_many does not apply
 * here: every status is fully specified. */
int zk_groth16_verify_many_bytes(zk_ctx *ctx, const zk_vk *vk, const uint8_t *proofs,
                                 const zk_fr *public_inputs, size_t n_inputs, size_t n_proofs,
                                 uint8_t *status, uint8_t *point_status);
/* The same for a sound key, as zk_groth16_verify_many_sound: else what
 * zk_groth16_verify_sound gives, a public input >= r making that proof
 * MALFORMED (its point statuses can then all be ZK_POINT_OK). */
int zk_groth16_verify_many_bytes_sound(zk_ctx *ctx, const zk_vk *vk, const uint8_t *proofs,
                                       const zk_fr *public_inputs, size_t n_inputs, size_t n_proofs,
                                       uint8_t *status, uint8_t *point_status);
/* ------------------------------------------ prepared verification keys --- */
/* A verification key prepared once and kept on the device, as arkworks'
 * PreparedVerifyingKey / prepare_inputs and bellman's prepare_verifying_key.
 * It holds what the batch calls above otherwise rebuild on the host per call
 * (the Miller value of (-alpha, beta), the line tables of gamma and delta) and
 * a window table of ic_g1[1 .. num_public]: for window width b and
 * W = ceil(255 / b) windows (sound) or ceil(64 / b) (reference mode) the
 * points [j 2^(b w)] ic_g1[k], j = 1 .. 2^b - 1, 96 bytes each.  b is 8 while
 * the table stays within 512 MiB (685 inputs of a sound key), else the widest
 * of 4, 2, 1 that does; there is no option for it.  The public-input sum of a
 * proof is then W mixed additions per input, spread over lanes, instead of a
 * 255-step (64-step) double-and-add per input inside the proof's lane.
 * The mode (sound != 0: whole public inputs, one >= r malformed; 0: lo64, the
 * reference's truncation) is fixed here, as it is for a zk_pk_dev.
 * zk_vk_prepare validates EVERY point of the key -- alpha, beta, gamma, delta
 * and all ic_len entries of ic_g1 -- as zk_g1_validate / zk_g2_validate do:
 * canonical, on its curve and IN ITS SUBGROUP, which is stricter than
 * zk_groth16_verify_many and makes every status of the prepared calls fully
 * specified.  An identity point is accepted (an identity ic_g1 entry
 * contributes nothing).  ZK_ERR_ARG for a bad point, zk_last_error naming it
 * ("verification key: ic_g1[3]: not in the prime-order subgroup"), for
 * ic_len < num_public + 1 and for a key whose table would exceed the bound at
 * b = 1 (more than 21 931 inputs of a sound key); ZK_ERR_DEVICE on a HIP
 * error.  The table is built on the GPU. */
typedef struct zk_vk_dev zk_vk_dev;   /* a prepared verification key in HBM */
int zk_vk_prepare(zk_ctx *ctx, const zk_vk *vk, int sound, zk_vk_dev **out);
void zk_vk_dev_free(zk_vk_dev *pvk);
/* Device memory the key holds: 4 (6676 + 24 (num_public + 1)) bytes of fixed
 * words and the window table. */
int zk_vk_dev_bytes(const zk_vk_dev *pvk, uint64_t *bytes);
int zk_vk_dev_is_sound(const zk_vk_dev *pvk);   /* 1 for a key prepared with sound != 0 */
/* ic[k] = ic_g1[0] + sum_i x_{k,i} ic_g1[i + 1] for n rows of n_inputs public
 * inputs (row k for proof k), exactly the sum the verify kernels form: in
 * reference mode x is lo64 of the input and lo64 = 0 contributes nothing; in
 * sound mode x is the whole input and a row with an input >= r gets ok[k] = 0
 * and all-zero words in ic[k] (else ok[k] = 1; ok may be NULL).  The identity
 * is written with its infinity byte set and zero coordinates.
 * n_inputs != the key's num_public -> ZK_ERR_INVALID_WITNESS; n == 0 -> ZK_OK.
 * The rows cross the GPU in chunks of ZK_OPT_VERIFY_CHUNK. */
int zk_groth16_prepare_inputs(zk_ctx *ctx, const zk_vk_dev *pvk, const zk_fr *public_inputs,
                              size_t n_inputs, size_t n, zk_g1_affine *ic, uint8_t *ok);
/* zk_groth16_verify_many / zk_groth16_verify_many_sound (by the key's mode)
 * with a prepared key: per chunk the sums above, then the same verify kernel
 * reading IC instead of forming it.  status[k] equals what the plain call
 * gives with the key zk_vk_prepare was given; return codes as the plain call
 * (the key's points were validated when it was prepared). */
int zk_groth16_verify_many_prepared(zk_ctx *ctx, const zk_vk_dev *pvk, const zk_proof *proofs,
                                    const zk_fr *public_inputs, size_t n_inputs, size_t n_proofs,
                                    uint8_t *status);
/* zk_groth16_verify_many_bytes / _bytes_sound with a prepared key, likewise. */
int zk_groth16_verify_many_bytes_prepared(zk_ctx *ctx, const zk_vk_dev *pvk, const uint8_t *proofs,
                                          const zk_fr *public_inputs, size_t n_inputs, size_t n_proofs,
                                          uint8_t *status, uint8_t *point_status);
/* n_products pairing products on the GPU, one lane per product: product j =
 * prod_{i<k} e(g1[jk+i], g2[jk+i]) with k = pairs_per_product; status[j] as
 * above (ACCEPT: the product is 1 -- zk_pairing_product_is_one's *result = 1;
 * MALFORMED where that call returns ZK_ERR_ARG).  An infinite point on either
 * side of a pair contributes 1. */
int zk_pairing_products(zk_ctx *ctx, const zk_g1_affine *g1, const zk_g2_affine *g2,
                        size_t pairs_per_product, size_t n_products, uint8_t *status);
/* Sound batch verification: "are all n_proofs proofs valid?" for a sound key
 * with ONE pairing check on the GPU (csrc/verify_all.hip).  With the explicit
 * coefficients c_k = coeffs[k] (as zk_groth16_verify_batch takes them),
 *   s = sum c_k, t_i = sum c_k x_{k,i} (mod r), IC* = s ic_g1[0] + sum t_i ic_g1[i+1],
 *   prod_k e(c_k A_k, B_k) e(-s alpha, beta) e(-IC*, gamma) e(-sum c_k C_k, delta) == 1.
 * *valid = 1 iff no proof is malformed and the check holds.  When every proof
 * verifies the check holds for every choice of coefficients; when exactly one
 * well-formed proof does not it fails for every choice; when several do not it
 * fails except with probability about 2^-127 over independent uniform
 * coefficients -- so draw them from a cryptographic generator, fresh per call
 * and unknown to whoever made the proofs.  Each coefficient must be non-zero
 * and below 2^128 (limbs 2 and 3 zero): else ZK_ERR_ARG, checked on the host
 * before any GPU work, zk_last_error naming the index.  *first_malformed (may
 * be NULL): the lowest index of a malformed proof, or n_proofs; any malformed
 * proof makes *valid = 0.  Malformed is what
 * zk_groth16_verify_many_bytes_sound calls MALFORMED -- range, curve,
 * SUBGROUP, a public input >= r -- because the argument above needs A, B and C
 * in the prime-order subgroup: unlike zk_groth16_verify_many this call runs
 * the endomorphism subgroup test on the affine points.  A set infinity byte is
 * the identity and is allowed; a pair with an infinite side contributes 1.
 * Returns ZK_OK whenever a verdict was reached, whatever it is;
 * n_inputs != vk->num_public -> ZK_ERR_INVALID_WITNESS; a malformed vk point or
 * ic_len < n_inputs + 1 -> ZK_ERR_ARG (as zk_groth16_verify_many); NULL coeffs
 * or valid with n_proofs > 0 -> ZK_ERR_ARG; a HIP error -> ZK_ERR_DEVICE;
 * n_proofs == 0 -> *valid = 1.  The batch crosses the GPU in chunks of
 * ZK_OPT_VERIFY_CHUNK proofs, the running accumulators staying on the device
 * between chunks.  It does not say WHICH proof is invalid: a caller that needs
 * that falls back to zk_groth16_verify_many_sound.  No reference counterpart:
 * BatchVerifier's one-bit rule is no sound batching in any mode. */
int zk_groth16_verify_all_sound(zk_ctx *ctx, const zk_vk *vk, const zk_proof *proofs,
                                const zk_fr *public_inputs, size_t n_inputs, size_t n_proofs,
                                const zk_fr *coeffs, int *valid, size_t *first_malformed);
/* The same from wire bytes: proofs is n_proofs x 192 bytes, decoded and
 * subgroup-checked by the proof decoder of zk_groth16_verify_many_bytes in the
 * same call; malformed additionally covers the encoding.  point_status: 3 n
 * bytes as in zk_proofs_deserialize_compressed (may be NULL).  The probability
 * clause above applies; no reference counterpart. */
int zk_groth16_verify_all_bytes_sound(zk_ctx *ctx, const zk_vk *vk, const uint8_t *proofs,
                                      const zk_fr *public_inputs, size_t n_inputs, size_t n_proofs,
                                      const zk_fr *coeffs, int *valid, size_t *first_malformed,
                                      uint8_t *point_status);

/* ------------------------------------------- phase-2 key contributions --- */
/* Sound keys only.  A key from zk_groth16_setup_sound is known to whoever held
 * its five parameters; the phase-2 step of a Groth16 ceremony removes that for
 * delta: each participant multiplies delta by a secret share d of their own,
 * anyone checks that the new key is the old one with only delta changed, and
 * the key is safe if a single participant forgot their share.  With
 * e = 1 / d mod r, by the sound-mode formulas above,
 *   delta_g1 <- d delta_g1, delta_g2 <- d delta_g2 (pk and vk: the same point)
 *   ic_g1[i] <- e ic_g1[i] (pk), h_g1[i] <- e h_g1[i]
 * and alpha_g1, beta_g1, beta_g2, a_g1, b_g1, b_g2, num_public, the vk's
 * gamma_g2 and the vk's ic_g1 (which is over gamma) stay: entry for entry the
 * key zk_groth16_setup_sound gives for delta d mod r in place of delta.  A
 * reference-mode key cannot be rescaled (its h_g1[i] = [lo64(tau~^i / delta~)]_1
 * is not linear in 1 / delta); the structs carry no mode flag, so the _sound
 * suffix is the caller's statement of mode, as with zk_pk_upload_sound.  No
 * reference counterpart: the reference's `ceremony` (setup:282-352) works over
 * its truncated scalars.
 *
 * out[i] = k pts[i] for n G1 points and ONE scalar, on the GPU, one lane per
 * point (csrc/ceremony.hip: a joint 128-bit walk over P and its endomorphism
 * image).  Canonical affine words out; a set infinity byte gives the identity
 * (zero coordinates, infinity byte 1), k = 0 gives n identities.  k >= r ->
 * ZK_ERR_ARG; n == 0 -> ZK_OK; out == pts (in place) is allowed.  The points
 * are ASSUMED canonical, on the curve and in the prime-order subgroup -- for
 * others the result is unspecified; a caller who does not know that runs
 * zk_g1_validate first, as for zk_pk_upload.  The array crosses the GPU in
 * chunks of ZK_OPT_POINT_CHUNK points; after ZK_ERR_DEVICE the chunks already
 * done are in out (in place: a caller who must keep the input works on a copy,
 * as zk_groth16_contribute_sound does). */
int zk_g1_mul_scalar(zk_ctx *ctx, const zk_g1_affine *pts, size_t n, const zk_fr *k,
                     zk_g1_affine *out);
/* One contribution with the share d, in place on a HOST key; vk may be NULL,
 * else its delta_g2 must be pk's (ZK_ERR_ARG) and is replaced with it.  d = 0
 * or d >= r -> ZK_ERR_ARG, checked before any GPU work.  The two delta points
 * go through the host curve code, ic_g1 and h_g1 through zk_g1_mul_scalar's
 * kernel with 1 / d.  On any error the key is exactly as it was.  Device keys
 * (zk_pk_dev) are not rescaled in place: a caller uploads the new host key
 * (zk_pk_upload_sound). */
int zk_groth16_contribute_sound(zk_ctx *ctx, zk_pk *pk, zk_vk *vk, const zk_fr *d);
/* Is (after, vk_after) a contribution on top of (before, vk_before)?  Returns
 * ZK_OK whenever a verdict was reached; *status is the first check that fails:
 *   SHAPE       array lengths or num_public differ, or n_coeffs != h_len + ic_len
 *   FIXED_PART  alpha_g1, beta_g1, beta_g2, a_g1, b_g1, b_g2 or the vk's
 *               alpha_g1, beta_g2, gamma_g2, ic_g1 differ byte for byte (struct
 *               padding excluded); or a vk's delta_g2 is not its pk's
 *   POINT       after's delta_g1, delta_g2 or an ic_g1 / h_g1 entry fails
 *               zk_g1_validate / zk_g2_validate (the subgroup matters: the
 *               pairing checks below say nothing about cofactor parts);
 *               zk_last_error names the array and the index
 *   DELTA       a new delta point is the identity, or
 *               e(delta_1', delta_2) e(-delta_1, delta_2') != 1 -- the product
 *               is 1 exactly when G1 and G2 got the same share
 *   RATIO       with S = sum rho_i h_g1[i] + sum rho_{h_len + j} ic_g1[j] over the
 *               old key and S' over the new one (two 255-bit MSMs),
 *               e(S', delta_2') e(-S, delta_2) != 1
 * rho = coeffs, as in zk_groth16_verify_all_sound: each non-zero and below
 * 2^128, else ZK_ERR_ARG (after the SHAPE check; zk_last_error names the
 * index).  An honest contribution passes for every choice; a key with a
 * rescaled entry off by a non-zero subgroup element fails except with
 * probability about 2^-127 over independent uniform coefficients -- draw them
 * from a cryptographic generator, fresh per call.  The old key is the caller's
 * own and is not validated (a malformed point of it is ZK_ERR_ARG at best).
 * What this call establishes is that the new key is a well-formed sound key
 * for some delta' related to the old delta; that the contributor KNOWS the
 * share is what a proof of knowledge (below, role ZK_POK_DELTA) adds. */
typedef enum { ZK_CONTRIB_OK = 0, ZK_CONTRIB_SHAPE, ZK_CONTRIB_FIXED_PART,
               ZK_CONTRIB_POINT, ZK_CONTRIB_DELTA, ZK_CONTRIB_RATIO } zk_contribution_status;
int zk_groth16_verify_contribution_sound(zk_ctx *ctx, const zk_pk *before, const zk_vk *vk_before,
                                         const zk_pk *after, const zk_vk *vk_after,
                                         const zk_fr *coeffs, size_t n_coeffs, int *status);

/* ---------------------------------- sound keys from a powers-of-tau string --- */
/* A contribution (above) removes the trust in delta only: the key it starts
 * from was made by zk_groth16_setup_sound, whose caller knows tau, alpha and
 * beta.  The standard remedy (Bowe, Gabizon, Miers: "Scalable multi-party
 * computation for zk-SNARK parameters in the random beacon model") builds the
 * initial phase-2 key from a phase-1 STRING of powers instead of from scalars,
 * with gamma = delta = 1; contributions then randomise delta.  No reference
 * counterpart.
 *
 * The string for domains up to N = 2^log_n; arrays caller-allocated, as zk_pk's:
 *   tau_g1[i] = [tau^i]_1, i < 2N      tau_g2[i] = [tau^i]_2, i < N
 *   alpha_tau_g1[i] = [alpha tau^i]_1  beta_tau_g1[i] = [beta tau^i]_1, i < N
 *   beta_g2 = [beta]_2
 * OUT OF SCOPE: file formats and the import of foreign transcripts (.ptau). */
typedef struct {
  uint32_t log_n;                                   /* N = 2^log_n, the largest domain served */
  zk_g1_affine *tau_g1;       uint64_t tau_g1_len;  /* 2N: [tau^i]_1                          */
  zk_g2_affine *tau_g2;       uint64_t tau_g2_len;  /* N                                      */
  zk_g1_affine *alpha_tau_g1; uint64_t alpha_len;   /* N: [alpha tau^i]_1                     */
  zk_g1_affine *beta_tau_g1;  uint64_t beta_len;    /* N                                      */
  zk_g2_affine beta_g2;
} zk_srs;
/* A string from KNOWN secrets, for tests, demos and benchmarks: WHOEVER RAN
 * THIS KNOWS tau, alpha AND beta AND CAN FORGE PROOFS for every key made from
 * the string, however many contributions follow.  A real string comes out of a
 * phase-1 ceremony.  The *_len fields of out must hold at least 2N, N, N, N
 * (else ZK_ERR_ARG) and are set to exactly that.  A zero parameter is
 * ZK_ERR_SETUP_PARAMS, one >= r ZK_ERR_ARG (as the sound setup), log_n > 31
 * ZK_ERR_DOMAIN. */
int zk_srs_generate(zk_ctx *ctx, uint32_t log_n, const zk_fr *tau, const zk_fr *alpha,
                    const zk_fr *beta, zk_srs *out);
/* The radix-2 transform of zk_ntt_fr over GROUP elements, in place on a host
 * array of 2^log_n affine points, natural order in and out: dir = +1 gives
 * X_k = sum_j w^(jk) P_j, dir = -1 the inverse with 1 / n (anything else
 * ZK_ERR_ARG); w is zk_ntt_fr's root.  log_n = 0 is the identity map;
 * log_n > 32 is ZK_ERR_DOMAIN.  The points are ASSUMED valid, as for
 * zk_g1_mul_scalar; the identity comes out as zero coordinates with infinity
 * byte 1.  The whole array is resident on the device for a transform (192 B
 * per G1 and 384 B per G2 point, twice: the passes alternate between two
 * arrays); the host array crosses PCIe in pieces of ZK_OPT_POINT_CHUNK points. */
int zk_g1_ntt(zk_ctx *ctx, zk_g1_affine *pts, uint32_t log_n, int dir);
int zk_g2_ntt(zk_ctx *ctx, zk_g2_affine *pts, uint32_t log_n, int dir);
/* The sound key of qap from a string, with gamma = delta = 1: entry for entry
 * and byte for byte what zk_groth16_setup_sound gives for (alpha, beta, 1, 1,
 * tau), without anyone handing over those scalars.  With n the circuit's domain
 * (n <= N) and L_i its Lagrange basis, [L_i(tau)]_1 = (1/n) sum_k w^(-ik) [tau^k]_1
 * is an inverse group transform of the first n powers (three in G1: of tau_g1,
 * alpha_tau_g1, beta_tau_g1; one in G2), a_g1[j] = sum_i A[i][j] [L_i]_1 a sparse
 * column sum over points (b_g1, b_g2 likewise), ic[j] = sum_i A[i][j] [beta L_i]_1
 * + B[i][j] [alpha L_i]_1 + C[i][j] [L_i]_1 (j <= num_public to the vk, the rest
 * to the pk, both undivided), h_g1[i] = tau_g1[i + n] - tau_g1[i];
 * alpha_g1 = alpha_tau_g1[0], beta_g1 = beta_tau_g1[0], beta_g2 the string's,
 * delta_g1, delta_g2, gamma_g2 the generators.  Fills host keys (lengths as
 * zk_groth16_setup_sound; vk may be NULL); the caller uploads with
 * zk_pk_upload_sound.  n > N or an array shorter than log_n states ->
 * ZK_ERR_DOMAIN; num_public >= num_variables -> ZK_ERR_SETUP_PARAMS;
 * tau_g1[n] == tau_g1[0] (tau on the domain, Z(tau) = 0) ->
 * ZK_ERR_SETUP_PARAMS with the sound setup's message.  On any error the
 * outputs are untouched.  The string is ASSUMED valid (zk_srs_verify). */
int zk_groth16_setup_srs_sound(zk_ctx *ctx, const zk_r1cs_csr *qap, const zk_srs *srs,
                               uint64_t num_public, zk_pk *pk, zk_vk *vk);
/* Is srs a well-formed string?  Returns ZK_OK whenever a verdict was reached;
 * *status is the first check that fails:
 *   SHAPE      a length is not what log_n states, or n_coeffs != 2N
 *   POINT      an entry fails zk_g1_validate / zk_g2_validate or is the identity;
 *              zk_last_error names the array and the index
 *   GENERATOR  tau_g1[0] or tau_g2[0] is not the generator
 *   POWERS_G1  e(sum rho_i tau_g1[i+1], g2) e(-sum rho_i tau_g1[i], tau_g2[1]) != 1, i < 2N - 1
 *   POWERS_G2  e(tau_g1[1], sum rho_i tau_g2[i]) e(-g1, sum rho_i tau_g2[i+1]) != 1, i < N - 1
 *   ALPHA      e(sum rho_i alpha_tau_g1[i], g2) != e(alpha_tau_g1[0], sum rho_i tau_g2[i]), i < N
 *   BETA       the same for beta_tau_g1, or e(beta_tau_g1[0], g2) != e(g1, beta_g2)
 * rho = coeffs as in zk_groth16_verify_contribution_sound: each non-zero and
 * below 2^128, else ZK_ERR_ARG (after the SHAPE check).  The sums are the public
 * 255-bit MSMs, the products the host pairing.  This establishes that the
 * arrays are consistent powers of SOME tau, alpha, beta, not where they came
 * from: the contributors' proofs of knowledge are checked by
 * zk_srs_verify_contribution_proofs (below). */
typedef enum { ZK_SRS_OK = 0, ZK_SRS_SHAPE, ZK_SRS_POINT, ZK_SRS_GENERATOR, ZK_SRS_POWERS_G1,
               ZK_SRS_POWERS_G2, ZK_SRS_ALPHA, ZK_SRS_BETA } zk_srs_status;
int zk_srs_verify(zk_ctx *ctx, const zk_srs *srs, const zk_fr *coeffs, size_t n_coeffs, int *status);

/* ------------------------------------------- prepared powers-of-tau strings --- */
/* The inverse group transforms of zk_groth16_setup_srs_sound depend on the
 * string and the domain size only, and they are nearly all of its time.  A
 * PREPARED string is their result for one n = 2^log_n, resident on the device:
 * [L_i]_1, [alpha L_i]_1, [beta L_i]_1 back to back, [L_i]_2 and
 * h[i] = tau_g1[i + n] - tau_g1[i], n * (3 * 96 + 192 + 96) bytes
 * (zk_srs_dev_bytes), beside alpha_tau_g1[0], beta_tau_g1[0] and beta_g2.
 * Prepare once, then make the key of any number of circuits of that size.  No
 * reference counterpart.
 *
 * zk_srs_prepare: log_n above the string's, or arrays shorter than the
 * string's log_n states -> ZK_ERR_DOMAIN; tau_g1[n] == tau_g1[0] ->
 * ZK_ERR_SETUP_PARAMS with the sound setup's message; a failed allocation ->
 * ZK_ERR_DEVICE.  The string is ASSUMED valid (zk_srs_verify).  On any error
 * *out is untouched.  The handle belongs to ctx's device and is read-only
 * after this call. */
typedef struct zk_srs_dev zk_srs_dev;
int  zk_srs_prepare(zk_ctx *ctx, const zk_srs *srs, uint32_t log_n, zk_srs_dev **out);
void zk_srs_dev_free(zk_srs_dev *p);
int  zk_srs_dev_log_n(const zk_srs_dev *p, uint32_t *log_n);
int  zk_srs_dev_bytes(const zk_srs_dev *p, uint64_t *bytes);
/* The prepared form on the host, n = 2^log_n entries per array
 * (caller-allocated, len >= n): l_g1[i] = [L_i(tau)]_1, alpha_l_g1, beta_l_g1
 * and l_g2 likewise, h_g1[i] = [tau^i (tau^n - 1)]_1; alpha_g1, beta_g1 and
 * beta_g2 the string's.  Export writes canonical points in pieces of
 * ZK_OPT_POINT_CHUNK and sets log_n and the three points (len < n or a NULL
 * array -> ZK_ERR_ARG).  Import checks the SHAPE only (len >= n, log_n <= 31
 * else ZK_ERR_DOMAIN, non-NULL arrays): whether the points are what they claim
 * is zk_srs_lagrange_verify's job.  Export then import gives a handle whose
 * keys are identical.  OUT OF SCOPE: a file format for either form. */
typedef struct {
  uint32_t log_n;
  zk_g1_affine *l_g1, *alpha_l_g1, *beta_l_g1, *h_g1;
  zk_g2_affine *l_g2;
  uint64_t len;                                     /* entries allocated in each array */
  zk_g1_affine alpha_g1, beta_g1;
  zk_g2_affine beta_g2;
} zk_srs_lagrange;
int zk_srs_dev_export(zk_ctx *ctx, const zk_srs_dev *p, zk_srs_lagrange *out);
int zk_srs_dev_import(zk_ctx *ctx, const zk_srs_lagrange *lag, zk_srs_dev **out);
/* Is lag the prepared form of srs at lag->log_n?  No transform of points runs:
 * with rho = coeffs (n of them) and c the inverse zk_ntt_fr transform of rho,
 * [L_i(tau)] = (1/n) sum_k w^(-ik) [tau^k] gives sum_i rho_i [L_i] =
 * sum_k c_k [tau^k], two MSMs whose results are points of one group and are
 * compared as affine words.  Returns ZK_OK whenever a verdict was reached;
 * *status is the first check that fails:
 *   SHAPE        lag->len < n, lag->log_n above the string's (or the string's
 *                arrays shorter than its log_n states), or n_coeffs != n
 *   POINT        an entry of the five arrays or one of the three points fails
 *                zk_g1_validate / zk_g2_validate or is the identity;
 *                zk_last_error names the array and the index
 *   FIXED        alpha_g1, beta_g1 or beta_g2 differ from alpha_tau_g1[0],
 *                beta_tau_g1[0], beta_g2 of the string
 *   LAGRANGE_G1  sum rho_i l_g1[i] != sum c_k tau_g1[k]
 *   ALPHA        the same over alpha_l_g1 / alpha_tau_g1
 *   BETA         the same over beta_l_g1 / beta_tau_g1
 *   LAGRANGE_G2  the same over l_g2 / tau_g2
 *   H            h_g1 is not the recomputed differences, byte for byte
 * Each coefficient is non-zero and below 2^128, else ZK_ERR_ARG (after the
 * SHAPE check).  The rho side runs as 128-bit, the c side as 255-bit public
 * MSMs.  Every point was shown to lie in the prime-order subgroup first, so a
 * wrong entry survives with probability about 2^-128 over independent uniform
 * coefficients.  The string is ASSUMED valid (zk_srs_verify). */
typedef enum { ZK_LAG_OK = 0, ZK_LAG_SHAPE, ZK_LAG_POINT, ZK_LAG_FIXED, ZK_LAG_LAGRANGE_G1, ZK_LAG_ALPHA,
               ZK_LAG_BETA, ZK_LAG_LAGRANGE_G2, ZK_LAG_H } zk_srs_lagrange_status;
int zk_srs_lagrange_verify(zk_ctx *ctx, const zk_srs *srs, const zk_srs_lagrange *lag,
                           const zk_fr *coeffs, size_t n_coeffs, int *status);
/* The key of zk_groth16_setup_srs_sound from a prepared string, byte for byte:
 * the column sums over the handle's points, the generators, h_g1 copied.  A
 * Lagrange basis belongs to one size: a circuit whose padded domain is not
 * exactly the handle's 2^log_n -> ZK_ERR_DOMAIN (zk_last_error names both).
 * Other errors as zk_groth16_setup_srs_sound; on any error the outputs are
 * untouched.  The handle is only read: any number of calls may follow. */
int zk_groth16_setup_prepared_sound(zk_ctx *ctx, const zk_r1cs_csr *qap, const zk_srs_dev *p,
                                    uint64_t num_public, zk_pk *pk, zk_vk *vk /* may be NULL */);
/* The same key straight into a device key (unsharded), without a host key:
 * what zk_pk_upload_sound makes of zk_groth16_setup_prepared_sound's pk --
 * the same zk_pk_device_bytes, the same proofs.  ZK_OPT_SOUND_WIN_C and
 * ZK_OPT_SOUND_COPIES apply as for zk_groth16_setup_sound_dev.  vk, when
 * given, is filled as above. */
int zk_groth16_setup_prepared_sound_dev(zk_ctx *ctx, const zk_r1cs_csr *qap, const zk_srs_dev *p,
                                        uint64_t num_public, zk_pk_dev **pk_out, zk_vk *vk /* may be NULL */);

/* ------------------------------------------------ a key against its string --- */
/* Is (pk, vk) the sound key of the circuit qap over the string srs, for SOME
 * delta and gamma = 1 (what zk_groth16_setup_srs_sound makes, after any number
 * of zk_groth16_contribute_sound)?  The step that joins the two phases of a
 * ceremony, without rebuilding the key: no group transform, and nothing but
 * the final key is needed.  No reference counterpart.
 *
 * With V = num_variables, l = pk->num_public, n the circuit's domain and w
 * zk_ntt_fr's root, coeffs = rho_0 .. rho_{V-1} then sigma_0 .. sigma_{n-1}
 * (n_coeffs = V + n).  rho = rho^pub + rho^priv, rho^pub keeping the entries
 * i <= l.  For M in {A, B, C} and part in {pub, priv}
 *   u^{M,part}_j = sum_i M[j][i] rho^part_i  (row j < num_constraints, else 0)
 *   m^{M,part} = iNTT_n(u^{M,part}), the coefficients of sum_i rho^part_i M_i(x)
 *   m^M = m^{M,pub} + m^{M,priv}
 *   T^part = sum_k m^{A,part}_k beta_tau_g1[k] + m^{B,part}_k alpha_tau_g1[k] + m^{C,part}_k tau_g1[k]
 * Returns ZK_OK whenever a verdict was reached; *status is the first check
 * that fails, in this order:
 *   SHAPE     a_len, b_len, b2_len != V, ic_len != V - l - 1, h_len != n,
 *             vk->ic_len != l + 1, vk->num_public != l, or n_coeffs != V + n
 *   POINT     a point or array entry of either key fails zk_g1_validate /
 *             zk_g2_validate (the identity is legal in the arrays: a variable
 *             absent from a matrix has one); zk_last_error names the array and
 *             the index.  Not optional: G1's cofactor has small factors, and a
 *             low-order component survives a random combination with
 *             noticeable probability
 *   FIXED     byte for byte (struct padding excluded): pk and vk alpha_g1 against
 *             alpha_tau_g1[0], pk beta_g1 against beta_tau_g1[0], pk and vk
 *             beta_g2 against the string's, vk gamma_g2 against the G2 generator,
 *             vk delta_g2 against pk delta_g2
 *   DELTA     a delta point is the identity, or e(delta_g1, g2) != e(g1, delta_g2)
 *   QUERY_A   sum_i rho_i a_g1[i] != sum_k m^A_k tau_g1[k]       (G1 points compared)
 *   QUERY_B1  sum_i rho_i b_g1[i] != sum_k m^B_k tau_g1[k]
 *   QUERY_B2  sum_i rho_i b_g2[i] != sum_k m^B_k tau_g2[k]       (G2)
 *   IC_VK     sum_{i<=l} rho_i vk->ic_g1[i] != T^pub             (gamma = 1)
 *   IC_PK     e(sum_{i>l} rho_i pk->ic_g1[i-l-1], delta_g2) != e(T^priv, g2)
 *   H         e(sum_i sigma_i h_g1[i], delta_g2) != e(sum_i sigma_i (tau_g1[i+n] - tau_g1[i]), g2)
 * The sums over the key are the public 255-bit MSMs; those over the string are
 * at most six device MSMs over its first n (2n) entries, uploaded once; the
 * products are the host pairing.  Each coefficient is non-zero and below 2^128,
 * else ZK_ERR_ARG (after the SHAPE check; zk_last_error names the index), as
 * in zk_groth16_verify_contribution_sound.  n > N, string arrays shorter than
 * log_n states and num_public >= num_variables give the codes of
 * zk_groth16_setup_srs_sound, before any check.
 * An honest key passes for every delta the chain has reached and every choice
 * of coefficients; a key with one entry off by a non-zero subgroup element
 * fails except with probability about 2^-127 over independent uniform
 * coefficients -- draw them from a cryptographic generator, fresh per call.
 * What this does NOT establish: that anyone knows the delta shares (the proofs
 * of knowledge below do that), and that the string itself is well formed -- it
 * is ASSUMED valid, as for zk_groth16_setup_srs_sound (zk_srs_verify). */
typedef enum { ZK_KEYSRS_OK = 0, ZK_KEYSRS_SHAPE, ZK_KEYSRS_POINT, ZK_KEYSRS_FIXED, ZK_KEYSRS_DELTA,
               ZK_KEYSRS_QUERY_A, ZK_KEYSRS_QUERY_B1, ZK_KEYSRS_QUERY_B2, ZK_KEYSRS_IC_VK,
               ZK_KEYSRS_IC_PK, ZK_KEYSRS_H } zk_key_srs_status;
int zk_groth16_verify_key_srs_sound(zk_ctx *ctx, const zk_r1cs_csr *qap, const zk_srs *srs,
                                    const zk_pk *pk, const zk_vk *vk,
                                    const zk_fr *coeffs, size_t n_coeffs, int *status);

/* ---------------------------------------------- phase-1 contributions --- */
/* zk_srs_generate's string is known to whoever ran it.  The phase-1 step of a
 * ceremony removes that: each participant multiplies tau, alpha and beta by
 * secret shares s, a, b of their own,
 *   tau_g1[i]       <- s^i   tau_g1[i]        i < 2N
 *   tau_g2[i]       <- s^i   tau_g2[i]        i < N
 *   alpha_tau_g1[i] <- a s^i alpha_tau_g1[i]  i < N
 *   beta_tau_g1[i]  <- b s^i beta_tau_g1[i]   i < N
 *   beta_g2         <- b     beta_g2
 * and the string is safe if a single participant forgot their shares.  No
 * reference counterpart.
 *
 * out[i] = k[i] pts[i] for n points and n DIFFERENT scalars, on the GPU, one
 * lane per point (csrc/mulvec.hpp: per-lane digits select an entry of a small
 * per-lane table in device memory -- G1 a joint 128-bit walk over P and its
 * endomorphism image, G2 a joint 64-bit walk over the four images [x^j] P).
 * The contract of zk_g1_mul_scalar: canonical affine words out; a set infinity
 * byte or k[i] = 0 gives the identity (zero coordinates, infinity byte 1);
 * n == 0 -> ZK_OK; out == pts (in place) is allowed; the points are ASSUMED
 * canonical, on the curve and in the prime-order subgroup; the array crosses
 * the GPU in chunks of ZK_OPT_POINT_CHUNK points on the ctx's main stream, with
 * buffers owned by the call (the tables among them: 576 B per G1 and 5760 B per
 * G2 point of a chunk).  ANY k[i] >= r -> ZK_ERR_ARG before any GPU work;
 * zk_last_error names the index. */
int zk_g1_mul_scalars(zk_ctx *ctx, const zk_g1_affine *pts, size_t n, const zk_fr *k /* n */,
                      zk_g1_affine *out);
int zk_g2_mul_scalars(zk_ctx *ctx, const zk_g2_affine *pts, size_t n, const zk_fr *k /* n */,
                      zk_g2_affine *out);
/* What a contributor publishes beside the new string: [s]_2, [a]_2, [b]_2. */
typedef struct { zk_g2_affine tau_g2, alpha_g2, beta_g2; } zk_srs_share;
/* One contribution with the shares s, a, b, in place on a HOST string; share
 * may be NULL.  A share that is zero or >= r, or an array length that is not
 * what log_n states -> ZK_ERR_ARG, checked before any GPU work; s = a = b = 1
 * is legal and leaves the string byte for byte as it was.  The four scalar
 * arrays are geometric progressions made on the device and never cross PCIe;
 * beta_g2 and the share points go through the host curve code.  On any error
 * the string is exactly as it was.  The string is ASSUMED valid
 * (zk_srs_verify). */
int zk_srs_contribute(zk_ctx *ctx, zk_srs *srs, const zk_fr *s, const zk_fr *a, const zk_fr *b,
                      zk_srs_share *share /* may be NULL */);
/* Is `after` a contribution with the published `share` on top of `before`?
 * Returns ZK_OK whenever a verdict was reached; *status is the first check
 * that fails:
 *   SHAPE   log_n or a length differs between the strings or from what log_n
 *           states, or n_coeffs != 2N
 *   SHARE   a share point fails zk_g2_validate or is the identity
 *   STRING  zk_srs_verify(after, coeffs) gives anything but ZK_SRS_OK; its
 *           verdict goes to *srs_status (ZK_SRS_OK otherwise)
 *   TAU     e(after.tau_g1[1], g2) != e(before.tau_g1[1], share.tau_g2)
 *   ALPHA   the same for alpha_tau_g1[0] and share.alpha_g2
 *   BETA    the same for beta_tau_g1[0] and share.beta_g2
 * The new string is consistent powers of some tau', alpha', beta' by STRING;
 * the three links pin them to s tau, a alpha, b beta for the published shares.
 * coeffs as zk_srs_verify's (a bad one is ZK_ERR_ARG).  `before` is the
 * caller's own and is not validated (a malformed point of it fails a link at
 * best).  That the contributor knows s, a, b is a separate check:
 * zk_srs_verify_contribution_proofs (below); a full audit runs both.  OUT OF
 * SCOPE: file formats and the import of foreign transcripts (.ptau). */
typedef enum { ZK_SRSC_OK = 0, ZK_SRSC_SHAPE, ZK_SRSC_SHARE, ZK_SRSC_STRING,
               ZK_SRSC_TAU, ZK_SRSC_ALPHA, ZK_SRSC_BETA } zk_srs_contribution_status;
int zk_srs_verify_contribution(zk_ctx *ctx, const zk_srs *before, const zk_srs *after,
                               const zk_srs_share *share, const zk_fr *coeffs, size_t n_coeffs,
                               int *status, int *srs_status);

/* ------------------------------------------------- proofs of knowledge --- */
/* The checks above establish that a new string or key is consistent for SOME
 * shares.  The security argument of Bowe, Gabizon, Miers needs each
 * contributor to prove KNOWLEDGE of their share, bound to the state they
 * started from: with R a point of G2 hashed from that state and from [s]_1,
 * the pair ([s]_1, [s] R) can only be made by someone who knows s.  No
 * reference counterpart.
 *
 * The hash to G2, ZKAMD-H2G2-V1 (this project's own construction, try and
 * increment -- NOT RFC 9380, whose SSWU map and isogeny are OUT OF SCOPE; the
 * inputs are public, so nothing here is constant-time).  With len(dst) <= 255:
 *   m0 = SHA-256("ZKAMD-H2G2-V1" | byte(len(dst)) | dst | msg)
 *   for ctr = 0 .. 255:
 *     d_j = SHA-256(m0 | byte(ctr) | byte(j)), j = 0..4
 *     x   = (int_be(d_0 | d_1) mod p) + (int_be(d_2 | d_3) mod p) u
 *     t   = x^3 + 4 (1 + u);  t == 0 or t not a square in Fq2 -> next ctr
 *     y   = the root of t whose sort flag (that of the compressed encoding:
 *           c1, or c0 when c1 == 0, above (p - 1) / 2) equals d_4[31] & 1
 *     Q   = [x^2 - x - 1] P + [x - 1] psi(P) + psi^2([2] P), P = (x, y),
 *           x = -0xd201000000010000 (Budroni-Pintore cofactor clearing,
 *           = [h_eff] P);  Q != O -> the hash is Q, tries = ctr
 *   no point after 256 tries -> an error (probability about 2^-256)
 *
 * SHA-256 of len bytes.  Host only. */
int zk_sha256(const uint8_t *msg, size_t len, uint8_t out[32]);
/* One hash on the host.  dst_len > 255 -> ZK_ERR_ARG; no point after 256
 * tries -> ZK_ERR_ARG with *tries = 0xff and out zeroed.  tries may be NULL. */
int zk_hash_to_g2_host(const uint8_t *msg, size_t msg_len, const uint8_t *dst, size_t dst_len,
                       zk_g2_affine *out, uint8_t *tries /* may be NULL */);
/* n hashes on the GPU, one lane per message (csrc/hash.hpp): msgs is n x
 * msg_len bytes, message i at msgs + i msg_len (no alignment assumed), all
 * with the one dst.  out[i]: canonical affine words; tries[i] (may be NULL):
 * the counter that gave the point, or 0xff with out[i] all zero where there
 * was none.  dst_len > 255 -> ZK_ERR_ARG; n == 0 -> ZK_OK.  The batch crosses
 * the GPU in chunks of ZK_OPT_POINT_CHUNK messages. */
int zk_hash_to_g2(zk_ctx *ctx, const uint8_t *msgs, size_t n, size_t msg_len,
                  const uint8_t *dst, size_t dst_len, zk_g2_affine *out, uint8_t *tries /* may be NULL */);

/* A proof of knowledge of s: [s]_1 and [s] R with
 *   R = H2G2(challenge | compress(s_g1) | byte(role), "ZKAMD-POK-V1")
 * (an 81-byte message; compress = zk_g1_compress's 48 bytes).  The role keeps
 * the proofs of one contribution apart; the challenge binds a proof to the
 * state the contribution started from (zk_srs_digest / zk_groth16_key_digest_sound). */
typedef struct { zk_g1_affine s_g1; zk_g2_affine s_r; } zk_pok;     /* [s]_1 and [s] R */
enum { ZK_POK_TAU = 0, ZK_POK_ALPHA = 1, ZK_POK_BETA = 2, ZK_POK_DELTA = 3 };   /* role */
/* What a proof can be: the first check that fails.
 *   POINT   s_g1 fails zk_g1_validate or s_r fails zk_g2_validate, or either is
 *           the identity
 *   REJECT  e(s_g1, R) e(-g1, s_r) != 1 (zk_srs_verify_contribution_proofs:
 *           or the link to the published share fails)
 *   HASH    no R after 256 tries */
typedef enum { ZK_POK_OK = 0, ZK_POK_POINT, ZK_POK_REJECT, ZK_POK_HASH } zk_pok_status;
/* Host only.  s = 0, s >= r or role > 3 -> ZK_ERR_ARG. */
int zk_pok_make(const zk_fr *s, uint8_t role, const uint8_t challenge[32], zk_pok *out);          /* host */
/* Host only: one proof through the host hash and the host pairing.  ZK_OK
 * whenever a verdict was reached; role > 3 -> ZK_ERR_ARG. */
int zk_pok_verify(const zk_pok *pok, uint8_t role, const uint8_t challenge[32], int *status);     /* host */
/* n proofs on the GPU, status[i] (a zk_pok_status) what zk_pok_verify gives
 * for proof i alone: point validation, the hash and the two-pair product all
 * run on the device in one call and R never visits the host (the arrangement
 * of zk_groth16_verify_many_bytes).  challenges is n x 32 bytes.  *first_bad
 * (may be NULL): the lowest index whose status is not OK, or n.  ZK_OK
 * whenever every proof got a status; a role > 3 -> ZK_ERR_ARG before any GPU
 * work (zk_last_error names the index); n == 0 -> ZK_OK.  The batch crosses
 * the GPU in chunks of ZK_OPT_VERIFY_CHUNK proofs. */
int zk_pok_verify_many(zk_ctx *ctx, const zk_pok *poks, const uint8_t *roles, const uint8_t *challenges /* n x 32 */,
                       size_t n, uint8_t *status, size_t *first_bad /* may be NULL */);
/* The challenge of a phase-1 contribution: SHA-256 over
 *   "ZKAMD-SRS-V1" (12 bytes) | be64(log_n) | be64(tau_g1_len) | be64(tau_g2_len)
 *   | be64(alpha_len) | be64(beta_len)
 *   | compress(tau_g1[0..]) | compress(tau_g2[0..]) | compress(alpha_tau_g1[0..])
 *   | compress(beta_tau_g1[0..]) | compress(beta_g2)
 * with be64 a big-endian u64 and compress the 48 / 96 bytes of zk_g1_compress /
 * zk_g2_compress per point.  Host only; the encoding is streamed through the
 * hash, never held whole. */
int zk_srs_digest(const zk_srs *srs, uint8_t out[32]);                                             /* host */
/* The challenge of a phase-2 contribution: SHA-256 over
 *   "ZKAMD-KEY-V1" (12 bytes) | be64(a_len) | be64(b_len) | be64(b2_len) | be64(ic_len)
 *   | be64(h_len) | be64(num_public) | be64(vk ic_len)
 *   | compress of the pk in zk_pk order: alpha_g1, beta_g1, delta_g1, beta_g2,
 *     delta_g2, a_g1[0..], b_g1[0..], b_g2[0..], ic_g1[0..], h_g1[0..]
 *   | compress(vk gamma_g2) | compress(vk ic_g1[0..])
 * (the vk's alpha_g1, beta_g2 and delta_g2 are the pk's).  Host only. */
int zk_groth16_key_digest_sound(const zk_pk *pk, const zk_vk *vk, uint8_t out[32]);                /* host */

/* ---------------------------------------------------------- tree digests --- */
/* The two digests above are one SHA-256 chain over every point: serial by
 * definition, on one host thread.  V2 is a second definition of the same two
 * challenges, parallel by construction: leaves of 256 points hashed
 * independently -- one GPU lane per leaf (csrc/digest.hpp) -- and one short
 * host hash over the leaf digests.  V1, its bytes and its calls stay as they
 * are; V2 is what a ceremony opts into, and ONE CEREMONY USES ONE VERSION
 * THROUGHOUT (a proof made over one version's challenge is REJECT under the
 * other's).  No reference counterpart.
 *
 * enc = zk_g1_compress / zk_g2_compress, byte for byte, including what they
 * write for an infinity byte that is non-zero but not 1 (the identity, 0xc0 and
 * zeros, whatever the coordinates hold), for junk coordinates and for
 * non-canonical words: the encoder does not validate, and neither does the
 * device.
 *
 *   LEAF = 256 points.
 *   leaf(g, P[0..m)), 1 <= m <= 256, g = 1 (G1) or 2 (G2):
 *       SHA-256( B0 | enc(P[0]) | ... | enc(P[m-1]) )
 *       B0 = 64 bytes: "ZKAMD-LEAF-V2" (13) | byte(g) | be16(m) | 48 zero bytes
 *   leaves(g, arr, n) = leaf(g, arr[256 j .. min(n, 256 j + 256))) for j = 0 .. ceil(n/256)-1,
 *                       concatenated; nothing for n = 0.
 *
 *   SRS V2 = SHA-256( "ZKAMD-SRS-V2" | the five be64 of V1 | enc(beta_g2)
 *                     | leaves(1,tau_g1) | leaves(2,tau_g2) | leaves(1,alpha_tau_g1) | leaves(1,beta_tau_g1) )
 *   KEY V2 = SHA-256( "ZKAMD-KEY-V2" | the seven be64 of V1
 *                     | enc(alpha_g1) | enc(beta_g1) | enc(delta_g1) | enc(beta_g2) | enc(delta_g2) | enc(vk gamma_g2)
 *                     | leaves(1,a_g1) | leaves(1,b_g1) | leaves(2,b_g2) | leaves(1,ic_g1) | leaves(1,h_g1) | leaves(1,vk ic_g1) )
 *
 * The 64-byte B0 puts the points on a block boundary (four G1 encodings, or
 * two G2 encodings, are then exactly three blocks) and keeps a leaf apart
 * from a top hash; the header's lengths and the order of the leaf digests fix
 * every leaf's place.  At 2^20 constraints a top hash covers under 2 MB.
 *
 * The leaf digests of n points: 32 ceil(n / 256) bytes at out.  ctx == NULL
 * selects the host twin -- the same definition in plain C++ -- so that a
 * verifier without a GPU reaches the same bytes; with a ctx EVERY array goes
 * through the GPU, whatever its length (there is no size rule), in chunks of
 * ZK_OPT_POINT_CHUNK points rounded down to a multiple of 256 (at least 256).
 * n == 0 -> ZK_OK, nothing written. */
int zk_g1_leaf_digests(zk_ctx *ctx /* NULL: host */, const zk_g1_affine *pts, size_t n, uint8_t *out);
int zk_g2_leaf_digests(zk_ctx *ctx /* NULL: host */, const zk_g2_affine *pts, size_t n, uint8_t *out);
/* The V2 challenges: zk_srs_digest's / zk_groth16_key_digest_sound's argument
 * checks (a NULL array with a non-zero length -> ZK_ERR_ARG); ctx == NULL: host. */
int zk_srs_digest_v2(zk_ctx *ctx /* NULL: host */, const zk_srs *srs, uint8_t out[32]);
int zk_groth16_key_digest_v2_sound(zk_ctx *ctx /* NULL: host */, const zk_pk *pk, const zk_vk *vk, uint8_t out[32]);

/* Phase 1: the three proofs of one zk_srs_contribute(before, s, a, b), roles
 * TAU, ALPHA, BETA, challenge zk_srs_digest(before).  Host only; the shares as
 * zk_srs_contribute takes them (zero or >= r -> ZK_ERR_ARG).  A V2 ceremony
 * needs no call of its own: zk_pok_make and zk_pok_verify_many take any
 * 32-byte challenge, so its three proofs are zk_pok_make over
 * zk_srs_digest_v2(before) with the same roles, and the check below takes
 * that digest in before_digests. */
typedef struct { zk_pok tau, alpha, beta; } zk_srs_contribution_proof;
int zk_srs_prove_contribution(const zk_srs *before, const zk_fr *s, const zk_fr *a, const zk_fr *b,
                              zk_srs_contribution_proof *out);                                     /* host */
/* The transcript check for m contributions: zk_pok_verify_many over the 3 m
 * proofs (status[3 i + j] for proof tau, alpha, beta of contribution i,
 * challenge before_digests + 32 i), and per proof the link to the published
 * share, e(s_g1, g2) e(-g1, share point) = 1, as a second two-pair product in
 * the same device pass; a failed link is REJECT.  The share points themselves
 * are validated by zk_srs_verify_contribution, which this call does not
 * replace: a full audit runs both.  ZK_OK whenever every proof got a status. */
int zk_srs_verify_contribution_proofs(zk_ctx *ctx, const uint8_t *before_digests /* m x 32 */,
                                      const zk_srs_share *shares, const zk_srs_contribution_proof *proofs,
                                      size_t m, uint8_t *status /* 3m */);

#ifdef __cplusplus
}
#endif
#endif /* ZKP_H */
