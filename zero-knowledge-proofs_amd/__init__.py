"""zero-knowledge-proofs_amd -- MI355X-native Groth16 prover hot path.

Python mirror of the reference's prover/setup interface (vats98754/
zero-knowledge-proofs, Rust) over the C ABI of include/zkp.h, which is
implemented by libzkp_amd.so (hand-written gfx950 HIP kernels).  Names,
argument meaning and error behaviour follow the reference crates:

  R1CS / LinearCombination / Variable  crates/groth16-r1cs/src/lib.rs:16-358
  QAP.from_r1cs / degree               crates/groth16-qap/src/lib.rs:95-187, 285-294
  SetupParams / CRS.generate_from_qap  crates/groth16-setup/src/lib.rs:82-278
  Witness / Prover.prove / Proof       crates/groth16-core/src/lib.rs:27-272
  Verifier / BatchVerifier             crates/groth16-core/src/lib.rs:303-432
  GrothError kinds                     crates/groth16-core/src/lib.rs:47-77

There is no CPU fallback: every compute call goes through libzkp_amd.so on a
GPU, and loading fails loudly when the library (or a GPU) is missing.
The package directory name contains hyphens; import it with
importlib.import_module("zero-knowledge-proofs_amd").
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# ZK_AMD_LIB: an alternative build of the same library (tooling: A/B runs of
# variant builds; the library itself reads no environment variables)
LIB_PATH = os.environ.get("ZK_AMD_LIB") or os.path.join(_HERE, "libzkp_amd.so")
# the GPU tests' diagnostic hooks (include/zkp_test.h), built on top of
# libzkp_amd.so; the product path never loads it
TEST_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "libzkp_amd_test.so")

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001  # Fr modulus

ZK_OK, ZK_ERR_MSM_LEN, ZK_ERR_INVALID_WITNESS, ZK_ERR_QAP_DIVISION, ZK_ERR_DOMAIN, \
    ZK_ERR_SETUP_PARAMS, ZK_ERR_DEVICE, ZK_ERR_RCCL, ZK_ERR_ARG, ZK_ERR_DIMENSION = range(10)
G1_WORDS, G2_WORDS = 13, 25
PARTIAL_BYTES = 1536

# C-ABI symbols declared in include/zkp.h (checked by tests/test_capi.py)
EXPORTS = (
    "zk_ctx_create", "zk_ctx_destroy", "zk_last_error", "zk_ctx_synchronize",
    "zk_ctx_profile", "zk_ctx_profile_read",
    "zk_msm_g1", "zk_msm_g2", "zk_msm_g1_upload", "zk_msm_g2_upload", "zk_msm_bases_free",
    "zk_msm_g1_dev", "zk_msm_g2_dev", "zk_ntt_fr", "zk_ntt_fr_dev",
    "zk_groth16_setup", "zk_groth16_setup_dev", "zk_pk_upload", "zk_pk_free",
    "zk_groth16_prove", "zk_groth16_prove_dev", "zk_pk_upload_shard",
    "zk_groth16_setup_dev_shard", "zk_groth16_prove_partial", "zk_groth16_prove_combine",
    "zk_proof_serialize_compressed", "zk_rccl_unique_id", "zk_ctx_attach_rccl",
    "zk_proof_deserialize_compressed", "zk_groth16_verify",
    "zk_groth16_verify_batch", "zk_pairing_product_is_one", "zk_msm_g1_upload_windows",
    "zk_msm_g2_upload_windows", "zk_build_id", "zk_ctx_set_schedule", "zk_qap_evaluate_at",
    "zk_poly_evaluate_batch", "zk_synthetic_witness_dev", "zk_ctx_set_option", "zk_ctx_timeline_read",
    "zk_ctx_attach_exchange", "zk_groth16_witness_ranges", "zk_groth16_prove_partial_host",
    "zk_ctx_detach_exchange",
    "zk_g1_compress", "zk_g2_compress", "zk_g1_decompress", "zk_g2_decompress",
    "zk_g1_validate", "zk_g2_validate",
    "zk_groth16_verify_many", "zk_pairing_products",
    "zk_groth16_setup_sound", "zk_groth16_setup_sound_dev", "zk_pk_upload_sound", "zk_pk_is_sound",
    "zk_groth16_verify_sound", "zk_groth16_verify_many_sound",
    "zk_msm_g1_upload_copies", "zk_msm_g2_upload_copies", "zk_pk_device_bytes",
    "zk_proofs_deserialize_compressed", "zk_groth16_verify_many_bytes", "zk_groth16_verify_many_bytes_sound",
    "zk_groth16_verify_all_sound", "zk_groth16_verify_all_bytes_sound",
    "zk_g1_mul_scalar", "zk_groth16_contribute_sound", "zk_groth16_verify_contribution_sound",
    "zk_srs_generate", "zk_g1_ntt", "zk_g2_ntt", "zk_groth16_setup_srs_sound", "zk_srs_verify",
    "zk_g1_mul_scalars", "zk_g2_mul_scalars", "zk_srs_contribute", "zk_srs_verify_contribution",
    "zk_sha256", "zk_hash_to_g2_host", "zk_hash_to_g2", "zk_pok_make", "zk_pok_verify", "zk_pok_verify_many",
    "zk_srs_digest", "zk_groth16_key_digest_sound", "zk_srs_prove_contribution",
    "zk_srs_verify_contribution_proofs",
    "zk_g1_leaf_digests", "zk_g2_leaf_digests", "zk_srs_digest_v2", "zk_groth16_key_digest_v2_sound",
    "zk_vk_prepare", "zk_vk_dev_free", "zk_vk_dev_bytes", "zk_vk_dev_is_sound", "zk_groth16_prepare_inputs",
    "zk_groth16_verify_many_prepared", "zk_groth16_verify_many_bytes_prepared",
    "zk_groth16_verify_key_srs_sound",
    "zk_srs_prepare", "zk_srs_dev_free", "zk_srs_dev_log_n", "zk_srs_dev_bytes", "zk_srs_dev_export",
    "zk_srs_dev_import", "zk_srs_lagrange_verify", "zk_groth16_setup_prepared_sound",
    "zk_groth16_setup_prepared_sound_dev",
)
# include/zkp_test.h (libzkp_amd_test.so)
TEST_EXPORTS = ("zk_test_prove_virtual_shards", "zk_test_exchange", "zk_test_fault_after_exchange",
                "zk_test_pk_bases", "zk_test_pk_info", "zk_test_pk_plan", "zk_test_fq_sqrt", "zk_test_fq2_sqrt",
                "zk_test_fq12", "zk_test_pairing_gt", "zk_test_fixed_base_g1", "zk_test_fixed_base_g2",
                "zk_test_verify_all_parts", "zk_test_g1_mul_scalar_plain",
                "zk_test_g1_mul_scalars_plain", "zk_test_g2_mul_scalars_plain", "zk_test_g1_mul_scalars_table",
                "zk_test_g2_mul_scalars_table", "zk_test_split_scalars", "zk_test_field", "zk_test_curve",
                "zk_test_gn_walk", "zk_test_hash_to_g2_capped", "zk_test_prepared_plan", "zk_test_prepared_run",
                "zk_test_prepared_force", "zk_test_prepared_info", "zk_test_msm_force", "zk_test_msm_info",
                "zk_test_msm_grouping", "zk_test_msm_scrub", "zk_test_key_srs_coeffs")
# words of zk_test_msm_info (include/zkp_test.h), and its workspaces beside the five prove slots
TEST_MSM_INFO = ("c", "nwin", "bits", "sw", "shared", "copies", "nred", "nseg", "segshift", "G", "T", "fix_max",
                 "M", "nbig", "natural_T", "n")
TEST_MSM_PART_G2, TEST_MSM_PART_ABI = 5, 6
ZK_OPT_QUOTIENT_PATH, ZK_OPT_PROVE_WIN_C, ZK_OPT_EXCHANGE_TIMEOUT_MS, ZK_OPT_DIST_QUOTIENT = 1, 2, 3, 5
ZK_OPT_EXCHANGE_FIRST = 6
ZK_OPT_POINT_CHUNK = 7
ZK_OPT_VERIFY_CHUNK = 8
ZK_OPT_SOUND_WIN_C = 9
ZK_OPT_SOUND_COPIES = 10
ZK_OPT_GNTT_MAP = 12
ZK_OPT_SRS_RUN = 13
# zk_verify_status: what a proof / pairing product of a GPU batch call can be
ZK_VERIFY_REJECT, ZK_VERIFY_ACCEPT, ZK_VERIFY_MALFORMED = range(3)
# ops of zk_test_fq12 (include/zkp_test.h); FINAL_EXP computes a^(FINAL_EXP_C (p^12 - 1) / r)
(ZK_TEST_FQ12_MUL, ZK_TEST_FQ12_SQR, ZK_TEST_FQ12_INV, ZK_TEST_FQ12_CONJ, ZK_TEST_FQ12_FROB1, ZK_TEST_FQ12_FROB2,
 ZK_TEST_FQ12_CYC_SQR, ZK_TEST_FQ12_LINE_MUL, ZK_TEST_FQ12_FINAL_EXP) = range(9)
FINAL_EXP_C = 3
# fields and ops of zk_test_field / zk_test_curve (include/zkp_test.h)
(ZK_TEST_FIELD_FR, ZK_TEST_FIELD_FQ, ZK_TEST_FIELD_FQ2, ZK_TEST_FIELD_FQ2H, ZK_TEST_FIELD_FQC,
 ZK_TEST_FIELD_FQ2C) = range(6)
(ZK_TEST_FOP_MUL, ZK_TEST_FOP_SQR, ZK_TEST_FOP_ADD, ZK_TEST_FOP_SUB, ZK_TEST_FOP_NEG, ZK_TEST_FOP_DBL,
 ZK_TEST_FOP_INV, ZK_TEST_FOP_TO_MONT, ZK_TEST_FOP_FROM_MONT, ZK_TEST_FOP_MUL_LAZY, ZK_TEST_FOP_MUL_SUB,
 ZK_TEST_FOP_FQ_INV, ZK_TEST_FOP_IS_ZERO) = range(13)
(ZK_TEST_COP_DBL, ZK_TEST_COP_DBL_CALL, ZK_TEST_COP_AFF_DBL, ZK_TEST_COP_MADD, ZK_TEST_COP_ADD,
 ZK_TEST_COP_ADD_ILP, ZK_TEST_COP_ADD_QUAD, ZK_TEST_COP_ADD_DUO) = range(8)
# 32-bit words of one element of each field as those hooks see it
TEST_FIELD_WORDS = (8, 12, 24, 24, 12, 24)
FQ12_WORDS = 72
# zk_point_status: what a decompressed / validated point can be
ZK_POINT_OK, ZK_POINT_ENCODING, ZK_POINT_NOT_CANONICAL, ZK_POINT_NOT_ON_CURVE, ZK_POINT_NOT_IN_SUBGROUP = range(5)
POINT_STATUS_TEXT = ("valid", "bad encoding flags", "coordinate not below p", "not on the curve",
                     "not in the prime-order subgroup")
G1_BYTES, G2_BYTES = 48, 96
# zk_contribution_status: the first check of CRS.verify_contribution that fails
(ZK_CONTRIB_OK, ZK_CONTRIB_SHAPE, ZK_CONTRIB_FIXED_PART, ZK_CONTRIB_POINT, ZK_CONTRIB_DELTA,
 ZK_CONTRIB_RATIO) = range(6)
# zk_srs_status: the first check of SRS.verify that fails
(ZK_SRS_OK, ZK_SRS_SHAPE, ZK_SRS_POINT, ZK_SRS_GENERATOR, ZK_SRS_POWERS_G1, ZK_SRS_POWERS_G2, ZK_SRS_ALPHA,
 ZK_SRS_BETA) = range(8)
# zk_srs_lagrange_status: the first check of LagrangeSRS.verify that fails
(ZK_LAG_OK, ZK_LAG_SHAPE, ZK_LAG_POINT, ZK_LAG_FIXED, ZK_LAG_LAGRANGE_G1, ZK_LAG_ALPHA, ZK_LAG_BETA,
 ZK_LAG_LAGRANGE_G2, ZK_LAG_H) = range(9)
# zk_key_srs_status: the first check of CRS.verify_against_srs that fails
(ZK_KEYSRS_OK, ZK_KEYSRS_SHAPE, ZK_KEYSRS_POINT, ZK_KEYSRS_FIXED, ZK_KEYSRS_DELTA, ZK_KEYSRS_QUERY_A,
 ZK_KEYSRS_QUERY_B1, ZK_KEYSRS_QUERY_B2, ZK_KEYSRS_IC_VK, ZK_KEYSRS_IC_PK, ZK_KEYSRS_H) = range(11)
# zk_srs_contribution_status: the first check of SRS.verify_contribution that fails
(ZK_SRSC_OK, ZK_SRSC_SHAPE, ZK_SRSC_SHARE, ZK_SRSC_STRING, ZK_SRSC_TAU, ZK_SRSC_ALPHA, ZK_SRSC_BETA) = range(7)
PROOF_BYTES, PROOF_WORDS = 192, 51
# proofs of knowledge (zk_pok): the role of a proof, and zk_pok_status
ZK_POK_TAU, ZK_POK_ALPHA, ZK_POK_BETA, ZK_POK_DELTA = range(4)
ZK_POK_OK, ZK_POK_POINT, ZK_POK_REJECT, ZK_POK_HASH = range(4)
POK_WORDS = G1_WORDS + G2_WORDS     # a zk_pok: s_g1 then s_r
H2_NO_POINT = 0xFF                  # the tries byte of a message the hash found no point for
POK_DST = b"ZKAMD-POK-V1"
FQ_MODULUS = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
G1_GENERATOR = (
    0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
    0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1)
CSRC = os.path.join(_HERE, "csrc")


# ------------------------------------------------------------- errors ----
class GrothError(Exception):
    """crates/groth16-core/src/lib.rs:47-77"""


class InvalidWitness(GrothError):
    pass


class MSMError(GrothError):
    pass


class QAPError(GrothError):
    """crates/groth16-qap/src/lib.rs:63-86"""


class PolynomialDivisionFailed(QAPError):
    pass


class DomainTooSmall(QAPError):
    pass


class DimensionMismatch(QAPError):
    """QAPError::FieldError(FieldError::DimensionMismatch), qap:191-198"""


class SetupError(GrothError):
    """crates/groth16-setup/src/lib.rs:95-113 (InvalidParams)"""


class DeviceError(GrothError):
    pass


class ExchangeError(DeviceError):
    """ZK_ERR_RCCL: the multi-GPU exchange (RCCL or host-staged) failed or was aborted."""


_STATUS = {ZK_ERR_MSM_LEN: MSMError, ZK_ERR_INVALID_WITNESS: InvalidWitness,
           ZK_ERR_QAP_DIVISION: PolynomialDivisionFailed, ZK_ERR_DOMAIN: DomainTooSmall,
           ZK_ERR_SETUP_PARAMS: SetupError, ZK_ERR_DEVICE: DeviceError,
           ZK_ERR_RCCL: ExchangeError, ZK_ERR_ARG: ValueError, ZK_ERR_DIMENSION: DimensionMismatch}


# ---------------------------------------------------------- C structs ----
_A2A_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)
_AMAX_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)
_ABORT_FN = C.CFUNCTYPE(None, C.c_void_p)


class _ExchangeOps(C.Structure):
    _fields_ = [("all_to_all", _A2A_FN), ("all_reduce_max", _AMAX_FN), ("abort", _ABORT_FN), ("user", C.c_void_p)]


class _Fr(C.Structure):
    _fields_ = [("l", C.c_uint64 * 4)]


class _G1(C.Structure):
    _fields_ = [("w", C.c_uint64 * G1_WORDS)]


class _G2(C.Structure):
    _fields_ = [("w", C.c_uint64 * G2_WORDS)]


class _Proof(C.Structure):
    _fields_ = [("a", _G1), ("b", _G2), ("c", _G1)]


class _CSR(C.Structure):
    _fields_ = [("num_constraints", C.c_uint64), ("num_variables", C.c_uint64)] + [
        (f"{m}_{f}", C.c_void_p) for m in "abc" for f in ("rowptr", "col", "val")]


class _SetupParams(C.Structure):
    _fields_ = [(k, _Fr) for k in ("alpha", "beta", "gamma", "delta", "tau")]


class _PK(C.Structure):
    _fields_ = [("alpha_g1", _G1), ("beta_g1", _G1), ("delta_g1", _G1),
                ("beta_g2", _G2), ("delta_g2", _G2),
                ("a_g1", C.c_void_p), ("a_len", C.c_uint64),
                ("b_g1", C.c_void_p), ("b_len", C.c_uint64),
                ("b_g2", C.c_void_p), ("b2_len", C.c_uint64),
                ("ic_g1", C.c_void_p), ("ic_len", C.c_uint64),
                ("h_g1", C.c_void_p), ("h_len", C.c_uint64),
                ("num_public", C.c_uint64)]


class _VK(C.Structure):
    _fields_ = [("alpha_g1", _G1), ("beta_g2", _G2), ("gamma_g2", _G2), ("delta_g2", _G2),
                ("ic_g1", C.c_void_p), ("ic_len", C.c_uint64), ("num_public", C.c_uint64)]


class _SRS(C.Structure):
    _fields_ = [("log_n", C.c_uint32),
                ("tau_g1", C.c_void_p), ("tau_g1_len", C.c_uint64),
                ("tau_g2", C.c_void_p), ("tau_g2_len", C.c_uint64),
                ("alpha_tau_g1", C.c_void_p), ("alpha_len", C.c_uint64),
                ("beta_tau_g1", C.c_void_p), ("beta_len", C.c_uint64),
                ("beta_g2", _G2)]


class _SRSLagrange(C.Structure):
    _fields_ = [("log_n", C.c_uint32),
                ("l_g1", C.c_void_p), ("alpha_l_g1", C.c_void_p), ("beta_l_g1", C.c_void_p), ("h_g1", C.c_void_p),
                ("l_g2", C.c_void_p), ("len", C.c_uint64),
                ("alpha_g1", _G1), ("beta_g1", _G1), ("beta_g2", _G2)]


class _SRSShare(C.Structure):
    _fields_ = [("tau_g2", _G2), ("alpha_g2", _G2), ("beta_g2", _G2)]


class _Pok(C.Structure):
    _fields_ = [("s_g1", _G1), ("s_r", _G2)]


class _SRSProof(C.Structure):
    _fields_ = [("tau", _Pok), ("alpha", _Pok), ("beta", _Pok)]


_lib = None


def lib():
    """Load libzkp_amd.so (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not built: run `make -C zero-knowledge-proofs_amd/csrc`")
        # One HIP runtime per process: torch bundles its own libamdhip64
        # (SONAME libamdhip64.so.7).  Loading torch first makes our DT_NEEDED
        # bind to that copy, so torch device memory, streams and RCCL
        # (torch.distributed) share the runtime with our kernels.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.zk_ctx_create.restype = C.c_void_p
        L.zk_ctx_create.argtypes = [C.c_int]
        L.zk_ctx_destroy.argtypes = [C.c_void_p]
        L.zk_last_error.restype = C.c_char_p
        L.zk_last_error.argtypes = [C.c_void_p]
        L.zk_build_id.restype = C.c_char_p
        for name in EXPORTS:
            # an A/B build of an older revision (ZK_AMD_LIB, tooling only) may
            # lack entry points added since; the product library must have all
            f = getattr(L, name, None)
            if f is None:
                if os.environ.get("ZK_AMD_LIB"):
                    continue
                raise ImportError(f"{LIB_PATH} does not export {name}")
            if name not in ("zk_ctx_create", "zk_ctx_destroy", "zk_last_error",
                            "zk_msm_bases_free", "zk_pk_free", "zk_build_id", "zk_vk_dev_free",
                            "zk_srs_dev_free"):
                f.restype = C.c_int
        L.zk_msm_bases_free.argtypes = [C.c_void_p]
        L.zk_pk_free.argtypes = [C.c_void_p]
        if hasattr(L, "zk_vk_dev_free"):
            L.zk_vk_dev_free.restype = None
            L.zk_vk_dev_free.argtypes = [C.c_void_p]
        if hasattr(L, "zk_srs_dev_free"):
            L.zk_srs_dev_free.restype = None
            L.zk_srs_dev_free.argtypes = [C.c_void_p]
        _lib = L
    return _lib


_test_lib = None


def test_lib():
    """Load libzkp_amd_test.so (include/zkp_test.h: virtual ranks, the bare
    exchange, fault injection) on top of libzkp_amd.so -- tests only."""
    global _test_lib
    if _test_lib is None:
        lib()
        if not os.path.exists(TEST_LIB_PATH):
            raise ImportError(f"{TEST_LIB_PATH} not built: run `make -C zero-knowledge-proofs_amd/csrc`")
        T = C.CDLL(TEST_LIB_PATH)
        for name in TEST_EXPORTS:
            getattr(T, name).restype = C.c_int
        _test_lib = T
    return _test_lib


def _p(a):
    return C.c_void_p(a.ctypes.data)


def build_id():
    """zk_build_id(): '<git HEAD>[-dirty] src:<source hash>' of the loaded library."""
    return lib().zk_build_id().decode()


def source_hash():
    """sha256 (16 hex) over csrc/*.hip and *.hpp (sorted) + include/zkp.h of THIS
    tree -- what the Makefile embeds in zk_build_id()."""
    import hashlib
    names = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp")))
    h = hashlib.sha256()
    for f in names:
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(fh.read())
    for hdr in ("zkp.h", "zkp_test.h"):
        with open(os.path.join(os.path.dirname(_HERE), "include", hdr), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def check_build():
    """Raise unless the loaded libzkp_amd.so was built from this tree's sources."""
    bid = build_id()
    want = source_hash()
    if not bid.endswith("src:" + want):
        raise ImportError(f"libzkp_amd.so build id {bid!r} does not match the sources (src:{want}); rebuild it")
    return bid


def _check(rc, ctx=None, what=""):
    if rc == ZK_OK:
        return
    detail = ""
    if ctx is not None:
        msg = lib().zk_last_error(ctx._h)
        detail = msg.decode() if msg else ""
    raise _STATUS.get(rc, GrothError)(f"{what} failed ({rc}) {detail}".strip())


# ------------------------------------------------------------ helpers ----
def to_limbs(v, k=4):
    v = int(v)
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(k)]


def from_limbs(a):
    return sum(int(x) << (64 * i) for i, x in enumerate(np.asarray(a).reshape(-1)))


def fr_array(values):
    """ints (reduced mod r) -> (n, 4) uint64 canonical limbs."""
    values = [int(v) % R for v in values]
    out = np.zeros((len(values), 4), dtype=np.uint64)
    for i, v in enumerate(values):
        out[i] = to_limbs(v)
    return out


def _fr(v):
    f = _Fr()
    for i, x in enumerate(to_limbs(int(v) % R)):
        f.l[i] = x
    return f


# ------------------------------------------------------------ context ----
class Context:
    """One GPU (zk_ctx): streams, cached NTT domains, MSM workspaces."""

    def __init__(self, device=0):
        self._h = lib().zk_ctx_create(int(device))
        if not self._h:
            raise DeviceError(f"zk_ctx_create({device}) failed: no usable GPU")
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            lib().zk_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- RCCL communicator for the distributed quotient of sharded keys ----
    @staticmethod
    def rccl_unique_id():
        buf = (C.c_uint8 * 128)()
        _check(lib().zk_rccl_unique_id(buf), None, "zk_rccl_unique_id")
        return bytes(buf)

    def attach_rccl(self, unique_id, rank, world):
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        _check(lib().zk_ctx_attach_rccl(C.c_void_p(self._h), buf, C.c_int(rank), C.c_int(world)), self,
               "zk_ctx_attach_rccl")

    def detach_exchange(self):
        """zk_ctx_detach_exchange: drop the attached exchange (RCCL: a local
        ncclCommAbort); sharded keys then compute the whole quotient on every
        rank.  Every rank of the job detaches together."""
        _check(lib().zk_ctx_detach_exchange(C.c_void_p(self._h)), self, "zk_ctx_detach_exchange")
        self._exchange_refs = None

    def test_exchange(self, chunk_bytes, status):
        """zk_test_exchange: one all-to-all and one status agreement on the
        attached exchange (RCCL or host-staged); returns the agreed max,
        raises ExchangeError when a received chunk is wrong."""
        out = C.c_int32()
        _check(test_lib().zk_test_exchange(C.c_void_p(self._h), C.c_size_t(chunk_bytes), C.c_int32(status),
                                           C.byref(out)), self, "zk_test_exchange")
        return out.value

    def test_fault_after_exchange(self, k):
        """zk_test_fault_after_exchange: the next distributed-quotient proof
        on this ctx fails right after its k-th all-to-all (tests only)."""
        _check(test_lib().zk_test_fault_after_exchange(C.c_void_p(self._h), C.c_int(int(k))), self,
               "zk_test_fault_after_exchange")

    def attach_exchange(self, exchange, rank, world):
        """zk_ctx_attach_exchange: the distributed quotient of sharded keys
        over a host-staged transport.  `exchange` has all_to_all(send_ptr,
        recv_ptr, chunk_bytes), all_reduce_max(int) -> int and abort()
        (e.g. TorchExchange over a gloo process group)."""
        def a2a(_u, send, recv, chunk):
            try:
                exchange.all_to_all(send, recv, chunk)
                return 0
            except Exception:
                return 1

        def amax(_u, pv):
            try:
                p = C.cast(pv, C.POINTER(C.c_int32))
                p[0] = int(exchange.all_reduce_max(int(p[0])))
                return 0
            except Exception:
                return 1

        def abort(_u):
            try:
                exchange.abort()
            except Exception:
                pass
        ops = _ExchangeOps(_A2A_FN(a2a), _AMAX_FN(amax), _ABORT_FN(abort), None)
        self._exchange_refs = (ops, exchange)   # the callbacks must outlive the attachment
        _check(lib().zk_ctx_attach_exchange(C.c_void_p(self._h), C.byref(ops), C.c_int(rank), C.c_int(world)), self,
               "zk_ctx_attach_exchange")

    def last_error(self):
        """zk_last_error: the detail text of the ctx's last failed call (or
        of a verdict that names a point, as CRS.verify_contribution's POINT)."""
        msg = lib().zk_last_error(self._h)
        return msg.decode() if msg else ""

    def set_schedule(self, schedule=-1):
        """zk_ctx_set_schedule: -1 / 0 overlapped streams (default), 3 every
        prove kernel in order on one stream (isolated kernel durations)."""
        _check(lib().zk_ctx_set_schedule(C.c_void_p(self._h), C.c_int(int(schedule))), self, "zk_ctx_set_schedule")

    def set_option(self, option, value):
        """zk_ctx_set_option: ZK_OPT_QUOTIENT_PATH (-1 by size, 0 small-domain,
        1 large-domain), ZK_OPT_PROVE_WIN_C (0 by size, 16, 22; keys made
        afterwards), ZK_OPT_SOUND_WIN_C (0 the default, 16, 20, 22; sound
        keys made afterwards), ZK_OPT_SOUND_COPIES (0 every window copy, k >= 1
        at most k copies of every base; sound keys made afterwards),
        ZK_OPT_EXCHANGE_TIMEOUT_MS (>= 1), ZK_OPT_DIST_QUOTIENT
        (-1 distributed when an exchange of the key's shape is attached, 0
        replicated), ZK_OPT_EXCHANGE_FIRST (0 MSMs start with the witness, 1
        they wait for the distributed quotient), ZK_OPT_POINT_CHUNK (points
        per launch of the decompress / validate / g1_mul_scalar calls, >= 1) or
        ZK_OPT_VERIFY_CHUNK (proofs / products per launch of verify_many /
        pairing_products, default 65536, >= 1).  Explicit path choices for
        tests and A/B runs."""
        _check(lib().zk_ctx_set_option(C.c_void_p(self._h), C.c_int(int(option)), C.c_int64(int(value))), self,
               "zk_ctx_set_option")

    def timeline_read(self):
        """The per-launch stream timeline recorded under profile(2), as text."""
        n = C.c_size_t()
        _check(lib().zk_ctx_timeline_read(C.c_void_p(self._h), None, C.c_size_t(0), C.byref(n)), self, "timeline")
        buf = C.create_string_buffer(n.value + 1)
        _check(lib().zk_ctx_timeline_read(C.c_void_p(self._h), buf, C.c_size_t(n.value + 1), C.byref(n)), self,
               "timeline")
        return buf.value.decode()

    def synthetic_witness(self, n, seed):
        """The groth16-cli circuit's witness z (3n+1 canonical Fr) generated
        on this GPU -> torch int64 tensor (3n+1, 4) on its device."""
        import torch
        z = torch.empty((3 * n + 1, 4), dtype=torch.int64, device=f"cuda:{self.device}")
        _check(lib().zk_synthetic_witness_dev(C.c_void_p(self._h), C.c_uint64(n), C.c_uint64(seed),
                                              C.c_void_p(z.data_ptr())), self, "zk_synthetic_witness_dev")
        return z

    # ---- live kernel timing (HIP events on the launching stream) ----
    def profile(self, enable=True):
        """0/False off, 1/True per-phase kernel times, 2 also the stream timeline."""
        _check(lib().zk_ctx_profile(C.c_void_p(self._h), C.c_int(int(enable))), self, "zk_ctx_profile")

    def profile_read(self):
        """{phase: {"ms": total device ms, "launches": n, "units": work units}}"""
        cap, k = 4096, 64
        names = C.create_string_buffer(cap)
        ms = (C.c_double * k)()
        la = (C.c_uint64 * k)()
        un = (C.c_uint64 * k)()
        n = C.c_size_t()
        _check(lib().zk_ctx_profile_read(C.c_void_p(self._h), names, C.c_size_t(cap), ms, la, un,
                                         C.c_size_t(k), C.byref(n)), self, "zk_ctx_profile_read")
        keys = names.raw.split(b"\0")[:n.value]
        return {kk.decode(): {"ms": ms[i], "launches": la[i], "units": un[i]} for i, kk in enumerate(keys)}

    # ---- MSM (crates/groth16-core/src/lib.rs:275-300) ----
    def msm_g1(self, bases, scalars, scalar_bits=255):
        """bases: (n, 13) uint64 canonical affine; scalars: (n, 4) uint64 canonical Fr."""
        bases = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, G1_WORDS)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros(G1_WORDS, dtype=np.uint64)
        rc = lib().zk_msm_g1(C.c_void_p(self._h), _p(bases), C.c_size_t(len(bases)), _p(scalars),
                             C.c_size_t(len(scalars)), C.c_uint32(scalar_bits), _p(out))
        _check(rc, self, "zk_msm_g1")
        return out

    def msm_g2(self, bases, scalars, scalar_bits=255):
        bases = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, G2_WORDS)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros(G2_WORDS, dtype=np.uint64)
        rc = lib().zk_msm_g2(C.c_void_p(self._h), _p(bases), C.c_size_t(len(bases)), _p(scalars),
                             C.c_size_t(len(scalars)), C.c_uint32(scalar_bits), _p(out))
        _check(rc, self, "zk_msm_g2")
        return out

    def msm_upload(self, bases, g2=False, scalar_bits=255, copies=None):
        """Bases kept in HBM for repeated MSMs -> MsmBases.  copies=None: the
        bases alone (zk_msm_*_upload); otherwise zk_msm_*_upload_copies with
        window-shifted copies for scalars of at most scalar_bits bits: 0 all
        W = ceil(scalar_bits / c) of them (one bucket set), k >= 1 min(k, W)
        (ceil(W / k) bucket sets).  bases: (n, 13 | 25) uint64 canonical affine."""
        words = G2_WORDS if g2 else G1_WORDS
        bases = np.ascontiguousarray(bases, dtype=np.uint64).reshape(-1, words)
        h = C.c_void_p()
        grp = "g2" if g2 else "g1"
        if copies is None:
            rc = getattr(lib(), f"zk_msm_{grp}_upload")(C.c_void_p(self._h), _p(bases), C.c_size_t(len(bases)),
                                                        C.byref(h))
        else:
            rc = getattr(lib(), f"zk_msm_{grp}_upload_copies")(
                C.c_void_p(self._h), _p(bases), C.c_size_t(len(bases)), C.c_uint32(int(scalar_bits)),
                C.c_uint32(int(copies)), C.byref(h))
        _check(rc, self, f"zk_msm_{grp}_upload")
        return MsmBases(self, h.value, len(bases), g2)

    # ---- points of a key file (ark CanonicalDeserialize, Validate::Yes) ----
    def _decompress(self, name, data, enc, words):
        if isinstance(data, np.ndarray):
            buf = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        else:
            buf = np.frombuffer(data, dtype=np.uint8)
        if len(buf) % enc:
            raise ValueError(f"{name}: {len(buf)} bytes is not a whole number of {enc}-byte points")
        n = len(buf) // enc
        out = np.zeros((n, words), dtype=np.uint64)
        st = np.zeros(n, dtype=np.uint8)
        if n:
            rc = getattr(lib(), name)(C.c_void_p(self._h), _p(buf), C.c_size_t(n), _p(out), _p(st), None)
            if not (rc == ZK_ERR_ARG and st.any()):   # invalid points are reported by their status
                _check(rc, self, name)
        return out, st

    def g1_decompress(self, data):
        """zk_g1_decompress: 48 n bytes -> ((n, 13) uint64 affine words, n
        uint8 zk_point_status).  An invalid point has a non-zero status and
        zero words; nothing is raised for it."""
        return self._decompress("zk_g1_decompress", data, G1_BYTES, G1_WORDS)

    def g2_decompress(self, data):
        """zk_g2_decompress: 96 n bytes -> ((n, 25) words, n statuses)."""
        return self._decompress("zk_g2_decompress", data, G2_BYTES, G2_WORDS)

    def _validate(self, name, arr, words):
        a = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, words)
        st = np.zeros(len(a), dtype=np.uint8)
        if len(a):
            rc = getattr(lib(), name)(C.c_void_p(self._h), _p(a), C.c_size_t(len(a)), _p(st), None)
            if not (rc == ZK_ERR_ARG and st.any()):
                _check(rc, self, name)
        return st

    def g1_validate(self, arr):
        """zk_g1_validate: (n, 13) affine words -> n uint8 zk_point_status
        (coordinates < p, on the curve, in the prime-order subgroup)."""
        return self._validate("zk_g1_validate", arr, G1_WORDS)

    def g2_validate(self, arr):
        """zk_g2_validate: (n, 25) affine words -> n statuses."""
        return self._validate("zk_g2_validate", arr, G2_WORDS)

    # ---- n G1 points times one scalar (phase-2 key contributions) ----
    def _g1_mul_scalar(self, fn, name, points, k):
        a = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, G1_WORDS)
        k = int(k)
        if k < 0 or k >> 256:
            raise ValueError(f"{name}: the scalar must be in [0, r)")
        kw = np.array(to_limbs(k), dtype=np.uint64)   # whole: a scalar >= r is the library's error
        out = np.zeros_like(a)
        _check(fn(C.c_void_p(self._h), _p(a) if len(a) else None, C.c_size_t(len(a)), _p(kw),
                  _p(out) if len(a) else None), self, name)
        return out

    def g1_mul_scalar(self, points, k):
        """zk_g1_mul_scalar: (n, 13) affine words and one scalar 0 <= k < r ->
        (n, 13) words of k * point, one lane per point.  The points are taken
        as canonical, on the curve and in the prime-order subgroup
        (g1_validate checks that).  ValueError for k >= r."""
        return self._g1_mul_scalar(lib().zk_g1_mul_scalar, "zk_g1_mul_scalar", points, k)

    def test_g1_mul_scalar_plain(self, points, k):
        """zk_test_g1_mul_scalar_plain (test library): g1_mul_scalar through
        the plain 255-bit double-and-add walk."""
        return self._g1_mul_scalar(test_lib().zk_test_g1_mul_scalar_plain, "zk_test_g1_mul_scalar_plain", points, k)

    # ---- n points times n scalars (phase-1 contributions to a string) ----
    def _mul_scalars(self, load, name, points, scalars, words):
        a = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, words)
        ks = [int(k) for k in scalars]
        if len(ks) != len(a):
            raise ValueError(f"{name}: {len(a)} points but {len(ks)} scalars")
        if any(k < 0 or k >> 256 for k in ks):
            raise ValueError(f"{name}: every scalar must be in [0, r)")
        # whole values: a scalar >= r is the library's error, which names the index
        kw = np.array([to_limbs(k) for k in ks], dtype=np.uint64).reshape(-1, 4)
        out = np.zeros_like(a)
        fn = getattr(load(), name)
        _check(fn(C.c_void_p(self._h), _p(a) if len(a) else None, C.c_size_t(len(a)), _p(kw) if len(a) else None,
                  _p(out) if len(a) else None), self, name)
        return out

    def g1_mul_scalars(self, points, scalars):
        """zk_g1_mul_scalars: (n, 13) affine words and n scalars 0 <= k_i < r ->
        (n, 13) words of k_i * point_i, one lane per point.  The points are
        taken as canonical, on the curve and in the prime-order subgroup
        (g1_validate checks that).  ValueError for a scalar >= r (the message
        names the index)."""
        return self._mul_scalars(lib, "zk_g1_mul_scalars", points, scalars, G1_WORDS)

    def g2_mul_scalars(self, points, scalars):
        """zk_g2_mul_scalars: the same for (n, 25) G2 words."""
        return self._mul_scalars(lib, "zk_g2_mul_scalars", points, scalars, G2_WORDS)

    def test_g1_mul_scalars_plain(self, points, scalars):
        """zk_test_g1_mul_scalars_plain (test library): g1_mul_scalars through
        the plain per-lane 255-bit double-and-add walk."""
        return self._mul_scalars(test_lib, "zk_test_g1_mul_scalars_plain", points,
                                 scalars, G1_WORDS)

    def test_g2_mul_scalars_plain(self, points, scalars):
        """zk_test_g2_mul_scalars_plain (test library)."""
        return self._mul_scalars(test_lib, "zk_test_g2_mul_scalars_plain", points,
                                 scalars, G2_WORDS)

    def test_g1_mul_scalars_table(self, points, scalars):
        """zk_test_g1_mul_scalars_table (test library): the table walk,
        whichever walk g1_mul_scalars ships."""
        return self._mul_scalars(test_lib, "zk_test_g1_mul_scalars_table", points,
                                 scalars, G1_WORDS)

    def test_g2_mul_scalars_table(self, points, scalars):
        """zk_test_g2_mul_scalars_table (test library)."""
        return self._mul_scalars(test_lib, "zk_test_g2_mul_scalars_table", points,
                                 scalars, G2_WORDS)

    def test_gn_walk(self, points, scalars, g2=False, mem=False):
        """zk_test_gn_walk (test library): (n, 13 | 25) affine words and n
        scalars 0 <= k_i < r -> the words of k_i * point_i through the per-lane
        walks of csrc/srs.hpp, every lane from its own top bit: gn_walk_aff
        (mem=False) or gn_walk_mem (mem=True).  scalars: ints, or an (n, 4)
        uint64 array of canonical limbs, passed on whole.  ValueError for a
        scalar >= r (the message names the index)."""
        words = G2_WORDS if g2 else G1_WORDS
        a = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, words)
        if isinstance(scalars, np.ndarray):
            kw = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        else:
            ks = [int(k) for k in scalars]
            if any(k < 0 or k >> 256 for k in ks):
                raise ValueError("zk_test_gn_walk: every scalar must be in [0, r)")
            kw = np.array([to_limbs(k) for k in ks], dtype=np.uint64).reshape(-1, 4)
        n = len(a)
        if len(kw) != n:
            raise ValueError(f"zk_test_gn_walk: {n} points but {len(kw)} scalars")
        out = np.zeros_like(a)
        _check(test_lib().zk_test_gn_walk(C.c_void_p(self._h), C.c_int(int(bool(g2))), C.c_int(int(bool(mem))),
                                          _p(a) if n else None, C.c_size_t(n), _p(kw) if n else None,
                                          _p(out) if n else None), self, "zk_test_gn_walk")
        return out

    def test_split_scalars(self, scalars):
        """zk_test_split_scalars (test library): the device decomposition of n
        scalars below r -> (g1, g2), two (n, 4) uint64 arrays: e1 (two words)
        and e2 (two words) with (e2, e1) = divmod(k, x^2), and the four base-x
        digits of k."""
        ks = [int(k) for k in scalars]
        if any(k < 0 or k >> 256 for k in ks):
            raise ValueError("zk_test_split_scalars: every scalar must be in [0, r)")
        kw = np.array([to_limbs(k) for k in ks], dtype=np.uint64).reshape(-1, 4)
        g1 = np.zeros_like(kw)
        g2 = np.zeros_like(kw)
        n = len(kw)
        _check(test_lib().zk_test_split_scalars(C.c_void_p(self._h), _p(kw) if n else None, C.c_size_t(n),
                                                _p(g1) if n else None, _p(g2) if n else None),
               self, "zk_test_split_scalars")
        return g1, g2

    # ---- batch verification on the GPU (one lane per proof / product) ----
    @staticmethod
    def _verify_inputs(vk, inputs, n):
        """the public inputs of n proofs as an (n, n_inputs, 4) uint64 array"""
        if isinstance(inputs, np.ndarray) and inputs.ndim == 3:
            inp = np.ascontiguousarray(inputs, dtype=np.uint64)
        else:
            rows = [_fr_rows(r) for r in inputs]
            if len({len(r) for r in rows}) > 1:
                raise InvalidWitness("verify_many: rows of public inputs of different lengths")
            inp = np.zeros((len(rows), len(rows[0]) if rows else vk.num_public, 4), dtype=np.uint64)
            for k, r in enumerate(rows):
                inp[k] = r
        if len(inp) != n or inp.shape[2] != 4:
            raise ValueError("verify_many: one row of public inputs (n_inputs x 4 words) per proof")
        return inp

    def verify_many(self, vk, proofs, inputs, sound=False):
        """zk_groth16_verify_many: n proofs (Proof objects, or an (n, 51)
        uint64 array of their words) against one vk, inputs an (n, n_inputs,
        4) uint64 array or n rows of ints -> n uint8 ZK_VERIFY_* statuses,
        each what Verifier.verify says for that proof alone (MALFORMED where
        it raises ValueError).  InvalidWitness when n_inputs != vk.num_public.
        sound: zk_groth16_verify_many_sound -- the whole public inputs, one
        >= r making its proof MALFORMED."""
        if isinstance(proofs, np.ndarray):
            pw = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 2 * G1_WORDS + G2_WORDS)
        else:
            pw = np.ascontiguousarray([p.words for p in proofs], dtype=np.uint64).reshape(-1, 2 * G1_WORDS + G2_WORDS)
        n = len(pw)
        inp = self._verify_inputs(vk, inputs, n)
        st = np.zeros(n, dtype=np.uint8)
        if isinstance(vk, PreparedVerificationKey):   # zk_groth16_verify_many_prepared: the mode is the key's
            fn, key = lib().zk_groth16_verify_many_prepared, vk._handle()
        else:
            fn = lib().zk_groth16_verify_many_sound if sound else lib().zk_groth16_verify_many
            key = C.byref(vk.s)
        rc = fn(C.c_void_p(self._h), key, _p(pw) if n else None, _p(inp) if inp.size else None,
                C.c_size_t(inp.shape[1]), C.c_size_t(n), _p(st) if n else None)
        _check(rc, self, "zk_groth16_verify_many")
        return st

    # ---- prepared verification keys ----
    def vk_prepare(self, vk, sound=None):
        """zk_vk_prepare: validate every point of vk (subgroup included) and
        keep its per-key words and the window table of its ic_g1 on the
        device -> PreparedVerificationKey.  sound: the key's mode, vk.sound by
        default.  ValueError naming a bad point."""
        h = C.c_void_p()
        sound = getattr(vk, "sound", False) if sound is None else bool(sound)
        _check(lib().zk_vk_prepare(C.c_void_p(self._h), C.byref(vk.s), C.c_int(int(sound)), C.byref(h)),
               self, "zk_vk_prepare")
        return PreparedVerificationKey(self, h.value, vk.num_public)

    def prepare_inputs(self, pvk, inputs):
        """zk_groth16_prepare_inputs: IC = ic[0] + sum x_k ic[k + 1] for n rows
        of public inputs ((n, n_inputs, 4) uint64, or rows of ints) -> ((n, 13)
        uint64 words, n uint8 ok).  A sound key's row with an input >= r has
        ok = 0 and zero words."""
        if isinstance(inputs, np.ndarray) and inputs.ndim == 3:
            n = len(inputs)
        else:
            inputs = list(inputs)
            n = len(inputs)
        inp = self._verify_inputs(pvk, inputs, n)
        ic = np.zeros((n, G1_WORDS), dtype=np.uint64)
        ok = np.zeros(n, dtype=np.uint8)
        rc = lib().zk_groth16_prepare_inputs(C.c_void_p(self._h), pvk._handle(), _p(inp) if inp.size else None,
                                             C.c_size_t(inp.shape[1]), C.c_size_t(n), _p(ic) if n else None,
                                             _p(ok) if n else None)
        _check(rc, self, "zk_groth16_prepare_inputs")
        return ic, ok

    def test_prepared_force(self, width=0, run=0):
        """zk_test_prepared_force (test library): the window width of the keys
        prepared from now on and the run length of every sum, 0 the rules."""
        _check(test_lib().zk_test_prepared_force(C.c_void_p(self._h), C.c_int(width), C.c_uint32(run)), self,
               "zk_test_prepared_force")

    def test_msm_force(self, T=0, fix_max=0):
        """zk_test_msm_force (test library): the accumulate units and the fixup
        threshold of every MSM this context launches from now on, 0 the rules."""
        _check(test_lib().zk_test_msm_force(C.c_void_p(self._h), C.c_uint32(T), C.c_uint32(fix_max)), self,
               "zk_test_msm_force")

    def test_msm_scrub(self):
        """zk_test_msm_scrub (test library): overwrite what earlier MSMs left in
        this context's MSM workspaces, so that no MSM can pass on stale sums."""
        _check(test_lib().zk_test_msm_scrub(C.c_void_p(self._h)), self, "zk_test_msm_scrub")

    def test_msm_info(self, which=0, g2=False):
        """zk_test_msm_info (test library): {name: value} over TEST_MSM_INFO for
        the last finished MSM of workspace `which`."""
        v = (C.c_uint32 * len(TEST_MSM_INFO))()
        _check(test_lib().zk_test_msm_info(C.c_void_p(self._h), C.c_int(which), C.c_int(1 if g2 else 0), v), self,
               "zk_test_msm_info")
        return dict(zip(TEST_MSM_INFO, (int(x) for x in v)))

    def test_msm_grouping(self, which=0):
        """zk_test_msm_grouping (test library): (off[0..G], key[0..M), ent[0..M))
        of the last finished MSM of workspace `which`, uint32 arrays."""
        G, M = C.c_size_t(), C.c_size_t()
        fn = test_lib().zk_test_msm_grouping
        _check(fn(C.c_void_p(self._h), C.c_int(which), None, None, None, C.c_size_t(0), C.byref(G), C.byref(M)),
               self, "zk_test_msm_grouping")
        cap = max(G.value + 1, M.value)
        off, key, ent = (np.zeros(cap, dtype=np.uint32) for _ in range(3))
        _check(fn(C.c_void_p(self._h), C.c_int(which), _p(off), _p(key), _p(ent), C.c_size_t(cap), C.byref(G),
                  C.byref(M)), self, "zk_test_msm_grouping")
        return off[:G.value + 1], key[:M.value], ent[:M.value]

    @staticmethod
    def _proof_bytes(data, what):
        """bytes, or an (n, 192) uint8 array -> (flat uint8 array, n)"""
        if isinstance(data, np.ndarray):
            buf = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        else:
            buf = np.frombuffer(bytes(data), dtype=np.uint8)
        if len(buf) % PROOF_BYTES:
            raise ValueError(f"{what}: {len(buf)} bytes is not a whole number of {PROOF_BYTES}-byte proofs")
        return buf, len(buf) // PROOF_BYTES

    def proofs_deserialize(self, data):
        """zk_proofs_deserialize_compressed: n compressed proofs (bytes, or an
        (n, 192) uint8 array) -> ((n, 51) uint64 proof words, (n, 3) uint8
        zk_point_status of a, b, c).  An invalid point has a non-zero status
        and zero words; nothing is raised for it."""
        buf, n = self._proof_bytes(data, "proofs_deserialize")
        out = np.zeros((n, PROOF_WORDS), dtype=np.uint64)
        pst = np.zeros((n, 3), dtype=np.uint8)
        if n:
            rc = lib().zk_proofs_deserialize_compressed(C.c_void_p(self._h), _p(buf), C.c_size_t(n), _p(out), _p(pst))
            if not (rc == ZK_ERR_ARG and pst.any()):   # invalid points are reported by their status
                _check(rc, self, "zk_proofs_deserialize_compressed")
        return out, pst

    def verify_many_bytes(self, vk, data, inputs, sound=False, point_status=False):
        """zk_groth16_verify_many_bytes: verify_many on n compressed proofs
        (bytes, or an (n, 192) uint8 array), decoded and subgroup-checked on
        the GPU in the same call -> n uint8 ZK_VERIFY_* statuses, MALFORMED
        where Proof.deserialize_compressed raises, else what Verifier.verify
        says.  point_status: also return the (n, 3) zk_point_status of a, b,
        c.  sound: zk_groth16_verify_many_bytes_sound."""
        buf, n = self._proof_bytes(data, "verify_many_bytes")
        inp = self._verify_inputs(vk, inputs, n)
        st = np.zeros(n, dtype=np.uint8)
        pst = np.zeros((n, 3), dtype=np.uint8)
        if isinstance(vk, PreparedVerificationKey):   # zk_groth16_verify_many_bytes_prepared
            fn, key = lib().zk_groth16_verify_many_bytes_prepared, vk._handle()
        else:
            fn = lib().zk_groth16_verify_many_bytes_sound if sound else lib().zk_groth16_verify_many_bytes
            key = C.byref(vk.s)
        rc = fn(C.c_void_p(self._h), key, _p(buf) if n else None, _p(inp) if inp.size else None,
                C.c_size_t(inp.shape[1]), C.c_size_t(n), _p(st) if n else None,
                _p(pst) if n and point_status else None)
        _check(rc, self, "zk_groth16_verify_many_bytes")
        return (st, pst) if point_status else st

    @staticmethod
    def _coeffs(coeffs, n):
        co = _fr_rows(coeffs) if n else np.zeros((0, 4), dtype=np.uint64)
        if len(co) != n:
            raise ValueError("verify_all: one coefficient per proof")
        return co

    def verify_all(self, vk, proofs, inputs, coeffs):
        """zk_groth16_verify_all_sound: ONE pairing check for n proofs (as
        verify_many takes them) against a sound vk, with the coefficients
        c_k (ints or (n, 4) words; non-zero, below 2^128) of the random linear
        combination -> (valid, first_malformed): valid iff no proof is
        malformed (range, curve, subgroup, an input >= r) and the combined
        check holds; first_malformed the lowest malformed index, or n.  With
        several invalid proofs the check passes with probability ~2^-127 over
        uniform coefficients: draw them with `secrets` (Verifier.verify_all
        does).  ValueError for a bad coefficient, InvalidWitness when
        n_inputs != vk.num_public."""
        if isinstance(proofs, np.ndarray):
            pw = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, PROOF_WORDS)
        else:
            pw = np.ascontiguousarray([p.words for p in proofs], dtype=np.uint64).reshape(-1, PROOF_WORDS)
        n = len(pw)
        inp = self._verify_inputs(vk, inputs, n)
        co = self._coeffs(coeffs, n)
        valid, first = C.c_int(0), C.c_size_t(0)
        rc = lib().zk_groth16_verify_all_sound(
            C.c_void_p(self._h), C.byref(vk.s), _p(pw) if n else None, _p(inp) if inp.size else None,
            C.c_size_t(inp.shape[1]), C.c_size_t(n), _p(co) if n else None, C.byref(valid), C.byref(first))
        _check(rc, self, "zk_groth16_verify_all_sound")
        return bool(valid.value), int(first.value)

    def verify_all_bytes(self, vk, data, inputs, coeffs, point_status=False):
        """zk_groth16_verify_all_bytes_sound: verify_all on n compressed
        proofs (bytes, or an (n, 192) uint8 array), decoded and
        subgroup-checked on the GPU in the same call -> (valid,
        first_malformed), with point_status also the (n, 3) zk_point_status
        of a, b, c."""
        buf, n = self._proof_bytes(data, "verify_all_bytes")
        inp = self._verify_inputs(vk, inputs, n)
        co = self._coeffs(coeffs, n)
        pst = np.zeros((n, 3), dtype=np.uint8)
        valid, first = C.c_int(0), C.c_size_t(0)
        rc = lib().zk_groth16_verify_all_bytes_sound(
            C.c_void_p(self._h), C.byref(vk.s), _p(buf) if n else None, _p(inp) if inp.size else None,
            C.c_size_t(inp.shape[1]), C.c_size_t(n), _p(co) if n else None, C.byref(valid), C.byref(first),
            _p(pst) if n and point_status else None)
        _check(rc, self, "zk_groth16_verify_all_bytes_sound")
        out = (bool(valid.value), int(first.value))
        return out + (pst,) if point_status else out

    def test_verify_all_parts(self, vk, proofs, inputs, coeffs):
        """zk_test_verify_all_parts (test library): the three folds of
        verify_all -> (S_C as 13 affine words, the n_inputs + 1 scalars
        (s, t_0 ..) as ints, FINAL_EXP(conj(F)) as 72 words)."""
        pw = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, PROOF_WORDS)
        n = len(pw)
        inp = self._verify_inputs(vk, inputs, n)
        co = self._coeffs(coeffs, n)
        sum_c = np.zeros(G1_WORDS, dtype=np.uint64)
        scal = np.zeros((inp.shape[1] + 1, 4), dtype=np.uint64)
        gt = np.zeros(FQ12_WORDS, dtype=np.uint64)
        rc = test_lib().zk_test_verify_all_parts(
            C.c_void_p(self._h), C.byref(vk.s), _p(pw) if n else None, _p(inp) if inp.size else None,
            C.c_size_t(inp.shape[1]), C.c_size_t(n), _p(co) if n else None, _p(sum_c), _p(scal), _p(gt))
        _check(rc, self, "zk_test_verify_all_parts")
        return sum_c, [sum(int(w) << (64 * i) for i, w in enumerate(row)) for row in scal], gt

    def test_fixed_base(self, scalars, g2=False):
        """zk_test_fixed_base_g1 / _g2 (test library): scalars (ints, or (n, 4)
        uint64 canonical limbs) -> (n, 13 | 25) words of scalar * generator
        through the 255-bit fixed-base kernel of a sound setup."""
        sc = _fr_rows(scalars)
        out = np.zeros((max(len(sc), 1), G2_WORDS if g2 else G1_WORDS), dtype=np.uint64)
        fn = test_lib().zk_test_fixed_base_g2 if g2 else test_lib().zk_test_fixed_base_g1
        _check(fn(C.c_void_p(self._h), _p(sc) if len(sc) else None, C.c_size_t(len(sc)), _p(out)), self,
               "zk_test_fixed_base")
        return out[:len(sc)]

    def test_key_srs_coeffs(self, qap, num_public, rho):
        """zk_test_key_srs_coeffs (test library): the coefficient side of
        CRS.verify_against_srs on its own -> six lists of n ints, the vectors
        m^{M,part} for A pub, A priv, B pub, B priv, C pub, C priv, for
        rho = num_variables values below r split at column num_public."""
        sc = _fr_rows(rho)
        if len(sc) != qap.num_variables:
            raise ValueError("test_key_srs_coeffs: one rho per variable")
        n = qap.domain_size
        out = np.zeros((6 * n, 4), dtype=np.uint64)
        _check(test_lib().zk_test_key_srs_coeffs(C.c_void_p(self._h), C.byref(qap.csr.s), C.c_uint64(num_public),
                                                 _p(sc), _p(out)), self, "zk_test_key_srs_coeffs")
        vals = [from_limbs(row) for row in out]
        return [vals[k * n:(k + 1) * n] for k in range(6)]

    def pairing_products(self, g1_points, g2_points, pairs_per_product):
        """zk_pairing_products: product j = prod_{i<k} e(g1[jk+i], g2[jk+i])
        with k = pairs_per_product -> one uint8 ZK_VERIFY_* status per product
        (ACCEPT: the product is 1; MALFORMED: a point of it is not canonical
        or off its curve)."""
        a = np.ascontiguousarray(g1_points, dtype=np.uint64).reshape(-1, G1_WORDS)
        b = np.ascontiguousarray(g2_points, dtype=np.uint64).reshape(-1, G2_WORDS)
        k = int(pairs_per_product)
        if len(a) != len(b) or k < 1 or len(a) % k:
            raise ValueError("as many G1 as G2 points, a whole number of products")
        n = len(a) // k
        st = np.zeros(n, dtype=np.uint8)
        rc = lib().zk_pairing_products(C.c_void_p(self._h), _p(a) if n else None, _p(b) if n else None, C.c_size_t(k),
                                       C.c_size_t(n), _p(st) if n else None)
        _check(rc, self, "zk_pairing_products")
        return st

    # ---- the hash to G2 and proofs of knowledge (include/zkp.h) ----
    @staticmethod
    def _messages(msgs):
        if isinstance(msgs, np.ndarray):
            m = np.ascontiguousarray(msgs, dtype=np.uint8)
            if m.ndim != 2:
                raise ValueError("hash_to_g2: messages as an (n, msg_len) uint8 array")
            return m
        msgs = [bytes(x) for x in msgs]
        if len({len(x) for x in msgs}) > 1:
            raise ValueError("hash_to_g2: the messages of one call share their length")
        ln = len(msgs[0]) if msgs else 0
        return np.frombuffer(b"".join(msgs), dtype=np.uint8).reshape(len(msgs), ln).copy()

    def _hash_to_g2(self, fn, name, msgs, dst, *extra):
        m = self._messages(msgs)
        n, ln = m.shape
        dst = bytes(dst)
        out = np.zeros((n, G2_WORDS), dtype=np.uint64)
        tries = np.zeros(n, dtype=np.uint8)
        d = np.frombuffer(dst, dtype=np.uint8) if dst else None
        rc = fn(C.c_void_p(self._h), _p(m) if m.size else None, C.c_size_t(n), C.c_size_t(ln),
                _p(d) if d is not None else None, C.c_size_t(len(dst)), *extra, _p(out) if n else None,
                _p(tries) if n else None)
        _check(rc, self, name)
        return out, tries

    def hash_to_g2(self, msgs, dst):
        """zk_hash_to_g2 (ZKAMD-H2G2-V1): messages of one length, as a list of
        bytes or an (n, msg_len) uint8 array, with one dst (at most 255 bytes)
        -> ((n, 25) affine words, n uint8 try counts); a message without a
        point has tries 0xff and zero words.  One lane per message."""
        return self._hash_to_g2(lib().zk_hash_to_g2, "zk_hash_to_g2", msgs, dst)

    def test_hash_to_g2_capped(self, msgs, dst, max_tries):
        """zk_test_hash_to_g2_capped: the same kernel, at most max_tries tries."""
        return self._hash_to_g2(test_lib().zk_test_hash_to_g2_capped, "zk_test_hash_to_g2_capped", msgs, dst,
                                C.c_uint32(int(max_tries)))

    def g1_leaf_digests(self, points):
        """zk_g1_leaf_digests on the GPU: (n, 13) affine words -> a
        (ceil(n / 256), 32) uint8 array, the V2 leaf digests (include/zkp.h,
        "tree digests"), one lane per leaf of 256 points."""
        return _leaf_digests(self, "zk_g1_leaf_digests", points, G1_WORDS)

    def g2_leaf_digests(self, points):
        """zk_g2_leaf_digests on the GPU: (n, 25) affine words -> leaf digests."""
        return _leaf_digests(self, "zk_g2_leaf_digests", points, G2_WORDS)

    def pok_verify_many(self, poks, roles, challenges):
        """zk_pok_verify_many: n proofs ((n, 38) words: s_g1 then s_r), their
        roles (ZK_POK_*) and 32-byte challenges -> (n uint8 ZK_POK_* statuses,
        first_bad: the lowest index that is not ZK_POK_OK, or n).  Validation,
        hash and pairing product run on the GPU in one call.  ValueError for a
        role above 3."""
        pk = np.ascontiguousarray(poks, dtype=np.uint64).reshape(-1, POK_WORDS)
        n = len(pk)
        ro = np.ascontiguousarray(roles, dtype=np.uint8).reshape(-1)
        ch = _challenges(challenges, n)
        if len(ro) != n:
            raise ValueError("pok_verify_many: one role and one challenge per proof")
        st = np.zeros(n, dtype=np.uint8)
        fb = C.c_size_t(n)
        rc = lib().zk_pok_verify_many(C.c_void_p(self._h), _p(pk) if n else None, _p(ro) if n else None,
                                      _p(ch) if n else None, C.c_size_t(n), _p(st) if n else None, C.byref(fb))
        _check(rc, self, "zk_pok_verify_many")
        return st, fb.value

    # ---- the pairing's test hooks (include/zkp_test.h) ----
    def test_fq12(self, op, a, b=None):
        """zk_test_fq12: (n, 72) canonical words -> (n, 72)."""
        a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, FQ12_WORDS)
        out = np.zeros_like(a)
        if b is not None:
            b = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, FQ12_WORDS)
            if len(b) != len(a):
                raise ValueError("as many b as a")
        _check(test_lib().zk_test_fq12(C.c_void_p(self._h), C.c_int(int(op)), _p(a), _p(b) if b is not None else None,
                                       C.c_size_t(len(a)), _p(out)), self, "zk_test_fq12")
        return out

    def test_pairing_gt(self, g1_points, g2_points):
        """zk_test_pairing_gt: the device's final-exponentiated e(P_i, Q_i), (n, 72) words."""
        a = np.ascontiguousarray(g1_points, dtype=np.uint64).reshape(-1, G1_WORDS)
        b = np.ascontiguousarray(g2_points, dtype=np.uint64).reshape(-1, G2_WORDS)
        if len(a) != len(b):
            raise ValueError("as many G1 as G2 points")
        out = np.zeros((len(a), FQ12_WORDS), dtype=np.uint64)
        _check(test_lib().zk_test_pairing_gt(C.c_void_p(self._h), _p(a), _p(b), C.c_size_t(len(a)), _p(out)), self,
               "zk_test_pairing_gt")
        return out

    # ---- the field and point-formula hooks (include/zkp_test.h) ----
    def test_field(self, field, op, a, b=None, c=None, d=None):
        """zk_test_field: (n, W) uint32 raw device words per operand -> (n, W),
        W = TEST_FIELD_WORDS[field]."""
        w = TEST_FIELD_WORDS[field]
        ops = [None if x is None else np.ascontiguousarray(x, dtype=np.uint32).reshape(-1, w) for x in (a, b, c, d)]
        n = len(ops[0])
        if any(x is not None and len(x) != n for x in ops):
            raise ValueError("as many elements in every operand")
        out = np.zeros((n, w), dtype=np.uint32)
        args = [_p(x) if x is not None else None for x in ops]
        _check(test_lib().zk_test_field(C.c_void_p(self._h), C.c_int(int(field)), C.c_int(int(op)), *args,
                                        C.c_size_t(n), _p(out)), self, "zk_test_field")
        return out

    def test_curve(self, field, op, p=None, q=None):
        """zk_test_curve: p (n, 4 W) XYZZ points, q (n, 4 W) XYZZ or (n, 2 W)
        affine points as raw uint32 device words -> (n, 4 W) points; ADD_QUAD
        -> (n, 4, 4 W) and ADD_DUO -> (n, 2, 4 W): every lane's / lane pair's
        result."""
        w = TEST_FIELD_WORDS[field]
        aff = op in (ZK_TEST_COP_MADD, ZK_TEST_COP_AFF_DBL)
        p = None if p is None else np.ascontiguousarray(p, dtype=np.uint32).reshape(-1, 4 * w)
        q = None if q is None else np.ascontiguousarray(q, dtype=np.uint32).reshape(-1, (2 if aff else 4) * w)
        n = len(p) if p is not None else len(q)
        if p is not None and q is not None and len(p) != len(q):
            raise ValueError("as many q as p")
        per = {ZK_TEST_COP_ADD_QUAD: 4, ZK_TEST_COP_ADD_DUO: 2}.get(op, 1)
        out = np.zeros((n, per, 4 * w), dtype=np.uint32)
        _check(test_lib().zk_test_curve(C.c_void_p(self._h), C.c_int(int(field)), C.c_int(int(op)),
                                        _p(p) if p is not None else None, _p(q) if q is not None else None,
                                        C.c_size_t(n), _p(out)), self, "zk_test_curve")
        return out if per > 1 else out[:, 0]

    # ---- NTT (ark-poly Radix2EvaluationDomain fft / ifft / coset) ----
    def ntt(self, data, inverse=False, coset=None):
        a = np.ascontiguousarray(data, dtype=np.uint64).reshape(-1, 4).copy()
        n = len(a)
        log_n = n.bit_length() - 1
        if n == 0 or (1 << log_n) != n:
            raise DomainTooSmall(f"NTT size {n} is not a power of two")
        g = C.byref(_fr(coset)) if coset is not None else None
        rc = lib().zk_ntt_fr(C.c_void_p(self._h), _p(a), C.c_uint32(log_n),
                             C.c_int(-1 if inverse else 1), g)
        _check(rc, self, "zk_ntt_fr")
        return a

    # ---- the same transform over group elements (sound keys from a string) ----
    def _group_ntt(self, name, points, words, inverse):
        a = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, words).copy()
        n = len(a)
        log_n = n.bit_length() - 1
        if n == 0 or (1 << log_n) != n:
            raise DomainTooSmall(f"group NTT size {n} is not a power of two")
        _check(getattr(lib(), name)(C.c_void_p(self._h), _p(a), C.c_uint32(log_n), C.c_int(-1 if inverse else 1)),
               self, name)
        return a

    def g1_ntt(self, points, inverse=False):
        """zk_g1_ntt: (n, 13) affine words, n a power of two -> (n, 13) words of
        X_k = sum_j w^(jk) P_j (inverse: w^-1 and 1 / n), natural order in and
        out, w the root of ntt().  The points are taken as valid."""
        return self._group_ntt("zk_g1_ntt", points, G1_WORDS, inverse)

    def g2_ntt(self, points, inverse=False):
        """zk_g2_ntt: g1_ntt over (n, 25) G2 words."""
        return self._group_ntt("zk_g2_ntt", points, G2_WORDS, inverse)


# --------------------------------------------------------------- R1CS ----
class Variable(int):
    """crates/groth16-r1cs/src/lib.rs:20-35; Variable.ONE = 0."""

    def index(self):
        return int(self)


Variable.ONE = Variable(0)


class LinearCombination:
    """Sparse sum of coeff * var (crates/groth16-r1cs/src/lib.rs:46-118)."""

    def __init__(self, terms=None):
        self.terms = {}
        for v, c in (terms or {}).items():
            self.add_term(v, c)

    @classmethod
    def from_variable(cls, var):
        return cls({Variable(var): 1})

    @classmethod
    def from_constant(cls, c):
        return cls({Variable.ONE: c} if int(c) % R else {})

    def add_term(self, var, coeff):
        coeff = int(coeff) % R
        if coeff == 0:
            return
        var = Variable(var)
        v = (self.terms.get(var, 0) + coeff) % R
        if v:
            self.terms[var] = v
        else:
            self.terms.pop(var, None)

    def sub_lc(self, other):
        for v, c in other.terms.items():
            self.add_term(v, -c)


class R1CS:
    """crates/groth16-r1cs/src/lib.rs:229-358 (the builder subset on the path)."""

    def __init__(self, num_public_inputs=0):
        self.constraints = []
        self.num_public_inputs = num_public_inputs
        self.num_variables = 1 + num_public_inputs

    def allocate_variable(self):
        v = Variable(self.num_variables)
        self.num_variables += 1
        return v

    def add_constraint(self, a, b, c):
        self.constraints.append((a, b, c))

    def enforce_multiplication(self, a, b, c):
        self.add_constraint(a, b, c)

    def enforce_equal(self, left, right):
        diff = LinearCombination(dict(left.terms))
        diff.sub_lc(right)
        self.add_constraint(diff, LinearCombination.from_constant(1), LinearCombination())

    def num_constraints(self):
        return len(self.constraints)

    def is_satisfied(self, z):
        z = [int(x) % R for x in z]
        for a, b, c in self.constraints:
            ev = [sum(z[v] * k for v, k in lc.terms.items() if v < len(z)) % R for lc in (a, b, c)]
            if ev[0] * ev[1] % R != ev[2]:
                return False
        return True


class CSRMatrices:
    """The constraint matrices in CSR (zk_r1cs_csr); keeps the buffers alive."""

    def __init__(self, num_constraints, num_variables, mats):
        self.num_constraints, self.num_variables = int(num_constraints), int(num_variables)
        self.mats = mats  # 3 x (rowptr u64[nc+1], col u32[nnz], val u64[nnz,4] or None)
        self.s = _CSR()
        self.s.num_constraints, self.s.num_variables = self.num_constraints, self.num_variables
        for m, (rp, col, val) in zip("abc", mats):
            setattr(self.s, f"{m}_rowptr", rp.ctypes.data)
            setattr(self.s, f"{m}_col", col.ctypes.data)
            setattr(self.s, f"{m}_val", val.ctypes.data if val is not None else None)

    @classmethod
    def from_r1cs(cls, cs):
        mats = []
        for m in range(3):
            rp, cols, vals = [0], [], []
            for con in cs.constraints:
                for var in sorted(con[m].terms):
                    cols.append(int(var))
                    vals.append(to_limbs(con[m].terms[var]))
                rp.append(len(cols))
            mats.append((np.array(rp, dtype=np.uint64), np.array(cols, dtype=np.uint32),
                         np.array(vals, dtype=np.uint64).reshape(-1, 4)))
        return cls(cs.num_constraints(), cs.num_variables, mats)

    @classmethod
    def synthetic(cls, n):
        """groth16-cli generate_crs circuit (crates/groth16-cli/src/lib.rs:57-70):
        n x (x_j * y_j = z_j), variables x_j = 1+3j, y_j = 2+3j, z_j = 3+3j,
        unit coefficients (val = NULL)."""
        rp = np.arange(n + 1, dtype=np.uint64)
        j = np.arange(n, dtype=np.uint32)
        mats = [(rp, (1 + 3 * j).astype(np.uint32), None), (rp, (2 + 3 * j).astype(np.uint32), None),
                (rp, (3 + 3 * j).astype(np.uint32), None)]
        return cls(n, 3 * n + 1, mats)


class QAP:
    """crates/groth16-qap/src/lib.rs:31-46 in sparse form: the constraint
    matrices plus the radix-2 domain; the per-variable polynomials of the
    reference are never materialised (they are implied by the matrices)."""

    def __init__(self, csr):
        self.csr = csr
        self.num_variables = csr.num_variables
        self.num_constraints = csr.num_constraints
        n = 1
        while n < self.num_constraints:
            n <<= 1
        if n.bit_length() - 1 > 32:
            raise DomainTooSmall(f"domain {n} exceeds 2^32")
        self.domain_size = n

    @classmethod
    def from_r1cs(cls, cs):
        return cls(CSRMatrices.from_r1cs(cs))

    def degree(self):
        """max(per-variable degree < n, deg Z = n) = n (qap:285-294)."""
        return self.domain_size

    def evaluate_at(self, point, assignment, ctx=None):
        """QAP::evaluate_at (qap:190-220) on the GPU -> QAPEvaluation with
        A(point), B(point), C(point) = sum_i z_i A_i(point) ..., Z(point)."""
        ctx = ctx or default_context()
        z = _fr_rows(assignment)
        out = (_Fr * 4)()
        rc = lib().zk_qap_evaluate_at(C.c_void_p(ctx._h), C.byref(self.csr.s), C.byref(_fr(point)),
                                      _p(z) if len(z) else None, C.c_size_t(len(z)), out)
        _check(rc, ctx, "zk_qap_evaluate_at")
        a, b, c, zv = (sum(int(x) << (64 * i) for i, x in enumerate(o.l)) for o in out)
        return QAPEvaluation(a, b, c, zv)

    @staticmethod
    def verify_evaluation(ev):
        """QAP::verify_evaluation (qap:274-282)."""
        if ev.h_val is not None:
            return (ev.a_val * ev.b_val - ev.c_val) % R == ev.h_val * ev.z_val % R
        return ev.a_val * ev.b_val % R == ev.c_val


class QAPEvaluation:
    """QAPEvaluation (crates/groth16-qap/src/lib.rs:49-57): field values as ints."""

    def __init__(self, a_val, b_val, c_val, z_val, h_val=None):
        self.a_val, self.b_val, self.c_val, self.z_val, self.h_val = a_val, b_val, c_val, z_val, h_val


def batch_evaluate(polynomials, point, ctx=None):
    """qap utils::batch_evaluate (qap:315-322) on the GPU: each polynomial is
    a coefficient list (lowest degree first) of Fr ints or an (m, 4) array."""
    ctx = ctx or default_context()
    rows = [_fr_rows(p) if len(p) else np.zeros((0, 4), dtype=np.uint64) for p in polynomials]
    offs = np.zeros(len(rows) + 1, dtype=np.uint64)
    for i, r in enumerate(rows):
        offs[i + 1] = offs[i] + len(r)
    flat = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 4), dtype=np.uint64))
    out = np.zeros((max(len(rows), 1), 4), dtype=np.uint64)
    rc = lib().zk_poly_evaluate_batch(C.c_void_p(ctx._h), _p(flat) if len(flat) else None, _p(offs),
                                      C.c_size_t(len(rows)), C.byref(_fr(point)), _p(out))
    _check(rc, ctx, "zk_poly_evaluate_batch")
    return [from_limbs(o) for o in out[:len(rows)]]


_default_ctx = None


def default_context():
    """Context(0), created on first use (for reference-shaped calls that take no ctx)."""
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


# -------------------------------------------------------------- setup ----
class SetupParams:
    """crates/groth16-setup/src/lib.rs:82-136 (`s` is tau)."""

    def __init__(self, alpha, beta, gamma, delta, s):
        self.alpha, self.beta, self.gamma, self.delta, self.s = (int(x) % R for x in (alpha, beta, gamma, delta, s))

    @classmethod
    def random(cls, rng):
        """rng: callable returning a uniform Fr int (e.g. SplitMix64.fr)."""
        return cls(rng(), rng(), rng(), rng(), rng())

    def validate(self):
        if 0 in (self.alpha, self.beta, self.gamma, self.delta):
            raise SetupError("Setup parameters must be non-zero")

    def _c(self):
        p = _SetupParams()
        for k, v in (("alpha", self.alpha), ("beta", self.beta), ("gamma", self.gamma),
                     ("delta", self.delta), ("tau", self.s)):
            setattr(p, k, _fr(v))
        return p


# ------------------------------------------------- points of a key ----
def compress_g1(words):
    """zk_g1_compress: (n, 13) affine words -> 48 n bytes (ark compressed
    G1Affine; host only, does not validate)."""
    a = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, G1_WORDS)
    out = np.zeros(G1_BYTES * len(a), dtype=np.uint8)
    if len(a):
        _check(lib().zk_g1_compress(_p(a), C.c_size_t(len(a)), _p(out)), None, "zk_g1_compress")
    return out.tobytes()


def compress_g2(words):
    """zk_g2_compress: (n, 25) affine words -> 96 n bytes."""
    a = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, G2_WORDS)
    out = np.zeros(G2_BYTES * len(a), dtype=np.uint8)
    if len(a):
        _check(lib().zk_g2_compress(_p(a), C.c_size_t(len(a)), _p(out)), None, "zk_g2_compress")
    return out.tobytes()


# every point of a key in file order: (field, group, is a single point)
_PK_FIELDS = (("alpha_g1", 1, True), ("beta_g1", 1, True), ("delta_g1", 1, True), ("beta_g2", 2, True),
              ("delta_g2", 2, True), ("a_g1", 1, False), ("b_g1", 1, False), ("b_g2", 2, False),
              ("ic_g1", 1, False), ("h_g1", 1, False))
_VK_FIELDS = (("alpha_g1", 1, True), ("beta_g2", 2, True), ("gamma_g2", 2, True), ("delta_g2", 2, True),
              ("ic_g1", 1, False))


class InvalidPoint(Exception):
    """A key point failed decompression / validation: field, index, zk_point_status."""

    def __init__(self, field, index, status):
        self.field, self.index, self.status = field, int(index), int(status)
        super().__init__(f"{field}[{self.index}]: {POINT_STATUS_TEXT[self.status]}")


def _check_fields(ctx, fields, compressed):
    """fields: [(name, group, data)] in key order, data = affine words, or
    compressed bytes when `compressed`.  Neighbouring fields of one group go
    through the GPU in one call.  Returns the affine words per field; raises
    InvalidPoint for the first bad point in key order."""
    out, i = [], 0
    while i < len(fields):
        j = i
        while j < len(fields) and fields[j][1] == fields[i][1]:
            j += 1
        g1 = fields[i][1] == 1
        if compressed:
            counts = [len(f[2]) // (G1_BYTES if g1 else G2_BYTES) for f in fields[i:j]]
            words, st = (ctx.g1_decompress if g1 else ctx.g2_decompress)(b"".join(f[2] for f in fields[i:j]))
        else:
            parts = [np.asarray(f[2], dtype=np.uint64).reshape(-1, G1_WORDS if g1 else G2_WORDS) for f in fields[i:j]]
            counts = [len(a) for a in parts]
            words = np.concatenate(parts)
            st = (ctx.g1_validate if g1 else ctx.g2_validate)(words)
        lo = 0
        for (name, _, _), k in zip(fields[i:j], counts):
            bad = np.flatnonzero(st[lo:lo + k])
            if len(bad):
                raise InvalidPoint(name, bad[0], st[lo + bad[0]])
            out.append(words[lo:lo + k])
            lo += k
        i = j
    return out


def _key_fields(key, table):
    return [(nm, g, key.point(nm).reshape(1, -1) if single else getattr(key, nm)) for nm, g, single in table]


class ProvingKey:
    """crates/groth16-setup/src/lib.rs:27-52 (host arrays, canonical affine).
    sound: made by a sound setup (whole scalars, Z(tau) in h_g1); upload()
    and the key files carry the flag, so a key never changes mode."""

    def __init__(self, V, n, num_public, qap, sound=False):
        self.sound = bool(sound)
        self.a_g1 = np.zeros((V, G1_WORDS), dtype=np.uint64)
        self.b_g1 = np.zeros((V, G1_WORDS), dtype=np.uint64)
        self.b_g2 = np.zeros((V, G2_WORDS), dtype=np.uint64)
        self.ic_g1 = np.zeros((max(V - num_public - 1, 0), G1_WORDS), dtype=np.uint64)
        self.h_g1 = np.zeros((n, G1_WORDS), dtype=np.uint64)
        self.num_public = num_public
        self.qap = qap
        self.s = _PK()

    def _bind(self):
        s = self.s
        s.a_g1, s.a_len = self.a_g1.ctypes.data, len(self.a_g1)
        s.b_g1, s.b_len = self.b_g1.ctypes.data, len(self.b_g1)
        s.b_g2, s.b2_len = self.b_g2.ctypes.data, len(self.b_g2)
        s.ic_g1, s.ic_len = (self.ic_g1.ctypes.data if len(self.ic_g1) else None), len(self.ic_g1)
        s.h_g1, s.h_len = self.h_g1.ctypes.data, len(self.h_g1)
        s.num_public = self.num_public
        return s

    def point(self, name):
        """alpha_g1 / beta_g1 / delta_g1 / beta_g2 / delta_g2 as uint64 words."""
        return np.array(getattr(self.s, name).w, dtype=np.uint64)

    def validate(self, ctx=None):
        """ark's Validate::Yes on every point of the key, on the GPU: the five
        single points and the five base vectors must be canonical, on their
        curve and in the prime-order subgroup.  Raises SetupError naming the
        field, the index and the reason ("b_g2[17]: not in the prime-order
        subgroup").  Uploading a key never checks it; this does."""
        try:
            _check_fields(ctx or default_context(), _key_fields(self, _PK_FIELDS), False)
        except InvalidPoint as e:
            raise SetupError(str(e)) from None

    def upload(self, ctx, shard=0, nshards=1):
        return DeviceProvingKey.upload(ctx, self, shard, nshards)


class VerificationKey:
    """crates/groth16-setup/src/lib.rs:56-69.  sound: made by a sound setup;
    Verifier dispatches on it."""

    def __init__(self, num_public, sound=False):
        self.sound = bool(sound)
        self.ic_g1 = np.zeros((num_public + 1, G1_WORDS), dtype=np.uint64)
        self.num_public = num_public
        self.s = _VK()
        self.s.ic_g1 = self.ic_g1.ctypes.data
        self.s.ic_len = num_public + 1
        self.s.num_public = num_public

    @classmethod
    def from_points(cls, alpha_g1, beta_g2, gamma_g2, delta_g2, ic_g1, sound=False):
        """Build from canonical affine words (13 per G1, 25 per G2 point)."""
        ic = np.asarray(ic_g1, dtype=np.uint64).reshape(-1, G1_WORDS)
        vk = cls(len(ic) - 1, sound)
        vk.ic_g1[:] = ic
        for name, words in (("alpha_g1", alpha_g1), ("beta_g2", beta_g2), ("gamma_g2", gamma_g2),
                            ("delta_g2", delta_g2)):
            field = getattr(vk.s, name)
            for i, w in enumerate(np.asarray(words, dtype=np.uint64).reshape(-1)):
                field.w[i] = int(w)
        return vk

    def point(self, name):
        return np.array(getattr(self.s, name).w, dtype=np.uint64)

    def validate(self, ctx=None):
        """ProvingKey.validate for the four single points and ic_g1."""
        try:
            _check_fields(ctx or default_context(), _key_fields(self, _VK_FIELDS), False)
        except InvalidPoint as e:
            raise SetupError(str(e)) from None

    def prepare(self, ctx):
        """Context.vk_prepare in this key's mode -> PreparedVerificationKey."""
        return ctx.vk_prepare(self)


class PreparedVerificationKey:
    """A verification key prepared once and resident in HBM (zk_vk_dev), from
    VerificationKey.prepare: Verifier.verify_many / verify_many_bytes and the
    Context calls of those names take it in place of the key.  Its mode
    (.sound) was fixed when it was prepared."""

    def __init__(self, ctx, handle, num_public):
        self.ctx, self._h, self.num_public = ctx, handle, num_public
        self.sound = bool(lib().zk_vk_dev_is_sound(C.c_void_p(handle)))

    def _handle(self):
        if not getattr(self, "_h", None):
            raise ValueError("the prepared verification key has been freed")
        return C.c_void_p(self._h)

    def device_bytes(self):
        """zk_vk_dev_bytes: device memory the key holds (fixed words and window table)."""
        b = C.c_uint64()
        _check(lib().zk_vk_dev_bytes(self._handle(), C.byref(b)), None, "zk_vk_dev_bytes")
        return b.value

    def prepare_inputs(self, rows):
        """Context.prepare_inputs with this key: ((n, 13) words of IC, n ok bytes)."""
        return self.ctx.prepare_inputs(self, rows)

    def test_info(self):
        """zk_test_prepared_info (test library): (window width, windows)."""
        v = [C.c_uint32() for _ in range(2)]
        _check(test_lib().zk_test_prepared_info(self._handle(), *[C.byref(x) for x in v]), None,
               "zk_test_prepared_info")
        return tuple(x.value for x in v)

    def free(self):
        if getattr(self, "_h", None):
            lib().zk_vk_dev_free(C.c_void_p(self._h))
            self._h = None

    def __del__(self):
        self.free()


class MsmBases:
    """MSM bases resident in HBM (zk_msm_bases), from Context.msm_upload."""

    def __init__(self, ctx, handle, n, g2):
        self.ctx, self._h, self.n, self.g2 = ctx, handle, n, g2

    def msm(self, scalars, scalar_bits=255):
        """zk_msm_g1_dev / zk_msm_g2_dev: sum_i scalars[i] * bases[i] -> 13 | 25
        words.  scalars: (n, 4) canonical Fr, a numpy array (uploaded) or a
        torch int64 tensor on the context's device."""
        import torch
        if isinstance(scalars, torch.Tensor):
            d = scalars.contiguous()
        else:
            sc = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
            d = torch.from_numpy(sc.view(np.int64).copy()).to(f"cuda:{self.ctx.device}")
        out = np.zeros(G2_WORDS if self.g2 else G1_WORDS, dtype=np.uint64)
        fn = lib().zk_msm_g2_dev if self.g2 else lib().zk_msm_g1_dev
        _check(fn(C.c_void_p(self.ctx._h), C.c_void_p(self._h), C.c_void_p(d.data_ptr()), C.c_size_t(len(d)),
                  C.c_uint32(int(scalar_bits)), _p(out)), self.ctx, "zk_msm_dev")
        return out

    def free(self):
        if getattr(self, "_h", None):
            lib().zk_msm_bases_free(C.c_void_p(self._h))
            self._h = None

    def __del__(self):
        self.free()


class DeviceProvingKey:
    """A proving key resident in HBM (zk_pk_dev)."""

    def __init__(self, ctx, handle, qap):
        self.ctx, self._h, self.qap = ctx, handle, qap

    @classmethod
    def upload(cls, ctx, pk, shard=0, nshards=1):
        h = C.c_void_p()
        s = pk._bind()
        if getattr(pk, "sound", False):
            if nshards != 1:
                raise ValueError("a sound proving key cannot be sharded (nshards must be 1)")
            rc = lib().zk_pk_upload_sound(C.c_void_p(ctx._h), C.byref(s), C.byref(pk.qap.csr.s), C.byref(h))
        elif nshards == 1:
            rc = lib().zk_pk_upload(C.c_void_p(ctx._h), C.byref(s), C.byref(pk.qap.csr.s), C.byref(h))
        else:
            rc = lib().zk_pk_upload_shard(C.c_void_p(ctx._h), C.byref(s), C.byref(pk.qap.csr.s),
                                          C.c_uint32(shard), C.c_uint32(nshards), C.byref(h))
        _check(rc, ctx, "zk_pk_upload")
        return cls(ctx, h.value, pk.qap)

    @property
    def sound(self):
        """zk_pk_is_sound: the key proves with whole scalars (a sound setup)."""
        return bool(lib().zk_pk_is_sound(C.c_void_p(self._h)))

    def witness_ranges(self):
        """zk_groth16_witness_ranges: (k, 2) array of the [lo, hi) witness
        index ranges this shard reads on its ctx."""
        n = C.c_size_t()
        _check(lib().zk_groth16_witness_ranges(C.c_void_p(self.ctx._h), C.c_void_p(self._h), None, C.c_size_t(0),
                                               C.byref(n)), self.ctx, "zk_groth16_witness_ranges")
        out = np.zeros((max(n.value, 1), 2), dtype=np.uint64)
        _check(lib().zk_groth16_witness_ranges(C.c_void_p(self.ctx._h), C.c_void_p(self._h), _p(out),
                                               C.c_size_t(n.value), C.byref(n)), self.ctx, "zk_groth16_witness_ranges")
        return out[:n.value]

    def test_info(self):
        """zk_test_pk_info (test library): (win, win_c, shard, nshards)."""
        v = [C.c_uint32() for _ in range(4)]
        _check(test_lib().zk_test_pk_info(C.c_void_p(self._h), *[C.byref(x) for x in v]), None, "zk_test_pk_info")
        return tuple(x.value for x in v)

    def test_plan(self):
        """zk_test_pk_plan (test library): (copies of every base the key
        holds, bucket sets per prove MSM)."""
        v = [C.c_uint32() for _ in range(2)]
        _check(test_lib().zk_test_pk_plan(C.c_void_p(self._h), *[C.byref(x) for x in v]), None, "zk_test_pk_plan")
        return tuple(x.value for x in v)

    def device_bytes(self):
        """zk_pk_device_bytes: device memory the key holds (bases, indices, CSR)."""
        b = C.c_uint64()
        _check(lib().zk_pk_device_bytes(C.c_void_p(self._h), C.byref(b)), None, "zk_pk_device_bytes")
        return b.value

    def test_bases(self, slot, window=0):
        """zk_test_pk_bases (test library): (variable / coefficient index per
        compacted base, canonical words of the compacted bases + extras,
        number of extras) of one MSM slot's window copy."""
        cnt, nex = C.c_size_t(), C.c_size_t()
        _check(test_lib().zk_test_pk_bases(C.c_void_p(self.ctx._h), C.c_void_p(self._h), C.c_int(slot),
                                           C.c_int(window), None, None, C.c_size_t(0), C.byref(cnt), C.byref(nex)),
               self.ctx, "zk_test_pk_bases")
        tot = cnt.value + nex.value
        words = G2_WORDS if slot == 1 else G1_WORDS
        idx = np.zeros(max(cnt.value, 1), dtype=np.uint32)
        out = np.zeros((max(tot, 1), words), dtype=np.uint64)
        _check(test_lib().zk_test_pk_bases(C.c_void_p(self.ctx._h), C.c_void_p(self._h), C.c_int(slot),
                                           C.c_int(window), _p(idx), _p(out), C.c_size_t(max(tot, 1)),
                                           C.byref(cnt), C.byref(nex)), self.ctx, "zk_test_pk_bases")
        return idx[:cnt.value], out[:tot], nex.value

    def witness_slice(self, assignment):
        """This shard's part of a full witness (rows of every witness range, in order)."""
        a = np.asarray(assignment, dtype=np.uint64).reshape(-1, 4)
        rs = self.witness_ranges()
        return np.ascontiguousarray(np.concatenate([a[int(lo):int(hi)] for lo, hi in rs]) if len(rs)
                                    else np.zeros((0, 4), dtype=np.uint64))

    def free(self):
        if getattr(self, "_h", None):
            lib().zk_pk_free(C.c_void_p(self._h))
            self._h = None

    def __del__(self):
        self.free()


# -------------------------------------- hash to G2, proofs of knowledge ----
def _challenges(challenges, n):
    if isinstance(challenges, np.ndarray):
        ch = np.ascontiguousarray(challenges, dtype=np.uint8).reshape(-1, 32)
    else:
        ch = np.frombuffer(b"".join(bytes(c) for c in challenges), dtype=np.uint8).reshape(-1, 32).copy()
    if len(ch) != n:
        raise ValueError("one 32-byte challenge per proof")
    return ch


def _bytes_arg(data):
    data = bytes(data)
    return (np.frombuffer(data, dtype=np.uint8) if data else None), len(data)


def sha256(data):
    """zk_sha256: the library's SHA-256 (the one under the hash to G2) -> 32 bytes."""
    a, n = _bytes_arg(data)
    out = np.zeros(32, dtype=np.uint8)
    _check(lib().zk_sha256(_p(a) if n else None, C.c_size_t(n), _p(out)), None, "zk_sha256")
    return out.tobytes()


def hash_to_g2_host(msg, dst):
    """zk_hash_to_g2_host: one ZKAMD-H2G2-V1 hash on the host -> (25 affine
    words, tries).  ValueError for a dst above 255 bytes."""
    m, ml = _bytes_arg(msg)
    d, dl = _bytes_arg(dst)
    out = np.zeros(G2_WORDS, dtype=np.uint64)
    tries = C.c_uint8(0)
    rc = lib().zk_hash_to_g2_host(_p(m) if ml else None, C.c_size_t(ml), _p(d) if dl else None, C.c_size_t(dl),
                                  _p(out), C.byref(tries))
    _check(rc, None, "zk_hash_to_g2_host")
    return out, tries.value


def _leaf_digests(ctx, name, points, words):
    a = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, words)
    out = np.zeros((-(-len(a) // 256), 32), dtype=np.uint8)
    rc = getattr(lib(), name)(C.c_void_p(ctx._h) if ctx is not None else None, _p(a) if len(a) else None,
                              C.c_size_t(len(a)), _p(out) if len(a) else None)
    _check(rc, ctx, name)
    return out


def g1_leaf_digests_host(points):
    """zk_g1_leaf_digests with ctx == NULL: the host twin of
    Context.g1_leaf_digests, the same bytes without a GPU."""
    return _leaf_digests(None, "zk_g1_leaf_digests", points, G1_WORDS)


def g2_leaf_digests_host(points):
    """zk_g2_leaf_digests with ctx == NULL."""
    return _leaf_digests(None, "zk_g2_leaf_digests", points, G2_WORDS)


def _digest_version(version, what):
    if version not in (1, 2):
        raise ValueError(f"{what}: digest version {version!r} does not exist (1 or 2)")
    return version


def _pok_c(pok):
    w = np.ascontiguousarray(pok, dtype=np.uint64).reshape(POK_WORDS)
    return _Pok.from_buffer_copy(w.tobytes())


def pok_make(s, role, challenge):
    """zk_pok_make: the proof of knowledge of 0 < s < r for a role (ZK_POK_*)
    and a 32-byte challenge -> 38 words: [s]_1, then [s] R with R hashed from
    challenge | compress([s]_1) | role.  ValueError for a bad share or role."""
    s, challenge = int(s), bytes(challenge)
    if not 0 < s < R or len(challenge) != 32 or not 0 <= int(role) <= 3:
        raise ValueError("pok_make: a share in (0, r), a role 0..3 and a 32-byte challenge")
    ch = np.frombuffer(challenge, dtype=np.uint8)
    out = _Pok()
    _check(lib().zk_pok_make(C.byref(_fr(s)), C.c_uint8(int(role)), _p(ch), C.byref(out)), None, "zk_pok_make")
    return np.array(list(out.s_g1.w) + list(out.s_r.w), dtype=np.uint64)


def pok_verify(pok, role, challenge):
    """zk_pok_verify on the host -> a ZK_POK_* status (ZK_POK_OK: the proof is good)."""
    challenge = bytes(challenge)
    if len(challenge) != 32 or not 0 <= int(role) <= 3:
        raise ValueError("pok_verify: a role 0..3 and a 32-byte challenge")
    ch = np.frombuffer(challenge, dtype=np.uint8)
    st = C.c_int(-1)
    _check(lib().zk_pok_verify(C.byref(_pok_c(pok)), C.c_uint8(int(role)), _p(ch), C.byref(st)), None,
           "zk_pok_verify")
    return st.value


class CRS:
    """crates/groth16-setup/src/lib.rs:72-78, 139-278 (GPU setup)."""

    def __init__(self, pk, vk):
        self.pk, self.vk = pk, vk

    @classmethod
    def generate_from_qap(cls, ctx, qap, params, num_public, sound=False):
        """sound: zk_groth16_setup_sound -- whole scalars and Z(tau) in h_g1
        (textbook Groth16) instead of the reference's truncated ones; the
        keys carry .sound.  tau on the evaluation domain is a SetupError."""
        params.validate()
        if num_public >= qap.num_variables:
            raise SetupError("Number of public inputs must be less than total variables")
        pk = ProvingKey(qap.num_variables, qap.domain_size, num_public, qap, sound)
        vk = VerificationKey(num_public, sound)
        s = pk._bind()
        fn = lib().zk_groth16_setup_sound if sound else lib().zk_groth16_setup
        rc = fn(C.c_void_p(ctx._h), C.byref(qap.csr.s), C.byref(params._c()), C.c_uint64(num_public), C.byref(s),
                C.byref(vk.s))
        _check(rc, ctx, "zk_groth16_setup_sound" if sound else "zk_groth16_setup")
        return cls(pk, vk)

    @classmethod
    def generate_random(cls, ctx, qap, num_public, rng, sound=False):
        return cls.generate_from_qap(ctx, qap, SetupParams.random(rng), num_public, sound)

    @classmethod
    def from_srs(cls, ctx, qap, srs, num_public, sound=True):
        """zk_groth16_setup_srs_sound: the sound CRS of qap from a
        powers-of-tau string (SRS), with gamma = delta = 1 -- entry for entry
        generate_from_qap(sound=True) for (alpha, beta, 1, 1, tau), without the
        scalars: inverse group transforms of the powers give [L_i(tau)], sparse
        column sums over points the queries.  contribute() then randomises
        delta.  DomainTooSmall when the circuit's domain exceeds the string's,
        SetupError for num_public >= num_variables, tau on the domain, or a
        reference-mode request (truncated scalars: no string can produce them)."""
        if not sound:
            raise SetupError("from_srs: sound keys only (a reference-mode key truncates its scalars)")
        if num_public >= qap.num_variables:
            raise SetupError("Number of public inputs must be less than total variables")
        pk = ProvingKey(qap.num_variables, qap.domain_size, num_public, qap, True)
        vk = VerificationKey(num_public, True)
        rc = lib().zk_groth16_setup_srs_sound(C.c_void_p(ctx._h), C.byref(qap.csr.s), C.byref(srs._bind()),
                                              C.c_uint64(num_public), C.byref(pk._bind()), C.byref(vk.s))
        _check(rc, ctx, "zk_groth16_setup_srs_sound")
        return cls(pk, vk)

    @classmethod
    def from_prepared(cls, ctx, qap, prepared, num_public):
        """zk_groth16_setup_prepared_sound: from_srs's CRS, byte for byte, from
        a PreparedSRS (SRS.prepare) -- the column sums only, the transforms were
        paid once.  DomainTooSmall unless the circuit's domain is exactly the
        prepared one; SetupError for num_public >= num_variables."""
        if num_public >= qap.num_variables:
            raise SetupError("Number of public inputs must be less than total variables")
        pk = ProvingKey(qap.num_variables, qap.domain_size, num_public, qap, True)
        vk = VerificationKey(num_public, True)
        rc = lib().zk_groth16_setup_prepared_sound(C.c_void_p(ctx._h), C.byref(qap.csr.s), C.c_void_p(prepared._h),
                                                   C.c_uint64(num_public), C.byref(pk._bind()), C.byref(vk.s))
        _check(rc, ctx, "zk_groth16_setup_prepared_sound")
        return cls(pk, vk)

    @staticmethod
    def from_prepared_device(ctx, qap, prepared, num_public, vk=None):
        """zk_groth16_setup_prepared_sound_dev: from_prepared's proving key
        straight into HBM, no host key in between -> DeviceProvingKey, the one
        DeviceProvingKey.upload makes of from_prepared(...).pk.  vk: a
        VerificationKey(num_public, sound=True) to fill beside it."""
        if num_public >= qap.num_variables:
            raise SetupError("Number of public inputs must be less than total variables")
        if vk is not None and (vk.num_public != num_public or not vk.sound):
            raise ValueError("from_prepared_device: vk needs the call's num_public and sound mode")
        h = C.c_void_p()
        rc = lib().zk_groth16_setup_prepared_sound_dev(C.c_void_p(ctx._h), C.byref(qap.csr.s),
                                                       C.c_void_p(prepared._h), C.c_uint64(num_public), C.byref(h),
                                                       C.byref(vk.s) if vk is not None else None)
        _check(rc, ctx, "zk_groth16_setup_prepared_sound_dev")
        return DeviceProvingKey(ctx, h.value, qap)

    # ---- phase-2 contributions (sound keys) ----
    def copy(self):
        """A CRS with arrays and points of its own."""
        pk, vk = self.pk, self.vk
        npk = ProvingKey(len(pk.a_g1), len(pk.h_g1), pk.num_public, pk.qap, pk.sound)
        for nm in ("a_g1", "b_g1", "b_g2", "ic_g1", "h_g1"):
            setattr(npk, nm, np.array(getattr(pk, nm), dtype=np.uint64, copy=True))
        for nm, _, single in _PK_FIELDS:
            if single:
                setattr(npk.s, nm, type(getattr(pk.s, nm)).from_buffer_copy(getattr(pk.s, nm)))
        nvk = VerificationKey.from_points(vk.point("alpha_g1"), vk.point("beta_g2"), vk.point("gamma_g2"),
                                          vk.point("delta_g2"), vk.ic_g1, vk.sound)
        return CRS(npk, nvk)

    def contribute(self, ctx, d):
        """zk_groth16_contribute_sound: one phase-2 contribution with the
        secret share 0 < d < r -> a NEW CRS (this one is left untouched):
        delta_g1 and delta_g2 times d, every pk ic_g1 and h_g1 entry times
        1 / d on the GPU, everything else as it was -- the key
        generate_from_qap(sound=True) gives for delta * d.  SetupError for a
        reference-mode key (its h_g1 is not linear in 1 / delta) or a bad
        share.  A device key is not rescaled: upload the new one."""
        if not (self.pk.sound and self.vk.sound):
            raise SetupError("contribute: sound keys only (a reference-mode key cannot be rescaled)")
        d = int(d)
        if not 0 < d < R:
            raise SetupError("contribute: the share must be in (0, r)")
        new = self.copy()
        rc = lib().zk_groth16_contribute_sound(C.c_void_p(ctx._h), C.byref(new.pk._bind()), C.byref(new.vk.s),
                                               C.byref(_fr(d)))
        if rc == ZK_ERR_ARG:
            msg = lib().zk_last_error(ctx._h)
            raise SetupError(f"zk_groth16_contribute_sound failed ({rc}) {msg.decode() if msg else ''}".strip())
        _check(rc, ctx, "zk_groth16_contribute_sound")
        return new

    @staticmethod
    def verify_contribution(ctx, before, after, coeffs=None):
        """zk_groth16_verify_contribution_sound: is the CRS `after` a
        contribution on top of `before`? -> (ok, status), status the first
        ZK_CONTRIB_* check that fails (SHAPE, FIXED_PART, POINT, DELTA, RATIO)
        or ZK_CONTRIB_OK.  coeffs: len(h_g1) + len(ic_g1) non-zero integers
        below 2^128 (h_g1's first); None draws them from `secrets`, which is
        what a real check uses -- a wrong key then passes with probability
        about 2^-127.  It does not prove that the contributor knows the share.
        SetupError for reference-mode keys, ValueError for a bad coefficient."""
        for crs in (before, after):
            if not (crs.pk.sound and crs.vk.sound):
                raise SetupError("verify_contribution: sound keys only")
        n = len(before.pk.h_g1) + len(before.pk.ic_g1)
        if coeffs is None:
            import secrets
            coeffs = []
            for _ in range(n):
                c = 0
                while not c:      # uniform on [1, 2^128)
                    c = secrets.randbits(128)
                coeffs.append(c)
        co = _fr_rows(coeffs) if len(coeffs) else np.zeros((0, 4), dtype=np.uint64)
        st = C.c_int(-1)
        rc = lib().zk_groth16_verify_contribution_sound(
            C.c_void_p(ctx._h), C.byref(before.pk._bind()), C.byref(before.vk.s), C.byref(after.pk._bind()),
            C.byref(after.vk.s), _p(co) if len(co) else None, C.c_size_t(len(co)), C.byref(st))
        _check(rc, ctx, "zk_groth16_verify_contribution_sound")
        return st.value == ZK_CONTRIB_OK, st.value

    def verify_against_srs(self, ctx, srs, coeffs=None):
        """zk_groth16_verify_key_srs_sound: is this CRS the sound key of its
        circuit (self.pk.qap) over the string `srs`, for some delta and
        gamma = 1 -- what from_srs gives, after any number of contribute calls?
        -> (ok, status), status the first ZK_KEYSRS_* check that fails (SHAPE,
        POINT, FIXED, DELTA, QUERY_A, QUERY_B1, QUERY_B2, IC_VK, IC_PK, H) or
        ZK_KEYSRS_OK.  coeffs: num_variables + domain_size non-zero integers
        below 2^128 (one per variable, then one per h_g1 entry; ints, or their
        (n, 4) uint64 limbs); None draws them from `secrets`, which is what a
        real check uses -- a wrong key then passes with probability about
        2^-127.  No group transform runs:
        sparse row products, six scalar inverse transforms, MSMs over the key
        and over the string, a few pairings.  It does not prove that anyone
        knows the delta shares, and it takes the string as valid (SRS.verify).
        SetupError for reference-mode keys, ValueError for a bad coefficient,
        DomainTooSmall when the circuit's domain exceeds the string's."""
        if not (self.pk.sound and self.vk.sound):
            raise SetupError("verify_against_srs: sound keys only")
        qap = self.pk.qap
        n = qap.num_variables + qap.domain_size
        if coeffs is None:
            import secrets
            co = np.zeros((n, 4), dtype=np.uint64)      # uniform on [1, 2^128): zero rows are drawn again
            todo = np.arange(n)
            while len(todo):
                co[todo, :2] = np.frombuffer(secrets.token_bytes(16 * len(todo)), dtype=np.uint64).reshape(-1, 2)
                todo = todo[(co[todo, 0] | co[todo, 1]) == 0]
        elif isinstance(coeffs, np.ndarray):                # (n, 4) canonical limbs, as fr_array gives
            co = _fr_rows(coeffs)
        else:
            coeffs = [int(c) for c in coeffs]
            for i, c in enumerate(coeffs):
                if not 0 <= c < R:
                    raise ValueError(f"verify_against_srs: coefficient {i} must be non-zero and below 2^128")
            co = _fr_rows(coeffs) if len(coeffs) else np.zeros((0, 4), dtype=np.uint64)
        bad = np.flatnonzero(((co[:, 0] | co[:, 1]) == 0) | ((co[:, 2] | co[:, 3]) != 0))
        if len(bad):
            raise ValueError(f"verify_against_srs: coefficient {bad[0]} must be non-zero and below 2^128")
        st = C.c_int(-1)
        rc = lib().zk_groth16_verify_key_srs_sound(
            C.c_void_p(ctx._h), C.byref(qap.csr.s), C.byref(srs._bind()), C.byref(self.pk._bind()),
            C.byref(self.vk.s), _p(co) if len(co) else None, C.c_size_t(len(co)), C.byref(st))
        _check(rc, ctx, "zk_groth16_verify_key_srs_sound")
        return st.value == ZK_KEYSRS_OK, st.value

    # ---- phase-2 contributions with a proof of knowledge ----
    def digest(self, ctx=None, version=1):
        """The challenge of the next contribution's proof -> 32 bytes (layouts:
        include/zkp.h).  version 1: zk_groth16_key_digest_sound, one SHA-256
        over the key's compressed points on the host (ctx is not used).
        version 2: zk_groth16_key_digest_v2_sound, the tree digest -- leaves
        of 256 points hashed on the GPU when a ctx is given, by the host twin
        otherwise, the same bytes either way.  One ceremony uses one version."""
        out = np.zeros(32, dtype=np.uint8)
        if _digest_version(version, "CRS.digest") == 1:
            _check(lib().zk_groth16_key_digest_sound(C.byref(self.pk._bind()), C.byref(self.vk.s), _p(out)), None,
                   "zk_groth16_key_digest_sound")
        else:
            _check(lib().zk_groth16_key_digest_v2_sound(C.c_void_p(ctx._h) if ctx is not None else None,
                                                        C.byref(self.pk._bind()), C.byref(self.vk.s), _p(out)), ctx,
                   "zk_groth16_key_digest_v2_sound")
        return out.tobytes()

    def contribute_proved(self, ctx, d, digest_version=1):
        """contribute(ctx, d) and the contributor's proof that they know d:
        -> (new_crs, proof), proof = pok_make(d, ZK_POK_DELTA, challenge) with
        challenge = self.digest() (digest_version 1) or the tree digest
        self.digest(ctx, 2) (digest_version 2)."""
        _digest_version(digest_version, "CRS.contribute_proved")
        new = self.contribute(ctx, d)
        return new, pok_make(d, ZK_POK_DELTA, self.digest(ctx, digest_version))

    @staticmethod
    def verify_contribution_proof(ctx, before, after, proof, digest_version=1):
        """Does `proof` show knowledge of the share that took delta from
        `before` to `after`? -> (ok, status): zk_pok_verify_many on the proof
        with the digest of `before` (digest_version: the version the ceremony
        uses, as in contribute_proved), then the link
        e(s_g1, delta_2 before) e(-g1, delta_2 after) = 1 through
        pairing_products (a failed link is ZK_POK_REJECT).  It does not replace
        CRS.verify_contribution: a full audit runs both."""
        _digest_version(digest_version, "CRS.verify_contribution_proof")
        pk = np.ascontiguousarray(proof, dtype=np.uint64).reshape(POK_WORDS)
        st, _ = ctx.pok_verify_many(pk.reshape(1, -1), [ZK_POK_DELTA], [before.digest(ctx, digest_version)])
        if st[0] != ZK_POK_OK:
            return False, int(st[0])
        neg_g1 = np.array(to_limbs(G1_GENERATOR[0], 6) + to_limbs(FQ_MODULUS - G1_GENERATOR[1], 6) + [0],
                          dtype=np.uint64)
        link = ctx.pairing_products(np.stack([pk[:G1_WORDS], neg_g1]),
                                    np.stack([before.pk.point("delta_g2"), after.pk.point("delta_g2")]), 2)
        ok = link[0] == ZK_VERIFY_ACCEPT
        return bool(ok), ZK_POK_OK if ok else ZK_POK_REJECT

    @staticmethod
    def generate_device(ctx, qap, params, num_public, shard=0, nshards=1, sound=False, vk=None):
        """Setup straight into HBM (no host round trip) -> DeviceProvingKey.
        sound: zk_groth16_setup_sound_dev (never sharded).  vk: a
        VerificationKey(num_public) to fill beside it (unsharded setups)."""
        h = C.c_void_p()
        vkp = C.byref(vk.s) if vk is not None else None
        if vk is not None and (nshards != 1 or vk.num_public != num_public or bool(vk.sound) != bool(sound)):
            raise ValueError("generate_device: vk needs an unsharded setup, and its num_public and mode")
        if sound:
            if nshards != 1:
                raise ValueError("a sound proving key cannot be sharded (nshards must be 1)")
            rc = lib().zk_groth16_setup_sound_dev(C.c_void_p(ctx._h), C.byref(qap.csr.s), C.byref(params._c()),
                                                  C.c_uint64(num_public), C.byref(h), vkp)
        elif nshards == 1:
            rc = lib().zk_groth16_setup_dev(C.c_void_p(ctx._h), C.byref(qap.csr.s), C.byref(params._c()),
                                            C.c_uint64(num_public), C.byref(h), vkp)
        else:
            rc = lib().zk_groth16_setup_dev_shard(C.c_void_p(ctx._h), C.byref(qap.csr.s),
                                                  C.byref(params._c()), C.c_uint64(num_public),
                                                  C.c_uint32(shard), C.c_uint32(nshards), C.byref(h))
        _check(rc, ctx, "zk_groth16_setup_dev")
        return DeviceProvingKey(ctx, h.value, qap)


class SRS:
    """A powers-of-tau string (zk_srs) for domains up to N = 2^log_n:
    tau_g1 (2N, 13), tau_g2 (N, 25), alpha_tau_g1 and beta_tau_g1 (N, 13) words
    and beta_g2 (25 words).  CRS.from_srs makes a circuit's sound key from it."""

    def __init__(self, log_n):
        self.log_n = int(log_n)
        if not 0 <= self.log_n <= 31:
            raise DomainTooSmall(f"a string for 2^{self.log_n} does not exist (log_n in [0, 31])")
        N = 1 << self.log_n
        self.tau_g1 = np.zeros((2 * N, G1_WORDS), dtype=np.uint64)
        self.tau_g2 = np.zeros((N, G2_WORDS), dtype=np.uint64)
        self.alpha_tau_g1 = np.zeros((N, G1_WORDS), dtype=np.uint64)
        self.beta_tau_g1 = np.zeros((N, G1_WORDS), dtype=np.uint64)
        self.beta_g2 = np.zeros(G2_WORDS, dtype=np.uint64)
        self.s = _SRS()

    def _bind(self):
        s = self.s
        s.log_n = self.log_n
        for nm, ln in (("tau_g1", "tau_g1_len"), ("tau_g2", "tau_g2_len"), ("alpha_tau_g1", "alpha_len"),
                       ("beta_tau_g1", "beta_len")):
            a = getattr(self, nm)
            if not (isinstance(a, np.ndarray) and a.dtype == np.uint64 and a.flags.c_contiguous):
                a = np.ascontiguousarray(a, dtype=np.uint64)
                setattr(self, nm, a)
            setattr(s, nm, a.ctypes.data)
            setattr(s, ln, len(a))
        for i, w in enumerate(np.asarray(self.beta_g2, dtype=np.uint64).reshape(-1)):
            s.beta_g2.w[i] = int(w)
        return s

    def copy(self):
        """A string with arrays of its own."""
        new = SRS(self.log_n)
        for nm in ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2"):
            setattr(new, nm, np.array(getattr(self, nm), dtype=np.uint64, copy=True))
        return new

    @classmethod
    def generate(cls, ctx, log_n, tau, alpha, beta):
        """zk_srs_generate: the string of KNOWN secrets 0 < tau, alpha, beta < r
        -- for tests, demos and benchmarks: whoever ran this can forge proofs
        for every key made from the string.  SetupError for a zero or
        out-of-range parameter."""
        vals = [int(v) for v in (tau, alpha, beta)]
        if any(not 0 < v < R for v in vals):
            raise SetupError("SRS.generate: tau, alpha and beta must be in (0, r)")
        srs = cls(log_n)
        s = srs._bind()
        _check(lib().zk_srs_generate(C.c_void_p(ctx._h), C.c_uint32(srs.log_n), C.byref(_fr(vals[0])),
                                     C.byref(_fr(vals[1])), C.byref(_fr(vals[2])), C.byref(s)), ctx, "zk_srs_generate")
        srs.beta_g2 = np.array(s.beta_g2.w, dtype=np.uint64)
        return srs

    def verify(self, ctx, coeffs=None):
        """zk_srs_verify: is this a well-formed string? -> (ok, status), status
        the first ZK_SRS_* check that fails (SHAPE, POINT, GENERATOR, POWERS_G1,
        POWERS_G2, ALPHA, BETA) or ZK_SRS_OK.  coeffs: 2N non-zero integers below
        2^128; None draws them from `secrets`, which is what a real check uses.
        It does not check any contributor's proof of knowledge.  ValueError for
        a bad coefficient."""
        N = 1 << self.log_n
        if coeffs is None:
            import secrets
            coeffs = []
            for _ in range(2 * N):
                c = 0
                while not c:      # uniform on [1, 2^128)
                    c = secrets.randbits(128)
                coeffs.append(c)
        coeffs = [int(c) for c in coeffs]
        if any(not 0 < c < (1 << 128) for c in coeffs):
            raise ValueError("SRS.verify: every coefficient must be non-zero and below 2^128")
        co = _fr_rows(coeffs) if len(coeffs) else np.zeros((0, 4), dtype=np.uint64)
        st = C.c_int(-1)
        rc = lib().zk_srs_verify(C.c_void_p(ctx._h), C.byref(self._bind()), _p(co) if len(co) else None,
                                 C.c_size_t(len(co)), C.byref(st))
        _check(rc, ctx, "zk_srs_verify")
        return st.value == ZK_SRS_OK, st.value

    def contribute(self, ctx, s, a, b):
        """zk_srs_contribute: one phase-1 contribution with the secret shares
        0 < s, a, b < r -> (new_srs, share); this string is left untouched.
        Entry i of tau_g1 and tau_g2 times s^i, of alpha_tau_g1 times a s^i, of
        beta_tau_g1 times b s^i (on the GPU), beta_g2 times b: the string
        generate gives for (tau s, alpha a, beta b).  share: a (3, 25) array,
        [s]_2, [a]_2, [b]_2, what the contributor publishes for
        verify_contribution.  ValueError for a zero or out-of-range share,
        raised before the GPU is touched."""
        vals = [int(v) for v in (s, a, b)]
        if any(not 0 < v < R for v in vals):
            raise ValueError("SRS.contribute: s, a and b must be in (0, r)")
        new = self.copy()
        c = new._bind()
        sh = _SRSShare()
        _check(lib().zk_srs_contribute(C.c_void_p(ctx._h), C.byref(c), C.byref(_fr(vals[0])), C.byref(_fr(vals[1])),
                                       C.byref(_fr(vals[2])), C.byref(sh)), ctx, "zk_srs_contribute")
        new.beta_g2 = np.array(c.beta_g2.w, dtype=np.uint64)
        share = np.array([list(sh.tau_g2.w), list(sh.alpha_g2.w), list(sh.beta_g2.w)], dtype=np.uint64)
        return new, share

    @staticmethod
    def verify_contribution(ctx, before, after, share, coeffs=None):
        """zk_srs_verify_contribution: is the string `after` a contribution
        with the published `share` ((3, 25) words: [s]_2, [a]_2, [b]_2) on top of
        `before`? -> (ok, status, srs_status): status the first ZK_SRSC_* check
        that fails (SHAPE, SHARE, STRING, TAU, ALPHA, BETA) or ZK_SRSC_OK;
        srs_status what SRS.verify says of `after` (ZK_SRS_OK unless status is
        STRING).  coeffs as SRS.verify's (2N of them); None draws them from
        `secrets`, which is what a real check uses.  It does not prove that the
        contributor knows the shares.  ValueError for a bad coefficient."""
        N = 1 << after.log_n
        if coeffs is None:
            import secrets
            coeffs = []
            for _ in range(2 * N):
                c = 0
                while not c:      # uniform on [1, 2^128)
                    c = secrets.randbits(128)
                coeffs.append(c)
        coeffs = [int(c) for c in coeffs]
        if any(c < 0 or c >> 256 for c in coeffs):
            raise ValueError("SRS.verify_contribution: every coefficient must be non-zero and below 2^128")
        # whole values: a bad coefficient is the library's error
        co = (np.array([to_limbs(c) for c in coeffs], dtype=np.uint64).reshape(-1, 4) if len(coeffs)
              else np.zeros((0, 4), dtype=np.uint64))
        shw = np.ascontiguousarray(share, dtype=np.uint64).reshape(3, G2_WORDS)
        sh = _SRSShare()
        for f, row in zip((sh.tau_g2, sh.alpha_g2, sh.beta_g2), shw):
            for i, w in enumerate(row):
                f.w[i] = int(w)
        st, sst = C.c_int(-1), C.c_int(-1)
        rc = lib().zk_srs_verify_contribution(C.c_void_p(ctx._h), C.byref(before._bind()), C.byref(after._bind()),
                                              C.byref(sh), _p(co) if len(co) else None, C.c_size_t(len(co)),
                                              C.byref(st), C.byref(sst))
        _check(rc, ctx, "zk_srs_verify_contribution")
        return st.value == ZK_SRSC_OK, st.value, sst.value

    # ---- contributions with proofs of knowledge ----
    def digest(self, ctx=None, version=1):
        """The challenge of the next contribution's proofs -> 32 bytes (layouts:
        include/zkp.h).  version 1: zk_srs_digest, one SHA-256 over the
        string's compressed points on the host (ctx is not used).  version 2:
        zk_srs_digest_v2, the tree digest -- leaves of 256 points hashed on
        the GPU when a ctx is given, by the host twin otherwise, the same
        bytes either way.  One ceremony uses one version."""
        out = np.zeros(32, dtype=np.uint8)
        if _digest_version(version, "SRS.digest") == 1:
            _check(lib().zk_srs_digest(C.byref(self._bind()), _p(out)), None, "zk_srs_digest")
        else:
            _check(lib().zk_srs_digest_v2(C.c_void_p(ctx._h) if ctx is not None else None, C.byref(self._bind()),
                                          _p(out)), ctx, "zk_srs_digest_v2")
        return out.tobytes()

    def contribute_proved(self, ctx, s, a, b, digest_version=1):
        """contribute(ctx, s, a, b) and the contributor's proofs that they know
        the shares -> (new_srs, share, proof): proof a (3, 38) array, the
        zk_pok of s, a, b with roles TAU, ALPHA, BETA and this string's
        digest as the challenge (digest_version 1: zk_srs_prove_contribution;
        2: pok_make over self.digest(ctx, 2), the tree digest)."""
        _digest_version(digest_version, "SRS.contribute_proved")
        new, share = self.contribute(ctx, s, a, b)
        if digest_version == 2:
            ch = self.digest(ctx, 2)
            return new, share, np.stack([pok_make(v, role, ch) for v, role in
                                         ((s, ZK_POK_TAU), (a, ZK_POK_ALPHA), (b, ZK_POK_BETA))])
        pr = _SRSProof()
        _check(lib().zk_srs_prove_contribution(C.byref(self._bind()), C.byref(_fr(s)), C.byref(_fr(a)),
                                               C.byref(_fr(b)), C.byref(pr)), None, "zk_srs_prove_contribution")
        proof = np.frombuffer(bytes(pr), dtype=np.uint64).reshape(3, POK_WORDS).copy()
        return new, share, proof

    @staticmethod
    def verify_contribution_proofs(ctx, digests, shares, proofs):
        """zk_srs_verify_contribution_proofs, the transcript check of m
        contributions: digests m x 32 bytes (the digest of the string each
        started from), shares (m, 3, 25) words, proofs (m, 3, 38) words ->
        an (m, 3) uint8 array of ZK_POK_* statuses (tau, alpha, beta).  Per
        proof: zk_pok_verify_many's check and the link to the published
        share, both on the GPU.  It does not replace verify_contribution."""
        sh = np.ascontiguousarray(shares, dtype=np.uint64).reshape(-1, 3, G2_WORDS)
        pr = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 3, POK_WORDS)
        m = len(pr)
        dg = _challenges(digests, m)
        if len(sh) != m:
            raise ValueError("verify_contribution_proofs: one digest, share and proof per contribution")
        st = np.zeros((m, 3), dtype=np.uint8)
        rc = lib().zk_srs_verify_contribution_proofs(C.c_void_p(ctx._h), _p(dg) if m else None, _p(sh) if m else None,
                                                     _p(pr) if m else None, C.c_size_t(m), _p(st) if m else None)
        _check(rc, ctx, "zk_srs_verify_contribution_proofs")
        return st

    # ---- prepared strings ----
    def prepare(self, ctx, log_n=None):
        """zk_srs_prepare: the Lagrange form of this string for the domain
        2^log_n (default: the string's own), resident on the device -> a
        PreparedSRS.  The four inverse group transforms run here, once;
        CRS.from_prepared / from_prepared_device then make the key of any
        circuit of that size from column sums alone.  DomainTooSmall for a
        log_n above the string's, SetupError for tau on that domain."""
        log_n = self.log_n if log_n is None else int(log_n)
        if not 0 <= log_n <= 31:
            raise DomainTooSmall(f"a domain of 2^{log_n} does not exist (log_n in [0, 31])")
        h = C.c_void_p()
        _check(lib().zk_srs_prepare(C.c_void_p(ctx._h), C.byref(self._bind()), C.c_uint32(log_n), C.byref(h)), ctx,
               "zk_srs_prepare")
        return PreparedSRS(ctx, h.value)


class PreparedSRS:
    """A prepared powers-of-tau string in HBM (zk_srs_dev): [L_i]_1,
    [alpha L_i]_1, [beta L_i]_1, [L_i]_2 and the h_g1 differences for ONE
    domain size, read-only.  From SRS.prepare or LagrangeSRS.upload."""

    def __init__(self, ctx, handle):
        self.ctx, self._h = ctx, handle

    @property
    def log_n(self):
        v = C.c_uint32()
        _check(lib().zk_srs_dev_log_n(C.c_void_p(self._h), C.byref(v)), None, "zk_srs_dev_log_n")
        return v.value

    @property
    def domain_size(self):
        return 1 << self.log_n

    @property
    def device_bytes(self):
        """zk_srs_dev_bytes: device memory the handle holds."""
        v = C.c_uint64()
        _check(lib().zk_srs_dev_bytes(C.c_void_p(self._h), C.byref(v)), None, "zk_srs_dev_bytes")
        return v.value

    def export(self):
        """zk_srs_dev_export -> a LagrangeSRS of canonical host points."""
        lag = LagrangeSRS(self.log_n)
        s = lag._bind()
        _check(lib().zk_srs_dev_export(C.c_void_p(self.ctx._h), C.c_void_p(self._h), C.byref(s)), self.ctx,
               "zk_srs_dev_export")
        for nm in ("alpha_g1", "beta_g1", "beta_g2"):
            setattr(lag, nm, np.array(getattr(s, nm).w, dtype=np.uint64))
        return lag

    def free(self):
        if getattr(self, "_h", None):
            lib().zk_srs_dev_free(C.c_void_p(self._h))
            self._h = None

    def __del__(self):
        self.free()


class LagrangeSRS:
    """A prepared string on the host (zk_srs_lagrange), n = 2^log_n entries per
    array: l_g1, alpha_l_g1, beta_l_g1, h_g1 (n, 13) and l_g2 (n, 25) words,
    alpha_g1, beta_g1 (13) and beta_g2 (25).  upload() takes it as it is;
    verify() is what tells whether it belongs to a string."""

    _ARRAYS = ("l_g1", "alpha_l_g1", "beta_l_g1", "h_g1", "l_g2")

    def __init__(self, log_n):
        self.log_n = int(log_n)
        if not 0 <= self.log_n <= 31:
            raise DomainTooSmall(f"a domain of 2^{self.log_n} does not exist (log_n in [0, 31])")
        n = 1 << self.log_n
        for nm in self._ARRAYS:
            setattr(self, nm, np.zeros((n, G2_WORDS if nm == "l_g2" else G1_WORDS), dtype=np.uint64))
        self.alpha_g1 = np.zeros(G1_WORDS, dtype=np.uint64)
        self.beta_g1 = np.zeros(G1_WORDS, dtype=np.uint64)
        self.beta_g2 = np.zeros(G2_WORDS, dtype=np.uint64)
        self.s = _SRSLagrange()

    def _bind(self):
        s = self.s
        s.log_n = self.log_n
        ln = None
        for nm in self._ARRAYS:
            a = getattr(self, nm)
            if not (isinstance(a, np.ndarray) and a.dtype == np.uint64 and a.flags.c_contiguous):
                a = np.ascontiguousarray(a, dtype=np.uint64)
                setattr(self, nm, a)
            setattr(s, nm, a.ctypes.data)
            ln = len(a) if ln is None else min(ln, len(a))
        s.len = ln
        for nm in ("alpha_g1", "beta_g1", "beta_g2"):
            f = getattr(s, nm)
            for i, w in enumerate(np.asarray(getattr(self, nm), dtype=np.uint64).reshape(-1)):
                f.w[i] = int(w)
        return s

    def copy(self):
        """A prepared string with arrays of its own."""
        new = LagrangeSRS(self.log_n)
        for nm in self._ARRAYS + ("alpha_g1", "beta_g1", "beta_g2"):
            setattr(new, nm, np.array(getattr(self, nm), dtype=np.uint64, copy=True))
        return new

    def upload(self, ctx):
        """zk_srs_dev_import -> a PreparedSRS.  Only the shape is checked."""
        h = C.c_void_p()
        _check(lib().zk_srs_dev_import(C.c_void_p(ctx._h), C.byref(self._bind()), C.byref(h)), ctx,
               "zk_srs_dev_import")
        return PreparedSRS(ctx, h.value)

    def verify(self, ctx, srs, coeffs=None):
        """zk_srs_lagrange_verify: is this the prepared form of `srs` at this
        log_n? -> (ok, status), status the first ZK_LAG_* check that fails
        (SHAPE, POINT, FIXED, LAGRANGE_G1, ALPHA, BETA, LAGRANGE_G2, H) or
        ZK_LAG_OK.  coeffs: 2^log_n non-zero integers below 2^128; None draws
        them from `secrets`, which is what a real check uses -- a wrong entry
        then passes with probability about 2^-128.  No group transform runs:
        one scalar inverse transform and eight MSMs.  It takes the string as
        valid (SRS.verify).  ValueError for a bad coefficient or count."""
        n = 1 << self.log_n
        if coeffs is None:
            import secrets
            co = np.zeros((n, 4), dtype=np.uint64)      # uniform on [1, 2^128): zero rows are drawn again
            todo = np.arange(n)
            while len(todo):
                co[todo, :2] = np.frombuffer(secrets.token_bytes(16 * len(todo)), dtype=np.uint64).reshape(-1, 2)
                todo = todo[(co[todo, 0] | co[todo, 1]) == 0]
        else:
            coeffs = [int(c) for c in coeffs]
            if len(coeffs) != n:
                raise ValueError(f"LagrangeSRS.verify: {n} coefficients, one per entry")
            if any(not 0 < c < (1 << 128) for c in coeffs):
                raise ValueError("LagrangeSRS.verify: every coefficient must be non-zero and below 2^128")
            co = _fr_rows(coeffs)
        st = C.c_int(-1)
        rc = lib().zk_srs_lagrange_verify(C.c_void_p(ctx._h), C.byref(srs._bind()), C.byref(self._bind()), _p(co),
                                          C.c_size_t(len(co)), C.byref(st))
        _check(rc, ctx, "zk_srs_lagrange_verify")
        return st.value == ZK_LAG_OK, st.value


# -------------------------------------------------------------- prove ----
class Witness:
    """crates/groth16-core/src/lib.rs:40-131"""

    def __init__(self, assignment, num_public):
        a = assignment
        if not isinstance(a, np.ndarray):
            a = fr_array(a)
        a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
        if not fr_rows_canonical(a):
            raise ValueError("assignment holds a value >= r (not a canonical Fr)")
        if num_public >= len(a):
            raise InvalidWitness("Number of public inputs must be less than total assignment length")
        if len(a) == 0 or not (a[0, 0] == 1 and not a[0, 1:].any()):
            raise InvalidWitness("First element of assignment must be 1 (constant)")
        self.assignment = a
        self.num_public = num_public

    def public_inputs(self):
        """core:101-104"""
        return self.assignment[1:self.num_public + 1]

    def private_inputs(self):
        """core:106-109"""
        return self.assignment[self.num_public + 1:]


_R_LIMBS = np.array([(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def fr_rows_canonical(a):
    """Every row (4 little-endian u64 limbs) < r, vectorised."""
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
    lt = np.zeros(len(a), dtype=bool)
    eq = np.ones(len(a), dtype=bool)
    for i in (3, 2, 1, 0):
        lt |= eq & (a[:, i] < _R_LIMBS[i])
        eq &= a[:, i] == _R_LIMBS[i]
    return bool(lt.all())


class Proof:
    """crates/groth16-core/src/lib.rs:27-36 (a: G1, b: G2, c: G1)."""

    def __init__(self, words):
        self.words = np.asarray(words, dtype=np.uint64).reshape(-1)
        self.a = self.words[:G1_WORDS]
        self.b = self.words[G1_WORDS:G1_WORDS + G2_WORDS]
        self.c = self.words[G1_WORDS + G2_WORDS:]

    @classmethod
    def _from_c(cls, p):
        return cls(list(p.a.w) + list(p.b.w) + list(p.c.w))

    def _c(self):
        p = _Proof()
        for i in range(G1_WORDS):
            p.a.w[i] = int(self.a[i])
            p.c.w[i] = int(self.c[i])
        for i in range(G2_WORDS):
            p.b.w[i] = int(self.b[i])
        return p

    def serialize_compressed(self):
        """ark CanonicalSerialize (compressed) of Proof: 48 + 96 + 48 bytes."""
        out = (C.c_uint8 * 192)()
        _check(lib().zk_proof_serialize_compressed(C.byref(self._c()), out), None, "serialize")
        return bytes(out)

    @classmethod
    def deserialize_compressed(cls, data):
        """ark CanonicalDeserialize (compressed, validated); ValueError on bad bytes."""
        data = bytes(data)
        if len(data) != 192:
            raise ValueError("a compressed Proof is 192 bytes")
        buf = (C.c_uint8 * 192).from_buffer_copy(data)
        out = _Proof()
        _check(lib().zk_proof_deserialize_compressed(buf, C.byref(out)), None, "deserialize")
        return cls._from_c(out)

    def __eq__(self, other):
        return isinstance(other, Proof) and np.array_equal(self.words, other.words)


class Prover:
    """Prover::prove (crates/groth16-core/src/lib.rs:139-272).  `r` and `s`
    are the two Fr::rand draws of core:152-153; pass them explicitly (or an
    `rng` callable returning Fr ints, drawn r then s)."""

    @staticmethod
    def prove(dpk, witness, r=None, s=None, rng=None):
        if r is None or s is None:
            if rng is None:
                raise ValueError("pass r and s, or an rng")
            r, s = rng(), rng()
        ctx = dpk.ctx
        out = _Proof()
        z = witness.assignment
        rc = lib().zk_groth16_prove(C.c_void_p(ctx._h), C.c_void_p(dpk._h), _p(z), C.c_size_t(len(z)),
                                    C.c_size_t(witness.num_public), C.byref(_fr(r)), C.byref(_fr(s)),
                                    C.byref(out))
        _check(rc, ctx, "zk_groth16_prove")
        return Proof._from_c(out)

    @staticmethod
    def prove_device(dpk, d_z_ptr, zlen, num_public, r, s):
        """z already in HBM (canonical zk_fr array at device pointer d_z_ptr)."""
        ctx = dpk.ctx
        out = _Proof()
        rc = lib().zk_groth16_prove_dev(C.c_void_p(ctx._h), C.c_void_p(dpk._h), C.c_void_p(d_z_ptr),
                                        C.c_size_t(zlen), C.c_size_t(num_public), C.byref(_fr(r)),
                                        C.byref(_fr(s)), C.byref(out))
        _check(rc, ctx, "zk_groth16_prove_dev")
        return Proof._from_c(out)

    @staticmethod
    def prove_partial(dpk, d_z_ptr, zlen, num_public, r, s):
        """This GPU's shard of the MSMs -> opaque bytes for the all-gather."""
        ctx = dpk.ctx
        buf = (C.c_uint8 * PARTIAL_BYTES)()
        rc = lib().zk_groth16_prove_partial(C.c_void_p(ctx._h), C.c_void_p(dpk._h), C.c_void_p(d_z_ptr),
                                            C.c_size_t(zlen), C.c_size_t(num_public), C.byref(_fr(r)),
                                            C.byref(_fr(s)), buf)
        _check(rc, ctx, "zk_groth16_prove_partial")
        return bytes(buf)

    @staticmethod
    def prove_partial_host(dpk, z_slice, zlen, num_public, r, s):
        """This GPU's shard of the proof from a HOST witness slice (only the
        entries of dpk.witness_ranges(), concatenated: dpk.witness_slice(z));
        zlen = length of the whole witness."""
        ctx = dpk.ctx
        zs = np.ascontiguousarray(z_slice, dtype=np.uint64).reshape(-1, 4)
        buf = (C.c_uint8 * PARTIAL_BYTES)()
        rc = lib().zk_groth16_prove_partial_host(C.c_void_p(ctx._h), C.c_void_p(dpk._h), _p(zs) if len(zs) else None,
                                                 C.c_size_t(len(zs)), C.c_size_t(zlen), C.c_size_t(num_public),
                                                 C.byref(_fr(r)), C.byref(_fr(s)), buf)
        _check(rc, ctx, "zk_groth16_prove_partial_host")
        return bytes(buf)

    @staticmethod
    def prove_virtual_shards(dpks, d_z_ptr, zlen, num_public, r, s):
        """Diagnostic: the distributed quotient + sharded MSMs of len(dpks)
        virtual ranks on one device (zk_test_prove_virtual_shards)."""
        ctx = dpks[0].ctx
        arr = (C.c_void_p * len(dpks))(*[C.c_void_p(d._h) for d in dpks])
        out = _Proof()
        rc = test_lib().zk_test_prove_virtual_shards(C.c_void_p(ctx._h), arr, C.c_uint32(len(dpks)),
                                                C.c_void_p(d_z_ptr), C.c_size_t(zlen), C.c_size_t(num_public),
                                                C.byref(_fr(r)), C.byref(_fr(s)), C.byref(out))
        _check(rc, ctx, "zk_test_prove_virtual_shards")
        return Proof._from_c(out)

    @staticmethod
    def combine(partials, r, s):
        k = len(partials)
        arr = (C.c_uint8 * (PARTIAL_BYTES * k)).from_buffer_copy(b"".join(partials))
        out = _Proof()
        rc = lib().zk_groth16_prove_combine(arr, C.c_size_t(k), C.byref(_fr(r)), C.byref(_fr(s)),
                                            C.byref(out))
        _check(rc, None, "zk_groth16_prove_combine")
        return Proof._from_c(out)


class TorchExchange:
    """Host-staged exchange over a torch.distributed process group (CPU
    tensors: gloo), for Context.attach_exchange: the distributed quotient's
    three all-to-alls as all_to_all_single, the status agreement as a MAX
    all-reduce.  abort() tears the group down (the default group unless one
    is given), so peers blocked in a transfer with this rank fail instead of
    waiting out the group's timeout."""

    def __init__(self, group=None):
        import torch.distributed as dist
        self.dist, self.group, self.dead = dist, group, False

    def all_to_all(self, send_ptr, recv_ptr, chunk_bytes):
        import torch
        if self.dead:
            raise ExchangeError("TorchExchange: aborted")
        nbytes = chunk_bytes * self.dist.get_world_size(self.group)
        send = torch.frombuffer((C.c_uint8 * nbytes).from_address(send_ptr), dtype=torch.uint8)
        recv = torch.frombuffer((C.c_uint8 * nbytes).from_address(recv_ptr), dtype=torch.uint8)
        self.dist.all_to_all_single(recv, send, group=self.group)

    def all_reduce_max(self, value):
        import torch
        if self.dead:
            raise ExchangeError("TorchExchange: aborted")
        t = torch.tensor([value], dtype=torch.int64)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX, group=self.group)
        return int(t.item())

    def abort(self):
        if self.dist.is_initialized():
            self.dist.destroy_process_group(self.group)
        self.group, self.dead = None, True   # the last reference: the group's connections close with it


# ------------------------------------------------------------- verify ----
def _fr_rows(values):
    a = values if isinstance(values, np.ndarray) else fr_array(values)
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)


def pairing_product_is_one(g1_points, g2_points):
    """prod e(P_i, Q_i) == 1 (Bls12_381::multi_pairing(..).is_zero(), core:352)."""
    a = np.ascontiguousarray(g1_points, dtype=np.uint64).reshape(-1, G1_WORDS)
    b = np.ascontiguousarray(g2_points, dtype=np.uint64).reshape(-1, G2_WORDS)
    if len(a) != len(b):
        raise ValueError("as many G1 as G2 points")
    out = C.c_int(0)
    _check(lib().zk_pairing_product_is_one(_p(a), _p(b), C.c_size_t(len(a)), C.byref(out)), None, "pairing")
    return bool(out.value)


class Verifier:
    """Verifier::verify (crates/groth16-core/src/lib.rs:308-355), on the host.
    A sound vk (vk.sound) goes through zk_groth16_verify_sound /
    zk_groth16_verify_many_sound: the whole public inputs, one >= r a
    ValueError.  verify_many and verify_many_bytes take a
    PreparedVerificationKey (vk.prepare(ctx)) in place of vk: same results,
    same exceptions, the key's tables made once."""

    @staticmethod
    def verify(vk, proof, public_inputs):
        inp = _fr_rows(public_inputs)
        valid = C.c_int(0)
        fn = lib().zk_groth16_verify_sound if getattr(vk, "sound", False) else lib().zk_groth16_verify
        rc = fn(C.byref(vk.s), C.byref(proof._c()), _p(inp) if len(inp) else None, C.c_size_t(len(inp)),
                C.byref(valid))
        _check(rc, None, "zk_groth16_verify")
        return bool(valid.value)

    @staticmethod
    def verify_many(vk, proofs_and_inputs, ctx=None):
        """n independent verify() calls against one vk on the GPU
        (Context.verify_many) -> bool array, entry k what verify(vk,
        *proofs_and_inputs[k]) returns.  ValueError naming the first
        malformed proof, InvalidWitness on an input-count mismatch."""
        ctx = ctx or default_context()
        rows = [_fr_rows(inp) for _, inp in proofs_and_inputs]
        if any(len(r) != vk.num_public for r in rows):
            raise InvalidWitness("verify_many: a proof's public inputs do not match vk.num_public")
        inp = np.zeros((len(rows), vk.num_public, 4), dtype=np.uint64)
        for k, r in enumerate(rows):
            inp[k] = r
        sound = getattr(vk, "sound", False)
        st = ctx.verify_many(vk, [p for p, _ in proofs_and_inputs], inp, sound=sound)
        bad = np.flatnonzero(st == ZK_VERIFY_MALFORMED)
        if len(bad):
            raise ValueError(f"verify_many: proof {int(bad[0])} has a point that is not canonical or not on its curve"
                             + (", or a public input that is not below r" if sound else ""))
        return st == ZK_VERIFY_ACCEPT

    @staticmethod
    def verify_many_bytes(vk, proofs_and_inputs, ctx=None):
        """verify_many on compressed proofs: proofs_and_inputs is n pairs
        (192 bytes, public inputs); decode, subgroup check and pairing check
        run on the GPU (Context.verify_many_bytes) -> bool array, entry k what
        verify(vk, Proof.deserialize_compressed(bytes_k), inputs_k) returns.
        ValueError naming the first malformed proof, its failing point and
        why; InvalidWitness on an input-count mismatch."""
        ctx = ctx or default_context()
        rows = [_fr_rows(inp) for _, inp in proofs_and_inputs]
        if any(len(r) != vk.num_public for r in rows):
            raise InvalidWitness("verify_many_bytes: a proof's public inputs do not match vk.num_public")
        if any(len(b) != PROOF_BYTES for b, _ in proofs_and_inputs):
            raise ValueError(f"verify_many_bytes: a compressed Proof is {PROOF_BYTES} bytes")
        inp = np.zeros((len(rows), vk.num_public, 4), dtype=np.uint64)
        for k, r in enumerate(rows):
            inp[k] = r
        sound = getattr(vk, "sound", False)
        st, pst = ctx.verify_many_bytes(vk, b"".join(bytes(b) for b, _ in proofs_and_inputs), inp, sound=sound,
                                        point_status=True)
        bad = np.flatnonzero(st == ZK_VERIFY_MALFORMED)
        if len(bad):
            k = int(bad[0])
            pts = np.flatnonzero(pst[k])
            if len(pts):
                j = int(pts[0])
                raise ValueError(f"verify_many_bytes: proof {k} point {'abc'[j]}: {POINT_STATUS_TEXT[pst[k][j]]}")
            raise ValueError(f"verify_many_bytes: proof {k} has a public input that is not below r")
        return st == ZK_VERIFY_ACCEPT


    @staticmethod
    def _all_args(vk, proofs_and_inputs, coeffs, what):
        if not getattr(vk, "sound", False):
            raise ValueError(f"{what}: sound keys only (the reference mode has no sound batching, DESIGN.md 2.9)")
        rows = [_fr_rows(inp) for _, inp in proofs_and_inputs]
        if any(len(r) != vk.num_public for r in rows):
            raise InvalidWitness(f"{what}: a proof's public inputs do not match vk.num_public")
        inp = np.zeros((len(rows), vk.num_public, 4), dtype=np.uint64)
        for k, r in enumerate(rows):
            inp[k] = r
        if coeffs is None:
            import secrets
            coeffs = []
            for _ in rows:
                c = 0
                while not c:      # uniform on [1, 2^128)
                    c = secrets.randbits(128)
                coeffs.append(c)
        return inp, coeffs

    @staticmethod
    def verify_all(vk, proofs_and_inputs, ctx=None, coeffs=None):
        """"Are all n proofs valid?" for a sound vk with one pairing check on
        the GPU (Context.verify_all) -> bool.  coeffs=None draws one non-zero
        128-bit coefficient per proof from `secrets`: a batch with invalid
        proofs then passes with probability ~2^-127 at most, and a batch with
        exactly one never.  It does not say which proof is invalid
        (verify_many does).  ValueError naming the first malformed proof
        (which here includes a point outside the prime-order subgroup),
        InvalidWitness on an input-count mismatch, ValueError for a vk that
        is not sound."""
        ctx = ctx or default_context()
        inp, coeffs = Verifier._all_args(vk, proofs_and_inputs, coeffs, "verify_all")
        valid, bad = ctx.verify_all(vk, [p for p, _ in proofs_and_inputs], inp, coeffs)
        if bad < len(proofs_and_inputs):
            raise ValueError(f"verify_all: proof {bad} has a point that is not canonical or not on its curve"
                             ", or a public input that is not below r, or a point outside the prime-order subgroup")
        return valid

    @staticmethod
    def verify_all_bytes(vk, proofs_and_inputs, ctx=None, coeffs=None):
        """verify_all on compressed proofs: n pairs (192 bytes, public inputs)
        -> bool.  ValueError naming the first malformed proof, its failing
        point and why, as verify_many_bytes."""
        ctx = ctx or default_context()
        inp, coeffs = Verifier._all_args(vk, proofs_and_inputs, coeffs, "verify_all_bytes")
        if any(len(b) != PROOF_BYTES for b, _ in proofs_and_inputs):
            raise ValueError(f"verify_all_bytes: a compressed Proof is {PROOF_BYTES} bytes")
        valid, k, pst = ctx.verify_all_bytes(vk, b"".join(bytes(b) for b, _ in proofs_and_inputs), inp, coeffs,
                                             point_status=True)
        if k < len(proofs_and_inputs):
            pts = np.flatnonzero(pst[k])
            if len(pts):
                j = int(pts[0])
                raise ValueError(f"verify_all_bytes: proof {k} point {'abc'[j]}: {POINT_STATUS_TEXT[pst[k][j]]}")
            raise ValueError(f"verify_all_bytes: proof {k} has a public input that is not below r")
        return valid


class BatchVerifier:
    """BatchVerifier::verify_batch (core:360-432).  The reference draws one
    Fr::rand coefficient per proof; pass them as `coeffs` (or an `rng`
    callable returning Fr ints)."""

    @staticmethod
    def verify_batch(vk, proofs_and_inputs, coeffs=None, rng=None):
        if getattr(vk, "sound", False):
            # the reference's one-bit rule is no sound batching in any mode
            raise ValueError("BatchVerifier is reference-only: verify a sound key's proofs with Verifier.verify_all "
                             "(one verdict for the batch) or Verifier.verify_many (one per proof)")
        k = len(proofs_and_inputs)
        if coeffs is None:
            if k and rng is None:
                raise ValueError("pass coeffs, or an rng")
            coeffs = [rng() for _ in range(k)]
        proofs = (_Proof * max(k, 1))()
        rows = [_fr_rows(inp) for _, inp in proofs_and_inputs]
        ptrs = (C.c_void_p * max(k, 1))(*[C.c_void_p(r.ctypes.data) for r in rows])
        lens = (C.c_size_t * max(k, 1))(*[len(r) for r in rows])
        for i, (pr, _) in enumerate(proofs_and_inputs):
            proofs[i] = pr._c()
        co = _fr_rows(coeffs) if k else np.zeros((1, 4), dtype=np.uint64)
        valid = C.c_int(0)
        rc = lib().zk_groth16_verify_batch(C.byref(vk.s), proofs, ptrs, lens, C.c_size_t(k), _p(co),
                                           C.byref(valid))
        _check(rc, None, "zk_groth16_verify_batch")
        return bool(valid.value)


# ------------------------------------------------------- file formats ----
# Binary key files (the reference's CLI writes JSON placeholders instead:
# crates/groth16-cli/src/lib.rs:157-219).  Little-endian, canonical affine
# words exactly as they cross the C ABI (13 u64 per G1, 25 per G2), so a
# 2^24-constraint key (~24 GB) streams through numpy without conversion.
#   proving key:  b"ZKAMDPK1", u64 x 9 (V, n, num_public, num_constraints,
#                 a_len, b_len, b2_len, ic_len, h_len), alpha_g1, beta_g1,
#                 delta_g1, beta_g2, delta_g2, the five base vectors, then the
#                 QAP (setup:51) as CSR: per matrix u64 nnz, u64 has_val,
#                 rowptr[nc+1] u64, col[nnz] u32 (+4 pad bytes if nnz odd),
#                 val[nnz x 4] u64 when has_val
#   verification key: b"ZKAMDVK1", u64 num_public, ic_len, alpha_g1,
#                 beta_g2, gamma_g2, delta_g2, ic_g1[ic_len]
#   proof:        the 192-byte ark compressed encoding (Proof::serialize_compressed)
# Compressed key files hold every point in the ark / zcash compressed encoding
# (48 bytes per G1, 96 per G2 point: under half the size) and are decompressed
# -- which validates every point -- on the GPU when they are loaded:
#   proving key:  b"ZKAMDPK2", the same u64 x 9 header, alpha_g1, beta_g1,
#                 delta_g1 (48 bytes each), beta_g2, delta_g2 (96 each), a_g1,
#                 b_g1, b_g2, ic_g1, h_g1 compressed, zero bytes up to a
#                 multiple of 8, then the CSR section byte for byte as above
#   verification key: b"ZKAMDVK2", u64 num_public, ic_len, alpha_g1 (48),
#                 beta_g2, gamma_g2, delta_g2 (96 each), ic_g1 compressed
# A sound key (key.sound) is written with its own magic -- b"ZKAMDPS1" /
# b"ZKAMDPS2", verification key b"ZKAMDVS1" / b"ZKAMDVS2" -- over the very
# same layouts, and load_* sets .sound from it: a key cannot change mode by
# being saved and loaded.
_PK_MAGIC, _VK_MAGIC = b"ZKAMDPK1", b"ZKAMDVK1"
_PK2_MAGIC, _VK2_MAGIC = b"ZKAMDPK2", b"ZKAMDVK2"
_PKS_MAGIC, _VKS_MAGIC = b"ZKAMDPS1", b"ZKAMDVS1"
_PKS2_MAGIC, _VKS2_MAGIC = b"ZKAMDPS2", b"ZKAMDVS2"
# magic -> (compressed, sound)
_PK_MAGICS = {_PK_MAGIC: (False, False), _PK2_MAGIC: (True, False), _PKS_MAGIC: (False, True),
              _PKS2_MAGIC: (True, True)}
_VK_MAGICS = {_VK_MAGIC: (False, False), _VK2_MAGIC: (True, False), _VKS_MAGIC: (False, True),
              _VKS2_MAGIC: (True, True)}


def _magic_of(table, compressed, sound):
    return next(m for m, v in table.items() if v == (bool(compressed), bool(sound)))


def _u64s(f, k):
    a = np.fromfile(f, dtype="<u8", count=k)
    if len(a) != k:
        raise ValueError("truncated key file")
    return a


def _read_exact(f, k):
    b = f.read(k)
    if len(b) != k:
        raise ValueError("truncated key file")
    return b


def _write_compressed(f, key, table):
    for nm, group, single in table:
        words = key.point(nm) if single else getattr(key, nm)
        f.write((compress_g1 if group == 1 else compress_g2)(words))


def _read_compressed(f, path, ctx, table, counts):
    """The compressed points of a key file, table order -> affine words per
    field, decompressed (and so validated) on the GPU."""
    fields = [(nm, group, _read_exact(f, k * (G1_BYTES if group == 1 else G2_BYTES)))
              for (nm, group, _), k in zip(table, counts)]
    try:
        return _check_fields(ctx or default_context(), fields, True)
    except InvalidPoint as e:
        raise ValueError(f"{path}: {e}") from None


def save_proving_key(pk, path, compressed=False):
    with open(path, "wb") as f:
        f.write(_magic_of(_PK_MAGICS, compressed, getattr(pk, "sound", False)))
        csr = pk.qap.csr
        np.array([pk.qap.num_variables, pk.qap.domain_size, pk.num_public, csr.num_constraints,
                  len(pk.a_g1), len(pk.b_g1), len(pk.b_g2), len(pk.ic_g1), len(pk.h_g1)], dtype="<u8").tofile(f)
        if compressed:
            _write_compressed(f, pk, _PK_FIELDS)
            f.write(b"\0" * (-f.tell() % 8))
        else:
            for nm in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2"):
                pk.point(nm).astype("<u8").tofile(f)
            for arr in (pk.a_g1, pk.b_g1, pk.b_g2, pk.ic_g1, pk.h_g1):
                np.ascontiguousarray(arr, dtype="<u8").tofile(f)
        for rp, col, val in csr.mats:
            nnz = len(col)
            np.array([nnz, val is not None], dtype="<u8").tofile(f)
            np.ascontiguousarray(rp, dtype="<u8").tofile(f)
            np.ascontiguousarray(col, dtype="<u4").tofile(f)
            if nnz & 1:
                f.write(b"\0" * 4)
            if val is not None:
                np.ascontiguousarray(val, dtype="<u8").tofile(f)


def load_proving_key(path, ctx=None, validate=False):
    """Read a ZKAMDPK1 or ZKAMDPK2 file (picked by its magic; ZKAMDPS1 /
    ZKAMDPS2: the same layouts for a sound key, which sets .sound).  A compressed
    file is decompressed on the GPU of `ctx` (default_context() when None),
    which validates every point; an uncompressed one is read as it is, and
    checked by ProvingKey.validate(ctx) only with validate=True.  An invalid
    point raises ValueError("<path>: <field>[<index>]: <reason>")."""
    with open(path, "rb") as f:
        magic = f.read(8)
        if magic not in _PK_MAGICS:
            raise ValueError(f"{path}: not a proving key file")
        compressed, sound = _PK_MAGICS[magic]
        V, n, npub, nc, la, lb, lb2, lic, lh = (int(x) for x in _u64s(f, 9))
        if compressed:
            got = _read_compressed(f, path, ctx, _PK_FIELDS, (1, 1, 1, 1, 1, la, lb, lb2, lic, lh))
            pts, arrs = [a.reshape(-1) for a in got[:5]], got[5:]
            _read_exact(f, -f.tell() % 8)
        else:
            pts = [_u64s(f, G1_WORDS) for _ in range(3)] + [_u64s(f, G2_WORDS) for _ in range(2)]
            arrs = [_u64s(f, k * w).reshape(k, w) for k, w in
                    ((la, G1_WORDS), (lb, G1_WORDS), (lb2, G2_WORDS), (lic, G1_WORDS), (lh, G1_WORDS))]
        mats = []
        for _ in range(3):
            nnz, has_val = (int(x) for x in _u64s(f, 2))
            rp = _u64s(f, nc + 1).astype(np.uint64)
            col = np.fromfile(f, dtype="<u4", count=nnz).astype(np.uint32)
            if len(col) != nnz:
                raise ValueError("truncated key file")
            if nnz & 1:
                f.read(4)
            val = _u64s(f, 4 * nnz).reshape(nnz, 4).astype(np.uint64) if has_val else None
            mats.append((rp, col, val))
    qap = QAP(CSRMatrices(nc, V, mats))
    if qap.domain_size != n:
        raise ValueError("key domain does not match its constraint system")
    pk = ProvingKey(0, 0, npub, qap, sound)
    pk.a_g1, pk.b_g1, pk.b_g2, pk.ic_g1, pk.h_g1 = (np.ascontiguousarray(a, dtype=np.uint64) for a in arrs)
    for nm, words in zip(("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2"), pts):
        field = getattr(pk.s, nm)
        for i, w in enumerate(words):
            field.w[i] = int(w)
    if validate and not compressed:
        _validate_loaded(pk, path, ctx)
    return pk


def _validate_loaded(key, path, ctx):
    try:
        key.validate(ctx)
    except SetupError as e:
        raise ValueError(f"{path}: {e}") from None


def save_verification_key(vk, path, compressed=False):
    with open(path, "wb") as f:
        f.write(_magic_of(_VK_MAGICS, compressed, getattr(vk, "sound", False)))
        np.array([vk.num_public, len(vk.ic_g1)], dtype="<u8").tofile(f)
        if compressed:
            _write_compressed(f, vk, _VK_FIELDS)
            return
        for nm in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2"):
            vk.point(nm).astype("<u8").tofile(f)
        np.ascontiguousarray(vk.ic_g1, dtype="<u8").tofile(f)


def load_verification_key(path, ctx=None, validate=False):
    """Read a ZKAMDVK1 or ZKAMDVK2 file (ZKAMDVS1 / ZKAMDVS2: a sound key);
    see load_proving_key."""
    with open(path, "rb") as f:
        magic = f.read(8)
        if magic not in _VK_MAGICS:
            raise ValueError(f"{path}: not a verification key file")
        compressed, sound = _VK_MAGICS[magic]
        npub, lic = (int(x) for x in _u64s(f, 2))
        if compressed:
            got = _read_compressed(f, path, ctx, _VK_FIELDS, (1, 1, 1, 1, lic))
            pts, ic = [a.reshape(-1) for a in got[:4]], got[4]
        else:
            pts = [_u64s(f, G1_WORDS)] + [_u64s(f, G2_WORDS) for _ in range(3)]
            ic = _u64s(f, lic * G1_WORDS).reshape(lic, G1_WORDS)
    vk = VerificationKey.from_points(*pts, ic, sound=sound)
    vk.num_public = vk.s.num_public = npub
    if validate and not compressed:
        _validate_loaded(vk, path, ctx)
    return vk


# The reference CLI's serde JSON shapes (crates/groth16-cli/src/lib.rs:16-51):
# coefficients and values are hex strings ("0x" optional).
def _hex(v):
    return int(v, 16) % R


def r1cs_from_circuit_json(doc):
    """CircuitDescription {num_variables (without the constant), num_public,
    constraints: [{a, b, c: [[var, coeff_hex], ...]}]} -> R1CS."""
    cs = R1CS(int(doc["num_public"]))
    while cs.num_variables < int(doc["num_variables"]) + 1:
        cs.allocate_variable()
    for con in doc["constraints"]:
        lcs = [LinearCombination({int(v): _hex(c) for v, c in con[m]}) for m in "abc"]
        cs.enforce_multiplication(*lcs)
    return cs


def witness_from_json(doc):
    """WitnessData {assignment: [hex], num_public} -> Witness."""
    return Witness([_hex(x) for x in doc["assignment"]], int(doc["num_public"]))


def public_inputs_from_json(doc):
    """PublicInputs {inputs: [hex]} -> list of ints."""
    return [_hex(x) for x in doc["inputs"]]
