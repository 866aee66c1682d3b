"""The V2 tree digests (include/zkp.h, "tree digests") restated in Python:
hashlib.sha256 over pyref's compressed encodings, independent of the library.
Shared by test_digest_v2_host.py and test_gpu_digest_v2.py, with the point
sets and the raw-word cases both of them run."""
import hashlib

import numpy as np

import pyref
import sound_ref
import srs_util

LEAF = 256
G1_COUNTS = (0, 1, 3, 4, 5, 255, 256, 257, 513)
G2_COUNTS = (0, 1, 2, 3, 255, 256, 257)
HALF = (pyref.P - 1) // 2


def _be64(v):
    return int(v).to_bytes(8, "big")


def leaf(g, encs):
    """encs: the 1..256 encodings of one leaf"""
    assert 1 <= len(encs) <= LEAF
    return hashlib.sha256(b"ZKAMD-LEAF-V2" + bytes([g]) + len(encs).to_bytes(2, "big") + bytes(48)
                          + b"".join(encs)).digest()


def leaves(g, encs):
    return b"".join(leaf(g, encs[lo:lo + LEAF]) for lo in range(0, len(encs), LEAF))


def leaves_of_bytes(g, data):
    """leaves over encodings given back to back (48 / 96 bytes each)"""
    k = 48 * g
    return leaves(g, [data[i:i + k] for i in range(0, len(data), k)])


def srs_v2(log_n, pts):
    """pts: tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1 (lists of pyref points), beta_g2"""
    c1, c2 = pyref.g1_compress, pyref.g2_compress
    h = hashlib.sha256(b"ZKAMD-SRS-V2" + _be64(log_n))
    for nm in ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1"):
        h.update(_be64(len(pts[nm])))
    h.update(c2(pts["beta_g2"]))
    for nm, g, enc in (("tau_g1", 1, c1), ("tau_g2", 2, c2), ("alpha_tau_g1", 1, c1), ("beta_tau_g1", 1, c1)):
        h.update(leaves(g, [enc(p) for p in pts[nm]]))
    return h.digest()


def key_v2(pk, vk):
    """pk, vk: sound_ref.build_case()'s dictionaries of pyref points"""
    c1, c2 = pyref.g1_compress, pyref.g2_compress
    h = hashlib.sha256(b"ZKAMD-KEY-V2")
    for n in (len(pk["a_g1"]), len(pk["b_g1"]), len(pk["b_g2"]), len(pk["ic_g1"]), len(pk["h_g1"]),
              pk["num_public"], len(vk["ic_g1"])):
        h.update(_be64(n))
    for enc, p in ((c1, pk["alpha_g1"]), (c1, pk["beta_g1"]), (c1, pk["delta_g1"]), (c2, pk["beta_g2"]),
                   (c2, pk["delta_g2"]), (c2, vk["gamma_g2"])):
        h.update(enc(p))
    for nm, g, enc in (("a_g1", 1, c1), ("b_g1", 1, c1), ("b_g2", 2, c2), ("ic_g1", 1, c1), ("h_g1", 1, c1)):
        h.update(leaves(g, [enc(p) for p in pk[nm]]))
    h.update(leaves(1, [c1(p) for p in vk["ic_g1"]]))
    return h.digest()


# ---- valid points: a few small multiples of the generators, reused cyclically ----
_BASE = {}


def base_points(g):
    """[(words, encoding)] of seven points, the identity among them"""
    if g not in _BASE:
        C, words, enc = ((pyref.G1, pyref.g1_words, pyref.g1_compress) if g == 1 else
                         (pyref.G2, pyref.g2_words, pyref.g2_compress))
        pts = [C.mul(C.gen, k) for k in (1, 2, 3, 5, 7, 11)]
        pts.insert(4, pyref.INF)
        _BASE[g] = [(words(p), enc(p)) for p in pts]
    return _BASE[g]


def cyclic(g, n):
    """n points -> ((n, 13 or 25) uint64 words, the restatement's leaf digests)"""
    base = base_points(g)
    idx = [i % len(base) for i in range(n)]
    words = np.array([base[i][0] for i in idx], dtype=np.uint64).reshape(n, 12 * g + 1)
    return words, leaves(g, [base[i][1] for i in idx])


# ---- raw words: what the encoder does with anything, valid or not ----
def _limbs(v, k=6):
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(k)]


JUNK = 0xA5A5A5A5_5A5A5A5A_DEADBEEF_01234567_89ABCDEF_FEDCBA98_76543210_0F1E2D3C_4B5A6978_8796A5B4_C3D2E1F0_11223344
X_TOP = (7 << 381) | 0x1234567   # the three bits the flags are OR-ed into, set in x itself


def raw_g1():
    """{name: 13 words}: rows of zk_g1_affine that no curve needs to hold"""
    x = 0x1357_9BDF << 300 | 0x2468
    return {
        "identity": _limbs(0) + _limbs(0) + [1],
        "identity_byte2_junk": _limbs(JUNK) + _limbs(JUNK >> 3) + [2],
        "pad_bytes_set": _limbs(x) + _limbs(5) + [0xFFFFFFFFFFFFFF00],   # the infinity BYTE is zero: a finite point
        "y_half": _limbs(x) + _limbs(HALF) + [0],
        "y_half_plus_1": _limbs(x) + _limbs(HALF + 1) + [0],
        "x_top_bits": _limbs(X_TOP) + _limbs(1) + [0],
        "x_top_bits_large_y": _limbs(X_TOP) + _limbs(pyref.P - 1) + [0],
        "y_not_canonical": _limbs(x) + _limbs((1 << 384) - 1) + [0],
    }


def raw_g2():
    """{name: 25 words}: x.c0, x.c1, y.c0, y.c1, infinity"""
    x0, x1 = 0xABCDEF << 200 | 0x77, 0x13579B << 330 | 0x99

    def pt(y0, y1, inf=0, xa=x0, xb=x1):
        return _limbs(xa) + _limbs(xb) + _limbs(y0) + _limbs(y1) + [inf]
    return {
        "identity": pt(0, 0, 1, 0, 0),
        "identity_byte2_junk": pt(JUNK >> 5, JUNK >> 7, 2, JUNK, JUNK >> 1),
        "c1_zero_c0_half": pt(HALF, 0),
        "c1_zero_c0_half_plus_1": pt(HALF + 1, 0),
        "c1_half_c0_large": pt(pyref.P - 1, HALF),          # c1 decides: not above half
        "c1_half_plus_1_c0_small": pt(1, HALF + 1),         # c1 decides: above half
        "c1_one_word": pt(pyref.P - 1, 1 << 320),           # c1 != 0 in one high word only
        "x_top_bits": pt(1, 1, 0, x0, X_TOP),
    }


def filler(g):
    """a finite valid point's words"""
    return base_points(g)[0][0]


# ---- the objects both test files digest ----
def string2(zkp):
    """the log_n = 2 string of srs_util's case, made with pyref (no GPU) ->
    (SRS, its points as pyref points)"""
    case = srs_util.case4(pyref)
    tau, alpha, beta, R = case["tau"], case["alpha"], case["beta"], pyref.R
    N = 4
    pts = {"tau_g1": [pyref.G1.mul(pyref.G1.gen, pow(tau, i, R)) for i in range(2 * N)],
           "tau_g2": [pyref.G2.mul(pyref.G2.gen, pow(tau, i, R)) for i in range(N)],
           "alpha_tau_g1": [pyref.G1.mul(pyref.G1.gen, alpha * pow(tau, i, R) % R) for i in range(N)],
           "beta_tau_g1": [pyref.G1.mul(pyref.G1.gen, beta * pow(tau, i, R) % R) for i in range(N)],
           "beta_g2": pyref.G2.mul(pyref.G2.gen, beta)}
    srs = zkp.SRS(2)
    for nm in ("tau_g1", "alpha_tau_g1", "beta_tau_g1"):
        getattr(srs, nm)[:] = [pyref.g1_words(p) for p in pts[nm]]
    srs.tau_g2[:] = [pyref.g2_words(p) for p in pts["tau_g2"]]
    srs.beta_g2[:] = pyref.g2_words(pts["beta_g2"])
    return srs, pts


def long_string(srs, pts):
    """string2 with tau_g1 and tau_g2 repeated past one leaf (514 and 257
    points; a digest does not ask that the lengths fit log_n)"""
    long = srs.copy()
    long.tau_g1 = np.array([srs.tau_g1[i % 8] for i in range(514)], dtype=np.uint64)
    long.tau_g2 = np.array([srs.tau_g2[i % 3] for i in range(257)], dtype=np.uint64)
    return long, dict(pts, tau_g1=[pts["tau_g1"][i % 8] for i in range(514)],
                      tau_g2=[pts["tau_g2"][i % 3] for i in range(257)])


def key(zkp):
    """sound_ref's shared case as a CRS -> (crs, the case's dictionaries)"""
    case = sound_ref.build_case()
    qap = zkp.QAP(zkp.CSRMatrices.synthetic(sound_ref.CASE_N))
    return zkp.CRS(sound_ref.pk_to_product(zkp, case["pk"], qap), sound_ref.vk_to_product(zkp, case["vk"])), case
