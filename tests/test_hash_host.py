"""The hash to G2 and the proofs of knowledge built on it, the parts that need
no GPU (include/zkp.h, "proofs of knowledge"; csrc/hash.hip's host code):
zk_sha256 against hashlib, zk_hash_to_g2_host against known answers and the
Python restatement (h2g2_ref.py), the cofactor clearing against [h_eff] P,
zk_pok_make / zk_pok_verify with every way a proof can be wrong, the digests
of a string and a key against a Python mirror, and the struct sizes."""
import ctypes
import hashlib

import numpy as np
import pytest

import h2g2_ref as H
import points_util as U
import sound_ref
import srs_util

# (msg, dst, tries, zk_g2_compress of the hash)
VECTORS = (
    (b"", b"", 1,
     "8c198a9669c9a6346a2b120052a03addbea79a8b479876edc42fc64402abdcc4ce85b2e8cfbf68e341aa597e9cf830b8"
     "02b97f680c98e3ee44d7eeba74bd6d68f2c4cbb9a5925fc08846004a3fe50a7f0ef9e59cd8f858e9de5ebc70f60b8032"),
    (bytes(64), b"test", 0,
     "839f3a1ffffa3490e585b9120effdea8e145528c13ddd877e46b1cf453f077b0ce76ed1b34e197c80bc38f3fab408d1e"
     "04eba9d0ed848a2119ab3b1d29b53f190e13338a133e6509e8d5a9e183eeb9e5a81fbc8c55096814b4d1891e4f55c640"),
    (bytes.fromhex("00000015") + bytes(60), b"test", 8,
     "a01b9b7ed0d24c3cdcc069a986378e51598111bec341799dd65e8295e78a8a9f7b053982e1e4842fa1f867891d62349f"
     "0a9536db27b0843d1d741fd139a9584baa4583237278eb2d28735980270fd792b1ee522ab9e39a0d99cee4ac2c70cc28"),
    (b"abc", b"ZKAMD-POK-V1", 0,
     "a538efa98e2c4786f0d2559992b0a8c0c3d0b9085a51370104c050a236ee8d8161d75f3dbefa8ba4c78b25bd9cebc7f3"
     "09c06b7f94d8591a5fcd08f26d7f5904ab570d79f0f9d5885da6cb958e5a141180cbc76e2e3ed30b8cf9f58ffcc05a85"),
)
CHALLENGE = hashlib.sha256(b"a state").digest()


def _g2_compress(zkp, words):
    w = np.ascontiguousarray(words, dtype=np.uint64).reshape(1, 25)
    out = np.zeros(96, dtype=np.uint8)
    assert zkp.lib().zk_g2_compress(zkp._p(w), ctypes.c_size_t(1), zkp._p(out)) == 0
    return out.tobytes()


# ------------------------------------------------------------------ SHA-256 ---
@pytest.mark.parametrize("n", [0, 1, 55, 56, 63, 64, 65, 119, 120, 1000])
def test_sha256(zkp, n):
    data = bytes((i * 7 + 3) & 0xFF for i in range(n))
    assert zkp.sha256(data) == hashlib.sha256(data).digest()


# ------------------------------------------------------------- hash to G2 ---
@pytest.mark.parametrize("k", range(len(VECTORS)))
def test_known_answers(zkp, pyref, k):
    msg, dst, tries, enc = VECTORS[k]
    words, got = zkp.hash_to_g2_host(msg, dst)
    assert got == tries
    assert _g2_compress(zkp, words).hex() == enc
    q, ref_tries = H.h2g2(msg, dst)                      # the restatement gives the same answers
    assert ref_tries == tries and pyref.g2_compress(q).hex() == enc


def test_host_against_reference(zkp, pyref):
    for msg in H.message_set(16):
        words, tries = zkp.hash_to_g2_host(msg, b"test")
        q, ref_tries = H.h2g2(msg, b"test")
        assert tries == ref_tries and list(words) == pyref.g2_words(q)


@pytest.mark.parametrize("dst", [b"", bytes(range(255))])
def test_dst_lengths(zkp, pyref, dst):
    words, tries = zkp.hash_to_g2_host(b"message", dst)
    q, ref_tries = H.h2g2(b"message", dst)
    assert tries == ref_tries and list(words) == pyref.g2_words(q)


def test_dst_too_long(zkp):
    with pytest.raises(ValueError):
        zkp.hash_to_g2_host(b"message", bytes(256))


def test_reference_try_counts():
    """the divergence case of the device tests: one wave whose lanes leave the
    try loop at seven different times"""
    counts = {}
    for msg in H.message_set(64):
        t = H.h2g2(msg, b"test")[1]
        counts[t] = counts.get(t, 0) + 1
    assert counts == {0: 28, 1: 22, 2: 6, 3: 4, 4: 2, 5: 1, 8: 1}


# -------------------------------------------------------- cofactor clearing ---
def test_clearing_is_h_eff(pyref):
    assert hex(H.H_EFF).startswith("0xbc69f08f") and hex(H.H_EFF).endswith("5aaa95551")
    for pt in U.g2_off_subgroup():
        q = H.clear_cofactor(pt)
        assert q == pyref.G2.mul(pt, H.H_EFF)
        assert pyref.G2.on_curve(q) and pyref.G2.mul(q, pyref.R) is pyref.INF


def test_outputs_in_subgroup(pyref):
    for msg, dst, _, _ in VECTORS:
        q = H.h2g2(msg, dst)[0]
        assert q is not pyref.INF and pyref.G2.on_curve(q) and pyref.G2.mul(q, pyref.R) is pyref.INF
    for msg in H.message_set(4):
        assert pyref.G2.mul(H.h2g2(msg, b"test")[0], pyref.R) is pyref.INF


# ------------------------------------------------------ proofs of knowledge ---
S = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % sound_ref.R


def _pok_ref(pyref, s, role, challenge):
    s_g1 = pyref.G1.mul(pyref.G1.gen, s)
    r = H.h2g2(H.pok_message(challenge, s_g1, role), H.POK_DST)[0]
    return s_g1, r


@pytest.mark.parametrize("role", range(4))
def test_pok_round_trip(zkp, pyref, role):
    pok = zkp.pok_make(S, role, CHALLENGE)
    s_g1, r = _pok_ref(pyref, S, role, CHALLENGE)
    assert list(pok[:13]) == pyref.g1_words(s_g1)
    assert list(pok[13:]) == pyref.g2_words(pyref.G2.mul(r, S))
    assert zkp.pok_verify(pok, role, CHALLENGE) == zkp.ZK_POK_OK


def test_pok_rejects(zkp, pyref):
    role = zkp.ZK_POK_ALPHA
    pok = zkp.pok_make(S, role, CHALLENGE)
    for other in (0, 2, 3):
        assert zkp.pok_verify(pok, other, CHALLENGE) == zkp.ZK_POK_REJECT
    for bit in (0, 255):
        ch = bytearray(CHALLENGE)
        ch[bit // 8] ^= 1 << (bit % 8)
        assert zkp.pok_verify(pok, role, bytes(ch)) == zkp.ZK_POK_REJECT
    s_g1, r = _pok_ref(pyref, S, role, CHALLENGE)
    bad = pok.copy()
    bad[:13] = pyref.g1_words(pyref.G1.add(s_g1, pyref.G1.gen))          # s_g1 <- [s + 1]_1
    assert zkp.pok_verify(bad, role, CHALLENGE) == zkp.ZK_POK_REJECT
    bad = pok.copy()
    bad[13:] = pyref.g2_words(pyref.G2.mul(r, S + 1))                    # s_r <- [s + 1] R
    assert zkp.pok_verify(bad, role, CHALLENGE) == zkp.ZK_POK_REJECT


def test_pok_bad_points(zkp, pyref):
    role = zkp.ZK_POK_TAU
    pok = zkp.pok_make(S, role, CHALLENGE)
    for lo, hi, words in ((0, 13, pyref.g1_words(pyref.INF)), (13, 38, pyref.g2_words(pyref.INF)),
                          (0, 13, pyref.g1_words(U.g1_off_subgroup()[1])),
                          (13, 38, pyref.g2_words(U.g2_off_subgroup()[0]))):
        bad = pok.copy()
        bad[lo:hi] = words
        assert zkp.pok_verify(bad, role, CHALLENGE) == zkp.ZK_POK_POINT


def test_pok_arguments(zkp):
    for s in (0, sound_ref.R):
        with pytest.raises(ValueError):
            zkp.pok_make(s, 0, CHALLENGE)
    with pytest.raises(ValueError):
        zkp.pok_make(S, 4, CHALLENGE)
    # the C calls themselves refuse the same
    fr = zkp._Fr()
    for i, x in enumerate(zkp.to_limbs(sound_ref.R)):
        fr.l[i] = x
    ch = np.frombuffer(CHALLENGE, dtype=np.uint8)
    out = zkp._Pok()
    L = zkp.lib()
    assert L.zk_pok_make(ctypes.byref(fr), ctypes.c_uint8(0), zkp._p(ch), ctypes.byref(out)) == zkp.ZK_ERR_ARG
    assert L.zk_pok_make(ctypes.byref(zkp._fr(0)), ctypes.c_uint8(0), zkp._p(ch), ctypes.byref(out)) == zkp.ZK_ERR_ARG
    assert L.zk_pok_make(ctypes.byref(zkp._fr(5)), ctypes.c_uint8(4), zkp._p(ch), ctypes.byref(out)) == zkp.ZK_ERR_ARG
    st = ctypes.c_int(-1)
    assert L.zk_pok_verify(ctypes.byref(out), ctypes.c_uint8(4), zkp._p(ch), ctypes.byref(st)) == zkp.ZK_ERR_ARG


# -------------------------------------------------------------------- digests ---
def _be64(v):
    return int(v).to_bytes(8, "big")


@pytest.fixture(scope="module")
def string2(zkp, pyref):
    """the log_n = 2 string of srs_util's case, made with pyref (no GPU)"""
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


def test_srs_digest(zkp, pyref, string2):
    srs, pts = string2
    h = hashlib.sha256(b"ZKAMD-SRS-V1" + _be64(2) + _be64(8) + _be64(4) + _be64(4) + _be64(4))
    for nm, enc in (("tau_g1", pyref.g1_compress), ("tau_g2", pyref.g2_compress),
                    ("alpha_tau_g1", pyref.g1_compress), ("beta_tau_g1", pyref.g1_compress)):
        for p in pts[nm]:
            h.update(enc(p))
    h.update(pyref.g2_compress(pts["beta_g2"]))
    assert srs.digest() == h.digest()
    other = srs.copy()
    other.alpha_tau_g1[3] = srs.alpha_tau_g1[2]
    assert other.digest() != srs.digest()
    other = srs.copy()
    other.beta_g2[:] = srs.tau_g2[1]
    assert other.digest() != srs.digest()


def test_key_digest(zkp, pyref):
    case = sound_ref.build_case()
    qap = zkp.QAP(zkp.CSRMatrices.synthetic(sound_ref.CASE_N))
    crs = zkp.CRS(sound_ref.pk_to_product(zkp, case["pk"], qap), sound_ref.vk_to_product(zkp, case["vk"]))
    pk, vk = case["pk"], case["vk"]
    h = hashlib.sha256(b"ZKAMD-KEY-V1")
    for n in (len(pk["a_g1"]), len(pk["b_g1"]), len(pk["b_g2"]), len(pk["ic_g1"]), len(pk["h_g1"]),
              pk["num_public"], len(vk["ic_g1"])):
        h.update(_be64(n))
    c1, c2 = pyref.g1_compress, pyref.g2_compress
    for enc, p in ((c1, pk["alpha_g1"]), (c1, pk["beta_g1"]), (c1, pk["delta_g1"]), (c2, pk["beta_g2"]),
                   (c2, pk["delta_g2"])):
        h.update(enc(p))
    for nm, enc in (("a_g1", c1), ("b_g1", c1), ("b_g2", c2), ("ic_g1", c1), ("h_g1", c1)):
        for p in pk[nm]:
            h.update(enc(p))
    h.update(c2(vk["gamma_g2"]))
    for p in vk["ic_g1"]:
        h.update(c1(p))
    assert crs.digest() == h.digest()
    other = crs.copy()
    other.pk.h_g1[1] = crs.pk.h_g1[0]
    assert other.digest() != crs.digest()
    other = crs.copy()
    other.vk.ic_g1[0] = crs.vk.ic_g1[1]
    assert other.digest() != crs.digest()


# --------------------------------------------------------------------- layout ---
def test_struct_sizes(zkp):
    assert ctypes.sizeof(zkp._Pok) == 104 + 200 == 8 * zkp.POK_WORDS
    assert ctypes.sizeof(zkp._SRSProof) == 3 * ctypes.sizeof(zkp._Pok)
    assert zkp._Pok.s_r.offset == 104 and zkp._SRSProof.beta.offset == 2 * 304
