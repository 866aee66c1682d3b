"""The V2 tree digests without a GPU (include/zkp.h, "tree digests"; ctx == NULL
selects csrc/digest.hip's host twin): leaf digests, the string digest and the
key digest against the Python restatement (digest_v2_ref.py), raw struct words
against zk_g1_compress / zk_g2_compress followed by hashlib, and what a digest
must notice."""
import numpy as np
import pytest

import digest_v2_ref as D

NEW_EXPORTS = ("zk_g1_leaf_digests", "zk_g2_leaf_digests", "zk_srs_digest_v2", "zk_groth16_key_digest_v2_sound")


def test_exports(zkp):
    for name in NEW_EXPORTS:
        assert name in zkp.EXPORTS and hasattr(zkp.lib(), name)


# ------------------------------------------------------------------ leaves ---
@pytest.mark.parametrize("n", D.G1_COUNTS)
def test_g1_leaves(zkp, n):
    words, want = D.cyclic(1, n)
    got = zkp.g1_leaf_digests_host(words)
    assert got.shape == (-(-n // 256), 32) and got.tobytes() == want


@pytest.mark.parametrize("n", D.G2_COUNTS)
def test_g2_leaves(zkp, n):
    words, want = D.cyclic(2, n)
    got = zkp.g2_leaf_digests_host(words)
    assert got.shape == (-(-n // 256), 32) and got.tobytes() == want


def test_leaf_is_not_its_group_or_length(zkp):
    """the prefix: m and g are hashed, so a shorter leaf is no prefix of a longer
    one and equal bytes under the other group give another digest"""
    w, _ = D.cyclic(1, 4)
    assert zkp.g1_leaf_digests_host(w[:2]).tobytes() != zkp.g1_leaf_digests_host(w).tobytes()
    two_g1 = zkp.compress_g1(w[:2])
    assert D.leaf(1, [two_g1[:48], two_g1[48:]]) != D.leaf(2, [two_g1])


@pytest.mark.parametrize("name", sorted(D.raw_g1()))
def test_raw_g1(zkp, name):
    """one raw row among valid ones: the twin hashes whatever the encoder writes"""
    words = np.array([D.filler(1), D.raw_g1()[name], D.filler(1)], dtype=np.uint64)
    want = D.leaves_of_bytes(1, zkp.compress_g1(words))
    assert zkp.g1_leaf_digests_host(words).tobytes() == want


@pytest.mark.parametrize("name", sorted(D.raw_g2()))
def test_raw_g2(zkp, name):
    words = np.array([D.filler(2), D.raw_g2()[name], D.filler(2)], dtype=np.uint64)
    want = D.leaves_of_bytes(2, zkp.compress_g2(words))
    assert zkp.g2_leaf_digests_host(words).tobytes() == want


def test_raw_encodings_are_what_the_cases_say(zkp):
    """the raw cases do hit the encoder's branches (flags in byte 0)"""
    g1, g2 = D.raw_g1(), D.raw_g2()

    def b0(fn, row):
        return bytes(fn(np.array([row], dtype=np.uint64)))[0]
    c1, c2 = zkp.compress_g1, zkp.compress_g2
    assert bytes(c1(np.array([g1["identity_byte2_junk"]], dtype=np.uint64))) == b"\xc0" + bytes(47)
    assert bytes(c2(np.array([g2["identity_byte2_junk"]], dtype=np.uint64))) == b"\xc0" + bytes(95)
    assert b0(c1, g1["pad_bytes_set"]) & 0xC0 == 0x80
    assert b0(c1, g1["y_half"]) & 0x20 == 0 and b0(c1, g1["y_half_plus_1"]) & 0x20 == 0x20
    assert b0(c1, g1["x_top_bits"]) == 0xE0 and b0(c1, g1["x_top_bits_large_y"]) == 0xE0
    assert b0(c2, g2["c1_zero_c0_half"]) & 0x20 == 0 and b0(c2, g2["c1_zero_c0_half_plus_1"]) & 0x20 == 0x20
    assert b0(c2, g2["c1_half_c0_large"]) & 0x20 == 0 and b0(c2, g2["c1_half_plus_1_c0_small"]) & 0x20 == 0x20
    assert b0(c2, g2["c1_one_word"]) & 0x20 == 0


# ------------------------------------------------------------------ string ---
@pytest.fixture(scope="module")
def string2(zkp):
    return D.string2(zkp)


def test_srs_digest_v2(zkp, string2):
    srs, pts = string2
    d2 = srs.digest(version=2)
    assert d2 == D.srs_v2(2, pts)
    assert d2 != srs.digest() and srs.digest() == srs.digest(version=1)
    other = srs.copy()
    other.beta_g2[:] = srs.tau_g2[1]
    assert other.digest(version=2) != d2
    other = srs.copy()
    other.alpha_tau_g1[3] = srs.alpha_tau_g1[2]
    assert other.digest(version=2) != d2
    # equal points, other lengths: the header and the leaf prefix both move
    other = srs.copy()
    other.beta_tau_g1 = srs.beta_tau_g1[:3].copy()
    assert other.digest(version=2) != d2


def test_srs_digest_v2_long_arrays(zkp, string2):
    """arrays past one leaf (repeated points): against the restatement, and a
    swap of the two points either side of a leaf boundary"""
    srs, pts = string2
    long, lpts = D.long_string(srs, pts)
    d2 = long.digest(version=2)
    assert d2 == D.srs_v2(2, lpts)
    for nm, at in (("tau_g1", 256), ("tau_g1", 512), ("tau_g2", 256)):
        other = long.copy()
        a = getattr(other, nm)
        assert not np.array_equal(a[at - 1], a[at])
        a[[at - 1, at]] = a[[at, at - 1]]
        assert other.digest(version=2) != d2


def test_versions(zkp, string2):
    srs, _ = string2
    for v in (0, 3, "2", None):
        with pytest.raises(ValueError):
            srs.digest(version=v)
    with pytest.raises(ValueError):
        srs.contribute_proved(None, 1, 2, 3, digest_version=3)


def test_srs_digest_v2_arguments(zkp, string2):
    import ctypes as C
    srs, _ = string2
    out = np.zeros(32, dtype=np.uint8)
    L = zkp.lib()
    assert L.zk_srs_digest_v2(None, None, zkp._p(out)) == zkp.ZK_ERR_ARG
    assert L.zk_srs_digest_v2(None, C.byref(srs._bind()), None) == zkp.ZK_ERR_ARG
    s = srs.copy()._bind()
    s.tau_g2 = None
    assert L.zk_srs_digest_v2(None, C.byref(s), zkp._p(out)) == zkp.ZK_ERR_ARG
    w, _ = D.cyclic(1, 3)
    assert L.zk_g1_leaf_digests(None, None, C.c_size_t(3), zkp._p(out)) == zkp.ZK_ERR_ARG
    assert L.zk_g1_leaf_digests(None, zkp._p(w), C.c_size_t(3), None) == zkp.ZK_ERR_ARG
    assert L.zk_g2_leaf_digests(None, None, C.c_size_t(0), None) == zkp.ZK_OK


# --------------------------------------------------------------------- key ---
@pytest.fixture(scope="module")
def key(zkp):
    return D.key(zkp)


def test_key_digest_v2(zkp, key):
    crs, case = key
    d2 = crs.digest(version=2)
    assert d2 == D.key_v2(case["pk"], case["vk"])
    assert d2 != crs.digest() and crs.digest() == crs.digest(version=1)
    other = crs.copy()
    other.vk.ic_g1[0] = crs.vk.ic_g1[1]
    assert other.digest(version=2) != d2
    other = crs.copy()
    other.pk.h_g1[1] = crs.pk.h_g1[0]
    assert other.digest(version=2) != d2
    with pytest.raises(ValueError):
        crs.digest(version=3)
    with pytest.raises(ValueError):
        zkp.CRS.verify_contribution_proof(None, crs, crs, np.zeros(38, dtype=np.uint64), digest_version=3)


def test_key_digest_v2_arguments(zkp, key):
    import ctypes as C
    crs, _ = key
    out = np.zeros(32, dtype=np.uint8)
    L = zkp.lib()
    pk, vk = crs.pk._bind(), crs.vk.s
    assert L.zk_groth16_key_digest_v2_sound(None, None, C.byref(vk), zkp._p(out)) == zkp.ZK_ERR_ARG
    assert L.zk_groth16_key_digest_v2_sound(None, C.byref(pk), None, zkp._p(out)) == zkp.ZK_ERR_ARG
    assert L.zk_groth16_key_digest_v2_sound(None, C.byref(pk), C.byref(vk), None) == zkp.ZK_ERR_ARG
    assert L.zk_groth16_key_digest_v2_sound(None, C.byref(pk), C.byref(vk), zkp._p(out)) == zkp.ZK_OK
    assert out.tobytes() == crs.digest(version=2)


def test_proof_over_v2_is_pok_make(zkp, key):
    """no proof call of its own: a V2 proof is pok_make over the V2 challenge,
    and the other version's challenge rejects it (host check)"""
    crs, _ = key
    d = 0x1234567
    proof = zkp.pok_make(d, zkp.ZK_POK_DELTA, crs.digest(version=2))
    assert zkp.pok_verify(proof, zkp.ZK_POK_DELTA, crs.digest(version=2)) == zkp.ZK_POK_OK
    assert zkp.pok_verify(proof, zkp.ZK_POK_DELTA, crs.digest()) == zkp.ZK_POK_REJECT
