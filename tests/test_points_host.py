"""Compressed point arrays and compressed key files, host side (no GPU):
zk_g1_compress / zk_g2_compress against oracle/pyref.py's encoders and the
host decoder of the proof codec, and the ZKAMDPK2 / ZKAMDVK2 layouts."""
import numpy as np
import pytest

import points_util as PU
import pyref as P
from helpers import g1_words, g2_words, golden

G = golden()
CASES = [next(c for c in G["prove"] if c["name"] == nm) for nm in ("synthetic_8", "random_5x9_pub2")]


def _g1_of(p):
    return P.INF if p is None else (P.Fq1(int(p[0], 16)), P.Fq1(int(p[1], 16)))


def _g2_of(p):
    if p is None:
        return P.INF
    c = [int(v, 16) for v in p]
    return (P.Fq2(c[0], c[1]), P.Fq2(c[2], c[3]))


def _key_points(case):
    pk = case["pk"]
    g1 = [pk[nm] for nm in ("alpha_g1", "beta_g1", "delta_g1")]
    for nm in ("a_g1", "b_g1", "ic_g1", "h_g1"):
        g1 += pk[nm]
    return g1, [pk["beta_g2"], pk["delta_g2"]] + pk["b_g2"]


def test_compress_matches_pyref_on_golden_keys(zkp):
    for case in CASES:
        g1, g2 = _key_points(case)
        assert any(p is None for p in g1) and any(p is None for p in g2)   # identities among them
        got = zkp.compress_g1(np.array([g1_words(p) for p in g1], dtype=np.uint64))
        assert got == b"".join(P.g1_compress(_g1_of(p)) for p in g1), case["name"]
        got = zkp.compress_g2(np.array([g2_words(p) for p in g2], dtype=np.uint64))
        assert got == b"".join(P.g2_compress(_g2_of(p)) for p in g2), case["name"]


def test_compress_identity_and_both_signs(zkp):
    g1 = [P.INF] + [q for p in PU.g1_points(8) for q in (p, P.G1.neg(p))]
    g2 = [P.INF] + [q for p in PU.g2_points(8) for q in (p, P.G2.neg(p))]
    e1, e2 = zkp.compress_g1(PU.words_g1(g1)), zkp.compress_g2(PU.words_g2(g2))
    assert e1 == b"".join(P.g1_compress(p) for p in g1)
    assert e2 == b"".join(P.g2_compress(p) for p in g2)
    assert e1[:48] == bytes([0xC0]) + bytes(47) and e2[:96] == bytes([0xC0]) + bytes(95)
    # P and -P differ in the sort flag only
    for k in range(8):
        a, b = e1[48 * (1 + 2 * k):48 * (2 + 2 * k)], e1[48 * (2 + 2 * k):48 * (3 + 2 * k)]
        assert a[0] ^ b[0] == 0x20 and a[1:] == b[1:]
    # the host decoder gives the same words back
    for i, p in enumerate(g1):
        assert np.array_equal(PU.host_decode(zkp, e1[48 * i:48 * i + 48]), P.g1_words(p))
    for i, p in enumerate(g2):
        assert np.array_equal(PU.host_decode(zkp, e2[96 * i:96 * i + 96]), P.g2_words(p))


def test_compress_g2_sort_flag_falls_back_to_c0(zkp):
    """y.c1 == 0: the flag looks at y.c0.  Compression does not validate, so
    these words need not be points."""
    pts = [(P.Fq2(3, 5), P.Fq2(y0, 0)) for y0 in (1, PU.HALF, PU.HALF + 1, PU.PMOD - 1)]
    pts += [(P.Fq2(3, 5), P.Fq2(PU.PMOD - 1, y1)) for y1 in (PU.HALF, PU.HALF + 1)]
    enc = zkp.compress_g2(PU.words_g2(pts))
    assert enc == b"".join(P.g2_compress(p) for p in pts)
    assert [bool(enc[96 * i] & 0x20) for i in range(6)] == [False, False, True, True, False, True]


def test_compress_empty(zkp):
    assert zkp.compress_g1(np.zeros((0, 13), dtype=np.uint64)) == b""
    assert zkp.compress_g2(np.zeros((0, 25), dtype=np.uint64)) == b""


def _keys(zkp, case):
    import gpu_util as U
    qap = U.qap_from_case(zkp, case)
    pk = U.pk_from_golden(zkp, case, qap)
    vkd = case["vk"]
    vk = zkp.VerificationKey.from_points(g1_words(case["pk"]["alpha_g1"]), g2_words(case["pk"]["beta_g2"]),
                                         g2_words(vkd["gamma_g2"]), g2_words(case["pk"]["delta_g2"]),
                                         [g1_words(p) for p in vkd["ic_g1"]])
    return pk, vk


def test_compressed_key_file_layout(zkp, tmp_path):
    for case in CASES:
        pk, vk = _keys(zkp, case)
        p1, p2 = tmp_path / "k1.bin", tmp_path / "k2.bin"
        zkp.save_proving_key(pk, p1)
        zkp.save_proving_key(pk, p2, compressed=True)
        b1, b2 = p1.read_bytes(), p2.read_bytes()
        n1 = len(pk.a_g1) + len(pk.b_g1) + len(pk.ic_g1) + len(pk.h_g1)
        n2 = len(pk.b_g2)
        pts1 = 3 * 104 + 2 * 200 + 104 * n1 + 200 * n2
        pts2 = 3 * 48 + 2 * 96 + 48 * n1 + 96 * n2
        pts2 += -(80 + pts2) % 8
        csr = len(b1) - 80 - pts1
        assert len(b2) == 80 + pts2 + csr
        assert b2[:8] == b"ZKAMDPK2" and b1[:8] == b"ZKAMDPK1"
        assert b2[8:80] == b1[8:80]                       # the header
        assert b2[80 + pts2:] == b1[80 + pts1:]           # the CSR section
        assert b2[80:128] == P.g1_compress(_g1_of(case["pk"]["alpha_g1"]))
        a0 = 80 + 3 * 48 + 2 * 96
        assert b2[a0:a0 + 48 * len(pk.a_g1)] == b"".join(P.g1_compress(_g1_of(p)) for p in case["pk"]["a_g1"])
        v1, v2 = tmp_path / "v1.bin", tmp_path / "v2.bin"
        zkp.save_verification_key(vk, v1)
        zkp.save_verification_key(vk, v2, compressed=True)
        c1, c2 = v1.read_bytes(), v2.read_bytes()
        assert len(c2) == 24 + 48 + 3 * 96 + 48 * len(vk.ic_g1) and c2[:8] == b"ZKAMDVK2"
        assert c2[8:24] == c1[8:24]
        assert c2[24 + 48 + 3 * 96:] == b"".join(P.g1_compress(_g1_of(p)) for p in case["vk"]["ic_g1"])
        # the uncompressed format is what it was
        back = zkp.load_proving_key(p1)
        assert np.array_equal(back.b_g2, pk.b_g2) and np.array_equal(back.h_g1, pk.h_g1)


def test_key_file_unknown_magic_and_truncation(zkp, tmp_path):
    pk, vk = _keys(zkp, CASES[0])
    p2, v2 = tmp_path / "k2.bin", tmp_path / "v2.bin"
    zkp.save_proving_key(pk, p2, compressed=True)
    zkp.save_verification_key(vk, v2, compressed=True)
    bad = tmp_path / "bad.bin"
    for good, load in ((p2, zkp.load_proving_key), (v2, zkp.load_verification_key)):
        data = good.read_bytes()
        bad.write_bytes(data[:6] + b"K3" + data[8:])
        with pytest.raises(ValueError, match="not a .* key file"):
            load(bad)
        # cut inside the points: refused before any point is looked at
        for cut in (20, 100, 24 + 48 + 3 * 96 + 10):
            bad.write_bytes(data[:cut])
            with pytest.raises(ValueError, match="truncated key file"):
                load(bad)
