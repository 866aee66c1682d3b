"""The V2 tree digests on the GPU (include/zkp.h, "tree digests";
csrc/digest.hpp's k_g1_leaf_digest / k_g2_leaf_digest, one lane per leaf of
256 points): leaf digests against the host twin and the Python restatement
(digest_v2_ref.py) at every count where a lane's path changes and under chunk
lengths whose edges fall inside the array, raw struct words, the string and
key digests, and both phases of a ceremony that opts into V2."""
import numpy as np
import pytest

import digest_v2_ref as D
import srs_util

pytestmark = pytest.mark.gpu

DEFAULT_CHUNK = 1 << 20
# more than one wave of leaves (64 x 256 points) and a partial last leaf
G1_COUNTS = D.G1_COUNTS + (64 * 256 + 17,)
G2_COUNTS = D.G2_COUNTS + (32 * 256 + 17,)
assert G1_COUNTS[-1] == 16401 and G2_COUNTS[-1] == 8209


@pytest.fixture(scope="module")
def arrays(zkp):
    """per group and count: (words, host twin's leaf digests), made once; the
    counts the restatement covers are checked against it here"""
    out = {}
    for g, counts, host in ((1, G1_COUNTS, zkp.g1_leaf_digests_host), (2, G2_COUNTS, zkp.g2_leaf_digests_host)):
        for n in counts:
            words, want = D.cyclic(g, n)
            twin = host(words)
            assert twin.tobytes() == want
            out[g, n] = (words, twin)
    return out


@pytest.fixture
def chunked(zkp, ctx):
    def set_chunk(c):
        ctx.set_option(zkp.ZK_OPT_POINT_CHUNK, c)
    yield set_chunk
    ctx.set_option(zkp.ZK_OPT_POINT_CHUNK, DEFAULT_CHUNK)


# chunks of 256 (256), 256 (300: rounded down), 768 (1000) and 2^20 points
@pytest.mark.parametrize("chunk", [256, 300, 1000, DEFAULT_CHUNK])
def test_g1_leaves(ctx, arrays, chunked, chunk):
    chunked(chunk)
    for n in G1_COUNTS:
        words, twin = arrays[1, n]
        got = ctx.g1_leaf_digests(words)
        assert got.shape == twin.shape and np.array_equal(got, twin), n


@pytest.mark.parametrize("chunk", [256, 300, 1000, DEFAULT_CHUNK])
def test_g2_leaves(ctx, arrays, chunked, chunk):
    chunked(chunk)
    for n in G2_COUNTS:
        words, twin = arrays[2, n]
        got = ctx.g2_leaf_digests(words)
        assert got.shape == twin.shape and np.array_equal(got, twin), n


def test_chunk_of_one_point_is_one_leaf(ctx, arrays, chunked):
    """ZK_OPT_POINT_CHUNK below 256 (other calls use such values): at least a leaf"""
    chunked(1)
    words, twin = arrays[1, 513]
    assert np.array_equal(ctx.g1_leaf_digests(words), twin)


def _raw_case(zkp, g, rows, n):
    """every raw row once in lane 0 -- the unrolled unit, each of its slots in
    turn -- and once in the last leaf, which the tail alone hashes; the rest
    valid points.  -> (words, leaf digests by compress + hashlib)"""
    per = 4 // g
    words = np.array([D.filler(g)] * n, dtype=np.uint64)
    tail = n - n % 256
    assert 0 < n - tail < per and len(rows) * per + per <= 256
    for i, row in enumerate(rows):
        words[per * i + i % per] = row
    want = []
    for i, row in enumerate(rows):          # the last leaf holds one raw row at a time
        w = words.copy()
        w[tail + i % (n - tail)] = row
        want.append(w)
    compress = zkp.compress_g1 if g == 1 else zkp.compress_g2
    return [(w, D.leaves_of_bytes(g, compress(w))) for w in want]


def test_raw_g1(zkp, ctx):
    for words, want in _raw_case(zkp, 1, list(D.raw_g1().values()), 2 * 256 + 3):
        assert ctx.g1_leaf_digests(words).tobytes() == want
        assert zkp.g1_leaf_digests_host(words).tobytes() == want


def test_raw_g2(zkp, ctx):
    for words, want in _raw_case(zkp, 2, list(D.raw_g2().values()), 2 * 256 + 1):
        assert ctx.g2_leaf_digests(words).tobytes() == want
        assert zkp.g2_leaf_digests_host(words).tobytes() == want


def test_nothing(ctx):
    assert ctx.g1_leaf_digests(np.zeros((0, 13), dtype=np.uint64)).shape == (0, 32)
    assert ctx.g2_leaf_digests(np.zeros((0, 25), dtype=np.uint64)).shape == (0, 32)


# ------------------------------------------------------- string and key ---
def test_srs_digest_v2(zkp, ctx, chunked):
    srs, pts = D.string2(zkp)
    long, lpts = D.long_string(srs, pts)
    for s, p in ((srs, pts), (long, lpts)):
        want = D.srs_v2(2, p)
        assert s.digest(ctx, version=2) == want and s.digest(version=2) == want
        assert s.digest(ctx) == s.digest() != want          # version 1 takes no notice of a ctx
    chunked(256)
    assert long.digest(ctx, version=2) == D.srs_v2(2, lpts)
    with pytest.raises(ValueError):
        srs.digest(ctx, version=3)


def test_key_digest_v2(zkp, ctx):
    crs, case = D.key(zkp)
    want = D.key_v2(case["pk"], case["vk"])
    assert crs.digest(ctx, version=2) == want and crs.digest(version=2) == want
    assert crs.digest(ctx) == crs.digest() != want
    other = crs.copy()
    other.vk.ic_g1[0] = crs.vk.ic_g1[1]
    assert other.digest(ctx, version=2) == other.digest(version=2) != want


def test_profile_phases(zkp, ctx):
    """the kernels and the upload are phases of the ctx profile"""
    words, _ = D.cyclic(1, 257)
    srs, _ = D.string2(zkp)
    ctx.profile(True)
    try:
        ctx.g1_leaf_digests(words)
        srs.digest(ctx, version=2)
        prof = ctx.profile_read()
    finally:
        ctx.profile(False)
    assert prof["leaf_digest_g1"]["launches"] == 4 and prof["leaf_digest_g1"]["units"] == 257 + 8 + 4 + 4
    assert prof["leaf_digest_g2"]["launches"] == 1 and prof["leaf_digest_g2"]["units"] == 4
    assert prof["leaf_upload"]["launches"] == 5 and prof["digest_top_hash"]["launches"] == 1


# ------------------------------------------------- a ceremony that uses V2 ---
def test_phase1_v2(zkp, ctx, pyref):
    case = srs_util.case4(pyref)
    s0 = srs_util.string(zkp, ctx, case, 4)
    rng = pyref.SplitMix64(0x7A5D)
    sh = [tuple(rng.fr() or 1 for _ in range(3)) for _ in range(2)]
    s1, share1, proof1 = s0.contribute_proved(ctx, *sh[0], digest_version=2)
    s2, share2, proof2 = s1.contribute_proved(ctx, *sh[1], digest_version=2)
    shares, proofs = np.stack([share1, share2]), np.stack([proof1, proof2])
    v2 = [s0.digest(ctx, version=2), s1.digest(ctx, version=2)]
    assert v2 == [s0.digest(version=2), s1.digest(version=2)]
    st = zkp.SRS.verify_contribution_proofs(ctx, v2, shares, proofs)
    assert st.shape == (2, 3) and (st == zkp.ZK_POK_OK).all()
    st = zkp.SRS.verify_contribution_proofs(ctx, [s0.digest(), s1.digest()], shares, proofs)
    assert (st == zkp.ZK_POK_REJECT).all()
    assert np.array_equal(proof2[2], zkp.pok_make(sh[1][2], zkp.ZK_POK_BETA, v2[1]))
    # the default is version 1, as before
    _, share, proof = s0.contribute_proved(ctx, *sh[0])
    assert np.array_equal(proof[0], zkp.pok_make(sh[0][0], zkp.ZK_POK_TAU, s0.digest()))
    assert np.array_equal(share, share1)


def test_phase2_v2(zkp, ctx, pyref):
    crs0, _ = D.key(zkp)
    rng = pyref.SplitMix64(0xD317B)
    d1 = rng.fr() or 1
    crs1, proof1 = crs0.contribute_proved(ctx, d1, digest_version=2)
    assert np.array_equal(proof1, zkp.pok_make(d1, zkp.ZK_POK_DELTA, crs0.digest(version=2)))
    assert zkp.CRS.verify_contribution_proof(ctx, crs0, crs1, proof1, digest_version=2) == (True, zkp.ZK_POK_OK)
    assert zkp.CRS.verify_contribution_proof(ctx, crs0, crs1, proof1, digest_version=1) == (False, zkp.ZK_POK_REJECT)
    assert zkp.CRS.verify_contribution_proof(ctx, crs0, crs1, proof1) == (False, zkp.ZK_POK_REJECT)
    # a version-1 proof under version 2
    _, proof_v1 = crs0.contribute_proved(ctx, d1)
    assert zkp.CRS.verify_contribution_proof(ctx, crs0, crs1, proof_v1) == (True, zkp.ZK_POK_OK)
    assert zkp.CRS.verify_contribution_proof(ctx, crs0, crs1, proof_v1, digest_version=2) == (False, zkp.ZK_POK_REJECT)
