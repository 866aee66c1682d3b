"""The hash to G2 on the GPU and the proofs of knowledge checked there
(zk_hash_to_g2, zk_pok_verify_many, zk_srs_verify_contribution_proofs;
csrc/hash.hip over csrc/hash.hpp): the device hash against the Python
restatement (h2g2_ref.py) on a wave whose lanes leave the try loop at seven
different times, against the host twin across block counts and both SHA-256
padding boundaries, the try cap, the batch check of proofs against the host
check proof by proof, and the two ceremonies end to end with every way a
transcript can be wrong."""
import concurrent.futures
import hashlib

import numpy as np
import pytest

import h2g2_ref as H
import points_util as U
import sound_ref
import srs_util

pytestmark = pytest.mark.gpu

R = sound_ref.R


@pytest.fixture(scope="module")
def reference(pyref):
    """the 64-message set under dst b"test": (messages, (64, 25) words, try counts)"""
    msgs = H.message_set(64)
    ref = [H.h2g2(m, b"test") for m in msgs]
    return msgs, np.array([pyref.g2_words(q) for q, _ in ref], dtype=np.uint64), np.array([t for _, t in ref])


def _host(zkp, msgs, dst):
    got = [zkp.hash_to_g2_host(m, dst) for m in msgs]
    return np.array([w for w, _ in got], dtype=np.uint64).reshape(-1, 25), np.array([t for _, t in got], dtype=np.uint8)


# ---------------------------------------------------------------- the hash ---
def test_hash_against_reference(ctx, reference):
    msgs, words, tries = reference
    assert set(range(6)) <= set(tries.tolist())           # the lanes of the one wave leave at different times
    out, got = ctx.hash_to_g2(msgs, b"test")
    assert np.array_equal(got, tries)
    assert np.array_equal(out, words)


@pytest.mark.parametrize("n", [1, 127, 128, 129, 257])
def test_device_against_host_blocks(zkp, ctx, n):
    """one block, a partial one, several: 36-byte messages"""
    msgs = [hashlib.sha256(b"blocks %d" % i).digest() + i.to_bytes(4, "little") for i in range(n)]
    words, tries = _host(zkp, msgs, b"test")
    out, got = ctx.hash_to_g2(msgs, b"test")
    assert np.array_equal(got, tries) and np.array_equal(out, words)


@pytest.mark.parametrize("msg_len", [0, 1, 27, 28, 36, 37, 81, 200])
def test_device_against_host_lengths(zkp, ctx, msg_len):
    """the prefix is 18 bytes with dst b"test": total lengths 45-55 and 56-64
    cross both padding boundaries of SHA-256; odd lengths leave every message
    but the first unaligned"""
    n = 5
    msgs = [bytes((17 * i + 3 * k + 1) & 0xFF for k in range(msg_len)) for i in range(n)]
    words, tries = _host(zkp, msgs, b"test")
    out, got = ctx.hash_to_g2(np.frombuffer(b"".join(msgs), dtype=np.uint8).reshape(n, msg_len), b"test")
    assert np.array_equal(got, tries) and np.array_equal(out, words)


def test_device_dst_lengths(zkp, ctx):
    msgs = H.message_set(3)
    for dst in (b"", bytes(range(255))):
        words, tries = _host(zkp, msgs, dst)
        out, got = ctx.hash_to_g2(msgs, dst)
        assert np.array_equal(got, tries) and np.array_equal(out, words)
    with pytest.raises(ValueError):
        ctx.hash_to_g2(msgs, bytes(256))


def test_hash_nothing(ctx):
    out, tries = ctx.hash_to_g2([], b"test")
    assert out.shape == (0, 25) and len(tries) == 0


def test_capped_tries(ctx, reference):
    """the same kernel with a cap of one try: the loop ends at the cap, exactly
    the messages whose first x is on the twist get their point, the others 0xff
    and zero words"""
    msgs, words, tries = reference
    out, got = ctx.test_hash_to_g2_capped(msgs, b"test", 1)
    first = tries == 0
    assert first.sum() == 28
    assert np.array_equal(got[first], tries[first]) and np.array_equal(out[first], words[first])
    assert (got[~first] == 0xFF).all() and not out[~first].any()
    out, got = ctx.test_hash_to_g2_capped(msgs, b"test", 4)       # a cap inside the spread of the wave
    some = tries < 4
    assert np.array_equal(got[some], tries[some]) and np.array_equal(out[some], words[some])
    assert (got[~some] == 0xFF).all() and not out[~some].any()


# ------------------------------------------------------ proofs of knowledge ---
def _host_verify(zkp, poks, roles, challenges):
    with concurrent.futures.ThreadPoolExecutor(8) as pool:       # the host pairing is tens of ms a proof
        return np.array(list(pool.map(lambda a: zkp.pok_verify(*a), zip(poks, roles, challenges))), dtype=np.uint8)


@pytest.fixture(scope="module")
def batch(zkp, pyref):
    """130 proofs over mixed roles and challenges, eight of them broken"""
    rng = pyref.SplitMix64(0x90C)
    n = 130
    roles = [i % 4 for i in range(n)]
    challenges = [hashlib.sha256(b"challenge %d" % (i % 7)).digest() for i in range(n)]
    shares = [rng.fr() or 1 for _ in range(n)]
    poks = np.array([zkp.pok_make(s, r, c) for s, r, c in zip(shares, roles, challenges)], dtype=np.uint64)
    want = np.zeros(n, dtype=np.uint8)
    for i in (3, 64):                                             # another role
        roles[i] = (roles[i] + 1) % 4
        want[i] = zkp.ZK_POK_REJECT
    for i in (9, 127):                                            # one challenge bit
        c = bytearray(challenges[i])
        c[i % 32] ^= 0x10
        challenges[i] = bytes(c)
        want[i] = zkp.ZK_POK_REJECT
    for i in (20, 128):                                           # s_g1 of another share
        poks[i, :13] = poks[i + 1, :13]
        want[i] = zkp.ZK_POK_REJECT
    for i in (33, 65):                                            # s_r of another proof
        poks[i, 13:] = poks[i + 1, 13:]
        want[i] = zkp.ZK_POK_REJECT
    poks[70, :13] = pyref.g1_words(pyref.INF)                     # the identity
    poks[99, 13:] = pyref.g2_words(U.g2_off_subgroup()[1])        # on the twist, outside G2
    want[70] = want[99] = zkp.ZK_POK_POINT
    return poks, roles, challenges, want


def test_pok_verify_many(zkp, ctx, batch):
    poks, roles, challenges, want = batch
    st, first_bad = ctx.pok_verify_many(poks, roles, challenges)
    assert np.array_equal(st, want)
    assert np.array_equal(st, _host_verify(zkp, poks, roles, challenges))
    assert first_bad == 3
    good = want == zkp.ZK_POK_OK
    st, first_bad = ctx.pok_verify_many(poks[good], np.array(roles)[good], np.array(
        [np.frombuffer(c, dtype=np.uint8) for c in challenges])[good])
    assert not st.any() and first_bad == int(good.sum())


def test_pok_verify_many_small(zkp, ctx, batch):
    poks, roles, challenges, want = batch
    st, first_bad = ctx.pok_verify_many(poks[:1], roles[:1], challenges[:1])
    assert st.tolist() == [zkp.ZK_POK_OK] and first_bad == 1
    st, first_bad = ctx.pok_verify_many(poks[3:4], roles[3:4], challenges[3:4])
    assert st.tolist() == [zkp.ZK_POK_REJECT] and first_bad == 0
    st, first_bad = ctx.pok_verify_many(np.zeros((0, 38), dtype=np.uint64), [], [])
    assert len(st) == 0 and first_bad == 0
    with pytest.raises(ValueError):
        ctx.pok_verify_many(poks[:2], [0, 4], challenges[:2])


def test_pok_verify_many_chunks(zkp, ctx, batch):
    """ZK_OPT_VERIFY_CHUNK = 50: three launches, the last one partial"""
    poks, roles, challenges, want = batch
    ctx.set_option(zkp.ZK_OPT_VERIFY_CHUNK, 50)
    try:
        st, first_bad = ctx.pok_verify_many(poks, roles, challenges)
    finally:
        ctx.set_option(zkp.ZK_OPT_VERIFY_CHUNK, 65536)
    assert np.array_equal(st, want) and first_bad == 3


# --------------------------------------------------------- phase 1, end to end ---
def _coeffs(pyref, n, seed=0x5125):
    rng = pyref.SplitMix64(seed)
    return [((rng.next() << 64) | rng.next()) or 1 for _ in range(n)]


def test_phase1_transcript(zkp, ctx, pyref):
    case = srs_util.case4(pyref)
    s0 = srs_util.string(zkp, ctx, case, 3)
    rng = pyref.SplitMix64(0x7A5C)
    sh = [tuple(rng.fr() or 1 for _ in range(3)) for _ in range(2)]
    s1, share1, proof1 = s0.contribute_proved(ctx, *sh[0])
    s2, share2, proof2 = s1.contribute_proved(ctx, *sh[1])
    digests = [s0.digest(), s1.digest()]
    shares, proofs = np.stack([share1, share2]), np.stack([proof1, proof2])
    ok = np.zeros((2, 3), dtype=np.uint8)
    assert np.array_equal(zkp.SRS.verify_contribution_proofs(ctx, digests, shares, proofs), ok)
    # each proof is the library's proof for the share, role and digest
    assert np.array_equal(proof2[1], zkp.pok_make(sh[1][1], zkp.ZK_POK_ALPHA, digests[1]))
    # a contribution replayed against the other digest
    st = zkp.SRS.verify_contribution_proofs(ctx, digests[::-1], shares, proofs)
    assert (st == zkp.ZK_POK_REJECT).all()
    # the published alpha and beta share points swapped: tau still holds
    swapped = shares.copy()
    swapped[0, 1], swapped[0, 2] = shares[0, 2], shares[0, 1]
    st = zkp.SRS.verify_contribution_proofs(ctx, digests, swapped, proofs)
    assert st.tolist() == [[zkp.ZK_POK_OK, zkp.ZK_POK_REJECT, zkp.ZK_POK_REJECT], [0, 0, 0]]
    # a good proof of knowledge, but of another share than the published one
    other = proofs.copy()
    other[1, 0] = zkp.pok_make(sh[1][0] + 1, zkp.ZK_POK_TAU, digests[1])
    assert zkp.pok_verify(other[1, 0], zkp.ZK_POK_TAU, digests[1]) == zkp.ZK_POK_OK
    st = zkp.SRS.verify_contribution_proofs(ctx, digests, shares, other)
    assert st.tolist() == [[0, 0, 0], [zkp.ZK_POK_REJECT, zkp.ZK_POK_OK, zkp.ZK_POK_OK]]
    # the check of the strings themselves still accepts them
    co = _coeffs(pyref, 16)
    assert zkp.SRS.verify_contribution(ctx, s0, s1, share1, co)[0]
    assert zkp.SRS.verify_contribution(ctx, s1, s2, share2, co)[0]
    # no contributions: nothing to do
    assert zkp.SRS.verify_contribution_proofs(ctx, [], np.zeros((0, 3, 25), dtype=np.uint64),
                                              np.zeros((0, 3, 38), dtype=np.uint64)).shape == (0, 3)


# --------------------------------------------------------- phase 2, end to end ---
def test_phase2_transcript(zkp, ctx, pyref):
    case = sound_ref.build_case()
    qap = zkp.QAP(zkp.CSRMatrices.synthetic(sound_ref.CASE_N))
    crs0 = zkp.CRS(sound_ref.pk_to_product(zkp, case["pk"], qap), sound_ref.vk_to_product(zkp, case["vk"]))
    rng = pyref.SplitMix64(0xD317A)
    d1, d2 = (rng.fr() or 1 for _ in range(2))
    crs1, proof1 = crs0.contribute_proved(ctx, d1)
    crs2, proof2 = crs1.contribute_proved(ctx, d2)
    assert zkp.CRS.verify_contribution_proof(ctx, crs0, crs1, proof1) == (True, zkp.ZK_POK_OK)
    assert zkp.CRS.verify_contribution_proof(ctx, crs1, crs2, proof2) == (True, zkp.ZK_POK_OK)
    # against the wrong `before`: the challenge differs
    assert zkp.CRS.verify_contribution_proof(ctx, crs1, crs1, proof1) == (False, zkp.ZK_POK_REJECT)
    assert zkp.CRS.verify_contribution_proof(ctx, crs0, crs2, proof2) == (False, zkp.ZK_POK_REJECT)
    # the right challenge, a key that moved by another share: the link fails
    assert zkp.CRS.verify_contribution_proof(ctx, crs0, crs2, proof1) == (False, zkp.ZK_POK_REJECT)
    assert np.array_equal(proof1, zkp.pok_make(d1, zkp.ZK_POK_DELTA, crs0.digest()))
    # the key check itself still accepts
    n = len(crs0.pk.h_g1) + len(crs0.pk.ic_g1)
    assert zkp.CRS.verify_contribution(ctx, crs0, crs1, _coeffs(pyref, n))[0]
