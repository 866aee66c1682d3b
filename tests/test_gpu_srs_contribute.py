"""Phase-1 contributions to a powers-of-tau string on the GPU (zk_srs_contribute,
zk_srs_verify_contribution; csrc/srs.hip over csrc/mulvec.hip): SRS.contribute
against SRS.generate with the multiplied secrets -- an independent path, the
fixed-base kernel --, chains, the trivial shares, the key and a proof from a
contributed string, every verdict of SRS.verify_contribution, and the errors."""
import ctypes

import numpy as np
import pytest

import points_util as U
import sound_ref

pytestmark = pytest.mark.gpu

R = sound_ref.R
ARRAYS = ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2")


def _same(a, b):
    assert a.log_n == b.log_n
    for nm in ARRAYS:
        assert np.array_equal(getattr(a, nm), getattr(b, nm)), nm


@pytest.fixture(scope="module")
def case4(pyref):
    """the parameters, witness and blinding of sound_ref's shared case (n = 4)"""
    rng = pyref.SplitMix64(sound_ref.CASE_SEED)
    alpha, beta, _, _, tau = (rng.fr() for _ in range(5))
    r, s = rng.fr(), rng.fr()
    return {"alpha": alpha, "beta": beta, "tau": tau, "r": r, "s": s,
            "z": pyref.synthetic_witness(sound_ref.CASE_N, sound_ref.CASE_SEED + 1)}


@pytest.fixture(scope="module")
def shares(pyref):
    rng = pyref.SplitMix64(0x5A4E5)
    return [tuple(rng.fr() for _ in range(3)) for _ in range(2)]


def _string(zkp, ctx, case, log_n, s=1, a=1, b=1):
    return zkp.SRS.generate(ctx, log_n, case["tau"] * s % R, case["alpha"] * a % R, case["beta"] * b % R)


@pytest.fixture(scope="module")
def strings(zkp, ctx, case4):
    return {log_n: _string(zkp, ctx, case4, log_n) for log_n in (2, 5)}


def _coeffs(pyref, n, seed=0x5125):
    rng = pyref.SplitMix64(seed)
    return [((rng.next() << 64) | rng.next()) or 1 for _ in range(n)]


def _g1(pyref, words):
    w = [int(x) for x in words]
    return (pyref.Fq1(sum(w[i] << (64 * i) for i in range(6))), pyref.Fq1(sum(w[6 + i] << (64 * i) for i in range(6))))


# -------------------------------------------------------------- contribute ---
@pytest.mark.parametrize("log_n", [2, 5])
def test_one_contribution(zkp, ctx, pyref, case4, strings, shares, log_n):
    srs = strings[log_n]
    keep = srs.copy()
    s, a, b = shares[0]
    new, share = srs.contribute(ctx, s, a, b)
    _same(srs, keep)                                               # the old string is untouched
    _same(new, _string(zkp, ctx, case4, log_n, s, a, b))
    assert np.array_equal(share, ctx.test_fixed_base([s, a, b], g2=True))
    N = 1 << log_n
    for nm, i, k in (("tau_g1", 1, s), ("tau_g1", 2 * N - 1, pow(s, 2 * N - 1, R)),
                     ("alpha_tau_g1", N - 1, a * pow(s, N - 1, R) % R), ("beta_tau_g1", 0, b),
                     ("beta_tau_g1", 2, b * s * s % R)):
        want = pyref.g1_words(pyref.G1.mul(_g1(pyref, getattr(srs, nm)[i]), k))
        assert list(getattr(new, nm)[i]) == want, (nm, i)
    assert list(new.tau_g2[1]) == pyref.g2_words(pyref.G2.mul(pyref.G2.gen, case4["tau"] * s % R))
    assert list(new.beta_g2) == pyref.g2_words(pyref.G2.mul(pyref.G2.gen, case4["beta"] * b % R))


@pytest.mark.parametrize("log_n", [2, 5])
def test_chain(zkp, ctx, case4, strings, shares, log_n):
    (s1, a1, b1), (s2, a2, b2) = shares
    mid, _ = strings[log_n].contribute(ctx, s1, a1, b1)
    end, _ = mid.contribute(ctx, s2, a2, b2)
    _same(end, _string(zkp, ctx, case4, log_n, s1 * s2, a1 * a2, b1 * b2))


@pytest.mark.parametrize("log_n", [2, 5])
def test_trivial_shares(zkp, ctx, strings, log_n):
    new, share = strings[log_n].contribute(ctx, 1, 1, 1)
    _same(new, strings[log_n])
    assert np.array_equal(share, ctx.test_fixed_base([1, 1, 1], g2=True))


def test_string_to_proof(zkp, ctx, case4, strings, shares):
    s, a, b = shares[0]
    new, _ = strings[2].contribute(ctx, s, a, b)
    qap = zkp.QAP(zkp.CSRMatrices.synthetic(sound_ref.CASE_N))
    crs = zkp.CRS.from_srs(ctx, qap, new, sound_ref.CASE_PUBLIC)
    params = zkp.SetupParams(case4["alpha"] * a % R, case4["beta"] * b % R, 1, 1, case4["tau"] * s % R)
    want = zkp.CRS.generate_from_qap(ctx, qap, params, sound_ref.CASE_PUBLIC, sound=True)
    for nm in ("a_g1", "b_g1", "b_g2", "ic_g1", "h_g1"):
        assert np.array_equal(getattr(crs.pk, nm), getattr(want.pk, nm)), nm
    for nm in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2"):
        assert np.array_equal(crs.pk.point(nm), want.pk.point(nm)), nm
    assert np.array_equal(crs.vk.ic_g1, want.vk.ic_g1)
    dpk = crs.pk.upload(ctx)
    try:
        proof = zkp.Prover.prove(dpk, zkp.Witness(case4["z"], sound_ref.CASE_PUBLIC), r=case4["r"], s=case4["s"])
    finally:
        dpk.free()
    x = case4["z"][1]
    assert zkp.Verifier.verify(crs.vk, proof, [x]) is True
    assert zkp.Verifier.verify(crs.vk, proof, [(x + 1) % R]) is False


# ---------------------------------------------------------------- verdicts ---
@pytest.mark.parametrize("log_n", [2, 5])
def test_verdicts(zkp, ctx, pyref, case4, strings, shares, log_n):
    Z = zkp
    srs = strings[log_n]
    N = 1 << log_n
    s, a, b = shares[0]
    new, share = srs.contribute(ctx, s, a, b)
    co = _coeffs(pyref, 2 * N)
    verify = lambda before, after, sh, c=co: Z.SRS.verify_contribution(ctx, before, after, sh, c)
    assert verify(srs, new, share) == (True, Z.ZK_SRSC_OK, Z.ZK_SRS_OK)
    assert Z.SRS.verify_contribution(ctx, srs, new, share) == (True, Z.ZK_SRSC_OK, Z.ZK_SRS_OK)   # from `secrets`

    other = strings[7 - log_n]
    assert verify(other, new, share, _coeffs(pyref, 2 * N))[:2] == (False, Z.ZK_SRSC_SHAPE)
    assert verify(srs, new, share, co[:-1])[:2] == (False, Z.ZK_SRSC_SHAPE)

    bad = share.copy()
    bad[1] = [0] * 24 + [1]
    assert verify(srs, new, bad)[:2] == (False, Z.ZK_SRSC_SHARE)
    bad = share.copy()
    bad[2] = pyref.g2_words(U.g2_off_subgroup()[0])
    assert verify(srs, new, bad)[:2] == (False, Z.ZK_SRSC_SHARE)

    t = new.copy()
    t.tau_g1[3] = ctx.g1_mul_scalar(t.tau_g1[3:4], 2)[0]
    assert verify(srs, t, share) == (False, Z.ZK_SRSC_STRING, Z.ZK_SRS_POWERS_G1)

    unrelated = Z.SRS.generate(ctx, log_n, 11, 13, 17)
    assert verify(srs, unrelated, share) == (False, Z.ZK_SRSC_TAU, Z.ZK_SRS_OK)

    assert verify(srs, new, share[[0, 2, 1]]) == (False, Z.ZK_SRSC_ALPHA, Z.ZK_SRS_OK)

    bad = share.copy()
    bad[2] = ctx.test_fixed_base([b + 1], g2=True)[0]
    assert verify(srs, new, bad) == (False, Z.ZK_SRSC_BETA, Z.ZK_SRS_OK)

    for c in (0, 1 << 128):
        with pytest.raises(ValueError):
            verify(srs, new, share, co[:4] + [c] + co[5:])


# ------------------------------------------------------------------ errors ---
def _raw(zkp, ctx, srs, s, a, b):
    """the C call -> (rc, the string byte for byte untouched)"""
    before = srs.copy()
    fr = lambda v: ctypes.byref(zkp._Fr((ctypes.c_uint64 * 4)(*zkp.to_limbs(v))))
    c = srs._bind()
    b2 = bytes(c.beta_g2)
    rc = zkp.lib().zk_srs_contribute(ctypes.c_void_p(ctx._h), ctypes.byref(c), fr(s), fr(a), fr(b), None)
    same = all(np.array_equal(getattr(srs, nm), getattr(before, nm)) for nm in ARRAYS) and bytes(c.beta_g2) == b2
    return rc, same


def test_errors(zkp, ctx, strings):
    srs = strings[2].copy()
    assert _raw(zkp, ctx, srs, 0, 5, 7) == (zkp.ZK_ERR_ARG, True)
    assert _raw(zkp, ctx, srs, 3, R, 7) == (zkp.ZK_ERR_ARG, True)
    assert _raw(zkp, ctx, srs, 3, 5, 1 << 255) == (zkp.ZK_ERR_ARG, True)
    short = srs.copy()
    short.alpha_tau_g1 = short.alpha_tau_g1[:3]
    assert _raw(zkp, ctx, short, 3, 5, 7) == (zkp.ZK_ERR_ARG, True)
    with pytest.raises(ValueError):
        short.contribute(ctx, 3, 5, 7)
    for bad in ((0, 5, 7), (3, R, 7), (3, 5, -1)):
        with pytest.raises(ValueError):
            srs.contribute(ctx, *bad)
    assert _raw(zkp, ctx, srs, 3, 5, 7) == (zkp.ZK_OK, False)
