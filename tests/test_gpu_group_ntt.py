"""The radix-2 transform over group elements (csrc/srs.hip: zk_g1_ntt,
zk_g2_ntt).  Every comparison is byte equality of canonical words.

The transform is linear, so for P_j = [s_j]G it must give [X_k]G with X the Fr
transform of s: the inputs come from the 255-bit fixed-base kernel, the
expected outputs from the Fr NTT through the same kernel.  A second path, free
of the Fr NTT, is the public MSM with the coefficients w^(+-jk) (/ n); pyref
pins the two smallest cases by a direct sum."""
import ctypes

import numpy as np
import pytest

import points_util as U

pytestmark = pytest.mark.gpu

GROUPS = ("g1", "g2")


def _ntt(ctx, g, pts, inverse):
    return ctx.g2_ntt(pts, inverse) if g == "g2" else ctx.g1_ntt(pts, inverse)


def _scalars(pyref, n, seed):
    rng = pyref.SplitMix64(seed)
    return [rng.fr() for _ in range(n)]


def _expect(zkp, ctx, g, scalars, inverse):
    """[NTT(s)_k]G: the Fr transform, then the fixed base"""
    return ctx.test_fixed_base(ctx.ntt(zkp.fr_array(scalars), inverse=inverse), g2=(g == "g2"))


def _identity(g):
    return [0] * (24 if g == "g2" else 12) + [1]


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 4, 5, 6, 7, 10])
@pytest.mark.parametrize("g", GROUPS)
def test_against_fr_ntt(zkp, ctx, pyref, g, log_n, inverse):
    """log_n = 7: the first size with more than one wave of butterflies;
    10: several blocks, stages whose waves share a twiddle and stages whose
    lanes each have their own."""
    s = _scalars(pyref, 1 << log_n, 0x6E77 + log_n)
    pts = ctx.test_fixed_base(s, g2=(g == "g2"))
    got = _ntt(ctx, g, pts, inverse)
    assert np.array_equal(got, _expect(zkp, ctx, g, s, inverse))
    if log_n == 0:
        assert np.array_equal(got, pts)


@pytest.mark.parametrize("g", GROUPS)
def test_lane_mappings_agree(zkp, ctx, pyref, g):
    """ZK_OPT_GNTT_MAP = 0 (a twiddle per lane in every stage) gives the bytes
    of the default mapping."""
    s = _scalars(pyref, 1 << 10, 0x3A9)
    pts = ctx.test_fixed_base(s, g2=(g == "g2"))
    want = _expect(zkp, ctx, g, s, True)
    try:
        ctx.set_option(zkp.ZK_OPT_GNTT_MAP, 0)
        assert np.array_equal(_ntt(ctx, g, pts, True), want)
    finally:
        ctx.set_option(zkp.ZK_OPT_GNTT_MAP, -1)
    assert np.array_equal(_ntt(ctx, g, pts, True), want)


def _msm_coeffs(pyref, n, k, inverse):
    w = pyref.root_of_unity(n)
    if inverse:
        w = pyref.fr_inv(w)
    scale = pyref.fr_inv(n) if inverse else 1
    return [pow(w, j * k, pyref.R) * scale % pyref.R for j in range(n)]


@pytest.mark.parametrize("g,log_n", [("g1", k) for k in range(5)] + [("g2", k) for k in range(4)])
def test_against_msm(zkp, ctx, pyref, g, log_n):
    """out[k] = sum_j w^(+-jk) (/ n) P_j for every k, both directions"""
    n = 1 << log_n
    pts = ctx.test_fixed_base(_scalars(pyref, n, 0x3535 + log_n), g2=(g == "g2"))
    msm = ctx.msm_g2 if g == "g2" else ctx.msm_g1
    for inverse in (False, True):
        got = _ntt(ctx, g, pts, inverse)
        for k in range(n):
            assert np.array_equal(got[k], msm(pts, zkp.fr_array(_msm_coeffs(pyref, n, k, inverse)))), (inverse, k)


def test_against_msm_2p10(zkp, ctx, pyref):
    n = 1 << 10
    pts = ctx.test_fixed_base(_scalars(pyref, n, 0x3545), g2=False)
    for inverse in (False, True):
        got = ctx.g1_ntt(pts, inverse)
        for k in (0, 1, 2, 63, 64, 511, 512, 1023):
            assert np.array_equal(got[k], ctx.msm_g1(pts, zkp.fr_array(_msm_coeffs(pyref, n, k, inverse)))), (inverse, k)


@pytest.mark.parametrize("n", [8, 256])
@pytest.mark.parametrize("g", GROUPS)
def test_edge_inputs(zkp, ctx, pyref, g, n):
    """Identities, equal points (the doubling branch of the butterfly's
    additions) and opposite points (its infinity branch)."""
    R = pyref.R
    s = pyref.SplitMix64(0xED6E + n).fr()
    ident = _identity(g)
    fb = lambda sc: ctx.test_fixed_base(sc, g2=(g == "g2"))

    # all identities
    pts = fb([0] * n)
    assert all(list(r) == ident for r in pts)
    for inverse in (False, True):
        assert np.array_equal(_ntt(ctx, g, pts, inverse), pts)

    # one entry that is not the identity
    sc = [0] * n
    sc[3] = s
    for inverse in (False, True):
        assert np.array_equal(_ntt(ctx, g, fb(sc), inverse), _expect(zkp, ctx, g, sc, inverse))

    # all entries the same point P: out[0] = n P, the rest the identity
    got = _ntt(ctx, g, fb([s] * n), False)
    assert np.array_equal(got[0], fb([n * s % R])[0])
    assert all(list(r) == ident for r in got[1:])
    got = _ntt(ctx, g, fb([s] * n), True)
    assert np.array_equal(got[0], fb([s])[0])
    assert all(list(r) == ident for r in got[1:])

    # P, -P, P, -P, ...: everything lands in out[n / 2]
    sc = [s if j % 2 == 0 else R - s for j in range(n)]
    got = _ntt(ctx, g, fb(sc), False)
    assert np.array_equal(got[n // 2], fb([n * s % R])[0])
    assert all(list(r) == ident for k, r in enumerate(got) if k != n // 2)
    assert np.array_equal(got, _expect(zkp, ctx, g, sc, False))

    # identities between points, and the inverse of the forward transform
    sc = _scalars(pyref, n, 0x1D + n)
    for j in range(0, n, 3):
        sc[j] = 0
    pts = fb(sc)
    fwd = _ntt(ctx, g, pts, False)
    assert np.array_equal(fwd, _expect(zkp, ctx, g, sc, False))
    assert np.array_equal(_ntt(ctx, g, fwd, True), pts)


def test_pyref_g1_inverse_n4(zkp, ctx, pyref):
    pts = U.g1_points(4)
    got = ctx.g1_ntt(U.words_g1(pts), inverse=True)
    for i in range(4):
        c = _msm_coeffs(pyref, 4, i, True)
        want = pyref.G1.msm([(c[k], pts[k]) for k in range(4)])
        assert list(got[i]) == pyref.g1_words(want), i


def test_pyref_g2_inverse_n2(zkp, ctx, pyref):
    pts = U.g2_points(2)
    got = ctx.g2_ntt(U.words_g2(pts), inverse=True)
    for i in range(2):
        c = _msm_coeffs(pyref, 2, i, True)
        want = pyref.G2.add(pyref.G2.mul(pts[0], c[0]), pyref.G2.mul(pts[1], c[1]))
        assert list(got[i]) == pyref.g2_words(want), i


def test_errors(zkp, ctx):
    buf = np.zeros((1, 25), dtype=np.uint64)
    h = ctypes.c_void_p(ctx._h)
    for fn in (zkp.lib().zk_g1_ntt, zkp.lib().zk_g2_ntt):
        assert fn(h, zkp._p(buf), ctypes.c_uint32(33), ctypes.c_int(1)) == zkp.ZK_ERR_DOMAIN
        assert fn(h, zkp._p(buf), ctypes.c_uint32(0), ctypes.c_int(0)) == zkp.ZK_ERR_ARG
        assert fn(h, None, ctypes.c_uint32(0), ctypes.c_int(1)) == zkp.ZK_ERR_ARG
    with pytest.raises(zkp.DomainTooSmall):
        ctx.g1_ntt(np.zeros((3, 13), dtype=np.uint64))
