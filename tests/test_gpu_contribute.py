"""Phase-2 key contributions on the GPU (csrc/ceremony.hip): the kernel "n G1
points times one scalar" (the shipped endomorphism walk and the test library's
plain walk) against pyref and against each other, CRS.contribute against the
sound setup with delta * d, chains, identity entries, proofs under the new
key, and every verdict of CRS.verify_contribution."""
import ctypes

import numpy as np
import pytest

import points_util as U
import sound_ref

pytestmark = pytest.mark.gpu

R = sound_ref.R
X2 = 0xD201000000010000 ** 2          # x^2: r = x^4 - x^2 + 1
PK_ARRAYS = ("a_g1", "b_g1", "b_g2", "ic_g1", "h_g1")
PK_POINTS = ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2")
VK_POINTS = ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2")


def _g1(pyref, words):
    w = [int(x) for x in words]
    if w[12]:
        return pyref.INF
    return (pyref.Fq1(sum(w[i] << (64 * i) for i in range(6))), pyref.Fq1(sum(w[6 + i] << (64 * i) for i in range(6))))


def _same_crs(a, b):
    for nm in PK_ARRAYS:
        assert np.array_equal(getattr(a.pk, nm), getattr(b.pk, nm)), nm
    for nm in PK_POINTS:
        assert np.array_equal(a.pk.point(nm), b.pk.point(nm)), nm
    assert a.pk.num_public == b.pk.num_public and a.vk.num_public == b.vk.num_public
    assert np.array_equal(a.vk.ic_g1, b.vk.ic_g1)
    for nm in VK_POINTS:
        assert np.array_equal(a.vk.point(nm), b.vk.point(nm)), nm


@pytest.fixture(scope="module")
def case4(pyref):
    """the parameters, witness and blinding of sound_ref's shared case (n = 4)"""
    rng = pyref.SplitMix64(sound_ref.CASE_SEED)
    params = tuple(rng.fr() for _ in range(5))
    r, s = rng.fr(), rng.fr()
    return {"params": params, "r": r, "s": s, "z": pyref.synthetic_witness(sound_ref.CASE_N, sound_ref.CASE_SEED + 1)}


@pytest.fixture(scope="module")
def qap4(zkp):
    return zkp.QAP(zkp.CSRMatrices.synthetic(sound_ref.CASE_N))


@pytest.fixture(scope="module")
def crs4(zkp, ctx, case4, qap4):
    return zkp.CRS.generate_from_qap(ctx, qap4, zkp.SetupParams(*case4["params"]), sound_ref.CASE_PUBLIC, sound=True)


def _with_delta(zkp, ctx, qap, params, delta, num_public=1):
    p = list(params)
    p[3] = delta % R
    return zkp.CRS.generate_from_qap(ctx, qap, zkp.SetupParams(*p), num_public, sound=True)


# ------------------------------------------------------------------ kernel ---
def test_kernel_against_pyref(zkp, ctx, pyref):
    """21 points (an identity in the middle), the scalars at which the split
    k = e2 x^2 + e1 degenerates (e1 = 0, e2 = 1, e2 = 0) and the ends of the
    range: both walks word for word, three points per scalar against pyref."""
    pts = list(U.g1_points(20))
    pts.insert(10, pyref.INF)
    words = U.words_g1(pts)
    rng = pyref.SplitMix64(0xCE4E)
    scalars = [0, 1, 2, X2 - 1, X2, X2 + 1, 1 << 128, R - 1, R - 2, rng.fr(), rng.fr()]
    for k in scalars:
        got = ctx.g1_mul_scalar(words, k)
        plain = ctx.test_g1_mul_scalar_plain(words, k)
        assert np.array_equal(got, plain), hex(k)
        assert list(got[10]) == [0] * 12 + [1], hex(k)
        for i in (0, 7, 20):
            assert list(got[i]) == pyref.g1_words(pyref.G1.mul(pts[i], k)), (hex(k), i)
        if k == 0:
            assert all(list(row) == [0] * 12 + [1] for row in got)
        if k == 1:
            assert np.array_equal(got, words)
    for fn in (ctx.g1_mul_scalar, ctx.test_g1_mul_scalar_plain):
        with pytest.raises(ValueError):
            fn(words, R)
    assert ctx.g1_mul_scalar(np.zeros((0, 13), dtype=np.uint64), 5).shape == (0, 13)


def test_kernel_blocks_and_chunks(zkp, ctx, pyref):
    """300 points: two full 128-lane blocks and a partial one; then chunks of
    100 (three full chunks, each with a partial block); then in place."""
    words = U.words_g1(U.g1_points(300))
    k = pyref.SplitMix64(0xB10C).fr()
    want = ctx.test_g1_mul_scalar_plain(words, k)
    got = ctx.g1_mul_scalar(words, k)
    assert np.array_equal(got, want)
    assert list(got[299]) == pyref.g1_words(pyref.G1.mul(U.g1_points(300)[299], k))
    try:
        ctx.set_option(zkp.ZK_OPT_POINT_CHUNK, 100)
        assert np.array_equal(ctx.g1_mul_scalar(words, k), want)
        assert np.array_equal(ctx.test_g1_mul_scalar_plain(words, k), want)
        buf = words.copy()
        kw = np.array(zkp.to_limbs(k), dtype=np.uint64)
        rc = zkp.lib().zk_g1_mul_scalar(ctypes.c_void_p(ctx._h), zkp._p(buf), ctypes.c_size_t(len(buf)), zkp._p(kw),
                                        zkp._p(buf))
        assert rc == zkp.ZK_OK and np.array_equal(buf, want)
    finally:
        ctx.set_option(zkp.ZK_OPT_POINT_CHUNK, 1 << 20)
    buf = words.copy()
    rc = zkp.lib().zk_g1_mul_scalar(ctypes.c_void_p(ctx._h), zkp._p(buf), ctypes.c_size_t(len(buf)), zkp._p(kw),
                                    zkp._p(buf))
    assert rc == zkp.ZK_OK and np.array_equal(buf, want)


# -------------------------------------------------------------- contribute ---
@pytest.mark.parametrize("which", ["random", "e_is_x2"])
def test_contribute_equals_setup_with_delta_d(zkp, ctx, pyref, case4, qap4, crs4, which):
    """Every array and point of pk and vk; ic_g1 and h_g1 also directly
    against pyref's e * old point (15 multiplications)."""
    d = pyref.SplitMix64(0xD1).fr() if which == "random" else pyref.fr_inv(X2)
    e = pyref.fr_inv(d)
    assert (which == "e_is_x2") == (e == X2)
    before = crs4.copy()
    new = crs4.contribute(ctx, d)
    _same_crs(crs4, before)                                        # the old CRS is untouched
    _same_crs(new, _with_delta(zkp, ctx, qap4, case4["params"], case4["params"][3] * d))
    assert new.pk.sound and new.vk.sound
    assert not np.array_equal(new.pk.point("delta_g1"), crs4.pk.point("delta_g1"))
    for nm in ("ic_g1", "h_g1"):
        old, now = getattr(crs4.pk, nm), getattr(new.pk, nm)
        assert len(old) == len(now)
        for i in range(len(old)):
            assert list(now[i]) == pyref.g1_words(pyref.G1.mul(_g1(pyref, old[i]), e)), (nm, i)


def test_contribute_300_constraints(zkp, ctx, pyref):
    """1411 rescaled points (ic 899 + h 512): many blocks, against the GPU setup alone."""
    qap = zkp.QAP(zkp.CSRMatrices.synthetic(300))
    rng = pyref.SplitMix64(0x300C)
    params = [rng.fr() for _ in range(5)]
    d = rng.fr()
    crs = zkp.CRS.generate_from_qap(ctx, qap, zkp.SetupParams(*params), 1, sound=True)
    assert len(crs.pk.h_g1) == 512 and len(crs.pk.ic_g1) == 899
    _same_crs(crs.contribute(ctx, d), _with_delta(zkp, ctx, qap, params, params[3] * d))


def test_chain(zkp, ctx, pyref, crs4):
    rng = pyref.SplitMix64(0xC4A1)
    d1, d2 = rng.fr(), rng.fr()
    _same_crs(crs4.contribute(ctx, d1).contribute(ctx, d2), crs4.contribute(ctx, d1 * d2 % R))


def test_identity_entries_stay(zkp, ctx, pyref, crs4):
    crs = crs4.copy()
    ident = np.array([0] * 12 + [1], dtype=np.uint64)
    crs.pk.h_g1[1] = ident
    crs.pk.ic_g1[5] = ident
    d = pyref.SplitMix64(0x1DE).fr()
    new = crs.contribute(ctx, d)
    assert np.array_equal(new.pk.h_g1[1], ident) and np.array_equal(new.pk.ic_g1[5], ident)
    ref = crs4.contribute(ctx, d)
    keep_h, keep_ic = [0, 2, 3], [i for i in range(len(ref.pk.ic_g1)) if i != 5]
    assert np.array_equal(new.pk.h_g1[keep_h], ref.pk.h_g1[keep_h])
    assert np.array_equal(new.pk.ic_g1[keep_ic], ref.pk.ic_g1[keep_ic])


def test_end_to_end(zkp, ctx, pyref, case4, crs4):
    new = crs4.contribute(ctx, pyref.SplitMix64(0xE2E).fr())
    w = zkp.Witness(case4["z"], sound_ref.CASE_PUBLIC)
    x = [case4["z"][1]]
    dpk_new, dpk_old = new.pk.upload(ctx), crs4.pk.upload(ctx)
    try:
        assert dpk_new.sound
        p_new = zkp.Prover.prove(dpk_new, w, r=case4["r"], s=case4["s"])
        p_old = zkp.Prover.prove(dpk_old, w, r=case4["r"], s=case4["s"])
    finally:
        dpk_new.free()
        dpk_old.free()
    assert zkp.Verifier.verify(new.vk, p_new, x) is True
    assert zkp.Verifier.verify(crs4.vk, p_old, x) is True
    assert zkp.Verifier.verify(crs4.vk, p_new, x) is False
    assert zkp.Verifier.verify(new.vk, p_old, x) is False


# ------------------------------------------------------ verify_contribution ---
def _coeffs(pyref, n, seed=0xC0EF):
    rng = pyref.SplitMix64(seed)
    return [((rng.next() << 64) | rng.next()) or 1 for _ in range(n)]


def _set_point(field, words):
    for i, w in enumerate(words):
        field.w[i] = int(w)


def test_verify_contribution(zkp, ctx, pyref, crs4):
    d = pyref.SplitMix64(0x7E51).fr()
    good = crs4.contribute(ctx, d)
    nh, nic = len(crs4.pk.h_g1), len(crs4.pk.ic_g1)
    co = _coeffs(pyref, nh + nic)
    V = zkp.CRS.verify_contribution
    assert V(ctx, crs4, good, co) == (True, zkp.ZK_CONTRIB_OK)
    assert V(ctx, crs4, good) == (True, zkp.ZK_CONTRIB_OK)                    # coefficients drawn from `secrets`
    assert V(ctx, crs4, good.contribute(ctx, 3), co) == (True, zkp.ZK_CONTRIB_OK)   # two shares at once: still one delta'

    t = good.copy()
    t.pk.a_g1[3] = t.pk.a_g1[4]
    assert V(ctx, crs4, t, co) == (False, zkp.ZK_CONTRIB_FIXED_PART)

    t = good.copy()
    _set_point(t.vk.s.delta_g2, crs4.vk.point("delta_g2"))
    assert V(ctx, crs4, t, co) == (False, zkp.ZK_CONTRIB_FIXED_PART)

    t = good.copy()
    t.pk.h_g1[2] = pyref.g1_words(U.g1_off_subgroup()[1])
    assert V(ctx, crs4, t, co) == (False, zkp.ZK_CONTRIB_POINT)
    assert "h_g1[2]" in ctx.last_error() and "subgroup" in ctx.last_error()

    t = good.copy()
    other = crs4.contribute(ctx, d + 1)
    _set_point(t.pk.s.delta_g2, other.pk.point("delta_g2"))
    _set_point(t.vk.s.delta_g2, other.pk.point("delta_g2"))
    assert V(ctx, crs4, t, co) == (False, zkp.ZK_CONTRIB_DELTA)

    t = good.copy()
    t.pk.h_g1[1] = ctx.g1_mul_scalar(t.pk.h_g1[1:2], 2)[0]
    assert V(ctx, crs4, t, co) == (False, zkp.ZK_CONTRIB_RATIO)

    t = good.copy()
    t.pk.ic_g1[[2, 7]] = t.pk.ic_g1[[7, 2]]
    assert not np.array_equal(t.pk.ic_g1, good.pk.ic_g1)
    assert V(ctx, crs4, t, co) == (False, zkp.ZK_CONTRIB_RATIO)

    # h'[0] += T, h'[1] -= T: the sum over equal coefficients does not see it
    t = good.copy()
    T = U.g1_points(4)[0]
    t.pk.h_g1[0] = pyref.g1_words(pyref.G1.add(_g1(pyref, good.pk.h_g1[0]), T))
    t.pk.h_g1[1] = pyref.g1_words(pyref.G1.add(_g1(pyref, good.pk.h_g1[1]), pyref.G1.neg(T)))
    assert co[0] != co[1]
    assert V(ctx, crs4, t, co) == (False, zkp.ZK_CONTRIB_RATIO)
    equal = list(co)
    equal[1] = equal[0]
    assert V(ctx, crs4, t, equal) == (True, zkp.ZK_CONTRIB_OK)                # so the coefficients are really used
    assert V(ctx, crs4, good, equal) == (True, zkp.ZK_CONTRIB_OK)

    assert V(ctx, crs4, good, co[:-1]) == (False, zkp.ZK_CONTRIB_SHAPE)
    for bad in (0, 1 << 128):
        with pytest.raises(ValueError):
            V(ctx, crs4, good, co[:4] + [bad] + co[5:])


# ------------------------------------------------------------------ errors ---
def test_errors(zkp, ctx, pyref, qap4, crs4, case4):
    for d in (0, R):
        t = crs4.copy()
        dw = np.array(zkp.to_limbs(d), dtype=np.uint64)
        rc = zkp.lib().zk_groth16_contribute_sound(ctypes.c_void_p(ctx._h), ctypes.byref(t.pk._bind()),
                                                   ctypes.byref(t.vk.s), zkp._p(dw))
        assert rc == zkp.ZK_ERR_ARG
        _same_crs(t, crs4)
        with pytest.raises(zkp.SetupError):
            crs4.contribute(ctx, d)
    ref = zkp.CRS.generate_from_qap(ctx, qap4, zkp.SetupParams(*case4["params"]), sound_ref.CASE_PUBLIC)
    with pytest.raises(zkp.SetupError):
        ref.contribute(ctx, 5)
    with pytest.raises(zkp.SetupError):
        zkp.CRS.verify_contribution(ctx, ref, ref)
