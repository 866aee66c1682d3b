"""CRS.verify_against_srs (csrc/keycheck.hip): is a sound key the key of its
circuit over a powers-of-tau string?  The new kernels and the transform glue
against the big-integer model (key_srs_ref.py) through zk_test_key_srs_coeffs,
then the call itself: what it must accept (keys from the string, down a chain
of contributions, and the trusted setup's independent construction), every
verdict, the errors, and that a call leaves nothing behind on its ctx.

Coefficients are explicit, pairwise distinct and hold 1 and 2^128 - 1, so a swap
of two differing entries changes a sum by (rho_i - rho_j)(P_j - P_i) != 0: it is
caught with certainty, not merely with high probability."""
import ctypes

import numpy as np
import pytest

import key_srs_ref as K
import points_util as U
import sound_ref
import srs_util
from srs_util import same_crs as _same_crs, string as _string

pytestmark = pytest.mark.gpu

R = K.R
L300 = 3          # num_public of the verdict tests: four vk entries, eight private ones


def _qap(zkp, mats, V):
    nc = len(mats[0])
    return zkp.QAP(zkp.CSRMatrices(nc, V, [srs_util.csr(m, nc) for m in mats]))


@pytest.fixture(scope="module")
def case4(pyref):
    return srs_util.case4(pyref)


@pytest.fixture(scope="module")
def circuits(zkp):
    """name -> (product QAP, model rows, V): the n = 4 synthetic case, the
    5-constraint circuit (n = 8), the 300-constraint circuit of
    test_gpu_setup_srs.py (n = 512: two 256-lane blocks, 212 padded rows, a
    column in every row) and the synthetic circuit at 300 constraints with
    *_val == NULL."""
    out = {}
    mats, V = K.synthetic_rows(sound_ref.CASE_N)
    out["syn4"] = (zkp.QAP(zkp.CSRMatrices.synthetic(sound_ref.CASE_N)), mats, V)
    mats, V = K.handmade5()
    out["hand5"] = (_qap(zkp, mats, V), mats, V)
    mats, V = K.handmade300()
    out["hand300"] = (_qap(zkp, mats, V), mats, V)
    mats, V = K.synthetic_rows(300)
    out["syn300"] = (zkp.QAP(zkp.CSRMatrices.synthetic(300)), mats, V)
    return out


@pytest.fixture(scope="module")
def srs9(zkp, ctx, case4):
    return _string(zkp, ctx, case4, 9)


def _coeffs(qap):
    return K.coefficients(qap.num_variables + qap.domain_size)


# ------------------------------------------------ the kernels against the model ---
COEFF_CASES = [(nm, l) for nm in ("syn4", "hand5", "hand300", "syn300") for l in (0, 1, 3)] + [("hand5", 6)]


@pytest.mark.parametrize("name,l", COEFF_CASES, ids=[f"{n}-l{l}" for n, l in COEFF_CASES])
def test_coeffs_against_model(ctx, pyref, circuits, name, l):
    qap, mats, V = circuits[name]
    rho = K.coefficients(V, seed=0xA0 + l)
    rho[-1] = pyref.SplitMix64(0xA1).fr()          # the hook takes any value below r
    assert rho[-1] >> 200
    got = ctx.test_key_srs_coeffs(qap, l, rho)
    want = K.coeff_vectors(mats, V, l, rho, intt=K.intt_fast)
    assert len(got) == 6
    for k, part in enumerate(("A pub", "A priv", "B pub", "B priv", "C pub", "C priv")):
        assert got[k] == want[k], part
    if l == V - 1:
        assert not any(got[1]) and not any(got[3]) and not any(got[5])


def test_coeffs_one_constraint(zkp, ctx):
    """nc = 1: n = 1, the transform is the identity"""
    mats = [[[(0, 3), (1, R - 2)]], [[(2, 5)]], [[(1, 7), (1, 7)]]]
    qap = _qap(zkp, mats, 3)
    assert qap.domain_size == 1
    rho = [1, (1 << 128) - 1, 0x1234567]
    assert ctx.test_key_srs_coeffs(qap, 0, rho) == K.coeff_vectors(mats, 3, 0, rho)
    assert ctx.test_key_srs_coeffs(qap, 0, rho)[1] == [(R - 2) * rho[1] % R]


# --------------------------------------------------------------- it accepts ---
ACCEPT_CASES = [("syn4", 1, 2), ("hand5", 1, 3), ("hand5", 6, 3), ("hand300", L300, 9), ("syn300", 1, 9)]


@pytest.mark.parametrize("name,l,exact", ACCEPT_CASES, ids=[f"{n}-l{l}" for n, l, _ in ACCEPT_CASES])
def test_accepts_keys_from_the_string(zkp, ctx, pyref, case4, circuits, srs9, name, l, exact):
    """a string of exactly the domain's size and a larger one; then down a chain"""
    qap = circuits[name][0]
    assert qap.domain_size == 1 << exact
    co = _coeffs(qap)
    ok = (True, zkp.ZK_KEYSRS_OK)
    crs = zkp.CRS.from_srs(ctx, qap, srs9, l)
    assert len(crs.pk.ic_g1) == qap.num_variables - l - 1
    assert crs.verify_against_srs(ctx, srs9, co) == ok
    if exact != 9:
        assert crs.verify_against_srs(ctx, _string(zkp, ctx, case4, exact), co) == ok
    rng = pyref.SplitMix64(0xCA11 + l)
    for _ in range(2):
        crs = crs.contribute(ctx, rng.fr())
        assert crs.verify_against_srs(ctx, srs9, co) == ok


@pytest.mark.parametrize("name,l", [("syn4", 1), ("hand300", 1)])
def test_accepts_the_trusted_setup(zkp, ctx, pyref, case4, circuits, srs9, name, l):
    """SetupParams(alpha, beta, 1, delta, tau) with a full-width delta: fixed-base
    tables over Lagrange values, no string anywhere"""
    qap = circuits[name][0]
    delta = pyref.SplitMix64(0xDE17A).fr()
    assert delta >> 200
    params = zkp.SetupParams(case4["alpha"], case4["beta"], 1, delta, case4["tau"])
    crs = zkp.CRS.generate_from_qap(ctx, qap, params, l, sound=True)
    assert crs.verify_against_srs(ctx, srs9, _coeffs(qap)) == (True, zkp.ZK_KEYSRS_OK)


def test_drawn_coefficients(zkp, ctx, case4, circuits, srs9):
    qap = circuits["syn4"][0]
    crs = zkp.CRS.from_srs(ctx, qap, srs9, 1).contribute(ctx, 0xD1CE)
    assert crs.verify_against_srs(ctx, srs9) == (True, zkp.ZK_KEYSRS_OK)


# ------------------------------------------------------------- every verdict ---
@pytest.fixture(scope="module")
def good300(zkp, ctx, pyref, circuits, srs9):
    """the 300-constraint key after one contribution, its share, and its coefficients"""
    qap = circuits["hand300"][0]
    d = pyref.SplitMix64(0x600D).fr()
    crs = zkp.CRS.from_srs(ctx, qap, srs9, L300).contribute(ctx, d)
    co = _coeffs(qap)
    assert crs.verify_against_srs(ctx, srs9, co) == (True, zkp.ZK_KEYSRS_OK)
    return crs, d, co


@pytest.fixture(scope="module")
def other_tau(zkp, ctx, case4, circuits, good300):
    """the same circuit, alpha, beta and share over a string of another tau"""
    srs = zkp.SRS.generate(ctx, 9, (case4["tau"] + 1) % R, case4["alpha"], case4["beta"])
    crs = zkp.CRS.from_srs(ctx, circuits["hand300"][0], srs, L300).contribute(ctx, good300[1])
    return srs, crs


def _array(crs, where):
    return crs.vk.ic_g1 if where == "vk.ic_g1" else getattr(crs.pk, where.split(".")[1])


# the array, two entries of it that differ, the verdict
QUERIES = [("pk.a_g1", 1, 2, "QUERY_A"), ("pk.b_g1", 2, 3, "QUERY_B1"), ("pk.b_g2", 2, 3, "QUERY_B2"),
           ("vk.ic_g1", 1, 2, "IC_VK"), ("pk.ic_g1", 0, 1, "IC_PK"), ("pk.h_g1", 2, 7, "H")]


@pytest.mark.parametrize("where,i,j,verdict", QUERIES, ids=[q[3] for q in QUERIES])
def test_query_verdicts(zkp, ctx, srs9, good300, other_tau, where, i, j, verdict):
    good, _, co = good300
    want = (False, getattr(zkp, "ZK_KEYSRS_" + verdict))
    t = good.copy()
    a = _array(t, where)
    assert not np.array_equal(a[i], a[j])
    a[[i, j]] = a[[j, i]]
    assert t.verify_against_srs(ctx, srs9, co) == want
    # the same entry of the key over another tau
    t = good.copy()
    a, b = _array(t, where), _array(other_tau[1], where)
    assert not np.array_equal(a[i], b[i])
    a[i] = b[i]
    assert t.verify_against_srs(ctx, srs9, co) == want


@pytest.mark.parametrize("matrix,row,verdict", [(0, 4, "QUERY_A"), (1, 4, "QUERY_B1"), (2, 0, "IC_VK"),
                                                 (2, 1, "IC_PK")])
def test_another_circuit(zkp, ctx, circuits, srs9, good300, matrix, row, verdict):
    """the key against a circuit with one coefficient of one matrix changed; in
    C row 0 the column is 3 (public at l = 3), in row 1 it is 4 (private)"""
    good, _, co = good300
    _, mats, V = circuits["hand300"]
    changed = [[list(r) for r in m] for m in mats]
    c, v = changed[matrix][row][-1]
    if matrix == 2:
        assert c == 3 + row
    changed[matrix][row][-1] = (c, (v + 1) % R)
    t = good.copy()
    t.pk.qap = _qap(zkp, changed, V)
    assert t.verify_against_srs(ctx, srs9, co) == (False, getattr(zkp, "ZK_KEYSRS_" + verdict))


def _set_point(field, words):
    for i, w in enumerate(words):
        field.w[i] = int(w)


def test_other_verdicts(zkp, ctx, pyref, case4, circuits, srs9, good300, other_tau):
    good, d, co = good300
    qap = circuits["hand300"][0]
    ok, st = good.verify_against_srs(ctx, other_tau[0], co)        # a string of another tau
    assert not ok and st != zkp.ZK_KEYSRS_OK

    # FIXED
    t = good.copy()
    _set_point(t.pk.s.alpha_g1, good.pk.point("beta_g1"))
    assert t.verify_against_srs(ctx, srs9, co) == (False, zkp.ZK_KEYSRS_FIXED)
    gamma = zkp.SetupParams(case4["alpha"], case4["beta"], 5, 7, case4["tau"])
    t = zkp.CRS.generate_from_qap(ctx, qap, gamma, L300, sound=True)
    assert t.verify_against_srs(ctx, srs9, co) == (False, zkp.ZK_KEYSRS_FIXED)
    t = good.copy()
    _set_point(t.vk.s.delta_g2, srs9.tau_g2[0])                     # the generator: delta before the contribution
    assert t.verify_against_srs(ctx, srs9, co) == (False, zkp.ZK_KEYSRS_FIXED)

    # DELTA: delta_g1 of one share, delta_g2 of another
    t = good.copy()
    other = good.contribute(ctx, 3)
    _set_point(t.pk.s.delta_g2, other.pk.point("delta_g2"))
    _set_point(t.vk.s.delta_g2, other.pk.point("delta_g2"))
    assert t.verify_against_srs(ctx, srs9, co) == (False, zkp.ZK_KEYSRS_DELTA)

    # POINT: on the curve, outside the subgroup
    t = good.copy()
    t.pk.h_g1[5] = pyref.g1_words(U.g1_off_subgroup()[1])
    assert t.verify_against_srs(ctx, srs9, co) == (False, zkp.ZK_KEYSRS_POINT)
    assert "pk.h_g1[5]" in ctx.last_error() and "subgroup" in ctx.last_error()

    # SHAPE
    assert good.verify_against_srs(ctx, srs9, co[:-1]) == (False, zkp.ZK_KEYSRS_SHAPE)
    t = good.copy()
    t.vk.s.num_public = L300 + 1
    assert t.verify_against_srs(ctx, srs9, co) == (False, zkp.ZK_KEYSRS_SHAPE)


def _raw(zkp, ctx, crs, srs, coeffs):
    cw = zkp.fr_array(coeffs)
    st = ctypes.c_int(-1)
    rc = zkp.lib().zk_groth16_verify_key_srs_sound(
        ctypes.c_void_p(ctx._h), ctypes.byref(crs.pk.qap.csr.s), ctypes.byref(srs._bind()),
        ctypes.byref(crs.pk._bind()), ctypes.byref(crs.vk.s), zkp._p(cw), ctypes.c_size_t(len(cw)), ctypes.byref(st))
    return rc, st.value


def test_errors_and_no_trace(zkp, ctx, case4, circuits, srs9, good300):
    good, _, co = good300
    qap = circuits["hand300"][0]
    ok = (True, zkp.ZK_KEYSRS_OK)
    for bad in (0, 1 << 128):
        with pytest.raises(ValueError, match="coefficient 4 "):
            good.verify_against_srs(ctx, srs9, co[:4] + [bad] + co[5:])
        rc, _ = _raw(zkp, ctx, good, srs9, co[:4] + [bad] + co[5:])
        assert rc == zkp.ZK_ERR_ARG and "coefficient 4 " in ctx.last_error()
        assert good.verify_against_srs(ctx, srs9, co) == ok          # the ctx still accepts
    assert _raw(zkp, ctx, good, srs9, co) == (zkp.ZK_OK, zkp.ZK_KEYSRS_OK)
    # the SHAPE check comes before the coefficients
    assert _raw(zkp, ctx, good, srs9, [0] + co[2:]) == (zkp.ZK_OK, zkp.ZK_KEYSRS_SHAPE)

    with pytest.raises(zkp.DomainTooSmall):
        good.verify_against_srs(ctx, _string(zkp, ctx, case4, 8), co)
    ref = zkp.CRS.generate_from_qap(ctx, qap, zkp.SetupParams(3, 5, 7, 11, 13), L300)
    with pytest.raises(zkp.SetupError):
        ref.verify_against_srs(ctx, srs9, co)

    # after a rejecting call the same ctx accepts, and builds the trusted key's bytes
    t = good.copy()
    t.pk.a_g1[[1, 2]] = t.pk.a_g1[[2, 1]]
    assert t.verify_against_srs(ctx, srs9, co) == (False, zkp.ZK_KEYSRS_QUERY_A)
    assert good.verify_against_srs(ctx, srs9, co) == ok
    _same_crs(zkp.CRS.from_srs(ctx, qap, srs9, L300), srs_util.trusted(zkp, ctx, qap, case4, L300))
