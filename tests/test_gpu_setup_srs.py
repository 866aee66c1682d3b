"""A sound key from a powers-of-tau string (csrc/srs.hip): CRS.from_srs must
give, entry for entry and byte for byte, the key of the sound setup for
(alpha, beta, gamma = 1, delta = 1, tau) -- an independent path (Lagrange values
over Fr and fixed-base tables), itself pinned to tests/sound_ref.py.  Then the
key under contributions and proofs, the errors, and every verdict of
SRS.verify."""
import ctypes

import numpy as np
import pytest

import points_util as U
import sound_ref
import srs_util
from srs_util import PK_ARRAYS, csr as _csr, same_crs as _same_crs, string as _string, trusted as _trusted

pytestmark = pytest.mark.gpu

R = sound_ref.R


@pytest.fixture(scope="module")
def case4(pyref):
    return srs_util.case4(pyref)


@pytest.fixture(scope="module")
def qap4(zkp):
    return zkp.QAP(zkp.CSRMatrices.synthetic(sound_ref.CASE_N))


@pytest.fixture(scope="module")
def srs2(zkp, ctx, case4):
    return _string(zkp, ctx, case4, 2)


# ------------------------------------------------------------------ the key ---
@pytest.mark.parametrize("log_n", [2, 5])
def test_synthetic_n4(zkp, ctx, case4, qap4, log_n):
    """a string of exactly the circuit's size, and a larger one (n < N)"""
    srs = _string(zkp, ctx, case4, log_n)
    crs = zkp.CRS.from_srs(ctx, qap4, srs, sound_ref.CASE_PUBLIC)
    assert crs.pk.sound and crs.vk.sound
    _same_crs(crs, _trusted(zkp, ctx, qap4, case4, sound_ref.CASE_PUBLIC))


def _csr(rows, nc):
    """rows: per constraint a list of (col, coeff), duplicates kept"""
    rp, cols, vals = [0], [], []
    for i in range(nc):
        for c, v in rows[i]:
            cols.append(c)
            vals.append([(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)])
        rp.append(len(cols))
    return (np.array(rp, dtype=np.uint64), np.array(cols, dtype=np.uint32),
            np.array(vals, dtype=np.uint64).reshape(-1, 4))


@pytest.fixture(scope="module")
def handmade(zkp, pyref):
    """300 constraints (n = 512, 212 padded rows), 12 variables.  A: variable 0
    in every row (a column longer than any run and than a wave), the
    coefficients 1, r - 1, 2 and a full-width one on variables 1..5, variable 7
    nowhere, variable 8 only as the pair 5, r - 5 on one (row, col) -- it
    cancels --, variable 9 as the pair 5, 3 on one (row, col).  C: variable 0 in
    every row too."""
    rng = pyref.SplitMix64(0x300)
    wide = rng.fr()
    assert wide >> 200
    coef = [1, R - 1, 2, wide]
    nc, V = 300, 12
    A = [[(0, 1), (1 + i % 5, coef[i % 4])] for i in range(nc)]
    A[10] += [(8, 5), (8, R - 5)]
    A[11] += [(9, 5), (9, 3)]
    B = [[(2 + i % 6, coef[(i + 1) % 4])] for i in range(nc)]
    B[7].append((7, wide))
    Cm = [[(0, 1), (3 + i % 8, rng.fr() if i % 16 == 0 else coef[(i + 2) % 4])] for i in range(nc)]
    csr = zkp.CSRMatrices(nc, V, [_csr(A, nc), _csr(B, nc), _csr(Cm, nc)])
    return zkp.QAP(csr)


@pytest.fixture(scope="module")
def srs9(zkp, ctx, case4):
    return _string(zkp, ctx, case4, 9)


@pytest.mark.parametrize("num_public", [0, 1, 3])
def test_handmade_300(zkp, ctx, case4, handmade, srs9, num_public):
    assert handmade.domain_size == 512
    crs = zkp.CRS.from_srs(ctx, handmade, srs9, num_public)
    _same_crs(crs, _trusted(zkp, ctx, handmade, case4, num_public))
    ident = [0] * 12 + [1]
    assert list(crs.pk.a_g1[7]) == ident and list(crs.pk.a_g1[8]) == ident
    assert list(crs.pk.a_g1[9]) != ident and list(crs.pk.a_g1[0]) != ident


def test_run_lengths_agree(zkp, ctx, case4, handmade, srs9):
    """ZK_OPT_SRS_RUN: runs of 1 and of 7 entries (43 runs in the long columns)
    give the default's bytes."""
    want = zkp.CRS.from_srs(ctx, handmade, srs9, 1)
    try:
        for run in (1, 7):
            ctx.set_option(zkp.ZK_OPT_SRS_RUN, run)
            _same_crs(zkp.CRS.from_srs(ctx, handmade, srs9, 1), want)
    finally:
        ctx.set_option(zkp.ZK_OPT_SRS_RUN, 0)


def test_unit_and_mixed_values(zkp, ctx, pyref, case4, srs9):
    """The synthetic circuit at 300 constraints: *_val == NULL everywhere (the
    all-ones path), then with B's values spelled out (A and C still NULL: the
    mixed ic sum fills in the ones)."""
    syn = zkp.CSRMatrices.synthetic(300)
    qap = zkp.QAP(syn)
    want = _trusted(zkp, ctx, qap, case4, 1)
    _same_crs(zkp.CRS.from_srs(ctx, qap, srs9, 1), want)
    ones = np.zeros((300, 4), dtype=np.uint64)
    ones[:, 0] = 1
    mats = [syn.mats[0], (syn.mats[1][0], syn.mats[1][1], ones), syn.mats[2]]
    _same_crs(zkp.CRS.from_srs(ctx, zkp.QAP(zkp.CSRMatrices(300, 901, mats)), srs9, 1), want)


def test_end_to_end(zkp, ctx, pyref, case4, qap4, srs2):
    """from_srs -> two contributions, each accepted -> upload -> prove -> verify"""
    crs0 = zkp.CRS.from_srs(ctx, qap4, srs2, sound_ref.CASE_PUBLIC)
    rng = pyref.SplitMix64(0xE2E5)
    crs1 = crs0.contribute(ctx, rng.fr())
    assert zkp.CRS.verify_contribution(ctx, crs0, crs1) == (True, zkp.ZK_CONTRIB_OK)
    crs2 = crs1.contribute(ctx, rng.fr())
    assert zkp.CRS.verify_contribution(ctx, crs1, crs2) == (True, zkp.ZK_CONTRIB_OK)
    dpk = crs2.pk.upload(ctx)
    try:
        assert dpk.sound
        proof = zkp.Prover.prove(dpk, zkp.Witness(case4["z"], sound_ref.CASE_PUBLIC), r=case4["r"], s=case4["s"])
    finally:
        dpk.free()
    x = case4["z"][1]
    assert zkp.Verifier.verify(crs2.vk, proof, [x]) is True
    assert zkp.Verifier.verify(crs2.vk, proof, [(x + 1) % R]) is False
    assert zkp.Verifier.verify(crs0.vk, proof, [x]) is False


# ------------------------------------------------------------------ errors ---
def _raw_setup(zkp, ctx, qap, srs, num_public):
    """the C call on keys filled with a pattern -> (rc, every output untouched)"""
    pk = zkp.ProvingKey(qap.num_variables, qap.domain_size, min(num_public, qap.num_variables - 1), qap, True)
    vk = zkp.VerificationKey(min(num_public, qap.num_variables - 1), True)
    arrays = [getattr(pk, nm) for nm in PK_ARRAYS] + [vk.ic_g1]
    for a in arrays:
        a[:] = 0xA5A5A5A5
    pk._bind()
    before_pk, before_vk = bytes(pk.s), bytes(vk.s)
    rc = zkp.lib().zk_groth16_setup_srs_sound(ctypes.c_void_p(ctx._h), ctypes.byref(qap.csr.s),
                                              ctypes.byref(srs._bind()), ctypes.c_uint64(num_public),
                                              ctypes.byref(pk.s), ctypes.byref(vk.s))
    same = all((a == 0xA5A5A5A5).all() for a in arrays) and bytes(pk.s) == before_pk and bytes(vk.s) == before_vk
    return rc, same


def test_errors(zkp, ctx, pyref, case4, qap4, srs2):
    small = _string(zkp, ctx, case4, 1)
    with pytest.raises(zkp.DomainTooSmall):
        zkp.CRS.from_srs(ctx, qap4, small, 1)
    assert _raw_setup(zkp, ctx, qap4, small, 1) == (zkp.ZK_ERR_DOMAIN, True)

    short = srs2.copy()
    short.tau_g1 = short.tau_g1[:7]
    assert _raw_setup(zkp, ctx, qap4, short, 1) == (zkp.ZK_ERR_DOMAIN, True)

    on_domain = zkp.SRS.generate(ctx, 2, pyref.root_of_unity(4), case4["alpha"], case4["beta"])
    with pytest.raises(zkp.SetupError, match="evaluation domain"):
        zkp.CRS.from_srs(ctx, qap4, on_domain, 1)
    assert _raw_setup(zkp, ctx, qap4, on_domain, 1) == (zkp.ZK_ERR_SETUP_PARAMS, True)

    with pytest.raises(zkp.SetupError):
        zkp.CRS.from_srs(ctx, qap4, srs2, qap4.num_variables)
    assert _raw_setup(zkp, ctx, qap4, srs2, qap4.num_variables) == (zkp.ZK_ERR_SETUP_PARAMS, True)
    assert _raw_setup(zkp, ctx, qap4, srs2, 1) == (zkp.ZK_OK, False)

    for bad in (0, R):
        with pytest.raises(zkp.SetupError):
            zkp.SRS.generate(ctx, 2, bad, 5, 7)
    s = zkp.SRS(2)
    h = ctypes.c_void_p(ctx._h)
    fr = lambda v: ctypes.byref(zkp._Fr((ctypes.c_uint64 * 4)(*zkp.to_limbs(v))))
    assert zkp.lib().zk_srs_generate(h, ctypes.c_uint32(2), fr(0), fr(5), fr(7), ctypes.byref(s._bind())) == \
        zkp.ZK_ERR_SETUP_PARAMS
    assert zkp.lib().zk_srs_generate(h, ctypes.c_uint32(2), fr(3), fr(R), fr(7), ctypes.byref(s._bind())) == \
        zkp.ZK_ERR_ARG


# -------------------------------------------------------------- SRS.verify ---
def _coeffs(pyref, n, seed=0x5125):
    rng = pyref.SplitMix64(seed)
    return [((rng.next() << 64) | rng.next()) or 1 for _ in range(n)]


def test_srs_verify(zkp, ctx, pyref, case4):
    srs = _string(zkp, ctx, case4, 4)
    tau, beta = case4["tau"], case4["beta"]
    co = _coeffs(pyref, 32)
    assert srs.verify(ctx, co) == (True, zkp.ZK_SRS_OK)
    assert srs.verify(ctx) == (True, zkp.ZK_SRS_OK)                      # coefficients drawn from `secrets`

    t = srs.copy()
    t.tau_g1[21] = ctx.g1_mul_scalar(t.tau_g1[21:22], 2)[0]
    assert t.verify(ctx, co) == (False, zkp.ZK_SRS_POWERS_G1)

    t = srs.copy()
    t.tau_g2[3] = ctx.test_fixed_base([2 * pow(tau, 3, R) % R], g2=True)[0]
    assert t.verify(ctx, co) == (False, zkp.ZK_SRS_POWERS_G2)

    t = srs.copy()
    t.alpha_tau_g1[3] = t.tau_g1[3]
    assert t.verify(ctx, co) == (False, zkp.ZK_SRS_ALPHA)

    t = srs.copy()
    t.beta_tau_g1[3] = t.tau_g1[3]
    assert t.verify(ctx, co) == (False, zkp.ZK_SRS_BETA)

    t = srs.copy()
    t.beta_g2 = ctx.test_fixed_base([2 * beta % R], g2=True)[0]
    assert t.verify(ctx, co) == (False, zkp.ZK_SRS_BETA)

    t = srs.copy()
    t.tau_g1[0] = ctx.test_fixed_base([2])[0]
    assert t.verify(ctx, co) == (False, zkp.ZK_SRS_GENERATOR)

    t = srs.copy()
    t.alpha_tau_g1[5] = [0] * 12 + [1]
    assert t.verify(ctx, co) == (False, zkp.ZK_SRS_POINT)
    assert "alpha_tau_g1[5]" in ctx.last_error() and "identity" in ctx.last_error()

    t = srs.copy()
    t.tau_g1[9] = pyref.g1_words(U.g1_off_subgroup()[1])
    assert t.verify(ctx, co) == (False, zkp.ZK_SRS_POINT)
    assert "tau_g1[9]" in ctx.last_error() and "subgroup" in ctx.last_error()

    t = srs.copy()
    t.tau_g2[2] = pyref.g2_words(U.g2_off_subgroup()[0])
    assert t.verify(ctx, co) == (False, zkp.ZK_SRS_POINT)
    assert "tau_g2[2]" in ctx.last_error()

    t = srs.copy()
    t.tau_g1 = t.tau_g1[:-1]
    assert t.verify(ctx, co) == (False, zkp.ZK_SRS_SHAPE)
    st = ctypes.c_int(-1)
    cw = zkp.fr_array(co[:-1])
    rc = zkp.lib().zk_srs_verify(ctypes.c_void_p(ctx._h), ctypes.byref(srs._bind()), zkp._p(cw),
                                 ctypes.c_size_t(len(cw)), ctypes.byref(st))
    assert (rc, st.value) == (zkp.ZK_OK, zkp.ZK_SRS_SHAPE)
    cw = zkp.fr_array(co[:4] + [1 << 128] + co[5:])
    rc = zkp.lib().zk_srs_verify(ctypes.c_void_p(ctx._h), ctypes.byref(srs._bind()), zkp._p(cw),
                                 ctypes.c_size_t(len(cw)), ctypes.byref(st))
    assert rc == zkp.ZK_ERR_ARG
