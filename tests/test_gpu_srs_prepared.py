"""Prepared powers-of-tau strings (csrc/lagrange.hip): SRS.prepare once per
domain size, then CRS.from_prepared / from_prepared_device per circuit.  The
reference for key bytes is the trusted sound setup for (alpha, beta, 1, 1, tau)
(srs_util.trusted), an independent path; equality with CRS.from_srs is asserted
in addition.  Then export / import, every verdict of LagrangeSRS.verify, the
device key, and a contribution on top of a key from a prepared string."""
import ctypes

import numpy as np
import pytest

import points_util as U
import sound_ref
import srs_util
from srs_util import PK_ARRAYS, csr as _csr, same_crs as _same_crs, string as _string, trusted as _trusted

pytestmark = pytest.mark.gpu

R = sound_ref.R
LAG_ARRAYS = ("l_g1", "alpha_l_g1", "beta_l_g1", "h_g1", "l_g2")
LAG_POINTS = ("alpha_g1", "beta_g1", "beta_g2")


def _same_lag(a, b):
    assert a.log_n == b.log_n
    for nm in LAG_ARRAYS + LAG_POINTS:
        assert np.array_equal(getattr(a, nm), getattr(b, nm)), nm


# ---------------------------------------------------------------- fixtures ---
@pytest.fixture(scope="module")
def case4(pyref):
    return srs_util.case4(pyref)


@pytest.fixture(scope="module")
def qap4(zkp):
    return zkp.QAP(zkp.CSRMatrices.synthetic(sound_ref.CASE_N))


@pytest.fixture(scope="module")
def srs2(zkp, ctx, case4):
    return _string(zkp, ctx, case4, 2)


@pytest.fixture(scope="module")
def srs9(zkp, ctx, case4):
    return _string(zkp, ctx, case4, 9)


@pytest.fixture(scope="module")
def prep9(ctx, srs9):
    p = srs9.prepare(ctx)
    yield p
    p.free()


@pytest.fixture(scope="module")
def lag9(prep9):
    return prep9.export()


@pytest.fixture(scope="module")
def handmade(zkp, pyref):
    """300 constraints (n = 512, 212 padded rows), 12 variables, SATISFIED by
    the witness that comes with it.  A: variable 0 in every row (a column longer
    than any run and than a wave), the coefficients 1, r - 1, 2 and a full-width
    one on variables 1..5, variable 8 only as the pair 5, r - 5 on one
    (row, col) -- it cancels, an identity base --, variable 9 as the pair 5, 3
    on one (row, col).  Variables 10 and 11 appear nowhere.  C: variable 0 in
    every row too, and per row the full-width coefficient that makes the row
    hold for z.  -> (qap, z)"""
    rng = pyref.SplitMix64(0x301)
    wide = rng.fr()
    assert wide >> 200
    coef = [1, R - 1, 2, wide]
    nc, V = 300, 12
    z = [1] + [rng.fr() or 1 for _ in range(V - 1)]
    A = [[(0, 1), (1 + i % 5, coef[i % 4])] for i in range(nc)]
    A[10] += [(8, 5), (8, R - 5)]
    A[11] += [(9, 5), (9, 3)]
    B = [[(2 + i % 6, coef[(i + 1) % 4])] for i in range(nc)]
    B[7].append((7, wide))
    dot = lambda row: sum(v * z[c] for c, v in row) % R
    Cm = []
    for i in range(nc):
        c = 3 + i % 7
        Cm.append([(0, 1), (c, (dot(A[i]) * dot(B[i]) - 1) * pow(z[c], R - 2, R) % R)])
        assert dot(A[i]) * dot(B[i]) % R == dot(Cm[i])
    csr = zkp.CSRMatrices(nc, V, [_csr(A, nc), _csr(B, nc), _csr(Cm, nc)])
    return zkp.QAP(csr), z


# ------------------------------------------------------------------- keys ---
@pytest.mark.parametrize("log_n", [2, 5])
def test_synthetic_n4(zkp, ctx, case4, qap4, log_n):
    """a string of exactly the circuit's size, and a larger one prepared at
    log_n = 2 (n < N)"""
    srs = _string(zkp, ctx, case4, log_n)
    prep = srs.prepare(ctx, 2)
    try:
        assert (prep.log_n, prep.domain_size) == (2, 4)
        assert prep.device_bytes == 4 * (3 * 96 + 192 + 96)
        crs = zkp.CRS.from_prepared(ctx, qap4, prep, sound_ref.CASE_PUBLIC)
    finally:
        prep.free()
    assert crs.pk.sound and crs.vk.sound
    _same_crs(crs, _trusted(zkp, ctx, qap4, case4, sound_ref.CASE_PUBLIC))
    _same_crs(crs, zkp.CRS.from_srs(ctx, qap4, srs, sound_ref.CASE_PUBLIC))


@pytest.mark.parametrize("num_public", [0, 1, 3])
def test_handmade_300(zkp, ctx, case4, handmade, srs9, prep9, num_public):
    qap, _ = handmade
    assert qap.domain_size == 512 and prep9.domain_size == 512
    assert prep9.device_bytes == 512 * (3 * 96 + 192 + 96)
    crs = zkp.CRS.from_prepared(ctx, qap, prep9, num_public)
    _same_crs(crs, _trusted(zkp, ctx, qap, case4, num_public))
    _same_crs(crs, zkp.CRS.from_srs(ctx, qap, srs9, num_public))
    ident = [0] * 12 + [1]
    assert list(crs.pk.a_g1[8]) == ident and list(crs.pk.a_g1[10]) == ident
    assert list(crs.pk.a_g1[9]) != ident and list(crs.pk.a_g1[0]) != ident


def test_unit_and_mixed_values(zkp, ctx, case4, prep9):
    """The synthetic circuit at 300 constraints: *_val == NULL everywhere, then
    with B's values spelled out (the mixed ic sum fills in the ones)."""
    syn = zkp.CSRMatrices.synthetic(300)
    qap = zkp.QAP(syn)
    want = _trusted(zkp, ctx, qap, case4, 1)
    _same_crs(zkp.CRS.from_prepared(ctx, qap, prep9, 1), want)
    ones = np.zeros((300, 4), dtype=np.uint64)
    ones[:, 0] = 1
    mats = [syn.mats[0], (syn.mats[1][0], syn.mats[1][1], ones), syn.mats[2]]
    _same_crs(zkp.CRS.from_prepared(ctx, zkp.QAP(zkp.CSRMatrices(300, 901, mats)), prep9, 1), want)


def test_run_lengths_agree(zkp, ctx, handmade, prep9):
    """ZK_OPT_SRS_RUN 1 and 7 give the default's bytes through the prepared path"""
    qap, _ = handmade
    want = zkp.CRS.from_prepared(ctx, qap, prep9, 1)
    try:
        for run in (1, 7):
            ctx.set_option(zkp.ZK_OPT_SRS_RUN, run)
            _same_crs(zkp.CRS.from_prepared(ctx, qap, prep9, 1), want)
    finally:
        ctx.set_option(zkp.ZK_OPT_SRS_RUN, 0)


def test_synthetic_4096_in_chunks(zkp, ctx, case4):
    """n = 2^12: several workgroups in every kernel, and export and import in
    more than one ZK_OPT_POINT_CHUNK piece (1000 points)."""
    qap = zkp.QAP(zkp.CSRMatrices.synthetic(3000))
    assert qap.domain_size == 4096
    srs = _string(zkp, ctx, case4, 12)
    want = _trusted(zkp, ctx, qap, case4, 1)
    prep = srs.prepare(ctx)
    try:
        _same_crs(zkp.CRS.from_prepared(ctx, qap, prep, 1), want)
        whole = prep.export()
        ctx.set_option(zkp.ZK_OPT_POINT_CHUNK, 1000)
        lag = prep.export()
        _same_lag(lag, whole)
        again = lag.upload(ctx)
        try:
            _same_crs(zkp.CRS.from_prepared(ctx, qap, again, 1), want)
        finally:
            again.free()
    finally:
        ctx.set_option(zkp.ZK_OPT_POINT_CHUNK, 1 << 20)
        prep.free()


def test_one_handle_many_circuits(zkp, ctx, case4, handmade, prep9, lag9):
    """three circuits of n = 512 from one handle, which stays what it was"""
    for qap, l in ((handmade[0], 2), (zkp.QAP(zkp.CSRMatrices.synthetic(400)), 1),
                   (zkp.QAP(zkp.CSRMatrices.synthetic(512)), 4)):
        assert qap.domain_size == 512
        _same_crs(zkp.CRS.from_prepared(ctx, qap, prep9, l), _trusted(zkp, ctx, qap, case4, l))
    _same_lag(prep9.export(), lag9)


# ------------------------------------------------------------- wrong size ---
def _raw_setup(zkp, ctx, qap, prep, num_public):
    """the C call on keys filled with a pattern -> (rc, every output untouched)"""
    pk = zkp.ProvingKey(qap.num_variables, qap.domain_size, min(num_public, qap.num_variables - 1), qap, True)
    vk = zkp.VerificationKey(min(num_public, qap.num_variables - 1), True)
    arrays = [getattr(pk, nm) for nm in PK_ARRAYS] + [vk.ic_g1]
    for a in arrays:
        a[:] = 0xA5A5A5A5
    pk._bind()
    before_pk, before_vk = bytes(pk.s), bytes(vk.s)
    rc = zkp.lib().zk_groth16_setup_prepared_sound(ctypes.c_void_p(ctx._h), ctypes.byref(qap.csr.s),
                                                   ctypes.c_void_p(prep._h), ctypes.c_uint64(num_public),
                                                   ctypes.byref(pk.s), ctypes.byref(vk.s))
    same = all((a == 0xA5A5A5A5).all() for a in arrays) and bytes(pk.s) == before_pk and bytes(vk.s) == before_vk
    return rc, same


def test_wrong_size_and_errors(zkp, ctx, pyref, case4, qap4, srs2, prep9, handmade):
    small = zkp.QAP(zkp.CSRMatrices.synthetic(200))
    assert small.domain_size == 256
    with pytest.raises(zkp.DomainTooSmall, match="256.*512"):
        zkp.CRS.from_prepared(ctx, small, prep9, 1)
    assert _raw_setup(zkp, ctx, small, prep9, 1) == (zkp.ZK_ERR_DOMAIN, True)
    with pytest.raises(zkp.DomainTooSmall):
        zkp.CRS.from_prepared_device(ctx, small, prep9, 1)
    h = ctypes.c_void_p(0)
    rc = zkp.lib().zk_groth16_setup_prepared_sound_dev(ctypes.c_void_p(ctx._h), ctypes.byref(small.csr.s),
                                                       ctypes.c_void_p(prep9._h), ctypes.c_uint64(1), ctypes.byref(h),
                                                       None)
    assert (rc, h.value) == (zkp.ZK_ERR_DOMAIN, None)

    qap = handmade[0]
    with pytest.raises(zkp.SetupError):
        zkp.CRS.from_prepared(ctx, qap, prep9, qap.num_variables)
    assert _raw_setup(zkp, ctx, qap, prep9, qap.num_variables) == (zkp.ZK_ERR_SETUP_PARAMS, True)
    assert _raw_setup(zkp, ctx, qap, prep9, 1) == (zkp.ZK_OK, False)

    with pytest.raises(zkp.DomainTooSmall):
        srs2.prepare(ctx, 3)
    out = ctypes.c_void_p(0)
    rc = zkp.lib().zk_srs_prepare(ctypes.c_void_p(ctx._h), ctypes.byref(srs2._bind()), ctypes.c_uint32(3),
                                  ctypes.byref(out))
    assert (rc, out.value) == (zkp.ZK_ERR_DOMAIN, None)
    short = srs2.copy()
    short.tau_g1 = short.tau_g1[:7]
    with pytest.raises(zkp.DomainTooSmall):
        short.prepare(ctx)

    on_domain = zkp.SRS.generate(ctx, 2, pyref.root_of_unity(4), case4["alpha"], case4["beta"])
    with pytest.raises(zkp.SetupError, match="evaluation domain"):
        on_domain.prepare(ctx)
    rc = zkp.lib().zk_srs_prepare(ctypes.c_void_p(ctx._h), ctypes.byref(on_domain._bind()), ctypes.c_uint32(2),
                                  ctypes.byref(out))
    assert (rc, out.value) == (zkp.ZK_ERR_SETUP_PARAMS, None)


# ------------------------------------------------------- export and import ---
def test_export_is_the_lagrange_basis(zkp, ctx, pyref, case4):
    """n = 8: every exported entry against [L_i(tau)], [alpha L_i(tau)],
    [beta L_i(tau)] in both groups and [tau^i (tau^n - 1)]_1, from the known
    secrets in big integers and pyref's curve arithmetic."""
    n = 8
    tau, alpha, beta = case4["tau"], case4["alpha"], case4["beta"]
    srs = _string(zkp, ctx, case4, 4)
    prep = srs.prepare(ctx, 3)
    try:
        lag = prep.export()
    finally:
        prep.free()
    w = pyref.root_of_unity(n)
    zt = (pow(tau, n, R) - 1) % R
    L = [zt * pow(w, i, R) % R * pow(n * (tau - pow(w, i, R)) % R, R - 2, R) % R for i in range(n)]
    assert sum(L) % R == 1
    g1 = lambda k: list(pyref.g1_words(pyref.G1.mul(pyref.G1.gen, k % R)))
    g2 = lambda k: list(pyref.g2_words(pyref.G2.mul(pyref.G2.gen, k % R)))
    for i in range(n):
        assert list(lag.l_g1[i]) == g1(L[i]), i
        assert list(lag.alpha_l_g1[i]) == g1(alpha * L[i]), i
        assert list(lag.beta_l_g1[i]) == g1(beta * L[i]), i
        assert list(lag.l_g2[i]) == g2(L[i]), i
        assert list(lag.h_g1[i]) == g1(pow(tau, i, R) * zt), i
    assert list(lag.alpha_g1) == g1(alpha) and list(lag.beta_g1) == g1(beta) and list(lag.beta_g2) == g2(beta)
    assert np.array_equal(lag.alpha_g1, srs.alpha_tau_g1[0]) and np.array_equal(lag.beta_g2, srs.beta_g2)


def test_export_upload_keys_identical(zkp, ctx, case4, handmade, prep9, lag9):
    qap = handmade[0]
    again = lag9.upload(ctx)
    try:
        assert again.log_n == 9 and again.device_bytes == prep9.device_bytes
        _same_crs(zkp.CRS.from_prepared(ctx, qap, again, 1), zkp.CRS.from_prepared(ctx, qap, prep9, 1))
        _same_lag(again.export(), lag9)
    finally:
        again.free()
    short = lag9.copy()
    short.l_g2 = short.l_g2[:-1]
    with pytest.raises(ValueError):
        short.upload(ctx)


# ------------------------------------------------------------------ verify ---
def _coeffs(pyref, n, seed=0x1A6):
    rng = pyref.SplitMix64(seed)
    return [((rng.next() << 64) | rng.next()) or 1 for _ in range(n)]


def _bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


@pytest.fixture(scope="module")
def lag2(ctx, srs2):
    p = srs2.prepare(ctx)
    try:
        return p.export()
    finally:
        p.free()


@pytest.fixture(scope="module", params=[2, 9])
def honest(request, srs2, srs9, lag2, lag9):
    return (srs2, lag2) if request.param == 2 else (srs9, lag9)


def test_verify_accepts_the_honest_export(zkp, ctx, pyref, honest):
    srs, lag = honest
    n = 1 << lag.log_n
    assert lag.verify(ctx, srs, _coeffs(pyref, n)) == (True, zkp.ZK_LAG_OK)
    assert lag.verify(ctx, srs) == (True, zkp.ZK_LAG_OK)                 # coefficients drawn from `secrets`
    assert lag.verify(ctx, srs, [1] * n) == (True, zkp.ZK_LAG_OK)


def test_verify_from_a_larger_string(zkp, ctx, pyref, case4, lag2):
    """the string may serve more than the prepared size (n < N)"""
    assert lag2.verify(ctx, _string(zkp, ctx, case4, 4), _coeffs(pyref, 4)) == (True, zkp.ZK_LAG_OK)


def test_verify_verdicts(zkp, ctx, pyref, case4, honest):
    srs, lag = honest
    log_n = lag.log_n
    n = 1 << log_n
    co = _coeffs(pyref, n)
    gen1, gen2 = pyref.g1_words(pyref.G1.gen), pyref.g2_words(pyref.G2.gen)

    def verdict(change):
        t = lag.copy()
        change(t)
        ok, st = t.verify(ctx, srs, co)
        assert ok == (st == zkp.ZK_LAG_OK)
        return st

    def shorten(t):
        t.beta_l_g1 = t.beta_l_g1[:-1]
    assert verdict(shorten) == zkp.ZK_LAG_SHAPE

    def off_curve(t):
        t.l_g1[3, 6] ^= np.uint64(1)
    assert verdict(off_curve) == zkp.ZK_LAG_POINT
    assert "l_g1[3]" in ctx.last_error()

    def off_subgroup_g1(t):
        t.h_g1[1] = pyref.g1_words(U.g1_off_subgroup()[1])
    assert verdict(off_subgroup_g1) == zkp.ZK_LAG_POINT
    assert "h_g1[1]" in ctx.last_error() and "subgroup" in ctx.last_error()

    def off_subgroup_g2(t):
        t.l_g2[2] = pyref.g2_words(U.g2_off_subgroup()[0])
    assert verdict(off_subgroup_g2) == zkp.ZK_LAG_POINT
    assert "l_g2[2]" in ctx.last_error()

    def identity(t):
        t.alpha_l_g1[n - 1] = [0] * 12 + [1]
    assert verdict(identity) == zkp.ZK_LAG_POINT
    assert "alpha_l_g1[%d]" % (n - 1) in ctx.last_error() and "identity" in ctx.last_error()

    def fixed(t):
        t.alpha_g1 = ctx.g1_mul_scalar(t.alpha_g1.reshape(1, -1), 2)[0]
    assert verdict(fixed) == zkp.ZK_LAG_FIXED

    def swap(t):
        t.l_g1[[1, 2]] = t.l_g1[[2, 1]]
    assert verdict(swap) == zkp.ZK_LAG_LAGRANGE_G1

    def bit_reversed(t):
        t.l_g1 = np.ascontiguousarray(t.l_g1[[_bitrev(i, log_n) for i in range(n)]])
    assert verdict(bit_reversed) == zkp.ZK_LAG_LAGRANGE_G1

    def doubled(t):
        t.l_g1 = ctx.g1_mul_scalar(t.l_g1, 2)
    assert verdict(doubled) == zkp.ZK_LAG_LAGRANGE_G1

    other = zkp.SRS.generate(ctx, log_n, (case4["tau"] + 1) % R, case4["alpha"], case4["beta"])
    p = other.prepare(ctx)
    try:
        foreign = p.export()
    finally:
        p.free()
    assert foreign.verify(ctx, other, co) == (True, zkp.ZK_LAG_OK)
    assert foreign.verify(ctx, srs, co) == (False, zkp.ZK_LAG_LAGRANGE_G1)

    def alpha(t):
        t.alpha_l_g1[2] = t.l_g1[2]
    assert verdict(alpha) == zkp.ZK_LAG_ALPHA

    def beta(t):
        t.beta_l_g1[n - 2] = t.l_g1[n - 2]
    assert verdict(beta) == zkp.ZK_LAG_BETA

    def g2_entry(t):
        t.l_g2[1] = gen2
    assert verdict(g2_entry) == zkp.ZK_LAG_LAGRANGE_G2

    def h_entry(t):
        t.h_g1[2] = t.h_g1[3]
    assert verdict(h_entry) == zkp.ZK_LAG_H
    assert "h_g1[2]" in ctx.last_error()
    assert not np.array_equal(lag.l_g1[0], gen1)


def test_verify_bad_coefficients(zkp, ctx, pyref, srs2, lag2):
    co = _coeffs(pyref, 4)
    for bad in (co[:1] + [0] + co[2:], co[:3] + [1 << 128], co[:3], co + [5]):
        with pytest.raises(ValueError):
            lag2.verify(ctx, srs2, bad)
    st = ctypes.c_int(-1)

    def raw(values):
        cw = zkp.fr_array(values)
        rc = zkp.lib().zk_srs_lagrange_verify(ctypes.c_void_p(ctx._h), ctypes.byref(srs2._bind()),
                                              ctypes.byref(lag2._bind()), zkp._p(cw), ctypes.c_size_t(len(cw)),
                                              ctypes.byref(st))
        return rc, st.value
    assert raw(co[:1] + [0] + co[2:])[0] == zkp.ZK_ERR_ARG
    assert raw(co[:3] + [1 << 128])[0] == zkp.ZK_ERR_ARG
    assert raw(co[:3]) == (zkp.ZK_OK, zkp.ZK_LAG_SHAPE)
    assert raw(co) == (zkp.ZK_OK, zkp.ZK_LAG_OK)


# -------------------------------------------------------------- device key ---
def _device_z(z_rows):
    import torch
    return torch.from_numpy(np.ascontiguousarray(z_rows).view(np.int64).copy()).cuda()


def _device_key_agrees(zkp, ctx, pyref, qap, z, srs, prep, num_public):
    rng = pyref.SplitMix64(0xDE7)
    r, s = rng.fr(), rng.fr()
    crs = zkp.CRS.from_srs(ctx, qap, srs, num_public)
    up = zkp.DeviceProvingKey.upload(ctx, crs.pk)
    vk = zkp.VerificationKey(num_public, True)
    dpk = zkp.CRS.from_prepared_device(ctx, qap, prep, num_public, vk=vk)
    try:
        assert dpk.sound and up.sound
        assert dpk.device_bytes() == up.device_bytes()
        assert dpk.test_info() == up.test_info() and dpk.test_plan() == up.test_plan()
        w = zkp.Witness(z, num_public)
        want = zkp.Prover.prove(up, w, r=r, s=s)
        got = zkp.Prover.prove(dpk, w, r=r, s=s)
        assert got.serialize_compressed() == want.serialize_compressed()
        dz = _device_z(w.assignment)
        got_dev = zkp.Prover.prove_device(dpk, dz.data_ptr(), len(w.assignment), num_public, r, s)
        assert got_dev.serialize_compressed() == want.serialize_compressed()
    finally:
        dpk.free()
        up.free()
    assert np.array_equal(vk.ic_g1, crs.vk.ic_g1)
    for nm in srs_util.VK_POINTS:
        assert np.array_equal(vk.point(nm), crs.vk.point(nm)), nm
    x = z[1:1 + num_public]
    assert zkp.Verifier.verify(vk, got, x) is True
    assert zkp.Verifier.verify(vk, got, [(x[0] + 1) % R] + x[1:]) is False


def test_device_key(zkp, ctx, pyref, handmade, srs9, prep9):
    qap, z = handmade
    _device_key_agrees(zkp, ctx, pyref, qap, z, srs9, prep9, 1)


def test_device_key_two_copies(zkp, ctx, pyref, handmade, srs9, prep9):
    qap, z = handmade
    try:
        ctx.set_option(zkp.ZK_OPT_SOUND_COPIES, 2)
        _device_key_agrees(zkp, ctx, pyref, qap, z, srs9, prep9, 3)
    finally:
        ctx.set_option(zkp.ZK_OPT_SOUND_COPIES, 0)


# -------------------------------------------------------------- downstream ---
def test_contribution_on_a_prepared_key(zkp, ctx, pyref, handmade, srs9, prep9):
    crs = zkp.CRS.from_prepared(ctx, handmade[0], prep9, 1)
    assert crs.verify_against_srs(ctx, srs9) == (True, zkp.ZK_KEYSRS_OK)
    after = crs.contribute(ctx, pyref.SplitMix64(0xC0).fr())
    assert zkp.CRS.verify_contribution(ctx, crs, after) == (True, zkp.ZK_CONTRIB_OK)
    assert after.verify_against_srs(ctx, srs9) == (True, zkp.ZK_KEYSRS_OK)
