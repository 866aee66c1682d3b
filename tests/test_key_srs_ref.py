"""The mathematics of CRS.verify_against_srs without a GPU (key_srs_ref.py):
the split row products and inverse transforms give the coefficients of
sum_i rho^part_i M_i(x), and with them the call's identities hold in the
exponent for known tau, alpha, beta, delta -- and stop holding when the key,
the circuit or a coefficient is changed."""
import pytest

import key_srs_ref as K
import pyref as P

R = K.R


def _secrets(seed):
    rng = P.SplitMix64(seed)
    return {nm: rng.fr() for nm in ("tau", "alpha", "beta", "delta")}


def _circuits():
    mats4, V4 = K.synthetic_rows(4)
    mats5, V5 = K.handmade5()
    return [("synthetic4", mats4, V4, (0, 1, V4 - 1)), ("handmade5", mats5, V5, (0, 1, V5 - 1))]


CASES = [(nm, mats, V, l) for nm, mats, V, ls in _circuits() for l in ls]


@pytest.mark.parametrize("name,mats,V,l", CASES, ids=[f"{c[0]}-l{c[3]}" for c in CASES])
def test_identities(name, mats, V, l):
    n = K.domain_size(len(mats[0]))
    co = K.coefficients(V + n)
    rho, sigma = co[:V], co[V:]
    ids = K.identities(mats, V, l, rho, sigma, **_secrets(0x1D))
    assert set(ids) == {"QUERY_A", "QUERY_B", "IC_VK", "IC_PK", "H"}
    for nm, (key, string) in ids.items():
        assert key == string, nm
    if l == V - 1:      # no private variable: both sides of IC_PK are the empty sum
        assert ids["IC_PK"] == (0, 0)


def test_shapes():
    mats, V = K.handmade5()
    assert K.domain_size(5) == 8 and K.domain_size(1) == 1 and K.domain_size(300) == 512
    m = K.coeff_vectors(mats, V, 1, K.coefficients(V))
    assert len(m) == 6 and all(len(v) == 8 for v in m)


def test_coefficients_are_the_column_polynomials():
    """m^{M,pub} + m^{M,priv} = sum_i rho_i M_i(x) coefficient by coefficient,
    M_i interpolated column by column; the split puts column i on its side"""
    mats, V = K.handmade5()
    n, l = 8, 2
    rho = K.coefficients(V, seed=0x77)
    m = K.coeff_vectors(mats, V, l, rho)
    for k, rows in enumerate(mats):
        cols = [[0] * n for _ in range(V)]
        for j, row in enumerate(rows):
            for c, v in row:
                cols[c][j] = (cols[c][j] + v) % R
        polys = [K.intt_naive(col) for col in cols]
        for part, keep in ((0, range(l + 1)), (1, range(l + 1, V))):
            want = [sum(rho[i] * polys[i][d] for i in keep) % R for d in range(n)]
            assert m[2 * k + part] == want, (k, part)
    # the cancelling pair leaves no trace of variable 4, and variable 5 is nowhere
    for unused in (4, 5):
        bumped = list(rho)
        bumped[unused] = (rho[unused] + 12345) % R
        assert K.coeff_vectors(mats, V, l, bumped) == m
    # the pair that adds (C row 3, column 1) counts twice
    rows = [list(r) for r in mats[2]]
    rows[3] = [(1, 2)]
    assert K.coeff_vectors([mats[0], mats[1], rows], V, l, rho) == m


def test_padded_rows_and_values():
    """rows >= nc are zero; the product vectors are what the transform inverts"""
    mats, V = K.handmade5()
    rho = K.coefficients(V)
    u = K.split_products(mats, V, 0, rho, 8)
    assert all(v[5:] == [0, 0, 0] for v in u)
    assert u[0][0] == rho[0] % R and u[1][0] == 2 * rho[1] % R          # A row 0: (0, 1) | (1, 2)
    assert u[1][3] == 3 * rho[1] % R                                     # the pair on column 4 cancels
    w = P.root_of_unity(8)
    for vec, m in zip(u, K.coeff_vectors(mats, V, 0, rho)):
        assert [P.poly_eval(m, pow(w, j, R)) for j in range(8)] == vec


@pytest.mark.parametrize("n", [1, 2, 8, 64])
def test_fast_transform_is_the_naive_one(n):
    rng = P.SplitMix64(0xF7 + n)
    u = [rng.fr() for _ in range(n)]
    assert K.intt_fast(u) == K.intt_naive(u)
    assert K.intt_naive(P.dft(u, n)) == u


def test_wrong_keys_break_the_identities():
    mats, V = K.handmade5()
    co = K.coefficients(V + 8)
    rho, sigma = co[:V], co[V:]
    sec = _secrets(0x2E)
    good = K.identities(mats, V, 1, rho, sigma, **sec)
    assert all(a == b for a, b in good.values())
    # the key of another circuit (one coefficient of A changed) against this one's coefficients
    other = [[list(r) for r in m] for m in mats]
    other[0][2] = [(3, 9)]
    key_side = K.identities(other, V, 1, rho, sigma, **sec)
    assert key_side["QUERY_A"][0] != good["QUERY_A"][1]
    assert key_side["IC_PK"][0] != good["IC_PK"][1]          # column 3 is private at l = 1
    assert key_side["QUERY_B"] == good["QUERY_B"] and key_side["IC_VK"][0] == good["IC_VK"][1]
    # another tau on the string's side
    sec2 = dict(sec, tau=(sec["tau"] + 1) % R)
    moved = K.identities(mats, V, 1, rho, sigma, **sec2)
    for nm in good:
        assert moved[nm][1] != good[nm][0], nm


def test_h_scalars():
    sigma = K.coefficients(4)
    d = K.h_scalars(sigma)
    assert len(d) == 8 and all(0 <= x < R for x in d)
    assert d[:4] == [R - s for s in sigma] and d[4:] == sigma


def test_explicit_coefficients():
    co = K.coefficients(600)
    assert len(set(co)) == 600 and co[0] == 1 and co[1] == (1 << 128) - 1
    assert all(0 < c < (1 << 128) for c in co)


# ------------------------------------------- the entry points, without a GPU ---
def test_symbols_and_statuses(zkp):
    import ctypes
    import os
    import re
    lib = ctypes.CDLL(zkp.LIB_PATH)
    assert hasattr(lib, "zk_groth16_verify_key_srs_sound") and "zk_groth16_verify_key_srs_sound" in zkp.EXPORTS
    assert not hasattr(lib, "zk_test_key_srs_coeffs")             # the coefficient hook is the test library's
    assert hasattr(zkp.test_lib(), "zk_test_key_srs_coeffs") and "zk_test_key_srs_coeffs" in zkp.TEST_EXPORTS
    hdr = open(os.path.join(os.path.dirname(zkp.CSRC), "..", "include", "zkp.h")).read()
    names = re.search(r"typedef enum \{([^}]*)\} zk_key_srs_status;", hdr).group(1)
    names = [s.split("=")[0].strip() for s in names.split(",")]
    assert names == ["ZK_KEYSRS_" + s for s in ("OK", "SHAPE", "POINT", "FIXED", "DELTA", "QUERY_A", "QUERY_B1",
                                                "QUERY_B2", "IC_VK", "IC_PK", "H")]
    assert [getattr(zkp, nm) for nm in names] == list(range(11))


def test_null_arguments_are_refused(zkp):
    import ctypes
    L = zkp.lib()
    csr, srs, pk, vk = zkp._CSR(), zkp._SRS(), zkp._PK(), zkp._VK()
    st = ctypes.c_int(-1)
    rc = L.zk_groth16_verify_key_srs_sound(None, ctypes.byref(csr), ctypes.byref(srs), ctypes.byref(pk),
                                           ctypes.byref(vk), None, ctypes.c_size_t(0), ctypes.byref(st))
    assert rc == zkp.ZK_ERR_ARG and st.value == -1
    fr = zkp._fr(5)
    assert zkp.test_lib().zk_test_key_srs_coeffs(None, ctypes.byref(csr), ctypes.c_uint64(0), ctypes.byref(fr),
                                                 ctypes.byref(fr)) == zkp.ZK_ERR_ARG
