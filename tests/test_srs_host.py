"""CPU checks of the string-based setup (csrc/srs.hip): the algebra it rests on,
over Fr with pyref alone; the ctypes layout of zk_srs; the Python argument
checks that need no GPU."""
import ctypes

import pytest

import sound_ref

R = sound_ref.R


def _lagrange(pyref, n, i, tau):
    """L_i(tau) over the size-n domain by the product formula"""
    w = pyref.root_of_unity(n)
    num, den = 1, 1
    wi = pow(w, i, R)
    for j in range(n):
        if j != i:
            wj = pow(w, j, R)
            num = num * (tau - wj) % R
            den = den * (wi - wj) % R
    return num * pyref.fr_inv(den) % R


@pytest.mark.parametrize("n", [4, 8])
def test_lagrange_is_an_inverse_transform_of_the_powers(pyref, n):
    """(1/n) sum_k w^(-ik) tau^k = L_i(tau): what the inverse group transform of
    [tau^k] computes in the exponent"""
    tau = pyref.SplitMix64(0x7A0 + n).fr()
    got = pyref.dft([pow(tau, k, R) for k in range(n)], n, inverse=True)
    assert got == [_lagrange(pyref, n, i, tau) for i in range(n)]


@pytest.mark.parametrize("n", [4, 8])
def test_column_sums_are_the_qap_polynomials(pyref, n):
    """sum_i M[i][j] L_i(tau) = M_j(tau) for the three matrices (n - 1
    constraints: one padded row)"""
    cs = pyref.synthetic_r1cs(n - 1)
    qap = pyref.QAP(cs)
    assert qap.n == n
    tau = pyref.SplitMix64(0xC01 + n).fr()
    L = [_lagrange(pyref, n, i, tau) for i in range(n)]
    for m in range(3):
        for j in range(qap.num_variables):
            s = sum(abc[m].get(j, 0) * L[i] for i, abc in enumerate(cs.constraints)) % R
            assert s == pyref.poly_eval(qap.polys[m][j], tau), (m, j)


def test_h_query_is_a_difference_of_powers(pyref):
    n = 8
    tau = pyref.SplitMix64(0x4D1F).fr()
    z = (pow(tau, n, R) - 1) % R
    for i in range(n):
        assert (pow(tau, i + n, R) - pow(tau, i, R)) % R == pow(tau, i, R) * z % R
    w = pyref.root_of_unity(n)
    assert pow(w, n, R) == 1          # tau on the domain: tau_g1[n] == tau_g1[0]


def test_srs_struct_layout(zkp):
    S = zkp._SRS
    assert S.log_n.offset == 0
    names = ("tau_g1", "tau_g1_len", "tau_g2", "tau_g2_len", "alpha_tau_g1", "alpha_len", "beta_tau_g1", "beta_len")
    assert [getattr(S, nm).offset for nm in names] == [8 * (k + 1) for k in range(8)]
    assert S.beta_g2.offset == 72 and ctypes.sizeof(S) == 272
    assert (zkp.ZK_SRS_OK, zkp.ZK_SRS_SHAPE, zkp.ZK_SRS_BETA) == (0, 1, 7)


def test_python_argument_checks(zkp):
    srs = zkp.SRS(2)
    assert srs.tau_g1.shape == (8, 13) and srs.tau_g2.shape == (4, 25)
    assert srs.alpha_tau_g1.shape == (4, 13) and srs.beta_tau_g1.shape == (4, 13)
    for bad in (0, 1 << 128, -1):
        with pytest.raises(ValueError):
            srs.verify(None, [1] * 3 + [bad] + [1] * 4)
    qap = zkp.QAP(zkp.CSRMatrices.synthetic(4))
    with pytest.raises(zkp.SetupError, match="sound"):
        zkp.CRS.from_srs(None, qap, srs, 1, sound=False)
    with pytest.raises(zkp.SetupError):
        zkp.CRS.from_srs(None, qap, srs, qap.num_variables)
    with pytest.raises(zkp.SetupError):
        zkp.SRS.generate(None, 2, 0, 1, 1)
    with pytest.raises(zkp.DomainTooSmall):
        zkp.SRS(32)
