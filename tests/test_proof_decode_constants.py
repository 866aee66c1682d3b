"""CPU checks of the proof decoder's subgroup tests (csrc/points.hpp,
pt_in_subgroup_endo): the constants gen_constants.py emits are beta =
2^((p-1)/3) and xi^(-(p-1)/3), xi^(-(p-1)/2) recomputed here with pyref, and
Scott's two criteria -- phi(P) = -[x^2]P on G1, psi(P) = [x]P on G2 -- accept
the subgroup points and reject the off-subgroup points of points_util, in
Python integers."""
import os
import re

import points_util as U
import pytest

X_ABS = 0xD201000000010000          # x = -X_ABS
RQ_DEV = 392                        # device Montgomery: R = 2^392 (gen_constants.py)


def _emitted(zkp, name, rows):
    """the words of constants.hpp's `name` as canonical integers, one per row of 12"""
    with open(os.path.join(zkp.CSRC, "constants.hpp")) as f:
        m = re.search(r"\b%s(?:\[\d+\])+ = \{(.*?)\};" % name, f.read())
    words = [int(w, 16) for w in re.findall(r"0x[0-9a-f]{8}", m.group(1))]
    assert len(words) == 12 * rows
    rinv = pow(1 << RQ_DEV, -1, U.PMOD)
    return [sum(w << (32 * i) for i, w in enumerate(words[12 * r:12 * r + 12])) * rinv % U.PMOD for r in range(rows)]


@pytest.fixture(scope="module")
def consts(pyref):
    p = pyref.P
    beta = pow(2, (p - 1) // 3, p)
    xi = pyref.Fq2(1, 1)

    def f2pow(a, e):
        acc = pyref.Fq2(1, 0)
        while e:
            if e & 1:
                acc = acc * a
            a = a * a
            e >>= 1
        return acc

    return beta, f2pow(xi, (p - 1) // 3).inv(), f2pow(xi, (p - 1) // 2).inv()


def test_emitted_constants_are_the_recomputed_ones(zkp, consts):
    beta, psi_x, psi_y = consts
    assert _emitted(zkp, "ENDO_BETA32", 1) == [beta]
    assert _emitted(zkp, "ENDO_PSI_X32", 2) == [psi_x.c0, psi_x.c1]
    assert _emitted(zkp, "ENDO_PSI_Y32", 2) == [psi_y.c0, psi_y.c1]


def _g1_in(pyref, consts, pt, beta=None):
    beta = consts[0] if beta is None else beta
    q = pyref.G1.mul(pt, X_ABS * X_ABS)
    return q is not pyref.INF and (pt[0] * beta, pt[1]) == pyref.G1.neg(q)


def _conj(pyref, a):
    return pyref.Fq2(a.c0, -a.c1)


def _psi(pyref, consts, pt):
    return (_conj(pyref, pt[0]) * consts[1], _conj(pyref, pt[1]) * consts[2])


def _g2_in(pyref, consts, pt):
    q = pyref.G2.mul(pt, X_ABS)
    return q is not pyref.INF and _psi(pyref, consts, pt) == pyref.G2.neg(q)


def test_generator_identities(pyref, consts):
    beta = consts[0]
    assert beta != 1 and pow(beta, 3, pyref.P) == 1
    assert _g1_in(pyref, consts, pyref.G1.gen)
    assert not _g1_in(pyref, consts, pyref.G1.gen, beta * beta % pyref.P)   # the other cube root is the wrong one
    assert pyref.G2.on_curve(_psi(pyref, consts, pyref.G2.gen))
    assert _g2_in(pyref, consts, pyref.G2.gen)


def test_criteria_accept_the_subgroup(pyref, consts):
    for pt in U.g1_points(4):
        assert pyref.G1.mul(pt, pyref.R) is pyref.INF and _g1_in(pyref, consts, pt)
    for pt in U.g2_points(4):
        assert pyref.G2.mul(pt, pyref.R) is pyref.INF and _g2_in(pyref, consts, pt)


def test_criteria_reject_points_off_the_subgroup(pyref, consts):
    for pt in U.g1_off_subgroup():
        assert pyref.G1.on_curve(pt) and pyref.G1.mul(pt, pyref.R) is not pyref.INF
        assert not _g1_in(pyref, consts, pt)
    for pt in U.g2_off_subgroup():
        assert pyref.G2.on_curve(pt) and pyref.G2.mul(pt, pyref.R) is not pyref.INF
        assert not _g2_in(pyref, consts, pt)
