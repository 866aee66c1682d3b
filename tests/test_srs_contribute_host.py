"""Phase-1 contributions, the parts that need no GPU: the digit algebra behind
csrc/mulvec.hpp's walks over plain integers, the contribution in the exponent
with pyref, the ctypes layout of zk_srs_share, the declarations and exports,
and the Python argument checks."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = 0xD201000000010000
NEW = ("zk_g1_mul_scalars", "zk_g2_mul_scalars", "zk_srs_contribute", "zk_srs_verify_contribution")
NEW_TEST = ("zk_test_g1_mul_scalars_plain", "zk_test_g2_mul_scalars_plain", "zk_test_g1_mul_scalars_table",
            "zk_test_g2_mul_scalars_table", "zk_test_split_scalars")


def _digits(k):
    d = []
    for _ in range(4):
        k, rem = divmod(k, X)
        d.append(rem)
    assert k == 0
    return d


def test_digit_algebra(pyref):
    R = pyref.R
    assert R == X**4 - X**2 + 1 and R < X**4 and X < 1 << 64 and X * X < 1 << 128
    rng = pyref.SplitMix64(0xD161)
    for k in [0, 1, X - 1, X, X**2, X**3, R - 2, R - 1] + [rng.fr() for _ in range(32)]:
        d = _digits(k)
        assert all(0 <= w < X for w in d)
        assert sum(w * X**j for j, w in enumerate(d)) == k
        # the G1 halves are the digits joined in pairs, and the walk's identity
        e2, e1 = divmod(k, X * X)
        assert (e1, e2) == (d[0] + d[1] * X, d[2] + d[3] * X) and e1 < 1 << 128 and e2 < 1 << 128
    assert _digits(R - 1) == [0, 0, X - 1, X - 1]
    assert 1 + X + X**2 + X**3 < R
    # the 15 non-empty subset sums of {1, x, x^2, x^3}: distinct, non-zero mod r,
    # no two negatives of each other (so no table entry is the identity and
    # building a table never doubles)
    sums = [sum(X**j for j in range(4) if m >> j & 1) % R for m in range(1, 16)]
    assert len(set(sums)) == 15 and 0 not in sums
    assert all((u + v) % R for u, v in itertools.product(sums, sums))
    # G1: {1, x^2, 1 + x^2}
    s1 = [1, X * X % R, (1 + X * X) % R]
    assert len(set(s1)) == 3 and all((u + v) % R for u, v in itertools.product(s1, s1))


def test_g1_endomorphism_identity(pyref):
    """[x^2] (x, y) = (beta x, -y) for a primitive cube root of unity beta, the
    identity the G1 decomposition rests on (the G2 one, psi(P) = [-x] P, is
    asserted where its constants are made, csrc/gen_constants.py)"""
    P1 = pyref.G1.mul(pyref.G1.gen, 0xC0FFEE)
    b = pow(2, (pyref.P - 1) // 3, pyref.P)
    assert b != 1 and pow(b, 3, pyref.P) == 1
    cands = [(P1[0] * pyref.Fq1(beta), -P1[1]) for beta in (b, b * b % pyref.P)]
    assert pyref.G1.mul(P1, X * X) in cands


def test_contributing_twice_is_contributing_the_products(pyref):
    """in the exponent: entry i of each array after (s1, a1, b1) then
    (s2, a2, b2) is the entry after (s1 s2, a1 a2, b1 b2)"""
    R = pyref.R
    rng = pyref.SplitMix64(0x7A1C)
    tau, alpha, beta, s1, a1, b1, s2, a2, b2 = (rng.fr() for _ in range(9))
    N = 4

    def contribute(e, s, a, b):
        return {"tau": [pow(s, i, R) * v % R for i, v in enumerate(e["tau"])],
                "alpha": [a * pow(s, i, R) * v % R for i, v in enumerate(e["alpha"])],
                "beta": [b * pow(s, i, R) * v % R for i, v in enumerate(e["beta"])],
                "beta2": b * e["beta2"] % R}

    def string(t, a, b):
        return {"tau": [pow(t, i, R) for i in range(2 * N)], "alpha": [a * pow(t, i, R) % R for i in range(N)],
                "beta": [b * pow(t, i, R) % R for i in range(N)], "beta2": b}

    e0 = string(tau, alpha, beta)
    twice = contribute(contribute(e0, s1, a1, b1), s2, a2, b2)
    assert twice == contribute(e0, s1 * s2 % R, a1 * a2 % R, b1 * b2 % R)
    assert twice == string(tau * s1 * s2 % R, alpha * a1 * a2 % R, beta * b1 * b2 % R)
    # and on the curve, one entry
    p = pyref.G1.mul(pyref.G1.gen, e0["alpha"][3])
    assert pyref.G1.mul(pyref.G1.mul(p, a1 * pow(s1, 3, R) % R), a2 * pow(s2, 3, R) % R) == \
        pyref.G1.mul(pyref.G1.gen, twice["alpha"][3])


def test_share_layout(zkp):
    """zk_srs_share is three zk_g2_affine (25 words each) back to back"""
    assert ctypes.sizeof(zkp._SRSShare) == 3 * ctypes.sizeof(zkp._G2) == 3 * 25 * 8
    assert [(n, getattr(zkp._SRSShare, n).offset) for n, _ in zkp._SRSShare._fields_] == \
        [("tau_g2", 0), ("alpha_g2", 200), ("beta_g2", 400)]
    with open(os.path.join(ROOT, "include", "zkp.h")) as f:
        src = f.read()
    assert re.search(r"typedef struct \{ zk_g2_affine tau_g2, alpha_g2, beta_g2; \} zk_srs_share;", src)
    assert (zkp.ZK_SRSC_OK, zkp.ZK_SRSC_SHAPE, zkp.ZK_SRSC_SHARE, zkp.ZK_SRSC_STRING, zkp.ZK_SRSC_TAU,
            zkp.ZK_SRSC_ALPHA, zkp.ZK_SRSC_BETA) == tuple(range(7))
    m = re.search(r"typedef enum \{([^}]*)\} zk_srs_contribution_status;", src)
    names = [t.split("=")[0].strip() for t in m.group(1).split(",")]
    assert names == ["ZK_SRSC_OK", "ZK_SRSC_SHAPE", "ZK_SRSC_SHARE", "ZK_SRSC_STRING", "ZK_SRSC_TAU", "ZK_SRSC_ALPHA",
                     "ZK_SRSC_BETA"]


def test_declared_and_exported(zkp):
    for header, names, table in (("zkp.h", NEW, zkp.EXPORTS), ("zkp_test.h", NEW_TEST, zkp.TEST_EXPORTS)):
        with open(os.path.join(ROOT, "include", header)) as f:
            src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
        for n in names:
            assert re.search(r"\bint %s\s*\(" % n, src), n
            assert n in table, n
    for n in ("g1_mul_scalars", "g2_mul_scalars", "test_g1_mul_scalars_plain", "test_g2_mul_scalars_plain",
              "test_split_scalars"):
        assert callable(getattr(zkp.Context, n))
    assert callable(zkp.SRS.contribute) and callable(zkp.SRS.verify_contribution)


def test_python_argument_checks(zkp, pyref, monkeypatch):
    """ValueError before either library is loaded, on a context without a handle"""
    def touched():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(zkp, "lib", touched)
    monkeypatch.setattr(zkp, "test_lib", touched)
    nogpu = object.__new__(zkp.Context)
    R = pyref.R
    srs = zkp.SRS(2)
    for bad in ((0, 5, 7), (3, 0, 7), (3, 5, 0), (R, 5, 7), (3, R + 1, 7), (3, 5, -1)):
        with pytest.raises(ValueError):
            srs.contribute(nogpu, *bad)
    with pytest.raises(ValueError):
        zkp.SRS.verify_contribution(nogpu, srs, srs, np.zeros((3, 25), dtype=np.uint64), [1] * 7 + [-1])
    with pytest.raises(ValueError):
        nogpu.g1_mul_scalars(np.zeros((2, 13), dtype=np.uint64), [1])
    with pytest.raises(ValueError):
        nogpu.g2_mul_scalars(np.zeros((1, 25), dtype=np.uint64), [1 << 256])
    with pytest.raises(ValueError):
        nogpu.test_g1_mul_scalars_plain(np.zeros((1, 13), dtype=np.uint64), [-1])
    with pytest.raises(ValueError):
        nogpu.test_split_scalars([-1])
