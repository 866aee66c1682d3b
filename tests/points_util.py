"""Point sets shared by test_points_host.py and test_gpu_points.py, built with
oracle/pyref.py (Python integers): subgroup points by repeated addition of the
generator, points on the curves but outside the prime-order subgroup, and the
invalid encodings of every status.  Everything is computed once per session."""
import functools

import numpy as np
import pyref as P

PMOD = P.P
HALF = (PMOD - 1) // 2
ST_OK, ST_ENCODING, ST_RANGE, ST_CURVE, ST_SUBGROUP = range(5)


# ---- square roots in Python (the norm method in Fq2: not the device's) ----
def fq_sqrt(a):
    a %= PMOD
    r = pow(a, (PMOD + 1) // 4, PMOD)
    return r if r * r % PMOD == a else None


def fq2_sqrt(a):
    if a.c1 == 0:
        r = fq_sqrt(a.c0)
        if r is not None:
            return P.Fq2(r, 0)
        return P.Fq2(0, fq_sqrt(-a.c0))        # -1 is a non-residue: (r u)^2 = -r^2
    n = fq_sqrt(a.c0 * a.c0 + a.c1 * a.c1)
    if n is None:
        return None
    for s in (n, -n):
        x0 = fq_sqrt((a.c0 + s) * pow(2, PMOD - 2, PMOD))
        if x0:
            r = P.Fq2(x0, a.c1 * pow(2 * x0, PMOD - 2, PMOD))
            assert r * r == a
            return r
    return None


def fq2_largest(y):
    """The encodings' sort flag of an Fq2 value: c1, or c0 when c1 == 0."""
    return P._largest(y.c1) if y.c1 else P._largest(y.c0)


# ---- subgroup points: P_{i+1} = P_i + G from [k]G with a 16-bit k ----------
def _walk(curve, k, n):
    pts, p = [], curve.mul(curve.gen, k)
    for _ in range(n):
        pts.append(p)
        p = curve.add(p, curve.gen)
    return pts


@functools.lru_cache(maxsize=None)
def g1_points(n, k=0x9E37):
    return _walk(P.G1, k, n)


@functools.lru_cache(maxsize=None)
def g2_points(n, k=0xB7E1):
    return _walk(P.G2, k, n)


def on_curve_g1(x):
    """The point of E(Fq) at this x with the smaller y, or None."""
    y = fq_sqrt(x ** 3 + 4)
    return None if y is None else (P.Fq1(x), P.Fq1(min(y, PMOD - y)))


def on_curve_g2(c0, c1):
    x = P.Fq2(c0, c1)
    y = fq2_sqrt(x * x * x + P.Fq2(4, 4))
    return None if y is None else (x, y)


@functools.lru_cache(maxsize=None)
def g1_off_subgroup():
    """Points of E(Fq) outside G1: order 3, three of full order, a subgroup
    point moved by the order-3 point, and [r]Q, which lies in the cofactor's
    torsion."""
    t3 = (P.Fq1(0), P.Fq1(2))
    q = [on_curve_g1(x) for x in (4, 5, 6)]
    assert all(p is not None and P.G1.on_curve(p) for p in q) and P.G1.on_curve(t3)
    rq = P.G1.mul(q[0], P.R)
    assert rq is not P.INF
    return [t3] + q + [P.G1.add(g1_points(4)[3], t3), rq]


@functools.lru_cache(maxsize=None)
def g2_off_subgroup():
    q = [on_curve_g2(*x) for x in ((0, 1), (1, 1), (2, 0))]
    assert all(p is not None and P.G2.on_curve(p) for p in q)
    rq = P.G2.mul(q[0], P.R)
    assert rq is not P.INF
    return q + [rq, P.G2.add(g2_points(4)[3], rq)]


# ---- encodings --------------------------------------------------------------
def be48(v):
    return int(v).to_bytes(48, "big")


def flagged(data, flags):
    b = bytearray(data)
    b[0] |= flags
    return bytes(b)


def invalid_g1():
    """[(encoding, expected status)] for G1, every status but 0."""
    out = [(be48(P.G1_GEN[0]), ST_ENCODING),                      # compression flag clear
           (bytes([0xE0]) + bytes(47), ST_ENCODING),              # infinity with the sort flag
           (bytes([0xC0]) + bytes(46) + b"\x01", ST_ENCODING),    # infinity with a stray low byte
           (flagged(be48(PMOD), 0x80), ST_RANGE),
           (flagged(be48(2 ** 381 - 1), 0x80), ST_RANGE)]
    for x in (1, 2, 3, 7):
        assert on_curve_g1(x) is None
        out.append((flagged(be48(x), 0x80), ST_CURVE))
    for pt in g1_off_subgroup():
        out.append((P.g1_compress(pt), ST_SUBGROUP))
        out.append((P.g1_compress(P.G1.neg(pt)), ST_SUBGROUP))
    return out


def invalid_g2():
    gx = P.G2_GEN[0]
    out = [(be48(gx[1]) + be48(gx[0]), ST_ENCODING),
           (bytes([0xE0]) + bytes(95), ST_ENCODING),
           (bytes([0xC0]) + bytes(94) + b"\x01", ST_ENCODING),
           (flagged(be48(PMOD) + be48(5), 0x80), ST_RANGE),         # c1 >= p, c0 fine
           (flagged(be48(5) + be48(PMOD), 0x80), ST_RANGE),         # c0 >= p, c1 fine
           (flagged(be48(2 ** 381 - 1) + be48(5), 0x80), ST_RANGE)]
    for x in ((0, 0), (1, 0), (3, 0)):
        assert on_curve_g2(*x) is None
        out.append((flagged(be48(x[1]) + be48(x[0]), 0x80), ST_CURVE))
    for pt in g2_off_subgroup():
        out.append((P.g2_compress(pt), ST_SUBGROUP))
        out.append((P.g2_compress(P.G2.neg(pt)), ST_SUBGROUP))
    return out


G1_GEN_ENC = P.g1_compress(P.G1.gen)
G2_GEN_ENC = P.g2_compress(P.G2.gen)


def host_decode(zkp, enc):
    """The host decoder's verdict on one encoding (48 bytes: G1, 96: G2),
    reached through the proof codec: the affine words, or None when it
    refuses."""
    g1 = len(enc) == 48
    data = (enc + G2_GEN_ENC + G1_GEN_ENC) if g1 else (G1_GEN_ENC + enc + G1_GEN_ENC)
    try:
        proof = zkp.Proof.deserialize_compressed(data)
    except ValueError:
        return None
    return np.array(proof.a if g1 else proof.b, dtype=np.uint64)


def words_g1(pts):
    return np.array([P.g1_words(p) for p in pts], dtype=np.uint64).reshape(-1, 13)


def words_g2(pts):
    return np.array([P.g2_words(p) for p in pts], dtype=np.uint64).reshape(-1, 25)
