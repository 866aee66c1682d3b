"""ZKAMD-H2G2-V1, the hash to G2 of the proofs of knowledge (include/zkp.h),
restated over hashlib and pyref's Python integers -- the independent second
implementation the library's host and device code are checked against.  The
square root is points_util's norm method, not the complex method the library
uses.  About 0.08 s per hash: results are cached."""
import functools
import hashlib

import pyref as P

import points_util as U

X = 0xD201000000010000            # |x|; the curve's parameter x is -X
TAG = b"ZKAMD-H2G2-V1"
POK_DST = b"ZKAMD-POK-V1"
_x = -X
H2 = (_x**8 - 4 * _x**7 + 5 * _x**6 - 4 * _x**4 + 6 * _x**3 - 4 * _x**2 - 4 * _x + 13) // 9
H_EFF = 3 * (_x * _x - 1) * H2
B2 = P.Fq2(4, 4)


def fq2_pow(a, e):
    acc = P.Fq2(1, 0)
    while e:
        if e & 1:
            acc = acc * a
        a = a * a
        e >>= 1
    return acc


PSI_X = fq2_pow(P.Fq2(1, 1), (P.P - 1) // 3).inv()
PSI_Y = fq2_pow(P.Fq2(1, 1), (P.P - 1) // 2).inv()


def conj(a):
    return P.Fq2(a.c0, -a.c1)


def psi(pt):
    if pt is P.INF:
        return pt
    return (conj(pt[0]) * PSI_X, conj(pt[1]) * PSI_Y)


def clear_cofactor(pt):
    """[x^2 - x - 1] P + [x - 1] psi(P) + psi^2([2] P) with x = -X (Budroni-Pintore)"""
    G = P.G2
    a = G.mul(pt, X * X + X - 1)
    b = G.neg(G.mul(psi(pt), X + 1))
    c = psi(psi(G.add(pt, pt)))
    return G.add(G.add(a, b), c)


def field_element(m0, ctr):
    d = [hashlib.sha256(m0 + bytes([ctr, j])).digest() for j in range(5)]
    return (P.Fq2(int.from_bytes(d[0] + d[1], "big") % P.P, int.from_bytes(d[2] + d[3], "big") % P.P),
            d[4][31] & 1)


@functools.lru_cache(maxsize=None)
def h2g2(msg, dst):
    """-> (Q, tries): a pyref G2 point and the counter that gave it"""
    assert len(dst) <= 255
    m0 = hashlib.sha256(TAG + bytes([len(dst)]) + dst + msg).digest()
    for ctr in range(256):
        x, sign = field_element(m0, ctr)
        t = x * x * x + B2
        if t.is_zero():
            continue
        y = U.fq2_sqrt(t)
        if y is None:
            continue
        if int(U.fq2_largest(y)) != sign:
            y = -y
        q = clear_cofactor((x, y))
        if q is not P.INF:
            return q, ctr
    raise ValueError("no point after 256 tries")


def message_set(n=64):
    """be32(i) | 60 zero bytes, i < n: with dst b"test" the try counts of the 64
    are 0:28, 1:22, 2:6, 3:4, 4:2, 5:1, 8:1"""
    return [i.to_bytes(4, "big") + bytes(60) for i in range(n)]


def pok_message(challenge, s_g1, role):
    return bytes(challenge) + P.g1_compress(s_g1) + bytes([role])
