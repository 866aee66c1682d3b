"""The XYZZ point formulas of csrc/curve.hpp one call at a time through
zk_test_curve, on raw Montgomery words against the affine group law of
oracle/pyref.py.  Inputs are built as XYZZ from affine points under chosen z
(X = x z^2, Y = y z^3, ZZ = z^2, ZZZ = z^3), which is how the branches an MSM
on random points all but never takes are reached: p == q and p == -q under
different scalings, infinity on either side, zero coordinates.  Every check
is exact: infinity <=> ZZ = 0, else X / ZZ and Y / ZZZ are the reference sum,
ZZ^3 = ZZZ^2, every word below p; and the variants of one formula must return
the same words."""
import ctypes as C
import random

import numpy as np
import pytest

import ff_model as fm
from ff_model import FQ, P

pytestmark = pytest.mark.gpu

RQ = fm.mont_r(FQ)
RQI = pow(RQ, -1, P)
LANE_SIZES = (1, 2, 3, 31, 32, 33, 63, 65, 127, 257)
COMMON_OPS = ("DBL", "DBL_CALL", "AFF_DBL", "MADD", "ADD", "ADD_ILP")
FIELDS = ("Fq", "Fq2", "Fq2h", "FqC", "Fq2C")
FORMULAS = [(f, op) for f in FIELDS for op in COMMON_OPS] + [("Fq", "ADD_QUAD"), ("Fq2h", "ADD_DUO")]


class Group:
    """One curve with the coordinate plumbing of its field (deg 1: Fq, 2: Fq2)."""

    def __init__(self, pyref, deg):
        self.deg, self.curve = deg, pyref.G1 if deg == 1 else pyref.G2
        self.el = (lambda *c: pyref.Fq1(c[0])) if deg == 1 else (lambda *c: pyref.Fq2(*c))
        self.coeffs = (lambda e: [e.v]) if deg == 1 else (lambda e: [e.c0, e.c1])
        self.zero, self.one = self.el(0, 0), self.el(1, 0)
        # 1 G .. 12 G, and on G1 the two curve points with x = 0 (order 3, outside the subgroup)
        self.multiples = [self.curve.mul(self.curve.gen, k) for k in range(1, 13)]
        self.points = list(self.multiples)
        if deg == 1:
            self.points += [(self.el(0), self.el(2)), (self.el(0), self.el(P - 2))]

    def rand(self, rng):
        return self.el(rng.randrange(1, P), rng.randrange(1, P))

    def zs(self, rng):
        """z = 1, p - 1, random, and over Fq2 a z with one zero coefficient."""
        z = [self.one, self.el(P - 1, 0), self.rand(rng), self.rand(rng)]
        if self.deg == 2:
            z += [self.el(0, rng.randrange(1, P)), self.el(rng.randrange(1, P), 0), self.el(0, 1), self.el(0, P - 1)]
        return z

    def xyzz(self, aff, z, rng=None):
        """The XYZZ form of an affine point under z; None: infinity (ZZ = 0), as the
        device sets it (0, 1, 0, 0) or, with rng, with arbitrary X, Y and ZZZ."""
        if aff is None:
            if rng is None:
                return (self.zero, self.one, self.zero, self.zero)
            return (self.rand(rng), self.rand(rng), self.zero, self.rand(rng))
        zz = z * z
        zzz = zz * z
        return (aff[0] * zz, aff[1] * zzz, zz, zzz)

    def encode(self, pts):
        """Tuples of field elements -> (n, 12 deg len) raw Montgomery words."""
        flat = [c * RQ % P for pt in pts for e in pt for c in self.coeffs(e)]
        return fm.to_words(flat, 12).reshape(len(pts), -1)

    def decode(self, arr):
        """(n, 48 deg) words -> XYZZ tuples of field elements; every word below p."""
        arr = np.asarray(arr)
        vals = fm.from_words(arr.reshape(-1, 12))
        assert all(v < P for v in vals), "a coordinate is not below p"
        d = self.deg
        els = [self.el(*[v * RQI % P for v in vals[i:i + d]]) for i in range(0, len(vals), d)]
        return [tuple(els[i:i + 4]) for i in range(0, len(els), 4)]

    def affine(self, pt):
        """XYZZ -> affine (None: infinity), asserting ZZ^3 = ZZZ^2."""
        X, Y, ZZ, ZZZ = pt
        if ZZ.is_zero():
            return None
        assert ZZ * ZZ * ZZ == ZZZ * ZZZ, "ZZ^3 != ZZZ^2"
        return (X * ZZ.inv(), Y * ZZZ.inv())


@pytest.fixture(scope="module")
def groups(pyref):
    g1, g2 = Group(pyref, 1), Group(pyref, 2)
    return {"Fq": g1, "FqC": g1, "Fq2": g2, "Fq2h": g2, "Fq2C": g2}


def same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a[0] == b[0] and a[1] == b[1])


def add_cases(g, rng):
    """(p, q, p + q) with p, q affine or None, and the z of each: every pair type."""
    cv, pts, zs = g.curve, g.points, g.zs(rng)
    out = []

    def put(A, B, za=None, zb=None, loose=False):
        za, zb = za or rng.choice(zs), zb or rng.choice(zs)
        out.append((g.xyzz(A, za, rng if loose else None), g.xyzz(B, zb, rng if loose else None), cv.add(A, B)))
    for i, A in enumerate(pts):
        for B in pts[i + 1:i + 4]:
            if not same(A, B) and not same(A, cv.neg(B)):
                put(A, B)
                put(B, A)
    for A in pts:
        for za in zs:
            zb = rng.choice([z for z in zs if not (z == za)])
            put(A, A, za, zb)                   # the same point under two z: the doubling branch
            put(A, cv.neg(A), za, zb)           # p and -q: infinity
        put(A, A, g.one, g.one)
        put(A, None), put(None, A), put(A, None, loose=True), put(None, A, loose=True)
    put(None, None), put(None, None, loose=True)
    return out


def madd_cases(g, rng):
    """(p XYZZ, a affine, p + a): generic, p infinity, p == a and p == -a under every z."""
    cv, pts, zs = g.curve, g.points, g.zs(rng)
    out = []
    for i, A in enumerate(pts):
        for B in pts[i + 1:i + 4]:
            if not same(A, B) and not same(A, cv.neg(B)):
                out.append((g.xyzz(A, rng.choice(zs)), B, cv.add(A, B)))
                out.append((g.xyzz(B, rng.choice(zs)), A, cv.add(A, B)))
    for A in pts:
        out += [(g.xyzz(None, None), A, A), (g.xyzz(None, None, rng), A, A)]
        for z in zs:
            out += [(g.xyzz(A, z), A, cv.add(A, A)), (g.xyzz(cv.neg(A), z), A, None)]
    return out


def dbl_cases(g, rng):
    cv, zs = g.curve, g.zs(rng)
    out = [(g.xyzz(A, z), cv.add(A, A)) for A in g.points for z in zs]
    return out + [(g.xyzz(None, None), None), (g.xyzz(None, None, rng), None)]


def cop(zkp, name):
    return getattr(zkp, "ZK_TEST_COP_" + name)


def fid(zkp, name):
    return getattr(zkp, "ZK_TEST_FIELD_" + name.upper())


def interleave(cases, rng):
    """Neighbouring elements always differ in kind: shuffle, so that edge cases sit between generic ones."""
    cases = list(cases)
    rng.shuffle(cases)
    return cases


def run(zkp, ctx, g, field, op, cases):
    """cases: (p, q, want) for the adds and MADD, (p, want) for the doublings,
    (a, want) for AFF_DBL -> the raw output words."""
    p = q = None
    if op in ("DBL", "DBL_CALL"):
        p = g.encode([c[0] for c in cases])
    elif op == "AFF_DBL":
        q = g.encode([c[0] for c in cases])
    else:
        p, q = g.encode([c[0] for c in cases]), g.encode([c[1] for c in cases])
    return ctx.test_curve(fid(zkp, field), cop(zkp, op), p, q)


def check(g, raw, cases, what):
    """Every lane's copy of every result is the reference group element."""
    raw = np.asarray(raw)
    n = len(cases)
    copies = raw.reshape(n, -1, 48 * g.deg)
    for k in range(1, copies.shape[1]):
        assert np.array_equal(copies[:, k], copies[:, 0]), "%s: lanes of one element disagree" % what
    got = g.decode(copies[:, 0])
    for i, (pt, case) in enumerate(zip(got, cases)):
        assert same(g.affine(pt), case[-1]), "%s: case %d of %d is not the reference point" % (what, i, n)


def cases_for(g, op, rng):
    if op in ("DBL", "DBL_CALL"):
        return dbl_cases(g, rng)
    if op == "AFF_DBL":
        return [(A, g.curve.add(A, A)) for A in g.points]
    if op == "MADD":
        return madd_cases(g, rng)
    return add_cases(g, rng)


@pytest.mark.parametrize("field,op", FORMULAS, ids=["%s-%s" % fo for fo in FORMULAS])
def test_formula(zkp, ctx, groups, field, op):
    g = groups[field]
    rng = random.Random(0xC0 + g.deg * 16 + len(op))
    cases = interleave(cases_for(g, op, rng), rng)
    assert len(cases) <= 2000
    check(g, run(zkp, ctx, g, field, op, cases), cases, "%s %s" % (field, op))


def test_order_three_points(zkp, ctx, groups):
    """(0, 2) and (0, -2) lie on y^2 = x^3 + 4 with x = 0: (0, 2) + (0, 2) = (0, -2), (0, 2) + (0, -2) = infinity."""
    g = groups["Fq"]
    T, U = (g.el(0), g.el(2)), (g.el(0), g.el(P - 2))
    assert g.curve.on_curve(T) and same(g.curve.add(T, T), U) and g.curve.add(T, U) is None
    rng = random.Random(3)
    z = g.rand(rng)
    for op in ("ADD", "ADD_ILP", "ADD_QUAD"):
        cases = [(g.xyzz(T, g.one), g.xyzz(T, z), U), (g.xyzz(T, z), g.xyzz(U, g.one), None),
                 (g.xyzz(U, z), g.xyzz(U, z), T)]
        check(g, run(zkp, ctx, g, "Fq", op, cases), cases, "order 3 " + op)
    cases = [(g.xyzz(T, z), T, U), (g.xyzz(T, z), U, None)]
    check(g, run(zkp, ctx, g, "Fq", "MADD", cases), cases, "order 3 MADD")
    cases = [(g.xyzz(T, z), U), (g.xyzz(U, g.one), T)]
    check(g, run(zkp, ctx, g, "Fq", "DBL", cases), cases, "order 3 DBL")


@pytest.mark.parametrize("deg", [1, 2], ids=["G1", "G2"])
def test_add_variants_return_identical_words(zkp, ctx, groups, deg):
    """All field results are canonical, so the same group operation on the same
    words gives the same words whichever add computes it (the byte-reproducible
    partial proofs rely on it)."""
    g = groups["Fq" if deg == 1 else "Fq2"]
    rng = random.Random(0x1DE + deg)
    cases = interleave(add_cases(g, rng), rng)
    if deg == 1:
        base = run(zkp, ctx, g, "Fq", "ADD", cases)
        others = {"ADD_ILP": run(zkp, ctx, g, "Fq", "ADD_ILP", cases), "FqC ADD": run(zkp, ctx, g, "FqC", "ADD", cases)}
        quad = run(zkp, ctx, g, "Fq", "ADD_QUAD", cases)
        others.update({"ADD_QUAD lane %d" % k: quad[:, k] for k in range(4)})
    else:
        base = run(zkp, ctx, g, "Fq2", "ADD", cases)
        others = {"Fq2 ADD_ILP": run(zkp, ctx, g, "Fq2", "ADD_ILP", cases),
                  "Fq2h ADD": run(zkp, ctx, g, "Fq2h", "ADD", cases),
                  "Fq2h ADD_ILP": run(zkp, ctx, g, "Fq2h", "ADD_ILP", cases),
                  "Fq2C ADD": run(zkp, ctx, g, "Fq2C", "ADD", cases)}
        duo = run(zkp, ctx, g, "Fq2h", "ADD_DUO", cases)
        others.update({"ADD_DUO unit %d" % k: duo[:, k] for k in range(2)})
    check(g, base, cases, "ADD")
    for name, out in others.items():
        bad = np.flatnonzero((out != base).any(axis=1))
        assert not len(bad), "%s differs from ADD in %d of %d cases, first %d" % (name, len(bad), len(cases), bad[0])


@pytest.mark.parametrize("field", FIELDS)
def test_doubling_variants_agree(zkp, ctx, groups, field):
    g = groups[field]
    rng = random.Random(0xDB1 + g.deg)
    cases = interleave(dbl_cases(g, rng), rng)
    a = run(zkp, ctx, g, field, "DBL", cases)
    b = run(zkp, ctx, g, field, "DBL_CALL", cases)
    assert np.array_equal(a, b), "DBL_CALL and DBL differ"
    # AFF_DBL(a) is DBL(from_aff(a)) as a group element (and here word for word)
    affs = [(A, g.curve.add(A, A)) for A in g.points]
    x = run(zkp, ctx, g, field, "AFF_DBL", affs)
    lifted = [(g.xyzz(A, g.one), w) for A, w in affs]
    y = run(zkp, ctx, g, field, "DBL", lifted)
    check(g, x, affs, "AFF_DBL")
    assert [g.affine(p) is None for p in g.decode(x)] == [g.affine(p) is None for p in g.decode(y)]
    assert all(same(g.affine(p), g.affine(q)) for p, q in zip(g.decode(x), g.decode(y)))
    assert np.array_equal(x, y)


@pytest.mark.parametrize("field", FIELDS)
def test_chains_of_formulas(zkp, ctx, groups, field):
    """Results fed to the next call: k B by k MADDs of B from infinity, and
    k B as the ADD of the doubles 2^j B picked by k's bits (infinity where a
    bit is clear), for several base points B side by side."""
    g = groups[field]
    cv = g.curve
    bases = g.points[:7]
    f = fid(zkp, field)
    acc = g.encode([g.xyzz(None, None)] * len(bases))
    aff = g.encode(bases)
    for k in range(1, 10):
        acc = ctx.test_curve(f, zkp.ZK_TEST_COP_MADD, acc, aff)
        want = [(cv.mul(B, k),) for B in bases]
        check(g, acc, want, "%s MADD chain step %d" % (field, k))
    ks = [0b10110, 0b1, 0b11111, 0b10000, 0b01010, 0b00111, 0b11001]
    dbl = g.encode([g.xyzz(B, g.one) for B in bases])
    inf = g.encode([g.xyzz(None, None)])[0]
    acc = g.encode([g.xyzz(None, None)] * len(bases))
    for j in range(5):
        q = np.array([dbl[i] if (k >> j) & 1 else inf for i, k in enumerate(ks)])
        acc = ctx.test_curve(f, zkp.ZK_TEST_COP_ADD, acc, q)
        dbl = ctx.test_curve(f, zkp.ZK_TEST_COP_DBL, dbl)
        check(g, dbl, [(cv.mul(B, 2 << j),) for B in bases], "%s DBL chain step %d" % (field, j))
    check(g, acc, [(cv.mul(B, k),) for B, k in zip(bases, ks)], "%s ADD of doubles" % field)


PLACED = [("Fq", "ADD_QUAD"), ("Fq2h", "ADD_DUO"), ("Fq2h", "ADD"), ("Fq2h", "ADD_ILP"), ("Fq2h", "MADD"),
          ("Fq2h", "DBL"), ("Fq2h", "DBL_CALL"), ("Fq2h", "AFF_DBL")]


@pytest.mark.parametrize("field,op", PLACED, ids=["%s-%s" % fo for fo in PLACED])
def test_lane_placement(zkp, ctx, groups, field, op):
    """The lane-cooperative forms with partly filled pairs of quads, rows and
    waves, neighbouring elements of different kinds (a doubling beside a
    cancellation beside a generic sum), and the same element at three
    positions: the results must not depend on where an element sits, and
    every lane of an element must hold the same result."""
    g = groups[field]
    rng = random.Random(0x9A + len(op))
    pool = interleave(cases_for(g, op, rng), rng)
    base = [pool[i % len(pool)] for i in range(max(LANE_SIZES))]   # shuffled kinds: neighbours always differ
    whole = run(zkp, ctx, g, field, op, base)
    check(g, whole, base, "%s %s n=%d" % (field, op, len(base)))
    whole = np.asarray(whole).reshape(len(base), -1)
    for n in LANE_SIZES:
        for rot in (0, 1, 2):
            idx = [(i + rot) % n for i in range(n)]
            out = np.asarray(run(zkp, ctx, g, field, op, [base[i] for i in idx])).reshape(n, -1)
            assert np.array_equal(out, whole[idx]), "%s %s: n=%d rotated by %d differs" % (field, op, n, rot)


def test_curve_hook_argument_errors(zkp, ctx, groups):
    g = groups["Fq"]
    T, h = zkp.test_lib(), C.c_void_p(ctx._h)
    p = g.encode([g.xyzz(g.points[0], g.one)] * 2)
    out = np.zeros((8, 48), dtype=np.uint32)
    pp, po = C.c_void_p(p.ctypes.data), C.c_void_p(out.ctypes.data)

    def call(ctxh, field, op, p_, q_, n, o_):
        return T.zk_test_curve(ctxh, C.c_int(field), C.c_int(op), p_, q_, C.c_size_t(n), o_)
    FQf, E = zkp.ZK_TEST_FIELD_FQ, zkp.ZK_ERR_ARG
    assert call(None, FQf, zkp.ZK_TEST_COP_DBL, pp, None, 2, po) == E
    assert call(h, FQf, zkp.ZK_TEST_COP_DBL, None, None, 2, po) == E
    assert call(h, FQf, zkp.ZK_TEST_COP_DBL, pp, None, 2, None) == E
    assert call(h, FQf, zkp.ZK_TEST_COP_ADD, pp, None, 2, po) == E
    assert call(h, FQf, zkp.ZK_TEST_COP_AFF_DBL, pp, None, 2, po) == E
    assert call(h, zkp.ZK_TEST_FIELD_FR, zkp.ZK_TEST_COP_DBL, pp, None, 2, po) == E
    assert call(h, 6, zkp.ZK_TEST_COP_DBL, pp, None, 2, po) == E
    assert call(h, FQf, 8, pp, pp, 2, po) == E
    assert call(h, FQf, -1, pp, pp, 2, po) == E
    assert call(h, FQf, zkp.ZK_TEST_COP_ADD_DUO, pp, pp, 1, po) == E
    for f in (zkp.ZK_TEST_FIELD_FQ2, zkp.ZK_TEST_FIELD_FQ2H, zkp.ZK_TEST_FIELD_FQC, zkp.ZK_TEST_FIELD_FQ2C):
        assert call(h, f, zkp.ZK_TEST_COP_ADD_QUAD, pp, pp, 1, po) == E
    assert call(h, zkp.ZK_TEST_FIELD_FQ2, zkp.ZK_TEST_COP_ADD_DUO, pp, pp, 1, po) == E
    assert not out.any()
    assert call(h, FQf, zkp.ZK_TEST_COP_ADD, None, None, 0, None) == zkp.ZK_OK     # n = 0: nothing to do
    assert call(h, FQf, zkp.ZK_TEST_COP_ADD_QUAD, pp, pp, 2, po) == zkp.ZK_OK
    want = g.curve.add(g.points[0], g.points[0])
    check(g, out.reshape(2, 4, 48), [(want,), (want,)], "ADD_QUAD through the C call")
