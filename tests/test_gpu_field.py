"""Device field arithmetic (csrc/ff.hpp) one operation at a time through
zk_test_field, on raw Montgomery words against plain Python integers: every
comparison is exact.  The inputs are the values random curve points never
supply -- 0, 1, m - 1, limb and word seams, operands at or above the modulus
where an operation allows them, a b - c d at its most negative -- and cases
constructed so that the rarely taken final subtraction of each Montgomery
product IS taken (tests/ff_model.py says which; the counts are asserted)."""
import itertools
import random
import zlib

import numpy as np
import pytest

import ff_model as fm
from ff_model import FQ, FR, P

pytestmark = pytest.mark.gpu

RQ = fm.mont_r(FQ)
RQI = pow(RQ, -1, P)
LANE_SIZES = (1, 2, 3, 31, 32, 33, 63, 65, 127, 257)


# ------------------------------------------------------------ input classes
def edge_values(prm, rng):
    """Canonical edge values: small, near m, the Montgomery constants, and the
    seams between the LB-bit multiply limbs and the 32-bit storage words."""
    m, LB = prm.m, prm.LB
    Rm = fm.mont_r(prm)
    v = [0, 1, 2, m - 1, m - 2, (m - 1) // 2, (m + 1) // 2, Rm % m, Rm * Rm % m,
         (1 << (m.bit_length() - 1)) - 1]                       # every limb all ones, cut below m
    for bit in sorted({LB * i for i in range(1, prm.NL)} | {32 * w for w in range(1, prm.N)}):
        v += [1 << bit, (1 << bit) - 1]
    v += [((1 << LB) - 1) << (LB * i) for i in range(prm.NL)]   # one limb all ones
    v += [0xFFFFFFFF << (32 * w) for w in range(prm.N)]         # one word all ones
    v = [x for x in v if x < m]
    return v + [rng.randrange(m) for _ in range(24)]


def wide_values(prm, rng):
    """Words at or above the modulus (MUL, SQR, MUL_LAZY, TO_MONT, FROM_MONT take them)."""
    m, top = prm.m, (1 << (32 * prm.N)) - 1
    return [m, m + 1, 2 * m - 1, top, top - 1, top - m] + [rng.getrandbits(32 * prm.N) for _ in range(24)]


def pairs_of(core, vals, rng):
    """Pairs of classes: the core edges against everything, both ways, and two shuffles."""
    s1, s2 = list(vals), list(vals)
    rng.shuffle(s1)
    rng.shuffle(s2)
    return list(itertools.product(core, vals)) + list(itertools.product(vals, core)) + list(zip(vals, s1)) + \
        list(zip(s2, vals))


def seed_of(*names):
    return zlib.crc32("-".join(names).encode())


def sqrt_mod(x, m):
    """A square root of x mod the prime m, or None (Tonelli-Shanks)."""
    x %= m
    if x == 0:
        return 0
    if pow(x, (m - 1) // 2, m) != 1:
        return None
    q, s = m - 1, 0
    while q % 2 == 0:
        q, s = q // 2, s + 1
    z = 2
    while pow(z, (m - 1) // 2, m) == 1:
        z += 1
    c, t, r = pow(z, q, m), pow(x, q, m), pow(x, (q + 1) // 2, m)
    while t != 1:
        i, u = 0, t
        while u != 1:
            u, i = u * u % m, i + 1
        b = pow(c, 1 << (s - i - 1), m)
        r, c, t, s = r * b % m, b * b % m, t * b * b % m, i
    return r


# ------------------------------------------------------------- references
def ref_prime(prm, op, a, b=0, c=0, d=0):
    m, Rm = prm.m, fm.mont_r(prm)
    ri = pow(Rm, -1, m)
    return {
        "MUL": lambda: a * b * ri % m, "MUL_LAZY": lambda: a * b * ri % m, "SQR": lambda: a * a * ri % m,
        "ADD": lambda: (a + b) % m, "SUB": lambda: (a - b) % m, "NEG": lambda: -a % m, "DBL": lambda: 2 * a % m,
        "INV": lambda: pow(a, m - 2, m) * Rm * Rm % m, "FQ_INV": lambda: pow(a, m - 2, m) * Rm * Rm % m,
        "TO_MONT": lambda: a * Rm % m, "FROM_MONT": lambda: a * ri % m,
        "MUL_SUB": lambda: (a * b - c * d) * ri % m,
    }[op]()


def f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def ref_fq2(op, a, b=(0, 0), c=(0, 0), d=(0, 0)):
    if op == "MUL":
        return tuple(x * RQI % P for x in f2mul(a, b))
    if op == "SQR":
        return tuple(x * RQI % P for x in f2mul(a, a))
    if op == "MUL_SUB":
        x, y = f2mul(a, b), f2mul(c, d)
        return ((x[0] - y[0]) * RQI % P, (x[1] - y[1]) * RQI % P)
    if op == "ADD":
        return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)
    if op == "SUB":
        return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)
    if op == "NEG":
        return (-a[0] % P, -a[1] % P)
    if op == "INV":    # (a / R)^-1 R; 0 -> 0
        n = pow(a[0] * a[0] + a[1] * a[1], P - 2, P) * RQ * RQ % P
        return (a[0] * n % P, -a[1] * n % P)
    if op == "IS_ZERO":
        return (1, 1) if a == (0, 0) else (0, 0)
    raise KeyError(op)


def fop(zkp, name):
    return getattr(zkp, "ZK_TEST_FOP_" + name)


def run_prime(zkp, ctx, prm, op, cols):
    field = zkp.ZK_TEST_FIELD_FQ if prm is FQ else zkp.ZK_TEST_FIELD_FR
    ops = [fm.to_words(list(col), prm.N) for col in cols]
    return fm.from_words(ctx.test_field(field, fop(zkp, op), *ops))


def run_fq2(zkp, ctx, field, op, cols):
    f = zkp.ZK_TEST_FIELD_FQ2 if field == "Fq2" else zkp.ZK_TEST_FIELD_FQ2H
    ops = [fm.to_words2(list(col)) for col in cols]
    return fm.from_words2(ctx.test_field(f, fop(zkp, op), *ops))


def check_equal(got, want, cases, what):
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, "%s: %d of %d differ, first at %d: in %s got %s want %s" % (
        what, len(bad), len(want), bad[0], [hexs(x) for x in cases[bad[0]]], hexs(got[bad[0]]), hexs(want[bad[0]]))


def hexs(x):
    return "(%s)" % ", ".join(hex(v) for v in x) if isinstance(x, tuple) else hex(x)


# ------------------------------------------------ Fr / Fq, one op at a time
UNARY = ("SQR", "NEG", "DBL", "INV", "FQ_INV", "TO_MONT", "FROM_MONT")
WIDE_OK = ("MUL", "SQR", "MUL_LAZY", "TO_MONT", "FROM_MONT")
SHARED_OPS = ("MUL", "SQR", "ADD", "SUB", "NEG", "DBL", "INV", "TO_MONT", "FROM_MONT")
PRIME_OPS = [(FR, op) for op in SHARED_OPS + ("MUL_LAZY",)] + [(FQ, op) for op in SHARED_OPS + ("FQ_INV",)]


@pytest.mark.parametrize("prm,op", PRIME_OPS, ids=["%s-%s" % (p.name, o) for p, o in PRIME_OPS])
def test_prime_field_op(zkp, ctx, prm, op):
    rng = random.Random(seed_of(prm.name, op))
    m = prm.m
    vals = edge_values(prm, rng)
    core = vals[:10]
    if op in WIDE_OK:
        wide = wide_values(prm, rng)
        vals, core = vals + wide, [0, 1, m - 1, fm.mont_r(prm) % m] + wide[:4]
    if op in UNARY:
        cases = [(a,) for a in vals]
    else:
        cases = pairs_of(core, vals, rng)
        if op == "ADD":     # a + b = m - 1, m, m + 1 (and the carry chain of m - 1 + 1)
            for a in vals[:40]:
                cases += [(a, (t - a) % m) for t in (m - 1, m, m + 1) if a and 0 <= t - a < m]
        if op == "SUB":     # a = b, a = 0, a < b by one (a full borrow chain when a = 0)
            for a in vals[:40]:
                cases += [(a, a), (0, a), (a, (a + 1) % m), ((a + 1) % m, a)]
    assert 60 <= len(cases) <= 2600
    got = run_prime(zkp, ctx, prm, op, zip(*cases))
    want = [ref_prime(prm, op, *c) for c in cases]
    if op != "MUL_LAZY":
        assert all(g < m for g in got), "a result is not below the modulus"
        check_equal(got, want, cases, "%s %s" % (prm.name, op))
        return
    assert all(g < 2 * m for g in got), "a lazy product is not below 2m"
    check_equal([g % m for g in got], want, cases, "Fr MUL_LAZY")
    # outputs in [m, 2m) go back in as operands, as the NTT feeds them back
    back = [g for g in got if g >= m]
    back += lazy_taken(rng, 48)[2]
    assert len(back) >= 48 and all(m <= g < 2 * m for g in back)
    cases2 = list(zip(back, reversed(back))) + [(g, g) for g in back] + \
        [(g, vals[i % len(vals)]) for i, g in enumerate(back)]
    got2 = run_prime(zkp, ctx, prm, op, zip(*cases2))
    assert all(g < 2 * m for g in got2)
    check_equal([g % m for g in got2], [ref_prime(prm, op, *c) for c in cases2], cases2, "Fr MUL_LAZY fed back")


def taken_mul(prm, rng, n):
    """(a, b) with a b / R = t small: the product's final subtraction is taken."""
    m, Rm = prm.m, fm.mont_r(prm)
    out = []
    for _ in range(n):
        a, t = rng.randrange(1, m), rng.getrandbits(200)
        out.append((a, t * Rm * pow(a, -1, m) % m))
    return out


def taken_sqr(prm, rng, n):
    m, Rm = prm.m, fm.mont_r(prm)
    out = []
    while len(out) < n:
        a = sqrt_mod(rng.getrandbits(200) * Rm, m)
        if a is not None:
            out.append((a,))
    return out


def lazy_taken(rng, n):
    """Fr operands whose lazy product stays in [r, 2r): (a's, b's, products)."""
    cases = taken_mul(FR, rng, n)
    vals = [fm.mul(FR, a, b).value for a, b in cases]
    return [a for a, _ in cases], [b for _, b in cases], vals


def split(flags):
    return sum(flags), len(flags) - sum(flags)


def need_both(flags, what):
    taken, kept = split(flags)
    assert taken >= 32 and kept >= 32, "%s: %d cases take the final subtraction, %d do not" % (what, taken, kept)


PRIME_SUBTRACT = [(FR, "MUL"), (FR, "SQR"), (FR, "MUL_LAZY"), (FQ, "MUL"), (FQ, "SQR")]


@pytest.mark.parametrize("prm,op", PRIME_SUBTRACT, ids=["%s-%s" % (p.name, o) for p, o in PRIME_SUBTRACT])
def test_final_subtraction_unsigned(zkp, ctx, prm, op):
    """Random operands take fp_reduce_once about once in 10^4 (Fq) or 4 in
    10^3 (Fr) products; these are built to take it, and the model says so."""
    rng = random.Random(0x5B7 + prm.N + len(op))
    m = prm.m
    if op == "SQR":
        cases = taken_sqr(prm, rng, 48) + [(rng.randrange(m),) for _ in range(48)]
        flags = [fm.takes_subtraction(prm, fm.mul(prm, a, a)) for a, in cases]
    else:
        cases = taken_mul(prm, rng, 48) + [(rng.randrange(m), rng.randrange(m)) for _ in range(48)]
        flags = [fm.takes_subtraction(prm, fm.mul(prm, a, b)) for a, b in cases]
    need_both(flags, "%s %s" % (prm.name, op))
    got = run_prime(zkp, ctx, prm, op, zip(*cases))
    want = [ref_prime(prm, op, *c) for c in cases]
    if op == "MUL_LAZY":   # the unreduced value is unique: (a b + (-a b / m mod R) m) / R
        Rm = fm.mont_r(prm)
        mi = pow(m, -1, Rm)
        check_equal(got, [(a * b + (-a * b * mi % Rm) * m) // Rm for a, b in cases], cases, "Fr MUL_LAZY value")
        got = [g % m for g in got]
    check_equal(got, want, cases, "%s %s" % (prm.name, op))


# -------------------------------------------------------- Fq MUL_SUB ------
def solve_mul_sub(rng, t):
    a, b, c = (rng.randrange(1, P) for _ in range(3))
    return (a, b, c, (a * b - t * RQ) * pow(c, -1, P) % P)


def small_t(rng):
    return rng.getrandbits(200)


def above_window(rng, k=5):
    """Just above k p^2 / R: the offset forms never take the subtraction there."""
    return k * P * P // RQ + 1 + rng.getrandbits(64)


def test_fq_mul_sub(zkp, ctx):
    rng = random.Random(0xAB5CD)
    vals = edge_values(FQ, rng)
    cases = [(0, 0, P - 1, P - 1), (0, 5, P - 1, P - 1), (P - 1, 0, P - 1, P - 1), (P - 1, P - 1, 0, 0),
             (P - 1, P - 1, P - 1, P - 1), (1, 1, P - 1, P - 1), (0, 0, 0, 0), (P - 1, 1, 1, P - 1)]
    for _ in range(40):     # a b = c d exactly: result 0
        a, b = rng.choice(vals), rng.choice(vals)
        cases += [(a, b, b, a), (a, b, a, b)]
        c = rng.randrange(1, P)
        cases.append((a, b, c, a * b * pow(c, -1, P) % P))
    cases += [tuple(rng.choice(vals) for _ in range(4)) for _ in range(600)]
    built = [solve_mul_sub(rng, small_t(rng)) for _ in range(40)] + \
            [solve_mul_sub(rng, 3 * P * P // RQ - 1 - rng.getrandbits(64)) for _ in range(8)] + \
            [solve_mul_sub(rng, above_window(rng)) for _ in range(40)]
    need_both([fm.takes_subtraction(FQ, fm.fq_mul_sub(*c)) for c in built], "fq_mul_sub")
    cases += built
    got = run_prime(zkp, ctx, FQ, "MUL_SUB", zip(*cases))
    assert all(g < P for g in got)
    check_equal(got, [ref_prime(FQ, "MUL_SUB", *c) for c in cases], cases, "Fq MUL_SUB")


# ------------------------------------------------------- Fq2 and Fq2h -----
def fq2_values(rng):
    """Fq2 elements: edge coefficients in both halves, one half zero, random."""
    core = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, RQ % P, (1 << 380) - 1, 1 << 364, (1 << 28) - 1]
    v = list(itertools.product(core, core))
    e = edge_values(FQ, rng)
    v += [(x, rng.randrange(P)) for x in e[11:60]] + [(rng.randrange(P), x) for x in e[60:]]
    v += [(0, rng.randrange(1, P)) for _ in range(6)] + [(rng.randrange(1, P), 0) for _ in range(6)]
    return v + [(rng.randrange(P), rng.randrange(P)) for _ in range(24)]


def fq2_mul_sub_cases(rng, vals):
    z, t = P - 1, (P - 1, P - 1)
    cases = [((0, 0), (0, 0), t, t), (t, t, (0, 0), (0, 0)), (t, t, t, t),
             # the subtracted coefficients at p - 1 and the added ones at 0, and the reverse:
             # lane 0 = a0 b0 - a1 b1 - c0 d0 + c1 d1, lane 1 = a1 b0 + a0 b1 - c1 d0 - c0 d1
             ((0, z), (0, z), (z, 0), (z, 0)), ((z, 0), (z, 0), (0, z), (0, z)),
             ((0, 0), (0, 0), (z, z), (z, z)), ((z, z), (z, z), (0, 0), (0, 0)),
             ((0, z), (z, 0), (z, z), (z, 0)), ((z, 0), (0, z), (z, 0), (z, z))]
    for _ in range(30):     # a b = c d: result 0
        a, b = rng.choice(vals), rng.choice(vals)
        cases += [(a, b, b, a), (a, b, a, b)]
    return cases + [tuple(rng.choice(vals) for _ in range(4)) for _ in range(500)]


FQ2_OPS = [("Fq2", op) for op in ("MUL", "SQR", "INV", "ADD", "SUB", "NEG", "MUL_SUB")] + \
          [("Fq2h", op) for op in ("MUL", "SQR", "MUL_SUB", "ADD", "SUB", "NEG", "IS_ZERO")]


def fq2_cases(op, rng):
    vals = fq2_values(rng)
    if op in ("SQR", "INV", "NEG", "IS_ZERO"):
        return [(a,) for a in vals]
    if op == "MUL_SUB":
        return fq2_mul_sub_cases(rng, vals)
    cases = pairs_of([(0, 0), (P - 1, P - 1), (0, P - 1)], vals, rng)
    if op == "ADD":
        cases += [(a, ((t - a[0]) % P, (u - a[1]) % P)) for a in vals[:60]
                  for t, u in ((P, P - 1), (P + 1, P), (P - 1, P + 1)) if a[0] > 1 and a[1] > 1]
    if op == "SUB":
        cases += [(a, a) for a in vals[:60]] + [((0, 0), a) for a in vals[:60]] + \
                 [(a, ((a[0] + 1) % P, (a[1] + 1) % P)) for a in vals[:60]]
    return cases


@pytest.mark.parametrize("field,op", FQ2_OPS, ids=["%s-%s" % fo for fo in FQ2_OPS])
def test_fq2_op(zkp, ctx, field, op):
    rng = random.Random(seed_of("fq2", op))     # the same cases for Fq2 and Fq2h
    cases = fq2_cases(op, rng)
    assert 100 <= len(cases) <= 2600
    got = run_fq2(zkp, ctx, field, op, zip(*cases))
    assert all(g[0] < P and g[1] < P for g in got)
    check_equal(got, [ref_fq2(op, *c) for c in cases], cases, "%s %s" % (field, op))


def built_fq2_mul(rng):
    """Fq2 products whose c0 (lane 0) or c1 (lane 1) result is tiny, or just
    above the window in which the offset forms may subtract."""
    out = []
    for k in range(160):
        a0, a1, b0 = (rng.randrange(1, P) for _ in range(3))
        t = small_t(rng) if k % 2 == 0 else above_window(rng, 6)
        if k % 4 < 2:
            b1 = (a0 * b0 - t * RQ) * pow(a1, -1, P) % P       # c0 = t
        else:
            b1 = (t * RQ - a1 * b0) * pow(a0, -1, P) % P       # c1 = t
        out.append(((a0, a1), (b0, b1)))
    return out


def built_fq2_sqr(rng):
    """Squares whose (a0 + a1)(a0 - a1) or 2 a0 a1 is tiny."""
    out = []
    half = pow(2, -1, P)
    for k in range(96):
        t = 2 * small_t(rng)
        if k % 2 == 0:
            u = rng.randrange(1, P)
            w = t * RQ * pow(u, -1, P) % P
            out.append((((u + w) * half % P, (u - w) * half % P),))
        else:
            a0 = rng.randrange(1, P)
            out.append(((a0, t * RQ * pow(2 * a0, -1, P) % P),))
    return out + [((rng.randrange(P), rng.randrange(P)),) for _ in range(48)]


def built_fq2_mul_sub(rng):
    out = []
    for k in range(160):
        a, b, c = ((rng.randrange(1, P), rng.randrange(1, P)) for _ in range(3))
        d0 = rng.randrange(P)
        t = small_t(rng) if k % 2 == 0 else above_window(rng, 6)
        if k % 4 < 2:   # lane 0: a0 b0 - a1 b1 - c0 d0 + c1 d1 = t R
            d1 = (t * RQ - a[0] * b[0] + a[1] * b[1] + c[0] * d0) * pow(c[1], -1, P) % P
        else:           # lane 1: a1 b0 + a0 b1 - c1 d0 - c0 d1 = t R
            d1 = (a[1] * b[0] + a[0] * b[1] - c[1] * d0 - t * RQ) * pow(c[0], -1, P) % P
        out.append((a, b, c, (d0, d1)))
    return out


@pytest.mark.parametrize("field,op", [("Fq2", "MUL"), ("Fq2h", "MUL"), ("Fq2", "SQR"), ("Fq2h", "SQR"),
                                      ("Fq2h", "MUL_SUB"), ("Fq2", "MUL_SUB")],
                         ids=["Fq2-MUL", "Fq2h-MUL", "Fq2-SQR", "Fq2h-SQR", "Fq2h-MUL_SUB", "Fq2-MUL_SUB"])
def test_final_subtraction_fq2(zkp, ctx, field, op):
    """The signed forms (fq_redc2<true>, the lane pair's f_mul / f_mul_sub)
    subtract only for results below ~3p^2/R, a 2^-9 sliver of the field; per
    output coefficient at least 32 cases here take it and 32 do not."""
    rng = random.Random(0x2F2 + len(op))
    if op == "MUL":
        cases = built_fq2_mul(rng)
        if field == "Fq2":
            res = [(fm.fq_redc2(True, a[0], b[0], a[1], b[1]), fm.fq_redc2(False, a[0], b[1], a[1], b[0]))
                   for a, b in cases]
        else:
            res = [fm.fq2h_mul(a, b) for a, b in cases]
    elif op == "SQR":
        cases = built_fq2_sqr(rng)
        # c1: fq_mul(a0, a1) doubled (Fq2, and Fq2h's select form) or fq_mul(2 a0, a1) (Fq2h's default)
        res = [(fm.mul(FQ, (a[0] + a[1]) % P, (a[0] - a[1]) % P), fm.mul(FQ, a[0], a[1])) for a, in cases]
        need_both([fm.takes_subtraction(FQ, fm.mul(FQ, 2 * a[0] % P, a[1])) for a, in cases], "f_sqr 2 a0 a1")
    elif field == "Fq2h":
        cases = built_fq2_mul_sub(rng)
        res = [fm.fq2h_mul_sub(*c) for c in cases]
    else:   # one lane per element: two lazy products and an Fq2 subtraction; the built product on either side
        prods = built_fq2_mul(rng)
        res = [(fm.fq_redc2(True, a[0], b[0], a[1], b[1]), fm.fq_redc2(False, a[0], b[1], a[1], b[0]))
               for a, b in prods]
        other = [((rng.randrange(P), rng.randrange(P)), (rng.randrange(P), rng.randrange(P))) for _ in prods]
        cases = [(a, b, c, d) for (a, b), (c, d) in zip(prods, other)] + \
                [(c, d, a, b) for (a, b), (c, d) in zip(prods, other)]
    for lane in (0, 1):
        need_both([fm.takes_subtraction(FQ, r[lane]) for r in res], "%s %s coefficient %d" % (field, op, lane))
    got = run_fq2(zkp, ctx, field, op, zip(*cases))
    assert all(g[0] < P and g[1] < P for g in got)
    check_equal(got, [ref_fq2(op, *c) for c in cases], cases, "%s %s built" % (field, op))


# ----------------------------------------------- lane placement of Fq2h ---
@pytest.mark.parametrize("op", ["MUL", "SQR", "MUL_SUB", "ADD", "SUB", "NEG", "IS_ZERO"])
def test_fq2h_lane_placement(zkp, ctx, op):
    """Neighbouring lane pairs hold different data (an edge element beside a
    random one), the last quad, row and wave are partly filled, and the same
    element gives the same words wherever it sits: the list rotated by one
    and by two positions gives the rotated results."""
    rng = random.Random(0x1A9E + len(op))
    edges = fq2_values(rng)[:121]
    built = {"MUL": built_fq2_mul, "SQR": built_fq2_sqr, "MUL_SUB": built_fq2_mul_sub}.get(op, lambda r: [])(rng)
    arity = {"MUL": 2, "ADD": 2, "SUB": 2, "MUL_SUB": 4}.get(op, 1)
    base = []
    for i in range(max(LANE_SIZES)):
        if i % 2 == 0:      # an edge element: zeros and p - 1 in one half or both
            base.append(tuple(edges[(i // 2 * (k + 3) + k) % len(edges)] for k in range(arity)))
        elif built and i % 4 == 1:
            base.append(built[i % len(built)])
        else:
            base.append(tuple((rng.randrange(P), rng.randrange(P)) for _ in range(arity)))
    if op == "IS_ZERO":
        base[0], base[1], base[2], base[3] = ((0, 0),), ((0, 5),), ((7, 0),), ((0, 0),)
    want_all = [ref_fq2(op, *c) for c in base]
    for n in LANE_SIZES:
        for rot in (0, 1, 2):
            idx = [(i + rot) % n for i in range(n)]
            cases = [base[i] for i in idx]
            got = run_fq2(zkp, ctx, "Fq2h", op, zip(*cases))
            check_equal(got, [want_all[i] for i in idx], cases, "Fq2h %s n=%d rotated by %d" % (op, n, rot))


def test_fq2_is_zero_and_inverse_with_one_zero_half(zkp, ctx):
    rng = random.Random(0x15E0)
    vals = [(0, 0), (0, 1), (1, 0), (0, P - 1), (P - 1, 0), (0, RQ % P), (RQ % P, 0)]
    vals += [(0, rng.randrange(1, P)) for _ in range(40)] + [(rng.randrange(1, P), 0) for _ in range(40)]
    vals += [(0, 0), (rng.randrange(P), rng.randrange(P)), (0, 0)]
    cases = [(a,) for a in vals]
    raw = ctx.test_field(zkp.ZK_TEST_FIELD_FQ2H, zkp.ZK_TEST_FOP_IS_ZERO, fm.to_words2(vals))
    lanes = raw.reshape(len(vals), 2, 12)
    assert not lanes[:, :, 1:].any()
    assert np.array_equal(lanes[:, 0, 0], lanes[:, 1, 0]), "the lanes of a pair disagree on IS_ZERO"
    assert [int(x) for x in lanes[:, 0, 0]] == [1 if a == (0, 0) else 0 for a in vals]
    got = run_fq2(zkp, ctx, "Fq2", "INV", zip(*cases))
    check_equal(got, [ref_fq2("INV", a) for a in vals], cases, "Fq2 INV")
    one = (RQ % P, 0)
    back = run_fq2(zkp, ctx, "Fq2", "MUL", [vals, got])
    assert back == [one if a != (0, 0) else (0, 0) for a in vals]


def test_field_hook_argument_errors(zkp, ctx):
    import ctypes as C
    T, h = zkp.test_lib(), C.c_void_p(ctx._h)
    a = fm.to_words([1, 2], 12)
    out = np.zeros_like(a)
    pa, po = C.c_void_p(a.ctypes.data), C.c_void_p(out.ctypes.data)

    def call(ctxh, field, op, a_, b_, c_, d_, n, o_):
        return T.zk_test_field(ctxh, C.c_int(field), C.c_int(op), a_, b_, c_, d_, C.c_size_t(n), o_)
    FQf, FRf, F2, F2H = (zkp.ZK_TEST_FIELD_FQ, zkp.ZK_TEST_FIELD_FR, zkp.ZK_TEST_FIELD_FQ2, zkp.ZK_TEST_FIELD_FQ2H)
    E = zkp.ZK_ERR_ARG
    assert call(None, FQf, zkp.ZK_TEST_FOP_NEG, pa, None, None, None, 2, po) == E
    assert call(h, FQf, zkp.ZK_TEST_FOP_NEG, None, None, None, None, 2, po) == E
    assert call(h, FQf, zkp.ZK_TEST_FOP_NEG, pa, None, None, None, 2, None) == E
    assert call(h, FQf, zkp.ZK_TEST_FOP_MUL, pa, None, None, None, 2, po) == E
    assert call(h, FQf, zkp.ZK_TEST_FOP_MUL_SUB, pa, pa, pa, None, 2, po) == E
    assert call(h, 9, zkp.ZK_TEST_FOP_NEG, pa, None, None, None, 2, po) == E
    assert call(h, zkp.ZK_TEST_FIELD_FQC, zkp.ZK_TEST_FOP_NEG, pa, None, None, None, 2, po) == E
    assert call(h, FQf, 13, pa, None, None, None, 2, po) == E
    assert call(h, FQf, -1, pa, None, None, None, 2, po) == E
    for field, op in ((FQf, "MUL_LAZY"), (FRf, "MUL_SUB"), (FRf, "FQ_INV"), (F2, "DBL"), (F2, "TO_MONT"),
                      (F2H, "INV"), (F2, "IS_ZERO"), (FQf, "IS_ZERO"), (F2H, "FROM_MONT")):
        assert call(h, field, fop(zkp, op), pa, pa, pa, pa, 1, po) == E, (field, op)
    assert not out.any()
    assert call(h, FQf, zkp.ZK_TEST_FOP_MUL, None, None, None, None, 0, None) == zkp.ZK_OK   # n = 0: nothing to do
    assert call(h, FQf, zkp.ZK_TEST_FOP_NEG, pa, None, None, None, 2, po) == zkp.ZK_OK
    assert fm.from_words(out) == [P - 1, P - 2]
