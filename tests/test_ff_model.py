"""CPU checks of tests/ff_model.py, the limb model the field GPU tests use to
classify their inputs: it computes a b / R mod m, the generated constants it
and the device share are the values p and r imply, and no column sum of any
product form leaves its 64-bit integer type at worst-case limbs."""
import os
import random

import pytest

import ff_model as fm
from ff_model import FQ, FR, P


def edge_values(prm, full_width):
    m, top = prm.m, (1 << (32 * prm.N)) - 1
    v = [0, 1, 2, m - 1, m - 2, (m - 1) // 2, (m + 1) // 2, fm.mont_r(prm) % m, fm.mont_r(prm) ** 2 % m]
    if full_width:
        v += [m, m + 1, 2 * m - 1, top]
    return v


@pytest.mark.parametrize("prm", [FQ, FR], ids=["Fq", "Fr"])
def test_unsigned_model_is_the_montgomery_product(prm):
    rng = random.Random(0xF1E1D + prm.N)
    m, rinv = prm.m, pow(fm.mont_r(prm), -1, prm.m)
    vals = edge_values(prm, True) + [rng.getrandbits(32 * prm.N) for _ in range(40)]
    vals += [rng.randrange(m) for _ in range(40)]
    for a in vals:
        for b in rng.sample(vals, 12) + [a]:
            res = fm.mul(prm, a, b)
            assert res.value < 2 * m and res.value % m == a * b * rinv % m, (hex(a), hex(b))
            assert 0 <= res.col_min and res.col_max < 1 << 64


def test_signed_model_is_the_difference_of_products():
    rng = random.Random(0x51D)
    rinv = pow(fm.mont_r(FQ), -1, P)
    vals = edge_values(FQ, False) + [rng.randrange(P) for _ in range(30)]
    quads = [tuple(rng.choice(vals) for _ in range(4)) for _ in range(300)]
    quads += [(0, 0, P - 1, P - 1), (P - 1, P - 1, 0, 0), (P - 1, P - 1, P - 1, P - 1), (0, 5, P - 1, P - 1)]
    for a, b, c, d in quads:
        res = fm.fq_mul_sub(a, b, c, d)
        assert res.value < 2 * P and res.value % P == (a * b - c * d) * rinv % P
        res = fm.fq_redc2(False, a, b, c, d)
        assert res.value < 2 * P and res.value % P == (a * b + c * d) * rinv % P
        assert -(1 << 63) <= res.col_min and res.col_max < 1 << 63
    for a0, a1, b0, b1 in quads[:120] + quads[-4:]:
        c0, c1, d0, d1 = rng.choice(quads)
        r0, r1 = fm.fq2h_mul((a0, a1), (b0, b1))
        assert r0.value < 2 * P and r0.value % P == (a0 * b0 - a1 * b1) * rinv % P
        assert r1.value < 2 * P and r1.value % P == (a1 * b0 + a0 * b1) * rinv % P
        r0, r1 = fm.fq2h_mul_sub((a0, a1), (b0, b1), (c0, c1), (d0, d1))
        assert r0.value < 2 * P and r0.value % P == (a0 * b0 - a1 * b1 - c0 * d0 + c1 * d1) * rinv % P
        assert r1.value < 2 * P and r1.value % P == (a1 * b0 + a0 * b1 - c1 * d0 - c0 * d1) * rinv % P
        for r in (r0, r1):
            assert -(1 << 63) <= r.col_min and r.col_max < 1 << 63


def test_subtraction_window_of_the_offset_forms():
    """With the 4p^2 offset the value before the final subtraction lies in
    [3p^2/R, p + 5p^2/R): results below 3p^2/R always take the subtraction,
    results above 5p^2/R never do (what the GPU tests' constructed cases and
    ff.hpp's comment rely on)."""
    rng = random.Random(0x0FF5E7)
    Rq = fm.mont_r(FQ)
    lo, hi = 3 * P * P // Rq, 5 * P * P // Rq + 1
    for k in range(200):
        a, b, c = (rng.randrange(1, P) for _ in range(3))
        t = rng.randrange(lo) if k % 2 == 0 else hi + rng.randrange(1 << 300)
        d = (a * b - t * Rq) * pow(c, -1, P) % P
        res = fm.fq_mul_sub(a, b, c, d)
        assert res.value % P == t
        assert fm.takes_subtraction(FQ, res) == (k % 2 == 0)


def test_constants_match_the_moduli(zkp):
    c = fm.parse_constants(os.path.join(zkp.CSRC, "constants.hpp"))
    for prm, d in ((FQ, c["FqParams"]), (FR, c["FrParams"])):
        m, Rm = prm.m, fm.mont_r(prm)
        assert (d["N"], d["NL"], d["LB"]) == (prm.N, prm.NL, prm.LB)
        assert 32 * prm.N <= prm.LB * prm.NL        # every N-word operand fits the multiply limbs
        assert fm.unlimbs(d["MOD"], 32) == m and len(d["MOD"]) == prm.N
        assert d["MODL"] == fm.limbs(m, prm.LB, prm.NL)
        assert d["INVL"] == (-pow(m, -1, 1 << prm.LB)) % (1 << prm.LB)
        assert fm.unlimbs(d["ONE"], 32) == Rm % m and len(d["ONE"]) == prm.N
        assert fm.unlimbs(d["R2"], 32) == Rm * Rm % m and len(d["R2"]) == prm.N
    q = c["FqParams"]
    assert q["MOD28"] == fm.limbs(P, 28, 14) and q["INV28"] == q["INVL"]
    assert len(q["P4SQ28"]) == 28 and all(x < 1 << 28 for x in q["P4SQ28"])
    assert fm.unlimbs(q["P4SQ28"], 28) == 4 * P * P


def test_column_sums_stay_inside_64_bits():
    """ff.hpp: "a column holds at most 2*NL products (Fq < 2^61, Fr < 2^62.2)"
    for the unsigned products; the signed forms hold up to four limb products
    and the modulus products per column in an int64_t."""
    lo, hi = fm.column_bound(FQ, 1, 0)
    assert lo == 0 and hi < 1 << 61
    lo, hi = fm.column_bound(FR, 1, 0)
    assert lo == 0 and hi < 2 ** 62.2 < 1 << 64
    for plus, minus in ((1, 1), (2, 0), (2, 2)):   # fq_redc2<true> / lane 0, lane 1 of f_mul, f_mul_sub
        lo, hi = fm.column_bound(FQ, plus, minus, 4 * P * P)
        assert -(1 << 63) < lo and hi < 1 << 63
    # and the model agrees on the most extreme operands the contracts allow
    top = (1 << 384) - 1
    assert fm.mul(FQ, top, top).col_max < 1 << 61
    assert fm.mul(FR, (1 << 256) - 1, (1 << 256) - 1).col_max < 2 ** 62.2
    r0, r1 = fm.fq2h_mul_sub((0, P - 1), (0, P - 1), (P - 1, 0), (P - 1, 0))   # lane 0 at its most negative
    assert r0.col_min < 0 and -(1 << 63) < r0.col_min and r0.value < 2 * P
    r0, r1 = fm.fq2h_mul_sub((P - 1, P - 1), (P - 1, P - 1), (0, 0), (0, 0))   # lane 1 at its most positive
    assert r1.col_max < 1 << 63 and r1.value < 2 * P
