"""A Python-integer restatement of the device's Montgomery products
(csrc/ff.hpp): radix-2^LB product scanning with the reduction interleaved per
column, unsigned (fp_mul / fp_sqr) and signed with the 4p^2 column offset
(fq_redc2, fq_mul_sub, the lane-pair f_mul / f_mul_sub).

This is NOT the correctness reference of the GPU tests (that is a b / R mod m
in plain integers).  It classifies inputs -- did this case take the final
subtraction? -- and it checks the column-overflow claims of ff.hpp's comments.
Also here: the raw-word helpers the field and curve GPU tests share."""
import re
from collections import namedtuple

import numpy as np

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001

# m: modulus, N: 32-bit storage words, LB / NL: bits and count of the multiply limbs
Params = namedtuple("Params", "name m N LB NL")
FQ = Params("Fq", P, 12, 28, 14)
FR = Params("Fr", R, 8, 29, 9)


def mont_r(prm):
    return 1 << (prm.LB * prm.NL)


def limbs(x, bits, count):
    mask = (1 << bits) - 1
    return [(x >> (bits * i)) & mask for i in range(count)]


def unlimbs(v, bits):
    return sum(int(x) << (bits * i) for i, x in enumerate(v))


# what Result holds: value = the packed result before fp_reduce_once,
# col_min / col_max = the extreme column sums (after the m_k MOD[0] term)
Result = namedtuple("Result", "value col_min col_max")


def redc(prm, products, offset=0):
    """One product-scanning pass over `products`, a list of (sign, x, y) with
    x, y integers below 2^(LB NL): value = (sum sign x y + offset + M m) / R
    exactly as the device's column loop computes it (arithmetic-shift carries,
    m_k from the low LB bits).  offset is added column-wise as the device adds
    P4SQ28 (its top limb after the last carry)."""
    LB, M = prm.LB, prm.NL
    mask = (1 << LB) - 1
    ml = limbs(prm.m, LB, M)
    inv = (-pow(prm.m, -1, 1 << LB)) & mask
    ops = [(s, limbs(x, LB, M), limbs(y, LB, M)) for s, x, y in products]
    off = limbs(offset, LB, 2 * M)
    mk, r = [0] * M, [0] * M
    carry, lo, hi = 0, 0, 0
    for k in range(2 * M - 1):
        acc = carry + off[k]
        for i in range(M):
            j = k - i
            if 0 <= j < M:
                for s, x, y in ops:
                    acc += s * x[i] * y[j]
            if i < k and 1 <= j < M:
                acc += mk[i] * ml[j]
        if k < M:
            mk[k] = (acc * inv) & mask
            acc += mk[k] * ml[0]
        else:
            r[k - M] = acc & mask
        lo, hi = min(lo, acc), max(hi, acc)
        carry = acc >> LB   # Python's >> floors, as the device's arithmetic shift
    r[M - 1] = carry + off[2 * M - 1]
    return Result(unlimbs(r, LB), lo, hi)


def mul(prm, a, b):
    """fp_mul / fp_sqr (the squaring's columns hold the same sums)."""
    return redc(prm, [(1, a, b)])


def fq_redc2(sub, x0, y0, x1, y1):
    """fq_redc2<SUB>: x0 y0 -/+ x1 y1."""
    return redc(FQ, [(1, x0, y0), (-1 if sub else 1, x1, y1)], 4 * P * P if sub else 0)


def fq_mul_sub(a, b, c, d):
    return fq_redc2(True, a, b, c, d)


def fq2h_mul(a, b):
    """The lane pair's f_mul: (lane 0, lane 1), both with the 4p^2 offset."""
    return (redc(FQ, [(1, a[0], b[0]), (-1, a[1], b[1])], 4 * P * P),
            redc(FQ, [(1, a[1], b[0]), (1, a[0], b[1])], 4 * P * P))


def fq2h_mul_sub(a, b, c, d):
    return (redc(FQ, [(1, a[0], b[0]), (-1, a[1], b[1]), (-1, c[0], d[0]), (1, c[1], d[1])], 4 * P * P),
            redc(FQ, [(1, a[1], b[0]), (1, a[0], b[1]), (-1, c[1], d[0]), (-1, c[0], d[1])], 4 * P * P))


def takes_subtraction(prm, res):
    return res.value >= prm.m


def column_bound(prm, plus, minus, offset=0):
    """Worst-case column sums with every limb (operands, m_k, modulus) at
    2^LB - 1: `plus` / `minus` products are added / subtracted.  Returns
    (lowest, highest) over all columns, the carry taken to its fixed point."""
    LB, M = prm.LB, prm.NL
    t = ((1 << LB) - 1) ** 2
    off = max(limbs(offset, LB, 2 * M)) if offset else 0
    hi = lo = 0
    for _ in range(8):
        hi = (hi >> LB) + off + M * t * plus + M * t
        lo = (lo >> LB) - M * t * minus
    return lo, hi


def parse_constants(path):
    """{struct: {name: int | [ints]}} of csrc/constants.hpp's FqParams / FrParams."""
    with open(path) as f:
        src = f.read()
    out = {}
    for struct in ("FqParams", "FrParams"):
        body = re.search(r"struct %s \{(.*?)\n\};" % struct, src, re.S).group(1)
        d = {}
        for name, val in re.findall(r"static constexpr uint32_t (\w+)\[\d+\] = \{([^}]*)\};", body):
            d[name] = [int(x, 16) for x in val.split(",")]
        for name, val in re.findall(r"static constexpr uint32_t (\w+) = (0x[0-9a-f]+);", body):
            d[name] = int(val, 16)
        ints = re.search(r"static constexpr int ([^;]*);", body).group(1)
        for name, val in re.findall(r"(\w+) = (\d+)", ints):
            d[name] = int(val)
        out[struct] = d
    return out


# ---- raw device words <-> integers (the GPU tests' side of the hooks) ----
def to_words(vals, nwords):
    """ints -> (n, nwords) uint32, little-endian."""
    raw = b"".join(int(v).to_bytes(4 * nwords, "little") for v in vals)   # raises unless 0 <= v < 2^(32 nwords)
    return np.frombuffer(raw, dtype="<u4").reshape(-1, nwords).astype(np.uint32)


def from_words(arr):
    """(n, nwords) uint32 -> ints."""
    return [int.from_bytes(row.tobytes(), "little") for row in np.ascontiguousarray(arr, dtype="<u4")]


def to_words2(pairs):
    """[(c0, c1)] -> (n, 24) uint32."""
    return np.concatenate([to_words([a for a, _ in pairs], 12), to_words([b for _, b in pairs], 12)], axis=1)


def from_words2(arr):
    arr = np.asarray(arr)
    return list(zip(from_words(arr[:, :12]), from_words(arr[:, 12:])))
