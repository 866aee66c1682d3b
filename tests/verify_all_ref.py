"""The reference of the sound batch check (zk_groth16_verify_all_sound):
batch_equation_holds computes c_k A_k, S_C = sum c_k C_k, IC* and s alpha with
oracle/pyref.py's big-integer curve code and asks the host pairing
(zkp.pairing_product_is_one) over the n + 3 pairs
    prod_k e(c_k A_k, B_k) e(-s alpha, beta) e(-IC*, gamma) e(-S_C, delta) == 1.
Nothing of the GPU path is in it.  A pyref multiplication by a 128-bit
coefficient costs tens of ms, so k P is cached per (point, k): the tests draw
their coefficients from a small pool and repeat a few proofs, and batches with
the same coefficients and inputs share s and the t_i."""
import numpy as np
import pyref as P

R = P.R
_MUL = {}


def g1_point(words):
    w = [int(x) for x in words]
    if w[12]:
        return P.INF
    return (P.Fq1(sum(w[i] << (64 * i) for i in range(6))), P.Fq1(sum(w[6 + i] << (64 * i) for i in range(6))))


def _key(p):
    return None if p is P.INF else (p[0].v, p[1].v)


def g1_mul(p, c):
    """c p, cached"""
    k = (_key(p), c)
    if k not in _MUL:
        _MUL[k] = P.G1.mul(p, c) if p is not P.INF and c else P.INF
    return _MUL[k]


def _int(limbs):
    a = np.asarray(limbs, dtype=np.uint64).reshape(-1)
    return sum(int(w) << (64 * i) for i, w in enumerate(a))


def input_ints(inputs):
    """rows of ints, or an (n, l, 4) array of limbs -> rows of ints"""
    if isinstance(inputs, np.ndarray) and inputs.ndim == 3:
        return [[_int(x) for x in row] for row in inputs]
    return [[int(x) for x in row] for row in inputs]


def batch_parts(vk, proofs, inputs, coeffs):
    """(the n points c_k A_k, S_C, the scalars [s, t_0 ..]) -- proofs as rows of 51 words"""
    rows = input_ints(inputs)
    ca = [g1_mul(g1_point(w[:13]), c) for w, c in zip(proofs, coeffs)]
    s_c = P.INF
    for w, c in zip(proofs, coeffs):
        s_c = P.G1.add(s_c, g1_mul(g1_point(w[38:51]), c))
    scal = [sum(coeffs) % R] + [sum(c * row[i] for c, row in zip(coeffs, rows)) % R for i in range(vk.num_public)]
    return ca, s_c, scal


def batch_equation_holds(zkp, pyref, vk, proofs, inputs, coeffs):
    """proofs: n Proof objects or rows of 51 words (well-formed, inputs below r); coeffs: n ints"""
    words = [np.asarray(getattr(p, "words", p), dtype=np.uint64) for p in proofs]
    assert len(words) == len(coeffs) == len(inputs)
    ca, s_c, scal = batch_parts(vk, words, inputs, coeffs)
    neg = pyref.G1.neg
    ic = pyref.INF
    for t, w in zip(scal, vk.ic_g1):
        base = g1_point(w)
        ic = pyref.G1.add(ic, g1_mul(base, t))
    s_alpha = g1_mul(g1_point(vk.point("alpha_g1")), scal[0])
    g1 = [pyref.g1_words(p) for p in ca] + [pyref.g1_words(neg(p)) for p in (s_alpha, ic, s_c)]
    g2 = [w[13:38] for w in words] + [vk.point("beta_g2"), vk.point("gamma_g2"), vk.point("delta_g2")]
    return zkp.pairing_product_is_one(g1, g2)
