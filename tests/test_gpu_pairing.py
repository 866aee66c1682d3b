"""GPU batch verification (csrc/pairing.hpp, pairing.hip): the device Fq12
tower and final exponentiation against a big-integer Fq12 written here, the
device pairing against bilinearity as Fq12 VALUES, zk_pairing_products against
the host's zk_pairing_product_is_one, and zk_groth16_verify_many against the
host verifier proof by proof.

The Python Fq12 below is schoolbook in the basis 1, w, ..., w^5 over Fq2
(w^6 = xi = 1 + u), which is host_pairing.hpp's tower written flat: tower
coefficient (c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2) sits at w^(0, 2, 4, 1, 3, 5).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
X_ABS = 0xD201000000010000
FINAL_EXP = (P ** 12 - 1) // R
WPOW = (0, 2, 4, 1, 3, 5)
M64 = (1 << 64) - 1


# ------------------------------------------------- big-integer Fq12 ----
def f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2xi(a):
    return ((a[0] - a[1]) % P, (a[0] + a[1]) % P)


def f2inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], P - 2, P)
    return (a[0] * n % P, -a[1] * n % P)


def f2pow(a, e):
    acc = (1, 0)
    while e:
        if e & 1:
            acc = f2mul(acc, a)
        a = f2mul(a, a)
        e >>= 1
    return acc


Z2 = (0, 0)
ONE = ((1, 0),) + (Z2,) * 5
ZERO = (Z2,) * 6


def mul(a, b):
    acc = [Z2] * 11
    for i in range(6):
        if a[i] == Z2:
            continue
        for j in range(6):
            k = WPOW[i] + WPOW[j]
            acc[k] = f2add(acc[k], f2mul(a[i], b[j]))
    out = [f2add(acc[k], f2xi(acc[k + 6])) if k + 6 <= 10 else acc[k] for k in range(6)]
    return tuple(out[WPOW[j]] for j in range(6))


def power(a, e):
    acc = ONE
    for bit in bin(e)[2:]:
        acc = mul(acc, acc)
        if bit == "1":
            acc = mul(acc, a)
    return acc


def conj(a):
    """a^(p^6): w -> -w"""
    return tuple(a[j] if WPOW[j] % 2 == 0 else f2sub(Z2, a[j]) for j in range(6))


_FROB = {}


def frob(a, k):
    """a^(p^k), k = 1, 2, from (c w^i)^(p^k) = c^(p^k) w^i xi^(i (p^k - 1) / 6); checked against
    power() in test_tower_frobenius"""
    if k not in _FROB:
        _FROB[k] = [f2pow((1, 1), i * (P ** k - 1) // 6) for i in range(6)]
    co = _FROB[k]
    return tuple(f2mul(a[j] if k % 2 == 0 else (a[j][0], -a[j][1] % P), co[WPOW[j]]) for j in range(6))


def inv(a):
    """1 / a: a conj(a) lies in Fq6 (even powers of w); its inverse by the norm to Fq2"""
    n = mul(a, conj(a))
    assert n[3] == n[4] == n[5] == Z2
    a0, a1, a2 = n[0], n[1], n[2]
    t0 = f2sub(f2mul(a0, a0), f2xi(f2mul(a1, a2)))
    t1 = f2sub(f2xi(f2mul(a2, a2)), f2mul(a0, a1))
    t2 = f2sub(f2mul(a1, a1), f2mul(a0, a2))
    d = f2inv(f2add(f2mul(a0, t0), f2xi(f2add(f2mul(a2, t1), f2mul(a1, t2)))))
    r = mul(conj(a), (f2mul(t0, d), f2mul(t1, d), f2mul(t2, d), Z2, Z2, Z2))
    assert mul(r, a) == ONE
    return r


def words(a):
    """Fq12 -> 72 canonical u64 words in tower order"""
    return [(c >> (64 * i)) & M64 for co in a for c in co for i in range(6)]


def unwords(w):
    v = [sum(int(w[6 * k + i]) << (64 * i) for i in range(6)) for k in range(12)]
    return tuple((v[2 * j], v[2 * j + 1]) for j in range(6))


def to_array(elems):
    return np.array([words(a) for a in elems], dtype=np.uint64).reshape(-1, 72)


def from_array(arr):
    return [unwords(row) for row in arr]


class _Rng:
    def __init__(self, pyref, seed):
        self.r = pyref.SplitMix64(seed)

    def fq(self):
        return sum(self.r.next() << (64 * i) for i in range(6)) % P

    def fq12(self):
        return tuple((self.fq(), self.fq()) for _ in range(6))


@pytest.fixture(scope="module")
def elems(pyref):
    """66 random elements (past a wave boundary), then 0, 1 and elements with zero coefficients"""
    rng = _Rng(pyref, 0xF12)
    out = [rng.fq12() for _ in range(66)]
    a = rng.fq12()
    out += [ZERO, ONE, (a[0], Z2, a[2], Z2, Z2, a[5]), ((a[0][0], 0), (0, a[1][1]), Z2, Z2, a[4], Z2)]
    return out


def _run(zkp, ctx, op, a, b=None):
    """the hook on a (and b) with a sentinel row past n, which must stay untouched"""
    A = np.concatenate([to_array(a), np.full((1, 72), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)])
    B = None if b is None else np.concatenate([to_array(b), np.zeros((1, 72), dtype=np.uint64)])
    out = np.full_like(A, 0xA5A5A5A5A5A5A5A5)
    rc = zkp.test_lib().zk_test_fq12(C.c_void_p(ctx._h), C.c_int(op), C.c_void_p(A.ctypes.data),
                                     C.c_void_p(B.ctypes.data) if B is not None else None, C.c_size_t(len(a)),
                                     C.c_void_p(out.ctypes.data))
    assert rc == 0
    assert (out[-1] == 0xA5A5A5A5A5A5A5A5).all()
    return from_array(out[:-1])


# ------------------------------------------------------- tower hook ----
def test_tower_mul_sqr_conj(zkp, ctx, elems):
    b = elems[1:] + elems[:1]
    assert _run(zkp, ctx, zkp.ZK_TEST_FQ12_MUL, elems, b) == [mul(x, y) for x, y in zip(elems, b)]
    assert _run(zkp, ctx, zkp.ZK_TEST_FQ12_SQR, elems) == [mul(x, x) for x in elems]
    assert _run(zkp, ctx, zkp.ZK_TEST_FQ12_CONJ, elems) == [conj(x) for x in elems]


def test_tower_line_mul(zkp, ctx, elems):
    # b's line coefficients: c0.c0, c0.c1, c1.c1; everything else in b is ignored by the hook
    lines = [(y[0], y[1], Z2, Z2, y[4], Z2) for y in elems[2:] + elems[:2]]
    lines[5] = (lines[5][0], lines[5][1], Z2, Z2, (lines[5][4][0], 0), Z2)   # an Fq-valued c1.c1, as a fixed line has
    noisy = [(l[0], l[1], x[2], x[3], l[4], x[5]) for l, x in zip(lines, elems)]
    assert _run(zkp, ctx, zkp.ZK_TEST_FQ12_LINE_MUL, elems, noisy) == [mul(x, l) for x, l in zip(elems, lines)]


def test_tower_inv(zkp, ctx, elems):
    got = _run(zkp, ctx, zkp.ZK_TEST_FQ12_INV, elems)
    for x, y in zip(elems, got):
        assert mul(x, y) == (ZERO if x == ZERO else ONE)


def test_tower_frobenius(zkp, ctx, elems):
    g1 = _run(zkp, ctx, zkp.ZK_TEST_FQ12_FROB1, elems)
    g2 = _run(zkp, ctx, zkp.ZK_TEST_FQ12_FROB2, elems)
    for i in (0, 63, 64, 65, 67, 68):        # both sides of the wave boundary, 1, a sparse element
        assert g1[i] == power(elems[i], P)
        assert g2[i] == power(elems[i], P * P)
    assert g1 == [frob(x, 1) for x in elems]
    assert g2 == [frob(x, 2) for x in elems]


def _cyclotomic(a):
    """a^((p^6 - 1)(p^2 + 1))"""
    m = mul(conj(a), inv(a))
    return mul(frob(m, 2), m)


def test_tower_cyclotomic_square(zkp, ctx, elems):
    cyc = [_cyclotomic(a) for a in elems[:5]] + [ONE]
    assert cyc[0] == power(elems[0], (P ** 6 - 1) * (P * P + 1))
    for m in cyc:
        assert mul(m, conj(m)) == ONE
    assert _run(zkp, ctx, zkp.ZK_TEST_FQ12_CYC_SQR, cyc) == [mul(m, m) for m in cyc]


def test_final_exponentiation(zkp, ctx, elems):
    a = elems[:3]
    assert _run(zkp, ctx, zkp.ZK_TEST_FQ12_FINAL_EXP, a) == [power(x, zkp.FINAL_EXP_C * FINAL_EXP) for x in a]


# ---------------------------------------------------------- GT hook ----
def g1w(pyref, p):
    return np.array(pyref.g1_words(p), dtype=np.uint64)


def g2w(pyref, p):
    return np.array(pyref.g2_words(p), dtype=np.uint64)


def test_pairing_values_are_bilinear(zkp, ctx, pyref):
    G1, G2, g1, g2 = pyref.G1, pyref.G2, pyref.G1.gen, pyref.G2.gen
    a, b, a2, b2 = 0xDEADBEEF12345, 0xC0FFEE99, 0x1234567, R - 5
    pairs = [(g1, g2), (G1.mul(g1, a), G2.mul(g2, b)), (G1.mul(g1, a2), g2), (g1, G2.mul(g2, b2)),
             (None, g2), (g1, None)]
    got = from_array(ctx.test_pairing_gt([g1w(pyref, p) for p, _ in pairs], [g2w(pyref, q) for _, q in pairs]))
    g = got[0]
    assert g != ONE and power(g, R) == ONE
    assert got[1] == power(g, a * b % R)
    assert got[2] == power(g, a2)
    assert got[3] == power(g, b2)
    assert got[4] == ONE and got[5] == ONE


def test_pairing_value_of_the_generators(zkp, ctx, pyref):
    """The device's e(G1, G2) is host_pairing.hpp's Miller loop (affine, written here in Python)
    raised to c (p^12 - 1) / r: the same pairing, not just some bilinear map."""
    F = pyref.Fq2
    (xp, yp), Q = (pyref.G1.gen[0].v, pyref.G1.gen[1].v), pyref.G2.gen

    def line(lam, tx, ty):
        c0, c1 = lam * tx - ty, -(lam * xp)
        return ((c0.c0, c0.c1), (c1.c0, c1.c1), Z2, Z2, (yp, 0), Z2)

    tx, ty, f = Q[0], Q[1], ONE
    for i in range(62, -1, -1):
        lam = (tx * tx * 3) * (ty * 2).inv()
        f = mul(mul(f, f), line(lam, tx, ty))
        nx = lam * lam - tx - tx
        tx, ty = nx, lam * (tx - nx) - ty
        if (X_ABS >> i) & 1:
            la = (Q[1] - ty) * (Q[0] - tx).inv()
            f = mul(f, line(la, tx, ty))
            ax = la * la - tx - Q[0]
            tx, ty = ax, la * (tx - ax) - ty
    assert isinstance(tx, F)
    want = power(conj(f), zkp.FINAL_EXP_C * FINAL_EXP)
    got = from_array(ctx.test_pairing_gt([g1w(pyref, pyref.G1.gen)], [g2w(pyref, Q)]))[0]
    assert got == want


# ------------------------------------------------- pairing_products ----
@pytest.fixture()
def chunk64(zkp, ctx):
    ctx.set_option(zkp.ZK_OPT_VERIFY_CHUNK, 64)
    yield
    ctx.set_option(zkp.ZK_OPT_VERIFY_CHUNK, 65536)


@pytest.fixture(scope="module")
def product_cases(zkp, pyref):
    """test_verifier.py::test_pairing_bilinear's cases as (g1 points, g2 points, host verdict)"""
    G1, G2, g1, g2 = pyref.G1, pyref.G2, pyref.G1.gen, pyref.G2.gen
    a, b = 0xDEADBEEF12345, 0xC0FFEE99
    Pt, Q = G1.mul(g1, a), G2.mul(g2, b)
    ab = G1.neg(G1.mul(g1, a * b % R))
    off = G1.neg(G1.mul(g1, (a * b + 1) % R))
    s = 0x5A5A_1234_5678_9ABC_DEF0_1111_2222_3333_4444_5555_6666_7777_8888_9999 % R
    two = [([Pt, ab], [Q, g2], True),                                                # e(aP, bQ) e(-abP, Q) = 1
           ([Pt, off], [Q, g2], False),                                              # off by one
           ([G1.mul(g1, 2), G1.neg(g1)], [g2, G2.mul(g2, 2)], True),                 # e(2P, Q) = e(P, 2Q)
           ([None, g1], [g2, None], True),                                           # infinity on either side
           ([G1.mul(g1, s), g1], [g2, G2.neg(G2.mul(g2, s))], True)]                 # full-width scalar
    one = [([g1], [g2], False), ([None], [g2], True), ([g1], [None], True)]          # non-degenerate; infinities
    four = [(two[0][0] + two[2][0], two[0][1] + two[2][1], True), (two[4][0] + two[1][0], two[4][1] + two[1][1], False),
            (two[3][0] + two[3][0], two[3][1] + two[3][1], True)]
    out = {}
    for k, cases in ((1, one), (2, two), (4, four)):
        rows = []
        for ps, qs, want in cases:
            pw, qw = [g1w(pyref, p) for p in ps], [g2w(pyref, q) for q in qs]
            host = zkp.pairing_product_is_one(pw, qw)
            assert host == want
            rows.append((np.array(pw), np.array(qw), host))
        out[k] = rows
    return out


def _corrupt(g1, g2, prod, k):
    """push the first finite point of product `prod` off its curve (an infinite point's
    coordinates are not looked at, here as on the host)"""
    for j in range(k * prod, k * (prod + 1)):
        if not g1[j][12]:
            g1[j][6] ^= 1
            return
        if not g2[j][24]:
            g2[j][13] ^= 1
            return
    raise AssertionError("a product of infinities only")


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("k", [1, 2, 4])
def test_pairing_products(zkp, ctx, product_cases, chunk64, k, n):
    cases = product_cases[k]
    pick = [cases[j % len(cases)] for j in range(n)]
    g1 = np.concatenate([c[0] for c in pick])
    g2 = np.concatenate([c[1] for c in pick])
    want = np.array([zkp.ZK_VERIFY_ACCEPT if c[2] else zkp.ZK_VERIFY_REJECT for c in pick], dtype=np.uint8)
    assert np.array_equal(ctx.pairing_products(g1, g2, k), want)
    # an off-curve point: MALFORMED for its product only (the last product: with n = 65, the
    # second launch), and the host refuses the same points
    bad1, bad2, want = g1.copy(), g2.copy(), want.copy()
    for prod in {n - 1, min(3, n - 1)}:
        _corrupt(bad1, bad2, prod, k)
        want[prod] = zkp.ZK_VERIFY_MALFORMED
        with pytest.raises(ValueError):
            zkp.pairing_product_is_one(bad1[k * prod:k * (prod + 1)], bad2[k * prod:k * (prod + 1)])
    assert np.array_equal(ctx.pairing_products(bad1, bad2, k), want)


# ------------------------------------------------------ verify_many ----
TOY_XY = [(3, 4), (0, 5), (1, 1), (2, 7), (5, 5), (6, 2), (9, 3), (4, 11)]


def _vk_of(zkp, ovk):
    return zkp.VerificationKey.from_points(ovk.field("alpha_g1"), ovk.field("beta_g2"), ovk.field("gamma_g2"),
                                           ovk.field("delta_g2"), ovk.ic_g1)


def _host_status(zkp, vk, words, inputs):
    try:
        ok = zkp.Verifier.verify(vk, zkp.Proof(words), inputs)
    except ValueError:
        return zkp.ZK_VERIFY_MALFORMED
    return zkp.ZK_VERIFY_ACCEPT if ok else zkp.ZK_VERIFY_REJECT


@pytest.fixture(scope="module")
def toy(zkp, oracle, pyref):
    """The reference's circuit x*y=z (x public) set up with [2,3,1,1,5] (derived scalars below 2^64),
    8 valid proofs from the oracle's prover and a pool of 16 (proof words, inputs, host status,
    status by construction or None)."""
    csr = oracle.CSR.from_constraints([({1: 1}, {2: 1}, {3: 1})], 4)
    rc, pk, ovk = oracle.setup(csr, [2, 3, 1, 1, 5], 1)
    assert rc == 0
    vk = _vk_of(zkp, ovk)
    rng = pyref.SplitMix64(4242)
    proofs = []
    for x, y in TOY_XY:
        rc, pr = oracle.prove(pk, csr, oracle.fr_array([1, x, y, x * y]), 1, rng.fr(), rng.fr())
        assert rc == 0
        proofs.append(np.array(pr, dtype=np.uint64))
    A, RJ, MF = zkp.ZK_VERIFY_ACCEPT, zkp.ZK_VERIFY_REJECT, zkp.ZK_VERIFY_MALFORMED
    pool = [(p, [x], A) for p, (x, _) in zip(proofs, TOY_XY)]
    t = proofs[0].copy(); t[:13] = proofs[1][:13]; pool.append((t, [3], RJ))             # another proof's A
    t = proofs[0].copy(); t[38:] = proofs[1][38:]; pool.append((t, [3], RJ))             # another proof's C
    pool.append((proofs[0], [5], RJ))                                                   # a wrong public input
    t = proofs[2].copy(); t[38 + 6] ^= 1; pool.append((t, [1], MF))                      # C off the curve
    t = proofs[3].copy(); t[:6] = [(P >> (64 * i)) & M64 for i in range(6)]; pool.append((t, [2], MF))   # A.x = p
    t = proofs[4].copy(); t[:13] = g1w(pyref, None); pool.append((t, [5], None))         # A = infinity
    pool.append((proofs[0], [3 + (5 << 64)], A))                                        # high limbs: lo64 decides
    pool.append((proofs[1], [7 << 64], A))                                              # lo64 = 0
    full = []
    for words, inp, want in pool:
        host = _host_status(zkp, vk, words, inp)
        assert want is None or host == want
        full.append((words, inp, host))
    return vk, full


def _raw_verify_many(zkp, ctx, vk, words, inputs, n_inputs):
    """the C entry point with a status buffer one longer than n: (rc, statuses, sentinel)"""
    n = len(words)
    st = np.full(n + 1, 0xAA, dtype=np.uint8)
    rc = zkp.lib().zk_groth16_verify_many(C.c_void_p(ctx._h), C.byref(vk.s), C.c_void_p(words.ctypes.data),
                                          C.c_void_p(inputs.ctypes.data) if inputs.size else None,
                                          C.c_size_t(n_inputs), C.c_size_t(n), C.c_void_p(st.ctypes.data))
    return rc, st[:n], st[n]


def _batch(zkp, pool, n, shift):
    pick = [pool[(j + shift) % len(pool)] for j in range(n)]
    words = np.ascontiguousarray([w for w, _, _ in pick], dtype=np.uint64)
    npub = len(pick[0][1])
    inputs = np.zeros((n, npub, 4), dtype=np.uint64)
    for j, (_, inp, _) in enumerate(pick):
        for k, v in enumerate(inp):
            inputs[j, k] = [(v >> (64 * i)) & M64 for i in range(4)]   # raw words: high limbs are kept
    want = np.array([h for _, _, h in pick], dtype=np.uint8)
    return words, inputs, want


@pytest.mark.parametrize("n,shift", [(1, 0), (1, 11), (63, 0), (64, 5), (65, 0), (130, 9)])
def test_verify_many_matches_the_host(zkp, ctx, toy, chunk64, n, shift):
    vk, pool = toy
    words, inputs, want = _batch(zkp, pool, n, shift)
    rc, st, sentinel = _raw_verify_many(zkp, ctx, vk, words, inputs, 1)
    assert rc == zkp.ZK_OK and sentinel == 0xAA
    assert np.array_equal(st, want)
    if n >= 16:
        assert {zkp.ZK_VERIFY_ACCEPT, zkp.ZK_VERIFY_REJECT, zkp.ZK_VERIFY_MALFORMED} == set(st.tolist())
    rc, again, _ = _raw_verify_many(zkp, ctx, vk, words, inputs, 1)
    assert rc == zkp.ZK_OK and again.tobytes() == st.tobytes()
    # the Python layers: statuses, then bools or the first malformed index
    proofs = [zkp.Proof(w) for w in words]
    assert np.array_equal(ctx.verify_many(vk, proofs, inputs), want)
    pairs = [(p, [int(zkp.from_limbs(row)) for row in inp]) for p, inp in zip(proofs, inputs)]
    bad = np.flatnonzero(want == zkp.ZK_VERIFY_MALFORMED)
    if len(bad):
        with pytest.raises(ValueError, match=rf"proof {int(bad[0])} "):
            zkp.Verifier.verify_many(vk, pairs, ctx)
    else:
        assert np.array_equal(zkp.Verifier.verify_many(vk, pairs, ctx), want == zkp.ZK_VERIFY_ACCEPT)


def _constructed(zkp, pyref, npub, seed):
    """test_verifier.py's _constructed: a key and a proof satisfying the Groth16 equation by
    construction (80-bit scalars keep the pyref multiplications short; C's scalar is full-width)"""
    G1, G2, g1, g2 = pyref.G1, pyref.G2, pyref.G1.gen, pyref.G2.gen
    rng = pyref.SplitMix64(seed)

    def sc():
        return (rng.next() << 16) | (rng.next() & 0xFFFF)

    al, be, ga, de, a, b = (sc() for _ in range(6))
    ks = [sc() for _ in range(npub + 1)]
    x = [rng.next() for _ in range(npub)]
    ic = (ks[0] + sum(xi * k for xi, k in zip(x, ks[1:]))) % R
    c = (a * b - al * be - ic * ga) * pow(de, R - 2, R) % R
    vk = zkp.VerificationKey.from_points(g1w(pyref, G1.mul(g1, al)), g2w(pyref, G2.mul(g2, be)),
                                         g2w(pyref, G2.mul(g2, ga)), g2w(pyref, G2.mul(g2, de)),
                                         [g1w(pyref, G1.mul(g1, k)) for k in ks])
    words = np.concatenate([g1w(pyref, G1.mul(g1, a)), g2w(pyref, G2.mul(g2, b)), g1w(pyref, G1.mul(g1, c))])
    return vk, words, x


@pytest.mark.parametrize("npub", [0, 3])
def test_verify_many_constructed_keys(zkp, ctx, pyref, chunk64, npub):
    vk, words, x = _constructed(zkp, pyref, npub, 70 + npub)
    A, RJ = zkp.ZK_VERIFY_ACCEPT, zkp.ZK_VERIFY_REJECT
    t = words.copy(); t[:13] = g1w(pyref, pyref.G1.gen)
    pool = [(words, x, A), (t, x, RJ)]
    if npub:
        pool.append((words, [(x[0] + 1) % (1 << 64)] + x[1:], RJ))
        pool.append((words, [xi + (5 << 64) for xi in x], A))
        pool.append((words, [x[0], x[1] + (1 << 64), x[2]], A))
    pool = [(w, inp, _host_status(zkp, vk, w, inp)) for w, inp, _ in pool]
    want_by_construction = [A, RJ, RJ, A, A][:len(pool)]
    assert [h for _, _, h in pool] == want_by_construction
    w, inputs, want = _batch(zkp, pool, 65, 0)
    rc, st, sentinel = _raw_verify_many(zkp, ctx, vk, w, inputs, npub)
    assert rc == zkp.ZK_OK and sentinel == 0xAA and np.array_equal(st, want)


def test_verify_many_error_returns(zkp, ctx, toy, pyref):
    vk, pool = toy
    words, inputs, want = _batch(zkp, pool, 3, 0)
    rc, st, _ = _raw_verify_many(zkp, ctx, vk, words, np.zeros((3, 2, 4), dtype=np.uint64), 2)
    assert rc == zkp.ZK_ERR_INVALID_WITNESS and (st == 0xAA).all()
    with pytest.raises(zkp.InvalidWitness):
        ctx.verify_many(vk, [zkp.Proof(w) for w in words], np.zeros((3, 2, 4), dtype=np.uint64))
    with pytest.raises(zkp.InvalidWitness):
        zkp.Verifier.verify_many(vk, [(zkp.Proof(words[0]), [3, 4])], ctx)
    # n_proofs = 0
    assert len(ctx.verify_many(vk, [], [])) == 0
    assert len(zkp.Verifier.verify_many(vk, [], ctx)) == 0
    # a malformed vk point: gamma or alpha off its curve; an ic entry, even one whose input is zero
    for field, word in (("gamma_g2", 12), ("alpha_g1", 6)):
        bad = zkp.VerificationKey.from_points(vk.point("alpha_g1"), vk.point("beta_g2"), vk.point("gamma_g2"),
                                              vk.point("delta_g2"), vk.ic_g1)
        getattr(bad.s, field).w[word] ^= 1
        rc, st, _ = _raw_verify_many(zkp, ctx, bad, words, inputs, 1)
        assert rc == zkp.ZK_ERR_ARG and (st == 0xAA).all()
    bad = zkp.VerificationKey.from_points(vk.point("alpha_g1"), vk.point("beta_g2"), vk.point("gamma_g2"),
                                          vk.point("delta_g2"), vk.ic_g1)
    bad.ic_g1[1][6] ^= 1
    zero_in = np.zeros((3, 1, 4), dtype=np.uint64)
    rc, st, _ = _raw_verify_many(zkp, ctx, bad, words, zero_in, 1)
    assert rc == zkp.ZK_ERR_ARG and (st == 0xAA).all()
    with pytest.raises(ValueError):
        ctx.verify_many(bad, [zkp.Proof(w) for w in words], zero_in)
    # ic_len < n_inputs + 1
    short = zkp.VerificationKey.from_points(vk.point("alpha_g1"), vk.point("beta_g2"), vk.point("gamma_g2"),
                                            vk.point("delta_g2"), vk.ic_g1)
    short.s.ic_len = 1
    rc, _, _ = _raw_verify_many(zkp, ctx, short, words, inputs, 1)
    assert rc == zkp.ZK_ERR_ARG


def test_verify_many_full_width_parameters_reject(zkp, ctx, oracle, pyref):
    """Random full-width setup parameters: lo64 truncation breaks the reference's own proof
    (test_verifier.py::test_verify_reference_toy_circuit); REJECT here as on the host."""
    rng = pyref.SplitMix64(777)
    r, s = rng.fr(), rng.fr()
    csr = oracle.CSR.from_constraints([({1: 1}, {2: 1}, {3: 1})], 4)
    rc, pk, ovk = oracle.setup(csr, [rng.fr() for _ in range(5)], 1)
    assert rc == 0
    rc, proof = oracle.prove(pk, csr, oracle.fr_array([1, 3, 4, 12]), 1, r, s)
    assert rc == 0
    vk = _vk_of(zkp, ovk)
    assert not zkp.Verifier.verify(vk, zkp.Proof(proof), [3])
    assert ctx.verify_many(vk, [zkp.Proof(proof)], [[3]]).tolist() == [zkp.ZK_VERIFY_REJECT]
    assert zkp.Verifier.verify_many(vk, [(zkp.Proof(proof), [3])], ctx).tolist() == [False]
