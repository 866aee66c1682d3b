"""Sound batch verification on the GPU (csrc/verify_all.hip):
zk_groth16_verify_all_sound and zk_groth16_verify_all_bytes_sound against
verify_all_ref.batch_equation_holds (pyref big integers and the host pairing
over the n + 3 pairs), the folds on their own through zk_test_verify_all_parts,
malformed proofs, and the return codes.

The num_public = 3 key and its two proofs are test_gpu_sound.py's
test_verify_many_sound recipe; a second key with num_public = 0 satisfies the
Groth16 equation by construction (test_gpu_verify_bytes.py's test_sound_mode
recipe), which also gives accepting proofs with the identity in them.
Coefficients come from a pool of six fixed 128-bit values (1 and 2^128 - 1
among them), so that the reference's cache of c P holds every product after the
first tests.  ZK_OPT_VERIFY_CHUNK = 64: 130 proofs are three chunks."""
import ctypes as C

import numpy as np
import pytest

import points_util as PU
import sound_ref
import verify_all_ref as VR

pytestmark = pytest.mark.gpu

R = sound_ref.R
TWO64, TWO128 = 1 << 64, 1 << 128


@pytest.fixture(autouse=True)
def chunk64(zkp, ctx):
    ctx.set_option(zkp.ZK_OPT_VERIFY_CHUNK, 64)
    yield
    ctx.set_option(zkp.ZK_OPT_VERIFY_CHUNK, 65536)


@pytest.fixture(scope="module")
def pool(pyref):
    rng = pyref.SplitMix64(0xC0EFF)
    out = [1, TWO128 - 1] + [(rng.next() << 64) | rng.next() for _ in range(4)]
    assert all(0 < c < TWO128 for c in out) and all(c >> 64 for c in out[1:]) and len(set(out)) == 6
    return out


def _coeffs(pool, n, shift=0):
    return [pool[(k + shift) % len(pool)] for k in range(n)]


@pytest.fixture(scope="module")
def main(zkp, ctx, pyref):
    """num_public = 3, full-width inputs: vk, proofs p1 p2 (words), x (3 ints), and the variants"""
    rng = pyref.SplitMix64(0x3A17)
    qap4 = zkp.QAP(zkp.CSRMatrices.synthetic(sound_ref.CASE_N))
    crs = zkp.CRS.generate_from_qap(ctx, qap4, zkp.SetupParams(*[rng.fr() for _ in range(5)]), 3, sound=True)
    z = pyref.synthetic_witness(sound_ref.CASE_N, 0x3A18)
    dpk = crs.pk.upload(ctx)
    p1 = zkp.Prover.prove(dpk, zkp.Witness(z, 3), r=rng.fr(), s=rng.fr()).words.copy()
    p2 = zkp.Prover.prove(dpk, zkp.Witness(z, 3), r=rng.fr(), s=rng.fr()).words.copy()
    dpk.free()
    x = [int(v) for v in z[1:4]]
    assert all(TWO64 <= v < R - TWO64 for v in x)
    vk = crs.vk
    assert vk.sound and zkp.Verifier.verify(vk, zkp.Proof(p1), x) and zkp.Verifier.verify(vk, zkp.Proof(p2), x)
    off = p1.copy()
    off[6] ^= np.uint64(1)                                       # A off its curve
    return {"vk": vk, "p1": p1, "p2": p2, "x": x, "off": off,
            "c_swap": np.concatenate([p1[:38], p2[38:]]),       # C of the other proof
            "c_swap2": np.concatenate([p2[:38], p1[38:]]),
            "plus": [x[0], x[1] + TWO64, x[2]],                  # limb 1 of x_1 only
            "big": [x[0], x[1], R]}


@pytest.fixture(scope="module")
def built(zkp, pyref):
    """num_public = 0: vk and make(a, b) -> the words of a proof that verifies by construction;
    a = 0 puts the identity in A, and c_zero(a) picks b so that C is the identity"""
    G1, G2, g1, g2 = pyref.G1, pyref.G2, pyref.G1.gen, pyref.G2.gen
    rng = pyref.SplitMix64(0x50D0)

    def sc():
        return (rng.next() << 16) | (rng.next() & 0xFFFF)

    al, be, ga, de, k0 = (sc() for _ in range(5))
    vk = zkp.VerificationKey.from_points(pyref.g1_words(G1.mul(g1, al)), pyref.g2_words(G2.mul(g2, be)),
                                         pyref.g2_words(G2.mul(g2, ga)), pyref.g2_words(G2.mul(g2, de)),
                                         [pyref.g1_words(G1.mul(g1, k0))], sound=True)
    rest = (al * be + k0 * ga) % R

    def make(a, b, c_shift=0):
        """c_shift: C = [c + c_shift] G, a proof off by c_shift"""
        c = ((a * b - rest) * pow(de, R - 2, R) + c_shift) % R
        return np.array(pyref.g1_words(G1.mul(g1, a)) + pyref.g2_words(G2.mul(g2, b)) + pyref.g1_words(G1.mul(g1, c)),
                        dtype=np.uint64)

    def c_zero(a):
        return make(a, rest * pow(a, R - 2, R) % R)

    def c_of(words_scalar_a, b):
        return ((words_scalar_a * b - rest) * pow(de, R - 2, R)) % R

    return {"vk": vk, "make": make, "c_zero": c_zero, "c_of": c_of, "sc": sc, "rest": rest, "de": de}


def _bytes(zkp, rows):
    return b"".join(zkp.Proof(w).serialize_compressed() for w in rows)


def _limbs(rows, npub):
    """rows of integers (or limbs already) -> (n, npub, 4) raw words: nothing is reduced"""
    if isinstance(rows, np.ndarray):
        return rows
    out = np.zeros((len(rows), npub, 4), dtype=np.uint64)
    for j, row in enumerate(rows):
        for k, v in enumerate(row):
            out[j, k] = [(v >> (64 * i)) & (TWO64 - 1) for i in range(4)]
    return out


def _both(zkp, ctx, vk, rows, inputs, coeffs):
    """(valid, first_malformed) through the struct entry and through bytes: they must agree"""
    words = np.array(rows, dtype=np.uint64).reshape(-1, 51)
    inputs = _limbs(inputs, vk.num_public)
    got = ctx.verify_all(vk, words, inputs, coeffs)
    assert ctx.verify_all_bytes(vk, _bytes(zkp, words), inputs, coeffs) == got
    return got


def _expect(zkp, pyref, vk, rows, inputs, coeffs):
    return VR.batch_equation_holds(zkp, pyref, vk, rows, inputs, coeffs)


# ------------------------------------------------- 1. verdicts ----
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130])
def test_verdict_equals_the_reference(zkp, ctx, pyref, main, pool, n):
    vk, x = main["vk"], main["x"]
    rows = [main["p1"] if k % 2 == 0 else main["p2"] for k in range(n)]
    inputs = [x] * n
    co = _coeffs(pool, n)
    want = _expect(zkp, pyref, vk, rows, inputs, co)
    assert want is True                                          # all(Verifier.verify): the fixture checked p1 and p2
    assert _both(zkp, ctx, vk, rows, inputs, co) == (True, n)
    assert zkp.Verifier.verify_all(vk, [(zkp.Proof(w), x) for w in rows], ctx, coeffs=co) is True
    if n < 130:                                                  # the 130 batches with an invalid proof: below
        rows[n // 2] = main["c_swap"]
        want = _expect(zkp, pyref, vk, rows, inputs, co)
        assert want is False
        assert _both(zkp, ctx, vk, rows, inputs, co) == (want, n)


# ---------------------------------------- 2. one invalid proof ----
@pytest.mark.parametrize("pos,kind", [(0, "c"), (63, "input"), (64, "c"), (129, "input")])
def test_one_invalid_proof_rejects(zkp, ctx, pyref, main, pool, pos, kind):
    vk, x, n = main["vk"], main["x"], 130
    rows = [main["p1"] if k % 2 == 0 else main["p2"] for k in range(n)]
    inputs = [x] * n
    if kind == "c":
        rows[pos] = main["c_swap"] if pos % 2 == 0 else main["c_swap2"]
    else:
        inputs[pos] = main["plus"]
    co = _coeffs(pool, n, shift=pos)
    want = _expect(zkp, pyref, vk, rows, inputs, co)
    assert want is False
    assert _both(zkp, ctx, vk, rows, inputs, co) == (False, n)


# ------------------------------------------------ 3. swapped pair ----
def test_swapped_pair(zkp, ctx, pyref, main, pool):
    """(A1, B1, C2) and (A2, B2, C1): the defects cancel exactly when c_1 = c_2.  Coefficients that
    differ in one limb only tell a kernel that truncates c_k from one that does not."""
    vk, x = main["vk"], main["x"]
    rows, inputs = [main["c_swap"], main["c_swap2"]], [x, x]
    base = pool[2]
    cases = [([1, 1], True), ([base, base], True), ([1, 2], False), ([base, base ^ (1 << 127)], False),
             ([base, base ^ (1 << 64)], False), ([pool[3], pool[4]], False)]
    for co, want in cases:
        assert _expect(zkp, pyref, vk, rows, inputs, co) is want, co
        assert _both(zkp, ctx, vk, rows, inputs, co) == (want, 2), co


# --------------------------------------------- 4. fold edge cases ----
def _inf_g1():
    return np.array([0] * 12 + [1], dtype=np.uint64)


def test_fold_edges_on_the_main_key(zkp, ctx, pyref, main, pool):
    vk, x, p1, p2 = main["vk"], main["x"], main["p1"], main["p2"]
    c = pool[3]
    neg_c = p2.copy()                                            # (A2, B2, -C1): S_C is the identity with p1
    neg_c[38:51] = pyref.g1_words(pyref.G1.neg(VR.g1_point(p1[38:51])))
    a_inf, c_inf = p1.copy(), p1.copy()
    a_inf[:13] = _inf_g1()
    c_inf[38:51] = _inf_g1()
    flip = [(R - v) % R for v in x]
    vk_ic = zkp.VerificationKey.from_points(vk.point("alpha_g1"), vk.point("beta_g2"), vk.point("gamma_g2"),
                                            vk.point("delta_g2"), vk.ic_g1, sound=True)
    vk_ic.ic_g1[2] = _inf_g1()
    cases = [
        ("the same proof four times, equal coefficients: the doubling case of the G1 fold",
         vk, [p1] * 4, [x] * 4, [c] * 4),
        ("S_C is the identity: inverse operands", vk, [p1, neg_c], [x, x], [c, c]),
        ("A is the identity", vk, [p1, a_inf, p2], [x] * 3, _coeffs(pool, 3)),
        ("C is the identity", vk, [p1, c_inf, p2], [x] * 3, _coeffs(pool, 3)),
        ("inputs that cancel: every t_i = 0", vk, [p1, p1], [x, flip], [c, c]),
        ("an ic_g1 entry is the identity", vk_ic, [p1, p2, p1], [x] * 3, _coeffs(pool, 3, 1)),
    ]
    seen = set()
    for what, key, rows, inputs, co in cases:
        want = _expect(zkp, pyref, key, rows, inputs, co)
        assert _both(zkp, ctx, key, rows, inputs, co) == (want, len(rows)), what
        seen.add(want)
    assert seen == {True, False}                                 # four copies of a valid proof accept


def test_fold_edges_that_accept(zkp, ctx, pyref, built, pool):
    """The num_public = 0 key: proofs valid by construction, the identity among their points."""
    vk, make, sc = built["vk"], built["make"], built["sc"]
    good = [make(sc(), sc()) for _ in range(3)]
    for w in good:
        assert zkp.Verifier.verify(vk, zkp.Proof(w), [])
    a_inf = make(0, sc())                                        # A = O: C alone carries the equation
    c_inf = built["c_zero"](sc())                                # C = O
    a1, b1 = sc(), sc()
    first = make(a1, b1)
    c1 = built["c_of"](a1, b1)
    a2 = sc()
    b2 = (built["rest"] - c1 * built["de"]) % R * pow(a2, R - 2, R) % R
    second = make(a2, b2)                                        # valid, and C2 = -C1
    assert list(second[38:50]) == pyref.g1_words(pyref.G1.neg(VR.g1_point(first[38:51])))[:12]
    c = pool[4]
    cases = [
        ("valid proofs", good * 22, _coeffs(pool, 66)),                  # 66 proofs, 6 (proof, c_k) pairs
        ("A is the identity", [good[0], a_inf, good[1]], _coeffs(pool, 3)),
        ("C is the identity", [c_inf, good[2]], _coeffs(pool, 2, 1)),
        ("S_C is the identity", [first, second], [c, c]),
        ("one proof off by G in C", good + [make(sc(), sc(), c_shift=1)], _coeffs(pool, 4)),
    ]
    for what, rows, co in cases:
        inputs = np.zeros((len(rows), 0, 4), dtype=np.uint64)
        want = _expect(zkp, pyref, vk, rows, inputs, co)
        assert want is (what != "one proof off by G in C"), what
        assert _both(zkp, ctx, vk, rows, inputs, co) == (want, len(rows)), what


# --------------------------------------------------- 5. malformed ----
def test_malformed_proofs(zkp, ctx, main, pool):
    vk, x, n = main["vk"], main["x"], 130
    rows = [main["p1"] if k % 2 == 0 else main["p2"] for k in range(n)]
    co = _coeffs(pool, n)
    with_off = list(rows)
    with_off[70] = main["off"]
    assert ctx.verify_all(vk, np.array(with_off), _limbs([x] * n, 3), co) == (False, 70)
    inputs = [x] * n
    inputs[70] = main["big"]                                     # an input = r
    assert _both(zkp, ctx, vk, rows, inputs, co) == (False, 70)
    inputs[129] = main["big"]
    with_off[3] = main["off"]
    lim = _limbs(inputs, 3)
    assert ctx.verify_all(vk, np.array(with_off), lim, co) == (False, 3)         # the lowest index
    with pytest.raises(ValueError, match="proof 3 "):
        zkp.Verifier.verify_all(vk, [(zkp.Proof(w), i) for w, i in zip(with_off, lim)], ctx, coeffs=co)
    with pytest.raises(ValueError, match="proof 70 has a public input that is not below r"):
        zkp.Verifier.verify_all_bytes(vk, [(zkp.Proof(w).serialize_compressed(), i) for w, i in zip(rows, lim)],
                                      ctx, coeffs=co)


def test_points_outside_the_subgroup_are_malformed(zkp, ctx, pyref, main, pool):
    """On-curve points outside the prime-order subgroup (points_util's, as test_gpu_verify_bytes.py
    builds its encodings) in A, in B and in C: malformed through both entries -- the struct entry
    runs the endomorphism test itself, which zk_groth16_verify_many does not."""
    vk, x, p1 = main["vk"], main["x"], main["p1"]
    off1, off2 = PU.g1_off_subgroup()[1], PU.g2_off_subgroup()[0]
    rec = zkp.Proof(p1).serialize_compressed()
    S, OK = zkp.ZK_POINT_NOT_IN_SUBGROUP, zkp.ZK_POINT_OK
    for slot in range(3):
        bad = p1.copy()
        if slot == 1:
            bad[13:38] = pyref.g2_words(off2)
            enc = rec[:48] + pyref.g2_compress(off2) + rec[144:]
        else:
            bad[(0, None, 38)[slot]:(13, None, 51)[slot]] = pyref.g1_words(off1)
            enc = pyref.g1_compress(off1) + rec[48:] if slot == 0 else rec[:144] + pyref.g1_compress(off1)
        rows = [p1, main["p2"], bad, p1]
        co = _coeffs(pool, 4, slot)
        assert ctx.verify_all(vk, np.array(rows), _limbs([x] * 4, 3), co) == (False, 2), slot
        data = rec + zkp.Proof(main["p2"]).serialize_compressed() + enc + rec
        valid, first, pst = ctx.verify_all_bytes(vk, data, _limbs([x] * 4, 3), co, point_status=True)
        assert (valid, first) == (False, 2), slot
        want = [[OK] * 3 for _ in range(4)]
        want[2][slot] = S
        assert pst.tolist() == want, slot
        with pytest.raises(ValueError, match=rf"proof 2 point {'abc'[slot]}: not in the prime-order subgroup"):
            zkp.Verifier.verify_all_bytes(vk, [(data[192 * k:192 * (k + 1)], x) for k in range(4)], ctx, coeffs=co)
    # the same four proofs without the bad one: valid
    assert ctx.verify_all(vk, np.array([p1, main["p2"], p1]), _limbs([x] * 3, 3), _coeffs(pool, 3)) == (True, 3)


# ------------------------------------------------------- 6. parts ----
def test_parts(zkp, ctx, pyref, main, pool):
    """n = 65, two chunks: each of the three folds against its own reference -- S_C against
    pyref, the scalars against the integers, and FINAL_EXP(conj(F)) word for word against the
    ZK_TEST_FQ12_MUL fold of zk_test_pairing_gt(c_k A_k, B_k), kernels that have their own tests."""
    vk, x, n = main["vk"], main["x"], 65
    rows = [main["p1"] if k % 2 == 0 else main["p2"] for k in range(n)]
    inputs = [x if k % 3 else main["plus"] for k in range(n)]
    co = _coeffs(pool, n)
    sum_c, scal, gt = ctx.test_verify_all_parts(vk, np.array(rows), _limbs(inputs, 3), co)
    ca, s_c, want_scal = VR.batch_parts(vk, rows, inputs, co)
    assert list(sum_c) == pyref.g1_words(s_c)
    assert scal == want_scal
    gts = ctx.test_pairing_gt([pyref.g1_words(p) for p in ca], [w[13:38] for w in rows])
    acc = gts[0:1]
    for k in range(1, n):
        acc = ctx.test_fq12(zkp.ZK_TEST_FQ12_MUL, acc, gts[k:k + 1])
    assert np.array_equal(gt, acc[0])


# ----------------------------------------------------- 7. returns ----
def _raw(zkp, ctx, vk, words, inputs, n_inputs, coeffs, n=None):
    """zk_groth16_verify_all_sound itself -> (rc, valid, first_malformed), both preset to 7"""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    inputs = np.ascontiguousarray(inputs, dtype=np.uint64)
    co = np.ascontiguousarray([zkp.to_limbs(c) for c in coeffs], dtype=np.uint64).reshape(-1, 4)
    n = len(co) if n is None else n
    valid, first = C.c_int(7), C.c_size_t(7)
    rc = zkp.lib().zk_groth16_verify_all_sound(
        C.c_void_p(ctx._h), C.byref(vk.s), C.c_void_p(words.ctypes.data) if words.size else None,
        C.c_void_p(inputs.ctypes.data) if inputs.size else None, C.c_size_t(n_inputs), C.c_size_t(n),
        C.c_void_p(co.ctypes.data) if co.size else None, C.byref(valid), C.byref(first))
    return rc, valid.value, first.value


def test_returns(zkp, ctx, main, pool):
    vk, x = main["vk"], main["x"]
    words = np.array([main["p1"], main["p2"], main["p1"]], dtype=np.uint64)
    inputs = np.array([[zkp.to_limbs(v) for v in x]] * 3, dtype=np.uint64)
    assert _raw(zkp, ctx, vk, words, inputs, 3, pool[:3]) == (zkp.ZK_OK, 1, 3)
    for bad in (0, TWO128):                                      # checked on the host, the index named
        rc, valid, first = _raw(zkp, ctx, vk, words, inputs, 3, [pool[0], pool[1], bad])
        assert rc == zkp.ZK_ERR_ARG and valid == 7
        assert "coefficient 2" in zkp.lib().zk_last_error(ctx._h).decode()
        with pytest.raises(ValueError, match="coefficient 2"):
            ctx.verify_all(vk, words, inputs, [pool[0], pool[1], bad])
    rc, valid, _ = _raw(zkp, ctx, vk, words, inputs[:, :2], 2, pool[:3])
    assert rc == zkp.ZK_ERR_INVALID_WITNESS and valid == 7
    with pytest.raises(zkp.InvalidWitness):
        zkp.Verifier.verify_all(vk, [(zkp.Proof(words[0]), x[:2])], ctx)
    with pytest.raises(zkp.InvalidWitness):
        zkp.Verifier.verify_all_bytes(vk, [(zkp.Proof(words[0]).serialize_compressed(), x[:2])], ctx)
    # n = 0: valid
    assert _raw(zkp, ctx, vk, np.zeros(0), np.zeros(0), 3, [], 0) == (zkp.ZK_OK, 1, 0)
    assert ctx.verify_all(vk, [], [], []) == (True, 0)
    assert ctx.verify_all_bytes(vk, b"", [], []) == (True, 0)
    assert zkp.Verifier.verify_all(vk, [], ctx) is True
    # NULL coeffs with n > 0
    valid = C.c_int(7)
    rc = zkp.lib().zk_groth16_verify_all_sound(C.c_void_p(ctx._h), C.byref(vk.s), C.c_void_p(words.ctypes.data),
                                               C.c_void_p(inputs.ctypes.data), C.c_size_t(3), C.c_size_t(3), None,
                                               C.byref(valid), None)
    assert rc == zkp.ZK_ERR_ARG and valid.value == 7
    # a malformed vk point
    bad_vk = zkp.VerificationKey.from_points(vk.point("alpha_g1"), vk.point("beta_g2"), vk.point("gamma_g2"),
                                             vk.point("delta_g2"), vk.ic_g1, sound=True)
    bad_vk.s.gamma_g2.w[12] ^= 1
    rc, valid, _ = _raw(zkp, ctx, bad_vk, words, inputs, 3, pool[:3])
    assert rc == zkp.ZK_ERR_ARG and valid == 7
    # a reference-mode vk: refused in Python, and BatchVerifier keeps refusing the sound one
    ref_vk = zkp.VerificationKey.from_points(vk.point("alpha_g1"), vk.point("beta_g2"), vk.point("gamma_g2"),
                                             vk.point("delta_g2"), vk.ic_g1, sound=False)
    with pytest.raises(ValueError, match="sound"):
        zkp.Verifier.verify_all(ref_vk, [(zkp.Proof(words[0]), x)], ctx)
    with pytest.raises(ValueError, match="sound"):
        zkp.Verifier.verify_all_bytes(ref_vk, [(zkp.Proof(words[0]).serialize_compressed(), x)], ctx)
    with pytest.raises(ValueError, match="verify_all"):
        zkp.BatchVerifier.verify_batch(vk, [(zkp.Proof(words[0]), x)], coeffs=[1])


def test_drawn_coefficients(zkp, ctx, main):
    """coeffs=None: fresh 128-bit coefficients from `secrets` per call"""
    vk, x = main["vk"], main["x"]
    good = [(zkp.Proof(main["p1"] if k % 2 else main["p2"]), x) for k in range(5)]
    assert zkp.Verifier.verify_all(vk, good, ctx) is True
    assert zkp.Verifier.verify_all_bytes(vk, [(p.serialize_compressed(), i) for p, i in good], ctx) is True
    bad = list(good)
    bad[3] = (zkp.Proof(main["c_swap"]), x)
    assert zkp.Verifier.verify_all(vk, bad, ctx) is False       # one invalid proof: every non-zero c_k rejects
    assert zkp.Verifier.verify_all_bytes(vk, [(p.serialize_compressed(), i) for p, i in bad], ctx) is False
