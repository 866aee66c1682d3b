"""GPU verification from proof bytes (csrc/points.hip's proof decoder in front
of csrc/pairing.hip's verify kernel): zk_proofs_deserialize_compressed against
the host decoder record by record, the decoder's endomorphism subgroup test
against the [r]P test of zk_g1/g2_decompress, and zk_groth16_verify_many_bytes
(_sound) against "host decode, then host verify" proof by proof.

Everything is built once per module with pyref / points_util and the oracle's
prover; every call runs at most 130 lanes with ZK_OPT_VERIFY_CHUNK = 64, so
130 proofs cross the GPU in three launches."""
import ctypes as C

import numpy as np
import pytest

import points_util as PU

pytestmark = pytest.mark.gpu

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
M64 = (1 << 64) - 1
TOY_XY = [(3, 4), (0, 5), (1, 1), (2, 7), (5, 5), (6, 2), (9, 3), (4, 11)]
G1_INF_ENC = bytes([0xC0]) + bytes(47)
G2_INF_ENC = bytes([0xC0]) + bytes(95)
SENTINEL = 0xAA


@pytest.fixture(autouse=True)
def chunk64(zkp, ctx):
    ctx.set_option(zkp.ZK_OPT_VERIFY_CHUNK, 64)
    yield
    ctx.set_option(zkp.ZK_OPT_VERIFY_CHUNK, 65536)


def _record(a, b, c):
    assert len(a) == 48 and len(b) == 96 and len(c) == 48
    return a + b + c


def _host_decode(zkp, rec):
    """the host decoder on one 192-byte record: its 51 words, or None where it refuses"""
    try:
        return np.array(zkp.Proof.deserialize_compressed(rec).words, dtype=np.uint64)
    except ValueError:
        return None


def _limbs(inputs, npub):
    """rows of integers -> (n, npub, 4) raw words (nothing is reduced)"""
    out = np.zeros((len(inputs), npub, 4), dtype=np.uint64)
    for j, row in enumerate(inputs):
        for k, v in enumerate(row):
            out[j, k] = [(v >> (64 * i)) & M64 for i in range(4)]
    return out


def _host_status(zkp, vk, rec, inp_words):
    """host decode refuses -> MALFORMED, else Verifier.verify (a ValueError of it: MALFORMED)"""
    words = _host_decode(zkp, rec)
    if words is None:
        return zkp.ZK_VERIFY_MALFORMED
    try:
        ok = zkp.Verifier.verify(vk, zkp.Proof(words), inp_words)
    except ValueError:
        return zkp.ZK_VERIFY_MALFORMED
    return zkp.ZK_VERIFY_ACCEPT if ok else zkp.ZK_VERIFY_REJECT


def _raw_deserialize(zkp, ctx, data, n, with_pst=True):
    """zk_proofs_deserialize_compressed with buffers one element longer than n"""
    buf = np.frombuffer(data, dtype=np.uint8)
    out = np.full((n + 1, 51), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    pst = np.full(3 * n + 1, SENTINEL, dtype=np.uint8)
    rc = zkp.lib().zk_proofs_deserialize_compressed(C.c_void_p(ctx._h), C.c_void_p(buf.ctypes.data), C.c_size_t(n),
                                                    C.c_void_p(out.ctypes.data),
                                                    C.c_void_p(pst.ctypes.data) if with_pst else None)
    assert (out[n] == 0xA5A5A5A5A5A5A5A5).all() and pst[3 * n] == SENTINEL
    return rc, out[:n], pst[:3 * n].reshape(n, 3)


def _raw_verify(zkp, ctx, vk, data, inputs, n_inputs, sound=False, with_pst=True, null_proofs=False):
    """zk_groth16_verify_many_bytes(_sound) with status buffers one byte longer than needed:
    (rc, statuses, point statuses); the sentinel bytes must survive"""
    n = len(inputs)
    buf = np.frombuffer(data, dtype=np.uint8)
    st = np.full(n + 1, SENTINEL, dtype=np.uint8)
    pst = np.full(3 * n + 1, SENTINEL, dtype=np.uint8)
    fn = zkp.lib().zk_groth16_verify_many_bytes_sound if sound else zkp.lib().zk_groth16_verify_many_bytes
    rc = fn(C.c_void_p(ctx._h), C.byref(vk.s), None if null_proofs else C.c_void_p(buf.ctypes.data),
            C.c_void_p(inputs.ctypes.data) if inputs.size else None, C.c_size_t(n_inputs), C.c_size_t(n),
            C.c_void_p(st.ctypes.data), C.c_void_p(pst.ctypes.data) if with_pst else None)
    assert st[n] == SENTINEL and pst[3 * n] == SENTINEL
    return rc, st[:n], pst[:3 * n].reshape(n, 3)


# ------------------------------------------------------------ fixtures ----
@pytest.fixture(scope="module")
def toy(zkp, oracle, pyref):
    """test_gpu_pairing.py's toy recipe, built again: x*y=z (x public) set up with [2,3,1,1,5],
    8 valid proofs from the oracle's prover -> (vk, [(192 bytes, words, x)])"""
    csr = oracle.CSR.from_constraints([({1: 1}, {2: 1}, {3: 1})], 4)
    rc, pk, ovk = oracle.setup(csr, [2, 3, 1, 1, 5], 1)
    assert rc == 0
    vk = zkp.VerificationKey.from_points(ovk.field("alpha_g1"), ovk.field("beta_g2"), ovk.field("gamma_g2"),
                                         ovk.field("delta_g2"), ovk.ic_g1)
    rng = pyref.SplitMix64(4242)
    proofs = []
    for x, y in TOY_XY:
        rc, pr = oracle.prove(pk, csr, oracle.fr_array([1, x, y, x * y]), 1, rng.fr(), rng.fr())
        assert rc == 0
        words = np.array(pr, dtype=np.uint64)
        rec = zkp.Proof(words).serialize_compressed()
        assert zkp.Verifier.verify(vk, zkp.Proof(words), [x])
        proofs.append((rec, words, x))
    return vk, proofs


@pytest.fixture(scope="module")
def decode_cases(zkp, toy):
    """[(record, slot or None, expected status of that slot)]: the 8 valid records, every invalid
    encoding of points_util in slot a, in slot c (G1) and in slot b (G2), the identity in each slot"""
    _, proofs = toy
    cases = [(rec, None, PU.ST_OK) for rec, _, _ in proofs]
    k = 0
    for slot in (0, 2):
        for enc, want in PU.invalid_g1():
            rec = proofs[k % 8][0]
            k += 1
            cases.append((enc + rec[48:] if slot == 0 else rec[:144] + enc, slot, want))
    for enc, want in PU.invalid_g2():
        rec = proofs[k % 8][0]
        k += 1
        cases.append((rec[:48] + enc + rec[144:], 1, want))
    rec = proofs[0][0]
    cases += [(G1_INF_ENC + rec[48:], 0, PU.ST_OK), (rec[:48] + G2_INF_ENC + rec[144:], 1, PU.ST_OK),
              (rec[:144] + G1_INF_ENC, 2, PU.ST_OK)]
    return cases


# ------------------------------------------- 1. decode equals the host ----
SLOT_WORDS = (slice(0, 13), slice(13, 38), slice(38, 51))


def test_decode_equals_the_host_decoder(zkp, ctx, toy, decode_cases):
    _, proofs = toy
    n = len(decode_cases)
    assert 64 < n <= 130        # a second launch
    data = b"".join(rec for rec, _, _ in decode_cases)
    rc, words, pst = _raw_deserialize(zkp, ctx, data, n)
    assert rc == zkp.ZK_ERR_ARG
    first = next(j for j, (_, _, want) in enumerate(decode_cases) if want != PU.ST_OK)
    slot, want = decode_cases[first][1:]
    msg = zkp.lib().zk_last_error(ctx._h).decode()
    assert f"proof {first} point {'abc'[slot]}: {zkp.POINT_STATUS_TEXT[want]}" in msg
    for j, (rec, slot, want) in enumerate(decode_cases):
        host = _host_decode(zkp, rec)
        if want == PU.ST_OK:
            assert host is not None and np.array_equal(words[j], host), j
            assert (pst[j] == zkp.ZK_POINT_OK).all(), j
            if slot is not None:        # the identity: zero coordinates, the infinity byte set
                w = words[j][SLOT_WORDS[slot]]
                assert w[-1] == 1 and not w[:-1].any()
            continue
        assert host is None, j          # the host decoder refuses the record
        for s in range(3):
            if s == slot:
                assert pst[j][s] == want and not words[j][SLOT_WORDS[s]].any(), (j, s)
            else:               # the other two points: valid, their words intact
                assert pst[j][s] == zkp.ZK_POINT_OK, (j, s)
                assert np.array_equal(words[j][SLOT_WORDS[s]], _untouched(zkp, rec, s)), (j, s)
    # the 8 valid records alone: ZK_OK, with and without the status buffer; the Python layer agrees
    good = b"".join(rec for rec, _, _ in proofs)
    for with_pst in (True, False):
        rc, w8, p8 = _raw_deserialize(zkp, ctx, good, 8, with_pst)
        assert rc == zkp.ZK_OK and np.array_equal(w8, np.array([w for _, w, _ in proofs]))
        assert (p8 == (zkp.ZK_POINT_OK if with_pst else SENTINEL)).all()
    pw, pp = ctx.proofs_deserialize(data)
    assert np.array_equal(pw, words) and np.array_equal(pp, pst)
    pw, pp = ctx.proofs_deserialize(np.frombuffer(data, dtype=np.uint8).reshape(n, 192))
    assert np.array_equal(pw, words) and np.array_equal(pp, pst)
    assert ctx.proofs_deserialize(b"")[0].shape == (0, 51)
    with pytest.raises(ValueError):
        ctx.proofs_deserialize(data[:-1])


_VALID_CACHE = {}


def _untouched(zkp, rec, s):
    """the host decoder's words of slot s of a record (decoded between two generator points,
    points_util.host_decode), cached per encoding"""
    enc = (rec[:48], rec[48:144], rec[144:])[s]
    if enc not in _VALID_CACHE:
        _VALID_CACHE[enc] = PU.host_decode(zkp, enc)
    return _VALID_CACHE[enc]


# --------------------------- 2. the new subgroup test agrees with [r]P ----
@pytest.fixture(scope="module")
def subgroup_encodings(pyref):
    """64 G1 and 64 G2 encodings of points ON their curves: 32 from the subgroup walks, 32 outside
    (consecutive small x, a few [r]Q, a few G + T with T of order 3 (G1) / T = [r]Q (G2))"""
    G1, G2 = pyref.G1, pyref.G2
    off1, x = [], 4
    while len(off1) < 24:
        pt = PU.on_curve_g1(x)
        if pt is not None:
            off1.append(pt)
        x += 1
    t3 = (pyref.Fq1(0), pyref.Fq1(2))
    off1 += [G1.mul(q, R) for q in off1[:4]] + [G1.add(g, t3) for g in PU.g1_points(4, 0x1234)]
    off2, c = [], 0
    while len(off2) < 24:
        pt = PU.on_curve_g2(c // 2, 1 + c % 2)
        if pt is not None:
            off2.append(pt)
        c += 1
    rq = [G2.mul(q, R) for q in off2[:4]]
    off2 += rq + [G2.add(g, t) for g, t in zip(PU.g2_points(4, 0x4321), rq)]
    on1, on2 = PU.g1_points(32, 0x7777), PU.g2_points(32, 0x5555)
    e1 = [pyref.g1_compress(p) for pair in zip(on1, off1) for p in pair]
    e2 = [pyref.g2_compress(p) for pair in zip(on2, off2) for p in pair]
    assert len(e1) == len(e2) == 64 and len(set(e1)) == len(set(e2)) == 64
    return e1, e2


def test_endomorphism_subgroup_test_agrees_with_r_times_p(zkp, ctx, subgroup_encodings):
    e1, e2 = subgroup_encodings
    _, want1 = ctx.g1_decompress(b"".join(e1))
    _, want2 = ctx.g2_decompress(b"".join(e2))
    for want in (want1, want2):       # both verdicts occur in both groups, and nothing else
        assert set(want.tolist()) == {zkp.ZK_POINT_OK, zkp.ZK_POINT_NOT_IN_SUBGROUP}
    # record k: a = G1 encoding k, c = G1 encoding 63 - k (the other parity), b = G2 encoding k
    data = b"".join(_record(e1[k], e2[k], e1[63 - k]) for k in range(64))
    rc, words, pst = _raw_deserialize(zkp, ctx, data, 64)
    assert rc == zkp.ZK_ERR_ARG
    assert np.array_equal(pst[:, 0], want1)
    assert np.array_equal(pst[:, 2], want1[::-1])
    assert np.array_equal(pst[:, 1], want2)
    # and the words are zk_g1/g2_decompress's
    w1, _ = ctx.g1_decompress(b"".join(e1))
    w2, _ = ctx.g2_decompress(b"".join(e2))
    assert np.array_equal(words[:, :13], w1) and np.array_equal(words[:, 38:], w1[::-1])
    assert np.array_equal(words[:, 13:38], w2)


# ------------------------------------------ 3. verdicts equal the host ----
@pytest.fixture(scope="module")
def pool(zkp, toy, decode_cases):
    """(record, inputs, host status): 8 ACCEPT, 3 REJECT (another proof's A, another proof's C, a
    wrong input), 3 MALFORMED (records of the decode cases: a off the subgroup, b not canonical,
    c with bad flags)"""
    vk, proofs = toy
    A, RJ, MF = zkp.ZK_VERIFY_ACCEPT, zkp.ZK_VERIFY_REJECT, zkp.ZK_VERIFY_MALFORMED
    out = [(rec, [x], A) for rec, _, x in proofs]
    r0, r1 = proofs[0][0], proofs[1][0]
    out += [(r1[:48] + r0[48:], [3], RJ), (r0[:144] + r1[144:], [3], RJ), (r0, [5], RJ)]
    for slot, status in ((0, PU.ST_SUBGROUP), (1, PU.ST_RANGE), (2, PU.ST_ENCODING)):
        rec = next(r for r, s, w in decode_cases if s == slot and w == status)
        out.append((rec, [TOY_XY[0][0]], MF))
    full = []
    for rec, inp, want in out:
        host = _host_status(zkp, vk, rec, _limbs([inp], 1)[0])
        assert host == want
        full.append((rec, inp, host))
    return full


@pytest.mark.parametrize("n,shift", [(1, 0), (63, 0), (64, 5), (65, 0), (130, 9)])
def test_verdicts_equal_the_host(zkp, ctx, toy, pool, n, shift):
    vk, _ = toy
    pick = [pool[(j + shift) % len(pool)] for j in range(n)]
    data = b"".join(rec for rec, _, _ in pick)
    inputs = _limbs([inp for _, inp, _ in pick], 1)
    want = np.array([h for _, _, h in pick], dtype=np.uint8)
    rc, st, pst = _raw_verify(zkp, ctx, vk, data, inputs, 1)
    assert rc == zkp.ZK_OK
    assert np.array_equal(st, want)
    assert np.array_equal(pst.any(axis=1), want == zkp.ZK_VERIFY_MALFORMED)
    if n >= 16:
        assert {zkp.ZK_VERIFY_ACCEPT, zkp.ZK_VERIFY_REJECT, zkp.ZK_VERIFY_MALFORMED} == set(st.tolist())
    rc, again, pst_again = _raw_verify(zkp, ctx, vk, data, inputs, 1)
    assert rc == zkp.ZK_OK and again.tobytes() == st.tobytes() and pst_again.tobytes() == pst.tobytes()
    # the Python layers: statuses (with and without the point statuses), then bools or the first malformed index
    assert np.array_equal(ctx.verify_many_bytes(vk, data, inputs), want)
    st2, pst2 = ctx.verify_many_bytes(vk, np.frombuffer(data, dtype=np.uint8).reshape(n, 192), inputs,
                                      point_status=True)
    assert np.array_equal(st2, want) and np.array_equal(pst2, pst)
    pairs = [(rec, inp) for rec, inp, _ in pick]
    bad = np.flatnonzero(want == zkp.ZK_VERIFY_MALFORMED)
    if len(bad):
        k = int(bad[0])
        slot = int(np.flatnonzero(pst[k])[0])
        text = zkp.POINT_STATUS_TEXT[pst[k][slot]]
        with pytest.raises(ValueError, match=rf"proof {k} point {'abc'[slot]}: {text}"):
            zkp.Verifier.verify_many_bytes(vk, pairs, ctx)
    else:
        got = zkp.Verifier.verify_many_bytes(vk, pairs, ctx)
        assert got.dtype == np.bool_ and np.array_equal(got, want == zkp.ZK_VERIFY_ACCEPT)


# ------------------------------------------------ 4. the gap this closes ----
def test_points_outside_the_subgroup_are_malformed(zkp, ctx, toy, pyref):
    """An accepting proof with A replaced by a point of E(Fq) outside G1, and one with B replaced
    by a point of the twist outside G2: MALFORMED here, with the slot named; zk_groth16_verify_many
    on the same points as words has no subgroup check and only promises 0 or 1."""
    vk, proofs = toy
    rec, words, x = proofs[2]
    off1, off2 = PU.g1_off_subgroup()[1], PU.g2_off_subgroup()[0]
    recs = [pyref.g1_compress(off1) + rec[48:], rec[:48] + pyref.g2_compress(off2) + rec[144:], rec]
    inputs = _limbs([[x]] * 3, 1)
    rc, st, pst = _raw_verify(zkp, ctx, vk, b"".join(recs), inputs, 1)
    assert rc == zkp.ZK_OK
    assert st.tolist() == [zkp.ZK_VERIFY_MALFORMED, zkp.ZK_VERIFY_MALFORMED, zkp.ZK_VERIFY_ACCEPT]
    S, OK = zkp.ZK_POINT_NOT_IN_SUBGROUP, zkp.ZK_POINT_OK
    assert pst.tolist() == [[S, OK, OK], [OK, S, OK], [OK, OK, OK]]
    as_words = np.array([words, words], dtype=np.uint64)
    as_words[0][:13] = pyref.g1_words(off1)
    as_words[1][13:38] = pyref.g2_words(off2)
    unchecked = ctx.verify_many(vk, as_words, inputs[:2])
    assert set(unchecked.tolist()) <= {zkp.ZK_VERIFY_REJECT, zkp.ZK_VERIFY_ACCEPT}


# --------------------------------------------------------- 5. sound mode ----
def test_sound_mode(zkp, ctx, pyref):
    """A key and a proof satisfying the Groth16 equation by construction (test_gpu_pairing.py's
    _constructed) with FULL-WIDTH public inputs under the sound IC = ic_0 + sum x_k ic_(k+1)."""
    G1, G2, g1, g2 = pyref.G1, pyref.G2, pyref.G1.gen, pyref.G2.gen
    rng = pyref.SplitMix64(0x50D)
    npub = 2

    def sc():
        return (rng.next() << 16) | (rng.next() & 0xFFFF)

    al, be, ga, de, a, b = (sc() for _ in range(6))
    ks = [sc() for _ in range(npub + 1)]
    x = [rng.fr() for _ in range(npub)]
    assert all(v >> 192 for v in x)
    ic = (ks[0] + sum(xi * k for xi, k in zip(x, ks[1:]))) % R
    c = (a * b - al * be - ic * ga) * pow(de, R - 2, R) % R

    def w1(p):
        return np.array(pyref.g1_words(p), dtype=np.uint64)

    def w2(p):
        return np.array(pyref.g2_words(p), dtype=np.uint64)

    vk = zkp.VerificationKey.from_points(w1(G1.mul(g1, al)), w2(G2.mul(g2, be)), w2(G2.mul(g2, ga)),
                                         w2(G2.mul(g2, de)), [w1(G1.mul(g1, k)) for k in ks], sound=True)
    rec = _record(pyref.g1_compress(G1.mul(g1, a)), pyref.g2_compress(G2.mul(g2, b)), pyref.g1_compress(G1.mul(g1, c)))
    rows = [x, [(x[0] + 1) % R, x[1]], [x[0], R]]
    want = [zkp.ZK_VERIFY_ACCEPT, zkp.ZK_VERIFY_REJECT, zkp.ZK_VERIFY_MALFORMED]
    inputs = _limbs(rows, npub)
    host = [_host_status(zkp, vk, rec, inputs[j]) for j in range(3)]     # zk_groth16_verify_sound
    assert host == want
    pick = [j % 3 for j in range(65)]
    rc, st, pst = _raw_verify(zkp, ctx, vk, rec * 65, np.ascontiguousarray(inputs[pick]), npub, sound=True)
    assert rc == zkp.ZK_OK
    assert st.tolist() == [want[j] for j in pick]
    assert not pst.any()        # an input >= r: MALFORMED with every point valid
    got, _ = ctx.verify_many_bytes(vk, rec * 3, inputs, sound=True, point_status=True)
    assert got.tolist() == want
    assert zkp.Verifier.verify_many_bytes(vk, [(rec, rows[0]), (rec, rows[1])], ctx).tolist() == [True, False]
    # the reference mode on the same bytes looks at lo64 only: its own entry point, another verdict path
    rc, lo, _ = _raw_verify(zkp, ctx, vk, rec * 3, inputs, npub, sound=False)
    assert rc == zkp.ZK_OK and zkp.ZK_VERIFY_MALFORMED not in lo.tolist()


# ------------------------------------------------------------ 6. returns ----
def test_returns(zkp, ctx, toy):
    vk, proofs = toy
    data = b"".join(rec for rec, _, _ in proofs[:3])
    inputs = _limbs([[x] for _, _, x in proofs[:3]], 1)
    # n_inputs != vk.num_public: nothing is written
    rc, st, pst = _raw_verify(zkp, ctx, vk, data, np.zeros((3, 2, 4), dtype=np.uint64), 2)
    assert rc == zkp.ZK_ERR_INVALID_WITNESS and (st == SENTINEL).all() and (pst == SENTINEL).all()
    with pytest.raises(zkp.InvalidWitness):
        ctx.verify_many_bytes(vk, data, np.zeros((3, 2, 4), dtype=np.uint64))
    with pytest.raises(zkp.InvalidWitness):
        zkp.Verifier.verify_many_bytes(vk, [(proofs[0][0], [3, 4])], ctx)
    # a malformed vk point
    bad = zkp.VerificationKey.from_points(vk.point("alpha_g1"), vk.point("beta_g2"), vk.point("gamma_g2"),
                                          vk.point("delta_g2"), vk.ic_g1)
    bad.s.gamma_g2.w[12] ^= 1
    rc, st, pst = _raw_verify(zkp, ctx, bad, data, inputs, 1)
    assert rc == zkp.ZK_ERR_ARG and (st == SENTINEL).all() and (pst == SENTINEL).all()
    with pytest.raises(ValueError):
        ctx.verify_many_bytes(bad, data, inputs)
    # n = 0
    rc, st, _ = _raw_verify(zkp, ctx, vk, b"", np.zeros((0, 1, 4), dtype=np.uint64), 1)
    assert rc == zkp.ZK_OK and len(st) == 0
    assert len(ctx.verify_many_bytes(vk, b"", [])) == 0
    assert len(zkp.Verifier.verify_many_bytes(vk, [], ctx)) == 0
    rc, _, _ = _raw_deserialize(zkp, ctx, b"", 0)
    assert rc == zkp.ZK_OK
    # NULL point_status is accepted
    rc, st, pst = _raw_verify(zkp, ctx, vk, data, inputs, 1, with_pst=False)
    assert rc == zkp.ZK_OK and (st == zkp.ZK_VERIFY_ACCEPT).all() and (pst == SENTINEL).all()
    # NULL proofs with n > 0
    rc, st, _ = _raw_verify(zkp, ctx, vk, data, inputs, 1, null_proofs=True)
    assert rc == zkp.ZK_ERR_ARG and (st == SENTINEL).all()
    rc = zkp.lib().zk_proofs_deserialize_compressed(C.c_void_p(ctx._h), None, C.c_size_t(1), None, None)
    assert rc == zkp.ZK_ERR_ARG
