"""Prepared verification keys on the GPU (csrc/prepared.hip): the public-input
sums from the device window table against points made from Python integers,
the verdicts of the prepared calls against the plain calls and the host
verifier, and the errors.

Keys are constructed as test_gpu_pairing.py's _constructed does: every point is
a known multiple of a generator, ic[k] = [e_k]G with short e_k, so the expected
sum is [(e_0 + sum x_k e_k) mod r]G -- one pyref multiplication per distinct row.
"""
import ctypes as C

import numpy as np
import pytest

import points_util as PU
from test_prepared_host import plan

pytestmark = pytest.mark.gpu

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
M64 = (1 << 64) - 1
AL, BE, GA, DE, PA, PB = 0x2B5F1, 0x31C07, 0x1D2E9, 0x3A46B, 0x27D35, 0x35E8F   # short scalars of the fixed points
_G1, _G2 = {}, {}


def ek(k):
    """the short scalar of ic[k]: 20 bits, odd, different for every k"""
    return ((k * 0x9E3779B1 + 0x7F4A7C15) >> 7) % (1 << 19) * 2 + 1


def g1pt(pyref, e):
    """[e]G, through the negative where that is the short multiplication"""
    e %= R
    if e not in _G1:
        G1 = pyref.G1
        if e == 0:
            _G1[e] = None
        elif R - e < (1 << 64):
            _G1[e] = G1.neg(G1.mul(G1.gen, R - e))
        else:
            _G1[e] = G1.mul(G1.gen, e)
    return _G1[e]


def g2pt(pyref, e):
    if e not in _G2:
        _G2[e] = pyref.G2.mul(pyref.G2.gen, e)
    return _G2[e]


def g1w(pyref, e):
    return np.array(pyref.g1_words(g1pt(pyref, e)), dtype=np.uint64)


def make_key(zkp, pyref, es, sound):
    """the key with ic[k] = [es[k]]G (an identity entry for 0) and alpha .. delta = [AL]G1, [BE]G2, [GA]G2, [DE]G2"""
    g2w = lambda e: np.array(pyref.g2_words(g2pt(pyref, e)), dtype=np.uint64)
    return zkp.VerificationKey.from_points(g1w(pyref, AL), g2w(BE), g2w(GA), g2w(DE), [g1w(pyref, e) for e in es],
                                           sound=sound)


def make_proof(pyref, es, row, sound):
    """a proof that satisfies the Groth16 equation for this row of inputs, by construction"""
    ic = (es[0] + sum((x if sound else x & M64) * e for x, e in zip(row, es[1:]))) % R
    c = (PA * PB - AL * BE - ic * GA) * pow(DE, R - 2, R) % R
    return np.concatenate([g1w(pyref, PA), np.array(pyref.g2_words(g2pt(pyref, PB)), dtype=np.uint64), g1w(pyref, c)])


def limbs(rows, npub):
    a = np.zeros((len(rows), npub, 4), dtype=np.uint64)
    for j, row in enumerate(rows):
        for k, v in enumerate(row):
            a[j, k] = [(v >> (64 * i)) & M64 for i in range(4)]   # raw words: nothing is reduced
    return a


def expected(pyref, es, row, sound):
    """(13 words of IC, ok) from Python integers"""
    if sound and any(x >= R for x in row):
        return np.zeros(13, dtype=np.uint64), 0
    s = (es[0] + sum((x if sound else x & M64) * e for x, e in zip(row, es[1:]))) % R
    return g1w(pyref, s), 1


@pytest.fixture()
def chunk64(zkp, ctx):
    ctx.set_option(zkp.ZK_OPT_VERIFY_CHUNK, 64)
    yield
    ctx.set_option(zkp.ZK_OPT_VERIFY_CHUNK, 65536)


@pytest.fixture()
def force(ctx):
    yield ctx.test_prepared_force
    ctx.test_prepared_force(0, 0)


def check_sums(ctx, pvk, pyref, es, rows, sound, ns):
    """prepare_inputs on the rows tiled to every n of ns: word for word the expected points, and
    the same bytes when the call is repeated"""
    npub = len(es) - 1
    want = [expected(pyref, es, row, sound) for row in rows]
    for n in ns:
        pick = [j % len(rows) for j in range(n)]
        inp = limbs([rows[j] for j in pick], npub)
        ic, ok = pvk.prepare_inputs(inp)
        assert ok.tolist() == [want[j][1] for j in pick]
        bad = [j for j in range(n) if not np.array_equal(ic[j], want[pick[j]][0])]
        assert not bad, (n, bad[:4])
        ic2, ok2 = ctx.prepare_inputs(pvk, inp)
        assert ic2.tobytes() == ic.tobytes() and ok2.tobytes() == ok.tobytes()


# ------------------------------------------------------------- sums ----
def sum_rows(pyref, npub, sound):
    """at most 16 distinct rows: random ones and the rows that aim at the digits"""
    if npub == 0:
        return [[]]
    rng = pyref.SplitMix64(0x1C + npub)
    wide = lambda: sum(rng.next() << (64 * i) for i in range(4))
    rows = [[rng.fr() if sound else wide() for _ in range(npub)] for _ in range(5)]
    rows.append([0] * npub)                                                   # nothing but ic[0]
    rows.append([R - 1] * npub)                                               # every digit of r - 1 (or of its lo64)
    rows.append([(0x73 << 248) if sound else (0xFF << 56)] * npub)            # the top digit alone
    rows.append([(5 << 64) | (7 << 192)] * npub)                              # high limbs, lo64 = 0
    rows.append([R] + [rng.next() for _ in range(npub - 1)])                  # an input equal to r
    rows.append([rng.next() for _ in range(npub - 1)] + [(1 << 256) - 1])     # and one of 2^256 - 1
    return rows


@pytest.mark.parametrize("sound", [False, True])
@pytest.mark.parametrize("npub", [0, 1, 2, 33, 64, 65, 130])
def test_sums_equal_the_points_from_integers(zkp, ctx, pyref, chunk64, force, npub, sound):
    es = [ek(k) for k in range(npub + 1)]
    vk = make_key(zkp, pyref, es, sound)
    rows = sum_rows(pyref, npub, sound)
    if npub:
        oks = [expected(pyref, es, row, sound)[1] for row in rows]
        assert oks.count(0) == (2 if sound else 0)
        # high limbs with lo64 = 0: reference mode skips them, sound mode counts them
        skipped = np.array_equal(expected(pyref, es, rows[8], sound)[0], g1w(pyref, es[0]))
        assert skipped == (not sound)
    for width in (8, 4):
        force(width, 0)
        pvk = vk.prepare(ctx)
        assert pvk.sound == sound and pvk.num_public == npub
        b, W, _, dev_bytes, _ = plan(zkp, sound, npub, width)
        assert pvk.test_info() == (b, W) == (width, -(-(255 if sound else 64) // width))
        assert pvk.device_bytes() == dev_bytes
        for run in (0, 7):
            force(width, run)
            check_sums(ctx, pvk, pyref, es, rows, sound, (1, 2, 63, 65, 130))
        pvk.free()
    # the width the library chooses by itself
    force(0, 0)
    pvk = vk.prepare(ctx)
    assert pvk.test_info()[0] == plan(zkp, sound, npub)[0] == 8 and pvk.device_bytes() == plan(zkp, sound, npub)[3]
    check_sums(ctx, pvk, pyref, es, rows[:3], sound, (3,))
    pvk.free()


# --------------------------------------- rows that aim at the formulas ----
def formula_cases(pyref):
    """(name, es, rows): keys whose sums meet the special cases of the addition"""
    e1, e2, e3, d = ek(1), ek(2), ek(3), 5
    rng = pyref.SplitMix64(0xF0)
    x2, x3 = rng.next(), rng.next()
    return [
        ("identity entry", [ek(0), e1, 0, e3], [[x2, x3, 9], [0, 7, 0], [3, R - 1, R - 2]]),
        ("first addition doubles", [d * e1, e1, e2], [[d, x2], [d, 0]]),              # ic[0] = [d] ic[1], x_1 = d
        ("identity mid-run", [-d * e1, e1, e2, e3], [[d, x2, x3], [d, 0, 0], [d, 0, 1]]),   # ic[0] = -[d] ic[1]
        ("the sum cancels", [-d * e1, e1], [[d]]),
        ("the sum cancels late", [-(d * e1 + 9 * e2), e1, e2], [[d, 9]]),
        ("equal entries", [ek(0), e1, e1], [[x2, x2], [1, 1], [d, d]]),
        ("opposite entries", [ek(0), e1, -e1], [[x2, x2], [1, 1]]),                  # an entry meets its negative
    ]


@pytest.mark.parametrize("sound", [False, True])
def test_sums_through_the_special_cases(zkp, ctx, pyref, chunk64, force, sound):
    for name, es, rows in formula_cases(pyref):
        es = [e % R for e in es]
        vk = make_key(zkp, pyref, es, sound)
        for width in (8, 4):
            force(width, 0)
            pvk = vk.prepare(ctx)
            for run in (0, 1, 7):     # 1: every addition is the second level's
                force(width, run)
                check_sums(ctx, pvk, pyref, es, rows, sound, (1, 65))
            pvk.free()
        if "cancels" in name:
            want, ok = expected(pyref, es, rows[0], sound)
            assert ok == 1 and want[12] == 1 and not want[:12].any()       # the ABI's identity


# --------------------------------------------------------- verdicts ----
def _host_status(zkp, vk, words, inputs):
    try:   # the inputs as raw words: an int would be reduced mod r on the way in
        ok = zkp.Verifier.verify(vk, zkp.Proof(words), limbs([inputs], len(inputs))[0])
    except ValueError:
        return zkp.ZK_VERIFY_MALFORMED
    return zkp.ZK_VERIFY_ACCEPT if ok else zkp.ZK_VERIFY_REJECT


def verdict_pool(zkp, pyref, es, row, sound):
    """(words, inputs, status by construction): a valid proof, a wrong A, one input off by one, a
    malformed point; sound: an input that is not below r"""
    A, RJ, MF = zkp.ZK_VERIFY_ACCEPT, zkp.ZK_VERIFY_REJECT, zkp.ZK_VERIFY_MALFORMED
    words = make_proof(pyref, es, row, sound)
    t = words.copy(); t[:13] = g1w(pyref, 1)
    u = words.copy(); u[38 + 6] ^= 1
    pool = [(words, row, A), (t, row, RJ), (u, row, MF)]
    if row:
        pool.append((words, [(row[0] + 1) % (1 << 64)] + row[1:], RJ))
        pool.append((words, [x + (5 << 64) for x in row], RJ if sound else A))       # high limbs: sound counts them
        if sound:
            pool.append((words, row[:-1] + [R], MF))
            pool.append((words, row[:-1] + [row[-1] + R], MF))
    return pool


@pytest.mark.parametrize("sound", [False, True])
@pytest.mark.parametrize("npub", [0, 3, 65])
def test_verdicts_equal_the_plain_calls_and_the_host(zkp, ctx, pyref, chunk64, npub, sound):
    es = [ek(k) for k in range(npub + 1)]
    vk = make_key(zkp, pyref, es, sound)
    rng = pyref.SplitMix64(0xBD + npub)
    row = [rng.next() for _ in range(npub)]
    pool = verdict_pool(zkp, pyref, es, row, sound)
    host = [_host_status(zkp, vk, w, inp) for w, inp, _ in pool]
    assert host == [want for _, _, want in pool]
    n = 65
    pick = [j % len(pool) for j in range(n)]
    words = np.ascontiguousarray([pool[j][0] for j in pick], dtype=np.uint64)
    inputs = limbs([pool[j][1] for j in pick], npub)
    want = np.array([host[j] for j in pick], dtype=np.uint8)
    pvk = vk.prepare(ctx)
    plain = ctx.verify_many(vk, words, inputs, sound=sound)
    got = ctx.verify_many(pvk, words, inputs)
    assert got.tobytes() == plain.tobytes() and np.array_equal(got, want)
    assert ctx.verify_many(pvk, words, inputs).tobytes() == got.tobytes()
    # the Python verifier takes the prepared key in place of the key: same results, same exceptions
    pairs = [(zkp.Proof(w), inp) for w, inp, _ in pool]
    fine = [p for p, h in zip(pairs, host) if h != zkp.ZK_VERIFY_MALFORMED]
    assert np.array_equal(zkp.Verifier.verify_many(pvk, fine, ctx), zkp.Verifier.verify_many(vk, fine, ctx))
    with pytest.raises(ValueError, match="proof 2 "):
        zkp.Verifier.verify_many(pvk, pairs, ctx)
    pvk.free()


@pytest.mark.parametrize("sound", [False, True])
def test_verdict_when_the_sum_is_the_identity(zkp, ctx, pyref, sound):
    """IC cancels to the identity: the pair (-IC, gamma) drops out, here as on the host"""
    es = [(-5 * ek(1)) % R, ek(1)]
    vk = make_key(zkp, pyref, es, sound)
    good, other = make_proof(pyref, es, [5], sound), make_proof(pyref, es, [6], sound)
    words = np.ascontiguousarray([good, other, good], dtype=np.uint64)
    inputs = limbs([[5], [5], [6]], 1)
    host = [_host_status(zkp, vk, w, x) for w, x in zip(words, ([5], [5], [6]))]
    assert host == [zkp.ZK_VERIFY_ACCEPT, zkp.ZK_VERIFY_REJECT, zkp.ZK_VERIFY_REJECT]
    pvk = vk.prepare(ctx)
    ic, ok = pvk.prepare_inputs(inputs[:1])
    assert ok.tolist() == [1] and ic[0][12] == 1 and not ic[0][:12].any()
    got = ctx.verify_many(pvk, words, inputs)
    assert got.tolist() == host == ctx.verify_many(vk, words, inputs, sound=sound).tolist()


def test_bytes_variant_equals_the_plain_bytes_call(zkp, ctx, oracle, pyref, chunk64):
    """the toy pool of test_gpu_pairing.py (proofs from the oracle's prover), as wire bytes"""
    from test_gpu_pairing import TOY_XY
    csr = oracle.CSR.from_constraints([({1: 1}, {2: 1}, {3: 1})], 4)
    rc, pk, ovk = oracle.setup(csr, [2, 3, 1, 1, 5], 1)
    assert rc == 0
    vk = zkp.VerificationKey.from_points(ovk.field("alpha_g1"), ovk.field("beta_g2"), ovk.field("gamma_g2"),
                                         ovk.field("delta_g2"), ovk.ic_g1)
    rng = pyref.SplitMix64(4242)
    recs = []
    for x, y in TOY_XY:
        rc, pr = oracle.prove(pk, csr, oracle.fr_array([1, x, y, x * y]), 1, rng.fr(), rng.fr())
        assert rc == 0
        recs.append(zkp.Proof(np.array(pr, dtype=np.uint64)).serialize_compressed())
    xs = [x for x, _ in TOY_XY]
    pool = [(rec, x) for rec, x in zip(recs, xs)]
    # another proof's A, another proof's C, a wrong input
    pool += [(recs[1][:48] + recs[0][48:], 3), (recs[0][:144] + recs[1][144:], 3), (recs[0], 5)]
    pool += [(bytes([recs[2][0] & 0x7F]) + recs[2][1:], xs[2])]                          # a's compression flag clear
    pool += [(pyref.g1_compress(PU.g1_off_subgroup()[1]) + recs[3][48:], xs[3])]         # a outside the subgroup
    pool += [(recs[0], 3 + (5 << 64)), (recs[1], 7 << 64)]                               # lo64 decides
    n = 65
    pick = [pool[(j * 7) % len(pool)] for j in range(n)]
    data = b"".join(rec for rec, _ in pick)
    inputs = limbs([[x] for _, x in pick], 1)
    pvk = vk.prepare(ctx)
    st, pst = ctx.verify_many_bytes(vk, data, inputs, point_status=True)
    got, gpst = ctx.verify_many_bytes(pvk, data, inputs, point_status=True)
    assert got.tobytes() == st.tobytes() and gpst.tobytes() == pst.tobytes()
    assert set(st.tolist()) == {zkp.ZK_VERIFY_ACCEPT, zkp.ZK_VERIFY_REJECT, zkp.ZK_VERIFY_MALFORMED}
    for j, (rec, x) in enumerate(pick):
        try:
            host = zkp.ZK_VERIFY_ACCEPT if zkp.Verifier.verify(vk, zkp.Proof.deserialize_compressed(rec), [x]) \
                else zkp.ZK_VERIFY_REJECT
        except ValueError:
            host = zkp.ZK_VERIFY_MALFORMED
        assert got[j] == host, j
    assert np.array_equal(ctx.verify_many_bytes(pvk, data, inputs), st)
    pairs = [(rec, [x]) for rec, x in pick]
    with pytest.raises(ValueError) as plain_err:
        zkp.Verifier.verify_many_bytes(vk, pairs, ctx)
    with pytest.raises(ValueError) as prep_err:
        zkp.Verifier.verify_many_bytes(pvk, pairs, ctx)
    assert str(prep_err.value) == str(plain_err.value)
    fine = [p for p, s in zip(pairs, st) if s != zkp.ZK_VERIFY_MALFORMED]
    assert np.array_equal(zkp.Verifier.verify_many_bytes(pvk, fine, ctx), zkp.Verifier.verify_many_bytes(vk, fine, ctx))


# ----------------------------------------------------------- errors ----
def _raw_prepare(zkp, ctx, vk, sound):
    h = C.c_void_p()
    rc = zkp.lib().zk_vk_prepare(C.c_void_p(ctx._h), C.byref(vk.s), C.c_int(int(sound)), C.byref(h))
    return rc, h.value


def test_prepare_refuses_bad_keys_and_names_the_point(zkp, ctx, pyref):
    es = [ek(k) for k in range(3)]
    row = [11, 12]
    words = make_proof(pyref, es, row, False).reshape(1, -1)
    inputs = limbs([row], 2)
    # off the curve: refused by both
    bad = make_key(zkp, pyref, es, False)
    bad.ic_g1[1][6] ^= 1
    rc, h = _raw_prepare(zkp, ctx, bad, False)
    assert rc == zkp.ZK_ERR_ARG and not h
    assert "ic_g1[1]" in ctx.last_error() and "not on the curve" in ctx.last_error()
    with pytest.raises(ValueError):
        ctx.verify_many(bad, words, inputs)
    # on the curve, outside the subgroup: refused here, accepted by the plain call
    off = make_key(zkp, pyref, es, False)
    off.ic_g1[2] = pyref.g1_words(PU.g1_off_subgroup()[1])
    with pytest.raises(ValueError, match=r"ic_g1\[2\]: not in the prime-order subgroup"):
        off.prepare(ctx)
    assert set(ctx.verify_many(off, words, inputs).tolist()) <= {zkp.ZK_VERIFY_REJECT, zkp.ZK_VERIFY_ACCEPT}
    g2off = pyref.g2_words(PU.g2_off_subgroup()[0])
    off = make_key(zkp, pyref, es, True)
    for i, w in enumerate(g2off):
        off.s.gamma_g2.w[i] = int(w)
    with pytest.raises(ValueError, match="gamma_g2: not in the prime-order subgroup"):
        off.prepare(ctx)
    # ic_len too short is refused
    short = make_key(zkp, pyref, es, False)
    short.s.ic_len = 2
    rc, h = _raw_prepare(zkp, ctx, short, False)
    assert rc == zkp.ZK_ERR_ARG and not h and "shorter" in ctx.last_error()
    assert zkp.lib().zk_vk_prepare(C.c_void_p(ctx._h), None, 0, None) == zkp.ZK_ERR_ARG


def test_calls_refuse_what_the_plain_calls_refuse(zkp, ctx, pyref):
    es = [ek(k) for k in range(3)]
    row = [11, 12 + (9 << 64)]
    ref, snd = make_key(zkp, pyref, es, False), make_key(zkp, pyref, es, True)
    pref, psnd = ref.prepare(ctx), snd.prepare(ctx)
    assert (pref.sound, psnd.sound) == (False, True)
    # the mode comes from the key: the same row and proof under both
    w_ref, w_snd = make_proof(pyref, es, row, False).reshape(1, -1), make_proof(pyref, es, row, True).reshape(1, -1)
    inputs = limbs([row], 2)
    A, RJ = zkp.ZK_VERIFY_ACCEPT, zkp.ZK_VERIFY_REJECT
    assert ctx.verify_many(pref, w_ref, inputs).tolist() == [A]
    assert ctx.verify_many(psnd, w_ref, inputs).tolist() == [RJ]
    assert ctx.verify_many(psnd, w_snd, inputs).tolist() == [A]
    assert ctx.verify_many(pref, w_snd, inputs).tolist() == [RJ]
    assert ctx.verify_many(pref, w_ref, inputs, sound=True).tolist() == [A]      # the argument does not override the key
    a, _ = pref.prepare_inputs(inputs)
    b, _ = psnd.prepare_inputs(inputs)
    assert np.array_equal(a[0], expected(pyref, es, row, False)[0])
    assert np.array_equal(b[0], expected(pyref, es, row, True)[0])
    assert not np.array_equal(a, b)
    # an input-count mismatch, in every call; then the key still works
    three = np.zeros((1, 3, 4), dtype=np.uint64)
    st = np.full(2, 0xAA, dtype=np.uint8)
    rc = zkp.lib().zk_groth16_verify_many_prepared(C.c_void_p(ctx._h), pref._handle(), C.c_void_p(w_ref.ctypes.data),
                                                   C.c_void_p(three.ctypes.data), C.c_size_t(3), C.c_size_t(1),
                                                   C.c_void_p(st.ctypes.data))
    assert rc == zkp.ZK_ERR_INVALID_WITNESS and (st == 0xAA).all()
    with pytest.raises(zkp.InvalidWitness):
        ctx.verify_many(pref, w_ref, three)
    with pytest.raises(zkp.InvalidWitness):
        pref.prepare_inputs(three)
    with pytest.raises(zkp.InvalidWitness):
        ctx.verify_many_bytes(pref, bytes(192), three)
    with pytest.raises(zkp.InvalidWitness):
        zkp.Verifier.verify_many(pref, [(zkp.Proof(w_ref[0]), [1, 2, 3])], ctx)
    assert ctx.verify_many(pref, w_ref, inputs).tolist() == [A]
    # n = 0
    assert len(ctx.verify_many(pref, [], [])) == 0 and len(ctx.verify_many_bytes(pref, b"", [])) == 0
    ic, ok = pref.prepare_inputs([])
    assert ic.shape == (0, 13) and len(ok) == 0
    assert len(zkp.Verifier.verify_many(pref, [], ctx)) == 0
    # freed twice through Python; the object is gone
    assert pref.device_bytes() == plan(zkp, False, 2)[3]
    pref.free()
    pref.free()
    assert pref._h is None
    with pytest.raises(ValueError, match="freed"):
        ctx.verify_many(pref, w_ref, inputs)
    with pytest.raises(ValueError, match="freed"):
        pref.device_bytes()
    assert ctx.verify_many(psnd, w_snd, inputs).tolist() == [A]
    psnd.free()
