"""Point decompression and validation on the GPU (csrc/points.hip) against
oracle/pyref.py and the host decoder of the proof codec: the square-root
hooks, valid and invalid encodings of every status, chunking, validation of
affine points, and compressed key files end to end."""
import ctypes as C

import numpy as np
import pytest

import gpu_util as U
import points_util as PU
import pyref as P
from helpers import fr_rows, golden

pytestmark = pytest.mark.gpu
G = golden()
PM = PU.PMOD


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _decompress(zkp, ctx, group, data):
    """The raw C call: (rc, words, status, first_bad)."""
    enc, w = (48, 13) if group == 1 else (96, 25)
    n = len(data) // enc
    buf = np.frombuffer(bytes(data) + bytes(16), dtype=np.uint8)
    out = np.full((n + 1, w), 0xEE, dtype=np.uint64)
    st = np.full(n + 1, 0xEE, dtype=np.uint8)
    fb = C.c_size_t(12345)
    fn = zkp.lib().zk_g1_decompress if group == 1 else zkp.lib().zk_g2_decompress
    rc = fn(C.c_void_p(ctx._h), _ptr(buf), C.c_size_t(n), _ptr(out), _ptr(st), C.byref(fb))
    assert st[n] == 0xEE and (out[n] == 0xEE).all()   # nothing past n is written
    return rc, out[:n], st[:n], fb.value


def _validate(zkp, ctx, group, words):
    a = np.ascontiguousarray(words, dtype=np.uint64)
    n = len(a)
    st = np.full(n + 1, 0xEE, dtype=np.uint8)
    fb = C.c_size_t(12345)
    fn = zkp.lib().zk_g1_validate if group == 1 else zkp.lib().zk_g2_validate
    rc = fn(C.c_void_p(ctx._h), _ptr(a), C.c_size_t(n), _ptr(st), C.byref(fb))
    assert st[n] == 0xEE
    return rc, st[:n], fb.value


def _limbs6(v):
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(6)]


def _int6(w):
    return sum(int(x) << (64 * i) for i, x in enumerate(w))


def _rand_fq(rng):
    return sum(rng.next() << (64 * i) for i in range(6)) % PM


# ------------------------------------------------------------ sqrt hooks ----
def test_fq_sqrt_hook(zkp, ctx):
    rng = P.SplitMix64(0x5157)
    vals = [0, 1, 4, PM - 1] + [pow(_rand_fq(rng), 2, PM) for _ in range(16)]
    non = []
    while len(non) < 8:
        v = _rand_fq(rng)
        if pow(v, (PM - 1) // 2, PM) == PM - 1:
            non.append(v)
    vals += non
    n = len(vals)
    inp = np.array([_limbs6(v) for v in vals], dtype=np.uint64)
    out = np.zeros((n, 6), dtype=np.uint64)
    ok, big = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    rc = zkp.test_lib().zk_test_fq_sqrt(C.c_void_p(ctx._h), _ptr(inp), C.c_size_t(n), _ptr(out), _ptr(ok), _ptr(big))
    assert rc == zkp.ZK_OK
    for i, v in enumerate(vals):
        want = PU.fq_sqrt(v) is not None
        assert bool(ok[i]) == want, (i, hex(v))
        r = _int6(out[i])
        if want:
            assert r < PM and r * r % PM == v, (i, hex(v))
            assert bool(big[i]) == P._largest(r), i
        else:
            assert r == 0 and big[i] == 0
    assert not ok[3] and not ok[-8:].any() and ok[:3].all() and ok[4:20].all()   # p - 1 is a non-residue


def test_fq2_sqrt_hook(zkp, ctx):
    rng = P.SplitMix64(0x5158)
    f2 = P.Fq2
    vals = [f2(0, 0), f2(1, 0), f2(PM - 1, 0), f2(0, 1)]
    for _ in range(16):
        a = f2(_rand_fq(rng), _rand_fq(rng))
        vals.append(a * a)
    for _ in range(2):   # roots with a zero coefficient
        a, b = f2(_rand_fq(rng), 0), f2(0, _rand_fq(rng))
        vals += [a * a, b * b]
    nonres = next(v for v in iter(lambda: _rand_fq(rng), None) if PU.fq_sqrt(v) is None)
    vals.append(f2(nonres, 0))   # inside Fq, a non-residue there: the root is purely imaginary
    non = []
    while len(non) < 8:
        a = f2(_rand_fq(rng), _rand_fq(rng))
        if PU.fq2_sqrt(a) is None:
            non.append(a)
    vals += non
    n = len(vals)
    inp = np.array([_limbs6(v.c0) + _limbs6(v.c1) for v in vals], dtype=np.uint64)
    out = np.zeros((n, 12), dtype=np.uint64)
    ok, big = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    rc = zkp.test_lib().zk_test_fq2_sqrt(C.c_void_p(ctx._h), _ptr(inp), C.c_size_t(n), _ptr(out), _ptr(ok),
                                         _ptr(big))
    assert rc == zkp.ZK_OK
    for i, v in enumerate(vals):
        want = PU.fq2_sqrt(v) is not None
        assert bool(ok[i]) == want, i
        r = f2(_int6(out[i][:6]), _int6(out[i][6:]))
        assert _int6(out[i][:6]) < PM and _int6(out[i][6:]) < PM
        if want:
            assert r * r == v, i
            assert bool(big[i]) == PU.fq2_largest(r), i
        else:
            assert r.is_zero() and big[i] == 0
    assert ok[:n - 8].all() and not ok[n - 8:].any()
    r_im = f2(_int6(out[n - 9][:6]), _int6(out[n - 9][6:]))
    assert r_im.c0 == 0 and r_im.c1 != 0


# ------------------------------------------------------ decompress: valid ----
def _with_identities(pts, n):
    pts = list(pts[:n])
    if n >= 3:
        for k in (0, n // 2, n - 1):
            pts[k] = P.INF
    return pts


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_g1_decompress_valid(zkp, ctx, n):
    for sign in (0, 1):
        pts = _with_identities([P.G1.neg(p) if sign else p for p in PU.g1_points(257)], n)
        rc, words, st, fb = _decompress(zkp, ctx, 1, b"".join(P.g1_compress(p) for p in pts))
        assert rc == zkp.ZK_OK and not st.any() and fb == n
        assert np.array_equal(words, PU.words_g1(pts))
    w2, s2 = ctx.g1_decompress(b"".join(P.g1_compress(p) for p in pts))
    assert np.array_equal(w2, words) and np.array_equal(s2, st)


@pytest.mark.parametrize("n", [0, 1, 65, 129])
def test_g2_decompress_valid(zkp, ctx, n):
    for sign in (0, 1):
        pts = _with_identities([P.G2.neg(p) if sign else p for p in PU.g2_points(129)], n)
        rc, words, st, fb = _decompress(zkp, ctx, 2, b"".join(P.g2_compress(p) for p in pts))
        assert rc == zkp.ZK_OK and not st.any() and fb == n
        assert np.array_equal(words, PU.words_g2(pts))
    w2, s2 = ctx.g2_decompress(b"".join(P.g2_compress(p) for p in pts))
    assert np.array_equal(w2, words) and np.array_equal(s2, st)


# --------------------------------------------------------------- chunking ----
def test_chunking_and_option(zkp, ctx):
    pts = list(PU.g1_points(257)[:200])
    data = bytearray(b"".join(P.g1_compress(p) for p in pts))
    data[48 * 130:48 * 131] = P.g1_compress(PU.g1_off_subgroup()[0])
    data = bytes(data)
    ref = _decompress(zkp, ctx, 1, data)
    setopt = zkp.lib().zk_ctx_set_option
    try:
        for bad in (0, -1):
            assert setopt(C.c_void_p(ctx._h), C.c_int(zkp.ZK_OPT_POINT_CHUNK), C.c_int64(bad)) == zkp.ZK_ERR_ARG
        ctx.set_option(zkp.ZK_OPT_POINT_CHUNK, 64)
        got = _decompress(zkp, ctx, 1, data)
    finally:
        ctx.set_option(zkp.ZK_OPT_POINT_CHUNK, 1 << 20)
    assert ref[0] == got[0] == zkp.ZK_ERR_ARG and ref[3] == got[3] == 130
    assert np.array_equal(ref[1], got[1]) and np.array_equal(ref[2], got[2])
    want = np.zeros(200, dtype=np.uint8)
    want[130] = PU.ST_SUBGROUP
    assert np.array_equal(got[2], want)
    exp = PU.words_g1(pts)
    exp[130] = 0
    assert np.array_equal(got[1], exp)


# ---------------------------------------------------- decompress: invalid ----
def _mixed_batch(invalid, valid_pts, compress):
    """3 valid points, then invalid and valid encodings alternating."""
    encs, want = [], []
    for k in range(3):
        encs.append(compress(valid_pts[k]))
        want.append((PU.ST_OK, valid_pts[k]))
    for k, (enc, st) in enumerate(invalid):
        encs.append(enc)
        want.append((st, None))
        p = valid_pts[3 + k]
        encs.append(compress(p))
        want.append((PU.ST_OK, p))
    return encs, want


@pytest.mark.parametrize("group", [1, 2])
def test_decompress_invalid(zkp, ctx, group):
    if group == 1:
        invalid, pts, compress, words_of = PU.invalid_g1(), PU.g1_points(257), P.g1_compress, P.g1_words
    else:
        invalid, pts, compress, words_of = PU.invalid_g2(), PU.g2_points(129), P.g2_compress, P.g2_words
    assert {s for _, s in invalid} == {1, 2, 3, 4}
    encs, want = _mixed_batch(invalid, pts, compress)
    rc, words, st, fb = _decompress(zkp, ctx, group, b"".join(encs))
    assert rc == zkp.ZK_ERR_ARG and fb == 3
    for i, (s, p) in enumerate(want):
        assert st[i] == s, (i, encs[i].hex())
        if s == PU.ST_OK:
            assert list(words[i]) == words_of(p), i
        else:
            assert not words[i].any(), i
        # the host decoder accepts exactly what the GPU accepts, with the same words
        host = PU.host_decode(zkp, encs[i])
        assert (host is None) == (s != PU.ST_OK), i
        if host is not None:
            assert np.array_equal(host, words[i]), i


# --------------------------------------------------------------- validate ----
def _validate_cases(group):
    """[(words, expected status)]: the first entries are the special ones."""
    if group == 1:
        curve, words_of, off, pts, w = P.G1, P.g1_words, PU.g1_off_subgroup(), PU.g1_points(257), 13
    else:
        curve, words_of, off, pts, w = P.G2, P.g2_words, PU.g2_off_subgroup(), PU.g2_points(129), 25
    out = []
    for q in off:
        out += [(words_of(q), PU.ST_SUBGROUP), (words_of(curve.neg(q)), PU.ST_SUBGROUP)]
    base = words_of(pts[0])
    half = (w - 1) // 2
    for pos in range(0, w - 1, 6):          # each coordinate (coefficient) set to p
        bad = list(base)
        bad[pos:pos + 6] = _limbs6(PM)
        out.append((bad, PU.ST_RANGE))
    bad = list(base)
    bad[half] ^= 1                           # y off by one
    out.append((bad, PU.ST_CURVE))
    out.append(([0] * (w - 1) + [0], PU.ST_CURVE))          # (0, 0) without the infinity byte
    out.append(([0xFFFFFFFFFFFFFFFF] * (w - 1) + [1], PU.ST_OK))   # infinity byte over garbage
    out.append((words_of(P.INF), PU.ST_OK))
    for p in pts:
        out += [(words_of(p), PU.ST_OK), (words_of(curve.neg(p)), PU.ST_OK)]
    return out


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("n", [1, 65, 257])
def test_validate(zkp, ctx, group, n):
    cases = _validate_cases(group)[:n]
    assert len(cases) == n
    words = np.array([c[0] for c in cases], dtype=np.uint64)
    want = np.array([c[1] for c in cases], dtype=np.uint8)
    rc, st, fb = _validate(zkp, ctx, group, words)
    assert np.array_equal(st, want), np.flatnonzero(st != want)
    assert rc == zkp.ZK_ERR_ARG and fb == 0      # the first case is an off-subgroup point
    good = words[want == 0]
    rc, st, fb = _validate(zkp, ctx, group, good)
    assert rc == zkp.ZK_OK and not st.any() and fb == len(good)
    assert np.array_equal((ctx.g1_validate if group == 1 else ctx.g2_validate)(words), want)


# ------------------------------------------------- key files, end to end ----
def _golden_key(zkp, name, identity_h):
    case = next(c for c in G["prove"] if c["name"] == name)
    pk = U.pk_from_golden(zkp, case, U.qap_from_case(zkp, case))
    if identity_h:
        # deg h <= n - 2: the last H base never enters a proof, so it may be the identity
        pk.h_g1[-1] = P.g1_words(P.INF)
    return case, pk


_PK_ARRAYS = ("a_g1", "b_g1", "b_g2", "ic_g1", "h_g1")
_PK_POINTS = ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2")


@pytest.mark.parametrize("name,identity_h", [("synthetic_8", False), ("random_5x9_pub2", True)])
def test_compressed_key_file_round_trip_and_prove(zkp, ctx, tmp_path, name, identity_h):
    case, pk = _golden_key(zkp, name, identity_h)
    path = tmp_path / "pk2.bin"
    zkp.save_proving_key(pk, path, compressed=True)
    back = zkp.load_proving_key(path, ctx=ctx)
    for nm in _PK_ARRAYS:
        assert np.array_equal(getattr(back, nm), getattr(pk, nm)), nm
    for nm in _PK_POINTS:
        assert np.array_equal(back.point(nm), pk.point(nm)), nm
    assert back.num_public == pk.num_public
    dpk = back.upload(ctx)
    w = zkp.Witness(fr_rows(case["z"]), case["num_public"])
    proof = zkp.Prover.prove(dpk, w, r=int(case["r"], 16), s=int(case["s"], 16))
    dpk.free()
    assert proof.serialize_compressed().hex() == case["proof_compressed"]
    # the verification key's compressed file
    from helpers import g1_words, g2_words
    vk = zkp.VerificationKey.from_points(g1_words(case["pk"]["alpha_g1"]), g2_words(case["pk"]["beta_g2"]),
                                         g2_words(case["vk"]["gamma_g2"]), g2_words(case["pk"]["delta_g2"]),
                                         [g1_words(p) for p in case["vk"]["ic_g1"]])
    vpath = tmp_path / "vk2.bin"
    zkp.save_verification_key(vk, vpath, compressed=True)
    vb = zkp.load_verification_key(vpath, ctx=ctx)
    assert np.array_equal(vb.ic_g1, vk.ic_g1) and vb.num_public == vk.num_public
    for nm in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2"):
        assert np.array_equal(vb.point(nm), vk.point(nm)), nm
    vk.validate(ctx)


def test_compressed_key_file_flipped_byte(zkp, ctx, tmp_path):
    _, pk = _golden_key(zkp, "synthetic_8", False)
    path = tmp_path / "pk2.bin"
    zkp.save_proving_key(pk, path, compressed=True)
    data = bytearray(path.read_bytes())
    idx = next(i for i in range(len(pk.b_g2)) if not pk.b_g2[i][24])   # a non-identity b_g2 entry
    off = 80 + 3 * 48 + 2 * 96 + 48 * (len(pk.a_g1) + len(pk.b_g1)) + 96 * idx
    data[off + 70] ^= 0x04                                                # inside x.c0 of b_g2[idx]
    path.write_bytes(bytes(data))
    with pytest.raises(ValueError, match=r"pk2\.bin: b_g2\[%d\]: " % idx):
        zkp.load_proving_key(path, ctx=ctx)


def test_uncompressed_key_validation(zkp, ctx, tmp_path):
    _, pk = _golden_key(zkp, "synthetic_8", False)
    path = tmp_path / "pk1.bin"
    zkp.save_proving_key(pk, path)
    zkp.load_proving_key(path, ctx=ctx, validate=True)
    pk.validate(ctx)
    pk.a_g1[2] = P.g1_words(PU.g1_off_subgroup()[0])       # the point of order 3
    zkp.save_proving_key(pk, path)
    assert np.array_equal(zkp.load_proving_key(path).a_g1, pk.a_g1)   # the default load does not look
    with pytest.raises(ValueError, match=r"pk1\.bin: a_g1\[2\]: not in the prime-order subgroup"):
        zkp.load_proving_key(path, ctx=ctx, validate=True)
    with pytest.raises(zkp.SetupError, match=r"a_g1\[2\]: not in the prime-order subgroup"):
        pk.validate(ctx)
