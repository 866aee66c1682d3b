"""Sound mode on the GPU: the 255-bit fixed-base kernel, sound setup and prove
against tests/sound_ref.py (synthetic n = 4), end-to-end proofs at sizes with
many blocks checked by the host pairing, verify_many in sound mode, the error
rules, and that the two modes do not leak into each other on one ctx."""
import numpy as np
import pytest

import sound_ref

pytestmark = pytest.mark.gpu

TWO64 = 1 << 64
R = sound_ref.R
SLOT_A, SLOT_B2, SLOT_B1, SLOT_IC, SLOT_H = range(5)


@pytest.fixture(scope="module")
def case():
    return sound_ref.build_case()


@pytest.fixture(scope="module")
def qap4(zkp):
    return zkp.QAP(zkp.CSRMatrices.synthetic(sound_ref.CASE_N))


@pytest.fixture(autouse=True)
def _default_options(zkp, ctx):
    yield
    ctx.set_schedule(-1)
    ctx.set_option(zkp.ZK_OPT_QUOTIENT_PATH, -1)
    ctx.set_option(zkp.ZK_OPT_SOUND_WIN_C, 0)


def _g1(pyref, words):
    w = [int(x) for x in words]
    if w[12]:
        return pyref.INF
    return (pyref.Fq1(sum(w[i] << (64 * i) for i in range(6))), pyref.Fq1(sum(w[6 + i] << (64 * i) for i in range(6))))


def _g2(pyref, words):
    w = [int(x) for x in words]
    if w[24]:
        return pyref.INF
    c = [sum(w[6 * k + i] << (64 * i) for i in range(6)) for k in range(4)]
    return (pyref.Fq2(c[0], c[1]), pyref.Fq2(c[2], c[3]))


def _neg_g1(zkp, words):
    """-P in canonical words (y -> p - y)."""
    w = np.array(words, dtype=np.uint64).copy()
    if w[12]:
        return w
    import pyref
    y = pyref.P - sum(int(w[6 + i]) << (64 * i) for i in range(6))
    w[6:12] = zkp.to_limbs(y, 6)
    return w


def _ic_point(zkp, ctx, vk, inputs):
    """IC = ic_g1[0] + sum x_i ic_g1[i+1] through the public 255-bit MSM."""
    sc = np.array([zkp.to_limbs(1)] + [zkp.to_limbs(x) for x in inputs], dtype=np.uint64)
    return ctx.msm_g1(vk.ic_g1, sc, 255)


def _pairing_accepts(zkp, ctx, vk, proof, inputs):
    """e(A,B) e(-alpha,beta) e(-IC,gamma) e(-C,delta) == 1 on the host pairing,
    with nothing of the sound verify code in it."""
    ic = _ic_point(zkp, ctx, vk, inputs)
    g1 = [proof.a, _neg_g1(zkp, vk.point("alpha_g1")), _neg_g1(zkp, ic), _neg_g1(zkp, proof.c)]
    g2 = [proof.b, vk.point("beta_g2"), vk.point("gamma_g2"), vk.point("delta_g2")]
    return zkp.pairing_product_is_one(g1, g2)


# ------------------------------------------------------ fixed base, 255 bits ---
def _edge_scalars(pyref):
    rng = pyref.SplitMix64(0xF1BA5E)
    return [0, 1, 2, 255, 256, TWO64 - 1, TWO64, (1 << 128) + 1, 1 << 248, 1 << 254, R - 1, R - 2, rng.fr(), rng.fr()]


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_fixed_base_255_edge_scalars(zkp, ctx, pyref, g2):
    ks = _edge_scalars(pyref)
    got = ctx.test_fixed_base(ks, g2=g2)
    curve, words = (pyref.G2, pyref.g2_words) if g2 else (pyref.G1, pyref.g1_words)
    for k, row in zip(ks, got):
        assert list(row) == words(curve.mul(curve.gen, k)), hex(k)


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_fixed_base_255_batch(zkp, ctx, pyref, g2):
    """300 scalars: two full 128-thread blocks and a partial third, each
    against the public MSM of the single term k * generator."""
    rng = pyref.SplitMix64(0xBA7C4)
    ks = [rng.fr() for _ in range(300)]
    got = ctx.test_fixed_base(ks, g2=g2)
    gen = np.array([(pyref.g2_words if g2 else pyref.g1_words)((pyref.G2 if g2 else pyref.G1).gen)], dtype=np.uint64)
    msm = ctx.msm_g2 if g2 else ctx.msm_g1
    for k, row in zip(ks, got):
        assert np.array_equal(row, msm(gen, np.array([zkp.to_limbs(k)], dtype=np.uint64), 255)), hex(k)
    with pytest.raises(ValueError):
        ctx.test_fixed_base(np.array([zkp.to_limbs(R)], dtype=np.uint64), g2=g2)


# ------------------------------------------------------------------- setup ---
def test_setup_equals_the_reference(zkp, ctx, pyref, case, qap4):
    crs = zkp.CRS.generate_from_qap(ctx, qap4, zkp.SetupParams(*case["params"]), sound_ref.CASE_PUBLIC, sound=True)
    assert crs.pk.sound and crs.vk.sound
    want = sound_ref.pk_to_product(zkp, case["pk"], qap4)
    for nm in ("a_g1", "b_g1", "b_g2", "ic_g1", "h_g1"):
        assert np.array_equal(getattr(crs.pk, nm), getattr(want, nm)), nm
    for nm in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2"):
        assert np.array_equal(crs.pk.point(nm), want.point(nm)), nm
    assert crs.pk.a_g1[0][12] == 1 and crs.pk.h_g1[-1][12] == 0     # identity entries are part of the comparison
    wvk = sound_ref.vk_to_product(zkp, case["vk"])
    assert np.array_equal(crs.vk.ic_g1, wvk.ic_g1)
    for nm in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2"):
        assert np.array_equal(crs.vk.point(nm), wvk.point(nm)), nm


def _host_rows(pk, slot):
    return {SLOT_A: pk.a_g1, SLOT_B2: pk.b_g2, SLOT_B1: pk.b_g1, SLOT_IC: pk.ic_g1, SLOT_H: pk.h_g1}[slot]


@pytest.mark.parametrize("c", [16, 22])
def test_device_key_bases_and_windows(zkp, ctx, pyref, case, qap4, c):
    """The device-built key holds the reference's non-identity bases (window
    0), its extras are alpha_1, delta_1 / beta_2, delta_2 / beta_1 alone, and
    window w of a base is 2^(c w) times it, for every window of the plan."""
    ctx.set_option(zkp.ZK_OPT_SOUND_WIN_C, c)
    dpk = zkp.CRS.generate_device(ctx, qap4, zkp.SetupParams(*case["params"]), sound_ref.CASE_PUBLIC, sound=True)
    assert dpk.sound
    win, win_c, shard, nshards = dpk.test_info()
    assert (win, win_c, shard, nshards) == ((255 + c - 1) // c, c, 0, 1)
    want = sound_ref.pk_to_product(zkp, case["pk"], qap4)
    npub = sound_ref.CASE_PUBLIC
    for slot, nex in ((SLOT_A, 2), (SLOT_B2, 2), (SLOT_B1, 1), (SLOT_IC, 0), (SLOT_H, 0)):
        idx, rows, extras = dpk.test_bases(slot, 0)
        assert extras == nex
        host = _host_rows(want, slot)
        off = npub + 1 if slot == SLOT_IC else 0
        keep = [i for i in range(len(host)) if not host[i][-1]]
        assert [int(i) - off for i in idx] == keep
        assert np.array_equal(rows[:len(idx)], host[keep])
    _, rows, _ = dpk.test_bases(SLOT_A, 0)
    assert np.array_equal(rows[-2], want.point("alpha_g1")) and np.array_equal(rows[-1], want.point("delta_g1"))
    _, rows, _ = dpk.test_bases(SLOT_B2, 0)
    assert np.array_equal(rows[-2], want.point("beta_g2")) and np.array_equal(rows[-1], want.point("delta_g2"))
    _, rows, _ = dpk.test_bases(SLOT_B1, 0)
    assert np.array_equal(rows[-1], want.point("beta_g1"))
    # every window by the chain rule (window w = 2^c x window w-1, public MSM),
    # the last one of three sampled bases against pyref too
    step = np.array([zkp.to_limbs(1 << c)], dtype=np.uint64)
    for slot, pick, g2 in ((SLOT_A, 0, False), (SLOT_B2, -1, True), (SLOT_H, 1, False)):
        prev = dpk.test_bases(slot, 0)[1][pick]
        first = prev
        for w in range(1, win):
            cur = dpk.test_bases(slot, w)[1][pick]
            assert np.array_equal(cur, (ctx.msm_g2 if g2 else ctx.msm_g1)(prev.reshape(1, -1), step, 255)), (slot, w)
            prev = cur
        curve, to_pt, words = (pyref.G2, _g2, pyref.g2_words) if g2 else (pyref.G1, _g1, pyref.g1_words)
        assert list(prev) == words(curve.mul(to_pt(pyref, first), 1 << (c * (win - 1))))
    with pytest.raises(ValueError):
        dpk.test_bases(SLOT_A, win)
    dpk.free()


# ------------------------------------------------------------------- prove ---
def _device_z(z_rows):
    import torch
    return torch.from_numpy(np.ascontiguousarray(z_rows).view(np.int64).copy()).cuda()


def test_prove_equals_the_reference(zkp, ctx, case, qap4):
    """Byte for byte (serialize_compressed): host and device witness, both
    schedules, both quotient paths, every window width."""
    want = sound_ref.proof_to_product(zkp, case["proof"]).serialize_compressed()
    w = zkp.Witness(case["z"], sound_ref.CASE_PUBLIC)
    dz = _device_z(w.assignment)
    host_pk = sound_ref.pk_to_product(zkp, case["pk"], qap4)
    r, s = case["r"], case["s"]
    for c in (16, 20, 22, 0):
        ctx.set_option(zkp.ZK_OPT_SOUND_WIN_C, c)
        keys = [host_pk.upload(ctx)]
        if c in (0, 16):
            keys.append(zkp.CRS.generate_device(ctx, qap4, zkp.SetupParams(*case["params"]), sound_ref.CASE_PUBLIC,
                                                sound=True))
        for dpk in keys:
            assert dpk.sound and dpk.test_info()[1] == (c or 20)
            for sched in (0, 3):
                for path in (0, 1):
                    ctx.set_schedule(sched)
                    ctx.set_option(zkp.ZK_OPT_QUOTIENT_PATH, path)
                    tag = (c, sched, path)
                    assert zkp.Prover.prove(dpk, w, r=r, s=s).serialize_compressed() == want, tag
                    got = zkp.Prover.prove_device(dpk, dz.data_ptr(), len(w.assignment), sound_ref.CASE_PUBLIC, r, s)
                    assert got.serialize_compressed() == want, tag
            ctx.set_schedule(-1)
            ctx.set_option(zkp.ZK_OPT_QUOTIENT_PATH, -1)
            assert zkp.Prover.prove(dpk, w, r=r, s=s).serialize_compressed() == want   # twice: identical bytes
            dpk.free()
    vk = sound_ref.vk_to_product(zkp, case["vk"])
    assert zkp.Verifier.verify(vk, zkp.Proof.deserialize_compressed(want), [case["z"][1]])


@pytest.mark.parametrize("removed", ["middle", "trailing"])
def test_prove_with_identity_h_bases(zkp, ctx, pyref, case, qap4, removed):
    """The whole-scalar twin of test_gpu_prove.py's test of the same name: the
    two ways H reaches the IC+H scalar vector, four words a scalar.  A sound
    setup never makes an identity h_g1 entry, so the reference key gets one by
    hand.  middle: index 1 -- the compacted H index is no longer the position
    (h_ident false), the quotient writes to its own buffer and a gather at
    offset count[IC] follows.  trailing: the last index with a non-zero
    coefficient, and the entry after it, whose coefficient is zero (n = 4: H
    has n - 1 coefficients, h_g1 n entries), so that the identity entries end
    the vector and only shorten it (h_ident true, count[H] < n): the quotient
    writes straight into the scalar vector.  Host and device witness, both
    quotient paths, against sound_ref.prove_sound on the same modified key."""
    n = sound_ref.CASE_N
    h = case["qap"].compute_quotient_polynomial(case["z"])
    last = max(i for i, c in enumerate(h) if c % R)
    gone = [1] if removed == "middle" else list(range(last, n))
    assert h[gone[0]] % R and not any(h[i] % R for i in gone[1:] if i < len(h))
    pk = dict(case["pk"])
    pk["h_g1"] = [pyref.INF if i in gone else p for i, p in enumerate(case["pk"]["h_g1"])]
    proof = sound_ref.prove_sound(pk, case["qap"], case["z"], sound_ref.CASE_PUBLIC, case["r"], case["s"])
    assert proof[2] != case["proof"][2] and proof[:2] == case["proof"][:2]   # the removed base carried a coefficient
    want = sound_ref.proof_to_product(zkp, proof).serialize_compressed()
    assert want != sound_ref.proof_to_product(zkp, case["proof"]).serialize_compressed()
    w = zkp.Witness(case["z"], sound_ref.CASE_PUBLIC)
    dz = _device_z(w.assignment)
    dpk = sound_ref.pk_to_product(zkp, pk, qap4).upload(ctx)
    try:
        assert dpk.sound
        idx, _, _ = dpk.test_bases(SLOT_H)
        assert len(idx) == n - len(gone)
        assert np.array_equal(idx, np.arange(len(idx))) == (removed == "trailing")
        for path in (0, 1):
            ctx.set_option(zkp.ZK_OPT_QUOTIENT_PATH, path)
            assert zkp.Prover.prove(dpk, w, r=case["r"], s=case["s"]).serialize_compressed() == want, path
            got = zkp.Prover.prove_device(dpk, dz.data_ptr(), len(w.assignment), sound_ref.CASE_PUBLIC, case["r"],
                                          case["s"])
            assert got.serialize_compressed() == want, path
    finally:
        dpk.free()


def test_reference_toy_verifies_in_sound_mode(zkp, ctx):
    """x * y = z, z = [1, 3, 4, 12], the full-width parameter set that
    test_gpu_prove.py::test_gpu_proof_verifies_when_untruncated expects to
    fail in reference mode.  n = 1: H = 0 and Z(tau) = tau - 1."""
    cs = zkp.R1CS(0)
    x, y, z = (cs.allocate_variable() for _ in range(3))
    cs.enforce_multiplication(zkp.LinearCombination.from_variable(x), zkp.LinearCombination.from_variable(y),
                              zkp.LinearCombination.from_variable(z))
    qap = zkp.QAP.from_r1cs(cs)
    w = zkp.Witness([1, 3, 4, 12], 1)
    params = (0x1234567890ABCDEF1234567890, 7, 11, 13, 17)
    crs = zkp.CRS.generate_from_qap(ctx, qap, zkp.SetupParams(*params), 1, sound=True)
    dpk = crs.pk.upload(ctx)
    proof = zkp.Prover.prove(dpk, w, r=0xABCDEF, s=0x123456789)
    assert zkp.Verifier.verify(crs.vk, proof, [3]) is True
    assert zkp.Verifier.verify(crs.vk, proof, [5]) is False
    assert _pairing_accepts(zkp, ctx, crs.vk, proof, [3])
    assert zkp.Proof.deserialize_compressed(proof.serialize_compressed()) == proof
    dpk.free()
    with pytest.raises(zkp.SetupError):     # tau = 1 lies on the size-1 domain: Z(tau) = 0
        zkp.CRS.generate_from_qap(ctx, qap, zkp.SetupParams(*params[:4], 1), 1, sound=True)
    with pytest.raises(zkp.SetupError):
        zkp.CRS.generate_device(ctx, qap, zkp.SetupParams(*params[:4], 1), 1, sound=True)


@pytest.mark.parametrize("nc", [1000, 4096])
def test_end_to_end_many_blocks(zkp, ctx, oracle, pyref, nc):
    """GPU sound setup, then prove: 1000 constraints (n = 1024, padded rows,
    V = 3001) and 2^12.  The proof satisfies the pairing equation on the host
    pairing with IC from the public MSM; pi_A and pi_B are rebuilt from the
    host key with the public 255-bit MSMs plus pyref additions of the extras."""
    qap = zkp.QAP(zkp.CSRMatrices.synthetic(nc))
    rng = pyref.SplitMix64(0xE2E + nc)
    params = [rng.fr() for _ in range(5)]
    r, s, r2, s2 = (rng.fr() for _ in range(4))
    z = oracle.synthetic_witness(nc, 77 + nc)
    w = zkp.Witness(z, 1)
    crs = zkp.CRS.generate_from_qap(ctx, qap, zkp.SetupParams(*params), 1, sound=True)
    assert qap.domain_size == (1024 if nc == 1000 else 4096) and len(crs.pk.h_g1) == qap.domain_size
    dpk = zkp.CRS.generate_device(ctx, qap, zkp.SetupParams(*params), 1, sound=True)
    proof = zkp.Prover.prove(dpk, w, r=r, s=s)
    up = crs.pk.upload(ctx)
    assert zkp.Prover.prove(up, w, r=r, s=s) == proof                 # uploaded host key: the same bytes
    x = [zkp.from_limbs(z[1])]
    assert _pairing_accepts(zkp, ctx, crs.vk, proof, x)
    assert zkp.Verifier.verify(crs.vk, proof, x) is True
    assert zkp.Verifier.verify(crs.vk, proof, [x[0] + TWO64]) is False
    # pi_A = alpha_1 + sum z_i a_g1[i] + r delta_1, pi_B likewise in G2
    a = pyref.G1.add(_g1(pyref, ctx.msm_g1(crs.pk.a_g1, z, 255)), _g1(pyref, crs.pk.point("alpha_g1")))
    a = pyref.G1.add(a, pyref.G1.mul(_g1(pyref, crs.pk.point("delta_g1")), r))
    assert list(proof.a) == pyref.g1_words(a)
    b = pyref.G2.add(_g2(pyref, ctx.msm_g2(crs.pk.b_g2, z, 255)), _g2(pyref, crs.pk.point("beta_g2")))
    b = pyref.G2.add(b, pyref.G2.mul(_g2(pyref, crs.pk.point("delta_g2")), s))
    assert list(proof.b) == pyref.g2_words(b)
    other = zkp.Prover.prove(dpk, w, r=r2, s=s2)
    assert not np.array_equal(other.a, proof.a) and not np.array_equal(other.b, proof.b)
    assert not np.array_equal(other.c, proof.c)
    assert zkp.Verifier.verify(crs.vk, other, x) is True and _pairing_accepts(zkp, ctx, crs.vk, other, x)
    mixed = zkp.Proof(np.concatenate([proof.a, proof.b, other.c]))
    assert zkp.Verifier.verify(crs.vk, mixed, x) is False
    dpk.free()
    up.free()


# ------------------------------------------------------------- verify_many ---
def test_verify_many_sound(zkp, ctx, pyref, qap4):
    """72 (proof, inputs) pairs -- more than one 64-lane block -- under a
    num_public = 3 key with full-width inputs: each status is what
    zk_groth16_verify_sound gives for the pair alone.  The same pool through
    the reference-mode call keeps that mode's statuses: what the unchanged
    host zk_groth16_verify says (lo64 inputs, so an input >= r is no error
    there), and REJECT for every well-formed pair."""
    rng = pyref.SplitMix64(0x3A17)
    crs = zkp.CRS.generate_from_qap(ctx, qap4, zkp.SetupParams(*[rng.fr() for _ in range(5)]), 3, sound=True)
    z = pyref.synthetic_witness(sound_ref.CASE_N, 0x3A18)
    dpk = crs.pk.upload(ctx)
    p1 = zkp.Prover.prove(dpk, zkp.Witness(z, 3), r=rng.fr(), s=rng.fr())
    p2 = zkp.Prover.prove(dpk, zkp.Witness(z, 3), r=rng.fr(), s=rng.fr())
    dpk.free()
    x = zkp.fr_array(z[1:4])
    assert all(v >= TWO64 for v in z[1:4])
    plus = x.copy()
    plus[1, 1] += np.uint64(1)                                  # x_1 + 2^64: limb 1 only
    big = x.copy()
    big[2] = zkp.to_limbs(R)                                    # x_2 = r
    off = p1.words.copy()
    off[6] ^= np.uint64(1)                                      # A off its curve
    swapped = np.concatenate([p1.a, p1.b, p2.c])
    A, RJ, M = zkp.ZK_VERIFY_ACCEPT, zkp.ZK_VERIFY_REJECT, zkp.ZK_VERIFY_MALFORMED
    variants = [(p1.words, x, A, RJ), (p2.words, x, A, RJ), (p1.words, plus, RJ, RJ), (p2.words, big, M, RJ),
                (off, x, M, M), (swapped, x, RJ, RJ)]
    for words, inp, want_sound, want_ref in variants:           # the expectations themselves, one pair at a time
        for vk_sound, want in ((True, want_sound), (False, want_ref)):
            crs.vk.sound = vk_sound
            try:
                got = A if zkp.Verifier.verify(crs.vk, zkp.Proof(words), inp) else RJ
            except ValueError:
                got = M
            assert got == want
    crs.vk.sound = True
    order = [k % len(variants) for k in range(72)]
    proofs = np.array([variants[k][0] for k in order], dtype=np.uint64)
    inputs = np.array([variants[k][1] for k in order], dtype=np.uint64)
    assert ctx.verify_many(crs.vk, proofs, inputs, sound=True).tolist() == [variants[k][2] for k in order]
    assert ctx.verify_many(crs.vk, proofs, inputs).tolist() == [variants[k][3] for k in order]
    good = [(zkp.Proof(variants[k][0]), variants[k][1]) for k in (0, 1, 2, 5)]
    assert zkp.Verifier.verify_many(crs.vk, good, ctx).tolist() == [True, True, False, False]
    with pytest.raises(ValueError):
        zkp.Verifier.verify_many(crs.vk, [(p2, big)], ctx)
    with pytest.raises(zkp.InvalidWitness):
        ctx.verify_many(crs.vk, proofs[:1], inputs[:1, :2], sound=True)


# ------------------------------------------------------------------ errors ---
def test_sound_errors(zkp, ctx, case, qap4):
    host_pk = sound_ref.pk_to_product(zkp, case["pk"], qap4)
    dpk = host_pk.upload(ctx)
    r, s = case["r"], case["s"]
    z = list(case["z"])
    bad = list(z)
    bad[6] = (bad[6] + 1) % R                     # row 1 (variables 4, 5, 6)
    with pytest.raises(zkp.InvalidWitness):
        zkp.Prover.prove(dpk, zkp.Witness(bad, 1), r=r, s=s)
    bad = list(z)
    bad[9] = (bad[9] + 1) % R                     # row 2 only
    with pytest.raises(zkp.PolynomialDivisionFailed):
        zkp.Prover.prove(dpk, zkp.Witness(bad, 1), r=r, s=s)
    rows = zkp.fr_array(z)
    rows[5] = zkp.to_limbs(R)                     # z_5 = r: not a canonical Fr
    dz = _device_z(rows)
    with pytest.raises(ValueError):
        zkp.Prover.prove_device(dpk, dz.data_ptr(), len(rows), 1, r, s)
    good = _device_z(zkp.fr_array(z))
    with pytest.raises(ValueError, match="sound"):
        zkp.Prover.prove_partial(dpk, good.data_ptr(), len(z), 1, r, s)
    with pytest.raises(ValueError, match="sound"):
        dpk.witness_ranges()
    with pytest.raises(ValueError):
        host_pk.upload(ctx, shard=0, nshards=2)
    with pytest.raises(ValueError):
        zkp.CRS.generate_device(ctx, qap4, zkp.SetupParams(*case["params"]), 1, nshards=2, sound=True)
    with pytest.raises(ValueError):
        ctx.set_option(zkp.ZK_OPT_SOUND_WIN_C, 18)
    # the key still proves after the refused calls
    want = sound_ref.proof_to_product(zkp, case["proof"])
    assert zkp.Prover.prove(dpk, zkp.Witness(z, 1), r=r, s=s) == want
    dpk.free()


# ------------------------------------------------------ modes do not leak ---
def test_modes_do_not_leak(zkp, ctx, oracle, pyref):
    """One ctx, in order: a reference key's proof, a sound key's, the
    reference key's again -- workspaces and plans (ctx->msm, the scalar
    buffers) are shared between the widths."""
    import gpu_util as U
    n = 1 << 10
    qap = zkp.QAP(zkp.CSRMatrices.synthetic(n))
    csr_o = oracle.CSR.synthetic(n)
    rng = pyref.SplitMix64(0x1EA4)
    params = [rng.fr() for _ in range(5)]
    r, s = rng.fr(), rng.fr()
    z = oracle.synthetic_witness(n, 0x1EA5)
    rc, opk, _ = oracle.setup(csr_o, params, 1, nthreads=8)
    assert rc == 0
    rc, oproof = oracle.prove(opk, csr_o, z, 1, r, s)
    assert rc == 0
    ref_key = U.pk_from_oracle(zkp, opk, qap, 1).upload(ctx)
    assert not ref_key.sound and ref_key.test_info()[:2] == (4, 16)
    crs = zkp.CRS.generate_from_qap(ctx, qap, zkp.SetupParams(*params), 1, sound=True)
    sound_key = crs.pk.upload(ctx)
    w = zkp.Witness(z, 1)
    first = zkp.Prover.prove(ref_key, w, r=r, s=s)
    sound_proof = zkp.Prover.prove(sound_key, w, r=r, s=s)
    again = zkp.Prover.prove(ref_key, w, r=r, s=s)
    assert np.array_equal(first.words, oproof) and np.array_equal(again.words, oproof)
    assert zkp.Verifier.verify(crs.vk, sound_proof, [zkp.from_limbs(z[1])]) is True
    assert zkp.Prover.prove(sound_key, w, r=r, s=s) == sound_proof
    ref_key.free()
    sound_key.free()


# --------------------------------------------------------------- key files ---
def test_compressed_sound_key_files(zkp, ctx, case, qap4, tmp_path):
    """ZKAMDPS2 / ZKAMDVS2 (decompressed on the GPU when loaded) keep .sound
    and every point."""
    pk = sound_ref.pk_to_product(zkp, case["pk"], qap4)
    vk = sound_ref.vk_to_product(zkp, case["vk"])
    zkp.save_proving_key(pk, tmp_path / "pk.bin", compressed=True)
    zkp.save_verification_key(vk, tmp_path / "vk.bin", compressed=True)
    assert open(tmp_path / "pk.bin", "rb").read(8) == b"ZKAMDPS2"
    assert open(tmp_path / "vk.bin", "rb").read(8) == b"ZKAMDVS2"
    back = zkp.load_proving_key(tmp_path / "pk.bin", ctx)
    assert back.sound is True
    for nm in ("a_g1", "b_g1", "b_g2", "ic_g1", "h_g1"):
        assert np.array_equal(getattr(back, nm), getattr(pk, nm)), nm
    for nm in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2"):
        assert np.array_equal(back.point(nm), pk.point(nm)), nm
    vb = zkp.load_verification_key(tmp_path / "vk.bin", ctx)
    assert vb.sound is True and np.array_equal(vb.ic_g1, vk.ic_g1)
    dpk = back.upload(ctx)
    assert dpk.sound
    proof = zkp.Prover.prove(dpk, zkp.Witness(case["z"], 1), r=case["r"], s=case["s"])
    assert proof == sound_ref.proof_to_product(zkp, case["proof"])
    assert zkp.Verifier.verify(vb, proof, [case["z"][1]]) is True
    dpk.free()
