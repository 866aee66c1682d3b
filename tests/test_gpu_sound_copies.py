"""Sound keys with fewer window copies (ZK_OPT_SOUND_COPIES): the proofs stay
the bytes of tests/sound_ref.py and of a default-options key whatever the
number of copies, the key holds exactly the copies asked for and shrinks with
them, and neither reference-mode keys nor keys made earlier notice the option."""
import numpy as np
import pytest

import gpu_util as U
import sound_ref
from helpers import fr_rows, golden, proof_words

pytestmark = pytest.mark.gpu

SLOT_A, SLOT_B2, SLOT_B1, SLOT_IC, SLOT_H = range(5)
DEFAULT_C = 20


def _windows(c):
    return (255 + c - 1) // c


def _sets(c, copies):
    w = _windows(c)
    s = min(copies, w)
    return s, (w + s - 1) // s


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
    ctx.set_option(zkp.ZK_OPT_SOUND_COPIES, 0)


def _device_z(z_rows):
    import torch
    return torch.from_numpy(np.ascontiguousarray(z_rows).view(np.int64).copy()).cuda()


def _sound_device_key(zkp, ctx, qap, params, num_public):
    return zkp.CRS.generate_device(ctx, qap, zkp.SetupParams(*params), num_public, sound=True)


# ------------------------------------------------------------- prove bytes ---
@pytest.mark.parametrize("copies", [1, 2, 4, 7, "W"])
@pytest.mark.parametrize("c", [16, 20, 22])
def test_prove_equals_the_reference(zkp, ctx, case, qap4, c, copies):
    """Byte for byte (serialize_compressed) for the uploaded host key and the
    device-built one: both schedules, both quotient paths, host and device
    witness.  4 and 7 do not divide 13 or 16: the last bucket set is partly
    used; W is the shared plan asked for by number."""
    copies = _windows(c) if copies == "W" else copies
    want = sound_ref.proof_to_product(zkp, case["proof"]).serialize_compressed()
    w = zkp.Witness(case["z"], sound_ref.CASE_PUBLIC)
    dz = _device_z(w.assignment)
    r, s = case["r"], case["s"]
    ctx.set_option(zkp.ZK_OPT_SOUND_WIN_C, c)
    ctx.set_option(zkp.ZK_OPT_SOUND_COPIES, copies)
    keys = [sound_ref.pk_to_product(zkp, case["pk"], qap4).upload(ctx),
            _sound_device_key(zkp, ctx, qap4, case["params"], sound_ref.CASE_PUBLIC)]
    for dpk in keys:
        assert dpk.sound and dpk.test_info()[:2] == (_windows(c), c)
        assert dpk.test_plan() == _sets(c, copies)
        for sched in (0, 3):
            for path in (0, 1):
                ctx.set_schedule(sched)
                ctx.set_option(zkp.ZK_OPT_QUOTIENT_PATH, path)
                tag = (c, copies, sched, path)
                assert zkp.Prover.prove(dpk, w, r=r, s=s).serialize_compressed() == want, tag
                got = zkp.Prover.prove_device(dpk, dz.data_ptr(), len(w.assignment), sound_ref.CASE_PUBLIC, r, s)
                assert got.serialize_compressed() == want, tag
        dpk.free()


# -------------------------------------------------------------- end to end ---
def _neg_g1(zkp, pyref, words):
    w = np.array(words, dtype=np.uint64).copy()
    if not w[12]:
        w[6:12] = zkp.to_limbs(pyref.P - sum(int(w[6 + i]) << (64 * i) for i in range(6)), 6)
    return w


def _pairing_accepts(zkp, ctx, pyref, vk, proof, inputs):
    """e(A,B) e(-alpha,beta) e(-IC,gamma) e(-C,delta) == 1 on the host pairing,
    IC = ic_g1[0] + sum x_i ic_g1[i+1] from the public 255-bit MSM."""
    sc = np.array([zkp.to_limbs(1)] + [zkp.to_limbs(x) for x in inputs], dtype=np.uint64)
    ic = ctx.msm_g1(vk.ic_g1, sc, 255)
    g1 = [proof.a] + [_neg_g1(zkp, pyref, p) for p in (vk.point("alpha_g1"), ic, proof.c)]
    g2 = [proof.b, vk.point("beta_g2"), vk.point("gamma_g2"), vk.point("delta_g2")]
    return zkp.pairing_product_is_one(g1, g2)


def test_end_to_end_many_blocks(zkp, ctx, oracle, pyref):
    """1000 constraints (n = 1024, padded rows, V = 3001), 3 copies at the
    default c = 20: 5 bucket sets, the last holding window 12 alone."""
    nc = 1000
    qap = zkp.QAP(zkp.CSRMatrices.synthetic(nc))
    rng = pyref.SplitMix64(0xC091E5 + nc)
    params = [rng.fr() for _ in range(5)]
    r, s = rng.fr(), rng.fr()
    z = oracle.synthetic_witness(nc, 91 + nc)
    w = zkp.Witness(z, 1)
    crs = zkp.CRS.generate_from_qap(ctx, qap, zkp.SetupParams(*params), 1, sound=True)
    full = crs.pk.upload(ctx)                                   # default options
    assert full.test_plan() == (13, 1)
    ctx.set_option(zkp.ZK_OPT_SOUND_COPIES, 3)
    dpk = _sound_device_key(zkp, ctx, qap, params, 1)
    up = crs.pk.upload(ctx)
    assert dpk.test_plan() == (3, 5) and up.test_plan() == (3, 5)
    want = zkp.Prover.prove(full, w, r=r, s=s)
    proof = zkp.Prover.prove(dpk, w, r=r, s=s)
    assert proof.serialize_compressed() == want.serialize_compressed()
    assert zkp.Prover.prove(up, w, r=r, s=s) == want
    dz = _device_z(w.assignment)
    assert zkp.Prover.prove_device(dpk, dz.data_ptr(), len(w.assignment), 1, r, s) == want
    x = [zkp.from_limbs(z[1])]
    assert zkp.Verifier.verify(crs.vk, proof, x) is True
    assert zkp.Verifier.verify(crs.vk, proof, [x[0] + 1]) is False
    assert _pairing_accepts(zkp, ctx, pyref, crs.vk, proof, x)
    for k in (full, dpk, up):
        k.free()


# --------------------------------------------------------------- key bases ---
def test_key_holds_the_copies_asked_for(zkp, ctx, case, qap4):
    """Copy w of a base is 2^c times copy w - 1 (public MSM) for every copy
    kept; the first one not kept cannot be read."""
    copies, c = 3, DEFAULT_C
    ctx.set_option(zkp.ZK_OPT_SOUND_COPIES, copies)
    dpk = _sound_device_key(zkp, ctx, qap4, case["params"], sound_ref.CASE_PUBLIC)
    assert dpk.test_info()[:2] == (13, c) and dpk.test_plan() == (3, 5)
    step = np.array([zkp.to_limbs(1 << c)], dtype=np.uint64)
    for slot, pick, g2 in ((SLOT_A, 0, False), (SLOT_A, -1, False), (SLOT_B2, -1, True), (SLOT_B2, 0, True),
                           (SLOT_H, 1, False), (SLOT_IC, 0, False)):
        prev = dpk.test_bases(slot, 0)[1][pick]
        assert not prev[-1]
        for w in range(1, copies):
            cur = dpk.test_bases(slot, w)[1][pick]
            assert np.array_equal(cur, (ctx.msm_g2 if g2 else ctx.msm_g1)(prev.reshape(1, -1), step, 255)), (slot, w)
            prev = cur
    for slot in (SLOT_A, SLOT_B2, SLOT_H):
        with pytest.raises(ValueError):
            dpk.test_bases(slot, copies)
    dpk.free()


# ------------------------------------------------------------ device bytes ---
def test_device_bytes_fall_with_the_copies(zkp, ctx, pyref):
    """A condition on the key, not a measurement: fewer copies, strictly fewer
    bytes, and the 12 copies between 13 and 1 are worth at least 10 times the
    one between 2 and 1 -- the CSR and index share (the same in every key)
    cannot hide a saving that is not there."""
    nc = 4096
    qap = zkp.QAP(zkp.CSRMatrices.synthetic(nc))
    rng = pyref.SplitMix64(0xB17E5)
    params = [rng.fr() for _ in range(5)]
    size = {}
    for copies in (0, 13, 4, 2, 1):
        ctx.set_option(zkp.ZK_OPT_SOUND_COPIES, copies)
        dpk = _sound_device_key(zkp, ctx, qap, params, 1)
        assert dpk.test_plan() == _sets(DEFAULT_C, copies or 13)
        size[copies] = dpk.device_bytes()
        dpk.free()
    assert size[0] == size[13]
    assert size[13] > size[4] > size[2] > size[1] > 0
    assert size[13] - size[1] >= 10 * (size[2] - size[1])
    # one copy: 128 B per G1 and 256 B per G2 point, about 8 G1 points' worth per constraint
    assert size[2] - size[1] >= 1000 * nc


# ---------------------------------------------------------- mode isolation ---
def test_reference_keys_ignore_the_option(zkp, ctx):
    toy = next(c for c in golden()["prove"] if c["name"] == "toy_xyz")
    qap = U.qap_from_case(zkp, toy)
    pk = U.pk_from_golden(zkp, toy, qap)
    before = pk.upload(ctx)
    info, plan, size = before.test_info(), before.test_plan(), before.device_bytes()
    before.free()
    ctx.set_option(zkp.ZK_OPT_SOUND_COPIES, 2)
    dpk = pk.upload(ctx)
    assert not dpk.sound
    assert dpk.test_info() == info and dpk.test_plan() == plan == (info[0], 1) and dpk.device_bytes() == size
    w = zkp.Witness(fr_rows(toy["z"]), toy["num_public"])
    proof = zkp.Prover.prove(dpk, w, r=int(toy["r"], 16), s=int(toy["s"], 16))
    assert list(proof.words) == proof_words(toy)
    assert proof.serialize_compressed().hex() == toy["proof_compressed"]
    dpk.free()


# ------------------------------------------------------ timing of the option ---
def test_option_governs_keys_made_after_it(zkp, ctx, case, qap4):
    want = sound_ref.proof_to_product(zkp, case["proof"])
    host_pk = sound_ref.pk_to_product(zkp, case["pk"], qap4)
    w = zkp.Witness(case["z"], sound_ref.CASE_PUBLIC)
    r, s = case["r"], case["s"]
    early = host_pk.upload(ctx)
    size = early.device_bytes()
    ctx.set_option(zkp.ZK_OPT_SOUND_COPIES, 2)
    assert early.test_plan() == (13, 1) and early.device_bytes() == size
    assert zkp.Prover.prove(early, w, r=r, s=s) == want
    late = host_pk.upload(ctx)
    assert late.test_plan() == (2, 7) and late.device_bytes() < size
    assert zkp.Prover.prove(late, w, r=r, s=s) == want
    assert zkp.Prover.prove(early, w, r=r, s=s) == want          # the two plans share the ctx's workspaces
    ctx.set_option(zkp.ZK_OPT_SOUND_COPIES, 0)
    assert late.test_plan() == (2, 7)
    assert zkp.Prover.prove(late, w, r=r, s=s) == want
    early.free()
    late.free()


# ------------------------------------------------------------------ errors ---
def test_option_errors(zkp, ctx):
    with pytest.raises(ValueError):
        ctx.set_option(zkp.ZK_OPT_SOUND_COPIES, -1)
    with pytest.raises(ValueError):
        ctx.set_option(11, 1)                                   # an unknown option still fails
    with pytest.raises(ValueError):
        ctx.set_option(zkp.ZK_OPT_SOUND_WIN_C, 18)
    ctx.set_option(zkp.ZK_OPT_SOUND_COPIES, 1 << 40)            # any count: clamps to the window count
