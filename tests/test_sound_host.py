"""Sound mode on the host (no GPU): zk_groth16_verify_sound against the
sound_ref key and proof (synthetic n = 4, whole parameters), the reference
mode's verdict on the same proof, and the sound key files."""
import numpy as np
import pytest

import sound_ref

TWO64 = 1 << 64


@pytest.fixture(scope="module")
def case():
    return sound_ref.build_case()


@pytest.fixture(scope="module")
def product(zkp, case):
    """(vk, proof, inputs) of the case in the product's layouts."""
    vk = sound_ref.vk_to_product(zkp, case["vk"])
    proof = sound_ref.proof_to_product(zkp, case["proof"])
    return vk, proof, [case["z"][1]]


def test_case_inputs_are_whole(case):
    """The case means something only with scalars past 64 bits everywhere."""
    assert all(p >= TWO64 for p in case["params"]) and case["z"][1] >= TWO64
    assert case["z"][1] + TWO64 < sound_ref.R


def test_verify_sound_accepts_the_reference_proof(zkp, product):
    vk, proof, inputs = product
    assert vk.sound
    assert zkp.Verifier.verify(vk, proof, inputs) is True


def test_reference_proof_satisfies_the_pairing_equation(zkp, pyref, case, product):
    """The same verdict without the new verify code: IC from pyref, then the
    host pairing product e(A,B) e(-alpha,beta) e(-IC,gamma) e(-C,delta)."""
    vk, proof, inputs = product
    neg = pyref.G1.neg
    ic = sound_ref.ic_sound(case["vk"], inputs)
    g1 = [pyref.g1_words(p) for p in (case["proof"][0], neg(case["vk"]["alpha_g1"]), neg(ic), neg(case["proof"][2]))]
    g2 = [proof.b, vk.point("beta_g2"), vk.point("gamma_g2"), vk.point("delta_g2")]
    assert zkp.pairing_product_is_one(g1, g2)


def test_verify_sound_sees_the_upper_limbs(zkp, product):
    """x + 2^64 differs from x in limb 1 only: the case the reference-mode
    verifier cannot tell apart."""
    vk, proof, inputs = product
    assert zkp.Verifier.verify(vk, proof, [inputs[0] + TWO64]) is False


def test_verify_sound_rejects_an_input_not_below_r(zkp, product):
    vk, proof, _ = product
    bad = np.array([zkp.to_limbs(sound_ref.R)], dtype=np.uint64)          # r itself
    with pytest.raises(ValueError):
        zkp.Verifier.verify(vk, proof, bad)
    valid = zkp.C.c_int(7)
    rc = zkp.lib().zk_groth16_verify_sound(zkp.C.byref(vk.s), zkp.C.byref(proof._c()), zkp._p(bad), zkp.C.c_size_t(1),
                                           zkp.C.byref(valid))
    assert rc == zkp.ZK_ERR_ARG and valid.value == 0
    top = np.array([[0xFFFFFFFFFFFFFFFF] * 4], dtype=np.uint64)
    with pytest.raises(ValueError):
        zkp.Verifier.verify(vk, proof, top)


def test_verify_sound_wrong_input_count(zkp, product):
    vk, proof, inputs = product
    with pytest.raises(zkp.InvalidWitness):
        zkp.Verifier.verify(vk, proof, inputs + [5])
    with pytest.raises(zkp.InvalidWitness):
        zkp.Verifier.verify(vk, proof, [])


def test_reference_mode_on_the_same_proof(zkp, case, product):
    """zk_groth16_verify (reference mode: lo64 of the input) on the sound
    proof and vk: False, as run on the parent commit -- the truncated IC is
    another point, so the pairing product is not 1."""
    _, proof, inputs = product
    ref_vk = sound_ref.vk_to_product(zkp, case["vk"], sound=False)
    assert not ref_vk.sound
    assert zkp.Verifier.verify(ref_vk, proof, inputs) is False


def test_batch_verifier_is_reference_only(zkp, product):
    vk, proof, inputs = product
    with pytest.raises(ValueError):
        zkp.BatchVerifier.verify_batch(vk, [(proof, inputs)], coeffs=[1])


def _assert_same_pk(a, b):
    for nm in ("a_g1", "b_g1", "b_g2", "ic_g1", "h_g1"):
        assert np.array_equal(getattr(a, nm), getattr(b, nm)), nm
    for nm in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2"):
        assert np.array_equal(a.point(nm), b.point(nm)), nm
    assert a.num_public == b.num_public


def test_sound_key_files_round_trip(zkp, case, product, tmp_path):
    """ZKAMDPS1 / ZKAMDVS1 keep .sound and every byte of the points; the
    compressed ZKAMDPS2 / ZKAMDVS2 files are the ZKAMDPK2 / ZKAMDVK2 bytes
    under the other magic (loading one decompresses on the GPU:
    test_gpu_sound.py)."""
    vk = product[0]
    qap = zkp.QAP(zkp.CSRMatrices.synthetic(sound_ref.CASE_N))
    pk = sound_ref.pk_to_product(zkp, case["pk"], qap)
    assert pk.sound
    zkp.save_proving_key(pk, tmp_path / "pk.bin")
    assert open(tmp_path / "pk.bin", "rb").read(8) == b"ZKAMDPS1"
    back = zkp.load_proving_key(tmp_path / "pk.bin")
    assert back.sound is True
    _assert_same_pk(back, pk)
    zkp.save_verification_key(vk, tmp_path / "vk.bin")
    assert open(tmp_path / "vk.bin", "rb").read(8) == b"ZKAMDVS1"
    vb = zkp.load_verification_key(tmp_path / "vk.bin")
    assert vb.sound is True and vb.num_public == vk.num_public and np.array_equal(vb.ic_g1, vk.ic_g1)
    for nm in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2"):
        assert np.array_equal(vb.point(nm), vk.point(nm))
    assert zkp.Verifier.verify(vb, product[1], product[2]) is True
    # compressed: the same layout as the reference-mode files, another magic
    for key, save, smagic, rmagic in ((pk, zkp.save_proving_key, b"ZKAMDPS2", b"ZKAMDPK2"),
                                      (vk, zkp.save_verification_key, b"ZKAMDVS2", b"ZKAMDVK2")):
        save(key, tmp_path / "s.bin", compressed=True)
        key.sound = False
        save(key, tmp_path / "r.bin", compressed=True)
        key.sound = True
        sb, rb = open(tmp_path / "s.bin", "rb").read(), open(tmp_path / "r.bin", "rb").read()
        assert sb[:8] == smagic and rb[:8] == rmagic and sb[8:] == rb[8:]


def test_reference_key_files_stay_reference(zkp, case, tmp_path):
    """A ZKAMDPK1 / ZKAMDVK1 file still loads with sound == False, and its
    bytes do not depend on this feature."""
    qap = zkp.QAP(zkp.CSRMatrices.synthetic(sound_ref.CASE_N))
    pk = sound_ref.pk_to_product(zkp, case["pk"], qap, sound=False)
    zkp.save_proving_key(pk, tmp_path / "pk.bin")
    assert open(tmp_path / "pk.bin", "rb").read(8) == b"ZKAMDPK1"
    back = zkp.load_proving_key(tmp_path / "pk.bin")
    assert back.sound is False
    _assert_same_pk(back, pk)
    vk = sound_ref.vk_to_product(zkp, case["vk"], sound=False)
    zkp.save_verification_key(vk, tmp_path / "vk.bin")
    assert open(tmp_path / "vk.bin", "rb").read(8) == b"ZKAMDVK1"
    assert zkp.load_verification_key(tmp_path / "vk.bin").sound is False
    with open(tmp_path / "junk.bin", "wb") as f:
        f.write(b"ZKAMDPS3" + bytes(72))
    with pytest.raises(ValueError):
        zkp.load_proving_key(tmp_path / "junk.bin")
