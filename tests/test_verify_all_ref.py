"""verify_all_ref.batch_equation_holds -- the reference the GPU tests of the
sound batch check compare with -- pinned without a GPU on the sound product of
tests/sound_ref.py: a valid proof accepts, a proof with another proof's C
rejects, and the swapped pair accepts with equal coefficients and rejects with
distinct ones, which is why the coefficients must be random."""
import numpy as np
import pytest

import sound_ref
import verify_all_ref as VR

C1, C2 = 0x9E3779B97F4A7C15F39CC0605CEDC835, (1 << 128) - 1


@pytest.fixture(scope="module")
def product(zkp):
    """(vk, p1, p2, inputs): two proofs of the same statement under the shared case's key"""
    case = sound_ref.build_case()
    rng = sound_ref.P.SplitMix64(0xA11)
    other = sound_ref.prove_sound(case["pk"], case["qap"], case["z"], sound_ref.CASE_PUBLIC, rng.fr(), rng.fr())
    vk = sound_ref.vk_to_product(zkp, case["vk"])
    p1, p2 = sound_ref.proof_to_product(zkp, case["proof"]), sound_ref.proof_to_product(zkp, other)
    assert not np.array_equal(p1.c, p2.c)
    return vk, p1, p2, [case["z"][1]]


def _swapped(zkp, p1, p2):
    """(A1, B1, C2) and (A2, B2, C1): the defects e(C1 - C2, delta) and its inverse"""
    return (zkp.Proof(np.concatenate([p1.a, p1.b, p2.c])), zkp.Proof(np.concatenate([p2.a, p2.b, p1.c])))


def test_a_valid_proof_accepts(zkp, pyref, product):
    vk, p1, p2, x = product
    assert zkp.Verifier.verify(vk, p1, x) and zkp.Verifier.verify(vk, p2, x)
    for c in (1, C1, C2):
        assert VR.batch_equation_holds(zkp, pyref, vk, [p1], [x], [c])
    assert VR.batch_equation_holds(zkp, pyref, vk, [p1, p2], [x, x], [C1, C2])


def test_another_proofs_c_rejects(zkp, pyref, product):
    vk, p1, p2, x = product
    mixed, _ = _swapped(zkp, p1, p2)
    assert not zkp.Verifier.verify(vk, mixed, x)
    for c in (1, C1, C2):
        assert not VR.batch_equation_holds(zkp, pyref, vk, [mixed], [x], [c])
    assert not VR.batch_equation_holds(zkp, pyref, vk, [p1, mixed], [x, x], [C1, C2])
    assert not VR.batch_equation_holds(zkp, pyref, vk, [p1], [[x[0] + (1 << 64)]], [C1])


def test_the_swapped_pair_needs_distinct_coefficients(zkp, pyref, product):
    vk, p1, p2, x = product
    pair = list(_swapped(zkp, p1, p2))
    assert not zkp.Verifier.verify(vk, pair[0], x) and not zkp.Verifier.verify(vk, pair[1], x)
    assert VR.batch_equation_holds(zkp, pyref, vk, pair, [x, x], [C1, C1])
    assert VR.batch_equation_holds(zkp, pyref, vk, pair, [x, x], [1, 1])
    assert not VR.batch_equation_holds(zkp, pyref, vk, pair, [x, x], [C1, C2])
    assert not VR.batch_equation_holds(zkp, pyref, vk, pair, [x, x], [1, 2])
