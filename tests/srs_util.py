"""Shared by the tests of sound keys made from a powers-of-tau string
(test_gpu_setup_srs.py, test_gpu_walk_scale.py): key comparison, a CSR matrix
from per-row lists, and the parameters of sound_ref's shared case."""
import numpy as np

import sound_ref

PK_ARRAYS = ("a_g1", "b_g1", "b_g2", "ic_g1", "h_g1")
PK_POINTS = ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2")
VK_POINTS = ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2")


def same_crs(a, b):
    for nm in PK_ARRAYS:
        assert np.array_equal(getattr(a.pk, nm), getattr(b.pk, nm)), nm
    for nm in PK_POINTS:
        assert np.array_equal(a.pk.point(nm), b.pk.point(nm)), nm
    assert a.pk.num_public == b.pk.num_public and a.vk.num_public == b.vk.num_public
    assert np.array_equal(a.vk.ic_g1, b.vk.ic_g1)
    for nm in VK_POINTS:
        assert np.array_equal(a.vk.point(nm), b.vk.point(nm)), nm


def csr(rows, nc):
    """rows: per constraint a list of (col, coeff), duplicates kept"""
    rp, cols, vals = [0], [], []
    for i in range(nc):
        for c, v in rows[i]:
            cols.append(c)
            vals.append([(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)])
        rp.append(len(cols))
    return (np.array(rp, dtype=np.uint64), np.array(cols, dtype=np.uint32),
            np.array(vals, dtype=np.uint64).reshape(-1, 4))


def case4(pyref):
    """the parameters, witness and blinding of sound_ref's shared case (n = 4)"""
    rng = pyref.SplitMix64(sound_ref.CASE_SEED)
    alpha, beta, _, _, tau = (rng.fr() for _ in range(5))
    r, s = rng.fr(), rng.fr()
    return {"alpha": alpha, "beta": beta, "tau": tau, "r": r, "s": s,
            "z": pyref.synthetic_witness(sound_ref.CASE_N, sound_ref.CASE_SEED + 1)}


def trusted(zkp, ctx, qap, case, num_public):
    """the sound setup for (alpha, beta, 1, 1, tau): what from_srs must give"""
    params = zkp.SetupParams(case["alpha"], case["beta"], 1, 1, case["tau"])
    return zkp.CRS.generate_from_qap(ctx, qap, params, num_public, sound=True)


def string(zkp, ctx, case, log_n):
    return zkp.SRS.generate(ctx, log_n, case["tau"], case["alpha"], case["beta"])
