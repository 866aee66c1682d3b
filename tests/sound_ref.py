"""Sound-mode reference: textbook Groth16 in the reference's arrangement of
pi_C, nothing truncated -- the formulas of include/zkp.h ("sound mode")
restated over pyref's QAP, poly_eval, G1 / G2, fr_inv and SplitMix64.  The
oracle mirrors the reference (lo64 scalars, no Z(tau) in h_g1), so this lives
beside the tests instead.

With l = num_public, n the domain size, Z(tau) = tau^n - 1:
  a_g1[i] = [A_i(tau)]_1, b_g1[i] = [B_i(tau)]_1, b_g2[i] = [B_i(tau)]_2     i < V
  pk ic_g1[i-l-1] = [(beta A_i + alpha B_i + C_i)(tau) / delta]_1            l < i < V
  vk ic_g1[i]     = [(beta A_i + alpha B_i + C_i)(tau) / gamma]_1            i <= l
  h_g1[i] = [tau^i Z(tau) / delta]_1                                          i < n
  pi_A = alpha_1 + sum z_i a_g1[i] + r delta_1
  pi_B = beta_2 + sum z_i b_g2[i] + s delta_2,   B_1 = beta_1 + sum z_i b_g1[i]
  pi_C = sum_{i>l} z_i ic_g1[i-l-1] + sum H_i h_g1[i] + s pi_A + r B_1
  IC   = ic_g1[0] + sum x_i ic_g1[i+1]
A full-width pyref scalar multiplication costs ~0.13 s: use the synthetic
circuit n = 4 (V = 13), nothing larger."""
import numpy as np
import pyref as P

R = P.R


class SetupError(Exception):
    pass


def setup_sound(qap, params, num_public):
    """params = (alpha, beta, gamma, delta, tau), whole Fr values -> (pk, vk)
    dicts of pyref affine points, laid out like pyref.generate_from_qap."""
    alpha, beta, gamma, delta, tau = (x % R for x in params)
    if 0 in (alpha, beta, gamma, delta):
        raise SetupError("Setup parameters must be non-zero")
    V, n = qap.num_variables, qap.n
    if num_public >= V:
        raise SetupError("num_public")
    zt = (pow(tau, n, R) - 1) % R
    if zt == 0:
        raise SetupError("tau on the evaluation domain")
    g1, g2 = P.G1.gen, P.G2.gen
    av = [P.poly_eval(p, tau) for p in qap.polys[0]]
    bv = [P.poly_eval(p, tau) for p in qap.polys[1]]
    cv = [P.poly_eval(p, tau) for p in qap.polys[2]]
    dinv, ginv = P.fr_inv(delta), P.fr_inv(gamma)
    mix = [(beta * av[i] + alpha * bv[i] + cv[i]) % R for i in range(V)]
    pk = {
        "alpha_g1": P.G1.mul(g1, alpha), "beta_g1": P.G1.mul(g1, beta), "delta_g1": P.G1.mul(g1, delta),
        "beta_g2": P.G2.mul(g2, beta), "delta_g2": P.G2.mul(g2, delta),
        "a_g1": [P.G1.mul(g1, a) for a in av],
        "b_g1": [P.G1.mul(g1, b) for b in bv],
        "b_g2": [P.G2.mul(g2, b) for b in bv],
        "ic_g1": [P.G1.mul(g1, mix[i] * dinv % R) for i in range(num_public + 1, V)],
        "h_g1": [P.G1.mul(g1, pow(tau, i, R) * zt % R * dinv % R) for i in range(n)],
        "num_public": num_public,
    }
    vk = {
        "alpha_g1": pk["alpha_g1"], "beta_g2": pk["beta_g2"], "gamma_g2": P.G2.mul(g2, gamma),
        "delta_g2": pk["delta_g2"],
        "ic_g1": [P.G1.mul(g1, mix[i] * ginv % R) for i in range(num_public + 1)],
        "num_public": num_public,
    }
    return pk, vk


def prove_sound(pk, qap, z, num_public, r, s):
    """-> (pi_A, pi_B, pi_C) as pyref affine points; z satisfies the circuit."""
    z = [x % R for x in z]
    assert z[0] == 1 and len(z) == qap.num_variables and num_public < len(z)
    h = qap.compute_quotient_polynomial(z)          # (A B - C) / (x^n - 1), whole
    assert len(h) <= qap.n - 1
    pi_a = P.G1.msm([(1, pk["alpha_g1"])] + [(zi, pk["a_g1"][i]) for i, zi in enumerate(z) if zi] +
                    [(r, pk["delta_g1"])])
    pi_b = P.G2.msm([(1, pk["beta_g2"])] + [(zi, pk["b_g2"][i]) for i, zi in enumerate(z) if zi] +
                    [(s, pk["delta_g2"])])
    b1 = P.G1.msm([(1, pk["beta_g1"])] + [(zi, pk["b_g1"][i]) for i, zi in enumerate(z) if zi])
    c_terms = [(z[i], pk["ic_g1"][i - num_public - 1]) for i in range(num_public + 1, len(z)) if z[i]]
    c_terms += [(c, pk["h_g1"][i]) for i, c in enumerate(h) if c]
    c_terms += [(s, pi_a), (r, b1)]
    return pi_a, pi_b, P.G1.msm(c_terms)


def ic_sound(vk, inputs):
    """IC = ic_g1[0] + sum x_i ic_g1[i+1] with the whole x_i (a pyref point)."""
    assert len(inputs) == vk["num_public"]
    return P.G1.msm([(1, vk["ic_g1"][0])] + [(x % R, vk["ic_g1"][i + 1]) for i, x in enumerate(inputs) if x % R])


# ---- layout conversions to the product's host keys and proofs ----------------
def pk_to_product(zkp, pk, qap_product, sound=True):
    """A sound_ref / pyref pk dict -> zkp.ProvingKey holding the same points."""
    out = zkp.ProvingKey(qap_product.num_variables, qap_product.domain_size, pk["num_public"], qap_product, sound)
    for nm in ("a_g1", "b_g1", "ic_g1", "h_g1"):
        if len(pk[nm]):
            getattr(out, nm)[:] = [P.g1_words(p) for p in pk[nm]]
    out.b_g2[:] = [P.g2_words(p) for p in pk["b_g2"]]
    for nm in ("alpha_g1", "beta_g1", "delta_g1"):
        for i, w in enumerate(P.g1_words(pk[nm])):
            getattr(out.s, nm).w[i] = w
    for nm in ("beta_g2", "delta_g2"):
        for i, w in enumerate(P.g2_words(pk[nm])):
            getattr(out.s, nm).w[i] = w
    return out


def vk_to_product(zkp, vk, sound=True):
    return zkp.VerificationKey.from_points(P.g1_words(vk["alpha_g1"]), P.g2_words(vk["beta_g2"]),
                                           P.g2_words(vk["gamma_g2"]), P.g2_words(vk["delta_g2"]),
                                           [P.g1_words(p) for p in vk["ic_g1"]], sound=sound)


def proof_to_product(zkp, proof):
    a, b, c = proof
    return zkp.Proof(np.array(P.g1_words(a) + P.g2_words(b) + P.g1_words(c), dtype=np.uint64))


# ---- the one shared case: synthetic n = 4, num_public = 1, whole parameters ----
CASE_N, CASE_PUBLIC, CASE_SEED = 4, 1, 0x50D1


def build_case():
    """{params, r, s, z, qap, pk, vk, proof}: built once per test module
    (about 60 non-zero full-width pyref multiplications, a few seconds)."""
    rng = P.SplitMix64(CASE_SEED)
    params = tuple(rng.fr() for _ in range(5))
    r, s = rng.fr(), rng.fr()
    qap = P.QAP(P.synthetic_r1cs(CASE_N))
    z = P.synthetic_witness(CASE_N, CASE_SEED + 1)
    pk, vk = setup_sound(qap, params, CASE_PUBLIC)
    proof = prove_sound(pk, qap, z, CASE_PUBLIC, r, s)
    return {"params": params, "r": r, "s": s, "z": z, "qap": qap, "pk": pk, "vk": vk, "proof": proof}
