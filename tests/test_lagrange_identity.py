"""The identity LagrangeSRS.verify rests on, over Fr alone (no GPU): with L_i
the Lagrange basis of the size-n domain and c the inverse transform of rho
(zk_ntt_fr's root and 1 / n, here through the oracle's DFT),
    sum_i rho_i L_i(tau) = sum_k c_k tau^k
so the two MSMs of the check, over [L_i(tau)] and over [tau^k], meet in one
group element."""


def test_lagrange_combination_is_a_monomial_combination(pyref):
    R = pyref.R
    n = 8
    rng = pyref.SplitMix64(0x1A6)
    tau = rng.fr()
    rho = [((rng.next() << 64) | rng.next()) or 1 for _ in range(n)]
    w = pyref.root_of_unity(n)
    zt = (pow(tau, n, R) - 1) % R
    assert zt
    # L_i(tau) = Z(tau) w^i / (n (tau - w^i))
    L = [zt * pow(w, i, R) % R * pyref.fr_inv(n * (tau - pow(w, i, R))) % R for i in range(n)]
    assert sum(L) % R == 1
    # ... and it is the inverse transform of the powers: L_i = (1/n) sum_k w^(-ik) tau^k
    assert L == pyref.dft([pow(tau, k, R) for k in range(n)], n, inverse=True)
    c = pyref.dft(rho, n, inverse=True)
    assert sum(r * l for r, l in zip(rho, L)) % R == sum(ck * pow(tau, k, R) for k, ck in enumerate(c)) % R
    # a permuted basis does not satisfy it
    swapped = [L[0], L[2], L[1]] + L[3:]
    assert sum(r * l for r, l in zip(rho, swapped)) % R != sum(ck * pow(tau, k, R) for k, ck in enumerate(c)) % R
