"""Big-integer model of the coefficient side of CRS.verify_against_srs
(csrc/keycheck.hip; include/zkp.h, "a key against its string"), and the six
identities of that call checked IN THE EXPONENT for known tau, alpha, beta,
delta -- no curve arithmetic, so it runs anywhere.

A circuit here is (mats, V): mats = [A, B, C], each a list of rows, a row a
list of (col, coeff) with duplicates kept (they add).  With l = num_public, n
the domain and w pyref's root of unity of order n:
  u^{M,part}_j = sum_i M[j][i] rho^part_i      rho^pub keeps i <= l, rho^priv i > l
  m^{M,part}   = iNTT_n(u^{M,part})            coefficients of sum_i rho^part_i M_i(x)
coeff_vectors gives the six m in the order A pub, A priv, B pub, B priv,
C pub, C priv -- what zk_test_key_srs_coeffs returns.  The key's side of every
identity is built another way: column by column, M_i(x) interpolated from the
column's values (duplicates summed) and evaluated at tau, as sound_ref does."""
import pyref as P

R = P.R


def domain_size(nc):
    n = 1
    while n < nc:
        n <<= 1
    return n


def split_products(mats, V, l, rho, n):
    """-> [u^{A,pub}, u^{A,priv}, u^{B,pub}, ...], each n values (padded rows 0)"""
    out = []
    for rows in mats:
        pub, priv = [0] * n, [0] * n
        for j, row in enumerate(rows):
            for c, v in row:
                if c >= V:
                    continue
                if c <= l:
                    pub[j] = (pub[j] + v * rho[c]) % R
                else:
                    priv[j] = (priv[j] + v * rho[c]) % R
        out += [pub, priv]
    return out


def intt_naive(u):
    """m_k = (1 / n) sum_j u_j w^(-j k), by the definition"""
    n = len(u)
    winv = P.fr_inv(P.root_of_unity(n))
    pw = [pow(winv, e, R) for e in range(n)]
    ninv = P.fr_inv(n)
    return [sum(u[j] * pw[j * k % n] for j in range(n)) % R * ninv % R for k in range(n)]


def intt_fast(u):
    """the same by radix-2 splitting (the 512-point cases of the GPU tests);
    test_key_srs_ref.py holds it to intt_naive"""
    n = len(u)
    winv = P.fr_inv(P.root_of_unity(n))

    def rec(x, w):
        if len(x) == 1:
            return x
        ev, od = rec(x[0::2], w * w % R), rec(x[1::2], w * w % R)
        h, out, t = len(x) // 2, [0] * len(x), 1
        for k in range(h):
            out[k], out[k + h] = (ev[k] + t * od[k]) % R, (ev[k] - t * od[k]) % R
            t = t * w % R
        return out

    ninv = P.fr_inv(n)
    return [x * ninv % R for x in rec([x % R for x in u], winv)]


def coeff_vectors(mats, V, l, rho, intt=intt_naive):
    nc = len(mats[0])
    return [intt(u) for u in split_products(mats, V, l, rho, domain_size(nc))]


def h_scalars(sigma):
    """d_k, k < 2 n: sum_k d_k tau^k = sum_i sigma_i tau^i (tau^n - 1)"""
    return [(R - s) % R for s in sigma] + [s % R for s in sigma]


def column_values(rows, V, n, tau):
    """[M_i(tau)], i < V: each column interpolated on the domain, then evaluated"""
    cols = [[0] * n for _ in range(V)]
    for j, row in enumerate(rows):
        for c, v in row:
            if c < V:
                cols[c][j] = (cols[c][j] + v) % R
    return [P.poly_eval(intt_naive(col), tau) for col in cols]


def _at(coeffs, tau):
    return P.poly_eval(coeffs, tau)


def identities(mats, V, l, rho, sigma, tau, alpha, beta, delta):
    """{name: (key side, string side)} as exponents; an honest key has both equal.
    The key side follows DESIGN.md 2.12 (gamma = 1): a_i = A_i(tau), ..., pk ic_i =
    (beta A_i + alpha B_i + C_i)(tau) / delta, h_i = tau^i (tau^n - 1) / delta; the
    pairing with delta_2 multiplies the last two by delta again."""
    n = domain_size(len(mats[0]))
    assert len(rho) == V and len(sigma) == n and l < V
    av, bv, cv = (column_values(m, V, n, tau) for m in mats)
    mix = [(beta * av[i] + alpha * bv[i] + cv[i]) % R for i in range(V)]
    dinv = P.fr_inv(delta)
    zt = (pow(tau, n, R) - 1) % R
    h = [pow(tau, i, R) * zt % R * dinv % R for i in range(n)]
    m = coeff_vectors(mats, V, l, rho)
    whole = [[(m[2 * k][i] + m[2 * k + 1][i]) % R for i in range(n)] for k in range(3)]
    t = [(beta * _at(m[0 + p], tau) + alpha * _at(m[2 + p], tau) + _at(m[4 + p], tau)) % R for p in range(2)]
    dot = lambda xs, ys: sum(x * y for x, y in zip(xs, ys)) % R
    return {
        "QUERY_A": (dot(rho, av), _at(whole[0], tau)),
        "QUERY_B": (dot(rho, bv), _at(whole[1], tau)),
        "IC_VK": (dot(rho[:l + 1], mix[:l + 1]), t[0]),
        "IC_PK": (dot(rho[l + 1:], [x * dinv % R for x in mix[l + 1:]]) * delta % R, t[1]),
        "H": (dot(sigma, h) * delta % R, _at(h_scalars(sigma), tau)),
    }


# ------------------------------------------------------------- circuits ---
def synthetic_rows(nc):
    """pyref.synthetic_r1cs as rows: constraint i is z_{3i+1} z_{3i+2} = z_{3i+3}"""
    return [[[(3 * i + 1 + m, 1)] for i in range(nc)] for m in range(3)], 3 * nc + 1


def handmade5():
    """5 constraints (n = 8, 3 padded rows), 7 variables: variable 4 only as a
    pair 5, r - 5 on one (row, col) of A -- it cancels --, variable 5 nowhere,
    two full-width coefficients, a pair that adds (C row 3)."""
    rng = P.SplitMix64(0x5C1)
    wide, wide2 = rng.fr(), rng.fr()
    assert wide >> 200 and wide2 >> 200
    A = [[(0, 1), (1, 2)], [(1, 1), (2, R - 1)], [(3, wide)], [(4, 5), (4, R - 5), (1, 3)], [(2, 1), (3, 1)]]
    B = [[(2, 1)], [(0, 1)], [(1, wide2)], [(3, 2)], [(6, 1), (0, R - 1)]]
    C = [[(3, 1)], [(6, 1)], [(2, 7)], [(1, 1), (1, 1)], [(6, 3)]]
    return [A, B, C], 7


def handmade300():
    """test_gpu_setup_srs.py's circuit: 300 constraints (n = 512, 212 padded
    rows), 12 variables; variable 0 in every row of A and C, coefficients 1,
    r - 1, 2 and a full-width one, variable 7 only in B, variable 8 only as a
    cancelling pair, variable 9 as a pair that adds."""
    rng = P.SplitMix64(0x300)
    wide = rng.fr()
    assert wide >> 200
    coef = [1, R - 1, 2, wide]
    nc = 300
    A = [[(0, 1), (1 + i % 5, coef[i % 4])] for i in range(nc)]
    A[10] += [(8, 5), (8, R - 5)]
    A[11] += [(9, 5), (9, 3)]
    B = [[(2 + i % 6, coef[(i + 1) % 4])] for i in range(nc)]
    B[7].append((7, wide))
    C = [[(0, 1), (3 + i % 8, rng.fr() if i % 16 == 0 else coef[(i + 2) % 4])] for i in range(nc)]
    return [A, B, C], 12


def coefficients(count, seed=0x6B5):
    """count pairwise distinct values in [1, 2^128), 1 and 2^128 - 1 among them"""
    rng = P.SplitMix64(seed)
    out = [1, (1 << 128) - 1][:count]
    while len(out) < count:
        c = (rng.next() << 64) | rng.next()
        if c and c not in out:
            out.append(c)
    return out
