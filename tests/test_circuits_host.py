"""The general-circuit builder (tests/circuits.py) holds the cases the GPU
tests of test_gpu_general_circuits.py rely on.  Conditions on the builder and
on the oracle's key, no GPU: if an edit to the builder loses a case, this
fails instead of the GPU tests passing on less."""
import numpy as np
import pytest

import circuits as CZ

R = CZ.R
SEED = 0x6E0


@pytest.fixture(scope="module", params=CZ.SHAPES, ids=lambda s: "%dx%d_pub%d" % s)
def circ(request):
    nc, V, num_public = request.param
    return CZ.general_circuit(nc, V, num_public, SEED + nc)


@pytest.fixture(scope="module")
def okey(circ, oracle, pyref):
    rng = pyref.SplitMix64(SEED + 1)
    csr = oracle.CSR(circ.nc, circ.V, circ.mats)
    rc, opk, ovk = oracle.setup(csr, [rng.fr() for _ in range(5)], circ.num_public, nthreads=oracle.default_threads())
    assert rc == 0
    return csr, opk, ovk


def _identity(words):
    return bool(words[-1] == 1)


def test_witness_satisfies(circ, oracle):
    assert circ.z_int[0] == 1 and all(0 < v < R for v in circ.z_int)
    for j in range(circ.nc):
        a, b, c = circ.row_values(j)
        assert a * b % R == c, j
    csr = oracle.CSR(circ.nc, circ.V, circ.mats)
    assert oracle.validate(csr, circ.z) == 0
    rc, _ = oracle.quotient(csr, circ.z)
    assert rc == 0


def test_deterministic(circ):
    again = CZ.general_circuit(circ.nc, circ.V, circ.num_public, SEED + circ.nc)
    for (rp, col, val), (rp2, col2, val2) in zip(circ.mats, again.mats):
        assert np.array_equal(rp, rp2) and np.array_equal(col, col2) and np.array_equal(val, val2)
    assert np.array_equal(circ.z, again.z)


def test_csr_arrays(circ):
    for m, (rp, col, val) in enumerate(circ.mats):
        assert rp.dtype == np.uint64 and col.dtype == np.uint32 and val.dtype == np.uint64
        assert len(rp) == circ.nc + 1 and rp[0] == 0 and rp[-1] == len(col) == len(val)
        assert [int(x) for x in np.diff(rp.astype(np.int64))] == [len(r) for r in circ.rows[m]]
    assert circ.domain == {1000: 1024, 300: 512, 4097: 8192}[circ.nc]


def test_row_lengths(circ):
    nc, V = circ.nc, circ.V
    la, lb, lc = ([len(r) for r in circ.rows[m]] for m in range(3))
    base = set()
    for j in range(nc):
        extra = 2 * (j % CZ.CANCEL_EVERY == 0) + 2 * (j in (CZ.CANCEL_ROW, CZ.DUPLICATE_ROW))
        if j % CZ.EMPTY_EVERY == 0:
            assert la[j] == 0, j
        elif j % CZ.LONG_EVERY == 0:
            assert la[j] == CZ.LONG_LEN + extra, j
        else:
            assert 1 <= la[j] - extra <= 3, j
            base.add(la[j] - extra)
        assert 1 <= lb[j] - (j % CZ.DROPPED_EVERY == 0) <= 2, j
        assert 1 <= lc[j] <= 3, j
    assert base == {1, 2, 3} and set(lc) == {1, 2, 3}
    assert {l - (j % CZ.DROPPED_EVERY == 0) for j, l in enumerate(lb)} == {1, 2}
    assert la.count(0) == (nc + CZ.EMPTY_EVERY - 1) // CZ.EMPTY_EVERY
    long_rows = [j for j in range(nc) if j % CZ.LONG_EVERY == 0 and j % CZ.EMPTY_EVERY]
    assert len(long_rows) >= 3
    # an empty row and a 40-entry row share a wave with rows of 1..3 entries
    assert max(la[64:128]) >= CZ.LONG_LEN and min(la[64:128]) == 0
    # rows nc <= j < n exist: the domain is padded
    assert circ.domain > nc


def test_coefficients(circ):
    vals = {v for m in range(3) for row in circ.rows[m] for _, v in row}
    assert {1, R - 1, 2} <= vals
    assert sum(1 for v in vals if v >> 200) > circ.nc // 8      # full-width draws
    assert all(0 <= v < R for v in vals)


def test_columns(circ):
    nc, V = circ.nc, circ.V
    A, B, C = circ.rows
    # the long column: variable 0 leads every second non-empty A row
    zero_rows = [j for j in range(nc) if any(c == 0 for c, _ in A[j])]
    assert {j for j in range(0, nc, 2) if j % CZ.EMPTY_EVERY} <= set(zero_rows)
    assert len(zero_rows) > nc * 0.45 and len(zero_rows) > 64
    # the out-of-range column ends every 11th B row and is nowhere else
    over = [(m, j) for m in range(3) for j in range(nc) for c, _ in circ.rows[m][j] if c >= V]
    assert over == [(1, j) for j in range(0, nc, CZ.DROPPED_EVERY)]
    assert all(B[j][-1][0] == V + 5 for j in range(0, nc, CZ.DROPPED_EVERY))
    # the cancelling duplicate ends every 13th non-empty A row
    for j in range(0, nc, CZ.CANCEL_EVERY):
        if j % CZ.EMPTY_EVERY:
            assert A[j][-2:] == [(3, 5), (3, R - 5)], j


def test_special_variables(circ):
    V = circ.V
    assert circ.rows_naming(circ.unreferenced) == []
    # the cancelling variable: one (row, col) of A, the pair 5, r - 5
    assert circ.rows_naming(circ.cancelling) == [CZ.CANCEL_ROW]
    assert [v for c, v in circ.rows[0][CZ.CANCEL_ROW] if c == circ.cancelling] == [5, R - 5]
    assert circ.column_sums(circ.cancelling) == [{CZ.CANCEL_ROW: 0}, {}, {}]
    # the duplicate-only variable: one (row, col) of A, the pair 5, 3
    assert circ.rows_naming(circ.duplicate) == [CZ.DUPLICATE_ROW]
    assert [v for c, v in circ.rows[0][CZ.DUPLICATE_ROW] if c == circ.duplicate] == [5, 3]
    assert circ.column_sums(circ.duplicate) == [{CZ.DUPLICATE_ROW: 8}, {}, {}]
    assert (circ.unreferenced, circ.cancelling, circ.duplicate) == (V - 3, V - 2, V - 1)
    # the variables of the verdict tests
    r1 = circ.rows_naming(circ.shared_row1)
    assert 1 in r1 and len(r1) >= 4
    rl = circ.rows_naming(circ.shared_last)
    assert 1 not in rl and circ.nc - 1 in rl and len(rl) >= 4
    # a variable named from rows of several ranks of a distributed quotient
    for N in (2, 4, 8):
        m = circ.domain // N
        assert len({(j % m) // (m // N) for j in circ.rows_naming(0)}) == N
    # variables no row names are many where V outruns the rows
    named = {c for m in range(3) for row in circ.rows[m] for c, _ in row}
    if V > 3 * circ.nc:
        assert len(set(range(V)) - named) > V // 2


def test_unit_b_variant(oracle):
    nc, V, num_public = CZ.SHAPES[1]
    circ = CZ.general_circuit(nc, V, num_public, SEED + nc, unit_b=True)
    assert circ.mats[1][2] is None and circ.mats[0][2] is not None and circ.mats[2][2] is not None
    assert any(c >= V for c in circ.mats[1][1])
    for j in range(nc):
        a, b, c = circ.row_values(j)
        assert a * b % R == c, j
    assert oracle.validate(oracle.CSR(nc, V, circ.mats), circ.z) == 0


def test_oracle_key_identities(circ, okey):
    """In the oracle's key the unreferenced and the cancelling variable have
    identity bases everywhere, the duplicate-only variable does not, and the
    kept set of every vector is irregular (no fixed period)."""
    _, opk, _ = okey
    for v in (circ.unreferenced, circ.cancelling):
        assert _identity(opk.a_g1[v]) and _identity(opk.b_g1[v]) and _identity(opk.b_g2[v]), v
    assert not _identity(opk.a_g1[circ.duplicate])
    assert not _identity(opk.a_g1[0])
    for nm in ("a_g1", "b_g1", "b_g2"):
        ident = getattr(opk, nm)[:, -1] == 1
        assert ident.any() and not ident.all(), nm
        gaps = np.diff(np.flatnonzero(ident))
        assert len(set(gaps.tolist())) > 2, nm
    assert not (opk.h_g1[:, -1] == 1).any()


def test_oracle_verdicts(circ, okey, oracle, pyref):
    """What the GPU verdict tests compare with: the oracle rejects a broken
    shared_row1 as an invalid witness, a broken shared_last in the division,
    z_0 = 2 as an invalid witness."""
    csr, opk, _ = okey
    rng = pyref.SplitMix64(SEED + 2)
    r, s = rng.fr(), rng.fr()
    assert oracle.prove(opk, csr, circ.z, circ.num_public, r, s)[0] == oracle.OR_OK
    for var, value, want in ((circ.shared_row1, (circ.z_int[circ.shared_row1] + 1) % R, oracle.OR_ERR_INVALID_WITNESS),
                             (circ.shared_last, (circ.z_int[circ.shared_last] + 1) % R, oracle.OR_ERR_QAP_DIVISION),
                             (0, 2, oracle.OR_ERR_INVALID_WITNESS)):
        zb = circ.witness_with(var, value)
        broken = []
        for j in circ.rows_naming(var):
            a, b, c = circ.row_values(j, zb)
            if a * b % R != c:
                broken.append(j)
        assert len(broken) >= 3, var           # one wrong variable breaks several rows at once
        if var == circ.shared_row1:
            assert 1 in broken
        if var == circ.shared_last:
            assert 1 not in broken and circ.nc - 1 in broken
        assert oracle.prove(opk, csr, CZ.fr_rows(zb), circ.num_public, r, s)[0] == want, var


def test_pyref_qap_matches_the_dense_transform(pyref):
    """circuits.pyref_qap fills pyref.QAP's polynomials column by column; on
    one column with repeated and cancelling entries it is pyref.dft itself."""
    circ = CZ.general_circuit(70, 40, 1, SEED)
    q = CZ.pyref_qap(circ)
    for m, var in ((0, 3), (0, 0), (0, circ.cancelling), (0, circ.duplicate), (1, 2), (2, 7)):
        col = [sum(v for c, v in circ.rows[m][j] if c == var) % R for j in range(circ.nc)]
        assert q.polys[m][var] == pyref.trim(pyref.dft(col, circ.domain, inverse=True)), (m, var)
    assert q.polys[0][circ.unreferenced] == [] and q.polys[0][circ.cancelling] == []
    w = pyref.root_of_unity(circ.domain)
    assert q.evaluate_at(pow(w, 5, R), circ.z_int) == circ.row_values(5)


def test_witness_range_model(circ):
    """circuits.witness_ranges: every variable is read by some rank, the
    unreferenced one by the rank its index falls to."""
    for N in (2, 4, 8):
        own = CZ.var_owner(circ, N)
        assert own[circ.unreferenced] == circ.unreferenced * N // circ.V
        seen = set()
        for k in range(N):
            for lo, hi in CZ.witness_ranges(circ, k, N):
                seen |= set(range(lo, hi))
        assert seen == set(range(circ.V))
