"""A deterministic general R1CS circuit for the reference-mode tests: every
feature below is there by construction, none by the luck of a draw, so the
same arrays exercise the product (zkp.CSRMatrices) and the checker
(oracle.CSR) on what the synthetic x * y = z circuit never has.

  rows     A: empty in every 37th row, 40 entries in every 97th, else 1..3;
           B: 1..2, C: 1..3 (the last C entry is solved for, so z satisfies);
  values   coefficients from {1, r - 1, 2, a full-width draw};
  columns  variable 0 leads every second (non-empty) A row: one long column;
           column V + 5 ends every 11th B row: out of range, dropped
           (qap:122-124); (3, 5), (3, r - 5) ends every 13th non-empty A row: a
           repeated column whose two entries cancel;
  variables  V - 3 (`unreferenced`) is in no row; V - 2 (`cancelling`) is in A
           only, as the pair 5, r - 5 on one (row, col): rows name it, yet its
           column sums are zero; V - 1 (`duplicate`) is in A only, as the pair
           5, 3 on one (row, col): its column sum is 8 L_row;
           `shared_row1` (2) is in row 1 and in every 64th row after it;
           `shared_last` is in row nc - 1 and in every 64th row from row 2, never
           in row 1;
  unit_b   B without values (val = None, all ones) beside A and C with them.

Everything is drawn from pyref.SplitMix64(seed)."""
import numpy as np

import pyref

R = pyref.R
EMPTY_EVERY, LONG_EVERY, LONG_LEN = 37, 97, 40
DROPPED_EVERY, CANCEL_EVERY, SHARED_EVERY = 11, 13, 64
CANCEL_ROW, DUPLICATE_ROW = 5, 6
SHAPES = ((1000, 777, 3), (300, 2500, 0), (4097, 3000, 5))   # (nc, V, num_public): domains 1024, 512, 8192


def _limbs(v):
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


def fr_rows(values):
    return np.array([_limbs(v) for v in values], dtype=np.uint64).reshape(-1, 4)


class Circuit:
    def __init__(self, nc, V, num_public, rows, z, unit_b):
        self.nc, self.V, self.num_public, self.unit_b = nc, V, num_public, unit_b
        self.rows = rows            # 3 x nc lists of (col, coeff), duplicates and columns >= V kept
        self.z_int = z
        self.z = fr_rows(z)
        self.unreferenced, self.cancelling, self.duplicate = V - 3, V - 2, V - 1
        self.shared_row1, self.shared_last = 2, target(nc - 1, V)
        self.mats = [self._csr(m, unit_b and m == 1) for m in range(3)]
        n = 1
        while n < nc:
            n <<= 1
        self.domain = n

    def _csr(self, m, unit):
        rp, cols, vals = [0], [], []
        for row in self.rows[m]:
            for c, v in row:
                cols.append(c)
                vals.append(_limbs(v))
            rp.append(len(cols))
        return (np.array(rp, dtype=np.uint64), np.array(cols, dtype=np.uint32),
                None if unit else np.array(vals, dtype=np.uint64).reshape(-1, 4))

    def row_values(self, j, z=None):
        """(A z)_j, (B z)_j, (C z)_j in Python integers, columns >= V dropped"""
        z = self.z_int if z is None else z
        return [sum(v * z[c] for c, v in self.rows[m][j] if c < self.V) % R for m in range(3)]

    def rows_naming(self, var):
        """the rows with an entry on var, in any matrix"""
        return [j for j in range(self.nc) if any(c == var for m in range(3) for c, _ in self.rows[m][j])]

    def column_sums(self, var):
        """per matrix the net coefficient of var in every row that names it: {row: sum}"""
        out = []
        for m in range(3):
            acc = {}
            for j in range(self.nc):
                for c, v in self.rows[m][j]:
                    if c == var:
                        acc[j] = (acc.get(j, 0) + v) % R
            out.append(acc)
        return out

    def witness_with(self, var, value):
        z = list(self.z_int)
        z[var] = value
        return z


def target(j, V):
    """the variable row j's C is solved on"""
    return 1 + j % (V - 4)


def general_circuit(nc, V, num_public, seed, unit_b=False):
    assert V >= 16 and nc > max(CANCEL_ROW, DUPLICATE_ROW, SHARED_EVERY + 2)
    rng = pyref.SplitMix64(seed)
    z = [1] + [rng.fr() or 1 for _ in range(V - 1)]
    free = V - 3                       # drawn columns stay below the three special variables
    last = target(nc - 1, V)
    assert last not in (0, 2)

    def coef():
        k = rng.next() % 4
        return (1, R - 1, 2)[k] if k < 3 else rng.fr()

    def draw(count, j):
        out = []
        while len(out) < count:
            c = rng.next() % free
            if j == 1 and c == last:   # shared_last stays out of row 1
                continue
            out.append((c, coef()))
        return out

    A, B, C = [], [], []
    for j in range(nc):
        # ---- A ----
        if j % EMPTY_EVERY == 0:
            a = []
        else:
            length = LONG_LEN if j % LONG_EVERY == 0 else 1 + rng.next() % 3
            a = ([(0, coef())] if j % 2 == 0 else []) + draw(length - (j % 2 == 0), j)
            if j % CANCEL_EVERY == 0:
                a += [(3, 5), (3, R - 5)]
            if j == CANCEL_ROW:
                a += [(V - 2, 5), (V - 2, R - 5)]
            if j == DUPLICATE_ROW:
                a += [(V - 1, 5), (V - 1, 3)]
        # ---- B ----
        length = 1 + rng.next() % 2
        if j % SHARED_EVERY == 1:
            b = [(2, coef())] + draw(length - 1, j)
        elif j % SHARED_EVERY == 2:
            b = [(last, coef())] + draw(length - 1, j)
        else:
            b = draw(length, j)
        if j % DROPPED_EVERY == 0:
            b.append((V + 5, coef()))
        if unit_b:
            b = [(c, 1) for c, _ in b]
        # ---- C: the last entry solved for a b = c ----
        c = draw(rng.next() % 3, j)
        av = sum(v * z[k] for k, v in a) % R
        bv = sum(v * z[k] for k, v in b if k < V) % R
        rest = sum(v * z[k] for k, v in c) % R
        tgt = target(j, V)
        c.append((tgt, (av * bv - rest) * pow(z[tgt], R - 2, R) % R))
        A.append(a)
        B.append(b)
        C.append(c)
    return Circuit(nc, V, num_public, (A, B, C), z, unit_b)


# ------------------------------------------------- reference-side helpers ---
def pyref_qap(circ):
    """A pyref.QAP of the circuit for its evaluate_at, without the O(V n^2)
    constructor: the per-variable polynomials are the inverse transforms of
    the matrix columns (pyref.dft(col, n, inverse=True), trimmed), summed
    here entry by entry so that empty columns cost nothing."""
    n, V = circ.domain, circ.V
    winv = pyref.fr_inv(pyref.root_of_unity(n))
    ninv = pyref.fr_inv(n)
    q = pyref.QAP.__new__(pyref.QAP)
    q.n, q.omega = n, pyref.root_of_unity(n)
    q.num_variables, q.num_constraints = V, circ.nc
    q.polys = []
    for m in range(3):
        polys = [None] * V
        for j, row in enumerate(circ.rows[m]):
            step = pow(winv, j, R)
            for c, v in row:
                if c >= V:
                    continue                      # qap:122
                if polys[c] is None:
                    polys[c] = [0] * n
                p, acc = polys[c], v * ninv % R
                for k in range(n):
                    p[k] = (p[k] + acc) % R
                    acc = acc * step % R
        q.polys.append([pyref.trim(p) if p is not None else [] for p in polys])
    return q


def var_owner(circ, N):
    """key.hip's var_owner restated: a variable belongs to the rank whose
    quotient rows name it first (row j: rank (j mod n / N) / (n / N^2), columns
    >= V ignored), a variable no row names to rank v N / V."""
    m = circ.domain // N
    q = m // N
    own = [None] * circ.V
    for j in range(circ.nc):
        rk = (j % m) // q
        for mat in range(3):
            for c, _ in circ.rows[mat][j]:
                if c < circ.V and own[c] is None:
                    own[c] = rk
    return [v * N // circ.V if o is None else o for v, o in enumerate(own)]


def witness_ranges(circ, shard, N):
    """the [lo, hi) ranges of z that rank `shard` of N reads with a
    distributed quotient: z_0, the variables it owns, and the columns of its
    rows a n / N + shard n / N^2 + b (a < N, b < n / N^2)"""
    m = circ.domain // N
    q = m // N
    own = var_owner(circ, N)
    vars_ = {0} | {v for v, o in enumerate(own) if o == shard}
    for a in range(N):
        for b in range(q):
            j = a * m + shard * q + b
            if j < circ.nc:
                vars_ |= {c for mat in range(3) for c, _ in circ.rows[mat][j] if c < circ.V}
    out = []
    for v in sorted(vars_):
        if out and out[-1][1] == v:
            out[-1][1] = v + 1
        else:
            out.append([v, v + 1])
    return out
