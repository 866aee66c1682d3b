"""The per-lane point walks at launch sizes past one block per CU (DESIGN.md
2.16, 2.17).  Every comparison is byte equality of canonical words.

The one wrong result on record (2.17, "A plain walk that went wrong") showed
only from block 257 of a launch on, in a kernel at two waves per SIMD whose
lanes walked from their own top bits.  The kernels that still do that -- the
group transform's stages (gn_walk_mem), the column sums (gn_walk_aff and
per-lane run lengths) -- run here at the smallest launches that reach that
regime: a block is 128 lanes, an MI355X has 256 CUs of 4 SIMDs, so up to 256
blocks can sit one per CU, a 2-waves/SIMD kernel holds 1024 blocks at once and
a 1-wave/SIMD kernel 512; past that a block starts in a slot another block has
left (reasoned from the resource table, not measured).  Hence N1 = 1026 blocks
(G1), N2 = 514 blocks (G2), the last block partial, and transforms whose stage
kernels have 512 .. 2048 blocks.

Reference: inputs are P_i = [s_i]G from the 255-bit fixed-base kernel (a fixed
trip count, no control flow on the scalar); k_i P_i must be the same kernel's
[s_i k_i mod r]G, the product in Python integers.  The fixed-base kernel and the
trusted key are anchored on the CPU oracle / Python integers at sampled
entries.

What it found: while gn_walk_aff / gn_walk_mem looped over a
per-lane trip count, test_hook_walks[g1-aff-*] failed from block 256 on (mixed:
32 123 of 131 237 lanes, uniform: 49 129, one scalar for all lanes: 47 614), a
whole wave's decision flipped at one step; every other test here passed.  With
the helpers' per-wave step count (gn_wave_top) all of it passes."""
import ctypes

import numpy as np
import pytest

import sound_ref
import srs_util

pytestmark = pytest.mark.gpu

R = sound_ref.R
X = 0xD201000000010000                # r = x^4 - x^2 + 1
BLOCK = 128
N1 = 1025 * BLOCK + 37                # G1: 1026 blocks, past 1024 resident ones
N2 = 513 * BLOCK + 37                 # G2: 514 blocks, past 512 resident ones
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 254, 255)
MASK64 = (1 << 64) - 1


def _limbs(ints):
    """ints in [0, 2^256) -> (n, 4) uint64 little-endian limbs"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), dtype="<u8").reshape(-1, 4).copy()


def _ints(limbs):
    return [int.from_bytes(row.tobytes(), "little") for row in np.ascontiguousarray(limbs, dtype="<u8")]


def _random_limbs(seed, n):
    """n values uniform below 2^254 (< r) as limbs"""
    a = np.random.default_rng(seed).integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 62) - 1)
    return a


def _random_fr(seed, n):
    """n values uniform below 2^255, reduced below r"""
    a = np.random.default_rng(seed).integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 63) - 1)
    return [v % R for v in _ints(a)]


class Group:
    def __init__(self, name):
        self.name, self.g2 = name, name == "g2"
        self.n = N2 if self.g2 else N1
        self.words = 25 if self.g2 else 13
        # the first block, block 257, the first block past the resident ones, the partial last one
        self.blocks = (0, 256, 512 if self.g2 else 1024, self.n // BLOCK)


GROUPS = {"g1": Group("g1"), "g2": Group("g2")}


@pytest.fixture(scope="module", params=["g1", "g2"])
def grp(request):
    return GROUPS[request.param]


# ------------------------------------------------------- points and scalars ---
@pytest.fixture(scope="module")
def base_scalars():
    """s_i of P_i = [s_i]G, N1 of them (G2 takes the first N2); every 16th point
    is the identity"""
    s = _random_fr(0x5CA1E, N1)
    for i in range(0, N1, 16):
        s[i] = 0
    return s


@pytest.fixture(scope="module")
def pools(ctx, base_scalars):
    """group name -> (s, points): made once, never changed"""
    out = {}
    for g in GROUPS.values():
        s = base_scalars[:g.n]
        pts = ctx.test_fixed_base(_limbs(s), g2=g.g2)
        pts.setflags(write=False)
        out[g.name] = (s, pts)
    return out


def _mixed(n):
    """Lane i draws its bit length from LENGTHS by i mod 14, so one wave holds
    every length several times: top bit set, random bits below, the draw reduced
    below r for length 255.  Then 1, r - 1, r - 2 in the sampled blocks and every
    23rd scalar 0."""
    draw = _ints(np.random.default_rng(0x317ED).integers(0, 1 << 64, size=(n, 4), dtype=np.uint64))
    ks = []
    for i, d in enumerate(draw):
        ln = LENGTHS[i % len(LENGTHS)]
        ks.append(0 if ln == 0 else ((1 << (ln - 1)) | (d & ((1 << (ln - 1)) - 1))) % R)
    for b in (0, 256, 512, 1024, n // BLOCK):
        if b * BLOCK + 12 < n:
            ks[b * BLOCK + 9: b * BLOCK + 12] = [1, R - 1, R - 2]
    for i in range(0, n, 23):
        ks[i] = 0
    return ks


def _by_wave(n):
    """One length per wave, from LENGTHS by the wave's index, random bits below
    the top one: the helpers walk a wave from its longest lane's top bit, so in
    the mixed vector (a 255-bit lane in every wave) a lane's own top bit counts
    for nothing; here it sets the wave's step count."""
    draw = _ints(np.random.default_rng(0x3A7E5).integers(0, 1 << 64, size=(n, 4), dtype=np.uint64))
    ks = []
    for i, d in enumerate(draw):
        ln = LENGTHS[(i // 64) % len(LENGTHS)]
        ks.append(0 if ln == 0 else ((1 << (ln - 1)) | (d & ((1 << (ln - 1)) - 1))) % R)
    return ks


@pytest.fixture(scope="module")
def vectors():
    """name -> N1 scalars (G2 takes the first N2)"""
    return {"mixed": _mixed(N1), "uniform": _random_fr(0x0F12, N1), "same": _random_fr(0x5A3E, 1) * N1,
            "waves": _by_wave(N1)}


@pytest.fixture(scope="module")
def expected(ctx, pools, vectors):
    """(group, vector) -> the words of [s_i k_i mod r]G, each made once"""
    memo = {}

    def get(g, which):
        if (g.name, which) not in memo:
            s, _ = pools[g.name]
            want = ctx.test_fixed_base(_limbs([a * k % R for a, k in zip(s, vectors[which])]), g2=g.g2)
            want.setflags(write=False)
            memo[g.name, which] = want
        return memo[g.name, which]
    return get


def test_reference_anchor(oracle, pools, grp):
    """the fixed-base kernel against the C oracle at 16 entries: four in each of
    the first block, block 257, the first block past the resident ones and the
    partial last block"""
    s, pts = pools[grp.name]
    gen = oracle.g2_generator() if grp.g2 else oracle.g1_generator()
    mul = oracle.g2_mul if grp.g2 else oracle.g1_mul
    for b in grp.blocks:
        for off in (1, 13, 29, 36):
            i = b * BLOCK + off
            assert s[i] != 0
            assert np.array_equal(pts[i], mul(gen, s[i])), i


# ------------------------------------------------------------- the hook walks ---
def _report(ctx, g, got, want, s, ks, what):
    """The wrong lanes by block, and for the first few whether the value is
    k' P for k' = k with one bit flipped (the pattern of DESIGN.md 2.17)."""
    bad = np.flatnonzero((got != want).any(axis=1))
    blocks, counts = np.unique(bad // BLOCK, return_counts=True)
    lines = ["%s: %d of %d lanes differ, in %d blocks from block %d to %d"
             % (what, len(bad), len(got), len(blocks), blocks[0], blocks[-1]),
             "wrong lanes per block: " + ", ".join("%d: %d" % bc for bc in list(zip(blocks, counts))[:24])]
    sample = [int(i) for i in bad[:8]]
    flips = [s[i] * (ks[i] ^ (1 << b)) % R for i in sample for b in range(255)]
    cand = ctx.test_fixed_base(_limbs(flips), g2=g.g2).reshape(len(sample), 255, -1)
    for row, i in zip(cand, sample):
        hit = [b for b in range(255) if np.array_equal(row[b], got[i])]
        lines.append("lane %d (block %d, lane %d of it), k of %d bits: %s"
                     % (i, i // BLOCK, i % BLOCK, ks[i].bit_length(),
                        "k with bit %d flipped" % hit[0] if hit else "no one-bit flip of k"))
    return "\n".join(lines)


@pytest.mark.parametrize("which", ["mixed", "uniform", "same", "waves"])
@pytest.mark.parametrize("mem", [False, True], ids=["aff", "mem"])
def test_hook_walks(ctx, pools, vectors, expected, grp, mem, which):
    """zk_test_gn_walk: gn_walk_aff / gn_walk_mem, every lane from its own top
    bit.  The mixed vector runs a second time and must give the first call's
    bytes: the recorded defect changed from run to run."""
    s, pts = pools[grp.name]
    ks = vectors[which][:grp.n]
    kw = _limbs(ks)
    want = expected(grp, which)
    got = ctx.test_gn_walk(pts, kw, g2=grp.g2, mem=mem)
    if not np.array_equal(got, want):
        pytest.fail(_report(ctx, grp, got, want, s, ks, "%s mem=%d %s" % (grp.name, mem, which)))
    if which == "mixed":
        again = ctx.test_gn_walk(pts, kw, g2=grp.g2, mem=mem)
        if not np.array_equal(again, got):
            pytest.fail(_report(ctx, grp, again, want, s, ks, "%s mem=%d mixed, second call" % (grp.name, mem)))
        ident = np.array([0] * (grp.words - 1) + [1], dtype=np.uint64)
        zero = np.array([a == 0 or k == 0 for a, k in zip(s, ks)])
        assert zero[::16].all() and zero[::23].all() and (got[zero] == ident).all()
        assert not (got[~zero] == ident).all(axis=1).any()


def test_hook_arguments(zkp, ctx, pools, grp):
    _, pts = pools[grp.name]
    with pytest.raises(ValueError, match="scalar 2 "):
        ctx.test_gn_walk(pts[:4], [1, 2, R, 3], g2=grp.g2)
    with pytest.raises(ValueError):
        ctx.test_gn_walk(pts[:4], [1, 2, 3], g2=grp.g2)
    assert ctx.test_gn_walk(pts[:0], [], g2=grp.g2, mem=True).shape == (0, grp.words)
    fn = zkp.test_lib().zk_test_gn_walk
    h, kw, out = ctypes.c_void_p(ctx._h), _limbs([1]), np.zeros((1, grp.words), dtype=np.uint64)
    one = np.ascontiguousarray(pts[1:2])
    for g2, mem in ((2, 0), (0, 2), (-1, 0)):
        assert fn(h, ctypes.c_int(g2), ctypes.c_int(mem), zkp._p(one), ctypes.c_size_t(1), zkp._p(kw),
                  zkp._p(out)) == zkp.ZK_ERR_ARG
    assert fn(h, ctypes.c_int(int(grp.g2)), ctypes.c_int(0), None, ctypes.c_size_t(1), zkp._p(kw),
              zkp._p(out)) == zkp.ZK_ERR_ARG
    assert fn(None, ctypes.c_int(0), ctypes.c_int(0), zkp._p(one), ctypes.c_size_t(1), zkp._p(kw),
              zkp._p(out)) == zkp.ZK_ERR_ARG


# ---------------------------------------------- shipped walks at the same sizes ---
@pytest.mark.parametrize("call", ["shipped", "table", "plain"])
def test_mul_scalars_mixed(zkp, ctx, pools, vectors, expected, grp, call):
    """zk_g*_mul_scalars and the table hooks (a fixed trip count by
    construction) and the plain baseline (every lane from bit 254) on the mixed
    vector"""
    s, pts = pools[grp.name]
    ks = vectors["mixed"][:grp.n]
    fn = (getattr(zkp.lib(), "zk_%s_mul_scalars" % grp.name) if call == "shipped"
          else getattr(zkp.test_lib(), "zk_test_%s_mul_scalars_%s" % (grp.name, call)))
    kw, out = _limbs(ks), np.zeros_like(pts)
    rc = fn(ctypes.c_void_p(ctx._h), zkp._p(pts), ctypes.c_size_t(len(pts)), zkp._p(kw), zkp._p(out))
    assert rc == zkp.ZK_OK, ctx.last_error()
    want = expected(grp, "mixed")
    if not np.array_equal(out, want):
        pytest.fail(_report(ctx, grp, out, want, s, ks, "%s_mul_scalars %s" % (grp.name, call)))


@pytest.mark.parametrize("which", ["x2+1", "r-1", "random"])
def test_g1_mul_scalar_one(ctx, pools, which):
    """zk_g1_mul_scalar (cm_walk_endo, one scalar for every lane) on N1 points"""
    s, pts = pools["g1"]
    k = {"x2+1": X * X + 1, "r-1": R - 1, "random": _random_fr(0x1CA, 1)[0]}[which]
    want = ctx.test_fixed_base(_limbs([a * k % R for a in s]))
    got = ctx.g1_mul_scalar(pts, k)
    if not np.array_equal(got, want):
        pytest.fail(_report(ctx, GROUPS["g1"], got, want, s, [k] * N1, "g1_mul_scalar " + which))


# ------------------------------------------------------------ group transform ---
# G1 stage kernel (2 waves/SIMD): 512 blocks at 2^17 (the first co-residency),
# 2048 at 2^19 (slot reuse).  G2 (1 wave/SIMD): 512 at 2^17, 1024 at 2^18.
TRANSFORMS = [("g1", 17, False), ("g1", 17, True), ("g1", 19, True),
              ("g2", 17, False), ("g2", 17, True), ("g2", 18, True)]
_T_IDS = ["%s-2p%d-%s" % (g, ln, "inv" if inv else "fwd") for g, ln, inv in TRANSFORMS]


def _ntt(ctx, g, pts, inverse):
    return ctx.g2_ntt(pts, inverse) if g == "g2" else ctx.g1_ntt(pts, inverse)


@pytest.fixture(scope="module")
def transforms(ctx):
    """Inputs, expected words and the default mapping's output of every
    transform, each made once.  Inputs: P_j = [s_j]G, every 97th the identity;
    expected: the fixed base of the Fr transform of s."""
    class Memo:
        inputs, wanted, outputs = {}, {}, {}

        def input(self, g, log_n):
            if (g, log_n) not in self.inputs:
                sc = _random_limbs(0x6E77 + log_n, 1 << log_n)
                sc[::97] = 0
                pts = ctx.test_fixed_base(sc, g2=(g == "g2"))
                pts.setflags(write=False)
                self.inputs[g, log_n] = (sc, pts)
            return self.inputs[g, log_n]

        def want(self, g, log_n, inverse):
            if (g, log_n, inverse) not in self.wanted:
                sc, _ = self.input(g, log_n)
                w = ctx.test_fixed_base(ctx.ntt(sc, inverse=inverse), g2=(g == "g2"))
                w.setflags(write=False)
                self.wanted[g, log_n, inverse] = w
            return self.wanted[g, log_n, inverse]

        def output(self, g, log_n, inverse):
            """the transform under the default (shared) mapping"""
            if (g, log_n, inverse) not in self.outputs:
                o = _ntt(ctx, g, self.input(g, log_n)[1], inverse)
                o.setflags(write=False)
                self.outputs[g, log_n, inverse] = o
            return self.outputs[g, log_n, inverse]
    return Memo()


def _wrong_rows(got, want):
    bad = np.flatnonzero((got != want).any(axis=1))
    return "%d of %d outputs differ, the first at %s" % (len(bad), len(got), bad[:16].tolist())


@pytest.mark.parametrize("g,log_n,inverse", TRANSFORMS, ids=_T_IDS)
def test_transform_against_fr_ntt(ctx, transforms, g, log_n, inverse):
    got = transforms.output(g, log_n, inverse)
    want = transforms.want(g, log_n, inverse)
    assert np.array_equal(got, want), _wrong_rows(got, want)


@pytest.mark.parametrize("g,log_n,inverse", [t for t in TRANSFORMS if t[1] == 17], ids=[i for i in _T_IDS if "2p17" in i])
def test_transform_per_lane_mapping(zkp, ctx, transforms, g, log_n, inverse):
    """ZK_OPT_GNTT_MAP = 0: a twiddle per lane in every stage, so every stage is
    a per-lane walk"""
    _, pts = transforms.input(g, log_n)
    want = transforms.want(g, log_n, inverse)
    try:
        ctx.set_option(zkp.ZK_OPT_GNTT_MAP, 0)
        got = _ntt(ctx, g, pts, inverse)
    finally:
        ctx.set_option(zkp.ZK_OPT_GNTT_MAP, -1)
    assert np.array_equal(got, want), _wrong_rows(got, want)


@pytest.fixture(scope="module")
def power_tables(pyref):
    """(n, inverse) -> limbs of w^(+-j) (/ n), j < n"""
    memo = {}

    def get(n, inverse):
        if (n, inverse) not in memo:
            w = pyref.root_of_unity(n)
            v = 1
            if inverse:
                w, v = pyref.fr_inv(w), pyref.fr_inv(n)
            buf = bytearray()
            for _ in range(n):
                buf += v.to_bytes(32, "little")
                v = v * w % R
            memo[n, inverse] = np.frombuffer(bytes(buf), dtype="<u8").reshape(n, 4)
        return memo[n, inverse]
    return get


@pytest.mark.parametrize("g,log_n,inverse", TRANSFORMS, ids=_T_IDS)
def test_transform_against_msm(ctx, transforms, power_tables, g, log_n, inverse):
    """Free of the Fr NTT: out[k] = sum_j w^(+-jk) (/ n) P_j through the public
    MSM, at the ends and around the middle"""
    n = 1 << log_n
    _, pts = transforms.input(g, log_n)
    got = transforms.output(g, log_n, inverse)
    table = power_tables(n, inverse)
    msm = ctx.msm_g2 if g == "g2" else ctx.msm_g1
    j = np.arange(n, dtype=np.uint64)
    for k in (0, 1, n // 2 - 1, n // 2, n - 1):
        co = np.ascontiguousarray(table[(j * np.uint64(k)) % np.uint64(n)])
        assert np.array_equal(got[k], msm(pts, co)), k


# ------------------------------------------- column sums through CRS.from_srs ---
LOG_D = 17
NC = (1 << LOG_D) - 300               # padded rows
NV = N1                               # k_gn_col_cols_g1 past 1024 blocks
NUM_PUBLIC = 3
# entries of column j >= 1: between 0 and 40, different in neighbouring columns
COL_LEN = np.array([0, 40, 3, 1, 17, 0, 2, 29, 1, 0, 8, 2, 36, 1, 5, 0, 12, 3, 0, 23, 1, 2, 40, 0, 9, 1, 4, 0, 31, 2,
                    1, 6], dtype=np.int64)
CYCLE = (1, R - 1, 2, 3, 1 << 64, (1 << 128) + 1)
COL_CANCEL, COL_DOUBLE = 32 * 100, 32 * 100 + 5       # both otherwise empty


def _matrix(m):
    """One constraint matrix in CSR, built with numpy (m = 0, 1, 2: A, B, C).
    Variable 0 in every row of A and C (one column of NC entries: many runs at
    any run length) and in every 64th row of B (2044 entries, still many runs:
    the lanes of a long column add their runs in sequence, and with a full-width
    coefficient in nearly every step of a wave a G2 column of NC entries alone
    takes over 10 s); column j >= 1 holds
    COL_LEN[(j + m) % 32] entries in distinct rows; the pair 5, r - 5 on one
    (row, col) of an otherwise empty column cancels, the pair 5, 3 on one
    (row, col) of another is a duplicate.  Coefficients cycle per entry (in CSR
    order) through CYCLE with a fresh value below 2^254 every 16th entry, so
    neighbouring entries of a column, and neighbouring runs, differ in walk
    length."""
    lens = COL_LEN[(np.arange(NV) + m) % len(COL_LEN)].copy()
    lens[0] = 0
    cols = np.repeat(np.arange(NV, dtype=np.int64), lens)
    starts = np.cumsum(lens) - lens
    t = np.arange(len(cols), dtype=np.int64) - np.repeat(starts, lens)
    rows = (cols * (131 + 2 * m) + t * 3001) % NC               # 40 * 3001 < NC: distinct within a column
    extra_c = [c for c in (COL_CANCEL - m, COL_DOUBLE - m) for _ in range(2)]
    assert all(lens[c] == 0 for c in extra_c)
    rows0 = np.arange(0, NC, 64 if m == 1 else 1, dtype=np.int64)
    rows = np.concatenate([rows0, rows, np.array([10, 10, 11, 11], dtype=np.int64)])
    cols = np.concatenate([np.zeros(len(rows0), dtype=np.int64), cols, np.array(extra_c, dtype=np.int64)])
    fixed = np.zeros(len(rows), dtype=np.int64)
    fixed[-4:] = (1, 2, 3, 4)
    order = np.argsort(rows, kind="stable")
    rows, cols, fixed = rows[order], cols[order], fixed[order]
    nnz = len(rows)
    e = np.arange(nnz)
    vals = _limbs(CYCLE)[e % len(CYCLE)]
    wide = _random_limbs(0xC0EF + m, (nnz + 15) // 16)
    vals[::16] = wide
    for tag, v in ((1, 5), (2, R - 5), (3, 5), (4, 3)):
        vals[fixed == tag] = _limbs([v])[0]
    rp = np.zeros(NC + 1, dtype=np.uint64)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=NC))
    return rp, cols.astype(np.uint32), np.ascontiguousarray(vals)


@pytest.fixture(scope="module")
def big(zkp, ctx, pyref):
    """the circuit, the string for its domain and the trusted key"""
    case = srs_util.case4(pyref)
    mats = [_matrix(m) for m in range(3)]
    qap = zkp.QAP(zkp.CSRMatrices(NC, NV, mats))
    assert qap.domain_size == 1 << LOG_D
    return {"case": case, "mats": mats, "qap": qap, "srs": srs_util.string(zkp, ctx, case, LOG_D),
            "trusted": srs_util.trusted(zkp, ctx, qap, case, NUM_PUBLIC)}


def test_trusted_key_anchor(oracle, pyref, big):
    """The trusted key at this size against Python integers: for 8 short columns
    of a_g1 and 4 of b_g2, [sum val L_row(tau)]G with
    L_i(tau) = (tau^n - 1) / n * w^i / (tau - w^i), through the oracle's
    multiplication of the generator."""
    n, tau = 1 << LOG_D, big["case"]["tau"]
    w = pyref.root_of_unity(n)
    zn = (pow(tau, n, R) - 1) * pyref.fr_inv(n) % R

    def column(m, j):
        rp, cols, vals = big["mats"][m]
        at = np.flatnonzero(cols == j)
        rows = np.searchsorted(rp, at, side="right") - 1
        acc = 0
        for i, v in zip(rows.tolist(), _ints(vals[at])):
            wi = pow(w, i, R)
            acc += v * zn * wi * pyref.fr_inv(tau - wi)
        return acc % R, len(at)

    pk = big["trusted"].pk
    g1, g2 = oracle.g1_generator(), oracle.g2_generator()
    for j in (1, 2, 3, 7, 12, COL_CANCEL, COL_DOUBLE, NV - 1):
        k, cnt = column(0, j)
        assert 0 < cnt <= 41
        assert np.array_equal(pk.a_g1[j], oracle.g1_mul(g1, k)), j
    assert int(pk.a_g1[COL_CANCEL][12]) == 1 and int(pk.a_g1[COL_DOUBLE][12]) == 0
    for j in (1, 6, COL_DOUBLE - 1, NV - 2):
        k, cnt = column(1, j)
        assert 0 < cnt <= 41
        assert np.array_equal(pk.b_g2[j], oracle.g2_mul(g2, k)), j


def test_key_from_string_2p17(zkp, ctx, big):
    """k_gn_col_runs_* / k_gn_col_cols_* at 1026 blocks of columns with per-lane
    run lengths and coefficient lengths that differ within a wave, after four
    transforms at 2^17.  One call, so it cannot be split: about 15 s on an
    MI355X, nearly all of it the 512-entry runs of variable 0's column in A and C,
    which a lane adds in sequence with a full-width coefficient somewhere in the
    wave at nearly every step (run length 7 below: 4 s)."""
    srs_util.same_crs(zkp.CRS.from_srs(ctx, big["qap"], big["srs"], NUM_PUBLIC), big["trusted"])


def test_key_from_string_2p17_run7(zkp, ctx, big):
    """ZK_OPT_SRS_RUN = 7: many more runs than columns, the same bytes"""
    try:
        ctx.set_option(zkp.ZK_OPT_SRS_RUN, 7)
        crs = zkp.CRS.from_srs(ctx, big["qap"], big["srs"], NUM_PUBLIC)
    finally:
        ctx.set_option(zkp.ZK_OPT_SRS_RUN, 0)
    srs_util.same_crs(crs, big["trusted"])
