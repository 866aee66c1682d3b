"""The grouped-window MSM plan alone, through the public MSM
(zk_msm_*_upload_copies + zk_msm_*_dev), on G1 and G2: `copies` shifted copies
of every base, digit window w over copy w mod copies into bucket set
w / copies.  Every number of copies must give the bytes of every other, of the
host-scalar MSM on the same inputs and, for one base, of pyref's multiple."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
# scalar width -> (the upload's window width c, window count W, the copies to run)
#   255 bits: 5 leaves the last set partly filled (windows 10-12 of 15 slots),
#   12 leaves the top window alone in set 1, 0 is "all", 40 clamps to 13
PLANS = {255: (20, 13, (1, 2, 3, 5, 12, 13, 0, 40)), 64: (16, 4, (1, 2, 3, 4))}


def _edge_scalars(bits):
    c, W, _ = PLANS[bits]
    half = 1 << (c - 1)

    def digits(d):
        """every non-top digit d, no top digit: below r (240 of 255 bits) and below 2^64 (48 of 64)"""
        v = sum(d << (c * w) for w in range(W - 1))
        assert v < R and v < (1 << bits)
        return v

    # the widest values the width allows: r - 1 and 2^254, or 2^64 - 1 and 2^63
    wide = (R - 1, 1 << 254) if bits == 255 else ((1 << 64) - 1, 1 << 63)
    return [0, 1, (1 << c) - 1, half, half + 1, *wide,
            digits(half + 1),      # a carry into every next window, across every copy and set boundary
            digits(half)]          # the largest digit that does not carry


def _rows(zkp, ks):
    return np.array([zkp.to_limbs(k) for k in ks], dtype=np.uint64).reshape(-1, 4)


_edge_want = {}


def _edge_expected(pyref, g2, bits):
    """pyref's k * generator for every edge scalar, once per (group, width)."""
    key = (g2, bits)
    if key not in _edge_want:
        curve, words = (pyref.G2, pyref.g2_words) if g2 else (pyref.G1, pyref.g1_words)
        _edge_want[key] = [words(curve.mul(curve.gen, k)) for k in _edge_scalars(bits)]
    return _edge_want[key]


@pytest.mark.parametrize("bits", [255, 64])
@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_one_base_edge_scalars(zkp, ctx, pyref, g2, bits):
    curve, words = (pyref.G2, pyref.g2_words) if g2 else (pyref.G1, pyref.g1_words)
    base = np.array([words(curve.gen)], dtype=np.uint64)
    ks = _edge_scalars(bits)
    want = _edge_expected(pyref, g2, bits)
    for copies in PLANS[bits][2]:
        h = ctx.msm_upload(base, g2=g2, scalar_bits=bits, copies=copies)
        for k, w in zip(ks, want):
            assert list(h.msm(_rows(zkp, [k]), bits)) == w, (copies, hex(k))
        h.free()


def _bases(oracle, g2, n):
    if not g2:
        return oracle.g1_lin_bases(0xDEADBEEF, 0xC0FFEE, n)
    g = oracle.g2_generator()
    pool = np.array([oracle.g2_mul(g, 0xB2 + 977 * i) for i in range(64)])
    return pool[np.random.default_rng(64).integers(0, 64, n)]


@pytest.fixture(scope="module", params=[(False, 300), (False, 5000), (True, 300), (True, 5000)],
                ids=["g1-300", "g1-5000", "g2-300", "g2-5000"])
def inputs(request, oracle):
    """(g2, bases, 255-bit scalars): identity bases and zero scalars mixed in.
    5000 points x 13 windows: several 8192-entry sort tiles and thousands of
    accumulate chunks; 300 x 13: one partly filled tile."""
    g2, n = request.param
    bases = _bases(oracle, g2, n).copy()
    sc = oracle.random_fr(n, 0xC0B1E5 + n)
    for i in range(3, n, 41):
        bases[i] = 0
        bases[i, -1] = 1               # the identity
    sc[7::53] = 0
    sc[11] = 0
    bases[11] = 0
    bases[11, -1] = 1                  # both at once
    return g2, bases, sc


@pytest.mark.parametrize("bits", [255, 64])
def test_random_every_plan_the_same_bytes(zkp, ctx, inputs, bits):
    g2, bases, sc = inputs
    sc = sc.copy()
    if bits == 64:
        sc[:, 1:] = 0
    want = (ctx.msm_g2 if g2 else ctx.msm_g1)(bases, sc, bits)
    assert not want[-1]                # a real point, not the identity
    for copies in PLANS[bits][2]:
        h = ctx.msm_upload(bases, g2=g2, scalar_bits=bits, copies=copies)
        assert np.array_equal(h.msm(sc, bits), want), copies
        h.free()


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_skewed_scalars_leave_long_runs_of_empty_buckets(zkp, ctx, oracle, g2):
    """Witness-like scalars (mostly 0 and 1, a few whole ones): every bucket
    set holds little beside bucket 0, so the bucket offsets are long runs of
    empty buckets inside and between the sets, beside the unused part of the
    last set (copies 1, 3 and 12: the top window alone in it)."""
    n = 300
    bases = _bases(oracle, g2, n)
    sc = np.zeros((n, 4), dtype=np.uint64)
    sc[:, 0] = np.random.default_rng(7).integers(0, 2, n, dtype=np.uint64)
    sc[::37] = oracle.random_fr(len(sc[::37]), 0x5CE3)
    want = (ctx.msm_g2 if g2 else ctx.msm_g1)(bases, sc, 255)
    for copies in (1, 3, 5, 12, 0):
        h = ctx.msm_upload(bases, g2=g2, scalar_bits=255, copies=copies)
        assert np.array_equal(h.msm(sc, 255), want), copies
        h.free()


def test_narrow_scalars_on_a_wide_upload(zkp, ctx, oracle):
    """A 255-bit upload (c = 20) serves 64-bit scalars with its first 4
    windows: 3 copies put window 3 into a second bucket set, 5 copies are
    more than the 4 windows (one set)."""
    bases = _bases(oracle, False, 300)
    sc = oracle.random_fr(300, 0x64B175)
    sc[:, 1:] = 0
    want = ctx.msm_g1(bases, sc, 64)
    for copies in (1, 3, 5):
        h = ctx.msm_upload(bases, scalar_bits=255, copies=copies)
        assert np.array_equal(h.msm(sc, 64), want), copies
        h.free()
