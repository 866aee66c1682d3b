"""n points times n different scalars on the GPU (csrc/mulvec.hip), both
groups: the device decomposition against Python's divmod, the shipped calls and
the table walks against the plain per-lane walk word for word and against
pyref, identity lanes, zero scalars among non-zero neighbours, blocks, chunks,
in place, and the argument checks."""
import ctypes

import numpy as np
import pytest

import points_util as U
import sound_ref

pytestmark = pytest.mark.gpu

R = sound_ref.R
X = 0xD201000000010000                # r = x^4 - x^2 + 1
EDGES = [0, 1, 2, X - 1, X, X + 1, X**2 - 1, X**2, X**2 + 1, X**3 - 1, X**3, X**3 + 1,
         1 << 64, 1 << 128, 1 << 192, R - 2, R - 1]
ID1, ID2 = [0] * 12 + [1], [0] * 24 + [1]


class Group:
    def __init__(self, name, pyref):
        g2 = name == "g2"
        self.name, self.words, self.ident = name, 25 if g2 else 13, ID2 if g2 else ID1
        self.curve = pyref.G2 if g2 else pyref.G1
        self.to_words = pyref.g2_words if g2 else pyref.g1_words
        self.points = U.g2_points if g2 else U.g1_points
        self.pack = U.words_g2 if g2 else U.words_g1

    def calls(self, ctx):
        """(shipped, table, plain)"""
        return tuple(getattr(ctx, f.format(self.name)) for f in
                     ("{}_mul_scalars", "test_{}_mul_scalars_table", "test_{}_mul_scalars_plain"))


@pytest.fixture(scope="module", params=["g1", "g2"])
def grp(request, pyref):
    return Group(request.param, pyref)


@pytest.fixture(scope="module")
def pts21(grp, pyref):
    """21 points with an identity in the middle"""
    pts = list(grp.points(20))
    pts.insert(10, pyref.INF)
    return pts, grp.pack(pts)


def test_split_scalars(ctx, pyref):
    rng = pyref.SplitMix64(0x5B117)
    ks = EDGES + [rng.fr() for _ in range(8)]
    g1, g2 = ctx.test_split_scalars(ks)
    for k, a, b in zip(ks, g1, g2):
        e1, e2 = int(a[0]) | (int(a[1]) << 64), int(a[2]) | (int(a[3]) << 64)
        assert (e2, e1) == divmod(k, X * X), hex(k)
        assert e1 < 1 << 128 and e2 < 1 << 128
        d = [int(w) for w in b]
        assert all(w < X for w in d), hex(k)
        assert sum(w * X**j for j, w in enumerate(d)) == k, hex(k)
    assert [int(w) for w in g2[EDGES.index(R - 1)]] == [0, 0, X - 1, X - 1]
    with pytest.raises(ValueError, match="scalar 1 "):
        ctx.test_split_scalars([5, R])
    e1, e2 = ctx.test_split_scalars([])
    assert e1.shape == (0, 4) and e2.shape == (0, 4)


def _vectors(pyref):
    """the edge scalars and random ones mixed in one wave, one per lane (the
    identity lane, 10, holds a random one); every lane the same scalar; zeros
    among non-zero neighbours; all ones"""
    rng = pyref.SplitMix64(0x3C21)
    mixed = EDGES[:10] + [rng.fr()] + EDGES[10:] + [rng.fr() for _ in range(21 - 1 - len(EDGES))]
    assert len(mixed) == 21
    same = [rng.fr()] * 21
    zeros = [rng.fr() for _ in range(21)]
    for i in (0, 4, 5, 20):
        zeros[i] = 0
    return {"mixed": (mixed, (3, 7, 11, 17, 20)), "same": (same, (0, 12, 20)), "zeros": (zeros, (3, 4, 6, 19)),
            "ones": ([1] * 21, ())}


@pytest.mark.parametrize("which", ["mixed", "same", "zeros", "ones"])
def test_walks_21_points(ctx, pyref, grp, pts21, which):
    pts, words = pts21
    ks, checked = _vectors(pyref)[which]
    shipped, table, plain = grp.calls(ctx)
    want = plain(words, ks)
    assert np.array_equal(shipped(words, ks), want)
    assert np.array_equal(table(words, ks), want)
    assert list(want[10]) == grp.ident
    for i in checked:
        assert list(want[i]) == grp.to_words(grp.curve.mul(pts[i], ks[i])), (which, i)
    for i, k in enumerate(ks):
        if k == 0:
            assert list(want[i]) == grp.ident
    if which == "ones":
        assert np.array_equal(want, words)


def test_blocks_and_chunks(zkp, ctx, pyref, grp):
    """300 points: two full 128-lane blocks and a partial one, 300 distinct
    scalars; then chunks of 100; then in place through the raw C call."""
    pts = grp.points(300)
    words = grp.pack(pts)
    rng = pyref.SplitMix64(0xB10C5)
    ks = [rng.fr() for _ in range(300)]
    shipped, table, plain = grp.calls(ctx)
    want = plain(words, ks)
    assert np.array_equal(shipped(words, ks), want)
    assert np.array_equal(table(words, ks), want)
    for i in (0, 299):
        assert list(want[i]) == grp.to_words(grp.curve.mul(pts[i], ks[i]))
    fn = getattr(zkp.lib(), "zk_%s_mul_scalars" % grp.name)
    kw = zkp.fr_array(ks)
    try:
        ctx.set_option(zkp.ZK_OPT_POINT_CHUNK, 100)
        assert np.array_equal(shipped(words, ks), want)
        assert np.array_equal(table(words, ks), want)
        assert np.array_equal(plain(words, ks), want)
        buf = words.copy()
        rc = fn(ctypes.c_void_p(ctx._h), zkp._p(buf), ctypes.c_size_t(300), zkp._p(kw), zkp._p(buf))
        assert rc == zkp.ZK_OK and np.array_equal(buf, want)
    finally:
        ctx.set_option(zkp.ZK_OPT_POINT_CHUNK, 1 << 20)
    buf = words.copy()
    rc = fn(ctypes.c_void_p(ctx._h), zkp._p(buf), ctypes.c_size_t(300), zkp._p(kw), zkp._p(buf))
    assert rc == zkp.ZK_OK and np.array_equal(buf, want)


def test_arguments(zkp, ctx, pyref, grp, pts21):
    _, words = pts21
    ks = [3] * 21
    ks[7] = R
    for call in grp.calls(ctx):
        with pytest.raises(ValueError, match="scalar 7 "):
            call(words, ks)
    with pytest.raises(ValueError):
        grp.calls(ctx)[0](words, ks[:20])
    out = np.full_like(words, 0xA5A5A5A5)
    kw = np.array([zkp.to_limbs(k) for k in ks], dtype=np.uint64)
    fn = getattr(zkp.lib(), "zk_%s_mul_scalars" % grp.name)
    rc = fn(ctypes.c_void_p(ctx._h), zkp._p(words), ctypes.c_size_t(21), zkp._p(kw), zkp._p(out))
    assert rc == zkp.ZK_ERR_ARG and (out == 0xA5A5A5A5).all()
    assert "7" in ctx.last_error()
    assert fn(ctypes.c_void_p(ctx._h), None, ctypes.c_size_t(0), None, None) == zkp.ZK_OK
    assert grp.calls(ctx)[0](np.zeros((0, grp.words), dtype=np.uint64), []).shape == (0, grp.words)
