"""CPU checks of the MSM indexing model (tests/msm_model.py) and of the case
table the GPU chunking tests run (tests/msm_cases.py): the model's digits
give back the scalar, an MSM over integers mod r run through the model's
buckets gives sum k_i b_i for every plan kind, and every case of the sweep
reaches what the table says it is there for.  No GPU and no library."""
import numpy as np
import pytest

import msm_cases as mc
import msm_model as mm

R = mm.R
# (kind, bits, c, copies): the widths the library's plans use, and small ones
PLAN_PARAMS = [("window", 64, 4, 0), ("window", 64, 8, 0), ("window", 255, 9, 0), ("window", 255, 5, 0),
               ("window", 64, 16, 0), ("shared", 64, 16, 0), ("shared", 255, 20, 0), ("shared", 255, 22, 0),
               ("grouped", 255, 20, 3), ("grouped", 255, 20, 5), ("grouped", 255, 20, 12), ("grouped", 64, 16, 3),
               ("grouped", 255, 20, 1), ("grouped", 255, 20, 40)]


def _ids(p):
    return "-".join(str(x) for x in p)


def test_chunk_len_and_levels():
    assert mm.chunk_len(0, 7) == 4 and mm.chunk_len(1, 1) == 4 and mm.chunk_len(260, 1) == 260
    assert mm.chunk_len(16384, 456) == 36 and mm.chunk_len(17, 4) == 8 and mm.chunk_len(16, 4) == 4
    assert [mm.merge_levels(t) for t in (1, 2, 3, 4, 5, 16, 17, 64, 65)] == [0, 1, 1, 1, 2, 2, 3, 3, 4]
    for M in (1, 5, 260, 1088, 16384, 53248):
        for K in mc.TARGET_K:
            if M > K * K // 4:      # below that, ceil(M / T) can fall more than 3 short of K
                assert mm.chunk_len(M, mm.units_for(M, K)) == K, (M, K)


@pytest.mark.parametrize("params", PLAN_PARAMS, ids=_ids)
def test_digits_reconstruct_the_scalar(params):
    kind, bits, c, copies = params
    plan = mm.Plan(kind, bits, c, copies=copies)
    vals = mc.edge_scalars(bits, c, plan.nwin) + mm.ints_of(mc.scalars("uniform", 200, bits, seed=3))
    # the edge scalars of test_gpu_msm_copies (c = 16 at 64 bits, 20 at 255) for every width
    c0, w0 = (16, 4) if bits == 64 else (20, 13)
    vals += mc.edge_scalars(bits, c0, w0)
    mag, neg = mm.digits(plan, mm.limbs_of(vals))
    assert mm.digits_value(plan, mag, neg) == vals
    half = 1 << (c - 1)
    assert (mag[:, :-1] <= half).all() and (mag[:, -1] <= (1 << plan.top)).all() and not neg[:, -1].any()
    assert (mag >= 0).all()      # (a window of all ones under a carry is digit 0 with a carry out: neg, mag 0)
    # a carry into every next window, and the largest digit that does not carry
    m2, n2 = mm.digits(plan, mm.limbs_of([sum((half + 1) << (c * w) for w in range(plan.nwin - 1)),
                                           sum(half << (c * w) for w in range(plan.nwin - 1))]))
    assert n2[0, :-1].all() and m2[0, 0] == half - 1 and (m2[0, 1:-1] == half - 2).all() and m2[0, -1] == 1
    assert not n2[1].any() and (m2[1, :-1] == half).all() and m2[1, -1] == 0


def _int_bases(n, seed):
    rng = np.random.default_rng(seed)
    b = [int(x) for x in rng.integers(1, 1 << 62, n)]
    for i in range(3, n, 41):
        b[i] = 0                        # an identity base
    if n > 12:
        b[11] = R - b[10]               # P, -P
    return b


@pytest.mark.parametrize("dist", ["uniform", "skewed", "staircase", "edges"])
@pytest.mark.parametrize("params", PLAN_PARAMS, ids=_ids)
def test_integer_msm_through_the_buckets(params, dist):
    kind, bits, c, copies = params
    plan = mm.Plan(kind, bits, c, copies=copies)
    n = 150
    sc = mc.scalars(dist, n, bits, plan, seed=5)
    b = _int_bases(n, 17)
    g = mm.Grouping(plan, sc)
    want = sum(k * v for k, v in zip(mm.ints_of(sc), b)) % R
    assert mm.bucket_sum(plan, g, b) == want
    # the layout: sorted keys inside [0, G), offsets that bracket every bucket, M by the plan kind
    assert (np.diff(g.key.astype(np.int64)) >= 0).all() and (g.M == 0 or g.key[-1] < plan.G)
    assert g.off[0] == 0 and g.off[-1] == g.M and len(g.off) == plan.G + 1
    nz = int((mm.digits(plan, sc)[0] > 0).sum())
    assert g.M == (nz if kind == "window" else n * plan.nwin)
    assert int((g.ent == mm.DUMMY).sum()) == (0 if kind == "window" else n * plan.nwin - nz)
    for bkt in np.unique(g.key)[:50]:
        assert (g.key[g.off[bkt]:g.off[bkt + 1]] == bkt).all()


@pytest.mark.parametrize("nseg", [1, 2, 3, 4])
def test_integer_msm_batch_of_segments(nseg):
    """A batch: every segment its own bucket set and its own sum; a segment
    that is a sub-range of a longer window-shifted vector (ioff, wstride)."""
    plan = mm.Plan("batch", 64, 16, nseg=nseg)
    segs, bases, want = [], [], []
    for k in range(nseg):
        full, ioff = 70 + 13 * k, 5 * k
        n = full - ioff - 3
        sc = mc.scalars(("uniform", "skewed", "ones", "edges")[k], n, 64, plan, seed=20 + k)
        b = _int_bases(full, 30 + k)
        segs.append((sc, ioff, full))
        bases.append(b)
        want.append(sum(s * v for s, v in zip(mm.ints_of(sc), b[ioff:ioff + n])) % R)
    g = mm.Grouping(plan, segs=segs)
    assert plan.G == nseg << 16 and g.M == sum(len(s[0]) for s in segs) * 4
    assert [mm.bucket_sum(plan, g, bases, seg=k) for k in range(nseg)] == want


def test_grouped_plan_shapes():
    """msm_make_plan_grouped: S >= W or S <= 0 is the shared plan; the sets are equal."""
    assert mm.Plan("grouped", 255, 20, copies=13).G == mm.Plan("shared", 255, 20).G == 1 << 19
    assert mm.Plan("grouped", 255, 20, copies=0).nsets == 1
    p = mm.Plan("grouped", 255, 20, copies=5)
    assert (p.nsets, p.copies, p.G, p.set_weight_exp(2)) == (3, 5, 3 << 19, 200)
    p = mm.Plan("grouped", 64, 16, copies=3)
    assert (p.nsets, p.setsize, p.G) == (2, 1 << 16, 1 << 17)     # the unsigned 16-bit top window: 2^16 buckets
    w = mm.Plan("window", 255, 9)
    assert (w.nwin, w.top, w.G) == (29, 3, 28 * 256 + 8)


def test_spans_by_hand():
    """Three buckets of 5, 9 and 2 entries under K = 4: chunks [0,4) [4,8) [8,12) [12,16)."""
    plan = mm.Plan("window", 64, 4)
    sc = mm.limbs_of([1] * 5 + [2] * 9 + [3] * 2)
    g = mm.Grouping(plan, sc)
    assert list(g.off[:5]) == [0, 5, 14, 16, 16] and g.M == 16
    K, P = g.spans(4)
    assert K == 4 and list(P[:4]) == [2, 3, 1, 0]
    ch = g.chunking(4, 2)
    assert (ch["nbig"], ch["max_span"], ch["split"], ch["by_boundary"], ch["nlevels"]) == (1, 3, 2, True, 1)
    assert g.chunking(2, 1)["K"] == 8 and g.chunking(2, 1)["nbig"] == 1 and g.chunking(1)["max_span"] == 1


# ---- the sweep's case table meets its own conditions -------------------------
_groupings = {}


def sweep_grouping(case):
    key = (case.plan, case.n, case.dist)
    if key not in _groupings:
        plan = mc.make_plan(case.plan, case.n)
        _groupings[key] = mm.Grouping(plan, mc.scalars(case.dist, case.n, plan.bits, plan))
    return _groupings[key]


@pytest.mark.parametrize("case", mc.SWEEP, ids=mc.case_id)
def test_sweep_case_meets_its_conditions(case):
    assert case.want, "a case must say what it is in the table for"
    g = sweep_grouping(case)
    T, fm, K, ch = mc.resolve(case, g)
    assert K in mc.TARGET_K or (T == 1 and case.K == 0)
    assert 1 <= T <= 1 << 22 and case.n <= 4096
    mc.check_want(case, ch, fm)
    if "merge" in case.want or "fixup" in case.want:
        assert T > 1


def test_sweep_covers_what_the_suite_lacked():
    cases = [(c, mc.resolve(c, sweep_grouping(c))) for c in mc.SWEEP]
    assert {K for c, (T, fm, K, ch) in cases} >= set(mc.TARGET_K)
    assert len({mc.case_id(c) for c in mc.SWEEP}) == len(mc.SWEEP)
    Ts = {T for c, (T, fm, K, ch) in cases}
    assert {1, 2, 3, 5, 17} <= Ts and any(T & (T - 1) for T in Ts)
    for curve in (0, 1):
        mine = [(c, r) for c, r in cases if c.g2 == curve]
        assert any(r[3]["nbig"] and 16 < r[3]["max_span"] <= 64 for c, r in mine)      # two merge levels
        assert any(r[3]["nbig"] and r[3]["max_span"] > 64 for c, r in mine)            # three and more
        assert any(not r[3]["nbig"] and r[3]["max_span"] >= 2 for c, r in mine)        # the fixup alone
        assert any("edge" in c.want for c, r in mine)
        assert any(T == 1 for c, (T, fm, K, ch) in mine)
    for kind in ("window", "shared", "grouped"):
        bb = {r[3]["by_boundary"] for c, r in cases if mc.PLANS[c.plan][0] == kind}
        assert bb == {True, False}, kind
    # chunks longer than one EntQ fill of 16, cut both at and off a multiple of 16
    assert {K for c, (T, fm, K, ch) in cases if K > 16 and K % 16} and {K for c, (T, fm, K, ch) in cases if K > 16 and K % 16 == 0}


def test_fix_max_cases():
    """test_gpu_msm_chunks' fix_max sweep: 1 sends every split bucket to the
    merge, 64 almost none, on both inputs at both chunk lengths."""
    for dist in ("staircase", "ones"):
        plan = mc.make_plan("S64", 4096)
        g = mm.Grouping(plan, mc.scalars(dist, 4096, 64, plan))
        for K in (4, 36):
            T = mm.units_for(g.M, K)
            assert mm.chunk_len(g.M, T) == K
            by_fm = {fm: g.chunking(T, fm) for fm in (1, 2, 8, 64)}
            assert by_fm[1]["nbig"] == by_fm[1]["split"] > 0
            assert by_fm[64]["nbig"] == 1                       # bucket 0: the zero digits' dummies
            assert by_fm[1]["nbig"] >= by_fm[2]["nbig"] >= by_fm[8]["nbig"] >= 1
            if dist == "staircase":
                assert by_fm[1]["nbig"] > by_fm[2]["nbig"] > by_fm[64]["nbig"]
