"""The MSM's chunking, fixup and merge at the chunk lengths production runs
(csrc/msm.hip), and its grouping (csrc/group.hip) entry by entry.

The accumulate cuts the M grouped entries into chunks of K = ceil(M / T)
(rounded up to 4), T one full-occupancy round of the chip: every input the
suite can afford runs with K = 4, while a 2^20 .. 2^24 prove runs with K = 64
.. 1024 and a witness of zeros and ones that sends bucket 0 of every set
through several merge levels.  zk_test_msm_force sets T (and the fixup
threshold) from here, so that 4096 points reach those shapes; the kernels are
the shipped ones.  zk_test_msm_info / zk_test_msm_grouping read back what the
MSM did, and tests/msm_model.py says what it should have done.

Everything is bit-exact.  Expected sums are the oracle's (oracle.msm_g1 /
msm_g2), never the library's own unforced result; equality with that is
asserted in addition.  Every forced value is set through `forced`, which
restores (0, 0): the context is session-wide."""
import contextlib

import numpy as np
import pytest

import msm_cases as mc
import msm_model as mm
from helpers import skewed_witness

pytestmark = pytest.mark.gpu

R = mm.R


@contextlib.contextmanager
def forced(ctx, T=0, fix_max=0):
    """(T, fix_max) for the MSMs inside, (0, 0) again after them.  The
    workspaces are overwritten first: the cases repeat their inputs, and a
    bucket that a broken fixup or merge never writes would otherwise still
    hold the right sum from the run before."""
    ctx.test_msm_scrub()
    ctx.test_msm_force(T, fix_max)
    try:
        yield
    finally:
        ctx.test_msm_force(0, 0)


# ---- inputs, made once ---------------------------------------------------------
_bases, _uploads, _want, _groupings = {}, {}, {}, {}


def bases_of(oracle, g2, n):
    """n points with identities, P / -P neighbours and equal neighbours among
    them (with equal scalars they meet in one bucket, next to each other)."""
    key = (g2, n)
    if key not in _bases:
        if g2:
            g = oracle.g2_generator()
            pool = np.array([oracle.g2_mul(g, 0xB2 + 977 * i) for i in range(48)])
            b = pool[np.random.default_rng(64 + n).integers(0, 48, n)].copy()   # many equal points
            neg = oracle.g2_mul
        else:
            b = oracle.g1_lin_bases(0xDEADBEEF, 0xC0FFEE, n).copy()
            neg = oracle.g1_mul
        for i in range(3, n, 41):
            b[i] = 0
            b[i, -1] = 1                                   # the identity
        for i in (10, 500, 1000, 2500):
            if i + 1 < n:
                b[i + 1] = neg(b[i], R - 1)                # P, -P
        for i in (20, 700, 3000):
            if i + 1 < n:
                b[i + 1] = b[i]                            # P, P
        _bases[key] = b
    return _bases[key]


def scalars_of(plan_name, n, dist):
    plan = mc.make_plan(plan_name, n)
    return plan, mc.scalars(dist, n, plan.bits, plan)


def grouping_of(plan_name, n, dist):
    key = (plan_name, n, dist)
    if key not in _groupings:
        plan, sc = scalars_of(plan_name, n, dist)
        _groupings[key] = (plan, sc, mm.Grouping(plan, sc))
    return _groupings[key]


def want_of(oracle, g2, n, bits, dist, sc):
    key = (g2, n, bits, dist)
    if key not in _want:
        _want[key] = (oracle.msm_g2 if g2 else oracle.msm_g1)(bases_of(oracle, g2, n), sc)
    return _want[key]


def run_msm(ctx, oracle, g2, plan_name, n, sc):
    """The public MSM call that runs the plan: zk_msm_* for the per-window
    plans, else zk_msm_*_dev over an upload with the plan's copies."""
    kind, bits, copies = mc.PLANS[plan_name]
    b = bases_of(oracle, g2, n)
    if kind == "window":
        return (ctx.msm_g2 if g2 else ctx.msm_g1)(b, sc, bits)
    key = (g2, plan_name, n)
    if key not in _uploads:
        _uploads[key] = ctx.msm_upload(b, g2=g2, scalar_bits=bits, copies=copies)
    return _uploads[key].msm(sc, bits)


@pytest.fixture(scope="module", autouse=True)
def _free_uploads(ctx):
    yield
    ctx.test_msm_force(0, 0)
    for h in _uploads.values():
        h.free()
    for d in (_uploads, _bases, _want, _groupings):
        d.clear()


def check_plan(info, plan, n):
    """The device ran the plan the model assumed (its c above all)."""
    for name, want in (("c", plan.c), ("nwin", plan.nwin), ("bits", plan.bits), ("sw", plan.sw), ("shared", plan.shared),
                       ("G", plan.G), ("n", n), ("nseg", 1),
                       ("nred", plan.nwin if plan.kind == "window" else plan.nsets)):
        assert info[name] == want, (name, info[name], want)
    if plan.shared:
        assert info["copies"] == plan.copies


# ---- the hooks -----------------------------------------------------------------
def test_force_arguments_and_natural_units(zkp, ctx, oracle):
    """T above 2^22 is refused and changes nothing; the natural T is what an
    unforced MSM runs with, whatever was forced before, and is reported for
    both curves (one full-occupancy round: about 3 waves per SIMD of one-lane
    G1 units, 1 wave of G2 lane pairs)."""
    with pytest.raises(ValueError):
        ctx.test_msm_force((1 << 22) + 1, 0)
    b, sc = bases_of(oracle, False, 65), mc.scalars("uniform", 65, 64)
    want = oracle.msm_g1(b, sc)
    with forced(ctx, 1 << 22, 1):
        pass                                               # the largest T the hook takes
    with forced(ctx, 300000, 3):                           # more units than the chip holds at once
        assert np.array_equal(ctx.msm_g1(b, sc, 64), want)
        i = ctx.test_msm_info(0)
        assert (i["T"], i["fix_max"]) == (300000, 3)
    with forced(ctx, 7, 0):
        assert np.array_equal(ctx.msm_g1(b, sc, 64), want)
        i = ctx.test_msm_info(0)
        assert (i["T"], i["fix_max"]) == (7, mm.FIX_MAX)
    assert np.array_equal(ctx.msm_g1(b, sc, 64), want)
    g1 = ctx.test_msm_info(0, g2=False)
    g2 = ctx.test_msm_info(0, g2=True)
    assert g1["T"] == g1["natural_T"] and g1["fix_max"] == mm.FIX_MAX
    assert g1["natural_T"] % 128 == 0 and g2["natural_T"] % 64 == 0 and g1["natural_T"] > g2["natural_T"] >= 1024
    print(f"\nnatural accumulate units: G1 {g1['natural_T']}, G2 {g2['natural_T']}")
    with pytest.raises(ValueError):
        ctx.test_msm_info(7)


# ---- a. the grouping against the model -------------------------------------------
# (curve, plan, sizes): around the 64-point rounds, around one 8192-entry tile of
# the plan's window count, and several tiles
def _tile_points(plan_name, n_near):
    return -(-8192 // mc.make_plan(plan_name, n_near).nwin)


GROUPING = [(0, "W64", 1024), (0, "W255", 161), (0, "S64", 2048), (0, "S255", 631), (0, "G255x3", 631),
            (0, "G255x5", 631), (1, "S64", 2048)]
GROUPING_CASES = [(g2, plan, n) for g2, plan, tile in GROUPING
                  for n in (1, 63, 64, 65, tile - 1, tile, tile + 1, 5000)]


@pytest.mark.parametrize("g2,plan_name,n", GROUPING_CASES,
                         ids=[f"{'g2' if g else 'g1'}-{p}-{n}" for g, p, n in GROUPING_CASES])
def test_grouping_equals_the_model(ctx, oracle, g2, plan_name, n):
    """off[], M, and per bucket the multiset of entries are the model's, for
    random, edge and {0, 1}-skewed scalars (zeros among them); the keys are
    sorted; the order inside a bucket is the same bytes on a second run."""
    for g_, p_, tile in GROUPING:
        if (g_, p_) == (g2, plan_name) and n in (tile - 1, tile, tile + 1):
            assert _tile_points(plan_name, n) == tile       # the sizes do sit at the plan's tile edge
    for dist in ("uniform", "edges", "skewed"):
        plan, sc = scalars_of(plan_name, n, dist)
        model = mm.Grouping(plan, sc)
        run_msm(ctx, oracle, g2, plan_name, n, sc)
        info = ctx.test_msm_info(0, g2)
        check_plan(info, plan, n)
        assert info["T"] == info["natural_T"] and info["M"] == model.M, (dist, info["M"], model.M)
        off, key, ent = ctx.test_msm_grouping(0)
        assert np.array_equal(off, model.off), dist
        assert (np.diff(key.astype(np.int64)) >= 0).all(), dist
        ck, ce = mm.canonical(key, ent)
        assert np.array_equal(ck, model.key) and np.array_equal(ce, model.ent), dist
        run_msm(ctx, oracle, g2, plan_name, n, sc)
        off2, key2, ent2 = ctx.test_msm_grouping(0)
        assert off.tobytes() == off2.tobytes() and key.tobytes() == key2.tobytes() and ent.tobytes() == ent2.tobytes()


# ---- b. the chunk-length sweep ---------------------------------------------------
def device_chunking(info, off):
    """The model's chunking record rebuilt from the device's own readbacks."""
    K = mm.chunk_len(info["M"], info["T"])
    o = off.astype(np.int64)
    P = np.where(o[1:] > o[:-1], (o[1:] - 1) // K - o[:-1] // K + 1, 0)
    return {"K": K, "T": info["T"], "nbig": info["nbig"], "max_span": int(P.max()), "split": int((P > 1).sum()),
            "by_boundary": info["G"] > info["T"], "nlevels": mm.merge_levels(info["T"]), "spans": P}


def run_forced_case(ctx, oracle, case, T, fm_arg, fm):
    """One MSM under (T, fix_max): the oracle's point, and M, T, nbig as the model has them."""
    plan, sc, model = grouping_of(case.plan, case.n, case.dist)
    want = want_of(oracle, case.g2, case.n, plan.bits, case.dist, sc)
    ch = model.chunking(T, fm)
    with forced(ctx, T, fm_arg):
        got = run_msm(ctx, oracle, case.g2, case.plan, case.n, sc)
        info = ctx.test_msm_info(0, case.g2)
        off, key, ent = ctx.test_msm_grouping(0)
    tag = mc.case_id(case)
    check_plan(info, plan, case.n)
    assert (info["M"], info["T"], info["fix_max"]) == (model.M, T, fm), tag
    assert np.array_equal(off, model.off), tag                       # else: the grouping
    assert info["nbig"] == ch["nbig"], (tag, info["nbig"], ch["nbig"])   # else: the fixup's count
    assert np.array_equal(got, want), tag                            # else: accumulate, fixup sums or merge
    return info, off, ch


@pytest.mark.parametrize("case", mc.SWEEP, ids=mc.case_id)
def test_chunk_length_sweep(ctx, oracle, case):
    plan, sc, model = grouping_of(case.plan, case.n, case.dist)
    T, fm, K, ch = mc.resolve(case, model)               # asserts chunk_len(M, T) == K
    mc.check_want(case, ch, fm)                          # the model's view (test_msm_model.py, again)
    info, off, _ = run_forced_case(ctx, oracle, case, T, case.fix_max, fm)
    dch = device_chunking(info, off)
    assert dch["K"] == K
    mc.check_want(case, dch, fm)                         # the device's view
    # and the unforced run of the same inputs: the same point
    want = want_of(oracle, case.g2, case.n, plan.bits, case.dist, sc)
    ctx.test_msm_scrub()
    assert np.array_equal(run_msm(ctx, oracle, case.g2, case.plan, case.n, sc), want)
    after = ctx.test_msm_info(0, case.g2)
    assert after["T"] == after["natural_T"] and after["fix_max"] == mm.FIX_MAX      # nothing leaked


# ---- c. the fixup / merge threshold ------------------------------------------------
@pytest.mark.parametrize("fix_max", [1, 2, 0, 64], ids=["fm1", "fm2", "rule", "fm64"])
@pytest.mark.parametrize("K", [4, 36])
@pytest.mark.parametrize("dist", ["staircase", "ones"])
@pytest.mark.parametrize("g2", [0, 1], ids=["g1", "g2"])
def test_fix_max(ctx, oracle, g2, dist, K, fix_max):
    """The same sums wherever the threshold sits: with 1 every split bucket
    goes through the merge, with 64 only bucket 0 (the zero digits' dummies)."""
    case = mc.Case(g2, "S64", 1024 if g2 else 4096, dist, K, fix_max, 0, ())
    plan, sc, model = grouping_of(case.plan, case.n, case.dist)
    T, fm, K_, ch = mc.resolve(case, model)
    assert K_ == K
    info, off, ch = run_forced_case(ctx, oracle, case, T, fix_max, fm)
    if fix_max == 1:
        assert info["nbig"] == ch["split"] > 0
    if fix_max == 64:
        assert info["nbig"] == 1
    if dist == "staircase":
        assert ch["split"] > 1                      # many buckets on either side of the threshold, not bucket 0 alone


# ---- d. prove under forced units -----------------------------------------------------
LOG_N = 10
UNITS = (0, 64, 1000, 20000)
SLOT_A, SLOT_B2, SLOT_H = 0, 1, 4


def _witness(oracle, n, kind):
    return oracle.synthetic_witness(n, 1234) if kind == "random" else skewed_witness(n, kind, 11)


def _device_z(z):
    import torch
    return torch.from_numpy(np.ascontiguousarray(z).view(np.int64).copy()).cuda()


@pytest.fixture(scope="module")
def circuit(zkp, oracle, pyref):
    n = 1 << LOG_N
    rng = pyref.SplitMix64(0xC4A2C5)
    return {"n": n, "qap": zkp.QAP(zkp.CSRMatrices.synthetic(n)), "csr_o": oracle.CSR.synthetic(n),
            "params": [rng.fr() for _ in range(5)], "r": rng.fr(), "s": rng.fr()}


@pytest.fixture(scope="module")
def reference_key(zkp, ctx, oracle, circuit):
    rc, opk, _ = oracle.setup(circuit["csr_o"], circuit["params"], 1, nthreads=8)
    assert rc == 0
    dpk = zkp.CRS.generate_device(ctx, circuit["qap"], zkp.SetupParams(*circuit["params"]), 1)
    yield opk, dpk
    dpk.free()


@pytest.mark.parametrize("kind", ["random", "bits", "ones"])
def test_prove_reference_key_under_forced_units(zkp, ctx, oracle, circuit, reference_key, kind):
    """A reference-mode key: one-word scalars, A + B1 as ONE batch of two
    segments (nseg = 2) and IC + H as a batch of one, pi_B a shared G2 plan.
    A device witness runs every MSM whole; a host witness runs pi_B and A + B1
    in two parts, MSM_BACK_FIXUP on the first part's workspace and then
    MSM_BACK_COMBINE.  (HOST_PARTS = 2 in this build: no middle part, so
    MSM_BACK_ACCUM is not reachable and not covered.)  The proof is the
    oracle's for every T."""
    opk, dpk = reference_key
    z = _witness(oracle, circuit["n"], kind)
    dz = _device_z(z)
    r, s = circuit["r"], circuit["s"]
    rc, want = oracle.prove(opk, circuit["csr_o"], z, 1, r, s)
    assert rc == 0
    for T in UNITS:
        with forced(ctx, T, 0):
            host = zkp.Prover.prove(dpk, zkp.Witness(z, 1), r=r, s=s)
            parts = [ctx.test_msm_info(zkp.TEST_MSM_PART_G2, True), ctx.test_msm_info(zkp.TEST_MSM_PART_ABI)]
            last = [ctx.test_msm_info(SLOT_B2, True), ctx.test_msm_info(SLOT_A)]
            dev = zkp.Prover.prove_device(dpk, dz.data_ptr(), len(z), 1, r, s)
            ab, b2, ich = (ctx.test_msm_info(k, k == SLOT_B2) for k in (SLOT_A, SLOT_B2, SLOT_H))
        assert np.array_equal(host.words, want), (kind, T, "host witness")
        assert np.array_equal(dev.words, want), (kind, T, "device witness")
        assert (ab["nseg"], ich["nseg"], b2["nseg"], ab["shared"], ab["sw"]) == (2, 1, 1, 1, 1)
        for i in (ab, b2, ich, *parts, *last):
            assert i["T"] == (T or i["natural_T"]) and i["c"] == 16 and i["nwin"] == 4
        # the two parts of a host witness are MSMs of their own, over fewer points each
        assert parts[1]["nseg"] == last[1]["nseg"] == 2
        assert 0 < parts[1]["n"] < ab["n"] and parts[1]["n"] + last[1]["n"] == ab["n"]
        assert 0 < parts[0]["n"] < b2["n"] and parts[0]["n"] + last[0]["n"] == b2["n"]
        if kind != "random" and T:
            # bucket 0 of every set holds the zeros' and ones' entries: many chunks, the merge runs
            assert min(ab["nbig"], b2["nbig"], ich["nbig"], parts[1]["nbig"], last[1]["nbig"]) >= 1, (kind, T)
    assert np.array_equal(zkp.Prover.prove_device(dpk, dz.data_ptr(), len(z), 1, r, s).words, want)
    after = ctx.test_msm_info(SLOT_A)
    assert after["T"] == after["natural_T"] and after["fix_max"] == mm.FIX_MAX


def _g1(pyref, words):
    w = [int(x) for x in words]
    if w[12]:
        return pyref.INF
    return (pyref.Fq1(sum(w[i] << (64 * i) for i in range(6))), pyref.Fq1(sum(w[6 + i] << (64 * i) for i in range(6))))


def _g2(pyref, words):
    w = [int(x) for x in words]
    if w[24]:
        return pyref.INF
    c = [sum(w[6 * k + i] << (64 * i) for i in range(6)) for k in range(4)]
    return (pyref.Fq2(c[0], c[1]), pyref.Fq2(c[2], c[3]))


@pytest.fixture(scope="module")
def sound_crs(zkp, ctx, circuit):
    return zkp.CRS.generate_from_qap(ctx, circuit["qap"], zkp.SetupParams(*circuit["params"]), 1, sound=True)


@pytest.mark.parametrize("kind", ["random", "bits", "ones"])
@pytest.mark.parametrize("copies", [0, 3], ids=["all-copies", "3-copies"])
def test_prove_sound_key_under_forced_units(zkp, ctx, oracle, pyref, circuit, sound_crs, copies, kind):
    """A sound key: four-word scalars, one grouped-window MSM per slot (13
    windows of c = 20; with ZK_OPT_SOUND_COPIES = 3 five bucket sets).  The
    oracle has no sound prover, so the expected proof is pinned down in two
    steps that do not pass through the MSM kernels: pi_A and pi_B are the
    oracle's MSMs over the host key plus pyref additions of the extras, and
    pi_C is the only point that satisfies the pairing equation with them (the
    host verifier).  Every forced proof must then be those bytes."""
    crs = sound_crs
    z = _witness(oracle, circuit["n"], kind)
    dz = _device_z(z)
    r, s = circuit["r"], circuit["s"]
    ctx.set_option(zkp.ZK_OPT_SOUND_COPIES, copies)
    try:
        dpk = zkp.CRS.generate_device(ctx, circuit["qap"], zkp.SetupParams(*circuit["params"]), 1, sound=True)
    finally:
        ctx.set_option(zkp.ZK_OPT_SOUND_COPIES, 0)
    try:
        assert dpk.test_plan() == ((3, 5) if copies else (13, 1))
        want = zkp.Prover.prove_device(dpk, dz.data_ptr(), len(z), 1, r, s)
        a = pyref.G1.add(_g1(pyref, oracle.msm_g1(crs.pk.a_g1, z)), _g1(pyref, crs.pk.point("alpha_g1")))
        a = pyref.G1.add(a, pyref.G1.mul(_g1(pyref, crs.pk.point("delta_g1")), r))
        b = pyref.G2.add(_g2(pyref, oracle.msm_g2(crs.pk.b_g2, z)), _g2(pyref, crs.pk.point("beta_g2")))
        b = pyref.G2.add(b, pyref.G2.mul(_g2(pyref, crs.pk.point("delta_g2")), s))
        assert list(want.a) == pyref.g1_words(a) and list(want.b) == pyref.g2_words(b)
        assert zkp.Verifier.verify(crs.vk, want, [zkp.from_limbs(z[1])]) is True
        for T in UNITS:
            with forced(ctx, T, 0):
                host = zkp.Prover.prove(dpk, zkp.Witness(z, 1), r=r, s=s)      # a sound key sends it up whole
                dev = zkp.Prover.prove_device(dpk, dz.data_ptr(), len(z), 1, r, s)
                infos = [ctx.test_msm_info(k, k == SLOT_B2) for k in (SLOT_A, SLOT_B2, 2, SLOT_H)]
            assert np.array_equal(dev.words, want.words), (kind, copies, T, "device witness")
            assert np.array_equal(host.words, want.words), (kind, copies, T, "host witness")
            for i in infos:
                assert i["T"] == (T or i["natural_T"]) and (i["c"], i["nwin"], i["sw"], i["nseg"]) == (20, 13, 4, 1)
                assert i["nred"] == (5 if copies else 1) and i["copies"] == (3 if copies else 13)
                assert i["G"] > i["T"]                               # 2^19 buckets a set: the fixup by boundary
            if kind != "random" and T:
                assert all(i["nbig"] >= 1 for i in infos), (kind, copies, T)
    finally:
        dpk.free()
