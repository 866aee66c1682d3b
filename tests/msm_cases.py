"""Inputs and the case table of the MSM chunking tests (test_msm_model.py on
the CPU, test_gpu_msm_chunks.py on the GPU): the plans the public MSM calls
reach, deterministic scalar distributions, and for every case of the
chunk-length sweep what it must reach -- asserted from the model on the CPU
(so the table cannot go vacuous) and again from the device's readbacks."""
from collections import namedtuple

import numpy as np

import msm_model as mm

# ---- the plans behind the public MSM calls -------------------------------
# name -> (model kind, scalar bits, copies): W* zk_msm_g1 / zk_msm_g2 (one
# bucket range per window, c by the cost rule), S* the window upload (c = 16
# up to 64 bits, else 20; every copy, one bucket set), G*x<k> upload_copies
# with k copies.
PLANS = {"W64": ("window", 64, 0), "W255": ("window", 255, 0), "S64": ("shared", 64, 0), "S255": ("shared", 255, 0),
         "G64x3": ("grouped", 64, 3), "G255x3": ("grouped", 255, 3), "G255x5": ("grouped", 255, 5)}
# The c msm_make_plan's cost rule picks for n points, tabulated once from the
# rule (first n of every width): the table's assumption, which the GPU tests
# compare with the c the device reports.
WINDOW_C = {64: ((1, 4), (84, 5), (224, 6), (847, 7), (1005, 8)),
            255: ((1, 4), (87, 5), (228, 6), (560, 7), (1249, 8), (3594, 9))}


def plan_c(name, n):
    kind, bits, _ = PLANS[name]
    if kind != "window":
        return 16 if bits == 64 else 20
    assert 1 <= n <= 5000
    return [c for n0, c in WINDOW_C[bits] if n >= n0][-1]


def make_plan(name, n):
    kind, bits, copies = PLANS[name]
    return mm.Plan(kind, bits, plan_c(name, n), copies=copies)


# ---- scalars ---------------------------------------------------------------
def _random(n, bits, rng):
    sc = rng.integers(0, 1 << 63, (n, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (n, 4), dtype=np.uint64)
    sc[:, 3] >>= np.uint64(2)          # below 2^254 < r
    if bits == 64:
        sc[:, 1:] = 0
    return sc


def edge_scalars(bits, c, nwin):
    """test_gpu_msm_copies._edge_scalars for any window width: 0, 1, the
    digits around 2^(c-1), the widest values, a carry through every window and
    the largest digits that do not carry."""
    half = 1 << (c - 1)

    def every(d):
        return sum(d << (c * w) for w in range(nwin - 1))

    wide = (mm.R - 1, 1 << 254) if bits == 255 else ((1 << 64) - 1, 1 << 63)
    vals = [0, 1, (1 << c) - 1, half, half + 1, *wide, every(half + 1), every(half)]
    return [v for v in vals if v < (1 << bits) and v < mm.R]


def staircase_len(n):
    """The largest J with 1 + 2 + ... + J <= n."""
    J = 1
    while (J + 1) * (J + 2) // 2 <= n:
        J += 1
    return J


def scalars(dist, n, bits, plan=None, seed=1):
    """(n, 4) uint64 canonical scalars below 2^bits and below r.
      uniform     whole random scalars
      ones        1 everywhere
      bits01      0 or 1
      onevalue    one value with a different digit in every window
      sparse      zero but for every 37th, a whole random scalar
      skewed      {0, 1} with every 29th a whole random scalar, some runs of zeros
      staircase   value j + 1 (bucket j of window 0) j times, j = 1 .. J, then zeros
      edges       edge_scalars of the plan, repeated"""
    rng = np.random.default_rng(0xC0FFEE + 1000003 * seed + n)
    sc = np.zeros((n, 4), dtype=np.uint64)
    if dist == "uniform":
        sc = _random(n, bits, rng)
    elif dist == "ones":
        sc[:, 0] = 1
    elif dist == "bits01":
        sc[:, 0] = rng.integers(0, 2, n, dtype=np.uint64)
    elif dist == "onevalue":
        v = 0x6B3A59C4D2E1F087 if bits == 64 else 0x2B3A59C4D2E1F0873C5D7E9FA1B2C4D6E8F00112233445566778899AABBCCDD
        sc[:] = mm.limbs_of([v])
    elif dist == "sparse":
        sc[::37] = _random(len(sc[::37]), bits, rng)
    elif dist == "skewed":
        sc[:, 0] = rng.integers(0, 2, n, dtype=np.uint64)
        sc[::29] = _random(len(sc[::29]), bits, rng)
        sc[5:n // 7] = 0
    elif dist == "staircase":
        J = staircase_len(n)
        vals = np.repeat(np.arange(1, J + 1, dtype=np.uint64), np.arange(1, J + 1)) + np.uint64(1)
        sc[:len(vals), 0] = vals
    elif dist == "edges":
        ev = edge_scalars(bits, plan.c, plan.nwin)
        sc[:] = mm.limbs_of([ev[i % len(ev)] for i in range(n)])
    else:
        raise ValueError(dist)
    return sc


# ---- the chunk-length sweep -------------------------------------------------
# curve g2, plan name, n, dist, the chunk length K the case must run with,
# fix_max (0: the rule), T (0: derived, ceil(M / K); else given -- more units
# than chunks keep K = 4, the unforced shape), and what the case is in the
# table for, every word of `want` a condition on the model's chunking:
#   merge    nbig > 0              merge2 / merge3   largest span > 16 / > 64
#   fixup    nbig == 0 and some bucket split over 2 .. fix_max chunks
#   edge     a bucket of exactly fix_max and one of exactly fix_max + 1 chunks
#   bb / nobb   G > T / G <= T     T=<k>   the units are exactly k
Case = namedtuple("Case", "g2 plan n dist K fix_max T want")
TARGET_K = (4, 8, 12, 16, 20, 32, 36, 64, 260)


def _c(g2, plan, n, dist, K, want, fix_max=0, T=0):
    return Case(g2, plan, n, dist, K, fix_max, T, tuple(want.split()))


SWEEP = [
    # G1, 4096 points.  The window upload at 64 bits: M = 16384 whatever the scalars
    _c(0, "S64", 4096, "ones", 4, "merge merge3 bb"),
    _c(0, "S64", 4096, "ones", 64, "merge merge3 bb"),
    _c(0, "S64", 4096, "bits01", 36, "merge merge3 bb"),
    _c(0, "S64", 4096, "onevalue", 20, "merge merge3"),
    _c(0, "S64", 4096, "uniform", 4, "fixup bb"),
    _c(0, "S64", 4096, "uniform", 4, "fixup nobb", T=70000),
    _c(0, "S64", 4096, "uniform", 8, "fixup"),
    _c(0, "S64", 4096, "uniform", 12, "fixup"),
    _c(0, "S64", 4096, "uniform", 16, "fixup"),
    _c(0, "S64", 4096, "uniform", 32, "fixup"),
    _c(0, "S64", 4096, "sparse", 8, "merge merge3"),
    _c(0, "S64", 4096, "staircase", 4, "merge merge3 edge"),
    _c(0, "S64", 4096, "staircase", 8, "merge edge"),
    _c(0, "S64", 4096, "staircase", 12, "merge edge", fix_max=4),
    _c(0, "S64", 4096, "staircase", 16, "merge edge", fix_max=2),
    _c(0, "S64", 4096, "staircase", 20, "merge edge", fix_max=3),
    _c(0, "S64", 4096, "staircase", 32, "merge edge", fix_max=2),
    _c(0, "S64", 4096, "staircase", 36, "merge edge", fix_max=1),
    _c(0, "S64", 4096, "staircase", 64, "merge edge", fix_max=1),
    # units that are no power of 4, and one chunk (no merge launch)
    _c(0, "S64", 65, "ones", 260, "T=1", fix_max=1),
    _c(0, "S64", 65, "uniform", 260, "T=1"),
    _c(0, "S64", 130, "ones", 260, "merge T=2", fix_max=1),
    _c(0, "S64", 195, "ones", 260, "merge T=3", fix_max=2),
    _c(0, "S64", 325, "skewed", 260, "merge T=5", fix_max=2),
    _c(0, "S64", 272, "ones", 64, "merge merge2 T=17"),
    _c(0, "S64", 272, "staircase", 64, "merge T=17", fix_max=1),
    _c(0, "W64", 256, "uniform", 0, "T=1"),           # K: whatever one chunk of its M is
    # two bucket sets (64 bits over 3 copies), and the full-width uploads
    _c(0, "G64x3", 4096, "skewed", 16, "merge merge3 bb"),
    _c(0, "G64x3", 4096, "uniform", 4, "fixup nobb", T=140000),
    _c(0, "S255", 4096, "ones", 32, "merge merge3 bb"),
    _c(0, "S255", 4096, "uniform", 16, "fixup bb"),
    _c(0, "S255", 4096, "staircase", 8, "merge merge3 edge"),
    _c(0, "G255x3", 4096, "bits01", 20, "merge merge3 bb"),
    _c(0, "G255x3", 4096, "onevalue", 12, "merge merge3"),
    _c(0, "G255x5", 4096, "staircase", 4, "merge merge3 edge"),
    _c(0, "G255x5", 4096, "uniform", 64, "fixup bb"),
    # zk_msm_g1: per-window buckets, M = the non-zero digits
    _c(0, "W64", 4096, "uniform", 4, "merge nobb"),
    _c(0, "W64", 4096, "uniform", 64, "fixup bb"),
    _c(0, "W64", 4096, "staircase", 8, "merge edge", fix_max=2),
    _c(0, "W64", 4096, "bits01", 12, "merge merge3"),
    _c(0, "W64", 4096, "onevalue", 36, "merge merge3 bb"),
    _c(0, "W255", 4096, "ones", 16, "merge merge3 bb"),
    _c(0, "W255", 4096, "ones", 64, "merge merge2 bb"),
    _c(0, "W255", 4096, "uniform", 260, "fixup bb"),
    _c(0, "W255", 4096, "sparse", 20, "fixup bb", fix_max=64),
    # G2, 1024 points (a lane pair per point)
    _c(1, "S64", 1024, "ones", 4, "merge merge3 bb"),
    _c(1, "S64", 1024, "staircase", 8, "merge merge3 edge", fix_max=2),
    _c(1, "S64", 1024, "uniform", 16, "fixup bb"),
    _c(1, "S64", 1024, "uniform", 4, "fixup nobb", T=66000),
    _c(1, "S64", 1024, "bits01", 36, "merge merge3"),
    _c(1, "S64", 1024, "onevalue", 20, "merge merge2"),
    _c(1, "S64", 1024, "skewed", 12, "merge merge3"),
    _c(1, "G255x3", 1024, "sparse", 32, "merge merge3 bb"),
    _c(1, "S255", 1024, "staircase", 64, "merge merge3 edge", fix_max=1),
    _c(1, "W64", 1024, "uniform", 64, "fixup bb"),
    _c(1, "W255", 1024, "skewed", 8, "merge merge2"),
    _c(1, "S64", 5, "uniform", 20, "T=1"),
    _c(1, "S64", 9, "ones", 36, "T=1", fix_max=1),
    _c(1, "S64", 16, "skewed", 64, "T=1"),
    _c(1, "S64", 34, "ones", 8, "merge merge2 T=17"),
    _c(1, "S64", 15, "ones", 12, "merge T=5", fix_max=2),
]
# T = 1 is a serial chain of n nwin dependent adds on one unit: small inputs only
G1_T1_MAX, G2_T1_MAX = 256, 64


def case_id(c):
    t = f"-T{c.T}" if c.T else ""
    return f"{'g2' if c.g2 else 'g1'}-{c.plan}-{c.n}-{c.dist}-K{c.K}-fm{c.fix_max or 'rule'}{t}"


def resolve(case, grouping):
    """(T, fix_max, K, chunking) of a case for the model's grouping of its
    inputs; asserts that the forced T gives the case's K."""
    fm = case.fix_max or mm.FIX_MAX
    K = case.K or mm.chunk_len(grouping.M, 1)
    T = case.T or mm.units_for(grouping.M, K)
    assert mm.chunk_len(grouping.M, T) == K, (case_id(case), grouping.M, T, mm.chunk_len(grouping.M, T))
    return T, fm, K, grouping.chunking(T, fm)


def check_want(case, ch, fm):
    """Every condition the table names for the case holds for the chunking
    ch (the model's, or one rebuilt from the device's readbacks)."""
    P = ch["spans"]
    cid = case_id(case)
    for wd in case.want:
        if wd == "merge":
            assert ch["nbig"] > 0, cid
        elif wd == "merge2":
            assert ch["nbig"] > 0 and ch["max_span"] > 16, (cid, ch["max_span"])
        elif wd == "merge3":
            assert ch["nbig"] > 0 and ch["max_span"] > 64, (cid, ch["max_span"])
        elif wd == "fixup":
            assert ch["nbig"] == 0 and ch["split"] > 0 and 2 <= ch["max_span"] <= fm, (cid, ch["max_span"], ch["split"])
        elif wd == "edge":
            assert (P == fm).any() and (P == fm + 1).any(), cid
        elif wd == "bb":
            assert ch["by_boundary"], cid
        elif wd == "nobb":
            assert not ch["by_boundary"], cid
        elif wd.startswith("T="):
            assert ch["T"] == int(wd[2:]), (cid, ch["T"])
        else:
            raise ValueError(wd)
    if ch["T"] == 1:
        assert case.n <= (G2_T1_MAX if case.g2 else G1_T1_MAX), cid
