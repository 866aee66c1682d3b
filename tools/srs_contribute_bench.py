"""Phase-1 contributions to a powers-of-tau string on one GPU (zk_srs_contribute
and zk_srs_verify_contribution), next to the host curve code.

One process, one ctx, a string from zk_srs_generate at each --log-n, shares
from SplitMix64:

  walks       n points times n scalars, the scalars a geometric progression s^i
              (the workload's distribution), over the first 2^16 and 2^20
              entries of tau_g1 and tau_g2: the table walk of csrc/mulvec.hpp
              (test library: g*_mul_scalars_table) against the plain per-lane
              255-bit walk (g*_mul_scalars_plain) on the same points and
              scalars, alternating; device time of the walk kernel alone
              (zk_ctx_profile), median of --runs after --warmup
  contribute  the whole zk_srs_contribute call on a host string (in place,
              again and again: every run is one more contribution): median of
              --runs wall times after --warmup, and the device time of its
              phases in the last run
  verify      the whole zk_srs_verify_contribution call (1 warm-up), and
              zk_srs_verify of the new string on its own
  host bar    the host curve code's full-width G1 multiplication on one thread
              (tools/contribute_bench.py host_mul_ms) x 4 N G1 multiplications
              + N G2 ones taken as 3 G1 ones each (an Fq2 product is three Fq
              products), over 16 CPUs -- reasoned, not measured.  A bar, not a
              measurement of a CPU implementation.

  python tools/srs_contribute_bench.py [--log-n 16 20] [--out profiles/srs_contribute_bench.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from contribute_bench import host_mul_ms, stats, wall  # noqa: E402


def progression(zkp, s, n):
    """s^i, i < n, as (n, 4) canonical words"""
    out = np.zeros((n, 4), dtype=np.uint64)
    v = 1
    for i in range(n):
        out[i] = zkp.to_limbs(v)
        v = v * s % zkp.R
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--walk-log-n", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "srs_contribute_bench.json"))
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs must be at least 5")

    zkp = importlib.import_module("zero-knowledge-proofs_amd")
    import pyref
    bid = zkp.check_build()
    rng = pyref.SplitMix64(0x51C0)
    tau, alpha, beta, s, a, b = (rng.fr() for _ in range(6))
    res = {"build": bid, "string": "zk_srs_generate, shares from SplitMix64(0x51C0)"}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")

    with zkp.Context(0) as ctx:
        h = C.c_void_p(ctx._h)
        top = max(args.log_n + args.walk_log_n)
        srs = zkp.SRS.generate(ctx, top, tau, alpha, beta)
        res["host_mul_ms"], res["host_mul_points"] = host_mul_ms(zkp, srs.tau_g1)
        print("host G1 mul", res["host_mul_ms"], "ms", flush=True)
        scal = progression(zkp, s, 1 << top)

        # ---- the walks alone: table against plain, alternating
        T = zkp.test_lib()
        for grp, src in (("g1", srs.tau_g1), ("g2", srs.tau_g2)):
            for lg in args.walk_log_n:
                m = 1 << lg
                pts = np.ascontiguousarray(src[:m])
                k = np.ascontiguousarray(scal[:m])
                outs = {}
                ms = {"table": [], "plain": []}
                order = ("table", "plain")
                for it in range(args.warmup + args.runs):
                    for walk in (order if it % 2 == 0 else order[::-1]):
                        name = "%s_mul_scalars_%s" % (grp, walk)
                        out = np.zeros_like(pts)
                        ctx.profile(0)
                        ctx.profile(1)
                        zkp._check(getattr(T, "zk_test_" + name)(h, zkp._p(pts), C.c_size_t(m), zkp._p(k), zkp._p(out)),
                                   ctx, name)
                        prof = ctx.profile_read()
                        outs[walk] = out
                        if it >= args.warmup:
                            ms[walk].append(prof[name]["ms"])
                ctx.profile(0)
                if not np.array_equal(outs["table"], outs["plain"]):
                    raise SystemExit("%s 2^%d: the two walks disagree" % (grp, lg))
                row = {w: stats(v) for w, v in ms.items()}
                row["points"] = m
                row["plain_over_table"] = row["plain"]["median_ms"] / row["table"]["median_ms"]
                # the slowest table run against the fastest plain one: the ship rule's margin
                row["plain_min_over_table_max"] = row["plain"]["min_ms"] / row["table"]["max_ms"]
                row["ns_per_point"] = {w: row[w]["median_ms"] * 1e6 / m for w in order}
                res["walk_%s_2p%d" % (grp, lg)] = row
                print("walk", grp, "2^%d" % lg, json.dumps(row), flush=True)
                save()
                del outs

        # ---- the whole calls
        for log_n in args.log_n:
            N = 1 << log_n
            work = srs.copy() if log_n == top else zkp.SRS.generate(ctx, log_n, tau, alpha, beta)
            before = work.copy()
            ws = work._bind()
            share = zkp._SRSShare()
            frs = [zkp._fr(v) for v in (s, a, b)]
            row = {"N": N}

            def contribute():
                zkp._check(zkp.lib().zk_srs_contribute(h, C.byref(ws), C.byref(frs[0]), C.byref(frs[1]),
                                                       C.byref(frs[2]), C.byref(share)), ctx, "zk_srs_contribute")
            contribute()                      # `work` is one contribution past `before` from here
            after = work.copy()
            after.beta_g2 = np.array(ws.beta_g2.w, dtype=np.uint64)
            sh = np.array([list(share.tau_g2.w), list(share.alpha_g2.w), list(share.beta_g2.w)], dtype=np.uint64)
            # the independent path: the fixed-base kernel over the multiplied secrets
            want = zkp.SRS.generate(ctx, log_n, tau * s % zkp.R, alpha * a % zkp.R, beta * b % zkp.R)
            for nm in ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2"):
                if not np.array_equal(getattr(after, nm), getattr(want, nm)):
                    raise SystemExit("2^%d: %s differs from generate with the multiplied secrets" % (log_n, nm))
            del want
            row["equals_generate"] = True
            row["contribute"] = wall(contribute, args.warmup, args.runs)
            ctx.profile(1)
            contribute()
            prof = ctx.profile_read()
            ctx.profile(0)
            row["contribute_phases_ms"] = {k: v["ms"] for k, v in prof.items()}
            row["contribute_cpu16_bar_ms"] = (4 * N + 3 * N) * res["host_mul_ms"] / 16

            co = zkp.fr_array([((rng.next() << 64) | rng.next()) or 1 for _ in range(2 * N)])

            def verify():
                st, sst = C.c_int(-1), C.c_int(-1)
                shs = zkp._SRSShare()
                for f, r in zip((shs.tau_g2, shs.alpha_g2, shs.beta_g2), sh):
                    for i, w in enumerate(r):
                        f.w[i] = int(w)
                zkp._check(zkp.lib().zk_srs_verify_contribution(h, C.byref(before._bind()), C.byref(after._bind()),
                                                                C.byref(shs), zkp._p(co), C.c_size_t(len(co)),
                                                                C.byref(st), C.byref(sst)), ctx, "verify_contribution")
                if st.value != zkp.ZK_SRSC_OK:
                    raise SystemExit("an honest contribution was refused: status %d / %d" % (st.value, sst.value))

            def verify_string():
                st = C.c_int(-1)
                zkp._check(zkp.lib().zk_srs_verify(h, C.byref(after._bind()), zkp._p(co), C.c_size_t(len(co)),
                                                   C.byref(st)), ctx, "srs_verify")
            row["verify_contribution"] = wall(verify, 1, args.runs)
            row["verify_string_alone"] = wall(verify_string, 0, args.runs)
            res["2p%d" % log_n] = row
            print("2^%d" % log_n, json.dumps(row), flush=True)
            save()


if __name__ == "__main__":
    main()
