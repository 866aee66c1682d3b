"""A sound key from a powers-of-tau string (zk_groth16_setup_srs_sound) on one
GPU, beside the trusted sound setup it must equal (zk_groth16_setup_sound).

One process, one ctx, the synthetic circuit n x (x*y = z) at each --log-n, a
string of exactly that size from known secrets:

  setup     the whole CRS.from_srs call and the whole CRS.generate_from_qap
            (sound, gamma = delta = 1) call, alternating: median of --runs wall
            times each after --warmup; the two keys are compared once
  phases    the device time of one profiled from_srs call (zk_ctx_profile): the
            three G1 inverse transforms, the G2 one, the four column sums and
            the H differences
  map       zk_g1_ntt / zk_g2_ntt (inverse) over the string's first n powers
            under ZK_OPT_GNTT_MAP = 1 (a wave shares its twiddle wherever a
            stage has 64 or more butterflies per twiddle) and 0 (a twiddle per
            lane in every stage), alternating: device time of the transform
            phase, median of --runs after --warmup
  run       the column sums of the same circuit with variable 0 added to every
            row of C (the constant-one column of a real circuit: one column of
            n entries) under each ZK_OPT_SRS_RUN of --srs-runs (0: the
            default, the power of two at or above sqrt(n)), the candidates in
            turn --runs times: device time of the ic column sum
  host bar  the host curve code's full-width G1 multiplication on one thread
            (tools/contribute_bench.py host_mul_ms) x the transforms'
            multiplication count, over 16 CPUs: 3 G1 transforms and one G2
            transform of (n / 2) (log n - 1) + n multiplications each (a stage's
            first twiddle is 1; the n are the 1 / n scaling), a G2
            multiplication taken as 3 G1 ones (an Fq2 product is three Fq
            products) -- reasoned, not measured.  A bar, not a measurement of
            a CPU implementation.

  python tools/srs_setup_bench.py [--log-n 16 20] [--out profiles/srs_setup_bench.json]

--prepared measures the prepared strings instead (zk_srs_prepare and what reads
its handle), in one process per size, every call in turn within one iteration
and the order reversed every other iteration, median of --runs wall times after
--warmup:

  prepare               SRS.prepare (the four inverse transforms and the H
                        differences, kept on the device)
  from_prepared         CRS.from_prepared, a host key
  from_prepared_device  CRS.from_prepared_device, a device key
  from_srs              CRS.from_srs, the host key from the monomial string
  from_srs_upload       CRS.from_srs and DeviceProvingKey.upload of its key
  lagrange_verify       LagrangeSRS.verify of the exported handle, drawn coefficients
  phases                one profiled call of each (zk_ctx_profile); srs_csc_host is
                        the host's CSC builds; prepared_* and lag_* are host wall
                        times too, each ending in a synchronise (the key's download
                        and the copy into the caller's arrays; the device key's
                        matrices, its slots and pk_finish; the check's validation
                        and its MSMs over either form)

  python tools/srs_setup_bench.py --prepared [--log-n 16 20] [--out profiles/srs_prepared_bench.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from contribute_bench import host_mul_ms, stats  # noqa: E402

PHASES = ("srs_ntt_g1_tau", "srs_ntt_g1_alpha", "srs_ntt_g1_beta", "srs_ntt_g2", "srs_colsum_a_g1", "srs_colsum_b_g1",
          "srs_colsum_b_g2", "srs_colsum_ic", "srs_hdiff")
PK_ARRAYS = ("a_g1", "b_g1", "b_g2", "ic_g1", "h_g1")
COLSUMS = ("srs_csc_host", "srs_colsum_a_g1", "srs_colsum_b_g1", "srs_colsum_b_g2", "srs_colsum_ic")
HOST_KEY = COLSUMS + ("prepared_download", "prepared_fill_host")
DEV_KEY = COLSUMS + ("prepared_dev_create", "prepared_dev_fill", "prepared_dev_finish")
LAG_PHASES = ("lag_validate", "lag_scalars", "lag_msm_lagrange", "lag_msm_srs", "srs_hdiff")


def prepared(args, zkp, pyref, bid):
    rng = pyref.SplitMix64(0x5255)
    tau, alpha, beta = rng.fr(), rng.fr(), rng.fr()
    res = {"build": bid, "circuit": "synthetic n x (x*y=z), num_public 1, sound keys, gamma = delta = 1",
           "method": "one process per record, one ctx; wall ms, median of %d after %d warm-up, the calls in turn "
                     "and the order reversed every other iteration" % (args.runs, args.warmup)}
    if os.path.exists(args.out):           # sizes measured by earlier calls stay
        with open(args.out) as f:
            old = json.load(f)
        if old.get("build") == bid:
            res = old
    with zkp.Context(0) as ctx:
        def profiled(fn, names):
            ctx.profile(0)
            ctx.profile(1)
            out = fn()
            prof = ctx.profile_read()
            ctx.profile(0)
            return out, {nm: prof[nm]["ms"] for nm in names if nm in prof}

        for log_n in args.log_n:
            n = 1 << log_n
            qap = zkp.QAP(zkp.CSRMatrices.synthetic(n))
            srs = zkp.SRS.generate(ctx, log_n, tau, alpha, beta)
            prep = srs.prepare(ctx)
            lag = prep.export()
            row = {"constraints": n, "prepared_device_bytes": prep.device_bytes}
            keep = {}

            def do_prepare():
                srs.prepare(ctx).free()

            def do_host():
                keep["prepared"] = zkp.CRS.from_prepared(ctx, qap, prep, 1)

            def do_device():
                zkp.CRS.from_prepared_device(ctx, qap, prep, 1).free()

            def do_srs():
                keep["srs"] = zkp.CRS.from_srs(ctx, qap, srs, 1)

            def do_srs_upload():
                zkp.DeviceProvingKey.upload(ctx, zkp.CRS.from_srs(ctx, qap, srs, 1).pk).free()

            def do_verify():
                if lag.verify(ctx, srs) != (True, zkp.ZK_LAG_OK):
                    raise SystemExit("the exported handle fails LagrangeSRS.verify")

            calls = (("prepare", do_prepare), ("from_prepared", do_host), ("from_prepared_device", do_device),
                     ("from_srs", do_srs), ("from_srs_upload", do_srs_upload), ("lagrange_verify", do_verify))
            ts = {name: [] for name, _ in calls}
            for it in range(args.warmup + args.runs):
                for name, fn in (calls if it % 2 == 0 else calls[::-1]):
                    t0 = time.perf_counter()
                    fn()
                    if it >= args.warmup:
                        ts[name].append((time.perf_counter() - t0) * 1e3)
            for nm in PK_ARRAYS:
                if not np.array_equal(getattr(keep["prepared"].pk, nm), getattr(keep["srs"].pk, nm)):
                    raise SystemExit("the key from the prepared string differs from from_srs's in " + nm)
            keep.clear()
            for name, _ in calls:
                row[name] = stats(ts[name])
            for name in ("from_prepared", "from_prepared_device"):
                row["from_srs_over_" + name] = row["from_srs"]["median_ms"] / row[name]["median_ms"]
            row["phases_ms"] = {
                "prepare": profiled(do_prepare, PHASES)[1],
                "from_prepared": profiled(do_host, HOST_KEY)[1],
                "from_prepared_device": profiled(do_device, DEV_KEY)[1],
                "from_srs": profiled(do_srs, PHASES + COLSUMS[:1])[1],
                "lagrange_verify": profiled(do_verify, LAG_PHASES)[1],
            }
            keep.clear()
            print("2^%d prepared" % log_n, json.dumps(row), flush=True)
            res["2p%d" % log_n] = row
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1, sort_keys=True)
                f.write("\n")
            prep.free()
            del srs, lag


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--srs-runs", type=int, nargs="+", default=[0, 64, 256, 1024, 4096])
    ap.add_argument("--prepared", action="store_true", help="measure the prepared strings instead")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.runs < 3:
        ap.error("--runs must be at least 3")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "srs_prepared_bench.json" if args.prepared else "srs_setup_bench.json")

    zkp = importlib.import_module("zero-knowledge-proofs_amd")
    import pyref
    bid = zkp.check_build()
    if args.prepared:
        return prepared(args, zkp, pyref, bid)
    rng = pyref.SplitMix64(0x5255)
    tau, alpha, beta = rng.fr(), rng.fr(), rng.fr()
    params = zkp.SetupParams(alpha, beta, 1, 1, tau)
    res = {"build": bid, "circuit": "synthetic n x (x*y=z), num_public 1, sound host key, gamma = delta = 1"}
    if os.path.exists(args.out):           # sizes measured by earlier calls stay
        with open(args.out) as f:
            old = json.load(f)
        if old.get("build") == bid:
            res = old

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")

    with zkp.Context(0) as ctx:
        def profiled(fn, names):
            ctx.profile(0)
            ctx.profile(1)
            fn()
            prof = ctx.profile_read()
            ctx.profile(0)
            return {nm: prof[nm]["ms"] for nm in names if nm in prof}

        for log_n in args.log_n:
            n = 1 << log_n
            qap = zkp.QAP(zkp.CSRMatrices.synthetic(n))
            t0 = time.perf_counter()
            srs = zkp.SRS.generate(ctx, log_n, tau, alpha, beta)
            row = {"constraints": n, "srs_generate_ms": (time.perf_counter() - t0) * 1e3}

            # ---- the two setups, alternating
            ts = {"from_srs": [], "trusted": []}
            keys = {}
            calls = (("from_srs", lambda: zkp.CRS.from_srs(ctx, qap, srs, 1)),
                     ("trusted", lambda: zkp.CRS.generate_from_qap(ctx, qap, params, 1, sound=True)))
            for it in range(args.warmup + args.runs):
                for name, fn in (calls if it % 2 == 0 else calls[::-1]):
                    t0 = time.perf_counter()
                    keys[name] = fn()
                    if it >= args.warmup:
                        ts[name].append((time.perf_counter() - t0) * 1e3)
            for nm in PK_ARRAYS:
                if not np.array_equal(getattr(keys["from_srs"].pk, nm), getattr(keys["trusted"].pk, nm)):
                    raise SystemExit("the key from the string differs from the trusted one in " + nm)
            keys.clear()
            row["from_srs"], row["trusted_setup_sound"] = stats(ts["from_srs"]), stats(ts["trusted"])
            row["from_srs_over_trusted"] = row["from_srs"]["median_ms"] / row["trusted_setup_sound"]["median_ms"]
            row["phases_ms"] = profiled(lambda: zkp.CRS.from_srs(ctx, qap, srs, 1), PHASES)
            print("2^%d setup" % log_n, json.dumps(row), flush=True)

            # ---- lane mapping of the transform stages
            ab = {}
            for g, fn, pts in (("g1_ntt", ctx.g1_ntt, srs.tau_g1[:n]), ("g2_ntt", ctx.g2_ntt, srs.tau_g2)):
                t = {1: [], 0: []}
                for it in range(args.warmup + args.runs):
                    for m in ((1, 0) if it % 2 == 0 else (0, 1)):
                        ctx.set_option(zkp.ZK_OPT_GNTT_MAP, m)
                        ms = profiled(lambda: fn(pts, inverse=True), (g,))[g]
                        if it >= args.warmup:
                            t[m].append(ms)
                ctx.set_option(zkp.ZK_OPT_GNTT_MAP, -1)
                ab[g] = {"shared_twiddle": stats(t[1]), "twiddle_per_lane": stats(t[0]),
                         "per_lane_over_shared": statistics.median(t[0]) / statistics.median(t[1])}
            row["map"] = ab
            print("2^%d map" % log_n, json.dumps(ab), flush=True)

            # ---- run length of the column sums: variable 0 in every row of C
            syn = qap.csr
            rp = (2 * np.arange(n + 1)).astype(np.uint64)
            col = np.zeros(2 * n, dtype=np.uint32)
            col[1::2] = syn.mats[2][1]
            long_qap = zkp.QAP(zkp.CSRMatrices(n, 3 * n + 1, [syn.mats[0], syn.mats[1], (rp, col, None)]))
            t = {r: [] for r in args.srs_runs}
            for it in range(args.runs):
                for r in args.srs_runs:
                    ctx.set_option(zkp.ZK_OPT_SRS_RUN, r)
                    t[r].append(profiled(lambda: zkp.CRS.from_srs(ctx, long_qap, srs, 1), ("srs_colsum_ic",))
                                ["srs_colsum_ic"])
            ctx.set_option(zkp.ZK_OPT_SRS_RUN, 0)
            row["run"] = {"column_entries": n, "srs_colsum_ic_ms": {str(r): stats(v) for r, v in t.items()}}
            print("2^%d run" % log_n, json.dumps(row["run"]), flush=True)

            # ---- host bar
            if "host_mul_ms" not in res:
                res["host_mul_ms"], res["host_mul_points"] = host_mul_ms(zkp, srs.tau_g1)
            muls = (n // 2) * (log_n - 1) + n
            row["transform_muls_each"] = muls
            row["cpu16_bar_ms"] = (3 * muls + 3 * muls) * res["host_mul_ms"] / 16
            res["2p%d" % log_n] = row
            save()
            del srs


if __name__ == "__main__":
    main()
