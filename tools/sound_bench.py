"""Sound-mode setup and prove on one GPU, next to the reference mode.

One process, one ctx, synthetic circuit n x (x*y = z), random full-width
setup parameters, a device witness:

  setup   CRS.generate_device (straight into HBM, window copies included) at
          each --setup-log-n, reference mode and sound mode in turn: median of
          --setup-runs timed calls after one untimed one
  prove   at --log-n: the reference-mode key (unless --no-reference), then a
          sound key per ZK_OPT_SOUND_WIN_C in --win-c and per
          ZK_OPT_SOUND_COPIES in --copies (0: every window copy, the shared
          plan; k: the grouped-window plan over k copies).  Each: the GPU
          setup timed like the setups above, the key's device_bytes(),
          --warmup untimed proofs, then the median of --runs timed
          Prover.prove_device calls (overlapped schedule, host wall time of
          the whole call, proof on the host), then --serial-runs proofs under
          schedule 3 with zk_ctx_profile: device ms per phase and per MSM (A,
          B1, B2, ICH; reference: AB, B2, ICH), per proof.  Every sound proof
          is checked by Verifier.verify once; a rejected proof fails the run.

  python tools/sound_bench.py [--out profiles/sound_prove_bench.json]
  python tools/sound_bench.py --setup-log-n --win-c 16 20 --copies 1 2 4 0 --out sweep.json
  python tools/sound_bench.py --setup-log-n --no-reference --log-n 24 --win-c 16 --copies 4 \\
      --setup-runs 1 --out one_plan_2p24.json      # one timed setup, no untimed one before it

A library given by ZK_AMD_LIB (an A/B build of another revision) may lack the
copies option: it then runs --copies 0 only.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def median_ms(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "runs": runs}


def serial_profile(zkp, ctx, prove, runs):
    """Device ms per proof under the serial schedule: per phase, and summed
    per MSM tag ("A", "B2", ...; "quotient" for the untagged phases)."""
    ctx.set_schedule(3)
    prove()
    ctx.profile(1)
    for _ in range(runs):
        prove()
    prof = ctx.profile_read()
    ctx.profile(0)
    ctx.set_schedule(-1)
    phases = {k: v["ms"] / runs for k, v in prof.items()}
    groups = {}
    for k, ms in phases.items():
        if k.startswith("host_") or k == "prove_gpu_span":
            continue
        tag = k.split("/")[0] if "/" in k else "quotient"
        groups[tag] = groups.get(tag, 0.0) + ms
    return {"per_msm_ms": groups, "device_sum_ms": sum(groups.values()), "phases_ms": phases,
            "gpu_span_ms": phases.get("prove_gpu_span")}


def write(res, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


def plan_name(c, copies):
    return "c%d" % c if not copies else "c%d_s%d" % (c, copies)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--setup-log-n", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--win-c", type=int, nargs="+", default=[16, 20, 22])
    ap.add_argument("--copies", type=int, nargs="+", default=[0],
                    help="ZK_OPT_SOUND_COPIES per sound key: 0 every window copy, k the first k")
    ap.add_argument("--no-reference", action="store_true", help="skip the reference-mode key")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--serial-runs", type=int, default=3)
    ap.add_argument("--setup-runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sound_prove_bench.json"))
    args = ap.parse_args()
    if args.runs < 10:
        ap.error("--runs must be at least 10")

    zkp = importlib.import_module("zero-knowledge-proofs_amd")
    import pyref
    other = bool(os.environ.get("ZK_AMD_LIB"))
    bid = zkp.build_id() if other else zkp.check_build()
    has_copies = hasattr(zkp.lib(), "zk_pk_device_bytes")
    if not has_copies and any(args.copies):
        ap.error("this library has no ZK_OPT_SOUND_COPIES: --copies 0 only")
    rng = pyref.SplitMix64(0x50B3)
    params = zkp.SetupParams(*[rng.fr() for _ in range(5)])
    r, s = rng.fr(), rng.fr()
    res = {"build": bid, "log_n": args.log_n, "circuit": "synthetic n x (x*y=z), num_public 1, device witness"}

    with zkp.Context(0) as ctx:
        # ---- setup, both modes in turn
        for log_n in args.setup_log_n:
            qap = zkp.QAP(zkp.CSRMatrices.synthetic(1 << log_n))
            for sound in (False, True):
                def run():
                    zkp.CRS.generate_device(ctx, qap, params, 1, sound=sound).free()
                t = median_ms(run, 1, args.setup_runs)
                res["setup_2p%d_%s" % (log_n, "sound" if sound else "reference")] = t
                print("setup 2^%d %s" % (log_n, "sound" if sound else "reference"), json.dumps(t), flush=True)

        # ---- prove
        def workload(log_n):
            n = 1 << log_n
            return zkp.QAP(zkp.CSRMatrices.synthetic(n)), ctx.synthetic_witness(n, 0x50B4), 3 * n + 1

        def bench_key(dpk, z, zlen):
            def prove():
                return zkp.Prover.prove_device(dpk, z.data_ptr(), zlen, 1, r, s)
            out = median_ms(prove, args.warmup, args.runs)
            out["serial"] = serial_profile(zkp, ctx, prove, args.serial_runs)
            if not other:
                out["win"], out["win_c"] = dpk.test_info()[:2]
            return out, prove()

        def bench_sound(qap, z, zlen, c, copies, setup_runs):
            """One sound key: timed GPU setups, its size, prove times, one verified proof."""
            ctx.set_option(zkp.ZK_OPT_SOUND_WIN_C, c)
            if has_copies:
                ctx.set_option(zkp.ZK_OPT_SOUND_COPIES, copies)
            vk = zkp.VerificationKey(1, sound=True)
            made = []

            def setup():
                if made:
                    made.pop().free()
                made.append(zkp.CRS.generate_device(ctx, qap, params, 1, sound=True, vk=vk))
            t_setup = median_ms(setup, 1 if setup_runs > 1 else 0, setup_runs)
            dpk = made.pop()
            out, proof = bench_key(dpk, z, zlen)
            out["setup"] = t_setup
            if has_copies:
                out["copies"], out["sets"] = dpk.test_plan()
                out["device_bytes"] = dpk.device_bytes()
            dpk.free()
            x = [zkp.from_limbs(z[1].cpu().numpy().view("uint64"))]
            if not zkp.Verifier.verify(vk, proof, x):
                raise SystemExit("sound proof rejected (c = %d, copies = %d)" % (c, copies))
            out["verified"] = True
            return out

        def show(name, out):
            print(name, json.dumps({k: v for k, v in out.items() if k != "serial"}),
                  json.dumps(out["serial"]["per_msm_ms"]), flush=True)

        qap, z, zlen = workload(args.log_n)
        ref = None
        if not args.no_reference:
            dpk = zkp.CRS.generate_device(ctx, qap, params, 1)
            ref, _ = bench_key(dpk, z, zlen)
            dpk.free()
            res["prove_reference"] = ref
            show("prove reference", ref)

        plans = [(c, k) for c in args.win_c for k in args.copies]
        for c, k in plans:
            out = bench_sound(qap, z, zlen, c, k, args.setup_runs)
            if ref:
                out["over_reference"] = out["median_ms"] / ref["median_ms"]
            res["prove_sound_" + plan_name(c, k)] = out
            show("prove sound c=%d copies=%d" % (c, k), out)
        best = min(plans, key=lambda p: res["prove_sound_" + plan_name(*p)]["median_ms"])
        res["fastest_win_c"] = best[0]
        res["fastest_copies"] = best[1]
        ctx.set_option(zkp.ZK_OPT_SOUND_WIN_C, 0)
        if has_copies:
            ctx.set_option(zkp.ZK_OPT_SOUND_COPIES, 0)

    write(res, args.out)
    print(json.dumps({k: v for k, v in res.items() if not k.startswith("prove_")}))


if __name__ == "__main__":
    main()
