"""Merge the runs behind profiles/sound_copies_bench.json into that file.

tools/sound_bench.py writes one flat result per run; the record of the
grouped-window plan is several runs of one session on one GPU:

  sweep_2p20   one run: --setup-log-n --win-c 16 20 --copies 1 2 4 0
  default_plan_vs_parent_2p20
               the default plan (--setup-log-n --no-reference --win-c 20
               --copies 0 --runs 30) as processes alternating between this
               tree's library and the parent commit's (built into another
               directory, loaded through ZK_AMD_LIB): --default-new and
               --default-parent, the files of each library in round order;
               beside each, bench.py --gpus 1 --steps 100 --warmup 10 in the
               same alternation (--bench-new / --bench-parent: its JSON lines)
  prove_2p24   one run: --setup-log-n --no-reference --log-n 24 --win-c C
               --copies S --setup-runs 1 at the fastest plan of the sweep
               that fits

  python tools/sound_copies_merge.py --sweep sweep.json --default-new n1.json n2.json \\
      --default-parent p1.json p2.json --bench-new bn1.json bn2.json --bench-parent bp1.json bp2.json \\
      --p24 p24.json [--out profiles/sound_copies_bench.json]
"""
import argparse
import json
import os
import statistics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load(path):
    with open(path) as f:
        return json.load(f)


def default_line(path, library, rnd):
    d = load(path)
    p = d["prove_sound_c20"]
    return {"library": library, "round": rnd, "build": d["build"], "median_ms": p["median_ms"], "min_ms": p["min_ms"],
            "max_ms": p["max_ms"], "runs": p["runs"], "serial_per_msm_ms": p["serial"]["per_msm_ms"],
            "setup_median_ms": p["setup"]["median_ms"]}


def bench_line(path, library, rnd):
    with open(path) as f:
        d = json.loads(f.read().strip().splitlines()[-1])
    return {"library": library, "round": rnd, "ms_per_step": d["ms_per_step"], "build_id": d["build_id"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", required=True)
    ap.add_argument("--default-new", nargs="+", required=True)
    ap.add_argument("--default-parent", nargs="+", required=True)
    ap.add_argument("--bench-new", nargs="*", default=[])
    ap.add_argument("--bench-parent", nargs="*", default=[])
    ap.add_argument("--p24")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sound_copies_bench.json"))
    args = ap.parse_args()

    out = {"method": "tools/sound_bench.py on one MI355X (synthetic circuit, device witness, random full-width "
                     "parameters; prove = median of whole zk_groth16_prove_dev calls, host wall time, after warm-ups; "
                     "serial = device ms per proof, phase and MSM under schedule 3; setup = median of timed "
                     "zk_groth16_setup_sound_dev calls after one untimed, a single call at 2^24; device_bytes = "
                     "zk_pk_device_bytes; every sound proof checked by Verifier.verify).  The sections are separate "
                     "runs of one session merged by tools/sound_copies_merge.py, whose docstring gives each command",
           "sweep_2p20": load(args.sweep)}
    cmp_ = {"what": "the default plan (ZK_OPT_SOUND_COPIES = 0, c = 20, 13 copies) at 2^20: this tree's library "
                    "against the parent commit's, processes alternating new / parent per round", "runs": []}
    for lib, files in (("new", args.default_new), ("parent", args.default_parent)):
        cmp_["runs"] += [default_line(p, lib, k + 1) for k, p in enumerate(files)]
        cmp_[lib + "_mean_of_medians_ms"] = statistics.mean(e["median_ms"] for e in cmp_["runs"] if e["library"] == lib)
    cmp_["runs"].sort(key=lambda e: (e["round"], e["library"]))
    cmp_["new_over_parent"] = cmp_["new_mean_of_medians_ms"] / cmp_["parent_mean_of_medians_ms"]
    flag = [bench_line(p, lib, k + 1) for lib, files in (("new", args.bench_new), ("parent", args.bench_parent))
            for k, p in enumerate(files)]
    if flag:
        cmp_["flagship_reference_prove"] = {
            "what": "bench.py --gpus 1 --steps 100 --warmup 10 (reference-mode 2^20 prove, ms per proof), same alternation",
            "runs": sorted(flag, key=lambda e: (e["round"], e["library"]))}
    out["default_plan_vs_parent_2p20"] = cmp_
    if args.p24:
        out["prove_2p24"] = load(args.p24)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: v for k, v in cmp_.items() if k != "runs"}))


if __name__ == "__main__":
    main()
