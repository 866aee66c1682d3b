"""Batch verification on one GPU against the host verifier.

Times Context.verify_many (zk_groth16_verify_many: one lane per proof) as
whole calls -- host arrays in, statuses out, the per-call key tables and all
copies included -- at n = 1, 64, 4096 and 65536 proofs (65536: one full wave
on every SIMD), and the host zk_groth16_verify on one thread over 16 proofs.
The proofs are a few valid proofs of the reference's test circuit x*y=z from
the oracle's prover, tiled; every status must be ACCEPT.

Each figure is the median of --runs timed calls after --warmup untimed ones;
kernel_ms is the `verify` phase of one extra run under zk_ctx_profile.
"bar" is the host verifier's time per proof divided by --cpus (the CPUs a box
leases): what the host verifier of this repository, spread perfectly over the
box, would need per proof.  It is the naive host verifier (affine Miller loop,
plain square-and-multiply final exponentiation), not an optimized CPU
library.

  python tools/verify_bench.py [--out profiles/verify_bench.json]
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

TOY_XY = [(3, 4), (0, 5), (1, 1), (2, 7), (5, 5), (6, 2), (9, 3), (4, 11)]


def timed(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 64, 4096, 65536])
    ap.add_argument("--host-proofs", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--cpus", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_bench.json"))
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs must be at least 5")

    zkp = importlib.import_module("zero-knowledge-proofs_amd")
    import binding as oracle
    import pyref
    bid = zkp.check_build()

    # the reference's test circuit with setup parameters whose derived scalars stay below 2^64
    csr = oracle.CSR.from_constraints([({1: 1}, {2: 1}, {3: 1})], 4)
    rc, pk, ovk = oracle.setup(csr, [2, 3, 1, 1, 5], 1)
    assert rc == 0
    vk = zkp.VerificationKey.from_points(ovk.field("alpha_g1"), ovk.field("beta_g2"), ovk.field("gamma_g2"),
                                         ovk.field("delta_g2"), ovk.ic_g1)
    rng = pyref.SplitMix64(0x7E21F)
    words, xs = [], []
    for x, y in TOY_XY:
        rc, pr = oracle.prove(pk, csr, oracle.fr_array([1, x, y, x * y]), 1, rng.fr(), rng.fr())
        assert rc == 0
        words.append(np.array(pr, dtype=np.uint64))
        xs.append(x)
    words = np.array(words)
    inputs = zkp.fr_array(xs).reshape(-1, 1, 4)

    res = {"build": bid, "cpus": args.cpus, "distinct_proofs": len(words), "num_public": 1}

    # the host verifier, one thread
    k = args.host_proofs
    host_proofs = [zkp.Proof(words[i % len(words)]) for i in range(k)]

    def host_run():
        for i, p in enumerate(host_proofs):
            assert zkp.Verifier.verify(vk, p, [xs[i % len(xs)]])
    r = timed(host_run, 1, 5)
    r["proofs"] = k
    r["ms_per_proof"] = r["median_ms"] / k
    r["bar_ms_per_proof"] = r["ms_per_proof"] / args.cpus
    res["host_verify"] = r
    bar = r["bar_ms_per_proof"]
    print("host_verify", json.dumps(r), flush=True)

    with zkp.Context(0) as ctx:
        for n in args.sizes:
            reps = -(-n // len(words))
            w = np.ascontiguousarray(np.tile(words, (reps, 1))[:n])
            inp = np.ascontiguousarray(np.tile(inputs, (reps, 1, 1))[:n])
            st = ctx.verify_many(vk, w, inp)
            assert len(st) == n and (st == zkp.ZK_VERIFY_ACCEPT).all()
            r = timed(lambda: ctx.verify_many(vk, w, inp), args.warmup, args.runs)
            ctx.profile(1)
            st = ctx.verify_many(vk, w, inp)
            r["kernel_ms"] = ctx.profile_read().get("verify", {}).get("ms", 0.0)
            ctx.profile(0)
            assert (st == zkp.ZK_VERIFY_ACCEPT).all()
            r["proofs"] = n
            r["ms_per_proof"] = r["median_ms"] / n
            r["bar_ms_per_proof"] = bar
            r["bar_over_gpu"] = bar / r["ms_per_proof"]
            r["below_bar"] = r["ms_per_proof"] < bar
            res["verify_many_%d" % n] = r
            print("verify_many_%d" % n, json.dumps(r), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
