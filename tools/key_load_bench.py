"""Load-time cost of compressed proving keys on one GPU.

Times, as whole calls (host buffers in, host buffers out, copies included):
  - zk_g1_decompress of 2^20 and zk_g2_decompress of 2^18 encodings of
    distinct subgroup points, and zk_g1_validate / zk_g2_validate of the same
    points in affine form;
  - load_proving_key of a compressed 2^16-constraint synthetic key file;
  - the host decoder on 256 of the same encodings, one thread, through
    zk_proof_deserialize_compressed (the encoding as `a` or `b`, the identity
    in the other slots, which the decoder answers without arithmetic).
The points come from the GPU setup of the synthetic circuit at 2^18
constraints (fixed-base path): ic_g1, h_g1 and the non-identity a_g1 entry
give 2^20 distinct G1 points, the non-identity b_g2 entries 2^18 G2 points.

Each figure is the median of --runs timed calls after --warmup untimed ones;
the kernel share comes from one extra run under zk_ctx_profile (HIP events
around the launches).  "bar" is the host decoder's time per point divided by
--cpus (the CPUs a box leases): what a perfectly parallel CPU loader would
need, and what the GPU path has to beat.

  python tools/key_load_bench.py [--out profiles/key_load_bench.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def timed(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "runs": runs}


def kernel_ms(ctx, fn, phase):
    ctx.profile(1)
    fn()
    ms = ctx.profile_read().get(phase, {}).get("ms", 0.0)
    ctx.profile(0)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-setup", type=int, default=18, help="constraints of the setup that makes the points")
    ap.add_argument("--log-key", type=int, default=16, help="constraints of the key file that is loaded")
    ap.add_argument("--host-points", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--cpus", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_load_bench.json"))
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs must be at least 5")

    zkp = importlib.import_module("zero-knowledge-proofs_amd")
    import pyref
    bid = zkp.check_build()
    rng = pyref.SplitMix64(0x10AD)
    res = {"build": bid, "log_setup": args.log_setup, "log_key": args.log_key, "cpus": args.cpus}

    with zkp.Context(0) as ctx:
        def setup(log_n):
            qap = zkp.QAP(zkp.CSRMatrices.synthetic(1 << log_n))
            return zkp.CRS.generate_from_qap(ctx, qap, zkp.SetupParams.random(rng.fr), 1).pk

        pk = setup(args.log_setup)
        g1 = np.concatenate([pk.ic_g1, pk.h_g1, pk.a_g1[pk.a_g1[:, 12] == 0][:1]])
        g2 = pk.b_g2[pk.b_g2[:, 24] == 0]
        g1 = np.ascontiguousarray(g1[g1[:, 12] == 0])
        g2 = np.ascontiguousarray(g2)
        assert len(np.unique(g1[:, :6], axis=0)) == len(g1) and len(np.unique(g2[:, :12], axis=0)) == len(g2)
        e1, e2 = zkp.compress_g1(g1), zkp.compress_g2(g2)
        res["g1_points"], res["g2_points"] = len(g1), len(g2)

        # results first: the timed calls must give back the points they were made from
        w1, s1 = ctx.g1_decompress(e1)
        w2, s2 = ctx.g2_decompress(e2)
        assert not s1.any() and not s2.any() and np.array_equal(w1, g1) and np.array_equal(w2, g2)
        assert not ctx.g1_validate(g1).any() and not ctx.g2_validate(g2).any()

        for name, fn, n, phase in (("g1_decompress", lambda: ctx.g1_decompress(e1), len(g1), "points_g1"),
                                   ("g2_decompress", lambda: ctx.g2_decompress(e2), len(g2), "points_g2"),
                                   ("g1_validate", lambda: ctx.g1_validate(g1), len(g1), "points_g1"),
                                   ("g2_validate", lambda: ctx.g2_validate(g2), len(g2), "points_g2")):
            r = timed(fn, args.warmup, args.runs)
            r["points"] = n
            r["ms_per_point"] = r["median_ms"] / n
            r["kernel_ms"] = kernel_ms(ctx, fn, phase)
            res[name] = r
            print(name, json.dumps(r), flush=True)

        # a compressed key file, end to end (read, decompress = validate, CSR section)
        kpk = pk if args.log_key == args.log_setup else setup(args.log_key)
        with tempfile.TemporaryDirectory() as d:
            p1, p2 = os.path.join(d, "pk1.bin"), os.path.join(d, "pk2.bin")
            zkp.save_proving_key(kpk, p1)
            zkp.save_proving_key(kpk, p2, compressed=True)
            back = zkp.load_proving_key(p2, ctx=ctx)
            assert all(np.array_equal(getattr(back, nm), getattr(kpk, nm))
                       for nm in ("a_g1", "b_g1", "b_g2", "ic_g1", "h_g1"))
            r = timed(lambda: zkp.load_proving_key(p2, ctx=ctx), args.warmup, args.runs)
            r["file_bytes"], r["uncompressed_file_bytes"] = os.path.getsize(p2), os.path.getsize(p1)
            r["g1_points"] = len(kpk.a_g1) + len(kpk.b_g1) + len(kpk.ic_g1) + len(kpk.h_g1) + 3
            r["g2_points"] = len(kpk.b_g2) + 2
            res["load_compressed_key"] = r
            print("load_compressed_key", json.dumps(r), flush=True)
            r = timed(lambda: zkp.load_proving_key(p1), args.warmup, args.runs)
            res["load_uncompressed_key_unchecked"] = r
            r = timed(lambda: zkp.load_proving_key(p1, ctx=ctx, validate=True), args.warmup, args.runs)
            res["load_uncompressed_key_validated"] = r

    # the host decoder, one thread, on the same encodings
    import ctypes as C
    inf1, inf2 = bytes([0xC0]) + bytes(47), bytes([0xC0]) + bytes(95)
    out = zkp._Proof()
    k = args.host_points
    for name, enc, size, wrap in (("g1", e1, 48, lambda e: e + inf2 + inf1), ("g2", e2, 96, lambda e: inf1 + e + inf1)):
        bufs = [(C.c_uint8 * 192).from_buffer_copy(wrap(enc[size * i:size * (i + 1)])) for i in range(k)]

        def run():
            for b in bufs:
                assert zkp.lib().zk_proof_deserialize_compressed(b, C.byref(out)) == 0
        r = timed(run, 1, 5)
        r["points"] = k
        r["ms_per_point"] = r["median_ms"] / k
        r["bar_ms_per_point"] = r["ms_per_point"] / args.cpus
        gpu = res[name + "_decompress"]["ms_per_point"]
        r["gpu_ms_per_point"] = gpu
        r["gpu_speedup_over_bar"] = r["bar_ms_per_point"] / gpu
        res["host_decoder_" + name] = r
        print("host_decoder_" + name, json.dumps(r), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
