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

--bytes: the same sizes from the proofs' 192 wire bytes, three pipelines in
one process, written to profiles/verify_bytes_bench.json:
  (a) Context.verify_many_bytes (zk_groth16_verify_many_bytes): decode,
      subgroup test and verification on the GPU in one call;
  (b) the calls that existed before it: restride the records on the host,
      zk_g1_decompress over A and C, zk_g2_decompress over B, reassemble the
      zk_proof words, verify_many;
  (c) the host decoder (zk_proof_deserialize_compressed, one thread, measured
      here over --host-proofs proofs) spread over --cpus CPUs, plus verify_many.
Kernel times come from one extra run of (a) and of (b) under zk_ctx_profile:
proof_decode_g1 / proof_decode_g2 (the endomorphism subgroup test) against
points_g1 / points_g2 ([r]P == O) on the same points, per point.

  python tools/verify_bench.py --bytes

--all: sound batch verification (Context.verify_all_bytes,
zk_groth16_verify_all_bytes_sound: one pairing check for the batch) against
Context.verify_many_bytes(sound=True) (one verdict per proof) on the same
bytes, alternating in one process, written to profiles/verify_all_bench.json.
Two keys: the tool's own (num_public = 1, marked sound: its proofs satisfy the
sound equation because every scalar is below 2^64) and a num_public = 3 key
with full-width inputs whose proofs hold by construction -- the IC
multiplications are what the batch check removes.  Whole calls (median), and
at n = 262144 as well (the other sizes fit one wave per SIMD, where a call
costs one lane's latency whatever it computes), and
from one extra run of each under zk_ctx_profile the phases verify_all_miller,
verify_all_fold, verify_all_finish against verify; the decode phases are the
same kernels on both sides.

  python tools/verify_bench.py --all

--prepared: prepared verification keys (VerificationKey.prepare,
zk_vk_prepare) in sound mode, written to profiles/verify_prepared_bench.json.
Constructed sound keys with 1, 3, 64 and 256 public inputs (--publics) and
full-width inputs; whole calls of Context.verify_many_bytes(sound=True) with
the plain key -- the behaviour before prepared keys, same kernels -- and of
the same call with the prepared key on the same bytes, alternating in one
process.  Beside them the time of zk_vk_prepare (median of 5, and the first
call) and the key's device bytes, and from one extra run of each under
zk_ctx_profile the phases: verify (plain key: sums and pairings in one lane)
against prepare_inputs and verify (prepared key).  The plain legs above
(verify_many at every size with the 1-input key) run in the same process and
land in the same file.

  python tools/verify_bench.py --prepared
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


def timed_alternating(fns, warmup, runs):
    """timed() for several pipelines measured against each other: one call of each in turn per
    round, so that a drift of the machine falls on all of them alike"""
    ts = {k: [] for k in fns}
    for i in range(warmup + runs):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            if i >= warmup:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "runs": runs}
            for k, t in ts.items()}


def bytes_leg(zkp, ctx, vk, words, inputs, args, res):
    """the three pipelines from wire bytes at every size (module docstring)"""
    recs = np.array([np.frombuffer(zkp.Proof(w).serialize_compressed(), dtype=np.uint8) for w in words])
    k = args.host_proofs
    host_recs = [recs[i % len(recs)].tobytes() for i in range(k)]
    r = timed(lambda: [zkp.Proof.deserialize_compressed(b) for b in host_recs], 1, 5)
    r["proofs"] = k
    r["ms_per_proof"] = r["median_ms"] / k
    r["bar_ms_per_proof"] = r["ms_per_proof"] / args.cpus
    res["host_decode"] = r
    print("host_decode", json.dumps(r), flush=True)
    host_decode_bar = r["bar_ms_per_proof"]

    def existing_calls(data, inp):
        a = data.reshape(-1, 192)
        n = len(a)
        g1 = np.ascontiguousarray(np.stack([a[:, :48], a[:, 144:]], axis=1))       # A and C of a proof side by side
        w1, s1 = ctx.g1_decompress(g1)
        w2, s2 = ctx.g2_decompress(np.ascontiguousarray(a[:, 48:144]))
        assert not s1.any() and not s2.any()
        w1 = w1.reshape(n, 2, 13)
        pw = np.concatenate([w1[:, 0], w2, w1[:, 1]], axis=1)
        return ctx.verify_many(vk, pw, inp), pw

    def profiled(fn):
        ctx.profile(1)
        fn()
        prof = ctx.profile_read()
        ctx.profile(0)
        return {ph: v["ms"] for ph, v in prof.items()}

    for n in args.sizes:
        reps = -(-n // len(words))
        want = np.ascontiguousarray(np.tile(words, (reps, 1))[:n])
        data = np.ascontiguousarray(np.tile(recs, (reps, 1))[:n])
        inp = np.ascontiguousarray(np.tile(inputs, (reps, 1, 1))[:n])
        st, pst = ctx.verify_many_bytes(vk, data, inp, point_status=True)
        assert (st == zkp.ZK_VERIFY_ACCEPT).all() and not pst.any()
        dw, _ = ctx.proofs_deserialize(data)
        assert np.array_equal(dw, want)
        st, pw = existing_calls(data, inp)
        assert (st == zkp.ZK_VERIFY_ACCEPT).all() and np.array_equal(pw, want)
        t = timed_alternating({"a": lambda: ctx.verify_many_bytes(vk, data, inp),
                               "b": lambda: existing_calls(data, inp),
                               "v": lambda: ctx.verify_many(vk, want, inp)}, args.warmup, args.runs)
        a, b, v = t["a"], t["b"], t["v"]
        ka = profiled(lambda: ctx.verify_many_bytes(vk, data, inp))
        kb = profiled(lambda: existing_calls(data, inp))
        c_ms = n * host_decode_bar + v["median_ms"]
        dec_a = ka.get("proof_decode_g1", 0.0) + ka.get("proof_decode_g2", 0.0)
        r = {"proofs": n, "a_verify_many_bytes": a, "b_existing_calls": b, "verify_many_words": v,
             "c_host_decode_bar_plus_verify_ms": c_ms, "a_kernel_ms": ka, "b_kernel_ms": kb,
             "a_ms_per_proof": a["median_ms"] / n, "b_over_a": b["median_ms"] / a["median_ms"],
             "c_over_a": c_ms / a["median_ms"], "a_below_b": a["median_ms"] < b["median_ms"],
             "decode_share_of_a_kernels": dec_a / (dec_a + ka.get("verify", 0.0)),
             "g1_ns_per_point": {"endomorphism": 1e6 * ka.get("proof_decode_g1", 0.0) / (2 * n),
                                 "r_times_p": 1e6 * kb.get("points_g1", 0.0) / (2 * n)},
             "g2_ns_per_point": {"endomorphism": 1e6 * ka.get("proof_decode_g2", 0.0) / n,
                                 "r_times_p": 1e6 * kb.get("points_g2", 0.0) / n}}
        res["bytes_%d" % n] = r
        print("bytes_%d" % n, json.dumps(r), flush=True)


def constructed_key(zkp, pyref, npub, count, key_bits=None):
    """a sound key and `count` proofs that satisfy the Groth16 equation by construction, with
    full-width public inputs -> (vk, (count, 51) words, (count, npub, 4) inputs).  key_bits: the
    width of the key's own scalars (full by default; short ones make a long key quickly here and
    are the same work for the GPU, which sees points)"""
    G1, G2, g1, g2, R = pyref.G1, pyref.G2, pyref.G1.gen, pyref.G2.gen, pyref.R
    rng = pyref.SplitMix64(0xA11B)
    sc = rng.fr if key_bits is None else (lambda: (rng.next() & ((1 << key_bits) - 1)) | 1)
    al, be, ga, de = (sc() for _ in range(4))
    ks = [sc() for _ in range(npub + 1)]
    vk = zkp.VerificationKey.from_points(pyref.g1_words(G1.mul(g1, al)), pyref.g2_words(G2.mul(g2, be)),
                                         pyref.g2_words(G2.mul(g2, ga)), pyref.g2_words(G2.mul(g2, de)),
                                         [pyref.g1_words(G1.mul(g1, k)) for k in ks], sound=True)
    words, inputs = [], []
    for _ in range(count):
        a, b = rng.fr(), rng.fr()
        x = [rng.fr() for _ in range(npub)]
        ic = (ks[0] + sum(xi * k for xi, k in zip(x, ks[1:]))) % R
        c = (a * b - al * be - ic * ga) * pow(de, R - 2, R) % R
        words.append(pyref.g1_words(G1.mul(g1, a)) + pyref.g2_words(G2.mul(g2, b)) + pyref.g1_words(G1.mul(g1, c)))
        inputs.append([zkp.to_limbs(v) for v in x])
    return vk, np.array(words, dtype=np.uint64), np.array(inputs, dtype=np.uint64).reshape(count, npub, 4)


def all_leg(zkp, ctx, pyref, keys, args, res):
    """verify_all_bytes against verify_many_bytes(sound=True) at every size, per key (module docstring)"""
    rng = pyref.SplitMix64(0xC0EF)

    def profiled(fn):
        ctx.profile(1)
        fn()
        prof = ctx.profile_read()
        ctx.profile(0)
        return {ph: v["ms"] for ph, v in prof.items()}

    for name, (vk, words, inputs) in keys.items():
        recs = np.array([np.frombuffer(zkp.Proof(w).serialize_compressed(), dtype=np.uint8) for w in words])
        for n in args.sizes:
            reps = -(-n // len(words))
            data = np.ascontiguousarray(np.tile(recs, (reps, 1))[:n])
            inp = np.ascontiguousarray(np.tile(inputs, (reps, 1, 1))[:n])
            co = np.zeros((n, 4), dtype=np.uint64)
            co[:, 0] = [rng.next() | 1 for _ in range(n)]
            co[:, 1] = [rng.next() for _ in range(n)]
            assert ctx.verify_all_bytes(vk, data, inp, co) == (True, n)
            assert (ctx.verify_many_bytes(vk, data, inp, sound=True) == zkp.ZK_VERIFY_ACCEPT).all()
            wrong = inp.copy()
            wrong[n // 2, 0, 0] ^= np.uint64(1)        # one wrong public input: the batch must reject
            assert ctx.verify_all_bytes(vk, data, wrong, co) == (False, n)
            t = timed_alternating({"all": lambda: ctx.verify_all_bytes(vk, data, inp, co),
                                   "many": lambda: ctx.verify_many_bytes(vk, data, inp, sound=True)},
                                  args.warmup, args.runs)
            ka = profiled(lambda: ctx.verify_all_bytes(vk, data, inp, co))
            km = profiled(lambda: ctx.verify_many_bytes(vk, data, inp, sound=True))
            new = sum(ka.get(ph, 0.0) for ph in ("verify_all_miller", "verify_all_fold", "verify_all_finish"))
            r = {"proofs": n, "num_public": int(vk.num_public), "verify_all_bytes": t["all"],
                 "verify_many_bytes_sound": t["many"], "many_over_all": t["many"]["median_ms"] / t["all"]["median_ms"],
                 "all_ms_per_proof": t["all"]["median_ms"] / n, "many_ms_per_proof": t["many"]["median_ms"] / n,
                 "all_kernel_ms": ka, "many_kernel_ms": km, "all_new_phases_ms": new,
                 "many_verify_phase_ms": km.get("verify", 0.0),
                 "verify_phase_over_new_phases": km.get("verify", 0.0) / new if new else None,
                 "new_phases_below_verify_phase": new < km.get("verify", 0.0)}
            res["%s_%d" % (name, n)] = r
            print("%s_%d" % (name, n), json.dumps(r), flush=True)


def prepared_leg(zkp, ctx, pyref, args, res):
    """verify_many_bytes(sound=True) with the plain key against the same call with the prepared
    key, at every size, for constructed sound keys of 1, 3, 64 and 256 public inputs (module
    docstring)"""
    def profiled(fn):
        ctx.profile(1)
        fn()
        prof = ctx.profile_read()
        ctx.profile(0)
        return {ph: v["ms"] for ph, v in prof.items()}

    for npub in args.publics:
        vk, words, inputs = constructed_key(zkp, pyref, npub, 2, key_bits=40)
        recs = np.array([np.frombuffer(zkp.Proof(w).serialize_compressed(), dtype=np.uint8) for w in words])
        t0 = time.perf_counter()
        pvk = vk.prepare(ctx)
        first_ms = (time.perf_counter() - t0) * 1e3
        pvk.free()
        prep = timed(lambda: vk.prepare(ctx).free(), 0, 5)
        pvk = vk.prepare(ctx)
        key = {"num_public": npub, "zk_vk_prepare": prep, "zk_vk_prepare_first_ms": first_ms,
               "device_bytes": pvk.device_bytes()}
        res["prepared_key_%d" % npub] = key
        print("prepared_key_%d" % npub, json.dumps(key), flush=True)
        for n in args.sizes:
            reps = -(-n // len(words))
            data = np.ascontiguousarray(np.tile(recs, (reps, 1))[:n])
            inp = np.ascontiguousarray(np.tile(inputs, (reps, 1, 1))[:n])
            plain = ctx.verify_many_bytes(vk, data, inp, sound=True)
            assert (plain == zkp.ZK_VERIFY_ACCEPT).all()
            assert ctx.verify_many_bytes(pvk, data, inp).tobytes() == plain.tobytes()
            wrong = inp.copy()
            wrong[n // 2, npub - 1, 3] ^= np.uint64(1)      # one wrong public input, in its top word
            st = ctx.verify_many_bytes(pvk, data, wrong)
            assert st[n // 2] == zkp.ZK_VERIFY_REJECT and (np.delete(st, n // 2) == zkp.ZK_VERIFY_ACCEPT).all()
            t = timed_alternating({"plain": lambda: ctx.verify_many_bytes(vk, data, inp, sound=True),
                                   "prepared": lambda: ctx.verify_many_bytes(pvk, data, inp)}, args.warmup, args.runs)
            kp = profiled(lambda: ctx.verify_many_bytes(vk, data, inp, sound=True))
            kq = profiled(lambda: ctx.verify_many_bytes(pvk, data, inp))
            r = {"proofs": n, "num_public": npub, "plain_key": t["plain"], "prepared_key": t["prepared"],
                 "plain_over_prepared": t["plain"]["median_ms"] / t["prepared"]["median_ms"],
                 "prepared_below_plain": t["prepared"]["median_ms"] < t["plain"]["median_ms"],
                 "plain_kernel_ms": kp, "prepared_kernel_ms": kq,
                 "plain_verify_phase_ms": kp.get("verify", 0.0),
                 "prepared_sum_phase_ms": kq.get("prepare_inputs", 0.0),
                 "prepared_verify_phase_ms": kq.get("verify", 0.0)}
            res["prepared_%d_%d" % (npub, n)] = r
            print("prepared_%d_%d" % (npub, n), json.dumps(r), flush=True)
        pvk.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=None,
                    help="default 1 64 4096 65536; --all adds 262144 (four waves per SIMD: throughput, not latency)")
    ap.add_argument("--host-proofs", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--cpus", type=int, default=16)
    ap.add_argument("--bytes", action="store_true", help="the wire-bytes pipelines (module docstring)")
    ap.add_argument("--all", action="store_true", help="sound batch verification against verify_many_bytes_sound")
    ap.add_argument("--prepared", action="store_true",
                    help="verify_many_bytes_sound with the plain key against the prepared key, beside the plain legs")
    ap.add_argument("--publics", type=int, nargs="+", default=[1, 3, 64, 256],
                    help="--prepared: the keys' public inputs")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "verify_all_bench.json" if args.all else
                                "verify_bytes_bench.json" if args.bytes else
                                "verify_prepared_bench.json" if args.prepared else "verify_bench.json")
    if args.runs < 5:
        ap.error("--runs must be at least 5")
    if args.sizes is None:
        args.sizes = [1, 64, 4096, 65536] + ([262144] if args.all else [])

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
        if args.all:
            svk = zkp.VerificationKey.from_points(vk.point("alpha_g1"), vk.point("beta_g2"), vk.point("gamma_g2"),
                                                  vk.point("delta_g2"), vk.ic_g1, sound=True)
            all_leg(zkp, ctx, pyref, {"public1": (svk, words, inputs),
                                      "public3": constructed_key(zkp, pyref, 3, len(words))}, args, res)
        elif args.bytes:
            bytes_leg(zkp, ctx, vk, words, inputs, args, res)
        elif args.prepared:
            prepared_leg(zkp, ctx, pyref, args, res)
        for n in [] if args.bytes or args.all else args.sizes:
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
