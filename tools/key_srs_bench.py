"""A sound key audited against its powers-of-tau string
(zk_groth16_verify_key_srs_sound, CRS.verify_against_srs) on one GPU, beside
what an auditor had to do without it for an INITIAL key: rebuild the key from
the string (zk_groth16_setup_srs_sound) and compare bytes.

One process, one ctx, the synthetic circuit n x (x*y = z) at each --log-n
(num_public 1), a string of exactly that size from known secrets, the key
after one contribution (the rebuild route cannot audit that key at all: it
rebuilds the initial key and is timed on it):

  verify    the whole CRS.verify_against_srs call on the contributed key, with
            coefficients drawn beforehand (a (n, 4) limb array: the drawing is
            host Python, not the call); it must accept
  rebuild   the whole CRS.from_srs call, then np.array_equal over the five
            arrays and the single points against the initial key
            the two routes alternate: median of --runs wall times each after
            --warmup
  phases    one profiled verify call (zk_ctx_profile): host wall time of the
            point validation, of the MSMs over the key and over the string and
            of the pairings; device time of the split row products, the six
            inverse transforms, the scalar preparation and the string's upload
  bytes     the key's host arrays and the part of the string the call reads

  python tools/key_srs_bench.py [--log-n 16 20] [--out profiles/key_srs_bench.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from contribute_bench import stats  # noqa: E402

PHASES = ("keysrs_validate", "keysrs_split", "keysrs_transforms", "keysrs_scalars", "keysrs_upload", "keysrs_msm_key",
          "keysrs_msm_srs", "keysrs_pairing")
PK_ARRAYS = ("a_g1", "b_g1", "b_g2", "ic_g1", "h_g1")
PK_POINTS = ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2")


def same_key(a, b):
    return (all(np.array_equal(getattr(a.pk, nm), getattr(b.pk, nm)) for nm in PK_ARRAYS) and
            all(np.array_equal(a.pk.point(nm), b.pk.point(nm)) for nm in PK_POINTS) and
            np.array_equal(a.vk.ic_g1, b.vk.ic_g1) and
            all(np.array_equal(a.vk.point(nm), b.vk.point(nm)) for nm in ("alpha_g1", "beta_g2", "gamma_g2", "delta_g2")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_srs_bench.json"))
    args = ap.parse_args()
    if args.runs < 3:
        ap.error("--runs must be at least 3")

    zkp = importlib.import_module("zero-knowledge-proofs_amd")
    import pyref
    bid = zkp.check_build()
    rng = pyref.SplitMix64(0x6B53)
    tau, alpha, beta, share = rng.fr(), rng.fr(), rng.fr(), rng.fr()
    res = {"build": bid, "circuit": "synthetic n x (x*y=z), num_public 1, sound host key after one contribution"}
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
        for log_n in args.log_n:
            n = 1 << log_n
            qap = zkp.QAP(zkp.CSRMatrices.synthetic(n))
            srs = zkp.SRS.generate(ctx, log_n, tau, alpha, beta)
            initial = zkp.CRS.from_srs(ctx, qap, srs, 1)
            key = initial.contribute(ctx, share)
            co = np.zeros((qap.num_variables + n, 4), dtype=np.uint64)
            g = np.random.default_rng(log_n)
            co[:, :2] = g.integers(1, 1 << 63, size=(len(co), 2), dtype=np.uint64)
            row = {"constraints": n, "variables": qap.num_variables,
                   "key_host_bytes": int(sum(getattr(key.pk, nm).nbytes for nm in PK_ARRAYS) + key.vk.ic_g1.nbytes),
                   "string_bytes_read": int(srs.tau_g1[:2 * n].nbytes + srs.tau_g2[:n].nbytes +
                                            srs.alpha_tau_g1[:n].nbytes + srs.beta_tau_g1[:n].nbytes)}

            def verify():
                if key.verify_against_srs(ctx, srs, co) != (True, zkp.ZK_KEYSRS_OK):
                    raise SystemExit("verify_against_srs rejected an honest key")

            def rebuild():
                if not same_key(zkp.CRS.from_srs(ctx, qap, srs, 1), initial):
                    raise SystemExit("the rebuilt key differs from the initial one")

            ts = {"verify": [], "rebuild": []}
            calls = (("verify", verify), ("rebuild", rebuild))
            for it in range(args.warmup + args.runs):
                for name, fn in (calls if it % 2 == 0 else calls[::-1]):
                    t0 = time.perf_counter()
                    fn()
                    if it >= args.warmup:
                        ts[name].append((time.perf_counter() - t0) * 1e3)
            row["verify_against_srs"], row["rebuild_and_compare"] = stats(ts["verify"]), stats(ts["rebuild"])
            row["rebuild_over_verify"] = row["rebuild_and_compare"]["median_ms"] / row["verify_against_srs"]["median_ms"]

            ctx.profile(0)
            ctx.profile(1)
            verify()
            prof = ctx.profile_read()
            ctx.profile(0)
            row["phases_ms"] = {nm: prof[nm]["ms"] for nm in PHASES if nm in prof}
            print("2^%d" % log_n, json.dumps(row), flush=True)
            res["2p%d" % log_n] = row
            save()
            del srs, initial, key


if __name__ == "__main__":
    main()
