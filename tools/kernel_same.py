"""Compare the MSM kernels of two device assembly files, kernel by kernel.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S msm.hip -o X.s   (both trees)
    python3 tools/kernel_same.py OLD.s NEW.s [scalar_width | unchanged]

(scalar_width: the prove / setup / dist kernels of SCALAR_WIDTH_MAP below
instead of the MSM ones; unchanged: every kernel that both files hold under
the same name, for a change that must leave existing kernels as they are,
such as points.hip's decompression template gaining a layout parameter.)  A kernel's body is the text between its label and its .Lfunc_end.  Before
comparing, comments, directives and blank lines are dropped, block labels
(.LBB<function>_<block>) and .Lpost_getpc<n> lose the numbering that depends
on the function's place in the file, and symbols that carry a kernel's name
(the kernel, its LDS variables) become KSYM.  Per kernel: identical / differ,
instructions and v_mad_u64_u32 (the field multiplier's instruction) on both
sides.  Exit status 1 if any kernel differs or is missing.
"""
import re
import sys

# old mangled prefix -> new mangled prefix (lane-layout refactor: the G2
# lane-pair twins became the <G2> instances of the one template per phase)
NAME_MAP = [
    ("_ZN2zk11k_msm_accumINS_2G1E", "_ZN2zk11k_msm_accumINS_2G1E"),
    ("_ZN2zk16k_msm_accum_pairE", "_ZN2zk11k_msm_accumINS_2G2E"),
    ("_ZN2zk11k_msm_fixupINS_2G1E", "_ZN2zk11k_msm_fixupINS_2G1E"),
    ("_ZN2zk16k_msm_fixup_pairE", "_ZN2zk11k_msm_fixupINS_2G2E"),
    ("_ZN2zk13k_msm_combineINS_2G1E", "_ZN2zk13k_msm_combineINS_2G1E"),
    ("_ZN2zk18k_msm_combine_pairE", "_ZN2zk13k_msm_combineINS_2G2E"),
    ("_ZN2zk12k_msm_rowcolINS_2G1E", "_ZN2zk12k_msm_rowcolINS_2G1E"),
    ("_ZN2zk17k_msm_rowcol_pairE", "_ZN2zk12k_msm_rowcolINS_2G2E"),
    ("_ZN2zk13k_msm_quant_qINS_2G1E", "_ZN2zk11k_msm_quantINS_2G1E"),
    ("_ZN2zk15k_msm_quant_duoI", "_ZN2zk11k_msm_quantINS_2G2E"),
    ("_ZN2zk11k_msm_mergeINS_2G1E", "_ZN2zk11k_msm_mergeINS_2G1E"),
    ("_ZN2zk11k_msm_mergeINS_2G2E", "_ZN2zk11k_msm_mergeINS_2G2E"),
]

# `python3 tools/kernel_same.py OLD.s NEW.s scalar_width`, each side the
# concatenated assembly of prove.hip, setup.hip, dist.hip and ntt.hip: the
# lo64 / whole-scalar twins became the <1> / <4> instances of one template over
# the scalar width.  Every kernel whose name did not change is compared too.
SCALAR_WIDTH_MAP = [
    ("_ZN2zk9k_h_finalE", "_ZN2zk9k_h_finalILi1EE"),
    ("_ZN2zk14k_h_final_fullE", "_ZN2zk9k_h_finalILi4EE"),
    ("_ZN2zk8k_h_lo64E", "_ZN2zk12k_fr_scalarsILi1EE"),
    ("_ZN2zk6k_lo64E", "_ZN2zk12k_fr_scalarsILi1EE"),
    ("_ZN2zk9k_h_canonE", "_ZN2zk12k_fr_scalarsILi4EE"),
    ("_ZN2zk11k_from_montE", "_ZN2zk12k_fr_scalarsILi4EE"),
    ("_ZN2zk13k_gather_lo64E", "_ZN2zk8k_gatherILi1EE"),
    ("_ZN2zk11k_gather_frE", "_ZN2zk8k_gatherILi4EE"),
    ("_ZN2zk15k_setup_scalarsE", "_ZN2zk15k_setup_scalarsILi1EE"),
    ("_ZN2zk20k_setup_scalars_fullE", "_ZN2zk15k_setup_scalarsILi4EE"),
    ("_ZN2zk12k_set_extrasE", "_ZN2zk12k_set_extrasE"),
    ("_ZN2zk15k_set_extras_frE", "_ZN2zk12k_set_extrasE"),
]


def kernels(path):
    """{mangled name: normalised instruction lines} of every function in the file."""
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        line = line.split(";")[0].strip()
        if not line or (line.startswith(".") and not line.endswith(":")):
            continue   # comment, blank, directive
        line = re.sub(r"\.LBB\d+_", ".LBB_", line)
        line = re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", line)
        line = re.sub(r"_ZN2zk\d+k_\w*", "KSYM", line)
        body.append(line)
    return out


def find(ks, prefix):
    hits = [k for k in ks if k.startswith(prefix)]
    return hits[0] if len(hits) == 1 else None


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    pairs = NAME_MAP
    if len(sys.argv) > 3 and sys.argv[3] == "scalar_width":
        mapped = {p for p, _ in SCALAR_WIDTH_MAP}
        pairs = SCALAR_WIDTH_MAP + [(k, k) for k in old if k in new and re.match(r"_ZN2zk\d+k_", k)
                                    and not any(k.startswith(p) for p in mapped)]
    if len(sys.argv) > 3 and sys.argv[3] == "unchanged":
        pairs = [(k, k) for k in old if k in new and re.match(r"_ZN2zk\d+k_", k)]
    bad = 0
    for po, pn in pairs:
        ko, kn = find(old, po), find(new, pn)
        if ko is None or kn is None:
            print(f"missing    {po} -> {pn}")
            bad += 1
            continue
        a, b = old[ko], new[kn]
        ia = [x for x in a if not x.endswith(":")]
        ib = [x for x in b if not x.endswith(":")]
        same = a == b
        bad += not same
        mad = lambda xs: sum(x.startswith("v_mad_u64_u32") for x in xs)
        print(f"{'identical' if same else 'differ   '}  {ko[:48]:48s} -> {kn[:48]:48s} "
              f"insts {len(ia)} / {len(ib)}  v_mad_u64_u32 {mad(ia)} / {mad(ib)}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
