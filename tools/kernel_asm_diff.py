"""Compare the gfx950 device code of two checkouts kernel by kernel (a refactor's "identical code" check; no GPU needed).

    python tools/kernel_asm_diff.py OLD_TREE NEW_TREE [--files misc.hip,norm.hip,gemm_mfma.hip] [--rename OLD_RE=NEW ...]
                                    [--expect-different NAME_RE]

Each source is compiled with the project's flags to device assembly with kernel-resource-usage remarks.  Per kernel, the
instruction stream (comments and directives dropped, local labels folded to one token, symbol names replaced) and the remarks
(registers, LDS, scratch, occupancy) must be equal.  --rename maps an OLD demangled kernel name onto its NEW one (regex
substitution, applied in order) for kernels that were merged or moved.  Exit status 1 if any kernel present on both sides differs,
other than those --expect-different names (a kernel whose change is the point of the commit)."""
import argparse
import os
import re
import subprocess
import sys

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def kernels(tree, src):
    """{demangled name without the parameter list: (instructions, remarks)} of one source file."""
    csrc = os.path.join(tree, "mm-vqa-healthcare_amd", "csrc")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(tree, "include"), "-I" + csrc,
                        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S", os.path.join(csrc, src), "-o", "-"],
                       capture_output=True, text=True, check=True)
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", p.stdout, re.M)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    remarks = {}
    for blk in re.split(r"remark: Function Name: ", p.stderr)[1:]:
        remarks[blk.split()[0]] = tuple(re.findall(r"remark:\s+(\w[^:\[]*(?:\[[^\]]*\])?: \S+)", blk))
    out = {}
    for sym, name in zip(names, plain):
        body = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end" % re.escape(sym), p.stdout, re.M | re.S).group(1)
        ins = []
        for line in body.splitlines():
            line = line.split(";")[0].strip()
            if not line or line.startswith(".") and not line.endswith(":"):
                continue
            line = re.sub(r"\.L\w+", "L", line)
            ins.append(re.sub(r"\b_Z\w+", "SYM", line))
        key = re.sub(r"^void ", "", name)
        key = key[:key.rindex("(")].replace("(anonymous namespace)::", "")
        out[key] = (ins, remarks[sym])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--files", default="misc.hip,norm.hip,gemm_mfma.hip")
    ap.add_argument("--rename", action="append", default=[])
    ap.add_argument("--expect-different", default=None)
    args = ap.parse_args()
    bad = 0
    for src in args.files.split(","):
        old, new = kernels(args.old, src), kernels(args.new, src)
        print(f"== {src}: {len(old)} kernels old, {len(new)} new")
        matched = set()
        for name, (ins, rem) in sorted(old.items()):
            to = name
            for r in args.rename:
                pat, rep = r.split("=", 1)
                to = re.sub(pat, rep, to)
            tag = name if to == name else f"{name} -> {to}"
            if to not in new:
                print(f"  ONLY OLD   {tag} ({len(ins)} instructions)")
                continue
            matched.add(to)
            same_i, same_r = ins == new[to][0], rem == new[to][1]
            expected = bool(args.expect_different and re.search(args.expect_different, name))
            bad += not (same_i and same_r) and not expected
            print(f"  {'equal    ' if same_i and same_r else 'expected ' if expected else 'DIFFERENT'}  {tag}: {len(ins)} / {len(new[to][0])} instructions"
                  + ("" if same_r else f"; remarks {rem} / {new[to][1]}"))
        for name in sorted(set(new) - matched):
            print(f"  ONLY NEW   {name} ({len(new[name][0])} instructions)")
    print(f"== {bad} kernels present on both sides differ unexpectedly")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
