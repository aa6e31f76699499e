"""Code generation of two versions of one translation unit, kernel by kernel.

    F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function \
       -I include -I nem-mcmc-optimization_amd/csrc --cuda-device-only -S \
       -Rpass-analysis=kernel-resource-usage"
    hipcc $F <old>/nemo_factored_i8.hip -o old.s 2> old.rpass
    hipcc $F <new>/nemo_factored_i8.hip -o new.s 2> new.rpass
    python tools/codegen_diff.py old.s old.rpass new.s new.rpass

For every kernel symbol present in both: the compiler-reported resource
figures (the -Rpass-analysis=kernel-resource-usage remarks, and the private
segment and static LDS sizes of the kernel descriptor) and the whole opcode
histogram of the kernel's body.  Prints the kernel counts, the symbols only
one side has, and every kernel whose figures or histogram differ (with the
differing entries); exit status 1 if any resource figure differs.
"""
import re
import shutil
import subprocess
import sys
from collections import Counter

DESC = (".amdhsa_private_segment_fixed_size", ".amdhsa_group_segment_fixed_size")


def parse_asm(path):
    """{symbol: (opcode histogram, {descriptor field: value})} of the kernels"""
    lines = open(path).read().split("\n")
    desc, cur = {}, None
    for l in lines:
        t = l.strip()
        if t.startswith(".amdhsa_kernel "):
            cur = t.split()[1]
            desc[cur] = {}
        elif t == ".end_amdhsa_kernel":
            cur = None
        elif cur and t.startswith(DESC):
            k, v = t.split()[:2]
            desc[cur][k[len(".amdhsa_"):]] = v
    out = {}
    i = 0
    while i < len(lines):
        m = re.match(r"^([A-Za-z_][\w$.]*):", lines[i])
        if m and m.group(1) in desc:
            ops = Counter()
            i += 1
            while i < len(lines) and not lines[i].startswith(".Lfunc_end"):
                t = lines[i].strip()
                if t and not t.startswith((";", ".")) and not t.endswith(":"):
                    ops[t.split()[0]] += 1
                i += 1
            out[m.group(1)] = (ops, desc[m.group(1)])
        i += 1
    return out


def parse_rpass(path):
    """{symbol: {figure: value}} from the kernel-resource-usage remarks"""
    out, cur = {}, None
    for l in open(path):
        m = re.search(r"remark: Function Name: (\S+)", l)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([^:]+): (\S+) \[-Rpass-analysis", l)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return out


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True)
        short = [re.sub(r"^void nemo::\(anonymous namespace\)::|\(.*$", "", s) for s in r.stdout.split("\n")]
        return dict(zip(names, short))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    olds, oldr, news, newr = sys.argv[1:5]
    a, b = parse_asm(olds), parse_asm(news)
    ra, rb = parse_rpass(oldr), parse_rpass(newr)
    names = demangle(sorted(set(a) | set(b)))
    print(f"kernels: old {len(a)}, new {len(b)}, in both {len(set(a) & set(b))}")
    for tag, only in (("old", set(a) - set(b)), ("new", set(b) - set(a))):
        for n in sorted(only, key=names.get):
            print(f"only in {tag}: {names[n]}")
    bad = same = 0
    for n in sorted(set(a) & set(b), key=names.get):
        fa = {**ra.get(n, {}), **a[n][1]}
        fb = {**rb.get(n, {}), **b[n][1]}
        res = {k: (fa.get(k), fb.get(k)) for k in sorted(set(fa) | set(fb)) if fa.get(k) != fb.get(k)}
        ha, hb = a[n][0], b[n][0]
        ops = {k: (ha[k], hb[k]) for k in sorted(set(ha) | set(hb)) if ha[k] != hb[k]}
        if not res and not ops:
            same += 1
            continue
        bad += bool(res)
        print(f"{names[n]}: instructions {sum(ha.values())} -> {sum(hb.values())}")
        for k, (x, y) in res.items():
            print(f"    RESOURCE {k}: {x} -> {y}")
        for k, (x, y) in ops.items():
            print(f"    {k}: {x} -> {y}")
    print(f"equal figures and histogram: {same} of {len(set(a) & set(b))} kernels; resource differences in {bad}")
    if "-v" in sys.argv:
        for n in sorted(set(a) & set(b), key=names.get):
            f = {**rb.get(n, {}), **b[n][1]}
            print(names[n], sum(b[n][0].values()), " ".join(f"{k}={v}" for k, v in f.items()))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
