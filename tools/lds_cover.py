"""How far ahead of its wait each LDS read of a loop body is issued.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S \
        -I include -I nem-mcmc-optimization_amd/csrc <file>.hip -o k.s
    python tools/lds_cover.py k.s <substring of the mangled kernel name> <label> [-v]

A plain-text parser, no GPU.  The loop body is the basic block that starts at
<label> (".LBB31_137") and everything up to the next label, so a conditional
tail without a label of its own (a set finish) is part of it.  For
every LDS read (ds_read_* / ds_load_*) in it the tool prints the issue cycles
between the read and the first s_waitcnt that covers it, and for the body the
number of s_waitcnt lgkmcnt(0), of s_nop and of the wait states the nops pad.

Assumptions, all of them rough on purpose (this measures distances in the
instruction stream, it does not simulate the CU):

  * LDS operations return in order, so "s_waitcnt lgkmcnt(n)" covers a read
    once at least n LDS operations were issued after it; every ds_ instruction
    (reads and writes) counts against lgkmcnt;
  * prices in issue cycles of one wave:  VALU 4,  MFMA 8,  s_nop n: n + 1,
    anything else 1;
  * a read that no wait of the body covers is "open": it is consumed in a
    later block, and its distance is that to the end of the body, a lower bound.
"""
import re
import statistics
import sys

VALU_CYCLES = 4
MFMA_CYCLES = 8
OTHER_CYCLES = 1
NEAR = 32  # a read waited on within this many issue cycles had no cover

_LABEL = re.compile(r"^([.\w$]+):")
_LGKM = re.compile(r"lgkmcnt\((\d+)\)")


def _instructions(text):
    """(label or None, instruction text) per line that holds one of either."""
    for line in text.split("\n"):
        m = _LABEL.match(line)
        if m:
            yield m.group(1), None
            continue
        t = line.split(";")[0].strip()
        if t and not t.startswith("."):
            yield None, t


def body_of(text, label):
    """The instructions from ``label`` up to the next label."""
    out, inside = [], False
    for lab, ins in _instructions(text):
        if lab is not None:
            if inside:
                break
            inside = lab == label
            continue
        if inside:
            out.append(ins)
    if not inside and not out:
        raise ValueError(f"label {label} not found")
    return out


def kernel_text(text, name):
    """The part of an assembly file that is the first kernel whose mangled name
    contains ``name`` (labels are only unique inside one function)."""
    lines = text.split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^\S*" + re.escape(name) + r"\S*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return "\n".join(lines[start + 1:end])


def _price(op, ins):
    if op.startswith("v_mfma"):
        return MFMA_CYCLES
    if op.startswith("v_"):
        return VALU_CYCLES
    if op == "s_nop":
        return int(ins.split()[1], 0) + 1
    return OTHER_CYCLES


def cover(text, label):
    """Parse the loop body at ``label`` of the assembly ``text``.

    Returns a dict: ``reads`` (one dict per LDS read, in issue order: ``op``,
    ``at`` = issue cycle in the body, ``dist`` = issue cycles to the covering
    wait, ``count`` = that wait's lgkmcnt, None when open, ``mfma_between``,
    ``valu_between``), ``lgkmcnt0``, ``nops``, ``nop_wait_states``, ``mfma``,
    ``valu``, ``cycles``, ``mfma_before_f64_fma``."""
    ins = body_of(text, label)
    reads, pending = [], []  # pending: reads no wait has covered yet
    clock = n_ds = valu = mfma = lgkm0 = nops = nop_states = 0
    mfma_before_fma = None
    for t in ins:
        op = t.split()[0]
        if op == "s_waitcnt":
            m = _LGKM.search(t)
            if m:
                n = int(m.group(1))
                lgkm0 += n == 0
                still = []
                for r in pending:
                    if n_ds - r["_seq"] - 1 >= n:
                        r.update(dist=clock - r["at"], count=n, mfma_between=mfma - r["_mfma"],
                                 valu_between=valu - r["_valu"])
                    else:
                        still.append(r)
                pending = still
        elif op.startswith("ds_"):
            if op.startswith(("ds_read", "ds_load")):
                r = {"op": op, "at": clock, "dist": None, "count": None, "_seq": n_ds, "_mfma": mfma, "_valu": valu}
                reads.append(r)
                pending.append(r)
            n_ds += 1
        elif op == "s_nop":
            nops += 1
            nop_states += int(t.split()[1], 0) + 1
        elif op.startswith("v_mfma"):
            mfma += 1
        elif op.startswith("v_"):
            valu += 1
            if mfma_before_fma is None and re.match(r"v_(fma|fmac)_f64", op):
                mfma_before_fma = mfma
        clock += _price(op, t)
    for r in pending:  # open: a lower bound
        r.update(dist=clock - r["at"], mfma_between=mfma - r["_mfma"], valu_between=valu - r["_valu"])
    for r in reads:
        for k in ("_seq", "_mfma", "_valu"):
            del r[k]
    return {"reads": reads, "lgkmcnt0": lgkm0, "nops": nops, "nop_wait_states": nop_states, "mfma": mfma,
            "valu": valu, "cycles": clock, "mfma_before_f64_fma": mfma_before_fma}


def summary(res):
    """Per read width: how many, how many waited on within NEAR cycles, how
    many drained by an lgkmcnt(0) within NEAR cycles, the median distance."""
    rows = {}
    for r in res["reads"]:
        rows.setdefault(r["op"], []).append(r)
    out = {}
    for op, rs in sorted(rows.items()):
        closed = [r for r in rs if r["count"] is not None]
        out[op] = {"reads": len(rs), "open": len(rs) - len(closed),
                   "near": sum(r["dist"] <= NEAR for r in closed),
                   "near_drained": sum(r["dist"] <= NEAR and r["count"] == 0 for r in closed),
                   "min": min(r["dist"] for r in rs), "median": statistics.median(r["dist"] for r in rs)}
    return out


def main():
    path, name, label = sys.argv[1:4]
    res = cover(kernel_text(open(path).read(), name), label)
    if "-v" in sys.argv:
        for i, r in enumerate(res["reads"]):
            how = "open" if r["count"] is None else f"lgkmcnt({r['count']})"
            print(f"{i:3d} {r['op']:14s} at {r['at']:5d} dist {r['dist']:5d} {how:12s} "
                  f"mfma {r['mfma_between']:2d} valu {r['valu_between']:3d}")
    print(f"{label}: {res['cycles']} issue cycles, {res['valu']} VALU, {res['mfma']} MFMA, "
          f"{res['mfma_before_f64_fma']} MFMA before the first f64 FMA")
    print(f"  s_waitcnt lgkmcnt(0): {res['lgkmcnt0']}   s_nop: {res['nops']} / {res['nop_wait_states']} wait states")
    for op, s in summary(res).items():
        print(f"  {op}: {s['reads']} reads, {s['near']} waited on within {NEAR} cycles "
              f"({s['near_drained']} by lgkmcnt(0)), {s['open']} open, distance min {s['min']} median {s['median']}")


if __name__ == "__main__":
    main()
