#!/usr/bin/env python3
"""Code generation of the fused layer kernels' forms, two builds side by side: for every instantiation of fwd_c32_w16_kernel,
fwd_c16_w16_kernel and bwd_c32_bf16_kernel in two device-assembly files of scn_blocked.hip (tools/isa_budget.py says how to make
one), the kernel's metadata (VGPRs, AGPRs, scratch, static LDS, the two spill counts, occupancy), the per-class static instruction
totals of tools/isa_budget.py and the s_waitcnt operands in program order.  Instantiations are paired by (kernel, activation, form):
a build that spells the form as a pack of bools (Lb0E / Lb1E in the mangled name) is read with the bit order of the FWD_* / BWD_*
flags, so a build from before the flags pairs with one from after.

    python tools/isa_forms_diff.py before.s after.s > profiles/launch_forms_isa.txt

Exit status 1 if anything outside the classes `smem` and `salu` differs."""
import collections
import re
import sys

from isa_budget import classify

KERNELS = {"fwd_c32_w16_kernel": ((1, "EXT0"), (2, "ACCUM"), (4, "FROMY"), (8, "KEEP")),
           "fwd_c16_w16_kernel": ((1, "EXT0"), (8, "KEEP")),
           "bwd_c32_bf16_kernel": ((1, "EXT0"), (2, "PAIR"), (4, "FIRST"), (8, "ACCUM"), (16, "FROMY"), (32, "DZMASK"), (64, "VISIT"))}
NAME = re.compile(r"^_ZN3scn\d+(%s)ILi(\d)E((?:Lb[01]E)+|Lj\d+E)E" % "|".join(KERNELS))
META = (("vgpr", r"^\s*\.vgpr_count:\s*(\d+)"), ("agpr", r"^\s*\.agpr_count:\s*(\d+)"),
        ("scratch", r"^\s*\.private_segment_fixed_size:\s*(\d+)"), ("lds", r"^\s*\.group_segment_fixed_size:\s*(\d+)"),
        ("sgpr_spill", r"^\s*\.sgpr_spill_count:\s*(\d+)"), ("vgpr_spill", r"^\s*\.vgpr_spill_count:\s*(\d+)"))
FREE = ("smem", "salu")


def form_of(kernel, args):
    if args.startswith("Lj"):
        return int(args[2:-1])
    bools = [a == "Lb1E" for a in re.findall(r"Lb[01]E", args)]
    return sum(bit for (bit, _), on in zip(KERNELS[kernel], bools) if on)


def form_name(kernel, form):
    return "|".join(n for bit, n in KERNELS[kernel] if form & bit) or "plain"


def read(path):
    lines = open(path).read().split("\n")
    out = {}
    i = 0
    while i < len(lines):
        m = NAME.match(lines[i])
        if not m or not re.match(r"^\S+:\s*(;.*)?$", lines[i]):          # the function's label, not a directive that names it
            i += 1
            continue
        sym = lines[i].split(":")[0]
        end = next(j for j in range(i, len(lines)) if lines[j].strip().startswith(".Lfunc_end"))
        ops = [l.split()[0:] for l in (x.strip() for x in lines[i + 1:end]) if l and not l.startswith((";", ".", "//"))]
        classes = collections.Counter(classify(o[0]) for o in ops)
        waits = [" ".join(o[1:]) for o in ops if o[0] == "s_waitcnt"]
        occ = next(int(l.split(":")[1]) for l in lines[end:end + 60] if l.startswith("; Occupancy:"))
        out[(m.group(1), int(m.group(2)), form_of(m.group(1), m.group(3)))] = {"sym": sym, "classes": classes, "waits": waits, "occupancy": occ}
        i = end
    # the metadata records (.amdgpu_metadata): one list entry per kernel, fields in alphabetical order
    by_sym = {v["sym"]: v for v in out.values()}
    cur = {}

    def commit():
        if cur.get("sym") in by_sym:
            by_sym[cur.pop("sym")].update(cur)
        cur.clear()
    for l in lines:
        if l.startswith("  - ."):                                       # (an argument's entry is indented further)
            commit()
            l = l.replace("- ", "  ", 1)
        for key, pat in META:
            m = re.match(pat, l)
            if m:
                cur[key] = int(m.group(1))
        m = re.match(r"^\s*\.symbol:\s*(\S+)\.kd", l)
        if m:
            cur["sym"] = m.group(1)
    commit()
    return out


def main():
    a, b = read(sys.argv[1]), read(sys.argv[2])
    bad = 0
    print("before: %s (%d instantiations)   after: %s (%d)" % (sys.argv[1].split("/")[-1], len(a), sys.argv[2].split("/")[-1], len(b)))
    print("%-20s %3s %-18s | %4s %4s %7s %6s %6s %6s %3s | %6s %6s | %s" % ("kernel", "act", "form", "vgpr", "agpr", "scratch", "lds", "s_spil",
                                                                               "v_spil", "occ", "d smem", "d salu", "verdict"))
    for key in sorted(set(a) | set(b)):
        k, act, form = key
        if key not in a or key not in b:
            print("%-20s %3d %-18s | only in %s" % (k, act, form_name(k, form), "before" if key in a else "after"))
            bad += 1
            continue
        x, y = a[key], b[key]
        diffs = [m for m, _ in META if x[m] != y[m]] + (["occupancy"] if x["occupancy"] != y["occupancy"] else [])
        diffs += ["class " + c for c in sorted(set(x["classes"]) | set(y["classes"])) if c not in FREE and x["classes"][c] != y["classes"][c]]
        if x["waits"] != y["waits"]:
            diffs.append("s_waitcnt operands")
        bad += bool(diffs)
        print("%-20s %3d %-18s | %4d %4d %7d %6d %6d %6d %3d | %+6d %+6d | %s" % (
            k, act, form_name(k, form), y["vgpr"], y["agpr"], y["scratch"], y["lds"], y["sgpr_spill"], y["vgpr_spill"], y["occupancy"],
            y["classes"]["smem"] - x["classes"]["smem"], y["classes"]["salu"] - x["classes"]["salu"],
            "equal (%d instructions, %d s_waitcnt)" % (sum(y["classes"].values()), len(y["waits"])) if not diffs else
            "DIFFERS: " + ", ".join("%s %s -> %s" % (d, x.get(d, x["classes"].get(d[6:], "")), y.get(d, y["classes"].get(d[6:], ""))) for d in diffs)))
    print("%d of %d instantiations differ outside %s" % (bad, len(set(a) | set(b)), " / ".join(FREE)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
