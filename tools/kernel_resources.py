"""Kernel resources and device assembly of rt_launch.hip, parent commit against this change, without a GPU.

  make -C raytrace-miniapp_amd/csrc asm 2> new.log        (in a checkout of each commit: the remarks of
                                                            -Rpass-analysis=kernel-resource-usage and rt_launch.gfx950.s)
  python tools/kernel_resources.py parent.log parent.s new.log new.s [note ...] > profiles/NAME.txt

Prints the table of profiles/step_kernel_resources.txt, then per kernel whether the instruction stream is the parent's
(comments, directives and the numbering of labels left out), with the instruction counts where it is not.
Exit status 1 if a resource figure of an existing kernel changed or a kernel is missing."""
import re
import subprocess
import sys

FIELDS = ("VGPRs", "AGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
          "Occupancy [waves/SIMD]")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}
    short = {}
    for n, d in zip(names, out):
        d = re.sub(r"^void ", "", d).replace("rt::", "")
        short[n] = re.sub(r"\((?:[^()]|\([^()]*\))*\)$", "", d)  # the argument list
    return short


def resources(log):
    """{mangled name: tuple of FIELDS}, in the order of the listing"""
    res, name = {}, None
    for line in open(log):
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        key, _, val = m.group(1).partition(": ")
        if key == "Function Name":
            name = val
            res[name] = {}
        elif name is not None and key.strip() in FIELDS:
            res[name][key.strip()] = val.strip()
    return {n: tuple(r.get(f, "?") for f in FIELDS) for n, r in res.items()}


def streams(asm, names):
    """{name: list of instructions} of the given functions: no comments, no directives, labels numbered by appearance"""
    out, cur, labels = {}, None, {}
    for line in open(asm):
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and m.group(1) in names:
            cur, labels = m.group(1), {}
            out[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        text = line.split(";")[0].strip()
        if not text or text.startswith("."):
            continue  # comment, directive or label
        text = re.sub(r"\.LBB\d+_\d+", lambda k: labels.setdefault(k.group(0), f".L{len(labels)}"), text)
        out[cur].append(re.sub(r"\s+", " ", text))
    return out


def main():
    plog, pasm, nlog, nasm = sys.argv[1:5]
    pres, nres = resources(plog), resources(nlog)
    names = list(dict.fromkeys(list(pres) + list(nres)))
    short = demangle(names)
    print("Kernel resources of rt_launch.hip for gfx950 (make -C raytrace-miniapp_amd/csrc asm: hipcc -O3 --offload-arch=gfx950")
    print("-Rpass-analysis=kernel-resource-usage), parent commit and this change side by side.  No GPU is needed for this listing.")
    print("Columns: VGPRs / AGPRs / SGPRs / SGPR spills (to VGPR lanes) / VGPR spills / scratch bytes per lane / static LDS bytes / waves per SIMD")
    print("by registers.  The LDS of these kernels is dynamic.\n")
    print(f"{'kernel':<62} | {'parent':<40} | this change")
    changed = missing = new = 0
    for n in names:
        a, b = pres.get(n), nres.get(n)
        changed += a is not None and b is not None and a != b
        missing += b is None
        new += a is None
        print(f"{short[n]:<62} | {' / '.join(a) if a else '(new)':<40} | {' / '.join(b) if b else '(missing)'}{'   <-- CHANGED' if a and b and a != b else ''}")
    print(f"\nexisting kernel instances: {len(pres)}, changed in any column: {changed}, missing from this change: {missing}; new instances: {new}")

    ps, ns = streams(pasm, set(names)), streams(nasm, set(names))
    same = [n for n in names if n in ps and n in ns and ps[n] == ns[n]]
    differ = [n for n in names if n in ps and n in ns and ps[n] != ns[n]]
    print("\nDevice assembly (rt_launch.gfx950.s), instruction by instruction, comments, directives and label numbers left out:")
    print(f"identical instruction stream: {len(same)} of {len(names)} kernels" + (":" if differ else " -- every one."))
    if differ:
        for n in same:
            print(f"    {short[n]}")
        print("different instruction stream (instructions parent -> this change; lines of a unified diff):")
        import difflib
        for n in differ:
            d = sum(1 for l in difflib.unified_diff(ps[n], ns[n], lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---"))
            print(f"    {short[n]:<58} {len(ps[n]):6d} -> {len(ns[n]):6d}   ({d} lines differ)")
    for note in sys.argv[5:]:
        print("\n" + note)
    return 1 if changed or missing else 0


if __name__ == "__main__":
    sys.exit(main())
