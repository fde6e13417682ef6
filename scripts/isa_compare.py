"""Which kernels' machine code did a change touch?  Compares two sets of the assembly listings that
`make -C webgputracer_amd isa` writes (webgputracer_amd/build/*.s), function by function:
  git archive <parent> webgputracer_amd include | tar -x -C /tmp/parent
  make -C /tmp/parent/webgputracer_amd isa && make -C webgputracer_amd isa
  python scripts/isa_compare.py /tmp/parent/webgputracer_amd/build webgputracer_amd/build
A function's text runs from its label to its end label (the kernel descriptor included), without
comments and blank lines, with the compiler's local labels renumbered in order of appearance (their
numbers count the functions and blocks of the whole file).  Prints one line per function of either
set: same, different, or the set it is missing from; for a different one also the VGPRs, scratch
bytes per lane and waves per SIMD that the listing states for it, parent -> branch.  A function is
named by its symbol whatever file it is in, so one that moved to another file still compares."""
import glob
import os
import re
import sys

LABEL = re.compile(r"\.L(BB|tmp|JTI|CPI)\d+(_\d+)?")
USAGE = (("vgpr", r"; NumVgprs: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"), ("waves", r"; Occupancy: (\d+)"))


FUNC = re.compile(r"^\t\.type\t(\w+),@function\n\1:[^\n]*\n(.*?)^\.Lfunc_end\d+:\n(.*?)(?=^\t\.type\t\w+,@function\n|\Z)", re.S | re.M)


def functions(build_dir):
    """symbol -> (normalised text, resource usage) of every function in build_dir/*.s"""
    out = {}
    for path in sorted(glob.glob(os.path.join(build_dir, "*.s"))):
        for name, body, after in FUNC.findall(open(path).read()):
            lines = [ln.split(";")[0].rstrip() for ln in body.split("\n")]
            ids = {}
            text = LABEL.sub(lambda m: ids.setdefault(m.group(0), f".L{m.group(1)}{len(ids)}"),
                             "\n".join(ln for ln in lines if ln))
            use = {k: int(m.group(1)) for k, pat in USAGE for m in [re.search(pat, after)] if m}
            out[name] = (text, use)
    return out


def short(name):
    return re.sub(r"EEvNS_8DevScene.*|EvNS_8DevScene.*", "", name).replace("_ZN3wgt", "")


a, b = functions(sys.argv[1]), functions(sys.argv[2])
for name in sorted(set(a) | set(b)):
    if name not in a or name not in b:
        print(f"{'only in parent' if name in a else 'only in branch':16s} {short(name)}")
    elif a[name][0] == b[name][0]:
        print(f"{'same':16s} {short(name)}")
    else:
        ua, ub = a[name][1], b[name][1]
        res = "  ".join(f"{k} {ua.get(k)} -> {ub.get(k)}" for k, _ in USAGE)
        print(f"{'different':16s} {short(name)}  {res}  lines {a[name][0].count(chr(10)) + 1} -> {b[name][0].count(chr(10)) + 1}")
