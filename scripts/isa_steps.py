"""Static instruction counts of label-delimited blocks of one kernel in an ISA dump (make isa):
the node step, the triangle step and the loop tail of k_render_ps's traversal, as tabulated in
profiles/mode_runs/README.md and profiles/tri_tail/README.md.
  python scripts/isa_steps.py build/wgt_kernels.s <kernel-symbol-substring>
      prints the kernel's outline (labels, vector and scalar loads, branches) to pick the blocks from
  python scripts/isa_steps.py build/wgt_kernels.s <kernel-symbol-substring> tri=BB60_190:BB60_221 ...
      counts each named range, from the first label up to (not including) the second, and the whole
      kernel with the resource usage the listing states for it
Columns: VALU (every v_* but lane reads and writes) / v_mov_b32 / scalar + branch / branches /
vector loads / LDS / v_readlane + v_writelane / scratch instructions."""
import re
import sys

s = open(sys.argv[1]).read()
key = sys.argv[2]
name = [m.group(1) for m in re.finditer(r"^(\S+):\s*;\s*@\1", s, re.M) if key in m.group(1)][0]
i = s.find("\n" + name + ":") + 1
j = s.find(".Lfunc_end", i)
body = s[i:j].splitlines()
after = s[j:j + 6000]

LABEL = re.compile(r"^(?:\.L(BB\d+_\d+)|; (%bb\.\d+)):")


def op_of(ln):
    t = ln.strip().split()
    if not t or t[0].startswith((".", ";")) or t[0].endswith(":"):
        return None
    return t[0]


def count(lines):
    c = dict(valu=0, mov=0, scalar=0, branch=0, vload=0, lds=0, lane=0, scratch=0)
    for ln in lines:
        op = op_of(ln)
        if op is None:
            continue
        if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
            c["lane"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
            c["mov"] += op.startswith("v_mov_b32")
        elif op.startswith("s_"):
            c["scalar"] += 1
            c["branch"] += op.startswith(("s_cbranch", "s_branch"))
        elif op.startswith(("global_load", "buffer_load", "flat_load")):
            c["vload"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith("scratch_"):
            c["scratch"] += 1
    return c


def fmt(c):
    return " / ".join(str(c[k]) for k in ("valu", "mov", "scalar", "branch", "vload", "lds", "lane", "scratch"))


at = {}
for n, ln in enumerate(body):
    m = LABEL.match(ln)
    if m:
        at[m.group(1) or m.group(2)] = n

if len(sys.argv) == 3:
    for n, ln in enumerate(body):
        op = op_of(ln)
        if LABEL.match(ln) or (op and (op.startswith(("global_load", "s_load", "s_cbranch", "s_branch", "scratch_")))):
            print(n, ln.split(";   in Loop")[0].rstrip())
    sys.exit(0)

print(name[:60])
print("block: VALU / v_mov_b32 / scalar+branch / branches / vector loads / LDS / lane r+w / scratch")
for arg in sys.argv[3:]:
    nm, rng = arg.split("=")
    tot = None
    for part in rng.split(","):  # out-of-line blocks: several ranges summed
        a, b = part.split(":")
        c = count(body[at[a]:at[b]])
        tot = c if tot is None else {k: tot[k] + c[k] for k in c}
    print(f"{nm}: {fmt(tot)}")
c = count(body)
print(f"kernel: {fmt(c)}")
print("s_load_dwordx4", sum(op_of(l) == "s_load_dwordx4" for l in body),
      "global_load_dwordx4", sum(op_of(l) == "global_load_dwordx4" for l in body))
for pat in (r"; NumSgprs: (\d+)", r"; NumVgprs: (\d+)", r"; ScratchSize: (\d+)", r"; Occupancy: (\d+)"):
    m = re.search(pat, after)
    print(pat.split(":")[0][2:], m.group(1) if m else "?")
