"""Instruction mix of the innermost (T-step) loop of one kernel in an AMDGPU assembly listing.
   python tools/isa_mix.py file.s [substring of the mangled kernel name]     (hipcc -S --cuda-device-only ... -o file.s)
The step loop is the innermost loop (backward branch) with the most VALU instructions, as in tools/issue_model.py.  The last
line is a digest of the kernel's whole instruction stream (comments and label numbers dropped): two listings whose digests
agree hold the same code for that kernel."""
import collections, os, re, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_digests import digest
lines = open(sys.argv[1]).read().split("\n")
pat = sys.argv[2] if len(sys.argv) > 2 else "mc_paths_kernelILi4ELi1ELi1ELb0ELb0E"
k0 = next(i for i, l in enumerate(lines) if l.startswith("_ZN3mcp") and pat in l.split(":")[0] and ":" in l)
k1 = next(i for i in range(k0, len(lines)) if "s_endpgm" in lines[i])
labels = {l.split(":")[0]: i for i, l in enumerate(lines[k0:k1], k0) if l.startswith(".LBB")}
loops = []
for i in range(k0, k1):
    m = re.search(r"s_cbranch_\w+\s+(\.LBB\w+)", lines[i])
    if m and m.group(1) in labels and labels[m.group(1)] < i:
        loops.append((labels[m.group(1)], i, m.group(1)))
inner = [(a, b, n) for a, b, n in loops if not any(a2 >= a and b2 <= b and (a2, b2) != (a, b) for a2, b2, _ in loops)]
vcount = lambda a, b: sum(1 for l in lines[a:b + 1] if l.strip().startswith("v_"))
start, end, lbl = max(inner, key=lambda t: vcount(t[0], t[1]))
ops = [l.split()[0] for l in lines[start:end + 1] if l.strip() and not l.strip().startswith(";") and not l.startswith(".")]
c = collections.Counter(ops)
valu = sum(n for o, n in c.items() if o.startswith("v_"))
print(f"{lines[k0].split(':')[0][:80]}  loop {lbl}: VALU {valu}  LDS {sum(n for o, n in c.items() if o.startswith('ds_'))}  "
      f"SMEM {sum(n for o, n in c.items() if o.startswith('s_load'))}  s_nop {c.get('s_nop', 0)}")
print("  " + "; ".join(f"{n} {o}" for o, n in c.most_common(18)))
div = {o: n for o, n in c.items() if o.startswith(("v_div_", "v_rcp_"))}
if div:
    print("  division: " + "; ".join(f"{n} {o}" for o, n in sorted(div.items())))
meta = [l.strip() for l in lines[k1:k1 + 200] if "NumVgprs" in l or "; Occupancy" in l or "ScratchSize" in l]
print("  " + " ".join(meta[:4]))
print("  code digest %s (%d instructions)" % digest(lines[k0 + 1:k1 + 1]))
