"""Every kernel of AMDGPU assembly listings at once: code digest (as tools/isa_mix.py defines it: the instruction stream without
comments and label numbers; taken to the end of the function, which is isa_mix's first s_endpgm wherever a kernel has one
only), NumVgprs, ScratchSize, Occupancy and LDS bytes per _ZN3mcp kernel symbol.
   python tools/isa_digests.py DIR                       one table per listing DIR/*.s
   python tools/isa_digests.py BEFORE AFTER [unit ...]   compares the listings of the same name in two directories: per unit the
                                                          symbol counts and how many symbols agree in all five figures; for the
                                                          named units (e.g. paths_nb4) also the full per-symbol list.
Exit status 1 when a symbol is missing on one side or any figure differs.
   (listings: hipcc -S --cuda-device-only <the Makefile's flags> [-DMCP_NB=n] unit.hip -o DIR/unit.s)"""
import glob, hashlib, os, re, sys


def digest(body):
    """(digest, instructions) of a kernel's lines: comments, label numbers and directives dropped.  tools/isa_mix.py prints the same."""
    body = [re.sub(r"\.LBB\d+_\d+", "L", x.split(";")[0].strip()) for x in body]
    body = [x for x in body if x and not x.startswith(".")]
    return hashlib.sha1("\n".join(body).encode()).hexdigest()[:16], len(body)


def kernels(path):
    """{symbol: (digest, instructions, vgprs, scratch, occupancy, lds)} of one listing."""
    lines = open(path).read().split("\n")
    names = {l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")}
    out = {}
    i = 0
    while i < len(lines):
        sym = lines[i].split(":")[0]
        if not (sym.startswith("_ZN3mcp") and sym in names):
            i += 1
            continue
        k1 = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end")) - 1   # also past an s_endpgm in mid-code
        meta = {}
        for x in lines[k1:k1 + 200]:
            m = re.match(r"\s*; (NumVgprs|ScratchSize|Occupancy|LDSByteSize): (\d+)", x)
            if m:
                meta.setdefault(m.group(1), int(m.group(2)))
        out[sym] = digest(lines[i + 1:k1 + 1]) + (meta["NumVgprs"], meta["ScratchSize"], meta["Occupancy"], meta["LDSByteSize"])
        i = k1 + 1
    return out


def row(sym, k):
    return f"{sym}\n  digest {k[0]} ({k[1]} instructions)  NumVgprs {k[2]}  ScratchSize {k[3]}  Occupancy {k[4]}  LDS {k[5]} B"


def units(d):
    order = lambda u: (re.sub(r"\d+$", "", u), int(re.search(r"\d+$", u).group()) if re.search(r"\d+$", u) else 0)
    return sorted((os.path.basename(p)[:-2] for p in glob.glob(os.path.join(d, "*.s"))), key=order)


def main(argv):
    if len(argv) == 1:
        for u in units(argv[0]):
            ks = kernels(os.path.join(argv[0], u + ".s"))
            print(f"## {u}: {len(ks)} kernel symbols")
            for sym in sorted(ks):
                print(row(sym, ks[sym]))
        return 0
    before, after, full = argv[0], argv[1], argv[2:]
    bad = 0
    tot = [0, 0, 0]
    details = []
    if units(before) != units(after):
        print(f"units differ: {units(before)} / {units(after)}")
        bad = 1
    print(f"{'unit':<16}{'before':>8}{'after':>8}{'same set':>10}{'all five figures equal':>26}")
    for u in units(after):
        if u not in units(before):
            continue
        b, a = kernels(os.path.join(before, u + ".s")), kernels(os.path.join(after, u + ".s"))
        same = sum(1 for s in a if s in b and a[s] == b[s])
        print(f"{u:<16}{len(b):>8}{len(a):>8}{'yes' if set(a) == set(b) else 'NO':>10}{same:>20} / {len(a)}")
        tot = [tot[0] + len(b), tot[1] + len(a), tot[2] + same]
        bad |= set(a) != set(b) or same != len(a)
        for s in sorted(set(a) | set(b)):
            if s not in a or s not in b:
                details.append(f"{u}: {s} only {'before' if s in b else 'after'}")
            elif a[s] != b[s]:
                details.append(f"{u}: {s}\n  before {b[s]}\n  after  {a[s]}")
        if u in full:
            details.append(f"## {u}: {len(a)} kernel symbols after, each with the digest before")
            for s in sorted(a):
                details.append(row(s, a[s]) + f"\n  before: digest {b[s][0] if s in b else 'none'} ({'equal' if s in b and a[s] == b[s] else 'DIFFERENT'})")
    print(f"{'total':<16}{tot[0]:>8}{tot[1]:>8}{'':>10}{tot[2]:>20} / {tot[1]}")
    print("\n".join(details))
    return int(bad)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
