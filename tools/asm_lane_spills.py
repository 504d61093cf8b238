"""Which wave-uniform scalars does a gfx950 kernel park in vector lanes, and where does it fetch them back?
usage: asm_lane_spills.py file.s <kernel-name-substring> [--lines] [--all-loops]
Reads `hipcc -S --cuda-device-only` output (as tools/asm_spills.py and tools/asm_count.py do).  When a kernel runs out of
SGPRs the register allocator spills them into the lanes of a VGPR: `v_writelane_b32 vN, sM, <lane>` parks one and
`v_readlane_b32 sM, vN, <lane>` fetches it back, both with a CONSTANT lane, both on the vector pipe.  The tool counts
those two forms and the scratch accesses per loop nest, by the compiler's own block comments ("Loop Header", "in Loop:
Header=", "Parent Loop"): `own` is the text of the loop outside its inner loops, `all` includes them.  Designed lane traffic --
a lane taken from an SGPR or m0, as the row tables of knn_brick do, or a write whose source is no scalar register -- is
not a spill and is listed apart as `var`.  Loop nests that hold neither are left out unless `--all-loops` is given.  Ends with the kernel's Sgpr / Vgpr / Scratch / Occupancy lines.  `--lines` also
prints every counted line with its loop.  It counts TEXT, as asm_count.py does: a block the path branches around still counts.
Works without a GPU."""
import argparse, collections, re, sys

SREG = r"(?:s\d+|vcc_lo|vcc_hi|exec_lo|exec_hi|ttmp\d+)"
RD = re.compile(r"^\s*v_readlane_b32\s+(%s),\s*v\d+,\s*(\S+)" % SREG)
WR = re.compile(r"^\s*v_writelane_b32\s+v\d+,\s*(\S+?),\s*(\S+)")
CONST = re.compile(r"^(?:\d+|0x[0-9a-fA-F]+)$")
KEYS = ("rd", "wr", "var", "sld", "sst", "valu")


def kernel_text(lines, sub):
    """(body, trailer): the instructions of the first kernel whose mangled name contains `sub`, and the lines after
    them up to the next function, where the compiler writes its resource comments"""
    start = end = None
    for i, l in enumerate(lines):
        if start is None:
            if re.match(r"^_Z\S*:", l) and sub in l:
                start = i
        elif l.startswith(".Lfunc_end"):
            end = i
            break
    if start is None:
        sys.exit("no kernel whose name contains %r" % sub)
    if end is None:
        end = len(lines)
    stop = end
    while stop < len(lines) and not (stop > end and re.match(r"^_Z\S*:", lines[stop])):
        stop += 1
    return lines[start:end], lines[end:stop]


def classify(line):
    """one of KEYS, or None, for a line of assembly"""
    t = line.strip().split()
    if not line.startswith(("\t", " ")) or not t or t[0].startswith((".", ";")):
        return None
    m = RD.match(line)
    if m:
        return "rd" if CONST.match(m.group(2)) else "var"
    m = WR.match(line)
    if m:
        return "wr" if CONST.match(m.group(2)) and re.match("^%s$" % SREG, m.group(1)) else "var"
    if t[0].startswith(("v_readlane", "v_writelane")):
        return "var"
    if t[0].startswith("scratch_load"):
        return "sld"
    if t[0].startswith("scratch_store"):
        return "sst"
    return "valu" if t[0].startswith("v_") else None


def loops_of(body):
    """per line the header of the innermost loop around it (None outside every loop), and per header its parent headers,
    innermost first"""
    starts = [i for i, l in enumerate(body) if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", l)]
    where, parents = [None] * len(body), {}
    for n, i in enumerate(starts):
        end = starts[n + 1] if n + 1 < len(starts) else len(body)
        text, j = body[i], i + 1
        while j < end and re.match(r"^\s+;", body[j]):   # a loop header's comment runs over several lines
            text += body[j]
            j += 1
        m = re.search(r"in Loop: Header=(BB\d+_\d+)", text)
        label = re.match(r"^\.(LBB\d+_\d+):", body[i])
        header = m.group(1) if m else (label.group(1)[1:] if label and "Loop Header" in text else None)
        if header is not None:
            if "Loop Header" in text:   # only the header's own comment names the loops around it, outermost first
                parents[header] = re.findall(r"Parent Loop (BB\d+_\d+)", text)[::-1]
            else:
                parents.setdefault(header, [])
        for k in range(i, end):
            where[k] = header
    return where, parents


def analyse(lines, sub):
    body, trailer = kernel_text(lines, sub)
    where, parents = loops_of(body)
    own = collections.defaultdict(collections.Counter)
    hits = []
    for i, l in enumerate(body):
        c = classify(l)
        if c:
            own[where[i]][c] += 1
            if c != "valu":
                hits.append((i, where[i], c, l.strip()))
    total = collections.defaultdict(collections.Counter)
    for h, cnt in own.items():
        total[h].update(cnt)
        for p in parents.get(h, []):
            total[p].update(cnt)
    order = sorted((h for h in parents), key=lambda h: next(i for i, w in enumerate(where) if w == h))
    meta = {}
    for l in trailer:
        m = re.match(r"^;\s*(TotalNumSgprs|NumVgprs|ScratchSize|Occupancy):\s*(\d+)", l)
        if m:
            meta[m.group(1)] = int(m.group(2))
    whole = collections.Counter()
    for cnt in own.values():
        whole.update(cnt)
    return {"own": own, "all": total, "parents": parents, "order": order, "meta": meta, "kernel": whole, "hits": hits,
            "name": body[0].rstrip(":")}


def fmt(c):
    return "rd %4d  wr %4d  var %3d  scratch ld %3d st %3d  valu %5d" % tuple(c[k] for k in KEYS)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("kernel")
    ap.add_argument("--lines", action="store_true")
    ap.add_argument("--all-loops", action="store_true")
    args = ap.parse_args(argv)
    r = analyse(open(args.asm).read().split("\n"), args.kernel)
    print("kernel", r["name"][:150])
    print("%-34s %s" % ("whole kernel", fmt(r["kernel"])))
    print("%-34s %s" % ("outside every loop", fmt(r["own"][None])))
    for h in r["order"]:
        if not args.all_loops and not any(r["all"][h][k] for k in ("rd", "wr", "sld", "sst")):
            continue   # a loop nest without parked scalars or scratch: only listed on request
        d = len(r["parents"][h])
        tag = "%sloop %s depth %d" % ("  " * d, h, d + 1)
        print("%-34s own %s" % (tag, fmt(r["own"][h])))
        if any(h in ps for ps in r["parents"].values()):
            print("%-34s all %s" % ("", fmt(r["all"][h])))
    if args.lines:
        for i, h, c, text in r["hits"]:
            print("%6d %-4s %-12s %s" % (i, c, h or "-", text[:90]))
    print("Sgpr %s  Vgpr %s  Scratch %s  Occupancy %s" % tuple(
        r["meta"].get(k, "?") for k in ("TotalNumSgprs", "NumVgprs", "ScratchSize", "Occupancy")))


if __name__ == "__main__":
    main()
