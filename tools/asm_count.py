"""How many instructions does a stretch of a gfx950 kernel issue?
usage: asm_count.py file.s <kernel-name-substring> --loop REGEX
       asm_count.py file.s <kernel-name-substring> --from REGEX[#n] --to REGEX[#n]
Reads `hipcc -S --cuda-device-only` output (as tools/asm_spills.py does).  `--loop REGEX` takes the innermost loop around the first
line matching REGEX, inner loops included, by the compiler's own block comments ("in Loop: Header=", "Parent Loop"); `--from/--to` take the lines between the n-th matches
(first by default) of two anchors, both inclusive.  Prints the vector ALU count (mnemonics starting with v_, matrix-core
v_mfma_* / v_smfmac_* counted apart), scalar ALU, LDS, memory and scratch counts and a histogram of the vector mnemonics.
It counts the TEXT of the stretch: a block that the stretch branches around (the last word of a loop, a row-skipping inner
loop) is counted once, as written.  Works without a GPU."""
import argparse, collections, re, sys


def kernel_body(lines, sub):
    start = end = None
    for i, l in enumerate(lines):
        if start is None and re.match(r"^_Z\S*:", l) and sub in l:
            start = i
        elif start is not None and (l.startswith("\t.amdhsa_kernel") or l.startswith(".Lfunc_end")):
            end = i
            break
    if start is None:
        sys.exit("no kernel whose name contains %r" % sub)
    return lines[start:end]


def blocks_of(body):
    """basic blocks with what the compiler's own comments say about their loop: (first line, last line, label, header of the
    innermost loop the block is in, headers of the loops around that one)"""
    starts = [i for i, l in enumerate(body) if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", l)]
    out = []
    for n, i in enumerate(starts):
        end = (starts[n + 1] if n + 1 < len(starts) else len(body)) - 1
        m = re.match(r"^\.(LBB\d+_\d+):", body[i])
        label = m.group(1) if m else None
        text = body[i]
        j = i + 1
        while j <= end and re.match(r"^\s+;", body[j]):   # a loop header's comment runs over several lines
            text += body[j]
            j += 1
        parents = re.findall(r"Parent Loop (BB\d+_\d+)", text)
        m = re.search(r"in Loop: Header=(BB\d+_\d+)", text)
        if m:
            header = m.group(1)
        elif "Loop Header" in text:
            header = label[1:] if label else None
        else:
            header = None
        out.append((i, end, label, header, parents))
    return out


def loop_lines(body, at):
    """the lines of the innermost loop around line `at`, inner loops included: the blocks the compiler's comments put there"""
    blocks = blocks_of(body)
    mine = [b for b in blocks if b[0] <= at <= b[1]]
    if not mine or mine[0][3] is None:
        sys.exit("line %d is in no loop" % at)
    head = mine[0][3]
    inner = {head} | {b[3] for b in blocks if b[3] and head in b[4]}   # headers of the loops nested in it
    lines = []
    for i, end, label, header, parents in blocks:
        if header in inner:
            lines += range(i, end + 1)
    return head, lines


def nth_match(body, spec, lo=0):
    rx, _, n = spec.partition("#")
    n = int(n) if n else 1
    for i in range(lo, len(body)):
        if re.search(rx, body[i]):
            n -= 1
            if n == 0:
                return i
    sys.exit("anchor %r not found" % spec)


def classify(mn):
    if mn.startswith(("v_mfma", "v_smfmac")):
        return "mfma"
    if mn.startswith("v_"):
        return "valu"
    if mn.startswith("s_"):
        return "salu"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith("scratch_"):
        return "scratch"
    if mn.startswith(("global_", "flat_", "buffer_")):
        return "vmem"
    return "other"


def count(stretch):
    cls, hist = collections.Counter(), collections.Counter()
    for l in stretch:
        t = l.strip().split()
        if not l.startswith("\t") or not t or t[0].startswith((".", ";")):
            continue
        c = classify(t[0])
        cls[c] += 1
        if c in ("valu", "mfma"):
            hist[re.sub(r"_e(32|64)$", "", t[0])] += 1
    return cls, hist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("kernel")
    ap.add_argument("--loop")
    ap.add_argument("--from", dest="a")
    ap.add_argument("--to", dest="b")
    args = ap.parse_args()
    body = kernel_body(open(args.asm).read().split("\n"), args.kernel)
    if args.loop:
        head, lines = loop_lines(body, nth_match(body, args.loop))
        stretch = [body[i] for i in lines]
        print("loop %s, %d lines in %d..%d" % (head, len(lines), lines[0], lines[-1]))
    else:
        a = nth_match(body, args.a)
        b = nth_match(body, args.b, a)
        stretch = body[a:b + 1]
        print("kernel lines %d..%d (%s .. %s)" % (a, b, body[a].strip()[:40], body[b].strip()[:40]))
    cls, hist = count(stretch)
    print("valu %d  mfma %d  salu %d  lds %d  vmem %d  scratch %d  other %d" % tuple(
        cls[k] for k in ("valu", "mfma", "salu", "lds", "vmem", "scratch", "other")))
    if cls["mfma"] > 2 and cls["mfma"] % 2 == 0:   # a loop unrolled over several words: two MFMA per word
        print("per MFMA pair: valu %.1f  salu %.1f" % (2.0 * cls["valu"] / cls["mfma"], 2.0 * cls["salu"] / cls["mfma"]))
    for mn, n in sorted(hist.items(), key=lambda x: (-x[1], x[0])):
        print("  %4d %s" % (n, mn))


main()
