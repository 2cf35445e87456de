#!/usr/bin/env python3
"""tools/asm_same.py <base.s> <new.s> [renames] : per kernel of two device listings: A (same text), B (same instructions and descriptor, registers renamed, local labels renumbered) or DIFFERENT, whose differing lines follow; a kernel only one listing has is NEW / GONE; exit status 1 if any kernel both listings have is neither A nor B, or one is GONE.  renames: a file of `old-symbol new-symbol` lines; a base kernel named there is compared, its name replaced in its text, with the new listing's kernel of the new name"""
import difflib, re, sys
REG = re.compile(r"\b([sva])\[(\d+):(\d+)\]|\b(?:([sva])\d+|(vcc_lo|vcc_hi)|(vcc))\b")   # s12, v7, a3, s[4:5], vcc, vcc_lo, vcc_hi as operands
def blank(m):
    """a register operand without its number: its file (vcc counts as SGPRs) and how many registers wide it is stay"""
    if m.group(1): return "%s[%d]" % (m.group(1), int(m.group(3)) - int(m.group(2)) + 1)
    return m.group(4) or ("s" if m.group(5) else "s[2]")

def kernels(path):
    """symbol -> the lines from `symbol:` to its .end_amdhsa_kernel, in one pass (lines that carry the source text's hash are left out)"""
    out, open_ = {}, {}   # open_: every symbol seen since the last kernel ended -> its lines so far
    for l in open(path):
        l = l.rstrip()
        if "__hip_cuid_" in l: continue
        m = re.match(r"([A-Za-z_]\w*):", l)
        if m: open_[m.group(1)] = []
        for body in open_.values(): body.append(l)
        if l.strip().startswith(".amdhsa_kernel "): sym = l.split()[1]
        if l.strip() == ".end_amdhsa_kernel": out[sym], open_ = open_[sym], {}
    return out

def blanked(body):
    """instructions, labels and directives with every register operand blanked; comments dropped"""
    code = (l.split(";")[0].rstrip() for l in body if ".amdhsa_" not in l)
    # (a function's local labels carry its ordinal in the listing, .LBB<ordinal>_<block>: a kernel added before it renumbers them)
    return [re.sub(r"\.(LBB|LJTI|LCPI)\d+_", r".\1_", REG.sub(blank, l)) for l in code if l]

base, new = kernels(sys.argv[1]), kernels(sys.argv[2])
for old, sym in (l.split() for l in open(sys.argv[3]) if l.strip()) if len(sys.argv) > 3 else ():
    if old in base: base[sym] = [l.replace(old, sym) for l in base.pop(old)]
count = {"A": 0, "B": 0, "DIFFERENT": 0, "NEW": 0, "GONE": 0}
for sym in sorted(set(base) | set(new)):
    a, b = base.get(sym), new.get(sym)
    if a is None or b is None: cls = "NEW" if a is None else "GONE"   # a kernel only one listing has
    elif a == b: cls = "A"
    elif blanked(a) == blanked(b) and [l for l in a if ".amdhsa_" in l] == [l for l in b if ".amdhsa_" in l]: cls = "B"
    else: cls = "DIFFERENT"
    count[cls] += 1
    print("%-9s %s" % (cls, sym))
    if cls == "DIFFERENT":   # (as compared: registers blanked, except where the two have the same number of lines, which then pair up as written)
        if len(a) == len(b): print("\n".join("    - %s\n    + %s" % (x.strip(), y.strip()) for x, y in zip(a, b) if blanked([x]) != blanked([y]) or (".amdhsa_" in x and x != y)))
        else: print("\n".join("    " + l for l in difflib.unified_diff(blanked(a), blanked(b), "", "", lineterm="", n=0) if l[:2] not in ("--", "++")))
print("%d kernels: A %d  B %d  different %d  new %d  gone %d" % (len(set(base) | set(new)), count["A"], count["B"], count["DIFFERENT"], count["NEW"], count["GONE"]))
sys.exit(1 if count["DIFFERENT"] or count["GONE"] else 0)   # (a kernel that vanished is a change to the existing instantiations; a NEW one is not)
