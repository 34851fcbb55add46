#!/usr/bin/env python3
"""The LDS instructions of the kernels in a hipcc -S listing, by form, priced in LDS-array cycles per wave-instruction (ds_read_b64 2,
ds_read_b128 4, ds_read2_b64 8, ds_write_b64 6, ds_write_b128 / ds_write2_b64 13, others 4), segment by segment: a segment ends at every
s_barrier and at every loop header, so a straight-line phase between two barriers and a loop body are counted apart.  With the kernel's
VGPRs, scratch and occupancy as the compiler states them.   usage: asm_lds_forms.py file.s kernel-substring [--segments]"""
import collections, re, sys
COST = {"ds_read_b64": 2, "ds_read_b128": 4, "ds_read2_b64": 8, "ds_read2st64_b64": 8, "ds_write_b64": 6, "ds_write_b128": 13, "ds_write2_b64": 13}
lines = open(sys.argv[1]).read().split("\n")
for start, l in enumerate(lines):
    m = re.match(r"^(_Z\S*" + re.escape(sys.argv[2]) + r"\S*):", l)
    if not m:
        continue
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    tail = "\n".join(lines[end:end + 60])
    res = [re.search(k + r":\s*(\d+)", tail) for k in (r"; NumVgprs", r"; ScratchSize", r"; Occupancy")]
    segs, cur = [], collections.Counter()
    for i in range(start, end):
        s = lines[i].strip()
        if s.startswith("s_barrier") or "Loop Header" in s:
            segs.append((i - start, s.split()[0] if s.startswith("s_barrier") else "loop", cur)); cur = collections.Counter()
        elif s.startswith("ds_"):
            cur[s.split()[0]] += 1
    segs.append((end - start, "end", cur))
    total = sum((c for _, _, c in segs), collections.Counter())
    price = lambda c: sum(COST.get(k, 4) * n for k, n in c.items())
    fmt = lambda c: ", ".join("%d %s" % (n, k) for k, n in sorted(c.items())) or "-"
    print("%s\n   VGPRs %s  scratch %s  occupancy %s   | %s | %d LDS-array cycles per wave" % ((m.group(1),) + tuple(r.group(1) if r else "?" for r in res) + (fmt(total), price(total))))
    if "--segments" in sys.argv:
        for off, why, c in segs:
            if c:
                print("      up to +%-5d (%s): %s | %d" % (off, why, fmt(c), price(c)))
