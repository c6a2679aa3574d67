#!/usr/bin/env python3
"""Two states of the kernels, kernel by kernel: the device assembly of `make OUT=<file> device-asm` and the
remarks of `make resource-usage`, for a parent tree (a `git archive` of it) and this one.

  python tools/device_asm_compare.py OLD.s NEW.s OLD_resource_usage.txt NEW_resource_usage.txt [OLD_SYMBOL_PART=NEW_SYMBOL_PART ...]

Whole files are only equal while no kernel is added, removed or renamed, so the comparison is per kernel: `__hip_cuid_<hex>` (names the
compilation unit by a hash of its text) is masked, the renames given on the command line are applied to the parent's mangled symbols
(parts of a symbol, with their length prefix: 15k_read_chain_lw=14k_read_chain_t), and the labels the compiler numbers through the whole
file — .LBB<function>_<block>, .Lfunc_begin / .Lfunc_end<function>, .Lpost_getpc<n> — lose their file-wide number, which shifts when a
kernel in front of them goes.  Prints the kernels only one side has, every kernel whose text or resource-usage lines differ, and one
SHA-256 per side over the text of the kernels both have."""
import hashlib
import re
import sys


def resource_usage(path):
    d, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: (.*?)( \[-Rpass-analysis=kernel-resource-usage\])?$", line.rstrip())
        if not m:
            continue
        f = re.match(r"Function Name: (\S+)", m.group(1))
        if f:
            cur = f.group(1)
            d[cur] = []
        elif cur:
            d[cur].append(m.group(1).strip())
    return d


def kernels(path):
    s = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(path).read())
    d = {}
    for m in re.finditer(r"^\s*\.globl\s+(\S+).*?^\.Lfunc_end\d+:.*?(?=^\s*\.(?:section|protected|globl|weak|text))", s, re.M | re.S):
        d[m.group(1)] = m.group(0)
    return d, hashlib.sha256(s.encode()).hexdigest(), len(s)


def unnumbered(t):
    t = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1N", t)
    t = re.sub(r"BB\d+_", "BBN_", t)
    t = re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpcN", t)
    return re.sub(r"[ \t]+;", " ;", t)


def main():
    old_s, new_s, old_ru, new_ru = sys.argv[1:5]
    renames = [a.split("=") for a in sys.argv[5:]]

    def renamed(t):
        for a, b in renames:
            t = t.replace(a, b)
        return t

    ro = {renamed(k): v for k, v in resource_usage(old_ru).items()}
    rn = resource_usage(new_ru)
    print("resource-usage: %d functions before, %d after" % (len(ro), len(rn)))
    print("  only before:", sorted(set(ro) - set(rn)))
    print("  only after: ", sorted(set(rn) - set(ro)))
    print("  lines differ:", sorted(k for k in set(ro) & set(rn) if ro[k] != rn[k]))
    for k in sorted(rn):
        if any(b in k for _, b in renames) and k in ro:
            print("  %s: %s" % (k, "; ".join(rn[k])))
    (ao, ho, lo), (an, hn, ln) = kernels(old_s), kernels(new_s)
    print("assembly, __hip_cuid masked: before %d bytes sha256 %s, after %d bytes sha256 %s" % (lo, ho, ln, hn))
    ao = {renamed(k): unnumbered(renamed(v)) for k, v in ao.items()}
    an = {k: unnumbered(v) for k, v in an.items()}
    both = sorted(set(ao) & set(an))
    print("  kernels: %d before, %d after, %d in both" % (len(ao), len(an), len(both)))
    print("  only before:", sorted(set(ao) - set(an)))
    print("  only after: ", sorted(set(an) - set(ao)))
    differ = [k for k in both if ao[k] != an[k]]
    for k in differ:
        x, y = ao[k].split("\n"), an[k].split("\n")
        print("  DIFFERS: %s, %d / %d lines, %d differ" % (k, len(x), len(y), sum(p != q for p, q in zip(x, y)) + abs(len(x) - len(y))))
    print("  identical: %d, differing: %d" % (len(both) - len(differ), len(differ)))
    for name, d in (("before", ao), ("after", an)):
        h = hashlib.sha256()
        for k in both:
            h.update(d[k].encode())
        print("  sha256 over the kernels in both, %s: %s" % (name, h.hexdigest()))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
