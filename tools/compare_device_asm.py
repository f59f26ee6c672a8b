"""Compare the device code of one translation unit before and after a host-only change.

    hipcc <build.py FLAGS> [-D...] --cuda-device-only -S vaura_amd/csrc/UNIT.hip -o UNIT.s     (once per tree)
    python tools/compare_device_asm.py OLD.s NEW.s

identical: equal bytes once the compile-unit id (__hip_cuid_<hash of the source path and options>) and the blanks that align the comment
           behind a local label (their count follows the digits of the function's index in the unit) are masked.
same-set : not identical, but equal after splitting at the function symbols and at the kernels' metadata records, masking the index of
           the function in its local labels (.LBB<i>_<j>, .Lfunc_end<i>) and sorting: host code instantiated the templates in another
           order; the set of symbols and every instruction stream are equal.  Anything else exits 1.

    python tools/compare_device_asm.py --subset OLD.s NEW.s
subset   : for a change that ADDS kernels to the unit: every function of OLD and every metadata record of OLD's kernels is in NEW,
           equal byte for byte under the same masking; the functions NEW adds are listed.  The padding the assembler puts behind the
           LAST function of the unit (.p2alignl / .fill of s_code_end words) is taken off first: it follows whichever function the
           unit ends with, not that function's code.  Anything else exits 1.

    python tools/compare_device_asm.py --moved OLD.s NEW1.s [NEW2.s ..] [--gone SYMBOL ..]
moved    : for a change that SPLITS a unit: the functions and metadata records of OLD are those of the NEW units taken together, equal
           byte for byte under the same masking, every one in exactly one NEW unit, none added, and the ones missing are exactly the
           SYMBOLs expected to disappear.  Anything else exits 1."""
import hashlib
import re
import sys


def load(p):
    # the compile-unit id, and the run of blanks that aligns a trailing "; comment" behind a local label: its width follows the number of
    # digits of the function's index in the unit (.LBB99_3: -> .LBB100_3:), which a unit that gains functions changes for the old ones
    return re.sub(r"(?m)^(\.L\w+:) +;", r"\1 ;", re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", open(p).read()))


def pieces(t):
    head, meta = t.split("\t.amdgpu_metadata\n")
    head, trailer = head.split("\t.section\t.AMDGPU.gpr_maximums")      # what follows the last function
    funcs = re.split(r"(?m)^(?=(?:\t\.section\t\.text\.\S+\n|\t\.text\n)?\t\.(?:protected|globl|weak)\t\S+ *; -- Begin function)", head)
    funcs = [re.sub(r"BB\d+_", "BB_", re.sub(r"(Lfunc_end|Lfunc_begin|LJTI|Ltmp|LCPI)\d+", r"\1", f)) for f in funcs]
    meta, tail = meta.split("amdhsa.target:")
    recs = re.split(r"(?m)^(?=  - \.(?:agpr_count|args):)", meta)
    return sorted(funcs) + [trailer, "<metadata>"] + sorted(recs) + [tail]


PAD = re.compile(r"\t\.text\n\t\.p2alignl \d+, \d+\n\t\.fill \d+, \d+, \d+\n\Z")


def subset(a, b):
    pa, pb = ([PAD.sub("", x) for x in pieces(t)] for t in (a, b))
    ia, ib = pa.index("<metadata>"), pb.index("<metadata>")
    fa, fb = pa[:ia - 1], set(pb[:ib - 1])                  # functions (without the trailer)
    ra, rb = pa[ia + 1:-1], set(pb[ib + 1:-1])              # metadata records (without the tail)
    missing = [f for f in fa if f not in fb] + [r for r in ra if r not in rb]
    added = sorted(m.group(1) for f in fb - set(fa) for m in [re.search(r"\t\.(?:protected|globl|weak)\t(\S+)", f)] if m)
    return missing, added, sha("".join(fa + ra))


def symbol(piece):
    # of a function or of a kernel's metadata record; None for what stands in front of a unit's first function / record
    m = re.search(r"\t\.(?:protected|globl|weak)\t(\S+)|^    \.name: +(\S+)", piece, re.M)
    return m and (m.group(1) or m.group(2))


def moved(old, news):
    def split(t):
        p = [PAD.sub("", x) for x in pieces(t)]
        i = p.index("<metadata>")
        return [x for x in p[:i - 1] + p[i + 1:-1] if symbol(x)]      # functions and records, without trailer and tail
    po, pn = split(old), [x for t in news for x in split(t)]
    twice = sorted({symbol(x) for x in pn if pn.count(x) > 1})
    lost = sorted({symbol(x) for x in po if x not in pn})
    added = sorted({symbol(x) for x in pn if x not in po})
    return twice, lost, added, len(po), len(pn), sha("".join(sorted(pn)))


def sha(s):
    return hashlib.sha256(s.encode()).hexdigest()


if __name__ == "__main__":
    if sys.argv[1] == "--subset":
        missing, added, h = subset(load(sys.argv[2]), load(sys.argv[3]))
        if missing:
            print("DIFFERENT", f"{len(missing)} pieces of the old unit are not in the new one")
            sys.exit(1)
        print("subset   ", h, f"(every old function and metadata record is in the new unit; {len(added)} functions added)")
        for name in added:
            print("  added:", name)
        sys.exit(0)
    if sys.argv[1] == "--moved":
        args = sys.argv[2:]
        files, gone = (args[:args.index("--gone")], args[args.index("--gone") + 1:]) if "--gone" in args else (args, [])
        twice, lost, added, n_old, n_new, h = moved(load(files[0]), [load(f) for f in files[1:]])
        # a symbol that differs shows up as lost AND added; one that disappeared as lost only
        if twice or added or lost != sorted(gone):
            print("DIFFERENT", f"in two units: {twice}; differ or added: {added}; not in the new units: {lost}; expected to go: {sorted(gone)}")
            sys.exit(1)
        print("moved    ", h, f"({n_new} of the old unit's {n_old} functions and metadata records, each in one of {len(files) - 1} units; "
              f"{len(lost)} symbols gone, none added)")
        for name in lost:
            print("  gone:", name)
        sys.exit(0)
    a, b = load(sys.argv[1]), load(sys.argv[2])
    if a == b:
        print("identical", sha(a))
        sys.exit(0)
    pa, pb = pieces(a), pieces(b)
    if pa == pb:
        print("same-set ", sha("".join(pa)), f"({len(pa)} pieces; order differs)")
        sys.exit(0)
    print("DIFFERENT", sha(a), sha(b), f"{len(set(pa) ^ set(pb))} pieces differ")
    sys.exit(1)
