"""Says whether two `hipcc -S` listings of mse_lib.hip hold the same device code (the command is in check_step_loops.py):

    python tools/same_isa.py OLD.s NEW.s

For every kernel, matched by its mangled name, it compares the instruction lines (comments and assembler directives
stripped, labels kept - but without the function's ordinal in the listing, which the compiler writes into every local
label (.LBB17_4, .LJTI17_0): a kernel added in front of others shifts that number and nothing else; likewise the listing-wide
count in a long branch's .Lpost_getpc<n>, renumbered per kernel by first appearance) and the kernel's
metadata: VGPR / AGPR / SGPR counts, spill counts, private and group segment sizes.  It prints one summary line
and, for each kernel that differs, its name and both instruction counts.  Exit status 1 on any difference, a kernel
present in only one listing included.  A refactor of the device code is checked with this instead of a timing run."""
import re
import sys

META = (".agpr_count", ".vgpr_count", ".sgpr_count", ".sgpr_spill_count", ".vgpr_spill_count",
        ".private_segment_fixed_size", ".group_segment_fixed_size")


ORDINAL = re.compile(r"\.L([A-Za-z_]+?)\d+_(\d+)")  # .LBB<function ordinal>_<block> -> .LBB_<block>
# .Lpost_getpc<n>, the label of a long branch's s_getpc_b64: n counts the long branches of the whole listing, so a kernel
# added in front shifts it like the ordinal.  Within a kernel the labels are renumbered by first appearance, so which label
# an instruction names is still compared.
LONG_BRANCH = re.compile(r"\.Lpost_getpc(\d+)")


def renumber_long_branches(text):
    seen = {}
    return [LONG_BRANCH.sub(lambda m: ".Lpost_getpc#%d" % seen.setdefault(m.group(1), len(seen)), t) for t in text]


def kernels(path):
    lines = open(path).read().split("\n")
    # the metadata: one YAML entry per kernel under amdhsa.kernels, keys at four columns
    meta, entry = {}, None
    for l in lines[lines.index("amdhsa.kernels:") + 1:]:
        if l.startswith("  - "):
            entry = {}
        elif not l.startswith("    "):
            break
        m = re.match(r"(?:  - |    )(\.\w+):\s*(\S+)\s*$", l)
        if m and m.group(1) in META:
            entry[m.group(1)] = m.group(2)
        elif m and m.group(1) == ".name":
            meta[m.group(2)] = entry
    # the text: from the kernel's symbol to the end of the function
    out = {}
    for i, l in enumerate(lines):
        name = l.split(":")[0]
        if name in meta and l.startswith(name + ":"):
            end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
            text = [ORDINAL.sub(r".L\1_\2", t) for t in (b.split(";")[0].strip() for b in lines[i + 1:end])
                    if t and (t[0] != "." or t.endswith(":"))]
            out[name] = (renumber_long_branches(text), tuple(meta[name].get(k) for k in META))
    return out


old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
differ = sorted(k for k in old.keys() & new.keys() if old[k] != new[k])
only = sorted(old.keys() ^ new.keys())
print(f"same_isa: {len(old)} kernels in {sys.argv[1]}, {len(new)} in {sys.argv[2]}: "
      f"{len(old.keys() & new.keys()) - len(differ)} identical, {len(differ)} differ, {len(only)} in one listing only")
for k in differ:
    note = "" if old[k][1] == new[k][1] else f"  metadata {dict(zip(META, old[k][1]))} -> {dict(zip(META, new[k][1]))}"
    n_old, n_new = (sum(1 for t in v[k][0] if not t.endswith(":")) for v in (old, new))
    print(f"  differs: {k}: {n_old} -> {n_new} instructions{note}")
for k in only:
    print(f"  only in {sys.argv[1] if k in old else sys.argv[2]}: {k}")
sys.exit(1 if differ or only else 0)
