#!/usr/bin/env python3
"""Compare device assembly kernel by kernel: BASE.s against one or more NEW.s taken together (a source that was split).

    hipcc <the project's flags> --cuda-device-only -S csrc/x.hip -o x.s      # per source and commit, then
    tools/compare_device_asm.py base/x.s new/x.s new/y.s

Per kernel of either side one line: identical, DIFFERENT, MISSING (not in NEW), NEW (not in BASE) or DUPLICATE (in two NEW
files), with the resource directives of its descriptor (VGPRs, SGPRs, scratch and static LDS bytes; BASE -> NEW where they
differ).  A kernel is identical when its instructions, with local labels renumbered, and all its .amdhsa_ directives are equal.
Kernels are matched by demangled name without "(anonymous namespace)::", so a parameter type that moved into or out of an
anonymous namespace (which changes the mangled name and nothing else) does not hide a kernel.  Exit status 1 unless all match.
"""
import re
import subprocess
import sys

SHOWN = (("vgpr", "next_free_vgpr"), ("sgpr", "next_free_sgpr"), ("scratch", "private_segment_fixed_size"),
         ("lds", "group_segment_fixed_size"))


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    except (OSError, subprocess.CalledProcessError):
        out = names  # no demangler: the mangled names are the keys
    return {m: d.replace("(anonymous namespace)::", "") for m, d in zip(names, out)}


def kernels(path):
    """{mangled name: (normalised instruction lines, {directive: value})} of one assembly file."""
    lines = open(path).read().split("\n")
    found = {}
    for at, line in enumerate(lines):
        m = re.match(r"\s+\.amdhsa_kernel (\S+)", line)
        if not m:
            continue
        name = m.group(1)
        start = next(i for i in range(at, -1, -1) if lines[i].startswith(name + ":"))  # the descriptor follows its function
        body = []
        for text in lines[start + 1:at]:
            if text.lstrip().startswith(".section"):
                break
            # local labels carry the function's number in the file: .LBB12_3, and BB12_3 in the loop comments
            text = re.sub(r"(\.L[A-Za-z_]+?|\bBB)\d+(_\d+)?\b", r"\1\2", text.replace(name, "<kernel>"))
            body.append(" ".join(text.split()))  # a comment's column moves with the width of its label's number
        directives = {}
        for text in lines[at + 1:]:
            if ".end_amdhsa_kernel" in text:
                break
            key, _, value = text.strip().partition(" ")
            directives[key.replace(".amdhsa_", "")] = value
        found[name] = (body, directives)
    return found


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    base, new, twice = kernels(argv[1]), {}, set()
    for path in argv[2:]:
        for name, k in kernels(path).items():
            if name in new:
                twice.add(name)
            new[name] = k
    names = demangle(sorted(set(base) | set(new)))
    base = {names[n]: k for n, k in base.items()}
    twice = {names[n] for n in twice}
    new = {names[n]: k for n, k in new.items()}
    tally = {}
    for key in sorted(set(base) | set(new)):
        b, n = base.get(key), new.get(key)
        status = ("DUPLICATE" if key in twice else "MISSING" if n is None else "NEW" if b is None else
                  "identical" if b == n else "DIFFERENT")
        tally[status] = tally.get(status, 0) + 1
        one = (b or n)[1]
        shown = " ".join(f"{label}={one.get(d)}" + (f"->{n[1].get(d)}" if b and n and b[1].get(d) != n[1].get(d) else "")
                         for label, d in SHOWN)
        print(f"{status:9s} {shown:44s} {key}")
    print(f"# {len(base)} kernels in {argv[1]}, {len(new)} in {', '.join(argv[2:])}: " +
          ", ".join(f"{v} {k}" for k, v in sorted(tally.items())))
    return 0 if set(tally) <= {"identical"} else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
