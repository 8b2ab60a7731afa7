#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds by their device assembly.  CPU only, nothing but Python.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC --cuda-device-only -S csrc/<unit>.hip -o <dir>/<unit>.s    (every unit, both trees)
    python tools/compare_isa.py <dir before> <dir after> [> profiles/<name>.txt]

A kernel is found by its name in whichever file holds it.  Its instruction text is compared with comments stripped and local labels
renumbered in order of appearance; --drop-arg lists mangled-name fragments (default: the `Li0E` that a removed trailing `int = 0`
template parameter leaves behind in assign_kernel / aggregate_kernel) that may vanish from a name.  One line per kernel, what differs first (a name beyond 120 characters is abbreviated): name, file
before -> after, identical | differs (with the instruction counts), and next_free_vgpr / next_free_sgpr / accum_offset /
private_segment_fixed_size / group_segment_fixed_size.  No assembly text is printed.  Exit status 1 when a kernel differs in text,
2 when one moved in a resource or exists on one side only."""
import glob
import os
import re
import sys

RES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size")
LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def canon(name, drop):
    for frag in drop:
        name = re.sub(r"^(_Z\d+(?:assign|aggregate)_kernelIL[ib]\d+E)" + frag, r"\1", name)
    return name


def kernels(directory, drop):
    """{canonical kernel name: (file, [instruction lines], {resource: value})}"""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        lines = open(path).read().split("\n")
        names = [m.group(1) for ln in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln))]
        for name in names:
            start = next(j for j, ln in enumerate(lines) if ln.split(";")[0].strip() == name + ":")
            body, res, labels, in_desc = [], {}, {}, False
            for ln in lines[start + 1:]:
                if ln.startswith(".Lfunc_end"):
                    break
                ln = ln.split(";")[0].strip()
                if ln.startswith(".amdhsa_kernel"):
                    in_desc = True
                elif ln.startswith(".end_amdhsa_kernel"):
                    in_desc = False
                elif in_desc:
                    key, _, val = ln.partition(" ")
                    if key[len(".amdhsa_"):] in RES:
                        res[key[len(".amdhsa_"):]] = val.strip()
                elif ln and not re.match(r"\.(section|text|p2align)\b", ln):
                    ln = LABEL.sub(lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), ln)
                    body.append(re.sub(r"\s+", " ", ln.replace(name, canon(name, drop))))
            out[canon(name, drop)] = (os.path.basename(path), body, res)
    return out


def main(argv):
    drop = ["Li0E"]
    args = [a for a in argv if not a.startswith("--drop-arg=")]
    drop += [a.split("=", 1)[1] for a in argv if a.startswith("--drop-arg=")]
    if len(args) != 2:
        sys.exit(__doc__)
    before, after = kernels(args[0], drop), kernels(args[1], drop)
    status = 0
    n_same = 0
    differs = lambda n: n not in before or n not in after or before[n][1:] != after[n][1:]
    short = lambda n: n if len(n) <= 120 else "%s...(%d characters)...%s" % (n[:80], len(n), n[-24:])   # (library templates)
    for name in sorted(set(before) | set(after), key=lambda n: (not differs(n), n)):   # what differs comes first
        if name not in before or name not in after:
            print("%s  %s  ONLY %s" % (short(name), (before.get(name) or after.get(name))[0], "before" if name in before else "after"))
            status = 2
            continue
        (fb, tb, rb), (fa, ta, ra) = before[name], after[name]
        same = tb == ta
        n_same += same
        count = lambda text: sum(not ln.endswith(":") for ln in text)   # (labels are part of the text, not of the count)
        verdict = "identical" if same else "differs (%d -> %d instructions)" % (count(tb), count(ta))
        res = " ".join("%s=%s" % (k, rb.get(k)) if rb.get(k) == ra.get(k) else "%s=%s->%s MOVED" % (k, rb.get(k), ra.get(k)) for k in RES)
        print("%s  %s -> %s  %s  %s" % (short(name), fb, fa, verdict, res))
        if rb != ra:
            status = 2
        elif not same:
            status = max(status, 1)
    print("# %d kernels before, %d after, %d identical" % (len(before), len(after), n_same))
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
