#!/usr/bin/env python3
"""Compare the device code of two builds of the library's HIP units kernel by kernel (runs without a GPU).

Each side is one assembly file or several, comma-separated: one per HIP source of build.SOURCES, made with the FLAGS of
build.py minus -shared -fPIC:

    for src in $(python -c "import sys; sys.path.insert(0, '<tree>/wgpu-3dgs-core_amd'); import build; \
                            print(' '.join(s for s in build.SOURCES if s.endswith('.hip')))"); do
        hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Wall -Wno-unused-function -S --cuda-device-only \
              -o <out>/$(basename $src .hip).s $src
    done
    python tools/compare_device_code.py A1.s,A2.s B1.s,B2.s

A side is the union of its files; a kernel that two files of one side define is an error (every kernel belongs to one
unit).  Kernels are matched by DEMANGLED name, with an empty template argument list dropped (a kernel that gained a parameter
pack which is empty in its old instantiations keeps its demangled name but not its mangled one); instruction streams are
compared after local labels and the kernels' own mangled names have been normalised.  Prints the kernels only in one
side, the kernels that differ, and the count of identical ones; exit status 1 if a kernel of A is missing from B or
differs, or a side defines a kernel twice.
"""
import re
import subprocess
import sys


def kernels(path):
    text = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    out = {}
    for name in names:
        start = text.index("\n", text.index("\n%s:" % name) + 1)
        body = text[start:re.compile(r"^\.Lfunc_end\d+:", re.M).search(text, start).start()]
        lines = []
        for ln in body.splitlines():
            ln = ln.split(";")[0].rstrip()
            if not ln.strip():
                continue
            lines.append(ln)
        body = "\n".join(lines).replace(name, "<self>")
        # local labels are numbered over the whole file: renumber them per kernel
        labels = {}
        body = re.sub(r"\.L[A-Za-z_]*\d+(?:_\d+)?", lambda mm: labels.setdefault(mm.group(0), ".L%d" % len(labels)), body)
        out[name] = body
    dem = subprocess.run(["c++filt"], input="\n".join(out), stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    res = {}
    for (name, body), d in zip(out.items(), dem):
        d = re.sub(r"^void (?=[\w:]+<>\()", "", d)      # (a template's mangled name carries its return type)
        d = re.sub(r"<>(?=\()", "", d)
        assert d not in res, d
        res[d] = body
    return res


def side(arg):
    """Union of the kernels of the comma-separated files, and the names that more than one of them defines."""
    res, twice = {}, []
    for path in arg.split(","):
        for name, body in kernels(path).items():
            if name in res:
                twice.append(name)
            res[name] = body
    return res, twice


def main():
    (a, dup_a), (b, dup_b) = side(sys.argv[1]), side(sys.argv[2])
    for title, lst in (("twice in A", dup_a), ("twice in B", dup_b)):
        print("%s: %d" % (title, len(lst)))
        for k in lst:
            print("   ", k[:200])
    only_a = sorted(set(a) - set(b))
    only_b = sorted(set(b) - set(a))
    differ = sorted(k for k in a if k in b and a[k] != b[k])
    for title, lst in (("only in A", only_a), ("only in B", only_b), ("differ", differ)):
        print("%s: %d" % (title, len(lst)))
        for k in lst:
            print("   ", k[:200])
    print("kernels: A %d, B %d, identical %d" % (len(a), len(b), sum(1 for k in a if k in b and a[k] == b[k])))
    sys.exit(1 if only_a or differ or dup_a or dup_b else 0)


if __name__ == "__main__":
    main()
