#!/usr/bin/env python3
"""Assert that a change left existing GPU kernels instruction-for-instruction identical.

Emits the gfx950 device assembly of the given sources twice -- from a base revision (git archive, default HEAD) and from
the working tree -- with the Makefile's flags (hipcc ... --cuda-device-only -S), and compares every function of the base
build with its counterpart in the new one: the instruction stream (comments dropped, local labels renumbered in order of
appearance) and the kernel descriptor (.amdhsa_* lines: registers, LDS, scratch).

Counterparts are found by demangled name.  A change that adds an element-type template parameter (the c8 kernels'
C8H / C8B traits, theanet_amd/csrc/c8_elem.h) renames every kernel; --drop-arg C8H (the default) removes that argument
from the new names, so `c8_conv_kernel<C8H, 2, 1, 4, true, false>` maps onto the base's `c8_conv_kernel<2, 1, 4, true,
false>` and a formerly plain kernel `c8_pack_kernel<C8H>(...)` onto `c8_pack_kernel(...)`.  New functions without a
base counterpart (the other element type's instantiations) are counted, not compared.

    python tools/isa_diff.py                       # conv_c8.hip fc_c8.hip elastic.hip against HEAD
    python tools/isa_diff.py --base main~1 conv_c8.hip

Exit status 0: every base function found and identical; 1 otherwise.  Needs only hipcc (no GPU)."""
import argparse
import concurrent.futures as cf
import os
import re
import shlex
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "theanet_amd/csrc"
DEFAULT_FILES = ["conv_c8.hip", "fc_c8.hip", "elastic.hip"]


def makefile_flags():
    """HIPCC and CXXFLAGS of theanet_amd/csrc/Makefile (ARCH substituted): the flags the library is built with."""
    text = open(os.path.join(ROOT, CSRC, "Makefile")).read()
    var = dict(re.findall(r"^(\w+)\s*\??=\s*(.*)$", text, re.M))
    flags = var["CXXFLAGS"].replace("$(ARCH)", var.get("ARCH", "gfx950"))
    return var.get("HIPCC", "/opt/rocm/bin/hipcc"), shlex.split(flags)


def emit_asm(hipcc, flags, src, out):
    cmd = [hipcc] + flags + ["--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, cwd=os.path.dirname(src), capture_output=True, text=True)
    if r.returncode:
        sys.exit("isa_diff: %s failed:\n%s" % (" ".join(cmd), r.stderr[-4000:]))
    return out


def demangle(names):
    # (binutils' c++filt does not know _Float16's mangling DF16_: it is spelled as the equivalent `half`, Dh, and a new
    # name's C8H::T -- _Float16 -- as `half` too, see normalize)
    names = [n.replace("DF16_", "Dh") for n in names]
    rocm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-cxxfilt")
    tool = rocm if os.path.exists(rocm) else shutil.which("llvm-cxxfilt") or "c++filt"
    r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True)
    return r.stdout.splitlines()


def parse(path):
    """{mangled function name: (instruction lines, descriptor lines)} of one device assembly file."""
    lines = open(path).read().splitlines()
    funcs = set(re.findall(r"^\s*\.type\s+([\w.$]+),@function", "\n".join(lines), re.M))
    body, desc = {}, {}
    cur = None
    kern = None
    for ln in lines:
        s = ln.split(";", 1)[0].rstrip()
        st = s.strip()
        m = re.match(r"^([\w.$]+):$", st)
        if m and m.group(1) in funcs:
            cur = m.group(1)
            body[cur] = []
            continue
        if cur is not None and re.match(r"^\.Lfunc_end\d+:$", st):
            cur = None
            continue
        m = re.match(r"^\.amdhsa_kernel\s+([\w.$]+)$", st)
        if m:
            kern = m.group(1)
            desc[kern] = []
            continue
        if st == ".end_amdhsa_kernel":
            kern = None
            continue
        if kern is not None and st:
            desc[kern].append(" ".join(st.split()))
        if cur is not None and st and not st.startswith("."):
            body[cur].append(" ".join(st.split()))
        elif cur is not None and re.match(r"^\.LBB\d+_\d+:$", st):
            body[cur].append(st)
    out = {}
    for f, ins in body.items():
        labels = {}
        norm = []
        for i in ins:
            for lab in re.findall(r"\.LBB\d+_\d+", i):
                labels.setdefault(lab, "L%d" % len(labels))
            norm.append(re.sub(r"\.LBB\d+_\d+", lambda m: labels[m.group(0)], i))
        out[f] = (norm, desc.get(f, []))
    return out


def normalize(name, drop):
    """Demangled name -> comparison key: the dropped template argument removed, a template's leading return type too."""
    name = name.replace("C8H::T", "half")
    for a in drop:
        name = re.sub(r"<%s>" % re.escape(a), "", name)
        name = re.sub(r"<%s,\s*" % re.escape(a), "<", name)
        name = re.sub(r",\s*%s(?=[,>])" % re.escape(a), "", name)
    return re.sub(r"^void\s+", "", name)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("files", nargs="*", default=DEFAULT_FILES, help="sources under %s (default: %s)" % (CSRC, " ".join(DEFAULT_FILES)))
    ap.add_argument("--base", default="HEAD", help="git revision of the 'before' build (default HEAD)")
    ap.add_argument("--drop-arg", action="append", default=None, help="template argument to drop from new names (default C8H)")
    ap.add_argument("-j", type=int, default=8, help="parallel compilations")
    ap.add_argument("--keep", help="copy the emitted assembly (<file>.old.s / <file>.new.s) into this directory")
    a = ap.parse_args()
    drop = a.drop_arg or ["C8H"]
    hipcc, flags = makefile_flags()
    with tempfile.TemporaryDirectory(prefix="isa_diff_") as tmp:
        base = os.path.join(tmp, "base")
        os.makedirs(base)
        arc = subprocess.run(["git", "-C", ROOT, "archive", a.base, CSRC, "include"], capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", base], input=arc, check=True)
        jobs = {}
        with cf.ThreadPoolExecutor(a.j) as ex:
            for f in a.files:
                for side, root in (("old", base), ("new", ROOT)):
                    jobs[(f, side)] = ex.submit(emit_asm, hipcc, flags, os.path.join(root, CSRC, f),
                                                os.path.join(tmp, "%s.%s.s" % (f, side)))
            paths = {k: v.result() for k, v in jobs.items()}
        if a.keep:
            os.makedirs(a.keep, exist_ok=True)
            for p in paths.values():
                shutil.copy(p, a.keep)
        bad = 0
        for f in a.files:
            old, new = parse(paths[(f, "old")]), parse(paths[(f, "new")])
            onames, nnames = sorted(old), sorted(new)
            okeys = dict(zip(onames, (normalize(n, []) for n in demangle(onames))))
            nkeys = {}
            for m, d in zip(nnames, demangle(nnames)):
                nkeys.setdefault(normalize(d, drop), m)
            same = 0
            matched = set()
            for o in onames:
                n = nkeys.get(okeys[o])
                if n is None:
                    print("%s: MISSING  %s" % (f, okeys[o]))
                    bad += 1
                    continue
                matched.add(n)
                if old[o] != new[n]:
                    oi, ni = old[o][0], new[n][0]
                    k = next((i for i in range(min(len(oi), len(ni))) if oi[i] != ni[i]), min(len(oi), len(ni)))
                    what = "instructions" if oi != ni else "descriptor"
                    print("%s: DIFFERS  %s (%s; %d vs %d instructions, first difference at %d)"
                          % (f, okeys[o], what, len(oi), len(ni), k))
                    bad += 1
                else:
                    same += 1
            ninstr = sum(len(old[o][0]) for o in onames)
            print("%s: %d of %d pre-existing functions identical (%d instructions); %d new functions"
                  % (f, same, len(onames), ninstr, len(set(nnames) - matched)))
    print("isa_diff: %s" % ("OK -- every pre-existing function is identical" if not bad else "%d function(s) differ or are missing" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
