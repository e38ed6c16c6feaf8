"""Per-kernel comparison of the gfx950 code in two object files (e.g. csrc/x.o before and after an edit that must not touch
the existing kernels): extracts the device code object of each (llvm-objdump --offloading), disassembles it and compares
the instruction streams kernel by kernel.

    python scripts/isa_diff.py /tmp/gemm_bf16.o.before kan-tts_amd/csrc/gemm_bf16.o

Kernels are matched by symbol.  When the edit renamed them (a template parameter was added), give one or more
``--rename REGEX REPLACEMENT``: the symbols of BOTH files are demangled, their parameter lists dropped, and every rename is
applied to the names of the second file before matching:

    python scripts/isa_diff.py /tmp/sconv.o.before kan-tts_amd/csrc/sconv.o --rename ', false>$' '>' --rename '<false>$' ''
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

BIN = "/opt/rocm/lib/llvm/bin"


def kernels(obj):
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(obj, os.path.join(d, "o.o"))
        subprocess.run([os.path.join(BIN, "llvm-objdump"), "--offloading", "o.o"], cwd=d, capture_output=True, check=True)
        dev = [f for f in os.listdir(d) if "amdgcn" in f]
        if not dev:
            raise SystemExit("no device code object in " + obj)
        text = subprocess.run([os.path.join(BIN, "llvm-objdump"), "-d", os.path.join(d, dev[0])], capture_output=True, text=True,
                              check=True).stdout
    out, cur = {}, None
    for ln in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln.strip())
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur is not None and "\t" in ln and ln.strip() != "...":  # "..." = padding between functions
            out[cur].append(ln.split("//")[0].strip())
    for ins in out.values():  # s_nop behind the last s_endpgm: alignment padding up to the next function or the section's end
        while len(ins) > 1 and ins[-1].split(":")[-1].split() == ["s_nop", "0"]:
            ins.pop()
    return out


def demangled(ks, renames):
    names = subprocess.run(["c++filt"], input="\n".join(ks), capture_output=True, text=True, check=True).stdout.splitlines()
    out = {}
    for k, n in zip(ks, names):
        n = re.sub(r"^void ", "", re.sub(r"\(.*", "", n))
        for pat, repl in renames:
            n = re.sub(pat, repl, n)
        out[n] = ks[k]
    return out


def main(a_path, b_path, renames=None):
    a, b = kernels(a_path), kernels(b_path)
    if renames is not None:
        a, b = demangled(a, []), demangled(b, renames)
    same = True
    for k in sorted(set(a) | set(b)):
        if k not in b:
            print("removed   %s" % k)
            same = False
        elif k not in a:
            print("new       %-90s %5d instructions" % (k[:90], len(b[k])))
        elif a[k] != b[k]:
            print("CHANGED   %-90s %5d -> %5d instructions" % (k[:90], len(a[k]), len(b[k])))
            same = False
        else:
            print("identical %-90s %5d instructions" % (k[:90], len(a[k])))
    return 0 if same else 1


if __name__ == "__main__":
    argv, ren = sys.argv[1:], []
    while "--rename" in argv:
        i = argv.index("--rename")
        ren.append((argv[i + 1], argv[i + 2]))
        del argv[i:i + 3]
    sys.exit(main(argv[0], argv[1], ren or None))
