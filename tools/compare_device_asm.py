"""Compare the gfx950 device assembly of one translation unit at two commits, kernel by kernel.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -S --cuda-device-only squidpy_amd/csrc/<unit>.hip -o <commit>.s
    python tools/compare_device_asm.py before.s after.s

The flags are those of ``squidpy_amd/_build.py``.  Per symbol of type ``@function`` the body (label to ``.Lfunc_end``) and, for a kernel,
its ``.amdhsa_kernel`` block (registers, LDS, scratch) are compared line for line.  Normalised, and nothing else: the hash of an
anonymous namespace in a mangled name; the function's ordinal in local labels (``.LBB<k>_<j>``, ``.Lfunc_end<k>``, also where a loop
comment quotes them), which follows the order in which the kernels are emitted; the column a trailing comment starts in, which follows
the label's width.  Exit status 1 if a symbol differs or exists on one side only.  No device is needed."""
import re
import shutil
import subprocess
import sys


def functions(path: str) -> dict:
    with open(path) as fh:
        text = fh.read()
    text = re.sub(r"_GLOBAL__N__[0-9a-f]+_[A-Za-z0-9_]*?_(hip|cu)_[0-9a-f]+", "_GLOBAL__N__X", text)
    text = re.sub(r"\.anon\.[0-9a-f]+", ".anon.X", text)
    out = {}
    for m in re.finditer(r"^\t\.type\t(\S+),@function\n(.*?)^\.Lfunc_end\d+:\n", text, re.S | re.M):
        body = re.sub(r"\.Lfunc_end\d+|BB\d+_|\.Lfunc_begin\d+", lambda x: re.sub(r"\d+", "N", x.group(0), 1), m.group(2))
        out.setdefault(m.group(1), []).append(re.sub(r"[ \t]+;", " ;", body))
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel\n", text, re.S | re.M):
        out.setdefault(m.group(1), []).append(m.group(2))
    return out


def demangled(names: list) -> dict:
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool:
        return {n: n for n in names}
    return dict(zip(names, subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()))


def main() -> int:
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    names = sorted(set(a) | set(b))
    plain, bad = demangled(names), 0
    for name in names:
        if name not in a or name not in b:
            verdict = "only " + ("before" if name in a else "after")
        elif a[name] == b[name]:
            verdict = f"identical ({sum(s.count(chr(10)) for s in a[name])} lines)"
        else:
            verdict = "DIFFERENT"
        bad += not verdict.startswith("identical")
        print(f"{verdict:24s} {plain[name][:160]}")
    print(f"{len(names)} kernels and device functions compared, {bad} not identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
