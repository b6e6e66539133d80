"""How the tests compile their C and C++ helpers: the reference libraries behind the tests/*_ref.py wrappers and the probes that
print a struct's layout.  No project imports: every wrapper and test module can take this one first."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_LIB = {}


def compile_ref(tmpdir, name, declare, include_oracle=False, defines=()):
    """tests/<name>.c as lib<name>.so in tmpdir (gcc -O2 -ffp-contract=off; include_oracle: -I oracle; defines: names for -D, which
    become a part of the output's name), loaded and handed to declare(lib) for its argtypes / restype once; cached by output path."""
    out = os.path.join(str(tmpdir), "lib" + "-".join([name, *defines]) + ".so")
    if out not in _LIB:
        include = ["-I", os.path.join(ROOT, "oracle")] if include_oracle else []
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", *include, *["-D" + d for d in defines], os.path.join(HERE, name + ".c"), "-o", out,
                               "-lm"])
        lib = C.CDLL(out)
        declare(lib)
        _LIB[out] = lib
    return _LIB[out]


def layout_probe(tmp_path, prints):
    """{label: printed value} of a g++-compiled probe (-std=c++17 -I csrc) that includes ShaderInterop.h and prints every
    (label, size_t expression) of prints, such as ("size", "sizeof(interop::BloomConsts)")."""
    lines = ['#include <cstdio>', '#include "ShaderInterop.h"', "int main() {"]
    lines += [f'    printf("{label} %zu\\n", {expr});' for label, expr in prints]
    lines += ["    return 0;", "}"]
    src = tmp_path / "probe.cpp"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "toyrenderer_amd", "csrc"), str(src), "-o", str(exe)])
    return dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
