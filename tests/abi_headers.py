"""The entry points the two C headers declare (include/rvcx.h, include/rvcx_test.h), parsed for the ABI tests."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def header_prototypes(name):
    """{entry point: number of parameters} of include/<name>: comments stripped, then every `int` / `const char*`
    function named rvcx_*, its parameters counted by the top-level commas of the parameter list."""
    src = re.sub(r"/\*.*?\*/", " ", open(os.path.join(REPO, "include", name)).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"^\s*(?:int|const char\*)\s+(rvcx_[a-z0-9_]+)\s*\(([^;{}]*)\)\s*;", src, re.M):
        params, depth, commas = m.group(2).strip(), 0, 0
        for ch in params:
            depth += ch in "(["
            depth -= ch in ")]"
            commas += ch == "," and depth == 0
        assert m.group(1) not in protos, f"{m.group(1)} declared twice in {name}"
        protos[m.group(1)] = 0 if params in ("", "void") else commas + 1
    return protos
