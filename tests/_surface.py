"""The surface of include/rt_tile.h as data, for tests/test_surface.py and the per-feature test_*_surface.py files: the header's text, a
parser of its prototypes, structs and constants, the C compiler's view of the layouts, the symbols a library exports, and the
fixture tests/golden/abi4_surface.json that pins all of it.  `python tests/_surface.py` rewrites the fixture from the header."""
import json
import re
import shutil
import subprocess
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
INCLUDE = ROOT / "include"
HEADER = (INCLUDE / "rt_tile.h").read_text()
FIXTURE = ROOT / "tests" / "golden" / "abi4_surface.json"


def _value(expr, constants):
    """An integer constant expression of the header: literals with a `u` suffix, `-`, `<<`, or the name of an earlier constant."""
    expr = expr.strip()
    if expr in constants:
        return constants[expr]
    assert re.fullmatch(r"[-0-9a-fA-FxXu<\s]+", expr), expr
    return eval(re.sub(r"(?<=[0-9a-fA-F])u\b", "", expr))


def _type(text):
    """A C type as the tables spell it: single spaces, every `*` attached to what precedes it."""
    return re.sub(r"\s*\*", "*", " ".join(text.split()))


def parse(text=HEADER):
    """{"functions": {name: [return type, [parameter types]]}, "structs": {name: [[type, field, array length or None]]},
    "constants": {name: value}} of a header, every RT_API prototype, struct with a body, integer #define and enumerator of it."""
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    constants = {}
    for m in re.finditer(r"#define\s+(RT_\w+)[ \t]+(\S+)[ \t]*$|\benum\s*\w*\s*\{([^}]*)\}", text, re.M):
        if m.group(3) is not None:
            for item in m.group(3).split(","):
                name, expr = item.split("=")
                constants[name.strip()] = _value(expr, constants)
        elif re.fullmatch(r"(0[xX][0-9a-fA-F]+|\d+)u?", m.group(2)):
            constants[m.group(1)] = _value(m.group(2), constants)
    functions = {}
    for ret, name, params in re.findall(r"RT_API\s+([\w\s\*]+?)\s*\b(rt_\w+)\s*\(([^)]*)\)\s*;", text):
        params = [] if params.strip() == "void" else [_type(re.sub(r"\b\w+\s*$", "", p)) for p in params.split(",")]
        functions[name] = [_type(ret), params]
    structs = {}
    for name, body in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", text, re.S):
        fields = []
        for decl in filter(None, (_type(d) for d in body.split(";"))):
            first, *rest = decl.split(",")
            typ, first = first.rsplit(" ", 1)
            for field in [first] + rest:
                m = re.fullmatch(r"\s*(\w+)(?:\[(\w+)\])?\s*", field)
                fields.append([typ, m.group(1), _value(m.group(2), constants) if m.group(2) else None])
        structs[name] = fields
    return {"functions": functions, "structs": structs, "constants": constants}


def compile_c(src, std="c11", extra=("-fsyntax-only",)):
    """Compile a C translation unit against include/ with -Wall -Werror; returns the finished process (returncode, stderr)."""
    gcc = shutil.which("gcc")
    assert gcc
    return subprocess.run([gcc, f"-std={std}", "-Wall", "-Werror", *extra, f"-I{INCLUDE}", "-x", "c", "-"], input=src,
                          capture_output=True, text=True)


def c_layouts(structs):
    """{struct: {"size": sizeof, "offsets": {field: offsetof}}} as the C compiler reports them for the header on disk."""
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "rt_tile.h"', "int main(void) {"]
    for name, fields in structs.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for _, f, _ in fields]
    with tempfile.TemporaryDirectory() as tmp:
        exe = Path(tmp) / "layouts"
        r = compile_c("\n".join(lines + ["return 0; }"]), extra=("-o", str(exe)))
        assert r.returncode == 0, r.stderr
        out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    layouts = {name: {"size": None, "offsets": {}} for name in structs}
    for what, value in (ln.split() for ln in out.splitlines()):
        name, _, field = what.partition(".")
        if field:
            layouts[name]["offsets"][field] = int(value)
        else:
            layouts[name]["size"] = int(value)
    return layouts


def surface():
    """parse() of the header on disk plus "layouts": what abi4_surface.json holds."""
    s = parse()
    s["layouts"] = c_layouts(s["structs"])
    return s


def write_json(path=FIXTURE):
    Path(path).write_text(json.dumps(surface(), indent=1) + "\n")


def all_exported(path):
    """Every symbol a shared library defines (`nm -D`)."""
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.split()}


def exported(path):
    """The rt_* symbols a shared library defines."""
    return {s for s in all_exported(path) if s.startswith("rt_")}


def check_abi_version_unchanged():
    """What every feature's surface file asserts of the ABI it was added to: RT_ABI_VERSION is 4 in the header, the binding and the
    loaded library."""
    from ray_tracer_s8_amd import _abi
    assert re.search(r"#define\s+RT_ABI_VERSION\s+4u", HEADER)
    assert _abi.RT_ABI_VERSION == 4 and _abi.load().rt_abi_version() == 4


def check_exports(names, debug=True, exactly=False):
    """A feature's entry points are exported by the product library (and, with debug, by the test library); with exactly, the
    product library still exports exactly what the header declares."""
    from ray_tracer_s8_amd import _abi, build
    _abi.load()
    paths = [build.LIB_PATH]
    if debug:
        _abi.load_debug()
        paths.append(build.DEBUG_LIB_PATH)
    for path in paths:
        assert set(names) <= exported(path), (path, set(names) - exported(path))
    if exactly:
        declared = set(parse()["functions"])
        assert exported(build.LIB_PATH) == declared, exported(build.LIB_PATH) ^ declared


if __name__ == "__main__":
    write_json()
