"""Build re-tuned copies of the library: the one recipe for an edited mgmc_tuning.hpp.

A variant is a copy of the product sources (build/exp_<name>/) whose mgmc_tuning.hpp has some constants replaced,
compiled by the product's own Makefile, so with the product's flags (-O3 -ffp-contract=off).  The copy is refreshed
file by file and only where the contents differ, and a digest of its inputs is kept beside the library, so a call
that finds nothing changed compiles nothing -- and a library older than the sources is never used.  The variants
build side by side and share at most 16 make jobs.

  * the variants of tests/tuning_variants.py -> build/libmgmc_tune_<name>.so: __graft_entry__.build(), the tuning
    tests (tests/test_gpu_tuning.py, tests/test_tuning_host.py), or
        python scripts/build_tuning_variants.py [name ...]
  * timing experiments (scripts/build_exp.sh) -> build/libmgmc_<name>.so:
        python scripts/build_tuning_variants.py --exp ty16=ZS_TY:16 nt256=QUADS_NT:256,QUADS_NT3:256
    (MGMC_EXP_CXXDEFS adds compile definitions to every such build)
"""
from __future__ import annotations

import hashlib
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multigridmc_amd", "csrc")
HEADER = os.path.join(CSRC, "mgmc_tuning.hpp")
# any `constexpr <integer type> NAME = <value>;`, indented or not
CONSTANT = re.compile(r"^[ \t]*(?:static[ \t]+|inline[ \t]+)*constexpr[ \t]+((?:\w+[ \t]+)+?)(\w+)[ \t]*=[ \t]*([^;]*);", re.M)


def variants() -> dict:
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from tests.tuning_variants import VARIANTS
    return VARIANTS


def _value(text: str) -> int:
    """An integer literal or a product of them (`16 * 1024`); anything else is an error."""
    out = 1
    for factor in text.split("*"):
        out *= int(factor.strip(), 0)
    return out


def header_text() -> str:
    with open(HEADER) as fh:
        return fh.read()


def header_constants(text: str | None = None) -> dict:
    """name -> value of every constexpr constant of mgmc_tuning.hpp."""
    return {m.group(2): _value(m.group(3)) for m in CONSTANT.finditer(header_text() if text is None else text)}


def edited_header(edits: dict) -> str:
    """The text of mgmc_tuning.hpp with `edits` applied; an unknown constant is an error."""
    text = header_text()
    for key, value in edits.items():
        def put(m):
            return m.group(0)[:m.start(3) - m.start(0)] + str(int(value)) + ";"
        hits = [m for m in CONSTANT.finditer(text) if m.group(2) == key]
        if len(hits) != 1:
            raise KeyError(f"no constant {key} in mgmc_tuning.hpp")
        m = hits[0]
        text = text[:m.start()] + put(m) + text[m.end():]
    return text


def library_path(name: str, prefix: str = "tune_") -> str:
    return os.path.join(ROOT, "build", f"libmgmc_{prefix}{name}.so")


def _put(path: str, data: bytes) -> None:
    if os.path.exists(path):
        with open(path, "rb") as fh:
            if fh.read() == data:
                return
    with open(path, "wb") as fh:
        fh.write(data)


def _sources(edits: dict) -> dict:
    """relative path -> contents of everything a variant is compiled from"""
    out = {}
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith((".hip", ".cpp", ".hpp", ".h")) or fn == "Makefile":
            if fn == "mgmc_tuning.hpp":
                out["multigridmc_amd/csrc/" + fn] = edited_header(edits).encode()
            else:
                with open(os.path.join(CSRC, fn), "rb") as fh:
                    out["multigridmc_amd/csrc/" + fn] = fh.read()
    inc = os.path.join(ROOT, "include")
    for fn in sorted(os.listdir(inc)):
        if fn.endswith(".h"):
            with open(os.path.join(inc, fn), "rb") as fh:
                out["include/" + fn] = fh.read()
    return out


def _digest(sources: dict, flags: str) -> str:
    h = hashlib.sha256(flags.encode())
    for rel, data in sources.items():
        h.update(rel.encode() + b"\0" + hashlib.sha256(data).digest())
    return h.hexdigest()


def up_to_date(lib: str, digest: str) -> bool:
    stamp = lib + ".inputs"
    if not (os.path.exists(lib) and os.path.exists(stamp)):
        return False
    with open(stamp) as fh:
        return fh.read().strip() == digest


def build(names=None, specs: dict | None = None, prefix: str = "tune_", cxxdefs: str = "") -> list:
    """Build the named variants of tests/tuning_variants.py (default: all), or the given {name: edits}, in parallel;
    returns the library paths.  A library whose inputs have not changed is left alone."""
    if specs is None:
        specs = {name: variants()[name] for name in (names or variants())}
    todo = []
    for name, edits in specs.items():
        sources = _sources(edits)
        digest = _digest(sources, cxxdefs)
        lib = library_path(name, prefix)
        if not up_to_date(lib, digest):
            todo.append((name, sources, digest, lib))
    jobs = max(1, min(16, os.cpu_count() or 1) // max(1, len(todo)))
    procs = []
    for name, sources, digest, lib in todo:
        top = os.path.join(ROOT, "build", f"exp_{prefix}{name}")
        for rel, data in sources.items():
            os.makedirs(os.path.dirname(os.path.join(top, rel)), exist_ok=True)
            _put(os.path.join(top, rel), data)
        src = os.path.join(top, "multigridmc_amd", "csrc")
        for fn in os.listdir(src):  # a source file the product no longer has
            if "multigridmc_amd/csrc/" + fn not in sources:
                os.remove(os.path.join(src, fn))
        if os.path.exists(lib + ".inputs"):
            os.remove(lib + ".inputs")  # (a failed compile leaves no library that looks current)
        cmd = ["make", "-j", str(jobs), "-C", src]
        if cxxdefs:  # the product's flags, plus the definitions
            cmd.append("HIPFLAGS=-O3 -std=c++17 -ffp-contract=off -fPIC -w --offload-arch=gfx950 " + cxxdefs)
        procs.append((name, src, digest, lib, subprocess.Popen(cmd, stdout=subprocess.DEVNULL)))
    failed = [name for name, _, _, _, p in procs if p.wait() != 0]
    if failed:
        raise RuntimeError(f"variant(s) {', '.join(failed)} failed to compile")
    for name, src, digest, lib, _ in procs:
        shutil.copy2(os.path.join(os.path.dirname(src), "libmgmc_hip.so"), lib + ".tmp")
        os.replace(lib + ".tmp", lib)
        with open(lib + ".inputs", "w") as fh:
            fh.write(digest + "\n")
    return [library_path(name, prefix) for name in specs]


def main(argv) -> int:
    if argv and argv[0] == "--exp":
        specs = {}
        for v in argv[1:]:
            name, _, edits = v.partition("=")
            specs[name] = {k: int(val, 0) for k, _, val in (e.partition(":") for e in edits.split(",") if e and e != "-")}
        paths = build(specs=specs, prefix="", cxxdefs=os.environ.get("MGMC_EXP_CXXDEFS", ""))
    else:
        paths = build(argv or None)
    for path in paths:
        print(path)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
