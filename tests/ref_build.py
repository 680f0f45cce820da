"""Builds and loads the CPU references under tests/support/ (tests only; not a conftest).

Each reference is one C++ file that includes the oracle's translation unit, compiled
with oracle/Makefile's flags into tests/support/build/lib<name>.so.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# oracle/Makefile's CXXFLAGS + ARCHFLAGS, exactly
FLAGS = ["-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fopenmp",
         "-march=x86-64-v3"]
LITERAL = os.path.join(ROOT, "oracle", "glsl_literal.cpp")
# what every reference is compiled from, besides its own source
ORACLE_DEPS = [os.path.join(ROOT, "oracle", "cvr_oracle.cpp"), LITERAL,
               os.path.join(ROOT, "oracle", "oracle_types.h")]


def build(name: str) -> str:
    """Compile tests/support/<name>.cpp (when its library is missing or older than a source)."""
    src = os.path.join(HERE, "support", name + ".cpp")
    out = os.path.join(HERE, "support", "build", f"lib{name}.so")
    deps = [src, *ORACLE_DEPS]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    tmp = out + f".{os.getpid()}.tmp"
    subprocess.run([os.environ.get("CXX", "g++"), *FLAGS, "-shared", "-o", tmp, src, LITERAL], check=True)
    os.replace(tmp, out)
    return out


_libs: dict = {}


def build_and_load(name: str, bind=None) -> ctypes.CDLL:
    """The library of tests/support/<name>.cpp, built when stale and loaded once per
    process; bind(lib) declares its functions' argument types on that first load."""
    if name not in _libs:
        L = ctypes.CDLL(build(name))
        if bind is not None:
            bind(L)
        _libs[name] = L
    return _libs[name]
