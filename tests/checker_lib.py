"""Builds and loads the C checkers of the tests (tests/*_checker.c).  TEST INFRASTRUCTURE.

  load(src_name, link_oracle=True, includes=())   tests/<src_name> compiled with gcc when its library is missing or older than what
                                                  it is made from, then ctypes.CDLL of it

Every checker is compiled with the flags of oracle/build.py (no contraction, no fast-math: the float32 order written in the source
is the order that runs).  `link_oracle`: the checker calls routines of the oracle library (oracle/librs_oracle.so, built when
stale) and is linked against it; `includes`: further files of tests/ the source #includes.
"""
import ctypes
import os
import subprocess
import tempfile

from oracle import build as obuild

HERE = os.path.dirname(os.path.abspath(__file__))
_libs = {}


def _out_dir():
    for d in (os.path.join(HERE, "_build"), os.path.join(tempfile.gettempdir(), f"rs_checkers_{os.getuid()}")):
        try:
            os.makedirs(d, exist_ok=True)
            if os.access(d, os.W_OK):
                return d
        except OSError:
            continue
    raise RuntimeError("no writable directory for the checker libraries")


def load(src_name, link_oracle=True, includes=()):
    if src_name not in _libs:
        src = os.path.join(HERE, src_name)
        out = os.path.join(_out_dir(), os.path.splitext(src_name)[0] + ".so")
        deps = [src, os.path.join(obuild.HERE, "rnnt_math.h")] + [os.path.join(HERE, p) for p in includes]
        link = []
        if link_oracle:
            from oracle import greedy as og
            og.lib()                                             # builds oracle/librs_oracle.so when stale, and loads it
            deps.append(obuild.OUT)
            link = [obuild.OUT, "-Wl,-rpath," + obuild.HERE]
        if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(p) for p in deps):
            subprocess.check_call(["gcc", "-O2", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-I", obuild.HERE,
                                   "-I", HERE, "-o", out, src] + link + ["-lm"])
        _libs[src_name] = ctypes.CDLL(out)
    return _libs[src_name]
