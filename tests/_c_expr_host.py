"""Evaluate translated C expressions as C, on the host.

The JIT translator emits a C expression over typed per-row values
v0..vN. Evaluating that text as Python/numpy hides exactly the bugs C
has and Python does not (truncating `/`, unsigned literals, 32-bit
overflow), so the CPU tier compiles it instead: every entry of a batch
becomes one function of a single translation unit, built once with the
host C++ compiler (`-O1 -ffp-contract=off`, nothing preloaded) and
loaded through ctypes. One compiler invocation per CExprLib."""
import ctypes
import os
import shutil
import subprocess

import numpy as np

# exactly qk_jit.cpp's type_name()
C_TYPE = {np.dtype(np.int32): "int", np.dtype(np.float64): "double",
          np.dtype(np.uint8): "unsigned char",
          np.dtype(np.int64): "long long"}


def find_cxx():
    """ROCm's clang (what csrc/Makefile's hipcc drives), else c++."""
    roots = [os.environ.get("ROCM_PATH"), "/opt/rocm"]
    for r in roots:
        if r:
            p = os.path.join(r, "llvm", "bin", "clang++")
            if os.path.exists(p):
                return p
    for name in ("c++", "clang++", "g++"):
        p = shutil.which(name)
        if p:
            return p
    raise AssertionError("no host C++ compiler found (looked for ROCm's "
                         "clang++, c++, clang++, g++)")


# An integer division by zero traps on the host (SIGFPE). The translator
# must never emit one, and a regression should fail its test, not end the
# test process: each function returns 1 when its loop trapped.
_PRELUDE = """#include <setjmp.h>
#include <signal.h>
static sigjmp_buf qk_jb;
static void qk_on_fpe(int) { siglongjmp(qk_jb, 1); }
#define QK_TRAP_BEGIN \\
  struct sigaction qk_sa = {}, qk_old; qk_sa.sa_handler = qk_on_fpe; \\
  sigaction(SIGFPE, &qk_sa, &qk_old); \\
  if (sigsetjmp(qk_jb, 1)) { sigaction(SIGFPE, &qk_old, 0); return 1; }
#define QK_TRAP_END sigaction(SIGFPE, &qk_old, 0); return 0;
"""


class CExprLib:
    """entries: list of (c_expr, coltypes) or (c_expr, coltypes, kind);
    coltypes are the numpy dtypes of v0..vN in order; kind is "pred"
    (stores (expr) != 0 into u8) or "arith" (stores (double)(expr))."""

    def __init__(self, entries, tmp_path, name="jitexpr"):
        self.entries = [(e[0], [np.dtype(t) for t in e[1]],
                         e[2] if len(e) > 2 else "pred") for e in entries]
        src = []
        for i, (expr, types, kind) in enumerate(self.entries):
            out_t = "unsigned char" if kind == "pred" else "double"
            args = "".join(", const %s* c%d" % (C_TYPE[t], k)
                           for k, t in enumerate(types))
            loads = "".join("    %s v%d = c%d[i];\n" % (C_TYPE[t], k, k)
                            for k, t in enumerate(types))
            store = ("((%s) != 0)" if kind == "pred"
                     else "(double)(%s)") % expr
            src.append('extern "C" int f%d(long n, %s* out%s) {\n'
                       "  QK_TRAP_BEGIN\n"
                       "  for (long i = 0; i < n; i++) {\n%s"
                       "    out[i] = %s;\n  }\n"
                       "  QK_TRAP_END\n}\n"
                       % (i, out_t, args, loads, store))
        cpath = os.path.join(str(tmp_path), name + ".cpp")
        sopath = os.path.join(str(tmp_path), name + ".so")
        with open(cpath, "w") as f:
            f.write(_PRELUDE + "".join(src))
        cmd = [find_cxx(), "-O1", "-ffp-contract=off", "-std=c++17", "-w",
               "-shared", "-fPIC", cpath, "-o", sopath]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, "host compile failed:\n%s" % r.stderr[-4000:]
        self.lib = ctypes.CDLL(sopath)

    def run(self, i, arrays, n=None):
        """arrays: the v0..vN inputs in order -> u8 bool / f64 output."""
        expr, types, kind = self.entries[i]
        assert len(arrays) == len(types), expr
        arrs = [np.ascontiguousarray(a, dtype=t)
                for a, t in zip(arrays, types)]
        if n is None:
            n = len(arrs[0])
        assert all(len(a) == n for a in arrs)
        out = np.zeros(n, dtype=np.uint8 if kind == "pred" else np.float64)
        fn = getattr(self.lib, "f%d" % i)
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_long] + [ctypes.c_void_p] * (1 + len(arrs))
        rc = fn(n, out.ctypes.data, *[a.ctypes.data for a in arrs])
        assert rc == 0, "integer division by zero trapped in: %s" % expr
        return out.astype(bool) if kind == "pred" else out
