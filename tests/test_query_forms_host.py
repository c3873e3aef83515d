"""The masked scenes' query forms of rtg_trace.h against the plain loops, on the
host, under AddressSanitizer + UBSan.

tests/hostsim/query_forms.cpp is a stand-alone program: it compiles the host
forms of closest_sel(_fused, _lazy), closest_hit_sel(_fused), closest_enter(_fused),
blocked_sel(_fused) and primary_container_sel and compares each, bit for bit,
with closest_hit, blocked and primary_container on hand-placed scenes:
selections of 0 to 3 spheres at bit positions 0, 31, 32 and 63; the own and the
origin sphere skipped as the only candidate and as either one of a pair; a
first sphere that blocks; two coincident spheres (equal t, the lower index
wins); directions that put 2a outside [2^-60, 2^60] (the division fallback);
NaN and infinite origins and directions (raygen.scaled's value set, restated in
the program).  It returns 0 only if every comparison held and the reference
answers were not vacuous (hits, blockers, passed guard tests, selections that
ran empty).  Built with -fsanitize=address,undefined and run as a program of
its own: no Python in that process.
"""
from __future__ import annotations

import os
import subprocess

from conftest import BUILD, ROOT

SRC = os.path.join(ROOT, "tests", "hostsim", "query_forms.cpp")
CSRC = os.path.join(ROOT, "raytracer-gamma_amd", "csrc")
FLAGS = ["-O1", "-mfma", "-ffp-contract=off", "-fno-fast-math", "-std=c++17",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
         "-g", "-static-libasan", "-static-libubsan"]  # the runtimes in the program itself


def _program():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "query_forms_san")
    deps = [SRC, os.path.abspath(__file__)] + [
        os.path.join(CSRC, f) for f in ("rtg_trace.h", "rtg_scene_pack.h", "rtg_internal.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        tmp = "%s.%d.tmp" % (exe, os.getpid())  # renamed into place (parallel workers)
        subprocess.run(["g++", *FLAGS, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, SRC,
                        "-o", tmp], check=True)
        os.replace(tmp, exe)
    return exe


def test_query_forms_equal_plain_loops_under_asan_ubsan():
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r =subprocess.run([_program()], env=env, capture_output=True, text=True, timeout=300)
    tail = (r.stdout + r.stderr)[-4000:]
    assert r.returncode == 0, tail
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, tail
    assert r.stdout.startswith("query_forms: ") and " 0 failed;" in r.stdout, tail
    assert "VACUOUS" not in r.stdout, tail
