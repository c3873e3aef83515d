"""CPU test of the one-shot calls' device layout (csrc/rtg_stage.h): where the
parts of a call lie in its one allocation.  A wrong offset here is an
out-of-bounds copy or kernel access on the GPU, so it is checked before anything
runs there.

tests/stage_layout.cpp includes the header alone and is built with the address
and undefined-behaviour sanitizers; it runs as a child process.
"""
from __future__ import annotations

import itertools
import os
import random
import subprocess

import pytest

from conftest import BUILD, ROOT

ALIGN = 256
SIZES = [0, 1, 15, 16, 17, 255, 256, 257, 2 ** 33 + 1]


@pytest.fixture(scope="module")
def stage_layout():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "stage_layout")
    src = os.path.join(ROOT, "tests", "stage_layout.cpp")
    hdr = os.path.join(ROOT, "raytracer-gamma_amd", "csrc", "rtg_stage.h")
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe)
                                      for d in (src, hdr, os.path.abspath(__file__))):
        tmp = "%s.%d.tmp" % (exe, os.getpid())  # (parallel workers: renamed into place)
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.dirname(hdr), src, "-o", tmp], check=True)
        os.replace(tmp, exe)

    def run(lists):
        """[(offsets, None where absent), total] per list of sizes."""
        out = subprocess.run([exe] + [",".join(map(str, sizes)) for sizes in lists], check=True,
                             capture_output=True, text=True).stdout.splitlines()
        assert len(out) == len(lists)
        res = []
        for line, sizes in zip(out, lists):
            words = line.split()
            assert len(words) == len(sizes) + 1, (sizes, line)
            res.append(([None if w == "-" else int(w) for w in words[:-1]], int(words[-1])))
        return res

    return run


def _lists():
    rng = random.Random(256)
    lists = [list(SIZES), list(reversed(SIZES)), [0], [0, 0, 0], [1], [2 ** 33 + 1] * 3]
    lists += [list(p) for p in itertools.product(SIZES, repeat=2)]
    for _ in range(40):  # every size in some order, then with runs of empty parts put in
        order = rng.sample(SIZES, len(SIZES))
        lists.append(order)
        holes = [s for s in order if s]
        for at in sorted(rng.sample(range(len(holes) + 1), 3), reverse=True):
            holes[at:at] = [0] * rng.randint(1, 3)
        lists.append([0] + holes + [0, 0])
    # empty parts first, last and adjacent, around every pair of sizes
    lists += [[0, 0, a, 0, 0, b, 0] for a in SIZES[1:] for b in SIZES[1:]]
    return lists


def test_layout(stage_layout):
    lists = _lists()
    for sizes, (offsets, total) in zip(lists, stage_layout(lists)):
        end = 0
        for size, at in zip(sizes, offsets):
            if size == 0:
                assert at is None, (sizes, offsets)  # an empty part is absent
                continue
            assert at is not None and at % ALIGN == 0, (sizes, offsets)
            assert at >= end, (sizes, offsets)  # list order, no overlap
            assert at - end < ALIGN, (sizes, offsets)  # and no more padding than the alignment
            end = at + size
        assert total == end, (sizes, offsets, total)  # the last end; all empty: 0
    assert stage_layout([[0, 0]]) == [([None, None], 0)] and stage_layout([[]]) == [([], 0)]
