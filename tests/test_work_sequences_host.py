"""The host side of a prepared list's work-item descriptors (csrc/work_sequences.h).

The header is plain C++.  It is compiled here with a small main of its own under AddressSanitizer and UBSan and run as a
stand-alone program: it prints the descriptor's layout and, for (npx, ch0, G, chunk_px) lines on stdin, the item's trips.
The trips are checked against a restatement of pixel_kernel's chunk loop; the layout against what pixel_desc_kernel relies
on -- 64 bytes, one uniform load, its head laid out as DevPatch's (elbo_device.h: off_h, off_w, H2, W2, bitmap_off, stamp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "celeste.jl_amd", "csrc")

MAIN = r"""
#include <cstdio>
#include "work_sequences.h"
#include "elbo_device.h"
int main() {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(WorkSeqDesc), alignof(WorkSeqDesc), offsetof(WorkSeqDesc, off_h),
           offsetof(WorkSeqDesc, off_w), offsetof(WorkSeqDesc, H2), offsetof(WorkSeqDesc, W2), offsetof(WorkSeqDesc, bitmap_off),
           offsetof(WorkSeqDesc, stamp));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", (size_t)64, (size_t)64, offsetof(DevPatch, off_h), offsetof(DevPatch, off_w),
           offsetof(DevPatch, H2), offsetof(DevPatch, W2), offsetof(DevPatch, bitmap_off), offsetof(DevPatch, stamp));
    long long npx; int ch0, G, chunk_px;
    while (scanf("%lld %d %d %d", &npx, &ch0, &G, &chunk_px) == 4) printf("%d\n", work_item_trips(npx, ch0, G, chunk_px));
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to compile csrc/work_sequences.h"
    d = tmp_path_factory.mktemp("work_sequences")
    src, exe = d / "main.cpp", d / "work_sequences_main"
    src.write_text(MAIN)
    subprocess.check_call([gxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-D__host__=", "-D__device__=", "-I", CSRC, str(src), "-o", str(exe)])
    return str(exe)


def _run(program, cases):
    text = "".join("%d %d %d %d\n" % c for c in cases)
    r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    return [int(x) for x in lines[0].split()], [int(x) for x in lines[1].split()], [int(x) for x in lines[2:]]


def test_the_descriptor_is_64_bytes_with_the_head_of_a_patch(program):
    desc, patch, _ = _run(program, [])
    assert desc[:2] == [64, 64]
    assert desc == patch


def test_trips_of_an_item_are_the_chunk_loops(program):
    cases = []
    for npx in (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 567, 768, 1025, 2600):
        for G in (1, 2, 4):
            for ch0 in range(0, 12, G):
                cases.append((npx, ch0, G, 256))
    cases += [(700, 0, 2, 128), (700, 4, 2, 128), (700, 6, 2, 128), (-5, 0, 2, 256)]
    _, _, got = _run(program, cases)
    assert len(got) == len(cases)
    for (npx, ch0, G, cpx), trips in zip(cases, got):
        want = 0
        for ch in range(ch0, ch0 + G):                                   # pixel_kernel's chunk loop
            if ch * cpx >= npx:
                break
            want += len(range(ch * cpx, min(npx, ch * cpx + cpx), 64))
        assert trips == want, (npx, ch0, G, cpx)
