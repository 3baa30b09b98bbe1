"""The host builder of a prepared list's neighbour-pixel set (csrc/value_union.h) against a brute-force numpy union.

The header is plain C++.  It is compiled here with a small main of its own under AddressSanitizer and UBSan and run as a
stand-alone program: boxes, links and the chunk size go in on stdin, offsets and items come back on stdout.  The
reference marks every link's rectangle -- value_kernel's: the rows of both patches, the columns of both with the
neighbour's last one excluded -- in a mask of the neighbour's patch and reads the mask back in buffer order (h fastest)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "celeste.jl_amd", "csrc")

MAIN = r"""
#include <cstdio>
#include "value_union.h"
int main() {
    int chunk_px, nb, nl;
    if (scanf("%d %d %d", &chunk_px, &nb, &nl) != 3) return 2;
    std::vector<ValueUnionBox> boxes((size_t)nb);
    for (auto &b : boxes) if (scanf("%d %d %d %d", &b.off_h, &b.off_w, &b.H2, &b.W2) != 4) return 2;
    std::vector<ValueUnionLink> links((size_t)nl);
    for (auto &l : links) if (scanf("%d %d", &l.vb, &l.va) != 2) return 2;
    std::vector<int32_t> offsets;
    std::vector<ValueUnionItem> items;
    if (!value_union_build(boxes.data(), links, chunk_px, offsets, items)) return 3;
    printf("%zu %zu\n", offsets.size(), items.size());
    for (int32_t o : offsets) printf("%d\n", o);
    for (auto &it : items) printf("%d %d %d %d\n", it.vb, it.first, it.count, it.trips);
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to compile csrc/value_union.h"
    d = tmp_path_factory.mktemp("value_union")
    src, exe = d / "main.cpp", d / "value_union_main"
    src.write_text(MAIN)
    subprocess.check_call([gxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)])
    return str(exe)


def _run(program, boxes, links, chunk_px=256):
    text = "%d %d %d\n" % (chunk_px, len(boxes), len(links))
    text += "".join("%d %d %d %d\n" % tuple(b) for b in boxes) + "".join("%d %d\n" % tuple(l) for l in links)
    r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    tok = np.array(r.stdout.split(), dtype=np.int64)
    n_off, n_items = int(tok[0]), int(tok[1])
    assert tok.size == 2 + n_off + 4 * n_items
    return tok[2:2 + n_off], tok[2 + n_off:].reshape(n_items, 4)


def _links(visit, neighbors, targets):
    """every (neighbour's visit, target's visit) pair of the listed targets, repeats and all; visit[s] = box of source s"""
    return [(visit[s2], visit[t]) for t in targets for s2 in neighbors[t]]


def _reference(boxes, links, chunk_px=256):
    offsets, items = [], []
    for vb in sorted({l[0] for l in links}):
        bh, bw, BH, BW = boxes[vb]
        mask = np.zeros((BW, BH), dtype=bool)                    # [w][h]: h fastest in the buffer
        for vb2, va in links:
            if vb2 != vb:
                continue
            ah, aw, AH, AW = boxes[va]
            h_lo, h_hi = max(ah, bh), min(ah + AH, bh + BH)
            w_lo, w_hi = max(aw, bw), min(aw + AW, bw + BW - 1)  # the neighbour's last column is excluded, the target's is not
            if h_hi > h_lo and w_hi > w_lo:
                mask[w_lo - bw:w_hi - bw, h_lo - bh:h_hi - bh] = True
        off = np.flatnonzero(mask.ravel())
        first = len(offsets)
        offsets.extend(off.tolist())
        for p0 in range(0, off.size, chunk_px):
            px = min(chunk_px, off.size - p0)
            items.append((vb, first + p0, px, (px + 63) // 64))
    items.sort(key=lambda it: -it[3])                            # stable: longest first, then by visit and chunk
    return np.array(offsets, dtype=np.int64), np.array(items, dtype=np.int64).reshape(-1, 4)


def _check(program, boxes, links, chunk_px=256):
    off, items = _run(program, boxes, links, chunk_px)
    roff, ritems = _reference(boxes, links, chunk_px)
    assert np.array_equal(off, roff)
    assert np.array_equal(items, ritems)
    # what the kernel relies on: the items tile the offsets, stay inside their patch, and never exceed a chunk
    assert items[:, 2].sum() == off.size and (items[:, 2] >= 1).all() and (items[:, 2] <= chunk_px).all()
    assert (np.diff(items[:, 3]) <= 0).all()
    for vb, first, count, _ in items:
        o = off[first:first + count]
        assert (np.diff(o) > 0).all() and o[0] >= 0 and o[-1] < boxes[vb][2] * boxes[vb][3]
    return off, items


def test_no_overlap(program):
    boxes = [(0, 0, 10, 10), (20, 20, 10, 10), (0, 10, 10, 10)]      # (box 2 touches box 0's last column from outside)
    off, items = _check(program, boxes, [(1, 0), (0, 1), (2, 0)])
    assert off.size == 0 and items.shape[0] == 0


def test_overlap_only_in_the_neighbours_last_column_is_empty(program):
    boxes = [(0, 0, 10, 10), (2, 9, 10, 10)]       # the target (1) starts in the neighbour's (0) last column
    off, items = _check(program, boxes, [(0, 1)])
    assert off.size == 0 and items.shape[0] == 0


def test_overlap_reaching_the_targets_last_column_is_kept(program):
    boxes = [(0, 5, 10, 10), (2, 0, 10, 8)]        # the target (1) ends at column 7, inside the neighbour (0)
    off, _ = _check(program, boxes, [(0, 1)])
    assert off.size == 8 * 3                       # rows 2..9, columns 5, 6 and 7: the target's last column is there
    assert 8 + 10 * 2 in off.tolist()              # (h0, w0) = (8, 7)


def test_patches_clipped_at_the_image_edge(program):
    # 30 x 30 image: patches of nominal size 13 cut at its borders, odd sizes, three sources all neighbours of each other
    boxes = [(0, 0, 7, 9), (3, 4, 13, 13), (22, 19, 8, 11), (0, 21, 11, 9), (18, 0, 12, 6)]
    nb = {s: [q for q in range(5) if q != s] for s in range(5)}
    off, _ = _check(program, boxes, _links(list(range(5)), nb, range(5)))
    assert off.size > 0


def test_two_targets_with_the_identical_rectangle(program):
    boxes = [(0, 0, 12, 12), (4, 4, 20, 20), (4, 4, 20, 20)]
    one, _ = _check(program, boxes, [(0, 1)])
    two, items = _check(program, boxes, [(0, 1), (0, 2)])
    assert np.array_equal(one, two) and one.size == 8 * 7 and items.shape[0] == 1


def test_a_repeated_target_changes_nothing(program):
    boxes = [(0, 0, 14, 14), (5, 3, 14, 14), (9, 9, 14, 14)]
    nb = {0: [1, 2], 1: [0, 2], 2: [0, 1]}
    once = _check(program, boxes, _links([0, 1, 2], nb, [0, 1]))
    again = _check(program, boxes, _links([0, 1, 2], nb, [0, 1, 1, 0, 0]))
    assert np.array_equal(once[0], again[0]) and np.array_equal(once[1], again[1])


def test_unions_of_256_257_and_320_pixels_split_and_order(program):
    # neighbours 0, 1, 2: 20 x 20 patches far apart; 3: a small one.  Targets (boxes 4 ..) placed on them:
    #   a 16 x 16 corner (256 pixels); the same and one more pixel (257); the same and a 4 x 16 strip (320); 130 pixels
    boxes = [(0, 0, 20, 20), (100, 0, 20, 20), (200, 0, 20, 20), (300, 0, 13, 11),
             (-4, -4, 20, 20),                                   # 4: rows 0..15, columns 0..15 of neighbour 0
             (96, -4, 20, 20), (119, 18, 5, 5),                  # 5, 6: the corner of neighbour 1 and its pixel (19, 18)
             (196, -4, 20, 20), (216, 0, 10, 16),                # 7, 8: the corner of neighbour 2 and rows 16..19, columns 0..15
             (300, 0, 13, 40)]                                   # 9: all of neighbour 3 but its last column: 13 x 10
    links = [(3, 9), (2, 8), (2, 7), (1, 6), (1, 5), (0, 4)]
    off, items = _check(program, boxes, links)
    assert off.size == 256 + 257 + 320 + 130
    assert [tuple(r) for r in items] == [(0, 0, 256, 4), (1, 256, 256, 4), (2, 513, 256, 4), (3, 833, 130, 3),
                                         (1, 512, 1, 1), (2, 769, 64, 1)]
    # another chunk size cuts the same offsets differently
    off128, items128 = _check(program, boxes, links, chunk_px=128)
    assert np.array_equal(off, off128) and items128.shape[0] == 2 + 3 + 3 + 2


def test_targets_without_neighbours_give_no_items(program):
    boxes = [(0, 0, 10, 10), (5, 5, 10, 10), (50, 50, 10, 10)]
    nb = {0: [1], 1: [0], 2: []}
    off, items = _check(program, boxes, _links([0, 1, 2], nb, [2, 2]))
    assert off.size == 0 and items.shape[0] == 0
