// The neighbour pixels a target list wants, each once (plain C++: no HIP in this header, tests/test_value_union_host.py
// compiles it on its own).
//
// value_kernel renders a neighbour's light once per LINK (target t -> neighbour s2, image): on the rectangle where s2's
// patch, minus its last column (elbo_objective.jl:349), overlaps t's patch.  A neighbour of several targets is rendered again
// for every one of them, into the same addresses of its own patch buffer, and every small rectangle ends in a partly
// empty wavefront.  The set of pixels is a function of (context, target list) and not of vp, so a prepared list
// (celeste_targets_t) has it made here once: per visit vb = (s2, image) the UNION of those rectangles over the list's
// targets, as ascending offsets (h0 - off_h) + H2 (w0 - off_w) into s2's own patch buffer (h fastest, as the buffer is
// laid out), concatenated for all visits; and work items {vb, first, count <= chunk_px} over that array, the items that
// take most 64-pixel trips first.  No pixel is added and none left out.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

struct ValueUnionBox { int32_t off_h, off_w, H2, W2; };      // a visit's patch: corner (0-based image coordinates) and size
struct ValueUnionLink { int32_t vb, va; };                    // visit of the neighbour, visit of the target (one image)
struct ValueUnionItem { int32_t vb, first, count, trips; };   // offsets[first, first + count) of visit vb; trips = ceil(count / 64)

// boxes[v]: the patch of visit v.  links: every (neighbour, target) pair of visits in one image, for the targets of the
// list; order and repeats do not matter (a repeated target, two targets with one rectangle).  chunk_px: a multiple of 64.
// Returns false when the offsets do not fit 32-bit indices (nothing is then to be used).
inline bool value_union_build(const ValueUnionBox *boxes, std::vector<ValueUnionLink> links, int chunk_px,
                              std::vector<int32_t> &offsets, std::vector<ValueUnionItem> &items) {
    offsets.clear(); items.clear();
    std::sort(links.begin(), links.end(), [](const ValueUnionLink &a, const ValueUnionLink &b) {
        return a.vb != b.vb ? a.vb < b.vb : a.va < b.va;
    });
    links.erase(std::unique(links.begin(), links.end(), [](const ValueUnionLink &a, const ValueUnionLink &b) {
        return a.vb == b.vb && a.va == b.va;
    }), links.end());
    const int n_cls = chunk_px / 64;
    std::vector<std::vector<ValueUnionItem>> by_len((size_t)std::max(n_cls, 1));   // [n_cls - trips]
    std::vector<unsigned char> wanted;
    for (size_t i = 0; i < links.size();) {
        const int32_t vb = links[i].vb;
        const ValueUnionBox &b = boxes[vb];
        const size_t npx = b.H2 > 0 && b.W2 > 0 ? (size_t)b.H2 * (size_t)b.W2 : 0;
        wanted.assign(npx, 0);
        for (; i < links.size() && links[i].vb == vb; ++i) {
            const ValueUnionBox &a = boxes[links[i].va];
            // value_kernel's rectangle: rows of both patches; columns of both, the neighbour's last one excluded
            const int64_t h_lo = std::max(a.off_h, b.off_h), h_hi = std::min((int64_t)a.off_h + a.H2, (int64_t)b.off_h + b.H2);
            const int64_t w_lo = std::max(a.off_w, b.off_w), w_hi = std::min((int64_t)a.off_w + a.W2, (int64_t)b.off_w + b.W2 - 1);
            for (int64_t w = w_lo; w < w_hi; ++w)
                for (int64_t h = h_lo; h < h_hi; ++h) wanted[(size_t)((h - b.off_h) + (int64_t)b.H2 * (w - b.off_w))] = 1;
        }
        const size_t first = offsets.size();
        for (size_t p = 0; p < npx; ++p) if (wanted[p]) offsets.push_back((int32_t)p);
        const size_t count = offsets.size() - first;
        if (offsets.size() > (size_t)INT32_MAX) { offsets.clear(); items.clear(); return false; }
        for (size_t p0 = 0; p0 < count; p0 += (size_t)chunk_px) {
            const int32_t px = (int32_t)std::min((size_t)chunk_px, count - p0), trips = (px + 63) / 64;
            by_len[(size_t)(n_cls - trips)].push_back({vb, (int32_t)(first + p0), px, trips});
        }
    }
    for (auto &v : by_len) items.insert(items.end(), v.begin(), v.end());
    return true;
}
