// A prepared list's work items, each described once (plain C++: no HIP in this header, tests/test_work_sequences_host.py
// compiles it on its own).
//
// pixel_kernel runs one workgroup (one wavefront) per work item: a group of up to G consecutive chunks of one patch.  Its
// prologue chases work[item] through four tables before the first pixel.  The items of a prepared list (celeste_targets_t)
// are a function of (context, target list) and not of vp, so the list has each of them described here once, in one
// 64-byte record that holds what the prologue looked up; workgroup b of pixel_desc_kernel starts from record b.
// (Packing several items into one workgroup was built and measured as a loss: TRIED.md, tools/variants/r11_item_packing.patch.)
#pragma once
#include <cstddef>
#include <cstdint>

// What a workgroup needs to start on an item, in one uniform 64-byte load.  Nothing in it depends on vp.  The first 32
// bytes are laid out as the head of DevPatch (elbo_device.h; pixel_desc_kernel asserts the offsets): the pixel loop reads
// the patch's corner, size and bitmap through a DevPatch pointer, and is handed this record instead of patches[v].
struct alignas(64) WorkSeqDesc {
    int32_t off_h, off_w, H2, W2;   // the patch: corner (0-based image coordinates) and size
    int64_t bitmap_off;             // -1: bitmap == !isnan(pixel)
    int32_t stamp;                  // its PSF stamp (star spline coefficients)
    int32_t nbn;                    // the target's neighbours: nbr_idx[nb0 .. nb0 + nbn)
    int64_t nb0;
    int64_t nv_row;                 // visit-list contexts: the row of this visit in nbr_vis
    int32_t v, n;                   // visit (table entry of the target in this image), image
    int32_t rec_base;               // first chunk record of the visit (rec_off[ti * M + j]); chunk ch writes record rec_base + ch
    int32_t ch0;                    // the item's first chunk; it runs up to G chunks, as many as the patch has
};
static_assert(sizeof(WorkSeqDesc) == 64 && offsetof(WorkSeqDesc, bitmap_off) == 16 && offsetof(WorkSeqDesc, stamp) == 24,
              "one uniform 64-byte load per item");

// 64-pixel trips of the work item that starts at chunk ch0 of a patch of npx pixels: up to G chunks of chunk_px pixels, as
// pixel_kernel's chunk loop runs them.  0 trips: the item does nothing (and gets no record).
inline int work_item_trips(int64_t npx, int ch0, int G, int chunk_px) {
    int trips = 0;
    for (int ch = ch0; ch < ch0 + G && (int64_t)ch * chunk_px < npx; ++ch) {
        const int64_t p0 = (int64_t)ch * chunk_px, p1 = npx < p0 + chunk_px ? npx : p0 + chunk_px;
        trips += (int)((p1 - p0 + 63) / 64);
    }
    return trips;
}
