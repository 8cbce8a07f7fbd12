// mixed_req_var_tile.h -- internal: what the parse kernels of the two server-side
// decodes over fixed-size and string plans share (mixed_req_var.hip: every plan
// in columns, k_mrv_parse; mixed_req_legs.hip: a plan's requests may also go to
// one device array of the caller's structs, k_mrl_parse): a lane's frame, in
// the image or in global memory, and the lane's bounded walk of its fields into
// the plan's columns.  With them the launches of the kernels that stay in
// mixed_req_var.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mixed_common.h"
#include "mixed_var_common.h"
#include "plan.h"
#include "srpc_gpu.h"

namespace srpc_impl {

// The frame of a lane: in the image when it lies whole inside it, else in
// global memory.
struct MrvFrame {
    const uint8_t* img;  // the image
    const uint8_t* g;    // the frame in global memory
    uint32_t q;          // the frame's image offset
    bool in_img;
};

// 8 bytes at frame byte c (c + 8 <= the frame's length).
__device__ __forceinline__ uint64_t mrv_u64(const MrvFrame& fr, uint64_t c) {
    return fr.in_img ? lds_u64(fr.img, fr.q + static_cast<uint32_t>(c)) : mv_get(fr.g + c, 8);
}

// The s <= 8 bytes at frame byte c.
__device__ __forceinline__ uint64_t mrv_field(const MrvFrame& fr, uint64_t c, uint32_t s) {
    if (!fr.in_img) return mv_get(fr.g + c, s);
    const uint32_t at = fr.q + static_cast<uint32_t>(c);
    return s == 1 ? fr.img[at] : lds_u64(fr.img, at) & (s == 8 ? ~0ull : (1ull << (8 * s)) - 1);
}

// Frame j of a tile (frame i of the batch), classified as one record of column
// plan k with rank `rank` < room[k]: its fixed leaves to element first[k] + rank
// of the plan's columns, each string's length into its offsets entry and its
// chars' stream offset to srcs.  lo[]: the tile's offsets (req_offsets), sp: its
// staged span (req_stage).  The class says the frame is one record of plan k;
// every read is still bounded by the frame's own extent, and what does not fit
// decodes to zero / empty.
__device__ __forceinline__ void mrv_lane_walk(const MvDesc* __restrict__ d, uint32_t k, uint32_t rank, uint32_t j,
                                              uint64_t i, const uint32_t* lo, const uint8_t* img, const ReqSpan& sp,
                                              const uint8_t* __restrict__ buf, uint64_t buf_len, uint64_t nframes,
                                              uint32_t* __restrict__ srcs) {
    const uint64_t o = lo[j], end = lo[j + 1];
    bool ok = o <= end && end <= buf_len;
    const uint64_t len = ok ? end - o : 0;
    MrvFrame fr;
    fr.img = img;
    fr.g = buf + o;
    fr.in_img = ok && o >= sp.s0 && o - sp.s0 + len <= sp.staged;
    fr.q = static_cast<uint32_t>(o - sp.s0);
    const uint64_t e = d->first[k] + rank;
    uint64_t c = (d->var[k] ? 4 : 0) + d->prefix_len[k];
    ok = ok && c <= len;
    uint32_t t = 0;
    for (uint32_t f = d->field0[k]; f < d->field0[k + 1]; ++f) {
        const uint32_t s = d->size[f];
        if (s) {
            ok = ok && s <= len - c;
            store_elem(d->col[f] + e * s, s, ok ? mrv_field(fr, c, s) : 0);
            if (ok) c += s;
        } else {
            ok = ok && 8 <= len - c;
            uint64_t sl = ok ? mrv_u64(fr, c) : 0;
            if (ok) c += 8;
            if (sl > len - c) {
                sl = 0;
                ok = false;
            }
            d->soffs[f][e + 1] = sl;  // its length: the slot scan turns lengths into offsets
            srcs[t * nframes + i] = static_cast<uint32_t>(o + c);
            c += sl;
            ++t;
        }
    }
}

// ---- mixed_req_var.hip ----
// The classify pass (k_mrv_classify: d.T frames a workgroup, the class byte of
// every frame) and the parse pass over plans that all live in columns
// (k_mrv_parse), nframes > 0.  mixed_req_legs.hip launches both: the first
// always, the second for a batch without a record plan.
void mrv_classify_launch(const MvDesc& d, const MvDesc* dd, const uint8_t* d_buf, uint64_t buf_len,
                         const uint32_t* d_offs, uint64_t nframes, uint8_t* d_class, hipStream_t s);
void mrv_parse_launch(const MvDesc& d, const MvDesc* dd, const uint8_t* d_class, const uint32_t* table, uint64_t rows,
                      const uint8_t* d_buf, uint64_t buf_len, const uint32_t* d_offs, uint64_t nframes, uint32_t* srcs,
                      uint32_t* counts, srpc_unpack_status* d_status, hipStream_t s);

}  // namespace srpc_impl
