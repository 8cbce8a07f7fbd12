// mixed_req_legs.hip -- the server's string-aware decode of a batch of request
// frames of several methods in arrival order: one host path
// (mv_unpack_requests), the mirror of mixed_legs.hip's request pack.  The entry
// points of include/srpc_gpu.h are adapters over it:
// srpc_frames_unpack_requests_mixed_legs, where a plan's requests go into
// columns (fixed-size or string plans) or into one device array of the caller's
// own structs (fixed-size plans; a record plan: h_stride[k] != 0), and
// srpc_frames_unpack_requests_mixed_var, which has no record arguments.
//
// Nothing here is a second implementation.  The description of the plans, the
// scratch, the slot scan and the char copy are mixed_var.hip's
// (mixed_var_common.h); the record plans' checks, tables and fills are
// mixed_legs_common.h's; the classify pass is mixed_req_var.hip's
// k_mrv_classify and the index mixed.hip's, so d_class, d_index and d_counts
// are the same whatever the plans' kinds.
//
//   k_mrl_parse   k_mrv_parse's tile -- the offsets, the granule's ranks from the
//       index, the span staged into the image -- with the record half of
//       k_req_decode_aos joined on: a lane of a column plan walks its frame as
//       k_mrv_parse's does (mrv_lane_walk, mixed_req_var_tile.h); a lane of a
//       record plan stores nothing itself but leaves pos[j], its frame's image
//       position or "outside the image" (a long string pushed it out of the
//       staged window: it is then read from global memory, at most F_k bytes,
//       its extent checked again).  The workgroup then writes the record plans'
//       slices of the tile as whole 16-byte pieces, non-temporally
//       (mix_aos_slices_*, mix_aos_store of mixed_aos_common.h).
//
// A batch without a record plan launches k_mrv_parse itself (mrv_parse_launch),
// for k_ml_parse's reason.  Scratch: mixed_legs.hip's layout.
// LDS of k_mrl_parse: image[W + 16] | tables and fills [desc_bytes],
// W = kMixImage - desc_bytes: the dynamic LDS of k_mrv_parse; then static wcnt,
// the tile's offsets, pos[], slot[] and the slices.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "aos_pieces.h"
#include "mixed_aos_common.h"
#include "mixed_common.h"
#include "mixed_legs_common.h"
#include "mixed_req_var_tile.h"
#include "mixed_var_common.h"
#include "mixed_var_tile.h"
#include "plan.h"
#include "srpc_gpu.h"

namespace srpc_impl {
namespace {

__global__ __launch_bounds__(kBlock) void k_mrl_parse(const MvDesc* __restrict__ d, MvLegs x,
                                                      const uint4* __restrict__ desc, const uint8_t* __restrict__ cls,
                                                      const uint32_t* __restrict__ table, uint64_t rows,
                                                      const uint8_t* __restrict__ buf, uint64_t buf_len,
                                                      const uint32_t* __restrict__ offs, uint64_t nframes,
                                                      uint32_t* __restrict__ srcs, uint32_t* __restrict__ counts,
                                                      srpc_unpack_status* st) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    __shared__ uint32_t wcnt[kMixLds];
    __shared__ uint32_t lo[kBlock + 1];
    __shared__ uint32_t pos[kBlock];
    __shared__ uint16_t slot[kBlock];
    __shared__ MixAosSlices sl;
    uint8_t* img = lds;
    uint8_t* dsc = lds + x.window + 16;
    const uint32_t K = d->nplans, T = d->T;
    mix_aos_slices_init(sl, x.x, K);
    for (uint32_t c = threadIdx.x; c < x.x.desc_bytes / 16; c += kBlock) reinterpret_cast<uint4*>(dsc)[c] = desc[c];
    const uint64_t c0 = static_cast<uint64_t>(blockIdx.x) * T;
    const uint64_t g = c0 / kMixGranule;
    const uint32_t j0 = static_cast<uint32_t>(c0 - g * kMixGranule);  // the tile's first lane
    const uint64_t i = g * kMixGranule + threadIdx.x;
    const uint32_t nr = c0 < nframes ? static_cast<uint32_t>(min<uint64_t>(T, nframes - c0)) : 0;
    req_offsets(lo, T, offs, nframes, c0, buf_len);

    const MixLane r = mix_ranks(cls, nframes, K, table, rows, g, wcnt);  // barrier: lo[] and the slices' init are complete
    // the batch's frames per plan, for the slot scan: the last tile's granule is the last one
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x < K) {
        uint32_t v = wcnt[kMixWaves * kMixRow + threadIdx.x];
        for (uint32_t w = 0; w < kMixWaves; ++w) v += wcnt[w * kMixRow + threadIdx.x];
        counts[threadIdx.x] = v;
    }
    const bool mine = threadIdx.x >= j0 && threadIdx.x < j0 + nr && r.cls < K;  // this tile's, and somebody's frame
    const bool good = mine && r.rank < d->room[r.cls];
    const bool rec = good && sl.stride[r.cls] != 0;
    const uint32_t j = threadIdx.x - j0;
    if (mine && !good && st) report_bad(st, SRPC_STATUS_BOUNDS, i);

    // the tile's slices: good frames of one record plan are consecutive ranks, ascending with the lane
    mix_aos_slices_count(sl, K, r, rec);

    // 1. the span of the tile's frames -> image, from a 16-byte boundary (ends with a barrier)
    const ReqSpan sp = req_stage(img, lo, nr, x.window, buf, buf_len);

    // 2. a lane per frame: a column plan's fields and string lengths, or where a record plan's frame is
    if (rec) {
        const uint64_t o = lo[j];
        const uint32_t F = d->F[r.cls];
        if (o > buf_len || F > buf_len - o) {
            pos[j] = kPosZero;  // the class says otherwise: never read past the buffer
        } else {
            const bool in_img = o >= sp.s0 && o - sp.s0 + F <= sp.staged;
            pos[j] = in_img ? static_cast<uint32_t>(o - sp.s0) : kPosGlobal;
        }
    } else if (good) {
        mrv_lane_walk(d, r.cls, r.rank, j, i, lo, img, sp, buf, buf_len, nframes, srcs);
    }

    // 3. image and fill -> the record plans' slices, one lane per (plan, 16-byte piece)
    mix_aos_store<true>(sl, *d, K, r, rec, j, img, lo, pos, slot, dsc, buf);
}

// The request decode: `legs` as at mv_pack_requests (mixed_legs.hip).
int mv_unpack_requests(bool legs, const srpc_plan* const* req_plans, int nplans, const uint8_t* d_buf,
                       uint64_t buf_len, const uint32_t* d_offs, uint64_t nframes, void* const* const* d_cols,
                       uint64_t* const* const* d_str_offs, const uint64_t* const* h_str_cap, void* const* d_recs,
                       const uint64_t* h_stride, const uint32_t* const* h_leaf_offs, const void* const* h_fill,
                       const uint64_t* h_first, const uint64_t* h_cap, uint8_t* d_class, void* d_index,
                       uint64_t index_bytes, uint64_t* d_counts, uint64_t* d_ends, srpc_unpack_status* d_status,
                       void* d_scratch, uint64_t scratch_bytes, void* stream) {
    const TimedCall timed;
    if (any_null(req_plans, d_cols, d_str_offs, h_str_cap, h_cap, d_index, d_counts, d_ends, d_scratch) ||
        mix_nplans_bad(nplans) || past_u32(buf_len) || past_u32(nframes) ||
        (nframes && any_null(d_buf, d_offs, d_class)))
        return SRPC_E_INVALID;
    if (legs && legs_args_invalid(d_recs, h_stride, h_leaf_offs, h_fill, true, h_first, h_cap, nplans))
        return SRPC_E_INVALID;
    if (!legs) h_stride = kAllColumns;
    static thread_local MvDesc d;
    d = MvDesc{};
    if (int rc = mv_plans(req_plans, nplans, 4, &d)) return rc;
    if (int rc = legs_plans_ok(req_plans, nplans, h_stride, true)) return rc;
    LegsTables t;  // d.T, for both passes: srpc_frames_mixed_legs_tile's
    if (int rc = legs_describe(req_plans, nplans, d_recs, h_stride, h_leaf_offs, h_fill, &d, &t)) return rc;
    if (!aligned(d_buf, 16) || !aligned(d_index, 8) || !aligned(d_counts, 8) || !aligned(d_ends, 8) ||
        !aligned(d_scratch, legs ? 16 : 8) || !aligned(d_offs, 4) ||
        !aos_recs_aligned(req_plans, nplans, d_recs, h_stride, h_leaf_offs))
        return SRPC_E_ALIGN;
    if (int rc = mv_cols(req_plans, nplans, reinterpret_cast<const void* const* const*>(d_cols),
                         reinterpret_cast<const uint64_t* const* const*>(d_str_offs), h_str_cap, h_first, h_cap, &d,
                         h_stride))
        return rc;
    legs_cols(req_plans, nplans, d_recs, h_stride, h_leaf_offs, &d);
    const MvScratch sc = mv_scratch(d, nframes);
    const uint64_t tables_at = legs_tables_at(sc);
    if (index_bytes < mix_index_bytes(nframes, nplans) ||
        scratch_bytes < (legs ? tables_at + t.x.x.desc_bytes : sc.bytes))
        return SRPC_E_CAPACITY;
    auto s = static_cast<hipStream_t>(stream);
    const MvCarve c(d_scratch, sc);
    auto* tables = static_cast<uint8_t*>(d_scratch) + tables_at;
    auto* table = static_cast<uint32_t*>(d_index);
    const uint64_t rows = mix_rows(nframes);
    if (d_status && status_reset_launch(d_status, s)) return SRPC_E_HIP;
    if (int rc = mix_upload(&d, sizeof d, d_scratch, s)) return rc;
    if (t.x.x.desc_bytes)
        if (int rc = mix_upload(t.desc.bytes, t.x.x.desc_bytes, tables, s)) return rc;
    if (nframes) mrv_classify_launch(d, c.dd, d_buf, buf_len, d_offs, nframes, d_class, s);
    // unknown frames (0xFF) are ids >= K: column K of the index; no status here
    if (int rc = mix_index_launch(d_class, nframes, nplans, table, d_counts, nullptr, s)) return rc;
    // without a record plan the kernel is mixed_req_var.hip's
    if (nframes && !t.x.x.desc_bytes)
        mrv_parse_launch(d, c.dd, d_class, table, rows, d_buf, buf_len, d_offs, nframes, c.srcs, c.counts, d_status, s);
    else if (nframes)
        launch(k_mrl_parse, dim3(static_cast<uint32_t>((nframes + d.T - 1) / d.T)), dim3(kBlock), kMixImage + 16, s, c.dd,
               t.x, reinterpret_cast<const uint4*>(tables), static_cast<const uint8_t*>(d_class),
               static_cast<const uint32_t*>(table), rows, d_buf, buf_len, d_offs, nframes, c.srcs, c.counts, d_status);
    return mv_strings_launch(d, c, sc.nb, d_class, table, nframes, d_buf, d_ends, s);
}

}  // namespace
}  // namespace srpc_impl

using namespace srpc_impl;

extern "C" {

int srpc_frames_unpack_requests_mixed_legs(const srpc_plan* const* req_plans, int nplans, const uint8_t* d_buf,
                                           uint64_t buf_len, const uint32_t* d_offs, uint64_t nframes,
                                           void* const* const* d_cols, uint64_t* const* const* d_str_offs,
                                           const uint64_t* const* h_str_cap, void* const* d_recs,
                                           const uint64_t* h_stride, const uint32_t* const* h_leaf_offs,
                                           const void* const* h_fill, const uint64_t* h_first, const uint64_t* h_cap,
                                           uint8_t* d_class, void* d_index, uint64_t index_bytes, uint64_t* d_counts,
                                           uint64_t* d_ends, srpc_unpack_status* d_status, void* d_scratch,
                                           uint64_t scratch_bytes, void* stream) {
    return mv_unpack_requests(true, req_plans, nplans, d_buf, buf_len, d_offs, nframes, d_cols, d_str_offs,
                              h_str_cap, d_recs, h_stride, h_leaf_offs, h_fill, h_first, h_cap, d_class, d_index,
                              index_bytes, d_counts, d_ends, d_status, d_scratch, scratch_bytes, stream);
}

int srpc_frames_unpack_requests_mixed_var(const srpc_plan* const* req_plans, int nplans, const uint8_t* d_buf,
                                          uint64_t buf_len, const uint32_t* d_offs, uint64_t nframes,
                                          void* const* const* d_cols, uint64_t* const* const* d_str_offs,
                                          const uint64_t* const* h_str_cap, const uint64_t* h_first,
                                          const uint64_t* h_cap, uint8_t* d_class, void* d_index, uint64_t index_bytes,
                                          uint64_t* d_counts, uint64_t* d_ends, srpc_unpack_status* d_status,
                                          void* d_scratch, uint64_t scratch_bytes, void* stream) {
    return mv_unpack_requests(false, req_plans, nplans, d_buf, buf_len, d_offs, nframes, d_cols, d_str_offs,
                              h_str_cap, nullptr, nullptr, nullptr, nullptr, h_first, h_cap, d_class, d_index, index_bytes,
                              d_counts, d_ends, d_status, d_scratch, scratch_bytes, stream);
}

}  // extern "C"
