// mixed_legs.hip -- the client's string-aware batches of calls of several methods
// in caller-given order: one host path for the request pack and one for the
// reply decode (mv_pack_requests, mv_unpack_replies).  The entry points of
// include/srpc_gpu.h are adapters over them: srpc_frames_*_mixed_legs, where a
// plan's calls lie in columns (fixed-size or string plans) or in one device
// array of the caller's own structs (fixed-size plans; a record plan:
// h_stride[k] != 0), and srpc_frames_*_mixed_var, which has no record arguments.
// mixed_req_legs.hip holds the server's request decode in the same way.
//
// Nothing here is a second implementation: the description of the plans, the
// sizes, the scan, the slot scan and the char copy are mixed_var.hip's launches
// (mixed_var_common.h), the record plans' checks and description
// mixed_legs_common.h's, and the two kernels mixed_var.hip's tile kernels with
// LEGS = true (mixed_var_tile.h): a record plan's leaf is a column whose element
// step is the struct's stride (k_ml_pack); lanes of record plans leave pos[j]
// and the workgroup writes their slices as whole 16-byte pieces (k_ml_parse,
// mixed_aos_common.h).  A batch without a record plan launches k_mv_pack /
// k_mv_parse themselves: k_ml_parse keeps more scalars live across the slice
// steps and is slower for column lanes too.
//
// Scratch: mv_scratch's layout, rounded up to 16 bytes, then the record plans'
// tables and fills (3 S16 + 16 bytes each), uploaded by mix_upload.
// LDS of the decode: image[W + 16] | tables and fills [desc_bytes] | templates at
// kMixImage + 16, W = kMixImage - desc_bytes: the dynamic LDS of k_mv_parse.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "aos_pieces.h"
#include "mixed_aos_common.h"
#include "mixed_common.h"
#include "mixed_legs_common.h"
#include "mixed_var_common.h"
#include "mixed_var_tile.h"
#include "plan.h"
#include "srpc_gpu.h"

namespace srpc_impl {
namespace {

__global__ __launch_bounds__(kBlock) void k_ml_pack(const MvDesc* __restrict__ d, MvLegs x,
                                                    const uint8_t* __restrict__ method,
                                                    const uint32_t* __restrict__ table, uint64_t rows, uint64_t ncalls,
                                                    const uint64_t* __restrict__ gsum, uint8_t* __restrict__ out,
                                                    uint64_t out_cap, uint32_t* __restrict__ offs,
                                                    srpc_unpack_status* st) {
    mv_pack_tile<true>(d, &x, method, table, rows, ncalls, gsum, out, out_cap, offs, st);
}

__global__ __launch_bounds__(kBlock) void k_ml_parse(const MvDesc* __restrict__ d, MvLegs x,
                                                     const uint4* __restrict__ desc, const uint8_t* __restrict__ method,
                                                     const uint32_t* __restrict__ table, uint64_t rows, uint64_t ncalls,
                                                     const uint8_t* __restrict__ buf, uint64_t buf_len,
                                                     const uint32_t* __restrict__ offs, uint64_t nframes,
                                                     uint32_t unanswered, uint8_t* __restrict__ codes,
                                                     uint32_t* __restrict__ srcs, uint32_t* __restrict__ counts,
                                                     srpc_unpack_status* st) {
    mv_parse_tile<true>(d, &x, desc, method, table, rows, ncalls, buf, buf_len, offs, nframes, unanswered, codes, srcs,
                        counts, st);
}

// The request pack.  legs: a _mixed_legs entry point called; a _mixed_var one
// passes nullptr for the record arguments.  What a caller sees of it, here and
// in the two decodes:
//   - _legs refuses a null record argument and checks the record plans
//     (legs_args_invalid, legs_plans_ok, aos_leaves_ok or legs_describe, then
//     each array's 16-byte and layout alignment);
//   - d_scratch must be aligned to 16 for _legs, to 8 for _var;
//   - a decode needs legs_tables_at(sc) + desc_bytes of scratch for _legs
//     (sc.bytes rounded up to 16, record plan or none), sc.bytes for _var.
// Either way the checks fire in one order, which decides the code of a call
// wrong in two ways: arguments, plans, the record plans' description, alignment,
// columns, capacity.  The kernels depend on the batch having a record plan only.
int mv_pack_requests(bool legs, const srpc_plan* const* req_plans, int nplans, const void* const* const* d_cols,
                     const uint64_t* const* const* d_str_offs, const void* const* d_recs, const uint64_t* h_stride,
                     const uint32_t* const* h_leaf_offs, const uint64_t* h_first, const uint64_t* h_cap,
                     const uint8_t* d_method, const void* d_index, uint64_t ncalls, uint8_t* d_out, uint64_t out_cap,
                     uint32_t* d_offs, uint64_t* d_total, srpc_unpack_status* d_status, void* d_scratch,
                     uint64_t scratch_bytes, void* stream) {
    const TimedCall timed;
    if (any_null(req_plans, d_cols, d_str_offs, h_cap, d_index, d_offs, d_total, d_scratch) ||
        mix_nplans_bad(nplans) || past_u32(ncalls) || (ncalls && any_null(d_method, d_out)) || past_u32(out_cap))
        return SRPC_E_INVALID;
    if (legs && legs_args_invalid(d_recs, h_stride, h_leaf_offs, nullptr, false, h_first, h_cap, nplans))
        return SRPC_E_INVALID;
    if (!legs) h_stride = kAllColumns;
    static thread_local MvDesc d;
    d = MvDesc{};
    if (int rc = mv_plans(req_plans, nplans, 4, &d)) return rc;
    if (int rc = legs_plans_ok(req_plans, nplans, h_stride, false)) return rc;
    for (int k = 0; k < nplans; ++k)
        if (h_stride[k])
            if (int rc = aos_leaves_ok(req_plans[k], h_leaf_offs[k], h_stride[k])) return rc;
    if (!aligned(d_out, 16) || !aligned(d_index, 8) || !aligned(d_scratch, legs ? 16 : 8) || !aligned(d_total, 8) ||
        !aligned(d_offs, 4) || !aos_recs_aligned(req_plans, nplans, d_recs, h_stride, h_leaf_offs))
        return SRPC_E_ALIGN;
    if (int rc = mv_cols(req_plans, nplans, d_cols, d_str_offs, nullptr, h_first, h_cap, &d, h_stride)) return rc;
    legs_cols(req_plans, nplans, const_cast<void* const*>(d_recs), h_stride, h_leaf_offs, &d);
    const MvScratch sc = mv_scratch(d, ncalls);
    if (scratch_bytes < sc.bytes) return SRPC_E_CAPACITY;
    MvLegs x{};
    x.window = kMixImage;
    for (int k = 0; k < nplans; ++k) x.x.stride[k] = static_cast<uint32_t>(h_stride[k]);
    const bool any_rec = std::any_of(h_stride, h_stride + nplans, [](uint64_t v) { return v != 0; });
    auto s = static_cast<hipStream_t>(stream);
    const MvCarve c(d_scratch, sc);
    const auto* table = static_cast<const uint32_t*>(d_index);
    const uint64_t rows = mix_rows(ncalls);
    if (int rc = mix_upload(&d, sizeof d, d_scratch, s)) return rc;
    mv_sizes_launch(c.dd, d_method, table, rows, ncalls, c.gsum, out_cap, d_offs, d_total, s);
    // without a record plan the kernel is mixed_var.hip's: kind-awareness costs the batch nothing
    if (ncalls && !any_rec)
        mv_pack_launch(d, c.dd, d_method, table, rows, ncalls, c.gsum, d_out, out_cap, d_offs, d_status, s);
    else if (ncalls)
        launch(k_ml_pack, dim3(static_cast<uint32_t>((ncalls + d.T - 1) / d.T)), dim3(kBlock), mv_lds(d), s, c.dd, x,
               d_method, table, rows, ncalls, c.gsum, d_out, out_cap, d_offs, d_status);
    return hipGetLastError() == hipSuccess ? SRPC_OK : SRPC_E_HIP;
}

// The reply decode: `legs` as at mv_pack_requests.
int mv_unpack_replies(bool legs, const srpc_plan* const* reply_plans, int nplans, const uint8_t* d_buf,
                      uint64_t buf_len, const uint32_t* d_offs, uint64_t nframes, const uint8_t* d_method,
                      const void* d_index, uint64_t ncalls, uint8_t unanswered_code, void* const* const* d_cols,
                      uint64_t* const* const* d_str_offs, const uint64_t* const* h_str_cap, void* const* d_recs,
                      const uint64_t* h_stride, const uint32_t* const* h_leaf_offs, const void* const* h_fill,
                      const uint64_t* h_first, const uint64_t* h_cap, uint8_t* d_codes, uint64_t* d_ends,
                      srpc_unpack_status* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream) {
    const TimedCall timed;
    if (any_null(reply_plans, d_cols, d_str_offs, h_str_cap, h_cap, d_index, d_codes, d_ends, d_scratch) ||
        mix_nplans_bad(nplans) || nframes > ncalls || past_u32(buf_len) || past_u32(ncalls) ||
        (ncalls && !d_method) || (nframes && any_null(d_buf, d_offs)))
        return SRPC_E_INVALID;
    if (legs && legs_args_invalid(d_recs, h_stride, h_leaf_offs, h_fill, true, h_first, h_cap, nplans))
        return SRPC_E_INVALID;
    if (!legs) h_stride = kAllColumns;
    static thread_local MvDesc d;
    d = MvDesc{};
    if (int rc = mv_plans(reply_plans, nplans, 5, &d)) return rc;
    if (int rc = legs_plans_ok(reply_plans, nplans, h_stride, true)) return rc;
    LegsTables t;
    if (int rc = legs_describe(reply_plans, nplans, d_recs, h_stride, h_leaf_offs, h_fill, &d, &t)) return rc;
    if (!aligned(d_buf, 16) || !aligned(d_index, 8) || !aligned(d_scratch, legs ? 16 : 8) || !aligned(d_ends, 8) ||
        !aligned(d_offs, 4) || !aos_recs_aligned(reply_plans, nplans, d_recs, h_stride, h_leaf_offs))
        return SRPC_E_ALIGN;
    if (int rc = mv_cols(reply_plans, nplans, reinterpret_cast<const void* const* const*>(d_cols),
                         reinterpret_cast<const uint64_t* const* const*>(d_str_offs), h_str_cap, h_first, h_cap, &d,
                         h_stride))
        return rc;
    legs_cols(reply_plans, nplans, d_recs, h_stride, h_leaf_offs, &d);
    const MvScratch sc = mv_scratch(d, ncalls);
    const uint64_t tables_at = legs_tables_at(sc);
    if (scratch_bytes < (legs ? tables_at + t.x.x.desc_bytes : sc.bytes)) return SRPC_E_CAPACITY;
    auto s = static_cast<hipStream_t>(stream);
    const MvCarve c(d_scratch, sc);
    auto* tables = static_cast<uint8_t*>(d_scratch) + tables_at;
    const auto* table = static_cast<const uint32_t*>(d_index);
    const uint64_t rows = mix_rows(ncalls);
    if (d_status && status_reset_launch(d_status, s)) return SRPC_E_HIP;
    if (int rc = mix_upload(&d, sizeof d, d_scratch, s)) return rc;
    if (t.x.x.desc_bytes)
        if (int rc = mix_upload(t.desc.bytes, t.x.x.desc_bytes, tables, s)) return rc;
    if (ncalls && !t.x.x.desc_bytes)
        mv_parse_launch(d, c.dd, d_method, table, rows, ncalls, d_buf, buf_len, d_offs, nframes,
                        static_cast<uint32_t>(unanswered_code), d_codes, c.srcs, c.counts, d_status, s);
    else if (ncalls)
        launch(k_ml_parse, dim3(static_cast<uint32_t>((ncalls + d.T - 1) / d.T)), dim3(kBlock), mv_lds(d), s, c.dd, t.x,
               reinterpret_cast<const uint4*>(tables), d_method, table, rows, ncalls, d_buf, buf_len, d_offs, nframes,
               static_cast<uint32_t>(unanswered_code), d_codes, c.srcs, c.counts, d_status);
    return mv_strings_launch(d, c, sc.nb, d_method, table, ncalls, d_buf, d_ends, s);
}

}  // namespace
}  // namespace srpc_impl

using namespace srpc_impl;

extern "C" {

int srpc_frames_mixed_legs_scratch_bytes(const srpc_plan* const* plans, int nplans, const uint64_t* h_stride,
                                         uint64_t ncalls, uint64_t* out) {
    if (any_null(plans, out) || mix_nplans_bad(nplans) || past_u32(ncalls)) return SRPC_E_INVALID;
    MvDesc d{};
    if (int rc = legs_query_plans(plans, nplans, h_stride, false, &d)) return rc;
    *out = legs_tables_at(mv_scratch(d, ncalls)) + aos_desc_bytes(h_stride ? h_stride : kAllColumns, nplans);
    return SRPC_OK;
}

int srpc_frames_mixed_legs_tile(const srpc_plan* const* plans, int nplans, const uint64_t* h_stride,
                                uint32_t* calls_per_tile, uint32_t* image_bytes) {
    if (any_null(plans, calls_per_tile, image_bytes) || mix_nplans_bad(nplans)) return SRPC_E_INVALID;
    MvDesc d{};
    if (int rc = legs_query_plans(plans, nplans, h_stride, true, &d)) return rc;
    MvLegs x{};
    legs_window(aos_desc_bytes(h_stride ? h_stride : kAllColumns, nplans), &d, &x);
    *image_bytes = x.window;
    *calls_per_tile = d.T;
    return SRPC_OK;
}

int srpc_frames_pack_requests_mixed_legs(const srpc_plan* const* req_plans, int nplans, const void* const* const* d_cols,
                                         const uint64_t* const* const* d_str_offs, const void* const* d_recs,
                                         const uint64_t* h_stride, const uint32_t* const* h_leaf_offs,
                                         const uint64_t* h_first, const uint64_t* h_cap, const uint8_t* d_method,
                                         const void* d_index, uint64_t ncalls, uint8_t* d_out, uint64_t out_cap,
                                         uint32_t* d_offs, uint64_t* d_total, srpc_unpack_status* d_status,
                                         void* d_scratch, uint64_t scratch_bytes, void* stream) {
    return mv_pack_requests(true, req_plans, nplans, d_cols, d_str_offs, d_recs, h_stride, h_leaf_offs, h_first,
                            h_cap, d_method, d_index, ncalls, d_out, out_cap, d_offs, d_total, d_status, d_scratch,
                            scratch_bytes, stream);
}

int srpc_frames_unpack_replies_mixed_legs(const srpc_plan* const* reply_plans, int nplans, const uint8_t* d_buf,
                                          uint64_t buf_len, const uint32_t* d_offs, uint64_t nframes,
                                          const uint8_t* d_method, const void* d_index, uint64_t ncalls,
                                          uint8_t unanswered_code, void* const* const* d_cols,
                                          uint64_t* const* const* d_str_offs, const uint64_t* const* h_str_cap,
                                          void* const* d_recs, const uint64_t* h_stride,
                                          const uint32_t* const* h_leaf_offs, const void* const* h_fill,
                                          const uint64_t* h_first, const uint64_t* h_cap, uint8_t* d_codes,
                                          uint64_t* d_ends, srpc_unpack_status* d_status, void* d_scratch,
                                          uint64_t scratch_bytes, void* stream) {
    return mv_unpack_replies(true, reply_plans, nplans, d_buf, buf_len, d_offs, nframes, d_method, d_index,
                             ncalls, unanswered_code, d_cols, d_str_offs, h_str_cap, d_recs, h_stride, h_leaf_offs, h_fill,
                             h_first, h_cap, d_codes, d_ends, d_status, d_scratch, scratch_bytes, stream);
}

int srpc_frames_mixed_var_scratch_bytes(const srpc_plan* const* plans, int nplans, uint64_t ncalls, uint64_t* out) {
    if (any_null(plans, out) || mix_nplans_bad(nplans) || past_u32(ncalls)) return SRPC_E_INVALID;
    MvDesc d{};
    if (int rc = mv_plans(plans, nplans, 4, &d)) return rc;
    *out = mv_scratch(d, ncalls).bytes;
    return SRPC_OK;
}

int srpc_frames_mixed_var_tile(const srpc_plan* const* plans, int nplans, uint32_t* calls_per_tile,
                               uint32_t* image_bytes) {
    return srpc_frames_mixed_legs_tile(plans, nplans, nullptr, calls_per_tile, image_bytes);
}

int srpc_frames_pack_requests_mixed_var(const srpc_plan* const* req_plans, int nplans, const void* const* const* d_cols,
                                        const uint64_t* const* const* d_str_offs, const uint64_t* h_first,
                                        const uint64_t* h_cap, const uint8_t* d_method, const void* d_index,
                                        uint64_t ncalls, uint8_t* d_out, uint64_t out_cap, uint32_t* d_offs,
                                        uint64_t* d_total, srpc_unpack_status* d_status, void* d_scratch,
                                        uint64_t scratch_bytes, void* stream) {
    return mv_pack_requests(false, req_plans, nplans, d_cols, d_str_offs, nullptr, nullptr, nullptr, h_first, h_cap,
                            d_method, d_index, ncalls, d_out, out_cap, d_offs, d_total, d_status, d_scratch, scratch_bytes,
                            stream);
}

int srpc_frames_unpack_replies_mixed_var(const srpc_plan* const* reply_plans, int nplans, const uint8_t* d_buf,
                                         uint64_t buf_len, const uint32_t* d_offs, uint64_t nframes,
                                         const uint8_t* d_method, const void* d_index, uint64_t ncalls,
                                         uint8_t unanswered_code, void* const* const* d_cols,
                                         uint64_t* const* const* d_str_offs, const uint64_t* const* h_str_cap,
                                         const uint64_t* h_first, const uint64_t* h_cap, uint8_t* d_codes,
                                         uint64_t* d_ends, srpc_unpack_status* d_status, void* d_scratch,
                                         uint64_t scratch_bytes, void* stream) {
    return mv_unpack_replies(false, reply_plans, nplans, d_buf, buf_len, d_offs, nframes, d_method, d_index, ncalls,
                             unanswered_code, d_cols, d_str_offs, h_str_cap, nullptr, nullptr, nullptr, nullptr, h_first,
                             h_cap, d_codes, d_ends, d_status, d_scratch, scratch_bytes, stream);
}

}  // extern "C"
