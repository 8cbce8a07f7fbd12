// mixed_legs.hip -- batches of calls of several methods in caller-given order,
// each plan's calls held in columns (fixed-size or string plans, as
// mixed_var.hip takes them) or in one device array of the caller's own structs
// (fixed-size plans, as mixed_aos.hip takes them), any combination in one batch
// (srpc_frames_pack_requests_mixed_legs, srpc_frames_unpack_replies_mixed_legs
// of include/srpc_gpu.h).  Plan k is a record plan exactly when h_stride[k] != 0.
//
// Nothing here is a second implementation: the description of the plans, the
// sizes, the scan, the slot scan and the char copy are mixed_var.hip's launches
// (mixed_var_common.h); the two kernels of this file are mixed_var.hip's tile
// kernels with LEGS = true (mixed_var_tile.h), whose record half is the slice
// and piece step of mixed_aos.hip (mixed_aos_common.h).
//
//   k_ml_pack    mv_pack_tile<true>: a record plan's leaf is a column whose
//       element step is the struct's stride, its base d_recs[k] + h_leaf_offs[k][f].
//   k_ml_parse   mv_parse_tile<true>: lanes of column plans store their fields
//       and string lengths; lanes of record plans leave pos[j], and the
//       workgroup writes the record plans' slices as whole 16-byte pieces.
//
// A batch without a record plan is mixed_var.hip's problem and launches its
// kernels (mv_pack_launch, mv_parse_launch): k_ml_parse keeps more scalars live
// across the slice steps than k_mv_parse and is slower for column lanes too.
//
// Scratch: mixed_var.hip's layout (mv_scratch), rounded up to 16 bytes, then the
// record plans' tables and fills (aos_describe over the record plans alone,
// 3 S16 + 16 bytes each), uploaded by mix_upload.
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

}  // namespace
}  // namespace srpc_impl

using namespace srpc_impl;

extern "C" {

int srpc_frames_mixed_legs_scratch_bytes(const srpc_plan* const* plans, int nplans, const uint64_t* h_stride,
                                         uint64_t ncalls, uint64_t* out) {
    if (!plans || !out || nplans <= 0 || nplans > kMixPlans || ncalls >= (1ull << 32)) return SRPC_E_INVALID;
    if (h_stride)
        for (int k = 0; k < nplans; ++k)
            if (h_stride[k] >= (1ull << 32)) return SRPC_E_INVALID;
    MvDesc d{};
    if (int rc = mv_plans(plans, nplans, 4, &d)) return rc;
    if (int rc = legs_plans_ok(plans, nplans, h_stride, false)) return rc;
    uint64_t tables = 0;  // a stride above what a decode takes is a pack's: no table
    if (h_stride)
        for (int k = 0; k < nplans; ++k)
            if (h_stride[k] && h_stride[k] <= kAosMaxStride) tables += aos_desc_bytes(h_stride + k, 1);
    *out = legs_tables_at(mv_scratch(d, ncalls)) + tables;
    return SRPC_OK;
}

int srpc_frames_mixed_legs_tile(const srpc_plan* const* plans, int nplans, const uint64_t* h_stride,
                                uint32_t* calls_per_tile, uint32_t* image_bytes) {
    if (!plans || !calls_per_tile || !image_bytes || nplans <= 0 || nplans > kMixPlans) return SRPC_E_INVALID;
    if (h_stride)
        for (int k = 0; k < nplans; ++k)
            if (h_stride[k] >= (1ull << 32)) return SRPC_E_INVALID;
    MvDesc d{};
    if (int rc = mv_plans(plans, nplans, 4, &d)) return rc;
    if (int rc = legs_plans_ok(plans, nplans, h_stride, true)) return rc;
    uint32_t tables = 0;
    if (h_stride)
        for (int k = 0; k < nplans; ++k)
            if (h_stride[k]) tables += aos_desc_bytes(h_stride + k, 1);
    *image_bytes = kMixImage - tables;
    *calls_per_tile = mix_tile(legs_fmax(d), kMixImage - tables);
    return SRPC_OK;
}

int srpc_frames_pack_requests_mixed_legs(const srpc_plan* const* req_plans, int nplans, const void* const* const* d_cols,
                                         const uint64_t* const* const* d_str_offs, const void* const* d_recs,
                                         const uint64_t* h_stride, const uint32_t* const* h_leaf_offs,
                                         const uint64_t* h_first, const uint64_t* h_cap, const uint8_t* d_method,
                                         const void* d_index, uint64_t ncalls, uint8_t* d_out, uint64_t out_cap,
                                         uint32_t* d_offs, uint64_t* d_total, srpc_unpack_status* d_status,
                                         void* d_scratch, uint64_t scratch_bytes, void* stream) {
    const TimedCall timed;
    // the arguments themselves are checked before any plan is read
    if (!req_plans || !d_cols || !d_str_offs || !d_recs || !h_stride || !h_leaf_offs || !h_cap || !d_index || !d_offs ||
        !d_total || !d_scratch || nplans <= 0 || nplans > kMixPlans || ncalls >= (1ull << 32) ||
        out_cap >= (1ull << 32) || (ncalls && (!d_method || !d_out)))
        return SRPC_E_INVALID;
    if (legs_args_invalid(d_recs, h_stride, h_leaf_offs, nullptr, false, h_first, h_cap, nplans)) return SRPC_E_INVALID;
    static thread_local MvDesc d;
    d = MvDesc{};
    if (int rc = mv_plans(req_plans, nplans, 4, &d)) return rc;
    if (int rc = legs_plans_ok(req_plans, nplans, h_stride, false)) return rc;
    for (int k = 0; k < nplans; ++k)
        if (h_stride[k])
            if (int rc = aos_leaves_ok(req_plans[k], h_leaf_offs[k], h_stride[k])) return rc;
    if (!aligned(d_out, 16) || !aligned(d_index, 8) || !aligned(d_scratch, 16) || !aligned(d_total, 8) ||
        !aligned(d_offs, 4))
        return SRPC_E_ALIGN;
    for (int k = 0; k < nplans; ++k)
        if (h_stride[k] && (!aligned(d_recs[k], 16) || !aos_layout_aligned(req_plans[k], h_leaf_offs[k], h_stride[k])))
            return SRPC_E_ALIGN;
    if (int rc = mv_cols(req_plans, nplans, d_cols, d_str_offs, nullptr, h_first, h_cap, &d, h_stride)) return rc;
    legs_cols(req_plans, nplans, const_cast<void* const*>(d_recs), h_stride, h_leaf_offs, &d);
    const MvScratch sc = mv_scratch(d, ncalls);
    if (scratch_bytes < sc.bytes) return SRPC_E_CAPACITY;
    MvLegs x{};
    bool any_rec = false;
    for (int k = 0; k < nplans; ++k) {
        x.x.stride[k] = static_cast<uint32_t>(h_stride[k]);
        any_rec = any_rec || h_stride[k];
    }
    x.window = kMixImage;
    auto s = static_cast<hipStream_t>(stream);
    auto* base = static_cast<uint8_t*>(d_scratch);
    const auto* dd = reinterpret_cast<const MvDesc*>(base);
    auto* gsum = reinterpret_cast<uint64_t*>(base + sc.gsum);
    const auto* table = static_cast<const uint32_t*>(d_index);
    const uint64_t rows = mix_rows(ncalls);
    if (int rc = mv_upload(d, d_scratch, s)) return rc;
    mv_sizes_launch(dd, d_method, table, rows, ncalls, gsum, out_cap, d_offs, d_total, s);
    // without a record plan the batch is mixed_var.hip's, and so is the kernel: kind-awareness costs it nothing
    if (ncalls && !any_rec) mv_pack_launch(d, dd, d_method, table, rows, ncalls, gsum, d_out, out_cap, d_offs, d_status, s);
    else if (ncalls)
        launch(k_ml_pack, dim3(static_cast<uint32_t>((ncalls + d.T - 1) / d.T)), dim3(kBlock), mv_lds(d), s, dd, x,
               d_method, table, rows, ncalls, gsum, d_out, out_cap, d_offs, d_status);
    return hipGetLastError() == hipSuccess ? SRPC_OK : SRPC_E_HIP;
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
    const TimedCall timed;
    if (!reply_plans || !d_cols || !d_str_offs || !h_str_cap || !d_recs || !h_stride || !h_leaf_offs || !h_fill ||
        !h_cap || !d_index || !d_codes || !d_ends || !d_scratch || nplans <= 0 || nplans > kMixPlans ||
        nframes > ncalls || buf_len >= (1ull << 32) || ncalls >= (1ull << 32) || (ncalls && !d_method) ||
        (nframes && (!d_buf || !d_offs)))
        return SRPC_E_INVALID;
    if (legs_args_invalid(d_recs, h_stride, h_leaf_offs, h_fill, true, h_first, h_cap, nplans)) return SRPC_E_INVALID;
    static thread_local MvDesc d;
    d = MvDesc{};
    if (int rc = mv_plans(reply_plans, nplans, 5, &d)) return rc;
    if (int rc = legs_plans_ok(reply_plans, nplans, h_stride, true)) return rc;
    // the record plans' tables and fills, as they will lie in scratch and in LDS
    LegRecs lr;
    leg_recs(reply_plans, nplans, d_recs, h_stride, h_leaf_offs, h_fill, &lr);
    AosDesc desc;
    MixAos xr{};
    if (lr.n)
        if (int rc = aos_describe(lr.plans, lr.n, lr.recs, lr.stride, lr.leaf_offs, lr.fill, &desc, &xr)) return rc;
    if (!aligned(d_buf, 16) || !aligned(d_index, 8) || !aligned(d_scratch, 16) || !aligned(d_ends, 8) ||
        !aligned(d_offs, 4))
        return SRPC_E_ALIGN;
    for (int k = 0; k < nplans; ++k)
        if (h_stride[k] && (!aligned(d_recs[k], 16) || !aos_layout_aligned(reply_plans[k], h_leaf_offs[k], h_stride[k])))
            return SRPC_E_ALIGN;
    if (int rc = mv_cols(reply_plans, nplans, reinterpret_cast<const void* const* const*>(d_cols),
                         reinterpret_cast<const uint64_t* const* const*>(d_str_offs), h_str_cap, h_first, h_cap, &d,
                         h_stride))
        return rc;
    legs_cols(reply_plans, nplans, d_recs, h_stride, h_leaf_offs, &d);
    MvLegs x{};
    for (int r = 0; r < lr.n; ++r) {
        const int k = lr.plan[r];
        x.x.recs[k] = xr.recs[r];
        x.x.stride[k] = xr.stride[r];
        x.x.tab[k] = xr.tab[r];
        x.x.fill[k] = xr.fill[r];
    }
    x.x.desc_bytes = xr.desc_bytes;
    x.window = kMixImage - xr.desc_bytes;
    d.T = mix_tile(legs_fmax(d), x.window);
    const MvScratch sc = mv_scratch(d, ncalls);
    const uint64_t tables_at = legs_tables_at(sc);
    if (scratch_bytes < tables_at + xr.desc_bytes) return SRPC_E_CAPACITY;
    auto s = static_cast<hipStream_t>(stream);
    auto* base = static_cast<uint8_t*>(d_scratch);
    const auto* dd = reinterpret_cast<const MvDesc*>(base);
    auto* counts = reinterpret_cast<uint32_t*>(base + sc.counts);
    auto* partial = reinterpret_cast<uint64_t*>(base + sc.partial);
    auto* srcs = reinterpret_cast<uint32_t*>(base + sc.srcs);
    const auto* table = static_cast<const uint32_t*>(d_index);
    const uint64_t rows = mix_rows(ncalls);
    if (d_status) mv_status_reset_launch(d_status, s);
    if (int rc = mv_upload(d, d_scratch, s)) return rc;
    if (xr.desc_bytes)
        if (int rc = mix_upload(desc.bytes, xr.desc_bytes, base + tables_at, s)) return rc;
    if (ncalls && !lr.n)
        mv_parse_launch(d, dd, d_method, table, rows, ncalls, d_buf, buf_len, d_offs, nframes,
                        static_cast<uint32_t>(unanswered_code), d_codes, srcs, counts, d_status, s);
    else if (ncalls)
        launch(k_ml_parse, dim3(static_cast<uint32_t>((ncalls + d.T - 1) / d.T)), dim3(kBlock), mv_lds(d), s, dd, x,
               reinterpret_cast<const uint4*>(base + tables_at), d_method, table, rows, ncalls, d_buf, buf_len, d_offs,
               nframes, static_cast<uint32_t>(unanswered_code), d_codes, srcs, counts, d_status);
    if (d.nslots) {
        mv_slots_launch(d, dd, counts, ncalls, partial, sc.nb, d_ends, s);
        if (ncalls) mv_copy_launch(dd, d_method, table, rows, ncalls, d_buf, srcs, s);
    }
    return hipGetLastError() == hipSuccess ? SRPC_OK : SRPC_E_HIP;
}

}  // extern "C"
