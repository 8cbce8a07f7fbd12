// mixed_aos.hip -- batches of calls of several methods in caller-given order,
// each plan's calls held as one device array of the caller's own structs
// (srpc_frames_pack_requests_mixed_aos, srpc_frames_unpack_replies_mixed_aos of
// include/srpc_gpu.h): the struct-array form of mixed.hip's two calls.
//
// The index, mix_ranks, the tile, the granule's byte offset, the LDS lookups by
// a lane's own plan, the prefix templates and the image are mixed.hip's
// (mixed_common.h); only the field step differs.  The slices and the piece
// step of the decode are shared with the request decode (mixed_aos_common.h).
//
//   k_mixed_pack_aos    mix_pack_tile<true>: a lane's leaves come from
//       recs[k] + e * stride[k] + loff[f]; lanes of one plan hold consecutive
//       ranks, so their structs are adjacent in memory.
//   k_mixed_unpack_aos  stage, rank and judge as k_mixed_unpack (req_stage,
//       mix_judge); each lane leaves pos[j] -- its frame's image position,
//       "outside the image" or "leaves are zero".  Within a tile the good calls
//       of plan k are consecutive ranks, so they are one contiguous slice of plan
//       k's array: per-wave ballots leave its first element and count, and every
//       lane its slot (slice position -> lane).  The workgroup then takes
//       (plan, 16-byte piece) pairs over the K slices: a piece is assembled run
//       by run through plan k's per-struct-byte table, as k_unpack_replies_aos
//       does (aos_pieces.h), from the image at the frame's position, zero, or plan
//       k's fill, and stored whole.  A slice starts and ends at any byte: its
//       first and last piece, where they are shared with a neighbouring tile's
//       slice (or lie at the array's edge), are stored bytewise, own bytes only.
//       Every struct byte of a good call is written exactly once, none is read.
//
// The K tables and fills (up to 12.5 KiB) do not fit kernel arguments: they go
// to the head of caller scratch by mix_upload's by-value chunk launches and
// every workgroup copies them to LDS with 16-byte loads.
// LDS of the decode: image[a.img + 32] | lo[T + 1] (8-byte padded) | the K
//   prefixes | pos[T] | slot[T] (u16) | 16-byte aligned: tab_k[S16_k] (u16) ... |
//   fill_k[S16_k + 16] ..., then static wcnt, the lookups and the slices.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "aos_pieces.h"
#include "mixed_aos_common.h"
#include "mixed_common.h"
#include "mixed_var_common.h"
#include "plan.h"
#include "srpc_gpu.h"

namespace srpc_impl {
namespace {

struct MixAosStride {
    uint32_t stride[kMixPlans];
};

inline size_t mix_aos_lds(const MixArgs& a, uint32_t tb, uint32_t desc_bytes) {
    const size_t head = a.img + 32 + ((4 * (a.T + 1) + 7) & ~7u) + tb + 4 * a.T + 2 * a.T;
    return ((head + 15) & ~size_t{15}) + desc_bytes;
}

__global__ __launch_bounds__(kBlock) void k_mixed_pack_aos(MixArgs a, MixAosStride x, const uint8_t* __restrict__ method,
                                                           const uint32_t* __restrict__ table, uint64_t rows,
                                                           uint64_t ncalls, uint8_t* __restrict__ out,
                                                           uint32_t* __restrict__ offs, srpc_unpack_status* st) {
    mix_pack_tile<true>(a, x.stride, method, table, rows, ncalls, out, offs, st);
}

__global__ __launch_bounds__(kBlock) void k_mixed_unpack_aos(MixArgs a, MixAos x, const uint4* __restrict__ desc,
                                                             const uint8_t* __restrict__ method,
                                                             const uint32_t* __restrict__ table, uint64_t rows,
                                                             uint64_t ncalls, const uint8_t* __restrict__ buf,
                                                             uint64_t buf_len, const uint32_t* __restrict__ offs,
                                                             uint64_t nframes, uint32_t unanswered,
                                                             uint8_t* __restrict__ codes, srpc_unpack_status* st) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    __shared__ uint32_t wcnt[kMixLds];
    __shared__ MixLds d;
    __shared__ MixAosSlices sl;
    const uint32_t K = a.nplans;
    const uint32_t lo_bytes = (4 * (a.T + 1) + 7) & ~7u;
    const uint32_t tb = a.tmpl[K - 1] + ((a.prefix_len[K - 1] + 7) & ~7u);
    uint8_t* img = lds;
    uint32_t* lo = reinterpret_cast<uint32_t*>(lds + a.img + 32);
    uint8_t* tmpl = lds + a.img + 32 + lo_bytes;
    uint32_t* pos = reinterpret_cast<uint32_t*>(tmpl + tb);
    uint16_t* slot = reinterpret_cast<uint16_t*>(pos + a.T);
    uint8_t* dsc = lds + ((a.img + 32 + lo_bytes + tb + 6 * a.T + 15) & ~15u);

    mix_lds_fill(d, a);
    mix_templates(tmpl, a);
    mix_aos_slices_init(sl, x, K);
    for (uint32_t c = threadIdx.x; c < x.desc_bytes / 16; c += kBlock) reinterpret_cast<uint4*>(dsc)[c] = desc[c];
    const uint64_t c0 = static_cast<uint64_t>(blockIdx.x) * a.T;
    const uint64_t g = c0 / kMixGranule;
    const uint32_t j0 = static_cast<uint32_t>(c0 - g * kMixGranule);
    const uint64_t i = g * kMixGranule + threadIdx.x;
    const uint32_t nr = c0 < nframes ? static_cast<uint32_t>(min<uint64_t>(a.T, nframes - c0)) : 0;
    req_offsets(lo, a.T, offs, nframes, c0, buf_len);

    const MixLane r = mix_ranks(method, ncalls, K, table, rows, g, wcnt);  // barrier: lo[] and the slices' init are complete
    const bool mine = threadIdx.x >= j0 && threadIdx.x < j0 + a.T && i < ncalls;
    const bool good = mine && r.cls < K && r.rank < d.room[r.cls];
    const uint32_t j = threadIdx.x - j0;

    // the tile's slices: good calls of one plan are consecutive ranks, ascending with the lane
    mix_aos_slices_count(sl, K, r, good);

    // 1. the span of the tile's frames -> image, from a 16-byte boundary (ends with a barrier)
    const ReqSpan sp = req_stage(img, lo, nr, a.img, buf, buf_len);

    // 2. a lane per call: judge its frame, store its code, leave where its leaves are
    if (mine) {
        const MixReply y = mix_judge(d, r, good, j, nr, lo, img, tmpl, sp, buf, buf_len, unanswered);
        codes[i] = static_cast<uint8_t>(y.code);
        if (y.flag && st) report_bad(st, y.flag, i);
        pos[j] = !y.decoded ? kPosZero : y.in_img ? y.q : kPosGlobal;
    }

    // 3. image, zero and fill -> the slices, one lane per (plan, 16-byte piece)
    mix_aos_store<true>(sl, d, K, r, good, j, img, lo, pos, slot, dsc, buf);
}

}  // namespace
}  // namespace srpc_impl

using namespace srpc_impl;

extern "C" {

int srpc_frames_mixed_aos_scratch_bytes(const srpc_plan* const* plans, int nplans, const uint64_t* h_stride,
                                        uint64_t* out) {
    if (any_null(plans, h_stride, out) || mix_nplans_bad(nplans)) return SRPC_E_INVALID;
    for (int k = 0; k < nplans; ++k)
        if (h_stride[k] == 0) return SRPC_E_INVALID;
    uint32_t fmax = 0;
    if (int rc = mix_plans_ok(plans, nplans, 4, &fmax)) return rc;
    for (int k = 0; k < nplans; ++k)
        if (h_stride[k] > kAosMaxStride) return SRPC_E_UNSUPPORTED;
    *out = aos_desc_bytes(h_stride, nplans);
    return SRPC_OK;
}

int srpc_frames_mixed_aos_tile(const srpc_plan* const* plans, int nplans, const uint64_t* h_stride,
                               uint32_t* calls_per_tile) {
    if (any_null(plans, h_stride, calls_per_tile) || mix_nplans_bad(nplans)) return SRPC_E_INVALID;
    for (int k = 0; k < nplans; ++k)
        if (h_stride[k] == 0) return SRPC_E_INVALID;
    uint32_t fmax = 0;
    if (int rc = mix_plans_ok(plans, nplans, 4, &fmax)) return rc;
    for (int k = 0; k < nplans; ++k)
        if (h_stride[k] > kAosMaxStride) return SRPC_E_UNSUPPORTED;
    *calls_per_tile = mix_aos_tile(fmax, aos_desc_bytes(h_stride, nplans));
    return SRPC_OK;
}

int srpc_frames_pack_requests_mixed_aos(const srpc_plan* const* req_plans, int nplans, const void* const* d_recs,
                                        const uint64_t* h_stride, const uint32_t* const* h_leaf_offs,
                                        const uint64_t* h_first, const uint64_t* h_cap, const uint8_t* d_method,
                                        const void* d_index, uint64_t ncalls, uint8_t* d_out, uint64_t out_cap,
                                        uint32_t* d_offs, srpc_unpack_status* d_status, void* stream) {
    const TimedCall timed;
    // the arguments themselves are checked before any plan is read
    if (any_null(req_plans, d_recs, h_stride, h_leaf_offs, h_cap, d_index) ||
        mix_nplans_bad(nplans) || past_u32(ncalls) || (ncalls && any_null(d_method, d_out)))
        return SRPC_E_INVALID;
    if (aos_args_invalid(d_recs, h_stride, h_leaf_offs, h_first, h_cap, nplans)) return SRPC_E_INVALID;
    uint32_t fmax = 0;
    if (int rc = mix_plans_ok(req_plans, nplans, 4, &fmax)) return rc;
    for (int k = 0; k < nplans; ++k)
        if (int rc = aos_leaves_ok(req_plans[k], h_leaf_offs[k], h_stride[k])) return rc;
    if (!aligned(d_out, 16) || !aligned(d_index, 8) || !aligned(d_offs, 4)) return SRPC_E_ALIGN;
    if (!aos_recs_aligned(req_plans, nplans, d_recs, h_stride, h_leaf_offs)) return SRPC_E_ALIGN;
    AosCols cols;
    aos_cols(req_plans, nplans, d_recs, h_leaf_offs, &cols);
    MixArgs a{};
    MixAosStride x{};
    uint32_t tb = 0;
    if (int rc = mix_args(req_plans, nplans, cols.plan, h_first, h_cap, fmax, &a, &tb, 1)) return rc;
    for (int k = 0; k < nplans; ++k) x.stride[k] = static_cast<uint32_t>(h_stride[k]);
    if (out_cap < ncalls * fmax) return SRPC_E_CAPACITY;
    if (d_offs && ncalls * fmax >= (1ull << 32)) return SRPC_E_INVALID;  // u32 offsets
    const uint32_t grid = static_cast<uint32_t>(std::max<uint64_t>(1, (ncalls + a.T - 1) / a.T));
    launch(k_mixed_pack_aos, dim3(grid), dim3(kBlock), a.img + tb + 16, static_cast<hipStream_t>(stream), a, x, d_method,
           static_cast<const uint32_t*>(d_index), mix_rows(ncalls), ncalls, d_out, d_offs, d_status);
    return hipGetLastError() == hipSuccess ? SRPC_OK : SRPC_E_HIP;
}

int srpc_frames_unpack_replies_mixed_aos(const srpc_plan* const* reply_plans, int nplans, const uint8_t* d_buf,
                                         uint64_t buf_len, const uint32_t* d_offs, uint64_t nframes,
                                         const uint8_t* d_method, const void* d_index, uint64_t ncalls,
                                         uint8_t unanswered_code, void* const* d_recs, const uint64_t* h_stride,
                                         const uint32_t* const* h_leaf_offs, const void* const* h_fill,
                                         const uint64_t* h_first, const uint64_t* h_cap, uint8_t* d_codes,
                                         srpc_unpack_status* d_status, void* d_scratch, uint64_t scratch_bytes,
                                         void* stream) {
    const TimedCall timed;
    if (any_null(reply_plans, d_recs, h_stride, h_leaf_offs, h_fill, h_cap, d_index, d_codes, d_scratch) ||
        mix_nplans_bad(nplans) || nframes > ncalls || past_u32(buf_len) || past_u32(ncalls) ||
        (ncalls && !d_method) || (nframes && any_null(d_buf, d_offs)))
        return SRPC_E_INVALID;
    if (aos_args_invalid(d_recs, h_stride, h_leaf_offs, h_first, h_cap, nplans)) return SRPC_E_INVALID;
    for (int k = 0; k < nplans; ++k)
        if (!h_fill[k]) return SRPC_E_INVALID;
    uint32_t fmax = 0;
    if (int rc = mix_plans_ok(reply_plans, nplans, 5, &fmax)) return rc;
    for (int k = 0; k < nplans; ++k)
        if (h_stride[k] > kAosMaxStride) return SRPC_E_UNSUPPORTED;
    // the tables and the fills, as they will lie in scratch and in LDS
    AosDesc desc;
    MixAos x{};
    if (int rc = aos_describe(reply_plans, nplans, d_recs, h_stride, h_leaf_offs, h_fill, &desc, &x)) return rc;
    if (!aligned(d_buf, 16) || !aligned(d_index, 8) || !aligned(d_offs, 4) || !aligned(d_scratch, 16)) return SRPC_E_ALIGN;
    if (!aos_recs_aligned(reply_plans, nplans, d_recs, h_stride, h_leaf_offs)) return SRPC_E_ALIGN;
    if (scratch_bytes < x.desc_bytes) return SRPC_E_CAPACITY;
    AosCols cols;
    aos_cols(reply_plans, nplans, d_recs, h_leaf_offs, &cols);
    MixArgs a{};
    uint32_t tb = 0;
    if (int rc = mix_args(reply_plans, nplans, cols.plan, h_first, h_cap, fmax, &a, &tb, 1)) return rc;
    a.T = mix_aos_tile(fmax, x.desc_bytes);
    a.img = (a.T * fmax + 16 + 15) & ~15u;
    auto s = static_cast<hipStream_t>(stream);
    if (d_status && status_reset_launch(d_status, s)) return SRPC_E_HIP;
    if (!ncalls) return SRPC_OK;
    if (int rc = mix_upload(desc.bytes, x.desc_bytes, d_scratch, s)) return rc;
    const uint32_t grid = static_cast<uint32_t>((ncalls + a.T - 1) / a.T);
    launch(k_mixed_unpack_aos, dim3(grid), dim3(kBlock), static_cast<uint32_t>(mix_aos_lds(a, tb, x.desc_bytes)), s, a, x,
           static_cast<const uint4*>(d_scratch), d_method, static_cast<const uint32_t*>(d_index), mix_rows(ncalls), ncalls,
           d_buf, buf_len, d_offs, nframes, static_cast<uint32_t>(unanswered_code), d_codes, d_status);
    return hipGetLastError() == hipSuccess ? SRPC_OK : SRPC_E_HIP;
}

}  // extern "C"
