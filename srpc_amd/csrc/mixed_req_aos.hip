// mixed_req_aos.hip -- a batch of request frames of several methods decoded in
// arrival order into one device array of the caller's own structs per method
// (server side; srpc_frames_unpack_requests_mixed_aos of include/srpc_gpu.h):
// the struct-array form of mixed_req.hip's call and the server's mirror of
// mixed_aos.hip's request pack.
//
//   k_req_classify  (mixed_req.hip, as it is, with the column call's tile) and
//       the index over the class bytes (mixed.hip): d_class, d_index and
//       d_counts are the column call's.
//   k_req_decode_aos  the first half of k_req_decode -- a tile's offsets, the
//       granule's ranks from the index, the tile's span staged into the LDS
//       image -- and the second half of k_mixed_unpack_aos
//       (mixed_aos_common.h): a lane is good when its frame is the tile's, has a
//       class and an element; it leaves pos[j], its frame's image position or
//       "outside the image" (an oversize junk frame pushed it out of the stage:
//       it is then read from global memory, at most F_k bytes, its extent
//       checked again).  The good frames of plan k within a tile are consecutive
//       ranks, one contiguous slice of plan k's array, which the workgroup
//       writes as whole 16-byte pieces assembled from the image and the fill.
//       A classified frame is always one whole record: there is no "leaves are
//       zero" state, but for a class byte that the extent contradicts (never
//       what the first pass wrote), where no stream byte is read.
//
// The tile is mix_aos_tile: the K tables and fills (head of caller scratch,
// copied to LDS with 16-byte loads) are taken out of the image's 32 KiB, so a
// workgroup's LDS stays at the column kernel's ~33 KiB and four workgroups share
// a compute unit's LDS, as for k_mixed_unpack_aos.
// LDS of the decode: image[a.img + 32] | lo[T + 1] (8-byte padded) | pos[T] |
//   slot[T] (u16) | 16-byte aligned: tab_k[S16_k] (u16) ... | fill_k[S16_k + 16]
//   ..., then static wcnt, the lookups and the slices.  No prefix templates.
//
// Piece stores are non-temporal, as the reply decode's: measured against plain
// stores (-DSRPC_REQ_AOS_PLAIN) the call is 6 % faster and leaves more of the
// stream in cache for whoever reads it next.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "aos_pieces.h"
#include "mixed_aos_common.h"
#include "mixed_common.h"
#include "mixed_var_common.h"
#include "plan.h"
#include "srpc_gpu.h"

namespace srpc_impl {
namespace {

#ifdef SRPC_REQ_AOS_PLAIN
constexpr bool kReqAosNt = false;
#else
constexpr bool kReqAosNt = true;
#endif

inline uint32_t req_aos_head(const MixArgs& a) { return a.img + 32 + ((4 * (a.T + 1) + 7) & ~7u) + 6 * a.T; }
inline uint32_t req_aos_lds(const MixArgs& a, uint32_t desc_bytes) { return ((req_aos_head(a) + 15) & ~15u) + desc_bytes; }

__global__ __launch_bounds__(kBlock) void k_req_decode_aos(MixArgs a, MixAos x, const uint4* __restrict__ desc,
                                                           const uint8_t* __restrict__ cls,
                                                           const uint32_t* __restrict__ table, uint64_t rows,
                                                           const uint8_t* __restrict__ buf, uint64_t buf_len,
                                                           const uint32_t* __restrict__ offs, uint64_t nframes,
                                                           srpc_unpack_status* st) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    __shared__ uint32_t wcnt[kMixLds];
    __shared__ MixLds d;
    __shared__ MixAosSlices sl;
    const uint32_t K = a.nplans;
    const uint32_t lo_bytes = (4 * (a.T + 1) + 7) & ~7u;
    uint8_t* img = lds;
    uint32_t* lo = reinterpret_cast<uint32_t*>(lds + a.img + 32);
    uint32_t* pos = reinterpret_cast<uint32_t*>(lds + a.img + 32 + lo_bytes);
    uint16_t* slot = reinterpret_cast<uint16_t*>(pos + a.T);
    uint8_t* dsc = lds + ((a.img + 32 + lo_bytes + 6 * a.T + 15) & ~15u);

    mix_lds_fill(d, a);
    mix_aos_slices_init(sl, x, K);
    for (uint32_t c = threadIdx.x; c < x.desc_bytes / 16; c += kBlock) reinterpret_cast<uint4*>(dsc)[c] = desc[c];
    const uint64_t c0 = static_cast<uint64_t>(blockIdx.x) * a.T;
    const uint64_t g = c0 / kMixGranule;
    const uint32_t j0 = static_cast<uint32_t>(c0 - g * kMixGranule);  // the tile's first lane
    const uint64_t i = g * kMixGranule + threadIdx.x;
    const uint32_t nr = c0 < nframes ? static_cast<uint32_t>(min<uint64_t>(a.T, nframes - c0)) : 0;
    req_offsets(lo, a.T, offs, nframes, c0, buf_len);

    const MixLane r = mix_ranks(cls, nframes, K, table, rows, g, wcnt);  // barrier: lo[], d and the slices' init are complete
    const bool mine = threadIdx.x >= j0 && threadIdx.x < j0 + nr && r.cls < K;  // this tile's, and somebody's frame
    const bool good = mine && r.rank < d.room[r.cls];
    const uint32_t j = threadIdx.x - j0;
    if (mine && !good && st) report_bad(st, SRPC_STATUS_BOUNDS, i);

    // the tile's slices: good frames of one plan are consecutive ranks, ascending with the lane
    mix_aos_slices_count(sl, K, r, good);

    // 1. the span of the tile's frames -> image, from a 16-byte boundary (ends with a barrier)
    const ReqSpan sp = req_stage(img, lo, nr, a.img, buf, buf_len);

    // 2. a lane per frame: where its record is
    if (good) {
        const uint64_t o = lo[j];
        const uint32_t F = d.F[r.cls];
        if (o > buf_len || F > buf_len - o) {
            pos[j] = kPosZero;  // the class says otherwise: never read past the buffer
        } else {
            const bool in_img = o >= sp.s0 && o - sp.s0 + F <= sp.staged;
            pos[j] = in_img ? static_cast<uint32_t>(o - sp.s0) : kPosGlobal;
        }
    }

    // 3. image and fill -> the slices, one lane per (plan, 16-byte piece)
    mix_aos_store<kReqAosNt>(sl, d, K, r, good, j, img, lo, pos, slot, dsc, buf);
}

}  // namespace
}  // namespace srpc_impl

using namespace srpc_impl;

extern "C" {

int srpc_frames_unpack_requests_mixed_aos(const srpc_plan* const* req_plans, int nplans, const uint8_t* d_buf,
                                          uint64_t buf_len, const uint32_t* d_offs, uint64_t nframes,
                                          void* const* d_recs, const uint64_t* h_stride,
                                          const uint32_t* const* h_leaf_offs, const void* const* h_fill,
                                          const uint64_t* h_first, const uint64_t* h_cap, uint8_t* d_class,
                                          void* d_index, uint64_t index_bytes, uint64_t* d_counts,
                                          srpc_unpack_status* d_status, void* d_scratch, uint64_t scratch_bytes,
                                          void* stream) {
    const TimedCall timed;
    // the arguments themselves are checked before any plan is read
    if (any_null(req_plans, d_recs, h_stride, h_leaf_offs, h_fill, h_cap, d_index, d_counts, d_scratch) ||
        mix_nplans_bad(nplans) || past_u32(buf_len) || past_u32(nframes) ||
        (nframes && any_null(d_buf, d_offs, d_class)))
        return SRPC_E_INVALID;
    if (aos_args_invalid(d_recs, h_stride, h_leaf_offs, h_first, h_cap, nplans)) return SRPC_E_INVALID;
    for (int k = 0; k < nplans; ++k)
        if (!h_fill[k]) return SRPC_E_INVALID;
    uint32_t fmax = 0;
    if (int rc = mix_plans_ok(req_plans, nplans, 4, &fmax)) return rc;
    for (int k = 0; k < nplans; ++k)
        if (h_stride[k] > kAosMaxStride) return SRPC_E_UNSUPPORTED;
    // the tables and the fills, as they will lie in scratch and in LDS
    AosDesc desc;
    MixAos x{};
    if (int rc = aos_describe(req_plans, nplans, d_recs, h_stride, h_leaf_offs, h_fill, &desc, &x)) return rc;
    if (!aligned(d_buf, 16) || !aligned(d_index, 8) || !aligned(d_counts, 8) || !aligned(d_offs, 4) ||
        !aligned(d_scratch, 16))
        return SRPC_E_ALIGN;
    if (!aos_recs_aligned(req_plans, nplans, d_recs, h_stride, h_leaf_offs)) return SRPC_E_ALIGN;
    if (index_bytes < mix_index_bytes(nframes, nplans) || scratch_bytes < x.desc_bytes) return SRPC_E_CAPACITY;
    AosCols cols;
    aos_cols(req_plans, nplans, d_recs, h_leaf_offs, &cols);
    MixArgs a{};  // the classify pass: the column call's tile
    uint32_t tb = 0;
    if (int rc = mix_args(req_plans, nplans, cols.plan, h_first, h_cap, fmax, &a, &tb, 1)) return rc;
    MixArgs b = a;  // the decode: the tables and fills share the image's budget
    b.T = mix_aos_tile(fmax, x.desc_bytes);
    b.img = (b.T * fmax + 16 + 15) & ~15u;
    auto s = static_cast<hipStream_t>(stream);
    auto* table = static_cast<uint32_t*>(d_index);
    if (d_status && status_reset_launch(d_status, s)) return SRPC_E_HIP;
    if (int rc = mix_upload(desc.bytes, x.desc_bytes, d_scratch, s)) return rc;
    if (nframes) req_classify_launch(a, tb, d_buf, buf_len, d_offs, nframes, d_class, s);
    // unknown frames (0xFF) are ids >= K: column K of the index; no status here
    if (int rc = mix_index_launch(d_class, nframes, nplans, table, d_counts, nullptr, s)) return rc;
    if (nframes)
        launch(k_req_decode_aos, dim3(static_cast<uint32_t>((nframes + b.T - 1) / b.T)), dim3(kBlock),
               req_aos_lds(b, x.desc_bytes), s, b, x, static_cast<const uint4*>(d_scratch),
               static_cast<const uint8_t*>(d_class), static_cast<const uint32_t*>(table), mix_rows(nframes), d_buf, buf_len,
               d_offs, nframes, d_status);
    return hipGetLastError() == hipSuccess ? SRPC_OK : SRPC_E_HIP;
}

}  // extern "C"
