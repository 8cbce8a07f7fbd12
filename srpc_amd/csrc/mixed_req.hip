// mixed_req.hip -- a batch of request frames of several methods decoded in
// arrival order (server side; srpc_frames_unpack_requests_mixed of
// include/srpc_gpu.h): the mirror of mixed.hip's reply decode, with the class
// of every frame found from the frame itself instead of given by the caller.
//
// Frame i is of plan k when it is exactly one record of it (srpc_frames_classify's
// rule for fixed-size plans); its fields go to element first[k] + rank(i) of plan
// k's columns, rank(i) being the frames of the same plan before it.  The ranks
// need the class of every earlier frame, so the stream is read twice and nothing
// waits on another workgroup:
//
//   k_req_classify  a workgroup per tile of T frames (mix_tile): the tile's span
//       is staged into the LDS image with 16-byte loads from a 16-byte boundary,
//       the K prefixes are LDS templates; a lane per frame compares, eight bytes
//       at a time, the prefixes of the plans whose F_k is its frame's length and
//       writes the class byte.
//   k_mixed_hist / k_mixed_scan (mixed.hip) over the class bytes: the call index
//       and the counts, unknown frames (0xFF >= K) in column K.
//   k_req_decode    the same tile and staging (the span is in L2 / Infinity Cache
//       from the first pass when the batch fits); the granule's ranks from the
//       index (mix_ranks), a lane per frame stores its fields per element.
//
// A frame that an oversize junk frame pushed out of the image is read on its
// own from global memory, at most F_k bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "mixed_common.h"
#include "plan.h"
#include "srpc_gpu.h"

namespace srpc_impl {
namespace {

constexpr uint32_t kReqUnknown = SRPC_FRAME_UNKNOWN;

// LDS of both kernels: image[a.img + 32] | lo[T + 1] (8-byte padded) | the K
// prefixes (classify only).
__device__ __forceinline__ uint32_t req_lo_at(const MixArgs& a) { return a.img + 32; }
__device__ __forceinline__ uint32_t req_tmpl_at(const MixArgs& a) { return a.img + 32 + ((4 * (a.T + 1) + 7) & ~7u); }

__global__ __launch_bounds__(kBlock) void k_req_classify(MixArgs a, const uint8_t* __restrict__ buf, uint64_t buf_len,
                                                         const uint32_t* __restrict__ offs, uint64_t nframes,
                                                         uint8_t* __restrict__ cls) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    __shared__ MixLds d;
    uint8_t* img = lds;
    uint32_t* lo = reinterpret_cast<uint32_t*>(lds + req_lo_at(a));
    const uint8_t* tmpl = lds + req_tmpl_at(a);
    const uint32_t K = a.nplans;
    const uint64_t c0 = static_cast<uint64_t>(blockIdx.x) * a.T;
    const uint32_t nr = c0 < nframes ? static_cast<uint32_t>(min<uint64_t>(a.T, nframes - c0)) : 0;
    mix_lds_fill(d, a);
    mix_templates(lds + req_tmpl_at(a), a);
    req_offsets(lo, a.T, offs, nframes, c0, buf_len);
    __syncthreads();
    const ReqSpan sp = req_stage(img, lo, nr, a.img, buf, buf_len);

    const uint32_t j = threadIdx.x;
    if (j >= nr) return;
    const uint64_t o = lo[j], e = lo[j + 1];
    uint32_t k = kReqUnknown;
    if (o <= e && e <= buf_len) {  // else: offsets out of order or past the buffer, no byte is read
        const uint64_t len = e - o;
        const bool in_img = o >= sp.s0 && o - sp.s0 + len <= sp.staged;
        const uint32_t q = static_cast<uint32_t>(o - sp.s0);
        for (uint32_t p = 0; p < K && k == kReqUnknown; ++p) {
            if (d.F[p] != len) continue;
            const uint32_t pl = d.prefix_len[p];  // <= F_p: the prefix is inside the frame
            const uint8_t* pre = tmpl + d.tmpl[p];
            bool eq = true;
            if (in_img) {
                for (uint32_t b = 0; b < pl; b += 8) {
                    const uint64_t m = pl - b >= 8 ? ~0ull : (1ull << (8 * (pl - b))) - 1;
                    eq &= ((lds_u64(img, q + b) ^ *reinterpret_cast<const uint64_t*>(pre + b)) & m) == 0;
                }
            } else {
                for (uint32_t b = 0; b < pl && eq; ++b) eq = buf[o + b] == pre[b];
            }
            if (eq) k = p;
        }
    }
    cls[c0 + j] = static_cast<uint8_t>(k);
}

__global__ __launch_bounds__(kBlock) void k_req_decode(MixArgs a, const uint8_t* __restrict__ cls,
                                                       const uint32_t* __restrict__ table, uint64_t rows,
                                                       const uint8_t* __restrict__ buf, uint64_t buf_len,
                                                       const uint32_t* __restrict__ offs, uint64_t nframes,
                                                       srpc_unpack_status* st) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    __shared__ uint32_t wcnt[kMixLds];
    __shared__ MixLds d;
    uint8_t* img = lds;
    uint32_t* lo = reinterpret_cast<uint32_t*>(lds + req_lo_at(a));
    const uint32_t K = a.nplans;
    const uint64_t c0 = static_cast<uint64_t>(blockIdx.x) * a.T;
    const uint64_t g = c0 / kMixGranule;
    const uint32_t j0 = static_cast<uint32_t>(c0 - g * kMixGranule);  // the tile's first lane
    const uint64_t i = g * kMixGranule + threadIdx.x;
    const uint32_t nr = c0 < nframes ? static_cast<uint32_t>(min<uint64_t>(a.T, nframes - c0)) : 0;
    mix_lds_fill(d, a);
    req_offsets(lo, a.T, offs, nframes, c0, buf_len);
    const MixLane r = mix_ranks(cls, nframes, K, table, rows, g, wcnt);  // barrier: lo[] and d are complete
    const ReqSpan sp = req_stage(img, lo, nr, a.img, buf, buf_len);

    if (threadIdx.x < j0 || threadIdx.x >= j0 + nr || r.cls >= K) return;  // not this tile's, or nobody's frame
    const uint32_t k = r.cls;
    if (r.rank >= d.room[k]) {
        if (st) report_bad(st, SRPC_STATUS_BOUNDS, i);
        return;
    }
    const uint64_t o = lo[threadIdx.x - j0];
    const uint32_t F = d.F[k];
    if (o > buf_len || F > buf_len - o) return;  // the class says otherwise: never read past the buffer
    const bool in_img = o >= sp.s0 && o - sp.s0 + F <= sp.staged;
    const uint32_t q = static_cast<uint32_t>(o - sp.s0);
    const uint64_t e = d.first[k] + r.rank;
    for (uint32_t f = d.field0[k]; f < d.field0[k + 1]; ++f) {
        const uint32_t s = d.size[f];
        uint64_t v = 0;
        if (in_img) {
            v = s == 1 ? img[q + d.off[f]] : lds_u64(img, q + d.off[f]);
        } else {
            const uint8_t* gp = buf + o + d.off[f];
            for (uint32_t b = 0; b < s; ++b) v |= static_cast<uint64_t>(gp[b]) << (8 * b);
        }
        store_elem(d.col[f] + e * s, s, v);
    }
}

}  // namespace

// k_req_classify over nframes frames (mixed_req_aos.hip's first pass too).
void req_classify_launch(const MixArgs& a, uint32_t tmpl_bytes, const uint8_t* d_buf, uint64_t buf_len,
                         const uint32_t* d_offs, uint64_t nframes, uint8_t* d_class, hipStream_t s) {
    const uint32_t grid = static_cast<uint32_t>((nframes + a.T - 1) / a.T);
    const uint32_t lds = a.img + 32 + ((4 * (a.T + 1) + 7) & ~7u);
    launch(k_req_classify, dim3(grid), dim3(kBlock), lds + tmpl_bytes, s, a, d_buf, buf_len, d_offs, nframes, d_class);
}

}  // namespace srpc_impl

using namespace srpc_impl;

extern "C" {

int srpc_frames_unpack_requests_mixed(const srpc_plan* const* req_plans, int nplans, const uint8_t* d_buf,
                                      uint64_t buf_len, const uint32_t* d_offs, uint64_t nframes,
                                      void* const* const* d_cols, const uint64_t* h_first, const uint64_t* h_cap,
                                      uint8_t* d_class, void* d_index, uint64_t index_bytes, uint64_t* d_counts,
                                      srpc_unpack_status* d_status, void* stream) {
    const TimedCall timed;
    // the arguments themselves are checked before any plan is read
    if (any_null(req_plans, d_cols, h_cap, d_index, d_counts) ||
        mix_nplans_bad(nplans) || past_u32(buf_len) || past_u32(nframes) ||
        (nframes && any_null(d_buf, d_offs, d_class)))
        return SRPC_E_INVALID;
    uint32_t fmax = 0;
    if (int rc = mix_plans_ok(req_plans, nplans, 4, &fmax)) return rc;
    if (!aligned(d_buf, 16) || !aligned(d_index, 8) || !aligned(d_counts, 8) || !aligned(d_offs, 4)) return SRPC_E_ALIGN;
    MixArgs a{};
    uint32_t tb = 0;
    if (int rc = mix_args(req_plans, nplans, reinterpret_cast<const void* const* const*>(d_cols), h_first, h_cap, fmax,
                          &a, &tb))
        return rc;
    if (index_bytes < mix_index_bytes(nframes, nplans)) return SRPC_E_CAPACITY;
    auto s = static_cast<hipStream_t>(stream);
    auto* table = static_cast<uint32_t*>(d_index);
    if (d_status && status_reset_launch(d_status, s)) return SRPC_E_HIP;
    const uint32_t grid = static_cast<uint32_t>((nframes + a.T - 1) / a.T);
    const uint32_t lds = a.img + 32 + ((4 * (a.T + 1) + 7) & ~7u);
    if (nframes) req_classify_launch(a, tb, d_buf, buf_len, d_offs, nframes, d_class, s);
    // unknown frames (0xFF) are ids >= K: column K of the index; no status here
    if (int rc = mix_index_launch(d_class, nframes, nplans, table, d_counts, nullptr, s)) return rc;
    if (nframes)
        launch(k_req_decode, dim3(grid), dim3(kBlock), lds, s, a, static_cast<const uint8_t*>(d_class),
               static_cast<const uint32_t*>(table), mix_rows(nframes), d_buf, buf_len, d_offs, nframes, d_status);
    return hipGetLastError() == hipSuccess ? SRPC_OK : SRPC_E_HIP;
}

}  // extern "C"
