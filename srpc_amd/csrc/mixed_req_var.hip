// mixed_req_var.hip -- a batch of request frames of several methods, string-
// bodied ones included, decoded in arrival order (server side): mixed_req.hip's
// decode over the two plan kinds of mixed_var.hip, the mirror of that file's
// request pack: the two kernels over plans that all lie in columns.  The entry
// point (srpc_frames_unpack_requests_mixed_var) is an adapter in
// mixed_req_legs.hip, beside the call's one host path (mv_unpack_requests).
//
// The class of a frame is found from the frame itself (srpc_frames_classify's
// rule); its fields go to element first[k] + rank(i) of plan k's columns, rank(i)
// being the frames of the same class before it.  The ranks need the class of
// every earlier frame, so the stream is read twice and nothing waits on another
// workgroup:
//
//   k_mrv_classify  a workgroup per tile of T frames (MvDesc::T): the tile's span
//       staged into the 32 KiB LDS image from a 16-byte boundary, the frame
//       offsets beside it, the K prefixes as LDS templates.  A lane per frame:
//       fixed plans are compared only where F_k is the frame's length, eight
//       bytes at a time; for string plans BE32 == len - 4 is tested once, then
//       per plan the least length, the prefix and the walk of the fields, which
//       reads the length words only (at most 16 per plan).  A frame that does
//       not lie whole inside the image is judged from global memory by its lane,
//       reading no more than its fixed part.  Writes the class byte only.
//   k_mixed_hist / k_mixed_scan (mixed.hip) over the class bytes: the index and
//       the counts, unknown frames in column K.
//   k_mrv_parse     the same tile and staging; the granule's ranks from the index
//       (mix_ranks); a lane per frame stores its fixed leaves, each string's
//       length into its offsets entry and its chars' stream offset to scratch.
//       Every read is bounded by the frame's own extent again: the class is
//       not trusted to keep the walk inside buf_len.  The lane's frame and its
//       walk (MrvFrame, mrv_lane_walk) live in mixed_req_var_tile.h, which
//       mixed_req_legs.hip's parse kernel shares; a batch without a record
//       plan is this kernel's (mrv_parse_launch).
//   the slot scan and the char copy of mixed_var.hip (mv_strings_launch) with
//       d_class as the method vector.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "mixed_common.h"
#include "mixed_req_var_tile.h"
#include "mixed_var_common.h"
#include "plan.h"
#include "srpc_gpu.h"

namespace srpc_impl {
namespace {

constexpr uint32_t kMrvUnknown = SRPC_FRAME_UNKNOWN;

// Frame bytes [at, at + pl) == the template (8-byte aligned in LDS, pl > 0).
__device__ __forceinline__ bool mrv_prefix_eq(const MrvFrame& fr, uint32_t at, const uint8_t* pre, uint32_t pl) {
    bool eq = true;
    if (fr.in_img) {
        for (uint32_t b = 0; b < pl; b += 8) {
            const uint64_t m = pl - b >= 8 ? ~0ull : (1ull << (8 * (pl - b))) - 1;
            eq &= ((lds_u64(fr.img, fr.q + at + b) ^ *reinterpret_cast<const uint64_t*>(pre + b)) & m) == 0;
        }
    } else {
        for (uint32_t b = 0; b < pl && eq; ++b) eq = fr.g[at + b] == pre[b];
    }
    return eq;
}

// LDS of k_mrv_classify: image[kMixImage + 16] | templates[tmpl_bytes] | 16 pad,
// then the static tile offsets.
__global__ __launch_bounds__(kBlock) void k_mrv_classify(const MvDesc* __restrict__ d, const uint8_t* __restrict__ buf,
                                                         uint64_t buf_len, const uint32_t* __restrict__ offs,
                                                         uint64_t nframes, uint8_t* __restrict__ cls) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    __shared__ uint32_t lo[kBlock + 1];
    uint8_t* img = lds;
    const uint8_t* tmpl = lds + kMixImage + 16;
    const uint32_t K = d->nplans, T = d->T;
    const uint64_t c0 = static_cast<uint64_t>(blockIdx.x) * T;
    const uint32_t nr = c0 < nframes ? static_cast<uint32_t>(min<uint64_t>(T, nframes - c0)) : 0;
    mv_templates(lds + kMixImage + 16, d);
    req_offsets(lo, T, offs, nframes, c0, buf_len);
    __syncthreads();
    const ReqSpan sp = req_stage(img, lo, nr, kMixImage, buf, buf_len);

    const uint32_t j = threadIdx.x;
    if (j >= nr) return;
    const uint64_t o = lo[j], e = lo[j + 1];
    uint32_t k = kMrvUnknown;
    if (o <= e && e <= buf_len) {  // else: offsets out of order or past the buffer, no byte is read
        const uint64_t len = e - o;
        MrvFrame fr;
        fr.img = img;
        fr.g = buf + o;
        fr.in_img = o >= sp.s0 && o - sp.s0 + len <= sp.staged;
        fr.q = static_cast<uint32_t>(o - sp.s0);
        // string plans: the BE32 is the payload's length, whichever the plan
        const bool framed = len >= 4 && __builtin_bswap32(static_cast<uint32_t>(mrv_field(fr, 0, 4))) == len - 4;
        for (uint32_t p = 0; p < K && k == kMrvUnknown; ++p) {
            const uint32_t pl = d->prefix_len[p];
            const uint8_t* pre = tmpl + d->tmpl[p];
            if (!d->var[p]) {
                // F_p >= pl: the prefix is inside the frame
                if (d->F[p] == len && mrv_prefix_eq(fr, 0, pre, pl)) k = p;
                continue;
            }
            // F_p = 4 + the least payload >= 4 + pl
            if (!framed || len < d->F[p] || !mrv_prefix_eq(fr, 4, pre, pl)) continue;
            // the walk of the fields ends exactly at the frame's end
            uint64_t c = 4 + pl;
            bool ok = true;
            for (uint32_t f = d->field0[p]; ok && f < d->field0[p + 1]; ++f) {
                const uint32_t s = d->size[f];
                if (s) {
                    ok = s <= len - c;
                    c += s;
                } else if (8 > len - c) {
                    ok = false;
                } else {
                    const uint64_t sl = mrv_u64(fr, c);
                    c += 8;
                    ok = sl <= len - c;  // 2^63 or 2^64 - 1 cannot wrap
                    if (ok) c += sl;
                }
            }
            if (ok && c == len) k = p;
        }
    }
    cls[c0 + j] = static_cast<uint8_t>(k);
}

// LDS of k_mrv_parse: image[kMixImage + 16], then static wcnt and the tile's
// offsets.
__global__ __launch_bounds__(kBlock) void k_mrv_parse(const MvDesc* __restrict__ d, const uint8_t* __restrict__ cls,
                                                      const uint32_t* __restrict__ table, uint64_t rows,
                                                      const uint8_t* __restrict__ buf, uint64_t buf_len,
                                                      const uint32_t* __restrict__ offs, uint64_t nframes,
                                                      uint32_t* __restrict__ srcs, uint32_t* __restrict__ counts,
                                                      srpc_unpack_status* st) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    __shared__ uint32_t wcnt[kMixLds];
    __shared__ uint32_t lo[kBlock + 1];
    uint8_t* img = lds;
    const uint32_t K = d->nplans, T = d->T;
    const uint64_t c0 = static_cast<uint64_t>(blockIdx.x) * T;
    const uint64_t g = c0 / kMixGranule;
    const uint32_t j0 = static_cast<uint32_t>(c0 - g * kMixGranule);  // the tile's first lane
    const uint64_t i = g * kMixGranule + threadIdx.x;
    const uint32_t nr = c0 < nframes ? static_cast<uint32_t>(min<uint64_t>(T, nframes - c0)) : 0;
    req_offsets(lo, T, offs, nframes, c0, buf_len);
    const MixLane r = mix_ranks(cls, nframes, K, table, rows, g, wcnt);  // barrier: lo[] is complete
    // the batch's frames per plan, for the slot scan: the last tile's granule is the last one
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x < K) {
        uint32_t v = wcnt[kMixWaves * kMixRow + threadIdx.x];
        for (uint32_t w = 0; w < kMixWaves; ++w) v += wcnt[w * kMixRow + threadIdx.x];
        counts[threadIdx.x] = v;
    }
    const ReqSpan sp = req_stage(img, lo, nr, kMixImage, buf, buf_len);

    if (threadIdx.x < j0 || threadIdx.x >= j0 + nr || r.cls >= K) return;  // not this tile's, or nobody's frame
    const uint32_t k = r.cls;
    if (r.rank >= d->room[k]) {
        if (st) report_bad(st, SRPC_STATUS_BOUNDS, i);
        return;
    }
    mrv_lane_walk(d, k, r.rank, threadIdx.x - j0, i, lo, img, sp, buf, buf_len, nframes, srcs);
}

}  // namespace

void mrv_classify_launch(const MvDesc& d, const MvDesc* dd, const uint8_t* d_buf, uint64_t buf_len,
                         const uint32_t* d_offs, uint64_t nframes, uint8_t* d_class, hipStream_t s) {
    launch(k_mrv_classify, dim3(static_cast<uint32_t>((nframes + d.T - 1) / d.T)), dim3(kBlock), mv_lds(d), s, dd, d_buf,
           buf_len, d_offs, nframes, d_class);
}

void mrv_parse_launch(const MvDesc& d, const MvDesc* dd, const uint8_t* d_class, const uint32_t* table, uint64_t rows,
                      const uint8_t* d_buf, uint64_t buf_len, const uint32_t* d_offs, uint64_t nframes, uint32_t* srcs,
                      uint32_t* counts, srpc_unpack_status* d_status, hipStream_t s) {
    launch(k_mrv_parse, dim3(static_cast<uint32_t>((nframes + d.T - 1) / d.T)), dim3(kBlock), kMixImage + 16, s, dd,
           d_class, table, rows, d_buf, buf_len, d_offs, nframes, srcs, counts, d_status);
}

}  // namespace srpc_impl
