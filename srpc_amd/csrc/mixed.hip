// mixed.hip -- batches of calls of several methods in caller-given order
// (client side; srpc_frames_mixed_index, srpc_frames_pack_requests_mixed,
// srpc_frames_unpack_replies_mixed of include/srpc_gpu.h).
//
// Call i of a chunk belongs to plan d_method[i]; its fields are element
// first[k] + rank(i) of plan k's columns, rank(i) being the number of earlier
// calls of the same plan.  Nothing here waits on another workgroup:
//
//   k_mixed_hist   a workgroup per super-row of 16 granules of 256 calls:
//       per-plan ballots give each granule's histogram (K plans and one column
//       for ids >= K); a granule's table row of K + 1 u32 is the calls before
//       it inside its super-row, the super-row holds their total.
//   k_mixed_scan   one workgroup turns the super-rows' columns into exclusive
//       prefixes (segments of rows per thread, the segment sums scanned in LDS)
//       and writes the chunk's counts.  The index IS that table: 4 (K + 1)
//       (1 + 1/16) bytes per 256 calls, no rank per call.
//   (k_mixed_pack's tile and the decode's judgement of a frame are
//   mix_pack_tile and mix_judge of mixed_common.h, shared with mixed_aos.hip.)
//   mix_ranks      (mixed_common.h; every consumer) the granule's 256 method bytes again: the
//       rank of a call is its plan's two table entries (granule + super-row)
//       plus the ballot counts of the lanes before it.
//   k_mixed_pack   a workgroup per tile of T calls (T = 256, or the power of
//       two >= 16 whose T * F_max fits the 32 KiB image; the tile's workgroup
//       still ranks its whole granule).  The byte offset of the granule is
//       sum_k min(table[k], room[k]) * F[k], the in-granule offsets a workgroup
//       scan of the frame lengths.  Each lane builds its frame in the LDS image
//       (prefix from an LDS template by lds_copy_run, fields by lds_put_small:
//       aligned LDS accesses only); the image leaves as aligned 16-byte stores,
//       the chunks shared with neighbouring tiles bytewise.
//   k_mixed_unpack the same tile: the span of its frames is staged into the
//       image with 16-byte loads, a lane per frame judges it by the table of
//       srpc_frames_unpack_replies against its own plan's prefix and stores
//       its fields per element.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "mixed_common.h"
#include "plan.h"
#include "srpc_gpu.h"

namespace srpc_impl {
namespace {

constexpr uint32_t kMixScanBlock = 1024;

// A workgroup per super-row of kMixSuper granules: granule row = the calls of
// each class before it inside the super-row, super-row = their total (scanned
// by k_mixed_scan).
__global__ __launch_bounds__(kBlock) void k_mixed_hist(const uint8_t* __restrict__ method, uint64_t ncalls, uint32_t K,
                                                       uint32_t* __restrict__ table, uint64_t rows,
                                                       srpc_unpack_status* st) {
    __shared__ uint32_t cnt[kMixSuper * kMixWaves * kMixRow];
    const uint64_t g0 = static_cast<uint64_t>(blockIdx.x) * kMixSuper;
    const uint32_t ng = static_cast<uint32_t>(min<uint64_t>(kMixSuper, rows - g0));
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // every granule's method byte first: the loads are in flight together
    uint32_t cls[kMixSuper];
#pragma unroll
    for (uint32_t q = 0; q < kMixSuper; ++q) {
        const uint64_t i = (g0 + q) * kMixGranule + threadIdx.x;
        cls[q] = q < ng && i < ncalls ? min(static_cast<uint32_t>(method[i]), K) : K + 1;
    }
#pragma unroll
    for (uint32_t q = 0; q < kMixSuper; ++q) {
        for (uint32_t k = 0; k <= K; ++k) {
            const uint64_t b = __ballot(cls[q] == k);
            if (lane == 0) cnt[(q * kMixWaves + w) * kMixRow + k] = __popcll(b);
        }
        if (cls[q] == K && st) report_bad(st, SRPC_STATUS_BOUNDS, (g0 + q) * kMixGranule + threadIdx.x);
    }
    __syncthreads();
    if (threadIdx.x <= K) {
        uint32_t run = 0;
        for (uint32_t q = 0; q < ng; ++q) {
            table[(g0 + q) * (K + 1) + threadIdx.x] = run;
            for (uint32_t x = 0; x < kMixWaves; ++x) run += cnt[(q * kMixWaves + x) * kMixRow + threadIdx.x];
        }
        table[(rows + blockIdx.x) * (K + 1) + threadIdx.x] = run;
    }
}

// One workgroup: table[r][c] (rows granules, cols K + 1) -> exclusive prefix
// down every column, the totals to counts[0..K].
__global__ __launch_bounds__(kMixScanBlock) void k_mixed_scan(uint32_t* __restrict__ table, uint64_t rows, uint32_t cols,
                                                              uint64_t* __restrict__ counts) {
    __shared__ uint32_t sums[kMixScanBlock];
    const uint32_t nseg = kMixScanBlock / cols;
    const uint32_t c = threadIdx.x % cols, seg = threadIdx.x / cols;
    const uint64_t per = (rows + nseg - 1) / nseg;
    const bool on = seg < nseg;
    const uint64_t r0 = min<uint64_t>(static_cast<uint64_t>(seg) * per, rows), r1 = min<uint64_t>(r0 + per, rows);
    uint32_t s = 0;
    if (on)
        for (uint64_t r = r0; r < r1; ++r) s += table[r * cols + c];
    sums[threadIdx.x] = s;
    __syncthreads();
    if (!on) return;
    uint32_t run = 0;
    for (uint32_t q = 0; q < seg; ++q) run += sums[q * cols + c];
    if (seg == nseg - 1) counts[c] = static_cast<uint64_t>(run) + s;
    for (uint64_t r = r0; r < r1; ++r) {
        const uint32_t v = table[r * cols + c];
        table[r * cols + c] = run;
        run += v;
    }
}

__global__ __launch_bounds__(kBlock) void k_mixed_ranks(const uint32_t* __restrict__ table, uint64_t rows,
                                                        const uint8_t* __restrict__ method, uint64_t ncalls, uint32_t K,
                                                        uint32_t* __restrict__ rank) {
    __shared__ uint32_t wcnt[kMixLds];
    const uint64_t g = blockIdx.x;
    const MixLane r = mix_ranks(method, ncalls, K, table, rows, g, wcnt);
    const uint64_t i = g * kMixGranule + threadIdx.x;
    if (i < ncalls) rank[i] = r.cls < K ? r.rank : kNoRank;
}

// The request pack over columns: mix_pack_tile (mixed_common.h) with a leaf of
// element e at col[f] + e * size[f].
__global__ __launch_bounds__(kBlock) void k_mixed_pack(MixArgs a, const uint8_t* __restrict__ method,
                                                       const uint32_t* __restrict__ table, uint64_t rows,
                                                       uint64_t ncalls, uint8_t* __restrict__ out,
                                                       uint32_t* __restrict__ offs, srpc_unpack_status* st) {
    mix_pack_tile<false>(a, nullptr, method, table, rows, ncalls, out, offs, st);
}

// LDS of k_mixed_unpack: image[a.img + 32] | lo[T + 1] (8-byte padded) | the K
// prefixes (8-byte aligned each), then static wcnt and the lookups.
__global__ __launch_bounds__(kBlock) void k_mixed_unpack(MixArgs a, const uint8_t* __restrict__ method,
                                                         const uint32_t* __restrict__ table, uint64_t rows,
                                                         uint64_t ncalls, const uint8_t* __restrict__ buf,
                                                         uint64_t buf_len,
                                                         const uint32_t* __restrict__ offs, uint64_t nframes,
                                                         uint32_t unanswered, uint8_t* __restrict__ codes,
                                                         srpc_unpack_status* st) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    __shared__ uint32_t wcnt[kMixLds];
    __shared__ MixLds d;
    uint8_t* img = lds;
    uint32_t* lo = reinterpret_cast<uint32_t*>(lds + a.img + 32);
    uint8_t* tmpl = lds + a.img + 32 + ((4 * (a.T + 1) + 7) & ~7u);
    const uint32_t K = a.nplans;
    mix_lds_fill(d, a);
    mix_templates(tmpl, a);
    const uint64_t c0 = static_cast<uint64_t>(blockIdx.x) * a.T;
    const uint64_t g = c0 / kMixGranule;
    const uint32_t j0 = static_cast<uint32_t>(c0 - g * kMixGranule);
    const uint64_t i = g * kMixGranule + threadIdx.x;
    // frames of this tile
    const uint32_t nr = c0 < nframes ? static_cast<uint32_t>(min<uint64_t>(a.T, nframes - c0)) : 0;
    req_offsets(lo, a.T, offs, nframes, c0, buf_len);

    const MixLane r = mix_ranks(method, ncalls, K, table, rows, g, wcnt);  // barrier: lo[] is complete
    const bool good = r.cls < K && r.rank < d.room[r.cls];

    // 1. the span of the tile's frames -> image, from a 16-byte boundary
    const ReqSpan sp = req_stage(img, lo, nr, a.img, buf, buf_len);

    // 2. a lane per call: judge its frame, store its code and fields
    const bool mine = threadIdx.x >= j0 && threadIdx.x < j0 + a.T && i < ncalls;
    if (!mine) return;
    const MixReply y = mix_judge(d, r, good, threadIdx.x - j0, nr, lo, img, tmpl, sp, buf, buf_len, unanswered);
    codes[i] = static_cast<uint8_t>(y.code);
    if (y.flag && st) report_bad(st, y.flag, i);
    if (!good) return;  // no column element is touched for a bad call
    const uint32_t k = r.cls;
    const uint64_t e = d.first[k] + r.rank;
    for (uint32_t f = d.field0[k]; f < d.field0[k + 1]; ++f) {
        const uint32_t s = d.size[f];
        uint64_t v = 0;
        if (y.decoded) {
            if (y.in_img) {
                v = s == 1 ? img[y.q + d.off[f]] : lds_u64(img, y.q + d.off[f]);
            } else {
                const uint8_t* gp = buf + y.o + d.off[f];
                for (uint32_t b = 0; b < s; ++b) v |= static_cast<uint64_t>(gp[b]) << (8 * b);
            }
        }
        store_elem(d.col[f] + e * s, s, v);
    }
}

}  // namespace

int mix_index_launch(const uint8_t* d_method, uint64_t ncalls, int nplans, uint32_t* table, uint64_t* d_counts,
                     srpc_unpack_status* d_status, hipStream_t s) {
    const uint64_t rows = mix_rows(ncalls);
    if (d_status && status_reset_launch(d_status, s)) return SRPC_E_HIP;
    if (rows)
        launch(k_mixed_hist, dim3(static_cast<uint32_t>(mix_super_rows(rows))), dim3(kBlock), 0, s, d_method, ncalls,
               static_cast<uint32_t>(nplans), table, rows, d_status);
    launch(k_mixed_scan, dim3(1), dim3(kMixScanBlock), 0, s, table + rows * (nplans + 1), mix_super_rows(rows),
           static_cast<uint32_t>(nplans + 1), d_counts);
    return hipGetLastError() == hipSuccess ? SRPC_OK : SRPC_E_HIP;
}

}  // namespace srpc_impl

using namespace srpc_impl;

extern "C" {

int srpc_frames_mixed_index_bytes(uint64_t ncalls, int nplans, uint64_t* out) {
    if (!out || mix_nplans_bad(nplans) || past_u32(ncalls)) return SRPC_E_INVALID;
    *out = mix_index_bytes(ncalls, nplans);
    return SRPC_OK;
}

int srpc_frames_mixed_index(const uint8_t* d_method, uint64_t ncalls, int nplans, void* d_index, uint64_t index_bytes,
                            uint64_t* d_counts, srpc_unpack_status* d_status, void* stream) {
    const TimedCall timed;
    if (any_null(d_index, d_counts) || (ncalls && !d_method) || mix_nplans_bad(nplans) || past_u32(ncalls))
        return SRPC_E_INVALID;
    if (!aligned(d_index, 8) || !aligned(d_counts, 8)) return SRPC_E_ALIGN;
    if (index_bytes < mix_index_bytes(ncalls, nplans)) return SRPC_E_CAPACITY;
    return mix_index_launch(d_method, ncalls, nplans, static_cast<uint32_t*>(d_index), d_counts, d_status,
                            static_cast<hipStream_t>(stream));
}

int srpc_frames_mixed_ranks(const void* d_index, const uint8_t* d_method, uint64_t ncalls, int nplans, uint32_t* d_rank,
                            void* stream) {
    if (!d_index || (ncalls && any_null(d_method, d_rank)) || mix_nplans_bad(nplans) || past_u32(ncalls))
        return SRPC_E_INVALID;
    if (!aligned(d_index, 8) || !aligned(d_rank, 4)) return SRPC_E_ALIGN;
    if (!ncalls) return SRPC_OK;
    hipLaunchKernelGGL(k_mixed_ranks, dim3(static_cast<uint32_t>(mix_rows(ncalls))), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), static_cast<const uint32_t*>(d_index), mix_rows(ncalls), d_method,
                       ncalls, static_cast<uint32_t>(nplans), d_rank);
    return hipGetLastError() == hipSuccess ? SRPC_OK : SRPC_E_HIP;
}

int srpc_frames_mixed_tile(const srpc_plan* const* plans, int nplans, uint32_t* calls_per_tile) {
    if (any_null(plans, calls_per_tile) || mix_nplans_bad(nplans)) return SRPC_E_INVALID;
    uint32_t fmax = 0;
    if (int rc = mix_plans_ok(plans, nplans, 4, &fmax)) return rc;
    *calls_per_tile = mix_tile(fmax);
    return SRPC_OK;
}

int srpc_frames_pack_requests_mixed(const srpc_plan* const* req_plans, int nplans, const void* const* const* d_cols,
                                    const uint64_t* h_first, const uint64_t* h_cap, const uint8_t* d_method,
                                    const void* d_index, uint64_t ncalls, uint8_t* d_out, uint64_t out_cap,
                                    uint32_t* d_offs, srpc_unpack_status* d_status, void* stream) {
    const TimedCall timed;
    // the arguments themselves are checked before any plan is read
    if (any_null(req_plans, d_cols, h_cap, d_index) || mix_nplans_bad(nplans) || past_u32(ncalls) ||
        (ncalls && any_null(d_method, d_out)))
        return SRPC_E_INVALID;
    uint32_t fmax = 0;
    if (int rc = mix_plans_ok(req_plans, nplans, 4, &fmax)) return rc;
    if (!aligned(d_out, 16) || !aligned(d_index, 8) || !aligned(d_offs, 4)) return SRPC_E_ALIGN;
    MixArgs a{};
    uint32_t tb = 0;
    if (int rc = mix_args(req_plans, nplans, d_cols, h_first, h_cap, fmax, &a, &tb)) return rc;
    if (out_cap < ncalls * fmax) return SRPC_E_CAPACITY;
    if (d_offs && ncalls * fmax >= (1ull << 32)) return SRPC_E_INVALID;  // u32 offsets
    const uint32_t grid = static_cast<uint32_t>(std::max<uint64_t>(1, (ncalls + a.T - 1) / a.T));
    launch(k_mixed_pack, dim3(grid), dim3(kBlock), a.img + tb + 16, static_cast<hipStream_t>(stream), a, d_method,
           static_cast<const uint32_t*>(d_index), mix_rows(ncalls), ncalls, d_out, d_offs, d_status);
    return hipGetLastError() == hipSuccess ? SRPC_OK : SRPC_E_HIP;
}

int srpc_frames_unpack_replies_mixed(const srpc_plan* const* reply_plans, int nplans, const uint8_t* d_buf,
                                     uint64_t buf_len, const uint32_t* d_offs, uint64_t nframes, const uint8_t* d_method,
                                     const void* d_index, uint64_t ncalls, uint8_t unanswered_code,
                                     void* const* const* d_cols, const uint64_t* h_first, const uint64_t* h_cap,
                                     uint8_t* d_codes, srpc_unpack_status* d_status, void* stream) {
    const TimedCall timed;
    if (any_null(reply_plans, d_cols, h_cap, d_index, d_codes) ||
        mix_nplans_bad(nplans) || nframes > ncalls || past_u32(buf_len) || past_u32(ncalls) ||
        (ncalls && !d_method) || (nframes && any_null(d_buf, d_offs)))
        return SRPC_E_INVALID;
    uint32_t fmax = 0;
    if (int rc = mix_plans_ok(reply_plans, nplans, 5, &fmax)) return rc;
    if (!aligned(d_buf, 16) || !aligned(d_index, 8) || !aligned(d_offs, 4)) return SRPC_E_ALIGN;
    MixArgs a{};
    uint32_t tb = 0;
    if (int rc = mix_args(reply_plans, nplans, reinterpret_cast<const void* const* const*>(d_cols), h_first, h_cap, fmax,
                          &a, &tb))
        return rc;
    auto s = static_cast<hipStream_t>(stream);
    if (d_status && status_reset_launch(d_status, s)) return SRPC_E_HIP;
    if (!ncalls) return SRPC_OK;
    const uint32_t grid = static_cast<uint32_t>((ncalls + a.T - 1) / a.T);
    launch(k_mixed_unpack, dim3(grid), dim3(kBlock), a.img + 32 + ((4 * (a.T + 1) + 7) & ~7u) + tb, s, a, d_method,
           static_cast<const uint32_t*>(d_index), mix_rows(ncalls), ncalls, d_buf, buf_len, d_offs, nframes,
           static_cast<uint32_t>(unanswered_code), d_codes, d_status);
    return hipGetLastError() == hipSuccess ? SRPC_OK : SRPC_E_HIP;
}

}  // extern "C"
