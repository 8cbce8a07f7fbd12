// mixed_var.hip -- batches of calls of several methods in caller-given order
// whose plans may have string fields, every plan in columns (client side): the
// kernels, their launches and the host-side builders of the plans' description
// (mixed_var_common.h).  The entry points (srpc_frames_*_mixed_var of
// include/srpc_gpu.h) are adapters in mixed_legs.hip, beside the one host path
// of each call.  The call index and mix_ranks are mixed.hip's (mixed_common.h).
// Nothing here waits on another workgroup.
//
// The description of the plans (MvDesc: columns, offsets arrays, layouts,
// 5.8 KiB -- more than kernel arguments hold) goes into scratch with a fixed
// number of k_mv_upload launches; every later kernel reads it there.  The two
// tile kernels' bodies are mixed_var_tile.h's mv_pack_tile<false> and
// mv_parse_tile<false>; mixed_legs.hip instantiates them for struct arrays.
//
// Pack:
//   k_mv_sizes   a workgroup per granule of 256 calls: mix_ranks, each lane's
//       frame length from its leg's offsets (u64, a frame saturates at 4 GiB),
//       the granule's total to scratch.
//   k_mv_scan    one workgroup: exclusive scan of the granule totals; the total
//       to *d_total and min(total, out_cap) to d_offs[ncalls].
//   k_mv_pack    a workgroup per tile of T calls.  Frames that lie whole inside
//       the image window (kMixImage bytes from the 16-byte boundary at or under
//       the tile's first byte) are built in LDS: BE32, prefix and fixed fields by
//       the frame's lane (lds_copy_run, lds_put_small), the chars by the whole
//       workgroup, round t moving every frame's t-th string, 8 bytes of the
//       round's chars per lane and step, so no lane's work grows with one
//       string.  The image leaves as aligned 16-byte stores, the chunks shared
//       with neighbouring tiles bytewise.  A frame outside the window goes to
//       global memory directly, by the same code with another destination.
// Decode:
//   k_mv_parse   the tile's span staged into LDS, a lane per frame: the table
//       of srpc_gpu.h by the call's own plan, codes, fixed fields, each string's
//       length into its offsets entry and its chars' stream offset to scratch.
//   k_mv_slot_*  one segmented scan over all string slots (blockIdx.y = slot):
//       reduce, partials (which adds the carry of the chunk before and writes
//       d_ends), apply.  Three launches whatever K.
//   k_mv_copy    a workgroup per granule: the chars, again in rounds by the
//       whole workgroup; nothing at or past a column's capacity is written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "mixed_common.h"
#include "mixed_var_common.h"
#include "mixed_var_tile.h"
#include "plan.h"
#include "srpc_gpu.h"

namespace srpc_impl {
namespace {

constexpr uint32_t kMvScanBlock = 1024;

struct MvChunk {
    uint4 w[kMvChunk / 16];
};

__global__ void k_mv_upload(MvChunk c, uint4* dst, uint32_t words) {
    for (uint32_t i = threadIdx.x; i < words; i += blockDim.x) dst[i] = c.w[i];
}

__global__ __launch_bounds__(kBlock) void k_mv_sizes(const MvDesc* __restrict__ d, const uint8_t* __restrict__ method,
                                                     const uint32_t* __restrict__ table, uint64_t rows, uint64_t ncalls,
                                                     uint64_t* __restrict__ gsum) {
    __shared__ uint32_t wcnt[kMixLds];
    __shared__ uint64_t wsum[kMixWaves];
    const uint64_t g = blockIdx.x;
    const MixLane r = mix_ranks(method, ncalls, d->nplans, table, rows, g, wcnt);
    const MvFrame fr = mv_frame(d, r);
    uint64_t total;
    mv_block_scan(fr.len, wsum, &total);
    if (threadIdx.x == 0) gsum[g] = total;
}

// One workgroup: gsum[0..rows) -> exclusive prefixes, gsum[rows] = the total.
__global__ __launch_bounds__(kMvScanBlock) void k_mv_scan(uint64_t* __restrict__ gsum, uint64_t rows, uint64_t ncalls,
                                                          uint64_t out_cap, uint32_t* __restrict__ offs,
                                                          uint64_t* __restrict__ d_total) {
    __shared__ uint64_t sums[kMvScanBlock];
    const uint64_t per = (rows + kMvScanBlock - 1) / kMvScanBlock;
    const uint64_t r0 = min<uint64_t>(threadIdx.x * per, rows), r1 = min<uint64_t>(r0 + per, rows);
    uint64_t s = 0;
    for (uint64_t r = r0; r < r1; ++r) s += gsum[r];
    sums[threadIdx.x] = s;
    __syncthreads();
    uint64_t run = 0;
    for (uint32_t q = 0; q < threadIdx.x; ++q) run += sums[q];
    if (threadIdx.x == kMvScanBlock - 1) {
        const uint64_t total = run + s;
        gsum[rows] = total;
        *d_total = total;
        offs[ncalls] = static_cast<uint32_t>(min(total, out_cap));
    }
    for (uint64_t r = r0; r < r1; ++r) {
        const uint64_t v = gsum[r];
        gsum[r] = run;
        run += v;
    }
}

__global__ __launch_bounds__(kBlock) void k_mv_pack(const MvDesc* __restrict__ d, const uint8_t* __restrict__ method,
                                                    const uint32_t* __restrict__ table, uint64_t rows, uint64_t ncalls,
                                                    const uint64_t* __restrict__ gsum, uint8_t* __restrict__ out,
                                                    uint64_t out_cap, uint32_t* __restrict__ offs,
                                                    srpc_unpack_status* st) {
    mv_pack_tile<false>(d, nullptr, method, table, rows, ncalls, gsum, out, out_cap, offs, st);
}

__global__ __launch_bounds__(kBlock) void k_mv_parse(const MvDesc* __restrict__ d, const uint8_t* __restrict__ method,
                                                     const uint32_t* __restrict__ table, uint64_t rows, uint64_t ncalls,
                                                     const uint8_t* __restrict__ buf, uint64_t buf_len,
                                                     const uint32_t* __restrict__ offs, uint64_t nframes,
                                                     uint32_t unanswered, uint8_t* __restrict__ codes,
                                                     uint32_t* __restrict__ srcs, uint32_t* __restrict__ counts,
                                                     srpc_unpack_status* st) {
    mv_parse_tile<false>(d, nullptr, nullptr, method, table, rows, ncalls, buf, buf_len, offs, nframes, unanswered, codes,
                         srcs, counts, st);
}

struct MvSlot {
    uint64_t* arr;   // the slot's offsets array
    uint64_t first;  // entries first + 1 .. first + n hold this chunk's lengths
    uint64_t n;
};

__device__ __forceinline__ MvSlot mv_slot(const MvDesc* __restrict__ d, const uint32_t* __restrict__ counts,
                                          uint64_t ncalls, uint32_t s) {
    const uint32_t f = d->slot_leaf[s], k = d->leaf_plan[f];
    MvSlot x;
    x.arr = d->soffs[f];
    x.first = d->first[k];
    x.n = ncalls ? min(counts[k], d->room[k]) : 0;
    return x;
}

__global__ __launch_bounds__(kBlock) void k_mv_slot_reduce(const MvDesc* __restrict__ d,
                                                           const uint32_t* __restrict__ counts, uint64_t ncalls,
                                                           uint64_t* __restrict__ partial, uint32_t nb) {
    __shared__ uint64_t wsum[kMixWaves];
    const MvSlot x = mv_slot(d, counts, ncalls, blockIdx.y);
    const uint64_t b0 = static_cast<uint64_t>(blockIdx.x) * kMvSlotBlock;
    uint64_t s = 0;
    for (uint32_t u = 0; u < kMvSlotItems; ++u) {
        const uint64_t idx = b0 + u * kBlock + threadIdx.x;
        if (idx < x.n) s += x.arr[x.first + 1 + idx];
    }
    uint64_t total;
    mv_block_scan(s, wsum, &total);
    if (threadIdx.x == 0) partial[static_cast<uint64_t>(blockIdx.y) * nb + blockIdx.x] = total;
}

// A workgroup per slot: its partials -> exclusive prefixes, starting from the
// offset the chunk before ended at; the slot's end to ends[s].
__global__ __launch_bounds__(kBlock) void k_mv_slot_partials(const MvDesc* __restrict__ d,
                                                             const uint32_t* __restrict__ counts, uint64_t ncalls,
                                                             uint64_t* __restrict__ partial, uint32_t nb,
                                                             uint64_t* __restrict__ ends) {
    __shared__ uint64_t wsum[kMixWaves];
    const MvSlot x = mv_slot(d, counts, ncalls, blockIdx.x);
    uint64_t* pp = partial + static_cast<uint64_t>(blockIdx.x) * nb;
    uint64_t carry = x.first ? x.arr[x.first] : 0;
    for (uint32_t b0 = 0; b0 < nb; b0 += kBlock) {
        const uint32_t b = b0 + threadIdx.x;
        const uint64_t v = b < nb ? pp[b] : 0;
        uint64_t total;
        const uint64_t at = mv_block_scan(v, wsum, &total);
        if (b < nb) pp[b] = carry + at;
        carry += total;
    }
    if (threadIdx.x == 0) {
        ends[blockIdx.x] = carry;
        if (!x.first) x.arr[0] = 0;
    }
}

__global__ __launch_bounds__(kBlock) void k_mv_slot_apply(const MvDesc* __restrict__ d,
                                                          const uint32_t* __restrict__ counts, uint64_t ncalls,
                                                          const uint64_t* __restrict__ partial, uint32_t nb) {
    __shared__ uint64_t wsum[kMixWaves];
    const MvSlot x = mv_slot(d, counts, ncalls, blockIdx.y);
    const uint64_t b0 = static_cast<uint64_t>(blockIdx.x) * kMvSlotBlock + static_cast<uint64_t>(threadIdx.x) * kMvSlotItems;
    if (static_cast<uint64_t>(blockIdx.x) * kMvSlotBlock >= x.n) return;  // the whole workgroup
    uint64_t v[kMvSlotItems], s = 0;
    for (uint32_t u = 0; u < kMvSlotItems; ++u) {
        v[u] = b0 + u < x.n ? x.arr[x.first + 1 + b0 + u] : 0;
        s += v[u];
    }
    uint64_t total;
    uint64_t run = partial[static_cast<uint64_t>(blockIdx.y) * nb + blockIdx.x] + mv_block_scan(s, wsum, &total);
    for (uint32_t u = 0; u < kMvSlotItems; ++u) {
        run += v[u];
        if (b0 + u < x.n) x.arr[x.first + 1 + b0 + u] = run;
    }
}

__global__ __launch_bounds__(kBlock) void k_mv_copy(const MvDesc* __restrict__ d, const uint8_t* __restrict__ method,
                                                    const uint32_t* __restrict__ table, uint64_t rows, uint64_t ncalls,
                                                    const uint8_t* __restrict__ buf, const uint32_t* __restrict__ srcs) {
    __shared__ uint32_t wcnt[kMixLds];
    __shared__ uint64_t wsum[kMixWaves];
    __shared__ uint64_t rel[kBlock + 1];
    __shared__ const uint8_t* rsrc[kBlock];
    __shared__ uint64_t rdst[kBlock];
    const uint32_t K = d->nplans;
    const uint64_t g = blockIdx.x;
    const uint64_t i = g * kMixGranule + threadIdx.x;
    const MixLane r = mix_ranks(method, ncalls, K, table, rows, g, wcnt);
    const bool good = r.cls < K && r.rank < d->room[r.cls];
    const uint32_t k = good ? r.cls : 0;
    const uint64_t e = good ? d->first[k] + r.rank : 0;
    const uint32_t ns = good ? d->nstr[k] : 0;
    for (uint32_t t = 0; t < d->maxstr; ++t) {
        uint64_t rl = 0, rd = 0;
        const uint8_t* rs = nullptr;
        if (t < ns) {
            const uint32_t f = d->str_leaf[k * kMvStr + t];
            const uint64_t a = d->soffs[f][e], b = d->soffs[f][e + 1];
            const uint64_t room = a < d->scap[f] ? d->scap[f] - a : 0;  // nothing at or past the column's capacity
            rl = min(b - a, room);
            rs = buf + srcs[t * ncalls + i];
            rd = reinterpret_cast<uint64_t>(d->col[f] + a);
        }
        uint64_t total;
        const uint64_t at = mv_block_scan(rl, wsum, &total);
        rel[threadIdx.x] = at;
        if (threadIdx.x == 0) rel[kBlock] = total;
        rsrc[threadIdx.x] = rs;
        rdst[threadIdx.x] = rd;
        __syncthreads();
        mv_copy_runs(rel, rsrc, rdst, nullptr);
        __syncthreads();
    }
}

}  // namespace

// ---- host side ----

// The plans of one side into d's layout part.  min_fixed_prefix: 4 (request) or
// 5 (reply).
int mv_plans(const srpc_plan* const* plans, int nplans, uint32_t min_fixed_prefix, MvDesc* d) {
    uint32_t nf = 0, tb = 0, fmax = 0, ns = 0, maxstr = 0;
    for (int k = 0; k < nplans; ++k)
        if (!plans[k]) return SRPC_E_INVALID;
    for (int k = 0; k < nplans; ++k) {
        const srpc_plan* p = plans[k];
        if (p->has_string ? (p->prefix_len < 1 || p->nstrings > static_cast<uint32_t>(kMvStr))
                          : p->prefix_len < min_fixed_prefix)
            return SRPC_E_UNSUPPORTED;
        nf += p->nfields;
    }
    if (nf > static_cast<uint32_t>(kMixFields)) return SRPC_E_UNSUPPORTED;
    nf = 0;
    for (int k = 0; k < nplans; ++k) {
        const srpc_plan* p = plans[k];
        d->field0[k] = static_cast<uint16_t>(nf);
        uint32_t t = 0;
        for (uint32_t f = 0; f < p->nfields; ++f, ++nf) {
            d->size[nf] = static_cast<uint8_t>(p->size[f]);
            d->leaf_plan[nf] = static_cast<uint8_t>(k);
            if (p->size[f] == 0) {
                d->slot_leaf[ns++] = static_cast<uint8_t>(nf);
                d->str_leaf[k * kMvStr + t++] = static_cast<uint8_t>(nf);
            }
        }
        d->prefix[k] = p->d_prefix;
        d->var[k] = p->has_string;
        d->nstr[k] = static_cast<uint8_t>(t);
        d->F[k] = p->has_string ? 4 + p->fixed_bytes : static_cast<uint32_t>(p->stride);
        d->prefix_len[k] = static_cast<uint16_t>(p->prefix_len);
        d->tmpl[k] = static_cast<uint16_t>(tb);
        tb += (p->prefix_len + 7) & ~7u;
        fmax = std::max(fmax, d->F[k]);
        maxstr = std::max(maxstr, t);
    }
    d->field0[nplans] = static_cast<uint16_t>(nf);
    d->nplans = static_cast<uint32_t>(nplans);
    d->nslots = ns;
    d->maxstr = maxstr;
    d->T = mix_tile(fmax);
    d->tmpl_bytes = tb;
    return SRPC_OK;
}

// Columns, offsets arrays and rooms.
int mv_cols(const srpc_plan* const* plans, int nplans, const void* const* const* d_cols,
            const uint64_t* const* const* d_str_offs, const uint64_t* const* h_str_cap, const uint64_t* h_first,
            const uint64_t* h_cap, MvDesc* d, const uint64_t* h_stride) {
    uint32_t nf = 0;
    for (int k = 0; k < nplans; ++k) {
        const srpc_plan* p = plans[k];
        // a first past the capacity leaves no element, as first == capacity does: every call of
        // the plan is BAD, and the slot scan's carry stays inside the cap + 1 offsets entries
        const uint64_t first = std::min(h_first ? h_first[k] : 0, h_cap[k]);
        const uint64_t room = h_cap[k] - first;
        d->first[k] = first;
        d->room[k] = static_cast<uint32_t>(std::min<uint64_t>(room, 0xffffffffull));
        if (h_stride && h_stride[k]) {  // a record plan: its leaves are the caller's to fill in
            nf += p->nfields;
            continue;
        }
        if (!d_cols[k] || (p->has_string && (!d_str_offs[k] || (h_str_cap && !h_str_cap[k])))) return SRPC_E_INVALID;
        for (uint32_t f = 0; f < p->nfields; ++f, ++nf) {
            const void* c = d_cols[k][f];
            const bool str = p->size[f] == 0;
            const uint64_t* so = str ? d_str_offs[k][f] : nullptr;
            if (str && !so) return SRPC_E_INVALID;
            if (room && !c && !str) return SRPC_E_INVALID;
            if (!aligned(c, 16) || !aligned(so, 8)) return SRPC_E_ALIGN;
            d->col[nf] = static_cast<uint8_t*>(const_cast<void*>(c));
            d->soffs[nf] = const_cast<uint64_t*>(so);
            d->scap[nf] = str && h_str_cap ? h_str_cap[k][f] : 0;
        }
    }
    return SRPC_OK;
}

int mix_upload(const void* src, size_t bytes, void* d_scratch, hipStream_t s) {
    for (size_t at = 0; at < bytes; at += kMvChunk) {
        MvChunk ch;
        const size_t nbytes = std::min<size_t>(kMvChunk, bytes - at);
        std::memset(&ch, 0, sizeof ch);
        std::memcpy(&ch, static_cast<const uint8_t*>(src) + at, nbytes);
        launch(k_mv_upload, dim3(1), dim3(128), 0, s, ch, reinterpret_cast<uint4*>(static_cast<uint8_t*>(d_scratch) + at),
               static_cast<uint32_t>(nbytes / 16));
    }
    return hipGetLastError() == hipSuccess ? SRPC_OK : SRPC_E_HIP;
}

void mv_sizes_launch(const MvDesc* dd, const uint8_t* d_method, const uint32_t* table, uint64_t rows, uint64_t ncalls,
                     uint64_t* gsum, uint64_t out_cap, uint32_t* d_offs, uint64_t* d_total, hipStream_t s) {
    if (rows)
        launch(k_mv_sizes, dim3(static_cast<uint32_t>(rows)), dim3(kBlock), 0, s, dd, d_method, table, rows, ncalls, gsum);
    launch(k_mv_scan, dim3(1), dim3(kMvScanBlock), 0, s, gsum, rows, ncalls, out_cap, d_offs, d_total);
}

void mv_pack_launch(const MvDesc& d, const MvDesc* dd, const uint8_t* d_method, const uint32_t* table, uint64_t rows,
                    uint64_t ncalls, const uint64_t* gsum, uint8_t* d_out, uint64_t out_cap, uint32_t* d_offs,
                    srpc_unpack_status* d_status, hipStream_t s) {
    launch(k_mv_pack, dim3(static_cast<uint32_t>((ncalls + d.T - 1) / d.T)), dim3(kBlock), mv_lds(d), s, dd, d_method, table,
           rows, ncalls, gsum, d_out, out_cap, d_offs, d_status);
}

void mv_parse_launch(const MvDesc& d, const MvDesc* dd, const uint8_t* d_method, const uint32_t* table, uint64_t rows,
                     uint64_t ncalls, const uint8_t* d_buf, uint64_t buf_len, const uint32_t* d_offs, uint64_t nframes,
                     uint32_t unanswered, uint8_t* d_codes, uint32_t* srcs, uint32_t* counts, srpc_unpack_status* d_status,
                     hipStream_t s) {
    launch(k_mv_parse, dim3(static_cast<uint32_t>((ncalls + d.T - 1) / d.T)), dim3(kBlock), mv_lds(d), s, dd, d_method,
           table, rows, ncalls, d_buf, buf_len, d_offs, nframes, unanswered, d_codes, srcs, counts, d_status);
}

int mv_strings_launch(const MvDesc& d, const MvCarve& c, uint32_t nb, const uint8_t* d_method, const uint32_t* table,
                      uint64_t ncalls, const uint8_t* d_buf, uint64_t* d_ends, hipStream_t s) {
    const uint64_t rows = mix_rows(ncalls);
    if (d.nslots) {
        launch(k_mv_slot_reduce, dim3(nb, d.nslots), dim3(kBlock), 0, s, c.dd, c.counts, ncalls, c.partial, nb);
        launch(k_mv_slot_partials, dim3(d.nslots), dim3(kBlock), 0, s, c.dd, c.counts, ncalls, c.partial, nb, d_ends);
        launch(k_mv_slot_apply, dim3(nb, d.nslots), dim3(kBlock), 0, s, c.dd, c.counts, ncalls, c.partial, nb);
        if (ncalls)
            launch(k_mv_copy, dim3(static_cast<uint32_t>(rows)), dim3(kBlock), 0, s, c.dd, d_method, table, rows, ncalls,
                   d_buf, c.srcs);
    }
    return hipGetLastError() == hipSuccess ? SRPC_OK : SRPC_E_HIP;
}

}  // namespace srpc_impl
