// mixed_aos_common.h -- internal: what the two arrival-order decodes into struct
// arrays share (mixed_aos.hip: replies, the class of a call given by the caller;
// mixed_req_aos.hip: requests, the class found from the frame): the kernels'
// struct-array arguments, the tables and fills as they lie in scratch and LDS,
// the tile, the argument checks, and the step that turns a tile's judged frames
// into whole 16-byte pieces of the K arrays (mix_aos_slices_*, mix_aos_store).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "aos_pieces.h"
#include "mixed_common.h"
#include "plan.h"
#include "srpc_gpu.h"

namespace srpc_impl {

struct MixAos {
    uint8_t* recs[kMixPlans];     // plan k's struct array
    uint32_t stride[kMixPlans];   // struct bytes
    uint16_t tab[kMixPlans];      // byte offset of plan k's table inside the description
    uint16_t fill[kMixPlans];     // ... of its fill record
    uint32_t desc_bytes;          // tables and fills (a multiple of 16)
};

// Table and fill bytes of the plans' strides: 2 S16 + S16 + 16 each.  A plan
// without a table is skipped, here and in aos_describe: stride 0 (a column plan
// of mixed_legs_common.h) or above kAosMaxStride (a pack's: decodes refuse it).
inline bool aos_has_table(uint64_t stride) { return stride && stride <= kAosMaxStride; }
inline uint32_t aos_desc_bytes(const uint64_t* h_stride, int nplans) {
    uint32_t b = 0;
    for (int k = 0; k < nplans; ++k)
        if (aos_has_table(h_stride[k])) b += 3 * s16_of(static_cast<uint32_t>(h_stride[k])) + 16;
    return b;
}

// Calls per tile of the decode: mix_tile with the tables and fills taken out of
// the image's budget, so image + tables + fills stay within the column kernel's
// image (at the floor of 16 calls: 16 * 1280 + 12.5 KiB, still under 33 KiB).
inline uint32_t mix_aos_tile(uint32_t fmax, uint32_t desc_bytes) { return mix_tile(fmax, kMixImage - desc_bytes); }

// The arguments every struct-array call shares, checked before any plan is read.
inline bool aos_args_invalid(const void* const* d_recs, const uint64_t* h_stride, const uint32_t* const* h_leaf_offs,
                             const uint64_t* h_first, const uint64_t* h_cap, int nplans) {
    for (int k = 0; k < nplans; ++k) {
        if (h_stride[k] == 0 || h_stride[k] >= (1ull << 32) || !h_leaf_offs[k]) return true;
        const uint64_t first = h_first ? h_first[k] : 0;
        if (h_cap[k] > first && !d_recs[k]) return true;
    }
    return false;
}

// Every leaf inside the stride and no two sharing a byte (any stride below 2^32).
inline int aos_leaves_ok(const srpc_plan* p, const uint32_t* offs, uint64_t stride) {
    for (uint32_t f = 0; f < p->nfields; ++f) {
        if (offs[f] + static_cast<uint64_t>(p->size[f]) > stride) return SRPC_E_INVALID;
        for (uint32_t g = 0; g < f; ++g)
            if (offs[f] < offs[g] + static_cast<uint64_t>(p->size[g]) && offs[g] < offs[f] + static_cast<uint64_t>(p->size[f]))
                return SRPC_E_INVALID;
    }
    return SRPC_OK;
}

// Every struct array (h_stride[k] != 0) on a 16-byte boundary, its layout naturally aligned.
inline bool aos_recs_aligned(const srpc_plan* const* plans, int nplans, const void* const* d_recs,
                             const uint64_t* h_stride, const uint32_t* const* h_leaf_offs) {
    for (int k = 0; k < nplans; ++k)
        if (h_stride[k] && (!aligned(d_recs[k], 16) || !aos_layout_aligned(plans[k], h_leaf_offs[k], h_stride[k])))
            return false;
    return true;
}

// Each leaf's address inside element 0 of its plan's array, as mix_args's columns.
struct AosCols {
    const void* leaf[kMixFields];
    const void* const* plan[kMixPlans];
};

inline void aos_cols(const srpc_plan* const* plans, int nplans, const void* const* d_recs,
                     const uint32_t* const* h_leaf_offs, AosCols* c) {
    uint32_t nf = 0;
    for (int k = 0; k < nplans; ++k) {
        c->plan[k] = c->leaf + nf;
        for (uint32_t f = 0; f < plans[k]->nfields; ++f)
            c->leaf[nf++] = static_cast<const uint8_t*>(d_recs[k]) + h_leaf_offs[k][f];
    }
}

// The tables and the fills of the plans that have them, as they will lie in
// scratch and in LDS, and the kernel's view of them (*x comes in zeroed: a plan
// without a table keeps stride 0).  SRPC_E_INVALID: as aos_sources.
struct AosDesc {
    alignas(16) uint8_t bytes[kMixPlans * (3 * kAosMaxStride + 16)];
};

inline int aos_describe(const srpc_plan* const* plans, int nplans, void* const* d_recs, const uint64_t* h_stride,
                        const uint32_t* const* h_leaf_offs, const void* const* h_fill, AosDesc* desc, MixAos* x) {
    std::memset(desc->bytes, 0, sizeof(desc->bytes));
    x->desc_bytes = aos_desc_bytes(h_stride, nplans);
    uint32_t at = 0;
    for (int k = 0; k < nplans; ++k) {
        if (!aos_has_table(h_stride[k])) continue;
        const uint32_t stride = static_cast<uint32_t>(h_stride[k]);
        int32_t from[kAosMaxStride];
        if (int rc = aos_sources(plans[k], h_leaf_offs[k], stride, from)) return rc;
        aos_run_table(from, stride, reinterpret_cast<uint16_t*>(desc->bytes + at));
        x->tab[k] = static_cast<uint16_t>(at);
        at += 2 * s16_of(stride);
    }
    for (int k = 0; k < nplans; ++k) {
        if (!aos_has_table(h_stride[k])) continue;
        const uint32_t stride = static_cast<uint32_t>(h_stride[k]);
        std::memcpy(desc->bytes + at, h_fill[k], stride);
        x->fill[k] = static_cast<uint16_t>(at);
        x->recs[k] = static_cast<uint8_t*>(d_recs[k]);
        x->stride[k] = stride;
        at += s16_of(stride) + 16;
    }
    return SRPC_OK;
}

// ---- a tile's slices of the K arrays ----
//
// Within a tile the good calls of plan k are consecutive ranks, so they are one
// contiguous slice of plan k's array.  Static LDS of the kernel that uses them.
struct MixAosSlices {
    uint64_t byte0[kMixPlans];      // the slice's first byte inside the array
    uint8_t* recs[kMixPlans];
    uint32_t first[kMixPlans];      // rank of the slice's first call
    uint32_t count[kMixPlans];      // its calls
    uint32_t base[kMixPlans];       // its first entry of slot[]
    uint32_t pbase[kMixPlans + 1];  // its first (plan, piece) pair
    uint32_t stride[kMixPlans];
    uint16_t tab[kMixPlans], fill[kMixPlans];
};

// Complete after the next barrier.
__device__ __forceinline__ void mix_aos_slices_init(MixAosSlices& s, const MixAos& x, uint32_t K) {
    if (threadIdx.x < K) {
        const uint32_t k = threadIdx.x;
        s.recs[k] = x.recs[k];
        s.stride[k] = x.stride[k];
        s.tab[k] = x.tab[k];
        s.fill[k] = x.fill[k];
        s.first[k] = 0xffffffffu;
        s.count[k] = 0;
    }
}

// Every wave's ballots leave the slices' first ranks and counts (ranks ascend
// with the lane).  After the barrier that follows mix_aos_slices_init; complete
// after the next one.
__device__ __forceinline__ void mix_aos_slices_count(MixAosSlices& s, uint32_t K, const MixLane& r, bool good) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t k = 0; k < K; ++k) {
        const uint64_t b = __ballot(good && r.cls == k);
        if (b) {
            const uint32_t rk = __shfl(r.rank, __ffsll(static_cast<long long>(b)) - 1, 64);
            if (lane == 0) {
                atomicMin(&s.first[k], rk);
                atomicAdd(&s.count[k], static_cast<uint32_t>(__popcll(b)));
            }
        }
    }
}

// Image, zero and fill -> the slices.  Every good lane j (of the tile) has left
// pos[j]: its frame's image position, kPosGlobal (a full frame at buf + lo[j])
// or kPosZero (its leaves are zero), and a barrier has passed since
// mix_aos_slices_count.  Every lane gets its slot (slice position -> lane); the
// workgroup then takes (plan, 16-byte piece) pairs over the K slices: a piece is
// assembled run by run through plan k's per-struct-byte table (aos_pieces.h)
// and stored whole, non-temporally when NT.  A slice starts and ends at any
// byte: its first and last piece, where they are shared with a neighbouring
// tile's slice (or lie at the array's edge), are stored bytewise, own bytes
// only.  dsc: the K tables and fills in LDS.  d: the kernel's plan lookups
// (MixLds, or MvDesc in mixed_var_tile.h), of which first[] is read.
template <bool NT, class D>
__device__ __forceinline__ void mix_aos_store(MixAosSlices& s, const D& d, uint32_t K, const MixLane& r, bool good,
                                              uint32_t j, const uint8_t* img, const uint32_t* lo, const uint32_t* pos,
                                              uint16_t* slot, const uint8_t* dsc, const uint8_t* __restrict__ buf) {
    if (threadIdx.x <= K) {
        uint32_t sb = 0, pb = 0;
        for (uint32_t q = 0; q < threadIdx.x; ++q) {
            const uint32_t n = s.count[q];
            const uint64_t b0 = (d.first[q] + s.first[q]) * s.stride[q];
            sb += n;
            pb += n ? static_cast<uint32_t>(((b0 & 15) + static_cast<uint64_t>(n) * s.stride[q] + 15) >> 4) : 0;
        }
        s.pbase[threadIdx.x] = pb;
        if (threadIdx.x < K) {
            s.base[threadIdx.x] = sb;
            s.byte0[threadIdx.x] =
                s.count[threadIdx.x] ? (d.first[threadIdx.x] + s.first[threadIdx.x]) * s.stride[threadIdx.x] : 0;
        }
    }
    __syncthreads();
    if (good) slot[s.base[r.cls] + (r.rank - s.first[r.cls])] = static_cast<uint16_t>(j);
    __syncthreads();

    const uint32_t total = s.pbase[K];
    for (uint32_t xx = threadIdx.x; xx < total; xx += kBlock) {
        uint32_t k = 0;
        for (uint32_t q = 1; q < K; ++q) k = s.pbase[q] <= xx ? q : k;
        const uint32_t stride = s.stride[k];
        const uint64_t B0 = s.byte0[k];
        const uint32_t a0 = static_cast<uint32_t>(B0 & 15);
        const uint32_t nbytes = s.count[k] * stride;    // <= 256 * 256
        const uint32_t p0 = 16 * (xx - s.pbase[k]);     // the piece, from the slice's first piece on
        const uint32_t x0 = p0 > a0 ? p0 - a0 : 0;      // its first byte of the slice
        const uint32_t x1 = min(p0 + 16 - a0, nbytes);  // ... and past its last
        const uint32_t b0 = x0 + a0 - p0, b1 = x1 + a0 - p0;  // the same, inside the piece
        const uint16_t* tab = reinterpret_cast<const uint16_t*>(dsc + s.tab[k]);
        const uint8_t* fill = dsc + s.fill[k];
        const uint16_t* sl = slot + s.base[k];
        uint32_t e = x0 / stride;
        uint32_t kk = x0 - e * stride;
        uint32_t jj = sl[e];
        uint32_t p = pos[jj];
        uint64_t vlo = 0, vhi = 0;
        uint32_t b = b0;
        while (b < b1) {
            const uint32_t t = tab[kk];
            const uint32_t m = min(t >> 12, b1 - b), w = t & 0xfff;
            uint64_t v = 0;
            if (w == kSrcFill) {
                v = lds_u64(fill, kk);
            } else if (p < kPosGlobal) {
                v = lds_u64(img, p + w);
            } else if (p == kPosGlobal) {
                const uint8_t* gp = buf + lo[jj] + w;  // inside the frame: w + m <= F
                for (uint32_t y = 0; y < m; ++y) v |= static_cast<uint64_t>(gp[y]) << (8 * y);
            }
            piece_put(vlo, vhi, b, v, m);
            b += m;
            kk += m;
            if (kk == stride) {  // runs end with their struct
                kk = 0;
                ++e;
                if (b < b1) {  // b < b1 keeps e inside the slice
                    jj = sl[e];
                    p = pos[jj];
                }
            }
        }
        uint8_t* dst = s.recs[k] + (B0 - a0) + p0;
        if (b1 - b0 == 16) {
            const aos_u32x4 v{static_cast<uint32_t>(vlo), static_cast<uint32_t>(vlo >> 32), static_cast<uint32_t>(vhi),
                              static_cast<uint32_t>(vhi >> 32)};
            if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<aos_u32x4*>(dst));
            else *reinterpret_cast<aos_u32x4*>(dst) = v;
        } else {  // a slice's first or last piece: its own bytes only
            for (uint32_t y = b0; y < b1; ++y)
                dst[y] = static_cast<uint8_t>(y < 8 ? vlo >> (8 * y) : vhi >> (8 * (y - 8)));
        }
    }
}

}  // namespace srpc_impl
