// mixed_var_common.h -- internal: what mixed_var.hip (client side: request pack,
// reply decode), mixed_req_var.hip (server side: request decode) and the two
// files over plans of both kinds (mixed_legs.hip, mixed_req_legs.hip) share: the
// description of the plans that they put into scratch (MvDesc), its host-side
// builders, the scratch layout, and the launches of the kernels that stay in
// mixed_var.hip -- the description upload, the segmented scan over the string
// slots and the char copy.
#pragma once

#include <algorithm>
#include <cstdint>

#include "mixed_common.h"
#include "plan.h"
#include "srpc_gpu.h"

namespace srpc_impl {

constexpr int kMvStr = SRPC_FRAMES_MAX_STRINGS;
constexpr uint32_t kMvSlotItems = 8;
constexpr uint32_t kMvSlotBlock = kBlock * kMvSlotItems;  // offsets entries per workgroup of the slot scan

struct alignas(16) MvDesc {
    uint8_t* col[kMixFields];         // plan k's leaves: [field0[k], field0[k + 1])
    uint64_t* soffs[kMixFields];      // a string leaf's offsets, else nullptr
    uint64_t scap[kMixFields];        // decode: bytes a string column has
    uint8_t size[kMixFields];         // 0: a string
    uint8_t leaf_plan[kMixFields];
    uint8_t slot_leaf[kMixFields];    // string slot -> leaf
    uint8_t str_leaf[kMixPlans * kMvStr];  // plan k's t-th string -> leaf
    const uint8_t* prefix[kMixPlans];
    uint64_t first[kMixPlans];
    uint32_t room[kMixPlans];
    uint32_t F[kMixPlans];            // fixed plan: frame bytes; string plan: the frame without its chars
    uint16_t prefix_len[kMixPlans];
    uint16_t tmpl[kMixPlans];         // LDS offset of plan k's prefix template
    uint16_t field0[kMixPlans + 1];
    uint8_t var[kMixPlans];
    uint8_t nstr[kMixPlans];
    uint32_t nplans;
    uint32_t nslots;
    uint32_t maxstr;                  // max_k nstr[k]
    uint32_t T;                       // calls per tile (divides kMixGranule)
    uint32_t tmpl_bytes;
};
static_assert(sizeof(MvDesc) % 16 == 0, "uploaded in 16-byte words");

constexpr uint32_t kMvChunk = 2048;
constexpr uint32_t kMvChunks = (sizeof(MvDesc) + kMvChunk - 1) / kMvChunk;

// The K prefixes into LDS at dst + d->tmpl[k].
__device__ __forceinline__ void mv_templates(uint8_t* dst, const MvDesc* __restrict__ d) {
    for (uint32_t k = 0; k < d->nplans; ++k) {
        const uint8_t* src = d->prefix[k];
        for (uint32_t b = threadIdx.x; b < d->prefix_len[k]; b += kBlock) dst[d->tmpl[k] + b] = src[b];
    }
}

// u64 of the k <= 8 bytes at p (LDS or global: a generic pointer), little-endian.
__device__ __forceinline__ uint64_t mv_get(const uint8_t* p, uint32_t k) {
    uint64_t v = 0;
    for (uint32_t b = 0; b < k; ++b) v |= static_cast<uint64_t>(p[b]) << (8 * b);
    return v;
}

// Scratch: desc | gsum[rows + 1] | counts[kMixPlans] | partial[nslots * nb] | srcs[maxstr * ncalls]
struct MvScratch {
    uint64_t gsum, counts, partial, srcs, bytes;
    uint32_t nb;
};

inline MvScratch mv_scratch(const MvDesc& d, uint64_t ncalls) {
    MvScratch s;
    s.nb = static_cast<uint32_t>(std::max<uint64_t>(1, (ncalls + kMvSlotBlock - 1) / kMvSlotBlock));
    uint64_t at = kMvChunks * kMvChunk;
    s.gsum = at;
    at += 8 * (mix_rows(ncalls) + 1);
    s.counts = at;
    at += 4 * kMixPlans;
    s.partial = at;
    at += 8ull * d.nslots * s.nb;
    s.srcs = at;
    at += (4ull * d.maxstr * ncalls + 7) & ~7ull;
    s.bytes = at;
    return s;
}

// What a call takes out of its scratch.
struct MvCarve {
    const MvDesc* dd;
    uint64_t *gsum, *partial;
    uint32_t *counts, *srcs;
    MvCarve(void* p, const MvScratch& sc)
        : dd(static_cast<const MvDesc*>(p)), gsum(at<uint64_t>(p, sc.gsum)), partial(at<uint64_t>(p, sc.partial)),
          counts(at<uint32_t>(p, sc.counts)), srcs(at<uint32_t>(p, sc.srcs)) {}
    template <class T>
    static T* at(void* p, uint64_t off) { return reinterpret_cast<T*>(static_cast<uint8_t*>(p) + off); }
};

// Dynamic LDS of a kernel with the image and the templates.
inline size_t mv_lds(const MvDesc& d) { return kMixImage + 16 + d.tmpl_bytes + 16; }

// ---- mixed_var.hip ----
// The plans of one side into d's layout part.  min_fixed_prefix: 4 (request) or
// 5 (reply).
int mv_plans(const srpc_plan* const* plans, int nplans, uint32_t min_fixed_prefix, MvDesc* d);
// Columns, offsets arrays and rooms.  A plan with h_stride[k] != 0 (h_stride
// may be nullptr) gets its first and room only: its d_cols[k], d_str_offs[k]
// and h_str_cap[k] are not read and its leaves' entries are left to the caller
// (mixed_legs.hip: a record plan).
int mv_cols(const srpc_plan* const* plans, int nplans, const void* const* const* d_cols,
            const uint64_t* const* const* d_str_offs, const uint64_t* const* h_str_cap, const uint64_t* h_first,
            const uint64_t* h_cap, MvDesc* d, const uint64_t* h_stride = nullptr);
// Any description (MvDesc; bytes: a multiple of 16) -> the head of d_scratch (16-byte
// aligned), kMvChunk bytes per launch, each chunk a by-value kernel argument:
// no host copy outlives the call (also mixed_aos.hip's tables and fills).
int mix_upload(const void* src, size_t bytes, void* d_scratch, hipStream_t s);
// The pack's first two launches: every granule's frame bytes, then their scan
// (gsum: rows + 1 u64 of scratch; the total to *d_total, d_offs[ncalls]).
void mv_sizes_launch(const MvDesc* dd, const uint8_t* d_method, const uint32_t* table, uint64_t rows, uint64_t ncalls,
                     uint64_t* gsum, uint64_t out_cap, uint32_t* d_offs, uint64_t* d_total, hipStream_t s);
// The two tile kernels over plans that all live in columns (k_mv_pack,
// k_mv_parse: d.T calls a workgroup), ncalls > 0.  mixed_legs.hip launches them
// too, for a batch without a record plan.
void mv_pack_launch(const MvDesc& d, const MvDesc* dd, const uint8_t* d_method, const uint32_t* table, uint64_t rows,
                    uint64_t ncalls, const uint64_t* gsum, uint8_t* d_out, uint64_t out_cap, uint32_t* d_offs,
                    srpc_unpack_status* d_status, hipStream_t s);
void mv_parse_launch(const MvDesc& d, const MvDesc* dd, const uint8_t* d_method, const uint32_t* table, uint64_t rows,
                     uint64_t ncalls, const uint8_t* d_buf, uint64_t buf_len, const uint32_t* d_offs, uint64_t nframes,
                     uint32_t unanswered, uint8_t* d_codes, uint32_t* srcs, uint32_t* counts, srpc_unpack_status* d_status,
                     hipStream_t s);
// The tail of every decode.  The segmented scan over all string slots (three
// launches whatever K): the lengths the parse left in the offsets arrays become
// offsets, d_ends[s] each slot's end.  Then the chars of every good call, from
// buf + c.srcs[t * ncalls + i] into the columns.  Returns the call's code.
int mv_strings_launch(const MvDesc& d, const MvCarve& c, uint32_t nb, const uint8_t* d_method, const uint32_t* table,
                      uint64_t ncalls, const uint8_t* d_buf, uint64_t* d_ends, hipStream_t s);

}  // namespace srpc_impl
