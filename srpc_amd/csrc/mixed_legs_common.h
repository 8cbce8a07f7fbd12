// mixed_legs_common.h -- internal: the host side that the calls over plans of
// both kinds share (mixed_legs.hip: the client's request pack and reply decode;
// mixed_req_legs.hip: the server's request decode): which plans are record
// plans (h_stride[k] != 0), the checks of their arguments, their leaves as
// columns of MvDesc, their description (legs_describe) and its place in scratch.
#pragma once

#include <algorithm>
#include <cstdint>

#include "aos_pieces.h"
#include "mixed_aos_common.h"
#include "mixed_common.h"
#include "mixed_var_common.h"
#include "mixed_var_tile.h"
#include "plan.h"
#include "srpc_gpu.h"

namespace srpc_impl {

// h_stride of a call without record arguments: every plan in columns.
constexpr uint64_t kAllColumns[kMixPlans] = {};

// What is checked of the struct-array arguments before any plan is read.
inline bool legs_args_invalid(const void* const* d_recs, const uint64_t* h_stride, const uint32_t* const* h_leaf_offs,
                              const void* const* h_fill, bool decode, const uint64_t* h_first, const uint64_t* h_cap,
                              int nplans) {
    if (any_null(d_recs, h_stride, h_leaf_offs) || (decode && !h_fill)) return true;
    for (int k = 0; k < nplans; ++k) {
        if (h_stride[k] >= (1ull << 32)) return true;
        if (!h_stride[k]) continue;
        if (!h_leaf_offs[k] || (decode && !h_fill[k])) return true;
        const uint64_t first = h_first ? h_first[k] : 0;
        if (h_cap[k] > first && !d_recs[k]) return true;
    }
    return false;
}

// A record plan is a fixed-size plan (mv_plans has passed: its prefix is framed).
inline int legs_plans_ok(const srpc_plan* const* plans, int nplans, const uint64_t* h_stride, bool decode) {
    for (int k = 0; k < nplans; ++k)
        if (h_stride && h_stride[k] && (plans[k]->has_string || (decode && h_stride[k] > kAosMaxStride)))
            return SRPC_E_UNSUPPORTED;
    return SRPC_OK;
}

// The plans of a size query into d's layout part (h_stride may be nullptr: no record plan).
inline int legs_query_plans(const srpc_plan* const* plans, int nplans, const uint64_t* h_stride, bool decode,
                            MvDesc* d) {
    for (int k = 0; h_stride && k < nplans; ++k)
        if (past_u32(h_stride[k])) return SRPC_E_INVALID;
    if (int rc = mv_plans(plans, nplans, 4, d)) return rc;
    return legs_plans_ok(plans, nplans, h_stride, decode);
}

// The record plans' leaves as columns of d: each leaf's address inside element 0.
inline void legs_cols(const srpc_plan* const* plans, int nplans, void* const* d_recs, const uint64_t* h_stride,
                      const uint32_t* const* h_leaf_offs, MvDesc* d) {
    for (int k = 0; k < nplans; ++k) {
        if (!h_stride[k]) continue;
        for (uint32_t f = 0; f < plans[k]->nfields; ++f) {
            const uint32_t nf = d->field0[k] + f;
            // an array may be null where h_cap leaves it no element: no call reads it
            d->col[nf] = d_recs[k] ? static_cast<uint8_t*>(d_recs[k]) + h_leaf_offs[k][f] : nullptr;
            d->soffs[nf] = nullptr;
            d->scap[nf] = 0;
        }
    }
}

inline uint32_t legs_fmax(const MvDesc& d) {
    uint32_t m = 0;
    for (uint32_t k = 0; k < d.nplans; ++k) m = std::max(m, d.F[k]);
    return m;
}

inline uint64_t legs_tables_at(const MvScratch& sc) { return (sc.bytes + 15) & ~15ull; }

// A decode's image window and tile once desc_bytes of tables and fills share the image's budget.
inline void legs_window(uint32_t desc_bytes, MvDesc* d, MvLegs* x) {
    x->x.desc_bytes = desc_bytes;
    x->window = kMixImage - desc_bytes;
    d->T = mix_tile(legs_fmax(*d), x->window);
}

// The record plans of a decode, described (mv_plans and legs_plans_ok have
// passed): their tables and fills as they will lie in scratch and in LDS, the
// kernel's argument, and in *d the tile that the window they leave allows.
struct LegsTables {
    AosDesc desc;
    MvLegs x{};  // x.x.desc_bytes == 0: no record plan, the batch is the column-only parse kernel's
};

inline int legs_describe(const srpc_plan* const* plans, int nplans, void* const* d_recs, const uint64_t* h_stride,
                         const uint32_t* const* h_leaf_offs, const void* const* h_fill, MvDesc* d, LegsTables* t) {
    if (aos_desc_bytes(h_stride, nplans))
        if (int rc = aos_describe(plans, nplans, d_recs, h_stride, h_leaf_offs, h_fill, &t->desc, &t->x.x)) return rc;
    legs_window(t->x.x.desc_bytes, d, &t->x);
    return SRPC_OK;
}

}  // namespace srpc_impl
