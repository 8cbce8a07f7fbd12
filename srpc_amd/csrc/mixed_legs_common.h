// mixed_legs_common.h -- internal: the host side that the calls over plans of
// both kinds share (mixed_legs.hip: the client's request pack and reply decode;
// mixed_req_legs.hip: the server's request decode): which plans are record
// plans (h_stride[k] != 0), the checks of their arguments, their leaves as
// columns of MvDesc, and where their tables and fills lie in scratch.
#pragma once

#include <algorithm>
#include <cstdint>

#include "aos_pieces.h"
#include "mixed_aos_common.h"
#include "mixed_common.h"
#include "mixed_var_common.h"
#include "plan.h"
#include "srpc_gpu.h"

namespace srpc_impl {

// The record plans of a call, compacted: what aos_describe and aos_desc_bytes take.
struct LegRecs {
    int n = 0;
    int plan[kMixPlans];  // record plan r is plan plan[r]
    const srpc_plan* plans[kMixPlans];
    void* recs[kMixPlans];
    uint64_t stride[kMixPlans];
    const uint32_t* leaf_offs[kMixPlans];
    const void* fill[kMixPlans];
};

inline void leg_recs(const srpc_plan* const* plans, int nplans, void* const* d_recs, const uint64_t* h_stride,
                     const uint32_t* const* h_leaf_offs, const void* const* h_fill, LegRecs* out) {
    for (int k = 0; k < nplans; ++k) {
        if (!h_stride[k]) continue;
        const int r = out->n++;
        out->plan[r] = k;
        out->plans[r] = plans[k];
        out->recs[r] = d_recs[k];
        out->stride[r] = h_stride[k];
        out->leaf_offs[r] = h_leaf_offs[k];
        out->fill[r] = h_fill ? h_fill[k] : nullptr;
    }
}

// What is checked of the struct-array arguments before any plan is read.
inline bool legs_args_invalid(const void* const* d_recs, const uint64_t* h_stride, const uint32_t* const* h_leaf_offs,
                              const void* const* h_fill, bool decode, const uint64_t* h_first, const uint64_t* h_cap,
                              int nplans) {
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

}  // namespace srpc_impl
