// aos_pieces.h -- internal: what the frame decodes into struct arrays share
// (frames_aos.hip: one plan; mixed_aos.hip: a plan per call; mixed_req_aos.hip:
// a plan per request frame, through mixed_aos_common.h): the per-struct-byte
// source table a 16-byte piece of the array is assembled through, its host-side
// builder and the layout checks of a struct with leaves at given offsets.
#pragma once

#include <algorithm>
#include <cstdint>

#include "plan.h"
#include "srpc_gpu.h"

namespace srpc_impl {

constexpr uint32_t kAosMaxStride = 256;       // struct bytes a decode takes
constexpr uint32_t kSrcFill = 0xfff;          // table entry: the byte comes from the fill record
constexpr uint32_t kPosZero = 0xffffffffu;    // pos[j]: the frame's leaves are zero
constexpr uint32_t kPosGlobal = 0xfffffffeu;  // pos[j]: a full frame outside the image

typedef uint32_t aos_u32x4 __attribute__((ext_vector_type(4)));

inline uint32_t s16_of(uint32_t stride) { return (stride + 15) & ~15u; }

// The k <= 8 low bytes of v into bytes [b, b + k) of the 16-byte piece lo | hi.
__device__ __forceinline__ void piece_put(uint64_t& lo, uint64_t& hi, uint32_t b, uint64_t v, uint32_t k) {
    if (k < 8) v &= (1ull << (8 * k)) - 1;
    if (b < 8) {
        lo |= v << (8 * b);
        if (b && b + k > 8) hi |= v >> (64 - 8 * b);
    } else {
        hi |= v << (8 * (b - 8));
    }
}

// from[k] of a struct of `stride` <= kAosMaxStride bytes: -1 for a byte no leaf
// covers, else the wire offset of the leaf byte there.  SRPC_E_INVALID: a leaf
// past the stride, or two leaves sharing a byte.
inline int aos_sources(const srpc_plan* p, const uint32_t* field_offsets, uint32_t stride, int32_t* from) {
    std::fill(from, from + stride, -1);
    for (uint32_t f = 0; f < p->nfields; ++f) {
        if (field_offsets[f] + static_cast<uint64_t>(p->size[f]) > stride) return SRPC_E_INVALID;
        for (uint32_t b = 0; b < p->size[f]; ++b) {
            if (from[field_offsets[f] + b] >= 0) return SRPC_E_INVALID;  // two leaves share a byte
            from[field_offsets[f] + b] = static_cast<int32_t>(p->off[f] + b);
        }
    }
    return SRPC_OK;
}

// Natural alignment, as in C++ structs: every offset and the stride against the leaf's size.
inline bool aos_layout_aligned(const srpc_plan* p, const uint32_t* field_offsets, uint64_t stride) {
    for (uint32_t f = 0; f < p->nfields; ++f)
        if (field_offsets[f] % p->size[f] || stride % p->size[f]) return false;
    return true;
}

// tab[k] = (run bytes from k on, 1..8) << 12 | wire offset or kSrcFill: a run is
// consecutive wire bytes, or fill, and ends with the struct.
inline void aos_run_table(const int32_t* from, uint32_t stride, uint16_t* tab) {
    for (uint32_t k = stride; k-- > 0;) {  // run lengths, from the struct's end
        uint32_t run = 1;
        if (k + 1 < stride && (from[k] < 0 ? from[k + 1] < 0 : from[k + 1] == from[k] + 1))
            run = std::min<uint32_t>(8, 1 + (tab[k + 1] >> 12));
        tab[k] = static_cast<uint16_t>((run << 12) | (from[k] < 0 ? kSrcFill : static_cast<uint32_t>(from[k])));
    }
}

}  // namespace srpc_impl
