// mixed_common.h -- internal: what the kernels of mixed.hip (fixed-size plans)
// and mixed_var.hip (fixed-size and string plans) share: the call index's
// geometry and mix_ranks, the rank of every call of a granule from that index.
#pragma once

#include <algorithm>
#include <cstdint>

#include "plan.h"
#include "srpc_gpu.h"

namespace srpc_impl {

constexpr int kMixPlans = SRPC_FRAMES_MAX_PLANS;
constexpr uint32_t kMixGranule = kBlock;   // calls per table row: one per lane
constexpr uint32_t kMixWaves = kBlock / 64;
constexpr uint32_t kMixSuper = 16;         // granules per super-row of the table
constexpr uint32_t kMixRow = kMixPlans + 2;  // words of one LDS count row
constexpr uint32_t kMixLds = (kMixWaves + 1) * kMixRow;  // per-wave counts, then the granule's bases
constexpr uint32_t kMixImage = 32768;      // image bytes per tile
constexpr int kMixFields = SRPC_FRAMES_MIXED_MAX_FIELDS;
constexpr uint32_t kNoRank = 0xffffffffu;

struct MixLane {
    uint32_t cls;   // plan, nplans for an id out of range, nplans + 1 for no call
    uint32_t rank;  // calls of the same plan before this one in the chunk
};

// The ranks of granule `g`'s calls, one per lane.  table: the index (rows
// granule rows, each the calls before it inside its super-row, then the
// super-rows' prefixes), or nullptr for ranks inside the granule.  wcnt: LDS,
// kMixLds words; its last row is left holding the granule's bases (the calls of
// each plan before the granule), the rows before it each wave's counts.  The
// method byte and the bases are loaded together, so the ranks cost one global
// latency.  Ends with a barrier.
__device__ __forceinline__ MixLane mix_ranks(const uint8_t* __restrict__ method, uint64_t ncalls, uint32_t K,
                                             const uint32_t* __restrict__ table, uint64_t rows, uint64_t g,
                                             uint32_t* wcnt) {
    const uint64_t i = g * kMixGranule + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t* base = wcnt + kMixWaves * kMixRow;
    if (threadIdx.x <= K)
        base[threadIdx.x] = table ? table[g * (K + 1) + threadIdx.x] + table[(rows + g / kMixSuper) * (K + 1) + threadIdx.x] : 0;
    MixLane r;
    r.cls = i < ncalls ? min(static_cast<uint32_t>(method[i]), K) : K + 1;
    uint32_t inw = 0;
    for (uint32_t k = 0; k <= K; ++k) {
        const uint64_t b = __ballot(r.cls == k);
        if (r.cls == k) inw = __popcll(b & ((1ull << lane) - 1));
        if (lane == 0) wcnt[w * kMixRow + k] = __popcll(b);
    }
    __syncthreads();
    r.rank = kNoRank;
    if (r.cls <= K) {
        uint32_t v = base[r.cls] + inw;
        for (uint32_t q = 0; q < w; ++q) v += wcnt[q * kMixRow + r.cls];
        r.rank = v;
    }
    return r;
}

__device__ __forceinline__ uint64_t load_elem(const uint8_t* p, uint32_t s) {
    switch (s) {
    case 1: return *p;
    case 2: return *reinterpret_cast<const uint16_t*>(p);
    case 4: return *reinterpret_cast<const uint32_t*>(p);
    default: return *reinterpret_cast<const uint64_t*>(p);
    }
}

__device__ __forceinline__ void store_elem(uint8_t* p, uint32_t s, uint64_t v) {
    switch (s) {
    case 1: *p = static_cast<uint8_t>(v); break;
    case 2: *reinterpret_cast<uint16_t*>(p) = static_cast<uint16_t>(v); break;
    case 4: *reinterpret_cast<uint32_t*>(p) = static_cast<uint32_t>(v); break;
    default: *reinterpret_cast<uint64_t*>(p) = v; break;
    }
}

__device__ __forceinline__ uint32_t mix_be32(const uint8_t* b) {
    return (static_cast<uint32_t>(b[0]) << 24) | (static_cast<uint32_t>(b[1]) << 16) | (static_cast<uint32_t>(b[2]) << 8) |
           static_cast<uint32_t>(b[3]);
}

inline uint64_t mix_rows(uint64_t ncalls) { return (ncalls + kMixGranule - 1) / kMixGranule; }
inline uint64_t mix_super_rows(uint64_t rows) { return (rows + kMixSuper - 1) / kMixSuper; }
inline uint64_t mix_index_bytes(uint64_t ncalls, int nplans) {
    const uint64_t rows = mix_rows(ncalls);
    return std::max<uint64_t>(8, ((rows + mix_super_rows(rows)) * (nplans + 1) * 4 + 7) & ~7ull);
}

}  // namespace srpc_impl
