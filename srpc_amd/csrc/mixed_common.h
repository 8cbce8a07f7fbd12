// mixed_common.h -- internal: what the kernels of mixed.hip (fixed-size plans,
// client side), mixed_req.hip (fixed-size plans, server side), mixed_var.hip and
// mixed_req_var.hip (fixed-size and string plans, client and server side)
// share: the call index's geometry and mix_ranks, the rank of every call of a
// granule from that index; for the two server-side files a tile's offsets and
// staging; for the two fixed-size files also the kernels' arguments, their LDS
// lookups and prefix templates; for mixed.hip and mixed_aos.hip (the client
// side over columns and over struct arrays) the request pack of a tile
// (mix_pack_tile) and the reply decode's judgement of a frame (mix_judge).
// What the two decodes into struct arrays share is mixed_aos_common.h.
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

// ---- the server-side decodes (mixed_req.hip, mixed_req_var.hip): a tile's frame
// offsets and its span of the stream in LDS ----

// lo[j] = the offset of frame c0 + j, buf_len past the last frame (the last
// frame ends at buf_len).  Complete after the next barrier.
__device__ __forceinline__ void req_offsets(uint32_t* lo, uint32_t T, const uint32_t* __restrict__ offs, uint64_t nframes,
                                            uint64_t c0, uint64_t buf_len) {
    for (uint32_t j = threadIdx.x; j <= T; j += kBlock)
        lo[j] = c0 + j < nframes ? offs[c0 + j] : static_cast<uint32_t>(buf_len);
}

struct ReqSpan {
    uint64_t s0;      // the image's first byte of the stream (16-byte aligned)
    uint32_t staged;  // bytes of the stream in the image
};

// The span of the tile's nr frames -> image, from a 16-byte boundary; bytes of
// [0, buf_len) only, at most cap of them.  lo[] is complete; ends with a barrier.
__device__ __forceinline__ ReqSpan req_stage(uint8_t* img, const uint32_t* lo, uint32_t nr, uint32_t cap,
                                             const uint8_t* __restrict__ buf, uint64_t buf_len) {
    ReqSpan sp{0, 0};
    if (nr) {
        const uint64_t o0 = lo[0], oe = lo[nr];
        sp.s0 = o0 & ~15ull;
        if (o0 <= buf_len) {
            const uint64_t end = oe >= o0 && oe <= buf_len ? oe : buf_len;
            sp.staged = static_cast<uint32_t>(min<uint64_t>(end - sp.s0, cap));
        }
    }
    const uint8_t* src = buf + sp.s0;
    const uint32_t full = sp.staged >> 4;
    constexpr int kLoads = 4;  // 16-byte loads in flight per lane
    for (uint32_t cb = threadIdx.x; cb < full; cb += kBlock * kLoads) {
        uint4 vv[kLoads];
#pragma unroll
        for (int u = 0; u < kLoads; ++u) vv[u] = *reinterpret_cast<const uint4*>(src + 16 * min(cb + u * kBlock, full - 1));
#pragma unroll
        for (int u = 0; u < kLoads; ++u)
            if (cb + u * kBlock < full) *reinterpret_cast<uint4*>(img + 16 * (cb + u * kBlock)) = vv[u];
    }
    for (uint32_t b = full * 16 + threadIdx.x; b < sp.staged; b += kBlock) img[b] = src[b];
    __syncthreads();
    return sp;
}

// ---- fixed-size plans: what mixed.hip (client side) and mixed_req.hip (server
// side) share ----

struct MixArgs {
    uint8_t* col[kMixFields];        // plan k's columns: [field0[k], field0[k + 1])
    uint16_t off[kMixFields];        // field offset inside the frame
    uint8_t size[kMixFields];
    const uint8_t* prefix[kMixPlans];  // device prefix (8-byte aligned, zero-padded 16 bytes past its end)
    uint64_t first[kMixPlans];       // element of the chunk's first call of plan k
    uint32_t room[kMixPlans];        // elements the columns have from `first` on
    uint32_t F[kMixPlans];           // frame bytes
    uint16_t prefix_len[kMixPlans];
    uint16_t tmpl[kMixPlans];        // LDS offset of plan k's prefix template (8-byte aligned)
    uint16_t field0[kMixPlans + 1];
    uint32_t nplans;
    uint32_t T;                      // calls per workgroup tile (divides kMixGranule)
    uint32_t img;                    // LDS bytes of the image (multiple of 16)
};

// The lookups a lane makes by its own plan, in LDS: indexed from the kernel
// arguments they would be vector loads, several of them dependent, per lane.
struct MixLds {
    uint8_t* col[kMixFields];
    uint64_t first[kMixPlans];
    uint32_t room[kMixPlans];
    uint32_t F[kMixPlans];
    uint16_t off[kMixFields];
    uint16_t prefix_len[kMixPlans];
    uint16_t tmpl[kMixPlans];
    uint16_t field0[kMixPlans + 1];
    uint8_t size[kMixFields];
};

// Filled by the whole workgroup; complete after the next barrier.
__device__ __forceinline__ void mix_lds_fill(MixLds& d, const MixArgs& a) {
    const uint32_t K = a.nplans, nf = a.field0[K];
    for (uint32_t f = threadIdx.x; f < nf; f += kBlock) {
        d.col[f] = a.col[f];
        d.off[f] = a.off[f];
        d.size[f] = a.size[f];
    }
    if (threadIdx.x <= K) d.field0[threadIdx.x] = a.field0[threadIdx.x];
    if (threadIdx.x < K) {
        const uint32_t k = threadIdx.x;
        d.first[k] = a.first[k];
        d.room[k] = a.room[k];
        d.F[k] = a.F[k];
        d.prefix_len[k] = a.prefix_len[k];
        d.tmpl[k] = a.tmpl[k];
    }
}

// The K prefixes into LDS at dst + a.tmpl[k]: a lane per byte of the template
// region, its plan picked with uniform (scalar) argument reads, so the
// prefixes cost one global latency whatever K is.
__device__ __forceinline__ void mix_templates(uint8_t* dst, const MixArgs& a) {
    const uint32_t K = a.nplans;
    const uint32_t tb = a.tmpl[K - 1] + a.prefix_len[K - 1];
    for (uint32_t t = threadIdx.x; t < tb; t += kBlock) {
        uint32_t off = 0, pl = a.prefix_len[0];
        const uint8_t* ptr = a.prefix[0];
        for (uint32_t k = 1; k < K; ++k) {
            const bool in = a.tmpl[k] <= t;
            off = in ? a.tmpl[k] : off;
            pl = in ? a.prefix_len[k] : pl;
            ptr = in ? a.prefix[k] : ptr;
        }
        if (t - off < pl) dst[t] = ptr[t - off];
    }
}

inline uint32_t mix_tile(uint32_t fmax, uint32_t image = kMixImage) {
    uint32_t t = kMixGranule;
    while (t > 16 && t * fmax > image) t >>= 1;
    return t;
}

// The plans of one side: fixed-size, a prefix of at least min_prefix bytes.
inline int mix_plans_ok(const srpc_plan* const* plans, int nplans, uint32_t min_prefix, uint32_t* fmax) {
    uint32_t fields = 0, m = 0;
    for (int k = 0; k < nplans; ++k) {
        const srpc_plan* p = plans[k];
        if (!p) return SRPC_E_INVALID;
        if (p->has_string || p->prefix_len < min_prefix) return SRPC_E_UNSUPPORTED;
        fields += p->nfields;
        m = std::max<uint32_t>(m, static_cast<uint32_t>(p->stride));
    }
    if (fields > static_cast<uint32_t>(kMixFields)) return SRPC_E_UNSUPPORTED;
    *fmax = m;
    return SRPC_OK;
}

// Columns, rooms and layouts into the kernel's arguments.  col_align: what a
// column pointer must keep (mixed_aos.hip passes each leaf's address inside
// element 0 of its plan's struct array as the "column", checked there).
inline int mix_args(const srpc_plan* const* plans, int nplans, const void* const* const* d_cols,
                    const uint64_t* h_first, const uint64_t* h_cap, uint32_t fmax, MixArgs* a, uint32_t* tmpl_bytes,
                    uintptr_t col_align = 16) {
    uint32_t nf = 0, tb = 0;
    for (int k = 0; k < nplans; ++k) {
        const srpc_plan* p = plans[k];
        const uint64_t first = h_first ? h_first[k] : 0;
        const uint64_t room = h_cap[k] > first ? h_cap[k] - first : 0;
        if (!d_cols[k]) return SRPC_E_INVALID;
        a->field0[k] = static_cast<uint16_t>(nf);
        for (uint32_t f = 0; f < p->nfields; ++f, ++nf) {
            const void* c = d_cols[k][f];
            if (room && !c) return SRPC_E_INVALID;
            if (!aligned(c, col_align)) return SRPC_E_ALIGN;
            a->col[nf] = static_cast<uint8_t*>(const_cast<void*>(c));
            a->off[nf] = static_cast<uint16_t>(p->off[f]);
            a->size[nf] = static_cast<uint8_t>(p->size[f]);
        }
        a->prefix[k] = p->d_prefix;
        a->first[k] = first;
        a->room[k] = static_cast<uint32_t>(std::min<uint64_t>(room, 0xffffffffull));
        a->F[k] = static_cast<uint32_t>(p->stride);
        a->prefix_len[k] = static_cast<uint16_t>(p->prefix_len);
        a->tmpl[k] = static_cast<uint16_t>(tb);
        tb += (p->prefix_len + 7) & ~7u;  // 8-byte aligned: the decode compares eight bytes at a time
    }
    a->field0[nplans] = static_cast<uint16_t>(nf);
    a->nplans = static_cast<uint32_t>(nplans);
    a->T = mix_tile(fmax);
    a->img = (a->T * fmax + 16 + 15) & ~15u;
    *tmpl_bytes = tb;
    return SRPC_OK;
}

// ---- the client-side kernels of mixed.hip (columns) and mixed_aos.hip (struct
// arrays): everything but where a call's fields live ----

// The request pack of one tile.  AOS = false: leaf f of element e is at
// col[f] + e * size[f] (a column).  AOS = true: at col[f] + e * stride[k],
// col[f] being the leaf's address inside element 0 of plan k's struct array
// and `stride` (kernel argument, K entries) the plans' struct bytes; lanes of
// one plan hold consecutive ranks, so their structs are adjacent in memory.
// Dynamic LDS: image[a.img] | templates[tmpl_bytes] | 16 pad.
template <bool AOS>
__device__ __forceinline__ void mix_pack_tile(const MixArgs& a, const uint32_t* stride,
                                              const uint8_t* __restrict__ method,
                                              const uint32_t* __restrict__ table, uint64_t rows, uint64_t ncalls,
                                              uint8_t* __restrict__ out, uint32_t* __restrict__ offs,
                                              srpc_unpack_status* st) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    __shared__ uint32_t wcnt[kMixLds];
    __shared__ uint32_t wsum[kMixWaves];
    __shared__ uint32_t range[2];
    __shared__ uint32_t step[AOS ? kMixPlans : 1];
    __shared__ MixLds d;
    if (ncalls == 0) {
        if (offs && threadIdx.x == 0) offs[0] = 0;
        return;
    }
    const uint32_t K = a.nplans;
    const uint64_t c0 = static_cast<uint64_t>(blockIdx.x) * a.T;
    const uint64_t g = c0 / kMixGranule;
    const uint32_t j0 = static_cast<uint32_t>(c0 - g * kMixGranule);  // the tile's first lane
    const uint64_t i = g * kMixGranule + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t* base = wcnt + kMixWaves * kMixRow;  // after mix_ranks: the calls of each plan before the granule

    mix_lds_fill(d, a);
    if constexpr (AOS)
        if (threadIdx.x < K) step[threadIdx.x] = stride[threadIdx.x];
    mix_templates(lds + a.img, a);  // the K prefixes as LDS templates

    const MixLane r = mix_ranks(method, ncalls, K, table, rows, g, wcnt);
    const bool present = r.cls <= K;
    const bool good = r.cls < K && r.rank < d.room[r.cls];
    const uint32_t F = good ? d.F[r.cls] : 0;

    // bytes of the frames before this granule, and an exclusive scan inside it
    uint64_t gbase = 0;
    for (uint32_t k = 0; k < K; ++k) gbase += static_cast<uint64_t>(min(base[k], a.room[k])) * a.F[k];
    uint32_t inc = F;
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint32_t at = inc - F;
    for (uint32_t q = 0; q < w; ++q) at += wsum[q];

    const bool mine = threadIdx.x >= j0 && threadIdx.x < j0 + a.T;
    if (threadIdx.x == j0) range[0] = at;
    if (threadIdx.x == j0 + a.T - 1) range[1] = at + F;
    __syncthreads();
    const uint64_t lo = gbase + range[0], hi = gbase + range[1];  // the tile's bytes of the stream
    const uint64_t A = lo & ~15ull;                                // the image's first byte

    if (mine && present) {
        const uint64_t o = gbase + at;
        if (offs) {
            offs[i] = static_cast<uint32_t>(o);
            if (i + 1 == ncalls) offs[ncalls] = static_cast<uint32_t>(o + F);
        }
        if (!good) {
            if (st) report_bad(st, SRPC_STATUS_BOUNDS, i);
        } else {
            const uint32_t k = r.cls;
            const uint32_t p = static_cast<uint32_t>(o - A);  // < T * F_max + 16 <= a.img
            const uint64_t e = d.first[k] + r.rank;
            const uint32_t f0 = d.field0[k], f1 = d.field0[k + 1];
            const uint64_t es = AOS ? e * step[k] : 0;  // the struct's byte offset
            // the first fields' loads are issued together, before the prefix is copied
            constexpr uint32_t kAhead = 2;
            uint64_t v[kAhead];
#pragma unroll
            for (uint32_t u = 0; u < kAhead; ++u) {
                const uint32_t f = min(f0 + u, f1 - 1);
                v[u] = load_elem(d.col[f] + (AOS ? es : e * d.size[f]), d.size[f]);
            }
            lds_copy_run(lds, p, a.img + d.tmpl[k], d.prefix_len[k]);
#pragma unroll
            for (uint32_t u = 0; u < kAhead; ++u)
                if (f0 + u < f1) lds_put_small(lds, p + d.off[f0 + u], v[u], d.size[f0 + u]);
            for (uint32_t f = f0 + kAhead; f < f1; ++f) {
                const uint32_t s = d.size[f];
                lds_put_small(lds, p + d.off[f], load_elem(d.col[f] + (AOS ? es : e * s), s), s);
            }
        }
    }
    __syncthreads();

    // image -> stream: whole 16-byte chunks inside [lo, hi) as one store, the rest bytewise
    const uint32_t nch = static_cast<uint32_t>((hi - A + 15) >> 4);
    for (uint32_t c = threadIdx.x; c < nch; c += kBlock) {
        const uint64_t b0 = A + 16ull * c;
        if (b0 >= lo && b0 + 16 <= hi) {
            *reinterpret_cast<uint4*>(out + b0) = *reinterpret_cast<const uint4*>(lds + 16 * c);
        } else {
            for (uint32_t b = 0; b < 16; ++b)
                if (b0 + b >= lo && b0 + b < hi) out[b0 + b] = lds[16 * c + b];
        }
    }
}

// What the reply decode finds for one call of its tile.
struct MixReply {
    uint64_t o;     // the frame's stream offset
    uint32_t code;  // d_codes[i]
    uint32_t flag;  // status flag, 0 for none
    uint32_t q;     // the frame's image position (in_img)
    bool decoded;   // a full frame of the call's own plan: its fields are the frame's
    bool in_img;    // ... and it lies inside the staged span; else it is read from buf + o
};

// Call j of a tile with nr frames, judged by the table of
// srpc_frames_unpack_replies against its own plan's prefix.  good: the call has
// a plan and an element.  lo[]: the tile's offsets (req_offsets), sp: its
// staged span (req_stage), tmpl: the K prefixes (mix_templates).
__device__ __forceinline__ MixReply mix_judge(const MixLds& d, const MixLane& r, bool good, uint32_t j, uint32_t nr,
                                              const uint32_t* lo, const uint8_t* img, const uint8_t* tmpl,
                                              const ReqSpan& sp, const uint8_t* __restrict__ buf, uint64_t buf_len,
                                              uint32_t unanswered) {
    MixReply y{0, SRPC_REPLY_NO_CODE, 0, 0, false, false};
    if (j >= nr) {
        y.code = unanswered;  // no frame: no flag
    } else if (!good) {
        y.flag = SRPC_STATUS_BOUNDS;  // no plan, or no element to decode into
    } else {
        const uint32_t k = r.cls;
        const uint64_t e = lo[j + 1];
        y.o = lo[j];
        if (!(y.o <= e && e <= buf_len) || e - y.o < 5) {
            y.flag = SRPC_STATUS_BOUNDS;
        } else {
            const uint64_t len = e - y.o;
            const uint64_t need = len == d.F[k] ? len : 5;
            y.in_img = y.o >= sp.s0 && y.o - sp.s0 + need <= sp.staged;
            y.q = static_cast<uint32_t>(y.o - sp.s0);
            const uint8_t* h = y.in_img ? img + y.q : buf + y.o;
            const uint32_t be = mix_be32(h), cb = h[4];
            if (be != len - 4) {
                y.flag = SRPC_STATUS_BOUNDS;
            } else {
                y.code = cb;
                if (len == d.F[k]) {
                    const uint32_t pl = d.prefix_len[k];
                    const uint8_t* pre = tmpl + d.tmpl[k];
                    bool eq = true;
                    if (y.in_img) {
                        for (uint32_t b = 0; b < pl; b += 8) {
                            uint64_t m = pl - b >= 8 ? ~0ull : (1ull << (8 * (pl - b))) - 1;
                            if (b == 0) m &= ~(0xffull << 32);  // the code byte
                            eq &= ((lds_u64(img, y.q + b) ^ *reinterpret_cast<const uint64_t*>(pre + b)) & m) == 0;
                        }
                    } else {
                        for (uint32_t b = 0; b < pl; ++b) eq &= b == 4 || buf[y.o + b] == pre[b];
                    }
                    if (eq) y.decoded = true;
                    else y.flag = SRPC_STATUS_PREFIX;
                } else if (!(len == 5 && cb != 0)) {
                    y.flag = SRPC_STATUS_PREFIX;
                }
            }
        }
    }
    return y;
}

// What every mixed call checks of its arguments before a plan is read (SRPC_E_INVALID).
template <class... P>
inline bool any_null(const P*... p) { return (... || !p); }
inline bool past_u32(uint64_t v) { return v >= (1ull << 32); }
inline bool mix_nplans_bad(int nplans) { return nplans <= 0 || nplans > kMixPlans; }

// mixed.hip: the index over ncalls method bytes (k_mixed_hist, k_mixed_scan;
// ids >= nplans land in column nplans), d_status reset and flagged when given.
int mix_index_launch(const uint8_t* d_method, uint64_t ncalls, int nplans, uint32_t* table, uint64_t* d_counts,
                     srpc_unpack_status* d_status, hipStream_t s);

// mixed_req.hip: the classify pass of the server-side decodes over fixed-size
// plans (a.T = mix_tile: the column call's tile), nframes > 0.
void req_classify_launch(const MixArgs& a, uint32_t tmpl_bytes, const uint8_t* d_buf, uint64_t buf_len,
                         const uint32_t* d_offs, uint64_t nframes, uint8_t* d_class, hipStream_t s);

}  // namespace srpc_impl
