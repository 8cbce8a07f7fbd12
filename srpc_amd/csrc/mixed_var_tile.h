// mixed_var_tile.h -- internal: the two tile kernels of the client-side calls
// over fixed-size and string plans as device functions, for the two files that
// launch them: mixed_var.hip (every plan in columns: LEGS = false, the kernels
// k_mv_pack and k_mv_parse as they always were) and mixed_legs.hip (LEGS = true:
// a plan's fields may also live in one device array of the caller's structs).
// With them what they are made of: the workgroup scan, a call's frame length
// and the copy of a round's runs.
//
// LEGS = true adds, and compiles into the LEGS = false kernels nothing of:
//   pack    a leaf of a record plan is a column whose element step is the
//       struct's stride (its base the leaf's address inside element 0), so the
//       per-lane field loop reads either form;
//   decode  a lane whose call belongs to a record plan stores nothing itself
//       but leaves pos[j]; the workgroup then writes the record plans' slices
//       of the tile as whole 16-byte pieces (mixed_aos_common.h).  The record
//       plans' tables and fills lie in the tail of the image's 32 KiB, the
//       image window being that much shorter.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "aos_pieces.h"
#include "mixed_aos_common.h"
#include "mixed_common.h"
#include "mixed_var_common.h"
#include "plan.h"
#include "srpc_gpu.h"

namespace srpc_impl {

constexpr uint64_t kMvSat = 1ull << 32;        // a frame length saturates here: past any out_cap
constexpr uint64_t kMvInImage = 1ull << 63;    // run destination: an image offset

// What the LEGS kernels know beyond MvDesc (a kernel argument).  x.stride[k] is
// 0 for a column plan; x.tab, x.fill and x.desc_bytes are the decode's.
struct MvLegs {
    MixAos x;
    uint32_t window;  // decode: bytes of the image window, kMixImage - x.desc_bytes
};

// Exclusive scan of one u64 per lane over the workgroup; *total = the sum.
// wsum: LDS, kMixWaves entries.  Ends with a barrier (wsum can be reused).
__device__ __forceinline__ uint64_t mv_block_scan(uint64_t x, uint64_t* wsum, uint64_t* total) {
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t inc = x;
    for (uint32_t s = 1; s < 64; s <<= 1) {
        const uint64_t t = __shfl_up(inc, s, 64);
        if (lane >= s) inc += t;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint64_t at = inc - x, all = 0;
    for (uint32_t q = 0; q < kMixWaves; ++q) {
        if (q < w) at += wsum[q];
        all += wsum[q];
    }
    __syncthreads();
    *total = all;
    return at;
}

struct MvFrame {
    uint64_t len;  // frame bytes, 0 for a bad call
    uint64_t e;    // element of the plan's columns
    bool good;
};

// The request frame of a call: its element and its length from the leg's
// string offsets.  A decreasing pair makes the call bad; no char is read here.
__device__ __forceinline__ MvFrame mv_frame(const MvDesc* __restrict__ d, const MixLane& r) {
    MvFrame fr{0, 0, false};
    if (r.cls >= d->nplans || r.rank >= d->room[r.cls]) return fr;
    const uint32_t k = r.cls;
    fr.e = d->first[k] + r.rank;
    fr.good = true;
    uint64_t len = d->F[k];
    for (uint32_t t = 0; t < d->nstr[k]; ++t) {
        const uint32_t f = d->str_leaf[k * kMvStr + t];
        const uint64_t a = d->soffs[f][fr.e], b = d->soffs[f][fr.e + 1];
        if (b < a) fr.good = false;
        else len = b - a > kMvSat - len ? kMvSat : len + (b - a);
    }
    fr.len = fr.good ? len : 0;
    return fr;
}

// The k <= 8 low bytes of v to frame byte `pos`: into the image, or bytewise to
// global memory.
__device__ __forceinline__ void mv_put(bool inimg, uint8_t* lds, uint32_t q, uint8_t* __restrict__ out, uint64_t o,
                                       uint32_t pos, uint64_t v, uint32_t k) {
    if (inimg) {
        lds_put_small(lds, q + pos, v, k);
    } else {
        for (uint32_t b = 0; b < k; ++b) out[o + pos + b] = static_cast<uint8_t>(v >> (8 * b));
    }
}

// The round's runs (one per lane: rel[j] = exclusive scan of their lengths,
// rel[kBlock] = total) copied by the whole workgroup, 8 bytes of the run space
// per lane and step.  dst[j] is a global address, or kMvInImage | image offset.
__device__ __forceinline__ void mv_copy_runs(const uint64_t* rel, const uint8_t* const* src, const uint64_t* dst,
                                             uint8_t* lds) {
    const uint64_t total = rel[kBlock];
    const uint64_t np = (total + 7) >> 3;
    for (uint64_t p = threadIdx.x; p < np; p += kBlock) {
        uint64_t r = p << 3;
        const uint64_t rend = min(r + 8, total);
        uint32_t lo_j = 0, hi_j = kBlock;  // the last j with rel[j] <= r
        while (hi_j - lo_j > 1) {
            const uint32_t m = (lo_j + hi_j) >> 1;
            if (rel[m] <= r) lo_j = m;
            else hi_j = m;
        }
        uint32_t j = lo_j;
        for (; r < rend; ++r) {
            while (rel[j + 1] <= r) ++j;  // empty runs; r < total keeps j < kBlock
            const uint64_t x = r - rel[j];
            const uint8_t v = src[j][x];
            const uint64_t t = dst[j];
            if (t & kMvInImage) lds[static_cast<uint32_t>(t) + static_cast<uint32_t>(x)] = v;
            else reinterpret_cast<uint8_t*>(t)[x] = v;
        }
    }
}

// The request pack of one tile of T calls.  LEGS: leaf f of element e of a plan
// with x->x.stride[k] != 0 is at col[f] + e * stride[k], col[f] being the leaf's
// address inside element 0 of the plan's struct array; every other leaf is at
// col[f] + e * size[f].  x is not read when !LEGS.
// Dynamic LDS: image[kMixImage + 16] | templates[tmpl_bytes] | 16 pad.
template <bool LEGS>
__device__ __forceinline__ void mv_pack_tile(const MvDesc* __restrict__ d, const MvLegs* x,
                                             const uint8_t* __restrict__ method, const uint32_t* __restrict__ table,
                                             uint64_t rows, uint64_t ncalls, const uint64_t* __restrict__ gsum,
                                             uint8_t* __restrict__ out, uint64_t out_cap, uint32_t* __restrict__ offs,
                                             srpc_unpack_status* st) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    __shared__ uint32_t wcnt[kMixLds];
    __shared__ uint64_t wsum[kMixWaves];
    __shared__ uint64_t tile_lo;
    __shared__ unsigned long long himg;
    __shared__ uint64_t rel[kBlock + 1];
    __shared__ const uint8_t* rsrc[kBlock];
    __shared__ uint64_t rdst[kBlock];
    __shared__ uint32_t step[LEGS ? kMixPlans : 1];  // a record plan's struct bytes, else 0
    const uint32_t K = d->nplans, T = d->T;
    const uint64_t c0 = static_cast<uint64_t>(blockIdx.x) * T;
    const uint64_t g = c0 / kMixGranule;
    const uint32_t j0 = static_cast<uint32_t>(c0 - g * kMixGranule);
    const uint64_t i = g * kMixGranule + threadIdx.x;
    const uint32_t tm = kMixImage + 16;  // the templates' LDS offset

    mv_templates(lds + tm, d);
    if constexpr (LEGS)
        if (threadIdx.x < K) step[threadIdx.x] = x->x.stride[threadIdx.x];
    const MixLane r = mix_ranks(method, ncalls, K, table, rows, g, wcnt);
    const bool present = r.cls <= K;
    const MvFrame fr = mv_frame(d, r);
    uint64_t gtotal;
    const uint64_t o = gsum[g] + mv_block_scan(fr.len, wsum, &gtotal);

    const bool mine = threadIdx.x >= j0 && threadIdx.x < j0 + T;
    if (threadIdx.x == j0) tile_lo = o;
    __syncthreads();
    const uint64_t lo = tile_lo;  // the tile's first byte of the stream
    const uint64_t A = lo & ~15ull;  // the image's first byte
    const bool whole = mine && fr.good && o + fr.len <= out_cap;
    const bool inimg = whole && o + fr.len - A <= kMixImage;
    if (threadIdx.x == j0) himg = lo;
    __syncthreads();
    if (inimg) atomicMax(&himg, static_cast<unsigned long long>(o + fr.len));

    if (mine && present) {
        offs[i] = static_cast<uint32_t>(min(o, out_cap));
        if (!whole && st) report_bad(st, SRPC_STATUS_BOUNDS, i);
    }

    // the lane's part of its frame: BE32, prefix, fixed fields, string lengths
    const uint32_t k = whole ? r.cls : 0;
    const uint32_t q = static_cast<uint32_t>(o - A);  // used when inimg
    uint32_t f = 0, f1 = 0;
    uint64_t pos = 0;  // bytes of the frame so far
    if (whole) {
        const uint32_t pl = d->prefix_len[k];
        if (d->var[k]) {
            const uint32_t be = static_cast<uint32_t>(fr.len - 4);
            mv_put(inimg, lds, q, out, o, 0, __builtin_bswap32(be), 4);
            pos = 4;
        }
        if (inimg) {
            lds_copy_run(lds, q + static_cast<uint32_t>(pos), tm + d->tmpl[k], pl);
        } else {
            for (uint32_t b = 0; b < pl; ++b) out[o + pos + b] = lds[tm + d->tmpl[k] + b];
        }
        pos += pl;
        f = d->field0[k];
        f1 = d->field0[k + 1];
    }
    const uint32_t rounds = d->maxstr;
    for (uint32_t t = 0; t <= rounds; ++t) {
        // up to the lane's next string (after the last round: to the frame's end)
        uint64_t rl = 0, rd = 0;
        const uint8_t* rs = nullptr;
        while (f < f1) {
            const uint32_t s = d->size[f];
            if (s) {
                if constexpr (LEGS) {  // the element step: a record plan's struct bytes, else the leaf's size
                    const uint32_t es = step[k] ? step[k] : s;
                    mv_put(inimg, lds, q, out, o, static_cast<uint32_t>(pos), load_elem(d->col[f] + fr.e * es, s), s);
                } else {
                    mv_put(inimg, lds, q, out, o, static_cast<uint32_t>(pos), load_elem(d->col[f] + fr.e * s, s), s);
                }
                pos += s;
                ++f;
            } else {
                const uint64_t a = d->soffs[f][fr.e], b = d->soffs[f][fr.e + 1];
                mv_put(inimg, lds, q, out, o, static_cast<uint32_t>(pos), b - a, 8);
                pos += 8;
                rl = b - a;
                rs = d->col[f] + a;
                rd = inimg ? (kMvInImage | (q + pos)) : reinterpret_cast<uint64_t>(out + o + pos);
                pos += rl;
                ++f;
                break;
            }
        }
        if (t == rounds) break;  // uniform: no string is left
        uint64_t total;
        const uint64_t at = mv_block_scan(rl, wsum, &total);
        rel[threadIdx.x] = at;
        if (threadIdx.x == 0) rel[kBlock] = total;
        rsrc[threadIdx.x] = rs;
        rdst[threadIdx.x] = rd;
        __syncthreads();
        mv_copy_runs(rel, rsrc, rdst, lds);
        __syncthreads();
    }
    __syncthreads();

    // image -> stream: whole 16-byte chunks inside [lo, hi) as one store, the rest bytewise
    const uint64_t hi = himg;
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

// The second half of the decode, a lane per call of the tile: judge the frame,
// store the call's code, and for a call that is not BAD its fields and string
// lengths.  LEGS: a lane whose call belongs to a record plan (rec) stores no
// field; it leaves pos[j]: its frame's image position, kPosGlobal for a full
// frame that does not lie whole inside the image, or kPosZero.
// lo[]: the tile's offsets, [s0, s0 + staged) the staged span, tmpl the K prefixes.
template <bool LEGS>
__device__ __forceinline__ void mv_parse_lane(const MvDesc* __restrict__ d, const MixLane& r, bool good, bool mine,
                                              bool rec, uint64_t i, uint32_t j, uint32_t nr, const uint32_t* lo,
                                              uint8_t* img, const uint8_t* tmpl, uint64_t s0, uint32_t staged,
                                              const uint8_t* __restrict__ buf, uint64_t buf_len, uint64_t ncalls,
                                              uint32_t unanswered, uint8_t* __restrict__ codes,
                                              uint32_t* __restrict__ srcs, uint32_t* pos, srpc_unpack_status* st) {
    if (!mine) return;
    uint32_t code = SRPC_REPLY_NO_CODE, flag = 0;
    bool full = false;
    uint64_t o = 0;
    const uint8_t* p = nullptr;  // the frame: in the image when it lies whole inside it, else in global memory
    uint32_t body = 0;           // a full frame's first field
    if (j >= nr) {
        code = unanswered;  // no frame: no flag
    } else if (!good) {
        flag = SRPC_STATUS_BOUNDS;  // no plan, or no element to decode into
    } else {
        const uint32_t k = r.cls;
        const uint64_t e = lo[j + 1];
        o = lo[j];
        if (!(o <= e && e <= buf_len) || e - o < 5) {
            flag = SRPC_STATUS_BOUNDS;
        } else {
            const uint64_t len = e - o;
            p = o >= s0 && e - s0 <= staged ? img + (o - s0) : buf + o;
            const uint32_t cb = p[4];
            if (mix_be32(p) != len - 4) {
                flag = SRPC_STATUS_BOUNDS;
            } else {
                code = cb;
                const uint32_t pl = d->prefix_len[k];
                const uint8_t* pre = tmpl + d->tmpl[k];
                if (len == 5 && cb != 0) {
                    // a bare error frame
                } else if (!d->var[k]) {
                    bool eq = len == d->F[k];
                    if (eq)
                        for (uint32_t b = 0; b < pl; ++b) eq &= b == 4 || p[b] == pre[b];
                    if (eq) {
                        full = true;
                        body = pl;
                    } else {
                        flag = SRPC_STATUS_PREFIX;
                    }
                } else {
                    bool eq = len - 4 >= pl;
                    if (eq)
                        for (uint32_t b = 1; b < pl; ++b) eq &= p[4 + b] == pre[b];
                    if (!eq) {
                        flag = SRPC_STATUS_PREFIX;
                    } else {
                        // the walk of the fields ends exactly at the frame's end
                        uint64_t c = 4 + pl;
                        bool ok = true;
                        for (uint32_t f = d->field0[k]; ok && f < d->field0[k + 1]; ++f) {
                            const uint32_t s = d->size[f];
                            if (s) {
                                ok = s <= len - c;
                                c += s;
                            } else if (8 > len - c) {
                                ok = false;
                            } else {
                                const uint64_t sl = mv_get(p + c, 8);
                                c += 8;
                                ok = sl <= len - c;  // 2^63 or 2^64 - 1 cannot wrap
                                if (ok) c += sl;
                            }
                        }
                        if (ok && c == len) {
                            full = true;
                            body = 4 + pl;
                        } else {
                            flag = SRPC_STATUS_BOUNDS;
                        }
                    }
                }
            }
        }
    }
    codes[i] = static_cast<uint8_t>(code);
    if (flag && st) report_bad(st, flag, i);
    if (!good) return;  // no column or offsets element is touched for a bad call
    if constexpr (LEGS) {
        if (rec) {  // a fixed plan: the workgroup writes its struct
            const bool in = full && o >= s0 && lo[j + 1] - s0 <= staged;
            pos[j] = !full ? kPosZero : in ? static_cast<uint32_t>(o - s0) : kPosGlobal;
            return;
        }
    }
    const uint32_t k = r.cls;
    const uint64_t e = d->first[k] + r.rank;
    uint64_t c = body;
    uint32_t t = 0;
    for (uint32_t f = d->field0[k]; f < d->field0[k + 1]; ++f) {
        const uint32_t s = d->size[f];
        if (s) {
            store_elem(d->col[f] + e * s, s, full ? mv_get(p + c, s) : 0);
            c += s;
        } else {
            const uint64_t sl = full ? mv_get(p + c, 8) : 0;
            c += 8;
            d->soffs[f][e + 1] = sl;  // its length: the slot scan turns lengths into offsets
            srcs[t * ncalls + i] = static_cast<uint32_t>(o + c);
            c += sl;
            ++t;
        }
    }
}

// The reply decode of one tile of T calls up to the chars (k_mv_copy's).
// LDS: image[W + 16] | LEGS: the record plans' tables and fills [x.desc_bytes] |
// templates[tmpl_bytes] at kMixImage + 16, then static wcnt and the tile's
// offsets; W = kMixImage, and kMixImage - x.desc_bytes when LEGS.  LEGS also
// holds pos[], slot[] and the slices as static LDS.  x and desc (the tables
// and fills in scratch) are not read when !LEGS.
template <bool LEGS>
__device__ __forceinline__ void mv_parse_tile(const MvDesc* __restrict__ d, const MvLegs* x,
                                              const uint4* __restrict__ desc, const uint8_t* __restrict__ method,
                                              const uint32_t* __restrict__ table, uint64_t rows, uint64_t ncalls,
                                              const uint8_t* __restrict__ buf, uint64_t buf_len,
                                              const uint32_t* __restrict__ offs, uint64_t nframes, uint32_t unanswered,
                                              uint8_t* __restrict__ codes, uint32_t* __restrict__ srcs,
                                              uint32_t* __restrict__ counts, srpc_unpack_status* st) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    __shared__ uint32_t wcnt[kMixLds];
    __shared__ uint32_t lo[kBlock + 1];
    __shared__ uint32_t pos[LEGS ? kBlock : 1];
    __shared__ uint16_t slot[LEGS ? kBlock : 1];
    __shared__ std::conditional_t<LEGS, MixAosSlices, uint32_t> sl;
    uint8_t* img = lds;
    const uint8_t* tmpl = lds + kMixImage + 16;
    const uint32_t K = d->nplans, T = d->T;
    uint32_t window = kMixImage;
    if constexpr (LEGS) window = x->window;
    mv_templates(lds + kMixImage + 16, d);
    if constexpr (LEGS) {
        mix_aos_slices_init(sl, x->x, K);
        uint4* dsc = reinterpret_cast<uint4*>(lds + window + 16);
        for (uint32_t c = threadIdx.x; c < x->x.desc_bytes / 16; c += kBlock) dsc[c] = desc[c];
    }
    const uint64_t c0 = static_cast<uint64_t>(blockIdx.x) * T;
    const uint64_t g = c0 / kMixGranule;
    const uint32_t j0 = static_cast<uint32_t>(c0 - g * kMixGranule);
    const uint64_t i = g * kMixGranule + threadIdx.x;
    const uint32_t nr = c0 < nframes ? static_cast<uint32_t>(min<uint64_t>(T, nframes - c0)) : 0;
    for (uint32_t j = threadIdx.x; j <= T; j += kBlock) lo[j] = c0 + j < nframes ? offs[c0 + j] : static_cast<uint32_t>(buf_len);

    const MixLane r = mix_ranks(method, ncalls, K, table, rows, g, wcnt);  // barrier: lo[] is complete
    const bool good = r.cls < K && r.rank < d->room[r.cls];
    // the chunk's calls per plan, for the slot scan: the last tile's granule is the last one
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x < K) {
        uint32_t v = wcnt[kMixWaves * kMixRow + threadIdx.x];
        for (uint32_t w = 0; w < kMixWaves; ++w) v += wcnt[w * kMixRow + threadIdx.x];
        counts[threadIdx.x] = v;
    }
    bool rec = false;  // a good call of the tile whose plan is a record plan
    if constexpr (LEGS) {
        rec = threadIdx.x >= j0 && threadIdx.x < j0 + T && i < ncalls && good && sl.stride[r.cls] != 0;
        // the tile's slices: good calls of one plan are consecutive ranks, ascending with the lane
        mix_aos_slices_count(sl, K, r, rec);
    }

    // 1. the span of the tile's frames -> image, from a 16-byte boundary
    uint64_t s0 = 0;
    uint32_t staged = 0;
    if (nr) {
        const uint64_t o0 = lo[0], oe = lo[nr];
        s0 = o0 & ~15ull;
        if (o0 <= buf_len) {
            const uint64_t end = oe >= o0 && oe <= buf_len ? oe : buf_len;
            staged = static_cast<uint32_t>(min<uint64_t>(end - s0, window));
        }
    }
    const uint8_t* src = buf + s0;
    const uint32_t full16 = staged >> 4;
    for (uint32_t cb = threadIdx.x; cb < full16; cb += kBlock)
        *reinterpret_cast<uint4*>(img + 16 * cb) = *reinterpret_cast<const uint4*>(src + 16 * cb);
    for (uint32_t b = full16 * 16 + threadIdx.x; b < staged; b += kBlock) img[b] = src[b];
    __syncthreads();

    // 2. a lane per call: judge its frame, store its code, fields and string lengths
    const bool mine = threadIdx.x >= j0 && threadIdx.x < j0 + T && i < ncalls;
    mv_parse_lane<LEGS>(d, r, good, mine, rec, i, threadIdx.x - j0, nr, lo, img, tmpl, s0, staged, buf, buf_len, ncalls,
                        unanswered, codes, srcs, pos, st);

    // 3. image, zero and fill -> the record plans' slices, one lane per (plan, 16-byte piece)
    if constexpr (LEGS)
        mix_aos_store<true>(sl, *d, K, r, rec, threadIdx.x - j0, img, lo, pos, slot, lds + window + 16, buf);
}

}  // namespace srpc_impl
