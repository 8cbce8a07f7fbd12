// frames_aos.hip -- the client's reply decode written straight into an array
// of the caller's own structs (srpc_frames_unpack_replies_aos): the AoS form of
// srpc_frames_unpack_replies (frames.hip, k_unpack_replies).
//
// The frame contract, the per-frame table, the codes and the status are the
// column call's; steps 1 and 2 below are k_unpack_replies's steps 1 and 2, kept
// in step with it on purpose (tests/test_gpu_replies_aos.py asserts the codes
// and the status of both calls equal on every input).  A workgroup takes R
// consecutive frames:
//
//   1. their span, from a 16-byte boundary, into an LDS image with 16-byte
//      loads (bytes past the last whole chunk inside buf_len bytewise);
//   2. one lane per frame judges it against the plan's prefix (template | mask
//      in LDS, the code byte masked out), writes its code and leaves pos[j]:
//      the frame's image position, "outside the image" or "fields are zero";
//   3. one lane per 16-byte piece of the tile's slice of the struct array
//      assembles that piece and stores it whole.  A table in LDS holds, for
//      every byte k of the struct, where it comes from -- a wire offset (a leaf
//      byte) or "fill" -- and how many of the following struct bytes continue
//      that run (consecutive wire bytes, or fill; at most 8).  A lane walks its
//      piece run by run: leaf bytes of a full frame from the image (eight
//      bytes per aligned LDS read), zero for leaf bytes of other frames, an LDS
//      copy of the fill record for every other byte.
//
// R is a multiple of 16, so every tile's slice starts on a 16-byte boundary of
// the 16-byte aligned array and only the array's last piece can be partial: it
// is stored bytewise.  Every struct byte is written exactly once and none is
// read (the store pattern of srpc_gpu_unpack_aos_fill's piece kernels,
// DESIGN §4.5).  A full frame outside the image (an oversize junk frame before
// it used the image up) is read from global memory, at most F bytes.
// LDS: image[R*F + 32] | tmpl[P8] | mask[P8] | pos[R] | offs[R + 1] (indexed)
//      | table[S16] (u16) | fill[S16 + 16],  S16 = stride rounded up to 16.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "aos_pieces.h"
#include "plan.h"
#include "srpc_gpu.h"

namespace srpc_impl {
namespace {

constexpr uint32_t kReplyTileBytes = 16384;   // LDS budget of image + table + fill, as the column kernel's image
constexpr int kReplyLoads = 4;                // 16-byte loads in flight per lane

struct ReplyAosArgs {
    const uint8_t* prefix;  // the plan's device prefix (zero-padded 16 bytes past its end)
    uint32_t F;             // bytes of a full frame
    uint32_t prefix_len;
    uint32_t R;             // frames per tile (multiple of 16)
    uint32_t stride;        // struct bytes
    uint16_t tab[kAosMaxStride];      // struct byte k: (run bytes from k on, 1..8) << 12 | wire offset or kSrcFill
    uint32_t fillw[kAosMaxStride / 4];  // the fill record (stride bytes, zero padded)
};

// Frames per tile: the column kernel's rule with the table's and the fill's
// bytes (2 S16 + S16, and their padding: under S16) taken out of the image's
// budget, so a workgroup's LDS stays under the column kernel's for the same F.
inline uint32_t reply_aos_tile_frames(uint32_t F, uint32_t stride) {
    return 16 * std::max<uint32_t>(1, (kReplyTileBytes - 4 * s16_of(stride)) / (16 * F));
}

inline size_t reply_aos_lds_bytes(uint32_t F, uint32_t prefix_len, uint32_t R, uint32_t stride, bool indexed) {
    return static_cast<size_t>(R) * F + 32 + 2 * ((prefix_len + 7) & ~7u) + 4 * R + (indexed ? 4 * (R + 1) : 0) + 12 +
           3 * s16_of(stride) + 16;
}

__device__ __forceinline__ uint32_t be32_at(const uint8_t* b) {
    return (static_cast<uint32_t>(b[0]) << 24) | (static_cast<uint32_t>(b[1]) << 16) |
           (static_cast<uint32_t>(b[2]) << 8) | static_cast<uint32_t>(b[3]);
}

template <bool INDEXED>
__global__ __launch_bounds__(kBlock) void k_unpack_replies_aos(ReplyAosArgs a, const uint8_t* __restrict__ buf,
                                                               uint64_t buf_len, const uint32_t* __restrict__ offs,
                                                               uint64_t n, uint8_t* __restrict__ recs,
                                                               uint8_t* __restrict__ codes, srpc_unpack_status* st) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const uint32_t cap = a.R * a.F + 16;  // image bytes a tile may stage (a multiple of 16)
    const uint32_t p8 = (a.prefix_len + 7) & ~7u;
    const uint32_t s16 = (a.stride + 15) & ~15u;
    uint8_t* img = lds;
    uint8_t* tmpl = lds + cap + 16;
    uint8_t* mask = tmpl + p8;
    uint32_t* pos = reinterpret_cast<uint32_t*>(mask + p8);
    uint32_t* lo = pos + a.R;  // indexed mode: the tile's offsets, lo[nr] = its end
    // table and fill start on a 16-byte boundary (cap, p8 and 4 R keep 8; R + 1 offsets may leave 4 or 12)
    const uint32_t after = cap + 16 + 2 * p8 + 4 * a.R + (INDEXED ? 4 * (a.R + 1) : 0);
    uint16_t* tab = reinterpret_cast<uint16_t*>(lds + ((after + 15) & ~15u));
    uint8_t* fill = reinterpret_cast<uint8_t*>(tab) + 2 * s16;
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * a.R;
    const uint32_t nr = static_cast<uint32_t>(min<uint64_t>(a.R, n - base));

    // the plan's prefix without its code byte, as template | mask; the struct's table and fill
    for (uint32_t i = threadIdx.x; i < p8; i += kBlock) {
        const bool keep = i < a.prefix_len && i != 4;
        tmpl[i] = keep ? a.prefix[i] : 0;
        mask[i] = keep ? 0xff : 0;
    }
    for (uint32_t i = threadIdx.x; i < s16 / 2; i += kBlock)
        reinterpret_cast<uint32_t*>(tab)[i] = reinterpret_cast<const uint32_t*>(a.tab)[i];
    for (uint32_t i = threadIdx.x; i < s16 / 4 + 4; i += kBlock)
        reinterpret_cast<uint32_t*>(fill)[i] = i < kAosMaxStride / 4 ? a.fillw[i] : 0;
    uint64_t s0;       // stream offset of the image's first byte (a multiple of 16)
    uint32_t staged;   // image bytes
    if constexpr (INDEXED) {
        for (uint32_t j = threadIdx.x; j <= nr; j += kBlock)
            lo[j] = base + j < n ? offs[base + j] : static_cast<uint32_t>(buf_len);
        __syncthreads();
        const uint64_t o0 = lo[0], oe = lo[nr];
        s0 = o0 & ~15ull;
        if (o0 > buf_len) {
            staged = 0;
        } else {
            const uint64_t end = oe >= o0 && oe <= buf_len ? oe : buf_len;
            staged = static_cast<uint32_t>(min<uint64_t>(end - s0, cap));
        }
    } else {
        s0 = base * a.F;
        staged = s0 >= buf_len ? 0 : static_cast<uint32_t>(min<uint64_t>(buf_len - s0, static_cast<uint64_t>(nr) * a.F));
    }

    // 1. stream -> image
    const uint8_t* src = buf + s0;
    const uint32_t full = staged >> 4;
    for (uint32_t c0 = threadIdx.x; c0 < full; c0 += kBlock * kReplyLoads) {
        uint4 vv[kReplyLoads];
#pragma unroll
        for (int u = 0; u < kReplyLoads; ++u) {
            // lanes past the span's end load its last chunk again: every slot is
            // defined, so the batch stays in registers
            const uint32_t c = min(c0 + u * kBlock, full - 1);
            vv[u] = *reinterpret_cast<const uint4*>(src + 16 * c);
        }
#pragma unroll
        for (int u = 0; u < kReplyLoads; ++u) {
            const uint32_t c = c0 + u * kBlock;
            if (c < full) *reinterpret_cast<uint4*>(img + 16 * c) = vv[u];
        }
    }
    for (uint32_t i = full * 16 + threadIdx.x; i < staged; i += kBlock) img[i] = src[i];
    __syncthreads();

    // 2. one lane per frame: code, status, where its fields are
    for (uint32_t j = threadIdx.x; j < nr; j += kBlock) {
        uint64_t o, e;
        if constexpr (INDEXED) {
            o = lo[j];
            e = lo[j + 1];
        } else {
            o = s0 + static_cast<uint64_t>(j) * a.F;
            e = o + a.F;
        }
        uint32_t code = SRPC_REPLY_NO_CODE, p = kPosZero, flag = 0;
        if (!(o <= e && e <= buf_len) || e - o < 5) {
            flag = SRPC_STATUS_BOUNDS;  // out of order, past the end, no header or no payload
        } else {
            const uint64_t len = e - o;
            const uint64_t need = len == a.F ? len : 5;
            const bool in_img = o >= s0 && o - s0 + need <= staged;
            const uint32_t q = static_cast<uint32_t>(o - s0);
            const uint8_t* h = in_img ? img + q : buf + o;
            const uint32_t be = be32_at(h), c0 = h[4];
            if (be != len - 4) {
                flag = SRPC_STATUS_BOUNDS;
            } else {
                code = c0;
                if (len == a.F) {
                    bool eq = true;
                    if (in_img) {
                        for (uint32_t b = 0; b < p8; b += 8)
                            eq &= ((lds_u64(img, q + b) ^ *reinterpret_cast<const uint64_t*>(tmpl + b)) &
                                   *reinterpret_cast<const uint64_t*>(mask + b)) == 0;
                    } else {
                        for (uint32_t b = 0; b < a.prefix_len; ++b) eq &= ((buf[o + b] ^ tmpl[b]) & mask[b]) == 0;
                    }
                    if (eq) p = in_img ? q : kPosGlobal;
                    else flag = SRPC_STATUS_PREFIX;
                } else if (!(len == 5 && c0 != 0)) {  // not a bare error frame either
                    flag = SRPC_STATUS_PREFIX;
                }
            }
        }
        pos[j] = p;
        codes[base + j] = static_cast<uint8_t>(code);
        if (flag && st) report_bad(st, flag, base + j);
    }
    __syncthreads();

    // 3. image, zero and fill -> the tile's structs, one lane per 16-byte piece
    uint8_t* dst = recs + base * a.stride;
    const uint32_t tbytes = nr * a.stride;
    const uint32_t npieces = (tbytes + 15) >> 4;
    for (uint32_t c = threadIdx.x; c < npieces; c += kBlock) {
        const uint32_t x0 = 16 * c;
        const uint32_t cnt = min(16u, tbytes - x0);
        uint32_t e = x0 / a.stride;
        uint32_t k = x0 - e * a.stride;
        uint32_t p = pos[e];
        uint64_t vlo = 0, vhi = 0;
        uint32_t b = 0;
        while (b < cnt) {
            const uint32_t t = tab[k];
            const uint32_t m = min(t >> 12, cnt - b), w = t & 0xfff;
            uint64_t v = 0;
            if (w == kSrcFill) {
                v = lds_u64(fill, k);
            } else if (p < kPosGlobal) {
                v = lds_u64(img, p + w);
            } else if (INDEXED && p == kPosGlobal) {
                const uint8_t* g = buf + lo[e] + w;  // inside the frame: w + m <= F
                for (uint32_t y = 0; y < m; ++y) v |= static_cast<uint64_t>(g[y]) << (8 * y);
            }
            piece_put(vlo, vhi, b, v, m);
            b += m;
            k += m;
            if (k == a.stride) {  // runs end with their struct
                k = 0;
                ++e;
                if (b < cnt) p = pos[e];  // b < cnt <= tbytes - x0 keeps e < nr
            }
        }
        if (cnt == 16) {
            __builtin_nontemporal_store(aos_u32x4{static_cast<uint32_t>(vlo), static_cast<uint32_t>(vlo >> 32),
                                                 static_cast<uint32_t>(vhi), static_cast<uint32_t>(vhi >> 32)},
                                        reinterpret_cast<aos_u32x4*>(dst + x0));
        } else {  // the array's last, partial piece: its own bytes only
            for (uint32_t y = 0; y < cnt; ++y)
                dst[x0 + y] = static_cast<uint8_t>(y < 8 ? vlo >> (8 * y) : vhi >> (8 * (y - 8)));
        }
    }
}

int reply_aos_plan_ok(const srpc_plan* p, uint64_t record_stride) {
    if (p->has_string || p->prefix_len < 5 || record_stride > kAosMaxStride) return SRPC_E_UNSUPPORTED;
    return SRPC_OK;
}

}  // namespace
}  // namespace srpc_impl

using namespace srpc_impl;

extern "C" {

int srpc_frames_replies_aos_per_tile(const srpc_plan* reply_plan, uint64_t record_stride, uint32_t* out) {
    if (!reply_plan || !out || record_stride == 0) return SRPC_E_INVALID;
    if (int rc = reply_aos_plan_ok(reply_plan, record_stride)) return rc;
    *out = reply_aos_tile_frames(static_cast<uint32_t>(reply_plan->stride), static_cast<uint32_t>(record_stride));
    return SRPC_OK;
}

int srpc_frames_unpack_replies_aos(const srpc_plan* reply_plan, const uint8_t* d_buf, uint64_t buf_len,
                                   const uint32_t* d_offs, uint64_t nframes, void* d_records, uint64_t record_stride,
                                   const uint32_t* field_offsets, const void* h_fill, uint8_t* d_codes,
                                   srpc_unpack_status* d_status, void* stream) {
    const TimedCall timed;
    // the pointers, the stride and the length are checked before the plan is looked at
    if (!reply_plan || (nframes && !d_records) || !field_offsets || !h_fill || !d_codes || record_stride == 0 ||
        buf_len >= (1ull << 32))
        return SRPC_E_INVALID;
    const srpc_plan* p = reply_plan;
    if (int rc = reply_aos_plan_ok(p, record_stride)) return rc;
    if (nframes > 0xffffffffull) return SRPC_E_UNSUPPORTED;
    if (nframes && !d_buf) return SRPC_E_INVALID;
    const uint32_t stride = static_cast<uint32_t>(record_stride);
    // the struct's bytes: -1 fill, else the wire offset of the leaf byte there
    int32_t from[kAosMaxStride];
    if (int rc = aos_sources(p, field_offsets, stride, from)) return rc;
    if (!aligned(d_buf, 16) || !aligned(d_records, 16)) return SRPC_E_ALIGN;
    if (!aos_layout_aligned(p, field_offsets, stride)) return SRPC_E_ALIGN;  // as in C++ structs
    auto s = static_cast<hipStream_t>(stream);
    if (d_status && status_reset_launch(d_status, s)) return SRPC_E_HIP;
    if (!nframes) return SRPC_OK;
    ReplyAosArgs a{};
    a.prefix = p->d_prefix;
    a.F = static_cast<uint32_t>(p->stride);
    a.prefix_len = p->prefix_len;
    a.stride = stride;
    a.R = reply_aos_tile_frames(a.F, stride);
    std::memcpy(a.fillw, h_fill, stride);
    aos_run_table(from, stride, a.tab);
    const uint32_t grid = static_cast<uint32_t>((nframes + a.R - 1) / a.R);
    const size_t lds = reply_aos_lds_bytes(a.F, a.prefix_len, a.R, stride, d_offs != nullptr);
    auto* recs = static_cast<uint8_t*>(d_records);
    if (d_offs) launch(k_unpack_replies_aos<true>, dim3(grid), dim3(kBlock), lds, s, a, d_buf, buf_len, d_offs, nframes, recs, d_codes, d_status);
    else launch(k_unpack_replies_aos<false>, dim3(grid), dim3(kBlock), lds, s, a, d_buf, buf_len, d_offs, nframes, recs, d_codes, d_status);
    if (hipGetLastError() != hipSuccess) return SRPC_E_HIP;
    // uniform mode, a stream shorter than nframes full frames: as srpc_gpu_unpack
    return !d_offs && buf_len / a.F < nframes ? SRPC_ERR_BOUNDS : SRPC_OK;
}

}  // extern "C"
