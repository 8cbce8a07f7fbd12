// frames.hip -- server-side batches of framed requests of several methods
// (SURVEY §8 f1).  The reference server dispatches every request by its
// method name (server.hpp:58-69: recv_data -> `>> funcname` -> call); a batch
// read from a socket holds frames of any registered method, in any order.
// srpc_frames_classify buckets such a batch on the GPU: frame i belongs to
// request plan k when it is exactly one record of that plan (its length is
// the plan's record bytes and it starts with the plan's constant prefix --
// BE32 length | str(method) | str(Req::name) for a framed request plan), the
// first matching plan winning.  Each bucket is then gathered into a
// contiguous batch for the plan's ordinary unpack, and the packed responses
// are scattered back into request order (srpc_frames_gather / _scatter).
// Frames no plan matches are left to the caller (the CPU server).
//
// Methods with string fields (variable-length frames) take var plans whose
// prefix is `str(method) | str(Req::name)` after the frame's BE32 length: a
// frame is such a plan's when its BE32 is its payload length, the payload
// starts with the prefix, and its fields walk to exactly the frame's end
// (every string length inside the frame) -- the one record of that plan the
// reference server would unpack from it (server.hpp:58-69, packer.hpp:216-222).
// Their payloads are gathered with a record index (srpc_frames_gather_var)
// for srpc_gpu_unpack_var, the packed responses are framed and scattered by
// the response index srpc_gpu_pack_var writes (srpc_frames_scatter_var), and
// the reply stream's offsets are recomputed once those sizes are known
// (srpc_frames_offsets).
//
// Client side (srpc::gpu::batch_client): the reply stream of a batch of calls
// -- full frames, bare error frames, junk -- is decoded in call order by one
// kernel, k_unpack_replies (srpc_frames_unpack_replies), described below.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "plan.h"
#include "scan.h"
#include "srpc_gpu.h"

namespace srpc_impl {
namespace {

constexpr uint32_t kNoClass = SRPC_FRAME_UNKNOWN;
constexpr int kMaxPlans = SRPC_FRAMES_MAX_PLANS;
constexpr int kMaxStr = SRPC_FRAMES_MAX_STRINGS;

struct ClassArgs {
    const uint8_t* prefix[kMaxPlans];  // device prefix of plan k
    uint32_t prefix_len[kMaxPlans];
    uint32_t frame_bytes[kMaxPlans];   // fixed plans: the record bytes (the whole frame); var: the least payload
    uint32_t resp_bytes[kMaxPlans];    // bytes of one response of plan k (0 for var plans)
    // var plans: fixed bytes before string s's length word (after the prefix or
    // the previous string's chars), gap[k][nstr[k]] = fixed bytes after the last
    uint16_t gap[kMaxPlans][kMaxStr + 1];
    uint8_t nstr[kMaxPlans];           // 0: a fixed plan
    uint32_t nplans;
};

__device__ __forceinline__ uint32_t be32_at(const uint8_t* b) {
    return (static_cast<uint32_t>(b[0]) << 24) | (static_cast<uint32_t>(b[1]) << 16) |
           (static_cast<uint32_t>(b[2]) << 8) | static_cast<uint32_t>(b[3]);
}

template <typename T>
__device__ __forceinline__ T ldu(const uint8_t* p) {
    T v;
    __builtin_memcpy(&v, p, sizeof(T));
    return v;
}

// One lane per frame: class, bucket slot (wave-aggregated atomics: one add per
// wave and plan), response bytes; block sums of the response bytes.
__global__ __launch_bounds__(kBlock) void k_classify(ClassArgs a, const uint8_t* __restrict__ buf, uint64_t buf_len,
                                                     const uint32_t* __restrict__ offs, uint64_t nf,
                                                     uint8_t* __restrict__ cls, uint32_t* __restrict__ index,
                                                     uint64_t* __restrict__ counts, uint32_t* __restrict__ rb) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
    uint32_t k = kNoClass;
    if (i < nf) {
        const uint64_t o = offs[i];
        const uint64_t end = i + 1 < nf ? offs[i + 1] : buf_len;
        // offsets out of order or past the buffer: the frame is no plan's (the
        // caller answers it), and no byte outside [0, buf_len) is read
        const bool inside = o <= end && end <= buf_len;
        for (uint32_t p = 0; inside && p < a.nplans && k == kNoClass; ++p) {
            const uint32_t ns = a.nstr[p];
            const uint64_t len = end - o;
            if (ns == 0 ? len != a.frame_bytes[p] : (len < 4 + uint64_t{a.frame_bytes[p]} || be32_at(buf + o) != len - 4))
                continue;
            const uint64_t at = ns ? o + 4 : o;  // var plans: the prefix follows the BE32 length
            if (a.prefix_len[p] > end - at) continue;
            const uint8_t* f = buf + at;
            const uint8_t* q = a.prefix[p];
            bool eq = true;
            uint32_t b = 0;
            for (; b + 8 <= a.prefix_len[p] && eq; b += 8) eq = ldu<uint64_t>(f + b) == ldu<uint64_t>(q + b);
            for (; b < a.prefix_len[p] && eq; ++b) eq = f[b] == q[b];
            if (eq && ns) {  // the record's walk ends exactly at the frame's end
                uint64_t c = at + a.prefix_len[p];
                for (uint32_t t = 0; t < ns && eq; ++t) {
                    c += a.gap[p][t];
                    if (c + 8 > end) {
                        eq = false;
                        break;
                    }
                    const uint64_t sl = ldu<uint64_t>(buf + c);
                    c += 8;
                    if (sl > end - c) eq = false;
                    else c += sl;
                }
                eq = eq && c + a.gap[p][ns] == end;
            }
            if (eq) k = p;
        }
        cls[i] = static_cast<uint8_t>(k);
        rb[i] = k == kNoClass ? 0 : a.resp_bytes[k];
    }
    // bucket slots: per plan, the wave's matching lanes take consecutive slots
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t p = 0; p < a.nplans; ++p) {
        const uint64_t m = __ballot(k == p);
        if (!m) continue;
        const uint32_t leader = __builtin_ctzll(m);
        uint64_t base = 0;
        if (lane == leader) base = atomicAdd(reinterpret_cast<unsigned long long*>(&counts[p]),
                                             static_cast<unsigned long long>(__popcll(m)));
        base = __shfl(base, leader, 64);
        if (k == p) index[p * nf + base + __popcll(m & ((1ull << lane) - 1))] = static_cast<uint32_t>(i);
    }
    const uint64_t mu = __ballot(i < nf && k == kNoClass);
    if (mu && lane == __builtin_ctzll(mu))
        atomicAdd(reinterpret_cast<unsigned long long*>(&counts[a.nplans + 1]), static_cast<unsigned long long>(__popcll(mu)));
}

// Bucket -> contiguous batch: 4 bytes per lane of the output (n records of
// rec bytes); record j is frame index[j].
__global__ __launch_bounds__(kBlock) void k_gather(const uint8_t* __restrict__ buf, const uint32_t* __restrict__ offs,
                                                   const uint32_t* __restrict__ index, uint64_t n, uint32_t rec,
                                                   uint8_t* __restrict__ out) {
    const uint64_t total = n * rec;
    const uint64_t gs = static_cast<uint64_t>(gridDim.x) * kBlock * 4;
    for (uint64_t x = (static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x) * 4; x < total; x += gs) {
        uint32_t w = 0;
        for (uint32_t b = 0; b < 4 && x + b < total; ++b) {
            const uint64_t j = (x + b) / rec, k = (x + b) - j * rec;
            w |= static_cast<uint32_t>(buf[offs[index[j]] + k]) << (8 * b);
        }
        if (x + 4 <= total) *reinterpret_cast<uint32_t*>(out + x) = w;
        else
            for (uint32_t b = 0; x + b < total; ++b) out[x + b] = static_cast<uint8_t>(w >> (8 * b));
    }
}

// Packed responses (n records of rec bytes) -> their frames' places.
__global__ __launch_bounds__(kBlock) void k_scatter(const uint8_t* __restrict__ resp, const uint32_t* __restrict__ index,
                                                    uint64_t n, uint32_t rec, const uint64_t* __restrict__ out_off,
                                                    uint8_t* __restrict__ out) {
    const uint64_t total = n * rec;
    const uint64_t gs = static_cast<uint64_t>(gridDim.x) * kBlock;
    for (uint64_t x = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; x < total; x += gs) {
        const uint64_t j = x / rec, k = x - j * rec;
        out[out_off[index[j]] + k] = resp[x];
    }
}

// Payload bytes (the frame after its BE32) of bucket record j.
__global__ __launch_bounds__(kBlock) void k_payload_lens(const uint8_t* __restrict__ buf, const uint32_t* __restrict__ offs,
                                                         const uint32_t* __restrict__ index, uint64_t n,
                                                         uint32_t* __restrict__ lens) {
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (j < n) lens[j] = be32_at(buf + offs[index[j]]);
}

// A wave per record (grid-stride): payload j -> out + rec_offs[j].
__global__ __launch_bounds__(kBlock) void k_gather_var(const uint8_t* __restrict__ buf, const uint32_t* __restrict__ offs,
                                                       const uint32_t* __restrict__ index, uint64_t n,
                                                       const uint64_t* __restrict__ rec_offs, uint8_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = static_cast<uint64_t>(gridDim.x) * (kBlock / 64);
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * (kBlock / 64) + threadIdx.x / 64; j < n; j += waves) {
        const uint8_t* src = buf + offs[index[j]] + 4;
        const uint64_t o = rec_offs[j], len = rec_offs[j + 1] - o;
        for (uint64_t b = lane; b < len; b += 64) out[o + b] = src[b];
    }
}

// A wave per response (grid-stride): BE32(len) | response j at out + out_off[index[j]].
__global__ __launch_bounds__(kBlock) void k_scatter_var(const uint8_t* __restrict__ resp,
                                                        const uint64_t* __restrict__ rec_offs,
                                                        const uint32_t* __restrict__ index, uint64_t n,
                                                        const uint64_t* __restrict__ out_off, uint8_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = static_cast<uint64_t>(gridDim.x) * (kBlock / 64);
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * (kBlock / 64) + threadIdx.x / 64; j < n; j += waves) {
        const uint64_t r = rec_offs[j], len = rec_offs[j + 1] - r;
        uint8_t* dst = out + out_off[index[j]];
        if (lane < 4) dst[lane] = static_cast<uint8_t>(len >> (8 * (3 - lane)));
        for (uint64_t b = lane; b < len; b += 64) dst[4 + b] = resp[r + b];
    }
}

struct VarOffs {
    const uint64_t* rec[kMaxPlans];  // response index of var plan k (NULL: a fixed plan)
};

// Response bytes of every frame: resp_bytes[k] for a fixed plan's frame, 0 for
// an unknown one (var plans' frames: k_var_sizes).
__global__ __launch_bounds__(kBlock) void k_fixed_sizes(const uint8_t* __restrict__ cls, uint64_t nf, ClassArgs a,
                                                        uint32_t* __restrict__ sizes) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= nf) return;
    const uint32_t c = cls[i];
    sizes[i] = c < a.nplans && a.nstr[c] == 0 ? a.resp_bytes[c] : 0;
}

// blockIdx.y = plan: BE32 + response bytes of each frame of a var plan's bucket.
__global__ __launch_bounds__(kBlock) void k_var_sizes(const uint32_t* __restrict__ index, uint64_t nf,
                                                      const uint64_t* __restrict__ counts, VarOffs v,
                                                      uint32_t* __restrict__ sizes) {
    const uint32_t k = blockIdx.y;
    const uint64_t* rec = v.rec[k];
    if (!rec) return;
    const uint64_t nk = counts[k];
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; j < nk;
         j += static_cast<uint64_t>(gridDim.x) * kBlock)
        sizes[index[k * nf + j]] = static_cast<uint32_t>(4 + rec[j + 1] - rec[j]);
}

__global__ void k_zero_counts(uint64_t* c, uint32_t n) {
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) c[i] = 0;
}

// The plans' match rules (see the file comment); SRPC_E_INVALID for a plan
// without a prefix, SRPC_E_UNSUPPORTED past SRPC_FRAMES_MAX_STRINGS strings.
int class_args(const srpc_plan* const* plans, const uint32_t* resp_bytes, int nplans, ClassArgs* a) {
    for (int k = 0; k < nplans; ++k) {
        const srpc_plan* p = plans[k];
        if (!p || p->prefix_len == 0) return SRPC_E_INVALID;
        a->prefix[k] = p->d_prefix;
        a->prefix_len[k] = p->prefix_len;
        if (!p->has_string) {
            a->frame_bytes[k] = static_cast<uint32_t>(p->stride);
            a->resp_bytes[k] = resp_bytes ? resp_bytes[k] : 0;
            continue;
        }
        if (p->nstrings > static_cast<uint32_t>(kMaxStr)) return SRPC_E_UNSUPPORTED;
        a->frame_bytes[k] = p->fixed_bytes;
        a->nstr[k] = static_cast<uint8_t>(p->nstrings);
        uint32_t t = 0, run = 0;
        for (uint32_t f = 0; f < p->nfields; ++f) {
            if (p->kinds[f] == SRPC_KIND_STRING) {
                a->gap[k][t++] = static_cast<uint16_t>(run);
                run = 0;
            } else {
                run += p->size[f];
            }
        }
        a->gap[k][t] = static_cast<uint16_t>(run);
    }
    a->nplans = static_cast<uint32_t>(nplans);
    return SRPC_OK;
}

uint32_t grid_for(uint64_t work, uint64_t per) {
    return static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>((work + per - 1) / per, 1u << 20)));
}

// ---------------------------------------------------------------------------
// Client side: a reply stream of mixed frames -> columns and one code per call,
// in call order (srpc_frames_unpack_replies).
//
// A workgroup takes R consecutive frames.  Their bytes are contiguous in the
// stream, so the tile is one span starting at a 16-byte boundary: it is staged
// into an LDS image with 16-byte loads (the bytes past the last whole chunk
// inside buf_len bytewise; nothing past buf_len is read).  One lane per frame
// then checks the frame against the table in srpc_gpu.h -- offsets, BE32,
// length, and the plan's prefix (code byte masked out) eight bytes at a time
// from aligned LDS dwords -- and leaves the frame's image position in pos[]
// (or "fields are zero").  Every field's column is then written as 16-byte
// chunks gathered from the image through pos[], as k_unpack_tile does with a
// fixed stride.  A frame whose bytes lie outside the image (an oversize junk
// frame before it used the image up, or its offset is out of order) is read
// from global memory on its own, at most F bytes.
// LDS: image[R*F + 32] | tmpl[P8] | mask[P8] | pos[R] | offs[R + 1] (indexed).
// ---------------------------------------------------------------------------
constexpr uint32_t kReplyTileBytes = 16384;  // target image bytes per tile
constexpr uint32_t kPosZero = 0xffffffffu;   // pos[j]: the frame's fields are zero
constexpr uint32_t kPosGlobal = 0xfffffffeu; // pos[j]: a full frame outside the image
constexpr int kReplyLoads = 4;               // 16-byte loads in flight per lane

typedef uint32_t r_u32x4 __attribute__((ext_vector_type(4)));

struct ReplyArgs {
    uint8_t* col[kMaxFields];
    uint32_t size[kMaxFields];
    uint32_t off[kMaxFields];  // field offset inside the frame
    const uint8_t* prefix;     // the plan's device prefix (zero-padded 16 bytes past its end)
    uint32_t nfields;
    uint32_t F;                // bytes of a full frame
    uint32_t prefix_len;
    uint32_t R;                // frames per tile (multiple of 16)
};

inline uint32_t reply_tile_frames(uint32_t F) { return 16 * std::max<uint32_t>(1, kReplyTileBytes / (16 * F)); }

inline size_t reply_lds_bytes(uint32_t F, uint32_t prefix_len, uint32_t R, bool indexed) {
    return static_cast<size_t>(R) * F + 32 + 2 * ((prefix_len + 7) & ~7u) + 4 * R + (indexed ? 4 * (R + 1) : 0);
}

// S <= 8 bytes at any LDS byte offset from aligned dword reads (may read up to
// 8 bytes past the value, inside the image's padding).
template <int S>
__device__ __forceinline__ uint64_t lds_get(const uint8_t* lds, uint32_t at) {
    if constexpr (S == 1) {
        return lds[at];
    } else if constexpr (S == 8) {
        return lds_u64(lds, at);
    } else {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(lds + (at & ~3u));
        const uint32_t v = __builtin_amdgcn_alignbyte(w[1], w[0], at & 3);
        return S == 2 ? (v & 0xffffu) : v;
    }
}

// Field bytes [off, off + S) of the tile's frame e: from the image, from global
// memory (a full frame outside the image), or zero.
template <int S, bool INDEXED>
__device__ __forceinline__ uint64_t reply_elem(const uint8_t* img, const uint32_t* pos, const uint32_t* lo,
                                               const uint8_t* __restrict__ buf, uint32_t off, uint32_t e) {
    const uint32_t p = pos[e];
    uint64_t v = 0;
    if (p < kPosGlobal) {
        v = lds_get<S>(img, p + off);
    } else if (INDEXED && p == kPosGlobal) {
        const uint8_t* g = buf + lo[e] + off;
#pragma unroll
        for (int k = 0; k < S; ++k) v |= static_cast<uint64_t>(g[k]) << (8 * k);
    }
    return v;
}

template <int S, bool INDEXED>
__device__ __forceinline__ void reply_chunk(const uint8_t* img, const uint32_t* pos, const uint32_t* lo,
                                            const uint8_t* __restrict__ buf, uint32_t off, uint32_t c, uint32_t nr,
                                            uint8_t* dstc) {
    constexpr uint32_t per = 16 / S;
    const uint32_t e0 = c * per;
    if (e0 + per <= nr) {
        // the chunk's positions with 8- or 16-byte LDS reads (pos + e0 is aligned
        // to its 4 * per bytes); a branch-free gather unless a frame of the chunk
        // lies outside the image, so the LDS reads of all elements issue together
        uint32_t p[per];
        if constexpr (per == 2) {
            const uint2 t = *reinterpret_cast<const uint2*>(pos + e0);
            p[0] = t.x;
            p[1] = t.y;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < per; j += 4) {
                const uint4 t = *reinterpret_cast<const uint4*>(pos + e0 + j);
                p[j] = t.x;
                p[j + 1] = t.y;
                p[j + 2] = t.z;
                p[j + 3] = t.w;
            }
        }
        bool outside = false;
        if constexpr (INDEXED) {
#pragma unroll
            for (uint32_t j = 0; j < per; ++j) outside |= p[j] == kPosGlobal;
        }
        uint4 q;
        uint8_t* b = reinterpret_cast<uint8_t*>(&q);
        if (!outside) {
#pragma unroll
            for (uint32_t j = 0; j < per; ++j) {
                const bool in = p[j] < kPosGlobal;
                const uint64_t g = lds_get<S>(img, in ? p[j] + off : 0);
                const uint64_t v = in ? g : 0;
                __builtin_memcpy(b + j * S, &v, S);
            }
        } else {
#pragma unroll
            for (uint32_t j = 0; j < per; ++j) {
                const uint64_t v = reply_elem<S, INDEXED>(img, pos, lo, buf, off, e0 + j);
                __builtin_memcpy(b + j * S, &v, S);
            }
        }
        __builtin_nontemporal_store(r_u32x4{q.x, q.y, q.z, q.w}, reinterpret_cast<r_u32x4*>(dstc) + c);
    } else {  // the column's last, partial chunk: whole elements, bytewise
        for (uint32_t e = e0; e < nr; ++e) {
            const uint64_t v = reply_elem<S, INDEXED>(img, pos, lo, buf, off, e);
#pragma unroll
            for (int k = 0; k < S; ++k) dstc[e * S + k] = static_cast<uint8_t>(v >> (8 * k));
        }
    }
}

template <bool INDEXED>
__global__ __launch_bounds__(kBlock) void k_unpack_replies(ReplyArgs a, const uint8_t* __restrict__ buf, uint64_t buf_len,
                                                           const uint32_t* __restrict__ offs, uint64_t n,
                                                           uint8_t* __restrict__ codes, srpc_unpack_status* st) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const uint32_t cap = a.R * a.F + 16;  // image bytes a tile may stage (a multiple of 16)
    const uint32_t p8 = (a.prefix_len + 7) & ~7u;
    uint8_t* img = lds;
    uint8_t* tmpl = lds + cap + 16;
    uint8_t* mask = tmpl + p8;
    uint32_t* pos = reinterpret_cast<uint32_t*>(mask + p8);
    uint32_t* lo = pos + a.R;  // indexed mode: the tile's offsets, lo[nr] = its end
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * a.R;
    const uint32_t nr = static_cast<uint32_t>(min<uint64_t>(a.R, n - base));

    // the plan's prefix without its code byte, as template | mask
    for (uint32_t i = threadIdx.x; i < p8; i += kBlock) {
        const bool keep = i < a.prefix_len && i != 4;
        tmpl[i] = keep ? a.prefix[i] : 0;
        mask[i] = keep ? 0xff : 0;
    }
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

    // 3. image -> columns
    for (uint32_t f = 0; f < a.nfields; ++f) {
        const uint32_t s = a.size[f];
        uint8_t* dstc = a.col[f] + base * s;
        const uint32_t nchunks = (nr * s + 15) >> 4;
        for (uint32_t c = threadIdx.x; c < nchunks; c += kBlock) {
            switch (s) {
            case 1: reply_chunk<1, INDEXED>(img, pos, lo, buf, a.off[f], c, nr, dstc); break;
            case 2: reply_chunk<2, INDEXED>(img, pos, lo, buf, a.off[f], c, nr, dstc); break;
            case 4: reply_chunk<4, INDEXED>(img, pos, lo, buf, a.off[f], c, nr, dstc); break;
            default: reply_chunk<8, INDEXED>(img, pos, lo, buf, a.off[f], c, nr, dstc); break;
            }
        }
    }
}

__global__ void k_reset_status(srpc_unpack_status* st) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        st->flags = 0;
        st->reserved = 0;
        st->first_bad_record = ~0ull;
    }
}

}  // namespace
}  // namespace srpc_impl

using namespace srpc_impl;

extern "C" {

int srpc_frames_scratch_bytes(uint64_t nframes, int nplans, uint64_t* out) {
    if (!out || nplans <= 0 || nplans > kMaxPlans) return SRPC_E_INVALID;
    *out = 4 * nframes + 8 * xscan_parts(nframes) + 256;
    return SRPC_OK;
}

int srpc_frames_classify(const srpc_plan* const* req_plans, const uint32_t* resp_bytes, int nplans,
                         const uint8_t* d_buf, uint64_t buf_len, const uint32_t* d_offs, uint64_t nframes,
                         uint8_t* d_class, uint32_t* d_index, uint64_t* d_counts, uint64_t* d_out_off,
                         void* d_scratch, uint64_t scratch_bytes, void* stream) {
    if (!req_plans || !resp_bytes || nplans <= 0 || nplans > kMaxPlans || !d_counts || !d_out_off) return SRPC_E_INVALID;
    uint64_t need = 0;
    srpc_frames_scratch_bytes(nframes, nplans, &need);
    if (!d_scratch || scratch_bytes < need || !aligned(d_scratch, 8)) return SRPC_E_CAPACITY;
    if (nframes && (!d_buf || !d_offs || !d_class || !d_index)) return SRPC_E_INVALID;
    if (nframes > 0xffffffffull) return SRPC_E_UNSUPPORTED;
    ClassArgs a{};
    if (int rc = class_args(req_plans, resp_bytes, nplans, &a)) return rc;
    auto s = static_cast<hipStream_t>(stream);
    auto* rb = static_cast<uint32_t*>(d_scratch);
    auto* part = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(d_scratch) + ((4 * nframes + 7) & ~7ull));
    hipLaunchKernelGGL(k_zero_counts, dim3(1), dim3(64), 0, s, d_counts, static_cast<uint32_t>(nplans + 2));
    if (nframes) {
        hipLaunchKernelGGL(k_classify, dim3(grid_for(nframes, kBlock)), dim3(kBlock), 0, s, a, d_buf, buf_len, d_offs,
                           nframes, d_class, d_index, d_counts, rb);
    }
    xscan(static_cast<const uint32_t*>(rb), nframes, part, d_counts + nplans, d_out_off, s);
    return hipGetLastError() == hipSuccess ? SRPC_OK : SRPC_E_HIP;
}

int srpc_frames_gather(const uint8_t* d_buf, const uint32_t* d_offs, const uint32_t* d_index, uint64_t n,
                       uint32_t record_bytes, uint8_t* d_out, void* stream) {
    if (!n) return SRPC_OK;
    if (!d_buf || !d_offs || !d_index || !d_out || !record_bytes) return SRPC_E_INVALID;
    hipLaunchKernelGGL(k_gather, dim3(grid_for(n * record_bytes, kBlock * 4)), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), d_buf, d_offs, d_index, n, record_bytes, d_out);
    return hipGetLastError() == hipSuccess ? SRPC_OK : SRPC_E_HIP;
}

int srpc_frames_scatter(const uint8_t* d_resp, const uint32_t* d_index, uint64_t n, uint32_t record_bytes,
                        const uint64_t* d_out_off, uint8_t* d_out, void* stream) {
    if (!n) return SRPC_OK;
    if (!d_resp || !d_index || !d_out_off || !d_out || !record_bytes) return SRPC_E_INVALID;
    hipLaunchKernelGGL(k_scatter, dim3(grid_for(n * record_bytes, kBlock)), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), d_resp, d_index, n, record_bytes, d_out_off, d_out);
    return hipGetLastError() == hipSuccess ? SRPC_OK : SRPC_E_HIP;
}

int srpc_frames_gather_var(const uint8_t* d_buf, const uint32_t* d_offs, const uint32_t* d_index, uint64_t n,
                           uint8_t* d_out, uint64_t* d_rec_offs, void* d_scratch, uint64_t scratch_bytes,
                           void* stream) {
    if (!d_rec_offs || (n && (!d_buf || !d_offs || !d_index || !d_out))) return SRPC_E_INVALID;
    uint64_t need = 0;
    srpc_frames_scratch_bytes(n, 1, &need);
    if (!d_scratch || scratch_bytes < need || !aligned(d_scratch, 8)) return SRPC_E_CAPACITY;
    if (!aligned(d_rec_offs, 8)) return SRPC_E_ALIGN;
    auto s = static_cast<hipStream_t>(stream);
    auto* lens = static_cast<uint32_t*>(d_scratch);
    auto* part = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(d_scratch) + ((4 * n + 7) & ~7ull));
    if (n) hipLaunchKernelGGL(k_payload_lens, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, s, d_buf, d_offs, d_index, n, lens);
    xscan(static_cast<const uint32_t*>(lens), n, part, part + xscan_parts(n), d_rec_offs, s);
    if (n)
        hipLaunchKernelGGL(k_gather_var, dim3(grid_for(n, kBlock / 64)), dim3(kBlock), 0, s, d_buf, d_offs, d_index, n,
                           static_cast<const uint64_t*>(d_rec_offs), d_out);
    return hipGetLastError() == hipSuccess ? SRPC_OK : SRPC_E_HIP;
}

int srpc_frames_scatter_var(const uint8_t* d_resp, const uint64_t* d_rec_offs, const uint32_t* d_index, uint64_t n,
                            const uint64_t* d_out_off, uint8_t* d_out, void* stream) {
    if (!n) return SRPC_OK;
    if (!d_resp || !d_rec_offs || !d_index || !d_out_off || !d_out) return SRPC_E_INVALID;
    hipLaunchKernelGGL(k_scatter_var, dim3(grid_for(n, kBlock / 64)), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                       d_resp, d_rec_offs, d_index, n, d_out_off, d_out);
    return hipGetLastError() == hipSuccess ? SRPC_OK : SRPC_E_HIP;
}

int srpc_frames_offsets(const srpc_plan* const* req_plans, const uint32_t* resp_bytes, int nplans,
                        const uint8_t* d_class, uint64_t nframes, const uint32_t* d_index, const uint64_t* d_counts,
                        const uint64_t* const* d_var_rec_offs, uint64_t* d_out_off, uint64_t* d_total,
                        void* d_scratch, uint64_t scratch_bytes, void* stream) {
    if (!req_plans || !resp_bytes || nplans <= 0 || nplans > kMaxPlans || !d_counts || !d_out_off || !d_total ||
        !d_var_rec_offs)
        return SRPC_E_INVALID;
    uint64_t need = 0;
    srpc_frames_scratch_bytes(nframes, nplans, &need);
    if (!d_scratch || scratch_bytes < need || !aligned(d_scratch, 8)) return SRPC_E_CAPACITY;
    if (nframes && (!d_class || !d_index)) return SRPC_E_INVALID;
    if (nframes > 0xffffffffull) return SRPC_E_UNSUPPORTED;
    ClassArgs a{};
    if (int rc = class_args(req_plans, resp_bytes, nplans, &a)) return rc;
    VarOffs v{};
    for (int k = 0; k < nplans; ++k) {
        if (a.nstr[k] && !d_var_rec_offs[k]) return SRPC_E_INVALID;
        v.rec[k] = a.nstr[k] ? d_var_rec_offs[k] : nullptr;
    }
    auto s = static_cast<hipStream_t>(stream);
    auto* sizes = static_cast<uint32_t*>(d_scratch);
    auto* part = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(d_scratch) + ((4 * nframes + 7) & ~7ull));
    if (nframes) {
        hipLaunchKernelGGL(k_fixed_sizes, dim3(grid_for(nframes, kBlock)), dim3(kBlock), 0, s, d_class, nframes, a, sizes);
        hipLaunchKernelGGL(k_var_sizes, dim3(std::min<uint32_t>(grid_for(nframes, kBlock), 1024), nplans), dim3(kBlock), 0,
                           s, d_index, nframes, d_counts, v, sizes);
    }
    xscan(static_cast<const uint32_t*>(sizes), nframes, part, d_total, d_out_off, s);
    return hipGetLastError() == hipSuccess ? SRPC_OK : SRPC_E_HIP;
}

int srpc_frames_replies_per_tile(const srpc_plan* reply_plan, uint32_t* out) {
    if (!reply_plan || !out) return SRPC_E_INVALID;
    if (reply_plan->has_string || reply_plan->prefix_len < 5) return SRPC_E_UNSUPPORTED;
    *out = reply_tile_frames(static_cast<uint32_t>(reply_plan->stride));
    return SRPC_OK;
}

int srpc_frames_unpack_replies(const srpc_plan* reply_plan, const uint8_t* d_buf, uint64_t buf_len,
                               const uint32_t* d_offs, uint64_t nframes, void* const* d_cols, uint8_t* d_codes,
                               srpc_unpack_status* d_status, void* stream) {
    const TimedCall timed;
    // the outputs and the length are checked before the plan is looked at
    if (!reply_plan || !d_cols || !d_codes || buf_len >= (1ull << 32)) return SRPC_E_INVALID;
    const srpc_plan* p = reply_plan;
    if (p->has_string || p->prefix_len < 5) return SRPC_E_UNSUPPORTED;
    if (nframes > 0xffffffffull) return SRPC_E_UNSUPPORTED;
    if (nframes && !d_buf) return SRPC_E_INVALID;
    if (!aligned(d_buf, 16)) return SRPC_E_ALIGN;
    for (uint32_t f = 0; nframes && f < p->nfields; ++f) {
        if (!d_cols[f]) return SRPC_E_INVALID;
        if (!aligned(d_cols[f], 16)) return SRPC_E_ALIGN;
    }
    auto s = static_cast<hipStream_t>(stream);
    if (d_status) {
        hipLaunchKernelGGL(k_reset_status, dim3(1), dim3(64), 0, s, d_status);
        if (hipGetLastError() != hipSuccess) return SRPC_E_HIP;
    }
    if (!nframes) return SRPC_OK;
    ReplyArgs a{};
    for (uint32_t f = 0; f < p->nfields; ++f) {
        a.col[f] = static_cast<uint8_t*>(d_cols[f]);
        a.size[f] = p->size[f];
        a.off[f] = p->off[f];
    }
    a.prefix = p->d_prefix;
    a.nfields = p->nfields;
    a.F = static_cast<uint32_t>(p->stride);
    a.prefix_len = p->prefix_len;
    a.R = reply_tile_frames(a.F);
    const uint32_t grid = static_cast<uint32_t>((nframes + a.R - 1) / a.R);
    const size_t lds = reply_lds_bytes(a.F, a.prefix_len, a.R, d_offs != nullptr);
    if (d_offs) launch(k_unpack_replies<true>, dim3(grid), dim3(kBlock), lds, s, a, d_buf, buf_len, d_offs, nframes, d_codes, d_status);
    else launch(k_unpack_replies<false>, dim3(grid), dim3(kBlock), lds, s, a, d_buf, buf_len, d_offs, nframes, d_codes, d_status);
    if (hipGetLastError() != hipSuccess) return SRPC_E_HIP;
    // uniform mode, a stream shorter than nframes full frames: as srpc_gpu_unpack
    return !d_offs && buf_len / a.F < nframes ? SRPC_ERR_BOUNDS : SRPC_OK;
}

}  // extern "C"
