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
// Replies with string fields take a parse pass, a scan per string field and a
// copy pass (srpc_frames_unpack_replies_var); string request records are framed
// for the socket by k_frame_var (srpc_frames_frame_var).
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

// ---------------------------------------------------------------------------
// Client side, string replies (srpc_frames_unpack_replies_var): frames of
// varying length -> one code per call, the fixed columns and the string
// columns, in call order.  Three steps, none of which waits on another
// workgroup:
//
//   k_replies_var_parse  a workgroup stages the contiguous span of its R frames
//       into an LDS image (16-byte loads from a 16-byte boundary) and one lane
//       per frame applies the table of srpc_gpu.h: it walks the frame's fields
//       once and writes as it goes (a walk that fails is overwritten with
//       zeros), so nothing per string is kept in registers.  Lane j writes
//       element base + j of the codes and of every
//       fixed column (coalesced), and each string's length and the stream
//       offset of its chars into scratch (0 / 0 unless the frame is full).
//   xscan                one exclusive scan of the lengths per string field,
//       straight into d_str_offs[f][0..n].
//   k_replies_var_copy   the same tiles again: tile t owns bytes [offs[base],
//       offs[base + nr]) of every string column and writes them as 16-byte
//       chunks on the column's own 16-byte grid (the ends bytewise, so tiles
//       never write the same byte).  A lane finds the frame of its chunk's
//       first byte by bisection in the tile's offsets (LDS) and assembles the
//       chunk from runs of the image, eight bytes per LDS read.
//
// A frame that does not lie whole inside the image (longer than the image, or
// pushed out by a long frame before it) is parsed by its lane from global
// memory -- at most the plan's fixed bytes, never the chars -- and its chars are
// copied from global memory by the same output-centric loop: every lane of the
// workgroup takes 16 bytes of the tile's output at a time, so a long string is
// moved by 256 lanes and no lane's work depends on one string's length.
// LDS: parse  image[cap + 16] | tmpl[P8] | mask[P8] | lo[R + 1]
//      copy   image[cap + 16] | lo[R + 1] | rel[R + 1] | src[R]
// ---------------------------------------------------------------------------
// 128 frames and a 16 KiB image (128 bytes per frame) keep a workgroup under
// 20 KiB of LDS: 8 workgroups, 32 waves, per CU.  Both passes are chains of
// dependent latencies (stage, barrier, parse or bisect), so resident
// workgroups are what hides them.
constexpr uint32_t kVarReplyFrames = 128;        // frames per tile: one lane each (<= kBlock)
constexpr uint32_t kVarReplyImage = 16384;       // image bytes per tile

struct ReplyVarArgs {
    uint8_t* col[kMaxFields];
    const uint64_t* soffs[kMaxFields];  // string field: its offsets (the scan's output), else NULL
    uint8_t size[kMaxFields];           // 0: a string
    const uint8_t* prefix;              // `u8 code | str(Resp::name)`, the code byte ignored
    uint32_t nfields;
    uint32_t nstr;
    uint32_t prefix_len;
};

inline size_t reply_var_parse_lds(uint32_t prefix_len) {
    return kVarReplyImage + 16 + 2 * ((prefix_len + 7) & ~7u) + 4 * (kVarReplyFrames + 1);
}
inline size_t reply_var_copy_lds() { return kVarReplyImage + 16 + 4 * (3 * kVarReplyFrames + 2); }

// The tile's frame offsets into lo[0..nr] (lo[nr] = the tile's end) and its span
// into the image: *s0 is the stream offset of image byte 0 (a multiple of 16),
// the return value the bytes staged.  Ends with a barrier.
__device__ __forceinline__ uint32_t reply_var_stage(uint8_t* img, uint32_t* lo, const uint8_t* __restrict__ buf,
                                                    uint64_t buf_len, const uint32_t* __restrict__ offs, uint64_t n,
                                                    uint64_t base, uint32_t nr, uint64_t* s0) {
    for (uint32_t j = threadIdx.x; j <= nr; j += kBlock)
        lo[j] = base + j < n ? offs[base + j] : static_cast<uint32_t>(buf_len);
    __syncthreads();
    const uint64_t o0 = lo[0], oe = lo[nr];
    *s0 = o0 & ~15ull;
    uint32_t staged = 0;
    if (o0 <= buf_len) {
        const uint64_t end = oe >= o0 && oe <= buf_len ? oe : buf_len;
        staged = static_cast<uint32_t>(min<uint64_t>(end - *s0, kVarReplyImage));
    }
    const uint8_t* src = buf + *s0;
    const uint32_t full = staged >> 4;
    for (uint32_t c0 = threadIdx.x; c0 < full; c0 += kBlock * kReplyLoads) {
        uint4 vv[kReplyLoads];
#pragma unroll
        for (int u = 0; u < kReplyLoads; ++u) {
            const uint32_t c = min(c0 + u * kBlock, full - 1);  // past the end: the last chunk again
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
    return staged;
}

// k <= 8 bytes at stream offset `at`: from the image (IMG: `at` is an image
// offset) or bytewise from global memory.
template <bool IMG>
__device__ __forceinline__ uint64_t reply_var_get(const uint8_t* img, const uint8_t* __restrict__ buf, uint64_t at,
                                                  uint32_t k) {
    if constexpr (IMG) {
        const uint32_t a = static_cast<uint32_t>(at);
        switch (k) {
        case 1: return lds_get<1>(img, a);
        case 2: return lds_get<2>(img, a);
        case 4: return lds_get<4>(img, a);
        default: return lds_get<8>(img, a);
        }
    } else {
        uint64_t v = 0;
        for (uint32_t b = 0; b < k; ++b) v |= static_cast<uint64_t>(buf[at + b]) << (8 * b);
        return v;
    }
}

__device__ __forceinline__ void reply_var_store(uint8_t* col, uint64_t i, uint32_t size, uint64_t v) {
    switch (size) {
    case 1: col[i] = static_cast<uint8_t>(v); break;
    case 2: reinterpret_cast<uint16_t*>(col)[i] = static_cast<uint16_t>(v); break;
    case 4: reinterpret_cast<uint32_t*>(col)[i] = static_cast<uint32_t>(v); break;
    default: reinterpret_cast<uint64_t*>(col)[i] = v; break;
    }
}

// The frame's fields from `c` (just past the prefix) to `e`: does the walk end
// exactly at e, every string inside the frame?  On the way it writes element i
// of the fixed columns, string t's length to lens[t * n + i] and the stream
// offset of its chars to srcs[t * n + i]; when it returns false the caller
// overwrites them.  IMG: c and e are image offsets and `shift` = the image's
// stream offset.
template <bool IMG>
__device__ __forceinline__ bool reply_var_walk(const ReplyVarArgs& a, const uint8_t* img,
                                               const uint8_t* __restrict__ buf, uint64_t c, uint64_t e,
                                               uint64_t shift, uint64_t i, uint64_t n, uint32_t* __restrict__ lens,
                                               uint32_t* __restrict__ srcs) {
    uint32_t t = 0;
    for (uint32_t f = 0; f < a.nfields; ++f) {
        const uint32_t s = a.size[f];
        if (s) {
            if (s > e - c) return false;
            reply_var_store(a.col[f], i, s, reply_var_get<IMG>(img, buf, c, s));
            c += s;
        } else {
            if (8 > e - c) return false;
            const uint64_t sl = reply_var_get<IMG>(img, buf, c, 8);
            c += 8;
            if (sl > e - c) return false;  // as k_classify: a length of 2^63 or 2^64 - 1 cannot wrap
            lens[t * n + i] = static_cast<uint32_t>(sl);
            srcs[t * n + i] = static_cast<uint32_t>(c + shift);
            c += sl;
            ++t;
        }
    }
    return c == e;
}

__global__ __launch_bounds__(kBlock) void k_replies_var_parse(ReplyVarArgs a, const uint8_t* __restrict__ buf,
                                                              uint64_t buf_len, const uint32_t* __restrict__ offs,
                                                              uint64_t n, uint8_t* __restrict__ codes,
                                                              uint32_t* __restrict__ lens, uint32_t* __restrict__ srcs,
                                                              srpc_unpack_status* st) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const uint32_t p8 = (a.prefix_len + 7) & ~7u;
    uint8_t* img = lds;
    uint8_t* tmpl = lds + kVarReplyImage + 16;
    uint8_t* mask = tmpl + p8;
    uint32_t* lo = reinterpret_cast<uint32_t*>(mask + p8);
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kVarReplyFrames;
    const uint32_t nr = static_cast<uint32_t>(min<uint64_t>(kVarReplyFrames, n - base));
    // the plan's prefix without its code byte, as template | mask
    for (uint32_t i = threadIdx.x; i < p8; i += kBlock) {
        const bool keep = i < a.prefix_len && i != 0;
        tmpl[i] = keep ? a.prefix[i] : 0;
        mask[i] = keep ? 0xff : 0;
    }
    uint64_t s0;
    const uint32_t staged = reply_var_stage(img, lo, buf, buf_len, offs, n, base, nr, &s0);

    const uint32_t j = threadIdx.x;
    if (j >= nr) return;
    const uint64_t i = base + j;
    const uint64_t o = lo[j], e = lo[j + 1];
    uint32_t code = SRPC_REPLY_NO_CODE, flag = 0;
    bool full = false, in_img = false;
    if (!(o <= e && e <= buf_len) || e - o < 5) {
        flag = SRPC_STATUS_BOUNDS;  // out of order, past the end, no header or no payload
    } else {
        const uint64_t len = e - o;
        in_img = o >= s0 && e - s0 <= staged;  // the whole frame is in the image
        const uint32_t q = static_cast<uint32_t>(o - s0);
        const uint8_t* h = in_img ? img + q : buf + o;
        const uint32_t be = be32_at(h), c0 = h[4];
        if (be != len - 4) {
            flag = SRPC_STATUS_BOUNDS;
        } else {
            code = c0;
            if (!(len == 5 && c0 != 0)) {  // not a bare error frame
                bool eq = len - 4 >= a.prefix_len;
                if (eq && in_img) {
                    for (uint32_t b = 0; b < p8; b += 8)
                        eq &= ((lds_u64(img, q + 4 + b) ^ *reinterpret_cast<const uint64_t*>(tmpl + b)) &
                               *reinterpret_cast<const uint64_t*>(mask + b)) == 0;
                } else if (eq) {
                    for (uint32_t b = 0; b < a.prefix_len; ++b) eq &= ((buf[o + 4 + b] ^ tmpl[b]) & mask[b]) == 0;
                }
                if (!eq) {
                    flag = SRPC_STATUS_PREFIX;
                } else {
                    // one walk that writes as it goes: element i of every output is
                    // this lane's alone, so a walk that fails is overwritten below
                    const uint64_t c = o + 4 + a.prefix_len;
                    full = in_img ? reply_var_walk<true>(a, img, buf, c - s0, e - s0, s0, i, n, lens, srcs)
                                  : reply_var_walk<false>(a, img, buf, c, e, 0, i, n, lens, srcs);
                    if (!full) flag = SRPC_STATUS_BOUNDS;
                }
            }
        }
    }
    codes[i] = static_cast<uint8_t>(code);
    if (!full) {
        uint32_t t = 0;
        for (uint32_t f = 0; f < a.nfields; ++f) {
            if (a.size[f]) {
                reply_var_store(a.col[f], i, a.size[f], 0);
            } else {
                lens[t * n + i] = 0;
                srcs[t * n + i] = 0;
                ++t;
            }
        }
    }
    if (flag && st) report_bad(st, flag, i);
}

// The k <= 8 low bytes of v into bytes [b, b + k) of the 16-byte chunk lo | hi.
__device__ __forceinline__ void chunk_put(uint64_t& lo, uint64_t& hi, uint32_t b, uint64_t v, uint32_t k) {
    if (k < 8) v &= (1ull << (8 * k)) - 1;
    if (b < 8) {
        lo |= v << (8 * b);
        if (b && b + k > 8) hi |= v >> (64 - 8 * b);
    } else {
        hi |= v << (8 * (b - 8));
    }
}

__global__ __launch_bounds__(kBlock) void k_replies_var_copy(ReplyVarArgs a, const uint8_t* __restrict__ buf,
                                                             uint64_t buf_len, const uint32_t* __restrict__ offs,
                                                             uint64_t n, const uint32_t* __restrict__ srcs) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    uint8_t* img = lds;
    uint32_t* lo = reinterpret_cast<uint32_t*>(lds + kVarReplyImage + 16);
    uint32_t* rel = lo + kVarReplyFrames + 1;  // rel[j]: chars of this field in the tile's frames before j
    uint32_t* src = rel + kVarReplyFrames + 1; // src[j]: stream offset of frame j's chars
    const uint64_t base = static_cast<uint64_t>(blockIdx.x) * kVarReplyFrames;
    const uint32_t nr = static_cast<uint32_t>(min<uint64_t>(kVarReplyFrames, n - base));
    // the first string field's offsets and sources are asked for before the
    // staging, so their latency overlaps it (lane j holds entry j: R < kBlock)
    static_assert(kVarReplyFrames < kBlock, "one lane per tile offset");
    uint32_t f0 = 0;
    while (a.size[f0]) ++f0;  // a string plan has a string field
    const uint64_t A0 = a.soffs[f0][base];
    uint64_t pre_so = 0;
    uint32_t pre_src = 0;
    if (threadIdx.x <= nr) pre_so = a.soffs[f0][base + threadIdx.x];
    if (threadIdx.x < nr) pre_src = srcs[base + threadIdx.x];
    uint64_t s0;
    const uint32_t staged = reply_var_stage(img, lo, buf, buf_len, offs, n, base, nr, &s0);

    uint32_t t = 0;
    for (uint32_t f = 0; f < a.nfields; ++f) {
        if (a.size[f]) continue;
        const uint64_t* so = a.soffs[f] + base;
        const uint64_t A = t ? so[0] : A0;  // the tile's first output byte in this column
        if (t) __syncthreads();             // the previous field's rel / src are no longer read
        // Ascending offsets keep a column's chars under buf_len.  Offsets out of
        // order can make full frames overlap and their chars total more: the
        // column has room for buf_len bytes, so what lies at or past buf_len is
        // not written (rel saturates there: still monotone, and no run is longer
        // than its string, so every source byte read is a char of its frame).
        const uint64_t room = A < buf_len ? buf_len - A : 0;
        if (const uint32_t j = threadIdx.x; j <= nr) {
            rel[j] = static_cast<uint32_t>(min<uint64_t>((t ? so[j] : pre_so) - A, room));
            if (j < nr) src[j] = t ? srcs[t * n + base + j] : pre_src;
        }
        __syncthreads();
        ++t;
        const uint64_t total = rel[nr];
        if (!total) continue;  // the same for every lane
        uint8_t* dst = a.col[f];
        const uint64_t x00 = A & ~15ull;
        const uint64_t nchunks = (A + total - x00 + 15) >> 4;
        for (uint64_t c = threadIdx.x; c < nchunks; c += kBlock) {
            const uint64_t x0 = x00 + 16 * c;
            const uint64_t xb = max(x0, A), xe = min(x0 + 16, A + total);
            const uint32_t r0 = static_cast<uint32_t>(xb - A), cnt = static_cast<uint32_t>(xe - xb);
            // the last j with rel[j] <= r0 (r0 < total = rel[nr], so j < nr); a count
            // of the offsets at or under r0 in two rounds of independent reads
            // (every 8th, then the 7 between) measured slower than these 7
            // dependent steps: the pass is bound by LDS instructions, not by latency
            uint32_t lo_j = 0, hi_j = nr;
            while (hi_j - lo_j > 1) {
                const uint32_t m = (lo_j + hi_j) >> 1;
                if (rel[m] <= r0) lo_j = m;
                else hi_j = m;
            }
            uint32_t j = lo_j;
            uint64_t vlo = 0, vhi = 0;
            uint32_t b = static_cast<uint32_t>(xb - x0);
            const uint32_t bend = b + cnt;
            uint32_t r = r0;
            while (b < bend) {
                while (rel[j + 1] <= r) ++j;  // empty strings; r < total keeps j < nr
                const uint32_t k = min(min(bend - b, rel[j + 1] - r), 8u);
                const uint64_t at = static_cast<uint64_t>(src[j]) + (r - rel[j]);
                uint64_t v;
                if (at >= s0 && at + k - s0 <= staged) v = lds_u64(img, static_cast<uint32_t>(at - s0));
                else v = reply_var_get<false>(img, buf, at, k);
                chunk_put(vlo, vhi, b, v, k);
                b += k;
                r += k;
            }
            if (cnt == 16) {
                __builtin_nontemporal_store(r_u32x4{static_cast<uint32_t>(vlo), static_cast<uint32_t>(vlo >> 32),
                                                    static_cast<uint32_t>(vhi), static_cast<uint32_t>(vhi >> 32)},
                                            reinterpret_cast<r_u32x4*>(dst + x0));
            } else {  // the tile's first or last, partial chunk: its own bytes only
                for (uint32_t y = static_cast<uint32_t>(xb - x0); y < bend; ++y)
                    dst[x0 + y] = static_cast<uint8_t>((y < 8 ? vlo >> (8 * y) : vhi >> (8 * (y - 8))));
            }
        }
    }
}

// A wave per record (grid-stride): BE32(len_j) | record j at out + rec_offs[j] + 4 j.
__global__ __launch_bounds__(kBlock) void k_frame_var(const uint8_t* __restrict__ rec, const uint64_t* __restrict__ rec_offs,
                                                      uint64_t n, uint8_t* __restrict__ out, uint64_t out_cap,
                                                      srpc_unpack_status* st) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = static_cast<uint64_t>(gridDim.x) * (kBlock / 64);
    for (uint64_t j = static_cast<uint64_t>(blockIdx.x) * (kBlock / 64) + threadIdx.x / 64; j < n; j += waves) {
        const uint64_t r = rec_offs[j], r1 = rec_offs[j + 1];
        const uint64_t len = r1 - r, at = r + 4 * j;
        if (r1 < r || len >= (1ull << 32) || at > out_cap || 4 + len > out_cap - at) {
            if (st && lane == 0) report_bad(st, SRPC_STATUS_BOUNDS, j);
            continue;
        }
        uint8_t* dst = out + at;
        if (lane < 4) dst[lane] = static_cast<uint8_t>(len >> (8 * (3 - lane)));
        for (uint64_t b = lane; b < len; b += 64) dst[4 + b] = rec[r + b];
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

int status_reset_launch(srpc_unpack_status* d_status, hipStream_t s) {
    hipLaunchKernelGGL(k_reset_status, dim3(1), dim3(64), 0, s, d_status);
    return hipGetLastError() == hipSuccess ? SRPC_OK : SRPC_E_HIP;
}

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
    if (d_status && status_reset_launch(d_status, s)) return SRPC_E_HIP;
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

// scratch of the string reply decode: lens[nstr][n] | srcs[nstr][n] (u32) | the scan's words
static int reply_var_plan_ok(const srpc_plan* p) {
    if (!p->has_string || p->prefix_len < 1 || p->nstrings > static_cast<uint32_t>(kMaxStr)) return SRPC_E_UNSUPPORTED;
    return SRPC_OK;
}

int srpc_frames_replies_var_scratch_bytes(const srpc_plan* reply_plan, uint64_t nframes, uint64_t* out) {
    if (!reply_plan || !out) return SRPC_E_INVALID;
    if (int rc = reply_var_plan_ok(reply_plan)) return rc;
    *out = 8 * static_cast<uint64_t>(reply_plan->nstrings) * nframes + 8 * (xscan_parts(nframes) + 1) + 256;
    return SRPC_OK;
}

int srpc_frames_replies_var_tile(const srpc_plan* reply_plan, uint32_t* frames, uint32_t* image_bytes) {
    if (!reply_plan || !frames || !image_bytes) return SRPC_E_INVALID;
    if (int rc = reply_var_plan_ok(reply_plan)) return rc;
    *frames = kVarReplyFrames;
    *image_bytes = kVarReplyImage;
    return SRPC_OK;
}

int srpc_frames_unpack_replies_var(const srpc_plan* reply_plan, const uint8_t* d_buf, uint64_t buf_len,
                                   const uint32_t* d_offs, uint64_t nframes, void* const* d_cols,
                                   uint64_t* const* d_str_offs, uint8_t* d_codes, srpc_unpack_status* d_status,
                                   void* d_scratch, uint64_t scratch_bytes, void* stream) {
    const TimedCall timed;
    // the pointers and the length are checked before the plan is looked at
    if (!reply_plan || !d_cols || !d_str_offs || !d_codes || !d_scratch || (nframes && !d_offs) ||
        buf_len >= (1ull << 32))
        return SRPC_E_INVALID;
    const srpc_plan* p = reply_plan;
    if (int rc = reply_var_plan_ok(p)) return rc;
    if (nframes > 0xffffffffull) return SRPC_E_UNSUPPORTED;
    if (nframes && !d_buf) return SRPC_E_INVALID;
    uint64_t need = 0;
    srpc_frames_replies_var_scratch_bytes(p, nframes, &need);
    if (scratch_bytes < need) return SRPC_E_CAPACITY;
    if (!aligned(d_buf, 16) || !aligned(d_scratch, 8)) return SRPC_E_ALIGN;
    ReplyVarArgs a{};
    for (uint32_t f = 0; f < p->nfields; ++f) {
        const bool str = p->kinds[f] == SRPC_KIND_STRING;
        if (str && !d_str_offs[f]) return SRPC_E_INVALID;
        if (str && !aligned(d_str_offs[f], 8)) return SRPC_E_ALIGN;
        if (nframes && !d_cols[f]) return SRPC_E_INVALID;
        if (!aligned(d_cols[f], 16)) return SRPC_E_ALIGN;
        a.col[f] = static_cast<uint8_t*>(d_cols[f]);
        a.soffs[f] = str ? d_str_offs[f] : nullptr;
        a.size[f] = static_cast<uint8_t>(str ? 0 : p->size[f]);
    }
    a.prefix = p->d_prefix;
    a.nfields = p->nfields;
    a.nstr = p->nstrings;
    a.prefix_len = p->prefix_len;
    auto s = static_cast<hipStream_t>(stream);
    if (d_status && status_reset_launch(d_status, s)) return SRPC_E_HIP;
    auto* lens = static_cast<uint32_t*>(d_scratch);
    auto* srcs = lens + a.nstr * nframes;
    auto* part = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(d_scratch) + 8 * a.nstr * nframes);
    const uint32_t grid = static_cast<uint32_t>((nframes + kVarReplyFrames - 1) / kVarReplyFrames);
    if (nframes)
        launch(k_replies_var_parse, dim3(grid), dim3(kBlock), reply_var_parse_lds(a.prefix_len), s, a, d_buf, buf_len,
               d_offs, nframes, d_codes, lens, srcs, d_status);
    uint32_t t = 0;
    for (uint32_t f = 0; f < p->nfields; ++f) {
        if (a.size[f]) continue;
        xscan(static_cast<const uint32_t*>(lens + t * nframes), nframes, part, part + xscan_parts(nframes), d_str_offs[f], s);
        ++t;
    }
    if (nframes)
        launch(k_replies_var_copy, dim3(grid), dim3(kBlock), reply_var_copy_lds(), s, a, d_buf, buf_len, d_offs, nframes,
               static_cast<const uint32_t*>(srcs));
    return hipGetLastError() == hipSuccess ? SRPC_OK : SRPC_E_HIP;
}

int srpc_frames_frame_var(const uint8_t* d_records, const uint64_t* d_rec_offs, uint64_t n, uint8_t* d_out,
                          uint64_t out_cap, srpc_unpack_status* d_status, void* stream) {
    if (!n) return SRPC_OK;
    if (!d_records || !d_rec_offs || !d_out) return SRPC_E_INVALID;
    hipLaunchKernelGGL(k_frame_var, dim3(grid_for(n, kBlock / 64)), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                       d_records, d_rec_offs, n, d_out, out_cap, d_status);
    return hipGetLastError() == hipSuccess ? SRPC_OK : SRPC_E_HIP;
}

}  // extern "C"
