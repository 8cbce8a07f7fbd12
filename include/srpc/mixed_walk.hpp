// srpc/mixed_walk.hpp -- the host form of a mixed batch's ranks and of the
// per-frame judgement of srpc_frames_unpack_replies_mixed and
// srpc_frames_unpack_replies_mixed_var (include/srpc_gpu.h).
// srpc::gpu::batch_client uses judge_reply_fixed (call, call_var) and
// judge_reply_mixed (both forms of call_mixed) as the per-frame judges of
// tally_replies when the device decode flagged a chunk (gpu_client.hpp); the
// kernels apply the same rules.  Host code only, no dependencies, so it can be
// tested (and sanitized) on its own, like frame_walk.hpp and reply_walk.hpp
// (whose reply_kind / reply_frame it shares).
#pragma once

#include <cstdint>

#include "reply_walk.hpp"

namespace srpc::gpu {

constexpr uint32_t mixed_no_rank = 0xffffffffu;

/// rank[i] = the number of calls j < i with method[j] == method[i], or
/// mixed_no_rank for an id >= nplans (nplans <= 256: ids are bytes).
/// counts[k] (nplans + 1 entries) = calls of plan k, counts[nplans] = calls
/// with an id out of range.  Returns the smallest call with such an id, or
/// UINT64_MAX.
inline uint64_t mixed_ranks(const uint8_t* method, uint64_t n, uint32_t nplans, uint32_t* rank, uint64_t* counts) {
    for (uint32_t k = 0; k <= nplans; ++k) counts[k] = 0;
    uint64_t first_bad = ~0ull;
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t k = method[i];
        if (k >= nplans) {
            rank[i] = mixed_no_rank;
            counts[nplans] += 1;
            if (first_bad == ~0ull) first_bad = i;
        } else {
            rank[i] = static_cast<uint32_t>(counts[k]++);
        }
    }
    return first_bad;
}

/// One frame of a fixed-size reply plan against the table of
/// srpc_frames_unpack_replies: bytes [o, e) of a stream of buf_len bytes
/// (offsets as the decode takes them: out of order or past the end is
/// bad_bounds).  prefix: the plan's framed response prefix `BE32(payload) | u8
/// code | str(Resp::name)` (its code byte is ignored), prefix_len >= 5; F: the
/// plan's frame bytes.  No byte outside [buf + o, buf + e) is read.
inline reply_frame judge_reply_fixed(const uint8_t* buf, uint64_t buf_len, uint64_t o, uint64_t e, uint64_t F,
                                     const uint8_t* prefix, uint64_t prefix_len) {
    reply_frame r;
    if (!(o <= e && e <= buf_len) || e - o < 5) return r;
    const uint8_t* f = buf + o;
    const uint64_t len = e - o;
    const uint64_t be = (static_cast<uint64_t>(f[0]) << 24) | (static_cast<uint64_t>(f[1]) << 16) |
                        (static_cast<uint64_t>(f[2]) << 8) | static_cast<uint64_t>(f[3]);
    if (be != len - 4) return r;
    r.code = f[4];
    if (len == F && prefix_len >= 5 && prefix_len <= F) {
        bool eq = true;
        for (uint64_t b = 0; b < prefix_len && eq; ++b) eq = b == 4 || f[b] == prefix[b];
        r.kind = eq ? reply_kind::full : reply_kind::bad_prefix;
    } else {
        r.kind = len == 5 && r.code != 0 ? reply_kind::bare : reply_kind::bad_prefix;
    }
    return r;
}

/// The plans of a mixed reply stream, as the decode sees them.
struct mixed_reply_plan {
    const uint8_t* prefix = nullptr;
    uint64_t prefix_len = 0;
    uint64_t F = 0;       // frame bytes
    uint64_t first = 0;   // h_first[k]
    uint64_t cap = 0;     // h_cap[k]
    // a string plan: prefix is the unframed `u8 code |
    // str(Resp::name)`, F is unused, leaf[f] the bytes of leaf f (0: a string)
    bool var = false;
    const uint8_t* leaf = nullptr;
    uint32_t nleaves = 0;
};

/// Frame i of a chunk against the table of srpc_frames_unpack_replies_mixed or
/// _mixed_var: a bad call (id out of range, or no element left in its plan's
/// columns) is the first row whatever its bytes; a frame of a string plan is
/// judged by walk_reply_var, one of a fixed plan by judge_reply_fixed.  rank:
/// from mixed_ranks; end: offs[i + 1], or buf_len for the last frame.  Offsets
/// out of order or past the end are bad_bounds under either; no byte outside
/// [buf + o, buf + end) is read.
inline reply_frame judge_reply_mixed(const uint8_t* buf, uint64_t buf_len, uint64_t o, uint64_t end, uint32_t method,
                                     uint32_t rank, const mixed_reply_plan* plans, uint32_t nplans) {
    if (method >= nplans || rank == mixed_no_rank) return reply_frame{};
    const mixed_reply_plan& p = plans[method];
    if (p.first >= p.cap || rank >= p.cap - p.first) return reply_frame{};
    if (!p.var) return judge_reply_fixed(buf, buf_len, o, end, p.F, p.prefix, p.prefix_len);
    if (!(o <= end && end <= buf_len)) return reply_frame{};
    return walk_reply_var(buf + o, end - o, p.prefix, p.prefix_len, p.leaf, p.nleaves);
}

}  // namespace srpc::gpu
