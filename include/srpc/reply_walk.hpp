// srpc/reply_walk.hpp -- one reply frame of a string response against the
// per-frame table of srpc_frames_unpack_replies_var (include/srpc_gpu.h), on
// the host, and the one rule by which srpc::gpu::batch_client counts a chunk's
// replies (tally_replies): every form of call recounts a chunk the device
// decode flagged with a per-frame judge (gpu_client.hpp); the kernels apply the
// same tables.  Host code only, no dependencies, so it can be tested (and
// sanitized) on its own, like frame_walk.hpp.
#pragma once

#include <algorithm>
#include <cstdint>

namespace srpc::gpu {

enum class reply_kind : uint8_t {
    full,          // prefix and walk fit the frame exactly: fields decoded
    bare,          // a payload of one nonzero byte: an answer without a body
    bad_bounds,    // no header, BE32 != len - 4, no payload, or the walk leaves the frame
    bad_prefix,    // a payload that is none of the above
};

struct reply_frame {
    reply_kind kind = reply_kind::bad_bounds;
    uint8_t code = 0xFF;  // SRPC_REPLY_NO_CODE where the frame has none
};

/// Frame bytes f[0, len) (BE32 first).  prefix: the unframed response prefix
/// `u8 code | str(Resp::name)` (its code byte is ignored); sizes[k]: bytes of
/// leaf field k in declaration order, 0 for a string (u64 length + chars).
/// No byte at or past f + len is read; lengths are compared as `n > end - c`,
/// so a string length of 2^63 or 2^64 - 1 cannot wrap.
inline reply_frame walk_reply_var(const uint8_t* f, uint64_t len, const uint8_t* prefix, uint64_t prefix_len,
                                  const uint8_t* sizes, uint32_t nfields) {
    reply_frame r;
    if (len < 5) return r;
    const uint64_t be = (static_cast<uint64_t>(f[0]) << 24) | (static_cast<uint64_t>(f[1]) << 16) |
                        (static_cast<uint64_t>(f[2]) << 8) | static_cast<uint64_t>(f[3]);
    if (be != len - 4) return r;
    r.code = f[4];
    if (len == 5 && r.code != 0) {
        r.kind = reply_kind::bare;
        return r;
    }
    r.kind = reply_kind::bad_prefix;
    if (prefix_len < 1 || len - 4 < prefix_len) return r;
    for (uint64_t b = 1; b < prefix_len; ++b)
        if (f[4 + b] != prefix[b]) return r;
    r.kind = reply_kind::bad_bounds;
    uint64_t c = 4 + prefix_len;
    for (uint32_t k = 0; k < nfields; ++k) {
        if (sizes[k]) {
            if (sizes[k] > len - c) return r;
            c += sizes[k];
        } else {
            if (8 > len - c) return r;
            uint64_t sl = 0;
            for (int b = 0; b < 8; ++b) sl |= static_cast<uint64_t>(f[c + b]) << (8 * b);
            c += 8;
            if (sl > len - c) return r;
            c += sl;
        }
    }
    if (c == len) r.kind = reply_kind::full;
    return r;
}

/// Adds a chunk's nframes replies to st.ok / st.failed / st.malformed.  A
/// chunk the decode did not flag holds only full and bare frames, so codes[i]
/// (the decode's) tells: 0 (RPC_SUCCESS) is ok, anything else failed.  A flagged
/// chunk is judged frame by frame on the host: judge(i) is the table's verdict
/// on frame i, a frame neither full nor bare is malformed whatever its code.
template <class Stats, class Judge>
void tally_replies(const uint8_t* codes, uint64_t nframes, bool flagged, Judge&& judge, Stats& st) {
    if (!flagged) {
        const uint64_t ok = static_cast<uint64_t>(std::count(codes, codes + nframes, uint8_t{0}));
        st.ok += ok;
        st.failed += nframes - ok;
        return;
    }
    for (uint64_t i = 0; i < nframes; ++i) {
        const reply_frame r = judge(i);
        if (r.kind != reply_kind::full && r.kind != reply_kind::bare) st.malformed += 1;
        else if (r.code == 0) st.ok += 1;
        else st.failed += 1;
    }
}

}  // namespace srpc::gpu
