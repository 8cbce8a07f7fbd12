// scripted_peer.hpp -- TEST INFRASTRUCTURE ONLY.
//
// A peer for srpc::gpu::batch_client tests whose reply stream the test writes
// itself, hostile frames included: it waits for the first chunk's requests,
// answers the whole batch in one send (the later chunks' replies then lie in
// the client's receive buffer before those chunks are packed), and reads until
// the client goes.  The frames are the rows of the reply tables of
// include/srpc_gpu.h.
#pragma once

#include <srpc/gpu_server.hpp>  // be32
#include <srpc/packer.hpp>
#include <sys/socket.h>
#include <unistd.h>

#include <cstdint>
#include <cstdlib>
#include <thread>
#include <vector>

namespace scripted {

using bytes = std::vector<uint8_t>;

/// `BE32 | packer::pack_response` of `value` with `code`: a full frame.
template <class Resp>
bytes full(Resp const& value, srpc::rpc_status_code code = srpc::RPC_SUCCESS) {
    srpc::packer p;
    srpc::response_t<Resp> r;
    r.set_code(code);
    r.set_value(value);
    p.pack_response(r);
    bytes f = srpc::gpu::be32(static_cast<uint32_t>(p.size()));
    f.insert(f.end(), p.data(), p.data() + p.size());
    return f;
}
/// The answer of a server that does not know the method.
inline bytes bare(uint8_t code) { return {0, 0, 0, 1, code}; }
/// BE32 == 0: a frame without a payload (BOUNDS, no code).
inline bytes empty() { return {0, 0, 0, 0}; }
/// A full frame with the first letter of Resp::name changed (PREFIX): BE32 | code | u64 | name.
inline bytes wrong_name(bytes f) {
    f[13] ^= 0x20;
    return f;
}
/// A full frame whose last leaf is a string of last_chars chars, its u64
/// length raised past the frame's end (BOUNDS; the frame keeps its length).
inline bytes string_overrun(bytes f, uint64_t last_chars) {
    f[f.size() - last_chars - 8 + 1] += 4;  // + 1024
    return f;
}

/// Reads `after` whole request frames from fd, sends `replies` in one send,
/// then reads until the client closes.  Owns fd.
inline std::thread answer_at_once(int fd, uint64_t after, bytes replies) {
    return std::thread([fd, after, replies = std::move(replies)] {
        bytes in;
        uint8_t tmp[4096];
        uint64_t seen = 0, at = 0;
        bool answered = false;
        while (true) {
            const ssize_t k = recv(fd, tmp, sizeof tmp, 0);
            if (k <= 0) break;
            if (answered) continue;
            in.insert(in.end(), tmp, tmp + k);
            while (in.size() - at >= 4) {
                const uint64_t len = 4 + ((uint64_t{in[at]} << 24) | (uint64_t{in[at + 1]} << 16) |
                                          (uint64_t{in[at + 2]} << 8) | uint64_t{in[at + 3]});
                if (in.size() - at < len) break;
                at += len;
                ++seen;
            }
            if (seen >= after) {
                // a blocking send of a few KiB: whole, or the test's byte counts tell
                (void)send(fd, replies.data(), replies.size(), MSG_NOSIGNAL);
                answered = true;
            }
        }
        close(fd);
    });
}

}  // namespace scripted
