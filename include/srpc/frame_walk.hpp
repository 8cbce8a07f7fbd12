// srpc/frame_walk.hpp -- frame boundaries of a received byte stream.
//
// transport.hpp frames every message as `BE32 length | payload` (send_data /
// recv_data).  A batched peer reads whatever the socket holds and walks those
// lengths; this is the only per-frame CPU work of srpc::gpu::batch_client
// (gpu_client.hpp), and the walk batch_server::serve_connection does.  Host
// code only, no dependencies, so it can be tested (and sanitized) on its own.
#pragma once

#include <cstdint>

namespace srpc::gpu {

struct frame_walk {
    uint64_t nframes = 0;   // whole frames found: offs[0..nframes)
    uint64_t walked = 0;    // bytes they cover, from the buffer's start
    bool all_full = true;   // every one of them is full_bytes long
    uint64_t next_len = 0;  // bytes of the frame cut at `walked` (4 + its BE32), 0 while its header is cut too
};

/// Walk the whole frames in buf[0, have), at most max_frames of them in all,
/// continuing from `w` (a default frame_walk starts at byte 0; `have` only
/// grows between calls on the same buffer).  offs[i] receives the byte offset
/// of frame i.  Offsets are 32-bit, as srpc_frames_unpack_replies takes them:
/// the walk stops before a frame that would end past 4 GiB - 1 (next_len
/// tells).  No byte at or past buf + have is read.
inline frame_walk walk_frames(const uint8_t* buf, uint64_t have, uint64_t max_frames, uint32_t* offs,
                              uint64_t full_bytes, frame_walk w = {}) {
    w.next_len = 0;
    while (w.nframes < max_frames && have - w.walked >= 4) {
        const uint8_t* b = buf + w.walked;
        const uint64_t len = 4 + ((static_cast<uint64_t>(b[0]) << 24) | (static_cast<uint64_t>(b[1]) << 16) |
                                  (static_cast<uint64_t>(b[2]) << 8) | static_cast<uint64_t>(b[3]));
        if (have - w.walked < len || w.walked + len > 0xffffffffull) {
            w.next_len = len;
            break;
        }
        offs[w.nframes++] = static_cast<uint32_t>(w.walked);
        w.walked += len;
        w.all_full = w.all_full && len == full_bytes;
    }
    return w;
}

}  // namespace srpc::gpu
