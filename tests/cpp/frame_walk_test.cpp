// srpc::gpu::walk_frames (include/srpc/frame_walk.hpp): the host walk of a
// reply stream's BE32 frame lengths.  A stand-alone program, so it can be
// built with -fsanitize=address,undefined and simply run: every buffer is a
// heap allocation of exactly the bytes the walk may read.
#include <srpc/frame_walk.hpp>

#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

using srpc::gpu::frame_walk;
using srpc::gpu::walk_frames;

static int g_fail = 0, g_pass = 0;
#define CHECK(c)                                                                    \
    do {                                                                            \
        if (c) ++g_pass;                                                            \
        else { ++g_fail; std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); } \
    } while (0)

static void frame(std::vector<uint8_t>& out, uint32_t payload, uint32_t claimed) {
    out.push_back(static_cast<uint8_t>(claimed >> 24));
    out.push_back(static_cast<uint8_t>(claimed >> 16));
    out.push_back(static_cast<uint8_t>(claimed >> 8));
    out.push_back(static_cast<uint8_t>(claimed));
    for (uint32_t i = 0; i < payload; ++i) out.push_back(static_cast<uint8_t>(0x40 + i));
}
static void frame(std::vector<uint8_t>& out, uint32_t payload) { frame(out, payload, payload); }

// The walk over an exact-size heap copy of `bytes` (a read past it is an ASan error).
static frame_walk walk(std::vector<uint8_t> const& bytes, uint64_t max_frames, std::vector<uint32_t>& offs,
                       uint64_t full, frame_walk from = {}) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[bytes.size() ? bytes.size() : 1]);
    if (!bytes.empty()) std::memcpy(exact.get(), bytes.data(), bytes.size());
    offs.assign(max_frames ? max_frames : 1, 0xdeadbeef);
    std::unique_ptr<uint32_t[]> o(new uint32_t[max_frames ? max_frames : 1]);
    for (uint64_t i = 0; i < max_frames; ++i) o[i] = 0xdeadbeef;
    const frame_walk w = walk_frames(exact.get(), bytes.size(), max_frames, o.get(), full, from);
    for (uint64_t i = 0; i < max_frames; ++i) offs[i] = o[i];
    return w;
}

int main() {
    std::vector<uint32_t> offs;
    {  // whole frames, all full
        std::vector<uint8_t> b;
        for (int i = 0; i < 5; ++i) frame(b, 19);
        const frame_walk w = walk(b, 100, offs, 23);
        CHECK(w.nframes == 5 && w.walked == 115 && w.all_full && w.next_len == 0);
        for (uint32_t i = 0; i < 5; ++i) CHECK(offs[i] == 23 * i);
        CHECK(offs[5] == 0xdeadbeef);
    }
    {  // whole frames, one bare among them
        std::vector<uint8_t> b;
        frame(b, 19);
        frame(b, 1);
        frame(b, 19);
        const frame_walk w = walk(b, 100, offs, 23);
        CHECK(w.nframes == 3 && w.walked == 51 && !w.all_full);
        CHECK(offs[0] == 0 && offs[1] == 23 && offs[2] == 28);
    }
    {  // nothing at all
        const frame_walk w = walk({}, 4, offs, 23);
        CHECK(w.nframes == 0 && w.walked == 0 && w.all_full && w.next_len == 0);
    }
    for (size_t cut = 1; cut <= 3; ++cut) {  // a cut header after two frames
        std::vector<uint8_t> b;
        frame(b, 19);
        frame(b, 19);
        frame(b, 19);
        b.resize(46 + cut);
        const frame_walk w = walk(b, 100, offs, 23);
        CHECK(w.nframes == 2 && w.walked == 46 && w.all_full && w.next_len == 0);
    }
    for (size_t cut : {4u, 5u, 22u}) {  // a cut frame: header whole, payload short
        std::vector<uint8_t> b;
        frame(b, 19);
        frame(b, 19);
        b.resize(23 + cut);
        const frame_walk w = walk(b, 100, offs, 23);
        CHECK(w.nframes == 1 && w.walked == 23 && w.next_len == 23);
        // the rest arrives: the walk continues where it stopped
        std::vector<uint8_t> whole;
        frame(whole, 19);
        frame(whole, 19);
        std::vector<uint32_t> offs2;
        const frame_walk w2 = walk(whole, 100, offs2, 23, w);
        CHECK(w2.nframes == 2 && w2.walked == 46 && w2.all_full && w2.next_len == 0 && offs2[1] == 23);
    }
    {  // a zero-length payload is a frame of 4 bytes
        std::vector<uint8_t> b;
        frame(b, 0);
        frame(b, 19);
        frame(b, 0);
        const frame_walk w = walk(b, 100, offs, 23);
        CHECK(w.nframes == 3 && w.walked == 31 && !w.all_full);
        CHECK(offs[0] == 0 && offs[1] == 4 && offs[2] == 27);
    }
    {  // exactly max_frames: the walk stops there and reads no further header
        std::vector<uint8_t> b;
        for (int i = 0; i < 4; ++i) frame(b, 19);
        frame(b, 1);
        const frame_walk w = walk(b, 4, offs, 23);
        CHECK(w.nframes == 4 && w.walked == 92 && w.all_full && w.next_len == 0);
        const frame_walk w0 = walk(b, 0, offs, 23);
        CHECK(w0.nframes == 0 && w0.walked == 0);
        const frame_walk w5 = walk(b, 5, offs, 23);
        CHECK(w5.nframes == 5 && w5.walked == 97 && !w5.all_full && offs[4] == 92);
    }
    {  // a length that would pass 4 GiB: 64-bit arithmetic, the frame is cut, nothing wraps
        std::vector<uint8_t> b;
        frame(b, 19);
        frame(b, 8, 0xffffffffu);
        const frame_walk w = walk(b, 100, offs, 23);
        CHECK(w.nframes == 1 && w.walked == 23 && w.next_len == 0x100000003ull);
        std::vector<uint8_t> c;
        frame(c, 8, 0xfffffffcu);  // 4 + BE32 == 2^32 exactly
        const frame_walk wc = walk(c, 100, offs, 23);
        CHECK(wc.nframes == 0 && wc.walked == 0 && wc.next_len == 0x100000000ull);
    }
    std::printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
