// srpc::gpu::walk_reply_var (include/srpc/reply_walk.hpp): the host form of the
// per-frame table of srpc_frames_unpack_replies_var, and tally_replies over a
// literal chunk of such frames.  A stand-alone program,
// so it can be built with -fsanitize=address,undefined and simply run: every
// frame is a heap allocation of exactly its bytes, so a read past the frame's
// end is an ASan error.
#include <srpc/reply_walk.hpp>

#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using srpc::gpu::reply_frame;
using srpc::gpu::reply_kind;
using srpc::gpu::walk_reply_var;

static int g_fail = 0, g_pass = 0;
#define CHECK(c)                                                                    \
    do {                                                                            \
        if (c) ++g_pass;                                                            \
        else { ++g_fail; std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); } \
    } while (0)

using bytes = std::vector<uint8_t>;

static void put_u64(bytes& b, uint64_t v) {
    for (int i = 0; i < 8; ++i) b.push_back(static_cast<uint8_t>(v >> (8 * i)));
}
static void put_str(bytes& b, std::string const& s) {
    put_u64(b, s.size());
    b.insert(b.end(), s.begin(), s.end());
}
static bytes prefix_of(uint8_t code, std::string const& name) {
    bytes p{code};
    put_str(p, name);
    return p;
}
// BE32(payload size) | payload
static bytes framed(bytes const& payload) {
    const uint32_t n = static_cast<uint32_t>(payload.size());
    bytes f{static_cast<uint8_t>(n >> 24), static_cast<uint8_t>(n >> 16), static_cast<uint8_t>(n >> 8),
            static_cast<uint8_t>(n)};
    f.insert(f.end(), payload.begin(), payload.end());
    return f;
}
static void set_be32(bytes& f, uint32_t n) {
    f[0] = static_cast<uint8_t>(n >> 24);
    f[1] = static_cast<uint8_t>(n >> 16);
    f[2] = static_cast<uint8_t>(n >> 8);
    f[3] = static_cast<uint8_t>(n);
}

// The message `string a | int32 b | string c | int16 d` named "Mix".
static const uint8_t kSizes[4] = {0, 4, 0, 2};
static const bytes kPrefix = prefix_of(0, "Mix");

static bytes body(std::string const& a, std::string const& c) {
    bytes b;
    put_str(b, a);
    for (int i = 0; i < 4; ++i) b.push_back(static_cast<uint8_t>(0x10 + i));
    put_str(b, c);
    b.push_back(0x77);
    b.push_back(0x78);
    return b;
}
static bytes full_frame(uint8_t code, std::string const& a, std::string const& c) {
    bytes p = prefix_of(code, "Mix");
    const bytes b = body(a, c);
    p.insert(p.end(), b.begin(), b.end());
    return framed(p);
}

// The walk over an exact-size heap copy of the frame.
static reply_frame walk(bytes const& f, uint64_t len) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[len ? len : 1]);
    if (len) std::memcpy(exact.get(), f.data(), len);
    std::unique_ptr<uint8_t[]> pre(new uint8_t[kPrefix.size()]);
    std::memcpy(pre.get(), kPrefix.data(), kPrefix.size());
    return walk_reply_var(exact.get(), len, pre.get(), kPrefix.size(), kSizes, 4);
}
static reply_frame walk(bytes const& f) { return walk(f, f.size()); }
static bool is(reply_frame r, reply_kind k, uint8_t code) { return r.kind == k && r.code == code; }

int main() {
    const uint64_t P = kPrefix.size();  // 1 + 8 + 3
    // ---- every row of the table ----
    for (uint8_t code : {0, 1, 2, 200}) {  // full, whatever the code; strings empty or not
        CHECK(is(walk(full_frame(code, "", "")), reply_kind::full, code));
        CHECK(is(walk(full_frame(code, "hello", "")), reply_kind::full, code));
        CHECK(is(walk(full_frame(code, "", std::string(300, 'x'))), reply_kind::full, code));
    }
    CHECK(is(walk(framed({1})), reply_kind::bare, 1));
    CHECK(is(walk(framed({255})), reply_kind::bare, 255));
    CHECK(is(walk(framed({0})), reply_kind::bad_prefix, 0));  // one zero byte is no answer
    CHECK(is(walk(framed({})), reply_kind::bad_bounds, 0xFF));  // an empty payload
    for (uint64_t k = 0; k < 4; ++k) CHECK(is(walk(bytes(k, 0)), reply_kind::bad_bounds, 0xFF));
    {  // BE32 off by one, either way
        bytes f = full_frame(0, "ab", "c");
        set_be32(f, static_cast<uint32_t>(f.size() - 4 + 1));
        CHECK(is(walk(f), reply_kind::bad_bounds, 0xFF));
        set_be32(f, static_cast<uint32_t>(f.size() - 4 - 1));
        CHECK(is(walk(f), reply_kind::bad_bounds, 0xFF));
    }
    {  // a wrong name, at its first and last byte and in its length
        for (uint64_t at : {uint64_t{4 + 1}, uint64_t{4 + 9}, 4 + P - 1}) {
            bytes f = full_frame(2, "ab", "c");
            f[at] ^= 0x20;
            CHECK(is(walk(f), reply_kind::bad_prefix, 2));
        }
        CHECK(is(walk(framed({7, 1, 2, 3})), reply_kind::bad_prefix, 7));  // junk shorter than the prefix
        bytes junk(4096, 0x5a);
        CHECK(is(walk(framed(junk)), reply_kind::bad_prefix, 0x5a));
    }
    // ---- a full frame cut at every byte, with its BE32 kept and with it corrected ----
    {
        const bytes f = full_frame(1, "hello", "wor");
        for (uint64_t k = 0; k < f.size(); ++k) {
            CHECK(walk(f, k).kind == reply_kind::bad_bounds && walk(f, k).code == 0xFF);  // BE32 says more
            if (k < 4) continue;
            bytes g(f.begin(), f.begin() + static_cast<long>(k));
            set_be32(g, static_cast<uint32_t>(k - 4));
            const reply_frame r = walk(g);
            if (k == 4) CHECK(is(r, reply_kind::bad_bounds, 0xFF));
            else if (k == 5) CHECK(is(r, reply_kind::bare, 1));
            else if (k - 4 < P) CHECK(is(r, reply_kind::bad_prefix, 1));
            else CHECK(is(r, reply_kind::bad_bounds, 1));  // the prefix is whole, the fields are not
        }
        bytes z = full_frame(0, "hello", "wor");  // code 0 cut to one byte: not bare
        z.resize(5);
        set_be32(z, 1);
        CHECK(is(walk(z), reply_kind::bad_prefix, 0));
    }
    // ---- string lengths that would wrap ----
    for (uint64_t huge : {uint64_t{1} << 63, ~uint64_t{0}, (uint64_t{1} << 32) + 5}) {
        for (int which = 0; which < 2; ++which) {
            bytes f = full_frame(0, "hello", "wor");
            const uint64_t at = which == 0 ? 4 + P : 4 + P + 8 + 5 + 4;  // the length word of a / of c
            for (int b = 0; b < 8; ++b) f[at + b] = static_cast<uint8_t>(huge >> (8 * b));
            CHECK(is(walk(f), reply_kind::bad_bounds, 0));
        }
    }
    // ---- the walk ends one byte before / after the frame's end ----
    {
        bytes f = full_frame(0, "hello", "wor");
        const uint64_t at = 4 + P + 8 + 5 + 4;  // c's length: 3
        f[at] = 2;                              // ends one byte short of the end
        CHECK(is(walk(f), reply_kind::bad_bounds, 0));
        f[at] = 4;                              // the last field would end one byte past it
        CHECK(is(walk(f), reply_kind::bad_bounds, 0));
        f[at] = 5;                              // the string itself ends exactly at the end: no room for d
        CHECK(is(walk(f), reply_kind::bad_bounds, 0));
        f[at] = 6;                              // the string runs one past the end
        CHECK(is(walk(f), reply_kind::bad_bounds, 0));
        f[at] = 3;
        CHECK(is(walk(f), reply_kind::full, 0));
        bytes g = f;  // one trailing byte after a good walk
        g.push_back(0);
        set_be32(g, static_cast<uint32_t>(g.size() - 4));
        CHECK(is(walk(g), reply_kind::bad_bounds, 0));
    }
    // ---- tally_replies over a literal chunk of string replies ----
    {
        struct tally {
            uint64_t ok = 0, failed = 0, malformed = 0;
            bool is(uint64_t o, uint64_t f, uint64_t m) const { return ok == o && failed == f && malformed == m; }
        };
        bytes wrong = full_frame(0, "ab", "c");
        wrong[4 + 9] ^= 0x20;  // the name's first letter
        bytes overrun = full_frame(0, "hello", "wor");
        overrun[4 + P + 8 + 5 + 4 + 1] = 4;  // c's length + 1024: past the frame's end
        const std::vector<bytes> frames = {full_frame(0, "hello", ""), full_frame(2, "", "x"), framed({1}), framed({0}),
                                           wrong,                      overrun,                framed({})};
        const uint8_t codes[7] = {0, 2, 1, 0, 0, 0, 0xFF};  // d_codes by the table
        auto judge = [&](uint64_t i) { return walk(frames[i]); };
        tally t;
        srpc::gpu::tally_replies(codes, 7, true, judge, t);  // flagged: frame by frame
        CHECK(t.is(1, 2, 4));
        tally s;
        srpc::gpu::tally_replies(codes, 7, false, judge, s);  // the shortcut trusts the codes: right only when unflagged
        CHECK(s.is(4, 3, 0));
        tally u, v;  // the three well-formed rows alone count the same either way
        srpc::gpu::tally_replies(codes, 3, false, judge, u);
        srpc::gpu::tally_replies(codes, 3, true, judge, v);
        CHECK(u.is(1, 2, 0) && v.is(1, 2, 0));
    }
    std::printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
