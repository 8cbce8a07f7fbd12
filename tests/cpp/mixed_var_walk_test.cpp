// srpc::gpu::judge_reply_mixed (include/srpc/mixed_walk.hpp): the host form
// of the per-frame tables of srpc_frames_unpack_replies_mixed_var -- a string
// plan's frame by the table of srpc_frames_unpack_replies_var, a fixed plan's by
// that of srpc_frames_unpack_replies, each call under its own plan.  A
// stand-alone program, so it can be built with -fsanitize=address,undefined and
// simply run: every stream is a heap allocation of exactly its bytes, so a read
// past its end is an ASan error.
#include <srpc/mixed_walk.hpp>

#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace srpc::gpu;

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
static bytes be32(uint32_t n) {
    return {static_cast<uint8_t>(n >> 24), static_cast<uint8_t>(n >> 16), static_cast<uint8_t>(n >> 8), static_cast<uint8_t>(n)};
}
// u8 code | u64 len(name) | name: the unframed response prefix
static bytes prefix_of(uint8_t code, std::string const& name) {
    bytes p{code};
    put_u64(p, name.size());
    p.insert(p.end(), name.begin(), name.end());
    return p;
}
static bytes framed(bytes const& payload) {
    bytes f = be32(static_cast<uint32_t>(payload.size()));
    f.insert(f.end(), payload.begin(), payload.end());
    return f;
}

// plan 0: Number (fixed, one int32), plan 1: Mix (string, int32, string, int16), plan 2: Text (one string)
struct plans3 {
    bytes fixed_prefix, mix_prefix, text_prefix;
    const uint8_t mix_leaf[4] = {0, 4, 0, 2};
    const uint8_t text_leaf[1] = {0};
    std::vector<mixed_reply_plan> plans;
    plans3() : plans(3) {
        fixed_prefix = framed(prefix_of(0, "Number"));
        const bytes len = be32(static_cast<uint32_t>(fixed_prefix.size() - 4 + 4));  // the payload holds the body too
        std::memcpy(fixed_prefix.data(), len.data(), 4);
        mix_prefix = prefix_of(0, "Mix");
        text_prefix = prefix_of(0, "Text");
        plans[0].prefix = fixed_prefix.data();
        plans[0].prefix_len = fixed_prefix.size();
        plans[0].F = fixed_prefix.size() + 4;
        plans[1].var = true;
        plans[1].prefix = mix_prefix.data();
        plans[1].prefix_len = mix_prefix.size();
        plans[1].leaf = mix_leaf;
        plans[1].nleaves = 4;
        plans[2].var = true;
        plans[2].prefix = text_prefix.data();
        plans[2].prefix_len = text_prefix.size();
        plans[2].leaf = text_leaf;
        plans[2].nleaves = 1;
        for (auto& p : plans) p.cap = 1000;
    }
    bytes number(uint8_t code, int32_t v) const {
        bytes f = fixed_prefix;
        f[4] = code;
        for (int i = 0; i < 4; ++i) f.push_back(static_cast<uint8_t>(static_cast<uint32_t>(v) >> (8 * i)));
        return f;
    }
    bytes mix(uint8_t code, std::string const& a, std::string const& c) const {
        bytes p = mix_prefix;
        p[0] = code;
        put_u64(p, a.size());
        p.insert(p.end(), a.begin(), a.end());
        p.insert(p.end(), {1, 2, 3, 4});
        put_u64(p, c.size());
        p.insert(p.end(), c.begin(), c.end());
        p.insert(p.end(), {5, 6});
        return framed(p);
    }
    bytes text(uint8_t code, std::string const& s) const {
        bytes p = text_prefix;
        p[0] = code;
        put_u64(p, s.size());
        p.insert(p.end(), s.begin(), s.end());
        return framed(p);
    }
};

// exactly-sized heap copy: ASan sees any read past `len`
static std::unique_ptr<uint8_t[]> exact(bytes const& b) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[b.empty() ? 1 : b.size()]);
    if (!b.empty()) std::memcpy(p.get(), b.data(), b.size());
    return p;
}

// the frame alone in a stream of exactly its bytes, judged as a call of plan k
static reply_frame judge(plans3 const& P, uint32_t k, bytes const& f, uint32_t rank = 0) {
    const auto b = exact(f);
    return judge_reply_mixed(b.get(), f.size(), 0, f.size(), k, rank, P.plans.data(), 3);
}

static bool is(reply_frame r, reply_kind kind, uint8_t code) { return r.kind == kind && r.code == code; }

static void rows_of_the_tables() {
    const plans3 P;
    // full frames, any code, each under its own plan
    for (uint8_t code : {uint8_t{0}, uint8_t{1}, uint8_t{2}}) {
        CHECK(is(judge(P, 0, P.number(code, -7)), reply_kind::full, code));
        CHECK(is(judge(P, 1, P.mix(code, "hello", "")), reply_kind::full, code));
        CHECK(is(judge(P, 1, P.mix(code, "", std::string(300, 'x'))), reply_kind::full, code));
        CHECK(is(judge(P, 2, P.text(code, "")), reply_kind::full, code));
    }
    // bare frames under every plan; a bare code 0 is no answer
    const bytes bare = framed({1}), bare0 = framed({0});
    for (uint32_t k = 0; k < 3; ++k) {
        CHECK(is(judge(P, k, bare), reply_kind::bare, 1));
        CHECK(is(judge(P, k, bare0), reply_kind::bad_prefix, 0));
    }
    // the first row: no header, BE32 != len - 4, an empty payload
    for (uint32_t k = 0; k < 3; ++k) {
        CHECK(is(judge(P, k, {}), reply_kind::bad_bounds, 0xFF));
        CHECK(is(judge(P, k, {0, 0, 0}), reply_kind::bad_bounds, 0xFF));
        CHECK(is(judge(P, k, be32(0)), reply_kind::bad_bounds, 0xFF));
        bytes f = P.text(0, "abc");
        f[3] += 1;
        CHECK(is(judge(P, k, f), reply_kind::bad_bounds, 0xFF));
    }
    // a frame valid for another plan than its call's
    CHECK(is(judge(P, 0, P.text(0, "abc")), reply_kind::bad_prefix, 0));
    CHECK(is(judge(P, 1, P.text(0, "abc")), reply_kind::bad_prefix, 0));
    CHECK(is(judge(P, 2, P.number(2, 5)), reply_kind::bad_prefix, 2));
    CHECK(is(judge(P, 2, P.mix(0, "a", "b")), reply_kind::bad_prefix, 0));
    // a fixed plan's frame one byte longer: not its length
    bytes longer = P.number(0, 1);
    longer.push_back(0);
    longer[3] += 1;
    CHECK(is(judge(P, 0, longer), reply_kind::bad_prefix, 0));
    // a payload shorter than the string plan's prefix
    bytes cut = P.text_prefix;
    cut.resize(cut.size() - 2);
    CHECK(is(judge(P, 2, framed(cut)), reply_kind::bad_prefix, 0));
    // the prefix matches but the walk leaves the frame, or ends before its end
    bytes early = P.mix(0, "hello", "world");
    early.push_back(9);
    early[3] += 1;
    CHECK(is(judge(P, 1, early), reply_kind::bad_bounds, 0));
    bytes late = P.mix(0, "hello", "world");
    late.pop_back();
    late[3] -= 1;
    CHECK(is(judge(P, 1, late), reply_kind::bad_bounds, 0));
    bytes nolen = P.text_prefix;  // no room for the string's length
    nolen.insert(nolen.end(), {1, 0, 0});
    CHECK(is(judge(P, 2, framed(nolen)), reply_kind::bad_bounds, 0));
}

static void string_lengths_cannot_wrap() {
    const plans3 P;
    for (uint64_t huge : {1ull << 63, ~0ull, (1ull << 63) - 1, 4ull}) {
        bytes f = P.text(0, "abc");
        const size_t at = 4 + P.text_prefix.size();
        for (int i = 0; i < 8; ++i) f[at + i] = static_cast<uint8_t>(huge >> (8 * i));
        CHECK(is(judge(P, 2, f), reply_kind::bad_bounds, 0));
        // the second string of Mix
        bytes g = P.mix(1, "hello", "xy");
        const size_t at2 = 4 + P.mix_prefix.size() + 8 + 5 + 4;
        for (int i = 0; i < 8; ++i) g[at2 + i] = static_cast<uint8_t>(huge >> (8 * i));
        CHECK(is(judge(P, 1, g), reply_kind::bad_bounds, 1));
    }
}

static void bad_calls_and_offsets() {
    plans3 P;
    const bytes f = P.text(0, "abc");
    // an id out of range, no rank, no element left: the first row whatever the bytes
    const auto b = exact(f);
    CHECK(is(judge_reply_mixed(b.get(), f.size(), 0, f.size(), 3, 0, P.plans.data(), 3), reply_kind::bad_bounds, 0xFF));
    CHECK(is(judge_reply_mixed(b.get(), f.size(), 0, f.size(), 2, mixed_no_rank, P.plans.data(), 3),
             reply_kind::bad_bounds, 0xFF));
    P.plans[2].first = 990;
    CHECK(is(judge(P, 2, f, 9), reply_kind::full, 0));
    CHECK(is(judge(P, 2, f, 10), reply_kind::bad_bounds, 0xFF));
    P.plans[2].first = 1000;
    CHECK(is(judge(P, 2, f, 0), reply_kind::bad_bounds, 0xFF));
    P.plans[2].first = 0;
    // offsets out of order or past the end, under a string plan and a fixed one: nothing is read
    for (uint32_t k : {0u, 2u}) {
        CHECK(is(judge_reply_mixed(b.get(), f.size(), 5, 2, k, 0, P.plans.data(), 3), reply_kind::bad_bounds, 0xFF));
        CHECK(is(judge_reply_mixed(b.get(), f.size(), 0, f.size() + 1, k, 0, P.plans.data(), 3), reply_kind::bad_bounds,
                 0xFF));
        CHECK(is(judge_reply_mixed(b.get(), f.size(), f.size() + 1, f.size() + 9, k, 0, P.plans.data(), 3),
                 reply_kind::bad_bounds, 0xFF));
    }
    // two frames in one stream, each judged inside its own bytes
    bytes two = P.mix(0, "a", "bc");
    const size_t cut = two.size();
    const bytes second = P.number(2, 9);
    two.insert(two.end(), second.begin(), second.end());
    const auto s = exact(two);
    CHECK(is(judge_reply_mixed(s.get(), two.size(), 0, cut, 1, 0, P.plans.data(), 3), reply_kind::full, 0));
    CHECK(is(judge_reply_mixed(s.get(), two.size(), cut, two.size(), 0, 0, P.plans.data(), 3), reply_kind::full, 2));
    CHECK(is(judge_reply_mixed(s.get(), two.size(), 0, two.size(), 1, 0, P.plans.data(), 3), reply_kind::bad_bounds, 0xFF));
}

int main() {
    rows_of_the_tables();
    string_lengths_cannot_wrap();
    bad_calls_and_offsets();
    std::printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
