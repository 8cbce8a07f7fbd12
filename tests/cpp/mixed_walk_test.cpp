// srpc::gpu::mixed_ranks / judge_reply_fixed / judge_reply_mixed
// (include/srpc/mixed_walk.hpp): the host form of a mixed batch's ranks and of
// the per-frame table of srpc_frames_unpack_replies_mixed, and tally_replies
// (include/srpc/reply_walk.hpp) over literal chunks of them.  A stand-alone
// program, so it can be built with -fsanitize=address,undefined and simply
// run: every stream is a heap allocation of exactly its bytes, so a read past
// its end is an ASan error.
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

// BE32(payload) | code | u64 len(name) | name: the framed response prefix of a body of `body` bytes
static bytes prefix_of(uint8_t code, std::string const& name, uint32_t body) {
    const uint32_t n = static_cast<uint32_t>(1 + 8 + name.size() + body);
    bytes p{static_cast<uint8_t>(n >> 24), static_cast<uint8_t>(n >> 16), static_cast<uint8_t>(n >> 8),
            static_cast<uint8_t>(n), code};
    for (int i = 0; i < 8; ++i) p.push_back(static_cast<uint8_t>(name.size() >> (8 * i)));
    p.insert(p.end(), name.begin(), name.end());
    return p;
}

struct plan3 {
    bytes prefix[3];
    uint32_t body[3] = {4, 17, 1};
    std::vector<mixed_reply_plan> plans;
    plan3() : plans(3) {
        const char* names[3] = {"Number", "all_kinds", "Flag"};
        for (int k = 0; k < 3; ++k) {
            prefix[k] = prefix_of(0, names[k], body[k]);
            plans[k].prefix = prefix[k].data();
            plans[k].prefix_len = prefix[k].size();
            plans[k].F = prefix[k].size() + body[k];
            plans[k].first = 0;
            plans[k].cap = 1000;
        }
    }
    bytes frame(int k, uint8_t code, uint8_t fill) const {
        bytes f = prefix[k];
        f[4] = code;
        f.insert(f.end(), body[k], fill);
        return f;
    }
};

// exactly-sized heap copy: ASan sees any read past `len`
static std::unique_ptr<uint8_t[]> exact(const uint8_t* p, size_t len) {
    std::unique_ptr<uint8_t[]> b(new uint8_t[len ? len : 1]);
    if (len) std::memcpy(b.get(), p, len);
    return b;
}

static void ranks() {
    const uint8_t m[] = {2, 0, 2, 2, 1, 0, 7, 2, 255, 1};
    uint32_t rank[10];
    uint64_t counts[4];
    const uint64_t bad = mixed_ranks(m, 10, 3, rank, counts);
    const uint32_t want[10] = {0, 0, 1, 2, 0, 1, mixed_no_rank, 3, mixed_no_rank, 1};
    CHECK(bad == 6 && std::memcmp(rank, want, sizeof want) == 0);
    CHECK(counts[0] == 2 && counts[1] == 2 && counts[2] == 4 && counts[3] == 2);
    CHECK(mixed_ranks(m, 6, 3, rank, counts) == ~0ull && counts[3] == 0);
    CHECK(mixed_ranks(nullptr, 0, 1, rank, counts) == ~0ull && counts[0] == 0 && counts[1] == 0);
}

static void table() {
    const plan3 P;
    for (int k = 0; k < 3; ++k) {
        const bytes f = P.frame(k, 2, 0x5a);
        auto b = exact(f.data(), f.size());
        reply_frame r = judge_reply_mixed(b.get(), f.size(), 0, f.size(), k, 0, P.plans.data(), 3);
        CHECK(r.kind == reply_kind::full && r.code == 2);
        // another plan's well-formed frame: bad_prefix with its code
        r = judge_reply_mixed(b.get(), f.size(), 0, f.size(), (k + 1) % 3, 0, P.plans.data(), 3);
        CHECK(r.kind == reply_kind::bad_prefix && r.code == 2);
        // a bad call is the first row whatever the bytes
        r = judge_reply_mixed(b.get(), f.size(), 0, f.size(), 3, mixed_no_rank, P.plans.data(), 3);
        CHECK(r.kind == reply_kind::bad_bounds && r.code == 0xFF);
        r = judge_reply_mixed(b.get(), f.size(), 0, f.size(), k, 1000, P.plans.data(), 3);
        CHECK(r.kind == reply_kind::bad_bounds && r.code == 0xFF);
        // a wrong name byte
        bytes g = f;
        g[g.size() - P.body[k] - 1] ^= 0x20;
        auto c = exact(g.data(), g.size());
        r = judge_reply_mixed(c.get(), g.size(), 0, g.size(), k, 0, P.plans.data(), 3);
        CHECK(r.kind == reply_kind::bad_prefix && r.code == 2);
    }
    const uint8_t bare[5] = {0, 0, 0, 1, 9}, bare0[5] = {0, 0, 0, 1, 0}, none[4] = {0, 0, 0, 0};
    auto b = exact(bare, 5);
    reply_frame r = judge_reply_mixed(b.get(), 5, 0, 5, 1, 0, P.plans.data(), 3);
    CHECK(r.kind == reply_kind::bare && r.code == 9);
    b = exact(bare0, 5);
    r = judge_reply_mixed(b.get(), 5, 0, 5, 1, 0, P.plans.data(), 3);
    CHECK(r.kind == reply_kind::bad_prefix && r.code == 0);
    b = exact(none, 4);
    r = judge_reply_mixed(b.get(), 4, 0, 4, 1, 0, P.plans.data(), 3);
    CHECK(r.kind == reply_kind::bad_bounds && r.code == 0xFF);
    // offsets out of order and past the end
    r = judge_reply_mixed(b.get(), 4, 3, 1, 1, 0, P.plans.data(), 3);
    CHECK(r.kind == reply_kind::bad_bounds);
    r = judge_reply_mixed(b.get(), 4, 0, 9, 1, 0, P.plans.data(), 3);
    CHECK(r.kind == reply_kind::bad_bounds);
    r = judge_reply_mixed(b.get(), 4, 1u << 31, ~0ull, 1, 0, P.plans.data(), 3);
    CHECK(r.kind == reply_kind::bad_bounds);
}

// A three-plan stream of 40 frames (full, bare, one junk) cut at every length:
// the frames that still end inside keep their verdict, the cut one is
// bad_bounds (its BE32 no longer matches), nothing is read past the cut.
static void truncated_streams() {
    const plan3 P;
    constexpr uint32_t n = 40;
    uint8_t method[n];
    bytes stream;
    std::vector<uint64_t> offs(n + 1);
    std::vector<reply_kind> kind(n);
    for (uint32_t i = 0; i < n; ++i) {
        method[i] = static_cast<uint8_t>((i * 7 + i / 3) % 3);
        offs[i] = stream.size();
        bytes f;
        if (i % 9 == 4) {
            f = {0, 0, 0, 1, 3};
            kind[i] = reply_kind::bare;
        } else if (i == 21) {
            f = {0, 0, 0, 6, 7, 1, 2, 3, 4, 5};
            kind[i] = reply_kind::bad_prefix;
        } else {
            f = P.frame(method[i], static_cast<uint8_t>(i % 3), static_cast<uint8_t>(i));
            kind[i] = reply_kind::full;
        }
        stream.insert(stream.end(), f.begin(), f.end());
    }
    offs[n] = stream.size();
    uint32_t rank[n];
    uint64_t counts[4];
    CHECK(mixed_ranks(method, n, 3, rank, counts) == ~0ull);
    bool ok = true;
    for (uint64_t len = 0; len <= stream.size(); ++len) {
        auto b = exact(stream.data(), len);
        for (uint32_t i = 0; i < n; ++i) {
            const uint64_t end = i + 1 < n ? offs[i + 1] : len;  // the decode's convention
            const reply_frame r = judge_reply_mixed(b.get(), len, offs[i], end, method[i], rank[i], P.plans.data(), 3);
            // a frame past the cut ends past buf_len; the last frame, cut, has a BE32 that is not its length
            const bool whole = i + 1 < n ? offs[i + 1] <= len : len == stream.size();
            ok = ok && r.kind == (whole ? kind[i] : reply_kind::bad_bounds);
        }
    }
    CHECK(ok);
    // offsets out of order over the whole stream, ids out of range
    auto b = exact(stream.data(), stream.size());
    ok = true;
    for (uint32_t i = 0; i + 1 < n; ++i) {
        reply_frame r = judge_reply_mixed(b.get(), stream.size(), offs[i + 1], offs[i], method[i], rank[i], P.plans.data(), 3);
        ok = ok && r.kind == reply_kind::bad_bounds && r.code == 0xFF;
        r = judge_reply_mixed(b.get(), stream.size(), offs[i], offs[i + 1], 3 + i, rank[i], P.plans.data(), 3);
        ok = ok && r.kind == reply_kind::bad_bounds && r.code == 0xFF;
    }
    CHECK(ok);
}

struct tally {
    uint64_t ok = 0, failed = 0, malformed = 0;
    bool is(uint64_t o, uint64_t f, uint64_t m) const { return ok == o && failed == f && malformed == m; }
};

// The rule batch_client::call counted a flagged chunk by before it used
// judge_reply_fixed: 'm' malformed, 'o' ok, 'f' failed, from the frame's bytes
// and the code the decode gave it.
static char inline_rule(const uint8_t* f, uint64_t len, uint64_t fout, bytes const& prefix, uint8_t code) {
    const bool full = len == fout && std::memcmp(f, prefix.data(), 4) == 0 &&
                      std::memcmp(f + 5, prefix.data() + 5, prefix.size() - 5) == 0;
    const bool bare = len == 5 && f[4] != 0;
    return !(full || bare) ? 'm' : code == 0 ? 'o' : 'f';
}

// tally_replies over a literal chunk of one fixed method (plan 0: Number, F =
// 23): the shortcut of an unflagged chunk trusts the codes, the recount of a
// flagged one judges every frame, and judge_reply_fixed classifies every row as
// the inline rule did.
static void tally_of_a_fixed_chunk() {
    const plan3 P;
    const uint64_t F = P.plans[0].F;
    struct row {
        bytes frame;
        uint8_t code;  // d_codes[i] by the table of srpc_frames_unpack_replies
        char want;     // the recount's verdict
    };
    std::vector<row> rows;
    rows.push_back({P.frame(0, 0, 0x11), 0, 'o'});  // full
    rows.push_back({P.frame(0, 2, 0x22), 2, 'f'});  // full with a nonzero code
    rows.push_back({{0, 0, 0, 1, 1}, 1, 'f'});      // bare
    rows.push_back({{0, 0, 0, 1, 0}, 0, 'm'});      // bare with code 0: no answer (PREFIX)
    bytes g = P.frame(0, 0, 0x33);
    g[13] ^= 0x20;
    rows.push_back({g, 0, 'm'});  // one prefix byte wrong, the length right (PREFIX)
    rows.push_back({P.frame(0, 200, 0x44), 200, 'f'});  // only the code byte differs from the plan's prefix: full
    g = P.frame(0, 0, 0x55);
    g.push_back(0);
    g[3] += 1;
    rows.push_back({g, 0, 'm'});  // one byte longer, its BE32 agreeing (PREFIX)
    g = P.frame(0, 0, 0x66);
    g.pop_back();
    g[3] -= 1;
    rows.push_back({g, 0, 'm'});             // one byte shorter
    rows.push_back({{0, 0, 0, 0}, 0xFF, 'm'});  // an empty payload (BOUNDS, SRPC_REPLY_NO_CODE)
    CHECK(rows[0].frame.size() == F);

    bytes stream;
    std::vector<uint64_t> offs;
    std::vector<uint8_t> codes;
    for (row const& r : rows) {
        offs.push_back(stream.size());
        stream.insert(stream.end(), r.frame.begin(), r.frame.end());
        codes.push_back(r.code);
    }
    offs.push_back(stream.size());
    auto b = exact(stream.data(), stream.size());
    const uint64_t n = rows.size();
    auto judge = [&](uint64_t i) {
        return judge_reply_fixed(b.get(), stream.size(), offs[i], offs[i + 1], F, P.prefix[0].data(), P.prefix[0].size());
    };
    // every row alone: the verdict stated, and the inline rule's
    bool each = true, as_before = true;
    for (uint64_t i = 0; i < n; ++i) {
        tally t;
        tally_replies(codes.data() + i, 1, true, [&](uint64_t) { return judge(i); }, t);
        const char got = t.malformed ? 'm' : t.ok ? 'o' : 'f';
        each = each && t.ok + t.failed + t.malformed == 1 && got == rows[i].want;
        as_before = as_before && got == inline_rule(b.get() + offs[i], offs[i + 1] - offs[i], F, P.prefix[0], codes[i]);
    }
    CHECK(each);
    CHECK(as_before);
    // the chunk, flagged: 1 ok, 3 failed, 5 malformed
    tally t;
    tally_replies(codes.data(), n, true, judge, t);
    CHECK(t.is(1, 3, 5));
    // the shortcut reads the codes alone: 5 zeros, 4 others, nothing malformed -- right only for an unflagged chunk
    tally s;
    tally_replies(codes.data(), n, false, judge, s);
    CHECK(s.is(5, 4, 0));
    // an unflagged chunk (the first three rows: full, full with a code, bare) counts the same either way
    tally u, v;
    tally_replies(codes.data(), 3, false, judge, u);
    tally_replies(codes.data(), 3, true, judge, v);
    CHECK(u.is(1, 2, 0) && v.is(1, 2, 0));
    // both add to what is there, and no frames add nothing
    tally_replies(codes.data(), 3, false, judge, u);
    tally_replies(codes.data(), 0, true, judge, u);
    tally_replies(codes.data(), 0, false, judge, u);
    CHECK(u.is(2, 4, 0));
}

// The same through judge_reply_mixed over two plans, one of them short of
// elements: a bad call's frame is malformed whatever its bytes.
static void tally_of_a_mixed_chunk() {
    plan3 P;
    P.plans[1].first = 998;  // two elements left
    const uint8_t method[6] = {0, 1, 1, 1, 0, 7};
    uint32_t rank[6];
    uint64_t counts[4];
    (void)mixed_ranks(method, 6, 3, rank, counts);
    const bytes frames[6] = {P.frame(0, 0, 1), P.frame(1, 0, 2), P.frame(1, 3, 3),
                             P.frame(1, 0, 4),  // plan 1's third call: no element left
                             {0, 0, 0, 1, 1},   // bare
                             P.frame(0, 0, 5)};  // an id out of range
    const uint8_t codes[6] = {0, 0, 3, 0xFF, 1, 0xFF};
    bytes stream;
    std::vector<uint64_t> offs;
    for (bytes const& f : frames) {
        offs.push_back(stream.size());
        stream.insert(stream.end(), f.begin(), f.end());
    }
    offs.push_back(stream.size());
    auto b = exact(stream.data(), stream.size());
    tally t;
    tally_replies(codes, 6, true, [&](uint64_t i) {
        return judge_reply_mixed(b.get(), stream.size(), offs[i], offs[i + 1], method[i], rank[i], P.plans.data(), 3);
    }, t);
    CHECK(t.is(2, 2, 2));
}

int main() {
    ranks();
    table();
    truncated_streams();
    tally_of_a_fixed_chunk();
    tally_of_a_mixed_chunk();
    std::printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
