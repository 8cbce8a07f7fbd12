// needs: gpu
// srpc::gpu::batch_server (include/srpc/gpu_server.hpp) across its three routes
// -- buckets, ordered, ordered with string methods -- at max_batch 16, driven
// in lock-step over a socketpair: one send() of exactly 16 request frames, all
// their replies read and compared byte for byte, then the next round.  Every
// round is one batch, so the byte counters are exact:
//   (a) one server object served over successive connections with methods
//       registered and the mode changed in between (release + ensure on a
//       server that has already served);
//   (b) batch_stats::h2d_bytes / d2h_bytes on every route, with and without
//       unknown frames and string-method frames in the batch, as literal sums
//       over the frames sent;
//   (c) the warm-up calls: every handler is run at serve start on one zero
//       record -- twice per (re)allocation of the buffers, a record handler
//       four times -- and not again while nothing changed;
//   (d) a string method on the bucket route whose responses do not fit their
//       columns: answered by the CPU server in place for those batches
//       (overflow_batches), the column and record methods still from the GPU.
// The handlers work through the host (this program is host code).
#include "mixed_var_fixture.hpp"
#include "served_socketpair.hpp"

#include <srpc/server.hpp>
#include <sys/time.h>

constexpr uint64_t kMax = 16;  // frames per batch and per round
static const std::string kSquare = kMethods[0], kAdd = kMethods[1], kEcho = kMethods[2], kTwice = kMethods[3],
                         kDivide = kMethods[4], kSub = "Calculator_servicer::subtract";

// ---- the handlers: what they were warmed up with, how many batches they saw ----

struct seen {
    uint64_t warm = 0, batches = 0;
};
static seen g_square, g_sub, g_add, g_echo, g_twice, g_whole, g_whole_var;
static uint64_t g_overflowing = 0;

static int32_t sub_of(int32_t l, int32_t r) { return static_cast<int32_t>(static_cast<uint32_t>(l) - static_cast<uint32_t>(r)); }

static int square_cols(void* const* rq, void* const* rs, uint64_t n, hipStream_t s) {
    int32_t first = 0;
    if (hipStreamSynchronize(s) != hipSuccess) return SRPC_E_HIP;
    if (hipMemcpy(&first, rq[0], 4, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    ++(n == 1 && first == 0 ? g_square.warm : g_square.batches);
    return calc_batch<0>(rq, rs, n, s);
}
static int sub_cols(void* const* rq, void* const* rs, uint64_t n, hipStream_t s) {
    std::vector<int32_t> l(n), r(n), out(n);
    if (hipStreamSynchronize(s) != hipSuccess) return SRPC_E_HIP;
    if (hipMemcpy(l.data(), rq[0], 4 * n, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    if (hipMemcpy(r.data(), rq[1], 4 * n, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    ++(n == 1 && l[0] == 0 && r[0] == 0 ? g_sub.warm : g_sub.batches);
    for (uint64_t i = 0; i < n; ++i) out[i] = sub_of(l[i], r[i]);
    return hipMemcpy(rs[0], out.data(), 4 * n, hipMemcpyHostToDevice) == hipSuccess ? 0 : SRPC_E_HIP;
}
// add over arrays of the host's own TwoNumbers / Number objects
static int add_records(const void* d_reqs, void* d_resps, uint64_t n, hipStream_t s) {
    static const std::vector<uint32_t> qo = srpc::gpu::leaf_offsets<TwoNumbers>(), ro = srpc::gpu::leaf_offsets<Number>();
    std::vector<uint8_t> in(n * sizeof(TwoNumbers)), out(n * sizeof(Number), 0);
    if (hipStreamSynchronize(s) != hipSuccess) return SRPC_E_HIP;
    if (hipMemcpy(in.data(), d_reqs, in.size(), hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    bool zeros = true;
    for (uint64_t i = 0; i < n; ++i) {
        int32_t l, r;
        std::memcpy(&l, in.data() + i * sizeof(TwoNumbers) + qo[0], 4);
        std::memcpy(&r, in.data() + i * sizeof(TwoNumbers) + qo[1], 4);
        zeros = zeros && l == 0 && r == 0;
        const int32_t v = compute(1, l, r);
        std::memcpy(out.data() + i * sizeof(Number) + ro[0], &v, 4);
    }
    ++(n == 1 && zeros ? g_add.warm : g_add.batches);
    return hipMemcpy(d_resps, out.data(), out.size(), hipMemcpyHostToDevice) == hipSuccess ? 0 : SRPC_E_HIP;
}
static int echo_strings(srpc::gpu::var_batch const& b, hipStream_t s) {
    bool zeros = true;
    const int rc = var_through_host<MP, MP>(b, s, [&zeros](MP const& q) {
        zeros = zeros && zero(q);
        return echo_fixture::answer(q);
    });
    ++(b.n == 1 && zeros ? g_echo.warm : g_echo.batches);
    return rc;
}
// twice with honest offsets and only the chars that fit: what a device handler
// that counts before it writes leaves behind.
static int twice_clipped(srpc::gpu::var_batch const& b, hipStream_t s) {
    if (hipStreamSynchronize(s) != hipSuccess) return SRPC_E_HIP;
    std::vector<uint64_t> offs(b.n + 1);
    if (hipMemcpy(offs.data(), b.req_str_offs[0], 8 * (b.n + 1), hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    std::vector<char> chars(offs[b.n] - offs[0]);
    if (!chars.empty() &&
        hipMemcpy(chars.data(), static_cast<const char*>(b.req_cols[0]) + offs[0], chars.size(), hipMemcpyDeviceToHost) !=
            hipSuccess)
        return SRPC_E_HIP;
    ++(b.n == 1 && chars.empty() ? g_twice.warm : g_twice.batches);
    std::string a, c;
    std::vector<uint64_t> oa(b.n + 1, 0), oc(b.n + 1, 0);
    for (uint64_t r = 0; r < b.n; ++r) {
        Text q;
        q.s.assign(chars.data() + (offs[r] - offs[0]), chars.data() + (offs[r + 1] - offs[0]));
        const TwoTexts t = twice(q);
        a += t.a, c += t.b;
        oa[r + 1] = a.size(), oc[r + 1] = c.size();
    }
    if (a.size() > b.resp_cap[0] || c.size() > b.resp_cap[1]) ++g_overflowing;
    a.resize(std::min<uint64_t>(a.size(), b.resp_cap[0]));
    c.resize(std::min<uint64_t>(c.size(), b.resp_cap[1]));
    if (!a.empty() && hipMemcpy(b.resp_cols[0], a.data(), a.size(), hipMemcpyHostToDevice) != hipSuccess) return SRPC_E_HIP;
    if (!c.empty() && hipMemcpy(b.resp_cols[1], c.data(), c.size(), hipMemcpyHostToDevice) != hipSuccess) return SRPC_E_HIP;
    if (hipMemcpy(b.resp_str_offs[0], oa.data(), 8 * (b.n + 1), hipMemcpyHostToDevice) != hipSuccess) return SRPC_E_HIP;
    return hipMemcpy(b.resp_str_offs[1], oc.data(), 8 * (b.n + 1), hipMemcpyHostToDevice) == hipSuccess ? 0 : SRPC_E_HIP;
}
// the whole-batch handlers: only ever run on the warm-up's one unknown frame here
static int whole_batch(srpc::gpu::ordered_batch const& b, hipStream_t) {
    if (b.n != 1 || b.methods != 1 || b.counts[0] != 0 || b.counts[1] != 1) return SRPC_E_INVALID;
    ++g_whole.warm;
    return 0;
}
static int whole_var_batch(srpc::gpu::ordered_var_batch const& b, hipStream_t) {
    if (b.n != 1 || b.methods != 1 || b.counts[0] != 0 || b.counts[1] != 1) return SRPC_E_INVALID;
    ++g_whole_var.warm;
    return 0;
}

// ---- the calls: a request frame and the reply frame it must get ----

using scripted::bytes;

struct call {
    char kind;  // q square, a add, s subtract, e echo, t twice, u divide (nobody's)
    bytes frame, reply;
};

template <class Req>
static bytes request(std::string const& method, Req const& v) {
    srpc::packer p;
    srpc::request_t<Req> q;
    q.set_method_name(method);
    q.set_value(v);
    p.pack_request(q);
    bytes f = srpc::gpu::be32(static_cast<uint32_t>(p.size()));
    f.insert(f.end(), p.data(), p.data() + p.size());
    return f;
}

static int32_t nonzero(uint64_t i) { return value(i) | 1; }

// Call i of kind `kind`.  twice_chars: the length of a twice request's string.
static call make_call(char kind, uint64_t i, uint64_t twice_chars = 3) {
    call c{kind, {}, {}};
    Number n;
    TwoNumbers two;
    two.left = nonzero(3 * i + 1), two.right = nonzero(7 * i + 2);
    switch (kind) {
    case 'q':
        n.num = nonzero(i);
        c.frame = request(kSquare, n);
        n.num = compute(0, n.num, 0);
        c.reply = scripted::full(n);
        break;
    case 'a':
        c.frame = request(kAdd, two);
        n.num = compute(1, two.left, two.right);
        c.reply = scripted::full(n);
        break;
    case 's':
        c.frame = request(kSub, two);
        n.num = sub_of(two.left, two.right);
        c.reply = scripted::full(n);
        break;
    case 'e': {
        MP m;
        echo_fixture::fill_request(m, i);
        c.frame = request(kEcho, m);
        c.reply = scripted::full(echo_fixture::answer(m));
        break;
    }
    case 't': {
        Text t;
        for (uint64_t j = 0; j < twice_chars; ++j) t.s.push_back(static_cast<char>('a' + (i + j) % 26));
        c.frame = request(kTwice, t);
        c.reply = scripted::full(twice(t));  // from the GPU or from the CPU server: the same bytes
        break;
    }
    default:
        c.frame = request(kDivide, two);
        c.reply = scripted::bare(srpc::RPC_ERR_FUNCTION_NOT_REGISTERED);
        break;
    }
    return c;
}

enum class route { bucket, ordered, ordered_var };

// What a connection's rounds add up to, by batch_server's accounting: per batch
// of nf frames in `used` bytes, h2d = used + 4 nf (the frames and their
// offsets); d2h = the GPU's reply bytes, plus
//   bucket / ordered: nf class bytes when the batch has unknown frames or a
//     string method is registered, and 8 (nf + 1) offset bytes when it has both
//     unknown frames and a string method's frames;
//   ordered_var: nf class bytes and 4 (nf + 1) offset bytes when it has unknown
//     frames.
// (The counts, the string ends and the statuses are not counted.)
struct tally {
    uint64_t rounds = 0, h2d = 0, d2h = 0, gpu = 0, cpu = 0, gpu_batches = 0, mixed = 0;
};

// One round: the 16 calls of `pattern` sent in one send(), their replies read
// and compared.  cpu_kinds: the kinds the CPU answers in this round.
static bool exchange(int fd, tally& t, route rt, bool string_methods, const char* pattern, const char* cpu_kinds = "u",
                     uint64_t twice_chars = 3) {
    std::vector<call> round;
    for (uint64_t i = 0; pattern[i]; ++i) round.push_back(make_call(pattern[i], 100 * t.rounds + i, twice_chars));
    if (round.size() != kMax) std::exit(3);
    bytes out, want;
    uint64_t total = 0, unknown = 0, per_kind[128] = {};
    bool any_var = false;
    for (call& c : round) {
        const bool cpu = std::strchr(cpu_kinds, c.kind) != nullptr;
        if (cpu && c.kind != 't') {  // no registered method's: the bare error, whatever the frame asks for
            c.kind = 'u';
            c.reply = scripted::bare(srpc::RPC_ERR_FUNCTION_NOT_REGISTERED);
        }
        out.insert(out.end(), c.frame.begin(), c.frame.end());
        want.insert(want.end(), c.reply.begin(), c.reply.end());
        if (cpu) ++unknown;
        else total += c.reply.size();
        any_var = any_var || c.kind == 'e' || c.kind == 't';  // a demoted bucket's frames included
        per_kind[static_cast<int>(c.kind)] += c.kind == 'u' ? 0 : 1;
    }
    const uint64_t nf = kMax;
    t.rounds += 1;
    t.h2d += out.size() + 4 * nf;
    t.d2h += rt == route::ordered_var ? total + (unknown ? nf + 4 * (nf + 1) : 0)
                                      : total + (unknown || string_methods ? nf : 0) + (unknown && any_var ? 8 * (nf + 1) : 0);
    t.gpu += nf - unknown;
    t.cpu += unknown;
    if (total) {
        t.gpu_batches += 1;
        bool mixed = false;  // a registered method has some of the frames, not all
        for (uint64_t n : per_kind) mixed = mixed || (n && n != nf);
        t.mixed += mixed ? 1 : 0;
    }
    if (send(fd, out.data(), out.size(), MSG_NOSIGNAL) != static_cast<ssize_t>(out.size())) return false;
    bytes got(want.size());
    uint64_t have = 0;
    while (have < got.size()) {
        const ssize_t k = recv(fd, got.data() + have, got.size() - have, 0);
        if (k <= 0) return false;  // closed, or the receive timeout: the server is stuck
        have += static_cast<uint64_t>(k);
    }
    return got == want;
}

static void check_stats(served_socketpair const& sp, tally const& t) {
    CHECK(sp.thrown == 0);
    CHECK(sp.stats.requests == t.gpu + t.cpu && sp.stats.gpu_requests == t.gpu && sp.stats.fallback_requests == t.cpu);
    CHECK(sp.stats.gpu_batches == t.gpu_batches && sp.stats.mixed_batches == t.mixed);
    CHECK(sp.stats.h2d_bytes == t.h2d);
    CHECK(sp.stats.d2h_bytes == t.d2h);
    if (sp.stats.h2d_bytes != t.h2d || sp.stats.d2h_bytes != t.d2h)
        std::fprintf(stderr, "h2d %llu (want %llu), d2h %llu (want %llu)\n", (unsigned long long)sp.stats.h2d_bytes,
                     (unsigned long long)t.h2d, (unsigned long long)sp.stats.d2h_bytes, (unsigned long long)t.d2h);
}

// A connection to `srv`: the rounds in `patterns`, then the stats.
static void serve_rounds(srpc::gpu::batch_server& srv, route rt, bool string_methods,
                         std::vector<const char*> const& patterns, const char* cpu_kinds = "u") {
    served_socketpair sp(srv);
    timeval tv{30, 0};  // a server that never answers fails the round instead of hanging it
    setsockopt(sp.fd, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof tv);
    tally t;
    bool right = true;
    for (const char* p : patterns) right = right && exchange(sp.fd, t, rt, string_methods, p, cpu_kinds);
    CHECK(right);
    sp.finish();
    check_stats(sp, t);
}

static void clear_seen() { g_square = g_sub = g_add = g_echo = g_twice = g_whole = g_whole_var = seen{}; }

// ---- (a), (b), (c): the bucket route with all three kinds of method, served again and again ----

static void one_server_methods_added() {
    clear_seen();
    srpc::gpu::batch_server srv(kMax);
    srv.register_method<Number, Number>(kSquare, square_cols);
    srv.register_record_method<TwoNumbers, Number>(kAdd, add_records);
    srv.register_var_method<MP, MP>(kEcho, echo_strings);
    // every kind with unknown frames; fixed only; fixed and unknown; strings without unknown; one method's frames alone
    serve_rounds(srv, route::bucket, true,
                 {"qaeuqaeuqqaaeeuu", "qqqqaaaaqqqqaaaa", "qaqaqaqauuuuqaqa", "qeqeqeqeaaaaeeee", "qqqqqqqqqqqqqqqq"});
    CHECK(g_square.warm == 2 && g_add.warm == 4 && g_echo.warm == 2);
    CHECK(g_square.batches == 5 && g_add.batches == 4 && g_echo.batches == 2);
    // nothing changed: served again without a warm-up
    serve_rounds(srv, route::bucket, true, {"qaeuqaeuqaeuqaeu", "sqsqsqsqaeaeaeae"}, "su");  // subtract: nobody's yet
    CHECK(g_square.warm == 2 && g_add.warm == 4 && g_echo.warm == 2 && g_sub.warm == 0 && g_sub.batches == 0);
    CHECK(g_square.batches == 7);
    // one more column method: the buffers are built again, every handler warmed up again
    srv.register_method<TwoNumbers, Number>(kSub, sub_cols);
    serve_rounds(srv, route::bucket, true, {"sqsqsqsqaeaeaeae", "qasuqasuqqaasseu"});  // ... now the GPU's
    CHECK(g_square.warm == 4 && g_add.warm == 8 && g_echo.warm == 4 && g_sub.warm == 2);
    CHECK(g_square.batches == 9 && g_sub.batches == 2);
}

// ---- (a), (b), (c): one server through the bucket, ordered, ordered_var and bucket routes ----

static void one_server_modes_changed() {
    clear_seen();
    srpc::gpu::batch_server srv(kMax);
    srv.register_method<Number, Number>(kSquare, square_cols);
    srv.register_method<TwoNumbers, Number>(kSub, sub_cols);
    const std::vector<const char*> fixed = {"qsqsqsqsqqqqssss", "qsuuqsuuqsuuqsuu", "qqqqqqqqqqqqqqqq", "quuuuuuuuuuuuuus"};
    serve_rounds(srv, route::bucket, false, fixed);
    CHECK(g_square.warm == 2 && g_sub.warm == 2 && g_square.batches == 4 && g_sub.batches == 3);
    srv.set_ordered(true);
    CHECK(srv.ordered() && !srv.ordered_var());
    serve_rounds(srv, route::ordered, false, fixed);
    CHECK(g_square.warm == 4 && g_sub.warm == 4 && g_square.batches == 8 && g_sub.batches == 6);
    serve_rounds(srv, route::ordered, false, {"qsqsqsqsqsqsqsqs"});  // no change, no warm-up
    CHECK(g_square.warm == 4 && g_sub.warm == 4 && g_square.batches == 9);
    srv.register_var_method<MP, MP>(kEcho, echo_strings);
    srv.set_ordered_var(true);
    CHECK(srv.ordered() && srv.ordered_var());
    const std::vector<const char*> strings = {"qseuqseuqqsseeuu", "qsqsqsqsqqqqssss", "qsqsqsqsuuuuqsqs", "qeqeqeqesssseeee",
                                              "qeeeeeeeeeeeeeee"};
    serve_rounds(srv, route::ordered_var, true, strings);
    CHECK(g_square.warm == 6 && g_sub.warm == 6 && g_echo.warm == 2);
    CHECK(g_square.batches == 14 && g_echo.batches == 3);
    srv.set_ordered(false);  // leaves both ordered modes: the bucket route, now with a string method
    CHECK(!srv.ordered() && !srv.ordered_var());
    serve_rounds(srv, route::bucket, true, strings);
    CHECK(g_square.warm == 8 && g_sub.warm == 8 && g_echo.warm == 4);
    CHECK(g_square.batches == 19 && g_echo.batches == 6);
}

// ---- (c) the whole-batch handlers' warm-up: a batch of one unknown frame, twice ----

static void whole_batch_handlers_warm_up() {
    clear_seen();
    srpc::gpu::batch_server srv(kMax);
    srv.register_method<Number, Number>(kSquare, square_cols);
    srv.set_ordered_handler(whole_batch);
    serve_rounds(srv, route::ordered, false, {});
    CHECK(g_whole.warm == 2 && g_square.warm == 0);
    serve_rounds(srv, route::ordered, false, {});
    CHECK(g_whole.warm == 2);
    srv.set_ordered_var_handler(whole_var_batch);
    serve_rounds(srv, route::ordered_var, false, {});
    CHECK(g_whole_var.warm == 2 && g_whole.warm == 2 && g_square.warm == 0);
}

// ---- (d) the bucket route's overflow demotion ----

// The CPU server's method: what the GPU side hands over when twice overflows.
struct Text_servicer : srpc::servicer_base {
    TwoTexts twice_(Text& q) { return twice(q); }
    static constexpr const char* name = "Text";
    static constexpr auto methods = std::make_tuple(STRUCT_MEMBER(Text_servicer, twice_, "Text_servicer::twice"));
};

static void overflowing_bucket_is_answered_on_the_cpu() {
    clear_seen();
    g_overflowing = 0;
    Text_servicer text;
    srpc::server cpu;
    cpu.register_service(text);
    srpc::gpu::batch_server srv(kMax, 0, &cpu);
    srv.register_method<Number, Number>(kSquare, square_cols);
    srv.register_record_method<TwoNumbers, Number>(kAdd, add_records);
    srpc::gpu::var_limits small;
    small.max_response_chars = 2;  // each response column: 16 * 2 + 16 = 48 bytes
    srv.register_var_method<Text, TwoTexts>(kTwice, twice_clipped, small);
    served_socketpair sp(srv);
    timeval tv{30, 0};
    setsockopt(sp.fd, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof tv);
    tally t;
    bool right = true;
    // four answers of 60 chars: past the column, the bucket goes to the CPU server, frame by frame in place
    right = right && exchange(sp.fd, t, route::bucket, true, "qatuqatuqatuqatu", "tu", 30);
    // one answer of 6 and 4 chars: fits, from the GPU
    right = right && exchange(sp.fd, t, route::bucket, true, "qqqqaaaatuqaqaqa", "u", 3);
    // overflowing again, no other unknown frame in the batch
    right = right && exchange(sp.fd, t, route::bucket, true, "ttttttttqqqqaaaa", "t", 30);
    // every frame the overflowing method's: nothing left for the GPU
    right = right && exchange(sp.fd, t, route::bucket, true, "tttttttttttttttt", "t", 30);
    right = right && exchange(sp.fd, t, route::bucket, true, "qaqaqaqaqaqaqaqu");
    CHECK(right);
    sp.finish();
    check_stats(sp, t);
    CHECK(g_overflowing == 3 && sp.stats.overflow_batches == g_overflowing);
    CHECK(g_twice.warm == 2 && g_twice.batches == 4);
    CHECK(g_square.batches == 4 && g_add.batches == 4);
}

int main() {
    // what a generated stub does: the CPU server finds its argument types by name
    srpc::message_registry["Text"] = []() -> std::unique_ptr<Text> { return std::make_unique<Text>(); };
    one_server_methods_added();
    one_server_modes_changed();
    whole_batch_handlers_warm_up();
    overflowing_bucket_is_answered_on_the_cpu();
    std::printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
