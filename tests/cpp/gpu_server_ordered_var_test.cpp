// needs: gpu
// srpc::gpu::batch_server in ordered mode with string-bodied methods
// (include/srpc/gpu_server.hpp: set_ordered_var, set_ordered_var_handler) with
// srpc::gpu::batch_client::call_mixed over leg_var legs as the peer on the other
// end of a socketpair:
//   (a) per-method handlers over seven methods -- two fixed, echo (strings on both
//       sides), twice (a string to two strings), divide (fixed), length (Text ->
//       Number) and spell (Number -> Text): every reply is the service's answer,
//       and every handler saw exactly its method's requests in arrival order;
//   (b) a stateful journal, append (Text -> Number) and bump (Number -> Text),
//       served by one ordered handler that walks every batch serially by d_method
//       / d_rank with its running value in device memory: every reply equals the
//       host's serial replay of the sent trace, across the two methods;
//   (c) three methods nobody registered: answered in their places with
//       RPC_ERR_FUNCTION_NOT_REGISTERED, the registered ones still in order;
//   (d) a string method whose responses do not fit its columns: answered by the
//       CPU server for those batches, in place (overflow_batches), the other
//       methods still from the GPU;
//   (e) set_ordered / set_ordered_handler keep refusing string methods, and
//       set_ordered(false) leaves the route.
// The handlers work through the host (this program is host code): they wait for
// the server's stream, copy the batch's columns out, compute, and copy back.
// The messages, columns and reply checks are mixed_var_fixture.hpp's.
#include "mixed_var_fixture.hpp"
#include "served_socketpair.hpp"

#include <srpc/server.hpp>

constexpr uint64_t kSrvBatch = 1024;  // both sides: several batches per call

// A batch_server on one end of a socketpair, on a thread.
struct ordered_pair : served_socketpair {
    explicit ordered_pair(std::function<void(srpc::gpu::batch_server&)> setup, srpc::server* fallback = nullptr)
        : served_socketpair(kSrvBatch, std::move(setup), fallback) {}
};

// ---- (a), (c): per-method handlers that keep what they saw ------------------------------------

static std::vector<int32_t> g_seen_square, g_seen_spell;
static std::vector<MP> g_seen_echo;
static std::vector<std::string> g_seen_twice, g_seen_length;

static void clear_seen() {
    g_seen_square.clear(), g_seen_spell.clear(), g_seen_echo.clear(), g_seen_twice.clear(), g_seen_length.clear();
}

// The one zero record every handler is run on at serve start is left out.  A
// real batch of exactly one all-zero request would be left out with it and fail
// the comparison below (same_order counts what was seen), not pass it.
static int square_seen(void* const* rq, void* const* rs, uint64_t n, hipStream_t s) {
    if (int rc = calc_batch<0>(rq, rs, n, s)) return rc;
    std::vector<int32_t> v(n);
    if (hipMemcpy(v.data(), rq[0], 4 * n, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    if (!(n == 1 && v[0] == 0)) g_seen_square.insert(g_seen_square.end(), v.begin(), v.end());
    return 0;
}
static int zero_batch(void* const*, void* const* rs, uint64_t n, hipStream_t s) {  // divide: answered with a zero
    return hipMemsetAsync(rs[0], 0, 4 * n, s) == hipSuccess ? 0 : SRPC_E_HIP;
}
static int echo_seen(srpc::gpu::var_batch const& b, hipStream_t s) {
    const bool warm = b.n == 1;
    return var_through_host<MP, MP>(b, s, [warm](MP const& q) {
        if (!(warm && zero(q))) g_seen_echo.push_back(q);
        return echo_fixture::answer(q);
    });
}
static int twice_seen(srpc::gpu::var_batch const& b, hipStream_t s) {
    const bool warm = b.n == 1;
    return var_through_host<Text, TwoTexts>(b, s, [warm](Text const& q) {
        if (!(warm && q.s.empty())) g_seen_twice.push_back(q.s);
        return twice(q);
    });
}
static int length_seen(srpc::gpu::var_batch const& b, hipStream_t s) {
    const bool warm = b.n == 1;
    return var_through_host<Text, Number>(b, s, [warm](Text const& q) {
        if (!(warm && q.s.empty())) g_seen_length.push_back(q.s);
        return length_of(q);
    });
}
static int spell_seen(srpc::gpu::var_batch const& b, hipStream_t s) {
    const bool warm = b.n == 1;
    return var_through_host<Number, Text>(b, s, [warm](Number const& q) {
        if (!(warm && q.num == 0)) g_seen_spell.push_back(q.num);
        return spell(q);
    });
}

static void register_known(srpc::gpu::batch_server& s, bool all) {
    s.register_method<Number, Number>(kMethods[0], square_seen);
    s.register_method<TwoNumbers, Number>(kMethods[1], calc_batch<1>);
    s.register_var_method<MP, MP>(kMethods[2], echo_seen);
    s.register_var_method<Text, TwoTexts>(kMethods[3], twice_seen);
    if (!all) return;
    s.register_method<TwoNumbers, Number>(kMethods[4], zero_batch);
    s.register_var_method<Text, Number>(kMethods[5], length_seen);
    s.register_var_method<Number, Text>(kMethods[6], spell_seen);
}

template <class T, class F>
static bool same_order(std::vector<T> const& seen, uint64_t count, F want) {
    if (seen.size() != count) return false;
    for (uint64_t r = 0; r < count; ++r)
        if (!want(seen[r], r)) return false;
    return true;
}

static void check_seen(mixed_calls const& d, bool all) {
    CHECK(same_order(g_seen_square, d.count[0], [&](int32_t v, uint64_t r) { return v == d.square.in[r].num; }));
    CHECK(same_order(g_seen_echo, d.count[2], [&](MP const& v, uint64_t r) { return same(v, d.echo.in[r]); }));
    CHECK(same_order(g_seen_twice, d.count[3], [&](std::string const& v, uint64_t r) { return v == d.text.in[r].s; }));
    if (!all) return;
    CHECK(same_order(g_seen_length, d.count[5], [&](std::string const& v, uint64_t r) { return v == d.length.in[r].s; }));
    CHECK(same_order(g_seen_spell, d.count[6], [&](int32_t v, uint64_t r) { return v == d.spelled.in[r].num; }));
}

static void per_method_handlers_see_arrival_order() {
    constexpr uint64_t n = 5000;
    clear_seen();
    ordered_pair sp([](srpc::gpu::batch_server& s) {
        register_known(s, true);
        s.set_ordered_var(true);
        if (!s.ordered_var() || !s.ordered()) std::exit(3);
    });
    mixed_calls d(n);
    {
        srpc::gpu::batch_client cl(sp.fd, kSrvBatch);
        const srpc::gpu::call_stats st = cl.call_mixed(d.legs(cl), d.d_method, n, d.d_codes, srpc::gpu::var_call_limits{});
        CHECK(st.calls == n && st.ok == n && st.chunks == 5);
    }
    check_replies(d, n, false);  // every method answered, divide with a zero
    for (int k = 0; k < kLegs; ++k) CHECK(d.count[k] > 500);
    sp.finish();
    check_seen(d, true);
    CHECK(sp.thrown == 0 && sp.stats.requests == n && sp.stats.gpu_requests == n && sp.stats.fallback_requests == 0);
    CHECK(sp.stats.gpu_batches >= 5 && sp.stats.mixed_batches >= 4 && sp.stats.overflow_batches == 0);
}

static void unknown_frames_answered_in_place() {
    constexpr uint64_t n = 5000;
    clear_seen();
    ordered_pair sp([](srpc::gpu::batch_server& s) {
        register_known(s, false);
        s.set_ordered_var(true);
    });
    mixed_calls d(n);
    {
        srpc::gpu::batch_client cl(sp.fd, kSrvBatch);
        const srpc::gpu::call_stats st = cl.call_mixed(d.legs(cl), d.d_method, n, d.d_codes, srpc::gpu::var_call_limits{});
        CHECK(st.calls == n && st.failed == d.count[4] + d.count[5] + d.count[6] && st.ok + st.failed == n);
    }
    check_replies(d, n, true);  // divide, length and spell: a bare RPC_ERR_FUNCTION_NOT_REGISTERED each, in its place
    sp.finish();
    check_seen(d, false);
    const uint64_t unknown = d.count[4] + d.count[5] + d.count[6];
    CHECK(sp.thrown == 0 && sp.stats.requests == n);
    CHECK(sp.stats.fallback_requests == unknown && sp.stats.gpu_requests == n - unknown);
}

// ---- (b) the journal --------------------------------------------------------------------------

static uint32_t* g_d_state = nullptr;  // the service's running value, in device memory across batches
static uint64_t g_journal_batches = 0;

static uint32_t journal_step(uint32_t state, int k, std::string const& s, int32_t num) {
    if (k == 0) {
        for (char c : s) state = state * 131u + static_cast<uint8_t>(c);
        return state + static_cast<uint32_t>(s.size());
    }
    return state * 31u + static_cast<uint32_t>(num);
}
static std::string journal_text(uint32_t state) { return std::string(state % 23, static_cast<char>('a' + state % 26)) + "."; }

// One handler for both methods: the batch walked serially in arrival order.
// Method 0 is append (Text -> Number), method 1 bump (Number -> Text).
static int journal_handler(srpc::gpu::ordered_var_batch const& b, hipStream_t s) {
    if (hipStreamSynchronize(s) != hipSuccess) return SRPC_E_HIP;
    if (b.methods != 2) return SRPC_E_INVALID;
    // the tables' shapes: offsets only where a leaf is a string
    if (!b.req_str_offs[0][0] || b.req_str_offs[1][0] || b.resp_str_offs[0][0] || !b.resp_str_offs[1][0]) return SRPC_E_INVALID;
    const uint64_t n0 = b.counts[0], n1 = b.counts[1];
    std::vector<uint8_t> method(b.n);
    std::vector<uint32_t> rank(b.n);
    if (hipMemcpy(method.data(), b.d_method, b.n, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    if (hipMemcpy(rank.data(), b.d_rank, 4 * b.n, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    std::vector<uint64_t> offs(n0 + 1, 0);
    std::vector<char> chars;
    std::vector<int32_t> nums(n1), out0(n0);
    if (n0) {
        if (hipMemcpy(offs.data(), b.req_str_offs[0][0], 8 * (n0 + 1), hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
        if (offs[0] != 0) return SRPC_E_INVALID;
        chars.resize(offs[n0]);
        if (!chars.empty() && hipMemcpy(chars.data(), b.req_cols[0][0], chars.size(), hipMemcpyDeviceToHost) != hipSuccess)
            return SRPC_E_HIP;
    }
    if (n1 && hipMemcpy(nums.data(), b.req_cols[1][0], 4 * n1, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    uint32_t state = 0;
    if (hipMemcpy(&state, g_d_state, 4, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    std::vector<std::string> out1(n1);
    uint64_t seen = 0;
    for (uint64_t i = 0; i < b.n; ++i) {
        const int k = method[i];
        if (k == SRPC_FRAME_UNKNOWN) {
            if (rank[i] != 0xffffffffu) return SRPC_E_INVALID;
            continue;
        }
        if (k > 1 || rank[i] >= b.counts[k]) return SRPC_E_INVALID;
        const uint32_t r = rank[i];
        if (k == 0) {
            state = journal_step(state, 0, std::string(chars.data() + offs[r], chars.data() + offs[r + 1]), 0);
            out0[r] = static_cast<int32_t>(state);
        } else {
            state = journal_step(state, 1, std::string(), nums[r]);
            out1[r] = journal_text(state);
        }
        ++seen;
    }
    if (seen != n0 + n1 || seen + b.counts[2] != b.n) return SRPC_E_INVALID;
    if (n0 && hipMemcpy(b.resp_cols[0][0], out0.data(), 4 * n0, hipMemcpyHostToDevice) != hipSuccess) return SRPC_E_HIP;
    if (n1) {
        std::vector<uint64_t> ro(n1 + 1, 0);
        std::string all;
        for (uint64_t r = 0; r < n1; ++r) all += out1[r], ro[r + 1] = all.size();
        if (all.size() > b.resp_cap[1][0]) return SRPC_E_CAPACITY;
        if (hipMemcpy(b.resp_cols[1][0], all.data(), all.size(), hipMemcpyHostToDevice) != hipSuccess) return SRPC_E_HIP;
        if (hipMemcpy(b.resp_str_offs[1][0], ro.data(), 8 * (n1 + 1), hipMemcpyHostToDevice) != hipSuccess) return SRPC_E_HIP;
    }
    if (seen) ++g_journal_batches;
    return hipMemcpy(g_d_state, &state, 4, hipMemcpyHostToDevice) == hipSuccess ? 0 : SRPC_E_HIP;
}

static void stateful_journal() {
    constexpr uint64_t n = 5000;
    const uint32_t start = 7;
    HIPCHECK(hipMalloc(reinterpret_cast<void**>(&g_d_state), 4));
    HIPCHECK(hipMemcpy(g_d_state, &start, 4, hipMemcpyHostToDevice));
    g_journal_batches = 0;
    ordered_pair sp([](srpc::gpu::batch_server& s) {
        s.register_var_method<Text, Number>("Journal_servicer::append", nullptr);
        s.register_var_method<Number, Text>("Journal_servicer::bump", nullptr);
        s.set_ordered_var_handler(journal_handler);
    });
    // the trace: a fixed pseudo-random order over the two methods, per-method columns in rank order
    std::vector<uint8_t> method(n);
    leg_data<Text, Number> append;
    leg_data<Number, Text> bump;
    std::vector<int32_t> want0;
    std::vector<std::string> want1;
    uint32_t state = start;
    uint64_t reply_chars = 0;
    uint32_t x = 88172645u;
    for (uint64_t i = 0; i < n; ++i) {
        x ^= x << 13, x ^= x >> 17, x ^= x << 5;
        method[i] = static_cast<uint8_t>((x >> 9) & 1);
        if (method[i] == 0) {
            MP m;
            echo_fixture::fill_request(m, i);
            Text t;
            t.s = m.arg4;
            append.in.push_back(t);
            state = journal_step(state, 0, t.s, 0);
            want0.push_back(static_cast<int32_t>(state));
        } else {
            Number v;
            v.num = value(i);
            bump.in.push_back(v);
            state = journal_step(state, 1, std::string(), v.num);
            want1.push_back(journal_text(state));
            reply_chars += want1.back().size();
        }
    }
    append.upload(0);
    bump.upload(reply_chars);  // exact: nothing to spare
    uint8_t *d_method = nullptr, *d_codes = nullptr;
    HIPCHECK(hipMalloc(reinterpret_cast<void**>(&d_method), n + 16));
    HIPCHECK(hipMalloc(reinterpret_cast<void**>(&d_codes), n + 16));
    HIPCHECK(hipMemcpy(d_method, method.data(), n, hipMemcpyHostToDevice));
    HIPCHECK(hipMemset(d_codes, 0xA5, n + 16));
    {
        srpc::gpu::batch_client cl(sp.fd, kSrvBatch);
        std::vector<srpc::gpu::mixed_leg> legs;
        legs.push_back(cl.leg_var<Text, Number>("Journal_servicer::append", append.req.data(), append.req_offs.data(),
                                                append.resp.data(), append.resp_offs.data(), append.cap.data(),
                                                append.in.size()));
        legs.push_back(cl.leg_var<Number, Text>("Journal_servicer::bump", bump.req.data(), bump.req_offs.data(),
                                                bump.resp.data(), bump.resp_offs.data(), bump.cap.data(), bump.in.size()));
        const srpc::gpu::call_stats st = cl.call_mixed(legs, d_method, n, d_codes, srpc::gpu::var_call_limits{});
        CHECK(st.calls == n && st.ok == n && st.chunks == 5);
    }
    std::vector<Number> got0;
    std::vector<Text> got1;
    CHECK(append.fetch(got0));
    CHECK(bump.fetch(got1));
    std::vector<uint8_t> codes(n);
    HIPCHECK(hipMemcpy(codes.data(), d_codes, n, hipMemcpyDeviceToHost));
    bool right = got0.size() == want0.size() && got1.size() == want1.size();
    for (uint64_t i = 0; i < n; ++i) right = right && codes[i] == srpc::RPC_SUCCESS;
    for (uint64_t r = 0; right && r < want0.size(); ++r) right = got0[r].num == want0[r];
    for (uint64_t r = 0; right && r < want1.size(); ++r) right = got1[r].s == want1[r];
    CHECK(right);
    CHECK(want0.size() > 1000 && want1.size() > 1000);
    sp.finish();
    CHECK(sp.thrown == 0 && sp.stats.requests == n && sp.stats.gpu_requests == n && sp.stats.fallback_requests == 0);
    CHECK(sp.stats.gpu_batches >= 5 && sp.stats.gpu_batches == g_journal_batches);
    uint32_t end = 0;
    HIPCHECK(hipMemcpy(&end, g_d_state, 4, hipMemcpyDeviceToHost));
    CHECK(end == state);
    (void)hipFree(d_method);
    (void)hipFree(d_codes);
    (void)hipFree(g_d_state);
}

// ---- (d) responses that do not fit ------------------------------------------------------------

// The CPU server's method: what the GPU side hands over when twice overflows.
struct Text_servicer : srpc::servicer_base {
    TwoTexts twice_(Text& q) { return twice(q); }
    static constexpr const char* name = "Text";
    static constexpr auto methods = std::make_tuple(STRUCT_MEMBER(Text_servicer, twice_, "Text_servicer::twice"));
};

static uint64_t g_overflowing = 0;

// twice with honest offsets and only the chars that fit: what a device handler
// that counts before it writes leaves behind.
static int twice_clipped(srpc::gpu::var_batch const& b, hipStream_t s) {
    if (hipStreamSynchronize(s) != hipSuccess) return SRPC_E_HIP;
    std::vector<uint64_t> offs(b.n + 1);
    if (hipMemcpy(offs.data(), b.req_str_offs[0], 8 * (b.n + 1), hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    std::vector<char> chars(offs[b.n]);
    if (!chars.empty() && hipMemcpy(chars.data(), b.req_cols[0], chars.size(), hipMemcpyDeviceToHost) != hipSuccess)
        return SRPC_E_HIP;
    std::string a, c;
    std::vector<uint64_t> oa(b.n + 1, 0), oc(b.n + 1, 0);
    for (uint64_t r = 0; r < b.n; ++r) {
        Text q;
        q.s.assign(chars.data() + offs[r], chars.data() + offs[r + 1]);
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

static void overflowing_method_is_answered_on_the_cpu() {
    constexpr uint64_t n = 5000;
    clear_seen();
    g_overflowing = 0;
    Text_servicer text;
    srpc::server cpu;
    cpu.register_service(text);
    ordered_pair sp(
        [](srpc::gpu::batch_server& s) {
            s.register_method<Number, Number>(kMethods[0], square_seen);
            s.register_method<TwoNumbers, Number>(kMethods[1], calc_batch<1>);
            s.register_var_method<MP, MP>(kMethods[2], echo_seen);
            srpc::gpu::var_limits small;
            small.max_response_chars = 2;  // a batch's answers average ~60 chars a field
            s.register_var_method<Text, TwoTexts>(kMethods[3], twice_clipped, small);
            s.register_method<TwoNumbers, Number>(kMethods[4], zero_batch);
            s.register_var_method<Text, Number>(kMethods[5], length_seen);
            s.register_var_method<Number, Text>(kMethods[6], spell_seen);
            s.set_ordered_var(true);
        },
        &cpu);
    mixed_calls d(n);
    {
        srpc::gpu::batch_client cl(sp.fd, kSrvBatch);
        const srpc::gpu::call_stats st = cl.call_mixed(d.legs(cl), d.d_method, n, d.d_codes, srpc::gpu::var_call_limits{});
        CHECK(st.calls == n && st.ok == n);
    }
    check_replies(d, n, false);  // twice's answers are the CPU server's, each in its place
    sp.finish();
    CHECK(same_order(g_seen_square, d.count[0], [&](int32_t v, uint64_t r) { return v == d.square.in[r].num; }));
    CHECK(same_order(g_seen_echo, d.count[2], [&](MP const& v, uint64_t r) { return same(v, d.echo.in[r]); }));
    CHECK(same_order(g_seen_spell, d.count[6], [&](int32_t v, uint64_t r) { return v == d.spelled.in[r].num; }));
    CHECK(sp.thrown == 0 && sp.stats.requests == n);
    CHECK(g_overflowing >= 5 && sp.stats.overflow_batches == g_overflowing);
    CHECK(sp.stats.fallback_requests == d.count[3] && sp.stats.gpu_requests == n - d.count[3]);
}

// ---- (e) the fixed-size ordered mode keeps its contract ---------------------------------------

static int never_var(srpc::gpu::var_batch const&, hipStream_t) { return SRPC_E_INVALID; }

static void ordered_without_var_still_refuses() {
    ordered_pair sp([](srpc::gpu::batch_server& s) {
        s.register_method<Number, Number>(kMethods[0], calc_batch<0>);
        s.register_var_method<Text, Text>("Text_servicer::echo", never_var);
        s.set_ordered(true);
        if (s.ordered_var()) std::exit(3);
    });
    sp.finish();
    CHECK(sp.thrown == SRPC_E_UNSUPPORTED);
    ordered_pair sq([](srpc::gpu::batch_server& s) {
        // (run at serve start on one empty request: its zeroed response offsets are one empty answer)
        s.register_var_method<Text, Text>("Text_servicer::echo", [](srpc::gpu::var_batch const&, hipStream_t) { return 0; });
        s.set_ordered_var(true);
        s.set_ordered(false);  // leaves the route altogether: the bucket route serves
        if (s.ordered_var() || s.ordered()) std::exit(3);
    });
    sq.finish();
    CHECK(sq.thrown == 0 && sq.stats.requests == 0);
}

int main() {
    // what a generated stub does: the CPU server finds its argument types by name
    srpc::message_registry["Text"] = []() -> std::unique_ptr<Text> { return std::make_unique<Text>(); };
    per_method_handlers_see_arrival_order();
    stateful_journal();
    unknown_frames_answered_in_place();
    overflowing_method_is_answered_on_the_cpu();
    ordered_without_var_still_refuses();
    std::printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
