// needs: gpu
// srpc::gpu::batch_server in ordered mode (include/srpc/gpu_server.hpp:
// set_ordered, set_ordered_handler) with srpc::gpu::batch_client::call_mixed as
// the peer on the other end of a socketpair:
//   (a) a stateful accumulator, acc_add / acc_mul, served by one ordered
//       handler that walks every batch serially by d_method / d_rank with its
//       running value in device memory: every reply equals the host's serial
//       replay of the sent trace;
//   (b) per-method handlers in ordered mode: handler k receives exactly the
//       requests of method k in arrival order;
//   (c) 10 % frames of a method only the CPU fallback server knows: answered in
//       their places;
//   (d) ordered mode with a string-bodied method: SRPC_E_UNSUPPORTED;
//   (e) ordered mode off on a single-method stream: the bucket route's stats
//       and reply bytes (and the ordered route's replies are the same bytes).
// The handlers work through the host (this program is host code): they wait for
// the server's stream, copy the batch's columns out, compute, and copy back.
#include <hip/hip_runtime_api.h>
#include <srpc/gpu_client.hpp>
#include <srpc/gpu_server.hpp>
#include <srpc/packer.hpp>
#include <sys/socket.h>
#include <unistd.h>

#include <array>
#include <cstdio>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>

#include "served_socketpair.hpp"

static int g_fail = 0, g_pass = 0;
#define CHECK(c)                                                                    \
    do {                                                                            \
        if (c) ++g_pass;                                                            \
        else { ++g_fail; std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); } \
    } while (0)
#define HIPCHECK(x)                                                                 \
    do {                                                                            \
        hipError_t e_ = (x);                                                        \
        if (e_ != hipSuccess) { std::fprintf(stderr, "HIP %s at %d\n", hipGetErrorString(e_), __LINE__); std::exit(2); } \
    } while (0)

struct Number : public srpc::message_base {
    int32_t num = 0;
    static constexpr const char* name = "Number";
    static constexpr auto fields = std::make_tuple(STRUCT_MEMBER(Number, num, "Number::num"));
    void unpack(srpc::buffer::ptr bp) override { srpc::packer p(bp); p >> num; }
};

struct TwoNumbers : public srpc::message_base {
    int32_t left = 0, right = 0;
    static constexpr const char* name = "TwoNumbers";
    static constexpr auto fields = std::make_tuple(STRUCT_MEMBER(TwoNumbers, left, "TwoNumbers::left"),
                                                   STRUCT_MEMBER(TwoNumbers, right, "TwoNumbers::right"));
    void unpack(srpc::buffer::ptr bp) override { srpc::packer p(bp); p >> left >> right; }
};

struct Wide : public srpc::message_base {
    int64_t v = 0;
    static constexpr const char* name = "Wide";
    static constexpr auto fields = std::make_tuple(STRUCT_MEMBER(Wide, v, "Wide::v"));
    void unpack(srpc::buffer::ptr bp) override { srpc::packer p(bp); p >> v; }
};

struct Text : public srpc::message_base {
    std::string s;
    static constexpr const char* name = "Text";
    static constexpr auto fields = std::make_tuple(STRUCT_MEMBER(Text, s, "Text::s"));
    void unpack(srpc::buffer::ptr bp) override { srpc::packer p(bp); p >> s; }
};

constexpr uint64_t kBatch = 1024;  // both sides: several batches, both staging slots
static const std::array<std::string, 5> kCalc = {"Calculator_servicer::square", "Calculator_servicer::add",
                                                 "Calculator_servicer::subtract", "Calculator_servicer::multiply",
                                                 "Calculator_servicer::divide"};

// two's-complement arithmetic without signed overflow
static int32_t compute(int op, int32_t l, int32_t r) {
    const uint32_t a = static_cast<uint32_t>(l), b = static_cast<uint32_t>(r);
    const uint32_t v = op == 0 ? a * a : op == 1 ? a + b : op == 2 ? a - b : op == 3 ? a * b : a ^ b;
    return static_cast<int32_t>(v);
}

// The CPU server's only method: what the GPU side does not register.
struct Divider_servicer : srpc::servicer_base {
    Number divide(TwoNumbers& q) {
        Number r;
        r.num = compute(4, q.left, q.right);
        return r;
    }
    static constexpr const char* name = "Calculator";
    static constexpr auto methods = std::make_tuple(STRUCT_MEMBER(Divider_servicer, divide, "Calculator_servicer::divide"));
};

// A batch_server on one end of a socketpair, on a thread.
struct served_pair : served_socketpair {
    explicit served_pair(std::function<void(srpc::gpu::batch_server&)> setup, srpc::server* fallback = nullptr)
        : served_socketpair(kBatch, std::move(setup), fallback) {}
};

static uint64_t mix64(uint64_t x) {
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// ---- (a) the accumulator ---------------------------------------------------------------------

static int64_t* g_d_state = nullptr;  // the service's running value, in device memory across batches
static uint64_t g_acc_batches = 0;

static int64_t acc_step(int64_t state, int k, int64_t v) {
    const uint64_t a = static_cast<uint64_t>(state), b = static_cast<uint64_t>(v);
    return static_cast<int64_t>(k == 0 ? a + b : a * b);
}

// One handler for both methods: the batch walked serially in arrival order.
static int acc_handler(srpc::gpu::ordered_batch const& b, hipStream_t s) {
    if (hipStreamSynchronize(s) != hipSuccess) return SRPC_E_HIP;
    if (b.methods != 2) return SRPC_E_INVALID;
    std::vector<uint8_t> method(b.n);
    std::vector<uint32_t> rank(b.n);
    std::array<std::vector<int64_t>, 2> in, out;
    if (hipMemcpy(method.data(), b.d_method, b.n, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    if (hipMemcpy(rank.data(), b.d_rank, 4 * b.n, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    for (int k = 0; k < 2; ++k) {
        in[k].resize(b.counts[k]);
        out[k].resize(b.counts[k]);
        if (b.counts[k] &&
            hipMemcpy(in[k].data(), b.req_cols[k][0], 8 * b.counts[k], hipMemcpyDeviceToHost) != hipSuccess)
            return SRPC_E_HIP;
    }
    int64_t state = 0;
    if (hipMemcpy(&state, g_d_state, 8, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    uint64_t seen = 0;
    for (uint64_t i = 0; i < b.n; ++i) {
        const int k = method[i];
        if (k == SRPC_FRAME_UNKNOWN) {
            if (rank[i] != 0xffffffffu) return SRPC_E_INVALID;
            continue;
        }
        if (k > 1 || rank[i] >= b.counts[k]) return SRPC_E_INVALID;
        state = acc_step(state, k, in[k][rank[i]]);
        out[k][rank[i]] = state;
        ++seen;
    }
    if (seen != b.counts[0] + b.counts[1] || seen + b.counts[2] != b.n) return SRPC_E_INVALID;
    for (int k = 0; k < 2; ++k)
        if (b.counts[k] &&
            hipMemcpy(b.resp_cols[k][0], out[k].data(), 8 * b.counts[k], hipMemcpyHostToDevice) != hipSuccess)
            return SRPC_E_HIP;
    if (seen) ++g_acc_batches;
    return hipMemcpy(g_d_state, &state, 8, hipMemcpyHostToDevice) == hipSuccess ? 0 : SRPC_E_HIP;
}

static void stateful_accumulator() {
    constexpr uint64_t n = 5000;
    const int64_t start = 3;
    HIPCHECK(hipMalloc(reinterpret_cast<void**>(&g_d_state), 8));
    HIPCHECK(hipMemcpy(g_d_state, &start, 8, hipMemcpyHostToDevice));
    g_acc_batches = 0;
    served_pair sp([](srpc::gpu::batch_server& s) {
        s.register_method<Wide, Wide>("Acc_servicer::acc_add", nullptr);
        s.register_method<Wide, Wide>("Acc_servicer::acc_mul", nullptr);
        s.set_ordered_handler(acc_handler);
    });
    // the trace: random order over the two methods, per-method columns in rank order
    std::vector<uint8_t> method(n);
    std::array<std::vector<int64_t>, 2> arg;
    std::vector<int64_t> want(n);
    int64_t state = start;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t x = mix64(i);
        method[i] = static_cast<uint8_t>((x >> 40) & 1);
        const int64_t v = static_cast<int64_t>(mix64(x) | 1);  // odd factors: the value never collapses to 0
        arg[method[i]].push_back(v);
        state = acc_step(state, method[i], v);
        want[i] = state;
    }
    std::array<void*, 2> d_arg{}, d_out{};
    for (int k = 0; k < 2; ++k) {
        const uint64_t c = arg[k].size();
        HIPCHECK(hipMalloc(&d_arg[k], 8 * c + 16));
        HIPCHECK(hipMalloc(&d_out[k], 8 * c + 16));
        HIPCHECK(hipMemcpy(d_arg[k], arg[k].data(), 8 * c, hipMemcpyHostToDevice));
        HIPCHECK(hipMemset(d_out[k], 0xA5, 8 * c + 16));
    }
    uint8_t *d_method = nullptr, *d_codes = nullptr;
    HIPCHECK(hipMalloc(reinterpret_cast<void**>(&d_method), n + 16));
    HIPCHECK(hipMalloc(reinterpret_cast<void**>(&d_codes), n + 16));
    HIPCHECK(hipMemcpy(d_method, method.data(), n, hipMemcpyHostToDevice));
    HIPCHECK(hipMemset(d_codes, 0xA5, n + 16));
    {
        srpc::gpu::batch_client cl(sp.fd, kBatch);
        std::vector<srpc::gpu::mixed_leg> legs;
        legs.push_back(cl.leg<Wide, Wide>("Acc_servicer::acc_add", &d_arg[0], &d_out[0], arg[0].size()));
        legs.push_back(cl.leg<Wide, Wide>("Acc_servicer::acc_mul", &d_arg[1], &d_out[1], arg[1].size()));
        const srpc::gpu::call_stats st = cl.call_mixed(legs, d_method, n, d_codes);
        CHECK(st.calls == n && st.ok == n && st.chunks == 5);
    }
    std::array<std::vector<int64_t>, 2> out;
    std::vector<uint8_t> codes(n);
    for (int k = 0; k < 2; ++k) {
        out[k].resize(arg[k].size());
        HIPCHECK(hipMemcpy(out[k].data(), d_out[k], 8 * out[k].size(), hipMemcpyDeviceToHost));
    }
    HIPCHECK(hipMemcpy(codes.data(), d_codes, n, hipMemcpyDeviceToHost));
    bool right = true;
    uint64_t rank[2] = {0, 0};
    for (uint64_t i = 0; i < n; ++i) {
        const int k = method[i];
        right = right && codes[i] == srpc::RPC_SUCCESS && out[k][rank[k]++] == want[i];
    }
    CHECK(right);
    CHECK(arg[0].size() > 1000 && arg[1].size() > 1000);
    sp.finish();
    CHECK(sp.thrown == 0 && sp.stats.requests == n && sp.stats.gpu_requests == n && sp.stats.fallback_requests == 0);
    CHECK(sp.stats.gpu_batches >= 5 && sp.stats.gpu_batches == g_acc_batches);
    CHECK(sp.stats.mixed_batches >= 4 && sp.stats.mixed_batches <= sp.stats.gpu_batches);
    int64_t end = 0;
    HIPCHECK(hipMemcpy(&end, g_d_state, 8, hipMemcpyDeviceToHost));
    CHECK(end == want[n - 1]);
    for (int k = 0; k < 2; ++k) {
        (void)hipFree(d_arg[k]);
        (void)hipFree(d_out[k]);
    }
    (void)hipFree(d_method);
    (void)hipFree(d_codes);
    (void)hipFree(g_d_state);
}

// ---- (b), (c), (e): the calculator ------------------------------------------------------------

// Every request column each per-method handler was given, batch after batch.
static std::array<std::vector<int32_t>, 4> g_seen_left, g_seen_right;

// A device method of the test server, through the host; it keeps what it saw.
// Sent values are never 0, so the one all-zero record each handler is run on
// at serve start (the warm-up) is told apart and left out.
template <int OP>
static int method_batch(void* const* rq, void* const* rs, uint64_t n, hipStream_t s) {
    std::vector<int32_t> l(n), r(n), out(n);
    if (hipStreamSynchronize(s) != hipSuccess) return SRPC_E_HIP;
    if (hipMemcpy(l.data(), rq[0], 4 * n, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    if (OP != 0 && hipMemcpy(r.data(), rq[1], 4 * n, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    const bool warm_up = n == 1 && l[0] == 0;
    for (uint64_t i = 0; i < n; ++i) out[i] = compute(OP, l[i], r[i]);
    if (!warm_up) {
        g_seen_left[OP].insert(g_seen_left[OP].end(), l.begin(), l.end());
        g_seen_right[OP].insert(g_seen_right[OP].end(), r.begin(), r.end());
    }
    return hipMemcpy(rs[0], out.data(), 4 * n, hipMemcpyHostToDevice) == hipSuccess ? 0 : SRPC_E_HIP;
}

static void register_calc(srpc::gpu::batch_server& s, int methods) {
    s.register_method<Number, Number>(kCalc[0], method_batch<0>);
    if (methods > 1) s.register_method<TwoNumbers, Number>(kCalc[1], method_batch<1>);
    if (methods > 2) s.register_method<TwoNumbers, Number>(kCalc[2], method_batch<2>);
    if (methods > 3) s.register_method<TwoNumbers, Number>(kCalc[3], method_batch<3>);
}

static int32_t value(uint64_t i) { return static_cast<int32_t>(static_cast<uint32_t>(mix64(i)) | 1u); }  // never 0

// n calls over the first `legs` calculator methods; `rare` > 0: leg 4 (divide)
// takes one call in `rare`, the four others share the rest.
struct calc_calls {
    uint64_t n;
    int nlegs;
    std::vector<uint8_t> method, hcodes;
    std::vector<uint32_t> rank;
    std::array<uint64_t, 5> count{};
    std::array<std::vector<int32_t>, 5> left, right, out;
    std::array<void*, 5> d_left{}, d_right{}, d_out{};
    std::array<std::array<void*, 2>, 5> req_cols{};
    uint8_t *d_method = nullptr, *d_codes = nullptr;

    calc_calls(uint64_t n, int nlegs, uint64_t rare = 0) : n(n), nlegs(nlegs), method(n), hcodes(n), rank(n) {
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t x = mix64(i + 77);
            method[i] = rare ? static_cast<uint8_t>(x % rare == 0 ? 4 : (x >> 20) % 4) : static_cast<uint8_t>(x % nlegs);
            rank[i] = static_cast<uint32_t>(count[method[i]]++);
        }
        for (int k = 0; k < nlegs; ++k) {
            const uint64_t c = count[k];
            left[k].resize(c), right[k].resize(c), out[k].resize(c);
            for (uint64_t r = 0; r < c; ++r) left[k][r] = value(r * 5 + k), right[k][r] = value(r * 31 + 7 * k + 1000003);
            HIPCHECK(hipMalloc(&d_left[k], 4 * c + 16));
            HIPCHECK(hipMalloc(&d_right[k], 4 * c + 16));
            HIPCHECK(hipMalloc(&d_out[k], 4 * c + 16));
            HIPCHECK(hipMemcpy(d_left[k], left[k].data(), 4 * c, hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(d_right[k], right[k].data(), 4 * c, hipMemcpyHostToDevice));
            HIPCHECK(hipMemset(d_out[k], 0xA5, 4 * c + 16));
            req_cols[k] = {d_left[k], d_right[k]};
        }
        HIPCHECK(hipMalloc(reinterpret_cast<void**>(&d_method), n + 16));
        HIPCHECK(hipMalloc(reinterpret_cast<void**>(&d_codes), n + 16));
        HIPCHECK(hipMemcpy(d_method, method.data(), n, hipMemcpyHostToDevice));
        HIPCHECK(hipMemset(d_codes, 0xA5, n + 16));
    }
    std::vector<srpc::gpu::mixed_leg> legs(srpc::gpu::batch_client& cl) {
        std::vector<srpc::gpu::mixed_leg> l;
        l.push_back(cl.leg<Number, Number>(kCalc[0], req_cols[0].data(), &d_out[0], count[0]));
        for (int k = 1; k < nlegs; ++k)
            l.push_back(cl.leg<TwoNumbers, Number>(kCalc[k], req_cols[k].data(), &d_out[k], count[k]));
        return l;
    }
    void fetch() {
        for (int k = 0; k < nlegs; ++k) HIPCHECK(hipMemcpy(out[k].data(), d_out[k], 4 * count[k], hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(hcodes.data(), d_codes, n, hipMemcpyDeviceToHost));
    }
    bool all_right() const {
        bool ok = true;
        for (uint64_t i = 0; i < n; ++i) {
            const int k = method[i];
            const uint32_t r = rank[i];
            ok = ok && hcodes[i] == srpc::RPC_SUCCESS && out[k][r] == compute(k, left[k][r], right[k][r]);
        }
        return ok;
    }
    ~calc_calls() {
        for (int k = 0; k < nlegs; ++k) {
            (void)hipFree(d_left[k]);
            (void)hipFree(d_right[k]);
            (void)hipFree(d_out[k]);
        }
        (void)hipFree(d_method);
        (void)hipFree(d_codes);
    }
};

static void clear_seen() {
    for (int k = 0; k < 4; ++k) g_seen_left[k].clear(), g_seen_right[k].clear();
}

static void per_method_handlers_see_arrival_order() {
    constexpr uint64_t n = 5000;
    clear_seen();
    served_pair sp([](srpc::gpu::batch_server& s) {
        register_calc(s, 4);
        s.set_ordered(true);
    });
    calc_calls d(n, 4);
    {
        srpc::gpu::batch_client cl(sp.fd, kBatch);
        const srpc::gpu::call_stats st = cl.call_mixed(d.legs(cl), d.d_method, n, d.d_codes);
        CHECK(st.ok == n && st.chunks == 5);
    }
    d.fetch();
    CHECK(d.all_right());
    sp.finish();
    // the client's columns are each method's calls in the order they were sent
    for (int k = 0; k < 4; ++k) {
        CHECK(d.count[k] > 1000);
        CHECK(g_seen_left[k] == d.left[k]);
        if (k) CHECK(g_seen_right[k] == d.right[k]);
    }
    CHECK(sp.thrown == 0 && sp.stats.requests == n && sp.stats.gpu_requests == n);
    CHECK(sp.stats.gpu_batches >= 5 && sp.stats.mixed_batches >= 4 && sp.stats.mixed_batches <= sp.stats.gpu_batches);
}

static void unknown_frames_answered_in_place() {
    constexpr uint64_t n = 5000;
    clear_seen();
    Divider_servicer div;
    srpc::server cpu;
    cpu.register_service(div);
    served_pair sp(
        [](srpc::gpu::batch_server& s) {
            register_calc(s, 4);
            s.set_ordered(true);
        },
        &cpu);
    calc_calls d(n, 5, 10);
    {
        srpc::gpu::batch_client cl(sp.fd, kBatch);
        const srpc::gpu::call_stats st = cl.call_mixed(d.legs(cl), d.d_method, n, d.d_codes);
        CHECK(st.ok == n && st.failed == 0 && st.malformed == 0 && st.unanswered == 0);
    }
    d.fetch();
    CHECK(d.all_right());  // leg 4's replies are the CPU server's, each in its place
    CHECK(d.count[4] > n / 20 && d.count[4] < n / 5);
    sp.finish();
    for (int k = 0; k < 4; ++k) CHECK(g_seen_left[k] == d.left[k]);
    CHECK(sp.thrown == 0 && sp.stats.requests == n);
    CHECK(sp.stats.fallback_requests == d.count[4] && sp.stats.gpu_requests == n - d.count[4]);
    CHECK(sp.stats.fallback_requests + sp.stats.gpu_requests == n);
}

static int never_var(srpc::gpu::var_batch const&, hipStream_t) { return SRPC_E_INVALID; }

static void ordered_refuses_string_methods() {
    served_pair sp([](srpc::gpu::batch_server& s) {
        register_calc(s, 1);
        s.register_var_method<Text, Text>("Text_servicer::echo", never_var);
        s.set_ordered(true);
    });
    sp.finish();
    CHECK(sp.thrown == SRPC_E_UNSUPPORTED);
    // ... whichever came first
    served_pair sq([](srpc::gpu::batch_server& s) {
        s.set_ordered_handler([](srpc::gpu::ordered_batch const&, hipStream_t) { return 0; });
        s.register_var_method<Text, Text>("Text_servicer::echo", never_var);
    });
    sq.finish();
    CHECK(sq.thrown == SRPC_E_UNSUPPORTED);
}

// One method, ordered off and on: the same calls, the same answers, the same
// byte counts; off, the stats are the bucket route's on a stream of one method
// (no batch needs a gather).
static void single_method_stream_both_routes() {
    constexpr uint64_t n = 3000;
    uint64_t received[2] = {0, 0};
    for (int ordered = 0; ordered < 2; ++ordered) {
        clear_seen();
        served_pair sp([ordered](srpc::gpu::batch_server& s) {
            register_calc(s, 1);
            s.set_ordered(ordered != 0);
            if (s.ordered() != (ordered != 0)) std::exit(3);
        });
        calc_calls d(n, 1);
        {
            srpc::gpu::batch_client cl(sp.fd, kBatch);
            const srpc::gpu::call_stats st = cl.call_mixed(d.legs(cl), d.d_method, n, d.d_codes);
            CHECK(st.ok == n && st.sent_bytes == n * 57);
            received[ordered] = st.received_bytes;
        }
        d.fetch();
        CHECK(d.all_right());
        sp.finish();
        CHECK(g_seen_left[0] == d.left[0]);
        CHECK(sp.thrown == 0 && sp.stats.requests == n && sp.stats.gpu_requests == n);
        CHECK(sp.stats.fallback_requests == 0 && sp.stats.mixed_batches == 0 && sp.stats.gpu_batches >= 3);
        CHECK(sp.stats.h2d_bytes == n * 57 + 4 * n && sp.stats.d2h_bytes == n * 23);
    }
    CHECK(received[0] == n * 23 && received[1] == received[0]);
}

int main() {
    // what a generated stub does: the CPU server finds its argument types by name
    srpc::message_registry["Number"] = [] { return std::make_unique<Number>(); };
    srpc::message_registry["TwoNumbers"] = [] { return std::make_unique<TwoNumbers>(); };
    stateful_accumulator();
    per_method_handlers_see_arrival_order();
    unknown_frames_answered_in_place();
    ordered_refuses_string_methods();
    single_method_stream_both_routes();
    std::printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
