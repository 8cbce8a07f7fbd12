// needs: gpu
// srpc::gpu::batch_client::call_mixed with struct-array legs (leg_records,
// include/srpc/gpu_client.hpp) against a srpc::gpu::batch_server with column
// and record methods on the two ends of a socketpair: an ordered batch of calls
// over the four Calculator methods, packed in call order from per-method arrays
// of the caller's own structs and decoded into per-method arrays of structs.
// Checked: every reply struct byte for byte (the leaves the host computes, every
// other byte the proto's) and every code; every tenth call rewritten to a method
// the server does not know (bare replies); the same calls through column legs
// (same values, same counts); a peer that closes five replies into the second
// chunk; the refusals.  `bench N` prints call_stats::gpu_seconds of N calls
// through record legs and through column legs.
#include <hip/hip_runtime_api.h>
#include <srpc/gpu_client.hpp>
#include <srpc/gpu_server.hpp>
#include <srpc/packer.hpp>
#include <sys/socket.h>
#include <unistd.h>

#include <array>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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
    int32_t num;
    static constexpr const char* name = "Number";
    static constexpr auto fields = std::make_tuple(STRUCT_MEMBER(Number, num, "Number::num"));
};

struct TwoNumbers : public srpc::message_base {
    int32_t left, right;
    static constexpr const char* name = "TwoNumbers";
    static constexpr auto fields = std::make_tuple(STRUCT_MEMBER(TwoNumbers, left, "TwoNumbers::left"),
                                                   STRUCT_MEMBER(TwoNumbers, right, "TwoNumbers::right"));
};

// 264 bytes: more than a reply struct may have
#define BIG_FIELDS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) \
    X(17) X(18) X(19) X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30)
struct Big : public srpc::message_base {
#define X(i) int64_t v##i;
    BIG_FIELDS(X) int64_t v31;
#undef X
    static constexpr const char* name = "Big";
#define X(i) STRUCT_MEMBER(Big, v##i, "Big::v" #i),
    static constexpr auto fields = std::make_tuple(BIG_FIELDS(X) STRUCT_MEMBER(Big, v31, "Big::v31"));
#undef X
};

struct Text : public srpc::message_base {
    std::string s;
    static constexpr const char* name = "Text";
    static constexpr auto fields = std::make_tuple(STRUCT_MEMBER(Text, s, "Text::s"));
};

constexpr uint64_t kBatch = 1024, kCalls = 5000;
constexpr int kLegs = 4;  // square (columns), add (records), subtract (columns), multiply (records) on the server
static const std::array<std::string, kLegs> kMethods = {"Calculator_servicer::square", "Calculator_servicer::add",
                                                        "Calculator_servicer::subtract", "Calculator_servicer::multiply"};

// two's-complement arithmetic without signed overflow
static int32_t compute(int op, int32_t l, int32_t r) {
    const uint32_t a = static_cast<uint32_t>(l), b = static_cast<uint32_t>(r);
    const uint32_t v = op == 0 ? a * a : op == 1 ? a + b : op == 2 ? a - b : a * b;
    return static_cast<int32_t>(v);
}

// The server's methods, through the host: a column method and a record method
// (the Resp array arrives zeroed and only its leaves are read back).
template <int OP>
static int column_batch(void* const* rq, void* const* rs, uint64_t n, hipStream_t s) {
    std::vector<int32_t> l(n), r(n), out(n);
    if (hipStreamSynchronize(s) != hipSuccess) return SRPC_E_HIP;
    if (hipMemcpy(l.data(), rq[0], 4 * n, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    if (OP != 0 && hipMemcpy(r.data(), rq[1], 4 * n, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    for (uint64_t i = 0; i < n; ++i) out[i] = compute(OP, l[i], r[i]);
    return hipMemcpy(rs[0], out.data(), 4 * n, hipMemcpyHostToDevice) == hipSuccess ? 0 : SRPC_E_HIP;
}
template <int OP>
static int record_batch(const void* q, void* r, uint64_t n, hipStream_t s) {
    const uint32_t ql = srpc::gpu::leaf_offsets<TwoNumbers>()[0], qr = srpc::gpu::leaf_offsets<TwoNumbers>()[1];
    const uint32_t ro = srpc::gpu::leaf_offsets<Number>()[0];
    std::vector<uint8_t> in(n * sizeof(TwoNumbers)), out(n * sizeof(Number));
    if (hipStreamSynchronize(s) != hipSuccess) return SRPC_E_HIP;
    if (hipMemcpy(in.data(), q, in.size(), hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    if (hipMemcpy(out.data(), r, out.size(), hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    for (uint64_t i = 0; i < n; ++i) {
        int32_t a, b;
        std::memcpy(&a, in.data() + i * sizeof(TwoNumbers) + ql, 4);
        std::memcpy(&b, in.data() + i * sizeof(TwoNumbers) + qr, 4);
        const int32_t v = compute(OP, a, b);
        std::memcpy(out.data() + i * sizeof(Number) + ro, &v, 4);
    }
    return hipMemcpy(r, out.data(), out.size(), hipMemcpyHostToDevice) == hipSuccess ? 0 : SRPC_E_HIP;
}

static void register_all(srpc::gpu::batch_server& srv) {
    srv.register_method<Number, Number>(kMethods[0], column_batch<0>);
    srv.register_record_method<TwoNumbers, Number>(kMethods[1], record_batch<1>);
    srv.register_method<TwoNumbers, Number>(kMethods[2], column_batch<2>);
    srv.register_record_method<TwoNumbers, Number>(kMethods[3], record_batch<3>);
}

struct served_pair : served_socketpair {
    explicit served_pair(uint64_t batch = kBatch) : served_socketpair(batch, register_all) {}
};

static int32_t value(uint64_t i) { return static_cast<int32_t>(static_cast<uint32_t>(i * 2654435761u + 12345u)); }

// A proto whose every byte outside the leaves is told apart from zero and from
// the 0xA5 the reply arrays start with (as gpu_records_test.cpp's).
template <class T>
static void mark_padding(T& proto) {
    auto* b = reinterpret_cast<uint8_t*>(&proto);
    std::vector<bool> leaf(sizeof(T), false);
    const std::vector<uint32_t> offs = srpc::gpu::leaf_offsets<T>();
    size_t f = 0;
    srpc::gpu::for_each_leaf<T>(proto, [&](const auto& v) {
        for (size_t k = 0; k < sizeof(v); ++k) leaf[offs[f] + k] = true;
        ++f;
    });
    for (size_t k = sizeof(void*); k < sizeof(T); ++k)  // the vtable pointer stays: it is a non-leaf byte run too
        if (!leaf[k]) b[k] = static_cast<uint8_t>(0xC0 + k);
}

// The bytes a record leg must leave for a reply: the proto's, with `num` as its leaf.
static std::vector<uint8_t> number_bytes(Number const& proto, int32_t num) {
    std::vector<uint8_t> out(reinterpret_cast<const uint8_t*>(&proto), reinterpret_cast<const uint8_t*>(&proto) + sizeof(Number));
    std::memcpy(out.data() + srpc::gpu::leaf_offsets<Number>()[0], &num, 4);
    return out;
}

// n calls in a fixed pseudo-random order over the four legs: per leg its
// request structs and columns (filled by rank), its reply structs and columns
// (0xA5, 16 guard bytes behind) and the codes.
struct mixed_calls {
    uint64_t n;
    std::vector<uint8_t> method, hcodes;
    std::vector<uint32_t> rank;
    std::array<uint64_t, kLegs> count{};
    std::array<std::vector<int32_t>, kLegs> left, right, out;
    std::array<std::vector<uint8_t>, kLegs> structs;  // the reply arrays and their guards, fetched
    std::array<void*, kLegs> d_left{}, d_right{}, d_out{}, d_req{}, d_resp{};
    std::array<std::array<void*, 2>, kLegs> req_cols{};
    uint8_t *d_method = nullptr, *d_codes = nullptr;
    Number proto{};

    explicit mixed_calls(uint64_t n) : n(n), method(n), hcodes(n + 16), rank(n) {
        mark_padding(proto);
        uint32_t x = 2463534242u;
        for (uint64_t i = 0; i < n; ++i) {
            x ^= x << 13, x ^= x >> 17, x ^= x << 5;
            method[i] = static_cast<uint8_t>(x % kLegs);
            rank[i] = static_cast<uint32_t>(count[method[i]]++);
        }
        for (int k = 0; k < kLegs; ++k) {
            const uint64_t c = count[k];
            left[k].resize(c), right[k].resize(c), out[k].resize(c);
            const uint64_t qs = k == 0 ? sizeof(Number) : sizeof(TwoNumbers);
            std::vector<uint8_t> q(c * qs);
            for (uint64_t r = 0; r < c; ++r) {
                left[k][r] = value(r * kLegs + k), right[k][r] = value(r * 31 + 7 * k + 1);
                if (k == 0) {
                    Number v;
                    v.num = left[k][r];
                    std::memcpy(q.data() + r * qs, static_cast<const void*>(&v), qs);
                } else {
                    TwoNumbers v;
                    v.left = left[k][r], v.right = right[k][r];
                    std::memcpy(q.data() + r * qs, static_cast<const void*>(&v), qs);
                }
            }
            HIPCHECK(hipMalloc(&d_left[k], 4 * c + 16));
            HIPCHECK(hipMalloc(&d_right[k], 4 * c + 16));
            HIPCHECK(hipMalloc(&d_out[k], 4 * c + 16));
            HIPCHECK(hipMalloc(&d_req[k], c * qs + 16));
            HIPCHECK(hipMalloc(&d_resp[k], c * sizeof(Number) + 16));
            HIPCHECK(hipMemcpy(d_left[k], left[k].data(), 4 * c, hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(d_right[k], right[k].data(), 4 * c, hipMemcpyHostToDevice));
            HIPCHECK(hipMemcpy(d_req[k], q.data(), c * qs, hipMemcpyHostToDevice));
            HIPCHECK(hipMemset(d_out[k], 0xA5, 4 * c + 16));
            HIPCHECK(hipMemset(d_resp[k], 0xA5, c * sizeof(Number) + 16));
            req_cols[k] = {d_left[k], d_right[k]};
        }
        HIPCHECK(hipMalloc(reinterpret_cast<void**>(&d_method), n + 16));
        HIPCHECK(hipMalloc(reinterpret_cast<void**>(&d_codes), n + 16));
        HIPCHECK(hipMemcpy(d_method, method.data(), n, hipMemcpyHostToDevice));
        HIPCHECK(hipMemset(d_codes, 0xA5, n + 16));
    }
    std::vector<srpc::gpu::mixed_leg> record_legs(srpc::gpu::batch_client& cl) {
        std::vector<srpc::gpu::mixed_leg> l;
        l.push_back(cl.leg_records<Number, Number>(kMethods[0], static_cast<const Number*>(d_req[0]),
                                                   static_cast<Number*>(d_resp[0]), count[0], proto));
        for (int k = 1; k < kLegs; ++k)
            l.push_back(cl.leg_records<TwoNumbers, Number>(kMethods[k], static_cast<const TwoNumbers*>(d_req[k]),
                                                           static_cast<Number*>(d_resp[k]), count[k], proto));
        return l;
    }
    std::vector<srpc::gpu::mixed_leg> column_legs(srpc::gpu::batch_client& cl) {
        std::vector<srpc::gpu::mixed_leg> l;
        l.push_back(cl.leg<Number, Number>(kMethods[0], req_cols[0].data(), &d_out[0], count[0]));
        for (int k = 1; k < kLegs; ++k)
            l.push_back(cl.leg<TwoNumbers, Number>(kMethods[k], req_cols[k].data(), &d_out[k], count[k]));
        return l;
    }
    void fetch() {
        for (int k = 0; k < kLegs; ++k) {
            HIPCHECK(hipMemcpy(out[k].data(), d_out[k], 4 * count[k], hipMemcpyDeviceToHost));
            structs[k].resize(count[k] * sizeof(Number) + 16);
            HIPCHECK(hipMemcpy(structs[k].data(), d_resp[k], structs[k].size(), hipMemcpyDeviceToHost));
        }
        HIPCHECK(hipMemcpy(hcodes.data(), d_codes, n + 16, hipMemcpyDeviceToHost));
    }
    // call i's reply struct is the proto with `num`
    bool struct_is(uint64_t i, int32_t num) const {
        const std::vector<uint8_t> want = number_bytes(proto, num);
        return std::memcmp(structs[method[i]].data() + rank[i] * sizeof(Number), want.data(), sizeof(Number)) == 0;
    }
    bool guards() const {
        bool ok = true;
        for (int k = 0; k < kLegs; ++k)
            for (uint64_t b = 0; b < 16; ++b) ok = ok && structs[k][count[k] * sizeof(Number) + b] == 0xA5;
        for (uint64_t b = 0; b < 16; ++b) ok = ok && hcodes[n + b] == 0xA5;
        return ok;
    }
    ~mixed_calls() {
        for (int k = 0; k < kLegs; ++k)
            for (void* p : {d_left[k], d_right[k], d_out[k], d_req[k], d_resp[k]}) (void)hipFree(p);
        (void)hipFree(d_method);
        (void)hipFree(d_codes);
    }
};

static bool unknown(uint64_t i) { return i % 10 == 3; }

// Every tenth call's frame is rewritten to a method the server does not know:
// `BE32 | u64 len | method ...`, another first letter.  Frames differ in length.
static void rewrite_every_tenth(uint8_t* frames, uint64_t first, uint64_t m, uint64_t) {
    uint64_t at = 0;
    for (uint64_t i = 0; i < m; ++i) {
        const uint64_t len = 4 + ((uint64_t{frames[at]} << 24) | (uint64_t{frames[at + 1]} << 16) |
                                  (uint64_t{frames[at + 2]} << 8) | uint64_t{frames[at + 3]});
        if (unknown(first + i)) frames[at + 12] = 'X';
        at += len;
    }
}

static void layouts() {
    using srpc::gpu::leaf_offsets;
    CHECK(sizeof(TwoNumbers) == 16 && leaf_offsets<TwoNumbers>() == (std::vector<uint32_t>{8, 12}));
    CHECK(sizeof(Number) == 16 && leaf_offsets<Number>() == (std::vector<uint32_t>{8}));
    CHECK(sizeof(Big) == 264);
}

static void record_legs_in_call_order() {
    uint64_t n_unknown = 0;
    for (uint64_t i = 0; i < kCalls; ++i) n_unknown += unknown(i);
    mixed_calls d(kCalls);
    srpc::gpu::call_stats st, stc;
    {
        served_pair sp;
        srpc::gpu::batch_client cl(sp.fd, kBatch);
        cl.set_request_hook(rewrite_every_tenth);
        st = cl.call_mixed(d.record_legs(cl), d.d_method, kCalls, d.d_codes);
        sp.finish();
        CHECK(sp.stats.requests == kCalls && sp.stats.fallback_requests == n_unknown);
    }
    d.fetch();
    bool structs = true, codes = true;
    for (uint64_t i = 0; i < kCalls; ++i) {
        const int k = d.method[i];
        const uint32_t r = d.rank[i];
        const bool u = unknown(i);
        structs = structs && d.struct_is(i, u ? 0 : compute(k, d.left[k][r], d.right[k][r]));
        codes = codes && d.hcodes[i] == (u ? srpc::RPC_ERR_FUNCTION_NOT_REGISTERED : srpc::RPC_SUCCESS);
    }
    CHECK(structs);
    CHECK(codes);
    CHECK(d.guards());
    for (int k = 0; k < kLegs; ++k) CHECK(d.count[k] > 1000);
    CHECK(st.calls == kCalls && st.chunks == 5 && st.malformed == 0 && st.unanswered == 0);
    CHECK(st.ok == kCalls - n_unknown && st.failed == n_unknown);
    // the same calls through column legs: the same values, codes and counts
    const std::vector<uint8_t> rec_codes = d.hcodes;
    HIPCHECK(hipMemset(d.d_codes, 0xA5, kCalls + 16));
    {
        served_pair sp;
        srpc::gpu::batch_client cl(sp.fd, kBatch);
        cl.set_request_hook(rewrite_every_tenth);
        stc = cl.call_mixed(d.column_legs(cl), d.d_method, kCalls, d.d_codes);
        sp.finish();
    }
    d.fetch();
    bool same = true;
    for (uint64_t i = 0; i < kCalls; ++i) same = same && d.struct_is(i, d.out[d.method[i]][d.rank[i]]);
    CHECK(same);
    CHECK(d.hcodes == rec_codes);
    CHECK(st.calls == stc.calls && st.ok == stc.ok && st.failed == stc.failed && st.malformed == stc.malformed &&
          st.unanswered == stc.unanswered && st.chunks == stc.chunks && st.uniform_chunks == stc.uniform_chunks &&
          st.sent_bytes == stc.sent_bytes && st.received_bytes == stc.received_bytes);
}

// A peer that answers every frame with a Number holding the request's last
// int32, 1029 of them (five replies into the second chunk), and closes: the
// following calls get RPC_ERR_RECV_TIMEOUT and the proto with zero leaves.
static void peer_closes_in_the_second_chunk() {
    constexpr uint64_t n = 3000, answered = kBatch + 5;
    int sv[2];
    if (socketpair(AF_UNIX, SOCK_STREAM, 0, sv) != 0) std::exit(2);
    std::thread peer([fd = sv[1]] {
        std::vector<uint8_t> in;
        uint8_t tmp[4096];
        uint64_t done = 0, at = 0;
        bool open = true;
        while (true) {
            const ssize_t k = recv(fd, tmp, sizeof tmp, 0);
            if (k <= 0) break;
            in.insert(in.end(), tmp, tmp + k);
            while (open && in.size() - at >= 4) {
                const uint64_t len = 4 + ((uint64_t{in[at]} << 24) | (uint64_t{in[at + 1]} << 16) |
                                          (uint64_t{in[at + 2]} << 8) | uint64_t{in[at + 3]});
                if (in.size() - at < len) break;
                int32_t v;
                std::memcpy(&v, in.data() + at + len - 4, 4);
                at += len;
                srpc::packer p;
                srpc::response_t<Number> r;
                Number num;
                num.num = v;
                r.set_value(num);
                p.pack_response(r);
                const std::vector<uint8_t> hdr = srpc::gpu::be32(static_cast<uint32_t>(p.size()));
                srpc::transport::send_all(fd, hdr.data(), hdr.size());
                srpc::transport::send_all(fd, p.data(), p.size());
                if (++done == answered) {
                    shutdown(fd, SHUT_WR);  // no more answers; keep reading until the client goes
                    open = false;
                }
            }
        }
        close(fd);
    });
    {
        mixed_calls d(n);
        srpc::gpu::batch_client cl(sv[0], kBatch);
        const srpc::gpu::call_stats st = cl.call_mixed(d.record_legs(cl), d.d_method, n, d.d_codes);
        d.fetch();
        bool structs = true, codes = true;
        for (uint64_t i = 0; i < n; ++i) {
            const int k = d.method[i];
            const uint32_t r = d.rank[i];
            const int32_t last = k == 0 ? d.left[k][r] : d.right[k][r];
            structs = structs && d.struct_is(i, i < answered ? last : 0);
            codes = codes && d.hcodes[i] == (i < answered ? srpc::RPC_SUCCESS : srpc::RPC_ERR_RECV_TIMEOUT);
        }
        CHECK(structs);
        CHECK(codes);
        CHECK(d.guards());
        CHECK(st.ok == answered && st.unanswered == n - answered && st.failed == 0 && st.malformed == 0);
        CHECK(st.chunks == 3);
    }
    close(sv[0]);
    peer.join();
}

template <class F>
static int thrown(F&& f) {
    try {
        f();
    } catch (srpc::gpu::plan_error const& e) {
        return e.code;
    }
    return 0;
}

static void refusals() {
    int sv[2];
    if (socketpair(AF_UNIX, SOCK_STREAM, 0, sv) != 0) std::exit(2);
    {
        mixed_calls d(100);
        srpc::gpu::batch_client cl(sv[0], kBatch);
        // a record leg beside a column leg
        std::vector<srpc::gpu::mixed_leg> legs = d.record_legs(cl);
        legs[2] = d.column_legs(cl)[2];
        CHECK(thrown([&] { (void)cl.call_mixed(legs, d.d_method, 100, d.d_codes); }) == SRPC_E_UNSUPPORTED);
        // ... and beside a string-bodied leg
        legs = d.record_legs(cl);
        void* cols[1] = {d.d_out[3]};
        uint64_t* offs[1] = {nullptr};
        const uint64_t* coffs[1] = {nullptr};
        const uint64_t cap[1] = {0};
        legs[3] = cl.leg_var<Text, Number>("Calculator_servicer::text", cols, coffs, cols, offs, cap, d.count[3]);
        CHECK(thrown([&] { (void)cl.call_mixed(legs, d.d_method, 100, d.d_codes); }) == SRPC_E_UNSUPPORTED);
        uint8_t byte;
        CHECK(recv(sv[1], &byte, 1, MSG_DONTWAIT) < 0 && (errno == EAGAIN || errno == EWOULDBLOCK));  // nothing was sent
        // a reply struct of more than 256 bytes, a string schema on either side: before the arrays are looked at
        CHECK(thrown([&] { (void)cl.leg_records<Number, Big>(kMethods[0], nullptr, nullptr, 3); }) == SRPC_E_UNSUPPORTED);
        CHECK(thrown([&] { (void)cl.leg_records<Text, Number>(kMethods[0], nullptr, nullptr, 3); }) == SRPC_E_UNSUPPORTED);
        CHECK(thrown([&] { (void)cl.leg_records<Number, Text>(kMethods[0], nullptr, nullptr, 3); }) == SRPC_E_UNSUPPORTED);
        CHECK(thrown([&] { (void)cl.leg_records<Big, Number>(kMethods[0], nullptr, nullptr, 0); }) == 0);  // a large Req is fine
    }
    close(sv[0]);
    close(sv[1]);
    // a leg declaring fewer calls than d_method holds (met in the second chunk, of which nothing is sent), and more
    constexpr uint64_t n = 2000;
    served_pair sp;
    mixed_calls d(n);
    {
        srpc::gpu::batch_client cl(sp.fd, kBatch);
        std::vector<srpc::gpu::mixed_leg> legs = d.record_legs(cl);
        legs[1].calls -= 1;
        CHECK(thrown([&] { (void)cl.call_mixed(legs, d.d_method, n, d.d_codes); }) == SRPC_E_INVALID);
        legs = d.record_legs(cl);
        legs[2].calls += 1;  // the array is not touched past the calls d_method holds
        CHECK(thrown([&] { (void)cl.call_mixed(legs, d.d_method, kBatch, d.d_codes); }) == SRPC_E_INVALID);
    }
    sp.finish();
    CHECK(sp.stats.requests == 2 * kBatch);  // the first chunk of the first call, and the second call's only chunk
}

// `bench N`: N calls over the four methods through record legs and through
// column legs, in chunks of 2^18, against the same server.  Not a test: it
// prints call_stats::gpu_seconds (pack + D2H, H2D + decode + the codes' D2H) and
// the wall time of each.
static int bench(uint64_t n) {
    constexpr uint64_t batch = 1u << 18;
    using clk = std::chrono::steady_clock;
    mixed_calls d(n);
    for (int round = 0; round < 6; ++round) {  // round 0 warms both forms up
        for (int form = 0; form < 2; ++form) {
            served_pair sp(batch);
            srpc::gpu::batch_client cl(sp.fd, batch);
            const std::vector<srpc::gpu::mixed_leg> legs = form ? d.column_legs(cl) : d.record_legs(cl);
            const auto t0 = clk::now();
            const srpc::gpu::call_stats st = cl.call_mixed(legs, d.d_method, n, d.d_codes);
            const double wall = std::chrono::duration<double>(clk::now() - t0).count();
            std::printf("round %d call_mixed %s legs n=%llu wall %.4f s gpu_seconds %.4f send %.4f recv %.4f %s\n", round,
                        form ? "column" : "record", static_cast<unsigned long long>(n), wall, st.gpu_seconds,
                        st.send_seconds, st.recv_seconds, st.ok == n ? "ok" : "WRONG");
            sp.finish();
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    HIPCHECK(hipSetDevice(0));
    if (argc == 3 && std::string(argv[1]) == "bench") return bench(std::strtoull(argv[2], nullptr, 10));
    layouts();
    record_legs_in_call_order();
    peer_closes_in_the_second_chunk();
    refusals();
    std::printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
