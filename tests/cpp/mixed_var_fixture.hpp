// mixed_var_fixture.hpp -- TEST INFRASTRUCTURE ONLY.
//
// The messages, the batch_server (square, add, echo, twice), the per-leg device
// columns and the reply checks shared by gpu_client_mixed_var_test.cpp and
// gpu_client_forms_test.cpp.
#pragma once

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
#include <map>
#include <thread>
#include <type_traits>
#include <vector>

#include "echo_records.hpp"
#include "scripted_peer.hpp"

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

struct Text : public srpc::message_base {
    std::string s;
    static constexpr const char* name = "Text";
    static constexpr auto fields = std::make_tuple(STRUCT_MEMBER(Text, s, "Text::s"));
    void unpack(srpc::buffer::ptr bp) override { srpc::packer p(bp); p >> s; }
};

struct TwoTexts : public srpc::message_base {
    std::string a, b;
    static constexpr const char* name = "TwoTexts";
    static constexpr auto fields = std::make_tuple(STRUCT_MEMBER(TwoTexts, a, "TwoTexts::a"),
                                                   STRUCT_MEMBER(TwoTexts, b, "TwoTexts::b"));
    void unpack(srpc::buffer::ptr bp) override { srpc::packer p(bp); p >> a >> b; }
};

struct multiple_primitives : public srpc::message_base {
    int8_t arg1 = 0;
    char arg2 = 0;
    int64_t arg3 = 0;
    std::string arg4;
    static constexpr const char* name = "multiple_primitives";
    static constexpr auto fields = std::make_tuple(STRUCT_MEMBER(multiple_primitives, arg1, "multiple_primitives::arg1"),
                                                   STRUCT_MEMBER(multiple_primitives, arg2, "multiple_primitives::arg2"),
                                                   STRUCT_MEMBER(multiple_primitives, arg3, "multiple_primitives::arg3"),
                                                   STRUCT_MEMBER(multiple_primitives, arg4, "multiple_primitives::arg4"));
    void unpack(srpc::buffer::ptr bp) override { srpc::packer p(bp); p >> arg1 >> arg2 >> arg3 >> arg4; }
};
using MP = multiple_primitives;

constexpr uint64_t kBatch = 4096;
// square, add, echo, twice; then the ones batch_server does not know: divide, length (a string
// request, a fixed reply), spell (a fixed request, a string reply)
constexpr int kLegs = 7;
static const std::array<std::string, kLegs> kMethods = {"Calculator_servicer::square", "Calculator_servicer::add",
                                                        echo_fixture::kMethod,         "Text_servicer::twice",
                                                        "Calculator_servicer::divide", "Text_servicer::length",
                                                        "Text_servicer::spell"};

static int32_t compute(int op, int32_t l, int32_t r) {
    const uint32_t a = static_cast<uint32_t>(l), b = static_cast<uint32_t>(r);
    return static_cast<int32_t>(op == 0 ? a * a : a + b);
}
static TwoTexts twice(Text const& q) {
    TwoTexts r;
    r.a = q.s + q.s;
    r.b = std::string(q.s.rbegin(), q.s.rend()) + "?";
    return r;
}

static Number length_of(Text const& q) {
    Number r;
    r.num = static_cast<int32_t>(q.s.size());
    return r;
}
static Text spell(Number const& q) {
    Text r;
    const uint32_t v = static_cast<uint32_t>(q.num);
    r.s = std::string(v % 37, static_cast<char>('a' + v % 26)) + "#";
    return r;
}

// ---- the test server's methods: the batch's columns through the host ----

template <int OP>
static int calc_batch(void* const* rq, void* const* rs, uint64_t n, hipStream_t s) {
    std::vector<int32_t> l(n), r(n), out(n);
    if (hipStreamSynchronize(s) != hipSuccess) return SRPC_E_HIP;
    if (hipMemcpy(l.data(), rq[0], 4 * n, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    if (OP != 0 && hipMemcpy(r.data(), rq[1], 4 * n, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    for (uint64_t i = 0; i < n; ++i) out[i] = compute(OP, l[i], r[i]);
    return hipMemcpy(rs[0], out.data(), 4 * n, hipMemcpyHostToDevice) == hipSuccess ? 0 : SRPC_E_HIP;
}

// A string-bodied method through host records: fn answers each request.
template <class Req, class Resp>
static int var_through_host(srpc::gpu::var_batch const& b, hipStream_t s, std::function<Resp(Req const&)> fn) {
    if (hipStreamSynchronize(s) != hipSuccess) return SRPC_E_HIP;
    srpc::gpu::host_columns<Req> hin;
    srpc::gpu::host_columns<Resp> hout;
    hin.scatter(std::vector<Req>(b.n));  // the columns' shapes
    for (size_t f = 0; f < hin.col.size(); ++f) {
        if (!hin.offs[f].empty()) {
            if (hipMemcpy(hin.offs[f].data(), b.req_str_offs[f], 8 * (b.n + 1), hipMemcpyDeviceToHost) != hipSuccess)
                return SRPC_E_HIP;
            hin.col[f].resize(hin.offs[f][b.n]);
        }
        if (!hin.col[f].empty() &&
            hipMemcpy(hin.col[f].data(), b.req_cols[f], hin.col[f].size(), hipMemcpyDeviceToHost) != hipSuccess)
            return SRPC_E_HIP;
    }
    std::vector<Req> in;
    hin.gather(in);
    std::vector<Resp> out(b.n);
    for (uint64_t i = 0; i < b.n; ++i) out[i] = fn(in[i]);
    hout.scatter(out);
    for (size_t f = 0; f < hout.col.size(); ++f) {
        if (hout.col[f].size() > b.resp_cap[f]) return SRPC_E_CAPACITY;
        if (!hout.col[f].empty() &&
            hipMemcpy(b.resp_cols[f], hout.col[f].data(), hout.col[f].size(), hipMemcpyHostToDevice) != hipSuccess)
            return SRPC_E_HIP;
        if (!hout.offs[f].empty() &&
            hipMemcpy(b.resp_str_offs[f], hout.offs[f].data(), 8 * (b.n + 1), hipMemcpyHostToDevice) != hipSuccess)
            return SRPC_E_HIP;
    }
    return 0;
}
static int echo_batch(srpc::gpu::var_batch const& b, hipStream_t s) {
    return var_through_host<MP, MP>(b, s, [](MP const& q) { return echo_fixture::answer(q); });
}
static int twice_batch(srpc::gpu::var_batch const& b, hipStream_t s) { return var_through_host<Text, TwoTexts>(b, s, twice); }

struct served_pair {
    int fd = -1, sfd = -1;
    std::thread t;
    srpc::gpu::batch_stats stats;
    served_pair() {
        int sv[2];
        if (socketpair(AF_UNIX, SOCK_STREAM, 0, sv) != 0) std::exit(2);
        fd = sv[0];
        sfd = sv[1];
        t = std::thread([this] {
            srpc::gpu::batch_server srv(kBatch);  // no fallback server
            srv.register_method<Number, Number>(kMethods[0], calc_batch<0>);
            srv.register_method<TwoNumbers, Number>(kMethods[1], calc_batch<1>);
            srv.register_var_method<MP, MP>(kMethods[2], echo_batch);
            srv.register_var_method<Text, TwoTexts>(kMethods[3], twice_batch);
            stats = srv.serve_connection(sfd);
            close(sfd);
        });
    }
    void finish() {
        shutdown(fd, SHUT_WR);
        t.join();
        close(fd);
    }
};

constexpr uint64_t kGuard = 64;

// One leg's calls on the device: request columns from host records, reply
// columns 0xA5-filled with kGuard bytes behind each.
template <class Req, class Resp>
struct leg_data {
    std::vector<Req> in;
    srpc::gpu::host_columns<Req> hin;
    srpc::gpu::host_columns<Resp> hout;  // fetch()
    std::vector<void*> req, resp;
    std::vector<uint64_t*> req_offs, resp_offs;
    std::vector<uint64_t> cap, size;  // reply leaves: bytes of the column, bytes of a leaf (0: a string)
    std::vector<std::vector<uint8_t>> raw;  // fetch(): the reply columns with their guards
    std::vector<std::vector<uint64_t>> raw_offs;

    void upload(uint64_t chars_cap) {
        const uint64_t n = in.size();
        hin.scatter(in);
        for (size_t f = 0; f < hin.col.size(); ++f) {
            void* d = nullptr;
            HIPCHECK(hipMalloc(&d, hin.col[f].size() + 16));
            HIPCHECK(hipMemcpy(d, hin.col[f].data(), hin.col[f].size(), hipMemcpyHostToDevice));
            req.push_back(d);
            uint64_t* o = nullptr;
            if (!hin.offs[f].empty()) {
                HIPCHECK(hipMalloc(reinterpret_cast<void**>(&o), 8 * (n + 1)));
                HIPCHECK(hipMemcpy(o, hin.offs[f].data(), 8 * (n + 1), hipMemcpyHostToDevice));
            }
            req_offs.push_back(o);
        }
        srpc::gpu::host_columns<Resp> shape;
        shape.scatter(std::vector<Resp>(1));
        for (size_t f = 0; f < shape.col.size(); ++f) {
            const bool str = !shape.offs[f].empty();
            size.push_back(str ? 0 : shape.col[f].size());
            cap.push_back(str ? chars_cap : n * shape.col[f].size());
            void* d = nullptr;
            HIPCHECK(hipMalloc(&d, cap[f] + kGuard));
            HIPCHECK(hipMemset(d, 0xA5, cap[f] + kGuard));
            resp.push_back(d);
            uint64_t* o = nullptr;
            if (str) {
                HIPCHECK(hipMalloc(reinterpret_cast<void**>(&o), 8 * (n + 1) + kGuard));
                HIPCHECK(hipMemset(o, 0xA5, 8 * (n + 1) + kGuard));
            }
            resp_offs.push_back(o);
        }
    }
    // the reply columns as records; false when a guard or the offsets' shape is broken
    bool fetch(std::vector<Resp>& got) {
        const uint64_t n = in.size();
        bool ok = true;
        hout.n = n;
        hout.col.assign(resp.size(), {});
        hout.offs.assign(resp.size(), {});
        raw.assign(resp.size(), {});
        raw_offs.assign(resp.size(), {});
        for (size_t f = 0; f < resp.size(); ++f) {
            raw[f].resize(cap[f] + kGuard);
            HIPCHECK(hipMemcpy(raw[f].data(), resp[f], cap[f] + kGuard, hipMemcpyDeviceToHost));
            uint64_t used = cap[f];
            if (!size[f]) {
                raw_offs[f].resize(n + 1 + kGuard / 8);
                HIPCHECK(hipMemcpy(raw_offs[f].data(), resp_offs[f], 8 * (n + 1) + kGuard, hipMemcpyDeviceToHost));
                for (uint64_t g = n + 1; g < raw_offs[f].size(); ++g) ok = ok && raw_offs[f][g] == 0xA5A5A5A5A5A5A5A5ull;
                ok = ok && raw_offs[f][0] == 0;
                for (uint64_t i = 0; i < n; ++i) ok = ok && raw_offs[f][i] <= raw_offs[f][i + 1];
                if (!ok) return false;
                hout.offs[f].assign(raw_offs[f].begin(), raw_offs[f].begin() + static_cast<long>(n) + 1);
                used = std::min(raw_offs[f][n], cap[f]);
                if (raw_offs[f][n] > cap[f]) return false;
            }
            for (uint64_t g = used; g < cap[f] + kGuard; ++g) ok = ok && raw[f][g] == 0xA5;
            hout.col[f].assign(raw[f].begin(), raw[f].begin() + static_cast<long>(used));
        }
        if (ok) hout.gather(got);
        return ok;
    }
    ~leg_data() {
        for (void* p : req) (void)hipFree(p);
        for (void* p : resp) (void)hipFree(p);
        for (uint64_t* p : req_offs) (void)hipFree(p);
        for (uint64_t* p : resp_offs) (void)hipFree(p);
    }
};

static int32_t value(uint64_t i) { return static_cast<int32_t>(static_cast<uint32_t>(i * 2654435761u + 12345u)); }

// n calls in a fixed pseudo-random order over the five legs.
struct mixed_calls {
    uint64_t n;
    std::vector<uint8_t> method, hcodes;
    std::vector<uint32_t> rank;
    std::array<uint64_t, kLegs> count{};
    leg_data<Number, Number> square;
    leg_data<TwoNumbers, Number> add, divide;
    leg_data<MP, MP> echo;
    leg_data<Text, TwoTexts> text;
    leg_data<Text, Number> length;
    leg_data<Number, Text> spelled;
    uint8_t *d_method = nullptr, *d_codes = nullptr;

    explicit mixed_calls(uint64_t n, uint64_t echo_cap_cut = 0) : n(n), method(n), hcodes(n), rank(n) {
        uint32_t x = 2463534242u;
        for (uint64_t i = 0; i < n; ++i) {
            x ^= x << 13, x ^= x >> 17, x ^= x << 5;
            method[i] = static_cast<uint8_t>(x % kLegs);
            rank[i] = static_cast<uint32_t>(count[method[i]]++);
        }
        square.in.resize(count[0]), add.in.resize(count[1]), echo.in.resize(count[2]), text.in.resize(count[3]);
        divide.in.resize(count[4]), length.in.resize(count[5]), spelled.in.resize(count[6]);
        for (uint64_t r = 0; r < count[0]; ++r) square.in[r].num = value(r * 5);
        for (uint64_t r = 0; r < count[1]; ++r) add.in[r].left = value(r * 5 + 1), add.in[r].right = value(r * 31 + 8);
        for (uint64_t r = 0; r < count[4]; ++r) divide.in[r].left = value(r * 5 + 4), divide.in[r].right = value(r * 31 + 29);
        uint64_t echo_chars = 0;
        for (uint64_t r = 0; r < count[2]; ++r) {
            echo_fixture::fill_request(echo.in[r], r);
            echo_chars += echo.in[r].arg4.size() + 1;  // the answer appends "!"
        }
        uint64_t text_chars = 0;
        for (uint64_t r = 0; r < count[3]; ++r) {
            MP m;
            echo_fixture::fill_request(m, r + 77777);
            text.in[r].s = m.arg4 + m.arg4 + m.arg4;  // 0..120 chars
            text_chars += 3 * text.in[r].s.size() + 1;  // both answers together
        }
        uint64_t spell_chars = 0;
        for (uint64_t r = 0; r < count[5]; ++r) {
            MP m;
            echo_fixture::fill_request(m, r + 5555);
            length.in[r].s = m.arg4;
        }
        for (uint64_t r = 0; r < count[6]; ++r) {
            spelled.in[r].num = value(r * 7 + 3);
            spell_chars += spell(spelled.in[r]).s.size();
        }
        square.upload(0), add.upload(0), divide.upload(0), length.upload(0);
        spelled.upload(spell_chars);
        echo.upload(echo_chars - echo_cap_cut);  // exact: nothing to spare
        text.upload(text_chars);
        HIPCHECK(hipMalloc(reinterpret_cast<void**>(&d_method), n + 16));
        HIPCHECK(hipMalloc(reinterpret_cast<void**>(&d_codes), n + 16));
        HIPCHECK(hipMemcpy(d_method, method.data(), n, hipMemcpyHostToDevice));
        HIPCHECK(hipMemset(d_codes, 0xA5, n + 16));
    }
    std::vector<srpc::gpu::mixed_leg> legs(srpc::gpu::batch_client& cl) {
        std::vector<srpc::gpu::mixed_leg> l;
        l.push_back(cl.leg<Number, Number>(kMethods[0], square.req.data(), square.resp.data(), count[0]));
        l.push_back(cl.leg<TwoNumbers, Number>(kMethods[1], add.req.data(), add.resp.data(), count[1]));
        l.push_back(cl.leg_var<MP, MP>(kMethods[2], echo.req.data(), echo.req_offs.data(), echo.resp.data(),
                                       echo.resp_offs.data(), echo.cap.data(), count[2]));
        l.push_back(cl.leg_var<Text, TwoTexts>(kMethods[3], text.req.data(), text.req_offs.data(), text.resp.data(),
                                               text.resp_offs.data(), text.cap.data(), count[3]));
        l.push_back(cl.leg<TwoNumbers, Number>(kMethods[4], divide.req.data(), divide.resp.data(), count[4]));
        l.push_back(cl.leg_var<Text, Number>(kMethods[5], length.req.data(), length.req_offs.data(), length.resp.data(),
                                             length.resp_offs.data(), length.cap.data(), count[5]));
        l.push_back(cl.leg_var<Number, Text>(kMethods[6], spelled.req.data(), spelled.req_offs.data(), spelled.resp.data(),
                                             spelled.resp_offs.data(), spelled.cap.data(), count[6]));
        return l;
    }
    // `BE32 | packer::pack_request` of call i
    std::vector<uint8_t> frame(uint64_t i) const {
        srpc::packer p;
        const uint32_t r = rank[i];
        auto pack = [&](auto const& v) {
            srpc::request_t<std::remove_cvref_t<decltype(v)>> q;
            q.set_method_name(kMethods[method[i]]);
            q.set_value(v);
            p.pack_request(q);
        };
        switch (method[i]) {
        case 0: pack(square.in[r]); break;
        case 1: pack(add.in[r]); break;
        case 2: pack(echo.in[r]); break;
        case 3: pack(text.in[r]); break;
        case 4: pack(divide.in[r]); break;
        case 5: pack(length.in[r]); break;
        default: pack(spelled.in[r]); break;
        }
        std::vector<uint8_t> f = srpc::gpu::be32(static_cast<uint32_t>(p.size()));
        f.insert(f.end(), p.data(), p.data() + p.size());
        return f;
    }
    // the service's answer to call i as a full reply frame (divide answered with a zero), and the
    // chars of its last leaf where that is a string
    std::vector<uint8_t> reply(uint64_t i, srpc::rpc_status_code code = srpc::RPC_SUCCESS, uint64_t* last_chars = nullptr) const {
        const uint32_t r = rank[i];
        Number num;
        uint64_t chars = 0;
        std::vector<uint8_t> f;
        switch (method[i]) {
        case 0: num.num = compute(0, square.in[r].num, 0), f = scripted::full(num, code); break;
        case 1: num.num = compute(1, add.in[r].left, add.in[r].right), f = scripted::full(num, code); break;
        case 2: chars = echo.in[r].arg4.size() + 1, f = scripted::full(echo_fixture::answer(echo.in[r]), code); break;
        case 3: chars = text.in[r].s.size() + 1, f = scripted::full(twice(text.in[r]), code); break;
        case 4: f = scripted::full(num, code); break;
        case 5: f = scripted::full(length_of(length.in[r]), code); break;
        default: chars = spell(spelled.in[r]).s.size(), f = scripted::full(spell(spelled.in[r]), code); break;
        }
        if (last_chars) *last_chars = chars;
        return f;
    }
    void fetch_codes() { HIPCHECK(hipMemcpy(hcodes.data(), d_codes, n, hipMemcpyDeviceToHost)); }
    ~mixed_calls() {
        (void)hipFree(d_method);
        (void)hipFree(d_codes);
    }
};

static bool same(MP const& a, MP const& b) {
    return a.arg1 == b.arg1 && a.arg2 == b.arg2 && a.arg3 == b.arg3 && a.arg4 == b.arg4;
}
static bool zero(MP const& a) { return a.arg1 == 0 && a.arg2 == 0 && a.arg3 == 0 && a.arg4.empty(); }

// Every reply of calls [0, answered) is the service's, the rest unanswered.
// served: batch_server, which answers divide, length and spell with a bare
// RPC_ERR_FUNCTION_NOT_REGISTERED; else the scalar peer, which answers all (divide with a zero).
// bad: calls whose reply is a malformed or bare frame, with the code the table gives them: zero
// fields and empty strings.
static void check_replies(mixed_calls& d, uint64_t answered, bool served = true,
                          std::map<uint64_t, uint8_t> const& bad = {}) {
    const uint8_t unknown_code = served ? srpc::RPC_ERR_FUNCTION_NOT_REGISTERED : srpc::RPC_SUCCESS;
    d.fetch_codes();
    std::vector<Number> sq, ad, dv, ln;
    std::vector<MP> ec;
    std::vector<TwoTexts> tx;
    std::vector<Text> sp;
    CHECK(d.length.fetch(ln));
    CHECK(d.spelled.fetch(sp));
    CHECK(d.square.fetch(sq));
    CHECK(d.add.fetch(ad));
    CHECK(d.divide.fetch(dv));
    CHECK(d.echo.fetch(ec));
    CHECK(d.text.fetch(tx));
    if (g_fail) return;
    bool right = true;
    for (uint64_t i = 0; i < d.n; ++i) {
        const int k = d.method[i];
        const uint32_t r = d.rank[i];
        const bool ans = i < answered;
        const uint8_t code = d.hcodes[i];
        bool ok;
        if (bad.count(i))
            ok = code == bad.at(i) && (k == 0   ? sq[r].num == 0
                                       : k == 1 ? ad[r].num == 0
                                       : k == 2 ? zero(ec[r])
                                       : k == 3 ? tx[r].a.empty() && tx[r].b.empty()
                                       : k == 4 ? dv[r].num == 0
                                       : k == 5 ? ln[r].num == 0
                                                : sp[r].s.empty());
        else if (k == 0) ok = ans ? code == srpc::RPC_SUCCESS && sq[r].num == compute(0, d.square.in[r].num, 0) : sq[r].num == 0;
        else if (k == 1) ok = ans ? code == srpc::RPC_SUCCESS && ad[r].num == compute(1, d.add.in[r].left, d.add.in[r].right)
                                  : ad[r].num == 0;
        else if (k == 2) ok = ans ? code == srpc::RPC_SUCCESS && same(ec[r], echo_fixture::answer(d.echo.in[r])) : zero(ec[r]);
        else if (k == 3) {
            const TwoTexts w = twice(d.text.in[r]);
            ok = ans ? code == srpc::RPC_SUCCESS && tx[r].a == w.a && tx[r].b == w.b : tx[r].a.empty() && tx[r].b.empty();
        } else if (k == 4) ok = (ans ? code == unknown_code : true) && dv[r].num == 0;  // code 1, zeros
        else if (k == 5) ok = (ans ? code == unknown_code : true) &&
                              ln[r].num == (ans && !served ? length_of(d.length.in[r]).num : 0);
        else ok = (ans ? code == unknown_code : true) && sp[r].s == (ans && !served ? spell(d.spelled.in[r]).s : std::string());
        if (!ans) ok = ok && code == srpc::RPC_ERR_RECV_TIMEOUT;
        if (!ok && right)
            std::fprintf(stderr, "call %llu of %llu answered (leg %d, rank %u): code %u, number %d\n", (unsigned long long)i,
                         (unsigned long long)answered, k, r, code, k == 0 ? sq[r].num : k == 1 ? ad[r].num : k == 4 ? dv[r].num : 0);
        right = right && ok;
    }
    CHECK(right);
}
