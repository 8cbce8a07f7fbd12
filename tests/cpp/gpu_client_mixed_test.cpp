// needs: gpu
// srpc::gpu::batch_client::call_mixed (include/srpc/gpu_client.hpp) against
// srpc::gpu::batch_server on the two ends of a socketpair: an ordered batch of
// calls over five methods -- square, add, subtract, multiply served on the
// device, divide unknown to the server -- packed in call order from per-method
// columns, answered in request order, decoded into per-method columns with one
// code per call; a leg that declares one call too few; a peer that closes after
// half the replies; a scripted peer whose middle chunk holds every malformed row
// of the reply table.
#include <hip/hip_runtime_api.h>
#include <srpc/gpu_client.hpp>
#include <srpc/gpu_server.hpp>
#include <srpc/packer.hpp>
#include <sys/socket.h>
#include <unistd.h>

#include <array>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

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
    int32_t num;
    static constexpr const char* name = "Number";
    static constexpr auto fields = std::make_tuple(STRUCT_MEMBER(Number, num, "Number::num"));
    void unpack(srpc::buffer::ptr bp) override { srpc::packer p(bp); p >> num; }
};

struct TwoNumbers : public srpc::message_base {
    int32_t left, right;
    static constexpr const char* name = "TwoNumbers";
    static constexpr auto fields = std::make_tuple(STRUCT_MEMBER(TwoNumbers, left, "TwoNumbers::left"),
                                                   STRUCT_MEMBER(TwoNumbers, right, "TwoNumbers::right"));
    void unpack(srpc::buffer::ptr bp) override { srpc::packer p(bp); p >> left >> right; }
};

constexpr uint64_t kBatch = 4096;
constexpr int kLegs = 5;  // square, add, subtract, multiply, divide (the server does not know it)
static const std::array<std::string, kLegs> kMethods = {
    "Calculator_servicer::square", "Calculator_servicer::add", "Calculator_servicer::subtract",
    "Calculator_servicer::multiply", "Calculator_servicer::divide"};

// two's-complement arithmetic without signed overflow
static int32_t compute(int op, int32_t l, int32_t r) {
    const uint32_t a = static_cast<uint32_t>(l), b = static_cast<uint32_t>(r);
    const uint32_t v = op == 0 ? a * a : op == 1 ? a + b : op == 2 ? a - b : a * b;
    return static_cast<int32_t>(v);
}

// A device method of the test server: the batch's columns through the host.
template <int OP>
static int method_batch(void* const* rq, void* const* rs, uint64_t n, hipStream_t s) {
    std::vector<int32_t> l(n), r(n), out(n);
    if (hipStreamSynchronize(s) != hipSuccess) return SRPC_E_HIP;
    if (hipMemcpy(l.data(), rq[0], 4 * n, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    if (OP != 0 && hipMemcpy(r.data(), rq[1], 4 * n, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    for (uint64_t i = 0; i < n; ++i) out[i] = compute(OP, l[i], r[i]);
    return hipMemcpy(rs[0], out.data(), 4 * n, hipMemcpyHostToDevice) == hipSuccess ? 0 : SRPC_E_HIP;
}

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
            srv.register_method<Number, Number>(kMethods[0], method_batch<0>);
            srv.register_method<TwoNumbers, Number>(kMethods[1], method_batch<1>);
            srv.register_method<TwoNumbers, Number>(kMethods[2], method_batch<2>);
            srv.register_method<TwoNumbers, Number>(kMethods[3], method_batch<3>);
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

static int32_t value(uint64_t i) { return static_cast<int32_t>(static_cast<uint32_t>(i * 2654435761u + 12345u)); }

// n calls in a fixed pseudo-random order over the five legs, with per-leg
// device columns (requests filled by rank, replies and codes 0xA5).
struct mixed_calls {
    uint64_t n;
    std::vector<uint8_t> method, hcodes;
    std::vector<uint32_t> rank;
    std::array<uint64_t, kLegs> count{};
    std::array<std::vector<int32_t>, kLegs> left, right, out;
    std::array<void*, kLegs> d_left{}, d_right{}, d_out{};
    std::array<std::array<void*, 2>, kLegs> req_cols{};
    uint8_t *d_method = nullptr, *d_codes = nullptr;

    explicit mixed_calls(uint64_t n) : n(n), method(n), hcodes(n), rank(n) {
        uint32_t x = 2463534242u;
        for (uint64_t i = 0; i < n; ++i) {
            x ^= x << 13, x ^= x >> 17, x ^= x << 5;
            method[i] = static_cast<uint8_t>(x % kLegs);
            rank[i] = static_cast<uint32_t>(count[method[i]]++);
        }
        for (int k = 0; k < kLegs; ++k) {
            const uint64_t c = count[k];
            left[k].resize(c), right[k].resize(c), out[k].resize(c);
            for (uint64_t r = 0; r < c; ++r) left[k][r] = value(r * kLegs + k), right[k][r] = value(r * 31 + 7 * k + 1);
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
        l.push_back(cl.leg<Number, Number>(kMethods[0], req_cols[0].data(), &d_out[0], count[0]));
        for (int k = 1; k < kLegs; ++k)
            l.push_back(cl.leg<TwoNumbers, Number>(kMethods[k], req_cols[k].data(), &d_out[k], count[k]));
        return l;
    }
    void fetch() {
        for (int k = 0; k < kLegs; ++k) HIPCHECK(hipMemcpy(out[k].data(), d_out[k], 4 * count[k], hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(hcodes.data(), d_codes, n, hipMemcpyDeviceToHost));
    }
    ~mixed_calls() {
        for (int k = 0; k < kLegs; ++k) {
            (void)hipFree(d_left[k]);
            (void)hipFree(d_right[k]);
            (void)hipFree(d_out[k]);
        }
        (void)hipFree(d_method);
        (void)hipFree(d_codes);
    }
};

static void five_legs_in_call_order() {
    constexpr uint64_t n = 10001;
    served_pair sp;
    mixed_calls d(n);
    srpc::gpu::batch_client cl(sp.fd, kBatch);
    const srpc::gpu::call_stats st = cl.call_mixed(d.legs(cl), d.d_method, n, d.d_codes);
    d.fetch();
    bool right = true;
    for (uint64_t i = 0; i < n; ++i) {
        const int k = d.method[i];
        const uint32_t r = d.rank[i];
        if (k == 4) right = right && d.hcodes[i] == srpc::RPC_ERR_FUNCTION_NOT_REGISTERED && d.out[k][r] == 0;
        else right = right && d.hcodes[i] == srpc::RPC_SUCCESS && d.out[k][r] == compute(k, d.left[k][r], d.right[k][r]);
    }
    CHECK(right);
    CHECK(d.count[4] > 0 && d.count[0] > 0);
    CHECK(st.calls == n && st.chunks == 3 && st.uniform_chunks == 0);
    CHECK(st.ok + st.failed == n && st.failed == d.count[4] && st.malformed == 0 && st.unanswered == 0);
    uint64_t sent = 0;
    const uint64_t fin[kLegs] = {57, 62, 67, 67, 65};
    for (int k = 0; k < kLegs; ++k) sent += d.count[k] * fin[k];
    CHECK(st.sent_bytes == sent && st.received_bytes == (n - d.count[4]) * 23 + d.count[4] * 5);
    sp.finish();
    CHECK(sp.stats.requests == n);
}

static void a_leg_one_call_short() {
    constexpr uint64_t n = 5000;  // two chunks; the missing element is met in the second
    served_pair sp;
    mixed_calls d(n);
    {
        srpc::gpu::batch_client cl(sp.fd, kBatch);
        std::vector<srpc::gpu::mixed_leg> legs = d.legs(cl);
        legs[1].calls -= 1;
        int code = 0;
        try {
            (void)cl.call_mixed(legs, d.d_method, n, d.d_codes);
        } catch (srpc::gpu::plan_error const& e) {
            code = e.code;
        }
        CHECK(code == SRPC_E_INVALID);
        // an id no leg has
        uint8_t bad = kLegs;
        HIPCHECK(hipMemcpy(d.d_method + kBatch + 7, &bad, 1, hipMemcpyHostToDevice));
        code = 0;
        try {
            (void)cl.call_mixed(d.legs(cl), d.d_method + kBatch, n - kBatch, d.d_codes);
        } catch (srpc::gpu::plan_error const& e) {
            code = e.code;
        }
        CHECK(code == SRPC_E_INVALID);
    }
    sp.finish();
    CHECK(sp.stats.requests == kBatch);  // the first chunk only: no byte of a refused chunk was sent
}

static void peer_closes_after_half() {
    constexpr uint64_t n = 1000, answered = 500;
    int sv[2];
    if (socketpair(AF_UNIX, SOCK_STREAM, 0, sv) != 0) std::exit(2);
    // answers every frame with a Number holding the request's last int32
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
        srpc::gpu::batch_client cl(sv[0], 256);
        const srpc::gpu::call_stats st = cl.call_mixed(d.legs(cl), d.d_method, n, d.d_codes);
        d.fetch();
        bool right = true;
        for (uint64_t i = 0; i < n; ++i) {
            const int k = d.method[i];
            const uint32_t r = d.rank[i];
            const int32_t last = k == 0 ? d.left[k][r] : d.right[k][r];
            if (i < answered) right = right && d.hcodes[i] == srpc::RPC_SUCCESS && d.out[k][r] == last;
            else right = right && d.hcodes[i] == srpc::RPC_ERR_RECV_TIMEOUT && d.out[k][r] == 0;
        }
        CHECK(right);
        CHECK(st.ok == answered && st.unanswered == n - answered && st.failed == 0 && st.malformed == 0);
        CHECK(st.chunks == 4);
    }
    close(sv[0]);
    peer.join();
}

// Three chunks of 16, 16 and 8 calls answered in one send by a scripted peer
// (every leg's reply a Number holding the request's last int32): the middle
// chunk holds a wrong name (PREFIX), a bare frame, an empty payload (BOUNDS) and a
// full frame with a nonzero code, on calls of at least two legs with nonzero
// first[], so its counts come from the host's recount (judge_reply_mixed).
static void flagged_middle_chunk() {
    constexpr uint64_t n = 40, batch = 16;
    mixed_calls d(n);
    // the chunk's first call, then the first call of another leg, then the next two
    const uint64_t kName = batch;
    uint64_t kBare = kName + 1;
    while (kBare < 2 * batch && d.method[kBare] == d.method[kName]) ++kBare;
    CHECK(kBare + 2 < 2 * batch);
    const uint64_t kEmpty = kBare + 1, kCode = kBare + 2;
    CHECK(d.rank[kName] > 0 || d.rank[kBare] > 0);  // first[k] != 0 for one of them
    scripted::bytes replies;
    std::vector<int32_t> last(n);
    for (uint64_t i = 0; i < n; ++i) {
        const int k = d.method[i];
        last[i] = k == 0 ? d.left[k][d.rank[i]] : d.right[k][d.rank[i]];
        Number v;
        v.num = last[i];
        const scripted::bytes f = i == kBare    ? scripted::bare(srpc::RPC_ERR_FUNCTION_NOT_REGISTERED)
                                  : i == kName  ? scripted::wrong_name(scripted::full(v))
                                  : i == kEmpty ? scripted::empty()
                                  : i == kCode  ? scripted::full(v, srpc::RPC_ERR_RECV_TIMEOUT)
                                                : scripted::full(v);
        replies.insert(replies.end(), f.begin(), f.end());
    }
    int sv[2];
    if (socketpair(AF_UNIX, SOCK_STREAM, 0, sv) != 0) std::exit(2);
    std::thread peer = scripted::answer_at_once(sv[1], batch, replies);
    {
        srpc::gpu::batch_client cl(sv[0], batch);
        const srpc::gpu::call_stats st = cl.call_mixed(d.legs(cl), d.d_method, n, d.d_codes);
        d.fetch();
        bool right = true;
        uint64_t sent = 0;
        const uint64_t fin[kLegs] = {57, 62, 67, 67, 65};
        for (uint64_t i = 0; i < n; ++i) {
            const int32_t out = d.out[d.method[i]][d.rank[i]];
            if (i < batch) sent += fin[d.method[i]];
            if (i == kBare) right = right && d.hcodes[i] == srpc::RPC_ERR_FUNCTION_NOT_REGISTERED && out == 0;
            else if (i == kName) right = right && d.hcodes[i] == srpc::RPC_SUCCESS && out == 0;  // payload[0], zero
            else if (i == kEmpty) right = right && d.hcodes[i] == SRPC_REPLY_NO_CODE && out == 0;
            else if (i == kCode) right = right && d.hcodes[i] == srpc::RPC_ERR_RECV_TIMEOUT && out == last[i];
            else right = right && d.hcodes[i] == srpc::RPC_SUCCESS && out == last[i];
        }
        CHECK(right);
        CHECK(st.calls == n && st.ok == n - 4 && st.failed == 2 && st.malformed == 2 && st.unanswered == 0);
        CHECK(st.chunks == 3 && st.uniform_chunks == 0);
        // the later chunks' replies were there before their requests could leave
        CHECK(st.received_bytes == replies.size() && st.sent_bytes == sent);
    }
    close(sv[0]);
    peer.join();
}

int main() {
    five_legs_in_call_order();
    a_leg_one_call_short();
    peer_closes_after_half();
    flagged_middle_chunk();
    std::printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
