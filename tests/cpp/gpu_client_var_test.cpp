// needs: gpu
// srpc::gpu::batch_client::call_var (include/srpc/gpu_client.hpp) against
// srpc::gpu::batch_server::register_var_method on the two ends of a
// socketpair: batches of calls whose request and/or response has a string
// field -- an echo of multiple_primitives over three chunks (the reply's string
// offsets continue across chunks), every 7th call rewritten to an unknown
// method (bare error frames among the full ones), the host-vector overload
// against packer::unpack_response on the same reply bytes, and a response
// column too small for the reply chars, requests too large for the send
// buffer.  Against a scalar peer built on the
// packer itself: Text -> Number and Number -> Text (each side's fixed path;
// batch_server's string methods take strings on both sides), a peer that
// closes after half the replies, and a scripted peer whose middle chunk holds
// every malformed row of the string reply table.
#include <hip/hip_runtime_api.h>
#include <srpc/gpu_client.hpp>
#include <srpc/gpu_server.hpp>
#include <srpc/packer.hpp>
#include <sys/socket.h>
#include <unistd.h>

#include <cstdio>
#include <cstring>
#include <functional>
#include <thread>
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

struct Text : public srpc::message_base {
    std::string s;
    static constexpr const char* name = "Text";
    static constexpr auto fields = std::make_tuple(STRUCT_MEMBER(Text, s, "Text::s"));
    void unpack(srpc::buffer::ptr bp) override { srpc::packer p(bp); p >> s; }
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

static const std::string kMethod = echo_fixture::kMethod;
constexpr uint64_t kBatch = 4096;
constexpr uint64_t kMaxChars = 40;  // echo_fixture's strings

// Echo on the device with copies alone: every column and the string's offsets.
static int echo_var(srpc::gpu::var_batch const& b, hipStream_t s) {
    const uint64_t sizes[3] = {1, 1, 8};
    bool ok = true;
    for (int f = 0; f < 3; ++f)
        ok = ok && hipMemcpyAsync(b.resp_cols[f], b.req_cols[f], b.n * sizes[f], hipMemcpyDeviceToDevice, s) == hipSuccess;
    ok = ok && hipMemcpyAsync(b.resp_str_offs[3], b.req_str_offs[3], 8 * (b.n + 1), hipMemcpyDeviceToDevice, s) == hipSuccess;
    const uint64_t chars = std::min<uint64_t>(b.resp_cap[3], b.n * kMaxChars);
    ok = ok && hipMemcpyAsync(b.resp_cols[3], b.req_cols[3], chars, hipMemcpyDeviceToDevice, s) == hipSuccess;
    return ok ? 0 : SRPC_E_HIP;
}

static std::string spell(int32_t v) {
    return std::string(static_cast<uint32_t>(v) % 37, static_cast<char>('a' + static_cast<uint32_t>(v) % 26)) + "#";
}

// A scalar server on a thread, one request at a time with the packer the
// generated stubs use (unpack_request -> fn -> pack_response -> BE32 frame);
// after `limit` answers it stops answering and only reads until the client goes.
template <class Req, class Resp>
static std::thread scalar_peer(int fd, std::function<Resp(Req const&)> fn, uint64_t limit = ~0ull) {
    return std::thread([fd, fn, limit] {
        std::vector<uint8_t> in;
        uint8_t tmp[4096];
        uint64_t done = 0, at = 0;
        bool open = true;
        while (true) {
            const ssize_t k = recv(fd, tmp, sizeof tmp, 0);
            if (k <= 0) break;
            in.insert(in.end(), tmp, tmp + k);
            while (open && in.size() - at >= 4) {
                const uint64_t len = (uint64_t{in[at]} << 24) | (uint64_t{in[at + 1]} << 16) | (uint64_t{in[at + 2]} << 8) |
                                     uint64_t{in[at + 3]};
                if (in.size() - at < 4 + len) break;
                srpc::packer q(in.data() + at + 4, len);
                const srpc::request_t<Req> rq = q.template unpack_request<Req>();
                at += 4 + len;
                srpc::packer p;
                srpc::response_t<Resp> r;
                r.set_value(fn(rq.value()));
                p.pack_response(r);
                const std::vector<uint8_t> hdr = srpc::gpu::be32(static_cast<uint32_t>(p.size()));
                srpc::transport::send_all(fd, hdr.data(), hdr.size());
                srpc::transport::send_all(fd, p.data(), p.size());
                if (++done == limit) {
                    shutdown(fd, SHUT_WR);  // no more answers; keep reading until the client goes
                    open = false;
                }
            }
        }
        close(fd);
    });
}

// A batch_server on one end of a socketpair, on a thread.
struct served_pair {
    int fd = -1;  // the client's end
    int sfd = -1;
    std::thread t;
    srpc::gpu::batch_stats stats;
    explicit served_pair(std::function<void(srpc::gpu::batch_server&)> setup, uint64_t batch = kBatch) {
        int sv[2];
        if (socketpair(AF_UNIX, SOCK_STREAM, 0, sv) != 0) std::exit(2);
        fd = sv[0];
        sfd = sv[1];
        t = std::thread([this, setup, batch] {
            srpc::gpu::batch_server srv(batch);
            setup(srv);
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
static void echo_setup(srpc::gpu::batch_server& s) { s.register_var_method<MP, MP>(kMethod, echo_var); }

// n multiple_primitives calls on the device, outputs filled with 0xA5.
struct mp_calls {
    uint64_t n, chars_cap;
    std::vector<MP> in;
    srpc::gpu::host_columns<MP> hin, hout;
    void *req[4] = {}, *resp[4] = {};
    uint64_t *req_offs[4] = {}, *resp_offs[4] = {};
    uint64_t cap[4] = {};
    uint8_t* codes = nullptr;
    std::vector<uint8_t> hcodes, rchars;
    std::vector<uint64_t> roffs;
    explicit mp_calls(uint64_t n, uint64_t chars_cap_ = 0) : n(n), in(n), hcodes(n), roffs(n + 1) {
        for (uint64_t i = 0; i < n; ++i) echo_fixture::fill_request(in[i], i);
        hin.scatter(in);
        chars_cap = chars_cap_ ? chars_cap_ : hin.col[3].size() + 64;
        const uint64_t sizes[4] = {1, 1, 8, 0};
        for (int f = 0; f < 4; ++f) {
            cap[f] = sizes[f] ? n * sizes[f] : chars_cap;
            HIPCHECK(hipMalloc(&req[f], hin.col[f].size() + 16));
            HIPCHECK(hipMemcpy(req[f], hin.col[f].data(), hin.col[f].size(), hipMemcpyHostToDevice));
            HIPCHECK(hipMalloc(&resp[f], cap[f] + 64));
            HIPCHECK(hipMemset(resp[f], 0xA5, cap[f] + 64));
        }
        HIPCHECK(hipMalloc(reinterpret_cast<void**>(&req_offs[3]), 8 * (n + 1)));
        HIPCHECK(hipMemcpy(req_offs[3], hin.offs[3].data(), 8 * (n + 1), hipMemcpyHostToDevice));
        HIPCHECK(hipMalloc(reinterpret_cast<void**>(&resp_offs[3]), 8 * (n + 1) + 16));
        HIPCHECK(hipMemset(resp_offs[3], 0xA5, 8 * (n + 1) + 16));
        HIPCHECK(hipMalloc(reinterpret_cast<void**>(&codes), n + 16));
        HIPCHECK(hipMemset(codes, 0xA5, n + 16));
        rchars.resize(chars_cap + 64);
    }
    srpc::gpu::call_stats call(srpc::gpu::batch_client& cl) {
        return cl.call_var<MP, MP>(kMethod, req, req_offs, n, resp, resp_offs, cap, codes);
    }
    // the response columns as host_columns (chars up to offs[upto])
    void fetch(uint64_t upto) {
        hout.n = upto;
        hout.col.assign(4, {});
        hout.offs.assign(4, {});
        const uint64_t sizes[3] = {1, 1, 8};
        for (int f = 0; f < 3; ++f) {
            hout.col[f].resize(upto * sizes[f]);
            HIPCHECK(hipMemcpy(hout.col[f].data(), resp[f], upto * sizes[f], hipMemcpyDeviceToHost));
        }
        HIPCHECK(hipMemcpy(roffs.data(), resp_offs[3], 8 * (n + 1), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(rchars.data(), resp[3], chars_cap + 64, hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(hcodes.data(), codes, n, hipMemcpyDeviceToHost));
        hout.offs[3].assign(roffs.begin(), roffs.begin() + static_cast<long>(upto) + 1);
        hout.col[3].assign(rchars.begin(), rchars.begin() + static_cast<long>(std::min<uint64_t>(roffs[upto], chars_cap)));
    }
    bool offsets_monotone_from_zero() const {
        bool ok = roffs[0] == 0;
        for (uint64_t i = 0; i < n; ++i) ok = ok && roffs[i] <= roffs[i + 1];
        return ok;
    }
    ~mp_calls() {
        for (int f = 0; f < 4; ++f) {
            (void)hipFree(req[f]);
            (void)hipFree(resp[f]);
            (void)hipFree(req_offs[f]);
            (void)hipFree(resp_offs[f]);
        }
        (void)hipFree(codes);
    }
};

static bool same(MP const& a, MP const& b) {
    return a.arg1 == b.arg1 && a.arg2 == b.arg2 && a.arg3 == b.arg3 && a.arg4 == b.arg4;
}
static bool zero(MP const& a) { return a.arg1 == 0 && a.arg2 == 0 && a.arg3 == 0 && a.arg4.empty(); }

static uint64_t frame_bytes(MP const& r, bool request) {
    const uint64_t pre = request ? srpc::gpu::request_prefix<MP>(kMethod).size()
                                 : srpc::gpu::response_prefix<MP>(srpc::RPC_SUCCESS).size();
    return 4 + pre + 1 + 1 + 8 + 8 + r.arg4.size();
}

static void echo_three_chunks() {
    constexpr uint64_t n = 10001;
    served_pair sp(echo_setup);
    mp_calls d(n);
    srpc::gpu::batch_client cl(sp.fd, kBatch);
    const srpc::gpu::call_stats st = d.call(cl);
    d.fetch(n);
    std::vector<MP> got;
    d.hout.gather(got);
    bool codes0 = true, eq = true;
    uint64_t sent = 0, received = 0;
    for (uint64_t i = 0; i < n; ++i) {
        codes0 = codes0 && d.hcodes[i] == srpc::RPC_SUCCESS;
        eq = eq && same(got[i], d.in[i]);
        sent += frame_bytes(d.in[i], true);
        received += frame_bytes(d.in[i], false);
    }
    CHECK(codes0);
    CHECK(eq);
    // absolute offsets over the three chunks: the requests' own
    CHECK(d.offsets_monotone_from_zero() && d.roffs == d.hin.offs[3]);
    CHECK(d.roffs[n] == d.hin.col[3].size() && d.roffs[kBatch] > 0 && d.roffs[2 * kBatch] > d.roffs[kBatch]);
    bool guard = true;
    for (uint64_t k = d.roffs[n]; k < d.chars_cap + 64; ++k) guard = guard && d.rchars[k] == 0xA5;
    CHECK(guard);
    CHECK(st.calls == n && st.ok == n && st.failed == 0 && st.malformed == 0 && st.unanswered == 0);
    CHECK(st.chunks == 3 && st.uniform_chunks == 0);
    CHECK(st.sent_bytes == sent && st.received_bytes == received);
    sp.finish();
    CHECK(sp.stats.requests == n && sp.stats.fallback_requests == 0);
}

// The request hook of a string request batch: frames found by their BE32s.
static void rewrite_every(uint64_t every, uint64_t which, uint8_t* frames, uint64_t first, uint64_t m, uint64_t fin) {
    if (fin != 0) {
        ++g_fail;  // string requests come with bytes-per-frame 0
        return;
    }
    uint64_t at = 0;
    for (uint64_t i = 0; i < m; ++i) {
        const uint64_t len = 4 + ((uint64_t{frames[at]} << 24) | (uint64_t{frames[at + 1]} << 16) |
                                  (uint64_t{frames[at + 2]} << 8) | uint64_t{frames[at + 3]});
        // frame: BE32 | u64 len | method ...: another first letter is a method nobody registered
        if ((first + i) % every == which) frames[at + 12] = 'X';
        at += len;
    }
}

static void every_seventh_unknown() {
    constexpr uint64_t n = 10001;
    served_pair sp(echo_setup);
    mp_calls d(n);
    srpc::gpu::batch_client cl(sp.fd, kBatch);
    cl.set_request_hook([](uint8_t* f, uint64_t first, uint64_t m, uint64_t fin) { rewrite_every(7, 3, f, first, m, fin); });
    const srpc::gpu::call_stats st = d.call(cl);
    d.fetch(n);
    std::vector<MP> got;
    d.hout.gather(got);
    uint64_t unknown = 0, received = 0;
    bool right = true;
    for (uint64_t i = 0; i < n; ++i) {
        if (i % 7 == 3) {
            ++unknown;
            received += 5;
            right = right && d.hcodes[i] == srpc::RPC_ERR_FUNCTION_NOT_REGISTERED && zero(got[i]);
        } else {
            received += frame_bytes(d.in[i], false);
            right = right && d.hcodes[i] == srpc::RPC_SUCCESS && same(got[i], d.in[i]);
        }
    }
    CHECK(right);
    CHECK(d.offsets_monotone_from_zero());
    CHECK(st.ok == n - unknown && st.failed == unknown && st.malformed == 0 && st.unanswered == 0);
    CHECK(st.calls == n && st.chunks == 3 && st.received_bytes == received);
    sp.finish();
    CHECK(sp.stats.requests == n && sp.stats.fallback_requests == unknown);
}

// batch_server's string methods need strings on both sides, so the peer of
// these two is the scalar packer itself.
static void each_side_fixed() {
    constexpr uint64_t n = 300;
    {  // Text -> Number: string requests, fixed replies (the uniform decode)
        int sv[2];
        if (socketpair(AF_UNIX, SOCK_STREAM, 0, sv) != 0) std::exit(2);
        std::thread peer = scalar_peer<Text, Number>(sv[1], [](Text const& t) {
            Number r;
            r.num = static_cast<int32_t>(t.s.size());
            return r;
        });
        std::vector<Text> reqs(n);
        for (uint64_t i = 0; i < n; ++i) reqs[i].s.assign((i * 7) % 53, static_cast<char>('a' + i % 26));
        {
            srpc::gpu::batch_client cl(sv[0], 128);
            cl.set_request_hook([](uint8_t*, uint64_t, uint64_t, uint64_t fin) {
                if (fin != 0) ++g_fail;  // string requests come with bytes-per-frame 0
            });
            const std::vector<srpc::response_t<Number>> got = cl.call_var<Text, Number>("T_servicer::len", reqs);
            bool right = got.size() == n;
            for (uint64_t i = 0; right && i < n; ++i)
                right = got[i].code() == srpc::RPC_SUCCESS && got[i].value().num == static_cast<int32_t>(reqs[i].s.size());
            CHECK(right);
            CHECK(cl.last_stats().ok == n && cl.last_stats().chunks == 3 && cl.last_stats().uniform_chunks == 3);
        }
        shutdown(sv[0], SHUT_WR);
        peer.join();
        close(sv[0]);
    }
    {  // Number -> Text: fixed requests (srpc_gpu_pack), string replies
        int sv[2];
        if (socketpair(AF_UNIX, SOCK_STREAM, 0, sv) != 0) std::exit(2);
        std::thread peer = scalar_peer<Number, Text>(sv[1], [](Number const& v) {
            Text r;
            r.s = spell(v.num);
            return r;
        });
        std::vector<Number> reqs(n);
        for (uint64_t i = 0; i < n; ++i) reqs[i].num = static_cast<int32_t>(i * 2654435761u);
        {
            srpc::gpu::batch_client cl(sv[0], 128);
            cl.set_request_hook([](uint8_t*, uint64_t, uint64_t, uint64_t fin) {
                if (fin == 0) ++g_fail;  // fixed requests keep their bytes-per-frame
            });
            const std::vector<srpc::response_t<Text>> got = cl.call_var<Number, Text>("T_servicer::spell", reqs);
            bool right = got.size() == n;
            for (uint64_t i = 0; right && i < n; ++i)
                right = got[i].code() == srpc::RPC_SUCCESS && got[i].value().s == spell(reqs[i].num);
            CHECK(right);
            CHECK(cl.last_stats().ok == n && cl.last_stats().chunks == 3 && cl.last_stats().uniform_chunks == 0);
        }
        shutdown(sv[0], SHUT_WR);
        peer.join();
        close(sv[0]);
    }
}

static void host_vectors_match_scalar_unpack() {
    constexpr uint64_t n = 1000;
    served_pair sp(echo_setup);
    std::vector<MP> reqs(n);
    for (uint64_t i = 0; i < n; ++i) echo_fixture::fill_request(reqs[i], i + 77);
    srpc::gpu::batch_client cl(sp.fd, 256);
    cl.keep_replies(true);
    cl.set_request_hook([](uint8_t* f, uint64_t first, uint64_t m, uint64_t fin) { rewrite_every(11, 5, f, first, m, fin); });
    const std::vector<srpc::response_t<MP>> got = cl.call_var<MP, MP>(kMethod, reqs);
    CHECK(got.size() == n && cl.last_stats().chunks == 4);
    // the same reply bytes through the scalar packer, one frame at a time
    std::vector<uint8_t> const& bytes = cl.reply_bytes();
    std::vector<uint32_t> offs(n);
    const srpc::gpu::frame_walk w = srpc::gpu::walk_frames(bytes.data(), bytes.size(), n, offs.data(), 0);
    CHECK(w.nframes == n && w.walked == bytes.size() && !w.all_full);
    bool eq = w.nframes == n && got.size() == n;
    for (uint64_t i = 0; eq && i < n; ++i) {
        const uint64_t end = i + 1 < n ? offs[i + 1] : bytes.size();
        const uint64_t len = end - offs[i] - 4;
        if (len == 1) {  // a bare error frame: the scalar unpack_response would read past it
            eq = got[i].code() == bytes[offs[i] + 4] && zero(got[i].value()) && i % 11 == 5;
            continue;
        }
        srpc::packer p(bytes.data() + offs[i] + 4, len);
        const srpc::response_t<MP> want = p.unpack_response<MP>();
        eq = p.ok() && got[i].code() == want.code() && same(got[i].value(), want.value()) && same(want.value(), reqs[i]);
    }
    CHECK(eq);
    sp.finish();
}

static void peer_closes_after_half() {
    constexpr uint64_t n = 1000, answered = 500;
    int sv[2];
    if (socketpair(AF_UNIX, SOCK_STREAM, 0, sv) != 0) std::exit(2);
    std::thread peer = scalar_peer<MP, MP>(sv[1], [](MP const& q) { return q; }, answered);
    {
        mp_calls d(n);
        srpc::gpu::batch_client cl(sv[0], 256);
        const srpc::gpu::call_stats st = d.call(cl);
        d.fetch(n);
        std::vector<MP> got;
        d.hout.gather(got);
        bool right = true;
        for (uint64_t i = 0; i < n; ++i) {
            if (i < answered) right = right && d.hcodes[i] == srpc::RPC_SUCCESS && same(got[i], d.in[i]);
            else right = right && d.hcodes[i] == srpc::RPC_ERR_RECV_TIMEOUT && zero(got[i]);
        }
        CHECK(right);
        CHECK(d.offsets_monotone_from_zero() && d.roffs[n] == d.hin.offs[3][answered]);
        CHECK(st.ok == answered && st.unanswered == n - answered && st.failed == 0 && st.malformed == 0);
        CHECK(st.chunks == 4);
    }
    close(sv[0]);
    peer.join();
}

// Three chunks of 16, 16 and 8 calls answered in one send by a scripted peer:
// the middle chunk holds a bare frame, a full frame with a nonzero code, a wrong
// name (PREFIX), an empty payload and a string running past its frame (BOUNDS),
// so its counts come from the host's recount (walk_reply_var).
static void flagged_middle_chunk() {
    constexpr uint64_t n = 40, batch = 16;
    constexpr uint64_t kBare = 18, kName = 21, kEmpty = 25, kOverrun = 27, kCode = 29;
    mp_calls d(n);
    scripted::bytes replies;
    uint64_t chars = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const scripted::bytes f = i == kBare      ? scripted::bare(srpc::RPC_ERR_FUNCTION_NOT_REGISTERED)
                                  : i == kName    ? scripted::wrong_name(scripted::full(d.in[i]))
                                  : i == kEmpty   ? scripted::empty()
                                  : i == kOverrun ? scripted::string_overrun(scripted::full(d.in[i]), d.in[i].arg4.size())
                                  : i == kCode    ? scripted::full(d.in[i], srpc::RPC_ERR_RECV_TIMEOUT)
                                                  : scripted::full(d.in[i]);
        replies.insert(replies.end(), f.begin(), f.end());
        if (i != kBare && i != kName && i != kEmpty && i != kOverrun) chars += d.in[i].arg4.size();
    }
    int sv[2];
    if (socketpair(AF_UNIX, SOCK_STREAM, 0, sv) != 0) std::exit(2);
    std::thread peer = scripted::answer_at_once(sv[1], batch, replies);
    {
        srpc::gpu::batch_client cl(sv[0], batch);
        const srpc::gpu::call_stats st = d.call(cl);
        d.fetch(n);
        std::vector<MP> got;
        d.hout.gather(got);
        bool right = true;
        uint64_t sent = 0;
        for (uint64_t i = 0; i < n; ++i) {
            if (i < batch) sent += frame_bytes(d.in[i], true);
            if (i == kBare) right = right && d.hcodes[i] == srpc::RPC_ERR_FUNCTION_NOT_REGISTERED && zero(got[i]);
            else if (i == kName || i == kOverrun) right = right && d.hcodes[i] == srpc::RPC_SUCCESS && zero(got[i]);  // payload[0]
            else if (i == kEmpty) right = right && d.hcodes[i] == SRPC_REPLY_NO_CODE && zero(got[i]);
            else if (i == kCode) right = right && d.hcodes[i] == srpc::RPC_ERR_RECV_TIMEOUT && same(got[i], d.in[i]);
            else right = right && d.hcodes[i] == srpc::RPC_SUCCESS && same(got[i], d.in[i]);
        }
        CHECK(right);
        // absolute offsets over the three chunks; the malformed replies are empty strings
        CHECK(d.offsets_monotone_from_zero() && d.roffs[n] == chars && d.roffs[batch] == d.hin.offs[3][batch]);
        bool guard = true;
        for (uint64_t k = d.roffs[n]; k < d.chars_cap + 64; ++k) guard = guard && d.rchars[k] == 0xA5;
        CHECK(guard);
        CHECK(st.calls == n && st.ok == n - 5 && st.failed == 2 && st.malformed == 3 && st.unanswered == 0);
        CHECK(st.chunks == 3 && st.uniform_chunks == 0);
        // the later chunks' replies were there before their requests could leave
        CHECK(st.received_bytes == replies.size() && st.sent_bytes == sent);
    }
    close(sv[0]);
    peer.join();
}

static void response_column_too_small() {
    constexpr uint64_t n = 1000, batch = 256;
    srpc::gpu::host_columns<MP> probe;
    {
        std::vector<MP> in(n);
        for (uint64_t i = 0; i < n; ++i) echo_fixture::fill_request(in[i], i);
        probe.scatter(in);
    }
    // room for the first chunk's chars and ten more: the second chunk does not fit
    const uint64_t cap = probe.offs[3][batch] + 10;
    served_pair sp(echo_setup, batch);
    mp_calls d(n, cap);
    srpc::gpu::batch_client cl(sp.fd, batch);
    int code = 0;
    try {
        (void)d.call(cl);
    } catch (srpc::gpu::plan_error const& e) {
        code = e.code;
    }
    CHECK(code == SRPC_E_CAPACITY);
    CHECK(cl.last_stats().chunks == 2 && cl.last_stats().ok == 2 * batch);
    d.fetch(batch);
    std::vector<MP> got;
    d.hout.gather(got);
    bool first = true, guard = true;
    for (uint64_t i = 0; i < batch; ++i) first = first && d.hcodes[i] == srpc::RPC_SUCCESS && same(got[i], d.in[i]);
    for (uint64_t k = d.roffs[batch]; k < cap + 64; ++k) guard = guard && d.rchars[k] == 0xA5;  // nothing past the first chunk
    CHECK(first);
    CHECK(guard);
    sp.finish();
}

// Requests that outgrow the send buffer: refused before a byte is sent.
static void requests_too_large() {
    constexpr uint64_t n = 600, batch = 256;
    served_pair sp(echo_setup, batch);
    mp_calls d(n);
    srpc::gpu::batch_client cl(sp.fd, batch);
    int code = 0;
    try {
        (void)cl.call_var<MP, MP>(kMethod, d.req, d.req_offs, n, d.resp, d.resp_offs, d.cap, d.codes,
                                  srpc::gpu::var_call_limits{8, 512});  // 256 * 8 + 4096 bytes for 256 frames of ~70
    } catch (srpc::gpu::plan_error const& e) {
        code = e.code;
    }
    CHECK(code == SRPC_E_CAPACITY);
    sp.finish();
    CHECK(sp.stats.requests == 0);
}

int main() {
    srpc::message_registry["Number"] = []() -> std::unique_ptr<Number> { return std::make_unique<Number>(); };
    srpc::message_registry["Text"] = []() -> std::unique_ptr<Text> { return std::make_unique<Text>(); };
    srpc::message_registry["multiple_primitives"] = []() -> std::unique_ptr<MP> { return std::make_unique<MP>(); };
    echo_three_chunks();
    every_seventh_unknown();
    each_side_fixed();
    host_vectors_match_scalar_unpack();
    peer_closes_after_half();
    flagged_middle_chunk();
    response_column_too_small();
    requests_too_large();
    std::printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
