// needs: gpu
// srpc::gpu::batch_client (include/srpc/gpu_client.hpp) against
// srpc::gpu::batch_server on the two ends of a socketpair: batches of calls
// from device columns, answered in GPU batches, decoded in call order with one
// status code per call -- all replies full (the uniform decode), every 7th
// call to a method the server does not know (bare error frames among full
// ones), the host-vector overload against packer::unpack_response<Number> on
// the same reply bytes, a peer that closes after half the replies, and a
// scripted peer whose middle chunk holds every malformed row of the reply table
// (the chunk is flagged and recounted frame by frame on the host).
#include <hip/hip_runtime_api.h>
#include <srpc/gpu_client.hpp>
#include <srpc/gpu_server.hpp>
#include <srpc/packer.hpp>
#include <sys/socket.h>
#include <unistd.h>

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

struct Text : public srpc::message_base {
    std::string s;
    static constexpr const char* name = "Text";
    static constexpr auto fields = std::make_tuple(STRUCT_MEMBER(Text, s, "Text::s"));
};

static const std::string kMethod = "Test_servicer::echo";
constexpr uint64_t kBatch = 4096;

static uint64_t request_bytes() { return srpc::gpu::framed_request_prefix<Number>(kMethod).size() + sizeof(int32_t); }

static int echo(void* const* rq, void* const* rs, uint64_t n, hipStream_t s) {
    return hipMemcpyAsync(rs[0], rq[0], n * sizeof(int32_t), hipMemcpyDeviceToDevice, s) == hipSuccess ? 0 : SRPC_E_HIP;
}

static int32_t value(uint64_t i) { return static_cast<int32_t>(static_cast<uint32_t>(i * 2654435761u + 12345u)); }

// A batch_server (echo, no fallback) on one end of a socketpair, on a thread.
struct served_pair {
    int fd = -1;  // the client's end
    int sfd = -1;
    std::thread t;
    srpc::gpu::batch_stats stats;
    served_pair() {
        int sv[2];
        if (socketpair(AF_UNIX, SOCK_STREAM, 0, sv) != 0) std::exit(2);
        fd = sv[0];
        sfd = sv[1];
        t = std::thread([this] {
            auto srv = srpc::gpu::batch_server::single<Number, Number>(kMethod, echo, kBatch);
            stats = srv->serve_connection(sfd);
            close(sfd);
        });
    }
    void finish() {
        shutdown(fd, SHUT_WR);
        t.join();
        close(fd);
    }
};

struct device_calls {
    uint64_t n;
    void *req = nullptr, *resp = nullptr;
    uint8_t* codes = nullptr;
    std::vector<int32_t> in, out;
    std::vector<uint8_t> hcodes;
    explicit device_calls(uint64_t n) : n(n), in(n), out(n), hcodes(n) {
        for (uint64_t i = 0; i < n; ++i) in[i] = value(i);
        HIPCHECK(hipMalloc(&req, 4 * n + 16));
        HIPCHECK(hipMalloc(&resp, 4 * n + 16));
        HIPCHECK(hipMalloc(reinterpret_cast<void**>(&codes), n + 16));
        HIPCHECK(hipMemcpy(req, in.data(), 4 * n, hipMemcpyHostToDevice));
        HIPCHECK(hipMemset(resp, 0xA5, 4 * n));
        HIPCHECK(hipMemset(codes, 0xA5, n));
    }
    void fetch() {
        HIPCHECK(hipMemcpy(out.data(), resp, 4 * n, hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(hcodes.data(), codes, n, hipMemcpyDeviceToHost));
    }
    ~device_calls() {
        (void)hipFree(req);
        (void)hipFree(resp);
        (void)hipFree(codes);
    }
};

static void all_registered() {
    constexpr uint64_t n = 10001;
    served_pair sp;
    device_calls d(n);
    srpc::gpu::batch_client cl(sp.fd, kBatch);
    const srpc::gpu::call_stats st = cl.call<Number, Number>(kMethod, &d.req, n, &d.resp, d.codes);
    d.fetch();
    bool codes0 = true, same = true;
    for (uint64_t i = 0; i < n; ++i) {
        codes0 = codes0 && d.hcodes[i] == srpc::RPC_SUCCESS;
        same = same && d.out[i] == d.in[i];
    }
    CHECK(codes0);
    CHECK(same);
    CHECK(st.calls == n && st.ok == n && st.failed == 0 && st.malformed == 0 && st.unanswered == 0);
    CHECK(st.chunks == 3 && st.uniform_chunks == 3);  // only full frames: no offsets were used
    CHECK(st.sent_bytes == n * request_bytes() && st.received_bytes == n * 23);
    sp.finish();
    CHECK(sp.stats.requests == n && sp.stats.fallback_requests == 0);
}

static void every_seventh_unknown() {
    constexpr uint64_t n = 10001;
    served_pair sp;
    device_calls d(n);
    srpc::gpu::batch_client cl(sp.fd, kBatch);
    // frame: BE32 | u64 len | method ...: another first letter is a method nobody registered
    cl.set_request_hook([](uint8_t* frames, uint64_t first, uint64_t m, uint64_t fin) {
        for (uint64_t i = 0; i < m; ++i)
            if ((first + i) % 7 == 3) frames[i * fin + 12] = 'X';
    });
    const srpc::gpu::call_stats st = cl.call<Number, Number>(kMethod, &d.req, n, &d.resp, d.codes);
    d.fetch();
    uint64_t unknown = 0;
    bool right = true;
    for (uint64_t i = 0; i < n; ++i) {
        if (i % 7 == 3) {
            ++unknown;
            right = right && d.hcodes[i] == srpc::RPC_ERR_FUNCTION_NOT_REGISTERED && d.out[i] == 0;
        } else {
            right = right && d.hcodes[i] == srpc::RPC_SUCCESS && d.out[i] == d.in[i];
        }
    }
    CHECK(right);
    CHECK(st.ok == n - unknown && st.failed == unknown && st.malformed == 0 && st.unanswered == 0);
    CHECK(st.chunks == 3 && st.uniform_chunks == 0);
    CHECK(st.received_bytes == (n - unknown) * 23 + unknown * 5);
    sp.finish();
    CHECK(sp.stats.requests == n && sp.stats.fallback_requests == unknown);
}

static void host_vectors_match_scalar_unpack() {
    constexpr uint64_t n = 1000;
    served_pair sp;
    std::vector<Number> reqs(n);
    for (uint64_t i = 0; i < n; ++i) reqs[i].num = value(i);
    srpc::gpu::batch_client cl(sp.fd, 256);
    cl.keep_replies(true);
    cl.set_request_hook([](uint8_t* frames, uint64_t first, uint64_t m, uint64_t fin) {
        for (uint64_t i = 0; i < m; ++i)
            if ((first + i) % 11 == 5) frames[i * fin + 12] = 'X';
    });
    const std::vector<srpc::response_t<Number>> got = cl.call<Number, Number>(kMethod, reqs);
    CHECK(got.size() == n && cl.last_stats().chunks == 4);
    // the same reply bytes through the scalar packer, one frame at a time
    std::vector<uint8_t> const& bytes = cl.reply_bytes();
    std::vector<uint32_t> offs(n);
    const srpc::gpu::frame_walk w = srpc::gpu::walk_frames(bytes.data(), bytes.size(), n, offs.data(), 23);
    CHECK(w.nframes == n && w.walked == bytes.size() && !w.all_full);
    bool same = w.nframes == n;
    for (uint64_t i = 0; same && i < n; ++i) {
        const uint64_t end = i + 1 < n ? offs[i + 1] : bytes.size();
        const uint64_t len = end - offs[i] - 4;
        if (len == 1) {  // a bare error frame: the scalar unpack_response would read past it
            same = got[i].code() == bytes[offs[i] + 4] && got[i].value().num == 0 && i % 11 == 5;
            continue;
        }
        srpc::packer p(bytes.data() + offs[i] + 4, len);
        const srpc::response_t<Number> want = p.unpack_response<Number>();
        same = p.ok() && got[i].code() == want.code() && got[i].value().num == want.value().num &&
               want.value().num == reqs[i].num;
    }
    CHECK(same);
    sp.finish();
}

static void peer_closes_after_half() {
    constexpr uint64_t n = 1000, answered = 500;
    const uint64_t fin = request_bytes();
    int sv[2];
    if (socketpair(AF_UNIX, SOCK_STREAM, 0, sv) != 0) std::exit(2);
    std::thread peer([fd = sv[1], fin] {
        std::vector<uint8_t> in;
        uint8_t tmp[4096];
        uint64_t done = 0;
        bool open = true;
        while (true) {
            const ssize_t k = recv(fd, tmp, sizeof tmp, 0);
            if (k <= 0) break;
            in.insert(in.end(), tmp, tmp + k);
            while (open && in.size() >= (done + 1) * fin) {
                int32_t v;
                std::memcpy(&v, in.data() + done * fin + fin - 4, 4);
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
        device_calls d(n);
        srpc::gpu::batch_client cl(sv[0], 256);
        const srpc::gpu::call_stats st = cl.call<Number, Number>(kMethod, &d.req, n, &d.resp, d.codes);
        d.fetch();
        bool right = true;
        for (uint64_t i = 0; i < n; ++i) {
            if (i < answered) right = right && d.hcodes[i] == srpc::RPC_SUCCESS && d.out[i] == d.in[i];
            else right = right && d.hcodes[i] == srpc::RPC_ERR_RECV_TIMEOUT && d.out[i] == 0;
        }
        CHECK(right);
        CHECK(st.ok == answered && st.unanswered == n - answered && st.failed == 0 && st.malformed == 0);
        CHECK(st.chunks == 4);
    }
    close(sv[0]);
    peer.join();
}

// Three chunks of 16, 16 and 8 calls answered in one send: the middle chunk
// holds a bare frame, a full frame with a nonzero code, a wrong name (PREFIX)
// and an empty payload (BOUNDS), so its counts come from the host's recount.
static void flagged_middle_chunk() {
    constexpr uint64_t n = 40, batch = 16;
    constexpr uint64_t kBare = 18, kName = 21, kEmpty = 25, kCode = 28;
    device_calls d(n);
    scripted::bytes replies;
    for (uint64_t i = 0; i < n; ++i) {
        Number v;
        v.num = d.in[i];
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
        const srpc::gpu::call_stats st = cl.call<Number, Number>(kMethod, &d.req, n, &d.resp, d.codes);
        d.fetch();
        bool right = true;
        for (uint64_t i = 0; i < n; ++i) {
            if (i == kBare) right = right && d.hcodes[i] == srpc::RPC_ERR_FUNCTION_NOT_REGISTERED && d.out[i] == 0;
            else if (i == kName) right = right && d.hcodes[i] == srpc::RPC_SUCCESS && d.out[i] == 0;  // payload[0], zero
            else if (i == kEmpty) right = right && d.hcodes[i] == SRPC_REPLY_NO_CODE && d.out[i] == 0;
            else if (i == kCode) right = right && d.hcodes[i] == srpc::RPC_ERR_RECV_TIMEOUT && d.out[i] == d.in[i];
            else right = right && d.hcodes[i] == srpc::RPC_SUCCESS && d.out[i] == d.in[i];
        }
        CHECK(right);
        CHECK(st.calls == n && st.ok == n - 4 && st.failed == 2 && st.malformed == 2 && st.unanswered == 0);
        CHECK(st.chunks == 3 && st.uniform_chunks == 2);
        // the later chunks' replies were there before their requests could leave
        CHECK(st.received_bytes == replies.size() && st.sent_bytes == batch * request_bytes());
    }
    close(sv[0]);
    peer.join();
}

static void string_schemas_refused() {
    int sv[2];
    if (socketpair(AF_UNIX, SOCK_STREAM, 0, sv) != 0) std::exit(2);
    srpc::gpu::batch_client cl(sv[0], 256);
    int code = 0;
    try {
        (void)cl.call<Text, Number>(kMethod, std::vector<Text>(3));
    } catch (srpc::gpu::plan_error const& e) {
        code = e.code;
    }
    CHECK(code == SRPC_E_UNSUPPORTED);
    code = 0;
    try {
        (void)cl.call<Number, Text>(kMethod, std::vector<Number>(3));
    } catch (srpc::gpu::plan_error const& e) {
        code = e.code;
    }
    CHECK(code == SRPC_E_UNSUPPORTED);
    close(sv[0]);
    close(sv[1]);
}

int main() {
    srpc::message_registry["Number"] = []() -> std::unique_ptr<Number> { return std::make_unique<Number>(); };
    all_registered();
    every_seventh_unknown();
    host_vectors_match_scalar_unpack();
    peer_closes_after_half();
    flagged_middle_chunk();
    string_schemas_refused();
    std::printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
