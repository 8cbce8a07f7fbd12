// needs: gpu
// srpc::gpu::batch_client::call_mixed with string-bodied legs
// (include/srpc/gpu_client.hpp: leg_var, the overload taking var_call_limits)
// against srpc::gpu::batch_server on the two ends of a socketpair: an ordered
// batch over square and add (fixed), echo (register_var_method, echo_fixture), a
// string-only method answering two strings, and three methods the server does
// not know: divide, and two with strings on one side only (Text -> Number,
// Number -> Text: a framed fixed plan beside a string plan in one leg), which a
// scalar peer answers in the last part.  Every sent frame is `BE32 | packer::pack_request` of its call, every
// reply the service's answer in its leg's columns with offsets absolute over the
// three chunks; then a reply column one byte short, a send buffer too small, a
// leg declaring one call too few, a peer that closes after half the replies, and
// a scripted peer whose middle chunk holds every malformed row of both tables.
// The messages, server and columns are mixed_var_fixture.hpp's.
#include "mixed_var_fixture.hpp"

static void all_legs_in_call_order() {
    constexpr uint64_t n = 10000;
    served_pair sp;
    mixed_calls d(n);
    srpc::gpu::batch_client cl(sp.fd, kBatch);
    std::vector<uint8_t> sent;
    std::vector<uint64_t> chunk_first;
    cl.set_request_hook([&](uint8_t* frames, uint64_t first, uint64_t calls, uint64_t per_frame) {
        CHECK(per_frame == 0);
        chunk_first.push_back(first);
        uint64_t at = 0;
        for (uint64_t j = 0; j < calls; ++j)
            at += 4 + ((uint64_t{frames[at]} << 24) | (uint64_t{frames[at + 1]} << 16) | (uint64_t{frames[at + 2]} << 8) |
                       uint64_t{frames[at + 3]});
        sent.insert(sent.end(), frames, frames + at);
    });
    const srpc::gpu::call_stats st = cl.call_mixed(d.legs(cl), d.d_method, n, d.d_codes, srpc::gpu::var_call_limits{});
    CHECK((chunk_first == std::vector<uint64_t>{0, kBatch, 2 * kBatch}));
    // every sent frame, in call order
    bool frames_ok = true;
    uint64_t at = 0;
    for (uint64_t i = 0; i < n && frames_ok; ++i) {
        const std::vector<uint8_t> f = d.frame(i);
        frames_ok = at + f.size() <= sent.size() && std::memcmp(sent.data() + at, f.data(), f.size()) == 0;
        at += f.size();
    }
    CHECK(frames_ok && at == sent.size());
    check_replies(d, n);
    for (int k = 0; k < kLegs; ++k) CHECK(d.count[k] > 0);
    // offsets absolute over the three chunks, the columns filled to the byte
    CHECK(d.echo.raw_offs[3][d.count[2]] == d.echo.cap[3]);
    CHECK(d.text.raw_offs[0][d.count[3]] + d.text.raw_offs[1][d.count[3]] == d.text.cap[0]);
    CHECK(st.calls == n && st.chunks == 3);
    CHECK(st.ok + st.failed == n && st.failed == d.count[4] + d.count[5] + d.count[6] && st.malformed == 0 &&
          st.unanswered == 0);
    CHECK(st.sent_bytes == sent.size());
    sp.finish();
    CHECK(sp.stats.requests == n);
}

static int code_of(std::function<void()> f) {
    try {
        f();
    } catch (srpc::gpu::plan_error const& e) {
        return e.code;
    }
    return 0;
}

static void resp_cap_one_byte_short() {
    constexpr uint64_t n = 3000;  // one chunk
    served_pair sp;
    mixed_calls d(n, 1);
    {
        srpc::gpu::batch_client cl(sp.fd, kBatch);
        CHECK(code_of([&] { (void)cl.call_mixed(d.legs(cl), d.d_method, n, d.d_codes, srpc::gpu::var_call_limits{}); }) ==
              SRPC_E_CAPACITY);
        // nothing at or past the capacity was written; the offsets count every reply
        std::vector<uint8_t> raw(d.echo.cap[3] + kGuard);
        HIPCHECK(hipMemcpy(raw.data(), d.echo.resp[3], raw.size(), hipMemcpyDeviceToHost));
        bool guard = true;
        for (uint64_t g = d.echo.cap[3]; g < raw.size(); ++g) guard = guard && raw[g] == 0xA5;
        CHECK(guard);
        uint64_t end = 0;
        HIPCHECK(hipMemcpy(&end, d.echo.resp_offs[3] + d.count[2], 8, hipMemcpyDeviceToHost));
        CHECK(end == d.echo.cap[3] + 1);
        CHECK(cl.last_stats().ok + cl.last_stats().failed == n);
    }
    sp.finish();
}

static void send_buffer_too_small() {
    constexpr uint64_t n = kBatch;  // one chunk of ~78 bytes per call
    served_pair sp;
    mixed_calls d(n);
    {
        srpc::gpu::batch_client cl(sp.fd, kBatch);
        srpc::gpu::var_call_limits lim;
        lim.max_request_bytes = 16;  // the fixed legs' 67-byte frames size the buffer: kBatch * 67 + 4096 bytes
        uint64_t bytes = 0;
        for (uint64_t i = 0; i < n; ++i) bytes += d.frame(i).size();
        CHECK(bytes > kBatch * 67 + 4096);
        CHECK(code_of([&] { (void)cl.call_mixed(d.legs(cl), d.d_method, n, d.d_codes, lim); }) == SRPC_E_CAPACITY);
    }
    sp.finish();
    CHECK(sp.stats.requests == 0);  // nothing of the refused chunk was sent
}

static void a_leg_one_call_short() {
    constexpr uint64_t n = 5000;  // two chunks; the missing element is met in the second
    served_pair sp;
    mixed_calls d(n);
    {
        srpc::gpu::batch_client cl(sp.fd, kBatch);
        std::vector<srpc::gpu::mixed_leg> legs = d.legs(cl);
        legs[2].calls -= 1;  // the echo leg
        CHECK(code_of([&] { (void)cl.call_mixed(legs, d.d_method, n, d.d_codes, srpc::gpu::var_call_limits{}); }) ==
              SRPC_E_INVALID);
    }
    sp.finish();
    CHECK(sp.stats.requests == kBatch);  // the first chunk only: no byte of a refused chunk was sent
}

static void peer_closes_after_half() {
    constexpr uint64_t n = 1000, answered = 500;
    int sv[2];
    if (socketpair(AF_UNIX, SOCK_STREAM, 0, sv) != 0) std::exit(2);
    // a scalar peer on the packer itself: dispatches by method name, one request at a time
    std::thread peer([fd = sv[1]] {
        std::vector<uint8_t> in;
        uint8_t tmp[4096];
        uint64_t done = 0, at = 0;
        bool open = true;
        auto reply = [&](auto const& resp) {
            srpc::packer p;
            srpc::response_t<std::remove_cvref_t<decltype(resp)>> r;
            r.set_value(resp);
            p.pack_response(r);
            const std::vector<uint8_t> hdr = srpc::gpu::be32(static_cast<uint32_t>(p.size()));
            srpc::transport::send_all(fd, hdr.data(), hdr.size());
            srpc::transport::send_all(fd, p.data(), p.size());
        };
        while (true) {
            const ssize_t k = recv(fd, tmp, sizeof tmp, 0);
            if (k <= 0) break;
            in.insert(in.end(), tmp, tmp + k);
            while (open && in.size() - at >= 4) {
                const uint64_t len = (uint64_t{in[at]} << 24) | (uint64_t{in[at + 1]} << 16) | (uint64_t{in[at + 2]} << 8) |
                                     uint64_t{in[at + 3]};
                if (in.size() - at < 4 + len) break;
                uint64_t ml = 0;
                std::memcpy(&ml, in.data() + at + 4, 8);
                const std::string m(reinterpret_cast<const char*>(in.data() + at + 12), ml);
                srpc::packer q(in.data() + at + 4, len);
                Number num;
                if (m == kMethods[0]) {
                    num.num = compute(0, q.unpack_request<Number>().value().num, 0);
                    reply(num);
                } else if (m == kMethods[2]) {
                    reply(echo_fixture::answer(q.unpack_request<MP>().value()));
                } else if (m == kMethods[3]) {
                    reply(twice(q.unpack_request<Text>().value()));
                } else if (m == kMethods[5]) {
                    reply(length_of(q.unpack_request<Text>().value()));
                } else if (m == kMethods[6]) {
                    reply(spell(q.unpack_request<Number>().value()));
                } else {  // add; divide answered like add here, so every answered call is full
                    const TwoNumbers t = q.unpack_request<TwoNumbers>().value();
                    num.num = m == kMethods[1] ? compute(1, t.left, t.right) : 0;
                    reply(num);
                }
                at += 4 + len;
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
        const srpc::gpu::call_stats st = cl.call_mixed(d.legs(cl), d.d_method, n, d.d_codes, srpc::gpu::var_call_limits{});
        check_replies(d, answered, false);  // this peer answers every method, divide with code 0 and a zero
        CHECK(d.count[5] > 0 && d.count[6] > 0);
        CHECK(st.ok == answered && st.unanswered == n - answered && st.failed == 0 && st.malformed == 0);
        CHECK(st.chunks == 4);
    }
    close(sv[0]);
    peer.join();
}

// Three chunks of 16, 16 and 8 calls answered in one send by a scripted peer
// (the scalar service's answers): the middle chunk holds a string running past
// its frame (BOUNDS) on a string leg, a wrong name (PREFIX) on another leg, a
// bare frame, an empty payload (BOUNDS) and a full frame with a nonzero code, so
// its counts come from the host's recount (judge_reply_mixed).
static void flagged_middle_chunk() {
    constexpr uint64_t n = 40, batch = 16;
    mixed_calls d(n);
    auto string_reply = [&](uint64_t i) { return d.method[i] == 2 || d.method[i] == 3 || d.method[i] == 6; };
    uint64_t kOverrun = batch;
    while (kOverrun < 2 * batch && !(string_reply(kOverrun) && d.rank[kOverrun] > 0)) ++kOverrun;  // first[k] != 0
    CHECK(kOverrun < 2 * batch);
    std::vector<uint64_t> others;  // kName on another leg, then kBare, kEmpty, kCode
    for (uint64_t i = batch; i < 2 * batch; ++i)
        if (i != kOverrun && (!others.empty() || d.method[i] != d.method[kOverrun])) others.push_back(i);
    CHECK(others.size() >= 4);
    if (g_fail) return;
    const uint64_t kName = others[0], kBare = others[1], kEmpty = others[2], kCode = others[3];
    const std::map<uint64_t, uint8_t> bad = {{kOverrun, srpc::RPC_SUCCESS},  // payload[0]
                                             {kName, srpc::RPC_SUCCESS},
                                             {kBare, srpc::RPC_ERR_FUNCTION_NOT_REGISTERED},
                                             {kEmpty, SRPC_REPLY_NO_CODE}};
    scripted::bytes replies;
    uint64_t sent = 0;
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t last_chars = 0;
        scripted::bytes f = d.reply(i, i == kCode ? srpc::RPC_ERR_RECV_TIMEOUT : srpc::RPC_SUCCESS, &last_chars);
        if (i == kOverrun) f = scripted::string_overrun(f, last_chars);
        else if (i == kName) f = scripted::wrong_name(f);
        else if (i == kBare) f = scripted::bare(srpc::RPC_ERR_FUNCTION_NOT_REGISTERED);
        else if (i == kEmpty) f = scripted::empty();
        replies.insert(replies.end(), f.begin(), f.end());
        if (i < batch) sent += d.frame(i).size();
    }
    int sv[2];
    if (socketpair(AF_UNIX, SOCK_STREAM, 0, sv) != 0) std::exit(2);
    std::thread peer = scripted::answer_at_once(sv[1], batch, replies);
    {
        srpc::gpu::batch_client cl(sv[0], batch);
        const srpc::gpu::call_stats st = cl.call_mixed(d.legs(cl), d.d_method, n, d.d_codes, srpc::gpu::var_call_limits{});
        d.fetch_codes();
        CHECK(d.hcodes[kCode] == srpc::RPC_ERR_RECV_TIMEOUT);
        d.hcodes[kCode] = srpc::RPC_SUCCESS;  // its fields are decoded like any full frame's: checked below
        HIPCHECK(hipMemcpy(d.d_codes + kCode, &d.hcodes[kCode], 1, hipMemcpyHostToDevice));
        check_replies(d, n, false, bad);
        CHECK(st.calls == n && st.ok == n - 5 && st.failed == 2 && st.malformed == 3 && st.unanswered == 0);
        CHECK(st.chunks == 3 && st.uniform_chunks == 0);
        // the later chunks' replies were there before their requests could leave
        CHECK(st.received_bytes == replies.size() && st.sent_bytes == sent);
    }
    close(sv[0]);
    peer.join();
}

int main() {
    // the scalar peer decodes requests with packer::unpack_request
    srpc::message_registry["Number"] = []() -> std::unique_ptr<Number> { return std::make_unique<Number>(); };
    srpc::message_registry["TwoNumbers"] = []() -> std::unique_ptr<TwoNumbers> { return std::make_unique<TwoNumbers>(); };
    srpc::message_registry["Text"] = []() -> std::unique_ptr<Text> { return std::make_unique<Text>(); };
    srpc::message_registry["multiple_primitives"] = []() -> std::unique_ptr<MP> { return std::make_unique<MP>(); };
    all_legs_in_call_order();
    resp_cap_one_byte_short();
    send_buffer_too_small();
    a_leg_one_call_short();
    peer_closes_after_half();
    flagged_middle_chunk();
    std::printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
