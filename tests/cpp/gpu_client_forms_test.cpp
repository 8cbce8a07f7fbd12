// needs: gpu
// One srpc::gpu::batch_client (include/srpc/gpu_client.hpp) making every form of
// call on one connection to a batch_server (mixed_var_fixture.hpp: square and
// add fixed, echo and twice string-bodied), 40 calls in chunks of 16, 16 and 8
// each: call, call_var, call_mixed over fixed legs, call_mixed with string legs,
// call again, and call_var with larger var_call_limits -- the staging grows
// after the var and mixed staging exists, is released and re-created whole, and
// every form still finds what it needs.  Codes, fields, strings and stats are
// checked as the per-form tests check them.
#include "mixed_var_fixture.hpp"

constexpr uint64_t kCalls = 40, kChunk = 16;

struct device_codes {
    uint8_t* d = nullptr;
    std::vector<uint8_t> h;
    explicit device_codes(uint64_t n) : h(n) {
        HIPCHECK(hipMalloc(reinterpret_cast<void**>(&d), n + 16));
        HIPCHECK(hipMemset(d, 0xA5, n + 16));
    }
    bool all(uint8_t code) {
        HIPCHECK(hipMemcpy(h.data(), d, h.size(), hipMemcpyDeviceToHost));
        bool ok = true;
        for (uint8_t c : h) ok = ok && c == code;
        return ok;
    }
    ~device_codes() { (void)hipFree(d); }
};

// `call`: square, every reply full (the uniform decode)
static void fixed_call(srpc::gpu::batch_client& cl, uint64_t seed) {
    leg_data<Number, Number> sq;
    sq.in.resize(kCalls);
    for (uint64_t i = 0; i < kCalls; ++i) sq.in[i].num = value(i * 3 + seed);
    sq.upload(0);
    device_codes codes(kCalls);
    const srpc::gpu::call_stats st = cl.call<Number, Number>(kMethods[0], sq.req.data(), kCalls, sq.resp.data(), codes.d);
    std::vector<Number> got;
    CHECK(sq.fetch(got));
    if (g_fail) return;
    bool right = codes.all(srpc::RPC_SUCCESS);
    for (uint64_t i = 0; i < kCalls; ++i) right = right && got[i].num == compute(0, sq.in[i].num, 0);
    CHECK(right);
    CHECK(st.calls == kCalls && st.ok == kCalls && st.failed == 0 && st.malformed == 0 && st.unanswered == 0);
    CHECK(st.chunks == 3 && st.uniform_chunks == 3);
    CHECK(st.sent_bytes == kCalls * 57 && st.received_bytes == kCalls * 23);
    CHECK(cl.last_stats().ok == st.ok && cl.last_stats().chunks == 3);
}

// `call_var`: echo, offsets absolute over the three chunks, the column filled to the byte
static void var_call(srpc::gpu::batch_client& cl, uint64_t seed, srpc::gpu::var_call_limits lim) {
    leg_data<MP, MP> ec;
    ec.in.resize(kCalls);
    uint64_t chars = 0, sent = 0, received = 0;
    const uint64_t rq = srpc::gpu::request_prefix<MP>(kMethods[2]).size(),
                   rs = srpc::gpu::response_prefix<MP>(srpc::RPC_SUCCESS).size();
    for (uint64_t i = 0; i < kCalls; ++i) {
        echo_fixture::fill_request(ec.in[i], i + seed);
        chars += ec.in[i].arg4.size() + 1;  // the answer appends "!"
        sent += 4 + rq + 18 + ec.in[i].arg4.size();
        received += 4 + rs + 18 + ec.in[i].arg4.size() + 1;
    }
    ec.upload(chars);
    device_codes codes(kCalls);
    const srpc::gpu::call_stats st = cl.call_var<MP, MP>(kMethods[2], ec.req.data(), ec.req_offs.data(), kCalls,
                                                         ec.resp.data(), ec.resp_offs.data(), ec.cap.data(), codes.d, lim);
    std::vector<MP> got;
    CHECK(ec.fetch(got));
    if (g_fail) return;
    bool right = codes.all(srpc::RPC_SUCCESS);
    for (uint64_t i = 0; i < kCalls; ++i) right = right && same(got[i], echo_fixture::answer(ec.in[i]));
    CHECK(right);
    CHECK(ec.raw_offs[3][kCalls] == chars && ec.raw_offs[3][kChunk] > 0 && ec.raw_offs[3][2 * kChunk] > ec.raw_offs[3][kChunk]);
    CHECK(st.calls == kCalls && st.ok == kCalls && st.failed == 0 && st.malformed == 0 && st.unanswered == 0);
    CHECK(st.chunks == 3 && st.uniform_chunks == 0);
    CHECK(st.sent_bytes == sent && st.received_bytes == received);
}

// `call_mixed` over fixed legs: square, add, and divide (which the server does not know)
static void fixed_mixed_call(srpc::gpu::batch_client& cl) {
    leg_data<Number, Number> sq;
    leg_data<TwoNumbers, Number> ad, dv;
    std::vector<uint8_t> method(kCalls);
    std::vector<uint32_t> rank(kCalls);
    uint64_t count[3] = {};
    for (uint64_t i = 0; i < kCalls; ++i) {
        method[i] = static_cast<uint8_t>((i * 7 + i / 5) % 3);
        rank[i] = static_cast<uint32_t>(count[method[i]]++);
    }
    sq.in.resize(count[0]), ad.in.resize(count[1]), dv.in.resize(count[2]);
    for (uint64_t r = 0; r < count[0]; ++r) sq.in[r].num = value(r * 11 + 2);
    for (uint64_t r = 0; r < count[1]; ++r) ad.in[r].left = value(r * 5 + 1), ad.in[r].right = value(r * 31 + 8);
    for (uint64_t r = 0; r < count[2]; ++r) dv.in[r].left = value(r * 5 + 4), dv.in[r].right = value(r * 31 + 29);
    sq.upload(0), ad.upload(0), dv.upload(0);
    uint8_t* d_method = nullptr;
    HIPCHECK(hipMalloc(reinterpret_cast<void**>(&d_method), kCalls + 16));
    HIPCHECK(hipMemcpy(d_method, method.data(), kCalls, hipMemcpyHostToDevice));
    device_codes codes(kCalls);
    std::vector<srpc::gpu::mixed_leg> legs;
    legs.push_back(cl.leg<Number, Number>(kMethods[0], sq.req.data(), sq.resp.data(), count[0]));
    legs.push_back(cl.leg<TwoNumbers, Number>(kMethods[1], ad.req.data(), ad.resp.data(), count[1]));
    legs.push_back(cl.leg<TwoNumbers, Number>(kMethods[4], dv.req.data(), dv.resp.data(), count[2]));
    const srpc::gpu::call_stats st = cl.call_mixed(legs, d_method, kCalls, codes.d);
    std::vector<Number> gs, ga, gd;
    CHECK(sq.fetch(gs));
    CHECK(ad.fetch(ga));
    CHECK(dv.fetch(gd));
    (void)codes.all(0);
    (void)hipFree(d_method);
    if (g_fail) return;
    bool right = true;
    for (uint64_t i = 0; i < kCalls; ++i) {
        const uint32_t r = rank[i];
        if (method[i] == 0) right = right && codes.h[i] == srpc::RPC_SUCCESS && gs[r].num == compute(0, sq.in[r].num, 0);
        else if (method[i] == 1)
            right = right && codes.h[i] == srpc::RPC_SUCCESS && ga[r].num == compute(1, ad.in[r].left, ad.in[r].right);
        else right = right && codes.h[i] == srpc::RPC_ERR_FUNCTION_NOT_REGISTERED && gd[r].num == 0;
    }
    CHECK(right);
    CHECK(count[0] > 0 && count[1] > 0 && count[2] > 0);
    CHECK(st.calls == kCalls && st.chunks == 3 && st.uniform_chunks == 0);
    CHECK(st.ok == count[0] + count[1] && st.failed == count[2] && st.malformed == 0 && st.unanswered == 0);
    CHECK(st.sent_bytes == count[0] * 57 + count[1] * 62 + count[2] * 65);
    CHECK(st.received_bytes == (count[0] + count[1]) * 23 + count[2] * 5);
}

// `call_mixed` with string legs: the seven legs of gpu_client_mixed_var_test.cpp
static void string_mixed_call(srpc::gpu::batch_client& cl) {
    mixed_calls d(kCalls);
    uint64_t sent = 0;
    for (uint64_t i = 0; i < kCalls; ++i) sent += d.frame(i).size();
    const srpc::gpu::call_stats st = cl.call_mixed(d.legs(cl), d.d_method, kCalls, d.d_codes, srpc::gpu::var_call_limits{});
    check_replies(d, kCalls);
    if (g_fail) return;
    CHECK(d.echo.raw_offs[3][d.count[2]] == d.echo.cap[3]);
    CHECK(d.text.raw_offs[0][d.count[3]] + d.text.raw_offs[1][d.count[3]] == d.text.cap[0]);
    CHECK(st.calls == kCalls && st.chunks == 3 && st.uniform_chunks == 0);
    CHECK(st.ok + st.failed == kCalls && st.failed == d.count[4] + d.count[5] + d.count[6] && st.malformed == 0 &&
          st.unanswered == 0);
    CHECK(st.sent_bytes == sent);
}

int main() {
    served_pair sp;
    {
        srpc::gpu::batch_client cl(sp.fd, kChunk);
        fixed_call(cl, 0);
        var_call(cl, 0, srpc::gpu::var_call_limits{});
        fixed_mixed_call(cl);
        string_mixed_call(cl);
        fixed_call(cl, 1000);
        // 16 * 2048 + 4096 bytes a side: the staging grows with the var and mixed staging in place
        var_call(cl, 1000, srpc::gpu::var_call_limits{2048, 2048});
        string_mixed_call(cl);
    }
    sp.finish();
    CHECK(sp.stats.requests == 7 * kCalls);
    std::printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
