// needs: gpu
// srpc::gpu::batch_client::call_legs (include/srpc/gpu_client.hpp) against a
// srpc::gpu::batch_server with column, record and string-bodied methods on the
// two ends of a socketpair: one ordered batch over square (column leg), add
// (record leg), subtract (column leg), multiply (record leg) and echo (a
// string-bodied leg), packed in call order by
// srpc_frames_pack_requests_mixed_legs and decoded by
// srpc_frames_unpack_replies_mixed_legs.
// Checked: every reply struct byte for byte (the leaf the host computes, every
// other byte the proto's), every column, string, code and call_stats field; the
// same calls through column legs and call_mixed (equal values and counts);
// every tenth call rewritten to a method the server does not know; a peer that
// closes five replies into the second chunk; call_mixed given the same legs
// still throws SRPC_E_UNSUPPORTED with nothing sent.
#include <cerrno>
#include <string>

#include "mixed_var_fixture.hpp"  // the messages, leg_data, calc_batch, echo_batch, value
#include "served_socketpair.hpp"

constexpr uint64_t kChunk = 1024, kCalls = 5000;
constexpr int kN = 5;
static const std::array<std::string, kN> kNames = {"Calculator_servicer::square", "Calculator_servicer::add",
                                                   "Calculator_servicer::subtract", "Calculator_servicer::multiply",
                                                   echo_fixture::kMethod};

// two's-complement arithmetic without signed overflow
static int32_t calc(int op, int32_t l, int32_t r) {
    const uint32_t a = static_cast<uint32_t>(l), b = static_cast<uint32_t>(r);
    const uint32_t v = op == 0 ? a * a : op == 1 ? a + b : op == 2 ? a - b : a * b;
    return static_cast<int32_t>(v);
}

static int subtract_batch(void* const* rq, void* const* rs, uint64_t n, hipStream_t s) {
    std::vector<int32_t> l(n), r(n), out(n);
    if (hipStreamSynchronize(s) != hipSuccess) return SRPC_E_HIP;
    if (hipMemcpy(l.data(), rq[0], 4 * n, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    if (hipMemcpy(r.data(), rq[1], 4 * n, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    for (uint64_t i = 0; i < n; ++i) out[i] = calc(2, l[i], r[i]);
    return hipMemcpy(rs[0], out.data(), 4 * n, hipMemcpyHostToDevice) == hipSuccess ? 0 : SRPC_E_HIP;
}

// A record method through the host: the Resp array arrives zeroed and only its leaf is written.
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
        const int32_t v = calc(OP, a, b);
        std::memcpy(out.data() + i * sizeof(Number) + ro, &v, 4);
    }
    return hipMemcpy(r, out.data(), out.size(), hipMemcpyHostToDevice) == hipSuccess ? 0 : SRPC_E_HIP;
}

static void register_all(srpc::gpu::batch_server& srv) {
    srv.register_method<Number, Number>(kNames[0], calc_batch<0>);
    srv.register_record_method<TwoNumbers, Number>(kNames[1], record_batch<1>);
    srv.register_method<TwoNumbers, Number>(kNames[2], subtract_batch);
    srv.register_record_method<TwoNumbers, Number>(kNames[3], record_batch<3>);
    srv.register_var_method<MP, MP>(kNames[4], echo_batch);
}

struct legs_pair : served_socketpair {
    legs_pair() : served_socketpair(kChunk, register_all) {}
};

// A proto whose every byte outside the leaf is told apart from zero and from
// the 0xA5 the reply arrays start with (the vtable pointer stays).
static Number marked_proto() {
    Number proto;
    auto* b = reinterpret_cast<uint8_t*>(&proto);
    const uint32_t leaf = srpc::gpu::leaf_offsets<Number>()[0];
    for (size_t k = sizeof(void*); k < sizeof(Number); ++k)
        if (k < leaf || k >= leaf + 4) b[k] = static_cast<uint8_t>(0xC0 + k);
    return proto;
}

// n calls in a fixed pseudo-random order over the five methods.  Every fixed
// method has its calls in columns (leg_data) and, add and multiply, as arrays
// of structs: the requests the host records themselves, the replies 0xA5 with
// 16 guard bytes behind.
struct legs_calls {
    uint64_t n;
    std::vector<uint8_t> method, hcodes;
    std::vector<uint32_t> rank;
    std::array<uint64_t, kN> count{};
    leg_data<Number, Number> square;
    std::array<leg_data<TwoNumbers, Number>, 3> two;  // add, subtract, multiply
    leg_data<MP, MP> echo;
    std::array<void*, 2> d_req{}, d_resp{};           // add, multiply
    std::array<std::vector<uint8_t>, 2> structs;      // fetch_structs(): the reply arrays with their guards
    uint8_t *d_method = nullptr, *d_codes = nullptr;
    Number proto = marked_proto();

    explicit legs_calls(uint64_t n) : n(n), method(n), hcodes(n + 16), rank(n) {
        uint32_t x = 2463534242u;
        for (uint64_t i = 0; i < n; ++i) {
            x ^= x << 13, x ^= x >> 17, x ^= x << 5;
            method[i] = static_cast<uint8_t>(x % kN);
            rank[i] = static_cast<uint32_t>(count[method[i]]++);
        }
        square.in.resize(count[0]);
        for (uint64_t r = 0; r < count[0]; ++r) square.in[r].num = value(r * 5);
        for (int t = 0; t < 3; ++t) {
            two[t].in.resize(count[1 + t]);
            for (uint64_t r = 0; r < count[1 + t]; ++r)
                two[t].in[r].left = value(r * 5 + 1 + t), two[t].in[r].right = value(r * 31 + 8 + 7 * t);
        }
        echo.in.resize(count[4]);
        uint64_t chars = 0;
        for (uint64_t r = 0; r < count[4]; ++r) {
            echo_fixture::fill_request(echo.in[r], r);
            chars += echo.in[r].arg4.size() + 1;  // the answer appends "!"
        }
        square.upload(0);
        for (auto& l : two) l.upload(0);
        echo.upload(chars);  // exact: nothing to spare
        for (int t = 0; t < 2; ++t) {
            auto const& in = two[2 * t].in;
            HIPCHECK(hipMalloc(&d_req[t], in.size() * sizeof(TwoNumbers) + 16));
            HIPCHECK(hipMalloc(&d_resp[t], in.size() * sizeof(Number) + 16));
            HIPCHECK(hipMemcpy(d_req[t], static_cast<const void*>(in.data()), in.size() * sizeof(TwoNumbers), hipMemcpyHostToDevice));
            HIPCHECK(hipMemset(d_resp[t], 0xA5, in.size() * sizeof(Number) + 16));
        }
        HIPCHECK(hipMalloc(reinterpret_cast<void**>(&d_method), n + 16));
        HIPCHECK(hipMalloc(reinterpret_cast<void**>(&d_codes), n + 16));
        HIPCHECK(hipMemcpy(d_method, method.data(), n, hipMemcpyHostToDevice));
        HIPCHECK(hipMemset(d_codes, 0xA5, n + 16));
    }
    srpc::gpu::mixed_leg echo_leg(srpc::gpu::batch_client& cl) {
        return cl.leg_var<MP, MP>(kNames[4], echo.req.data(), echo.req_offs.data(), echo.resp.data(), echo.resp_offs.data(),
                                  echo.cap.data(), count[4]);
    }
    // square and subtract in columns, add and multiply in records, echo string-bodied
    std::vector<srpc::gpu::mixed_leg> mixed_legs(srpc::gpu::batch_client& cl) {
        std::vector<srpc::gpu::mixed_leg> l;
        l.push_back(cl.leg<Number, Number>(kNames[0], square.req.data(), square.resp.data(), count[0]));
        l.push_back(cl.leg_records<TwoNumbers, Number>(kNames[1], static_cast<const TwoNumbers*>(d_req[0]),
                                                       static_cast<Number*>(d_resp[0]), count[1], proto));
        l.push_back(cl.leg<TwoNumbers, Number>(kNames[2], two[1].req.data(), two[1].resp.data(), count[2]));
        l.push_back(cl.leg_records<TwoNumbers, Number>(kNames[3], static_cast<const TwoNumbers*>(d_req[1]),
                                                       static_cast<Number*>(d_resp[1]), count[3], proto));
        l.push_back(echo_leg(cl));
        return l;
    }
    std::vector<srpc::gpu::mixed_leg> column_legs(srpc::gpu::batch_client& cl) {
        std::vector<srpc::gpu::mixed_leg> l;
        l.push_back(cl.leg<Number, Number>(kNames[0], square.req.data(), square.resp.data(), count[0]));
        for (int t = 0; t < 3; ++t)
            l.push_back(cl.leg<TwoNumbers, Number>(kNames[1 + t], two[t].req.data(), two[t].resp.data(), count[1 + t]));
        l.push_back(echo_leg(cl));
        return l;
    }
    void fetch_structs() {
        for (int t = 0; t < 2; ++t) {
            structs[t].resize(count[1 + 2 * t] * sizeof(Number) + 16);
            HIPCHECK(hipMemcpy(structs[t].data(), d_resp[t], structs[t].size(), hipMemcpyDeviceToHost));
        }
        HIPCHECK(hipMemcpy(hcodes.data(), d_codes, n + 16, hipMemcpyDeviceToHost));
    }
    // record reply r of add (t = 0) or multiply (t = 1) is the proto with `num`, every byte
    bool struct_is(int t, uint32_t r, int32_t num) const {
        std::vector<uint8_t> want(reinterpret_cast<const uint8_t*>(&proto), reinterpret_cast<const uint8_t*>(&proto) + sizeof(Number));
        std::memcpy(want.data() + srpc::gpu::leaf_offsets<Number>()[0], &num, 4);
        return std::memcmp(structs[t].data() + r * sizeof(Number), want.data(), sizeof(Number)) == 0;
    }
    bool guards() const {
        bool ok = true;
        for (int t = 0; t < 2; ++t)
            for (uint64_t b = 0; b < 16; ++b) ok = ok && structs[t][count[1 + 2 * t] * sizeof(Number) + b] == 0xA5;
        for (uint64_t b = 0; b < 16; ++b) ok = ok && hcodes[n + b] == 0xA5;
        return ok;
    }
    // what the service answers call i with
    int32_t number(uint64_t i) const {
        const int k = method[i];
        const uint32_t r = rank[i];
        return k == 0 ? calc(0, square.in[r].num, 0) : calc(k, two[k - 1].in[r].left, two[k - 1].in[r].right);
    }
    ~legs_calls() {
        for (void* p : {d_req[0], d_req[1], d_resp[0], d_resp[1]}) (void)hipFree(p);
        (void)hipFree(d_method);
        (void)hipFree(d_codes);
    }
};

static bool same_mp(MP const& a, MP const& b) {
    return a.arg1 == b.arg1 && a.arg2 == b.arg2 && a.arg3 == b.arg3 && a.arg4 == b.arg4;
}

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

// Every value a batch left behind, against `answered(i)` (the call got the
// service's reply) and `code(i)`: records byte for byte, columns, strings.
// records: add and multiply were record legs (else their columns are checked).
template <class A, class C>
static void check_values(legs_calls& d, bool records, A answered, C code) {
    d.fetch_structs();
    std::vector<Number> sq, sub, add, mul;
    std::vector<MP> ec;
    CHECK(d.square.fetch(sq));
    CHECK(d.two[1].fetch(sub));
    CHECK(d.echo.fetch(ec));
    if (!records) {
        CHECK(d.two[0].fetch(add));
        CHECK(d.two[2].fetch(mul));
    }
    bool structs = true, columns = true, strings = true, codes = true;
    for (uint64_t i = 0; i < d.n; ++i) {
        const int k = d.method[i];
        const uint32_t r = d.rank[i];
        const bool a = answered(i);
        const int32_t num = a && k < 4 ? d.number(i) : 0;
        if (k == 0) columns = columns && sq[r].num == num;
        else if (k == 2) columns = columns && sub[r].num == num;
        else if (k == 4) strings = strings && same_mp(ec[r], a ? echo_fixture::answer(d.echo.in[r]) : MP{});
        else if (records) structs = structs && d.struct_is(k == 3, r, num);
        else columns = columns && (k == 1 ? add : mul)[r].num == num;
        codes = codes && d.hcodes[i] == code(i);
    }
    CHECK(structs);
    CHECK(columns);
    CHECK(strings);
    CHECK(codes);
    CHECK(d.guards());
}

static void all_three_kinds_in_call_order() {
    legs_calls d(kCalls);
    for (int k = 0; k < kN; ++k) CHECK(d.count[k] > 800);
    srpc::gpu::call_stats st, stc;
    {
        legs_pair sp;
        srpc::gpu::batch_client cl(sp.fd, kChunk);
        st = cl.call_legs(d.mixed_legs(cl), d.d_method, kCalls, d.d_codes);
        sp.finish();
        CHECK(sp.thrown == 0 && sp.stats.requests == kCalls);
    }
    check_values(d, true, [](uint64_t) { return true; }, [](uint64_t) { return srpc::RPC_SUCCESS; });
    CHECK(st.calls == kCalls && st.chunks == 5 && st.ok == kCalls && st.failed == 0 && st.malformed == 0 &&
          st.unanswered == 0 && st.sent_bytes > 0 && st.received_bytes > 0);
    // the same calls through column legs and call_mixed: the same values, codes and counts
    const std::vector<uint8_t> codes = d.hcodes;
    HIPCHECK(hipMemset(d.d_codes, 0xA5, kCalls + 16));
    {
        legs_pair sp;
        srpc::gpu::batch_client cl(sp.fd, kChunk);
        stc = cl.call_mixed(d.column_legs(cl), d.d_method, kCalls, d.d_codes, srpc::gpu::var_call_limits{});
        sp.finish();
    }
    check_values(d, false, [](uint64_t) { return true; }, [](uint64_t) { return srpc::RPC_SUCCESS; });
    CHECK(d.hcodes == codes);
    CHECK(st.calls == stc.calls && st.ok == stc.ok && st.failed == stc.failed && st.malformed == stc.malformed &&
          st.unanswered == stc.unanswered && st.chunks == stc.chunks && st.uniform_chunks == stc.uniform_chunks &&
          st.sent_bytes == stc.sent_bytes && st.received_bytes == stc.received_bytes);
    // ... and through column legs and call_legs itself: all of one kind is a valid call
    HIPCHECK(hipMemset(d.d_codes, 0xA5, kCalls + 16));
    {
        legs_pair sp;
        srpc::gpu::batch_client cl(sp.fd, kChunk);
        stc = cl.call_legs(d.column_legs(cl), d.d_method, kCalls, d.d_codes);
        sp.finish();
    }
    check_values(d, false, [](uint64_t) { return true; }, [](uint64_t) { return srpc::RPC_SUCCESS; });
    CHECK(d.hcodes == codes && stc.ok == kCalls && stc.sent_bytes == st.sent_bytes);
}

static void every_tenth_call_unknown() {
    uint64_t n_unknown = 0;
    for (uint64_t i = 0; i < kCalls; ++i) n_unknown += unknown(i);
    legs_calls d(kCalls);
    srpc::gpu::call_stats st;
    {
        legs_pair sp;
        srpc::gpu::batch_client cl(sp.fd, kChunk);
        cl.set_request_hook(rewrite_every_tenth);
        st = cl.call_legs(d.mixed_legs(cl), d.d_method, kCalls, d.d_codes);
        sp.finish();
        CHECK(sp.stats.requests == kCalls && sp.stats.fallback_requests == n_unknown);
    }
    check_values(d, true, [](uint64_t i) { return !unknown(i); },
                 [](uint64_t i) { return unknown(i) ? srpc::RPC_ERR_FUNCTION_NOT_REGISTERED : srpc::RPC_SUCCESS; });
    CHECK(st.calls == kCalls && st.chunks == 5 && st.malformed == 0 && st.unanswered == 0);
    CHECK(st.ok == kCalls - n_unknown && st.failed == n_unknown);
}

// A peer that answers 1029 frames (five replies into the second chunk) and
// closes: echo with the service's answer, every other method with a Number
// holding the request's last int32.  The calls after them get
// RPC_ERR_RECV_TIMEOUT, the proto with a zero leaf, zero fields, empty strings.
static void peer_closes_in_the_second_chunk() {
    constexpr uint64_t n = 3000, answered = kChunk + 5;
    int sv[2];
    if (socketpair(AF_UNIX, SOCK_STREAM, 0, sv) != 0) std::exit(2);
    std::thread peer([fd = sv[1]] {
        std::vector<uint8_t> in;
        uint8_t tmp[4096];
        uint64_t done = 0, at = 0;
        bool open = true;
        auto u64 = [&in](uint64_t o) {
            uint64_t v;
            std::memcpy(&v, in.data() + o, 8);
            return v;
        };
        while (true) {
            const ssize_t k = recv(fd, tmp, sizeof tmp, 0);
            if (k <= 0) break;
            in.insert(in.end(), tmp, tmp + k);
            while (open && in.size() - at >= 4) {
                const uint64_t len = 4 + ((uint64_t{in[at]} << 24) | (uint64_t{in[at + 1]} << 16) |
                                          (uint64_t{in[at + 2]} << 8) | uint64_t{in[at + 3]});
                if (in.size() - at < len) break;
                // BE32 | u64 | method | u64 | Req::name | fields
                const uint64_t mlen = u64(at + 4);
                const std::string method(reinterpret_cast<const char*>(in.data() + at + 12), mlen);
                const uint64_t body = at + 12 + mlen + 8 + u64(at + 12 + mlen);
                srpc::packer p;
                if (method == echo_fixture::kMethod) {
                    MP q;
                    q.arg1 = static_cast<int8_t>(in[body]);
                    q.arg2 = static_cast<char>(in[body + 1]);
                    std::memcpy(&q.arg3, in.data() + body + 2, 8);
                    q.arg4.assign(reinterpret_cast<const char*>(in.data() + body + 18), u64(body + 10));
                    srpc::response_t<MP> r;
                    r.set_value(echo_fixture::answer(q));
                    p.pack_response(r);
                } else {
                    Number num;
                    std::memcpy(&num.num, in.data() + at + len - 4, 4);
                    srpc::response_t<Number> r;
                    r.set_value(num);
                    p.pack_response(r);
                }
                at += len;
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
        legs_calls d(n);
        srpc::gpu::batch_client cl(sv[0], kChunk);
        const srpc::gpu::call_stats st = cl.call_legs(d.mixed_legs(cl), d.d_method, n, d.d_codes);
        d.fetch_structs();
        std::vector<Number> sq, sub;
        std::vector<MP> ec;
        CHECK(d.square.fetch(sq));
        CHECK(d.two[1].fetch(sub));
        CHECK(d.echo.fetch(ec));
        bool structs = true, columns = true, strings = true, codes = true;
        for (uint64_t i = 0; i < n; ++i) {
            const int k = d.method[i];
            const uint32_t r = d.rank[i];
            const bool a = i < answered;
            const int32_t last = !a || k == 4 ? 0 : k == 0 ? d.square.in[r].num : d.two[k - 1].in[r].right;
            if (k == 0) columns = columns && sq[r].num == last;
            else if (k == 2) columns = columns && sub[r].num == last;
            else if (k == 4) strings = strings && same_mp(ec[r], a ? echo_fixture::answer(d.echo.in[r]) : MP{});
            else structs = structs && d.struct_is(k == 3, r, last);
            codes = codes && d.hcodes[i] == (a ? srpc::RPC_SUCCESS : srpc::RPC_ERR_RECV_TIMEOUT);
        }
        CHECK(structs);
        CHECK(columns);
        CHECK(strings);
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

static void call_mixed_is_unchanged() {
    int sv[2];
    if (socketpair(AF_UNIX, SOCK_STREAM, 0, sv) != 0) std::exit(2);
    {
        legs_calls d(100);
        srpc::gpu::batch_client cl(sv[0], kChunk);
        const std::vector<srpc::gpu::mixed_leg> legs = d.mixed_legs(cl);
        CHECK(thrown([&] { (void)cl.call_mixed(legs, d.d_method, 100, d.d_codes); }) == SRPC_E_UNSUPPORTED);
        CHECK(thrown([&] { (void)cl.call_mixed(legs, d.d_method, 100, d.d_codes, srpc::gpu::var_call_limits{}); }) ==
              SRPC_E_UNSUPPORTED);
        uint8_t byte;
        CHECK(recv(sv[1], &byte, 1, MSG_DONTWAIT) < 0 && (errno == EAGAIN || errno == EWOULDBLOCK));  // nothing was sent
        // call_legs keeps call_mixed's argument checks
        CHECK(thrown([&] { (void)cl.call_legs({}, d.d_method, 100, d.d_codes); }) == SRPC_E_INVALID);
        CHECK(thrown([&] { (void)cl.call_legs(legs, nullptr, 100, d.d_codes); }) == SRPC_E_INVALID);
        CHECK(recv(sv[1], &byte, 1, MSG_DONTWAIT) < 0 && (errno == EAGAIN || errno == EWOULDBLOCK));
    }
    close(sv[0]);
    close(sv[1]);
    // a record leg declaring fewer calls than d_method holds: met in the second chunk, of which nothing is sent
    constexpr uint64_t n = 2000;
    legs_pair sp;
    legs_calls d(n);
    {
        srpc::gpu::batch_client cl(sp.fd, kChunk);
        std::vector<srpc::gpu::mixed_leg> legs = d.mixed_legs(cl);
        legs[1].calls -= 1;
        CHECK(thrown([&] { (void)cl.call_legs(legs, d.d_method, n, d.d_codes); }) == SRPC_E_INVALID);
    }
    sp.finish();
    CHECK(sp.stats.requests == kChunk);
}

int main() {
    HIPCHECK(hipSetDevice(0));
    CHECK(sizeof(TwoNumbers) == 16 && sizeof(Number) == 16);
    all_three_kinds_in_call_order();
    every_tenth_call_unknown();
    peer_closes_in_the_second_chunk();
    call_mixed_is_unchanged();
    std::printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
