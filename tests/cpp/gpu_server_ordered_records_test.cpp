// needs: gpu
// srpc::gpu::batch_server in ordered records mode (include/srpc/gpu_server.hpp:
// set_ordered_records, set_ordered_records_handler): record methods -- handlers
// over device arrays of the caller's own structs -- served in arrival order,
// over a socketpair, the peer being this program's own frames from
// srpc::packer:
//   (a) per-method record handlers, lock-step batches of 16: each handler
//       appends its requests' keys to a log in device memory; the log is the
//       method's frames in arrival order across batches (what the bucket route,
//       whose buckets are filled with atomics, does not give), every reply byte
//       for byte, and every non-leaf byte of every Req seen a Req{}'s (Entry has
//       padding and a defaulted member that is no leaf);
//   (b) one ordered_records_handler for a ledger whose running sum every
//       method's requests add to, in device memory across batches: 5000 frames
//       over three methods, every tenth a method only the CPU fallback server
//       knows, answered in its place after the handler; every reply equals the
//       host's replay of the trace;
//   (c) one server served three times -- ordered records, set_ordered_records
//       (false) (the bucket route), ordered records again -- on the same frames
//       of stateless methods: the same reply bytes, consistent counters;
//   (d) the refusals: a column method, a string method or a Req above 256 bytes
//       beside record methods; set_ordered / set_ordered_var with record methods.
// The handlers work through the host (this program is host code): they wait for
// the server's stream, copy the batch's structs out, compute, and copy back.
#include <hip/hip_runtime_api.h>
#include <srpc/gpu_server.hpp>
#include <srpc/packer.hpp>
#include <srpc/server.hpp>
#include <sys/socket.h>
#include <sys/time.h>
#include <unistd.h>

#include <array>
#include <cstdio>
#include <cstring>
#include <functional>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "echo_records.hpp"
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

using bytes = std::vector<uint8_t>;

// 32 bytes: vtable slot, tag at 8, three bytes of padding, key at 12, amount at
// 16, then a member that is no leaf and has a default, and four bytes of padding.
struct Entry : public srpc::message_base {
    int8_t tag = 0;
    int32_t key = 0;
    int64_t amount = 0;
    uint32_t epoch = 0xC0FFEE11u;  // not on the wire
    static constexpr const char* name = "Entry";
    static constexpr auto fields = std::make_tuple(STRUCT_MEMBER(Entry, tag, "Entry::tag"), STRUCT_MEMBER(Entry, key, "Entry::key"),
                                                   STRUCT_MEMBER(Entry, amount, "Entry::amount"));
};

struct Number : public srpc::message_base {
    int32_t num = 0;
    static constexpr const char* name = "Number";
    static constexpr auto fields = std::make_tuple(STRUCT_MEMBER(Number, num, "Number::num"));
    void unpack(srpc::buffer::ptr bp) override { srpc::packer p(bp); p >> num; }
};

struct Balance : public srpc::message_base {  // 24 bytes: every other struct of an array starts off a 16-byte boundary
    int64_t sum = 0;
    int32_t key = 0;
    static constexpr const char* name = "Balance";
    static constexpr auto fields =
        std::make_tuple(STRUCT_MEMBER(Balance, sum, "Balance::sum"), STRUCT_MEMBER(Balance, key, "Balance::key"));
};

// 264 bytes: a Req the ordered records route does not take
#define BIG_FIELDS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) \
    X(17) X(18) X(19) X(20) X(21) X(22) X(23) X(24) X(25) X(26) X(27) X(28) X(29) X(30)
struct Big : public srpc::message_base {
#define X(i) int64_t v##i = 0;
    BIG_FIELDS(X) int64_t v31 = 0;
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

static const std::string kDeposit = "Ledger_servicer::deposit", kWithdraw = "Ledger_servicer::withdraw",
                         kBump = "Ledger_servicer::bump", kClose = "Ledger_servicer::close";

// The CPU server's only method: what the GPU side does not register.
struct Closer_servicer : srpc::servicer_base {
    Number close(Number& q) {
        Number r;
        r.num = static_cast<int32_t>(static_cast<uint32_t>(q.num) + 1000u);
        return r;
    }
    static constexpr const char* name = "Ledger";
    static constexpr auto methods = std::make_tuple(STRUCT_MEMBER(Closer_servicer, close, "Ledger_servicer::close"));
};

template <class Req>
static bytes request(std::string const& method, Req const& v) {
    srpc::packer p;
    srpc::request_t<Req> q;
    q.set_method_name(method);
    q.set_value(v);
    p.pack_request(q);
    bytes f = srpc::gpu::be32(static_cast<uint32_t>(p.size()));
    f.insert(f.end(), p.data(), p.data() + p.size());
    return f;
}
template <class Resp>
static bytes reply(Resp const& value) {
    srpc::packer p;
    srpc::response_t<Resp> r;
    r.set_code(srpc::RPC_SUCCESS);
    r.set_value(value);
    p.pack_response(r);
    bytes f = srpc::gpu::be32(static_cast<uint32_t>(p.size()));
    f.insert(f.end(), p.data(), p.data() + p.size());
    return f;
}

static uint64_t rnd(uint64_t i) {
    uint64_t s = echo_fixture::kSeed + i * 0xD1B54A32D192ED03ull;
    return echo_fixture::next(s);
}
// Request i of an Entry method: a key that is never 0 (the warm-up's zero record is told apart) and tells i.
static Entry entry(uint64_t i) {
    const uint64_t z = rnd(i);
    Entry q;
    q.tag = static_cast<int8_t>(z);
    q.key = static_cast<int32_t>(i + 1);
    q.amount = static_cast<int64_t>(z >> 8);
    return q;
}
static Number number(uint64_t i) {
    Number q;
    q.num = static_cast<int32_t>(i + 1);
    return q;
}

// The bytes of a T{} that are no leaf and no padding: the vtable slot, and Entry's defaulted member.
template <class T>
static std::vector<std::pair<size_t, size_t>> named_non_leaf_bytes() {
    std::vector<std::pair<size_t, size_t>> r{{0, sizeof(void*)}};
    if constexpr (std::is_same_v<T, Entry>) {
        const Entry probe{};
        const size_t at = static_cast<size_t>(reinterpret_cast<const uint8_t*>(&probe.epoch) - reinterpret_cast<const uint8_t*>(&probe));
        r.push_back({at, at + sizeof(probe.epoch)});
    }
    return r;
}

// The leaves of n structs of T at src (as the device holds them) -> objects.  *clean stays true
// while every byte no leaf covers is a T{}'s: the vtable slot and the members that are no leaves
// equal this program's T{}, and all of them, padding included (whose value a T{} does not
// promise, so the server's image is taken from the first struct seen: *image, empty before), are
// the same in every struct of every batch.
template <class T>
static std::vector<T> objects(const uint8_t* src, uint64_t n, bool* clean, bytes* image) {
    static const std::vector<uint32_t> offs = srpc::gpu::leaf_offsets<T>();
    const T proto{};
    std::vector<bool> leaf(sizeof(T), false);
    {
        size_t f = 0;
        srpc::gpu::for_each_leaf<T>(proto, [&](const auto& v) {
            for (size_t k = 0; k < sizeof(v); ++k) leaf[offs[f] + k] = true;
            ++f;
        });
    }
    std::vector<T> out(n);
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t* one = src + i * sizeof(T);
        size_t f = 0;
        srpc::gpu::for_each_leaf<T>(out[i], [&](auto& v) { std::memcpy(&v, one + offs[f++], sizeof(v)); });
        if (image->empty()) {
            image->assign(one, one + sizeof(T));
            for (auto const& [a, b] : named_non_leaf_bytes<T>())
                if (std::memcmp(one + a, reinterpret_cast<const uint8_t*>(&proto) + a, b - a) != 0) *clean = false;
        }
        for (size_t k = 0; k < sizeof(T); ++k)
            if (!leaf[k] && one[k] != (*image)[k]) *clean = false;
    }
    return out;
}
// The leaves of `v` into n zeroed structs of T (only leaves are read by the pack).
template <class T>
static bytes structs(std::vector<T> const& v) {
    static const std::vector<uint32_t> offs = srpc::gpu::leaf_offsets<T>();
    bytes out(v.size() * sizeof(T), 0);
    for (uint64_t i = 0; i < v.size(); ++i) {
        size_t f = 0;
        srpc::gpu::for_each_leaf<T>(v[i], [&](const auto& x) { std::memcpy(out.data() + i * sizeof(T) + offs[f++], &x, sizeof(x)); });
    }
    return out;
}

static int64_t add64(int64_t a, int64_t b) { return static_cast<int64_t>(static_cast<uint64_t>(a) + static_cast<uint64_t>(b)); }
static int64_t sub64(int64_t a, int64_t b) { return static_cast<int64_t>(static_cast<uint64_t>(a) - static_cast<uint64_t>(b)); }

// ---- the stateless answers (a, c) ----
static Balance deposit_of(Entry const& q) {
    Balance r;
    r.sum = add64(q.amount, q.tag);
    r.key = q.key;
    return r;
}
static Balance withdraw_of(Entry const& q) {
    Balance r;
    r.sum = sub64(q.tag, q.amount);
    r.key = q.key;
    return r;
}
static Balance bump_of(Number const& q) {
    Balance r;
    r.sum = add64(q.num, 7);
    r.key = q.num;
    return r;
}

// What the per-method handlers saw, batch after batch: the keys in a device log, the rest on the host.
struct method_log {
    int32_t* d_keys = nullptr;  // device
    uint64_t n = 0, batches = 0, warm = 0;
    bool clean = true;          // the non-leaf bytes of every Req
    bytes image;                // ... as the first Req seen had them
    bool payload = true;        // every Req's other leaves are its key's
};
static std::array<method_log, 3> g_log;
constexpr uint64_t kLogCap = 1 << 14;

template <class Req, int K, class Answer, class Same>
static int record_handler(const void* d_reqs, void* d_resps, uint64_t n, hipStream_t s, Answer answer, Same same) {
    method_log& log = g_log[K];
    bytes in(n * sizeof(Req));
    if (hipStreamSynchronize(s) != hipSuccess) return SRPC_E_HIP;
    if (hipMemcpy(in.data(), d_reqs, in.size(), hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    bool clean = true;
    bool unused = true;
    bytes unused_image;
    const std::vector<Req> reqs = objects<Req>(in.data(), n, &unused, &unused_image);
    std::vector<Balance> out(n);
    std::vector<int32_t> keys(n);
    for (uint64_t i = 0; i < n; ++i) {
        out[i] = answer(reqs[i]);
        keys[i] = out[i].key;
    }
    if (n == 1 && keys[0] == 0) {  // the warm-up's record: no sent key is 0
        ++log.warm;
    } else {
        ++log.batches;
        (void)objects<Req>(in.data(), n, &clean, &log.image);  // (the warm-up's record is not the batches' image)
        log.clean = log.clean && clean;
        for (uint64_t i = 0; i < n; ++i) log.payload = log.payload && same(reqs[i]);
        if (log.n + n > kLogCap) return SRPC_E_CAPACITY;
        if (hipMemcpy(log.d_keys + log.n, keys.data(), 4 * n, hipMemcpyHostToDevice) != hipSuccess) return SRPC_E_HIP;
        log.n += n;
    }
    const bytes raw = structs(out);
    return hipMemcpy(d_resps, raw.data(), raw.size(), hipMemcpyHostToDevice) == hipSuccess ? 0 : SRPC_E_HIP;
}
static bool same_entry(Entry const& q) {
    const Entry w = entry(static_cast<uint64_t>(q.key) - 1);
    return q.tag == w.tag && q.amount == w.amount;
}
static int deposit_records(const void* q, void* r, uint64_t n, hipStream_t s) {
    return record_handler<Entry, 0>(q, r, n, s, deposit_of, same_entry);
}
static int withdraw_records(const void* q, void* r, uint64_t n, hipStream_t s) {
    return record_handler<Entry, 1>(q, r, n, s, withdraw_of, same_entry);
}
static int bump_records(const void* q, void* r, uint64_t n, hipStream_t s) {
    return record_handler<Number, 2>(q, r, n, s, bump_of, [](Number const&) { return true; });
}
static void register_ledger(srpc::gpu::batch_server& s) {
    s.register_record_method<Entry, Balance>(kDeposit, deposit_records);
    s.register_record_method<Entry, Balance>(kWithdraw, withdraw_records);
    s.register_record_method<Number, Balance>(kBump, bump_records);
}
static void reset_logs() {
    for (method_log& l : g_log) {
        if (!l.d_keys) HIPCHECK(hipMalloc(reinterpret_cast<void**>(&l.d_keys), 4 * kLogCap));
        l.n = l.batches = l.warm = 0;
        l.clean = l.payload = true;
        l.image.clear();
    }
}

// Call i of the trace: method (i's hash) of three, or with `unknown` every tenth the CPU server's.
struct call {
    int k;  // 0 deposit, 1 withdraw, 2 bump, 3 close (nobody's on the GPU)
    bytes frame, reply;
};
static call stateless_call(uint64_t i, bool unknown) {
    call c;
    c.k = unknown && i % 10 == 7 ? 3 : static_cast<int>(rnd(i + 99) % 3);
    switch (c.k) {
    case 0: c.frame = request(kDeposit, entry(i)), c.reply = reply(deposit_of(entry(i))); break;
    case 1: c.frame = request(kWithdraw, entry(i)), c.reply = reply(withdraw_of(entry(i))); break;
    case 2: c.frame = request(kBump, number(i)), c.reply = reply(bump_of(number(i))); break;
    default: {
        Closer_servicer cs;
        Number q = number(i);
        c.frame = request(kClose, q);
        c.reply = reply(cs.close(q));
    }
    }
    return c;
}

static bool read_all(int fd, bytes& got) {
    uint64_t have = 0;
    while (have < got.size()) {
        const ssize_t k = recv(fd, got.data() + have, got.size() - have, 0);
        if (k <= 0) return false;  // closed, or the receive timeout: the server is stuck
        have += static_cast<uint64_t>(k);
    }
    return true;
}
static void set_timeout(int fd) {
    timeval tv{60, 0};
    (void)setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof tv);
}

// `rounds` lock-step rounds of 16 calls: one send, their replies read and compared -> all right.
static bool lock_step(int fd, uint64_t rounds, bool unknown, std::array<std::vector<int32_t>, 3>* sent, bytes* all_replies,
                      uint64_t* n_unknown) {
    bool right = true;
    for (uint64_t r = 0; r < rounds && right; ++r) {
        bytes out, want;
        for (uint64_t j = 0; j < 16; ++j) {
            const uint64_t i = 16 * r + j;
            const call c = stateless_call(i, unknown);
            out.insert(out.end(), c.frame.begin(), c.frame.end());
            want.insert(want.end(), c.reply.begin(), c.reply.end());
            if (c.k < 3) (*sent)[c.k].push_back(static_cast<int32_t>(i + 1));
            else ++*n_unknown;
        }
        if (send(fd, out.data(), out.size(), MSG_NOSIGNAL) != static_cast<ssize_t>(out.size())) return false;
        bytes got(want.size());
        right = read_all(fd, got) && got == want;
        if (all_replies) all_replies->insert(all_replies->end(), got.begin(), got.end());
    }
    return right;
}

static std::vector<int32_t> device_log(method_log const& l) {
    std::vector<int32_t> v(l.n);
    if (l.n) HIPCHECK(hipMemcpy(v.data(), l.d_keys, 4 * l.n, hipMemcpyDeviceToHost));
    return v;
}

// ---- (a) ----
static void handlers_see_arrival_order_across_batches() {
    constexpr uint64_t rounds = 40;
    reset_logs();
    served_socketpair sp(16, [](srpc::gpu::batch_server& s) {
        register_ledger(s);
        s.set_ordered_records(true);
        if (!s.ordered_records() || !s.ordered() || s.ordered_var()) std::exit(3);
    });
    set_timeout(sp.fd);
    std::array<std::vector<int32_t>, 3> sent;
    uint64_t unknown = 0;
    CHECK(lock_step(sp.fd, rounds, false, &sent, nullptr, &unknown));
    sp.finish();
    for (int k = 0; k < 3; ++k) {
        CHECK(sent[k].size() > 100);
        CHECK(device_log(g_log[k]) == sent[k]);  // arrival order, across batches
        CHECK(g_log[k].clean && g_log[k].payload);
        CHECK(g_log[k].batches > 0 && g_log[k].batches <= rounds && g_log[k].warm == 2);
    }
    CHECK(sp.thrown == 0 && sp.stats.requests == 16 * rounds && sp.stats.gpu_requests == 16 * rounds);
    CHECK(sp.stats.fallback_requests == 0 && sp.stats.gpu_batches == rounds);
    CHECK(sp.stats.mixed_batches >= 1 && sp.stats.mixed_batches <= rounds);
}

// ---- (b) the ledger ----
static int64_t* g_d_sum = nullptr;  // the service's running sum, in device memory across batches
static uint64_t g_ledger_batches = 0;
static bool g_ledger_clean = true;
static std::array<bytes, 3> g_ledger_image;

static int64_t ledger_step(int64_t sum, int k, int64_t v) { return k == 1 ? sub64(sum, v) : add64(sum, v); }

// One handler for the three methods: the batch walked serially in arrival order.
static int ledger_handler(srpc::gpu::ordered_records_batch const& b, hipStream_t s) {
    if (hipStreamSynchronize(s) != hipSuccess) return SRPC_E_HIP;
    if (b.methods != 3 || b.req_stride[0] != sizeof(Entry) || b.req_stride[1] != sizeof(Entry) ||
        b.req_stride[2] != sizeof(Number) || b.resp_stride[0] != sizeof(Balance) || b.resp_stride[2] != sizeof(Balance))
        return SRPC_E_INVALID;
    std::vector<uint8_t> method(b.n);
    std::vector<uint32_t> rank(b.n);
    if (hipMemcpy(method.data(), b.d_method, b.n, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    if (hipMemcpy(rank.data(), b.d_rank, 4 * b.n, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    std::array<bytes, 3> in;
    for (int k = 0; k < 3; ++k) {
        in[k].resize(b.counts[k] * b.req_stride[k]);
        if (b.counts[k] && hipMemcpy(in[k].data(), b.req_recs[k], in[k].size(), hipMemcpyDeviceToHost) != hipSuccess)
            return SRPC_E_HIP;
    }
    bool clean = true;
    const std::vector<Entry> dep = objects<Entry>(in[0].data(), b.counts[0], &clean, &g_ledger_image[0]),
                             wit = objects<Entry>(in[1].data(), b.counts[1], &clean, &g_ledger_image[1]);
    const std::vector<Number> bum = objects<Number>(in[2].data(), b.counts[2], &clean, &g_ledger_image[2]);
    std::array<std::vector<Balance>, 3> out;
    for (int k = 0; k < 3; ++k) out[k].resize(b.counts[k]);
    int64_t sum = 0;
    if (hipMemcpy(&sum, g_d_sum, 8, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    uint64_t seen = 0;
    for (uint64_t i = 0; i < b.n; ++i) {
        const int k = method[i];
        if (k == SRPC_FRAME_UNKNOWN) {
            if (rank[i] != 0xffffffffu) return SRPC_E_INVALID;
            continue;
        }
        if (k > 2 || rank[i] >= b.counts[k]) return SRPC_E_INVALID;
        const uint32_t r = rank[i];
        const int64_t v = k == 0 ? dep[r].amount : k == 1 ? wit[r].amount : bum[r].num;
        sum = ledger_step(sum, k, v);
        out[k][r].sum = sum;
        out[k][r].key = k == 0 ? dep[r].key : k == 1 ? wit[r].key : bum[r].num;
        ++seen;
    }
    if (seen != b.counts[0] + b.counts[1] + b.counts[2] || seen + b.counts[3] != b.n) return SRPC_E_INVALID;
    for (int k = 0; k < 3; ++k) {
        const bytes raw = structs(out[k]);
        if (b.counts[k] && hipMemcpy(b.resp_recs[k], raw.data(), raw.size(), hipMemcpyHostToDevice) != hipSuccess)
            return SRPC_E_HIP;
    }
    if (seen) {
        ++g_ledger_batches;
        g_ledger_clean = g_ledger_clean && clean;
    }
    return hipMemcpy(g_d_sum, &sum, 8, hipMemcpyHostToDevice) == hipSuccess ? 0 : SRPC_E_HIP;
}

static void stateful_ledger_with_unknown_frames() {
    constexpr uint64_t n = 5000;
    const int64_t start = 11;
    HIPCHECK(hipMalloc(reinterpret_cast<void**>(&g_d_sum), 8));
    HIPCHECK(hipMemcpy(g_d_sum, &start, 8, hipMemcpyHostToDevice));
    g_ledger_batches = 0;
    g_ledger_clean = true;
    for (bytes& im : g_ledger_image) im.clear();
    Closer_servicer closer;
    srpc::server cpu;
    cpu.register_service(closer);
    served_socketpair sp(
        1024,
        [](srpc::gpu::batch_server& s) {
            s.register_record_method<Entry, Balance>(kDeposit, nullptr);
            s.register_record_method<Entry, Balance>(kWithdraw, nullptr);
            s.register_record_method<Number, Balance>(kBump, nullptr);
            s.set_ordered_records_handler(ledger_handler);
            if (!s.ordered_records()) std::exit(3);
        },
        &cpu);
    set_timeout(sp.fd);
    // the trace and the host's replay of it
    bytes out, want;
    int64_t sum = start;
    uint64_t count[4] = {0, 0, 0, 0};
    for (uint64_t i = 0; i < n; ++i) {
        const int k = i % 10 == 7 ? 3 : static_cast<int>(rnd(i + 5) % 3);
        ++count[k];
        bytes f, r;
        if (k == 3) {
            Number q = number(i);
            f = request(kClose, q);
            r = reply(closer.close(q));
        } else if (k == 2) {
            const Number q = number(i);
            sum = ledger_step(sum, k, q.num);
            Balance b;
            b.sum = sum, b.key = q.num;
            f = request(kBump, q);
            r = reply(b);
        } else {
            const Entry q = entry(i);
            sum = ledger_step(sum, k, q.amount);
            Balance b;
            b.sum = sum, b.key = q.key;
            f = request(k == 0 ? kDeposit : kWithdraw, q);
            r = reply(b);
        }
        out.insert(out.end(), f.begin(), f.end());
        want.insert(want.end(), r.begin(), r.end());
    }
    std::thread writer([fd = sp.fd, &out] { srpc::transport::send_all(fd, out.data(), out.size()); });
    bytes got(want.size());
    CHECK(read_all(sp.fd, got));
    writer.join();
    CHECK(got == want);
    sp.finish();
    CHECK(count[0] > 1000 && count[1] > 1000 && count[2] > 1000 && count[3] == n / 10);
    CHECK(sp.thrown == 0 && sp.stats.requests == n);
    CHECK(sp.stats.fallback_requests == count[3] && sp.stats.gpu_requests == n - count[3]);
    CHECK(sp.stats.gpu_requests + sp.stats.fallback_requests == sp.stats.requests);
    CHECK(sp.stats.gpu_batches >= 5 && sp.stats.gpu_batches == g_ledger_batches && g_ledger_clean);
    int64_t end = 0;
    HIPCHECK(hipMemcpy(&end, g_d_sum, 8, hipMemcpyDeviceToHost));
    CHECK(end == sum);
    (void)hipFree(g_d_sum);
}

// ---- (c) one server, three connections ----
static void same_replies_as_the_bucket_route_and_mode_switches() {
    constexpr uint64_t rounds = 12;
    Closer_servicer closer;
    srpc::server cpu;
    cpu.register_service(closer);
    srpc::gpu::batch_server srv(16, 0, &cpu);
    register_ledger(srv);
    std::array<bytes, 3> replies;
    for (int pass = 0; pass < 3; ++pass) {
        const bool on = pass != 1;
        srv.set_ordered_records(on);
        CHECK(srv.ordered_records() == on && srv.ordered() == on && !srv.ordered_var());
        reset_logs();
        served_socketpair sp(srv);
        set_timeout(sp.fd);
        std::array<std::vector<int32_t>, 3> sent;
        uint64_t unknown = 0;
        CHECK(lock_step(sp.fd, rounds, true, &sent, &replies[pass], &unknown));
        sp.finish();
        CHECK(sp.thrown == 0 && sp.stats.requests == 16 * rounds && unknown > 0);
        CHECK(sp.stats.fallback_requests == unknown && sp.stats.gpu_requests == 16 * rounds - unknown);
        CHECK(sp.stats.gpu_requests + sp.stats.fallback_requests == sp.stats.requests);
        CHECK(sp.stats.gpu_batches == rounds);
        for (int k = 0; k < 3; ++k) {
            CHECK(g_log[k].n == sent[k].size() && g_log[k].clean && g_log[k].payload);
            if (on) CHECK(device_log(g_log[k]) == sent[k]);
        }
    }
    CHECK(!replies[0].empty() && replies[1] == replies[0] && replies[2] == replies[0]);
    // set_ordered(false) clears the mode; set_ordered_var takes it over
    srv.set_ordered_records(true);
    srv.set_ordered(false);
    CHECK(!srv.ordered_records() && !srv.ordered());
    srv.set_ordered_records(true);
    srv.set_ordered_var(true);
    CHECK(!srv.ordered_records() && srv.ordered_var() && srv.ordered());
}

// ---- (d) ----
static int never_cols(void* const*, void* const*, uint64_t, hipStream_t) { return SRPC_E_INVALID; }
static int never_var(srpc::gpu::var_batch const&, hipStream_t) { return SRPC_E_INVALID; }
static int never_records(const void*, void*, uint64_t, hipStream_t) { return SRPC_E_INVALID; }

static int thrown_by(std::function<void(srpc::gpu::batch_server&)> setup) {
    served_socketpair sp(16, std::move(setup));
    sp.finish();
    return sp.thrown;
}

static void refusals() {
    CHECK(thrown_by([](srpc::gpu::batch_server& s) {
              register_ledger(s);
              s.register_method<Number, Number>("Ledger_servicer::columns", never_cols);
              s.set_ordered_records(true);
          }) == SRPC_E_UNSUPPORTED);
    CHECK(thrown_by([](srpc::gpu::batch_server& s) {
              s.set_ordered_records(true);  // ... whichever came first
              s.register_method<Number, Number>("Ledger_servicer::columns", never_cols);
          }) == SRPC_E_UNSUPPORTED);
    CHECK(thrown_by([](srpc::gpu::batch_server& s) {
              register_ledger(s);
              s.register_var_method<Text, Text>("Ledger_servicer::text", never_var);
              s.set_ordered_records(true);
          }) == SRPC_E_UNSUPPORTED);
    CHECK(thrown_by([](srpc::gpu::batch_server& s) {
              register_ledger(s);
              s.register_record_method<Big, Number>("Ledger_servicer::big", never_records);
              s.set_ordered_records_handler([](srpc::gpu::ordered_records_batch const&, hipStream_t) { return 0; });
          }) == SRPC_E_UNSUPPORTED);
    // a Resp of any size is taken
    CHECK(thrown_by([](srpc::gpu::batch_server& s) {
              s.register_record_method<Number, Big>("Ledger_servicer::wide_reply",
                                                    [](const void*, void*, uint64_t, hipStream_t) { return 0; });
              s.set_ordered_records(true);
          }) == 0);
    // the other ordered modes keep refusing record methods
    CHECK(thrown_by([](srpc::gpu::batch_server& s) {
              register_ledger(s);
              s.set_ordered(true);
          }) == SRPC_E_UNSUPPORTED);
    CHECK(thrown_by([](srpc::gpu::batch_server& s) {
              register_ledger(s);
              s.set_ordered_var(true);
          }) == SRPC_E_UNSUPPORTED);
}

int main() {
    HIPCHECK(hipSetDevice(0));
    // what a generated stub does: the CPU server finds its argument types by name
    srpc::message_registry["Number"] = [] { return std::make_unique<Number>(); };
    CHECK(sizeof(Entry) == 32 && srpc::gpu::leaf_offsets<Entry>() == (std::vector<uint32_t>{8, 12, 16}));
    CHECK(sizeof(Balance) == 24 && sizeof(Number) == 16 && sizeof(Big) == 264);
    handlers_see_arrival_order_across_batches();
    stateful_ledger_with_unknown_frames();
    same_replies_as_the_bucket_route_and_mode_switches();
    refusals();
    std::printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
