// needs: gpu
// srpc::gpu::batch_server in ordered legs mode (include/srpc/gpu_server.hpp:
// set_ordered_legs, set_ordered_legs_handler): a column method, a record method
// and a string-bodied method side by side, served in arrival order over a
// socketpair, one srpc_frames_unpack_requests_mixed_legs and one
// srpc_frames_pack_requests_mixed_legs a batch:
//   (a) per-method handlers of the three kinds, lock-step batches of 16: each
//       handler appends its requests' keys to a log in device memory; every log
//       is its method's frames in arrival order across batches, every reply byte
//       for byte, and every non-leaf byte of every Req the record handler saw a
//       Req{}'s (Entry has padding and a defaulted member that is no leaf);
//   (b) one ordered_legs_handler for a ledger whose running sum all three
//       methods' requests add to, in device memory across batches: 5000 frames,
//       every tenth a method only the CPU fallback server knows, answered in its
//       place after the handler; every reply equals the host's replay;
//   (c) batch_client::call_legs with a leg, a leg_records and a leg_var against
//       this server: reply columns, structs, strings and codes equal the host's
//       replay; the same server then serves the same trace with
//       set_ordered_legs(false) (the bucket route): byte-equal replies;
//   (d) a string method whose responses outgrow max_response_chars: answered on
//       the CPU for that batch, in place; the other methods' elements do not
//       move; overflow_batches counts it;
//   (e) the refusals: a record Req of 264 bytes; set_ordered, set_ordered_var
//       and set_ordered_records with methods of several kinds.
// The handlers work through the host (this program is host code): they wait for
// the server's stream, copy the batch out, compute, and copy back.
#include <srpc/server.hpp>
#include <sys/time.h>

#include <string>
#include <utility>

#include "mixed_var_fixture.hpp"  // Number, MP, leg_data, CHECK, HIPCHECK
#include "served_socketpair.hpp"

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

struct Balance : public srpc::message_base {  // 24 bytes: every other struct of an array starts off a 16-byte boundary
    int64_t sum = 0;
    int32_t key = 0;
    static constexpr const char* name = "Balance";
    static constexpr auto fields =
        std::make_tuple(STRUCT_MEMBER(Balance, sum, "Balance::sum"), STRUCT_MEMBER(Balance, key, "Balance::key"));
};

// 264 bytes: a Req the ordered legs route does not take
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

// bump: a column method; deposit: a record method; note: a string-bodied method; close: the CPU server's
static const std::string kBump = "Ledger_servicer::bump", kDeposit = "Ledger_servicer::deposit",
                         kNote = "Ledger_servicer::note", kClose = "Ledger_servicer::close";

struct Cpu_servicer : srpc::servicer_base {
    Number close(Number& q) {
        Number r;
        r.num = static_cast<int32_t>(static_cast<uint32_t>(q.num) + 1000u);
        return r;
    }
    MP note(MP& q) { return echo_fixture::answer(q); }  // what the GPU side hands over when note overflows
    static constexpr const char* name = "Ledger";
    static constexpr auto methods = std::make_tuple(STRUCT_MEMBER(Cpu_servicer, close, "Ledger_servicer::close"),
                                                    STRUCT_MEMBER(Cpu_servicer, note, "Ledger_servicer::note"));
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
// Request i of each method: a key that is never 0 (the warm-up's zero record is told apart) and tells i.
static Number number(uint64_t i) {
    Number q;
    q.num = static_cast<int32_t>(i + 1);
    return q;
}
static Entry entry(uint64_t i) {
    const uint64_t z = rnd(i);
    Entry q;
    q.tag = static_cast<int8_t>(z);
    q.key = static_cast<int32_t>(i + 1);
    q.amount = static_cast<int64_t>(z >> 8);
    return q;
}
static MP note(uint64_t i) {
    MP q;
    echo_fixture::fill_request(q, i);
    q.arg3 = static_cast<int64_t>(i + 1);
    return q;
}

static int64_t add64(int64_t a, int64_t b) { return static_cast<int64_t>(static_cast<uint64_t>(a) + static_cast<uint64_t>(b)); }

// ---- the stateless answers (a, c, d) ----
static Balance bump_of(Number const& q) {
    Balance r;
    r.sum = add64(q.num, 7);
    r.key = q.num;
    return r;
}
static Balance deposit_of(Entry const& q) {
    Balance r;
    r.sum = add64(q.amount, q.tag);
    r.key = q.key;
    return r;
}

// ---- a batch's columns and structs through the host ----

// n requests of a method held in columns (fixed leaves, and chars with offsets).
template <class T>
static bool fetch_columns(void* const* cols, const uint64_t* const* offs, uint64_t n, std::vector<T>& out) {
    srpc::gpu::host_columns<T> h;
    h.scatter(std::vector<T>(n));  // the columns' shapes
    for (size_t f = 0; f < h.col.size(); ++f) {
        if (!h.offs[f].empty()) {
            if (!offs || !offs[f]) return false;
            if (hipMemcpy(h.offs[f].data(), offs[f], 8 * (n + 1), hipMemcpyDeviceToHost) != hipSuccess) return false;
            if (h.offs[f][0] != 0) return false;  // a method's request offsets start at 0
            h.col[f].resize(h.offs[f][n]);
        }
        if (!h.col[f].empty() && hipMemcpy(h.col[f].data(), cols[f], h.col[f].size(), hipMemcpyDeviceToHost) != hipSuccess)
            return false;
    }
    h.gather(out);
    return true;
}
// The answers into a method's response columns; *over: a string column was too small (the chars that fit are written).
template <class T>
static int store_columns(std::vector<T> const& v, void* const* cols, uint64_t* const* offs, const uint64_t* cap, bool* over) {
    srpc::gpu::host_columns<T> h;
    h.scatter(v);
    for (size_t f = 0; f < h.col.size(); ++f) {
        uint64_t nbytes = h.col[f].size();
        if (!h.offs[f].empty()) {
            if (cap && nbytes > cap[f]) {
                if (!over) return SRPC_E_CAPACITY;
                *over = true;
                nbytes = cap[f];
            }
            if (hipMemcpy(offs[f], h.offs[f].data(), 8 * (v.size() + 1), hipMemcpyHostToDevice) != hipSuccess) return SRPC_E_HIP;
        }
        if (nbytes && hipMemcpy(cols[f], h.col[f].data(), nbytes, hipMemcpyHostToDevice) != hipSuccess) return SRPC_E_HIP;
    }
    return 0;
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
            if (std::memcmp(one, &proto, sizeof(void*)) != 0) *clean = false;  // the vtable slot
            if constexpr (std::is_same_v<T, Entry>) {
                const size_t at = static_cast<size_t>(reinterpret_cast<const uint8_t*>(&proto.epoch) -
                                                      reinterpret_cast<const uint8_t*>(&proto));
                if (std::memcmp(one + at, &proto.epoch, sizeof(proto.epoch)) != 0) *clean = false;
            }
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

// ---- the per-method handlers (a, c, d) ----

// What a handler saw, batch after batch: the keys in a device log, the rest on the host.
struct method_log {
    int32_t* d_keys = nullptr;  // device
    uint64_t n = 0, batches = 0, warm = 0;
    bool clean = true;    // the non-leaf bytes of every Req (the record method)
    bytes image;          // ... as the first Req seen had them
    bool payload = true;  // every Req's other leaves are its key's
};
static std::array<method_log, 3> g_log;
constexpr uint64_t kLogCap = 1 << 14;
static uint64_t g_overflowing = 0;  // batches whose notes did not fit their column

static void reset_logs() {
    for (method_log& l : g_log) {
        if (!l.d_keys) HIPCHECK(hipMalloc(reinterpret_cast<void**>(&l.d_keys), 4 * kLogCap));
        l.n = l.batches = l.warm = 0;
        l.clean = l.payload = true;
        l.image.clear();
    }
    g_overflowing = 0;
}
// False for the warm-up's zero record (no sent key is 0), else the batch's keys appended to the device log.
static bool log_keys(int k, std::vector<int32_t> const& keys, int* rc) {
    method_log& log = g_log[k];
    *rc = 0;
    if (keys.size() == 1 && keys[0] == 0) {
        ++log.warm;
        return false;
    }
    ++log.batches;
    if (log.n + keys.size() > kLogCap) *rc = SRPC_E_CAPACITY;
    else if (hipMemcpy(log.d_keys + log.n, keys.data(), 4 * keys.size(), hipMemcpyHostToDevice) != hipSuccess) *rc = SRPC_E_HIP;
    else log.n += keys.size();
    return true;
}
static std::vector<int32_t> device_log(method_log const& l) {
    std::vector<int32_t> v(l.n);
    if (l.n) HIPCHECK(hipMemcpy(v.data(), l.d_keys, 4 * l.n, hipMemcpyDeviceToHost));
    return v;
}

static int bump_columns(void* const* rq, void* const* rs, uint64_t n, hipStream_t s) {
    if (hipStreamSynchronize(s) != hipSuccess) return SRPC_E_HIP;
    std::vector<Number> in;
    if (!fetch_columns<Number>(rq, nullptr, n, in)) return SRPC_E_HIP;
    std::vector<Balance> out(n);
    std::vector<int32_t> keys(n);
    for (uint64_t i = 0; i < n; ++i) out[i] = bump_of(in[i]), keys[i] = in[i].num;
    int rc;
    (void)log_keys(0, keys, &rc);
    return rc ? rc : store_columns(out, rs, nullptr, nullptr, nullptr);
}
static int deposit_records(const void* d_reqs, void* d_resps, uint64_t n, hipStream_t s) {
    if (hipStreamSynchronize(s) != hipSuccess) return SRPC_E_HIP;
    bytes in(n * sizeof(Entry));
    if (hipMemcpy(in.data(), d_reqs, in.size(), hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    bool unused = true;
    bytes unused_image;
    const std::vector<Entry> reqs = objects<Entry>(in.data(), n, &unused, &unused_image);
    std::vector<Balance> out(n);
    std::vector<int32_t> keys(n);
    for (uint64_t i = 0; i < n; ++i) out[i] = deposit_of(reqs[i]), keys[i] = reqs[i].key;
    int rc;
    if (log_keys(1, keys, &rc)) {  // (the warm-up's record is not the batches' image)
        bool clean = true;
        (void)objects<Entry>(in.data(), n, &clean, &g_log[1].image);
        g_log[1].clean = g_log[1].clean && clean;
        for (Entry const& q : reqs) {
            const Entry w = entry(static_cast<uint64_t>(q.key) - 1);
            g_log[1].payload = g_log[1].payload && q.tag == w.tag && q.amount == w.amount;
        }
    }
    if (rc) return rc;
    const bytes raw = structs(out);
    return hipMemcpy(d_resps, raw.data(), raw.size(), hipMemcpyHostToDevice) == hipSuccess ? 0 : SRPC_E_HIP;
}
// Honest offsets and only the chars that fit: what a device handler that counts before it writes leaves behind.
static int note_strings(srpc::gpu::var_batch const& b, hipStream_t s) {
    if (hipStreamSynchronize(s) != hipSuccess) return SRPC_E_HIP;
    std::vector<MP> in;
    if (!fetch_columns<MP>(b.req_cols, b.req_str_offs, b.n, in)) return SRPC_E_HIP;
    std::vector<MP> out(b.n);
    std::vector<int32_t> keys(b.n);
    for (uint64_t i = 0; i < b.n; ++i) out[i] = echo_fixture::answer(in[i]), keys[i] = static_cast<int32_t>(in[i].arg3);
    int rc;
    if (log_keys(2, keys, &rc))
        for (MP const& q : in) {
            MP w = note(static_cast<uint64_t>(q.arg3) - 1);
            g_log[2].payload = g_log[2].payload && q.arg1 == w.arg1 && q.arg2 == w.arg2 && q.arg4 == w.arg4;
        }
    if (rc) return rc;
    bool over = false;
    rc = store_columns(out, b.resp_cols, b.resp_str_offs, b.resp_cap, &over);
    g_overflowing += over;
    return rc;
}
static void register_ledger(srpc::gpu::batch_server& s, srpc::gpu::var_limits lim = {}) {
    s.register_method<Number, Balance>(kBump, bump_columns);
    s.register_record_method<Entry, Balance>(kDeposit, deposit_records);
    s.register_var_method<MP, MP>(kNote, note_strings, lim);
}

// Call i of the stateless trace: method (i's hash) of three, or with `unknown` every tenth the CPU server's.
struct call {
    int k;  // 0 bump, 1 deposit, 2 note, 3 close (nobody's on the GPU)
    bytes frame, reply;
};
static call stateless_call(uint64_t i, bool unknown) {
    call c;
    c.k = unknown && i % 10 == 7 ? 3 : static_cast<int>(rnd(i + 99) % 3);
    switch (c.k) {
    case 0: c.frame = request(kBump, number(i)), c.reply = reply(bump_of(number(i))); break;
    case 1: c.frame = request(kDeposit, entry(i)), c.reply = reply(deposit_of(entry(i))); break;
    case 2: c.frame = request(kNote, note(i)), c.reply = reply(echo_fixture::answer(note(i))); break;
    default: {
        Cpu_servicer cs;
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
static bool lock_step(int fd, uint64_t rounds, bool unknown, std::array<std::vector<int32_t>, 3>* sent, uint64_t* n_unknown) {
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
    }
    return right;
}

// ---- (a) ----
static void handlers_see_arrival_order_across_batches() {
    constexpr uint64_t rounds = 40;
    reset_logs();
    served_socketpair sp(16, [](srpc::gpu::batch_server& s) {
        register_ledger(s);
        s.set_ordered_legs(true);
        if (!s.ordered_legs() || !s.ordered() || s.ordered_var() || s.ordered_records()) std::exit(3);
    });
    set_timeout(sp.fd);
    std::array<std::vector<int32_t>, 3> sent;
    uint64_t unknown = 0;
    CHECK(lock_step(sp.fd, rounds, false, &sent, &unknown));
    sp.finish();
    for (int k = 0; k < 3; ++k) {
        CHECK(sent[k].size() > 100);
        CHECK(device_log(g_log[k]) == sent[k]);  // arrival order, across batches
        CHECK(g_log[k].clean && g_log[k].payload);
        CHECK(g_log[k].batches > 0 && g_log[k].batches <= rounds && g_log[k].warm == 2);
    }
    CHECK(sp.thrown == 0 && sp.stats.requests == 16 * rounds && sp.stats.gpu_requests == 16 * rounds);
    CHECK(sp.stats.fallback_requests == 0 && sp.stats.gpu_batches == rounds && sp.stats.overflow_batches == 0);
    CHECK(sp.stats.mixed_batches >= 1 && sp.stats.mixed_batches <= rounds && g_overflowing == 0);
}

// ---- (b) the ledger ----
static int64_t* g_d_sum = nullptr;  // the service's running sum, in device memory across batches
static uint64_t g_ledger_batches = 0;
static bool g_ledger_clean = true;
static bytes g_ledger_image;

// What request v of method k adds to the sum.
static int64_t ledger_value(Number const& q) { return q.num; }
static int64_t ledger_value(Entry const& q) { return q.amount; }
static int64_t ledger_value(MP const& q) { return static_cast<int64_t>(q.arg4.size()) + q.arg1; }
static MP receipt(MP const& q, int64_t sum) {
    MP r = echo_fixture::answer(q);
    r.arg3 = sum;
    return r;
}

// One handler for the three methods: the batch walked serially in arrival order.
static int ledger_handler(srpc::gpu::ordered_legs_batch const& b, hipStream_t s) {
    if (hipStreamSynchronize(s) != hipSuccess) return SRPC_E_HIP;
    // a column method has no array, a record method no columns
    if (b.methods != 3 || b.req_stride[0] != 0 || b.req_stride[1] != sizeof(Entry) || b.req_stride[2] != 0 ||
        b.resp_stride[0] != 0 || b.resp_stride[1] != sizeof(Balance) || b.resp_stride[2] != 0 || b.req_recs[0] ||
        !b.req_recs[1] || b.req_recs[2] || b.resp_recs[0] || !b.resp_recs[1] || b.resp_recs[2] || !b.req_cols[0] ||
        b.req_cols[1] || !b.req_cols[2] || !b.resp_cols[0] || b.resp_cols[1] || !b.resp_cols[2] || !b.req_str_offs[2] ||
        !b.resp_str_offs[2] || !b.resp_cap[2])
        return SRPC_E_INVALID;
    std::vector<uint8_t> method(b.n);
    std::vector<uint32_t> rank(b.n);
    if (hipMemcpy(method.data(), b.d_method, b.n, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    if (hipMemcpy(rank.data(), b.d_rank, 4 * b.n, hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    std::vector<Number> bum;
    std::vector<MP> notes;
    if (!fetch_columns<Number>(b.req_cols[0], nullptr, b.counts[0], bum)) return SRPC_E_HIP;
    if (!fetch_columns<MP>(b.req_cols[2], b.req_str_offs[2], b.counts[2], notes)) return SRPC_E_HIP;
    bytes in(b.counts[1] * sizeof(Entry));
    if (b.counts[1] && hipMemcpy(in.data(), b.req_recs[1], in.size(), hipMemcpyDeviceToHost) != hipSuccess) return SRPC_E_HIP;
    bool clean = true;
    const std::vector<Entry> dep = objects<Entry>(in.data(), b.counts[1], &clean, &g_ledger_image);
    std::vector<Balance> out0(b.counts[0]), out1(b.counts[1]);
    std::vector<MP> out2(b.counts[2]);
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
        sum = add64(sum, k == 0 ? ledger_value(bum[r]) : k == 1 ? ledger_value(dep[r]) : ledger_value(notes[r]));
        if (k == 0) out0[r].sum = sum, out0[r].key = bum[r].num;
        else if (k == 1) out1[r].sum = sum, out1[r].key = dep[r].key;
        else out2[r] = receipt(notes[r], sum);
        ++seen;
    }
    if (seen != b.counts[0] + b.counts[1] + b.counts[2] || seen + b.counts[3] != b.n) return SRPC_E_INVALID;
    if (int rc = store_columns(out0, b.resp_cols[0], nullptr, nullptr, nullptr)) return rc;
    if (int rc = store_columns(out2, b.resp_cols[2], b.resp_str_offs[2], b.resp_cap[2], nullptr)) return rc;
    const bytes raw = structs(out1);
    if (b.counts[1] && hipMemcpy(b.resp_recs[1], raw.data(), raw.size(), hipMemcpyHostToDevice) != hipSuccess) return SRPC_E_HIP;
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
    g_ledger_image.clear();
    Cpu_servicer closer;
    srpc::server cpu;
    cpu.register_service(closer);
    served_socketpair sp(
        1024,
        [](srpc::gpu::batch_server& s) {
            s.register_method<Number, Balance>(kBump, nullptr);
            s.register_record_method<Entry, Balance>(kDeposit, nullptr);
            s.register_var_method<MP, MP>(kNote, nullptr);
            s.set_ordered_legs_handler(ledger_handler);
            if (!s.ordered_legs() || !s.ordered()) std::exit(3);
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
        } else if (k == 0) {
            const Number q = number(i);
            sum = add64(sum, ledger_value(q));
            Balance b;
            b.sum = sum, b.key = q.num;
            f = request(kBump, q);
            r = reply(b);
        } else if (k == 1) {
            const Entry q = entry(i);
            sum = add64(sum, ledger_value(q));
            Balance b;
            b.sum = sum, b.key = q.key;
            f = request(kDeposit, q);
            r = reply(b);
        } else {
            const MP q = note(i);
            sum = add64(sum, ledger_value(q));
            f = request(kNote, q);
            r = reply(receipt(q, sum));
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
    CHECK(sp.stats.gpu_batches >= 5 && sp.stats.gpu_batches == g_ledger_batches && g_ledger_clean);
    CHECK(sp.stats.overflow_batches == 0);
    int64_t end = 0;
    HIPCHECK(hipMemcpy(&end, g_d_sum, 8, hipMemcpyDeviceToHost));
    CHECK(end == sum);
    (void)hipFree(g_d_sum);
}

// ---- (c) batch_client::call_legs against this server ----

// A proto whose every byte outside the leaves is told apart from zero and from
// the 0xA5 the reply array starts with (the vtable pointer stays).
static Balance marked_proto() {
    Balance proto;
    auto* b = reinterpret_cast<uint8_t*>(&proto);
    for (size_t k = 20; k < sizeof(Balance); ++k) b[k] = static_cast<uint8_t>(0xC0 + k);  // the padding behind key
    return proto;
}

// n calls in a fixed pseudo-random order over bump (a column leg), deposit (a
// record leg) and note (a string-bodied leg); what the device holds after the
// batch, as raw bytes, to compare two servings with.
struct legs_trace {
    uint64_t n;
    std::vector<uint8_t> method, hcodes;
    std::vector<uint32_t> rank;
    std::array<uint64_t, 3> count{};
    leg_data<Number, Balance> bump;
    leg_data<MP, MP> notes;
    std::vector<Entry> deposits;
    void *d_req = nullptr, *d_resp = nullptr;
    bytes structs_raw;
    uint8_t *d_method = nullptr, *d_codes = nullptr;
    Balance proto = marked_proto();

    explicit legs_trace(uint64_t n) : n(n), method(n), hcodes(n + 16), rank(n) {
        for (uint64_t i = 0; i < n; ++i) {
            method[i] = static_cast<uint8_t>(rnd(i + 31) % 3);
            rank[i] = static_cast<uint32_t>(count[method[i]]++);
        }
        uint64_t chars = 0;
        for (uint64_t i = 0; i < n; ++i) {
            if (method[i] == 0) bump.in.push_back(number(i));
            else if (method[i] == 1) deposits.push_back(entry(i));
            else notes.in.push_back(note(i)), chars += notes.in.back().arg4.size() + 1;  // the answer appends "!"
        }
        bump.upload(0);
        notes.upload(chars);  // exact: nothing to spare
        HIPCHECK(hipMalloc(&d_req, deposits.size() * sizeof(Entry) + 16));
        HIPCHECK(hipMalloc(&d_resp, deposits.size() * sizeof(Balance) + 16));
        HIPCHECK(hipMemcpy(d_req, static_cast<const void*>(deposits.data()), deposits.size() * sizeof(Entry), hipMemcpyHostToDevice));
        HIPCHECK(hipMalloc(reinterpret_cast<void**>(&d_method), n + 16));
        HIPCHECK(hipMalloc(reinterpret_cast<void**>(&d_codes), n + 16));
        HIPCHECK(hipMemcpy(d_method, method.data(), n, hipMemcpyHostToDevice));
        clear_replies();
    }
    void clear_replies() {
        HIPCHECK(hipMemset(d_resp, 0xA5, deposits.size() * sizeof(Balance) + 16));
        HIPCHECK(hipMemset(d_codes, 0xA5, n + 16));
        for (auto* l : {&bump.resp, &notes.resp})
            for (size_t f = 0; f < l->size(); ++f)
                HIPCHECK(hipMemset((*l)[f], 0xA5, (l == &bump.resp ? bump.cap[f] : notes.cap[f]) + kGuard));
        for (uint64_t* o : notes.resp_offs)
            if (o) HIPCHECK(hipMemset(o, 0xA5, 8 * (notes.in.size() + 1) + kGuard));
    }
    std::vector<srpc::gpu::mixed_leg> legs(srpc::gpu::batch_client& cl) {
        std::vector<srpc::gpu::mixed_leg> l;
        l.push_back(cl.leg<Number, Balance>(kBump, bump.req.data(), bump.resp.data(), count[0]));
        l.push_back(cl.leg_records<Entry, Balance>(kDeposit, static_cast<const Entry*>(d_req), static_cast<Balance*>(d_resp),
                                                   count[1], proto));
        l.push_back(cl.leg_var<MP, MP>(kNote, notes.req.data(), notes.req_offs.data(), notes.resp.data(),
                                       notes.resp_offs.data(), notes.cap.data(), count[2]));
        return l;
    }
    // Every value the batch left behind against the host's replay: columns, structs byte for byte, strings, codes.
    void check_values() {
        std::vector<Balance> b;
        std::vector<MP> m;
        CHECK(bump.fetch(b));
        CHECK(notes.fetch(m));
        structs_raw.resize(deposits.size() * sizeof(Balance) + 16);
        HIPCHECK(hipMemcpy(structs_raw.data(), d_resp, structs_raw.size(), hipMemcpyDeviceToHost));
        HIPCHECK(hipMemcpy(hcodes.data(), d_codes, n + 16, hipMemcpyDeviceToHost));
        if (g_fail) return;
        static const std::vector<uint32_t> lo = srpc::gpu::leaf_offsets<Balance>();
        bool columns = true, recs = true, strings = true, codes = true;
        for (uint64_t r = 0; r < count[0]; ++r) {
            const Balance w = bump_of(bump.in[r]);
            columns = columns && b[r].sum == w.sum && b[r].key == w.key;
        }
        for (uint64_t r = 0; r < count[1]; ++r) {
            const Balance w = deposit_of(deposits[r]);
            bytes want(reinterpret_cast<const uint8_t*>(&proto), reinterpret_cast<const uint8_t*>(&proto) + sizeof(Balance));
            std::memcpy(want.data() + lo[0], &w.sum, 8);
            std::memcpy(want.data() + lo[1], &w.key, 4);
            recs = recs && std::memcmp(structs_raw.data() + r * sizeof(Balance), want.data(), sizeof(Balance)) == 0;
        }
        for (uint64_t r = 0; r < count[2]; ++r) strings = strings && same(m[r], echo_fixture::answer(notes.in[r]));
        for (uint64_t i = 0; i < n; ++i) codes = codes && hcodes[i] == srpc::RPC_SUCCESS;
        for (uint64_t g = 0; g < 16; ++g)
            codes = codes && hcodes[n + g] == 0xA5 && structs_raw[deposits.size() * sizeof(Balance) + g] == 0xA5;
        CHECK(columns);
        CHECK(recs);
        CHECK(strings);
        CHECK(codes);
    }
    // The reply bytes on the device after check_values, guards included.
    std::vector<bytes> reply_bytes() const {
        std::vector<bytes> all = bump.raw;
        all.insert(all.end(), notes.raw.begin(), notes.raw.end());
        for (auto const& o : notes.raw_offs)
            all.emplace_back(reinterpret_cast<const uint8_t*>(o.data()), reinterpret_cast<const uint8_t*>(o.data() + o.size()));
        all.push_back(structs_raw);
        all.push_back(hcodes);
        return all;
    }
    ~legs_trace() {
        for (void* p : {d_req, d_resp}) (void)hipFree(p);
        (void)hipFree(d_method);
        (void)hipFree(d_codes);
    }
};

static void call_legs_against_this_server_and_the_bucket_route() {
    constexpr uint64_t n = 3000, chunk = 1024;
    srpc::gpu::batch_server srv(chunk);
    register_ledger(srv);
    legs_trace d(n);
    for (int k = 0; k < 3; ++k) CHECK(d.count[k] > 800);
    std::array<std::vector<bytes>, 2> replies;
    for (int pass = 0; pass < 2; ++pass) {
        const bool on = pass == 0;
        srv.set_ordered_legs(on);
        CHECK(srv.ordered_legs() == on && srv.ordered() == on && !srv.ordered_var() && !srv.ordered_records());
        reset_logs();
        d.clear_replies();
        served_socketpair sp(srv);
        srpc::gpu::call_stats st;
        {
            srpc::gpu::batch_client cl(sp.fd, chunk);
            st = cl.call_legs(d.legs(cl), d.d_method, n, d.d_codes);
        }
        sp.finish();
        d.check_values();
        replies[pass] = d.reply_bytes();
        CHECK(st.calls == n && st.ok == n && st.failed == 0 && st.malformed == 0 && st.unanswered == 0 && st.chunks == 3);
        CHECK(sp.thrown == 0 && sp.stats.requests == n && sp.stats.gpu_requests == n && sp.stats.fallback_requests == 0);
        for (int k = 0; k < 3; ++k) {
            CHECK(g_log[k].n == d.count[k] && g_log[k].clean && g_log[k].payload);
            if (!on) continue;
            // arrival order: the keys are the calls' indices + 1, ascending
            const std::vector<int32_t> log = device_log(g_log[k]);
            bool ascending = true;
            for (size_t r = 1; r < log.size(); ++r) ascending = ascending && log[r - 1] < log[r];
            CHECK(ascending);
        }
    }
    CHECK(!replies[0].empty() && replies[1] == replies[0]);
    // set_ordered(false) clears the mode; the other sub-modes take it over
    srv.set_ordered_legs(true);
    srv.set_ordered(false);
    CHECK(!srv.ordered_legs() && !srv.ordered());
    srv.set_ordered_legs(true);
    srv.set_ordered_var(true);
    CHECK(!srv.ordered_legs() && srv.ordered_var() && srv.ordered());
    srv.set_ordered_legs(true);
    CHECK(srv.ordered_legs() && !srv.ordered_var());
    srv.set_ordered_records(true);
    CHECK(!srv.ordered_legs() && srv.ordered_records() && srv.ordered());
}

// ---- (d) responses that do not fit ----
static void overflowing_string_method_is_answered_on_the_cpu() {
    constexpr uint64_t rounds = 30;
    reset_logs();
    Cpu_servicer cs;
    srpc::server cpu;
    cpu.register_service(cs);
    served_socketpair sp(
        16,
        [](srpc::gpu::batch_server& s) {
            srpc::gpu::var_limits small;
            small.max_response_chars = 4;  // 64 chars and 16 spare a batch; a note's answer averages 21
            register_ledger(s, small);
            s.set_ordered_legs(true);
        },
        &cpu);
    set_timeout(sp.fd);
    std::array<std::vector<int32_t>, 3> sent;
    uint64_t unknown = 0;
    CHECK(lock_step(sp.fd, rounds, false, &sent, &unknown));  // the CPU server's notes in their places
    sp.finish();
    CHECK(sp.thrown == 0 && sp.stats.requests == 16 * rounds);
    CHECK(g_overflowing >= 5 && g_overflowing <= g_log[2].batches && sp.stats.overflow_batches == g_overflowing);
    CHECK(sp.stats.fallback_requests >= g_overflowing && sp.stats.fallback_requests <= sent[2].size());
    CHECK(sp.stats.gpu_requests + sp.stats.fallback_requests == sp.stats.requests);
    // the other methods' elements did not move, and every handler still saw arrival order
    for (int k = 0; k < 3; ++k) {
        CHECK(device_log(g_log[k]) == sent[k]);
        CHECK(g_log[k].clean && g_log[k].payload);
    }
}

// ---- (e) ----
static int never_cols(void* const*, void* const*, uint64_t, hipStream_t) { return SRPC_E_INVALID; }
static int never_records(const void*, void*, uint64_t, hipStream_t) { return SRPC_E_INVALID; }

static int thrown_by(std::function<void(srpc::gpu::batch_server&)> setup) {
    served_socketpair sp(16, std::move(setup));
    sp.finish();
    return sp.thrown;
}

static void refusals() {
    CHECK(thrown_by([](srpc::gpu::batch_server& s) {
              register_ledger(s);
              s.register_record_method<Big, Number>("Ledger_servicer::big", never_records);
              s.set_ordered_legs(true);
          }) == SRPC_E_UNSUPPORTED);
    CHECK(thrown_by([](srpc::gpu::batch_server& s) {
              s.set_ordered_legs_handler([](srpc::gpu::ordered_legs_batch const&, hipStream_t) { return 0; });
              s.register_record_method<Big, Number>("Ledger_servicer::big", never_records);  // ... whichever came first
          }) == SRPC_E_UNSUPPORTED);
    // a Resp of any size, and a Big in columns, are taken
    CHECK(thrown_by([](srpc::gpu::batch_server& s) {
              s.register_record_method<Number, Big>("Ledger_servicer::wide_reply",
                                                    [](const void*, void*, uint64_t, hipStream_t) { return 0; });
              s.register_method<Big, Number>("Ledger_servicer::big", [](void* const*, void* const*, uint64_t, hipStream_t) { return 0; });
              s.set_ordered_legs(true);
          }) == 0);
    // all of one kind is a valid registration
    CHECK(thrown_by([](srpc::gpu::batch_server& s) {
              s.register_method<Number, Balance>(kBump, bump_columns);
              s.set_ordered_legs(true);
          }) == 0);
    // the other ordered modes keep refusing what they refuse
    CHECK(thrown_by([](srpc::gpu::batch_server& s) {
              register_ledger(s);
              s.set_ordered(true);
          }) == SRPC_E_UNSUPPORTED);
    CHECK(thrown_by([](srpc::gpu::batch_server& s) {
              register_ledger(s);
              s.set_ordered_var(true);
          }) == SRPC_E_UNSUPPORTED);
    CHECK(thrown_by([](srpc::gpu::batch_server& s) {
              register_ledger(s);
              s.set_ordered_records(true);
          }) == SRPC_E_UNSUPPORTED);
    CHECK(thrown_by([](srpc::gpu::batch_server& s) {
              s.register_method<Number, Balance>(kBump, never_cols);
              s.register_record_method<Entry, Balance>(kDeposit, never_records);
              s.set_ordered_legs(true);
              s.set_ordered(false), s.set_ordered(true);  // the plain ordered mode, not the legs one
              if (s.ordered_legs()) std::exit(3);
          }) == SRPC_E_UNSUPPORTED);
}

int main() {
    HIPCHECK(hipSetDevice(0));
    // what a generated stub does: the CPU server finds its argument types by name
    srpc::message_registry["Number"] = [] { return std::make_unique<Number>(); };
    srpc::message_registry["multiple_primitives"] = [] { return std::make_unique<MP>(); };
    CHECK(sizeof(Entry) == 32 && srpc::gpu::leaf_offsets<Entry>() == (std::vector<uint32_t>{8, 12, 16}));
    CHECK(sizeof(Balance) == 24 && srpc::gpu::leaf_offsets<Balance>() == (std::vector<uint32_t>{8, 16}));
    CHECK(sizeof(Number) == 16 && sizeof(Big) == 264);
    handlers_see_arrival_order_across_batches();
    stateful_ledger_with_unknown_frames();
    call_legs_against_this_server_and_the_bucket_route();
    overflowing_string_method_is_answered_on_the_cpu();
    refusals();
    std::printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
