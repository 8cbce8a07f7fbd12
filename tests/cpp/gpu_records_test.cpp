// needs: gpu
// Calls and handlers over device arrays of the caller's own structs:
// srpc::gpu::batch_client::call_records (include/srpc/gpu_client.hpp) against
// srpc::gpu::batch_server::register_record_method (include/srpc/gpu_server.hpp)
// on the two ends of a socketpair.  Two methods are served from struct arrays
// by kernels with one thread per struct (compiled at run time, so this file
// stays host code), a third from columns.  Checked: every reply struct, byte
// for byte (the leaves the host computes, every other byte the proto's), and
// every code; the same calls through the column form; every tenth call
// rewritten to a method nobody registered (bare replies); a peer that closes
// five replies into the second chunk; the refusals.
#include <dlfcn.h>
#include <hip/hip_runtime_api.h>
#include <srpc/gpu_client.hpp>
#include <srpc/gpu_server.hpp>
#include <srpc/packer.hpp>
#include <sys/socket.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

struct TwoNumbers : public srpc::message_base {
    int32_t a;
    int32_t b;
    static constexpr const char* name = "TwoNumbers";
    static constexpr auto fields =
        std::make_tuple(STRUCT_MEMBER(TwoNumbers, a, "TwoNumbers::a"), STRUCT_MEMBER(TwoNumbers, b, "TwoNumbers::b"));
};

struct Number : public srpc::message_base {
    int32_t num;
    static constexpr const char* name = "Number";
    static constexpr auto fields = std::make_tuple(STRUCT_MEMBER(Number, num, "Number::num"));
};

struct Wide : public srpc::message_base {
    bool k_bool;
    int8_t k_i8;
    char k_char;
    int16_t k_i16;
    int32_t k_i32;
    int64_t k_i64;
    static constexpr const char* name = "Wide";
    static constexpr auto fields =
        std::make_tuple(STRUCT_MEMBER(Wide, k_bool, "Wide::k_bool"), STRUCT_MEMBER(Wide, k_i8, "Wide::k_i8"),
                        STRUCT_MEMBER(Wide, k_char, "Wide::k_char"), STRUCT_MEMBER(Wide, k_i16, "Wide::k_i16"),
                        STRUCT_MEMBER(Wide, k_i32, "Wide::k_i32"), STRUCT_MEMBER(Wide, k_i64, "Wide::k_i64"));
};

struct Odd : public srpc::message_base {  // 24 bytes: every other struct of an array starts off a 16-byte boundary
    int64_t sum;
    int32_t diff;
    static constexpr const char* name = "Odd";
    static constexpr auto fields = std::make_tuple(STRUCT_MEMBER(Odd, sum, "Odd::sum"), STRUCT_MEMBER(Odd, diff, "Odd::diff"));
};

// 264 bytes: past what srpc_gpu_unpack_aos_fill takes, so the server fills its Req array once
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

static const std::string kAdd = "Calc_servicer::add", kWide = "Calc_servicer::wide", kEcho = "Calc_servicer::echo",
                         kOdd = "Calc_servicer::odd", kBig = "Calc_servicer::big";
constexpr uint64_t kBatch = 1024, kCalls = 5000;

// ---- the handlers' kernels: the layouts above as the device sees them ----
static const char* kKernels = R"(
struct TwoNumbers { void* vptr; int a; int b; };
struct Number { void* vptr; int num; };
struct Wide { void* vptr; bool k_bool; signed char k_i8; char k_char; short k_i16; int k_i32; long long k_i64; };
extern "C" __global__ void k_add(const TwoNumbers* q, Number* r, unsigned long long n) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) r[i].num = (int)((unsigned)q[i].a + (unsigned)q[i].b);
}
struct Big { void* vptr; long long v[32]; };
extern "C" __global__ void k_big(const Big* q, Number* r, unsigned long long n) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) r[i].num = (int)(unsigned)((unsigned long long)q[i].v[0] + (unsigned long long)q[i].v[17] +
                                          (unsigned long long)q[i].v[31]);
}
extern "C" __global__ void k_wide(const Wide* q, Wide* r, unsigned long long n) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    r[i].k_bool = !q[i].k_bool;
    r[i].k_i8 = (signed char)((unsigned char)q[i].k_i8 + 1u);
    r[i].k_char = (char)((unsigned char)q[i].k_char + 2u);
    r[i].k_i16 = (short)((unsigned short)q[i].k_i16 + 3u);
    r[i].k_i32 = (int)((unsigned)q[i].k_i32 + 4u);
    r[i].k_i64 = (long long)((unsigned long long)q[i].k_i64 + 5ull);
}
)";

static Number add_of(TwoNumbers const& q) {
    Number r;
    r.num = static_cast<int32_t>(static_cast<uint32_t>(q.a) + static_cast<uint32_t>(q.b));
    return r;
}
static Wide wide_of(Wide const& q) {
    Wide r;
    r.k_bool = !q.k_bool;
    r.k_i8 = static_cast<int8_t>(static_cast<uint8_t>(q.k_i8) + 1u);
    r.k_char = static_cast<char>(static_cast<uint8_t>(q.k_char) + 2u);
    r.k_i16 = static_cast<int16_t>(static_cast<uint16_t>(q.k_i16) + 3u);
    r.k_i32 = static_cast<int32_t>(static_cast<uint32_t>(q.k_i32) + 4u);
    r.k_i64 = static_cast<int64_t>(static_cast<uint64_t>(q.k_i64) + 5ull);
    return r;
}

static Number big_of(Big const& q) {
    Number r;
    r.num = static_cast<int32_t>(static_cast<uint32_t>(static_cast<uint64_t>(q.v0) + static_cast<uint64_t>(q.v17) +
                                                       static_cast<uint64_t>(q.v31)));
    return r;
}

static hipFunction_t g_add = nullptr, g_wide = nullptr, g_big = nullptr;

// The run-time compiler through dlopen: the test programs link the HIP runtime only.
static void compile_kernels() {
    void* rtc = dlopen("libhiprtc.so", RTLD_NOW);
    if (!rtc) { std::fprintf(stderr, "dlopen libhiprtc.so: %s\n", dlerror()); std::exit(2); }
    using prog_t = void*;
    auto create = reinterpret_cast<int (*)(prog_t*, const char*, const char*, int, const char**, const char**)>(
        dlsym(rtc, "hiprtcCreateProgram"));
    auto compile = reinterpret_cast<int (*)(prog_t, int, const char**)>(dlsym(rtc, "hiprtcCompileProgram"));
    auto code_size = reinterpret_cast<int (*)(prog_t, size_t*)>(dlsym(rtc, "hiprtcGetCodeSize"));
    auto get_code = reinterpret_cast<int (*)(prog_t, char*)>(dlsym(rtc, "hiprtcGetCode"));
    auto log_size = reinterpret_cast<int (*)(prog_t, size_t*)>(dlsym(rtc, "hiprtcGetProgramLogSize"));
    auto get_log = reinterpret_cast<int (*)(prog_t, char*)>(dlsym(rtc, "hiprtcGetProgramLog"));
    if (!create || !compile || !code_size || !get_code || !log_size || !get_log) std::exit(2);
    hipDeviceProp_t prop;
    HIPCHECK(hipGetDeviceProperties(&prop, 0));
    const std::string arch = std::string("--offload-arch=") + prop.gcnArchName;
    const char* opts[] = {arch.c_str()};
    prog_t prog = nullptr;
    if (create(&prog, kKernels, "records_handlers.hip", 0, nullptr, nullptr) != 0) std::exit(2);
    if (compile(prog, 1, opts) != 0) {
        size_t ls = 0;
        log_size(prog, &ls);
        std::string log(ls, '\0');
        get_log(prog, log.data());
        std::fprintf(stderr, "handler kernels did not compile:\n%s\n", log.c_str());
        std::exit(2);
    }
    size_t cs = 0;
    code_size(prog, &cs);
    static std::vector<char> code;
    code.resize(cs);
    get_code(prog, code.data());
    hipModule_t mod;
    HIPCHECK(hipModuleLoadData(&mod, code.data()));
    HIPCHECK(hipModuleGetFunction(&g_add, mod, "k_add"));
    HIPCHECK(hipModuleGetFunction(&g_wide, mod, "k_wide"));
    HIPCHECK(hipModuleGetFunction(&g_big, mod, "k_big"));
}

static int launch(hipFunction_t f, const void* q, void* r, uint64_t n, hipStream_t s) {
    unsigned long long nn = n;
    void* qq = const_cast<void*>(q);
    void* args[] = {&qq, &r, &nn};
    const unsigned grid = static_cast<unsigned>((n + 255) / 256);
    return hipModuleLaunchKernel(f, grid, 1, 1, 256, 1, 1, 0, s, args, nullptr) == hipSuccess ? 0 : SRPC_E_HIP;
}
static int add_records(const void* q, void* r, uint64_t n, hipStream_t s) { return launch(g_add, q, r, n, s); }
static int wide_records(const void* q, void* r, uint64_t n, hipStream_t s) { return launch(g_wide, q, r, n, s); }
static int big_records(const void* q, void* r, uint64_t n, hipStream_t s) { return launch(g_big, q, r, n, s); }
static int echo_columns(void* const* rq, void* const* rs, uint64_t n, hipStream_t s) {
    return hipMemcpyAsync(rs[0], rq[0], n * sizeof(int32_t), hipMemcpyDeviceToDevice, s) == hipSuccess ? 0 : SRPC_E_HIP;
}

static void register_all(srpc::gpu::batch_server& srv) {
    srv.register_record_method<TwoNumbers, Number>(kAdd, add_records);
    srv.register_method<Number, Number>(kEcho, echo_columns);
    srv.register_record_method<Wide, Wide>(kWide, wide_records);
    srv.register_record_method<Big, Number>(kBig, big_records);
}

// A batch_server (two record methods, one column method, no fallback) on one
// end of a socketpair, on a thread.
struct served_pair : served_socketpair {
    explicit served_pair(uint64_t batch = kBatch) : served_socketpair(batch, register_all) {}
};

static uint64_t mix(uint64_t i) {
    uint64_t z = (i + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    return z ^ (z >> 27);
}
static TwoNumbers two(uint64_t i) {
    TwoNumbers q;
    q.a = static_cast<int32_t>(mix(i));
    q.b = static_cast<int32_t>(mix(i) >> 32);
    return q;
}
static Big big(uint64_t i) {
    Big q;
    uint64_t k = 0;
    srpc::gpu::for_each_leaf<Big>(q, [&](auto& v) { v = static_cast<int64_t>(mix(32 * i + k++)); });
    return q;
}
static Wide wide(uint64_t i) {
    const uint64_t z = mix(i);
    Wide q;
    q.k_bool = z & 1;
    q.k_i8 = static_cast<int8_t>(z >> 1);
    q.k_char = static_cast<char>(z >> 9);
    q.k_i16 = static_cast<int16_t>(z >> 17);
    q.k_i32 = static_cast<int32_t>(z >> 33);
    q.k_i64 = static_cast<int64_t>(mix(z));
    return q;
}

// A proto whose every byte outside the leaves is told apart from zero and from
// the 0xA5 the reply array starts with.
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

// The bytes call_records must leave for a reply: the proto's, with `leaves`' leaf fields.
template <class T>
static std::vector<uint8_t> struct_bytes(T const& proto, T const& leaves) {
    std::vector<uint8_t> out(reinterpret_cast<const uint8_t*>(&proto), reinterpret_cast<const uint8_t*>(&proto) + sizeof(T));
    const std::vector<uint32_t> offs = srpc::gpu::leaf_offsets<T>();
    size_t f = 0;
    srpc::gpu::for_each_leaf<T>(leaves, [&](const auto& v) { std::memcpy(out.data() + offs[f++], &v, sizeof(v)); });
    return out;
}

template <class T>
struct device_array {
    T* p = nullptr;
    uint64_t n;
    explicit device_array(uint64_t n, int fill = 0xA5) : n(n) {
        HIPCHECK(hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T) + 16));
        HIPCHECK(hipMemset(p, fill, n * sizeof(T) + 16));
    }
    void put(const void* src) { HIPCHECK(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice)); }
    std::vector<uint8_t> bytes(uint64_t extra = 0) const {
        std::vector<uint8_t> out(n * sizeof(T) + extra);
        HIPCHECK(hipMemcpy(out.data(), p, out.size(), hipMemcpyDeviceToHost));
        return out;
    }
    ~device_array() { (void)hipFree(p); }
};

// Raw bytes of host objects (the one DMA a caller makes of its std::vector<T>).
template <class T>
static std::vector<uint8_t> raw(std::vector<T> const& v) {
    std::vector<uint8_t> out(v.size() * sizeof(T));
    if (!v.empty()) std::memcpy(static_cast<void*>(out.data()), static_cast<const void*>(v.data()), out.size());
    return out;
}

// call_records of kCalls calls of one record method; unknown(i): call i is
// rewritten to a method nobody registered.  Compares every struct and code.
template <class Req, class Resp, class Make, class Answer, class Unknown>
static srpc::gpu::call_stats records_case(std::string const& method, Make make, Answer answer, Unknown unknown,
                                          uint64_t* n_unknown) {
    served_pair sp;
    std::vector<Req> reqs(kCalls);
    for (uint64_t i = 0; i < kCalls; ++i) reqs[i] = make(i);
    device_array<Req> d_req(kCalls);
    d_req.put(raw(reqs).data());
    device_array<Resp> d_resp(kCalls);
    device_array<uint8_t> d_codes(kCalls);
    Resp proto{};
    mark_padding(proto);
    srpc::gpu::batch_client cl(sp.fd, kBatch);
    cl.set_request_hook([&](uint8_t* frames, uint64_t first, uint64_t m, uint64_t fin) {
        // frame: BE32 | u64 len | method ...: another first letter is a method nobody registered
        for (uint64_t i = 0; i < m; ++i)
            if (unknown(first + i)) frames[i * fin + 12] = 'X';
    });
    const srpc::gpu::call_stats st = cl.call_records<Req, Resp>(method, d_req.p, kCalls, d_resp.p, d_codes.p, proto);
    const std::vector<uint8_t> got = d_resp.bytes(16), codes = d_codes.bytes(16);
    bool structs = true, right_codes = true;
    *n_unknown = 0;
    for (uint64_t i = 0; i < kCalls; ++i) {
        const bool u = unknown(i);
        *n_unknown += u;
        const std::vector<uint8_t> want = struct_bytes(proto, u ? Resp{} : answer(reqs[i]));
        structs = structs && std::memcmp(got.data() + i * sizeof(Resp), want.data(), sizeof(Resp)) == 0;
        right_codes = right_codes && codes[i] == (u ? srpc::RPC_ERR_FUNCTION_NOT_REGISTERED : srpc::RPC_SUCCESS);
    }
    CHECK(structs);
    CHECK(right_codes);
    bool guards = true;
    for (uint64_t k = 0; k < 16; ++k)
        guards = guards && got[kCalls * sizeof(Resp) + k] == 0xA5 && codes[kCalls + k] == 0xA5;
    CHECK(guards);
    CHECK(st.calls == kCalls && st.chunks == 5 && st.malformed == 0 && st.unanswered == 0);
    CHECK(st.ok == kCalls - *n_unknown && st.failed == *n_unknown);
    sp.finish();
    CHECK(sp.stats.requests == kCalls && sp.stats.fallback_requests == *n_unknown);
    return st;
}

static void layouts_match_the_kernels() {
    using srpc::gpu::leaf_offsets;
    CHECK(sizeof(TwoNumbers) == 16 && leaf_offsets<TwoNumbers>() == (std::vector<uint32_t>{8, 12}));
    CHECK(sizeof(Number) == 16 && leaf_offsets<Number>() == (std::vector<uint32_t>{8}));
    CHECK(sizeof(Wide) == 32 && leaf_offsets<Wide>() == (std::vector<uint32_t>{8, 9, 10, 12, 16, 24}));
    CHECK(sizeof(Big) == 264 && leaf_offsets<Big>().size() == 32 && leaf_offsets<Big>()[31] == 256);
    CHECK(sizeof(Odd) == 24 && leaf_offsets<Odd>() == (std::vector<uint32_t>{8, 16}));
}

static void all_registered() {
    const auto none = [](uint64_t) { return false; };
    uint64_t u = 0;
    srpc::gpu::call_stats st = records_case<TwoNumbers, Number>(kAdd, two, add_of, none, &u);
    CHECK(st.uniform_chunks == 5);  // only full frames: no offsets were used
    st = records_case<Wide, Wide>(kWide, wide, wide_of, none, &u);
    CHECK(st.uniform_chunks == 5);
    st = records_case<Big, Number>(kBig, big, big_of, none, &u);  // a Req of more than 256 bytes
    CHECK(st.uniform_chunks == 5);
}

static void every_tenth_unknown() {
    const auto tenth = [](uint64_t i) { return i % 10 == 3; };
    uint64_t u = 0;
    srpc::gpu::call_stats st = records_case<TwoNumbers, Number>(kAdd, two, add_of, tenth, &u);
    CHECK(u == 500 && st.uniform_chunks == 0);
    st = records_case<Wide, Wide>(kWide, wide, wide_of, tenth, &u);
    CHECK(u == 500 && st.uniform_chunks == 0);
}

// The same calls through the column form, and the column method beside the record ones.
static void columns_give_the_same() {
    served_pair sp;
    std::vector<int32_t> a(kCalls), b(kCalls), sum(kCalls);
    for (uint64_t i = 0; i < kCalls; ++i) {
        const TwoNumbers q = two(i);
        a[i] = q.a;
        b[i] = q.b;
    }
    device_array<int32_t> d_a(kCalls), d_b(kCalls), d_sum(kCalls), d_echo(kCalls);
    device_array<uint8_t> d_codes(kCalls);
    d_a.put(a.data());
    d_b.put(b.data());
    srpc::gpu::batch_client cl(sp.fd, kBatch);
    void* rq[2] = {d_a.p, d_b.p};
    void* rs[1] = {d_sum.p};
    srpc::gpu::call_stats st = cl.call<TwoNumbers, Number>(kAdd, rq, kCalls, rs, d_codes.p);
    CHECK(st.ok == kCalls && st.chunks == 5);
    std::vector<uint8_t> got = d_sum.bytes(), codes = d_codes.bytes();
    bool same = true;
    for (uint64_t i = 0; i < kCalls; ++i) {
        const int32_t want = add_of(two(i)).num;
        same = same && std::memcmp(got.data() + 4 * i, &want, 4) == 0 && codes[i] == srpc::RPC_SUCCESS;
    }
    CHECK(same);
    void* erq[1] = {d_a.p};
    void* ers[1] = {d_echo.p};
    st = cl.call<Number, Number>(kEcho, erq, kCalls, ers, d_codes.p);
    CHECK(st.ok == kCalls);
    got = d_echo.bytes();
    CHECK(std::memcmp(got.data(), a.data(), 4 * kCalls) == 0);
    sp.finish();
    CHECK(sp.stats.requests == 2 * kCalls && sp.stats.fallback_requests == 0);
}

// A peer that answers 1029 calls (five replies into the second chunk) and
// closes: the rest get RPC_ERR_RECV_TIMEOUT and the proto with zero leaves.
// Odd is 24 bytes, so the first unanswered struct starts off a 16-byte boundary.
static void peer_closes_after_the_first_chunk() {
    constexpr uint64_t n = 3000, answered = kBatch + 5;
    const uint64_t fin = srpc::gpu::framed_request_prefix<TwoNumbers>(kOdd).size() + 8;
    auto odd_of = [](TwoNumbers const& q) {
        Odd r;
        r.sum = static_cast<int64_t>(q.a) + q.b;
        r.diff = static_cast<int32_t>(static_cast<uint32_t>(q.a) - static_cast<uint32_t>(q.b));
        return r;
    };
    int sv[2];
    if (socketpair(AF_UNIX, SOCK_STREAM, 0, sv) != 0) std::exit(2);
    std::thread peer([fd = sv[1], fin, odd_of] {
        std::vector<uint8_t> in;
        uint8_t tmp[4096];
        uint64_t done = 0;
        bool open = true;
        while (true) {
            const ssize_t k = recv(fd, tmp, sizeof tmp, 0);
            if (k <= 0) break;
            in.insert(in.end(), tmp, tmp + k);
            while (open && in.size() >= (done + 1) * fin) {
                TwoNumbers q;
                std::memcpy(&q.a, in.data() + done * fin + fin - 8, 4);
                std::memcpy(&q.b, in.data() + done * fin + fin - 4, 4);
                srpc::packer p;
                srpc::response_t<Odd> r;
                r.set_value(odd_of(q));
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
        std::vector<TwoNumbers> reqs(n);
        for (uint64_t i = 0; i < n; ++i) reqs[i] = two(i);
        device_array<TwoNumbers> d_req(n);
        d_req.put(raw(reqs).data());
        device_array<Odd> d_resp(n);
        device_array<uint8_t> d_codes(n);
        Odd proto{};
        mark_padding(proto);
        srpc::gpu::batch_client cl(sv[0], kBatch);
        const srpc::gpu::call_stats st = cl.call_records<TwoNumbers, Odd>(kOdd, d_req.p, n, d_resp.p, d_codes.p, proto);
        const std::vector<uint8_t> got = d_resp.bytes(16), codes = d_codes.bytes(16);
        bool structs = true, right_codes = true;
        for (uint64_t i = 0; i < n; ++i) {
            const std::vector<uint8_t> want = struct_bytes(proto, i < answered ? odd_of(reqs[i]) : Odd{});
            structs = structs && std::memcmp(got.data() + i * sizeof(Odd), want.data(), sizeof(Odd)) == 0;
            right_codes = right_codes && codes[i] == (i < answered ? srpc::RPC_SUCCESS : srpc::RPC_ERR_RECV_TIMEOUT);
        }
        CHECK(structs);
        CHECK(right_codes);
        bool guards = true;
        for (uint64_t k = 0; k < 16; ++k) guards = guards && got[n * sizeof(Odd) + k] == 0xA5 && codes[n + k] == 0xA5;
        CHECK(guards);
        CHECK(st.ok == answered && st.unanswered == n - answered && st.failed == 0 && st.malformed == 0);
        CHECK(st.chunks == 3);
    }
    close(sv[0]);
    peer.join();
}

static void refusals() {
    int sv[2];
    if (socketpair(AF_UNIX, SOCK_STREAM, 0, sv) != 0) std::exit(2);
    // ordered mode, either kind, with a record method registered
    for (int var = 0; var < 2; ++var) {
        srpc::gpu::batch_server srv(kBatch);
        register_all(srv);
        if (var) srv.set_ordered_var(true);
        else srv.set_ordered(true);
        int code = 0;
        try {
            (void)srv.serve_connection(sv[1]);
        } catch (srpc::gpu::plan_error const& e) {
            code = e.code;
        }
        CHECK(code == SRPC_E_UNSUPPORTED);
    }
    // a string schema on either side is refused before the arrays are looked at: null will do
    srpc::gpu::batch_client cl(sv[0], kBatch);
    int code = 0;
    try {
        (void)cl.call_records<Text, Number>(kAdd, nullptr, 3, nullptr, nullptr);
    } catch (srpc::gpu::plan_error const& e) {
        code = e.code;
    }
    CHECK(code == SRPC_E_UNSUPPORTED);
    code = 0;
    try {
        (void)cl.call_records<Number, Text>(kAdd, nullptr, 3, nullptr, nullptr);
    } catch (srpc::gpu::plan_error const& e) {
        code = e.code;
    }
    CHECK(code == SRPC_E_UNSUPPORTED);
    code = 0;
    try {
        srpc::gpu::batch_server srv(kBatch);
        srv.register_record_method<Text, Number>(kAdd, add_records);
    } catch (srpc::gpu::plan_error const& e) {
        code = e.code;
    }
    CHECK(code == SRPC_E_UNSUPPORTED);
    close(sv[0]);
    close(sv[1]);
}

// `gpu_records_test bench N`: N add calls each way on the same records, in
// chunks of 2^18 -- call_records from a device copy of the vector, and the
// host-vector form of `call`, which transposes on the CPU both ways.  Not a
// test: it prints the host wall time and call_stats::gpu_seconds of each, and
// `rest`: the wall time outside the GPU steps and the socket (the host's
// copies, and for the vector form its transposes).
static int bench(uint64_t n) {
    constexpr uint64_t batch = 1u << 18;
    std::vector<TwoNumbers> reqs(n);
    for (uint64_t i = 0; i < n; ++i) reqs[i] = two(i);
    using clk = std::chrono::steady_clock;
    auto secs = [](clk::time_point t0) { return std::chrono::duration<double>(clk::now() - t0).count(); };
    for (int round = 0; round < 6; ++round) {  // round 0 warms both forms up
        {
            served_pair sp(batch);
            srpc::gpu::batch_client cl(sp.fd, batch);
            device_array<TwoNumbers> d_req(n);
            device_array<Number> d_resp(n);
            device_array<uint8_t> d_codes(n);
            std::vector<Number> out(n);
            const auto t0 = clk::now();
            d_req.put(static_cast<const void*>(reqs.data()));
            const srpc::gpu::call_stats st = cl.call_records<TwoNumbers, Number>(kAdd, d_req.p, n, d_resp.p, d_codes.p);
            HIPCHECK(hipMemcpy(static_cast<void*>(out.data()), d_resp.p, n * sizeof(Number), hipMemcpyDeviceToHost));
            const double wall = secs(t0);
            bool ok = st.ok == n;
            for (uint64_t i = 0; i < n; i += 997) ok = ok && out[i].num == add_of(reqs[i]).num;
            std::printf("round %d call_records       n=%llu wall %.4f s (copies of the struct arrays included) gpu_seconds %.4f "
                        "send %.4f recv %.4f rest %.4f %s\n",
                        round, static_cast<unsigned long long>(n), wall, st.gpu_seconds, st.send_seconds, st.recv_seconds,
                        wall - st.gpu_seconds - st.send_seconds - st.recv_seconds, ok ? "ok" : "WRONG");
            sp.finish();
        }
        {
            served_pair sp(batch);
            srpc::gpu::batch_client cl(sp.fd, batch);
            const auto t0 = clk::now();
            const std::vector<srpc::response_t<Number>> got = cl.call<TwoNumbers, Number>(kAdd, reqs);
            const double wall = secs(t0);
            const srpc::gpu::call_stats st = cl.last_stats();
            bool ok = st.ok == n;
            for (uint64_t i = 0; i < n; i += 997) ok = ok && got[i].value().num == add_of(reqs[i]).num;
            std::printf("round %d call(vector<Req>)  n=%llu wall %.4f s (host transposes and column copies included) gpu_seconds "
                        "%.4f send %.4f recv %.4f rest %.4f %s\n",
                        round, static_cast<unsigned long long>(n), wall, st.gpu_seconds, st.send_seconds, st.recv_seconds,
                        wall - st.gpu_seconds - st.send_seconds - st.recv_seconds, ok ? "ok" : "WRONG");
            sp.finish();
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    HIPCHECK(hipSetDevice(0));
    compile_kernels();
    if (argc == 3 && std::string(argv[1]) == "bench") return bench(std::strtoull(argv[2], nullptr, 10));
    layouts_match_the_kernels();
    all_registered();
    every_tenth_unknown();
    columns_give_the_same();
    peer_closes_after_the_first_chunk();
    refusals();
    std::printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
