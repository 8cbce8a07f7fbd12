// srpc/gpu_server.hpp -- GPU-batched request serving.
//
// The reference server (include/srpc/server.hpp:45-74) handles one request at
// a time: recv_data -> `>> funcname` -> call -> getv<I> -> method ->
// pack_response -> send_data.  For streams of requests of methods with
// fixed-size bodies (Calculator.square: 57-byte frames = u32 BE 53 | 53-byte
// request), batch_server serves whole batches on the GPU with the same frames
// on the wire.
//
// Every batch goes through one skeleton (process_begin / process_end):
//
//   socket -> pinned host buffer (the CPU only walks the BE32 frame lengths)
//   -> H2D of the frames and their offsets -> the route's steps, which leave
//   the reply stream in the device's reply buffer, the number of frames that
//   go to the CPU and where each answer ends -> D2H of the replies (the class
//   bytes when a frame goes to the CPU, the statuses) -> an event; once it
//   fired, the GPU's answers are sent in runs with the CPU's in their places.
//
// A frame no registered method matches (another method, a corrupt header or
// string length, trailing bytes) is answered on the CPU by an ordinary
// srpc::server, in its place in the reply order; only those frames leave the
// GPU path.  A frame longer than the batch buffer is read on its own and
// answered the same way.  The routes are the skeleton's middle:
//
// The bucket route (the default):
//
//   srpc_frames_classify (each frame against every registered method's
//   constant `BE32 len | str(method) | str(Req::name)` prefix and length;
//   per-method buckets; each response's offset in the reply stream)
//   -> per method: srpc_frames_gather -> srpc_gpu_unpack -> user device
//   handler -> srpc_gpu_pack (`BE32 len | code | str(Resp::name) | body`
//   frames) -> srpc_frames_scatter into request order.
//
// A batch of one method skips the gather and scatter (its frames are already
// the plan's contiguous records).  Methods with string fields
// (register_var_method) take the variable-length form of each step:
// srpc_frames_classify matches their frames by `str(method) | str(Req::name)`
// after the BE32 and walks their fields to the frame's end;
// srpc_frames_gather_var strips the BE32s and builds the record index ->
// srpc_gpu_unpack_var -> the user's var handler (chars + offsets per string
// field) -> srpc_gpu_pack_var -> srpc_frames_offsets (the reply stream's
// offsets, now that the responses' sizes are known) ->
// srpc_frames_scatter_var (`BE32 len | response` into request order).
// Methods registered with register_record_method take the same steps with a
// handler over arrays of the caller's own structs: srpc_gpu_unpack_aos_fill into
// a Req array -> handler -> srpc_gpu_pack_aos from a Resp array (this route, or
// the ordered records route below).
//
// The buckets are filled with atomics: a handler sees its requests in an order
// that differs from run to run, and no handler sees the order across methods.
// The ordered route (set_ordered / set_ordered_handler; fixed-size methods
// only) serves a batch in arrival order instead:
//
//   srpc_frames_unpack_requests_mixed (every frame classified as above and
//   decoded straight into its method's request columns at its arrival rank)
//   -> the handlers, or the one ordered handler with each frame's method and
//   rank -> srpc_frames_pack_requests_mixed over the framed response plans
//   (the replies in arrival order, nothing for an unknown frame).
//
// No gather, no scatter and no second response buffer, whatever the mix.
//
// The ordered route over string-bodied methods too (set_ordered_var /
// set_ordered_var_handler) is the same decode, handlers and pack through the
// calls that take both plan kinds:
//
//   srpc_frames_unpack_requests_mixed_var (fixed leaves, chars and offsets of
//   every method at their arrival ranks) -> the handlers (a string method's
//   var_handler_t on its n = counts[k] requests), or the one ordered handler
//   -> srpc_frames_pack_requests_mixed_var over the response plans with
//   d_method = d_class -> the total (and, with unknown frames, the offsets).
//
// The ordered route over record methods (set_ordered_records /
// set_ordered_records_handler; every method a register_record_method one with
// sizeof(Req) <= 256) is the same skeleton over the methods' struct arrays:
//
//   srpc_frames_unpack_requests_mixed_aos (every frame classified and decoded
//   into element `arrival rank` of its method's Req array, the bytes no leaf
//   covers a Req{}'s) -> the record handlers on their counts[k] requests, or the
//   one ordered records handler -> srpc_frames_pack_requests_mixed_aos over the
//   framed response plans from the Resp arrays with d_method = d_class.
//
// The reply stream's size is known from the counts, so two batches stay in
// flight as on the fixed ordered route.
//
// The ordered route over methods of all three kinds side by side
// (set_ordered_legs / set_ordered_legs_handler; a record method's sizeof(Req)
// <= 256) is the string route's skeleton through the calls that take, per
// method, columns or a struct array:
//
//   srpc_frames_unpack_requests_mixed_legs (a column or string method's leaves,
//   chars and offsets, a record method's Req structs, all at their arrival
//   ranks) -> the handlers of each kind on their counts[k] requests, or the one
//   ordered legs handler -> srpc_frames_pack_requests_mixed_legs over the
//   response plans with d_method = d_class -> the total (and, with unknown
//   frames, the offsets).  One batch in flight, as on the string route.
//
// On the routes that serve string methods the string responses' sizes are
// checked on the host against their columns before anything reads the chars:
// a method that overflows is answered on the CPU for this batch, its frames
// turned into unknown ones (demote_overflowing).
#pragma once

#include <hip/hip_runtime_api.h>
#include <sys/ioctl.h>
#include <sys/socket.h>
#include <sys/uio.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "gpu.hpp"
#include "server.hpp"
#include "transport.hpp"

namespace srpc::gpu {

inline std::vector<uint8_t> be32(uint32_t v) {
    return {static_cast<uint8_t>(v >> 24), static_cast<uint8_t>(v >> 16), static_cast<uint8_t>(v >> 8),
            static_cast<uint8_t>(v)};
}

/// A plan over an explicit prefix (used for framed envelopes).
class raw_plan {
public:
    raw_plan(std::vector<int32_t> const& kinds, std::vector<uint8_t> const& prefix, int device) {
        srpc_schema_desc d{static_cast<uint32_t>(kinds.size()), kinds.data(), prefix.empty() ? nullptr : prefix.data(),
                           static_cast<uint32_t>(prefix.size())};
        if (int rc = srpc_plan_create(&d, device, &_p); rc != SRPC_OK) throw plan_error("srpc_plan_create", rc);
        srpc_plan_record_bytes(_p, &_rb);
    }
    raw_plan(raw_plan const&) = delete;
    raw_plan& operator=(raw_plan const&) = delete;
    ~raw_plan() {
        if (_p) srpc_plan_destroy(_p);
    }
    srpc_plan* get() const { return _p; }
    uint64_t record_bytes() const { return _rb; }

private:
    srpc_plan* _p = nullptr;
    uint64_t _rb = 0;
};

template <SrpcMessage T>
uint64_t body_bytes() {
    uint64_t s = 0;
    T probe{};
    for_each_leaf<T>(probe, [&](const auto& v) { s += sizeof(v); });
    return s;
}

/// Constant prefix of a framed request: BE32(payload) | str(method) | str(T::name).
template <SrpcMessage T>
std::vector<uint8_t> framed_request_prefix(std::string const& method) {
    std::vector<uint8_t> hdr = request_prefix<T>(method);
    std::vector<uint8_t> out = be32(static_cast<uint32_t>(hdr.size() + body_bytes<T>()));
    out.insert(out.end(), hdr.begin(), hdr.end());
    return out;
}

/// Constant prefix of a framed response: BE32(payload) | code | str(T::name).
template <SrpcMessage T>
std::vector<uint8_t> framed_response_prefix(rpc_status_code code) {
    std::vector<uint8_t> hdr = response_prefix<T>(code);
    std::vector<uint8_t> out = be32(static_cast<uint32_t>(hdr.size() + body_bytes<T>()));
    out.insert(out.end(), hdr.begin(), hdr.end());
    return out;
}

/// Bytes of a record of T with every string empty (prefix excluded): the
/// fixed leaves plus 8 (the length) per string.
template <SrpcMessage T>
uint64_t min_body_bytes() {
    uint64_t s = 0;
    T probe{};
    for_each_leaf<T>(probe, [&](const auto& v) {
        using F = std::remove_cvref_t<decltype(v)>;
        s += std::is_same_v<F, std::string> ? 8 : sizeof(F);
    });
    return s;
}

/// A batch of a string-bodied method on the device, one entry per flattened
/// field of Req / Resp: a fixed field is n values; a string field is its
/// chars back to back (`*_cols[f]`) plus n+1 u64 offsets (`*_str_offs[f]`,
/// nullptr for fixed fields) -- the layout of srpc_gpu_unpack_var /
/// srpc_gpu_pack_var.  The handler writes every response column and the n+1
/// offsets of every response string field (offs[0] need not be 0; at most
/// resp_cap[f] chars).
struct var_batch {
    uint64_t n = 0;
    void* const* req_cols = nullptr;
    const uint64_t* const* req_str_offs = nullptr;
    void* const* resp_cols = nullptr;
    uint64_t* const* resp_str_offs = nullptr;
    const uint64_t* resp_cap = nullptr;  // bytes of each response column
};

/// Sizing of a string-bodied method's buffers (per request of a batch).
struct var_limits {
    uint64_t max_request_bytes = 512;  // frame bytes the receive buffer is sized for
    uint64_t max_response_chars = 256; // chars of one response's string field (batch average)
};

/// A batch in ordered mode (batch_server::set_ordered_handler): the n frames
/// of the batch in arrival order.  Frame i is a request of method d_method[i]
/// (registration order) and element d_rank[i] of that method's columns --
/// req_cols[k][f] / resp_cols[k][f], one column per flattened field of the
/// method's Req / Resp, as handler_t gets them.  d_method[i] ==
/// SRPC_FRAME_UNKNOWN (d_rank[i] == 0xFFFFFFFF): no registered method's frame;
/// the CPU server answers it after the handler ran.  The handler writes element
/// d_rank[i] of method d_method[i]'s response columns for every other frame.
struct ordered_batch {
    uint64_t n = 0;
    const uint8_t* d_method = nullptr;   // device, n
    const uint32_t* d_rank = nullptr;    // device, n
    const uint64_t* counts = nullptr;    // host, methods + 1: frames per method, then the unknown ones
    size_t methods = 0;
    void* const* const* req_cols = nullptr;   // host array per method of device columns
    void* const* const* resp_cols = nullptr;
};

/// A batch in ordered mode with string-bodied methods
/// (batch_server::set_ordered_var_handler): ordered_batch's fields, and per
/// method the offsets arrays of its string leaves -- req_str_offs[k][f] /
/// resp_str_offs[k][f], one entry per flattened field, nullptr for a fixed leaf
/// -- as var_batch has them: request element r's string is bytes [offs[r],
/// offs[r + 1]) of req_cols[k][f], offs[0] == 0.  The handler writes every
/// response column and, for every response string leaf of method k, its
/// counts[k] + 1 offsets (at most resp_cap[k][f] chars).
struct ordered_var_batch {
    uint64_t n = 0;
    const uint8_t* d_method = nullptr;   // device, n
    const uint32_t* d_rank = nullptr;    // device, n
    const uint64_t* counts = nullptr;    // host, methods + 1: frames per method, then the unknown ones
    size_t methods = 0;
    void* const* const* req_cols = nullptr;   // host array per method of device columns
    void* const* const* resp_cols = nullptr;
    const uint64_t* const* const* req_str_offs = nullptr;  // host array per method of per-leaf device pointers
    uint64_t* const* const* resp_str_offs = nullptr;
    const uint64_t* const* resp_cap = nullptr;             // per method: the bytes of each response column
};

/// A batch in ordered records mode (batch_server::set_ordered_records_handler):
/// ordered_batch's n, d_method, d_rank, counts and methods, with one array of
/// the caller's own structs per method and side in place of its columns.  Frame
/// i is element d_rank[i] of method d_method[i]'s Req array -- req_recs[k] +
/// d_rank[i] * req_stride[k], every byte no leaf covers a Req{}'s -- and the
/// handler writes the leaves of element d_rank[i] of resp_recs[k] (zeroed when
/// allocated; only leaves are read).  Unknown frames as in ordered_batch.
struct ordered_records_batch {
    uint64_t n = 0;
    const uint8_t* d_method = nullptr;   // device, n
    const uint32_t* d_rank = nullptr;    // device, n
    const uint64_t* counts = nullptr;    // host, methods + 1: frames per method, then the unknown ones
    size_t methods = 0;
    const void* const* req_recs = nullptr;   // per method: its device Req array
    void* const* resp_recs = nullptr;        // per method: its device Resp array
    const uint64_t* req_stride = nullptr;    // host, per method: sizeof(Req)
    const uint64_t* resp_stride = nullptr;   // host, per method: sizeof(Resp)
};

/// A batch in ordered legs mode (batch_server::set_ordered_legs_handler): the
/// union of ordered_var_batch and ordered_records_batch.  Method k is a column
/// method (fixed-size or string-bodied: the column fields are
/// ordered_var_batch's, the record fields null / 0) or a record method (the
/// record fields are ordered_records_batch's, entry k of every column field
/// null).  Unknown frames as in ordered_batch.
struct ordered_legs_batch {
    uint64_t n = 0;
    const uint8_t* d_method = nullptr;   // device, n
    const uint32_t* d_rank = nullptr;    // device, n
    const uint64_t* counts = nullptr;    // host, methods + 1: frames per method, then the unknown ones
    size_t methods = 0;
    void* const* const* req_cols = nullptr;   // per column method: its device columns
    void* const* const* resp_cols = nullptr;
    const uint64_t* const* const* req_str_offs = nullptr;  // per column method: per-leaf device pointers
    uint64_t* const* const* resp_str_offs = nullptr;
    const uint64_t* const* resp_cap = nullptr;             // per column method: the bytes of each response column
    const void* const* req_recs = nullptr;   // per record method: its device Req array
    void* const* resp_recs = nullptr;        // per record method: its device Resp array
    const uint64_t* req_stride = nullptr;    // host, per method: sizeof(Req), 0 for a column method
    const uint64_t* resp_stride = nullptr;   // host, per method: sizeof(Resp), 0 for a column method
};

struct batch_stats {
    uint64_t requests = 0;           // frames answered
    uint64_t gpu_batches = 0;        // batches that went through the GPU path
    uint64_t gpu_requests = 0;       // frames answered from the GPU
    uint64_t fallback_requests = 0;  // frames answered on the CPU (unknown method / shape)
    uint64_t oversize_requests = 0;  // of those, frames longer than the batch buffer
    uint64_t overflow_batches = 0;   // string-method buckets answered on the CPU: responses past max_response_chars
    uint64_t mixed_batches = 0;      // GPU batches that needed the gather / scatter
    uint64_t h2d_bytes = 0;
    uint64_t d2h_bytes = 0;
    double gpu_seconds = 0;  // H2D + classify + unpack + handler + pack + D2H, host-timed per batch
    double classify_seconds = 0;     // of which: H2D + classify + the counts' D2H (first sync)
    double first_batch_seconds = 0;  // gpu_seconds of the connection's first batch
    double recv_seconds = 0;
    double send_seconds = 0;
    double fallback_seconds = 0;
};

class batch_server {
public:
    /// handler(d_req_cols, d_resp_cols, n, stream): a method over a batch on
    /// the device (one column per flattened field of Req / Resp).
    using handler_t = std::function<int(void* const*, void* const*, uint64_t, hipStream_t)>;
    /// handler(batch, stream) for a method with string fields (var_batch).
    using var_handler_t = std::function<int(var_batch const&, hipStream_t)>;

    /// max_batch: frames per GPU batch; fallback: the CPU server for frames
    /// no registered method matches (nullptr: answered with
    /// RPC_ERR_FUNCTION_NOT_REGISTERED, as the reference does for an unknown name).
    explicit batch_server(uint64_t max_batch = 1u << 20, int device = 0, server* fallback = nullptr)
        : _fallback(fallback), _max(std::max<uint64_t>(max_batch, 1)), _dev(device) {
        check(hipSetDevice(device));
        check(hipStreamCreateWithFlags(&_s, hipStreamNonBlocking));
    }
    /// One method (the round-1 form).
    template <SrpcMessage Req, SrpcMessage Resp>
    static std::unique_ptr<batch_server> single(std::string method, handler_t handler, uint64_t max_batch = 1u << 20,
                                                int device = 0, server* fallback = nullptr) {
        auto s = std::make_unique<batch_server>(max_batch, device, fallback);
        s->register_method<Req, Resp>(std::move(method), std::move(handler));
        return s;
    }
    batch_server(batch_server const&) = delete;
    batch_server& operator=(batch_server const&) = delete;
    ~batch_server() {
        release();
        (void)hipStreamDestroy(_s);
    }

    /// Serve `method` (frames `BE32 | str(method) | str(Req::name) | Req body`)
    /// with `handler` on the device; answers are `BE32 | RPC_SUCCESS |
    /// str(Resp::name) | Resp body` frames.  Up to SRPC_FRAMES_MAX_PLANS methods.
    template <SrpcMessage Req, SrpcMessage Resp>
    void register_method(std::string method, handler_t handler) {
        add_method<Req, Resp>("batch_server::register_method", std::move(method), false).handler = std::move(handler);
    }

    /// handler(d_reqs, d_resps, n, stream): a method over a batch of the
    /// caller's own structs on the device -- d_reqs is n Req objects, d_resps n
    /// Resp objects (the kernel a servicer ported from the reference wants: one
    /// thread per Req, write one Resp).
    using record_handler_t = std::function<int(const void* d_reqs, void* d_resps, uint64_t n, hipStream_t)>;

    /// register_method for a handler over struct arrays (fixed-size Req and
    /// Resp; a string schema throws plan_error SRPC_E_UNSUPPORTED).  The same
    /// frames on the wire and the same bucket route, with the AoS kernels in
    /// place of the column ones: classify -> gather -> srpc_gpu_unpack_aos_fill
    /// (framed request plan) into a Req array -> handler ->
    /// srpc_gpu_pack_aos (framed response plan) from a Resp array -> scatter.
    /// Every byte of a d_reqs[i] that no leaf covers is a Req{}'s (for
    /// sizeof(Req) > 256 the array is filled with Req{} once and
    /// srpc_gpu_unpack_aos writes the leaves); the Resp array is zeroed when it
    /// is allocated and only its leaves are read, so the handler writes the
    /// leaves and nothing else matters.  Handlers must not call a virtual
    /// function on these objects: a vtable slot holds a host pointer (Req) or
    /// zero (Resp).  Record methods and column methods mix freely in one server.
    /// The bucket route, or arrival order with set_ordered_records (record
    /// methods only) or set_ordered_legs (beside column and string methods):
    /// with a record method registered, serve_connection throws
    /// plan_error(SRPC_E_UNSUPPORTED) in set_ordered / set_ordered_var mode.
    template <SrpcMessage Req, SrpcMessage Resp>
    void register_record_method(std::string method, record_handler_t handler) {
        method_entry& m = add_method<Req, Resp>("batch_server::register_record_method", std::move(method), false, true);
        m.rec = true;
        m.rhandler = std::move(handler);
        m.req_stride = sizeof(Req);
        m.resp_stride = sizeof(Resp);
        m.req_loffs = leaf_offsets<Req>();
        m.resp_loffs = leaf_offsets<Resp>();
        const Req proto{};
        m.req_fill.assign(reinterpret_cast<const uint8_t*>(&proto), reinterpret_cast<const uint8_t*>(&proto) + sizeof(Req));
    }

    /// Serve `method` whose request and/or response has string fields: frames
    /// `BE32 | str(method) | str(Req::name) | Req record`, answered with
    /// `BE32 | RPC_SUCCESS | str(Resp::name) | Resp record` frames; `handler`
    /// runs on whole batches of them (var_batch).  The receive buffer holds
    /// max_batch frames of lim.max_request_bytes; longer frames still batch
    /// while they fit, and one longer than the whole buffer is answered on
    /// the CPU.  Up to SRPC_FRAMES_MAX_STRINGS string fields in Req.
    template <SrpcMessage Req, SrpcMessage Resp>
    void register_var_method(std::string method, var_handler_t handler, var_limits lim = {}) {
        method_entry& m = add_method<Req, Resp>("batch_server::register_var_method", std::move(method), true);
        m.vhandler = std::move(handler);
        m.fin = std::max<uint64_t>(lim.max_request_bytes, 4 + m.min_in);
        m.fout = 0;  // response frames vary
        m.lim = lim;
    }

    /// handler(batch, stream) over a whole batch of every method in arrival
    /// order (ordered_batch).
    using ordered_handler_t = std::function<int(ordered_batch const&, hipStream_t)>;

    /// Ordered mode (off by default).  The bucket route hands each method its
    /// requests in an order that differs from run to run; in ordered mode
    /// request r of a method's batch is the r-th frame of that method in
    /// arrival order, and the batch goes through one
    /// srpc_frames_unpack_requests_mixed and one srpc_frames_pack_requests_mixed
    /// over the response plans whatever its mix: no gather, no scatter.
    /// Fixed-size methods only: serve_connection throws
    /// plan_error(SRPC_E_UNSUPPORTED) when a register_var_method method is
    /// present.
    void set_ordered(bool on) {
        if (on == _ordered) return;
        _ordered = on;
        if (!on) _ordered_var = _ordered_rec = _ordered_legs = false;
        release();
    }
    bool ordered() const { return _ordered; }
    /// One handler for every method, run once per batch instead of the
    /// per-method handlers; implies ordered mode.  Batches reach it in
    /// connection order on the server's stream, so device state it keeps sees
    /// the registered methods' requests in the order they arrived, across
    /// methods.  Frames the GPU path does not take (a method nobody registered,
    /// a malformed frame) are answered by the CPU server AFTER the batch's
    /// handler ran: a service that needs a total order registers all its
    /// methods.  At serve start it is run once on a batch of one unknown frame
    /// (every counts[k] == 0), as the per-method handlers are run on one zero
    /// record.
    void set_ordered_handler(ordered_handler_t handler) {
        _ohandler = std::move(handler);
        set_ordered(true);
    }

    /// handler(batch, stream) over a whole batch of every method, string-bodied
    /// ones included, in arrival order (ordered_var_batch).
    using ordered_var_handler_t = std::function<int(ordered_var_batch const&, hipStream_t)>;

    /// Ordered mode that admits register_var_method methods (off by default;
    /// implies ordered mode).  Fixed methods keep their handler_t; a string
    /// method's var_handler_t gets a var_batch with n = counts[k] whose request r
    /// is the method's r-th frame in arrival order (its request offsets start at
    /// 0).  A batch goes through one srpc_frames_unpack_requests_mixed_var and
    /// one srpc_frames_pack_requests_mixed_var over the response plans.  A string
    /// method whose responses do not fit their columns (var_limits) is answered
    /// by the CPU server for that batch, its frames in their places
    /// (batch_stats::overflow_batches); the other methods' elements do not move.
    /// One batch is in flight at a time: the route syncs for the reply stream's
    /// size.  set_ordered / set_ordered_handler keep refusing string methods.
    void set_ordered_var(bool on) {
        if (on == _ordered_var && on == _ordered) return;
        _ordered_var = on;
        _ordered = on;
        _ordered_rec = _ordered_legs = false;
        release();
    }
    bool ordered_var() const { return _ordered_var; }
    /// One handler for every method, string-bodied ones included, run once per
    /// batch instead of the per-method handlers; implies set_ordered_var(true).
    /// Timing and warm-up are set_ordered_handler's: batches reach it in
    /// connection order on the server's stream, frames the GPU path does not
    /// take are answered by the CPU server after the batch's handler ran, and at
    /// serve start it is run on a batch of one unknown frame.
    void set_ordered_var_handler(ordered_var_handler_t handler) {
        _ovhandler = std::move(handler);
        set_ordered_var(true);
    }

    /// handler(batch, stream) over a whole batch of every record method in
    /// arrival order (ordered_records_batch).
    using ordered_records_handler_t = std::function<int(ordered_records_batch const&, hipStream_t)>;

    /// Ordered mode over register_record_method methods (off by default; implies
    /// ordered mode; set_ordered(false) clears it).  Request r of a method's
    /// batch is the method's r-th frame in arrival order: a record handler sees
    /// (d_reqs, d_resps, counts[k]) with its requests in the order they came, in
    /// every run and across batches.  A batch goes through one
    /// srpc_frames_unpack_requests_mixed_aos into the methods' Req arrays (every
    /// byte no leaf covers a Req{}'s) and one srpc_frames_pack_requests_mixed_aos
    /// over the response plans from their Resp arrays: no gather, no scatter, two
    /// batches in flight.  Every registered method must be a record method with
    /// sizeof(Req) <= 256 (sizeof(Resp) is free): serve_connection throws
    /// plan_error(SRPC_E_UNSUPPORTED) for a register_method or
    /// register_var_method method beside them, or a larger Req.  set_ordered /
    /// set_ordered_var keep refusing record methods.
    void set_ordered_records(bool on) {
        if (on == _ordered_rec && on == _ordered) return;
        _ordered_rec = on;
        _ordered = on;
        _ordered_var = _ordered_legs = false;
        release();
    }
    bool ordered_records() const { return _ordered_rec; }
    /// One handler for every record method, run once per batch instead of the
    /// per-method handlers; implies set_ordered_records(true).  Timing and
    /// warm-up are set_ordered_handler's: batches reach it in connection order on
    /// the server's stream, frames the GPU path does not take are answered by the
    /// CPU server after the batch's handler ran, and at serve start it is run on
    /// a batch of one unknown frame.
    void set_ordered_records_handler(ordered_records_handler_t handler) {
        _orhandler = std::move(handler);
        set_ordered_records(true);
    }

    /// handler(batch, stream) over a whole batch of every method of any kind in
    /// arrival order (ordered_legs_batch).
    using ordered_legs_handler_t = std::function<int(ordered_legs_batch const&, hipStream_t)>;

    /// Ordered mode that admits register_method, register_var_method and
    /// register_record_method methods side by side (off by default; implies
    /// ordered mode and clears set_ordered_var / set_ordered_records;
    /// set_ordered(false) clears it).  Request r of a method's batch is the
    /// method's r-th frame in arrival order, whatever its kind: a column method
    /// keeps its handler_t, a string method's var_handler_t gets a var_batch with
    /// n = counts[k] (its request offsets start at 0), a record method's handler
    /// gets (const Req*, Resp*, counts[k]) with every byte no leaf covers a
    /// Req{}'s.  A batch goes through one srpc_frames_unpack_requests_mixed_legs
    /// and one srpc_frames_pack_requests_mixed_legs over the response plans.
    /// Timing and overflow handling are set_ordered_var's: one batch is in flight,
    /// the route syncs for the reply stream's size, and a string method whose
    /// responses do not fit their columns is answered by the CPU server for that
    /// batch (batch_stats::overflow_batches) while the other methods' elements do
    /// not move.  serve_connection throws plan_error(SRPC_E_UNSUPPORTED) for a
    /// record method with sizeof(Req) > 256 (sizeof(Resp) is free).  set_ordered,
    /// set_ordered_var and set_ordered_records keep refusing what they refuse.
    void set_ordered_legs(bool on) {
        if (on == _ordered_legs && on == _ordered) return;
        _ordered_legs = on;
        _ordered = on;
        _ordered_var = _ordered_rec = false;
        release();
    }
    bool ordered_legs() const { return _ordered_legs; }
    /// One handler for every method of any kind, run once per batch instead of
    /// the per-method handlers; implies set_ordered_legs(true).  Timing, warm-up
    /// and the treatment of unknown frames are set_ordered_handler's: batches
    /// reach it in connection order on the server's stream, frames the GPU path
    /// does not take are answered by the CPU server after the batch's handler ran,
    /// and at serve start it is run on a batch of one unknown frame.
    void set_ordered_legs_handler(ordered_legs_handler_t handler) {
        _olhandler = std::move(handler);
        set_ordered_legs(true);
    }

    uint64_t request_frame_bytes(size_t k = 0) const { return _m.at(k)->fin; }
    uint64_t response_frame_bytes(size_t k = 0) const { return _m.at(k)->fout; }
    /// Bytes of the receive buffer: max_batch frames of the longest method.
    uint64_t buffer_bytes() const { return _max * max_fin(); }

    /// Serve one connected socket until the peer closes it.
    ///
    /// Servers whose methods are all fixed-size run two batches in flight:
    /// batch k's copies and kernels are enqueued (process_begin) and the next
    /// batch is received into the other half of the double-buffered pinned
    /// staging while they run; batch k's answers are sent (process_end) once
    /// batch k + 1 is enqueued -- or before any recv that would block, so a
    /// peer that waits for every answer before it closes is never kept
    /// waiting.  Answers leave in request order.
    batch_stats serve_connection(int fd) {
        if (_m.empty()) throw plan_error("batch_server::serve_connection (no methods)", SRPC_E_INVALID);
        if (_ordered && !strings_route() && any_var_method())
            throw plan_error("batch_server::serve_connection (ordered mode with a string-bodied method)",
                             SRPC_E_UNSUPPORTED);
        if (_ordered && !_ordered_rec && !_ordered_legs && any_record_method())
            throw plan_error("batch_server::serve_connection (ordered mode with a record method)", SRPC_E_UNSUPPORTED);
        if (_ordered_rec)
            for (auto const& m : _m) {
                if (m->var)
                    throw plan_error("batch_server::serve_connection (ordered records mode with a string-bodied method)",
                                     SRPC_E_UNSUPPORTED);
                if (!m->rec)
                    throw plan_error("batch_server::serve_connection (ordered records mode with a column method)",
                                     SRPC_E_UNSUPPORTED);
                if (m->req_stride > kRecordFillMax)
                    throw plan_error("batch_server::serve_connection (ordered records mode with a Req above 256 bytes)",
                                     SRPC_E_UNSUPPORTED);
            }
        if (_ordered_legs)
            for (auto const& m : _m)
                if (m->rec && m->req_stride > kRecordFillMax)
                    throw plan_error("batch_server::serve_connection (ordered legs mode with a Req above 256 bytes)",
                                     SRPC_E_UNSUPPORTED);
        check(hipSetDevice(_dev));
        ensure();
        batch_stats st;
        const uint64_t cap = _cap;
        uint64_t have = 0;     // bytes in h_in
        uint64_t walked = 0;   // bytes of whole frames found so far (frames h_offs[0..nf))
        uint64_t nf = 0;
        bool eof = false;
        bool buffered = false;  // whole frames already wait in h_in: walk them before blocking in recv
        int cur = 0;            // the staging slot frames are received into
        uint8_t* h_in = _slots[cur].h_in;
        uint32_t* h_offs = _slots[cur].h_offs;
        pending pend;
        auto finish = [&] {
            if (!pend.valid) return;
            process_end(fd, pend, st);
            pend.valid = false;
        };
        while (true) {
            if (!eof && !buffered) {
                // answer a batch in flight before a recv that would block
                if (pend.valid && !more_pending(fd)) finish();
                // cap - have > 0 here: a full buffer is always consumed below,
                // so recv returning 0 is the peer's orderly shutdown
                auto t0 = clock::now();
                ssize_t k = recv(fd, h_in + have, cap - have, 0);
                if (k < 0 && errno == EINTR) continue;
                st.recv_seconds += secs(t0);
                if (k <= 0) eof = true;
                else have += static_cast<uint64_t>(k);
            }
            buffered = false;
            // frame boundaries (the only per-frame CPU work on the fast path)
            uint64_t next_len = 0;
            bool next_hdr = false;
            while (nf < _max && have - walked >= 4) {
                next_len = 4 + static_cast<uint64_t>(be32_at(h_in + walked));
                next_hdr = true;
                if (have - walked < next_len) break;
                h_offs[nf++] = static_cast<uint32_t>(walked);
                walked += next_len;
                next_hdr = false;
            }
            const bool oversize = next_hdr && next_len > cap;
            const bool full = nf == _max || have == cap || oversize;
            if (_trace)
                std::fprintf(stderr, "recv: have %llu walked %llu nf %llu next %llu%s%s\n", (unsigned long long)have,
                             (unsigned long long)walked, (unsigned long long)nf, (unsigned long long)next_len,
                             eof ? " eof" : "", full ? " full" : "");
            if (nf == 0 && !oversize) {
                if (eof) break;
                continue;
            }
            if (!full && !eof && more_pending(fd)) continue;  // fill the batch while data streams in
            if (nf) {
                if (_nslots == 2) {
                    pending p = process_begin(cur, nf, walked, st);
                    finish();  // the previous batch's answers: its work ran while this one arrived
                    pend = p;
                    // the rest of the buffer (a cut frame) continues in the other slot
                    cur ^= 1;
                    std::memcpy(_slots[cur].h_in, h_in + walked, have - walked);
                    h_in = _slots[cur].h_in;
                    h_offs = _slots[cur].h_offs;
                } else {
                    pending p = process_begin(cur, nf, walked, st);
                    process_end(fd, p, st);
                    std::memmove(h_in, h_in + walked, have - walked);
                }
            } else {
                std::memmove(h_in, h_in + walked, have - walked);
            }
            have -= walked;
            walked = 0;
            nf = 0;
            if (oversize) {
                finish();
                if (!serve_oversize(fd, h_in, have, st)) return st;
                have = 0;
            }
            // A batch ends at max_batch frames, so the buffer can still hold
            // whole frames (frames shorter than the method's fin) while the
            // peer, having sent everything, waits for their answers: serve
            // them before the next recv, which would block.
            buffered = have >= 4 && have - 4 >= be32_at(h_in);
        }
        finish();
        return st;  // bytes of a cut final frame are dropped, as the reference's recv_data does
    }

private:
    using clock = std::chrono::steady_clock;
    /// A registered method: what add_method and its register_* built, then the
    /// device buffers and the pointer tables over them (alloc_method; release).
    struct method_entry {
        std::string name;
        bool var = false, rec = false;  // register_var_method, register_record_method
        handler_t handler;
        var_handler_t vhandler;
        record_handler_t rhandler;
        // `in` / `out`: framed fixed-size plans, or (var) string plans behind the unframed prefix
        std::unique_ptr<raw_plan> in, out;
        uint64_t fin = 0, fout = 0;
        std::vector<int32_t> in_kinds, out_kinds;
        std::vector<bool> req_string, resp_string;   // per leaf
        std::vector<uint64_t> req_size, resp_size;   // fixed leaves' bytes (0: a string)
        uint64_t min_in = 0, min_out = 0;            // records with empty strings
        std::vector<uint8_t> req_prefix;             // str(method) | str(Req::name)
        std::vector<uint8_t> framed_in, framed_out;  // BE32(min) | prefix
        var_limits lim;
        // ordered mode with string methods: the plan kinds the *_mixed_var calls take, per side --
        // `in` / `out` where they already are of that kind, else a fixed-size plan behind the framed prefix
        std::unique_ptr<raw_plan> ord_in, ord_out;
        // struct-array methods: no columns; one array per side
        uint64_t req_stride = 0, resp_stride = 0;    // sizeof(Req), sizeof(Resp)
        std::vector<uint32_t> req_loffs, resp_loffs; // leaf_offsets<Req>(), <Resp>()
        std::vector<uint8_t> req_fill;               // a Req{}'s bytes
        device_buffer<uint8_t> d_reqs, d_resps;
        // the columns: per leaf its values or chars, and a string leaf's n+1 offsets
        std::vector<device_buffer<uint8_t>> req_buf, resp_buf;
        std::vector<device_buffer<uint64_t>> req_off_buf, resp_off_buf;
        std::vector<uint64_t> req_bytes, resp_bytes;  // bytes of every column
        std::vector<uint64_t> req_scap;               // of which a decode may fill
        // the bucket route's string methods: packed responses and their index, the response offsets' ends
        device_buffer<uint8_t> resp_wire;
        uint64_t resp_wire_cap = 0;
        device_buffer<uint64_t> resp_rec;
        pinned_buffer<uint64_t> h_ends;               // per response field, offs[0] and offs[n]
        // the tables the library calls and the handlers read (nullptr offsets: a fixed leaf)
        std::vector<void*> req_cols, resp_cols;
        std::vector<const void*> c_resp_cols;
        std::vector<uint64_t*> req_offs, resp_offs;
        std::vector<const uint64_t*> c_req_offs, c_resp_offs;

        bool in_str() const { return std::find(req_string.begin(), req_string.end(), true) != req_string.end(); }
        bool out_str() const { return std::find(resp_string.begin(), resp_string.end(), true) != resp_string.end(); }
        void release() {
            for (auto* v : {&req_buf, &resp_buf}) v->clear();
            for (auto* v : {&req_off_buf, &resp_off_buf}) v->clear();
            d_reqs.reset(), d_resps.reset(), resp_wire.reset(), resp_rec.reset(), h_ends.reset();
            ord_in.reset(), ord_out.reset();
        }
    };

    /// What every register_* shares: the limit, the plans, the per-leaf tables.
    /// var: string plans behind the unframed prefix, else framed fixed-size ones.
    template <SrpcMessage Req, SrpcMessage Resp>
    method_entry& add_method(const char* what, std::string name, bool var, bool fixed_only = false) {
        if (_m.size() >= SRPC_FRAMES_MAX_PLANS) throw plan_error(what, SRPC_E_UNSUPPORTED);
        auto m = std::make_unique<method_entry>();
        m->in_kinds = flat_kinds<Req>();
        m->out_kinds = flat_kinds<Resp>();
        if (fixed_only)
            for (const auto* kinds : {&m->in_kinds, &m->out_kinds})
                for (int32_t k : *kinds)
                    if (k == SRPC_KIND_STRING)
                        throw plan_error((std::string(what) + " (string schema)").c_str(), SRPC_E_UNSUPPORTED);
        check(hipSetDevice(_dev));
        m->name = std::move(name);
        m->var = var;
        m->req_prefix = request_prefix<Req>(m->name);
        const std::vector<uint8_t> rs = response_prefix<Resp>(RPC_SUCCESS);
        m->min_in = m->req_prefix.size() + min_body_bytes<Req>();
        m->min_out = rs.size() + min_body_bytes<Resp>();
        m->framed_in = be32(static_cast<uint32_t>(m->min_in));
        m->framed_in.insert(m->framed_in.end(), m->req_prefix.begin(), m->req_prefix.end());
        m->framed_out = be32(static_cast<uint32_t>(m->min_out));
        m->framed_out.insert(m->framed_out.end(), rs.begin(), rs.end());
        m->in = std::make_unique<raw_plan>(m->in_kinds, var ? m->req_prefix : m->framed_in, _dev);
        m->out = std::make_unique<raw_plan>(m->out_kinds, var ? rs : m->framed_out, _dev);
        m->fin = m->in->record_bytes();
        m->fout = m->out->record_bytes();
        Req rq{};
        for_each_leaf<Req>(rq, [&](const auto& v) {
            using F = std::remove_cvref_t<decltype(v)>;
            m->req_string.push_back(std::is_same_v<F, std::string>);
            m->req_size.push_back(std::is_same_v<F, std::string> ? 0 : sizeof(F));
        });
        Resp rp{};
        for_each_leaf<Resp>(rp, [&](const auto& v) {
            using F = std::remove_cvref_t<decltype(v)>;
            m->resp_string.push_back(std::is_same_v<F, std::string>);
            m->resp_size.push_back(std::is_same_v<F, std::string> ? 0 : sizeof(F));
        });
        _m.push_back(std::move(m));
        release();  // buffers are sized for the largest frames on the next serve
        return *_m.back();
    }

    static double secs(clock::time_point t0) { return std::chrono::duration<double>(clock::now() - t0).count(); }
    static void check(hipError_t e) {
        if (e != hipSuccess) throw std::runtime_error(std::string("HIP: ") + hipGetErrorString(e));
    }
    static void check_srpc(int rc, const char* what) {
        if (rc < 0) throw plan_error(what, rc);
    }
    static uint32_t be32_at(const uint8_t* b) {
        return (uint32_t(b[0]) << 24) | (uint32_t(b[1]) << 16) | (uint32_t(b[2]) << 8) | uint32_t(b[3]);
    }
    static bool more_pending(int fd) {
        int avail = 0;
        return ::ioctl(fd, FIONREAD, &avail) == 0 && avail > 0;
    }
    uint64_t max_fin() const {
        uint64_t f = 0;
        for (auto const& m : _m) f = std::max(f, m->fin);
        return f;
    }
    uint64_t max_fout() const {
        uint64_t f = 0;
        for (auto const& m : _m) f = std::max(f, m->fout);
        return f;
    }
    /// Bytes of a batch's reply stream: every frame of the widest fixed
    /// response, plus every string method's framed responses.
    uint64_t out_cap() const {
        uint64_t c = _max * max_fout();
        for (auto const& m : _m)
            if (m->var) c += m->resp_wire_cap + 4 * _max;
        return c;
    }
    bool any_var_method() const {
        for (auto const& m : _m)
            if (m->var) return true;
        return false;
    }
    bool any_record_method() const {
        for (auto const& m : _m)
            if (m->rec) return true;
        return false;
    }
    /// An ordered route that serves string methods: one batch in flight, the
    /// replies sized on the device (set_ordered_var, set_ordered_legs).
    bool strings_route() const { return _ordered_var || _ordered_legs; }
    static constexpr uint64_t kRecordFillMax = 256;  // struct bytes srpc_gpu_unpack_aos_fill takes

    // ---- the buffers: owned in groups, built by ensure(), dropped by release() ----

    /// A staging slot: the pinned halves of a batch in flight, and its last copy's event.
    struct slot {
        pinned_buffer<uint8_t> h_in, h_out, h_cls;
        pinned_buffer<uint32_t> h_offs;
        // per method: its unpack status [k], its pack status [K + k] (each
        // call resets its own, so methods never clear each other's)
        pinned_buffer<srpc_unpack_status> h_status;
        hipEvent_t done = nullptr;  // the batch's last copy
        slot() = default;
        slot(slot const&) = delete;
        slot& operator=(slot const&) = delete;
        ~slot() { reset(); }
        void reset() {
            h_in.reset(), h_out.reset(), h_cls.reset(), h_offs.reset(), h_status.reset();
            if (done) (void)hipEventDestroy(done);
            done = nullptr;
        }
    };
    struct batch_buffers {  // every route
        device_buffer<uint8_t> d_in, d_cls, d_out;
        device_buffer<uint32_t> d_offs;
        device_buffer<uint64_t> d_counts;
        device_buffer<srpc_unpack_status> d_status;
        pinned_buffer<uint64_t> h_counts;
    };
    struct bucket_buffers {
        device_buffer<uint32_t> d_index;
        device_buffer<uint64_t> d_out_off;
        device_buffer<uint8_t> d_gather, d_resp;
        device_buffer<void> d_scratch;
        // with a string method registered (either route that serves them)
        device_buffer<uint64_t> d_var_rec;  // the request index of the bucket being served
        device_buffer<void> d_var_scratch;
        pinned_buffer<uint64_t> h_out_off;
    };
    struct ordered_buffers {  // the call index and the ranks stand in for the buckets
        device_buffer<void> d_mix_index;
        device_buffer<uint32_t> d_rank;
    };
    struct ordered_records_buffers {
        device_buffer<void> d_scratch;  // the decode's tables and fills
    };
    struct ordered_var_buffers {
        device_buffer<void> d_scratch;
        device_buffer<uint64_t> d_ends, d_total;
        device_buffer<uint32_t> d_offs;
        pinned_buffer<uint64_t> h_ends, h_total;
        pinned_buffer<uint32_t> h_offs;
    };

    /// Method m's device buffers for batches of _max frames in _cap bytes, and
    /// the pointer tables over them.
    void alloc_method(method_entry& m) {
        if (m.rec) {
            m.d_reqs.alloc(_max * m.req_stride + 16);
            m.d_resps.alloc(_max * m.resp_stride + 16);
            check(hipMemset(m.d_resps, 0, _max * m.resp_stride + 16));
            if (m.req_stride > kRecordFillMax) {  // past the fill call's limit: every struct a Req{} once, leaves per batch
                std::vector<uint8_t> all(_max * m.req_stride);
                for (uint64_t i = 0; i < _max; ++i) std::memcpy(all.data() + i * m.req_stride, m.req_fill.data(), m.req_stride);
                check(hipMemcpy(m.d_reqs, all.data(), all.size(), hipMemcpyHostToDevice));
            } else {  // the ordered warm-up's handlers run on element 0 before any decode wrote it
                check(hipMemset(m.d_reqs, 0, _max * m.req_stride + 16));
            }
            return;
        }
        auto side = [&](std::vector<bool> const& str, std::vector<uint64_t> const& size, uint64_t str_bytes,
                        std::vector<device_buffer<uint8_t>>& buf, std::vector<device_buffer<uint64_t>>& off_buf,
                        std::vector<uint64_t>& bytes, std::vector<void*>& cols, std::vector<uint64_t*>& offs) {
            buf.clear(), off_buf.clear(), bytes.clear(), cols.clear(), offs.clear();
            buf.resize(str.size()), off_buf.resize(str.size());
            for (size_t f = 0; f < str.size(); ++f) {
                bytes.push_back(str[f] ? str_bytes : _max * size[f] + 16);
                buf[f].alloc(bytes[f]);
                if (str[f]) off_buf[f].alloc(8 * (_max + 1) + 16);
                cols.push_back(buf[f]);
                offs.push_back(off_buf[f]);
            }
        };
        side(m.req_string, m.req_size, _cap + 16, m.req_buf, m.req_off_buf, m.req_bytes, m.req_cols, m.req_offs);
        side(m.resp_string, m.resp_size, _max * m.lim.max_response_chars + 16, m.resp_buf, m.resp_off_buf, m.resp_bytes,
             m.resp_cols, m.resp_offs);
        m.c_resp_cols.assign(m.resp_cols.begin(), m.resp_cols.end());
        m.c_req_offs.assign(m.req_offs.begin(), m.req_offs.end());
        m.c_resp_offs.assign(m.resp_offs.begin(), m.resp_offs.end());
        m.req_scap.clear();
        for (uint64_t b : m.req_bytes) m.req_scap.push_back(b - 16);  // a string column: the receive buffer's bytes
        if (!m.var) return;
        m.resp_wire_cap = _max * m.min_out + 16;
        for (size_t f = 0; f < m.resp_string.size(); ++f)
            if (m.resp_string[f]) m.resp_wire_cap += m.resp_bytes[f];
        m.h_ends.alloc(16 * m.resp_string.size() + 16);
        if (strings_route()) return;  // the replies are packed straight into the reply stream
        m.resp_wire.alloc(m.resp_wire_cap);
        m.resp_rec.alloc(8 * (_max + 1) + 16);
        uint64_t a = 0, b = 0;
        check_srpc(srpc_plan_var_scratch_bytes(m.in->get(), _max, _cap, &a), "srpc_plan_var_scratch_bytes");
        check_srpc(srpc_plan_var_scratch_bytes(m.out->get(), _max, m.resp_wire_cap, &b), "srpc_plan_var_scratch_bytes");
        _var_scratch_bytes = std::max({_var_scratch_bytes, a, b});
    }

    void ensure() {
        if (_slots[0].h_in) return;
        const uint64_t K = _m.size();
        _cap = _max * max_fin();
        if (_cap > 0xffffffffull) throw plan_error("batch_server: batch buffer over 4 GiB", SRPC_E_UNSUPPORTED);
        _var_methods = any_var_method();
        _var_scratch_bytes = 0;
        for (auto& m : _m) alloc_method(*m);
        if (_var_scratch_bytes) _bk.d_var_scratch.alloc(_var_scratch_bytes);
        if (_var_methods) {
            _bk.d_var_rec.alloc(8 * (_max + 1) + 16);
            _bk.h_out_off.alloc(8 * (_max + 1) + 16);
        }
        const uint64_t out_cap = this->out_cap();
        // two staging slots (two batches in flight) unless a string method's
        // batches need the host between their kernels (SRPC_SERVER_SLOTS=1:
        // one batch at a time, the A/B baseline)
        const char* slots_env = std::getenv("SRPC_SERVER_SLOTS");
        _nslots = _var_methods || strings_route() || (slots_env && slots_env[0] == '1') ? 1 : 2;
        for (int i = 0; i < _nslots; ++i) {
            slot& z = _slots[i];
            z.h_in.alloc(_cap + 16);
            z.h_offs.alloc(4 * _max + 16);
            z.h_out.alloc(out_cap + 16);
            z.h_cls.alloc(_max + 16);
            z.h_status.alloc(2 * K * sizeof(srpc_unpack_status));
            check(hipEventCreateWithFlags(&z.done, hipEventDisableTiming));
        }
        _b.h_counts.alloc(8 * (K + 2) + 16);
        _b.d_in.alloc(_cap + 16);
        _b.d_offs.alloc(4 * _max + 16);
        _b.d_cls.alloc(_max + 16);
        _b.d_counts.alloc(8 * (K + 2) + 16);
        _b.d_out.alloc(out_cap + 16);
        _b.d_status.alloc(2 * K * sizeof(srpc_unpack_status));
        build_tables();
        if (_ordered) {
            // no bucket index, no gather buffer, no second response buffer
            check_srpc(srpc_frames_mixed_index_bytes(_max, static_cast<int>(K), &_mix_index_bytes),
                       "srpc_frames_mixed_index_bytes");
            _od.d_mix_index.alloc(_mix_index_bytes + 16);
            _od.d_rank.alloc(4 * _max + 16);
            if (_ordered_rec) {
                check_srpc(srpc_frames_mixed_aos_scratch_bytes(_ord_in_plans.data(), static_cast<int>(K),
                                                               _or_req_stride.data(), &_or_scratch_bytes),
                           "srpc_frames_mixed_aos_scratch_bytes");
                _or.d_scratch.alloc(_or_scratch_bytes + 16);
            }
            if (strings_route()) {
                if (out_cap > 0xffffffffull) throw plan_error("batch_server: reply buffer over 4 GiB", SRPC_E_UNSUPPORTED);
                uint64_t a = 0, b = 0;
                if (_ordered_legs) {  // the same layout, then the record methods' tables and fills
                    check_srpc(srpc_frames_mixed_legs_scratch_bytes(_ord_in_plans.data(), static_cast<int>(K),
                                                                    _or_req_stride.data(), _max, &a),
                               "srpc_frames_mixed_legs_scratch_bytes");
                    check_srpc(srpc_frames_mixed_legs_scratch_bytes(_ord_out_plans.data(), static_cast<int>(K),
                                                                    _or_resp_stride.data(), _max, &b),
                               "srpc_frames_mixed_legs_scratch_bytes");
                } else {
                    check_srpc(srpc_frames_mixed_var_scratch_bytes(_ord_in_plans.data(), static_cast<int>(K), _max, &a),
                               "srpc_frames_mixed_var_scratch_bytes");
                    check_srpc(srpc_frames_mixed_var_scratch_bytes(_ord_out_plans.data(), static_cast<int>(K), _max, &b),
                               "srpc_frames_mixed_var_scratch_bytes");
                }
                _ov_scratch_bytes = std::max(a, b);
                _ov.d_scratch.alloc(_ov_scratch_bytes + 16);
                _ov.d_ends.alloc(8 * (_ov_slots + 1) + 16);
                _ov.d_total.alloc(16);
                _ov.d_offs.alloc(4 * (_max + 1) + 16);
                _ov.h_ends.alloc(8 * (_ov_slots + 1) + 16);
                _ov.h_total.alloc(16);
                _ov.h_offs.alloc(4 * (_max + 1) + 16);
            }
        } else {
            _bk.d_index.alloc(4 * K * _max + 16);
            _bk.d_out_off.alloc(8 * (_max + 1) + 16);
            _bk.d_gather.alloc(_cap + 16);
            _bk.d_resp.alloc(out_cap + 16);
            check_srpc(srpc_frames_scratch_bytes(_max, static_cast<int>(K), &_scratch_bytes),
                       "srpc_frames_scratch_bytes");
            _bk.d_scratch.alloc(_scratch_bytes);
        }
        warm_up();
    }

    /// The per-method tables every route's calls take, over the methods' own
    /// (alloc_method).  The ordered routes' plans, per method and per side: a
    /// side with strings keeps the unframed-prefix string plan, a side without
    /// gets a fixed-size plan behind the framed prefix (register_method's own,
    /// or one built here for a string method's fixed side).
    void build_tables() {
        _in_plans.clear(), _ord_in_plans.clear(), _ord_out_plans.clear(), _resp_bytes.clear(), _var_rec.clear();
        _req_tbl.clear(), _resp_tbl.clear(), _resp_mut_tbl.clear();
        _ov_req_offs.clear(), _ov_c_req_offs.clear(), _ov_resp_offs.clear(), _ov_c_resp_offs.clear();
        _ov_req_scap.clear(), _ov_resp_cap.clear();
        _or_req_recs.clear(), _or_c_req_recs.clear(), _or_resp_recs.clear(), _or_c_resp_recs.clear();
        _or_req_stride.clear(), _or_resp_stride.clear(), _or_req_loffs.clear(), _or_resp_loffs.clear(), _or_fill.clear();
        _caps.assign(_m.size(), _max);
        _ov_slots = 0;
        for (auto& m : _m) {
            if (strings_route() && m->var && !m->in_str()) m->ord_in = std::make_unique<raw_plan>(m->in_kinds, m->framed_in, _dev);
            if (strings_route() && m->var && !m->out_str())
                m->ord_out = std::make_unique<raw_plan>(m->out_kinds, m->framed_out, _dev);
            _in_plans.push_back(m->in->get());
            _ord_in_plans.push_back(m->ord_in ? m->ord_in->get() : m->in->get());
            _ord_out_plans.push_back(m->ord_out ? m->ord_out->get() : m->out->get());
            _resp_bytes.push_back(static_cast<uint32_t>(m->fout));
            _var_rec.push_back(m->resp_rec);
            // a column method's columns and offsets arrays (null for a record method)
            _req_tbl.push_back(m->rec ? nullptr : m->req_cols.data());
            _resp_mut_tbl.push_back(m->rec ? nullptr : m->resp_cols.data());
            _resp_tbl.push_back(m->rec ? nullptr : m->c_resp_cols.data());
            _ov_req_offs.push_back(m->rec ? nullptr : m->req_offs.data());
            _ov_c_req_offs.push_back(m->rec ? nullptr : m->c_req_offs.data());
            _ov_resp_offs.push_back(m->rec ? nullptr : m->resp_offs.data());
            _ov_c_resp_offs.push_back(m->rec ? nullptr : m->c_resp_offs.data());
            _ov_req_scap.push_back(m->rec ? nullptr : m->req_scap.data());
            _ov_resp_cap.push_back(m->rec ? nullptr : m->resp_bytes.data());
            for (uint64_t* o : m->req_offs) _ov_slots += o ? 1 : 0;
            // a record method's struct arrays (null and zero for the others)
            _or_req_recs.push_back(m->d_reqs);
            _or_c_req_recs.push_back(m->d_reqs);
            _or_resp_recs.push_back(m->d_resps);
            _or_c_resp_recs.push_back(m->d_resps);
            _or_req_stride.push_back(m->req_stride);
            _or_resp_stride.push_back(m->resp_stride);
            _or_req_loffs.push_back(m->req_loffs.data());
            _or_resp_loffs.push_back(m->resp_loffs.data());
            _or_fill.push_back(m->req_fill.data());
        }
    }

    void release() {
        for (auto& m : _m) m->release();
        for (slot& z : _slots) z.reset();
        _nslots = 0;
        _b = {}, _bk = {}, _od = {}, _or = {}, _ov = {};
    }

    // ---- the steps of a batch, shared by the batches and the warm-up ----

    /// A batch between process_begin and process_end: the skeleton fills the
    /// first line, the route's steps the rest.
    struct pending {
        bool valid = false;
        int slot = 0;
        uint64_t nf = 0, used = 0;
        double gpu_s = 0;  // host time spent on the batch's GPU work (enqueue, syncs, the final wait)
        uint64_t unknown = 0, total = 0;  // frames for the CPU; bytes of the GPU's replies
        bool mixed = false;
        bool cls_on_host = false;  // the route already fetched the class bytes
        // where frame i's answer ends: [i + 1] of the route's offsets, or (neither) after its fixed frame
        const uint64_t* ends64 = nullptr;
        const uint32_t* ends32 = nullptr;
        uint64_t d2h_extra = 0;  // d2h_bytes beyond the replies: the class bytes and offsets the route fetched
    };
    /// The batch being enqueued, for the trace (SRPC_SERVER_TRACE) and its timers.
    struct trace_point {
        bool on = false;
        uint64_t batch = 0, nf = 0;
        clock::time_point t0;
    };
    void mark(const char* what) const {
        if (_tp.on)
            std::fprintf(stderr, "batch %llu nf %llu %-10s %.3f ms\n", (unsigned long long)_tp.batch,
                         (unsigned long long)_tp.nf, what, 1e3 * secs(_tp.t0));
    }
    void clear_status() {
        check(hipMemsetAsync(_b.d_status, 0, 2 * _m.size() * sizeof(srpc_unpack_status), _s));
    }

    /// A string method's handler over n requests in its columns.
    int run_var_handler(method_entry& m, uint64_t n) {
        var_batch b;
        b.n = n;
        b.req_cols = m.req_cols.data();
        b.req_str_offs = m.c_req_offs.data();
        b.resp_cols = m.resp_cols.data();
        b.resp_str_offs = m.resp_offs.data();
        b.resp_cap = m.resp_bytes.data();
        return m.vhandler(b, _s);
    }
    /// The first and last offsets of every response string field of m's n
    /// responses to m.h_ends (checked against the columns' sizes before
    /// anything reads the chars: demote_overflowing).
    void copy_response_ends(method_entry& m, uint64_t n) {
        for (size_t f = 0; f < m.resp_offs.size(); ++f) {
            if (!m.resp_offs[f]) continue;
            check(hipMemcpyAsync(m.h_ends + 2 * f, m.resp_offs[f], 8, hipMemcpyDeviceToHost, _s));
            check(hipMemcpyAsync(m.h_ends + 2 * f + 1, m.resp_offs[f] + n, 8, hipMemcpyDeviceToHost, _s));
        }
    }
    /// The handler's response strings of method k fit its columns: offs[0] <=
    /// offs[n] <= the column's bytes (m.h_ends, after a sync).  The handler
    /// contract (var_batch) asks for non-decreasing offsets within the column.
    bool var_responses_fit(method_entry const& m) const {
        for (size_t f = 0; f < m.resp_offs.size(); ++f) {
            if (!m.resp_offs[f]) continue;
            const uint64_t a = m.h_ends[2 * f], e = m.h_ends[2 * f + 1];
            if (a > e || e > m.resp_bytes[f]) return false;
        }
        return true;
    }
    /// Overflow demotion, after the string methods' handlers and
    /// copy_response_ends: the sync the ends need; every string method whose
    /// responses do not fit their columns (max_response_chars) is answered on the
    /// CPU server for this batch, in place -- its frames become unknown in
    /// z.h_cls (fetched first unless cls_on_host) and d_cls, its count moves to
    /// `unknown`.  True when a method was demoted: the caller then brings what
    /// else its route keeps on the device in line with the new classes.
    bool demote_overflowing(slot& z, uint64_t nf, bool cls_on_host, uint64_t& unknown, batch_stats& st) {
        const size_t K = _m.size();
        check(hipStreamSynchronize(_s));  // the responses' sizes
        bool demoted[SRPC_FRAMES_MAX_PLANS] = {};
        bool any = false;
        for (size_t k = 0; k < K; ++k) {
            if (!_m[k]->var || !_b.h_counts[k] || var_responses_fit(*_m[k])) continue;
            demoted[k] = any = true;
            st.overflow_batches += 1;
        }
        if (!any) return false;
        if (!cls_on_host) {
            check(hipMemcpyAsync(z.h_cls, _b.d_cls, nf, hipMemcpyDeviceToHost, _s));
            check(hipStreamSynchronize(_s));
        }
        for (uint64_t i = 0; i < nf; ++i)
            if (z.h_cls[i] != SRPC_FRAME_UNKNOWN && demoted[z.h_cls[i]]) z.h_cls[i] = SRPC_FRAME_UNKNOWN;
        for (size_t k = 0; k < K; ++k)
            if (demoted[k]) {
                unknown += _b.h_counts[k];
                _b.h_counts[k] = 0;
            }
        check(hipMemcpyAsync(_b.d_cls, z.h_cls, nf, hipMemcpyHostToDevice, _s));
        return true;
    }

    // -- the bucket route --

    void classify(uint64_t nf, uint64_t used) {
        const int K = static_cast<int>(_m.size());
        check_srpc(srpc_frames_classify(_in_plans.data(), _resp_bytes.data(), K, _b.d_in, used, _b.d_offs, nf, _b.d_cls,
                                        _bk.d_index, _b.d_counts, _bk.d_out_off, _bk.d_scratch, _scratch_bytes, _s),
                   "srpc_frames_classify");
        check(hipMemcpyAsync(_b.h_counts, _b.d_counts, 8 * (K + 2), hipMemcpyDeviceToHost, _s));
    }
    /// A record method's three steps on n contiguous request frames at src:
    /// decode into its Req array (status slot st), handler, framed responses from
    /// its Resp array to dst.  Returns the decode's status (positive for the
    /// warm-up's zero frame); the handler and the pack throw.
    int run_record_method(method_entry& m, const uint8_t* src, uint64_t n, srpc_unpack_status* st, uint8_t* dst,
                          const char* what) {
        const int rc = m.req_stride <= kRecordFillMax
                           ? srpc_gpu_unpack_aos_fill(m.in->get(), src, n * m.fin, n, m.d_reqs, m.req_stride,
                                                      m.req_loffs.data(), m.req_fill.data(), st, _s)
                           : srpc_gpu_unpack_aos(m.in->get(), src, n * m.fin, n, m.d_reqs, m.req_stride,
                                                 m.req_loffs.data(), st, _s);
        if (rc < 0) return rc;
        check_srpc(m.rhandler(m.d_reqs, m.d_resps, n, _s), what);
        check_srpc(srpc_gpu_pack_aos(m.out->get(), m.d_resps, m.resp_stride, m.resp_loffs.data(), n, dst, n * m.fout, _s),
                   "srpc_gpu_pack_aos");
        return rc;
    }
    /// Fixed-size method k on n contiguous request frames at src: decode,
    /// handler, framed responses to dst.  (A decode status is positive on the
    /// warm-up's zero frame: expected, and never sent.)
    void run_fixed_method(method_entry& m, size_t k, const uint8_t* src, uint64_t n, uint8_t* dst, const char* what) {
        if (m.rec) {
            check_srpc(run_record_method(m, src, n, _b.d_status + k, dst, what), "srpc_gpu_unpack_aos");
            mark("record method");
            return;
        }
        check_srpc(srpc_gpu_unpack(m.in->get(), src, n * m.fin, n, m.req_cols.data(), _b.d_status + k, _s),
                   "srpc_gpu_unpack");
        mark("unpack");
        check_srpc(m.handler(m.req_cols.data(), m.resp_cols.data(), n, _s), what);
        mark("handler");
        check_srpc(srpc_gpu_pack(m.out->get(), m.resp_cols.data(), n, dst, n * m.fout, _s), "srpc_gpu_pack");
        mark("pack");
    }
    /// unpack_var -> handler over n gathered requests (d_gather, index
    /// d_var_rec, at most wire_len bytes) of string method k, then its
    /// responses' ends to the host.
    void run_var_unpack(method_entry& m, size_t k, uint64_t n, uint64_t wire_len) {
        check_srpc(srpc_gpu_unpack_var(m.in->get(), _bk.d_gather, wire_len, n, _bk.d_var_rec, m.req_cols.data(),
                                       m.req_offs.data(), _b.d_status + k, _bk.d_var_scratch, _var_scratch_bytes, _s),
                   "srpc_gpu_unpack_var");
        check_srpc(run_var_handler(m, n), "batch handler");
        copy_response_ends(m, n);
    }
    void run_var_pack(method_entry& m, size_t k, uint64_t n) {
        check_srpc(srpc_gpu_pack_var(m.out->get(), m.c_resp_cols.data(), m.c_resp_offs.data(), n, m.resp_wire,
                                     m.resp_wire_cap, m.resp_rec, _b.d_status + _m.size() + k, _bk.d_var_scratch,
                                     _var_scratch_bytes, _s),
                   "srpc_gpu_pack_var");
    }

    /// The bucket route's steps between the H2D and the D2H: classify and the
    /// first sync, the string methods (their responses' sizes place every
    /// answer: a second sync, the demotion, the offsets, a third for the reply
    /// stream's size), then every fixed-size method's bucket.
    void bucket_steps(slot& z, uint64_t nf, uint64_t used, batch_stats& st, pending& pd) {
        const size_t K = _m.size();
        classify(nf, used);
        if (_var_methods) check(hipMemcpyAsync(z.h_cls, _b.d_cls, nf, hipMemcpyDeviceToHost, _s));
        mark("classify");
        check(hipStreamSynchronize(_s));
        mark("sync1");
        st.classify_seconds += secs(_tp.t0);
        uint64_t* counts = _b.h_counts;
        uint64_t unknown = counts[K + 1];
        bool mixed = false, any_var = false;
        for (size_t k = 0; k < K; ++k) any_var |= _m[k]->var && counts[k] > 0;
        uint64_t var_bytes[SRPC_FRAMES_MAX_PLANS] = {};  // payload bytes of each string method's frames
        if (any_var)
            for (uint64_t i = 0; i < nf; ++i) {
                const uint8_t c = z.h_cls[i];
                if (c != SRPC_FRAME_UNKNOWN && _m[c]->var)
                    var_bytes[c] += (i + 1 < nf ? z.h_offs[i + 1] : used) - z.h_offs[i] - 4;
            }
        clear_status();
        if (any_var) {
            for (size_t k = 0; k < K; ++k) {
                method_entry& m = *_m[k];
                const uint64_t n = counts[k];
                if (!m.var || !n) continue;
                mixed |= n != nf;
                check_srpc(srpc_frames_gather_var(_b.d_in, _b.d_offs, _bk.d_index + k * nf, n, _bk.d_gather, _bk.d_var_rec,
                                                  _bk.d_scratch, _scratch_bytes, _s),
                           "srpc_frames_gather_var");
                run_var_unpack(m, k, n, var_bytes[k]);
                mark("var unpack");
            }
            if (demote_overflowing(z, nf, true, unknown, st)) {
                check(hipMemcpyAsync(_b.d_counts, counts, 8 * K, hipMemcpyHostToDevice, _s));
                // the copies read pinned memory the next batch rewrites
                check(hipStreamSynchronize(_s));
            }
            for (size_t k = 0; k < K; ++k)
                if (_m[k]->var && counts[k]) run_var_pack(*_m[k], k, counts[k]);
            mark("var pack");
            check_srpc(srpc_frames_offsets(_in_plans.data(), _resp_bytes.data(), static_cast<int>(K), _b.d_cls, nf,
                                           _bk.d_index, _b.d_counts, _var_rec.data(), _bk.d_out_off, _b.d_counts + K,
                                           _bk.d_scratch, _scratch_bytes, _s),
                       "srpc_frames_offsets");
            check(hipMemcpyAsync(counts + K, _b.d_counts + K, 8, hipMemcpyDeviceToHost, _s));
        }
        for (size_t k = 0; k < K; ++k) {
            const uint64_t n = counts[k];
            method_entry& m = *_m[k];
            if (!n || m.var) continue;
            const bool whole = n == nf;  // every frame is method k: they already are its contiguous records
            mixed |= !whole;
            const uint8_t* src = _b.d_in;
            if (!whole) {
                check_srpc(srpc_frames_gather(_b.d_in, _b.d_offs, _bk.d_index + k * nf, n, static_cast<uint32_t>(m.fin),
                                              _bk.d_gather, _s),
                           "srpc_frames_gather");
                src = _bk.d_gather;
            }
            uint8_t* dst = whole ? _b.d_out : _bk.d_resp;
            run_fixed_method(m, k, src, n, dst, "batch handler");
            if (!whole)
                check_srpc(srpc_frames_scatter(dst, _bk.d_index + k * nf, n, static_cast<uint32_t>(m.fout), _bk.d_out_off,
                                               _b.d_out, _s),
                           "srpc_frames_scatter");
        }
        if (any_var) {
            for (size_t k = 0; k < K; ++k)
                if (_m[k]->var && counts[k])
                    check_srpc(srpc_frames_scatter_var(_m[k]->resp_wire, _m[k]->resp_rec, _bk.d_index + k * nf, counts[k],
                                                       _bk.d_out_off, _b.d_out, _s),
                               "srpc_frames_scatter_var");
            if (unknown) check(hipMemcpyAsync(_bk.h_out_off, _bk.d_out_off, 8 * (nf + 1), hipMemcpyDeviceToHost, _s));
            check(hipStreamSynchronize(_s));  // the reply stream's size
            mark("sync_var");
            pd.ends64 = _bk.h_out_off;
        }
        pd.unknown = unknown;
        pd.total = counts[K];
        pd.mixed = mixed;
        pd.cls_on_host = _var_methods;
        pd.d2h_extra = (unknown || _var_methods ? nf : 0) + (unknown && any_var ? 8 * (nf + 1) : 0);
    }
    /// One string-method batch on one well-formed request with empty strings
    /// (its prefix, zeros): every kernel of the var path and the handler load
    /// their code objects here, not on the first batch.
    void warm_up_var(method_entry& m, size_t k) {
        std::vector<uint8_t> f = m.framed_in;
        f.resize(4 + m.min_in, 0);
        check(hipMemcpyAsync(_b.d_in, f.data(), f.size(), hipMemcpyHostToDevice, _s));
        check(hipMemsetAsync(_bk.d_index, 0, 4, _s));
        check(hipMemsetAsync(_b.d_offs, 0, 4, _s));
        check_srpc(srpc_frames_gather_var(_b.d_in, _b.d_offs, _bk.d_index, 1, _bk.d_gather, _bk.d_var_rec, _bk.d_scratch,
                                          _scratch_bytes, _s),
                   "srpc_frames_gather_var");
        run_var_unpack(m, k, 1, m.min_in);
        run_var_pack(m, k, 1);
        check_srpc(srpc_frames_scatter_var(m.resp_wire, m.resp_rec, _bk.d_index, 1, _bk.d_out_off, _b.d_out, _s),
                   "srpc_frames_scatter_var");
    }
    /// The bucket route's steps on the warm-up's one all-zero frame: every
    /// method's bucket as if the frame were its own, through both destinations.
    void bucket_warm_up_steps() {
        classify(1, 8);
        check(hipStreamSynchronize(_s));
        clear_status();
        for (size_t k = 0; k < _m.size(); ++k) {
            method_entry& m = *_m[k];
            if (m.var) {
                warm_up_var(m, k);
                continue;
            }
            check_srpc(srpc_frames_gather(_b.d_in, _b.d_offs, _bk.d_index, 1, static_cast<uint32_t>(m.fin), _bk.d_gather, _s),
                       "srpc_frames_gather");
            // the handler's own kernels load their code object on first use
            // too: it runs on the one zero record (its output is never sent)
            run_fixed_method(m, k, _bk.d_gather, 1, _b.d_out, "batch handler (warm-up)");
            if (m.rec)  // the same on its struct arrays, into the other destination
                run_fixed_method(m, k, _bk.d_gather, 1, _bk.d_resp, "batch handler (warm-up)");
            else
                check_srpc(srpc_gpu_pack(m.out->get(), m.resp_cols.data(), 1, _bk.d_resp, m.fout, _s), "srpc_gpu_pack");
            check_srpc(srpc_frames_scatter(_bk.d_resp, _bk.d_index, 1, static_cast<uint32_t>(m.fout), _bk.d_out_off,
                                           _b.d_out, _s),
                       "srpc_frames_scatter");
        }
    }

    // -- the ordered routes (set_ordered, set_ordered_var, set_ordered_records, set_ordered_legs): one decode, the handlers, one pack --

    bool whole_batch_handler() const {
        return _ordered_legs ? bool(_olhandler)
               : _ordered_var ? bool(_ovhandler)
               : _ordered_rec ? bool(_orhandler)
                              : bool(_ohandler);
    }

    /// The decode half of a batch: one srpc_frames_unpack_requests_mixed[_var|_aos|_legs]
    /// over the nf frames in d_in[0, used) into the methods' request columns
    /// (chars and offsets too) or Req arrays, the ranks when the ordered handler is set, then
    /// the counts (and the string slots' ends) on the host after one sync.
    void ordered_decode(uint64_t nf, uint64_t used) {
        const int K = static_cast<int>(_m.size());
        clear_status();
        if (_ordered_legs)
            check_srpc(srpc_frames_unpack_requests_mixed_legs(
                           _ord_in_plans.data(), K, _b.d_in, used, _b.d_offs, nf, _req_tbl.data(), _ov_req_offs.data(),
                           _ov_req_scap.data(), _or_req_recs.data(), _or_req_stride.data(), _or_req_loffs.data(),
                           _or_fill.data(), nullptr, _caps.data(), _b.d_cls, _od.d_mix_index, _mix_index_bytes,
                           _b.d_counts, _ov.d_ends, _b.d_status, _ov.d_scratch, _ov_scratch_bytes, _s),
                       "srpc_frames_unpack_requests_mixed_legs");
        else if (_ordered_var)
            check_srpc(srpc_frames_unpack_requests_mixed_var(
                           _ord_in_plans.data(), K, _b.d_in, used, _b.d_offs, nf, _req_tbl.data(), _ov_req_offs.data(),
                           _ov_req_scap.data(), nullptr, _caps.data(), _b.d_cls, _od.d_mix_index, _mix_index_bytes,
                           _b.d_counts, _ov.d_ends, _b.d_status, _ov.d_scratch, _ov_scratch_bytes, _s),
                       "srpc_frames_unpack_requests_mixed_var");
        else if (_ordered_rec)
            check_srpc(srpc_frames_unpack_requests_mixed_aos(
                           _ord_in_plans.data(), K, _b.d_in, used, _b.d_offs, nf, _or_req_recs.data(), _or_req_stride.data(),
                           _or_req_loffs.data(), _or_fill.data(), nullptr, _caps.data(), _b.d_cls, _od.d_mix_index,
                           _mix_index_bytes, _b.d_counts, _b.d_status, _or.d_scratch, _or_scratch_bytes, _s),
                       "srpc_frames_unpack_requests_mixed_aos");
        else
            check_srpc(srpc_frames_unpack_requests_mixed(_ord_in_plans.data(), K, _b.d_in, used, _b.d_offs, nf,
                                                         _req_tbl.data(), nullptr, _caps.data(), _b.d_cls,
                                                         _od.d_mix_index, _mix_index_bytes, _b.d_counts, _b.d_status, _s),
                       "srpc_frames_unpack_requests_mixed");
        if (whole_batch_handler())
            check_srpc(srpc_frames_mixed_ranks(_od.d_mix_index, _b.d_cls, nf, K, _od.d_rank, _s), "srpc_frames_mixed_ranks");
        check(hipMemcpyAsync(_b.h_counts, _b.d_counts, 8 * (static_cast<uint64_t>(K) + 1), hipMemcpyDeviceToHost, _s));
        if (strings_route() && _ov_slots)
            check(hipMemcpyAsync(_ov.h_ends, _ov.d_ends, 8 * _ov_slots, hipMemcpyDeviceToHost, _s));
        check(hipStreamSynchronize(_s));
    }
    /// The ordered handler over the batch of nf frames, or every method's
    /// handler over its requests in arrival order (warm: over one zero record).
    void ordered_handlers(uint64_t nf, bool warm) {
        if (whole_batch_handler()) {
            const char* what = warm ? "ordered batch handler (warm-up)" : "ordered batch handler";
            if (_ordered_rec) {
                ordered_records_batch b;
                b.n = nf;
                b.d_method = _b.d_cls;
                b.d_rank = _od.d_rank;
                b.counts = _b.h_counts;
                b.methods = _m.size();
                b.req_recs = _or_c_req_recs.data();
                b.resp_recs = _or_resp_recs.data();
                b.req_stride = _or_req_stride.data();
                b.resp_stride = _or_resp_stride.data();
                check_srpc(_orhandler(b, _s), what);
                return;
            }
            auto fill = [&](auto& b) {
                b.n = nf;
                b.d_method = _b.d_cls;
                b.d_rank = _od.d_rank;
                b.counts = _b.h_counts;
                b.methods = _m.size();
                b.req_cols = _req_tbl.data();
                b.resp_cols = _resp_mut_tbl.data();
            };
            auto fill_strings = [&](auto& b) {
                b.req_str_offs = _ov_c_req_offs.data();
                b.resp_str_offs = _ov_resp_offs.data();
                b.resp_cap = _ov_resp_cap.data();
            };
            if (_ordered_legs) {
                ordered_legs_batch b;
                fill(b);
                fill_strings(b);
                b.req_recs = _or_c_req_recs.data();
                b.resp_recs = _or_resp_recs.data();
                b.req_stride = _or_req_stride.data();
                b.resp_stride = _or_resp_stride.data();
                check_srpc(_olhandler(b, _s), what);
            } else if (_ordered_var) {
                ordered_var_batch b;
                fill(b);
                fill_strings(b);
                check_srpc(_ovhandler(b, _s), what);
            } else {
                ordered_batch b;
                fill(b);
                check_srpc(_ohandler(b, _s), what);
            }
            return;
        }
        for (size_t k = 0; k < _m.size(); ++k) {
            method_entry& m = *_m[k];
            const uint64_t n = warm ? 1 : _b.h_counts[k];
            if (!n) continue;
            check_srpc(m.var   ? run_var_handler(m, n)
                       : m.rec ? m.rhandler(m.d_reqs, m.d_resps, n, _s)
                               : m.handler(m.req_cols.data(), m.resp_cols.data(), n, _s),
                       warm ? "batch handler (warm-up)" : "batch handler");
        }
    }
    /// The reply half: the response plans' frames in arrival order straight
    /// into d_out (an unknown frame gets no bytes: the pack's "bad call",
    /// answered on the CPU in its place).  With string methods, the stream's
    /// size and, with unknown frames, every answer's offset go to the host.  No
    /// sync here.
    void ordered_pack(uint64_t nf, bool unknown) {
        const int K = static_cast<int>(_m.size());
        if (_ordered_rec) {  // the same from the Resp arrays
            check_srpc(srpc_frames_pack_requests_mixed_aos(_ord_out_plans.data(), K, _or_c_resp_recs.data(),
                                                           _or_resp_stride.data(), _or_resp_loffs.data(), nullptr,
                                                           _caps.data(), _b.d_cls, _od.d_mix_index, nf, _b.d_out, out_cap(),
                                                           nullptr, nullptr, _s),
                       "srpc_frames_pack_requests_mixed_aos (replies)");
            return;
        }
        if (!strings_route()) {  // (the flag a bad call would raise is not asked for)
            check_srpc(srpc_frames_pack_requests_mixed(_ord_out_plans.data(), K, _resp_tbl.data(), nullptr, _caps.data(),
                                                       _b.d_cls, _od.d_mix_index, nf, _b.d_out, out_cap(), nullptr, nullptr,
                                                       _s),
                       "srpc_frames_pack_requests_mixed (replies)");
            return;
        }
        // an unknown frame is the pack's "bad call" and would raise its flag: asked for only without one
        if (_ordered_legs)  // a record method's replies from its Resp array
            check_srpc(srpc_frames_pack_requests_mixed_legs(
                           _ord_out_plans.data(), K, _resp_tbl.data(), _ov_c_resp_offs.data(), _or_c_resp_recs.data(),
                           _or_resp_stride.data(), _or_resp_loffs.data(), nullptr, _caps.data(), _b.d_cls, _od.d_mix_index,
                           nf, _b.d_out, out_cap(), _ov.d_offs, _ov.d_total, unknown ? nullptr : _b.d_status + K,
                           _ov.d_scratch, _ov_scratch_bytes, _s),
                       "srpc_frames_pack_requests_mixed_legs (replies)");
        else
            check_srpc(srpc_frames_pack_requests_mixed_var(
                           _ord_out_plans.data(), K, _resp_tbl.data(), _ov_c_resp_offs.data(), nullptr, _caps.data(),
                           _b.d_cls, _od.d_mix_index, nf, _b.d_out, out_cap(), _ov.d_offs, _ov.d_total,
                           unknown ? nullptr : _b.d_status + K, _ov.d_scratch, _ov_scratch_bytes, _s),
                       "srpc_frames_pack_requests_mixed_var (replies)");
        check(hipMemcpyAsync(_ov.h_total, _ov.d_total, 8, hipMemcpyDeviceToHost, _s));
        if (unknown) check(hipMemcpyAsync(_ov.h_offs, _ov.d_offs, 4 * (nf + 1), hipMemcpyDeviceToHost, _s));
    }
    /// The ordered routes' steps between the H2D and the D2H.  The methods'
    /// columns and d_cls are shared by the two staging slots: everything that
    /// touches them is in stream order.  With string methods: the string
    /// responses' sizes checked against their columns (a second sync, only when
    /// a string response exists) before the pack, the total and a sync after.
    void ordered_steps(slot& z, uint64_t nf, uint64_t used, batch_stats& st, pending& pd) {
        const size_t K = _m.size();
        ordered_decode(nf, used);
        mark("decode");
        st.classify_seconds += secs(_tp.t0);
        uint64_t unknown = _b.h_counts[K], total = 0;
        bool mixed = false, sized = false;
        for (size_t k = 0; k < K; ++k) {
            const uint64_t n = _b.h_counts[k];
            total += n * _m[k]->fout;  // (the whole of it without string methods)
            mixed |= n && n != nf;
            sized |= n && _m[k]->var && _m[k]->out_str();
        }
        ordered_handlers(nf, false);
        mark("handler");
        if (!strings_route()) {
            if (total) ordered_pack(nf, false);
            mark("pack");
            pd.d2h_extra = unknown ? nf : 0;
        } else {
            if (sized) {
                for (size_t k = 0; k < K; ++k)
                    if (_m[k]->var && _b.h_counts[k]) copy_response_ends(*_m[k], _b.h_counts[k]);
                // its frames become unknown; the ranks are per method, so the other methods' elements stay
                pd.cls_on_host = demote_overflowing(z, nf, false, unknown, st);
                if (pd.cls_on_host)
                    check_srpc(srpc_frames_mixed_index(_b.d_cls, nf, static_cast<int>(K), _od.d_mix_index, _mix_index_bytes,
                                                       _b.d_counts, nullptr, _s),
                               "srpc_frames_mixed_index");
                mark("sizes");
            }
            ordered_pack(nf, unknown != 0);
            check(hipStreamSynchronize(_s));  // the reply stream's size
            total = _ov.h_total[0];
            if (total > out_cap()) throw plan_error("batch_server: the replies overran the reply buffer", SRPC_E_INVALID);
            mark("pack");
            pd.ends32 = _ov.h_offs;
            pd.d2h_extra = unknown ? nf + 4 * (nf + 1) : 0;
        }
        pd.unknown = unknown;
        pd.total = total;
        pd.mixed = mixed;
    }

    /// One-frame run of every kernel the batches use (the library's and each
    /// handler, on one all-zero record -- or the ordered handler on that batch
    /// of one unknown frame) and one copy through every staging buffer, at
    /// serve start: first uses cost milliseconds that otherwise land on the
    /// connection's first batch (profiles/r02_e2e_warmup.log).
    void warm_up() {
        slot& z = _slots[0];
        const uint64_t out_cap = this->out_cap();
        _tp.on = false;
        check(hipMemsetAsync(_b.d_out, 0, out_cap + 16, _s));
        check(hipMemsetAsync(_b.d_cls, 0, _max + 16, _s));
        if (_ordered) {
            check(hipMemsetAsync(_od.d_mix_index, 0, _mix_index_bytes + 16, _s));
            check(hipMemsetAsync(_od.d_rank, 0, 4 * _max + 16, _s));
            if (strings_route()) {
                check(hipMemsetAsync(_ov.d_scratch, 0, _ov_scratch_bytes, _s));
                check(hipMemsetAsync(_ov.d_offs, 0, 4 * (_max + 1) + 16, _s));
            }
        } else {
            check(hipMemsetAsync(_bk.d_resp, 0, out_cap + 16, _s));
            check(hipMemsetAsync(_bk.d_gather, 0, _cap + 16, _s));
            check(hipMemsetAsync(_bk.d_index, 0, 4 * _m.size() * _max + 16, _s));
            check(hipMemsetAsync(_bk.d_out_off, 0, 8 * (_max + 1) + 16, _s));
            check(hipMemsetAsync(_bk.d_scratch, 0, _scratch_bytes, _s));
            if (_bk.d_var_scratch) check(hipMemsetAsync(_bk.d_var_scratch, 0, _var_scratch_bytes, _s));
        }
        for (auto const& m : _m) {
            for (size_t f = 0; f < m->req_cols.size(); ++f) check(hipMemsetAsync(m->req_cols[f], 0, m->req_bytes[f], _s));
            for (size_t f = 0; f < m->resp_cols.size(); ++f) check(hipMemsetAsync(m->resp_cols[f], 0, m->resp_bytes[f], _s));
            for (auto const* offs : {&m->req_offs, &m->resp_offs})
                for (uint64_t* p : *offs)
                    if (p) check(hipMemsetAsync(p, 0, 8 * (_max + 1), _s));
        }
        std::memset(z.h_in, 0, _cap);
        std::memset(z.h_offs, 0, 4 * _max);
        // a batch's exact sequence of copies and launches on one all-zero frame
        // (nobody's), twice (the first pass pays the first uses; whole buffers move)
        for (int pass = 0; pass < 2; ++pass) {
            check(hipMemcpyAsync(_b.d_in, z.h_in, _cap, hipMemcpyHostToDevice, _s));
            check(hipMemcpyAsync(_b.d_offs, z.h_offs, 4 * _max, hipMemcpyHostToDevice, _s));
            if (_ordered) {
                ordered_decode(1, std::min<uint64_t>(8, _cap));
                ordered_handlers(1, true);
                ordered_pack(1, true);
            } else {
                bucket_warm_up_steps();
            }
            check(hipMemcpyAsync(z.h_out, _b.d_out, out_cap, hipMemcpyDeviceToHost, _s));
            check(hipMemcpyAsync(z.h_cls, _b.d_cls, _max, hipMemcpyDeviceToHost, _s));
            check(hipMemcpyAsync(z.h_status, _b.d_status, 2 * _m.size() * sizeof(srpc_unpack_status), hipMemcpyDeviceToHost,
                                 _s));
            check(hipStreamSynchronize(_s));
        }
    }

    // ---- the batch skeleton ----

    /// The GPU path for the nf whole frames in slot si's h_in[0, used): every
    /// copy and kernel enqueued (with the host syncs the batch's own decisions
    /// need: its counts, a string method's response sizes), the last copy
    /// marked by the slot's event.  process_end answers it.
    pending process_begin(int si, uint64_t nf, uint64_t used, batch_stats& st) {
        slot& z = _slots[si];
        _tp = {_trace, st.gpu_batches, nf, clock::now()};
        check(hipMemcpyAsync(_b.d_in, z.h_in, used, hipMemcpyHostToDevice, _s));
        check(hipMemcpyAsync(_b.d_offs, z.h_offs, 4 * nf, hipMemcpyHostToDevice, _s));
        mark("h2d");
        pending pd;
        if (_ordered) ordered_steps(z, nf, used, st, pd);
        else bucket_steps(z, nf, used, st, pd);
        if (pd.total) check(hipMemcpyAsync(z.h_out, _b.d_out, pd.total, hipMemcpyDeviceToHost, _s));
        if (!_ordered) mark("d2h_out");
        if (pd.unknown && !pd.cls_on_host) check(hipMemcpyAsync(z.h_cls, _b.d_cls, nf, hipMemcpyDeviceToHost, _s));
        check(hipMemcpyAsync(z.h_status, _b.d_status, 2 * _m.size() * sizeof(srpc_unpack_status), hipMemcpyDeviceToHost,
                             _s));
        mark("d2h");
        check(hipEventRecord(z.done, _s));
        pd.valid = true;
        pd.slot = si;
        pd.nf = nf;
        pd.used = used;
        pd.gpu_s = secs(_tp.t0);
        _tp.on = false;
        return pd;
    }

    /// Wait for a batch's last copy (its slot's buffers in use), check its
    /// statuses and send its answers: the GPU's in runs, the CPU's in their
    /// places.
    void process_end(int fd, pending const& pd, batch_stats& st) {
        slot& z = _slots[pd.slot];
        const size_t K = _m.size();
        const uint64_t nf = pd.nf, unknown = pd.unknown, total = pd.total;
        auto t0 = clock::now();
        check(hipEventSynchronize(z.done));
        if (_trace)
            std::fprintf(stderr, "batch %llu nf %llu wait       %.3f ms\n", (unsigned long long)st.gpu_batches,
                         (unsigned long long)nf, 1e3 * secs(t0));
        // classification already matched every prefix and length (and walked
        // string records to their frame's end), and string responses were
        // checked against their columns before packing: a status here means
        // the buckets and the plans disagree (an internal invariant)
        for (size_t k = 0; k < 2 * K; ++k)
            if (z.h_status[k].flags)
                throw plan_error(k < K ? "batch_server: classified frame failed to unpack"
                                       : "batch_server: string responses overran a sized wire",
                                 SRPC_E_INVALID);
        const double dt = pd.gpu_s + secs(t0);
        if (st.gpu_batches == 0 && st.fallback_requests == 0) st.first_batch_seconds = dt;
        st.gpu_seconds += dt;
        st.h2d_bytes += pd.used + 4 * nf;
        st.d2h_bytes += total + pd.d2h_extra;
        if (total) {
            st.gpu_batches += 1;
            st.mixed_batches += pd.mixed ? 1 : 0;
        }
        st.gpu_requests += nf - unknown;
        st.requests += nf - unknown;
        auto t1 = clock::now();
        if (!unknown) {
            transport::send_all(fd, z.h_out, total);
            st.send_seconds += secs(t1);
            return;
        }
        // GPU answers in runs, the CPU's in their places, one gathered send
        // (separate small sends would meet Nagle + delayed ACK on the socket)
        _arena.clear();
        _pieces.clear();
        uint64_t run = 0, pos = 0;
        for (uint64_t i = 0; i < nf; ++i) {
            const uint8_t c = z.h_cls[i];
            if (c != SRPC_FRAME_UNKNOWN) {
                // the end of frame i's answer
                run = pd.ends32 ? pd.ends32[i + 1] : pd.ends64 ? pd.ends64[i + 1] : run + _m[c]->fout;
                if (pd.ends32 && pd.ends32[i + 1] == pd.ends32[i])
                    throw plan_error("batch_server: a handler's response offsets decrease", SRPC_E_INVALID);
                continue;
            }
            if (run > pos) _pieces.push_back({true, pos, run - pos});
            pos = run;
            const uint64_t o = z.h_offs[i];
            const uint64_t a0 = _arena.size();
            answer_cpu(z.h_in + o + 4, be32_at(z.h_in + o), st);
            _pieces.push_back({false, a0, _arena.size() - a0});
        }
        if (run > pos) _pieces.push_back({true, pos, run - pos});
        send_pieces(fd, z.h_out);
        st.send_seconds += secs(t1);
    }

    struct piece {
        bool gpu;  // h_out or _arena
        uint64_t off, len;
    };

    /// sendmsg over the pieces, IOV_MAX at a time, resuming partial sends.
    void send_pieces(int fd, uint8_t* h_out) {
        if (_pieces.size() > 4096) {  // many short runs: one copy beats ~170 ns per iovec in the kernel
            _flat.resize(0);
            for (piece const& p : _pieces) {
                const uint8_t* b = (p.gpu ? h_out : _arena.data()) + p.off;
                _flat.insert(_flat.end(), b, b + p.len);
            }
            transport::send_all(fd, _flat.data(), _flat.size());
            return;
        }
        std::vector<iovec> iov;
        iov.reserve(_pieces.size());
        for (piece const& p : _pieces)
            iov.push_back({(p.gpu ? h_out : _arena.data()) + p.off, static_cast<size_t>(p.len)});
        size_t at = 0;
        while (at < iov.size()) {
            msghdr mh{};
            mh.msg_iov = iov.data() + at;
            mh.msg_iovlen = std::min<size_t>(iov.size() - at, 1024);
            ssize_t k = sendmsg(fd, &mh, MSG_NOSIGNAL);
            if (k < 0 && errno == EINTR) continue;
            if (k <= 0) return;  // the peer is gone; the recv side ends the connection
            auto left = static_cast<size_t>(k);
            while (at < iov.size() && left >= iov[at].iov_len) left -= iov[at++].iov_len;
            if (left) {
                iov[at].iov_base = static_cast<uint8_t*>(iov[at].iov_base) + left;
                iov[at].iov_len -= left;
            }
        }
    }

    /// A frame longer than the batch buffer: `have` bytes of it are at the
    /// start of h_in; read the rest and answer it on the CPU.  False at EOF.
    bool serve_oversize(int fd, const uint8_t* h_in, uint64_t have, batch_stats& st) {
        const uint64_t len = be32_at(h_in);
        std::vector<uint8_t> payload(len);
        std::memcpy(payload.data(), h_in + 4, have - 4);
        auto t0 = clock::now();
        const bool ok = transport::recv_all(fd, payload.data() + (have - 4), len - (have - 4));
        st.recv_seconds += secs(t0);
        if (!ok) return false;
        st.oversize_requests += 1;
        _arena.clear();
        answer_cpu(payload.data(), len, st);
        transport::send_all(fd, _arena.data(), _arena.size());
        return true;
    }

    /// One frame's payload through the scalar server (reference server.hpp:58-69);
    /// the framed answer (BE32 | response, as transport::send_data) goes to _arena.
    void answer_cpu(const uint8_t* payload, uint64_t len, batch_stats& st) {
        auto t0 = clock::now();
        packer::ptr r;
        if (_fallback) {
            packer::ptr p = std::make_shared<packer>(payload, len);
            std::string fn;
            (*p) >> fn;
            r = _fallback->call(fn, p);
        } else {
            r = std::make_shared<packer>();
            (*r) << static_cast<uint8_t>(RPC_ERR_FUNCTION_NOT_REGISTERED);
        }
        const std::vector<uint8_t> hdr = be32(static_cast<uint32_t>(r->size()));
        _arena.insert(_arena.end(), hdr.begin(), hdr.end());
        _arena.insert(_arena.end(), r->data(), r->data() + r->size());
        st.fallback_requests += 1;
        st.requests += 1;
        st.fallback_seconds += secs(t0);
    }

    server* _fallback;
    uint64_t _max;
    int _dev;
    hipStream_t _s = nullptr;
    std::vector<std::unique_ptr<method_entry>> _m;
    std::vector<uint8_t> _arena;  // CPU answers of the batch being sent
    std::vector<piece> _pieces;
    std::vector<uint8_t> _flat;
    bool _trace = std::getenv("SRPC_SERVER_TRACE") != nullptr;  // per-recv / per-batch timeline on stderr
    trace_point _tp;
    bool _ordered = false, _ordered_var = false, _ordered_rec = false, _ordered_legs = false;
    ordered_handler_t _ohandler;
    ordered_var_handler_t _ovhandler;
    ordered_records_handler_t _orhandler;
    ordered_legs_handler_t _olhandler;
    // the buffers (ensure / release)
    slot _slots[2];
    int _nslots = 0;
    batch_buffers _b;
    bucket_buffers _bk;
    ordered_buffers _od;
    ordered_records_buffers _or;
    ordered_var_buffers _ov;
    uint64_t _cap = 0, _scratch_bytes = 0, _var_scratch_bytes = 0, _mix_index_bytes = 0, _ov_scratch_bytes = 0;
    uint64_t _or_scratch_bytes = 0;
    bool _var_methods = false;  // a string method is registered
    uint32_t _ov_slots = 0;     // string leaves of all requests
    // per method, in registration order (build_tables)
    std::vector<const srpc_plan*> _in_plans;                  // classify's: `in`
    std::vector<const srpc_plan*> _ord_in_plans, _ord_out_plans;  // the ordered routes' decode and pack
    std::vector<uint32_t> _resp_bytes;                        // fout
    std::vector<const uint64_t*> _var_rec;                    // its response index (nullptr: fixed)
    std::vector<uint64_t> _caps;                              // elements of its columns (_max)
    std::vector<void* const*> _req_tbl, _resp_mut_tbl;        // its request / response columns
    std::vector<const void* const*> _resp_tbl;
    std::vector<uint64_t* const*> _ov_req_offs, _ov_resp_offs;  // its leaves' offsets arrays
    std::vector<const uint64_t* const*> _ov_c_req_offs, _ov_c_resp_offs;
    std::vector<const uint64_t*> _ov_req_scap, _ov_resp_cap;  // bytes a decode may fill / of its response columns
    std::vector<void*> _or_req_recs, _or_resp_recs;           // its Req / Resp array (record methods)
    std::vector<const void*> _or_c_req_recs, _or_c_resp_recs;
    std::vector<uint64_t> _or_req_stride, _or_resp_stride;    // sizeof(Req), sizeof(Resp)
    std::vector<const uint32_t*> _or_req_loffs, _or_resp_loffs;
    std::vector<const void*> _or_fill;                        // a Req{}'s bytes
};

}  // namespace srpc::gpu
