// srpc/gpu_client.hpp -- GPU-batched calls: the client-side mirror of
// srpc::gpu::batch_server (gpu_server.hpp).
//
// The reference's generated stub makes one call at a time
// (examples/calculator_srpc.cpp: pack_request -> send_data -> recv_data ->
// unpack_response<R>).  batch_client makes a whole batch of calls of one
// method from device columns, with the same frames on the wire:
//
//   request columns (device) -> srpc_gpu_pack with the framed request prefix
//   (`BE32 len | str(method) | str(Req::name) | body` frames) -> D2H -> socket,
//   sent while the replies are received (poll: the server answers while it
//   still receives, and both socket buffers are finite) -> the CPU only walks
//   the replies' BE32 lengths (walk_frames) -> H2D -> srpc_frames_unpack_replies:
//   one status code per call and the reply columns, in call order.
//
// A reply may be a full `BE32 | code | str(Resp::name) | body` frame or the
// bare `BE32(1) | code` a server sends for a method it does not know
// (server.hpp:20-24, gpu_server.hpp answer_cpu); see include/srpc_gpu.h for
// the table.  When the host walk saw only full-size frames the decode runs in
// its uniform mode and reads no offsets.  Calls the peer never answers (it
// closed the connection, or the wait timed out) get RPC_ERR_RECV_TIMEOUT and
// zero fields; every later call on this client is then unanswered too.
//
// `call` takes fixed-size Req and Resp (string schemas throw plan_error
// SRPC_E_UNSUPPORTED).  `call_var` takes methods whose request and/or response
// has std::string members, with the columns of batch_server's var_batch: a
// string request batch is packed by srpc_gpu_pack_var (prefix `str(method) |
// str(Req::name)`) and framed by srpc_frames_frame_var; a string reply stream
// is decoded by srpc_frames_unpack_replies_var (reply plan: the unframed `u8
// code | str(Resp::name)`) into the client's staging, and its chars reach the
// caller's columns only once their total is known to fit.  Both run one chunk
// loop (run_calls): each side branches on whether it has strings, and `call` is
// the case where neither has.  A method's plans are built once (one entry, one
// cache) whichever form uses it.
//
// `call_records` is `call` from and into device arrays of the caller's own
// structs (fixed-size Req and Resp, sizeof(Resp) <= 256): the same chunk loop
// with srpc_gpu_pack_aos as its pack call and srpc_frames_unpack_replies_aos as
// its decode call, so nothing is transposed on the host or on the device.
//
// `call_mixed` takes an ordered sequence of calls over up to 16 fixed-size
// methods (a trace replayed against a stateful service, a pipeline whose calls
// depend on their order): d_method[i] names call i's leg (its method, columns
// and call count), its fields are the next element of that leg's columns.  Per
// chunk: srpc_frames_mixed_index -> srpc_frames_pack_requests_mixed (the frames
// batch_server buckets per method and answers in request order) -> one
// exchange -> srpc_frames_unpack_replies_mixed, one code per call in call
// order and each reply in its leg's columns.  With a string-bodied leg
// (`leg_var`, call_var's column form) a chunk takes the same steps through
// srpc_frames_pack_requests_mixed_var and srpc_frames_unpack_replies_mixed_var:
// the traffic batch_server buckets with register_var_method beside the fixed
// methods, still in call order and one exchange per chunk.  Reply strings go
// straight to the leg's columns with offsets absolute over the whole call; a
// column's capacity is never passed, and an overflow throws SRPC_E_CAPACITY
// once the chunk is accounted for.  Both overloads are one chunk loop too: the
// pack call (and where the chunk's request bytes are read), the decode call and
// the string capacities are its only branches on `any_var`.  With struct-array
// legs (`leg_records`, call_records' form: every leg of the call, fixed-size Req
// and Resp) the same loop makes srpc_frames_pack_requests_mixed_aos and
// srpc_frames_unpack_replies_mixed_aos its pack and decode calls: call i's
// request is the next struct of its leg's request array and its reply is
// written whole into the next struct of its reply array, so a trace over
// objects keeps its call order and its one exchange per chunk without a column
// copy of any message.  `call_mixed` takes record legs as all of its legs or
// none.  `call_legs` is the same loop (run_mixed) without that restriction: any
// mix of leg, leg_var and leg_records legs, with
// srpc_frames_pack_requests_mixed_legs and
// srpc_frames_unpack_replies_mixed_legs as its pack and decode calls, so a
// client that keeps its objects as structs and has one string-bodied method
// keeps its call order across all of them.
//
// Every loop counts a chunk's replies by one rule (tally_replies,
// reply_walk.hpp): from the codes when the decode flagged nothing, otherwise
// frame by frame on the host with the judge of its table (judge_reply_fixed,
// walk_reply_var, judge_reply_mixed), and ends a chunk the same way
// (end_chunk).  The staging is owning buffers: a grow releases all of it, and
// each form re-creates what it needs.
#pragma once

#include <hip/hip_runtime_api.h>
#include <poll.h>
#include <sys/socket.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "frame_walk.hpp"
#include "reply_walk.hpp"
#include "mixed_walk.hpp"
#include "gpu.hpp"
#include "gpu_server.hpp"  // raw_plan, framed_request_prefix, framed_response_prefix

namespace srpc::gpu {

struct call_stats {
    uint64_t calls = 0;
    uint64_t ok = 0;          // full replies with code RPC_SUCCESS
    uint64_t failed = 0;      // well-formed replies (full or bare) with another code
    uint64_t malformed = 0;   // replies the decode flagged (SRPC_STATUS_PREFIX / _BOUNDS)
    uint64_t unanswered = 0;  // no reply: RPC_ERR_RECV_TIMEOUT
    uint64_t chunks = 0;          // batches of at most max_batch calls
    uint64_t uniform_chunks = 0;  // of those, decoded without offsets (every reply full size)
    uint64_t sent_bytes = 0;
    uint64_t received_bytes = 0;
    double send_seconds = 0;  // in send()
    double recv_seconds = 0;  // in poll() and recv()
    double gpu_seconds = 0;   // pack + D2H, H2D + decode + the codes' D2H, host-timed per chunk
};

/// Sizing of call_var's staging, per call (the batch average): the send
/// buffer holds max_batch * max_request_bytes + 4096 bytes of request frames,
/// the receive buffer max_batch * max_reply_bytes + 4096 of reply frames.
struct var_call_limits {
    uint64_t max_request_bytes = 512;
    uint64_t max_reply_bytes = 512;
};

/// One method of a mixed batch (batch_client::leg): its plans, its columns and
/// the number of its calls in the batch.
struct mixed_leg {
    const srpc_plan* req = nullptr;
    const srpc_plan* resp = nullptr;
    uint64_t fin = 0, fout = 0;                    // request / full reply frame bytes
    const std::vector<uint8_t>* resp_prefix = nullptr;
    void* const* d_req_cols = nullptr;
    void* const* d_resp_cols = nullptr;
    uint64_t calls = 0;
    // string-bodied legs (batch_client::leg_var); leg<> leaves these as they are
    bool req_var = false, resp_var = false;
    const uint64_t* const* d_req_str_offs = nullptr;   // per request leaf, NULL for fixed leaves
    uint64_t* const* d_resp_str_offs = nullptr;        // per reply leaf, calls + 1 entries each
    const uint64_t* resp_cap = nullptr;                // per reply leaf: the bytes a string column has
    const std::vector<uint8_t>* resp_leaf = nullptr;   // reply leaf bytes, 0: a string
    // struct-array legs (batch_client::leg_records); the column pointers above stay null
    bool records = false;
    const void* d_req_recs = nullptr;
    void* d_resp_recs = nullptr;
    uint64_t req_stride = 0, resp_stride = 0;          // sizeof(Req), sizeof(Resp)
    std::vector<uint32_t> req_offs, resp_offs;         // leaf_offsets<Req>(), leaf_offsets<Resp>()
    std::vector<uint8_t> proto;                        // resp_stride bytes: every reply byte no leaf covers
};

class batch_client {
public:
    /// Testing hook: sees every chunk's request frames in the staging buffer
    /// before they are sent (frames, index of the chunk's first call, calls,
    /// bytes per frame) and may rewrite them.
    using request_hook_t = std::function<void(uint8_t*, uint64_t, uint64_t, uint64_t)>;

    /// fd: a connected stream socket (not owned).  max_batch: calls per chunk
    /// (rounded down to a multiple of 16, the columns' alignment rule).
    explicit batch_client(int fd, uint64_t max_batch = 1u << 20, int device = 0)
        : _fd(fd), _max(std::max<uint64_t>(16, max_batch & ~15ull)), _dev(device) {
        check(hipSetDevice(device));
    }
    batch_client(batch_client const&) = delete;
    batch_client& operator=(batch_client const&) = delete;

    void set_request_hook(request_hook_t h) { _hook = std::move(h); }
    /// Keep every reply byte received by later calls (reply_bytes()).
    void keep_replies(bool on) { _keep = on; }
    std::vector<uint8_t> const& reply_bytes() const { return _kept; }
    /// How long to wait for the peer before the outstanding calls count as
    /// unanswered; negative (the default): until it answers or closes.
    void set_timeout_ms(int ms) { _timeout_ms = ms; }
    call_stats const& last_stats() const { return _last; }

    /// n calls of `method`: request field f of call i is d_req_cols[f][i];
    /// the reply's fields go to d_resp_cols[f][i] and its status code to
    /// d_codes[i] (device memory, columns 16-byte aligned).  Returns when the
    /// outputs are complete.
    template <SrpcMessage Req, SrpcMessage Resp>
    call_stats call(std::string const& method, void* const* d_req_cols, uint64_t n, void* const* d_resp_cols,
                    uint8_t* d_codes, hipStream_t stream = nullptr) {
        check(hipSetDevice(_dev));
        entry& e = plans<Req, Resp>(method);
        ensure(e.fin, e.fout);
        return run_calls(e, d_req_cols, nullptr, n, d_resp_cols, nullptr, nullptr, d_codes, stream);
    }

    /// The same from and to host records (host_columns<T> transposes them).
    template <SrpcMessage Req, SrpcMessage Resp>
    std::vector<response_t<Resp>> call(std::string const& method, std::vector<Req> const& reqs) {
        check(hipSetDevice(_dev));
        // string schemas are refused before anything is allocated
        return call_host_records<Req, Resp>(plans<Req, Resp>(method), method, reqs, nullptr);
    }

    /// n calls of `method` from and into device arrays of the caller's own
    /// structs (fixed-size Req and Resp; a string schema or sizeof(Resp) > 256
    /// throws plan_error SRPC_E_UNSUPPORTED before anything is allocated):
    /// call i takes its request from d_reqs[i] (srpc_gpu_pack_aos over
    /// leaf_offsets<Req>()) and leaves its reply in d_resps[i], written whole by
    /// srpc_frames_unpack_replies_aos -- the reply's leaves (zero unless the
    /// reply is a full frame, as `call` gives zero fields; unanswered calls
    /// likewise, with RPC_ERR_RECV_TIMEOUT), every other byte from `proto`.
    /// d_resps is 16-byte aligned, d_reqs naturally.  No transpose, on the host
    /// or on the device; chunks, hooks and counts are `call`'s.  Device code
    /// must not call a virtual function on a d_resps[i]: its vtable slot holds
    /// proto's host pointer.
    template <SrpcMessage Req, SrpcMessage Resp>
    call_stats call_records(std::string const& method, const Req* d_reqs, uint64_t n, Resp* d_resps, uint8_t* d_codes,
                            const Resp& proto = Resp{}, hipStream_t stream = nullptr) {
        check(hipSetDevice(_dev));
        if (sizeof(Resp) > 256) throw plan_error("batch_client::call_records (sizeof(Resp) > 256)", SRPC_E_UNSUPPORTED);
        entry& e = plans<Req, Resp>(method);  // string schemas are refused here, before a plan is built
        ensure(e.fin, e.fout);
        const std::vector<uint32_t> qo = leaf_offsets<Req>(), so = leaf_offsets<Resp>();
        const record_io rec{reinterpret_cast<const uint8_t*>(d_reqs), sizeof(Req), qo.data(),
                            reinterpret_cast<uint8_t*>(d_resps), sizeof(Resp), so.data(), &proto};
        return run_calls(e, nullptr, nullptr, n, nullptr, nullptr, nullptr, d_codes, stream, &rec);
    }

    /// n calls of a method whose Req and/or Resp has string fields.  The
    /// columns follow var_batch (gpu_server.hpp): a fixed field is n values, a
    /// string field its chars back to back plus n+1 u64 offsets
    /// (d_req_str_offs[f] / d_resp_str_offs[f], nullptr for fixed fields).
    /// resp_cap[f]: bytes of response column f.  The reply's string offsets
    /// are absolute over the whole call ([0] = 0, chunk k continuing from chunk
    /// k - 1's total).  Calls the peer never answers get RPC_ERR_RECV_TIMEOUT,
    /// zero fields and empty strings.  Throws plan_error(SRPC_E_CAPACITY) when
    /// a chunk's request frames outgrow the send buffer (before anything of the
    /// chunk is sent) or when the reply chars of a chunk do not fit resp_cap[f]
    /// (after the chunk is received; nothing past the cap is written).
    /// The request hook sees bytes-per-frame 0 for string requests: the frames
    /// are found by their BE32s.
    template <SrpcMessage Req, SrpcMessage Resp>
    call_stats call_var(std::string const& method, void* const* d_req_cols, const uint64_t* const* d_req_str_offs,
                        uint64_t n, void* const* d_resp_cols, uint64_t* const* d_resp_str_offs,
                        const uint64_t* resp_cap, uint8_t* d_codes, var_call_limits lim = {},
                        hipStream_t stream = nullptr) {
        check(hipSetDevice(_dev));
        entry& e = any_plans<Req, Resp>(method);
        for (size_t f = 0; f < e.resp_size.size(); ++f)
            if (e.resp_size[f] && n * e.resp_size[f] > resp_cap[f])
                throw plan_error("batch_client::call_var (response column)", SRPC_E_CAPACITY);
        ensure_bytes(_max * (e.req_var ? lim.max_request_bytes : e.fin) + 4096,
                     _max * (e.resp_var ? lim.max_reply_bytes : e.fout) + 4096);
        ensure_var(e);
        return run_calls(e, d_req_cols, d_req_str_offs, n, d_resp_cols, d_resp_str_offs, resp_cap, d_codes, stream);
    }

    /// The same from and to host records (host_columns<T> transposes them,
    /// strings included).  A response string column is given room for every
    /// reply byte the limits allow.
    template <SrpcMessage Req, SrpcMessage Resp>
    std::vector<response_t<Resp>> call_var(std::string const& method, std::vector<Req> const& reqs,
                                           var_call_limits lim = {}) {
        check(hipSetDevice(_dev));
        return call_host_records<Req, Resp>(any_plans<Req, Resp>(method), method, reqs, &lim);
    }

    /// One method of a call_mixed batch: `calls` calls of `method`, call r of
    /// them (in batch order) taking its request fields from d_req_cols[f][r]
    /// and leaving its reply in d_resp_cols[f][r] (device memory, columns
    /// 16-byte aligned, `calls` elements).  The plans are call()'s, cached by
    /// this client; a string schema throws plan_error(SRPC_E_UNSUPPORTED).
    template <SrpcMessage Req, SrpcMessage Resp>
    mixed_leg leg(std::string const& method, void* const* d_req_cols, void* const* d_resp_cols, uint64_t calls) {
        check(hipSetDevice(_dev));
        return make_leg(plans<Req, Resp>(method), d_req_cols, nullptr, d_resp_cols, nullptr, nullptr, calls);
    }

    /// A leg whose request and/or response has std::string members, in
    /// call_var's column form: a string leaf's column holds the leg's chars back
    /// to back in call order, its offsets array `calls` + 1 u64 absolute over the
    /// leg (request: read; reply: written, entry 0 included).  resp_cap[f] is
    /// read for string leaves of the reply: the bytes column f has.  The plans
    /// are call_var's.  Such legs need the call_mixed overload taking
    /// var_call_limits (the other forwards to it with the default limits).
    template <SrpcMessage Req, SrpcMessage Resp>
    mixed_leg leg_var(std::string const& method, void* const* d_req_cols, const uint64_t* const* d_req_str_offs,
                      void* const* d_resp_cols, uint64_t* const* d_resp_str_offs, const uint64_t* resp_cap,
                      uint64_t calls) {
        check(hipSetDevice(_dev));
        return make_leg(any_plans<Req, Resp>(method), d_req_cols, d_req_str_offs, d_resp_cols, d_resp_str_offs, resp_cap,
                        calls);
    }

    /// A leg from and into device arrays of the caller's own structs (fixed-size
    /// Req and Resp; a string schema or sizeof(Resp) > 256 throws plan_error
    /// SRPC_E_UNSUPPORTED before anything is allocated): call r of the leg (in
    /// batch order) takes its request from d_reqs[r] (leaf_offsets<Req>()) and
    /// leaves its reply in d_resps[r], written whole by
    /// srpc_frames_unpack_replies_mixed_aos -- the reply's leaves (zero unless
    /// the reply is a full frame, as a column leg gets zero fields; unanswered
    /// calls likewise, with RPC_ERR_RECV_TIMEOUT), every other byte from `proto`,
    /// whose bytes the leg keeps.  Both arrays are 16-byte aligned and hold
    /// `calls` structs.  The plans are call()'s, cached by this client.  Every
    /// leg of a call_mixed must then be a record leg: beside a column leg or a
    /// leg_var leg the call throws plan_error(SRPC_E_UNSUPPORTED) before anything
    /// is sent.  No transpose, on the host or on the device.  Device code must
    /// not call a virtual function on a d_resps[r]: its vtable slot holds proto's
    /// host pointer.
    template <SrpcMessage Req, SrpcMessage Resp>
    mixed_leg leg_records(std::string const& method, const Req* d_reqs, Resp* d_resps, uint64_t calls,
                          const Resp& proto = Resp{}) {
        check(hipSetDevice(_dev));
        if (sizeof(Resp) > 256) throw plan_error("batch_client::leg_records (sizeof(Resp) > 256)", SRPC_E_UNSUPPORTED);
        entry& e = plans<Req, Resp>(method);  // string schemas are refused here, before a plan is built
        mixed_leg l = make_leg(e, nullptr, nullptr, nullptr, nullptr, nullptr, calls);
        l.records = true;
        l.d_req_recs = d_reqs;
        l.d_resp_recs = d_resps;
        l.req_stride = sizeof(Req);
        l.resp_stride = sizeof(Resp);
        l.req_offs = leaf_offsets<Req>();
        l.resp_offs = leaf_offsets<Resp>();
        l.proto.assign(reinterpret_cast<const uint8_t*>(&proto), reinterpret_cast<const uint8_t*>(&proto) + sizeof(Resp));
        return l;
    }

    /// n calls in the caller's order over at most SRPC_FRAMES_MAX_PLANS legs:
    /// call i is the next call of legs[d_method[i]] (d_method: n device bytes);
    /// d_codes[i] receives its status code.  The frames leave in call order,
    /// one exchange per chunk of max_batch calls.  An id out of range, more
    /// calls of a leg than it declares (found before anything of that chunk is
    /// sent) or fewer (found after the last chunk) throws
    /// plan_error(SRPC_E_INVALID).  Calls the peer never answers get
    /// RPC_ERR_RECV_TIMEOUT and zero fields.  The request hook sees
    /// bytes-per-frame 0: the frames differ in length.
    call_stats call_mixed(std::vector<mixed_leg> const& legs, const uint8_t* d_method, uint64_t n, uint8_t* d_codes,
                          hipStream_t stream = nullptr) {
        return call_mixed(legs, d_method, n, d_codes, var_call_limits{}, stream);
    }

    /// call_mixed over legs of which some are string-bodied (leg_var); without
    /// one it is the call above and `lim` is not used.  `lim` sizes the staging
    /// as for call_var (a fixed leg's frames count with their own size).  Beyond
    /// the call above:
    /// plan_error(SRPC_E_CAPACITY) before anything of a chunk is sent when its
    /// request frames outgrow the send buffer, and after a chunk is received and
    /// accounted for when the chars of some reply column pass its resp_cap
    /// (nothing at or past the capacity was written); SRPC_E_INVALID also for a
    /// request string whose offsets decrease.  Unanswered calls get
    /// RPC_ERR_RECV_TIMEOUT, zero fields and empty strings.  Reply offsets are
    /// absolute over the whole call; the host makes no pass over them.
    call_stats call_mixed(std::vector<mixed_leg> const& legs, const uint8_t* d_method, uint64_t n, uint8_t* d_codes,
                          var_call_limits lim, hipStream_t stream = nullptr) {
        return run_mixed(legs, d_method, n, d_codes, lim, stream, false);
    }

    /// call_mixed without its restriction on the kinds of legs: any mix of
    /// leg, leg_var and leg_records legs in one ordered batch, packed by
    /// srpc_frames_pack_requests_mixed_legs and decoded by
    /// srpc_frames_unpack_replies_mixed_legs, one exchange per chunk.  Every
    /// leg keeps its own contract: a column leg's and a string leg's columns
    /// and offsets as call_mixed states them; a record leg's d_resps[r] is
    /// written whole -- the reply's leaves, every other byte from its `proto`
    /// -- and both its arrays are 16-byte aligned.  `lim` is used when a leg is
    /// string-bodied.  The errors, the capacity rules, the unanswered calls and
    /// call_stats are call_mixed's; a flagged chunk is judged on the host frame
    /// by frame, a record leg as the fixed plan it is.
    call_stats call_legs(std::vector<mixed_leg> const& legs, const uint8_t* d_method, uint64_t n, uint8_t* d_codes,
                         var_call_limits lim = {}, hipStream_t stream = nullptr) {
        return run_mixed(legs, d_method, n, d_codes, lim, stream, true);
    }

private:
    /// The chunk loop of call_mixed and call_legs.  The form of the batch --
    /// fixed columns, struct arrays, columns with strings, or (call_legs) legs
    /// of any kind -- picks the pack call, the decode call and the scratch
    /// sizing; everything else is one path.
    call_stats run_mixed(std::vector<mixed_leg> const& legs, const uint8_t* d_method, uint64_t n, uint8_t* d_codes,
                         var_call_limits lim, hipStream_t stream, bool any_kinds) {
        check(hipSetDevice(_dev));
        const std::string who = any_kinds ? "batch_client::call_legs" : "batch_client::call_mixed";
        auto error = [&who](const char* what, int code) { return plan_error((who + what).c_str(), code); };
        const size_t K = legs.size();
        if (K == 0 || K > SRPC_FRAMES_MAX_PLANS || (n && (!d_method || !d_codes))) throw error("", SRPC_E_INVALID);
        bool any_str = false;
        size_t nrec = 0;
        for (mixed_leg const& l : legs) {
            any_str = any_str || l.req_var || l.resp_var;
            nrec += l.records;
        }
        // call_mixed: struct-array legs are all of the legs, or none
        if (!any_kinds && nrec && (nrec != K || any_str))
            throw error(" (record legs beside column legs)", SRPC_E_UNSUPPORTED);
        const bool recs = !any_kinds && nrec != 0;
        // the string-aware calls: u64 totals, frames found by their offsets, out_cap under 4 GiB
        const bool any_var = any_kinds || any_str;
        uint64_t fin = any_str ? lim.max_request_bytes : 0, fout = any_str ? lim.max_reply_bytes : 0;
        std::vector<const srpc_plan*> rq(K), rs(K);
        std::vector<const void* const*> rqc(K);
        std::vector<void* const*> rsc(K);
        std::vector<const uint64_t* const*> rqo(K, nullptr);
        std::vector<uint64_t* const*> rso(K, nullptr);
        std::vector<std::vector<uint64_t>> scap(K);
        std::vector<const uint64_t*> scapp(K, nullptr);
        std::vector<uint64_t> first(K, 0), cap(K), slot_cap;
        std::vector<mixed_reply_plan> judge(K);
        std::vector<const void*> qrec(K), fill(K);
        std::vector<void*> srec(K);
        std::vector<uint64_t> qstride(K), sstride(K);
        std::vector<const uint32_t*> qoff(K), soff(K);
        for (size_t k = 0; k < K; ++k) {
            mixed_leg const& l = legs[k];
            if (!l.req || !l.resp || !l.resp_prefix ||
                (l.records ? (l.calls && (!l.d_req_recs || !l.d_resp_recs)) || l.proto.size() != l.resp_stride
                           : !l.d_req_cols || !l.d_resp_cols) ||
                (l.req_var && !l.d_req_str_offs) || (l.resp_var && (!l.d_resp_str_offs || !l.resp_cap || !l.resp_leaf)))
                throw error(" (leg)", SRPC_E_INVALID);
            qrec[k] = l.d_req_recs;
            srec[k] = l.d_resp_recs;
            qstride[k] = l.records ? l.req_stride : 0;  // call_legs: 0 names a column leg
            sstride[k] = l.records ? l.resp_stride : 0;
            qoff[k] = l.req_offs.data();
            soff[k] = l.resp_offs.data();
            fill[k] = l.proto.data();
            fin = std::max(fin, l.fin);
            fout = std::max(fout, l.fout);
            rq[k] = l.req;
            rs[k] = l.resp;
            rqc[k] = const_cast<const void* const*>(l.d_req_cols);
            rsc[k] = l.d_resp_cols;
            rqo[k] = l.req_var ? l.d_req_str_offs : nullptr;
            cap[k] = l.calls;
            judge[k].prefix = l.resp_prefix->data();
            judge[k].prefix_len = l.resp_prefix->size();
            judge[k].F = l.fout;
            judge[k].cap = l.calls;
            if (l.resp_var) {
                rso[k] = l.d_resp_str_offs;
                judge[k].var = true;
                judge[k].leaf = l.resp_leaf->data();
                judge[k].nleaves = static_cast<uint32_t>(l.resp_leaf->size());
                scap[k].resize(l.resp_leaf->size(), 0);
                for (size_t f = 0; f < l.resp_leaf->size(); ++f)
                    if ((*l.resp_leaf)[f] == 0) {
                        scap[k][f] = l.resp_cap[f];
                        slot_cap.push_back(l.resp_cap[f]);
                    }
                scapp[k] = scap[k].data();
            }
        }
        const int nk = static_cast<int>(K);
        // staging by the largest frame of each side
        if (any_str) ensure_bytes(_max * fin + 4096, _max * fout + 4096);
        else ensure(fin, fout);
        ensure_mixed();
        if (any_var) ensure_mixed_var(rq.data(), rs.data(), nk, any_kinds ? qstride.data() : nullptr, sstride.data());
        if (recs) {  // the decode's tables and fills
            uint64_t b = 0;
            check_srpc(srpc_frames_mixed_aos_scratch_bytes(rs.data(), nk, sstride.data(), &b),
                       "srpc_frames_mixed_aos_scratch_bytes");
            ensure_vscratch(b);
        }
        const uint64_t out_cap = std::min<uint64_t>(_out_cap, (1ull << 32) - 1);
        const size_t nslots = slot_cap.size();
        uint64_t* const h_counts = _s.h_mcounts;
        call_stats st;
        st.calls = n;
        for (uint64_t lo = 0; lo < n; lo += _max) {
            const uint64_t m = std::min(_max, n - lo);
            st.chunks += 1;
            auto t0 = clock::now();
            check_srpc(srpc_frames_mixed_index(d_method + lo, m, nk, _s.d_mindex, _s.mindex_bytes, _s.d_mcounts, _s.d_status,
                                               stream),
                       "srpc_frames_mixed_index");
            // the pack runs even after the peer closed: its status says whether the chunk is well formed
            if (any_kinds)
                check_srpc(srpc_frames_pack_requests_mixed_legs(rq.data(), nk, rqc.data(), rqo.data(), qrec.data(),
                                                                qstride.data(), qoff.data(), first.data(), cap.data(),
                                                                d_method + lo, _s.d_mindex, m, _s.d_out, out_cap, _s.d_moffs,
                                                                _s.d_mv, _s.d_status, _s.d_vscratch, _s.vscratch_cap, stream),
                           "srpc_frames_pack_requests_mixed_legs");
            else if (any_var)
                check_srpc(srpc_frames_pack_requests_mixed_var(rq.data(), nk, rqc.data(), rqo.data(), first.data(), cap.data(),
                                                               d_method + lo, _s.d_mindex, m, _s.d_out, out_cap, _s.d_moffs,
                                                               _s.d_mv, _s.d_status, _s.d_vscratch, _s.vscratch_cap, stream),
                           "srpc_frames_pack_requests_mixed_var");
            else if (recs)
                check_srpc(srpc_frames_pack_requests_mixed_aos(rq.data(), nk, qrec.data(), qstride.data(), qoff.data(),
                                                               first.data(), cap.data(), d_method + lo, _s.d_mindex, m,
                                                               _s.d_out, _out_cap, _s.d_moffs, _s.d_status, stream),
                           "srpc_frames_pack_requests_mixed_aos");
            else
                check_srpc(srpc_frames_pack_requests_mixed(rq.data(), nk, rqc.data(), first.data(), cap.data(), d_method + lo,
                                                           _s.d_mindex, m, _s.d_out, _out_cap, _s.d_moffs, _s.d_status, stream),
                           "srpc_frames_pack_requests_mixed");
            check(hipMemcpyAsync(h_counts, _s.d_mcounts, 8 * (K + 1), hipMemcpyDeviceToHost, stream));
            // the chunk's request bytes: a u64 total, or the last of the u32 frame offsets
            if (any_var) check(hipMemcpyAsync(_s.h_mv, _s.d_mv, 8, hipMemcpyDeviceToHost, stream));
            else check(hipMemcpyAsync(h_counts + SRPC_FRAMES_MAX_PLANS + 1, _s.d_moffs + m, 4, hipMemcpyDeviceToHost, stream));
            check(hipMemcpyAsync(_s.h_status, _s.d_status, sizeof(srpc_unpack_status), hipMemcpyDeviceToHost, stream));
            check(hipStreamSynchronize(stream));
            bool fits = h_counts[K] == 0;  // no id out of range
            // no leg with too few calls declared: the fixed pack flags one itself
            if (!any_var) fits = fits && _s.h_status->flags == 0;
            for (size_t k = 0; any_var && k < K; ++k) fits = fits && h_counts[k] <= cap[k] - std::min(cap[k], first[k]);
            if (!fits) {
                _last = st;
                throw error(" (d_method does not match the legs)", SRPC_E_INVALID);
            }
            if (any_var && _s.h_mv[0] > out_cap) {
                _last = st;
                throw error(" (requests outgrow max_request_bytes)", SRPC_E_CAPACITY);
            }
            if (any_var && _s.h_status->flags) {
                _last = st;
                throw error(" (a request string's offsets decrease)", SRPC_E_INVALID);
            }
            const uint64_t packed =
                any_var ? _s.h_mv[0] : *reinterpret_cast<const uint32_t*>(h_counts + SRPC_FRAMES_MAX_PLANS + 1);
            const uint64_t total = _eof ? 0 : packed;
            if (total) {
                check(hipMemcpyAsync(_s.h_out, _s.d_out, total, hipMemcpyDeviceToHost, stream));
                check(hipStreamSynchronize(stream));
            }
            st.gpu_seconds += secs(t0);
            if (total && _hook) _hook(_s.h_out, lo, m, 0);
            const frame_walk w = exchange(m, total, 0, st);
            t0 = clock::now();
            const uint64_t nf = w.nframes;
            if (nf) {
                check(hipMemcpyAsync(_s.d_in, _s.h_in, w.walked, hipMemcpyHostToDevice, stream));
                check(hipMemcpyAsync(_s.d_offs, _s.h_offs, 4 * nf, hipMemcpyHostToDevice, stream));
            }
            // calls without a reply get RPC_ERR_RECV_TIMEOUT, zero fields and empty strings from the decode itself
            if (any_kinds)
                check_srpc(srpc_frames_unpack_replies_mixed_legs(
                               rs.data(), nk, _s.d_in, w.walked, _s.d_offs, nf, d_method + lo, _s.d_mindex, m,
                               static_cast<uint8_t>(RPC_ERR_RECV_TIMEOUT), rsc.data(), rso.data(), scapp.data(), srec.data(),
                               sstride.data(), soff.data(), fill.data(), first.data(), cap.data(), d_codes + lo, _s.d_mv + 1,
                               _s.d_status, _s.d_vscratch, _s.vscratch_cap, stream),
                           "srpc_frames_unpack_replies_mixed_legs");
            else if (any_var)
                check_srpc(srpc_frames_unpack_replies_mixed_var(rs.data(), nk, _s.d_in, w.walked, _s.d_offs, nf, d_method + lo,
                                                                _s.d_mindex, m, static_cast<uint8_t>(RPC_ERR_RECV_TIMEOUT),
                                                                rsc.data(), rso.data(), scapp.data(), first.data(), cap.data(),
                                                                d_codes + lo, _s.d_mv + 1, _s.d_status, _s.d_vscratch,
                                                                _s.vscratch_cap, stream),
                           "srpc_frames_unpack_replies_mixed_var");
            else if (recs)
                check_srpc(srpc_frames_unpack_replies_mixed_aos(rs.data(), nk, _s.d_in, w.walked, _s.d_offs, nf, d_method + lo,
                                                                _s.d_mindex, m, static_cast<uint8_t>(RPC_ERR_RECV_TIMEOUT),
                                                                srec.data(), sstride.data(), soff.data(), fill.data(),
                                                                first.data(), cap.data(), d_codes + lo, _s.d_status,
                                                                _s.d_vscratch, _s.vscratch_cap, stream),
                           "srpc_frames_unpack_replies_mixed_aos");
            else
                check_srpc(srpc_frames_unpack_replies_mixed(rs.data(), nk, _s.d_in, w.walked, _s.d_offs, nf, d_method + lo,
                                                            _s.d_mindex, m, static_cast<uint8_t>(RPC_ERR_RECV_TIMEOUT),
                                                            rsc.data(), first.data(), cap.data(), d_codes + lo, _s.d_status,
                                                            stream),
                           "srpc_frames_unpack_replies_mixed");
            if (nf) check(hipMemcpyAsync(_s.h_codes, d_codes + lo, nf, hipMemcpyDeviceToHost, stream));
            if (nslots) check(hipMemcpyAsync(_s.h_mv + 1, _s.d_mv + 1, 8 * nslots, hipMemcpyDeviceToHost, stream));
            check(hipMemcpyAsync(_s.h_status, _s.d_status, sizeof(srpc_unpack_status), hipMemcpyDeviceToHost, stream));
            check(hipStreamSynchronize(stream));
            st.gpu_seconds += secs(t0);
            st.unanswered += m - nf;
            if (nf) {
                std::vector<uint8_t> hm;
                std::vector<uint32_t> rank;
                if (_s.h_status->flags) {  // a flagged chunk: the tables on the host, frame by frame
                    hm.resize(m);
                    rank.resize(m);
                    std::vector<uint64_t> cnt(K + 1);
                    check(hipMemcpy(hm.data(), d_method + lo, m, hipMemcpyDeviceToHost));
                    mixed_ranks(hm.data(), m, static_cast<uint32_t>(K), rank.data(), cnt.data());
                    for (size_t k = 0; k < K; ++k) judge[k].first = first[k];
                }
                count(w, st, [&](uint64_t i, uint64_t o, uint64_t end) {
                    return judge_reply_mixed(_s.h_in, w.walked, o, end, hm[i], rank[i], judge.data(), static_cast<uint32_t>(K));
                });
            }
            for (size_t k = 0; k < K; ++k) first[k] += h_counts[k];
            end_chunk(w);
            for (size_t s = 0; s < nslots; ++s)
                if (_s.h_mv[1 + s] > slot_cap[s]) {
                    _last = st;
                    throw error(" (reply chars outgrow resp_cap)", SRPC_E_CAPACITY);
                }
        }
        if (!n && any_str) {  // no chunk ran: the offsets of no calls
            for (size_t k = 0; k < K; ++k)
                for (size_t f = 0; legs[k].resp_var && f < legs[k].resp_leaf->size(); ++f)
                    if ((*legs[k].resp_leaf)[f] == 0) check(hipMemsetAsync(legs[k].d_resp_str_offs[f], 0, 8, stream));
            check(hipStreamSynchronize(stream));
        }
        _last = st;
        for (size_t k = 0; k < K; ++k)
            if (first[k] != legs[k].calls)
                throw error(" (a leg declares more calls than d_method holds)", SRPC_E_INVALID);
        return st;
    }

    using clock = std::chrono::steady_clock;

    /// A method's plans and leaf sizes, whichever form calls it: a side with
    /// strings is a string plan (unframed prefix), one without the framed fixed
    /// plan.
    struct entry {
        std::unique_ptr<raw_plan> req, resp;
        bool req_var = false, resp_var = false;
        uint64_t fin = 0, fout = 0;                 // fixed sides: request / full reply frame bytes
        std::vector<uint64_t> req_size, resp_size;  // leaf bytes, 0: a string
        std::vector<uint32_t> resp_sidx;            // string leaves: which string field of Resp
        std::vector<uint8_t> resp_leaf;             // resp_size as bytes, for walk_reply_var
        uint32_t resp_nstr = 0;
        std::vector<uint8_t> resp_prefix;           // framed (fixed Resp) or `code | str(Resp::name)`
    };

    static double secs(clock::time_point t0) { return std::chrono::duration<double>(clock::now() - t0).count(); }
    static void check(hipError_t e) {
        if (e != hipSuccess) throw plan_error(hipGetErrorString(e), SRPC_E_HIP);
    }
    static void check_srpc(int rc, const char* what) {
        if (rc < 0) throw plan_error(what, rc);
    }

    /// All of the staging (self-freeing buffers, gpu.hpp): ensure_bytes
    /// sizes the first group, the others are created by the forms that need
    /// them, and a grow starts from an empty one.
    struct staging {
        device_buffer<uint8_t> d_out, d_in;
        pinned_buffer<uint8_t> h_out, h_in, h_codes;
        device_buffer<uint32_t> d_offs;
        pinned_buffer<uint32_t> h_offs;
        device_buffer<srpc_unpack_status> d_status;
        pinned_buffer<srpc_unpack_status> h_status;
        // string sides (ensure_var, ensure_mixed_var)
        device_buffer<uint8_t> d_wire;
        device_buffer<uint64_t> d_rec;
        pinned_buffer<uint64_t> h_ends, h_soffs;
        device_buffer<void> d_vscratch;
        uint64_t vscratch_cap = 0;
        std::vector<device_buffer<uint8_t>> d_schars;
        std::vector<device_buffer<uint64_t>> d_soffs;
        // call_mixed (ensure_mixed, ensure_mixed_var)
        device_buffer<void> d_mindex;
        uint64_t mindex_bytes = 0;
        device_buffer<uint64_t> d_mcounts;
        pinned_buffer<uint64_t> h_mcounts;  // [17]: the chunk's request bytes (fixed legs)
        device_buffer<uint32_t> d_moffs;
        device_buffer<uint64_t> d_mv;
        pinned_buffer<uint64_t> h_mv;  // [0]: the chunk's request bytes, [1 + s]: reply string slot s's end
    };

    /// The plans of `method`, built once per client.
    template <SrpcMessage Req, SrpcMessage Resp>
    entry& any_plans(std::string const& method) {
        const std::string key = method + '\0' + Req::name + '\0' + Resp::name;
        auto it = _plans.find(key);
        if (it != _plans.end()) return it->second;
        const std::vector<int32_t> kq = flat_kinds<Req>(), ks = flat_kinds<Resp>();
        entry e;
        for (int32_t k : kq) e.req_var = e.req_var || k == SRPC_KIND_STRING;
        for (int32_t k : ks) e.resp_var = e.resp_var || k == SRPC_KIND_STRING;
        e.resp_prefix = e.resp_var ? response_prefix<Resp>(RPC_SUCCESS) : framed_response_prefix<Resp>(RPC_SUCCESS);
        e.req = std::make_unique<raw_plan>(kq, e.req_var ? request_prefix<Req>(method) : framed_request_prefix<Req>(method),
                                           _dev);
        e.resp = std::make_unique<raw_plan>(ks, e.resp_prefix, _dev);
        e.fin = e.req->record_bytes();
        e.fout = e.resp->record_bytes();
        Req rq{};
        for_each_leaf<Req>(rq, [&](const auto& v) {
            using F = std::remove_cvref_t<decltype(v)>;
            e.req_size.push_back(std::is_same_v<F, std::string> ? 0 : sizeof(F));
        });
        Resp rs{};
        for_each_leaf<Resp>(rs, [&](const auto& v) {
            using F = std::remove_cvref_t<decltype(v)>;
            const bool str = std::is_same_v<F, std::string>;
            e.resp_size.push_back(str ? 0 : sizeof(F));
            e.resp_leaf.push_back(static_cast<uint8_t>(str ? 0 : sizeof(F)));
            e.resp_sidx.push_back(str ? e.resp_nstr++ : 0);
        });
        if (e.resp_nstr > SRPC_FRAMES_MAX_STRINGS) throw plan_error("batch_client::call_var", SRPC_E_UNSUPPORTED);
        return _plans.emplace(key, std::move(e)).first->second;
    }

    /// The same for call and leg: a string schema is refused before a plan is built.
    template <SrpcMessage Req, SrpcMessage Resp>
    entry& plans(std::string const& method) {
        for (int32_t k : flat_kinds<Req>())
            if (k == SRPC_KIND_STRING) throw plan_error("batch_client::call (string request)", SRPC_E_UNSUPPORTED);
        for (int32_t k : flat_kinds<Resp>())
            if (k == SRPC_KIND_STRING) throw plan_error("batch_client::call (string response)", SRPC_E_UNSUPPORTED);
        return any_plans<Req, Resp>(method);
    }

    mixed_leg make_leg(entry& e, void* const* d_req_cols, const uint64_t* const* d_req_str_offs, void* const* d_resp_cols,
                       uint64_t* const* d_resp_str_offs, const uint64_t* resp_cap, uint64_t calls) {
        mixed_leg l;
        l.req = e.req->get();
        l.resp = e.resp->get();
        l.fin = e.req_var ? 0 : e.fin;
        l.fout = e.resp_var ? 0 : e.fout;
        l.resp_prefix = &e.resp_prefix;
        l.d_req_cols = d_req_cols;
        l.d_resp_cols = d_resp_cols;
        l.calls = calls;
        l.req_var = e.req_var;
        l.resp_var = e.resp_var;
        l.d_req_str_offs = d_req_str_offs;
        l.d_resp_str_offs = d_resp_str_offs;
        l.resp_cap = resp_cap;
        l.resp_leaf = &e.resp_leaf;
        return l;
    }

    /// call_records' struct arrays, in place of run_calls' columns.
    struct record_io {
        const uint8_t* d_reqs;
        uint64_t req_stride;
        const uint32_t* req_offs;  // leaf_offsets<Req>()
        uint8_t* d_resps;
        uint64_t resp_stride;
        const uint32_t* resp_offs;
        const void* fill;          // resp_stride host bytes: the proto
    };

    /// The chunk loop of call, call_var and call_records over a staging already
    /// sized.  A side without strings (for `call`, both) is packed by
    /// srpc_gpu_pack and decoded by srpc_frames_unpack_replies; the string
    /// arguments of such a side are not read.  With `rec` (fixed sides only) the
    /// columns are not read either: the pack call is srpc_gpu_pack_aos over the
    /// chunk's slice of the request structs and the decode call
    /// srpc_frames_unpack_replies_aos over its slice of the reply structs.
    call_stats run_calls(entry& e, void* const* d_req_cols, const uint64_t* const* d_req_str_offs, uint64_t n,
                         void* const* d_resp_cols, uint64_t* const* d_resp_str_offs, const uint64_t* resp_cap,
                         uint8_t* d_codes, hipStream_t stream, const record_io* rec = nullptr) {
        const size_t nq = rec ? 0 : e.req_size.size(), ns = rec ? 0 : e.resp_size.size();
        call_stats st;
        st.calls = n;
        std::vector<const void*> rq(nq);
        std::vector<const uint64_t*> rqo(nq, nullptr);
        std::vector<void*> rs(ns);
        std::vector<uint64_t*> rso(ns, nullptr);
        std::vector<uint64_t> base(ns, 0);  // chars of response field f in the chunks before this one
        for (uint64_t lo = 0; lo < n; lo += _max) {
            const uint64_t m = std::min(_max, n - lo);
            st.chunks += 1;
            uint64_t total = 0;  // the chunk's request bytes
            if (!_eof) {
                auto t0 = clock::now();
                for (size_t f = 0; f < nq; ++f) {
                    const bool str = e.req_size[f] == 0;
                    // a string column's offsets are absolute: its chars stay where they are
                    rq[f] = str ? d_req_cols[f] : static_cast<const uint8_t*>(d_req_cols[f]) + lo * e.req_size[f];
                    rqo[f] = str ? d_req_str_offs[f] + lo : nullptr;
                }
                if (e.req_var) {
                    check_srpc(srpc_gpu_pack_var(e.req->get(), rq.data(), rqo.data(), m, _s.d_wire, _out_cap, _s.d_rec,
                                                 _s.d_status, _s.d_vscratch, _s.vscratch_cap, stream),
                               "srpc_gpu_pack_var");
                    check_srpc(srpc_frames_frame_var(_s.d_wire, _s.d_rec, m, _s.d_out, _out_cap, _s.d_status, stream),
                               "srpc_frames_frame_var");
                    check(hipMemcpyAsync(_s.h_ends, _s.d_rec + m, 8, hipMemcpyDeviceToHost, stream));
                    check(hipMemcpyAsync(_s.h_status, _s.d_status, sizeof(srpc_unpack_status), hipMemcpyDeviceToHost, stream));
                    check(hipStreamSynchronize(stream));
                    total = _s.h_ends[0] + 4 * m;
                    if (total > _out_cap || _s.h_status->flags)
                        throw plan_error("batch_client::call_var (requests outgrow max_request_bytes)", SRPC_E_CAPACITY);
                } else if (rec) {
                    total = m * e.fin;
                    check_srpc(srpc_gpu_pack_aos(e.req->get(), rec->d_reqs + lo * rec->req_stride, rec->req_stride,
                                                 rec->req_offs, m, _s.d_out, total, stream),
                               "srpc_gpu_pack_aos");
                } else {
                    total = m * e.fin;
                    check_srpc(srpc_gpu_pack(e.req->get(), rq.data(), m, _s.d_out, total, stream), "srpc_gpu_pack");
                }
                check(hipMemcpyAsync(_s.h_out, _s.d_out, total, hipMemcpyDeviceToHost, stream));
                check(hipStreamSynchronize(stream));
                st.gpu_seconds += secs(t0);
                if (_hook) _hook(_s.h_out, lo, m, e.req_var ? 0 : e.fin);
            }
            const frame_walk w = exchange(m, total, e.resp_var ? 0 : e.fout, st);
            auto t0 = clock::now();
            const uint64_t nf = w.nframes;
            for (size_t f = 0; f < ns; ++f) {
                const bool str = e.resp_size[f] == 0;
                // string fields are decoded into the client's staging first
                rs[f] = str ? static_cast<void*>(_s.d_schars[e.resp_sidx[f]].p)
                            : static_cast<uint8_t*>(d_resp_cols[f]) + lo * e.resp_size[f];
                rso[f] = str ? _s.d_soffs[e.resp_sidx[f]].p : nullptr;
            }
            if (nf) {
                check(hipMemcpyAsync(_s.d_in, _s.h_in, w.walked, hipMemcpyHostToDevice, stream));
                const bool uniform = !e.resp_var && w.all_full;
                if (!uniform) check(hipMemcpyAsync(_s.d_offs, _s.h_offs, 4 * nf, hipMemcpyHostToDevice, stream));
                st.uniform_chunks += uniform;
                if (e.resp_var) {
                    check_srpc(srpc_frames_unpack_replies_var(e.resp->get(), _s.d_in, w.walked, _s.d_offs, nf, rs.data(),
                                                              rso.data(), d_codes + lo, _s.d_status, _s.d_vscratch,
                                                              _s.vscratch_cap, stream),
                               "srpc_frames_unpack_replies_var");
                    for (uint32_t t = 0; t < e.resp_nstr; ++t)
                        check(hipMemcpyAsync(_s.h_soffs + t * (_max + 1), _s.d_soffs[t], 8 * (nf + 1), hipMemcpyDeviceToHost,
                                             stream));
                } else if (rec) {
                    check_srpc(srpc_frames_unpack_replies_aos(e.resp->get(), _s.d_in, w.walked,
                                                              uniform ? nullptr : _s.d_offs.p, nf,
                                                              rec->d_resps + lo * rec->resp_stride, rec->resp_stride,
                                                              rec->resp_offs, rec->fill, d_codes + lo, _s.d_status, stream),
                               "srpc_frames_unpack_replies_aos");
                } else {
                    check_srpc(srpc_frames_unpack_replies(e.resp->get(), _s.d_in, w.walked, uniform ? nullptr : _s.d_offs.p,
                                                          nf, rs.data(), d_codes + lo, _s.d_status, stream),
                               "srpc_frames_unpack_replies");
                }
                check(hipMemcpyAsync(_s.h_codes, d_codes + lo, nf, hipMemcpyDeviceToHost, stream));
                check(hipMemcpyAsync(_s.h_status, _s.d_status, sizeof(srpc_unpack_status), hipMemcpyDeviceToHost, stream));
            }
            if (nf < m) {  // no reply: RPC_ERR_RECV_TIMEOUT, zero fields (empty strings: below)
                if (rec) unanswered_records(e, *rec, lo + nf, m - nf, d_codes, stream);  // writes their codes too: first
                check(hipMemsetAsync(d_codes + lo + nf, RPC_ERR_RECV_TIMEOUT, m - nf, stream));
                for (size_t f = 0; f < ns; ++f)
                    if (e.resp_size[f])
                        check(hipMemsetAsync(static_cast<uint8_t*>(rs[f]) + nf * e.resp_size[f], 0,
                                             (m - nf) * e.resp_size[f], stream));
                st.unanswered += m - nf;
            }
            check(hipStreamSynchronize(stream));
            // the chunk's chars, now that their totals are known: they must fit
            // the caller's columns before a byte of them is written there
            bool overflow = false;
            for (size_t f = 0; f < ns; ++f) {
                if (e.resp_size[f]) continue;
                const uint32_t t = e.resp_sidx[f];
                uint64_t* ho = _s.h_soffs + t * (_max + 1);
                const uint64_t chars = nf ? ho[nf] : 0;
                if (chars > resp_cap[f] || base[f] > resp_cap[f] - chars) {
                    overflow = true;  // thrown once the chunk's bytes are accounted for
                    continue;
                }
                if (chars)
                    check(hipMemcpyAsync(static_cast<uint8_t*>(d_resp_cols[f]) + base[f], _s.d_schars[t], chars,
                                         hipMemcpyDeviceToDevice, stream));
                // absolute offsets; unanswered calls are empty strings at the chunk's end
                if (!nf) ho[0] = 0;
                for (uint64_t j = 0; j <= nf; ++j) ho[j] += base[f];
                for (uint64_t j = nf + 1; j <= m; ++j) ho[j] = base[f] + chars;
                check(hipMemcpyAsync(d_resp_str_offs[f] + lo, ho, 8 * (m + 1), hipMemcpyHostToDevice, stream));
                base[f] += chars;
            }
            if (e.resp_var) check(hipStreamSynchronize(stream));
            st.gpu_seconds += secs(t0);
            if (nf)
                count(w, st, [&](uint64_t, uint64_t o, uint64_t end) {
                    return e.resp_var ? walk_reply_var(_s.h_in + o, end - o, e.resp_prefix.data(), e.resp_prefix.size(),
                                                       e.resp_leaf.data(), static_cast<uint32_t>(e.resp_leaf.size()))
                                      : judge_reply_fixed(_s.h_in, w.walked, o, end, e.fout, e.resp_prefix.data(),
                                                          e.resp_prefix.size());
                });
            end_chunk(w);
            if (overflow) {
                _last = st;
                throw plan_error("batch_client::call_var (reply chars outgrow resp_cap)", SRPC_E_CAPACITY);
            }
        }
        if (!n && d_resp_str_offs) {  // call_var, and no chunk ran: the offsets of no calls
            for (size_t f = 0; f < ns; ++f)
                if (!e.resp_size[f]) check(hipMemsetAsync(d_resp_str_offs[f], 0, 8, stream));
            check(hipStreamSynchronize(stream));
        }
        _last = st;
        return st;
    }

    /// call_records' structs of calls [first, first + k) the peer never answered:
    /// the proto with zero leaves.  That struct is what the decode makes of a
    /// frame that is not there (a BOUNDS row of its table), so it runs in its
    /// uniform mode over an empty stream, without a status; the codes it writes
    /// are overwritten by the caller.  The decode wants a 16-byte
    /// aligned array: the structs before the first aligned one (fewer than 16)
    /// are assembled on the host.
    void unanswered_records(entry& e, record_io const& rec, uint64_t first, uint64_t k, uint8_t* d_codes,
                            hipStream_t stream) {
        const uint64_t S = rec.resp_stride;
        std::vector<uint8_t> one(static_cast<const uint8_t*>(rec.fill), static_cast<const uint8_t*>(rec.fill) + S);
        for (size_t f = 0; f < e.resp_size.size(); ++f) std::memset(one.data() + rec.resp_offs[f], 0, e.resp_size[f]);
        uint64_t head = 0;  // structs before the first 16-byte aligned one
        while (head < k && ((first + head) * S) % 16) ++head;
        if (head) {
            _unanswered.resize(head * S);
            for (uint64_t i = 0; i < head; ++i) std::memcpy(_unanswered.data() + i * S, one.data(), S);
            check(hipMemcpyAsync(rec.d_resps + first * S, _unanswered.data(), head * S, hipMemcpyHostToDevice, stream));
        }
        if (head < k) {
            check_srpc(srpc_frames_unpack_replies_aos(e.resp->get(), _s.d_in, 0, nullptr, k - head,
                                                      rec.d_resps + (first + head) * S, S, rec.resp_offs, one.data(),
                                                      d_codes + first + head, nullptr, stream),
                       "srpc_frames_unpack_replies_aos");
        }
    }

    /// The host-record forms: the records' columns to the device, the call
    /// (`call` without limits, `call_var` with), the reply columns back.
    template <SrpcMessage Req, SrpcMessage Resp>
    std::vector<response_t<Resp>> call_host_records(entry& e, std::string const& method,
                                                    std::vector<Req> const& reqs, const var_call_limits* lim) {
        const uint64_t n = reqs.size();
        host_columns<Req> in;
        in.scatter(reqs);
        const size_t nq = e.req_size.size(), ns = e.resp_size.size();
        std::vector<device_buffer<uint8_t>> mem;  // freed together
        auto add = [&](uint64_t bytes) {
            mem.emplace_back().alloc(bytes + 16);
            return mem.back().p;
        };
        std::vector<void*> rq(nq), rs(ns);
        std::vector<const uint64_t*> rqo(nq, nullptr);
        std::vector<uint64_t*> rso(ns, nullptr);
        std::vector<uint64_t> cap(ns);
        for (size_t f = 0; f < nq; ++f) {
            rq[f] = add(in.col[f].size());
            if (!in.col[f].empty()) check(hipMemcpy(rq[f], in.col[f].data(), in.col[f].size(), hipMemcpyHostToDevice));
            if (e.req_size[f]) continue;
            uint64_t* o = reinterpret_cast<uint64_t*>(add(8 * (n + 1)));
            check(hipMemcpy(o, in.offs[f].data(), 8 * (n + 1), hipMemcpyHostToDevice));
            rqo[f] = o;
        }
        for (size_t f = 0; f < ns; ++f) {
            cap[f] = e.resp_size[f] ? n * e.resp_size[f] : n * lim->max_reply_bytes + 4096;
            rs[f] = add(cap[f]);
            if (!e.resp_size[f]) rso[f] = reinterpret_cast<uint64_t*>(add(8 * (n + 1)));
        }
        uint8_t* d_codes = add(n);
        if (lim) call_var<Req, Resp>(method, rq.data(), rqo.data(), n, rs.data(), rso.data(), cap.data(), d_codes, *lim);
        else call<Req, Resp>(method, rq.data(), n, rs.data(), d_codes);
        host_columns<Resp> out;
        out.n = n;
        out.col.resize(ns);
        out.offs.resize(ns);
        for (size_t f = 0; f < ns; ++f) {
            uint64_t bytes = n * e.resp_size[f];
            if (!e.resp_size[f]) {
                out.offs[f].resize(n + 1);
                check(hipMemcpy(out.offs[f].data(), rso[f], 8 * (n + 1), hipMemcpyDeviceToHost));
                bytes = out.offs[f][n];
            }
            out.col[f].resize(bytes);
            if (bytes) check(hipMemcpy(out.col[f].data(), rs[f], bytes, hipMemcpyDeviceToHost));
        }
        std::vector<uint8_t> codes(n);
        if (n) check(hipMemcpy(codes.data(), d_codes, n, hipMemcpyDeviceToHost));
        std::vector<Resp> vals;
        out.gather(vals);
        std::vector<response_t<Resp>> res(n);
        for (uint64_t i = 0; i < n; ++i) {
            res[i].set_code(static_cast<rpc_status_code>(codes[i]));
            res[i].set_value(vals[i]);
        }
        return res;
    }

    /// The scratch of the string calls, grown to `need` bytes.
    void ensure_vscratch(uint64_t need) {
        if (need <= _s.vscratch_cap) return;
        _s.vscratch_cap = 0;
        _s.d_vscratch.alloc(need);
        _s.vscratch_cap = need;
    }

    /// call_var's own staging beside ensure_bytes': the packed records before
    /// they are framed, the scratch of the var calls, and per response string
    /// field the chars and offsets a chunk is decoded into.
    void ensure_var(entry const& e) {
        uint64_t need = 0, b = 0;
        if (e.req_var) {
            check_srpc(srpc_plan_var_scratch_bytes(e.req->get(), _max, _out_cap, &b), "srpc_plan_var_scratch_bytes");
            need = std::max(need, b);
        }
        if (e.resp_var) {
            check_srpc(srpc_frames_replies_var_scratch_bytes(e.resp->get(), _max, &b),
                       "srpc_frames_replies_var_scratch_bytes");
            need = std::max(need, b);
        }
        ensure_vscratch(need);
        if (e.req_var && !_s.d_wire) {
            _s.d_wire.alloc(_out_cap + 16);
            _s.d_rec.alloc(8 * (_max + 1) + 16);
        }
        if (!_s.h_ends) _s.h_ends.alloc(64);
        if (e.resp_nstr > _s.d_schars.size()) _s.h_soffs.reset();
        while (_s.d_schars.size() < e.resp_nstr) {
            _s.d_schars.emplace_back().alloc(_in_cap + 16);
            _s.d_soffs.emplace_back().alloc(8 * (_max + 1) + 16);
        }
        if (e.resp_nstr && !_s.h_soffs) _s.h_soffs.alloc(8 * (_max + 1) * _s.d_schars.size());
    }

    /// call_mixed's own staging beside ensure's: the call index of a chunk,
    /// its counts and its request offsets.
    void ensure_mixed() {
        if (_s.d_mindex) return;
        check_srpc(srpc_frames_mixed_index_bytes(_max, SRPC_FRAMES_MAX_PLANS, &_s.mindex_bytes), "srpc_frames_mixed_index_bytes");
        _s.d_mindex.alloc(_s.mindex_bytes);
        _s.d_mcounts.alloc(8 * (SRPC_FRAMES_MAX_PLANS + 1));
        _s.d_moffs.alloc(4 * (_max + 1));
        _s.h_mcounts.alloc(8 * (SRPC_FRAMES_MAX_PLANS + 2));
    }

    /// The string form's staging beside ensure_mixed's: the scratch of both
    /// calls and, device and pinned, the chunk's request bytes followed by the
    /// end offset of every reply string slot.
    void ensure_mixed_var(const srpc_plan* const* rq, const srpc_plan* const* rs, int nk, const uint64_t* qstride,
                          const uint64_t* sstride) {
        uint64_t a = 0, b = 0;
        if (qstride) {  // call_legs: the record legs' tables and fills behind the same layout
            check_srpc(srpc_frames_mixed_legs_scratch_bytes(rq, nk, qstride, _max, &a), "srpc_frames_mixed_legs_scratch_bytes");
            check_srpc(srpc_frames_mixed_legs_scratch_bytes(rs, nk, sstride, _max, &b), "srpc_frames_mixed_legs_scratch_bytes");
        } else {
            check_srpc(srpc_frames_mixed_var_scratch_bytes(rq, nk, _max, &a), "srpc_frames_mixed_var_scratch_bytes");
            check_srpc(srpc_frames_mixed_var_scratch_bytes(rs, nk, _max, &b), "srpc_frames_mixed_var_scratch_bytes");
        }
        ensure_vscratch(std::max(a, b));
        if (!_s.d_mv) {
            _s.d_mv.alloc(8 * (1 + SRPC_FRAMES_MIXED_MAX_FIELDS));
            _s.h_mv.alloc(8 * (1 + SRPC_FRAMES_MIXED_MAX_FIELDS));
        }
    }

    /// Staging for chunks of _max calls with fin-byte requests and fout-byte
    /// replies.  The receive buffer has room for a chunk of full replies and
    /// 4 KiB more; a peer whose replies outgrow it is treated as closed.
    void ensure(uint64_t fin, uint64_t fout) { ensure_bytes(_max * fin + 16, _max * fout + 4096); }
    void ensure_bytes(uint64_t out, uint64_t in) {
        if (out <= _out_cap && in <= _in_cap) return;
        if (in >= (1ull << 32)) throw plan_error("batch_client: max_batch replies pass 4 GiB", SRPC_E_CAPACITY);
        std::vector<uint8_t> carry;
        if (_have) carry.assign(_s.h_in.p, _s.h_in + _have);
        _s = staging{};  // the string and mixed staging is sized by the same capacities
        _have = 0;
        _out_cap = std::max(out, _out_cap);
        _in_cap = std::max(in, _in_cap);
        _s.d_out.alloc(_out_cap);
        _s.d_in.alloc(_in_cap + 16);
        _s.d_offs.alloc(4 * _max);
        _s.d_status.alloc(sizeof(srpc_unpack_status));
        _s.h_out.alloc(_out_cap);
        _s.h_in.alloc(_in_cap);
        _s.h_offs.alloc(4 * _max);
        _s.h_codes.alloc(_max);
        _s.h_status.alloc(sizeof(srpc_unpack_status));
        if (!carry.empty()) std::memcpy(_s.h_in, carry.data(), carry.size());
        _have = carry.size();
    }

    /// Send the chunk's `total` request bytes while receiving its m replies.
    /// Neither direction blocks: poll waits for whichever is ready.
    frame_walk exchange(uint64_t m, uint64_t total, uint64_t fout, call_stats& st) {
        frame_walk w = walk_frames(_s.h_in, _have, m, _s.h_offs, fout);
        uint64_t sent = 0;
        bool send_dead = false;
        while (w.nframes < m && !_eof) {
            if (_have == _in_cap) {  // replies larger than the buffer: give the connection up
                _eof = true;
                break;
            }
            pollfd p{_fd, static_cast<short>(POLLIN | (sent < total && !send_dead ? POLLOUT : 0)), 0};
            auto t0 = clock::now();
            const int r = poll(&p, 1, _timeout_ms);
            st.recv_seconds += secs(t0);
            if (r < 0 && errno == EINTR) continue;
            if (r <= 0) {  // an error, or nothing for _timeout_ms
                _eof = true;
                break;
            }
            if (p.revents & (POLLIN | POLLHUP | POLLERR)) {
                t0 = clock::now();
                const ssize_t k = recv(_fd, _s.h_in + _have, _in_cap - _have, MSG_DONTWAIT);
                st.recv_seconds += secs(t0);
                if (k > 0) {
                    _have += static_cast<uint64_t>(k);
                    st.received_bytes += static_cast<uint64_t>(k);
                    w = walk_frames(_s.h_in, _have, m, _s.h_offs, fout, w);
                } else if (k == 0 || (errno != EAGAIN && errno != EWOULDBLOCK && errno != EINTR)) {
                    _eof = true;
                }
            }
            if ((p.revents & POLLOUT) && sent < total && !send_dead) {
                t0 = clock::now();
                const ssize_t k = send(_fd, _s.h_out + sent, total - sent, MSG_DONTWAIT | MSG_NOSIGNAL);
                st.send_seconds += secs(t0);
                if (k > 0) {
                    sent += static_cast<uint64_t>(k);
                    st.sent_bytes += static_cast<uint64_t>(k);
                } else if (k < 0 && errno != EAGAIN && errno != EWOULDBLOCK && errno != EINTR) {
                    send_dead = true;  // the peer stopped reading; what it already answered still arrives
                }
            }
        }
        return w;
    }

    /// The chunk's counts (tally_replies): from the codes, or, for a chunk the
    /// decode flagged, from judge(i, o, end) on frame i = bytes [o, end) of the
    /// receive buffer -- the table of include/srpc_gpu.h on the host.
    template <class Judge>
    void count(frame_walk const& w, call_stats& st, Judge&& judge) {
        const uint32_t* offs = _s.h_offs;
        tally_replies(_s.h_codes, w.nframes, _s.h_status->flags != 0,
                      [&](uint64_t i) { return judge(i, offs[i], i + 1 < w.nframes ? offs[i + 1] : w.walked); }, st);
    }

    /// The end of every chunk: its reply bytes are kept if asked for; bytes
    /// after its last frame belong to the next chunk's replies.
    void end_chunk(frame_walk const& w) {
        if (_keep) _kept.insert(_kept.end(), _s.h_in.p, _s.h_in + w.walked);
        std::memmove(_s.h_in, _s.h_in + w.walked, _have - w.walked);
        _have -= w.walked;
    }

    int _fd;
    uint64_t _max;
    int _dev;
    int _timeout_ms = -1;
    bool _eof = false;
    bool _keep = false;
    request_hook_t _hook;
    std::map<std::string, entry> _plans;
    std::vector<uint8_t> _kept;
    call_stats _last;
    std::vector<uint8_t> _unanswered;  // call_records: the first structs of an unanswered tail, until they are copied
    uint64_t _out_cap = 0, _in_cap = 0, _have = 0;
    staging _s;
};

}  // namespace srpc::gpu
