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
// caller's columns only once their total is known to fit.  A side without
// strings takes `call`'s path.
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
// once the chunk is accounted for.
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
    ~batch_client() { release(); }

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
        call_stats st;
        st.calls = n;
        std::vector<const void*> rq(e.req_size.size());
        std::vector<void*> rs(e.resp_size.size());
        for (uint64_t lo = 0; lo < n; lo += _max) {
            const uint64_t m = std::min(_max, n - lo);
            st.chunks += 1;
            for (size_t f = 0; f < rq.size(); ++f) rq[f] = static_cast<const uint8_t*>(d_req_cols[f]) + lo * e.req_size[f];
            for (size_t f = 0; f < rs.size(); ++f) rs[f] = static_cast<uint8_t*>(d_resp_cols[f]) + lo * e.resp_size[f];
            frame_walk w;
            if (!_eof) {
                auto t0 = clock::now();
                check_srpc(srpc_gpu_pack(e.req->get(), rq.data(), m, _d_out, m * e.fin, stream), "srpc_gpu_pack");
                check(hipMemcpyAsync(_h_out, _d_out, m * e.fin, hipMemcpyDeviceToHost, stream));
                check(hipStreamSynchronize(stream));
                st.gpu_seconds += secs(t0);
                if (_hook) _hook(_h_out, lo, m, e.fin);
            }
            w = exchange(m, m * e.fin, e.fout, st);
            auto t0 = clock::now();
            const uint64_t nf = w.nframes;
            if (nf) {
                check(hipMemcpyAsync(_d_in, _h_in, w.walked, hipMemcpyHostToDevice, stream));
                const bool uniform = w.all_full;
                if (!uniform) check(hipMemcpyAsync(_d_offs, _h_offs, 4 * nf, hipMemcpyHostToDevice, stream));
                st.uniform_chunks += uniform;
                check_srpc(srpc_frames_unpack_replies(e.resp->get(), _d_in, w.walked, uniform ? nullptr : _d_offs, nf,
                                                      rs.data(), d_codes + lo, _d_status, stream),
                           "srpc_frames_unpack_replies");
                check(hipMemcpyAsync(_h_codes, d_codes + lo, nf, hipMemcpyDeviceToHost, stream));
                check(hipMemcpyAsync(_h_status, _d_status, sizeof(srpc_unpack_status), hipMemcpyDeviceToHost, stream));
            }
            if (nf < m) {  // no reply: RPC_ERR_RECV_TIMEOUT, zero fields
                check(hipMemsetAsync(d_codes + lo + nf, RPC_ERR_RECV_TIMEOUT, m - nf, stream));
                for (size_t f = 0; f < rs.size(); ++f)
                    check(hipMemsetAsync(static_cast<uint8_t*>(rs[f]) + nf * e.resp_size[f], 0, (m - nf) * e.resp_size[f], stream));
                st.unanswered += m - nf;
            }
            check(hipStreamSynchronize(stream));
            st.gpu_seconds += secs(t0);
            if (nf) count(e.fout, e.resp_prefix, w, st);
            if (_keep) _kept.insert(_kept.end(), _h_in, _h_in + w.walked);
            // bytes after the chunk's last frame belong to the next chunk's replies
            std::memmove(_h_in, _h_in + w.walked, _have - w.walked);
            _have -= w.walked;
        }
        _last = st;
        return st;
    }

    /// The same from and to host records (host_columns<T> transposes them).
    template <SrpcMessage Req, SrpcMessage Resp>
    std::vector<response_t<Resp>> call(std::string const& method, std::vector<Req> const& reqs) {
        check(hipSetDevice(_dev));
        (void)plans<Req, Resp>(method);  // string schemas are refused before anything is allocated
        const uint64_t n = reqs.size();
        host_columns<Req> in;
        in.scatter(reqs);
        host_columns<Resp> out;
        out.n = n;
        {
            Resp probe{};
            for_each_leaf<Resp>(probe, [&](const auto& v) { out.col.emplace_back(n * sizeof(v)); });
            out.offs.resize(out.col.size());
        }
        device_buffers rq(in.col), rs(out.col);
        std::vector<uint8_t> codes(n);
        device_buffers dc(std::vector<std::vector<uint8_t>>{codes});
        for (size_t f = 0; f < in.col.size(); ++f)
            check(hipMemcpy(rq.p[f], in.col[f].data(), in.col[f].size(), hipMemcpyHostToDevice));
        call<Req, Resp>(method, rq.p.data(), n, rs.p.data(), static_cast<uint8_t*>(dc.p[0]));
        for (size_t f = 0; f < out.col.size(); ++f)
            check(hipMemcpy(out.col[f].data(), rs.p[f], out.col[f].size(), hipMemcpyDeviceToHost));
        check(hipMemcpy(codes.data(), dc.p[0], n, hipMemcpyDeviceToHost));
        std::vector<Resp> vals;
        out.gather(vals);
        std::vector<response_t<Resp>> res(n);
        for (uint64_t i = 0; i < n; ++i) {
            res[i].set_code(static_cast<rpc_status_code>(codes[i]));
            res[i].set_value(vals[i]);
        }
        return res;
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
        var_entry& e = var_plans<Req, Resp>(method);
        const size_t nq = e.req_size.size(), ns = e.resp_size.size();
        for (size_t f = 0; f < ns; ++f)
            if (e.resp_size[f] && n * e.resp_size[f] > resp_cap[f])
                throw plan_error("batch_client::call_var (response column)", SRPC_E_CAPACITY);
        ensure_bytes(_max * (e.req_var ? lim.max_request_bytes : e.fin) + 4096,
                     _max * (e.resp_var ? lim.max_reply_bytes : e.fout) + 4096);
        ensure_var(e);
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
                    check_srpc(srpc_gpu_pack_var(e.req->get(), rq.data(), rqo.data(), m, _d_wire, _out_cap, _d_rec,
                                                 _d_status, _d_vscratch, _vscratch_cap, stream),
                               "srpc_gpu_pack_var");
                    check_srpc(srpc_frames_frame_var(_d_wire, _d_rec, m, _d_out, _out_cap, _d_status, stream),
                               "srpc_frames_frame_var");
                    check(hipMemcpyAsync(_h_ends, _d_rec + m, 8, hipMemcpyDeviceToHost, stream));
                    check(hipMemcpyAsync(_h_status, _d_status, sizeof(srpc_unpack_status), hipMemcpyDeviceToHost, stream));
                    check(hipStreamSynchronize(stream));
                    total = _h_ends[0] + 4 * m;
                    if (total > _out_cap || _h_status->flags)
                        throw plan_error("batch_client::call_var (requests outgrow max_request_bytes)", SRPC_E_CAPACITY);
                } else {
                    total = m * e.fin;
                    check_srpc(srpc_gpu_pack(e.req->get(), rq.data(), m, _d_out, total, stream), "srpc_gpu_pack");
                }
                check(hipMemcpyAsync(_h_out, _d_out, total, hipMemcpyDeviceToHost, stream));
                check(hipStreamSynchronize(stream));
                st.gpu_seconds += secs(t0);
                if (_hook) _hook(_h_out, lo, m, e.req_var ? 0 : e.fin);
            }
            const frame_walk w = exchange(m, total, e.resp_var ? 0 : e.fout, st);
            auto t0 = clock::now();
            const uint64_t nf = w.nframes;
            for (size_t f = 0; f < ns; ++f) {
                const bool str = e.resp_size[f] == 0;
                // string fields are decoded into the client's staging first
                rs[f] = str ? static_cast<void*>(_d_schars[e.resp_sidx[f]])
                            : static_cast<uint8_t*>(d_resp_cols[f]) + lo * e.resp_size[f];
                rso[f] = str ? _d_soffs[e.resp_sidx[f]] : nullptr;
            }
            if (nf) {
                check(hipMemcpyAsync(_d_in, _h_in, w.walked, hipMemcpyHostToDevice, stream));
                const bool uniform = !e.resp_var && w.all_full;
                if (!uniform) check(hipMemcpyAsync(_d_offs, _h_offs, 4 * nf, hipMemcpyHostToDevice, stream));
                st.uniform_chunks += uniform;
                if (e.resp_var) {
                    check_srpc(srpc_frames_unpack_replies_var(e.resp->get(), _d_in, w.walked, _d_offs, nf, rs.data(),
                                                              rso.data(), d_codes + lo, _d_status, _d_vscratch,
                                                              _vscratch_cap, stream),
                               "srpc_frames_unpack_replies_var");
                    for (uint32_t t = 0; t < e.resp_nstr; ++t)
                        check(hipMemcpyAsync(_h_soffs + t * (_max + 1), _d_soffs[t], 8 * (nf + 1), hipMemcpyDeviceToHost,
                                             stream));
                } else {
                    check_srpc(srpc_frames_unpack_replies(e.resp->get(), _d_in, w.walked, uniform ? nullptr : _d_offs,
                                                          nf, rs.data(), d_codes + lo, _d_status, stream),
                               "srpc_frames_unpack_replies");
                }
                check(hipMemcpyAsync(_h_codes, d_codes + lo, nf, hipMemcpyDeviceToHost, stream));
                check(hipMemcpyAsync(_h_status, _d_status, sizeof(srpc_unpack_status), hipMemcpyDeviceToHost, stream));
            }
            if (nf < m) {  // no reply: RPC_ERR_RECV_TIMEOUT, zero fields (empty strings: below)
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
                uint64_t* ho = _h_soffs + t * (_max + 1);
                const uint64_t chars = nf ? ho[nf] : 0;
                if (chars > resp_cap[f] || base[f] > resp_cap[f] - chars) {
                    overflow = true;  // thrown once the chunk's bytes are accounted for
                    continue;
                }
                if (chars)
                    check(hipMemcpyAsync(static_cast<uint8_t*>(d_resp_cols[f]) + base[f], _d_schars[t], chars,
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
            if (nf) {
                if (e.resp_var) count_var(e, w, st);
                else count(e.fout, e.resp_prefix, w, st);
            }
            if (_keep) _kept.insert(_kept.end(), _h_in, _h_in + w.walked);
            std::memmove(_h_in, _h_in + w.walked, _have - w.walked);
            _have -= w.walked;
            if (overflow) {
                _last = st;
                throw plan_error("batch_client::call_var (reply chars outgrow resp_cap)", SRPC_E_CAPACITY);
            }
        }
        if (!n) {  // no chunk ran: the offsets of no calls
            for (size_t f = 0; f < ns; ++f)
                if (!e.resp_size[f]) check(hipMemsetAsync(d_resp_str_offs[f], 0, 8, stream));
            check(hipStreamSynchronize(stream));
        }
        _last = st;
        return st;
    }

    /// The same from and to host records (host_columns<T> transposes them,
    /// strings included).  A response string column is given room for every
    /// reply byte the limits allow.
    template <SrpcMessage Req, SrpcMessage Resp>
    std::vector<response_t<Resp>> call_var(std::string const& method, std::vector<Req> const& reqs,
                                           var_call_limits lim = {}) {
        check(hipSetDevice(_dev));
        var_entry& e = var_plans<Req, Resp>(method);
        const uint64_t n = reqs.size();
        host_columns<Req> in;
        in.scatter(reqs);
        const size_t nq = e.req_size.size(), ns = e.resp_size.size();
        device_allocs mem;
        std::vector<void*> rq(nq), rs(ns);
        std::vector<const uint64_t*> rqo(nq, nullptr);
        std::vector<uint64_t*> rso(ns, nullptr);
        std::vector<uint64_t> cap(ns);
        for (size_t f = 0; f < nq; ++f) {
            rq[f] = mem.add(in.col[f].size());
            if (!in.col[f].empty()) check(hipMemcpy(rq[f], in.col[f].data(), in.col[f].size(), hipMemcpyHostToDevice));
            if (e.req_size[f]) continue;
            uint64_t* o = static_cast<uint64_t*>(mem.add(8 * (n + 1)));
            check(hipMemcpy(o, in.offs[f].data(), 8 * (n + 1), hipMemcpyHostToDevice));
            rqo[f] = o;
        }
        for (size_t f = 0; f < ns; ++f) {
            cap[f] = e.resp_size[f] ? n * e.resp_size[f] : n * lim.max_reply_bytes + 4096;
            rs[f] = mem.add(cap[f]);
            if (!e.resp_size[f]) rso[f] = static_cast<uint64_t*>(mem.add(8 * (n + 1)));
        }
        uint8_t* d_codes = static_cast<uint8_t*>(mem.add(n));
        call_var<Req, Resp>(method, rq.data(), rqo.data(), n, rs.data(), rso.data(), cap.data(), d_codes, lim);
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

    /// One method of a call_mixed batch: `calls` calls of `method`, call r of
    /// them (in batch order) taking its request fields from d_req_cols[f][r]
    /// and leaving its reply in d_resp_cols[f][r] (device memory, columns
    /// 16-byte aligned, `calls` elements).  The plans are call()'s, cached by
    /// this client; a string schema throws plan_error(SRPC_E_UNSUPPORTED).
    template <SrpcMessage Req, SrpcMessage Resp>
    mixed_leg leg(std::string const& method, void* const* d_req_cols, void* const* d_resp_cols, uint64_t calls) {
        check(hipSetDevice(_dev));
        entry& e = plans<Req, Resp>(method);
        mixed_leg l;
        l.req = e.req->get();
        l.resp = e.resp->get();
        l.fin = e.fin;
        l.fout = e.fout;
        l.resp_prefix = &e.resp_prefix;
        l.d_req_cols = d_req_cols;
        l.d_resp_cols = d_resp_cols;
        l.calls = calls;
        return l;
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
        var_entry& e = var_plans<Req, Resp>(method);
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
        check(hipSetDevice(_dev));
        const size_t K = legs.size();
        if (K == 0 || K > SRPC_FRAMES_MAX_PLANS || (n && (!d_method || !d_codes)))
            throw plan_error("batch_client::call_mixed", SRPC_E_INVALID);
        for (mixed_leg const& l : legs)
            if (l.req_var || l.resp_var) return call_mixed(legs, d_method, n, d_codes, var_call_limits{}, stream);
        uint64_t fin = 0, fout = 0;
        std::vector<const srpc_plan*> rq(K), rs(K);
        std::vector<const void* const*> rqc(K);
        std::vector<void* const*> rsc(K);
        std::vector<uint64_t> first(K, 0), cap(K);
        std::vector<mixed_reply_plan> judge(K);
        for (size_t k = 0; k < K; ++k) {
            mixed_leg const& l = legs[k];
            if (!l.req || !l.resp || !l.resp_prefix || !l.d_req_cols || !l.d_resp_cols)
                throw plan_error("batch_client::call_mixed (leg)", SRPC_E_INVALID);
            fin = std::max(fin, l.fin);
            fout = std::max(fout, l.fout);
            rq[k] = l.req;
            rs[k] = l.resp;
            rqc[k] = const_cast<const void* const*>(l.d_req_cols);
            rsc[k] = l.d_resp_cols;
            cap[k] = l.calls;
            judge[k].prefix = l.resp_prefix->data();
            judge[k].prefix_len = l.resp_prefix->size();
            judge[k].F = l.fout;
            judge[k].cap = l.calls;
        }
        ensure(fin, fout);  // staging by the largest frame of each side
        ensure_mixed();
        const int nk = static_cast<int>(K);
        call_stats st;
        st.calls = n;
        for (uint64_t lo = 0; lo < n; lo += _max) {
            const uint64_t m = std::min(_max, n - lo);
            st.chunks += 1;
            auto t0 = clock::now();
            check_srpc(srpc_frames_mixed_index(d_method + lo, m, nk, _d_mindex, _mindex_bytes, _d_mcounts, _d_status, stream),
                       "srpc_frames_mixed_index");
            // the pack runs even after the peer closed: its status says whether the chunk is well formed
            check_srpc(srpc_frames_pack_requests_mixed(rq.data(), nk, rqc.data(), first.data(), cap.data(), d_method + lo,
                                                       _d_mindex, m, _d_out, _out_cap, _d_moffs, _d_status, stream),
                       "srpc_frames_pack_requests_mixed");
            check(hipMemcpyAsync(_h_mcounts, _d_mcounts, 8 * (K + 1), hipMemcpyDeviceToHost, stream));
            check(hipMemcpyAsync(_h_mcounts + SRPC_FRAMES_MAX_PLANS + 1, _d_moffs + m, 4, hipMemcpyDeviceToHost, stream));
            check(hipMemcpyAsync(_h_status, _d_status, sizeof(srpc_unpack_status), hipMemcpyDeviceToHost, stream));
            check(hipStreamSynchronize(stream));
            if (_h_status->flags || _h_mcounts[K]) {  // an id out of range, or a leg with too few calls declared
                _last = st;
                throw plan_error("batch_client::call_mixed (d_method does not match the legs)", SRPC_E_INVALID);
            }
            const uint64_t total = _eof ? 0 : *reinterpret_cast<const uint32_t*>(_h_mcounts + SRPC_FRAMES_MAX_PLANS + 1);
            if (total) {
                check(hipMemcpyAsync(_h_out, _d_out, total, hipMemcpyDeviceToHost, stream));
                check(hipStreamSynchronize(stream));
            }
            st.gpu_seconds += secs(t0);
            if (total && _hook) _hook(_h_out, lo, m, 0);
            const frame_walk w = exchange(m, total, 0, st);
            t0 = clock::now();
            const uint64_t nf = w.nframes;
            if (nf) {
                check(hipMemcpyAsync(_d_in, _h_in, w.walked, hipMemcpyHostToDevice, stream));
                check(hipMemcpyAsync(_d_offs, _h_offs, 4 * nf, hipMemcpyHostToDevice, stream));
            }
            // calls without a reply get RPC_ERR_RECV_TIMEOUT and zero fields from the decode itself
            check_srpc(srpc_frames_unpack_replies_mixed(rs.data(), nk, _d_in, w.walked, _d_offs, nf, d_method + lo,
                                                        _d_mindex, m, static_cast<uint8_t>(RPC_ERR_RECV_TIMEOUT),
                                                        rsc.data(), first.data(), cap.data(), d_codes + lo, _d_status,
                                                        stream),
                       "srpc_frames_unpack_replies_mixed");
            if (nf) check(hipMemcpyAsync(_h_codes, d_codes + lo, nf, hipMemcpyDeviceToHost, stream));
            check(hipMemcpyAsync(_h_status, _d_status, sizeof(srpc_unpack_status), hipMemcpyDeviceToHost, stream));
            check(hipStreamSynchronize(stream));
            st.gpu_seconds += secs(t0);
            st.unanswered += m - nf;
            if (nf && _h_status->flags == 0) {
                const uint64_t ok = static_cast<uint64_t>(std::count(_h_codes, _h_codes + nf, static_cast<uint8_t>(RPC_SUCCESS)));
                st.ok += ok;
                st.failed += nf - ok;
            } else if (nf) {  // a flagged chunk: the table on the host, frame by frame
                std::vector<uint8_t> hm(m);
                std::vector<uint32_t> rank(m);
                std::vector<uint64_t> cnt(K + 1);
                check(hipMemcpy(hm.data(), d_method + lo, m, hipMemcpyDeviceToHost));
                mixed_ranks(hm.data(), m, static_cast<uint32_t>(K), rank.data(), cnt.data());
                for (size_t k = 0; k < K; ++k) judge[k].first = first[k];
                for (uint64_t i = 0; i < nf; ++i) {
                    const reply_frame r = judge_reply_mixed(_h_in, w.walked, _h_offs[i], i + 1 < nf ? _h_offs[i + 1] : w.walked,
                                                            hm[i], rank[i], judge.data(), static_cast<uint32_t>(K));
                    if (r.kind != reply_kind::full && r.kind != reply_kind::bare) st.malformed += 1;
                    else if (r.code == RPC_SUCCESS) st.ok += 1;
                    else st.failed += 1;
                }
            }
            for (size_t k = 0; k < K; ++k) first[k] += _h_mcounts[k];
            if (_keep) _kept.insert(_kept.end(), _h_in, _h_in + w.walked);
            std::memmove(_h_in, _h_in + w.walked, _have - w.walked);
            _have -= w.walked;
        }
        _last = st;
        for (size_t k = 0; k < K; ++k)
            if (first[k] != legs[k].calls)
                throw plan_error("batch_client::call_mixed (a leg declares more calls than d_method holds)", SRPC_E_INVALID);
        return st;
    }

    /// call_mixed over legs of which some are string-bodied (leg_var); without
    /// one it is the call above.  `lim` sizes the staging as for call_var (a
    /// fixed leg's frames count with their own size).  Beyond the call above:
    /// plan_error(SRPC_E_CAPACITY) before anything of a chunk is sent when its
    /// request frames outgrow the send buffer, and after a chunk is received and
    /// accounted for when the chars of some reply column pass its resp_cap
    /// (nothing at or past the capacity was written); SRPC_E_INVALID also for a
    /// request string whose offsets decrease.  Unanswered calls get
    /// RPC_ERR_RECV_TIMEOUT, zero fields and empty strings.  Reply offsets are
    /// absolute over the whole call; the host makes no pass over them.
    call_stats call_mixed(std::vector<mixed_leg> const& legs, const uint8_t* d_method, uint64_t n, uint8_t* d_codes,
                          var_call_limits lim, hipStream_t stream = nullptr) {
        check(hipSetDevice(_dev));
        const size_t K = legs.size();
        if (K == 0 || K > SRPC_FRAMES_MAX_PLANS || (n && (!d_method || !d_codes)))
            throw plan_error("batch_client::call_mixed", SRPC_E_INVALID);
        bool any_var = false;
        for (mixed_leg const& l : legs) any_var = any_var || l.req_var || l.resp_var;
        if (!any_var) return call_mixed(legs, d_method, n, d_codes, stream);
        uint64_t fin = lim.max_request_bytes, fout = lim.max_reply_bytes;
        std::vector<const srpc_plan*> rq(K), rs(K);
        std::vector<const void* const*> rqc(K);
        std::vector<void* const*> rsc(K);
        std::vector<const uint64_t* const*> rqo(K, nullptr);
        std::vector<uint64_t* const*> rso(K, nullptr);
        std::vector<std::vector<uint64_t>> scap(K);
        std::vector<const uint64_t*> scapp(K, nullptr);
        std::vector<uint64_t> first(K, 0), cap(K), slot_cap;
        std::vector<mixed_reply_plan> judge(K);
        for (size_t k = 0; k < K; ++k) {
            mixed_leg const& l = legs[k];
            if (!l.req || !l.resp || !l.resp_prefix || !l.d_req_cols || !l.d_resp_cols ||
                (l.req_var && !l.d_req_str_offs) || (l.resp_var && (!l.d_resp_str_offs || !l.resp_cap || !l.resp_leaf)))
                throw plan_error("batch_client::call_mixed (leg)", SRPC_E_INVALID);
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
        ensure_bytes(_max * fin + 4096, _max * fout + 4096);
        ensure_mixed();
        const int nk = static_cast<int>(K);
        ensure_mixed_var(rq.data(), rs.data(), nk);
        const uint64_t out_cap = std::min<uint64_t>(_out_cap, (1ull << 32) - 1);
        const size_t nslots = slot_cap.size();
        call_stats st;
        st.calls = n;
        for (uint64_t lo = 0; lo < n; lo += _max) {
            const uint64_t m = std::min(_max, n - lo);
            st.chunks += 1;
            auto t0 = clock::now();
            check_srpc(srpc_frames_mixed_index(d_method + lo, m, nk, _d_mindex, _mindex_bytes, _d_mcounts, _d_status, stream),
                       "srpc_frames_mixed_index");
            // the pack runs even after the peer closed: its status says whether the chunk is well formed
            check_srpc(srpc_frames_pack_requests_mixed_var(rq.data(), nk, rqc.data(), rqo.data(), first.data(), cap.data(),
                                                           d_method + lo, _d_mindex, m, _d_out, out_cap, _d_moffs, _d_mv,
                                                           _d_status, _d_vscratch, _vscratch_cap, stream),
                       "srpc_frames_pack_requests_mixed_var");
            check(hipMemcpyAsync(_h_mcounts, _d_mcounts, 8 * (K + 1), hipMemcpyDeviceToHost, stream));
            check(hipMemcpyAsync(_h_mv, _d_mv, 8, hipMemcpyDeviceToHost, stream));
            check(hipMemcpyAsync(_h_status, _d_status, sizeof(srpc_unpack_status), hipMemcpyDeviceToHost, stream));
            check(hipStreamSynchronize(stream));
            bool fits = _h_mcounts[K] == 0;  // no id out of range, no leg with too few calls declared
            for (size_t k = 0; k < K; ++k) fits = fits && _h_mcounts[k] <= cap[k] - std::min(cap[k], first[k]);
            if (!fits) {
                _last = st;
                throw plan_error("batch_client::call_mixed (d_method does not match the legs)", SRPC_E_INVALID);
            }
            if (_h_mv[0] > out_cap) {
                _last = st;
                throw plan_error("batch_client::call_mixed (requests outgrow max_request_bytes)", SRPC_E_CAPACITY);
            }
            if (_h_status->flags) {
                _last = st;
                throw plan_error("batch_client::call_mixed (a request string's offsets decrease)", SRPC_E_INVALID);
            }
            const uint64_t total = _eof ? 0 : _h_mv[0];
            if (total) {
                check(hipMemcpyAsync(_h_out, _d_out, total, hipMemcpyDeviceToHost, stream));
                check(hipStreamSynchronize(stream));
            }
            st.gpu_seconds += secs(t0);
            if (total && _hook) _hook(_h_out, lo, m, 0);
            const frame_walk w = exchange(m, total, 0, st);
            t0 = clock::now();
            const uint64_t nf = w.nframes;
            if (nf) {
                check(hipMemcpyAsync(_d_in, _h_in, w.walked, hipMemcpyHostToDevice, stream));
                check(hipMemcpyAsync(_d_offs, _h_offs, 4 * nf, hipMemcpyHostToDevice, stream));
            }
            // calls without a reply get RPC_ERR_RECV_TIMEOUT, zero fields and empty strings from the decode itself
            check_srpc(srpc_frames_unpack_replies_mixed_var(rs.data(), nk, _d_in, w.walked, _d_offs, nf, d_method + lo,
                                                            _d_mindex, m, static_cast<uint8_t>(RPC_ERR_RECV_TIMEOUT),
                                                            rsc.data(), rso.data(), scapp.data(), first.data(), cap.data(),
                                                            d_codes + lo, _d_mv + 1, _d_status, _d_vscratch, _vscratch_cap,
                                                            stream),
                       "srpc_frames_unpack_replies_mixed_var");
            if (nf) check(hipMemcpyAsync(_h_codes, d_codes + lo, nf, hipMemcpyDeviceToHost, stream));
            if (nslots) check(hipMemcpyAsync(_h_mv + 1, _d_mv + 1, 8 * nslots, hipMemcpyDeviceToHost, stream));
            check(hipMemcpyAsync(_h_status, _d_status, sizeof(srpc_unpack_status), hipMemcpyDeviceToHost, stream));
            check(hipStreamSynchronize(stream));
            st.gpu_seconds += secs(t0);
            st.unanswered += m - nf;
            if (nf && _h_status->flags == 0) {
                const uint64_t ok = static_cast<uint64_t>(std::count(_h_codes, _h_codes + nf, static_cast<uint8_t>(RPC_SUCCESS)));
                st.ok += ok;
                st.failed += nf - ok;
            } else if (nf) {  // a flagged chunk: the tables on the host, frame by frame
                std::vector<uint8_t> hm(m);
                std::vector<uint32_t> rank(m);
                std::vector<uint64_t> cnt(K + 1);
                check(hipMemcpy(hm.data(), d_method + lo, m, hipMemcpyDeviceToHost));
                mixed_ranks(hm.data(), m, static_cast<uint32_t>(K), rank.data(), cnt.data());
                for (size_t k = 0; k < K; ++k) judge[k].first = first[k];
                for (uint64_t i = 0; i < nf; ++i) {
                    const reply_frame r = judge_reply_mixed_var(_h_in, w.walked, _h_offs[i],
                                                                i + 1 < nf ? _h_offs[i + 1] : w.walked, hm[i], rank[i],
                                                                judge.data(), static_cast<uint32_t>(K));
                    if (r.kind != reply_kind::full && r.kind != reply_kind::bare) st.malformed += 1;
                    else if (r.code == RPC_SUCCESS) st.ok += 1;
                    else st.failed += 1;
                }
            }
            for (size_t k = 0; k < K; ++k) first[k] += _h_mcounts[k];
            if (_keep) _kept.insert(_kept.end(), _h_in, _h_in + w.walked);
            std::memmove(_h_in, _h_in + w.walked, _have - w.walked);
            _have -= w.walked;
            for (size_t s = 0; s < nslots; ++s)
                if (_h_mv[1 + s] > slot_cap[s]) {
                    _last = st;
                    throw plan_error("batch_client::call_mixed (reply chars outgrow resp_cap)", SRPC_E_CAPACITY);
                }
        }
        if (!n) {  // no chunk ran: the offsets of no calls
            for (size_t k = 0; k < K; ++k)
                for (size_t f = 0; legs[k].resp_var && f < legs[k].resp_leaf->size(); ++f)
                    if ((*legs[k].resp_leaf)[f] == 0) check(hipMemsetAsync(legs[k].d_resp_str_offs[f], 0, 8, stream));
            check(hipStreamSynchronize(stream));
        }
        _last = st;
        for (size_t k = 0; k < K; ++k)
            if (first[k] != legs[k].calls)
                throw plan_error("batch_client::call_mixed (a leg declares more calls than d_method holds)", SRPC_E_INVALID);
        return st;
    }

private:
    using clock = std::chrono::steady_clock;
    struct entry {
        std::unique_ptr<raw_plan> req, resp;
        uint64_t fin = 0, fout = 0;  // request / full reply frame bytes
        std::vector<uint64_t> req_size, resp_size;
        std::vector<uint8_t> resp_prefix;
    };
    struct device_buffers {
        std::vector<void*> p;
        explicit device_buffers(std::vector<std::vector<uint8_t>> const& cols) {
            for (auto const& c : cols) {
                void* d = nullptr;
                if (hipMalloc(&d, c.size() + 16) != hipSuccess) {
                    free_all();
                    throw plan_error("batch_client: hipMalloc", SRPC_E_HIP);
                }
                p.push_back(d);
            }
        }
        device_buffers(device_buffers const&) = delete;
        device_buffers& operator=(device_buffers const&) = delete;
        ~device_buffers() { free_all(); }
        void free_all() {
            for (void* d : p) (void)hipFree(d);
            p.clear();
        }
    };

    /// Device allocations of one host-form call, freed together.
    struct device_allocs {
        std::vector<void*> p;
        device_allocs() = default;
        device_allocs(device_allocs const&) = delete;
        device_allocs& operator=(device_allocs const&) = delete;
        ~device_allocs() {
            for (void* d : p) (void)hipFree(d);
        }
        void* add(uint64_t bytes) {
            void* d = nullptr;
            if (hipMalloc(&d, bytes + 16) != hipSuccess) throw plan_error("batch_client: hipMalloc", SRPC_E_HIP);
            p.push_back(d);
            return d;
        }
    };
    /// A method of call_var: each side is a string plan (unframed prefix) or,
    /// without strings, the framed fixed plan `call` uses.
    struct var_entry {
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

    template <SrpcMessage Req, SrpcMessage Resp>
    entry& plans(std::string const& method) {
        const std::string key = method + '\0' + Req::name + '\0' + Resp::name;
        auto it = _plans.find(key);
        if (it != _plans.end()) return it->second;
        const std::vector<int32_t> kq = flat_kinds<Req>(), ks = flat_kinds<Resp>();
        for (int32_t k : kq)
            if (k == SRPC_KIND_STRING) throw plan_error("batch_client::call (string request)", SRPC_E_UNSUPPORTED);
        for (int32_t k : ks)
            if (k == SRPC_KIND_STRING) throw plan_error("batch_client::call (string response)", SRPC_E_UNSUPPORTED);
        entry e;
        e.resp_prefix = framed_response_prefix<Resp>(RPC_SUCCESS);
        e.req = std::make_unique<raw_plan>(kq, framed_request_prefix<Req>(method), _dev);
        e.resp = std::make_unique<raw_plan>(ks, e.resp_prefix, _dev);
        e.fin = e.req->record_bytes();
        e.fout = e.resp->record_bytes();
        Req rq{};
        for_each_leaf<Req>(rq, [&](const auto& v) { e.req_size.push_back(sizeof(v)); });
        Resp rs{};
        for_each_leaf<Resp>(rs, [&](const auto& v) { e.resp_size.push_back(sizeof(v)); });
        return _plans.emplace(key, std::move(e)).first->second;
    }

    template <SrpcMessage Req, SrpcMessage Resp>
    var_entry& var_plans(std::string const& method) {
        const std::string key = method + '\0' + Req::name + '\0' + Resp::name;
        auto it = _vplans.find(key);
        if (it != _vplans.end()) return it->second;
        const std::vector<int32_t> kq = flat_kinds<Req>(), ks = flat_kinds<Resp>();
        var_entry e;
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
        return _vplans.emplace(key, std::move(e)).first->second;
    }

    /// call_var's own staging beside ensure_bytes': the packed records before
    /// they are framed, the scratch of the var calls, and per response string
    /// field the chars and offsets a chunk is decoded into.
    void ensure_var(var_entry const& e) {
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
        if (need > _vscratch_cap) {
            (void)hipFree(_d_vscratch);
            _d_vscratch = nullptr;
            _vscratch_cap = 0;
            check(hipMalloc(&_d_vscratch, need));
            _vscratch_cap = need;
        }
        if (e.req_var && !_d_wire) {
            check(hipMalloc(reinterpret_cast<void**>(&_d_wire), _out_cap + 16));
            check(hipMalloc(reinterpret_cast<void**>(&_d_rec), 8 * (_max + 1) + 16));
        }
        if (!_h_ends) check(hipHostMalloc(reinterpret_cast<void**>(&_h_ends), 64));
        if (e.resp_nstr > _d_schars.size() && _h_soffs) {
            (void)hipHostFree(_h_soffs);
            _h_soffs = nullptr;
        }
        while (_d_schars.size() < e.resp_nstr) {
            void *c = nullptr, *o = nullptr;
            check(hipMalloc(&c, _in_cap + 16));
            _d_schars.push_back(static_cast<uint8_t*>(c));
            check(hipMalloc(&o, 8 * (_max + 1) + 16));
            _d_soffs.push_back(static_cast<uint64_t*>(o));
        }
        if (e.resp_nstr && !_h_soffs)
            check(hipHostMalloc(reinterpret_cast<void**>(&_h_soffs), 8 * (_max + 1) * _d_schars.size()));
    }

    /// call_mixed's own staging beside ensure's: the call index of a chunk,
    /// its counts and its request offsets.
    void ensure_mixed() {
        if (_d_mindex) return;
        check_srpc(srpc_frames_mixed_index_bytes(_max, SRPC_FRAMES_MAX_PLANS, &_mindex_bytes), "srpc_frames_mixed_index_bytes");
        check(hipMalloc(&_d_mindex, _mindex_bytes));
        check(hipMalloc(reinterpret_cast<void**>(&_d_mcounts), 8 * (SRPC_FRAMES_MAX_PLANS + 1)));
        check(hipMalloc(reinterpret_cast<void**>(&_d_moffs), 4 * (_max + 1)));
        check(hipHostMalloc(reinterpret_cast<void**>(&_h_mcounts), 8 * (SRPC_FRAMES_MAX_PLANS + 2)));
    }

    /// The string form's staging beside ensure_mixed's: the scratch of both
    /// calls and, device and pinned, the chunk's request bytes followed by the
    /// end offset of every reply string slot.
    void ensure_mixed_var(const srpc_plan* const* rq, const srpc_plan* const* rs, int nk) {
        uint64_t a = 0, b = 0;
        check_srpc(srpc_frames_mixed_var_scratch_bytes(rq, nk, _max, &a), "srpc_frames_mixed_var_scratch_bytes");
        check_srpc(srpc_frames_mixed_var_scratch_bytes(rs, nk, _max, &b), "srpc_frames_mixed_var_scratch_bytes");
        const uint64_t need = std::max(a, b);
        if (need > _vscratch_cap) {
            (void)hipFree(_d_vscratch);
            _d_vscratch = nullptr;
            _vscratch_cap = 0;
            check(hipMalloc(&_d_vscratch, need));
            _vscratch_cap = need;
        }
        if (!_d_mv) {
            check(hipMalloc(reinterpret_cast<void**>(&_d_mv), 8 * (1 + SRPC_FRAMES_MIXED_MAX_FIELDS)));
            check(hipHostMalloc(reinterpret_cast<void**>(&_h_mv), 8 * (1 + SRPC_FRAMES_MIXED_MAX_FIELDS)));
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
        if (_have) carry.assign(_h_in, _h_in + _have);
        release();
        _out_cap = std::max(out, _out_cap);
        _in_cap = std::max(in, _in_cap);
        check(hipMalloc(reinterpret_cast<void**>(&_d_out), _out_cap));
        check(hipMalloc(reinterpret_cast<void**>(&_d_in), _in_cap + 16));
        check(hipMalloc(reinterpret_cast<void**>(&_d_offs), 4 * _max));
        check(hipMalloc(reinterpret_cast<void**>(&_d_status), sizeof(srpc_unpack_status)));
        check(hipHostMalloc(reinterpret_cast<void**>(&_h_out), _out_cap));
        check(hipHostMalloc(reinterpret_cast<void**>(&_h_in), _in_cap));
        check(hipHostMalloc(reinterpret_cast<void**>(&_h_offs), 4 * _max));
        check(hipHostMalloc(reinterpret_cast<void**>(&_h_codes), _max));
        check(hipHostMalloc(reinterpret_cast<void**>(&_h_status), sizeof(srpc_unpack_status)));
        if (!carry.empty()) std::memcpy(_h_in, carry.data(), carry.size());
        _have = carry.size();
    }

    void release() {
        (void)hipFree(_d_mv);
        (void)hipHostFree(_h_mv);
        _d_mv = _h_mv = nullptr;
        (void)hipFree(_d_mindex);
        (void)hipFree(_d_mcounts);
        (void)hipFree(_d_moffs);
        (void)hipHostFree(_h_mcounts);
        _d_mindex = nullptr;
        _d_mcounts = _h_mcounts = nullptr;
        _d_moffs = nullptr;
        // call_var's staging is sized by the same capacities
        (void)hipFree(_d_wire);
        (void)hipFree(_d_rec);
        (void)hipFree(_d_vscratch);
        (void)hipHostFree(_h_ends);
        (void)hipHostFree(_h_soffs);
        for (uint8_t* c : _d_schars) (void)hipFree(c);
        for (uint64_t* o : _d_soffs) (void)hipFree(o);
        _d_schars.clear();
        _d_soffs.clear();
        _d_wire = nullptr;
        _d_rec = _h_ends = _h_soffs = nullptr;
        _d_vscratch = nullptr;
        _vscratch_cap = 0;
        (void)hipFree(_d_out);
        (void)hipFree(_d_in);
        (void)hipFree(_d_offs);
        (void)hipFree(_d_status);
        (void)hipHostFree(_h_out);
        (void)hipHostFree(_h_in);
        (void)hipHostFree(_h_offs);
        (void)hipHostFree(_h_codes);
        (void)hipHostFree(_h_status);
        _d_out = _d_in = _h_out = _h_in = _h_codes = nullptr;
        _d_offs = _h_offs = nullptr;
        _d_status = _h_status = nullptr;
        _have = 0;
    }

    /// Send the chunk's `total` request bytes while receiving its m replies.
    /// Neither direction blocks: poll waits for whichever is ready.
    frame_walk exchange(uint64_t m, uint64_t total, uint64_t fout, call_stats& st) {
        frame_walk w = walk_frames(_h_in, _have, m, _h_offs, fout);
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
                const ssize_t k = recv(_fd, _h_in + _have, _in_cap - _have, MSG_DONTWAIT);
                st.recv_seconds += secs(t0);
                if (k > 0) {
                    _have += static_cast<uint64_t>(k);
                    st.received_bytes += static_cast<uint64_t>(k);
                    w = walk_frames(_h_in, _have, m, _h_offs, fout, w);
                } else if (k == 0 || (errno != EAGAIN && errno != EWOULDBLOCK && errno != EINTR)) {
                    _eof = true;
                }
            }
            if ((p.revents & POLLOUT) && sent < total && !send_dead) {
                t0 = clock::now();
                const ssize_t k = send(_fd, _h_out + sent, total - sent, MSG_DONTWAIT | MSG_NOSIGNAL);
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

    /// The chunk's counts from the codes; only a chunk the decode flagged is
    /// looked at frame by frame (the table of include/srpc_gpu.h on the host).
    void count(uint64_t fout, std::vector<uint8_t> const& resp_prefix, frame_walk const& w, call_stats& st) {
        const uint64_t nf = w.nframes;
        if (_h_status->flags == 0) {
            const uint64_t ok = static_cast<uint64_t>(std::count(_h_codes, _h_codes + nf, static_cast<uint8_t>(RPC_SUCCESS)));
            st.ok += ok;
            st.failed += nf - ok;
            return;
        }
        for (uint64_t i = 0; i < nf; ++i) {
            const uint64_t o = _h_offs[i], end = i + 1 < nf ? _h_offs[i + 1] : w.walked, len = end - o;
            const uint8_t* f = _h_in + o;
            const bool full = len == fout && std::memcmp(f, resp_prefix.data(), 4) == 0 &&
                              std::memcmp(f + 5, resp_prefix.data() + 5, resp_prefix.size() - 5) == 0;
            const bool bare = len == 5 && f[4] != 0;
            if (!(full || bare)) st.malformed += 1;
            else if (_h_codes[i] == RPC_SUCCESS) st.ok += 1;
            else st.failed += 1;
        }
    }

    /// count for a string reply stream: a flagged chunk is recounted with the
    /// table of srpc_frames_unpack_replies_var on the host (walk_reply_var).
    void count_var(var_entry const& e, frame_walk const& w, call_stats& st) {
        const uint64_t nf = w.nframes;
        if (_h_status->flags == 0) {
            const uint64_t ok = static_cast<uint64_t>(std::count(_h_codes, _h_codes + nf, static_cast<uint8_t>(RPC_SUCCESS)));
            st.ok += ok;
            st.failed += nf - ok;
            return;
        }
        for (uint64_t i = 0; i < nf; ++i) {
            const uint64_t o = _h_offs[i], end = i + 1 < nf ? _h_offs[i + 1] : w.walked;
            const reply_frame r = walk_reply_var(_h_in + o, end - o, e.resp_prefix.data(), e.resp_prefix.size(),
                                                 e.resp_leaf.data(), static_cast<uint32_t>(e.resp_leaf.size()));
            if (r.kind != reply_kind::full && r.kind != reply_kind::bare) st.malformed += 1;
            else if (r.code == RPC_SUCCESS) st.ok += 1;
            else st.failed += 1;
        }
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
    uint64_t _out_cap = 0, _in_cap = 0, _have = 0;
    uint8_t *_d_out = nullptr, *_d_in = nullptr, *_h_out = nullptr, *_h_in = nullptr, *_h_codes = nullptr;
    uint32_t *_d_offs = nullptr, *_h_offs = nullptr;
    srpc_unpack_status *_d_status = nullptr, *_h_status = nullptr;
    // call_var
    std::map<std::string, var_entry> _vplans;
    uint8_t* _d_wire = nullptr;
    uint64_t *_d_rec = nullptr, *_h_ends = nullptr, *_h_soffs = nullptr;
    void* _d_vscratch = nullptr;
    uint64_t _vscratch_cap = 0;
    std::vector<uint8_t*> _d_schars;
    std::vector<uint64_t*> _d_soffs;
    // call_mixed
    void* _d_mindex = nullptr;
    uint64_t _mindex_bytes = 0;
    uint64_t *_d_mcounts = nullptr, *_h_mcounts = nullptr;  // _h_mcounts[17]: the chunk's request bytes
    uint32_t* _d_moffs = nullptr;
    uint64_t *_d_mv = nullptr, *_h_mv = nullptr;  // [0]: the chunk's request bytes, [1 + s]: reply string slot s's end
};

}  // namespace srpc::gpu
