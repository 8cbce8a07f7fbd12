"""Host-side batch packer over the HIP C ABI.

Mirrors the reference packer's vocabulary (include/srpc/packer.hpp):
``pack`` / ``unpack`` are the batched ``p << r`` / ``r.unpack(bp)`` loops,
``for_request`` / ``for_response`` build the constant envelope header that
``packer::pack_request`` (packer.hpp:77-82) and ``packer::pack_response``
(packer.hpp:86-91) emit in front of every body.

Device memory is passed as raw device pointers (ints) or as any object with a
``data_ptr()`` method (e.g. a torch tensor on the GPU); streams as a raw
``hipStream_t`` (int) or an object with ``cuda_stream``.
"""
from __future__ import annotations

import ctypes as C
import struct
from dataclasses import dataclass, field
from typing import Iterable, Optional, Sequence

from . import _lib
from ._lib import SrpcError, check

# IDL kinds (include/srpc_gpu.h, = the type table of parser.hpp:253-290)
BOOL, INT8, CHAR, INT16, INT32, INT64, STRING = 1, 2, 3, 4, 5, 6, 7
KIND_NAMES = {"bool": BOOL, "int8": INT8, "char": CHAR, "int16": INT16, "int32": INT32,
              "int64": INT64, "string": STRING}
KIND_SIZE = {BOOL: 1, INT8: 1, CHAR: 1, INT16: 2, INT32: 4, INT64: 8, STRING: 0}

# rpc_status_code (packer.hpp:16-20)
RPC_SUCCESS, RPC_ERR_FUNCTION_NOT_REGISTERED, RPC_ERR_RECV_TIMEOUT = 0, 1, 2


@dataclass(frozen=True)
class Schema:
    """A message type: its name (``T::name``) and its flattened fields in
    ``T::fields`` declaration order (nested messages inlined, as
    ``pack_arg`` does for message-typed members, packer.hpp:185-186)."""

    name: str
    fields: tuple = field(default_factory=tuple)  # ((field_name, kind), ...)

    @staticmethod
    def of(name: str, *fields) -> "Schema":
        out = []
        for fname, kind in fields:
            if isinstance(kind, Schema):  # nested message: inline its fields
                out.extend((f"{fname}.{n}", k) for n, k in kind.fields)
            else:
                out.append((fname, KIND_NAMES[kind] if isinstance(kind, str) else int(kind)))
        return Schema(name, tuple(out))

    @property
    def kinds(self) -> list[int]:
        return [k for _, k in self.fields]

    @property
    def body_bytes(self) -> int:
        """Fixed body size, 0 if the schema has a string field."""
        if any(k == STRING for k in self.kinds):
            return 0
        return sum(KIND_SIZE[k] for k in self.kinds)


def request_prefix(method: str, msg_name: str) -> bytes:
    """``u64 len(method) | method | u64 len(T::name) | T::name`` (packer.hpp:77-82,
    strings per pack_arg<std::string> 193-198 and pack_arg<const char*> 203-208)."""
    m, n = method.encode(), msg_name.encode()
    return struct.pack("<Q", len(m)) + m + struct.pack("<Q", len(n)) + n


def response_prefix(code: int, msg_name: str) -> bytes:
    """``u8 code | u64 len(T::name) | T::name`` (packer.hpp:86-91)."""
    n = msg_name.encode()
    return bytes([code & 0xFF]) + struct.pack("<Q", len(n)) + n


def _dptr(x) -> int:
    if x is None:
        return 0
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        return int(x.data_ptr())
    raise TypeError(f"expected a device pointer or tensor, got {type(x)!r}")


def _stream(s) -> int:
    if s is None:
        return 0
    if isinstance(s, int):
        return s
    if hasattr(s, "cuda_stream"):
        return int(s.cuda_stream)
    raise TypeError(f"expected a hipStream_t handle or stream object, got {type(s)!r}")


class GpuPacker:
    """A plan for one record schema (+ optional envelope prefix) on one device."""

    def __init__(self, schema: Schema, prefix: bytes = b"", device: int = 0):
        self.schema = schema
        self.prefix = bytes(prefix)
        self.device = device
        L = _lib.lib()
        kinds = (C.c_int32 * len(schema.kinds))(*schema.kinds)
        pre = (C.c_uint8 * max(1, len(self.prefix))).from_buffer_copy(self.prefix or b"\0")
        desc = _lib.SchemaDesc(len(schema.kinds), kinds, pre, len(self.prefix))
        h = C.c_void_p()
        check(L.srpc_plan_create(C.byref(desc), device, C.byref(h)), "srpc_plan_create")
        self._h = h
        rb = C.c_uint64()
        check(L.srpc_plan_record_bytes(h, C.byref(rb)), "srpc_plan_record_bytes")
        self.record_bytes = rb.value

    @classmethod
    def for_request(cls, schema: Schema, method: str, device: int = 0) -> "GpuPacker":
        return cls(schema, request_prefix(method, schema.name), device)

    @classmethod
    def for_response(cls, schema: Schema, code: int = RPC_SUCCESS, device: int = 0) -> "GpuPacker":
        return cls(schema, response_prefix(code, schema.name), device)

    # -- plan info ---------------------------------------------------------
    @property
    def path(self) -> int:
        p = C.c_int()
        check(_lib.lib().srpc_plan_path(self._h, C.byref(p)), "srpc_plan_path")
        return p.value

    def force_path(self, path: int) -> None:
        check(_lib.lib().srpc_plan_force_path(self._h, path), "srpc_plan_force_path")

    def tune(self, records_per_lane: int | None = None, iters: int | None = None,
             nontemporal: int | None = None, tile_bytes: int | None = None,
             grid: int | None = None, pack_tile_bytes: int | None = None,
             var_kernel: int | None = None, var_image_bytes: int | None = None,
             var_chars_bytes: int | None = None, wave_pack_bytes: int | None = None,
             wave_unpack_bytes: int | None = None, rec_kernel: int | None = None,
             sweep: int | None = None, unpack_nontemporal: int | None = None) -> None:
        """Performance knobs (srpc_plan_tune); output bytes never change.
        var_kernel: VAR pack, 1 = record tiles (one pass), 0 = scan + chunk walk.
        rec_kernel: TILE schema-specialised kernels, 1 = where measured faster, 2 = both directions, 0 = off.
        sweep: DWORD path, bit 0 = pack walks the records downwards, bit 1 = unpack does."""
        L = _lib.lib()
        for knob, val in ((1, records_per_lane), (2, iters), (3, nontemporal), (4, tile_bytes),
                          (5, grid), (9, pack_tile_bytes), (7, var_kernel), (8, var_image_bytes),
                          (10, var_chars_bytes), (11, wave_pack_bytes), (12, wave_unpack_bytes),
                          (13, rec_kernel), (14, sweep), (15, unpack_nontemporal)):
            if val is not None:
                check(L.srpc_plan_tune(self._h, knob, int(val)), "srpc_plan_tune")

    def wire_bytes(self, n: int) -> int:
        return n * self.record_bytes

    # -- hot path ----------------------------------------------------------
    def _cols(self, cols: Sequence) -> C.Array:
        if len(cols) != len(self.schema.kinds):
            raise ValueError(f"{self.schema.name}: expected {len(self.schema.kinds)} columns, "
                             f"got {len(cols)}")
        return (C.c_void_p * len(cols))(*[_dptr(c) for c in cols])

    def pack(self, cols: Sequence, n: int, wire, wire_cap: int | None = None, stream=None) -> int:
        """Pack n records from device columns into device wire bytes (async)."""
        arr = self._cols(cols)
        cap = self.wire_bytes(n) if wire_cap is None else wire_cap
        check(_lib.lib().srpc_gpu_pack(self._h, arr, n, _dptr(wire), cap, _stream(stream)),
              "srpc_gpu_pack")
        return self.wire_bytes(n)

    def unpack(self, wire, wire_len: int, n: int, cols: Sequence, status=None, stream=None) -> int:
        """Unpack n records from device wire bytes into device columns (async).
        ``status``: device pointer to a 16-byte srpc_unpack_status, or None.
        Returns SRPC_OK or SRPC_ERR_BOUNDS."""
        arr = self._cols(cols)
        return check(_lib.lib().srpc_gpu_unpack(self._h, _dptr(wire), wire_len, n, arr,
                                                _dptr(status), _stream(stream)),
                     "srpc_gpu_unpack")

    # -- framed reply streams (client side) ----------------------------------
    def unpack_replies(self, buf, buf_len: int, offs, nframes: int, cols: Sequence, codes, status=None,
                       stream=None) -> int:
        """Decode a reply stream of mixed frames in call order (async): this
        plan's prefix is a framed response prefix (``framed_response_prefix``).
        ``offs``: nframes u32 device offsets of the frames, or None when every
        frame is full size (uniform mode).  ``codes``: nframes device bytes,
        one status code per call (SRPC_REPLY_NO_CODE where none could be read).
        Returns SRPC_OK or SRPC_ERR_BOUNDS."""
        arr = self._cols(cols)
        return check(_lib.lib().srpc_frames_unpack_replies(self._h, _dptr(buf), buf_len, _dptr(offs), nframes, arr,
                                                           _dptr(codes), _dptr(status), _stream(stream)),
                     "srpc_frames_unpack_replies")

    @property
    def replies_per_tile(self) -> int:
        """Frames one workgroup of unpack_replies takes (testing hook)."""
        out = C.c_uint32()
        check(_lib.lib().srpc_frames_replies_per_tile(self._h, C.byref(out)), "srpc_frames_replies_per_tile")
        return out.value

    def unpack_replies_aos(self, buf, buf_len: int, offs, nframes: int, records, record_stride: int,
                           field_offsets: Sequence[int], fill: bytes, codes, status=None, stream=None) -> int:
        """As unpack_replies, straight into a device array of structs (async):
        every one of the nframes structs is written whole, its leaf fields from
        the frame (zero unless the frame is full), every other byte from `fill`
        (record_stride bytes, e.g. a T{} image; at most 256).  Returns SRPC_OK
        or SRPC_ERR_BOUNDS."""
        if len(fill) != record_stride:
            raise ValueError("fill must be record_stride bytes")
        hb = C.create_string_buffer(bytes(fill), record_stride)
        return check(_lib.lib().srpc_frames_unpack_replies_aos(self._h, _dptr(buf), buf_len, _dptr(offs), nframes,
                                                               _dptr(records), record_stride,
                                                               self._offsets(field_offsets), hb, _dptr(codes),
                                                               _dptr(status), _stream(stream)),
                     "srpc_frames_unpack_replies_aos")

    def replies_aos_per_tile(self, record_stride: int) -> int:
        """Frames one workgroup of unpack_replies_aos takes for this stride (testing hook)."""
        out = C.c_uint32()
        check(_lib.lib().srpc_frames_replies_aos_per_tile(self._h, record_stride, C.byref(out)),
              "srpc_frames_replies_aos_per_tile")
        return out.value

    # -- framed reply streams with string fields (client side) ----------------
    def replies_var_scratch_bytes(self, nframes: int) -> int:
        """Device scratch for unpack_replies_var (8-byte aligned)."""
        out = C.c_uint64()
        check(_lib.lib().srpc_frames_replies_var_scratch_bytes(self._h, nframes, C.byref(out)),
              "srpc_frames_replies_var_scratch_bytes")
        return out.value

    def unpack_replies_var(self, buf, buf_len: int, offs, nframes: int, cols: Sequence, str_offs: Sequence, codes,
                           scratch, scratch_bytes: int, status=None, stream=None) -> None:
        """Decode a reply stream of mixed frames of a string response in call
        order (async): this plan's prefix is the unframed ``response_prefix``.
        ``offs``: nframes u32 device offsets of the frames.  String field f's
        chars go to cols[f] (room for buf_len bytes), its nframes+1 offsets to
        str_offs[f]; ``codes``: one status code per call."""
        check(_lib.lib().srpc_frames_unpack_replies_var(self._h, _dptr(buf), buf_len, _dptr(offs), nframes,
                                                        self._cols(cols), self._str_offs(str_offs), _dptr(codes),
                                                        _dptr(status), _dptr(scratch), scratch_bytes,
                                                        _stream(stream)),
              "srpc_frames_unpack_replies_var")

    @property
    def replies_var_tile(self) -> tuple[int, int]:
        """(frames per workgroup tile, LDS image bytes) of unpack_replies_var (testing hook)."""
        fr, im = C.c_uint32(), C.c_uint32()
        check(_lib.lib().srpc_frames_replies_var_tile(self._h, C.byref(fr), C.byref(im)),
              "srpc_frames_replies_var_tile")
        return fr.value, im.value

    # -- host-terminated batches (ABI 7) ---------------------------------------
    def host_scratch_bytes(self, chunk_records: int, depth: int = 3) -> int:
        out = C.c_uint64()
        check(_lib.lib().srpc_plan_host_scratch_bytes(self._h, chunk_records, depth, C.byref(out)),
              "srpc_plan_host_scratch_bytes")
        return out.value

    def pack_host(self, h_cols: Sequence, n: int, h_wire, chunk_records: int, scratch, scratch_bytes: int,
                  depth: int = 3, wire_cap: int | None = None, stream=None) -> int:
        """Pack n records from HOST columns into HOST wire bytes, pipelined
        through `depth` device buffers of `chunk_records` (async on `stream`;
        host buffers: pinned tensors or addresses)."""
        arr = self._cols(h_cols)
        cap = self.wire_bytes(n) if wire_cap is None else wire_cap
        check(_lib.lib().srpc_gpu_pack_host(self._h, arr, n, _dptr(h_wire), cap, chunk_records, depth,
                                            _dptr(scratch), scratch_bytes, _stream(stream)), "srpc_gpu_pack_host")
        return self.wire_bytes(n)

    def unpack_host(self, h_wire, wire_len: int, n: int, h_cols: Sequence, chunk_records: int, scratch,
                    scratch_bytes: int, depth: int = 3, status=None, stream=None) -> int:
        """Unpack n records from HOST wire bytes into HOST columns (the mirror
        of pack_host).  Returns SRPC_OK or SRPC_ERR_BOUNDS."""
        arr = self._cols(h_cols)
        return check(_lib.lib().srpc_gpu_unpack_host(self._h, _dptr(h_wire), wire_len, n, arr, chunk_records, depth,
                                                     _dptr(scratch), scratch_bytes, _dptr(status), _stream(stream)),
                     "srpc_gpu_unpack_host")

    # -- records as structs (AoS) ---------------------------------------------
    def _offsets(self, field_offsets: Sequence[int]) -> C.Array:
        if len(field_offsets) != len(self.schema.kinds):
            raise ValueError(f"{self.schema.name}: expected {len(self.schema.kinds)} field offsets")
        return (C.c_uint32 * len(field_offsets))(*[int(o) for o in field_offsets])

    def pack_aos(self, records, record_stride: int, field_offsets: Sequence[int], n: int, wire,
                 wire_cap: int | None = None, stream=None) -> int:
        """Pack n records from a device array of structs (e.g. a numpy structured
        dtype's bytes): field f of record r at r * record_stride + field_offsets[f]."""
        cap = self.wire_bytes(n) if wire_cap is None else wire_cap
        check(_lib.lib().srpc_gpu_pack_aos(self._h, _dptr(records), record_stride, self._offsets(field_offsets), n,
                                           _dptr(wire), cap, _stream(stream)), "srpc_gpu_pack_aos")
        return self.wire_bytes(n)

    def unpack_aos(self, wire, wire_len: int, n: int, records, record_stride: int, field_offsets: Sequence[int],
                   status=None, stream=None) -> int:
        """Unpack n records into the leaf fields of a device array of structs
        (other bytes untouched).  Returns SRPC_OK or SRPC_ERR_BOUNDS."""
        return check(_lib.lib().srpc_gpu_unpack_aos(self._h, _dptr(wire), wire_len, n, _dptr(records), record_stride,
                                                    self._offsets(field_offsets), _dptr(status), _stream(stream)),
                     "srpc_gpu_unpack_aos")

    def unpack_aos_fill(self, wire, wire_len: int, n: int, records, record_stride: int,
                        field_offsets: Sequence[int], fill: bytes, status=None, stream=None) -> int:
        """As unpack_aos into fresh objects: every struct byte no leaf field
        covers is set from `fill` (record_stride bytes, e.g. a T{} image)."""
        if len(fill) != record_stride:
            raise ValueError("fill must be record_stride bytes")
        buf = C.create_string_buffer(bytes(fill), record_stride)
        return check(_lib.lib().srpc_gpu_unpack_aos_fill(self._h, _dptr(wire), wire_len, n, _dptr(records),
                                                         record_stride, self._offsets(field_offsets), buf,
                                                         _dptr(status), _stream(stream)),
                     "srpc_gpu_unpack_aos_fill")

    # -- string schemas (SRPC_PATH_VAR) -------------------------------------
    def var_scratch_bytes(self, n: int, wire_bytes: int) -> int:
        """Device scratch for pack_var (wire_bytes = wire_cap) / unpack_var (= wire_len)."""
        out = C.c_uint64()
        check(_lib.lib().srpc_plan_var_scratch_bytes(self._h, n, wire_bytes, C.byref(out)),
              "srpc_plan_var_scratch_bytes")
        return out.value

    def _str_offs(self, str_offs: Sequence) -> C.Array:
        ptrs = [_dptr(o) if (o is not None and k == STRING) else 0
                for o, k in zip(str_offs, self.schema.kinds)]
        return (C.c_void_p * len(ptrs))(*ptrs)

    def pack_var(self, cols: Sequence, str_offs: Sequence, n: int, wire, wire_cap: int, rec_offs,
                 scratch, scratch_bytes: int, status=None, stream=None) -> None:
        """Pack n records with string fields; writes rec_offs[0..n] (async).
        ``str_offs[f]``: n+1 u64 device offsets for string fields, None otherwise."""
        check(_lib.lib().srpc_gpu_pack_var(self._h, self._cols(cols), self._str_offs(str_offs), n,
                                           _dptr(wire), wire_cap, _dptr(rec_offs), _dptr(status),
                                           _dptr(scratch), scratch_bytes, _stream(stream)),
              "srpc_gpu_pack_var")

    def unpack_var(self, wire, wire_len: int, n: int, rec_offs, cols: Sequence, str_offs: Sequence,
                   scratch, scratch_bytes: int, status=None, stream=None) -> None:
        """Unpack n records whose starts are rec_offs[0..n] (async).  String
        field f's chars go to cols[f] (room for wire_len bytes), its n+1
        offsets to str_offs[f]."""
        check(_lib.lib().srpc_gpu_unpack_var(self._h, _dptr(wire), wire_len, n, _dptr(rec_offs),
                                             self._cols(cols), self._str_offs(str_offs),
                                             _dptr(status), _dptr(scratch), scratch_bytes,
                                             _stream(stream)),
              "srpc_gpu_unpack_var")

    def var_tile_table_words(self, n: int) -> int:
        """u64 words of a batch's tile table (srpc_gpu_var_tile_table)."""
        out = C.c_uint64()
        check(_lib.lib().srpc_var_tile_table_words(self._h, n, C.byref(out)), "srpc_var_tile_table_words")
        return out.value

    def var_tile_table(self, str_offs: Sequence, n: int, table, stream=None) -> None:
        """The tile table of n records from their string offsets (async)."""
        check(_lib.lib().srpc_gpu_var_tile_table(self._h, self._str_offs(str_offs), n, _dptr(table), _stream(stream)),
              "srpc_gpu_var_tile_table")

    def unpack_var_tiled(self, wire, wire_len: int, n: int, rec_offs, table, cols: Sequence, str_offs: Sequence,
                         scratch, scratch_bytes: int, status=None, stream=None) -> None:
        """unpack_var with the batch's tile table (output bases without the look-back)."""
        check(_lib.lib().srpc_gpu_unpack_var_tiled(self._h, _dptr(wire), wire_len, n, _dptr(rec_offs), _dptr(table),
                                                   self._cols(cols), self._str_offs(str_offs), _dptr(status),
                                                   _dptr(scratch), scratch_bytes, _stream(stream)),
              "srpc_gpu_unpack_var_tiled")

    def var_stream_scratch_bytes(self, n: int, wire_len: int) -> int:
        """Device scratch for unpack_var_stream (256-byte aligned)."""
        out = C.c_uint64()
        check(_lib.lib().srpc_plan_var_stream_scratch_bytes(self._h, n, wire_len, C.byref(out)),
              "srpc_plan_var_stream_scratch_bytes")
        return out.value

    def unpack_var_stream(self, wire, wire_len: int, n: int, rec_offs, cols: Sequence, str_offs: Sequence,
                          scratch, scratch_bytes: int, status=None, stream=None) -> None:
        """Unpack n records from a concatenated stream with no index (the
        reference's shared-cursor decode); writes rec_offs[0..n] (async).
        The wire needs no alignment.  When record e is the first the cursor
        cannot read, nothing of it is decoded: rec_offs[e+1..n] == wire_len
        and str_offs[f][e+1..n] == str_offs[f][e] (srpc_gpu.h)."""
        check(_lib.lib().srpc_gpu_unpack_var_stream(self._h, _dptr(wire), wire_len, n, _dptr(rec_offs),
                                                    self._cols(cols), self._str_offs(str_offs),
                                                    _dptr(status), _dptr(scratch), scratch_bytes,
                                                    _stream(stream)),
              "srpc_gpu_unpack_var_stream")

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().srpc_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fill_splitmix_i32(cols: Iterable, n: int, seed: int, first_record: int = 0, stream=None) -> None:
    """Synthetic int32 columns on the device (SURVEY.md §8c splitmix64 stream)."""
    ptrs = [_dptr(c) for c in cols]
    arr = (C.c_void_p * len(ptrs))(*ptrs)
    check(_lib.lib().srpc_gpu_fill_splitmix_i32(arr, len(ptrs), n, seed, first_record,
                                                _stream(stream)), "srpc_gpu_fill_splitmix_i32")


def time_next_call(start=None, stop=None) -> None:
    """Arm srpc_time_next_call: the kernels of the next pack/unpack call made
    on this thread stamp their dispatch begin (first kernel) and end (last
    kernel) into ``start`` / ``stop``.  Each is a torch.cuda.Event created
    with enable_timing=True and recorded at least once (torch creates the HIP
    event lazily, on first record), or a raw hipEvent_t handle."""
    def handle(e):
        if e is None:
            return None
        if hasattr(e, "cuda_event"):
            if not e.cuda_event:
                raise ValueError("time_next_call: record the event once first (torch creates it lazily)")
            return e.cuda_event
        return int(e)

    check(_lib.lib().srpc_time_next_call(handle(start), handle(stop)), "srpc_time_next_call")


def framed_request_prefix(schema: Schema, method: str) -> bytes:
    """``BE32 payload | str(method) | str(T::name)``: the constant head of every
    frame Calculator_stub-style clients send for a fixed-size request
    (transport.hpp send_data + packer.hpp:77-82)."""
    pre = request_prefix(method, schema.name)
    return struct.pack(">I", len(pre) + schema.body_bytes) + pre


def framed_response_prefix(schema: Schema, code: int = RPC_SUCCESS) -> bytes:
    pre = response_prefix(code, schema.name)
    return struct.pack(">I", len(pre) + schema.body_bytes) + pre


def frame_var(records, rec_offs, n: int, out, out_cap: int, status=None, stream=None) -> None:
    """Frame the n records ``pack_var`` wrote (``rec_offs``: its record index)
    for the socket: ``BE32(len_j) | record j`` at out + rec_offs[j] + 4 j (async)."""
    check(_lib.lib().srpc_frames_frame_var(_dptr(records), _dptr(rec_offs), n, _dptr(out), out_cap, _dptr(status),
                                           _stream(stream)), "srpc_frames_frame_var")


class FrameClassifier:
    """Buckets a batch of socket frames by method on the device
    (srpc_frames_classify / _gather / _scatter): ``methods`` is a list of
    (request GpuPacker with a framed prefix, response record bytes)."""

    def __init__(self, methods: Sequence[tuple["GpuPacker", int]]):
        self.methods = list(methods)
        k = len(self.methods)
        self._plans = (C.c_void_p * k)(*[m[0]._h.value for m in self.methods])
        self._rb = (C.c_uint32 * k)(*[int(m[1]) for m in self.methods])

    def scratch_bytes(self, nframes: int) -> int:
        out = C.c_uint64()
        check(_lib.lib().srpc_frames_scratch_bytes(nframes, len(self.methods), C.byref(out)),
              "srpc_frames_scratch_bytes")
        return out.value

    def classify(self, buf, buf_len: int, offs, nframes: int, cls, index, counts, out_off, scratch,
                 scratch_bytes: int, stream=None) -> None:
        check(_lib.lib().srpc_frames_classify(self._plans, self._rb, len(self.methods), _dptr(buf), buf_len,
                                              _dptr(offs), nframes, _dptr(cls), _dptr(index), _dptr(counts),
                                              _dptr(out_off), _dptr(scratch), scratch_bytes, _stream(stream)),
              "srpc_frames_classify")

    @staticmethod
    def gather(buf, offs, index, n: int, record_bytes: int, out, stream=None) -> None:
        check(_lib.lib().srpc_frames_gather(_dptr(buf), _dptr(offs), _dptr(index), n, record_bytes, _dptr(out),
                                            _stream(stream)), "srpc_frames_gather")

    @staticmethod
    def scatter(resp, index, n: int, record_bytes: int, out_off, out, stream=None) -> None:
        check(_lib.lib().srpc_frames_scatter(_dptr(resp), _dptr(index), n, record_bytes, _dptr(out_off),
                                             _dptr(out), _stream(stream)), "srpc_frames_scatter")

    # string plans (request GpuPackers built with request_prefix, no BE32):
    @staticmethod
    def gather_var(buf, offs, index, n: int, out, rec_offs, scratch, scratch_bytes: int, stream=None) -> None:
        check(_lib.lib().srpc_frames_gather_var(_dptr(buf), _dptr(offs), _dptr(index), n, _dptr(out), _dptr(rec_offs),
                                                _dptr(scratch), scratch_bytes, _stream(stream)),
              "srpc_frames_gather_var")

    @staticmethod
    def scatter_var(resp, rec_offs, index, n: int, out_off, out, stream=None) -> None:
        check(_lib.lib().srpc_frames_scatter_var(_dptr(resp), _dptr(rec_offs), _dptr(index), n, _dptr(out_off),
                                                 _dptr(out), _stream(stream)), "srpc_frames_scatter_var")

    def offsets(self, cls, nframes: int, index, counts, var_rec_offs, out_off, total, scratch, scratch_bytes: int,
                stream=None) -> None:
        """var_rec_offs: per method, the response index of a string method's
        bucket (device buffer) or None for a fixed one."""
        k = len(self.methods)
        vr = (C.c_void_p * k)(*[_dptr(v) if v is not None else None for v in var_rec_offs])
        check(_lib.lib().srpc_frames_offsets(self._plans, self._rb, k, _dptr(cls), nframes, _dptr(index), _dptr(counts),
                                             vr, _dptr(out_off), _dptr(total), _dptr(scratch), scratch_bytes,
                                             _stream(stream)), "srpc_frames_offsets")


class MixedFrames:
    """A batch of calls of several fixed-size methods in call order
    (srpc_frames_mixed_index / _pack_requests_mixed / _unpack_replies_mixed):
    ``plans`` are GpuPackers with framed prefixes, request plans for ``pack``,
    reply plans for ``unpack``.  Every call returns the C status (negative:
    refused, nothing launched)."""

    def __init__(self, plans: Sequence["GpuPacker"]):
        self.plans = list(plans)
        self.k = len(self.plans)
        self._plans = (C.c_void_p * self.k)(*[p._h.value for p in self.plans])

    @staticmethod
    def index_bytes(ncalls: int, nplans: int) -> int:
        out = C.c_uint64()
        check(_lib.lib().srpc_frames_mixed_index_bytes(ncalls, nplans, C.byref(out)), "srpc_frames_mixed_index_bytes")
        return out.value

    @staticmethod
    def index(method, ncalls: int, nplans: int, index, index_bytes: int, counts, status=None, stream=None) -> int:
        return _lib.lib().srpc_frames_mixed_index(_dptr(method), ncalls, nplans, _dptr(index), index_bytes,
                                                  _dptr(counts), _dptr(status), _stream(stream))

    @staticmethod
    def ranks(index, method, ncalls: int, nplans: int, rank, stream=None) -> int:
        return _lib.lib().srpc_frames_mixed_ranks(_dptr(index), _dptr(method), ncalls, nplans, _dptr(rank),
                                                  _stream(stream))

    @property
    def tile(self) -> int:
        out = C.c_uint32()
        check(_lib.lib().srpc_frames_mixed_tile(self._plans, self.k, C.byref(out)), "srpc_frames_mixed_tile")
        return out.value

    def _args(self, cols, first, cap):
        self._keep = [(C.c_void_p * len(c))(*[_dptr(x) for x in c]) for c in cols]
        arr = (C.c_void_p * self.k)(*[C.cast(a, C.c_void_p).value for a in self._keep])
        h_first = None if first is None else (C.c_uint64 * self.k)(*[int(x) for x in first])
        h_cap = (C.c_uint64 * self.k)(*[int(x) for x in cap])
        return arr, h_first, h_cap

    def pack(self, cols, first, cap, method, index, ncalls: int, out, out_cap: int, offs=None, status=None,
             stream=None) -> int:
        """cols[k]: plan k's request columns; first / cap: per plan (first may be None)."""
        arr, h_first, h_cap = self._args(cols, first, cap)
        return _lib.lib().srpc_frames_pack_requests_mixed(self._plans, self.k, arr, h_first, h_cap, _dptr(method),
                                                          _dptr(index), ncalls, _dptr(out), out_cap, _dptr(offs),
                                                          _dptr(status), _stream(stream))

    def unpack(self, buf, buf_len: int, offs, nframes: int, method, index, ncalls: int, unanswered: int, cols, first,
               cap, codes, status=None, stream=None) -> int:
        arr, h_first, h_cap = self._args(cols, first, cap)
        return _lib.lib().srpc_frames_unpack_replies_mixed(self._plans, self.k, _dptr(buf), buf_len, _dptr(offs),
                                                           nframes, _dptr(method), _dptr(index), ncalls, unanswered,
                                                           arr, h_first, h_cap, _dptr(codes), _dptr(status),
                                                           _stream(stream))

    def unpack_requests(self, buf, buf_len: int, offs, nframes: int, cols, first, cap, cls, index, index_bytes: int,
                        counts, status=None, stream=None) -> int:
        """Server side (srpc_frames_unpack_requests_mixed): classify the frames
        against these request plans and decode each into its plan's columns at
        its arrival rank; ``cls``, ``index`` and ``counts`` are outputs."""
        arr, h_first, h_cap = self._args(cols, first, cap)
        return _lib.lib().srpc_frames_unpack_requests_mixed(self._plans, self.k, _dptr(buf), buf_len, _dptr(offs),
                                                            nframes, arr, h_first, h_cap, _dptr(cls), _dptr(index),
                                                            index_bytes, _dptr(counts), _dptr(status),
                                                            _stream(stream))


class MixedAosFrames:
    """``MixedFrames.pack`` / ``unpack`` with one device array of structs per
    plan in place of its columns (srpc_frames_pack_requests_mixed_aos /
    _unpack_replies_mixed_aos; the index is ``MixedFrames.index``), and the
    server's ``unpack_requests`` (srpc_frames_unpack_requests_mixed_aos).
    ``strides[k]``: plan k's struct bytes, ``leaf_offsets[k][f]``: the byte
    offset of leaf f in it.  Every call returns the C status (negative: refused,
    nothing launched)."""

    def __init__(self, plans: Sequence["GpuPacker"], strides: Sequence[int], leaf_offsets: Sequence[Sequence[int]]):
        self.plans = list(plans)
        self.k = len(self.plans)
        self._plans = (C.c_void_p * self.k)(*[p._h.value for p in self.plans])
        self._strides = (C.c_uint64 * self.k)(*[int(s) for s in strides])
        self._keep_offs = [(C.c_uint32 * max(1, len(o)))(*[int(x) for x in o]) for o in leaf_offsets]
        self._offs = (C.c_void_p * self.k)(*[C.cast(a, C.c_void_p).value for a in self._keep_offs])

    @property
    def scratch_bytes(self) -> int:
        out = C.c_uint64()
        check(_lib.lib().srpc_frames_mixed_aos_scratch_bytes(self._plans, self.k, self._strides, C.byref(out)),
              "srpc_frames_mixed_aos_scratch_bytes")
        return out.value

    @property
    def tile(self) -> int:
        """Calls per workgroup tile of ``unpack`` and of ``unpack_requests``'s decode
        (``pack`` tiles as ``MixedFrames.tile``)."""
        out = C.c_uint32()
        check(_lib.lib().srpc_frames_mixed_aos_tile(self._plans, self.k, self._strides, C.byref(out)),
              "srpc_frames_mixed_aos_tile")
        return out.value

    def _args(self, recs, first, cap):
        arr = (C.c_void_p * self.k)(*[_dptr(r) for r in recs])
        h_first = None if first is None else (C.c_uint64 * self.k)(*[int(x) for x in first])
        h_cap = (C.c_uint64 * self.k)(*[int(x) for x in cap])
        return arr, h_first, h_cap

    def pack(self, recs, first, cap, method, index, ncalls: int, out, out_cap: int, offs=None, status=None,
             stream=None) -> int:
        """recs[k]: plan k's request structs; first / cap: per plan, in structs (first may be None)."""
        arr, h_first, h_cap = self._args(recs, first, cap)
        return _lib.lib().srpc_frames_pack_requests_mixed_aos(self._plans, self.k, arr, self._strides, self._offs,
                                                              h_first, h_cap, _dptr(method), _dptr(index), ncalls,
                                                              _dptr(out), out_cap, _dptr(offs), _dptr(status),
                                                              _stream(stream))

    def unpack(self, buf, buf_len: int, offs, nframes: int, method, index, ncalls: int, unanswered: int, recs, fills,
               first, cap, codes, scratch, scratch_bytes: int, status=None, stream=None) -> int:
        """recs[k]: plan k's reply structs; fills[k]: ``strides[k]`` host bytes for what no leaf covers."""
        arr, h_first, h_cap = self._args(recs, first, cap)
        keep = [C.create_string_buffer(bytes(f), max(1, len(bytes(f)))) for f in fills]
        h_fill = (C.c_void_p * self.k)(*[C.cast(b, C.c_void_p).value for b in keep])
        return _lib.lib().srpc_frames_unpack_replies_mixed_aos(self._plans, self.k, _dptr(buf), buf_len, _dptr(offs),
                                                               nframes, _dptr(method), _dptr(index), ncalls, unanswered,
                                                               arr, self._strides, self._offs, h_fill, h_first, h_cap,
                                                               _dptr(codes), _dptr(status), _dptr(scratch),
                                                               scratch_bytes, _stream(stream))

    def unpack_requests(self, buf, buf_len: int, offs, nframes: int, recs, fills, first, cap, cls, index,
                        index_bytes: int, counts, scratch, scratch_bytes: int, status=None, stream=None) -> int:
        """Server side (srpc_frames_unpack_requests_mixed_aos): classify the
        frames against these request plans and decode each into element
        ``first[k] + rank`` of ``recs[k]``, its plan's request structs, bytes no
        leaf covers from ``fills[k]``; ``cls``, ``index`` and ``counts`` are
        outputs.  The ordered reply pack is ``pack`` of the response plans'
        MixedAosFrames with ``method=cls`` and this ``index``."""
        arr, h_first, h_cap = self._args(recs, first, cap)
        keep = [C.create_string_buffer(bytes(f), max(1, len(bytes(f)))) for f in fills]
        h_fill = (C.c_void_p * self.k)(*[C.cast(b, C.c_void_p).value for b in keep])
        return _lib.lib().srpc_frames_unpack_requests_mixed_aos(self._plans, self.k, _dptr(buf), buf_len, _dptr(offs),
                                                                nframes, arr, self._strides, self._offs, h_fill, h_first,
                                                                h_cap, _dptr(cls), _dptr(index), index_bytes,
                                                                _dptr(counts), _dptr(status), _dptr(scratch),
                                                                scratch_bytes, _stream(stream))


class MixedVarFrames:
    """A batch of calls of several methods in call order, string-bodied ones
    included (srpc_frames_pack_requests_mixed_var / _unpack_replies_mixed_var;
    the index is ``MixedFrames.index``).  ``plans``: GpuPackers -- a fixed-size
    one with a framed prefix, a string one with the unframed prefix
    (``request_prefix`` / ``response_prefix``).  ``cols[k]`` are plan k's
    columns, ``str_offs[k]`` its per-leaf offsets arrays (None for fixed leaves;
    None for a fixed plan).  Every call returns the C status (negative: refused,
    nothing launched)."""

    def __init__(self, plans: Sequence["GpuPacker"]):
        self.plans = list(plans)
        self.k = len(self.plans)
        self._plans = (C.c_void_p * self.k)(*[p._h.value for p in self.plans])

    def scratch_bytes(self, ncalls: int) -> int:
        out = C.c_uint64()
        check(_lib.lib().srpc_frames_mixed_var_scratch_bytes(self._plans, self.k, ncalls, C.byref(out)),
              "srpc_frames_mixed_var_scratch_bytes")
        return out.value

    @property
    def tile(self) -> tuple[int, int]:
        """(calls per workgroup tile, bytes of its LDS image window)."""
        t, img = C.c_uint32(), C.c_uint32()
        check(_lib.lib().srpc_frames_mixed_var_tile(self._plans, self.k, C.byref(t), C.byref(img)),
              "srpc_frames_mixed_var_tile")
        return t.value, img.value

    def _table(self, rows, conv, ctype):
        keep = [None if r is None else (ctype * len(r))(*[conv(x) for x in r]) for r in rows]
        arr = (C.c_void_p * self.k)(*[None if a is None else C.cast(a, C.c_void_p).value for a in keep])
        return arr, keep

    def _args(self, cols, str_offs, first, cap):
        c_arr, k1 = self._table(cols, _dptr, C.c_void_p)
        s_arr, k2 = self._table(str_offs, lambda x: None if x is None else _dptr(x), C.c_void_p)
        self._keep = (k1, k2)
        h_first = None if first is None else (C.c_uint64 * self.k)(*[int(x) for x in first])
        h_cap = (C.c_uint64 * self.k)(*[int(x) for x in cap])
        return c_arr, s_arr, h_first, h_cap

    def pack(self, cols, str_offs, first, cap, method, index, ncalls: int, out, out_cap: int, offs, total, status,
             scratch, scratch_bytes: int, stream=None) -> int:
        c_arr, s_arr, h_first, h_cap = self._args(cols, str_offs, first, cap)
        return _lib.lib().srpc_frames_pack_requests_mixed_var(self._plans, self.k, c_arr, s_arr, h_first, h_cap,
                                                              _dptr(method), _dptr(index), ncalls, _dptr(out), out_cap,
                                                              _dptr(offs), _dptr(total), _dptr(status), _dptr(scratch),
                                                              scratch_bytes, _stream(stream))

    def unpack(self, buf, buf_len: int, offs, nframes: int, method, index, ncalls: int, unanswered: int, cols,
               str_offs, str_cap, first, cap, codes, ends, status, scratch, scratch_bytes: int, stream=None) -> int:
        """str_cap[k]: per leaf, the bytes a string column has (ignored for fixed
        leaves; None for a fixed plan)."""
        c_arr, s_arr, h_first, h_cap = self._args(cols, str_offs, first, cap)
        cap_arr, k3 = self._table(str_cap, lambda x: 0 if x is None else int(x), C.c_uint64)
        self._keep += (k3,)
        return _lib.lib().srpc_frames_unpack_replies_mixed_var(self._plans, self.k, _dptr(buf), buf_len, _dptr(offs),
                                                               nframes, _dptr(method), _dptr(index), ncalls, unanswered,
                                                               c_arr, s_arr, cap_arr, h_first, h_cap, _dptr(codes),
                                                               _dptr(ends), _dptr(status), _dptr(scratch),
                                                               scratch_bytes, _stream(stream))

    def unpack_requests(self, buf, buf_len: int, offs, nframes: int, cols, str_offs, str_cap, first, cap, cls, index,
                        index_bytes: int, counts, ends, status, scratch, scratch_bytes: int, stream=None) -> int:
        """Server side (srpc_frames_unpack_requests_mixed_var): classify the
        frames against these request plans and decode each into its plan's
        columns at its arrival rank; ``cls``, ``index``, ``counts`` and ``ends``
        are outputs.  The ordered reply pack is ``pack`` of the response plans'
        MixedVarFrames with ``method=cls`` and this ``index``."""
        c_arr, s_arr, h_first, h_cap = self._args(cols, str_offs, first, cap)
        cap_arr, k3 = self._table(str_cap, lambda x: 0 if x is None else int(x), C.c_uint64)
        self._keep += (k3,)
        return _lib.lib().srpc_frames_unpack_requests_mixed_var(self._plans, self.k, _dptr(buf), buf_len, _dptr(offs),
                                                                nframes, c_arr, s_arr, cap_arr, h_first, h_cap,
                                                                _dptr(cls), _dptr(index), index_bytes, _dptr(counts),
                                                                _dptr(ends), _dptr(status), _dptr(scratch),
                                                                scratch_bytes, _stream(stream))


class MixedLegFrames(MixedVarFrames):
    """``MixedVarFrames.pack`` / ``unpack`` with, per plan, the choice between
    columns and one device array of the caller's structs
    (srpc_frames_pack_requests_mixed_legs / _unpack_replies_mixed_legs; the
    index is ``MixedFrames.index``), and the server's ``unpack_requests``
    (srpc_frames_unpack_requests_mixed_legs).  ``strides[k]``: plan k's struct bytes, or 0
    for a plan held in columns (fixed-size or string); ``leaf_offsets[k][f]``:
    the byte offset of leaf f in the struct (None for a column plan).
    ``cols[k]`` / ``str_offs[k]`` / ``str_cap[k]`` are ``MixedVarFrames``'s and
    may be None for a record plan; ``recs[k]`` / ``fills[k]`` are
    ``MixedAosFrames``'s and may be None for a column plan.  Every call returns
    the C status (negative: refused, nothing launched)."""

    def __init__(self, plans: Sequence["GpuPacker"], strides: Sequence[int],
                 leaf_offsets: Sequence[Optional[Sequence[int]]]):
        super().__init__(plans)
        self.strides = [int(s) for s in strides]
        self._strides = (C.c_uint64 * self.k)(*self.strides)
        self._keep_offs = [None if o is None else (C.c_uint32 * max(1, len(o)))(*[int(x) for x in o])
                           for o in leaf_offsets]
        self._offs = (C.c_void_p * self.k)(*[None if a is None else C.cast(a, C.c_void_p).value
                                             for a in self._keep_offs])

    def scratch_bytes(self, ncalls: int) -> int:
        out = C.c_uint64()
        check(_lib.lib().srpc_frames_mixed_legs_scratch_bytes(self._plans, self.k, self._strides, ncalls,
                                                              C.byref(out)), "srpc_frames_mixed_legs_scratch_bytes")
        return out.value

    @property
    def tile(self) -> tuple[int, int]:
        """(calls per workgroup tile of ``unpack``, bytes of its LDS image window);
        ``pack`` tiles as ``MixedVarFrames.tile``."""
        t, img = C.c_uint32(), C.c_uint32()
        check(_lib.lib().srpc_frames_mixed_legs_tile(self._plans, self.k, self._strides, C.byref(t), C.byref(img)),
              "srpc_frames_mixed_legs_tile")
        return t.value, img.value

    def _recs(self, recs):
        return (C.c_void_p * self.k)(*[None if r is None else _dptr(r) for r in recs])

    def pack(self, cols, str_offs, recs, first, cap, method, index, ncalls: int, out, out_cap: int, offs, total,
             status, scratch, scratch_bytes: int, stream=None) -> int:
        c_arr, s_arr, h_first, h_cap = self._args(cols, str_offs, first, cap)
        return _lib.lib().srpc_frames_pack_requests_mixed_legs(self._plans, self.k, c_arr, s_arr, self._recs(recs),
                                                               self._strides, self._offs, h_first, h_cap,
                                                               _dptr(method), _dptr(index), ncalls, _dptr(out), out_cap,
                                                               _dptr(offs), _dptr(total), _dptr(status),
                                                               _dptr(scratch), scratch_bytes, _stream(stream))

    def unpack(self, buf, buf_len: int, offs, nframes: int, method, index, ncalls: int, unanswered: int, cols,
               str_offs, str_cap, recs, fills, first, cap, codes, ends, status, scratch, scratch_bytes: int,
               stream=None) -> int:
        c_arr, s_arr, h_first, h_cap = self._args(cols, str_offs, first, cap)
        cap_arr, k3 = self._table(str_cap, lambda x: 0 if x is None else int(x), C.c_uint64)
        keep = [None if f is None else C.create_string_buffer(bytes(f), max(1, len(bytes(f)))) for f in fills]
        h_fill = (C.c_void_p * self.k)(*[None if b is None else C.cast(b, C.c_void_p).value for b in keep])
        self._keep += (k3, keep)
        return _lib.lib().srpc_frames_unpack_replies_mixed_legs(self._plans, self.k, _dptr(buf), buf_len, _dptr(offs),
                                                                nframes, _dptr(method), _dptr(index), ncalls,
                                                                unanswered, c_arr, s_arr, cap_arr, self._recs(recs),
                                                                self._strides, self._offs, h_fill, h_first, h_cap,
                                                                _dptr(codes), _dptr(ends), _dptr(status),
                                                                _dptr(scratch), scratch_bytes, _stream(stream))

    def unpack_requests(self, buf, buf_len: int, offs, nframes: int, cols, str_offs, str_cap, recs, fills, first, cap,
                        cls, index, index_bytes: int, counts, ends, status, scratch, scratch_bytes: int,
                        stream=None) -> int:
        """Server side (srpc_frames_unpack_requests_mixed_legs): classify the
        frames against these request plans and decode each at its arrival rank
        into its plan's columns, or into element ``first[k] + rank`` of
        ``recs[k]`` for a record plan, bytes no leaf covers from ``fills[k]``;
        ``cls``, ``index``, ``counts`` and ``ends`` are outputs.  The ordered
        reply pack is ``pack`` of the response plans' MixedLegFrames with
        ``method=cls`` and this ``index``."""
        c_arr, s_arr, h_first, h_cap = self._args(cols, str_offs, first, cap)
        cap_arr, k3 = self._table(str_cap, lambda x: 0 if x is None else int(x), C.c_uint64)
        keep = [None if f is None else C.create_string_buffer(bytes(f), max(1, len(bytes(f)))) for f in fills]
        h_fill = (C.c_void_p * self.k)(*[None if b is None else C.cast(b, C.c_void_p).value for b in keep])
        self._keep += (k3, keep)
        return _lib.lib().srpc_frames_unpack_requests_mixed_legs(self._plans, self.k, _dptr(buf), buf_len, _dptr(offs),
                                                                 nframes, c_arr, s_arr, cap_arr, self._recs(recs),
                                                                 self._strides, self._offs, h_fill, h_first, h_cap,
                                                                 _dptr(cls), _dptr(index), index_bytes, _dptr(counts),
                                                                 _dptr(ends), _dptr(status), _dptr(scratch),
                                                                 scratch_bytes, _stream(stream))


__all__ = ["Schema", "GpuPacker", "SrpcError", "request_prefix", "response_prefix",
           "fill_splitmix_i32", "time_next_call", "framed_request_prefix", "framed_response_prefix",
           "FrameClassifier", "frame_var", "MixedFrames", "MixedVarFrames", "MixedLegFrames", "BOOL", "INT8", "CHAR", "INT16", "INT32", "INT64", "STRING",
           "RPC_SUCCESS", "RPC_ERR_FUNCTION_NOT_REGISTERED", "RPC_ERR_RECV_TIMEOUT"]
