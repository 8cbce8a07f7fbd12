/*
 * srpc_gpu.h -- C ABI of the MI355X (gfx950) batched sRPC packer.
 *
 * This is the drop-in boundary for the reference's packer hot path.  The
 * reference has no FFI of its own: its "operator API" is the header-only C++
 * template surface of namespace srpc (include/srpc/packer.hpp:53-181).  Each
 * entry point below replaces a loop over one of those calls with one batched,
 * stream-ordered launch over N records:
 *
 *   srpc_gpu_pack    <- `packer p; for (r : batch) p << r;`
 *                       (packer.hpp:73 -> pack_arg 183-191 -> pack_struct 172-178),
 *                       and, with a request/response prefix, the loops over
 *                       pack_request (packer.hpp:77-82) / pack_response (86-91)
 *   srpc_gpu_unpack  <- `for (r : batch) r.unpack(bp);` (generated unpack,
 *                       examples/calculator_srpc.cpp:19-22, calling
 *                       packer::operator>> 70 -> pipe_output 210-222), and,
 *                       with a prefix, unpack_request / unpack_response / getv
 *                       (packer.hpp:95-162) for records of one known type
 *   srpc_plan_create <- the compile-time reflection over T::fields
 *                       (core.hpp:9-14, STRUCT_MEMBER) that fixes field order
 *                       and sizes; the C++ side (include/srpc/gpu.hpp) builds
 *                       the descriptor from T::fields automatically.
 *
 * Wire bytes are identical to the reference's: raw little-endian fields in
 * declaration order, no padding, nested messages inlined, strings as a u64
 * length followed by the bytes, records back to back.
 *
 * Conventions
 *   - All data pointers are DEVICE pointers (hipMalloc'd) unless named h_*.
 *     The library allocates nothing on the pack/unpack hot path.
 *   - `stream` is a hipStream_t (NULL = the default stream).  Calls are
 *     asynchronous and stream-ordered; they are safe to capture in a hipGraph.
 *   - Return values: 0 = launched; <0 = argument / HIP error (nothing launched);
 *     >0 = a data error detected on the host (see SRPC_ERR_*).  No exception
 *     ever crosses this ABI (the reference terminates instead: core.hpp:28-33
 *     throws inside noexcept functions).
 *   - Threading: a plan is immutable after creation and may be used from any
 *     host thread and on any stream of its device concurrently.
 */
#ifndef SRPC_GPU_H
#define SRPC_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRPC_GPU_ABI_VERSION 8

/* Field kinds = the IDL type table of the reference (parser.hpp:253-290).
 * Nested message fields are flattened into their members by the caller. */
typedef enum srpc_kind {
    SRPC_KIND_BOOL = 1,   /* bool    : 1 byte               */
    SRPC_KIND_INT8 = 2,   /* int8_t  : 1 byte               */
    SRPC_KIND_CHAR = 3,   /* char    : 1 byte               */
    SRPC_KIND_INT16 = 4,  /* int16_t : 2 bytes LE           */
    SRPC_KIND_INT32 = 5,  /* int32_t : 4 bytes LE           */
    SRPC_KIND_INT64 = 6,  /* int64_t : 8 bytes LE           */
    SRPC_KIND_STRING = 7  /* u64 LE length + raw bytes      */
} srpc_kind;

/* Return codes. */
#define SRPC_OK 0
#define SRPC_E_INVALID (-1)     /* bad argument or schema                       */
#define SRPC_E_ALIGN (-2)       /* a device pointer violates the alignment rule */
#define SRPC_E_HIP (-3)         /* HIP runtime / launch failure                 */
#define SRPC_E_UNSUPPORTED (-4) /* no kernel for this schema / layout; chunked host call in a capture */
#define SRPC_E_CAPACITY (-5)    /* output buffer too small                      */
#define SRPC_ERR_BOUNDS 2       /* wire shorter than n records; the records that
                                   fit were decoded, the status says where the
                                   first missing one starts                      */

/* Device-side decode status bits (srpc_unpack_status.flags). */
#define SRPC_STATUS_PREFIX 1u   /* a record's envelope header != the plan's prefix */
#define SRPC_STATUS_BOUNDS 2u   /* a record (or string) ran past the wire end      */
#define SRPC_STATUS_STALLED 4u  /* srpc_gpu_unpack_var, several string fields: a
                                   tile's chars-offset look-back polled its
                                   predecessors past its budget (2^21 polls of
                                   one word, ~1 s: only a device shared with
                                   kernels that keep every earlier tile from
                                   being scheduled).  The outputs are not valid;
                                   retry the call.  The stream decode
                                   (srpc_gpu_unpack_var_stream) never waits and
                                   never reports it. */

/* Written by srpc_gpu_unpack when its d_status argument is non-NULL.
 * Reset by the call itself (stream-ordered) before decoding starts. */
typedef struct srpc_unpack_status {
    uint32_t flags;             /* OR of SRPC_STATUS_* over the batch          */
    uint32_t reserved;          /* diagnostics of srpc_gpu_unpack_var_stream: bit 0 =
                                   the cursor entered some block at a table slot
                                   other than the block's speculated start, bit 1 =
                                   it entered some block where no table slot was
                                   (that block was walked record by record),
                                   bit 2 = the first scan met such a position and
                                   the repair pass gave every block exit slots,
                                   bit 3 = some block had more possible entries
                                   than its exit slots hold (those may walk),
                                   bits 8-31 = scan waves that walked (saturating);
                                   0 from every other call                     */
    uint64_t first_bad_record;  /* smallest failing record index, or UINT64_MAX */
} srpc_unpack_status;

/* A flat record schema: fields in T::fields declaration order
 * (packer.hpp:172-178), plus an optional constant per-record header: the
 * `u64 len | method | u64 len | T::name` of pack_request, or the
 * `u8 code | u64 len | T::name` of pack_response. */
typedef struct srpc_schema_desc {
    uint32_t nfields;
    const int32_t* kinds;   /* host array of nfields srpc_kind values */
    const uint8_t* prefix;  /* host bytes, may be NULL when prefix_len == 0 */
    uint32_t prefix_len;
} srpc_schema_desc;

typedef struct srpc_plan srpc_plan;

/* Which kernel family a plan runs (srpc_plan_info). */
#define SRPC_PATH_DWORD 1   /* every field 4/8 B, no prefix, record <= 32 B:
                               one record per lane, register-assembled records          */
#define SRPC_PATH_TILE 2    /* any fixed-size schema: LDS-staged tiles, 16 B global I/O  */
#define SRPC_PATH_VAR 3     /* string fields: per-record sizes + wavefront/device scan   */

/* Validate a schema and prepare its kernels on `device` (allocates the
 * plan's small device-side prefix copy; never called on the hot path).
 * Limits of this build (the reference's pack_struct has none, packer.hpp:
 * 172-178): at most SRPC_MAX_FIELDS leaf fields after flattening and an
 * envelope prefix of at most SRPC_MAX_PREFIX bytes -- so a fixed record is at
 * most 1024 + 32 * 8 = 1280 bytes.  A schema past a limit is refused with
 * SRPC_E_UNSUPPORTED before any device work; nfields == 0, an unknown kind or
 * a NULL pointer is SRPC_E_INVALID.  (srpc::gpu::batch_packer<T> throws
 * srpc::gpu::plan_error carrying the code.) */
#define SRPC_MAX_FIELDS 32
#define SRPC_MAX_PREFIX 1024
int srpc_plan_create(const srpc_schema_desc* desc, int device, srpc_plan** out);
int srpc_plan_destroy(srpc_plan* plan);

/* Fixed wire bytes per record (prefix included); 0 for string schemas. */
int srpc_plan_record_bytes(const srpc_plan* plan, uint64_t* out);
/* Kernel family in use (SRPC_PATH_*). */
int srpc_plan_path(const srpc_plan* plan, int* out);
/* Testing hook: force a kernel family the schema is eligible for
 * (SRPC_PATH_TILE is valid for every fixed schema). */
int srpc_plan_force_path(srpc_plan* plan, int path);

/* Performance knobs (defaults are the measured best on
 * MI355X; results are identical for every setting). */
#define SRPC_TUNE_RECORDS_PER_LANE 1 /* 1 or 4 (4: 16-byte column loads, needs 4-byte
                                        fields and 16-byte aligned columns) */
#define SRPC_TUNE_ITER 2             /* records (or quads) per lane per launch: 1,2,4,8 */
#define SRPC_TUNE_NONTEMPORAL 3      /* bit0 non-temporal stores, bit1 loads      */
#define SRPC_TUNE_TILE_BYTES 4       /* TILE path: target LDS image bytes per tile
                                        (1024..49152), pack and unpack           */
#define SRPC_TUNE_WAVE_PACK_BYTES 11   /* TILE path: pack with one wave per tile of about this
                                         many image bytes (0 = workgroup tiles)        */
#define SRPC_TUNE_WAVE_UNPACK_BYTES 12 /* TILE path: the same for unpack                */
#define SRPC_TUNE_PACK_TILE_BYTES 9  /* TILE path: the same for the pack kernel only */
#define SRPC_TUNE_VAR_KERNEL 7       /* VAR: 1 = record tiles, one pass (default; unpack of
                                        records under 40 bytes on average keeps 0), 0 =
                                        offset scans + chunk walks, 2 = record tiles for
                                        every unpack */
#define SRPC_TUNE_VAR_IMAGE_BYTES 8  /* VAR record tiles: LDS image bytes (8192..65536,
                                        multiple of 16); larger tiles take the walk  */
#define SRPC_TUNE_VAR_CHARS_BYTES 10 /* VAR record tiles: LDS chars stage bytes
                                        (0..65536, multiple of 16).  A schema whose
                                        image + stage + column slices pass a workgroup's
                                        LDS packs with the scan + chunk walk          */
#define SRPC_TUNE_REC_KERNEL 13      /* TILE path: schema-specialised kernels for the
                                        layouts that have one: 1 = in the directions
                                        where they measured faster (default), 2 = both
                                        directions, 0 = generic kernels only        */
#define SRPC_TUNE_GRID 5             /* DWORD path: max workgroups (0 = one per
                                        256*iter records; else grid-stride)       */
#define SRPC_TUNE_SWEEP 14           /* DWORD path: order in which a call walks its records.
                                        bit0: pack starts at the last record and walks
                                        down, bit1: unpack does (0..3).  A consumer that
                                        starts where its producer finished finds the
                                        producer's last lines still on die where the cache
                                        replaces least-recently-used lines first; measured
                                        neutral on MI355X with the default stores, so the
                                        default is 0.  Results are byte-identical for
                                        every value.                                 */
#define SRPC_TUNE_UNPACK_NONTEMPORAL 15 /* DWORD path: unpack's non-temporal bits alone
                                        (SRPC_TUNE_NONTEMPORAL sets pack's and unpack's) */
int srpc_plan_tune(srpc_plan* plan, int knob, int value);

/* Pack n records.  d_cols[f] (host array of nfields device pointers) holds
 * n elements of field f's C type, 4-byte aligned (16-byte for the TILE
 * path).  d_wire receives n * record_bytes bytes; wire_cap is its size.
 * d_wire must be 16-byte aligned. */
int srpc_gpu_pack(const srpc_plan* plan, const void* const* d_cols, uint64_t n,
                  uint8_t* d_wire, uint64_t wire_cap, void* stream);

/* Unpack n records from wire_len bytes at d_wire into the columns d_cols.
 * Every record's prefix is checked against the plan's; mismatches are
 * reported in *d_status (if non-NULL), and the record's fields are still
 * decoded from their fixed positions.  If wire_len < n * record_bytes the
 * records that fit are decoded and SRPC_ERR_BOUNDS is returned (status
 * flags BOUNDS, first_bad_record = wire_len / record_bytes). */
int srpc_gpu_unpack(const srpc_plan* plan, const uint8_t* d_wire, uint64_t wire_len,
                    uint64_t n, void* const* d_cols, srpc_unpack_status* d_status,
                    void* stream);

/* ---- fixed-size records held as the caller's own structs (AoS) -------------
 * The reference's caller holds std::vector<T> and loops `p << r`
 * (packer.hpp:73).  These take the struct array itself, copied to the device
 * as raw bytes: record r's leaf field f is at d_records + r * record_stride +
 * field_offsets[f] (host array, nfields entries, T::fields order, nested
 * messages flattened), naturally aligned (offset, stride and base multiples of
 * the field size: SRPC_E_ALIGN otherwise); no two fields may share a byte of
 * the struct (SRPC_E_INVALID: each leaf has its own bytes in a C++ object).
 * Any stride up to 2^32 - 1 is taken: a struct too wide for a tile of 16 in a
 * workgroup's LDS moves field by field.  Wire bytes are those of
 * srpc_gpu_pack / srpc_gpu_unpack.  unpack_aos writes only the leaf fields'
 * bytes of each struct; every other byte (padding, a vtable pointer) keeps
 * what d_records held.  srpc::gpu::batch_packer<T>::pack_records /
 * unpack_records compute the offsets from T::fields. */
int srpc_gpu_pack_aos(const srpc_plan* plan, const void* d_records, uint64_t record_stride,
                      const uint32_t* field_offsets, uint64_t n, uint8_t* d_wire, uint64_t wire_cap,
                      void* stream);
int srpc_gpu_unpack_aos(const srpc_plan* plan, const uint8_t* d_wire, uint64_t wire_len, uint64_t n,
                        void* d_records, uint64_t record_stride, const uint32_t* field_offsets,
                        srpc_unpack_status* d_status, void* stream);
/* Unpack into FRESH objects (the reference's `std::vector<T> out(n); for
 * (auto& r : out) r.unpack(...)`, generated T::unpack writing only the leaf
 * fields of default-constructed objects): as srpc_gpu_unpack_aos, but every
 * struct byte no leaf field covers is set from h_fill (host, record_stride
 * bytes: e.g. the bytes of a T{} -- its vtable pointer and the defaults of
 * members the message does not carry) instead of being kept, so the old
 * array is never read.  record_stride <= 256 (SRPC_E_UNSUPPORTED otherwise);
 * h_fill is copied during the call.  Records past a short wire (BOUNDS) are
 * left as they were, as in srpc_gpu_unpack_aos. */
int srpc_gpu_unpack_aos_fill(const srpc_plan* plan, const uint8_t* d_wire, uint64_t wire_len, uint64_t n,
                             void* d_records, uint64_t record_stride, const uint32_t* field_offsets,
                             const void* h_fill, srpc_unpack_status* d_status, void* stream);

/* ---- variable-length (string) schemas (SRPC_PATH_VAR) ----------------------
 * A string field f is given as its chars d_cols[f] plus n+1 u64 byte offsets
 * d_str_offs[f] (lengths are offs[i+1]-offs[i]; offs[0] need not be 0).
 * d_str_offs is a host array of nfields device pointers, NULL for fixed fields.
 * Record starts: d_rec_offs, n+1 u64, [0] = 0, [n] = total wire bytes.
 * Both calls need `scratch_bytes` of device scratch (8-byte aligned) from
 * srpc_plan_var_scratch_bytes(plan, n, wire_bytes), wire_bytes being the
 * pack call's wire_cap or the unpack call's wire_len; like the fixed calls
 * they are stream-ordered and allocate nothing.
 * The scratch contract, here and for every later call that takes d_scratch
 * (the frame calls below included): what the scratch holds on entry is
 * arbitrary -- uninitialised memory, or whatever another call, of any plan,
 * kind or size, finished or failed, left in it -- and every call resets the
 * words it reads before it reads them; a scratch larger than the size asked
 * for is fine, and the bytes past that size are not touched; nothing in the
 * scratch carries from one call to the next, so one buffer sized for the
 * largest need may serve any sequence of calls on one stream
 * (tests/test_gpu_scratch_reuse.py). */
int srpc_plan_var_scratch_bytes(const srpc_plan* plan, uint64_t n, uint64_t wire_bytes,
                                uint64_t* out);

/* Pack n records (reference: the `p << r` / pack_request loop over records
 * with std::string members, packer.hpp:193-198).  Writes d_rec_offs[0..n]
 * (an exclusive scan of the record sizes) and the wire bytes.  If the batch
 * needs more than wire_cap bytes, only the first wire_cap are written and
 * *d_status (if non-NULL) gets SRPC_STATUS_BOUNDS with the first record that
 * did not fit; the caller reads d_rec_offs[n] for the size actually needed. */
int srpc_gpu_pack_var(const srpc_plan* plan, const void* const* d_cols,
                      const uint64_t* const* d_str_offs, uint64_t n, uint8_t* d_wire,
                      uint64_t wire_cap, uint64_t* d_rec_offs, srpc_unpack_status* d_status,
                      void* d_scratch, uint64_t scratch_bytes, void* stream);

/* Unpack n records whose starts are d_rec_offs[0..n] (the record index the
 * packer produced, or the frame boundaries of a socket stream) (reference:
 * pipe_output<std::string>, packer.hpp:216-222).  Fixed fields go to
 * d_cols[f] (aligned to their size); string field f's bytes go back to back
 * into d_cols[f] (16-byte aligned, room for wire_len bytes) with offsets
 * d_str_offs[f][0..n].  Prefix mismatches, string lengths past a record's
 * end and records whose size disagrees with the index are reported in
 * *d_status. */
int srpc_gpu_unpack_var(const srpc_plan* plan, const uint8_t* d_wire, uint64_t wire_len,
                        uint64_t n, const uint64_t* d_rec_offs, void* const* d_cols,
                        uint64_t* const* d_str_offs, srpc_unpack_status* d_status,
                        void* d_scratch, uint64_t scratch_bytes, void* stream);

/* Tile table (ABI 6): for every 256-record tile t of a string batch and
 * every string field s (in field order), the chars of field s in records
 * [0, min(256 t, n)): (ceil(n / 256) + 1) * nstrings u64, written by
 * srpc_gpu_var_tile_table from the batch's string offsets (e.g. the pack
 * call's input d_str_offs).  Given to srpc_gpu_unpack_var_tiled, every tile
 * of a schema with several string fields takes its output bases from it
 * instead of looking back at the tiles before it; each tile checks its own
 * totals against the table's differences (a wrong table is detected and the
 * batch decoded again with the look-back, bit-identically).  The table moves
 * 8 bytes per 256 records per string field beside the record index.
 * A NULL table: srpc_gpu_unpack_var. */
int srpc_var_tile_table_words(const srpc_plan* plan, uint64_t n, uint64_t* out);
int srpc_gpu_var_tile_table(const srpc_plan* plan, const uint64_t* const* d_str_offs, uint64_t n,
                            uint64_t* d_table, void* stream);
int srpc_gpu_unpack_var_tiled(const srpc_plan* plan, const uint8_t* d_wire, uint64_t wire_len,
                              uint64_t n, const uint64_t* d_rec_offs, const uint64_t* d_table,
                              void* const* d_cols, uint64_t* const* d_str_offs,
                              srpc_unpack_status* d_status, void* d_scratch, uint64_t scratch_bytes,
                              void* stream);

/* Unpack n records from a stream with NO record index -- the reference's own
 * decode of a concatenated batch with one shared cursor (buffer::_offset,
 * core.hpp:39; packer.hpp:210-222) -- e.g. the bytes a reference packer
 * appended.  The record starts are found on the device and written to
 * d_rec_offs[0..n] with the records decoded as by srpc_gpu_unpack_var: per
 * 8 KiB block, speculative walks from plausible record starts give a table
 * from "where the cursor enters the block" to "where it leaves" (records,
 * chars per string field); an in-order scan of the tables gives every block
 * its exact entry and output bases; then every block writes its records.
 * Nothing waits on the device; work is bounded by the stream's bytes on any
 * input (a cursor position no table holds is walked record by record).
 * The first record the cursor cannot read (prefix mismatch, or a field /
 * string past the end) is reported in *d_status as the first bad record
 * (PREFIX or BOUNDS), as orc_unpack / the reference would meet it; its start
 * is d_rec_offs[i] and every later entry is wire_len (those records are
 * BOUNDS too).  Nothing of record i is decoded: every record before it is
 * exact, d_str_offs[f][i] counts the chars of records 0..i-1 and
 * d_str_offs[f][i+1..n] == d_str_offs[f][i] for every string field f (the
 * later records hold no chars).  A schema with more than four string fields
 * is decoded by srpc_gpu_unpack_var over the index built here and follows
 * the same rule: that decode is given records i..n-1 as empty, and its
 * status is replaced by the stream's (so a prefix mismatch in record i
 * decodes none of its fields, unlike a direct srpc_gpu_unpack_var call).
 * No byte at or past d_wire + wire_len influences any output.
 * Alignment: d_wire may have ANY alignment (the result is the same bytes
 * wherever the wire starts); d_rec_offs and every d_str_offs[f] 8 bytes, a
 * fixed column its field size, a chars column 16 bytes (SRPC_E_ALIGN before
 * any launch, nothing written).
 * Scratch: srpc_plan_var_stream_scratch_bytes (256-byte aligned); the result
 * does not depend on what the scratch held. */
int srpc_plan_var_stream_scratch_bytes(const srpc_plan* plan, uint64_t n, uint64_t wire_len,
                                       uint64_t* out);
int srpc_gpu_unpack_var_stream(const srpc_plan* plan, const uint8_t* d_wire, uint64_t wire_len,
                               uint64_t n, uint64_t* d_rec_offs, void* const* d_cols,
                               uint64_t* const* d_str_offs, srpc_unpack_status* d_status,
                               void* d_scratch, uint64_t scratch_bytes, void* stream);

/* ---- multi-GPU: sharded batches, packed bytes gathered over RCCL -------------
 * The reference packer appends (core.hpp:34, packer.hpp:73), so a batch
 * split into contiguous record shards [lo_g, hi_g) in rank order, each packed
 * on its own GPU, concatenates back to the single-GPU wire exactly.  The only
 * collective is a gather of the shards' wire bytes to a root (ncclSend /
 * ncclRecv in one group), bound by the root's xGMI ingress. */
#define SRPC_SHARD_ALIGN_RECORDS 16  /* shard starts are multiples of 16 records */
#define SRPC_COMM_ID_BYTES 128       /* an RCCL unique id                         */
typedef struct srpc_comm srpc_comm;

/* Records [*lo, *hi) of shard `rank` of n records over nranks shards:
 * contiguous, in rank order, starts aligned to SRPC_SHARD_ALIGN_RECORDS.
 * Host arithmetic only. */
int srpc_shard_range(uint64_t n, int rank, int nranks, uint64_t* lo, uint64_t* hi);

/* One process per GPU: rank 0 makes an id, the caller distributes it
 * (e.g. over its own process group), every rank joins with its device. */
int srpc_comm_unique_id(uint8_t* id_out /* SRPC_COMM_ID_BYTES */);
int srpc_comm_init_rank(const uint8_t* id, int nranks, int rank, int device, srpc_comm** out);
/* One process driving ndev devices: out[g] is rank g on devices[g]. */
int srpc_comm_init_all(const int* devices, int ndev, srpc_comm** out /* ndev */);
int srpc_comm_destroy(srpc_comm* comm);
int srpc_comm_rank(const srpc_comm* comm, int* rank, int* nranks);

/* Each rank contributes one u64 (e.g. its shard's wire bytes, read from the
 * last entry of its d_rec_offs for string schemas); d_out gets nranks. */
int srpc_allgather_u64(srpc_comm* comm, const uint64_t* d_in, uint64_t* d_out, void* stream);

/* The gather's plan, host arithmetic only: the operations rank `rank` of
 * srpc_gather_wire enqueues, in order -- a non-root rank one SEND of its shard
 * (none when it is empty); the root a RECV from every other rank with bytes
 * and a COPY of its own shard, each at byte offset sum(h_all_bytes[0..peer))
 * of the root's wire.  The same argument checks as srpc_gather_wire
 * (SRPC_E_INVALID, SRPC_E_CAPACITY) in the same order; ops gets at most
 * cap_ops entries (SRPC_E_CAPACITY when nranks would not fit), *nops the
 * count.  srpc_gather_wire runs exactly this list, so a transport other
 * than RCCL (a test's gloo) can replay it byte for byte. */
#define SRPC_GATHER_SEND 1
#define SRPC_GATHER_RECV 2
#define SRPC_GATHER_COPY 3
typedef struct srpc_gather_op {
    int32_t kind;    /* SRPC_GATHER_SEND / _RECV / _COPY                       */
    int32_t peer;    /* SEND: the root; RECV: the sender; COPY: the root itself */
    uint64_t offset; /* byte offset into the root's wire (0 for SEND)           */
    uint64_t bytes;
} srpc_gather_op;
int srpc_gather_plan(int rank, int nranks, int root, uint64_t shard_bytes, const uint64_t* h_all_bytes,
                     uint64_t root_cap, srpc_gather_op* ops, int cap_ops, int* nops);

/* Gather: every rank calls it with its shard's wire bytes; the root receives
 * shard r at byte offset sum(h_all_bytes[0..r)) of d_root_wire (root_cap
 * bytes) -- the single-GPU wire of the whole batch.  h_all_bytes (host, one
 * entry per rank) is needed on the root only.  Stream-ordered.  Every
 * argument is checked before the RCCL group is opened; if an operation then
 * cannot be enqueued the group is ended unlaunched and the communicators it
 * touched are aborted (later calls on them return SRPC_E_INVALID). */
int srpc_gather_wire(srpc_comm* comm, const uint8_t* d_shard, uint64_t shard_bytes,
                     uint8_t* d_root_wire, uint64_t root_cap, const uint64_t* h_all_bytes,
                     int root, void* stream);
/* The same from one process for all ndev ranks of srpc_comm_init_all
 * (streams[g] on device g). */
int srpc_group_gather_wire(srpc_comm* const* comms, int ndev, const uint8_t* const* d_shards,
                           const uint64_t* h_bytes, uint8_t* d_root_wire, uint64_t root_cap,
                           int root, void* const* streams);
/* One process, ndev devices, a fixed-size schema: plans[g] (created on device
 * g) packs shard g -- d_cols[g] holds records srpc_shard_range(n, g, ndev) on
 * device g -- into d_shard_wire[g], then the shards are gathered into
 * d_root_wire on the root. */
int srpc_group_pack_gather(const srpc_plan* const* plans, srpc_comm* const* comms, int ndev,
                           const void* const* const* d_cols, uint64_t n, uint8_t* const* d_shard_wire,
                           uint8_t* d_root_wire, uint64_t root_cap, int root, void* const* streams);

/* ---- framed request batches of several methods (server side) ----------------
 * The reference server reads one frame (transport.hpp recv_data: BE32 length |
 * payload) and dispatches it by the method name it starts with (server.hpp:
 * 58-69).  A batch read from a socket holds frames of any method in any order.
 * srpc_frames_classify puts frame i (bytes [d_offs[i], d_offs[i+1]) of d_buf,
 * the last frame ending at buf_len) into bucket k when it is exactly one record
 * of req_plans[k]; the first matching plan wins:
 *   - a fixed-size plan whose prefix is the frame's constant
 *     `BE32 len | str(method) | str(Req::name)`: same length, same prefix;
 *   - a string plan (a method whose request has string fields; at most
 *     SRPC_FRAMES_MAX_STRINGS of them) whose prefix is `str(method) |
 *     str(Req::name)`: the frame's BE32 is its payload length, the payload
 *     starts with the prefix and its fields, each string length read from
 *     the frame, end exactly at the frame's end.
 * A frame whose offsets are out of order or run past buf_len is
 * SRPC_FRAME_UNKNOWN (no byte outside d_buf is read).
 * Outputs (device):
 *   d_class[i]             k, or SRPC_FRAME_UNKNOWN (the caller answers it);
 *   d_index[k*nframes + j] the frames of bucket k (j < d_counts[k]; order
 *                          within a bucket is unspecified; for fixed-size plans
 *                          srpc_frames_unpack_requests_mixed keeps arrival order);
 *   d_counts[0..nplans+1]  frames per bucket, then the response stream's total
 *                          bytes, then the number of unknown frames;
 *   d_out_off[0..nframes]  byte offset of frame i's response in the batch's
 *                          response stream (resp_bytes[k] per frame of bucket
 *                          k, 0 for unknown frames and for string plans' frames,
 *                          whose sizes srpc_frames_offsets adds), total at
 *                          [nframes].
 * nplans <= SRPC_FRAMES_MAX_PLANS.  Scratch: srpc_frames_scratch_bytes, 8-byte
 * aligned.  Stream-ordered; nothing is synchronised. */
#define SRPC_FRAME_UNKNOWN 0xFF
#define SRPC_FRAMES_MAX_PLANS 16
#define SRPC_FRAMES_MAX_STRINGS 16
int srpc_frames_scratch_bytes(uint64_t nframes, int nplans, uint64_t* out);
int srpc_frames_classify(const srpc_plan* const* req_plans, const uint32_t* resp_bytes, int nplans,
                         const uint8_t* d_buf, uint64_t buf_len, const uint32_t* d_offs,
                         uint64_t nframes, uint8_t* d_class, uint32_t* d_index, uint64_t* d_counts,
                         uint64_t* d_out_off, void* d_scratch, uint64_t scratch_bytes, void* stream);
/* d_out[j*record_bytes ..] = the record_bytes bytes at d_buf + d_offs[d_index[j]], j < n. */
int srpc_frames_gather(const uint8_t* d_buf, const uint32_t* d_offs, const uint32_t* d_index,
                       uint64_t n, uint32_t record_bytes, uint8_t* d_out, void* stream);
/* d_out + d_out_off[d_index[j]] = response j (record_bytes bytes of d_resp), j < n. */
int srpc_frames_scatter(const uint8_t* d_resp, const uint32_t* d_index, uint64_t n,
                        uint32_t record_bytes, const uint64_t* d_out_off, uint8_t* d_out,
                        void* stream);
/* String plans' buckets.  gather_var: the payloads (each frame after its BE32
 * length) of frames d_index[0..n) back to back into d_out -- the records of a
 * string request plan -- and their record index d_rec_offs[0..n] (n+1 u64) for
 * srpc_gpu_unpack_var.  Frames must be ones srpc_frames_classify put in a
 * string plan's bucket.  Scratch: srpc_frames_scratch_bytes(n, 1, ..). */
int srpc_frames_gather_var(const uint8_t* d_buf, const uint32_t* d_offs, const uint32_t* d_index,
                           uint64_t n, uint8_t* d_out, uint64_t* d_rec_offs, void* d_scratch,
                           uint64_t scratch_bytes, void* stream);
/* scatter_var: response j (bytes [d_rec_offs[j], d_rec_offs[j+1]) of d_resp, as
 * srpc_gpu_pack_var wrote them with their index) framed as `BE32 len |
 * response` at d_out + d_out_off[d_index[j]], j < n. */
int srpc_frames_scatter_var(const uint8_t* d_resp, const uint64_t* d_rec_offs,
                            const uint32_t* d_index, uint64_t n, const uint64_t* d_out_off,
                            uint8_t* d_out, void* stream);
/* The reply stream's offsets once string plans' responses are packed: frame i
 * takes resp_bytes[k] (fixed plan k), 4 + its response's bytes (string plan k:
 * d_var_rec_offs[k], a host array of nplans device pointers -- the index
 * srpc_gpu_pack_var wrote for bucket k's records in d_index order; NULL for
 * fixed plans), 0 (unknown).  Writes d_out_off[0..nframes] and *d_total.
 * Same plans, d_class, d_index and d_counts as the classify call; same
 * scratch size. */
int srpc_frames_offsets(const srpc_plan* const* req_plans, const uint32_t* resp_bytes, int nplans,
                        const uint8_t* d_class, uint64_t nframes, const uint32_t* d_index,
                        const uint64_t* d_counts, const uint64_t* const* d_var_rec_offs,
                        uint64_t* d_out_off, uint64_t* d_total, void* d_scratch,
                        uint64_t scratch_bytes, void* stream);

/* ---- framed reply batches (client side; added within ABI 8) -------------------
 * The reference's generated stub answers one call at a time: send_data ->
 * recv_data -> unpack_response<R>, which reads `u8 code | str(R::name) | body`
 * (packer.hpp:123-137).  srpc_frames_unpack_replies decodes the reply stream of
 * a whole batch of calls in one launch, in call order: one status code per
 * call in d_codes[i] and the reply's fields in d_cols[f][i] (16-byte aligned
 * columns, as for the TILE path).
 *
 * reply_plan is a fixed-size plan whose prefix is a framed response prefix,
 * `BE32(payload) | u8 code | str(Resp::name)`; its code byte is ignored.  F is
 * its record bytes, the whole frame.  Frame i is bytes [d_offs[i], end_i) of
 * d_buf (16-byte aligned), end_i = d_offs[i+1], or buf_len for the last frame
 * (the convention of srpc_frames_classify).  d_offs == NULL is the uniform
 * mode: frame i is [i*F, (i+1)*F) and no offset is read; if buf_len is short
 * of nframes frames, the frames that fit are decoded, the rest are BOUNDS
 * frames of the table below and SRPC_ERR_BOUNDS is returned (first_bad_record
 * = buf_len / F), as from srpc_gpu_unpack.
 *
 *   frame i                                     d_codes[i]          fields   status
 *   offsets out of order, end_i > buf_len,      SRPC_REPLY_NO_CODE  zero     BOUNDS
 *     shorter than 4 bytes, BE32 != len - 4,
 *     or an empty payload
 *   full: len == F and every prefix byte but    payload[0]          decoded  -
 *     the code byte equals the plan's
 *   bare: a payload of one nonzero byte (the    that byte           zero     -
 *     `BE32(1) | RPC_ERR_FUNCTION_NOT_REGISTERED`
 *     a server sends for an unknown method)
 *   anything else with a payload                payload[0]          zero     PREFIX
 *
 * A full frame is decoded whatever its code, as unpack_response decodes the
 * body after reading any code.  *d_status (may be NULL) is reset by the call;
 * first_bad_record is the smallest flagged i.  (The reference terminates on
 * bare and malformed frames -- buffer::increment throws inside noexcept -- so
 * this table is the contract.)
 * No byte outside [d_buf, d_buf + buf_len) is read.  Work is bounded by
 * buf_len + nframes * F; the call is stream-ordered, allocates nothing, waits
 * on nothing and can be captured.  One kernel: a workgroup stages the span of
 * srpc_frames_replies_per_tile consecutive frames (16 * max(1, 16384 / (16 F)))
 * into LDS with 16-byte loads, parses one frame per lane and writes the
 * columns as 16-byte chunks; frames an oversize junk frame pushed out of the
 * image are read on their own.
 * Refused with nothing launched: a string plan or a prefix under 5 bytes
 * (SRPC_E_UNSUPPORTED); a NULL reply_plan, d_cols or d_codes, or buf_len >=
 * 4 GiB (SRPC_E_INVALID); a misaligned d_buf or column (SRPC_E_ALIGN). */
#define SRPC_REPLY_NO_CODE 0xFF
int srpc_frames_unpack_replies(const srpc_plan* reply_plan, const uint8_t* d_buf, uint64_t buf_len,
                               const uint32_t* d_offs, uint64_t nframes, void* const* d_cols,
                               uint8_t* d_codes, srpc_unpack_status* d_status, void* stream);
/* Testing hook: frames per workgroup tile for this reply plan. */
int srpc_frames_replies_per_tile(const srpc_plan* reply_plan, uint32_t* out);

/* ---- framed reply batches into structs (client side; added within ABI 8) ------
 * srpc_frames_unpack_replies with an array of the caller's own structs in place
 * of the columns: the reply of call i is decoded straight into struct i, as a
 * generated stub of the reference returns a response_t<Resp>.
 *
 * Frames: the contract of srpc_frames_unpack_replies, unchanged -- the same
 * reply_plan (a fixed-size plan behind a framed response prefix, code byte
 * ignored), the same frame convention, d_offs == NULL the uniform mode, the
 * per-frame table above, SRPC_REPLY_NO_CODE, and SRPC_ERR_BOUNDS for a short
 * uniform stream.  d_codes[i], the status flags and first_bad_record are
 * identical to the column call's on the same input.
 *
 * Structs: field_offsets and record_stride as for srpc_gpu_unpack_aos_fill
 * (leaf f of struct i at d_records + i * record_stride + field_offsets[f];
 * natural alignment, no two leaves sharing a byte, record_stride <= 256).
 * h_fill is record_stride host bytes (e.g. the image of a Resp{}), copied
 * during the call.  Every one of the nframes structs is written whole: a full
 * frame gives its leaf fields the frame's values, any other frame gives zero
 * leaf fields (as the column call gives zero fields), and in both cases every
 * byte no leaf covers comes from h_fill.  No byte at or past d_records +
 * nframes * record_stride is written, and the old array is never read.
 *
 * Refused with nothing launched, in this order:
 *   1. SRPC_E_INVALID: a NULL reply_plan, d_records (nframes > 0),
 *      field_offsets, h_fill or d_codes; record_stride == 0; buf_len >= 4 GiB
 *      (checked before the plan is read);
 *   2. SRPC_E_UNSUPPORTED: a string plan, a prefix under 5 bytes, or
 *      record_stride > 256;
 *   3. SRPC_E_INVALID: overlapping leaves, or a leaf past the stride;
 *   4. SRPC_E_ALIGN: a misaligned d_buf (16) or d_records (16), or an offset or
 *      the stride against its field's size.
 * No byte outside [d_buf, d_buf + buf_len) is read; the call is stream-ordered,
 * allocates nothing, waits on nothing and can be captured.
 *
 * One kernel, the column call's with its last step replaced: a workgroup
 * stages the span of R consecutive frames into LDS and judges one frame per
 * lane; then one lane per 16-byte piece of the tile's structs assembles that
 * piece -- leaf bytes from the image or zero, the rest from an LDS copy of
 * h_fill, through a per-struct-byte source table in LDS -- and stores it whole
 * (the array's last piece bytewise when nframes * record_stride is no multiple
 * of 16).  R = 16 * max(1, (16384 - 4 * S16) / (16 F)), S16 = record_stride
 * rounded up to 16: the column call's rule with the table and the fill taken
 * out of the image's bytes, so image + table + fill stay within the 16 KiB the
 * column kernel's image may take and as many workgroups are resident. */
int srpc_frames_unpack_replies_aos(const srpc_plan* reply_plan, const uint8_t* d_buf, uint64_t buf_len,
                                   const uint32_t* d_offs, uint64_t nframes,
                                   void* d_records, uint64_t record_stride, const uint32_t* field_offsets,
                                   const void* h_fill, uint8_t* d_codes,
                                   srpc_unpack_status* d_status, void* stream);
/* Testing hook: frames per workgroup tile for this plan and stride. */
int srpc_frames_replies_aos_per_tile(const srpc_plan* reply_plan, uint64_t record_stride, uint32_t* out);

/* ---- framed reply batches with string fields (client side; added within ABI 8) --
 * The reply stream of a batch of calls to a method whose response has
 * std::string members (the reference's stub: unpack_response<R> over a string
 * body, packer.hpp:123-137, 216-222), decoded in call order: one code per call
 * in d_codes[i], fixed field f in d_cols[f][i], string field f's chars back to
 * back in d_cols[f] with offsets d_str_offs[f][0..nframes] ([0] = 0).
 *
 * reply_plan is a string plan (SRPC_PATH_VAR, at most SRPC_FRAMES_MAX_STRINGS
 * strings) whose prefix is the UNFRAMED response prefix `u8 code |
 * str(Resp::name)`; it follows the frame's BE32 (the convention of
 * srpc_frames_classify for string plans) and its code byte is ignored.  Frame i
 * is bytes [d_offs[i], end_i) of d_buf (16-byte aligned), end_i = d_offs[i+1],
 * or buf_len for the last frame.  d_offs is required: frames of varying length
 * have no uniform mode.  Columns are 16-byte aligned; a string column has room
 * for buf_len bytes, as for srpc_gpu_unpack_var.  d_str_offs is the host array
 * srpc_gpu_unpack_var takes (8-byte aligned device pointers, NULL for fixed
 * fields).
 *
 *   frame i                                     d_codes[i]          fixed   strings  status
 *   offsets out of order, end_i > buf_len,      SRPC_REPLY_NO_CODE  zero    empty    BOUNDS
 *     shorter than 4 bytes, BE32 != len - 4,
 *     or an empty payload
 *   full: the payload starts with the plan's    payload[0]          decoded copied   -
 *     prefix (code byte excepted) and the walk
 *     of its fields, each string's u64 length
 *     read from the frame, ends exactly at end_i
 *   bare: a payload of one nonzero byte         that byte           zero    empty    -
 *   the prefix matches, but a field or string   payload[0]          zero    empty    BOUNDS
 *     runs past end_i, or the walk ends before
 *     end_i
 *   anything else with a payload (one shorter   payload[0]          zero    empty    PREFIX
 *     than the prefix included)
 *
 * "Empty" is offs[i+1] == offs[i]: later calls' chars stay packed back to back.
 * A string length is compared as `len > end - cursor`, so 2^63 or 2^64 - 1
 * cannot wrap.  *d_status (may be NULL) is reset by the call; first_bad_record
 * is the smallest flagged i.  With ascending offsets (what walk_frames gives)
 * the chars of a column total under buf_len.  Offsets out of order can make
 * full frames overlap and their chars total more: the offsets still count every
 * full frame, but no byte of a string column at or past buf_len is written.
 * Properties:
 *   - no byte outside [d_buf, d_buf + buf_len) is read;
 *   - no byte of a column is written past its nframes elements, and none of a
 *     string column past offs[nframes] (the last partial 16-byte chunk is
 *     written bytewise);
 *   - the call is stream-ordered and allocates nothing;
 *   - it waits on nothing on the device: no look-back polling, no STALLED case;
 *   - the number of launches (a parse pass, one scan of three launches per
 *     string field, a copy pass, the status reset) does not depend on the data,
 *     so the call can be captured;
 *   - work is bounded by buf_len + nframes * (fixed bytes) on any input.
 * A tile is srpc_frames_replies_var_tile's `frames` consecutive frames, whose
 * span is staged into an LDS image of `image_bytes`; a frame that does not lie
 * whole inside the image is parsed from global memory by its lane (the fixed
 * bytes only) and its chars are copied from global memory 16 output bytes per
 * lane by the whole workgroup.
 * Scratch: srpc_frames_replies_var_scratch_bytes, 8-byte aligned.
 * Refused with nothing launched: a fixed plan, a prefix under 1 byte or more
 * than SRPC_FRAMES_MAX_STRINGS strings (SRPC_E_UNSUPPORTED); a NULL
 * reply_plan, d_offs (with nframes > 0), d_cols, d_str_offs, d_codes or
 * d_scratch, a NULL column or offsets pointer of a string field, or buf_len >=
 * 4 GiB (SRPC_E_INVALID; the arguments themselves are checked before the plan
 * is read); too little scratch (SRPC_E_CAPACITY); a misaligned d_buf, column,
 * offsets array or scratch (SRPC_E_ALIGN). */
int srpc_frames_replies_var_scratch_bytes(const srpc_plan* reply_plan, uint64_t nframes, uint64_t* out);
int srpc_frames_unpack_replies_var(const srpc_plan* reply_plan, const uint8_t* d_buf, uint64_t buf_len,
                                   const uint32_t* d_offs, uint64_t nframes, void* const* d_cols,
                                   uint64_t* const* d_str_offs, uint8_t* d_codes,
                                   srpc_unpack_status* d_status, void* d_scratch, uint64_t scratch_bytes,
                                   void* stream);
/* Testing hook: frames per workgroup tile and the tile's LDS image bytes. */
int srpc_frames_replies_var_tile(const srpc_plan* reply_plan, uint32_t* frames, uint32_t* image_bytes);

/* d_out + d_rec_offs[j] + 4 j = BE32(len_j) | record j, j < n: the records
 * srpc_gpu_pack_var wrote (with the prefix `str(method) | str(Req::name)`: a
 * string request batch), framed for transport.hpp's recv_data.  out_cap >=
 * d_rec_offs[n] + 4 n is the caller's promise; a record of 4 GiB or more, or
 * one whose frame would pass out_cap, sets SRPC_STATUS_BOUNDS in *d_status
 * (may be NULL; not reset by this call, so it can be the pack call's) and its
 * frame is not written. */
int srpc_frames_frame_var(const uint8_t* d_records, const uint64_t* d_rec_offs, uint64_t n,
                          uint8_t* d_out, uint64_t out_cap, srpc_unpack_status* d_status, void* stream);

/* ---- batches of calls of several methods, in call order (client side; added
 * within ABI 8) ----------------------------------------------------------------
 * The mirror of srpc_frames_classify: a chunk of ncalls calls of up to
 * SRPC_FRAMES_MAX_PLANS fixed-size methods, in the caller's order, is packed
 * into request frames in one pass and its reply stream decoded in one pass.
 *
 *   K = nplans, 1..SRPC_FRAMES_MAX_PLANS.  Plan k is a fixed-size plan with a
 *     framed prefix (request: `BE32(payload) | str(method) | str(Req::name)`,
 *     reply: `BE32(payload) | u8 code | str(Resp::name)`); F_k is its record
 *     bytes, the whole frame.  The plans of one call have at most
 *     SRPC_FRAMES_MIXED_MAX_FIELDS leaf fields in all (SRPC_E_UNSUPPORTED past it).
 *   d_method[i] (u8, device) is the plan of call i; rank(i) the number of calls
 *     j < i with d_method[j] == d_method[i].
 *   Call i's fields are element h_first[k] + rank(i) of plan k's columns
 *     d_cols[k][f] (host array of K host arrays of device pointers, 16-byte
 *     aligned).  h_first[k] (host; NULL = zeros) is the number of calls of
 *     plan k in earlier chunks of the batch, h_cap[k] (host) the elements plan
 *     k's columns have.
 *   A call is BAD when d_method[i] >= K or h_first[k] + rank(i) >= h_cap[k]; no
 *     column element is read or written for a bad call.
 *
 * srpc_frames_mixed_index builds the chunk's call index in caller memory
 * (d_index: opaque, 8-byte aligned, srpc_frames_mixed_index_bytes): one row of
 * K + 1 u32 per 256 calls and one more per 16 rows -- the calls of each plan
 * (and of ids >= K) before that row -- so 4 (K + 1) (1 + 1/16) / 256 bytes per
 * call (0.08 B at K = 4, 0.28 B at K = 16) and no rank per call; every
 * workgroup of the calls below finds its calls' ranks from its rows and
 * per-plan ballots over the row's 256 method bytes.  d_counts[k] = calls of plan k, d_counts[K] = calls with an id >= K.
 * *d_status (may be NULL) is reset, then gets SRPC_STATUS_BOUNDS with the
 * smallest such call when one exists.  Three launches whatever the data (status
 * reset, the histograms, one workgroup scanning the 4096-call rows); nothing
 * waits on another workgroup.
 *
 * srpc_frames_mixed_ranks (testing hook, and the recount of a flagged chunk)
 * writes rank(i) to d_rank[i], 0xFFFFFFFF for an id >= K.
 * srpc_frames_mixed_tile: the calls one workgroup of pack / decode takes with
 * these plans: 256, or the power of two >= 16 whose frames of max_k F_k bytes
 * fit the 32 KiB LDS image.
 *
 * srpc_frames_pack_requests_mixed writes the request frames in call order:
 * frame i is plan d_method[i]'s prefix followed by the call's fields, raw
 * little-endian as srpc_gpu_pack writes them, at the byte offset that is the
 * sum of the frames before it.  A bad call gets no frame (zero bytes,
 * d_offs[i + 1] == d_offs[i], SRPC_STATUS_BOUNDS, first_bad_record the smallest
 * such i); the other frames stay contiguous and correct.  d_offs (may be NULL)
 * receives ncalls + 1 u32: the frame offsets and the total.  *d_status (may be
 * NULL) is NOT reset: it can be the index call's.  out_cap < ncalls * max_k F_k
 * is SRPC_E_CAPACITY.  No byte of d_out (16-byte aligned) at or past the total
 * is written.  One launch.
 *
 * srpc_frames_unpack_replies_mixed decodes the chunk's reply stream: frame i
 * (i < nframes <= ncalls) is bytes [d_offs[i], end_i) of d_buf, end_i =
 * d_offs[i + 1], or buf_len for the last frame, judged by the table of
 * srpc_frames_unpack_replies with F = F_k and plan k's prefix, k =
 * d_method[i]: d_codes[i] as in that table, the fields (decoded for a full
 * frame, zero otherwise) to element h_first[k] + rank(i) of plan k's columns.
 * A bad call's frame is the table's first row (SRPC_REPLY_NO_CODE, BOUNDS) and
 * no column element is touched for it.  Calls nframes <= i < ncalls have no
 * frame: d_codes[i] = unanswered_code, zero fields, no status flag.  nframes ==
 * 0 may come with d_buf == NULL; d_offs is required otherwise (frames of
 * different plans differ in length: there is no uniform mode).
 *   - no byte outside [d_buf, d_buf + buf_len) is read;
 *   - no column element is written but those of the chunk's ncalls calls;
 *   - *d_status (may be NULL) is reset; first_bad_record is the smallest
 *     flagged i;
 *   - the call is stream-ordered, allocates nothing, waits on nothing; its
 *     launches (status reset, one decode) do not depend on the data;
 *   - work is bounded by buf_len + ncalls * max_k F_k.
 *
 * Refused with nothing launched, in this order: a NULL required pointer,
 * nplans outside 1..16, nframes > ncalls, buf_len >= 4 GiB or ncalls >= 2^32
 * (SRPC_E_INVALID; checked before any plan is read); a string plan, a reply
 * prefix under 5 or a request prefix under 4 bytes (SRPC_E_UNSUPPORTED); a
 * misaligned d_buf, d_out, column (16), index (8) or d_offs (4) (SRPC_E_ALIGN);
 * too small an index or out_cap (SRPC_E_CAPACITY). */
#define SRPC_FRAMES_MIXED_MAX_FIELDS 192
int srpc_frames_mixed_index_bytes(uint64_t ncalls, int nplans, uint64_t* out);
int srpc_frames_mixed_index(const uint8_t* d_method, uint64_t ncalls, int nplans, void* d_index,
                            uint64_t index_bytes, uint64_t* d_counts /* nplans + 1 */,
                            srpc_unpack_status* d_status, void* stream);
int srpc_frames_mixed_ranks(const void* d_index, const uint8_t* d_method, uint64_t ncalls, int nplans,
                            uint32_t* d_rank, void* stream);
int srpc_frames_mixed_tile(const srpc_plan* const* plans, int nplans, uint32_t* calls_per_tile);
int srpc_frames_pack_requests_mixed(const srpc_plan* const* req_plans, int nplans,
                                    const void* const* const* d_cols, const uint64_t* h_first,
                                    const uint64_t* h_cap, const uint8_t* d_method, const void* d_index,
                                    uint64_t ncalls, uint8_t* d_out, uint64_t out_cap,
                                    uint32_t* d_offs /* ncalls + 1, may be NULL */,
                                    srpc_unpack_status* d_status, void* stream);
int srpc_frames_unpack_replies_mixed(const srpc_plan* const* reply_plans, int nplans, const uint8_t* d_buf,
                                     uint64_t buf_len, const uint32_t* d_offs, uint64_t nframes,
                                     const uint8_t* d_method, const void* d_index, uint64_t ncalls,
                                     uint8_t unanswered_code, void* const* const* d_cols,
                                     const uint64_t* h_first, const uint64_t* h_cap, uint8_t* d_codes,
                                     srpc_unpack_status* d_status, void* stream);

/* ---- batches of calls of several methods from struct arrays, in call order
 * (client side; added within ABI 8) ---------------------------------------------
 * srpc_frames_pack_requests_mixed and srpc_frames_unpack_replies_mixed with
 * one device array of the caller's own structs per plan in place of its
 * columns.  Everything that is not about where a call's fields live is the
 * section above, unchanged: K, the fixed-size plans with framed prefixes,
 * d_method, rank(i), h_first, h_cap, BAD calls, the call index of
 * srpc_frames_mixed_index (used as it is), the reply table of
 * srpc_frames_unpack_replies per call's own plan, SRPC_REPLY_NO_CODE and the
 * status rules.
 *
 * Structs: plan k's calls live in d_recs[k] (host array of K device pointers,
 * 16-byte aligned), h_stride[k] bytes each, leaf f of the plan's field order at
 * byte h_leaf_offs[k][f] (u32); the conventions of srpc_gpu_pack_aos /
 * srpc_gpu_unpack_aos_fill: natural alignment, no two leaves sharing a byte, no
 * leaf past the stride.  Call i's struct is element h_first[k] + rank(i);
 * h_cap[k] is the elements the array has.
 *
 * srpc_frames_pack_requests_mixed_aos: the output bytes, d_offs, the status,
 * the handling of BAD calls and of out_cap are the column call's on the same
 * values.  Only leaf bytes of the chunk's own structs are read; h_stride[k] is
 * any value below 2^32.  One launch; no scratch.
 *
 * The ordered reply pack of a server over struct arrays is
 * srpc_frames_pack_requests_mixed_aos itself, which by its contract writes the
 * frames of any fixed-size plans with framed prefixes from struct arrays:
 * called with the framed RESPONSE plans, the Resp arrays, d_method = d_class and
 * the d_index srpc_frames_unpack_requests_mixed_aos wrote, it writes the reply
 * stream in arrival order.  An unknown frame is that call's bad call: zero
 * bytes, d_offs[i + 1] == d_offs[i], for the caller to answer in its place.
 *
 * srpc_frames_unpack_replies_mixed_aos: d_codes, the flags and
 * first_bad_record are the column call's on the same input.  h_fill[k] is
 * h_stride[k] <= 256 host bytes (e.g. the image of a Resp{}), copied during the
 * call.  Every struct of the chunk's ncalls calls that is not BAD is written
 * whole, exactly once, and never read: leaf bytes get the frame's values for a
 * full frame, zero for any other frame and for calls nframes <= i < ncalls
 * (which also get unanswered_code); every other byte comes from plan k's fill.
 * No byte outside elements [h_first[k], h_first[k] + calls of k in the chunk)
 * of any array is written, and nothing is written for a BAD call.
 * d_scratch (16-byte aligned, srpc_frames_mixed_aos_scratch_bytes, which takes
 * the plans of either side, request prefixes of 4 bytes included: the plans'
 * per-struct-byte source tables and fills, 3 S16 + 16 bytes per plan, S16 =
 * h_stride[k] rounded up to 16) receives them by by-value launches: no host
 * copy outlives the call.
 *
 * Both calls are stream-ordered, allocate nothing, wait on nothing on the host
 * or the device and can be captured; their launches (pack: one; decode: status
 * reset, one per 2 KiB of scratch, one decode) do not depend on the data; work
 * is bounded as the column calls state.
 *
 * The decode's workgroup takes srpc_frames_mixed_aos_tile calls: the rule of
 * srpc_frames_mixed_tile with the scratch bytes taken out of the 32 KiB image.
 * It stages and judges as the column kernel; then, the good calls of one plan
 * being consecutive elements of its array, it assembles every 16-byte piece of
 * those K slices from the image, zero or the fill through the plan's table and
 * stores it whole; a slice's first and last bytes that share a piece with a
 * neighbouring tile's slice are stored bytewise.
 *
 * Refused with nothing launched, in this order:
 *   1. SRPC_E_INVALID (before any plan is read): the column calls' NULL and
 *      range checks with d_recs, h_stride, h_leaf_offs, h_leaf_offs[k], h_fill,
 *      h_fill[k], d_scratch and d_recs[k] (where h_cap[k] leaves an element)
 *      among the pointers; h_stride[k] == 0 or >= 2^32;
 *   2. SRPC_E_UNSUPPORTED: a string plan, a short prefix, more than
 *      SRPC_FRAMES_MIXED_MAX_FIELDS leaves, a decode stride above 256;
 *   3. SRPC_E_INVALID: overlapping leaves, or a leaf past the stride;
 *   4. SRPC_E_ALIGN: d_buf, d_out, an array, d_scratch (16), the index (8),
 *      d_offs (4), or an offset or stride against its leaf's size;
 *   5. SRPC_E_CAPACITY: scratch_bytes or out_cap. */
int srpc_frames_mixed_aos_scratch_bytes(const srpc_plan* const* plans, int nplans, const uint64_t* h_stride,
                                        uint64_t* out);
/* Testing hook: calls per workgroup tile of a decode into struct arrays with
 * these plans (the pack's is srpc_frames_mixed_tile). */
int srpc_frames_mixed_aos_tile(const srpc_plan* const* plans, int nplans, const uint64_t* h_stride,
                               uint32_t* calls_per_tile);
int srpc_frames_pack_requests_mixed_aos(const srpc_plan* const* req_plans, int nplans,
                                        const void* const* d_recs, const uint64_t* h_stride,
                                        const uint32_t* const* h_leaf_offs, const uint64_t* h_first,
                                        const uint64_t* h_cap, const uint8_t* d_method, const void* d_index,
                                        uint64_t ncalls, uint8_t* d_out, uint64_t out_cap,
                                        uint32_t* d_offs /* ncalls + 1, may be NULL */,
                                        srpc_unpack_status* d_status, void* stream);
int srpc_frames_unpack_replies_mixed_aos(const srpc_plan* const* reply_plans, int nplans, const uint8_t* d_buf,
                                         uint64_t buf_len, const uint32_t* d_offs, uint64_t nframes,
                                         const uint8_t* d_method, const void* d_index, uint64_t ncalls,
                                         uint8_t unanswered_code, void* const* d_recs, const uint64_t* h_stride,
                                         const uint32_t* const* h_leaf_offs, const void* const* h_fill,
                                         const uint64_t* h_first, const uint64_t* h_cap, uint8_t* d_codes,
                                         srpc_unpack_status* d_status, void* d_scratch, uint64_t scratch_bytes,
                                         void* stream);

/* ---- batches of request frames of several methods, in arrival order (server
 * side; added within ABI 8) ------------------------------------------------------
 * The server's counterpart of the section above: where srpc_frames_classify
 * fills per-method buckets in no particular order, this call keeps the order
 * the frames arrived in, within a method and (through d_class and the index)
 * across methods, and needs no per-method gather.
 *
 * srpc_frames_unpack_requests_mixed takes K = nplans fixed-size request plans
 * with framed prefixes (as the *_mixed calls above) and nframes frames, frame i
 * being bytes [d_offs[i], end_i) of d_buf, end_i = d_offs[i + 1], or buf_len for
 * the last frame (the extent convention of srpc_frames_classify).
 *   d_class[i] (u8, device, out) is k when the frame is exactly one record of
 *     plan k: its length is F_k and its first prefix_len_k bytes are plan k's
 *     prefix, the BE32 included; the first matching plan wins.  Every other
 *     frame is SRPC_FRAME_UNKNOWN: offsets out of order, an end past buf_len, a
 *     frame under 4 bytes.  This is srpc_frames_classify's rule for fixed-size
 *     plans; the two calls write the same d_class for every input.
 *   rank(i) is the number of frames j < i with d_class[j] == d_class[i].  A
 *     frame of class k has its fields (raw little-endian, as srpc_gpu_unpack
 *     reads them) written to element h_first[k] + rank(i) of d_cols[k][f];
 *     d_cols, h_first (NULL = zeros) and h_cap as in the section above.  No
 *     element is written for an unknown frame.  A frame whose element would be
 *     at or past h_cap[k] keeps its class and writes nothing: SRPC_STATUS_BOUNDS,
 *     first_bad_record the smallest such i.
 *   d_index (opaque, 8-byte aligned, srpc_frames_mixed_index_bytes(nframes, K))
 *     receives the call index over d_class, the one srpc_frames_mixed_index
 *     builds: it serves srpc_frames_mixed_ranks and the reply pack below.
 *   d_counts[k] (u64, device, K + 1 entries) = frames of plan k, d_counts[K] =
 *     unknown frames.
 *   - no byte outside [d_buf, d_buf + buf_len) is read;
 *   - no column element is written but the frames' own;
 *   - *d_status (may be NULL) is reset by the call;
 *   - the call is stream-ordered, allocates nothing, waits on nothing; its
 *     launches (status reset, classify, the index's two, decode) do not depend
 *     on the data; work is bounded by buf_len + nframes * max_k F_k.  The
 *     stream is read twice: a frame's rank needs the class of every frame
 *     before it.
 *
 * Refused with nothing launched, in this order: a NULL required pointer
 * (req_plans, d_cols, h_cap, d_index, d_counts; d_buf, d_offs, d_class when
 * nframes > 0), nplans outside 1..16, buf_len >= 4 GiB or nframes >= 2^32
 * (SRPC_E_INVALID; checked before any plan is read); a string plan, a prefix
 * under 4 bytes or more than SRPC_FRAMES_MIXED_MAX_FIELDS leaves
 * (SRPC_E_UNSUPPORTED); a misaligned d_buf, column (16), index, d_counts (8) or
 * d_offs (4) (SRPC_E_ALIGN); an index smaller than
 * srpc_frames_mixed_index_bytes(nframes, nplans) (SRPC_E_CAPACITY).
 *
 * The ordered reply pack is srpc_frames_pack_requests_mixed itself, which by
 * its contract writes the frames of any fixed-size plans with framed prefixes:
 * called with the framed RESPONSE plans, the response columns, d_method =
 * d_class and the d_index this call wrote, it writes the reply stream in
 * arrival order.  An unknown frame is that call's bad call: zero bytes,
 * d_offs[i + 1] == d_offs[i], for the caller to answer in its place.  The
 * SRPC_STATUS_BOUNDS it raises for ids >= K then means only "unknown frames
 * present" (or a short response column): such callers pass a status of their
 * own, or NULL. */
int srpc_frames_unpack_requests_mixed(const srpc_plan* const* req_plans, int nplans, const uint8_t* d_buf,
                                      uint64_t buf_len, const uint32_t* d_offs, uint64_t nframes,
                                      void* const* const* d_cols, const uint64_t* h_first,
                                      const uint64_t* h_cap, uint8_t* d_class /* nframes, out */,
                                      void* d_index, uint64_t index_bytes,
                                      uint64_t* d_counts /* nplans + 1, out */,
                                      srpc_unpack_status* d_status, void* stream);

/* ---- batches of request frames of several methods into struct arrays, in
 * arrival order (server side; added within ABI 8) --------------------------------
 * srpc_frames_unpack_requests_mixed with one device array of the caller's own
 * structs per plan in place of its columns: the server's counterpart of
 * srpc_frames_pack_requests_mixed_aos.  Everything that is not about where a
 * frame's fields live is the section above, unchanged: K, the framed request
 * plans, the frame extents, the classification rule (srpc_frames_classify's,
 * the first matching plan wins), rank(i), d_counts and the status rules.
 * d_class and d_index are byte-identical to what the column call writes for the
 * same input, so the index serves srpc_frames_mixed_ranks and the reply pack
 * (srpc_frames_pack_requests_mixed_aos over the response plans, see there).
 *
 * Structs: the conventions of srpc_frames_unpack_replies_mixed_aos.  Plan k's
 * requests live in d_recs[k] (host array of K device pointers, 16-byte
 * aligned), h_stride[k] <= 256 bytes each, leaf f at byte h_leaf_offs[k][f]
 * (u32): natural alignment, no two leaves sharing a byte, no leaf past the
 * stride.  h_fill[k] is h_stride[k] host bytes (e.g. the image of a Req{}),
 * copied during the call.
 *
 * A frame of class k is element h_first[k] + rank(i) of plan k's array.  When
 * that element is below h_cap[k] its struct is written whole, exactly once, and
 * never read: leaf bytes come from the frame, raw little-endian, every other
 * byte from plan k's fill.
 *   - nothing is written for an unknown frame;
 *   - nothing is written for a frame whose element is at or past h_cap[k]: it
 *     keeps its class and raises SRPC_STATUS_BOUNDS, first_bad_record the
 *     smallest such i;
 *   - no byte outside elements [h_first[k], h_first[k] + frames of k) of any
 *     array is written;
 *   - no byte outside [d_buf, d_buf + buf_len) is read, whatever d_offs holds:
 *     the decode pass checks every extent again and does not trust d_class;
 *   - *d_status (may be NULL) is reset by the call;
 *   - the call is stream-ordered, allocates nothing, waits on nothing on the
 *     host or the device and can be captured; its launches (status reset, one
 *     per 2 KiB of scratch, classify, the index's two, decode) do not depend on
 *     the data; work is bounded by buf_len + nframes * max_k F_k.  The stream
 *     is read twice.
 *
 * d_scratch (16-byte aligned) receives the plans' tables and fills by by-value
 * launches; its size and the decode's frames per tile are
 * srpc_frames_mixed_aos_scratch_bytes and srpc_frames_mixed_aos_tile, called
 * with the request plans.  The classify pass keeps the column call's tile.  The
 * decode stages and ranks as the column kernel; then, the frames of one plan
 * that have an element being consecutive elements of its array, it assembles
 * every 16-byte piece of those K slices from the image or the fill through the
 * plan's table and stores it whole; a slice's first and last bytes that share a
 * piece with a neighbouring tile's slice are stored bytewise.
 *
 * Refused with nothing launched, in this order:
 *   1. SRPC_E_INVALID (before any plan is read): the column call's NULL and
 *      range checks with d_recs, h_stride, h_leaf_offs, h_leaf_offs[k], h_fill,
 *      h_fill[k], d_scratch and d_recs[k] (where h_cap[k] leaves an element)
 *      among the pointers; h_stride[k] == 0 or >= 2^32;
 *   2. SRPC_E_UNSUPPORTED: a string plan, a prefix under 4 bytes, more than
 *      SRPC_FRAMES_MIXED_MAX_FIELDS leaves, a stride above 256;
 *   3. SRPC_E_INVALID: overlapping leaves, or a leaf past the stride;
 *   4. SRPC_E_ALIGN: d_buf, an array, d_scratch (16), the index, d_counts (8),
 *      d_offs (4), or an offset or stride against its leaf's size;
 *   5. SRPC_E_CAPACITY: the index or scratch_bytes. */
int srpc_frames_unpack_requests_mixed_aos(const srpc_plan* const* req_plans, int nplans, const uint8_t* d_buf,
                                          uint64_t buf_len, const uint32_t* d_offs, uint64_t nframes,
                                          void* const* d_recs, const uint64_t* h_stride,
                                          const uint32_t* const* h_leaf_offs, const void* const* h_fill,
                                          const uint64_t* h_first, const uint64_t* h_cap,
                                          uint8_t* d_class /* nframes, out */, void* d_index,
                                          uint64_t index_bytes, uint64_t* d_counts /* nplans + 1, out */,
                                          srpc_unpack_status* d_status, void* d_scratch,
                                          uint64_t scratch_bytes, void* stream);

/* ---- batches of calls of several methods with string bodies, in call order
 * (client side; added within ABI 8) ----------------------------------------------
 * The calls above with string plans allowed beside the fixed-size ones: the
 * client-side mirror of srpc_frames_classify over register_var_method traffic.
 * K, d_method, rank(i), h_first[k], h_cap[k], BAD calls and the index are those
 * of the section above; the index srpc_frames_mixed_index built is used as is.
 * The srpc_frames_*_mixed calls above keep refusing string plans.
 *
 * Plan k is one of two kinds, and both may appear in one batch:
 *   - a fixed-size plan with a framed prefix, exactly as the *_mixed calls take;
 *   - a string plan (SRPC_PATH_VAR, at most SRPC_FRAMES_MAX_STRINGS strings)
 *     with the UNFRAMED prefix -- request: `str(method) | str(Req::name)`, reply:
 *     `u8 code | str(Resp::name)`, its code byte ignored -- the convention of
 *     srpc_frames_classify and srpc_frames_unpack_replies_var.  Its frame is
 *     `BE32(len) | prefix | fields`, each string as `u64 length | chars`.
 * All plans together have at most SRPC_FRAMES_MIXED_MAX_FIELDS leaves; buf_len
 * and out_cap are under 4 GiB, ncalls under 2^32.
 * d_cols is as above.  d_str_offs is a host array of K host arrays, one entry
 * per leaf (NULL for fixed leaves; the array of a fixed plan may be NULL): each a
 * device pointer to h_cap[k] + 1 u64, absolute over the leg -- element e's
 * string is bytes [offs[e], offs[e + 1]) of its column, which holds the leg's
 * chars back to back in element order.
 * Scratch: srpc_frames_mixed_var_scratch_bytes(plans of that call, ncalls),
 * 8-byte aligned, monotone in ncalls; its contents need not be kept or cleared
 * between calls.  srpc_frames_mixed_var_tile (testing hook): the calls one
 * workgroup of pack / decode takes with these plans (256, or the power of two >=
 * 16 whose frames without their chars fit the image) and the bytes of its LDS
 * image window.
 *
 * srpc_frames_pack_requests_mixed_var: frame i is plan d_method[i]'s frame of
 * element h_first[k] + rank(i); the frames lie back to back in call order, each
 * byte-identical to `BE32 | pack_request` of the scalar packer (packer.hpp:77-82,
 * 193-198).  A call is also BAD when a pair of its strings' offsets decreases;
 * for a BAD call no chars are read, no frame is written (zero bytes) and BOUNDS
 * is set.  Offsets are computed in 64 bits (one frame's length saturates at
 * 4 GiB, which no out_cap admits): *d_total (device, 8-byte aligned) receives
 * the untruncated total, d_offs[j] = min(offset_j, out_cap) for j <= ncalls.
 * When the total exceeds out_cap, BOUNDS is set with first_bad_record the first
 * call whose frame ends past out_cap; the frames ending at or before out_cap are
 * complete and no byte at or past out_cap is written.  No byte at or past the
 * total is written.  *d_status (may be NULL) is NOT reset: it can be the index
 * call's.
 *
 * srpc_frames_unpack_replies_mixed_var: frame i (i < nframes) is judged by the
 * table of srpc_frames_unpack_replies_var when plan d_method[i] is a string
 * plan, by that of srpc_frames_unpack_replies when it is fixed.  d_codes[i] is as
 * in the table; fixed fields go to element h_first[k] + rank(i), decoded for a
 * full frame and zero otherwise; string fields are copied for a full frame and
 * empty otherwise.  String offsets are absolute over the leg: the call writes
 * entry 0 = 0 when h_first[k] == 0, otherwise it continues from entry
 * h_first[k], which the previous chunk's call wrote, and it writes entries
 * h_first[k] + 1 .. h_first[k] + count_k.  d_ends[s] (device, one u64 per string
 * slot; slots are numbered over the plans and then their string leaves, in
 * order) receives the end offset of slot s, so the host sees every total in one
 * copy.  h_str_cap[k][f] (host array of K host arrays, read for string leaves;
 * the array of a fixed plan may be NULL) is the bytes string column f of plan k
 * has: no char is written at or past it, while the offsets still count every
 * full frame, so an overflow shows as d_ends[s] > capacity.  Calls nframes <= i
 * < ncalls get unanswered_code, zero fields, empty strings and no flag.  A BAD
 * call's frame is the table's first row and no column or offsets element is
 * touched for it.  *d_status (may be NULL) is reset; first_bad_record is the
 * smallest flagged i.  nframes == 0 may come with d_buf == NULL.
 *
 * Both calls:
 *   - touch no byte outside [d_buf, d_buf + buf_len) or d_out[0, out_cap);
 *   - write the last partial 16-byte chunk of any output bytewise;
 *   - are stream-ordered and allocate nothing;
 *   - wait on no other workgroup: there is no look-back spin;
 *   - make a number of launches that depends on neither the data nor K (pack:
 *     the plans' description into scratch, sizes, one scan, pack; decode: status
 *     reset, the description, parse, one segmented scan of all string slots in
 *     three launches, copy);
 *   - do work bounded by the bytes plus ncalls * the largest fixed part, on any
 *     input.  A frame that does not lie whole inside its tile's image window is
 *     written (read) from global memory: head and fixed part by its lane, chars
 *     by the whole workgroup, as every other frame's chars are.
 *
 * Refused with nothing launched, in this order: a NULL required pointer (plans,
 * d_cols, d_str_offs, h_cap, d_index, d_scratch; pack: d_offs, d_total, and
 * d_method, d_out with calls; decode: h_str_cap, d_codes, d_ends, d_method with
 * calls, d_buf and d_offs with frames), nplans outside 1..16, nframes > ncalls,
 * buf_len or out_cap >= 4 GiB, ncalls >= 2^32 (SRPC_E_INVALID; checked before
 * any plan is read); a fixed plan with a prefix under 4 bytes (request) or 5
 * (reply), a string plan with a prefix under 1 byte or more than
 * SRPC_FRAMES_MAX_STRINGS strings, more than SRPC_FRAMES_MIXED_MAX_FIELDS leaves
 * (SRPC_E_UNSUPPORTED); a misaligned d_buf, d_out or column (16), offsets array,
 * index, d_total, d_ends or scratch (8), d_offs (4) (SRPC_E_ALIGN); too little
 * scratch (SRPC_E_CAPACITY). */
int srpc_frames_mixed_var_scratch_bytes(const srpc_plan* const* plans, int nplans, uint64_t ncalls, uint64_t* out);
int srpc_frames_mixed_var_tile(const srpc_plan* const* plans, int nplans, uint32_t* calls_per_tile,
                               uint32_t* image_bytes);
int srpc_frames_pack_requests_mixed_var(const srpc_plan* const* req_plans, int nplans,
                                        const void* const* const* d_cols,
                                        const uint64_t* const* const* d_str_offs, const uint64_t* h_first,
                                        const uint64_t* h_cap, const uint8_t* d_method, const void* d_index,
                                        uint64_t ncalls, uint8_t* d_out, uint64_t out_cap,
                                        uint32_t* d_offs /* ncalls + 1 */, uint64_t* d_total,
                                        srpc_unpack_status* d_status, void* d_scratch, uint64_t scratch_bytes,
                                        void* stream);
int srpc_frames_unpack_replies_mixed_var(const srpc_plan* const* reply_plans, int nplans, const uint8_t* d_buf,
                                         uint64_t buf_len, const uint32_t* d_offs, uint64_t nframes,
                                         const uint8_t* d_method, const void* d_index, uint64_t ncalls,
                                         uint8_t unanswered_code, void* const* const* d_cols,
                                         uint64_t* const* const* d_str_offs, const uint64_t* const* h_str_cap,
                                         const uint64_t* h_first, const uint64_t* h_cap, uint8_t* d_codes,
                                         uint64_t* d_ends, srpc_unpack_status* d_status, void* d_scratch,
                                         uint64_t scratch_bytes, void* stream);

/* ---- batches of calls of several methods in call order, each plan's calls in
 * columns or in a struct array (client side; added within ABI 8) ----------------
 * srpc_frames_pack_requests_mixed_var and srpc_frames_unpack_replies_mixed_var
 * with, per plan, the choice srpc_frames_*_mixed_aos offers for all plans at
 * once: one device array of the caller's own structs in place of the plan's
 * columns.  The arguments are the _mixed_var calls' plus the struct-array
 * arrays of the _mixed_aos calls (d_recs, h_stride, h_leaf_offs; h_fill on the
 * decode), all host arrays of K entries.  The contract is the union of the two
 * sections above, per plan, and nothing new.
 *
 * Plan k is a RECORD plan exactly when h_stride[k] != 0.  It must be a
 * fixed-size plan with a framed prefix; its calls live in d_recs[k] as the
 * section "from struct arrays" states (16-byte aligned array, h_stride[k] bytes
 * a struct, leaf f at byte h_leaf_offs[k][f], natural alignment, no two leaves
 * sharing a byte, none past the stride; call i's struct is element h_first[k] +
 * rank(i), h_cap[k] the elements the array has).  Its d_cols[k], d_str_offs[k]
 * and h_str_cap[k] are not read and may be NULL.
 * Every other plan is a COLUMN plan, fixed-size or string, exactly as the
 * _mixed_var calls take it; its d_recs[k], h_leaf_offs[k] and h_fill[k] are not
 * read.  Any combination of kinds in any plan order is one valid call, all of
 * one kind included.  K, d_method, rank(i), BAD calls and the index of
 * srpc_frames_mixed_index are unchanged.
 *
 * srpc_frames_pack_requests_mixed_legs: the output bytes, d_offs, *d_total, the
 * status, the handling of BAD calls and the out_cap rule are
 * srpc_frames_pack_requests_mixed_var's on the same values: the frames lie back
 * to back in call order, each byte-identical to `BE32 | pack_request` of the
 * scalar packer, whichever form its plan's fields live in.  Of a record plan
 * only leaf bytes of the chunk's own structs are read; h_stride[k] is any value
 * below 2^32.  Given the RESPONSE plans, d_method = d_class and the index a
 * request decode wrote, it is a server's ordered reply pack, as the calls above.
 *
 * srpc_frames_unpack_replies_mixed_legs: d_codes, the flags, first_bad_record,
 * d_ends, the string offsets and unanswered_code are
 * srpc_frames_unpack_replies_mixed_var's on the same input (string slots are
 * numbered over the string plans as there), and a column plan's columns are
 * written as that call writes them.  A record plan's structs follow
 * srpc_frames_unpack_replies_mixed_aos: h_fill[k] is h_stride[k] <= 256 host
 * bytes, copied during the call; every struct of the chunk's calls that is not
 * BAD is written whole, exactly once, and never read -- leaf bytes from a full
 * frame, zero for any other frame and for calls nframes <= i < ncalls, every
 * other byte from h_fill[k]; no byte outside the plan's elements of this chunk
 * is written and nothing is written for a BAD call.
 *
 * Scratch: srpc_frames_mixed_legs_scratch_bytes(plans of that call, h_stride,
 * ncalls), 16-byte aligned: the _mixed_var layout, then the record plans'
 * per-struct-byte source tables and fills (3 S16 + 16 bytes per record plan,
 * S16 = h_stride[k] rounded up to 16), which the decode writes there by
 * by-value launches: no host copy outlives the call.  A stride above 256, which
 * only a pack takes, counts no table; h_stride == NULL sizes a call without
 * record plans.
 *
 * Both calls are stream-ordered, allocate nothing, wait on nothing on the host
 * or the device and can be captured.  Their launches are the _mixed_var calls'
 * (the decode's: plus one per 2 KiB of tables and fills) and depend on neither
 * the data nor the order of the plans; work is bounded by the bytes plus ncalls
 * * the largest fixed part, on any input.
 *
 * Tile rule.  A workgroup of the pack takes srpc_frames_mixed_var_tile's calls
 * and image window.  A workgroup of the decode takes
 * srpc_frames_mixed_legs_tile's: the record plans' tables and fills lie in the
 * tail of the 32 KiB image, so the image window is 32 KiB minus their bytes and
 * the calls per tile are 256, or the power of two >= 16 whose frames without
 * their chars fit that window.  The workgroup's dynamic LDS is that of the
 * _mixed_var decode, whatever the record plans.  Without record plans both are
 * srpc_frames_mixed_var_tile's values, and both calls launch the _mixed_var
 * calls' own kernels.  The decode stages and judges as the
 * _mixed_var kernel; a lane of a column plan stores its fields and string
 * lengths, a lane of a record plan leaves where its leaves are, and the
 * workgroup then writes the record plans' slices of the tile as whole 16-byte
 * pieces, as the _mixed_aos kernel does (a full frame that a long string pushed
 * out of the window is read from d_buf).
 *
 * Refused with nothing launched, in this order:
 *   1. SRPC_E_INVALID (before any plan is read): the _mixed_var calls' NULL and
 *      range checks with d_recs, h_stride, h_leaf_offs (decode: h_fill) among
 *      the pointers; h_stride[k] >= 2^32; for a record plan a NULL
 *      h_leaf_offs[k] (decode: h_fill[k]), or a NULL d_recs[k] where h_cap[k]
 *      leaves an element;
 *   2. SRPC_E_UNSUPPORTED: what the _mixed_var calls refuse so; a string plan
 *      with a non-zero stride; a decode stride above 256;
 *   3. SRPC_E_INVALID: a record plan's leaves overlapping or past the stride;
 *   4. SRPC_E_ALIGN: d_buf, d_out, an array, d_scratch (16), the index, d_total,
 *      d_ends (8), d_offs (4), an offset or stride against its leaf's size; then
 *      the column plans' pointers as the _mixed_var calls check them (a NULL
 *      one: SRPC_E_INVALID);
 *   5. SRPC_E_CAPACITY: scratch_bytes. */
int srpc_frames_mixed_legs_scratch_bytes(const srpc_plan* const* plans, int nplans,
                                         const uint64_t* h_stride /* may be NULL */, uint64_t ncalls,
                                         uint64_t* out);
/* Testing hook: calls per workgroup tile of a decode with these plans and the
 * bytes of its LDS image window (h_stride may be NULL: no record plan). */
int srpc_frames_mixed_legs_tile(const srpc_plan* const* plans, int nplans, const uint64_t* h_stride,
                                uint32_t* calls_per_tile, uint32_t* image_bytes);
int srpc_frames_pack_requests_mixed_legs(const srpc_plan* const* req_plans, int nplans,
                                         const void* const* const* d_cols,
                                         const uint64_t* const* const* d_str_offs, const void* const* d_recs,
                                         const uint64_t* h_stride, const uint32_t* const* h_leaf_offs,
                                         const uint64_t* h_first, const uint64_t* h_cap, const uint8_t* d_method,
                                         const void* d_index, uint64_t ncalls, uint8_t* d_out, uint64_t out_cap,
                                         uint32_t* d_offs /* ncalls + 1 */, uint64_t* d_total,
                                         srpc_unpack_status* d_status, void* d_scratch, uint64_t scratch_bytes,
                                         void* stream);
int srpc_frames_unpack_replies_mixed_legs(const srpc_plan* const* reply_plans, int nplans, const uint8_t* d_buf,
                                          uint64_t buf_len, const uint32_t* d_offs, uint64_t nframes,
                                          const uint8_t* d_method, const void* d_index, uint64_t ncalls,
                                          uint8_t unanswered_code, void* const* const* d_cols,
                                          uint64_t* const* const* d_str_offs, const uint64_t* const* h_str_cap,
                                          void* const* d_recs, const uint64_t* h_stride,
                                          const uint32_t* const* h_leaf_offs, const void* const* h_fill,
                                          const uint64_t* h_first, const uint64_t* h_cap, uint8_t* d_codes,
                                          uint64_t* d_ends, srpc_unpack_status* d_status, void* d_scratch,
                                          uint64_t scratch_bytes, void* stream);

/* ---- batches of request frames of several methods with string bodies, in
 * arrival order (server side; added within ABI 8) --------------------------------
 * srpc_frames_unpack_requests_mixed with string plans allowed beside the
 * fixed-size ones: the union of the two sections above, and the mirror of
 * srpc_frames_pack_requests_mixed_var.  srpc_frames_unpack_requests_mixed keeps
 * refusing string plans.
 *
 * Plans: K = nplans = 1..16 REQUEST plans, each of one of the two kinds the
 * *_mixed_var calls take -- a fixed-size plan with the framed prefix `BE32(payload)
 * | str(method) | str(Req::name)`, or a string plan (SRPC_PATH_VAR, at most
 * SRPC_FRAMES_MAX_STRINGS strings) with the unframed prefix `str(method) |
 * str(Req::name)`; at most SRPC_FRAMES_MIXED_MAX_FIELDS leaves in all; buf_len
 * under 4 GiB, nframes under 2^32.
 * Frames: frame i is bytes [d_offs[i], end_i) of d_buf, end_i = d_offs[i + 1], or
 * buf_len for the last frame.
 *   d_class[i] (u8, device, out) is exactly what srpc_frames_classify writes for
 *     the same plans and input; the first matching plan wins.  A fixed plan
 *     matches when the frame's length is F_k and its first prefix_len_k bytes are
 *     the plan's prefix.  A string plan matches when the length is >= 4 + the
 *     least payload (prefix, fixed fields, 8 per string), BE32 == len - 4, the
 *     payload starts with the plan's prefix and the walk of its fields ends
 *     exactly at end_i, each string's u64 length being read from the frame and
 *     compared as `len > end - cursor`, so 2^63 and 2^64 - 1 cannot wrap.
 *     Everything else is SRPC_FRAME_UNKNOWN: offsets out of order, an end past
 *     buf_len, a frame under 4 bytes, a string that runs past the end, trailing
 *     bytes after the walk.
 *   rank(i) is the number of frames j < i with the same class.  A frame of class
 *     k goes to element e = h_first[k] + rank(i): fixed leaves to d_cols[k][f][e],
 *     a string leaf's chars back to back into d_cols[k][f] in element order.
 *     d_cols, d_str_offs, h_str_cap, h_first (NULL = zeros) and h_cap are those
 *     of srpc_frames_unpack_replies_mixed_var, and the string offsets follow its
 *     rule: absolute in d_str_offs[k][f], entry 0 written as 0 when h_first[k] ==
 *     0, otherwise continuing from entry h_first[k]; entries h_first[k] + 1 ..
 *     h_first[k] + count_k are written, never past entry h_cap[k].  d_ends[s]
 *     (device, one u64 per string slot, numbered over the plans and then their
 *     string leaves) is the end offset of slot s.  No char at or past
 *     h_str_cap[k][f] is written while the offsets still count every frame: an
 *     overflow shows as d_ends[s] > capacity.
 *   A frame whose element would be at or past h_cap[k] keeps its class and
 *     writes no column or offsets element: SRPC_STATUS_BOUNDS, first_bad_record
 *     the smallest such i.  Nothing is written for an unknown frame.
 *   d_index (opaque, 8-byte aligned, srpc_frames_mixed_index_bytes(nframes, K))
 *     receives the index srpc_frames_mixed_index builds over d_class: it serves
 *     srpc_frames_mixed_ranks and the reply pack.  d_counts[0..K] are as in
 *     srpc_frames_unpack_requests_mixed.
 *   Scratch: srpc_frames_mixed_var_scratch_bytes(req_plans, K, nframes), 8-byte
 *     aligned.
 *   - no byte outside [d_buf, d_buf + buf_len) is read;
 *   - no column, offsets or char byte is written but the frames' own; the last
 *     partial 16-byte chunk of any output is written bytewise;
 *   - *d_status (may be NULL) is reset by the call;
 *   - the call is stream-ordered, allocates nothing and waits on no other
 *     workgroup; its launches (status reset, the plans' description into
 *     scratch, classify, the index's two, parse, the slot scan's three, copy)
 *     depend neither on the data nor on K, so it can be captured.  The stream
 *     is read twice: a frame's rank needs the class of every frame before it;
 *   - work is bounded by buf_len + nframes * (K prefix compares + the largest
 *     fixed part) on any input: a frame that does not lie whole inside its
 *     tile's image window is judged and parsed from global memory by its lane,
 *     which touches its fixed part and its length words only.
 *
 * Refused with nothing launched, in this order: a NULL required pointer
 * (req_plans, d_cols, d_str_offs, h_str_cap, h_cap, d_index, d_counts, d_ends,
 * d_scratch; d_buf, d_offs, d_class when nframes > 0), nplans outside 1..16,
 * buf_len >= 4 GiB or nframes >= 2^32 (SRPC_E_INVALID; checked before any plan
 * is read); a fixed plan with a prefix under 4 bytes, a string plan with a prefix
 * under 1 byte or more than SRPC_FRAMES_MAX_STRINGS strings, more than
 * SRPC_FRAMES_MIXED_MAX_FIELDS leaves (SRPC_E_UNSUPPORTED); a misaligned d_buf or
 * column (16), offsets array, index, d_counts, d_ends or scratch (8), d_offs (4)
 * (SRPC_E_ALIGN); an index or a scratch that is too small (SRPC_E_CAPACITY).
 *
 * The ordered reply pack is srpc_frames_pack_requests_mixed_var itself: called
 * with the RESPONSE plans (of the same two kinds), the response columns,
 * d_method = d_class and the d_index this call wrote, it writes the reply stream
 * in arrival order, zero bytes for an unknown frame. */
int srpc_frames_unpack_requests_mixed_var(
    const srpc_plan* const* req_plans, int nplans,
    const uint8_t* d_buf, uint64_t buf_len, const uint32_t* d_offs, uint64_t nframes,
    void* const* const* d_cols, uint64_t* const* const* d_str_offs,
    const uint64_t* const* h_str_cap, const uint64_t* h_first, const uint64_t* h_cap,
    uint8_t* d_class /* nframes, out */, void* d_index, uint64_t index_bytes,
    uint64_t* d_counts /* nplans + 1, out */, uint64_t* d_ends /* one per string slot, out */,
    srpc_unpack_status* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream);

/* ---- batches of request frames of several methods in arrival order, each plan's
 * requests into columns or into a struct array (server side; added within ABI 8) --
 * srpc_frames_unpack_requests_mixed_var with, per plan, the choice
 * srpc_frames_unpack_requests_mixed_aos offers for all plans at once: one device
 * array of the caller's own structs in place of the plan's columns.  It is the
 * mirror of srpc_frames_pack_requests_mixed_legs.  The arguments are the
 * _mixed_var request call's plus d_recs, h_stride, h_leaf_offs and h_fill of the
 * _mixed_aos request call, all host arrays of K entries.  The contract is the
 * union of the two sections above ("with string bodies, in arrival order" and
 * "into struct arrays, in arrival order"), per plan, and nothing new.
 *
 * Plan k is a RECORD plan exactly when h_stride[k] != 0, the rule of the
 * _mixed_legs client calls.  It must be a fixed-size plan with a framed prefix
 * and h_stride[k] <= 256; its d_cols[k], d_str_offs[k] and h_str_cap[k] are not
 * read and may be NULL.  Every other plan is a COLUMN plan, fixed-size or
 * string, exactly as srpc_frames_unpack_requests_mixed_var takes it; its
 * d_recs[k], h_leaf_offs[k] and h_fill[k] are not read.  Any combination of
 * kinds in any plan order is one valid call, all of one kind included.
 *
 *   d_class, d_index, d_counts and d_ends are byte-identical to what
 *     srpc_frames_unpack_requests_mixed_var writes for the same plans and bytes
 *     (string slots are numbered over the string plans, as there): the class is
 *     srpc_frames_classify's, the first matching plan wins.  A frame whose
 *     element h_first[k] + rank(i) would be at or past h_cap[k] keeps its class
 *     and writes nothing: SRPC_STATUS_BOUNDS, first_bad_record the smallest such
 *     i; *d_status (may be NULL) is reset by the call.
 *   A column plan's fixed leaves, chars and absolute string offsets are written
 *     as srpc_frames_unpack_requests_mixed_var writes them, the continuation
 *     from entry h_first[k] included.
 *   A record plan's structs are written as srpc_frames_unpack_requests_mixed_aos
 *     writes them: element h_first[k] + rank(i), when below h_cap[k], is written
 *     whole, exactly once, and never read -- leaf bytes from the frame, every
 *     other byte from h_fill[k] (h_stride[k] host bytes, copied during the
 *     call).  Nothing is written for an unknown frame or an element past the
 *     cap, and no byte outside the plan's elements of this batch is written.
 *   - no byte outside [d_buf, d_buf + buf_len) is read, whatever d_offs holds:
 *     the decode pass checks every extent again and does not trust d_class;
 *   - the call is stream-ordered, allocates nothing and waits on no other
 *     workgroup; its launches are the _mixed_var request call's plus one per
 *     2 KiB of tables and fills, and depend on neither the data nor the order
 *     of the plans, so it can be captured.
 *
 * Scratch: srpc_frames_mixed_legs_scratch_bytes(req_plans, K, h_stride, nframes),
 * 16-byte aligned.  Tile rule: both passes take srpc_frames_mixed_legs_tile's
 * frames per tile, called with the request plans, and the parse pass its image
 * window: the record plans' tables and fills lie in the tail of the 32 KiB
 * image, so the workgroup's dynamic LDS is that of the _mixed_var request
 * decode.  A lane of a column plan walks and stores its frame as that decode's
 * does; a lane of a record plan leaves where its frame is, and the workgroup
 * writes the record plans' slices of the tile as whole 16-byte pieces with
 * non-temporal stores (a frame that a long string pushed out of the window is
 * read from d_buf, at most F_k bytes, its extent checked again).  Without a
 * record plan the call launches the _mixed_var request call's own kernels.
 *
 * Refused with nothing launched, in the order of
 * srpc_frames_unpack_replies_mixed_legs:
 *   1. SRPC_E_INVALID (before any plan is read): the _mixed_var request call's
 *      NULL and range checks with d_recs, h_stride, h_leaf_offs and h_fill among
 *      the pointers; h_stride[k] >= 2^32; for a record plan a NULL
 *      h_leaf_offs[k] or h_fill[k], or a NULL d_recs[k] where h_cap[k] leaves an
 *      element;
 *   2. SRPC_E_UNSUPPORTED: what the _mixed_var request call refuses so; a string
 *      plan with a non-zero stride; a stride above 256;
 *   3. SRPC_E_INVALID: a record plan's leaves overlapping or past the stride;
 *   4. SRPC_E_ALIGN: d_buf, an array, d_scratch (16), the index, d_counts, d_ends
 *      (8), d_offs (4), an offset or stride against its leaf's size; then the
 *      column plans' pointers as the _mixed_var request call checks them (a NULL
 *      one: SRPC_E_INVALID);
 *   5. SRPC_E_CAPACITY: index_bytes or scratch_bytes.
 *
 * The ordered reply pack needs no call of its own: it is
 * srpc_frames_pack_requests_mixed_legs with the RESPONSE plans (each in columns
 * or in a struct array, whatever its request plan's kind), d_method = d_class
 * and the d_index this call wrote; it writes the reply stream in arrival order,
 * zero bytes for an unknown frame. */
int srpc_frames_unpack_requests_mixed_legs(
    const srpc_plan* const* req_plans, int nplans,
    const uint8_t* d_buf, uint64_t buf_len, const uint32_t* d_offs, uint64_t nframes,
    void* const* const* d_cols, uint64_t* const* const* d_str_offs, const uint64_t* const* h_str_cap,
    void* const* d_recs, const uint64_t* h_stride, const uint32_t* const* h_leaf_offs, const void* const* h_fill,
    const uint64_t* h_first, const uint64_t* h_cap,
    uint8_t* d_class /* nframes, out */, void* d_index, uint64_t index_bytes,
    uint64_t* d_counts /* nplans + 1, out */, uint64_t* d_ends /* one per string slot, out */,
    srpc_unpack_status* d_status, void* d_scratch, uint64_t scratch_bytes, void* stream);

/* ---- utilities--------------------------------------------------------------*/

/* Synthetic input of SURVEY.md §8c: nfields int32 columns, record i field f =
 * low 32 bits of splitmix64 draw number (first_record + i) * nfields + f + 1
 * from state `seed`.  Used by bench.py to build inputs in HBM. */
int srpc_gpu_fill_splitmix_i32(int32_t* const* d_cols, uint32_t nfields, uint64_t n,
                               uint64_t seed, uint64_t first_record, void* stream);

/* Host-terminated pack / unpack (ABI 7): columns and wire bytes in HOST
 * memory (pinned for overlap), as the reference's batches start and end --
 * the packer's byte vector written to the socket (transport.hpp:94-123) and
 * the received bytes the generated unpack reads (calculator_srpc.cpp:19-22).
 * A fixed-width batch moves in chunks of `chunk_records` through a ring of
 * `depth` device buffers carved from d_scratch (256-byte aligned, at least
 * srpc_plan_host_scratch_bytes), pipelined over internal streams (H2D /
 * kernels / D2H), ordered after the work on `stream` and before what is
 * enqueued on it later.  The results equal srpc_gpu_pack / srpc_gpu_unpack
 * on the whole batch, statuses included (first_bad_record is batch-relative).
 * chunk_records == 0 is the direct mode: when every host buffer is page-
 * locked and device-mapped (hipHostMalloc, hipHostRegister, torch pin_memory)
 * the kernels read and write them in place over PCIe, both directions at
 * once, no scratch, no copies; each buffer's pinned allocation must cover its
 * n records (else SRPC_E_INVALID, nothing launched).  Every argument is
 * checked before anything is enqueued.  The chunked mode borrows three
 * streams and their events from a per-device pool (created on first use, kept
 * for the process, grown only by calls in flight at once); unlike the other
 * calls it is not meant for hipGraph capture.  An error part way through the
 * chunked ring still orders everything the call enqueued before `stream`'s
 * later work.  String schemas: SRPC_E_UNSUPPORTED. */
int srpc_plan_host_scratch_bytes(const srpc_plan* plan, uint64_t chunk_records, uint32_t depth,
                                 uint64_t* out);
int srpc_gpu_pack_host(const srpc_plan* plan, const void* const* h_cols, uint64_t n, uint8_t* h_wire,
                       uint64_t wire_cap, uint64_t chunk_records, uint32_t depth, void* d_scratch,
                       uint64_t scratch_bytes, void* stream);
int srpc_gpu_unpack_host(const srpc_plan* plan, const uint8_t* h_wire, uint64_t wire_len, uint64_t n,
                         void* const* h_cols, uint64_t chunk_records, uint32_t depth, void* d_scratch,
                         uint64_t scratch_bytes, srpc_unpack_status* d_status, void* stream);

/* Measurement hook (bench.py): the data-path kernels launched by the NEXT
 * srpc_gpu_pack / _unpack / _pack_var / _unpack_var /
 * srpc_frames_unpack_replies / _unpack_replies_aos / _unpack_replies_var /
 * srpc_frames_mixed_index /
 * _pack_requests_mixed / _unpack_replies_mixed / _unpack_requests_mixed /
 * _pack_requests_mixed_var / _unpack_replies_mixed_var /
 * _unpack_requests_mixed_var call made on this host
 * thread record the begin timestamp of the first kernel into `start_event`
 * and the end timestamp of the last into `stop_event` (hipEvent_t handles
 * created with timing enabled; either may be NULL), taken from the dispatch
 * packets themselves (hipExtLaunchKernel) -- kernel-only time, the interval
 * rocprofv3 --kernel-trace reports.  Status-reset launches are not timed.
 * The hook is consumed by that one call, whatever it returns. */
int srpc_time_next_call(void* start_event, void* stop_event);

const char* srpc_status_string(int code);
int srpc_gpu_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* SRPC_GPU_H */
