/*
 * ibu_hip.h — C ABI of libibu_hip.so, the MI355X (gfx950) batch record-stream + 2-bit codec
 * path for the IBU binary format.
 *
 * This is the drop-in boundary.  The reference (noamteyssier/ibu, Rust) has no FFI of its
 * own; its boundary is the crate's public API (src/lib.rs:178-181).  Every entry point below
 * names the reference item it stands behind, so that a Rust `extern "C"` shim (source in
 * bindings/rust/, walkthrough in INTEGRATION.md) can re-create `Header / Record / Reader /
 * Writer / MmapReader / ParallelProcessor` on top of it.
 *
 * Conventions
 *   - plain C types only: pointers, sizes, fixed-width ints.  No C++/torch types.
 *   - every fallible function returns int32_t: 0 = IBU_OK, 1..10 = the ten IbuError variants
 *     in declaration order (src/error.rs:56-128), 11.. = codec / argument errors that the
 *     reference expresses as panics or leaves to `bitnuc`, >=100 = HIP runtime.
 *   - the payload of the failing call (expected/actual, pos, idx/max, errno, message) is
 *     kept per calling thread and read with ibu_last_error().
 *   - nothing throws or aborts across this boundary.
 *   - host pointers are `h_` / unprefixed; device pointers are prefixed `d_`.  `stream` is a
 *     hipStream_t passed as void* (NULL = the context's own stream).  Launch functions are
 *     asynchronous, allocate nothing and never synchronise: they can be captured into a hipGraph and replayed
 *     (tests/test_gpu_parity.py::test_launch_functions_can_be_captured_into_a_hip_graph).
 *   - the caller owns every buffer it passes; the library owns only what *_open/_create
 *     returned, until the matching *_close/_destroy.
 *
 * 2-bit codec convention (the reference only documents the table, src/constructs/record.rs:19-27;
 * its README defers to the `bitnuc` crate which is not a dependency — parity for the codec is
 * therefore UNPINNED):
 *   A/a=00 C/c=01 G/g=10 T/t=11; base i of a sequence occupies bits [2i, 2i+1] (first base in
 *   the least-significant bits: "ACGT" -> 0b11100100); len in 1..=32; bits >= 2*len are
 *   ignored on unpack and written as zero on pack; unpack emits upper-case ASCII; any other
 *   input byte on pack is IBU_ERR_INVALID_BASE.
 */
#ifndef IBU_HIP_H
#define IBU_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- constants (src/constructs/header.rs:5-7, record.rs:3, io/reader.rs:14, io/mmap.rs:284) */
#define IBU_MAGIC 0x21554249u /* "IBU!" little-endian */
#define IBU_VERSION 2u
#define IBU_HEADER_SIZE 32
#define IBU_RECORD_SIZE 24
#define IBU_DEFAULT_BUFFER_SIZE (48 * 1024 * IBU_RECORD_SIZE) /* 1 179 648 B */
#define IBU_BATCH_SIZE (1024 * 1024)                          /* records per parallel batch */
#define IBU_MAX_SEQ_LEN 32
#define IBU_FLAG_SORTED 1ull

/* ---- POD types, layout-identical to the #[repr(C)] structs ---------------------------- */
typedef struct ibu_header { /* src/constructs/header.rs:48-61 */
  uint32_t magic;
  uint32_t version;
  uint32_t bc_len;
  uint32_t umi_len;
  uint64_t flags;
  uint8_t reserved[8];
} ibu_header_t;

typedef struct ibu_record { /* src/constructs/record.rs:58-66 */
  uint64_t barcode;
  uint64_t umi;
  uint64_t index;
} ibu_record_t;

/* ---- status codes ---------------------------------------------------------------------- */
enum {
  IBU_OK = 0,
  IBU_ERR_IO = 1,               /* IbuError::Io                 error.rs:58  detail.os_errno        */
  IBU_ERR_NIFFLER = 2,          /* IbuError::Niffler            error.rs:62  (decompression)        */
  IBU_ERR_INVALID_MAGIC = 3,    /* InvalidMagicNumber{expected,actual}       detail.a=exp, .b=act   */
  IBU_ERR_TRUNCATED_RECORD = 4, /* TruncatedRecord{pos}                      detail.a=pos           */
  IBU_ERR_INVALID_VERSION = 5,  /* InvalidVersion{expected,actual}           detail.a=exp, .b=act   */
  IBU_ERR_INVALID_BC_LEN = 6,   /* InvalidBarcodeLength(u32)                 detail.a=len           */
  IBU_ERR_INVALID_UMI_LEN = 7,  /* InvalidUmiLength(u32)                     detail.a=len           */
  IBU_ERR_INVALID_MAP_SIZE = 8, /* InvalidMapSize                                                   */
  IBU_ERR_INVALID_INDEX = 9,    /* InvalidIndex{idx,max}                     detail.a=idx, .b=max   */
  IBU_ERR_PROCESS = 10,         /* Process(Box<dyn Error>)   user processor returned non-zero:
                                   detail.a = that value                                            */
  IBU_ERR_INVALID_BASE = 11,    /* codec: byte outside ACGTacgt; detail.a = first bad record,
                                   detail.b = number of offending records                           */
  IBU_ERR_SEQ_LEN = 12,         /* codec: len outside 1..=32; detail.a=len                          */
  IBU_ERR_INVALID_ARG = 13,     /* NULL/size misuse — where the reference would panic
                                   (Header::from_bytes on a wrong length, header.rs:226)            */
  IBU_ERR_HIP = 100,            /* any hipError_t != hipSuccess; detail.a = hipError_t              */
  IBU_ERR_NO_DEVICE = 101       /* no usable gfx950 device: the device path FAILS, never falls back */
};

typedef struct ibu_error_detail {
  int32_t code;
  int32_t os_errno;
  uint64_t a;
  uint64_t b;
  char message[232]; /* Display text in the reference's wording (error.rs:57-127) */
} ibu_error_detail_t;

/* Detail of the last failing call made by the calling thread. */
void ibu_last_error(ibu_error_detail_t* out);
/* Static name of a status code ("InvalidMagicNumber", ...). */
const char* ibu_status_name(int32_t status);
/* Library version string and ABI revision (bumped on any signature change). */
const char* ibu_version(void);
uint32_t ibu_abi_revision(void);
/* Free a buffer returned by ibu_load_to_vec / ibu_writer_into_inner. */
void ibu_free(void* p);

/* ======================================================================================= */
/* A2  Header                                                     src/constructs/header.rs */
/* ======================================================================================= */
void ibu_header_init(ibu_header_t* h, uint32_t bc_len, uint32_t umi_len); /* Header::new :84-93    */
void ibu_header_set_sorted(ibu_header_t* h);                              /* set_sorted  :111-113  */
int32_t ibu_header_sorted(const ibu_header_t* h);                         /* sorted      :130-132  */
int32_t ibu_header_validate(const ibu_header_t* h);                       /* validate    :167-187  */
int32_t ibu_header_from_bytes(const uint8_t* bytes, size_t len, ibu_header_t* out); /* :226-228    */
int32_t ibu_header_as_bytes(const ibu_header_t* h, uint8_t* out, size_t cap);       /* :203-205    */

/* ======================================================================================= */
/* A1  Record                                                     src/constructs/record.rs */
/* ======================================================================================= */
int32_t ibu_record_from_bytes(const uint8_t* bytes, size_t len, ibu_record_t* out); /* :130-132    */
int32_t ibu_record_as_bytes(const ibu_record_t* r, uint8_t* out, size_t cap);       /* :108-110    */
/* derive(Ord): lexicographic (barcode, umi, index) -> -1/0/+1                         :58         */
int32_t ibu_record_cmp(const ibu_record_t* a, const ibu_record_t* b);

/* ======================================================================================= */
/* A3/A4  Writer<W>                                                    src/io/writer.rs     */
/* ======================================================================================= */
typedef struct ibu_writer ibu_writer_t;
/* W: Write as two callbacks.  write must consume all `len` bytes or return non-zero (errno). */
typedef int32_t (*ibu_write_fn)(void* user, const uint8_t* data, size_t len);
typedef int32_t (*ibu_flush_fn)(void* user);

/* Writer::new(inner, header) :129-143 — header written immediately, NOT validated (quirk Q2).
 * header == NULL gives Writer::new_headless :169-179. */
int32_t ibu_writer_open_callback(ibu_write_fn wr, ibu_flush_fn fl, void* user,
                                 const ibu_header_t* header, ibu_writer_t** out);
int32_t ibu_writer_open_path(const char* path, const ibu_header_t* header, ibu_writer_t** out); /* from_path :556-559 */
int32_t ibu_writer_open_fd(int fd, const ibu_header_t* header, ibu_writer_t** out); /* from_stdout :587-589 (fd 1) */
int32_t ibu_writer_open_mem(const ibu_header_t* header, ibu_writer_t** out);        /* Writer<Vec<u8>>            */

int32_t ibu_writer_write_record(ibu_writer_t* w, const ibu_record_t* r);                /* :260-273 */
int32_t ibu_writer_write_batch(ibu_writer_t* w, const ibu_record_t* recs, size_t n);    /* :315-351 */
int32_t ibu_writer_ingest(ibu_writer_t* w, ibu_writer_t* other_mem);                    /* :477-482 */
int32_t ibu_writer_finish(ibu_writer_t* w);                                             /* :429-433 */
uint64_t ibu_writer_records_written(const ibu_writer_t* w);                             /* :207-209 */
/* Bytes the inner sink has received so far (what `into_inner()` of a Vec<u8> writer would hold). */
int32_t ibu_writer_mem_view(const ibu_writer_t* w, const uint8_t** data, size_t* len);
/* into_inner :507-511 — NO flush (ManuallyDrop skips Drop); frees the writer; mem writers hand
 * their bytes to the caller (release with ibu_free), other sinks return data=NULL. */
int32_t ibu_writer_into_inner(ibu_writer_t* w, uint8_t** data, size_t* len);
/* Drop :519-523 — finish().ok(), errors swallowed, then free. */
void ibu_writer_close(ibu_writer_t* w);

/* ======================================================================================= */
/* A5  Reader<R>                                                       src/io/reader.rs     */
/* ======================================================================================= */
typedef struct ibu_reader ibu_reader_t;
/* R: Read as one callback: fill up to cap bytes, *got = bytes read (0 = EOF); non-zero = errno. */
typedef int32_t (*ibu_read_fn)(void* user, uint8_t* dst, size_t cap, size_t* got);

/* Reader::new :152-176 — read_exact 32 B, validate. */
int32_t ibu_reader_open_callback(ibu_read_fn rd, void* user, ibu_reader_t** out);
/* Reader::new(Cursor<&[u8]>) — bytes are borrowed, not copied. */
int32_t ibu_reader_open_mem(const uint8_t* data, size_t len, ibu_reader_t** out);
/* Reader::from_path :345-352 — sniffs the format by magic bytes (niffler's role): gzip (BGZF input is inflated
 * block-parallel), bzip2, xz and zstd are decoded (the last three through the host's libbz2 / liblzma / libzstd,
 * bound at run time; IBU_ERR_NIFFLER if the library is absent); plain files pass through. */
int32_t ibu_reader_open_path(const char* path, ibu_reader_t** out);
int32_t ibu_reader_open_fd(int fd, ibu_reader_t** out); /* from_stdin :389-396 (fd 0), sniffs too */

int32_t ibu_reader_header(const ibu_reader_t* r, ibu_header_t* out);   /* header()    :244-246 */
int32_t ibu_reader_read_batch(ibu_reader_t* r, int32_t* has_data);     /* read_batch  :218-242 */
/* Iterator::next :279-306 — *got = 1 and *out filled, or *got = 0 (None); error = Some(Err). */
int32_t ibu_reader_next(ibu_reader_t* r, ibu_record_t* out, int32_t* got);
/* Zero-copy view of the records left in the current buffer and how many to mark consumed
 * (feeds the device ring; no reference equivalent — Reader keeps `buffer` private). */
int32_t ibu_reader_buffered(ibu_reader_t* r, const ibu_record_t** recs, size_t* n);
int32_t ibu_reader_consume(ibu_reader_t* r, size_t n);
uint64_t ibu_reader_bytes_read(const ibu_reader_t* r);                 /* field :107-108        */
void ibu_reader_close(ibu_reader_t* r);

/* A6  load_to_vec :510-535 — uncompressed files only (quirk Q10); *records from ibu_free. */
int32_t ibu_load_to_vec(const char* path, ibu_header_t* header, ibu_record_t** records, size_t* n);

/* ======================================================================================= */
/* A7/A8  MmapReader + ParallelReader                                  src/io/mmap.rs       */
/* ======================================================================================= */
typedef struct ibu_mmap ibu_mmap_t;
int32_t ibu_mmap_open(const char* path, ibu_mmap_t** out);              /* MmapReader::new :143-161 */
int32_t ibu_mmap_clone(ibu_mmap_t* m, ibu_mmap_t** out);                /* Clone (Arc<Mmap>) :99    */
size_t ibu_mmap_len(const ibu_mmap_t* m);                               /* len    :178-180          */
int32_t ibu_mmap_header(const ibu_mmap_t* m, ibu_header_t* out);        /* header :201-203          */
/* slice :253-270 — InvalidIndex{idx:end,max:len} if start>=len || end>len || end<=start (Q7). */
int32_t ibu_mmap_slice(const ibu_mmap_t* m, size_t start, size_t end, const ibu_record_t** recs,
                       size_t* n);
const void* ibu_mmap_base(const ibu_mmap_t* m); /* Arc::ptr_eq analogue, mmap.rs:541 */
void ibu_mmap_close(ibu_mmap_t* m);

/* Static contiguous range split of mmap.rs:297-307: per = len/n, remainder to the LAST shard.
 * Used for OS threads by the reference and for GPUs / ranks by this library. */
int32_t ibu_shard_range(size_t len, size_t n_shards, size_t shard, size_t* start, size_t* end);

/* ParallelProcessor :100-190 as a C vtable.  `clone` is P: Clone (one copy per worker);
 * process_record / on_batch_complete return 0 or a non-zero user code -> IBU_ERR_PROCESS.
 * set_tid is part of the trait but is never called by process_parallel (quirk Q4). */
typedef struct ibu_processor_vtable {
  void* (*clone)(void* user);
  void (*drop)(void* user_clone);
  int32_t (*process_record)(void* user_clone, const ibu_record_t* rec);
  int32_t (*on_batch_complete)(void* user_clone); /* may be NULL: default Ok(()) */
  void (*set_tid)(void* user_clone, size_t tid);  /* may be NULL */
} ibu_processor_vtable_t;

/* process_parallel :286-332 with a HOST processor (user code, exactly the reference's
 * contract: n = 0 -> all cores, else min(n, cores); 1Mi-record batches; join in spawn order,
 * first Err wins — quirk Q12). */
int32_t ibu_mmap_process_parallel(const ibu_mmap_t* m, const ibu_processor_vtable_t* vt, void* user,
                                  size_t num_threads);

/* ======================================================================================= */
/* Device context                                                                           */
/* ======================================================================================= */
typedef struct ibu_ctx ibu_ctx_t;
/* One context per host thread and device; owns a stream, a status slot and reduce scratch.
 * Fails with IBU_ERR_NO_DEVICE when the device is absent or not gfx950. */
int32_t ibu_ctx_create(int32_t device, ibu_ctx_t** out);
void ibu_ctx_destroy(ibu_ctx_t* ctx);
int32_t ibu_ctx_device(const ibu_ctx_t* ctx);
/* Where the context's device hangs off the host and where its pinned ring landed (option "numa").  The reference's workers are
 * OS threads over one shared map (mmap.rs:308-322) and leave placement to the kernel; with a GPU per worker the copy
 * page cache -> pinned ring -> PCIe is local only if ring and feeder threads sit on the GPU's socket. */
typedef struct ibu_numa_info {
  int32_t mode;          /* option "numa": 1 auto, 0 off */
  int32_t node;          /* NUMA node of the device's PCI function; -1: the platform does not say */
  int32_t usable_cpus;   /* CPUs of that node the process may run on (what the feeder threads are pinned to when mode = 1) */
  int32_t ring_node;     /* node the pinned ring's pages are on, as the kernel reports it (move_pages); -1: no ring yet / it will not say */
  int32_t ring_placed;   /* 1: the ring was allocated under a preferred-node policy the kernel accepted */
  int32_t reserved;
  char pci_bus_id[32];   /* "0000:c1:00.0" */
  char cpulist[256];     /* the node's CPUs as sysfs spells them, "" when unknown */
} ibu_numa_info_t;
int32_t ibu_ctx_numa(const ibu_ctx_t* ctx, ibu_numa_info_t* out);
/* The lookup on its own, against any sysfs tree (sysfs_root NULL = "/sys"): *node = NUMA node of PCI function `pci_bus_id`
 * (-1 unknown), cpulist = the node's CPUs ("" unknown), *usable_cpus (nullable) = how many of them the calling thread may use. */
int32_t ibu_numa_of_pci(const char* sysfs_root, const char* pci_bus_id, int32_t* node, char* cpulist, size_t cap,
                        int32_t* usable_cpus);
void* ibu_ctx_stream(const ibu_ctx_t* ctx);        /* hipStream_t */
int32_t ibu_ctx_synchronize(ibu_ctx_t* ctx, void* stream);
int32_t ibu_device_count(int32_t* n);
/* Tuning knobs (all optional; defaults are the measured best for MI355X):
 *   "blocks_per_cu"  1..8   cap on resident 256-thread workgroups per CU for the persistent grids
 *   "sort_variant"   0..6   tile shape of the 24-byte radix passes (0 = default: 2560-record tiles; the rest are A/B shapes of the
 *                           same algorithm kept for measurement: ibu_amd/csrc/sort.hip, kSweep)
 *   "sort_compact"   0..8   compact-key passes of the sort: when at most 12 bytes of the 24-byte key vary (16/12 records
 *                           with indices below 2^32: 11) the passes move 12-byte elements instead of records, when 13 .. 16
 *                           vary, 16-byte elements.  0 = never
 *                           (24-byte passes only), 1 = default tile shape, 2..8 = A/B tile shapes (sort.hip, kCompact).
 *                           Same result either way, byte for byte.
 *   "sort_guess"     0 | 1 | k  large compact-key sorts read the records once instead of twice: a census of three sample ranges
 *                           guesses the varying bytes, the compress pass runs on the guess and takes the exact census on the
 *                           way; a guess that missed a byte is detected and the sort continues from the exact census.
 *                           0 = never, 1 = inputs of 2^17 records and more (default), k = of k records and more.
 *   "sort_hybrid"    0 | 1 | 2  PREFIX + FINISH: instead of one pass per varying key byte, passes over the most significant P
 *                           varying bytes only, then one finishing pass that completes every run of equal prefix inside LDS.
 *                           P comes from a pair count over sample ranges (compact keys) or from n (24-byte records); runs too
 *                           long for the finishing kernel make it report an overflow, and all passes run.  0 = never,
 *                           1 = when passes are saved (default), 2 = whenever one is (tests).  Same bytes either way.
 *   "sort_idx64"     0 | 1  test knob: 1 = element / record positions are 64-bit at any size (what inputs of 2^32 records and more
 *                           take), so that those kernels can be checked against the oracle at sizes it can sort.
 *   "base_order"     0 | 1  bit order of the 2-bit codec for every pack / unpack / decode / encode issued through
 *                           this context (device kernels and the stream entry points alike):
 *                             0 = IBU_BASE_ORDER_LSB_FIRST (default): base i at bits [2i, 2i+1], "ACGT" -> 0b11100100
 *                                 (bitnuc's convention as recalled; README.md:45 names the crate, record.rs:19-27
 *                                 gives only the code table);
 *                             1 = IBU_BASE_ORDER_MSB_FIRST: base i at bits [2(len-1-i), ...], "ACGT" -> 0b00011011.
 *                           The reference holds no codec code and no vector, so the order is UNPINNED; the second
 *                           value is the hedge: if an external bitnuc vector shows the other order, callers flip this
 *                           option and no kernel changes.
 *   "alloc_probe_tries" 0..16  placement probing as a property of the library, for the arrays the library allocates and that stay
 *                           resident — ibu_device_alloc, the destination of ibu_load_to_device, the context's sort scratch.
 *                           0 = auto (default): an allocation of at least 1 GiB of which at least three candidates fit in the
 *                           device's free memory draws up to four and keeps the fastest, anything else is a plain
 *                           allocation; the drawing ends early at a candidate whose hipMalloc took longer than 10 ms + 2 ms
 *                           per GB (the driver hands out memory slowly right after large frees: more candidates would
 *                           multiply that wait, not the choice); 1 = never probe; k > 1 = allocations of at least 256 MiB
 *                           draw k candidates, however long they take.  What
 *                           probing is and why: ibu_device_alloc_probed.  What it costs: a write + read of every candidate
 *                           (~0.3 ms per GB each, twice), the candidates' memory (k x bytes at the peak; the ones not kept
 *                           are freed by a helper thread right after the choice — the driver clears VRAM when it is freed,
 *                           15-25 GB/s, which a caller need not wait for; the next probing allocation and ibu_ctx_destroy
 *                           join that thread, and so does any allocation of the LIBRARY's that would otherwise fail for want
 *                           of memory — it then tries once more; a caller about to allocate with an allocator of its own
 *                           can wait for that memory by setting this option, to any value), and one synchronisation of the
 *                           context's stream per probed allocation.  It never touches the reduce
 *                           accumulator (reset / reduce ... / fetch may span allocations).  IBU_TRACE_SORT=1 prints what was
 *                           drawn and chosen.
 *   "inflate_one_launch" 0..49152  a test knob: ibu_load_bgzf_*_to_device launches its decoder AHEAD of the copies (the waves wait for
 *                           their blocks to arrive) for files of more blocks than this; 0 (default) = one round of the decoder's short
 *                           form, 49 152 blocks: smaller files get one launch behind the last copy.
 *   "bgzf_device"    0 | 1  1 (default): ibu_stream_open_path and ibu_reader_process_device on an untouched BGZF file inflate on the
 *                           device (see there); 0: through the Reader's host inflate.
 *   "bgzf_range_bytes"  >= 0  a test knob: about the compressed bytes per range of that device form (0 = default: 3.2 GB); the ranges
 *                           are whole refills, as ibu_stream_open_path says.
 *   "bgzf_stream_ahead" 0 | 1  the decoder's launch form for the ranges after the first of ibu_stream_open_path: 1 (default) ahead of
 *                           the copies (the waves wait for their bytes), 0 behind the range's last copy.
 *   "load_piece_delay_ms" 0..10000  a test knob: the BGZF loads sleep that long before every piece they copy (a slow source: the waves
 *                           of a launch that runs ahead give up after ~4 s, and what they left is inflated once everything has arrived).
 *   "release_staging"    1  one-shot: frees the device staging the BGZF loads keep between calls (the size of the compressed bytes
 *                           of the largest load so far) and the two range buffers of ibu_stream_open_path's device form; the next
 *                           load allocates them again.  Refused while such a stream is open.
 *   "numa"           0 | 1  1 = auto (default): the context looks up the NUMA node its device hangs off (PCI bus id ->
 *                           /sys/bus/pci/devices/<bdf>/numa_node -> that node's cpulist) and keeps its host side there: the pinned
 *                           ring is allocated under a preferred-node policy, the threads that fill it (the stream producer and its
 *                           feeders, the preads of ibu_load_to_device, the inflate workers a stream starts) run on the node's
 *                           CPUs (those of them the process may use).  A platform that does not say (node -1, no sysfs, a
 *                           kernel that refuses set_mempolicy) changes nothing: threads and pages go where they went before.
 *                           0 = off.  ibu_ctx_numa says what was found and where the ring landed.
 *   "peer_access"    0 | 1  the multi-GPU sort's pulls (ibu_sort_records_contexts): 1 (default) = the pulling context enables direct
 *                           peer access to the shard's device where the topology has it (copies go over xGMI without staging; it
 *                           stays enabled for the process), 0 = never: the runtime stages the copies through the host.
 *   "sort_pull_streams" 0 | 1  test knob of the multi-GPU sort: its pulls travel on one stream per PEER DEVICE (xGMI is point to point:
 *                           copies queued on one stream would use one link at a time); 1 = peers on the puller's own device get
 *                           such streams too, so that a rehearsal on one GPU runs the fork / join of those streams.
 *   "trace_rows"     0 | 1  tests: one stderr line per kernel launch of the streaming entry points saying how many rows took
 *                           the tiled and how many the one-thread-per-row kernel.  A context starts with the value the
 *                           environment variable IBU_TRACE_ROWS had when the library first created a context (read once).
 * Unknown keys / out-of-range values return IBU_ERR_INVALID_ARG. */
#define IBU_BASE_ORDER_LSB_FIRST 0
#define IBU_BASE_ORDER_MSB_FIRST 1
int32_t ibu_ctx_set_option(ibu_ctx_t* ctx, const char* key, int64_t value);
/* Device memory helpers for callers without their own allocator (tests in C, Rust shim).  Large allocations are placement-probed
 * as option "alloc_probe_tries" says (default auto: >= 1 GiB with room for three candidates; ibu_device_alloc_probed below). */
int32_t ibu_device_alloc(ibu_ctx_t* ctx, size_t bytes, void** d_ptr);
int32_t ibu_device_free(ibu_ctx_t* ctx, void* d_ptr);
/* ibu_device_alloc with PLACEMENT PROBING, for arrays that stay resident (no reference counterpart: the crate holds its records in
 * a Vec, reader.rs:528; this is the device-side "where does the Vec live" decision).  On MI355X the rate of a streaming kernel
 * depends on which physical pages the driver handed out — the same kernel on the same GPU runs 9.4 ... 11.3 ms from one
 * allocation to the next, and an allocation keeps its rate for as long as it lives.  Allocates up to `tries` candidates of
 * `bytes` bytes (all held at once, so that they are different pages; stops quietly at the first that does not fit), streams
 * one write and one read over each, keeps the fastest in *d_ptr and frees the others.  tries <= 1, or fewer than 4096
 * records' worth of bytes: a plain allocation.  `report` (nullable) says what was measured; candidate 0 is what
 * ibu_device_alloc would have returned.  Contents unspecified.  Runs on the context's stream and synchronises it; the reduce
 * accumulator is not touched (the probe reduces into scratch of its own), so reset / reduce ... / fetch may span allocations.
 * Holds tries x bytes of device memory while it measures.  Release with ibu_device_free. */
#define IBU_ALLOC_PROBE_MAX 16
typedef struct ibu_alloc_probe {
  uint32_t tries;                  /* candidates that were allocated and timed (<= the request) */
  uint32_t chosen;                 /* the one kept */
  float ms[IBU_ALLOC_PROBE_MAX];   /* write + read time of each candidate over its whole range (0 when nothing was timed) */
} ibu_alloc_probe_t;
int32_t ibu_device_alloc_probed(ibu_ctx_t* ctx, size_t bytes, uint32_t tries, void** d_ptr, ibu_alloc_probe_t* report);
int32_t ibu_memcpy_h2d(ibu_ctx_t* ctx, void* d_dst, const void* h_src, size_t bytes, void* stream);
int32_t ibu_memcpy_d2h(ibu_ctx_t* ctx, void* h_dst, const void* d_src, size_t bytes, void* stream);

/* ======================================================================================= */
/* Hot-path kernels (all asynchronous on `stream`)                                          */
/* ======================================================================================= */
/* K1  deserialise: AoS 24-byte records -> three u64 columns.  The reference's cast_slice
 * (reader.rs:301,531; mmap.rs:268) followed by the field access every consumer performs.
 * 24 B read + 24 B written per record. */
int32_t ibu_deserialize(ibu_ctx_t* ctx, const void* d_records, size_t n, uint64_t* d_barcode,
                        uint64_t* d_umi, uint64_t* d_index, void* stream);
/* K1' serialise: three u64 columns -> AoS records (Record::new + write_batch's cast_slice,
 * record.rs:87-93, writer.rs:315-318).  48 B per record. */
int32_t ibu_serialize(ibu_ctx_t* ctx, const uint64_t* d_barcode, const uint64_t* d_umi,
                      const uint64_t* d_index, size_t n, void* d_records, void* stream);
/* 2-bit unpack of one u64 column to n*len ASCII bytes (row i at d_ascii + i*len).          */
int32_t ibu_unpack_2bit(ibu_ctx_t* ctx, const uint64_t* d_codes, size_t n, uint32_t len,
                        uint8_t* d_ascii, void* stream);
/* 2-bit pack of n rows of len ASCII bytes into one u64 column; invalid bytes are reported
 * through ibu_codec_status(). */
int32_t ibu_pack_2bit(ibu_ctx_t* ctx, const uint8_t* d_ascii, size_t n, uint32_t len,
                      uint64_t* d_codes, void* stream);
/* K2  fused decode: AoS records -> barcode ASCII (n*bc_len), UMI ASCII (n*umi_len), index
 * column.  24 B read + (bc_len+umi_len+8) B written per record.  Any output may be NULL to
 * skip that column. */
int32_t ibu_decode_ascii(ibu_ctx_t* ctx, const void* d_records, size_t n, uint32_t bc_len,
                         uint32_t umi_len, uint8_t* d_bc_ascii, uint8_t* d_umi_ascii,
                         uint64_t* d_index, void* stream);
/* K3  fused encode: barcode/UMI ASCII + index column -> AoS records.  d_index == NULL writes
 * index = first_index + i (the usual "record number" use, README.md:38-47). */
int32_t ibu_encode_ascii(ibu_ctx_t* ctx, const uint8_t* d_bc_ascii, const uint8_t* d_umi_ascii,
                         const uint64_t* d_index, uint64_t first_index, size_t n, uint32_t bc_len,
                         uint32_t umi_len, void* d_records, void* stream);
/* Invalid-base report for every pack/encode launched on this context since the last call.
 * Synchronises `stream`, returns IBU_OK or IBU_ERR_INVALID_BASE (detail.a = first offending
 * record index, detail.b = offending record count) and re-arms the slot. */
int32_t ibu_codec_status(ibu_ctx_t* ctx, void* stream, uint64_t* first_bad_record,
                         uint64_t* n_bad_records);

/* K4  reduce: the device ParallelProcessor.  Fixed processors restating the reference's
 * in-repo ones: count (lib.rs:117-129), wrapping sum of the three fields
 * (examples/parallel.rs:21-36, mmap.rs:358-373), XOR of the three fields
 * (examples/roundtrip.rs:84-87).  24 B read per record. */
typedef struct ibu_reduce_result {
  uint64_t count;
  uint64_t sum[3]; /* barcode, umi, index — wrapping (mod 2^64) */
  uint64_t xor_[3];
} ibu_reduce_result_t;
/* Accumulates INTO the context's device accumulator (call ibu_reduce_reset first). */
int32_t ibu_reduce_reset(ibu_ctx_t* ctx, void* stream);
int32_t ibu_reduce(ibu_ctx_t* ctx, const void* d_records, size_t n, void* stream);
/* Synchronises `stream` and copies the accumulator out. */
int32_t ibu_reduce_fetch(ibu_ctx_t* ctx, void* stream, ibu_reduce_result_t* out);

/* Counter-based synthetic records: r(i,k) = splitmix64(seed + 3*i + k);
 * barcode = r(i,0) & mask(2*bc_len), umi = r(i,1) & mask(2*umi_len), index = i, for
 * i in [first, first+n).  Shard-independent, so each GPU materialises its own range. */
int32_t ibu_generate(ibu_ctx_t* ctx, uint64_t seed, uint64_t first, size_t n, uint32_t bc_len,
                     uint32_t umi_len, void* d_records, void* stream);

/* Streaming device-to-device copy of `bytes` bytes (ranges must not overlap): the device form of the
 * reference's memcpy hot loops (Writer::write_slice copy_from_slice writer.rs:335-347, Writer::ingest
 * append writer.rs:477-482 when both writers' batches live in HBM).  Also the on-device copy ceiling
 * bench.py prices the other kernels against.  16-B aligned ranges take the dwordx4 kernel, anything
 * else a byte kernel. */
int32_t ibu_device_copy(ibu_ctx_t* ctx, void* d_dst, const void* d_src, size_t bytes, void* stream);

/* Device-side sort by (barcode, umi, index) — the order `derive(Ord)` defines (record.rs:58)
 * and the header's sorted flag promises (header.rs:111-113).  d_tmp: n*24 B scratch.  The context
 * additionally keeps (and grows on demand) about 1.75 B per record of its own scratch.  Any n the
 * device can hold (n < 2^40).  NOT purely asynchronous: the call synchronises `stream` a few times (64- to 128-byte
 * read-backs pick the path: the census of the varying bytes, from 2^17 records on a sample census, from 8192 records on a
 * pair count that estimates the runs of equal prefix, and the finishing kernel's overflow flag); the last kernels may still be queued
 * when it returns.
 * Stable radix sort over the key bytes that vary; when at most 16 of them do (and d_records is 16-byte
 * aligned) it runs on 12- or 16-byte compacted keys held in d_tmp (and, for 16-byte keys, in the head of
 * d_records) (option "sort_compact").  Large inputs whose keys are well spread take passes over the most significant
 * varying bytes only and one finishing pass (option "sort_hybrid"); the result is the same bytes on every path. */
int32_t ibu_sort_records(ibu_ctx_t* ctx, void* d_records, void* d_tmp, size_t n, void* stream);

/* Merge of sorted records on the device (k_merge.hip): the way several sorted pieces — lanes, samples, shards, pulled batches that were
 * each sorted — become one sorted array without being sorted again.  The reference has no merge; the semantics are this library's and
 * are stated in full here.  Order is ibu_record_cmp: the three little-endian 64-bit words of a record in storage order, unsigned;
 * records that went through ibu_records_swap_umi_index merge the same way.
 *
 * ibu_merge_sorted: d_out[0 .. na+nb) = the STABLE merge of the sorted inputs d_a[0 .. na) and d_b[0 .. nb): among equal records those
 * of a come first, and within each input the order is kept.  Per record: a[i] lands at i + #{b < a[i]}, b[j] lands at j + #{a <= b[j]}.
 * Per output prefix of length d: the number of a-records in it is the result of the binary search over i in
 * [max(0, d - nb), min(d, na)] with the step `if a[mid] <= b[d-1-mid] then lo = mid + 1 else hi = mid` (the two statements are the
 * same; the library partitions the output by the second and fills each part by the first).  d_source (nullable): d_source[p] = 0 or 1,
 * the input output record p came from — equal records are the same 24 bytes, so stability shows only here; it is also the lane or
 * sample tag of a two-way merge.
 *   Arrays are 8-byte aligned.  Full 16-byte stores need d_out (and d_source, where given) 16-byte aligned; an output of 8-byte phase
 *   runs on word stores.  d_a and d_b may have either 8-byte phase.  na, nb < 2^40, all index arithmetic in 64 bits (inputs of 2^32
 *   records and more — about 100 GB — are UNTESTED).  na == 0 or nb == 0: a copy of the other input, d_source filled; both 0: OK,
 *   nothing touched.  d_out overlapping either input: IBU_ERR_INVALID_ARG, nothing touched.  The two inputs may overlap each other or
 *   be the same array.
 *   Unsorted input yields an unspecified permutation of the input multiset (in fact a followed by b wherever the kernels notice), with
 *   every write inside d_out[0, na+nb) and d_source[0, na+nb); nothing is ever read or written out of bounds.
 *   Asynchronous on `stream`, no synchronisation; the only allocation is growth of the context's sort scratch (8 bytes per 256 output
 *   records).  48 B per record: one read, one write.
 *
 * ibu_merge_sorted_runs: d_records holds k consecutive sorted runs of run_lengths[0 .. k) records (a host array; n = their sum); d_tmp
 * is n*24 B of scratch, the contract of ibu_sort_records.  On return, in stream order, d_records holds all n records sorted: byte for
 * byte what ibu_sort_records gives on the same input.  ceil(log2 k) levels of pairwise merges of neighbouring runs ping-pong between
 * the two buffers, an unpaired last run of a level is copied, and when the last level lands in d_tmp (an odd number of levels) one
 * more copy brings it back: (levels [+ 1]) x 48 B per record.  k == 0 or n == 0: OK; k == 1: nothing to do; runs of length 0 are
 * allowed.  run_lengths is read before the call returns; asynchronous otherwise.  n >= 2^40, a NULL or misaligned pointer with n > 0
 * and k > 1, or d_tmp overlapping d_records: IBU_ERR_INVALID_ARG. */
int32_t ibu_merge_sorted(ibu_ctx_t* ctx, const void* d_a, size_t na, const void* d_b, size_t nb, void* d_out, uint8_t* d_source,
                         void* stream);
int32_t ibu_merge_sorted_runs(ibu_ctx_t* ctx, void* d_records, void* d_tmp, const size_t* run_lengths, size_t k, void* stream);

/* The same order over SEVERAL shards, one per context (= per GPU), in one call — the multi-GPU form of the sort (SURVEY 8f-2:
 * sample sort with one device-to-device exchange), as ibu_mmap_process_contexts is the multi-GPU form of process_parallel.
 * EXPERIMENTAL: rehearsed with up to 16 contexts on one GPU, never run on two distinct GPUs (no such box in any round).
 * shards[i] lives on ctxs[i]'s device: n records in d_records, which has room for `capacity` records; d_tmp: capacity * 24
 * bytes of scratch on the same device.  On return shard i holds the i-th contiguous range of the global order and
 * shards[i].n says how many records that is (their sum is unchanged).  Evenly spaced samples of every shard, in proportion to
 * its size (max(16 384, 512 x n_ctxs) records in all, at most 2^19), pick the splitters; every record travels once to the owner of
 * its range (hipMemcpyPeerAsync: over xGMI between GPUs).  Three forms (multi_sort.cpp):
 *   partition first on elements — at most 11 key bytes vary over ALL shards (16/12 records with indices below 2^32), at most 32
 *     shards, 16-byte aligned buffers: a shard is compacted to 12-byte elements (one plan for all shards from the combined census
 *     words — of sample ranges when the shards are large, checked against the exact census the partition pass takes on its way;
 *     a miss re-runs that pass only), the elements are put in the order of 256 sampled key ranges by one pass of the sort's own
 *     kernels, the owners are cut on the exact counts at range boundaries, pull their pieces (12 bytes per record on the links)
 *     and sort them straight into records;
 *   partition first on records — any other key or alignment, at most 32 shards: the same on 24-byte records (their key range in
 *     the digit side stream, one 24-byte pass into the shard's scratch, the owners pull over their own records and sort once —
 *     on the census words that pass took over all shards and on one sampled prefix estimate made for all owners, not one each);
 *   sort first — more than 32 shards, option "sort_compact" = 0 on ctxs[0], or a range cut of the first two forms that does not
 *     fit a shard's capacity: every shard sorted where it lives, cut at n_ctxs - 1 splitters by binary search, 24-byte records
 *     exchanged (12-byte elements when at most 12 bytes vary), owners sort again.
 * Nothing is sorted twice in the first two.  How even the shares come out: the partition-first forms cut at the boundaries of 256
 * sampled ranges, so an owner's load is quantised to about total / 256 — 3 % of a share with 8 shards, 12 % with 32 —; the
 * sort-first form cuts at sampled quantiles of sorted shards, a few percent at any shard count.  In the partition-first forms the
 * host joins its worker threads where it needs every shard's answer (samples, range counts — copied out before the partition pass's
 * scatter kernel has run, so the plan is made while it runs) and once at the end; the exchange and the owners' sorts are ordered on
 * the devices (a pull waits for the event of the shard it reads, a sort for the pulls that read its scratch).  An owner's pulls go out on one stream per
 * peer device, so that the point-to-point links carry their pieces at the same time.
 * One host thread per context; the first error in context order is the call's.  A shard that would receive more than its
 * capacity: IBU_ERR_INVALID_ARG (detail.a = records it would receive, detail.b = its capacity) before anything has moved between
 * shards: every shard still holds its own records (untouched, or sorted locally on the sort-first path) — leave headroom for
 * uneven splits (see above for how even the shares come out; many equal records all go to one owner).  After ANY
 * OTHER error (a failed copy or kernel once the exchange has begun) the contents of the shards are unspecified.  Capacity: at
 * least n_ctxs + 1 records and 24 x capacity >= 32 x (n_ctxs - 1) bytes (the sort-first form stages the splitters and their
 * positions in d_tmp).  n_ctxs == 1 is ibu_sort_records.  Two contexts may share a device (a rehearsal on one GPU); the same
 * context twice is refused.  Peer access between the devices involved is enabled where the topology has it and stays enabled.
 * Synchronous. */
typedef struct ibu_sort_shard {
  void* d_records; /* device, 8-byte aligned: `capacity` records of room, `n` of them valid */
  void* d_tmp;     /* device, 8-byte aligned: capacity * 24 bytes of scratch                 */
  size_t n;        /* in: records of this shard; out: records of its range of the global order */
  size_t capacity;
} ibu_sort_shard_t;
int32_t ibu_sort_records_contexts(ibu_ctx_t* const* ctxs, size_t n_ctxs, ibu_sort_shard_t* shards);
/* Per-barcode aggregation of SORTED device records: the device form of the reference's BarcodeAnalyzer
 * processor (src/parallel.rs:72-98 — HashMap<barcode, count> merged in on_batch_complete).  Writes, in
 * ascending barcode order, d_barcodes[k], d_counts[k] (records with that barcode) and, when
 * d_unique_umis != NULL, the number of distinct (barcode, umi) pairs of barcode k.  *n_barcodes
 * receives the number of distinct barcodes, *n_barcode_umi_pairs (nullable) the number of distinct
 * pairs.  Size query: d_barcodes = d_counts = NULL and cap = 0.  cap too small: IBU_ERR_INVALID_ARG with
 * *n_barcodes set.  The input must be sorted (ibu_sort_records / a file whose header says sorted);
 * unsorted input yields the run-length encoding of the barcode column instead.  Synchronises `stream`
 * once (the counts come back to size the output).  n < 2^40.  Reads the records once where barcodes
 * repeat (at most 32 run heads per 8192 records: the count pass keeps them), twice where they do not;
 * the size query alone is one read — a caller that knows a bound (its whitelist) skips it and passes
 * that bound as cap. */
int32_t ibu_barcode_counts(ibu_ctx_t* ctx, const void* d_sorted_records, size_t n, uint64_t* d_barcodes,
                           uint64_t* d_counts, uint64_t* d_unique_umis, size_t cap, size_t* n_barcodes,
                           size_t* n_barcode_umi_pairs, void* stream);
/* Count matrix on the device: reads and distinct UMIs per (barcode, index) pair — cell x feature, the `index` word being where
 * users of the format keep the feature / gene number (reference README.md:40-47).  The reference has no such function (as it has no
 * sort and no aggregation); the semantics are this library's and are stated in full here.  Write w0, w1, w2 for the three
 * little-endian 64-bit words of a 24-byte record in storage order (normally barcode, umi, index).
 *
 * ibu_records_swap_umi_index: record i of d_dst = {w0, w2, w1} of record i of d_src.  Its own inverse.  d_dst == d_src (in place) is
 * allowed; any other overlap of the two n-record ranges is IBU_ERR_INVALID_ARG.  8-byte aligned arrays, n < 2^40, n == 0 is OK and
 * touches nothing, asynchronous on `stream`.  48 B per record (one read, one write): the tiled kernel when both bases have the same
 * phase modulo 16 (an 8- but not 16-byte aligned pair peels one record), one thread per record otherwise.  Why it exists:
 * ibu_sort_records compares the three words in storage order and nothing else, so (barcode, index, umi) order — which makes the
 * records of one (barcode, index) pair adjacent — is the sort applied to records whose second and third words changed places. */
int32_t ibu_records_swap_umi_index(ibu_ctx_t* ctx, const void* d_src, void* d_dst, size_t n, void* stream);
/* Run-length aggregation at pair level (k_aggregate.hip).  An ENTRY is a maximal run of consecutive records with equal (w0, w1).
 * For entry k, in input order: d_first[k] = w0, d_second[k] = w1, d_records_per_pair[k] = the length of the run, and, when
 * d_distinct_third != NULL, d_distinct_third[k] = the number of positions in the run whose w2 differs from the record before it (the
 * first record of a run counts) — on sorted input the number of distinct w2 of the pair.  *n_pairs = the number of entries,
 * *n_triples (nullable) = the sum of d_distinct_third (computed whether or not that array is asked for).
 * Two uses:
 *   on records that went through ibu_records_swap_umi_index and ibu_sort_records, entries are (barcode, index) pairs,
 *     records_per_pair = reads, distinct_third = distinct UMIs (molecules): the count matrix in COO form, rows ascending by
 *     (barcode, index);
 *   on ordinarily sorted records, entries are (barcode, umi) molecules with their reads and the number of distinct indices — the
 *     molecules with more than one are the chimeric ones a caller may want to drop.
 * Row pointers, row ordinals and the barcode of every row for a CSR view: ibu_matrix_rows on d_first (below).  The row LENGTHS alone
 * also come from ibu_barcode_counts on the swapped-and-sorted records, as unique_umis (examples/count_file.cpp).
 * Unsorted input yields the run-length encoding described above, as ibu_barcode_counts documents for itself.  Size query: d_first =
 * d_second = d_records_per_pair = NULL and cap = 0.  cap too small: IBU_ERR_INVALID_ARG with *n_pairs (and *n_triples) set and
 * nothing written (detail.a = entries, detail.b = cap).  n == 0: OK, both totals 0.  n < 2^40; 8-byte aligned arrays.  Synchronises
 * `stream` once (the totals come back to size the output); the writes may still be queued on return.  Reads the records twice (once
 * for the size query): entries are typically a sizeable fraction of n, so the count pass keeps no heads.  Scratch: the context's
 * sort scratch (per-segment tables) and 16 B per entry of its run scratch, grown on demand. */
int32_t ibu_pair_counts(ibu_ctx_t* ctx, const void* d_sorted_records, size_t n, uint64_t* d_first, uint64_t* d_second,
                        uint64_t* d_records_per_pair, uint64_t* d_distinct_third, size_t cap, size_t* n_pairs, size_t* n_triples,
                        void* stream);
/* The count matrix in one call: swap in place -> ibu_sort_records(d_records, d_tmp) -> ibu_pair_counts -> swap back in place.
 * Input in any order (sorted or not); d_tmp: n*24 B of scratch.  Entry k, ascending by (barcode, index): d_barcodes[k], d_indices[k],
 * d_reads[k] = records of the pair, d_umis[k] (nullable) = its distinct UMIs; *n_entries = entries, *n_molecules (nullable) = the sum
 * of d_umis.  On return the records are the input multiset, every record with its fields in their normal places, ordered by
 * (barcode, index, umi).  flags: IBU_COUNT_LEAVE_SWAPPED skips the last pass and leaves {barcode, index, umi} records (for a caller
 * that goes on to ibu_barcode_counts for the row pointers); any other bit is IBU_ERR_INVALID_ARG (nothing touched).  No size query
 * (it would cost the sort): d_barcodes, d_indices and d_reads must be non-NULL, and a cap that is too small fails AFTER the sort with
 * IBU_ERR_INVALID_ARG, *n_entries set, nothing written to the outputs and the records in the state the flags promise.  The safe cap
 * is n, or the caller's bound (whitelist size x features).  n == 0: OK.  n < 2^40.  Synchronises `stream` as ibu_sort_records and
 * ibu_pair_counts do; the last kernels may still be queued on return. */
#define IBU_COUNT_LEAVE_SWAPPED 1u
int32_t ibu_count_matrix(ibu_ctx_t* ctx, void* d_records, void* d_tmp, size_t n, uint32_t flags, uint64_t* d_barcodes,
                         uint64_t* d_indices, uint64_t* d_reads, uint64_t* d_umis, size_t cap, size_t* n_entries, size_t* n_molecules,
                         void* stream);
/* Matrix export, on the device (k_matrix.hip): the two steps between the entry table above and what readers of a single-cell matrix
 * take — a CSR triple with rows numbered from 0, or the 10x directory (matrix.mtx, barcodes.tsv, features.tsv) that scanpy's
 * read_10x_mtx and Seurat's Read10X read.  Both calls work on the ENTRY TABLE, the device columns ibu_pair_counts / ibu_count_matrix
 * produce, not on the records, so they follow any chain of filters.  The reference has no such function; the semantics are this
 * library's and are stated in full here.  The input columns are never written.
 *
 * ibu_matrix_rows: the row structure of a column.  A ROW is a maximal run of consecutive entries with equal d_first[k]; equal values
 * in runs that are not adjacent are different rows (A, B, A is three rows), as every run-level call here documents for itself.  Each
 * of the three outputs is nullable on its own:
 *   d_row_of_entry[k]  the 0-based number of the row entry k lies in; n_entries words;
 *   d_row_keys[r]      the value of row r;
 *   d_row_ptr[r]       the index of row r's first entry for r < *n_rows, and d_row_ptr[*n_rows] = n_entries — the CSR indptr.  The
 *                      array holds cap + 1 words; exactly *n_rows + 1 are written.
 * With d_first = the barcodes of the entry table, d_row_ptr / d_second / the counts are the CSR triple (indptr, indices, data) of
 * the cell x feature matrix and d_row_keys its barcodes.  *n_rows = the number of rows.  Size query: the three outputs NULL and
 * cap = 0 (with the outputs NULL any cap gives the count alone).  cap < *n_rows with any output given: IBU_ERR_INVALID_ARG with
 * *n_rows set and nothing written (detail.a = rows, detail.b = cap).  n_entries == 0: OK, *n_rows = 0, nothing touched — not even
 * d_row_ptr[0].  n_entries < 2^40; 8-byte aligned arrays; the outputs must not overlap d_first or each other.  Synchronises
 * `stream` once (the number of rows comes back); the writes may still be queued on return.  Reads the column twice (once for the size
 * query) and writes 8 B per entry and 16 B per row.  Scratch: 8 B per 2048 entries of the context's sort scratch, grown on demand.
 *
 * ibu_matrix_market_body: three u64 columns as decimal text.  Line k is
 *   dec(d_a[k] + add_a) ' ' dec(d_b[k] + add_b) ' ' dec(d_c[k]) '\n'
 * with the sums taken modulo 2^64 (2^64 - 1 with an addend of 1 prints 0) and dec(v) the shortest decimal form of v: "0" for zero, no
 * sign, no padding.  A line is 6 to 63 bytes.  The text is the concatenation of the lines in entry order — every line ends in its
 * '\n', and nothing (no NUL) follows the last.  *n_bytes = its length.  maxima (nullable, host) = the largest PRINTED value of each
 * column (after the addition), all zero when n_entries == 0: a caller checks the dimensions it writes in a header against them
 * without downloading a column.  d_text may have ANY byte alignment; no byte in front of d_text and none from d_text + *n_bytes on
 * is written, not even with the value it already holds.  The three columns may be one and the same array.  With d_a = the indices,
 * add_a = 1, d_b = d_row_of_entry, add_b = 1 and d_c = a count column this is the body of a MatrixMarket coordinate file, features x
 * barcodes, 1-based, as 10x writes it.  Size query: d_text = NULL and cap_bytes = 0.  cap_bytes < *n_bytes: IBU_ERR_INVALID_ARG with
 * *n_bytes (and maxima) set and nothing written (detail.a = bytes, detail.b = cap_bytes).  n_entries == 0: OK, *n_bytes = 0, nothing
 * touched.  n_entries < 2^40; 8-byte aligned columns; d_text must not overlap a column.  Synchronises `stream` once (the length
 * and the maxima come back); the write pass may still be queued on return.  Reads the columns twice (once for the size query).
 * Scratch: as ibu_matrix_rows. */
int32_t ibu_matrix_rows(ibu_ctx_t* ctx, const uint64_t* d_first, size_t n_entries, uint64_t* d_row_of_entry, uint64_t* d_row_keys,
                        uint64_t* d_row_ptr, size_t cap, size_t* n_rows, void* stream);
int32_t ibu_matrix_market_body(ibu_ctx_t* ctx, const uint64_t* d_a, const uint64_t* d_b, const uint64_t* d_c, size_t n_entries,
                               uint64_t add_a, uint64_t add_b, char* d_text, size_t cap_bytes, size_t* n_bytes,
                               uint64_t maxima[3] /* host, nullable */, void* stream);
/* One line per row of the entry table, on the device (k_matrix.hip): the dominant feature of every cell — which hashtag, antibody or
 * guide a cell carries, with how many UMIs, how far ahead of the runner-up, and whether the call is clean.  Both calls work on the
 * ENTRY TABLE (the device columns ibu_pair_counts / ibu_count_matrix produce), so they follow any chain of filters.  The reference has
 * no such function; the semantics are this library's and are stated in full here.  The input columns are never written.
 *
 * ibu_matrix_row_top: a ROW is a maximal run of consecutive entries with equal d_first[k] — the rows of ibu_matrix_rows (A, B, A is
 * three rows), and row r here is row r there.  Entry k TAKES PART iff d_set == NULL, or d_second[k] < set_bits and bit d_second[k] of
 * the bitmap d_set is set — the bitmap has the layout ibu_barcode_metrics takes (bit v is bit v & 63 of u64 word v >> 6; set_bits at
 * most 2^32; 8-byte aligned).  A key of set_bits or more never takes part, however its low bits read: 2^32 + j is not bit j.
 * d_set == NULL requires set_bits == 0 (IBU_ERR_INVALID_ARG otherwise).  Per row r, over the entries of the row that take part — each
 * output nullable on its own, one u64 per row:
 *   d_top_value[r]    the largest d_values[k];
 *   d_top_key[r]      d_second[k] of the FIRST entry, in entry order, that holds the largest value — on sorted input the smallest
 *                     feature number among the tied ones;
 *   d_next_value[r]   the largest value among the OTHER entries that take part: equal to d_top_value[r] when the top is tied, 0 when
 *                     fewer than two entries take part;
 *   d_row_sum[r]      the sum of the values modulo 2^64;
 *   d_row_entries[r]  how many entries take part.
 * A row with no entry taking part gets IBU_NO_KEY, 0, 0, 0, 0.  *n_rows = the number of rows.  Size query: the five outputs NULL (any
 * cap gives the count alone).  cap < *n_rows with any output given: IBU_ERR_INVALID_ARG with *n_rows set and nothing written
 * (detail.a = rows, detail.b = cap).  n_entries == 0: OK, *n_rows = 0, nothing touched.  n_entries < 2^40; 8-byte aligned arrays; the
 * outputs must not overlap an input column or each other (IBU_ERR_INVALID_ARG, nothing written); the three input columns may be one
 * and the same array.  Synchronises `stream` once (the number of rows comes back); the writes may still be queued on return.
 * Traffic: d_first is read twice (once for the size query), d_second and d_values once, one gathered bitmap word per entry with a set;
 * 40 B per row are written.  A row that crosses the seams of the 2048-entry units the kernels work in is put together from 40-byte
 * partial results, one per unit, by one wave, 64 units per step: a row of m entries adds m / 2048 such reads and ceil(m / 131072)
 * dependent steps — rows are not walked entry by entry by one thread, however long.  Scratch: 96 B per 2048 entries of the context's
 * sort scratch (8 for the row ordinals, 88 for the partial results and a flag), grown on demand.
 *
 * ibu_assign_rows: one class byte per row from three of those columns.  The class of row r is the first that applies:
 *   IBU_ROW_NONE      d_top_value[r] < max(rule->min_value, 1);
 *   IBU_ROW_ASSIGNED  d_top_value[r] > d_next_value[r] and d_top_value[r] * den >= num * d_row_sum[r];
 *   IBU_ROW_MIXED     otherwise.
 * The products are exact (128 bits), as every share test of this library is in integers; equality passes.  num == 0 switches the
 * share test off.  The strict top > next makes the winner unique whatever the share.  den >= 1 and num <= den are required and rule
 * must not be NULL (IBU_ERR_INVALID_ARG, nothing touched).  d_row_class (nullable): n_rows bytes.  counts (nullable, host): rows =
 * n_rows and the rows of each class.  The two may not both be NULL.  n_rows == 0 is OK: all counts are 0.  n_rows < 2^40; 8-byte
 * aligned columns.  Asynchronous on `stream`; it synchronises only when counts is given.  24 B per row read, 1 B written. */
#define IBU_NO_KEY UINT64_MAX
int32_t ibu_matrix_row_top(ibu_ctx_t* ctx, const uint64_t* d_first, const uint64_t* d_second, const uint64_t* d_values, size_t n_entries,
                           const uint64_t* d_set /*nullable*/, uint64_t set_bits, uint64_t* d_top_key, uint64_t* d_top_value,
                           uint64_t* d_next_value, uint64_t* d_row_sum, uint64_t* d_row_entries, size_t cap, size_t* n_rows, void* stream);
#define IBU_ROW_ASSIGNED 0
#define IBU_ROW_NONE 1
#define IBU_ROW_MIXED 2
typedef struct ibu_assign_rule {
  uint64_t min_value; /* a top value below max(min_value, 1) is no call */
  uint64_t num, den;  /* the least share of the row sum the top must hold: num <= den, den >= 1; num == 0: no share test */
} ibu_assign_rule_t;
typedef struct ibu_assign_counts {
  uint64_t rows, assigned, none, mixed; /* rows = assigned + none + mixed */
} ibu_assign_counts_t;
int32_t ibu_assign_rows(ibu_ctx_t* ctx, const uint64_t* d_top_value, const uint64_t* d_next_value, const uint64_t* d_row_sum, size_t n_rows,
                        const ibu_assign_rule_t* rule, uint8_t* d_row_class /*nullable*/, ibu_assign_counts_t* counts /*nullable, host*/,
                        void* stream);
/* One index per molecule, on the device (k_molecules.hip) — the step between ibu_sort_records and the count matrix that drops
 * chimeric reads: a (barcode, umi) seen with two or more index values (PCR chimeras, index hopping, multi-mapped reads) would
 * otherwise be counted once under every one of them.  The reference has no such function; the semantics are this library's and are
 * stated in full here.  Write w0, w1, w2 for the three 64-bit words of a record in storage order.
 *   A MOLECULE is a maximal run of consecutive records with equal (w0, w1).
 *   A CANDIDATE is a maximal run of consecutive records with equal (w0, w1, w2).  Its `reads` is its length.
 *   For a molecule, `best` is the largest `reads` among its candidates.
 * Every record gets one class byte:
 *   0 kept   its candidate is the only one of its molecule with reads == best (a molecule with one candidate included)
 *   1 minor  its molecule has exactly one candidate at best, and this is another one
 *   2 tied   its molecule has two or more candidates at best (all records of the molecule, the smaller candidates too)
 * flags: IBU_MOLECULES_TIE_FIRST changes the tied case only — in a tied molecule the first candidate at best in input order is
 * class 0 and every other record of the molecule is class 1 (on sorted input that candidate has the smallest index); class 2 then
 * never occurs.  Any other bit is IBU_ERR_INVALID_ARG, and nothing is touched.
 * On records sorted by (barcode, umi, index) the runs are the molecules and their indices.  On unsorted input the result is the same
 * run-level computation on the runs as they stand: a molecule that is interrupted and returns is two molecules, as ibu_barcode_counts
 * and ibu_pair_counts document for themselves.  The records are never written.
 * d_class (nullable: totals only): n bytes.  counts (nullable): molecules / candidates = the runs of equal (w0, w1) / of equal
 * (w0, w1, w2); resolved = molecules with two or more candidates and exactly one at best; tied = molecules with two or more at best
 * (counted under IBU_MOLECULES_TIE_FIRST too); reads_kept + reads_minor + reads_tied = n, the records of each class; reserved = 0.
 * ibu_select_records(..., keep_mask = 1 << IBU_MOLECULE_KEPT) then gives the chimera-free records in input order, still sorted.
 * Records 8-byte aligned: a 16-byte aligned array takes the tiled path, an 8- but not 16-byte aligned one peels one record, as
 * ibu_pair_counts does.  n < 2^40.  n == 0 is OK: nothing is touched and all totals are 0.  A NULL context is an error.
 * Synchronises `stream` once (the candidate and molecule totals come back to size the scratch); the class writes may still be queued
 * on return.  With counts != NULL it waits a second time, for the totals, which are final only behind the verdicts.
 * Traffic: the records are read twice (count, emit); 8 B per candidate travel once each way (the candidate table: first row, and
 * whether it begins a molecule), the verdict is 1 B per candidate, the class write 1 B per record — filled from the table and from
 * 16 B of head ballots per 128 records the emit pass keeps, not from the records.  A molecule of any number of candidates costs the
 * same per candidate (a segmented scan per 1024 candidates, a second one over the blocks).  Scratch: the context's sort scratch for
 * the per-segment tables and the ballots (n / 8 bytes), and 9.1 B per candidate of its run scratch (8 table + 1 verdict + 68 B per
 * 1024 candidates of block summaries), grown on demand. */
#define IBU_MOLECULE_KEPT 0
#define IBU_MOLECULE_MINOR 1
#define IBU_MOLECULE_TIED 2
#define IBU_MOLECULES_TIE_FIRST 1u
typedef struct ibu_molecule_counts {
  uint64_t molecules, candidates;                 /* runs of equal (w0,w1) / of equal (w0,w1,w2) */
  uint64_t resolved;                              /* molecules with >= 2 candidates and exactly one at best */
  uint64_t tied;                                  /* molecules with >= 2 candidates at best (counted under TIE_FIRST too) */
  uint64_t reads_kept, reads_minor, reads_tied;   /* records per class; their sum is n */
  uint64_t reserved;                              /* 0 */
} ibu_molecule_counts_t;
int32_t ibu_classify_molecules(ibu_ctx_t* ctx, const void* d_sorted_records, size_t n, uint32_t flags, uint8_t* d_class,
                               ibu_molecule_counts_t* counts, void* stream);
/* Cell calling on the device (k_cells.hip): which barcodes of sorted records are cells — the cut by per-barcode UMI count that every
 * single-cell pipeline makes before the matrix is used (real input has 10-100 times more barcodes than cells: ambient RNA, empty
 * droplets).  The reference has no such function; the semantics are this library's and are stated in full here.  Write w0, w1 for
 * the first two 64-bit words of a record in storage order.
 *   A BARCODE is a maximal run of consecutive records with equal w0 — the runs of ibu_barcode_counts.
 *   Its `reads` is the length of the run; its `umis` the number of positions in the run whose w1 differs from the record before it
 *   (the first position counts) — what ibu_barcode_counts returns as unique_umis.
 *   The METRIC of a barcode is its umis, or its reads under the flag IBU_CELLS_BY_READS.
 * Let B be the number of barcodes and m(1) >= m(2) >= ... >= m(B) their metrics in descending order.  Every mode comes down to one
 * integer threshold T, and a barcode is a cell iff its metric >= T:
 *   IBU_CELLS_MIN     T = param (T = 0: every barcode is a cell); baseline = 0.
 *   IBU_CELLS_TOP     param = K >= 1: T = m(min(K, B)).  The barcodes tied with the K-th are all cells, so cells >= min(K, B);
 *                     baseline = 0.
 *   IBU_CELLS_ORDMAG  param = the expected number of cells E >= 1: E' = min(E, B), baseline = m(E' / 100 + 1) with integer division
 *                     (the 99th percentile of the top E', no interpolation), T = (baseline + 9) / 10 — a tenth of it, rounded up.
 * Every record gets the class of its barcode: IBU_CELL (0) or IBU_CELL_BACKGROUND (1).  ibu_select_records(..., keep_mask =
 * 1 << IBU_CELL) then gives the records of the cells in input order, still sorted.
 * d_class (nullable: totals only): n bytes.  counts (nullable): barcodes = B; cells = the class-0 barcodes; threshold = T; baseline as
 * above; reads_cells + reads_background = n, the records of each class; umis_cells + umis_background = the (barcode, umi) pair
 * total of ibu_barcode_counts — UMI totals under IBU_CELLS_BY_READS as well.
 * On unsorted input the result is the same run-level computation on the runs as they stand (a barcode that is interrupted and
 * returns is two barcodes), as ibu_barcode_counts documents for itself.  The records are never written.
 * IBU_ERR_INVALID_ARG: an unknown mode, an unknown bit in flags, param == 0 in the TOP and ORDMAG modes (checked first, whatever n
 * is), a NULL or misaligned d_sorted_records with n > 0, n >= 2^40 — a refused call touches nothing, `counts` included.  n == 0 is
 * OK: nothing is touched and all totals are 0, except threshold = param in the MIN mode.  A NULL context is an error.  Records 8-byte aligned: a 16-byte aligned array takes the tiled path, an 8- but not 16-byte aligned one peels
 * one record, as ibu_pair_counts does.
 * Synchronises `stream` once (the barcode and pair totals come back to size the scratch); the class writes may still be queued on
 * return.  With counts != NULL it waits a second time, for the totals.  The threshold of the TOP and ORDMAG modes is found on the
 * device — a radix selection over the B metrics, five digit passes — with no host round trip in between.
 * Traffic: the records are read twice (count, emit; two of their three words); 24 B per barcode are written and read (first row, pair
 * rank, metric), the selection reads the B metrics once per digit, the verdict is 1 B per barcode and the class write 1 B per
 * record — filled from the verdicts and from 16 B of run-head ballots per 128 records the emit pass keeps, not from the records.
 * No atomic per record or per barcode.  Scratch: the context's sort scratch for the per-segment tables and the ballots (n / 8
 * bytes), and 25 B per barcode (+ 10 KiB of histograms) of its run scratch, grown on demand. */
#define IBU_CELL 0
#define IBU_CELL_BACKGROUND 1
#define IBU_CELLS_MIN 0u    /* param = T */
#define IBU_CELLS_TOP 1u    /* param = K >= 1 */
#define IBU_CELLS_ORDMAG 2u /* param = expected cells E >= 1 */
#define IBU_CELLS_BY_READS 1u /* flag: the metric is reads, not umis */
typedef struct ibu_cell_counts {
  uint64_t barcodes, cells;                 /* runs of equal w0 / those of class 0 */
  uint64_t threshold, baseline;             /* T / m(E' / 100 + 1) in the ORDMAG mode, else 0 */
  uint64_t reads_cells, reads_background;   /* records per class; their sum is n */
  uint64_t umis_cells, umis_background;     /* (barcode, umi) pairs per class */
} ibu_cell_counts_t;
int32_t ibu_call_cells(ibu_ctx_t* ctx, const void* d_sorted_records, size_t n, uint32_t mode, uint64_t param, uint32_t flags,
                       uint8_t* d_class, ibu_cell_counts_t* counts, void* stream);
/* Per-barcode QC metrics and the barcode filter, on the device (k_metrics.hip) — the step between "these barcodes are cells" and
 * the matrix: per barcode its reads, UMIs, features detected and the share of its reads or UMIs that fall in a feature set
 * (mitochondrial, ribosomal, spike-in), and the filter that drops barcodes with too few features, with implausibly many (doublets),
 * or with too high a share.  The reference has no such function; the semantics are this library's and are stated in full here.
 * Write w0, w1, w2 for the three 64-bit words of a record in storage order.
 *   A BARCODE is a maximal run of consecutive records with equal w0.
 *   A PAIR is a maximal run of consecutive records with equal (w0, w1).
 *   A TRIPLE is a maximal run of consecutive records with equal (w0, w1, w2).
 * A FEATURE SET is a device bitmap d_set of set_bits bits, stored as 8-byte aligned uint64_t words: value v is bit v & 63 of word
 * v >> 6 ((set_bits + 63) / 64 words are read, nothing behind them).  set_word is 1 or 2.  A record is IN THE SET iff the value v of
 * its word set_word satisfies v < set_bits and bit v is set.  d_set == NULL together with set_bits == 0: no record is in the set.
 * set_bits <= 2^32.  All records of a triple agree in every word, so "a triple is in the set" is well defined.
 * For barcode k, in input order: barcode[k] = w0; reads[k], pairs[k], triples[k] = its records, and the pairs and triples that begin
 * in it; set_reads[k] = its records in the set; set_triples[k] = its triples in the set.
 * Two uses:
 *   on records that went through ibu_records_swap_umi_index and the sort (what IBU_COUNT_LEAVE_SWAPPED leaves), with set_word = 1:
 *     pairs are features detected, triples are UMIs, set_triples are UMIs in the set;
 *   on ordinarily sorted records behind ibu_classify_molecules and select, with set_word = 2: pairs equal triples and both are
 *     UMIs, set_triples are UMIs in the set; features are not available in that order.
 * Unsorted input gives the same computation on the runs as they stand (a barcode that is interrupted and returns is two barcodes),
 * as ibu_barcode_counts documents for itself.  The records are never written.
 *
 * ibu_barcode_metrics: every output column is nullable on its own.  *n_barcodes = the number of barcodes.  Size query: all six
 * columns NULL and cap == 0.  cap too small (with any column given): IBU_ERR_INVALID_ARG with *n_barcodes set and nothing written
 * (detail.a = barcodes, detail.b = cap).  n == 0: OK, *n_barcodes = 0, nothing touched.  IBU_ERR_INVALID_ARG, with nothing touched
 * (*n_barcodes included): set_word outside {1, 2}, set_bits > 2^32, NULL d_set with set_bits > 0, a misaligned d_set, a NULL
 * n_barcodes, n >= 2^40, and, with n > 0, a NULL or misaligned d_records or a misaligned column.  A NULL context is an error.
 * Records 8-byte aligned: a 16-byte aligned array takes the tiled path, an 8- but not 16-byte aligned one peels one record, as
 * ibu_pair_counts does.  Synchronises `stream` once (the barcode total comes back to size the table); the writes may still be queued
 * on return.
 *
 * ibu_filter_barcodes: every record gets the class byte of its barcode; the first class that applies wins:
 *   IBU_BARCODE_PASS 0
 *   IBU_BARCODE_LOW  1   reads < min_reads, pairs < min_pairs or triples < min_triples
 *   IBU_BARCODE_HIGH 2   reads > max_reads, pairs > max_pairs or triples > max_triples, for the maxima that are not 0
 *   IBU_BARCODE_SET  3   set_den != 0 and set_x * set_den > set_num * x, where (set_x, x) = (set_reads, reads) for set_of == 0 and
 *                        (set_triples, triples) for set_of == 1 — the share of the set is above set_num / set_den
 * A maximum of 0 means no maximum, set_den == 0 no set test: a zeroed limits struct passes everything.  The set test is integer
 * arithmetic: equality passes and there is no float anywhere.  set_num <= set_den < 2^24 is required, so that with counts below 2^40
 * no product overflows 64 bits.  ibu_select_records(..., keep_mask = 1 << IBU_BARCODE_PASS) then keeps the passing barcodes'
 * records in input order, still sorted.
 * d_class (nullable: totals only): n bytes at any alignment.  counts (nullable): barcodes = the number of barcodes;
 * barcodes_by_class[c] / reads_by_class[c] = the barcodes / records of class c (the reads sum to n); triples_passed,
 * set_triples_passed = the triples / set triples of the class-0 barcodes; reserved = 0.
 * IBU_ERR_INVALID_ARG: the set errors above, a NULL limits, set_of > 1, set_num > set_den, set_den >= 2^24 (all checked whatever n
 * is), a NULL or misaligned d_records with n > 0, n >= 2^40 — a refused call touches nothing, `counts` included.  n == 0 is OK:
 * nothing is touched and all totals are 0.  A NULL context is an error.  Synchronises `stream` once (the barcode total comes back
 * to size the scratch); the class writes may still be queued on return.  With counts != NULL it waits a second time, for the totals.
 *
 * Traffic of both: the records are read twice (count, emit), and one 8-byte word of the bitmap is gathered per record and pass (a
 * set of 60 000 features is 7.5 KB and stays in cache); 40 B per barcode are written and read (the row, and the pairs, triples, set
 * reads and set triples in front of it — the metrics are differences of neighbouring rows), the verdict is 1 B per barcode and the
 * class write 1 B per record, filled from the verdicts and from 16 B of barcode-head ballots per 128 records the emit pass keeps.
 * No atomic per record or per barcode.  Scratch: the context's sort scratch for the per-segment tables (536 B per 8192 records)
 * and the ballots (n / 8 bytes), and 41 B per barcode (+ 128 B) of its run scratch, grown on demand. */
#define IBU_BARCODE_PASS 0
#define IBU_BARCODE_LOW 1
#define IBU_BARCODE_HIGH 2
#define IBU_BARCODE_SET 3
typedef struct ibu_barcode_limits {
  uint64_t min_reads, max_reads;       /* a maximum of 0: none */
  uint64_t min_pairs, max_pairs;
  uint64_t min_triples, max_triples;
  uint64_t set_num, set_den;           /* set_den == 0: no set test; else set_num <= set_den < 2^24 */
  uint32_t set_of;                     /* 0: the share of reads, 1: of triples */
  uint32_t reserved;                   /* ignored */
} ibu_barcode_limits_t;
typedef struct ibu_barcode_filter_counts {
  uint64_t barcodes;                   /* runs of equal w0 */
  uint64_t barcodes_by_class[4];
  uint64_t reads_by_class[4];          /* their sum is n */
  uint64_t triples_passed, set_triples_passed;
  uint64_t reserved;                   /* 0 */
} ibu_barcode_filter_counts_t;
int32_t ibu_barcode_metrics(ibu_ctx_t* ctx, const void* d_records, size_t n, const uint64_t* d_set, uint64_t set_bits, uint32_t set_word,
                            uint64_t* d_barcodes, uint64_t* d_reads, uint64_t* d_pairs, uint64_t* d_triples, uint64_t* d_set_reads,
                            uint64_t* d_set_triples, size_t cap, size_t* n_barcodes, void* stream);
int32_t ibu_filter_barcodes(ibu_ctx_t* ctx, const void* d_records, size_t n, const uint64_t* d_set, uint64_t set_bits, uint32_t set_word,
                            const ibu_barcode_limits_t* limits, uint8_t* d_class, ibu_barcode_filter_counts_t* counts, void* stream);
/* Per-feature metrics and the feature filter, on the device (k_features.hip) — the other axis of the count matrix: for every feature
 * (the index word: gene, antibody, guide) the reads and UMIs it received and the cells it was seen in, and the filter that drops the
 * features seen in too few cells (scanpy's filter_genes(min_cells = 3), Seurat's min.cells).  The reference has no such function;
 * the semantics are this library's and are stated in full here.  PAIRS and TRIPLES are those of the per-barcode block above: a pair
 * is a maximal run of consecutive records with equal (w0, w1), a triple one with equal (w0, w1, w2).  THE FEATURE of a record is the
 * value f of its word feature_word, which is 1 or 2.  1 <= n_features <= 2^32.
 *
 * ibu_feature_metrics.  feature_word == 1 is for records that went through ibu_records_swap_umi_index and the sort (what
 * IBU_COUNT_LEAVE_SWAPPED leaves: sorted by (barcode, index, umi)).  For every f < n_features:
 *   reads[f] = the records whose feature is f;
 *   umis[f]  = the triples whose feature is f (all records of a triple agree in every word);
 *   cells[f] = the pairs whose feature is f (all records of a pair agree in w1).  A record that begins a barcode begins a pair even
 *              where it leaves w1 unchanged: two neighbouring barcodes with the same feature count two cells.
 * feature_word == 2 is for ordinarily sorted records (barcode, umi, index): reads and umis are defined the same way; cells are not
 * available in that order, a non-NULL d_cells is IBU_ERR_INVALID_ARG and totals[2] is 0.
 * A record with f >= n_features enters no column — a value of 2^32 and more whose low bits name a valid feature included.
 * totals (nullable, host) = {the sum of reads, the sum of umis, the sum of cells, the records with f >= n_features}: the first and
 * the last add up to n.  Unsorted input gives the same computation on the runs as they stand (a pair that is interrupted and returns
 * is two cells).  The records are never written.
 * Each column is nullable on its own and holds n_features uint64_t, 8-byte aligned.  The call zeroes the columns it is given; with
 * flags bit 0, IBU_FEATURE_ACCUMULATE, it does not and adds on top of their contents — shards cut at barcode boundaries, or several
 * samples into one table.  A pair (or triple) that the boundary between two such calls cuts counts once in each call: cut shards
 * where a barcode begins.  totals are always those of this call alone.
 * n == 0 is OK: the columns are zeroed unless accumulating, and the totals are 0.  Asynchronous on `stream`; with totals != NULL
 * the call waits once, for them.  The results are sums of integers: two runs give the same columns.
 * IBU_ERR_INVALID_ARG, with nothing touched: feature_word outside {1, 2}, n_features outside 1 .. 2^32, an unknown bit in flags, a
 * misaligned column, d_cells with feature_word == 2, n >= 2^40, and, with n > 0, a NULL or misaligned d_records.  A NULL context
 * is an error.
 *
 * ibu_filter_features.  The three columns are INPUTS here: what ibu_feature_metrics made, possibly on other records (the called
 * cells) than the ones that are classed (all records) — which is why these are two calls.  The verdict of feature f < n_features is
 * the first that applies:
 *   IBU_FEATURE_LOW  1   reads[f] < min_reads, umis[f] < min_umis or cells[f] < min_cells
 *   IBU_FEATURE_HIGH 2   reads[f] > max_reads, umis[f] > max_umis or cells[f] > max_cells, for the maxima that are not 0
 *   IBU_FEATURE_PASS 0   otherwise
 * A maximum of 0 means no maximum: a zeroed limits struct passes every feature.  A feature without reads is LOW as soon as one
 * minimum is positive.  A column may be NULL when its two limits are both 0; otherwise IBU_ERR_INVALID_ARG.
 * Every record gets the verdict of its feature in d_class (nullable: totals only; n bytes at any alignment), and
 * IBU_FEATURE_UNKNOWN 3 where f >= n_features.  d_verdict (nullable) receives the n_features verdict bytes.  counts (nullable,
 * host): features_by_class[v] = the table entries of verdict v (they sum to n_features), reads_by_class[c] = the records of class c
 * (they sum to n), reserved = 0.  With n == 0 the verdicts and features_by_class are still produced and no record is touched.
 * ibu_select_records(..., keep_mask = 1 << IBU_FEATURE_PASS) then keeps the records of the kept features in input order, still
 * sorted, and ibu_pair_counts on them is the filtered matrix with no second sort.
 * IBU_ERR_INVALID_ARG, with nothing touched (`counts` included): feature_word outside {1, 2}, n_features outside 1 .. 2^32, a NULL
 * limits, a misaligned column, a NULL column with a non-zero limit, n >= 2^40, and, with n > 0, a NULL or misaligned d_records.
 * A NULL context is an error.  Asynchronous on `stream`; with counts != NULL the call waits once, for them.
 *
 * Traffic: the metrics read the records once and issue at most three 8-byte integer atomics per group — a pair (feature_word 1) or
 * a triple (2), cut where a step of 128 records ends — into columns of 8 B per feature that stay in L2; the filter reads the columns
 * once, the records once, gathers one verdict byte per record and writes one class byte per record.  Scratch: 128 B of the
 * context's run scratch, and n_features bytes more when d_verdict is NULL. */
#define IBU_FEATURE_PASS 0
#define IBU_FEATURE_LOW 1
#define IBU_FEATURE_HIGH 2
#define IBU_FEATURE_UNKNOWN 3
#define IBU_FEATURE_ACCUMULATE 1u     /* flags bit 0 */
int32_t ibu_feature_metrics(ibu_ctx_t* ctx, const void* d_records, size_t n, uint32_t feature_word, uint64_t n_features, uint32_t flags,
                            uint64_t* d_reads, uint64_t* d_umis, uint64_t* d_cells, uint64_t totals[4] /*nullable, host*/, void* stream);
typedef struct ibu_feature_limits {
  uint64_t min_reads, max_reads;       /* a maximum of 0: none */
  uint64_t min_umis, max_umis;
  uint64_t min_cells, max_cells;
} ibu_feature_limits_t;
typedef struct ibu_feature_filter_counts {
  uint64_t features_by_class[3];       /* their sum is n_features */
  uint64_t reads_by_class[4];          /* their sum is n */
  uint64_t reserved;                   /* 0 */
} ibu_feature_filter_counts_t;
int32_t ibu_filter_features(ibu_ctx_t* ctx, const void* d_records, size_t n, uint32_t feature_word, uint64_t n_features,
                            const uint64_t* d_reads, const uint64_t* d_umis, const uint64_t* d_cells, const ibu_feature_limits_t* limits,
                            uint8_t* d_class /*nullable*/, uint8_t* d_verdict /*nullable, n_features bytes*/,
                            ibu_feature_filter_counts_t* counts /*nullable, host*/, void* stream);
/* Read subsampling and the saturation curve, on the device (k_saturation.hip): a reproducible random subset of the reads — what
 * brings samples of different depth to a common depth — and the number every single-cell summary reports first: how many distinct
 * molecules and barcodes would have been seen at a fraction of the reads.  The reference has nothing like this; the semantics are
 * this library's and are stated in full here.  Write w0, w1 for the first two 64-bit words of a record in storage order, and
 * splitmix64(z) for: z += 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 * z ^ (z >> 31) — all modulo 2^64 (splitmix64(0) = 0xE220A8397B1DCDAF).
 *   THE NUMBER OF A READ  u(row) = splitmix64(splitmix64(seed) + first_row + row), the sums modulo 2^64.  `row` is the record's
 *     position in the array given to the call, `first_row` a caller's offset, so that the pieces of a larger array hash as the whole
 *     would.  The records' contents do not enter: two identical records are two reads.  The result therefore DEPENDS ON THE ORDER
 *     of the records — apply it at one fixed stage of a pipeline, normally the sorted records.
 *   KEPT  a read is kept at a threshold t (64 bits, unsigned) iff u(row) < t, or t == UINT64_MAX, which keeps every read; t == 0
 *     keeps none.  The sets are nested: a read kept at t is kept at every larger t.  A fraction f of the reads is the threshold
 *     floor(f * 2^64), f >= 1 is UINT64_MAX.
 * ibu_subsample_class: d_class[row] = IBU_SAMPLE_KEPT (0) or IBU_SAMPLE_DROPPED (1) for the n rows; no record is read.
 * ibu_select_records(..., keep_mask = 1 << IBU_SAMPLE_KEPT) then gives the subset in input order, still sorted.  d_class (nullable:
 * the count only): n bytes at any alignment.  n_kept (nullable): the number of kept rows; non-NULL synchronises `stream`, NULL leaves
 * the call asynchronous (as `counts` of ibu_correct_barcodes, and under its rule of one such call in flight per context).  n == 0 is
 * OK and touches nothing (*n_kept = 0).  IBU_ERR_INVALID_ARG: n >= 2^40; d_class == NULL together with n_kept == NULL, a call with
 * nothing to do — a refused call leaves *n_kept alone.  A NULL context is an error.  Writes 1 B per row, sixteen rows per lane and
 * store where the alignment of d_class allows; no atomic per row.
 * ibu_saturation_curve: `thresholds` is a HOST array of 1 <= k <= IBU_SATURATION_MAX_POINTS values, non-decreasing (duplicates are
 * allowed), `points` a HOST array of k structs.  For point j: threshold = thresholds[j];
 *   reads      the reads kept at thresholds[j];
 *   barcodes   the maximal runs of consecutive records with equal w0 that have at least one kept read;
 *   molecules  the same for the runs of equal (w0, w1).
 * On records sorted by (barcode, umi, index), 1 - molecules / reads is the sequencing saturation at that depth; on records that went
 * through ibu_records_swap_umi_index and the sort, `molecules` counts the (barcode, index) pairs with a kept read — the non-zero
 * entries of the count matrix, "genes detected".  At UINT64_MAX the three are n, the runs of ibu_barcode_counts and those of
 * ibu_pair_counts.  On unsorted input the result is the same computation on the runs as they stand, as ibu_barcode_counts documents
 * for itself.  The records are never written.
 * IBU_ERR_INVALID_ARG, with nothing touched, `points` included: k == 0, k > 32, a threshold below the one before it, NULL
 * thresholds or points, a NULL or misaligned d_sorted_records with n > 0, n >= 2^40.  A NULL context is an error.  n == 0 is OK:
 * every point is {threshold, 0, 0, 0}.  Records 8-byte aligned: a 16-byte aligned array takes the tiled path, an 8- but not 16-byte
 * aligned one peels one record, as ibu_pair_counts does.  Synchronises `stream` once.
 * Traffic: the records are read ONCE for all k points (two of their three words are looked at): every read falls into the bin
 * "number of thresholds <= u", a run into the smallest bin of its reads, and the curve is the three histograms read cumulatively.
 * 408 B per 8192 records of per-segment counters are written and read once; runs that span segments are stitched by a segmented
 * min-scan over the segments (n / 8192 entries whatever the run lengths).  No atomic per record.  Scratch: the context's sort
 * scratch, 408 B per 8192 records (+ 2 KiB), grown on demand. */
#define IBU_SAMPLE_KEPT 0
#define IBU_SAMPLE_DROPPED 1
#define IBU_SATURATION_MAX_POINTS 32u
typedef struct ibu_saturation_point {
  uint64_t threshold;                       /* thresholds[j] */
  uint64_t reads, barcodes, molecules;      /* kept reads / runs of equal w0 / of equal (w0, w1) with a kept read */
} ibu_saturation_point_t;
int32_t ibu_subsample_class(ibu_ctx_t* ctx, size_t n, uint64_t first_row, uint64_t seed, uint64_t threshold, uint8_t* d_class,
                            size_t* n_kept, void* stream);
int32_t ibu_saturation_curve(ibu_ctx_t* ctx, const void* d_sorted_records, size_t n, uint64_t first_row, uint64_t seed,
                             const uint64_t* thresholds, uint32_t k, ibu_saturation_point_t* points, void* stream);
/* Barcode correction against a whitelist, on the device (k_whitelist.hip) — the step between a load and ibu_sort_records /
 * ibu_barcode_counts that makes the latter's "a caller that knows a bound (its whitelist)" true of real input.  The reference has
 * no such function (as it has no sort and no aggregation); the semantics are this library's and are stated in full here.
 * A whitelist is a set of w >= 1 codes, each a bc_len-base barcode in the 2-bit form the records hold (1 <= bc_len <= 32, every bit
 * at or above 2*bc_len zero); duplicates count once.  For a record, low = barcode & mask(2*bc_len); the bits above are carried
 * along untouched (the decoder ignores them).  A neighbour of low is low ^ (x << 2i), i in [0, bc_len), x in {1, 2, 3}: one base
 * substituted — the same set under either base order, so the option "base_order" does not enter.  Every record gets one class:
 *   0 exact      low is in the whitelist                                   the record is untouched
 *   1 corrected  not exact, exactly one neighbour is in the whitelist      the low 2*bc_len bits of barcode become that neighbour
 *   2 ambiguous  not exact, two or more neighbours are in the whitelist    untouched
 *   3 unmatched  neither                                                   untouched
 * With max_mismatches == 0 only classes 0 and 3 occur.  umi, index and the barcode bits above 2*bc_len are never written.
 * The device table: open addressing over 64-bit keys, a power of two of slots (at least 1024, at least 2 w), 8 bytes each. */
typedef struct ibu_whitelist ibu_whitelist_t;
typedef struct ibu_correct_counts { uint64_t exact, corrected, ambiguous, unmatched; } ibu_correct_counts_t;
/* Builds the device lookup table from w codes in DEVICE memory (what ibu_pack_2bit writes; 8-byte aligned).  Synchronous.
 * IBU_ERR_INVALID_ARG: w == 0, w > 2^31, bc_len outside 1..32, a code with bits at or above 2*bc_len (detail.a = the lowest
 * position of such a code).  A NULL ctx on a host without a device: IBU_ERR_NO_DEVICE.  The whitelist belongs to `ctx` (and its
 * device); it is read-only once built and may serve any number of ibu_correct_barcodes calls, on different streams at once (see there for
 * `counts`). */
int32_t ibu_whitelist_create(ibu_ctx_t* ctx, const uint64_t* d_codes, size_t w, uint32_t bc_len, void* stream, ibu_whitelist_t** out);
/* Any of the three outputs may be NULL.  n_distinct: the codes after duplicates are dropped; device_bytes: what the table takes. */
int32_t ibu_whitelist_info(const ibu_whitelist_t* wl, uint32_t* bc_len, size_t* n_distinct, size_t* device_bytes);
void ibu_whitelist_destroy(ibu_whitelist_t* wl); /* before its context is destroyed */
/* In place over n device records (8-byte aligned).  d_class (nullable): n bytes, one class per record.  counts (nullable): this
 * call's four totals; non-NULL synchronises `stream`, NULL leaves the call asynchronous.  max_mismatches: 0 or 1 (anything else
 * IBU_ERR_INVALID_ARG).  A whitelist of another context: IBU_ERR_INVALID_ARG.  n < 2^40.  n == 0 is OK and touches nothing.
 * Reads 24 B per record and a table line for its barcode; writes 1 B of class and, for corrected records only, 8 B.  Only records
 * that miss look at their 3*bc_len neighbours (a wave searches its missing records one after the other, 64 neighbours at a time).
 * The totals of a call with counts != NULL pass through the context (as every small read-back does): of the calls in flight on ONE
 * context at the same time — other streams, other host threads — at most one may ask for counts; the others pass counts == NULL. */
int32_t ibu_correct_barcodes(ibu_ctx_t* ctx, const ibu_whitelist_t* wl, void* d_records, size_t n, uint32_t max_mismatches,
                             uint8_t* d_class, ibu_correct_counts_t* counts, void* stream);
/* Stable compaction: the records whose class c has bit c of keep_mask set, in their input order, to d_out (8-byte aligned; must
 * not overlap d_records).  *n_out = how many.  Size query: d_out == NULL and cap == 0.  cap too small: IBU_ERR_INVALID_ARG with
 * *n_out set and nothing written (detail.a = records kept, detail.b = cap).  Class bytes above 7 are never kept.  Synchronises
 * `stream` once (the count comes back before anything is written); the writes may still be queued on return.  n < 2^40.  Uses the
 * context's sort scratch (8 bytes per 2048 records). */
int32_t ibu_select_records(ibu_ctx_t* ctx, const void* d_records, const uint8_t* d_class, size_t n, uint32_t keep_mask,
                           void* d_out, size_t cap, size_t* n_out, void* stream);
/* Stable multi-way partition by class byte, in one pass over the records (k_partition.hip): every sample of a multiplexed library at
 * once, where ibu_select_records keeps one subset per call and never a class above 7.  The reference has nothing like this; the
 * semantics are this library's and are stated in full here (tests/partition_np.py states them in numpy).
 * part_of (host, 256 bytes, nullable): part_of[c] is the part of class byte c — a value below n_parts, or IBU_PART_NONE (255) for a
 * record that is dropped.  Several classes may map to one part.  NULL means the identity for c < n_parts and IBU_PART_NONE above.
 * n_parts is 1 .. 255.  d_out (8-byte aligned; must not overlap d_records, by the test ibu_select_records makes) receives part 0,
 * then part 1, and so on; within a part the records keep their input order, so every part of sorted input is still sorted, and the
 * output bytes are fully determined by the input.  offsets (host, n_parts + 1 words, required): offsets[p] = the first record of
 * part p in d_out, offsets[n_parts] = the number of records kept.
 * Size query: d_out == NULL and cap == 0 fills offsets and writes nothing.  cap (records) smaller than offsets[n_parts]:
 * IBU_ERR_INVALID_ARG with offsets filled and nothing written (detail.a = records kept, detail.b = cap); with a larger cap the
 * bytes behind the last kept record are untouched.  n == 0 is OK: all offsets are 0 and nothing is touched.  n < 2^40.
 * IBU_ERR_INVALID_ARG, with nothing touched: n_parts outside 1 .. 255; a part_of entry that is neither below n_parts nor 255
 * (detail.a = the class, detail.b = the entry); offsets == NULL; with n > 0 a NULL or misaligned d_records, a NULL d_class, a
 * misaligned or overlapping d_out (these leave offsets zeroed); more parts x units than one scan takes (below).
 * Synchronises `stream` once (the offsets come back before anything is written); the scatter may still be queued on return.  The
 * offsets pass through the context, as every small read-back does (the rule ibu_correct_barcodes states): of the calls in flight on
 * ONE context at the same time, at most one may be such a call.
 * Three kernels: count (a wave owns a UNIT of consecutive records and counts it per part in LDS), one exclusive scan of the
 * part-major table of (part, unit) counts, scatter (a wave keeps its unit's running position per part in LDS; per 64 records the
 * lanes of equal part find each other with the sort's match-any).  Reads 1 B of class per record twice and 24 B per kept record;
 * writes 24 B per kept record.  The unit is max(2048, the power of two at or above 64 * n_parts) records, and the table lives in the
 * context's sort scratch: 8 * (n_parts * ceil(n / unit) + n_parts + 2) bytes, at most n / 8 + 4096 for any n_parts.  The scan
 * indexes the table with 32 bits: n_parts * ceil(n / unit) above 2^32 - 16385 is refused (255 parts: from 2.7e11 records). */
#define IBU_PART_NONE 255u
int32_t ibu_partition_records(ibu_ctx_t* ctx, const void* d_records, const uint8_t* d_class, size_t n, const uint8_t part_of[256],
                              uint32_t n_parts, void* d_out, size_t cap, uint64_t* offsets, void* stream);
/* Whitelist abundance and the resolution of ambiguous barcodes, on the device (k_whitelist.hip): what recovers the records that
 * ibu_correct_barcodes classes 2 (two or more whitelist entries one substitution away) with a prior, as Cell Ranger and STARsolo
 * (1MM_multi) do — the candidate that carries nearly all of the exactly matching reads among the candidates wins.  Records carry no
 * base qualities, so the prior is the whole posterior, in integers.  The reference has nothing like this; the semantics are this
 * library's and are stated in full here.
 * An ABUNDANCE belongs to one whitelist and one context.  It holds one uint64_t counter per slot of the whitelist's table and one for
 * the all-ones key, which never enters the table: a counter for every whitelist entry.  All counters are zero after create and after
 * reset.  Create is synchronous; reset is asynchronous on `stream`.  info: device_bytes (nullable) = what the counters take, 8 bytes
 * per table slot + 8.  Destroy the abundance before its whitelist, and both before their context.  A NULL ctx on a host without a
 * device: IBU_ERR_NO_DEVICE (ibu_abundance_create).  A whitelist, abundance or context that do not belong together:
 * IBU_ERR_INVALID_ARG, in every call below.
 *
 * ibu_abundance_add: record i CONTRIBUTES when d_class == NULL, or when d_class[i] < 8 and bit d_class[i] of class_mask is set.  For
 * such a record, low = barcode & mask(2*bc_len); if low is in the whitelist, its counter grows by one.  Records whose low is not in
 * the whitelist are skipped silently: d_class == NULL on raw records counts the exact hits, class_mask = 0b0011 on the records and
 * classes ibu_correct_barcodes left counts exact and corrected reads.  Asynchronous; reads only (records 8-byte aligned, class bytes
 * at any alignment).  Counters accumulate over calls, and calls on several streams may add to one abundance at once: the adds are
 * integer atomics, and the result does not depend on the order of the records or of the calls.  n == 0 is OK and touches nothing.
 * n < 2^40 per call, and no counter ever exceeds 2^40: the library keeps, on the host, the running total of records OFFERED to add
 * since create / reset (n per call, whatever contributes), and a call that would take it past 2^40 is refused with
 * IBU_ERR_INVALID_ARG (detail.a = the total so far, detail.b = n) and adds nothing.
 * Reads 24 B per record (+ 1 B of class) and a table line for each contributing barcode; one 8-byte atomic add per run of records
 * with equal counter inside a 128-record tile — one per counted record on input in read order, one per tile and barcode on sorted
 * input.
 *
 * ibu_abundance_counts: d_counts[j] = the counter of d_codes[j] (k codes and k counts in DEVICE memory, 8-byte aligned); 0 for a code
 * that is not in the whitelist, and 0 for a code with bits at or above 2*bc_len.  Asynchronous.  k == 0 is OK.  The read-back for
 * users and tests.
 *
 * ibu_resolve_barcodes: every record with d_class[i] == 2 (IBU ambiguous) is EXAMINED; no other record is read or written.  Its
 * CANDIDATES are the neighbours of low that are in the whitelist — the neighbour set of ibu_correct_barcodes, recomputed here.
 * total = the sum of the candidates' counters, best = the largest.  The record is RESOLVED iff best > 0 and best * den >= num * total
 * (integers; equality passes, as in the set test of ibu_filter_barcodes).  1 <= num <= den < 2^24 and 2 * num > den are required
 * (anything else: IBU_ERR_INVALID_ARG, whatever n is): a share above one half makes the winner unique, so there is no tie rule, and
 * with counters of at most 2^40 no product overflows 64 bits.  A resolved record gets the winner in the low 2*bc_len bits of its
 * barcode — the bits above, umi and index are untouched — and its class byte becomes IBU_BARCODE_RESOLVED (4).  Otherwise record and
 * class byte stay as they are.  d_class is required (NULL with n > 0: IBU_ERR_INVALID_ARG), n bytes at any alignment.
 * counts (nullable): examined; resolved; below_share = examined records with total > 0 that were not resolved; unseen = those with
 * total == 0 (the three sum to examined).  Non-NULL synchronises `stream`, NULL leaves the call asynchronous; the totals pass through
 * the context under the rule ibu_correct_barcodes states: of the calls in flight on one context, at most one may ask.
 * n == 0 is OK and touches nothing (counts = 0).  n < 2^40.  A refused call touches nothing.
 * ibu_select_records(..., keep_mask = 0b10011) then keeps exact, corrected and resolved records.  Resolve adds nothing to the
 * abundance, so a second call finds no class-2 record it could resolve and changes nothing more.
 * Reads 1 B of class per record, sixteen per lane and load where the alignment of d_class allows; gathers the 8 barcode bytes of the
 * class-2 records only; a wave examines its class-2 records one after the other, 64 neighbours (probe and counter) at a time. */
#define IBU_BARCODE_RESOLVED 4
typedef struct ibu_abundance ibu_abundance_t;
typedef struct ibu_resolve_counts { uint64_t examined, resolved, below_share, unseen; } ibu_resolve_counts_t;
int32_t ibu_abundance_create(ibu_ctx_t* ctx, const ibu_whitelist_t* wl, void* stream, ibu_abundance_t** out);
int32_t ibu_abundance_reset(ibu_abundance_t* ab, void* stream);
int32_t ibu_abundance_info(const ibu_abundance_t* ab, size_t* device_bytes);
void ibu_abundance_destroy(ibu_abundance_t* ab); /* before its whitelist is destroyed */
int32_t ibu_abundance_add(ibu_ctx_t* ctx, ibu_abundance_t* ab, const void* d_records, const uint8_t* d_class, size_t n,
                          uint32_t class_mask, void* stream);
int32_t ibu_abundance_counts(ibu_ctx_t* ctx, const ibu_abundance_t* ab, const uint64_t* d_codes, size_t k, uint64_t* d_counts,
                             void* stream);
int32_t ibu_resolve_barcodes(ibu_ctx_t* ctx, const ibu_whitelist_t* wl, const ibu_abundance_t* ab, void* d_records, size_t n,
                             uint64_t num, uint64_t den, uint8_t* d_class, ibu_resolve_counts_t* counts, void* stream);
/* Per-barcode labels onto records, on the device (k_whitelist.hip): what carries a verdict that exists per BARCODE — the hashtag a
 * cell was assigned (ibu_assign_rows), a cluster id, a doublet flag, a QC verdict — onto the records of ANY library that shares the
 * barcodes, in any order, so that ibu_select_records can split a library into its samples and a lane can report its reads per sample.
 * Every other class byte this library writes comes from a walk over the same records; this one comes from a table keyed by barcode.
 * The reference has nothing like this; the semantics are this library's and are stated in full here.
 * A LABEL TABLE (ibu_labels_t) belongs to one whitelist and one context, as an abundance does.  It holds one byte per slot of the
 * whitelist's table and one for the all-ones key, which never enters the table: a label for every whitelist entry.
 *
 * ibu_labels_create: every entry's label starts as `fill` (at most 255).  Synchronous.  A NULL ctx on a host without a device:
 * IBU_ERR_NO_DEVICE.  info: device_bytes (nullable) = what the labels take, one byte per table slot + 1.  Destroy the labels before
 * their whitelist, and both before their context.  Labels or a whitelist created on another context: IBU_ERR_INVALID_ARG, in every
 * call below.  (No call takes labels and a whitelist together: labels always act through the whitelist they were created on.)
 *
 * ibu_labels_set: the label of d_codes[j] becomes d_labels[j], for j in [0, k) (DEVICE memory: the codes 8-byte aligned, the label
 * bytes at any alignment).  A code with bits at or above 2*bc_len, or a code that is not in the whitelist, is SKIPPED: nothing is
 * written for it, and *n_skipped (host, nullable) counts such codes.  A non-NULL n_skipped synchronises `stream` (the count passes
 * through the context under the rule ibu_correct_barcodes states for `counts`); NULL leaves the call asynchronous.  The codes are
 * meant to be distinct: if one code occurs twice in a call with different labels the entry ends as one of them, as a whole byte.  A
 * later call overrides an earlier one, in stream order.  k == 0 is OK.  k < 2^40.
 *
 * ibu_labels_get: d_labels_out[j] = the label of d_codes[j]; `missing` (at most 255) for a code that is not an entry — not in the
 * whitelist, or with bits at or above 2*bc_len.  Asynchronous.  k == 0 is OK.  The read-back for users and tests.
 *
 * ibu_label_records: for record i, low = barcode & mask(2*bc_len); the record is FOUND when low is a whitelist entry, and its label
 * is that entry's byte.
 *   flags == 0 (plain mode): d_class[i] = the label when found, otherwise missing_class, which may be any byte.
 *   flags == IBU_LABEL_MATCH (match mode): d_class[i] = IBU_LABEL_IS (0) when the record is found and its label equals `match`,
 *     IBU_LABEL_OTHER (1) when it is found with another label, IBU_LABEL_MISSING (2) when it is not found.
 *     ibu_select_records(..., keep_mask = 1 << IBU_LABEL_IS) then extracts the records of any one of up to 256 labels;
 *     ibu_select_records never keeps class bytes above 7, so match mode is the only way to reach labels 8 and above.
 * hist (host, uint64_t[257], nullable): hist[l] = the number of found records with label l, hist[256] = the number of records not
 * found — in either mode, whatever `match` is; the 257 entries sum to n.  A non-NULL hist synchronises `stream`, NULL leaves the
 * call asynchronous; the totals pass through the context under the rule ibu_correct_barcodes states: of the calls in flight on one
 * context, at most one may ask for totals.  d_class (nullable): n bytes at any alignment.  d_class == NULL with hist != NULL is the
 * "reads per label" query: it reads 24 B per record and writes nothing per record.  (Both NULL: the call checks its arguments and
 * does nothing.)  The records (8-byte aligned) are never written.  n == 0 is OK and touches nothing (hist = 0).  n < 2^40.
 * IBU_ERR_INVALID_ARG: labels of another context, a flag bit other than IBU_LABEL_MATCH, match or missing_class above 255 (in either
 * mode), a NULL or misaligned d_records with n > 0.  A refused call touches nothing, hist included.  A NULL ctx on a host without a
 * device: IBU_ERR_NO_DEVICE, as for create — there is no host form to fall back to.
 * Reads 24 B per record, a table line for its barcode and one gathered label byte; writes 1 B of class.  The histogram costs no
 * global atomic per record: runs of equal label inside a 128-record tile are merged, run lengths go into a per-workgroup histogram
 * in LDS, and every workgroup adds its non-zero bins to the totals once, at the end of its sweep; a call without hist runs a kernel
 * that has none of it. */
#define IBU_LABEL_MATCH 1u
#define IBU_LABEL_IS 0
#define IBU_LABEL_OTHER 1
#define IBU_LABEL_MISSING 2
#define IBU_LABEL_BINS 257u
typedef struct ibu_labels ibu_labels_t;
int32_t ibu_labels_create(ibu_ctx_t* ctx, const ibu_whitelist_t* wl, uint32_t fill, void* stream, ibu_labels_t** out);
int32_t ibu_labels_info(const ibu_labels_t* lb, size_t* device_bytes);
void ibu_labels_destroy(ibu_labels_t* lb); /* before its whitelist is destroyed */
int32_t ibu_labels_set(ibu_ctx_t* ctx, ibu_labels_t* lb, const uint64_t* d_codes, const uint8_t* d_labels, size_t k, size_t* n_skipped,
                       void* stream);
int32_t ibu_labels_get(ibu_ctx_t* ctx, const ibu_labels_t* lb, const uint64_t* d_codes, size_t k, uint32_t missing,
                       uint8_t* d_labels_out, void* stream);
int32_t ibu_label_records(ibu_ctx_t* ctx, const ibu_labels_t* lb, const void* d_records, size_t n, uint32_t flags, uint32_t match,
                          uint32_t missing_class, uint8_t* d_class, uint64_t* hist, void* stream);
/* BGZF / DEFLATE on the device (k_inflate.hip).  A bgzip file — to niffler (src/io/reader.rs:345-352) a gzip stream of many
 * members — is a chain of independent deflate blocks of at most 64 KiB whose compressed and uncompressed sizes stand in their
 * headers and trailers: the blocks can be found without inflating them, their COMPRESSED bytes can cross the PCIe link (half the
 * bytes of a records file) and every block can go to a wave of its own.
 * ibu_bgzf_scan (host): walks the block headers in buf[0, len) and describes up to `cap` whole blocks: comp_offset / comp_len = the
 * raw deflate bytes inside the member (behind FEXTRA and, when their flags are set, FNAME, FCOMMENT and FHCRC), out_len and crc32
 * from its trailer, out_offset = the sum of the out_len before it.  Reserved flag bits and a wrong header CRC-16 are refused as
 * zlib refuses them.
 * *consumed = bytes of buf the described blocks cover (the next call starts there), *out_bytes = their uncompressed size.  A
 * member that is not a BGZF block, or one that is cut off with final != 0: IBU_ERR_NIFFLER (the blocks in front of it are
 * described, *n_blocks says how many); a block that is not whole yet with final == 0 ends the walk quietly.
 * ibu_inflate_blocks_device: inflates the n blocks d_blocks describes (device memory, comp_offset relative to d_comp, out_offset
 * — signed — relative to d_out) — d_comp must be readable IBU_INFLATE_PAD bytes past the last block's end — and verifies length,
 * the end of the deflate stream on the block's last byte and the CRC-32, exactly as the host decoder does.  d_status[i] = 0 good /
 * 1 not a valid deflate stream of these sizes / 2 CRC-32 mismatch; *d_first_bad (device; the caller sets it to 0xFFFFFFFF) = the
 * lowest bad block.  A block writes only its own out_len bytes.  Asynchronous on `stream`; the lanes' tables live in the context's
 * sort scratch (calls of more than 49 152 blocks; one such call per context at a time, as for the sort).  One LANE per block: 64
 * blocks per wave; BGZF level 1 of 16/12 records: 53 GB/s of output for 1e8 records, 100 GB/s for 3e8 (the 16 host inflate threads
 * of the same box: 9.6).
 * A wave takes ~46 ms for its 64 blocks whatever the call's size, so a call wants tens of thousands of blocks:
 * ibu_load_bgzf_to_device (above) and the range loads of ibu_stream_open_path (below) are the library's own uses of it; the streams over
 * a Reader or a map keep the host inflate (a ring slot holds too few blocks). */
#define IBU_INFLATE_PAD 2048
typedef struct ibu_inflate_block {
  uint64_t comp_offset;
  int64_t out_offset;
  uint32_t comp_len, out_len, crc32, reserved;
} ibu_inflate_block_t;
int32_t ibu_bgzf_scan(const uint8_t* buf, size_t len, int32_t final, ibu_inflate_block_t* blocks, size_t cap, size_t* n_blocks,
                      size_t* consumed, uint64_t* out_bytes);
int32_t ibu_inflate_blocks_device(ibu_ctx_t* ctx, const void* d_comp, const ibu_inflate_block_t* d_blocks, size_t n, void* d_out,
                                  uint32_t* d_status, uint32_t* d_first_bad, void* stream);
/* For each of the k key records d_keys[j] (24 B each): the first position p in the SORTED device records with
 * records[p] >= key under ibu_record_cmp (record.rs:58), i.e. slice::partition_point(|r| r < key); n if there is none.
 * Positions land in d_pos[0..k) on the device; asynchronous on `stream`.  This is the splitter search of the
 * multi-GPU sample sort (ibu_amd/sharding.py): one launch for all splitters instead of a host binary search. */
int32_t ibu_lower_bound_records(ibu_ctx_t* ctx, const void* d_sorted_records, size_t n, const void* d_keys, size_t k,
                                uint64_t* d_pos, void* stream);
/* ---- compacted keys: the bytes of a set of records that VARY, as 12-byte elements --------------------------------------
 * A record is 24 bytes, but of 16-base barcodes, 12-base UMIs and indices below 2^32 only 4 + 3 + 4 bytes differ between
 * records.  ibu_sort_records sorts such inputs as 12-byte elements internally; these entry points expose the same
 * transformation so that the multi-GPU sort (ibu_amd/sharding.py) ships elements instead of records through its one
 * all-to-all — half the bytes over the point-to-point xGMI links.  There is no reference counterpart (the crate has no sort
 * and no exchange); the records that come out are the records that went in (record.rs:58-66), byte for byte.
 *
 * ibu_records_census: out[0..2] = OR of barcode / umi / index over the n records, out[3..5] = AND (n = 0: 0 and ~0, the
 *   identities, so words of several shards combine with | and &), out[6] != 0: some index is smaller than its
 *   predecessor's, out[7] != 0: some record is smaller than its predecessor (not sorted).  Synchronises `stream`.
 * ibu_key_plan_init: the plan for records whose OR / AND words are given (one shard's, or all shards' combined — every
 *   rank must use the same plan).  plan->k = number of varying bytes; compact / expand need k <= 12
 *   (IBU_ERR_INVALID_ARG otherwise).  Element byte j = the j-th least significant varying byte of the key (index bytes
 *   first, barcode bytes last): elements compared as 96-bit little-endian integers order like the records.
 * ibu_records_compact: n records -> n elements (12 n bytes at d_elems, 4-byte aligned).  ibu_records_expand: the inverse.
 *   Asynchronous on `stream`; record arrays that are 8- but not 16-byte aligned (a shard at an odd record) peel one record. */
typedef struct ibu_key_plan {
  uint32_t csel[4][3]; /* byte-gather selectors, records -> elements (v_perm_b32); row 3: the sort's 16-byte elements */
  uint32_t xsel[6][2]; /* elements -> records */
  uint32_t k;          /* varying bytes */
  uint32_t index_bytes; /* how many of them belong to the index (the least significant element bytes) */
  uint64_t base[3];    /* the constant bytes of barcode / umi / index */
} ibu_key_plan_t;
int32_t ibu_records_census(ibu_ctx_t* ctx, const void* d_records, size_t n, uint64_t out[8], void* stream);
int32_t ibu_key_plan_init(const uint64_t or_words[3], const uint64_t and_words[3], ibu_key_plan_t* plan);
int32_t ibu_records_compact(ibu_ctx_t* ctx, const ibu_key_plan_t* plan, const void* d_records, size_t n, void* d_elems, void* stream);
int32_t ibu_records_expand(ibu_ctx_t* ctx, const ibu_key_plan_t* plan, const void* d_elems, size_t n, void* d_records, void* stream);
/* `a == b` on two device-resident slices of n records each (Record derives PartialEq / Eq, record.rs:58): *first = the
 * index of the first record that differs, n if none does.  8-byte aligned inputs (16-byte: the fast path).  Synchronises. */
int32_t ibu_records_first_mismatch(ibu_ctx_t* ctx, const void* d_a, const void* d_b, size_t n, uint64_t* first, void* stream);
/* 1 if the n records are non-decreasing under ibu_record_cmp. Synchronises. */
int32_t ibu_is_sorted(ibu_ctx_t* ctx, const void* d_records, size_t n, void* stream,
                      int32_t* sorted);

/* ======================================================================================= */
/* Record streams: file / mmap / gzip  <->  device, through a pinned ring                   */
/* ======================================================================================= */
typedef struct ibu_ring_config {
  uint32_t slots;        /* pinned hipHostMalloc staging slots (>= 2; default 4)             */
  uint32_t slot_records; /* records per slot (default IBU_BATCH_SIZE * 4 = 96 MiB)           */
  uint32_t feeder_threads; /* host threads copying mmap pages into a slot (default 4)        */
  uint32_t reserved;
} ibu_ring_config_t;

typedef struct ibu_stream_stats {
  uint64_t records;
  uint64_t bytes_h2d;
  uint64_t bytes_d2h;
  uint64_t batches;
  double seconds_total;
  double seconds_kernel; /* sum of hipEvent kernel spans */
  int32_t numa_node;     /* ABI revision 4: node of the device the stream fed (-1: unknown or option "numa" = 0) */
  int32_t ring_node;     /* node the pinned ring's pages are on (-1: the kernel would not say) */
} ibu_stream_stats_t;

/* Device analogue of load_to_vec (reader.rs:510-535): whole uncompressed file -> device AoS
 * buffer of *n records.  If *d_records is NULL the library hipMallocs it (release with
 * ibu_device_free); otherwise cap_records bounds it. */
int32_t ibu_load_to_device(ibu_ctx_t* ctx, const char* path, const ibu_ring_config_t* cfg,
                           ibu_header_t* header, void** d_records, size_t cap_records, size_t* n,
                           ibu_stream_stats_t* stats);
/* The same for a BGZF (bgzip) file of the records, INFLATED ON THE DEVICE: the compressed bytes cross the link (half of them for a
 * 16/12 records file) and every block inflates straight to its place among the records (ibu_inflate_blocks_device below; the block
 * headers are walked on a thread of their own while the copies run; 1e8 records: 0.074 s against 0.25 s through the Reader; 1e9:
 * 0.31 s — the PLAIN file of the same records: 0.44 s; large files get one launch of the decoder ahead of the copies whose waves wait
 * for their blocks to arrive).  The result is what ibu_load_to_device gives for the gunzipped file — the
 * reference's load_to_vec does not decompress (reader.rs:510-535 reads the file as it is; its Reader does, through niffler,
 * :345-352): this is the bulk form of that Reader path.  Header too short: IBU_ERR_IO; invalid header: as ibu_header_validate;
 * (length - 32) % 24 != 0: IBU_ERR_INVALID_MAP_SIZE; a member that is not a BGZF block, a file that ends inside one, a block that
 * does not inflate to its announced length and CRC-32: IBU_ERR_NIFFLER (an ordinary gzip file: use the Reader).  The context keeps
 * the file size + 36 bytes per block of device memory as staging until it is destroyed (it grows only; option "release_staging" frees
 * it).  A file larger than the device's memory is loaded range by range with the _shard_ form below (every call walks the block
 * headers again: 10 ms per 6 GB). */
int32_t ibu_load_bgzf_to_device(ibu_ctx_t* ctx, const char* path, const ibu_ring_config_t* cfg, ibu_header_t* header, void** d_records,
                                size_t cap_records, size_t* n, ibu_stream_stats_t* stats);
/* ... and shard `shard` of `n_shards` of its records — the contiguous range ibu_shard_range gives (the split of process_parallel,
 * mmap.rs:297-307), *first_record (nullable) = its first record's number: every device of a node loads its own range of the same file,
 * only that range's blocks cross its link (the at most two blocks that straddle the range's ends are inflated on the host, like the
 * blocks that hold the header).  ibu_load_bgzf_to_device is shard 0 of 1. */
int32_t ibu_load_bgzf_shard_to_device(ibu_ctx_t* ctx, const char* path, const ibu_ring_config_t* cfg, size_t shard, size_t n_shards,
                                      ibu_header_t* header, void** d_records, size_t cap_records, size_t* n, uint64_t* first_record,
                                      ibu_stream_stats_t* stats);

/* Device analogue of Writer::write_batch (writer.rs:315-351): n device-resident AoS records
 * are copied back through the ring and appended to the writer (same buffered/direct rules).
 * Stream ordering: the copies are ordered behind ibu_ctx_stream(ctx).  Records produced by a kernel entry point that was
 * given another stream: use ibu_writer_write_batch_device_on below (or complete them first).  ibu_codec_status reads ONE
 * status word per context: encodes issued on several streams share it. */
int32_t ibu_writer_write_batch_device(ibu_writer_t* w, ibu_ctx_t* ctx, const ibu_ring_config_t* cfg,
                                      const void* d_records, size_t n, ibu_stream_stats_t* stats);
/* The same, with the stream the records were produced on (a kernel entry point that was given `stream`, e.g. a sort on the
 * caller's stream): the copies wait for the work queued on `producer_stream` so far; NULL = ibu_ctx_stream(ctx), i.e. the
 * call above. */
int32_t ibu_writer_write_batch_device_on(ibu_writer_t* w, ibu_ctx_t* ctx, const ibu_ring_config_t* cfg,
                                         const void* d_records, size_t n, void* producer_stream, ibu_stream_stats_t* stats);

/* ---- pull-style device record stream ------------------------------------------------------------------------------------
 * The device form of Reader::read_batch + Iterator (reader.rs:218-242, :279-306) and of the per-batch loop of process_parallel
 * (mmap.rs:312-320): the CALLER pulls one device-resident batch at a time and runs whatever it likes on it — its own kernels,
 * or this library's (decode, sort, reduce, aggregation) — the user half of ParallelProcessor (parallel.rs:100-190) with the
 * records already in HBM.  ibu_mmap_process_device / ibu_reader_process_device (below) are this loop with one of the two
 * built-in processors as the body; there is one pipeline.
 *
 *   source --producer thread (+ feeders)--> pinned slot --copy stream H2D--> device slot --ibu_stream_next--> caller
 *
 * open: the stream borrows the context's ring (cfg as for the other stream calls) and starts a producer thread that fills
 *   pinned slots from the source and queues their H2D copies; the first batch is on its way before the first next().  Until
 *   close, the context's other ring users (load_to_device, write_batch_device, process_device, another stream) return
 *   IBU_ERR_INVALID_ARG; kernel entry points, the sort and the host<->host codec pipelines are unaffected.  A reader source is
 *   borrowed, read from where it stands (records already buffered by read_batch / next come first) and must not be touched
 *   until close; an mmap source is one shard of the static split (ibu_shard_range).
 * next: *d_records = the batch (a device ring slot: *n records of 24 bytes, 16-byte aligned), *first_index = the number of the
 *   batch's first record (mmap: its position in the map; reader: records this stream delivered before it).  `stream`
 *   (NULL = ibu_ctx_stream(ctx)) is the stream the caller will read the batch on: it is made to wait for the batch's copy, so
 *   work queued on it afterwards sees the records.  *n == 0 with IBU_OK: the end of the stream (again on every later call).
 *   Batches are whole slots except the last; their concatenation is the source's record sequence.  Blocks while no batch is ready.
 * release: the caller is done queueing work on the batch; the slot is refilled once everything queued on `stream` so far has
 *   run.  Batches may be held and released in any order, at most slots - 1 at a time: next() with every slot held returns
 *   IBU_ERR_INVALID_ARG instead of waiting for ever.
 * Errors of the source surface in order: next() first hands out every batch in front of the error, then returns it, and
 *   keeps returning it.  A stream that ends inside a record is TruncatedRecord{pos} with the reference's position, after
 *   exactly the records the reference's iterator yields before its Err: whole refills of IBU_DEFAULT_BUFFER_SIZE counted from
 *   where the stream took over; the complete records of the final partial refill are dropped with it (quirk Q8,
 *   reader.rs:232-237).
 * close: stops the producer (a producer blocked inside the source — a pipe nobody writes to — is waited for: close the writing end
 *   first), waits for the copies in flight and for the context's stream, returns the ring.  Batches still held are invalid
 *   afterwards.  The reader / map stays open and is the caller's to close.  ibu_ctx_destroy under an open stream shuts the
 *   stream down first (producer joined, ring returned); the handle stays valid for ibu_stream_close only.
 * A source error (Io, Niffler) inside a refill behaves like the truncation: the whole refills in front of it are delivered,
 *   the refill under way is lost with the error (reader.rs:225-230). */
typedef struct ibu_stream ibu_stream_t;
int32_t ibu_stream_open_reader(ibu_reader_t* r, ibu_ctx_t* ctx, const ibu_ring_config_t* cfg, ibu_stream_t** out);
int32_t ibu_stream_open_mmap(const ibu_mmap_t* m, ibu_ctx_t* ctx, const ibu_ring_config_t* cfg, size_t shard, size_t n_shards,
                             ibu_stream_t** out);
/* Reader::from_path + the stream (reader.rs:345-352; ABI revision 5): opens `path` once (one descriptor) and sniffs it.  The stream owns
 * its source and closes it.
 * A BGZF file the device load takes (every member a BGZF block, whole records, a valid header; context option "bgzf_device" = 1, the
 *   default) is read in RANGES: only a range's compressed bytes cross the link (through the ring's pinned slots), its blocks are
 *   inflated on the device (ibu_inflate_blocks_device's decoder; the blocks straddling the range's ends on the host), and next() hands
 *   out views into the range's device buffer.  Open builds the block index (one walk) and sizes the inflate staging for the largest range.
 *   Ranges: about option "bgzf_range_bytes" compressed bytes (default 3.2 GB, ~6.4 GB of 16/12 records); every range but the last holds a
 *     multiple of IBU_DEFAULT_BUFFER_SIZE's 49 152 records, and of lcm(slot_records, 49 152) where that is no larger than the range —
 *     with the default ring every batch but the last is then a whole slot.  A batch holds at most slot_records records, is 16-byte
 *     aligned and never spans two ranges.
 *   Two range buffers: range k + 1 is copied and inflated while the caller works on the batches of range k.  A buffer is loaded again
 *     only once every batch of it has been released AND the work queued on the release streams has run.  next() that would need a
 *     buffer whose batches the caller still holds returns IBU_ERR_INVALID_ARG at once (as with every slot held); after a release the
 *     same call succeeds.
 *   Device memory: the two range buffers (2 x range records x 24 B; the second is allocated only when a second range is loaded) plus
 *     the inflate staging (the largest range's compressed bytes, descriptors and tables).  The context keeps all of them after close,
 *     like the staging of ibu_load_bgzf_to_device, and they grow only: the next stream or call does not allocate them again.  Option
 *     "release_staging" frees them; it is refused while such a stream is open.
 *   Launch form: every range launches the decoder ahead of its copies (its waves wait for their bytes), as the load does, also while
 *     the caller's kernels run on the range before: measured against launching behind the last copy in launches of eight waves per CU
 *     (context option "bgzf_stream_ahead" = 0), it was as fast at 1e8 records and 3 % faster at 1e9.
 *   The caller may run the library's kernels (decode, sort, barcode counts, reduce) on a held batch on the same context while the
 *     next range loads: the loader's tables live in the inflate staging and its copies and launches go out on its own streams only.
 *   Errors: a block the device refuses in the first range sends the whole file through the host path below.  In a later range the
 *     host inflate takes over at the range's first record (a refill boundary): the stream ends with exactly the records and the
 *     error ibu_stream_open_reader gives on the same file.
 *   Stats: bytes_h2d = the compressed file bytes the loads copied over the link (a file of one range: the whole file, as
 *     ibu_load_bgzf_to_device), plus the record bytes of the host path after a takeover; batches / records = what was queued.
 * Anything else (a plain file, one gzip member, zstd / xz / bz2, a BGZF file with a foreign member, a cut, a bad header, "bgzf_device"
 *   = 0): exactly ibu_stream_open_reader over ibu_reader_open_fd of the same descriptor — the same batches, errors and stats. */
int32_t ibu_stream_open_path(const char* path, ibu_ctx_t* ctx, const ibu_ring_config_t* cfg, ibu_stream_t** out);
int32_t ibu_stream_header(const ibu_stream_t* s, ibu_header_t* out);
int32_t ibu_stream_next(ibu_stream_t* s, void* stream, const void** d_records, size_t* n, uint64_t* first_index);
int32_t ibu_stream_release(ibu_stream_t* s, const void* d_records, void* stream);
/* records / batches / bytes_h2d delivered so far, seconds since open, the NUMA fields; seconds_kernel is 0 (the kernels are the caller's) */
int32_t ibu_stream_stats(const ibu_stream_t* s, ibu_stream_stats_t* out);
void ibu_stream_close(ibu_stream_t* s);

/* Device processors for process_parallel. */
enum {
  IBU_PROC_REDUCE = 1, /* count + sums + xors -> ibu_reduce_result_t                         */
  IBU_PROC_DECODE = 2  /* fused decode of every batch into caller-provided device columns    */
};
typedef struct ibu_decode_sink {
  uint8_t* d_bc_ascii; /* cap_records * bc_len bytes (NULL: skip the column) */
  uint8_t* d_umi_ascii;
  uint64_t* d_index;
  size_t cap_records;  /* rows every non-NULL column can hold (ABI revision 3).  A compressed stream does not say how many
                        * records it holds before it ends: the moment a batch would not fit, the call stops, drains the ring
                        * and returns IBU_ERR_INVALID_ARG (detail.a = rows needed so far, detail.b = cap_records) — never a
                        * write past the columns.  An mmap shard is checked before any work starts. */
} ibu_decode_sink_t;

/* Device analogue of MmapReader::process_parallel (mmap.rs:286-332) for ONE shard of the
 * static split: shard `shard` of `n_shards` (one per GPU / rank) streams its record range
 * through the pinned ring in IBU_BATCH_SIZE-multiples, H2D || kernel overlapped on two
 * streams.  `sink` is ibu_reduce_result_t* or ibu_decode_sink_t* according to `proc`. */
int32_t ibu_mmap_process_device(const ibu_mmap_t* m, ibu_ctx_t* ctx, const ibu_ring_config_t* cfg,
                                int32_t proc, size_t shard, size_t n_shards, void* sink,
                                ibu_stream_stats_t* stats);

/* MmapReader::process_parallel(processor, n) (mmap.rs:286-332) with a GPU per worker, in ONE call: worker i = one host thread
 * + one context on devices[i], shard i of the static split (ibu_shard_range(len, n_devices, i): per = len / n, remainder to
 * the last), workers joined in spawn order, the first error in that order is the call's (quirk Q12; the other workers still
 * run to completion, as the reference's detached threads do).  n_devices == 0: every visible device, as num_threads == 0
 * means every core (mmap.rs:292-296); an ordinal may appear more than once (two workers sharing a GPU).
 *   proc == IBU_PROC_REDUCE: `sinks` = NULL or ibu_reduce_result_t[n_devices] (the per-device partials); *total (nullable) =
 *     their sum — count and the three sums wrapping mod 2^64, the three XORs — added on the host: seven words per device,
 *     no collective (the path shards with no exchange step).
 *   proc == IBU_PROC_DECODE: `sinks` = ibu_decode_sink_t[n_devices]; sink i's columns live on devices[i] and hold shard i's
 *     rows (row r of the shard at column + r * len); total->count = records decoded.
 * `stats`: NULL or ibu_stream_stats_t[n_devices].  The context form takes contexts the caller keeps (their rings, streams and
 * scratch are reused from call to call); the device form creates and destroys one context per entry. */
int32_t ibu_mmap_process_devices(const ibu_mmap_t* m, const int32_t* devices, size_t n_devices, const ibu_ring_config_t* cfg,
                                 int32_t proc, void* sinks, ibu_reduce_result_t* total, ibu_stream_stats_t* stats);
int32_t ibu_mmap_process_contexts(const ibu_mmap_t* m, ibu_ctx_t* const* ctxs, size_t n_ctxs, const ibu_ring_config_t* cfg,
                                  int32_t proc, void* sinks, ibu_reduce_result_t* total, ibu_stream_stats_t* stats);

/* Streaming Reader (plain or gzip; reader.rs:345-352 path) -> device processor: host inflate
 * thread -> pinned ring -> H2D || kernel.  Consumes the reader to EOF.
 * A reader opened by ibu_reader_open_path on a BGZF file from which nothing has been read yet: the loop runs over the device form of
 * ibu_stream_open_path on the reader's own file (a descriptor of its own on the file the reader has open, so a name renamed or
 * replaced since does not matter and the reader's position never moves), with the reader as its host path — the compressed bytes
 * over the link, the blocks inflated on the device, range k + 1 loaded while the processor runs on range k (context option
 * "bgzf_device" = 1, the default; 0: through the Reader's host inflate): 1e8 records REDUCE / DECODE 1.3 G records/s instead of 0.4.
 * Same results; the reader stands at its end afterwards; stats as for that stream (bytes_h2d = the compressed bytes: the file's size
 * for a file of one range).  A file that form does not take (a foreign member, a cut, a length that is no whole number of records,
 * another header, a block the device refuses in the first range) goes through the Reader's own path and fails as it fails there; a
 * block refused in a later range ends the call with the records and the error of the Reader's path, as the stream does. */
int32_t ibu_reader_process_device(ibu_reader_t* r, ibu_ctx_t* ctx, const ibu_ring_config_t* cfg,
                                  int32_t proc, void* sink, ibu_stream_stats_t* stats);

/* ---- host <-> host codec pipelines (data starts and ends in host memory / a file) ------------------------ */
/* One shard of an MmapReader -> barcode / UMI ASCII and the index column IN HOST MEMORY: the reference's
 * consumer loop (MmapReader::slice / process_parallel -> Record -> sequences, mmap.rs:253-332 + the 2-bit
 * table record.rs:19-27) with the unpacking done on the GPU: map -> pinned ring -> H2D -> K2 decode -> D2H ->
 * caller buffers, three streams overlapped.  Buffers hold shard_records rows (row i of the shard at
 * h_bc_ascii + i*bc_len ...); any of them may be NULL to skip that column.
 * WHEN NOT TO CALL THIS: whenever the columns are wanted in HOST memory and nothing else runs on the device.  Every record
 * crosses PCIe twice (24 B in, bc_len + umi_len + 8 B out) between two host copies (map -> pinned, pinned -> caller, the
 * second one faulting in the caller's fresh pages), and the kernel is 2 % of the wall time: 0.3-0.7 G records/s at 16/12 on
 * a one-GPU box of this pool into FRESH output arrays at every size from 1e6 to 1e9 records (tools/e2e.py rows "mmap
 * decode_to_host": the rate does not grow with the size, so there is no crossover) — 58 of 145 ms at 1e8 records are the
 * kernel's page faults on 3.6 GB of new pages, which neither more threads nor MADV_POPULATE_WRITE ahead of the copies make
 * cheaper (profiles/r04_k_*) — and 1.15-1.2 G records/s into arrays that have been written before (a reused buffer); a
 * plain loop over MmapReader::slice with a scalar 2-bit unpack on the same box's 16 CPUs decodes AND re-encodes 0.55-0.84 G
 * records/s (bench.py: cpu_baseline) and pays the same page faults.  The call exists so that the
 * API is complete for consumers that hold their sequences in host memory; the device pays off when the columns STAY
 * resident — ibu_mmap_process_device(s) with IBU_PROC_DECODE (2.2 G records/s, PCIe-bound one way) and everything behind
 * it (sort, per-barcode aggregation, re-encoding) at HBM rates. */
int32_t ibu_mmap_decode_to_host(const ibu_mmap_t* m, ibu_ctx_t* ctx, const ibu_ring_config_t* cfg, size_t shard,
                                size_t n_shards, uint8_t* h_bc_ascii, uint8_t* h_umi_ascii, uint64_t* h_index,
                                ibu_stream_stats_t* stats);
/* n rows of barcode / UMI ASCII in host memory (+ optional index column; NULL -> first_index + i) -> 2-bit
 * records -> the writer: README.md:38-47's "sequences -> Record::new -> writer.write_record" loop as one
 * batch call (H2D -> K3 encode -> D2H -> Writer::write_batch's buffered/direct rule, writer.rs:321-351).
 * A byte outside ACGTacgt: IBU_ERR_INVALID_BASE (detail.a = first offending row, detail.b = offending
 * rows); batches before the first offending one are already written, nothing from it on is. */
int32_t ibu_writer_write_ascii_batch(ibu_writer_t* w, ibu_ctx_t* ctx, const ibu_ring_config_t* cfg,
                                     const uint8_t* h_bc_ascii, const uint8_t* h_umi_ascii, const uint64_t* h_index,
                                     uint64_t first_index, size_t n, uint32_t bc_len, uint32_t umi_len,
                                     ibu_stream_stats_t* stats);

#ifdef __cplusplus
} /* extern "C" */
#endif
#endif /* IBU_HIP_H */
