// ibu.hpp — the reference crate's public API (src/lib.rs:178-181), restated in C++17 ABOVE the C ABI of
// ibu_hip.h.  Header-only; links against libibu_hip.so.  Same names, argument meaning and error behaviour
// as the Rust items, so tests written against it read like the reference's own (tests/cpp/).
//
//   Rust                                   here
//   ------------------------------------   ---------------------------------------------------------------
//   Header / Record (repr(C) PODs)         ibu::Header / ibu::Record — the ABI structs themselves
//   Result<T, IbuError>                    T, or throws ibu::IbuError {kind(), expected/actual/pos/idx/max}
//   Writer<W: Write>                       ibu::Writer — sinks: std::ostream&, Vec<u8> (to_vec), path, stdout
//   Reader<R: Read> + Iterator             ibu::Reader — sources: std::istream&, byte slice, path, stdin;
//                                          next() -> std::optional<Record>; range-for
//   load_to_vec                            ibu::load_to_vec
//   MmapReader (Clone = Arc)               ibu::MmapReader (copy = clone of the shared map)
//   ParallelProcessor / ParallelReader     any copyable type with process_record(const Record&) and
//                                          optionally on_batch_complete(), set_tid(size_t), get_tid();
//                                          MmapReader::process_parallel(proc, num_threads)
//   — (new: device path)                   ibu::device::Context, DeviceBuffer; Writer::write_batch_device,
//                                          MmapReader::process_device_*, Reader::process_device_*
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <istream>
#include <optional>
#include <ostream>
#include <stdexcept>
#include <string>
#include <array>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "ibu_hip.h"

namespace ibu {

constexpr uint32_t MAGIC = IBU_MAGIC;          // header.rs:5
constexpr uint32_t VERSION = IBU_VERSION;      // header.rs:6
constexpr size_t HEADER_SIZE = IBU_HEADER_SIZE;  // header.rs:7
constexpr size_t RECORD_SIZE = IBU_RECORD_SIZE;  // record.rs:3
constexpr size_t DEFAULT_BUFFER_SIZE = IBU_DEFAULT_BUFFER_SIZE;  // reader.rs:14, writer.rs:10 (48 Ki records)

// ---- error.rs:56-128 ------------------------------------------------------------------------------------------
class IbuError : public std::runtime_error {
 public:
  enum Kind {
    Io = IBU_ERR_IO, Niffler = IBU_ERR_NIFFLER, InvalidMagicNumber = IBU_ERR_INVALID_MAGIC,
    TruncatedRecord = IBU_ERR_TRUNCATED_RECORD, InvalidVersion = IBU_ERR_INVALID_VERSION,
    InvalidBarcodeLength = IBU_ERR_INVALID_BC_LEN, InvalidUmiLength = IBU_ERR_INVALID_UMI_LEN,
    InvalidMapSize = IBU_ERR_INVALID_MAP_SIZE, InvalidIndex = IBU_ERR_INVALID_INDEX, Process = IBU_ERR_PROCESS,
    InvalidBase = IBU_ERR_INVALID_BASE, SeqLen = IBU_ERR_SEQ_LEN, InvalidArg = IBU_ERR_INVALID_ARG,
    Hip = IBU_ERR_HIP, NoDevice = IBU_ERR_NO_DEVICE
  };
  IbuError(int32_t code, const ibu_error_detail_t& d)
      : std::runtime_error(std::string(ibu_status_name(code)) + ": " + d.message), code_(code), d_(d) {}
  Kind kind() const { return static_cast<Kind>(code_); }
  const char* name() const { return ibu_status_name(code_); }
  uint64_t expected() const { return d_.a; }  // InvalidMagicNumber / InvalidVersion
  uint64_t actual() const { return d_.b; }
  uint64_t pos() const { return d_.a; }       // TruncatedRecord
  uint64_t idx() const { return d_.a; }       // InvalidIndex
  uint64_t max() const { return d_.b; }
  uint64_t length() const { return d_.a; }    // InvalidBarcodeLength / InvalidUmiLength
  uint64_t first_bad() const { return d_.a; } // InvalidBase
  uint64_t n_bad() const { return d_.b; }
  int os_errno() const { return d_.os_errno; }

 private:
  int32_t code_;
  ibu_error_detail_t d_;
};
inline void check(int32_t rc) {
  if (rc == IBU_OK) return;
  ibu_error_detail_t d;
  ibu_last_error(&d);
  throw IbuError(rc, d);
}

// ---- constructs/record.rs ------------------------------------------------------------------------------------
struct Record : ibu_record_t {
  Record() : ibu_record_t{0, 0, 0} {}                                        // Default
  Record(uint64_t barcode_, uint64_t umi_, uint64_t index_) : ibu_record_t{barcode_, umi_, index_} {}  // new :87-93
  const uint8_t* as_bytes() const { return reinterpret_cast<const uint8_t*>(this); }  // :108-110
  static Record from_bytes(const uint8_t* bytes, size_t len) {               // :130-132 (panics there, throws here)
    Record r;
    check(ibu_record_from_bytes(bytes, len, &r));
    return r;
  }
  int cmp(const Record& o) const { return ibu_record_cmp(this, &o); }        // derive(Ord) :58
  friend bool operator==(const Record& a, const Record& b) { return a.cmp(b) == 0; }
  friend bool operator!=(const Record& a, const Record& b) { return a.cmp(b) != 0; }
  friend bool operator<(const Record& a, const Record& b) { return a.cmp(b) < 0; }
  friend bool operator>(const Record& a, const Record& b) { return a.cmp(b) > 0; }
  friend bool operator<=(const Record& a, const Record& b) { return a.cmp(b) <= 0; }
  friend bool operator>=(const Record& a, const Record& b) { return a.cmp(b) >= 0; }
};
static_assert(sizeof(Record) == RECORD_SIZE, "Record is the 24-byte POD (record.rs:149-152)");

// ---- constructs/header.rs ------------------------------------------------------------------------------------
struct Header : ibu_header_t {
  Header() { std::memset(this, 0, sizeof *this); }
  Header(uint32_t bc_len_, uint32_t umi_len_) { ibu_header_init(this, bc_len_, umi_len_); }  // new :84-93
  void set_sorted() { ibu_header_set_sorted(this); }                         // :111-113
  bool sorted() const { return ibu_header_sorted(this) != 0; }               // :130-132
  void validate() const { check(ibu_header_validate(this)); }                // :167-187
  const uint8_t* as_bytes() const { return reinterpret_cast<const uint8_t*>(this); }  // :203-205
  static Header from_bytes(const uint8_t* bytes, size_t len) {               // :226-228
    Header h;
    check(ibu_header_from_bytes(bytes, len, &h));
    return h;
  }
  friend bool operator==(const Header& a, const Header& b) { return std::memcmp(&a, &b, sizeof a) == 0; }
  friend bool operator!=(const Header& a, const Header& b) { return !(a == b); }
};
static_assert(sizeof(Header) == HEADER_SIZE, "Header is the 32-byte POD (header.rs:248-251)");

struct RecordSlice {  // &[Record]
  const Record* ptr = nullptr;
  size_t len = 0;
  const Record* begin() const { return ptr; }
  const Record* end() const { return ptr + len; }
  size_t size() const { return len; }
  const Record& operator[](size_t i) const { return ptr[i]; }
};

namespace device {
class Context;
}
using StreamStats = ibu_stream_stats_t;
using RingConfig = ibu_ring_config_t;
using ReduceResult = ibu_reduce_result_t;
using DecodeSink = ibu_decode_sink_t;   // {d_bc_ascii, d_umi_ascii, d_index, cap_records}: device columns and the rows they hold
using AllocProbe = ibu_alloc_probe_t;
using NumaInfo = ibu_numa_info_t;
class DeviceStream;

// ---- io/writer.rs ----------------------------------------------------------------------------------------------
class Writer {
 public:
  Writer(std::ostream& inner, const Header& header) { open_stream(&inner, &header); }  // Writer::new :129-143
  static Writer new_headless(std::ostream& inner) { Writer w; w.open_stream(&inner, nullptr); return w; }  // :169-179
  static Writer to_vec(const Header& header) { Writer w; check(ibu_writer_open_mem(&header, &w.w_)); return w; }
  static Writer to_vec_headless() { Writer w; check(ibu_writer_open_mem(nullptr, &w.w_)); return w; }
  static Writer from_path(const std::string& path, const Header& header) {   // :556-559
    Writer w; check(ibu_writer_open_path(path.c_str(), &header, &w.w_)); return w;
  }
  static Writer from_stdout(const Header& header) { Writer w; check(ibu_writer_open_fd(1, &header, &w.w_)); return w; }  // :587-589
  static Writer from_optional_path(const std::optional<std::string>& path, const Header& header) {  // :617-626
    return path ? from_path(*path, header) : from_stdout(header);
  }
  Writer(Writer&& o) noexcept : w_(o.w_), os_(o.os_) { o.w_ = nullptr; rebind(); }
  Writer& operator=(Writer&& o) noexcept { close(); w_ = o.w_; os_ = o.os_; o.w_ = nullptr; rebind(); return *this; }
  Writer(const Writer&) = delete;
  Writer& operator=(const Writer&) = delete;
  ~Writer() { close(); }                                                     // Drop :519-523 (flush, errors swallowed)

  void write_record(const Record& r) { check(ibu_writer_write_record(w_, &r)); }              // :260-273
  void write_batch(const Record* recs, size_t n) { check(ibu_writer_write_batch(w_, recs, n)); }  // :315-318
  void write_batch(const std::vector<Record>& recs) { write_batch(recs.data(), recs.size()); }
  template <class It>
  void write_iter(It first, It last) { for (; first != last; ++first) write_record(*first); }  // :383-391
  void ingest(Writer& other) { check(ibu_writer_ingest(w_, other.w_)); }                       // :477-482
  void finish() { check(ibu_writer_finish(w_)); }                                             // :429-433
  uint64_t records_written() const { return ibu_writer_records_written(w_); }                 // :207-209
  // what the Vec<u8> sink holds right now (tests peek at `writer.inner`)
  std::vector<uint8_t> inner() const {
    const uint8_t* p = nullptr; size_t n = 0;
    check(ibu_writer_mem_view(w_, &p, &n));
    return std::vector<uint8_t>(p, p + n);
  }
  std::vector<uint8_t> into_inner() {                                        // :507-511 — NO flush
    uint8_t* p = nullptr; size_t n = 0;
    ibu_writer_t* w = w_; w_ = nullptr;
    check(ibu_writer_into_inner(w, &p, &n));
    std::vector<uint8_t> v(p, p + n);
    ibu_free(p);
    return v;
  }
  // device-resident AoS records -> pinned ring -> this writer, same buffered/direct rule (writer.rs:321-351)
  // producer_stream: the stream the records were produced on (nullptr: the context's own)
  inline StreamStats write_batch_device(device::Context& ctx, const void* d_records, size_t n, const RingConfig* ring = nullptr,
                                        void* producer_stream = nullptr);
  // n rows of host ASCII (+ optional index column; nullptr -> first_index + i) -> GPU 2-bit encode -> this writer
  // (README.md:38-47's encode-then-write loop as one batch call).  Throws InvalidBase{first_bad, n_bad}.
  inline StreamStats write_ascii_batch(device::Context& ctx, const uint8_t* bc_ascii, const uint8_t* umi_ascii, const uint64_t* index,
                                       size_t n, uint32_t bc_len, uint32_t umi_len, uint64_t first_index = 0,
                                       const RingConfig* ring = nullptr);
  ibu_writer_t* raw() const { return w_; }

 private:
  Writer() = default;
  void open_stream(std::ostream* os, const Header* h) {
    os_ = os;
    check(ibu_writer_open_callback(&Writer::wr, &Writer::fl, os_, h, &w_));
  }
  void rebind() {}  // the callback user pointer is the std::ostream itself, which does not move
  void close() { if (w_) { ibu_writer_close(w_); w_ = nullptr; } }
  static int32_t wr(void* u, const uint8_t* d, size_t n) {
    auto* os = static_cast<std::ostream*>(u);
    os->write(reinterpret_cast<const char*>(d), (std::streamsize)n);
    return os->good() ? 0 : 5 /*EIO*/;
  }
  static int32_t fl(void* u) {
    auto* os = static_cast<std::ostream*>(u);
    os->flush();
    return os->good() ? 0 : 5;
  }
  ibu_writer_t* w_ = nullptr;
  std::ostream* os_ = nullptr;
};

// ---- io/reader.rs ----------------------------------------------------------------------------------------------
class Reader {
 public:
  explicit Reader(std::istream& inner) { check(ibu_reader_open_callback(&Reader::rd, &inner, &r_)); }  // new :152-176
  Reader(const uint8_t* bytes, size_t len) { check(ibu_reader_open_mem(bytes, len, &r_)); }            // new(Cursor<&[u8]>)
  explicit Reader(const std::vector<uint8_t>& bytes) : Reader(bytes.data(), bytes.size()) {}
  static Reader from_path(const std::string& path) { Reader r; check(ibu_reader_open_path(path.c_str(), &r.r_)); return r; }  // :345-352
  static Reader from_stdin() { Reader r; check(ibu_reader_open_fd(0, &r.r_)); return r; }             // :389-396
  static Reader from_optional_path(const std::optional<std::string>& path) { return path ? from_path(*path) : from_stdin(); }  // :425-434
  Reader(Reader&& o) noexcept : r_(o.r_) { o.r_ = nullptr; }
  Reader& operator=(Reader&& o) noexcept { close(); r_ = o.r_; o.r_ = nullptr; return *this; }
  Reader(const Reader&) = delete;
  Reader& operator=(const Reader&) = delete;
  ~Reader() { close(); }

  Header header() const { Header h; check(ibu_reader_header(r_, &h)); return h; }                     // :244-246
  bool read_batch() { int32_t has = 0; check(ibu_reader_read_batch(r_, &has)); return has != 0; }     // :218-242
  std::optional<Record> next() {                                             // Iterator::next :279-306; Some(Err) throws
    Record r; int32_t got = 0;
    check(ibu_reader_next(r_, &r, &got));
    if (!got) return std::nullopt;
    return r;
  }
  uint64_t bytes_read() const { return ibu_reader_bytes_read(r_); }
  std::vector<Record> collect() { std::vector<Record> v; while (auto r = next()) v.push_back(*r); return v; }
  struct iterator {
    Reader* rd; std::optional<Record> cur;
    const Record& operator*() const { return *cur; }
    iterator& operator++() { cur = rd->next(); return *this; }
    bool operator!=(const iterator&) const { return cur.has_value(); }
  };
  iterator begin() { return iterator{this, next()}; }
  iterator end() { return iterator{this, std::nullopt}; }
  // device: stream the rest of this reader (plain or gzip) through the pinned ring
  inline std::pair<ReduceResult, StreamStats> process_device_reduce(device::Context& ctx, const RingConfig* ring = nullptr);
  // sink.cap_records: rows the columns hold; a longer stream throws IbuError (InvalidArg) instead of writing past them.
  // (The sink is ONE argument on purpose: revision 3 had squeezed `size_t cap_records` in front of other defaulted size_t
  // parameters, and a revision-2 positional call still compiled with shifted meanings.  Old calls no longer compile.)
  inline StreamStats process_device_decode(device::Context& ctx, const DecodeSink& sink, const RingConfig* ring = nullptr);
  // pull-style device stream over the rest of this reader: the caller takes one device-resident batch at a time (DeviceStream below)
  inline DeviceStream device_stream(device::Context& ctx, const RingConfig* ring = nullptr);
  ibu_reader_t* raw() const { return r_; }

 private:
  Reader() = default;
  void close() { if (r_) { ibu_reader_close(r_); r_ = nullptr; } }
  static int32_t rd(void* u, uint8_t* dst, size_t cap, size_t* got) {
    auto* is = static_cast<std::istream*>(u);
    is->read(reinterpret_cast<char*>(dst), (std::streamsize)cap);
    *got = (size_t)is->gcount();
    if (is->bad()) return 5;
    if (is->eof()) is->clear(is->rdstate() & ~std::ios::failbit);  // short read at EOF is not an error
    return 0;
  }
  ibu_reader_t* r_ = nullptr;
};

inline std::pair<Header, std::vector<Record>> load_to_vec(const std::string& path) {  // reader.rs:510-535
  Header h; ibu_record_t* p = nullptr; size_t n = 0;
  check(ibu_load_to_vec(path.c_str(), &h, &p, &n));
  std::vector<Record> v(n);
  if (n) std::memcpy(static_cast<void*>(v.data()), p, n * RECORD_SIZE);
  ibu_free(p);
  return {h, std::move(v)};
}

inline std::pair<size_t, size_t> shard_range(size_t len, size_t n_shards, size_t shard) {  // mmap.rs:297-307
  size_t s = 0, e = 0;
  check(ibu_shard_range(len, n_shards, shard, &s, &e));
  return {s, e};
}

// ---- parallel.rs + io/mmap.rs --------------------------------------------------------------------------------
// A processor error: throw ProcessError (or anything) from process_record / on_batch_complete; it reaches the
// caller of process_parallel as IbuError{Process} (first error in handle order wins — mmap.rs:326-328).
struct ProcessError : std::runtime_error {
  int32_t code;
  explicit ProcessError(const std::string& what, int32_t code_ = 1) : std::runtime_error(what), code(code_) {}
};
namespace detail {
template <class P, class = void> struct has_batch : std::false_type {};
template <class P> struct has_batch<P, std::void_t<decltype(std::declval<P&>().on_batch_complete())>> : std::true_type {};
template <class P, class = void> struct has_set_tid : std::false_type {};
template <class P> struct has_set_tid<P, std::void_t<decltype(std::declval<P&>().set_tid(size_t{}))>> : std::true_type {};
template <class F> int32_t guarded(F&& f) {
  try { f(); return 0; }
  catch (const ProcessError& e) { return e.code ? e.code : 1; }
  catch (...) { return 1; }
}
}  // namespace detail

class MmapReader {
 public:
  static constexpr size_t BATCH_SIZE = IBU_BATCH_SIZE;                       // mmap.rs:284
  explicit MmapReader(const std::string& path) { check(ibu_mmap_open(path.c_str(), &m_)); }  // new :143-161
  MmapReader(const MmapReader& o) { check(ibu_mmap_clone(o.m_, &m_)); }      // Clone: shares the map (Arc)
  MmapReader& operator=(const MmapReader& o) { if (this != &o) { close(); check(ibu_mmap_clone(o.m_, &m_)); } return *this; }
  MmapReader(MmapReader&& o) noexcept : m_(o.m_) { o.m_ = nullptr; }
  ~MmapReader() { close(); }
  size_t len() const { return ibu_mmap_len(m_); }                            // :178-180
  Header header() const { Header h; check(ibu_mmap_header(m_, &h)); return h; }  // :201-203
  RecordSlice slice(size_t start, size_t end) const {                        // :253-270
    const ibu_record_t* p = nullptr; size_t n = 0;
    check(ibu_mmap_slice(m_, start, end, &p, &n));
    return RecordSlice{static_cast<const Record*>(p), n};
  }
  const void* map_ptr() const { return ibu_mmap_base(m_); }                  // Arc::ptr_eq analogue (mmap.rs:541)

  // ParallelReader::process_parallel :286-332.  P: copyable (Clone), process_record(const Record&) [,
  // on_batch_complete(), set_tid(size_t)].  num_threads 0 = all cores.
  template <class P>
  void process_parallel(const P& processor, size_t num_threads) const {
    ibu_processor_vtable_t vt{};
    vt.clone = [](void* u) -> void* { return new P(*static_cast<const P*>(u)); };
    vt.drop = [](void* c) { delete static_cast<P*>(c); };
    vt.process_record = [](void* c, const ibu_record_t* r) -> int32_t {
      return detail::guarded([&] { static_cast<P*>(c)->process_record(*static_cast<const Record*>(r)); });
    };
    if constexpr (detail::has_batch<P>::value)
      vt.on_batch_complete = [](void* c) -> int32_t { return detail::guarded([&] { static_cast<P*>(c)->on_batch_complete(); }); };
    if constexpr (detail::has_set_tid<P>::value)
      vt.set_tid = [](void* c, size_t tid) { static_cast<P*>(c)->set_tid(tid); };
    check(ibu_mmap_process_parallel(m_, &vt, const_cast<P*>(&processor), num_threads));
  }
  // device: ONE shard of the same static split per GPU / rank
  inline std::pair<ReduceResult, StreamStats> process_device_reduce(device::Context& ctx, size_t shard = 0, size_t n_shards = 1,
                                                                     const RingConfig* ring = nullptr) const;
  inline StreamStats process_device_decode(device::Context& ctx, const DecodeSink& sink, size_t shard = 0, size_t n_shards = 1,
                                           const RingConfig* ring = nullptr) const;
  // process_parallel(processor, n) with a GPU per worker, ONE call (mmap.rs:286-332): worker i = a host thread + a context on
  // devices[i], shard i of the static split; an empty list = every visible device (num_threads == 0 = every core).  The
  // reduce form returns the total (wrapping sums, XORs) and the per-device partials; the decode form fills sinks[i] on devices[i].
  inline std::pair<ReduceResult, std::vector<ReduceResult>> process_devices_reduce(const std::vector<int32_t>& devices = {},
                                                                                   const RingConfig* ring = nullptr) const;
  inline void process_devices_decode(const std::vector<int32_t>& devices, std::vector<DecodeSink>& sinks, const RingConfig* ring = nullptr) const;
  // one shard -> ASCII barcodes / UMIs + index column in HOST memory, unpacked on the GPU
  struct Decoded { std::vector<uint8_t> bc, umi; std::vector<uint64_t> index; StreamStats stats; };
  inline Decoded decode_to_host(device::Context& ctx, size_t shard = 0, size_t n_shards = 1, const RingConfig* ring = nullptr) const;
  // pull-style device stream over one shard of the static split (DeviceStream below)
  inline DeviceStream device_stream(device::Context& ctx, size_t shard = 0, size_t n_shards = 1, const RingConfig* ring = nullptr) const;
  ibu_mmap_t* raw() const { return m_; }

 private:
  void close() { if (m_) { ibu_mmap_close(m_); m_ = nullptr; } }
  ibu_mmap_t* m_ = nullptr;
};

// ---- device path (no reference equivalent: the MI355X side of the boundary) --------------------------------
namespace device {
class Whitelist;
using CorrectCounts = ibu_correct_counts_t;
class Abundance;
class Labels;
using ResolveCounts = ibu_resolve_counts_t;
using MoleculeCounts = ibu_molecule_counts_t;
using CellCounts = ibu_cell_counts_t;
using SaturationPoint = ibu_saturation_point_t;
using BarcodeLimits = ibu_barcode_limits_t;
using BarcodeFilterCounts = ibu_barcode_filter_counts_t;
using FeatureLimits = ibu_feature_limits_t;
using FeatureFilterCounts = ibu_feature_filter_counts_t;
using AssignRule = ibu_assign_rule_t;       // ibu_assign_rows: {min_value, num, den}
using AssignCounts = ibu_assign_counts_t;
// the five per-row columns of ibu_matrix_row_top, device arrays of one u64 per row, each nullable
struct RowTopColumns { uint64_t* top_key; uint64_t* top_value; uint64_t* next_value; uint64_t* row_sum; uint64_t* row_entries; };
// the totals of one ibu_feature_metrics call: reads, umis and cells of the features below n_features, and the records that are not
struct FeatureTotals { uint64_t reads, umis, cells, reads_out_of_range; };
// one row of ibu_barcode_metrics: a barcode, its records, the (w0, w1) pairs and (w0, w1, w2) triples that begin in it, and its
// records / triples in the feature set
struct BarcodeMetrics { uint64_t barcode, reads, pairs, triples, set_reads, set_triples; };
// a feature set of ibu_barcode_metrics / ibu_filter_barcodes: a device bitmap of `bits` bits (nullptr and 0: the empty set)
struct FeatureSet { const uint64_t* d_bits = nullptr; uint64_t bits = 0; };
// one entry of ibu_pair_counts / ibu_count_matrix: (barcode, index, reads, distinct UMIs) on the count-matrix path
struct MatrixEntry { uint64_t first, second, records, distinct; };
inline int device_count() { int32_t n = 0; return ibu_device_count(&n) == IBU_OK ? n : 0; }

class Context {
 public:
  explicit Context(int device = 0) { check(ibu_ctx_create(device, &c_)); }   // throws NoDevice without a gfx950 GPU
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  ~Context() { if (c_) ibu_ctx_destroy(c_); }
  ibu_ctx_t* raw() const { return c_; }
  void synchronize(void* stream = nullptr) { check(ibu_ctx_synchronize(c_, stream)); }
  void set_option(const char* key, int64_t v) { check(ibu_ctx_set_option(c_, key, v)); }

  void decode_ascii(const void* d_recs, size_t n, const Header& h, uint8_t* d_bc, uint8_t* d_umi, uint64_t* d_idx, void* st = nullptr) {
    check(ibu_decode_ascii(c_, d_recs, n, h.bc_len, h.umi_len, d_bc, d_umi, d_idx, st));
  }
  void encode_ascii(const uint8_t* d_bc, const uint8_t* d_umi, const uint64_t* d_idx, size_t n, const Header& h, void* d_recs,
                    uint64_t first_index = 0, void* st = nullptr) {
    check(ibu_encode_ascii(c_, d_bc, d_umi, d_idx, first_index, n, h.bc_len, h.umi_len, d_recs, st));
  }
  void codec_status(void* st = nullptr) { check(ibu_codec_status(c_, st, nullptr, nullptr)); }  // throws InvalidBase
  void deserialize(const void* d_recs, size_t n, uint64_t* bc, uint64_t* umi, uint64_t* idx, void* st = nullptr) {
    check(ibu_deserialize(c_, d_recs, n, bc, umi, idx, st));
  }
  void serialize(const uint64_t* bc, const uint64_t* umi, const uint64_t* idx, size_t n, void* d_recs, void* st = nullptr) {
    check(ibu_serialize(c_, bc, umi, idx, n, d_recs, st));
  }
  void unpack_2bit(const uint64_t* codes, size_t n, uint32_t len, uint8_t* ascii, void* st = nullptr) { check(ibu_unpack_2bit(c_, codes, n, len, ascii, st)); }
  void pack_2bit(const uint8_t* ascii, size_t n, uint32_t len, uint64_t* codes, void* st = nullptr) { check(ibu_pack_2bit(c_, ascii, n, len, codes, st)); }
  ReduceResult reduce(const void* d_recs, size_t n, void* st = nullptr) {
    ReduceResult r;
    check(ibu_reduce_reset(c_, st));
    check(ibu_reduce(c_, d_recs, n, st));
    check(ibu_reduce_fetch(c_, st, &r));
    return r;
  }
  void generate(uint64_t seed, uint64_t first, size_t n, const Header& h, void* d_recs, void* st = nullptr) {
    check(ibu_generate(c_, seed, first, n, h.bc_len, h.umi_len, d_recs, st));
  }
  void copy(void* d_dst, const void* d_src, size_t bytes, void* st = nullptr) { check(ibu_device_copy(c_, d_dst, d_src, bytes, st)); }
  void sort_records(void* d_recs, void* d_tmp, size_t n, void* st = nullptr) { check(ibu_sort_records(c_, d_recs, d_tmp, n, st)); }
  // the stable merge of two sorted record arrays into d_out (equal records: those of d_a first); d_source (nullable): one byte per
  // output record, 0 = from d_a, 1 = from d_b (ibu_merge_sorted).  Asynchronous.
  void merge_sorted(const void* d_a, size_t na, const void* d_b, size_t nb, void* d_out, uint8_t* d_source = nullptr, void* st = nullptr) {
    check(ibu_merge_sorted(c_, d_a, na, d_b, nb, d_out, d_source, st));
  }
  // d_recs = consecutive sorted runs of these lengths -> all of them sorted, what sort_records gives (ibu_merge_sorted_runs)
  void merge_sorted_runs(void* d_recs, void* d_tmp, const std::vector<size_t>& run_lengths, void* st = nullptr) {
    check(ibu_merge_sorted_runs(c_, d_recs, d_tmp, run_lengths.data(), run_lengths.size(), st));
  }
  // the sort over several shards, one per context (= per GPU), in one call: shard i ends up with the i-th range of the global
  // order and shards[i].n says how long it is (ibu_sort_records_contexts)
  static void sort_records_contexts(const std::vector<Context*>& ctxs, std::vector<ibu_sort_shard_t>& shards) {
    if (shards.size() != ctxs.size()) {                        // the C side reads n_ctxs entries of both arrays
      ibu_error_detail_t d{};
      d.code = IBU_ERR_INVALID_ARG;
      snprintf(d.message, sizeof d.message, "Invalid argument: one shard per context");
      throw IbuError(IBU_ERR_INVALID_ARG, d);
    }
    std::vector<ibu_ctx_t*> raw;
    for (Context* c : ctxs) raw.push_back(c->c_);
    check(ibu_sort_records_contexts(raw.data(), raw.size(), shards.data()));
  }
  void lower_bound(const void* d_sorted, size_t n, const void* d_keys, size_t k, uint64_t* d_pos, void* st = nullptr) { check(ibu_lower_bound_records(c_, d_sorted, n, d_keys, k, d_pos, st)); }
  // index of the first record that differs, n if the slices are equal (Record: PartialEq, record.rs:58)
  size_t first_mismatch(const void* d_a, const void* d_b, size_t n, void* st = nullptr) { uint64_t f = 0; check(ibu_records_first_mismatch(c_, d_a, d_b, n, &f, st)); return (size_t)f; }
  bool is_sorted(const void* d_recs, size_t n, void* st = nullptr) { int32_t s = 0; check(ibu_is_sorted(c_, d_recs, n, st, &s)); return s != 0; }
  // compacted keys (the exchange format of the multi-GPU sort): OR / AND census, plan, records <-> 12-byte elements
  std::array<uint64_t, 8> census(const void* d_recs, size_t n, void* st = nullptr) { std::array<uint64_t, 8> c{}; check(ibu_records_census(c_, d_recs, n, c.data(), st)); return c; }
  static ibu_key_plan_t key_plan(const uint64_t or_words[3], const uint64_t and_words[3]) { ibu_key_plan_t p; check(ibu_key_plan_init(or_words, and_words, &p)); return p; }
  void compact(const ibu_key_plan_t& plan, const void* d_recs, size_t n, void* d_elems, void* st = nullptr) { check(ibu_records_compact(c_, &plan, d_recs, n, d_elems, st)); }
  void expand(const ibu_key_plan_t& plan, const void* d_elems, size_t n, void* d_recs, void* st = nullptr) { check(ibu_records_expand(c_, &plan, d_elems, n, d_recs, st)); }
  // BarcodeAnalyzer (parallel.rs:72-98) on sorted device records: (barcode, records, distinct UMIs), ascending barcode
  inline std::vector<std::tuple<uint64_t, uint64_t, uint64_t>> barcode_counts(const void* d_sorted, size_t n);
  // count matrix.  swap_umi_index: record i of d_dst = {barcode, index, umi} of record i of d_src; d_dst == d_src is in place.
  void swap_umi_index(const void* d_src, void* d_dst, size_t n, void* st = nullptr) { check(ibu_records_swap_umi_index(c_, d_src, d_dst, n, st)); }
  // one entry per run of equal (first word, second word): (first, second, records, distinct third words), in input order (ibu_pair_counts)
  inline std::vector<MatrixEntry> pair_counts(const void* d_sorted, size_t n);
  // the count matrix of n records in any order: (barcode, index, reads, umis) ascending by (barcode, index); the records come back
  // ordered by (barcode, index, umi), with the umi and index words exchanged if leave_swapped (ibu_count_matrix).  cap: a bound on
  // the number of entries, 0 = n (always fits)
  inline std::vector<MatrixEntry> count_matrix(void* d_recs, void* d_tmp, size_t n, size_t cap = 0, bool leave_swapped = false);
  // barcode correction against a whitelist, in place (ibu_correct_barcodes): d_class (nullable) receives one class byte per record;
  // returns the four totals (synchronises).  correct_barcodes_async: no totals, nothing synchronised.
  inline CorrectCounts correct_barcodes(const Whitelist& wl, void* d_recs, size_t n, uint32_t max_mismatches = 1, uint8_t* d_class = nullptr,
                                        void* st = nullptr);
  inline void correct_barcodes_async(const Whitelist& wl, void* d_recs, size_t n, uint32_t max_mismatches = 1, uint8_t* d_class = nullptr,
                                     void* st = nullptr);
  // ambiguous barcodes (class 2 of correct_barcodes) to the candidate that holds at least num / den of the reads `ab` counted for the
  // candidates, in place over records and class bytes (ibu_resolve_barcodes): a resolved record gets class IBU_BARCODE_RESOLVED;
  // returns the four totals (synchronises).  resolve_barcodes_async: no totals, nothing synchronised.
  // select_records(.., 0b10011, ..) then keeps exact, corrected and resolved records
  inline ResolveCounts resolve_barcodes(const Whitelist& wl, const Abundance& ab, void* d_recs, size_t n, uint8_t* d_class, uint64_t num = 39,
                                        uint64_t den = 40, void* st = nullptr);
  inline void resolve_barcodes_async(const Whitelist& wl, const Abundance& ab, void* d_recs, size_t n, uint8_t* d_class, uint64_t num = 39,
                                     uint64_t den = 40, void* st = nullptr);
  // per-barcode labels onto records (ibu_label_records): a record is found when its barcode is an entry of the whitelist `lb` belongs
  // to.  Plain mode: d_class[i] = the entry's label, or missing_class where not found.  label_records_match: IBU_LABEL_IS / _OTHER /
  // _MISSING against `match`, so that select_records(.., 1u << IBU_LABEL_IS, ..) extracts one of up to 256 labels.  d_class (n bytes)
  // and hist (host, uint64_t[IBU_LABEL_BINS]: reads per label, then the reads not found) are each nullable; a non-null hist synchronises
  inline void label_records(const Labels& lb, const void* d_recs, size_t n, uint8_t* d_class, uint64_t* hist = nullptr, uint32_t missing_class = 255,
                            void* st = nullptr);
  inline void label_records_match(const Labels& lb, const void* d_recs, size_t n, uint32_t match, uint8_t* d_class, uint64_t* hist = nullptr,
                                  void* st = nullptr);
  // one index per (barcode, umi) molecule of sorted records (ibu_classify_molecules): d_class (n bytes, or nullptr for the totals
  // only) gets IBU_MOLECULE_KEPT / _MINOR / _TIED per record; select_records(.., 1u << IBU_MOLECULE_KEPT, ..) drops the chimeric reads
  MoleculeCounts classify_molecules(const void* d_sorted, size_t n, uint8_t* d_class, bool tie_first = false, void* st = nullptr) {
    MoleculeCounts c{};
    check(ibu_classify_molecules(c_, d_sorted, n, tie_first ? IBU_MOLECULES_TIE_FIRST : 0u, d_class, &c, st));
    return c;
  }
  // which barcodes of sorted records are cells (ibu_call_cells): mode IBU_CELLS_MIN / _TOP / _ORDMAG with its parameter, flags 0 or
  // IBU_CELLS_BY_READS; d_class (n bytes, or nullptr for the totals only) gets IBU_CELL / IBU_CELL_BACKGROUND per record;
  // select_records(.., 1u << IBU_CELL, ..) keeps the records of the cells
  CellCounts call_cells(const void* d_sorted, size_t n, uint32_t mode, uint64_t param, uint8_t* d_class, uint32_t flags = 0, void* st = nullptr) {
    CellCounts c{};
    check(ibu_call_cells(c_, d_sorted, n, mode, param, flags, d_class, &c, st));
    return c;
  }
  // the per-barcode QC table (ibu_barcode_metrics): one row per run of equal first word, in input order; set_word (1 or 2) is the
  // record word looked up in `set`.  On swapped-and-sorted records with set_word = 1: pairs = features detected, triples = UMIs
  inline std::vector<BarcodeMetrics> barcode_metrics(const void* d_recs, size_t n, const FeatureSet& set = {}, uint32_t set_word = 1);
  // the QC filter made from that table (ibu_filter_barcodes): d_class (n bytes, or nullptr for the totals only) gets the class of
  // the record's barcode — IBU_BARCODE_PASS / _LOW / _HIGH / _SET; a zeroed BarcodeLimits passes everything;
  // select_records(.., 1u << IBU_BARCODE_PASS, ..) keeps the passing barcodes
  BarcodeFilterCounts filter_barcodes(const void* d_recs, size_t n, const FeatureSet& set, uint32_t set_word, const BarcodeLimits& limits,
                                      uint8_t* d_class, void* st = nullptr) {
    BarcodeFilterCounts c{};
    check(ibu_filter_barcodes(c_, d_recs, n, set.d_bits, set.bits, set_word, &limits, d_class, &c, st));
    return c;
  }
  // the per-feature columns (ibu_feature_metrics): for every feature f < n_features (the value of a record's word feature_word, 1
  // or 2) its reads, its triples (UMIs) and, with feature_word = 1, its pairs (cells) — device columns of n_features u64, each
  // nullable, zeroed by the call unless flags has IBU_FEATURE_ACCUMULATE; d_cells must be nullptr with feature_word = 2.
  // Synchronises once, for the totals
  FeatureTotals feature_metrics(const void* d_recs, size_t n, uint64_t n_features, uint64_t* d_reads, uint64_t* d_umis, uint64_t* d_cells,
                                uint32_t feature_word = 1, uint32_t flags = 0, void* st = nullptr) {
    uint64_t t[4] = {0, 0, 0, 0};
    check(ibu_feature_metrics(c_, d_recs, n, feature_word, n_features, flags, d_reads, d_umis, d_cells, t, st));
    return FeatureTotals{t[0], t[1], t[2], t[3]};
  }
  // the feature filter made from those columns (ibu_filter_features), which may come from other records than the ones classed:
  // d_class (n bytes, or nullptr for the totals only) gets the verdict of the record's feature — IBU_FEATURE_PASS / _LOW / _HIGH,
  // and IBU_FEATURE_UNKNOWN where it is not below n_features; d_verdict (n_features bytes, nullable) the verdicts themselves;
  // select_records(.., 1u << IBU_FEATURE_PASS, ..) keeps the records of the kept features
  FeatureFilterCounts filter_features(const void* d_recs, size_t n, uint64_t n_features, const uint64_t* d_reads, const uint64_t* d_umis,
                                      const uint64_t* d_cells, const FeatureLimits& limits, uint8_t* d_class, uint8_t* d_verdict = nullptr,
                                      uint32_t feature_word = 1, void* st = nullptr) {
    FeatureFilterCounts c{};
    check(ibu_filter_features(c_, d_recs, n, feature_word, n_features, d_reads, d_umis, d_cells, &limits, d_class, d_verdict, &c, st));
    return c;
  }
  // the row structure of a column of the entry table (ibu_matrix_rows): a row is a maximal run of equal d_first[k].  Each output is
  // nullable: d_row_of_entry (n_entries words) the 0-based row of every entry, d_row_keys (cap words) the value of every row,
  // d_row_ptr (cap + 1 words) the CSR indptr.  All three nullptr and cap = 0: the size query.  Returns the number of rows
  // (synchronises once, for it)
  size_t matrix_rows(const uint64_t* d_first, size_t n_entries, uint64_t* d_row_of_entry, uint64_t* d_row_keys, uint64_t* d_row_ptr, size_t cap,
                     void* st = nullptr) {
    size_t rows = 0;
    check(ibu_matrix_rows(c_, d_first, n_entries, d_row_of_entry, d_row_keys, d_row_ptr, cap, &rows, st));
    return rows;
  }
  // three u64 columns as decimal text (ibu_matrix_market_body): line k = d_a[k] + add_a, d_b[k] + add_b, d_c[k], separated by blanks
  // and ended by '\n'.  d_text (any alignment) holds cap_bytes; nullptr and 0: the size query.  Returns the bytes of the text;
  // maxima (nullable) receives the largest printed value of each column.  Synchronises once, for both
  size_t matrix_market_body(const uint64_t* d_a, const uint64_t* d_b, const uint64_t* d_c, size_t n_entries, char* d_text, size_t cap_bytes,
                            uint64_t add_a = 1, uint64_t add_b = 1, uint64_t maxima[3] = nullptr, void* st = nullptr) {
    size_t bytes = 0;
    check(ibu_matrix_market_body(c_, d_a, d_b, d_c, n_entries, add_a, add_b, d_text, cap_bytes, &bytes, maxima, st));
    return bytes;
  }
  // the dominant entry of every row of the entry table (ibu_matrix_row_top): per row — a maximal run of equal d_first[k] — the largest
  // d_values[k], the d_second[k] of the first entry that holds it, the largest value among the other entries, the sum modulo 2^64 and
  // the number of entries, over the entries whose d_second[k] is in the bitmap d_set of set_bits bits (nullptr and 0: all entries).
  // A row in which nothing takes part gets IBU_NO_KEY, 0, 0, 0, 0.  All five columns nullptr: the size query.  Returns the number of
  // rows (synchronises once, for it)
  size_t matrix_row_top(const uint64_t* d_first, const uint64_t* d_second, const uint64_t* d_values, size_t n_entries, const RowTopColumns& out,
                        size_t cap, const uint64_t* d_set = nullptr, uint64_t set_bits = 0, void* st = nullptr) {
    size_t rows = 0;
    check(ibu_matrix_row_top(c_, d_first, d_second, d_values, n_entries, d_set, set_bits, out.top_key, out.top_value, out.next_value, out.row_sum,
                             out.row_entries, cap, &rows, st));
    return rows;
  }
  // the class of every row from three of those columns (ibu_assign_rows): IBU_ROW_NONE where the top is below max(rule.min_value, 1),
  // else IBU_ROW_ASSIGNED where it is above the runner-up and top * den >= num * sum (exact; num = 0: no share test), else
  // IBU_ROW_MIXED.  d_row_class: n_rows bytes, or nullptr for the totals only.  Synchronises, for the totals; assign_rows_async: no
  // totals, nothing synchronised
  AssignCounts assign_rows(const uint64_t* d_top_value, const uint64_t* d_next_value, const uint64_t* d_row_sum, size_t n_rows,
                           const AssignRule& rule, uint8_t* d_row_class, void* st = nullptr) {
    AssignCounts c{};
    check(ibu_assign_rows(c_, d_top_value, d_next_value, d_row_sum, n_rows, &rule, d_row_class, &c, st));
    return c;
  }
  void assign_rows_async(const uint64_t* d_top_value, const uint64_t* d_next_value, const uint64_t* d_row_sum, size_t n_rows, const AssignRule& rule,
                         uint8_t* d_row_class, void* st = nullptr) {
    check(ibu_assign_rows(c_, d_top_value, d_next_value, d_row_sum, n_rows, &rule, d_row_class, nullptr, st));
  }
  // a reproducible random subset of n rows (ibu_subsample_class): d_class (n bytes, or nullptr for the count only) gets
  // IBU_SAMPLE_KEPT where the row's number splitmix64(splitmix64(seed) + first_row + row) is below `threshold` (all ones keeps every
  // row) and IBU_SAMPLE_DROPPED elsewhere; no record is read.  Returns the number kept (synchronises).  subsample_class_async: no
  // count, nothing synchronised.  select_records(.., 1u << IBU_SAMPLE_KEPT, ..) then makes the subset
  size_t subsample_class(size_t n, uint64_t threshold, uint8_t* d_class, uint64_t seed = 0, uint64_t first_row = 0, void* st = nullptr) {
    size_t k = 0;
    check(ibu_subsample_class(c_, n, first_row, seed, threshold, d_class, &k, st));
    return k;
  }
  void subsample_class_async(size_t n, uint64_t threshold, uint8_t* d_class, uint64_t seed = 0, uint64_t first_row = 0, void* st = nullptr) {
    check(ibu_subsample_class(c_, n, first_row, seed, threshold, d_class, nullptr, st));
  }
  // the threshold that keeps `fraction` of the reads: all ones from 1 on, otherwise the floor of fraction * 2^64 (exact: a double
  // below 1 times 2^64 is a whole number below 2^64)
  static uint64_t sample_threshold(double fraction) {
    if (!(fraction >= 0)) {
      ibu_error_detail_t d{};
      d.code = IBU_ERR_INVALID_ARG;
      snprintf(d.message, sizeof d.message, "Invalid argument: the fraction must be a number >= 0");
      throw IbuError(IBU_ERR_INVALID_ARG, d);
    }
    return fraction >= 1 ? UINT64_MAX : (uint64_t)std::ldexp(fraction, 64);
  }
  // what would have been seen at each of 1 .. 32 non-decreasing thresholds, from one read of the sorted records
  // (ibu_saturation_curve): per point the kept reads and the barcodes / (barcode, umi) molecules with a kept read
  std::vector<SaturationPoint> saturation_curve(const void* d_sorted, size_t n, const std::vector<uint64_t>& thresholds, uint64_t seed = 0,
                                                uint64_t first_row = 0, void* st = nullptr) {
    std::vector<SaturationPoint> points(thresholds.size());
    check(ibu_saturation_curve(c_, d_sorted, n, first_row, seed, thresholds.data(), (uint32_t)(thresholds.size() > 0xFFFFFFFFu ? 0xFFFFFFFFu : thresholds.size()),
                               points.data(), st));
    return points;
  }
  // stable compaction by class (ibu_select_records) -> how many records went to d_out (capacity `cap` records); d_out == nullptr
  // and cap == 0: only count
  size_t select_records(const void* d_recs, const uint8_t* d_class, size_t n, uint32_t keep_mask, void* d_out, size_t cap, void* st = nullptr) {
    size_t k = 0;
    check(ibu_select_records(c_, d_recs, d_class, n, keep_mask, d_out, cap, &k, st));
    return k;
  }
  // stable multi-way partition by class byte in one pass (ibu_partition_records): part_of (host, 256 bytes, or nullptr for the identity
  // below n_parts) gives the part of every class byte, IBU_PART_NONE drops; d_out receives part 0, then part 1, ..., each in input
  // order -> the n_parts + 1 offsets (part p is records offsets[p] .. offsets[p + 1] of d_out).  d_out == nullptr and cap == 0: only count
  std::vector<uint64_t> partition_records(const void* d_recs, const uint8_t* d_class, size_t n, const uint8_t* part_of, uint32_t n_parts, void* d_out,
                                          size_t cap, void* st = nullptr) {
    std::vector<uint64_t> offsets((n_parts < 255 ? n_parts : 255) + 1, 0);
    check(ibu_partition_records(c_, d_recs, d_class, n, part_of, n_parts, d_out, cap, offsets.data(), st));
    return offsets;
  }
  // load_to_vec, device form -> (header, device pointer owned by the caller: release with free(), n)
  std::tuple<Header, void*, size_t> load_to_device(const std::string& path, const RingConfig* ring = nullptr, StreamStats* stats = nullptr) {
    Header h; void* p = nullptr; size_t n = 0;
    check(ibu_load_to_device(c_, path.c_str(), ring, &h, &p, 0, &n, stats));
    return {h, p, n};
  }
  // The same for a BGZF (bgzip) file of the records, inflated on the device: the compressed bytes cross the link.
  std::tuple<Header, void*, size_t> load_bgzf_to_device(const std::string& path, const RingConfig* ring = nullptr, StreamStats* stats = nullptr) {
    Header h; void* p = nullptr; size_t n = 0;
    check(ibu_load_bgzf_to_device(c_, path.c_str(), ring, &h, &p, 0, &n, stats));
    return {h, p, n};
  }
  // ... shard `shard` of `n_shards` of its records (the split of process_parallel) -> (header, device pointer, n, first record's number)
  std::tuple<Header, void*, size_t, uint64_t> load_bgzf_shard_to_device(const std::string& path, size_t shard, size_t n_shards,
                                                                        const RingConfig* ring = nullptr, StreamStats* stats = nullptr) {
    Header h; void* p = nullptr; size_t n = 0; uint64_t first = 0;
    check(ibu_load_bgzf_shard_to_device(c_, path.c_str(), ring, shard, n_shards, &h, &p, 0, &n, &first, stats));
    return {h, p, n, first};
  }
  void* alloc(size_t bytes) { void* p = nullptr; check(ibu_device_alloc(c_, bytes, &p)); return p; }
  // for arrays that stay resident: up to `tries` candidates, the one that streams fastest is kept (ibu_device_alloc_probed)
  void* alloc_probed(size_t bytes, uint32_t tries, AllocProbe* report = nullptr) {
    void* p = nullptr; check(ibu_device_alloc_probed(c_, bytes, tries, &p, report)); return p;
  }
  void free(void* p) { check(ibu_device_free(c_, p)); }
  // where the device hangs off the host and where the pinned ring landed (option "numa")
  NumaInfo numa() const { NumaInfo i; check(ibu_ctx_numa(c_, &i)); return i; }
  void upload(void* d_dst, const void* h_src, size_t bytes) { check(ibu_memcpy_h2d(c_, d_dst, h_src, bytes, nullptr)); synchronize(); }
  void download(void* h_dst, const void* d_src, size_t bytes) { check(ibu_memcpy_d2h(c_, h_dst, d_src, bytes, nullptr)); synchronize(); }

 private:
  ibu_ctx_t* c_ = nullptr;
};

class DeviceBuffer {  // RAII hipMalloc through the context
 public:
  DeviceBuffer(Context& ctx, size_t bytes) : ctx_(&ctx), bytes_(bytes), p_(ctx.alloc(bytes ? bytes : 16)) {}
  DeviceBuffer(DeviceBuffer&& o) noexcept : ctx_(o.ctx_), bytes_(o.bytes_), p_(o.p_) { o.p_ = nullptr; }
  DeviceBuffer(const DeviceBuffer&) = delete;
  ~DeviceBuffer() { if (p_) ibu_device_free(ctx_->raw(), p_); }
  void* ptr() const { return p_; }
  template <class T> T* as() const { return static_cast<T*>(p_); }
  size_t bytes() const { return bytes_; }
  template <class T> void upload(const std::vector<T>& v) { ctx_->upload(p_, v.data(), v.size() * sizeof(T)); }
  template <class T> std::vector<T> download(size_t count) const { std::vector<T> v(count); if (count) ctx_->download(static_cast<void*>(v.data()), p_, count * sizeof(T)); return v; }

 private:
  Context* ctx_;
  size_t bytes_;
  void* p_;
};

// The device lookup table of a barcode whitelist (ibu_whitelist_t), built from w 2-bit codes in device memory.  Destroy it before
// its context.
class Whitelist {
 public:
  Whitelist(Context& ctx, const uint64_t* d_codes, size_t w, uint32_t bc_len, void* st = nullptr) {
    check(ibu_whitelist_create(ctx.raw(), d_codes, w, bc_len, st, &w_));
  }
  Whitelist(Whitelist&& o) noexcept : w_(o.w_) { o.w_ = nullptr; }
  Whitelist(const Whitelist&) = delete;
  Whitelist& operator=(const Whitelist&) = delete;
  ~Whitelist() { if (w_) ibu_whitelist_destroy(w_); }
  const ibu_whitelist_t* raw() const { return w_; }
  uint32_t bc_len() const { uint32_t b = 0; check(ibu_whitelist_info(w_, &b, nullptr, nullptr)); return b; }
  size_t n_distinct() const { size_t n = 0; check(ibu_whitelist_info(w_, nullptr, &n, nullptr)); return n; }
  size_t device_bytes() const { size_t n = 0; check(ibu_whitelist_info(w_, nullptr, nullptr, &n)); return n; }

 private:
  ibu_whitelist_t* w_ = nullptr;
};
// One read counter per entry of a whitelist (ibu_abundance_t), all zero at first.  Destroy it before its whitelist.
class Abundance {
 public:
  Abundance(Context& ctx, const Whitelist& wl, void* st = nullptr) : ctx_(ctx.raw()) { check(ibu_abundance_create(ctx_, wl.raw(), st, &a_)); }
  Abundance(Abundance&& o) noexcept : ctx_(o.ctx_), a_(o.a_) { o.a_ = nullptr; }
  Abundance(const Abundance&) = delete;
  Abundance& operator=(const Abundance&) = delete;
  ~Abundance() { if (a_) ibu_abundance_destroy(a_); }
  const ibu_abundance_t* raw() const { return a_; }
  // counts the records whose barcode is in the whitelist (ibu_abundance_add): all of them with d_class == nullptr, else those whose
  // class c < 8 has bit c of class_mask set.  Asynchronous; accumulates over calls
  void add(const void* d_recs, size_t n, const uint8_t* d_class = nullptr, uint32_t class_mask = 1, void* st = nullptr) {
    check(ibu_abundance_add(ctx_, a_, d_recs, d_class, n, class_mask, st));
  }
  // d_counts[j] = the counter of d_codes[j], 0 for a code that is not in the whitelist (ibu_abundance_counts); asynchronous
  void counts(const uint64_t* d_codes, size_t k, uint64_t* d_counts, void* st = nullptr) const {
    check(ibu_abundance_counts(ctx_, a_, d_codes, k, d_counts, st));
  }
  void reset(void* st = nullptr) { check(ibu_abundance_reset(a_, st)); }
  size_t device_bytes() const { size_t n = 0; check(ibu_abundance_info(a_, &n)); return n; }

 private:
  ibu_ctx_t* ctx_ = nullptr;
  ibu_abundance_t* a_ = nullptr;
};
// One label byte per entry of a whitelist (ibu_labels_t), all `fill` at first.  Destroy it before its whitelist.
class Labels {
 public:
  Labels(Context& ctx, const Whitelist& wl, uint32_t fill = 255, void* st = nullptr) : ctx_(ctx.raw()) {
    check(ibu_labels_create(ctx_, wl.raw(), fill, st, &l_));
  }
  Labels(Labels&& o) noexcept : ctx_(o.ctx_), l_(o.l_) { o.l_ = nullptr; }
  Labels(const Labels&) = delete;
  Labels& operator=(const Labels&) = delete;
  ~Labels() { if (l_) ibu_labels_destroy(l_); }
  const ibu_labels_t* raw() const { return l_; }
  // the label of d_codes[j] becomes d_labels[j] (ibu_labels_set; device arrays); returns the number of codes skipped — not in the
  // whitelist, or with bits at or above 2*bc_len (synchronises).  set_async: no count, nothing synchronised
  size_t set(const uint64_t* d_codes, const uint8_t* d_labels, size_t k, void* st = nullptr) {
    size_t skipped = 0;
    check(ibu_labels_set(ctx_, l_, d_codes, d_labels, k, &skipped, st));
    return skipped;
  }
  void set_async(const uint64_t* d_codes, const uint8_t* d_labels, size_t k, void* st = nullptr) {
    check(ibu_labels_set(ctx_, l_, d_codes, d_labels, k, nullptr, st));
  }
  // d_labels_out[j] = the label of d_codes[j], `missing` for a code that is not an entry (ibu_labels_get); asynchronous
  void get(const uint64_t* d_codes, size_t k, uint8_t* d_labels_out, uint32_t missing = 255, void* st = nullptr) const {
    check(ibu_labels_get(ctx_, l_, d_codes, k, missing, d_labels_out, st));
  }
  size_t device_bytes() const { size_t n = 0; check(ibu_labels_info(l_, &n)); return n; }

 private:
  ibu_ctx_t* ctx_ = nullptr;
  ibu_labels_t* l_ = nullptr;
};
inline void Context::label_records(const Labels& lb, const void* d_recs, size_t n, uint8_t* d_class, uint64_t* hist, uint32_t missing_class, void* st) {
  check(ibu_label_records(c_, lb.raw(), d_recs, n, 0, 0, missing_class, d_class, hist, st));
}
inline void Context::label_records_match(const Labels& lb, const void* d_recs, size_t n, uint32_t match, uint8_t* d_class, uint64_t* hist, void* st) {
  check(ibu_label_records(c_, lb.raw(), d_recs, n, IBU_LABEL_MATCH, match, 255, d_class, hist, st));
}
inline ResolveCounts Context::resolve_barcodes(const Whitelist& wl, const Abundance& ab, void* d_recs, size_t n, uint8_t* d_class, uint64_t num,
                                               uint64_t den, void* st) {
  ResolveCounts c{};
  check(ibu_resolve_barcodes(c_, wl.raw(), ab.raw(), d_recs, n, num, den, d_class, &c, st));
  return c;
}
inline void Context::resolve_barcodes_async(const Whitelist& wl, const Abundance& ab, void* d_recs, size_t n, uint8_t* d_class, uint64_t num,
                                            uint64_t den, void* st) {
  check(ibu_resolve_barcodes(c_, wl.raw(), ab.raw(), d_recs, n, num, den, d_class, nullptr, st));
}
inline CorrectCounts Context::correct_barcodes(const Whitelist& wl, void* d_recs, size_t n, uint32_t max_mismatches, uint8_t* d_class, void* st) {
  CorrectCounts c{};
  check(ibu_correct_barcodes(c_, wl.raw(), d_recs, n, max_mismatches, d_class, &c, st));
  return c;
}
inline void Context::correct_barcodes_async(const Whitelist& wl, void* d_recs, size_t n, uint32_t max_mismatches, uint8_t* d_class, void* st) {
  check(ibu_correct_barcodes(c_, wl.raw(), d_recs, n, max_mismatches, d_class, nullptr, st));
}

inline std::vector<MatrixEntry> Context::pair_counts(const void* d_sorted, size_t n) {
  size_t np = 0, nt = 0;
  check(ibu_pair_counts(c_, d_sorted, n, nullptr, nullptr, nullptr, nullptr, 0, &np, &nt, nullptr));
  std::vector<MatrixEntry> out;
  if (!np) return out;
  DeviceBuffer a(*this, 8 * np), b(*this, 8 * np), c(*this, 8 * np), d(*this, 8 * np);
  check(ibu_pair_counts(c_, d_sorted, n, a.as<uint64_t>(), b.as<uint64_t>(), c.as<uint64_t>(), d.as<uint64_t>(), np, &np, &nt, nullptr));
  auto ha = a.download<uint64_t>(np), hb = b.download<uint64_t>(np), hc = c.download<uint64_t>(np), hd = d.download<uint64_t>(np);
  out.reserve(np);
  for (size_t k = 0; k < np; ++k) out.push_back({ha[k], hb[k], hc[k], hd[k]});
  return out;
}
inline std::vector<MatrixEntry> Context::count_matrix(void* d_recs, void* d_tmp, size_t n, size_t cap, bool leave_swapped) {
  std::vector<MatrixEntry> out;
  if (!n) return out;
  if (!cap) cap = n;
  DeviceBuffer a(*this, 8 * cap), b(*this, 8 * cap), c(*this, 8 * cap), d(*this, 8 * cap);
  size_t ne = 0, nm = 0;
  check(ibu_count_matrix(c_, d_recs, d_tmp, n, leave_swapped ? IBU_COUNT_LEAVE_SWAPPED : 0u, a.as<uint64_t>(), b.as<uint64_t>(), c.as<uint64_t>(),
                         d.as<uint64_t>(), cap, &ne, &nm, nullptr));
  auto ha = a.download<uint64_t>(ne), hb = b.download<uint64_t>(ne), hc = c.download<uint64_t>(ne), hd = d.download<uint64_t>(ne);
  out.reserve(ne);
  for (size_t k = 0; k < ne; ++k) out.push_back({ha[k], hb[k], hc[k], hd[k]});
  return out;
}
inline std::vector<BarcodeMetrics> Context::barcode_metrics(const void* d_recs, size_t n, const FeatureSet& set, uint32_t set_word) {
  size_t nb = 0;
  check(ibu_barcode_metrics(c_, d_recs, n, set.d_bits, set.bits, set_word, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &nb, nullptr));
  std::vector<BarcodeMetrics> out;
  if (!nb) return out;
  DeviceBuffer a(*this, 8 * nb), b(*this, 8 * nb), c(*this, 8 * nb), d(*this, 8 * nb), e(*this, 8 * nb), f(*this, 8 * nb);
  check(ibu_barcode_metrics(c_, d_recs, n, set.d_bits, set.bits, set_word, a.as<uint64_t>(), b.as<uint64_t>(), c.as<uint64_t>(), d.as<uint64_t>(),
                            e.as<uint64_t>(), f.as<uint64_t>(), nb, &nb, nullptr));
  auto ha = a.download<uint64_t>(nb), hb = b.download<uint64_t>(nb), hc = c.download<uint64_t>(nb), hd = d.download<uint64_t>(nb),
       he = e.download<uint64_t>(nb), hf = f.download<uint64_t>(nb);
  out.reserve(nb);
  for (size_t k = 0; k < nb; ++k) out.push_back({ha[k], hb[k], hc[k], hd[k], he[k], hf[k]});
  return out;
}
inline std::vector<std::tuple<uint64_t, uint64_t, uint64_t>> Context::barcode_counts(const void* d_sorted, size_t n) {
  size_t nb = 0, np = 0;
  check(ibu_barcode_counts(c_, d_sorted, n, nullptr, nullptr, nullptr, 0, &nb, &np, nullptr));
  std::vector<std::tuple<uint64_t, uint64_t, uint64_t>> out;
  if (!nb) return out;
  DeviceBuffer b(*this, 8 * nb), c(*this, 8 * nb), u(*this, 8 * nb);
  check(ibu_barcode_counts(c_, d_sorted, n, b.as<uint64_t>(), c.as<uint64_t>(), u.as<uint64_t>(), nb, &nb, &np, nullptr));
  auto hb = b.download<uint64_t>(nb), hc = c.download<uint64_t>(nb), hu = u.download<uint64_t>(nb);
  out.reserve(nb);
  for (size_t k = 0; k < nb; ++k) out.emplace_back(hb[k], hc[k], hu[k]);
  return out;
}
}  // namespace device

inline StreamStats Writer::write_batch_device(device::Context& ctx, const void* d_records, size_t n, const RingConfig* ring, void* producer_stream) {
  StreamStats st{};
  check(ibu_writer_write_batch_device_on(w_, ctx.raw(), ring, d_records, n, producer_stream, &st));
  return st;
}
inline StreamStats Writer::write_ascii_batch(device::Context& ctx, const uint8_t* bc_ascii, const uint8_t* umi_ascii, const uint64_t* index,
                                             size_t n, uint32_t bc_len, uint32_t umi_len, uint64_t first_index, const RingConfig* ring) {
  StreamStats st{};
  check(ibu_writer_write_ascii_batch(w_, ctx.raw(), ring, bc_ascii, umi_ascii, index, first_index, n, bc_len, umi_len, &st));
  return st;
}
inline MmapReader::Decoded MmapReader::decode_to_host(device::Context& ctx, size_t shard, size_t n_shards, const RingConfig* ring) const {
  const auto range = shard_range(len(), n_shards, shard);
  const size_t n = range.second - range.first;
  const Header h = header();
  Decoded d;
  d.bc.resize(n * h.bc_len); d.umi.resize(n * h.umi_len); d.index.resize(n);
  d.stats = StreamStats{};
  check(ibu_mmap_decode_to_host(m_, ctx.raw(), ring, shard, n_shards, d.bc.data(), d.umi.data(), d.index.data(), &d.stats));
  return d;
}
// ---- pull-style device record stream (ibu_stream_*) -------------------------------------------------------------------
// The device form of Reader::read_batch + Iterator (reader.rs:218-242, :279-306) and of process_parallel's per-batch loop
// (mmap.rs:312-320): `while (auto b = stream.next()) { ...kernels on b->d_records...; }` — a batch gives its ring slot back
// when it goes out of scope (work queued on its stream so far is waited for before the slot is refilled).
class DeviceBatch {
 public:
  const void* d_records = nullptr;   // n AoS records in a device ring slot
  size_t n = 0;
  uint64_t first_index = 0;          // number of the batch's first record (mmap: position in the map; reader: records delivered before)
  DeviceBatch(ibu_stream_t* s, const void* d, size_t n_, uint64_t first, void* stream) : d_records(d), n(n_), first_index(first), s_(s), stream_(stream) {}
  DeviceBatch(DeviceBatch&& o) noexcept : d_records(o.d_records), n(o.n), first_index(o.first_index), s_(o.s_), stream_(o.stream_) { o.s_ = nullptr; }
  DeviceBatch(const DeviceBatch&) = delete;
  DeviceBatch& operator=(const DeviceBatch&) = delete;
  ~DeviceBatch() { if (s_) (void)ibu_stream_release(s_, d_records, stream_); }
  void release() { if (s_) { ibu_stream_t* s = s_; s_ = nullptr; check(ibu_stream_release(s, d_records, stream_)); } }
 private:
  ibu_stream_t* s_;
  void* stream_;
};
class DeviceStream {
 public:
  explicit DeviceStream(ibu_stream_t* s) : s_(s) {}
  DeviceStream(DeviceStream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
  DeviceStream(const DeviceStream&) = delete;
  DeviceStream& operator=(const DeviceStream&) = delete;
  ~DeviceStream() { if (s_) ibu_stream_close(s_); }
  Header header() const { Header h; check(ibu_stream_header(s_, &h)); return h; }
  // `stream`: the hipStream_t the batch will be read on (nullptr: the context's).  nullopt at the end; a source error
  // (TruncatedRecord, Io, Niffler ...) throws after the batches in front of it have been handed out.
  std::optional<DeviceBatch> next(void* stream = nullptr) {
    const void* d = nullptr; size_t n = 0; uint64_t first = 0;
    check(ibu_stream_next(s_, stream, &d, &n, &first));
    if (n == 0) return std::nullopt;
    return std::optional<DeviceBatch>(std::in_place, s_, d, n, first, stream);
  }
  StreamStats stats() const { StreamStats st{}; check(ibu_stream_stats(s_, &st)); return st; }
  ibu_stream_t* raw() const { return s_; }
  // Reader::from_path + the stream (ibu_stream_open_path): a BGZF file the device load takes is read in ranges inflated on the device,
  // anything else through the Reader of the same descriptor.  The stream owns its source.
  static inline DeviceStream from_path(const char* path, device::Context& ctx, const RingConfig* ring = nullptr);
 private:
  ibu_stream_t* s_;
};
inline DeviceStream DeviceStream::from_path(const char* path, device::Context& ctx, const RingConfig* ring) {
  ibu_stream_t* s = nullptr;
  check(ibu_stream_open_path(path, ctx.raw(), ring, &s));
  return DeviceStream(s);
}
inline DeviceStream Reader::device_stream(device::Context& ctx, const RingConfig* ring) {
  ibu_stream_t* s = nullptr;
  check(ibu_stream_open_reader(r_, ctx.raw(), ring, &s));
  return DeviceStream(s);
}
inline DeviceStream MmapReader::device_stream(device::Context& ctx, size_t shard, size_t n_shards, const RingConfig* ring) const {
  ibu_stream_t* s = nullptr;
  check(ibu_stream_open_mmap(m_, ctx.raw(), ring, shard, n_shards, &s));
  return DeviceStream(s);
}
inline std::pair<ReduceResult, StreamStats> Reader::process_device_reduce(device::Context& ctx, const RingConfig* ring) {
  ReduceResult r{}; StreamStats st{};
  check(ibu_reader_process_device(r_, ctx.raw(), ring, IBU_PROC_REDUCE, &r, &st));
  return {r, st};
}
inline StreamStats Reader::process_device_decode(device::Context& ctx, const DecodeSink& sink_in, const RingConfig* ring) {
  ibu_decode_sink_t sink = sink_in; StreamStats st{};
  check(ibu_reader_process_device(r_, ctx.raw(), ring, IBU_PROC_DECODE, &sink, &st));
  return st;
}
inline std::pair<ReduceResult, StreamStats> MmapReader::process_device_reduce(device::Context& ctx, size_t shard, size_t n_shards,
                                                                               const RingConfig* ring) const {
  ReduceResult r{}; StreamStats st{};
  check(ibu_mmap_process_device(m_, ctx.raw(), ring, IBU_PROC_REDUCE, shard, n_shards, &r, &st));
  return {r, st};
}
inline StreamStats MmapReader::process_device_decode(device::Context& ctx, const DecodeSink& sink_in, size_t shard, size_t n_shards,
                                                     const RingConfig* ring) const {
  ibu_decode_sink_t sink = sink_in; StreamStats st{};
  check(ibu_mmap_process_device(m_, ctx.raw(), ring, IBU_PROC_DECODE, shard, n_shards, &sink, &st));
  return st;
}
inline std::pair<ReduceResult, std::vector<ReduceResult>> MmapReader::process_devices_reduce(const std::vector<int32_t>& devices,
                                                                                             const RingConfig* ring) const {
  size_t n = devices.size();
  if (n == 0) n = (size_t)device::device_count();
  ReduceResult total{};
  std::vector<ReduceResult> parts(n ? n : 1);
  check(ibu_mmap_process_devices(m_, devices.empty() ? nullptr : devices.data(), devices.size(), ring, IBU_PROC_REDUCE, parts.data(), &total, nullptr));
  parts.resize(n);
  return {total, parts};
}
inline void MmapReader::process_devices_decode(const std::vector<int32_t>& devices, std::vector<DecodeSink>& sinks, const RingConfig* ring) const {
  if (devices.empty() || sinks.size() != devices.size()) {
    ibu_error_detail_t d{};
    d.code = IBU_ERR_INVALID_ARG;
    snprintf(d.message, sizeof d.message, "Invalid argument: one DecodeSink per listed device");
    throw IbuError(IBU_ERR_INVALID_ARG, d);
  }
  check(ibu_mmap_process_devices(m_, devices.data(), devices.size(), ring, IBU_PROC_DECODE, sinks.data(), nullptr, nullptr));
}

}  // namespace ibu
