"""ibu_amd — MI355X-native batch record-stream + 2-bit codec path for the IBU format.

A thin Python mirror of the reference crate's public API (src/lib.rs:178-181:
Header, Record, HEADER_SIZE, MAGIC, RECORD_SIZE, VERSION, IbuError, load_to_vec, MmapReader,
Reader, Writer, ParallelProcessor, ParallelReader) over the C ABI of include/ibu_hip.h, plus
the device context that exposes the HIP kernels.  All work happens in libibu_hip.so; this
package binds it and nothing else (no numpy/torch arithmetic stands in for a kernel).

The device pipeline of a single-cell run, every step on resident records: load -> Context.correct_barcodes (-> Abundance.add ->
Context.resolve_barcodes: ambiguous barcodes to the candidate with nearly all of the exact reads) -> select_records -> sort_records -> classify_molecules -> select_records -> call_cells -> select_records -> count_matrix(leave_swapped=True) ->
filter_barcodes (the per-barcode QC filter: too few or too many features / UMIs, too large a share of a feature set built with
Context.feature_bitmap; barcode_metrics returns the table itself) -> select_records -> feature_metrics -> filter_features (the
other axis: features seen in too few cells) -> select_records -> pair_counts, or, in the forms other tools read, matrix_csr (a CSR
triple on the device) and write_matrix_market (the 10x directory, its text formatted on the device); for hashtag, antibody and guide
libraries assign_features (one line per cell: its dominant feature, the runner-up, the row total and a class, from matrix_row_top
and assign_rows over the entry table), and, to carry such a per-barcode verdict onto the records of any library with the same
barcodes, labels_from_assignment -> label_records (-> select_records: one sample of a multiplexed library; partition_records /
partition_by_label: every sample at once, in one pass).
"""
import copy
import ctypes as C
import weakref
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import CAllocProbe, CAssignCounts, CAssignRule, CBarcodeFilterCounts, CBarcodeLimits, CFeatureFilterCounts, CFeatureLimits, CCellCounts, CCorrectCounts, CResolveCounts, CDecodeSink, CMoleculeCounts, CErrorDetail, CKeyPlan, CHeader, CNumaInfo, CProcessorVTable, CRecord, CReduceResult, CRingConfig, CSaturationPoint, CStreamStats

lib = _lib.load()

MAGIC = 0x21554249  # src/constructs/header.rs:5
VERSION = 2  # header.rs:6
HEADER_SIZE = 32  # header.rs:7
RECORD_SIZE = 24  # record.rs:3
DEFAULT_BUFFER_SIZE = 48 * 1024 * RECORD_SIZE  # reader.rs:14, writer.rs:10
BATCH_SIZE = 1024 * 1024  # mmap.rs:284

PROC_REDUCE, PROC_DECODE = 1, 2
COUNT_LEAVE_SWAPPED = 1  # ibu_count_matrix flags (IBU_COUNT_LEAVE_SWAPPED)
MOLECULE_KEPT, MOLECULE_MINOR, MOLECULE_TIED = 0, 1, 2  # the classes of ibu_classify_molecules (IBU_MOLECULE_*)
MOLECULES_TIE_FIRST = 1  # ibu_classify_molecules flags (IBU_MOLECULES_TIE_FIRST)

CELL, CELL_BACKGROUND = 0, 1  # the classes of ibu_call_cells (IBU_CELL, IBU_CELL_BACKGROUND)
CELLS_MIN, CELLS_TOP, CELLS_ORDMAG = 0, 1, 2  # its modes (IBU_CELLS_*)
CELLS_BY_READS = 1  # its flag (IBU_CELLS_BY_READS)
BARCODE_PASS, BARCODE_LOW, BARCODE_HIGH, BARCODE_SET = 0, 1, 2, 3  # the classes of ibu_filter_barcodes (IBU_BARCODE_*)
BARCODE_RESOLVED = 4  # the class ibu_resolve_barcodes gives a record it resolves (IBU_BARCODE_RESOLVED), beside 0..3 of ibu_correct_barcodes
LABEL_MATCH = 1  # ibu_label_records flags (IBU_LABEL_MATCH)
LABEL_IS, LABEL_OTHER, LABEL_MISSING = 0, 1, 2  # its classes in match mode (IBU_LABEL_*)
LABEL_BINS = 257  # its histogram: the labels 0 .. 255, then the records not found (IBU_LABEL_BINS)
PART_NONE = 255  # ibu_partition_records: the part_of entry of a class whose records are dropped (IBU_PART_NONE)
#: the table of ibu_barcode_metrics: one numpy u64 column each, a row per barcode in input order
BarcodeMetrics = namedtuple("BarcodeMetrics", "barcodes reads pairs triples set_reads set_triples")
#: the totals of one ibu_filter_barcodes call (ibu_barcode_filter_counts_t without its reserved word); the by_class fields are 4-tuples
BarcodeFilterCounts = namedtuple("BarcodeFilterCounts", "barcodes barcodes_by_class reads_by_class triples_passed set_triples_passed")
FEATURE_PASS, FEATURE_LOW, FEATURE_HIGH, FEATURE_UNKNOWN = 0, 1, 2, 3  # the classes of ibu_filter_features (IBU_FEATURE_*)
FEATURE_ACCUMULATE = 1  # ibu_feature_metrics flags (IBU_FEATURE_ACCUMULATE)
#: the table of ibu_feature_metrics: three DeviceBuffers of n_features u64 each (cells is None for feature_word 2), and the totals of
#: the call that made it — (reads, umis, cells in range, reads out of range)
FeatureTable = namedtuple("FeatureTable", "reads umis cells n_features totals")
#: the totals of one ibu_filter_features call (ibu_feature_filter_counts_t without its reserved word): a 3-tuple and a 4-tuple
FeatureFilterCounts = namedtuple("FeatureFilterCounts", "features_by_class reads_by_class")
#: what ibu_matrix_rows leaves: the number of rows and three DeviceBuffers of u64 — the value of every row (n_rows words), the CSR
#: indptr (n_rows + 1 words) and the 0-based row of every entry (None where not asked for)
MatrixRows = namedtuple("MatrixRows", "n_rows d_keys d_ptr d_row_of_entry")
NO_KEY = (1 << 64) - 1  # the top key of a row in which no entry took part (IBU_NO_KEY)
ROW_ASSIGNED, ROW_NONE, ROW_MIXED = 0, 1, 2  # the classes of ibu_assign_rows (IBU_ROW_*)
#: the totals of one ibu_assign_rows call (ibu_assign_counts_t)
AssignCounts = namedtuple("AssignCounts", "rows assigned none mixed")
MTX_BANNER = "%%MatrixMarket matrix coordinate integer general"
SAMPLE_KEPT, SAMPLE_DROPPED = 0, 1  # the classes of ibu_subsample_class (IBU_SAMPLE_KEPT, IBU_SAMPLE_DROPPED)
SATURATION_MAX_POINTS = 32
#: one point of ibu_saturation_curve (ibu_saturation_point_t)
SaturationPoint = namedtuple("SaturationPoint", "threshold reads barcodes molecules")
#: the totals of one ibu_call_cells call (ibu_cell_counts_t)
CellCounts = namedtuple("CellCounts", "barcodes cells threshold baseline reads_cells reads_background umis_cells umis_background")
#: the totals of one ibu_classify_molecules call (ibu_molecule_counts_t without its reserved word)
MoleculeCounts = namedtuple("MoleculeCounts", "molecules candidates resolved tied reads_kept reads_minor reads_tied")

#: numpy view of a `&[Record]` (bytemuck::cast_slice)
REC_DTYPE = np.dtype([("barcode", "<u8"), ("umi", "<u8"), ("index", "<u8")])


# ---- errors (src/error.rs:56-128) ---------------------------------------------------------------
class IbuError(Exception):
    """`kind` is the reference's variant name; payload fields follow the variant."""

    def __init__(self, code, detail):
        self.code = code
        self.kind = lib.ibu_status_name(code).decode()
        self.a, self.b, self.os_errno = detail.a, detail.b, detail.os_errno
        self.expected, self.actual = detail.a, detail.b  # InvalidMagicNumber / InvalidVersion
        self.pos = detail.a  # TruncatedRecord
        self.idx, self.max = detail.a, detail.b  # InvalidIndex
        self.length = detail.a  # InvalidBarcodeLength / InvalidUmiLength
        self.first_bad, self.n_bad = detail.a, detail.b  # InvalidBase
        super().__init__(f"{self.kind}: {detail.message.decode(errors='replace')}")


def _check(rc):
    if rc:
        d = CErrorDetail()
        lib.ibu_last_error(C.byref(d))
        raise IbuError(rc, d)


# ---- Header / Record ---------------------------------------------------------------------------------
class Header:
    """src/constructs/header.rs:44-61 — 32-byte POD."""

    def __init__(self, bc_len, umi_len):  # Header::new :84-93
        self._h = CHeader()
        lib.ibu_header_init(C.byref(self._h), bc_len, umi_len)

    magic = property(lambda s: s._h.magic, lambda s, v: setattr(s._h, "magic", v))
    version = property(lambda s: s._h.version, lambda s, v: setattr(s._h, "version", v))
    bc_len = property(lambda s: s._h.bc_len, lambda s, v: setattr(s._h, "bc_len", v))
    umi_len = property(lambda s: s._h.umi_len, lambda s, v: setattr(s._h, "umi_len", v))
    flags = property(lambda s: s._h.flags, lambda s, v: setattr(s._h, "flags", v))
    reserved = property(lambda s: bytes(s._h.reserved))

    def set_sorted(self):  # :111-113
        lib.ibu_header_set_sorted(C.byref(self._h))

    def sorted(self):  # :130-132
        return bool(lib.ibu_header_sorted(C.byref(self._h)))

    def validate(self):  # :167-187
        _check(lib.ibu_header_validate(C.byref(self._h)))

    def as_bytes(self):  # :203-205
        buf = C.create_string_buffer(HEADER_SIZE)
        _check(lib.ibu_header_as_bytes(C.byref(self._h), buf, HEADER_SIZE))
        return buf.raw

    @classmethod
    def from_bytes(cls, b):  # :226-228 (the reference panics on a wrong length; here InvalidArg)
        h = cls.__new__(cls)
        h._h = CHeader()
        _check(lib.ibu_header_from_bytes(bytes(b), len(b), C.byref(h._h)))
        return h

    @classmethod
    def _wrap(cls, ch):
        h = cls.__new__(cls)
        h._h = ch
        return h

    def __eq__(self, o):
        return isinstance(o, Header) and self.as_bytes() == o.as_bytes()

    def __hash__(self):
        return hash(self.as_bytes())

    def __repr__(self):
        return (f"Header {{ magic: {self.magic:#x}, version: {self.version}, bc_len: {self.bc_len}, "
                f"umi_len: {self.umi_len}, flags: {self.flags} }}")


class Record(namedtuple("Record", ["barcode", "umi", "index"])):
    """src/constructs/record.rs:58-66 — tuple order is the derived lexicographic Ord."""
    __slots__ = ()

    def __new__(cls, barcode=0, umi=0, index=0):
        return super().__new__(cls, int(barcode), int(umi), int(index))

    def _c(self):
        return CRecord(self.barcode, self.umi, self.index)

    def as_bytes(self):  # :108-110
        buf = C.create_string_buffer(RECORD_SIZE)
        r = self._c()
        _check(lib.ibu_record_as_bytes(C.byref(r), buf, RECORD_SIZE))
        return buf.raw

    @classmethod
    def from_bytes(cls, b):  # :130-132
        r = CRecord()
        _check(lib.ibu_record_from_bytes(bytes(b), len(b), C.byref(r)))
        return cls(r.barcode, r.umi, r.index)

    def cmp(self, other):
        a, b = self._c(), Record(*other)._c()
        return lib.ibu_record_cmp(C.byref(a), C.byref(b))


def records_array(rows):
    """iterable of Record / 3-tuples, or an (n,3) integer array -> contiguous AoS array."""
    if isinstance(rows, np.ndarray) and rows.dtype == REC_DTYPE:
        return np.ascontiguousarray(rows)
    a = np.asarray(list(rows) if not isinstance(rows, np.ndarray) else rows, dtype=np.uint64).reshape(-1, 3)
    out = np.empty(a.shape[0], dtype=REC_DTYPE)
    out["barcode"], out["umi"], out["index"] = a[:, 0], a[:, 1], a[:, 2]
    return out


def _hptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- Writer (src/io/writer.rs) ---------------------------------------------------------------------------
class Writer:
    """`Writer<W>`; W is a path (from_path), a file descriptor, a Python file-like (callback
    sink) or memory (`Writer::new(Vec::new(), header)`)."""

    def __init__(self, inner=None, header=None, _handle=None):
        self._w = _handle
        self._cb = None
        if _handle is not None:
            return
        hp = C.byref(header._h) if header is not None else None
        out = C.c_void_p()
        if inner is None or isinstance(inner, (bytearray, list)):  # Vec<u8>
            _check(lib.ibu_writer_open_mem(hp, C.byref(out)))
        elif isinstance(inner, int):
            _check(lib.ibu_writer_open_fd(inner, hp, C.byref(out)))
        else:  # any object with .write(bytes) [and .flush()]
            def _wr(_u, data, n, _f=inner):
                try:
                    _f.write(C.string_at(data, n))
                    return 0
                except OSError as e:
                    return e.errno or 5
            def _fl(_u, _f=inner):
                try:
                    if hasattr(_f, "flush"):
                        _f.flush()
                    return 0
                except OSError as e:
                    return e.errno or 5
            self._cb = (_lib.WRITE_FN(_wr), _lib.FLUSH_FN(_fl))
            _check(lib.ibu_writer_open_callback(self._cb[0], self._cb[1], None, hp, C.byref(out)))
        self._w = out

    @classmethod
    def new(cls, inner, header):  # Writer::new :129-143
        return cls(inner, header)

    @classmethod
    def new_headless(cls, inner=None):  # :169-179
        return cls(inner, None)

    @classmethod
    def from_path(cls, path, header):  # :556-559
        out = C.c_void_p()
        _check(lib.ibu_writer_open_path(str(path).encode(), C.byref(header._h) if header else None, C.byref(out)))
        return cls(_handle=out)

    @classmethod
    def from_stdout(cls, header):  # :587-589
        return cls(1, header)

    @classmethod
    def from_optional_path(cls, path, header):  # :617-626
        return cls.from_path(path, header) if path is not None else cls.from_stdout(header)

    def write_record(self, record):  # :260-273
        r = Record(*record)._c()
        _check(lib.ibu_writer_write_record(self._w, C.byref(r)))

    def write_batch(self, records):  # :315-318
        a = records_array(records)
        _check(lib.ibu_writer_write_batch(self._w, _hptr(a), a.shape[0]))

    def write_iter(self, records):  # :383-391
        for r in records:
            self.write_record(r)

    def write_batch_device(self, ctx, d_records, n, ring=None, stream=None):
        """Device-resident AoS records -> pinned ring -> this writer (write_batch rules).  `stream`: the stream the
        records were produced on (None: the context's own)."""
        st = CStreamStats()
        _check(lib.ibu_writer_write_batch_device_on(self._w, ctx._c, _ring(ring), _dptr(d_records), n, stream, C.byref(st)))
        return st

    def write_ascii_batch(self, ctx, bc_ascii, umi_ascii, bc_len, umi_len, index=None, first_index=0, ring=None):
        """Host ASCII rows (uint8 arrays of n*bc_len / n*umi_len bytes) -> 2-bit records -> this writer, encoded on
        the GPU (README.md:38-47's encode-then-write loop as one batch call)."""
        bc = np.ascontiguousarray(bc_ascii, dtype=np.uint8).reshape(-1)
        umi = np.ascontiguousarray(umi_ascii, dtype=np.uint8).reshape(-1)
        n = bc.size // bc_len
        assert bc.size == n * bc_len and umi.size == n * umi_len
        idx = None if index is None else np.ascontiguousarray(index, dtype=np.uint64)
        st = CStreamStats()
        _check(lib.ibu_writer_write_ascii_batch(self._w, ctx._c, _ring(ring), _hptr(bc), _hptr(umi),
                                                _hptr(idx) if idx is not None else None, first_index, n, bc_len, umi_len,
                                                C.byref(st)))
        return st

    def ingest(self, other):  # :477-482
        _check(lib.ibu_writer_ingest(self._w, other._w))

    def finish(self):  # :429-433
        _check(lib.ibu_writer_finish(self._w))

    def records_written(self):  # :207-209
        return lib.ibu_writer_records_written(self._w)

    def inner_bytes(self):
        """What a `Vec<u8>` sink holds right now (tests peek at `writer.inner`)."""
        p, n = C.c_void_p(), C.c_size_t()
        _check(lib.ibu_writer_mem_view(self._w, C.byref(p), C.byref(n)))
        return C.string_at(p, n.value) if n.value else b""

    def into_inner(self):  # :507-511 — no flush
        p, n = C.c_void_p(), C.c_size_t()
        w, self._w = self._w, None
        _check(lib.ibu_writer_into_inner(w, C.byref(p), C.byref(n)))
        if not p:
            return None
        data = C.string_at(p, n.value)
        lib.ibu_free(p)
        return data

    def close(self):  # Drop :519-523
        if getattr(self, "_w", None):
            lib.ibu_writer_close(self._w)
            self._w = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


# ---- Reader (src/io/reader.rs) -------------------------------------------------------------------------------
class Reader:
    """`Reader<R>`; R is bytes (Cursor), a file descriptor or a file-like with .readinto/.read."""

    def __init__(self, inner=None, _handle=None):
        self._r, self._keep, self._cb = _handle, None, None
        if _handle is not None:
            return
        out = C.c_void_p()
        if isinstance(inner, (bytes, bytearray, memoryview, np.ndarray)):
            self._keep = np.frombuffer(bytes(inner), dtype=np.uint8)
            _check(lib.ibu_reader_open_mem(_hptr(self._keep), self._keep.size, C.byref(out)))
        elif isinstance(inner, int):
            _check(lib.ibu_reader_open_fd(inner, C.byref(out)))
        else:
            def _rd(_u, dst, cap, got, _f=inner):
                try:
                    b = _f.read(cap)
                    C.memmove(dst, b, len(b))
                    got[0] = len(b)
                    return 0
                except OSError as e:
                    return e.errno or 5
            self._cb = _lib.READ_FN(_rd)
            _check(lib.ibu_reader_open_callback(self._cb, None, C.byref(out)))
        self._r = out

    @classmethod
    def new(cls, inner):  # :152-176
        return cls(inner)

    @classmethod
    def from_path(cls, path):  # :345-352 (format sniffed: gzip / BGZF / bzip2 / xz / zstd, like niffler)
        out = C.c_void_p()
        _check(lib.ibu_reader_open_path(str(path).encode(), C.byref(out)))
        return cls(_handle=out)

    @classmethod
    def from_stdin(cls):  # :389-396
        out = C.c_void_p()
        _check(lib.ibu_reader_open_fd(0, C.byref(out)))
        return cls(_handle=out)

    @classmethod
    def from_optional_path(cls, path):  # :425-434
        return cls.from_path(path) if path is not None else cls.from_stdin()

    def header(self):  # :244-246
        h = CHeader()
        _check(lib.ibu_reader_header(self._r, C.byref(h)))
        return Header._wrap(h)

    def read_batch(self):  # :218-242
        has = C.c_int32()
        _check(lib.ibu_reader_read_batch(self._r, C.byref(has)))
        return bool(has.value)

    @property
    def bytes_read(self):
        return lib.ibu_reader_bytes_read(self._r)

    def buffered(self):
        """Zero-copy numpy view of the records left in the current refill."""
        p, n = C.c_void_p(), C.c_size_t()
        _check(lib.ibu_reader_buffered(self._r, C.byref(p), C.byref(n)))
        if not n.value:
            return np.empty(0, dtype=REC_DTYPE)
        raw = (C.c_uint8 * (n.value * RECORD_SIZE)).from_address(p.value)
        raw._owner = self  # valid until the next read_batch(); keeps the reader itself alive
        return np.frombuffer(raw, dtype=REC_DTYPE)

    def consume(self, n):
        _check(lib.ibu_reader_consume(self._r, n))

    def __iter__(self):
        return self

    def __next__(self):  # Iterator::next :279-306; an Err item is raised
        r, got = CRecord(), C.c_int32()
        _check(lib.ibu_reader_next(self._r, C.byref(r), C.byref(got)))
        if not got.value:
            raise StopIteration
        return Record(r.barcode, r.umi, r.index)

    def process_device(self, ctx, proc=PROC_REDUCE, sink=None, ring=None):
        """Stream the rest of this reader (plain or gzip) through the pinned ring to a device
        processor.  Returns (result, stats).  PROC_DECODE: sink = (d_bc, d_umi, d_index[, cap_records]); without
        cap_records the capacity is what the DeviceBuffers hold.  A stream longer than that raises InvalidArg."""
        h = self.header()
        return ctx._run_proc(lambda c, rg, s, st: lib.ibu_reader_process_device(self._r, c, rg, proc, s, st),
                             proc, sink, ring, (h.bc_len, h.umi_len))

    def device_stream(self, ctx, ring=None):
        """Pull-style device stream over the rest of this reader (ibu_stream_open_reader): iterate DeviceBatches."""
        return DeviceStream._open(lambda out: lib.ibu_stream_open_reader(self._r, ctx._c, _ring(ring), out), ctx, self)

    def close(self):
        for st in list(getattr(self, "_streams", ())):   # a producer thread must not outlive the reader it reads
            st.close()
        if getattr(self, "_r", None):
            lib.ibu_reader_close(self._r)
            self._r = None

    __del__ = close


def load_to_vec(path):  # src/io/reader.rs:510-535
    h, p, n = CHeader(), C.c_void_p(), C.c_size_t()
    _check(lib.ibu_load_to_vec(str(path).encode(), C.byref(h), C.byref(p), C.byref(n)))
    # (c_char * nbytes).from_address: string_at takes a C int and fails beyond 2 GiB
    recs = (np.frombuffer((C.c_char * (n.value * RECORD_SIZE)).from_address(p.value), dtype=REC_DTYPE).copy()
            if n.value else np.empty(0, REC_DTYPE))
    lib.ibu_free(p)
    return Header._wrap(h), recs


# ---- parallel (src/parallel.rs, src/io/mmap.rs) ------------------------------------------------------------------
class ParallelProcessor:
    """src/parallel.rs:100-190.  Subclass and override process_record (and optionally
    on_batch_complete / set_tid / get_tid).  `clone()` is `P: Clone`: shallow copy, so shared
    accumulators (the Arc<Mutex<..>> pattern) stay shared."""

    def process_record(self, record):
        raise NotImplementedError

    def on_batch_complete(self):  # default Ok(()) :137-139
        return None

    def set_tid(self, tid):  # default no-op :166-168
        pass

    def get_tid(self):  # default None :187-189
        return None

    def clone(self):
        return copy.copy(self)


class ProcessError(Exception):
    """Raise from process_record / on_batch_complete to return IbuError::Process."""


def shard_range(length, n_shards, shard):  # mmap.rs:297-307
    s, e = C.c_size_t(), C.c_size_t()
    _check(lib.ibu_shard_range(length, n_shards, shard, C.byref(s), C.byref(e)))
    return s.value, e.value


class MmapReader:
    """src/io/mmap.rs:99-332 (MmapReader + its ParallelReader impl)."""

    def __init__(self, path=None, _handle=None):
        if _handle is None:
            _handle = C.c_void_p()
            _check(lib.ibu_mmap_open(str(path).encode(), C.byref(_handle)))
        self._m = _handle

    @classmethod
    def new(cls, path):  # :143-161
        return cls(path)

    def clone(self):  # Arc clone :99
        out = C.c_void_p()
        _check(lib.ibu_mmap_clone(self._m, C.byref(out)))
        return MmapReader(_handle=out)

    def len(self):  # :178-180
        return lib.ibu_mmap_len(self._m)

    __len__ = len

    def header(self):  # :201-203
        h = CHeader()
        _check(lib.ibu_mmap_header(self._m, C.byref(h)))
        return Header._wrap(h)

    def slice(self, start, end):  # :253-270 — zero-copy view into the map
        p, n = C.c_void_p(), C.c_size_t()
        _check(lib.ibu_mmap_slice(self._m, start, end, C.byref(p), C.byref(n)))
        raw = (C.c_uint8 * (n.value * RECORD_SIZE)).from_address(p.value)
        raw._owner = self  # the borrow `&'a [Record]`: the view keeps this handle (and so the map) alive
        return np.frombuffer(raw, dtype=REC_DTYPE)

    def map_ptr(self):
        return lib.ibu_mmap_base(self._m)

    def process_parallel(self, processor, num_threads):  # :286-332, host processor (user code)
        clones, errors = {}, []

        def _clone(_u):
            c = processor.clone()
            key = len(clones) + 1
            clones[key] = c
            return key

        def _drop(_k):
            pass

        def _proc(k, rec):
            try:
                r = rec[0]
                clones[k].process_record(Record(r.barcode, r.umi, r.index))
                return 0
            except Exception as e:  # -> IbuError::Process
                errors.append(e)
                return 1

        def _batch(k):
            try:
                clones[k].on_batch_complete()
                return 0
            except Exception as e:
                errors.append(e)
                return 1

        vt = CProcessorVTable(_lib.CLONE_FN(_clone), _lib.DROP_FN(_drop), _lib.PROCESS_FN(_proc),
                              _lib.BATCH_FN(_batch), _lib.TID_FN())
        _check(lib.ibu_mmap_process_parallel(self._m, C.byref(vt), None, num_threads))

    def process_device(self, ctx, proc=PROC_REDUCE, shard=0, n_shards=1, sink=None, ring=None):
        """One shard of the static split on one GPU, through the pinned ring."""
        h = self.header()
        return ctx._run_proc(
            lambda c, rg, s, st: lib.ibu_mmap_process_device(self._m, c, rg, proc, shard, n_shards, s, st),
            proc, sink, ring, (h.bc_len, h.umi_len))

    def process_devices(self, devices=(), proc=PROC_REDUCE, sinks=None, ring=None, contexts=None):
        """process_parallel(processor, n) with a GPU per worker, in ONE call (mmap.rs:286-332; ibu_mmap_process_devices):
        worker i = one host thread + one context on devices[i], shard i of the static split, first error in worker order
        wins.  devices = () means every visible device.  contexts: a list of Contexts to reuse instead of device ordinals
        (ibu_mmap_process_contexts).  PROC_REDUCE -> (total, [partial per device], [stats]); PROC_DECODE: `sinks` = one
        (d_bc, d_umi, d_index, cap_records) per device, each on its device -> (count, None, [stats])."""
        n = len(contexts) if contexts is not None else (len(devices) or device_count())
        stats = (CStreamStats * max(n, 1))()
        total = CReduceResult()
        if proc == PROC_REDUCE:
            parts = (CReduceResult * max(n, 1))()
            sink_p = C.cast(parts, C.c_void_p)
        else:
            if sinks is None or len(sinks) != n:
                raise ValueError("PROC_DECODE needs one sink per device")
            arr = (CDecodeSink * n)(*[CDecodeSink(_dptr(a), _dptr(b), _dptr(c), int(cap)) for a, b, c, cap in sinks])
            sink_p = C.cast(arr, C.c_void_p)
        if contexts is not None:
            cs = (C.c_void_p * n)(*[c._c for c in contexts])
            _check(lib.ibu_mmap_process_contexts(self._m, cs, n, _ring(ring), proc, sink_p, C.byref(total), stats))
        else:
            devs = (C.c_int32 * len(devices))(*devices) if len(devices) else None
            _check(lib.ibu_mmap_process_devices(self._m, devs, len(devices), _ring(ring), proc, sink_p, C.byref(total), stats))
        as_dict = lambda r: {"count": r.count, "sum": list(r.sum), "xor": list(r.xor_)}
        if proc == PROC_REDUCE:
            return as_dict(total), [as_dict(parts[i]) for i in range(n)], list(stats)[:n]
        return total.count, None, list(stats)[:n]

    def device_stream(self, ctx, shard=0, n_shards=1, ring=None):
        """Pull-style device stream over one shard of the static split (ibu_stream_open_mmap): iterate DeviceBatches."""
        return DeviceStream._open(lambda out: lib.ibu_stream_open_mmap(self._m, ctx._c, _ring(ring), shard, n_shards, out), ctx, self)

    def decode_to_host(self, ctx, shard=0, n_shards=1, ring=None, want=("bc", "umi", "index"), out=None):
        """One shard -> (barcode ASCII [n, bc_len], UMI ASCII [n, umi_len], index [n]) as numpy arrays in host
        memory, unpacked on the GPU.  Columns not in `want` come back as None.  out = (bc, umi, index) arrays of those
        shapes to fill instead of fresh ones (memory that has been written before takes no page faults: 1.7x the rate)."""
        a, b = shard_range(self.len(), n_shards, shard)
        n, h = b - a, self.header()
        if out is not None:
            bc, umi, idx = out
            for arr, shape, dt in ((bc, (n, h.bc_len), np.uint8), (umi, (n, h.umi_len), np.uint8), (idx, (n,), np.uint64)):
                if arr is not None and (arr.shape != shape or arr.dtype != dt or not arr.flags.c_contiguous):
                    raise ValueError("out: C-contiguous arrays of shapes (n, bc_len) u8, (n, umi_len) u8, (n,) u64")
        else:
            bc = np.empty((n, h.bc_len), dtype=np.uint8) if "bc" in want else None
            umi = np.empty((n, h.umi_len), dtype=np.uint8) if "umi" in want else None
            idx = np.empty(n, dtype=np.uint64) if "index" in want else None
        st = CStreamStats()
        _check(lib.ibu_mmap_decode_to_host(self._m, ctx._c, _ring(ring), shard, n_shards,
                                           _hptr(bc) if bc is not None else None, _hptr(umi) if umi is not None else None,
                                           _hptr(idx) if idx is not None else None, C.byref(st)))
        return bc, umi, idx, st

    def close(self):
        for st in list(getattr(self, "_streams", ())):   # a producer thread must not outlive the map it copies from
            st.close()
        if getattr(self, "_m", None):
            lib.ibu_mmap_close(self._m)
            self._m = None

    __del__ = close


# ---- device side ----------------------------------------------------------------------------------------------------
def _dptr(x):
    """int | DeviceBuffer | torch.Tensor | None -> c_void_p."""
    if x is None:
        return None
    if isinstance(x, int):
        return C.c_void_p(x)
    if hasattr(x, "ptr"):
        return C.c_void_p(x.ptr)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    raise TypeError(f"not a device pointer: {type(x)}")


def _ring(r):
    if r is None:
        return None
    if isinstance(r, CRingConfig):
        return C.byref(r)
    return C.byref(CRingConfig(r.get("slots", 0), r.get("slot_records", 0), r.get("feeder_threads", 0), 0))


def key_plan(or_words, and_words):
    """ibu_key_plan_t for records whose OR / AND words are given (Context.census, combined over the shards with | and &).
    plan.k = number of varying key bytes; compact / expand need plan.k <= 12."""
    plan = CKeyPlan()
    _check(lib.ibu_key_plan_init((C.c_uint64 * 3)(*[int(v) & (2**64 - 1) for v in or_words]),
                                 (C.c_uint64 * 3)(*[int(v) & (2**64 - 1) for v in and_words]), C.byref(plan)))
    return plan


def device_count():
    n = C.c_int32()
    rc = lib.ibu_device_count(C.byref(n))
    return n.value if rc == 0 else 0


class DeviceBuffer:
    """hipMalloc'ed bytes owned through the context (for callers without torch)."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes, self.owned = ctx, int(nbytes), True
        p = C.c_void_p()
        _check(lib.ibu_device_alloc(ctx._c, self.nbytes, C.byref(p)))
        self.ptr = p.value
        ctx._buffers.add(self)   # a context that closes first frees what it still owns (Context.close)

    @classmethod
    def wrap(cls, ctx, ptr, nbytes):
        """View of device memory owned by someone else (e.g. what load_to_device returned): never freed here."""
        b = cls.__new__(cls)
        b.ctx, b.ptr, b.nbytes, b.owned = ctx, int(ptr), int(nbytes), False
        return b

    @property
    def __cuda_array_interface__(self):
        """Flat uint8 view for consumers of the CUDA array interface (torch.as_tensor(buf, device=...) on ROCm too):
        bench.py uses it to compare buffers with torch as a checker that is not this library."""
        return {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.ptr, False), "version": 2, "strides": None}

    def upload(self, host):
        a = np.ascontiguousarray(host)
        assert a.nbytes <= self.nbytes
        _check(lib.ibu_memcpy_h2d(self.ctx._c, self.ptr, _hptr(a), a.nbytes, None))
        self.ctx.synchronize()
        return self

    def download(self, dtype=np.uint8, count=None, offset=0):
        dt = np.dtype(dtype)
        nbytes = (self.nbytes - offset) if count is None else count * dt.itemsize
        out = np.empty(nbytes // dt.itemsize, dtype=dt)
        _check(lib.ibu_memcpy_d2h(self.ctx._c, _hptr(out), self.ptr + offset, out.nbytes, None))
        self.ctx.synchronize()
        return out

    def free(self):
        if getattr(self, "ptr", 0) and getattr(self, "owned", False) and getattr(self.ctx, "_c", None):
            lib.ibu_device_free(self.ctx._c, self.ptr)
        self.ptr = 0

    __del__ = free


class CsrMatrix:
    """The cell x feature count matrix in CSR form, on the device (Context.matrix_csr): DeviceBuffers of u64 — `barcodes` (n_rows
    codes, row r's barcode), `indptr` (n_rows + 1), `indices` and `data` (nnz each; the feature number and the count of every
    entry).  The buffers speak the CUDA array interface as flat bytes, so torch.as_tensor(buf, device=...).view(torch.int64) wraps
    one without a copy."""

    def __init__(self, barcodes, indptr, indices, data, n_rows, nnz):
        self.barcodes, self.indptr, self.indices, self.data, self.n_rows, self.nnz = barcodes, indptr, indices, data, n_rows, nnz

    def download(self):
        """-> (barcodes, indptr, indices, data) as numpy u64 arrays."""
        e = np.empty(0, np.uint64)
        if self.nnz == 0:
            return e, np.zeros(1, np.uint64), e.copy(), e.copy()
        return (self.barcodes.download(np.uint64, self.n_rows), self.indptr.download(np.uint64, self.n_rows + 1),
                self.indices.download(np.uint64, self.nnz), self.data.download(np.uint64, self.nnz))

    def free(self):
        for b in (self.barcodes, self.indptr, self.indices, self.data):
            if b is not None:
                b.free()


class RowTop:
    """What ibu_matrix_row_top leaves, on the device (Context.matrix_row_top): five DeviceBuffers of n_rows u64 — per row of the
    entry table `top_key` (the feature of the first entry with the largest value; NO_KEY where no entry took part), `top_value`,
    `next_value` (the largest value among the other entries), `row_sum` (modulo 2^64) and `row_entries`."""

    def __init__(self, top_key, top_value, next_value, row_sum, row_entries, n_rows):
        self.top_key, self.top_value, self.next_value, self.row_sum, self.row_entries, self.n_rows = (
            top_key, top_value, next_value, row_sum, row_entries, n_rows)

    def _buffers(self):
        return self.top_key, self.top_value, self.next_value, self.row_sum, self.row_entries

    def download(self):
        """-> (top_key, top_value, next_value, row_sum, row_entries) as numpy u64 arrays."""
        if self.n_rows == 0:
            return tuple(np.empty(0, np.uint64) for _ in range(5))
        return tuple(b.download(np.uint64, self.n_rows) for b in self._buffers())

    def free(self):
        for b in self._buffers():
            if b is not None:
                b.free()


class DeviceBatch:
    """One device-resident batch of a DeviceStream: `n` AoS records at device pointer `ptr` (a ring slot), the first of them
    record number `first_index` of the stream.  release() (or leaving the `with` block) gives the slot back: it is refilled once
    the work queued so far on `stream` (default: the context's) has run."""

    def __init__(self, stream, ptr, n, first_index):
        self._s, self.ptr, self.n, self.first_index, self.nbytes = stream, ptr, n, first_index, n * RECORD_SIZE

    def download(self):
        """The batch as a host REC_DTYPE array (synchronises the context's stream)."""
        return DeviceBuffer.wrap(self._s.ctx, self.ptr, self.nbytes).download().view(REC_DTYPE)

    def release(self, stream=None):
        if self.ptr:
            p, self.ptr = self.ptr, 0
            _check(lib.ibu_stream_release(self._s._s, p, stream))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.release()


class DeviceStream:
    """ibu_stream_t — the device form of `Reader::read_batch` + `Iterator` (reader.rs:218-242, :279-306) and of the per-batch loop
    of process_parallel (mmap.rs:312-320): iterate to pull one DeviceBatch at a time, run any kernels on it, release it.
    A source error (TruncatedRecord, Io, Niffler ...) is raised by the iteration after the batches in front of it."""

    @classmethod
    def _open(cls, call, ctx, source):
        out = C.c_void_p()
        _check(call(C.byref(out)))
        s = cls.__new__(cls)
        s._s, s.ctx, s._source = out, ctx, source   # the source (Reader / MmapReader) must outlive the stream:
        if not hasattr(source, "_streams"):         # closing the source closes the streams still open on it first
            source._streams = weakref.WeakSet()
        source._streams.add(s)
        return s

    @classmethod
    def from_path(cls, path, ctx, ring=None):
        """`Reader::from_path` + the stream (ibu_stream_open_path), as a context manager that owns its source: a BGZF file the device
        load takes is read in ranges whose blocks are inflated on the device, anything else goes through the Reader of the same
        descriptor.  The same iteration and DeviceBatch as Reader.device_stream."""
        out = C.c_void_p()
        _check(lib.ibu_stream_open_path(str(path).encode(), ctx._c, _ring(ring), C.byref(out)))
        s = cls.__new__(cls)
        s._s, s.ctx, s._source = out, ctx, None
        return s

    def header(self):
        h = CHeader()
        _check(lib.ibu_stream_header(self._s, C.byref(h)))
        return Header._wrap(h)

    def next_batch(self, stream=None):
        """-> DeviceBatch, or None at the end of the stream.  `stream`: the stream the batch will be read on (None: the context's)."""
        p, n, first = C.c_void_p(), C.c_size_t(), C.c_uint64()
        _check(lib.ibu_stream_next(self._s, stream, C.byref(p), C.byref(n), C.byref(first)))
        if n.value == 0:
            return None
        return DeviceBatch(self, p.value, n.value, first.value)

    def __iter__(self):
        return self

    def __next__(self):
        b = self.next_batch()
        if b is None:
            raise StopIteration
        return b

    def stats(self):
        st = CStreamStats()
        _check(lib.ibu_stream_stats(self._s, C.byref(st)))
        return st

    def close(self):
        if getattr(self, "_s", None):
            lib.ibu_stream_close(self._s)
            self._s = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


INFLATE_BLOCK_DTYPE = np.dtype([("comp_offset", "<u8"), ("out_offset", "<i8"), ("comp_len", "<u4"), ("out_len", "<u4"), ("crc32", "<u4"),
                                ("reserved", "<u4")])   # ibu_inflate_block_t


def bgzf_scan(buf, final=True, cap=None):
    """ibu_bgzf_scan over `buf` (bytes-like): (ctypes array of ibu_inflate_block_t, consumed bytes, uncompressed bytes, status).
    status is 0 or 2 = IBU_ERR_NIFFLER (the blocks in front of the bad spot are described).  cap: at most that many blocks."""
    from ._lib import CInflateBlock
    a = np.frombuffer(buf, dtype=np.uint8)
    step = 1 << 16
    tmp = (CInflateBlock * step)()
    parts, pos, total, rc, left = [], 0, 0, 0, (None if cap is None else int(cap))
    while pos < len(a) and (left is None or left > 0):
        n, consumed, out_bytes = C.c_size_t(), C.c_size_t(), C.c_uint64()
        want = step if left is None else min(step, left)
        rc = lib.ibu_bgzf_scan(_hptr(a[pos:]), len(a) - pos, 1 if final else 0, tmp, want, C.byref(n), C.byref(consumed), C.byref(out_bytes))
        if n.value:
            part = np.frombuffer(tmp, dtype=INFLATE_BLOCK_DTYPE, count=n.value).copy()
            part["comp_offset"] += pos
            part["out_offset"] += total
            parts.append(part)
            if left is not None:
                left -= n.value
        pos += consumed.value
        total += out_bytes.value
        if rc or consumed.value == 0 or n.value < want:
            break
    allb = np.concatenate(parts) if parts else np.empty(0, INFLATE_BLOCK_DTYPE)
    blocks = (CInflateBlock * len(allb)).from_buffer_copy(allb.tobytes()) if len(allb) else (CInflateBlock * 0)()
    return blocks, pos, total, rc


def numa_of_pci(pci_bus_id, sysfs_root=None):
    """(node, cpulist, usable_cpus) of a PCI function from a sysfs tree (ibu_numa_of_pci); node -1 = the platform does not say."""
    node, usable, buf = C.c_int32(), C.c_int32(), C.create_string_buffer(256)
    _check(lib.ibu_numa_of_pci(None if sysfs_root is None else str(sysfs_root).encode(), str(pci_bus_id).encode(), C.byref(node),
                               buf, 256, C.byref(usable)))
    return node.value, buf.value.decode(), usable.value


def sample_threshold(fraction):
    """The threshold of ibu_subsample_class / ibu_saturation_curve that keeps `fraction` of the reads, exactly: all ones for a
    fraction of 1 or more, otherwise the floor of fraction * 2^64.  fraction: a float, an int or a fractions.Fraction."""
    from fractions import Fraction
    if fraction != fraction or fraction < 0:
        raise ValueError("the fraction must be a number >= 0")
    if fraction >= 1:
        return (1 << 64) - 1
    return int(Fraction(fraction) * (1 << 64))            # (Fraction of a float is exact, int() of a positive Fraction its floor)


def _u64_arg(name, v):
    if not 0 <= v < 1 << 64:
        raise ValueError(f"{name} must fit an unsigned 64-bit integer")
    return int(v)


def _u32_arg(name, v):
    if not 0 <= v < 1 << 32:
        raise ValueError(f"{name} must fit an unsigned 32-bit integer")
    return int(v)


def _one_threshold(fraction, threshold):
    if (fraction is None) == (threshold is None):
        raise ValueError("exactly one of fraction and threshold must be given")
    return sample_threshold(fraction) if threshold is None else _u64_arg("threshold", threshold)


def feature_bitmap_words(values, n_bits):
    """The bitmap ibu_barcode_metrics / ibu_filter_barcodes read as a feature set, as numpy u64 words: bit v & 63 of word v >> 6
    is set for every v in `values` (integers in [0, n_bits)); (n_bits + 63) // 64 words, at least one."""
    n_bits = int(n_bits)
    if not 0 <= n_bits <= 1 << 32:
        raise ValueError("n_bits must be in 0 .. 2^32")
    v = np.asarray(values, dtype=np.uint64).ravel()
    if len(v) and int(v.max()) >= n_bits:
        raise ValueError("a value is not below n_bits")
    words = np.zeros(max((n_bits + 63) // 64, 1), np.uint64)
    np.bitwise_or.at(words, (v >> np.uint64(6)).astype(np.int64), np.uint64(1) << (v & np.uint64(63)))
    return words


def _feature_set(feature_set):
    """None | (device bitmap, n_bits) -> (c_void_p | None, n_bits)."""
    if feature_set is None:
        return None, 0
    d_set, bits = feature_set
    return _dptr(d_set), _u64_arg("n_bits", bits)


class Context:
    """ibu_ctx_t: one per host thread and GPU.  Every method launches asynchronously on
    `stream` (default: the context's own stream) unless it says it synchronises."""

    def __init__(self, device=0):
        c = C.c_void_p()
        _check(lib.ibu_ctx_create(device, C.byref(c)))
        self._c = c
        self._buffers = weakref.WeakSet()   # live DeviceBuffers allocated through this context
        self._whitelists = weakref.WeakSet()   # live Whitelists built on it

    @property
    def stream(self):
        return lib.ibu_ctx_stream(self._c)

    def synchronize(self, stream=None):
        _check(lib.ibu_ctx_synchronize(self._c, stream))

    def set_option(self, key, value):
        _check(lib.ibu_ctx_set_option(self._c, key.encode(), int(value)))

    def numa(self):
        """Where the device hangs off the host and where the pinned ring landed (ibu_ctx_numa)."""
        i = CNumaInfo()
        _check(lib.ibu_ctx_numa(self._c, C.byref(i)))
        return {"mode": i.mode, "node": i.node, "usable_cpus": i.usable_cpus, "ring_node": i.ring_node,
                "ring_placed": bool(i.ring_placed), "pci_bus_id": i.pci_bus_id.decode(), "cpulist": i.cpulist.decode()}

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def alloc_probed(self, nbytes, tries):
        """ibu_device_alloc_probed: up to `tries` candidate allocations (all held at once), the one a write + read streams
        over fastest is kept, the others freed.  -> (DeviceBuffer, {"tries", "chosen", "ms": [...]})."""
        p, rep = C.c_void_p(), CAllocProbe()
        _check(lib.ibu_device_alloc_probed(self._c, int(nbytes), int(tries), C.byref(p), C.byref(rep)))
        b = DeviceBuffer.wrap(self, p.value, nbytes)
        b.owned = True
        self._buffers.add(b)
        return b, {"tries": rep.tries, "chosen": rep.chosen, "ms": [round(float(rep.ms[k]), 4) for k in range(rep.tries)]}

    def upload(self, host):
        a = np.ascontiguousarray(host)
        return DeviceBuffer(self, max(a.nbytes, 16)).upload(a)

    # K1 / K1'
    def deserialize(self, d_records, n, d_barcode, d_umi, d_index, stream=None):
        _check(lib.ibu_deserialize(self._c, _dptr(d_records), n, _dptr(d_barcode), _dptr(d_umi), _dptr(d_index), stream))

    def serialize(self, d_barcode, d_umi, d_index, n, d_records, stream=None):
        _check(lib.ibu_serialize(self._c, _dptr(d_barcode), _dptr(d_umi), _dptr(d_index), n, _dptr(d_records), stream))

    # column codec
    def unpack_2bit(self, d_codes, n, length, d_ascii, stream=None):
        _check(lib.ibu_unpack_2bit(self._c, _dptr(d_codes), n, length, _dptr(d_ascii), stream))

    def pack_2bit(self, d_ascii, n, length, d_codes, stream=None):
        _check(lib.ibu_pack_2bit(self._c, _dptr(d_ascii), n, length, _dptr(d_codes), stream))

    # K2 / K3
    def decode_ascii(self, d_records, n, bc_len, umi_len, d_bc, d_umi, d_index, stream=None):
        _check(lib.ibu_decode_ascii(self._c, _dptr(d_records), n, bc_len, umi_len, _dptr(d_bc), _dptr(d_umi),
                                    _dptr(d_index), stream))

    def encode_ascii(self, d_bc, d_umi, d_index, n, bc_len, umi_len, d_records, first_index=0, stream=None):
        _check(lib.ibu_encode_ascii(self._c, _dptr(d_bc), _dptr(d_umi), _dptr(d_index), first_index, n, bc_len,
                                    umi_len, _dptr(d_records), stream))

    def codec_status(self, stream=None):
        """Synchronises; raises IbuError(InvalidBase) if any pack/encode since the last call saw a bad byte."""
        fb, nb = C.c_uint64(), C.c_uint64()
        _check(lib.ibu_codec_status(self._c, stream, C.byref(fb), C.byref(nb)))

    # K4
    def reduce(self, d_records, n, stream=None, reset=True, fetch=True):
        if reset:
            _check(lib.ibu_reduce_reset(self._c, stream))
        _check(lib.ibu_reduce(self._c, _dptr(d_records), n, stream))
        return self.reduce_fetch(stream) if fetch else None

    def reduce_fetch(self, stream=None):
        r = CReduceResult()
        _check(lib.ibu_reduce_fetch(self._c, stream, C.byref(r)))
        return {"count": r.count, "sum": list(r.sum), "xor": list(r.xor_)}

    def generate(self, seed, first, n, bc_len, umi_len, d_records, stream=None):
        _check(lib.ibu_generate(self._c, seed, first, n, bc_len, umi_len, _dptr(d_records), stream))

    def copy(self, d_dst, d_src, nbytes, stream=None):
        _check(lib.ibu_device_copy(self._c, _dptr(d_dst), _dptr(d_src), nbytes, stream))

    def sort_records(self, d_records, d_tmp, n, stream=None):
        _check(lib.ibu_sort_records(self._c, _dptr(d_records), _dptr(d_tmp), n, stream))

    def merge_sorted(self, d_a, na, d_b, nb, d_out=None, source=False, stream=None):
        """ibu_merge_sorted: the stable merge of two sorted record arrays (equal records: those of d_a first) ->
        (d_out, d_source | None).  d_out: (na + nb) * 24 bytes that overlap neither input, allocated when None; source:
        True allocates, or a DeviceBuffer receives, one byte per output record (0 = from d_a, 1 = from d_b).
        Asynchronous on `stream`."""
        n = na + nb
        if d_out is None:
            d_out = self.alloc(max(24 * n, 1))
        d_source = self.alloc(max(n, 1)) if source is True else (source or None)
        _check(lib.ibu_merge_sorted(self._c, _dptr(d_a), na, _dptr(d_b), nb, _dptr(d_out), _dptr(d_source), stream))
        return d_out, d_source

    def merge_sorted_runs(self, d_records, d_tmp, run_lengths, stream=None):
        """ibu_merge_sorted_runs: d_records = consecutive sorted runs of these lengths -> all of them sorted, in place
        (what sort_records gives); d_tmp: as many bytes of scratch.  Asynchronous on `stream`."""
        lengths = (C.c_size_t * max(len(run_lengths), 1))(*[int(x) for x in run_lengths])
        _check(lib.ibu_merge_sorted_runs(self._c, _dptr(d_records), _dptr(d_tmp), lengths, len(run_lengths), stream))

    @staticmethod
    def sort_records_contexts(ctxs, shards):
        """The sort over several shards, one per context (= per GPU), in one call (ibu_sort_records_contexts): shards =
        [(d_records, d_tmp, n, capacity_in_records), ...]; returns the new record counts — shard i holds the i-th
        contiguous range of the global order."""
        if len(shards) != len(ctxs):   # the C side reads n_ctxs entries of both arrays
            raise ValueError(f"{len(ctxs)} contexts but {len(shards)} shards")
        arr = (C.c_void_p * len(ctxs))(*[c._c for c in ctxs])
        sh = (_lib.CSortShard * len(shards))()
        for k, (r, t, n, cap) in enumerate(shards):
            sh[k].d_records, sh[k].d_tmp, sh[k].n, sh[k].capacity = _dptr(r).value, _dptr(t).value, n, cap
        _check(lib.ibu_sort_records_contexts(arr, len(ctxs), sh))
        return [int(x.n) for x in sh]

    def barcode_counts(self, d_sorted_records, n, unique_umis=True, stream=None):
        """BarcodeAnalyzer (parallel.rs:72-98) on sorted device records ->
        (barcodes, counts, unique_umis | None) as numpy u64 arrays in ascending barcode order."""
        nb, npairs = C.c_size_t(), C.c_size_t()
        _check(lib.ibu_barcode_counts(self._c, _dptr(d_sorted_records), n, None, None, None, 0, C.byref(nb),
                                      C.byref(npairs), stream))
        u = nb.value
        if u == 0:
            e = np.empty(0, np.uint64)
            return e, e.copy(), (e.copy() if unique_umis else None)
        d_b, d_c = self.alloc(8 * u), self.alloc(8 * u)
        d_u = self.alloc(8 * u) if unique_umis else None
        _check(lib.ibu_barcode_counts(self._c, _dptr(d_sorted_records), n, _dptr(d_b), _dptr(d_c), _dptr(d_u), u,
                                      C.byref(nb), C.byref(npairs), stream))
        self.synchronize(stream)
        return (d_b.download(np.uint64), d_c.download(np.uint64), d_u.download(np.uint64) if d_u else None)

    # count matrix: reads and distinct UMIs per (barcode, index) pair
    def swap_umi_index(self, d_src, d_dst, n, stream=None):
        """ibu_records_swap_umi_index: record i of d_dst = {barcode, index, umi} of record i of d_src (its own inverse).
        d_dst may be d_src (in place); asynchronous on `stream`."""
        _check(lib.ibu_records_swap_umi_index(self._c, _dptr(d_src), _dptr(d_dst), n, stream))

    def pair_counts(self, d_sorted_records, n, distinct_third=True, stream=None):
        """ibu_pair_counts: one entry per maximal run of records with equal first and second words ->
        (first, second, records_per_pair, distinct_third | None) as numpy u64 arrays in input order.  On records that went
        through swap_umi_index and sort_records: the count matrix in COO form (barcode, index, reads, distinct UMIs); on
        ordinarily sorted records: the molecules (barcode, umi, reads, distinct indices)."""
        npairs, ntriples = C.c_size_t(), C.c_size_t()
        _check(lib.ibu_pair_counts(self._c, _dptr(d_sorted_records), n, None, None, None, None, 0, C.byref(npairs),
                                   C.byref(ntriples), stream))
        u = npairs.value
        if u == 0:
            e = np.empty(0, np.uint64)
            return e, e.copy(), e.copy(), (e.copy() if distinct_third else None)
        outs = [self.alloc(8 * u) for _ in range(3)] + [self.alloc(8 * u) if distinct_third else None]
        _check(lib.ibu_pair_counts(self._c, _dptr(d_sorted_records), n, *[_dptr(o) for o in outs], u, C.byref(npairs),
                                   C.byref(ntriples), stream))
        self.synchronize(stream)
        return tuple(o.download(np.uint64) if o else None for o in outs)

    def count_matrix(self, d_records, d_tmp, n, cap=None, leave_swapped=False, stream=None):
        """ibu_count_matrix over n device records in any order (d_tmp: 24 n bytes of scratch) ->
        (barcodes, indices, reads, umis) as numpy u64 arrays, ascending by (barcode, index): the count matrix in COO form.
        On return the records are ordered by (barcode, index, umi), with their fields in place unless leave_swapped.
        cap: a bound on the number of entries (default n, which always fits)."""
        if n == 0:
            e = np.empty(0, np.uint64)
            return e, e.copy(), e.copy(), e.copy()
        cap = n if cap is None else cap
        outs = [self.alloc(max(8 * cap, 16)) for _ in range(4)]
        ne, nm = C.c_size_t(), C.c_size_t()
        _check(lib.ibu_count_matrix(self._c, _dptr(d_records), _dptr(d_tmp), n, COUNT_LEAVE_SWAPPED if leave_swapped else 0,
                                    *[_dptr(o) for o in outs], cap, C.byref(ne), C.byref(nm), stream))
        self.synchronize(stream)
        return tuple(o.download(np.uint64, count=ne.value) for o in outs)

    # matrix export: CSR row structure and Matrix Market text from the entry table
    def matrix_rows(self, d_first, n_entries, ordinals=True, stream=None):
        """ibu_matrix_rows over a device column of n_entries u64 (the barcodes of the entry table): a row is a maximal run of equal
        values -> MatrixRows(n_rows, d_keys, d_ptr, d_row_of_entry), DeviceBuffers of u64: the value of every row, the CSR indptr
        (n_rows + 1 words, the last n_entries) and, with ordinals, the 0-based row of every entry.  Synchronises once."""
        nr = C.c_size_t()
        _check(lib.ibu_matrix_rows(self._c, _dptr(d_first), n_entries, None, None, None, 0, C.byref(nr), stream))
        r = nr.value
        d_keys, d_ptr = self.alloc(max(8 * r, 16)), self.alloc(8 * (r + 1) + 8)
        d_ord = self.alloc(max(8 * n_entries, 16)) if ordinals else None
        if n_entries == 0:
            d_ptr.upload(np.zeros(1, np.uint64))                 # the call touches nothing: indptr of no rows is [0]
        _check(lib.ibu_matrix_rows(self._c, _dptr(d_first), n_entries, _dptr(d_ord), _dptr(d_keys), _dptr(d_ptr), r, C.byref(nr), stream))
        return MatrixRows(r, d_keys, d_ptr, d_ord)

    def matrix_market_body(self, d_a, d_b, d_c, n_entries, add=(1, 1), stream=None):
        """ibu_matrix_market_body: three device columns of n_entries u64 as decimal text, line k = "a[k]+add[0] b[k]+add[1] c[k]\\n"
        (sums modulo 2^64) -> (DeviceBuffer holding the text, n_bytes, maxima): maxima = the largest printed value of each column.
        Two calls, the size query and the write: the columns are read three times.  Synchronises."""
        add_a, add_b = (_u64_arg("add", v) for v in add)
        cols = [_dptr(d_a), _dptr(d_b), _dptr(d_c)]
        nb, mx = C.c_size_t(), (C.c_uint64 * 3)()
        _check(lib.ibu_matrix_market_body(self._c, *cols, n_entries, add_a, add_b, None, 0, C.byref(nb), mx, stream))
        d_text = self.alloc(max(nb.value, 16))
        _check(lib.ibu_matrix_market_body(self._c, *cols, n_entries, add_a, add_b, _dptr(d_text), nb.value, C.byref(nb), mx, stream))
        return d_text, nb.value, tuple(int(x) for x in mx)

    def _entry_columns(self, d_records, n, stream):
        """ibu_pair_counts into device columns -> ([first, second, records_per_pair, distinct_third], entries)."""
        npairs = C.c_size_t()
        _check(lib.ibu_pair_counts(self._c, _dptr(d_records), n, None, None, None, None, 0, C.byref(npairs), None, stream))
        u = npairs.value
        cols = [self.alloc(max(8 * u, 16)) for _ in range(4)]
        _check(lib.ibu_pair_counts(self._c, _dptr(d_records), n, *[_dptr(c) for c in cols], u, C.byref(npairs), None, stream))
        return cols, u

    @staticmethod
    def _values_column(values):
        if values not in ("umis", "reads"):
            raise ValueError('values must be "umis" or "reads"')
        return 3 if values == "umis" else 2

    def matrix_csr(self, d_records, n, values="umis", stream=None):
        """The count matrix of the {barcode, index, umi} records count_matrix(leave_swapped=True) leaves (or what a chain of filters
        and select_records kept of them), as a CsrMatrix on the device: ibu_pair_counts into device columns, then ibu_matrix_rows.
        values: "umis" (distinct UMIs per entry) or "reads".  Nothing is downloaded; CsrMatrix.download() gives numpy arrays."""
        which = self._values_column(values)
        cols, nnz = self._entry_columns(d_records, n, stream)
        rows = self.matrix_rows(cols[0], nnz, ordinals=False, stream=stream)
        self.synchronize(stream)
        for k in (0, 5 - which):
            cols[k].free()
        return CsrMatrix(rows.d_keys, rows.d_ptr, cols[1], cols[which], rows.n_rows, nnz)

    # the dominant feature of every row: per-row top-2 of the entry table, and the class made from it
    def matrix_row_top(self, d_first, d_second, d_values, n_entries, feature_set=None, stream=None):
        """ibu_matrix_row_top over three device columns of n_entries u64 (the barcodes, the feature numbers and a count column of
        the entry table): per row — a maximal run of equal d_first — the largest value, the feature of the first entry that holds
        it, the largest value among the other entries, the sum modulo 2^64 and the number of entries, over the entries whose
        feature is in feature_set (what feature_bitmap returned; None: all entries) -> RowTop, on the device.  A row in which
        nothing takes part has NO_KEY, 0, 0, 0, 0.  Two calls, the size query and the write; synchronises once each."""
        d_set, bits = _feature_set(feature_set)
        cols = [_dptr(d_first), _dptr(d_second), _dptr(d_values)]
        nr = C.c_size_t()
        _check(lib.ibu_matrix_row_top(self._c, *cols, n_entries, d_set, bits, None, None, None, None, None, 0, C.byref(nr), stream))
        r = nr.value
        outs = [self.alloc(max(8 * r, 16)) for _ in range(5)]
        _check(lib.ibu_matrix_row_top(self._c, *cols, n_entries, d_set, bits, *[_dptr(o) for o in outs], r, C.byref(nr), stream))
        return RowTop(*outs, r)

    def assign_rows(self, row_top, min_value=1, min_share=(0, 1), d_class=None, counts=True, stream=None):
        """ibu_assign_rows over the columns of a RowTop: one class byte per row — ROW_NONE where the top value is below
        max(min_value, 1), else ROW_ASSIGNED where it is above the runner-up and holds at least min_share = (num, den) of the row
        sum (top * den >= num * sum in exact integers, equality passes; num = 0: no share test), else ROW_MIXED.
        -> (d_class, AssignCounts).  d_class: n_rows bytes of device memory; None allocates them, False asks for the totals only
        (and returns None in its place).  counts=False returns None for the totals and does not wait for them."""
        num, den = min_share
        rule = CAssignRule(_u64_arg("min_value", min_value), _u64_arg("min_share", num), _u64_arg("min_share", den))
        if d_class is None:
            d_class = self.alloc(max(row_top.n_rows, 16))
        elif d_class is False:
            d_class = None
        c = CAssignCounts() if counts else None
        _check(lib.ibu_assign_rows(self._c, _dptr(row_top.top_value), _dptr(row_top.next_value), _dptr(row_top.row_sum), row_top.n_rows,
                                   C.byref(rule), _dptr(d_class), C.byref(c) if counts else None, stream))
        return d_class, (AssignCounts(*[int(getattr(c, f)) for f in AssignCounts._fields]) if counts else None)

    def assign_features(self, d_records, n, feature_set=None, values="umis", stream=None, **rule):
        """The dominant feature of every barcode of the {barcode, index, umi} records count_matrix(leave_swapped=True) leaves (or
        what a chain of filters and select_records kept of them): ibu_pair_counts into device columns, the row barcodes
        (ibu_matrix_rows, keys only), matrix_row_top over the features in feature_set, assign_rows with **rule (min_value,
        min_share) -> (d_barcodes, RowTop, d_class, AssignCounts): row r is barcode d_barcodes[r] (a DeviceBuffer of n_rows u64).
        values: "umis" (distinct UMIs per entry) or "reads".  Nothing but the totals is downloaded."""
        which = self._values_column(values)
        cols, nnz = self._entry_columns(d_records, n, stream)
        nr = C.c_size_t()
        _check(lib.ibu_matrix_rows(self._c, _dptr(cols[0]), nnz, None, None, None, 0, C.byref(nr), stream))
        d_keys = self.alloc(max(8 * nr.value, 16))
        _check(lib.ibu_matrix_rows(self._c, _dptr(cols[0]), nnz, None, _dptr(d_keys), None, nr.value, C.byref(nr), stream))
        top = self.matrix_row_top(cols[0], cols[1], cols[which], nnz, feature_set, stream)
        d_class, counts = self.assign_rows(top, stream=stream, **rule)
        self.synchronize(stream)
        for c in cols:
            c.free()
        return d_keys, top, d_class, counts

    def write_matrix_market(self, directory, d_records, n, n_features, bc_len, values="umis", barcode_suffix="", feature_names=None,
                            stream=None, piece_bytes=64 << 20):
        """The 10x directory of the same records: matrix.mtx (features x barcodes, 1-based, the body formatted on the device by
        ibu_matrix_market_body), barcodes.tsv (ibu_unpack_2bit of the row keys, each followed by barcode_suffix) and features.tsv
        ("id\\tname\\tGene Expression": the decimal feature number for both unless feature_names gives n_features names) — what
        scanpy.read_10x_mtx and Seurat's Read10X read.  An index that is not below n_features raises ValueError before any file is
        created.  The text comes down in pieces of piece_bytes.  -> (n_rows, nnz).  Synchronises."""
        import os
        which = self._values_column(values)
        n_features = _u64_arg("n_features", n_features)
        if not 1 <= bc_len <= 32:
            raise ValueError("bc_len must be in 1 .. 32")
        if feature_names is not None and len(feature_names) != n_features:
            raise ValueError("feature_names must hold n_features names")
        cols, nnz = self._entry_columns(d_records, n, stream)
        rows = self.matrix_rows(cols[0], nnz, stream=stream)
        trio = [_dptr(cols[1]), _dptr(rows.d_row_of_entry), _dptr(cols[which])]
        # the size query on the values as they stand: the largest index comes back unwrapped, and adding one to the first two
        # columns lengthens a line by at most two bytes
        nb, mx = C.c_size_t(), (C.c_uint64 * 3)()
        _check(lib.ibu_matrix_market_body(self._c, *trio, nnz, 0, 0, None, 0, C.byref(nb), mx, stream))
        if nnz and int(mx[0]) >= n_features:
            raise ValueError(f"the records hold index {int(mx[0])}, which is not below n_features = {n_features}")
        cap = nb.value + 2 * nnz
        d_text = self.alloc(max(cap, 16))
        _check(lib.ibu_matrix_market_body(self._c, *trio, nnz, 1, 1, _dptr(d_text), cap, C.byref(nb), None, stream))
        d_ascii = self.alloc(max(rows.n_rows * bc_len, 16))
        self.unpack_2bit(rows.d_keys, rows.n_rows, bc_len, d_ascii, stream)
        self.synchronize(stream)
        os.makedirs(directory, exist_ok=True)
        with open(os.path.join(directory, "matrix.mtx"), "wb") as f:
            f.write(f"{MTX_BANNER}\n{n_features} {rows.n_rows} {nnz}\n".encode())
            for off in range(0, nb.value, piece_bytes):
                f.write(d_text.download(np.uint8, min(piece_bytes, nb.value - off), off).tobytes())
        tail = np.frombuffer(barcode_suffix.encode() + b"\n", np.uint8)
        per = max(1, piece_bytes // (bc_len + len(tail)))
        with open(os.path.join(directory, "barcodes.tsv"), "wb") as f:
            for r0 in range(0, rows.n_rows, per):
                k = min(per, rows.n_rows - r0)
                text = d_ascii.download(np.uint8, k * bc_len, r0 * bc_len).reshape(k, bc_len)
                f.write(np.concatenate([text, np.broadcast_to(tail, (k, len(tail)))], axis=1).tobytes())
        with open(os.path.join(directory, "features.tsv"), "w") as f:
            for j in range(n_features):
                name = str(j) if feature_names is None else str(feature_names[j])
                f.write(f"{name}\t{name}\tGene Expression\n")
        for b in (*cols, rows.d_keys, rows.d_ptr, rows.d_row_of_entry, d_text, d_ascii):
            b.free()
        return rows.n_rows, nnz

    def classify_molecules(self, d_sorted_records, n, d_class=None, tie_first=False, counts=True, stream=None):
        """ibu_classify_molecules over n device records sorted by (barcode, umi, index): one class byte per record — MOLECULE_KEPT
        for the index its (barcode, umi) molecule was seen with strictly most often, MOLECULE_MINOR for the molecule's other
        reads, MOLECULE_TIED for all reads of a molecule whose top is shared (tie_first: the first index at the top is kept and
        the rest is minor instead).  -> (d_class, MoleculeCounts).  d_class: n bytes of device memory; None allocates them, False
        asks for the totals only (and returns None in its place).  counts=False returns None for the totals and does not wait
        for them.  select_records(d_records, d_class, n, keep_mask=1 << MOLECULE_KEPT) then drops the chimeric reads."""
        if d_class is None:
            d_class = self.alloc(max(n, 16))
        elif d_class is False:
            d_class = None
        c = CMoleculeCounts() if counts else None
        _check(lib.ibu_classify_molecules(self._c, _dptr(d_sorted_records), n, MOLECULES_TIE_FIRST if tie_first else 0,
                                          _dptr(d_class), C.byref(c) if counts else None, stream))
        return d_class, (MoleculeCounts(*[int(getattr(c, f)) for f in MoleculeCounts._fields]) if counts else None)

    def call_cells(self, d_sorted_records, n, *, min_umis=None, top=None, expected_cells=None, by_reads=False, d_class=None, counts=True,
                   stream=None):
        """ibu_call_cells over n sorted device records: one class byte per record — CELL where its barcode's UMI count (by_reads:
        its read count) reaches the threshold, CELL_BACKGROUND otherwise.  Exactly one of min_umis (the threshold itself), top (the
        K barcodes with the largest counts, and those tied with the K-th) and expected_cells (a tenth of the count at the 99th
        percentile of the top expected_cells barcodes) must be given.  -> (d_class, CellCounts).  d_class: n bytes of device
        memory; None allocates them, False asks for the totals only (and returns None in its place).  counts=False returns None
        for the totals and does not wait for them.  select_records(d_records, d_class, n, keep_mask=1 << CELL) then keeps the
        records of the cells."""
        given = [(m, p) for m, p in ((CELLS_MIN, min_umis), (CELLS_TOP, top), (CELLS_ORDMAG, expected_cells)) if p is not None]
        if len(given) != 1:
            raise ValueError("exactly one of min_umis, top and expected_cells must be given")
        mode, param = given[0]
        if param < 0 or param >= 1 << 64:
            raise ValueError("the parameter must fit an unsigned 64-bit integer")
        if d_class is None:
            d_class = self.alloc(max(n, 16))
        elif d_class is False:
            d_class = None
        c = CCellCounts() if counts else None
        _check(lib.ibu_call_cells(self._c, _dptr(d_sorted_records), n, mode, param, CELLS_BY_READS if by_reads else 0, _dptr(d_class),
                                  C.byref(c) if counts else None, stream))
        return d_class, (CellCounts(*[int(getattr(c, f)) for f in CellCounts._fields]) if counts else None)

    # per-barcode QC metrics and the barcode filter
    def feature_bitmap(self, values, n_bits):
        """A feature set for barcode_metrics / filter_barcodes: the bitmap of n_bits bits (at most 2^32) with the bits `values`
        set (integers in [0, n_bits); bit v is bit v & 63 of u64 word v >> 6), built in numpy and uploaded -> (DeviceBuffer, n_bits)."""
        return self.upload(feature_bitmap_words(values, n_bits)), int(n_bits)

    def barcode_metrics(self, d_records, n, feature_set=None, set_word=1, stream=None):
        """ibu_barcode_metrics over n device records: one row per barcode (maximal run of equal first word), in input order ->
        BarcodeMetrics(barcodes, reads, pairs, triples, set_reads, set_triples) as numpy u64 columns: the barcode, its records,
        the runs of equal (w0, w1) and of equal (w0, w1, w2) that begin in it, and its records / triples whose word set_word (1 or
        2) is in feature_set (what feature_bitmap returned; None: nothing is).  On records that went through swap_umi_index and
        sort_records (what count_matrix(leave_swapped=True) leaves), with set_word=1: pairs are the features detected, triples
        the UMIs, set_triples the UMIs in the set.  On ordinarily sorted records, with set_word=2: pairs = triples = UMIs."""
        d_set, bits = _feature_set(feature_set)
        nb = C.c_size_t()
        _check(lib.ibu_barcode_metrics(self._c, _dptr(d_records), n, d_set, bits, set_word, None, None, None, None, None, None, 0,
                                       C.byref(nb), stream))
        u = nb.value
        if u == 0:
            return BarcodeMetrics(*[np.empty(0, np.uint64) for _ in range(6)])
        outs = [self.alloc(max(8 * u, 16)) for _ in range(6)]
        _check(lib.ibu_barcode_metrics(self._c, _dptr(d_records), n, d_set, bits, set_word, *[_dptr(o) for o in outs], u, C.byref(nb), stream))
        self.synchronize(stream)
        return BarcodeMetrics(*[o.download(np.uint64, count=u) for o in outs])

    def filter_barcodes(self, d_records, n, feature_set=None, set_word=1, *, min_reads=0, max_reads=0, min_pairs=0, max_pairs=0,
                        min_triples=0, max_triples=0, max_set_fraction=None, set_of="reads", d_class=None, counts=True, stream=None):
        """ibu_filter_barcodes over n device records: one class byte per record, the class of its barcode — BARCODE_LOW where its
        reads, pairs or triples (as barcode_metrics counts them) are below their minimum, else BARCODE_HIGH where one is above its
        maximum (0: no maximum), else BARCODE_SET where its share in feature_set is above max_set_fraction = (num, den) —
        set_x * den > num * x in integers, x the reads or (set_of="triples") the triples; equality passes — else BARCODE_PASS.
        -> (d_class, BarcodeFilterCounts).  d_class: n bytes of device memory; None allocates them, False asks for the totals only
        (and returns None in its place).  counts=False returns None for the totals and does not wait for them.
        select_records(d_records, d_class, n, keep_mask=1 << BARCODE_PASS) then keeps the passing barcodes."""
        if set_of not in ("reads", "triples"):
            raise ValueError('set_of must be "reads" or "triples"')
        num, den = (0, 0) if max_set_fraction is None else max_set_fraction
        for name, v in (("min_reads", min_reads), ("max_reads", max_reads), ("min_pairs", min_pairs), ("max_pairs", max_pairs),
                        ("min_triples", min_triples), ("max_triples", max_triples), ("max_set_fraction", num), ("max_set_fraction", den)):
            _u64_arg(name, v)
        if max_set_fraction is not None and not (0 < den < 1 << 24 and num <= den):
            raise ValueError("max_set_fraction = (num, den) wants num <= den and 0 < den < 2^24")
        d_set, bits = _feature_set(feature_set)
        lim = CBarcodeLimits(min_reads, max_reads, min_pairs, max_pairs, min_triples, max_triples, num, den, 1 if set_of == "triples" else 0, 0)
        if d_class is None:
            d_class = self.alloc(max(n, 16))
        elif d_class is False:
            d_class = None
        c = CBarcodeFilterCounts() if counts else None
        _check(lib.ibu_filter_barcodes(self._c, _dptr(d_records), n, d_set, bits, set_word, C.byref(lim), _dptr(d_class),
                                       C.byref(c) if counts else None, stream))
        if not counts:
            return d_class, None
        return d_class, BarcodeFilterCounts(int(c.barcodes), tuple(int(x) for x in c.barcodes_by_class), tuple(int(x) for x in c.reads_by_class),
                                            int(c.triples_passed), int(c.set_triples_passed))

    # per-feature metrics and the feature filter
    def feature_metrics(self, d_records, n, n_features, feature_word=1, accumulate_into=None, totals=True, stream=None):
        """ibu_feature_metrics over n device records: for every feature f < n_features (the value of a record's word feature_word)
        its reads, its UMIs (runs of equal (w0, w1, w2)) and, with feature_word=1, the cells it was seen in (runs of equal (w0, w1))
        -> FeatureTable(reads, umis, cells, n_features, totals): three DeviceBuffers of n_features u64 (cells is None with
        feature_word=2, for ordinarily sorted records) and totals = (reads, umis, cells in range, reads with f >= n_features) of
        this call.  feature_word=1 is for what count_matrix(leave_swapped=True) leaves.  accumulate_into: a FeatureTable of an
        earlier call — the counts are added on top of its columns (shards cut where a barcode begins, or several samples) and the
        same buffers come back.  totals=False returns None for the totals and leaves the call asynchronous."""
        n_features = int(n_features)
        if not 1 <= n_features <= 1 << 32:
            raise ValueError("n_features must be in 1 .. 2^32")
        if feature_word not in (1, 2):
            raise ValueError("feature_word must be 1 or 2")
        if accumulate_into is not None:
            if accumulate_into.n_features != n_features or (accumulate_into.cells is None) != (feature_word == 2):
                raise ValueError("accumulate_into is a table of another shape")
            cols = list(accumulate_into[:3])
        else:
            cols = [self.alloc(max(8 * n_features, 16)) for _ in range(3 if feature_word == 1 else 2)] + [None] * (feature_word - 1)
        t = (C.c_uint64 * 4)() if totals else None
        _check(lib.ibu_feature_metrics(self._c, _dptr(d_records), n, feature_word, n_features, FEATURE_ACCUMULATE if accumulate_into is not None else 0,
                                       *[_dptr(c) for c in cols], t, stream))
        return FeatureTable(*cols, n_features, tuple(int(x) for x in t) if totals else None)

    def filter_features(self, d_records, n, table, feature_word=1, *, min_reads=0, max_reads=0, min_umis=0, max_umis=0, min_cells=0,
                        max_cells=0, d_class=None, d_verdict=None, counts=True, stream=None):
        """ibu_filter_features over n device records with the columns of `table` (a FeatureTable, made on these records or on
        others — the called cells, say): feature f is FEATURE_LOW where its reads, umis or cells are below their minimum, else
        FEATURE_HIGH where one is above its maximum (0: no maximum), else FEATURE_PASS; every record gets the class of its
        feature, FEATURE_UNKNOWN where it is not below table.n_features.  -> (d_class, FeatureFilterCounts).  d_class: n bytes of
        device memory; None allocates them, False asks for the totals only (and returns None in its place).  d_verdict: a
        DeviceBuffer of n_features bytes that receives the per-feature verdicts.  counts=False returns None for the totals and does
        not wait for them.  select_records(d_records, d_class, n, keep_mask=1 << FEATURE_PASS) then keeps the kept features."""
        given = {"reads": (min_reads, max_reads), "umis": (min_umis, max_umis), "cells": (min_cells, max_cells)}
        for name, (lo, hi) in given.items():
            _u64_arg("min_" + name, lo), _u64_arg("max_" + name, hi)
            if hi and lo > hi:
                raise ValueError(f"min_{name} is above max_{name}")
            if getattr(table, name) is None and (lo or hi):
                raise ValueError(f"a limit on {name}, and the table has no such column")
        if feature_word not in (1, 2):
            raise ValueError("feature_word must be 1 or 2")
        lim = CFeatureLimits(min_reads, max_reads, min_umis, max_umis, min_cells, max_cells)
        if d_class is None:
            d_class = self.alloc(max(n, 16))
        elif d_class is False:
            d_class = None
        c = CFeatureFilterCounts() if counts else None
        _check(lib.ibu_filter_features(self._c, _dptr(d_records), n, feature_word, table.n_features, _dptr(table.reads), _dptr(table.umis),
                                       _dptr(table.cells), C.byref(lim), _dptr(d_class), _dptr(d_verdict), C.byref(c) if counts else None, stream))
        if not counts:
            return d_class, None
        return d_class, FeatureFilterCounts(tuple(int(x) for x in c.features_by_class), tuple(int(x) for x in c.reads_by_class))

    # read subsampling and the saturation curve
    def subsample_class(self, n, d_class=None, *, fraction=None, threshold=None, seed=0, first_row=0, count=True, stream=None):
        """ibu_subsample_class: one class byte for each of n rows — SAMPLE_KEPT where the row's number u(row) =
        splitmix64(splitmix64(seed) + first_row + row) is below the threshold, SAMPLE_DROPPED otherwise; no record is read, so the
        subset depends on the ORDER of the records it is applied to (apply it at one fixed stage, normally the sorted records).
        Exactly one of fraction (see sample_threshold) and threshold (a u64; all ones keeps everything) must be given.
        -> (d_class, n_kept).  d_class: n bytes of device memory; None allocates them, False asks for the count only (and returns
        None in its place).  count=False returns None for the count and leaves the call asynchronous.
        select_records(d_records, d_class, n, keep_mask=1 << SAMPLE_KEPT) then makes the subset."""
        t = _one_threshold(fraction, threshold)
        _u64_arg("seed", seed), _u64_arg("first_row", first_row)
        if d_class is False and not count:
            raise ValueError("d_class=False with count=False leaves nothing to do")
        if d_class is None:
            d_class = self.alloc(max(n, 16))
        elif d_class is False:
            d_class = None
        k = C.c_size_t() if count else None
        _check(lib.ibu_subsample_class(self._c, n, first_row, seed, t, _dptr(d_class), C.byref(k) if count else None, stream))
        return d_class, (k.value if count else None)

    def saturation_curve(self, d_sorted_records, n, *, fractions=None, thresholds=None, seed=0, first_row=0, stream=None):
        """ibu_saturation_curve over n sorted device records: what would have been seen at each depth, from one read of the
        records -> a list of SaturationPoint(threshold, reads, barcodes, molecules), one per depth: the reads kept at it, and the
        runs of equal barcode / of equal (barcode, umi) with at least one kept read.  1 - molecules / reads is the sequencing
        saturation at that depth.  Exactly one of fractions (each through sample_threshold) and thresholds (u64 values) must be
        given: 1 .. 32 of them, non-decreasing.  seed / first_row as in subsample_class: the reads kept at a depth are the ones
        subsample_class keeps at the same threshold."""
        if (fractions is None) == (thresholds is None):
            raise ValueError("exactly one of fractions and thresholds must be given")
        ts = [sample_threshold(f) for f in fractions] if thresholds is None else [_u64_arg("threshold", t) for t in thresholds]
        if not 1 <= len(ts) <= SATURATION_MAX_POINTS:
            raise ValueError("between 1 and 32 depths must be given")
        if any(b < a for a, b in zip(ts, ts[1:])):
            raise ValueError("the depths must be non-decreasing")
        _u64_arg("seed", seed), _u64_arg("first_row", first_row)
        arr = (C.c_uint64 * len(ts))(*ts)
        pts = (CSaturationPoint * len(ts))()
        _check(lib.ibu_saturation_curve(self._c, _dptr(d_sorted_records), n, first_row, seed, arr, len(ts), pts, stream))
        return [SaturationPoint(int(p.threshold), int(p.reads), int(p.barcodes), int(p.molecules)) for p in pts]

    # barcode correction against a whitelist
    def correct_barcodes(self, wl, d_records, n, max_mismatches=1, d_class=None, counts=True, stream=None):
        """ibu_correct_barcodes, in place over n device records: exact whitelist hits stay, a barcode with exactly one
        whitelist entry one substitution away moves onto it.  d_class (optional): n bytes, one class per record (0 exact,
        1 corrected, 2 ambiguous, 3 unmatched).  counts=True synchronises and returns the four totals as a dict;
        counts=False leaves the call asynchronous and returns None."""
        c = CCorrectCounts() if counts else None
        _check(lib.ibu_correct_barcodes(self._c, wl._c, _dptr(d_records), n, max_mismatches, _dptr(d_class),
                                        C.byref(c) if counts else None, stream))
        if not counts:
            return None
        return {"exact": c.exact, "corrected": c.corrected, "ambiguous": c.ambiguous, "unmatched": c.unmatched}

    def resolve_barcodes(self, wl, ab, d_records, n, d_class, min_share=(39, 40), counts=True, stream=None):
        """ibu_resolve_barcodes, in place over n device records and their class bytes (what correct_barcodes left): a record of
        class 2 (ambiguous) whose best candidate — the whitelisted neighbour with the largest counter in the Abundance `ab` — holds
        at least min_share = (num, den) of its candidates' counted reads (best * den >= num * total in integers, best > 0;
        1 <= num <= den < 2^24 and 2 * num > den) moves onto that candidate and gets class BARCODE_RESOLVED; every other record
        and class byte stays.  counts=True synchronises and returns {"examined", "resolved", "below_share", "unseen"};
        counts=False leaves the call asynchronous and returns None.  select_records(..., keep_mask=0b10011) then keeps exact,
        corrected and resolved records."""
        num, den = min_share
        c = CResolveCounts() if counts else None
        _check(lib.ibu_resolve_barcodes(self._c, getattr(wl, "_c", None), getattr(ab, "_c", None), _dptr(d_records), n, _u64_arg("num", num),
                                        _u64_arg("den", den), _dptr(d_class), C.byref(c) if counts else None, stream))
        if not counts:
            return None
        return {"examined": c.examined, "resolved": c.resolved, "below_share": c.below_share, "unseen": c.unseen}

    # per-barcode labels onto records
    def label_records(self, labels, d_records, n, d_class=None, match=None, missing_class=255, hist=False, stream=None):
        """ibu_label_records over n device records (never written): a record is found when its barcode (the low 2*bc_len bits) is
        an entry of the whitelist `labels` belongs to, and its label is that entry's byte.  d_class (optional): n bytes — with
        match=None the label, or missing_class where not found; with match=L the classes LABEL_IS (found, label == L), LABEL_OTHER
        and LABEL_MISSING, so that select_records(..., keep_mask=1 << LABEL_IS) extracts the records of label L.  hist=True
        synchronises and returns a numpy u64[257]: reads per label, then the reads not found (d_class=None with hist=True is the
        "reads per label" query and writes nothing per record); hist=False leaves the call asynchronous and returns None."""
        h = (C.c_uint64 * LABEL_BINS)() if hist else None
        _check(lib.ibu_label_records(self._c, getattr(labels, "_c", None), _dptr(d_records), n, 0 if match is None else LABEL_MATCH,
                                     _u32_arg("match", 0 if match is None else match), _u32_arg("missing_class", missing_class),
                                     _dptr(d_class), h, stream))
        return np.array(h, dtype=np.uint64) if hist else None

    def labels_from_assignment(self, row_barcodes, row_top, row_class, features, bc_len, mixed=254, none=253, stream=None):
        """A Whitelist and a Labels table from what assign_features returned (its d_barcodes, RowTop and d_class) -> (Whitelist,
        Labels): the whitelist holds the row barcodes (their low 2*bc_len bits), and the label of a ROW_ASSIGNED row is the
        position of its top feature in `features`, of a ROW_MIXED row `mixed`, of a ROW_NONE row — and of an assigned row whose top
        feature is not in `features` — `none`.  `features` may therefore hold at most 253 positions; more raise ValueError, and so do
        rows whose barcodes differ only in bits at or above 2*bc_len (they would be one entry with two labels).
        label_records(labels, ...) then carries the verdict onto the records of any library with these barcodes.
        The byte column is composed on the HOST in numpy, from one download per column of the per-barcode table (barcodes, top
        features, classes): that table has one row per barcode, far fewer than there are records, and nothing per record leaves the
        device.  Close the labels and the whitelist (in that order, or the whitelist alone) when done.  Synchronises."""
        feats = [int(f) for f in features]
        if len(feats) > 253:
            raise ValueError(f"features holds {len(feats)} positions; a label byte has room for 253 beside `mixed` and `none`")
        if len(set(feats)) != len(feats):
            raise ValueError("features must be distinct")
        for name, v in (("mixed", mixed), ("none", none)):
            if not len(feats) <= v <= 255:
                raise ValueError(f"{name} must be a byte that is no position of `features`")
        r = row_top.n_rows
        if r == 0:
            raise ValueError("no rows: a whitelist needs at least one barcode")
        if not 1 <= bc_len <= 32:
            raise ValueError("bc_len must be in 1 .. 32")
        self.synchronize(stream)
        keys = row_barcodes.download(np.uint64, r)
        top = row_top.top_key.download(np.uint64, r)
        cls = row_class.download(np.uint8, r)
        if bc_len < 32:
            keys = keys & np.uint64((1 << (2 * bc_len)) - 1)
        if len(np.unique(keys)) != r:                            # one label per barcode: two rows of one barcode would leave it either's
            raise ValueError("row barcodes that differ only in bits at or above 2*bc_len are one barcode: mask the records' barcodes "
                             "before they are counted")
        order = np.argsort(np.array(feats, np.uint64), kind="stable") if feats else np.empty(0, np.int64)
        sorted_feats = np.array(feats, np.uint64)[order]
        pos = np.minimum(np.searchsorted(sorted_feats, top), max(len(feats) - 1, 0))
        known = (sorted_feats[pos] == top) if feats else np.zeros(r, bool)
        lab = np.full(r, none, np.uint8)
        on = (cls == ROW_ASSIGNED) & known
        lab[on] = order[pos[on]].astype(np.uint8)
        lab[cls == ROW_MIXED] = mixed
        d_keys = self.upload(keys)
        try:
            wl = Whitelist(self, d_keys, r, bc_len, stream)
        finally:
            d_keys.free()
        try:
            labels = wl.labels(fill=none, stream=stream)
            labels.set(keys, lab, stream=stream)
        except BaseException:
            wl.close()                                           # (closes the labels on it as well)
            raise
        return wl, labels

    def select_records(self, d_records, d_class, n, keep_mask=0b0011, stream=None):
        """ibu_select_records: the records whose class has its bit set in keep_mask (default: exact and corrected), in
        input order -> (DeviceBuffer, n_out).  One call, so one count pass and one synchronisation: the buffer has room for
        all n records (what a whitelist step usually keeps nearly all of); the first n_out of them are valid once `stream` has
        run (the scatter may still be queued on return)."""
        k = C.c_size_t()
        out = self.alloc(max(24 * n, 16))
        _check(lib.ibu_select_records(self._c, _dptr(d_records), _dptr(d_class), n, keep_mask, _dptr(out), n, C.byref(k), stream))
        return out, k.value

    def partition_records(self, d_records, d_class, n, n_parts=None, part_of=None, out=None, stream=None):
        """ibu_partition_records: a stable multi-way partition of n device records by class byte, in one pass -> (DeviceBuffer,
        offsets as numpy u64[n_parts + 1]).  part_of (256 bytes, optional): the part of every class byte, a value below n_parts or
        PART_NONE for a class whose records are dropped; None is the identity below n_parts.  n_parts (1 .. 255) may be left out
        when part_of is given: one more than its largest part.  The buffer holds part 0, then part 1, ..., each in input order:
        part p is records offsets[p] .. offsets[p + 1], and offsets[n_parts] records are kept.  out (optional): a DeviceBuffer to
        write to, its capacity out.nbytes // 24 records; otherwise one with room for all n records is allocated, as select_records
        does.  One count pass and one synchronisation; the records are valid once `stream` has run (the scatter may still be
        queued on return)."""
        if part_of is not None:
            po = np.ascontiguousarray(part_of)
            if po.shape != (256,) or po.dtype.kind not in "ui" or ((po < 0) | (po > 255)).any():
                raise ValueError("part_of must hold 256 bytes")
            po = po.astype(np.uint8)
            if n_parts is None:
                kept = po[po != PART_NONE]
                n_parts = int(kept.max()) + 1 if kept.size else 1
        elif n_parts is None:
            raise ValueError("partition_records needs n_parts or part_of")
        n_parts = _u32_arg("n_parts", n_parts)
        offsets = (C.c_uint64 * (min(n_parts, 255) + 1))()
        own = out is None
        if own:
            out = self.alloc(max(24 * n, 16))
        cap = n if own else out.nbytes // 24
        try:
            _check(lib.ibu_partition_records(self._c, _dptr(d_records), _dptr(d_class), n,
                                             None if part_of is None else po.ctypes.data_as(_lib.u8p), n_parts, _dptr(out), cap, offsets,
                                             stream))
        except BaseException:
            if own:
                out.free()
            raise
        return out, np.array(offsets, dtype=np.uint64)

    def partition_by_label(self, lb, d_records, n, labels, stream=None):
        """Every sample of a multiplexed library at once: one label_records call in plain mode and one partition_records call ->
        (DeviceBuffer, offsets as numpy u64[len(labels) + 1]).  Part j holds the records whose barcode carries the label labels[j]
        in the Labels table `lb`, in input order; records with any other label, and records whose barcode is no entry, are
        dropped.  labels: 1 .. 255 distinct bytes (anything else raises ValueError before any device call)."""
        labs = [int(v) for v in labels]
        if not 1 <= len(labs) <= 255:
            raise ValueError(f"labels holds {len(labs)} values; a partition has 1 .. 255 parts")
        if any(not 0 <= v <= 255 for v in labs):
            raise ValueError("a label is one byte")
        if len(set(labs)) != len(labs):
            raise ValueError("labels must be distinct")
        missing = next(v for v in range(256) if v not in set(labs))   # at most 255 labels: a byte is free
        part_of = np.full(256, PART_NONE, np.uint8)
        part_of[labs] = np.arange(len(labs), dtype=np.uint8)
        d_class = self.alloc(max(n, 16))
        try:
            self.label_records(lb, d_records, n, d_class=d_class, missing_class=missing, stream=stream)
            return self.partition_records(d_records, d_class, n, n_parts=len(labs), part_of=part_of, stream=stream)
        finally:
            self.synchronize(stream)                             # the scatter reads the class bytes
            d_class.free()

    def inflate_blocks(self, d_comp, blocks, d_out, stream=None):
        """ibu_inflate_blocks_device: the deflate blocks `blocks` (a ctypes array of ibu_inflate_block_t, or what bgzf_scan
        returned) of the compressed bytes at d_comp -> d_out.  Returns (status per block as numpy u32, first bad block or None);
        synchronises."""
        n = len(blocks)
        if n == 0:
            return np.empty(0, np.uint32), None
        raw = np.frombuffer(bytes(blocks), dtype=np.uint8) if not isinstance(blocks, np.ndarray) else blocks.view(np.uint8)
        d_blocks = self.upload(raw)
        d_status = self.alloc(4 * n + 4)
        first = np.full(1, 0xFFFFFFFF, np.uint32)
        _check(lib.ibu_memcpy_h2d(self._c, d_status.ptr + 4 * n, _hptr(first), 4, stream))
        _check(lib.ibu_inflate_blocks_device(self._c, _dptr(d_comp), d_blocks.ptr, n, _dptr(d_out), d_status.ptr, d_status.ptr + 4 * n, stream))
        self.synchronize(stream)
        st = d_status.download(np.uint32)
        d_blocks.free()
        d_status.free()
        return st[:n].copy(), (None if st[n] == 0xFFFFFFFF else int(st[n]))

    def lower_bound(self, d_sorted_records, n, d_keys, k, d_pos, stream=None):
        """d_pos[j] (u64, device) = first position whose record is >= key j (24-byte records in d_keys); asynchronous."""
        _check(lib.ibu_lower_bound_records(self._c, _dptr(d_sorted_records), n, _dptr(d_keys), k, _dptr(d_pos), stream))

    # compacted keys (the exchange format of the multi-GPU sort)
    def census(self, d_records, n, stream=None):
        """{"or": [3], "and": [3], "index_drops": bool, "order_drops": bool} of n device records; synchronises."""
        out = (C.c_uint64 * 8)()
        _check(lib.ibu_records_census(self._c, _dptr(d_records), n, out, stream))
        return {"or": [int(v) for v in out[0:3]], "and": [int(v) for v in out[3:6]], "index_drops": bool(out[6]),
                "order_drops": bool(out[7])}

    def compact(self, plan, d_records, n, d_elems, stream=None):
        """n records -> n 12-byte elements (plan: key_plan(); plan.k <= 12); asynchronous."""
        _check(lib.ibu_records_compact(self._c, C.byref(plan), _dptr(d_records), n, _dptr(d_elems), stream))

    def expand(self, plan, d_elems, n, d_records, stream=None):
        """n 12-byte elements -> the n records they stand for; asynchronous."""
        _check(lib.ibu_records_expand(self._c, C.byref(plan), _dptr(d_elems), n, _dptr(d_records), stream))

    def first_mismatch(self, d_a, d_b, n, stream=None):
        """Index of the first of n records in which the two device slices differ; n if they are equal
        (`a == b` on record slices: Record derives PartialEq / Eq, record.rs:58)."""
        f = C.c_uint64()
        _check(lib.ibu_records_first_mismatch(self._c, _dptr(d_a), _dptr(d_b), n, C.byref(f), stream))
        return int(f.value)

    def records_equal(self, d_a, d_b, n, stream=None):
        return self.first_mismatch(d_a, d_b, n, stream) == n

    def is_sorted(self, d_records, n, stream=None):
        s = C.c_int32()
        _check(lib.ibu_is_sorted(self._c, _dptr(d_records), n, stream, C.byref(s)))
        return bool(s.value)

    # streams
    def load_to_device(self, path, ring=None, d_records=None, cap_records=0):
        """Device analogue of load_to_vec -> (Header, device pointer (int) or the given buffer, n, stats)."""
        h, n, st = CHeader(), C.c_size_t(), CStreamStats()
        p = C.c_void_p(_dptr(d_records).value if d_records is not None else None)
        _check(lib.ibu_load_to_device(self._c, str(path).encode(), _ring(ring), C.byref(h), C.byref(p), cap_records,
                                      C.byref(n), C.byref(st)))
        return Header._wrap(h), p.value, n.value, st

    def load_bgzf_to_device(self, path, ring=None, d_records=None, cap_records=0):
        """ibu_load_bgzf_to_device: a BGZF file of the records -> device records, inflated on the device (the compressed bytes cross
        the link) -> (Header, device pointer (int) or the given buffer, n, stats)."""
        h, n, st = CHeader(), C.c_size_t(), CStreamStats()
        p = C.c_void_p(_dptr(d_records).value if d_records is not None else None)
        _check(lib.ibu_load_bgzf_to_device(self._c, str(path).encode(), _ring(ring), C.byref(h), C.byref(p), cap_records,
                                           C.byref(n), C.byref(st)))
        return Header._wrap(h), p.value, n.value, st

    def load_bgzf_shard_to_device(self, path, shard, n_shards, ring=None, d_records=None, cap_records=0):
        """ibu_load_bgzf_shard_to_device: shard `shard` of `n_shards` of the file's records (the split of process_parallel)
        -> (Header, device pointer, n, first record's number, stats)."""
        h, n, first, st = CHeader(), C.c_size_t(), C.c_uint64(), CStreamStats()
        p = C.c_void_p(_dptr(d_records).value if d_records is not None else None)
        _check(lib.ibu_load_bgzf_shard_to_device(self._c, str(path).encode(), _ring(ring), shard, n_shards, C.byref(h), C.byref(p), cap_records,
                                                 C.byref(n), C.byref(first), C.byref(st)))
        return Header._wrap(h), p.value, n.value, first.value, st

    def free(self, ptr):
        _check(lib.ibu_device_free(self._c, ptr))

    def _run_proc(self, call, proc, sink, ring, lens=(1, 1)):
        st = CStreamStats()
        if proc == PROC_REDUCE:
            r = CReduceResult()
            _check(call(self._c, _ring(ring), C.cast(C.byref(r), C.c_void_p), C.byref(st)))
            return {"count": r.count, "sum": list(r.sum), "xor": list(r.xor_)}, st
        cols = list(sink[:3])
        if len(sink) > 3:
            cap = int(sink[3])
        else:  # capacity = what the buffers hold (DeviceBuffer / torch tensors know their size)
            sizes = [(c, w) for c, w in zip(cols, (lens[0], lens[1], 8)) if c is not None]
            if not all(hasattr(c, "nbytes") or hasattr(c, "numel") for c, _ in sizes):
                raise TypeError("a decode sink of raw pointers needs its capacity: sink=(d_bc, d_umi, d_index, cap_records)")
            cap = min((c.nbytes if hasattr(c, "nbytes") else c.numel() * c.element_size()) // w for c, w in sizes) if sizes else 0
        s = CDecodeSink(*(_dptr(x) for x in cols), cap)
        _check(call(self._c, _ring(ring), C.cast(C.byref(s), C.c_void_p), C.byref(st)))
        return None, st

    def close(self):
        if getattr(self, "_c", None):
            for b in list(getattr(self, "_buffers", ())):   # buffers that outlive the context would leak their HBM
                b.free()
            for w in list(getattr(self, "_whitelists", ())):   # a whitelist (and the abundances on it) goes before its context
                w.close()
            lib.ibu_ctx_destroy(self._c)
            self._c = None

    __del__ = close


class Whitelist:
    """ibu_whitelist_t: the device lookup table of a barcode whitelist, built from `w` 2-bit codes in device memory
    (what Context.pack_2bit writes).  Belongs to `ctx`; close it before the context."""

    def __init__(self, ctx, d_codes, w, bc_len, stream=None):
        h = C.c_void_p()
        _check(lib.ibu_whitelist_create(getattr(ctx, "_c", None), _dptr(d_codes), w, bc_len, stream, C.byref(h)))
        self._c, self.ctx = h, ctx
        self._abundances = weakref.WeakSet()   # live Abundances and Labels on it
        ctx._whitelists.add(self)   # a context that closes first destroys what was built on it (Context.close)
        b, nd, db = C.c_uint32(), C.c_size_t(), C.c_size_t()
        _check(lib.ibu_whitelist_info(self._c, C.byref(b), C.byref(nd), C.byref(db)))
        self.bc_len, self.n_distinct, self.device_bytes = b.value, nd.value, db.value

    @classmethod
    def from_ascii(cls, ctx, barcodes):
        """From barcodes as text: a list of equally long str / bytes, or a 2-D uint8 array (one row per barcode).
        Uploads them and packs them on the device (Context.pack_2bit; a byte outside ACGTacgt raises InvalidBase)."""
        if isinstance(barcodes, np.ndarray):
            a = np.ascontiguousarray(barcodes, dtype=np.uint8)
        else:
            rows = [b.encode() if isinstance(b, str) else bytes(b) for b in barcodes]
            if not rows or any(len(r) != len(rows[0]) for r in rows):
                raise ValueError("a whitelist needs at least one barcode, all of one length")
            a = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), len(rows[0]))
        if a.ndim != 2 or a.shape[0] == 0:
            raise ValueError("barcodes must be a non-empty list or a 2-D uint8 array")
        w, bc_len = a.shape
        d_ascii, d_codes = ctx.upload(a), ctx.alloc(8 * w)
        try:
            ctx.pack_2bit(d_ascii, w, bc_len, d_codes)
            ctx.codec_status()
            return cls(ctx, d_codes, w, bc_len)
        finally:
            d_ascii.free()
            d_codes.free()

    def abundance(self, stream=None):
        """A new Abundance on this whitelist: one read counter per entry, all zero."""
        return Abundance(self.ctx, self, stream)

    def labels(self, fill=255, stream=None):
        """A new Labels table on this whitelist: one label byte per entry, all `fill`."""
        return Labels(self.ctx, self, fill, stream)

    def close(self):
        if getattr(self, "_c", None):
            for a in list(getattr(self, "_abundances", ())):   # an abundance or a label table goes before its whitelist
                a.close()
            lib.ibu_whitelist_destroy(self._c)
            self._c = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Abundance:
    """ibu_abundance_t: one u64 read counter per entry of a Whitelist, on the device (Whitelist.abundance()).  add() counts
    records, Context.resolve_barcodes reads the counters.  Belongs to its whitelist and that whitelist's context; close it before
    them (a whitelist that closes first closes it)."""

    def __init__(self, ctx, wl, stream=None):
        h = C.c_void_p()
        _check(lib.ibu_abundance_create(getattr(ctx, "_c", None), getattr(wl, "_c", None), stream, C.byref(h)))
        self._c, self.ctx, self.wl = h, ctx, wl
        wl._abundances.add(self)
        db = C.c_size_t()
        _check(lib.ibu_abundance_info(self._c, C.byref(db)))
        self.device_bytes = db.value

    def add(self, d_records, n, d_class=None, class_mask=1, stream=None):
        """ibu_abundance_add over n device records: the counter of a record's barcode (its low 2*bc_len bits) grows by one where
        that barcode is in the whitelist and the record contributes — every record with d_class=None, else the records whose class
        byte c < 8 has bit c of class_mask set (default: class 0, the exact hits).  Asynchronous; accumulates over calls."""
        _check(lib.ibu_abundance_add(self.ctx._c, self._c, _dptr(d_records), _dptr(d_class), n, class_mask, stream))

    def counts(self, codes, stream=None):
        """ibu_abundance_counts: the counters of `codes` (host u64 values) as a numpy u64 array; 0 for a code that is not in the
        whitelist.  Synchronises."""
        a = np.ascontiguousarray(codes, dtype=np.uint64).reshape(-1)
        if len(a) == 0:
            return np.empty(0, np.uint64)
        d_codes, d_out = self.ctx.upload(a), self.ctx.alloc(max(8 * len(a), 16))
        try:
            _check(lib.ibu_abundance_counts(self.ctx._c, self._c, d_codes.ptr, len(a), d_out.ptr, stream))
            self.ctx.synchronize(stream)
            return d_out.download(np.uint64, len(a))
        finally:
            d_codes.free()
            d_out.free()

    def reset(self, stream=None):
        """All counters back to zero (asynchronous)."""
        _check(lib.ibu_abundance_reset(self._c, stream))

    def close(self):
        if getattr(self, "_c", None):
            lib.ibu_abundance_destroy(self._c)
            self._c = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Labels:
    """ibu_labels_t: one label byte per entry of a Whitelist, on the device (Whitelist.labels()).  set() writes labels by barcode,
    Context.label_records carries them onto records.  Belongs to its whitelist and that whitelist's context; close it before them
    (a whitelist that closes first closes it)."""

    def __init__(self, ctx, wl, fill=255, stream=None):
        h = C.c_void_p()
        _check(lib.ibu_labels_create(getattr(ctx, "_c", None), getattr(wl, "_c", None), _u32_arg("fill", fill), stream, C.byref(h)))
        self._c, self.ctx, self.wl = h, ctx, wl
        wl._abundances.add(self)
        db = C.c_size_t()
        _check(lib.ibu_labels_info(self._c, C.byref(db)))
        self.device_bytes = db.value

    def set(self, codes, labels, stream=None):
        """ibu_labels_set: the label of codes[j] (host u64 values) becomes labels[j] (host bytes, one per code).  -> the number of
        codes skipped: not in the whitelist, or with bits at or above 2*bc_len.  Synchronises."""
        a = np.ascontiguousarray(codes, dtype=np.uint64).reshape(-1)
        v = np.ascontiguousarray(labels, dtype=np.uint8).reshape(-1)
        if len(a) != len(v):
            raise ValueError("one label per code")
        if len(a) == 0:
            return 0
        d_codes, d_vals = self.ctx.upload(a), self.ctx.upload(v)
        try:
            k = C.c_size_t()
            _check(lib.ibu_labels_set(self.ctx._c, self._c, d_codes.ptr, d_vals.ptr, len(a), C.byref(k), stream))
            return k.value
        finally:
            d_codes.free()
            d_vals.free()

    def get(self, codes, missing=255, stream=None):
        """ibu_labels_get: the labels of `codes` (host u64 values) as a numpy u8 array; `missing` for a code that is not an entry.
        Synchronises."""
        a = np.ascontiguousarray(codes, dtype=np.uint64).reshape(-1)
        missing = _u32_arg("missing", missing)
        if len(a) == 0:
            return np.empty(0, np.uint8)
        d_codes, d_out = self.ctx.upload(a), self.ctx.alloc(max(len(a), 16))
        try:
            _check(lib.ibu_labels_get(self.ctx._c, self._c, d_codes.ptr, len(a), missing, d_out.ptr, stream))
            self.ctx.synchronize(stream)
            return d_out.download(np.uint8, len(a))
        finally:
            d_codes.free()
            d_out.free()

    def close(self):
        if getattr(self, "_c", None):
            lib.ibu_labels_destroy(self._c)
            self._c = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


__all__ = ["Whitelist", "Abundance", "Labels", "Header", "Record", "HEADER_SIZE", "MAGIC", "RECORD_SIZE", "VERSION", "IbuError", "load_to_vec",
           "MmapReader", "Reader", "Writer", "ParallelProcessor", "ProcessError", "shard_range", "Context",
           "DeviceBuffer", "DeviceStream", "DeviceBatch", "numa_of_pci", "records_array", "key_plan", "REC_DTYPE", "device_count", "PROC_REDUCE", "PROC_DECODE",
           "DEFAULT_BUFFER_SIZE", "BATCH_SIZE"]
