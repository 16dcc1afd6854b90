// host_io.hpp — internal hooks the streaming layer (stream.cpp) needs from host_io.cpp.
#pragma once
#include <errno.h>
#include <stddef.h>
#include <stdint.h>
#include <sys/types.h>

#include "../../include/ibu_hip.h"

namespace ibu {
// Writer::write_slice (writer.rs:321-351) on raw bytes — used by the device write_batch path.
int32_t writer_write_bytes(ibu_writer_t* w, const uint8_t* bytes, size_t len);
// Front half of load_to_vec (reader.rs:511-526): open, header, validate, size check.
int32_t open_plain_file(const char* path, int* fd_out, ibu_header_t* header, size_t* n_records);
// The device streaming path's refill: reads straight from the reader's source into `dst` (a pinned ring slot) until
// `cap_bytes` are there or the stream ends, without the detour through the reader's own 1.18 MB buffer (which must be
// empty: ibu_reader_buffered == 0).  Whole records only: a stream that ends inside a record is TruncatedRecord with the
// position read_batch would report (reader.rs:232-237), with *got_bytes = the complete record bytes in front of the cut and
// r->bytes_read unchanged; a source error likewise leaves in *got_bytes the complete record bytes read in front of it.
// *eof: the stream ended (possibly with *got_bytes > 0).
int32_t reader_read_direct(ibu_reader_t* r, uint8_t* dst, size_t cap_bytes, size_t* got_bytes, bool* eof);
int reader_bgzf_fd_if_untouched(const ibu_reader_t* r);   // host_io.cpp
void reader_set_drained(ibu_reader_t* r, uint64_t records);
// A Reader over the BGZF file open on `fd` that takes over at record `records_before`: the host inflate from the member at file byte
// `member_offset` on, its first `skip` bytes dropped (the member holds that record's first byte), header `h`.  It reads as the Reader
// of the whole file reads from there: the same errors, positions counted from the file's start.  `fd` stays the caller's.
int32_t reader_open_bgzf_at(int fd, uint64_t member_offset, size_t skip, const ibu_header_t& h, uint64_t records_before, ibu_reader_t** out);
// pread until `len` bytes are in, the file ends or an error other than EINTR comes: 0 or errno, *got = the bytes read either way.
int pread_upto(int fd, uint8_t* dst, size_t len, off_t off, size_t* got);
// The same where a short read is an error: EIO (the file shrank underneath us).
inline int pread_all(int fd, uint8_t* dst, size_t len, off_t off) {
  size_t got = 0;
  const int e = pread_upto(fd, dst, len, off, &got);
  return e ? e : (got < len ? EIO : 0);
}
// A whole file mapped read-only (MAP_PRIVATE); unmapped when its owner goes.
struct FileMap {
  const uint8_t* p = nullptr;
  size_t n = 0;
  FileMap() {}
  FileMap(const FileMap&) = delete;
  FileMap& operator=(const FileMap&) = delete;
  ~FileMap();
};
// Opens `path`, hands its size to `check` (a status other than IBU_OK is returned as it is, nothing mapped), maps it whole and closes
// the descriptor.  Its own errors: err_io(errno, path), err_io(errno, "metadata"), err_io(errno, "mmap").
int32_t map_file(const char* path, FileMap* m, int32_t (*check)(size_t size));
// num_cpus::get()
size_t host_cores();
// Threads for the inflate workers (BGZF blocks, pgzip chunks): the CPUs this process may run on, but at most twice its
// cgroup CPU quota.  Twice, because the batch pipeline has serial stretches (windows, hand-over, the consumer's copies) in
// which the quota goes unused and a decode thread stalls on a table-lookup chain that a second thread on the core's other
// hardware thread fills: measured on the 16-CPU-quota box of this pool, 32 threads inflate 1.37x (1e9 records, sustained,
// throttling included) to 1.47x (1e8) faster than 16.  The quota still bounds the CPU time; without a quota this is the
// affinity count.
size_t inflate_threads();
}  // namespace ibu
