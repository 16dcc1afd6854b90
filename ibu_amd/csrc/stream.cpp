// stream.cpp — record streams between files / mmap / gzip and the device, through a ring of
// pinned (hipHostMalloc) staging slots.  Host work (page-cache memcpy, pread, inflate) for
// slot k+1 overlaps the H2D copy of slot k (copy stream) and the kernel on slot k-1 (compute
// stream); the two streams are chained per slot with events, never with a device-wide sync.
//
//   file/mmap/gz --host threads--> pinned[slot] --copy_stream H2D--> dev[slot] --stream--> kernel
//
// ONE pipeline feeds the device: the pull stream (ibu_stream_*, below) — a producer thread that fills pinned slots and queues
// their H2D copies, and a consumer that takes device-resident batches in order.  ibu_mmap_process_device and
// ibu_reader_process_device are that consumer with one of the two built-in processors as the loop body.  A BGZF file goes through
// the same stream in its device form (ibu_stream_open_path; ibu_reader_process_device of an untouched BGZF Reader): the producer
// loads ranges of records inflated on the device (BgzfLoad) and the batches are views into the range buffers.
//
// These are the device-backed forms of load_to_vec (reader.rs:510-535), Writer::write_batch
// (writer.rs:315-351), MmapReader::process_parallel (mmap.rs:286-332, ONE shard of its static
// split per call = per GPU) and the streaming Reader (reader.rs:279-306, incl. the gzip path
// of reader.rs:345-352).
#include <errno.h>
#include <fcntl.h>
#include <pthread.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "bgzf_plan.hpp"
#include "ctx.hpp"
#include "host_io.hpp"
#include "kernels.h"

using namespace ibu;

namespace {

struct KernelClock {  // sums hipEvent spans of the per-slot kernels
  std::vector<hipEvent_t> a, b;
  std::vector<char> live;
  double ms = 0;
  int32_t init(uint32_t slots) {
    a.resize(slots);
    b.resize(slots);
    live.assign(slots, 0);
    for (uint32_t i = 0; i < slots; ++i) {
      IBU_HIP(hipEventCreate(&a[i]));
      IBU_HIP(hipEventCreate(&b[i]));
    }
    return IBU_OK;
  }
  void harvest(uint32_t s) {
    if (!live[s]) return;
    float t = 0;
    if (hipEventSynchronize(b[s]) == hipSuccess && hipEventElapsedTime(&t, a[s], b[s]) == hipSuccess) ms += t;
    live[s] = 0;
  }
  ~KernelClock() {
    for (auto e : a) (void)hipEventDestroy(e);
    for (auto e : b) (void)hipEventDestroy(e);
  }
};

int32_t drain(ibu_ctx* ctx, int32_t rc) {  // leave no copy or kernel in flight over ring memory
  (void)hipStreamSynchronize(ctx->copy_stream);
  (void)hipStreamSynchronize(ctx->stream);
  return rc;
}

struct DeviceProc {  // the device-side ParallelProcessor applied to each staged slot
  ibu_ctx* ctx;
  int32_t kind;
  uint32_t bc_len, umi_len;
  ibu_decode_sink_t sink{};
  // the columns of a DECODE sink hold cap_records rows: a batch that does not fit is refused BEFORE anything is launched
  int32_t fits(size_t n, size_t row0) const {
    if (kind != IBU_PROC_DECODE || row0 + n <= sink.cap_records) return IBU_OK;
    return set_error(IBU_ERR_INVALID_ARG, row0 + n, sink.cap_records, 0,
                     "Invalid argument: decode sink holds %zu records, the stream has at least %zu", sink.cap_records, row0 + n);
  }
  int32_t launch(const uint8_t* d_slot, size_t n, size_t row0) {
    if (kind == IBU_PROC_REDUCE) {
      IBU_HIP(launch_reduce(ctx->cfg, d_slot, n, ctx->d_acc, ctx->stream));
    } else {
      IBU_HIP(launch_decode(ctx->cfg, d_slot, n, bc_len, umi_len,
                            sink.d_bc_ascii ? sink.d_bc_ascii + row0 * bc_len : nullptr,
                            sink.d_umi_ascii ? sink.d_umi_ascii + row0 * umi_len : nullptr,
                            sink.d_index ? sink.d_index + row0 : nullptr, ctx->stream));
    }
    return IBU_OK;
  }
};

int32_t make_proc(ibu_ctx* ctx, int32_t proc, const ibu_header_t& h, void* sink, DeviceProc* out) {
  if (!sink) return err_arg("sink is NULL");
  out->ctx = ctx;
  out->kind = proc;
  out->bc_len = h.bc_len;
  out->umi_len = h.umi_len;
  if (proc == IBU_PROC_DECODE) out->sink = *static_cast<ibu_decode_sink_t*>(sink);
  else if (proc != IBU_PROC_REDUCE) return err_arg("unknown device processor");
  return IBU_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// ring management
// ------------------------------------------------------------------------------------------
void ibu::ring_release(ibu_ctx* ctx) {
  Ring& r = ctx->ring;
  for (auto p : r.pinned)
    if (p) (void)hipHostFree(p);
  for (auto p : r.dev)
    if (p) (void)hipFree(p);
  for (auto e : r.copied) (void)hipEventDestroy(e);
  for (auto e : r.consumed) (void)hipEventDestroy(e);
  r = Ring();
}

int32_t ibu::ring_ensure(ibu_ctx* ctx, const ibu_ring_config_t* cfg, bool need_dev) {
  uint32_t slots = cfg && cfg->slots ? cfg->slots : 4;
  if (slots < 2) slots = 2;
  size_t slot_records = cfg && cfg->slot_records ? cfg->slot_records : 4u * IBU_BATCH_SIZE;
  slot_records = (slot_records + 127) & ~(size_t)127;  // whole kernel tiles, 16-B aligned column offsets
  const size_t slot_bytes = slot_records * IBU_RECORD_SIZE;
  Ring& r = ctx->ring;
  if (ctx->ring_lent) return err_arg("the context's ring is lent to an open ibu_stream_t: close the stream first (or use a second context)");
  if (r.slots == slots && r.slot_bytes == slot_bytes && (!need_dev || !r.dev.empty())) return IBU_OK;
  (void)hipStreamSynchronize(ctx->copy_stream);
  (void)hipStreamSynchronize(ctx->stream);
  ring_release(ctx);
  r.pinned.assign(slots, nullptr);
  r.copied.resize(slots);
  r.consumed.resize(slots);
  for (uint32_t i = 0; i < slots; ++i) {
    IBU_HIP(hipEventCreateWithFlags(&r.copied[i], hipEventDisableTiming));
    IBU_HIP(hipEventCreateWithFlags(&r.consumed[i], hipEventDisableTiming));
  }
  {
    // Option "numa": the pinned slots on the node the device hangs off.  Under a preferred-node policy of this thread the
    // allocation follows it (hipHostMallocNumaUser); a kernel that refuses the policy (a container's seccomp profile) leaves
    // the runtime's own choice, as before.  Either way ring.node says where the pages are, if the kernel will tell.
    PreferNode prefer(ctx->numa_mode ? ctx->place.node : -1);
    const unsigned flags = prefer.active() ? hipHostMallocNumaUser : hipHostMallocDefault;
    for (uint32_t i = 0; i < slots; ++i)
      IBU_HIP(hipHostMalloc(reinterpret_cast<void**>(&r.pinned[i]), slot_bytes, flags));
    r.placed = prefer.active();
  }
  r.node = node_of_range(r.pinned[0], slot_bytes);
  if (need_dev) {
    r.dev.assign(slots, nullptr);
    for (uint32_t i = 0; i < slots; ++i) IBU_HIP(ctx_malloc(ctx, reinterpret_cast<void**>(&r.dev[i]), slot_bytes));
  }
  r.slots = slots;
  r.slot_bytes = slot_bytes;
  return IBU_OK;
}

// ------------------------------------------------------------------------------------------
// load_to_vec, device form
// ------------------------------------------------------------------------------------------
extern "C" int32_t ibu_load_to_device(ibu_ctx_t* ctx, const char* path, const ibu_ring_config_t* cfg,
                                      ibu_header_t* header, void** d_records, size_t cap_records, size_t* n,
                                      ibu_stream_stats_t* stats) {
  if (!ctx || !path || !header || !d_records || !n) return err_arg("NULL argument");
  IBU_HIP(hipSetDevice(ctx->device));
  RunOnNode on_node(feed_place(ctx));   // for the length of the call this thread and the pread threads it starts run on the device's node (option "numa")
  const double t0 = now_s();
  int fd = -1;
  size_t num = 0;
  int32_t rc = open_plain_file(path, &fd, header, &num);
  if (rc) return rc;
  bool owned = false;
  if (*d_records == nullptr) {
    rc = ctx_alloc(ctx, num * IBU_RECORD_SIZE, d_records);   // (placement-probed under option "alloc_probe_tries")
    if (rc) {
      close(fd);
      return rc;
    }
    owned = true;
  } else if (num > cap_records) {
    close(fd);
    return err_arg("device buffer too small for the file");
  }
  rc = ring_ensure(ctx, cfg, false);
  Ring& r = ctx->ring;
  const size_t slot_records = r.slot_bytes / IBU_RECORD_SIZE;
  if (stats) memset(stats, 0, sizeof *stats);
  for (size_t done = 0, k = 0; rc == IBU_OK && done < num; ++k) {
    const uint32_t s = (uint32_t)(k % r.slots);
    const size_t nb = num - done < slot_records ? num - done : slot_records;
    const size_t bytes = nb * IBU_RECORD_SIZE;
    hipError_t e = hipEventSynchronize(r.copied[s]);  // slot's previous H2D has left the pinned buffer
    if (e != hipSuccess) { rc = hip_fail(e, "hipEventSynchronize"); break; }
    const off_t base = (off_t)(IBU_HEADER_SIZE + done * IBU_RECORD_SIZE);
    uint8_t* dst = r.pinned[s];
    int err = parallel_bytes(bytes, feeder_threads(cfg), (size_t)1 << 20, [&](size_t off, size_t len) {
      return pread_all(fd, dst + off, len, base + (off_t)off);
    });
    if (err) { rc = err_io(err, "read records"); break; }
    e = hipMemcpyAsync(static_cast<uint8_t*>(*d_records) + done * IBU_RECORD_SIZE, dst, bytes, hipMemcpyHostToDevice,
                       ctx->copy_stream);
    if (e == hipSuccess) e = hipEventRecord(r.copied[s], ctx->copy_stream);
    if (e != hipSuccess) { rc = hip_fail(e, "H2D"); break; }
    if (stats) { stats->bytes_h2d += bytes; stats->batches += 1; }
    done += nb;
  }
  close(fd);
  hipError_t e = hipStreamSynchronize(ctx->copy_stream);
  if (rc == IBU_OK && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize");
  if (rc != IBU_OK) {
    if (owned) { (void)hipFree(*d_records); *d_records = nullptr; }
    return rc;
  }
  *n = num;
  if (stats) { stats->records = num; stats->seconds_total = now_s() - t0; }
  return IBU_OK;
}

// ------------------------------------------------------------------------------------------
// load_to_vec of a BGZF file, inflated on the device (k_inflate.hip): the COMPRESSED bytes cross the link
// ------------------------------------------------------------------------------------------
// The result is what ibu_load_to_device gives for the gunzipped file (load_to_vec, reader.rs:510-535).  A block is accepted exactly as the
// host decoder accepts it; anything else — a member that is not a BGZF block, a file that ends inside one, a block that does not inflate
// to its announced length and CRC — is IBU_ERR_NIFFLER, as from the Reader (the index: bgzf_plan.cpp).
namespace {

// The file, mapped: an empty one is a cut-off header, and it is read front to back.
int32_t map_bgzf(const char* path, FileMap* m) {
  const int32_t rc = map_file(path, m, [](size_t size) -> int32_t { return size ? IBU_OK : err_io(0, "read header"); });
  if (rc == IBU_OK) (void)madvise(const_cast<uint8_t*>(m->p), m->n, MADV_SEQUENTIAL);
  return rc;
}

// The staging on the device — the compressed file; the descriptors and status words behind it once their number is known — is the
// context's and grows only (freeing 1.2 GB and allocating it again cost a call of 1e8 records 12 of its 104 ms).
int32_t grow_stage(ibu_ctx* ctx, size_t need) {
  if (need <= ctx->inflate_stage_bytes) return IBU_OK;
  void* p = nullptr;
  hipError_t e = ctx_malloc(ctx, &p, need);
  if (e != hipSuccess) return hip_fail(e, "hipMalloc");
  if (ctx->d_inflate_stage) {                              // (the bytes copied so far move along)
    e = hipMemcpyAsync(p, ctx->d_inflate_stage, ctx->inflate_stage_bytes, hipMemcpyDeviceToDevice, ctx->copy_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->copy_stream);
    (void)hipFree(ctx->d_inflate_stage);
    if (e != hipSuccess) { (void)hipFree(p); ctx->d_inflate_stage = nullptr; ctx->inflate_stage_bytes = 0; return hip_fail(e, "hipMemcpy"); }
  }
  ctx->d_inflate_stage = p;
  ctx->inflate_stage_bytes = need;
  return IBU_OK;
}

// The device staging one load of `plan` needs: its compressed bytes, the descriptors, the status words and the lanes' tables of the
// decoder's scratch form (a load of more blocks than one round of the short form, or than option "inflate_one_launch")
size_t stage_bytes(const ibu_ctx* ctx, const ShardPlan& plan, size_t* comp_room, size_t* desc_room, size_t* status_room, size_t* tables_room) {
  const size_t nrest = plan.dev_blocks();
  *comp_room = (plan.cend - plan.cbeg + kInflatePad + 255) & ~(size_t)255;
  *desc_room = (nrest * sizeof(InflateBlockDesc) + 255) & ~(size_t)255;
  *status_room = (4 * nrest + 16 + 255) & ~(size_t)255;
  const size_t ahead_from = ctx->inflate_one_launch ? ctx->inflate_one_launch : inflate_one_round(ctx->cfg.cus);
  *tables_room = nrest > ahead_from ? inflate_scratch_bytes(ctx->cfg, nrest, 2) : 256;   // (the short form needs none)
  return *comp_room + *desc_room + *status_room + 256 + *tables_room;
}

// One load of one shard.  At most one round of the decoder's short form (inflate_one_round: 49 152 blocks, 3 GB of records): ONE launch
// behind the last copy — a wave takes its ~45 ms whatever the launch's size, so the call ends that long after its last byte has arrived
// either way.  More: ONE launch as well, but AHEAD of the copies, in the decoder's other form (tables in scratch, eight waves per CU): its
// waves take the blocks in file order and each waits until the copy stream has said that its blocks are there (`d_ready`, written
// behind every piece; k_inflate.hip), so the device inflates at the rate the bytes come in.
struct BgzfLoad {
  static constexpr uint32_t kNone = 0xFFFFFFFFu;
  ibu_ctx* ctx;
  const ibu_ring_config_t* cfg;
  const FileMap& file;
  ibu_stream_stats_t* stats;
  ibu_header_t* header;
  void** d_records;                                        // nullptr: allocated here
  size_t cap_records, shard, n_shards;
  const BgzfIndex* idx = nullptr;                          // the index and the plan the caller made (the pull stream's ranges), or the
  ShardPlan plan{};                                        // walk beside the copies makes the index and plan_shard the plan
  bool ring_lent = false;                                  // the caller holds the context's ring (the pull stream): no ring_ensure
  bool behind = false;                                     // launch behind the last copy in chunks (inflate_late's), never ahead of the copies
  std::vector<uint8_t> edge_bytes{};                       // (the host side of the asynchronous copies lives as long as the load)
  std::vector<ibu_inflate_block_t> desc_host{};
  uint32_t none_word = kNone;
  BgzfIndex walked{};
  std::thread walker{};
  std::atomic<bool> walk_done{false};
  int32_t walk_rc = IBU_OK;
  ibu_error_detail_t walk_detail{};
  bool prepared = false, owned = false, ahead = false;     // ahead: the launch that runs ahead of the copies is out
  uint8_t *d_out = nullptr, *d_tables = nullptr;           // d_tables: the lanes' tables of a launch in the decoder's scratch form
  InflateBlockDesc* d_desc = nullptr;
  uint32_t *d_status = nullptr, *d_first_bad = nullptr, last_slot = 0;
  size_t tables_room = 0, launches = 0;
  std::vector<size_t> piece_end{};                         // piece k of the copies ends at this file byte
  double t0 = now_s(), t_mark = t0, t_ph[4] = {0, 0, 0, 0};   // (IBU_TRACE_SORT=1: where the call's time went)
  ~BgzfLoad() { if (walker.joinable()) walker.join(); }
  void lap(int k) { const double t = now_s(); t_ph[k] += t - t_mark; t_mark = t; }
  size_t ahead_from() const { return ctx->inflate_one_launch ? ctx->inflate_one_launch : inflate_one_round(ctx->cfg.cus); }
  uint64_t* d_ready() const { return ctx->h_inflate_marks; }   // (pinned host memory: the device reads it over the link)
  hipStream_t q() const { return ctx->inflate_streams[0]; }
  // The walk on a thread of its own while this one already copies the file to the device: the copies need nothing but the file's size.
  // (In line, the walk's 12.5 ms of page faults stood in front of a call of 1e8 records that takes 88.)
  void walk_beside() {
    plan.cend = file.n;                                    // (one shard of one: the whole file, before the walk is done)
    auto run = [this] {
      if ((walk_rc = bgzf_index(file.p, file.n, &walked))) walk_detail = tls_error();   // (the detail lives in the walker's thread)
      walk_done.store(true, std::memory_order_release);
    };
    try { walker = std::thread(run); } catch (...) { run(); }   // no thread to be had: in line
  }
  int32_t run(size_t* n, uint64_t* first_record) {
    int32_t rc = IBU_OK;
    try { rc = load(); } catch (...) { rc = caught_io("ibu_load_bgzf_to_device"); }
    if (rc) {                                              // every failure: nothing left running, nothing kept that this call allocated
      if (walker.joinable()) walker.join();
      if (ahead) __atomic_store_n(d_ready(), ~0ull, __ATOMIC_RELEASE);   // its waves must not wait for bytes that will not come
      (void)hipStreamSynchronize(ctx->copy_stream);
      for (hipStream_t s : ctx->inflate_streams)
        if (s) (void)hipStreamSynchronize(s);
      if (owned) { (void)hipFree(*d_records); *d_records = nullptr; }
      return rc;
    }
    *n = plan.num;
    if (first_record) *first_record = plan.rec_first;
    if (stats) { stats->records = plan.num; stats->seconds_total = now_s() - t0; stats->numa_node = feed_place(ctx).node; stats->ring_node = ctx->ring.node; }
    return IBU_OK;
  }
  int32_t load() {
    // (one shard of one: room for the whole file and the descriptors of 64 KiB blocks: the copies start at once, nothing is allocated twice)
    int32_t rc = ring_lent ? IBU_OK : ring_ensure(ctx, cfg, false);   // (first: a context whose ring is lent keeps its staging untouched)
    if (!rc && n_shards == 1 && !idx) rc = grow_stage(ctx, ((file.n + kInflatePad + 255) & ~(size_t)255) + 40 * (file.n / 8192 + 64));
    hipError_t e = hipSuccess;
    for (hipStream_t& s : ctx->inflate_streams)
      if (!s && !rc && e == hipSuccess) e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (rc || e != hipSuccess) return rc ? rc : hip_fail(e, "hipStreamCreate");
    lap(0);
    if ((n_shards > 1 || idx) && (rc = prepare())) return rc;   // (a shard's bytes are known only after the walk)
    if ((rc = copy())) return rc;
    lap(1);
    if ((!prepared && (rc = prepare())) || (rc = launch(true))) return rc;
    lap(2);
    if ((rc = finish())) return rc;
    lap(3);
    if (trace_sort())
      fprintf(stderr, "ibu load_bgzf: %zu blocks (walked %s), %zu launches; ms: staging %.2f, copies (the walk beside them) and early launches %.2f, walk's results to the "
              "device + last launches %.2f, waiting for them %.2f\n", idx->blocks.size(), idx->in_pieces ? "in 8 pieces side by side" : "in one go", launches,
              1e3 * t_ph[0], 1e3 * t_ph[1], 1e3 * t_ph[2], 1e3 * t_ph[3]);
    return IBU_OK;
  }
  // What the index allows, once it is there: the plan, the destination, the host-inflated bytes, the descriptors on the device
  int32_t prepare() {
    if (!idx) {
      if (walker.joinable()) walker.join();
      idx = &walked;
      if (walked.head.size() >= IBU_HEADER_SIZE) *header = walked.header;
      if (walk_rc) { tls_error() = walk_detail; return walk_rc; }
      if (int32_t rc = plan_shard(*idx, shard, n_shards, &plan)) return rc;
    }
    const size_t nrest = plan.dev_blocks();
    if (*d_records == nullptr) {
      if (int32_t rc = ctx_alloc(ctx, plan.num * IBU_RECORD_SIZE, d_records)) return rc;
      owned = true;
    } else if (plan.num > cap_records) {
      return set_error(IBU_ERR_INVALID_ARG, plan.num, cap_records, 0, "Invalid argument: device buffer too small for the shard (%zu records, room for %zu)",
                       plan.num, cap_records);
    }
    d_out = static_cast<uint8_t*>(*d_records);
    hipError_t e = hipSuccess;
    // Every copy of the load goes out on its own non-blocking streams: a synchronous copy would wait for the work of every blocking stream
    // (the pull stream loads the next range while the caller's kernels run on its batches)
    auto put = [&](const uint8_t* bytes, uint64_t at, uint64_t len) {   // bytes [at, at + len) of the stream, as far as they are the shard's
      const uint64_t a = std::max(at, plan.lo), z = std::min(at + len, plan.hi);
      if (a < z && e == hipSuccess) e = hipMemcpyAsync(d_out + (a - plan.lo), bytes + (a - at), z - a, hipMemcpyHostToDevice, q());
    };
    put(idx->head.data(), 0, idx->head.size());            // the records behind the header in the blocks inflated for it
    pgz::RawInflater raw;
    edge_bytes.resize(2 * 65536);
    for (size_t k = 0; k < plan.n_edges; ++k) {            // the blocks that straddle the shard's ends
      const ibu_inflate_block_t& b = idx->blocks[plan.edge[k]];
      uint8_t* edge = edge_bytes.data() + k * 65536;
      if (int32_t rc = inflate_block_on_host(raw, file.p, b, edge)) return rc;
      put(edge, (uint64_t)b.out_offset, b.out_len);
    }
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy");
    size_t comp_room = 0, desc_room = 0, status_room = 0;
    if (int32_t rc = grow_stage(ctx, stage_bytes(ctx, plan, &comp_room, &desc_room, &status_room, &tables_room))) return rc;
    d_desc = reinterpret_cast<InflateBlockDesc*>(static_cast<uint8_t*>(ctx->d_inflate_stage) + comp_room);
    d_status = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(d_desc) + desc_room);
    d_first_bad = d_status + nrest;
    d_tables = reinterpret_cast<uint8_t*>(d_status) + status_room + 256;
    if (!ctx->h_inflate_marks) {                           // (coherent whatever HIP_HOST_COHERENT says: the device must see the host's stores)
      e = hipHostMalloc(reinterpret_cast<void**>(&ctx->h_inflate_marks), 8 * sizeof(uint64_t), hipHostMallocMapped | hipHostMallocCoherent);
      if (e != hipSuccess) { ctx->h_inflate_marks = nullptr; return hip_fail(e, "hipHostMalloc"); }
    }
    desc_host.assign(idx->blocks.begin() + (ptrdiff_t)plan.dev_first, idx->blocks.begin() + (ptrdiff_t)plan.dev_end);
    for (ibu_inflate_block_t& b : desc_host) {             // relative to the shard's records / to the bytes on the device
      b.out_offset -= (int64_t)plan.lo;
      b.comp_offset -= plan.cbeg;
    }
    if (nrest && e == hipSuccess) e = hipMemcpyAsync(d_desc, desc_host.data(), nrest * sizeof(InflateBlockDesc), hipMemcpyHostToDevice, q());
    if (e == hipSuccess) e = hipMemcpyAsync(d_first_bad, &none_word, 4, hipMemcpyHostToDevice, q());
    __atomic_store_n(d_ready(), 0ull, __ATOMIC_RELEASE);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy");
    prepared = true;
    return IBU_OK;
  }
  void publish(size_t done_upto) {                         // the host has SEEN the copies up to this file byte complete: the launch may use them
    if (ahead) __atomic_store_n(d_ready(), (uint64_t)(done_upto - plan.cbeg), __ATOMIC_RELEASE);
  }
  int32_t copy() {
    Ring& r = ctx->ring;
    for (size_t k = 0, up = plan.cbeg; up < plan.cend; ++k) {   // up: file bytes [cbeg, up) are on their way
      const uint32_t sl = (uint32_t)(k % r.slots);
      const size_t len = std::min(plan.cend - up, r.slot_bytes);
      if (ctx->load_piece_delay_ms) std::this_thread::sleep_for(std::chrono::milliseconds(ctx->load_piece_delay_ms));
      hipError_t e = hipEventSynchronize(r.copied[sl]);
      if (e != hipSuccess) return hip_fail(e, "hipEventSynchronize");
      if (k >= r.slots) publish(piece_end[k - r.slots]);   // (this slot's previous piece has landed: so has everything in front of it)
      uint8_t* dst = r.pinned[sl];
      const uint8_t* src = file.p + up;
      parallel_memcpy(dst, src, len, feeder_threads(cfg), (size_t)1 << 20);
      e = hipMemcpyAsync(static_cast<uint8_t*>(ctx->d_inflate_stage) + (up - plan.cbeg), dst, len, hipMemcpyHostToDevice, ctx->copy_stream);
      if (e == hipSuccess) e = hipEventRecord(r.copied[sl], ctx->copy_stream);
      if (e != hipSuccess) return hip_fail(e, "H2D");
      up += len;
      last_slot = sl;
      if (stats) { stats->bytes_h2d += len; stats->batches += 1; }
      piece_end.push_back(up);
      int32_t rc = IBU_OK;
      if (!prepared && walk_done.load(std::memory_order_acquire) && (rc = prepare())) return rc;
      if (prepared && (rc = launch(false))) return rc;
    }
    return IBU_OK;
  }
  int32_t launch(bool all) {
    const size_t nrest = plan.dev_blocks();
    if (behind) return all && !launches && nrest ? launch_behind(0) : IBU_OK;
    const bool streamed = nrest > ahead_from();
    if (launches || nrest == 0 || (!streamed && !all)) return IBU_OK;
    ahead = streamed;
    hipError_t e = hipSuccess;
    if (streamed)
      e = launch_inflate_blocks(ctx->cfg, ctx->d_inflate_stage, d_desc, nrest, d_out, d_status, d_first_bad, d_tables, tables_room, q(), 2, d_ready(),
                                plan.cend - plan.cbeg);
    else if ((e = hipStreamWaitEvent(q(), ctx->ring.copied[last_slot], 0)) == hipSuccess)   // (at most one round: the short form, behind the last copy)
      e = launch_inflate_blocks(ctx->cfg, ctx->d_inflate_stage, d_desc, nrest, d_out, d_status, d_first_bad, d_tables, tables_room, q(), 0);
    if (e != hipSuccess) return hip_fail(e, "inflate");
    ++launches;
    return IBU_OK;
  }
  // Blocks [at, nrest) in launches of at most eight waves of 64 blocks per CU, behind the last copy (everything is on the device by then)
  int32_t launch_behind(size_t at) {
    const size_t nrest = plan.dev_blocks();
    hipError_t e = hipStreamWaitEvent(q(), ctx->ring.copied[last_slot], 0);
    for (size_t cnt = 0; at < nrest && e == hipSuccess; at += cnt, ++launches) {
      cnt = std::min(nrest - at, (size_t)ctx->cfg.cus * 8 * 64);
      e = launch_inflate_blocks(ctx->cfg, ctx->d_inflate_stage, d_desc + at, cnt, d_out, d_status + at, d_first_bad, d_tables, tables_room, q(),
                                cnt > inflate_one_round(ctx->cfg.cus) ? 2 : 0);
    }
    return e == hipSuccess ? IBU_OK : hip_fail(e, "inflate");
  }
  int32_t finish() {
    uint32_t first_bad = kNone;
    hipError_t e = hipStreamSynchronize(ctx->copy_stream);
    if (e == hipSuccess) publish(plan.cend);               // every byte is there
    for (hipStream_t s : ctx->inflate_streams)
      if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipMemcpyAsync(&first_bad, d_first_bad, 4, hipMemcpyDeviceToHost, q());
    if (e == hipSuccess) e = hipStreamSynchronize(q());
    if (e != hipSuccess) return hip_fail(e, "ibu_load_bgzf_to_device");
    if (first_bad != kNone && ahead)
      if (int32_t rc = inflate_late(&first_bad)) return rc;
    if (first_bad == kNone) return IBU_OK;
    if (trace_sort()) {
      uint32_t st1 = 0;
      (void)hipMemcpy(&st1, d_status + first_bad, 4, hipMemcpyDeviceToHost);
      fprintf(stderr, "ibu load_bgzf: block %u of the device's %zu refused (status %u: 1 not a deflate stream of these sizes, 2 CRC-32, 3 its bytes never arrived)\n",
              first_bad, plan.dev_blocks(), st1);
    }
    return err_niffler("a BGZF block does not inflate to its announced length and CRC-32");
  }
  // Waves of the launch that ran ahead give up after ~4 s without their blocks (status 3): a slow source, not a bad file.  Everything
  // is on the device now: those blocks — from the first of them on — go through a plain launch.  A block that was REFUSED stays refused.
  int32_t inflate_late(uint32_t* first_bad) {
    const size_t nrest = plan.dev_blocks();
    std::vector<uint32_t> stv(nrest);
    hipError_t e = hipMemcpyAsync(stv.data(), d_status, 4 * nrest, hipMemcpyDeviceToHost, q());
    if (e == hipSuccess) e = hipStreamSynchronize(q());
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy");
    if (std::any_of(stv.begin(), stv.end(), [](uint32_t st) { return st && st != 3; })) return IBU_OK;   // (refused stays refused)
    const size_t late = (size_t)(std::find(stv.begin(), stv.end(), 3u) - stv.begin());
    if (late == nrest) return IBU_OK;
    if (trace_sort()) fprintf(stderr, "ibu load_bgzf: the bytes of blocks %zu ... came later than the waves waited: inflating them now\n", late);
    e = hipMemcpyAsync(d_first_bad, &none_word, 4, hipMemcpyHostToDevice, q());
    ahead = false;                                         // (nothing to release any more on a failure)
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy");
    if (int32_t rc = launch_behind(late)) return rc;
    e = hipMemcpyAsync(first_bad, d_first_bad, 4, hipMemcpyDeviceToHost, q());
    if (e == hipSuccess) e = hipStreamSynchronize(q());
    return e == hipSuccess ? IBU_OK : hip_fail(e, "ibu_load_bgzf_to_device");
  }
};

}  // namespace

extern "C" int32_t ibu_load_bgzf_to_device(ibu_ctx_t* ctx, const char* path, const ibu_ring_config_t* cfg, ibu_header_t* header,
                                           void** d_records, size_t cap_records, size_t* n, ibu_stream_stats_t* stats) {
  return ibu_load_bgzf_shard_to_device(ctx, path, cfg, 0, 1, header, d_records, cap_records, n, nullptr, stats);
}
// Shard `shard` of `n_shards` of the file's records (the split of process_parallel, mmap.rs:297-307): the blocks that lie wholly inside
// the shard's bytes are copied and inflated on the device, the (at most two) blocks that straddle its ends are inflated on the host and
// their part copied — as the blocks holding the header always are.  Every device of a node loads its own range of the same file.
extern "C" int32_t ibu_load_bgzf_shard_to_device(ibu_ctx_t* ctx, const char* path, const ibu_ring_config_t* cfg, size_t shard, size_t n_shards,
                                                 ibu_header_t* header, void** d_records, size_t cap_records, size_t* n, uint64_t* first_record,
                                                 ibu_stream_stats_t* stats) {
  if (!ctx || !path || !header || !d_records || !n) return err_arg("NULL argument");
  if (n_shards == 0 || shard >= n_shards) return err_arg("shard out of range");
  IBU_HIP(hipSetDevice(ctx->device));
  RunOnNode on_node(feed_place(ctx));
  if (stats) memset(stats, 0, sizeof *stats);
  FileMap file;
  if (int32_t rc = map_bgzf(path, &file)) return rc;
  BgzfLoad L{ctx, cfg, file, stats, header, d_records, cap_records, shard, n_shards};
  L.walk_beside();
  return L.run(n, first_record);
}

// ------------------------------------------------------------------------------------------
// Writer::write_batch, device form
// ------------------------------------------------------------------------------------------
extern "C" int32_t ibu_writer_write_batch_device(ibu_writer_t* w, ibu_ctx_t* ctx, const ibu_ring_config_t* cfg,
                                                 const void* d_records, size_t n, ibu_stream_stats_t* stats) {
  return ibu_writer_write_batch_device_on(w, ctx, cfg, d_records, n, nullptr, stats);
}
extern "C" int32_t ibu_writer_write_batch_device_on(ibu_writer_t* w, ibu_ctx_t* ctx, const ibu_ring_config_t* cfg,
                                                    const void* d_records, size_t n, void* producer_stream,
                                                    ibu_stream_stats_t* stats) {
  if (!w || !ctx || (!d_records && n)) return err_arg("NULL argument");
  IBU_HIP(hipSetDevice(ctx->device));
  RunOnNode on_node(feed_place(ctx));   // the copies pinned ring -> writer buffer / file on the device's node (option "numa")
  const double t0 = now_s();
  if (stats) memset(stats, 0, sizeof *stats);
  int32_t rc = ring_ensure(ctx, cfg, false);
  if (rc) return rc;
  Ring& r = ctx->ring;
  const size_t slot_records = r.slot_bytes / IBU_RECORD_SIZE;
  const size_t nchunks = (n + slot_records - 1) / slot_records;
  const uint8_t* src = static_cast<const uint8_t*>(d_records);
  // the records were produced on `producer_stream` (NULL: the context's own stream): order the copy stream behind it
  IBU_HIP(hipEventRecord(r.consumed[0], pick_stream(ctx, producer_stream)));
  IBU_HIP(hipStreamWaitEvent(ctx->copy_stream, r.consumed[0], 0));
  auto issue = [&](size_t c) -> int32_t {
    const uint32_t s = (uint32_t)(c % r.slots);
    const size_t row = c * slot_records;
    const size_t nb = n - row < slot_records ? n - row : slot_records;
    IBU_HIP(hipMemcpyAsync(r.pinned[s], src + row * IBU_RECORD_SIZE, nb * IBU_RECORD_SIZE, hipMemcpyDeviceToHost,
                           ctx->copy_stream));
    IBU_HIP(hipEventRecord(r.copied[s], ctx->copy_stream));
    return IBU_OK;
  };
  for (size_t c = 0; c < nchunks && c < r.slots && rc == IBU_OK; ++c) rc = issue(c);
  for (size_t c = 0; c < nchunks && rc == IBU_OK; ++c) {
    const uint32_t s = (uint32_t)(c % r.slots);
    const size_t row = c * slot_records;
    const size_t nb = n - row < slot_records ? n - row : slot_records;
    hipError_t e = hipEventSynchronize(r.copied[s]);
    if (e != hipSuccess) { rc = hip_fail(e, "hipEventSynchronize"); break; }
    rc = writer_write_bytes(w, r.pinned[s], nb * IBU_RECORD_SIZE);  // buffered / direct rule of writer.rs:321-351
    if (rc) break;
    if (stats) { stats->bytes_d2h += nb * IBU_RECORD_SIZE; stats->batches += 1; }
    if (c + r.slots < nchunks) rc = issue(c + r.slots);
  }
  if (rc) return drain(ctx, rc);
  if (stats) { stats->records = n; stats->seconds_total = now_s() - t0; }
  return IBU_OK;
}

// ------------------------------------------------------------------------------------------
// The pull stream: Reader::read_batch + Iterator (reader.rs:218-242, :279-306) and the per-batch loop of process_parallel
// (mmap.rs:312-320) with the batch in HBM
// ------------------------------------------------------------------------------------------
// A producer thread owns the source, the pinned slots and the copy stream; the consumer (the caller's thread) owns the order in
// which batches are taken and the streams that read them.  Slot s goes FREE -> FILLING -> (H2D queued) READY -> (next) HELD ->
// (release: `consumed[s]` recorded on the caller's stream) RELEASED -> (producer waits for that event) FILLING ...  The producer
// takes ANY slot the consumer does not hold, so batches held for long (at most slots - 1) never stall the others.
struct ibu_stream {
  ibu_ctx* ctx = nullptr;
  ibu_header_t header{};
  ibu_reader_t* rd = nullptr;        // source: a borrowed Reader ...
  const ibu_mmap_t* m = nullptr;     // ... or records [start, end) of a map
  size_t start = 0, end = 0;
  uint32_t feeders = 4;
  size_t slot_records = 0;
  uint64_t first0 = 0;               // number of the stream's first record (mmap: start; reader: 0)
  double t0 = 0;
  std::mutex mu;
  std::condition_variable cv;
  enum : uint8_t { FREE, FILLING, READY, HELD, RELEASED };
  struct Slot { uint8_t state = FREE; size_t n = 0; uint64_t first = 0, seq = 0; };   // seq: when it was released (oldest refilled first)
  uint64_t release_seq = 0;
  std::vector<Slot> slot;
  std::deque<uint32_t> ready;        // READY slots in stream order
  uint32_t held = 0;
  bool stop = false, done = false, started = false;
  int32_t rc = IBU_OK;               // the source's error, delivered after the batches in front of it
  ibu_error_detail_t detail{};
  ibu_stream_stats_t stats{};
  std::vector<uint8_t> stage;        // Reader sources with slots smaller than one refill: the refill being handed out piecewise
  size_t stage_pos = 0, stage_len = 0;   // records
  bool src_eof = false;              // the Reader source reported its end
  std::thread producer;
  // A path stream (ibu_stream_open_path; ibu_reader_process_device of a BGZF file) owns a descriptor of its file and the Reader of the
  // host path where it opens one (the whole file when no Reader is borrowed, or the rest of it from a range the device refused) ...
  int own_fd = -1;
  ibu_reader_t* own_rd = nullptr;
  ibu_ring_config_t cfg{};
  // ... and, in the device form, the file mapped and indexed once and read in ranges of range_records into the context's two range
  // buffers (ctx->d_range_buf)
  bool ranges = false;
  std::unique_ptr<FileMap> file;
  BgzfIndex idx;
  size_t range_records = 0, n_ranges = 0;
  struct RangeBuf { uint32_t out = 0; std::vector<hipEvent_t> released; };   // out: batches queued or held
  RangeBuf rbuf[2];
  std::vector<hipEvent_t> spare_events;
  int waiting = -1;                  // the producer waits for this range buffer's batches to come back
  // What next() hands out: a ring slot's batch (slot >= 0) or a view into range buffer `buf`
  struct Batch { uint8_t* p = nullptr; size_t n = 0; uint64_t first = 0; int slot = -1, buf = -1; };
  std::deque<Batch> rready;          // a range's batches in stream order, in front of any slot batch
  std::vector<Batch> rheld;
};

namespace {

// One slot's worth of a Reader source into `dst`: *filled records to deliver (possibly > 0 together with an error: the batch in
// front of a truncation), *eof = the source has ended.
// The stream delivers EXACTLY the records the reference's iterator yields, also in front of an error.  The reference refills
// IBU_DEFAULT_BUFFER_SIZE (= 49 152 records) at a time and a source that ends inside a record loses its whole final refill
// (reader.rs:232-237, quirk Q8); a record may therefore only be handed out once the refill it belongs to has arrived whole.
// So the stream reads in whole refills, counted from where it took over (the reader's own buffer empty = a refill boundary):
//   a slot of at least one refill asks the source for floor(room / refill) refills in one call, straight into the pinned slot
//     (parallel preads of a plain file, the inflate threads' own copies; no detour through the reader's buffer) — every batch
//     ends on a refill boundary;
//   a smaller slot (test rings) goes through a one-refill staging buffer.
int32_t fill_from_reader(ibu_stream* s, uint8_t* dst, size_t* filled, bool* eof) {
  ibu_reader_t* rd = s->rd;
  const size_t cap = s->slot_records;
  constexpr size_t kRefill = IBU_DEFAULT_BUFFER_SIZE, kRefillRecords = kRefill / IBU_RECORD_SIZE;
  size_t n = 0;
  *filled = 0;
  for (;;) {
    const ibu_record_t* recs;
    size_t have = 0;
    ibu_reader_buffered(rd, &recs, &have);
    if (have == 0) break;            // records the caller had pulled into the reader's buffer before the stream took over go first
    const size_t take = have < cap - n ? have : cap - n;
    memcpy(dst + n * IBU_RECORD_SIZE, recs, take * IBU_RECORD_SIZE);
    ibu_reader_consume(rd, take);
    n += take;
    if (n == cap) { *filled = n; return IBU_OK; }
  }
  if (s->stage_pos < s->stage_len) {                   // small slots: the rest of the staged refill
    const size_t take = s->stage_len - s->stage_pos < cap - n ? s->stage_len - s->stage_pos : cap - n;
    memcpy(dst + n * IBU_RECORD_SIZE, s->stage.data() + s->stage_pos * IBU_RECORD_SIZE, take * IBU_RECORD_SIZE);
    s->stage_pos += take;
    *filled = n + take;
    *eof = s->src_eof && s->stage_pos == s->stage_len;
    return IBU_OK;
  }
  if (s->src_eof) { *filled = n; *eof = true; return IBU_OK; }
  const size_t room = cap - n;
  if (room >= kRefillRecords) {
    const size_t ask = room / kRefillRecords * kRefill;
    size_t got = 0;
    const int32_t rc = reader_read_direct(rd, dst + n * IBU_RECORD_SIZE, ask, &got, &s->src_eof);
    if (rc) {                                          // a stream that ends inside a record, or a source error (reader.rs:225-237): `got` = the
      *filled = n + got / kRefill * kRefillRecords;    // complete record bytes in front of it — their WHOLE refills go out, as the reference's
      *eof = true;                                     // iterator has yielded them by then; the refill under way is lost with the error
      return rc;
    }
    *filled = n + got / IBU_RECORD_SIZE;
    *eof = s->src_eof;               // a short read is the end of the source: this batch is the last
    return IBU_OK;
  }
  if (n) { *filled = n; return IBU_OK; }               // buffered records left less than a refill of room: a short batch
  try {
    if (s->stage.size() < kRefill) s->stage.resize(kRefill);
  } catch (...) {
    *eof = true;
    return caught_io("ibu_stream: staging buffer");
  }
  size_t got = 0;
  const int32_t rc = reader_read_direct(rd, s->stage.data(), kRefill, &got, &s->src_eof);
  if (rc) { *eof = true; return rc; }                  // truncated: the final refill is dropped whole
  s->stage_len = got / IBU_RECORD_SIZE;
  s->stage_pos = s->stage_len < cap ? s->stage_len : cap;
  memcpy(dst, s->stage.data(), s->stage_pos * IBU_RECORD_SIZE);
  *filled = s->stage_pos;
  *eof = s->src_eof && s->stage_pos == s->stage_len;
  return IBU_OK;
}

// The ring's device slots, for a path stream that goes over to the host path (the device form lends only the pinned side)
int32_t ring_add_dev(ibu_ctx* ctx) {
  Ring& r = ctx->ring;
  if (!r.dev.empty()) return IBU_OK;
  r.dev.assign(r.slots, nullptr);
  for (uint32_t i = 0; i < r.slots; ++i) {
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&r.dev[i]), r.slot_bytes);
    if (e != hipSuccess) {
      for (uint8_t* p : r.dev)
        if (p) (void)hipFree(p);
      r.dev.clear();
      return hip_fail(e, "hipMalloc");
    }
  }
  return IBU_OK;
}

// The host path of a path stream from record `from` on: the whole file through the borrowed Reader or one of the same descriptor
// (from == 0), or the member holding that record's first byte on (a range boundary, so a refill boundary: the refills are counted on
// unchanged)
int32_t host_take_over(ibu_stream* s, uint64_t from) {
  if (int32_t rc = ring_add_dev(s->ctx)) return rc;
  if (from == 0 && s->rd) return IBU_OK;                   // (the caller's Reader, untouched: it reads as it would have read)
  if (from == 0) {
    if (lseek(s->own_fd, 0, SEEK_SET) < 0) return err_io(errno, "seek");
    const int32_t rc = ibu_reader_open_fd(s->own_fd, &s->own_rd);
    if (rc == IBU_OK) s->rd = s->own_rd;
    return rc;
  }
  const std::vector<ibu_inflate_block_t>& B = s->idx.blocks;
  const uint64_t lo = IBU_HEADER_SIZE + (uint64_t)IBU_RECORD_SIZE * from;
  size_t j = s->idx.lead;
  while (j < B.size() && (uint64_t)B[j].out_offset + B[j].out_len <= lo) ++j;
  if (j == B.size()) return err_niffler("corrupt or truncated compressed stream");
  const uint64_t member = j ? B[j - 1].comp_offset + B[j - 1].comp_len + 8 : 0;   // (every member is a BGZF block: they follow each other)
  const int32_t rc = reader_open_bgzf_at(s->own_fd, member, (size_t)(lo - (uint64_t)B[j].out_offset), s->header, from, &s->own_rd);
  if (rc == IBU_OK) s->rd = s->own_rd;
  return rc;
}

// Range k of a path stream's device form: records [k * range_records, ...) (plan_records); a file of one range is the load's whole-file
// plan (plan_shard: every byte of the file crosses the link, as for ibu_load_bgzf_to_device)
int32_t range_plan(const ibu_stream* s, size_t k, ShardPlan* plan) {
  if (s->n_ranges == 1) return plan_shard(s->idx, 0, 1, plan);
  const size_t total = (size_t)((s->idx.total - IBU_HEADER_SIZE) / IBU_RECORD_SIZE), first = k * s->range_records;
  return plan_records(s->idx, first, std::min(s->range_records, total - first), plan);
}

// The device form of a path stream: range k goes to range buffer k % 2 once every batch of the range before it there has been released
// and the work queued on the release streams has run; its compressed bytes cross the link through the ring's pinned slots and its blocks
// are inflated on the device (BgzfLoad), and its batches — views into the buffer — go out.  A load that fails hands over to the host path:
// *host = true, *from = the range's first record (the first range: anything; later ones: a block the device refused).
int32_t produce_ranges(ibu_stream* s, bool* host, uint64_t* from) {
  ibu_ctx* ctx = s->ctx;
  for (size_t k = 0; k < s->n_ranges; ++k) {
    const int b = (int)(k & 1);
    ibu_stream::RangeBuf& rb = s->rbuf[b];
    std::vector<hipEvent_t> released;
    {
      std::unique_lock<std::mutex> lk(s->mu);
      s->waiting = b;
      s->cv.notify_all();
      s->cv.wait(lk, [&] { return s->stop || rb.out == 0; });
      s->waiting = -1;
      if (s->stop) return IBU_OK;
      released.swap(rb.released);
    }
    hipError_t e = hipSuccess;
    for (hipEvent_t ev : released)
      if (e == hipSuccess) e = hipEventSynchronize(ev);
    {
      std::lock_guard<std::mutex> g(s->mu);
      s->spare_events.insert(s->spare_events.end(), released.begin(), released.end());
    }
    if (e != hipSuccess) return hip_fail(e, "hipEventSynchronize");
    ShardPlan plan;
    if (int32_t rc = range_plan(s, k, &plan)) return rc;
    // The range buffer: the context keeps it and it grows only (freeing and allocating 2.4 GB around every call cost a call of 1e8 records
    // 80 of its 155 ms); allocated when first needed, so a file of one range has one buffer.  Plain hipMalloc: no placement probing (the
    // records only pass through), and this thread must not touch the context's allocator state beside the caller's calls on the context.
    void*& d = ctx->d_range_buf[b];
    size_t& cap = ctx->range_buf_bytes[b];
    if (cap < plan.num * IBU_RECORD_SIZE) {
      (void)hipFree(d);
      d = nullptr;
      cap = 0;
      if ((e = hipMalloc(&d, plan.num * IBU_RECORD_SIZE)) != hipSuccess) { d = nullptr; return hip_fail(e, "hipMalloc"); }
      cap = plan.num * IBU_RECORD_SIZE;
    }
    ibu_stream_stats_t st{};
    ibu_header_t h = s->header;
    void* dst = d;
    size_t n = 0;
    const ibu_error_detail_t keep = tls_error();
    BgzfLoad L{ctx, &s->cfg, *s->file, &st, &h, &dst, cap / IBU_RECORD_SIZE, 0, 1, &s->idx, plan};
    L.ring_lent = true;
    L.behind = k > 0 && !ctx->bgzf_stream_ahead;           // (the first range, with nothing held, always launches ahead of its copies, as the load does)
    const int32_t rc = L.run(&n, nullptr);
    if (rc && (k == 0 || rc == IBU_ERR_NIFFLER)) {         // the host path decides: the same records, the same error
      tls_error() = keep;
      *host = true;
      *from = plan.rec_first;
      std::lock_guard<std::mutex> g(s->mu);
      if (k) s->stats.bytes_h2d += st.bytes_h2d;           // (the first range: the stats are the Reader stream's alone)
      return IBU_OK;
    }
    if (rc) return rc;
    std::lock_guard<std::mutex> g(s->mu);
    for (size_t at = 0; at < n; at += s->slot_records) {
      ibu_stream::Batch bt;
      bt.p = static_cast<uint8_t*>(d) + at * IBU_RECORD_SIZE;
      bt.n = std::min(s->slot_records, n - at);
      bt.first = plan.rec_first + at;
      bt.buf = b;
      s->rready.push_back(bt);
      ++rb.out;
      s->stats.batches += 1;
    }
    s->stats.records += n;
    s->stats.bytes_h2d += st.bytes_h2d;
    s->cv.notify_all();
  }
  return IBU_OK;
}

void stream_produce(ibu_stream* s) {
  ibu_ctx* ctx = s->ctx;
  Ring& r = ctx->ring;
  (void)pthread_setname_np(pthread_self(), "ibu-feed");
  RunOnNode on_node(feed_place(ctx));   // this thread and every thread it starts (feeders, inflate workers) on the device's node
  {
    std::lock_guard<std::mutex> g(s->mu);
    s->started = true;               // name and affinity are in place: ibu_stream_open_* returns only now (what ibu_ctx_numa and a
    s->cv.notify_all();              // look at /proc/self/task say is true from the first moment the caller holds the handle)
  }
  int32_t rc = IBU_OK;
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) rc = hip_fail(e, "hipSetDevice");
  const uint8_t* map = s->m ? static_cast<const uint8_t*>(ibu_mmap_base(s->m)) + IBU_HEADER_SIZE : nullptr;
  uint64_t delivered = 0;
  size_t row = s->start;
  bool eof = s->m ? s->start >= s->end : false;
  if (rc == IBU_OK && s->ranges) {   // the device form: the ranges, and the host path only from where the device refused a block
    bool host = false;
    rc = produce_ranges(s, &host, &delivered);
    if (rc == IBU_OK) eof = !host;
    if (rc == IBU_OK && host) rc = host_take_over(s, delivered);
  }
  while (rc == IBU_OK && !eof) {
    // any slot the consumer does not hold will do (never-used ones first, then the one released longest ago): with slots - 1 batches
    // held the one slot left keeps the stream moving — filling in ring order would wait for a HELD slot while a free one sat idle
    uint32_t si = 0;
    bool released = false;
    {
      std::unique_lock<std::mutex> lk(s->mu);
      int pick = -1;
      s->cv.wait(lk, [&] {
        if (s->stop) return true;
        pick = -1;
        for (uint32_t i = 0; i < r.slots && pick < 0; ++i)
          if (s->slot[i].state == ibu_stream::FREE) pick = (int)i;
        if (pick < 0)
          for (uint32_t i = 0; i < r.slots; ++i)
            if (s->slot[i].state == ibu_stream::RELEASED && (pick < 0 || s->slot[i].seq < s->slot[pick].seq)) pick = (int)i;
        return pick >= 0;
      });
      if (s->stop) break;
      si = (uint32_t)pick;
      released = s->slot[si].state == ibu_stream::RELEASED;
      s->slot[si].state = ibu_stream::FILLING;
    }
    if (released) {                  // the consumer's work on the slot's previous batch (and so its H2D) is done
      e = hipEventSynchronize(r.consumed[si]);
      if (e != hipSuccess) { rc = hip_fail(e, "hipEventSynchronize"); break; }
    }
    size_t n = 0;
    int32_t src_rc = IBU_OK;
    if (s->m) {
      n = s->end - row < s->slot_records ? s->end - row : s->slot_records;
      const uint8_t* srcp = map + row * IBU_RECORD_SIZE;
      uint8_t* dst = r.pinned[si];
      parallel_memcpy(dst, srcp, n * IBU_RECORD_SIZE, s->feeders, (size_t)1 << 20);  // page-cache / page-fault side of the reference's hot loop
      row += n;
      eof = row >= s->end;
    } else {
      src_rc = fill_from_reader(s, r.pinned[si], &n, &eof);
    }
    if (n) {
      const size_t bytes = n * IBU_RECORD_SIZE;
      e = hipMemcpyAsync(r.dev[si], r.pinned[si], bytes, hipMemcpyHostToDevice, ctx->copy_stream);
      if (e == hipSuccess) e = hipEventRecord(r.copied[si], ctx->copy_stream);
      if (e != hipSuccess) { rc = hip_fail(e, "H2D"); break; }
      std::lock_guard<std::mutex> g(s->mu);
      s->slot[si].state = ibu_stream::READY;
      s->slot[si].n = n;
      s->slot[si].first = s->first0 + delivered;
      s->ready.push_back(si);
      s->stats.records += n;
      s->stats.bytes_h2d += bytes;
      s->stats.batches += 1;
      delivered += n;
      s->cv.notify_all();
    } else {
      std::lock_guard<std::mutex> g(s->mu);
      s->slot[si].state = ibu_stream::FREE;     // nothing came (the end, or an error with no batch in front of it)
    }
    if (src_rc) rc = src_rc;
  }
  std::lock_guard<std::mutex> g(s->mu);
  s->rc = rc;
  if (rc) s->detail = tls_error();   // the detail lives in THIS thread's slot: next() copies it into its caller's
  s->done = true;
  s->cv.notify_all();
}

int32_t stream_open(ibu_ctx* ctx, const ibu_ring_config_t* cfg, ibu_stream* s) {
  IBU_HIP(hipSetDevice(ctx->device));
  int32_t rc = ring_ensure(ctx, cfg, !s->ranges);      // (the device form of a path stream copies through the pinned side only)
  if (rc) return rc;
  Ring& r = ctx->ring;
  s->ctx = ctx;
  s->feeders = feeder_threads(cfg);
  s->slot_records = r.slot_bytes / IBU_RECORD_SIZE;
  s->t0 = now_s();
  s->stats.numa_node = feed_place(ctx).node;
  s->stats.ring_node = r.node;
  try {
    s->slot.assign(r.slots, ibu_stream::Slot());
    ctx->ring_lent = s;
    s->producer = std::thread(stream_produce, s);
  } catch (...) {
    ctx->ring_lent = nullptr;
    return caught_io("ibu_stream_open");
  }
  std::unique_lock<std::mutex> lk(s->mu);
  s->cv.wait(lk, [&] { return s->started; });
  return IBU_OK;
}

// The consumer side of next(): a range's next batch (inflated before it was queued: nothing for `st` to wait for), else the oldest READY
// slot with `st` ordered behind its copy.  b->n == 0: end of stream.
int32_t stream_take(ibu_stream* s, hipStream_t st, ibu_stream::Batch* b) {
  Ring& r = s->ctx->ring;
  {
    std::unique_lock<std::mutex> lk(s->mu);
    for (;;) {
      if (!s->rready.empty()) {
        *b = s->rready.front();
        s->rready.pop_front();
        s->rheld.push_back(*b);
        return IBU_OK;
      }
      if (!s->ready.empty()) break;
      if (s->done) {
        b->n = 0;
        if (s->rc) { tls_error() = s->detail; return s->rc; }
        return IBU_OK;
      }
      if (s->held >= r.slots) return err_arg("every ring slot is held: release a batch before asking for the next");
      if (s->waiting >= 0 && s->rbuf[s->waiting].out)
        return err_arg("the next range goes to the range buffer whose batches are held: release them before asking for the next");
      s->cv.wait(lk);
    }
    const uint32_t si = s->ready.front();
    s->ready.pop_front();
    s->slot[si].state = ibu_stream::HELD;
    ++s->held;
    b->p = r.dev[si];
    b->n = s->slot[si].n;
    b->first = s->slot[si].first;
    b->slot = (int)si;
  }
  IBU_HIP(hipStreamWaitEvent(st, r.copied[b->slot], 0));
  return IBU_OK;
}

// release: a ring slot is refilled once `st` has run up to here (`consumed`); a range buffer is loaded again once every batch of it has
// come back and the work queued on the release streams has run (the producer waits for these events)
int32_t stream_give_back(ibu_stream* s, const ibu_stream::Batch& b, hipStream_t st) {
  hipError_t e = b.slot >= 0 ? hipEventRecord(s->ctx->ring.consumed[b.slot], st) : hipSuccess;
  std::lock_guard<std::mutex> g(s->mu);
  if (b.buf >= 0) {
    hipEvent_t ev = nullptr;
    if (!s->spare_events.empty()) {
      ev = s->spare_events.back();
      s->spare_events.pop_back();
    } else {
      e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    }
    if (e == hipSuccess) e = hipEventRecord(ev, st);
    if (e == hipSuccess) s->rbuf[b.buf].released.push_back(ev);
    else if (ev) s->spare_events.push_back(ev);
    for (size_t i = 0; i < s->rheld.size(); ++i)
      if (s->rheld[i].p == b.p) { s->rheld.erase(s->rheld.begin() + (ptrdiff_t)i); break; }
    --s->rbuf[b.buf].out;
  } else {
    s->slot[b.slot].state = ibu_stream::RELEASED;
    s->slot[b.slot].seq = ++s->release_seq;
    --s->held;
  }
  s->cv.notify_all();                // (even when the record failed: the stream must be able to end)
  return e == hipSuccess ? IBU_OK : hip_fail(e, "hipEventRecord");
}

void stream_shutdown(ibu_stream* s) {
  ibu_ctx* ctx = s->ctx;
  {
    std::lock_guard<std::mutex> g(s->mu);
    s->stop = true;
    s->cv.notify_all();
  }
  if (s->producer.joinable()) s->producer.join();
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->copy_stream);
  (void)hipStreamSynchronize(ctx->stream);
  for (uint32_t i = 0; i < s->slot.size(); ++i)   // work the caller queued on its own streams before releasing
    if (s->slot[i].state == ibu_stream::RELEASED) (void)hipEventSynchronize(ctx->ring.consumed[i]);
  for (ibu_stream::RangeBuf& rb : s->rbuf) {      // a path stream's own: its events, its Reader and descriptor (the range buffers are
    for (hipEvent_t ev : rb.released) {            // the context's)
      (void)hipEventSynchronize(ev);
      (void)hipEventDestroy(ev);
    }
    rb = ibu_stream::RangeBuf();
  }
  for (hipEvent_t ev : s->spare_events) (void)hipEventDestroy(ev);
  s->spare_events.clear();
  s->rready.clear();
  s->rheld.clear();
  if (s->ranges) ctx->stage_lent = false;
  if (s->own_rd) ibu_reader_close(s->own_rd);
  s->own_rd = nullptr;
  s->rd = nullptr;
  if (s->own_fd >= 0) close(s->own_fd);
  s->own_fd = -1;
  ctx->ring_lent = nullptr;
}

}  // namespace

extern "C" int32_t ibu_stream_open_reader(ibu_reader_t* r, ibu_ctx_t* ctx, const ibu_ring_config_t* cfg, ibu_stream_t** out) {
  if (!r || !ctx || !out) return err_arg("NULL argument");
  *out = nullptr;
  ibu_stream* s = new (std::nothrow) ibu_stream;
  if (!s) return err_io(ENOMEM, "ibu_stream_open_reader");
  s->rd = r;
  ibu_reader_header(r, &s->header);
  const int32_t rc = stream_open(ctx, cfg, s);
  if (rc) { delete s; return rc; }
  *out = s;
  return IBU_OK;
}

extern "C" int32_t ibu_stream_open_mmap(const ibu_mmap_t* m, ibu_ctx_t* ctx, const ibu_ring_config_t* cfg, size_t shard,
                                        size_t n_shards, ibu_stream_t** out) {
  if (!m || !ctx || !out) return err_arg("NULL argument");
  *out = nullptr;
  size_t start = 0, end = 0;
  int32_t rc = ibu_shard_range(ibu_mmap_len(m), n_shards, shard, &start, &end);  // mmap.rs:297-307
  if (rc) return rc;
  ibu_stream* s = new (std::nothrow) ibu_stream;
  if (!s) return err_io(ENOMEM, "ibu_stream_open_mmap");
  s->m = m;
  s->start = start;
  s->end = end;
  s->first0 = start;
  ibu_mmap_header(m, &s->header);
  rc = stream_open(ctx, cfg, s);
  if (rc) { delete s; return rc; }
  *out = s;
  return IBU_OK;
}

// Reader::from_path + the pull stream (reader.rs:345-352): one descriptor, sniffed once.  A BGZF file the device load takes is read in ranges
// inflated on the device (produce_ranges); anything else goes through a Reader: ibu_stream_open_reader over ibu_reader_open_fd of that
// descriptor, or over the caller's Reader of the same file (ibu_reader_process_device).
namespace {
// The device form over s->own_fd: sniffed, mapped, indexed once, the ranges planned for the context's ring (ring_ensure first) and the
// inflate staging sized for the largest.  A header other than `want` (when given) is a refusal like any other.
int32_t index_and_plan(ibu_stream* s, ibu_ctx* ctx, const ibu_header_t* want) {
  struct stat st;
  if (fstat(s->own_fd, &st) || !S_ISREG(st.st_mode) || st.st_size < 18 || getenv("IBU_NO_PARALLEL_BGZF")) return IBU_ERR_NIFFLER;
  void* p = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, s->own_fd, 0);
  if (p == MAP_FAILED) return IBU_ERR_IO;
  s->file.reset(new FileMap);
  s->file->p = static_cast<const uint8_t*>(p);
  s->file->n = (size_t)st.st_size;
  const uint8_t* m = s->file->p;                           // the Reader's sniff: a BGZF block first
  if (!(m[0] == 0x1f && m[1] == 0x8b && m[2] == 8 && (m[3] & 4) && m[12] == 'B' && m[13] == 'C' && m[14] == 2 && m[15] == 0)) return IBU_ERR_NIFFLER;
  (void)madvise(const_cast<uint8_t*>(m), s->file->n, MADV_SEQUENTIAL);
  RunOnNode on_node(feed_place(ctx));
  if (int32_t rc = bgzf_index(m, s->file->n, &s->idx)) return rc;
  if (want && memcmp(&s->idx.header, want, sizeof *want) != 0) return IBU_ERR_NIFFLER;
  s->header = s->idx.header;
  const size_t total = (size_t)((s->idx.total - IBU_HEADER_SIZE) / IBU_RECORD_SIZE);
  const size_t target = ctx->bgzf_range_bytes_opt ? ctx->bgzf_range_bytes_opt : (size_t)3200000000ull;
  s->range_records = plan_range_records(s->idx, target, ctx->ring.slot_bytes / IBU_RECORD_SIZE);
  s->n_ranges = (total + s->range_records - 1) / s->range_records;
  size_t need = 0;                                         // the staging for the largest range, now: a load never grows it under the caller
  for (size_t k = 0; k < s->n_ranges; ++k) {
    ShardPlan plan;
    if (int32_t rc = range_plan(s, k, &plan)) return rc;
    size_t a, b, c, d;
    need = std::max(need, stage_bytes(ctx, plan, &a, &b, &c, &d));
  }
  if (s->n_ranges && need > ctx->inflate_stage_bytes) {
    (void)hipFree(ctx->d_inflate_stage);
    ctx->d_inflate_stage = nullptr;
    ctx->inflate_stage_bytes = 0;
    if (hipError_t e = ctx_malloc(ctx, &ctx->d_inflate_stage, need); e != hipSuccess) { ctx->d_inflate_stage = nullptr; return hip_fail(e, "hipMalloc"); }
    ctx->inflate_stage_bytes = need;
  }
  s->ranges = true;
  return IBU_OK;
}

// The same, or false: not for the device form (option "bgzf_device" = 0, no descriptor, anything index_and_plan refuses), as if it had not
// been tried: nothing kept, the error detail as it was
bool open_device_form(ibu_stream* s, ibu_ctx* ctx, const ibu_header_t* want) {
  if (!ctx->bgzf_device || s->own_fd < 0) return false;
  const ibu_error_detail_t keep = tls_error();
  int32_t rc = IBU_OK;
  try {
    rc = index_and_plan(s, ctx, want);
  } catch (...) {
    rc = caught_io("ibu_stream_open_path");
  }
  if (rc) {
    tls_error() = keep;
    s->file.reset();
    s->idx = BgzfIndex();
  }
  return rc == IBU_OK;
}

// A path stream over descriptor `fd` (-1: none), which it owns from here on (closed on a failure too).  `rd`: the caller's Reader of the
// same file, borrowed as the host path from record 0 and as the whole source where the device form does not take the file; NULL: a
// Reader of `fd` where needed.  The context's ring is sized already (ring_ensure).
int32_t open_path_stream(int fd, ibu_reader_t* rd, ibu_ctx* ctx, const ibu_ring_config_t* cfg, ibu_stream** out) {
  std::unique_ptr<ibu_stream> s(new (std::nothrow) ibu_stream);
  if (!s) {
    if (fd >= 0) close(fd);
    return err_io(ENOMEM, "ibu_stream_open_path");
  }
  s->own_fd = fd;
  struct Own { ibu_stream* s; ~Own() { if (s && s->own_rd) ibu_reader_close(s->own_rd); if (s && s->own_fd >= 0) close(s->own_fd); } } own{s.get()};   // (until the stream runs)
  if (cfg) s->cfg = *cfg;
  ibu_header_t want{};
  if (rd) ibu_reader_header(rd, &want);
  if (!open_device_form(s.get(), ctx, rd ? &want : nullptr)) {
    if (!rd) {
      if (int32_t rc = ibu_reader_open_fd(fd, &s->own_rd)) return rc;
      rd = s->own_rd;
    }
    ibu_reader_header(rd, &s->header);
  }
  s->rd = rd;
  if (int32_t rc = stream_open(ctx, cfg, s.get())) return rc;
  if (s->ranges) ctx->stage_lent = true;
  own.s = nullptr;
  *out = s.release();
  return IBU_OK;
}
}  // namespace

extern "C" int32_t ibu_stream_open_path(const char* path, ibu_ctx_t* ctx, const ibu_ring_config_t* cfg, ibu_stream_t** out) {
  if (!path || !ctx || !out) return err_arg("NULL argument");
  *out = nullptr;
  IBU_HIP(hipSetDevice(ctx->device));
  if (int32_t rc = ring_ensure(ctx, cfg, false)) return rc;   // (a ring lent to another stream: refused before the file is touched)
  const int fd = ::open(path, O_RDONLY | O_CLOEXEC);
  if (fd < 0) return err_io(errno, path);
  return open_path_stream(fd, nullptr, ctx, cfg, out);
}

extern "C" int32_t ibu_stream_header(const ibu_stream_t* s, ibu_header_t* out) {
  if (!s || !out) return err_arg("NULL argument");
  *out = s->header;
  return IBU_OK;
}

extern "C" int32_t ibu_stream_next(ibu_stream_t* s, void* stream, const void** d_records, size_t* n, uint64_t* first_index) {
  if (!s || !d_records || !n) return err_arg("NULL argument");
  *d_records = nullptr;
  *n = 0;
  if (!s->ctx) return err_arg("the stream's context has been destroyed");
  IBU_HIP(hipSetDevice(s->ctx->device));
  ibu_stream::Batch b;
  const int32_t rc = stream_take(s, pick_stream(s->ctx, stream), &b);
  if (rc || b.n == 0) return rc;
  *d_records = b.p;
  *n = b.n;
  if (first_index) *first_index = b.first;
  return IBU_OK;
}

extern "C" int32_t ibu_stream_release(ibu_stream_t* s, const void* d_records, void* stream) {
  if (!s || !d_records) return err_arg("NULL argument");
  if (!s->ctx) return err_arg("the stream's context has been destroyed");
  IBU_HIP(hipSetDevice(s->ctx->device));
  Ring& r = s->ctx->ring;
  ibu_stream::Batch b;
  {
    std::lock_guard<std::mutex> g(s->mu);
    for (const ibu_stream::Batch& h : s->rheld)
      if (h.p == d_records) b = h;
    for (uint32_t i = 0; i < r.dev.size() && !b.p; ++i)
      if (r.dev[i] == d_records && s->slot[i].state == ibu_stream::HELD) {
        b.p = r.dev[i];
        b.slot = (int)i;
      }
  }
  if (!b.p) return err_arg("not a batch this stream handed out and still holds");
  return stream_give_back(s, b, pick_stream(s->ctx, stream));
}

extern "C" int32_t ibu_stream_stats(const ibu_stream_t* s, ibu_stream_stats_t* out) {
  if (!s || !out) return err_arg("NULL argument");
  ibu_stream* m = const_cast<ibu_stream*>(s);
  std::lock_guard<std::mutex> g(m->mu);
  *out = m->stats;
  out->seconds_total = now_s() - m->t0;
  return IBU_OK;
}

extern "C" void ibu_stream_close(ibu_stream_t* s) {
  if (!s) return;
  if (s->ctx) stream_shutdown(s);    // (an orphan — its context was destroyed first — has been shut down already)
  delete s;
}
// ibu_ctx_destroy under an open stream: the producer is stopped and joined and the ring given back BEFORE the context frees it; the
// handle stays valid for ibu_stream_close (every other call on it reports the destroyed context).
void ibu::stream_orphan(ibu_ctx* ctx) {
  ibu_stream* s = static_cast<ibu_stream*>(ctx->ring_lent);
  if (!s) return;
  stream_shutdown(s);
  s->ctx = nullptr;
}

// ------------------------------------------------------------------------------------------
// The two built-in device processors over the pull stream: process_parallel (mmap.rs:286-332, one shard of the static split)
// and the streaming Reader (reader.rs:279-306, :345-352), device forms
// ------------------------------------------------------------------------------------------
namespace {
int32_t run_processor(ibu_stream* s, int32_t proc, void* sink, ibu_stream_stats_t* stats) {
  ibu_ctx* ctx = s->ctx;
  Ring& r = ctx->ring;
  DeviceProc dp;
  int32_t rc = make_proc(ctx, proc, s->header, sink, &dp);
  if (rc) return rc;
  KernelClock kc;
  rc = kc.init(r.slots);
  if (rc) return rc;
  if (proc == IBU_PROC_REDUCE) IBU_HIP(hipMemsetAsync(ctx->d_acc, 0, kReduceAccBytes, ctx->stream));
  for (uint64_t seq = 0;; ++seq) {
    ibu_stream::Batch b;
    rc = stream_take(s, ctx->stream, &b);
    if (rc || b.n == 0) break;
    const size_t row0 = (size_t)(b.first - s->first0);
    rc = dp.fits(b.n, row0);         // a gzip / BGZF / xz / zstd stream does not announce its length: every batch is checked
    if (rc == IBU_OK) {
      // the clock's pair of a ring batch is its slot's: the slot's previous kernel finished before the producer refilled it, no wait.
      // A range's batches take the pairs in turn (harvesting one waits for the kernel slots batches back)
      const uint32_t k = b.slot >= 0 ? (uint32_t)b.slot : (uint32_t)(seq % r.slots);
      kc.harvest(k);
      hipError_t e = hipEventRecord(kc.a[k], ctx->stream);
      if (e == hipSuccess) {
        rc = dp.launch(b.p, b.n, row0);
        if (rc == IBU_OK) e = hipEventRecord(kc.b[k], ctx->stream);
      }
      if (rc == IBU_OK && e != hipSuccess) rc = hip_fail(e, "hipEventRecord");
      if (rc == IBU_OK) kc.live[k] = 1;
    }
    const int32_t rel = stream_give_back(s, b, ctx->stream);
    if (rc == IBU_OK) rc = rel;
    if (rc) break;
  }
  if (rc) return rc;
  if (proc == IBU_PROC_REDUCE) rc = ibu_reduce_fetch(ctx, ctx->stream, static_cast<ibu_reduce_result_t*>(sink));
  else if (hipError_t e = hipStreamSynchronize(ctx->stream); e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize");
  if (rc) return rc;
  for (uint32_t i = 0; i < r.slots; ++i) kc.harvest(i);
  if (stats) {
    std::lock_guard<std::mutex> g(s->mu);
    *stats = s->stats;
    stats->seconds_kernel = kc.ms * 1e-3;
  }
  return IBU_OK;
}
// open -> run -> close, with the error (and its detail) of the first failing step; *records (nullable): the records delivered
int32_t process_stream(ibu_stream* s, int32_t open_rc, int32_t proc, void* sink, ibu_stream_stats_t* stats, double t0,
                       uint64_t* records = nullptr) {
  if (open_rc) return open_rc;
  const int32_t rc = run_processor(s, proc, sink, stats);
  if (records) {
    std::lock_guard<std::mutex> g(s->mu);
    *records = s->stats.records;
  }
  const ibu_error_detail_t keep = tls_error();
  ibu_stream_close(s);               // drains the copy stream and the context's stream: nothing is in flight over ring memory
  if (rc) { tls_error() = keep; return rc; }
  if (stats) stats->seconds_total = now_s() - t0;
  return IBU_OK;
}
}  // namespace

extern "C" int32_t ibu_mmap_process_device(const ibu_mmap_t* m, ibu_ctx_t* ctx, const ibu_ring_config_t* cfg,
                                           int32_t proc, size_t shard, size_t n_shards, void* sink,
                                           ibu_stream_stats_t* stats) {
  if (!m || !ctx) return err_arg("NULL argument");
  const double t0 = now_s();
  if (stats) memset(stats, 0, sizeof *stats);
  size_t start = 0, end = 0;
  int32_t rc = ibu_shard_range(ibu_mmap_len(m), n_shards, shard, &start, &end);  // mmap.rs:297-307
  if (rc) return rc;
  ibu_header_t h;
  ibu_mmap_header(m, &h);
  DeviceProc dp;
  rc = make_proc(ctx, proc, h, sink, &dp);
  if (rc) return rc;
  rc = dp.fits(end - start, 0);   // the shard's size is known up front: refused before any work starts
  if (rc) return rc;
  ibu_stream_t* s = nullptr;
  rc = ibu_stream_open_mmap(m, ctx, cfg, shard, n_shards, &s);
  return process_stream(s, rc, proc, sink, stats, t0);
}

// ------------------------------------------------------------------------------------------
// MmapReader::process_parallel across DEVICES in one call (mmap.rs:286-332 with a GPU per worker)
// ------------------------------------------------------------------------------------------
// The reference's loop: n workers, worker i owns shard i of the static split (mmap.rs:297-307), workers are joined in spawn
// order and the first Err in that order is the call's result (quirk Q12).  Here a worker is one host thread driving one
// context (= one device): ibu_mmap_process_device(m, ctx_i, cfg, proc, i, n, sink_i).  No data-path collective exists: the
// only cross-device value is the reduce processor's {count, 3 wrapping sums, 3 XORs}, seven words per device, added on the
// host by the calling thread once the workers are joined (latency-bound, the xGMI links play no part).
// A worker's error detail lives in ITS thread's slot; the winner's is copied into the caller's.
namespace {
int32_t process_contexts(const ibu_mmap_t* m, ibu_ctx_t* const* ctxs, size_t n, const ibu_ring_config_t* cfg, int32_t proc,
                         void* sinks, ibu_reduce_result_t* total, ibu_stream_stats_t* stats) {
  if (proc != IBU_PROC_REDUCE && proc != IBU_PROC_DECODE) return err_arg("unknown device processor");
  if (proc == IBU_PROC_DECODE && !sinks) return err_arg("IBU_PROC_DECODE needs one ibu_decode_sink_t per device");
  std::vector<int32_t> rc;
  std::vector<ibu_error_detail_t> detail;
  std::vector<ibu_reduce_result_t> part;
  try {
    rc.assign(n, IBU_OK);
    detail.resize(n);
    part.resize(n);
  } catch (...) {
    return caught_io("ibu_mmap_process_devices");
  }
  for (auto& r : part) memset(&r, 0, sizeof r);
  run_pieces((unsigned)n, [&](unsigned i) {     // never throws; a thread that cannot start runs on the caller (common.hpp)
    void* sink = proc == IBU_PROC_REDUCE ? static_cast<void*>(&part[i]) : static_cast<void*>(static_cast<ibu_decode_sink_t*>(sinks) + i);
    rc[i] = ibu_mmap_process_device(m, ctxs[i], cfg, proc, i, n, sink, stats ? stats + i : nullptr);
    if (rc[i] != IBU_OK) detail[i] = tls_error();
  });
  for (size_t i = 0; i < n; ++i)
    if (rc[i] != IBU_OK) {                      // first error in worker order (mmap.rs:326-328)
      tls_error() = detail[i];
      return rc[i];
    }
  ibu_reduce_result_t t;
  memset(&t, 0, sizeof t);
  if (proc == IBU_PROC_REDUCE) {
    for (size_t i = 0; i < n; ++i) {
      t.count += part[i].count;
      for (int f = 0; f < 3; ++f) { t.sum[f] += part[i].sum[f]; t.xor_[f] ^= part[i].xor_[f]; }   // wrapping (mod 2^64), as the device adds
    }
    if (sinks) memcpy(sinks, part.data(), n * sizeof(ibu_reduce_result_t));
  } else {
    t.count = ibu_mmap_len(m);                  // every shard decoded: the whole map
  }
  if (total) *total = t;
  return IBU_OK;
}
}  // namespace

extern "C" int32_t ibu_mmap_process_contexts(const ibu_mmap_t* m, ibu_ctx_t* const* ctxs, size_t n_ctxs, const ibu_ring_config_t* cfg,
                                             int32_t proc, void* sinks, ibu_reduce_result_t* total, ibu_stream_stats_t* stats) {
  if (!m || !ctxs || n_ctxs == 0) return err_arg("NULL argument or no context");
  if (n_ctxs > 1024) return err_arg("more than 1024 contexts");
  for (size_t i = 0; i < n_ctxs; ++i) {
    if (!ctxs[i]) return err_arg("a context is NULL");
    for (size_t j = 0; j < i; ++j)
      if (ctxs[j] == ctxs[i]) return err_arg("the same context twice (a context serves one host thread; create two on one device instead)");
  }
  return process_contexts(m, ctxs, n_ctxs, cfg, proc, sinks, total, stats);
}

extern "C" int32_t ibu_mmap_process_devices(const ibu_mmap_t* m, const int32_t* devices, size_t n_devices, const ibu_ring_config_t* cfg,
                                            int32_t proc, void* sinks, ibu_reduce_result_t* total, ibu_stream_stats_t* stats) {
  if (!m) return err_arg("NULL argument");
  std::vector<int32_t> all;
  std::vector<ibu_ctx_t*> ctxs;
  try {
    if (n_devices == 0) {                       // "0 = all of them", as num_threads == 0 means all cores (mmap.rs:292-296)
      int32_t c = 0;
      int32_t rc = ibu_device_count(&c);
      if (rc) return rc;
      if (c <= 0) return set_error(IBU_ERR_NO_DEVICE, 0, 0, 0, "no HIP device visible");
      for (int32_t d = 0; d < c; ++d) all.push_back(d);
      devices = all.data();
      n_devices = all.size();
    } else if (!devices) {
      return err_arg("devices is NULL");
    }
    if (n_devices > 1024) return err_arg("more than 1024 devices");
    ctxs.assign(n_devices, nullptr);
  } catch (...) {
    return caught_io("ibu_mmap_process_devices");
  }
  // The contexts of this form live for ONE call, so their rings are allocated and pinned inside it: 4 x 96 MiB (the default
  // of a kept context) costs 70 ms per context — more than streaming an eighth of a 24 GB file — and pinning serialises in
  // the driver.  Without a caller's ring configuration the one-shot form uses 3 x 24 MiB slots (1 Mi records, the
  // reference's BATCH_SIZE, mmap.rs:284): 18 ms, 54.5 GB/s against 56.1 (profiles/README.md r03_y).
  ibu_ring_config_t one_shot;
  memset(&one_shot, 0, sizeof one_shot);
  one_shot.slots = 3;
  one_shot.slot_records = IBU_BATCH_SIZE;
  if (!cfg) cfg = &one_shot;
  int32_t rc = IBU_OK;
  for (size_t i = 0; i < n_devices && rc == IBU_OK; ++i) rc = ibu_ctx_create(devices[i], &ctxs[i]);   // in order: the first bad ordinal is the error
  if (rc == IBU_OK) rc = process_contexts(m, ctxs.data(), n_devices, cfg, proc, sinks, total, stats);
  const ibu_error_detail_t keep = tls_error();
  for (ibu_ctx_t* c : ctxs) ibu_ctx_destroy(c);
  if (rc != IBU_OK) tls_error() = keep;
  return rc;
}

// ------------------------------------------------------------------------------------------
// streaming Reader (plain / gzip), device form
// ------------------------------------------------------------------------------------------
// A Reader over a BGZF FILE nothing has been read from: the processors need not pull it through the Reader's host inflate (0.4 G records/s
// on 16 CPUs) — the path stream's device form reads the Reader's own file (a descriptor of its own, through /proc/self/fd: the Reader's
// position never moves, and a name renamed or replaced since does not matter) with the Reader as its host path from record 0.  A file
// that form does not take, or a descriptor that will not open, goes through the Reader's own path, error and all.
extern "C" int32_t ibu_reader_process_device(ibu_reader_t* rd, ibu_ctx_t* ctx, const ibu_ring_config_t* cfg,
                                             int32_t proc, void* sink, ibu_stream_stats_t* stats) {
  if (!rd || !ctx) return err_arg("NULL argument");
  const double t0 = now_s();
  if (stats) memset(stats, 0, sizeof *stats);
  ibu_header_t h;
  ibu_reader_header(rd, &h);
  DeviceProc dp;
  int32_t rc = make_proc(ctx, proc, h, sink, &dp);   // argument errors before the producer thread exists
  if (rc) return rc;
  ibu_stream_t* s = nullptr;
  const int bgzf_fd = ctx->bgzf_device ? reader_bgzf_fd_if_untouched(rd) : -1;
  if (bgzf_fd < 0) {
    rc = ibu_stream_open_reader(rd, ctx, cfg, &s);
    return process_stream(s, rc, proc, sink, stats, t0);
  }
  IBU_HIP(hipSetDevice(ctx->device));
  if ((rc = ring_ensure(ctx, cfg, false))) return rc;
  char name[40];
  snprintf(name, sizeof name, "/proc/self/fd/%d", bgzf_fd);
  rc = open_path_stream(::open(name, O_RDONLY | O_CLOEXEC), rd, ctx, cfg, &s);
  const bool device = rc == IBU_OK && s->ranges;
  uint64_t records = 0;
  rc = process_stream(s, rc, proc, sink, stats, t0, &records);
  if (rc == IBU_OK && device) reader_set_drained(rd, records);   // (the host path may have been a Reader of its own from a later range on)
  return rc;
}
