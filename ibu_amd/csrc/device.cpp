// device.cpp — device context and the kernel entry points of the C ABI (include/ibu_hip.h).
//
// Every function here fails loudly (IBU_ERR_NO_DEVICE / IBU_ERR_HIP) when there is no gfx950
// device; nothing falls back to host arithmetic.  Launch functions are asynchronous, allocate
// nothing and never synchronise, so callers may capture them into hipGraphs.
#include <stdlib.h>
#include <stddef.h>
#include <string.h>

#include <chrono>
#include <utility>
#include <vector>

#include <cstddef>
#include "bgzf_plan.hpp"
#include "ctx.hpp"

using namespace ibu;

namespace {

int32_t check_ctx(const ibu_ctx* ctx) {
  if (!ctx) return err_arg("ctx is NULL");
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
  return IBU_OK;
}
int32_t check_lens(uint32_t bc_len, uint32_t umi_len) {  // header.rs:180-185
  if (bc_len == 0 || bc_len > 32) return err_bc_len(bc_len);
  if (umi_len == 0 || umi_len > 32) return err_umi_len(umi_len);
  return IBU_OK;
}
bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

extern "C" int32_t ibu_device_count(int32_t* n) {
  if (!n) return err_arg("n is NULL");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    *n = 0;
    return hip_fail(e, "hipGetDeviceCount");
  }
  *n = c;
  return IBU_OK;
}

extern "C" int32_t ibu_ctx_create(int32_t device, ibu_ctx_t** out) {
  if (!out) return err_arg("out is NULL");
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
  if (device < 0 || device >= count)
    return set_error(IBU_ERR_NO_DEVICE, 0, 0, 0, "device %d not present (%d visible)", device, count);
  IBU_HIP(hipSetDevice(device));
  hipDeviceProp_t prop;
  IBU_HIP(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return set_error(IBU_ERR_NO_DEVICE, 0, 0, 0, "device %d is %s; this library carries gfx950 code objects only",
                     device, prop.gcnArchName);
  ibu_ctx* ctx = new ibu_ctx;
  ctx->device = device;
  ctx->cfg.cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  // blocks_per_cu keeps LaunchCfg's measured default; ibu_ctx_set_option overrides it
  static const int trace_rows_env = [] { const char* v = getenv("IBU_TRACE_ROWS"); return (v && *v && *v != '0') ? 1 : 0; }();   // read once
  ctx->cfg.trace_rows = trace_rows_env;
  // Where the device hangs off the host (numa.hpp): feeds the ring's placement and the feeder threads' affinity (option "numa").
  // IBU_SYSFS_ROOT: a test tree instead of /sys.  Failure of any step leaves node -1: nothing is pinned, as before round 5.
  if (hipDeviceGetPCIBusId(ctx->pci_bus_id, (int)sizeof ctx->pci_bus_id, device) == hipSuccess)
    numa_lookup(getenv("IBU_SYSFS_ROOT"), ctx->pci_bus_id, nullptr, &ctx->place);
  else
    (void)hipGetLastError();
  hipError_t rc = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
  if (rc == hipSuccess) rc = hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking);
  if (rc == hipSuccess) rc = hipStreamCreateWithFlags(&ctx->d2h_stream, hipStreamNonBlocking);
  if (rc == hipSuccess) rc = hipMalloc(reinterpret_cast<void**>(&ctx->d_status), 2 * sizeof(uint64_t));
  if (rc == hipSuccess) rc = hipMalloc(reinterpret_cast<void**>(&ctx->d_acc), kReduceAccBytes);
  if (rc == hipSuccess) rc = hipMalloc(reinterpret_cast<void**>(&ctx->d_flag), 16);
  if (rc == hipSuccess) rc = hipHostMalloc(reinterpret_cast<void**>(&ctx->h_pinned), 128 * sizeof(uint64_t), hipHostMallocDefault);
  if (rc == hipSuccess) rc = hipMemsetAsync(ctx->d_acc, 0, kReduceAccBytes, ctx->stream);
  if (rc == hipSuccess) rc = launch_fill2(ctx->d_status, ~0ull, 0, ctx->stream);
  if (rc == hipSuccess) rc = hipStreamSynchronize(ctx->stream);
  if (rc != hipSuccess) {
    ibu_ctx_destroy(ctx);
    return hip_fail(rc, "ibu_ctx_create");
  }
  *out = ctx;
  return IBU_OK;
}

extern "C" void ibu_ctx_destroy(ibu_ctx_t* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->ring_lent) stream_orphan(ctx);   // a stream still open on this context: stop its producer before the ring goes
  if (ctx->loser_free.joinable()) ctx->loser_free.join();
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);
  if (ctx->d2h_stream) (void)hipStreamSynchronize(ctx->d2h_stream);
  ring_release(ctx);
  codec_ring_release(ctx);
  for (hipStream_t ps : ctx->pull_streams) { (void)hipStreamSynchronize(ps); (void)hipStreamDestroy(ps); }
  for (hipEvent_t pe : ctx->pull_events) (void)hipEventDestroy(pe);
  if (ctx->d_sort_scratch) (void)hipFree(ctx->d_sort_scratch);
  if (ctx->d_runs_scratch) (void)hipFree(ctx->d_runs_scratch);
  if (ctx->d_status) (void)hipFree(ctx->d_status);
  if (ctx->d_acc) (void)hipFree(ctx->d_acc);
  if (ctx->d_flag) (void)hipFree(ctx->d_flag);
  if (ctx->d_correct_acc) (void)hipFree(ctx->d_correct_acc);
  if (ctx->d_resolve_acc) (void)hipFree(ctx->d_resolve_acc);
  if (ctx->h_pinned) (void)hipHostFree(ctx->h_pinned);
  if (ctx->h_part) (void)hipHostFree(ctx->h_part);
  if (ctx->side_stream) (void)hipStreamDestroy(ctx->side_stream);
  for (hipStream_t q : ctx->inflate_streams)
    if (q) (void)hipStreamDestroy(q);
  if (ctx->d_inflate_stage) (void)hipFree(ctx->d_inflate_stage);
  for (void* p : ctx->d_range_buf)
    if (p) (void)hipFree(p);
  if (ctx->h_inflate_marks) (void)hipHostFree(ctx->h_inflate_marks);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
  if (ctx->d2h_stream) (void)hipStreamDestroy(ctx->d2h_stream);
  delete ctx;
}
extern "C" int32_t ibu_ctx_set_option(ibu_ctx_t* ctx, const char* key, int64_t value) {
  if (!ctx || !key) return err_arg("ctx or key is NULL");
  if (strcmp(key, "blocks_per_cu") == 0) {
    if (value < 1 || value > 8) return err_arg("blocks_per_cu must be 1..8");
    ctx->cfg.blocks_per_cu = (int)value;
    return IBU_OK;
  }
  if (strcmp(key, "sort_variant") == 0) {
    if (value < 0 || value >= sort_num_variants()) return err_arg("sort_variant out of range");
    ctx->cfg.sort_variant = (int)value;
    return IBU_OK;
  }
  if (strcmp(key, "sort_guess") == 0) {
    if (value < 0 || value > (1ll << 31)) return err_arg("sort_guess out of range");
    ctx->cfg.sort_guess = (int)value;
    return IBU_OK;
  }
  if (strcmp(key, "sort_hybrid") == 0) {
    if (value < 0 || value > 2) return err_arg("sort_hybrid must be 0, 1 or 2");
    ctx->cfg.sort_hybrid = (int)value;
    return IBU_OK;
  }
  if (strcmp(key, "sort_idx64") == 0) {
    if (value != 0 && value != 1) return err_arg("sort_idx64 must be 0 or 1");
    ctx->cfg.sort_idx64 = (int)value;
    return IBU_OK;
  }
  if (strcmp(key, "sort_compact") == 0) {
    if (value < 0 || value > sort_num_compact_variants()) return err_arg("sort_compact out of range");
    ctx->cfg.sort_compact = (int)value;
    return IBU_OK;
  }
  if (strcmp(key, "alloc_probe_tries") == 0) {
    if (value < 0 || value > IBU_ALLOC_PROBE_MAX) return err_arg("alloc_probe_tries must be 0 (auto) .. 16");
    ctx->cfg.alloc_probe_tries = (int)value;
    if (ctx->loser_free.joinable()) ctx->loser_free.join();   // (documented: setting the option waits for candidates still being freed)
    return IBU_OK;
  }
  if (strcmp(key, "inflate_one_launch") == 0) {          // a test knob: the block count from which a BGZF load launches its decoder ahead of the copies
    if (value < 0 || value > (int64_t)inflate_one_round(ctx->cfg.cus)) return err_arg("inflate_one_launch must be 0 (default) .. one round of the decoder's short form");
    ctx->inflate_one_launch = (size_t)value;
    return IBU_OK;
  }
  if (strcmp(key, "bgzf_range_bytes") == 0) {            // a test knob: the ranges of a path stream's device form (also under ibu_reader_process_device)
    if (value < 0) return err_arg("bgzf_range_bytes must be >= 0");
    ctx->bgzf_range_bytes_opt = (size_t)value;
    return IBU_OK;
  }
  if (strcmp(key, "bgzf_device") == 0) {
    if (value != 0 && value != 1) return err_arg("bgzf_device must be 0 or 1");
    ctx->bgzf_device = (int)value;
    return IBU_OK;
  }
  if (strcmp(key, "bgzf_stream_ahead") == 0) {           // the launch form of a path stream's ranges after the first
    if (value != 0 && value != 1) return err_arg("bgzf_stream_ahead must be 0 or 1");
    ctx->bgzf_stream_ahead = (int)value;
    return IBU_OK;
  }
  if (strcmp(key, "load_piece_delay_ms") == 0) {         // a test knob: a slow source for the BGZF loads
    if (value < 0 || value > 10000) return err_arg("load_piece_delay_ms must be 0 .. 10000");
    ctx->load_piece_delay_ms = (uint32_t)value;
    return IBU_OK;
  }
  if (strcmp(key, "release_staging") == 0) {             // one-shot: the device staging the BGZF loads keep (the compressed file's size, the range buffers) goes back now
    if (value != 1) return err_arg("release_staging must be 1");
    if (ctx->stage_lent) return err_arg("an open ibu_stream_open_path stream loads through the staging: close it first");
    IBU_HIP(hipSetDevice(ctx->device));
    for (hipStream_t q : ctx->inflate_streams)
      if (q) IBU_HIP(hipStreamSynchronize(q));
    if (ctx->d_inflate_stage) IBU_HIP(hipFree(ctx->d_inflate_stage));
    ctx->d_inflate_stage = nullptr;
    ctx->inflate_stage_bytes = 0;
    for (int b = 0; b < 2; ++b) {
      if (ctx->d_range_buf[b]) IBU_HIP(hipFree(ctx->d_range_buf[b]));
      ctx->d_range_buf[b] = nullptr;
      ctx->range_buf_bytes[b] = 0;
    }
    return IBU_OK;
  }
  if (strcmp(key, "sort_pull_streams") == 0) {
    if (value != 0 && value != 1) return err_arg("sort_pull_streams must be 0 or 1");
    ctx->force_pull_streams = (int)value;
    return IBU_OK;
  }
  if (strcmp(key, "peer_access") == 0) {
    if (value != 0 && value != 1) return err_arg("peer_access must be 0 or 1");
    ctx->peer_access = (int)value;
    return IBU_OK;
  }
  if (strcmp(key, "numa") == 0) {
    if (value != 0 && value != 1) return err_arg("numa must be 0 (off) or 1 (auto)");
    ctx->numa_mode = (int)value;
    return IBU_OK;
  }
  if (strcmp(key, "trace_rows") == 0) {
    ctx->cfg.trace_rows = value != 0;
    return IBU_OK;
  }
  if (strcmp(key, "base_order") == 0) {
    if (value != IBU_BASE_ORDER_LSB_FIRST && value != IBU_BASE_ORDER_MSB_FIRST) return err_arg("base_order must be 0 (LSB first) or 1 (MSB first)");
    ctx->cfg.base_order = (uint32_t)value;
    return IBU_OK;
  }
  return err_arg("unknown option key");
}
extern "C" int32_t ibu_ctx_device(const ibu_ctx_t* ctx) { return ctx ? ctx->device : -1; }
extern "C" int32_t ibu_ctx_numa(const ibu_ctx_t* ctx, ibu_numa_info_t* out) {
  if (!ctx || !out) return err_arg("ctx or out is NULL");
  memset(out, 0, sizeof *out);
  out->mode = ctx->numa_mode;
  out->node = ctx->place.node;
  out->usable_cpus = ctx->place.ncpus;
  out->ring_node = ctx->ring.slots ? ctx->ring.node : -1;
  out->ring_placed = ctx->ring.slots && ctx->ring.placed ? 1 : 0;
  snprintf(out->pci_bus_id, sizeof out->pci_bus_id, "%s", ctx->pci_bus_id);
  snprintf(out->cpulist, sizeof out->cpulist, "%s", ctx->place.cpulist);
  return IBU_OK;
}
extern "C" void* ibu_ctx_stream(const ibu_ctx_t* ctx) { return ctx ? ctx->stream : nullptr; }
extern "C" int32_t ibu_ctx_synchronize(ibu_ctx_t* ctx, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  IBU_HIP(hipStreamSynchronize(pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_device_alloc(ibu_ctx_t* ctx, size_t bytes, void** d_ptr) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!d_ptr) return err_arg("d_ptr is NULL");
  return ibu::ctx_alloc(ctx, bytes, d_ptr);
}
// Long-lived device memory the library allocates for a caller: with the context option "alloc_probe_tries" > 1, arrays of at least
// 256 MiB go through the placement probing below (smaller ones are not worth the candidates' time: the ring's slots, scratch).
// Option "alloc_probe_tries": how many candidates an allocation of `bytes` draws.  Auto (0) probes only what is worth it and
// cannot hurt: at least 1 GiB (the arrays whose placement the streaming kernels feel; smaller ones are ring slots and scratch
// tables) and at least three candidates fitting the free memory at once (so that the candidates never push a caller out of memory).
static int32_t alloc_probed_impl(ibu_ctx_t* ctx, size_t bytes, uint32_t tries, void** d_ptr, ibu_alloc_probe_t* report, double alloc_budget_ms,
                                 double* slow_ms);
static uint32_t probe_tries_for(const ibu_ctx* ctx, size_t bytes) {
  const int t = ctx->cfg.alloc_probe_tries;
  if (t == 1) return 1;
  if (t > 1) return bytes >= ((size_t)256 << 20) ? (uint32_t)t : 1u;
  if (bytes < ((size_t)1 << 30)) return 1;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return 1; }
  const size_t fit = free_b / bytes;
  return fit < 3 ? 1u : (fit < 4 ? (uint32_t)fit : 4u);
}
hipError_t ibu::ctx_malloc(ibu_ctx* ctx, void** p, size_t bytes) {
  hipError_t e = hipMalloc(p, bytes ? bytes : 16);
  if (e == hipErrorOutOfMemory && ctx->loser_free.joinable()) {
    (void)hipGetLastError();
    ctx->loser_free.join();
    e = hipMalloc(p, bytes ? bytes : 16);
    if (trace_sort()) fprintf(stderr, "ibu alloc: %zu bytes did not fit while candidates were being freed: waited for them, %s\n", bytes, e == hipSuccess ? "fits now" : "still does not fit");
  }
  return e;
}
int32_t ibu::ctx_alloc(ibu_ctx* ctx, size_t bytes, void** d_ptr) {
  const uint32_t tries = probe_tries_for(ctx, bytes);
  if (tries > 1) {
    ibu_alloc_probe_t rep;
    // auto: a candidate may take 10 ms + 2 ms per GB to allocate (the runtime's usual 0.1-1 ms with a wide margin); beyond that the
    // driver is busy handing out cleared memory and drawing more candidates would multiply the wait, not the choice
    const double budget = ctx->cfg.alloc_probe_tries == 0 ? 10.0 + 2.0 * ((double)bytes / 1e9) : 0.0;
    double slow = 0;
    const int32_t rc = alloc_probed_impl(ctx, bytes, tries, d_ptr, &rep, budget, &slow);
    if (rc == IBU_OK && trace_sort()) {
      if (rep.tries > 1) {
        fprintf(stderr, "ibu alloc: %zu bytes probed: %u candidates, kept #%u (ms:", bytes, rep.tries, rep.chosen);
        for (uint32_t k = 0; k < rep.tries; ++k) fprintf(stderr, " %.3f", rep.ms[k]);
        fprintf(stderr, ")%s\n", slow > 0 ? "; the drawing stopped at a slow allocation" : "");
      } else {
        fprintf(stderr, "ibu alloc: %zu bytes not probed: the allocation took %.1f ms (the driver is handing out memory slowly)\n", bytes, slow);
      }
    }
    return rc;
  }
  IBU_HIP(ctx_malloc(ctx, d_ptr, bytes));
  return IBU_OK;
}
// Placement probing behind the ABI (round 3; bench.py did this in Python in round 2).  On this part the rate of a streaming
// kernel depends on WHERE the driver put an array's physical pages (the same kernel runs 9.4 ... 11.3 ms from one allocation to
// the next; the rate belongs to the physical region and an allocation keeps it for as long as it lives: profiles/README.md
// r02_ag).  A caller that keeps an array resident can therefore choose: allocate `tries` candidates — all held at once, so that
// the allocator has to hand out different pages —, stream a write and a read over each (the write-only generator kernel and the
// read-only reduce kernel over the whole range, timed with events on the context's stream, second run of two), keep the
// fastest, free the rest.  Allocation stops quietly at the first candidate that does not fit.  The contents are unspecified.
// alloc_budget_ms > 0 (the auto mode): a candidate whose hipMalloc took longer than that ends the drawing — what costs in probing is
// not the measuring (0.8 ms per GB and candidate) but the driver handing out memory slowly (right after large frees it clears VRAM:
// seconds for 24 GB, profiles/README.md r05_h), and every further candidate would pay that again.  *slow_ms: that allocation's time.
static int32_t alloc_probed_impl(ibu_ctx_t* ctx, size_t bytes, uint32_t tries, void** d_ptr, ibu_alloc_probe_t* report, double alloc_budget_ms,
                                 double* slow_ms) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!d_ptr) return err_arg("d_ptr is NULL");
  if (slow_ms) *slow_ms = 0;
  if (report) memset(report, 0, sizeof *report);
  if (tries < 1) tries = 1;
  if (tries > IBU_ALLOC_PROBE_MAX) tries = IBU_ALLOC_PROBE_MAX;
  const size_t nrec = bytes / IBU_RECORD_SIZE;
  if (nrec < 4096) tries = 1;                   // nothing to measure on a few kilobytes
  void* cand[IBU_ALLOC_PROBE_MAX] = {nullptr};
  float ms[IBU_ALLOC_PROBE_MAX] = {0};
  uint32_t got = 0;
  for (; got < tries; ++got) {
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t e = got == 0 ? ctx_malloc(ctx, &cand[got], bytes) : hipMalloc(&cand[got], bytes ? bytes : 16);   // (further candidates: what fits now)
    if (e != hipSuccess) {
      (void)hipGetLastError();
      cand[got] = nullptr;
      if (got == 0) return hip_fail(e, "hipMalloc");
      break;                                    // the candidates that exist are the field
    }
    const double ms_alloc = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (trace_sort() && tries > 1) fprintf(stderr, "ibu alloc: candidate %u of %zu bytes: hipMalloc %.2f ms\n", got, bytes, ms_alloc);
    if (alloc_budget_ms > 0 && ms_alloc > alloc_budget_ms) {   // the driver is slow right now: no further candidates
      if (slow_ms) *slow_ms = ms_alloc;
      ++got;
      break;
    }
  }
  uint32_t best = 0;
  if (got > 1) {
    // The read half of the probe is the reduce kernel; it accumulates into a PRIVATE scratch accumulator, never into ctx->d_acc:
    // reset; {load_to_device; reduce} x N; fetch must add up over all N files whether or not the loads were probed.
    hipEvent_t e0 = nullptr, e1 = nullptr;
    uint64_t* d_probe_acc = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d_probe_acc), kReduceAccBytes);
    if (e == hipSuccess) e = hipMemsetAsync(d_probe_acc, 0, kReduceAccBytes, ctx->stream);
    for (uint32_t k = 0; k < got && e == hipSuccess; ++k)
      for (int run = 0; run < 2 && e == hipSuccess; ++run) {   // the first run touches the pages' translations
        e = hipEventRecord(e0, ctx->stream);
        if (e == hipSuccess) e = launch_generate(ctx->cfg, 0x1B0, 0, nrec, 32, 32, cand[k], ctx->stream);
        if (e == hipSuccess) e = launch_reduce(ctx->cfg, cand[k], nrec, d_probe_acc, ctx->stream);
        if (e == hipSuccess) e = hipEventRecord(e1, ctx->stream);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms[k], e0, e1);
      }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (d_probe_acc) (void)hipFree(d_probe_acc);
    if (e != hipSuccess) {
      for (uint32_t k = 0; k < got; ++k) (void)hipFree(cand[k]);
      return hip_fail(e, "ibu_device_alloc_probed");
    }
    for (uint32_t k = 1; k < got; ++k)
      if (ms[k] < ms[best]) best = k;
    // The candidates not kept go back on a helper thread: hipFree of a block kernels have touched takes tens of milliseconds per
    // gigabyte-sized block in a busy process (three losers of 2.4 GB: 100-200 ms, four times the load they were probed for), and
    // nothing the caller does next depends on it.  One helper at a time per context; the next probing allocation and
    // ibu_ctx_destroy join it.
    if (ctx->loser_free.joinable()) ctx->loser_free.join();
    std::vector<void*> losers;
    bool deferred = false;
    try {
      for (uint32_t k = 0; k < got; ++k)
        if (k != best) losers.push_back(cand[k]);
      const int dev = ctx->device;
      const bool trace = trace_sort();
      ctx->loser_free = std::thread([losers, dev, trace] {
        const auto tf = std::chrono::steady_clock::now();
        (void)hipSetDevice(dev);
        for (void* q : losers) (void)hipFree(q);
        if (trace) fprintf(stderr, "ibu alloc: freed the %zu candidates not kept in %.2f ms (helper thread)\n", losers.size(),
                           std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tf).count());
      });
      deferred = true;
    } catch (...) {
    }
    if (!deferred)
      for (uint32_t k = 0; k < got; ++k)
        if (k != best) (void)hipFree(cand[k]);
  }
  *d_ptr = cand[best];
  if (report) {
    report->tries = got;
    report->chosen = best;
    for (uint32_t k = 0; k < got; ++k) report->ms[k] = ms[k];
  }
  return IBU_OK;
}
extern "C" int32_t ibu_device_alloc_probed(ibu_ctx_t* ctx, size_t bytes, uint32_t tries, void** d_ptr, ibu_alloc_probe_t* report) {
  return alloc_probed_impl(ctx, bytes, tries, d_ptr, report, 0, nullptr);
}
extern "C" int32_t ibu_device_free(ibu_ctx_t* ctx, void* d_ptr) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  IBU_HIP(hipFree(d_ptr));
  return IBU_OK;
}
extern "C" int32_t ibu_memcpy_h2d(ibu_ctx_t* ctx, void* d_dst, const void* h_src, size_t bytes, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (bytes) IBU_HIP(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_memcpy_d2h(ibu_ctx_t* ctx, void* h_dst, const void* d_src, size_t bytes, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (bytes) IBU_HIP(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, pick_stream(ctx, stream)));
  return IBU_OK;
}

// ---- K1 / K1' ------------------------------------------------------------------------------
extern "C" int32_t ibu_deserialize(ibu_ctx_t* ctx, const void* d_records, size_t n, uint64_t* d_barcode,
                                   uint64_t* d_umi, uint64_t* d_index, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (n == 0) return IBU_OK;
  if (!d_records || !d_barcode || !d_umi || !d_index) return err_arg("NULL device pointer");
  if (!aligned8(d_records) || !aligned8(d_barcode) || !aligned8(d_umi) || !aligned8(d_index))
    return err_arg("u64 data must be 8-byte aligned");
  IBU_HIP(launch_deserialize(ctx->cfg, d_records, n, d_barcode, d_umi, d_index, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_serialize(ibu_ctx_t* ctx, const uint64_t* d_barcode, const uint64_t* d_umi,
                                 const uint64_t* d_index, size_t n, void* d_records, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (n == 0) return IBU_OK;
  if (!d_records || !d_barcode || !d_umi || !d_index) return err_arg("NULL device pointer");
  if (!aligned8(d_records) || !aligned8(d_barcode) || !aligned8(d_umi) || !aligned8(d_index))
    return err_arg("u64 data must be 8-byte aligned");
  IBU_HIP(launch_serialize(ctx->cfg, d_barcode, d_umi, d_index, n, d_records, pick_stream(ctx, stream)));
  return IBU_OK;
}

// ---- column codec ----------------------------------------------------------------------------
extern "C" int32_t ibu_unpack_2bit(ibu_ctx_t* ctx, const uint64_t* d_codes, size_t n, uint32_t len, uint8_t* d_ascii,
                                   void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (len == 0 || len > 32) return err_seq_len(len);
  if (n == 0) return IBU_OK;
  if (!d_codes || !d_ascii) return err_arg("NULL device pointer");
  if (!aligned8(d_codes)) return err_arg("u64 data must be 8-byte aligned");
  IBU_HIP(launch_unpack(ctx->cfg, d_codes, n, len, d_ascii, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_pack_2bit(ibu_ctx_t* ctx, const uint8_t* d_ascii, size_t n, uint32_t len, uint64_t* d_codes,
                                 void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (len == 0 || len > 32) return err_seq_len(len);
  if (n == 0) return IBU_OK;
  if (!d_codes || !d_ascii) return err_arg("NULL device pointer");
  if (!aligned8(d_codes)) return err_arg("u64 data must be 8-byte aligned");
  IBU_HIP(launch_pack(ctx->cfg, d_ascii, n, len, d_codes, ctx->d_status, pick_stream(ctx, stream)));
  return IBU_OK;
}

// ---- K2 / K3 -----------------------------------------------------------------------------------
extern "C" int32_t ibu_decode_ascii(ibu_ctx_t* ctx, const void* d_records, size_t n, uint32_t bc_len, uint32_t umi_len,
                                    uint8_t* d_bc_ascii, uint8_t* d_umi_ascii, uint64_t* d_index, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  rc = check_lens(bc_len, umi_len);
  if (rc) return rc;
  if (n == 0) return IBU_OK;
  if (!d_records) return err_arg("d_records is NULL");
  if (!aligned8(d_records) || !aligned8(d_index)) return err_arg("u64 data must be 8-byte aligned");
  IBU_HIP(launch_decode(ctx->cfg, d_records, n, bc_len, umi_len, d_bc_ascii, d_umi_ascii, d_index,
                        pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_encode_ascii(ibu_ctx_t* ctx, const uint8_t* d_bc_ascii, const uint8_t* d_umi_ascii,
                                    const uint64_t* d_index, uint64_t first_index, size_t n, uint32_t bc_len,
                                    uint32_t umi_len, void* d_records, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  rc = check_lens(bc_len, umi_len);
  if (rc) return rc;
  if (n == 0) return IBU_OK;
  if (!d_records || !d_bc_ascii || !d_umi_ascii) return err_arg("NULL device pointer");
  if (!aligned8(d_records) || !aligned8(d_index)) return err_arg("u64 data must be 8-byte aligned");
  IBU_HIP(launch_encode(ctx->cfg, d_bc_ascii, d_umi_ascii, d_index, first_index, n, bc_len, umi_len, d_records,
                        ctx->d_status, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_codec_status(ibu_ctx_t* ctx, void* stream, uint64_t* first_bad_record, uint64_t* n_bad_records) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  hipStream_t st = pick_stream(ctx, stream);
  IBU_HIP(hipMemcpyAsync(ctx->h_pinned, ctx->d_status, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  IBU_HIP(hipStreamSynchronize(st));
  const uint64_t first = ctx->h_pinned[0], nbad = ctx->h_pinned[1];
  if (first_bad_record) *first_bad_record = first;
  if (n_bad_records) *n_bad_records = nbad;
  if (nbad == 0) return IBU_OK;
  IBU_HIP(launch_fill2(ctx->d_status, ~0ull, 0, st));  // re-arm
  return set_error(IBU_ERR_INVALID_BASE, first, nbad, 0,
                   "Invalid base: %llu record(s) hold a byte outside ACGTacgt, first at record %llu",
                   (unsigned long long)nbad, (unsigned long long)first);
}

// ---- K4 ---------------------------------------------------------------------------------------------
extern "C" int32_t ibu_reduce_reset(ibu_ctx_t* ctx, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  IBU_HIP(hipMemsetAsync(ctx->d_acc, 0, kReduceAccBytes, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_reduce(ibu_ctx_t* ctx, const void* d_records, size_t n, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (n == 0) return IBU_OK;
  if (!d_records || !aligned8(d_records)) return err_arg("d_records must be non-NULL and 8-byte aligned");
  IBU_HIP(launch_reduce(ctx->cfg, d_records, n, ctx->d_acc, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_reduce_fetch(ibu_ctx_t* ctx, void* stream, ibu_reduce_result_t* out) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!out) return err_arg("out is NULL");
  hipStream_t st = pick_stream(ctx, stream);
  IBU_HIP(launch_reduce_fold(ctx->d_acc, st));
  IBU_HIP(hipMemcpyAsync(ctx->h_pinned, ctx->d_acc, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  IBU_HIP(hipStreamSynchronize(st));
  out->count = ctx->h_pinned[0];
  for (int k = 0; k < 3; ++k) {
    out->sum[k] = ctx->h_pinned[1 + k];
    out->xor_[k] = ctx->h_pinned[4 + k];
  }
  return IBU_OK;
}

// ---- synthetic records, sortedness, sort ---------------------------------------------------------------
extern "C" int32_t ibu_generate(ibu_ctx_t* ctx, uint64_t seed, uint64_t first, size_t n, uint32_t bc_len,
                                uint32_t umi_len, void* d_records, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  rc = check_lens(bc_len, umi_len);
  if (rc) return rc;
  if (n == 0) return IBU_OK;
  if (!d_records || !aligned8(d_records)) return err_arg("d_records must be non-NULL and 8-byte aligned");
  IBU_HIP(launch_generate(ctx->cfg, seed, first, n, bc_len, umi_len, d_records, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_device_copy(ibu_ctx_t* ctx, void* d_dst, const void* d_src, size_t bytes, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (bytes == 0) return IBU_OK;
  if (!d_dst || !d_src) return err_arg("NULL device pointer");
  const uintptr_t a = reinterpret_cast<uintptr_t>(d_dst), b = reinterpret_cast<uintptr_t>(d_src);
  if (a < b + bytes && b < a + bytes) return err_arg("source and destination overlap");
  IBU_HIP(launch_copy(ctx->cfg, d_src, d_dst, bytes, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_lower_bound_records(ibu_ctx_t* ctx, const void* d_sorted_records, size_t n, const void* d_keys, size_t k,
                                           uint64_t* d_pos, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (k == 0) return IBU_OK;
  if (k > (1u << 20)) return err_arg("at most 2^20 keys per call");
  if (!d_keys || !d_pos || !aligned8(d_keys) || !aligned8(d_pos)) return err_arg("d_keys / d_pos must be non-NULL and 8-byte aligned");
  if (n && (!d_sorted_records || !aligned8(d_sorted_records))) return err_arg("d_sorted_records must be non-NULL and 8-byte aligned");
  IBU_HIP(launch_lower_bound(d_sorted_records, n, d_keys, k, d_pos, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_is_sorted(ibu_ctx_t* ctx, const void* d_records, size_t n, void* stream, int32_t* sorted) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!sorted) return err_arg("sorted is NULL");
  *sorted = 1;
  if (n < 2) return IBU_OK;
  if (!d_records || !aligned8(d_records)) return err_arg("d_records must be non-NULL and 8-byte aligned");
  hipStream_t st = pick_stream(ctx, stream);
  IBU_HIP(hipMemsetAsync(ctx->d_flag, 0, 4, st));
  IBU_HIP(launch_sorted_check(ctx->cfg, d_records, n, ctx->d_flag, st));
  IBU_HIP(hipMemcpyAsync(ctx->h_pinned + 8, ctx->d_flag, 4, hipMemcpyDeviceToHost, st));
  IBU_HIP(hipStreamSynchronize(st));
  *sorted = (*reinterpret_cast<uint32_t*>(ctx->h_pinned + 8)) == 0;
  return IBU_OK;
}
// `a == b` on two device-resident record slices, with the position (Record: PartialEq / Eq, record.rs:58).
extern "C" int32_t ibu_records_first_mismatch(ibu_ctx_t* ctx, const void* d_a, const void* d_b, size_t n, uint64_t* first,
                                              void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!first) return err_arg("first is NULL");
  *first = n;
  if (n == 0) return IBU_OK;
  if (!d_a || !d_b || !aligned8(d_a) || !aligned8(d_b)) return err_arg("d_a / d_b must be non-NULL and 8-byte aligned");
  if (n > (~(size_t)0) / 3) return err_arg("n too large");
  hipStream_t st = pick_stream(ctx, stream);
  uint64_t* slot = reinterpret_cast<uint64_t*>(ctx->d_flag) + 1;   // d_flag: 16 bytes; [0] is the sortedness flag
  IBU_HIP(hipMemsetAsync(slot, 0xFF, 8, st));
  IBU_HIP(launch_mismatch(ctx->cfg, d_a, d_b, 3 * n, slot, st));
  IBU_HIP(hipMemcpyAsync(ctx->h_pinned + 10, slot, 8, hipMemcpyDeviceToHost, st));
  IBU_HIP(hipStreamSynchronize(st));
  const uint64_t w = ctx->h_pinned[10];
  if (w != ~0ull) *first = w / 3;
  return IBU_OK;
}
// ---- compacted keys: census, plan, records <-> 12-byte elements (the exchange format of the multi-GPU sort) ----------
static_assert(sizeof(ibu_key_plan_t) == sizeof(ibu::CompactPlan) && offsetof(ibu_key_plan_t, base) == offsetof(ibu::CompactPlan, base) &&
                  offsetof(ibu_key_plan_t, k) == offsetof(ibu::CompactPlan, k),
              "ibu_key_plan_t is the kernels' CompactPlan");
static_assert(sizeof(ibu_inflate_block_t) == sizeof(InflateBlockDesc) && offsetof(ibu_inflate_block_t, crc32) == offsetof(InflateBlockDesc, crc) &&
              offsetof(ibu_inflate_block_t, out_offset) == offsetof(InflateBlockDesc, ooff) && IBU_INFLATE_PAD == kInflatePad,
              "ibu_inflate_block_t is the kernel's descriptor");
extern "C" int32_t ibu_inflate_blocks_device(ibu_ctx_t* ctx, const void* d_comp, const ibu_inflate_block_t* d_blocks, size_t n, void* d_out,
                                             uint32_t* d_status, uint32_t* d_first_bad, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (n == 0) return IBU_OK;
  if (!d_comp || !d_blocks || !d_out || !d_status || !d_first_bad) return err_arg("NULL argument");
  if (n >= (1ull << 31)) return err_arg("fewer than 2^31 blocks per call");
  rc = ensure_sort_scratch(ctx, inflate_scratch_bytes(ctx->cfg, n));   // (the lanes' symbol tables: the context's scratch, as the sort's)
  if (rc) return rc;
  IBU_HIP(launch_inflate_blocks(ctx->cfg, d_comp, reinterpret_cast<const InflateBlockDesc*>(d_blocks), n, d_out, d_status, d_first_bad,
                                ctx->d_sort_scratch, ctx->sort_scratch_bytes, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_records_census(ibu_ctx_t* ctx, const void* d_records, size_t n, uint64_t out[8], void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!out) return err_arg("out is NULL");
  if (n && (!d_records || !aligned8(d_records))) return err_arg("d_records must be non-NULL and 8-byte aligned");
  rc = ensure_sort_scratch(ctx, 4096);   // the census slots (sort.hip: kCensusBytes)
  if (rc) return rc;
  hipStream_t st = pick_stream(ctx, stream);
  uint64_t* d_c = static_cast<uint64_t*>(ctx->d_sort_scratch);
  IBU_HIP(launch_records_census(ctx->cfg, d_records, n, d_c, st));
  IBU_HIP(hipMemcpyAsync(out, d_c, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  IBU_HIP(hipStreamSynchronize(st));
  return IBU_OK;
}
extern "C" int32_t ibu_key_plan_init(const uint64_t or_words[3], const uint64_t and_words[3], ibu_key_plan_t* plan) {
  if (!or_words || !and_words || !plan) return err_arg("NULL argument");
  compact_plan_init(or_words, and_words, reinterpret_cast<CompactPlan*>(plan));
  return IBU_OK;
}
static int32_t check_plan(const ibu_key_plan_t* plan) {
  if (!plan) return err_arg("plan is NULL");
  if (plan->k > 12) return err_arg("more than 12 key bytes vary: these records do not fit 12-byte elements");
  return IBU_OK;
}
extern "C" int32_t ibu_records_compact(ibu_ctx_t* ctx, const ibu_key_plan_t* plan, const void* d_records, size_t n, void* d_elems,
                                       void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if ((rc = check_plan(plan)) != 0) return rc;
  if (n == 0) return IBU_OK;
  if (!d_records || !aligned8(d_records)) return err_arg("d_records must be non-NULL and 8-byte aligned");
  if (!d_elems || (reinterpret_cast<uintptr_t>(d_elems) & 3u)) return err_arg("d_elems must be non-NULL and 4-byte aligned");
  IBU_HIP(launch_compact(ctx->cfg, *reinterpret_cast<const CompactPlan*>(plan), d_records, n, d_elems, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_records_expand(ibu_ctx_t* ctx, const ibu_key_plan_t* plan, const void* d_elems, size_t n, void* d_records,
                                      void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if ((rc = check_plan(plan)) != 0) return rc;
  if (n == 0) return IBU_OK;
  if (!d_records || !aligned8(d_records)) return err_arg("d_records must be non-NULL and 8-byte aligned");
  if (!d_elems || (reinterpret_cast<uintptr_t>(d_elems) & 3u)) return err_arg("d_elems must be non-NULL and 4-byte aligned");
  IBU_HIP(launch_expand(ctx->cfg, *reinterpret_cast<const CompactPlan*>(plan), d_elems, n, d_records, pick_stream(ctx, stream)));
  return IBU_OK;
}
// the emit scratch of the run-length aggregations (16 bytes per entry): grows only
static int32_t ensure_runs_scratch(ibu_ctx* ctx, size_t need) {
  if (need <= ctx->runs_scratch_bytes) return IBU_OK;
  if (ctx->d_runs_scratch) IBU_HIP(hipFree(ctx->d_runs_scratch));
  ctx->d_runs_scratch = nullptr;
  ctx->runs_scratch_bytes = 0;
  IBU_HIP(ctx_malloc(ctx, &ctx->d_runs_scratch, need));
  ctx->runs_scratch_bytes = need;
  return IBU_OK;
}
// The first half of every run-length aggregation: a count scratch of `need` bytes, the count pass, and its two totals (runs, ranked
// heads) read back into ctx->h_pinned[0..1].  Synchronises the stream.
static int32_t runs_count_totals(ibu_ctx* ctx, const void* d_sorted_records, size_t n, size_t need, RunsCount what, hipStream_t st) {
  int32_t rc = ensure_sort_scratch(ctx, need);
  if (rc) return rc;
  IBU_HIP(launch_runs_count(ctx->cfg, d_sorted_records, n, ctx->d_sort_scratch, ctx->sort_scratch_bytes, what, st));
  IBU_HIP(hipMemcpyAsync(ctx->h_pinned, ctx->d_sort_scratch, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  IBU_HIP(hipStreamSynchronize(st));
  return IBU_OK;
}
// BarcodeAnalyzer (parallel.rs:72-98) on sorted device records.
extern "C" int32_t ibu_barcode_counts(ibu_ctx_t* ctx, const void* d_sorted_records, size_t n, uint64_t* d_barcodes,
                                      uint64_t* d_counts, uint64_t* d_unique_umis, size_t cap, size_t* n_barcodes,
                                      size_t* n_barcode_umi_pairs, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!n_barcodes) return err_arg("n_barcodes is NULL");
  *n_barcodes = 0;
  if (n_barcode_umi_pairs) *n_barcode_umi_pairs = 0;
  if (n == 0) return IBU_OK;
  if (!d_sorted_records || !aligned8(d_sorted_records)) return err_arg("d_sorted_records must be non-NULL and 8-byte aligned");
  if (n >= (1ull << 40)) return err_arg("barcode_counts handles fewer than 2^40 records per call");
  hipStream_t st = pick_stream(ctx, stream);
  const bool size_query = !d_barcodes && !d_counts && cap == 0;
  // (with outputs to fill, the count pass keeps every segment's first few run heads: the emit pass then reads the records again only
  // where runs are short — k_aggregate.hip)
  rc = runs_count_totals(ctx, d_sorted_records, n, runs_scratch_bytes(n), size_query ? RunsCount::Barcode : RunsCount::BarcodeStash, st);
  if (rc) return rc;
  const uint64_t runs = ctx->h_pinned[0], pairs = ctx->h_pinned[1];
  *n_barcodes = runs;
  if (n_barcode_umi_pairs) *n_barcode_umi_pairs = pairs;
  if (size_query) return IBU_OK;
  if (!d_barcodes || !d_counts) return err_arg("d_barcodes / d_counts are NULL");
  if (runs > cap) return err_arg("output capacity is smaller than the number of distinct barcodes (see *n_barcodes)");
  rc = ensure_runs_scratch(ctx, runs_emit_scratch_bytes(runs));
  if (rc) return rc;
  IBU_HIP(launch_runs_emit(ctx->cfg, d_sorted_records, n, ctx->d_sort_scratch, ctx->d_runs_scratch, runs, pairs, d_barcodes, nullptr,
                           d_counts, d_unique_umis, st));
  return IBU_OK;
}
// ---- barcode correction against a whitelist (k_whitelist.hip) --------------------------------------------------------
struct ibu_whitelist {
  ibu_ctx* ctx = nullptr;
  void* d_mem = nullptr;       // the table's slots, then the build's four status words
  size_t slots = 0, n_distinct = 0, device_bytes = 0;
  uint32_t bc_len = 0;
  bool has_ones = false;       // the all-ones key (a legal code at 32 bases only) is in the whitelist
};
extern "C" int32_t ibu_whitelist_create(ibu_ctx_t* ctx, const uint64_t* d_codes, size_t w, uint32_t bc_len, void* stream,
                                        ibu_whitelist_t** out) {
  if (!ctx) {   // without a context there is nothing to build on: say whether a device is missing altogether
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
    if (count == 0) return set_error(IBU_ERR_NO_DEVICE, 0, 0, 0, "no HIP device: a whitelist lives on a device context");
    return err_arg("ctx is NULL");
  }
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!out) return err_arg("out is NULL");
  *out = nullptr;
  if (w == 0) return err_arg("a whitelist needs at least one code");
  if (bc_len == 0 || bc_len > 32) return err_arg("bc_len must be 1..32");
  if (!d_codes || !aligned8(d_codes)) return err_arg("d_codes must be non-NULL and 8-byte aligned");
  if (w > (1ull << 31)) return err_arg("a whitelist holds at most 2^31 codes");
  hipStream_t st = pick_stream(ctx, stream);
  ibu_whitelist* wl = new ibu_whitelist;
  wl->ctx = ctx;
  wl->bc_len = bc_len;
  wl->slots = whitelist_slots(w);
  wl->device_bytes = wl->slots * sizeof(uint64_t) + 4 * sizeof(uint64_t);
  hipError_t e = ctx_malloc(ctx, &wl->d_mem, wl->device_bytes);
  uint64_t* table = static_cast<uint64_t*>(wl->d_mem);
  uint64_t* status = table ? table + wl->slots : nullptr;
  if (e == hipSuccess) e = hipMemsetAsync(table, 0xFF, (wl->slots + 1) * sizeof(uint64_t), st);   // free slots, status[0] = no bad code
  if (e == hipSuccess) e = hipMemsetAsync(status + 1, 0, 3 * sizeof(uint64_t), st);
  if (e == hipSuccess) e = launch_whitelist_build(ctx->cfg, d_codes, w, bc_len, table, wl->slots, status, st);
  if (e == hipSuccess) e = hipMemcpyAsync(ctx->h_pinned, status, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    ibu_whitelist_destroy(wl);
    return hip_fail(e, "ibu_whitelist_create");
  }
  const uint64_t first_bad = ctx->h_pinned[0];
  wl->n_distinct = ctx->h_pinned[1];
  wl->has_ones = ctx->h_pinned[2] != 0;
  if (first_bad != ~0ull) {
    ibu_whitelist_destroy(wl);
    return set_error(IBU_ERR_INVALID_ARG, first_bad, bc_len, 0, "Invalid argument: whitelist code %llu has bits at or above 2*bc_len (bc_len %u)",
                     (unsigned long long)first_bad, bc_len);
  }
  *out = wl;
  return IBU_OK;
}
extern "C" int32_t ibu_whitelist_info(const ibu_whitelist_t* wl, uint32_t* bc_len, size_t* n_distinct, size_t* device_bytes) {
  if (!wl) return err_arg("wl is NULL");
  if (bc_len) *bc_len = wl->bc_len;
  if (n_distinct) *n_distinct = wl->n_distinct;
  if (device_bytes) *device_bytes = wl->device_bytes;
  return IBU_OK;
}
extern "C" void ibu_whitelist_destroy(ibu_whitelist_t* wl) {
  if (!wl) return;
  if (wl->d_mem) {
    (void)hipSetDevice(wl->ctx->device);
    (void)hipFree(wl->d_mem);   // (waits for launches that still probe the table)
  }
  delete wl;
}
extern "C" int32_t ibu_correct_barcodes(ibu_ctx_t* ctx, const ibu_whitelist_t* wl, void* d_records, size_t n, uint32_t max_mismatches,
                                        uint8_t* d_class, ibu_correct_counts_t* counts, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!wl) return err_arg("wl is NULL");
  if (wl->ctx != ctx) return err_arg("the whitelist was created on another context");
  if (max_mismatches > 1) return err_arg("max_mismatches must be 0 or 1");
  if (counts) *counts = ibu_correct_counts_t{0, 0, 0, 0};
  if (n == 0) return IBU_OK;
  if (!d_records || !aligned8(d_records)) return err_arg("d_records must be non-NULL and 8-byte aligned");
  if (n >= (1ull << 40)) return err_arg("correct_barcodes handles fewer than 2^40 records per call");
  hipStream_t st = pick_stream(ctx, stream);
  const WhitelistTable t{static_cast<const uint64_t*>(wl->d_mem), wl->slots, wl->bc_len, wl->has_ones};
  if (!counts) {   // nothing to bring back: the launch stays asynchronous and touches no per-call state
    IBU_HIP(launch_correct(ctx->cfg, t, d_records, n, max_mismatches, d_class, nullptr, st));
    return IBU_OK;
  }
  if (!ctx->d_correct_acc) IBU_HIP(ctx_malloc(ctx, reinterpret_cast<void**>(&ctx->d_correct_acc), kCorrectAccBytes));
  IBU_HIP(hipMemsetAsync(ctx->d_correct_acc, 0, kCorrectAccBytes, st));
  IBU_HIP(launch_correct(ctx->cfg, t, d_records, n, max_mismatches, d_class, ctx->d_correct_acc, st));
  IBU_HIP(launch_correct_fold(ctx->d_correct_acc, st));
  IBU_HIP(hipMemcpyAsync(ctx->h_pinned, ctx->d_correct_acc, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  IBU_HIP(hipStreamSynchronize(st));
  counts->exact = ctx->h_pinned[0];
  counts->corrected = ctx->h_pinned[1];
  counts->ambiguous = ctx->h_pinned[2];
  counts->unmatched = ctx->h_pinned[3];
  return IBU_OK;
}
// ---- whitelist abundance and the resolution of ambiguous barcodes (k_whitelist.hip) ----------------------------------------
struct ibu_abundance {
  ibu_ctx* ctx = nullptr;
  const ibu_whitelist* wl = nullptr;
  uint64_t* d_counters = nullptr;          // slots + 1: one per table slot, the last for the all-ones key
  size_t device_bytes = 0;
  std::atomic<uint64_t> offered{0};        // records offered to ibu_abundance_add since create / reset: no counter can pass it
};
static constexpr uint64_t kAbundanceMax = 1ull << 40;
extern "C" int32_t ibu_abundance_create(ibu_ctx_t* ctx, const ibu_whitelist_t* wl, void* stream, ibu_abundance_t** out) {
  if (!ctx) {   // as ibu_whitelist_create: say whether a device is missing altogether
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
    if (count == 0) return set_error(IBU_ERR_NO_DEVICE, 0, 0, 0, "no HIP device: an abundance lives on a device context");
    return err_arg("ctx is NULL");
  }
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!out) return err_arg("out is NULL");
  *out = nullptr;
  if (!wl) return err_arg("wl is NULL");
  if (wl->ctx != ctx) return err_arg("the whitelist was created on another context");
  hipStream_t st = pick_stream(ctx, stream);
  ibu_abundance* ab = new ibu_abundance;
  ab->ctx = ctx;
  ab->wl = wl;
  ab->device_bytes = (wl->slots + 1) * sizeof(uint64_t);
  hipError_t e = ctx_malloc(ctx, reinterpret_cast<void**>(&ab->d_counters), ab->device_bytes);
  if (e == hipSuccess) e = hipMemsetAsync(ab->d_counters, 0, ab->device_bytes, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    ibu_abundance_destroy(ab);
    return hip_fail(e, "ibu_abundance_create");
  }
  *out = ab;
  return IBU_OK;
}
extern "C" int32_t ibu_abundance_reset(ibu_abundance_t* ab, void* stream) {
  if (!ab) return err_arg("ab is NULL");
  int32_t rc = check_ctx(ab->ctx);
  if (rc) return rc;
  IBU_HIP(hipMemsetAsync(ab->d_counters, 0, ab->device_bytes, pick_stream(ab->ctx, stream)));
  ab->offered.store(0);
  return IBU_OK;
}
extern "C" int32_t ibu_abundance_info(const ibu_abundance_t* ab, size_t* device_bytes) {
  if (!ab) return err_arg("ab is NULL");
  if (device_bytes) *device_bytes = ab->device_bytes;
  return IBU_OK;
}
extern "C" void ibu_abundance_destroy(ibu_abundance_t* ab) {
  if (!ab) return;
  if (ab->d_counters) {
    (void)hipSetDevice(ab->ctx->device);
    (void)hipFree(ab->d_counters);   // (waits for launches that still add to or read the counters)
  }
  delete ab;
}
static int32_t check_abundance(const ibu_ctx* ctx, const ibu_abundance* ab) {
  if (!ab) return err_arg("ab is NULL");
  if (ab->ctx != ctx) return err_arg("the abundance was created on another context");
  return IBU_OK;
}
static WhitelistTable table_of(const ibu_whitelist* wl) {
  return WhitelistTable{static_cast<const uint64_t*>(wl->d_mem), wl->slots, wl->bc_len, wl->has_ones};
}
extern "C" int32_t ibu_abundance_add(ibu_ctx_t* ctx, ibu_abundance_t* ab, const void* d_records, const uint8_t* d_class, size_t n,
                                     uint32_t class_mask, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  rc = check_abundance(ctx, ab);
  if (rc) return rc;
  if (n == 0) return IBU_OK;
  if (!d_records || !aligned8(d_records)) return err_arg("d_records must be non-NULL and 8-byte aligned");
  if (n >= kAbundanceMax) return err_arg("abundance_add handles fewer than 2^40 records per call");
  uint64_t seen = ab->offered.load();
  do {
    if (seen + n > kAbundanceMax)
      return set_error(IBU_ERR_INVALID_ARG, seen, n, 0, "Invalid argument: %llu records offered so far and %llu more would pass 2^40 (reset the abundance)",
                       (unsigned long long)seen, (unsigned long long)n);
  } while (!ab->offered.compare_exchange_weak(seen, seen + n));
  IBU_HIP(launch_abundance_add(ctx->cfg, table_of(ab->wl), d_records, d_class, n, class_mask & 0xFFu, ab->d_counters, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_abundance_counts(ibu_ctx_t* ctx, const ibu_abundance_t* ab, const uint64_t* d_codes, size_t k, uint64_t* d_counts,
                                        void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  rc = check_abundance(ctx, ab);
  if (rc) return rc;
  if (k == 0) return IBU_OK;
  if (!d_codes || !aligned8(d_codes) || !d_counts || !aligned8(d_counts)) return err_arg("d_codes / d_counts must be non-NULL and 8-byte aligned");
  if (k >= kAbundanceMax) return err_arg("abundance_counts handles fewer than 2^40 codes per call");
  IBU_HIP(launch_abundance_counts(ctx->cfg, table_of(ab->wl), ab->d_counters, d_codes, k, d_counts, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_resolve_barcodes(ibu_ctx_t* ctx, const ibu_whitelist_t* wl, const ibu_abundance_t* ab, void* d_records, size_t n,
                                        uint64_t num, uint64_t den, uint8_t* d_class, ibu_resolve_counts_t* counts, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!wl) return err_arg("wl is NULL");
  if (wl->ctx != ctx) return err_arg("the whitelist was created on another context");
  rc = check_abundance(ctx, ab);
  if (rc) return rc;
  if (ab->wl != wl) return err_arg("the abundance belongs to another whitelist");
  if (num < 1 || num > den || den >= (1ull << 24) || 2 * num <= den)
    return err_arg("the share num / den must satisfy 1 <= num <= den < 2^24 and 2 * num > den");
  if (counts) *counts = ibu_resolve_counts_t{0, 0, 0, 0};
  if (n == 0) return IBU_OK;
  if (!d_records || !aligned8(d_records)) return err_arg("d_records must be non-NULL and 8-byte aligned");
  if (!d_class) return err_arg("d_class is NULL");
  if (n >= (1ull << 40)) return err_arg("resolve_barcodes handles fewer than 2^40 records per call");
  hipStream_t st = pick_stream(ctx, stream);
  const WhitelistTable t = table_of(wl);
  if (!counts) {   // nothing to bring back: the launch stays asynchronous and touches no per-call state
    IBU_HIP(launch_resolve(ctx->cfg, t, ab->d_counters, d_records, n, num, den, d_class, nullptr, st));
    return IBU_OK;
  }
  if (!ctx->d_resolve_acc) IBU_HIP(ctx_malloc(ctx, reinterpret_cast<void**>(&ctx->d_resolve_acc), kCorrectAccBytes));
  IBU_HIP(hipMemsetAsync(ctx->d_resolve_acc, 0, kCorrectAccBytes, st));
  IBU_HIP(launch_resolve(ctx->cfg, t, ab->d_counters, d_records, n, num, den, d_class, ctx->d_resolve_acc, st));
  IBU_HIP(launch_correct_fold(ctx->d_resolve_acc, st));
  IBU_HIP(hipMemcpyAsync(ctx->h_pinned, ctx->d_resolve_acc, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  IBU_HIP(hipStreamSynchronize(st));
  counts->examined = ctx->h_pinned[0];
  counts->resolved = ctx->h_pinned[1];
  counts->below_share = ctx->h_pinned[2];
  counts->unseen = ctx->h_pinned[3];
  return IBU_OK;
}
extern "C" int32_t ibu_select_records(ibu_ctx_t* ctx, const void* d_records, const uint8_t* d_class, size_t n, uint32_t keep_mask,
                                      void* d_out, size_t cap, size_t* n_out, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!n_out) return err_arg("n_out is NULL");
  *n_out = 0;
  if (n == 0) return IBU_OK;
  if (!d_records || !aligned8(d_records)) return err_arg("d_records must be non-NULL and 8-byte aligned");
  if (!d_class) return err_arg("d_class is NULL");
  if (n >= (1ull << 40)) return err_arg("select_records handles fewer than 2^40 records per call");
  const bool size_query = !d_out && cap == 0;
  if (!size_query) {
    if (!d_out || !aligned8(d_out)) return err_arg("d_out must be non-NULL and 8-byte aligned");
    const uintptr_t a = reinterpret_cast<uintptr_t>(d_out), b = reinterpret_cast<uintptr_t>(d_records);
    const size_t cap_in = cap < n ? cap : n;   // no more than n records are ever written
    if (a < b + 24 * n && b < a + 24 * cap_in) return err_arg("d_out overlaps d_records");
  }
  hipStream_t st = pick_stream(ctx, stream);
  rc = ensure_sort_scratch(ctx, select_scratch_bytes(n));
  if (rc) return rc;
  IBU_HIP(launch_select_count(ctx->cfg, d_class, n, keep_mask & 0xFFu, ctx->d_sort_scratch, ctx->sort_scratch_bytes, st));
  IBU_HIP(hipMemcpyAsync(ctx->h_pinned, ctx->d_sort_scratch, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  IBU_HIP(hipStreamSynchronize(st));
  const uint64_t kept = ctx->h_pinned[0];
  *n_out = kept;
  if (size_query) return IBU_OK;
  if (kept > cap)
    return set_error(IBU_ERR_INVALID_ARG, kept, cap, 0, "Invalid argument: output capacity %llu is smaller than the %llu records kept (see *n_out)",
                     (unsigned long long)cap, (unsigned long long)kept);
  IBU_HIP(launch_select_scatter(ctx->cfg, d_records, d_class, n, keep_mask & 0xFFu, ctx->d_sort_scratch, d_out, st));
  return IBU_OK;
}
extern "C" int32_t ibu_sort_records(ibu_ctx_t* ctx, void* d_records, void* d_tmp, size_t n, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (n < 2) return IBU_OK;
  if (!d_records || !d_tmp || !aligned8(d_records) || !aligned8(d_tmp))
    return err_arg("d_records / d_tmp must be non-NULL and 8-byte aligned");
  if (n >= (1ull << 40)) return err_arg("sort_records handles fewer than 2^40 records per call");  // an argument limit, not a HIP error
  rc = ensure_sort_scratch(ctx, sort_scratch_bytes(ctx->cfg, n));
  if (rc) return rc;
  IBU_HIP(launch_sort_records(ctx->cfg, d_records, d_tmp, n, ctx->d_sort_scratch, ctx->sort_scratch_bytes,
                              pick_stream(ctx, stream)));
  return IBU_OK;
}
// ---- merge of sorted records (k_merge.hip).  The semantics are this library's: include/ibu_hip.h.
// One two-way merge, arguments checked by the caller; an empty input is a copy of the other (and its source bytes a fill).
static int32_t merge_two(ibu_ctx_t* ctx, const void* d_a, size_t na, const void* d_b, size_t nb, void* d_out, uint8_t* d_source, hipStream_t st) {
  if (na == 0 || nb == 0) {
    const size_t n = na + nb;
    if (n == 0) return IBU_OK;
    IBU_HIP(launch_copy(ctx->cfg, na ? d_a : d_b, d_out, 24 * n, st));
    if (d_source) IBU_HIP(hipMemsetAsync(d_source, na ? 0 : 1, n, st));
    return IBU_OK;
  }
  IBU_HIP(launch_merge(ctx->cfg, d_a, na, d_b, nb, d_out, d_source, ctx->d_sort_scratch, st));
  return IBU_OK;
}
extern "C" int32_t ibu_merge_sorted(ibu_ctx_t* ctx, const void* d_a, size_t na, const void* d_b, size_t nb, void* d_out, uint8_t* d_source,
                                    void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (na >= (1ull << 40) || nb >= (1ull << 40)) return err_arg("merge_sorted handles fewer than 2^40 records per input");
  const size_t n = na + nb;
  if (n == 0) return IBU_OK;
  if ((na && (!d_a || !aligned8(d_a))) || (nb && (!d_b || !aligned8(d_b))) || !d_out || !aligned8(d_out))
    return err_arg("d_a / d_b / d_out must be non-NULL and 8-byte aligned");
  const uintptr_t o = reinterpret_cast<uintptr_t>(d_out), a = reinterpret_cast<uintptr_t>(d_a), b = reinterpret_cast<uintptr_t>(d_b);
  if ((na && o < a + 24 * na && a < o + 24 * n) || (nb && o < b + 24 * nb && b < o + 24 * n)) return err_arg("d_out overlaps an input");
  rc = ensure_sort_scratch(ctx, merge_scratch_bytes(n));
  if (rc) return rc;
  return merge_two(ctx, d_a, na, d_b, nb, d_out, d_source, pick_stream(ctx, stream));
}
extern "C" int32_t ibu_merge_sorted_runs(ibu_ctx_t* ctx, void* d_records, void* d_tmp, const size_t* run_lengths, size_t k, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (k == 0) return IBU_OK;
  if (!run_lengths) return err_arg("run_lengths is NULL");
  size_t n = 0;
  for (size_t i = 0; i < k; ++i) {
    if (run_lengths[i] >= (1ull << 40)) return err_arg("merge_sorted_runs handles fewer than 2^40 records per call");
    n += run_lengths[i];
    if (n >= (1ull << 40)) return err_arg("merge_sorted_runs handles fewer than 2^40 records per call");
  }
  if (n == 0 || k == 1) return IBU_OK;
  if (!d_records || !d_tmp || !aligned8(d_records) || !aligned8(d_tmp)) return err_arg("d_records / d_tmp must be non-NULL and 8-byte aligned");
  const uintptr_t r = reinterpret_cast<uintptr_t>(d_records), t = reinterpret_cast<uintptr_t>(d_tmp);
  if (r < t + 24 * n && t < r + 24 * n) return err_arg("d_tmp overlaps d_records");
  rc = ensure_sort_scratch(ctx, merge_scratch_bytes(n));   // once, for the largest merge: nothing is allocated between the levels
  if (rc) return rc;
  hipStream_t st = pick_stream(ctx, stream);
  std::vector<size_t> runs(run_lengths, run_lengths + k), next;
  uint8_t* from = static_cast<uint8_t*>(d_records);
  uint8_t* to = static_cast<uint8_t*>(d_tmp);
  while (runs.size() > 1) {                                // one level: neighbouring runs pairwise, an unpaired last run copied
    next.clear();
    size_t at = 0;
    for (size_t i = 0; i < runs.size(); i += 2) {
      const size_t na = runs[i], nb = i + 1 < runs.size() ? runs[i + 1] : 0;
      rc = merge_two(ctx, from + 24 * at, na, from + 24 * (at + na), nb, to + 24 * at, nullptr, st);
      if (rc) return rc;
      next.push_back(na + nb);
      at += na + nb;
    }
    runs.swap(next);
    std::swap(from, to);
  }
  if (from != d_records) IBU_HIP(launch_copy(ctx->cfg, from, d_records, 24 * n, st));   // an odd number of levels ended in d_tmp
  return IBU_OK;
}
// ---- count matrix: distinct UMIs and reads per (barcode, index) pair (k_records.hip: the field exchange; k_aggregate.hip: the
// pair-level run walk).  The semantics are this library's: include/ibu_hip.h.
extern "C" int32_t ibu_records_swap_umi_index(ibu_ctx_t* ctx, const void* d_src, void* d_dst, size_t n, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (n == 0) return IBU_OK;
  if (!d_src || !d_dst || !aligned8(d_src) || !aligned8(d_dst)) return err_arg("d_src / d_dst must be non-NULL and 8-byte aligned");
  if (n >= (1ull << 40)) return err_arg("records_swap_umi_index handles fewer than 2^40 records per call");
  const uintptr_t a = reinterpret_cast<uintptr_t>(d_dst), b = reinterpret_cast<uintptr_t>(d_src);
  if (a != b && a < b + 24 * n && b < a + 24 * n) return err_arg("d_dst overlaps d_src (only d_dst == d_src, in place, is allowed)");
  IBU_HIP(launch_swap_fields(ctx->cfg, d_src, d_dst, n, pick_stream(ctx, stream)));
  return IBU_OK;
}
extern "C" int32_t ibu_pair_counts(ibu_ctx_t* ctx, const void* d_sorted_records, size_t n, uint64_t* d_first, uint64_t* d_second,
                                   uint64_t* d_records_per_pair, uint64_t* d_distinct_third, size_t cap, size_t* n_pairs,
                                   size_t* n_triples, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!n_pairs) return err_arg("n_pairs is NULL");
  *n_pairs = 0;
  if (n_triples) *n_triples = 0;
  if (n == 0) return IBU_OK;
  if (!d_sorted_records || !aligned8(d_sorted_records)) return err_arg("d_sorted_records must be non-NULL and 8-byte aligned");
  if (n >= (1ull << 40)) return err_arg("pair_counts handles fewer than 2^40 records per call");
  hipStream_t st = pick_stream(ctx, stream);
  rc = runs_count_totals(ctx, d_sorted_records, n, runs_scratch_bytes(n), RunsCount::Pair, st);
  if (rc) return rc;
  const bool size_query = !d_first && !d_second && !d_records_per_pair && cap == 0;
  const uint64_t pairs = ctx->h_pinned[0], triples = ctx->h_pinned[1];
  *n_pairs = pairs;
  if (n_triples) *n_triples = triples;
  if (size_query) return IBU_OK;
  if (!d_first || !d_second || !d_records_per_pair) return err_arg("d_first / d_second / d_records_per_pair are NULL");
  if (!aligned8(d_first) || !aligned8(d_second) || !aligned8(d_records_per_pair) || !aligned8(d_distinct_third))
    return err_arg("the output arrays must be 8-byte aligned");
  if (pairs > cap)
    return set_error(IBU_ERR_INVALID_ARG, pairs, cap, 0, "Invalid argument: output capacity %llu is smaller than the %llu entries (see *n_pairs)",
                     (unsigned long long)cap, (unsigned long long)pairs);
  rc = ensure_runs_scratch(ctx, runs_emit_scratch_bytes(pairs));
  if (rc) return rc;
  IBU_HIP(launch_runs_emit(ctx->cfg, d_sorted_records, n, ctx->d_sort_scratch, ctx->d_runs_scratch, pairs, triples, d_first, d_second,
                           d_records_per_pair, d_distinct_third, st));
  return IBU_OK;
}
// One index per (w0, w1) molecule: the candidate with strictly the most records (k_molecules.hip; the rule: include/ibu_hip.h).
extern "C" int32_t ibu_classify_molecules(ibu_ctx_t* ctx, const void* d_sorted_records, size_t n, uint32_t flags, uint8_t* d_class,
                                          ibu_molecule_counts_t* counts, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (flags & ~(uint32_t)IBU_MOLECULES_TIE_FIRST) return err_arg("unknown bit in flags");
  if (counts) *counts = ibu_molecule_counts_t{0, 0, 0, 0, 0, 0, 0, 0};
  if (n == 0) return IBU_OK;
  if (!d_sorted_records || !aligned8(d_sorted_records)) return err_arg("d_sorted_records must be non-NULL and 8-byte aligned");
  if (n >= (1ull << 40)) return err_arg("classify_molecules handles fewer than 2^40 records per call");
  hipStream_t st = pick_stream(ctx, stream);
  rc = runs_count_totals(ctx, d_sorted_records, n, molecules_scratch_bytes(n), RunsCount::Pair, st);
  if (rc) return rc;
  const uint64_t molecules = ctx->h_pinned[0], candidates = ctx->h_pinned[1];
  rc = ensure_runs_scratch(ctx, molecules_run_scratch_bytes(candidates));
  if (rc) return rc;
  IBU_HIP(launch_molecules_classify(ctx->cfg, d_sorted_records, n, ctx->d_sort_scratch, ctx->d_runs_scratch, candidates,
                                    (flags & IBU_MOLECULES_TIE_FIRST) != 0, d_class, st));
  if (!counts) return IBU_OK;
  IBU_HIP(hipMemcpyAsync(ctx->h_pinned, ctx->d_runs_scratch, 5 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  IBU_HIP(hipStreamSynchronize(st));
  counts->molecules = molecules;
  counts->candidates = candidates;
  counts->resolved = ctx->h_pinned[0];
  counts->tied = ctx->h_pinned[1];
  counts->reads_kept = ctx->h_pinned[2];
  counts->reads_minor = ctx->h_pinned[3];
  counts->reads_tied = ctx->h_pinned[4];
  return IBU_OK;
}
// Which barcodes are cells: one threshold on the per-barcode UMI (or read) count (k_cells.hip; the rule: include/ibu_hip.h).
extern "C" int32_t ibu_call_cells(ibu_ctx_t* ctx, const void* d_sorted_records, size_t n, uint32_t mode, uint64_t param, uint32_t flags,
                                  uint8_t* d_class, ibu_cell_counts_t* counts, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (mode > IBU_CELLS_ORDMAG) return err_arg("unknown mode");
  if (flags & ~(uint32_t)IBU_CELLS_BY_READS) return err_arg("unknown bit in flags");
  if (mode != IBU_CELLS_MIN && param == 0) return err_arg("param must be at least 1 in the TOP and ORDMAG modes");
  if (n && (!d_sorted_records || !aligned8(d_sorted_records))) return err_arg("d_sorted_records must be non-NULL and 8-byte aligned");
  if (n >= (1ull << 40)) return err_arg("call_cells handles fewer than 2^40 records per call");
  if (counts) {   // (behind the last argument check: a refused call leaves the totals alone)
    *counts = ibu_cell_counts_t{0, 0, 0, 0, 0, 0, 0, 0};
    if (mode == IBU_CELLS_MIN) counts->threshold = param;
  }
  if (n == 0) return IBU_OK;
  hipStream_t st = pick_stream(ctx, stream);
  rc = runs_count_totals(ctx, d_sorted_records, n, cells_scratch_bytes(n), RunsCount::Barcode, st);
  if (rc) return rc;
  const uint64_t barcodes = ctx->h_pinned[0], pairs = ctx->h_pinned[1];
  rc = ensure_runs_scratch(ctx, cells_run_scratch_bytes(barcodes));
  if (rc) return rc;
  IBU_HIP(launch_cells_call(ctx->cfg, d_sorted_records, n, ctx->d_sort_scratch, ctx->d_runs_scratch, barcodes, pairs, mode, param,
                            (flags & IBU_CELLS_BY_READS) != 0, d_class, st));
  if (!counts) return IBU_OK;
  IBU_HIP(hipMemcpyAsync(ctx->h_pinned, ctx->d_runs_scratch, 7 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  IBU_HIP(hipStreamSynchronize(st));
  counts->barcodes = barcodes;
  counts->cells = ctx->h_pinned[0];
  counts->reads_cells = ctx->h_pinned[1];
  counts->reads_background = ctx->h_pinned[2];
  counts->umis_cells = ctx->h_pinned[3];
  counts->umis_background = ctx->h_pinned[4];
  counts->threshold = ctx->h_pinned[5];
  counts->baseline = ctx->h_pinned[6];
  return IBU_OK;
}
// ---- per-barcode QC metrics and the barcode filter (k_metrics.hip).  The semantics are this library's: include/ibu_hip.h.
static_assert(sizeof(ibu_barcode_limits_t) == sizeof(MetricsLimits) && offsetof(ibu_barcode_limits_t, set_of) == offsetof(MetricsLimits, set_of) &&
                  offsetof(ibu_barcode_limits_t, set_num) == offsetof(MetricsLimits, set_num) && sizeof(ibu_barcode_filter_counts_t) == 96,
              "ibu_hip.h and kernels.h disagree");
static int32_t check_feature_set(const uint64_t* d_set, uint64_t set_bits, uint32_t set_word) {
  if (!metrics_set_ok(d_set, set_bits, set_word))
    return err_arg("the feature set: set_word must be 1 or 2, set_bits at most 2^32, d_set 8-byte aligned and non-NULL unless set_bits is 0");
  return IBU_OK;
}
// The first half of both: the count pass and its five totals read back into ctx->h_pinned[0..4].  Synchronises the stream.
static int32_t metrics_count_totals(ibu_ctx* ctx, const void* d_records, size_t n, const uint64_t* d_set, uint64_t set_bits, uint32_t set_word,
                                    hipStream_t st) {
  int32_t rc = ensure_sort_scratch(ctx, metrics_scratch_bytes(n));
  if (rc) return rc;
  IBU_HIP(launch_metrics_count(ctx->cfg, d_records, n, d_set, set_bits, set_word, ctx->d_sort_scratch, ctx->sort_scratch_bytes, st));
  IBU_HIP(hipMemcpyAsync(ctx->h_pinned, ctx->d_sort_scratch, 5 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  IBU_HIP(hipStreamSynchronize(st));
  return IBU_OK;
}
extern "C" int32_t ibu_barcode_metrics(ibu_ctx_t* ctx, const void* d_records, size_t n, const uint64_t* d_set, uint64_t set_bits,
                                       uint32_t set_word, uint64_t* d_barcodes, uint64_t* d_reads, uint64_t* d_pairs, uint64_t* d_triples,
                                       uint64_t* d_set_reads, uint64_t* d_set_triples, size_t cap, size_t* n_barcodes, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!n_barcodes) return err_arg("n_barcodes is NULL");
  rc = check_feature_set(d_set, set_bits, set_word);
  if (rc) return rc;
  if (n >= (1ull << 40)) return err_arg("barcode_metrics handles fewer than 2^40 records per call");
  if (n && (!d_records || !aligned8(d_records))) return err_arg("d_records must be non-NULL and 8-byte aligned");
  if (n && (!aligned8(d_barcodes) || !aligned8(d_reads) || !aligned8(d_pairs) || !aligned8(d_triples) || !aligned8(d_set_reads) ||
            !aligned8(d_set_triples)))
    return err_arg("the output arrays must be 8-byte aligned");
  *n_barcodes = 0;
  if (n == 0) return IBU_OK;
  hipStream_t st = pick_stream(ctx, stream);
  rc = metrics_count_totals(ctx, d_records, n, d_set, set_bits, set_word, st);
  if (rc) return rc;
  const uint64_t barcodes = ctx->h_pinned[0];
  *n_barcodes = barcodes;
  const bool any_column = d_barcodes || d_reads || d_pairs || d_triples || d_set_reads || d_set_triples;
  if (!any_column) return IBU_OK;   // the size query (cap == 0), or a cap and nothing to write
  if (barcodes > cap)
    return set_error(IBU_ERR_INVALID_ARG, barcodes, cap, 0, "Invalid argument: output capacity %llu is smaller than the %llu barcodes (see *n_barcodes)",
                     (unsigned long long)cap, (unsigned long long)barcodes);
  rc = ensure_runs_scratch(ctx, metrics_run_scratch_bytes(barcodes));
  if (rc) return rc;
  IBU_HIP(launch_metrics_table(ctx->cfg, d_records, n, d_set, set_bits, set_word, ctx->d_sort_scratch, ctx->d_runs_scratch, barcodes, d_barcodes,
                               d_reads, d_pairs, d_triples, d_set_reads, d_set_triples, st));
  return IBU_OK;
}
extern "C" int32_t ibu_filter_barcodes(ibu_ctx_t* ctx, const void* d_records, size_t n, const uint64_t* d_set, uint64_t set_bits,
                                       uint32_t set_word, const ibu_barcode_limits_t* limits, uint8_t* d_class,
                                       ibu_barcode_filter_counts_t* counts, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  rc = check_feature_set(d_set, set_bits, set_word);
  if (rc) return rc;
  if (!limits) return err_arg("limits is NULL");
  const MetricsLimits lim{limits->min_reads, limits->max_reads, limits->min_pairs, limits->max_pairs, limits->min_triples, limits->max_triples,
                          limits->set_num, limits->set_den, limits->set_of, 0};
  if (!metrics_limits_ok(lim)) return err_arg("limits: set_of must be 0 (reads) or 1 (triples), and set_num <= set_den < 2^24");
  if (n && (!d_records || !aligned8(d_records))) return err_arg("d_records must be non-NULL and 8-byte aligned");
  if (n >= (1ull << 40)) return err_arg("filter_barcodes handles fewer than 2^40 records per call");
  if (counts) *counts = ibu_barcode_filter_counts_t{};   // (behind the last argument check: a refused call leaves the totals alone)
  if (n == 0) return IBU_OK;
  hipStream_t st = pick_stream(ctx, stream);
  rc = metrics_count_totals(ctx, d_records, n, d_set, set_bits, set_word, st);
  if (rc) return rc;
  const uint64_t barcodes = ctx->h_pinned[0];
  rc = ensure_runs_scratch(ctx, metrics_run_scratch_bytes(barcodes));
  if (rc) return rc;
  IBU_HIP(launch_metrics_filter(ctx->cfg, d_records, n, d_set, set_bits, set_word, ctx->d_sort_scratch, ctx->d_runs_scratch, barcodes, lim, d_class, st));
  if (!counts) return IBU_OK;
  IBU_HIP(hipMemcpyAsync(ctx->h_pinned, ctx->d_runs_scratch, 10 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  IBU_HIP(hipStreamSynchronize(st));
  counts->barcodes = barcodes;
  for (int c = 0; c < 4; ++c) {
    counts->barcodes_by_class[c] = ctx->h_pinned[c];
    counts->reads_by_class[c] = ctx->h_pinned[4 + c];
  }
  counts->triples_passed = ctx->h_pinned[8];
  counts->set_triples_passed = ctx->h_pinned[9];
  return IBU_OK;
}
// ---- read subsampling and the saturation curve (k_saturation.hip).  The semantics are this library's: include/ibu_hip.h.
extern "C" int32_t ibu_subsample_class(ibu_ctx_t* ctx, size_t n, uint64_t first_row, uint64_t seed, uint64_t threshold, uint8_t* d_class,
                                       size_t* n_kept, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!d_class && !n_kept) return err_arg("d_class and n_kept are both NULL: nothing to do");
  if (n >= (1ull << 40)) return err_arg("subsample_class handles fewer than 2^40 rows per call");
  if (n_kept) *n_kept = 0;
  if (n == 0) return IBU_OK;
  hipStream_t st = pick_stream(ctx, stream);
  const uint64_t base = sample_base(seed, first_row);
  if (!n_kept) {   // nothing to bring back: the launch stays asynchronous and touches no per-call state
    IBU_HIP(launch_subsample(ctx->cfg, n, base, threshold, d_class, nullptr, st));
    return IBU_OK;
  }
  rc = ensure_sort_scratch(ctx, kSubsampleAccBytes);
  if (rc) return rc;
  IBU_HIP(launch_subsample(ctx->cfg, n, base, threshold, d_class, static_cast<uint64_t*>(ctx->d_sort_scratch), st));
  IBU_HIP(hipMemcpyAsync(ctx->h_pinned, ctx->d_sort_scratch, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  IBU_HIP(hipStreamSynchronize(st));
  *n_kept = ctx->h_pinned[0];
  return IBU_OK;
}
extern "C" int32_t ibu_saturation_curve(ibu_ctx_t* ctx, const void* d_sorted_records, size_t n, uint64_t first_row, uint64_t seed,
                                        const uint64_t* thresholds, uint32_t k, ibu_saturation_point_t* points, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (k == 0 || k > IBU_SATURATION_MAX_POINTS) return err_arg("k must be 1..32");
  if (!thresholds || !points) return err_arg("thresholds / points are NULL");
  for (uint32_t j = 1; j < k; ++j)
    if (thresholds[j] < thresholds[j - 1]) return err_arg("the thresholds must be non-decreasing");
  if (n && (!d_sorted_records || !aligned8(d_sorted_records))) return err_arg("d_sorted_records must be non-NULL and 8-byte aligned");
  if (n >= (1ull << 40)) return err_arg("saturation_curve handles fewer than 2^40 records per call");
  if (n == 0) {
    for (uint32_t j = 0; j < k; ++j) points[j] = ibu_saturation_point_t{thresholds[j], 0, 0, 0};
    return IBU_OK;
  }
  hipStream_t st = pick_stream(ctx, stream);
  rc = ensure_sort_scratch(ctx, saturation_scratch_bytes(n));
  if (rc) return rc;
  IBU_HIP(launch_saturation(ctx->cfg, d_sorted_records, n, sample_base(seed, first_row), thresholds, k, ctx->d_sort_scratch,
                            ctx->sort_scratch_bytes, st));
  static_assert(3 * kSaturationMaxPoints <= 128, "the points come back through h_pinned");
  IBU_HIP(hipMemcpyAsync(ctx->h_pinned, static_cast<const uint8_t*>(ctx->d_sort_scratch) + saturation_points_offset(),
                         3 * kSaturationMaxPoints * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  IBU_HIP(hipStreamSynchronize(st));
  for (uint32_t j = 0; j < k; ++j)
    points[j] = ibu_saturation_point_t{thresholds[j], ctx->h_pinned[j], ctx->h_pinned[kSaturationMaxPoints + j],
                                       ctx->h_pinned[2 * kSaturationMaxPoints + j]};
  return IBU_OK;
}
// TEST HOOK, not part of the ABI (not declared in include/ibu_hip.h, no binding): the selection ibu_call_cells runs, on a caller's
// array — *value = the rank-th largest (1 <= rank <= n) of n device values below 2^40.  Records cannot reach the digit passes above
// bit 31 at any size a test can afford; tests/test_gpu_cells.py reaches them through this.  Synchronises.
extern "C" int32_t ibu_test_rank_select(ibu_ctx_t* ctx, const uint64_t* d_values, size_t n, uint64_t rank, uint64_t* value, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!value) return err_arg("value is NULL");
  if (n == 0 || rank == 0 || rank > n) return err_arg("rank must be in 1..n");
  if (!d_values || !aligned8(d_values)) return err_arg("d_values must be non-NULL and 8-byte aligned");
  if (n >= (1ull << 40)) return err_arg("rank_select handles fewer than 2^40 values per call");
  hipStream_t st = pick_stream(ctx, stream);
  rc = ensure_runs_scratch(ctx, rank_select_work_bytes());
  if (rc) return rc;
  IBU_HIP(launch_rank_select(ctx->cfg, d_values, n, rank, ctx->d_runs_scratch, st));
  IBU_HIP(hipMemcpyAsync(ctx->h_pinned, ctx->d_runs_scratch, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  IBU_HIP(hipStreamSynchronize(st));
  *value = ctx->h_pinned[0];
  return IBU_OK;
}
extern "C" int32_t ibu_count_matrix(ibu_ctx_t* ctx, void* d_records, void* d_tmp, size_t n, uint32_t flags, uint64_t* d_barcodes,
                                    uint64_t* d_indices, uint64_t* d_reads, uint64_t* d_umis, size_t cap, size_t* n_entries,
                                    size_t* n_molecules, void* stream) {
  int32_t rc = check_ctx(ctx);
  if (rc) return rc;
  if (!n_entries) return err_arg("n_entries is NULL");
  *n_entries = 0;
  if (n_molecules) *n_molecules = 0;
  if (flags & ~(uint32_t)IBU_COUNT_LEAVE_SWAPPED) return err_arg("unknown bit in flags");
  if (n == 0) return IBU_OK;
  if (!d_records || !d_tmp || !aligned8(d_records) || !aligned8(d_tmp))
    return err_arg("d_records / d_tmp must be non-NULL and 8-byte aligned");
  if (!d_barcodes || !d_indices || !d_reads) return err_arg("d_barcodes / d_indices / d_reads are NULL");
  if (!aligned8(d_barcodes) || !aligned8(d_indices) || !aligned8(d_reads) || !aligned8(d_umis))
    return err_arg("the output arrays must be 8-byte aligned");
  if (n >= (1ull << 40)) return err_arg("count_matrix handles fewer than 2^40 records per call");
  if ((rc = ibu_records_swap_umi_index(ctx, d_records, d_records, n, stream)) != 0) return rc;
  if ((rc = ibu_sort_records(ctx, d_records, d_tmp, n, stream)) != 0) return rc;
  // a capacity that is too small is reported once the records are back in the state the flags promise
  const int32_t rc_counts = ibu_pair_counts(ctx, d_records, n, d_barcodes, d_indices, d_reads, d_umis, cap, n_entries, n_molecules, stream);
  if (!(flags & IBU_COUNT_LEAVE_SWAPPED) && (rc_counts == IBU_OK || rc_counts == IBU_ERR_INVALID_ARG))
    if ((rc = ibu_records_swap_umi_index(ctx, d_records, d_records, n, stream)) != 0) return rc;
  return rc_counts;
}
