// k_molecules.hip — ibu_classify_molecules: one index per (barcode, umi) molecule.  A molecule is a run of equal (w0, w1), a candidate
// a run of equal (w0, w1, w2) inside it; the candidate with strictly the most records is kept (class 0), the others are minor (1), and
// a molecule whose top is shared is tied (2) — include/ibu_hip.h has the rule in full.  Five steps, the records read twice:
//   count    launch_runs_count(RunsCount::Pair) of k_aggregate.hip, as for ibu_pair_counts: molecules and candidates per segment,
//            scanned; the two totals go back to the host to size the candidate table.
//   emit     the D = 2 walk of runs_walk.hpp again, with MolEmit as its sink: table[c] = first row of candidate c, bit 63 set where
//            it begins a molecule (8 bytes per candidate), and, when class bytes are wanted, the walk's own ballots of triple heads (16
//            bytes per 128-record tile) — the fill pass needs nothing else of the records.
//   verdict  one workgroup per 1024 candidates: reads(c) = start(c + 1) - start(c), a segmented scan of (best, how many at best, first
//            at best) over the block, every molecule's total dropped in LDS under its ordinal in the block and picked up by its
//            candidates.  Molecules inside a block are settled here (one verdict byte per candidate, the totals per wave, per block,
//            one atomic per block and total).  The piece in front of a block's first molecule head and the piece behind its last one
//            are left to the two kernels below together with their partial aggregates.
//   chains   one workgroup runs the same segmented scan over the blocks' summaries, 1024 per round: a molecule that leaves its
//            block gets its total at the block it began in.  fix: every block settles its two open pieces from those totals.  A
//            molecule of any length costs a constant per candidate this way: 1e6 candidates are 977 blocks, one round here.
//   fill     launch_class_fill of k_aggregate.hip: the ballots and the ranked heads' bases give each record's candidate number, the
//            verdicts leave as class bytes.
// Launcher: launch_molecules_classify (kernels.h); C ABI: ibu_classify_molecules (api_analysis.cpp).
#include "runs_walk.hpp"

namespace ibu {

static constexpr u64 kMolHead = 1ull << 63;
static constexpr u64 kRowMask = (1ull << 40) - 1;
static constexpr u32 kMolItems = 4;
static constexpr u32 kMolBlock = kSortThreads * kMolItems;    // candidates per verdict workgroup
static constexpr u32 kNoChain = 0xFFFFFFFFu;

// best reads << 4 | min(2, candidates at best) << 2 | min(2, candidates); first = the first candidate at best; s = the block a chain
// began in (ibu_k_molecules_chains only).  key == 0: nothing.
struct MolAgg { u64 key; u64 first; u32 s; };
__device__ __forceinline__ MolAgg mol_none() { return {0, 0, kNoChain}; }
__device__ __forceinline__ MolAgg mol_combine(const MolAgg a, const MolAgg b) {   // a in front of b
  const u64 ak = a.key, bk = b.key, af = a.first, bf = b.first;   // (values, not references: a select between two fields must not become one between two addresses)
  const u32 as = a.s, bs = b.s;
  const u64 ba = ak >> 4, bb = bk >> 4;
  const u32 ca = (u32)(ak >> 2) & 3u, cb = (u32)(bk >> 2) & 3u;
  u32 nn = ((u32)ak & 3u) + ((u32)bk & 3u);
  nn = nn < 2 ? nn : 2;
  u32 cc = ca + cb;
  cc = cc < 2 ? cc : 2;
  const bool a_wins = ba > bb, b_wins = bb > ba;
  MolAgg r;
  r.s = bs != kNoChain ? bs : as;
  r.key = ((a_wins ? ba : bb) << 4) | ((a_wins ? ca : b_wins ? cb : cc) << 2) | nn;
  r.first = (a_wins || (!b_wins && ca)) ? af : bf;
  return r;
}
struct MolScanLds { MolAgg v[kSortWaves]; u32 f[kSortWaves]; };
// Segmented scan over the 256 threads of a workgroup.  Thread t brings (f, v): f = one of its items begins a segment, v = the aggregate
// of its items behind its last segment start (all of them when f is false).  Returns what is open in front of the thread — the
// aggregate from the last segment start before it, `carry` included where no thread in front has one — and leaves in *total what is
// open behind the last thread.
__device__ __forceinline__ MolAgg mol_block_scan(bool f, MolAgg v, const MolAgg& carry, MolScanLds* lds, MolAgg* total) {
  const u32 lane = threadIdx.x & (kWave - 1), wib = threadIdx.x >> 6;
  u32 ff = f ? 1u : 0u;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    MolAgg p;
    p.key = shfl_up64(v.key, d); p.first = shfl_up64(v.first, d); p.s = __shfl_up(v.s, d);
    const u32 pf = __shfl_up(ff, d);
    if (lane >= (u32)d) {
      if (!ff) v = mol_combine(p, v);
      ff |= pf;
    }
  }
  if (lane == kWave - 1) { lds->v[wib] = v; lds->f[wib] = ff; }
  __syncthreads();
  MolAgg in = carry, all = carry;                          // open in front of this wave / behind the last one
#pragma unroll
  for (int w = 0; w < kSortWaves; ++w) {
    const MolAgg wv = lds->v[w];
    all = lds->f[w] ? wv : mol_combine(all, wv);
    if ((u32)w + 1 == wib) in = all;
  }
  __syncthreads();                                          // the slots may be reused by the caller's next scan
  *total = all;
  const MolAgg inc = ff ? v : mol_combine(in, v);
  MolAgg ex;
  ex.key = shfl_up64(inc.key, 1); ex.first = shfl_up64(inc.first, 1); ex.s = __shfl_up(inc.s, 1);
  return lane == 0 ? in : ex;
}
__device__ __forceinline__ u32 mol_class(const MolAgg& m, u64 c, u32 tie_first) {
  if (((m.key >> 2) & 3u) >= 2 && !tie_first) return 2;     // IBU_MOLECULE_TIED
  return c == m.first ? 0u : 1u;                            // KEPT : MINOR
}
// one candidate into a thread's five totals (static indices only: the array stays in registers), which block_accumulate adds into
// acc: [0] resolved molecules, [1] tied molecules, [2..4] records of class 0, 1, 2
__device__ __forceinline__ void mol_tally(u64 (&t)[5], u32 cls, u64 reads, bool mol_head, u64 key) {
  t[2] += cls == 0 ? reads : 0;
  t[3] += cls == 1 ? reads : 0;
  t[4] += cls == 2 ? reads : 0;
  const bool several = mol_head && (key & 3u) >= 2, top_shared = ((key >> 2) & 3u) >= 2;
  t[0] += several && !top_shared ? 1 : 0;
  t[1] += several && top_shared ? 1 : 0;
}

struct MolEmit : BallotSink {                               // keeps the ballots of triple heads
  u64* table;
  __device__ __forceinline__ void head(u64, u64 c, u64 row, u64, u64, bool mol_head) const { table[c] = row | (mol_head ? kMolHead : 0); }
  __device__ __forceinline__ void ballots(u64 at, bool tiled, u64, u64, u64 even, u64 odd) const { keep(at, tiled, even, odd); }
};
extern "C" __global__ void __launch_bounds__(kSortThreads, 8)
ibu_k_molecules_emit(const u64* __restrict__ recs, SegPlan sp, const u64* __restrict__ seg_base /*[2][nseg], scanned*/, u64* __restrict__ table,
                     u64* __restrict__ masks /*nullable*/) {
  runs_kernel<2>(recs, sp, seg_base, nullptr, MolEmit{{{}, masks}, table});
}

// What a verdict block leaves for the chain scan: the aggregate of the candidates in front of its first molecule head (`lead`, all
// of the block when it has none) and of those from its last molecule head on when that molecule goes on in the next block (`trail`).
struct __attribute__((aligned(16))) MolSummary { u64 lead_key, lead_first, trail_key, trail_first; u32 lead_len, trail_off, has_head, open; };
struct __attribute__((aligned(16))) MolFull { u64 key, first; };

extern "C" __global__ void __launch_bounds__(kSortThreads)
ibu_k_molecules_verdict(const u64* __restrict__ table, u64 ncand, u64 n, u32 tie_first, uint8_t* __restrict__ verdict, MolSummary* __restrict__ summary,
                        u64* __restrict__ acc) {
  __shared__ MolFull tot[kMolBlock + 1];                    // slot 0: the lead piece; slot m: the block's m-th molecule
  __shared__ MolScanLds scan;
  __shared__ u32 wsum[kSortWaves];
  __shared__ u64 accl[kSortWaves * 5];
  __shared__ u32 s_lead_len, s_trail_off, s_open;
  const u32 tid = threadIdx.x;
  const u64 base = (u64)blockIdx.x * kMolBlock, c0 = base + kMolItems * tid;
  const u32 in_block = (u32)(ncand - base < kMolBlock ? ncand - base : kMolBlock);
  if (tid == 0) { s_lead_len = in_block; s_trail_off = 0; s_open = 0; }
  const u64 sentinel = n | kMolHead;
  u64 e[kMolItems + 1];
#pragma unroll
  for (u32 j = 0; j <= kMolItems; ++j) e[j] = c0 + j < ncand ? table[c0 + j] : sentinel;
  auto reads_of = [&](u32 j) { return (e[j + 1] & kRowMask) - (e[j] & kRowMask); };
  auto item_of = [&](u32 j) { return c0 + j < ncand ? MolAgg{(reads_of(j) << 4) | 5u, c0 + j, kNoChain} : mol_none(); };
  MolAgg run = mol_none();
  bool seen = false;
  u32 nh = 0;
#pragma unroll
  for (u32 j = 0; j < kMolItems; ++j) {
    const bool valid = c0 + j < ncand;
    const MolAgg item = item_of(j);
    if (e[j] & kMolHead) { run = item; seen = true; nh += valid ? 1u : 0u; }
    else run = mol_combine(run, item);
  }
  MolAgg unused;
  run = mol_block_scan(seen, run, mol_none(), &scan, &unused);   // now: what is open in front of this thread's candidates
  u32 nheads;
  u32 m = block_exclusive_scan(nh, wsum, &nheads);           // molecule heads of the block in front of this thread
  u32 slot[kMolItems];
#pragma unroll
  for (u32 j = 0; j < kMolItems; ++j) {
    const bool valid = c0 + j < ncand;
    const MolAgg item = item_of(j);
    const bool head = valid && (e[j] & kMolHead);
    run = (e[j] & kMolHead) ? item : mol_combine(run, item);  // the molecule from its beginning in the block to this candidate
    if (head) {
      ++m;
      if (m == 1) s_lead_len = kMolItems * tid + j;
      if (m == nheads) s_trail_off = kMolItems * tid + j;
    }
    const bool block_end = kMolItems * tid + j + 1 == kMolBlock;
    if (valid && ((e[j + 1] & kMolHead) || block_end)) {
      tot[m] = MolFull{run.key, run.first};
      if (block_end && !(e[j + 1] & kMolHead)) s_open = 1;
    }
    slot[j] = m;
  }
  __syncthreads();
  const u32 open = nheads ? s_open : 0;                     // (a block without a molecule head is all lead)
  u64 t[5] = {0, 0, 0, 0, 0};
  u32 packed = 0;
#pragma unroll
  for (u32 j = 0; j < kMolItems; ++j) {
    const bool settled = c0 + j < ncand && slot[j] >= 1 && !(open && slot[j] == nheads);
    if (settled) {
      const MolFull f = tot[slot[j]];
      const MolAgg mol{f.key, f.first, 0};
      const u32 cls = mol_class(mol, c0 + j, tie_first);
      packed |= cls << (8 * j);
      mol_tally(t, cls, reads_of(j), (e[j] & kMolHead) != 0, f.key);
    }
  }
  if (c0 < ncand) *reinterpret_cast<u32*>(verdict + c0) = packed;   // (the array is padded to a multiple of four; open pieces: ibu_k_molecules_fix)
  if (tid == 0) {
    MolSummary sm;
    const bool has_lead = s_lead_len > 0;
    sm.lead_key = has_lead ? tot[0].key : 0; sm.lead_first = has_lead ? tot[0].first : 0;
    sm.trail_key = open ? tot[nheads].key : 0; sm.trail_first = open ? tot[nheads].first : 0;
    sm.lead_len = s_lead_len; sm.trail_off = s_trail_off; sm.has_head = nheads ? 1u : 0u; sm.open = open;
    summary[blockIdx.x] = sm;
  }
  block_accumulate(t, acc, accl);
}

// One workgroup.  Block j enters the scan as a segment start with its trail when it has a molecule head, and as its lead (all of
// it) otherwise; what is open in front of j, joined with j's lead, is the total of the molecule that ends in j.  A molecule that
// ends on the last candidate of a block without a head ends in no block's lead: its total is what is open in front of the next block.
extern "C" __global__ void __launch_bounds__(kSortThreads)
ibu_k_molecules_chains(const MolSummary* __restrict__ summary, u32 nblk, u32* __restrict__ chain_start, MolFull* __restrict__ chain_full) {
  __shared__ MolScanLds scan;
  MolAgg carry = mol_none();
  for (u32 base = 0; base < nblk; base += kMolBlock) {      // (block-uniform trip count: the scan has barriers)
    const u32 j0 = base + kMolItems * threadIdx.x;
    MolAgg run = mol_none();
    bool seen = false;
#pragma unroll
    for (u32 k = 0; k < kMolItems; ++k) {
      if (j0 + k < nblk) {
        const MolSummary sm = summary[j0 + k];
        if (sm.has_head) { run = MolAgg{sm.trail_key, sm.trail_first, j0 + k}; seen = true; }
        else run = mol_combine(run, MolAgg{sm.lead_key, sm.lead_first, kNoChain});
      }
    }
    MolAgg total;
    run = mol_block_scan(seen, run, carry, &scan, &total);    // now: what is open in front of this thread's blocks
    carry = total;
#pragma unroll
    for (u32 k = 0; k < kMolItems; ++k) {
      const u32 j = j0 + k;
      if (j < nblk) {
        const MolSummary sm = summary[j];
        const MolAgg lead{sm.lead_key, sm.lead_first, kNoChain};
        if (sm.lead_len && run.s != kNoChain) {
          chain_start[j] = run.s;
          if (sm.has_head || j + 1 == nblk) { const MolAgg f = mol_combine(run, lead); chain_full[run.s] = MolFull{f.key, f.first}; }
        } else if (!sm.lead_len && run.key && run.s != kNoChain) {
          // a molecule head on the block's first candidate: the chain that came through blocks without a head ended on the last
          // candidate of j - 1 (run.key == 0: j - 1 has a head and is not open, nothing comes in)
          chain_full[run.s] = MolFull{run.key, run.first};
        }
        run = sm.has_head ? MolAgg{sm.trail_key, sm.trail_first, j} : mol_combine(run, lead);
      }
    }
  }
}

extern "C" __global__ void __launch_bounds__(kSortThreads)
ibu_k_molecules_fix(const u64* __restrict__ table, u64 ncand, u64 n, u32 tie_first, const MolSummary* __restrict__ summary,
                    const u32* __restrict__ chain_start, const MolFull* __restrict__ chain_full, uint8_t* __restrict__ verdict, u64* __restrict__ acc) {
  __shared__ u64 accl[kSortWaves * 5];
  const MolSummary sm = summary[blockIdx.x];
  if (!sm.lead_len && !sm.open) return;                     // block-uniform: every molecule of the block was settled in it
  const u64 base = (u64)blockIdx.x * kMolBlock;
  const u32 in_block = (u32)(ncand - base < kMolBlock ? ncand - base : kMolBlock);
  u64 t[5] = {0, 0, 0, 0, 0};
  for (int piece = 0; piece < 2; ++piece) {
    if (piece == 0 ? !sm.lead_len : !sm.open) continue;
    u32 from = piece == 0 ? chain_start[blockIdx.x] : blockIdx.x;
    from = from < gridDim.x ? from : 0;                      // (never taken: a lead piece has a block with a molecule head in front of it)
    const MolFull f = chain_full[from];
    const MolAgg mol{f.key, f.first, 0};
    const u32 lo = piece == 0 ? 0 : sm.trail_off, hi = piece == 0 ? sm.lead_len : in_block;
    for (u32 i = lo + threadIdx.x; i < hi; i += kSortThreads) {
      const u64 c = base + i;
      const u64 next = c + 1 < ncand ? table[c + 1] & kRowMask : n;
      const u32 cls = mol_class(mol, c, tie_first);
      verdict[c] = (uint8_t)cls;
      mol_tally(t, cls, next - (table[c] & kRowMask), piece == 1 && i == lo /*the molecule head is here*/, f.key);
    }
  }
  block_accumulate(t, acc, accl);
}

// run scratch: acc u64[8] | table u64[ncand] | verdict bytes | summaries | chain starts | chain totals
struct MolLayout { size_t table, verdict, summary, chain_start, chain_full, bytes; u32 nblk; };
static MolLayout mol_layout(uint64_t ncand) {
  MolLayout L;
  L.nblk = (u32)((ncand + kMolBlock - 1) / kMolBlock);
  const size_t nb = L.nblk ? L.nblk : 1;
  L.table = 64;
  L.verdict = align_up(L.table + 8 * (size_t)(ncand ? ncand : 1), 16);
  L.summary = align_up(L.verdict + (size_t)ncand + 4, 16);
  L.chain_start = align_up(L.summary + sizeof(MolSummary) * nb, 16);
  L.chain_full = align_up(L.chain_start + sizeof(u32) * nb, 16);
  L.bytes = align_up(L.chain_full + sizeof(MolFull) * nb, 16);
  return L;
}
size_t molecules_run_scratch_bytes(uint64_t candidates) { return mol_layout(candidates).bytes; }
size_t molecules_scratch_bytes(size_t n) { return runs_layout(n).mol_bytes; }
hipError_t launch_molecules_classify(const LaunchCfg& cfg, const void* recs, size_t n, void* scratch, void* run_scratch, uint64_t candidates,
                                     bool tie_first, uint8_t* d_class, hipStream_t st) {
  (void)hipGetLastError();
  if (candidates == 0 || candidates > n || n >= (1ull << 40)) return hipErrorInvalidValue;
  const SegPlan sp = seg_plan(cfg, recs, n);
  const RunsLayout R = runs_layout(n);
  const u64* base = scratch_at<const u64>(scratch, R.seg_base);
  u64* masks = d_class ? scratch_at<u64>(scratch, R.mol_masks) : nullptr;
  const MolLayout L = mol_layout(candidates);
  uint8_t* rs = static_cast<uint8_t*>(run_scratch);
  u64* acc = reinterpret_cast<u64*>(rs);
  u64* table = reinterpret_cast<u64*>(rs + L.table);
  uint8_t* verdict = rs + L.verdict;
  MolSummary* summary = reinterpret_cast<MolSummary*>(rs + L.summary);
  u32* chain_start = reinterpret_cast<u32*>(rs + L.chain_start);
  MolFull* chain_full = reinterpret_cast<MolFull*>(rs + L.chain_full);
  hipError_t e = hipMemsetAsync(acc, 0, 64, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ibu_k_molecules_emit, seg_grid(sp), dim3(kSortThreads), 0, st, (const u64*)recs, sp, base, table, masks);
  hipLaunchKernelGGL(ibu_k_molecules_verdict, dim3(L.nblk), dim3(kSortThreads), 0, st, (const u64*)table, (u64)candidates, (u64)n,
                     tie_first ? 1u : 0u, verdict, summary, acc);
  hipLaunchKernelGGL(ibu_k_molecules_chains, dim3(1), dim3(kSortThreads), 0, st, (const MolSummary*)summary, L.nblk, chain_start, chain_full);
  hipLaunchKernelGGL(ibu_k_molecules_fix, dim3(L.nblk), dim3(kSortThreads), 0, st, (const u64*)table, (u64)candidates, (u64)n,
                     tie_first ? 1u : 0u, (const MolSummary*)summary, (const u32*)chain_start, (const MolFull*)chain_full, verdict, acc);
  if (d_class) return launch_class_fill(cfg, recs, n, scratch, true, verdict, d_class, st);
  return hipGetLastError();
}

}  // namespace ibu
