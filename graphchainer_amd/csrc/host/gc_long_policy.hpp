// The whole-read pass's sizing and growth rules (batch/gc_long_pass.hip is their one user): how many alignment slots, trace cells, work entries, scratch lanes and blocks a
// batch gets, how many candidate seeds a round tries, and by how much a pool that overflowed grows. Arithmetic only - every rule is the expression the pass used to hold
// inline between its HIP calls, with the same integer types; the capacity overrides (gc_params::capacity, GC_TEST_*) stay at the call sites.
// Standard library only: tests/long_policy_host builds it without HIP.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <optional>

namespace gc {

// ---- alignment slots
// alignments kept per read: the reference has no limit; 32 is far above what 10 kb reads produce (3.6 seeds extended on average), longer
// and noisier reads get room in proportion. A read that needs more (a read inside a tandem array collects 40-130) ends with status 3 and runs
// again with four times the slots (longAlnSlotGrowth), so the common read pays for 32 and no read is cut short at them.
inline uint32_t longFirstAlnCap(uint64_t maxReadLen) { return (uint32_t)std::max<uint64_t>(32, maxReadLen / 512); }

// A read that found more alignments than it had slots for gets four times as many. An alignment comes from a seed of its own, so a read with as many slots as seeds cannot
// run out; the limit beyond which a read is flagged instead is LONG_ALN_SLOTS_MAX per read and 2^32 slots per batch.
// Returns the read's new number of slots, or nothing when it cannot be given more (cap: its slots now; seeds: its seed count; total: the batch's slots so far).
inline constexpr uint32_t LONG_ALN_SLOTS_MAX = 1u << 16;
inline std::optional<uint32_t> longAlnSlotGrowth(uint32_t cap, uint32_t seeds, uint64_t total)
{
	const uint32_t limit = std::min<uint32_t>(LONG_ALN_SLOTS_MAX, std::max<uint32_t>(1, seeds));
	if (cap >= limit) return std::nullopt;
	const uint32_t next = (uint32_t)std::min<uint64_t>(limit, 4ull * cap);
	if (total + next >= 0xffffffffull) return std::nullopt;
	return next;
}

// ---- the merged-trace cell pool
// cells per read base + slack per read (offsets: the batch's read offsets, n + 1 of them)
inline uint64_t longCellBudget(const uint64_t* offsets, uint64_t n, uint64_t perBase) { uint64_t b = 0; for (uint64_t r = 0; r < n; r++) b += perBase * (offsets[r + 1] - offsets[r]) + 1024; return b; }
// a pool is not grown beyond 256 cells per read base or 64 GB (cells: longCellBudget at perBase)
inline bool longCellPoolRefused(uint64_t perBase, uint64_t cells, uint64_t cellBytes) { return perBase > 256 || cells * cellBytes > (64ull << 30); }
// the pass runs again after the rounds overflowed the pool.
// r5: by what the pass asked for, not three times the last size (8 -> 24 cells per read base put 38 GB into a 2 000 x 50 kb batch in flight): the pool's cursor counts every
// request, refused ones included; a read that was refused stops asking, so the count is a lower bound - half as much again, and the loop comes back if that is still short
inline uint64_t longCellsPerBaseForRerun(uint64_t cur, uint64_t asked, uint64_t bases) { return std::max<uint64_t>(cur + 2, (asked + asked / 2 + bases - 1) / bases); }
// the plain-layout reruns found the pool full: it doubles in place
inline uint64_t longCellsPerBaseDoubled(uint64_t cur) { return std::min<uint64_t>(256, cur * 2); }

// ---- one extension's sizes, from the batch's longest read (L) and "force_global or precise clipping"
struct LongExtendSizes {
	uint32_t maxSlices, maxItems, maxPending, maxTrace;
	int64_t defaultCols;   // the column store when neither the parameters nor the environment name one
};
inline LongExtendSizes longExtendSizes(uint64_t maxReadLen, bool globalOrClip)
{
	LongExtendSizes s;
	s.maxSlices = (uint32_t)(maxReadLen / 64 + 3);
	s.maxItems = (uint32_t)std::max<uint64_t>(8192, (maxReadLen / 64 + 3) * 24);   // (slice, node) tiles of one extension: ~8 per slice on cfg2, room for 24
	s.maxPending = 96;
	// (an extension's trace: rows + 1 + score cells. force_global keeps every slice, so the score reaches the rows)
	// (precise clipping keeps slices the correctness trim would drop: the trace is bounded by the rows and the score as under force_global)
	s.maxTrace = globalOrClip ? (uint32_t)(2 * maxReadLen + 2 + 512) : (uint32_t)(maxReadLen + maxReadLen / 2 + 512);
	// column store of the one-extension-per-wave kernel: the DP keeps every column (16 B) so that the backtrace loads its tiles' columns back instead of
	// recomputing them (45 % of the kernel's column steps). ~2.1 columns per read row on cfg2; an extension that needs more than this room ends
	// with EXT_OVERFLOW and its read goes to the plain-layout kernel, which recomputes. GC_TEST_LONG_MAX_COLS=0: no store (the r2 behaviour).
	s.defaultCols = (int64_t)(3 * maxReadLen + 4096);
	return s;
}

// ---- the rounds
// words of the rounds' trace pool: up to four candidate seeds' worth per read (the speculation rule below keeps rounds within it); a seed's two traces: len + 1 + score cells
inline uint64_t longRoundTraceBudget(const uint64_t* offsets, uint64_t n, bool globalOrClip)
{
	uint64_t budget = 0;
	for (uint64_t r = 0; r < n; r++) { uint64_t len = offsets[r + 1] - offsets[r]; budget += 4 * ((globalOrClip ? 2 * len + 2 : len + len / 2) + 1024); }
	return budget;
}
inline uint64_t longWorkCapacity(uint64_t n) { return 8 * n + 64; }   // entries of the rounds' work arrays
// extension scratch: one region per lane of a resident wave (persistent waves fetch work items), bounded by a memory budget in bytes
// (r5: no more lanes than a round can hold without speculation - two work items per read; the late rounds' speculation stays below that, and a round that does exceed
// it runs persistent waves. A 2 000 x 50 kb batch reserved 48 GB for rounds of 4 000 extensions, a 10 k x 10 kb batch 48 GB for 20 000: now 20 and 27 GB)
inline uint64_t longScratchLanes(uint64_t workCapacity, uint64_t n, uint64_t scratchBudget, uint64_t waveWords)
{
	return std::min<uint64_t>(std::min<uint64_t>(workCapacity + 64, 2 * n + 128), std::max<uint64_t>(2048, std::min<uint64_t>(65536 + 64, scratchBudget / (waveWords * 8))));
}
// candidate seeds per read in a round (lastWork: the round before's work items; n: reads of the batch).
// tail rounds: once fewer than a quarter of the reads are still active the chip is mostly idle, so the
// remaining reads try several seeds per round (exact: k_long_merge re-checks them in order)
// (the number of work items stays below what round 0 had: active reads x candidates <= n)
inline uint32_t longCandidatesPerRead(int round, uint32_t lastWork, uint64_t n)
{
	uint32_t maxCand = 1;
	if (round > 0 && lastWork > 0) maxCand = (uint32_t)std::min<uint64_t>(8, std::max<uint64_t>(1, (2 * n) / lastWork));
	if (round > 0 && lastWork < 8192) maxCand = 8;   // fewer work items than wave slots: the round costs one extension's latency whatever it holds
	// at most lastWork/2 reads are still active, so this keeps the round within the work arrays (8 per read) and the trace budget (4 seeds' worth per read)
	if (round > 0 && lastWork > 0) maxCand = (uint32_t)std::min<uint64_t>(maxCand, std::max<uint64_t>(1, (8 * n) / lastWork));
	return maxCand;
}
// blocks of a round's extension launch (team: lanes per wave sharing one extension), and of its retry launch (two lanes per wave):
// (persistent waves over a list that is almost always empty on 10 kb reads; 50 kb CLR-like reads on a genome-sized graph list a few dozen per round, and one such extension lasts 10-50 ms)
inline uint32_t longRoundBlocks(uint32_t nWorkItems, uint32_t team, uint64_t scratchLanes) { return std::min<uint32_t>((nWorkItems + team - 1) / team, (uint32_t)std::max<uint64_t>(1, (scratchLanes - 64) / team)); }
inline uint32_t longRetryBlocks(uint64_t scratchLanes) { return std::min<uint32_t>(128, (uint32_t)std::max<uint64_t>(1, (scratchLanes - 64) / 2)); }

// ---- passes side by side
// r5: how many passes may run side by side on a device is decided per batch. A pass whose rounds cannot fill the chip - round 0 holds two work items per read, k_long_extend<1> has
// 5 120 wave slots (256 CUs x 4 SIMDs x 5 waves) - shares the device with a second one: 2 000 x 50 kb reads on a 192 Mbp graph 4.0-4.2 k -> 5.0-5.3 k reads/s (`gpurun_out/r5_cfg5_tok`);
// a pass that fills it (10 k x 10 kb: 20 000 items) keeps the device to itself (two side by side measured slower in r4). GC_LONG_TOKENS=1|2 overrides (read per batch: the tests switch
// inside one process). The second token has a scratch of its own and is only taken when the device has the memory for it.
inline constexpr uint64_t LONG_WAVE_SLOTS = 5120;
// r6: ... and only while the fragment pipeline leaves the device room for it, told by the fragment extensions the stream's previous batch ran per read base (a count, not a time:
// times under five batches in flight are residencies, and a rule on them would feed back on itself). On a 192 Mbp graph that is 0.09 and two passes side by side gave 4.2 -> 5.0 k
// reads/s (r5); at 960 Mbp, where chance hits of 15-mers make it 0.42, the second pass that r6's freed memory suddenly had room for cost 4.31 -> 3.63 k (`gpurun_out/r6_cfg5_960p` / `_960q`)
inline int longTokenCount(std::optional<int> tokensOverride, uint64_t nReads, uint64_t streamBatchesDone, double extensionsPerBase)
{
	if (tokensOverride) return *tokensOverride;
	// (a stream's first batch sizes its buffers - pools that rerun and grow: a second scratch taken while the device still looks empty cost config 5 at 960 Mbp its fifth stream)
	return streamBatchesDone > 0 && 2 * nReads + 128 <= LONG_WAVE_SLOTS && extensionsPerBase < 0.2 ? 2 : 1;
}

} // namespace gc
