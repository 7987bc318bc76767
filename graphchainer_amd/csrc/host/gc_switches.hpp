// The GC_* environment switches of the library (INTEGRATION.md §7 is the reader's table): which exist, their defaults, their ranges. Switches::fromEnvironment() is the one
// place the library reads them; everything else reads a field of a snapshot.
// When a snapshot is taken: once per process (processSwitches(): how the host waits, the worker pools' sizes and CPU accounting, the result block cache), once per
// gc_align_batch / gc_align_batch_seeded (BatchRun holds it: a batch sees one value per variable from start to end), and once per call of the other entry points that read
// one (gc_edit_distance, gc_seeder_create, the graph upload, the graph builders, StageClock). Standard library only: host/gc_graph.cpp is also built without HIP.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <optional>

namespace gc {

inline constexpr int LONG_TOKENS_MAX = 2;   // whole-read passes side by side on a device, at most (gc_runtime.hpp: PassTokens)

struct Switches {
	// ---- host set-up
	std::optional<size_t> hostThreads;             // GC_HOST_THREADS: threads of the wide worker pool (output encoders)
	std::optional<size_t> batchThreads;            // GC_BATCH_THREADS: threads of the batch pipeline's own pool
	std::optional<size_t> buildThreads;            // GC_BUILD_THREADS: threads of the first graph build (values below 1 are ignored)
	size_t resultCacheMin = 32ull << 20;           // GC_RESULT_CACHE_MIN: the smallest result array (bytes) the library keeps for reuse
	// ---- run time
	int spinSync = 2;                              // GC_SPIN_SYNC: how the host waits for a stream: 2 poll + sleep, 1 spin, 0 blocking event wait
	int syncPollUs = 40;                           // GC_SYNC_POLL_US: the first sleep between two polls
	int longToken = 1;                             // GC_LONG_TOKEN: 0 no whole-read token, passes of batches in flight overlap (see the two functions below)
	std::optional<int> longTokens;                 // GC_LONG_TOKENS: how many passes may run side by side on a device (unset: decided per batch)
	bool debugTimes = false;                       // GC_DEBUG_TIMES: stage times, CPU, pool sizes to stderr
	bool debugEd = false;                          // GC_DEBUG_ED: every chain edit-distance pair with its band to stderr
	// ---- fall-back paths kept for A/B and tests, same results
	bool hostAnchors = false;                      // GC_HOST_ANCHORS=1: the result's anchor arrays from the host's walk over the slots
	bool extLazy = true;                           // GC_EXT_LAZY=0: every seed extended up front
	bool extendSlab = false;                       // GC_EXTEND_SLAB=1: fragment extensions by the plain-layout kernel on per-lane slabs
	bool hostStitch = false;                       // GC_HOST_STITCH: chain stitching on the host workers
	std::optional<int> stitchClass;                // GC_STITCH_CLASS: forces the stitching kernel's class, 3 or 0 (unset: by read length)
	bool chainPlainScan = false;                   // GC_CHAIN_PLAIN_SCAN=1: the chaining scratch launch scans its threshold lists plainly
	std::optional<uint32_t> edFirstK;              // GC_ED_FIRST_K: gc_edit_distance's first band, treated as a bound
	bool seederBuildOnHost = false;                // GC_SEEDER_BUILD=host: the minimizer index built by the host
	bool buildReferenceContainers = false;         // GC_BUILD_REFERENCE_CONTAINERS=1: the first graph build on the reference's own container types
	// ---- test hooks (GC_TEST_*: not for a host); the capacities win over gc_params::capacity (capacityOr)
	std::optional<int64_t> testExtMaxItems;        // GC_TEST_EXT_MAX_ITEMS: (slice, node) tiles of a fragment extension
	std::optional<int64_t> testExtMaxPending;      // GC_TEST_EXT_MAX_PENDING: queue entries of a fragment extension
	std::optional<int64_t> testExtMaxTrace;        // GC_TEST_EXT_MAX_TRACE: trace cells of a fragment extension
	std::optional<uint32_t> testExtRetryMaxItems;  // GC_TEST_EXT_RETRY_MAX_ITEMS: tiles of the retry launch, so that the retry overflows too
	std::optional<int64_t> testLongMaxItems;       // GC_TEST_LONG_MAX_ITEMS: tiles of a whole-read extension
	std::optional<int64_t> testLongMaxCols;        // GC_TEST_LONG_MAX_COLS: the whole-read kernel's column store (0: none)
	std::optional<int64_t> testLongCellsPerBase;   // GC_TEST_LONG_CELLS_PER_BASE: merged-trace cells per read base (pins the pool)
	std::optional<uint32_t> testLongMaxAlignments; // GC_TEST_LONG_MAX_ALIGNMENTS: the alignment slots a read starts with
	std::optional<uint64_t> testLongScratchGb;     // GC_TEST_LONG_SCRATCH_GB: the whole-read extension scratch's budget
	std::optional<int64_t> testStitchSetMax;       // GC_TEST_STITCH_SET_MAX: the stitching kernel's node set
	std::optional<int64_t> testStitchBfsCap;       // GC_TEST_STITCH_BFS_CAP: the stitching kernel's bridge search
	std::optional<uint32_t> testSeedFilterBits;    // GC_TEST_SEED_FILTER_BITS: log2 of the seeder's membership filter
	std::optional<long> testFailLong;              // GC_TEST_FAIL_LONG: this read's whole-read pass "asserts" (shared with the oracle)
	bool testLongForceFallback = false;            // GC_TEST_LONG_FORCE_FALLBACK: every read through the plain-layout kernel too
	std::optional<uint32_t> testLongRegCap;        // GC_TEST_LONG_REG_CAP: the whole-read kernel's register tables, to force the LDS-table retry
	std::optional<uint32_t> testLongMaxBlocks;     // GC_TEST_LONG_MAX_BLOCKS: blocks of a round's extension launch, to force persistent waves
	std::optional<uint32_t> testLongTeam;          // GC_TEST_LONG_TEAM: lanes per wave of the whole-read kernel (1, 2, 4, ..., 64; anything else is ignored)
	uint32_t testLongOrder = 1;                    // GC_TEST_LONG_ORDER: 0 runs a round's extensions as emitted, not longest first
	std::optional<uint32_t> testLongSpeculate;     // GC_TEST_LONG_SPECULATE: candidate seeds per read and round, from round 0
	bool testChainForceScratch = false;            // GC_TEST_CHAIN_FORCE_SCRATCH: every read through the chaining scratch launch
	std::optional<double> testPoolFirstGuess;      // GC_TEST_POOL_FIRST_GUESS: trace cells per slot a stream's first batch guesses
	size_t testPoolShrinkFloor = 64u << 20;        // GC_TEST_POOL_SHRINK_FLOOR: pools below this many spare bytes do not shrink
	bool testResultCachePoison = false;            // GC_TEST_RESULT_CACHE_POISON: result arrays are filled with 0xA5 when handed out
	size_t testUploadSlice = (size_t)64 << 20;     // GC_TEST_UPLOAD_SLICE: backward links per slice of the graph upload
	size_t testSeedfilePiece = (size_t)32 << 20;   // GC_TEST_SEEDFILE_PIECE: bytes of messages per piece a seed store uploads (a longer message makes the piece grow)
	uint32_t testSeedfileHashBits = 64;            // GC_TEST_SEEDFILE_HASH_BITS: only that many bits of a seed store's name hash are kept (1..64), to force collisions

	bool shareLongScratch() const { return longToken >= 1; }   // the pass works in the device's shared scratch (whoever holds the token owns it)
	bool onePassAtATime() const { return longToken != 0; }     // the pass takes the device's token

	// the two hooks of the seed store (gc_seed_store_open); tests/test_seedfile_switches_host.py holds their cases
	static const char* seedfileSwitch(const char* name) { return getenv(name); }

	static Switches fromEnvironment()
	{
		Switches s;
		if (const char* e = getenv("GC_HOST_THREADS")) s.hostThreads = (size_t)std::max(1, atoi(e));
		if (const char* e = getenv("GC_BATCH_THREADS")) s.batchThreads = (size_t)std::max(1, atoi(e));
		if (const char* e = getenv("GC_BUILD_THREADS")) { long v = atol(e); if (v >= 1) s.buildThreads = (size_t)v; }
		if (const char* e = getenv("GC_RESULT_CACHE_MIN")) s.resultCacheMin = (size_t)std::max(1ll, atoll(e));

		if (const char* e = getenv("GC_SPIN_SYNC")) s.spinSync = atoi(e);
		if (const char* e = getenv("GC_SYNC_POLL_US")) s.syncPollUs = std::max(1, atoi(e));
		if (const char* e = getenv("GC_LONG_TOKEN")) s.longToken = atoi(e);
		if (const char* e = getenv("GC_LONG_TOKENS")) s.longTokens = std::max(1, std::min(LONG_TOKENS_MAX, atoi(e)));
		s.debugTimes = getenv("GC_DEBUG_TIMES") != nullptr;
		s.debugEd = getenv("GC_DEBUG_ED") != nullptr;

		if (const char* e = getenv("GC_HOST_ANCHORS")) s.hostAnchors = atoi(e) == 1;
		if (const char* e = getenv("GC_EXT_LAZY")) s.extLazy = !(atoi(e) == 0);
		if (const char* e = getenv("GC_EXTEND_SLAB")) s.extendSlab = atoi(e) == 1;
		if (const char* e = getenv("GC_HOST_STITCH")) s.hostStitch = atoi(e) != 0;
		if (const char* e = getenv("GC_STITCH_CLASS")) s.stitchClass = atoi(e) == 3 ? 3 : 0;
		if (const char* e = getenv("GC_CHAIN_PLAIN_SCAN")) s.chainPlainScan = atoi(e) == 1;
		if (const char* e = getenv("GC_ED_FIRST_K")) s.edFirstK = (uint32_t)std::max(1, atoi(e));
		if (const char* e = getenv("GC_SEEDER_BUILD")) s.seederBuildOnHost = !strcmp(e, "host");
		if (const char* e = getenv("GC_BUILD_REFERENCE_CONTAINERS")) s.buildReferenceContainers = atoi(e) == 1;

		if (const char* e = getenv("GC_TEST_EXT_MAX_ITEMS")) s.testExtMaxItems = atoll(e);
		if (const char* e = getenv("GC_TEST_EXT_MAX_PENDING")) s.testExtMaxPending = atoll(e);
		if (const char* e = getenv("GC_TEST_EXT_MAX_TRACE")) s.testExtMaxTrace = atoll(e);
		if (const char* e = getenv("GC_TEST_EXT_RETRY_MAX_ITEMS")) s.testExtRetryMaxItems = (uint32_t)std::max(8, atoi(e));
		if (const char* e = getenv("GC_TEST_LONG_MAX_ITEMS")) s.testLongMaxItems = atoll(e);
		if (const char* e = getenv("GC_TEST_LONG_MAX_COLS")) s.testLongMaxCols = atoll(e);
		if (const char* e = getenv("GC_TEST_LONG_CELLS_PER_BASE")) s.testLongCellsPerBase = atoll(e);
		if (const char* e = getenv("GC_TEST_LONG_MAX_ALIGNMENTS")) s.testLongMaxAlignments = (uint32_t)std::max(1, std::min(1 << 16, atoi(e)));
		if (const char* e = getenv("GC_TEST_LONG_SCRATCH_GB")) s.testLongScratchGb = (uint64_t)std::max(1, atoi(e));
		if (const char* e = getenv("GC_TEST_STITCH_SET_MAX")) s.testStitchSetMax = atoll(e);
		if (const char* e = getenv("GC_TEST_STITCH_BFS_CAP")) s.testStitchBfsCap = atoll(e);
		if (const char* e = getenv("GC_TEST_SEED_FILTER_BITS")) s.testSeedFilterBits = (uint32_t)std::max(10, std::min(30, atoi(e)));
		if (const char* e = getenv("GC_TEST_FAIL_LONG")) s.testFailLong = atol(e);
		s.testLongForceFallback = getenv("GC_TEST_LONG_FORCE_FALLBACK") != nullptr;
		if (const char* e = getenv("GC_TEST_LONG_REG_CAP")) s.testLongRegCap = (uint32_t)std::max(1, std::min(64, atoi(e)));
		if (const char* e = getenv("GC_TEST_LONG_MAX_BLOCKS")) s.testLongMaxBlocks = (uint32_t)std::max(1, atoi(e));
		if (const char* e = getenv("GC_TEST_LONG_TEAM")) { int v = atoi(e); if (v == 1 || v == 2 || v == 4 || v == 8 || v == 16 || v == 32 || v == 64) s.testLongTeam = (uint32_t)v; }
		if (const char* e = getenv("GC_TEST_LONG_ORDER")) s.testLongOrder = (uint32_t)atoi(e);
		if (const char* e = getenv("GC_TEST_LONG_SPECULATE")) s.testLongSpeculate = (uint32_t)std::min(2, std::max(1, atoi(e)));
		s.testChainForceScratch = getenv("GC_TEST_CHAIN_FORCE_SCRATCH") != nullptr;
		if (const char* e = getenv("GC_TEST_POOL_FIRST_GUESS")) s.testPoolFirstGuess = std::max(0.0, atof(e));
		if (const char* e = getenv("GC_TEST_POOL_SHRINK_FLOOR")) s.testPoolShrinkFloor = (size_t)std::max(0ll, atoll(e));
		s.testResultCachePoison = getenv("GC_TEST_RESULT_CACHE_POISON") != nullptr;
		if (const char* e = getenv("GC_TEST_UPLOAD_SLICE")) s.testUploadSlice = (size_t)std::max(1, atoi(e));
		if (const char* e = seedfileSwitch("GC_TEST_SEEDFILE_PIECE")) s.testSeedfilePiece = (size_t)std::max(1ll, atoll(e));
		if (const char* e = seedfileSwitch("GC_TEST_SEEDFILE_HASH_BITS")) s.testSeedfileHashBits = (uint32_t)std::max(1, std::min(64, atoi(e)));
		return s;
	}
};

// the first snapshot of the process, for what is decided once per process
inline const Switches& processSwitches() { static const Switches s = Switches::fromEnvironment(); return s; }

} // namespace gc
