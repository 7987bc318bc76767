// Shared by the translation units of the library's host side (capi/gc_capi_*.hip - the C entry points, one file per subject - and gc_batch.hip - gc_align_batch and the batch
// pipeline; one 3 500-line file until r4): error reporting, device / pinned buffers, the whole-read tokens and the device's shared scratch, the worker pool, the block caches, the
// opaque handle types of the C ABI, graph upload, the edit-distance launcher. Everything here has ONE definition in the library (inline functions and variables).
#pragma once
// C ABI of the MI355X GraphChainer hot path (include/graphchainer_amd.h) and the batched host pipeline that
// drives the HIP kernels. No CPU fallback: every entry point that needs the device fails with GC_ERR_DEVICE
// when HIP is unavailable.
#include "../../include/graphchainer_amd.h"
#include "hip/gc_kernels.hpp"
#include "host/gc_graph.hpp"
#include "host/gc_hashorder.hpp"
#include "host/gc_evalue.hpp"
#include "host/gc_output.hpp"
#include "host/gc_index_cache.hpp"
#include "host/gc_correctness.hpp"
#include "host/gc_selection.hpp"
#include "host/gc_switches.hpp"
#include "host/gc_mxm_build.hpp"
#include "host/gc_mxm_cache.hpp"
#include "host/gc_layout.hpp"
#include "host/gc_long_policy.hpp"
#include "host/gc_output_plan.hpp"
#include "hip/gc_mxm_core.hpp"
#include "hip/gc_seedfile_core.hpp"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_set>
#include <vector>

using namespace gcdev;

inline thread_local std::string g_lastError;
inline int fail(int code, const std::string& msg) { g_lastError = msg; return code; }

struct DeviceError : std::runtime_error { using std::runtime_error::runtime_error; };
#define HIP_CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) throw DeviceError(std::string("HIP error: ") + hipGetErrorString(e_) + " at " #expr); } while (0)

// HIP maps its streams onto GPU_MAX_HW_QUEUES hardware queues (4 by default), and kernels of different streams that share a hardware queue
// run one after the other. A batch in flight uses a dozen streams (fragment pipeline, whole-read rounds, edit-distance classes), two batches
// twice that: on 4 queues the whole-read pass's rounds wait behind the other batch's k_extend / k_chain / k_stitch (kernel trace: 60 ms of
// foreign kernels between two rounds). 16 queues: 228 -> 209 ms per batch on cfg2; 32 oversubscribe the command processor (290 ms).
// The HIP runtime reads the variable at its first call and it configures the whole process, so it is the HOST's to set (bench.py and the
// scripts set GPU_MAX_HW_QUEUES=16 before anything touches HIP - unless the host has preset it: a box that presets 4 keeps 4); the library only says so, once, when a
// second stream is created without it.
// The whole-read pass's critical path does not count on the setting. Dispatches of streams that share a hardware queue run in submission order, one after the other, so
// whatever the other batches' streams put on the pass's queue while it ran executed inside it (profiles/passgap_timeline_parent.txt: 20 ms per pass on 4 queues, in front
// of the round's extension, while the host fetched its work count). Queueing the rounds ahead of the count only moved those dispatches. The remedy is a
// queue nobody shares: the rounds of every gc_stream run on the one stream of the token slot, created at the highest stream priority (RoundStream below).
inline void noteHardwareQueues(int streamsAlive)
{
	static std::atomic<bool> said { false };
	const char* e = getenv("GPU_MAX_HW_QUEUES");
	if (streamsAlive >= 2 && (!e || atoi(e) < 8) && !said.exchange(true))
		fprintf(stderr, "[graphchainer_amd] note: GPU_MAX_HW_QUEUES is %s; with several gc_streams per device set it to 16 before the process's first HIP call (INTEGRATION.md §7), or batches in flight serialise on HIP's 4 default hardware queues\n", e ? e : "unset");
}

namespace gcrt {

template <typename T>
T* uploadVector(const std::vector<T>& v)
{
	T* d = nullptr;
	size_t bytes = std::max<size_t>(v.size(), 1) * sizeof(T);
	HIP_CHECK(hipMalloc((void**)&d, bytes));
	if (!v.empty()) HIP_CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
	return d;
}

struct DeviceBuffer {   // growable device allocation owned by a stream object
	void* ptr = nullptr;
	size_t bytes = 0;
	template <typename T> T* reserve(size_t count, bool tight = false)   // tight: no head room (the pools that are sized by use bring their own slack)
	{
		size_t need = std::max<size_t>(count, 1) * sizeof(T);
		if (need > bytes) {
			if (ptr) HIP_CHECK(hipFree(ptr));
			ptr = nullptr;
			bytes = 0;
			size_t want = tight ? need + 256 : need + need / 8 + 256;
			HIP_CHECK(hipMalloc(&ptr, want));
			bytes = want;
		}
		return (T*)ptr;
	}
	// grows to count elements in a new block, the first usedCount elements copied over on `stream` (awaited before the old block goes); the pointer changes
	template <typename T> T* growKeeping(size_t count, size_t usedCount, hipStream_t stream, bool tight = false);
	void release() { if (ptr) (void)hipFree(ptr); ptr = nullptr; bytes = 0; }
	// a pool that a rerun sized from an overshooting request count comes back to what its batches use: called once, by the batch after the rerun (hipFree drains the device)
	void shrinkTo(size_t needBytes, size_t floor)   // (floor: 64 MB; GC_TEST_POOL_SHRINK_FLOOR lets small pools shrink too)
	{
		if (bytes > needBytes + needBytes / 4 + floor) release();
	}
	~DeviceBuffer() { if (ptr) (void)hipFree(ptr); }
};

// One whole-read pass at a time per device: its rounds saturate the scalar issue ports of the whole chip, so two passes side by side
// (two batches in flight on two gc_streams) only take turns at a finer grain and both finish late. With the token the second batch's
// seeding, seed glue and fragment pipeline overlap the first batch's whole-read pass, and its own pass starts the moment the first
// one ends - a software pipeline over batches (GC_LONG_TOKEN=0 turns it off).
// r4 / r5: two tokens per device, each with a scratch of its own, for passes that cannot fill the chip (longTokenCount, host/gc_long_policy.hpp)
using gc::LONG_TOKENS_MAX;
struct PassTokens {
	std::mutex m;
	std::condition_variable cv;
	bool busy[LONG_TOKENS_MAX] = { false, false };
	bool exclusive = false;       // slot 0 is held by a pass that fills the chip: nobody beside it
	int exclusiveWaiting = 0;     // such passes waiting (sharers let them go first: a stream of small batches must not starve a large one)
	// n: the slots the pass may take (1 or 2). alone: the pass fills the chip and runs with NO other pass beside it (r5 decided the count per batch but a count of 1 only
	// restricted the caller's choice of slot, so a large batch could run beside a small one holding slot 1 - ADVICE r5); a sharer never starts beside such a pass
	int acquire(int n, bool alone)
	{
		std::unique_lock<std::mutex> l(m);
		if (alone) {
			exclusiveWaiting++;
			cv.wait(l, [&]() { for (int s = 0; s < LONG_TOKENS_MAX; s++) if (busy[s]) return false; return true; });
			exclusiveWaiting--;
			busy[0] = true; exclusive = true;
			return 0;
		}
		int slot = -1;
		cv.wait(l, [&]() { if (exclusive || exclusiveWaiting > 0) return false; for (int s = 0; s < n; s++) if (!busy[s]) { slot = s; return true; } return false; });
		busy[slot] = true;
		return slot;
	}
	void release(int slot) { { std::lock_guard<std::mutex> l(m); busy[slot] = false; if (slot == 0) exclusive = false; } cv.notify_all(); }
};
inline PassTokens g_longPassToken[16];
// what std::unique_lock was for the single token: released when the holder goes out of scope
struct TokenHold {
	PassTokens* tokens = nullptr;
	int slot = -1;
	void lock(PassTokens& t, int n, bool alone) { tokens = &t; slot = t.acquire(n, alone); }
	bool owns_lock() const { return slot >= 0; }
	void unlock() { if (slot >= 0) { tokens->release(slot); slot = -1; } }
	~TokenHold() { unlock(); }
};
// (how many passes may run side by side is decided per batch: longTokenCount, host/gc_long_policy.hpp)
using gc::longTokenCount;
// The pass's extension scratch (up to 48 GB: one region per resident wave) is only touched while the token is held, so the gc_streams of a device share ONE
// (r3: 85 -> 37 GB per stream for 10 k x 10 kb batches, which is what lets five batches be in flight on a 288 GB device instead of three). It belongs to the
// token: reserved (grown) by the pass that holds it, freed when the device's last gc_stream goes.
// The round loop's stream belongs to the token as well: one pass per token slot runs its rounds at a time, so the slot has ONE stream (and event ring) that every pass
// holding it uses in turn - not one per gc_stream, four of which sat idle among five batches' sixty-odd streams. Created by the slot's first pass, destroyed with the scratch.
// GC_LONG_TOKEN=0 (no token, passes overlap) keeps one per gc_stream (gc_stream::ownRounds).
inline constexpr int LONG_EVENT_RING = 8;
struct RoundStream {
	hipStream_t q = nullptr;
	hipEvent_t ring[2 * LONG_EVENT_RING] {};   // (begin, end) pairs around the rounds' extension launches
	// ofToken: the slot's stream is created at the device's highest stream priority. HIP keeps the hardware queues of each priority apart, so the pass's rounds - the step's
	// critical path, one pass per slot at a time - get a queue that the dozens of default-priority streams of the batches in flight do not share, however few queues the host
	// was granted (GPU_MAX_HW_QUEUES); on a shared queue every foreign dispatch submitted during the pass ran inside it, one after the other. That HIP does so is what the
	// kernel traces show, not a documented promise: in profiles/passgap_timeline.txt every dispatch of the token's stream is on queue id 5, which no other stream's dispatch uses.
	// r3 tried priorities on the five per-stream round streams and lost; this is one stream, used only while the token is held. Without a token: default priority.
	void ensure(bool ofToken)
	{
		if (q) return;
		for (auto& e : ring) if (!e) HIP_CHECK(hipEventCreate(&e));
		int least = 0, greatest = 0;
		if (ofToken) HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
		if (ofToken && greatest != least) HIP_CHECK(hipStreamCreateWithPriority(&q, hipStreamNonBlocking, greatest));
		else HIP_CHECK(hipStreamCreateWithFlags(&q, hipStreamNonBlocking));
	}
	void release()
	{
		for (auto& e : ring) { if (e) (void)hipEventDestroy(e); e = nullptr; }
		if (q) (void)hipStreamDestroy(q);
		q = nullptr;
	}
};
struct SharedLongScratch { DeviceBuffer buffer[LONG_TOKENS_MAX]; RoundStream rounds[LONG_TOKENS_MAX]; int streams = 0; };
inline SharedLongScratch g_longScratch[16];
inline std::mutex g_longScratchCount;

inline double nowUs() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// CPU time of the whole process (all threads), for GC_DEBUG_TIMES' host budget lines
inline double threadCpuMs() { timespec ts {}; clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec / 1e6; }
inline double processCpuMs() { timespec ts {}; clock_gettime(CLOCK_PROCESS_CPUTIME_ID, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec / 1e6; }

// Waiting for a stream. hipStreamSynchronize spins on a CPU, and a batch has two host threads waiting most of its 200 ms (two batches in
// flight: four CPUs' worth of spinning, half of what a batch costs the host). Modes (GC_SPIN_SYNC): 2 (default) polls hipStreamQuery and
// sleeps 40 us between polls - the waits are tens of microseconds late and cost next to no CPU; 1 spins (the r2 behaviour); 0 sleeps on a
// hipEventBlockingSync event (interrupt-driven; measured slower than spinning on this pool's boxes: 255 against 237 ms per batch).
inline void syncStream(hipStream_t q)
{
	const int mode = gc::processSwitches().spinSync;
	if (mode == 1) { HIP_CHECK(hipStreamSynchronize(q)); return; }
	if (mode == 2) {
		// r5: the sleep between polls backs off from 40 us (GC_SYNC_POLL_US) to four times that once a wait has lasted a millisecond: a batch's threads wait ~1 s in all per 150 ms
		// step, mostly for kernels of tens of milliseconds, and every poll is a runtime call and a nanosleep
		const int pollUs = gc::processSwitches().syncPollUs;
		int sleepUs = pollUs;
		for (int spins = 0;; spins++) {
			const hipError_t e = hipStreamQuery(q);
			if (e == hipSuccess) return;
			if (e != hipErrorNotReady) HIP_CHECK(e);
			if (spins >= 4) {   // (the first few polls back to back: many waits are for kernels of a few microseconds)
				std::this_thread::sleep_for(std::chrono::microseconds(sleepUs));
				if (spins >= 12 && sleepUs < 4 * pollUs) sleepUs += sleepUs / 4 + 1;
			}
		}
	}
	// one blocking-sync event per device this thread has waited on, destroyed with the thread (the whole-read pass threads live for one batch)
	struct Events { hipEvent_t e[16] = {}; ~Events() { for (auto& x : e) if (x) (void)hipEventDestroy(x); } };
	static thread_local Events events;
	int device = 0;
	HIP_CHECK(hipGetDevice(&device));
	hipEvent_t& e = events.e[device & 15];
	if (!e) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventBlockingSync | hipEventDisableTiming));
	HIP_CHECK(hipEventRecord(e, q));
	HIP_CHECK(hipEventSynchronize(e));
}

// The same for one event (the round token of the whole-read pass is released the moment its extension kernel has finished).
inline void syncEvent(hipEvent_t ev)
{
	const int pollUs = gc::processSwitches().syncPollUs;
	int sleepUs = pollUs;
	for (int spins = 0;; spins++) {
		const hipError_t e = hipEventQuery(ev);
		if (e == hipSuccess) return;
		if (e != hipErrorNotReady) HIP_CHECK(e);
		if (spins >= 4) {
			std::this_thread::sleep_for(std::chrono::microseconds(sleepUs));
			if (spins >= 12 && sleepUs < 4 * pollUs) sleepUs += sleepUs / 4 + 1;
		}
	}
}

template <typename T> T* DeviceBuffer::growKeeping(size_t count, size_t usedCount, hipStream_t stream, bool tight)
{
	DeviceBuffer larger;
	T* dLarger = larger.reserve<T>(count, tight);
	if (usedCount) HIP_CHECK(hipMemcpyAsync(dLarger, ptr, usedCount * sizeof(T), hipMemcpyDeviceToDevice, stream));
	syncStream(stream);
	std::swap(ptr, larger.ptr); std::swap(bytes, larger.bytes);
	return dLarger;
}

// Persistent worker pool for the per-read host work between the kernels: bookkeeping, selection, host stitching, result assembly (threads are created once per process).
class WorkerPool {
public:
	static WorkerPool& instance() { static WorkerPool p(0); return p; }
	// r5: the batch pipeline's own, smaller pool. Its jobs became short (the seed glue, the stitching and the anchor arrays are kernels now: what is left is a few ms of per-read
	// bookkeeping and memcpy per stage), and a job wakes every thread of its pool: with 32 workers a batch cost 0.29 CPU-seconds, with 8 0.185 at the same rate (`gpurun_out/r5_hostcpu`).
	// The output encoders (GAF text, zlib) keep the wide pool.
	static WorkerPool& batch() { static WorkerPool p(1); return p; }
	size_t size() const { return workers.size() + 1; }
	// runs body(i, worker) for i in [0, n); worker in [0, size())
	void run(size_t n, const std::function<void(size_t, size_t)>& body)
	{
		if (n == 0) return;
		if (workers.empty() || n < 4) { for (size_t i = 0; i < n; i++) body(i, 0); return; }
		std::lock_guard<std::mutex> oneJob(runMutex);   // batches in flight on different gc_streams take turns on the pool
		{
			std::unique_lock<std::mutex> lock(mutex);
			job = &body;
			total = n;
			next.store(0);
			pending = workers.size();
			failure = nullptr;
			generation++;
		}
		wake.notify_all();
		work(0);
		std::unique_lock<std::mutex> lock(mutex);
		done.wait(lock, [&]() { return pending == 0; });
		job = nullptr;
		if (failure) { std::exception_ptr e = failure; failure = nullptr; std::rethrow_exception(e); }   // (an exception in a pool thread used to end the process)
	}
private:
	explicit WorkerPool(int kind)
	{
		size_t n = std::max(1u, std::thread::hardware_concurrency());
		n = std::min<size_t>(n, 96);   // the glue is memory-bound; more threads stop helping
		// A container with a CPU bandwidth quota (cgroup cpu.max) shows all of the machine's threads but is throttled for the rest of the
		// 100 ms period once a burst of workers has spent the quota - measured on a 16-CPU quota: 96 workers finish a stage in 10 ms and the
		// whole process (the whole-read pass's round loop included) then stalls for 50-60 ms. Twice the quota keeps the bursts inside it.
		const double quota = gc::cpuQuota();
		if (quota > 0) n = std::min<size_t>(n, std::max<size_t>(4, (size_t)(2 * quota + 0.5)));
		if (gc::processSwitches().hostThreads) n = *gc::processSwitches().hostThreads;
		if (kind == 1) {
			n = std::min<size_t>(n, quota > 0 ? std::max<size_t>(4, (size_t)(quota / 2 + 0.5)) : 8);
			if (gc::processSwitches().batchThreads) n = *gc::processSwitches().batchThreads;
		}
		for (size_t t = 1; t < n; t++) workers.emplace_back([this, t]() { loop(t); });
	}
	~WorkerPool()
	{
		{ std::unique_lock<std::mutex> lock(mutex); stop = true; generation++; }
		wake.notify_all();
		for (auto& w : workers) w.join();
	}
	void work(size_t id)
	{
		const size_t chunk = 4;
		const bool account = gc::processSwitches().debugTimes;
		const double cpu0 = account ? threadCpuMs() : 0;
		try {
			for (size_t i; (i = next.fetch_add(chunk)) < total;)
				for (size_t k = i; k < std::min(total, i + chunk); k++) (*job)(k, id);
			if (account) cpuUs.fetch_add((uint64_t)((threadCpuMs() - cpu0) * 1e3));
		} catch (...) {
			next.store(total);   // the first failure ends the job: the other threads stop fetching, the caller rethrows
			std::unique_lock<std::mutex> lock(mutex);
			if (!failure) failure = std::current_exception();
		}
	}
	void loop(size_t id)
	{
		size_t seen = 0;
		while (true) {
			{
				std::unique_lock<std::mutex> lock(mutex);
				wake.wait(lock, [&]() { return generation != seen; });
				seen = generation;
				if (stop) return;
			}
			work(id);
			std::unique_lock<std::mutex> lock(mutex);
			if (--pending == 0) done.notify_one();
		}
	}
	std::vector<std::thread> workers;
	std::mutex mutex, runMutex;
	std::condition_variable wake, done;
	const std::function<void(size_t, size_t)>* job = nullptr;
	std::atomic<size_t> next { 0 };
public:
	std::atomic<uint64_t> cpuUs { 0 };   // GC_DEBUG_TIMES: CPU time spent inside jobs by all threads (what a stage costs beside its own thread)
private:
	size_t total = 0, pending = 0, generation = 0;
	std::exception_ptr failure;
	bool stop = false;
};

struct PinnedBuffer {   // growable page-locked host staging buffer (full-rate PCIe copies)
	void* ptr = nullptr;
	size_t bytes = 0;
	template <typename T> T* reserve(size_t count)
	{
		size_t need = std::max<size_t>(count, 1) * sizeof(T);
		if (need > bytes) {
			if (ptr) HIP_CHECK(hipHostFree(ptr));
			ptr = nullptr;
			bytes = 0;
			size_t want = need + need / 8 + 4096;
			HIP_CHECK(hipHostMalloc(&ptr, want, hipHostMallocDefault));
			bytes = want;
		}
		return (T*)ptr;
	}
	~PinnedBuffer() { if (ptr) (void)hipHostFree(ptr); }
};

template <typename T> inline T* mallocArray(size_t n) { return (T*)malloc(std::max<size_t>(n, 1) * sizeof(T)); }

// The arrays of a gc_result. The big ones (the trace arrays of keep_traces: 0.1-0.5 GB each for 10 k x 10 kb reads) come from a small cache of blocks that
// gc_result_free gives back: fresh memory of that size is mapped and zero-filled page by page on first touch, every batch again (r3: ~1.5 of the 3.4 CPU-seconds the
// assembly of a traced batch cost). Every array carries a 64-byte header with its size, so gc_result_free knows what it holds.
struct ResultBlockCache {
	static constexpr size_t HEADER = 64, MAX_HELD = 24ull << 30;
	// test hooks: GC_RESULT_CACHE_MIN=bytes recycles arrays from that size on (default 32 MB), GC_TEST_RESULT_CACHE_POISON=1 fills every array with 0xA5 when it is handed out -
	// together they show any reader that counts on an array's unwritten part being zero (fresh pages are, recycled ones are not)
	const size_t BIG = gc::processSwitches().resultCacheMin;
	const bool poison = gc::processSwitches().testResultCachePoison;
	std::mutex mutex;
	std::vector<std::pair<char*, size_t>> blocks;   // (base, capacity in bytes without the header)
	size_t held = 0;
	void* get(size_t bytes)
	{
		if (bytes >= BIG) {
			std::lock_guard<std::mutex> lock(mutex);
			size_t best = blocks.size();
			for (size_t i = 0; i < blocks.size(); i++)
				if (blocks[i].second >= bytes && blocks[i].second <= 2 * bytes && (best == blocks.size() || blocks[i].second < blocks[best].second)) best = i;
			if (best < blocks.size()) {
				char* base = blocks[best].first;
				held -= blocks[best].second;
				const size_t capacityHeld = blocks[best].second;
				blocks.erase(blocks.begin() + (long)best);
				if (poison) memset(base + HEADER, 0xA5, capacityHeld);
				return base + HEADER;
			}
		}
		const size_t capacity = bytes >= BIG ? bytes + bytes / 16 : bytes;   // (a little slack: the next batch's arrays are about, not exactly, this size)
		char* base = (char*)malloc(capacity + HEADER);
		if (!base) throw std::bad_alloc();
		*(size_t*)base = capacity;
		if (poison) memset(base + HEADER, 0xA5, capacity);
		return base + HEADER;
	}
	void put(void* p)
	{
		if (!p) return;
		char* base = (char*)p - HEADER;
		const size_t capacity = *(size_t*)base;
		if (capacity >= BIG) {
			std::lock_guard<std::mutex> lock(mutex);
			if (held + capacity <= MAX_HELD && blocks.size() < 64) { blocks.emplace_back(base, capacity); held += capacity; return; }
		}
		free(base);
	}
	void trim()   // gives every held block back to the allocator (gc_result_cache_trim)
	{
		std::lock_guard<std::mutex> lock(mutex);
		for (auto& b : blocks) free(b.first);
		blocks.clear();
		held = 0;
	}
};
// deliberately never destroyed: a language runtime's finalizers may still call gc_result_free while the process's static destructors run
inline ResultBlockCache& g_resultBlocks = *new ResultBlockCache();
template <typename T> inline T* resultArray(size_t n) { return (T*)g_resultBlocks.get(std::max<size_t>(n, 1) * sizeof(T)); }

} // namespace gcrt
using namespace gcrt;

// ----------------------------------------------------------------------------------------------------
struct gc_graph {
	gc::AlignmentGraph host;
	bool hostMpcTrimmed = false;   // gc_graph_trim_host: host.mpc / paths / backwards / topo / topo_ids / component_ids are empty
	// dense-by-bigraph-node-id copies of the twin lookup tables (the same arrays the device gets): original node size, and the
	// split nodes of every bigraph node in offset order (chunk k covers offsets [64k, 64k+64))
	std::vector<uint32_t> hOrigSize, hLookupOff, hLookup;
	// reverse-strand twin of (split node, offset): GetReversePosition + GetUnitigNode (src/AlignmentGraph.cpp:832-868) without the hash maps
	inline void twinOf(uint32_t node, uint32_t offset, uint32_t& twinNode, uint32_t& twinOffset) const
	{
		uint32_t id = (uint32_t)host.nodeIDs[node];
		uint32_t rev = hOrigSize[id] - 1 - ((uint32_t)host.nodeOffset[node] + offset);
		twinNode = hLookup[hLookupOff[id ^ 1] + rev / 64];
		twinOffset = rev - (uint32_t)host.nodeOffset[twinNode];
	}
	DGraph dev {};
	OutNames devNames {};            // GFA segment names by bigraph node id (output encoding on the device, gc_output.hip)
	std::vector<void*> allocations;
	CorrectnessTables* devTables = nullptr;
	uint8_t* devIupac = nullptr;
	uint32_t maxMpcWidth = 0, maxPathsPerNode = 1, maxBackPerNode = 1;
	~gc_graph() { for (void* p : allocations) (void)hipFree(p); }
	template <typename T> const T* up(const std::vector<T>& v) { T* d = uploadVector(v); allocations.push_back(d); return d; }
};

struct gc_seeder {
	gc::MinimizerIndex host;
	SeedIndex dev {};
	std::vector<void*> allocations;
	~gc_seeder() { for (void* p : allocations) (void)hipFree(p); }
};

// Device and pinned blocks of read batches, kept for the next batch (r4). gc_reads_upload used to hipMalloc nine arrays per batch and gc_reads_destroy to hipFree them:
// hipFree waits for the device to drain, so with five batches in flight every destroy stalled its host thread for the length of whatever was queued (and the upload of the
// next batch behind it: 245 ms per batch in the end-to-end leg, `gpurun_out/r4_ab3`). One block per batch now, carved into the arrays, returned to a small cache.
struct BlockCache {
	bool pinned;
	std::mutex mutex;
	struct Block { void* ptr; size_t bytes; int device; };
	std::vector<Block> blocks;
	static constexpr size_t MAX_BLOCKS = 12;
	size_t maxBytes;          // r5: the cache holds back at most this many bytes in all (a block that would exceed it is freed instead)
	size_t heldBytes = 0;
	explicit BlockCache(bool pinned, size_t maxBytes = (size_t)24 << 30) : pinned(pinned), maxBytes(maxBytes) {}
	void* get(size_t bytes, int device, size_t& capacity)
	{
		{
			std::lock_guard<std::mutex> lock(mutex);
			size_t best = blocks.size();
			for (size_t i = 0; i < blocks.size(); i++)
				if (blocks[i].device == device && blocks[i].bytes >= bytes && blocks[i].bytes <= 2 * bytes + (1u << 20) && (best == blocks.size() || blocks[i].bytes < blocks[best].bytes)) best = i;
			if (best < blocks.size()) { Block b = blocks[best]; blocks.erase(blocks.begin() + (long)best); heldBytes -= b.bytes; capacity = b.bytes; return b.ptr; }
		}
		capacity = bytes + bytes / 8 + 4096;   // (a little slack: the next batch is about, not exactly, this size)
		void* p = nullptr;
		if (pinned) HIP_CHECK(hipHostMalloc(&p, capacity, hipHostMallocDefault));
		else HIP_CHECK(hipMalloc(&p, capacity));
		return p;
	}
	void put(void* p, size_t bytes, int device)
	{
		if (!p) return;
		{
			std::lock_guard<std::mutex> lock(mutex);
			if (blocks.size() < MAX_BLOCKS && heldBytes + bytes <= maxBytes) { blocks.push_back(Block { p, bytes, device }); heldBytes += bytes; return; }
		}
		if (pinned) (void)hipHostFree(p); else (void)hipFree(p);
	}
	void trim()   // gives everything held back to the allocator (gc_result_cache_trim)
	{
		std::vector<Block> mine;
		{ std::lock_guard<std::mutex> lock(mutex); mine.swap(blocks); heldBytes = 0; }
		for (const Block& b : mine) { if (pinned) (void)hipHostFree(b.ptr); else (void)hipFree(b.ptr); }
	}
};
inline BlockCache& g_readDeviceBlocks = *new BlockCache(false);   // (leaked on purpose, like the result cache: finalizers may run late)
inline BlockCache& g_readPinnedBlocks = *new BlockCache(true);
// r5: the GAM deflate's staging (a batch's inflated groups plus the output bound: hundreds of MB) has caches of its own - in the read batches' caches its other
// size class evicted read blocks, and an evicted block is a hipFree / hipHostFree: the device-wide stall the caches exist to avoid
inline BlockCache& g_deflateDeviceBlocks = *new BlockCache(false, (size_t)4 << 30);
inline BlockCache& g_deflatePinnedBlocks = *new BlockCache(true, (size_t)4 << 30);

// a stream of the calling thread's own for its uploads and small jobs (created on first use, recreated when the thread changes device)
inline hipStream_t threadStream(int device)
{
	static thread_local struct ThreadStream { hipStream_t q = nullptr; int device = -1; ~ThreadStream() { if (q) (void)hipStreamDestroy(q); } } ts;
	if (!ts.q || ts.device != device) { if (ts.q) (void)hipStreamDestroy(ts.q); ts.q = nullptr; HIP_CHECK(hipStreamCreateWithFlags(&ts.q, hipStreamNonBlocking)); ts.device = device; }
	return ts.q;
}

// A cache's block for the length of a call. It goes back to its cache only after the stream has drained: after an exception between a launch and the call's own wait the
// block would otherwise be handed to the next caller while this call's copies and kernels still use it. release() hands the block on to an owner that outlives
// the call (a read batch that was built without a failure).
struct HeldBlock {
	BlockCache& cache; int device; hipStream_t q;
	void* p = nullptr; size_t bytes = 0;
	HeldBlock(BlockCache& cache, int device, hipStream_t q) : cache(cache), device(device), q(q) {}
	HeldBlock(const HeldBlock&) = delete;
	void* acquire(size_t want) { p = cache.get(want, device, bytes); return p; }
	void* release() { void* mine = p; p = nullptr; return mine; }
	~HeldBlock() { if (p) { (void)hipStreamSynchronize(q); cache.put(p, bytes, device); } }
};

// N timing events for the length of a call
template <int N> struct EventSet {
	hipEvent_t e[N] {};
	EventSet() { for (auto& x : e) { const hipError_t err = hipEventCreate(&x); if (err != hipSuccess) { destroy(); HIP_CHECK(err); } } }
	EventSet(const EventSet&) = delete;
	~EventSet() { destroy(); }
	hipEvent_t operator[](int i) const { return e[i]; }
	float elapsedMs(int i, int j) const { float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, e[i], e[j])); return ms; }   // (after a synchronize behind both)
private:
	void destroy() { for (auto& x : e) if (x) { (void)hipEventDestroy(x); x = nullptr; } }
};

struct gc_reads {
	void* deviceBlock = nullptr; size_t deviceBlockBytes = 0; int device = 0;   // every device array below is carved from this one block
	std::vector<uint64_t> offsets;   // host copy [n+1]
	uint64_t totalBases = 0;
	std::vector<uint8_t> invalid;    // read has a character outside the IUPAC alphabet (the reference's Complement() asserts)
	char* devBases = nullptr;        // [2*totalBases]: all reads forward, then every read reverse-complemented in place
	uint64_t* devOffsets = nullptr;
	// per read: match-mask bit vectors [strand fwd/rc][A,C,G,T][words] (bit i set: read position i matches that base)
	uint64_t* devMasks = nullptr;
	std::vector<uint64_t> maskOff;   // [n] word offset of read r's masks
	std::vector<uint32_t> maskWords; // [n] words per bit vector
	const uint64_t* devMaskOff = nullptr; const uint32_t* devMaskWords = nullptr;   // the two on the device (the fragment extension kernel reads its rows' masks through them)
	const uint64_t* devEqOff = nullptr;   // [n] word offset of read r's exact-match masks (the pack kernel's)
	// exact-match bit vectors of the forward strand [A,C,G,T][words] and the per-read records of the NW kernel (rows = read bases)
	uint64_t* devEqMasks = nullptr;
	EdRead* devEdReads = nullptr;
	uint32_t* devChunkRead = nullptr;   // read containing the first base of every 64-base chunk of the concatenated forward bases
	uint64_t* devPacked = nullptr;      // the forward bases, 2 bits each, big-endian inside 64-bit words (for the seed kernel's k-mers)
	uint64_t* devInvalid = nullptr;     // one bit per forward base: not A, C, G or T (same big-endian convention)
	uint8_t* devReadInvalid = nullptr;  // [n] the device's copy of `invalid`
	~gc_reads() { g_readDeviceBlocks.put(deviceBlock, deviceBlockBytes, device); }
};
static_assert(sizeof(gc::EdReadRecord) == sizeof(EdRead) && offsetof(gc::EdReadRecord, eqOff) == offsetof(EdRead, eqOff) && offsetof(gc::EdReadRecord, len) == offsetof(EdRead, len) &&
	offsetof(gc::EdReadRecord, words) == offsetof(EdRead, words), "the layout's record is the kernels' EdRead");

// The one layout of a read batch (host/gc_layout.hpp) on a block of L.blockBytes: gc_reads_upload and the parsers build their batches through these two.
// The block stays its HeldBlock's until the call has succeeded; R.deviceBlock is set then.
inline void bindReads(gc_reads& R, const gc::ReadBatchLayout& L, void* block)
{
	char* D = (char*)block;
	R.maskOff = L.maskOff; R.maskWords = L.maskWords;
	R.devBases = D + L.oBases; R.devOffsets = (uint64_t*)(D + L.oOffsets); R.devMasks = (uint64_t*)(D + L.oMasks); R.devEqMasks = (uint64_t*)(D + L.oEqMasks); R.devEdReads = (EdRead*)(D + L.oEdReads);
	R.devPacked = (uint64_t*)(D + L.oPacked); R.devInvalid = (uint64_t*)(D + L.oInvalid); R.devChunkRead = (uint32_t*)(D + L.oChunkRead); R.devReadInvalid = (uint8_t*)(D + L.oReadInvalid);
	R.devMaskOff = (uint64_t*)(D + L.oMaskOff); R.devMaskWords = (uint32_t*)(D + L.oMaskWords); R.devEqOff = (uint64_t*)(D + L.oEqOff);
}
// the four per-read arrays through the caller's pinned staging (n elements each) to the device, behind the offsets' copy
inline void stageReadLayout(const gc_reads& R, const gc::ReadBatchLayout& L, uint64_t* hMaskOff, uint32_t* hMaskWords, uint64_t* hEqOff, EdRead* hEdReads, hipStream_t q)
{
	const size_t n = L.maskOff.size();
	if (!n) return;
	memcpy(hMaskOff, L.maskOff.data(), n * sizeof(uint64_t)); memcpy(hMaskWords, L.maskWords.data(), n * sizeof(uint32_t));
	memcpy(hEqOff, L.eqOff.data(), n * sizeof(uint64_t)); memcpy(hEdReads, L.edReads.data(), n * sizeof(EdRead));
	HIP_CHECK(hipMemcpyAsync((void*)R.devMaskOff, hMaskOff, n * sizeof(uint64_t), hipMemcpyHostToDevice, q));
	HIP_CHECK(hipMemcpyAsync((void*)R.devMaskWords, hMaskWords, n * sizeof(uint32_t), hipMemcpyHostToDevice, q));
	HIP_CHECK(hipMemcpyAsync((void*)R.devEqOff, hEqOff, n * sizeof(uint64_t), hipMemcpyHostToDevice, q));
	HIP_CHECK(hipMemcpyAsync(R.devEdReads, hEdReads, n * sizeof(EdRead), hipMemcpyHostToDevice, q));
}

// a read batch's seed hits from the host's own seeder (gc_seeds_upload), resolved by k_seed_resolve: read-only afterwards, shared by streams
struct gc_seeds {
	int device = 0;
	uint64_t nHits = 0;
	std::vector<uint64_t> readOffsets;     // the read batch's offsets [n+1]: the hits' seq_pos were checked against these lengths
	uint32_t* devReadHitOff = nullptr;     // [n+1] the caller's read_hit_off: where a read's seeds begin in every per-seed array of the batch
	SeedHitArrays dev {};                  // [nHits] each, carved from one allocation
	void* block = nullptr;
	SeedHit* devHits = nullptr;            // [nHits] the raw records in the block's tail, as uploaded or as gc_seeds_mxm wrote them (gc_seeds_hits)
	double kernelMs = 0;                   // gc_seeds_mxm: device time from the first kernel to the last
	~gc_seeds() { if (block) (void)hipFree(block); }
};
// The one layout of a seed batch (host/gc_layout.hpp): allocates H.block for H.nHits hits of nReads reads and points H's arrays into it. Returns the three words for the
// kernels' first refused hit (resolve, match_len, raw_goodness), not yet set.
inline unsigned long long* allocateSeedBlock(gc_seeds& H, uint64_t nReads)
{
	const gc::SeedBatchLayout L(nReads, H.nHits);
	HIP_CHECK(hipMalloc(&H.block, L.blockBytes));
	char* D = (char*)H.block;
	H.devReadHitOff = (uint32_t*)(D + L.oOff);
	uint32_t* arrays = (uint32_t*)(D + L.oArrays);
	H.dev = SeedHitArrays { arrays, arrays + H.nHits, arrays + 2 * H.nHits, arrays + 3 * H.nHits, arrays + 4 * H.nHits };
	H.devHits = (SeedHit*)(D + L.oHits);
	return (unsigned long long*)(D + L.oBad);
}

// the seeds of the -s files (gc_seed_store_open), decoded and sorted by name hash in HBM: read-only, shared by streams
struct gc_seed_store {
	int device = 0;
	SfStoreView dev {};
	uint64_t messages = 0, seeds = 0, distinct = 0, deviceBytes = 0;
	double inflateMs = 0, frameMs = 0, uploadMs = 0, decodeMs = 0, sortMs = 0;
	std::vector<void*> allocations;
	~gc_seed_store() { for (void* p : allocations) (void)hipFree(p); }
};

// the MUM / MEM index of a graph's forward segments (gc_mxm_index_create): suffix array, packed text, segment table and prefix table in HBM; read-only, shared by streams
struct gc_mxm_index {
	const gc_graph* graph = nullptr;       // the graph it was built from: gc_seeds_mxm refuses another
	int device = 0;
	std::vector<uint32_t> nodeStart;       // host copies of the two small tables
	std::vector<int32_t> nodeId;
	MxmIndexView dev {};
	uint64_t deviceBytes = 0;
	double buildSeconds = 0;               // text and suffix array: built on the host or the device, or read from the cache file and verified
	double saSeconds = 0;                  // of buildSeconds, the suffix array alone (0 when loaded)
	int buildMode = 0;                     // 0 host build, 1 device build, 2 loaded from the cache (gc_mxm_index_open)
	uint32_t buildRounds = 0;              // doubling rounds after the first sort (0 when loaded)
	uint64_t buildScratchBytes = 0;        // what a device build allocated beside the SA, freed again
	double cacheSaveSeconds = 0;           // writing <prefix>.gcmxm after a build (0: nothing written)
	std::vector<void*> allocations;
	~gc_mxm_index() { for (void* p : allocations) (void)hipFree(p); }
};

struct StitchedPath { std::vector<uint32_t> nodes; uint32_t firstOffset = 0, lastOffset = 0; uint64_t cells = 0; };

struct ReadGlue {
	std::vector<LongAln> longAlns;        // final order (the reference's repeated sort by alignmentStart)
	uint64_t longBegin = 0, longTraceBegin = 0, longSeedBegin = 0;
	bool failed = false;
	bool longFailed = false;              // the whole-read pass asserted: no anchors, chain or alignment for this read
	bool capacityExceeded = false;        // a capacity of this library (not of the reference) was exceeded while processing this read
	bool capacityExceededLong = false;    // same, raised by the whole-read pass (its own thread; joined into capacityExceeded after the pass)
	uint64_t slotBegin = 0, fragBegin = 0;
	uint32_t nSeedsR = 0, nWindows = 0;   // seeds of the read (fragment order, at seedBegin) and fragments that hold seeds
	uint64_t nAnchors = 0, nPath = 0, nTrace = 0, anchorBegin = 0, pathBegin = 0, traceBegin = 0, seedBegin = 0, chainBegin = 0;
	StitchedPath stitched;                // chain stitching result
	bool stitchedOnDevice = false;        // its nodes are also in the device's stitch regions
	uint64_t stitchedBegin = 0;
	std::vector<uint32_t> longSelected;   // GreedyLength selection (src/Aligner.cpp:636-639): indices into longAlns
	uint64_t longSelectedBegin = 0;
	int64_t longEditDistance = -1, chainEditDistance = -1;
	// the chained alignment (src/Aligner.cpp:845-897): trace in output coordinates, alignmentStart / alignmentEnd
	std::vector<int32_t> chainTraceNode; std::vector<uint32_t> chainTraceOffset, chainTraceSeqPos; std::vector<uint8_t> chainTraceSwitch;
	uint32_t chainAlnStart = 0, chainAlnEnd = 0;
	bool hasChainAlignment = false, chainWins = false;
	uint64_t chainTraceBegin = 0;
	// back to the state of a fresh record, keeping the vectors' storage: the records live in the gc_stream and are reused by
	// every batch (allocating and destroying 10 k x 6 vectors per batch cost ~10 ms of teardown plus the allocations)
	void reset()
	{
		longAlns.clear(); longSelected.clear();
		stitched.nodes.clear(); stitched.firstOffset = stitched.lastOffset = 0; stitched.cells = 0;
		longBegin = longTraceBegin = longSeedBegin = 0;
		failed = longFailed = capacityExceeded = capacityExceededLong = false;
		slotBegin = fragBegin = 0;
		nSeedsR = nWindows = 0;
		nAnchors = nPath = nTrace = anchorBegin = pathBegin = traceBegin = seedBegin = chainBegin = 0;
		stitchedBegin = longSelectedBegin = 0;
		longEditDistance = chainEditDistance = -1;
		chainTraceNode.clear(); chainTraceOffset.clear(); chainTraceSeqPos.clear(); chainTraceSwitch.clear();
		chainAlnStart = chainAlnEnd = 0;
		hasChainAlignment = chainWins = false;
		chainTraceBegin = 0;
	}
};

struct EditDistanceRun {
	hipStream_t streams[8] {};         // one per kernel class: three pairs per wave, two pairs per wave, units of 1, 2, 4, 8, 16 blocks, a workgroup per pair (the whole matrix)
	uint32_t begin[9] {};              // the classes' ranges in the grouped order
	std::vector<uint32_t> lens;        // the pairs' read lengths, grouped order (the reruns choose their kernel by them)
	hipEvent_t ready = nullptr;
	std::vector<uint32_t> perm;        // position in the grouped order -> original pair index
	std::vector<int64_t> grouped;      // results in grouped order (pinned not needed: small)
	~EditDistanceRun() { for (auto& q : streams) if (q) (void)hipStreamDestroy(q); if (ready) (void)hipEventDestroy(ready); }
};

// Coverage accumulators (gc_coverage_*; hip/gc_coverage.hip): they live across batches, across the streams set to the handle and, merged, across devices
struct gc_coverage {
	int device = 0;
	uint32_t nIds = 0;                 // bigraph node ids of the graph it was made for
	std::vector<uint64_t> segStart;    // [segments + 1] first forward base of every segment: the graph's shape as gc_coverage_merge compares it
	CovGraph dev {};
	OutNames names {};                 // the graph's (it must outlive the handle)
	const gc_graph* graph = nullptr;
	unsigned long long* dBases = nullptr;   // [segments]
	uint32_t* dDepth = nullptr;             // [forward bases], only with per_base
	uint32_t* dBad = nullptr;               // flag word: 1 a cell outside the graph was met (and not counted), 2 the finish step's runs did not pair up, 4 a node change that is no link, 8 a GFA line of 2^32 bytes, COV_BAD_SEQPOS a cell's seqPos behind its read
	void* dSegStart = nullptr;
	bool hasLinks = false;                  // GC_COVERAGE_LINKS: the graph's links, sorted canonical keys (gc_coverage_links_core.hpp), here and on the device with a 64-bit counter each
	std::vector<uint64_t> linkKeys;
	uint64_t* dLinkKeys = nullptr;
	unsigned long long* dLinkCounts = nullptr;
	CovLinks links {};                      // (counts == nullptr without links: launchCoverageAdd then takes the kernel without the traversal step)
	uint32_t* dPile = nullptr;              // GC_COVERAGE_PILEUP: [8 * forward bases] the rows of hip/gc_pileup_core.hpp (null without the pileup: launchCoverageAdd then takes the kernel without that step)
	CovPile pileFor(const char* reads) const { return CovPile { graph->dev, graph->devIupac, reads, dPile }; }   // the kernel's view, over the resident bases the jobs' readOff point into
	~gc_coverage() { for (void* p : { (void*)dBases, (void*)dDepth, (void*)dBad, dSegStart, (void*)dLinkKeys, (void*)dLinkCounts, (void*)dPile }) if (p) (void)hipFree(p); }
};

struct gc_stream {
	std::vector<ReadGlue> glue;   // per-read host records of the batch in flight (storage reused)
	gc_coverage* coverage = nullptr;   // gc_stream_set_coverage: the batches of this stream with device_output != 0 are counted into it
	int device = 0;            // the device the stream was created on; gc_align_batch selects it for the calling thread
	hipStream_t stream = nullptr;
	hipEvent_t ev[12] {};
	hipEvent_t fragEv[16] {};   // r5: a (begin, end) pair around each of the lazy rounds' k_extend launches [0..7] and k_build_anchors launches [8..15]: kernel_us[1] / [2] are sums of exactly those
	DeviceBuffer tmp, matches, readMatchOff, readMatchCount, cursors, readSeeds, fragFirstSeed, extLists, fragItems, fragRetryList, fragClaims, pendingFrags, fragNext, roundCounts, work, results, scratch, scratchRetry, tracePool, frags, fragSeeds, anchors, fragStatus, fragExtended, readTies, pathPool, jobs, chainOut, chainLen, chainScore, chainStatus, chainScratch, counters;
	PinnedBuffer hFragDeclined, hReadSeeds, hFragFirstSeed, hFrags, hJobs, hAnchors, hFragStatus, hFragExtended, hReadTies, hChainOut, hChainLen, hChainScore, hChainStatus, hPathPool, hSmall;
	DeviceBuffer edPathNodes, edJobs, edLetters, edLettersLen, edPairs, edOut;
	PinnedBuffer hEdPathNodes, hEdJobs, hEdPairs, hEdOut;
	// The device output encoder's own: what batch/gc_output_encoder.hip (OutputEncoder) works in, kept from batch to batch. Between the whole-read pass's selectionKnown
	// hook and the pass's join it is the pass thread's alone; after the join the main thread's.
	struct Output {
		DeviceBuffer outJobs, outRecs, outOffsets, outMapSizes, outPathText, outCigarText, outVgBytes, outTotals;   // output encoding on the device (gc_output.hip)
		DeviceBuffer corrLens, corrOffsets, corrText, corrTotal;   // corrected reads' pieces (gc_corrected.hip; device_output & 8)
		PinnedBuffer hCorrLens, hCorrOffsets, hCorrText, hCorrTotal;
		PinnedBuffer hOutJobs, hOutRecs, hOutOffsets, hOutPathText, hOutCigarText, hOutVgBytes, hOutTotals;
		DeviceBuffer covKeep, covCells, covJobs;   // (coverage, gc_coverage.hip) a batch's keep bytes over its output jobs; the chained winners' cells and jobs
		PinnedBuffer hCovKeep, hCovCells, hCovJobs;
	} output;
	DeviceBuffer stitchSlotOf, stitchRegions, stitchNodes, stitchInfo, stitchCursor, stitchSpill;   // chain stitching on the device (gc_stitch.hip)
	DeviceBuffer anchorPerRead, anchorSlotEnd, anchorOff, anchorDense;   // the result's dense anchor arrays made on the device (gc_results.hip)
	PinnedBuffer hAnchorPerRead, hAnchorOff, hAnchorDense;
	PinnedBuffer hStitchNodes, hStitchInfo, hStitchCursor;
	EditDistanceRun edChainRun;
	DeviceBuffer edPathJobs, edPathOps, edPathLen, edPathScratch;   // alignment path of the chained alignment (gc_edpath.hip)
	PinnedBuffer hEdPathJobs, hEdPathOps, hEdPathLen;
	DeviceBuffer fastJobs, fastScore, fastTraceJobs, fastTrace, fastWritten;   // the chained alignment of gc_params::fast_mode (gc_fastchain.hip)
	PinnedBuffer hFastJobs, hFastScore, hFastTraceJobs, hFastTrace, hFastWritten;
	// The whole-read pass's own: what batch/gc_long_pass.hip (WholeReadPass) works in, kept from batch to batch. While a batch's pass thread runs it is that thread's alone.
	struct LongPass {
		hipStream_t longStream = nullptr;        // the pass runs on its own stream, concurrently with the fragment kernels
		// whole-read decision (selection + edit distance of the best alignment)
		struct LongDecision {
			PinnedBuffer hJobs, hPairs, hOut;
			DeviceBuffer jobs, letters, lettersLen, pairs, out;
			EditDistanceRun run;
			std::vector<uint32_t> pairRead;
			uint32_t nPairs = 0;
		} edLong;
		uint64_t longCellsPerBase = 4;           // merged-trace cells per read base the whole-read pass reserves (10 kb ONT-like reads use 1.1, 50 kb CLR-like reads on a genome with repeats 9-10; grows by what a batch asks for)
		RoundStream ownRounds;                   // the round loop's stream WITHOUT the token (GC_LONG_TOKEN=0; created by the stream's first such pass). With it the rounds run on the token slot's stream
		                                         // (SharedLongScratch::rounds); longStream carries the pass's uploads, its first select, reruns and decision
		DeviceBuffer longRetryList, longJobs, longAlns, longResults, longScratch, longCells, longCursor, longJobsFallback, longResultsFallback, longScratchFallback;
		DeviceBuffer longState, longWork, longWorkResults, longRoundTrace, longCandSeed, longWorkLen, longOrder;
		PinnedBuffer hLongJobs, hLongAlns, hLongResults, hLongSmall, hLongCells;
	} longPass;
	double fragShare = 0;                     // fragment extensions per read base in the stream's last batch (longTokenCount)
	uint64_t batchesDone = 0;                 // batches this stream has finished (a second whole-read token is only taken from the second batch on: the first sizes the stream's buffers)
	bool poolsRerun = false;                  // the last batch ran its fragment pipeline again with larger pools: the next one gives back what that overshot
	double traceCellsPerSlot = 0, pathWordsPerSlot = 0;   // what this stream's batches have used of the fragment pipeline's trace pool / anchor path pool per anchor slot (0: no batch yet)
	DeviceBuffer longSeeds;   // the seeds in the whole-read pass's order: written by the seeding stage, read by the pass
	DeviceBuffer gluePerRead, glueCursors, glueOut, glueSeedCap, glueSeedOff, glueWinCapOff, glueU32[8], glueSort, gluePos, glueWin;   // seed glue on the device (gc_seedglue.hip)
	PinnedBuffer hGlueOut, hGlueWinCapOff, hGlueSmall;
	// every device allocation of the stream with its size (GC_DEBUG_TIMES: "[gc mem]" lines; the whole-read decision's and the edit-distance runs' own buffers are listed by their owners)
	template <typename F> void forEachDeviceBuffer(F f) const
	{
		const LongPass& L = longPass;
		const Output& O = output;
		f("tmp", tmp.bytes); f("matches", matches.bytes); f("readMatchOff", readMatchOff.bytes); f("readMatchCount", readMatchCount.bytes); f("cursors", cursors.bytes); f("readSeeds", readSeeds.bytes);
		f("fragFirstSeed", fragFirstSeed.bytes); f("longRetryList", L.longRetryList.bytes); f("extLists", extLists.bytes); f("pendingFrags", pendingFrags.bytes); f("fragNext", fragNext.bytes);
		f("roundCounts", roundCounts.bytes); f("fragItems", fragItems.bytes); f("fragRetryList", fragRetryList.bytes); f("work", work.bytes); f("results", results.bytes); f("scratch", scratch.bytes); f("scratchRetry", scratchRetry.bytes); f("tracePool", tracePool.bytes);
		f("frags", frags.bytes); f("fragSeeds", fragSeeds.bytes); f("anchors", anchors.bytes); f("fragStatus", fragStatus.bytes); f("fragExtended", fragExtended.bytes); f("readTies", readTies.bytes);
		f("pathPool", pathPool.bytes); f("jobs", jobs.bytes); f("chainOut", chainOut.bytes); f("chainLen", chainLen.bytes); f("chainScore", chainScore.bytes); f("chainStatus", chainStatus.bytes);
		f("chainScratch", chainScratch.bytes); f("counters", counters.bytes); f("edPathNodes", edPathNodes.bytes); f("edJobs", edJobs.bytes); f("edLetters", edLetters.bytes);
		f("edLettersLen", edLettersLen.bytes); f("edPairs", edPairs.bytes); f("edOut", edOut.bytes); f("outJobs", O.outJobs.bytes); f("outRecs", O.outRecs.bytes); f("outOffsets", O.outOffsets.bytes);
		f("outMapSizes", O.outMapSizes.bytes); f("outPathText", O.outPathText.bytes); f("outCigarText", O.outCigarText.bytes); f("outVgBytes", O.outVgBytes.bytes); f("outTotals", O.outTotals.bytes);
		f("corrLens", O.corrLens.bytes); f("corrOffsets", O.corrOffsets.bytes); f("corrText", O.corrText.bytes); f("corrTotal", O.corrTotal.bytes);
		f("covKeep", O.covKeep.bytes); f("covCells", O.covCells.bytes); f("covJobs", O.covJobs.bytes);
		f("stitchSlotOf", stitchSlotOf.bytes); f("stitchRegions", stitchRegions.bytes); f("stitchNodes", stitchNodes.bytes); f("stitchInfo", stitchInfo.bytes); f("stitchCursor", stitchCursor.bytes); f("stitchSpill", stitchSpill.bytes);
		f("anchorPerRead", anchorPerRead.bytes); f("anchorSlotEnd", anchorSlotEnd.bytes); f("anchorOff", anchorOff.bytes); f("anchorDense", anchorDense.bytes);
		f("edPathJobs", edPathJobs.bytes); f("edPathOps", edPathOps.bytes); f("edPathLen", edPathLen.bytes); f("edPathScratch", edPathScratch.bytes); f("longSeeds", longSeeds.bytes);
		f("fastJobs", fastJobs.bytes); f("fastScore", fastScore.bytes); f("fastTraceJobs", fastTraceJobs.bytes); f("fastTrace", fastTrace.bytes); f("fastWritten", fastWritten.bytes);
		f("longJobs", L.longJobs.bytes); f("longAlns", L.longAlns.bytes); f("longResults", L.longResults.bytes); f("longScratch", L.longScratch.bytes); f("longCells", L.longCells.bytes);
		f("longCursor", L.longCursor.bytes); f("longJobsFallback", L.longJobsFallback.bytes); f("longResultsFallback", L.longResultsFallback.bytes); f("longScratchFallback", L.longScratchFallback.bytes);
		f("gluePerRead", gluePerRead.bytes); f("glueCursors", glueCursors.bytes); f("glueOut", glueOut.bytes); f("glueSeedCap", glueSeedCap.bytes); f("glueSeedOff", glueSeedOff.bytes);
		f("glueWinCapOff", glueWinCapOff.bytes); f("glueU32[0]", glueU32[0].bytes); f("glueU32[1]", glueU32[1].bytes); f("glueU32[2]", glueU32[2].bytes); f("glueU32[3]", glueU32[3].bytes);
		f("glueU32[4]", glueU32[4].bytes); f("glueU32[5]", glueU32[5].bytes); f("glueU32[6]", glueU32[6].bytes); f("glueU32[7]", glueU32[7].bytes); f("glueSort", glueSort.bytes);
		f("gluePos", gluePos.bytes); f("glueWin", glueWin.bytes); f("longState", L.longState.bytes); f("longWork", L.longWork.bytes); f("longWorkResults", L.longWorkResults.bytes);
		f("longRoundTrace", L.longRoundTrace.bytes); f("longCandSeed", L.longCandSeed.bytes); f("longWorkLen", L.longWorkLen.bytes); f("longOrder", L.longOrder.bytes);
		f("edLong.letters", L.edLong.letters.bytes); f("edLong.jobs+pairs+out", L.edLong.jobs.bytes + L.edLong.lettersLen.bytes + L.edLong.pairs.bytes + L.edLong.out.bytes);
	}
	~gc_stream()
	{
		for (auto& e : ev) if (e) (void)hipEventDestroy(e);
		for (auto& e : fragEv) if (e) (void)hipEventDestroy(e);
		longPass.ownRounds.release();
		if (stream) (void)hipStreamDestroy(stream);
		if (longPass.longStream) (void)hipStreamDestroy(longPass.longStream);
	}
};

// ----------------------------------------------------------------------------------------------------
// set of bases (A=1,C=2,G=4,T=8) a read character can stand for; 0 = matches nothing.
// reference: characterMatch / ambiguousMatch, src/GraphAlignerCommon.h:190-297
inline void buildIupacTable(uint8_t* t)
{
	memset(t, 0, 256);
	auto set = [&](const char* chars, uint8_t m) { for (const char* c = chars; *c; c++) t[(uint8_t)*c] = m; };
	set("Aa", 1); set("Cc", 2); set("Gg", 4); set("TtUu", 8);
	set("Rr", 1 | 4); set("Yy", 2 | 8); set("Kk", 4 | 8); set("Mm", 1 | 2); set("Ss", 2 | 4); set("Ww", 1 | 8);
	set("Bb", 2 | 4 | 8); set("Dd", 1 | 4 | 8); set("Hh", 1 | 2 | 8); set("Vv", 1 | 2 | 4); set("Nn", 15);
}

inline void uploadGraph(gc_graph* G)   // (reads GC_TEST_UPLOAD_SLICE)
{
	const gc::AlignmentGraph& h = G->host;
	size_t n = h.NodeSize();
	if (n >= 0xfffffff0ull) throw std::runtime_error("graph too large for 32-bit node ids");
	// Every staging array is uploaded and released before the next one is made: at 3.1 Gbp the flattened copies are ~90 GB together (28 B per graph base) beside a host graph
	// of ~230 GB - too much for a 300 GiB host when they all live until the function returns, as they did up to r5
	DGraph& d = G->dev;
	d.nNodes = (uint32_t)n;
	d.firstAmbiguous = (uint32_t)h.firstAmbiguous;
	int maxId = -1;
	{
		std::vector<uint8_t> nodeLength(n);
		std::vector<uint32_t> nodeOffset(n);
		std::vector<int32_t> nodeIDs(n);
		for (size_t i = 0; i < n; i++) {
			nodeLength[i] = (uint8_t)h.nodeLength[i];
			nodeOffset[i] = (uint32_t)h.nodeOffset[i];
			nodeIDs[i] = h.nodeIDs[i];
			maxId = std::max(maxId, h.nodeIDs[i]);
		}
		d.nodeLength = G->up(nodeLength);
		d.nodeOffset = G->up(nodeOffset);
		d.nodeIDs = G->up(nodeIDs);
	}
	{
		std::vector<uint32_t> componentNumber(n), componentMap(n), topoId(n);
		for (size_t i = 0; i < n; i++) {
			componentNumber[i] = (uint32_t)h.componentNumber[i];
			componentMap[i] = (uint32_t)h.component_map[i];
			topoId[i] = (uint32_t)h.topo_ids[h.component_map[i]][h.component_idx[i]];
		}
		d.componentNumber = G->up(componentNumber);
		d.componentMap = G->up(componentMap);
		d.topoId = G->up(topoId);
	}
	{
		std::vector<uint64_t> nodeSeq(2 * h.firstAmbiguous);
		for (size_t i = 0; i < h.firstAmbiguous; i++) { nodeSeq[2 * i] = h.nodeSequences[i][0]; nodeSeq[2 * i + 1] = h.nodeSequences[i][1]; }
		d.nodeSeq = G->up(nodeSeq);
	}
	{
		std::vector<uint64_t> ambSeq(4 * (n - h.firstAmbiguous));
		for (size_t i = h.firstAmbiguous; i < n; i++) {
			const gc::AmbiguousSeq& s = h.ambiguousNodeSequences[i - h.firstAmbiguous];
			size_t at = 4 * (i - h.firstAmbiguous);
			ambSeq[at] = s.A; ambSeq[at + 1] = s.C; ambSeq[at + 2] = s.G; ambSeq[at + 3] = s.T;
		}
		d.ambSeq = G->up(ambSeq);
	}
	auto csr = [&](const std::vector<std::vector<size_t>>& adj, const uint32_t*& devOff, const uint32_t*& devFlat) {
		std::vector<uint32_t> off(n + 1, 0), flat;
		for (size_t i = 0; i < n; i++) off[i + 1] = off[i] + (uint32_t)adj[i].size();
		flat.reserve(off[n]);
		for (size_t i = 0; i < n; i++) for (size_t v : adj[i]) flat.push_back((uint32_t)v);
		devOff = G->up(off); devFlat = G->up(flat);
	};
	csr(h.inNeighbors, d.inOff, d.inAdj);
	csr(h.outNeighbors, d.outOff, d.outAdj);
	const size_t nB = (size_t)maxId + 1;
	{
		std::vector<uint32_t> origSize(nB, 0), lookupOff(nB + 1, 0), lookup;
		lookup.reserve(n);
		for (size_t id = 0; id < nB; id++) {
			const bool known = h.nodeLookup.contains((int)id);
			lookupOff[id + 1] = lookupOff[id] + (known ? (uint32_t)h.nodeLookup.at((int)id).size() : 0u);
			if (known) {
				origSize[id] = (uint32_t)h.originalNodeSize.at((int)id);
				for (size_t s : h.nodeLookup.at((int)id)) lookup.push_back((uint32_t)s);
			}
		}
		for (size_t id = 0; id < nB; id++)
			for (uint32_t k = lookupOff[id]; k < lookupOff[id + 1]; k++)
				if (h.nodeOffset[lookup[k]] != 64ull * (k - lookupOff[id])) throw std::runtime_error("split nodes are not 64-aligned chunks of their original node");
		d.origSize = G->up(origSize); d.lookupOff = G->up(lookupOff); d.lookup = G->up(lookup);
		G->hOrigSize = std::move(origSize); G->hLookupOff = std::move(lookupOff); G->hLookup = std::move(lookup);
	}
	{
		// MPC index, flattened to global node ids. The per-node path lists stay on the host while the backward links - 12 bytes each, 4.5 per node - are made and sent in slices of
		// nodes: all of them at once were 37 GB of staging at 3.1 Gbp, the top of the host's peak (235 GiB of 300)
		std::vector<uint32_t> pathsOff(n + 1, 0), pathsFlat, pathsPos, backOff(n + 1, 0), mpcWidth(h.mpc.size());
		for (size_t c = 0; c < h.mpc.size(); c++) { mpcWidth[c] = (uint32_t)h.mpc[c].size(); G->maxMpcWidth = std::max(G->maxMpcWidth, mpcWidth[c]); }
		size_t nPaths = 0, nBack = 0;
		for (size_t i = 0; i < n; i++) { const size_t c = h.component_map[i], x = h.component_idx[i]; nPaths += h.paths[c][x].size(); nBack += h.backwards[c][x].size(); }
		if (nPaths >= 0xffffffffull || nBack >= 0xffffffffull) throw std::runtime_error("MPC index too large for 32-bit offsets");
		pathsFlat.reserve(nPaths);
		for (size_t i = 0; i < n; i++) {
			size_t c = h.component_map[i], x = h.component_idx[i];
			for (size_t k : h.paths[c][x]) pathsFlat.push_back((uint32_t)k);
			pathsOff[i + 1] = (uint32_t)pathsFlat.size();
			G->maxPathsPerNode = std::max(G->maxPathsPerNode, pathsOff[i + 1] - pathsOff[i]);
			backOff[i + 1] = backOff[i] + (uint32_t)h.backwards[c][x].size();
			G->maxBackPerNode = std::max(G->maxBackPerNode, backOff[i + 1] - backOff[i]);
		}
		// position of every node on every path through it (paths[v] lists path ids in ascending order, and a path visits
		// its nodes in order, so walking path k in order fills the (v,k) entries)
		pathsPos.assign(pathsFlat.size(), 0);
		for (size_t c = 0; c < h.mpc.size(); c++)
			for (size_t k = 0; k < h.mpc[c].size(); k++)
				for (size_t j = 0; j < h.mpc[c][k].size(); j++) {
					size_t node = h.mpc[c][k][j];
					for (uint32_t e = pathsOff[node]; e < pathsOff[node + 1]; e++) if (pathsFlat[e] == k) pathsPos[e] = (uint32_t)j;   // last visit wins, as in last2reach (:1340-1345)
				}
		auto posOf = [&](uint32_t node, uint32_t k) -> uint32_t {
			for (uint32_t e = pathsOff[node]; e < pathsOff[node + 1]; e++) if (pathsFlat[e] == k) return pathsPos[e];
			throw std::runtime_error("MPC index: node not on path");
		};
		uint32_t *dBackNode = nullptr, *dBackPath = nullptr, *dBackPos = nullptr;
		for (uint32_t** p : { &dBackNode, &dBackPath, &dBackPos }) { HIP_CHECK(hipMalloc((void**)p, std::max<size_t>(nBack, 1) * sizeof(uint32_t))); G->allocations.push_back(*p); }
		const size_t sliceLinks = gc::Switches::fromEnvironment().testUploadSlice;   // (test hook: many small slices)
		std::vector<uint32_t> backNode, backPath, backPos;
		for (size_t first = 0; first < n;) {
			size_t last = first;
			while (last < n && (last == first || (size_t)(backOff[last + 1] - backOff[first]) <= sliceLinks)) last++;
			backNode.clear(); backPath.clear(); backPos.clear();
			for (size_t i = first; i < last; i++) {
				const size_t c = h.component_map[i], x = h.component_idx[i];
				for (const auto& b : h.backwards[c][x]) {
					const uint32_t node = (uint32_t)h.component_ids[c][b.first], path = (uint32_t)b.second;
					backNode.push_back(node); backPath.push_back(path); backPos.push_back(posOf(node, path));
				}
			}
			if (backNode.size() != (size_t)(backOff[last] - backOff[first])) throw std::runtime_error("MPC index: backward links counted differently");
			if (!backNode.empty()) {
				HIP_CHECK(hipMemcpy(dBackNode + backOff[first], backNode.data(), backNode.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
				HIP_CHECK(hipMemcpy(dBackPath + backOff[first], backPath.data(), backPath.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
				HIP_CHECK(hipMemcpy(dBackPos + backOff[first], backPos.data(), backPos.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
			}
			first = last;
		}
		d.pathsOff = G->up(pathsOff); d.paths = G->up(pathsFlat); d.pathsPos = G->up(pathsPos);
		d.backOff = G->up(backOff); d.backNode = dBackNode; d.backPath = dBackPath; d.backPos = dBackPos;
		d.mpcWidth = G->up(mpcWidth);
	}
	{
		std::vector<uint32_t> chainNumber(n);
		std::vector<uint64_t> chainApproxPos(n);
		for (size_t i = 0; i < n; i++) {
			if (h.chainNumber[i] >= 0xffffffffull) throw std::runtime_error("too many chains for 32-bit chain numbers");
			chainNumber[i] = (uint32_t)h.chainNumber[i];
			chainApproxPos[i] = (uint64_t)h.chainApproxPos[i];
		}
		d.chainNumber = G->up(chainNumber);
		d.chainApproxPos = G->up(chainApproxPos);
	}
	{
		// the names the output encoders print (OriginalNodeName; empty: they print id / 2), by bigraph node id
		std::vector<uint32_t> nameOff(nB + 1, 0);
		std::vector<char> nameBytes;
		{
			size_t total = 1;
			for (size_t id = 0; id < nB; id++) if (const std::string* name = h.originalNodeName.find((int)id)) total += name->size();
			nameBytes.reserve(total);
		}
		for (size_t id = 0; id < nB; id++) {
			const std::string* name = h.originalNodeName.find((int)id);
			if (name) nameBytes.insert(nameBytes.end(), name->begin(), name->end());
			if (nameBytes.size() >= 0xffffffffull) throw std::runtime_error("node names exceed 4 GB");
			nameOff[id + 1] = (uint32_t)nameBytes.size();
		}
		nameBytes.push_back(0);
		G->devNames.nameOff = G->up(nameOff);
		G->devNames.nameBytes = G->up(nameBytes);
	}
	{
		NodeRec* recs = nullptr;
		HIP_CHECK(hipMalloc((void**)&recs, std::max<size_t>(1, n) * sizeof(NodeRec)));
		G->allocations.push_back(recs);
		launchBuildNodeRecs(nullptr, d, recs);
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipDeviceSynchronize());
		d.nodeRec = recs;
	}
	CorrectnessTables t;
	buildCorrectnessTables(t);
	HIP_CHECK(hipMalloc((void**)&G->devTables, sizeof(t)));
	G->allocations.push_back(G->devTables);
	HIP_CHECK(hipMemcpy(G->devTables, &t, sizeof(t), hipMemcpyHostToDevice));
	uint8_t iupac[256];
	buildIupacTable(iupac);
	HIP_CHECK(hipMalloc((void**)&G->devIupac, 256));
	G->allocations.push_back(G->devIupac);
	HIP_CHECK(hipMemcpy(G->devIupac, iupac, 256, hipMemcpyHostToDevice));
}

// One capacity: the GC_* environment variable (experiments, test hooks) wins over gc_params::capacity, 0 there means automatic.
inline int64_t capacityOr(std::optional<int64_t> env, int64_t param, int64_t automatic)
{
	if (env) return *env;
	return param != 0 ? param : automatic;
}

// gc_params_ext as the batch runs with it: the cut-off the reference would run with (0.66 for an X-drop without one, src/AlignerMain.cpp:443-448) and its error cost in double
struct ClipOptions {
	double cutoff = 0;     // preciseClippingIdentityCutoff; 0: clipping off
	double errorCost = 0;  // XscoreErrorCost = c / (1 - c) + 1 (src/GraphAlignerCommon.h:108)
	int32_t xDrop = 0;     // Xdropcutoff
	bool on() const { return cutoff != 0; }
	void apply(ExtendConfig& cfg) const { if (on()) { cfg.setClipErrorCost(errorCost); cfg.xDrop = xDrop; } }
};

template <typename F>
inline int guarded(F&& f)
{
	try {
		return f();
	} catch (const DeviceError& e) {
		return fail(GC_ERR_DEVICE, e.what());
	} catch (const std::exception& e) {
		return fail(GC_ERR_INTERNAL, e.what());
	}
}

inline void requireDevice()
{
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess || n <= 0) throw DeviceError("no HIP device available: the product path has no CPU fallback");
}

namespace gcrt {

// Chain stitching, reference: src/Aligner.cpp:754-822 (+ pathToTrace :409-424, getChainPath src/AlignmentGraph.cpp:1866-1916).
// The chain's anchor paths are concatenated; consecutive anchors that are not adjacent are bridged by the fewest-hops
// path (bounded BFS); where no bridge exists within --colinear-gap the path is cut and the longest piece (most graph
// bases, the size of the reference's pathToTrace vector) is kept. `slots` = this read's kept anchors in anchor-index
// order. The piece is returned as its node path plus the offsets of its first and last base; pathToTrace's cell list
// (one entry per base) follows from those and is not materialised here.
inline void stitchChain(const gc::AlignmentGraph& graph, long long colinearGap, const uint32_t* chain, uint32_t chainLen, const uint32_t* slots,
	const AnchorRec* anchors, const uint32_t* pathPool, StitchedPath& longest)
{
	std::vector<size_t> posPath;
	std::unordered_set<size_t> nodes;
	size_t firstNodeOffset = 0, lastNodeOffset = 0;
	longest = StitchedPath();
	auto keepIfLonger = [&]() {
		uint64_t cells = 0;   // size of pathToTrace(posPath, firstNodeOffset, lastNodeOffset), src/Aligner.cpp:409-424
		for (size_t node : posPath) {
			size_t S = 0, L = graph.NodeLength(node);
			if (node == posPath[0]) S = firstNodeOffset;
			else if (node == posPath.back()) L = lastNodeOffset + 1;
			cells += L > S ? L - S : 0;
		}
		if (longest.cells < cells) {
			longest.nodes.assign(posPath.begin(), posPath.end());
			longest.firstOffset = (uint32_t)firstNodeOffset;
			longest.lastOffset = (uint32_t)lastNodeOffset;
			longest.cells = cells;
		}
	};
	for (uint32_t c = 0; c < chainLen; c++) {
		const AnchorRec& a = anchors[slots[chain[c]]];
		const uint32_t* apath = pathPool + a.pathOff;
		if (posPath.empty()) {
			posPath.assign(apath, apath + a.pathLen);
			firstNodeOffset = a.firstOffset;
			lastNodeOffset = a.lastOffset;
			for (size_t j : posPath) nodes.insert(j);
		} else {
			bool gap = apath[0] == posPath.back() && colinearGap != -1 && (long long)a.firstOffset - (long long)lastNodeOffset > colinearGap + 1;
			std::vector<size_t> bridge;
			if (!nodes.count(apath[0]) && posPath.back() != a.firstNode) {
				long long gapLimit = colinearGap;
				if (gapLimit != -1) gapLimit -= (long long)a.firstOffset + (long long)(graph.NodeLength(posPath.back()) - (long long)lastNodeOffset - 1);
				bridge = graph.getChainPath(posPath.back(), a.firstNode, gapLimit);
				if (bridge.empty()) gap = true;
			}
			if (gap) {
				keepIfLonger();
				nodes.clear();
				posPath.clear();
				firstNodeOffset = a.firstOffset;
			} else {
				for (size_t j : bridge) if (!nodes.count(j)) { nodes.insert(j); posPath.push_back(j); }
			}
			for (uint32_t k = 0; k < a.pathLen; k++) { size_t j = apath[k]; if (!nodes.count(j)) { nodes.insert(j); posPath.push_back(j); } }
			lastNodeOffset = a.lastOffset;
		}
	}
	if (!posPath.empty()) keepIfLonger();
}

// Exact-match bit vectors of a read for the NW kernel: [A,C,G,T][words], bit i set when base i is exactly that letter.
inline void buildEqMasks(const char* seq, uint64_t len, uint64_t words, uint64_t* out)
{
	for (uint64_t i = 0; i < len; i++) {
		int b = seq[i] == 'A' ? 0 : seq[i] == 'C' ? 1 : seq[i] == 'G' ? 2 : seq[i] == 'T' ? 3 : -1;
		if (b >= 0) out[(uint64_t)b * words + (i >> 6)] |= 1ull << (i & 63);
	}
}

// Runs the NW kernel over `pairs`. The rows-per-lane unit (1, 2, 4, 8, 16 blocks) a pair needs follows from its band
// half-width k and its read length (gc_editdist.hip); pairs are grouped by unit, every group runs on its own stream (a
// group of a few wide-band pairs is one long-running wave each and would otherwise hold up the others), and pairs
// whose k had to grow past their unit's limit are rerun with the next unit.
// hPairs/hOut: pinned host staging; dPairs/dOut: device arrays of at least nPairs elements; readLen: host read lengths.
inline uint32_t editDistanceUnit(uint32_t k, uint32_t readLen)
{
	uint32_t unit = 1;
	while (unit < 16 && k >= editDistanceMaxK(unit) && (readLen + 64 * unit - 1) / (64 * unit) > 64) unit *= 2;
	return unit;
}
// Every stream of the library (fragment pipeline, edit distances, whole-read pass) is non-blocking with the default priority.
inline void createStream(hipStream_t* q) { HIP_CHECK(hipStreamCreateWithFlags(q, hipStreamNonBlocking)); }

inline void launchEditDistances(EditDistanceRun& run, hipStream_t stream, EdPair* hPairs, int64_t* hOut, uint32_t nPairs, EdPair* dPairs, int64_t* dOut, const EdRead* dReads, const char* dBases,
	const uint64_t* dEqMasks, const char* dLetters, const uint32_t* dLettersLen, const std::function<uint32_t(uint32_t)>& readLen, bool debugTimes)
{
	if (!nPairs) return;
	if (!run.ready) HIP_CHECK(hipEventCreateWithFlags(&run.ready, hipEventDisableTiming));
	// (a class's stream is created when the class is first used: the batch's streams share the device's 16 hardware queues, and on cfg2 only the
	// two-pairs-per-wave class and the one-block class ever hold pairs)
	std::vector<uint32_t> cls(nPairs), lenOf(nPairs);
	uint32_t count[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
	uint32_t blockThreads = 64;        // class 7: threads of a workgroup = the 64-row blocks of the class's longest read
	uint32_t* begin = run.begin;
	for (uint32_t i = 0; i < nPairs; i++) {
		const uint32_t len = readLen(hPairs[i].read);
		lenOf[i] = len;
		const uint32_t askedK = hPairs[i].k;   // the caller's band, before the team classes widen it to what their lanes hold anyway (class 7 below is judged on this one: ADVICE r4)
		uint32_t unit = editDistanceUnit(hPairs[i].k, len), c = 0;
		while ((1u << c) < unit) c++;
		c += 2;                                                               // classes 2..6: one pair per wave, units of 1..16 blocks
		if (unit == 1 && hPairs[i].k < editDistanceMaxK(0) && len <= 131072) {   // class 1: two pairs per wave (small first band)
			c = 1;
			// class 0 (r4): three pairs per wave, bands up to what a team of 21 lanes holds (1 441 with groups of 8 columns). A whole-read pair's k comes from the alignment itself:
			// one sweep, always enough. A chain pair's k is a guess: at the r4 limit of 1 289, 45 % of cfg2's chain pairs (distances 1 100-1 300) came back for a second sweep and
			// they stayed with two per wave; at 1 441, 0.7 % come back and the caller sends them here (gc_batch_results.inc)
			if (len <= 65536 && hPairs[i].k < editDistanceTeamMaxK(3)) c = 0;
			// a sweep of these kernels takes column groups + units steps whatever the band, as long as the band fits the team's lanes - so the first guess may as well be the widest band that
			// does (any k >= the distance gives the distance): a chain pair whose guess (length difference + 14 %) was a little short used to pay a failed sweep here, a second
			// failed sweep with the same guess in the one-pair-per-wave kernel and a third with the doubled band (r3)
			hPairs[i].k = c == 0 ? editDistanceTeamMaxK(3) - 1 : std::max(hPairs[i].k, editDistanceMaxK(0) - 1);
		}
		// class 7 (r4): a band of half the read or more covers most of the matrix - a chain whose path spells a fraction of its read, a whole-read alignment of a sliver: the pair
		// gets a workgroup with one thread per 64-row block and the whole matrix (exact, no retry) instead of one wave with up to sixteen blocks per lane and step
		if (len >= 1 && len <= editDistanceBlockMaxRows() && 2ull * askedK >= len) { hPairs[i].k = askedK; c = 7; blockThreads = std::max(blockThreads, (len + 63u) / 64u); }
		cls[i] = c;
		count[c]++;
	}
	begin[0] = 0;
	for (int c = 0; c < 8; c++) begin[c + 1] = begin[c] + count[c];
	run.perm.resize(nPairs);
	{
		uint32_t at[8] = { begin[0], begin[1], begin[2], begin[3], begin[4], begin[5], begin[6], begin[7] };
		std::vector<EdPair> grouped(nPairs);
		run.lens.resize(nPairs);
		for (uint32_t i = 0; i < nPairs; i++) { grouped[at[cls[i]]] = hPairs[i]; run.lens[at[cls[i]]] = lenOf[i]; run.perm[at[cls[i]]++] = i; }
		memcpy(hPairs, grouped.data(), (size_t)nPairs * sizeof(EdPair));   // hPairs is now in grouped order
	}
	HIP_CHECK(hipMemcpyAsync(dPairs, hPairs, (size_t)nPairs * sizeof(EdPair), hipMemcpyHostToDevice, stream));
	HIP_CHECK(hipEventRecord(run.ready, stream));
	for (int c = 0; c < 8; c++) {
		if (!count[c]) continue;
		if (!run.streams[c]) createStream(&run.streams[c]);
		HIP_CHECK(hipStreamWaitEvent(run.streams[c], run.ready, 0));
		if (c == 7) launchEditDistanceBlock(run.streams[c], blockThreads, dPairs + begin[c], count[c], dReads, dBases, dEqMasks, dLetters, dLettersLen, dOut + begin[c]);
		else if (c < 2) launchEditDistanceTeam(run.streams[c], c == 0 ? 3u : 2u, dPairs + begin[c], count[c], dReads, dBases, dEqMasks, dLetters, dLettersLen, dOut + begin[c]);
		else launchEditDistance(run.streams[c], 1u << (c - 2), dPairs + begin[c], count[c], dReads, dBases, dEqMasks, dLetters, dLettersLen, dOut + begin[c]);
		HIP_CHECK(hipMemcpyAsync(hOut + begin[c], dOut + begin[c], (size_t)count[c] * sizeof(int64_t), hipMemcpyDeviceToHost, run.streams[c]));
	}
	if (debugTimes) fprintf(stderr, "[gc times] edit distance classes (3 per wave, 2 per wave, units 1..16, workgroup per pair): %u %u %u %u %u %u %u %u\n", count[0], count[1], count[2], count[3], count[4], count[5], count[6], count[7]);
}
inline void finishEditDistances(EditDistanceRun& run, hipStream_t stream, EdPair* hPairs, int64_t* hOut, uint32_t nPairs, EdPair* dPairs, int64_t* dOut, const EdRead* dReads, const char* dBases,
	const uint64_t* dEqMasks, const char* dLetters, const uint32_t* dLettersLen, bool debugTimes)
{
	if (!nPairs) return;
	for (auto& q : run.streams) if (q) syncStream(q);
	// reruns for the pairs whose band outgrew their unit (grouped order throughout)
	std::vector<uint32_t> todo;
	for (uint32_t i = 0; i < nPairs; i++) {
		if (hOut[i] == -2) todo.push_back(i);   // (-3: the path letters overflowed their slot - stays, the caller flags the read)
	}
	std::vector<EdPair> sub;
	std::vector<int64_t> subOut;
	if (debugTimes) fprintf(stderr, "[gc times] edit distance reruns: %zu of %u pairs\n", todo.size(), nPairs);
	// unit 0 here: the two-pairs-per-wave kernel for what the three-pairs-per-wave kernel handed back (its pairs come first in the grouped order)
	for (uint32_t unit = 0; unit <= 16 && !todo.empty(); unit = unit ? unit * 2 : 1) {   // (unit 1 for what the two-pairs-per-wave kernel handed back)
		std::vector<uint32_t> later;
		if (unit == 0) {
			std::vector<uint32_t> now;
			for (uint32_t i : todo) (i < run.begin[1] ? now : later).push_back(i);
			todo.swap(now);
			if (todo.empty()) { todo.swap(later); continue; }
		}
		// r4: from unit 4 on a rerun goes to the workgroup-per-pair kernel when the read fits it (<= 65 536 bases): columns + blocks steps whatever the band, exact - a pair that has failed the
		// narrower bands is far from its path, and the wide units give it one wave with 4-16 blocks per lane and step (config 5: 145 ms at unit 8, 304 ms at unit 16 per launch)
		if (unit >= 4) {
			std::vector<uint32_t> wide, rest;
			uint32_t threads = 64;
			for (uint32_t i : todo) {
				if (run.lens[i] >= 1 && run.lens[i] <= editDistanceBlockMaxRows()) { wide.push_back(i); threads = std::max(threads, (run.lens[i] + 63u) / 64u); }
				else rest.push_back(i);
			}
			if (!wide.empty()) {
				sub.resize(wide.size());
				subOut.resize(wide.size());
				for (size_t i = 0; i < wide.size(); i++) sub[i] = hPairs[wide[i]];
				HIP_CHECK(hipMemcpyAsync(dPairs, sub.data(), sub.size() * sizeof(EdPair), hipMemcpyHostToDevice, stream));
				launchEditDistanceBlock(stream, threads, dPairs, (uint32_t)sub.size(), dReads, dBases, dEqMasks, dLetters, dLettersLen, dOut);
				HIP_CHECK(hipMemcpyAsync(subOut.data(), dOut, sub.size() * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
				syncStream(stream);
				for (size_t i = 0; i < wide.size(); i++) hOut[wide[i]] = subOut[i];
			}
			todo.swap(rest);
			if (todo.empty()) break;
		}
		sub.resize(todo.size());
		subOut.resize(todo.size());
		// (what reaches unit U has failed every band below it: the team kernels' limits for U = 0 and 1, the limit of unit U / 2 otherwise - start there, not at the first guess)
		const uint32_t failedBelow = unit == 0 ? editDistanceMaxK(0) - 1 : unit == 1 ? editDistanceMaxK(0) : editDistanceMaxK(unit / 2);
		for (size_t i = 0; i < todo.size(); i++) { sub[i] = hPairs[todo[i]]; sub[i].k = std::max(sub[i].k, failedBelow); }
		HIP_CHECK(hipMemcpyAsync(dPairs, sub.data(), sub.size() * sizeof(EdPair), hipMemcpyHostToDevice, stream));
		launchEditDistance(stream, unit, dPairs, (uint32_t)sub.size(), dReads, dBases, dEqMasks, dLetters, dLettersLen, dOut);
		HIP_CHECK(hipMemcpyAsync(subOut.data(), dOut, sub.size() * sizeof(int64_t), hipMemcpyDeviceToHost, stream));
		syncStream(stream);
		std::vector<uint32_t> next;
		for (size_t i = 0; i < todo.size(); i++) { hOut[todo[i]] = subOut[i]; if (subOut[i] == -2) next.push_back(todo[i]); }
		todo.swap(next);
		todo.insert(todo.end(), later.begin(), later.end());
	}
	// still -2: the band is too wide for the NW kernel (a read longer than 65536 bases 64000 or more edits away from its path: k_edit_distance<16> ends on the widest band its lanes hold); the caller flags the read
	// back to the caller's order
	run.grouped.assign(hOut, hOut + nPairs);
	for (uint32_t i = 0; i < nPairs; i++) hOut[run.perm[i]] = run.grouped[i];
}

template <typename T> inline T* copyOut(const std::vector<T>& v)
{
	T* p = mallocArray<T>(v.size());
	if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
	return p;
}

} // namespace
