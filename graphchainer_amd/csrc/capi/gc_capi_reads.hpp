// What the read loaders share (capi/gc_capi_reads.hip defines it; capi/gc_capi_bam.hip uses it): where a parse's bytes come from, the end of every parse - from read and id
// offsets on the host to the gc_reads and the host's table - and the BGZF front of the two *_bgzf entry points.
#pragma once
#include "../gc_runtime.hpp"
#include <functional>

// Where the bytes of a parse come from. place() puts the len bytes at devText with work on q (pinnedText [len] is the call's staging block, free until the tables are built)
// and returns their last byte (any value for none); done(), if set, runs once the tables are built, while the bytes still lie on the device.
struct FxSource {
	uint32_t len = 0;
	std::function<char(char* devText, char* pinnedText, hipStream_t q, int device)> place;
	std::function<void(const char* devText, uint32_t consumed, hipStream_t q)> done;
};
struct InvalidInput : std::runtime_error { using std::runtime_error::runtime_error; };   // GC_ERR_INVALID from inside a guarded call

// a parse's second, small pinned block: offsets | id offsets | invalid flags | the four layout arrays that go up; n: the reads, or a bound on them
struct BatchStaging {
	size_t off, nameOff, invalid, maskOff, maskWords, eqOff, edReads, bytes;
	explicit BatchStaging(uint64_t n)
	{
		gc::Arena s;
		off = s.part((n + 1) * 8); nameOff = s.part((n + 1) * 4); invalid = s.part(n); maskOff = s.part(n * 8); maskWords = s.part(n * 4); eqOff = s.part(n * 8); edReads = s.part(n * sizeof(EdRead));
		bytes = s.bytes();
	}
};

// The end of a parse. S: the staging block, its offsets [n + 1] and id offsets [n + 1] filled in; H: pinned, at least `limit` bytes (bases and ids come down into it: together
// they are no longer than the bytes they were parsed from); devNames: the ids on the device. Builds the read batch in the one layout gc_reads_upload builds its batch in -
// gather(devBases) writes the bases where the upload's copy would have put them, the packing kernels follow - then calls done(), if set, and makes the host's table *T
// (malloc'd) with `consumed` and the kernel time, to which the gather's and the packing kernels' is added. `what` names the entry point in what it throws.
void finishParsedBatch(const char* what, gc_reads* R, gc_fastx_table** T, hipStream_t q, EventSet<2>& ev, double& kernelMs, uint64_t n, uint32_t total, uint32_t limit, uint32_t consumed,
	char* S, const BatchStaging& st, char* H, const char* devNames, HeldBlock& batchBlock, const std::function<hipError_t(char* devBases)>& gather, const std::function<void()>& done);

// The two *_bgzf entry points behind their own checks: scans the whole BGZF blocks at the front of data, refuses head + inflated text of 2^32 - 16 bytes or more, and calls
// parse() with a source that puts head and the inflated blocks together on the device and brings the bytes behind the parse's `consumed` down as the tail.
int parseOverBgzf(const char* what, const char* head, uint64_t head_len, const void* data, uint64_t len, const std::function<int(const FxSource&)>& parse,
	char** tail, uint64_t* tail_len, uint64_t* consumed, gc_bgzf_stats* stats);
