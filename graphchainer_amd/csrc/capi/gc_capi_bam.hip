// C entry points, unaligned BAM read files: gc_reads_parse_bam, gc_reads_parse_bam_bgzf. The bytes go up once (or are inflated where they lie); record starts, fields, ids and
// letters are made on the device (hip/gc_bam.hip), and the batch is finished as gc_reads_parse finishes its own (finishParsedBatch): the same layout, the same packing kernels.
#include "gc_capi_reads.hpp"
#include "../hip/gc_bam_core.hpp"

static_assert(GC_FASTX_FINAL == gcdev::BAM_FINAL && GC_BAM_HEADER == gcdev::BAM_HEADER, "the header's constants are the kernels'");

// gc_reads_parse_bam and gc_reads_parse_bam_bgzf from the point where the bytes lie on the device
static int bamParseFrom(const char* what, const FxSource& src, uint32_t flags, gc_reads** reads, gc_fastx_table** table, gc_bam_stats* stats)
{
	gc_reads* R = new gc_reads();
	gc_fastx_table* T = nullptr;
	gc_bam_stats bam {};
	auto body = [&]() {
		requireDevice();
		using namespace gcdev;
		HIP_CHECK(hipGetDevice(&R->device));
		const int device = R->device;
		hipStream_t q = threadStream(device);
		const uint32_t L = src.len;
		HeldBlock textBlock(g_readDeviceBlocks, device, q), tableBlock(g_readDeviceBlocks, device, q), pinned(g_readPinnedBlocks, device, q), small(g_readPinnedBlocks, device, q),
			batchBlock(g_readDeviceBlocks, device, q);
		EventSet<2> ev;
		EventSet<3> stage;
		double kernelMs = 0;

		// ---- 1: the bytes go up; one wave walks the header and the chain of block_size words ----
		// device: bytes [L] (their part is a multiple of 256, so the walk's 16-byte loads stay inside it) | record starts (a record has 36 bytes at least) | counts
		const size_t recordRoom = (size_t)L / (4 + BAM_FIXED) + 1;
		gc::Arena textParts;
		textParts.part(L);
		const size_t oRecStart = textParts.part(recordRoom * 4), oMeta = textParts.part(BAM_META_WORDS * sizeof(uint32_t));
		gc::Arena pinnedParts;   // pinned: bytes [L], used again at the end for the bases and ids coming down | counts
		pinnedParts.part(L);
		const size_t hMeta = pinnedParts.part(BAM_META_WORDS * sizeof(uint32_t));
		char* H = (char*)pinned.acquire(pinnedParts.bytes());
		uint32_t* hostMeta = (uint32_t*)(H + hMeta);
		char* devText = (char*)textBlock.acquire(textParts.bytes());
		const uint8_t* text = (const uint8_t*)devText;
		uint32_t* devMeta = (uint32_t*)(devText + oMeta);
		src.place(devText, H, q, device);
		HIP_CHECK(hipEventRecord(ev[0], q));
		HIP_CHECK(bamWalkRecords(q, text, L, flags, (uint32_t*)(devText + oRecStart), devMeta));
		HIP_CHECK(hipEventRecord(ev[1], q));
		HIP_CHECK(hipMemcpyAsync(hostMeta, devMeta, BAM_META_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipStreamSynchronize(q));
		bam.walk_ms = ev.elapsedMs(0, 1);
		kernelMs += bam.walk_ms;
		const uint32_t nRecords = hostMeta[BAM_META_RECORDS], consumed = hostMeta[BAM_META_CONSUMED], walkStatus = hostMeta[BAM_META_WALK_STATUS], walkBadAt = hostMeta[BAM_META_WALK_BAD_AT];
		if (nRecords >= recordRoom || consumed > L || walkStatus >= BAM_STATUS_COUNT) throw std::runtime_error(std::string(what) + ": the record table is out of range");
		if (walkStatus != BAM_OK && hostMeta[BAM_META_IN_HEADER])
			throw InvalidInput(std::string(what) + ": the file header at byte 0 refused: " + bamStatusName(walkStatus));

		// ---- 2: fields, scans, the kept records' tables, ids; counts and offsets come down together (sized by the records, of which the kept ones are a part) ----
		const size_t n1 = (size_t)nRecords + 1;
		gc::Arena a;
		const size_t oKeep = a.part(n1 * 4), oSeqLen = a.part(n1 * 4), oNameLen = a.part(n1 * 4), oKept = a.part(n1 * 4), oSeqOff = a.part(n1 * 4), oNameOffAll = a.part(n1 * 4),
			oSpansAll = a.part(n1 * sizeof(BamSpan)), oSpans = a.part(n1 * sizeof(BamSpan)), oReadOff = a.part(n1 * 8), oNameOff = a.part(n1 * 4), oNames = a.part((size_t)L + 1);
		BamTables t {};
		t.tempBytes = bamScanTempBytes(nRecords);
		const size_t oTemp = a.part(t.tempBytes);
		char* D = (char*)tableBlock.acquire(a.bytes());
		t.recStart = (const uint32_t*)(devText + oRecStart); t.keep = (uint32_t*)(D + oKeep); t.seqLen = (uint32_t*)(D + oSeqLen); t.nameLen = (uint32_t*)(D + oNameLen); t.kept = (uint32_t*)(D + oKept);
		t.seqOff = (uint32_t*)(D + oSeqOff); t.nameOffAll = (uint32_t*)(D + oNameOffAll); t.spansAll = (BamSpan*)(D + oSpansAll); t.spans = (BamSpan*)(D + oSpans); t.readOff = (uint64_t*)(D + oReadOff);
		t.nameOff = (uint32_t*)(D + oNameOff); t.meta = devMeta; t.temp = D + oTemp;
		const BatchStaging st(nRecords);
		char* S = (char*)small.acquire(st.bytes);
		uint64_t* hostOff = (uint64_t*)(S + st.off);
		uint32_t* hostNameOff = (uint32_t*)(S + st.nameOff);
		HIP_CHECK(hipEventRecord(stage[0], q));
		HIP_CHECK(bamBuildRecords(q, text, nRecords, t));
		HIP_CHECK(hipEventRecord(stage[1], q));
		HIP_CHECK(bamWriteNames(q, text, nRecords, t, D + oNames));
		HIP_CHECK(hipEventRecord(stage[2], q));
		HIP_CHECK(hipMemcpyAsync(hostMeta, devMeta, BAM_META_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipMemcpyAsync(hostOff, D + oReadOff, n1 * 8, hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipMemcpyAsync(hostNameOff, D + oNameOff, n1 * 4, hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipStreamSynchronize(q));
		bam.fields_ms = stage.elapsedMs(0, 1); bam.names_ms = stage.elapsedMs(1, 2);
		kernelMs += bam.fields_ms + bam.names_ms;

		// the first record refused: by its fields, or the one at which the walk stopped (behind every record whose fields were looked at)
		unsigned long long refused = (unsigned long long)hostMeta[BAM_META_REFUSED_LO] | (unsigned long long)hostMeta[BAM_META_REFUSED_HI] << 32;
		uint32_t refusedAt = walkBadAt;
		if (refused != BAM_NONE_REFUSED) {
			if ((refused >> BAM_STATUS_BITS) >= nRecords) throw std::runtime_error(std::string(what) + ": the refused record is out of range");
			HIP_CHECK(hipMemcpyAsync(hostMeta, t.recStart + (refused >> BAM_STATUS_BITS), sizeof(uint32_t), hipMemcpyDeviceToHost, q));
			HIP_CHECK(hipStreamSynchronize(q));
			refusedAt = hostMeta[0];
		} else if (walkStatus != BAM_OK) refused = ((unsigned long long)nRecords << BAM_STATUS_BITS) | walkStatus;
		if (refused != BAM_NONE_REFUSED)
			throw InvalidInput(std::string(what) + ": record " + std::to_string(refused >> BAM_STATUS_BITS) + " at byte " + std::to_string(refusedAt) + " refused: " +
				bamStatusName((uint32_t)(refused & ((1u << BAM_STATUS_BITS) - 1))));
		const uint32_t nKept = hostMeta[BAM_META_KEPT], total = hostMeta[BAM_META_BASES];
		if (nKept > nRecords || total > L) throw std::runtime_error(std::string(what) + ": the record table is out of range");
		bam.records = nRecords; bam.skipped = nRecords - nKept;

		// ---- 3: the read batch and the host's table ----
		finishParsedBatch(what, R, &T, q, ev, kernelMs, nKept, total, L, consumed, S, st, H, D + oNames, batchBlock,
			[&](char* devBases) {
				HIP_CHECK(hipEventRecord(stage[0], q));
				const hipError_t e = bamUnpackBases(q, text, t, nKept, total, devBases);
				HIP_CHECK(hipEventRecord(stage[1], q));
				return e;
			}, [&]() { bam.unpack_ms = stage.elapsedMs(0, 1); if (src.done) src.done(devText, consumed, q); });
		return (int)GC_OK;
	};
	int rc = guarded([&]() { try { return body(); } catch (const InvalidInput& e) { return fail(GC_ERR_INVALID, e.what()); } });
	if (rc != GC_OK) {
		delete R;
		free(T);
		return rc;
	}
	*reads = R;
	*table = T;
	if (stats) *stats = bam;
	return GC_OK;
}

extern "C" {

int gc_reads_parse_bam(const void* data, uint64_t len, uint32_t flags, gc_reads** reads, gc_fastx_table** table, gc_bam_stats* stats)
{
	// host checks first: a malformed call is GC_ERR_INVALID whether or not a device is present
	if (!reads || !table || (!data && len)) return fail(GC_ERR_INVALID, "null argument");
	*reads = nullptr; *table = nullptr;
	if (stats) *stats = gc_bam_stats {};
	if (flags & ~(uint32_t)(GC_FASTX_FINAL | GC_BAM_HEADER)) return fail(GC_ERR_INVALID, "gc_reads_parse_bam: unknown flag bits");
	if (len >= 0xfffffff0ull) return fail(GC_ERR_INVALID, "gc_reads_parse_bam: the loader uses 32-bit positions: split the bytes into chunks below 2^32 - 16 bytes");
	FxSource src;
	src.len = (uint32_t)len;
	src.place = [&](char* devText, char* pinnedText, hipStream_t q, int) {
		if (!len) return '\0';
		memcpy(pinnedText, data, len);
		HIP_CHECK(hipMemcpyAsync(devText, pinnedText, len, hipMemcpyHostToDevice, q));
		return '\0';
	};
	return bamParseFrom("gc_reads_parse_bam", src, flags, reads, table, stats);
}

int gc_reads_parse_bam_bgzf(const void* head, uint64_t head_len, const void* data, uint64_t len, uint32_t flags, gc_reads** reads, gc_fastx_table** table,
	void** tail, uint64_t* tail_len, uint64_t* consumed, gc_bgzf_stats* stats, gc_bam_stats* bam_stats)
{
	if (!reads || !table || !tail || !tail_len || !consumed || (!head && head_len) || (!data && len)) return fail(GC_ERR_INVALID, "null argument");
	*reads = nullptr; *table = nullptr; *tail = nullptr; *tail_len = 0; *consumed = 0;
	if (stats) *stats = gc_bgzf_stats {};
	if (bam_stats) *bam_stats = gc_bam_stats {};
	if (flags & ~(uint32_t)(GC_FASTX_FINAL | GC_BAM_HEADER)) return fail(GC_ERR_INVALID, "gc_reads_parse_bam_bgzf: unknown flag bits");
	char* tailMem = nullptr;
	const int rc = parseOverBgzf("gc_reads_parse_bam_bgzf", (const char*)head, head_len, data, len,
		[&](const FxSource& src) { return bamParseFrom("gc_reads_parse_bam_bgzf", src, flags, reads, table, bam_stats); }, &tailMem, tail_len, consumed, stats);
	*tail = tailMem;
	return rc;
}

} // extern "C"
