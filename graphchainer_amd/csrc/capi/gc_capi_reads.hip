// C entry points, read batches: gc_reads_upload, gc_reads_destroy, gc_reads_parse, gc_reads_parse_bgzf, gc_bgzf_inflate, gc_fastx_table_free. Every batch is laid out by
// host/gc_layout.hpp's ReadBatchLayout and bound by bindReads (gc_runtime.hpp).
#include "gc_capi_reads.hpp"
#include "../hip/gc_fastx_core.hpp"
#include "../hip/gc_inflate_core.hpp"

extern "C" {

int gc_reads_upload(const char* bases, const uint64_t* offsets, uint64_t n, gc_reads** out)
{
	if (!offsets || !out || (!bases && n > 0 && offsets[n] > 0)) return fail(GC_ERR_INVALID, "null argument");
	*out = nullptr;
	gc_reads* R = new gc_reads();
	int rc = guarded([&]() {
		requireDevice();
		R->offsets.assign(offsets, offsets + n + 1);
		R->totalBases = offsets[n];
		if (n >= 0xffffffffull) throw std::runtime_error("too many reads in one batch");
		const gc::ReadBatchLayout L(offsets, n);
		const uint64_t total = R->totalBases;
		// one device block for everything (256-byte aligned parts), one pinned block for what goes up; both come from small caches (see BlockCache)
		HIP_CHECK(hipGetDevice(&R->device));
		hipStream_t q = threadStream(R->device);
		HeldBlock block(g_readDeviceBlocks, R->device, q);   // (the batch's own once the call has succeeded)
		bindReads(*R, L, block.acquire(L.blockBytes));
		// staging: the bases and the five small arrays in one pinned block, copied asynchronously on a stream of the calling thread's own (a synchronous copy from pageable
		// memory goes through the runtime's bounce buffers at a few GB/s and its null-stream semantics)
		gc::Arena h;
		const size_t hBases = h.part(total), hOffsets = h.part((n + 1) * sizeof(uint64_t)), hMaskOff = h.part(n * sizeof(uint64_t)), hMaskWords = h.part(n * sizeof(uint32_t)), hEqOff = h.part(n * sizeof(uint64_t)),
			hEdReads = h.part(n * sizeof(EdRead)), hInvalidBack = h.part(n);
		HeldBlock pinned(g_readPinnedBlocks, R->device, q);
		char* H = (char*)pinned.acquire(h.bytes());
		if (total) memcpy(H + hBases, bases, total);
		memcpy(H + hOffsets, offsets, (n + 1) * sizeof(uint64_t));
		if (total) HIP_CHECK(hipMemcpyAsync(R->devBases, H + hBases, total, hipMemcpyHostToDevice, q));
		HIP_CHECK(hipMemcpyAsync(R->devOffsets, H + hOffsets, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, q));
		stageReadLayout(*R, L, (uint64_t*)(H + hMaskOff), (uint32_t*)(H + hMaskWords), (uint64_t*)(H + hEqOff), (EdRead*)(H + hEdReads), q);
		launchPackReads(q, R->devOffsets, (uint32_t)n, total, R->devBases, R->devMaskOff, R->devMaskWords, R->devMasks, R->devEqOff, R->devEqMasks, R->devReadInvalid, R->devPacked, R->devInvalid, R->devChunkRead);
		R->invalid.assign(n, 0);
		if (n) HIP_CHECK(hipMemcpyAsync(H + hInvalidBack, R->devReadInvalid, n, hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipStreamSynchronize(q));
		if (n) memcpy(R->invalid.data(), H + hInvalidBack, n);
		R->deviceBlockBytes = block.bytes; R->deviceBlock = block.release();
		return (int)GC_OK;
	});
	if (rc != GC_OK) { delete R; return rc; }
	*out = R;
	return GC_OK;
}
void gc_reads_destroy(gc_reads* r) { delete r; }

} // extern "C"

void finishParsedBatch(const char* what, gc_reads* R, gc_fastx_table** T, hipStream_t q, EventSet<2>& ev, double& kernelMs, uint64_t n, uint32_t total, uint32_t limit, uint32_t consumed,
	char* S, const BatchStaging& st, char* H, const char* devNames, HeldBlock& batchBlock, const std::function<hipError_t(char* devBases)>& gather, const std::function<void()>& done)
{
	const std::string name(what);
	const uint64_t* hostOff = (const uint64_t*)(S + st.off);
	const uint32_t* hostNameOff = (const uint32_t*)(S + st.nameOff);
	const uint64_t namesBytes = hostNameOff[n];
	if (hostOff[n] != total || namesBytes + total > limit) throw std::runtime_error(name + ": the read offsets disagree with the base count");
	for (uint64_t r = 0; r < n; r++) if (hostOff[r + 1] < hostOff[r] || hostNameOff[r + 1] <= hostNameOff[r]) throw std::runtime_error(name + ": offsets decrease");

	R->offsets.assign(hostOff, hostOff + n + 1);
	R->totalBases = total;
	const gc::ReadBatchLayout lay(hostOff, n);
	bindReads(*R, lay, batchBlock.acquire(lay.blockBytes));
	HIP_CHECK(hipMemcpyAsync(R->devOffsets, hostOff, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, q));
	stageReadLayout(*R, lay, (uint64_t*)(S + st.maskOff), (uint32_t*)(S + st.maskWords), (uint64_t*)(S + st.eqOff), (EdRead*)(S + st.edReads), q);
	HIP_CHECK(hipEventRecord(ev[0], q));
	HIP_CHECK(gather(R->devBases));
	launchPackReads(q, R->devOffsets, (uint32_t)n, total, R->devBases, R->devMaskOff, R->devMaskWords, R->devMasks, R->devEqOff, R->devEqMasks, R->devReadInvalid, R->devPacked, R->devInvalid, R->devChunkRead);
	HIP_CHECK(hipEventRecord(ev[1], q));
	R->invalid.assign(n, 0);
	if (n) HIP_CHECK(hipMemcpyAsync(S + st.invalid, R->devReadInvalid, n, hipMemcpyDeviceToHost, q));
	if (total) HIP_CHECK(hipMemcpyAsync(H, R->devBases, total, hipMemcpyDeviceToHost, q));
	if (namesBytes) HIP_CHECK(hipMemcpyAsync(H + total, devNames, namesBytes, hipMemcpyDeviceToHost, q));
	HIP_CHECK(hipStreamSynchronize(q));
	kernelMs += ev.elapsedMs(0, 1);
	if (n) memcpy(R->invalid.data(), S + st.invalid, n);
	if (done) done();

	// the host's table: one allocation, the struct | offsets | name_off | bases | names
	const size_t tHead = (sizeof(gc_fastx_table) + 15) & ~(size_t)15, tArr = (n + 1) * sizeof(uint64_t);
	char* mem = (char*)malloc(tHead + 2 * tArr + total + namesBytes + 2);
	if (!mem) throw std::runtime_error(name + ": out of host memory");
	gc_fastx_table* t = (gc_fastx_table*)mem;
	*T = t;
	t->n_reads = n; t->consumed = consumed; t->kernel_ms = kernelMs;
	t->offsets = (uint64_t*)(mem + tHead); t->name_off = (uint64_t*)(mem + tHead + tArr); t->bases = mem + tHead + 2 * tArr; t->names = t->bases + total + 1;
	memcpy(t->offsets, hostOff, tArr);
	for (uint64_t r = 0; r <= n; r++) t->name_off[r] = hostNameOff[r];
	if (total) memcpy(t->bases, H, total);
	t->bases[total] = 0;
	if (namesBytes) memcpy(t->names, H + total, namesBytes);
	t->names[namesBytes] = 0;
	R->deviceBlockBytes = batchBlock.bytes; R->deviceBlock = batchBlock.release();
}

extern "C" {

// gc_reads_parse and gc_reads_parse_bgzf from the point where the text lies on the device
static int readsParseFrom(const FxSource& src, int32_t format, uint32_t flags, gc_reads** reads, gc_fastx_table** table)
{
	const uint64_t len = src.len;
	gc_reads* R = new gc_reads();
	gc_fastx_table* T = nullptr;
	auto body = [&]() {
		requireDevice();
		using namespace gcdev;
		HIP_CHECK(hipGetDevice(&R->device));
		const int device = R->device;
		hipStream_t q = threadStream(device);
		const uint32_t L = (uint32_t)len;
		const bool final = (flags & GC_FASTX_FINAL) != 0;
		// blocks of this call: the text and its tables on the device, one pinned block for what goes up and comes down, the batch's own block until the call has succeeded;
		// all from the read batches' caches
		HeldBlock textBlock(g_readDeviceBlocks, device, q), tableBlock(g_readDeviceBlocks, device, q), pinned(g_readPinnedBlocks, device, q), small(g_readPinnedBlocks, device, q),
			batchBlock(g_readDeviceBlocks, device, q);
		EventSet<2> ev;
		double kernelMs = 0;
		auto addSegment = [&]() { kernelMs += ev.elapsedMs(0, 1); };   // (after the synchronize that follows the segment)

		// ---- 1: the text goes up, its newlines are counted (the line tables are sized by the count) ----
		// pinned: text [L] | counts. The text's part is used again at the end for the bases and ids coming down: a line gives bytes to one of them at most, so both fit
		gc::Arena textParts;
		textParts.part(L);
		const size_t hMeta = textParts.part(FX_META_WORDS * sizeof(uint32_t));
		char* H = (char*)pinned.acquire(textParts.bytes());
		uint32_t* hostMeta = (uint32_t*)(H + hMeta);
		char* devText = (char*)textBlock.acquire(textParts.bytes());
		uint32_t* devMeta = (uint32_t*)(devText + hMeta);
		const char lastByte = src.place(devText, H, q, device);
		HIP_CHECK(hipEventRecord(ev[0], q));
		HIP_CHECK(fxCountNewlines(q, devText, L, devMeta));
		HIP_CHECK(hipEventRecord(ev[1], q));
		HIP_CHECK(hipMemcpyAsync(hostMeta, devMeta, FX_META_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipStreamSynchronize(q));
		addSegment();

		FxView v {};
		v.text = devText; v.len = L; v.format = format; v.final = final ? 1u : 0u;
		v.nNewlines = hostMeta[FX_META_NEWLINES];
		if (v.nNewlines > L) throw std::runtime_error("gc_reads_parse: more newlines than bytes");
		v.nLines = v.nNewlines + (final && L && lastByte != '\n' ? 1u : 0u);

		// ---- 2: line table, roles, destinations; the counts come down ----
		// device: per line, then per record (at most one per line), then the ids (every id with its NUL is as long as its header line: at most L bytes in all), then the scans' scratch
		const size_t lines = v.nLines;
		gc::Arena a;
		const size_t oLineEnd = a.part(lines * 4), oMap = a.part(lines), oScanned = a.part(lines), oHdr = a.part(lines * 4), oRecIdx = a.part(lines * 4), oContrib = a.part((lines + 1) * 4),
			oDest = a.part((lines + 1) * 4), oRecLine = a.part(lines * 4), oReadOff = a.part((lines + 1) * 8), oNameLen = a.part((lines + 1) * 4), oNameOff = a.part((lines + 1) * 4),
			oNames = a.part((size_t)L + 1);
		FxTables t {};
		t.tempBytes = fxScanTempBytes(L, v.nLines);
		const size_t oTemp = a.part(t.tempBytes);
		char* D = (char*)tableBlock.acquire(a.bytes());
		t.lineEnd = (uint32_t*)(D + oLineEnd); t.map = (uint8_t*)(D + oMap); t.scanned = (uint8_t*)(D + oScanned); t.hdr = (uint32_t*)(D + oHdr); t.recIdx = (uint32_t*)(D + oRecIdx);
		t.contrib = (uint32_t*)(D + oContrib); t.dest = (uint32_t*)(D + oDest); t.recLine = (uint32_t*)(D + oRecLine); t.meta = devMeta; t.temp = D + oTemp;
		v.lineEnd = t.lineEnd;
		uint32_t nHeaders = 0, nRecords = 0, total = 0, consumed = final ? L : 0;
		if (v.nLines) {
			HIP_CHECK(hipEventRecord(ev[0], q));
			HIP_CHECK(fxBuildTables(q, v, t));
			HIP_CHECK(hipEventRecord(ev[1], q));
			HIP_CHECK(hipMemcpyAsync(hostMeta, devMeta, FX_META_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, q));
			HIP_CHECK(hipStreamSynchronize(q));
			addSegment();
			if (v.nNewlines && hostMeta[FX_META_SELECTED] != v.nNewlines) throw std::runtime_error("gc_reads_parse: the line table disagrees with the newline count");
			nHeaders = hostMeta[FX_META_HEADERS]; nRecords = hostMeta[FX_META_RECORDS]; total = hostMeta[FX_META_BASES]; consumed = hostMeta[FX_META_CONSUMED];
			if (nRecords > nHeaders || nHeaders > v.nLines || total > L || consumed > L) throw std::runtime_error("gc_reads_parse: the record table is out of range");
		}
		const uint64_t n = nRecords;

		// ---- 3: read offsets and id offsets, down to the host for the per-read layout ----
		const BatchStaging st(n);
		char* S = (char*)small.acquire(st.bytes);
		uint64_t* hostOff = (uint64_t*)(S + st.off);
		uint32_t* hostNameOff = (uint32_t*)(S + st.nameOff);
		hostOff[0] = 0; hostNameOff[0] = 0;
		if (v.nLines) {
			HIP_CHECK(hipEventRecord(ev[0], q));
			HIP_CHECK(fxBuildRecords(q, v, t, nHeaders, nRecords, (uint64_t*)(D + oReadOff), (uint32_t*)(D + oNameLen), (uint32_t*)(D + oNameOff)));
			HIP_CHECK(fxWriteNames(q, v, t, nRecords, (const uint32_t*)(D + oNameOff), D + oNames));
			HIP_CHECK(hipEventRecord(ev[1], q));
			HIP_CHECK(hipMemcpyAsync(hostOff, D + oReadOff, (n + 1) * 8, hipMemcpyDeviceToHost, q));
			HIP_CHECK(hipMemcpyAsync(hostNameOff, D + oNameOff, (n + 1) * 4, hipMemcpyDeviceToHost, q));
			HIP_CHECK(hipStreamSynchronize(q));
			addSegment();
		}

		// ---- 4: the read batch and the host's table ----
		finishParsedBatch("gc_reads_parse", R, &T, q, ev, kernelMs, n, total, L, consumed, S, st, H, D + oNames, batchBlock,
			[&](char* devBases) { return v.nLines ? fxGatherBases(q, v, t, total, devBases) : hipSuccess; }, [&]() { if (src.done) src.done(devText, consumed, q); });
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
	return GC_OK;
}

// FASTA / FASTQ text -> the read batch gc_reads_upload builds from the same reads, and the host's table of them. The text goes up once; lines, roles, records, the
// compacted bases and the ids are made on the device (hip/gc_fastx.hip); the per-read layout needs the lengths on the host, so the offsets come down before the gather.
int gc_reads_parse(const char* text, uint64_t len, int32_t format, uint32_t flags, gc_reads** reads, gc_fastx_table** table)
{
	// host checks first: a malformed call is GC_ERR_INVALID whether or not a device is present
	if (!reads || !table || (!text && len)) return fail(GC_ERR_INVALID, "null argument");
	*reads = nullptr; *table = nullptr;
	if (format != GC_FASTX_FASTA && format != GC_FASTX_FASTQ) return fail(GC_ERR_INVALID, "gc_reads_parse: format is GC_FASTX_FASTA or GC_FASTX_FASTQ");
	if (flags & ~(uint32_t)GC_FASTX_FINAL) return fail(GC_ERR_INVALID, "gc_reads_parse: unknown flag bits");
	if (len >= 0xfffffff0ull) return fail(GC_ERR_INVALID, "gc_reads_parse: the loader uses 32-bit positions: split the text into chunks below 2^32 - 16 bytes");
	static_assert(GC_FASTX_FASTA == gcdev::FX_FASTA && GC_FASTX_FASTQ == gcdev::FX_FASTQ && GC_FASTX_FINAL == gcdev::FX_FINAL, "the header's constants are the kernels'");
	FxSource src;
	src.len = (uint32_t)len;
	src.place = [&](char* devText, char* pinnedText, hipStream_t q, int) {
		if (!len) return '\n';
		memcpy(pinnedText, text, len);
		HIP_CHECK(hipMemcpyAsync(devText, pinnedText, len, hipMemcpyHostToDevice, q));
		return text[len - 1];
	};
	return readsParseFrom(src, format, flags, reads, table);
}
void gc_fastx_table_free(gc_fastx_table* t) { free(t); }

// ---- BGZF: the whole blocks at the front of a compressed piece, inflated on the device (hip/gc_inflate.hip) --------------
namespace {

struct BgzfScan {
	std::vector<gcdev::InfBlock> blocks;   // inOff from the piece's start, outOff from the text's start (behind the head)
	std::vector<uint64_t> starts;          // of every block in the piece
	uint64_t consumed = 0, textBytes = 0;
};

// walks the BSIZE chain up to the first member that is not a whole BGZF block
static void bgzfScan(const uint8_t* data, uint64_t len, uint64_t headLen, BgzfScan& s)
{
	using namespace gcdev;
	while (s.consumed < len) {
		InfBlock b;
		uint32_t size = 0;
		if (infHeader(data + s.consumed, len - s.consumed, b, size) != INF_FRAME_BLOCK) break;
		b.inOff += s.consumed;
		b.outOff = headLen + s.textBytes;
		s.blocks.push_back(b);
		s.starts.push_back(s.consumed);
		s.textBytes += b.isize;
		s.consumed += size;
	}
}

// The blocks of the scan from data into devText (outOff counts from there), with work on q; waits for it. Throws InvalidInput naming the first bad block. lastByte, if
// asked for, is the byte at devText[lastAt]. Times: the copy to the staging block and up (uploadMs), the kernel (kernelMs).
static void bgzfInflateTo(hipStream_t q, int device, const uint8_t* data, const BgzfScan& s, uint8_t* devText, uint64_t lastAt, char* lastByte, double& uploadMs, double& kernelMs)
{
	using namespace gcdev;
	const size_t nBlocks = s.blocks.size();
	gc::Arena a;   // the compressed bytes | the block table | the status words and 16 spare bytes
	a.part(s.consumed);
	const size_t oTable = a.part(nBlocks * sizeof(InfBlock)), oStatus = a.part(nBlocks * sizeof(uint32_t) + 16);
	HeldBlock dev(g_readDeviceBlocks, device, q), pin(g_readPinnedBlocks, device, q);
	EventSet<3> ev;
	uint8_t* H = (uint8_t*)pin.acquire(a.bytes());
	uint8_t* D = (uint8_t*)dev.acquire(a.bytes());
	const auto t0 = std::chrono::steady_clock::now();
	memcpy(H, data, s.consumed);
	if (nBlocks) memcpy(H + oTable, s.blocks.data(), nBlocks * sizeof(InfBlock));
	const double stageMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	uint32_t* hostStatus = (uint32_t*)(H + oStatus);
	HIP_CHECK(hipEventRecord(ev[0], q));
	HIP_CHECK(hipMemcpyAsync(D, H, oStatus, hipMemcpyHostToDevice, q));
	HIP_CHECK(hipMemsetAsync(D + oStatus, 0xff, nBlocks * sizeof(uint32_t) + 16, q));
	HIP_CHECK(hipEventRecord(ev[1], q));
	HIP_CHECK(infLaunch(q, D, (const InfBlock*)(D + oTable), (uint32_t)nBlocks, devText, (uint32_t*)(D + oStatus)));
	HIP_CHECK(hipEventRecord(ev[2], q));
	HIP_CHECK(hipMemcpyAsync(hostStatus, D + oStatus, nBlocks * sizeof(uint32_t) + 16, hipMemcpyDeviceToHost, q));
	char* hostLast = (char*)(H + oStatus + nBlocks * sizeof(uint32_t));   // (the 16 spare bytes behind the status words)
	if (lastByte) HIP_CHECK(hipMemcpyAsync(hostLast, devText + lastAt, 1, hipMemcpyDeviceToHost, q));
	HIP_CHECK(hipStreamSynchronize(q));
	uploadMs = stageMs + ev.elapsedMs(0, 1);
	kernelMs = ev.elapsedMs(1, 2);
	for (size_t i = 0; i < nBlocks; i++) if (hostStatus[i] != INF_OK)
		throw InvalidInput("BGZF block " + std::to_string(i) + " at byte " + std::to_string(s.starts[i]) + " " GC_BGZF_REFUSED ": " + infStatusName(hostStatus[i]));
	if (lastByte) *lastByte = *hostLast;
}

} // namespace

int gc_bgzf_inflate(const void* data, uint64_t len, void** out, uint64_t* out_len, uint64_t* consumed)
{
	if (!out || !out_len || !consumed || (!data && len)) return fail(GC_ERR_INVALID, "null argument");
	*out = nullptr; *out_len = 0; *consumed = 0;
	char* text = nullptr;
	int rc = guarded([&]() {
		try {
			BgzfScan s;
			bgzfScan((const uint8_t*)data, len, 0, s);
			text = (char*)malloc(s.textBytes + 1);
			if (!text) throw std::runtime_error("gc_bgzf_inflate: out of host memory");
			text[s.textBytes] = 0;
			if (s.blocks.empty()) { *consumed = 0; return (int)GC_OK; }
			requireDevice();
			int device = 0;
			HIP_CHECK(hipGetDevice(&device));
			hipStream_t q = threadStream(device);
			HeldBlock devText(g_readDeviceBlocks, device, q);
			devText.acquire(s.textBytes + 256);
			double uploadMs = 0, kernelMs = 0;
			bgzfInflateTo(q, device, (const uint8_t*)data, s, (uint8_t*)devText.p, 0, nullptr, uploadMs, kernelMs);
			if (s.textBytes) HIP_CHECK(hipMemcpyAsync(text, devText.p, s.textBytes, hipMemcpyDeviceToHost, q));
			HIP_CHECK(hipStreamSynchronize(q));
			*out_len = s.textBytes; *consumed = s.consumed;
			return (int)GC_OK;
		} catch (const InvalidInput& e) { return fail(GC_ERR_INVALID, std::string("gc_bgzf_inflate: ") + e.what()); }
	});
	if (rc != GC_OK) { free(text); *out_len = 0; *consumed = 0; return rc; }
	*out = text;
	return GC_OK;
}

} // extern "C"

int parseOverBgzf(const char* what, const char* head, uint64_t head_len, const void* data, uint64_t len, const std::function<int(const FxSource&)>& parse,
	char** tail, uint64_t* tail_len, uint64_t* consumed, gc_bgzf_stats* stats)
{
	const std::string name = std::string(what) + ": ";
	BgzfScan s;
	const auto t0 = std::chrono::steady_clock::now();
	try { bgzfScan((const uint8_t*)data, len, head_len, s); }
	catch (const InvalidInput& e) { return fail(GC_ERR_INVALID, name + e.what()); }
	catch (const std::exception& e) { return fail(GC_ERR_INTERNAL, e.what()); }
	const double scanMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	if (head_len >= 0xfffffff0ull || head_len + s.textBytes >= 0xfffffff0ull)
		return fail(GC_ERR_INVALID, name + "the loader uses 32-bit positions: head and inflated text must stay below 2^32 - 16 bytes");
	double uploadMs = 0, kernelMs = 0;
	char* tailMem = nullptr;
	uint64_t tailBytes = 0;
	FxSource src;
	src.len = (uint32_t)(head_len + s.textBytes);
	src.place = [&](char* devText, char* pinnedText, hipStream_t q, int device) {
		if (head_len) { memcpy(pinnedText, head, head_len); HIP_CHECK(hipMemcpyAsync(devText, pinnedText, head_len, hipMemcpyHostToDevice, q)); }
		char last = head_len ? head[head_len - 1] : '\n';
		if (!s.blocks.empty()) {
			try { bgzfInflateTo(q, device, (const uint8_t*)data, s, (uint8_t*)devText, src.len ? src.len - 1 : 0, s.textBytes ? &last : nullptr, uploadMs, kernelMs); }
			catch (const InvalidInput& e) { throw InvalidInput(name + e.what()); }
		}
		return last;
	};
	src.done = [&](const char* devText, uint32_t textConsumed, hipStream_t q) {
		tailBytes = src.len - textConsumed;
		tailMem = (char*)malloc(tailBytes + 1);
		if (!tailMem) throw std::runtime_error(name + "out of host memory");
		if (tailBytes) { HIP_CHECK(hipMemcpyAsync(tailMem, devText + textConsumed, tailBytes, hipMemcpyDeviceToHost, q)); HIP_CHECK(hipStreamSynchronize(q)); }
		tailMem[tailBytes] = 0;
	};
	const int rc = parse(src);
	if (rc != GC_OK) { free(tailMem); return rc; }
	*tail = tailMem; *tail_len = tailBytes; *consumed = s.consumed;
	if (stats) { stats->blocks = s.blocks.size(); stats->inflated_bytes = s.textBytes; stats->scan_ms = scanMs; stats->upload_ms = uploadMs; stats->kernel_ms = kernelMs; }
	return GC_OK;
}

extern "C" {

int gc_reads_parse_bgzf(const char* head, uint64_t head_len, const void* data, uint64_t len, int32_t format, uint32_t flags,
	gc_reads** reads, gc_fastx_table** table, char** tail, uint64_t* tail_len, uint64_t* consumed, gc_bgzf_stats* stats)
{
	if (!reads || !table || !tail || !tail_len || !consumed || (!head && head_len) || (!data && len)) return fail(GC_ERR_INVALID, "null argument");
	*reads = nullptr; *table = nullptr; *tail = nullptr; *tail_len = 0; *consumed = 0;
	if (stats) *stats = gc_bgzf_stats {};
	if (format != GC_FASTX_FASTA && format != GC_FASTX_FASTQ) return fail(GC_ERR_INVALID, "gc_reads_parse_bgzf: format is GC_FASTX_FASTA or GC_FASTX_FASTQ");
	if (flags & ~(uint32_t)GC_FASTX_FINAL) return fail(GC_ERR_INVALID, "gc_reads_parse_bgzf: unknown flag bits");
	return parseOverBgzf("gc_reads_parse_bgzf", head, head_len, data, len, [&](const FxSource& src) { return readsParseFrom(src, format, flags, reads, table); }, tail, tail_len, consumed, stats);
}

} // extern "C"
