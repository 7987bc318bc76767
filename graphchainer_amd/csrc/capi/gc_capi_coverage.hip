// C entry points of the coverage accumulators: gc_coverage_create / _create2 / _destroy, gc_stream_set_coverage, gc_coverage_add_traces, gc_coverage_counts, _link_counts,
// gc_coverage_merge, gc_coverage_format_segments / _bases / _links / _gfa_segments / _gfa_links, and the pileup's gc_coverage_add_traces2, gc_coverage_pileup_counts, gc_coverage_format_pileup. The kernels are in hip/gc_coverage.hip, the per-batch counting in batch/gc_output_encoder.hip (OutputEncoder::choose, countCoverage).
#include "../gc_runtime.hpp"
#include "../hip/gc_coverage_links_core.hpp"

namespace {

// the handle's device for the calling thread while a call works on it, the caller's afterwards
struct OnDevice {
	int before = 0;
	explicit OnDevice(int device) { HIP_CHECK(hipGetDevice(&before)); if (before != device) HIP_CHECK(hipSetDevice(device)); }
	~OnDevice() { int now = 0; if (hipGetDevice(&now) == hipSuccess && now != before) (void)hipSetDevice(before); }
};

void checkFlags(gc_coverage* cov, hipStream_t q)
{
	uint32_t flags = 0;
	HIP_CHECK(hipMemcpyAsync(&flags, cov->dBad, sizeof flags, hipMemcpyDeviceToHost, q));
	HIP_CHECK(hipStreamSynchronize(q));
	if (flags & 1u) throw std::runtime_error("internal: the coverage kernel met a trace cell outside the graph (it was not counted)");
	if (flags & 4u) throw std::runtime_error("internal: the coverage kernel met a node change that is no link of the graph (it was not counted)");
	if (flags & COV_BAD_SEQPOS) throw std::runtime_error("internal: the coverage kernel met a trace cell whose read position lies behind its read (the pileup did not count it)");
}

// The graph's links (include/graphchainer_amd.h): the distinct canonical forms of (nodeIDs[x], nodeIDs[y]) over the out-edges x -> y of the split nodes with different ids,
// ascending. Read from nodeIDs and outNeighbors, which gc_graph_trim_host leaves in place.
std::vector<uint64_t> linkKeysOf(const gc::AlignmentGraph& h)
{
	std::vector<uint64_t> keys;
	for (size_t x = 0; x < h.outNeighbors.size(); x++)
		for (size_t y : h.outNeighbors[x])
			if (h.nodeIDs[x] != h.nodeIDs[y]) keys.push_back(gcdev::covLinkKey((uint32_t)h.nodeIDs[x], (uint32_t)h.nodeIDs[y]));
	std::sort(keys.begin(), keys.end());
	keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
	return keys;
}

} // namespace

extern "C" {

int gc_coverage_create(const gc_graph* G, int per_base, gc_coverage** out) { return gc_coverage_create2(G, per_base ? GC_COVERAGE_PER_BASE : 0, out); }

int gc_coverage_create2(const gc_graph* G, unsigned flags, gc_coverage** out)
{
	if (!G || !out) return fail(GC_ERR_INVALID, "null argument");
	*out = nullptr;
	if (flags & ~(unsigned)(GC_COVERAGE_PER_BASE | GC_COVERAGE_LINKS | GC_COVERAGE_PILEUP)) return fail(GC_ERR_INVALID, "gc_coverage_create2: unknown flag");
	const bool per_base = (flags & (GC_COVERAGE_PER_BASE | GC_COVERAGE_PILEUP)) != 0;   // (the pileup's match column is depth - mismatches - deletions: it implies the depth)
	gc_coverage* cov = new gc_coverage();
	int rc = guarded([&]() {
		requireDevice();
		HIP_CHECK(hipGetDevice(&cov->device));
		const size_t nIds = G->hOrigSize.size(), nSeg = (nIds + 1) / 2;
		cov->graph = G; cov->nIds = (uint32_t)nIds; cov->names = G->devNames;
		cov->segStart.assign(nSeg + 1, 0);
		for (size_t s = 0; s < nSeg; s++) {
			const uint32_t fw = G->hOrigSize[2 * s], bw = 2 * s + 1 < nIds ? G->hOrigSize[2 * s + 1] : 0;
			if (fw && bw && fw != bw) throw std::runtime_error("gc_coverage_create: a segment's two strands differ in length");
			cov->segStart[s + 1] = cov->segStart[s] + (fw ? fw : bw);
		}
		const uint64_t nBases = cov->segStart[nSeg];
		HIP_CHECK(hipMalloc(&cov->dSegStart, (nSeg + 1) * sizeof(uint64_t)));
		HIP_CHECK(hipMemcpy(cov->dSegStart, cov->segStart.data(), (nSeg + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
		HIP_CHECK(hipMalloc((void**)&cov->dBases, std::max<size_t>(1, nSeg) * sizeof(unsigned long long)));
		HIP_CHECK(hipMemset(cov->dBases, 0, std::max<size_t>(1, nSeg) * sizeof(unsigned long long)));
		HIP_CHECK(hipMalloc((void**)&cov->dBad, sizeof(uint32_t)));
		HIP_CHECK(hipMemset(cov->dBad, 0, sizeof(uint32_t)));
		if (per_base) {
			const size_t bytes = std::max<uint64_t>(1, nBases) * sizeof(uint32_t);
			if (hipMalloc((void**)&cov->dDepth, bytes) != hipSuccess) {
				(void)hipGetLastError();
				cov->dDepth = nullptr;
				throw DeviceError("gc_coverage_create: the per-base depth needs " + std::to_string(bytes) + " bytes of device memory (4 per forward base of the graph) and they could not be allocated");
			}
			HIP_CHECK(hipMemset(cov->dDepth, 0, bytes));
		}
		if (flags & GC_COVERAGE_PILEUP) {
			const size_t bytes = std::max<uint64_t>(1, nBases) * 8 * sizeof(uint32_t);
			if (hipMalloc((void**)&cov->dPile, bytes) != hipSuccess) {
				(void)hipGetLastError();
				cov->dPile = nullptr;
				throw DeviceError("gc_coverage_create2: the pileup rows need " + std::to_string(bytes) + " bytes of device memory (32 per forward base of the graph, beside the 4 of the depth) and they could not be allocated");
			}
			HIP_CHECK(hipMemset(cov->dPile, 0, bytes));
		}
		if (flags & GC_COVERAGE_LINKS) {
			cov->linkKeys = linkKeysOf(G->host);
			const size_t n = cov->linkKeys.size(), room = std::max<size_t>(1, n);
			if (hipMalloc((void**)&cov->dLinkKeys, room * sizeof(uint64_t)) != hipSuccess || hipMalloc((void**)&cov->dLinkCounts, room * sizeof(unsigned long long)) != hipSuccess) {
				(void)hipGetLastError();
				throw DeviceError("gc_coverage_create2: the link table needs " + std::to_string(16 * room) + " bytes of device memory (16 per link of the graph) and they could not be allocated");
			}
			if (n) HIP_CHECK(hipMemcpy(cov->dLinkKeys, cov->linkKeys.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice));
			HIP_CHECK(hipMemset(cov->dLinkCounts, 0, room * sizeof(unsigned long long)));
			cov->hasLinks = true;
			cov->links = CovLinks { cov->dLinkKeys, cov->dLinkCounts, (uint64_t)n };
		}
		HIP_CHECK(hipDeviceSynchronize());
		cov->dev = CovGraph { (const uint64_t*)cov->dSegStart, (uint64_t)nSeg, nBases, (uint32_t)nIds };
		return (int)GC_OK;
	});
	if (rc != GC_OK) {
		int current = 0;
		if (hipGetDevice(&current) == hipSuccess && current != cov->device) { (void)hipSetDevice(cov->device); delete cov; (void)hipSetDevice(current); } else delete cov;
		return rc;
	}
	*out = cov;
	return GC_OK;
}

void gc_coverage_destroy(gc_coverage* cov)
{
	if (!cov) return;
	int current = 0;
	const int device = cov->device;
	const bool known = hipGetDevice(&current) == hipSuccess;
	if (known && current != device) (void)hipSetDevice(device);
	delete cov;
	if (known && current != device) (void)hipSetDevice(current);
}

int gc_stream_set_coverage(gc_stream* st, gc_coverage* cov)
{
	if (!st) return fail(GC_ERR_INVALID, "null argument");
	if (cov && cov->device != st->device) return fail(GC_ERR_INVALID, "gc_stream_set_coverage: the handle lives on another device than the stream");
	st->coverage = cov;
	return GC_OK;
}

// gc_coverage_add_traces (seq_pos, bases, read_off null) and gc_coverage_add_traces2
static int addTraces(const char* call, gc_coverage* cov, const int32_t* node, const uint32_t* offset, const uint32_t* seq_pos, const uint64_t* trace_off, uint64_t n_aln, const char* bases, const uint64_t* read_off)
{
	const std::string who = std::string(call) + ": ";
	if (!cov || !trace_off) return fail(GC_ERR_INVALID, "null argument");
	const bool withReads = seq_pos != nullptr || bases != nullptr || read_off != nullptr;
	if (cov->dPile && !read_off) return fail(GC_ERR_INVALID, who + "a handle with the pileup counts traces with their reads (gc_coverage_add_traces2)");
	const uint64_t cellsTotal = trace_off[n_aln];
	if (cellsTotal && (!node || !offset || (withReads && !seq_pos))) return fail(GC_ERR_INVALID, "null argument");
	if (n_aln >= 0xffffffffull) return fail(GC_ERR_INVALID, who + "too many alignments");
	if (trace_off[0] != 0) return fail(GC_ERR_INVALID, who + "trace_off must start at 0");
	for (uint64_t a = 0; a < n_aln; a++) if (trace_off[a + 1] < trace_off[a] || trace_off[a + 1] - trace_off[a] >= (1ull << 32)) return fail(GC_ERR_INVALID, who + "trace_off must ascend, traces below 2^32 cells");
	// every cell against the graph before the kernel indexes anything with it
	const std::vector<uint32_t>& size = cov->graph->hOrigSize;
	for (uint64_t i = 0; i < cellsTotal; i++)
		if (node[i] < 0 || (uint64_t)node[i] >= size.size() || offset[i] >= size[node[i]]) return fail(GC_ERR_INVALID, who + "no such node / offset");
	// with reads: every read position against its read
	uint64_t basesTotal = 0;
	if (withReads) {
		if (!read_off) return fail(GC_ERR_INVALID, "null argument");
		if (read_off[0] != 0) return fail(GC_ERR_INVALID, who + "read_off must start at 0");
		for (uint64_t a = 0; a < n_aln; a++) if (read_off[a + 1] < read_off[a] || read_off[a + 1] - read_off[a] >= (1ull << 32)) return fail(GC_ERR_INVALID, who + "read_off must ascend, reads below 2^32 bases");
		basesTotal = read_off[n_aln];
		if (basesTotal && !bases) return fail(GC_ERR_INVALID, "null argument");
		for (uint64_t a = 0; a < n_aln; a++)
			for (uint64_t i = trace_off[a]; i < trace_off[a + 1]; i++)
				if (seq_pos[i] >= read_off[a + 1] - read_off[a]) return fail(GC_ERR_INVALID, who + "a cell's seq_pos lies behind its read");
	}
	// with links: every node change must leave its segment at the last base (in that orientation), enter the next at offset 0 and be a link of the graph
	if (cov->hasLinks)
		for (uint64_t a = 0; a < n_aln; a++)
			for (uint64_t i = trace_off[a] + 1; i < trace_off[a + 1]; i++) {
				if (node[i] == node[i - 1]) continue;
				if (offset[i - 1] != size[node[i - 1]] - 1 || offset[i] != 0) return fail(GC_ERR_INVALID, who + "a trace changes its node elsewhere than from a segment's last base to the next one's first");
				if (gcdev::covLinkFind(cov->linkKeys.data(), cov->linkKeys.size(), gcdev::covLinkKey((uint32_t)node[i - 1], (uint32_t)node[i])) == cov->linkKeys.size())
					return fail(GC_ERR_INVALID, who + "a trace changes its node along no link of the graph");
			}
	if (n_aln == 0 || cellsTotal == 0) return GC_OK;
	return guarded([&]() {
		requireDevice();
		OnDevice here(cov->device);
		hipStream_t q = threadStream(cov->device);
		std::vector<LongCell> cells(cellsTotal);
		for (uint64_t i = 0; i < cellsTotal; i++) cells[i] = LongCell { node[i], offset[i], withReads ? seq_pos[i] : 0u, 0u };
		std::vector<OutJob> jobs(n_aln);
		for (uint64_t a = 0; a < n_aln; a++)
			jobs[a] = OutJob { trace_off[a], withReads ? read_off[a] : 0, (uint32_t)(trace_off[a + 1] - trace_off[a]), withReads ? (uint32_t)(read_off[a + 1] - read_off[a]) : 0u, 0, 0 };
		DeviceBuffer dCells, dJobs, dReads;
		LongCell* pCells = dCells.reserve<LongCell>(cells.size());
		OutJob* pJobs = dJobs.reserve<OutJob>(n_aln);
		char* pReads = cov->dPile ? dReads.reserve<char>(std::max<uint64_t>(1, basesTotal)) : nullptr;
		HIP_CHECK(hipMemcpyAsync(pCells, cells.data(), cells.size() * sizeof(LongCell), hipMemcpyHostToDevice, q));
		HIP_CHECK(hipMemcpyAsync(pJobs, jobs.data(), n_aln * sizeof(OutJob), hipMemcpyHostToDevice, q));
		if (pReads && basesTotal) HIP_CHECK(hipMemcpyAsync(pReads, bases, basesTotal, hipMemcpyHostToDevice, q));
		launchCoverageAdd(q, cov->dev, cov->links, pJobs, (uint32_t)n_aln, nullptr, pCells, cov->dBases, cov->dDepth, cov->dBad, cov->pileFor(pReads));
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipStreamSynchronize(q));   // (the buffers go when this returns)
		return (int)GC_OK;
	});
}

int gc_coverage_add_traces(gc_coverage* cov, const int32_t* node, const uint32_t* offset, const uint64_t* trace_off, uint64_t n_aln)
{
	return addTraces("gc_coverage_add_traces", cov, node, offset, nullptr, trace_off, n_aln, nullptr, nullptr);
}

int gc_coverage_add_traces2(gc_coverage* cov, const int32_t* node, const uint32_t* offset, const uint32_t* seq_pos, const uint64_t* trace_off, uint64_t n_aln, const char* bases, const uint64_t* read_off)
{
	if (!read_off) return fail(GC_ERR_INVALID, "null argument");
	return addTraces("gc_coverage_add_traces2", cov, node, offset, seq_pos, trace_off, n_aln, bases, read_off);
}

int gc_coverage_pileup_counts(gc_coverage* cov, uint32_t** rows, uint64_t* n_bases)
{
	if (!cov || !rows || !n_bases) return fail(GC_ERR_INVALID, "null argument");
	*rows = nullptr;
	if (!cov->dPile) return fail(GC_ERR_INVALID, "gc_coverage_pileup_counts: the handle was created without the pileup");
	return guarded([&]() {
		requireDevice();
		OnDevice here(cov->device);
		hipStream_t q = threadStream(cov->device);
		checkFlags(cov, q);
		const uint64_t nBases = cov->dev.nBases;
		uint32_t* r = mallocArray<uint32_t>(8 * nBases);
		if (!r) throw std::runtime_error("out of memory");
		struct Free { void* p; ~Free() { free(p); } } gr { r };
		if (nBases) HIP_CHECK(hipMemcpyAsync(r, cov->dPile, 8 * nBases * sizeof(uint32_t), hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipStreamSynchronize(q));
		gr.p = nullptr;
		*rows = r; *n_bases = nBases;
		return (int)GC_OK;
	});
}

int gc_coverage_format_pileup(gc_coverage* cov, uint64_t first_base, uint64_t count, uint64_t min_alt, double min_fraction, char** text, uint64_t* len, uint64_t** line_off, uint64_t* n_lines)
{
	if (!cov || !text || !len) return fail(GC_ERR_INVALID, "null argument");
	*text = nullptr;
	if (line_off) *line_off = nullptr;
	if (!cov->dPile) return fail(GC_ERR_INVALID, "gc_coverage_format_pileup: the handle was created without the pileup");
	if (!(min_fraction >= 0.0 && min_fraction <= 1.0)) return fail(GC_ERR_INVALID, "gc_coverage_format_pileup: min_fraction must lie in [0, 1]");
	if (first_base > cov->dev.nBases) return fail(GC_ERR_INVALID, "the first row lies behind the table's end");
	count = std::min(count, cov->dev.nBases - first_base);
	if (count + 1 >= 0x7fffffffull) return fail(GC_ERR_INVALID, "2^31 rows or more in one call: ask for a smaller range");
	return guarded([&]() {
		requireDevice();
		OnDevice here(cov->device);
		hipStream_t q = threadStream(cov->device);
		checkFlags(cov, q);
		char* t = nullptr; uint64_t l = 0, n = 0; uint64_t* off = nullptr;
		const hipError_t e = coverageFormatPileup(q, cov->dev, cov->graph->dev, cov->names, cov->dDepth, cov->dPile, first_base, count, min_alt, min_fraction, &t, &l, &off, &n);
		if (e == hipErrorInvalidValue) throw std::runtime_error("internal: a range outside the pileup table");
		HIP_CHECK(e);
		*text = t; *len = l;
		if (line_off) *line_off = off; else free(off);
		if (n_lines) *n_lines = n;
		return (int)GC_OK;
	});
}

int gc_coverage_counts(gc_coverage* cov, uint64_t** bases, uint64_t* n_segments, uint32_t** depth, uint64_t* n_bases)
{
	if (!cov || !bases || !n_segments || !depth || !n_bases) return fail(GC_ERR_INVALID, "null argument");
	*bases = nullptr; *depth = nullptr;
	return guarded([&]() {
		requireDevice();
		OnDevice here(cov->device);
		hipStream_t q = threadStream(cov->device);
		checkFlags(cov, q);
		const uint64_t nSeg = cov->dev.nSegments, nBases = cov->dev.nBases;
		uint64_t* b = mallocArray<uint64_t>(nSeg);
		uint32_t* d = cov->dDepth ? mallocArray<uint32_t>(nBases) : nullptr;
		if (!b || (cov->dDepth && !d)) { free(b); free(d); throw std::runtime_error("out of memory"); }
		struct Free { void* p; ~Free() { free(p); } } gb { b }, gd { d };
		static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "64-bit counts");
		if (nSeg) HIP_CHECK(hipMemcpyAsync(b, cov->dBases, nSeg * sizeof(uint64_t), hipMemcpyDeviceToHost, q));
		if (d && nBases) HIP_CHECK(hipMemcpyAsync(d, cov->dDepth, nBases * sizeof(uint32_t), hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipStreamSynchronize(q));
		gb.p = nullptr; gd.p = nullptr;
		*bases = b; *n_segments = nSeg; *depth = d; *n_bases = nBases;
		return (int)GC_OK;
	});
}

int gc_coverage_link_counts(gc_coverage* cov, int32_t** from, int32_t** to, uint64_t** traversals, uint64_t* n_links)
{
	if (!cov || !from || !to || !traversals || !n_links) return fail(GC_ERR_INVALID, "null argument");
	*from = nullptr; *to = nullptr; *traversals = nullptr;
	if (!cov->hasLinks) return fail(GC_ERR_INVALID, "gc_coverage_link_counts: the handle was created without links");
	return guarded([&]() {
		requireDevice();
		OnDevice here(cov->device);
		hipStream_t q = threadStream(cov->device);
		checkFlags(cov, q);
		const uint64_t n = cov->linkKeys.size();
		int32_t* f = mallocArray<int32_t>(n);
		int32_t* t = mallocArray<int32_t>(n);
		uint64_t* c = mallocArray<uint64_t>(n);
		struct Free { void* p; ~Free() { free(p); } } gf { f }, gt { t }, gc { c };
		if (!f || !t || !c) throw std::runtime_error("out of memory");
		for (uint64_t i = 0; i < n; i++) { f[i] = (int32_t)gcdev::covLinkFrom(cov->linkKeys[i]); t[i] = (int32_t)gcdev::covLinkTo(cov->linkKeys[i]); }
		if (n) HIP_CHECK(hipMemcpyAsync(c, cov->dLinkCounts, n * sizeof(uint64_t), hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipStreamSynchronize(q));
		gf.p = nullptr; gt.p = nullptr; gc.p = nullptr;
		*from = f; *to = t; *traversals = c; *n_links = n;
		return (int)GC_OK;
	});
}

int gc_coverage_merge(gc_coverage* dst, const gc_coverage* src)
{
	if (!dst || !src) return fail(GC_ERR_INVALID, "null argument");
	if (dst == src) return fail(GC_ERR_INVALID, "gc_coverage_merge: a handle cannot be merged into itself");
	if (dst->segStart != src->segStart || dst->nIds != src->nIds) return fail(GC_ERR_INVALID, "gc_coverage_merge: the handles were made for graphs of different shape");
	if ((dst->dDepth != nullptr) != (src->dDepth != nullptr)) return fail(GC_ERR_INVALID, "gc_coverage_merge: one handle counts per base and the other does not");
	if (dst->hasLinks != src->hasLinks) return fail(GC_ERR_INVALID, "gc_coverage_merge: one handle counts links and the other does not");
	if ((dst->dPile != nullptr) != (src->dPile != nullptr)) return fail(GC_ERR_INVALID, "gc_coverage_merge: one handle counts the pileup and the other does not");
	if (dst->linkKeys != src->linkKeys) return fail(GC_ERR_INVALID, "gc_coverage_merge: the handles were made for graphs of different shape");
	return guarded([&]() {
		requireDevice();
		OnDevice here(dst->device);
		hipStream_t q = threadStream(dst->device);
		const uint64_t nSeg = dst->dev.nSegments, nDepth = dst->dDepth ? dst->dev.nBases : 0, nLinks = dst->linkKeys.size();
		uint32_t srcFlags = 0;
		if (src->device == dst->device) {
			HIP_CHECK(hipMemcpyAsync(&srcFlags, src->dBad, sizeof srcFlags, hipMemcpyDeviceToHost, q));
			launchCoverageMerge(q, dst->dBases, src->dBases, nSeg, dst->dDepth, src->dDepth, nDepth, dst->dLinkCounts, src->dLinkCounts, nLinks);
			if (dst->dPile) launchCoverageMerge(q, nullptr, nullptr, 0, dst->dPile, src->dPile, 8 * dst->dev.nBases);   // the rows: 32-bit words that stop at 2^32 - 1, as the depth's
			HIP_CHECK(hipGetLastError());
			HIP_CHECK(hipStreamSynchronize(q));
		} else {
			// two devices: through the host, the depth in slices so that neither side holds a second copy of it
			const uint64_t slice = 64ull << 20;   // words
			std::vector<unsigned long long> hBases(std::max<uint64_t>(1, nSeg)), hLinks(std::max<uint64_t>(1, nLinks));
			std::vector<uint32_t> hDepth(std::max<uint64_t>(1, std::min(slice, dst->dPile ? 8 * dst->dev.nBases : nDepth)));
			DeviceBuffer dBases, dDepth, dLinks;
			unsigned long long* pBases = dBases.reserve<unsigned long long>(nSeg);
			unsigned long long* pLinks = dLinks.reserve<unsigned long long>(nLinks);
			uint32_t* pDepth = dDepth.reserve<uint32_t>(hDepth.size());
			{
				OnDevice there(src->device);
				HIP_CHECK(hipMemcpy(&srcFlags, src->dBad, sizeof srcFlags, hipMemcpyDeviceToHost));
				if (nSeg) HIP_CHECK(hipMemcpy(hBases.data(), src->dBases, nSeg * sizeof(unsigned long long), hipMemcpyDeviceToHost));
				if (nLinks) HIP_CHECK(hipMemcpy(hLinks.data(), src->dLinkCounts, nLinks * sizeof(unsigned long long), hipMemcpyDeviceToHost));
			}
			if (nSeg) HIP_CHECK(hipMemcpyAsync(pBases, hBases.data(), nSeg * sizeof(unsigned long long), hipMemcpyHostToDevice, q));
			if (nLinks) HIP_CHECK(hipMemcpyAsync(pLinks, hLinks.data(), nLinks * sizeof(unsigned long long), hipMemcpyHostToDevice, q));
			launchCoverageMerge(q, dst->dBases, pBases, nSeg, nullptr, nullptr, 0, dst->dLinkCounts, pLinks, nLinks);
			HIP_CHECK(hipStreamSynchronize(q));
			auto mergeWords = [&](uint32_t* dstWords, const uint32_t* srcWords, uint64_t nWords) {
				for (uint64_t at = 0; at < nWords; at += slice) {
					const uint64_t m = std::min(slice, nWords - at);
					{
						OnDevice there(src->device);
						HIP_CHECK(hipMemcpy(hDepth.data(), srcWords + at, m * sizeof(uint32_t), hipMemcpyDeviceToHost));
					}
					HIP_CHECK(hipMemcpyAsync(pDepth, hDepth.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice, q));
					launchCoverageMerge(q, nullptr, nullptr, 0, dstWords + at, pDepth, m);
					HIP_CHECK(hipGetLastError());
					HIP_CHECK(hipStreamSynchronize(q));
				}
			};
			mergeWords(dst->dDepth, src->dDepth, nDepth);
			if (dst->dPile) mergeWords(dst->dPile, src->dPile, 8 * dst->dev.nBases);   // (the rows through the same slices)
		}
		if (srcFlags & 1u) throw std::runtime_error("internal: the merged handle's kernel met a trace cell outside the graph (it was not counted)");
		if (srcFlags & 4u) throw std::runtime_error("internal: the merged handle's kernel met a node change that is no link of the graph (it was not counted)");
		if (srcFlags & COV_BAD_SEQPOS) throw std::runtime_error("internal: the merged handle's kernel met a trace cell whose read position lies behind its read (the pileup did not count it)");
		return (int)GC_OK;
	});
}

static int formatTable(gc_coverage* cov, bool perBase, char** text, uint64_t* len, uint64_t** line_off, uint64_t* n_lines)
{
	if (!cov || !text || !len) return fail(GC_ERR_INVALID, "null argument");
	if (perBase && !cov->dDepth) return fail(GC_ERR_INVALID, "gc_coverage_format_bases: the handle was created without per-base depth");
	*text = nullptr;
	if (line_off) *line_off = nullptr;
	return guarded([&]() {
		requireDevice();
		OnDevice here(cov->device);
		hipStream_t q = threadStream(cov->device);
		checkFlags(cov, q);
		char* t = nullptr; uint64_t l = 0, n = 0; uint64_t* off = nullptr;
		const hipError_t e = perBase ? coverageFormatBases(q, cov->dev, cov->names, cov->dDepth, cov->dBad, &t, &l, &off, &n)
		                             : coverageFormatSegments(q, cov->dev, cov->names, cov->dBases, &t, &l, &off, &n);
		if (e == hipErrorInvalidValue) throw std::runtime_error("internal: the coverage tables' counting and placing passes disagree, or a table has 2^31 lines or more");
		HIP_CHECK(e);
		*text = t; *len = l;
		if (line_off) *line_off = off; else free(off);
		if (n_lines) *n_lines = n;
		return (int)GC_OK;
	});
}

int gc_coverage_format_segments(gc_coverage* cov, char** text, uint64_t* len, uint64_t** line_off, uint64_t* n_lines) { return formatTable(cov, false, text, len, line_off, n_lines); }
int gc_coverage_format_bases(gc_coverage* cov, char** text, uint64_t* len, uint64_t** line_off, uint64_t* n_lines) { return formatTable(cov, true, text, len, line_off, n_lines); }

// kind 0: the link table, 1: the GFA's S lines, 2: its L lines
static int formatRows(gc_coverage* cov, int kind, uint64_t first, uint64_t count, int supported_only, char** text, uint64_t* len, uint64_t** line_off, uint64_t* n_lines)
{
	if (!cov || !text || !len) return fail(GC_ERR_INVALID, "null argument");
	*text = nullptr;
	if (line_off) *line_off = nullptr;
	if (kind != 1 && !cov->hasLinks) return fail(GC_ERR_INVALID, "the handle was created without links");
	const uint64_t rows = kind == 1 ? cov->dev.nSegments : cov->linkKeys.size();
	if (first > rows) return fail(GC_ERR_INVALID, "the first row lies behind the table's end");
	count = std::min(count, rows - first);
	if (count + 1 >= 0x7fffffffull) return fail(GC_ERR_INVALID, "2^31 rows or more in one call: ask for a smaller range");
	return guarded([&]() {
		requireDevice();
		OnDevice here(cov->device);
		hipStream_t q = threadStream(cov->device);
		checkFlags(cov, q);
		char* t = nullptr; uint64_t l = 0, n = 0; uint64_t* off = nullptr;
		const hipError_t e = kind == 0 ? coverageFormatLinks(q, cov->names, cov->links, first, count, &t, &l, &off, &n)
		                   : kind == 1 ? coverageFormatGfaSegments(q, cov->dev, cov->graph->dev, cov->names, cov->dBases, cov->dBad, first, count, supported_only != 0, &t, &l, &off, &n)
		                               : coverageFormatGfaLinks(q, cov->names, cov->links, first, count, supported_only != 0, &t, &l, &off, &n);
		if (e == hipErrorInvalidValue) throw std::runtime_error("internal: a range outside the table, or a segment's line of 2^32 bytes or more");
		HIP_CHECK(e);
		*text = t; *len = l;
		if (line_off) *line_off = off; else free(off);
		if (n_lines) *n_lines = n;
		return (int)GC_OK;
	});
}

int gc_coverage_format_links(gc_coverage* cov, uint64_t first, uint64_t count, char** text, uint64_t* len, uint64_t** line_off, uint64_t* n_lines) { return formatRows(cov, 0, first, count, 0, text, len, line_off, n_lines); }
int gc_coverage_format_gfa_segments(gc_coverage* cov, uint64_t first, uint64_t count, int supported_only, char** text, uint64_t* len, uint64_t** line_off, uint64_t* n_lines) { return formatRows(cov, 1, first, count, supported_only, text, len, line_off, n_lines); }
int gc_coverage_format_gfa_links(gc_coverage* cov, uint64_t first, uint64_t count, int supported_only, char** text, uint64_t* len, uint64_t** line_off, uint64_t* n_lines) { return formatRows(cov, 2, first, count, supported_only, text, len, line_off, n_lines); }

} // extern "C"
