// The C entry points of include/graphchainer_amd.h except gc_align_batch (gc_batch.hip): graphs, seeders, index cache, read batches, streams, edit distances, output formats.
#include "gc_runtime.hpp"
#include "host/gc_stageclock.hpp"
#include "hip/gc_seedhits_core.hpp"
#include "hip/gc_fastx_core.hpp"
#include "hip/gc_inflate_core.hpp"
#include "host/gc_seedfile_frame.hpp"
#include <malloc.h>
#include <zlib.h>

extern "C" {

const char* gc_last_error(void) { return g_lastError.c_str(); }
void gc_free(void* p) { free(p); }

// Global (NW) edit distances of n_pairs string pairs on the GPU: what edlibAlign(a, b, EDLIB_MODE_NW, EDLIB_TASK_DISTANCE)
// returns at src/Aligner.cpp:645,845.
int gc_edit_distance(const char* a, const uint64_t* a_off, const char* b, const uint64_t* b_off, uint64_t n_pairs, int64_t* out)
{
	if ((!a && n_pairs) || !a_off || (!b && n_pairs) || !b_off || !out) return fail(GC_ERR_INVALID, "null argument");
	return guarded([&]() {
		requireDevice();
		if (n_pairs == 0) return (int)GC_OK;
		if (n_pairs >= 0xffffffffull) throw std::runtime_error("too many pairs");
		const uint64_t aBytes = a_off[n_pairs], bBytes = b_off[n_pairs];
		std::vector<EdRead> reads(n_pairs);
		uint64_t words = 0;
		for (uint64_t i = 0; i < n_pairs; i++) {
			uint64_t len = b_off[i + 1] - b_off[i];
			if (len >= 0x7fffffffull || a_off[i + 1] - a_off[i] >= 0x7fffffffull) throw std::runtime_error("sequence too long");
			reads[i] = EdRead { b_off[i], words, (uint32_t)len, (uint32_t)((len + 63) / 64 + 1) };
			words += 4ull * reads[i].words;
		}
		std::vector<uint64_t> masks(words, 0);
		for (uint64_t i = 0; i < n_pairs; i++) buildEqMasks(b + b_off[i], reads[i].len, reads[i].words, masks.data() + reads[i].eqOff);
		const gc::Switches sw = gc::Switches::fromEnvironment();
		std::vector<EdPair> pairs(n_pairs);
		for (uint64_t i = 0; i < n_pairs; i++) {
			uint32_t m = (uint32_t)(a_off[i + 1] - a_off[i]);
			pairs[i] = EdPair { a_off[i], m, 0, (uint32_t)i, std::max<uint32_t>(64, (m + reads[i].len) / 16) };
			if (sw.edFirstK) pairs[i].k = *sw.edFirstK;   // test hook: the first band, as small as a whole-read alignment's own bound (score + clipped ends + 8)
		}
		DeviceBuffer dA, dB, dMasks, dReads, dPairs, dOut;
		char* pa = dA.reserve<char>(aBytes); char* pb = dB.reserve<char>(bBytes);
		uint64_t* pm = dMasks.reserve<uint64_t>(words);
		EdRead* pr = dReads.reserve<EdRead>(n_pairs);
		EdPair* pp = dPairs.reserve<EdPair>(n_pairs);
		int64_t* po = dOut.reserve<int64_t>(n_pairs);
		if (aBytes) HIP_CHECK(hipMemcpy(pa, a, aBytes, hipMemcpyHostToDevice));
		if (bBytes) HIP_CHECK(hipMemcpy(pb, b, bBytes, hipMemcpyHostToDevice));
		if (words) HIP_CHECK(hipMemcpy(pm, masks.data(), words * sizeof(uint64_t), hipMemcpyHostToDevice));
		HIP_CHECK(hipMemcpy(pr, reads.data(), n_pairs * sizeof(EdRead), hipMemcpyHostToDevice));
		EditDistanceRun run;
		auto readLenOf = [&](uint32_t r) { return reads[r].len; };
		launchEditDistances(run, nullptr, pairs.data(), out, (uint32_t)n_pairs, pp, po, pr, pb, pm, pa, nullptr, readLenOf, sw.debugTimes);
		finishEditDistances(run, nullptr, pairs.data(), out, (uint32_t)n_pairs, pp, po, pr, pb, pm, pa, nullptr, sw.debugTimes);
		return (int)GC_OK;
	});
}

// The alignment path edlib returns for EDLIB_TASK_PATH (src/Aligner.cpp:845), for arbitrary string pairs: k_edit_distance for the
// distance, k_edit_path for the ops. Rows = a (the reference passes the path letters first), columns = b (the read).
int gc_edit_path(const char* a, const uint64_t* a_off, const char* b, const uint64_t* b_off, uint64_t n_pairs, const uint64_t* ops_off, uint8_t* ops, uint32_t* ops_len, int64_t* distance)
{
	if ((!a && n_pairs) || !a_off || (!b && n_pairs) || !b_off || !ops_off || !ops || !ops_len || !distance) return fail(GC_ERR_INVALID, "null argument");
	int rc = gc_edit_distance(a, a_off, b, b_off, n_pairs, distance);
	if (rc != GC_OK) return rc;
	return guarded([&]() {
		if (n_pairs == 0) return (int)GC_OK;
		const uint64_t aBytes = a_off[n_pairs], bBytes = b_off[n_pairs];
		std::vector<EdPathJob> jobs(n_pairs);
		uint32_t maxQ = 1, maxT = 1;
		uint64_t opsEnd = 0;
		for (uint64_t i = 0; i < n_pairs; i++) {
			const uint32_t q = (uint32_t)(a_off[i + 1] - a_off[i]), t = (uint32_t)(b_off[i + 1] - b_off[i]);
			jobs[i] = EdPathJob { a_off[i], b_off[i], ops_off[i], q, t, (int32_t)distance[i], 0 };
			maxQ = std::max(maxQ, q); maxT = std::max(maxT, t);
			opsEnd = std::max<uint64_t>(opsEnd, ops_off[i] + q + t);
		}
		DeviceBuffer dA, dB, dJobs, dOps, dLen, dScratch;
		char* pa = dA.reserve<char>(aBytes); char* pb = dB.reserve<char>(bBytes);
		EdPathJob* pj = dJobs.reserve<EdPathJob>(n_pairs);
		uint8_t* po = dOps.reserve<uint8_t>(opsEnd);
		uint32_t* pl = dLen.reserve<uint32_t>(n_pairs);
		uint8_t* ps = dScratch.reserve<uint8_t>((uint64_t)editPathGridBlocks((uint32_t)n_pairs) * editPathScratchBytes(maxQ, maxT));
		if (aBytes) HIP_CHECK(hipMemcpy(pa, a, aBytes, hipMemcpyHostToDevice));
		if (bBytes) HIP_CHECK(hipMemcpy(pb, b, bBytes, hipMemcpyHostToDevice));
		HIP_CHECK(hipMemcpy(pj, jobs.data(), n_pairs * sizeof(EdPathJob), hipMemcpyHostToDevice));
		launchEditPath(nullptr, pj, (uint32_t)n_pairs, pa, pb, ps, maxQ, maxT, po, pl);
		HIP_CHECK(hipDeviceSynchronize());
		HIP_CHECK(hipMemcpy(ops_len, pl, n_pairs * sizeof(uint32_t), hipMemcpyDeviceToHost));
		if (opsEnd) HIP_CHECK(hipMemcpy(ops, po, opsEnd, hipMemcpyDeviceToHost));
		return (int)GC_OK;
	});
}

// E-value model of --E-cutoff (host only): out2 = {alignment score, E-value}; what SelectECutoff compares with the cut-off
// (src/AlignmentSelection.cpp:91-99, src/EValue.cpp:35-48).
int gc_evalue(double min_identity, uint64_t database_size, uint64_t query_size, uint64_t alignment_length, uint64_t num_edits, double* out2)
{
	if (!out2) return fail(GC_ERR_INVALID, "null argument");
	gc::EValueModel model(min_identity);
	out2[0] = model.alignmentScore(alignment_length, num_edits);
	out2[1] = model.evalue(database_size, query_size, alignment_length, num_edits);
	return GC_OK;
}

// Output of a batch's final alignments in the reference's formats (src/Aligner.cpp:1003-1023: the read's list sorted by
// alignmentStart, AddAlignment / AddGAFLine per alignment, sorted again; writeGAMToQueue :261-281, writeJSONToQueue :283-298,
// writeGAFToQueue :300-311). Needs a result produced with long_pass, keep_traces and edit_distances; a read whose chained
// alignment won (chained_better) is written from its chain_trace_* arrays (chain_traces >= 1), and counted as skipped only
// when the result carries no trace for it.
enum OutputKind { OUT_GAF, OUT_JSON, OUT_GAM };

// GC_GAM_DEVICE_HUFFMAN: every non-empty element of `groups` (a read's uncompressed group) becomes its gzip member, deflated on the device (hip/gc_deflate.hip: one
// dynamic-Huffman block of literals per read). The host stages the bytes in pinned memory, frames the members and computes their CRC-32s.
static void gzipGroupsOnDevice(std::vector<std::string>& groups, bool skipEmpty = true, bool lz = false)   // lz (r6, GC_GAM_DEVICE_LZ): LZ77 matches in front of the Huffman stage
{
	std::vector<uint32_t> which;
	std::vector<uint64_t> rawOff { 0 };
	for (size_t i = 0; i < groups.size(); i++) if (!skipEmpty || !groups[i].empty()) { which.push_back((uint32_t)i); rawOff.push_back(rawOff.back() + groups[i].size()); }
	const size_t m = which.size();
	if (!m) return;
	const uint64_t rawTotal = rawOff.back();
	requireDevice();
	int device = 0;
	HIP_CHECK(hipGetDevice(&device));
	const uint64_t outBound = rawTotal + 5 * (rawTotal / 65535 + m) + 4 * m;   // stored blocks are the worst case the plan accepts; 4-byte placement
	size_t at = 0;
	auto part = [&](size_t bytes) { const size_t here = at; at += (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255; return here; };
	const size_t oRaw = part(rawTotal), oRawOff = part((m + 1) * sizeof(uint64_t)), oLens = part(m * (size_t)std::max(260u, deflateLzLensStride())), oPlan = part(m * sizeof(uint2)), oOutOff = part((m + 1) * sizeof(uint64_t)), oOut = part(outBound);
	size_t deviceBytes = 0, pinnedBytes = 0;
	hipStream_t q = threadStream(device);
	// (the guards wait for the stream before a block goes back to its cache: on an exception between a launch and the wait below the block would otherwise be handed to the next caller
	// while this thread's copies and kernels still use it - ADVICE r4)
	char* D = (char*)g_deflateDeviceBlocks.get(at, device, deviceBytes);
	struct DeviceReturn { char* p; size_t bytes; int device; hipStream_t q; ~DeviceReturn() { (void)hipStreamSynchronize(q); g_deflateDeviceBlocks.put(p, bytes, device); } } deviceReturn { D, deviceBytes, device, q };
	size_t hat = 0;
	auto hpart = [&](size_t bytes) { const size_t here = hat; hat += (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255; return here; };
	const size_t hRaw = hpart(std::max<uint64_t>(rawTotal, outBound)), hRawOff = hpart((m + 1) * sizeof(uint64_t)), hPlan = hpart(m * sizeof(uint2)), hOutOff = hpart((m + 1) * sizeof(uint64_t));
	char* H = (char*)g_deflatePinnedBlocks.get(hat, device, pinnedBytes);
	struct PinnedReturn { char* p; size_t bytes; int device; hipStream_t q; ~PinnedReturn() { (void)hipStreamSynchronize(q); g_deflatePinnedBlocks.put(p, bytes, device); } } pinnedReturn { H, pinnedBytes, device, q };
	WorkerPool::instance().run(m, [&](size_t k, size_t) { memcpy(H + hRaw + rawOff[k], groups[which[k]].data(), groups[which[k]].size()); });
	memcpy(H + hRawOff, rawOff.data(), (m + 1) * sizeof(uint64_t));
	if (rawTotal) HIP_CHECK(hipMemcpyAsync(D + oRaw, H + hRaw, rawTotal, hipMemcpyHostToDevice, q));
	HIP_CHECK(hipMemcpyAsync(D + oRawOff, H + hRawOff, (m + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, q));
	(lz ? launchDeflateLzPlan : launchDeflatePlan)(q, (const uint8_t*)(D + oRaw), (const uint64_t*)(D + oRawOff), (uint32_t)m, (uint8_t*)(D + oLens), (uint2*)(D + oPlan));
	HIP_CHECK(hipMemcpyAsync(H + hPlan, D + oPlan, m * sizeof(uint2), hipMemcpyDeviceToHost, q));
	HIP_CHECK(hipStreamSynchronize(q));
	const uint2* plan = (const uint2*)(H + hPlan);
	uint64_t* outOff = (uint64_t*)(H + hOutOff);
	outOff[0] = 0;
	for (size_t k = 0; k < m; k++) outOff[k + 1] = outOff[k] + (((uint64_t)plan[k].x + 3) & ~(uint64_t)3);
	if (outOff[m] > outBound) throw std::runtime_error("device deflate: planned sizes exceed the bound");
	HIP_CHECK(hipMemcpyAsync(D + oOutOff, outOff, (m + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, q));
	(lz ? launchDeflateLzWrite : launchDeflateWrite)(q, (const uint8_t*)(D + oRaw), (const uint64_t*)(D + oRawOff), (uint32_t)m, (const uint8_t*)(D + oLens), (const uint2*)(D + oPlan), (uint8_t*)(D + oOut), (const uint64_t*)(D + oOutOff));
	HIP_CHECK(hipMemcpyAsync(H + hRaw, D + oOut, outOff[m], hipMemcpyDeviceToHost, q));
	HIP_CHECK(hipStreamSynchronize(q));
	WorkerPool::instance().run(m, [&](size_t k, size_t) { std::string& g = groups[which[k]]; g = gc::gzipMember((const uint8_t*)(H + hRaw + outOff[k]), plan[k].x, g); });
}

static int formatBatch(const gc_graph* G, const gc_result* r, const char* const* read_names, const char* bases, const uint64_t* offsets, OutputKind kind, int cigar_match_mismatch_merge,
	char** out_text, uint64_t* out_len, uint64_t* n_chained_skipped, int gamLevel = -1)
{
	if (!G || !r || !read_names || !offsets || !out_text || !out_len) return fail(GC_ERR_INVALID, "null argument");
	const bool pieces = r->read_out_off != nullptr;   // the result carries the alignments as the device encoded them (gc_params::device_output)
	if (pieces) {
		// the pieces' CIGAR style (= / X or M) was fixed when the batch was aligned (device_output bit 0 / 1); a call that asks for the other style would get the device's pieces in one
		// style and the chained winners' lines (encoded here, on the host) in the other: refused
		if (kind == OUT_GAF && (r->device_output & 3) && ((r->device_output & 2) != 0) != (cigar_match_mismatch_merge != 0))
			return fail(GC_ERR_INVALID, "gc_format_gaf: cigar_match_mismatch_merge differs from the style the result's pieces were encoded in (gc_params::device_output 1: = / X, 2: M)");
		if (kind == OUT_GAF && !r->out_cigar_off) return fail(GC_ERR_INVALID, "the result holds no GAF pieces");
		if (kind == OUT_GAF && r->out_cigar_off[r->read_out_off[r->n_reads]] == 0 && r->out_vg_off[r->read_out_off[r->n_reads]] != 0) return fail(GC_ERR_INVALID, "the result was produced without the GAF pieces (gc_params::device_output & 3)");
		if (kind != OUT_GAF && r->out_vg_off[r->read_out_off[r->n_reads]] == 0 && r->out_cigar_off[r->read_out_off[r->n_reads]] != 0) return fail(GC_ERR_INVALID, "the result was produced without the vg::Path bytes (gc_params::device_output & 4)");
	}
	if (!pieces && (!r->long_trace_off || !r->read_long_off || !r->long_index)) return fail(GC_ERR_INVALID, "the output encoders need a result with long_pass, keep_traces and edit_distances");
	return guarded([&]() {
		const uint64_t n = r->n_reads;
		std::vector<std::string> perRead(n);
		std::atomic<uint64_t> skipped { 0 };
		const bool onDevice = gamLevel == GC_GAM_DEVICE_HUFFMAN || gamLevel == GC_GAM_DEVICE_LZ;
		auto group = [&](const std::vector<std::string>& messages) { return onDevice ? gc::gamGroupRaw(messages) : gc::gamGroup(messages, gamLevel); };
		WorkerPool::instance().run(n, [&](size_t i, size_t) {
			std::string& text = perRead[i];
			std::vector<std::string> messages;
			const std::string name = read_names[i] ? read_names[i] : "";
			const uint64_t len = offsets[i + 1] - offsets[i];
			if (pieces && !r->chained_better[i]) {
				// put together from what the device wrote: the path and CIGAR columns, or the vg::Path bytes, plus the numbers of the other columns / fields
				for (uint64_t e = r->read_out_off[i]; e < r->read_out_off[i + 1]; e++) {
					const uint64_t* num = r->out_numbers + 12 * e;
					gc::EncodedAlignment ea;
					ea.nodePathLen = num[0]; ea.nodePathStart = num[1]; ea.nodePathEnd = num[2]; ea.matches = num[3]; ea.mismatches = num[4]; ea.insertions = num[5]; ea.deletions = num[6];
					ea.cells = num[7]; ea.alignmentStart = num[8]; ea.alignmentEnd = num[9]; ea.score = (int32_t)num[11];
					if (kind == OUT_GAF) {
						ea.path = r->out_path_text + r->out_path_off[e]; ea.pathLen = r->out_path_off[e + 1] - r->out_path_off[e];
						ea.cigar = r->out_cigar_text + r->out_cigar_off[e]; ea.cigarLen = r->out_cigar_off[e + 1] - r->out_cigar_off[e];
						gc::appendGafLine(text, name, len, ea);
						text += '\n';
					} else {
						ea.vgPath = r->out_vg_path + r->out_vg_off[e]; ea.vgPathLen = r->out_vg_off[e + 1] - r->out_vg_off[e];
						if (kind == OUT_JSON) { text += gc::vgToJson(gc::vgFromEncoded(name, bases + offsets[i], ea)); text += '\n'; }
						else messages.push_back(gc::vgProtobufFromEncoded(name, bases + offsets[i], ea));
					}
				}
				if (kind == OUT_GAM && !messages.empty()) text = group(messages);
				return;
			}
			if (r->chained_better[i]) {
				// the chained alignment replaces the whole-read ones (src/Aligner.cpp:901-920): a single item, trace score 0
				const uint64_t t0 = r->read_chain_trace_off ? r->read_chain_trace_off[i] : 0, t1 = r->read_chain_trace_off ? r->read_chain_trace_off[i + 1] : 0;
				if (t1 == t0) { skipped++; return; }   // result produced without chain_traces
				gc::TraceView tv { r->chain_trace_node + t0, r->chain_trace_offset + t0, r->chain_trace_seqpos + t0, r->chain_trace_switch + t0, t1 - t0 };
				if (kind == OUT_GAF) {
					text += gc::formatGafLine(G->host, name, bases + offsets[i], len, tv, cigar_match_mismatch_merge != 0);
					text += '\n';
				} else {
					gc::VgAlignment aln = gc::buildVgAlignment(G->host, name, bases + offsets[i], len, tv, 0, r->chain_aln_start[i], r->chain_aln_end[i]);
					if (kind == OUT_JSON) { text += gc::vgToJson(aln); text += '\n'; }
					else text = group({ gc::vgToProtobuf(aln) });
				}
				return;
			}
			if (pieces) return;   // (a read without alignments)
			struct Item { uint32_t start; uint64_t aln; };
			std::vector<Item> items;
			for (uint64_t k = r->read_long_off[i]; k < r->read_long_off[i + 1]; k++) {
				uint64_t a = r->read_longall_off[i] + r->long_index[k];
				items.push_back(Item { r->longall_start[a], a });
			}
			if (items.empty()) return;
			auto byStart = [](const Item& l, const Item& rr) { return l.start < rr.start; };
			std::sort(items.begin(), items.end(), byStart);   // src/Aligner.cpp:1003
			std::sort(items.begin(), items.end(), byStart);   // :1023 (an unstable sort may move ties even in a sorted list)
			for (const Item& it : items) {
				uint64_t t0 = r->long_trace_off[it.aln], t1 = r->long_trace_off[it.aln + 1];
				gc::TraceView tv { r->long_trace_node + t0, r->long_trace_offset + t0, r->long_trace_seqpos + t0, r->long_trace_switch + t0, t1 - t0 };
				if (kind == OUT_GAF) {
					text += gc::formatGafLine(G->host, name, bases + offsets[i], len, tv, cigar_match_mismatch_merge != 0);
					text += '\n';
				} else {
					gc::VgAlignment aln = gc::buildVgAlignment(G->host, name, bases + offsets[i], len, tv, (int32_t)r->longall_score[it.aln], r->longall_start[it.aln], r->longall_end[it.aln]);
					if (kind == OUT_JSON) { text += gc::vgToJson(aln); text += '\n'; }
					else messages.push_back(gc::vgToProtobuf(aln));
				}
			}
			if (kind == OUT_GAM) text = group(messages);
		});
		if (kind == OUT_GAM && onDevice) gzipGroupsOnDevice(perRead, true, gamLevel == GC_GAM_DEVICE_LZ);
		uint64_t total = 0;
		for (const auto& t : perRead) total += t.size();
		char* buf = (char*)malloc(total + 1);
		if (!buf) throw std::runtime_error("out of memory");
		uint64_t at = 0;
		for (const auto& t : perRead) { memcpy(buf + at, t.data(), t.size()); at += t.size(); }
		buf[total] = 0;
		*out_text = buf;
		*out_len = total;
		if (n_chained_skipped) *n_chained_skipped = skipped.load();
		return (int)GC_OK;
	});
}

int gc_format_gaf(const gc_graph* G, const gc_result* r, const char* const* read_names, const char* bases, const uint64_t* offsets, int cigar_match_mismatch_merge,
	char** out_text, uint64_t* out_len, uint64_t* n_chained_skipped)
{
	return formatBatch(G, r, read_names, bases, offsets, OUT_GAF, cigar_match_mismatch_merge, out_text, out_len, n_chained_skipped);
}
int gc_format_json(const gc_graph* G, const gc_result* r, const char* const* read_names, const char* bases, const uint64_t* offsets, char** out_text, uint64_t* out_len, uint64_t* n_chained_skipped)
{
	return formatBatch(G, r, read_names, bases, offsets, OUT_JSON, 0, out_text, out_len, n_chained_skipped);
}
int gc_format_gam(const gc_graph* G, const gc_result* r, const char* const* read_names, const char* bases, const uint64_t* offsets, char** out_bytes, uint64_t* out_len, uint64_t* n_chained_skipped)
{
	// r6: without a level the members are deflated on the device with LZ77 matches (GC_GAM_DEVICE_LZ): the inflated stream is the contract - the reference's own bytes depend on its
	// zlib build - and zlib's default level on the host is a fifth of the hot path's rate (gc_format_gam_level(-1) still gives it)
	return formatBatch(G, r, read_names, bases, offsets, OUT_GAM, 0, out_bytes, out_len, n_chained_skipped, GC_GAM_DEVICE_LZ);
}

// gc_result_free keeps the large arrays of freed results (up to 24 GB) for the next batch instead of returning them to the allocator; this returns them.
void gc_result_cache_trim(void)
{
	g_resultBlocks.trim();
	// r5: the device / pinned blocks held back by gc_reads_destroy and by the device deflate's staging as well (blocks in use are not in the caches and are unaffected)
	g_readDeviceBlocks.trim(); g_readPinnedBlocks.trim(); g_deflateDeviceBlocks.trim(); g_deflatePinnedBlocks.trim();
}

// One alignment at a time, for a host that keeps the reference's own per-alignment calls (include/graphchainer_amd_shim.hpp: AddGAFLine / AddAlignment,
// src/GraphAlignerWrapper.h:43-44): the trace in output coordinates in, the GAF line / the vg::Alignment message out. Host code (no device work).
int gc_format_gaf_trace(const gc_graph* G, const char* read_name, const char* sequence, uint64_t sequence_len, const int32_t* node, const uint32_t* offset, const uint32_t* seqpos, const uint8_t* node_switch,
	uint64_t n, int cigar_match_mismatch_merge, char** out_text, uint64_t* out_len)
{
	if (!G || !sequence || !out_text || !out_len || (n && (!node || !offset || !seqpos || !node_switch))) return fail(GC_ERR_INVALID, "null argument");
	return guarded([&]() {
		gc::TraceView tv { node, offset, seqpos, node_switch, n };
		const std::string line = gc::formatGafLine(G->host, read_name ? read_name : "", sequence, sequence_len, tv, cigar_match_mismatch_merge != 0);
		char* buf = (char*)malloc(line.size() + 1);
		if (!buf) throw std::runtime_error("out of memory");
		memcpy(buf, line.data(), line.size());
		buf[line.size()] = 0;
		*out_text = buf; *out_len = line.size();
		return (int)GC_OK;
	});
}
static int formatVgTrace(const gc_graph* G, const char* read_name, const char* sequence, uint64_t sequence_len, const int32_t* node, const uint32_t* offset, const uint32_t* seqpos, const uint8_t* node_switch,
	uint64_t n, int32_t score, uint64_t alignment_start, uint64_t alignment_end, char** out_bytes, uint64_t* out_len, bool digraphIds);
int gc_format_vg_trace(const gc_graph* G, const char* read_name, const char* sequence, uint64_t sequence_len, const int32_t* node, const uint32_t* offset, const uint32_t* seqpos, const uint8_t* node_switch,
	uint64_t n, int32_t score, uint64_t alignment_start, uint64_t alignment_end, char** out_bytes, uint64_t* out_len)
{
	return formatVgTrace(G, read_name, sequence, sequence_len, node, offset, seqpos, node_switch, n, score, alignment_start, alignment_end, out_bytes, out_len, false);
}
// the message as AddAlignment leaves it (src/GraphAligner.h:205-212): digraph node ids (2 x segment index + strand), no names - for a host that calls
// replaceDigraphNodeIdsWithOriginalNodeIds itself right after (src/Aligner.cpp:1009), as the reference's own loop does
int gc_format_vg_trace_digraph(const gc_graph* G, const char* read_name, const char* sequence, uint64_t sequence_len, const int32_t* node, const uint32_t* offset, const uint32_t* seqpos, const uint8_t* node_switch,
	uint64_t n, int32_t score, uint64_t alignment_start, uint64_t alignment_end, char** out_bytes, uint64_t* out_len)
{
	return formatVgTrace(G, read_name, sequence, sequence_len, node, offset, seqpos, node_switch, n, score, alignment_start, alignment_end, out_bytes, out_len, true);
}
static int formatVgTrace(const gc_graph* G, const char* read_name, const char* sequence, uint64_t sequence_len, const int32_t* node, const uint32_t* offset, const uint32_t* seqpos, const uint8_t* node_switch,
	uint64_t n, int32_t score, uint64_t alignment_start, uint64_t alignment_end, char** out_bytes, uint64_t* out_len, bool digraphIds)
{
	if (!G || !sequence || !out_bytes || !out_len || (n && (!node || !offset || !seqpos || !node_switch))) return fail(GC_ERR_INVALID, "null argument");
	if (alignment_end < alignment_start || alignment_end > sequence_len) return fail(GC_ERR_INVALID, "gc_format_vg_trace: alignment_start / alignment_end outside the read");
	return guarded([&]() {
		gc::TraceView tv { node, offset, seqpos, node_switch, n };
		gc::VgAlignment aln = gc::buildVgAlignment(G->host, read_name ? read_name : "", sequence, sequence_len, tv, score, alignment_start, alignment_end);
		if (digraphIds) for (gc::VgMapping& m : aln.mappings) { m.nodeId = 2 * m.nodeId + (m.isReverse ? 1 : 0); m.name.clear(); }   // the inverse of replaceDigraphNodeIdsWithOriginalNodeIds (src/Aligner.cpp:152-165)
		const std::string msg = gc::vgToProtobuf(aln);
		char* buf = (char*)malloc(msg.size() + 1);
		if (!buf) throw std::runtime_error("out of memory");
		memcpy(buf, msg.data(), msg.size());
		buf[msg.size()] = 0;
		*out_bytes = buf; *out_len = msg.size();
		return (int)GC_OK;
	});
}
// The graph letter under each (bigraph node id, offset in the original node): what the reference's TraceItem constructor looks up (src/GraphAlignerCommon.h:148-153)
int gc_graph_letters(const gc_graph* G, const int32_t* node, const uint32_t* offset, uint64_t n, char* out)
{
	if (!G || !out || (n && (!node || !offset))) return fail(GC_ERR_INVALID, "null argument");
	return guarded([&]() {
		gc::GraphLetters letters(G->host);
		for (uint64_t i = 0; i < n; i++) {
			const size_t* size = G->host.originalNodeSize.find(node[i]);
			if (!size || offset[i] >= *size) throw std::runtime_error("gc_graph_letters: no such node / offset");
			out[i] = letters.at(node[i], offset[i]);
		}
		return (int)GC_OK;
	});
}

int gc_format_gam_level(const gc_graph* G, const gc_result* r, const char* const* read_names, const char* bases, const uint64_t* offsets, int level, char** out_bytes, uint64_t* out_len, uint64_t* n_chained_skipped)
{
	if ((level < -1 || level > 9) && level != GC_GAM_DEVICE_HUFFMAN && level != GC_GAM_DEVICE_LZ) return fail(GC_ERR_INVALID, "gc_format_gam_level: zlib levels are -1 (default) and 0..9, or GC_GAM_DEVICE_HUFFMAN / GC_GAM_DEVICE_LZ");
	return formatBatch(G, r, read_names, bases, offsets, OUT_GAM, 0, out_bytes, out_len, n_chained_skipped, level);
}

// gzip members of independent byte streams, deflated on the device as GC_GAM_DEVICE_HUFFMAN / GC_GAM_DEVICE_LZ do for the GAM groups (an empty stream gives an empty member)
static int gzipStreams(const uint8_t* bytes, const uint64_t* offsets, uint64_t n, char** out_bytes, uint64_t* out_offsets, bool lz);
int gc_gzip_streams(const uint8_t* bytes, const uint64_t* offsets, uint64_t n, char** out_bytes, uint64_t* out_offsets) { return gzipStreams(bytes, offsets, n, out_bytes, out_offsets, false); }
int gc_gzip_streams_lz(const uint8_t* bytes, const uint64_t* offsets, uint64_t n, char** out_bytes, uint64_t* out_offsets) { return gzipStreams(bytes, offsets, n, out_bytes, out_offsets, true); }
static int gzipStreams(const uint8_t* bytes, const uint64_t* offsets, uint64_t n, char** out_bytes, uint64_t* out_offsets, bool lz)
{
	if (!offsets || !out_bytes || !out_offsets || (offsets[n] && !bytes)) return fail(GC_ERR_INVALID, "null argument");
	for (uint64_t i = 0; i < n; i++) if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] >= (1ull << 32)) return fail(GC_ERR_INVALID, "gc_gzip_streams: offsets must ascend, streams below 4 GB");
	return guarded([&]() {
		std::vector<std::string> groups(n);
		for (uint64_t i = 0; i < n; i++) groups[i].assign((const char*)bytes + offsets[i], (const char*)bytes + offsets[i + 1]);
		gzipGroupsOnDevice(groups, false, lz);
		out_offsets[0] = 0;
		for (uint64_t i = 0; i < n; i++) out_offsets[i + 1] = out_offsets[i] + groups[i].size();
		char* buf = (char*)malloc(out_offsets[n] + 1);
		if (!buf) throw std::runtime_error("out of memory");
		for (uint64_t i = 0; i < n; i++) memcpy(buf + out_offsets[i], groups[i].data(), groups[i].size());
		*out_bytes = buf;
		return (int)GC_OK;
	});
}

// Test entry: the permutation the device's replay of libstdc++'s std::sort (hip/gc_stdsort_wave.hpp, what k_seed_glue runs for the reference's three order-critical unstable sorts)
// gives for arrays of 32-bit keys: array s = keys[offsets[s] .. offsets[s + 1]), perm_out likewise - perm_out[offsets[s] + i] = the index (inside its array) of the element
// that ends at place i. depth_limit < 0: the reference's 2 floor(log2 n); smaller values force the heapsort path.
int gc_std_sort_permutations(const uint32_t* keys, const uint64_t* offsets, uint64_t n_arrays, int64_t depth_limit, uint32_t* perm_out)
{
	if (!offsets || !perm_out || (!keys && n_arrays && offsets[n_arrays] > 0)) return fail(GC_ERR_INVALID, "null argument");
	return guarded([&]() {
		requireDevice();
		const uint64_t total = offsets[n_arrays];
		if (n_arrays >= 0xffffffffull) throw std::runtime_error("too many arrays");
		std::vector<unsigned long long> elems(total);
		for (uint64_t s = 0; s < n_arrays; s++) {
			if (offsets[s + 1] < offsets[s] || offsets[s + 1] - offsets[s] >= 0xffffffffull) throw std::runtime_error("bad offsets");
			for (uint64_t i = offsets[s]; i < offsets[s + 1]; i++) elems[i] = ((unsigned long long)keys[i] << 32) | (i - offsets[s]);
		}
		DeviceBuffer dElems, dOff, dScratch;
		unsigned long long* de = dElems.reserve<unsigned long long>(total);
		uint64_t* dof = dOff.reserve<uint64_t>(n_arrays + 1);
		uint32_t* ds = dScratch.reserve<uint32_t>(3 * total + 64 * n_arrays + 64);
		if (total) HIP_CHECK(hipMemcpy(de, elems.data(), total * sizeof(unsigned long long), hipMemcpyHostToDevice));
		HIP_CHECK(hipMemcpy(dof, offsets, (n_arrays + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
		launchTestStdSort(nullptr, de, dof, (uint32_t)n_arrays, ds, (long)depth_limit);
		HIP_CHECK(hipDeviceSynchronize());
		if (total) HIP_CHECK(hipMemcpy(elems.data(), de, total * sizeof(unsigned long long), hipMemcpyDeviceToHost));
		for (uint64_t i = 0; i < total; i++) perm_out[i] = (uint32_t)elems[i];
		return (int)GC_OK;
	});
}

// Test entry: the plain-layout kernel's column maximum (clipMaxXScore, hip/gc_device.hpp) on the caller's columns
int gc_test_max_x_score(const uint64_t* vp, const uint64_t* vn, const int32_t* score_end, uint64_t n, double error_cost, int32_t cells, int32_t* out)
{
	if (!out || ((!vp || !vn || !score_end) && n)) return fail(GC_ERR_INVALID, "null argument");
	if (cells < 1 || cells > 64 || n >= 0xffffffffull) return fail(GC_ERR_INVALID, "gc_test_max_x_score: cells must be in [1, 64]");
	return guarded([&]() {
		requireDevice();
		if (!n) return (int)GC_OK;
		DeviceBuffer dVp, dVn, dScore, dOut;
		uint64_t* a = dVp.reserve<uint64_t>(n); uint64_t* b = dVn.reserve<uint64_t>(n);
		int32_t* c = dScore.reserve<int32_t>(n); int32_t* o = dOut.reserve<int32_t>(n);
		HIP_CHECK(hipMemcpy(a, vp, n * sizeof(uint64_t), hipMemcpyHostToDevice));
		HIP_CHECK(hipMemcpy(b, vn, n * sizeof(uint64_t), hipMemcpyHostToDevice));
		HIP_CHECK(hipMemcpy(c, score_end, n * sizeof(int32_t), hipMemcpyHostToDevice));
		launchTestMaxXScore(nullptr, a, b, c, (uint32_t)n, error_cost, cells, o);
		HIP_CHECK(hipDeviceSynchronize());
		HIP_CHECK(hipMemcpy(out, o, n * sizeof(int32_t), hipMemcpyDeviceToHost));
		return (int)GC_OK;
	});
}

int gc_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

// free and total bytes of the current device's memory (hipMemGetInfo): what a host sizing its batches - or a benchmark reporting its peak - needs
int gc_device_memory(uint64_t* free_bytes, uint64_t* total_bytes)
{
	if (!free_bytes || !total_bytes) return fail(GC_ERR_INVALID, "null argument");
	return guarded([&]() {
		requireDevice();
		size_t f = 0, t = 0;
		HIP_CHECK(hipMemGetInfo(&f, &t));
		*free_bytes = f; *total_bytes = t;
		return (int)GC_OK;
	});
}

int gc_set_device(int device)
{
	return guarded([&]() { HIP_CHECK(hipSetDevice(device)); return (int)GC_OK; });
}

// fast_mode took the struct's tail padding: the other fields are where they were and the size is what it was
static_assert(sizeof(gc_params) == 216 && offsetof(gc_params, fast_mode) == offsetof(gc_params, selection_method) + 4 && offsetof(gc_params, fast_mode) + 4 == sizeof(gc_params), "gc_params layout");

static_assert(sizeof(gc_params_ext) == 16 && offsetof(gc_params_ext, precise_clipping) == 8, "gc_params_ext layout");
void gc_params_ext_default(gc_params_ext* e)
{
	if (!e) return;
	e->struct_size = (uint32_t)sizeof(gc_params_ext);
	e->x_drop = 0;               // off (src/AlignerMain.cpp: Xdropcutoff 0)
	e->precise_clipping = 0.0;   // off
}

void gc_params_default(gc_params* p)
{
	if (!p) return;
	p->bandwidth = 10;
	p->split_len = 35;
	p->split_gap = 35;
	p->colinear_gap = 10000;
	p->seed_density = 10;
	p->min_cluster_size = 1;
	p->long_pass = 0;
	p->keep_traces = 0;
	p->keep_seeds = 0;
	p->stitch = 1;
	p->edit_distances = 1;
	p->chain_traces = 1;
	p->device_output = 0;
	p->e_cutoff = -1;
	memset(&p->capacity, 0, sizeof(p->capacity));   // automatic
	p->ramp_bandwidth = 0;          // off (src/AlignerMain.cpp:147)
	p->max_cells_per_slice = -1;    // unlimited (src/AlignerMain.cpp:149: SIZE_MAX)
	p->force_global = 0;            // off (src/AlignerMain.cpp:160)
	p->seed_extend_density = -1;    // all seeds (chaining mode: tryAllSeeds, src/AlignerMain.cpp:204,449-453)
	p->extra_heuristic = 0;         // off (src/AlignerMain.cpp:170,192)
	p->colinear_chaining = 1;       // on; 0 is --no-colinear-chaining (src/AlignerMain.cpp:176,198-199)
	p->selection_method = GC_SELECT_GREEDY_LENGTH;
	p->fast_mode = 0;               // off (src/AlignerMain.cpp:180,195-196)
}

int gc_graph_create_from_gfa(const char* gfa_path, gc_graph** out)
{
	if (!gfa_path || !out) return fail(GC_ERR_INVALID, "null argument");
	*out = nullptr;
	gc_graph* G = new gc_graph();
	try {
		requireDevice();
		gc::StageClock clock;
		G->host = gc::AlignmentGraph::BuildFromGFAFile(gfa_path);
		G->host.buildMPC(true);
		malloc_trim(0);   // (the builders' freed small blocks back to the system: the host graph stays, and at config 5's sizes the host's memory is what bounds the graph)
		clock.lap("graph + MPC built");
		uploadGraph(G);
		clock.lap("graph uploaded");
	} catch (const DeviceError& e) {
		delete G;
		return fail(GC_ERR_DEVICE, e.what());
	} catch (const std::exception& e) {
		delete G;
		return fail(GC_ERR_GRAPH, e.what());
	}
	*out = G;
	return GC_OK;
}

int gc_graph_create(const gc_graph_desc* desc, gc_graph** out)
{
	if (!desc || !out) return fail(GC_ERR_INVALID, "null argument");
	*out = nullptr;
	gc_graph* G = new gc_graph();
	try {
		requireDevice();
		gc::AlignmentGraph& h = G->host;
		size_t n = desc->n_nodes;
		h.firstAmbiguous = desc->first_ambiguous;
		h.nodeLength.resize(n); h.nodeOffset.resize(n); h.nodeIDs.resize(n); h.reverse.resize(n); h.linearizable.assign(n, false);
		h.inNeighbors.resize(n); h.outNeighbors.resize(n);
		h.componentNumber.resize(n); h.chainNumber.resize(n); h.chainApproxPos.resize(n);
		for (size_t i = 0; i < n; i++) {
			h.nodeLength[i] = desc->node_length[i];
			h.nodeOffset[i] = desc->node_offset[i];
			h.nodeIDs[i] = desc->node_ids[i];
			h.reverse[i] = desc->node_ids[i] & 1;   // reverse-complement strand nodes have odd bigraph ids (src/BigraphToDigraph.cpp:101-104)
			h.bpSize += desc->node_length[i];
			for (uint64_t e = desc->in_off[i]; e < desc->in_off[i + 1]; e++) h.inNeighbors[i].push_back(desc->in_adj[e]);
			for (uint64_t e = desc->out_off[i]; e < desc->out_off[i + 1]; e++) h.outNeighbors[i].push_back(desc->out_adj[e]);
			h.componentNumber[i] = desc->component_number[i];
			h.chainNumber[i] = desc->chain_number[i];
			h.chainApproxPos[i] = desc->chain_approx_pos[i];
		}
		h.nodeSequences.resize(h.firstAmbiguous);
		for (size_t i = 0; i < h.firstAmbiguous; i++) h.nodeSequences[i] = { desc->node_seq[2 * i], desc->node_seq[2 * i + 1] };
		h.ambiguousNodeSequences.resize(n - h.firstAmbiguous);
		for (size_t i = 0; i < n - h.firstAmbiguous; i++) h.ambiguousNodeSequences[i] = { desc->ambiguous_seq[4 * i], desc->ambiguous_seq[4 * i + 1], desc->ambiguous_seq[4 * i + 2], desc->ambiguous_seq[4 * i + 3] };
		// nodeLookup: split nodes of each bigraph node in offset order
		std::vector<size_t> order(n);
		for (size_t i = 0; i < n; i++) order[i] = i;
		std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return h.nodeIDs[a] != h.nodeIDs[b] ? h.nodeIDs[a] < h.nodeIDs[b] : h.nodeOffset[a] < h.nodeOffset[b]; });
		// (without a lookup_order from the caller the minimizer index follows the order an unordered_map filled with the ids in ascending order iterates in - as r1-r3 built it)
		gc::HashOrder ascending;
		std::vector<int> ascendingIds;
		for (size_t at = 0; at < n;) {
			size_t end = at;
			while (end < n && h.nodeIDs[order[end]] == h.nodeIDs[order[at]]) end++;
			h.nodeLookup.add(h.nodeIDs[order[at]], order.data() + at, end - at);
			for (size_t k = at; k < end; k++) h.originalNodeSize[h.nodeIDs[order[at]]] += h.nodeLength[order[k]];
			ascending.insert(std::hash<int>()(h.nodeIDs[order[at]]));
			ascendingIds.push_back(h.nodeIDs[order[at]]);
			at = end;
		}
		for (uint32_t e : ascending.order()) h.nodeLookupOrder.push_back(ascendingIds[e]);
		if (desc->lookup_order) {
			// the host's nodeLookup iteration order: the minimizer index enumerates nodes in it (src/MinimizerSeeder.cpp:354-357)
			if (desc->n_lookup != h.nodeLookup.size()) throw std::runtime_error("lookup_order must list every bigraph node id once");
			std::unordered_set<int> seen;
			for (uint64_t i = 0; i < desc->n_lookup; i++)
				if (!h.nodeLookup.count(desc->lookup_order[i]) || !seen.insert(desc->lookup_order[i]).second) throw std::runtime_error("lookup_order must list every bigraph node id once");
			h.nodeLookupOrder.assign(desc->lookup_order, desc->lookup_order + desc->n_lookup);
		}
		h.finalized = true;
		h.buildMPC(true);
		uploadGraph(G);
	} catch (const DeviceError& e) {
		delete G;
		return fail(GC_ERR_DEVICE, e.what());
	} catch (const std::exception& e) {
		delete G;
		return fail(GC_ERR_GRAPH, e.what());
	}
	*out = G;
	return GC_OK;
}

void gc_graph_destroy(gc_graph* g) { delete g; malloc_trim(0); }   // (the host graph's many small blocks back to the system, not to the allocator's free lists: a graph loaded next would sit beside them)
uint64_t gc_graph_num_nodes(const gc_graph* g) { return g ? g->host.NodeSize() : 0; }
uint64_t gc_graph_size_bp(const gc_graph* g) { return g ? g->host.SizeInBP() : 0; }

int gc_graph_trim_host(gc_graph* G)
{
	if (!G) return fail(GC_ERR_INVALID, "null argument");
	gc::AlignmentGraph& h = G->host;
	std::vector<std::vector<std::vector<size_t>>>().swap(h.mpc);
	std::vector<std::vector<std::vector<size_t>>>().swap(h.paths);
	std::vector<std::vector<std::vector<std::pair<size_t, size_t>>>>().swap(h.backwards);
	std::vector<std::vector<size_t>>().swap(h.topo);
	std::vector<std::vector<size_t>>().swap(h.topo_ids);
	std::vector<std::vector<size_t>>().swap(h.component_ids);
	G->hostMpcTrimmed = true;
	malloc_trim(0);
	return GC_OK;
}

int gc_graph_array(const gc_graph* G, const char* name, int64_t** out, uint64_t* count)
{
	if (!G || !name || !out || !count) return fail(GC_ERR_INVALID, "null argument");
	if (G->hostMpcTrimmed && (strncmp(name, "mpc_", 4) == 0 || strncmp(name, "paths", 5) == 0 || strncmp(name, "back_", 5) == 0 || strcmp(name, "topo_id") == 0))
		return fail(GC_ERR_INVALID, "the host copy of the MPC index was released (gc_graph_trim_host)");
	const gc::AlignmentGraph& g = G->host;
	std::vector<int64_t> v;
	std::string nm = name;
	size_t n = g.NodeSize();
	if (nm == "nodeLength") for (size_t i = 0; i < n; i++) v.push_back(g.nodeLength[i]);
	else if (nm == "nodeOffset") for (size_t i = 0; i < n; i++) v.push_back(g.nodeOffset[i]);
	else if (nm == "nodeIDs") for (size_t i = 0; i < n; i++) v.push_back(g.nodeIDs[i]);
	else if (nm == "reverse") for (size_t i = 0; i < n; i++) v.push_back(g.reverse[i]);
	else if (nm == "componentNumber") for (size_t i = 0; i < n; i++) v.push_back(g.componentNumber[i]);
	else if (nm == "chainNumber") for (size_t i = 0; i < n; i++) v.push_back(g.chainNumber[i]);
	else if (nm == "chainApproxPos") for (size_t i = 0; i < n; i++) v.push_back(g.chainApproxPos[i]);
	else if (nm == "component_map") for (size_t i = 0; i < n; i++) v.push_back(g.component_map[i]);
	else if (nm == "out_off") { v.push_back(0); for (size_t i = 0; i < n; i++) v.push_back(v.back() + (int64_t)g.outNeighbors[i].size()); }
	else if (nm == "out_adj") for (size_t i = 0; i < n; i++) for (size_t x : g.outNeighbors[i]) v.push_back(x);
	else if (nm == "in_off") { v.push_back(0); for (size_t i = 0; i < n; i++) v.push_back(v.back() + (int64_t)g.inNeighbors[i].size()); }
	else if (nm == "in_adj") for (size_t i = 0; i < n; i++) for (size_t x : g.inNeighbors[i]) v.push_back(x);
	else if (nm == "mpc_width") for (size_t c = 0; c < g.mpc.size(); c++) v.push_back(g.mpc[c].size());
	else if (nm == "firstAmbiguous") v.push_back((int64_t)std::min(g.firstAmbiguous, n));
	else if (nm == "nodeSeq") for (size_t i = 0; i < n && i < g.firstAmbiguous; i++) { v.push_back((int64_t)g.nodeSequences[i][0]); v.push_back((int64_t)g.nodeSequences[i][1]); }   // bit patterns
	else if (nm == "ambiguousSeq") for (const gc::AmbiguousSeq& a : g.ambiguousNodeSequences) { v.push_back((int64_t)a.A); v.push_back((int64_t)a.T); v.push_back((int64_t)a.C); v.push_back((int64_t)a.G); }
	else if (nm == "component_idx") for (size_t i = 0; i < n; i++) v.push_back(g.component_idx[i]);
	else if (nm == "topo_id") for (size_t i = 0; i < n; i++) v.push_back(g.topo_ids[g.component_map[i]][g.component_idx[i]]);
	// the path cover: mpc_path_comp[p] = component of path p, mpc_path_off / mpc_path_nodes = its nodes (global ids) in order
	else if (nm == "mpc_path_comp") { for (size_t c = 0; c < g.mpc.size(); c++) for (size_t k = 0; k < g.mpc[c].size(); k++) v.push_back(c); }
	else if (nm == "mpc_path_off") { v.push_back(0); for (size_t c = 0; c < g.mpc.size(); c++) for (const auto& p : g.mpc[c]) v.push_back(v.back() + (int64_t)p.size()); }
	else if (nm == "mpc_path_nodes") { for (size_t c = 0; c < g.mpc.size(); c++) for (const auto& p : g.mpc[c]) for (size_t x : p) v.push_back(x); }
	// per node (global id): the path ids through it (local to its component), and the backward links (node = global id, path id)
	else if (nm == "paths_off") { v.push_back(0); for (size_t i = 0; i < n; i++) v.push_back(v.back() + (int64_t)g.paths[g.component_map[i]][g.component_idx[i]].size()); }
	else if (nm == "paths") { for (size_t i = 0; i < n; i++) for (size_t k : g.paths[g.component_map[i]][g.component_idx[i]]) v.push_back(k); }
	else if (nm == "back_off") { v.push_back(0); for (size_t i = 0; i < n; i++) v.push_back(v.back() + (int64_t)g.backwards[g.component_map[i]][g.component_idx[i]].size()); }
	else if (nm == "back_node") { for (size_t i = 0; i < n; i++) for (const auto& b : g.backwards[g.component_map[i]][g.component_idx[i]]) v.push_back(g.component_ids[g.component_map[i]][b.first]); }
	else if (nm == "back_path") { for (size_t i = 0; i < n; i++) for (const auto& b : g.backwards[g.component_map[i]][g.component_idx[i]]) v.push_back(b.second); }
	else if (nm == "lookupOrder") { for (int id : g.nodeLookupOrder) v.push_back(id); }
	else return fail(GC_ERR_INVALID, "unknown graph array " + nm);
	*out = mallocArray<int64_t>(v.size());
	memcpy(*out, v.data(), v.size() * sizeof(int64_t));
	*count = v.size();
	return GC_OK;
}

// ---- seeder -------------------------------------------------------------------------------------------
static inline uint32_t hostHashKmer(uint64_t kmer) { kmer *= 0x9E3779B97F4A7C15ull; return (uint32_t)(kmer >> 32); }

// hash table, membership filter and start offsets of a built minimizer index -> HBM
static void uploadSeeder(gc_seeder* S, std::optional<uint32_t> filterBitsOverride)   // (GC_TEST_SEED_FILTER_BITS)
{
	size_t nKeys = S->host.kmers.size();
	size_t tableSize = 16;
	while (tableSize < 2 * nKeys) tableSize <<= 1;
	std::vector<uint64_t> table(tableSize, ~0ull);
	for (size_t i = 0; i < nKeys; i++) {
		uint32_t hsh = hostHashKmer(S->host.kmers[i]) & (uint32_t)(tableSize - 1);
		while (table[hsh] != ~0ull) hsh = (hsh + 1) & (uint32_t)(tableSize - 1);
		table[hsh] = ((S->host.kmers[i] & 0xffffffffull) << 32) | (uint64_t)i;   // (k <= 15: the whole k-mer; longer ones are verified against wideKmers)
	}
	if (nKeys >= 0xffffffffull) throw std::runtime_error("minimizer index too large for 32-bit key indices");
	S->dev.wideKmers = nullptr;
	if (S->host.k > 15) {
		uint64_t* dKmers = uploadVector(S->host.kmers);
		S->allocations.push_back(dKmers);
		S->dev.wideKmers = dKmers;
	}
	uint64_t* dTable = uploadVector(table);
	S->allocations.push_back(dTable);
	// membership filter in front of the table (see filterBit in gc_kernels.hip): ~8 bits per key, at most 2^28 bits; on cfg2 (5 M keys)
	// 2^25 bits = 4 MB, which stays in every XCD's L2 (a 32 MB filter missed to the fabric on every probe)
	uint32_t filterBits = 20;
	while (filterBits < 28 && (1ull << filterBits) < 8 * nKeys) filterBits++;
	if (filterBitsOverride) filterBits = *filterBitsOverride;
	std::vector<uint32_t> filter((1ull << filterBits) / 32, 0);
	for (size_t i = 0; i < nKeys; i++) { uint32_t fb = (uint32_t)((S->host.kmers[i] * 0xD6E8FEB86659FD93ull) >> (64 - filterBits)); filter[fb >> 5] |= 1u << (fb & 31); }
	S->dev.filterShift = 64 - filterBits;
	uint32_t* dFilter = uploadVector(filter);
	S->allocations.push_back(dFilter);
	S->dev.filter = dFilter;
	uint64_t* dStart = uploadVector(S->host.startPos);
	S->allocations.push_back(dStart);
	S->dev.table = dTable;
	S->dev.tableMask = (uint32_t)(tableSize - 1);
	S->dev.startPos = dStart;
	uint64_t* dPositions = uploadVector(S->host.positions);   // the occurrence lists: the device expands the seeds itself (gc_seedglue.hip)
	S->allocations.push_back(dPositions);
	S->dev.positions = dPositions;
	S->dev.nKeys = (uint32_t)nKeys;
	S->dev.maxCount = (uint32_t)std::min<size_t>(S->host.maxCount, 0xffffffffu);
	S->dev.k = (int32_t)S->host.k;
	S->dev.w = (int32_t)S->host.w;
}

// The minimizer index built by the device (gc_minimizer.hip): window scan per bigraph node, one radix sort; the host only cuts the sorted
// pairs into the k-mer groups. Same index as gc::MinimizerIndex::Build (tests/test_index_cache.py compares them array by array).
// false = not applicable here (deque longer than the kernel's ring), the caller builds on the host - as it does under GC_SEEDER_BUILD=host.
static bool buildSeederOnDevice(const gc_graph* G, gc_seeder* S, size_t k, size_t w, double keepLeastFrequentFraction)
{
	if (w - k + 2 > 32 || k > 15) return false;   // (the device build packs the k-mer into 30 bits of its sort key: longer minimizers are built on the host)
	const gc::AlignmentGraph& h = G->host;
	// minimizers ending inside an overlap prefix are skipped (src/MinimizerSeeder.cpp:323-340,369): never the case for the 0M graphs the
	// library loads, checked rather than assumed
	for (size_t i = 0; i < h.NodeSize(); i++) {
		if (h.nodeOffset[i] == 0) continue;
		for (size_t nb : h.inNeighbors[i]) if (h.nodeIDs[nb] != h.nodeIDs[i]) return false;
	}
	std::vector<int32_t> idOrder(h.nodeLookupOrder.begin(), h.nodeLookupOrder.end());   // arrival order at -t 1: nodeLookup iteration order (:354-357)
	if (idOrder.empty()) return false;
	int32_t* dOrder = uploadVector(idOrder);
	uint64_t *dKeys = nullptr, *dValues = nullptr;
	uint64_t n = gcdev::buildMinimizerPairsDevice(G->dev, dOrder, (uint32_t)idOrder.size(), (uint32_t)k, (uint32_t)w, &dKeys, &dValues);
	(void)hipFree(dOrder);
	if (n == ~0ull) { (void)hipGetLastError(); return false; }
	std::vector<uint64_t> keys(n);
	gc::MinimizerIndex& idx = S->host;
	idx = gc::MinimizerIndex();
	idx.k = k; idx.w = w;
	idx.positions.resize(n);
	if (n) {
		HIP_CHECK(hipMemcpy(keys.data(), dKeys, n * 8, hipMemcpyDeviceToHost));
		HIP_CHECK(hipMemcpy(idx.positions.data(), dValues, n * 8, hipMemcpyDeviceToHost));
		(void)hipFree(dKeys); (void)hipFree(dValues);
	}
	for (size_t i = 0; i < n; i++) {
		uint64_t kmer = keys[i] >> 34;
		if (idx.kmers.empty() || idx.kmers.back() != kmer) { idx.kmers.push_back(kmer); idx.startPos.push_back(i); }
	}
	idx.startPos.push_back(n);
	idx.maxCount = gc::minimizerMaxCount(idx.startPos, keepLeastFrequentFraction);
	return true;
}

static bool seederShapeOk(int64_t k, int64_t w) { return k >= 1 && k <= 31 && w >= k; }   // (the reference's range: src/AlignerMain.cpp:221,390)

int gc_seeder_create(const gc_graph* g, int32_t k, int32_t w, double keepFraction, gc_seeder** out)
{
	if (!g || !out) return fail(GC_ERR_INVALID, "null argument");
	if (!seederShapeOk(k, w)) return fail(GC_ERR_INVALID, "supported minimizer length is 1..31 with w >= k");
	*out = nullptr;
	gc_seeder* S = new gc_seeder();
	int rc = guarded([&]() {
		requireDevice();
		const gc::Switches sw = gc::Switches::fromEnvironment();
		if (sw.seederBuildOnHost || !buildSeederOnDevice(g, S, (size_t)k, (size_t)w, keepFraction)) S->host = gc::MinimizerIndex::Build(g->host, (size_t)k, (size_t)w, keepFraction);
		uploadSeeder(S, sw.testSeedFilterBits);
		return (int)GC_OK;
	});
	if (rc != GC_OK) { delete S; return rc; }
	*out = S;
	return GC_OK;
}

// ---- index cache (host/gc_index_cache.hpp) -----------------------------------------------
int gc_index_build(const char* gfa_path, int32_t k, int32_t w, double keepFraction, const char* cache_path)
{
	if (!gfa_path || !cache_path) return fail(GC_ERR_INVALID, "null argument");
	if (k > 0 && !seederShapeOk(k, w)) return fail(GC_ERR_INVALID, "supported minimizer length is 1..31 with w >= k");
	try {
		gc::AlignmentGraph graph = gc::AlignmentGraph::BuildFromGFAFile(gfa_path);
		graph.buildMPC(true);
		if (k > 0) {
			gc::MinimizerIndex idx = gc::MinimizerIndex::Build(graph, (size_t)k, (size_t)w, keepFraction);
			gc::SaveIndexCache(cache_path, graph, &idx);
		} else {
			gc::SaveIndexCache(cache_path, graph, nullptr);
		}
	} catch (const std::exception& e) {
		return fail(GC_ERR_GRAPH, e.what());
	}
	return GC_OK;
}

int gc_index_save(const gc_graph* g, const gc_seeder* s, const char* cache_path)
{
	if (!g || !cache_path) return fail(GC_ERR_INVALID, "null argument");
	try {
		if (g->hostMpcTrimmed) return fail(GC_ERR_INVALID, "the host copy of the MPC index was released (gc_graph_trim_host): nothing to write the cache from");
		gc::SaveIndexCache(cache_path, g->host, s ? &s->host : nullptr);
	} catch (const std::exception& e) {
		return fail(GC_ERR_GRAPH, e.what());
	}
	return GC_OK;
}

static void fillIndexInfo(const gc::IndexCacheInfo& info, uint64_t* out)
{
	if (!out) return;
	out[0] = gc::INDEX_CACHE_VERSION; out[1] = info.nodes; out[2] = info.bp; out[3] = info.hasSeeder ? 1 : 0;
	out[4] = info.k; out[5] = info.w; out[6] = info.kmers; out[7] = info.positions;
}

int gc_index_check(const char* cache_path, uint64_t* info8)
{
	if (!cache_path) return fail(GC_ERR_INVALID, "null argument");
	try {
		fillIndexInfo(gc::CheckIndexCache(cache_path), info8);
	} catch (const std::exception& e) {
		return fail(GC_ERR_GRAPH, e.what());
	}
	return GC_OK;
}

int gc_index_load(const char* cache_path, gc_graph** graph_out, gc_seeder** seeder_out)
{
	if (!cache_path || !graph_out) return fail(GC_ERR_INVALID, "null argument");
	*graph_out = nullptr;
	if (seeder_out) *seeder_out = nullptr;
	gc_graph* G = new gc_graph();
	gc_seeder* S = new gc_seeder();
	try {
		requireDevice();
		gc::IndexCacheInfo info = gc::LoadIndexCache(cache_path, G->host, S->host);
		uploadGraph(G);
		if (info.hasSeeder && seeder_out) {
			if (!seederShapeOk((int64_t)S->host.k, (int64_t)S->host.w)) throw std::runtime_error("index cache holds a minimizer index this library cannot run");
			uploadSeeder(S, gc::Switches::fromEnvironment().testSeedFilterBits);
		} else {
			delete S;
			S = nullptr;
		}
	} catch (const DeviceError& e) {
		delete G; delete S;
		return fail(GC_ERR_DEVICE, e.what());
	} catch (const std::exception& e) {
		delete G; delete S;
		return fail(GC_ERR_GRAPH, e.what());
	}
	*graph_out = G;
	if (seeder_out) *seeder_out = S;
	return GC_OK;
}

void gc_seeder_destroy(gc_seeder* s) { delete s; malloc_trim(0); }

int gc_seeder_array(const gc_seeder* s, const char* name, int64_t** out, uint64_t* count)
{
	if (!s || !name || !out || !count) return fail(GC_ERR_INVALID, "null argument");
	std::string nm = name;
	const std::vector<uint64_t>* src = nullptr;
	std::vector<uint64_t> single;
	if (nm == "kmers") src = &s->host.kmers;
	else if (nm == "start") src = &s->host.startPos;
	else if (nm == "positions") src = &s->host.positions;
	else if (nm == "maxcount") { single.push_back(s->host.maxCount); src = &single; }
	else if (nm == "k") { single.push_back((uint64_t)s->dev.k); src = &single; }
	else if (nm == "w") { single.push_back((uint64_t)s->dev.w); src = &single; }
	else return fail(GC_ERR_INVALID, "unknown seeder array " + nm);
	*out = mallocArray<int64_t>(src->size());
	for (size_t i = 0; i < src->size(); i++) (*out)[i] = (int64_t)(*src)[i];
	*count = src->size();
	return GC_OK;
}

// ---- streams / reads ------------------------------------------------------------------------------------
int gc_stream_create(gc_stream** out)
{
	if (!out) return fail(GC_ERR_INVALID, "null argument");
	*out = nullptr;
	gc_stream* st = new gc_stream();
	int rc = guarded([&]() {
		requireDevice();
		HIP_CHECK(hipGetDevice(&st->device));
		if (st->device < 0 || st->device >= 16) throw std::runtime_error("gc_stream_create: device index beyond the 16 per-device slots of the whole-read token and scratch");
		createStream(&st->stream);       // non-blocking: uploads of another batch on the null stream do not serialise with this one
		createStream(&st->longStream);
		for (auto& e : st->ev) HIP_CHECK(hipEventCreate(&e));
		for (auto& e : st->fragEv) HIP_CHECK(hipEventCreate(&e));
		for (auto& e : st->longEv) HIP_CHECK(hipEventCreate(&e));
		return (int)GC_OK;
	});
	if (rc != GC_OK) { delete st; return rc; }
	{ std::lock_guard<std::mutex> lock(g_longScratchCount); noteHardwareQueues(++g_longScratch[st->device & 15].streams); }
	*out = st;
	return GC_OK;
}
void gc_stream_destroy(gc_stream* st)
{
	if (!st) return;
	{
		std::lock_guard<std::mutex> count(g_longScratchCount);
		SharedLongScratch& shared = g_longScratch[st->device & 15];
		if (--shared.streams == 0) {   // the device's last stream: nobody can hold the token any more
			TokenHold alone;
			alone.lock(g_longPassToken[st->device & 15], 1, true);   // (every slot free and nobody beside: as a pass that fills the chip waits)
			int current = 0;
			if (hipGetDevice(&current) == hipSuccess) { (void)hipSetDevice(st->device); for (auto& b : shared.buffer) b.release(); for (auto& r : shared.rounds) r.release(); (void)hipSetDevice(current); }
		}
	}
	delete st;
}

int gc_reads_upload(const char* bases, const uint64_t* offsets, uint64_t n, gc_reads** out)
{
	if (!offsets || !out || (!bases && n > 0 && offsets[n] > 0)) return fail(GC_ERR_INVALID, "null argument");
	*out = nullptr;
	gc_reads* R = new gc_reads();
	hipStream_t uploadStream = nullptr;
	int rc = guarded([&]() {
		requireDevice();
		R->offsets.assign(offsets, offsets + n + 1);
		R->totalBases = offsets[n];
		if (n >= 0xffffffffull) throw std::runtime_error("too many reads in one batch");
		// per-read layout of the bit vectors (host, O(n)); everything per base is derived on the device from one copy of the raw bases
		R->maskOff.assign(n, 0);
		R->maskWords.assign(n, 0);
		std::vector<EdRead> edReads(n);
		std::vector<uint64_t> eqOff(n);
		uint64_t totalWords = 0, eqWords = 0;
		for (uint64_t r = 0; r < n; r++) {
			R->maskOff[r] = totalWords;
			R->maskWords[r] = (uint32_t)((offsets[r + 1] - offsets[r] + 63) / 64 + 1);
			totalWords += 8ull * R->maskWords[r];
			edReads[r] = EdRead { offsets[r], eqWords, (uint32_t)(offsets[r + 1] - offsets[r]), R->maskWords[r] };
			eqOff[r] = eqWords;
			eqWords += 4ull * R->maskWords[r];
		}
		const uint64_t total = R->totalBases;
		// one device block for everything (256-byte aligned parts), one pinned block for what goes up; both come from small caches (see BlockCache)
		HIP_CHECK(hipGetDevice(&R->device));
		size_t at = 0;
		auto part = [&](size_t bytes) { const size_t here = at; at += (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255; return here; };
		const size_t oBases = part(2 * total), oOffsets = part((n + 1) * sizeof(uint64_t)), oMasks = part(totalWords * sizeof(uint64_t)), oEqMasks = part(eqWords * sizeof(uint64_t)),
			oEdReads = part(n * sizeof(EdRead)), oPacked = part(((total >> 5) + 1) * sizeof(uint64_t)), oInvalid = part(((total >> 6) + 1) * sizeof(uint64_t)), oChunkRead = part(((total >> 6) + 1) * sizeof(uint32_t)),
			oMaskOff = part(n * sizeof(uint64_t)), oMaskWords = part(n * sizeof(uint32_t)), oEqOff = part(n * sizeof(uint64_t)), oReadInvalid = part(n);
		R->deviceBlock = g_readDeviceBlocks.get(at, R->device, R->deviceBlockBytes);
		char* D = (char*)R->deviceBlock;
		R->devBases = D + oBases; R->devOffsets = (uint64_t*)(D + oOffsets); R->devMasks = (uint64_t*)(D + oMasks); R->devEqMasks = (uint64_t*)(D + oEqMasks); R->devEdReads = (EdRead*)(D + oEdReads);
		R->devPacked = (uint64_t*)(D + oPacked); R->devInvalid = (uint64_t*)(D + oInvalid); R->devChunkRead = (uint32_t*)(D + oChunkRead); R->devReadInvalid = (uint8_t*)(D + oReadInvalid);
		uint64_t* pMaskOff = (uint64_t*)(D + oMaskOff);
		uint32_t* pMaskWords = (uint32_t*)(D + oMaskWords);
		uint64_t* pEqOff = (uint64_t*)(D + oEqOff);
		uint8_t* pInvalid = R->devReadInvalid;
		R->devMaskOff = pMaskOff; R->devMaskWords = pMaskWords;
		// staging: the bases and the five small arrays in one pinned block, copied asynchronously on a stream of the calling thread's own (a synchronous copy from pageable
		// memory goes through the runtime's bounce buffers at a few GB/s and its null-stream semantics)
		size_t hat = 0;
		auto hpart = [&](size_t bytes) { const size_t here = hat; hat += (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255; return here; };
		const size_t hBases = hpart(total), hOffsets = hpart((n + 1) * sizeof(uint64_t)), hMaskOff = hpart(n * sizeof(uint64_t)), hMaskWords = hpart(n * sizeof(uint32_t)), hEqOff = hpart(n * sizeof(uint64_t)),
			hEdReads = hpart(n * sizeof(EdRead)), hInvalidBack = hpart(n);
		size_t pinnedBytes = 0;
		struct { hipStream_t q; } up { threadStream(R->device) };
		uploadStream = up.q;
		char* H = (char*)g_readPinnedBlocks.get(hat, R->device, pinnedBytes);
		// (waits for the stream before the block goes back: after an exception between the copies / kernels and the wait below they may still be reading it - ADVICE r4)
		struct PinnedReturn { char* p; size_t bytes; int device; hipStream_t q; ~PinnedReturn() { (void)hipStreamSynchronize(q); g_readPinnedBlocks.put(p, bytes, device); } } pinnedReturn { H, pinnedBytes, R->device, up.q };
		if (total) memcpy(H + hBases, bases, total);
		memcpy(H + hOffsets, offsets, (n + 1) * sizeof(uint64_t));
		if (n) {
			memcpy(H + hMaskOff, R->maskOff.data(), n * sizeof(uint64_t)); memcpy(H + hMaskWords, R->maskWords.data(), n * sizeof(uint32_t));
			memcpy(H + hEqOff, eqOff.data(), n * sizeof(uint64_t)); memcpy(H + hEdReads, edReads.data(), n * sizeof(EdRead));
		}
		if (total) HIP_CHECK(hipMemcpyAsync(R->devBases, H + hBases, total, hipMemcpyHostToDevice, up.q));
		HIP_CHECK(hipMemcpyAsync(R->devOffsets, H + hOffsets, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, up.q));
		if (n) {
			HIP_CHECK(hipMemcpyAsync(pMaskOff, H + hMaskOff, n * sizeof(uint64_t), hipMemcpyHostToDevice, up.q));
			HIP_CHECK(hipMemcpyAsync(pMaskWords, H + hMaskWords, n * sizeof(uint32_t), hipMemcpyHostToDevice, up.q));
			HIP_CHECK(hipMemcpyAsync(pEqOff, H + hEqOff, n * sizeof(uint64_t), hipMemcpyHostToDevice, up.q));
			HIP_CHECK(hipMemcpyAsync(R->devEdReads, H + hEdReads, n * sizeof(EdRead), hipMemcpyHostToDevice, up.q));
		}
		launchPackReads(up.q, R->devOffsets, (uint32_t)n, total, R->devBases, pMaskOff, pMaskWords, R->devMasks, pEqOff, R->devEqMasks, pInvalid, R->devPacked, R->devInvalid, R->devChunkRead);
		R->invalid.assign(n, 0);
		if (n) HIP_CHECK(hipMemcpyAsync(H + hInvalidBack, pInvalid, n, hipMemcpyDeviceToHost, up.q));
		HIP_CHECK(hipStreamSynchronize(up.q));
		if (n) memcpy(R->invalid.data(), H + hInvalidBack, n);
		return (int)GC_OK;
	});
	if (rc != GC_OK) {
		if (uploadStream) (void)hipStreamSynchronize(uploadStream);   // ~gc_reads returns the device block to its cache: nothing of this call may still be writing to it
		delete R;
		return rc;
	}
	*out = R;
	return GC_OK;
}
void gc_reads_destroy(gc_reads* r) { delete r; }

// Where the text of a parse comes from. place() puts the len bytes at devText with work on q (pinnedText [len] is the call's staging block, free until the tables are built)
// and returns the text's last byte (any value for an empty text); done(), if set, runs once the tables are built, while the text still lies on the device.
struct FxSource {
	uint32_t len = 0;
	std::function<char(char* devText, char* pinnedText, hipStream_t q, int device)> place;
	std::function<void(const char* devText, uint32_t consumed, hipStream_t q)> done;
};
struct InvalidInput : std::runtime_error { using std::runtime_error::runtime_error; };   // GC_ERR_INVALID from inside a guarded call

// gc_reads_parse and gc_reads_parse_bgzf from the point where the text lies on the device
static int readsParseFrom(const FxSource& src, int32_t format, uint32_t flags, gc_reads** reads, gc_fastx_table** table)
{
	const uint64_t len = src.len;
	gc_reads* R = new gc_reads();
	gc_fastx_table* T = nullptr;
	hipStream_t uploadStream = nullptr;
	auto body = [&]() {
		requireDevice();
		using namespace gcdev;
		HIP_CHECK(hipGetDevice(&R->device));
		const int device = R->device;
		hipStream_t q = threadStream(device);
		uploadStream = q;
		const uint32_t L = (uint32_t)len;
		const bool final = (flags & GC_FASTX_FINAL) != 0;
		auto round = [](size_t bytes) { return (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255; };
		// blocks of this call: the text and its tables on the device, one pinned block for what goes up and comes down; all from the read batches' caches
		struct Held { BlockCache* cache; void* p = nullptr; size_t bytes = 0; int device; hipStream_t q;
			~Held() { if (p) { (void)hipStreamSynchronize(q); cache->put(p, bytes, device); } } };   // (waits: a copy or kernel of a failed call may still use the block)
		Held textBlock { &g_readDeviceBlocks, nullptr, 0, device, q }, tableBlock { &g_readDeviceBlocks, nullptr, 0, device, q }, pinned { &g_readPinnedBlocks, nullptr, 0, device, q },
			small { &g_readPinnedBlocks, nullptr, 0, device, q };
		struct Events { hipEvent_t a = nullptr, b = nullptr; ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } ev;
		HIP_CHECK(hipEventCreate(&ev.a)); HIP_CHECK(hipEventCreate(&ev.b));
		double kernelMs = 0;
		auto addSegment = [&]() { float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, ev.a, ev.b)); kernelMs += ms; };   // (after the synchronize that follows the segment)

		// ---- 1: the text goes up, its newlines are counted (the line tables are sized by the count) ----
		// pinned: text [L] | counts. The text's part is used again at the end for the bases and ids coming down: a line gives bytes to one of them at most, so both fit
		const size_t hMeta = round(L), pinnedBytes = hMeta + round(FX_META_WORDS * sizeof(uint32_t));
		pinned.p = g_readPinnedBlocks.get(pinnedBytes, device, pinned.bytes);
		char* H = (char*)pinned.p;
		uint32_t* hostMeta = (uint32_t*)(H + hMeta);
		textBlock.p = g_readDeviceBlocks.get(pinnedBytes, device, textBlock.bytes);
		char* devText = (char*)textBlock.p;
		uint32_t* devMeta = (uint32_t*)(devText + hMeta);
		const char lastByte = src.place(devText, H, q, device);
		HIP_CHECK(hipEventRecord(ev.a, q));
		HIP_CHECK(fxCountNewlines(q, devText, L, devMeta));
		HIP_CHECK(hipEventRecord(ev.b, q));
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
		size_t at = 0;
		auto part = [&](size_t bytes) { const size_t here = at; at += round(bytes); return here; };
		const size_t oLineEnd = part(lines * 4), oMap = part(lines), oScanned = part(lines), oHdr = part(lines * 4), oRecIdx = part(lines * 4), oContrib = part((lines + 1) * 4),
			oDest = part((lines + 1) * 4), oRecLine = part(lines * 4), oReadOff = part((lines + 1) * 8), oNameLen = part((lines + 1) * 4), oNameOff = part((lines + 1) * 4),
			oNames = part((size_t)L + 1);
		FxTables t {};
		t.tempBytes = fxScanTempBytes(L, v.nLines);
		const size_t oTemp = part(t.tempBytes);
		tableBlock.p = g_readDeviceBlocks.get(at, device, tableBlock.bytes);
		char* D = (char*)tableBlock.p;
		t.lineEnd = (uint32_t*)(D + oLineEnd); t.map = (uint8_t*)(D + oMap); t.scanned = (uint8_t*)(D + oScanned); t.hdr = (uint32_t*)(D + oHdr); t.recIdx = (uint32_t*)(D + oRecIdx);
		t.contrib = (uint32_t*)(D + oContrib); t.dest = (uint32_t*)(D + oDest); t.recLine = (uint32_t*)(D + oRecLine); t.meta = devMeta; t.temp = D + oTemp;
		v.lineEnd = t.lineEnd;
		uint32_t nHeaders = 0, nRecords = 0, total = 0, consumed = final ? L : 0;
		if (v.nLines) {
			HIP_CHECK(hipEventRecord(ev.a, q));
			HIP_CHECK(fxBuildTables(q, v, t));
			HIP_CHECK(hipEventRecord(ev.b, q));
			HIP_CHECK(hipMemcpyAsync(hostMeta, devMeta, FX_META_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, q));
			HIP_CHECK(hipStreamSynchronize(q));
			addSegment();
			if (v.nNewlines && hostMeta[FX_META_SELECTED] != v.nNewlines) throw std::runtime_error("gc_reads_parse: the line table disagrees with the newline count");
			nHeaders = hostMeta[FX_META_HEADERS]; nRecords = hostMeta[FX_META_RECORDS]; total = hostMeta[FX_META_BASES]; consumed = hostMeta[FX_META_CONSUMED];
			if (nRecords > nHeaders || nHeaders > v.nLines || total > L || consumed > L) throw std::runtime_error("gc_reads_parse: the record table is out of range");
		}
		const uint64_t n = nRecords;

		// ---- 3: read offsets and id offsets, down to the host for the per-read layout ----
		// a second, small pinned block: offsets | id offsets | invalid flags | the four layout arrays that go up
		size_t sat = 0;
		auto spart = [&](size_t bytes) { const size_t here = sat; sat += round(bytes); return here; };
		const size_t sOff = spart((n + 1) * 8), sNameOff = spart((n + 1) * 4), sInvalid = spart(n), sMaskOff = spart(n * 8), sMaskWords = spart(n * 4), sEqOff = spart(n * 8), sEdReads = spart(n * sizeof(EdRead));
		small.p = g_readPinnedBlocks.get(sat, device, small.bytes);
		char* S = (char*)small.p;
		uint64_t* hostOff = (uint64_t*)(S + sOff);
		uint32_t* hostNameOff = (uint32_t*)(S + sNameOff);
		hostOff[0] = 0; hostNameOff[0] = 0;
		if (v.nLines) {
			HIP_CHECK(hipEventRecord(ev.a, q));
			HIP_CHECK(fxBuildRecords(q, v, t, nHeaders, nRecords, (uint64_t*)(D + oReadOff), (uint32_t*)(D + oNameLen), (uint32_t*)(D + oNameOff)));
			HIP_CHECK(fxWriteNames(q, v, t, nRecords, (const uint32_t*)(D + oNameOff), D + oNames));
			HIP_CHECK(hipEventRecord(ev.b, q));
			HIP_CHECK(hipMemcpyAsync(hostOff, D + oReadOff, (n + 1) * 8, hipMemcpyDeviceToHost, q));
			HIP_CHECK(hipMemcpyAsync(hostNameOff, D + oNameOff, (n + 1) * 4, hipMemcpyDeviceToHost, q));
			HIP_CHECK(hipStreamSynchronize(q));
			addSegment();
		}
		const uint64_t namesBytes = hostNameOff[n];
		if (hostOff[n] != total || namesBytes + total > L) throw std::runtime_error("gc_reads_parse: the read offsets disagree with the base count");
		for (uint64_t r = 0; r < n; r++) if (hostOff[r + 1] < hostOff[r] || hostNameOff[r + 1] <= hostNameOff[r]) throw std::runtime_error("gc_reads_parse: offsets decrease");

		// ---- 4: the read batch, laid out as gc_reads_upload lays it out; the gather writes the bases where the upload's copy would have put them ----
		R->offsets.assign(hostOff, hostOff + n + 1);
		R->totalBases = total;
		R->maskOff.assign(n, 0);
		R->maskWords.assign(n, 0);
		uint64_t* hMaskOff = (uint64_t*)(S + sMaskOff); uint32_t* hMaskWords = (uint32_t*)(S + sMaskWords); uint64_t* hEqOff = (uint64_t*)(S + sEqOff); EdRead* hEdReads = (EdRead*)(S + sEdReads);
		uint64_t totalWords = 0, eqWords = 0;
		for (uint64_t r = 0; r < n; r++) {
			R->maskOff[r] = hMaskOff[r] = totalWords;
			R->maskWords[r] = hMaskWords[r] = (uint32_t)((hostOff[r + 1] - hostOff[r] + 63) / 64 + 1);
			totalWords += 8ull * hMaskWords[r];
			hEdReads[r] = EdRead { hostOff[r], eqWords, (uint32_t)(hostOff[r + 1] - hostOff[r]), hMaskWords[r] };
			hEqOff[r] = eqWords;
			eqWords += 4ull * hMaskWords[r];
		}
		size_t rat = 0;
		auto rpart = [&](size_t bytes) { const size_t here = rat; rat += round(bytes); return here; };
		const uint64_t total64 = total;
		const size_t oBases = rpart(2 * total64), oOffsets = rpart((n + 1) * sizeof(uint64_t)), oMasks = rpart(totalWords * sizeof(uint64_t)), oEqMasks = rpart(eqWords * sizeof(uint64_t)),
			oEdReads = rpart(n * sizeof(EdRead)), oPacked = rpart(((total64 >> 5) + 1) * sizeof(uint64_t)), oInvalid = rpart(((total64 >> 6) + 1) * sizeof(uint64_t)), oChunkRead = rpart(((total64 >> 6) + 1) * sizeof(uint32_t)),
			oMaskOff = rpart(n * sizeof(uint64_t)), oMaskWords = rpart(n * sizeof(uint32_t)), oEqOff = rpart(n * sizeof(uint64_t)), oReadInvalid = rpart(n);
		R->deviceBlock = g_readDeviceBlocks.get(rat, device, R->deviceBlockBytes);
		char* B = (char*)R->deviceBlock;
		R->devBases = B + oBases; R->devOffsets = (uint64_t*)(B + oOffsets); R->devMasks = (uint64_t*)(B + oMasks); R->devEqMasks = (uint64_t*)(B + oEqMasks); R->devEdReads = (EdRead*)(B + oEdReads);
		R->devPacked = (uint64_t*)(B + oPacked); R->devInvalid = (uint64_t*)(B + oInvalid); R->devChunkRead = (uint32_t*)(B + oChunkRead); R->devReadInvalid = (uint8_t*)(B + oReadInvalid);
		uint64_t* pMaskOff = (uint64_t*)(B + oMaskOff);
		uint32_t* pMaskWords = (uint32_t*)(B + oMaskWords);
		uint64_t* pEqOff = (uint64_t*)(B + oEqOff);
		R->devMaskOff = pMaskOff; R->devMaskWords = pMaskWords;
		HIP_CHECK(hipMemcpyAsync(R->devOffsets, hostOff, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, q));
		if (n) {
			HIP_CHECK(hipMemcpyAsync(pMaskOff, hMaskOff, n * sizeof(uint64_t), hipMemcpyHostToDevice, q));
			HIP_CHECK(hipMemcpyAsync(pMaskWords, hMaskWords, n * sizeof(uint32_t), hipMemcpyHostToDevice, q));
			HIP_CHECK(hipMemcpyAsync(pEqOff, hEqOff, n * sizeof(uint64_t), hipMemcpyHostToDevice, q));
			HIP_CHECK(hipMemcpyAsync(R->devEdReads, hEdReads, n * sizeof(EdRead), hipMemcpyHostToDevice, q));
		}
		HIP_CHECK(hipEventRecord(ev.a, q));
		if (v.nLines) HIP_CHECK(fxGatherBases(q, v, t, total, R->devBases));
		launchPackReads(q, R->devOffsets, (uint32_t)n, total, R->devBases, pMaskOff, pMaskWords, R->devMasks, pEqOff, R->devEqMasks, R->devReadInvalid, R->devPacked, R->devInvalid, R->devChunkRead);
		HIP_CHECK(hipEventRecord(ev.b, q));
		R->invalid.assign(n, 0);
		if (n) HIP_CHECK(hipMemcpyAsync(S + sInvalid, R->devReadInvalid, n, hipMemcpyDeviceToHost, q));
		if (total) HIP_CHECK(hipMemcpyAsync(H, R->devBases, total, hipMemcpyDeviceToHost, q));
		if (namesBytes) HIP_CHECK(hipMemcpyAsync(H + total, D + oNames, namesBytes, hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipStreamSynchronize(q));
		addSegment();
		if (n) memcpy(R->invalid.data(), S + sInvalid, n);
		if (src.done) src.done(devText, consumed, q);

		// ---- the host's table: one allocation, the struct | offsets | name_off | bases | names ----
		const size_t tHead = (sizeof(gc_fastx_table) + 15) & ~(size_t)15, tArr = (n + 1) * sizeof(uint64_t);
		char* mem = (char*)malloc(tHead + 2 * tArr + total + namesBytes + 2);
		if (!mem) throw std::runtime_error("gc_reads_parse: out of host memory");
		T = (gc_fastx_table*)mem;
		T->n_reads = n; T->consumed = consumed; T->kernel_ms = kernelMs;
		T->offsets = (uint64_t*)(mem + tHead); T->name_off = (uint64_t*)(mem + tHead + tArr); T->bases = mem + tHead + 2 * tArr; T->names = T->bases + total + 1;
		memcpy(T->offsets, hostOff, tArr);
		for (uint64_t r = 0; r <= n; r++) T->name_off[r] = hostNameOff[r];
		if (total) memcpy(T->bases, H, total);
		T->bases[total] = 0;
		if (namesBytes) memcpy(T->names, H + total, namesBytes);
		T->names[namesBytes] = 0;
		return (int)GC_OK;
	};
	int rc = guarded([&]() { try { return body(); } catch (const InvalidInput& e) { return fail(GC_ERR_INVALID, e.what()); } });
	if (rc != GC_OK) {
		if (uploadStream) (void)hipStreamSynchronize(uploadStream);
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

struct BgzfHeld { BlockCache* cache; void* p = nullptr; size_t bytes = 0; int device = 0; hipStream_t q = nullptr;
	~BgzfHeld() { if (p) { (void)hipStreamSynchronize(q); cache->put(p, bytes, device); } } };   // (waits: a copy or kernel of a failed call may still use the block)

// The blocks of the scan from data into devText (outOff counts from there), with work on q; waits for it. Throws InvalidInput naming the first bad block. lastByte, if
// asked for, is the byte at devText[lastAt]. Times: the copy to the staging block and up (uploadMs), the kernel (kernelMs).
static void bgzfInflateTo(hipStream_t q, int device, const uint8_t* data, const BgzfScan& s, uint8_t* devText, uint64_t lastAt, char* lastByte, double& uploadMs, double& kernelMs)
{
	using namespace gcdev;
	const size_t nBlocks = s.blocks.size();
	auto round = [](size_t bytes) { return (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255; };
	const size_t oTable = round(s.consumed), oStatus = oTable + round(nBlocks * sizeof(InfBlock)), total = oStatus + round(nBlocks * sizeof(uint32_t) + 16);
	BgzfHeld dev { &g_readDeviceBlocks, nullptr, 0, device, q }, pin { &g_readPinnedBlocks, nullptr, 0, device, q };
	struct Events { hipEvent_t a = nullptr, b = nullptr, c = nullptr; ~Events() { for (hipEvent_t e : { a, b, c }) if (e) (void)hipEventDestroy(e); } } ev;
	HIP_CHECK(hipEventCreate(&ev.a)); HIP_CHECK(hipEventCreate(&ev.b)); HIP_CHECK(hipEventCreate(&ev.c));
	pin.p = g_readPinnedBlocks.get(total, device, pin.bytes);
	dev.p = g_readDeviceBlocks.get(total, device, dev.bytes);
	uint8_t* H = (uint8_t*)pin.p;
	uint8_t* D = (uint8_t*)dev.p;
	const auto t0 = std::chrono::steady_clock::now();
	memcpy(H, data, s.consumed);
	if (nBlocks) memcpy(H + oTable, s.blocks.data(), nBlocks * sizeof(InfBlock));
	const double stageMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	uint32_t* hostStatus = (uint32_t*)(H + oStatus);
	HIP_CHECK(hipEventRecord(ev.a, q));
	HIP_CHECK(hipMemcpyAsync(D, H, oStatus, hipMemcpyHostToDevice, q));
	HIP_CHECK(hipMemsetAsync(D + oStatus, 0xff, nBlocks * sizeof(uint32_t) + 16, q));
	HIP_CHECK(hipEventRecord(ev.b, q));
	HIP_CHECK(infLaunch(q, D, (const InfBlock*)(D + oTable), (uint32_t)nBlocks, devText, (uint32_t*)(D + oStatus)));
	HIP_CHECK(hipEventRecord(ev.c, q));
	HIP_CHECK(hipMemcpyAsync(hostStatus, D + oStatus, nBlocks * sizeof(uint32_t) + 16, hipMemcpyDeviceToHost, q));
	char* hostLast = (char*)(H + oStatus + nBlocks * sizeof(uint32_t));   // (the 16 spare bytes behind the status words)
	if (lastByte) HIP_CHECK(hipMemcpyAsync(hostLast, devText + lastAt, 1, hipMemcpyDeviceToHost, q));
	HIP_CHECK(hipStreamSynchronize(q));
	float ms = 0;
	HIP_CHECK(hipEventElapsedTime(&ms, ev.a, ev.b)); uploadMs = stageMs + ms;
	HIP_CHECK(hipEventElapsedTime(&ms, ev.b, ev.c)); kernelMs = ms;
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
			BgzfHeld devText { &g_readDeviceBlocks, nullptr, 0, device, q };
			devText.p = g_readDeviceBlocks.get(s.textBytes + 256, device, devText.bytes);
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

int gc_reads_parse_bgzf(const char* head, uint64_t head_len, const void* data, uint64_t len, int32_t format, uint32_t flags,
	gc_reads** reads, gc_fastx_table** table, char** tail, uint64_t* tail_len, uint64_t* consumed, gc_bgzf_stats* stats)
{
	if (!reads || !table || !tail || !tail_len || !consumed || (!head && head_len) || (!data && len)) return fail(GC_ERR_INVALID, "null argument");
	*reads = nullptr; *table = nullptr; *tail = nullptr; *tail_len = 0; *consumed = 0;
	if (stats) *stats = gc_bgzf_stats {};
	if (format != GC_FASTX_FASTA && format != GC_FASTX_FASTQ) return fail(GC_ERR_INVALID, "gc_reads_parse_bgzf: format is GC_FASTX_FASTA or GC_FASTX_FASTQ");
	if (flags & ~(uint32_t)GC_FASTX_FINAL) return fail(GC_ERR_INVALID, "gc_reads_parse_bgzf: unknown flag bits");
	BgzfScan s;
	const auto t0 = std::chrono::steady_clock::now();
	try { bgzfScan((const uint8_t*)data, len, head_len, s); }
	catch (const InvalidInput& e) { return fail(GC_ERR_INVALID, std::string("gc_reads_parse_bgzf: ") + e.what()); }
	catch (const std::exception& e) { return fail(GC_ERR_INTERNAL, e.what()); }
	const double scanMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	if (head_len >= 0xfffffff0ull || head_len + s.textBytes >= 0xfffffff0ull)
		return fail(GC_ERR_INVALID, "gc_reads_parse_bgzf: the loader uses 32-bit positions: head and inflated text must stay below 2^32 - 16 bytes");
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
			catch (const InvalidInput& e) { throw InvalidInput(std::string("gc_reads_parse_bgzf: ") + e.what()); }
		}
		return last;
	};
	src.done = [&](const char* devText, uint32_t textConsumed, hipStream_t q) {
		tailBytes = src.len - textConsumed;
		tailMem = (char*)malloc(tailBytes + 1);
		if (!tailMem) throw std::runtime_error("gc_reads_parse_bgzf: out of host memory");
		if (tailBytes) { HIP_CHECK(hipMemcpyAsync(tailMem, devText + textConsumed, tailBytes, hipMemcpyDeviceToHost, q)); HIP_CHECK(hipStreamSynchronize(q)); }
		tailMem[tailBytes] = 0;
	};
	const int rc = readsParseFrom(src, format, flags, reads, table);
	if (rc != GC_OK) { free(tailMem); return rc; }
	*tail = tailMem; *tail_len = tailBytes; *consumed = s.consumed;
	if (stats) { stats->blocks = s.blocks.size(); stats->inflated_bytes = s.textBytes; stats->scan_ms = scanMs; stats->upload_ms = uploadMs; stats->kernel_ms = kernelMs; }
	return GC_OK;
}

// ---- seed hits from the host's own seeder -------------------------------------------------------------------
int gc_seeds_upload(const gc_graph* G, const gc_reads* R, const gc_seed_hit* hits, const uint64_t* read_hit_off, uint64_t n_reads, gc_seeds** out)
{
	static_assert(sizeof(gc_seed_hit) == sizeof(SeedHit) && sizeof(SeedHit) == 24, "gc_seed_hit is what k_seed_resolve reads");
	// host checks first: a malformed call is GC_ERR_INVALID whether or not a device is present
	if (!G || !R || !read_hit_off || !out) return fail(GC_ERR_INVALID, "null argument");
	*out = nullptr;
	if (n_reads != R->offsets.size() - 1) return fail(GC_ERR_INVALID, "gc_seeds_upload: n_reads differs from the read batch's");
	if (read_hit_off[0] != 0) return fail(GC_ERR_INVALID, "gc_seeds_upload: read_hit_off must start at 0");
	for (uint64_t r = 0; r < n_reads; r++) if (read_hit_off[r + 1] < read_hit_off[r]) return fail(GC_ERR_INVALID, "gc_seeds_upload: read_hit_off decreases at read " + std::to_string(r));
	const uint64_t nHits = read_hit_off[n_reads];
	if (nHits >= 0xfffffff0ull) return fail(GC_ERR_INVALID, "gc_seeds_upload: 2^32 hits or more; split the batch");
	if (nHits && !hits) return fail(GC_ERR_INVALID, "null argument");
	for (uint64_t r = 0; r < n_reads; r++) {
		// the seed goodness is a 32-bit word: a cluster's matching base pairs are at most its first seed's match_len plus the read positions it spans, and any hit of the cluster
		// adds its own raw goodness to them (src/GraphAligner.h:273-287)
		const uint64_t len = R->offsets[r + 1] - R->offsets[r];
		uint64_t longest = 0, best = 0, bestAt = 0;
		for (uint64_t i = read_hit_off[r]; i < read_hit_off[r + 1]; i++) {
			if (hits[i].match_len > 0x7fffffffu) return fail(GC_ERR_INVALID, "gc_seeds_upload: read " + std::to_string(r) + " hit " + std::to_string(i - read_hit_off[r]) + ": match_len of 2^31 or more");
			longest = std::max<uint64_t>(longest, hits[i].match_len);
			if (hits[i].raw_goodness >= best) { best = hits[i].raw_goodness; bestAt = i; }
		}
		if (longest + len + best > 0xffffffffull)
			return fail(GC_ERR_INVALID, "gc_seeds_upload: read " + std::to_string(r) + " hit " + std::to_string(bestAt - read_hit_off[r]) + ": raw_goodness too large for the 32-bit seed goodness (match_len + read length + raw_goodness must stay below 2^32)");
	}
	gc_seeds* H = new gc_seeds();
	int rc = guarded([&]() {
		requireDevice();
		HIP_CHECK(hipGetDevice(&H->device));
		H->nHits = nHits;
		H->readOffsets = R->offsets;
		std::vector<uint32_t> off32(n_reads + 1);
		for (uint64_t r = 0; r <= n_reads; r++) off32[r] = (uint32_t)read_hit_off[r];
		size_t at = 0;
		auto part = [&](size_t bytes) { const size_t here = at; at += (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255; return here; };
		const size_t oOff = part((n_reads + 1) * sizeof(uint32_t)), oArrays = part(5 * nHits * sizeof(uint32_t)), oBad = part(sizeof(unsigned long long)), oHits = part(nHits * sizeof(SeedHit));
		HIP_CHECK(hipMalloc(&H->block, at));
		char* D = (char*)H->block;
		H->devReadHitOff = (uint32_t*)(D + oOff);
		uint32_t* arrays = (uint32_t*)(D + oArrays);
		H->dev = SeedHitArrays { arrays, arrays + nHits, arrays + 2 * nHits, arrays + 3 * nHits, arrays + 4 * nHits };
		unsigned long long* dBad = (unsigned long long*)(D + oBad);
		SeedHit* dHits = (SeedHit*)(D + oHits);   // (the raw records stay in the block's tail: 24 B per hit beside the 20 B the glue reads)
		H->devHits = dHits;
		hipStream_t q = threadStream(H->device);
		unsigned long long bad = ~0ull;
		HIP_CHECK(hipMemcpyAsync(H->devReadHitOff, off32.data(), (n_reads + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, q));
		HIP_CHECK(hipMemcpyAsync(dBad, &bad, sizeof(bad), hipMemcpyHostToDevice, q));
		if (nHits) HIP_CHECK(hipMemcpyAsync(dHits, hits, nHits * sizeof(SeedHit), hipMemcpyHostToDevice, q));
		const SeedLookup lookup { G->dev.origSize, G->dev.lookupOff, G->dev.lookup, G->dev.nodeOffset, (uint32_t)G->hOrigSize.size() };
		launchSeedResolve(q, lookup, dHits, nHits, H->devReadHitOff, (uint32_t)n_reads, R->devOffsets, H->dev, dBad);
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipMemcpyAsync(&bad, dBad, sizeof(bad), hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipStreamSynchronize(q));
		if (bad != ~0ull) {
			const uint64_t i = bad >> 2;
			const uint64_t r = (uint64_t)(std::upper_bound(read_hit_off, read_hit_off + n_reads + 1, i) - read_hit_off) - 1;
			const char* what[] = { "", "no such node in the graph", "node_offset is not inside the original node", "seq_pos is not inside the read" };
			return fail(GC_ERR_INVALID, "gc_seeds_upload: read " + std::to_string(r) + " hit " + std::to_string(i - read_hit_off[r]) + ": " + what[bad & 3]);
		}
		return (int)GC_OK;
	});
	if (rc != GC_OK) { delete H; return rc; }
	*out = H;
	return GC_OK;
}
void gc_seeds_destroy(gc_seeds* s) { delete s; }

int gc_seeds_hits(const gc_seeds* s, gc_seed_hit** hits, uint64_t** read_hit_off, uint64_t* n_reads)
{
	if (!s || !hits || !read_hit_off || !n_reads) return fail(GC_ERR_INVALID, "null argument");
	*hits = nullptr; *read_hit_off = nullptr;
	const uint64_t n = s->readOffsets.size() - 1;
	std::vector<uint32_t> off32(n + 1);
	gc_seed_hit* h = mallocArray<gc_seed_hit>(s->nHits);
	uint64_t* off = mallocArray<uint64_t>(n + 1);
	int rc = guarded([&]() {
		requireDevice();
		HIP_CHECK(hipMemcpy(off32.data(), s->devReadHitOff, (n + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
		if (s->nHits) HIP_CHECK(hipMemcpy(h, s->devHits, s->nHits * sizeof(gc_seed_hit), hipMemcpyDeviceToHost));
		return (int)GC_OK;
	});
	if (rc != GC_OK) { free(h); free(off); return rc; }
	for (uint64_t r = 0; r <= n; r++) off[r] = off32[r];
	*hits = h; *read_hit_off = off; *n_reads = n;
	return GC_OK;
}
double gc_seeds_kernel_ms(const gc_seeds* s) { return s ? s->kernelMs : 0; }

// ---- the MUM / MEM seeder (the reference's MummerSeeder, src/MummerSeeder.cpp) ---------------
// what gc_mxm_index_create and gc_mxm_index_open share. `who`: the entry point's name for the messages; cachePrefix empty: no cache
static int mxmIndexOpen(const char* who, const gc_graph* G, int32_t build, const std::string& cachePrefix, gc_mxm_index** out)
{
	// the forward original segments, from what the graph holds: bigraph id 2 * nodeID, its split nodes in offset order (64-letter chunks)
	const size_t nB = G->hOrigSize.size();
	uint64_t letters = 0;
	std::vector<uint32_t> ids;
	for (size_t id = 0; id < nB; id += 2) if (G->hLookupOff[id + 1] > G->hLookupOff[id]) { ids.push_back((uint32_t)id); letters += (uint64_t)G->hOrigSize[id] + 1; }
	if (letters >= 0xfffffff0ull) return fail(GC_ERR_INVALID, std::string(who) + ": a text of 2^32 - 16 letters or more (the segments and one separator each) does not fit the index's 32-bit positions");
	const std::string cachePath = cachePrefix.empty() ? std::string() : gc::mxmCachePath(cachePrefix);
	const bool load = !cachePath.empty() && gc::mxmCacheExists(cachePath);
	// (a host check, before a device is needed; nothing falls back to the host build by itself)
	if (!load && build == GC_MXM_BUILD_DEVICE && !gc::mxmDeviceBuildTakes(letters))
		return fail(GC_ERR_INVALID, std::string(who) + ": the device build takes a text of fewer than 2^31 - 1 letters (hipCUB counts in int) and this one has " + std::to_string(letters) + "; build it on the host (GC_MXM_BUILD_HOST)");
	gc_mxm_index* X = new gc_mxm_index();
	int rc = guarded([&]() {
		try {
		requireDevice();
		HIP_CHECK(hipGetDevice(&X->device));
		X->graph = G;
		const auto t0 = std::chrono::steady_clock::now();
		const uint32_t n = (uint32_t)letters;
		std::vector<uint8_t> codes(n, 0);
		X->nodeStart.resize(ids.size() + 1);
		X->nodeId.resize(ids.size());
		uint32_t at = 0;
		for (size_t k = 0; k < ids.size(); k++) { X->nodeStart[k] = at; X->nodeId[k] = (int32_t)(ids[k] / 2); at += G->hOrigSize[ids[k]] + 1; }
		X->nodeStart[ids.size()] = n;
		const gc::AlignmentGraph& g = G->host;
		WorkerPool::instance().run(ids.size(), [&](size_t k, size_t) {
			uint8_t* dst = codes.data() + X->nodeStart[k];
			for (uint32_t e = G->hLookupOff[ids[k]]; e < G->hLookupOff[ids[k] + 1]; e++) {
				const uint32_t node = G->hLookup[e];
				const size_t len = g.nodeLength[node], off = g.nodeOffset[node];
				for (size_t j = 0; j < len; j++) dst[off + j] = gc::mxmRefCode(g.NodeSequences(node, j));
			}
		});
		const uint64_t fingerprint = cachePath.empty() ? 0 : gc::mxmTextFingerprint(codes.data(), n);
		hipStream_t q = threadStream(X->device);
		MxmIndexView& d = X->dev;
		d.n = n; d.nNodes = (uint32_t)ids.size(); d.prefixLen = gc::MXM_PREFIX_LEN;
		auto upRaw = [&](const auto* src, size_t count) {
			std::remove_const_t<std::remove_pointer_t<decltype(src)>>* p = nullptr;
			const size_t bytes = std::max<size_t>(count, 1) * sizeof(*src);
			HIP_CHECK(hipMalloc((void**)&p, bytes));
			X->allocations.push_back((void*)p);
			X->deviceBytes += bytes;
			if (count) HIP_CHECK(hipMemcpy(p, src, count * sizeof(*src), hipMemcpyHostToDevice));
			return p;
		};
		auto up = [&](const auto& v) { return upRaw(v.data(), v.size()); };
		if (load) {
			gc::MxmCacheFile file;
			gc::mxmCacheLoad(cachePath, file, &fingerprint);
			// (the fingerprint covers every letter and separator, so the segment starts agree; the node ids are compared on their own)
			if (file.info.n != n || file.info.segments != ids.size() || memcmp(file.nodeStart, X->nodeStart.data(), (ids.size() + 1) * 4) != 0 || memcmp(file.nodeId, X->nodeId.data(), ids.size() * 4) != 0)
				throw gc::MxmCacheError("MUM / MEM index cache " + cachePath + ": segment table mismatch (the cache was built from another graph)");
			X->buildSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
			X->buildMode = 2;
			d.sa = upRaw(file.sa, n); d.packed = upRaw(file.packed, file.packedWords); d.invalid = upRaw(file.invalid, file.invalidWords);
		} else {
			std::vector<uint32_t> sa;
			std::vector<uint64_t> packed, invalid;
			const auto tSa = std::chrono::steady_clock::now();
			if (build == GC_MXM_BUILD_DEVICE) {
				uint32_t* dSa = nullptr;
				HIP_CHECK(hipMalloc((void**)&dSa, std::max<size_t>(n, 1) * sizeof(uint32_t)));
				X->allocations.push_back(dSa);
				X->deviceBytes += std::max<size_t>(n, 1) * sizeof(uint32_t);
				MxmSaBuild info;
				HIP_CHECK(launchMxmSuffixArray(q, codes.data(), n, dSa, info));
				X->saSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - tSa).count();
				gc::mxmPackText(codes.data(), n, packed, invalid);
				X->buildRounds = info.rounds; X->buildScratchBytes = info.scratchBytes; X->buildMode = 1;
				d.sa = dSa;
			} else {
				auto parallelFor = [](size_t count, const std::function<void(size_t)>& body) { WorkerPool::instance().run(count, [&](size_t i, size_t) { body(i); }); };
				sa = gc::mxmSuffixArray(codes.data(), n, parallelFor, &X->buildRounds);
				X->saSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - tSa).count();
				gc::mxmPackText(codes.data(), n, packed, invalid);
			}
			X->buildSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
			if (build != GC_MXM_BUILD_DEVICE) d.sa = up(sa);
			d.packed = up(packed); d.invalid = up(invalid);
			if (!cachePath.empty()) {
				const auto t1 = std::chrono::steady_clock::now();
				if (build == GC_MXM_BUILD_DEVICE) { sa.resize(n); if (n) HIP_CHECK(hipMemcpy(sa.data(), d.sa, (size_t)n * 4, hipMemcpyDeviceToHost)); }
				gc::mxmCacheSave(cachePath, X->nodeStart, X->nodeId, packed, invalid, sa.data(), n, fingerprint);
				X->cacheSaveSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
			}
		}
		d.nodeStart = up(X->nodeStart); d.nodeId = up(X->nodeId);
		uint32_t* table = nullptr;
		const size_t tableBytes = ((size_t)2 << (2 * d.prefixLen)) * sizeof(uint32_t);
		HIP_CHECK(hipMalloc((void**)&table, tableBytes));
		X->allocations.push_back(table);
		X->deviceBytes += tableBytes;
		d.prefix = table;
		HIP_CHECK(hipMemsetAsync(table, 0, tableBytes, q));
		launchMxmPrefixTable(q, d, table);
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipStreamSynchronize(q));
		return (int)GC_OK;
		} catch (const gc::MxmCacheError& e) {
			return fail(GC_ERR_GRAPH, e.what());   // (a cache that cannot be used or written: never used half, never overwritten)
		}
	});
	if (rc != GC_OK) { delete X; return rc; }
	*out = X;
	return GC_OK;
}

int gc_mxm_index_create(const gc_graph* G, gc_mxm_index** out)
{
	if (!G || !out) return fail(GC_ERR_INVALID, "null argument");
	*out = nullptr;
	return mxmIndexOpen("gc_mxm_index_create", G, GC_MXM_BUILD_HOST, std::string(), out);
}

void gc_mxm_options_default(gc_mxm_options* o)
{
	if (!o) return;
	o->build = GC_MXM_BUILD_HOST; o->reserved = 0; o->cache_prefix = nullptr;
}

int gc_mxm_index_open(const gc_graph* G, const gc_mxm_options* o, gc_mxm_index** out)
{
	// host checks first: a malformed call is GC_ERR_INVALID whether or not a device is present
	if (!G || !o || !out) return fail(GC_ERR_INVALID, "null argument");
	*out = nullptr;
	if (o->build != GC_MXM_BUILD_HOST && o->build != GC_MXM_BUILD_DEVICE) return fail(GC_ERR_INVALID, "gc_mxm_index_open: build is neither GC_MXM_BUILD_HOST nor GC_MXM_BUILD_DEVICE");
	if (o->reserved != 0) return fail(GC_ERR_INVALID, "gc_mxm_index_open: reserved must be 0");
	return mxmIndexOpen("gc_mxm_index_open", G, o->build, o->cache_prefix ? std::string(o->cache_prefix) : std::string(), out);
}

int gc_mxm_cache_check(const char* cache_prefix, uint64_t* info)
{
	if (!cache_prefix || !*cache_prefix) return fail(GC_ERR_INVALID, "gc_mxm_cache_check: no cache prefix");
	const std::string path = gc::mxmCachePath(cache_prefix);
	try {
		gc::MxmCacheFile file;
		gc::mxmCacheLoad(path, file);
		if (gc::mxmCacheTextFingerprint(file) != file.info.fingerprint) throw gc::MxmCacheError("MUM / MEM index cache " + path + ": the stored text does not have the stored fingerprint");
		if (info) { info[0] = file.info.version; info[1] = file.info.n; info[2] = file.info.segments; info[3] = file.info.fileBytes; info[4] = file.info.fingerprint; }
	} catch (const std::exception& e) {
		return fail(GC_ERR_GRAPH, e.what());
	}
	return GC_OK;
}
void gc_mxm_index_destroy(gc_mxm_index* x) { delete x; }

int gc_mxm_index_array(const gc_mxm_index* X, const char* name, int64_t** out, uint64_t* count)
{
	if (!X || !name || !out || !count) return fail(GC_ERR_INVALID, "null argument");
	const std::string nm = name;
	std::vector<int64_t> v;
	if (nm == "node_start") v.assign(X->nodeStart.begin(), X->nodeStart.end());
	else if (nm == "node_id") v.assign(X->nodeId.begin(), X->nodeId.end());
	else if (nm == "bytes") v.push_back((int64_t)X->deviceBytes);
	else if (nm == "build_us") v.push_back((int64_t)(X->buildSeconds * 1e6));
	else if (nm == "prefix_len") v.push_back((int64_t)X->dev.prefixLen);
	else if (nm == "sa_us") v.push_back((int64_t)(X->saSeconds * 1e6));
	else if (nm == "build_mode") v.push_back((int64_t)X->buildMode);
	else if (nm == "build_rounds") v.push_back((int64_t)X->buildRounds);
	else if (nm == "build_scratch_bytes") v.push_back((int64_t)X->buildScratchBytes);
	else if (nm == "cache_save_us") v.push_back((int64_t)(X->cacheSaveSeconds * 1e6));
	else if (nm == "sa") {
		std::vector<uint32_t> sa(X->dev.n);
		int rc = guarded([&]() { requireDevice(); if (X->dev.n) HIP_CHECK(hipMemcpy(sa.data(), X->dev.sa, (size_t)X->dev.n * 4, hipMemcpyDeviceToHost)); return (int)GC_OK; });
		if (rc != GC_OK) return rc;
		v.assign(sa.begin(), sa.end());
	}
	else return fail(GC_ERR_INVALID, "unknown index array " + nm);
	*out = mallocArray<int64_t>(v.size());
	memcpy(*out, v.data(), v.size() * sizeof(int64_t));
	*count = v.size();
	return GC_OK;
}

int gc_seeds_mxm(const gc_graph* G, const gc_mxm_index* X, const gc_reads* R, int32_t mode, uint64_t max_count, uint32_t min_len, gc_seeds** out)
{
	// host checks first: a malformed call is GC_ERR_INVALID whether or not a device is present
	if (!G || !X || !R || !out) return fail(GC_ERR_INVALID, "null argument");
	*out = nullptr;
	if (mode != GC_MXM_MUM && mode != GC_MXM_MEM) return fail(GC_ERR_INVALID, "gc_seeds_mxm: mode is neither GC_MXM_MUM nor GC_MXM_MEM");
	if (min_len < 2) return fail(GC_ERR_INVALID, "gc_seeds_mxm: min_len must be at least 2");
	if (max_count == 0) return fail(GC_ERR_INVALID, "gc_seeds_mxm: max_count must be at least 1 (UINT64_MAX: all)");
	if (X->graph != G) return fail(GC_ERR_INVALID, "gc_seeds_mxm: the index was built from another graph");
	const uint64_t nReads = R->offsets.size() - 1;
	// a read's tiles: 64 query positions of one strand each, forward strand first; none for a read shorter than min_len or with a letter outside the alphabet
	std::vector<uint32_t> tileOff(nReads + 1, 0);
	uint64_t tiles = 0;
	for (uint64_t r = 0; r < nReads; r++) {
		const uint64_t len = R->offsets[r + 1] - R->offsets[r];
		// (a hit's match_len and raw_goodness are at most the read's length, and match_len + read length + raw_goodness must stay below 2^32 as at upload)
		if (len >= 0x40000000ull) return fail(GC_ERR_INVALID, "gc_seeds_mxm: read " + std::to_string(r) + " has 2^30 letters or more");
		tileOff[r] = (uint32_t)tiles;
		if (len >= min_len && !R->invalid[r]) tiles += 2 * ((len - min_len + 1 + 63) / 64);
		if (tiles >= 0x7ffffff0ull) return fail(GC_ERR_INVALID, "gc_seeds_mxm: too many query positions in one batch; split the batch");
	}
	tileOff[nReads] = (uint32_t)tiles;
	gc_seeds* H = new gc_seeds();
	int rc = guarded([&]() {
		requireDevice();
		HIP_CHECK(hipGetDevice(&H->device));
		H->readOffsets = R->offsets;
		hipStream_t q = threadStream(H->device);
		DeviceBuffer dTileOff;
		uint32_t* pTileOff = dTileOff.reserve<uint32_t>(nReads + 1);
		HIP_CHECK(hipMemcpyAsync(pTileOff, tileOff.data(), (nReads + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, q));
		hipEvent_t e0 = nullptr, e1 = nullptr;
		struct Events { hipEvent_t &a, &b; ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } events { e0, e1 };
		HIP_CHECK(hipEventCreate(&e0)); HIP_CHECK(hipEventCreate(&e1));
		HIP_CHECK(hipEventRecord(e0, q));
		MxmSeedRun run;
		struct Drain { hipStream_t q; ~Drain() { (void)hipStreamSynchronize(q); } } drain { q };   // (before `run` frees its scratch and dTileOff goes: nothing of this call may still be running)
		HIP_CHECK(run.candidates(q, X->dev, R->devBases, R->devOffsets, pTileOff, (uint32_t)nReads, (uint32_t)tiles, mode, min_len));
		if (run.nCandidates > 0x7fffffffull) return fail(GC_ERR_INVALID, "gc_seeds_mxm: 2^31 matches or more in one batch; split the batch");
		uint64_t nHits = 0;
		HIP_CHECK(run.select(q, (uint32_t)nReads, max_count, nHits));
		H->nHits = nHits;
		size_t at = 0;
		auto part = [&](size_t bytes) { const size_t here = at; at += (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255; return here; };
		const size_t oOff = part((nReads + 1) * sizeof(uint32_t)), oArrays = part(5 * nHits * sizeof(uint32_t)), oBad = part(sizeof(unsigned long long)), oHits = part(nHits * sizeof(SeedHit));   // (gc_seeds_upload's layout)
		HIP_CHECK(hipMalloc(&H->block, at));
		char* D = (char*)H->block;
		H->devReadHitOff = (uint32_t*)(D + oOff);
		uint32_t* arrays = (uint32_t*)(D + oArrays);
		H->dev = SeedHitArrays { arrays, arrays + nHits, arrays + 2 * nHits, arrays + 3 * nHits, arrays + 4 * nHits };
		unsigned long long* dBad = (unsigned long long*)(D + oBad);
		H->devHits = (SeedHit*)(D + oHits);
		unsigned long long bad = ~0ull;
		HIP_CHECK(hipMemcpyAsync(dBad, &bad, sizeof(bad), hipMemcpyHostToDevice, q));
		HIP_CHECK(hipMemsetAsync(H->devReadHitOff, 0, (nReads + 1) * sizeof(uint32_t), q));
		HIP_CHECK(run.write(q, (uint32_t)nReads, nHits, H->devHits, H->devReadHitOff));
		const SeedLookup lookup { G->dev.origSize, G->dev.lookupOff, G->dev.lookup, G->dev.nodeOffset, (uint32_t)G->hOrigSize.size() };
		launchSeedResolve(q, lookup, H->devHits, nHits, H->devReadHitOff, (uint32_t)nReads, R->devOffsets, H->dev, dBad);
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipEventRecord(e1, q));
		HIP_CHECK(hipMemcpyAsync(&bad, dBad, sizeof(bad), hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipStreamSynchronize(q));
		float ms = 0;
		HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
		H->kernelMs = ms;
		if (bad != ~0ull) throw std::runtime_error("gc_seeds_mxm: a match does not resolve to a position of the graph (hit " + std::to_string(bad >> 2) + ")");   // (the index and the graph disagree: a bug, not an input)
		return (int)GC_OK;
	});
	if (rc != GC_OK) { delete H; return rc; }
	*out = H;
	return GC_OK;
}

// ---- seeds from GAM files (the reference's -s: src/Aligner.cpp:1169-1190, src/stream.hpp:81-123) --------------------
} // extern "C"

namespace {

struct SeedFileInvalid : std::runtime_error { using std::runtime_error::runtime_error; };
struct SeedFileUnreadable : std::runtime_error { using std::runtime_error::runtime_error; };

// a device array that grows by doubling and keeps what it holds
struct SeedStoreArray {
	void* p = nullptr;
	size_t cap = 0;
	void ensure(size_t used, size_t need, hipStream_t q)
	{
		if (need <= cap) return;
		const size_t want = std::max(need + 256, cap * 2);
		void* grown = nullptr;
		HIP_CHECK(hipMalloc(&grown, want));
		hipError_t e = used ? hipMemcpyAsync(grown, p, used, hipMemcpyDeviceToDevice, q) : hipSuccess;
		if (e == hipSuccess) e = hipStreamSynchronize(q);
		if (e != hipSuccess) { (void)hipFree(grown); HIP_CHECK(e); }
		if (p) (void)hipFree(p);
		p = grown; cap = want;
	}
	// the doubling's head room goes back before the store keeps the array
	void fit(size_t used, hipStream_t q)
	{
		if (!p || cap <= used + used / 16 + 4096) return;
		SeedStoreArray exact;
		exact.ensure(0, used, q);
		HIP_CHECK(hipMemcpyAsync(exact.p, p, used, hipMemcpyDeviceToDevice, q));
		HIP_CHECK(hipStreamSynchronize(q));
		std::swap(p, exact.p); std::swap(cap, exact.cap);
	}
	void* handOver(gc_seed_store& S) { void* r = p; if (r) { S.allocations.push_back(r); S.deviceBytes += cap; } p = nullptr; cap = 0; return r; }
	~SeedStoreArray() { if (p) (void)hipFree(p); }
};

double msSince(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// pieces in, a gc_seed_store out: every piece is uploaded, decoded into the growing arrays and dropped
struct SeedStoreBuilder {
	gc_seed_store& S;
	hipStream_t q;
	gc::Switches sw = gc::Switches::fromEnvironment();
	SeedStoreArray hits, hash, nameOff, nameLen, pool;
	DeviceBuffer piece, msgOff, nameStart, local, temp, flags;
	hipEvent_t e0 = nullptr, e1 = nullptr;
	uint64_t n = 0, poolUsed = 0;
	unsigned long long* dBad = nullptr;
	std::vector<uint64_t> fileFirst;   // the first message of every file among all messages
	double sinkMs = 0;

	SeedStoreBuilder(gc_seed_store& store, hipStream_t stream) : S(store), q(stream)
	{
		HIP_CHECK(hipEventCreate(&e0)); HIP_CHECK(hipEventCreate(&e1));
		dBad = flags.reserve<unsigned long long>(2);
		const unsigned long long none = ~0ull;
		HIP_CHECK(hipMemcpyAsync(dBad, &none, sizeof(none), hipMemcpyHostToDevice, q));
		HIP_CHECK(hipMemsetAsync(dBad + 1, 0, sizeof(unsigned long long), q));
		HIP_CHECK(hipStreamSynchronize(q));
	}
	~SeedStoreBuilder() { (void)hipStreamSynchronize(q); if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }

	void addPiece(const uint8_t* bytes, size_t len, const uint32_t* off, uint32_t count)
	{
		const auto t0 = std::chrono::steady_clock::now();
		if (n + count >= 0x7fffffffull) throw SeedFileInvalid("2^31 - 1 messages or more");
		uint8_t* dPiece = piece.reserve<uint8_t>(len + 16);   // (k_sf_decode stages whole 16-byte words)
		uint32_t* dOff = msgOff.reserve<uint32_t>((size_t)count + 1);
		HIP_CHECK(hipMemcpyAsync(dPiece, bytes, len, hipMemcpyHostToDevice, q));
		HIP_CHECK(hipMemcpyAsync(dOff, off, ((size_t)count + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, q));
		hits.ensure(n * sizeof(SeedHit), (n + count) * sizeof(SeedHit), q);
		hash.ensure(n * 8, (n + count) * 8, q);
		nameOff.ensure(n * 8, (n + count) * 8, q);
		nameLen.ensure(n * 4, (n + count) * 4, q);
		uint32_t* dStart = nameStart.reserve<uint32_t>(count);
		uint32_t* dLocal = local.reserve<uint32_t>(count);
		const size_t tempBytes = sfTempBytes(count, 0);
		void* dTemp = temp.reserve<char>(tempBytes);
		HIP_CHECK(hipStreamSynchronize(q));
		S.uploadMs += msSince(t0);
		uint32_t* lens = (uint32_t*)nameLen.p + n;
		HIP_CHECK(hipEventRecord(e0, q));
		HIP_CHECK(sfDecodePiece(q, dPiece, dOff, count, n, sw.testSeedfileHashBits, (SeedHit*)hits.p + n, (uint64_t*)hash.p + n, dStart, lens, dBad));
		HIP_CHECK(sfScanNameLengths(q, dTemp, tempBytes, lens, count, dLocal));
		uint32_t last[2] = { 0, 0 };
		HIP_CHECK(hipMemcpyAsync(&last[0], dLocal + (count - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipMemcpyAsync(&last[1], lens + (count - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipStreamSynchronize(q));
		const uint64_t total = (uint64_t)last[0] + last[1];   // (the names lie inside the piece: at most its bytes)
		pool.ensure(poolUsed, poolUsed + total, q);
		HIP_CHECK(sfCopyNames(q, dPiece, dOff, dStart, lens, dLocal, count, poolUsed, (uint8_t*)pool.p, (uint64_t*)nameOff.p + n));
		HIP_CHECK(hipEventRecord(e1, q));
		HIP_CHECK(hipStreamSynchronize(q));
		float ms = 0;
		HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
		S.decodeMs += ms;
		poolUsed += total;
		n += count;
		sinkMs += msSince(t0);
	}

	// after every file: the first message the device refused, by file and index
	void check()
	{
		unsigned long long bad = ~0ull;
		HIP_CHECK(hipMemcpyAsync(&bad, dBad, sizeof(bad), hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipStreamSynchronize(q));
		if (bad == ~0ull) return;
		const uint64_t i = bad >> 2;
		const size_t f = (size_t)(std::upper_bound(fileFirst.begin(), fileFirst.end(), i) - fileFirst.begin()) - 1;
		const char* what[] = { "", "has no mapping", "has a mapping without an edit", "does not parse as a vg::Alignment" };
		throw SeedFileInvalid("file " + std::to_string(f) + " message " + std::to_string(i - fileFirst[f]) + " " + what[bad & 3]);
	}

	void oneStream(uint32_t index, const std::function<void(gc::SeedFileFramer&)>& feed)
	{
		fileFirst.push_back(n);
		gc::SeedFileFramer framer(sw.testSeedfilePiece, [&](const uint8_t* bytes, size_t len, const uint32_t* off, uint32_t count, uint64_t) { addPiece(bytes, len, off, count); });
		try {
			feed(framer);
			framer.finish();
		} catch (const gc::SeedFileError& e) {
			throw SeedFileInvalid("file " + std::to_string(index) + ": " + e.what());
		} catch (const SeedFileInvalid& e) {
			throw SeedFileInvalid("file " + std::to_string(index) + ": " + e.what());
		}
		S.messages += framer.messages();
		S.seeds += framer.seeds();
		check();
	}

	void finish()
	{
		if (n) {
			SeedStoreArray sorted, order;
			sorted.ensure(0, n * 8, q);
			order.ensure(0, n * 4, q);
			const size_t tempBytes = sfTempBytes((uint32_t)n, 0);
			void* dTemp = temp.reserve<char>(tempBytes);
			uint32_t* dIota = local.reserve<uint32_t>(n);
			HIP_CHECK(hipEventRecord(e0, q));
			HIP_CHECK(sfSortStore(q, dTemp, tempBytes, (const uint64_t*)hash.p, (uint32_t)n, (uint64_t*)sorted.p, (uint32_t*)order.p, dIota, (uint32_t*)(dBad + 1)));
			HIP_CHECK(hipEventRecord(e1, q));
			uint32_t distinct = 0;
			HIP_CHECK(hipMemcpyAsync(&distinct, dBad + 1, sizeof(distinct), hipMemcpyDeviceToHost, q));
			HIP_CHECK(hipStreamSynchronize(q));
			float ms = 0;
			HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
			S.sortMs = ms;
			S.distinct = distinct;
			S.dev.sortedHash = (const uint64_t*)sorted.handOver(S);
			S.dev.order = (const uint32_t*)order.handOver(S);
		}
		hits.fit(n * sizeof(SeedHit), q); nameOff.fit(n * 8, q); nameLen.fit(n * 4, q); pool.fit(poolUsed, q);
		S.dev.hits = (const SeedHit*)hits.handOver(S);
		S.dev.nameOff = (const uint64_t*)nameOff.handOver(S);
		S.dev.nameLen = (const uint32_t*)nameLen.handOver(S);
		S.dev.namePool = (const uint8_t*)pool.handOver(S);
		S.dev.n = (uint32_t)n;
		S.dev.hashBits = sw.testSeedfileHashBits;
	}
};

// the file's inflated bytes into the framer: gzip or zlib by the header, concatenated members read through (as api._file_chunks reads a read file)
void seedFileInflate(const char* path, gc::SeedFileFramer& framer, SeedStoreBuilder& B)
{
	FILE* f = fopen(path, "rb");
	if (!f) throw SeedFileUnreadable(std::string("cannot open seeds file ") + path);
	struct Close { FILE* f; ~Close() { fclose(f); } } close { f };
	z_stream z;
	memset(&z, 0, sizeof(z));
	if (inflateInit2(&z, 47) != Z_OK) throw std::runtime_error("zlib: inflateInit2 failed");
	struct End { z_stream* z; ~End() { inflateEnd(z); } } end { &z };
	std::vector<uint8_t> in(1 << 20), out(4 << 20);
	bool inMember = false;
	for (;;) {
		const size_t got = fread(in.data(), 1, in.size(), f);
		if (!got) break;
		z.next_in = in.data(); z.avail_in = (uInt)got;
		while (z.avail_in) {
			z.next_out = out.data(); z.avail_out = (uInt)out.size();
			const auto t0 = std::chrono::steady_clock::now();
			const int rc = inflate(&z, Z_NO_FLUSH);
			B.S.inflateMs += msSince(t0);
			const size_t produced = out.size() - z.avail_out;
			if (rc != Z_OK && rc != Z_STREAM_END && !(rc == Z_BUF_ERROR && produced)) throw SeedFileInvalid(std::string("the stream is neither gzip nor zlib, or is damaged (") + (z.msg ? z.msg : "zlib error") + ")");
			inMember = rc != Z_STREAM_END;
			if (produced) {
				const auto t1 = std::chrono::steady_clock::now();
				const double sinkBefore = B.sinkMs;
				framer.push(out.data(), produced);
				B.S.frameMs += msSince(t1) - (B.sinkMs - sinkBefore);
			}
			if (rc == Z_STREAM_END && inflateReset(&z) != Z_OK) throw std::runtime_error("zlib: inflateReset failed");
		}
	}
	if (inMember) throw SeedFileInvalid("the file ends inside a compressed member");
}

int seedStoreMake(uint32_t n, const std::function<void(uint32_t, gc::SeedFileFramer&, SeedStoreBuilder&)>& feed, gc_seed_store** out)
{
	gc_seed_store* S = new gc_seed_store();
	int rc = guarded([&]() {
		try {
			requireDevice();
			HIP_CHECK(hipGetDevice(&S->device));
			SeedStoreBuilder B(*S, threadStream(S->device));
			for (uint32_t i = 0; i < n; i++) B.oneStream(i, [&](gc::SeedFileFramer& framer) { feed(i, framer, B); });
			B.finish();
			return (int)GC_OK;
		} catch (const SeedFileInvalid& e) {
			return fail(GC_ERR_INVALID, std::string("seeds file: ") + e.what());
		} catch (const SeedFileUnreadable& e) {
			return fail(GC_ERR_GRAPH, e.what());
		}
	});
	if (rc != GC_OK) { delete S; return rc; }
	*out = S;
	return GC_OK;
}

} // namespace

extern "C" {

int gc_seed_store_open(const char* const* paths, uint32_t n_paths, gc_seed_store** out)
{
	if (!out || (n_paths && !paths)) return fail(GC_ERR_INVALID, "null argument");
	*out = nullptr;
	for (uint32_t i = 0; i < n_paths; i++) if (!paths[i]) return fail(GC_ERR_INVALID, "null argument");
	return seedStoreMake(n_paths, [&](uint32_t i, gc::SeedFileFramer& framer, SeedStoreBuilder& B) { seedFileInflate(paths[i], framer, B); }, out);
}

int gc_seed_store_from_memory(const void* const* streams, const uint64_t* lens, uint32_t n, gc_seed_store** out)
{
	if (!out || (n && (!streams || !lens))) return fail(GC_ERR_INVALID, "null argument");
	*out = nullptr;
	for (uint32_t i = 0; i < n; i++) if (!streams[i] && lens[i]) return fail(GC_ERR_INVALID, "null argument");
	return seedStoreMake(n, [&](uint32_t i, gc::SeedFileFramer& framer, SeedStoreBuilder& B) {
		const auto t0 = std::chrono::steady_clock::now();
		const double sinkBefore = B.sinkMs;
		if (lens[i]) framer.push((const uint8_t*)streams[i], lens[i]);
		B.S.frameMs += msSince(t0) - (B.sinkMs - sinkBefore);
	}, out);
}

int gc_seed_store_info(const gc_seed_store* s, gc_seed_store_stats* o)
{
	if (!s || !o) return fail(GC_ERR_INVALID, "null argument");
	o->messages = s->messages; o->seeds = s->seeds; o->distinct_hashes = s->distinct; o->hbm_bytes = s->deviceBytes;
	o->inflate_ms = s->inflateMs; o->frame_ms = s->frameMs; o->upload_ms = s->uploadMs; o->decode_ms = s->decodeMs; o->sort_ms = s->sortMs;
	o->host_ms = s->inflateMs + s->frameMs; o->device_ms = s->decodeMs + s->sortMs;
	return GC_OK;
}
void gc_seed_store_destroy(gc_seed_store* s) { delete s; }

int gc_seeds_from_store(const gc_graph* G, const gc_seed_store* S, const gc_reads* R, const char* names, const uint64_t* name_off, uint64_t n_reads, gc_seeds** out)
{
	// host checks first: a malformed call is GC_ERR_INVALID whether or not a device is present
	if (!G || !S || !R || !name_off || !out) return fail(GC_ERR_INVALID, "null argument");
	*out = nullptr;
	if (n_reads != R->offsets.size() - 1) return fail(GC_ERR_INVALID, "gc_seeds_from_store: n_reads differs from the read batch's");
	if (n_reads >= 0xfffffff0ull) return fail(GC_ERR_INVALID, "gc_seeds_from_store: too many reads");
	if (name_off[0] != 0) return fail(GC_ERR_INVALID, "gc_seeds_from_store: name_off must start at 0");
	for (uint64_t r = 0; r < n_reads; r++) if (name_off[r + 1] <= name_off[r]) return fail(GC_ERR_INVALID, "gc_seeds_from_store: read " + std::to_string(r) + " has no name and terminator byte in name_off");
	const uint64_t nameBytes = name_off[n_reads];
	if (nameBytes && !names) return fail(GC_ERR_INVALID, "null argument");
	gc_seeds* H = new gc_seeds();
	int rc = guarded([&]() {
		requireDevice();
		HIP_CHECK(hipGetDevice(&H->device));
		H->readOffsets = R->offsets;
		hipStream_t q = threadStream(H->device);
		struct Drain { hipStream_t q; ~Drain() { (void)hipStreamSynchronize(q); } };
		DeviceBuffer dNames, dNameOff, dFirst, dCount, dOff64, dTemp;
		Drain drain { q };   // (before the buffers above go: nothing of this call may still be running)
		uint8_t* pNames = dNames.reserve<uint8_t>(nameBytes);
		uint64_t* pNameOff = dNameOff.reserve<uint64_t>(n_reads + 1);
		uint32_t* pFirst = dFirst.reserve<uint32_t>(n_reads);
		uint64_t* pCount = dCount.reserve<uint64_t>(n_reads + 1);
		uint64_t* pOff64 = dOff64.reserve<uint64_t>(n_reads + 1);
		const size_t tempBytes = sfTempBytes(0, (uint32_t)n_reads);
		void* pTemp = dTemp.reserve<char>(tempBytes);
		if (nameBytes) HIP_CHECK(hipMemcpyAsync(pNames, names, nameBytes, hipMemcpyHostToDevice, q));
		HIP_CHECK(hipMemcpyAsync(pNameOff, name_off, (n_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, q));
		hipEvent_t e0 = nullptr, e1 = nullptr;
		struct Events { hipEvent_t &a, &b; ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } events { e0, e1 };
		HIP_CHECK(hipEventCreate(&e0)); HIP_CHECK(hipEventCreate(&e1));
		HIP_CHECK(hipEventRecord(e0, q));
		HIP_CHECK(sfJoinCount(q, S->dev, pNames, pNameOff, (uint32_t)n_reads, pFirst, pCount));
		HIP_CHECK(sfJoinScan(q, pTemp, tempBytes, pCount, (uint32_t)n_reads, pOff64));
		uint64_t nHits = 0;
		HIP_CHECK(hipMemcpyAsync(&nHits, pOff64 + n_reads, sizeof(nHits), hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipStreamSynchronize(q));
		if (nHits >= 0xfffffff0ull) return fail(GC_ERR_INVALID, "gc_seeds_from_store: 2^32 hits or more; split the batch");
		H->nHits = nHits;
		size_t at = 0;
		auto part = [&](size_t bytes) { const size_t here = at; at += (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255; return here; };
		const size_t oOff = part((n_reads + 1) * sizeof(uint32_t)), oArrays = part(5 * nHits * sizeof(uint32_t)), oBad = part(3 * sizeof(unsigned long long)), oHits = part(nHits * sizeof(SeedHit));   // (gc_seeds_upload's layout)
		HIP_CHECK(hipMalloc(&H->block, at));
		char* D = (char*)H->block;
		H->devReadHitOff = (uint32_t*)(D + oOff);
		uint32_t* arrays = (uint32_t*)(D + oArrays);
		H->dev = SeedHitArrays { arrays, arrays + nHits, arrays + 2 * nHits, arrays + 3 * nHits, arrays + 4 * nHits };
		unsigned long long* dBad = (unsigned long long*)(D + oBad);   // resolve, match_len, raw_goodness
		H->devHits = (SeedHit*)(D + oHits);
		unsigned long long bad[3] = { ~0ull, ~0ull, ~0ull };
		HIP_CHECK(hipMemcpyAsync(dBad, bad, sizeof(bad), hipMemcpyHostToDevice, q));
		HIP_CHECK(sfJoinGather(q, S->dev, pNames, pNameOff, (uint32_t)n_reads, pFirst, pOff64, R->devOffsets, H->devHits, H->devReadHitOff, dBad + 1, dBad + 2));
		const SeedLookup lookup { G->dev.origSize, G->dev.lookupOff, G->dev.lookup, G->dev.nodeOffset, (uint32_t)G->hOrigSize.size() };
		launchSeedResolve(q, lookup, H->devHits, nHits, H->devReadHitOff, (uint32_t)n_reads, R->devOffsets, H->dev, dBad);
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipEventRecord(e1, q));
		HIP_CHECK(hipMemcpyAsync(bad, dBad, sizeof(bad), hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipStreamSynchronize(q));
		float ms = 0;
		HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
		H->kernelMs = ms;
		// gc_seeds_upload's order: its host checks read by read (a read's match_len before its raw_goodness), then the device's
		if (bad[1] != ~0ull || bad[2] != ~0ull) {
			const bool len = bad[1] != ~0ull && (bad[2] == ~0ull || (bad[1] >> 32) <= (bad[2] >> 32));
			const unsigned long long b = len ? bad[1] : bad[2];
			return fail(GC_ERR_INVALID, "gc_seeds_from_store: read " + std::to_string(b >> 32) + " hit " + std::to_string(b & 0xffffffffull) + ": " +
				(len ? "match_len of 2^31 or more" : "raw_goodness too large for the 32-bit seed goodness (match_len + read length + raw_goodness must stay below 2^32)"));
		}
		if (bad[0] != ~0ull) {
			const uint64_t i = bad[0] >> 2;
			std::vector<uint32_t> off32(n_reads + 1);
			HIP_CHECK(hipMemcpy(off32.data(), H->devReadHitOff, (n_reads + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
			const uint64_t r = (uint64_t)(std::upper_bound(off32.begin(), off32.end(), (uint32_t)i) - off32.begin()) - 1;
			const char* what[] = { "", "no such node in the graph", "node_offset is not inside the original node", "seq_pos is not inside the read" };
			return fail(GC_ERR_INVALID, "gc_seeds_from_store: read " + std::to_string(r) + " hit " + std::to_string(i - off32[r]) + ": " + what[bad[0] & 3]);
		}
		return (int)GC_OK;
	});
	if (rc != GC_OK) { delete H; return rc; }
	*out = H;
	return GC_OK;
}

// ---- the batch pipeline -----------------------------------------------------------------------------------

void gc_result_free(gc_result* r)
{
	if (!r) return;
	void* ptrs[] = { r->read_seed_off, r->seed_node, r->seed_offset, r->seed_seqpos, r->seed_goodness, r->read_anchor_off, r->anchor_x, r->anchor_y, r->anchor_path_off,
		r->anchor_path, r->anchor_first_node, r->anchor_first_offset, r->anchor_first_seqpos, r->anchor_last_node, r->anchor_last_offset, r->anchor_last_seqpos, r->anchor_score,
		r->anchor_trace_off, r->anchor_trace_node, r->anchor_trace_offset, r->anchor_trace_seqpos, r->anchor_trace_switch, r->read_chain_off, r->chain, r->chain_score,
		r->read_longall_off, r->longall_start, r->longall_end, r->longall_score, r->long_trace_off, r->long_trace_node, r->long_trace_offset, r->long_trace_seqpos, r->long_trace_switch,
		r->failed_assertion, r->seeds_extended, r->seeds_extended_long, r->read_path_off, r->path_node, r->path_first_offset, r->path_last_offset, r->path_cells,
		r->read_long_off, r->long_index, r->long_edit_distance, r->chain_edit_distance, r->chained_better,
		r->capacity_exceeded, r->read_chain_trace_off, r->chain_trace_node, r->chain_trace_offset, r->chain_trace_seqpos, r->chain_trace_switch, r->chain_aln_start, r->chain_aln_end,
		r->read_out_off, r->out_source, r->out_numbers, r->out_path_off, r->out_path_text, r->out_cigar_off, r->out_cigar_text, r->out_vg_off, r->out_vg_path, r->flatten_ties, r->flatten_ties_long };
	for (void* p : ptrs) g_resultBlocks.put(p);
	free(r);
}

// One batch through the whole path, stage by stage (r3: this was one 1 200-line function). A BatchRun holds what the stages share - the call's arguments, the sizes the seed
// stage leaves behind, the device and pinned-host buffers a later stage reads again - and every stage is one member function, in the batch's order:
//   seeds -> prepareWholeReadPass -> startWholeReadPass (the pass runs on its own host thread and stream from there: runLongRounds, then afterLongPass) -> [main thread, meanwhile]
//   fragmentPipeline -> resultsBack -> stitchAndChainDistances -> joinWholeReadPass -> chainedAlignments -> assemble.
// Capacities are per read (flags in the result), errors of the reference's own making per read or fragment (failed_assertion); only invalid arguments and device errors fail
// the call (they throw; gc_align_batch turns that into its return code, and ~BatchRun joins the pass thread first).

} // extern "C"
