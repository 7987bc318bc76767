// C entry points, a batch's alignments in the reference's formats: gc_format_gaf / _json / _gam / _gam_level, gc_format_gaf_trace, gc_format_vg_trace / _digraph,
// gc_graph_letters, gc_gzip_streams / _lz, and gzipGroupsOnDevice, the GAM groups' deflate staging; gc_format_corrected / _trace and gc_corrected_pieces, the corrected reads.
#include "../gc_runtime.hpp"
#include "../hip/gc_corrected_core.hpp"

extern "C" {

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
	gc::Arena d;
	const size_t oRaw = d.part(rawTotal), oRawOff = d.part((m + 1) * sizeof(uint64_t)), oLens = d.part(m * (size_t)std::max(260u, deflateLzLensStride())), oPlan = d.part(m * sizeof(uint2)), oOutOff = d.part((m + 1) * sizeof(uint64_t)), oOut = d.part(outBound);
	hipStream_t q = threadStream(device);
	HeldBlock deviceBlock(g_deflateDeviceBlocks, device, q), pinnedBlock(g_deflatePinnedBlocks, device, q);
	char* D = (char*)deviceBlock.acquire(d.bytes());
	gc::Arena h;
	const size_t hRaw = h.part(std::max<uint64_t>(rawTotal, outBound)), hRawOff = h.part((m + 1) * sizeof(uint64_t)), hPlan = h.part(m * sizeof(uint2)), hOutOff = h.part((m + 1) * sizeof(uint64_t));
	char* H = (char*)pinnedBlock.acquire(h.bytes());
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
	if (pieces && (r->device_output & 8) && kind == OUT_GAF && !(r->device_output & 3)) return fail(GC_ERR_INVALID, "the result was produced without the GAF pieces (gc_params::device_output & 3)");
	if (pieces && (r->device_output & 8) && kind != OUT_GAF && !(r->device_output & 4)) return fail(GC_ERR_INVALID, "the result was produced without the vg::Path bytes (gc_params::device_output & 4)");
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

// ---- corrected reads (GraphAligner's --corrected-out / --corrected-clipped-out)

// AddCorrected (src/GraphAligner.h:220-231) on the host: the plain loop over one trace
static std::string correctedPieceOnHost(const gc::AlignmentGraph& graph, const int32_t* node, const uint32_t* offset, const uint8_t* nodeSwitch, uint64_t n)
{
	std::string piece;
	gc::GraphLetters letters(graph);
	for (uint64_t i = 0; i < n; i++)
		if (gcdev::corrKeeps(i == 0, i ? node[i - 1] : 0, i ? offset[i - 1] : 0, i ? nodeSwitch[i - 1] : 0, node[i], offset[i])) piece += letters.at(node[i], offset[i]);
	return piece;
}
static char* mallocCopy(const std::string& s)
{
	char* buf = (char*)malloc(s.size() + 1);
	if (!buf) throw std::runtime_error("out of memory");
	memcpy(buf, s.data(), s.size());
	buf[s.size()] = 0;
	return buf;
}

int gc_format_corrected(const gc_graph* G, const gc_result* r, const char* const* read_names, const char* bases, const uint64_t* offsets, int clipped,
	char** out_text, uint64_t* out_len, uint64_t** rec_off, uint64_t* n_rec, uint64_t* n_chained_skipped)
{
	if (!G || !r || !read_names || !bases || !offsets || !out_text || !out_len) return fail(GC_ERR_INVALID, "null argument");
	const bool pieces = r->out_corrected_off != nullptr;   // the device spelled the pieces (gc_params::device_output & 8)
	if (!pieces && (!r->long_trace_off || !r->read_long_off || !r->long_index || !r->read_longall_off || (r->read_longall_off[r->n_reads] > 0 && r->long_trace_off[r->read_longall_off[r->n_reads]] == 0))) return fail(GC_ERR_INVALID, "gc_format_corrected needs a result with device_output & 8, or with long_pass, keep_traces and edit_distances");
	return guarded([&]() {
		const uint64_t n = r->n_reads;
		const size_t maxOverlap = 0;   // getDBGoverlap of the graphs this library loads (0M overlaps): getLongestOverlap is 0, nothing is trimmed
		std::vector<std::string> perRead(n);
		std::vector<std::vector<uint64_t>> recEnds(n);   // ends of the read's records inside perRead[i]
		std::atomic<uint64_t> skipped { 0 };
		WorkerPool::instance().run(n, [&](size_t i, size_t) {
			if (r->failed_assertion[i] || r->capacity_exceeded[i]) return;   // the reference `continue`s: no record
			std::string& text = perRead[i];
			const std::string id = read_names[i] ? read_names[i] : "";
			const char* raw = bases + offsets[i];
			const uint64_t rawLen = offsets[i + 1] - offsets[i];
			std::vector<std::string> spelled;            // pieces made here, on the host
			std::vector<gcdev::CorrPiece> list;
			if (r->chained_better[i]) {
				// the chained alignment replaces the whole-read ones (src/Aligner.cpp:901-920): a single item
				const uint64_t t0 = r->read_chain_trace_off ? r->read_chain_trace_off[i] : 0, t1 = r->read_chain_trace_off ? r->read_chain_trace_off[i + 1] : 0;
				if (t1 == t0) { skipped++; return; }   // result produced without chain_traces
				spelled.push_back(correctedPieceOnHost(G->host, r->chain_trace_node + t0, r->chain_trace_offset + t0, r->chain_trace_switch + t0, t1 - t0));
				list.push_back(gcdev::CorrPiece { r->chain_aln_start[i], r->chain_aln_end[i], nullptr, 0 });
			} else if (pieces) {
				for (uint64_t e = r->read_out_off[i]; e < r->read_out_off[i + 1]; e++)
					list.push_back(gcdev::CorrPiece { r->out_numbers[12 * e + 8], r->out_numbers[12 * e + 9], r->out_corrected_text + r->out_corrected_off[e], r->out_corrected_off[e + 1] - r->out_corrected_off[e] });
			} else {
				struct Item { uint32_t start; uint64_t aln; };
				std::vector<Item> items;
				for (uint64_t k = r->read_long_off[i]; k < r->read_long_off[i + 1]; k++) { const uint64_t a = r->read_longall_off[i] + r->long_index[k]; items.push_back(Item { r->longall_start[a], a }); }
				auto byStart = [](const Item& l, const Item& rr) { return l.start < rr.start; };
				std::sort(items.begin(), items.end(), byStart);   // src/Aligner.cpp:1003
				std::sort(items.begin(), items.end(), byStart);   // :1023
				for (const Item& it : items) {
					const uint64_t t0 = r->long_trace_off[it.aln], t1 = r->long_trace_off[it.aln + 1];
					spelled.push_back(correctedPieceOnHost(G->host, r->long_trace_node + t0, r->long_trace_offset + t0, r->long_trace_switch + t0, t1 - t0));
					list.push_back(gcdev::CorrPiece { r->longall_start[it.aln], r->longall_end[it.aln], nullptr, 0 });
				}
			}
			for (size_t k = 0, s = 0; k < list.size(); k++) if (!list[k].text) { list[k].text = spelled[s].data(); list[k].len = spelled[s].size(); s++; }
			if (!clipped) { gcdev::corrRecord(text, id, raw, rawLen, list, maxOverlap); recEnds[i].push_back(text.size()); }
			else for (size_t k = 0; k < list.size(); k++) { gcdev::corrClippedRecord(text, id, k, list[k]); recEnds[i].push_back(text.size()); }
		});
		uint64_t total = 0, records = 0;
		for (uint64_t i = 0; i < n; i++) { total += perRead[i].size(); records += recEnds[i].size(); }
		char* buf = (char*)malloc(total + 1);
		uint64_t* off = rec_off ? (uint64_t*)malloc((records + 1) * sizeof(uint64_t)) : nullptr;
		if (!buf || (rec_off && !off)) { free(buf); free(off); throw std::runtime_error("out of memory"); }
		uint64_t at = 0, k = 0;
		for (uint64_t i = 0; i < n; i++) {
			memcpy(buf + at, perRead[i].data(), perRead[i].size());
			if (off) for (uint64_t end : recEnds[i]) off[++k] = at + end;
			at += perRead[i].size();
		}
		if (off) off[0] = 0;
		buf[total] = 0;
		*out_text = buf; *out_len = total;
		if (rec_off) *rec_off = off;
		if (n_rec) *n_rec = records;
		if (n_chained_skipped) *n_chained_skipped = skipped.load();
		return (int)GC_OK;
	});
}

int gc_format_corrected_trace(const gc_graph* G, const int32_t* node, const uint32_t* offset, const uint8_t* node_switch, uint64_t n, char** out_text, uint64_t* out_len)
{
	if (!G || !out_text || !out_len || (n && (!node || !offset || !node_switch))) return fail(GC_ERR_INVALID, "null argument");
	return guarded([&]() {
		for (uint64_t i = 0; i < n; i++) {
			const size_t* size = G->host.originalNodeSize.find(node[i]);
			if (!size || offset[i] >= *size) throw std::runtime_error("gc_format_corrected_trace: no such node / offset");
		}
		const std::string piece = correctedPieceOnHost(G->host, node, offset, node_switch, n);
		*out_text = mallocCopy(piece); *out_len = piece.size();
		return (int)GC_OK;
	});
}

int gc_corrected_pieces(const gc_graph* G, const int32_t* node, const uint32_t* offset, const uint8_t* node_switch, const uint64_t* trace_off, uint64_t n_aln, char** out_text, uint64_t** out_off)
{
	if (!G || !trace_off || !out_text || !out_off) return fail(GC_ERR_INVALID, "null argument");
	const uint64_t cellsTotal = trace_off[n_aln];
	if (cellsTotal && (!node || !offset || !node_switch)) return fail(GC_ERR_INVALID, "null argument");
	if (n_aln >= 0xffffffffull) return fail(GC_ERR_INVALID, "gc_corrected_pieces: too many alignments");
	if (trace_off[0] != 0) return fail(GC_ERR_INVALID, "gc_corrected_pieces: trace_off must start at 0");
	for (uint64_t a = 0; a < n_aln; a++) if (trace_off[a + 1] < trace_off[a] || trace_off[a + 1] - trace_off[a] >= (1ull << 32)) return fail(GC_ERR_INVALID, "gc_corrected_pieces: trace_off must ascend, traces below 2^32 cells");
	// the kernels index the graph's tables with what the cells say: every cell is checked here first
	for (uint64_t i = 0; i < cellsTotal; i++) {
		const size_t* size = G->host.originalNodeSize.find(node[i]);
		if (!size || offset[i] >= *size) return fail(GC_ERR_INVALID, "gc_corrected_pieces: no such node / offset");
	}
	return guarded([&]() {
		uint64_t* off = (uint64_t*)calloc(n_aln + 1, sizeof(uint64_t));
		if (!off) throw std::runtime_error("out of memory");
		if (n_aln == 0) { *out_text = mallocCopy(std::string()); *out_off = off; return (int)GC_OK; }
		struct Free { void* p; ~Free() { free(p); } } offGuard { off };
		requireDevice();
		int device = 0;
		HIP_CHECK(hipGetDevice(&device));
		hipStream_t q = threadStream(device);
		std::vector<LongCell> cells(std::max<uint64_t>(1, cellsTotal));
		for (uint64_t i = 0; i < cellsTotal; i++) cells[i] = LongCell { node[i], offset[i], 0u, (uint32_t)(node_switch[i] != 0) };
		std::vector<OutJob> jobs(n_aln);
		for (uint64_t a = 0; a < n_aln; a++) jobs[a] = OutJob { trace_off[a], 0, (uint32_t)(trace_off[a + 1] - trace_off[a]), 0, 0, 0 };
		DeviceBuffer dCells, dJobs, dLens, dOffsets, dTotal, dText;
		LongCell* pCells = dCells.reserve<LongCell>(cells.size());
		OutJob* pJobs = dJobs.reserve<OutJob>(n_aln);
		uint32_t* pLens = dLens.reserve<uint32_t>(n_aln);
		uint64_t* pOffsets = dOffsets.reserve<uint64_t>(n_aln + 1);
		unsigned long long* pTotal = dTotal.reserve<unsigned long long>(1);
		HIP_CHECK(hipMemcpyAsync(pCells, cells.data(), cells.size() * sizeof(LongCell), hipMemcpyHostToDevice, q));
		HIP_CHECK(hipMemcpyAsync(pJobs, jobs.data(), n_aln * sizeof(OutJob), hipMemcpyHostToDevice, q));
		launchCorrectedCount(q, G->dev, pJobs, (uint32_t)n_aln, pCells, pLens, pOffsets, pTotal);
		unsigned long long total = 0;
		HIP_CHECK(hipMemcpyAsync(&total, pTotal, sizeof total, hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipStreamSynchronize(q));
		if (total > cellsTotal) throw std::runtime_error("internal: the corrected-read kernel counted more letters than cells");
		char* pText = dText.reserve<char>(total + 1);
		launchCorrectedWrite(q, G->dev, pJobs, (uint32_t)n_aln, pCells, pLens, pOffsets, pText);
		std::vector<uint32_t> lens(n_aln);
		std::string text(total, '\0');
		HIP_CHECK(hipMemcpyAsync(lens.data(), pLens, n_aln * sizeof(uint32_t), hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipMemcpyAsync(off, pOffsets, (n_aln + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, q));
		if (total) HIP_CHECK(hipMemcpyAsync(&text[0], pText, total, hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipStreamSynchronize(q));
		for (uint32_t l : lens) if (l == 0xffffffffu) throw std::runtime_error("internal: the corrected-read kernel's two passes disagree on an alignment's size");
		*out_text = mallocCopy(text);
		offGuard.p = nullptr;
		*out_off = off;
		return (int)GC_OK;
	});
}

} // extern "C"
