// The device output encoder (struct OutputEncoder, batch/gc_output_encoder.hpp): the final alignments encoded where their traces are, the coverage count, the pieces into the
// result. Host code only: the kernels are hip/gc_output.hip, hip/gc_corrected.hip and hip/gc_coverage.hip, the index rules host/gc_output_plan.hpp.
#include "gc_output_encoder.hpp"

// Started by the whole-read pass's own thread as soon as the selection is known (the end of afterLongPass): the main thread is still in the fragment pipeline, the stitching and the
// chain distances then, so the two passes of the encoder, their two waits and the download of the text overlap that work instead of following it (r4: with the encoder after the
// join, every batch's latency grew by the encoder's launches waiting for wave slots among the other batches' kernels, and five streams in flight completed a batch every 255-268 ms
// end to end against 160 for the hot path). Every read's selected alignments are encoded; a read whose chained alignment wins in the end (known only after the join) drops its pieces
// in choose() - wasted work in proportion to the winners.
void OutputEncoder::encodeSelected()
{
	if (!P->device_output) return;
	const double t0 = nowUs();
	readJobBegin.assign(n + 1, 0);
	jobAln.clear();
	for (uint64_t r = 0; r < n; r++) {
		const ReadGlue& gl = glue[r];
		readJobBegin[r] = jobAln.size();
		if (gl.longFailed) continue;
		std::vector<gc::OutputJobItem> items;
		for (uint32_t k : gl.longSelected) items.push_back(gc::OutputJobItem { gl.longAlns[k].start, k });
		gc::outputJobOrder(items);
		for (const gc::OutputJobItem& it : items) jobAln.push_back(it.aln);
	}
	readJobBegin[n] = jobAln.size();
	nOutJobs = jobAln.size();
	if (nOutJobs == 0) return;
	if (nOutJobs >= 0xffffffffull) throw std::runtime_error("too many alignments in one batch for the output encoder");
	OutJob* hJobsOut = st->output.hOutJobs.reserve<OutJob>(nOutJobs);
	const uint32_t flags = ((P->device_output & 2) ? 1u : 0u) | ((P->device_output & 3) ? 2u : 0u) | ((P->device_output & 4) ? 4u : 0u);
	for (uint64_t r = 0; r < n; r++)
		for (uint64_t k = readJobBegin[r]; k < readJobBegin[r + 1]; k++) {
			const LongAln& al = glue[r].longAlns[jobAln[k]];
			hJobsOut[k] = OutJob { al.traceOff, R->offsets[r], al.traceLen, (uint32_t)(R->offsets[r + 1] - R->offsets[r]), flags, 0 };
		}
	hipStream_t q = st->longPass.longStream;   // (the pass and its decision are done with it)
	OutJob* dJobsOut = st->output.outJobs.reserve<OutJob>(nOutJobs);
	OutRec* dRecs = st->output.outRecs.reserve<OutRec>(nOutJobs);
	uint64_t* dOffsets = st->output.outOffsets.reserve<uint64_t>(3 * (nOutJobs + 1));
	unsigned long long* dTotals = st->output.outTotals.reserve<unsigned long long>(4);
	uint32_t* dMapSizes = (P->device_output & 4) ? st->output.outMapSizes.reserve<uint32_t>(std::max<uint64_t>(1, pass.cellsAsked()))   /* one word per cell of the pool in use */ : nullptr;
	unsigned long long* hTotals = st->output.hOutTotals.reserve<unsigned long long>(4);
	HIP_CHECK(hipMemcpyAsync(dJobsOut, hJobsOut, nOutJobs * sizeof(OutJob), hipMemcpyHostToDevice, q));
	hipEvent_t timed[6] = {};   // GC_DEBUG_TIMES: device time of the encoder's and the corrected reads' kernels, each pass between events of its own
	if (sw.debugTimes) for (auto& e : timed) HIP_CHECK(hipEventCreate(&e));
	auto mark = [&](int k) { if (timed[k]) HIP_CHECK(hipEventRecord(timed[k], q)); };
	mark(0);
	launchOutCount(q, G->dev, G->devNames, G->devIupac, dJobsOut, (uint32_t)nOutJobs, pass.deviceCells(), R->devBases, dRecs, dOffsets, dMapSizes, dTotals);
	mark(1);
	HIP_CHECK(hipMemcpyAsync(hTotals, dTotals, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, q));
	// corrected reads (device_output & 8; gc_corrected.hip): their own kernels behind the encoder's on the same stream, their count and text beside the encoder's
	const bool corrected = (P->device_output & 8) != 0;
	uint32_t* dCorrLens = nullptr; uint64_t* dCorrOffsets = nullptr; unsigned long long* hCorrTotal = nullptr;
	if (corrected) {
		dCorrLens = st->output.corrLens.reserve<uint32_t>(nOutJobs);
		dCorrOffsets = st->output.corrOffsets.reserve<uint64_t>(nOutJobs + 1);
		unsigned long long* dCorrTotal = st->output.corrTotal.reserve<unsigned long long>(1);
		hCorrTotal = st->output.hCorrTotal.reserve<unsigned long long>(1);
		launchCorrectedCount(q, G->dev, dJobsOut, (uint32_t)nOutJobs, pass.deviceCells(), dCorrLens, dCorrOffsets, dCorrTotal);
		HIP_CHECK(hipMemcpyAsync(hCorrTotal, dCorrTotal, sizeof(unsigned long long), hipMemcpyDeviceToHost, q));
	}
	mark(2);
	syncStream(q);
	const uint64_t pathBytes = hTotals[0], cigarBytes = hTotals[1], vgBytes = hTotals[2];
	char* dPath = st->output.outPathText.reserve<char>(pathBytes + 1);
	char* dCigar = st->output.outCigarText.reserve<char>(cigarBytes + 1);
	uint8_t* dVg = st->output.outVgBytes.reserve<uint8_t>(vgBytes + 1);
	mark(3);
	launchOutWrite(q, G->dev, G->devNames, G->devIupac, dJobsOut, (uint32_t)nOutJobs, pass.deviceCells(), R->devBases, dRecs, dOffsets, dMapSizes, dPath, dCigar, dVg);
	mark(4);
	OutRec* recs = st->output.hOutRecs.reserve<OutRec>(nOutJobs);
	uint64_t* offs = st->output.hOutOffsets.reserve<uint64_t>(3 * (nOutJobs + 1));
	char* pathText = st->output.hOutPathText.reserve<char>(pathBytes + 1);
	char* cigarText = st->output.hOutCigarText.reserve<char>(cigarBytes + 1);
	uint8_t* vg = st->output.hOutVgBytes.reserve<uint8_t>(vgBytes + 1);
	HIP_CHECK(hipMemcpyAsync(recs, dRecs, nOutJobs * sizeof(OutRec), hipMemcpyDeviceToHost, q));
	HIP_CHECK(hipMemcpyAsync(offs, dOffsets, 3 * (nOutJobs + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, q));
	if (pathBytes) HIP_CHECK(hipMemcpyAsync(pathText, dPath, pathBytes, hipMemcpyDeviceToHost, q));
	if (cigarBytes) HIP_CHECK(hipMemcpyAsync(cigarText, dCigar, cigarBytes, hipMemcpyDeviceToHost, q));
	if (vgBytes) HIP_CHECK(hipMemcpyAsync(vg, dVg, vgBytes, hipMemcpyDeviceToHost, q));
	uint64_t corrBytes = 0;
	uint32_t* corrLens = nullptr;
	if (corrected) {
		corrBytes = *hCorrTotal;
		char* dCorrText = st->output.corrText.reserve<char>(corrBytes + 1);
		launchCorrectedWrite(q, G->dev, dJobsOut, (uint32_t)nOutJobs, pass.deviceCells(), dCorrLens, dCorrOffsets, dCorrText);
		mark(5);
		corrLens = st->output.hCorrLens.reserve<uint32_t>(nOutJobs);
		uint64_t* corrOffs = st->output.hCorrOffsets.reserve<uint64_t>(nOutJobs + 1);
		char* corrText = st->output.hCorrText.reserve<char>(corrBytes + 1);
		HIP_CHECK(hipMemcpyAsync(corrLens, dCorrLens, nOutJobs * sizeof(uint32_t), hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipMemcpyAsync(corrOffs, dCorrOffsets, (nOutJobs + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, q));
		if (corrBytes) HIP_CHECK(hipMemcpyAsync(corrText, dCorrText, corrBytes, hipMemcpyDeviceToHost, q));
		hCorrOffsets = corrOffs; hCorrText = corrText;
	}
	syncStream(q);
	if (corrected) for (uint64_t k = 0; k < nOutJobs; k++) if (corrLens[k] == 0xffffffffu) throw std::runtime_error("internal: the corrected-read kernel's two passes disagree on an alignment's size");
	for (uint64_t k = 0; k < nOutJobs; k++) if (recs[k].steps == 0xffffffffu) throw std::runtime_error("internal: the output encoder's two passes disagree on an alignment's size");
	hOutRecs = recs; hOutOffsets = offs; hOutPath = pathText; hOutCigar = cigarText; hOutVg = vg;
	if (sw.debugTimes) fprintf(stderr, "[gc times] output encoding on the device: %llu alignments, %.1f MB of path text, %.1f MB of CIGAR, %.1f MB of vg::Path bytes, %.1f ms (on the whole-read pass's thread, beside the fragment pipeline)\n",
		(unsigned long long)nOutJobs, pathBytes / 1e6, cigarBytes / 1e6, vgBytes / 1e6, (nowUs() - t0) / 1e3);
	if (timed[0]) {
		auto between = [&](int a, int b) { float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, timed[a], timed[b])); return (double)ms; };
		const double encodeMs = between(0, 1) + between(3, 4), correctedMs = corrected ? between(1, 2) + between(4, 5) : 0.0;
		for (hipEvent_t e : timed) HIP_CHECK(hipEventDestroy(e));
		fprintf(stderr, "[gc times] output kernels on the device: k_out_encode (both passes, k_out_place) %.3f ms; corrected reads (k_corr_walk both passes, k_corr_place) %.3f ms, %.1f MB of letters down\n",
			encodeMs, correctedMs, corrBytes / 1e6);
	}
}

// After the decision: which of the encoded alignments are the batch's output, in the reference's order
void OutputEncoder::choose(hipStream_t fragmentStream)
{
	if (!P->device_output) return;
	gc::outputEntries(n, [&](uint64_t r) { return glue[r].longFailed; }, [&](uint64_t r) { return glue[r].chainWins; }, readJobBegin.data(), jobAln.data(), readOutOff, outEntries, outJobOfEntry);
	if (st->coverage) countCoverage(fragmentStream);
}

// gc_stream_set_coverage: the batch's output entries - exactly the alignments the writers will print - are counted into the handle (gc_coverage.hip). Here and not beside the
// encoder: the encoder runs before the chained-versus-whole-read decision and drops the losers' pieces afterwards, and a count cannot be dropped. Entries of source 0 are
// read where they lie, in the cell pool (still resident: nothing reserves it again before the next batch), under a keep byte per encoder job; the chained winners' traces
// exist only on the host (chain_trace_*: edlib's path walked, or the fast mode's stitched cells) and go up for the same kernel, each job with its read's place in the
// batch's resident bases (the pileup reads the letter under seqPos). The stream is waited for: a finished batch
// is a counted batch.
void OutputEncoder::countCoverage(hipStream_t stream)
{
	gc_coverage* cov = st->coverage;
	const double t0 = nowUs();
	hipEvent_t timed[2] = {};
	if (sw.debugTimes) for (auto& e : timed) HIP_CHECK(hipEventCreate(&e));
	if (timed[0]) HIP_CHECK(hipEventRecord(timed[0], stream));
	uint64_t nKept = 0, nWinners = 0, winnerCells = 0;
	if (nOutJobs) {
		uint8_t* hKeep = st->output.hCovKeep.reserve<uint8_t>(nOutJobs);
		memset(hKeep, 0, nOutJobs);
		for (uint64_t k : outJobOfEntry) if (k != ~0ull) { hKeep[k] = 1; nKept++; }
		if (nKept) {
			uint8_t* dKeep = st->output.covKeep.reserve<uint8_t>(nOutJobs);
			HIP_CHECK(hipMemcpyAsync(dKeep, hKeep, nOutJobs, hipMemcpyHostToDevice, stream));
			launchCoverageAdd(stream, cov->dev, cov->links, (const OutJob*)st->output.outJobs.ptr, (uint32_t)nOutJobs, dKeep, pass.deviceCells(), cov->dBases, cov->dDepth, cov->dBad, cov->pileFor(R->devBases));
		}
	}
	for (const OutEntry& en : outEntries) if (en.source == 1) { nWinners++; winnerCells += glue[en.read].chainTraceNode.size(); }
	if (nWinners) {
		if (nWinners >= 0xffffffffull) throw std::runtime_error("too many chained alignments in one batch for the coverage kernel");
		LongCell* hCells = st->output.hCovCells.reserve<LongCell>(winnerCells);
		OutJob* hJobsCov = st->output.hCovJobs.reserve<OutJob>(nWinners);
		uint64_t at = 0, w = 0;
		for (const OutEntry& en : outEntries) {
			if (en.source != 1) continue;
			const ReadGlue& gl = glue[en.read];
			const size_t cells = gl.chainTraceNode.size();
			if (cells == 0) throw std::runtime_error("coverage: a chained alignment won and the batch holds no trace for it (chain_traces == 0?)");
			hJobsCov[w++] = OutJob { at, R->offsets[en.read], (uint32_t)cells, (uint32_t)(R->offsets[en.read + 1] - R->offsets[en.read]), 0, 0 };   // (the read, in the batch's resident bases: the pileup looks under seqPos)
			for (size_t i = 0; i < cells; i++) hCells[at++] = LongCell { gl.chainTraceNode[i], gl.chainTraceOffset[i], gl.chainTraceSeqPos[i], gl.chainTraceSwitch[i] };
		}
		LongCell* dCells = st->output.covCells.reserve<LongCell>(winnerCells);
		OutJob* dJobsCov = st->output.covJobs.reserve<OutJob>(nWinners);
		HIP_CHECK(hipMemcpyAsync(dCells, hCells, winnerCells * sizeof(LongCell), hipMemcpyHostToDevice, stream));
		HIP_CHECK(hipMemcpyAsync(dJobsCov, hJobsCov, nWinners * sizeof(OutJob), hipMemcpyHostToDevice, stream));
		launchCoverageAdd(stream, cov->dev, cov->links, dJobsCov, (uint32_t)nWinners, nullptr, dCells, cov->dBases, cov->dDepth, cov->dBad, cov->pileFor(R->devBases));
	}
	if (timed[1]) HIP_CHECK(hipEventRecord(timed[1], stream));
	HIP_CHECK(hipGetLastError());
	syncStream(stream);
	if (timed[0]) {
		float ms = 0;
		HIP_CHECK(hipEventElapsedTime(&ms, timed[0], timed[1]));
		for (hipEvent_t e : timed) HIP_CHECK(hipEventDestroy(e));
		fprintf(stderr, "[gc times] coverage: k_cov_add over %llu alignments in the cell pool and %llu chained winners (%llu cells up), %.3f ms on the device, %.1f ms in all; per-base depth %s, links %s, pileup %s\n",
			(unsigned long long)nKept, (unsigned long long)nWinners, (unsigned long long)winnerCells, ms, (nowUs() - t0) / 1e3, cov->dDepth ? "on" : "off", cov->hasLinks ? "on" : "off", cov->dPile ? "on" : "off");
	}
}

// where every entry's piece of one stream goes (entryOff: the result's offsets, nOut + 1 of them, filled here), and the result's blob for them
OutputEncoder::PieceStream OutputEncoder::placePieces(const void* src, const uint64_t* jobOff, uint64_t* entryOff) const
{
	const uint64_t bytes = gc::outputPieceOffsets(outJobOfEntry.data(), outEntries.size(), jobOff, entryOff);
	return PieceStream { (const char*)src, jobOff, resultArray<char>(bytes + 1), entryOff, bytes };
}

// the kept jobs' bytes of `count` streams back to back into the result: the device's blobs whole, in 16 parts each, when job k is entry k; entry by entry otherwise
void OutputEncoder::copyPieces(const PieceStream* streams, size_t count, bool allKept)
{
	const size_t parts = 16;
	if (allKept) pool.run(count * parts, [&](size_t i, size_t) {
		const PieceStream& s = streams[i / parts];
		const size_t part = i % parts;
		const uint64_t b = s.bytes * part / parts, e = s.bytes * (part + 1) / parts;
		if (e > b) memcpy(s.dst + b, s.src + b, e - b);
	});
	else pool.run(outEntries.size(), [&](size_t e, size_t) {
		const uint64_t k = outJobOfEntry[e];
		if (k == ~0ull) return;
		for (size_t i = 0; i < count; i++) { const PieceStream& s = streams[i]; memcpy(s.dst + s.entryOff[e], s.src + s.jobOff[k], s.jobOff[k + 1] - s.jobOff[k]); }
	});
}

void OutputEncoder::assembleInto(gc_result* res)   // the pieces into the result (entries of chained winners stay empty: source 1)
{
	res->device_output = P->device_output;
	if (!P->device_output) return;
	const uint64_t nOut = outEntries.size();
	res->read_out_off = resultArray<uint64_t>(n + 1);
	memcpy(res->read_out_off, readOutOff.data(), (n + 1) * sizeof(uint64_t));
	res->out_source = resultArray<uint8_t>(nOut);
	res->out_numbers = resultArray<uint64_t>(12 * nOut);
	res->out_path_off = resultArray<uint64_t>(nOut + 1); res->out_cigar_off = resultArray<uint64_t>(nOut + 1); res->out_vg_off = resultArray<uint64_t>(nOut + 1);
	auto jobOffsets = [&](uint64_t which) { return hOutOffsets ? hOutOffsets + which * (nOutJobs + 1) : nullptr; };   // (null: a batch without jobs)
	// where every entry's pieces go: the kept jobs' bytes back to back (all of them, in order, unless chained alignments won)
	const PieceStream text[3] = { placePieces(hOutPath, jobOffsets(0), res->out_path_off), placePieces(hOutCigar, jobOffsets(1), res->out_cigar_off), placePieces(hOutVg, jobOffsets(2), res->out_vg_off) };
	res->out_path_text = text[0].dst; res->out_cigar_text = text[1].dst; res->out_vg_path = (uint8_t*)text[2].dst;
	const bool allKept = gc::outputAllKept(outJobOfEntry.data(), nOut, nOutJobs);
	copyPieces(text, 3, allKept);
	res->out_path_text[text[0].bytes] = 0; res->out_cigar_text[text[1].bytes] = 0;
	if (P->device_output & 8) {   // the corrected pieces, compacted like the other three (entries of chained winners stay empty: the host spells them from chain_trace_*)
		res->out_corrected_off = resultArray<uint64_t>(nOut + 1);
		const PieceStream corrected = placePieces(hCorrText, hCorrOffsets, res->out_corrected_off);
		res->out_corrected_text = corrected.dst;
		copyPieces(&corrected, 1, allKept);
		res->out_corrected_text[corrected.bytes] = 0;
	}
	for (uint64_t e = 0; e < nOut; e++) {
		const OutEntry& en = outEntries[e];
		res->out_source[e] = en.source;
		uint64_t* num = res->out_numbers + 12 * e;
		if (en.source == 0) {
			const OutRec& rec = hOutRecs[outJobOfEntry[e]];
			const LongAln& al = glue[en.read].longAlns[en.aln];
			num[0] = rec.nodePathLen; num[1] = rec.nodePathStart; num[2] = rec.nodePathEnd; num[3] = rec.matches; num[4] = rec.mismatches; num[5] = rec.insertions; num[6] = rec.deletions;
			num[7] = al.traceLen; num[8] = al.start; num[9] = al.end; num[10] = rec.steps; num[11] = al.score;
		} else for (int i = 0; i < 12; i++) num[i] = 0;
	}
}
