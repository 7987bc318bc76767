// The device output encoder of a batch (gc_params::device_output; hip/gc_output.hip, hip/gc_corrected.hip, hip/gc_coverage.hip): the GAF path / CIGAR text, the vg::Path
// bytes and the corrected pieces of every alignment the reference would write for the batch (src/Aligner.cpp:901-920,1003-1023), made where the traces are so that no trace
// cell has to come down for the writers; the coverage count of exactly those alignments; the pieces compacted into the result. Defined in batch/gc_output_encoder.hip, a
// translation unit that cannot name a BatchRun member: what the batch (BatchRun, gc_batch.hip) and the encoder share is this interface. The index rules - job order,
// entries after the decision, compaction - are host/gc_output_plan.hpp.
//
// Which thread calls what, and what each call may touch:
// - encodeSelected(): the whole-read pass's thread, from the pass's selectionKnown hook (batch/gc_long_pass.hpp). It reads the ReadGlue fields the pass has just written
//   (longFailed, longSelected, longAlns) and, of the pass, only cellsAsked() and deviceCells(); it writes this object's members and st->output, and works on
//   st->longPass.longStream. Between the hook and WholeReadPass::join() the main thread touches neither this object nor st->output.
// - choose(), assembleInto(): the main thread, after WholeReadPass::join() has returned and - choose() - after the chained alignments' decision (ReadGlue::chainWins and the
//   winners' chainTrace*). They read what encodeSelected() left; choose() writes the entries and, with a coverage handle on the stream, counts them on the fragment
//   pipeline's stream and waits for it; assembleInto() writes the result's out_* arrays.
//
// Lifetime: the batch declares its encoder before its WholeReadPass, so the pass - whose destructor joins a thread that is still running - goes first and the hook's target
// outlives the thread.
#pragma once
#include "gc_long_pass.hpp"

struct OutputEncoder {
	// st: output, longPass.longStream, coverage, glue (the fields named above)
	OutputEncoder(const gc::Switches& sw, const gc_graph* G, const gc_reads* R, const gc_params* P, gc_stream* st, WorkerPool& pool, const WholeReadPass& pass)
		: sw(sw), G(G), R(R), P(P), st(st), pool(pool), pass(pass), n(R->offsets.size() - 1), glue(st->glue) {}
	OutputEncoder(const OutputEncoder&) = delete;
	OutputEncoder& operator=(const OutputEncoder&) = delete;

	// pass thread. Every read's selected alignments are encoded as soon as the selection is known (see the .hip for why here and not after the join)
	void encodeSelected();
	// main thread. After the decision: which of the encoded alignments are the batch's output, in the reference's order; counted into st->coverage when there is one
	// (fragmentStream: the stream the count runs on and is waited for)
	void choose(hipStream_t fragmentStream);
	// main thread. The pieces into the result (entries of chained winners stay empty: source 1)
	void assembleInto(gc_result* res);

private:
	using OutEntry = gc::OutputEntry;
	// one stream of pieces on its way into the result: the device's blob and its job offsets, the result's blob and its entry offsets
	struct PieceStream { const char* src; const uint64_t* jobOff; char* dst; const uint64_t* entryOff; uint64_t bytes; };
	void countCoverage(hipStream_t stream);
	PieceStream placePieces(const void* src, const uint64_t* jobOff, uint64_t* entryOff) const;
	void copyPieces(const PieceStream* streams, size_t count, bool allKept);

	// ---- the call
	const gc::Switches& sw;
	const gc_graph* const G; const gc_reads* const R; const gc_params* const P;
	gc_stream* const st;
	WorkerPool& pool;
	const WholeReadPass& pass;
	const uint64_t n;                        // reads in the batch
	std::vector<ReadGlue>& glue;             // per-read host records (the fields named in the header comment)
	// ---- encodeSelected()
	std::vector<uint64_t> readJobBegin;   // first job of every read (jobs of a read: its selected alignments sorted by alignmentStart); [n] = number of jobs
	std::vector<uint32_t> jobAln;         // the alignment (index into the read's longAlns) of every job
	uint64_t nOutJobs = 0;
	const OutRec* hOutRecs = nullptr; const uint64_t* hOutOffsets = nullptr;
	const char* hOutPath = nullptr; const char* hOutCigar = nullptr; const uint8_t* hOutVg = nullptr;
	const uint64_t* hCorrOffsets = nullptr; const char* hCorrText = nullptr;   // (device_output & 8) the corrected pieces of the jobs: [nOutJobs + 1], letters
	// ---- choose()
	std::vector<OutEntry> outEntries;
	std::vector<uint64_t> readOutOff;
	std::vector<uint64_t> outJobOfEntry;
};
