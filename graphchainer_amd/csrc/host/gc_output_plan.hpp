// The device output encoder's host rules (batch/gc_output_encoder.hip is their one user): the order a read's selected alignments get as encoder jobs, which of the encoded
// jobs are the batch's output entries once the chained-versus-whole-read decision is known, and where the kept jobs' pieces go in the result. Index arithmetic only - every
// rule is the expression the encoder used to hold inline between its HIP calls, with the same integer types.
// Standard library only: tests/output_plan_host builds it without HIP.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gc {

// ---- the job order of one read
// its selected alignments (aln: index into the read's alignments) by alignmentStart, as the reference leaves them: sorted twice with an unstable sort
// (src/Aligner.cpp:1003 and :1023 - the second may move ties even in a sorted list), so two calls of std::sort with the one comparator and ties in libstdc++'s order
struct OutputJobItem { uint32_t start; uint32_t aln; };
inline void outputJobOrder(std::vector<OutputJobItem>& items)
{
	auto byStart = [](const OutputJobItem& l, const OutputJobItem& rr) { return l.start < rr.start; };
	std::sort(items.begin(), items.end(), byStart);   // src/Aligner.cpp:1003
	std::sort(items.begin(), items.end(), byStart);   // :1023 (an unstable sort may move ties even in a sorted list)
}

// ---- the entries after the decision
// aln: index into the read's alignments (source 0); source 1: the read's chained alignment, which no encoder job holds (its job in jobOfEntry: OUTPUT_NO_JOB)
struct OutputEntry { uint32_t read, aln; uint8_t source; };
inline constexpr uint64_t OUTPUT_NO_JOB = ~0ull;
// In the reference's order: a failed read has no entry, a read whose chained alignment wins has that one entry and drops its jobs, every other read keeps its jobs
// [readJobBegin[r], readJobBegin[r + 1]) in order. longFailed(r), chainWins(r): the two flags of read r; readOutOff gets n + 1 elements.
template <typename Failed, typename Wins>
inline void outputEntries(uint64_t n, Failed&& longFailed, Wins&& chainWins, const uint64_t* readJobBegin, const uint32_t* jobAln,
	std::vector<uint64_t>& readOutOff, std::vector<OutputEntry>& entries, std::vector<uint64_t>& jobOfEntry)
{
	readOutOff.assign(n + 1, 0);
	entries.clear();
	jobOfEntry.clear();
	for (uint64_t r = 0; r < n; r++) {
		readOutOff[r] = entries.size();
		if (longFailed(r)) continue;
		if (chainWins(r)) { entries.push_back(OutputEntry { (uint32_t)r, 0, 1 }); jobOfEntry.push_back(OUTPUT_NO_JOB); continue; }
		for (uint64_t k = readJobBegin[r]; k < readJobBegin[r + 1]; k++) { entries.push_back(OutputEntry { (uint32_t)r, jobAln[k], 0 }); jobOfEntry.push_back(k); }
	}
	readOutOff[n] = entries.size();
}

// ---- compaction of one piece stream
// where every entry's piece goes: the kept jobs' bytes back to back (jobOff: the stream's job offsets, nJobs + 1 of them; entryOff gets nOut + 1). An entry without a
// job gets begin = end. Returns the total.
inline uint64_t outputPieceOffsets(const uint64_t* jobOfEntry, uint64_t nOut, const uint64_t* jobOff, uint64_t* entryOff)
{
	uint64_t bytes = 0;
	for (uint64_t e = 0; e < nOut; e++) {
		entryOff[e] = bytes;
		const uint64_t k = jobOfEntry[e];
		if (k != OUTPUT_NO_JOB) bytes += jobOff[k + 1] - jobOff[k];
	}
	entryOff[nOut] = bytes;
	return bytes;
}

// no chained winner: the device's blobs are the result's, job k is entry k
// (a winner's one entry can stand where a read's one dropped job was: the counts alone do not tell)
inline bool outputAllKept(const uint64_t* jobOfEntry, uint64_t nOut, uint64_t nJobs)
{
	bool allKept = nOut == nJobs;
	for (uint64_t e = 0; e < nOut && allKept; e++) allKept = jobOfEntry[e] == e;
	return allKept;
}

} // namespace gc
