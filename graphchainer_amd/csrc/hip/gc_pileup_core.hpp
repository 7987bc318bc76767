// The pileup of the counted alignments (--pileup-out; GC_COVERAGE_PILEUP; this build's own like the coverage it rides on), the parts that compile for the host as well as
// for the device (tests/pileup_host). include/graphchainer_amd.h has the definition; here it is as code:
//   pileKind        a trace cell by `covers` (covCovers, gc_coverage_core.hpp) and `moved` (cell 0, or seqPos differs from the cell before): covers and moved an aligned
//                   pair (match or mismatch), covers alone a deletion, moved alone an insertion, neither nothing
//   pileChannel     the channel a read letter counts into when it is a mismatch: A C G T/U (either case) their own, every other byte mmN; on an odd bigraph id the letter is
//                   complemented first (the row is the forward strand's)
//   pileCellChannel the channel of one cell, or PILE_NONE for a match and for nothing
//   pilePasses / pileLineLen / pileLine   the filter and the line of the table (gc_coverage_format_pileup)
// A row is eight 32-bit words per forward base, PILE_* below; every word saturates at 2^32 - 1 like the depth word (covSatAdd).
#pragma once
#include "gc_coverage_core.hpp"

namespace gcdev {

enum : uint32_t { PILE_MM_A = 0, PILE_MM_C = 1, PILE_MM_G = 2, PILE_MM_T = 3, PILE_MM_N = 4, PILE_DEL = 5, PILE_INS_AFTER = 6, PILE_INS_BEFORE = 7, PILE_CHANNELS = 8, PILE_NONE = 0xffffffffu };
enum : uint32_t { PILE_KIND_NOTHING = 0, PILE_KIND_PAIR = 1, PILE_KIND_DELETION = 2, PILE_KIND_INSERTION = 3 };

GC_COV_HD bool pileMoved(bool first, uint32_t prevSeqPos, uint32_t seqPos) { return first || seqPos != prevSeqPos; }

GC_COV_HD uint32_t pileKind(bool covers, bool moved)
{
	return covers ? (moved ? PILE_KIND_PAIR : PILE_KIND_DELETION) : (moved ? PILE_KIND_INSERTION : PILE_KIND_NOTHING);
}

// the mismatch channel of every byte a read may hold, forward strand
struct PileLetterTable {
	uint8_t channel[256];
	constexpr PileLetterTable() : channel()
	{
		for (int i = 0; i < 256; i++) channel[i] = (uint8_t)PILE_MM_N;
		channel['A'] = channel['a'] = (uint8_t)PILE_MM_A;
		channel['C'] = channel['c'] = (uint8_t)PILE_MM_C;
		channel['G'] = channel['g'] = (uint8_t)PILE_MM_G;
		channel['T'] = channel['t'] = channel['U'] = channel['u'] = (uint8_t)PILE_MM_T;
	}
};

// A <-> T, C <-> G; mmN is its own complement
GC_COV_HD uint32_t pileComplement(uint32_t channel) { return channel < PILE_MM_N ? 3u - channel : channel; }

GC_COV_HD uint32_t pileChannel(uint8_t readLetter, bool oddNode)
{
	static constexpr PileLetterTable table {};
	const uint32_t channel = table.channel[readLetter];
	return oddNode ? pileComplement(channel) : channel;
}

// readSet / graphSet: the sets of plain bases (A 1, C 2, G 4, T 8) the two letters stand for, as the GAF encoder compares them: a match iff they intersect
GC_COV_HD uint32_t pileCellChannel(uint32_t kind, bool oddNode, uint8_t readLetter, uint32_t readSet, uint32_t graphSet)
{
	if (kind == PILE_KIND_PAIR) return (readSet & graphSet) ? (uint32_t)PILE_NONE : pileChannel(readLetter, oddNode);
	if (kind == PILE_KIND_DELETION) return PILE_DEL;
	if (kind == PILE_KIND_INSERTION) return oddNode ? PILE_INS_BEFORE : PILE_INS_AFTER;
	return PILE_NONE;
}

GC_COV_HD uint32_t pileAlt(const uint32_t* row)
{
	uint32_t alt = 0;
	for (uint32_t c = 0; c < PILE_CHANNELS; c++) if (row[c] > alt) alt = row[c];
	return alt;
}

// a base has a line iff it is covered and its largest channel reaches both thresholds
GC_COV_HD bool pilePasses(uint32_t depth, const uint32_t* row, uint64_t minAlt, double minFraction)
{
	const uint32_t alt = pileAlt(row);
	return depth > 0 && (uint64_t)alt >= minAlt && (double)alt >= minFraction * (double)depth;
}

// depth = matches + mismatches + deletions (a word that stopped at 2^32 - 1 no longer says how many: the difference stops at 0)
GC_COV_HD uint32_t pileMatches(uint32_t depth, const uint32_t* row)
{
	uint64_t others = 0;
	for (uint32_t c = 0; c <= PILE_DEL; c++) others += row[c];
	return others < depth ? (uint32_t)(depth - others) : 0u;
}

// segment \t pos \t ref \t depth \t match \t mmA \t mmC \t mmG \t mmT \t mmN \t del \t ins_before \t ins_after \n
GC_COV_HD uint32_t pileLineLen(uint32_t nameLen, uint64_t segment, uint64_t pos, uint32_t depth, const uint32_t* row)
{
	uint32_t n = covNameLen(nameLen, segment) + 1 + covDecimalLen(pos) + 1 + 1 + 1 + covDecimalLen(depth) + 1 + covDecimalLen(pileMatches(depth, row));
	for (uint32_t c = 0; c < PILE_CHANNELS; c++) n += 1 + covDecimalLen(row[c]);
	return n + 1;
}
GC_COV_HD uint32_t pileLine(char* out, const char* name, uint32_t nameLen, uint64_t segment, uint64_t pos, char ref, uint32_t depth, const uint32_t* row)
{
	uint32_t at = covName(out, name, nameLen, segment);
	out[at++] = '\t'; at += covDecimal(out + at, pos);
	out[at++] = '\t'; out[at++] = ref;
	out[at++] = '\t'; at += covDecimal(out + at, depth);
	out[at++] = '\t'; at += covDecimal(out + at, pileMatches(depth, row));
	for (uint32_t c = 0; c <= PILE_DEL; c++) { out[at++] = '\t'; at += covDecimal(out + at, row[c]); }
	out[at++] = '\t'; at += covDecimal(out + at, row[PILE_INS_BEFORE]);
	out[at++] = '\t'; at += covDecimal(out + at, row[PILE_INS_AFTER]);
	out[at++] = '\n';
	return at;
}

// One chunk of a wave on the host, lane by lane, as the kernel takes it: channel[l] of every valid lane (PILE_NONE where the cell counts nothing)
struct PileLane { int32_t node; uint32_t offset, seqPos; };
template <typename ReadSet, typename GraphSet>
inline void pileChunk(const PileLane* lanes, uint32_t nValid, uint32_t base, const PileLane& carry, const uint8_t* read, uint32_t readLen, ReadSet&& readSet, GraphSet&& graphSet, uint32_t* channel, bool* bad)
{
	for (uint32_t l = 0; l < nValid; l++) {
		const PileLane& p = l == 0 ? carry : lanes[l - 1];
		const bool first = base + l == 0;
		const uint32_t kind = pileKind(covCovers(first, p.node, p.offset, lanes[l].node, lanes[l].offset), pileMoved(first, p.seqPos, lanes[l].seqPos));
		if (lanes[l].seqPos >= readLen) { channel[l] = PILE_NONE; *bad = true; continue; }
		const uint8_t letter = read[lanes[l].seqPos];
		channel[l] = pileCellChannel(kind, (lanes[l].node & 1) != 0, letter, readSet(letter), graphSet(lanes[l].node, lanes[l].offset));
	}
}

} // namespace gcdev
