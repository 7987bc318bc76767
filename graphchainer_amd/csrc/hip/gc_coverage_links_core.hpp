// Link coverage (--link-coverage-out / --coverage-gfa-out / --supported-subgraph-out; this build's own, beside gc_coverage_core.hpp), the parts that compile for the host
// as well as for the device (tests/linkcov_host):
//   covTraverses    the per-cell rule: cell i > 0 of a trace is a traversal iff its node differs from cell i-1's. It walks the directed pair (node[i-1], node[i]) of bigraph
//                   ids (2 * segment + strand). An insertion repeats its predecessor's position and never traverses.
//   covLinkKey      the canonical form: the mate of (u, v) is (v ^ 1, u ^ 1), the same link read on the other strand; the canonical form is the lexicographically smaller
//                   of the two, as the key u << 32 | v (numeric order of the keys = lexicographic order of the pairs). A hairpin (u, u ^ 1) is its own mate.
//   covLinkFind     the link's number: binary search over the graph's sorted distinct canonical keys; nLinks when the pair is no link
//   covLinkChunk    one 64-cell step of a wave, lane by lane: which lanes traverse and the key each forms; lane 0's predecessor is the carry. The kernel does this with
//                   one shuffle; the host test runs this function over 64 emulated lanes.
//   covLinkLine / covGfaLinkLine / covGfaSegmentLine   the lines of the link table and of the tagged GFA, each with the function that counts its bytes
#pragma once
#include "gc_coverage_core.hpp"

namespace gcdev {

GC_COV_HD bool covTraverses(bool first, int32_t prevNode, int32_t node) { return !first && node != prevNode; }

GC_COV_HD uint64_t covLinkKey(uint32_t u, uint32_t v)
{
	const uint64_t own = (uint64_t)u << 32 | v, mate = (uint64_t)(v ^ 1u) << 32 | (u ^ 1u);
	return own < mate ? own : mate;
}
GC_COV_HD uint32_t covLinkFrom(uint64_t key) { return (uint32_t)(key >> 32); }
GC_COV_HD uint32_t covLinkTo(uint64_t key) { return (uint32_t)key; }

// keys[nLinks] ascend, all different -> the index of `key`, or nLinks
GC_COV_HD uint64_t covLinkFind(const uint64_t* keys, uint64_t nLinks, uint64_t key)
{
	uint64_t lo = 0, hi = nLinks;   // everything below lo is < key, everything from hi on is >= key
	while (lo < hi) {
		const uint64_t mid = lo + (hi - lo) / 2;
		if (keys[mid] < key) lo = mid + 1; else hi = mid;
	}
	return lo < nLinks && keys[lo] == key ? lo : nLinks;
}

// One chunk of nValid cells whose first cell has index `base`; carry = the cell before the chunk (unused when base == 0). -> mask of the traversing lanes, keyOut[lane] for those
GC_COV_HD uint64_t covLinkChunk(const CovLane* lanes, uint32_t nValid, uint32_t base, const CovLane& carry, uint64_t* keyOut)
{
	uint64_t mask = 0;
	for (uint32_t l = 0; l < nValid; l++) {
		const CovLane& p = l == 0 ? carry : lanes[l - 1];
		if (!covTraverses(base + l == 0, p.node, lanes[l].node)) continue;
		mask |= 1ull << l;
		keyOut[l] = covLinkKey((uint32_t)p.node, (uint32_t)lanes[l].node);
	}
	return mask;
}

GC_COV_HD char covOrient(uint32_t node) { return (node & 1u) ? '-' : '+'; }

// from "\t" +- "\t" to "\t" +- : what the link table's line and the GFA's L line share
GC_COV_HD uint32_t covLinkEndsLen(uint32_t fromNameLen, uint32_t toNameLen, uint32_t from, uint32_t to)
{
	return covNameLen(fromNameLen, from >> 1) + 3 + covNameLen(toNameLen, to >> 1) + 2;
}
GC_COV_HD uint32_t covLinkEnds(char* out, const char* fromName, uint32_t fromNameLen, const char* toName, uint32_t toNameLen, uint32_t from, uint32_t to)
{
	uint32_t at = covName(out, fromName, fromNameLen, from >> 1);
	out[at++] = '\t'; out[at++] = covOrient(from); out[at++] = '\t';
	at += covName(out + at, toName, toNameLen, to >> 1);
	out[at++] = '\t'; out[at++] = covOrient(to);
	return at;
}

// the link table: from "\t" +- "\t" to "\t" +- "\t" traversals "\n"
GC_COV_HD uint32_t covLinkLineLen(uint32_t fromNameLen, uint32_t toNameLen, uint32_t from, uint32_t to, uint64_t traversals)
{
	return covLinkEndsLen(fromNameLen, toNameLen, from, to) + 1 + covDecimalLen(traversals) + 1;
}
GC_COV_HD uint32_t covLinkLine(char* out, const char* fromName, uint32_t fromNameLen, const char* toName, uint32_t toNameLen, uint32_t from, uint32_t to, uint64_t traversals)
{
	uint32_t at = covLinkEnds(out, fromName, fromNameLen, toName, toNameLen, from, to);
	out[at++] = '\t'; at += covDecimal(out + at, traversals);
	out[at++] = '\n';
	return at;
}

// the tagged GFA's link: "L\t" from "\t" +- "\t" to "\t" +- "\t0M\tRC:i:" traversals "\n"
GC_COV_HD uint32_t covGfaLinkLineLen(uint32_t fromNameLen, uint32_t toNameLen, uint32_t from, uint32_t to, uint64_t traversals)
{
	return 2 + covLinkEndsLen(fromNameLen, toNameLen, from, to) + 9 + covDecimalLen(traversals) + 1;
}
GC_COV_HD uint32_t covGfaLinkLine(char* out, const char* fromName, uint32_t fromNameLen, const char* toName, uint32_t toNameLen, uint32_t from, uint32_t to, uint64_t traversals)
{
	uint32_t at = 0;
	out[at++] = 'L'; out[at++] = '\t';
	at += covLinkEnds(out + at, fromName, fromNameLen, toName, toNameLen, from, to);
	const char tags[9] = { '\t', '0', 'M', '\t', 'R', 'C', ':', 'i', ':' };
	for (uint32_t i = 0; i < 9; i++) out[at++] = tags[i];
	at += covDecimal(out + at, traversals);
	out[at++] = '\n';
	return at;
}

// the tagged GFA's segment: "S\t" name "\t" LETTERS "\tLN:i:" length "\tRC:i:" bases "\n". The letters are `length` bytes at covGfaSegmentLettersAt: the kernel leaves
// them to a thread per base (covGfaSegmentLine with letterAt == nullptr skips over them), the host test passes them in.
GC_COV_HD uint32_t covGfaSegmentLettersAt(uint32_t nameLen, uint64_t segment) { return 2 + covNameLen(nameLen, segment) + 1; }
GC_COV_HD uint64_t covGfaSegmentLineLen(uint32_t nameLen, uint64_t segment, uint64_t length, uint64_t bases)
{
	return (uint64_t)covGfaSegmentLettersAt(nameLen, segment) + length + 6 + covDecimalLen(length) + 6 + covDecimalLen(bases) + 1;
}
GC_COV_HD uint64_t covGfaSegmentLine(char* out, const char* name, uint32_t nameLen, uint64_t segment, const char* letters, uint64_t length, uint64_t bases)
{
	uint64_t at = 0;
	out[at++] = 'S'; out[at++] = '\t';
	at += covName(out + at, name, nameLen, segment);
	out[at++] = '\t';
	if (letters) for (uint64_t i = 0; i < length; i++) out[at + i] = letters[i];
	at += length;
	const char ln[6] = { '\t', 'L', 'N', ':', 'i', ':' }, rc[6] = { '\t', 'R', 'C', ':', 'i', ':' };
	for (uint32_t i = 0; i < 6; i++) out[at++] = ln[i];
	at += covDecimal(out + at, length);
	for (uint32_t i = 0; i < 6; i++) out[at++] = rc[i];
	at += covDecimal(out + at, bases);
	out[at++] = '\n';
	return at;
}

} // namespace gcdev
