// The MUM / MEM seeder (gc_seeds_mxm; the reference's MummerSeeder, src/MummerSeeder.cpp), the parts that compile for the host as well as for the device (tests/mxm_host):
//   mxmTextWord / mxmQueryWord   32 letters of the index text / of one strand of a read as one 2-bit word, with the number of leading letters that are a, c, g or t
//   mxmInterval                  the suffix-array interval of the suffixes that start with q[i .. i + minLen): prefix table, then binary search on the packed words
//   mxmOccurrence                one occurrence of that interval -> left-maximality, extension to the right word by word, uniqueness for MUM, (segment, offset) and the SeedHit
// The text is every original segment in forward orientation in ascending node id, each followed by a separator; a letter that is not a, c, g, t (u) is a separator too, and a read
// letter that is none of them equals nothing (lowercaseRef / lowercaseSeq, src/MummerSeeder.cpp). The suffix array orders suffixes with separator < a < c < g < t.
#pragma once
#include "gc_seedhits_core.hpp"
#include <cstdint>

#if defined(__HIPCC__)
#define GC_MXM_HD __host__ __device__ __forceinline__
#else
#define GC_MXM_HD inline
#endif

namespace gcdev {

enum MxmMode : int32_t { MXM_MUM = 1, MXM_MEM = 2 };

struct MxmIndexView {
	const uint32_t* sa;          // [n] every text position, separators included
	const uint64_t* packed;      // [(n >> 5) + 2] 2 bits per letter, first letter in the top bits (as gc_reads' packed bases)
	const uint64_t* invalid;     // [(n >> 6) + 2] bit set: separator, or beyond the text (first letter in the top bit)
	const uint32_t* nodeStart;   // [nNodes + 1] text position of every segment's first letter; nodeStart[nNodes] = n
	const int32_t* nodeId;       // [nNodes] SeedHit::nodeID of the segment
	const uint32_t* prefix;      // [2 << (2 * prefixLen)] SA interval [lo, hi) of every prefixLen-mer (0, 0: none), or nullptr
	uint32_t n, nNodes, prefixLen;
};

struct MxmQuery {   // one strand of one read; the reverse strand is the forward bases complemented on the fly
	const char* fw;
	uint32_t len, reverse;
};

GC_MXM_HD uint32_t mxmClz64(uint64_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return (uint32_t)__clzll((long long)x);
#else
	return x ? (uint32_t)__builtin_clzll(x) : 64u;
#endif
}

GC_MXM_HD uint32_t mxmLetterCode(char c)   // 0..3 = a c g t, 4 = anything else
{
	switch (c) {
		case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': case 'U': case 'u': return 3;
	}
	return 4;
}

GC_MXM_HD uint32_t mxmQueryCode(const MxmQuery& q, uint32_t j)   // j < q.len, in the searched orientation
{
	if (!q.reverse) return mxmLetterCode(q.fw[j]);
	const uint32_t c = mxmLetterCode(q.fw[q.len - 1 - j]);
	return c < 4 ? 3 - c : 4;
}

// letters j .. j + 31 of the strand; valid = how many leading ones are a, c, g, t (0 at and beyond the end)
GC_MXM_HD uint64_t mxmQueryWord(const MxmQuery& q, uint32_t j, uint32_t& valid)
{
	uint64_t w = 0;
	uint32_t k = 0;
	for (; k < 32 && j + k < q.len; k++) {
		const uint32_t c = mxmQueryCode(q, j + k);
		if (c > 3) break;
		w |= (uint64_t)c << (62 - 2 * k);
	}
	valid = k;
	return w;
}

// letters p .. p + 31 of the text (p <= n); valid as above. Bits behind the valid letters are unspecified.
GC_MXM_HD uint64_t mxmTextWord(const MxmIndexView& ix, uint32_t p, uint32_t& valid)
{
	const uint32_t w = p >> 5, s = (p & 31) * 2, v = p >> 6, t = p & 63;
	const uint64_t word = s ? (ix.packed[w] << s) | (ix.packed[w + 1] >> (64 - s)) : ix.packed[w];
	const uint64_t inv = t ? (ix.invalid[v] << t) | (ix.invalid[v + 1] >> (64 - t)) : ix.invalid[v];
	const uint32_t z = mxmClz64(inv);
	valid = z < 32 ? z : 32;
	return word;
}

GC_MXM_HD uint32_t mxmTextCode(const MxmIndexView& ix, uint32_t p)   // p < n
{
	if ((ix.invalid[p >> 6] >> (63 - (p & 63))) & 1) return 4;
	return (uint32_t)(ix.packed[p >> 5] >> (62 - 2 * (p & 31))) & 3;
}

GC_MXM_HD uint32_t mxmCommonOfWords(uint64_t a, uint32_t validA, uint64_t b, uint32_t validB)
{
	const uint64_t x = a ^ b;
	uint32_t m = mxmClz64(x) >> 1;
	if (m > validA) m = validA;
	if (m > validB) m = validB;
	return m;
}

// length of the longest common prefix of T[p ..] and q[j ..] over a, c, g, t, 32 letters per step; stops at `cap` or soon after (the result may exceed cap by up to 31)
GC_MXM_HD uint32_t mxmCommon(const MxmIndexView& ix, const MxmQuery& q, uint32_t p, uint32_t j, uint32_t cap)
{
	uint32_t l = 0;
	while (l < cap) {
		uint32_t vt, vq;
		const uint64_t tw = mxmTextWord(ix, p + l, vt);
		const uint64_t qw = mxmQueryWord(q, j + l, vq);
		const uint32_t m = mxmCommonOfWords(tw, vt, qw, vq);
		l += m;
		if (m < 32) break;
	}
	return l;
}

// the suffix at p against the pattern q[i .. i + m) (all of it a, c, g, t): -1 the suffix sorts before every suffix that starts with the pattern, 0 it starts with it, 1 after.
// qw0 / vq0: the pattern's first word, which every step of a binary search would cut again.
GC_MXM_HD int mxmCompare(const MxmIndexView& ix, const MxmQuery& q, uint32_t p, uint32_t i, uint32_t m, uint64_t qw0, uint32_t vq0)
{
	uint32_t vt;
	const uint64_t tw = mxmTextWord(ix, p, vt);
	uint32_t c = mxmCommonOfWords(tw, vt, qw0, vq0);
	if (c == 32 && m > 32) c += mxmCommon(ix, q, p + 32, i + 32, m - 32);
	if (c >= m) return 0;
	if (p + c >= ix.n) return -1;
	const uint32_t tc = mxmTextCode(ix, p + c);
	if (tc > 3) return -1;   // a separator sorts before every letter
	return tc < mxmQueryCode(q, i + c) ? -1 : 1;
}

// true: q[i .. i + minLen) lies inside the strand and is all a, c, g, t, and [lo, hi) are the suffixes that start with it (maybe none)
GC_MXM_HD bool mxmInterval(const MxmIndexView& ix, const MxmQuery& q, uint32_t i, uint32_t minLen, uint32_t& lo, uint32_t& hi)
{
	lo = hi = 0;
	if (q.len < minLen || i > q.len - minLen) return false;
	uint32_t vq0;
	const uint64_t qw0 = mxmQueryWord(q, i, vq0);
	if (vq0 < 32 && vq0 < minLen) return false;   // a window with a letter outside the alphabet is rejected before any lookup
	for (uint32_t l = 32; l < minLen; l += 32) {
		uint32_t v;
		(void)mxmQueryWord(q, i + l, v);
		if (v < 32 && l + v < minLen) return false;
	}
	uint32_t a = 0, b = ix.n;
	if (ix.prefix && minLen >= ix.prefixLen) {
		const uint64_t code = qw0 >> (64 - 2 * ix.prefixLen);
		a = ix.prefix[2 * code]; b = ix.prefix[2 * code + 1];
		if (minLen == ix.prefixLen || a >= b) { lo = a; hi = b; return true; }
	}
	uint32_t x = a, y = b;   // first suffix that does not sort before the pattern
	while (x < y) { const uint32_t mid = x + ((y - x) >> 1); if (mxmCompare(ix, q, ix.sa[mid], i, minLen, qw0, vq0) < 0) x = mid + 1; else y = mid; }
	lo = hi = x;
	if (x >= b || mxmCompare(ix, q, ix.sa[x], i, minLen, qw0, vq0) != 0) return true;   // most windows are not in the text at all: one comparison instead of a second search
	x++; y = b;              // first suffix that sorts after it
	while (x < y) { const uint32_t mid = x + ((y - x) >> 1); if (mxmCompare(ix, q, ix.sa[mid], i, minLen, qw0, vq0) <= 0) x = mid + 1; else y = mid; }
	hi = x;
	return true;
}

GC_MXM_HD uint32_t mxmSegmentOf(const MxmIndexView& ix, uint32_t p)   // the last segment that starts at or before p
{
	uint32_t lo = 0, hi = ix.nNodes;
	while (lo + 1 < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (ix.nodeStart[mid] <= p) lo = mid; else hi = mid; }
	return lo;
}

// Occurrence k of the interval [lo, hi) of q[i .. i + minLen). A MEM: left-maximal, extended to the right as far as text and strand agree. A MUM (mummer's MAM): a MEM whose
// matched string occurs once in the text - the suffixes beside k do not share it (the occurrences of a string are neighbours in the suffix array).
// tpos: the text position, for the defined order of equal lengths.
GC_MXM_HD bool mxmOccurrence(const MxmIndexView& ix, const MxmQuery& q, int32_t mode, uint32_t minLen, uint32_t i, uint32_t lo, uint32_t hi, uint32_t k, SeedHit& hit, uint32_t& tpos)
{
	const uint32_t p = ix.sa[k];
	if (i > 0 && p > 0) {
		const uint32_t tc = mxmTextCode(ix, p - 1);
		if (tc < 4 && tc == mxmQueryCode(q, i - 1)) return false;
	}
	const uint32_t len = minLen + mxmCommon(ix, q, p + minLen, i + minLen, 0xffffffffu);
	if (mode == MXM_MUM) {
		if (k > lo && minLen + mxmCommon(ix, q, ix.sa[k - 1] + minLen, i + minLen, len - minLen) >= len) return false;
		if (k + 1 < hi && minLen + mxmCommon(ix, q, ix.sa[k + 1] + minLen, i + minLen, len - minLen) >= len) return false;
	}
	const uint32_t seg = mxmSegmentOf(ix, p);
	const uint32_t off = p - ix.nodeStart[seg], nodeLen = ix.nodeStart[seg + 1] - ix.nodeStart[seg] - 1;
	hit.nodeId = ix.nodeId[seg];
	hit.matchLen = len; hit.rawGoodness = len; hit.reverse = q.reverse;
	if (q.reverse) { hit.nodeOffset = nodeLen - off - len; hit.seqPos = q.len - i - len; }   // matchesToSeeds, src/MummerSeeder.cpp
	else { hit.nodeOffset = off; hit.seqPos = i; }
	tpos = p;
	return true;
}

// The defined order of a read's hits: matchLen descending, forward before reverse, query position in the searched orientation, text position. Two stable 64-bit sorts give it:
// first by mxmOrderKeyInner over the batch, then by mxmOrderKeyOuter.
GC_MXM_HD uint64_t mxmOrderKeyInner(uint32_t reverse, uint32_t i, uint32_t tpos) { return ((uint64_t)reverse << 63) | ((uint64_t)i << 32) | tpos; }   // (i < 2^31: a read is shorter)
GC_MXM_HD uint64_t mxmOrderKeyOuter(uint32_t read, uint32_t matchLen) { return ((uint64_t)read << 32) | (0xffffffffu - matchLen); }

} // namespace gcdev
