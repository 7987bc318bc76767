// The unit step of the banded edit-distance kernels (gc_editdist.hip), the part that compiles for the host as well as for the device (tests/ed_host):
//   edBand / edWindow    Ukkonen's corridor of a pair and the steps at which one unit (64 G rows) is inside it
//   edStep               one step of one unit: C columns of Myers' recurrence, the publication for the unit below, the final cell
//   edRingHolds / edRingEnd / edRingFill   which path letters the letter ring has to hold at a step
//
// Rows = read bases, 64 per word; a unit is G consecutive words. The units sweep the matrix as a skewed wavefront of column GROUPS: at step t unit B
// works on group g = t - B, the columns gC .. min(gC + C - 1, m - 1), in one unrolled loop of C Myers columns. The window tests, the unit change, the
// neighbour hand-off, the ring read and the refill test are paid once per step, so a sweep costs (m / C + units) steps of (overhead + C columns)
// instead of (m + units) steps of (overhead + 1 column). After a step a unit publishes, for the unit below it,
//   - the score of its bottom row after the group's last computed column, and
//   - the group's horizontal deltas of that row as bit fields: bit c = column c went +1, bit C + c = column c went -1;
// the unit below reads it one step later, when it is on the same group. A unit that starts in the middle of the matrix ("fresh") takes the
// neighbour's score minus the sum of those deltas - the neighbour's bottom row one column before the group - plus its own rows, all +1.
// The corridor is kept in whole groups (gBegin = c0 / C, gEnd = lastCol / C): it only widens, band values stay upper bounds that are exact along
// every path of cost <= k, so a result <= k is still the distance. Whether the upper neighbour feeds a unit is decided per group as well.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GC_ED_HD __host__ __device__ __forceinline__
#define GC_ED_UNROLL _Pragma("unroll")
#define GC_ED_NOUNROLL _Pragma("nounroll")
#else
#define GC_ED_HD inline
#define GC_ED_UNROLL
#define GC_ED_NOUNROLL
#endif

namespace gcdev {

// A lane owns the units l, l + lanes, ...: unit B is inside the corridor for the groups c0(B) / C .. lastCol(B) / C with c0 >= rows B - reachRight,
// lastCol <= rows B + rows - 1 + reachLeft and reachLeft + reachRight <= k, at the steps group + B. The lane's units B and B + lanes are disjoint in
// time iff lastCol(B) / C < c0(B + lanes) / C + lanes, which holds whenever c0(B + lanes) + C lanes - lastCol(B) >= C, i.e. for every
// k <= rows lanes + C lanes - (rows - 1) - C = (rows + C)(lanes - 1) + 1.
GC_ED_HD constexpr uint32_t edMaxBand(uint32_t rowsPerUnit, uint32_t lanes, uint32_t cols) { return (rowsPerUnit + cols) * (lanes - 1) + 1; }

// Columns per step, and the bands (exclusive) up to which the teams of 32 and of 21 lanes (two and three pairs per wave) take a pair whose read has more
// units than the team has lanes: three pairs per wave up to all that the formula allows, two per wave as before the column groups.
// C = 8 is one 64-bit LDS read per group; measured against C = 4 in DESIGN.md section 3.7 (`make variant NAME=c4 FLAGS=-DGC_ED_COLS=4` builds the other one).
#ifndef GC_ED_COLS
#define GC_ED_COLS 8
#endif
constexpr uint32_t ED_COLS = GC_ED_COLS;
constexpr uint32_t ED_HALF_KMAX = 1900, ED_THIRD_KMAX = edMaxBand(64, 21, ED_COLS) + 1;   // 1 442 at C = 8
// a unit of G words runs G Myers words per column, so the per-step overhead is already spread over G of them and C G words of temporaries have to fit the
// registers: the wide units take fewer columns per step
GC_ED_HD constexpr uint32_t edColsOfUnit(uint32_t words) { return words >= ED_COLS ? 1u : ED_COLS / words; }
static_assert(ED_HALF_KMAX - 1 <= edMaxBand(64, 32, ED_COLS) && ED_THIRD_KMAX - 1 <= edMaxBand(64, 21, ED_COLS), "a lane's consecutive units must stay disjoint in time");
// false: the band is too wide for a lane's consecutive units to stay apart (with one unit per lane at most there is nothing to keep apart: any band works)
GC_ED_HD bool edLanesHold(uint32_t k, uint32_t kMaxExclusive, uint32_t nU, uint32_t lanes) { return k < kMaxExclusive || nU <= lanes; }

GC_ED_HD constexpr uint32_t edColsMask(uint32_t cols) { return (1u << cols) - 1u; }
GC_ED_HD int edPop(uint64_t v) { return __builtin_popcountll(v); }
GC_ED_HD int32_t edDeltaSum(uint32_t bits, uint32_t cols) { return edPop(bits & edColsMask(cols)) - edPop(bits >> cols); }
GC_ED_HD uint8_t edLetterCode(uint8_t ch) { return ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : 4; }

struct EdBand {
	uint32_t n, m, nU, lastUnit;      // rows, columns, units, the unit that holds row n - 1
	uint32_t reachRight, reachLeft;   // row - column at most reachRight, column - row at most reachLeft
};

// Ukkonen's corridor: a path of cost <= k from (0,0) to (n-1,m-1) spends at least |row - column| to get where it is and at least
// |(n - m) - (row - column)| to get home, so it only visits diagonals with |d| + |(n - m) - d| <= k: from min(0, n-m) - a to
// max(0, n-m) + a with a = (k - |n-m|) / 2. n, m >= 1 and |n - m| <= k.
template <uint32_t RB>
GC_ED_HD EdBand edBand(uint32_t n, uint32_t m, uint32_t k)
{
	EdBand bd;
	bd.n = n; bd.m = m;
	bd.nU = (n + RB - 1) / RB;
	bd.lastUnit = (n - 1) / RB;
	const uint32_t diff = n > m ? n - m : m - n;
	uint32_t slack = (k - diff) / 2;
	// a corridor of one diagonal (n == m, k = 1): a unit starts on the column below its upper neighbour's last row, which the neighbour never
	// computes, and would read a stale publication - one diagonal of slack on either side keeps c0(B) <= lastCol(B - 1)
	if (n == m && slack == 0) slack = 1;
	bd.reachRight = (n > m ? n - m : 0) + slack;   // (at most max(n, m) + 1)
	bd.reachLeft = (m > n ? m - n : 0) + slack;
	return bd;
}

struct EdWindow { uint32_t tBegin, tEnd, tHinEnd, finalStep; };   // steps of one unit: first, last, last one whose group the upper neighbour also computes, the one with column m - 1 (last unit only)

template <uint32_t RB, uint32_t C>
GC_ED_HD EdWindow edWindow(const EdBand& bd, uint32_t b)
{
	EdWindow w { 0xffffffffu, 0xffffffffu, 0, 0xffffffffu };
	if (b >= bd.nU) return w;
	const uint64_t rowBase = (uint64_t)RB * b;
	const uint64_t c0 = rowBase > bd.reachRight ? rowBase - bd.reachRight : 0;
	const uint64_t c1 = rowBase + RB - 1 + bd.reachLeft;
	const uint64_t lastCol = c1 < bd.m - 1 ? c1 : bd.m - 1;
	w.tBegin = c0 > lastCol ? 0xffffffffu : (uint32_t)(c0 / C + b);   // (a unit below the band at every column never runs)
	w.tEnd = (uint32_t)(lastCol / C + b);
	if (b > 0) { const uint64_t up = rowBase - 1 + bd.reachLeft; w.tHinEnd = (uint32_t)((up < bd.m - 1 ? up : bd.m - 1) / C + b); }
	if (b == bd.lastUnit) w.finalStep = (bd.m - 1) / C + b;
	return w;
}
// the whole matrix, no corridor (the workgroup kernel): every unit computes every group
template <uint32_t C>
GC_ED_HD EdWindow edWindowFull(const EdBand& bd, uint32_t b)
{
	EdWindow w { 0xffffffffu, 0xffffffffu, 0, 0xffffffffu };
	if (b >= bd.nU) return w;
	w.tBegin = b;
	w.tEnd = (bd.m - 1) / C + b;
	w.tHinEnd = b > 0 ? w.tEnd : 0;
	if (b == bd.lastUnit) w.finalStep = w.tEnd;
	return w;
}

// ---- the letter ring: one code per column (0-3 = ACGT, 4 = any other letter), RING a power of two, refilled every PERIOD steps.
// Columns read at step t lie in [lo(t), hi(t)], by either of two arguments:
//   by units: unit B reads the group t - B, 0 <= B < nU:                      (t - nU + 1) C <= column <= t C + C - 1
//   by band:  unit B is inside the corridor on the group's first column x:     RB B - reachRight - (C - 1) <= x <= RB B + RB - 1 + reachLeft,
//             and t C = x + B C, so  (C RB t - C (reachRight + C - 1)) / (RB + C) <= x <= (C RB t + C (RB - 1 + reachLeft)) / (RB + C)
// The refill at step t0 loads up to hi(t0 + PERIOD - 1) and overwrites what lies RING columns before that, so the ring serves a pass when
// hi(t0 + PERIOD - 1) + 1 - lo(t0) <= RING for every t0 by one of the two.
template <uint32_t RB, uint32_t C>
GC_ED_HD bool edRingHolds(const EdBand& bd, uint32_t ring, uint32_t period)
{
	const uint64_t byUnits = ((uint64_t)period + bd.nU - 1) * C;
	const uint64_t byBand = ((uint64_t)C * ((uint64_t)RB * (period - 1) + RB + (uint64_t)bd.reachLeft + bd.reachRight + C - 2)) / (RB + C) + C + 2;
	return byUnits <= ring || byBand <= ring;
}
// one past the last column any unit reads before step tNext, at most m rounded up to a whole group (the columns from m on are filled with code 0)
template <uint32_t RB, uint32_t C>
GC_ED_HD uint32_t edRingEnd(const EdBand& bd, uint32_t tNext)
{
	const uint64_t tl = tNext - 1;
	const uint64_t byUnits = tl * C + C;
	const uint64_t byBand = ((uint64_t)C * RB * tl + (uint64_t)C * ((uint64_t)RB - 1 + bd.reachLeft)) / (RB + C) + C;
	const uint64_t mPad = ((uint64_t)bd.m + C - 1) / C * C;
	uint64_t end = byUnits < byBand ? byUnits : byBand;
	return (uint32_t)(end < mPad ? end : mPad);
}
// the columns from + first, from + first + stride, ... below end
GC_ED_HD void edRingFill(uint8_t* ring, uint32_t ringMask, const char* path, uint32_t m, uint32_t from, uint32_t end, uint32_t first, uint32_t stride)
{
	for (uint32_t c = from + first; c < end; c += stride) ring[c & ringMask] = c < m ? edLetterCode((uint8_t)path[c]) : (uint8_t)0;
}
// the C codes of the group that starts at column col (a multiple of C): one aligned read of C bytes
template <uint32_t C>
GC_ED_HD uint64_t edRingRead(const uint8_t* ring, uint32_t ringMask, uint32_t col)
{
	static_assert(C == 1 || C == 2 || C == 4 || C == 8, "a group is read from the ring in one piece");
	const uint8_t* p = ring + (col & ringMask);
	if (C == 8) { uint64_t v; __builtin_memcpy(&v, __builtin_assume_aligned(p, 8), 8); return v; }
	if (C == 4) { uint32_t v; __builtin_memcpy(&v, __builtin_assume_aligned(p, 4), 4); return v; }
	if (C == 2) { uint16_t v; __builtin_memcpy(&v, __builtin_assume_aligned(p, 2), 2); return v; }
	return *p;
}

// ---- one unit
template <int G> struct EdUnit {
	uint64_t VP[G], VN[G];               // vertical deltas of the unit's rows in the last computed column
	uint64_t eqA[G], eqC[G], eqG[G], eqT[G];
	int32_t score;                       // the unit's bottom row in the last computed column
};
struct EdPub { int32_t score; uint32_t bits; };
struct EdSource {
	const uint64_t* masks;               // [A,C,G,T][words] exact-match bit vectors of the read
	uint32_t words;
	const char* path;                    // the m column letters
	const char* readBases;               // the n row letters
	uint32_t n, m;
};

// one column of Myers' recurrence down the G words of a unit; hP/hN: the horizontal delta entering at the top, leaving at the bottom
template <int G, bool EXACT>
GC_ED_HD void edColumn(EdUnit<G>& u, const EdSource& s, uint32_t B, uint32_t code, uint32_t col, uint64_t& hP, uint64_t& hN)
{
GC_ED_UNROLL
	for (int q = 0; q < G; q++) {
		uint64_t Eq;
		if (EXACT || code < 4) {
			const uint64_t lo = (code & 1) ? u.eqC[q] : u.eqA[q], hi = (code & 1) ? u.eqT[q] : u.eqG[q];
			Eq = (code & 2) ? hi : lo;
		} else {                             // any other letter: compare the 64 read bases of this word directly
			Eq = 0;
			const uint8_t letter = (uint8_t)s.path[col];
			const uint64_t row0 = 64ull * ((uint64_t)G * B + q);
			GC_ED_NOUNROLL
			for (uint32_t i = 0; i < 64 && row0 + i < s.n; i++) if ((uint8_t)s.readBases[row0 + i] == letter) Eq |= 1ull << i;
		}
		const uint64_t vp = u.VP[q], vn = u.VN[q];
		const uint64_t Xv = Eq | vn;
		Eq |= hN;
		const uint64_t Xh = (((Eq & vp) + vp) ^ vp) | Eq;
		uint64_t Ph = vn | ~(Xh | vp);
		uint64_t Mh = vp & Xh;
		const uint64_t outP = Ph >> 63, outN = Mh >> 63;
		Ph = (Ph << 1) | hP;
		Mh = (Mh << 1) | hN;
		u.VP[q] = Mh | ~(Xv | Ph);
		u.VN[q] = Ph & Xv;
		hP = outP; hN = outN;
	}
}

// the cell (n - 1, m - 1) from the last unit's bottom row in column m - 1: subtract the deltas of the padding rows below row n - 1
template <int G>
GC_ED_HD int32_t edFinal(const EdUnit<G>& u, uint32_t B, uint32_t n)
{
	int32_t d = u.score;
GC_ED_UNROLL
	for (int q = 0; q < G; q++) {
		const uint64_t row0 = 64ull * ((uint64_t)G * B + q);
		uint64_t pad = 0;
		if (row0 >= n) pad = ~0ull;
		else if (row0 + 64 > n) pad = ~0ull << (n - row0);
		d -= edPop(u.VP[q] & pad);
		d += edPop(u.VN[q] & pad);
	}
	return d;
}

// a unit about to compute its first column: all +1 below whatever lies above it, and the read's exact-match vectors of its words
template <int G>
GC_ED_HD void edEnter(EdUnit<G>& u, const EdSource& s, uint32_t B)
{
GC_ED_UNROLL
	for (int q = 0; q < G; q++) {
		u.VP[q] = ~0ull; u.VN[q] = 0;
		const uint32_t word = (uint32_t)G * B + q;
		const bool in = word < s.words;
		u.eqA[q] = in ? s.masks[word] : 0ull;
		u.eqC[q] = in ? s.masks[(uint64_t)s.words + word] : 0ull;
		u.eqG[q] = in ? s.masks[2ull * s.words + word] : 0ull;
		u.eqT[q] = in ? s.masks[3ull * s.words + word] : 0ull;
	}
}

// Step t of unit B, w.tBegin <= t <= w.tEnd. nb: what the unit above published one step ago (anything for B = 0). Returns true when this step held the
// final cell, whose value is then in result.
template <uint32_t C, int G>
GC_ED_HD bool edStep(EdUnit<G>& u, bool& fresh, const EdWindow& w, const EdSource& s, uint32_t B, uint32_t t, const EdPub& nb, const uint8_t* ring, uint32_t ringMask, EdPub& pub, int32_t& result)
{
	constexpr uint32_t RB = 64u * G, ALL = edColsMask(C);
	constexpr uint64_t OTHER = 0x0404040404040404ull & (C == 8 ? ~0ull : (1ull << (8 * (C & 7))) - 1);
	const uint32_t g = t - B, col0 = g * C;
	if (fresh) {
		fresh = false;
		edEnter<G>(u, s, B);
		if (g == 0) u.score = (int32_t)(RB * (B + 1));                         // the column before the first: D[i][-1] = i + 1
		else u.score = nb.score - edDeltaSum(nb.bits, C) + (int32_t)RB;        // below the upper neighbour's column before this group, all +1
	}
	const uint64_t codes = edRingRead<C>(ring, ringMask, col0);
	const uint32_t in = (B > 0 && t <= w.tHinEnd) ? nb.bits : ALL;             // top of the band (and row -1 of the matrix): +1 per column
	const uint32_t cnt = s.m - col0 < C ? s.m - col0 : C;
	uint32_t out = 0;
	if (C > 1 && cnt == C && !(codes & OTHER)) {   // (a group of one column has nothing to unroll: the general loop does it)
GC_ED_UNROLL
		for (uint32_t c = 0; c < C; c++) {
			uint64_t hP = (in >> c) & 1u, hN = (in >> (C + c)) & 1u;
			edColumn<G, true>(u, s, B, (uint32_t)(codes >> (8 * c)) & 3u, col0 + c, hP, hN);
			out |= ((uint32_t)hP << c) | ((uint32_t)hN << (C + c));
		}
	} else {                                 // the group with column m - 1 when m is no multiple of C, and a group with a letter outside ACGT
		GC_ED_NOUNROLL
		for (uint32_t c = 0; c < cnt; c++) {
			uint64_t hP = (in >> c) & 1u, hN = (in >> (C + c)) & 1u;
			edColumn<G, false>(u, s, B, (uint32_t)(codes >> (8 * c)) & 7u, col0 + c, hP, hN);
			out |= ((uint32_t)hP << c) | ((uint32_t)hN << (C + c));
		}
	}
	u.score += edDeltaSum(out, C);
	pub.score = u.score;
	pub.bits = out;
	if (t != w.finalStep) return false;
	result = edFinal<G>(u, B, s.n);
	return true;
}

} // namespace gcdev
