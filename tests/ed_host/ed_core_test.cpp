// The unit step of the edit-distance kernels (csrc/hip/gc_editdist_core.hpp) on the host: the core driven unit by unit (every unit a lane of its own), as the lanes of a
// team of 21 and of 32 (a lane moves through the units l, l + TEAM, ...), and over the whole matrix as the workgroup kernel drives it, each with the letter ring the kernels
// keep and its refill rule, against a plain DP held here. A sweep is ONE banded pass, as the kernels run it before they double k. The units of 2, 8 and 16 words run with
// the columns per step that k_edit_distance<G> gives them (edColsOfUnit) as well, on one lane per unit and on two or three lanes.
#include "gc_editdist_core.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using namespace gcdev;

static long failures = 0, sweeps = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint32_t plainDistance(const std::string& a, const std::string& b)
{
	std::vector<uint32_t> prev(b.size() + 1), cur(b.size() + 1);
	for (size_t j = 0; j <= b.size(); j++) prev[j] = (uint32_t)j;
	for (size_t i = 1; i <= a.size(); i++) {
		cur[0] = (uint32_t)i;
		for (size_t j = 1; j <= b.size(); j++) cur[j] = std::min({ prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] == b[j - 1] ? 0u : 1u) });
		prev.swap(cur);
	}
	return prev[b.size()];
}

static void eqMasks(const std::string& seq, uint64_t words, std::vector<uint64_t>& out)   // buildEqMasks of gc_runtime.hpp
{
	out.assign(4 * words, 0);
	for (size_t i = 0; i < seq.size(); i++) {
		const int b = seq[i] == 'A' ? 0 : seq[i] == 'C' ? 1 : seq[i] == 'G' ? 2 : seq[i] == 'T' ? 3 : -1;
		if (b >= 0) out[(uint64_t)b * words + (i >> 6)] |= 1ull << (i & 63);
	}
}

static uint32_t clampK(uint32_t k, uint32_t n, uint32_t m)   // what every kernel does to the k it is given
{
	const uint32_t diff = n > m ? n - m : m - n, cap = std::max(n, m);
	k = std::max(k, diff);
	if (k < 1) k = 1;
	return std::min(k, cap);
}

enum Mode { BANDED, FULL };

// the band (exclusive) a team is given: the shipped limit, which is derived for ED_COLS columns per step - with fewer columns, what the formula leaves of it
static uint32_t thirdLimit(uint32_t C) { return std::min(ED_THIRD_KMAX, edMaxBand(64, 21, C) + 1); }
static uint32_t halfLimit(uint32_t C) { return std::min(ED_HALF_KMAX, edMaxBand(64, 32, C) + 1); }

// One pass. lanes = 0: one lane per unit. Returns the value of the final cell, or -2 when the lanes or the ring cannot hold the band.
template <uint32_t C, int G>
static int64_t sweep(const std::string& read, const std::string& path, uint32_t kAsked, uint32_t lanes, uint32_t kMaxExclusive, uint32_t ringSize, Mode mode)
{
	constexpr uint32_t RB = 64u * G;
	sweeps++;
	const uint32_t n = (uint32_t)read.size(), m = (uint32_t)path.size();
	const uint32_t k = clampK(kAsked, n, m);
	const EdBand bd = edBand<RB>(n, m, k);
	if (lanes == 0) lanes = bd.nU;
	const uint32_t period = ringSize / (2 * C);
	if (mode == BANDED) {
		if (!edLanesHold(k, kMaxExclusive, bd.nU, lanes)) return -2;
		if (!edRingHolds<RB, C>(bd, ringSize, period)) return -2;
	} else if (((uint64_t)period + bd.nU - 1) * C > ringSize) return -2;
	auto window = [&](uint32_t b) { return mode == BANDED ? edWindow<RB, C>(bd, b) : edWindowFull<C>(bd, b); };
	// a lane's consecutive units are disjoint in time, and a unit starts no later than the unit above it ends
	for (uint32_t b = 0; b + lanes < bd.nU; b++) {
		const EdWindow w0 = window(b), w1 = window(b + lanes);
		CHECK(w0.tEnd < w1.tBegin, "units %u and %u of one lane overlap (n %u m %u k %u lanes %u C %u)", b, b + lanes, n, m, k, lanes, C);
	}
	for (uint32_t b = 1; b < bd.nU; b++) {
		const EdWindow up = window(b - 1), w = window(b);
		CHECK(w.tBegin != 0xffffffffu && (w.tBegin == b || (w.tBegin - 1 >= up.tBegin && w.tBegin - 1 <= up.tEnd)), "unit %u starts on a group its neighbour never computes (n %u m %u k %u C %u)", b, n, m, k, C);
	}
	const uint64_t words = (n + 63) / 64;
	std::vector<uint64_t> masks;
	eqMasks(read, words, masks);
	EdSource src { masks.data(), (uint32_t)words, path.data(), read.data(), n, m };
	std::vector<uint8_t> ring(ringSize, 0xee);
	std::vector<int64_t> ringCol(ringSize, -1);
	std::vector<EdUnit<G>> unit(lanes);
	std::vector<uint32_t> B(lanes);
	std::vector<uint8_t> fresh(lanes, 1);
	std::vector<EdWindow> w(lanes);
	std::vector<EdPub> pub(lanes, EdPub { 0, 0 }), before(lanes);
	for (uint32_t l = 0; l < lanes; l++) { B[l] = l; w[l] = window(l); memset(&unit[l], 0, sizeof(unit[l])); }
	int64_t result = -1;
	uint32_t loadedEnd = 0;
	const uint32_t steps = (m - 1) / C + bd.nU;
	for (uint32_t t = 0; t < steps; t++) {
		if (t % period == 0) {
			const uint32_t end = mode == BANDED ? edRingEnd<RB, C>(bd, t + period) : (uint32_t)std::min<uint64_t>((uint64_t)(t + period) * C, ((uint64_t)m + C - 1) / C * C);
			if (end > loadedEnd) {
				edRingFill(ring.data(), ringSize - 1, path.data(), m, loadedEnd, end, 0, 1);
				for (uint32_t c = loadedEnd; c < end; c++) ringCol[c & (ringSize - 1)] = c;
				loadedEnd = end;
			}
		}
		before = pub;
		for (uint32_t l = 0; l < lanes; l++) {
			const EdPub nb = before[(l + lanes - 1) % lanes];
			if (B[l] < bd.nU && t > w[l].tEnd) { do { B[l] += lanes; w[l] = window(B[l]); fresh[l] = 1; } while (B[l] < bd.nU && t > w[l].tEnd); }
			if (t < w[l].tBegin) continue;
			const uint32_t col0 = (t - B[l]) * C;
			for (uint32_t c = col0; c < col0 + C; c++) CHECK(ringCol[c & (ringSize - 1)] == (int64_t)c, "the ring does not hold column %u at step %u (n %u m %u k %u C %u ring %u)", c, t, n, m, k, C, ringSize);
			bool f = fresh[l] != 0;
			int32_t d = -1;
			if (edStep<C, G>(unit[l], f, w[l], src, B[l], t, nb, ring.data(), ringSize - 1, pub[l], d)) { CHECK(result == -1, "two final cells"); result = d; }
			fresh[l] = f;
		}
	}
	CHECK(result >= 0, "no final cell (n %u m %u k %u C %u)", n, m, k, C);
	return result;
}

struct Rng {
	std::mt19937_64 g;
	explicit Rng(uint64_t s) : g(s) {}
	uint32_t below(uint32_t n) { return (uint32_t)(g() % n); }
	double unit() { return (double)(g() >> 11) / 9007199254740992.0; }
	char letter(bool iupac) { static const char other[] = "NRYKMSWBDHV"; return iupac && below(20) == 0 ? other[below(11)] : "ACGT"[below(4)]; }
};

static std::string randomSeq(Rng& r, uint32_t len, bool iupac) { std::string s(len, 'A'); for (auto& c : s) c = r.letter(iupac); return s; }
static std::string mutate(Rng& r, const std::string& s, double rate, bool iupac)
{
	std::string out;
	for (char c : s) {
		if (r.unit() < rate) {
			const uint32_t what = r.below(3);
			if (what == 0) out.push_back(r.letter(iupac));                       // substitution
			else if (what == 1) { out.push_back(c); out.push_back(r.letter(iupac)); }   // insertion
		} else out.push_back(c);
	}
	return out;
}
static void fitColumns(Rng& r, std::string& path, uint32_t C, uint32_t rem)   // m % C == rem
{
	while (path.empty() || path.size() % C != rem % C) path.push_back(r.letter(false));
}

// every driver on one pair at one k
template <uint32_t C>
static void checkPair(const std::string& read, const std::string& path, uint32_t d, uint32_t kAsked, bool wide)
{
	const uint32_t n = (uint32_t)read.size(), m = (uint32_t)path.size(), k = clampK(kAsked, n, m);
	auto verdict = [&](int64_t got, const char* who) {
		if (got == -2) return;
		CHECK(got >= (int64_t)d, "%s: %lld below the distance %u (n %u m %u k %u C %u)", who, (long long)got, d, n, m, k, C);
		if (d <= k) CHECK(got == (int64_t)d, "%s: %lld, distance %u <= k %u (n %u m %u C %u)", who, (long long)got, d, k, n, m, C);
	};
	const int64_t perUnit = sweep<C, 1>(read, path, kAsked, 0, 0, 8192, BANDED);
	CHECK(perUnit != -2, "one lane per unit refused (n %u m %u k %u C %u)", n, m, k, C);
	verdict(perUnit, "one lane per unit");
	verdict(sweep<C, 1>(read, path, kAsked, 21, thirdLimit(C), 2048, BANDED), "team of 21");
	verdict(sweep<C, 1>(read, path, kAsked, 32, halfLimit(C), 4096, BANDED), "team of 32");
	// the limits of the formula itself, not only the shipped ones
	verdict(sweep<C, 1>(read, path, kAsked, 21, edMaxBand(64, 21, C) + 1, 2048, BANDED), "team of 21 at the formula's limit");
	verdict(sweep<C, 1>(read, path, kAsked, 32, edMaxBand(64, 32, C) + 1, 4096, BANDED), "team of 32 at the formula's limit");
	const int64_t full = sweep<C, 1>(read, path, kAsked, 0, 0, 16384, FULL);
	CHECK(full == (int64_t)d, "whole matrix: %lld, distance %u (n %u m %u C %u)", (long long)full, d, n, m, C);
	if (wide) {
		verdict(sweep<C, 2>(read, path, kAsked, 0, 0, 8192, BANDED), "units of two words");
		verdict(sweep<C, 4>(read, path, kAsked, 3, edMaxBand(256, 3, C) + 1, 8192, BANDED), "units of four words, three lanes");
		// the wide units with the columns per step k_edit_distance<G> gives them (edColsOfUnit), a lane moving through several units
		if constexpr (C == edColsOfUnit(2)) verdict(sweep<C, 2>(read, path, kAsked, 3, edMaxBand(128, 3, C) + 1, 8192, BANDED), "units of two words at their own columns, three lanes");
		if constexpr (C == edColsOfUnit(8)) {
			verdict(sweep<C, 8>(read, path, kAsked, 0, 0, 8192, BANDED), "units of eight words");
			verdict(sweep<C, 8>(read, path, kAsked, 2, edMaxBand(512, 2, C) + 1, 8192, BANDED), "units of eight words, two lanes");
		}
		if constexpr (C == edColsOfUnit(16)) {
			verdict(sweep<C, 16>(read, path, kAsked, 0, 0, 8192, BANDED), "units of sixteen words");
			verdict(sweep<C, 16>(read, path, kAsked, 2, edMaxBand(1024, 2, C) + 1, 8192, BANDED), "units of sixteen words, two lanes");
		}
	}
}

template <uint32_t C>
static void checkAllK(const std::string& read, const std::string& path, bool wide)
{
	const uint32_t d = plainDistance(read, path), cap = (uint32_t)std::max(read.size(), path.size());
	const uint32_t ks[] = { 1, d / 2 + 1, d, d + 1, d + 8, 2 * d + 3, cap };
	uint32_t seen[7]; int nSeen = 0;
	for (uint32_t k : ks) {
		const uint32_t kc = clampK(k, (uint32_t)read.size(), (uint32_t)path.size());
		if (std::find(seen, seen + nSeen, kc) != seen + nSeen) continue;   // (the same clamped k: the same sweep)
		seen[nSeen++] = kc;
		checkPair<C>(read, path, d, k, wide);
	}
}

template <uint32_t C>
static void checkColumns(uint64_t seed)
{
	Rng r(seed * 1000 + C);
	const uint32_t lengths[] = { 1, C > 1 ? C - 1 : 2, C, C + 1, 63, 64, 65, 127, 128, 129, 700, 64 * 21 - 1, 64 * 21, 64 * 21 + 1, 64 * 32 - 1, 64 * 32, 64 * 32 + 1, 3000 };
	const double rates[] = { 0.0, 0.05, 0.2, 0.5 };
	int turn = 0;
	for (uint32_t len : lengths) for (double rate : rates) {
		const bool iupac = (turn % 3) == 2;                        // every third pair carries letters outside ACGT, in the read and in the path
		const uint32_t rems[3] = { 0, 1, C - 1 };
		const uint32_t rem = rems[turn % 3];
		turn++;
		std::string read = randomSeq(r, len, iupac), path = mutate(r, read, rate, iupac);
		fitColumns(r, path, C, rem);
		if (iupac && path.size() > C) { path[path.size() / C / 2 * C] = 'N'; if (C > 1) path[path.size() / C / 2 * C + 1] = 'A'; }   // a group that mixes both kinds
		const bool wide = len <= 700 || rate == 0.05;
		checkAllK<C>(read, path, wide);
		checkAllK<C>(path, read, wide);                           // both orders
		// every remainder of m at the small lengths, where the last group is most of the matrix
		if (len <= 129) for (uint32_t extra = 1; extra < C; extra++) { std::string p2 = path + randomSeq(r, extra, false); checkAllK<C>(read, p2, false); }
	}
	{   // very unequal lengths
		std::string a = randomSeq(r, 300, false), b = randomSeq(r, 2000, false);
		b.replace(900, 300, mutate(r, a, 0.1, false));
		checkAllK<C>(a, b, true);
		checkAllK<C>(b, a, true);
	}
}

// At the class limit a lane's units stay disjoint (sweep() checks every pair of them) and the answer is exact; one above it the lanes refuse.
template <uint32_t C>
static void checkLimits(uint64_t seed)
{
	Rng r(seed);
	for (uint32_t len : { 64u * 21 + 1, 64u * 32 + 1, 3000u, 10000u }) for (double rate : { 0.05, 0.3 }) {
		std::string read = randomSeq(r, len, false), path = mutate(r, read, rate, false);
		const uint32_t n = (uint32_t)read.size(), m = (uint32_t)path.size(), d = plainDistance(read, path);
		struct Team { uint32_t lanes, kMax, ring; } teams[] = { { 21, thirdLimit(C), 2048 }, { 32, halfLimit(C), 4096 }, { 21, edMaxBand(64, 21, C) + 1, 2048 }, { 32, edMaxBand(64, 32, C) + 1, 4096 } };
		for (const Team& tm : teams) {
			if (clampK(tm.kMax, n, m) != tm.kMax) continue;        // (the pair is too short for a band that wide)
			const int64_t at = sweep<C, 1>(read, path, tm.kMax - 1, tm.lanes, tm.kMax, tm.ring, BANDED);
			CHECK(at >= (int64_t)d && (d > tm.kMax - 1 || at == (int64_t)d), "team of %u at its limit %u: %lld, distance %u (n %u m %u C %u)", tm.lanes, tm.kMax - 1, (long long)at, d, n, m, C);
			const int64_t over = sweep<C, 1>(read, path, tm.kMax, tm.lanes, tm.kMax, tm.ring, BANDED);
			CHECK((n + 63) / 64 > tm.lanes ? over == -2 : over >= (int64_t)d, "team of %u one above its limit: %lld (n %u m %u C %u)", tm.lanes, (long long)over, n, m, C);
		}
	}
}

// one past each ring size, at the length the rings were sized for, and n == m with a band of one diagonal
template <uint32_t C>
static void checkRings(uint64_t seed)
{
	Rng r(seed);
	for (uint32_t len : { 2049u, 4097u, 8193u }) for (uint32_t rem : { 0u, 1u, C - 1 }) {
		std::string read = randomSeq(r, len, false), path = mutate(r, read, 0.02, false);
		fitColumns(r, path, C, rem);
		const uint32_t d = plainDistance(read, path);
		checkPair<C>(read, path, d, d + 8, true);
		checkPair<C>(path, read, d, 1899, false);
	}
	for (uint32_t len : { 1u, 5u, 64u, 65u, 200u, 1500u }) {
		std::string read = randomSeq(r, len, false), path = read;
		checkPair<C>(read, path, 0, 1, true);
		path[len / 2] = path[len / 2] == 'A' ? 'C' : 'A';
		checkPair<C>(read, path, 1, 1, true);
	}
}

// Pairs whose optimal path runs along the corridor's edge: X + S against S + Y with |X| = |Y| = s (the path leaves the main diagonal at once, follows the diagonal s away from
// it and comes back in the last s columns: both edges of the corridor at k = d) and X + S against S (the overhang: one edge), with k one below, at and one above the
// distance, both orders. A mutated pair stays near the main diagonal, where a corridor one diagonal too narrow costs nothing.
struct EdgePair { std::string a, b; uint32_t d; };
static std::vector<EdgePair> edgePairs(uint64_t seed)
{
	Rng r(seed + 77);
	std::vector<EdgePair> out;
	for (uint32_t len : { 200u, 700u, 2049u, 5000u }) for (uint32_t s : { 1u, 31u, 64u, 65u, 300u }) {
		const std::string S = randomSeq(r, len, false), X = randomSeq(r, s, false), Y = randomSeq(r, s, false);
		out.push_back({ X + S, S + Y, 0 });
		out.push_back({ X + S, S, 0 });
	}
	for (EdgePair& p : out) p.d = plainDistance(p.a, p.b);
	return out;
}
template <uint32_t C>
static void checkEdges(const std::vector<EdgePair>& pairs)
{
	for (const EdgePair& p : pairs) for (uint32_t k : { p.d - 1, p.d, p.d + 1 }) {
		checkPair<C>(p.a, p.b, p.d, k, true);
		checkPair<C>(p.b, p.a, p.d, k, true);
	}
}

int main(int argc, char** argv)
{
	const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
	static_assert(edMaxBand(64, 21, 1) == 1301 && edMaxBand(64, 21, 8) == 1441 && edMaxBand(64, 32, 8) == 2233, "the band a team holds");
	checkColumns<1>(seed); checkColumns<2>(seed); checkColumns<4>(seed); checkColumns<8>(seed);
	checkLimits<1>(seed); checkLimits<4>(seed); checkLimits<8>(seed);
	checkRings<1>(seed); checkRings<4>(seed); checkRings<8>(seed);
	const std::vector<EdgePair> edges = edgePairs(seed);
	checkEdges<1>(edges); checkEdges<2>(edges); checkEdges<4>(edges); checkEdges<8>(edges);
	if (failures) { printf("FAILED: %ld checks of %ld sweeps\n", failures, sweeps); return 1; }
	printf("OK %ld sweeps\n", sweeps);
	return 0;
}
