// The host side of the MUM / MEM index (gc_mxm_index_create): the text, its suffix array and the packed form the kernels read. Standard library only, so that a CPU program can
// drive it (tests/mxm_host).
//   text           every original segment forward, in ascending node id, each followed by a separator; a, c, g, t (u) in either case are letters, everything else is a separator
//                  at its own position, so text position - segment start is the offset in the segment (lowercaseRef, src/MummerSeeder.cpp)
//   suffix array   of the whole text over separator < a < c < g < t, a suffix that is a prefix of another first: every position, separators included (the reference's is
//                  create_auto(seq, size, 0, true): full, K = 1). Built by prefix doubling from a 21-letter radix key, refining only the groups that are still tied
//                  (Larsson-Sadakane): a round costs the size of the unresolved groups times the log of the largest, and a repeat of length L takes log2(L / 21) rounds -
//                  nothing depends on L itself, and a text without long repeats is done after the first sort.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstddef>
#include <utility>
#include <vector>

namespace gc {

// letters of the direct-address table in front of the suffix array: 4^12 intervals of 8 bytes = 128 MiB, and what is left of a 20-letter window's search is a handful of steps
inline constexpr uint32_t MXM_PREFIX_LEN = 12;

// the device build of the suffix array (hip/gc_mxm_sa.hip) counts its items in int, as hipCUB does: it takes a text of fewer letters than this, the host build any text the
// index's 32-bit positions hold
inline constexpr uint64_t MXM_DEVICE_BUILD_MAX = 0x7fffffffull;
inline bool mxmDeviceBuildTakes(uint64_t letters) { return letters < MXM_DEVICE_BUILD_MAX; }

struct MxmText {
	std::vector<uint8_t> codes;        // 0 separator, 1..4 = a c g t
	std::vector<uint32_t> nodeStart;   // [segments + 1]; the last entry is the text's length
	std::vector<int32_t> nodeId;
};   // (32-bit positions: the caller refuses a text of 2^32 - 16 letters or more before anything is appended)

inline uint8_t mxmRefCode(char c)
{
	switch (c) {
		case 'A': case 'a': return 1; case 'C': case 'c': return 2; case 'G': case 'g': return 3; case 'T': case 't': case 'U': case 'u': return 4;
	}
	return 0;
}

// segments must arrive in ascending node id
inline void mxmAppendSegment(MxmText& t, int32_t nodeId, const char* letters, size_t n)
{
	t.nodeStart.push_back((uint32_t)t.codes.size());
	t.nodeId.push_back(nodeId);
	for (size_t i = 0; i < n; i++) t.codes.push_back(mxmRefCode(letters[i]));
	t.codes.push_back(0);
}
inline void mxmFinishText(MxmText& t) { t.nodeStart.push_back((uint32_t)t.codes.size()); }

// parallelFor(n, body): runs body(i) for i in [0, n), on as many threads as the caller has (the library passes its worker pool, a test a plain loop); rounds: the doubling
// rounds it took after the first sort, when asked for
template <class ParallelFor>
std::vector<uint32_t> mxmSuffixArray(const uint8_t* codes, uint32_t n, ParallelFor&& parallelFor, uint32_t* rounds = nullptr)
{
	std::vector<uint32_t> sa(n);
	if (rounds) *rounds = 0;
	if (!n) return sa;
	constexpr uint32_t K = 21;   // letters of the first key: 3 bits each (0 beyond the text, separator 1, letters 2..5)
	std::vector<uint64_t> key(n);
	const uint32_t CHUNK = 1u << 16, nChunks = (n + CHUNK - 1) / CHUNK;
	parallelFor((size_t)nChunks, [&](size_t c) {
		const uint32_t a = (uint32_t)c * CHUNK, b = std::min<uint64_t>(n, (uint64_t)a + CHUNK);
		uint64_t k = 0;   // the key of position b: the chunk's own keys follow from it one letter at a time
		for (uint32_t j = 0; j < K && (uint64_t)b + j < n; j++) k |= (uint64_t)(codes[b + j] + 1) << (60 - 3 * j);
		for (uint32_t i = b; i-- > a;) { k = ((uint64_t)(codes[i] + 1) << 60) | (k >> 3); key[i] = k; }
	});
	// first sort: buckets by the first four letters (12 bits), every bucket sorted by (key, position) on its own
	constexpr uint32_t BUCKET_BITS = 12, BUCKETS = 1u << BUCKET_BITS;
	std::vector<uint32_t> bucketOff(BUCKETS + 1, 0);
	for (uint32_t i = 0; i < n; i++) bucketOff[(key[i] >> (63 - BUCKET_BITS)) + 1]++;
	for (uint32_t b = 0; b < BUCKETS; b++) bucketOff[b + 1] += bucketOff[b];
	{
		std::vector<uint32_t> at(bucketOff.begin(), bucketOff.end() - 1);
		for (uint32_t i = 0; i < n; i++) sa[at[key[i] >> (63 - BUCKET_BITS)]++] = i;
	}
	parallelFor((size_t)BUCKETS, [&](size_t b) {
		std::sort(sa.begin() + bucketOff[b], sa.begin() + bucketOff[b + 1], [&](uint32_t x, uint32_t y) { return key[x] != key[y] ? key[x] < key[y] : x < y; });
	});
	// rank = the index of the group's first suffix; groups = the runs of equal keys with more than one member
	std::vector<uint32_t> rank(n);
	std::vector<std::pair<uint32_t, uint32_t>> groups, next;
	for (uint32_t a = 0; a < n;) {
		uint32_t b = a + 1;
		while (b < n && key[sa[b]] == key[sa[a]]) b++;
		for (uint32_t i = a; i < b; i++) rank[sa[i]] = a;
		if (b - a > 1) groups.emplace_back(a, b);
		a = b;
	}
	std::vector<uint64_t>().swap(key);
	// doubling: the members of a group agree in their first h letters, so rank[i + h] orders them by their first 2h. A group reads ranks of other groups and writes only its own
	// members' (after every group has been sorted: the new ranks are staged in `fresh`), so groups are independent within a round.
	std::vector<uint32_t> fresh;
	for (uint64_t h = K; !groups.empty(); h *= 2) {
		if (rounds) ++*rounds;
		auto second = [&](uint32_t i) -> int64_t { return (uint64_t)i + h < n ? (int64_t)rank[i + h] : -1; };
		parallelFor(groups.size(), [&](size_t g) {
			std::sort(sa.begin() + groups[g].first, sa.begin() + groups[g].second, [&](uint32_t x, uint32_t y) { return second(x) < second(y); });
		});
		size_t members = 0;
		for (const auto& g : groups) members += g.second - g.first;
		fresh.resize(members);
		next.clear();
		size_t at = 0;
		for (const auto& g : groups) {
			for (uint32_t a = g.first; a < g.second;) {
				uint32_t b = a + 1;
				while (b < g.second && second(sa[b]) == second(sa[a])) b++;
				for (uint32_t i = a; i < b; i++) fresh[at++] = a;
				if (b - a > 1) next.emplace_back(a, b);
				a = b;
			}
		}
		at = 0;
		for (const auto& g : groups) for (uint32_t i = g.first; i < g.second; i++) rank[sa[i]] = fresh[at++];
		groups.swap(next);
	}
	return sa;
}

// the text as the kernels read it: 2 bits per letter and one "not a letter" bit per position, first position in the top bits; positions at and beyond n count as separators
inline void mxmPackText(const uint8_t* codes, uint32_t n, std::vector<uint64_t>& packed, std::vector<uint64_t>& invalid)
{
	packed.assign(((size_t)n >> 5) + 2, 0);
	invalid.assign(((size_t)n >> 6) + 2, ~0ull);
	for (uint32_t i = 0; i < n; i++) {
		if (!codes[i]) continue;
		packed[i >> 5] |= (uint64_t)(codes[i] - 1) << (62 - 2 * (i & 31));
		invalid[i >> 6] &= ~(1ull << (63 - (i & 63)));
	}
}

} // namespace gc
