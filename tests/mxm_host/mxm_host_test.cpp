// CPU program for tests/test_mxm_host.py: the MUM / MEM seeder's host builder (csrc/host/gc_mxm_build.hpp) and its per-position routine (csrc/hip/gc_mxm_core.hpp) compiled with g++.
//   mxm_host_test sa                the suffix array of the product's builder against a naive suffix sort, on the texts listed in main(); the homopolymer build is timed
//   mxm_host_test hits <case file>  the per-position routine on one lane, serially over every (read, strand, position), in the defined order; prints the hits
// Case file: "<mode> <min_len> <count or -1> <prefix_len or 0>", then "S <n>" and n lines "<id> <sequence or *>", then "R <n>" and n lines "<read or *>".
#include "gc_mxm_build.hpp"
#include "gc_mxm_core.hpp"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <iostream>
#include <random>
#include <string>
#include <tuple>
#include <vector>

using namespace gcdev;

static void serialFor(size_t n, const std::function<void(size_t)>& body) { for (size_t i = 0; i < n; i++) body(i); }

struct HostIndex {
	gc::MxmText text;
	std::vector<uint32_t> sa, prefix;
	std::vector<uint64_t> packed, invalid;
	MxmIndexView view {};
	void build(uint32_t prefixLen)
	{
		gc::mxmFinishText(text);
		const uint32_t n = (uint32_t)text.codes.size();
		sa = gc::mxmSuffixArray(text.codes.data(), n, serialFor);
		gc::mxmPackText(text.codes.data(), n, packed, invalid);
		view = MxmIndexView { sa.data(), packed.data(), invalid.data(), text.nodeStart.data(), text.nodeId.data(), nullptr, n, (uint32_t)text.nodeId.size(), prefixLen };
		if (prefixLen) {   // what k_mxm_prefix_table leaves: [lo, hi) of every prefixLen-mer, (0, 0) for the absent ones
			prefix.assign((size_t)2 << (2 * prefixLen), 0);
			for (uint32_t idx = 0; idx < n; idx++) {
				uint64_t code = 0;
				bool whole = true;
				for (uint32_t j = 0; j < prefixLen && whole; j++) { whole = sa[idx] + j < n && text.codes[sa[idx] + j]; if (whole) code = code << 2 | (text.codes[sa[idx] + j] - 1); }
				if (!whole) continue;
				if (prefix[2 * code + 1] == 0) prefix[2 * code] = idx;
				prefix[2 * code + 1] = idx + 1;
			}
			view.prefix = prefix.data();
		}
	}
};

static bool checkSuffixArray(const char* what, const std::vector<std::pair<int, std::string>>& segments, double* seconds = nullptr)
{
	HostIndex ix;
	for (const auto& s : segments) gc::mxmAppendSegment(ix.text, s.first, s.second.data(), s.second.size());
	gc::mxmFinishText(ix.text);
	const std::vector<uint8_t>& c = ix.text.codes;
	const uint32_t n = (uint32_t)c.size();
	const auto t0 = std::chrono::steady_clock::now();
	const std::vector<uint32_t> sa = gc::mxmSuffixArray(c.data(), n, serialFor);
	if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
	std::vector<uint32_t> naive(n);
	for (uint32_t i = 0; i < n; i++) naive[i] = i;
	std::sort(naive.begin(), naive.end(), [&](uint32_t a, uint32_t b) { return std::lexicographical_compare(c.begin() + a, c.end(), c.begin() + b, c.end()); });
	if (sa != naive) { printf("FAIL %s: the suffix array differs from the naive sort (n = %u)\n", what, n); return false; }
	// the packed text gives back every letter
	std::vector<uint64_t> packed, invalid;
	gc::mxmPackText(c.data(), n, packed, invalid);
	const MxmIndexView v { sa.data(), packed.data(), invalid.data(), ix.text.nodeStart.data(), ix.text.nodeId.data(), nullptr, n, (uint32_t)ix.text.nodeId.size(), 0 };
	for (uint32_t p = 0; p < n; p++) if (mxmTextCode(v, p) != (c[p] ? c[p] - 1u : 4u)) { printf("FAIL %s: packed letter %u\n", what, p); return false; }
	uint32_t valid;
	(void)mxmTextWord(v, n, valid);
	if (valid != 0) { printf("FAIL %s: letters beyond the text\n", what); return false; }
	return true;
}

static int runSuffixArrays()
{
	std::mt19937 rng(12345);
	auto random = [&](size_t len) { std::string s(len, 'A'); for (auto& ch : s) ch = "ACGT"[rng() & 3]; return s; };
	bool ok = true;
	{
		std::vector<std::pair<int, std::string>> segs;   // 40 segments, 5 kb, with a few repeated pieces so that the doubling rounds have groups to refine
		const std::string repeat = random(90);
		for (int i = 0; i < 40; i++) { std::string s = random(80 + (rng() % 90)); if (i % 7 == 3) s = s.substr(0, 20) + repeat + s.substr(20, 15); segs.emplace_back(i + 1, s); }
		size_t total = 0;
		for (auto& s : segs) total += s.second.size();
		if (total < 4500 || total > 6500) { printf("FAIL random text of %zu letters\n", total); return 1; }
		ok &= checkSuffixArray("random", segs);
	}
	double polySeconds = 0;
	ok &= checkSuffixArray("homopolymer", { { 1, std::string(1000, 'A') } }, &polySeconds);
	{ std::string ac; for (int i = 0; i < 300; i++) ac += "AC"; ok &= checkSuffixArray("AC repeat", { { 1, ac } }); }
	ok &= checkSuffixArray("IUPAC", { { 1, "ACGTNNACGTRYACGTacgtuUACGT" }, { 2, "NACGTACGTN" }, { 5, "ACGTACGTACGTWACGTACGTACGT" } });
	ok &= checkSuffixArray("one letter", { { 1, "A" }, { 2, "C" }, { 3, "ACGT" } });
	ok &= checkSuffixArray("empty after mapping", { { 1, "NNNN" }, { 2, "ACGTACGT" }, { 3, "" }, { 4, "N" } });
	ok &= checkSuffixArray("no segment", {});
	// a comparison sort of the suffixes of 1000 equal letters compares 500 letters per step; prefix doubling does six rounds over 1000 suffixes. Well under a second even unoptimised.
	if (polySeconds > 0.5) { printf("FAIL homopolymer build took %.3f s\n", polySeconds); ok = false; }
	if (!ok) return 1;
	printf("OK homopolymer_seconds=%.6f\n", polySeconds);
	return 0;
}

static int runHits(const char* path)
{
	std::ifstream in(path);
	int mode; uint32_t minLen, prefixLen; long long count;
	std::string tag; size_t n;
	if (!(in >> mode >> minLen >> count >> prefixLen)) return 2;
	HostIndex ix;
	if (!(in >> tag >> n) || tag != "S") return 2;
	for (size_t k = 0; k < n; k++) { int id; std::string s; in >> id >> s; if (s == "*") s.clear(); gc::mxmAppendSegment(ix.text, id, s.data(), s.size()); }
	ix.build(prefixLen);
	if (!(in >> tag >> n) || tag != "R") return 2;
	for (size_t r = 0; r < n; r++) {
		std::string read;
		in >> read;
		if (read == "*") read.clear();
		std::vector<std::tuple<uint64_t, uint64_t, SeedHit>> found;   // (outer key, inner key, hit): the two stable sorts of the device in one
		for (uint32_t strand = 0; strand < 2; strand++) {
			const MxmQuery q { read.data(), (uint32_t)read.size(), strand };
			for (uint32_t i = 0; i < read.size(); i++) {
				uint32_t lo, hi;
				if (!mxmInterval(ix.view, q, i, minLen, lo, hi)) continue;
				for (uint32_t k = lo; k < hi; k++) {
					SeedHit hit; uint32_t tpos;
					if (mxmOccurrence(ix.view, q, mode, minLen, i, lo, hi, k, hit, tpos)) found.emplace_back(mxmOrderKeyOuter(0, hit.matchLen), mxmOrderKeyInner(strand, i, tpos), hit);
				}
			}
		}
		std::sort(found.begin(), found.end(), [](const auto& a, const auto& b) { return std::get<0>(a) != std::get<0>(b) ? std::get<0>(a) < std::get<0>(b) : std::get<1>(a) < std::get<1>(b); });
		if (count >= 0 && found.size() > (size_t)count) found.resize((size_t)count);
		printf("R %zu %zu\n", r, found.size());
		for (const auto& f : found) { const SeedHit& h = std::get<2>(f); printf("%d %u %u %u %u %u\n", h.nodeId, h.nodeOffset, h.seqPos, h.matchLen, h.rawGoodness, h.reverse); }
	}
	return 0;
}

int main(int argc, char** argv)
{
	if (argc >= 2 && std::string(argv[1]) == "sa") return runSuffixArrays();
	if (argc >= 3 && std::string(argv[1]) == "hits") return runHits(argv[2]);
	fprintf(stderr, "usage: mxm_host_test sa | hits <case file>\n");
	return 2;
}
