// CPU program for tests/test_mxm_cache_host.py: the MUM / MEM index's cache file (csrc/host/gc_mxm_cache.hpp) written, read back and damaged, on texts built by csrc/host/gc_mxm_build.hpp.
//   mxm_cache_host_test run <dir>        every check below in <dir> (an empty directory); prints OK or the first failure
//   mxm_cache_host_test write <prefix>   writes <prefix>.gcmxm for the random text and prints "<letters> <segments> <file bytes> <fingerprint>" for gc_mxm_cache_check to be held to
#include "gc_mxm_build.hpp"
#include "gc_mxm_cache.hpp"
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <fstream>
#include <functional>
#include <iterator>
#include <random>
#include <string>
#include <vector>

static void serialFor(size_t n, const std::function<void(size_t)>& body) { for (size_t i = 0; i < n; i++) body(i); }

struct Built {
	gc::MxmText text;
	std::vector<uint32_t> sa;
	std::vector<uint64_t> packed, invalid;
	uint64_t fingerprint = 0;
	uint32_t n() const { return (uint32_t)text.codes.size(); }
	explicit Built(const std::vector<std::pair<int, std::string>>& segments)
	{
		for (const auto& s : segments) gc::mxmAppendSegment(text, s.first, s.second.data(), s.second.size());
		gc::mxmFinishText(text);
		sa = gc::mxmSuffixArray(text.codes.data(), n(), serialFor);
		gc::mxmPackText(text.codes.data(), n(), packed, invalid);
		fingerprint = gc::mxmTextFingerprint(text.codes.data(), n());
	}
	void save(const std::string& path) const { gc::mxmCacheSave(path, text.nodeStart, text.nodeId, packed, invalid, sa.data(), n(), fingerprint); }
};

static std::vector<std::pair<int, std::string>> randomSegments()
{
	std::mt19937 rng(4711);
	auto random = [&](size_t len) { std::string s(len, 'A'); for (auto& ch : s) ch = "ACGT"[rng() & 3]; return s; };
	std::vector<std::pair<int, std::string>> segs;   // 40 segments, about 5 kb, a few with a shared piece and one with letters outside a c g t
	const std::string repeat = random(90);
	for (int i = 0; i < 40; i++) { std::string s = random(80 + (rng() % 90)); if (i % 7 == 3) s = s.substr(0, 20) + repeat + s.substr(20, 15); if (i == 11) s[30] = 'N'; segs.emplace_back(2 * i + 1, s); }
	return segs;
}

static std::vector<uint8_t> readBytes(const std::string& path)
{
	std::ifstream in(path, std::ios::binary);
	return std::vector<uint8_t>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}
static void writeBytes(const std::string& path, const std::vector<uint8_t>& b)
{
	std::ofstream out(path, std::ios::binary | std::ios::trunc);
	out.write((const char*)b.data(), (std::streamsize)b.size());
}

static bool fails(const char* what, bool ok) { if (!ok) printf("FAIL %s\n", what); return !ok; }

// a load of `bytes` written to `path` must be refused with `needle` and the path in the message, and must leave the file as it was
static bool refused(const std::string& path, const std::vector<uint8_t>& bytes, const char* needle, const char* what, const uint64_t* expect = nullptr)
{
	writeBytes(path, bytes);
	bool thrown = false;
	try {
		gc::MxmCacheFile f;
		gc::mxmCacheLoad(path, f, expect);
	} catch (const gc::MxmCacheError& e) {
		const std::string msg = e.what();
		thrown = msg.find(needle) != std::string::npos && msg.find(path) != std::string::npos;
		if (!thrown) printf("FAIL %s: refused with \"%s\", expected \"%s\" and the file's name\n", what, msg.c_str(), needle);
	}
	if (!thrown) { printf("FAIL %s: not refused as expected\n", what); return false; }
	if (readBytes(path) != bytes) { printf("FAIL %s: the refused file was changed\n", what); return false; }
	return true;
}

static bool roundTrip(const std::string& dir, const char* name, const Built& b)
{
	const std::string path = gc::mxmCachePath(dir + "/" + name);
	b.save(path);
	size_t entries = 0;
	for (const auto& e : std::filesystem::directory_iterator(dir)) { entries++; if (e.path().extension() != ".gcmxm") { printf("FAIL %s: %s left behind by the save\n", name, e.path().c_str()); return false; } }
	if (fails(name, entries >= 1 && gc::mxmCacheExists(path))) return false;
	gc::MxmCacheFile f;
	gc::mxmCacheLoad(path, f, &b.fingerprint);
	const uint32_t n = b.n();
	const size_t segs = b.text.nodeId.size();
	bool same = f.info.version == gc::MXM_CACHE_VERSION && f.info.n == n && f.info.segments == segs && f.info.fingerprint == b.fingerprint && f.info.fileBytes == std::filesystem::file_size(path)
		&& std::vector<uint32_t>(f.nodeStart, f.nodeStart + segs + 1) == b.text.nodeStart && std::vector<int32_t>(f.nodeId, f.nodeId + segs) == b.text.nodeId
		&& std::vector<uint64_t>(f.packed, f.packed + f.packedWords) == b.packed && std::vector<uint64_t>(f.invalid, f.invalid + f.invalidWords) == b.invalid
		&& std::vector<uint32_t>(f.sa, f.sa + n) == b.sa && gc::mxmCacheTextFingerprint(f) == b.fingerprint;
	if (!same) { printf("FAIL %s: the file read back differs from what was written\n", name); return false; }
	// saving again over an existing file gives the same bytes (the format has no time stamp), again without a temporary left
	const std::vector<uint8_t> first = readBytes(path);
	b.save(path);
	return !fails(name, readBytes(path) == first && f.info.fileBytes == first.size());
}

static int run(const std::string& dir)
{
	const Built random(randomSegments());
	if (fails("random text size", random.n() > 4500 && random.n() < 6500)) return 1;
	const Built empty({}), one({ { 7, "G" } }), twins({ { 1, "ACGTTGCAACGGT" }, { 2, "ACGTTGCAACGGT" } }), other({ { 1, "ACGTTGCAACGGA" }, { 2, "ACGTTGCAACGGT" } });
	if (fails("empty text", empty.n() == 0 && empty.sa.empty()) || fails("one letter", one.n() == 2) || fails("twins", twins.n() == other.n() && twins.fingerprint != other.fingerprint)) return 1;
	if (!roundTrip(dir, "random", random) || !roundTrip(dir, "empty", empty) || !roundTrip(dir, "one", one) || !roundTrip(dir, "twins", twins)) return 1;

	const std::string path = gc::mxmCachePath(dir + "/random");
	const std::vector<uint8_t> good = readBytes(path);
	const std::string victim = gc::mxmCachePath(dir + "/victim");
	const size_t saBytes = (size_t)random.n() * 4 + (random.n() & 1 ? 4 : 0), saBegin = good.size() - 8 - saBytes;
	auto flipped = [&](size_t at) { std::vector<uint8_t> b = good; b[at] ^= 0x10; return b; };
	auto cut = [&](size_t keep) { return std::vector<uint8_t>(good.begin(), good.begin() + keep); };
	bool ok = true;
	ok &= refused(victim, flipped(2), "magic", "flipped byte in the magic");
	ok &= refused(victim, flipped(17), "bytes, the header describes", "flipped byte in the header's letter count");
	ok &= refused(victim, flipped(33), "checksum", "flipped byte in the header's fingerprint");
	ok &= refused(victim, flipped(saBegin + saBytes / 2), "checksum", "flipped byte in the suffix array");
	ok &= refused(victim, flipped(good.size() - 3), "checksum", "flipped byte in the checksum");
	ok &= refused(victim, cut(20), "truncated", "truncated inside the header");
	ok &= refused(victim, cut(saBegin + 100), "truncated", "truncated inside the suffix array");
	ok &= refused(victim, cut(good.size() - 1), "truncated", "truncated by one byte");
	ok &= refused(victim, cut(0), "truncated", "an empty file");
	auto resealed = [&](std::vector<uint8_t> b) { const uint64_t h = gc::mxmFnv(gc::MXM_FNV_SEED, b.data(), b.size() - 8); memcpy(b.data() + b.size() - 8, &h, 8); return b; };
	{ std::vector<uint8_t> b = good; b[8] = (uint8_t)(gc::MXM_CACHE_VERSION + 1); ok &= refused(victim, resealed(b), "version", "another version, checksum valid"); }
	{ std::vector<uint8_t> b = good; const uint32_t beyond = random.n(); memcpy(b.data() + saBegin + 40, &beyond, 4); ok &= refused(victim, resealed(b), "suffix array entry beyond the text", "suffix array entry beyond the text, checksum valid"); }
	{ std::vector<uint8_t> b = good; b[40] = 1; ok &= refused(victim, resealed(b), "segment table", "segment table that does not start at 0, checksum valid"); }
	ok &= refused(victim, good, "fingerprint", "the cache of another text", &other.fingerprint);
	ok &= refused(gc::mxmCachePath(dir + "/twins"), readBytes(gc::mxmCachePath(dir + "/twins")), "fingerprint", "twins' cache against a text of the same length", &other.fingerprint);
	// and the undamaged bytes still load, with and without a text to compare with
	writeBytes(victim, good);
	try { gc::MxmCacheFile f; gc::mxmCacheLoad(victim, f); gc::mxmCacheLoad(victim, f, &random.fingerprint); } catch (const std::exception& e) { printf("FAIL the good file is refused: %s\n", e.what()); ok = false; }
	bool missing = false;
	try { gc::MxmCacheFile f; gc::mxmCacheLoad(gc::mxmCachePath(dir + "/nothing"), f); } catch (const gc::MxmCacheError&) { missing = true; }
	ok &= !fails("a missing file is refused", missing);
	// the device build's limit (hipCUB counts in int): the last text it takes has 2^31 - 2 letters
	ok &= !fails("device build limit", gc::mxmDeviceBuildTakes(0) && gc::mxmDeviceBuildTakes(0x7ffffffeull) && !gc::mxmDeviceBuildTakes(0x7fffffffull) && !gc::mxmDeviceBuildTakes(0xffffffefull));
	if (!ok) return 1;
	printf("OK\n");
	return 0;
}

int main(int argc, char** argv)
{
	try {
		if (argc >= 3 && std::string(argv[1]) == "run") return run(argv[2]);
		if (argc >= 3 && std::string(argv[1]) == "write") {
			const Built random(randomSegments());
			const std::string path = gc::mxmCachePath(argv[2]);
			random.save(path);
			printf("%u %zu %llu %llu\n", random.n(), random.text.nodeId.size(), (unsigned long long)std::filesystem::file_size(path), (unsigned long long)random.fingerprint);
			return 0;
		}
	} catch (const std::exception& e) {
		printf("FAIL exception: %s\n", e.what());
		return 1;
	}
	fprintf(stderr, "usage: mxm_cache_host_test run <dir> | write <prefix>\n");
	return 2;
}
