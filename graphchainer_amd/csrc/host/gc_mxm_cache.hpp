// The MUM / MEM index on disk (gc_mxm_index_open with a cache prefix; the reference's --seeds-mxm-cache-prefix, src/MummerSeeder.cpp:65-89,137-161): writer, reader and verifier.
// Standard library only, like gc_mxm_build.hpp, so that a CPU program can drive it (tests/mxm_cache_host).
// The reference writes <prefix>.aux (a boost text archive) and mummer's own <prefix>_index files; neither can be produced without those libraries, so this is ONE file of our
// own, <prefix>.gcmxm, in a private format. Little-endian, every section at a multiple of 8 bytes:
//   header   magic u64 | version u32 | 0 u32 | n (text letters, separators included) u64 | segments u64 | FNV-1a-64 of the text's codes (0 separator, 1..4 = a c g t) u64
//   tables   nodeStart u32 [segments + 1] | nodeId i32 [segments] | 4 bytes of zero
//   text     packed u64 [(n >> 5) + 2] | not-a-letter mask u64 [(n >> 6) + 2]        (mxmPackText: what the kernels read, uploaded as it lies in the file)
//   sa       u32 [n], raw - 4 bytes per letter, so that a load is a read | 4 bytes of zero when n is odd
//   check    FNV-1a-64 of every byte before it u64
// The prefix table is not stored: the device rebuilds it from the suffix array. A load verifies magic, version, the sizes against the file's length, the checksum, the tables
// (ascending, ending at n), every suffix-array entry (< n) and, when the caller has the text, its fingerprint; whatever fails is an MxmCacheError that names the file and the
// failure, and the file is neither used nor touched. A save goes to a temporary name beside the target and is renamed, so a killed process leaves no half-written cache.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include <unistd.h>

namespace gc {

inline constexpr uint64_t MXM_CACHE_MAGIC = 0x0a4d584d43470089ull;   // the file's first eight bytes: 0x89, 0, "GCMXM", a line feed
inline constexpr uint32_t MXM_CACHE_VERSION = 1;
inline constexpr uint64_t MXM_FNV_SEED = 0xcbf29ce484222325ull;

struct MxmCacheError : std::runtime_error { using std::runtime_error::runtime_error; };

inline uint64_t mxmFnv(uint64_t h, const void* data, size_t n)
{
	const uint8_t* p = (const uint8_t*)data;
	for (size_t i = 0; i < n; i++) { h ^= p[i]; h *= 0x100000001b3ull; }
	return h;
}
inline uint64_t mxmTextFingerprint(const uint8_t* codes, size_t n) { return mxmFnv(MXM_FNV_SEED, codes, n); }
inline std::string mxmCachePath(const std::string& prefix) { return prefix + ".gcmxm"; }
inline bool mxmCacheExists(const std::string& path) { return access(path.c_str(), F_OK) == 0; }

struct MxmCacheInfo { uint64_t version = 0, n = 0, segments = 0, fileBytes = 0, fingerprint = 0; };

// a loaded file: the sections are read where they lie in `raw`
struct MxmCacheFile {
	std::vector<uint64_t> raw;
	MxmCacheInfo info;
	const uint32_t* nodeStart = nullptr;   // [segments + 1]
	const int32_t* nodeId = nullptr;       // [segments]
	const uint64_t* packed = nullptr;      // [packedWords]
	const uint64_t* invalid = nullptr;     // [invalidWords]
	const uint32_t* sa = nullptr;          // [n]
	size_t packedWords = 0, invalidWords = 0;
};

namespace mxmcache {
inline constexpr size_t HEADER_BYTES = 40;
inline size_t tableBytes(uint64_t segments) { return (size_t)(2 * segments + 1) * 4 + 4; }
inline size_t packedWords(uint64_t n) { return (size_t)(n >> 5) + 2; }
inline size_t invalidWords(uint64_t n) { return (size_t)(n >> 6) + 2; }
inline size_t saBytes(uint64_t n) { return ((size_t)n * 4 + 7) & ~(size_t)7; }
}

// packed / invalid as mxmPackText leaves them for a text of n letters; sa [n]
inline void mxmCacheSave(const std::string& path, const std::vector<uint32_t>& nodeStart, const std::vector<int32_t>& nodeId, const std::vector<uint64_t>& packed, const std::vector<uint64_t>& invalid,
	const uint32_t* sa, uint64_t n, uint64_t fingerprint)
{
	const uint64_t segments = nodeId.size();
	if (nodeStart.size() != segments + 1 || packed.size() != mxmcache::packedWords(n) || invalid.size() != mxmcache::invalidWords(n)) throw std::logic_error("mxmCacheSave: the arrays do not belong to a text of n letters");
	const std::string tmp = path + ".tmp" + std::to_string((long)getpid());
	FILE* f = fopen(tmp.c_str(), "wb");
	if (!f) throw MxmCacheError("cannot create " + tmp);
	uint64_t hash = MXM_FNV_SEED;
	bool ok = true;
	auto put = [&](const void* p, size_t bytes) { if (!bytes || !ok) return; hash = mxmFnv(hash, p, bytes); ok = fwrite(p, 1, bytes, f) == bytes; };
	const uint32_t version = MXM_CACHE_VERSION, zero = 0;
	put(&MXM_CACHE_MAGIC, 8); put(&version, 4); put(&zero, 4); put(&n, 8); put(&segments, 8); put(&fingerprint, 8);
	put(nodeStart.data(), nodeStart.size() * 4); put(nodeId.data(), nodeId.size() * 4); put(&zero, 4);
	put(packed.data(), packed.size() * 8); put(invalid.data(), invalid.size() * 8);
	put(sa, (size_t)n * 4);
	if (n & 1) put(&zero, 4);
	const uint64_t check = hash;
	put(&check, 8);
	ok = (fclose(f) == 0) && ok;
	if (!ok) { remove(tmp.c_str()); throw MxmCacheError("short write to " + tmp); }
	if (rename(tmp.c_str(), path.c_str()) != 0) { remove(tmp.c_str()); throw MxmCacheError("cannot move the MUM / MEM index cache to " + path); }
}

// expectFingerprint: the fingerprint of the text the caller holds (nullptr: none to compare with)
inline void mxmCacheLoad(const std::string& path, MxmCacheFile& out, const uint64_t* expectFingerprint = nullptr)
{
	auto refuse = [&](const std::string& what) -> void { throw MxmCacheError("MUM / MEM index cache " + path + ": " + what); };
	FILE* f = fopen(path.c_str(), "rb");
	if (!f) refuse("cannot be opened");
	struct Close { FILE* f; ~Close() { fclose(f); } } closer { f };
	if (fseek(f, 0, SEEK_END) != 0) refuse("cannot be read");
	const long long size = ftell(f);
	if (size < 0 || fseek(f, 0, SEEK_SET) != 0) refuse("cannot be read");
	const size_t bytes = (size_t)size;
	if (bytes < mxmcache::HEADER_BYTES + 8) refuse("truncated (" + std::to_string(bytes) + " bytes hold no header)");
	uint8_t head[mxmcache::HEADER_BYTES];
	if (fread(head, 1, sizeof(head), f) != sizeof(head)) refuse("cannot be read");
	uint64_t magic, n, segments, fingerprint;
	uint32_t version, reserved;
	memcpy(&magic, head, 8); memcpy(&version, head + 8, 4); memcpy(&reserved, head + 12, 4); memcpy(&n, head + 16, 8); memcpy(&segments, head + 24, 8); memcpy(&fingerprint, head + 32, 8);
	if (magic != MXM_CACHE_MAGIC) refuse("not a MUM / MEM index cache (magic)");
	if (version != MXM_CACHE_VERSION) refuse("version " + std::to_string(version) + ", this library reads version " + std::to_string(MXM_CACHE_VERSION));
	if (reserved != 0) refuse("damaged header");
	// bounds before anything is sized by the header: 32-bit positions, every segment holds at least its separator
	if (n >= 0xfffffff0ull || segments > n) refuse("damaged header (" + std::to_string(n) + " letters, " + std::to_string(segments) + " segments)");
	const size_t oTables = mxmcache::HEADER_BYTES, oPacked = oTables + mxmcache::tableBytes(segments), oInvalid = oPacked + mxmcache::packedWords(n) * 8, oSa = oInvalid + mxmcache::invalidWords(n) * 8,
		oCheck = oSa + mxmcache::saBytes(n);
	if (bytes != oCheck + 8) refuse(std::string(bytes < oCheck + 8 ? "truncated" : "too long") + " (" + std::to_string(bytes) + " bytes, the header describes " + std::to_string(oCheck + 8) + ")");
	out.raw.assign(bytes / 8, 0);
	memcpy(out.raw.data(), head, sizeof(head));
	if (fread((uint8_t*)out.raw.data() + sizeof(head), 1, bytes - sizeof(head), f) != bytes - sizeof(head)) refuse("cannot be read");
	const uint8_t* base = (const uint8_t*)out.raw.data();
	uint64_t stored;
	memcpy(&stored, base + oCheck, 8);
	if (mxmFnv(MXM_FNV_SEED, base, oCheck) != stored) refuse("checksum mismatch (damaged file)");
	out.nodeStart = (const uint32_t*)(base + oTables);
	out.nodeId = (const int32_t*)(out.nodeStart + segments + 1);
	out.packed = (const uint64_t*)(base + oPacked);
	out.invalid = (const uint64_t*)(base + oInvalid);
	out.sa = (const uint32_t*)(base + oSa);
	out.packedWords = mxmcache::packedWords(n);
	out.invalidWords = mxmcache::invalidWords(n);
	if (out.nodeStart[segments] != n || (segments && out.nodeStart[0] != 0)) refuse("segment table does not span the text");
	for (uint64_t k = 0; k < segments; k++) if (out.nodeStart[k + 1] <= out.nodeStart[k]) refuse("segment table does not ascend");
	uint32_t worst = 0;
	for (uint64_t i = 0; i < n; i++) worst = out.sa[i] > worst ? out.sa[i] : worst;
	if (n && worst >= n) refuse("suffix array entry beyond the text");
	if (expectFingerprint && *expectFingerprint != fingerprint) refuse("text fingerprint mismatch (the cache was built from another graph)");
	out.info.version = version; out.info.n = n; out.info.segments = segments; out.info.fileBytes = bytes; out.info.fingerprint = fingerprint;
}

// the fingerprint of the text a loaded file holds, from its packed words and mask (what gc_mxm_cache_check compares with the stored one)
inline uint64_t mxmCacheTextFingerprint(const MxmCacheFile& file)
{
	uint64_t h = MXM_FNV_SEED;
	uint8_t chunk[4096];
	for (uint64_t a = 0; a < file.info.n; a += sizeof(chunk)) {
		const uint64_t b = file.info.n - a < sizeof(chunk) ? file.info.n - a : sizeof(chunk);
		for (uint64_t k = 0; k < b; k++) {
			const uint64_t i = a + k;
			const bool letter = !((file.invalid[i >> 6] >> (63 - (i & 63))) & 1);
			chunk[k] = letter ? (uint8_t)(((file.packed[i >> 5] >> (62 - 2 * (i & 31))) & 3) + 1) : 0;
		}
		h = mxmFnv(h, chunk, (size_t)b);
	}
	return h;
}

} // namespace gc
