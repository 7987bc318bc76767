// C entry points, seed hits from outside the minimizer seeder: gc_seeds_upload / _destroy / _hits / _kernel_ms, the MUM / MEM seeder (gc_mxm_options_default, gc_mxm_index_create /
// _open / _destroy / _array, gc_mxm_cache_check, gc_seeds_mxm) and GAM seed files (gc_seed_store_open / _from_memory / _info / _destroy, gc_seeds_from_store). Every batch is laid
// out by host/gc_layout.hpp's SeedBatchLayout (allocateSeedBlock, gc_runtime.hpp).
#include "../gc_runtime.hpp"
#include "../hip/gc_seedhits_core.hpp"
#include "../host/gc_seedfile_frame.hpp"
#include <zlib.h>

extern "C" {

// ---- seed hits from the host's own seeder -------------------------------------------------------------------
int gc_seeds_upload(const gc_graph* G, const gc_reads* R, const gc_seed_hit* hits, const uint64_t* read_hit_off, uint64_t n_reads, gc_seeds** out)
{
	static_assert(sizeof(gc_seed_hit) == sizeof(SeedHit) && sizeof(SeedHit) == 24 && gc::SEED_HIT_BYTES == 24, "gc_seed_hit is what k_seed_resolve reads");
	// host checks first: a malformed call is GC_ERR_INVALID whether or not a device is present
	if (!G || !R || !read_hit_off || !out) return fail(GC_ERR_INVALID, "null argument");
	*out = nullptr;
	if (n_reads != R->offsets.size() - 1) return fail(GC_ERR_INVALID, "gc_seeds_upload: n_reads differs from the read batch's");
	if (read_hit_off[0] != 0) return fail(GC_ERR_INVALID, "gc_seeds_upload: read_hit_off must start at 0");
	for (uint64_t r = 0; r < n_reads; r++) if (read_hit_off[r + 1] < read_hit_off[r]) return fail(GC_ERR_INVALID, "gc_seeds_upload: read_hit_off decreases at read " + std::to_string(r));
	const uint64_t nHits = read_hit_off[n_reads];
	if (nHits >= 0xfffffff0ull) return fail(GC_ERR_INVALID, "gc_seeds_upload: 2^32 hits or more; split the batch");
	if (nHits && !hits) return fail(GC_ERR_INVALID, "null argument");
	for (uint64_t r = 0; r < n_reads; r++) {
		// the seed goodness is a 32-bit word: a cluster's matching base pairs are at most its first seed's match_len plus the read positions it spans, and any hit of the cluster
		// adds its own raw goodness to them (src/GraphAligner.h:273-287)
		const uint64_t len = R->offsets[r + 1] - R->offsets[r];
		uint64_t longest = 0, best = 0, bestAt = 0;
		for (uint64_t i = read_hit_off[r]; i < read_hit_off[r + 1]; i++) {
			if (hits[i].match_len > 0x7fffffffu) return fail(GC_ERR_INVALID, "gc_seeds_upload: read " + std::to_string(r) + " hit " + std::to_string(i - read_hit_off[r]) + ": match_len of 2^31 or more");
			longest = std::max<uint64_t>(longest, hits[i].match_len);
			if (hits[i].raw_goodness >= best) { best = hits[i].raw_goodness; bestAt = i; }
		}
		if (longest + len + best > 0xffffffffull)
			return fail(GC_ERR_INVALID, "gc_seeds_upload: read " + std::to_string(r) + " hit " + std::to_string(bestAt - read_hit_off[r]) + ": raw_goodness too large for the 32-bit seed goodness (match_len + read length + raw_goodness must stay below 2^32)");
	}
	gc_seeds* H = new gc_seeds();
	int rc = guarded([&]() {
		requireDevice();
		HIP_CHECK(hipGetDevice(&H->device));
		H->nHits = nHits;
		H->readOffsets = R->offsets;
		std::vector<uint32_t> off32(n_reads + 1);
		for (uint64_t r = 0; r <= n_reads; r++) off32[r] = (uint32_t)read_hit_off[r];
		unsigned long long* dBad = allocateSeedBlock(*H, n_reads);
		SeedHit* dHits = H->devHits;
		hipStream_t q = threadStream(H->device);
		unsigned long long bad = ~0ull;
		HIP_CHECK(hipMemcpyAsync(H->devReadHitOff, off32.data(), (n_reads + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, q));
		HIP_CHECK(hipMemcpyAsync(dBad, &bad, sizeof(bad), hipMemcpyHostToDevice, q));
		if (nHits) HIP_CHECK(hipMemcpyAsync(dHits, hits, nHits * sizeof(SeedHit), hipMemcpyHostToDevice, q));
		const SeedLookup lookup { G->dev.origSize, G->dev.lookupOff, G->dev.lookup, G->dev.nodeOffset, (uint32_t)G->hOrigSize.size() };
		launchSeedResolve(q, lookup, dHits, nHits, H->devReadHitOff, (uint32_t)n_reads, R->devOffsets, H->dev, dBad);
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipMemcpyAsync(&bad, dBad, sizeof(bad), hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipStreamSynchronize(q));
		if (bad != ~0ull) {
			const uint64_t i = bad >> 2;
			const uint64_t r = (uint64_t)(std::upper_bound(read_hit_off, read_hit_off + n_reads + 1, i) - read_hit_off) - 1;
			const char* what[] = { "", "no such node in the graph", "node_offset is not inside the original node", "seq_pos is not inside the read" };
			return fail(GC_ERR_INVALID, "gc_seeds_upload: read " + std::to_string(r) + " hit " + std::to_string(i - read_hit_off[r]) + ": " + what[bad & 3]);
		}
		return (int)GC_OK;
	});
	if (rc != GC_OK) { delete H; return rc; }
	*out = H;
	return GC_OK;
}
void gc_seeds_destroy(gc_seeds* s) { delete s; }

int gc_seeds_hits(const gc_seeds* s, gc_seed_hit** hits, uint64_t** read_hit_off, uint64_t* n_reads)
{
	if (!s || !hits || !read_hit_off || !n_reads) return fail(GC_ERR_INVALID, "null argument");
	*hits = nullptr; *read_hit_off = nullptr;
	const uint64_t n = s->readOffsets.size() - 1;
	std::vector<uint32_t> off32(n + 1);
	gc_seed_hit* h = mallocArray<gc_seed_hit>(s->nHits);
	uint64_t* off = mallocArray<uint64_t>(n + 1);
	int rc = guarded([&]() {
		requireDevice();
		HIP_CHECK(hipMemcpy(off32.data(), s->devReadHitOff, (n + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
		if (s->nHits) HIP_CHECK(hipMemcpy(h, s->devHits, s->nHits * sizeof(gc_seed_hit), hipMemcpyDeviceToHost));
		return (int)GC_OK;
	});
	if (rc != GC_OK) { free(h); free(off); return rc; }
	for (uint64_t r = 0; r <= n; r++) off[r] = off32[r];
	*hits = h; *read_hit_off = off; *n_reads = n;
	return GC_OK;
}
double gc_seeds_kernel_ms(const gc_seeds* s) { return s ? s->kernelMs : 0; }

// ---- the MUM / MEM seeder (the reference's MummerSeeder, src/MummerSeeder.cpp) ---------------
// what gc_mxm_index_create and gc_mxm_index_open share. `who`: the entry point's name for the messages; cachePrefix empty: no cache
static int mxmIndexOpen(const char* who, const gc_graph* G, int32_t build, const std::string& cachePrefix, gc_mxm_index** out)
{
	// the forward original segments, from what the graph holds: bigraph id 2 * nodeID, its split nodes in offset order (64-letter chunks)
	const size_t nB = G->hOrigSize.size();
	uint64_t letters = 0;
	std::vector<uint32_t> ids;
	for (size_t id = 0; id < nB; id += 2) if (G->hLookupOff[id + 1] > G->hLookupOff[id]) { ids.push_back((uint32_t)id); letters += (uint64_t)G->hOrigSize[id] + 1; }
	if (letters >= 0xfffffff0ull) return fail(GC_ERR_INVALID, std::string(who) + ": a text of 2^32 - 16 letters or more (the segments and one separator each) does not fit the index's 32-bit positions");
	const std::string cachePath = cachePrefix.empty() ? std::string() : gc::mxmCachePath(cachePrefix);
	const bool load = !cachePath.empty() && gc::mxmCacheExists(cachePath);
	// (a host check, before a device is needed; nothing falls back to the host build by itself)
	if (!load && build == GC_MXM_BUILD_DEVICE && !gc::mxmDeviceBuildTakes(letters))
		return fail(GC_ERR_INVALID, std::string(who) + ": the device build takes a text of fewer than 2^31 - 1 letters (hipCUB counts in int) and this one has " + std::to_string(letters) + "; build it on the host (GC_MXM_BUILD_HOST)");
	gc_mxm_index* X = new gc_mxm_index();
	int rc = guarded([&]() {
		try {
		requireDevice();
		HIP_CHECK(hipGetDevice(&X->device));
		X->graph = G;
		const auto t0 = std::chrono::steady_clock::now();
		const uint32_t n = (uint32_t)letters;
		std::vector<uint8_t> codes(n, 0);
		X->nodeStart.resize(ids.size() + 1);
		X->nodeId.resize(ids.size());
		uint32_t at = 0;
		for (size_t k = 0; k < ids.size(); k++) { X->nodeStart[k] = at; X->nodeId[k] = (int32_t)(ids[k] / 2); at += G->hOrigSize[ids[k]] + 1; }
		X->nodeStart[ids.size()] = n;
		const gc::AlignmentGraph& g = G->host;
		WorkerPool::instance().run(ids.size(), [&](size_t k, size_t) {
			uint8_t* dst = codes.data() + X->nodeStart[k];
			for (uint32_t e = G->hLookupOff[ids[k]]; e < G->hLookupOff[ids[k] + 1]; e++) {
				const uint32_t node = G->hLookup[e];
				const size_t len = g.nodeLength[node], off = g.nodeOffset[node];
				for (size_t j = 0; j < len; j++) dst[off + j] = gc::mxmRefCode(g.NodeSequences(node, j));
			}
		});
		const uint64_t fingerprint = cachePath.empty() ? 0 : gc::mxmTextFingerprint(codes.data(), n);
		hipStream_t q = threadStream(X->device);
		MxmIndexView& d = X->dev;
		d.n = n; d.nNodes = (uint32_t)ids.size(); d.prefixLen = gc::MXM_PREFIX_LEN;
		auto upRaw = [&](const auto* src, size_t count) {
			std::remove_const_t<std::remove_pointer_t<decltype(src)>>* p = nullptr;
			const size_t bytes = std::max<size_t>(count, 1) * sizeof(*src);
			HIP_CHECK(hipMalloc((void**)&p, bytes));
			X->allocations.push_back((void*)p);
			X->deviceBytes += bytes;
			if (count) HIP_CHECK(hipMemcpy(p, src, count * sizeof(*src), hipMemcpyHostToDevice));
			return p;
		};
		auto up = [&](const auto& v) { return upRaw(v.data(), v.size()); };
		if (load) {
			gc::MxmCacheFile file;
			gc::mxmCacheLoad(cachePath, file, &fingerprint);
			// (the fingerprint covers every letter and separator, so the segment starts agree; the node ids are compared on their own)
			if (file.info.n != n || file.info.segments != ids.size() || memcmp(file.nodeStart, X->nodeStart.data(), (ids.size() + 1) * 4) != 0 || memcmp(file.nodeId, X->nodeId.data(), ids.size() * 4) != 0)
				throw gc::MxmCacheError("MUM / MEM index cache " + cachePath + ": segment table mismatch (the cache was built from another graph)");
			X->buildSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
			X->buildMode = 2;
			d.sa = upRaw(file.sa, n); d.packed = upRaw(file.packed, file.packedWords); d.invalid = upRaw(file.invalid, file.invalidWords);
		} else {
			std::vector<uint32_t> sa;
			std::vector<uint64_t> packed, invalid;
			const auto tSa = std::chrono::steady_clock::now();
			if (build == GC_MXM_BUILD_DEVICE) {
				uint32_t* dSa = nullptr;
				HIP_CHECK(hipMalloc((void**)&dSa, std::max<size_t>(n, 1) * sizeof(uint32_t)));
				X->allocations.push_back(dSa);
				X->deviceBytes += std::max<size_t>(n, 1) * sizeof(uint32_t);
				MxmSaBuild info;
				HIP_CHECK(launchMxmSuffixArray(q, codes.data(), n, dSa, info));
				X->saSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - tSa).count();
				gc::mxmPackText(codes.data(), n, packed, invalid);
				X->buildRounds = info.rounds; X->buildScratchBytes = info.scratchBytes; X->buildMode = 1;
				d.sa = dSa;
			} else {
				auto parallelFor = [](size_t count, const std::function<void(size_t)>& body) { WorkerPool::instance().run(count, [&](size_t i, size_t) { body(i); }); };
				sa = gc::mxmSuffixArray(codes.data(), n, parallelFor, &X->buildRounds);
				X->saSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - tSa).count();
				gc::mxmPackText(codes.data(), n, packed, invalid);
			}
			X->buildSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
			if (build != GC_MXM_BUILD_DEVICE) d.sa = up(sa);
			d.packed = up(packed); d.invalid = up(invalid);
			if (!cachePath.empty()) {
				const auto t1 = std::chrono::steady_clock::now();
				if (build == GC_MXM_BUILD_DEVICE) { sa.resize(n); if (n) HIP_CHECK(hipMemcpy(sa.data(), d.sa, (size_t)n * 4, hipMemcpyDeviceToHost)); }
				gc::mxmCacheSave(cachePath, X->nodeStart, X->nodeId, packed, invalid, sa.data(), n, fingerprint);
				X->cacheSaveSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
			}
		}
		d.nodeStart = up(X->nodeStart); d.nodeId = up(X->nodeId);
		uint32_t* table = nullptr;
		const size_t tableBytes = ((size_t)2 << (2 * d.prefixLen)) * sizeof(uint32_t);
		HIP_CHECK(hipMalloc((void**)&table, tableBytes));
		X->allocations.push_back(table);
		X->deviceBytes += tableBytes;
		d.prefix = table;
		HIP_CHECK(hipMemsetAsync(table, 0, tableBytes, q));
		launchMxmPrefixTable(q, d, table);
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipStreamSynchronize(q));
		return (int)GC_OK;
		} catch (const gc::MxmCacheError& e) {
			return fail(GC_ERR_GRAPH, e.what());   // (a cache that cannot be used or written: never used half, never overwritten)
		}
	});
	if (rc != GC_OK) { delete X; return rc; }
	*out = X;
	return GC_OK;
}

int gc_mxm_index_create(const gc_graph* G, gc_mxm_index** out)
{
	if (!G || !out) return fail(GC_ERR_INVALID, "null argument");
	*out = nullptr;
	return mxmIndexOpen("gc_mxm_index_create", G, GC_MXM_BUILD_HOST, std::string(), out);
}

void gc_mxm_options_default(gc_mxm_options* o)
{
	if (!o) return;
	o->build = GC_MXM_BUILD_HOST; o->reserved = 0; o->cache_prefix = nullptr;
}

int gc_mxm_index_open(const gc_graph* G, const gc_mxm_options* o, gc_mxm_index** out)
{
	// host checks first: a malformed call is GC_ERR_INVALID whether or not a device is present
	if (!G || !o || !out) return fail(GC_ERR_INVALID, "null argument");
	*out = nullptr;
	if (o->build != GC_MXM_BUILD_HOST && o->build != GC_MXM_BUILD_DEVICE) return fail(GC_ERR_INVALID, "gc_mxm_index_open: build is neither GC_MXM_BUILD_HOST nor GC_MXM_BUILD_DEVICE");
	if (o->reserved != 0) return fail(GC_ERR_INVALID, "gc_mxm_index_open: reserved must be 0");
	return mxmIndexOpen("gc_mxm_index_open", G, o->build, o->cache_prefix ? std::string(o->cache_prefix) : std::string(), out);
}

int gc_mxm_cache_check(const char* cache_prefix, uint64_t* info)
{
	if (!cache_prefix || !*cache_prefix) return fail(GC_ERR_INVALID, "gc_mxm_cache_check: no cache prefix");
	const std::string path = gc::mxmCachePath(cache_prefix);
	try {
		gc::MxmCacheFile file;
		gc::mxmCacheLoad(path, file);
		if (gc::mxmCacheTextFingerprint(file) != file.info.fingerprint) throw gc::MxmCacheError("MUM / MEM index cache " + path + ": the stored text does not have the stored fingerprint");
		if (info) { info[0] = file.info.version; info[1] = file.info.n; info[2] = file.info.segments; info[3] = file.info.fileBytes; info[4] = file.info.fingerprint; }
	} catch (const std::exception& e) {
		return fail(GC_ERR_GRAPH, e.what());
	}
	return GC_OK;
}
void gc_mxm_index_destroy(gc_mxm_index* x) { delete x; }

int gc_mxm_index_array(const gc_mxm_index* X, const char* name, int64_t** out, uint64_t* count)
{
	if (!X || !name || !out || !count) return fail(GC_ERR_INVALID, "null argument");
	const std::string nm = name;
	std::vector<int64_t> v;
	if (nm == "node_start") v.assign(X->nodeStart.begin(), X->nodeStart.end());
	else if (nm == "node_id") v.assign(X->nodeId.begin(), X->nodeId.end());
	else if (nm == "bytes") v.push_back((int64_t)X->deviceBytes);
	else if (nm == "build_us") v.push_back((int64_t)(X->buildSeconds * 1e6));
	else if (nm == "prefix_len") v.push_back((int64_t)X->dev.prefixLen);
	else if (nm == "sa_us") v.push_back((int64_t)(X->saSeconds * 1e6));
	else if (nm == "build_mode") v.push_back((int64_t)X->buildMode);
	else if (nm == "build_rounds") v.push_back((int64_t)X->buildRounds);
	else if (nm == "build_scratch_bytes") v.push_back((int64_t)X->buildScratchBytes);
	else if (nm == "cache_save_us") v.push_back((int64_t)(X->cacheSaveSeconds * 1e6));
	else if (nm == "sa") {
		std::vector<uint32_t> sa(X->dev.n);
		int rc = guarded([&]() { requireDevice(); if (X->dev.n) HIP_CHECK(hipMemcpy(sa.data(), X->dev.sa, (size_t)X->dev.n * 4, hipMemcpyDeviceToHost)); return (int)GC_OK; });
		if (rc != GC_OK) return rc;
		v.assign(sa.begin(), sa.end());
	}
	else return fail(GC_ERR_INVALID, "unknown index array " + nm);
	*out = mallocArray<int64_t>(v.size());
	memcpy(*out, v.data(), v.size() * sizeof(int64_t));
	*count = v.size();
	return GC_OK;
}

int gc_seeds_mxm(const gc_graph* G, const gc_mxm_index* X, const gc_reads* R, int32_t mode, uint64_t max_count, uint32_t min_len, gc_seeds** out)
{
	// host checks first: a malformed call is GC_ERR_INVALID whether or not a device is present
	if (!G || !X || !R || !out) return fail(GC_ERR_INVALID, "null argument");
	*out = nullptr;
	if (mode != GC_MXM_MUM && mode != GC_MXM_MEM) return fail(GC_ERR_INVALID, "gc_seeds_mxm: mode is neither GC_MXM_MUM nor GC_MXM_MEM");
	if (min_len < 2) return fail(GC_ERR_INVALID, "gc_seeds_mxm: min_len must be at least 2");
	if (max_count == 0) return fail(GC_ERR_INVALID, "gc_seeds_mxm: max_count must be at least 1 (UINT64_MAX: all)");
	if (X->graph != G) return fail(GC_ERR_INVALID, "gc_seeds_mxm: the index was built from another graph");
	const uint64_t nReads = R->offsets.size() - 1;
	// a read's tiles: 64 query positions of one strand each, forward strand first; none for a read shorter than min_len or with a letter outside the alphabet
	std::vector<uint32_t> tileOff(nReads + 1, 0);
	uint64_t tiles = 0;
	for (uint64_t r = 0; r < nReads; r++) {
		const uint64_t len = R->offsets[r + 1] - R->offsets[r];
		// (a hit's match_len and raw_goodness are at most the read's length, and match_len + read length + raw_goodness must stay below 2^32 as at upload)
		if (len >= 0x40000000ull) return fail(GC_ERR_INVALID, "gc_seeds_mxm: read " + std::to_string(r) + " has 2^30 letters or more");
		tileOff[r] = (uint32_t)tiles;
		if (len >= min_len && !R->invalid[r]) tiles += 2 * ((len - min_len + 1 + 63) / 64);
		if (tiles >= 0x7ffffff0ull) return fail(GC_ERR_INVALID, "gc_seeds_mxm: too many query positions in one batch; split the batch");
	}
	tileOff[nReads] = (uint32_t)tiles;
	gc_seeds* H = new gc_seeds();
	int rc = guarded([&]() {
		requireDevice();
		HIP_CHECK(hipGetDevice(&H->device));
		H->readOffsets = R->offsets;
		hipStream_t q = threadStream(H->device);
		DeviceBuffer dTileOff;
		uint32_t* pTileOff = dTileOff.reserve<uint32_t>(nReads + 1);
		HIP_CHECK(hipMemcpyAsync(pTileOff, tileOff.data(), (nReads + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, q));
		EventSet<2> ev;
		HIP_CHECK(hipEventRecord(ev[0], q));
		MxmSeedRun run;
		StreamDrain drain { q };   // (before `run` frees its scratch and dTileOff goes: nothing of this call may still be running)
		HIP_CHECK(run.candidates(q, X->dev, R->devBases, R->devOffsets, pTileOff, (uint32_t)nReads, (uint32_t)tiles, mode, min_len));
		if (run.nCandidates > 0x7fffffffull) return fail(GC_ERR_INVALID, "gc_seeds_mxm: 2^31 matches or more in one batch; split the batch");
		uint64_t nHits = 0;
		HIP_CHECK(run.select(q, (uint32_t)nReads, max_count, nHits));
		H->nHits = nHits;
		unsigned long long* dBad = allocateSeedBlock(*H, nReads);
		unsigned long long bad = ~0ull;
		HIP_CHECK(hipMemcpyAsync(dBad, &bad, sizeof(bad), hipMemcpyHostToDevice, q));
		HIP_CHECK(hipMemsetAsync(H->devReadHitOff, 0, (nReads + 1) * sizeof(uint32_t), q));
		HIP_CHECK(run.write(q, (uint32_t)nReads, nHits, H->devHits, H->devReadHitOff));
		const SeedLookup lookup { G->dev.origSize, G->dev.lookupOff, G->dev.lookup, G->dev.nodeOffset, (uint32_t)G->hOrigSize.size() };
		launchSeedResolve(q, lookup, H->devHits, nHits, H->devReadHitOff, (uint32_t)nReads, R->devOffsets, H->dev, dBad);
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipEventRecord(ev[1], q));
		HIP_CHECK(hipMemcpyAsync(&bad, dBad, sizeof(bad), hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipStreamSynchronize(q));
		H->kernelMs = ev.elapsedMs(0, 1);
		if (bad != ~0ull) throw std::runtime_error("gc_seeds_mxm: a match does not resolve to a position of the graph (hit " + std::to_string(bad >> 2) + ")");   // (the index and the graph disagree: a bug, not an input)
		return (int)GC_OK;
	});
	if (rc != GC_OK) { delete H; return rc; }
	*out = H;
	return GC_OK;
}

// ---- seeds from GAM files (the reference's -s: src/Aligner.cpp:1169-1190, src/stream.hpp:81-123) --------------------
} // extern "C"

namespace {

struct SeedFileInvalid : std::runtime_error { using std::runtime_error::runtime_error; };
struct SeedFileUnreadable : std::runtime_error { using std::runtime_error::runtime_error; };

// a device array that grows by doubling and keeps what it holds
struct SeedStoreArray {
	void* p = nullptr;
	size_t cap = 0;
	void ensure(size_t used, size_t need, hipStream_t q)
	{
		if (need <= cap) return;
		const size_t want = std::max(need + 256, cap * 2);
		void* grown = nullptr;
		HIP_CHECK(hipMalloc(&grown, want));
		hipError_t e = used ? hipMemcpyAsync(grown, p, used, hipMemcpyDeviceToDevice, q) : hipSuccess;
		if (e == hipSuccess) e = hipStreamSynchronize(q);
		if (e != hipSuccess) { (void)hipFree(grown); HIP_CHECK(e); }
		if (p) (void)hipFree(p);
		p = grown; cap = want;
	}
	// the doubling's head room goes back before the store keeps the array
	void fit(size_t used, hipStream_t q)
	{
		if (!p || cap <= used + used / 16 + 4096) return;
		SeedStoreArray exact;
		exact.ensure(0, used, q);
		HIP_CHECK(hipMemcpyAsync(exact.p, p, used, hipMemcpyDeviceToDevice, q));
		HIP_CHECK(hipStreamSynchronize(q));
		std::swap(p, exact.p); std::swap(cap, exact.cap);
	}
	void* handOver(gc_seed_store& S) { void* r = p; if (r) { S.allocations.push_back(r); S.deviceBytes += cap; } p = nullptr; cap = 0; return r; }
	~SeedStoreArray() { if (p) (void)hipFree(p); }
};

double msSince(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// pieces in, a gc_seed_store out: every piece is uploaded, decoded into the growing arrays and dropped
struct SeedStoreBuilder {
	gc_seed_store& S;
	hipStream_t q;
	gc::Switches sw = gc::Switches::fromEnvironment();
	SeedStoreArray hits, hash, nameOff, nameLen, pool;
	DeviceBuffer piece, msgOff, nameStart, local, temp, flags;
	hipEvent_t e0 = nullptr, e1 = nullptr;
	uint64_t n = 0, poolUsed = 0;
	unsigned long long* dBad = nullptr;
	std::vector<uint64_t> fileFirst;   // the first message of every file among all messages
	double sinkMs = 0;

	SeedStoreBuilder(gc_seed_store& store, hipStream_t stream) : S(store), q(stream)
	{
		HIP_CHECK(hipEventCreate(&e0)); HIP_CHECK(hipEventCreate(&e1));
		dBad = flags.reserve<unsigned long long>(2);
		const unsigned long long none = ~0ull;
		HIP_CHECK(hipMemcpyAsync(dBad, &none, sizeof(none), hipMemcpyHostToDevice, q));
		HIP_CHECK(hipMemsetAsync(dBad + 1, 0, sizeof(unsigned long long), q));
		HIP_CHECK(hipStreamSynchronize(q));
	}
	~SeedStoreBuilder() { (void)hipStreamSynchronize(q); if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }

	void addPiece(const uint8_t* bytes, size_t len, const uint32_t* off, uint32_t count)
	{
		const auto t0 = std::chrono::steady_clock::now();
		if (n + count >= 0x7fffffffull) throw SeedFileInvalid("2^31 - 1 messages or more");
		uint8_t* dPiece = piece.reserve<uint8_t>(len + 16);   // (k_sf_decode stages whole 16-byte words)
		uint32_t* dOff = msgOff.reserve<uint32_t>((size_t)count + 1);
		HIP_CHECK(hipMemcpyAsync(dPiece, bytes, len, hipMemcpyHostToDevice, q));
		HIP_CHECK(hipMemcpyAsync(dOff, off, ((size_t)count + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, q));
		hits.ensure(n * sizeof(SeedHit), (n + count) * sizeof(SeedHit), q);
		hash.ensure(n * 8, (n + count) * 8, q);
		nameOff.ensure(n * 8, (n + count) * 8, q);
		nameLen.ensure(n * 4, (n + count) * 4, q);
		uint32_t* dStart = nameStart.reserve<uint32_t>(count);
		uint32_t* dLocal = local.reserve<uint32_t>(count);
		const size_t tempBytes = sfTempBytes(count, 0);
		void* dTemp = temp.reserve<char>(tempBytes);
		HIP_CHECK(hipStreamSynchronize(q));
		S.uploadMs += msSince(t0);
		uint32_t* lens = (uint32_t*)nameLen.p + n;
		HIP_CHECK(hipEventRecord(e0, q));
		HIP_CHECK(sfDecodePiece(q, dPiece, dOff, count, n, sw.testSeedfileHashBits, (SeedHit*)hits.p + n, (uint64_t*)hash.p + n, dStart, lens, dBad));
		HIP_CHECK(sfScanNameLengths(q, dTemp, tempBytes, lens, count, dLocal));
		uint32_t last[2] = { 0, 0 };
		HIP_CHECK(hipMemcpyAsync(&last[0], dLocal + (count - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipMemcpyAsync(&last[1], lens + (count - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipStreamSynchronize(q));
		const uint64_t total = (uint64_t)last[0] + last[1];   // (the names lie inside the piece: at most its bytes)
		pool.ensure(poolUsed, poolUsed + total, q);
		HIP_CHECK(sfCopyNames(q, dPiece, dOff, dStart, lens, dLocal, count, poolUsed, (uint8_t*)pool.p, (uint64_t*)nameOff.p + n));
		HIP_CHECK(hipEventRecord(e1, q));
		HIP_CHECK(hipStreamSynchronize(q));
		float ms = 0;
		HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
		S.decodeMs += ms;
		poolUsed += total;
		n += count;
		sinkMs += msSince(t0);
	}

	// after every file: the first message the device refused, by file and index
	void check()
	{
		unsigned long long bad = ~0ull;
		HIP_CHECK(hipMemcpyAsync(&bad, dBad, sizeof(bad), hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipStreamSynchronize(q));
		if (bad == ~0ull) return;
		const uint64_t i = bad >> 2;
		const size_t f = (size_t)(std::upper_bound(fileFirst.begin(), fileFirst.end(), i) - fileFirst.begin()) - 1;
		const char* what[] = { "", "has no mapping", "has a mapping without an edit", "does not parse as a vg::Alignment" };
		throw SeedFileInvalid("file " + std::to_string(f) + " message " + std::to_string(i - fileFirst[f]) + " " + what[bad & 3]);
	}

	void oneStream(uint32_t index, const std::function<void(gc::SeedFileFramer&)>& feed)
	{
		fileFirst.push_back(n);
		gc::SeedFileFramer framer(sw.testSeedfilePiece, [&](const uint8_t* bytes, size_t len, const uint32_t* off, uint32_t count, uint64_t) { addPiece(bytes, len, off, count); });
		try {
			feed(framer);
			framer.finish();
		} catch (const gc::SeedFileError& e) {
			throw SeedFileInvalid("file " + std::to_string(index) + ": " + e.what());
		} catch (const SeedFileInvalid& e) {
			throw SeedFileInvalid("file " + std::to_string(index) + ": " + e.what());
		}
		S.messages += framer.messages();
		S.seeds += framer.seeds();
		check();
	}

	void finish()
	{
		if (n) {
			SeedStoreArray sorted, order;
			sorted.ensure(0, n * 8, q);
			order.ensure(0, n * 4, q);
			const size_t tempBytes = sfTempBytes((uint32_t)n, 0);
			void* dTemp = temp.reserve<char>(tempBytes);
			uint32_t* dIota = local.reserve<uint32_t>(n);
			HIP_CHECK(hipEventRecord(e0, q));
			HIP_CHECK(sfSortStore(q, dTemp, tempBytes, (const uint64_t*)hash.p, (uint32_t)n, (uint64_t*)sorted.p, (uint32_t*)order.p, dIota, (uint32_t*)(dBad + 1)));
			HIP_CHECK(hipEventRecord(e1, q));
			uint32_t distinct = 0;
			HIP_CHECK(hipMemcpyAsync(&distinct, dBad + 1, sizeof(distinct), hipMemcpyDeviceToHost, q));
			HIP_CHECK(hipStreamSynchronize(q));
			float ms = 0;
			HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
			S.sortMs = ms;
			S.distinct = distinct;
			S.dev.sortedHash = (const uint64_t*)sorted.handOver(S);
			S.dev.order = (const uint32_t*)order.handOver(S);
		}
		hits.fit(n * sizeof(SeedHit), q); nameOff.fit(n * 8, q); nameLen.fit(n * 4, q); pool.fit(poolUsed, q);
		S.dev.hits = (const SeedHit*)hits.handOver(S);
		S.dev.nameOff = (const uint64_t*)nameOff.handOver(S);
		S.dev.nameLen = (const uint32_t*)nameLen.handOver(S);
		S.dev.namePool = (const uint8_t*)pool.handOver(S);
		S.dev.n = (uint32_t)n;
		S.dev.hashBits = sw.testSeedfileHashBits;
	}
};

// the file's inflated bytes into the framer: gzip or zlib by the header, concatenated members read through (as api._file_chunks reads a read file)
void seedFileInflate(const char* path, gc::SeedFileFramer& framer, SeedStoreBuilder& B)
{
	FILE* f = fopen(path, "rb");
	if (!f) throw SeedFileUnreadable(std::string("cannot open seeds file ") + path);
	struct Close { FILE* f; ~Close() { fclose(f); } } close { f };
	z_stream z;
	memset(&z, 0, sizeof(z));
	if (inflateInit2(&z, 47) != Z_OK) throw std::runtime_error("zlib: inflateInit2 failed");
	struct End { z_stream* z; ~End() { inflateEnd(z); } } end { &z };
	std::vector<uint8_t> in(1 << 20), out(4 << 20);
	bool inMember = false;
	for (;;) {
		const size_t got = fread(in.data(), 1, in.size(), f);
		if (!got) break;
		z.next_in = in.data(); z.avail_in = (uInt)got;
		while (z.avail_in) {
			z.next_out = out.data(); z.avail_out = (uInt)out.size();
			const auto t0 = std::chrono::steady_clock::now();
			const int rc = inflate(&z, Z_NO_FLUSH);
			B.S.inflateMs += msSince(t0);
			const size_t produced = out.size() - z.avail_out;
			if (rc != Z_OK && rc != Z_STREAM_END && !(rc == Z_BUF_ERROR && produced)) throw SeedFileInvalid(std::string("the stream is neither gzip nor zlib, or is damaged (") + (z.msg ? z.msg : "zlib error") + ")");
			inMember = rc != Z_STREAM_END;
			if (produced) {
				const auto t1 = std::chrono::steady_clock::now();
				const double sinkBefore = B.sinkMs;
				framer.push(out.data(), produced);
				B.S.frameMs += msSince(t1) - (B.sinkMs - sinkBefore);
			}
			if (rc == Z_STREAM_END && inflateReset(&z) != Z_OK) throw std::runtime_error("zlib: inflateReset failed");
		}
	}
	if (inMember) throw SeedFileInvalid("the file ends inside a compressed member");
}

int seedStoreMake(uint32_t n, const std::function<void(uint32_t, gc::SeedFileFramer&, SeedStoreBuilder&)>& feed, gc_seed_store** out)
{
	gc_seed_store* S = new gc_seed_store();
	int rc = guarded([&]() {
		try {
			requireDevice();
			HIP_CHECK(hipGetDevice(&S->device));
			SeedStoreBuilder B(*S, threadStream(S->device));
			for (uint32_t i = 0; i < n; i++) B.oneStream(i, [&](gc::SeedFileFramer& framer) { feed(i, framer, B); });
			B.finish();
			return (int)GC_OK;
		} catch (const SeedFileInvalid& e) {
			return fail(GC_ERR_INVALID, std::string("seeds file: ") + e.what());
		} catch (const SeedFileUnreadable& e) {
			return fail(GC_ERR_GRAPH, e.what());
		}
	});
	if (rc != GC_OK) { delete S; return rc; }
	*out = S;
	return GC_OK;
}

} // namespace

extern "C" {

int gc_seed_store_open(const char* const* paths, uint32_t n_paths, gc_seed_store** out)
{
	if (!out || (n_paths && !paths)) return fail(GC_ERR_INVALID, "null argument");
	*out = nullptr;
	for (uint32_t i = 0; i < n_paths; i++) if (!paths[i]) return fail(GC_ERR_INVALID, "null argument");
	return seedStoreMake(n_paths, [&](uint32_t i, gc::SeedFileFramer& framer, SeedStoreBuilder& B) { seedFileInflate(paths[i], framer, B); }, out);
}

int gc_seed_store_from_memory(const void* const* streams, const uint64_t* lens, uint32_t n, gc_seed_store** out)
{
	if (!out || (n && (!streams || !lens))) return fail(GC_ERR_INVALID, "null argument");
	*out = nullptr;
	for (uint32_t i = 0; i < n; i++) if (!streams[i] && lens[i]) return fail(GC_ERR_INVALID, "null argument");
	return seedStoreMake(n, [&](uint32_t i, gc::SeedFileFramer& framer, SeedStoreBuilder& B) {
		const auto t0 = std::chrono::steady_clock::now();
		const double sinkBefore = B.sinkMs;
		if (lens[i]) framer.push((const uint8_t*)streams[i], lens[i]);
		B.S.frameMs += msSince(t0) - (B.sinkMs - sinkBefore);
	}, out);
}

int gc_seed_store_info(const gc_seed_store* s, gc_seed_store_stats* o)
{
	if (!s || !o) return fail(GC_ERR_INVALID, "null argument");
	o->messages = s->messages; o->seeds = s->seeds; o->distinct_hashes = s->distinct; o->hbm_bytes = s->deviceBytes;
	o->inflate_ms = s->inflateMs; o->frame_ms = s->frameMs; o->upload_ms = s->uploadMs; o->decode_ms = s->decodeMs; o->sort_ms = s->sortMs;
	o->host_ms = s->inflateMs + s->frameMs; o->device_ms = s->decodeMs + s->sortMs;
	return GC_OK;
}
void gc_seed_store_destroy(gc_seed_store* s) { delete s; }

int gc_seeds_from_store(const gc_graph* G, const gc_seed_store* S, const gc_reads* R, const char* names, const uint64_t* name_off, uint64_t n_reads, gc_seeds** out)
{
	// host checks first: a malformed call is GC_ERR_INVALID whether or not a device is present
	if (!G || !S || !R || !name_off || !out) return fail(GC_ERR_INVALID, "null argument");
	*out = nullptr;
	if (n_reads != R->offsets.size() - 1) return fail(GC_ERR_INVALID, "gc_seeds_from_store: n_reads differs from the read batch's");
	if (n_reads >= 0xfffffff0ull) return fail(GC_ERR_INVALID, "gc_seeds_from_store: too many reads");
	if (name_off[0] != 0) return fail(GC_ERR_INVALID, "gc_seeds_from_store: name_off must start at 0");
	for (uint64_t r = 0; r < n_reads; r++) if (name_off[r + 1] <= name_off[r]) return fail(GC_ERR_INVALID, "gc_seeds_from_store: read " + std::to_string(r) + " has no name and terminator byte in name_off");
	const uint64_t nameBytes = name_off[n_reads];
	if (nameBytes && !names) return fail(GC_ERR_INVALID, "null argument");
	gc_seeds* H = new gc_seeds();
	int rc = guarded([&]() {
		requireDevice();
		HIP_CHECK(hipGetDevice(&H->device));
		H->readOffsets = R->offsets;
		hipStream_t q = threadStream(H->device);
		DeviceBuffer dNames, dNameOff, dFirst, dCount, dOff64, dTemp;
		StreamDrain drain { q };   // (before the buffers above go: nothing of this call may still be running)
		uint8_t* pNames = dNames.reserve<uint8_t>(nameBytes);
		uint64_t* pNameOff = dNameOff.reserve<uint64_t>(n_reads + 1);
		uint32_t* pFirst = dFirst.reserve<uint32_t>(n_reads);
		uint64_t* pCount = dCount.reserve<uint64_t>(n_reads + 1);
		uint64_t* pOff64 = dOff64.reserve<uint64_t>(n_reads + 1);
		const size_t tempBytes = sfTempBytes(0, (uint32_t)n_reads);
		void* pTemp = dTemp.reserve<char>(tempBytes);
		if (nameBytes) HIP_CHECK(hipMemcpyAsync(pNames, names, nameBytes, hipMemcpyHostToDevice, q));
		HIP_CHECK(hipMemcpyAsync(pNameOff, name_off, (n_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, q));
		EventSet<2> ev;
		HIP_CHECK(hipEventRecord(ev[0], q));
		HIP_CHECK(sfJoinCount(q, S->dev, pNames, pNameOff, (uint32_t)n_reads, pFirst, pCount));
		HIP_CHECK(sfJoinScan(q, pTemp, tempBytes, pCount, (uint32_t)n_reads, pOff64));
		uint64_t nHits = 0;
		HIP_CHECK(hipMemcpyAsync(&nHits, pOff64 + n_reads, sizeof(nHits), hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipStreamSynchronize(q));
		if (nHits >= 0xfffffff0ull) return fail(GC_ERR_INVALID, "gc_seeds_from_store: 2^32 hits or more; split the batch");
		H->nHits = nHits;
		unsigned long long* dBad = allocateSeedBlock(*H, n_reads);   // resolve, match_len, raw_goodness
		unsigned long long bad[3] = { ~0ull, ~0ull, ~0ull };
		HIP_CHECK(hipMemcpyAsync(dBad, bad, sizeof(bad), hipMemcpyHostToDevice, q));
		HIP_CHECK(sfJoinGather(q, S->dev, pNames, pNameOff, (uint32_t)n_reads, pFirst, pOff64, R->devOffsets, H->devHits, H->devReadHitOff, dBad + 1, dBad + 2));
		const SeedLookup lookup { G->dev.origSize, G->dev.lookupOff, G->dev.lookup, G->dev.nodeOffset, (uint32_t)G->hOrigSize.size() };
		launchSeedResolve(q, lookup, H->devHits, nHits, H->devReadHitOff, (uint32_t)n_reads, R->devOffsets, H->dev, dBad);
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipEventRecord(ev[1], q));
		HIP_CHECK(hipMemcpyAsync(bad, dBad, sizeof(bad), hipMemcpyDeviceToHost, q));
		HIP_CHECK(hipStreamSynchronize(q));
		H->kernelMs = ev.elapsedMs(0, 1);
		// gc_seeds_upload's order: its host checks read by read (a read's match_len before its raw_goodness), then the device's
		if (bad[1] != ~0ull || bad[2] != ~0ull) {
			const bool len = bad[1] != ~0ull && (bad[2] == ~0ull || (bad[1] >> 32) <= (bad[2] >> 32));
			const unsigned long long b = len ? bad[1] : bad[2];
			return fail(GC_ERR_INVALID, "gc_seeds_from_store: read " + std::to_string(b >> 32) + " hit " + std::to_string(b & 0xffffffffull) + ": " +
				(len ? "match_len of 2^31 or more" : "raw_goodness too large for the 32-bit seed goodness (match_len + read length + raw_goodness must stay below 2^32)"));
		}
		if (bad[0] != ~0ull) {
			const uint64_t i = bad[0] >> 2;
			std::vector<uint32_t> off32(n_reads + 1);
			HIP_CHECK(hipMemcpy(off32.data(), H->devReadHitOff, (n_reads + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
			const uint64_t r = (uint64_t)(std::upper_bound(off32.begin(), off32.end(), (uint32_t)i) - off32.begin()) - 1;
			const char* what[] = { "", "no such node in the graph", "node_offset is not inside the original node", "seq_pos is not inside the read" };
			return fail(GC_ERR_INVALID, "gc_seeds_from_store: read " + std::to_string(r) + " hit " + std::to_string(i - off32[r]) + ": " + what[bad[0] & 3]);
		}
		return (int)GC_OK;
	});
	if (rc != GC_OK) { delete H; return rc; }
	*out = H;
	return GC_OK;
}

} // extern "C"
