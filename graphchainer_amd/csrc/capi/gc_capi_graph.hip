// C entry points, graphs, minimizer seeders and the index cache: gc_graph_create / _create_from_gfa / _destroy / _num_nodes / _size_bp / _trim_host / _array,
// gc_seeder_create / _destroy / _array, gc_index_build / _save / _check / _load.
#include "../gc_runtime.hpp"
#include "../host/gc_stageclock.hpp"
#include <malloc.h>

extern "C" {

int gc_graph_create_from_gfa(const char* gfa_path, gc_graph** out)
{
	if (!gfa_path || !out) return fail(GC_ERR_INVALID, "null argument");
	*out = nullptr;
	gc_graph* G = new gc_graph();
	try {
		requireDevice();
		gc::StageClock clock;
		G->host = gc::AlignmentGraph::BuildFromGFAFile(gfa_path);
		G->host.buildMPC(true);
		malloc_trim(0);   // (the builders' freed small blocks back to the system: the host graph stays, and at config 5's sizes the host's memory is what bounds the graph)
		clock.lap("graph + MPC built");
		uploadGraph(G);
		clock.lap("graph uploaded");
	} catch (const DeviceError& e) {
		delete G;
		return fail(GC_ERR_DEVICE, e.what());
	} catch (const std::exception& e) {
		delete G;
		return fail(GC_ERR_GRAPH, e.what());
	}
	*out = G;
	return GC_OK;
}

int gc_graph_create(const gc_graph_desc* desc, gc_graph** out)
{
	if (!desc || !out) return fail(GC_ERR_INVALID, "null argument");
	*out = nullptr;
	gc_graph* G = new gc_graph();
	try {
		requireDevice();
		gc::AlignmentGraph& h = G->host;
		size_t n = desc->n_nodes;
		h.firstAmbiguous = desc->first_ambiguous;
		h.nodeLength.resize(n); h.nodeOffset.resize(n); h.nodeIDs.resize(n); h.reverse.resize(n); h.linearizable.assign(n, false);
		h.inNeighbors.resize(n); h.outNeighbors.resize(n);
		h.componentNumber.resize(n); h.chainNumber.resize(n); h.chainApproxPos.resize(n);
		for (size_t i = 0; i < n; i++) {
			h.nodeLength[i] = desc->node_length[i];
			h.nodeOffset[i] = desc->node_offset[i];
			h.nodeIDs[i] = desc->node_ids[i];
			h.reverse[i] = desc->node_ids[i] & 1;   // reverse-complement strand nodes have odd bigraph ids (src/BigraphToDigraph.cpp:101-104)
			h.bpSize += desc->node_length[i];
			for (uint64_t e = desc->in_off[i]; e < desc->in_off[i + 1]; e++) h.inNeighbors[i].push_back(desc->in_adj[e]);
			for (uint64_t e = desc->out_off[i]; e < desc->out_off[i + 1]; e++) h.outNeighbors[i].push_back(desc->out_adj[e]);
			h.componentNumber[i] = desc->component_number[i];
			h.chainNumber[i] = desc->chain_number[i];
			h.chainApproxPos[i] = desc->chain_approx_pos[i];
		}
		h.nodeSequences.resize(h.firstAmbiguous);
		for (size_t i = 0; i < h.firstAmbiguous; i++) h.nodeSequences[i] = { desc->node_seq[2 * i], desc->node_seq[2 * i + 1] };
		h.ambiguousNodeSequences.resize(n - h.firstAmbiguous);
		for (size_t i = 0; i < n - h.firstAmbiguous; i++) h.ambiguousNodeSequences[i] = { desc->ambiguous_seq[4 * i], desc->ambiguous_seq[4 * i + 1], desc->ambiguous_seq[4 * i + 2], desc->ambiguous_seq[4 * i + 3] };
		// nodeLookup: split nodes of each bigraph node in offset order
		std::vector<size_t> order(n);
		for (size_t i = 0; i < n; i++) order[i] = i;
		std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return h.nodeIDs[a] != h.nodeIDs[b] ? h.nodeIDs[a] < h.nodeIDs[b] : h.nodeOffset[a] < h.nodeOffset[b]; });
		// (without a lookup_order from the caller the minimizer index follows the order an unordered_map filled with the ids in ascending order iterates in - as r1-r3 built it)
		gc::HashOrder ascending;
		std::vector<int> ascendingIds;
		for (size_t at = 0; at < n;) {
			size_t end = at;
			while (end < n && h.nodeIDs[order[end]] == h.nodeIDs[order[at]]) end++;
			h.nodeLookup.add(h.nodeIDs[order[at]], order.data() + at, end - at);
			for (size_t k = at; k < end; k++) h.originalNodeSize[h.nodeIDs[order[at]]] += h.nodeLength[order[k]];
			ascending.insert(std::hash<int>()(h.nodeIDs[order[at]]));
			ascendingIds.push_back(h.nodeIDs[order[at]]);
			at = end;
		}
		for (uint32_t e : ascending.order()) h.nodeLookupOrder.push_back(ascendingIds[e]);
		if (desc->lookup_order) {
			// the host's nodeLookup iteration order: the minimizer index enumerates nodes in it (src/MinimizerSeeder.cpp:354-357)
			if (desc->n_lookup != h.nodeLookup.size()) throw std::runtime_error("lookup_order must list every bigraph node id once");
			std::unordered_set<int> seen;
			for (uint64_t i = 0; i < desc->n_lookup; i++)
				if (!h.nodeLookup.count(desc->lookup_order[i]) || !seen.insert(desc->lookup_order[i]).second) throw std::runtime_error("lookup_order must list every bigraph node id once");
			h.nodeLookupOrder.assign(desc->lookup_order, desc->lookup_order + desc->n_lookup);
		}
		h.finalized = true;
		h.buildMPC(true);
		uploadGraph(G);
	} catch (const DeviceError& e) {
		delete G;
		return fail(GC_ERR_DEVICE, e.what());
	} catch (const std::exception& e) {
		delete G;
		return fail(GC_ERR_GRAPH, e.what());
	}
	*out = G;
	return GC_OK;
}

void gc_graph_destroy(gc_graph* g) { delete g; malloc_trim(0); }   // (the host graph's many small blocks back to the system, not to the allocator's free lists: a graph loaded next would sit beside them)
uint64_t gc_graph_num_nodes(const gc_graph* g) { return g ? g->host.NodeSize() : 0; }
uint64_t gc_graph_size_bp(const gc_graph* g) { return g ? g->host.SizeInBP() : 0; }

int gc_graph_trim_host(gc_graph* G)
{
	if (!G) return fail(GC_ERR_INVALID, "null argument");
	gc::AlignmentGraph& h = G->host;
	std::vector<std::vector<std::vector<size_t>>>().swap(h.mpc);
	std::vector<std::vector<std::vector<size_t>>>().swap(h.paths);
	std::vector<std::vector<std::vector<std::pair<size_t, size_t>>>>().swap(h.backwards);
	std::vector<std::vector<size_t>>().swap(h.topo);
	std::vector<std::vector<size_t>>().swap(h.topo_ids);
	std::vector<std::vector<size_t>>().swap(h.component_ids);
	G->hostMpcTrimmed = true;
	malloc_trim(0);
	return GC_OK;
}

int gc_graph_array(const gc_graph* G, const char* name, int64_t** out, uint64_t* count)
{
	if (!G || !name || !out || !count) return fail(GC_ERR_INVALID, "null argument");
	if (G->hostMpcTrimmed && (strncmp(name, "mpc_", 4) == 0 || strncmp(name, "paths", 5) == 0 || strncmp(name, "back_", 5) == 0 || strcmp(name, "topo_id") == 0))
		return fail(GC_ERR_INVALID, "the host copy of the MPC index was released (gc_graph_trim_host)");
	const gc::AlignmentGraph& g = G->host;
	std::vector<int64_t> v;
	std::string nm = name;
	size_t n = g.NodeSize();
	if (nm == "nodeLength") for (size_t i = 0; i < n; i++) v.push_back(g.nodeLength[i]);
	else if (nm == "nodeOffset") for (size_t i = 0; i < n; i++) v.push_back(g.nodeOffset[i]);
	else if (nm == "nodeIDs") for (size_t i = 0; i < n; i++) v.push_back(g.nodeIDs[i]);
	else if (nm == "reverse") for (size_t i = 0; i < n; i++) v.push_back(g.reverse[i]);
	else if (nm == "componentNumber") for (size_t i = 0; i < n; i++) v.push_back(g.componentNumber[i]);
	else if (nm == "chainNumber") for (size_t i = 0; i < n; i++) v.push_back(g.chainNumber[i]);
	else if (nm == "chainApproxPos") for (size_t i = 0; i < n; i++) v.push_back(g.chainApproxPos[i]);
	else if (nm == "component_map") for (size_t i = 0; i < n; i++) v.push_back(g.component_map[i]);
	else if (nm == "out_off") { v.push_back(0); for (size_t i = 0; i < n; i++) v.push_back(v.back() + (int64_t)g.outNeighbors[i].size()); }
	else if (nm == "out_adj") for (size_t i = 0; i < n; i++) for (size_t x : g.outNeighbors[i]) v.push_back(x);
	else if (nm == "in_off") { v.push_back(0); for (size_t i = 0; i < n; i++) v.push_back(v.back() + (int64_t)g.inNeighbors[i].size()); }
	else if (nm == "in_adj") for (size_t i = 0; i < n; i++) for (size_t x : g.inNeighbors[i]) v.push_back(x);
	else if (nm == "mpc_width") for (size_t c = 0; c < g.mpc.size(); c++) v.push_back(g.mpc[c].size());
	else if (nm == "firstAmbiguous") v.push_back((int64_t)std::min(g.firstAmbiguous, n));
	else if (nm == "nodeSeq") for (size_t i = 0; i < n && i < g.firstAmbiguous; i++) { v.push_back((int64_t)g.nodeSequences[i][0]); v.push_back((int64_t)g.nodeSequences[i][1]); }   // bit patterns
	else if (nm == "ambiguousSeq") for (const gc::AmbiguousSeq& a : g.ambiguousNodeSequences) { v.push_back((int64_t)a.A); v.push_back((int64_t)a.T); v.push_back((int64_t)a.C); v.push_back((int64_t)a.G); }
	else if (nm == "component_idx") for (size_t i = 0; i < n; i++) v.push_back(g.component_idx[i]);
	else if (nm == "topo_id") for (size_t i = 0; i < n; i++) v.push_back(g.topo_ids[g.component_map[i]][g.component_idx[i]]);
	// the path cover: mpc_path_comp[p] = component of path p, mpc_path_off / mpc_path_nodes = its nodes (global ids) in order
	else if (nm == "mpc_path_comp") { for (size_t c = 0; c < g.mpc.size(); c++) for (size_t k = 0; k < g.mpc[c].size(); k++) v.push_back(c); }
	else if (nm == "mpc_path_off") { v.push_back(0); for (size_t c = 0; c < g.mpc.size(); c++) for (const auto& p : g.mpc[c]) v.push_back(v.back() + (int64_t)p.size()); }
	else if (nm == "mpc_path_nodes") { for (size_t c = 0; c < g.mpc.size(); c++) for (const auto& p : g.mpc[c]) for (size_t x : p) v.push_back(x); }
	// per node (global id): the path ids through it (local to its component), and the backward links (node = global id, path id)
	else if (nm == "paths_off") { v.push_back(0); for (size_t i = 0; i < n; i++) v.push_back(v.back() + (int64_t)g.paths[g.component_map[i]][g.component_idx[i]].size()); }
	else if (nm == "paths") { for (size_t i = 0; i < n; i++) for (size_t k : g.paths[g.component_map[i]][g.component_idx[i]]) v.push_back(k); }
	else if (nm == "back_off") { v.push_back(0); for (size_t i = 0; i < n; i++) v.push_back(v.back() + (int64_t)g.backwards[g.component_map[i]][g.component_idx[i]].size()); }
	else if (nm == "back_node") { for (size_t i = 0; i < n; i++) for (const auto& b : g.backwards[g.component_map[i]][g.component_idx[i]]) v.push_back(g.component_ids[g.component_map[i]][b.first]); }
	else if (nm == "back_path") { for (size_t i = 0; i < n; i++) for (const auto& b : g.backwards[g.component_map[i]][g.component_idx[i]]) v.push_back(b.second); }
	else if (nm == "lookupOrder") { for (int id : g.nodeLookupOrder) v.push_back(id); }
	else return fail(GC_ERR_INVALID, "unknown graph array " + nm);
	*out = mallocArray<int64_t>(v.size());
	memcpy(*out, v.data(), v.size() * sizeof(int64_t));
	*count = v.size();
	return GC_OK;
}

// ---- seeder -------------------------------------------------------------------------------------------
static inline uint32_t hostHashKmer(uint64_t kmer) { kmer *= 0x9E3779B97F4A7C15ull; return (uint32_t)(kmer >> 32); }

// hash table, membership filter and start offsets of a built minimizer index -> HBM
static void uploadSeeder(gc_seeder* S, std::optional<uint32_t> filterBitsOverride)   // (GC_TEST_SEED_FILTER_BITS)
{
	size_t nKeys = S->host.kmers.size();
	size_t tableSize = 16;
	while (tableSize < 2 * nKeys) tableSize <<= 1;
	std::vector<uint64_t> table(tableSize, ~0ull);
	for (size_t i = 0; i < nKeys; i++) {
		uint32_t hsh = hostHashKmer(S->host.kmers[i]) & (uint32_t)(tableSize - 1);
		while (table[hsh] != ~0ull) hsh = (hsh + 1) & (uint32_t)(tableSize - 1);
		table[hsh] = ((S->host.kmers[i] & 0xffffffffull) << 32) | (uint64_t)i;   // (k <= 15: the whole k-mer; longer ones are verified against wideKmers)
	}
	if (nKeys >= 0xffffffffull) throw std::runtime_error("minimizer index too large for 32-bit key indices");
	S->dev.wideKmers = nullptr;
	if (S->host.k > 15) {
		uint64_t* dKmers = uploadVector(S->host.kmers);
		S->allocations.push_back(dKmers);
		S->dev.wideKmers = dKmers;
	}
	uint64_t* dTable = uploadVector(table);
	S->allocations.push_back(dTable);
	// membership filter in front of the table (see filterBit in gc_seedlookup.hip): ~8 bits per key, at most 2^28 bits; on cfg2 (5 M keys)
	// 2^25 bits = 4 MB, which stays in every XCD's L2 (a 32 MB filter missed to the fabric on every probe)
	uint32_t filterBits = 20;
	while (filterBits < 28 && (1ull << filterBits) < 8 * nKeys) filterBits++;
	if (filterBitsOverride) filterBits = *filterBitsOverride;
	std::vector<uint32_t> filter((1ull << filterBits) / 32, 0);
	for (size_t i = 0; i < nKeys; i++) { uint32_t fb = (uint32_t)((S->host.kmers[i] * 0xD6E8FEB86659FD93ull) >> (64 - filterBits)); filter[fb >> 5] |= 1u << (fb & 31); }
	S->dev.filterShift = 64 - filterBits;
	uint32_t* dFilter = uploadVector(filter);
	S->allocations.push_back(dFilter);
	S->dev.filter = dFilter;
	uint64_t* dStart = uploadVector(S->host.startPos);
	S->allocations.push_back(dStart);
	S->dev.table = dTable;
	S->dev.tableMask = (uint32_t)(tableSize - 1);
	S->dev.startPos = dStart;
	uint64_t* dPositions = uploadVector(S->host.positions);   // the occurrence lists: the device expands the seeds itself (gc_seedglue.hip)
	S->allocations.push_back(dPositions);
	S->dev.positions = dPositions;
	S->dev.nKeys = (uint32_t)nKeys;
	S->dev.maxCount = (uint32_t)std::min<size_t>(S->host.maxCount, 0xffffffffu);
	S->dev.k = (int32_t)S->host.k;
	S->dev.w = (int32_t)S->host.w;
}

// The minimizer index built by the device (gc_minimizer.hip): window scan per bigraph node, one radix sort; the host only cuts the sorted
// pairs into the k-mer groups. Same index as gc::MinimizerIndex::Build (tests/test_index_cache.py compares them array by array).
// false = not applicable here (deque longer than the kernel's ring), the caller builds on the host - as it does under GC_SEEDER_BUILD=host.
static bool buildSeederOnDevice(const gc_graph* G, gc_seeder* S, size_t k, size_t w, double keepLeastFrequentFraction)
{
	if (w - k + 2 > 32 || k > 15) return false;   // (the device build packs the k-mer into 30 bits of its sort key: longer minimizers are built on the host)
	const gc::AlignmentGraph& h = G->host;
	// minimizers ending inside an overlap prefix are skipped (src/MinimizerSeeder.cpp:323-340,369): never the case for the 0M graphs the
	// library loads, checked rather than assumed
	for (size_t i = 0; i < h.NodeSize(); i++) {
		if (h.nodeOffset[i] == 0) continue;
		for (size_t nb : h.inNeighbors[i]) if (h.nodeIDs[nb] != h.nodeIDs[i]) return false;
	}
	std::vector<int32_t> idOrder(h.nodeLookupOrder.begin(), h.nodeLookupOrder.end());   // arrival order at -t 1: nodeLookup iteration order (:354-357)
	if (idOrder.empty()) return false;
	int32_t* dOrder = uploadVector(idOrder);
	uint64_t *dKeys = nullptr, *dValues = nullptr;
	uint64_t n = gcdev::buildMinimizerPairsDevice(G->dev, dOrder, (uint32_t)idOrder.size(), (uint32_t)k, (uint32_t)w, &dKeys, &dValues);
	(void)hipFree(dOrder);
	if (n == ~0ull) { (void)hipGetLastError(); return false; }
	std::vector<uint64_t> keys(n);
	gc::MinimizerIndex& idx = S->host;
	idx = gc::MinimizerIndex();
	idx.k = k; idx.w = w;
	idx.positions.resize(n);
	if (n) {
		HIP_CHECK(hipMemcpy(keys.data(), dKeys, n * 8, hipMemcpyDeviceToHost));
		HIP_CHECK(hipMemcpy(idx.positions.data(), dValues, n * 8, hipMemcpyDeviceToHost));
		(void)hipFree(dKeys); (void)hipFree(dValues);
	}
	for (size_t i = 0; i < n; i++) {
		uint64_t kmer = keys[i] >> 34;
		if (idx.kmers.empty() || idx.kmers.back() != kmer) { idx.kmers.push_back(kmer); idx.startPos.push_back(i); }
	}
	idx.startPos.push_back(n);
	idx.maxCount = gc::minimizerMaxCount(idx.startPos, keepLeastFrequentFraction);
	return true;
}

static bool seederShapeOk(int64_t k, int64_t w) { return k >= 1 && k <= 31 && w >= k; }   // (the reference's range: src/AlignerMain.cpp:221,390)

int gc_seeder_create(const gc_graph* g, int32_t k, int32_t w, double keepFraction, gc_seeder** out)
{
	if (!g || !out) return fail(GC_ERR_INVALID, "null argument");
	if (!seederShapeOk(k, w)) return fail(GC_ERR_INVALID, "supported minimizer length is 1..31 with w >= k");
	*out = nullptr;
	gc_seeder* S = new gc_seeder();
	int rc = guarded([&]() {
		requireDevice();
		const gc::Switches sw = gc::Switches::fromEnvironment();
		if (sw.seederBuildOnHost || !buildSeederOnDevice(g, S, (size_t)k, (size_t)w, keepFraction)) S->host = gc::MinimizerIndex::Build(g->host, (size_t)k, (size_t)w, keepFraction);
		uploadSeeder(S, sw.testSeedFilterBits);
		return (int)GC_OK;
	});
	if (rc != GC_OK) { delete S; return rc; }
	*out = S;
	return GC_OK;
}

// ---- index cache (host/gc_index_cache.hpp) -----------------------------------------------
int gc_index_build(const char* gfa_path, int32_t k, int32_t w, double keepFraction, const char* cache_path)
{
	if (!gfa_path || !cache_path) return fail(GC_ERR_INVALID, "null argument");
	if (k > 0 && !seederShapeOk(k, w)) return fail(GC_ERR_INVALID, "supported minimizer length is 1..31 with w >= k");
	try {
		gc::AlignmentGraph graph = gc::AlignmentGraph::BuildFromGFAFile(gfa_path);
		graph.buildMPC(true);
		if (k > 0) {
			gc::MinimizerIndex idx = gc::MinimizerIndex::Build(graph, (size_t)k, (size_t)w, keepFraction);
			gc::SaveIndexCache(cache_path, graph, &idx);
		} else {
			gc::SaveIndexCache(cache_path, graph, nullptr);
		}
	} catch (const std::exception& e) {
		return fail(GC_ERR_GRAPH, e.what());
	}
	return GC_OK;
}

int gc_index_save(const gc_graph* g, const gc_seeder* s, const char* cache_path)
{
	if (!g || !cache_path) return fail(GC_ERR_INVALID, "null argument");
	try {
		if (g->hostMpcTrimmed) return fail(GC_ERR_INVALID, "the host copy of the MPC index was released (gc_graph_trim_host): nothing to write the cache from");
		gc::SaveIndexCache(cache_path, g->host, s ? &s->host : nullptr);
	} catch (const std::exception& e) {
		return fail(GC_ERR_GRAPH, e.what());
	}
	return GC_OK;
}

static void fillIndexInfo(const gc::IndexCacheInfo& info, uint64_t* out)
{
	if (!out) return;
	out[0] = gc::INDEX_CACHE_VERSION; out[1] = info.nodes; out[2] = info.bp; out[3] = info.hasSeeder ? 1 : 0;
	out[4] = info.k; out[5] = info.w; out[6] = info.kmers; out[7] = info.positions;
}

int gc_index_check(const char* cache_path, uint64_t* info8)
{
	if (!cache_path) return fail(GC_ERR_INVALID, "null argument");
	try {
		fillIndexInfo(gc::CheckIndexCache(cache_path), info8);
	} catch (const std::exception& e) {
		return fail(GC_ERR_GRAPH, e.what());
	}
	return GC_OK;
}

int gc_index_load(const char* cache_path, gc_graph** graph_out, gc_seeder** seeder_out)
{
	if (!cache_path || !graph_out) return fail(GC_ERR_INVALID, "null argument");
	*graph_out = nullptr;
	if (seeder_out) *seeder_out = nullptr;
	gc_graph* G = new gc_graph();
	gc_seeder* S = new gc_seeder();
	try {
		requireDevice();
		gc::IndexCacheInfo info = gc::LoadIndexCache(cache_path, G->host, S->host);
		uploadGraph(G);
		if (info.hasSeeder && seeder_out) {
			if (!seederShapeOk((int64_t)S->host.k, (int64_t)S->host.w)) throw std::runtime_error("index cache holds a minimizer index this library cannot run");
			uploadSeeder(S, gc::Switches::fromEnvironment().testSeedFilterBits);
		} else {
			delete S;
			S = nullptr;
		}
	} catch (const DeviceError& e) {
		delete G; delete S;
		return fail(GC_ERR_DEVICE, e.what());
	} catch (const std::exception& e) {
		delete G; delete S;
		return fail(GC_ERR_GRAPH, e.what());
	}
	*graph_out = G;
	if (seeder_out) *seeder_out = S;
	return GC_OK;
}

void gc_seeder_destroy(gc_seeder* s) { delete s; malloc_trim(0); }

int gc_seeder_array(const gc_seeder* s, const char* name, int64_t** out, uint64_t* count)
{
	if (!s || !name || !out || !count) return fail(GC_ERR_INVALID, "null argument");
	std::string nm = name;
	const std::vector<uint64_t>* src = nullptr;
	std::vector<uint64_t> single;
	if (nm == "kmers") src = &s->host.kmers;
	else if (nm == "start") src = &s->host.startPos;
	else if (nm == "positions") src = &s->host.positions;
	else if (nm == "maxcount") { single.push_back(s->host.maxCount); src = &single; }
	else if (nm == "k") { single.push_back((uint64_t)s->dev.k); src = &single; }
	else if (nm == "w") { single.push_back((uint64_t)s->dev.w); src = &single; }
	else return fail(GC_ERR_INVALID, "unknown seeder array " + nm);
	*out = mallocArray<int64_t>(src->size());
	for (size_t i = 0; i < src->size(); i++) (*out)[i] = (int64_t)(*src)[i];
	*count = src->size();
	return GC_OK;
}

} // extern "C"
