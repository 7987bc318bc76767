// C entry points, the library's own housekeeping: gc_last_error, gc_free, gc_device_count, gc_device_memory, gc_set_device, gc_params_default, gc_params_ext_default,
// gc_stream_create / _destroy, gc_result_free, gc_result_cache_trim, gc_evalue, and the test entries gc_std_sort_permutations and gc_test_max_x_score.
#include "../gc_runtime.hpp"

extern "C" {

const char* gc_last_error(void) { return g_lastError.c_str(); }
void gc_free(void* p) { free(p); }

// E-value model of --E-cutoff (host only): out2 = {alignment score, E-value}; what SelectECutoff compares with the cut-off
// (src/AlignmentSelection.cpp:91-99, src/EValue.cpp:35-48).
int gc_evalue(double min_identity, uint64_t database_size, uint64_t query_size, uint64_t alignment_length, uint64_t num_edits, double* out2)
{
	if (!out2) return fail(GC_ERR_INVALID, "null argument");
	gc::EValueModel model(min_identity);
	out2[0] = model.alignmentScore(alignment_length, num_edits);
	out2[1] = model.evalue(database_size, query_size, alignment_length, num_edits);
	return GC_OK;
}

// gc_result_free keeps the large arrays of freed results (up to 24 GB) for the next batch instead of returning them to the allocator; this returns them.
void gc_result_cache_trim(void)
{
	g_resultBlocks.trim();
	// r5: the device / pinned blocks held back by gc_reads_destroy and by the device deflate's staging as well (blocks in use are not in the caches and are unaffected)
	g_readDeviceBlocks.trim(); g_readPinnedBlocks.trim(); g_deflateDeviceBlocks.trim(); g_deflatePinnedBlocks.trim();
}

// Test entry: the permutation the device's replay of libstdc++'s std::sort (hip/gc_stdsort_wave.hpp, what k_seed_glue runs for the reference's three order-critical unstable sorts)
// gives for arrays of 32-bit keys: array s = keys[offsets[s] .. offsets[s + 1]), perm_out likewise - perm_out[offsets[s] + i] = the index (inside its array) of the element
// that ends at place i. depth_limit < 0: the reference's 2 floor(log2 n); smaller values force the heapsort path.
int gc_std_sort_permutations(const uint32_t* keys, const uint64_t* offsets, uint64_t n_arrays, int64_t depth_limit, uint32_t* perm_out)
{
	if (!offsets || !perm_out || (!keys && n_arrays && offsets[n_arrays] > 0)) return fail(GC_ERR_INVALID, "null argument");
	return guarded([&]() {
		requireDevice();
		const uint64_t total = offsets[n_arrays];
		if (n_arrays >= 0xffffffffull) throw std::runtime_error("too many arrays");
		std::vector<unsigned long long> elems(total);
		for (uint64_t s = 0; s < n_arrays; s++) {
			if (offsets[s + 1] < offsets[s] || offsets[s + 1] - offsets[s] >= 0xffffffffull) throw std::runtime_error("bad offsets");
			for (uint64_t i = offsets[s]; i < offsets[s + 1]; i++) elems[i] = ((unsigned long long)keys[i] << 32) | (i - offsets[s]);
		}
		DeviceBuffer dElems, dOff, dScratch;
		unsigned long long* de = dElems.reserve<unsigned long long>(total);
		uint64_t* dof = dOff.reserve<uint64_t>(n_arrays + 1);
		uint32_t* ds = dScratch.reserve<uint32_t>(3 * total + 64 * n_arrays + 64);
		if (total) HIP_CHECK(hipMemcpy(de, elems.data(), total * sizeof(unsigned long long), hipMemcpyHostToDevice));
		HIP_CHECK(hipMemcpy(dof, offsets, (n_arrays + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
		launchTestStdSort(nullptr, de, dof, (uint32_t)n_arrays, ds, (long)depth_limit);
		HIP_CHECK(hipDeviceSynchronize());
		if (total) HIP_CHECK(hipMemcpy(elems.data(), de, total * sizeof(unsigned long long), hipMemcpyDeviceToHost));
		for (uint64_t i = 0; i < total; i++) perm_out[i] = (uint32_t)elems[i];
		return (int)GC_OK;
	});
}

// Test entry: the plain-layout kernel's column maximum (clipMaxXScore, hip/gc_device.hpp) on the caller's columns
int gc_test_max_x_score(const uint64_t* vp, const uint64_t* vn, const int32_t* score_end, uint64_t n, double error_cost, int32_t cells, int32_t* out)
{
	if (!out || ((!vp || !vn || !score_end) && n)) return fail(GC_ERR_INVALID, "null argument");
	if (cells < 1 || cells > 64 || n >= 0xffffffffull) return fail(GC_ERR_INVALID, "gc_test_max_x_score: cells must be in [1, 64]");
	return guarded([&]() {
		requireDevice();
		if (!n) return (int)GC_OK;
		DeviceBuffer dVp, dVn, dScore, dOut;
		uint64_t* a = dVp.reserve<uint64_t>(n); uint64_t* b = dVn.reserve<uint64_t>(n);
		int32_t* c = dScore.reserve<int32_t>(n); int32_t* o = dOut.reserve<int32_t>(n);
		HIP_CHECK(hipMemcpy(a, vp, n * sizeof(uint64_t), hipMemcpyHostToDevice));
		HIP_CHECK(hipMemcpy(b, vn, n * sizeof(uint64_t), hipMemcpyHostToDevice));
		HIP_CHECK(hipMemcpy(c, score_end, n * sizeof(int32_t), hipMemcpyHostToDevice));
		launchTestMaxXScore(nullptr, a, b, c, (uint32_t)n, error_cost, cells, o);
		HIP_CHECK(hipDeviceSynchronize());
		HIP_CHECK(hipMemcpy(out, o, n * sizeof(int32_t), hipMemcpyDeviceToHost));
		return (int)GC_OK;
	});
}

int gc_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

// free and total bytes of the current device's memory (hipMemGetInfo): what a host sizing its batches - or a benchmark reporting its peak - needs
int gc_device_memory(uint64_t* free_bytes, uint64_t* total_bytes)
{
	if (!free_bytes || !total_bytes) return fail(GC_ERR_INVALID, "null argument");
	return guarded([&]() {
		requireDevice();
		size_t f = 0, t = 0;
		HIP_CHECK(hipMemGetInfo(&f, &t));
		*free_bytes = f; *total_bytes = t;
		return (int)GC_OK;
	});
}

int gc_set_device(int device)
{
	return guarded([&]() { HIP_CHECK(hipSetDevice(device)); return (int)GC_OK; });
}

// fast_mode took the struct's tail padding: the other fields are where they were and the size is what it was
static_assert(sizeof(gc_params) == 216 && offsetof(gc_params, fast_mode) == offsetof(gc_params, selection_method) + 4 && offsetof(gc_params, fast_mode) + 4 == sizeof(gc_params), "gc_params layout");

static_assert(sizeof(gc_params_ext) == 16 && offsetof(gc_params_ext, precise_clipping) == 8, "gc_params_ext layout");
void gc_params_ext_default(gc_params_ext* e)
{
	if (!e) return;
	e->struct_size = (uint32_t)sizeof(gc_params_ext);
	e->x_drop = 0;               // off (src/AlignerMain.cpp: Xdropcutoff 0)
	e->precise_clipping = 0.0;   // off
}

void gc_params_default(gc_params* p)
{
	if (!p) return;
	p->bandwidth = 10;
	p->split_len = 35;
	p->split_gap = 35;
	p->colinear_gap = 10000;
	p->seed_density = 10;
	p->min_cluster_size = 1;
	p->long_pass = 0;
	p->keep_traces = 0;
	p->keep_seeds = 0;
	p->stitch = 1;
	p->edit_distances = 1;
	p->chain_traces = 1;
	p->device_output = 0;
	p->e_cutoff = -1;
	memset(&p->capacity, 0, sizeof(p->capacity));   // automatic
	p->ramp_bandwidth = 0;          // off (src/AlignerMain.cpp:147)
	p->max_cells_per_slice = -1;    // unlimited (src/AlignerMain.cpp:149: SIZE_MAX)
	p->force_global = 0;            // off (src/AlignerMain.cpp:160)
	p->seed_extend_density = -1;    // all seeds (chaining mode: tryAllSeeds, src/AlignerMain.cpp:204,449-453)
	p->extra_heuristic = 0;         // off (src/AlignerMain.cpp:170,192)
	p->colinear_chaining = 1;       // on; 0 is --no-colinear-chaining (src/AlignerMain.cpp:176,198-199)
	p->selection_method = GC_SELECT_GREEDY_LENGTH;
	p->fast_mode = 0;               // off (src/AlignerMain.cpp:180,195-196)
}

int gc_stream_create(gc_stream** out)
{
	if (!out) return fail(GC_ERR_INVALID, "null argument");
	*out = nullptr;
	gc_stream* st = new gc_stream();
	int rc = guarded([&]() {
		requireDevice();
		HIP_CHECK(hipGetDevice(&st->device));
		if (st->device < 0 || st->device >= 16) throw std::runtime_error("gc_stream_create: device index beyond the 16 per-device slots of the whole-read token and scratch");
		createStream(&st->stream);       // non-blocking: uploads of another batch on the null stream do not serialise with this one
		createStream(&st->longPass.longStream);
		for (auto& e : st->ev) HIP_CHECK(hipEventCreate(&e));
		for (auto& e : st->fragEv) HIP_CHECK(hipEventCreate(&e));
		return (int)GC_OK;
	});
	if (rc != GC_OK) { delete st; return rc; }
	{ std::lock_guard<std::mutex> lock(g_longScratchCount); noteHardwareQueues(++g_longScratch[st->device & 15].streams); }
	*out = st;
	return GC_OK;
}
void gc_stream_destroy(gc_stream* st)
{
	if (!st) return;
	{
		std::lock_guard<std::mutex> count(g_longScratchCount);
		SharedLongScratch& shared = g_longScratch[st->device & 15];
		if (--shared.streams == 0) {   // the device's last stream: nobody can hold the token any more
			TokenHold alone;
			alone.lock(g_longPassToken[st->device & 15], 1, true);   // (every slot free and nobody beside: as a pass that fills the chip waits)
			int current = 0;
			if (hipGetDevice(&current) == hipSuccess) { (void)hipSetDevice(st->device); for (auto& b : shared.buffer) b.release(); for (auto& r : shared.rounds) r.release(); (void)hipSetDevice(current); }
		}
	}
	delete st;
}

void gc_result_free(gc_result* r)
{
	if (!r) return;
	void* ptrs[] = { r->read_seed_off, r->seed_node, r->seed_offset, r->seed_seqpos, r->seed_goodness, r->read_anchor_off, r->anchor_x, r->anchor_y, r->anchor_path_off,
		r->anchor_path, r->anchor_first_node, r->anchor_first_offset, r->anchor_first_seqpos, r->anchor_last_node, r->anchor_last_offset, r->anchor_last_seqpos, r->anchor_score,
		r->anchor_trace_off, r->anchor_trace_node, r->anchor_trace_offset, r->anchor_trace_seqpos, r->anchor_trace_switch, r->read_chain_off, r->chain, r->chain_score,
		r->read_longall_off, r->longall_start, r->longall_end, r->longall_score, r->long_trace_off, r->long_trace_node, r->long_trace_offset, r->long_trace_seqpos, r->long_trace_switch,
		r->failed_assertion, r->seeds_extended, r->seeds_extended_long, r->read_path_off, r->path_node, r->path_first_offset, r->path_last_offset, r->path_cells,
		r->read_long_off, r->long_index, r->long_edit_distance, r->chain_edit_distance, r->chained_better,
		r->capacity_exceeded, r->read_chain_trace_off, r->chain_trace_node, r->chain_trace_offset, r->chain_trace_seqpos, r->chain_trace_switch, r->chain_aln_start, r->chain_aln_end,
		r->read_out_off, r->out_source, r->out_numbers, r->out_path_off, r->out_path_text, r->out_cigar_off, r->out_cigar_text, r->out_vg_off, r->out_vg_path, r->flatten_ties, r->flatten_ties_long,
		r->out_corrected_off, r->out_corrected_text };
	for (void* p : ptrs) g_resultBlocks.put(p);
	free(r);
}

} // extern "C"
