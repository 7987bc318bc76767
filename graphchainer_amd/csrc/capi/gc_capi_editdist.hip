// C entry points, edit distances of arbitrary string pairs: gc_edit_distance, gc_edit_path.
#include "../gc_runtime.hpp"

extern "C" {

// Global (NW) edit distances of n_pairs string pairs on the GPU: what edlibAlign(a, b, EDLIB_MODE_NW, EDLIB_TASK_DISTANCE)
// returns at src/Aligner.cpp:645,845.
int gc_edit_distance(const char* a, const uint64_t* a_off, const char* b, const uint64_t* b_off, uint64_t n_pairs, int64_t* out)
{
	if ((!a && n_pairs) || !a_off || (!b && n_pairs) || !b_off || !out) return fail(GC_ERR_INVALID, "null argument");
	return guarded([&]() {
		requireDevice();
		if (n_pairs == 0) return (int)GC_OK;
		if (n_pairs >= 0xffffffffull) throw std::runtime_error("too many pairs");
		const uint64_t aBytes = a_off[n_pairs], bBytes = b_off[n_pairs];
		std::vector<EdRead> reads(n_pairs);
		uint64_t words = 0;
		for (uint64_t i = 0; i < n_pairs; i++) {
			uint64_t len = b_off[i + 1] - b_off[i];
			if (len >= 0x7fffffffull || a_off[i + 1] - a_off[i] >= 0x7fffffffull) throw std::runtime_error("sequence too long");
			reads[i] = EdRead { b_off[i], words, (uint32_t)len, (uint32_t)((len + 63) / 64 + 1) };
			words += 4ull * reads[i].words;
		}
		std::vector<uint64_t> masks(words, 0);
		for (uint64_t i = 0; i < n_pairs; i++) buildEqMasks(b + b_off[i], reads[i].len, reads[i].words, masks.data() + reads[i].eqOff);
		const gc::Switches sw = gc::Switches::fromEnvironment();
		std::vector<EdPair> pairs(n_pairs);
		for (uint64_t i = 0; i < n_pairs; i++) {
			uint32_t m = (uint32_t)(a_off[i + 1] - a_off[i]);
			pairs[i] = EdPair { a_off[i], m, 0, (uint32_t)i, std::max<uint32_t>(64, (m + reads[i].len) / 16) };
			if (sw.edFirstK) pairs[i].k = *sw.edFirstK;   // test hook: the first band, as small as a whole-read alignment's own bound (score + clipped ends + 8)
		}
		DeviceBuffer dA, dB, dMasks, dReads, dPairs, dOut;
		char* pa = dA.reserve<char>(aBytes); char* pb = dB.reserve<char>(bBytes);
		uint64_t* pm = dMasks.reserve<uint64_t>(words);
		EdRead* pr = dReads.reserve<EdRead>(n_pairs);
		EdPair* pp = dPairs.reserve<EdPair>(n_pairs);
		int64_t* po = dOut.reserve<int64_t>(n_pairs);
		if (aBytes) HIP_CHECK(hipMemcpy(pa, a, aBytes, hipMemcpyHostToDevice));
		if (bBytes) HIP_CHECK(hipMemcpy(pb, b, bBytes, hipMemcpyHostToDevice));
		if (words) HIP_CHECK(hipMemcpy(pm, masks.data(), words * sizeof(uint64_t), hipMemcpyHostToDevice));
		HIP_CHECK(hipMemcpy(pr, reads.data(), n_pairs * sizeof(EdRead), hipMemcpyHostToDevice));
		EditDistanceRun run;
		auto readLenOf = [&](uint32_t r) { return reads[r].len; };
		launchEditDistances(run, nullptr, pairs.data(), out, (uint32_t)n_pairs, pp, po, pr, pb, pm, pa, nullptr, readLenOf, sw.debugTimes);
		finishEditDistances(run, nullptr, pairs.data(), out, (uint32_t)n_pairs, pp, po, pr, pb, pm, pa, nullptr, sw.debugTimes);
		return (int)GC_OK;
	});
}

// The alignment path edlib returns for EDLIB_TASK_PATH (src/Aligner.cpp:845), for arbitrary string pairs: k_edit_distance for the
// distance, k_edit_path for the ops. Rows = a (the reference passes the path letters first), columns = b (the read).
int gc_edit_path(const char* a, const uint64_t* a_off, const char* b, const uint64_t* b_off, uint64_t n_pairs, const uint64_t* ops_off, uint8_t* ops, uint32_t* ops_len, int64_t* distance)
{
	if ((!a && n_pairs) || !a_off || (!b && n_pairs) || !b_off || !ops_off || !ops || !ops_len || !distance) return fail(GC_ERR_INVALID, "null argument");
	int rc = gc_edit_distance(a, a_off, b, b_off, n_pairs, distance);
	if (rc != GC_OK) return rc;
	return guarded([&]() {
		if (n_pairs == 0) return (int)GC_OK;
		const uint64_t aBytes = a_off[n_pairs], bBytes = b_off[n_pairs];
		std::vector<EdPathJob> jobs(n_pairs);
		uint32_t maxQ = 1, maxT = 1;
		uint64_t opsEnd = 0;
		for (uint64_t i = 0; i < n_pairs; i++) {
			const uint32_t q = (uint32_t)(a_off[i + 1] - a_off[i]), t = (uint32_t)(b_off[i + 1] - b_off[i]);
			jobs[i] = EdPathJob { a_off[i], b_off[i], ops_off[i], q, t, (int32_t)distance[i], 0 };
			maxQ = std::max(maxQ, q); maxT = std::max(maxT, t);
			opsEnd = std::max<uint64_t>(opsEnd, ops_off[i] + q + t);
		}
		DeviceBuffer dA, dB, dJobs, dOps, dLen, dScratch;
		char* pa = dA.reserve<char>(aBytes); char* pb = dB.reserve<char>(bBytes);
		EdPathJob* pj = dJobs.reserve<EdPathJob>(n_pairs);
		uint8_t* po = dOps.reserve<uint8_t>(opsEnd);
		uint32_t* pl = dLen.reserve<uint32_t>(n_pairs);
		uint8_t* ps = dScratch.reserve<uint8_t>((uint64_t)editPathGridBlocks((uint32_t)n_pairs) * editPathScratchBytes(maxQ, maxT));
		if (aBytes) HIP_CHECK(hipMemcpy(pa, a, aBytes, hipMemcpyHostToDevice));
		if (bBytes) HIP_CHECK(hipMemcpy(pb, b, bBytes, hipMemcpyHostToDevice));
		HIP_CHECK(hipMemcpy(pj, jobs.data(), n_pairs * sizeof(EdPathJob), hipMemcpyHostToDevice));
		launchEditPath(nullptr, pj, (uint32_t)n_pairs, pa, pb, ps, maxQ, maxT, po, pl);
		HIP_CHECK(hipDeviceSynchronize());
		HIP_CHECK(hipMemcpy(ops_len, pl, n_pairs * sizeof(uint32_t), hipMemcpyDeviceToHost));
		if (opsEnd) HIP_CHECK(hipMemcpy(ops, po, opsEnd, hipMemcpyDeviceToHost));
		return (int)GC_OK;
	});
}

} // extern "C"
