// The whole-read extension kernel k_long_extend and the launcher of one team size. Private to gc_long_extend.hip (which picks the team size's launcher) and to
// gc_long_extend_t<N>.hip (one object per team size, six instantiations each: the kernel is most of the library's compile time, so the seven build side by side).
#pragma once
#include "gc_kernels.hpp"
#include "gc_device_wave.hpp"

namespace gcdev {

// LANES = active lanes per wave ("team"). The pass is latency-bound and leaves most of the chip idle, so when there
// are fewer work items than the chip has SIMDs x 64 lanes, running fewer lanes per wave shortens every wave: a wave's
// instruction stream is the union of its lanes' divergent paths, and LDS per wave shrinks so more waves fit per CU.
#ifndef GC_LONG_MIN_WAVES
#define GC_LONG_MIN_WAVES 1
#endif
template <int LANES, bool PERSISTENT, bool BAND = false, bool CLIP = false>   // BAND: the band controls of cfg (extendSeedWave<.., true>); CLIP: precise clipping / the X-drop (extendSeedWave<.., true, true>)
#ifndef GC_LONG_WAVES_ONE
#define GC_LONG_WAVES_ONE 5   // waves per SIMD the one-extension-per-wave instantiation is compiled for. 8: 64 VGPRs, 35 of them spilled to 112 B of scratch per lane; 7: 72 / 80 B; 6: 80 / 48 B;
                              // 5 (and 4): 87 VGPRs, no scratch. The kernel is bound by the CU's scalar unit, not by latency: all five measure the same, so the build without scratch is kept
#endif
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(LANES == 1 ? GC_LONG_WAVES_ONE : GC_LONG_MIN_WAVES, 8))) k_long_extend(DGraph g, const CorrectnessTables* __restrict__ ct, const uint64_t* __restrict__ masks, ExtendConfig cfg,
	const LongWork* __restrict__ work, const uint32_t* __restrict__ order, uint32_t nWork, unsigned long long* __restrict__ scratch, uint64_t wordsPerLane,
	unsigned long long* __restrict__ tracePool, unsigned long long* __restrict__ traceCursor, uint64_t traceCapacity, LongWorkResult* __restrict__ results, unsigned long long* __restrict__ counters,
	unsigned long long* __restrict__ nextSlot, uint32_t retryStatus, const unsigned long long* __restrict__ nWorkOnDevice, uint32_t* __restrict__ capListOut, unsigned long long* __restrict__ capCountOut)
{
	__shared__ WaveLdsT<LANES> lds;
	if (nWorkOnDevice) nWork = (uint32_t)*nWorkOnDevice;   // (the retry launch: its items are a list another kernel has just written)
	// One extension per wave (LANES == 1): all 64 lanes stay alive and run the same code on the same values - nothing depends
	// on the lane id, so the compiler keeps the extension's state in scalar registers - and the lanes' VGPRs hold the 64
	// backtrace columns. Stores hit one address with one value; atomics and the result record go through lane 0 only.
	if (LANES > 1 && threadIdx.x >= LANES) return;
	const uint32_t lane = LANES == 1 ? 0u : threadIdx.x;
	const bool leader = LANES > 1 || threadIdx.x == 0;
	WaveScratch wsx;
	wsx.base = scratch + (uint64_t)blockIdx.x * wordsPerLane * LANES;
	wsx.lane = lane;
	wsx.lanes = LANES;
	wsx.maxSlices = cfg.maxSlices; wsx.maxItems = cfg.maxItems; wsx.maxTrace = cfg.maxTrace;
	wsx.maxCols = LANES == 1 ? cfg.maxCols : 0;   // (the column store is laid out for one extension per wave; the region is reserved for every team size)
	wsx.allLanes = LANES == 1;
	wsx.regCap = cfg.regCap;
	ExtCounters cnt {};
	// One work item per wave while the launch fits the scratch (the host sizes it for up to 65536 lanes in flight under a memory budget); larger rounds run
	// persistent waves that fetch work items in execution order (longest first). The two are separate instantiations:
	// the fetch loop costs the common case 6 % (265 vs 283 ms on cfg2) in register pressure.
	bool done = false;
	while (true) {
		unsigned long long first = 0;
		if (!PERSISTENT) { if (done) break; done = true; first = (unsigned long long)blockIdx.x * LANES; }
		else {
			if (threadIdx.x == 0) first = atomicAdd(nextSlot, (unsigned long long)LANES);
			if (LANES > 1) first = __shfl(first, 0);
			else first = (unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)first) | ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(first >> 32)) << 32);   // an atomic's result is per-lane to the compiler: say it is uniform so the extension state stays in scalar registers
		}
		if (first >= nWork) break;
		const uint32_t slot = (uint32_t)first + lane;
		if (slot >= nWork) break;
		const uint32_t w = order[slot];   // execution order (longest first / length-balanced waves), results stay indexed by work item
		if (retryStatus != 0 && results[w].status != retryStatus) { if (PERSISTENT) continue; else break; }   // retry launch: only the items the first launch gave up on
		LongWork it = work[w];
		LongWorkResult res { 0, 0, EXT_FAILED, 0, 0 };
		if (it.seqLen > 0) {
			uint32_t nTrace = 0;
			int32_t score = 0;
			EqSource eqSrc { masks + it.maskOff, it.maskWords, it.startBit };
			if (CLIP) res.status = extendSeedWave<LANES == 1, true, true>(g, *ct, eqSrc, cfg.bandwidth, (lds_u32*)&lds.w[0][0], wsx, (int)it.seqLen, it.node, it.offset, 0, nTrace, score, cnt,
				cfg.rampBandwidth, cfg.maxCells, cfg.forceGlobal != 0, cfg.clipErrorCost(), cfg.xDrop);
			else if (BAND) res.status = extendSeedWave<LANES == 1, true>(g, *ct, eqSrc, cfg.bandwidth, (lds_u32*)&lds.w[0][0], wsx, (int)it.seqLen, it.node, it.offset, 0, nTrace, score, cnt,
				cfg.rampBandwidth, cfg.maxCells, cfg.forceGlobal != 0);
			else res.status = extendSeedWave<LANES == 1>(g, *ct, eqSrc, cfg.bandwidth, (lds_u32*)&lds.w[0][0], wsx, (int)it.seqLen, it.node, it.offset, 0, nTrace, score, cnt);
			res.score = score;
			res.pad = cnt.flattenTie;   // (k_long_merge adds the flags of the extensions the reference would have run to the read's count)
			if (res.status == EXT_OK) {
				unsigned long long base = 0;
				if (leader) base = atomicAdd(traceCursor, (unsigned long long)nTrace);
				if (LANES == 1) base = (unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)base) | ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(base >> 32)) << 32);
				if (base + nTrace <= traceCapacity) {
					if (LANES == 1) { for (uint32_t i = threadIdx.x; i < nTrace; i += 64) tracePool[base + i] = wsx.word(wsx.traceBase(i, 0)); }
					else for (uint32_t i = 0; i < nTrace; i++) tracePool[base + i] = wsx.word(wsx.traceBase(i, 0));
					res.traceOff = base;
					res.traceLen = nTrace;
				} else res.status = EXT_OVERFLOW;
			}
		}
		if (leader) results[w] = res;
		// (the work items whose band outgrew this layout's tables go on the list of the retry launch: almost always none - the list saves a kernel
		// that looked at every result, and the retry is a handful of waves)
		if (leader && capListOut && res.status == EXT_LDS_CAP) capListOut[atomicAdd(capCountOut, 1ull)] = w;
	}
	if (cnt.extensions && leader) {
		atomicAdd(&counters[0], cnt.dpTiles);
		atomicAdd(&counters[1], cnt.recomputeTiles);
		atomicAdd(&counters[2], cnt.columnSteps);
		atomicAdd(&counters[3], cnt.traceItems);
		atomicAdd(&counters[4], cnt.extensions);
		atomicAdd(&counters[5], cnt.backtraceTiles);
#ifdef GC_STAMPS
		for (int i = 0; i < 16; i++) atomicAdd(&counters[8 + i], cnt.cyc[i]);
#endif
	}
}

// what launchLongExtend passes on: its own arguments with the scratch words per lane worked out and the instantiation chosen
#define GC_LONG_EXTEND_PARAMS hipStream_t stream, const DGraph& g, const CorrectnessTables* ct, const uint64_t* masks, const ExtendConfig& cfg, const LongWork* work, const uint32_t* order, uint32_t nWork, \
	unsigned long long* scratch, uint64_t words, uint32_t blocks, unsigned long long* tracePool, unsigned long long* traceCursor, uint64_t traceCapacity, LongWorkResult* results, unsigned long long* counters, \
	unsigned long long* nextSlot, uint32_t retryStatus, const unsigned long long* nWorkOnDevice, uint32_t* capListOut, unsigned long long* capCountOut, bool persistent, bool band, bool clip
#define GC_LONG_EXTEND_ARGS stream, g, ct, masks, cfg, work, order, nWork, scratch, words, blocks, tracePool, traceCursor, traceCapacity, results, counters, nextSlot, retryStatus, nWorkOnDevice, capListOut, capCountOut, persistent, band, clip
#define GC_LAUNCH_ONE(N, P, B, C) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_long_extend<N, P, B, C>), dim3(blocks), dim3(64), 0, stream, g, ct, masks, cfg, work, order, nWork, scratch, words, tracePool, traceCursor, traceCapacity, results, counters, nextSlot, retryStatus, nWorkOnDevice, capListOut, capCountOut)
#define GC_LAUNCH_TEAM(N) do { if (clip) { if (persistent) GC_LAUNCH_ONE(N, true, true, true); else GC_LAUNCH_ONE(N, false, true, true); } \
	else if (band) { if (persistent) GC_LAUNCH_ONE(N, true, true, false); else GC_LAUNCH_ONE(N, false, true, false); } \
	else if (persistent) GC_LAUNCH_ONE(N, true, false, false); else GC_LAUNCH_ONE(N, false, false, false); } while (0)
// a team size's object: GC_LONG_EXTEND_TEAM(N) is all that gc_long_extend_t<N>.hip holds
#define GC_LONG_EXTEND_TEAM(N) namespace gcdev { void launchLongExtendTeam##N(GC_LONG_EXTEND_PARAMS) { GC_LAUNCH_TEAM(N); } }
void launchLongExtendTeam1(GC_LONG_EXTEND_PARAMS);
void launchLongExtendTeam2(GC_LONG_EXTEND_PARAMS);
void launchLongExtendTeam4(GC_LONG_EXTEND_PARAMS);
void launchLongExtendTeam8(GC_LONG_EXTEND_PARAMS);
void launchLongExtendTeam16(GC_LONG_EXTEND_PARAMS);
void launchLongExtendTeam32(GC_LONG_EXTEND_PARAMS);
void launchLongExtendTeam64(GC_LONG_EXTEND_PARAMS);

} // namespace gcdev
