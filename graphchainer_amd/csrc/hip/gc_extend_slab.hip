// The plain-layout fragment extension (K3): what the lockstep kernel of gc_extend_frag.hip declines, and everything when that one is switched off.
#include "gc_kernels.hpp"

namespace gcdev {

// =====================================================================================================
// K3 - seed extension. One lane per extension (see gc_device.hpp). A persistent grid strides over the work
// items; every lane owns a scratch slab in HBM; finished traces are appended to a shared pool.
// reference: GraphAlignerBitvectorBanded::getReverseTraceFromSeed, src/GraphAlignerBitvectorBanded.h:46-71.
// =====================================================================================================

#ifndef GC_EXTEND_RING
#define GC_EXTEND_RING 8   // columns per lane of the backtrace ring in LDS (power of two; 0: the whole tile in the lane's HBM slab, as before r4)
#endif
// 4 waves per SIMD (<= 128 VGPRs; the kernel wanted 131 and ran 3): it waits on memory 56 % of the time, so the extra wave
// pays for the 4 spilled registers: 34.2 -> 29.0 ms alone on cfg2 (5 or 6 waves spill 57 / 196 registers and lose).
#define GC_EXTEND_SLAB_PARAMS DGraph g, const CorrectnessTables* __restrict__ ct, const uint8_t* __restrict__ iupac, ExtendConfig cfg, 	const ExtItem* __restrict__ work, uint32_t nWork, const char* __restrict__ bases, ExtResult* __restrict__ results, 	uint8_t* __restrict__ scratch, uint64_t slabBytes, PoolCell* __restrict__ tracePool, unsigned long long* __restrict__ traceCursor, uint64_t traceCapacity, 	unsigned long long* __restrict__ counters, uint32_t retryStatus, ExtSelection sel
template <bool BAND, bool CLIP = false>
__device__ __forceinline__ void extendSlabBody(GC_EXTEND_SLAB_PARAMS)
{
#if defined(GC_EXTEND_PRIO) && GC_EXTEND_PRIO
	__builtin_amdgcn_s_setprio(GC_EXTEND_PRIO);   // (experiment, -DGC_EXTEND_PRIO=3: the fragment extension's waves ahead of the whole-read kernel's - 149.9 / 149.2 / 152.3 ms per batch against 154.0 / 147.2 / 151.6, `gpurun_out/r4_extprio`: no effect, off)
#endif
	const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t stride = gridDim.x * blockDim.x;
	LaneScratch sc = laneScratch(scratch + (uint64_t)tid * slabBytes, cfg);
#if GC_EXTEND_RING
	// r4: the backtrace's recomputed columns in LDS - a ring of the last GC_EXTEND_RING columns per lane, lane-interleaved - instead of 64 columns in the lane's HBM slab
	__shared__ WCol columnRing[GC_EXTEND_RING * 64];
	sc.columns = columnRing + threadIdx.x;
	sc.colMask = GC_EXTEND_RING - 1; sc.colStride = 64;
#endif
	ExtCounters cnt {};
	// which work items: all of them, the two extensions of every fragment's first seed, or a list written by k_build_anchors (count on the device)
	const uint32_t nSelected = sel.mode == 0 ? nWork : sel.mode == 1 ? 2 * sel.nFrags : (uint32_t)*sel.listCount;
	for (uint32_t at = tid; at < nSelected; at += stride) {
		const uint32_t w = sel.mode == 0 ? at : sel.mode == 1 ? 2 * sel.frags[at >> 1].seedBegin + (at & 1u) : sel.list[at];
		if (retryStatus != 0 && results[w].status != retryStatus) continue;   // retry launch (larger slabs): only the items the first launch gave up on
		ExtItem it = work[w];
		uint32_t nTrace = 0;
		int32_t score = 0;
		uint32_t status = extendSeed<BAND, CLIP>(g, *ct, iupac, cfg, sc, bases + it.seqOff, (int)it.seqLen, it.node, it.offset, nTrace, score, cnt);
		ExtResult res;
		res.status = status;
		res.score = score;
		res.traceLen = 0;
		res.traceOff = 0;
		res.pad = cnt.flattenTie;   // r5: the extension's last-slice minimum was attained in more than one node (k_build_anchors sums what the reference would have run, per read)
		if (status == EXT_OK) {
			unsigned long long base = atomicAdd(traceCursor, (unsigned long long)nTrace);
			if (base + nTrace <= traceCapacity) {
				for (uint32_t i = 0; i < nTrace; i++) { const TraceCell c = sc.trace[i]; tracePool[base + i] = PoolCell { c.node, (uint16_t)c.offsetAndSwitch, (int16_t)c.seqPos }; }
				res.traceOff = base;
				res.traceLen = nTrace;
			} else {
				res.status = EXT_OVERFLOW;
			}
		}
		results[w] = res;
	}
	// one set of atomics per lane that did work
	if (cnt.extensions) {
		atomicAdd(&counters[0], cnt.dpTiles);
		atomicAdd(&counters[1], cnt.recomputeTiles);
		atomicAdd(&counters[2], cnt.columnSteps);
		atomicAdd(&counters[3], cnt.traceItems);
		atomicAdd(&counters[4], cnt.extensions);
		atomicAdd(&counters[5], cnt.backtraceTiles);
	}
}

// 4 waves per SIMD (<= 128 VGPRs): everything, when the lockstep kernel is switched off (GC_EXTEND_SLAB=1)
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 8))) k_extend_slab(GC_EXTEND_SLAB_PARAMS)
{
	extendSlabBody<false>(g, ct, iupac, cfg, work, nWork, bases, results, scratch, slabBytes, tracePool, traceCursor, traceCapacity, counters, retryStatus, sel);
}
// the same with the band controls (gc_params::ramp_bandwidth / max_cells_per_slice): the fragments whose slice reaches the cell limit, which k_extend declines
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 8))) k_extend_slab_band(GC_EXTEND_SLAB_PARAMS)
{
	extendSlabBody<true>(g, ct, iupac, cfg, work, nWork, bases, results, scratch, slabBytes, tracePool, traceCursor, traceCapacity, counters, retryStatus, sel);
}
// the same with precise clipping / the X-drop (gc_params_ext): every fragment extension of a clipped batch - the lockstep kernel does not clip
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 8))) k_extend_slab_clip(GC_EXTEND_SLAB_PARAMS)
{
	extendSlabBody<true, true>(g, ct, iupac, cfg, work, nWork, bases, results, scratch, slabBytes, tracePool, traceCursor, traceCapacity, counters, retryStatus, sel);
}

// =====================================================================================================
// launchers
// =====================================================================================================

uint64_t extendSlabBytes(const ExtendConfig& cfg)
{
	uint64_t b = sizeof(SliceInfo) * (uint64_t)cfg.maxSlices + sizeof(NodeItem) * (uint64_t)cfg.maxItems + sizeof(Pending) * (uint64_t)cfg.maxPending + sizeof(WCol) * 64 + sizeof(TraceCell) * (uint64_t)cfg.maxTrace + sizeof(uint32_t) * (uint64_t)cfg.maxItems;
	return (b + 63) & ~63ull;
}

uint32_t extendGridLanes(uint32_t nWork)
{
	// 256 CUs x 16 resident waves is plenty to hide latency for this register-heavy kernel; never more lanes than work
	uint32_t lanes = 256u * 16u * 64u;
	uint32_t need = (nWork + 63) / 64 * 64;
	return need < lanes ? need : lanes;
}

void launchExtend(hipStream_t stream, const DGraph& g, const CorrectnessTables* ct, const uint8_t* iupac, const ExtendConfig& cfg,
	const ExtItem* work, uint32_t nWork, const char* bases, ExtResult* results, uint8_t* scratch, uint64_t slabBytes,
	PoolCell* tracePool, unsigned long long* traceCursor, uint64_t traceCapacity, unsigned long long* counters, uint32_t retryStatus, uint32_t retryLanes, ExtSelection sel)
{
	if (nWork == 0) return;
	const uint32_t upper = sel.mode == 1 ? 2 * sel.nFrags : nWork;   // (a device-side list holds at most nWork items; waves beyond its count leave at once)
	uint32_t lanes = retryStatus ? retryLanes : extendGridLanes(upper);
	if (cfg.clipOn()) hipLaunchKernelGGL(k_extend_slab_clip, dim3(lanes / 64), dim3(64), 0, stream, g, ct, iupac, cfg, work, nWork, bases, results, scratch, slabBytes, tracePool, traceCursor, traceCapacity, counters, retryStatus, sel);
	else if (cfg.bandControls()) hipLaunchKernelGGL(k_extend_slab_band, dim3(lanes / 64), dim3(64), 0, stream, g, ct, iupac, cfg, work, nWork, bases, results, scratch, slabBytes, tracePool, traceCursor, traceCapacity, counters, retryStatus, sel);
	else hipLaunchKernelGGL(k_extend_slab, dim3(lanes / 64), dim3(64), 0, stream, g, ct, iupac, cfg, work, nWork, bases, results, scratch, slabBytes, tracePool, traceCursor, traceCapacity, counters, retryStatus, sel);
}

// test entry (gc_test_max_x_score): one column per thread through the extension core's column maximum
__global__ void __launch_bounds__(64) k_test_max_x_score(const uint64_t* __restrict__ vp, const uint64_t* __restrict__ vn, const int32_t* __restrict__ scoreEnd, uint32_t n, double errorCost, int cells, int32_t* __restrict__ out)
{
	const uint32_t i = blockIdx.x * 64 + threadIdx.x;
	if (i < n) out[i] = clipMaxXScore(WS { vp[i], vn[i], scoreEnd[i] }, errorCost, cells);
}
void launchTestMaxXScore(hipStream_t stream, const uint64_t* vp, const uint64_t* vn, const int32_t* scoreEnd, uint32_t n, double errorCost, int cells, int32_t* out)
{
	if (n) hipLaunchKernelGGL(k_test_max_x_score, dim3((n + 63) / 64), dim3(64), 0, stream, vp, vn, scoreEnd, n, errorCost, cells, out);
}

} // namespace gcdev
