// The whole-read extension launch: team size, scratch per lane, and which of the kernel's instantiations runs (one object per team size, gc_long_extend_t<N>.hip).
#include "gc_long_extend.hpp"

namespace gcdev {

uint64_t longWaveWordsPerLane(const ExtendConfig& cfg) { return waveScratchWords(cfg.maxSlices, cfg.maxItems, cfg.maxTrace, cfg.maxCols); }

uint32_t longExtendTeamSize(uint32_t nWork, uint32_t teamOverride)
{
	// Measured on MI355X (cfg2, 20k extensions in the first round): 1 lane per wave 260 ms, 2 lanes 352 ms, 4 lanes 397 ms,
	// 8 lanes 555 ms for the whole pass. The extension core is branchy serial code; lanes sharing a wave pay for the
	// union of their paths, and the chip has far more wave slots than a round has extensions. GC_TEST_LONG_TEAM overrides.
	if (teamOverride) return teamOverride;
	(void)nWork;
	return 1;
}

void launchLongExtend(hipStream_t stream, const DGraph& g, const CorrectnessTables* ct, const uint64_t* masks, const ExtendConfig& cfg, const LongWork* work, const uint32_t* order, uint32_t nWork,
	unsigned long long* scratch, uint32_t lanes, uint32_t blocks, unsigned long long* tracePool, unsigned long long* traceCursor, uint64_t traceCapacity, LongWorkResult* results, unsigned long long* counters,
	unsigned long long* nextSlot, uint32_t retryStatus, const unsigned long long* nWorkOnDevice, uint32_t* capListOut, unsigned long long* capCountOut)
{
	if (!nWork) return;
	uint64_t words = longWaveWordsPerLane(cfg);
	// fewer lanes than work items (or a count only the device knows): waves loop and fetch
	const bool persistent = nWorkOnDevice || (uint64_t)blocks * lanes < nWork;
	// the band controls (gc_params::ramp_bandwidth / max_cells_per_slice) run in their own instantiation: the default one is compiled as before
	const bool band = cfg.bandControls();
	const bool clip = cfg.clipOn();   // precise clipping / the X-drop: an instantiation of its own, with the band controls
	switch (lanes) {
		case 1: launchLongExtendTeam1(GC_LONG_EXTEND_ARGS); break;
		case 2: launchLongExtendTeam2(GC_LONG_EXTEND_ARGS); break;
		case 4: launchLongExtendTeam4(GC_LONG_EXTEND_ARGS); break;
		case 8: launchLongExtendTeam8(GC_LONG_EXTEND_ARGS); break;
		case 16: launchLongExtendTeam16(GC_LONG_EXTEND_ARGS); break;
		case 32: launchLongExtendTeam32(GC_LONG_EXTEND_ARGS); break;
		default: launchLongExtendTeam64(GC_LONG_EXTEND_ARGS); break;
	}
}

} // namespace gcdev
