// BGZF blocks to text on the device (gc_bgzf_inflate, gc_reads_parse_bgzf): the kernel around gc_inflate_core.hpp. One wavefront per BGZF block, one wavefront per
// workgroup. A deflate stream is serial - the place of every symbol follows from the one before it - so a wave has one decoder, and all 64 lanes run it: every value of
// the decode loop (the bit buffer, the tables in LDS, the symbol, the output position) is the same in all lanes, the branches are taken by the whole wave, a load of the
// compressed data is one address for the wave and an LDS read is a broadcast. Nothing is handed from lane to lane; what the lanes share out is the work that is not
// serial: a match of `len` bytes is copied by min(len, 64) lanes at once (its source lies wholly before the write position, so an overlapping copy reads
// out[pos - dist + k mod dist]), a stored block likewise, and the CRC-32 is taken by 64 slices and combined (infCrcLane). Literals are stored by lane 0.
// The text is read back by the wave that wrote it (match sources, the CRC): vector memory operations of one wave complete in order on this chip, and the wave-scope
// fences keep the compiler from moving a load over the stores before it.
// 4.5 KB of LDS per wave (the tables and the CRC table), so a CU holds its full complement of waves; a file of 3 200 blocks is one launch of 3 200 waves.
#include <hip/hip_runtime.h>
#include "gc_inflate_core.hpp"

namespace gcdev {

namespace {

struct InfWaveSink {
	uint8_t* out;          // the block's text (not __restrict__: it is read back)
	uint32_t lane;
	__device__ __forceinline__ void lit(uint32_t pos, uint8_t v) { if (lane == 0) out[pos] = v; }
	__device__ __forceinline__ void copy(uint32_t pos, uint32_t len, uint32_t dist)
	{
		__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
		const uint8_t* src = out + pos - dist;
		for (uint32_t k = lane; k < len; k += INF_LANES) out[pos + k] = src[k < dist ? k : k % dist];
		__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
	}
	__device__ __forceinline__ void stored(uint32_t pos, const uint8_t* src, uint32_t n)
	{
		for (uint32_t k = lane; k < n; k += INF_LANES) out[pos + k] = src[k];
	}
};

static_assert(INF_LANES == 64, "one wave per workgroup: the tables in LDS are built by all lanes in lockstep (gc_inflate_core.hpp)");
// launched with INF_LANES threads per workgroup and no more: see INF_LANES for why a second wave must not share `tables`
__global__ void __launch_bounds__(INF_LANES) k_bgzf_inflate(const uint8_t* __restrict__ data, const InfBlock* __restrict__ blocks, uint32_t nBlocks, uint8_t* out, uint32_t* __restrict__ status)
{
	__shared__ InfTables tables;
	__shared__ uint32_t crcTable[256];
	const uint32_t blk = blockIdx.x, lane = threadIdx.x;
	if (blk >= nBlocks) return;
	for (uint32_t i = lane; i < 256; i += INF_LANES) crcTable[i] = infCrcTableEntry(i);
	__syncthreads();
	const InfBlock b = blocks[blk];
	uint8_t* text = out + b.outOff;
	InfWaveSink sink { text, lane };
	uint32_t st = infBlock(data + b.inOff, b.inLen, b.isize, tables, sink);
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
	if (st == INF_OK) {
		uint32_t crc = infCrcLane(crcTable, text, b.isize, lane, INF_LANES);
		for (int d = 32; d; d >>= 1) crc ^= __shfl_xor(crc, d);
		if (crc != b.crc) st = INF_CRC;
	}
	if (lane == 0) status[blk] = st;
}

} // namespace

// blocks [nBlocks] rows on the device; the caller has checked inOff + inLen against the compressed piece, outOff + isize against the output and isize against INF_MAX_ISIZE
hipError_t infLaunch(hipStream_t q, const uint8_t* data, const InfBlock* blocks, uint32_t nBlocks, uint8_t* out, uint32_t* status)
{
	if (!nBlocks) return hipSuccess;
	hipLaunchKernelGGL(k_bgzf_inflate, dim3(nBlocks), dim3(INF_LANES), 0, q, data, blocks, nBlocks, out, status);
	return hipGetLastError();
}

} // namespace gcdev
