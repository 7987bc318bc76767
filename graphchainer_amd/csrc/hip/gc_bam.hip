// Unaligned BAM to a read batch on the device (gc_reads_parse_bam, gc_reads_parse_bam_bgzf): the kernels around gc_bam_core.hpp, which says what a record becomes. The
// inflated bytes of one chunk lie in HBM (on the BGZF path they exist nowhere else).
//   k_bam_walk     block_size is a chain, so one wave follows it: all 64 lanes run bamWalk with the same values (as the inflater's lanes run one decoder), reading through
//                  a 16 KB window in LDS that the lanes refill together with 16-byte loads whenever the next word lies outside it - a record longer than the window
//                  costs one refill, not a pass over its bytes. Lane 0 writes the record starts. The same walk steps over the file header.
//   k_bam_fields   one lane per record: bamFields' checks (an atomic minimum keeps the first record refused, as k_sf_decode does), the keep flag, l_seq and the name's
//                  length for the three hipCUB scans, and the record's spans
//   k_bam_compact  the kept records' spans, read offsets and id offsets behind the scans, and the counts
//   k_bam_names    the ids with their NUL, 8 lanes per record (k_sf_names' shape)
//   k_bam_unpack   one thread per 16 letters of the compacted reads (bamUnpackSpan), stored as one 128-bit word
// Everything but the walk is memory-bound with a few registers per thread; the walk is bound by the latency of one LDS read per record and one refill per 16 KB.
#include <hip/hip_runtime.h>
#include "gc_bam_core.hpp"
#include <hipcub/hipcub.hpp>

namespace gcdev {

namespace {

#define BAM_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

inline uint32_t bamBlocks(uint64_t items) { return (uint32_t)((items + BAM_BLOCK - 1) / BAM_BLOCK); }

// the walk's Reader: `at` is the same in every lane, so the refill is taken by the whole wave
struct BamWindowReader {
	const uint8_t* text;
	uint32_t padded;       // the bytes rounded up to 16: the text's block reaches that far
	uint8_t* window;       // [BAM_WINDOW] LDS
	uint32_t lane, base;
	bool filled;
	__device__ __forceinline__ uint32_t u32(uint32_t at)
	{
		if (!filled || at < base || at - base > BAM_WINDOW - 4) {
			__syncthreads();                                   // (the reads of the old window are done)
			base = at & ~15u;
			filled = true;
			for (uint32_t o = lane * 16; o < BAM_WINDOW; o += 64 * 16)
				if ((uint64_t)base + o < padded) *reinterpret_cast<uint4*>(window + o) = *reinterpret_cast<const uint4*>(text + base + o);   // (the text starts at a 256-byte boundary)
			__syncthreads();
		}
		return bamU32(window + (at - base));
	}
};

__global__ void __launch_bounds__(64) k_bam_walk(const uint8_t* __restrict__ text, uint32_t len, uint32_t flags, uint32_t* __restrict__ recStart, uint32_t* __restrict__ meta)
{
	__shared__ __attribute__((aligned(16))) uint8_t window[BAM_WINDOW];
	BamWindowReader rd { text, (len + 15u) & ~15u, window, threadIdx.x, 0, false };
	const uint32_t lane = threadIdx.x;
	const BamWalk w = bamWalk(rd, len, flags, [&](uint32_t k, uint32_t start) { if (lane == 0) recStart[k] = start; });
	if (lane == 0) {
		meta[BAM_META_RECORDS] = w.n; meta[BAM_META_CONSUMED] = w.consumed; meta[BAM_META_WALK_STATUS] = w.status; meta[BAM_META_WALK_BAD_AT] = w.badAt; meta[BAM_META_IN_HEADER] = w.inHeader;
	}
}

// one thread per record and one more (the scans' last entry)
__global__ void __launch_bounds__(BAM_BLOCK) k_bam_fields(const uint8_t* __restrict__ text, uint32_t nRecords, const uint32_t* __restrict__ recStart, uint32_t* __restrict__ keep,
	uint32_t* __restrict__ seqLen, uint32_t* __restrict__ nameLen, BamSpan* __restrict__ spansAll, unsigned long long* __restrict__ refused)
{
	const uint32_t i = blockIdx.x * BAM_BLOCK + threadIdx.x;
	if (i > nRecords) return;
	if (i == nRecords) { keep[i] = 0; seqLen[i] = 0; nameLen[i] = 0; return; }
	const BamRecord r = bamFields(text, recStart[i]);
	if (r.status != BAM_OK) atomicMin(refused, ((unsigned long long)i << BAM_STATUS_BITS) | r.status);
	keep[i] = r.keep;
	seqLen[i] = r.keep ? r.span.lSeqRev & 0x7fffffffu : 0;
	nameLen[i] = r.keep ? r.span.nameLen : 0;
	spansAll[i] = r.span;
}

__global__ void __launch_bounds__(BAM_BLOCK) k_bam_compact(uint32_t nRecords, BamTables t)
{
	const uint32_t i = blockIdx.x * BAM_BLOCK + threadIdx.x;
	if (i > nRecords) return;
	const uint32_t k = t.kept[i];
	if (i == nRecords) {
		t.readOff[k] = t.seqOff[i]; t.nameOff[k] = t.nameOffAll[i];
		t.meta[BAM_META_KEPT] = k; t.meta[BAM_META_BASES] = t.seqOff[i]; t.meta[BAM_META_NAME_BYTES] = t.nameOffAll[i];
	} else if (t.keep[i]) {
		t.spans[k] = t.spansAll[i]; t.readOff[k] = t.seqOff[i]; t.nameOff[k] = t.nameOffAll[i];
	}
}

__global__ void __launch_bounds__(BAM_BLOCK) k_bam_names(const uint8_t* __restrict__ text, uint32_t nRecords, const uint32_t* __restrict__ keep, const BamSpan* __restrict__ spansAll,
	const uint32_t* __restrict__ nameOffAll, char* __restrict__ names)
{
	const uint64_t th = (uint64_t)blockIdx.x * BAM_BLOCK + threadIdx.x;
	const uint64_t i = th / BAM_NAME_LANES;
	if (i >= nRecords || !keep[i]) return;
	const BamSpan s = spansAll[i];
	const uint8_t* src = text + s.nameAt;
	char* dst = names + nameOffAll[i];
	for (uint32_t k = (uint32_t)(th % BAM_NAME_LANES); k < s.nameLen; k += BAM_NAME_LANES) dst[k] = (char)src[k];   // (the last byte is the NUL: bamFields has seen it)
}

__global__ void __launch_bounds__(BAM_BLOCK) k_bam_unpack(const uint8_t* __restrict__ text, const BamSpan* __restrict__ spans, const uint64_t* __restrict__ readOff, uint32_t nKept,
	uint32_t total, char* __restrict__ bases)
{
	const uint64_t p0 = ((uint64_t)blockIdx.x * BAM_BLOCK + threadIdx.x) * BAM_UNPACK_LETTERS;
	if (p0 >= total) return;
	const uint64_t p1 = p0 + BAM_UNPACK_LETTERS < total ? p0 + BAM_UNPACK_LETTERS : total;
	uint64_t lo = 0, hi = 0;
	bamUnpackSpan(text, spans, readOff, nKept, p0, p1, [&](uint32_t k, uint8_t c) {
		if (k < 8) lo |= (uint64_t)c << (8 * k); else hi |= (uint64_t)c << (8 * (k - 8));
	});
	if (p1 - p0 == BAM_UNPACK_LETTERS) {
		*reinterpret_cast<uint4*>(bases + p0) = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));   // (bases starts at a 256-byte boundary)
	} else {
		for (uint32_t k = 0; k < p1 - p0; k++) bases[p0 + k] = (char)((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8))) & 0xff);
	}
}

} // namespace

size_t bamScanTempBytes(uint32_t nRecords)
{
	size_t bytes = 0;
	if (hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int64_t)nRecords + 1) != hipSuccess) bytes = 0;
	return bytes + 256;
}

// recStart: room for every record the bytes can hold (len / 36 + 1); meta: BAM_META_WORDS words, zeroed here but for the refused word, which is set to BAM_NONE_REFUSED
hipError_t bamWalkRecords(hipStream_t q, const uint8_t* text, uint32_t len, uint32_t flags, uint32_t* recStart, uint32_t* meta)
{
	BAM_TRY(hipMemsetAsync(meta, 0, BAM_META_WORDS * sizeof(uint32_t), q));
	BAM_TRY(hipMemsetAsync(meta + BAM_META_REFUSED_LO, 0xff, sizeof(unsigned long long), q));
	hipLaunchKernelGGL(k_bam_walk, dim3(1), dim3(64), 0, q, text, len, flags, recStart, meta);
	return hipGetLastError();
}

// fields, scans, the kept records' tables and the counts in meta
hipError_t bamBuildRecords(hipStream_t q, const uint8_t* text, uint32_t nRecords, const BamTables& t)
{
	const uint32_t blocks = bamBlocks((uint64_t)nRecords + 1);
	hipLaunchKernelGGL(k_bam_fields, dim3(blocks), dim3(BAM_BLOCK), 0, q, text, nRecords, t.recStart, t.keep, t.seqLen, t.nameLen, t.spansAll, (unsigned long long*)(t.meta + BAM_META_REFUSED_LO));
	BAM_TRY(hipGetLastError());
	size_t bytes = t.tempBytes;
	BAM_TRY(hipcub::DeviceScan::ExclusiveSum(t.temp, bytes, (const uint32_t*)t.keep, t.kept, (int64_t)nRecords + 1, q));
	bytes = t.tempBytes;
	BAM_TRY(hipcub::DeviceScan::ExclusiveSum(t.temp, bytes, (const uint32_t*)t.seqLen, t.seqOff, (int64_t)nRecords + 1, q));
	bytes = t.tempBytes;
	BAM_TRY(hipcub::DeviceScan::ExclusiveSum(t.temp, bytes, (const uint32_t*)t.nameLen, t.nameOffAll, (int64_t)nRecords + 1, q));
	hipLaunchKernelGGL(k_bam_compact, dim3(blocks), dim3(BAM_BLOCK), 0, q, nRecords, t);
	return hipGetLastError();
}

hipError_t bamWriteNames(hipStream_t q, const uint8_t* text, uint32_t nRecords, const BamTables& t, char* names)
{
	if (!nRecords) return hipSuccess;
	hipLaunchKernelGGL(k_bam_names, dim3(bamBlocks((uint64_t)nRecords * BAM_NAME_LANES)), dim3(BAM_BLOCK), 0, q, text, nRecords, (const uint32_t*)t.keep, (const BamSpan*)t.spansAll,
		(const uint32_t*)t.nameOffAll, names);
	return hipGetLastError();
}

hipError_t bamUnpackBases(hipStream_t q, const uint8_t* text, const BamTables& t, uint32_t nKept, uint32_t total, char* bases)
{
	if (!total) return hipSuccess;
	hipLaunchKernelGGL(k_bam_unpack, dim3(bamBlocks(((uint64_t)total + BAM_UNPACK_LETTERS - 1) / BAM_UNPACK_LETTERS)), dim3(BAM_BLOCK), 0, q, text, (const BamSpan*)t.spans, (const uint64_t*)t.readOff, nKept, total, bases);
	return hipGetLastError();
}

} // namespace gcdev
