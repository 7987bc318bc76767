// FASTA / FASTQ text to a read batch on the device (gc_reads_parse): the kernels around gc_fastx_core.hpp, which says what each table means. The text of one chunk lies in
// HBM; the passes are a newline count, a selection of the newline positions, one thread per line for the line's map or header flag, hipCUB scans (map composition, header
// count, destinations, name offsets), one thread per 16 bytes of the compacted reads for the gather and one wave per record for the ids. All are memory-bound and use blocks
// of 256 threads with a few registers each, so every CU holds its full complement of waves; nothing here keeps a wave busy for long.
#include <hip/hip_runtime.h>
#include "gc_fastx_core.hpp"
#include <hipcub/hipcub.hpp>

namespace gcdev {

namespace {

#define FX_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

inline uint32_t fxBlocks(uint64_t items) { return (uint32_t)((items + FX_BLOCK - 1) / FX_BLOCK); }

// every block counts the '\n' of its FX_COUNT_TILE bytes: 128-bit loads where 16 bytes are left, single bytes at the text's end
__global__ void __launch_bounds__(FX_BLOCK) k_fx_count(const char* __restrict__ text, uint32_t len, uint32_t* __restrict__ meta)
{
	const uint64_t tile = (uint64_t)blockIdx.x * FX_COUNT_TILE;
	uint32_t count = 0;
	for (uint32_t step = 0; step < FX_COUNT_TILE / (FX_BLOCK * FX_COUNT_BYTES); step++) {
		const uint64_t at = tile + ((uint64_t)step * FX_BLOCK + threadIdx.x) * FX_COUNT_BYTES;
		if (at + FX_COUNT_BYTES <= len) {
			const uint4 w = *reinterpret_cast<const uint4*>(text + at);   // (the text starts at a 256-byte boundary)
			count += fxNewlinesInWord(w.x) + fxNewlinesInWord(w.y) + fxNewlinesInWord(w.z) + fxNewlinesInWord(w.w);
		} else {
			for (uint64_t p = at; p < len; p++) count += text[p] == '\n';
		}
	}
	for (int d = 32; d; d >>= 1) count += __shfl_down(count, d);
	if ((threadIdx.x & 63) == 0 && count) atomicAdd(&meta[FX_META_NEWLINES], count);
}

struct FxIsNewline {
	const char* text;
	__host__ __device__ __forceinline__ bool operator()(uint32_t p) const { return text[p] == '\n'; }
};

__global__ void __launch_bounds__(FX_BLOCK) k_fx_lines(FxView v, uint8_t* __restrict__ map, uint32_t* __restrict__ hdr)
{
	const uint32_t i = blockIdx.x * FX_BLOCK + threadIdx.x;
	if (i >= v.nLines) return;
	const FxLine l = fxLine(v, i);
	if (v.format == FX_FASTQ) map[i] = fxFastqMap(l);
	else hdr[i] = fxFastaHeader(v, l, i) ? 1u : 0u;
}

__global__ void __launch_bounds__(FX_BLOCK) k_fx_fastq_headers(uint32_t nLines, const uint8_t* __restrict__ scanned, uint32_t* __restrict__ hdr)
{
	const uint32_t i = blockIdx.x * FX_BLOCK + threadIdx.x;
	if (i < nLines) hdr[i] = fxFastqIsHeader(scanned[i]) ? 1u : 0u;
}

// one thread per line and one more: the line's bytes in the compacted reads, and for a header the line of its record
__global__ void __launch_bounds__(FX_BLOCK) k_fx_contrib(FxView v, const uint8_t* __restrict__ scanned, const uint32_t* __restrict__ hdr, const uint32_t* __restrict__ recIdx,
	uint32_t* __restrict__ contrib, uint32_t* __restrict__ recLine)
{
	const uint32_t i = blockIdx.x * FX_BLOCK + threadIdx.x;
	if (i > v.nLines) return;
	if (i == v.nLines) { contrib[i] = 0; return; }
	const uint32_t nHeaders = recIdx[v.nLines - 1];
	const bool isHeader = hdr[i] != 0;
	contrib[i] = fxContribution(v, fxLine(v, i), i, recIdx[i], nHeaders, v.format == FX_FASTQ ? scanned[i] : (uint8_t)0, isHeader);
	if (isHeader) recLine[recIdx[i] - 1] = i;
}

__global__ void k_fx_meta(FxView v, const uint32_t* __restrict__ recIdx, const uint32_t* __restrict__ recLine, const uint32_t* __restrict__ dest, uint32_t* __restrict__ meta)
{
	if (blockIdx.x || threadIdx.x) return;
	const uint32_t nHeaders = recIdx[v.nLines - 1];
	const uint32_t nRecords = fxRecordCount(v, nHeaders, nHeaders ? recLine[nHeaders - 1] : 0);
	meta[FX_META_HEADERS] = nHeaders;
	meta[FX_META_RECORDS] = nRecords;
	meta[FX_META_BASES] = dest[v.nLines];
	meta[FX_META_CONSUMED] = fxConsumed(v, nHeaders, nRecords, recLine);
}

// one thread per record and one more: the read's offset and the bytes of its id with the NUL
__global__ void __launch_bounds__(FX_BLOCK) k_fx_records(FxView v, uint32_t nHeaders, uint32_t nRecords, const uint32_t* __restrict__ recLine, const uint32_t* __restrict__ dest,
	uint64_t* __restrict__ readOff, uint32_t* __restrict__ nameLen)
{
	const uint32_t r = blockIdx.x * FX_BLOCK + threadIdx.x;
	if (r > nRecords) return;
	readOff[r] = r < nHeaders ? dest[recLine[r]] : dest[v.nLines];
	nameLen[r] = r < nRecords ? fxLine(v, recLine[r]).len : 0;   // (the line without its first byte, and the NUL)
}

__global__ void __launch_bounds__(FX_BLOCK) k_fx_gather(FxView v, const uint32_t* __restrict__ dest, uint32_t total, char* __restrict__ bases)
{
	const uint64_t p0 = ((uint64_t)blockIdx.x * FX_BLOCK + threadIdx.x) * FX_GATHER_BYTES;
	if (p0 >= total) return;
	const uint32_t p1 = (uint32_t)(p0 + FX_GATHER_BYTES < total ? p0 + FX_GATHER_BYTES : total);
	uint64_t lo = 0, hi = 0;
	fxGatherSpan(v, dest, (uint32_t)p0, p1, [&](uint32_t k, char c) {
		const uint64_t b = (uint64_t)(uint8_t)c;
		if (k < 8) lo |= b << (8 * k); else hi |= b << (8 * (k - 8));
	});
	if (p1 - p0 == FX_GATHER_BYTES) {
		*reinterpret_cast<uint4*>(bases + p0) = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));   // (bases starts at a 256-byte boundary)
	} else {
		for (uint32_t k = 0; k < p1 - p0; k++) bases[p0 + k] = (char)((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8))) & 0xff);
	}
}

__global__ void __launch_bounds__(FX_NAME_LANES) k_fx_names(FxView v, uint32_t nRecords, const uint32_t* __restrict__ recLine, const uint32_t* __restrict__ nameOff, char* __restrict__ names)
{
	const uint32_t r = blockIdx.x;
	if (r >= nRecords) return;
	const FxLine l = fxLine(v, recLine[r]);
	char* out = names + nameOff[r];
	for (uint32_t k = threadIdx.x; k + 1 < l.len; k += FX_NAME_LANES) out[k] = v.text[l.start + 1 + k];
	if (threadIdx.x == 0) out[l.len - 1] = 0;   // (a header line has its first byte: len >= 1)
}

} // namespace

size_t fxScanTempBytes(uint32_t len, uint32_t nLines)
{
	size_t most = 0, bytes = 0;
	if (hipcub::DeviceSelect::If(nullptr, bytes, hipcub::CountingInputIterator<uint32_t>(0), (uint32_t*)nullptr, (uint32_t*)nullptr, (int64_t)len, FxIsNewline { nullptr }) == hipSuccess && bytes > most) most = bytes;
	if (hipcub::DeviceScan::InclusiveScan(nullptr, bytes, (const uint8_t*)nullptr, (uint8_t*)nullptr, FxCompose(), (int64_t)nLines + 1) == hipSuccess && bytes > most) most = bytes;
	if (hipcub::DeviceScan::InclusiveSum(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int64_t)nLines + 1) == hipSuccess && bytes > most) most = bytes;
	if (hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int64_t)nLines + 1) == hipSuccess && bytes > most) most = bytes;
	return most + 256;
}

hipError_t fxCountNewlines(hipStream_t q, const char* text, uint32_t len, uint32_t* meta)
{
	FX_TRY(hipMemsetAsync(meta, 0, FX_META_WORDS * sizeof(uint32_t), q));
	if (!len) return hipSuccess;
	hipLaunchKernelGGL(k_fx_count, dim3((uint32_t)(((uint64_t)len + FX_COUNT_TILE - 1) / FX_COUNT_TILE)), dim3(FX_BLOCK), 0, q, text, len, meta);
	return hipGetLastError();
}

// the line table, the roles, the destinations and the counts in meta; v.nLines > 0
hipError_t fxBuildTables(hipStream_t q, const FxView& v, const FxTables& t)
{
	size_t bytes = t.tempBytes;
	if (v.nNewlines) FX_TRY(hipcub::DeviceSelect::If(t.temp, bytes, hipcub::CountingInputIterator<uint32_t>(0), t.lineEnd, t.meta + FX_META_SELECTED, (int64_t)v.len, FxIsNewline { v.text }, q));
	hipLaunchKernelGGL(k_fx_lines, dim3(fxBlocks(v.nLines)), dim3(FX_BLOCK), 0, q, v, t.map, t.hdr);
	FX_TRY(hipGetLastError());
	if (v.format == FX_FASTQ) {
		bytes = t.tempBytes;
		FX_TRY(hipcub::DeviceScan::InclusiveScan(t.temp, bytes, (const uint8_t*)t.map, t.scanned, FxCompose(), (int64_t)v.nLines, q));
		hipLaunchKernelGGL(k_fx_fastq_headers, dim3(fxBlocks(v.nLines)), dim3(FX_BLOCK), 0, q, v.nLines, (const uint8_t*)t.scanned, t.hdr);
		FX_TRY(hipGetLastError());
	}
	bytes = t.tempBytes;
	FX_TRY(hipcub::DeviceScan::InclusiveSum(t.temp, bytes, (const uint32_t*)t.hdr, t.recIdx, (int64_t)v.nLines, q));
	hipLaunchKernelGGL(k_fx_contrib, dim3(fxBlocks((uint64_t)v.nLines + 1)), dim3(FX_BLOCK), 0, q, v, (const uint8_t*)t.scanned, (const uint32_t*)t.hdr, (const uint32_t*)t.recIdx, t.contrib, t.recLine);
	FX_TRY(hipGetLastError());
	bytes = t.tempBytes;
	FX_TRY(hipcub::DeviceScan::ExclusiveSum(t.temp, bytes, (const uint32_t*)t.contrib, t.dest, (int64_t)v.nLines + 1, q));
	hipLaunchKernelGGL(k_fx_meta, dim3(1), dim3(64), 0, q, v, (const uint32_t*)t.recIdx, (const uint32_t*)t.recLine, (const uint32_t*)t.dest, t.meta);
	return hipGetLastError();
}

// readOff [nRecords + 1] (64-bit, what the packing kernels take), nameLen and nameOff [nRecords + 1]
hipError_t fxBuildRecords(hipStream_t q, const FxView& v, const FxTables& t, uint32_t nHeaders, uint32_t nRecords, uint64_t* readOff, uint32_t* nameLen, uint32_t* nameOff)
{
	hipLaunchKernelGGL(k_fx_records, dim3(fxBlocks((uint64_t)nRecords + 1)), dim3(FX_BLOCK), 0, q, v, nHeaders, nRecords, (const uint32_t*)t.recLine, (const uint32_t*)t.dest, readOff, nameLen);
	FX_TRY(hipGetLastError());
	size_t bytes = t.tempBytes;
	return hipcub::DeviceScan::ExclusiveSum(t.temp, bytes, (const uint32_t*)nameLen, nameOff, (int64_t)nRecords + 1, q);
}

hipError_t fxGatherBases(hipStream_t q, const FxView& v, const FxTables& t, uint32_t total, char* bases)
{
	if (!total) return hipSuccess;
	hipLaunchKernelGGL(k_fx_gather, dim3((uint32_t)(((uint64_t)total + FX_GATHER_TILE - 1) / FX_GATHER_TILE)), dim3(FX_BLOCK), 0, q, v, (const uint32_t*)t.dest, total, bases);
	return hipGetLastError();
}

hipError_t fxWriteNames(hipStream_t q, const FxView& v, const FxTables& t, uint32_t nRecords, const uint32_t* nameOff, char* names)
{
	if (!nRecords) return hipSuccess;
	hipLaunchKernelGGL(k_fx_names, dim3(nRecords), dim3(FX_NAME_LANES), 0, q, v, nRecords, (const uint32_t*)t.recLine, nameOff, names);
	return hipGetLastError();
}

} // namespace gcdev
