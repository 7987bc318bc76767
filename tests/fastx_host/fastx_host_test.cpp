// The FASTA / FASTQ loader without a GPU: csrc/hip/gc_fastx_core.hpp compiled for the host, driven the way hip/gc_fastx.hip drives it - the newline count in tiles of
// FX_COUNT_TILE bytes with one 16-byte word per thread and step, one call per line for the maps and header flags, the scans (map composition, header count,
// destinations, id offsets) as tiles of FX_BLOCK items with a carry between them, and the gather as one 16-byte span per thread packed into two 64-bit words as the
// kernel packs them. Reads cases "<format> <final> <hex of the text or ->" from the file given and prints "<consumed> <n>" and n lines "<hex id> <hex sequence>" for each.
#include "gc_fastx_core.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

using namespace gcdev;

static void die(const char* what) { fprintf(stderr, "fastx_host_test: %s\n", what); exit(2); }

template <typename T, typename Op>
static void tiledInclusiveScan(const std::vector<T>& in, std::vector<T>& out, size_t n, Op op)
{
	bool have = false;
	T carry {};
	for (size_t tile = 0; tile < n; tile += FX_BLOCK) {
		const size_t end = tile + FX_BLOCK < n ? tile + FX_BLOCK : n;
		T local = in[tile];                       // the tile's own scan first, then the carry in front of every item, as a decoupled scan combines them
		std::vector<T> own(end - tile);
		own[0] = local;
		for (size_t i = tile + 1; i < end; i++) own[i - tile] = local = op(local, in[i]);
		for (size_t i = tile; i < end; i++) out[i] = have ? op(carry, own[i - tile]) : own[i - tile];
		carry = out[end - 1];
		have = true;
	}
}

struct Parsed { uint32_t consumed = 0; std::vector<std::string> ids, seqs; };

static Parsed parse(const std::string& textIn, int format, bool final)
{
	// the device's copy of the text is in a block of its own: give the sanitizer the exact bounds
	std::vector<char> text(textIn.begin(), textIn.end());
	const uint32_t L = (uint32_t)text.size();
	// ---- newline count, tile by tile ----
	uint32_t counted = 0;
	for (uint64_t tile = 0; tile < L; tile += FX_COUNT_TILE)
		for (uint32_t step = 0; step < FX_COUNT_TILE / (FX_BLOCK * FX_COUNT_BYTES); step++)
			for (uint32_t tid = 0; tid < FX_BLOCK; tid++) {
				const uint64_t at = tile + ((uint64_t)step * FX_BLOCK + tid) * FX_COUNT_BYTES;
				if (at + FX_COUNT_BYTES <= L) {
					uint32_t w[4];
					memcpy(w, text.data() + at, 16);
					for (uint32_t x : w) counted += fxNewlinesInWord(x);
				} else {
					for (uint64_t p = at; p < L; p++) counted += text[p] == '\n';
				}
			}
	std::vector<uint32_t> lineEnd;
	for (uint32_t p = 0; p < L; p++) if (text[p] == '\n') lineEnd.push_back(p);
	if (lineEnd.size() != counted) die("the tiled newline count differs from the selection");
	FxView v {};
	v.text = text.data(); v.len = L; v.nNewlines = counted; v.format = format; v.final = final ? 1u : 0u; v.lineEnd = lineEnd.data();
	v.nLines = counted + (final && L && text[L - 1] != '\n' ? 1u : 0u);
	Parsed out;
	out.consumed = final ? L : 0;
	if (!v.nLines) return out;
	const size_t n = v.nLines;
	std::vector<uint8_t> map(n, 0), scanned(n, 0);
	std::vector<uint32_t> hdr(n, 0), recIdx(n, 0), contrib(n + 1, 0), dest(n + 1, 0), recLine(n, 0);
	for (uint32_t i = 0; i < n; i++) {
		const FxLine l = fxLine(v, i);
		if (format == FX_FASTQ) map[i] = fxFastqMap(l); else hdr[i] = fxFastaHeader(v, l, i) ? 1u : 0u;
	}
	if (format == FX_FASTQ) {
		tiledInclusiveScan(map, scanned, n, FxCompose());
		for (uint32_t i = 0; i < n; i++) hdr[i] = fxFastqIsHeader(scanned[i]) ? 1u : 0u;
	}
	tiledInclusiveScan(hdr, recIdx, n, [](uint32_t a, uint32_t b) { return a + b; });
	const uint32_t nHeaders = recIdx[n - 1];
	for (uint32_t i = 0; i < n; i++) {
		contrib[i] = fxContribution(v, fxLine(v, i), i, recIdx[i], nHeaders, scanned[i], hdr[i] != 0);
		if (hdr[i]) recLine[recIdx[i] - 1] = i;
	}
	{
		std::vector<uint32_t> inclusive(n + 1, 0);
		tiledInclusiveScan(contrib, inclusive, n + 1, [](uint32_t a, uint32_t b) { return a + b; });
		for (size_t i = 0; i <= n; i++) dest[i] = inclusive[i] - contrib[i];
	}
	const uint32_t nRecords = fxRecordCount(v, nHeaders, nHeaders ? recLine[nHeaders - 1] : 0), total = dest[n];
	out.consumed = fxConsumed(v, nHeaders, nRecords, recLine.data());
	std::vector<uint64_t> readOff(nRecords + 1);
	for (uint32_t r = 0; r <= nRecords; r++) readOff[r] = r < nHeaders ? dest[recLine[r]] : dest[n];
	if (readOff[nRecords] != total) die("the offset of the end is not the number of bases");
	// ---- gather: every thread's span through the kernel's two words ----
	std::vector<char> bases(total);
	for (uint64_t p0 = 0; p0 < total; p0 += FX_GATHER_BYTES) {
		const uint32_t p1 = (uint32_t)(p0 + FX_GATHER_BYTES < total ? p0 + FX_GATHER_BYTES : total);
		uint64_t lo = 0, hi = 0;
		uint32_t calls = 0;
		fxGatherSpan(v, dest.data(), (uint32_t)p0, p1, [&](uint32_t k, char c) {
			const uint64_t b = (uint64_t)(uint8_t)c;
			if (k != calls++) die("the gather skipped a byte");
			if (k < 8) lo |= b << (8 * k); else hi |= b << (8 * (k - 8));
		});
		if (calls != p1 - p0) die("the gather stopped early");
		for (uint32_t k = 0; k < p1 - p0; k++) bases[p0 + k] = (char)((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8))) & 0xff);
	}
	for (uint32_t r = 0; r < nRecords; r++) {
		const FxLine l = fxLine(v, recLine[r]);
		if (!l.len) die("a header line without its first byte");
		out.ids.emplace_back(text.data() + l.start + 1, l.len - 1);
		out.seqs.emplace_back(bases.data() + readOff[r], readOff[r + 1] - readOff[r]);
	}
	return out;
}

static std::string unhex(const std::string& h)
{
	std::string s;
	if (h == "-") return s;
	for (size_t i = 0; i + 1 < h.size(); i += 2) s.push_back((char)strtol(h.substr(i, 2).c_str(), nullptr, 16));
	return s;
}
static void hex(const std::string& s) { if (s.empty()) printf("-"); for (unsigned char c : s) printf("%02x", c); }

int main(int argc, char** argv)
{
	if (argc < 2) die("usage: fastx_host_test CASES");
	// the composition is associative and the identity map is neutral: what lets a scan regroup it
	for (int a = 0; a < 256; a += 7) for (int b = 0; b < 256; b += 5) for (int c = 0; c < 256; c += 11)
		if (FxCompose()(FxCompose()((uint8_t)a, (uint8_t)b), (uint8_t)c) != FxCompose()((uint8_t)a, FxCompose()((uint8_t)b, (uint8_t)c))) die("composition is not associative");
	for (int a = 0; a < 256; a++) if (FxCompose()((uint8_t)a, FX_MAP_IDENTITY) != a || FxCompose()(FX_MAP_IDENTITY, (uint8_t)a) != a) die("the identity map is not neutral");
	std::ifstream in(argv[1]);
	std::string fmt, fin, data;
	size_t cases = 0;
	while (in >> fmt >> fin >> data) {
		const Parsed p = parse(unhex(data), fmt == "fastq" ? FX_FASTQ : FX_FASTA, fin == "1");
		printf("%u %zu\n", p.consumed, p.ids.size());
		for (size_t r = 0; r < p.ids.size(); r++) { hex(p.ids[r]); printf(" "); hex(p.seqs[r]); printf("\n"); }
		cases++;
	}
	fprintf(stderr, "%zu cases\n", cases);
	return 0;
}
