/* graphchainer_amd - C ABI of the MI355X-native GraphChainer hot path.
 *
 * The reference (algbio/GraphChainer) has no plugin/FFI layer; its de-facto seam is the free-function
 * facade src/GraphAlignerWrapper.h:39-47 plus MinimizerSeeder::getSeeds (src/MinimizerSeeder.h:33) and
 * AlignmentGraph::colinearChaining (src/AlignmentGraph.h:121), all called per read from
 * runComponentMappings (src/Aligner.cpp:538,560,565,660,666,691,735). This library replaces that
 * per-read call sequence with one batched call; every entry point cites what it stands in for.
 * INTEGRATION.md shows the shim a maintainer would add to src/Aligner.cpp.
 *
 * Conventions: plain pointers and sizes, no C++/torch types. Every function returns 0 on success and
 * a negative gc_status otherwise; gc_last_error() gives the message for the calling thread. Handles are
 * immutable after creation and may be shared between threads; one gc_align_batch per gc_stream at a
 * time (the reference's rule of one AlignerGraphsizedState per worker, src/Aligner.cpp:469).
 * Per-read failures (the reference's per-read catch of AssertionFailure, src/Aligner.cpp:585-592) and per-read
 * capacity overflows of this library are reported in the result arrays (failed_assertion, capacity_exceeded),
 * never as a call failure.
 */
#ifndef GRAPHCHAINER_AMD_H
#define GRAPHCHAINER_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gc_status {
	GC_OK = 0,
	GC_ERR_INVALID = -1,      /* bad argument */
	GC_ERR_GRAPH = -2,        /* invalid graph (reference: InvalidGraphException, cyclic graph) */
	GC_ERR_DEVICE = -3,       /* HIP error or no device: the product path never falls back to the CPU */
	GC_ERR_INTERNAL = -4
} gc_status;

typedef struct gc_graph gc_graph;     /* AlignmentGraph + MPC index, resident in HBM */
typedef struct gc_seeder gc_seeder;   /* MinimizerSeeder index, resident in HBM */
typedef struct gc_stream gc_stream;   /* per-worker reusable state (HIP stream + arenas) */
typedef struct gc_reads gc_reads;     /* a batch of reads uploaded to HBM */
typedef struct gc_seeds gc_seeds;     /* a read batch's seed hits from the host's own seeder, resolved and resident in HBM */

/* Capacities of the device-side tables one batch uses. The reference grows std::vectors and hash maps as it goes; a kernel works in tables sized before the launch.
 * Every table is PER EXTENSION or PER READ, never per batch, and what outgrows one never fails the call: the work is rerun with more room (second launch, other
 * kernel layout, larger pool) and, only if that overflows too, the READ is flagged in gc_result::capacity_exceeded and reported without the affected part.
 * 0 = automatic (the values in brackets, derived from the batch's longest read L); set a field only to trade memory against reruns on unusual inputs
 * (dense variant clusters, very noisy long reads). The same knobs exist as GC_TEST_* environment variables for tests; the environment wins. */
typedef struct gc_capacities {
	int64_t ext_max_items;          /* fragment extensions (k_extend): (slice, node) tiles per extension [72; the retry launch has 16x] (GC_TEST_EXT_MAX_ITEMS) */
	int64_t ext_max_pending;        /* ... entries of the per-slice node queue [48; retry 16x] (GC_TEST_EXT_MAX_PENDING) */
	int64_t ext_max_trace;          /* ... trace cells per extension [192; retry 16x] (GC_TEST_EXT_MAX_TRACE) */
	int64_t long_max_items;         /* whole-read extensions (k_long_extend): tiles per extension [max(8192, 24 per slice)] (GC_TEST_LONG_MAX_ITEMS) */
	int64_t long_column_store;      /* ... DP columns kept for the backtrace per extension [3 L + 4096]; -1: keep none, the backtrace recomputes its tiles (GC_TEST_LONG_MAX_COLS) */
	int64_t long_cells_per_base;    /* merged trace cells per read base in the batch's pool [8, tripled and the pass rerun when a batch overflows it; the stream remembers]
	                                 * (GC_TEST_LONG_CELLS_PER_BASE; setting it pins the pool: overflowing reads are flagged instead) */
	int64_t long_scratch_bytes;     /* upper bound of the whole-read pass's per-wave scratch [48 GiB; 0.8 MB per resident wave at L = 10 kb, 2.4 MB at 50 kb] (GC_TEST_LONG_SCRATCH_GB) */
	int64_t stitch_set_max;         /* chain stitching (k_stitch): nodes of one bridged region searched on the device [automatic]; larger regions go to the host (GC_TEST_STITCH_SET_MAX) */
	int64_t stitch_bfs_cap;         /* ... frontier entries of one bridge search [automatic] (GC_TEST_STITCH_BFS_CAP) */
	int64_t reserved[3];            /* must be 0 */
} gc_capacities;

/* Alignment parameters. Defaults = the reference's chaining-mode presets, src/AlignerMain.cpp:186-209. */
typedef struct gc_params {
	int32_t bandwidth;          /* -b, initialBandwidth (10) */
	int32_t split_len;          /* --colinear-split-len (35) */
	int32_t split_gap;          /* --colinear-split-gap (35); --sampling-step 0.5 == 18 */
	int64_t colinear_gap;       /* --colinear-gap (10000) */
	double  seed_density;       /* --seeds-minimizer-density (10) */
	int32_t min_cluster_size;   /* --seeds-clustersize (1) */
	int32_t long_pass;          /* 1: also run the whole-read GraphAligner pass (src/Aligner.cpp:630-654) */
	int32_t keep_traces;        /* 1: return the traces of every anchor and of every whole-read alignment (parity tests); 2: the alignments' traces only
	                             *    (long_trace_*: what gc_format_gaf / _json / _gam read; the anchors' traces - 13 B x ~37 cells per anchor - stay on the device) */
	int32_t keep_seeds;         /* 1: return the ordered seed list of every read (seed_* arrays; else they are empty) */
	int32_t stitch;             /* 1: stitch the chain into one path (src/Aligner.cpp:754-822): read_path_off / path_* */
	int32_t edit_distances;     /* 1: GreedyLength selection of the whole-read alignments and the two NW edit distances that pick
	                             *    the winner (src/Aligner.cpp:636-654,845,901-905): read_long_off / long_index / *_edit_distance / chained_better */
	int32_t chain_traces;       /* the chained alignment's trace (edlibAlign(pathseq, read, NW, EDLIB_TASK_PATH) walked over the stitched path,
	                             *    src/Aligner.cpp:845-897): 0 none, 1 for the reads whose chained alignment wins (default; what the output
	                             *    encoders need), 2 for every read with a stitched path. Needs stitch and edit_distances. Cost: one k_edit_path
	                             *    pair per traced read plus ~13 B of result memory per trace cell; with long_pass == 0 every read with a stitched
	                             *    path counts as a winner (nothing to beat, src/Aligner.cpp:905), i.e. mode 1 then traces them all - pass 0 when
	                             *    only anchors and chains are wanted. */
	int32_t device_output;      /* r4: encode the final alignments on the device, where their traces already are, instead of bringing the traces down (keep_traces)
	                             *    for gc_format_*: bit 0 (1) the GAF path and cg:Z: CIGAR text with = / X items, bit 1 (2) the same with M items
	                             *    (--cigar-match-mismatch merge; give one of the two), bit 2 (4) the vg::Path wire bytes that gc_format_gam / _json wrap,
	                             *    bit 3 (8) the corrected reads' pieces (GraphAligner's --corrected-out / --corrected-clipped-out: AddCorrected, src/GraphAligner.h:220-231)
	                             *    that gc_format_corrected puts into records; bit 3 also works alone, without GAF or vg pieces.
	                             *    Fills gc_result::read_out_off / out_*; needs long_pass and edit_distances. (Sits in what used to be padding: the layout of the
	                             *    other fields is unchanged.) */
	double  e_cutoff;           /* --E-cutoff (src/AlignerMain.cpp:159,271-274; SelectECutoff src/AlignmentSelection.cpp:57-61,91-99):
	                             *    alignments with a larger E-value are dropped before selection; -1 (default) keeps all */
	gc_capacities capacity;     /* sizes of the device-side tables (all 0 = automatic: sized from the batch) */
	int32_t ramp_bandwidth;     /* -B, --ramp-bandwidth, rampBandwidth (src/AlignerMain.cpp:95,147,248): 0 (default) off; else > bandwidth
	                             *    (src/AlignerMain.cpp:380-383; GC_ERR_INVALID otherwise). An extension's first slice, and the slices redone after
	                             *    a slice turns "not currently correct", run with this band (getViterbiSlices, src/GraphAlignerBitvectorBanded.h:530-644).
	                             *    A fragment extension is one slice, so the fragment pass runs at this bandwidth outright. */
	int64_t max_cells_per_slice; /* -C, --tangle-effort, maxCellsPerSlice (src/AlignerMain.cpp:96,149,249): -1 (default) unlimited; 0 and up literal
	                             *    (< -1: GC_ERR_INVALID). A slice stops taking nodes once its DP cells pass this count, and a slice that reaches it
	                             *    is backtraced with the "scores not valid" rules (src/GraphAlignerBitvectorBanded.h:400-405,579-584, ...Common.h:599-804). */
	int32_t force_global;       /* --global-alignment, forceGlobal (src/AlignerMain.cpp:66,160,299): 0 (default) off, 1 on (anything else: GC_ERR_INVALID).
	                             *    Every extension of the whole-read pass and of the fragment pass keeps all its slices: it does not stop at a slice that
	                             *    is not "correct from correct" and does not drop a wrongly aligned end, so a successful extension reaches the read's
	                             *    (the fragment's) end however poor its score (src/GraphAlignerBitvectorBanded.h:51,120,587-645). With ramp_bandwidth
	                             *    only the first slice runs at the ramp band (:544: nothing rewinds); max_cells_per_slice acts as without the flag. */
	double  seed_extend_density; /* --seeds-extend-density, seedExtendDensity of the WHOLE-READ AlignOneWay (src/GraphAligner.h:121-136): the pass stops once
	                             *    size_t(density x read length + 1) seeds have been extended (failed extensions count) and the next seed scores below the last one
	                             *    extended. -1 (default): all seeds. <= 0 and not -1, or NaN: GC_ERR_INVALID (src/AlignerMain.cpp:405). With colinear_chaining == 1
	                             *    anything but -1 is GC_ERR_INVALID: the reference's front end sets tryAllSeeds with chaining (:204) and then overrides the density
	                             *    (:449-453); this library refuses where the reference overrides. The fragment pass never sees it (its budget is the window's seeds). */
	int32_t extra_heuristic;    /* --extra-heuristic, nondeterministicOptimizations (src/GraphAligner.h:127,132,152): 0 (default) off, 1 on (else GC_ERR_INVALID).
	                             *    Whole-read pass only: a seed as good as the end-to-end cut-off ends the scan too (the cut-off starts at 0: a seed of goodness 0
	                             *    ends it before anything is extended), a full seed budget ends it whatever the next seed's goodness, and a seed inside an
	                             *    alignment is skipped whatever that alignment's goodness. It has no effect in the fragment pass: that call is not sloppy and its
	                             *    budget is the window's seed count, so neither :127 nor :132 can fire there and :152 is not reached. */
	int32_t colinear_chaining;  /* 1 (default): chaining mode. 0: --no-colinear-chaining (src/AlignerMain.cpp:198-199, src/Aligner.cpp:596-600,927-930), plain
	                             *    GraphAligner: seeding and the whole-read pass alone, then SelectAlignments(selection_method). No fragment extension, anchors,
	                             *    chains, stitching, NW distances or chained trace are computed: those arrays come back empty (their [n_reads + 1] offsets all 0),
	                             *    chained_better is 0, chain_edit_distance and long_edit_distance are -1. read_long_off / long_index hold what SelectAlignments
	                             *    returns, in its order; the writers sort by alignmentStart (:1004). Needs long_pass == 1 (else, or not 0 / 1: GC_ERR_INVALID). */
	int32_t selection_method;   /* GC_SELECT_* below, the reference's SelectionMethod in its own order (src/AlignmentSelection.h:14-24). Read only when
	                             *    colinear_chaining == 0; with chaining it has no effect: the whole-read side is always GreedyLength (src/Aligner.cpp:639) and
	                             *    :904 selects among one alignment. Outside 0..7: GC_ERR_INVALID. */
	int32_t fast_mode;          /* --fast-mode, fastMode (src/AlignerMain.cpp:48,195-196, src/Aligner.cpp:834-843): 0 (default) off, 1 on (anything else: GC_ERR_INVALID).
	                             *    The chained alignment is made without edlib: its trace is the stitched piece itself, one cell per path base (path_cells of them),
	                             *    cell j at read position min(y, x + j) with x = anchor_x of the CHAIN's first anchor (not of the longest piece's) and y = anchor_y of
	                             *    its last. chain_edit_distance then holds the number of cells whose graph letter differs from the read letter at that position (letters
	                             *    compared literally, IUPAC letters included), NOT an NW distance; chain_aln_start = x, chain_aln_end = min(y, x + path_cells - 1) + 1.
	                             *    --E-cutoff and the decision (:904-905) use these numbers; chain_traces keeps its meaning. Neither k_edit_path nor an NW distance of
	                             *    the chain runs: two small kernels (gc_fastchain.hip) count and write the cells. The whole-read side (long_*, long_edit_distance) is
	                             *    untouched. Read only when colinear_chaining == 1 and stitch and edit_distances are set; no effect otherwise (the reference accepts
	                             *    --fast-mode --no-colinear-chaining and never looks at the flag again). (Sits in what used to be padding: sizeof(gc_params) and the
	                             *    layout of the other fields are unchanged.) */
} gc_params;

enum { GC_SELECT_GREEDY_LENGTH = 0, GC_SELECT_GREEDY_SCORE = 1, GC_SELECT_GREEDY_E = 2, GC_SELECT_SCHEDULE_INVERSE_E_SUM = 3, GC_SELECT_SCHEDULE_INVERSE_E_PRODUCT = 4,
       GC_SELECT_SCHEDULE_SCORE = 5, GC_SELECT_SCHEDULE_LENGTH = 6, GC_SELECT_ALL = 7 };

void gc_params_default(gc_params* p);

/* ---- graph (replaces getGraph + AlignmentGraph::buildMPC, src/Aligner.cpp:1137-1156) -------------- */

/* Loads a GFA (S/L lines, 0M overlaps), builds the split-node DAG with the reference's node numbering,
 * the MPC index, and uploads everything to the current HIP device. */
int gc_graph_create_from_gfa(const char* gfa_path, gc_graph** out);

/* Same, from arrays the existing C++ host already holds (src/AlignmentGraph.h:145-172): for a host that
 * keeps its own AlignmentGraph. Adjacency is CSR in the reference's neighbour order.
 * lookup_order (optional): the bigraph node ids in the iteration order of the host's nodeLookup hash map. The reference's
 * minimizer index enumerates nodes in that order (src/MinimizerSeeder.cpp:299-365), and the order of a k-mer's position
 * list - and with it tie-breaks among equally good seeds - follows from it; with it the index built on this graph is
 * identical to the one built on the gc_graph_create_from_gfa graph (tested). Without it (NULL) nodes are enumerated in
 * ascending id, which can order position lists differently. Node names are only known to gc_graph_create_from_gfa (the
 * output encoders print numeric ids otherwise). */
typedef struct gc_graph_desc {
	uint64_t n_nodes;                 /* split nodes */
	uint64_t first_ambiguous;         /* nodes >= this index use ambiguous_seq */
	const uint8_t*  node_length;      /* [n] 1..64 */
	const uint32_t* node_offset;      /* [n] offset inside the original (bigraph) node */
	const int32_t*  node_ids;         /* [n] bigraph node id (2*gfa_id + strand) */
	const uint64_t* node_seq;         /* [2*first_ambiguous] 2 bits/bp */
	const uint64_t* ambiguous_seq;    /* [4*(n-first_ambiguous)] one-hot A,T,C,G words */
	const uint64_t* in_off;  const uint32_t* in_adj;    /* CSR [n+1], [m] */
	const uint64_t* out_off; const uint32_t* out_adj;
	const uint32_t* component_number; /* [n] topological rank (src/AlignmentGraph.cpp:1008) */
	const uint32_t* chain_number;     /* [n] */
	const uint64_t* chain_approx_pos; /* [n] */
	const int32_t*  lookup_order;     /* [n_lookup] or NULL, see above */
	uint64_t n_lookup;
} gc_graph_desc;
int gc_graph_create(const gc_graph_desc* desc, gc_graph** out);
void gc_graph_destroy(gc_graph* g);

/* Read-only views of the host copy (for parity tests and for hosts that want the numbering). */
uint64_t gc_graph_num_nodes(const gc_graph* g);
uint64_t gc_graph_size_bp(const gc_graph* g);
/* name in {"nodeLength","nodeOffset","nodeIDs","reverse","componentNumber","chainNumber","chainApproxPos",
 * "component_map","out_off","out_adj","in_off","in_adj","mpc_width","firstAmbiguous","nodeSeq","ambiguousSeq" (64-bit
 * patterns, gc_graph_desc layout),"lookupOrder", and the MPC index in global node ids: "component_idx","topo_id","mpc_path_comp",
 * "mpc_path_off","mpc_path_nodes","paths_off","paths","back_off","back_node","back_path"}; returns a malloc'd int64 array
 * (free with gc_free). */
int gc_graph_array(const gc_graph* g, const char* name, int64_t** out, uint64_t* count);
/* Frees the HOST copy of the MPC index (path cover, per-node path lists, backward links, topological orders: ~33 bytes of host memory per graph base, 100 GB at 3.1 Gbp);
 * the device keeps its own and aligning reads nothing of it. For hosts that do not write the index cache afterwards: gc_index_save and the MPC arrays of gc_graph_array
 * ("mpc_*", "paths*", "back_*", "topo_id") return GC_ERR_INVALID on a trimmed graph. No reference counterpart (the reference's AlignmentGraph keeps everything). */
int gc_graph_trim_host(gc_graph* g);

/* ---- seeder (replaces MinimizerSeeder::MinimizerSeeder, src/Aligner.cpp:1162) --------------------- */
int gc_seeder_create(const gc_graph* g, int32_t k, int32_t w, double keep_least_frequent_fraction, gc_seeder** out);
void gc_seeder_destroy(gc_seeder* s);
int gc_seeder_array(const gc_seeder* s, const char* name, int64_t** out, uint64_t* count);   /* "kmers","start","positions","maxcount","k","w" */

/* ---- index cache --------------------------------------------------------------
 * The start-up work above (GFA parse, node splitting, topological order, greedy path cover + max-flow shrink, MPC index,
 * minimizer scan: src/AlignmentGraph.cpp:1267-1391,1465-1495, src/MinimizerSeeder.cpp:299-492) written once to a file and
 * loaded instead of recomputed. The reference declares saveMPC/loadMPC (src/AlignmentGraph.h:96-97) with empty bodies and
 * rebuilds everything on every run; these entry points are what those two would bind. The file is checksummed and
 * versioned; a damaged, truncated or other-version file is refused (GC_ERR_GRAPH), never used.
 *   gc_index_build  host only, no HIP device needed: builds graph + MPC (+ minimizer index when k > 0) and writes the cache.
 *   gc_index_save   writes the cache from objects already built (seeder may be NULL).
 *   gc_index_load   reads the cache and uploads to the current device; *seeder_out is NULL when the file holds no
 *                   minimizer index (seeder_out may itself be NULL to skip it). Results are identical to the built objects'.
 *   gc_index_check  host only: verifies the file (checksum, bounds, re-serialises to the same bytes) and reports
 *                   info8 = {version, split nodes, bp, has seeder, k, w, distinct k-mers, positions} (info8 may be NULL). */
int gc_index_build(const char* gfa_path, int32_t k, int32_t w, double keep_least_frequent_fraction, const char* cache_path);
int gc_index_save(const gc_graph* g, const gc_seeder* s, const char* cache_path);
int gc_index_load(const char* cache_path, gc_graph** graph_out, gc_seeder** seeder_out);
int gc_index_check(const char* cache_path, uint64_t* info8);

/* ---- streams and read batches --------------------------------------------------------------------- */
int gc_stream_create(gc_stream** out);
void gc_stream_destroy(gc_stream* st);

/* Uploads n reads (ASCII, concatenated; read i = bases[offsets[i] .. offsets[i+1])) to HBM. */
int gc_reads_upload(const char* bases, const uint64_t* offsets, uint64_t n, gc_reads** out);
void gc_reads_destroy(gc_reads* r);

/* FASTA / FASTQ text to a read batch, parsed on the device: the reads FastQ::streamFastqFromFile (src/fastqloader.h, as the reader thread calls it, src/Aligner.cpp:167-187)
 * yields for the same bytes, as the gc_reads that gc_reads_upload builds from them, plus a table in HOST memory of what the output writers need beside a result.
 * format: GC_FASTX_FASTA / GC_FASTX_FASTQ (the caller looks at the file name as the reference does; a .gz is inflated by the caller). The read's id is its whole header
 * line behind the first byte; read letters are not looked at here (gc_reads_upload's rules hold: a letter outside IUPAC flags the read in the result).
 * flags: GC_FASTX_FINAL - the text runs to the end of the file: the reference's end-of-file rules apply and consumed == len. Without it the text is a chunk
 * from the middle of a file: only lines that end in '\n' count, a record whose end is not yet known (a FASTQ record without its fourth line; the last FASTA record, whose
 * next header has not been seen) is left out, and consumed is the byte where the caller's next chunk must begin - 0 with n_reads 0 when the chunk holds no complete
 * record: the caller then brings more. A text of length 0 is valid and gives an empty batch.
 * GC_ERR_INVALID, checked before a device is needed: a null pointer, another format, unknown flag bits, len of 2^32 - 16 or more (the loader uses 32-bit positions: split
 * the file). Free the table with the function below, the reads as any read batch. */
#define GC_FASTX_FASTA 1
#define GC_FASTX_FASTQ 2
#define GC_FASTX_FINAL 1u
typedef struct gc_fastx_table {
	uint64_t n_reads;
	uint64_t consumed;
	uint64_t* offsets;       /* [n_reads + 1] read i = bases[offsets[i] .. offsets[i+1]): the arrays the output writers take */
	char* bases;             /* the compacted reads */
	uint64_t* name_off;      /* [n_reads + 1] id i = names + name_off[i], NUL-terminated */
	char* names;
	double kernel_ms;        /* device time of the loader's kernels and the packing kernels, copies and waits left out */
} gc_fastx_table;
int gc_reads_parse(const char* text, uint64_t len, int32_t format, uint32_t flags, gc_reads** reads, gc_fastx_table** table);
void gc_fastx_table_free(gc_fastx_table* t);

/* BGZF - the blocked gzip that bgzip, htslib and `samtools fastq` write: a chain of gzip members of at most 64 KiB of text each, every member independent of the others and
 * with its compressed size in its header. A BGZF member here is 1f 8b 08, FLG exactly 4, a BC subfield with SLEN 2 and an ISIZE of at most 64 KiB. The blocks are inflated on the device, one
 * wavefront per block (hip/gc_inflate.hip), under zlib's acceptance rules and with the CRC-32 and ISIZE of every block checked there; any other gzip is the caller's.
 *
 * gc_bgzf_inflate: inflates the whole blocks at the front of data[0 .. len) and hands their text back in *out (malloc'd, *out_len bytes and a NUL; free with gc_free).
 * *consumed is the compressed size of those blocks: a trailing partial block is left for the next call, and a member that is not BGZF stops the walk there, so
 * *consumed == 0 (with *out_len 0, and no device needed) says that the data does not start with a whole BGZF block.
 *
 * gc_reads_parse_bgzf: gc_reads_parse on the text `head` followed by the inflated whole blocks at the front of data. head is plain text carried over from the call
 * before (the *tail it returned); the text is put together in HBM and parsed there by gc_reads_parse's kernels under the same chunk protocol and flags, and never comes
 * down: only *tail does, the text behind the table's consumed (the record cut by the end; malloc'd, NUL behind *tail_len bytes, gc_free), which is the next call's head.
 * table->consumed counts bytes of head + inflated text, *consumed counts compressed bytes as in gc_bgzf_inflate. head_len plus the inflated text must stay below
 * 2^32 - 16. stats, if not NULL: the blocks, their text, and where the time went.
 *
 * Both: GC_ERR_INVALID for a block that does not inflate (a bad deflate stream, a length or CRC that differs); gc_last_error names the first such block's index and its
 * byte offset in data and holds the words of GC_BGZF_REFUSED, by which a caller tells this refusal from GC_ERR_INVALID's other causes. Nothing is returned then, and
 * the device stays usable. */
#define GC_BGZF_REFUSED "could not be inflated"
typedef struct gc_bgzf_stats {
	uint64_t blocks;          /* whole blocks inflated */
	uint64_t inflated_bytes;  /* their text */
	double scan_ms;           /* host: the walk over the block headers */
	double upload_ms;         /* the compressed bytes to the staging block and up */
	double kernel_ms;         /* the inflate kernel (the loader's kernels are in table->kernel_ms) */
} gc_bgzf_stats;
int gc_bgzf_inflate(const void* data, uint64_t len, void** out, uint64_t* out_len, uint64_t* consumed);
int gc_reads_parse_bgzf(const char* head, uint64_t head_len, const void* data, uint64_t len, int32_t format, uint32_t flags,
                        gc_reads** reads, gc_fastx_table** table, char** tail, uint64_t* tail_len, uint64_t* consumed, gc_bgzf_stats* stats /* may be NULL */);

/* Unaligned BAM (uBAM, what ONT basecallers and PacBio instruments deliver) to a read batch, decoded on the device (hip/gc_bam.hip). A .bam file is a chain of BGZF blocks;
 * the bytes here are the inflated ones. The format as this build defines it (SAMv1 section 4.2; little-endian throughout):
 *   file header, only at the start of a file: "BAM\1", l_text u32, text[l_text], n_ref u32, n_ref x (l_name u32, name[l_name], l_ref u32). Stepped over whole, nothing of it used.
 *   record: block_size u32 (the bytes that follow it), refID i32, pos i32, l_read_name u8, mapq u8, bin u16, n_cigar_op u16, flag u16, l_seq u32, next_refID i32,
 *           next_pos i32, tlen i32, read_name[l_read_name] (NUL-terminated, the NUL counted), cigar u32 x n_cigar_op, seq[(l_seq + 1) / 2], qual[l_seq], tags to the end
 *           of the block. Base i is the high nibble of seq[i / 2] for even i, the low one for odd i, spelled by "=ACMGRSVTWYHKDBN".
 * A record becomes a read: its id is read_name without the NUL, its letters are the l_seq bases, reverse-complemented when flag 0x10 is set (in nibble space the complement
 * is the 4-bit reversal; '=' and N stay). Records with flag 0x100 or 0x800 are left out, as `samtools fastq` leaves them out by default, and counted. Qualities, CIGAR and
 * tags are stepped over. l_seq 0 gives a read of length 0, as an empty FASTQ sequence line does. '=' is outside IUPAC: gc_reads_upload's rule flags that read in the result.
 * flags: GC_BAM_HEADER - the bytes start with the file's header; GC_FASTX_FINAL - they run to the end of the file. The chunk protocol is gc_reads_parse's: data begins at the
 * header or at a record boundary, only whole records are returned, table->consumed is the byte where the next chunk must begin (0 with n_reads 0 when not even the header
 * is whole), and under GC_FASTX_FINAL consumed == len or the call is refused: a truncated file is an error here, unlike FASTQ's lenient end.
 * GC_ERR_INVALID, nothing returned, the device still usable, gc_last_error naming the record's index among the chunk's records (kept or not) and its byte offset in the
 * bytes: a wrong magic where a header is expected; block_size < 32; l_read_name 0 or a name whose last byte is not NUL;
 * 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq > block_size; l_seq >= 2^31; under GC_FASTX_FINAL a header or record that the end of the bytes cuts.
 * GC_ERR_INVALID, checked before a device is needed: a null pointer, unknown flag bits, len (head_len + inflated bytes) of 2^32 - 16 or more.
 * gc_reads_parse_bam_bgzf is to gc_reads_parse_bam what gc_reads_parse_bgzf is to gc_reads_parse: head, the bytes behind the previous call's consumed, then the inflated
 * whole BGZF blocks at the front of data (the end-of-file block of ISIZE 0 among them), put together and decoded in HBM; only *tail comes down.
 * The gc_reads is the object gc_reads_upload builds from the same strings; the table is gc_reads_parse's. stats, if not NULL: the records seen, those left out, and the
 * milliseconds of the walk, of fields and scans, of the ids and of the unpacking (all within table->kernel_ms, which holds the packing kernels too). */
#define GC_BAM_HEADER 2u
typedef struct gc_bam_stats {
	uint64_t records;         /* whole records in the bytes */
	uint64_t skipped;         /* of them, left out for flag 0x100 or 0x800 */
	double walk_ms, fields_ms, names_ms, unpack_ms;
} gc_bam_stats;
int gc_reads_parse_bam(const void* data, uint64_t len, uint32_t flags, gc_reads** reads, gc_fastx_table** table, gc_bam_stats* stats /* may be NULL */);
int gc_reads_parse_bam_bgzf(const void* head, uint64_t head_len, const void* data, uint64_t len, uint32_t flags, gc_reads** reads, gc_fastx_table** table,
                            void** tail, uint64_t* tail_len, uint64_t* consumed, gc_bgzf_stats* stats /* may be NULL */, gc_bam_stats* bam_stats /* may be NULL */);

/* ---- seed hits from the host's own seeder ----------------------------------------------------------- */
/* SeedHit as a seeder hands it over (src/GraphAlignerWrapper.h:14): what Seeder::getSeeds returns whether the hits come from minimizers, MUM / MEM matches or a
 * seeds file (src/Aligner.cpp:87-108), before OrderSeeds. */
typedef struct gc_seed_hit {
	int32_t  node_id;            /* SeedHit::nodeID (bigraph id / 2) */
	uint32_t node_offset;        /* offset in the ORIENTED original node (bigraph id 2*node_id + reverse) */
	uint32_t seq_pos;            /* read position the seed cell is aligned with */
	uint32_t match_len;
	uint32_t raw_goodness;       /* rawSeedGoodness */
	uint32_t reverse;            /* 0 / 1 */
} gc_seed_hit;

/* Uploads and resolves the hits of a read batch: read i has hits[read_hit_off[i] .. read_hit_off[i+1]), in the order its seeder returned them - the reference's unstable sorts
 * are replayed on that order, so it is part of the contract. Every hit is resolved on the device as orderSeedsByChaining does (GetUnitigNode and the split node's offset,
 * src/GraphAligner.h:250-252). The result is read-only and may be shared by streams, like a gc_reads; it belongs to `reads` (same lengths) and to `g`.
 * GC_ERR_INVALID, checked on the host before a device is needed: a null pointer, offsets that do not start at 0 or decrease, n_reads other than the batch's, 2^32 hits or
 * more, a match_len of 2^31 or more, a raw_goodness that could overflow the 32-bit seed goodness (match_len + read length + raw_goodness must stay below 2^32).
 * GC_ERR_INVALID from the device, with the first such hit's read and index in gc_last_error and nothing clamped: a node id that is not in the graph, node_offset >= the
 * original node's size, seq_pos >= the read's length. Hits the reference asserts on (match_len < 2, src/GraphAligner.h:280; chainApproxPos + offset < seq_pos, :253)
 * are accepted here and set the read's failed_assertion in the batch. */
int gc_seeds_upload(const gc_graph* g, const gc_reads* reads, const gc_seed_hit* hits, const uint64_t* read_hit_off /* [n_reads+1] */, uint64_t n_reads, gc_seeds** out);
void gc_seeds_destroy(gc_seeds* s);
/* The raw records of a gc_seeds, read back from HBM: hits[read_hit_off[i] .. read_hit_off[i+1]) are read i's, as uploaded or as gc_seeds_mxm found them. Both arrays are
 * malloc'd (free with gc_free). */
int gc_seeds_hits(const gc_seeds* s, gc_seed_hit** hits, uint64_t** read_hit_off /* [n_reads+1] */, uint64_t* n_reads);
/* Device milliseconds gc_seeds_mxm spent between its first kernel and its last (0 for uploaded seeds). */
double gc_seeds_kernel_ms(const gc_seeds* s);

/* ---- MUM / MEM seeds on the device (replaces MummerSeeder, src/MummerSeeder.cpp; --seeds-mum-count / --seeds-mem-count / --seeds-mxm-length) ---------- */
/* The index: every original segment of g in forward orientation, in ascending node id, each followed by a separator - letters a, c, g, t (u) in either case, anything else a
 * separator - with its full suffix array (separator < a < c < g < t; built on the host by prefix doubling on the library's worker threads), the text packed 2 bits per letter
 * plus a mask, the segment start table and a table from the first 12 letters to a suffix-array interval. In HBM: about 4.3 bytes per text letter plus 4^12 x 8 bytes. 32-bit
 * positions: a text of 2^32 - 16 letters or more is GC_ERR_INVALID. The graph may come from gc_graph_create_from_gfa, gc_graph_create or the index cache; the index is not
 * stored in the gc_index_* cache, and this call builds it on the host every time (gc_mxm_index_open: the device build and a file of its own). Read-only, may be shared by
 * streams; it belongs to g, which must outlive it. */
typedef struct gc_mxm_index gc_mxm_index;
int gc_mxm_index_create(const gc_graph* g, gc_mxm_index** out);
void gc_mxm_index_destroy(gc_mxm_index* x);
/* name in {"sa","node_start","node_id","bytes","build_us","prefix_len","build_mode","build_rounds","build_scratch_bytes","cache_save_us","sa_us"}: the suffix array (text positions), the
 * text position of every segment's first letter (plus the text's length), the segments' node ids, the index's bytes in HBM, the time to produce text and suffix array (a build, or
 * a file read plus verification), the table's letters, how the suffix array came to be (0 host build, 1 device build, 2 loaded from the cache), the doubling rounds of the build
 * after its first sort (0 when loaded), the peak device scratch of a device build (else 0), the time spent writing the cache file (0: none written), of build_us the suffix array alone (0 when loaded); a malloc'd int64 array (free
 * with gc_free). */
int gc_mxm_index_array(const gc_mxm_index* x, const char* name, int64_t** out, uint64_t* count);

/* gc_mxm_index_create with a choice of builder and the reference's --seeds-mxm-cache-prefix (src/AlignerMain.cpp:87,227, src/MummerSeeder.cpp:65-89,137-161: load the index if
 * the cache exists, else build it and save it). gc_mxm_options_default: host build, no cache - what gc_mxm_index_create does.
 *   build          GC_MXM_BUILD_HOST: prefix doubling on the library's worker threads. GC_MXM_BUILD_DEVICE: the same algorithm on the GPU (radix sort of a 21-letter key, then
 *                  doubling rounds over the tied suffixes only); the suffix array is the host's element for element. Its scratch, freed before the call returns, is 29 bytes
 *                  per text letter plus 8 per letter still tied after the first sort. It takes a text of fewer than 2^31 - 1 letters (hipCUB counts in int): a longer one is
 *                  GC_ERR_INVALID, checked on the host - build that one with GC_MXM_BUILD_HOST; nothing falls back by itself.
 *   cache_prefix   NULL or "": no file. Else the file is <prefix>.gcmxm - ONE file in a private format of this library (csrc/host/gc_mxm_cache.hpp), not the reference's
 *                  <prefix>.aux (a boost text archive) and mummer's <prefix>_index files, which cannot be written or read without those libraries. If the file exists it is
 *                  loaded and nothing is built (`build` is not looked at); otherwise the index is built by `build` and saved, through a temporary name in the same directory
 *                  and a rename. The file holds the segment table, the packed text, the raw suffix array (4 bytes per letter), an FNV-1a-64 fingerprint of the text and a
 *                  checksum; the prefix table is rebuilt on the device. A load verifies magic, version, sizes, checksum, tables, suffix-array bounds and the fingerprint and
 *                  segment table against g: any mismatch is GC_ERR_GRAPH with the file and the failure in gc_last_error, and the file is neither used nor overwritten (delete
 *                  it to rebuild). A file that cannot be written is GC_ERR_GRAPH too.
 * GC_ERR_INVALID before a device is needed: a null pointer, another build value, reserved != 0.
 * gc_mxm_cache_check: host only, as gc_index_check is - verifies <prefix>.gcmxm (all of the above but the comparison with a graph; the stored text against its fingerprint
 * instead) and fills info[5] = { version, text letters, segments, file bytes, text fingerprint }; info may be NULL. */
#define GC_MXM_BUILD_HOST   0
#define GC_MXM_BUILD_DEVICE 1
typedef struct gc_mxm_options {
	int32_t build;              /* GC_MXM_BUILD_*; anything else: GC_ERR_INVALID */
	int32_t reserved;           /* must be 0 */
	const char* cache_prefix;   /* --seeds-mxm-cache-prefix; NULL or "": no cache */
} gc_mxm_options;
void gc_mxm_options_default(gc_mxm_options* o);
int gc_mxm_index_open(const gc_graph* g, const gc_mxm_options* o, gc_mxm_index** out);
int gc_mxm_cache_check(const char* cache_prefix, uint64_t* info /* [5] or NULL */);

#define GC_MXM_MUM 1
#define GC_MXM_MEM 2
/* The seeds MummerSeeder::getMumSeeds / getMemSeeds return for every read of the batch, found on the device and resolved there (as gc_seeds_upload resolves): a gc_seeds bound
 * to `reads` and `g` that gc_align_batch_seeded / gc_align_batch_ext take unchanged.
 * A MEM is (p, i, l): l >= min_len, T[p..p+l) == q[i..i+l) over a, c, g, t, and neither side can be extended (i == 0, p == 0 or T[p-1] != q[i-1]; the same at p+l, i+l); the
 * separator and a read letter outside a, c, g, t (u) equal nothing, so a match never leaves a segment. A MUM is mummer's MAM: a MEM whose matched string occurs once in the text
 * (forward segments only; the forward read and its reverse complement are separate queries; uniqueness in the query is not required). A reverse-strand match becomes
 * node_offset = node length - offset - l, seq_pos = read length - i - l, reverse = 1; every hit has raw_goodness = match_len = l.
 * max_count: the longest that many matches of a read over both strands are kept, UINT64_MAX: all. The order of a read's hits, and so which of the equal-length matches at the
 * cut-off stay, is this library's own (the reference's follows mummer's emission order through a priority queue and an unstable sort): match_len descending, forward strand
 * before reverse, query position in the searched orientation ascending, text position ascending.
 * A read with a letter outside the IUPAC alphabet (flagged at upload) gets no hits. GC_ERR_INVALID, checked on the host before a device is needed: a null pointer, another mode,
 * min_len < 2, max_count == 0, an index built from another graph; from the device: 2^31 matches or more in the batch before the cut (split the batch). */
int gc_seeds_mxm(const gc_graph* g, const gc_mxm_index* x, const gc_reads* reads, int32_t mode, uint64_t max_count, uint32_t min_len, gc_seeds** out);

/* ---- seeds from GAM files (replaces -s / --seeds-file: the loop at src/Aligner.cpp:1169-1190, its reader stream::for_each, src/stream.hpp:81-123, and the lookup by read name
 * of Seeder::Mode::File, src/Aligner.cpp:91-94) ---------- */
/* A seed store: every seed of the files, decoded on the device and kept in HBM under a hash of its read's name. A file is a gzip (or zlib) stream, concatenated members read
 * through, of groups `varint64 count`, count x (`varint32 size`, vg::Alignment of size bytes). A first count of 0 ends the file, a later one is an empty group, a size of 0
 * gives no seed, an empty stream has none. The host inflates and finds the message boundaries, piece by piece; neither side ever holds a whole inflated file. One message is
 * one gc_seed_hit, as the reference's lambda builds it (src/Aligner.cpp:1178): node_id = (int32) path.mapping(0).position.node_id, node_offset = ...position.offset, seq_pos =
 * query_position, match_len = raw_goodness = path.mapping(0).edit(0).from_length as uint32, reverse = ...position.is_reverse, stored under `name`, with protobuf's rules for
 * unknown, repeated and merged fields. A node_offset or seq_pos outside 0 .. 2^32 - 2 is stored as 2^32 - 1; nothing is clamped into range (see the join below).
 * In HBM: 48 bytes per seed and its name's bytes.
 * GC_ERR_INVALID, with the file's index and the message's index or byte offset in gc_last_error: a stream that is neither gzip nor zlib or ends inside a member, a count or
 * size that runs past the end of the stream, a message that does not parse (a truncated field, a varint of more than 10 bytes, a group wire type, a length that runs past the
 * message), a message without a mapping, a mapping without an edit, 2^31 - 1 messages or more (hipCUB counts in int). A file that cannot be opened is GC_ERR_GRAPH.
 * Read-only once made; may be shared by streams. */
typedef struct gc_seed_store gc_seed_store;
int gc_seed_store_open(const char* const* paths, uint32_t n_paths, gc_seed_store** out);                                     /* src/Aligner.cpp:1171-1183 */
/* The same from streams that are inflated already (hosts with their own reader, tests). */
int gc_seed_store_from_memory(const void* const* streams, const uint64_t* lens, uint32_t n, gc_seed_store** out);         /* src/stream.hpp:93-116 */
typedef struct gc_seed_store_stats {
	uint64_t messages;          /* size-prefixed messages, the empty ones among them */
	uint64_t seeds;             /* ... that gave a seed */
	uint64_t distinct_hashes;   /* distinct name hashes: the read names of the files, unless two collide */
	uint64_t hbm_bytes;
	double host_ms;             /* inflate_ms + frame_ms */
	double device_ms;           /* decode_ms + sort_ms */
	double inflate_ms, frame_ms, upload_ms, decode_ms, sort_ms;   /* upload: host to device copies and their waits; decode: decode, name scan and name copy kernels */
} gc_seed_store_stats;
int gc_seed_store_info(const gc_seed_store* s, gc_seed_store_stats* out);                                                    /* the reference prints "<n> seeds", :1182 */
void gc_seed_store_destroy(gc_seed_store* s);
/* The seeds of a read batch (src/Aligner.cpp:91-94): read i gets every seed stored under its name - names[name_off[i] .. name_off[i+1] - 1), each name followed by one
 * terminator byte: gc_fastx_table's layout, so the loader's table goes in unchanged - in file order, files in the order they were given; a read without an entry gets none.
 * The names' bytes are compared, not only their hashes. Joined and resolved on the device; the result is an ordinary gc_seeds for gc_align_batch_seeded / gc_align_batch_ext,
 * gc_seeds_hits reads it back and gc_seeds_kernel_ms is the join's device time. GC_ERR_INVALID as gc_seeds_upload documents, naming read and hit. */
int gc_seeds_from_store(const gc_graph* g, const gc_seed_store* store, const gc_reads* reads, const char* names, const uint64_t* name_off /* [n_reads+1] */, uint64_t n_reads, gc_seeds** out);

/* ---- the hot path ---------------------------------------------------------------------------------- */

/* Flat (CSR) result of one batch. All arrays are host memory owned by the result; free with
 * gc_result_free. Node ids are split-node indices unless stated otherwise. */
typedef struct gc_result {
	uint64_t n_reads;
	/* seeds in fragment-pass order: MinimizerSeeder::getSeeds + OrderSeeds + sort by seqPos
	 * (src/Aligner.cpp:660-667) */
	uint64_t* read_seed_off;      /* [n_reads+1] */
	uint32_t* seed_node; uint32_t* seed_offset; uint32_t* seed_seqpos; uint64_t* seed_goodness;
	/* anchors = fragment alignments (src/Aligner.cpp:706-729) */
	uint64_t* read_anchor_off;    /* [n_reads+1] */
	uint32_t* anchor_x; uint32_t* anchor_y;
	uint64_t* anchor_path_off;    /* [n_anchors+1] */
	uint32_t* anchor_path;
	uint32_t* anchor_first_node; uint32_t* anchor_first_offset; uint32_t* anchor_first_seqpos;
	uint32_t* anchor_last_node;  uint32_t* anchor_last_offset;  uint32_t* anchor_last_seqpos;
	int32_t*  anchor_score;
	/* optional traces (keep_traces): bigraph node id, offset in original node, seqPos in the fragment */
	uint64_t* anchor_trace_off;   /* [n_anchors+1] or NULL */
	int32_t*  anchor_trace_node; uint32_t* anchor_trace_offset; uint32_t* anchor_trace_seqpos; uint8_t* anchor_trace_switch;
	/* chain = AlignmentGraph::colinearChaining (src/Aligner.cpp:735): anchor indices local to the read */
	uint64_t* read_chain_off;     /* [n_reads+1] */
	uint32_t* chain;
	uint64_t* chain_score;        /* [n_reads] covered read bases */
	/* whole-read pass (long_pass): all alignments of AlignOneWay(sloppy), src/Aligner.cpp:565 */
	uint64_t* read_longall_off;   /* [n_reads+1] */
	uint32_t* longall_start; uint32_t* longall_end; uint32_t* longall_score;
	uint64_t* long_trace_off;     /* [n_longall+1] */
	int32_t*  long_trace_node; uint32_t* long_trace_offset; uint32_t* long_trace_seqpos; uint8_t* long_trace_switch;
	/* per read flags */
	uint8_t*  failed_assertion;   /* [n_reads] the reference would have thrown on this read */
	uint8_t*  capacity_exceeded;  /* [n_reads] 1: a capacity of THIS library was exceeded for the read (an extension with more tiles than even the
	                               *    retry launch holds, a full cell pool, an NW band beyond the kernel's range, more than 65 536 whole-read alignments -
	                               *    a read starts with max(32, longest read / 512) alignment slots and, when it finds more alignments, runs again with
	                               *    four times as many, up to its number of seeds): its results are incomplete. The reference has no such limits; the batch always
	                               *    completes and every other read is unaffected. */
	uint64_t* seeds_extended;     /* [n_reads] fragment pass (stats.seedsExtended, src/Aligner.cpp:705) */
	uint64_t* seeds_extended_long; /* [n_reads] whole-read pass (AlignmentResult::seedsExtended) */
	/* chain stitching (stitch): the longest stitched piece of the chain (src/Aligner.cpp:754-822) as its split-node
	 * path and the offsets of its first and last base. pathToTrace (src/Aligner.cpp:409-424) expands this to the
	 * reference's `longest` vector, one (node, offset) cell per graph base; path_cells is that vector's size. */
	uint64_t* read_path_off;      /* [n_reads+1] into path_node */
	uint32_t* path_node;
	uint32_t* path_first_offset; uint32_t* path_last_offset;   /* [n_reads] */
	uint64_t* path_cells;         /* [n_reads] */
	/* decision (edit_distances): whole-read alignments kept by SelectAlignments(GreedyLength) (src/Aligner.cpp:636-639) as
	 * indices into the read's longall_* list, best first; the NW edit distance of the best one's path against the read
	 * (:645) and of the stitched path against the read (:845), -1 where there is none; and the test of :901-905 */
	uint64_t* read_long_off;      /* [n_reads+1] */
	uint32_t* long_index;
	int64_t*  long_edit_distance; int64_t* chain_edit_distance;   /* [n_reads] */
	uint8_t*  chained_better;     /* [n_reads] 1: the chained alignment is the read's result, 0: the selected whole-read alignments are */
	/* the chained alignment (chain_traces): its trace in output coordinates like long_trace_* (bigraph node id, offset in the original
	 * node, read position, "next cell is in another split node"), one cell per op of edlib's alignment (src/Aligner.cpp:855-887);
	 * alignmentStart / alignmentEnd (:894-895). Its alignmentScore is chain_edit_distance, its trace score 0 (never set, :739,891).
	 * With gc_params::fast_mode: one cell per base of the stitched piece, and chain_edit_distance is the count of differing letters (see there). */
	uint64_t* read_chain_trace_off; /* [n_reads+1] */
	int32_t*  chain_trace_node; uint32_t* chain_trace_offset; uint32_t* chain_trace_seqpos; uint8_t* chain_trace_switch;
	uint32_t* chain_aln_start; uint32_t* chain_aln_end;   /* [n_reads]; 0,0 where there is no chained alignment */
	/* work counters of the fragment pass: [0] dp tiles, [1] recompute tiles (last-slice flatten + backtrace),
	 * [2] column steps, [3] trace items, [4] extensions, [5] backtrace tiles (subset of [1]);
	 * [6] (r5) times the batch's fragment pipeline ran again because its trace pool or anchor path pool - sized by what the stream's earlier batches used - was too small;
	 * [7] reads whose chain was stitched on the host because it did not fit the stitching kernel's tables */
	uint64_t counters[8];
	uint64_t counters_long[8];    /* the same for the whole-read pass */
	/* device time of each kernel of this batch in microseconds (HIP events on the stream):
	 * [0] seed lookup, [1] fragment extension (k_extend: every lazy round's launches with their retry launches, each between an event pair of its own), [2] anchor build
	 * (k_build_anchors, every round, likewise), [3] chaining, [4] whole-read extension kernels, summed over all
	 * rounds of all read groups (the groups run concurrently on their own streams, so this can exceed the wall clock),
	 * [5] whole-read pass wall clock, first group's start to last group's end (host clock; overlaps 1-3) */
	double kernel_us[8];
	double host_us[4];            /* wall time: [0] host seed glue, [1] result assembly, [2] seed lookup + transfers, [3] extension..chaining + transfers */
	/* Final alignments encoded on the device (params->device_output; NULL otherwise): one entry per alignment the reference would write, in its order
	 * (src/Aligner.cpp:901-920,1003-1023: the chained alignment when it won, else the selected whole-read alignments sorted by alignmentStart).
	 * out_source[k] = 0: the pieces below hold it (GraphAlignerGAFAlignment::traceToAlignment / GraphAlignerVGAlignment::traceToAlignment run on the device);
	 * 1: it is the read's chained alignment, whose trace the host builds (chain_trace_*): the gc_format_* functions encode it from there.
	 * out_numbers[12 k ..]: node path length, start, end (GAF columns 7-9), matches, mismatches, insertions, deletions, trace cells (column 11), alignmentStart,
	 * alignmentEnd, path steps (mappings), alignmentScore. */
	uint64_t* read_out_off;       /* [n_reads+1] */
	uint8_t*  out_source;         /* [n_out] */
	uint64_t* out_numbers;        /* [12 * n_out] */
	uint64_t* out_path_off;  char* out_path_text;     /* [n_out+1]; GAF column 6, e.g. ">12>13<7" (device_output & 3) */
	uint64_t* out_cigar_off; char* out_cigar_text;    /* [n_out+1]; the cg:Z: value (device_output & 3) */
	uint64_t* out_vg_off;    uint8_t* out_vg_path;    /* [n_out+1]; the alignment's vg::Path in proto3 wire format, src/vg.proto:52-109 (device_output & 4) */
	/* r5 (appended: the layout above is unchanged). How often this read exercised the ONE rule this library defines instead of reproducing: the reference's
	 * flattenLastSliceEnd (src/GraphAlignerBitvectorCommon.h:1170-1229) takes the last partial slice's minimum cell with a strict '<' in the iteration order of a
	 * parallel-hashmap (src/NodeSlice.h:54) - a library absent from the reference tree here - so when the minimum is attained in MORE THAN ONE NODE the cell the
	 * reference starts its backtrace from depends on that order; this library takes the node that entered the slice's band first. flatten_ties[r] /
	 * flatten_ties_long[r] = the extensions of read r (fragment pass / whole-read pass; only extensions the reference would have run) with such a tie.
	 * 0 for a read means: nothing in its result depends on the defined order. DESIGN.md §7 says how often a tie changes an output. */
	uint32_t* flatten_ties;       /* [n_reads] */
	uint32_t* flatten_ties_long;  /* [n_reads] */
	int32_t device_output;        /* the gc_params::device_output the batch ran with: gc_format_gaf refuses a cigar_match_mismatch_merge that differs from the pieces' style */
	/* Appended (the layout above is unchanged; NULL unless device_output & 8): the corrected piece of every entry - the graph's letters along its trace, insertions left
	 * out (AddCorrected, src/GraphAligner.h:220-231), as the device spelled them (hip/gc_corrected.hip). Entries with out_source 1 are empty: gc_format_corrected spells
	 * those on the host from chain_trace_*. */
	uint64_t* out_corrected_off;  /* [n_out+1] */
	char*     out_corrected_text;
} gc_result;

/* Runs seeding, fragment seed-extension, anchor construction and co-linear chaining (and, with
 * params->long_pass, the whole-read pass) for every read of the batch. Replaces, per read:
 * MinimizerSeeder::getSeeds, OrderSeeds, AlignOneWay, AlignmentGraph::colinearChaining. */
int gc_align_batch(const gc_graph* g, const gc_seeder* s, gc_stream* st, const gc_reads* reads, const gc_params* params, gc_result** out);
void gc_result_free(gc_result* r);
/* The same from the host's own seed hits (gc_seeds_upload) in place of MinimizerSeeder::getSeeds: OrderSeeds, the fragment windows and everything after them run on those hits,
 * each with its own match_len. No gc_seeder is needed - a host with its own seeds never builds or uploads the minimizer index. params->seed_density is not used (it belongs to
 * MinimizerSeeder::getSeeds); min_cluster_size and everything else behave as in gc_align_batch. Where the reference leaves the order of equal keys inside a seed cluster to
 * std::sort (hits of one cluster at one read position with different match_len) the cluster's matching base pairs follow a stable sort. */
int gc_align_batch_seeded(const gc_graph* g, gc_stream* st, const gc_reads* reads, const gc_seeds* seeds, const gc_params* params, gc_result** out);

/* Extension block of gc_params, whose layout is frozen: options added after it, starting with the reference's --precise-clipping and --X-drop.
 *
 * precise_clipping is preciseClippingIdentityCutoff c, the caller's double bit for bit; the error cost E = c / (1 - c) + 1 (XscoreErrorCost, src/GraphAlignerCommon.h:108) is
 * computed from it in double. With it on, in BOTH extension passes:
 *  - every DP column's maximum X score is taken - max over the column's local minima of (ScoreType)(cells - score * E), a double expression (a rounded product, a rounded
 *    difference) truncated toward zero, over all 64 rows (calculateNodeInner<PreciseClipping = true>, src/GraphAlignerBitvectorCommon.h:971-975,1148-1151; WordSlice::maxXScore,
 *    src/WordSlice.h:223-242,313-336); a slice keeps the first strict maximum in node-pop order with its node (calculateSlice, src/GraphAlignerBitvectorBanded.h:394-398) plus
 *    the slice's first row (fillDPSlice, :456); the initial slice has 0 at the seed's node (...Common.h:1259-1260);
 *  - flattenLastSliceEnd is not called (...Banded.h:414) and removeWronglyAlignedEnd is not called (:51,120); the slice loop (getViterbiSlices) is otherwise unchanged;
 *  - the backtrace starts where getReverseTraceFromTableExactEndPos (...Common.h:321-383) puts it: the slice with the first strict maximum from slice 1 on, its node's tile
 *    recomputed, the largest row inside the read that attains the score (the first column at equal rows); the trace's score is that cell's value; the walk is unchanged.
 *    The assertions at :358,365,377-379 fail the read (failed_assertion), as every assertion of the reference does here;
 *  - the E-value model's identity is c instead of 0.7 (src/Aligner.cpp:474-482): e_cutoff, the alignment selection and the chained alignment's test use it.
 * x_drop is Xdropcutoff: with it on the slice loop is getXdropSlices (...Banded.h:703-830) - every slice at the initial bandwidth, no correctness stop, no ramp, no rewind;
 * the best X score starts at the initial slice's 0; a slice whose score is below best - x_drop is dropped and ends the loop (the first slice dropped: the extension fails);
 * scoresNotValid is set with >= (:768). x_drop > 0 with precise_clipping == 0 runs with c = 0.66 (src/AlignerMain.cpp:443-448; the reference's default, a caller's value is
 * never overridden). x_drop > 0 with gc_params::force_global: GC_ERR_INVALID (getSlices asserts, :504). Ranges: src/AlignerMain.cpp:300-322.
 *
 * What the mode changes in a result: alignments and anchors may end before the read's (fragment's) end, and flatten_ties / flatten_ties_long are 0 - the one rule this
 * library defines instead of reproducing (the order of tied minima in flattenLastSliceEnd) is never reached, so a clipped result follows from the reference's sources alone.
 * The fragment pass runs every extension in the plain-layout kernel (the lockstep kernel does not clip); the whole-read pass keeps its rounds, in the clipping
 * instantiation of its one-extension-per-wave kernel. */
typedef struct gc_params_ext {
	uint32_t struct_size;        /* sizeof(gc_params_ext) of the caller's header; a larger value than the library knows: GC_ERR_INVALID */
	int32_t  x_drop;             /* --X-drop, Xdropcutoff: 0 (default) off, >= 1 on; < 0: GC_ERR_INVALID */
	double   precise_clipping;   /* --precise-clipping, preciseClippingIdentityCutoff: 0 (default) off; else in [0.001, 0.999]; anything else, NaN included: GC_ERR_INVALID */
} gc_params_ext;
void gc_params_ext_default(gc_params_ext* e);
/* gc_align_batch (seeder given, seeds NULL) or gc_align_batch_seeded (seeder NULL, seeds given) with the extension block; both or neither: GC_ERR_INVALID. ext == NULL: the
 * defaults - exactly those two calls. The block and the parameters are checked on the host before anything else is looked at, so an invalid combination is refused
 * with or without a device. */
int gc_align_batch_ext(const gc_graph* g, const gc_seeder* s, gc_stream* st, const gc_reads* reads, const gc_seeds* seeds, const gc_params* params, const gc_params_ext* ext, gc_result** out);

/* gc_result_free keeps the large arrays of freed results (trace cells, output text: up to 24 GB in all) for the next batch's result - fresh memory of that size is
 * mapped and zero-filled page by page every batch otherwise; gc_reads_destroy and the device deflate keep their device / pinned blocks the same way (up to 24 GB and 4 GB per cache).
 * gc_result_cache_trim gives everything that is held back to the allocator (e.g. when a host stops aligning). */
void gc_result_cache_trim(void);

const char* gc_last_error(void);
void gc_free(void* p);
/* Global (NW) edit distance of each pair (a[a_off[i]..a_off[i+1]), b[b_off[i]..b_off[i+1])) on the GPU: the value
 * edlibAlign(a, |a|, b, |b|, edlibNewAlignConfig(-1, EDLIB_MODE_NW, EDLIB_TASK_DISTANCE, NULL, 0)).editDistance returns at
 * src/Aligner.cpp:645 and :845 (characters compare by equality, as in edlib's default alphabet handling). */
int gc_edit_distance(const char* a, const uint64_t* a_off, const char* b, const uint64_t* b_off, uint64_t n_pairs, int64_t* out);
/* The alignment edlibAlign(a, |a|, b, |b|, edlibNewAlignConfig(-1, EDLIB_MODE_NW, EDLIB_TASK_PATH, NULL, 0)) returns at src/Aligner.cpp:845
 * for each pair, on the GPU: distance[i] = editDistance, ops (0 match, 1 letter of a alone, 2 letter of b alone, 3 mismatch) of pair i at
 * ops[ops_off[i] .. ops_off[i] + ops_len[i]); the caller provides ops_off with room for |a_i| + |b_i| ops per pair. ops_len[i] = 0 where
 * edlib returns no alignment (an empty side). edlib's own choice among the optimal alignments is reproduced (Hirschberg split order and
 * traceback preference, edlib/src/edlib.cpp:917-1419). */
int gc_edit_path(const char* a, const uint64_t* a_off, const char* b, const uint64_t* b_off, uint64_t n_pairs, const uint64_t* ops_off, uint8_t* ops, uint32_t* ops_len, int64_t* distance);

/* The E-value --E-cutoff compares (EValueCalculator, src/EValue.cpp; host only, no device needed): out2 = {alignment score, E-value}
 * of an alignment of alignment_length read bases with num_edits edits, for a graph of database_size bp and a read of query_size bp. */
int gc_evalue(double min_identity, uint64_t database_size, uint64_t query_size, uint64_t alignment_length, uint64_t num_edits, double* out2);

/* ---- output ------------------------------------------------------------------------ */

/* GAF text of the batch's final alignments, one line per alignment in the reference's order (AddGAFLine +
 * GraphAlignerGAFAlignment::traceToAlignment, src/GraphAlignerGAFAlignment.h:38-196; the per-read list sorted by
 * alignmentStart, src/Aligner.cpp:1022, written by writeGAFToQueue :300-311). `result` must come from gc_align_batch with
 * long_pass, keep_traces, edit_distances and chain_traces >= 1; bases/offsets are the read batch as given to gc_reads_upload;
 * (or, r4, with device_output instead of keep_traces: the lines are then put together from the pieces the device wrote - no trace comes down);
 * with device_output the pieces' CIGAR style is the one the batch was aligned with: cigar_match_mismatch_merge must agree with it (GC_ERR_INVALID otherwise);
 * read_names[i] is the FASTQ id. A read whose chained alignment won (chained_better) is written from its chain_trace_*
 * (src/Aligner.cpp:901-920); n_chained_skipped counts winners the result holds no trace for (0 unless chain_traces was 0).
 * *out_text is malloc'd (gc_free), NUL-terminated, *out_len bytes long. */
int gc_format_gaf(const gc_graph* g, const gc_result* result, const char* const* read_names, const char* bases, const uint64_t* offsets,
                  int cigar_match_mismatch_merge, char** out_text, uint64_t* out_len, uint64_t* n_chained_skipped);

/* The same alignments as vg::Alignment messages (GraphAlignerVGAlignment::traceToAlignment + AddAlignment +
 * replaceDigraphNodeIdsWithOriginalNodeIds): JSON lines as MessageToJsonString(preserve_proto_field_names) prints them
 * (writeJSONToQueue, src/Aligner.cpp:283-298), or GAM: per read one gzip member holding varint count + (varint size, proto3
 * bytes) per alignment (writeGAMToQueue, src/Aligner.cpp:261-281; the gzip bytes depend on the zlib build, the inflated
 * stream is the reference's). r6: gc_format_gam deflates the members on the device (GC_GAM_DEVICE_LZ below; needs the GPU);
 * gc_format_gam_level(-1) is zlib's default level on the host, the reference's own setting. */
int gc_format_json(const gc_graph* g, const gc_result* result, const char* const* read_names, const char* bases, const uint64_t* offsets,
                   char** out_text, uint64_t* out_len, uint64_t* n_chained_skipped);
int gc_format_gam(const gc_graph* g, const gc_result* result, const char* const* read_names, const char* bases, const uint64_t* offsets,
                  char** out_bytes, uint64_t* out_len, uint64_t* n_chained_skipped);

/* One alignment at a time, for a host that keeps the reference's per-alignment output calls (src/GraphAlignerWrapper.h:43-44; include/graphchainer_amd_shim.hpp
 * forwards AddGAFLine / AddAlignment here). The trace is in output coordinates (bigraph node id, offset in the original node, read position, "the next cell is in
 * another split node": long_trace_* / chain_trace_* / anchor_trace_* of a gc_result, or a reference OnewayTrace). Host code, no device work; free the output with gc_free.
 *   gc_format_gaf_trace  GraphAlignerGAFAlignment::traceToAlignment (src/GraphAlignerGAFAlignment.h:38-196): the GAF line, no newline.
 *   gc_format_vg_trace   GraphAlignerVGAlignment::traceToAlignment + AddAlignment's sequence / query_position + replaceDigraphNodeIdsWithOriginalNodeIds
 *                        (src/GraphAlignerVGAlignment.h:36-163, src/GraphAligner.h:205-212, src/Aligner.cpp:152-165): the vg::Alignment message, proto3 wire bytes.
 *   gc_format_vg_trace_digraph   the same message as AddAlignment alone leaves it (src/GraphAligner.h:205-212): position.node_id = the digraph node id (2 x segment index
 *                        + strand) and no position.name - for a host that keeps the reference's own call to replaceDigraphNodeIdsWithOriginalNodeIds right after AddAlignment
 *                        (src/Aligner.cpp:1009; include/graphchainer_amd_shim.hpp's AddAlignment goes here, so that an unchanged src/Aligner.cpp:1006-1012 gives the reference's ids).
 *   gc_graph_letters     the graph letter under each (node id, offset): TraceItem's graphCharacter (src/GraphAlignerCommon.h:148-153). */
int gc_format_gaf_trace(const gc_graph* g, const char* read_name, const char* sequence, uint64_t sequence_len, const int32_t* node, const uint32_t* offset, const uint32_t* seqpos,
                        const uint8_t* node_switch, uint64_t n, int cigar_match_mismatch_merge, char** out_text, uint64_t* out_len);
int gc_format_vg_trace(const gc_graph* g, const char* read_name, const char* sequence, uint64_t sequence_len, const int32_t* node, const uint32_t* offset, const uint32_t* seqpos,
                       const uint8_t* node_switch, uint64_t n, int32_t score, uint64_t alignment_start, uint64_t alignment_end, char** out_bytes, uint64_t* out_len);
int gc_format_vg_trace_digraph(const gc_graph* g, const char* read_name, const char* sequence, uint64_t sequence_len, const int32_t* node, const uint32_t* offset, const uint32_t* seqpos,
                               const uint8_t* node_switch, uint64_t n, int32_t score, uint64_t alignment_start, uint64_t alignment_end, char** out_bytes, uint64_t* out_len);
int gc_graph_letters(const gc_graph* g, const int32_t* node, const uint32_t* offset, uint64_t n, char* out);

/* Corrected reads: GraphAligner's --corrected-out and --corrected-clipped-out (the mechanism the reference still carries: AddCorrected src/GraphAligner.h:220-231,
 * getCorrected src/ReadCorrection.cpp:38-64, writeCorrectedToQueue / writeCorrectedClippedToQueue src/Aligner.cpp:313-374,984,1037,1050-1051).
 * An alignment's piece is the graph letter (TraceItem::graphCharacter, what gc_graph_letters returns: IUPAC codes and the N of an all-zero column included) of its first
 * trace cell, then of every cell that is not an insertion: cell i adds nothing when cell i-1 is not flagged nodeSwitch and cell i stands on its node and offset.
 * clipped == 0: one record per read, ">" id "\n" body "\n", the id being the whole read_names[i]; the body takes the read's alignments in the result's output order
 * (read_out_off) with currentEnd = 0: tolower(raw[currentEnd:start]) when start > currentEnd, then toupper(piece), currentEnd = end (even when that moves it backwards),
 * and tolower(raw[currentEnd:]) after the last. maxOverlap is getDBGoverlap, 0 for the graphs this library loads: nothing is trimmed where start < currentEnd. A read
 * without alignments gives its lower-cased self; a flagged read (failed_assertion, capacity_exceeded) gives no record. raw = bases[offsets[i] .. offsets[i+1]).
 * clipped != 0: one record per alignment, ">" id "_" i "_" start "_" end "\n" piece "\n", i counting within the read's output list.
 * Works from the device's pieces (device_output & 8) for out_source 0 and spells chained winners on the host from chain_trace_*; without the bit it works from a
 * keep_traces result (long_pass, edit_distances, chain_traces >= 1), everything spelled on the host. rec_off (may be NULL): malloc'd [*n_rec + 1] byte offsets of the
 * records in *out_text, for a host that compresses them one by one. n_chained_skipped counts winners the result holds no trace for. Free both with gc_free. */
int gc_format_corrected(const gc_graph* g, const gc_result* result, const char* const* read_names, const char* bases, const uint64_t* offsets, int clipped,
                        char** out_text, uint64_t* out_len, uint64_t** rec_off, uint64_t* n_rec, uint64_t* n_chained_skipped);
/* One alignment's piece from its trace on the host (beside gc_format_gaf_trace; no device work): *out_text malloc'd, NUL-terminated, *out_len letters. */
int gc_format_corrected_trace(const gc_graph* g, const int32_t* node, const uint32_t* offset, const uint8_t* node_switch, uint64_t n, char** out_text, uint64_t* out_len);
/* The device kernels over a caller's own traces (a host that keeps its traces; the tests, which need exact shapes): alignment a is cells trace_off[a] .. trace_off[a+1]
 * of node / offset / node_switch; *out_text holds the pieces back to back, piece a at (*out_off)[a] .. (*out_off)[a+1] (n_aln + 1 entries). Every (node, offset) is
 * checked against the graph first (GC_ERR_INVALID). Free both with gc_free. */
int gc_corrected_pieces(const gc_graph* g, const int32_t* node, const uint32_t* offset, const uint8_t* node_switch, const uint64_t* trace_off, uint64_t n_aln,
                        char** out_text, uint64_t** out_off);

/* Coverage: how often every segment and every base of the graph lies under a final alignment (--coverage-out / --base-coverage-out). This library's own; the reference has
 * no counterpart, so the meaning is defined here. The alignments counted are the entries of gc_result::out_* - the set and order of the GAF lines: the chained alignment where
 * it won, otherwise the selected whole-read alignments; flagged reads count nothing. Each is a trace of cells (node, offset) in output coordinates. Cell i covers the graph
 * base under it iff i == 0 or (node, offset) differs from cell i-1's: insertions cover nothing, matches, mismatches and deletions one base each. The base is reported on
 * segment node / 2 (the internal segment number: the order in which the GFA first names them) in forward coordinates: offset for an even id, length - 1 - offset for an odd one.
 * depth[segment][pos] = covering cells over all counted alignments, bases[segment] = the sum of its depth. This is what the vg JSON of the same run shows: every mapping
 * covers [position.offset, position.offset + sum of from_length) of its node in its orientation.
 * The accumulators live on the device the handle was created on (the current one) and across batches: bases is 8 bytes per segment; depth, only with per_base != 0, 4 bytes per
 * forward base (gc_graph_size_bp / 2: 20 MB at 5 Mbp, 12.4 GB at 3.1 Gbp) - when that does not fit, GC_ERR_DEVICE and gc_last_error says how much was asked for. A host sizing
 * its batches by gc_device_memory creates the handle first. All counts are integers added with atomics: they do not depend on the order of the batches or of anything inside one.
 * Limit: a depth word holds 2^32 - 1 and stays there once it is reached, in a batch's additions and in gc_coverage_merge.
 * The graph must outlive the handle. */
typedef struct gc_coverage gc_coverage;
int gc_coverage_create(const gc_graph* g, int per_base, gc_coverage** out);
void gc_coverage_destroy(gc_coverage* cov);
/* From now on every batch aligned on the stream with device_output != 0 (which needs long_pass and edit_distances) is counted into cov before its call returns: a finished batch is
 * a counted batch. The winners' traces are made for it whatever chain_traces says. NULL turns it off. Several streams of one device may share a handle - that is the batches in
 * flight; the handle must live on the stream's device (GC_ERR_INVALID) and outlive its use. */
int gc_stream_set_coverage(gc_stream* stream, gc_coverage* cov);
/* The same kernel over a caller's own traces (a host that keeps its traces; the tests, which need exact shapes): alignment a is cells trace_off[a] .. trace_off[a+1] of
 * node / offset. Every (node, offset) is checked against the graph first (GC_ERR_INVALID, nothing counted). Returns when the counts are in. */
int gc_coverage_add_traces(gc_coverage* cov, const int32_t* node, const uint32_t* offset, const uint64_t* trace_off, uint64_t n_aln);
/* The counts as they stand: *bases malloc'd [*n_segments]; *depth malloc'd [*n_bases], segment after segment in forward coordinates, or NULL without per_base. Free with gc_free.
 * This and the calls below read the accumulators: no batch may be in flight on a stream set to the handle. */
int gc_coverage_counts(gc_coverage* cov, uint64_t** bases, uint64_t* n_segments, uint32_t** depth, uint64_t* n_bases);
/* dst += src. One device or two (two go through the host, the depth in slices). Handles for graphs of different shape, or only one of them per_base: GC_ERR_INVALID. */
int gc_coverage_merge(gc_coverage* dst, const gc_coverage* src);
/* The two tables, spelled on the device; only text comes down. Segments: "#segment\tlength\tbases\n", then one line per segment, zero rows included, in ascending segment number;
 * the name is the GFA's, or the number where that is empty, as the GAF path prints it. Bases (per_base handles): "segment\tstart\tend\tdepth\n" without a head line, 0-based
 * half-open forward coordinates, one line per maximal run of equal non-zero depth inside one segment, segments ascending, runs ascending within a segment.
 * *text malloc'd, NUL-terminated, *len bytes; *line_off (may be NULL) malloc'd [*n_lines + 1] byte offsets of the lines, the head line counted, for a host that compresses
 * the text in pieces of whole lines. Free both with gc_free. */
int gc_coverage_format_segments(gc_coverage* cov, char** text, uint64_t* len, uint64_t** line_off, uint64_t* n_lines);
int gc_coverage_format_bases(gc_coverage* cov, char** text, uint64_t* len, uint64_t** line_off, uint64_t* n_lines);

/* Link coverage: which links the counted alignments walk (--link-coverage-out / --coverage-gfa-out / --supported-subgraph-out). This library's own as well. The alignments
 * counted are the same. Cell i > 0 of a trace is a traversal iff node[i] != node[i-1]; it walks the directed pair (u, v) = (node[i-1], node[i]) of bigraph ids
 * (2 * segment + strand). An insertion cell repeats its predecessor's position and never traverses; the graph is a DAG, so an alignment walks a link at most once.
 * The mate of (u, v) is (v ^ 1, u ^ 1), the same link read on the other strand; the canonical form of a pair is the lexicographically smaller of the pair and its mate
 * (a hairpin (u, u ^ 1) is its own mate). The graph's links are the distinct canonical forms of all (nodeIDs[x], nodeIDs[y]) with y an out-neighbour of split node x and
 * nodeIDs[x] != nodeIDs[y], numbered in ascending canonical (u, v); they are taken from the handle's host graph (after gc_graph_create, gc_graph_create_from_gfa or
 * gc_index_load alike, and after gc_graph_trim_host). traversals[link] = the traversals over all counted alignments whose canonical form is that link.
 * gc_coverage_create2 is gc_coverage_create with flags: GC_COVERAGE_LINKS builds the link table once and keeps it on the device, 16 bytes per link (the sorted keys
 * u << 32 | v and a 64-bit counter each); GC_ERR_DEVICE when that does not fit. Without the flag nothing here costs anything: the batches' counting kernel is then the one
 * without the traversal step. */
#define GC_COVERAGE_PER_BASE 1u
#define GC_COVERAGE_LINKS 2u
int gc_coverage_create2(const gc_graph* g, unsigned flags, gc_coverage** out);
/* On a handle with links gc_coverage_add_traces additionally checks every traversal before anything is counted: the predecessor's offset is its segment's last base in that
 * orientation, the new offset is 0, and the pair is a link of the graph - otherwise GC_ERR_INVALID and nothing is counted, segments included.
 * gc_coverage_merge adds the link counters too; handles of which only one has links: GC_ERR_INVALID.
 * The links as they stand: *from / *to malloc'd [*n_links] canonical bigraph ids in link order, *traversals malloc'd [*n_links]. Free with gc_free. */
int gc_coverage_link_counts(gc_coverage* cov, int32_t** from, int32_t** to, uint64_t** traversals, uint64_t* n_links);
/* Three more texts spelled on the device, each over rows [first, first + count) (count is cut at the table's end; first behind it: GC_ERR_INVALID), so that the caller bounds
 * the text one call makes; text, len, line_off and n_lines as above.
 * Links: "from\tfrom_orient\tto\tto_orient\ttraversals\n" per link, zero rows included, in link order; the call with first == 0 puts the head line
 * "#from\tfrom_orient\tto\tto_orient\ttraversals\n" in front (counted in n_lines). A canonical (u, v) is spelled name(u >> 1), + for even u and - for odd, name(v >> 1) and
 * likewise for v; a segment without a name prints its number.
 * GFA segments (any handle): "S\tname\tLETTERS\tLN:i:<length>\tRC:i:<bases>\n" per segment in ascending segment number; LETTERS is the forward strand read from the graph on
 * the device, upper case, the IUPAC code where a base is ambiguous; RC is the segment's bases count (RC / LN = its mean depth).
 * GFA links: "L\tfrom\t+-\tto\t+-\t0M\tRC:i:<traversals>\n" per link in link order.
 * supported_only != 0 leaves out the segments with bases == 0 / the links with traversals == 0 (n_lines counts the lines written). A link that is kept has both its
 * segments kept: a traversal covers a base on either side. */
int gc_coverage_format_links(gc_coverage* cov, uint64_t first, uint64_t count, char** text, uint64_t* len, uint64_t** line_off, uint64_t* n_lines);
int gc_coverage_format_gfa_segments(gc_coverage* cov, uint64_t first, uint64_t count, int supported_only, char** text, uint64_t* len, uint64_t** line_off, uint64_t* n_lines);
int gc_coverage_format_gfa_links(gc_coverage* cov, uint64_t first, uint64_t count, int supported_only, char** text, uint64_t* len, uint64_t** line_off, uint64_t* n_lines);

/* Pileup: at which bases the counted alignments disagree with the graph, and how (--pileup-out). This library's own as well; the alignments counted are exactly those the
 * coverage counts, the entries of gc_result::out_*. For cell i of a trace, with `covers` as above (i == 0 or (node, offset) differs from cell i-1's) and `moved` = (i == 0 or
 * seqPos differs from cell i-1's):
 *   covers and moved   an aligned pair: read letter read[seqPos], graph letter under the cell. A match iff their IUPAC sets intersect (the test the GAF's CIGAR makes; a read
 *                      byte that is no nucleotide code has the empty set), otherwise a mismatch, counted in the channel of the read letter on the forward strand
 *   covers only        a deletion: a graph base that no read base stands on
 *   moved only         an insertion: a read base standing on the base of the cell before
 *   neither            nothing
 * The base is the one the coverage reports: segment node / 2, forward coordinate. On an odd node id the read letter is complemented before it picks its channel. The
 * single-letter sets A, C, G, T/U (either case) go to mmA, mmC, mmG, mmT, every other read letter to mmN. An insertion on an even id counts into ins_after of its base (it lies
 * behind that base on the forward strand), one on an odd id into ins_before.
 * A row is eight 32-bit channels per forward base in the order mmA mmC mmG mmT mmN del ins_after ins_before; each holds 2^32 - 1 and stays there once it is reached, in a
 * batch's additions and in gc_coverage_merge, like the depth word. depth[b] = matches + mmA + mmC + mmG + mmT + mmN + del, so the table prints match = depth - those six and
 * GC_COVERAGE_PILEUP implies GC_COVERAGE_PER_BASE: 4 + 32 = 36 bytes per forward base on the handle's device (GC_ERR_DEVICE with the bytes asked for when the rows do not fit).
 * A cell whose seqPos is not below its read's length is counted in no channel and raises bit 8 (0x100) of the handle's flag word: the next call that reads the handle fails.
 * A batch's own cells never do; a caller's are refused on the host before anything is launched. */
#define GC_COVERAGE_PILEUP 4u
/* gc_coverage_add_traces with the reads: cell i has read position seq_pos[i] in the read of its alignment a, bases[read_off[a] .. read_off[a+1]) (read_off[0] == 0, ascending).
 * Every cell is checked on the host first, seq_pos < the read's length included (GC_ERR_INVALID, nothing counted). Any handle takes it; a handle with the pileup takes only
 * this one: the call without reads answers GC_ERR_INVALID there. */
int gc_coverage_add_traces2(gc_coverage* cov, const int32_t* node, const uint32_t* offset, const uint32_t* seq_pos, const uint64_t* trace_off, uint64_t n_aln,
                            const char* bases, const uint64_t* read_off);
/* The rows as they stand: *rows malloc'd [8 * *n_bases], base after base in the order of gc_coverage_counts' depth. Free with gc_free. */
int gc_coverage_pileup_counts(gc_coverage* cov, uint32_t** rows, uint64_t* n_bases);
/* The table, spelled on the device, over forward bases [first_base, first_base + count) in the order of depth (count is cut at the end; first_base behind it:
 * GC_ERR_INVALID; fewer than 2^31 bases per call): "segment\tpos\tref\tdepth\tmatch\tmmA\tmmC\tmmG\tmmT\tmmN\tdel\tins_before\tins_after\n" for every base with depth > 0,
 * alt >= min_alt and (double)alt >= min_fraction * (double)depth, where alt is the largest of the eight channels (min_alt 0 and min_fraction 0: every covered base;
 * min_fraction outside [0, 1]: GC_ERR_INVALID). pos is 0-based forward, ref the graph's letter in upper case as the GFA segments spell it. The call with first_base == 0 puts
 * the same line with a leading '#' in front as the head line (counted in n_lines). text, len, line_off and n_lines as above.
 * gc_coverage_merge adds the rows too; handles of which only one has the pileup: GC_ERR_INVALID. */
int gc_coverage_format_pileup(gc_coverage* cov, uint64_t first_base, uint64_t count, uint64_t min_alt, double min_fraction,
                              char** text, uint64_t* len, uint64_t** line_off, uint64_t* n_lines);

/* gc_format_gam with the zlib level of the gzip members chosen by the caller (-1 = Z_DEFAULT_COMPRESSION, what the reference's GzipOutputStream uses and gc_format_gam
 * gives; 0..9). The inflated stream is the same at every level; deflate at the default level costs ~1 ms of CPU per 10 kb read - more than the whole alignment costs the
 * GPU - so a host that writes GAM at the hot path's rate wants level 1 (or its own compressor on the bytes of level 0), or GC_GAM_DEVICE_HUFFMAN: the members are then
 * deflated on the device, every read's group as one dynamic-Huffman block of literals (no LZ77 matches: a larger file than zlib's, the same inflated stream, and the host
 * only frames the members and computes their CRC-32s). */
#define GC_GAM_DEVICE_HUFFMAN 100
/* r6: the same with LZ77 matches in front of the Huffman stage (one probe of a hash of 4-byte prefixes per position, greedy parse): ~1.2 x zlib's default bytes instead of 2 x,
 * the same inflated stream; what the reference's GzipOutputStream costs the host (src/Aligner.cpp:261-281) stays on the device. */
#define GC_GAM_DEVICE_LZ 101
int gc_format_gam_level(const gc_graph* g, const gc_result* result, const char* const* read_names, const char* bases, const uint64_t* offsets, int level,
                        char** out_bytes, uint64_t* out_len, uint64_t* n_chained_skipped);

/* The device deflate behind GC_GAM_DEVICE_HUFFMAN on the caller's own byte streams: stream i = bytes[offsets[i] .. offsets[i+1]) becomes the gzip member
 * out_bytes[out_offsets[i] .. out_offsets[i+1]) (out_offsets: n + 1 entries, caller's; out_bytes: gc_free). */
int gc_gzip_streams(const uint8_t* bytes, const uint64_t* offsets, uint64_t n, char** out_bytes, uint64_t* out_offsets);
/* ... and the deflate behind GC_GAM_DEVICE_LZ (r6; no counterpart in the reference: its gzip layer is protobuf's GzipOutputStream, src/Aligner.cpp:261-281) */
int gc_gzip_streams_lz(const uint8_t* bytes, const uint64_t* offsets, uint64_t n, char** out_bytes, uint64_t* out_offsets);

/* Test entry (no counterpart in the reference): the permutation the device's replay of libstdc++'s std::sort gives for arrays of 32-bit keys. The reference feeds three UNSTABLE
 * std::sort calls into order-sensitive logic (src/MinimizerSeeder.cpp:497, src/GraphAligner.h:293, src/Aligner.cpp:667), so the permutation libstdc++ produces for equal keys is
 * part of its behaviour; the seed kernels replay that algorithm on the 64 lanes of a wave (csrc/hip/gc_stdsort_wave.hpp) and the tests hold this entry against the local std::sort.
 * Array s = keys[offsets[s] .. offsets[s + 1]); perm_out[offsets[s] + i] = index inside its array of the element that ends at place i. depth_limit < 0: the reference's
 * 2 floor(log2 n); a small value forces introsort's heapsort path. */
int gc_std_sort_permutations(const uint32_t* keys, const uint64_t* offsets, uint64_t n_arrays, int64_t depth_limit, uint32_t* perm_out);

/* Test entry (no counterpart in the reference): the extension kernels' maximum X score (the local-minima form) of n DP columns (vp, vn, score_end: WordSlice's VP, VN, scoreEnd) over their
 * first `cells` rows (1..64) with the error cost given as a double - WordSlice::maxXScoreFirstSlices on the device, where a fused multiply-subtract would round differently. */
int gc_test_max_x_score(const uint64_t* vp, const uint64_t* vn, const int32_t* score_end, uint64_t n, double error_cost, int32_t cells, int32_t* out);

int gc_device_count(void);
int gc_set_device(int device);
/* free / total bytes of the current device's memory (a host that sizes its batches: a 10 k x 10 kb batch in flight holds ~19 GB, a 2 k x 50 kb batch 28-42 GB, beside the device's shared whole-read scratch of 21-27 GB - two of them when small batches run two passes side by side) */
int gc_device_memory(uint64_t* free_bytes, uint64_t* total_bytes);

#ifdef __cplusplus
}
#endif
#endif
