"""Python host side of the MI355X GraphChainer hot path.

Thin ctypes layer over the C ABI (include/graphchainer_amd.h, built into graphchainer_amd/libgraphchainer_amd.so).
Class and method names mirror the reference objects they stand in for:

  AlignmentGraph   <- AlignmentGraph + buildMPC          (src/AlignmentGraph.h, src/Aligner.cpp:1137-1156)
  MinimizerSeeder  <- MinimizerSeeder                    (src/MinimizerSeeder.h:32)
  Aligner.align_reads(reads) <- the per-read body of runComponentMappings (src/Aligner.cpp:601-922), batched

There is no CPU fallback: if the HIP library is missing or no GPU is visible these raise.
"""
import ctypes as C
import os
import zlib

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GC_LIBRARY") or os.path.join(_HERE, "libgraphchainer_amd.so")   # GC_LIBRARY: profiling builds (make stamps)

EXPORTED_SYMBOLS = [
    "gc_params_default", "gc_graph_create_from_gfa", "gc_graph_create", "gc_graph_destroy", "gc_graph_num_nodes",
    "gc_graph_size_bp", "gc_graph_array", "gc_graph_trim_host", "gc_seeder_create", "gc_seeder_destroy", "gc_seeder_array",
    "gc_stream_create", "gc_stream_destroy", "gc_reads_upload", "gc_reads_destroy", "gc_align_batch",
    "gc_seeds_upload", "gc_seeds_destroy", "gc_seeds_hits", "gc_seeds_kernel_ms", "gc_mxm_index_create", "gc_mxm_options_default", "gc_mxm_index_open", "gc_mxm_cache_check", "gc_mxm_index_destroy", "gc_mxm_index_array", "gc_seeds_mxm", "gc_align_batch_seeded", "gc_params_ext_default", "gc_align_batch_ext", "gc_test_max_x_score",
    "gc_result_free", "gc_last_error", "gc_free", "gc_device_count", "gc_set_device", "gc_device_memory", "gc_edit_distance", "gc_edit_path", "gc_evalue", "gc_format_gaf", "gc_format_json", "gc_format_gam", "gc_format_gam_level", "gc_gzip_streams", "gc_gzip_streams_lz", "gc_format_gaf_trace", "gc_format_vg_trace", "gc_format_vg_trace_digraph", "gc_graph_letters", "gc_std_sort_permutations",
    "gc_format_corrected", "gc_format_corrected_trace", "gc_corrected_pieces",
    "gc_coverage_create", "gc_coverage_destroy", "gc_stream_set_coverage", "gc_coverage_add_traces", "gc_coverage_counts", "gc_coverage_merge",
    "gc_coverage_format_segments", "gc_coverage_format_bases",
    "gc_coverage_link_counts", "gc_coverage_format_links", "gc_coverage_format_gfa_segments", "gc_coverage_format_gfa_links",
    "gc_coverage_pileup_counts", "gc_coverage_format_pileup",
    "gc_index_build", "gc_index_save", "gc_index_load", "gc_index_check", "gc_result_cache_trim",
    "gc_reads_parse", "gc_fastx_table_free", "gc_bgzf_inflate", "gc_reads_parse_bgzf", "gc_reads_parse_bam", "gc_reads_parse_bam_bgzf",
    "gc_seed_store_open", "gc_seed_store_from_memory", "gc_seed_store_info", "gc_seed_store_destroy", "gc_seeds_from_store",
]
EXPORTED_SYMBOLS_NUMBERED = ["gc_coverage_create2", "gc_coverage_add_traces2"]   # declared in the header too; apart because tests/test_library_exports.py reads the header for names of letters and underscores only
GC_COVERAGE_PER_BASE, GC_COVERAGE_LINKS, GC_COVERAGE_PILEUP = 1, 2, 4
PILEUP_CHANNELS = ("mmA", "mmC", "mmG", "mmT", "mmN", "del", "ins_after", "ins_before")   # the columns of Coverage.pileup_counts
PILEUP_PIECE_BASES = 1 << 20         # Coverage.pileup_pieces: forward bases per call into the library (a line is some 40 bytes)
GFA_PIECE_BYTES = 64 << 20           # Coverage.gfa_pieces / link_table: about this much text per call into the library


class GcCapacities(C.Structure):
    """gc_capacities (include/graphchainer_amd.h): sizes of the device-side tables; 0 = automatic."""
    _fields_ = [("ext_max_items", C.c_int64), ("ext_max_pending", C.c_int64), ("ext_max_trace", C.c_int64), ("long_max_items", C.c_int64), ("long_column_store", C.c_int64),
                ("long_cells_per_base", C.c_int64), ("long_scratch_bytes", C.c_int64), ("stitch_set_max", C.c_int64), ("stitch_bfs_cap", C.c_int64), ("reserved", C.c_int64 * 3)]


class GcParamsExt(C.Structure):
    """gc_params_ext (include/graphchainer_amd.h): the options added after gc_params' layout was frozen."""
    _fields_ = [("struct_size", C.c_uint32), ("x_drop", C.c_int32), ("precise_clipping", C.c_double)]


class GcParams(C.Structure):
    _fields_ = [("bandwidth", C.c_int32), ("split_len", C.c_int32), ("split_gap", C.c_int32), ("colinear_gap", C.c_int64),
                ("seed_density", C.c_double), ("min_cluster_size", C.c_int32), ("long_pass", C.c_int32), ("keep_traces", C.c_int32), ("keep_seeds", C.c_int32), ("stitch", C.c_int32), ("edit_distances", C.c_int32),
                ("chain_traces", C.c_int32), ("device_output", C.c_int32), ("e_cutoff", C.c_double), ("capacity", GcCapacities),
                ("ramp_bandwidth", C.c_int32), ("max_cells_per_slice", C.c_int64), ("force_global", C.c_int32),
                ("seed_extend_density", C.c_double), ("extra_heuristic", C.c_int32), ("colinear_chaining", C.c_int32), ("selection_method", C.c_int32), ("fast_mode", C.c_int32)]


# gc_params::selection_method: the reference's SelectionMethod in its own order (GC_SELECT_* of include/graphchainer_amd.h)
SELECT_GREEDY_LENGTH, SELECT_GREEDY_SCORE, SELECT_GREEDY_E, SELECT_SCHEDULE_INVERSE_E_SUM, SELECT_SCHEDULE_INVERSE_E_PRODUCT, SELECT_SCHEDULE_SCORE, SELECT_SCHEDULE_LENGTH, SELECT_ALL = range(8)


_P = C.POINTER


class GcResult(C.Structure):
    _fields_ = [
        ("n_reads", C.c_uint64),
        ("read_seed_off", _P(C.c_uint64)), ("seed_node", _P(C.c_uint32)), ("seed_offset", _P(C.c_uint32)), ("seed_seqpos", _P(C.c_uint32)), ("seed_goodness", _P(C.c_uint64)),
        ("read_anchor_off", _P(C.c_uint64)), ("anchor_x", _P(C.c_uint32)), ("anchor_y", _P(C.c_uint32)),
        ("anchor_path_off", _P(C.c_uint64)), ("anchor_path", _P(C.c_uint32)),
        ("anchor_first_node", _P(C.c_uint32)), ("anchor_first_offset", _P(C.c_uint32)), ("anchor_first_seqpos", _P(C.c_uint32)),
        ("anchor_last_node", _P(C.c_uint32)), ("anchor_last_offset", _P(C.c_uint32)), ("anchor_last_seqpos", _P(C.c_uint32)),
        ("anchor_score", _P(C.c_int32)),
        ("anchor_trace_off", _P(C.c_uint64)), ("anchor_trace_node", _P(C.c_int32)), ("anchor_trace_offset", _P(C.c_uint32)),
        ("anchor_trace_seqpos", _P(C.c_uint32)), ("anchor_trace_switch", _P(C.c_uint8)),
        ("read_chain_off", _P(C.c_uint64)), ("chain", _P(C.c_uint32)), ("chain_score", _P(C.c_uint64)),
        ("read_longall_off", _P(C.c_uint64)), ("longall_start", _P(C.c_uint32)), ("longall_end", _P(C.c_uint32)), ("longall_score", _P(C.c_uint32)),
        ("long_trace_off", _P(C.c_uint64)), ("long_trace_node", _P(C.c_int32)), ("long_trace_offset", _P(C.c_uint32)),
        ("long_trace_seqpos", _P(C.c_uint32)), ("long_trace_switch", _P(C.c_uint8)),
        ("failed_assertion", _P(C.c_uint8)), ("capacity_exceeded", _P(C.c_uint8)), ("seeds_extended", _P(C.c_uint64)), ("seeds_extended_long", _P(C.c_uint64)),
        ("read_path_off", _P(C.c_uint64)), ("path_node", _P(C.c_uint32)), ("path_first_offset", _P(C.c_uint32)), ("path_last_offset", _P(C.c_uint32)), ("path_cells", _P(C.c_uint64)),
        ("read_long_off", _P(C.c_uint64)), ("long_index", _P(C.c_uint32)), ("long_edit_distance", _P(C.c_int64)), ("chain_edit_distance", _P(C.c_int64)), ("chained_better", _P(C.c_uint8)),
        ("read_chain_trace_off", _P(C.c_uint64)), ("chain_trace_node", _P(C.c_int32)), ("chain_trace_offset", _P(C.c_uint32)), ("chain_trace_seqpos", _P(C.c_uint32)), ("chain_trace_switch", _P(C.c_uint8)),
        ("chain_aln_start", _P(C.c_uint32)), ("chain_aln_end", _P(C.c_uint32)),
        ("counters", C.c_uint64 * 8), ("counters_long", C.c_uint64 * 8), ("kernel_us", C.c_double * 8), ("host_us", C.c_double * 4),
        ("read_out_off", _P(C.c_uint64)), ("out_source", _P(C.c_uint8)), ("out_numbers", _P(C.c_uint64)),
        ("out_path_off", _P(C.c_uint64)), ("out_path_text", _P(C.c_char)), ("out_cigar_off", _P(C.c_uint64)), ("out_cigar_text", _P(C.c_char)),
        ("out_vg_off", _P(C.c_uint64)), ("out_vg_path", _P(C.c_uint8)),
        ("flatten_ties", _P(C.c_uint32)), ("flatten_ties_long", _P(C.c_uint32)), ("device_output", C.c_int32),
        ("out_corrected_off", _P(C.c_uint64)), ("out_corrected_text", _P(C.c_char)),
    ]


_lib = None


def load_library():
    """Loads the in-tree HIP library; fails loudly if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C graphchainer_amd/csrc` (or __graft_entry__.build())")
    lib = C.CDLL(LIB_PATH)
    lib.gc_last_error.restype = C.c_char_p
    lib.gc_graph_create_from_gfa.argtypes = [C.c_char_p, _P(C.c_void_p)]
    lib.gc_graph_destroy.argtypes = [C.c_void_p]
    lib.gc_graph_num_nodes.restype = C.c_uint64
    lib.gc_graph_num_nodes.argtypes = [C.c_void_p]
    lib.gc_graph_size_bp.restype = C.c_uint64
    lib.gc_graph_size_bp.argtypes = [C.c_void_p]
    lib.gc_graph_array.argtypes = [C.c_void_p, C.c_char_p, _P(_P(C.c_int64)), _P(C.c_uint64)]
    lib.gc_graph_trim_host.argtypes = [C.c_void_p]
    lib.gc_seeder_create.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_double, _P(C.c_void_p)]
    lib.gc_seeder_destroy.argtypes = [C.c_void_p]
    lib.gc_seeder_array.argtypes = [C.c_void_p, C.c_char_p, _P(_P(C.c_int64)), _P(C.c_uint64)]
    lib.gc_stream_create.argtypes = [_P(C.c_void_p)]
    lib.gc_stream_destroy.argtypes = [C.c_void_p]
    lib.gc_reads_upload.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, _P(C.c_void_p)]
    lib.gc_reads_destroy.argtypes = [C.c_void_p]
    lib.gc_align_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _P(GcParams), _P(_P(GcResult))]
    lib.gc_seeds_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _P(C.c_void_p)]
    lib.gc_seeds_destroy.argtypes = [C.c_void_p]
    lib.gc_seeds_hits.argtypes = [C.c_void_p, _P(C.c_void_p), _P(C.c_void_p), _P(C.c_uint64)]
    lib.gc_seeds_kernel_ms.argtypes = [C.c_void_p]
    lib.gc_seeds_kernel_ms.restype = C.c_double
    lib.gc_mxm_index_create.argtypes = [C.c_void_p, _P(C.c_void_p)]
    lib.gc_mxm_options_default.argtypes = [_P(GcMxmOptions)]
    lib.gc_mxm_options_default.restype = None
    lib.gc_mxm_index_open.argtypes = [C.c_void_p, _P(GcMxmOptions), _P(C.c_void_p)]
    lib.gc_mxm_cache_check.argtypes = [C.c_char_p, _P(C.c_uint64)]
    lib.gc_mxm_index_destroy.argtypes = [C.c_void_p]
    lib.gc_mxm_index_array.argtypes = [C.c_void_p, C.c_char_p, _P(_P(C.c_int64)), _P(C.c_uint64)]
    lib.gc_seeds_mxm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_uint32, _P(C.c_void_p)]
    lib.gc_align_batch_seeded.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _P(GcParams), _P(_P(GcResult))]
    lib.gc_result_free.argtypes = [_P(GcResult)]
    lib.gc_params_default.argtypes = [_P(GcParams)]
    lib.gc_params_ext_default.argtypes = [_P(GcParamsExt)]
    lib.gc_params_ext_default.restype = None
    lib.gc_align_batch_ext.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _P(GcParams), _P(GcParamsExt), _P(_P(GcResult))]
    lib.gc_test_max_x_score.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_double, C.c_int32, C.c_void_p]
    lib.gc_free.argtypes = [C.c_void_p]
    lib.gc_set_device.argtypes = [C.c_int]
    lib.gc_index_build.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_double, C.c_char_p]
    lib.gc_index_save.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p]
    lib.gc_index_load.argtypes = [C.c_char_p, _P(C.c_void_p), _P(C.c_void_p)]
    lib.gc_index_check.argtypes = [C.c_char_p, _P(C.c_uint64)]
    _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        raise RuntimeError(f"graphchainer_amd error {rc}: {load_library().gc_last_error().decode()}")


def device_count():
    return load_library().gc_device_count()


def device_memory():
    """(free, total) bytes of the current device's memory."""
    lib = load_library()
    free, total = C.c_uint64(), C.c_uint64()
    lib.gc_device_memory.argtypes = [_P(C.c_uint64), _P(C.c_uint64)]
    _check(lib.gc_device_memory(C.byref(free), C.byref(total)))
    return int(free.value), int(total.value)


def set_device(index):
    _check(load_library().gc_set_device(index))


def edit_distance(a_list, b_list):
    """Global (NW) edit distance of each (a, b) pair of byte strings on the GPU (edlib NW distance, src/Aligner.cpp:645,845)."""
    assert len(a_list) == len(b_list)
    lib = load_library()
    n = len(a_list)
    a = b"".join(a_list)
    b = b"".join(b_list)
    a_off = np.zeros(n + 1, dtype=np.uint64)
    b_off = np.zeros(n + 1, dtype=np.uint64)
    a_off[1:] = np.cumsum([len(x) for x in a_list], dtype=np.uint64) if n else []
    b_off[1:] = np.cumsum([len(x) for x in b_list], dtype=np.uint64) if n else []
    out = np.zeros(max(n, 1), dtype=np.int64)
    lib.gc_edit_distance.restype = C.c_int
    lib.gc_edit_distance.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p]
    _check(lib.gc_edit_distance(a, a_off.ctypes.data, b, b_off.ctypes.data, n, out.ctypes.data))
    return out[:n]


def edit_path(a_list, b_list):
    """edlibAlign(a, b, NW, EDLIB_TASK_PATH) of each pair on the GPU (src/Aligner.cpp:845): returns (distances, [op arrays]);
    ops: 0 match, 1 letter of a alone, 2 letter of b alone, 3 mismatch."""
    assert len(a_list) == len(b_list)
    lib = load_library()
    n = len(a_list)
    a, b = b"".join(a_list), b"".join(b_list)
    a_off = np.zeros(n + 1, dtype=np.uint64)
    b_off = np.zeros(n + 1, dtype=np.uint64)
    a_off[1:] = np.cumsum([len(x) for x in a_list], dtype=np.uint64) if n else []
    b_off[1:] = np.cumsum([len(x) for x in b_list], dtype=np.uint64) if n else []
    ops_off = (a_off + b_off).astype(np.uint64)
    ops = np.zeros(max(int(ops_off[-1]), 1), dtype=np.uint8)
    ops_len = np.zeros(max(n, 1), dtype=np.uint32)
    dist = np.zeros(max(n, 1), dtype=np.int64)
    lib.gc_edit_path.restype = C.c_int
    lib.gc_edit_path.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _check(lib.gc_edit_path(a, a_off.ctypes.data, b, b_off.ctypes.data, n, ops_off.ctypes.data, ops.ctypes.data, ops_len.ctypes.data, dist.ctypes.data))
    return dist[:n], [ops[int(ops_off[i]):int(ops_off[i]) + int(ops_len[i])].copy() for i in range(n)]


GAM_DEVICE_HUFFMAN = 100   # GC_GAM_DEVICE_HUFFMAN: gam_level value that has the gzip members deflated on the device
GAM_DEVICE_LZ = 101        # GC_GAM_DEVICE_LZ (r6): ... with LZ77 matches in front of the Huffman stage


def max_x_scores(vp, vn, score_end, error_cost, cells=64):
    """Test entry: WordSlice::maxXScoreFirstSlices of DP columns as the extension kernel computes it (gc_test_max_x_score)."""
    lib = load_library()
    vp = np.ascontiguousarray(vp, dtype=np.uint64)
    vn = np.ascontiguousarray(vn, dtype=np.uint64)
    score_end = np.ascontiguousarray(score_end, dtype=np.int32)
    out = np.zeros(len(vp), dtype=np.int32)
    _check(lib.gc_test_max_x_score(vp.ctypes.data, vn.ctypes.data, score_end.ctypes.data, len(vp), float(error_cost), int(cells), out.ctypes.data))
    return out



def std_sort_permutations(arrays, depth_limit=-1):
    """Test entry: the permutations the device's wave-cooperative replay of libstdc++'s std::sort (csrc/hip/gc_stdsort_wave.hpp) gives for arrays of uint32 keys."""
    lib = load_library()
    arrays = [np.ascontiguousarray(a, dtype=np.uint32) for a in arrays]
    off = np.zeros(len(arrays) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(a) for a in arrays])
    keys = np.concatenate(arrays) if arrays else np.zeros(0, dtype=np.uint32)
    perm = np.zeros(len(keys), dtype=np.uint32)
    lib.gc_std_sort_permutations.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int64, C.c_void_p]
    _check(lib.gc_std_sort_permutations(keys.ctypes.data, off.ctypes.data, len(arrays), int(depth_limit), perm.ctypes.data))
    return [perm[int(off[i]):int(off[i + 1])] for i in range(len(arrays))]


def gzip_streams(streams, lz=False):
    """One gzip member per byte string, deflated on the GPU as one dynamic-Huffman block of literals (what gam_level=GAM_DEVICE_HUFFMAN does with a batch's GAM groups);
    lz: with LZ77 matches in front of the Huffman stage (GAM_DEVICE_LZ)."""
    lib = load_library()
    n = len(streams)
    raw = b"".join(streams)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in streams], dtype=np.uint64) if n else []
    out_off = np.zeros(n + 1, dtype=np.uint64)
    ptr = C.c_void_p()
    fn = lib.gc_gzip_streams_lz if lz else lib.gc_gzip_streams
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, _P(C.c_void_p), C.c_void_p]
    _check(fn(raw, off.ctypes.data, n, C.byref(ptr), out_off.ctypes.data))
    data = C.string_at(ptr.value, int(out_off[n]))
    lib.gc_free(ptr)
    return [data[int(out_off[i]):int(out_off[i + 1])] for i in range(n)]


BGZF_REFUSED = "could not be inflated"   # GC_BGZF_REFUSED (include/graphchainer_amd.h; tests/test_inflate_host.py holds the two together)


class BgzfError(zlib.error):
    """A BGZF block that the device inflater refuses: what zlib.error is for a gzip member that the host's zlib refuses."""


def _check_bgzf(rc):
    if rc != 0:
        text = load_library().gc_last_error().decode()
        if rc == -1 and BGZF_REFUSED in text:                  # GC_ERR_INVALID naming the block
            raise BgzfError(f"graphchainer_amd error {rc}: {text}")
        raise RuntimeError(f"graphchainer_amd error {rc}: {text}")


def bgzf_inflate(data):
    """The whole BGZF blocks at the front of data, inflated on the device (gc_bgzf_inflate): -> (text, consumed). consumed counts compressed bytes: a trailing partial
    block is left, a member that is not BGZF stops the walk, and 0 says that data does not start with a whole BGZF block. BgzfError names a block that does not inflate."""
    lib = load_library()
    data = bytes(data) if not isinstance(data, bytes) else data
    lib.gc_bgzf_inflate.restype = C.c_int
    lib.gc_bgzf_inflate.argtypes = [C.c_char_p, C.c_uint64, _P(C.c_void_p), _P(C.c_uint64), _P(C.c_uint64)]
    ptr, n, consumed = C.c_void_p(), C.c_uint64(), C.c_uint64()
    _check_bgzf(lib.gc_bgzf_inflate(data, len(data), C.byref(ptr), C.byref(n), C.byref(consumed)))
    try:
        return C.string_at(ptr.value, n.value), int(consumed.value)
    finally:
        lib.gc_free(ptr)


def evalue(min_identity, database_size, query_size, alignment_length, num_edits):
    """{alignment score, E-value} of the --E-cutoff model (host only)."""
    lib = load_library()
    out = np.zeros(2, dtype=np.float64)
    lib.gc_evalue.restype = C.c_int
    lib.gc_evalue.argtypes = [C.c_double, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    _check(lib.gc_evalue(min_identity, database_size, query_size, alignment_length, num_edits, out.ctypes.data))
    return out


def format_gaf_trace(graph, name, read, node, offset, seqpos, switch, merge=False):
    """GAF line (bytes, no newline) of one alignment given as a trace in output coordinates (gc_format_gaf_trace: GraphAlignerGAFAlignment::traceToAlignment; host only)."""
    lib = load_library()
    node = np.ascontiguousarray(node, dtype=np.int32)
    offset = np.ascontiguousarray(offset, dtype=np.uint32)
    seqpos = np.ascontiguousarray(seqpos, dtype=np.uint32)
    switch = np.ascontiguousarray(switch, dtype=np.uint8)
    assert len(node) == len(offset) == len(seqpos) == len(switch)
    read = read if isinstance(read, bytes) else read.encode()
    text, length = C.c_void_p(), C.c_uint64()
    lib.gc_format_gaf_trace.restype = C.c_int
    lib.gc_format_gaf_trace.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, _P(C.c_void_p), _P(C.c_uint64)]
    _check(lib.gc_format_gaf_trace(graph.handle, name if isinstance(name, bytes) else name.encode(), read, len(read), node.ctypes.data, offset.ctypes.data, seqpos.ctypes.data,
                                   switch.ctypes.data, len(node), int(bool(merge)), C.byref(text), C.byref(length)))
    line = C.string_at(text.value, int(length.value))
    lib.gc_free(text)
    return line


def graph_letters(graph, node, offset):
    """The graph letter under each (bigraph node id, offset in the original node) (gc_graph_letters: TraceItem's graphCharacter; host only) as bytes."""
    lib = load_library()
    node = np.ascontiguousarray(node, dtype=np.int32)
    offset = np.ascontiguousarray(offset, dtype=np.uint32)
    assert len(node) == len(offset)
    out = C.create_string_buffer(max(len(node), 1))
    lib.gc_graph_letters.restype = C.c_int
    lib.gc_graph_letters.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p]
    _check(lib.gc_graph_letters(graph.handle, node.ctypes.data, offset.ctypes.data, len(node), out))
    return out.raw[:len(node)]


def format_corrected_trace(graph, node, offset, switch):
    """The corrected piece (bytes) of one alignment given as a trace in output coordinates (gc_format_corrected_trace: GraphAligner's AddCorrected; host only)."""
    lib = load_library()
    node = np.ascontiguousarray(node, dtype=np.int32)
    offset = np.ascontiguousarray(offset, dtype=np.uint32)
    switch = np.ascontiguousarray(switch, dtype=np.uint8)
    assert len(node) == len(offset) == len(switch)
    text, length = C.c_void_p(), C.c_uint64()
    lib.gc_format_corrected_trace.restype = C.c_int
    lib.gc_format_corrected_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _P(C.c_void_p), _P(C.c_uint64)]
    _check(lib.gc_format_corrected_trace(graph.handle, node.ctypes.data, offset.ctypes.data, switch.ctypes.data, len(node), C.byref(text), C.byref(length)))
    piece = C.string_at(text.value, int(length.value))
    lib.gc_free(text)
    return piece


def corrected_pieces(graph, traces):
    """The corrected pieces of a list of traces, each (node, offset, switch), spelled by the device kernels (gc_corrected_pieces): a list of bytes, one per trace."""
    lib = load_library()
    n = len(traces)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(t[0]) for t in traces], dtype=np.uint64) if n else []
    cat = lambda k, dtype: np.ascontiguousarray(np.concatenate([np.asarray(t[k], dtype=dtype) for t in traces]) if n else np.zeros(0, dtype=dtype), dtype=dtype)   # noqa: E731
    node, offset, switch = cat(0, np.int32), cat(1, np.uint32), cat(2, np.uint8)
    assert len(node) == len(offset) == len(switch) == int(off[n])
    text, out_off = C.c_void_p(), C.c_void_p()
    lib.gc_corrected_pieces.restype = C.c_int
    lib.gc_corrected_pieces.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _P(C.c_void_p), _P(C.c_void_p)]
    _check(lib.gc_corrected_pieces(graph.handle, node.ctypes.data, offset.ctypes.data, switch.ctypes.data, off.ctypes.data, n, C.byref(text), C.byref(out_off)))
    try:
        at = np.ctypeslib.as_array(C.cast(out_off, _P(C.c_uint64)), shape=(n + 1,)).copy()
        data = C.string_at(text.value, int(at[n]))
    finally:
        lib.gc_free(text)
        lib.gc_free(out_off)
    return [data[int(at[i]):int(at[i + 1])] for i in range(n)]


def _join_pieces(pieces, line_offsets):
    """(bytes, line offsets) pieces as one text (and its line offsets)."""
    texts, offsets, at = [], [np.zeros(1, dtype=np.uint64)], 0
    for text, off in pieces:
        texts.append(text)
        offsets.append(off[1:] + np.uint64(at))
        at += len(text)
    data = b"".join(texts)
    return (data, np.concatenate(offsets)) if line_offsets else data


class Coverage:
    """How often every segment and every base of the graph lies under a final alignment (gc_coverage_*; include/graphchainer_amd.h has the meaning). The accumulators
    live on the current device, across batches: Aligner.align_batch(..., coverage=cov) or Aligner.set_coverage(cov) counts a batch's output alignments before the call
    returns, and several aligners may share one handle. per_base: also a 32-bit depth per forward base (4 bytes each on the device; RuntimeError when that does not fit).
    links: also how often every link of the graph is walked (16 bytes per link on the device; the header has the meaning of a link and its canonical form).
    pileup: also eight 32-bit channels per forward base - mismatches by read letter, deletions, insertions after and before (PILEUP_CHANNELS; the header has the rule);
    it implies per_base, 36 bytes per forward base in all.
    Integers added with atomics: the same reads give the same counts however they were batched."""

    def __init__(self, graph, per_base=False, links=False, pileup=False):
        self.lib = load_library()
        self.graph, self.per_base, self.links, self.pileup = graph, bool(per_base) or bool(pileup), bool(links), bool(pileup)          # (the graph must outlive the handle)
        self.handle = C.c_void_p()
        self.lib.gc_coverage_create2.restype = C.c_int
        self.lib.gc_coverage_create2.argtypes = [C.c_void_p, C.c_uint, _P(C.c_void_p)]
        _check(self.lib.gc_coverage_create2(graph.handle, (GC_COVERAGE_PER_BASE if self.per_base else 0) | (GC_COVERAGE_LINKS if self.links else 0) | (GC_COVERAGE_PILEUP if self.pileup else 0), C.byref(self.handle)))

    def add_traces(self, traces, seq_pos=None, reads=None):
        """Counts a list of traces, each (node, offset) in output coordinates, with the kernel the batches use (gc_coverage_add_traces); every cell is checked against the graph first.
        seq_pos / reads (both or neither; a handle with the pileup needs them): per trace the read position of every cell and the read's letters (bytes) - gc_coverage_add_traces2,
        which also checks every position against its read."""
        n = len(traces)
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(t[0]) for t in traces], dtype=np.uint64) if n else []
        cat = lambda rows, dtype: np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=dtype) for r in rows]) if n else np.zeros(0, dtype=dtype), dtype=dtype)   # noqa: E731
        node, offset = cat([t[0] for t in traces], np.int32), cat([t[1] for t in traces], np.uint32)
        assert len(node) == len(offset) == int(off[n])
        if seq_pos is None and reads is None:
            self.lib.gc_coverage_add_traces.restype = C.c_int
            self.lib.gc_coverage_add_traces.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
            _check(self.lib.gc_coverage_add_traces(self.handle, node.ctypes.data, offset.ctypes.data, off.ctypes.data, n))
            return
        if seq_pos is None or reads is None or len(seq_pos) != n or len(reads) != n:
            raise ValueError("add_traces: seq_pos and reads go together, one of each per trace")
        positions = cat(seq_pos, np.uint32)
        assert len(positions) == len(node)
        letters = b"".join(bytes(r) for r in reads)
        read_off = np.zeros(n + 1, dtype=np.uint64)
        read_off[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64) if n else []
        self.lib.gc_coverage_add_traces2.restype = C.c_int
        self.lib.gc_coverage_add_traces2.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_void_p]
        _check(self.lib.gc_coverage_add_traces2(self.handle, node.ctypes.data, offset.ctypes.data, positions.ctypes.data, off.ctypes.data, n, letters, read_off.ctypes.data))

    def counts(self):
        """-> (bases [segments] uint64, depth [forward bases] uint32 or None without per_base): the accumulators as they stand."""
        bases, depth, n_seg, n_bases = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
        self.lib.gc_coverage_counts.restype = C.c_int
        self.lib.gc_coverage_counts.argtypes = [C.c_void_p, _P(C.c_void_p), _P(C.c_uint64), _P(C.c_void_p), _P(C.c_uint64)]
        _check(self.lib.gc_coverage_counts(self.handle, C.byref(bases), C.byref(n_seg), C.byref(depth), C.byref(n_bases)))
        try:
            b = np.ctypeslib.as_array(C.cast(bases, _P(C.c_uint64)), shape=(int(n_seg.value),)).copy() if n_seg.value else np.zeros(0, dtype=np.uint64)
            d = None
            if depth:
                d = np.ctypeslib.as_array(C.cast(depth, _P(C.c_uint32)), shape=(int(n_bases.value),)).copy() if n_bases.value else np.zeros(0, dtype=np.uint32)
        finally:
            self.lib.gc_free(bases)
            self.lib.gc_free(depth)
        return b, d

    def merge(self, other):
        """self += other (gc_coverage_merge): handles of one device or of two, made for graphs of the same shape."""
        self.lib.gc_coverage_merge.restype = C.c_int
        self.lib.gc_coverage_merge.argtypes = [C.c_void_p, C.c_void_p]
        _check(self.lib.gc_coverage_merge(self.handle, other.handle))

    def _table(self, fn):
        text, length, line_off, n_lines = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, _P(C.c_void_p), _P(C.c_uint64), _P(C.c_void_p), _P(C.c_uint64)]
        _check(fn(self.handle, C.byref(text), C.byref(length), C.byref(line_off), C.byref(n_lines)))
        try:
            data = C.string_at(text.value, int(length.value))
            offsets = np.ctypeslib.as_array(C.cast(line_off, _P(C.c_uint64)), shape=(int(n_lines.value) + 1,)).copy()
        finally:
            self.lib.gc_free(text)
            self.lib.gc_free(line_off)
        return data, offsets

    def segment_table(self, line_offsets=False):
        """The --coverage-out table (bytes), spelled on the device: "#segment\tlength\tbases", then a line per segment. line_offsets: -> (bytes, byte offsets of the lines)."""
        data, offsets = self._table(self.lib.gc_coverage_format_segments)
        return (data, offsets) if line_offsets else data

    def base_table(self, line_offsets=False):
        """The --base-coverage-out table (bytes; needs per_base): "segment\tstart\tend\tdepth" per maximal run of equal non-zero depth inside a segment."""
        data, offsets = self._table(self.lib.gc_coverage_format_bases)
        return (data, offsets) if line_offsets else data

    def link_counts(self):
        """-> (from, to [links] int32, traversals [links] uint64): the graph's links in link order, canonical bigraph ids (2 * segment + strand), and how often each was walked."""
        src, dst, counts, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
        self.lib.gc_coverage_link_counts.restype = C.c_int
        self.lib.gc_coverage_link_counts.argtypes = [C.c_void_p, _P(C.c_void_p), _P(C.c_void_p), _P(C.c_void_p), _P(C.c_uint64)]
        _check(self.lib.gc_coverage_link_counts(self.handle, C.byref(src), C.byref(dst), C.byref(counts), C.byref(n)))
        try:
            take = lambda p, t, dtype: np.ctypeslib.as_array(C.cast(p, _P(t)), shape=(int(n.value),)).copy() if n.value else np.zeros(0, dtype=dtype)   # noqa: E731
            return take(src, C.c_int32, np.int32), take(dst, C.c_int32, np.int32), take(counts, C.c_uint64, np.uint64)
        finally:
            for p in (src, dst, counts):
                self.lib.gc_free(p)

    def _rows(self, fn, first, count, *flags):
        text, length, line_off, n_lines = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64] + [C.c_int] * len(flags) + [_P(C.c_void_p), _P(C.c_uint64), _P(C.c_void_p), _P(C.c_uint64)]
        _check(fn(self.handle, int(first), int(count), *[int(f) for f in flags], C.byref(text), C.byref(length), C.byref(line_off), C.byref(n_lines)))
        try:
            data = C.string_at(text.value, int(length.value))
            offsets = np.ctypeslib.as_array(C.cast(line_off, _P(C.c_uint64)), shape=(int(n_lines.value) + 1,)).copy()
        finally:
            self.lib.gc_free(text)
            self.lib.gc_free(line_off)
        return data, offsets

    def _n_links(self):
        if getattr(self, "_link_total", None) is None:
            self._link_total = len(self.link_counts()[0])
        return self._link_total

    def _segment_lengths(self):
        """Forward length of every segment, from the graph's split nodes (what the S ranges of gfa_pieces are chosen by)."""
        if getattr(self, "_lengths", None) is None:
            ids, lengths = self.graph.array("nodeIDs"), self.graph.array("nodeLength")
            per_id = np.bincount(ids, weights=lengths).astype(np.int64) if len(ids) else np.zeros(0, dtype=np.int64)
            per_id = np.concatenate([per_id, np.zeros(len(per_id) & 1, dtype=np.int64)])
            self._lengths = np.maximum(per_id[0::2], per_id[1::2])
        return self._lengths

    def link_pieces(self, piece_bytes=GFA_PIECE_BYTES):
        """The --link-coverage-out table (needs links) as a generator of (bytes, byte offsets of the lines): "#from\tfrom_orient\tto\tto_orient\ttraversals", then a
        line per link in link order, zero rows included; about piece_bytes of text per piece."""
        n, step = self._n_links(), max(1, int(piece_bytes) // 48)
        for first in range(0, max(n, 1), step):
            yield self._rows(self.lib.gc_coverage_format_links, first, step)

    def link_table(self, line_offsets=False, piece_bytes=GFA_PIECE_BYTES):
        """The --link-coverage-out table (bytes; needs links), spelled on the device. line_offsets: -> (bytes, byte offsets of the lines)."""
        return _join_pieces(self.link_pieces(piece_bytes), line_offsets)

    def gfa_pieces(self, supported_only=False, piece_bytes=GFA_PIECE_BYTES):
        """The graph as a GFA with coverage tags (--coverage-gfa-out; needs links), spelled on the device, as a generator of (bytes, byte offsets of the lines): the line
        "H\tVN:Z:1.0", the segments "S\tname\tLETTERS\tLN:i:length\tRC:i:bases" (RC / LN = mean depth) in ranges chosen from the segment lengths so that a piece stays near
        piece_bytes, then the links "L\tfrom\t+-\tto\t+-\t0M\tRC:i:traversals" in link order. supported_only (--supported-subgraph-out): only segments with
        bases > 0 and links with traversals > 0."""
        head = b"H\tVN:Z:1.0\n"
        yield head, np.array([0, len(head)], dtype=np.uint64)
        lengths = self._segment_lengths()
        ends = np.cumsum(lengths + 48)                              # a line is its letters and about 48 bytes of name and tags
        first = 0
        while first < len(lengths):
            before = int(ends[first - 1]) if first else 0
            last = max(first + 1, int(np.searchsorted(ends, before + int(piece_bytes), side="right")))
            yield self._rows(self.lib.gc_coverage_format_gfa_segments, first, last - first, supported_only)
            first = last
        n, step = self._n_links(), max(1, int(piece_bytes) // 48)
        for first in range(0, n, step):
            yield self._rows(self.lib.gc_coverage_format_gfa_links, first, step, supported_only)

    def pileup_counts(self):
        """-> rows [forward bases, 8] uint32 (needs pileup), columns PILEUP_CHANNELS, bases in the order of counts()'s depth."""
        rows, n_bases = C.c_void_p(), C.c_uint64()
        self.lib.gc_coverage_pileup_counts.restype = C.c_int
        self.lib.gc_coverage_pileup_counts.argtypes = [C.c_void_p, _P(C.c_void_p), _P(C.c_uint64)]
        _check(self.lib.gc_coverage_pileup_counts(self.handle, C.byref(rows), C.byref(n_bases)))
        try:
            n = int(n_bases.value)
            return np.ctypeslib.as_array(C.cast(rows, _P(C.c_uint32)), shape=(n, 8)).copy() if n else np.zeros((0, 8), dtype=np.uint32)
        finally:
            self.lib.gc_free(rows)

    def _pileup_rows(self, first, count, min_alt, min_fraction):
        text, length, line_off, n_lines = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
        fn = self.lib.gc_coverage_format_pileup
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_double, _P(C.c_void_p), _P(C.c_uint64), _P(C.c_void_p), _P(C.c_uint64)]
        _check(fn(self.handle, int(first), int(count), int(min_alt), float(min_fraction), C.byref(text), C.byref(length), C.byref(line_off), C.byref(n_lines)))
        try:
            data = C.string_at(text.value, int(length.value))
            offsets = np.ctypeslib.as_array(C.cast(line_off, _P(C.c_uint64)), shape=(int(n_lines.value) + 1,)).copy()
        finally:
            self.lib.gc_free(text)
            self.lib.gc_free(line_off)
        return data, offsets

    def pileup_table(self, first=0, count=None, min_alt=1, min_fraction=0.0, line_offsets=False):
        """The --pileup-out table (bytes; needs pileup) over forward bases [first, first + count) (count None: to the end), spelled on the device by one call:
        "#segment\tpos\tref\tdepth\tmatch\tmmA\tmmC\tmmG\tmmT\tmmN\tdel\tins_before\tins_after" (only with first == 0), then a line per base with depth > 0 whose largest
        channel is >= min_alt and >= min_fraction * depth. line_offsets: -> (bytes, byte offsets of the lines)."""
        data, offsets = self._pileup_rows(first, (1 << 31) - 2 if count is None else count, min_alt, min_fraction)
        return (data, offsets) if line_offsets else data

    def pileup_pieces(self, min_alt=1, min_fraction=0.0, piece_bases=PILEUP_PIECE_BASES):
        """The --pileup-out table as a generator of (bytes, byte offsets of the lines), piece_bases forward bases per piece: the text of a large graph is never whole."""
        n, step = int(np.sum(self._segment_lengths())), max(1, int(piece_bases))
        for first in range(0, max(n, 1), step):
            yield self._pileup_rows(first, step, min_alt, min_fraction)

    def close(self):
        if self.handle:
            self.lib.gc_coverage_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _fetch_array(fn, handle, name):
    lib = load_library()
    ptr = _P(C.c_int64)()
    n = C.c_uint64()
    _check(fn(handle, name.encode(), C.byref(ptr), C.byref(n)))
    out = np.ctypeslib.as_array(ptr, shape=(n.value,)).copy() if n.value else np.zeros(0, dtype=np.int64)
    lib.gc_free(ptr)
    return out


class GcGraphDesc(C.Structure):
    _fields_ = [("n_nodes", C.c_uint64), ("first_ambiguous", C.c_uint64), ("node_length", C.c_void_p), ("node_offset", C.c_void_p),
                ("node_ids", C.c_void_p), ("node_seq", C.c_void_p), ("ambiguous_seq", C.c_void_p), ("in_off", C.c_void_p), ("in_adj", C.c_void_p),
                ("out_off", C.c_void_p), ("out_adj", C.c_void_p), ("component_number", C.c_void_p), ("chain_number", C.c_void_p),
                ("chain_approx_pos", C.c_void_p), ("lookup_order", C.c_void_p), ("n_lookup", C.c_uint64)]


def build_index_cache(gfa_path, cache_path, minimizer_length=15, window_size=20, keep_least_frequent_fraction=1 - 0.001):
    """Builds graph + MPC index (+ minimizer index unless minimizer_length is 0) on the host and writes the cache file;
    needs no GPU (the reference's saveMPC, src/AlignmentGraph.h:96, is an empty stub)."""
    _check(load_library().gc_index_build(os.fsencode(gfa_path), minimizer_length, window_size, keep_least_frequent_fraction, os.fsencode(cache_path)))


def save_index_cache(graph, seeder, cache_path):
    _check(load_library().gc_index_save(graph.handle, seeder.handle if seeder is not None else None, os.fsencode(cache_path)))


def check_index_cache(cache_path):
    """Verifies a cache file on the host and returns what it holds; raises RuntimeError for a damaged or foreign file."""
    info = (C.c_uint64 * 8)()
    _check(load_library().gc_index_check(os.fsencode(cache_path), info))
    keys = ["version", "nodes", "bp", "has_seeder", "k", "w", "kmers", "positions"]
    return {k: int(v) for k, v in zip(keys, info)}


def load_index_cache(cache_path):
    """-> (AlignmentGraph, MinimizerSeeder or None) uploaded to the current device from a cache file."""
    lib = load_library()
    g, s = C.c_void_p(), C.c_void_p()
    _check(lib.gc_index_load(os.fsencode(cache_path), C.byref(g), C.byref(s)))
    graph = AlignmentGraph(None, _handle=g)
    seeder = MinimizerSeeder(graph, _handle=s) if s else None
    return graph, seeder


class AlignmentGraph:
    """Split-node DAG + MPC index resident in HBM (reference: AlignmentGraph, src/AlignmentGraph.h)."""

    def __init__(self, gfa_path, _handle=None):
        self.lib = load_library()
        self.handle = C.c_void_p()
        if _handle is not None:
            self.handle = _handle
            return
        _check(self.lib.gc_graph_create_from_gfa(os.fsencode(gfa_path), C.byref(self.handle)))

    @classmethod
    def from_arrays(cls, arrays, with_lookup_order=True):
        """gc_graph_create: a graph from the arrays a host that keeps its own AlignmentGraph would hand over (the names are
        those of gc_graph_array)."""
        lib = load_library()
        keep = {
            "node_length": np.ascontiguousarray(arrays["nodeLength"], dtype=np.uint8),
            "node_offset": np.ascontiguousarray(arrays["nodeOffset"], dtype=np.uint32),
            "node_ids": np.ascontiguousarray(arrays["nodeIDs"], dtype=np.int32),
            "node_seq": np.ascontiguousarray(arrays["nodeSeq"]).view(np.uint64) if len(arrays["nodeSeq"]) else np.zeros(1, dtype=np.uint64),
            "ambiguous_seq": np.ascontiguousarray(arrays["ambiguousSeq"]).view(np.uint64) if len(arrays["ambiguousSeq"]) else np.zeros(1, dtype=np.uint64),
            "in_off": np.ascontiguousarray(arrays["in_off"], dtype=np.uint64), "in_adj": np.ascontiguousarray(arrays["in_adj"], dtype=np.uint32),
            "out_off": np.ascontiguousarray(arrays["out_off"], dtype=np.uint64), "out_adj": np.ascontiguousarray(arrays["out_adj"], dtype=np.uint32),
            "component_number": np.ascontiguousarray(arrays["componentNumber"], dtype=np.uint32),
            "chain_number": np.ascontiguousarray(arrays["chainNumber"], dtype=np.uint32),
            "chain_approx_pos": np.ascontiguousarray(arrays["chainApproxPos"], dtype=np.uint64),
            "lookup_order": np.ascontiguousarray(arrays["lookupOrder"], dtype=np.int32),
        }
        desc = GcGraphDesc()
        desc.n_nodes = len(keep["node_length"])
        desc.first_ambiguous = int(arrays["firstAmbiguous"][0])
        for name, arr in keep.items():
            setattr(desc, name, arr.ctypes.data)
        desc.n_lookup = len(keep["lookup_order"])
        if not with_lookup_order:
            desc.lookup_order, desc.n_lookup = None, 0
        handle = C.c_void_p()
        lib.gc_graph_create.argtypes = [_P(GcGraphDesc), _P(C.c_void_p)]
        _check(lib.gc_graph_create(C.byref(desc), C.byref(handle)))
        return cls(None, _handle=handle)

    def NodeSize(self):
        return self.lib.gc_graph_num_nodes(self.handle)

    def SizeInBP(self):
        return self.lib.gc_graph_size_bp(self.handle)

    def array(self, name):
        return _fetch_array(self.lib.gc_graph_array, self.handle, name)

    def trim_host(self):
        """Release the host copy of the MPC index (gc_graph_trim_host): aligning does not read it, saving the index cache does."""
        _check(self.lib.gc_graph_trim_host(self.handle))

    def close(self):
        if self.handle:
            self.lib.gc_graph_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MinimizerSeeder:
    """reference: MinimizerSeeder(graph, k, w, threads, 1 - discardMostNumerousFraction), src/Aligner.cpp:1162"""

    def __init__(self, graph, minimizer_length=15, window_size=20, keep_least_frequent_fraction=1 - 0.001, _handle=None):
        self.lib = load_library()
        self.graph = graph
        self.handle = C.c_void_p()
        if _handle is not None:
            self.handle = _handle
            return
        _check(self.lib.gc_seeder_create(graph.handle, minimizer_length, window_size, keep_least_frequent_fraction, C.byref(self.handle)))

    def array(self, name):
        return _fetch_array(self.lib.gc_seeder_array, self.handle, name)

    def close(self):
        if self.handle:
            self.lib.gc_seeder_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ReadBatch:
    """A batch of reads resident in HBM."""

    def __init__(self, reads):
        self.lib = load_library()
        bs = [r.encode() if isinstance(r, str) else bytes(r) for r in reads]
        self.lengths = np.array([len(b) for b in bs], dtype=np.uint64)
        self.offsets = np.zeros(len(bs) + 1, dtype=np.uint64)
        self.offsets[1:] = np.cumsum(self.lengths)
        blob = b"".join(bs)
        self.blob = blob               # host copy: the output encoders read bases next to the device results
        self.handle = C.c_void_p()
        _check(self.lib.gc_reads_upload(blob, self.offsets.ctypes.data, len(bs), C.byref(self.handle)))

    @classmethod
    def from_text(cls, data, fmt, final=True):
        """FASTA / FASTQ text parsed on the device (gc_reads_parse): -> (batch, ids, consumed). fmt: "fasta" / "fastq" (or GC_FASTX_*). The batch is what ReadBatch(list of
        the reads) is - blob, offsets, lengths and the same device object - and ids are the header lines behind their first byte, as bytes. final=False: data is a chunk
        from the middle of a file; only records whose end it holds are returned and `consumed` is where the next chunk must begin (0: bring more)."""
        lib = load_library()
        code = FASTX_FORMATS.get(fmt, fmt)
        if not isinstance(code, int):
            raise ValueError("fmt is 'fasta' or 'fastq'")
        data = bytes(data) if not isinstance(data, bytes) else data
        lib.gc_reads_parse.argtypes = [C.c_char_p, C.c_uint64, C.c_int32, C.c_uint32, _P(C.c_void_p), _P(_P(GcFastxTable))]
        lib.gc_fastx_table_free.argtypes = [_P(GcFastxTable)]
        lib.gc_fastx_table_free.restype = None
        handle, table = C.c_void_p(), _P(GcFastxTable)()
        _check(lib.gc_reads_parse(data, len(data), code, FASTX_FINAL if final else 0, C.byref(handle), C.byref(table)))
        return cls._from_table(lib, handle, table)

    @classmethod
    def _from_table(cls, lib, handle, table):
        try:
            t = table.contents
            n = int(t.n_reads)
            self = cls.__new__(cls)
            self.lib, self.handle = lib, handle
            self.offsets = np.ctypeslib.as_array(t.offsets, shape=(n + 1,)).copy()
            self.lengths = np.diff(self.offsets)
            self.blob = C.string_at(t.bases, int(self.offsets[n]))
            name_off = np.ctypeslib.as_array(t.name_off, shape=(n + 1,))
            names = C.string_at(t.names, int(name_off[n]))
            ids = [names[int(name_off[i]):int(name_off[i + 1]) - 1] for i in range(n)]
            self.kernel_ms = float(t.kernel_ms)
            return self, ids, int(t.consumed)
        finally:
            lib.gc_fastx_table_free(table)

    @classmethod
    def from_bgzf(cls, head, data, fmt, final=True):
        """from_text on `head` followed by the inflated whole BGZF blocks at the front of `data` (gc_reads_parse_bgzf): -> (batch, ids, tail, consumed). The blocks are
        inflated on the device and their text is parsed where it lies; `tail` is the text behind the last complete record - the next call's head - and the only text that
        comes down, `consumed` counts compressed bytes as bgzf_inflate's does. batch.bgzf holds the blocks, their text, and the scan, upload and kernel milliseconds."""
        lib = load_library()
        code = FASTX_FORMATS.get(fmt, fmt)
        if not isinstance(code, int):
            raise ValueError("fmt is 'fasta' or 'fastq'")
        head = bytes(head) if not isinstance(head, bytes) else head
        data = bytes(data) if not isinstance(data, bytes) else data
        lib.gc_reads_parse_bgzf.restype = C.c_int
        lib.gc_reads_parse_bgzf.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_int32, C.c_uint32, _P(C.c_void_p), _P(_P(GcFastxTable)), _P(C.c_void_p), _P(C.c_uint64),
                                            _P(C.c_uint64), _P(GcBgzfStats)]
        lib.gc_fastx_table_free.argtypes = [_P(GcFastxTable)]
        lib.gc_fastx_table_free.restype = None
        handle, table, tail, tail_len, consumed, stats = C.c_void_p(), _P(GcFastxTable)(), C.c_void_p(), C.c_uint64(), C.c_uint64(), GcBgzfStats()
        _check_bgzf(lib.gc_reads_parse_bgzf(head, len(head), data, len(data), code, FASTX_FINAL if final else 0, C.byref(handle), C.byref(table), C.byref(tail), C.byref(tail_len),
                                            C.byref(consumed), C.byref(stats)))
        try:
            text = C.string_at(tail.value, tail_len.value)
        finally:
            lib.gc_free(tail)
        self, ids, _ = cls._from_table(lib, handle, table)
        self.bgzf = {"blocks": int(stats.blocks), "inflated_bytes": int(stats.inflated_bytes), "scan_ms": float(stats.scan_ms), "upload_ms": float(stats.upload_ms), "kernel_ms": float(stats.kernel_ms)}
        return self, ids, text, int(consumed.value)

    @classmethod
    def from_bam(cls, data, header, final=True):
        """Inflated unaligned BAM bytes decoded on the device (gc_reads_parse_bam): -> (batch, ids, consumed), as from_text gives them. header: data starts with the
        file's header (else at a record boundary). Records with flag 0x100 or 0x800 are left out; batch.bam holds the records seen, those skipped and the kernels'
        milliseconds. final=True refuses a header or record that the end of data cuts."""
        lib = load_library()
        data = bytes(data) if not isinstance(data, bytes) else data
        lib.gc_reads_parse_bam.restype = C.c_int
        lib.gc_reads_parse_bam.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, _P(C.c_void_p), _P(_P(GcFastxTable)), _P(GcBamStats)]
        lib.gc_fastx_table_free.argtypes = [_P(GcFastxTable)]
        lib.gc_fastx_table_free.restype = None
        handle, table, stats = C.c_void_p(), _P(GcFastxTable)(), GcBamStats()
        _check(lib.gc_reads_parse_bam(data, len(data), (FASTX_FINAL if final else 0) | (BAM_HEADER if header else 0), C.byref(handle), C.byref(table), C.byref(stats)))
        self, ids, consumed = cls._from_table(lib, handle, table)
        self.bam = stats.as_dict()
        return self, ids, consumed

    @classmethod
    def from_bam_bgzf(cls, head, data, header, final=True):
        """from_bam on `head` followed by the inflated whole BGZF blocks at the front of `data` (gc_reads_parse_bam_bgzf): -> (batch, ids, tail, consumed), as from_bgzf
        gives them: `tail` is the bytes behind the last whole record, the next call's head; `consumed` counts compressed bytes. batch.bgzf and batch.bam hold the counts."""
        lib = load_library()
        head = bytes(head) if not isinstance(head, bytes) else head
        data = bytes(data) if not isinstance(data, bytes) else data
        lib.gc_reads_parse_bam_bgzf.restype = C.c_int
        lib.gc_reads_parse_bam_bgzf.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_uint32, _P(C.c_void_p), _P(_P(GcFastxTable)), _P(C.c_void_p), _P(C.c_uint64),
                                                _P(C.c_uint64), _P(GcBgzfStats), _P(GcBamStats)]
        lib.gc_fastx_table_free.argtypes = [_P(GcFastxTable)]
        lib.gc_fastx_table_free.restype = None
        handle, table, tail, tail_len, consumed, stats, bam = C.c_void_p(), _P(GcFastxTable)(), C.c_void_p(), C.c_uint64(), C.c_uint64(), GcBgzfStats(), GcBamStats()
        _check_bgzf(lib.gc_reads_parse_bam_bgzf(head, len(head), data, len(data), (FASTX_FINAL if final else 0) | (BAM_HEADER if header else 0), C.byref(handle), C.byref(table),
                                                C.byref(tail), C.byref(tail_len), C.byref(consumed), C.byref(stats), C.byref(bam)))
        try:
            rest = C.string_at(tail.value, tail_len.value)
        finally:
            lib.gc_free(tail)
        self, ids, _ = cls._from_table(lib, handle, table)
        self.bgzf = {"blocks": int(stats.blocks), "inflated_bytes": int(stats.inflated_bytes), "scan_ms": float(stats.scan_ms), "upload_ms": float(stats.upload_ms), "kernel_ms": float(stats.kernel_ms)}
        self.bam = bam.as_dict()
        return self, ids, rest, int(consumed.value)

    def close(self):
        if self.handle:
            self.lib.gc_reads_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


FASTX_FASTA, FASTX_FASTQ, FASTX_FINAL = 1, 2, 1   # GC_FASTX_FASTA / GC_FASTX_FASTQ / GC_FASTX_FINAL
BAM_HEADER = 2                                    # GC_BAM_HEADER
FASTX_FORMATS = {"fasta": FASTX_FASTA, "fastq": FASTX_FASTQ}


class GcFastxTable(C.Structure):
    """gc_fastx_table (include/graphchainer_amd.h): what gc_reads_parse hands back in host memory."""
    _fields_ = [("n_reads", C.c_uint64), ("consumed", C.c_uint64), ("offsets", _P(C.c_uint64)), ("bases", _P(C.c_char)), ("name_off", _P(C.c_uint64)), ("names", _P(C.c_char)),
                ("kernel_ms", C.c_double)]


class GcBgzfStats(C.Structure):
    """gc_bgzf_stats (include/graphchainer_amd.h)."""
    _fields_ = [("blocks", C.c_uint64), ("inflated_bytes", C.c_uint64), ("scan_ms", C.c_double), ("upload_ms", C.c_double), ("kernel_ms", C.c_double)]


class GcBamStats(C.Structure):
    """gc_bam_stats (include/graphchainer_amd.h)."""
    _fields_ = [("records", C.c_uint64), ("skipped", C.c_uint64), ("walk_ms", C.c_double), ("fields_ms", C.c_double), ("names_ms", C.c_double), ("unpack_ms", C.c_double)]

    def as_dict(self):
        return {"records": int(self.records), "skipped": int(self.skipped), "walk_ms": float(self.walk_ms), "fields_ms": float(self.fields_ms), "names_ms": float(self.names_ms),
                "unpack_ms": float(self.unpack_ms)}


def fastx_file_format(path):
    """FastQ::streamFastqFromFile's choice by file name (src/fastqloader.h:98-139): ("fasta" | "fastq" | None, gzipped). None: the reference reads nothing from such a
    file and reports nothing. This build's own: a name that ends in .bam is ("bam", True) - unaligned BAM, which is BGZF throughout (a .bam.gz is not)."""
    name = os.fsdecode(path)
    if len(name) > 4 and name.endswith(".bam"):
        return "bam", True
    gz = len(name) > 3 and name.endswith(".gz")
    if gz:
        name = name[:-3]
    fastq = (len(name) > 6 and name.endswith(".fastq")) or (len(name) > 3 and name.endswith(".fq"))
    fasta = (len(name) > 6 and name.endswith(".fasta")) or (len(name) > 3 and name.endswith(".fa"))
    return ("fasta" if fasta else "fastq" if fastq else None), gz


class BgzfPiece(bytes):
    """A piece of file_pieces(bgzf="device"): whole BGZF blocks, still compressed; .text_bytes is what they inflate to."""
    text_bytes = 0


def bgzf_member(buf, at=0):
    """The gzip member at buf[at:] as include/graphchainer_amd.h defines a BGZF block (1f 8b 08, FLG exactly 4, a BC subfield with SLEN 2, ISIZE at most 64 KiB): (block size, ISIZE) of a
    whole block, 0 where it may be a block that the end of buf cuts, None where it is something else."""
    avail = len(buf) - at
    if buf[at:at + 4] != b"\x1f\x8b\x08\x04"[:max(0, min(4, avail))]:
        return None
    if avail < 12:
        return 0
    xlen = buf[at + 10] | buf[at + 11] << 8
    if avail < 12 + xlen:
        return 0
    sub, size = 0, None
    while sub + 4 <= xlen:
        f = at + 12 + sub
        slen = buf[f + 2] | buf[f + 3] << 8
        if sub + 4 + slen > xlen:
            return None
        if size is None and buf[f:f + 2] == b"BC" and slen == 2:
            size = (buf[f + 4] | buf[f + 5] << 8) + 1
        sub += 4 + slen
    if size is None or sub != xlen or size < 12 + xlen + 8:
        return None
    if avail < size:
        return 0
    isize = int.from_bytes(buf[at + size - 4:at + size], "little")
    return (size, isize) if isize <= 65536 else None               # more text than a BGZF block holds: an ordinary member, zlib's


def _bgzf_chunks(f, size):
    """The whole BGZF blocks at the front of the open file, compressed, in pieces of about `size` bytes of text (the ISIZE sum); returns the file's bytes already read
    behind them: empty at a clean end, else a member that is not a whole BGZF block, which is the host's from there on."""
    raw, start, at, text = b"", 0, 0, 0
    while True:
        got = bgzf_member(raw, at)
        if got == 0:
            more = f.read(max(size // 4, 1 << 16))
            if not more:
                break
            raw, at, start = raw[start:] + more, at - start, 0
            continue
        if got is None:
            break
        at += got[0]
        text += got[1]
        if text >= size:
            piece = BgzfPiece(raw[start:at])
            piece.text_bytes, start, text = text, at, 0
            yield piece
    if at > start:
        piece = BgzfPiece(raw[start:at])
        piece.text_bytes = text
        yield piece
    return raw[at:]


def _file_chunks(path, gz, size, bgzf="host"):
    """The file's bytes in pieces of about `size`; a .gz is inflated piece by piece, concatenated members included (as zstr does). bgzf="device": the BGZF blocks at the
    front of a .gz are given as they are (BgzfPiece), and zlib takes over at the first member that is not one."""
    with open(path, "rb") as f:
        if not gz:
            while True:
                piece = f.read(size)
                if not piece:
                    return
                yield piece
        raw = b""
        if bgzf == "device":
            raw = yield from _bgzf_chunks(f, size)
        inflate = zlib.decompressobj(47)   # gzip or zlib header, by itself
        started = False   # started: inside a member
        while True:
            if not raw:
                raw = f.read(max(size // 4, 1 << 16))
                if not raw:
                    if started:
                        raise EOFError(f"{os.fsdecode(path)}: the file ends inside a gzip member")
                    return
            started = True
            piece = inflate.decompress(raw, size)
            raw = inflate.unconsumed_tail
            if inflate.eof:               # the member ended: another may follow
                raw = inflate.unused_data
                inflate = zlib.decompressobj(47)
                started = False
            if piece:
                yield piece


def file_pieces(paths, batch_bytes=100 << 20, bgzf="host"):
    """The reader's half of read_files, free of the library (a host thread of its own may run it: read() and zlib release the GIL): generator of (fmt, piece, last) over
    the read files in order - about batch_bytes of file text, inflated, and whether the file ends with it. A file whose name gives no format gives nothing; an empty
    file gives one empty last piece. bgzf="device": a .gz whose first member is a BGZF block gives its whole blocks still compressed, as BgzfPiece, cut where their
    ISIZE sum reaches about batch_bytes - parse_pieces inflates them on the device; from a member that is not BGZF on (an ordinary gzip member appended to a BGZF file)
    the rest of the file is inflated here as under "host", the default, under which every .gz is. A .bam file ("bam") goes the .gz way under both settings: it is BGZF
    throughout, and its end-of-file block travels with the last piece."""
    if bgzf not in ("host", "device"):
        raise ValueError("bgzf is 'host' or 'device'")
    batch_bytes = max(int(batch_bytes), 1)
    for path in ([paths] if isinstance(paths, (str, bytes, os.PathLike)) else paths):
        fmt, gz = fastx_file_format(path)
        if fmt is None:
            continue
        pieces = _file_chunks(path, gz, batch_bytes, bgzf)
        piece = next(pieces, b"")
        while True:
            nxt = next(pieces, None)
            yield fmt, piece, nxt is None
            if nxt is None:
                break
            piece = nxt


def parse_pieces(pieces, before_parse=None, counts=None):
    """The parser's half of read_files: generator of (batch, ids) over what file_pieces gives. A record cut by the end of a piece is carried over to the next one, a
    record longer than the piece makes the chunk grow, and the chunk that ends a file is parsed as the end of a file. Sequential by its nature: the next chunk begins
    where gc_reads_parse says the previous one was consumed. before_parse() is called ahead of every gc_reads_parse (the command line selects the device there). A
    BgzfPiece goes through gc_reads_parse_bgzf with the carried text as its head; counts, a dict, gains the blocks inflated there under "bgzf_blocks". A "bam" piece goes
    through from_bam / from_bam_bgzf the same way; the file's header is expected at the start of a file - the first piece, or the one after a `last` - until a call has
    consumed it, and counts gains the records left out under "bam_skipped"."""
    held, at_start = b"", True
    for fmt, piece, last in pieces:
        if before_parse is not None:
            before_parse()
        if fmt == "bam":
            if isinstance(piece, BgzfPiece):
                batch, ids, tail, consumed = ReadBatch.from_bam_bgzf(held, piece, header=at_start, final=last)
                if consumed != len(piece):
                    raise RuntimeError("parse_pieces: a piece of whole BGZF blocks was not consumed whole")
                if counts is not None:
                    counts["bgzf_blocks"] = counts.get("bgzf_blocks", 0) + batch.bgzf["blocks"]
                moved = len(held) + batch.bgzf["inflated_bytes"] - len(tail)
                held = tail
            else:
                held += piece
                batch, ids, moved = ReadBatch.from_bam(held, header=at_start, final=last)
                held = held[moved:]
            if counts is not None:
                counts["bam_skipped"] = counts.get("bam_skipped", 0) + batch.bam["skipped"]
            at_start = last or (at_start and not moved)
            if last:
                held = b""
        elif isinstance(piece, BgzfPiece):
            batch, ids, tail, consumed = ReadBatch.from_bgzf(held, piece, fmt, final=last)
            if consumed != len(piece):
                raise RuntimeError("parse_pieces: a piece of whole BGZF blocks was not consumed whole")
            if counts is not None:
                counts["bgzf_blocks"] = counts.get("bgzf_blocks", 0) + batch.bgzf["blocks"]
            held = b"" if last else tail
        else:
            held += piece
            batch, ids, consumed = ReadBatch.from_text(held, fmt, final=last)
            held = b"" if last else held[consumed:]
        if ids:
            yield batch, ids
        else:
            batch.close()                  # no complete record yet: the chunk grows


def read_files(paths, batch_bytes=100 << 20, bgzf="host"):
    """Generator of (batch, ids) over read files, the reference's way (src/Aligner.cpp:167-187): the format by the file name (fastx_file_format; a file of another name
    gives nothing), .gz inflated on the host with zlib, about batch_bytes of file text per batch. A record cut by the end of a chunk is carried over to the next one, a
    record longer than the chunk makes the chunk grow; files are never joined - the end of each file is parsed as the end of a file. (file_pieces and parse_pieces are
    its two halves.)"""
    return parse_pieces(file_pieces(paths, batch_bytes, bgzf))


# gc_seed_hit (include/graphchainer_amd.h): SeedHit as a seeder hands it over, src/GraphAlignerWrapper.h:14
SEED_HIT_DTYPE = np.dtype([("node_id", np.int32), ("node_offset", np.uint32), ("seq_pos", np.uint32), ("match_len", np.uint32), ("raw_goodness", np.uint32), ("reverse", np.uint32)])


class SeedBatch:
    """A read batch's seed hits from the caller's own seeder (a seeds file, MEM matches, filtered minimizer hits), resolved and resident in HBM (gc_seeds_upload).
    hits_per_read: per read of `batch`, in the order its seeder returned them, a structured array of SEED_HIT_DTYPE or a list of
    (node_id, node_offset, seq_pos, match_len, raw_goodness, reverse) tuples. Read-only afterwards; may be shared by aligners, like the ReadBatch it belongs to."""

    def __init__(self, graph, batch, hits_per_read):
        self.lib = load_library()
        self.handle = C.c_void_p()
        per_read = []
        for hits in hits_per_read:
            if isinstance(hits, np.ndarray) and hits.dtype.names:
                per_read.append(np.ascontiguousarray(hits.astype(SEED_HIT_DTYPE, copy=False)))
            else:
                per_read.append(np.array([tuple(int(x) for x in h) for h in hits], dtype=SEED_HIT_DTYPE))
        self.offsets = np.zeros(len(per_read) + 1, dtype=np.uint64)
        self.offsets[1:] = np.cumsum([len(h) for h in per_read], dtype=np.uint64) if per_read else []
        flat = np.concatenate(per_read) if per_read else np.zeros(0, dtype=SEED_HIT_DTYPE)
        _check(self.lib.gc_seeds_upload(graph.handle, batch.handle, flat.ctypes.data if len(flat) else None, self.offsets.ctypes.data, len(per_read), C.byref(self.handle)))

    @classmethod
    def _adopt(cls, handle):
        """A SeedBatch around a gc_seeds the library made itself (MxmIndex.seeds)."""
        self = cls.__new__(cls)
        self.lib = load_library()
        self.handle = handle
        return self

    def hits(self):
        """The raw records as they lie in HBM (gc_seeds_hits): per read a SEED_HIT_DTYPE array - what was uploaded, or what the device seeder found, in its defined order."""
        ptr, off, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        _check(self.lib.gc_seeds_hits(self.handle, C.byref(ptr), C.byref(off), C.byref(n)))
        try:
            offsets = np.ctypeslib.as_array(C.cast(off, _P(C.c_uint64)), shape=(n.value + 1,)).copy()
            total = int(offsets[-1])
            flat = np.frombuffer(C.string_at(ptr.value, total * SEED_HIT_DTYPE.itemsize), dtype=SEED_HIT_DTYPE).copy() if total else np.zeros(0, dtype=SEED_HIT_DTYPE)
        finally:
            self.lib.gc_free(ptr)
            self.lib.gc_free(off)
        return [flat[int(offsets[r]):int(offsets[r + 1])] for r in range(n.value)]

    @property
    def kernel_ms(self):
        """Device milliseconds of the seeder that made these hits (0 for uploaded ones)."""
        return float(self.lib.gc_seeds_kernel_ms(self.handle))

    def close(self):
        if self.handle:
            self.lib.gc_seeds_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GcSeedStoreStats(C.Structure):
    """gc_seed_store_stats (include/graphchainer_amd.h)."""
    _fields_ = [("messages", C.c_uint64), ("seeds", C.c_uint64), ("distinct_hashes", C.c_uint64), ("hbm_bytes", C.c_uint64), ("host_ms", C.c_double), ("device_ms", C.c_double),
                ("inflate_ms", C.c_double), ("frame_ms", C.c_double), ("upload_ms", C.c_double), ("decode_ms", C.c_double), ("sort_ms", C.c_double)]


class SeedStore:
    """The seeds of the reference's -s / --seeds-file files, decoded on the device and resident in HBM (gc_seed_store_open): SeedStore(paths) reads GAM files (gzip or zlib, in
    the order given), SeedStore(streams=[bytes, ...]) takes streams that are inflated already. seeds(graph, batch, ids) joins a read batch's names - the ids ReadBatch.from_text
    or read_files returned - to their seeds on the device: a SeedBatch for Aligner.align_batch(batch, seeds=...). Read-only; may be shared by aligners."""

    def __init__(self, paths=None, streams=None):
        if (paths is None) == (streams is None):
            raise ValueError("give paths or streams")
        self.lib = lib = load_library()
        lib.gc_seed_store_open.argtypes = [_P(C.c_char_p), C.c_uint32, _P(C.c_void_p)]
        lib.gc_seed_store_from_memory.argtypes = [_P(C.c_void_p), C.c_void_p, C.c_uint32, _P(C.c_void_p)]
        lib.gc_seed_store_info.argtypes = [C.c_void_p, _P(GcSeedStoreStats)]
        lib.gc_seed_store_destroy.argtypes = [C.c_void_p]
        lib.gc_seed_store_destroy.restype = None
        lib.gc_seeds_from_store.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64, _P(C.c_void_p)]
        self.handle = C.c_void_p()
        if paths is not None:
            paths = [paths] if isinstance(paths, (str, bytes, os.PathLike)) else list(paths)
            array = (C.c_char_p * max(len(paths), 1))(*[os.fsencode(p) for p in paths])
            _check(lib.gc_seed_store_open(array, len(paths), C.byref(self.handle)))
        else:
            streams = [bytes(s) for s in streams]
            buffers = [C.create_string_buffer(s, max(len(s), 1)) for s in streams]
            array = (C.c_void_p * max(len(streams), 1))(*[C.cast(b, C.c_void_p) for b in buffers])
            lens = np.array([len(s) for s in streams] + [0], dtype=np.uint64)
            _check(lib.gc_seed_store_from_memory(array, lens.ctypes.data, len(streams), C.byref(self.handle)))

    def seeds(self, graph, batch, ids):
        names = b"".join((i if isinstance(i, bytes) else i.encode()) + b"\0" for i in ids)
        name_off = np.zeros(len(ids) + 1, dtype=np.uint64)
        name_off[1:] = np.cumsum([len(i if isinstance(i, bytes) else i.encode()) + 1 for i in ids], dtype=np.uint64) if len(ids) else []
        handle = C.c_void_p()
        _check(self.lib.gc_seeds_from_store(graph.handle, self.handle, batch.handle, names, name_off.ctypes.data, len(ids), C.byref(handle)))
        return SeedBatch._adopt(handle)

    def info(self):
        stats = GcSeedStoreStats()
        _check(self.lib.gc_seed_store_info(self.handle, C.byref(stats)))
        return {name: getattr(stats, name) for name, _ in GcSeedStoreStats._fields_}

    def close(self):
        if self.handle:
            self.lib.gc_seed_store_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


MXM_MUM, MXM_MEM = 1, 2   # GC_MXM_MUM / GC_MXM_MEM
MXM_BUILDS = {"host": 0, "device": 1}   # GC_MXM_BUILD_HOST / GC_MXM_BUILD_DEVICE


class GcMxmOptions(C.Structure):
    _fields_ = [("build", C.c_int32), ("reserved", C.c_int32), ("cache_prefix", C.c_char_p)]


def mxm_cache_check(prefix):
    """Verifies <prefix>.gcmxm on the host (gc_mxm_cache_check; no GPU needed): dict of version, text_letters, segments, file_bytes, text_fingerprint. A file that is missing,
    damaged, truncated or of another version raises."""
    info = (C.c_uint64 * 5)()
    _check(load_library().gc_mxm_cache_check(os.fsencode(prefix), info))
    return dict(zip(("version", "text_letters", "segments", "file_bytes", "text_fingerprint"), (int(x) for x in info)))


class MxmIndex:
    """The MUM / MEM seeder's index of a graph's forward segments, resident in HBM (gc_mxm_index_open): suffix array, packed text, segment table, prefix table.
    build: "host" (default) or "device" - who builds the suffix array, the same array either way. cache_prefix: the reference's --seeds-mxm-cache-prefix - <prefix>.gcmxm is
    loaded if it exists, else the index is built and saved there. With neither argument this is gc_mxm_index_create.
    seeds() is the reference's --seeds-mum-count / --seeds-mem-count N with --seeds-mxm-length L: index.seeds(batch, "mum" | "mem", count=N (None or -1: all), min_len=L)."""

    def __init__(self, graph, build="host", cache_prefix=None):
        self.lib = load_library()
        self.graph = graph           # the index belongs to the graph: keep it alive
        self.handle = C.c_void_p()
        options = GcMxmOptions()
        self.lib.gc_mxm_options_default(C.byref(options))
        mode = MXM_BUILDS.get(build, build)
        if not isinstance(mode, int):
            raise ValueError("build is 'host' or 'device'")
        options.build = mode
        options.cache_prefix = os.fsencode(cache_prefix) if cache_prefix else None
        _check(self.lib.gc_mxm_index_open(graph.handle, C.byref(options), C.byref(self.handle)))

    def array(self, name):
        """'sa', 'node_start', 'node_id', 'bytes', 'build_us', 'prefix_len', 'build_mode' (0 host, 1 device, 2 loaded from the cache), 'build_rounds', 'build_scratch_bytes',
        'cache_save_us', 'sa_us' (gc_mxm_index_array)."""
        return _fetch_array(self.lib.gc_mxm_index_array, self.handle, name)

    def seeds(self, batch, mode="mem", count=None, min_len=20, graph=None):
        """The batch's MUM / MEM seeds, found and resolved on the device: a SeedBatch for Aligner.align_batch(batch, seeds=...). graph: the graph to resolve against, the index's own
        unless given (another one is refused)."""
        modes = {"mum": MXM_MUM, "mem": MXM_MEM}
        mode = modes.get(mode, mode)
        if not isinstance(mode, int):
            raise ValueError("mode is 'mum' or 'mem'")
        max_count = 0xFFFFFFFFFFFFFFFF if count is None or count == -1 else int(count)
        if max_count < 0 or min_len < 0:
            raise ValueError("count and min_len cannot be negative")
        handle = C.c_void_p()
        _check(self.lib.gc_seeds_mxm((graph or self.graph).handle, self.handle, batch.handle, mode, max_count, int(min_len), C.byref(handle)))
        return SeedBatch._adopt(handle)

    def close(self):
        if self.handle:
            self.lib.gc_mxm_index_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_RESULT_FIELDS = {
    # name: (count expression)
    "read_seed_off": "n+1", "seed_node": "seeds", "seed_offset": "seeds", "seed_seqpos": "seeds", "seed_goodness": "seeds",
    "read_anchor_off": "n+1", "anchor_x": "anchors", "anchor_y": "anchors", "anchor_path_off": "anchors+1", "anchor_path": "paths",
    "anchor_first_node": "anchors", "anchor_first_offset": "anchors", "anchor_first_seqpos": "anchors",
    "anchor_last_node": "anchors", "anchor_last_offset": "anchors", "anchor_last_seqpos": "anchors", "anchor_score": "anchors",
    "read_chain_off": "n+1", "chain": "chains", "chain_score": "n",
    "failed_assertion": "n", "capacity_exceeded": "n", "seeds_extended": "n", "seeds_extended_long": "n", "flatten_ties": "n", "flatten_ties_long": "n",
    "read_longall_off": "n+1", "longall_start": "longs", "longall_end": "longs", "longall_score": "longs",
}


class _ResultHolder:
    """Owns one gc_result; frees it when the last reference goes away."""

    def __init__(self, lib, res):
        self.lib, self.res = lib, res

    def __del__(self):
        try:
            if self.res:
                self.lib.gc_result_free(self.res)
                self.res = None
        except Exception:
            pass


class _ResultArray(np.ndarray):
    """ndarray view of C memory that keeps the owning gc_result alive: every array (and every slice or view made from one, through
    numpy's .base chain) references the holder, so `x = aligner.align_batch(b)["chain"]` stays valid after the dict is gone."""
    _holder = None


class BatchResult(dict):
    """dict of numpy arrays that are VIEWS of the C result (no copies on the hot path). Each array keeps the C result alive
    (see _ResultArray); the memory is freed when the last of them goes away."""
    _holder = None


class Aligner:
    """Batched stand-in for the reference's per-read hot path (src/Aligner.cpp:601-922)."""

    def __init__(self, graph, seeder=None, bandwidth=10, split_len=35, split_gap=35, colinear_gap=10000, seed_density=10.0, keep_traces=False, keep_seeds=False, long_pass=False, stitch=True, edit_distances=True, chain_traces=None, e_cutoff=-1.0, capacities=None, device_output=0, ramp_bandwidth=0, max_cells_per_slice=-1, force_global=False, seed_extend_density=-1.0, extra_heuristic=False, colinear_chaining=True, selection_method=0, fast_mode=False, precise_clipping=0.0, x_drop=0):
        """capacities: {field of gc_capacities: value} for the device-side tables (default: all automatic).
        seeder: the MinimizerSeeder, or None for a caller that brings its own seeds to every batch (align_batch(batch, seeds=SeedBatch(...))).
        device_output: gc_params::device_output - 1 / 2: the final alignments' GAF path and CIGAR text (= / X or M items), + 4: their vg::Path bytes, written
        by the device from the traces it holds; align_batch(gaf_names=...) then needs no keep_traces. + 8 (also alone): the corrected reads' pieces (GraphAligner's
        --corrected-out / --corrected-clipped-out) for formats "corrected" / "corrected_clipped".
        ramp_bandwidth / max_cells_per_slice: the reference's -B / -C (gc_params; 0 and -1: off).
        force_global: the reference's --global-alignment (gc_params::force_global): every extension of both passes keeps all its slices, so an alignment
        reaches the read's end however poor its score. An int other than 0 / 1 is passed on as it is (and refused by the library).
        seed_extend_density / extra_heuristic: the reference's --seeds-extend-density / --extra-heuristic for the whole-read pass (gc_params; -1: all seeds).
        A density other than -1 needs colinear_chaining=False.
        colinear_chaining=False: --no-colinear-chaining, plain GraphAligner - seeding and the whole-read pass alone (needs long_pass=True); the anchor, chain, path
        and chain-trace arrays come back empty, both edit distances -1, and long_index holds SelectAlignments(selection_method: one of SELECT_*).
        fast_mode: the reference's --fast-mode (gc_params::fast_mode): the chained alignment is the stitched path itself, cell j at read position min(y, x + j), and
        chain_edit_distance counts its differing letters instead of an NW distance; no effect without chaining. An int other than 0 / 1 is refused by the library.
        precise_clipping / x_drop: the reference's --precise-clipping / --X-drop (gc_params_ext; 0: off): alignments and anchors end at the cell with the best X score
        for the identity cut-off instead of at the correctness trim, flatten_ties* are 0; an X-drop without a cut-off runs with 0.66. Values out of range are refused
        by the library."""
        self.lib = load_library()
        self.graph = graph
        self.seeder = seeder
        self.params = GcParams()
        self.lib.gc_params_default(C.byref(self.params))
        self.params.bandwidth = bandwidth
        self.params.split_len = split_len
        self.params.split_gap = split_gap
        self.params.colinear_gap = colinear_gap
        self.params.seed_density = seed_density
        self.params.keep_traces = int(keep_traces)
        self.params.keep_seeds = int(keep_seeds)
        self.params.long_pass = int(long_pass)
        self.params.stitch = int(stitch)
        self.params.edit_distances = int(edit_distances)
        # the chained alignment's trace costs a k_edit_path run, the op strings coming down and ~13 B per trace cell of result memory; without
        # the whole-read pass EVERY read with a stitched path "wins" (src/Aligner.cpp:905: nothing to beat), so a caller that only wants anchors
        # and chains (long_pass=False) gets none unless it asks (chain_traces=1: winners, 2: every read)
        self.params.chain_traces = int(chain_traces) if chain_traces is not None else (1 if long_pass else 0)
        self.params.e_cutoff = float(e_cutoff)
        self.params.device_output = int(device_output)
        self.params.ramp_bandwidth = int(ramp_bandwidth)
        self.params.max_cells_per_slice = int(max_cells_per_slice)
        self.params.force_global = int(force_global)
        self.params.seed_extend_density = float(seed_extend_density)
        self.params.extra_heuristic = int(extra_heuristic)
        self.params.colinear_chaining = int(colinear_chaining)
        self.params.selection_method = int(selection_method)
        self.params.fast_mode = int(fast_mode)
        self.params_ext = GcParamsExt()
        self.lib.gc_params_ext_default(C.byref(self.params_ext))
        self.params_ext.precise_clipping = float(precise_clipping)
        self.params_ext.x_drop = int(x_drop)
        for name, value in (capacities or {}).items():
            if name not in dict(GcCapacities._fields_) or name == "reserved":
                raise ValueError("no such capacity: " + name)
            setattr(self.params.capacity, name, int(value))
        self.stream = C.c_void_p()
        _check(self.lib.gc_stream_create(C.byref(self.stream)))
        self.coverage = None

    def set_coverage(self, coverage):
        """From now on every batch of this aligner (device_output != 0) is counted into `coverage` (a Coverage of this device; None: off) before align_batch returns."""
        self.lib.gc_stream_set_coverage.restype = C.c_int
        self.lib.gc_stream_set_coverage.argtypes = [C.c_void_p, C.c_void_p]
        _check(self.lib.gc_stream_set_coverage(self.stream, coverage.handle if coverage is not None else None))
        self.coverage = coverage

    def align_batch(self, batch, seeds=None, gaf_names=None, cigar_match_mismatch_merge=False, other_formats=False, formats=None, gam_level=None, coverage=None):
        """Runs the hot path for a ReadBatch; returns a dict of arrays. seeds: a SeedBatch made for this batch - its hits replace the seeder's. With gaf_names (one id per read; needs long_pass and
        keep_traces or device_output) the dict also holds "gaf" (bytes: the reference's GAF lines) and "gaf_chained_skipped"; with other_formats also "json" (JSON
        lines) and "gam" (gzip members of framed vg::Alignment messages; gam_level: their zlib level, or GAM_DEVICE_HUFFMAN for the device's deflate). formats may also name
        "corrected" / "corrected_clipped" (gc_format_corrected: FASTA records of the corrected reads / of every alignment's piece; device_output & 8 or keep_traces):
        the dict then holds their bytes and, under "corrected_rec_off" / "corrected_clipped_rec_off", the records' byte offsets (one more entry than records).
        coverage: a Coverage this one batch is counted into (needs device_output; set_coverage's handle, if any, is back in place afterwards)."""
        if coverage is not None:
            if not self.params.device_output:
                raise ValueError("coverage counts the batch's output alignments: the Aligner needs device_output != 0")
            standing = self.coverage
            self.set_coverage(coverage)
            try:
                return self.align_batch(batch, seeds=seeds, gaf_names=gaf_names, cigar_match_mismatch_merge=cigar_match_mismatch_merge, other_formats=other_formats, formats=formats, gam_level=gam_level)
            finally:
                self.set_coverage(standing)
        res = _P(GcResult)()
        ext_on = self.params_ext.precise_clipping != 0 or self.params_ext.x_drop != 0   # (with both off: the calls that take no block)
        if ext_on and (seeds is not None or self.seeder is not None):
            _check(self.lib.gc_align_batch_ext(self.graph.handle, None if seeds is not None else self.seeder.handle, self.stream, batch.handle, seeds.handle if seeds is not None else None,
                                               C.byref(self.params), C.byref(self.params_ext), C.byref(res)))
        elif seeds is not None:   # the caller's own hits in place of the minimizer seeder (gc_align_batch_seeded; seed_density does not apply)
            _check(self.lib.gc_align_batch_seeded(self.graph.handle, self.stream, batch.handle, seeds.handle, C.byref(self.params), C.byref(res)))
        elif self.seeder is None:
            raise ValueError("this Aligner has no seeder: pass seeds=SeedBatch(graph, batch, hits_per_read)")
        else:
            _check(self.lib.gc_align_batch(self.graph.handle, self.seeder.handle, self.stream, batch.handle, C.byref(self.params), C.byref(res)))
        holder = _ResultHolder(self.lib, res)
        if True:
            gaf = None
            if gaf_names is not None:
                # formats: which of "gaf", "json", "gam" to produce (default: GAF, all three with other_formats)
                want = tuple(formats) if formats is not None else (("gaf", "json", "gam") if other_formats else ("gaf",))
                gaf = self._format(res, batch, gaf_names, want, cigar_match_mismatch_merge, gam_level)
            r = res.contents
            n = int(r.n_reads)

            def arr(ptr, count):
                if not count:
                    return np.zeros(0, dtype=np.int64)
                a = np.ctypeslib.as_array(ptr, shape=(count,)).view(_ResultArray)
                a._holder = holder
                return a

            out = BatchResult()
            out._holder = holder
            out["read_seed_off"] = arr(r.read_seed_off, n + 1)
            seeds = int(out["read_seed_off"][-1])
            out["read_anchor_off"] = arr(r.read_anchor_off, n + 1)
            anchors = int(out["read_anchor_off"][-1])
            out["anchor_path_off"] = arr(r.anchor_path_off, anchors + 1)
            paths = int(out["anchor_path_off"][-1])
            out["read_chain_off"] = arr(r.read_chain_off, n + 1)
            chains = int(out["read_chain_off"][-1])
            out["read_longall_off"] = arr(r.read_longall_off, n + 1)
            longs = int(out["read_longall_off"][-1])
            out["read_path_off"] = arr(r.read_path_off, n + 1)
            cells_path = int(out["read_path_off"][-1])
            out["path_node"] = arr(r.path_node, cells_path)
            out["path_first_offset"] = arr(r.path_first_offset, n)
            out["path_last_offset"] = arr(r.path_last_offset, n)
            out["path_cells"] = arr(r.path_cells, n)
            out["read_long_off"] = arr(r.read_long_off, n + 1)
            out["long_index"] = arr(r.long_index, int(out["read_long_off"][-1]))
            out["long_edit_distance"] = arr(r.long_edit_distance, n)
            out["chain_edit_distance"] = arr(r.chain_edit_distance, n)
            out["chained_better"] = arr(r.chained_better, n)
            out["read_chain_trace_off"] = arr(r.read_chain_trace_off, n + 1)
            ctrace = int(out["read_chain_trace_off"][-1])
            for name in ("chain_trace_node", "chain_trace_offset", "chain_trace_seqpos", "chain_trace_switch"):
                out[name] = arr(getattr(r, name), ctrace)
            out["chain_aln_start"] = arr(r.chain_aln_start, n)
            out["chain_aln_end"] = arr(r.chain_aln_end, n)
            counts = {"n": n, "n+1": n + 1, "seeds": seeds, "anchors": anchors, "paths": paths, "chains": chains, "longs": longs}
            for name, expr in _RESULT_FIELDS.items():
                if name in out:
                    continue
                out[name] = arr(getattr(r, name), counts[expr])
            if self.params.keep_traces:
                out["long_trace_off"] = arr(r.long_trace_off, longs + 1)
                lcells = int(out["long_trace_off"][-1]) if longs else 0
                for name in ("long_trace_node", "long_trace_offset", "long_trace_seqpos", "long_trace_switch"):
                    out[name] = arr(getattr(r, name), lcells)
            if self.params.keep_traces == 1:   # (2: the alignments' traces only)
                out["anchor_trace_off"] = arr(r.anchor_trace_off, anchors + 1)
                cells = int(out["anchor_trace_off"][-1])
                for name in ("anchor_trace_node", "anchor_trace_offset", "anchor_trace_seqpos", "anchor_trace_switch"):
                    out[name] = arr(getattr(r, name), cells)
            if self.params.device_output:
                out["read_out_off"] = arr(r.read_out_off, n + 1)
                n_out = int(out["read_out_off"][-1])
                out["out_source"] = arr(r.out_source, n_out)
                out["out_numbers"] = arr(r.out_numbers, 12 * n_out)
                for name in ("out_path_off", "out_cigar_off", "out_vg_off"):
                    out[name] = arr(getattr(r, name), n_out + 1)
                if self.params.device_output & 8:
                    out["out_corrected_off"] = arr(r.out_corrected_off, n_out + 1)
            out["counters"] = np.array(list(r.counters), dtype=np.uint64)
            out["counters_long"] = np.array(list(r.counters_long), dtype=np.uint64)
            out["kernel_us"] = np.array(list(r.kernel_us))
            out["host_us"] = np.array(list(r.host_us))
            if gaf is not None:
                out.update(gaf[0])
                out["gaf_chained_skipped"] = gaf[1]
            return out   # arrays keep the C ABI's dtypes (uint32/uint64/...) and are views: no copies on the hot path

    def _format(self, res, batch, names, formats, cigar_match_mismatch_merge=False, gam_level=None):
        if not isinstance(names, C.Array):
            names = (C.c_char_p * len(names))(*[n.encode() if isinstance(n, str) else bytes(n) for n in names])

        def encode(fn, *extra):
            text, length, skipped = C.c_void_p(), C.c_uint64(), C.c_uint64()
            fn.restype = C.c_int
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p] + [C.c_int] * len(extra) + [C.c_void_p, C.c_void_p, C.c_void_p]
            _check(fn(self.graph.handle, res, names, batch.blob, batch.offsets.ctypes.data, *extra, C.byref(text), C.byref(length), C.byref(skipped)))
            data = C.string_at(text.value, length.value)
            self.lib.gc_free(text)
            return data, int(skipped.value)

        def corrected(clipped):
            text, length, rec_off, n_rec, skipped = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64(), C.c_uint64()
            fn = self.lib.gc_format_corrected
            fn.restype = C.c_int
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            _check(fn(self.graph.handle, res, names, batch.blob, batch.offsets.ctypes.data, int(clipped), C.byref(text), C.byref(length), C.byref(rec_off), C.byref(n_rec), C.byref(skipped)))
            try:
                data = C.string_at(text.value, length.value)
                offsets = np.ctypeslib.as_array(C.cast(rec_off, _P(C.c_uint64)), shape=(int(n_rec.value) + 1,)).copy()
            finally:
                self.lib.gc_free(text)
                self.lib.gc_free(rec_off)
            return data, offsets, int(skipped.value)

        texts, skipped = {}, 0
        for fmt in formats:
            if fmt in ("corrected", "corrected_clipped"):
                texts[fmt], texts[fmt + "_rec_off"], skipped = corrected(fmt == "corrected_clipped")
            elif fmt == "gaf":
                texts[fmt], skipped = encode(self.lib.gc_format_gaf, int(cigar_match_mismatch_merge))
            elif fmt == "gam" and gam_level is not None:
                texts[fmt], skipped = encode(self.lib.gc_format_gam_level, int(gam_level))
            else:
                texts[fmt], skipped = encode(self.lib.gc_format_json if fmt == "json" else self.lib.gc_format_gam)
        return texts, skipped

    def format_batch(self, out, batch, names, formats=("gaf",), cigar_match_mismatch_merge=False, gam_level=None):
        """The writers on a result align_batch returned earlier (gc_format_gaf / _json / _gam): needs the graph and the result, not the stream - a host can
        format one batch while the stream aligns the next. names: one id per read, or a prebuilt ctypes array of them. gam_level: zlib level of the GAM's gzip
        members (default: the reference's, Z_DEFAULT_COMPRESSION). Returns ({format: bytes}, chained winners the result held no trace for)."""
        return self._format(out._holder.res, batch, names, tuple(formats), cigar_match_mismatch_merge, gam_level)

    def align_reads(self, reads, **kw):
        batch = ReadBatch(reads)
        try:
            return self.align_batch(batch, **kw)
        finally:
            batch.close()

    def close(self):
        if self.stream:
            self.lib.gc_stream_destroy(self.stream)
            self.stream = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
