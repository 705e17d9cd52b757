"""ctypes view of libpalace_hip.so (the C ABI declared in include/palace_hip.h).

This is plumbing for tests/ and bench.py: it adds no compute of its own and has no CPU
fallback -- if the HIP library is missing or a call fails, it raises.  The product's host side
is the C++ under palace_amd/host/, which links the same library.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("PALACE_HIP_SO") or os.path.join(_HERE, "libpalace_hip.so")     # override: A/B timing of two builds
_LIB = None


class PalaceError(RuntimeError):
    pass


def build(force: bool = False) -> str:
    """Compile csrc/*.hip for gfx950 with hipcc (cross-compiles without a GPU)."""
    args = ["make", "-C", os.path.join(_HERE, "csrc")]
    if force:
        subprocess.run(args + ["clean"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(args, check=True, stdout=subprocess.DEVNULL)
    return SO_PATH


class GraphParams(C.Structure):
    """palace_graph_params (defaults = generate_graph.cpp:20-44)."""
    _fields_ = [("max_end", C.c_int32), ("min_mapq", C.c_int32), ("max_nm", C.c_int32), ("enable_paired", C.c_int32),
                ("both_order", C.c_int32), ("reserved", C.c_int32), ("max_span_frac", C.c_double)]

    @classmethod
    def default(cls):
        return cls(300, 0, 5, 1, 0, 0, 0.80)


class BamCols(C.Structure):
    _fields_ = [("n", C.c_int64)] + [(k, C.c_void_p) for k in
                                     ("tid", "pos", "mtid", "mpos", "nm", "ref_len", "read_len", "clip_s", "clip_e",
                                      "flag", "mapq", "qkey", "sa_off")]


class GzipParams(C.Structure):
    _fields_ = [("stride", C.c_int64), ("span", C.c_int64), ("text_cap", C.c_int64), ("check_guards", C.c_int64)]


class GzipStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("chunks_found", "chunks_accepted", "false_hits", "rounds", "members", "spans", "batches", "text_bytes")] + \
        [("fallback", C.c_int32), ("guards_bad", C.c_int32)] + \
        [(k, C.c_double) for k in ("ms_upload", "ms_find", "ms_size", "ms_decode", "ms_chain", "ms_resolve", "ms_crc", "ms_sink")]


GZIP_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int)


class Stage04Inputs(C.Structure):
    """palace_stage04_inputs"""
    _fields_ = [("n_segs", C.c_int32), ("min_count", C.c_int32), ("seed", C.c_void_p), ("tlen", C.c_void_p), ("rank", C.c_void_p),
                ("name_len", C.c_void_p), ("n_paths", C.c_int64), ("path_off", C.c_void_p), ("path_tok", C.c_void_p)]


SA_ITEM_DTYPE = np.dtype([(k, np.int32) for k in ("tid2", "pos2", "mapq2", "nm2", "clip_s2", "clip_e2", "len2", "rev2")])
CAND_DTYPE = np.dtype([("ord", np.int64), ("qkey", np.uint64), ("left", np.int32), ("right", np.int32),
                       ("mtid", np.int32), ("ref_len", np.int32), ("dL", np.int32), ("dR", np.int32),
                       ("nmL", np.int32), ("nmR", np.int32), ("mapqL", np.int16), ("mapqR", np.int16),
                       ("kind", np.uint8), ("cls", np.uint8), ("found", np.uint8), ("in_fastg", np.uint8),
                       ("oL", np.uint8), ("oR", np.uint8), ("pad0", np.uint8), ("pad1", np.uint8), ("sa_index", np.int32)])
EDGE_DTYPE = np.dtype([("left", np.int32), ("right", np.int32), ("counts", np.uint32, 4), ("oL", np.uint8),
                       ("oR", np.uint8), ("pad", np.uint8, 6)])
FASTQ_CURSOR_DTYPE = np.dtype([("line", np.int64), ("reads", np.int64), ("bases", np.int64), ("open", np.int32), ("error", np.int32)])
DEPTH_CURSOR_DTYPE = np.dtype([("lines", np.int64), ("sum", np.uint64), ("bad_line", np.int64), ("win_runs", np.int64), ("win_name_bytes", np.int64),
                               ("tail_len", np.int32), ("tail_buf", np.int32), ("error", np.int32), ("reserved0", np.int32), ("reserved1", np.int64),
                               ("tail", np.uint8, (2, 4096))])
DEPTH_RUN_DTYPE = np.dtype([("sum", np.uint64), ("lines", np.uint64), ("name_off", np.uint32), ("name_len", np.uint32)])
assert DEPTH_CURSOR_DTYPE.itemsize == 64 + 8192 and DEPTH_RUN_DTYPE.itemsize == 24
FASTA_REC_DTYPE = np.dtype([(k, np.int64) for k in ("name_off", "name_len", "seq_off", "length", "line_bases", "line_width")])
FASTA_TILE_BYTES = 4096                 # PALACE_FASTA_TILE_BYTES
FAIDX_REGION_DTYPE = np.dtype([(k, np.int64) for k in ("rec", "beg", "len")])       # palace_faidx_region
CONTIG_FEATURES, CONTIG_FSUMS, CONTIG_CHUNK_BASES = 12288, 64, 4096     # PALACE_CONTIG_FEATURES, _FSUMS, _CHUNK_BASES
CONTIG_INFO_DTYPE = np.dtype([("length", np.int64), ("bases", np.int64)])
PATH_NOTHING, PATH_NOT_FOUND, PATH_REVERSE, PATH_SECOND_TRY = -1, -2, 1, 2


class BaiStatus(C.Structure):
    """palace_bai_status"""
    _fields_ = [("n_bad", C.c_int64), ("first_bad", C.c_int64), ("first_unsorted", C.c_int64), ("n_no_coor", C.c_int64)]


SORT_TILE = 4096        # PALACE_SORT_TILE: the keys one workgroup of palace_sort_u64 ranks per pass
# the eref count partition (csrc/eref.hip, csrc/eref_common.hpp)
EREF_BIN_THREADS = 512          # kBinThreads: lanes of a level-1 workgroup (a tile is kBinThreads * P positions, P = 6 or 8)
EREF_L1_REPLICAS = 32           # kL1Replicas: regions per level-1 bucket; a tile writes to replica blockIdx.x % kL1Replicas
EREF_GROUP_KEYS = 5             # kGroupKeys: keys of one 16-byte level-1 group
EREF_TILE2_GROUPS = 5120        # kTile2Groups: groups one level-2 workgroup takes
EREF_ROW_SLOTS = 72             # kRowSlots: slots of a level-2 staging row
EREF_XCDS = 8                   # kXcds: sub-regions of a fine bucket's region
EREF_COUNT_ROUND_VECTORS = 1024  # kBatch * kCountThreads: 8-key vectors one round of the count kernel's loop applies


class FastaStatus(C.Structure):
    """palace_fasta_status"""
    _fields_ = [("n_records", C.c_int64), ("bad_line", C.c_int64), ("error", C.c_int32), ("reserved", C.c_int32)]


class ReadqcParams(C.Structure):
    """palace_readqc_params (defaults = fastp's for paired input)."""
    _fields_ = [(k, C.c_int32) for k in ("qualified_quality", "unqualified_percent", "n_limit", "min_length", "no_trim", "no_quality_filter",
                                         "no_length_filter", "overlap_require", "diff_limit", "diff_pct", "diff_window", "reserved")]

    @classmethod
    def default(cls, **kw):
        p = cls(15, 40, 5, 15, 0, 0, 0, 30, 5, 20, 50, 0)
        for k, v in kw.items():
            assert hasattr(p, k), k
            setattr(p, k, int(v))
        return p


READQC_OUT = ("reads_before", "bases_before", "reads_after", "bases_after", "low_quality", "too_many_n", "too_short", "trimmed_reads", "trimmed_bases",
              "bytes_1", "bytes_2")                # PALACE_READQC_* of include/palace_hip.h
READQC_ISIZE_MAX = 512  # PALACE_READQC_ISIZE_MAX: the insert-size histogram's "unknown" slot
READQC_CYCLE_TILE = 256  # kCycleTile of csrc/readqc.hip: the cycles a workgroup of palace_readqc_cycle_stats owns

assert CAND_DTYPE.itemsize == 64 and EDGE_DTYPE.itemsize == 32 and SA_ITEM_DTYPE.itemsize == 32 and C.sizeof(ReadqcParams) == 48

_SIGS = {
    "palace_ctx_create": [C.c_int, C.POINTER(C.c_void_p)],
    "palace_ctx_create_prio": [C.c_int, C.c_int, C.POINTER(C.c_void_p)],
    "palace_ctx_create_on_stream": [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)],
    "palace_ctx_destroy": [C.c_void_p],
    "palace_sync": [C.c_void_p],
    "palace_malloc": [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)],
    "palace_free": [C.c_void_p, C.c_void_p],
    "palace_memset": [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t],
    "palace_h2d": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t],
    "palace_d2h": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t],
    "palace_d2d": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t],
    "palace_host_alloc": [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)],
    "palace_host_free": [C.c_void_p, C.c_void_p],
    "palace_d2h_async": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t],
    "palace_h2d_async": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t],
    "palace_mark_wait": [C.c_void_p, C.c_int],
    "palace_mark_wait_for": [C.c_void_p, C.c_int, C.c_double],
    "palace_wait_for_mark": [C.c_void_p, C.c_void_p, C.c_int],
    "palace_timer_begin": [C.c_void_p],
    "palace_timer_end": [C.c_void_p, C.POINTER(C.c_float)],
    "palace_mark": [C.c_void_p, C.c_int],
    "palace_mark_elapsed": [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)],
    "palace_eref_set_coder": [C.c_void_p, C.c_void_p],
    "palace_eref_index_refs": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
    "palace_eref_table_reset": [C.c_void_p],
    "palace_eref_reserve": [C.c_void_p, C.c_int64],
    "palace_eref_count_reads": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64],
    "palace_eref_pack_reads": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "palace_eref_count_reads_packed": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64],
    "palace_eref_set_count_mode": [C.c_void_p, C.c_int, C.c_int64],
    "palace_eref_set_key_buckets": [C.c_void_p, C.c_void_p],
    "palace_eref_set_option": [C.c_void_p, C.c_char_p, C.c_int64],
    "palace_eref_scan_refs": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int,
                              C.c_void_p],
    "palace_eref_probe_index_build": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_void_p)],
    "palace_eref_attach_probe_index": [C.c_void_p, C.c_void_p],
    "palace_eref_entry_layout": [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)],
    "palace_eref_entry_buffers_attach": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "palace_eref_entry_buffers": [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)],
    "palace_eref_entry_hits_from_counts": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t],
    "palace_eref_entry_hits_complete": [C.c_void_p, C.c_void_p, C.c_int64],
    "palace_eref_entry_counts_valid": [C.c_void_p, C.c_void_p],
    "palace_eref_probe_index_free": [C.c_void_p, C.c_void_p],
    "palace_eref_scan_refs_indexed": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int,
                                      C.c_void_p],
    "palace_eref_table_planes": [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)],
    "palace_eref_table_attach": [C.c_void_p, C.POINTER(C.c_void_p)],
    "palace_eref_table_invalidate": [C.c_void_p],
    "palace_eref_table_merge_slices": [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t],
    "palace_eref_table_merge_slices_packed": [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t],
    "palace_eref_table_pack_low": [C.c_void_p, C.c_void_p],
    "palace_eref_plane_pack": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p],
    "palace_eref_plane_unpack": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p],
    "palace_eref_table_lookup": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p],
    "palace_eref_table_popcounts": [C.c_void_p, C.POINTER(C.c_uint64)],
    "palace_graph_classify": [C.c_void_p, C.POINTER(BamCols), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_int64, C.POINTER(GraphParams), C.c_int64, C.c_void_p, C.c_void_p,
                              C.c_int64, C.POINTER(C.c_int64)],
    "palace_depth_sum_covered": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                 C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
    "palace_depth_per_contig": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p],
    "palace_graph_copy_numbers": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_void_p],
    "palace_match_greedy": [C.c_void_p, C.c_int32, C.c_int64] + [C.c_void_p] * 10 + [C.POINTER(C.c_int32)],
    "palace_match_arcs_from_edges": [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)],
    "palace_match_set_option": [C.c_void_p, C.c_char_p, C.c_int64],
    "palace_match_last_run": [C.c_void_p, C.POINTER(C.c_int64)],
    "palace_match_decompose":[C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                               C.c_int32, C.POINTER(C.c_void_p)],
    "palace_match_decompose_ex": [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                  C.c_int32, C.c_int32, C.POINTER(C.c_void_p)],
    "palace_graph_resolve": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(GraphParams), C.c_void_p,
                             C.c_void_p, C.c_int64, C.POINTER(C.c_int64)],
    "palace_graph_classify_ex": [C.c_void_p, C.POINTER(BamCols), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_int64, C.POINTER(GraphParams), C.c_int64, C.c_void_p, C.c_void_p,
                                 C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "palace_graph_classify_ix": [C.c_void_p, C.POINTER(BamCols), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(GraphParams), C.c_int64, C.c_void_p, C.c_void_p,
                                 C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "palace_graph_fastg_offsets": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p],
    "palace_bgzf_inflate": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "palace_fastq_scratch_bytes": [C.c_int64],          # (returns size_t: restype set below)
    "palace_crc32_members": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "palace_bgzf_deflate": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "palace_bgzf_deflate_lz": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "palace_bgzf_compact": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "palace_depth_text_create": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                 C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)],
    "palace_depth_text_destroy": [C.c_void_p, C.c_void_p],
    "palace_depth_text_emit": [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p],
    "palace_depth_text_windows": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "palace_gzip_inflate": [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(GzipParams), GZIP_SINK, C.c_void_p, C.POINTER(GzipStats)],
    "palace_fastq_parse": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                           C.c_void_p, C.c_size_t],
    "palace_depth_parse_scratch_bytes": [C.c_int64],    # (returns size_t: restype set below)
    "palace_depth_parse": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                           C.c_void_p, C.c_size_t],
    "palace_graph_score_border": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(GraphParams)],
    "palace_graph_resolve_ex": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.POINTER(GraphParams), C.c_void_p,
                                C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int64)],
    "palace_bam_walk_scratch_bytes": [C.c_int64, C.c_int64, C.c_int64],          # (returns size_t: restype set below)
    "palace_bam_walk": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int64,
                        C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "palace_bam_walk_starts": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int64],
    "palace_bam_match_segments": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_int64, C.POINTER(C.c_int64)],
    "palace_bam_columns": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_uint64, C.POINTER(BamCols)],
    "palace_bam_name_keys": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_uint64, C.c_void_p],
    "palace_bam_names_differ": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)],
    "palace_bam_names_create": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)],
    "palace_bam_names_destroy": [C.c_void_p, C.c_void_p],
    "palace_bam_sa_items": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                            C.POINTER(C.c_int64)],
    "palace_stage04_create": [C.c_void_p, C.POINTER(Stage04Inputs), C.POINTER(C.c_void_p)],
    "palace_stage04_destroy": [C.c_void_p, C.c_void_p],
    "palace_stage04_reserve": [C.c_void_p, C.c_void_p, C.c_int64],
    "palace_stage04_filter": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64],
    "palace_stage04_flags": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64],
    "palace_stage04_counts": [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)],
    "palace_stage04_match": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32],
    "palace_stage04_result": [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)],
    "palace_fasta_index_scratch_bytes": [C.c_int64],    # (returns size_t: restype set below)
    "palace_fasta_index": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.POINTER(FastaStatus)],
    "palace_fasta_names_create": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_void_p)],
    "palace_fasta_names_destroy": [C.c_void_p, C.c_void_p],
    "palace_path_resolve": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p],
    "palace_path_fasta_lengths": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
    "palace_fastg_derive": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(FastaStatus)],
    "palace_fastg_plan": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "palace_fastg_write": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p],
    "palace_fai_rows_plan": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int64)],
    "palace_fai_rows_write": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p],
    "palace_faidx_resolve": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p],
    "palace_faidx_plan": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "palace_faidx_write": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64,
                           C.c_int64, C.c_void_p],
    "palace_path_fasta_write": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_int64, C.c_int64, C.c_void_p],
    "palace_cycle_trim": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                          C.c_void_p, C.c_void_p],
    "palace_final_fasta_lengths": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p],
    "palace_final_fasta_write": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p],
    "palace_blast_identity_cuts": [C.c_double, C.POINTER(C.c_int64)],
    "palace_blast_groups": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_double, C.POINTER(C.c_int64), C.c_void_p,
                            C.POINTER(C.c_int64)],
    "palace_filter_result_plan": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "palace_paths_first_of_equal": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p],
    "palace_path_borders": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p],
    "palace_path_tandems": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)],
    "palace_paths_length_relation_bytes": [C.c_int64],  # (returns size_t: restype set below)
    "palace_paths_length_relation": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p],
    "palace_paths_base_set_in": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p],
    "palace_bam_sort_keys": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    "palace_sort_u64_scratch_bytes": [C.c_int64],       # (returns size_t: restype set below)
    "palace_sort_u64": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_size_t],
    "palace_bam_gather_plan": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)],
    "palace_bam_gather_write": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p],
    "palace_bai_records": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                           C.POINTER(BaiStatus)],
    "palace_bai_chunks": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                          C.c_int64, C.POINTER(C.c_int64)],
    "palace_bai_linear": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                          C.c_void_p, C.c_int64, C.c_void_p],
    "palace_bgzf_voffsets": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p],
    "palace_sam_scratch_bytes": [C.c_int64],            # (returns size_t: restype set below)
    "palace_sam_lines": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)],
    "palace_sam_plan": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_uint32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                        C.POINTER(C.c_int64)],
    "palace_sam_encode": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "palace_fastq_records": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int64)],
    "palace_readqc_plan": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(ReadqcParams), C.c_void_p, C.c_void_p, C.c_void_p,
                           C.c_void_p, C.POINTER(C.c_int64)],
    "palace_readqc_write": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p],
    "palace_readqc_plan_ex": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(ReadqcParams), C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)],
    "palace_readqc_insert_sizes": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(ReadqcParams), C.c_void_p],
    "palace_readqc_cycle_stats": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p],
    "palace_contig_features_scratch_bytes": [C.c_int64, C.c_int64],    # (returns size_t: restype set below)
    "palace_contig_features": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_size_t],
}


def declared_symbols():
    """Every function include/palace_hip.h declares (parsed from the header itself)."""
    import re
    text = open(os.path.join(_HERE, "..", "include", "palace_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(palace_[a-z0-9_]+)\s*\(", text)))


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        if not os.path.exists(SO_PATH):
            raise PalaceError(f"{SO_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        _LIB = C.CDLL(SO_PATH)
        _LIB.palace_last_error.restype = C.c_char_p
        _LIB.palace_version.restype = C.c_char_p
        _LIB.palace_stream.restype = C.c_void_p
        _LIB.palace_stream.argtypes = [C.c_void_p]
        _LIB.palace_eref_packed_bytes.restype = C.c_size_t
        _LIB.palace_eref_packed_bytes.argtypes = [C.c_int64]
        for nm, rt in (("count", C.c_int64), ("bare_count", C.c_int64), ("bare", C.POINTER(C.c_uint64)), ("offsets", C.POINTER(C.c_int64)), ("verts", C.POINTER(C.c_int32)),
                       ("kind", C.POINTER(C.c_uint8)), ("iter", C.POINTER(C.c_int32)), ("open_at", C.POINTER(C.c_int32))):
            fn = getattr(_LIB, "palace_match_result_" + nm)
            fn.argtypes = [C.c_void_p]
            fn.restype = rt
        _LIB.palace_match_result_free.argtypes = [C.c_void_p]
        _LIB.palace_match_result_free.restype = None
        for name, sig in _SIGS.items():
            fn = getattr(_LIB, name)
            fn.argtypes = sig
            fn.restype = C.c_int
        _LIB.palace_fastq_scratch_bytes.restype = C.c_size_t
        _LIB.palace_bam_walk_scratch_bytes.restype = C.c_size_t
        _LIB.palace_depth_parse_scratch_bytes.restype = C.c_size_t
        _LIB.palace_fasta_index_scratch_bytes.restype = C.c_size_t
        _LIB.palace_sort_u64_scratch_bytes.restype = C.c_size_t
        _LIB.palace_sam_scratch_bytes.restype = C.c_size_t
        _LIB.palace_contig_features_scratch_bytes.restype = C.c_size_t
        _LIB.palace_paths_length_relation_bytes.restype = C.c_size_t
    return _LIB


def _check(rc: int, what: str):
    if rc != 0:
        raise PalaceError(f"{what} -> {rc}: {lib().palace_last_error().decode()}")


class DevBuf:
    """A device allocation owned through palace_malloc/palace_free."""

    def __init__(self, ctx: "Ctx", nbytes: int, dtype=np.uint8, shape=None):
        self.ctx, self.nbytes, self.dtype, self.shape = ctx, int(nbytes), np.dtype(dtype), shape
        p = C.c_void_p()
        _check(lib().palace_malloc(ctx.h, self.nbytes, C.byref(p)), "palace_malloc")
        self.ptr = p.value

    def to_host(self) -> np.ndarray:
        out = np.empty(self.nbytes // self.dtype.itemsize, dtype=self.dtype)
        _check(lib().palace_d2h(self.ctx.h, out.ctypes.data, self.ptr, self.nbytes), "palace_d2h")
        return out.reshape(self.shape) if self.shape is not None else out

    def free(self):
        if self.ptr:
            lib().palace_free(self.ctx.h, self.ptr)
            self.ptr = None


class Ctx:
    """One device context (one HIP stream).  `calls` go straight to the C ABI."""

    def __init__(self, device: int = 0, high_priority: bool = False, stream: int | None = None):
        """stream: a hipStream_t of the caller's to run on instead of a stream of the context's own (palace_ctx_create_on_stream)"""
        h = C.c_void_p()
        if stream:
            _check(lib().palace_ctx_create_on_stream(device, C.c_void_p(stream), C.byref(h)), "palace_ctx_create_on_stream")
        else:
            _check(lib().palace_ctx_create_prio(device, int(high_priority), C.byref(h)), "palace_ctx_create_prio")
        self.h = h
        self.device = device

    def close(self):
        if self.h:
            lib().palace_ctx_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- memory ---------------------------------------------------------------------------
    def upload(self, arr: np.ndarray) -> DevBuf:
        a = np.ascontiguousarray(arr)
        b = DevBuf(self, max(a.nbytes, 1), a.dtype, a.shape)
        if a.nbytes:
            _check(lib().palace_h2d(self.h, b.ptr, a.ctypes.data, a.nbytes), "palace_h2d")
        return b

    def empty(self, shape, dtype) -> DevBuf:
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return DevBuf(self, max(n, 1), dtype, tuple(np.atleast_1d(shape)))

    def d2d(self, dst_ptr: int, src_ptr: int, nbytes: int):
        _check(lib().palace_d2d(self.h, dst_ptr, src_ptr, nbytes), "palace_d2d")

    def memset(self, ptr: int, value: int, nbytes: int):
        _check(lib().palace_memset(self.h, ptr, value, nbytes), "palace_memset")

    def sync(self):
        _check(lib().palace_sync(self.h), "palace_sync")

    def timer_begin(self):
        _check(lib().palace_timer_begin(self.h), "palace_timer_begin")

    def timer_end(self) -> float:
        ms = C.c_float()
        _check(lib().palace_timer_end(self.h, C.byref(ms)), "palace_timer_end")
        return ms.value

    def mark(self, i: int):
        _check(lib().palace_mark(self.h, i), "palace_mark")

    def mark_wait(self, i: int):
        """the host waits for mark i of this context's stream"""
        _check(lib().palace_mark_wait(self.h, i), "palace_mark_wait")

    def wait_for_mark(self, other: "Ctx", i: int):
        _check(lib().palace_wait_for_mark(self.h, other.h, i), "palace_wait_for_mark")

    def mark_elapsed(self, a: int, b: int) -> float:
        ms = C.c_float()
        _check(lib().palace_mark_elapsed(self.h, a, b, C.byref(ms)), "palace_mark_elapsed")
        return ms.value

    @property
    def stream(self) -> int:
        return lib().palace_stream(self.h)

    # -- eref -----------------------------------------------------------------------------
    def eref_set_coder(self, header400: np.ndarray):
        h = np.ascontiguousarray(header400, dtype=np.uint8)
        assert h.size == 400
        _check(lib().palace_eref_set_coder(self.h, h.ctypes.data), "palace_eref_set_coder")

    def eref_table_reset(self):
        _check(lib().palace_eref_table_reset(self.h), "palace_eref_table_reset")

    def eref_count_reads(self, d_bases: DevBuf, d_offsets: DevBuf, n_reads: int, d_keep: DevBuf | None = None,
                         total_bases: int = -1):
        _check(lib().palace_eref_count_reads(self.h, d_bases.ptr, d_offsets.ptr, n_reads,
                                             d_keep.ptr if d_keep else None, total_bases), "palace_eref_count_reads")

    def eref_pack_reads(self, d_bases: DevBuf, d_offsets: DevBuf, n_reads: int, d_keep, total_bases: int, d_p0: DevBuf, d_p1: DevBuf, d_u: DevBuf):
        _check(lib().palace_eref_pack_reads(self.h, d_bases.ptr, d_offsets.ptr, n_reads, d_keep.ptr if d_keep else None, total_bases,
                                            d_p0.ptr, d_p1.ptr, d_u.ptr), "palace_eref_pack_reads")

    def eref_count_reads_packed(self, d_p0: DevBuf, d_p1: DevBuf, d_u: DevBuf, n_positions: int, n_reads_hint: int = 0):
        _check(lib().palace_eref_count_reads_packed(self.h, d_p0.ptr, d_p1.ptr, d_u.ptr, n_positions, n_reads_hint),
               "palace_eref_count_reads_packed")

    def eref_set_count_mode(self, mode: int, bucket_cap: int = 0):
        _check(lib().palace_eref_set_count_mode(self.h, mode, bucket_cap), "palace_eref_set_count_mode")

    def eref_set_key_buckets(self, buckets=None):
        """the level-1 buckets (0..127) count calls take in; None = all"""
        m = (C.c_uint32 * 4)(*([0xFFFFFFFF] * 4 if buckets is None else [0] * 4))
        for b in ([] if buckets is None else buckets):
            m[b >> 5] |= 1 << (b & 31)
        _check(lib().palace_eref_set_key_buckets(self.h, m), "palace_eref_set_key_buckets")

    def eref_set_option(self, name: str, value: int):
        _check(lib().palace_eref_set_option(self.h, name.encode(), value), "palace_eref_set_option")

    def eref_scan_refs(self, d_bases: DevBuf, d_offsets: DevBuf, n_refs: int, total_bases: int,
                       one_min: int, three_min: int, d_rows: DevBuf):
        _check(lib().palace_eref_scan_refs(self.h, d_bases.ptr, d_offsets.ptr, n_refs, total_bases,
                                           one_min, three_min, d_rows.ptr), "palace_eref_scan_refs")

    def eref_probe_index_build(self, d_bases: DevBuf, d_offsets: DevBuf, n_refs: int, total_bases: int) -> C.c_void_p:
        """Per-DB probe index (device resident); free with eref_probe_index_free."""
        h = C.c_void_p()
        _check(lib().palace_eref_probe_index_build(self.h, d_bases.ptr, d_offsets.ptr, n_refs, total_bases, C.byref(h)),
               "palace_eref_probe_index_build")
        return h

    def eref_attach_probe_index(self, index):
        """count calls that run as the final count also probe channel 0 of this DB (palace_eref_attach_probe_index); None detaches"""
        _check(lib().palace_eref_attach_probe_index(self.h, index), "palace_eref_attach_probe_index")

    def eref_entry_layout(self, index):
        """-> (bytes of the partial-count block, bytes of the hit-bit block) of a probe index (palace_eref_entry_layout)"""
        cb, hb = C.c_size_t(), C.c_size_t()
        _check(lib().palace_eref_entry_layout(index, C.byref(cb), C.byref(hb)), "palace_eref_entry_layout")
        return int(cb.value), int(hb.value)

    def eref_entry_buffers_attach(self, index, counts_ptr: int | None, hits_ptr: int | None):
        """the caller's device buffers stand in for the index's count / hit-bit blocks (None: the index's own)"""
        _check(lib().palace_eref_entry_buffers_attach(self.h, index, counts_ptr, hits_ptr), "palace_eref_entry_buffers_attach")

    def eref_entry_buffers(self, index):
        """-> (device pointer of the count block, of the hit-bit block) as they are attached now (counts: None before a first attach)"""
        counts, hits = C.c_void_p(), C.c_void_p()
        _check(lib().palace_eref_entry_buffers(index, C.byref(counts), C.byref(hits)), "palace_eref_entry_buffers")
        return counts.value, hits.value

    def eref_entry_hits_from_counts(self, index, parts_ptr: int, n_parts: int, part_stride: int, off: int, nbytes: int):
        """sum n_parts partial-count arrays over the count block's bytes [off, off + nbytes) into the hit bits of that entry range"""
        _check(lib().palace_eref_entry_hits_from_counts(self.h, index, parts_ptr, n_parts, part_stride, off, nbytes), "palace_eref_entry_hits_from_counts")

    def eref_entry_counts_valid(self, index) -> bool:
        """a count call of this context (option probe_all_sets 2) stands behind the count block `index` points at"""
        return bool(lib().palace_eref_entry_counts_valid(self.h, index))

    def eref_entry_hits_complete(self, index, keys_counted: int = -1):
        """the hit-bit block of the attached index is whole: the next indexed scan starts from it"""
        _check(lib().palace_eref_entry_hits_complete(self.h, index, keys_counted), "palace_eref_entry_hits_complete")

    def eref_probe_index_free(self, index: C.c_void_p):
        _check(lib().palace_eref_probe_index_free(self.h, index), "palace_eref_probe_index_free")

    def eref_scan_refs_indexed(self, index: C.c_void_p, d_bases: DevBuf, d_offsets: DevBuf, n_refs: int, total_bases: int,
                               one_min: int, three_min: int, d_rows: DevBuf):
        _check(lib().palace_eref_scan_refs_indexed(self.h, index, d_bases.ptr, d_offsets.ptr, n_refs, total_bases,
                                                   one_min, three_min, d_rows.ptr), "palace_eref_scan_refs_indexed")

    def eref_index_refs(self, d_bases: DevBuf, d_offsets: DevBuf, n_refs: int, d_out: DevBuf, d_out_offsets: DevBuf):
        _check(lib().palace_eref_index_refs(self.h, d_bases.ptr, d_offsets.ptr, n_refs, d_out.ptr,
                                            d_out_offsets.ptr), "palace_eref_index_refs")

    def eref_table_lookup(self, keys: np.ndarray) -> np.ndarray:
        k = self.upload(np.ascontiguousarray(keys, dtype=np.uint32))
        out = self.empty(len(keys), np.uint8)
        _check(lib().palace_eref_table_lookup(self.h, k.ptr, len(keys), out.ptr), "palace_eref_table_lookup")
        res = out.to_host()
        k.free()
        out.free()
        return res

    def eref_table_popcounts(self):
        out = (C.c_uint64 * 3)()
        _check(lib().palace_eref_table_popcounts(self.h, out), "palace_eref_table_popcounts")
        return [int(v) for v in out]

    def eref_table_planes(self):
        ptrs = (C.c_void_p * 3)()
        nbytes = C.c_size_t()
        _check(lib().palace_eref_table_planes(self.h, ptrs, C.byref(nbytes)), "palace_eref_table_planes")
        return [int(p) for p in ptrs], int(nbytes.value)

    def eref_plane_write(self, p: int, off: int, data: np.ndarray):
        """bytes [off, off + len(data)) of plane p (0..2) <- data, through the pointers of eref_table_planes; then the invalidate
        the header's contract for caller-written planes demands"""
        planes, nbytes = self.eref_table_planes()
        a = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        assert 0 <= off and off + a.nbytes <= nbytes
        if a.nbytes:
            _check(lib().palace_h2d(self.h, planes[p] + off, a.ctypes.data, a.nbytes), "palace_h2d")
        self.eref_table_invalidate()

    def eref_plane_read(self, p: int, off: int, n: int) -> np.ndarray:
        """bytes [off, off + n) of plane p (0..2)"""
        planes, nbytes = self.eref_table_planes()
        assert 0 <= off and off + n <= nbytes
        out = np.empty(n, dtype=np.uint8)
        if n:
            _check(lib().palace_d2h(self.h, out.ctypes.data, planes[p] + off, n), "palace_d2h")
        return out

    def eref_table_attach(self, ptrs):
        arr = (C.c_void_p * 3)(*[int(p) for p in ptrs])
        _check(lib().palace_eref_table_attach(self.h, arr), "palace_eref_table_attach")

    def match_set_option(self, name: str, value: int):
        _check(lib().palace_match_set_option(self.h, name.encode(), value), "palace_match_set_option")

    def eref_table_invalidate(self):
        _check(lib().palace_eref_table_invalidate(self.h), "palace_eref_table_invalidate")

    def eref_table_merge_slices(self, parts_ptr: int, n_parts: int, slice_off: int, slice_bytes: int, packed: bool = False):
        fn = lib().palace_eref_table_merge_slices_packed if packed else lib().palace_eref_table_merge_slices
        _check(fn(self.h, parts_ptr, n_parts, slice_off, slice_bytes), "palace_eref_table_merge_slices")

    def eref_table_pack_low(self, low_ptr: int):
        _check(lib().palace_eref_table_pack_low(self.h, low_ptr), "palace_eref_table_pack_low")

    @staticmethod
    def _bucket_mask(buckets):
        m = (C.c_uint32 * 4)(0, 0, 0, 0)
        for b in buckets:
            m[b >> 5] |= 1 << (b & 31)
        return m

    def eref_plane_pack(self, buckets, counts_ptr: int, keys_ptr: int, cap_keys: int, first_ptr: int):
        """the '>= 3' plane of the level-1 buckets `buckets` in sparse form (palace_eref_plane_pack): device pointers to
        512 * len(buckets) uint32 counts, cap_keys uint16 keys, 512 * len(buckets) + 1 uint64 prefix entries"""
        _check(lib().palace_eref_plane_pack(self.h, self._bucket_mask(buckets), counts_ptr, keys_ptr, cap_keys, first_ptr), "palace_eref_plane_pack")

    def eref_plane_unpack(self, buckets, counts_ptr: int, keys_ptr: int, cap_keys: int, first_ptr: int):
        _check(lib().palace_eref_plane_unpack(self.h, self._bucket_mask(buckets), counts_ptr, keys_ptr, cap_keys, first_ptr), "palace_eref_plane_unpack")

    # -- compressed FASTQ for eref ---------------------------------------------------------
    def crc32_members(self, d_data_ptr: int, n_members: int, d_off: DevBuf, d_len: DevBuf, d_crc: DevBuf):
        _check(lib().palace_crc32_members(self.h, d_data_ptr, n_members, d_off.ptr, d_len.ptr, d_crc.ptr), "palace_crc32_members")

    def bgzf_deflate(self, d_text_ptr: int, n_members: int, d_off: DevBuf, d_len: DevBuf, d_crc: DevBuf, d_slots: DevBuf, d_member_len: DevBuf):
        _check(lib().palace_bgzf_deflate(self.h, d_text_ptr, n_members, d_off.ptr, d_len.ptr, d_crc.ptr, d_slots.ptr, d_member_len.ptr),
               "palace_bgzf_deflate")

    def bgzf_deflate_lz(self, d_text_ptr: int, n_members: int, d_off: DevBuf, d_len: DevBuf, d_crc: DevBuf, d_slots: DevBuf, d_member_len: DevBuf):
        _check(lib().palace_bgzf_deflate_lz(self.h, d_text_ptr, n_members, d_off.ptr, d_len.ptr, d_crc.ptr, d_slots.ptr, d_member_len.ptr),
               "palace_bgzf_deflate_lz")

    def bgzf_compact(self, d_slots: DevBuf, n_members: int, d_member_len: DevBuf, d_file: DevBuf, d_member_off: DevBuf):
        _check(lib().palace_bgzf_compact(self.h, d_slots.ptr, n_members, d_member_len.ptr, d_file.ptr, d_member_off.ptr), "palace_bgzf_compact")

    def fastq_parse(self, d_text_ptr: int, n: int, final_window: bool, d_cursor: DevBuf, d_bases: DevBuf, bases_cap: int,
                    d_offsets: DevBuf, offsets_cap: int, d_scratch: DevBuf):
        _check(lib().palace_fastq_parse(self.h, d_text_ptr, n, int(final_window), d_cursor.ptr, d_bases.ptr, bases_cap, d_offsets.ptr,
                                        offsets_cap, d_scratch.ptr, d_scratch.nbytes), "palace_fastq_parse")


def depth_parse_windows(ctx: Ctx, text: bytes, cuts=(), runs_cap: int | None = None, names_cap: int | None = None, guard: int = 64):
    """`samtools depth` text through palace_depth_parse, handed over in windows cut at the ascending positions `cuts` (equal
    positions give empty windows).  Returns (the cursor after the last window, per window the list of its runs as
    (name bytes, depth sum, lines) -- None for a window refused for its capacities --, whether the `guard` bytes behind d_runs and
    d_names are as they were, whether ALL of d_runs and d_names is as it was).  runs_cap / names_cap: the capacities handed to every
    call (default: what any window of the text could need)."""
    text = bytes(text)
    bounds = [0] + [min(max(int(c), 0), len(text)) for c in cuts] + [len(text)]
    widest = max(b - a for a, b in zip(bounds, bounds[1:]))
    runs_cap = len(text) // 2 + 2 if runs_cap is None else runs_cap
    names_cap = len(text) + 1 if names_cap is None else names_cap
    d_win = DevBuf(ctx, max(16, widest + 16))
    fill = np.full(runs_cap * 24 + guard, 0xA5, np.uint8), np.full(names_cap + guard, 0xA5, np.uint8)
    d_runs, d_names = ctx.upload(fill[0]), ctx.upload(fill[1])
    d_scratch = DevBuf(ctx, int(lib().palace_depth_parse_scratch_bytes(widest)))
    d_cur = ctx.upload(np.zeros(1, DEPTH_CURSOR_DTYPE))
    windows = []
    try:
        for k, (a, b) in enumerate(zip(bounds, bounds[1:])):
            chunk = np.frombuffer(text[a:b], dtype=np.uint8)
            if len(chunk):
                _check(lib().palace_h2d(ctx.h, d_win.ptr, chunk.ctypes.data, len(chunk)), "palace_h2d")
            _check(lib().palace_depth_parse(ctx.h, d_win.ptr, len(chunk), int(k == len(bounds) - 2), d_cur.ptr, d_runs.ptr, runs_cap, d_names.ptr,
                                            names_cap, d_scratch.ptr, d_scratch.nbytes), "palace_depth_parse")
            ctx.sync()
            cur = d_cur.to_host().view(DEPTH_CURSOR_DTYPE)[0]
            if cur["error"]:
                windows.append(None)
                continue
            raw_runs, names = d_runs.to_host(), d_names.to_host().tobytes()
            runs = raw_runs[:int(cur["win_runs"]) * 24].view(DEPTH_RUN_DTYPE)
            windows.append([(names[int(r["name_off"]):int(r["name_off"]) + int(r["name_len"])], int(r["sum"]), int(r["lines"])) for r in runs])
        cur = d_cur.to_host().view(DEPTH_CURSOR_DTYPE)[0].copy()
        intact = bool((d_runs.to_host()[runs_cap * 24:] == 0xA5).all() and (d_names.to_host()[names_cap:] == 0xA5).all())
        untouched = bool((d_runs.to_host() == 0xA5).all() and (d_names.to_host() == 0xA5).all())
        return cur, windows, intact, untouched
    finally:
        for buf in (d_win, d_runs, d_names, d_scratch, d_cur):
            buf.free()


_FILL64 = 0xA5A5A5A5A5A5A5A5


def _depth_inputs(ctx: Ctx, tlen, segs, tbase_entries: int):
    """the device arrays the depth entry points share: tlen (int32), tbase (int64, the first `tbase_entries` exclusive prefixes) and the
    three segment columns exactly as given -- nothing filtered, nothing sorted -> (buffers, n_targets, total_len, n_segs)"""
    tl = np.ascontiguousarray(tlen, dtype=np.int32).reshape(-1)
    tbase = np.concatenate([np.zeros(1, np.int64), np.cumsum(tl, dtype=np.int64)])
    if isinstance(segs, np.ndarray) and segs.ndim == 2:
        assert segs.shape[1] == 3
        segs = (segs[:, 0], segs[:, 1], segs[:, 2])
    cols = [np.asarray(c) for c in segs]
    assert len(cols) == 3 and all(c.ndim == 1 and len(c) == len(cols[0]) and c.dtype == np.int32 for c in cols), "segments are three int32 columns"
    bufs = [ctx.upload(c) for c in cols] + [ctx.upload(tl), ctx.upload(tbase[:tbase_entries])]
    return bufs, len(tl), int(tbase[-1]), len(cols[0])


def depth_sum_covered(ctx: Ctx, tlen, segs):
    """palace_depth_sum_covered -> (sum, covered).  segs: three int32 arrays (tid, pos, len) or one (n, 3) array; d_tbase has exactly
    n_targets entries, as the header says."""
    bufs, n_targets, total_len, n = _depth_inputs(ctx, tlen, segs, len(np.atleast_1d(tlen)))
    s, c = C.c_uint64(_FILL64), C.c_uint64(_FILL64)
    try:
        _check(lib().palace_depth_sum_covered(ctx.h, n, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, n_targets, bufs[3].ptr, bufs[4].ptr, total_len,
                                              C.byref(s), C.byref(c)), "palace_depth_sum_covered")
        return int(s.value), int(c.value)
    finally:
        for b in bufs:
            b.free()


def depth_per_contig(ctx: Ctx, tlen, segs):
    """palace_depth_per_contig -> (sum, covered, contig_sum[], contig_covered[]).  The two device arrays hold a non-zero pattern
    before the call, so an entry the call leaves alone shows."""
    bufs, n_targets, total_len, n = _depth_inputs(ctx, tlen, segs, len(np.atleast_1d(tlen)))
    bufs += [ctx.upload(np.full(max(n_targets, 1), _FILL64, np.uint64)) for _ in range(2)]
    s, c = C.c_uint64(_FILL64), C.c_uint64(_FILL64)
    try:
        _check(lib().palace_depth_per_contig(ctx.h, n, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, n_targets, bufs[3].ptr, bufs[4].ptr, total_len,
                                             C.byref(s), C.byref(c), bufs[5].ptr, bufs[6].ptr), "palace_depth_per_contig")
        ctx.sync()
        return int(s.value), int(c.value), bufs[5].to_host()[:n_targets].copy(), bufs[6].to_host()[:n_targets].copy()
    finally:
        for b in bufs:
            b.free()


class DepthText:
    """palace_depth_text_create and what is asked of its handle.  tlen, tbase (n_targets + 1 entries), the names blob and the name
    offsets stay on the device until close(), as the header demands; the segments are passed as given and freed after create."""

    def __init__(self, ctx: Ctx, tlen, names, segs):
        self.ctx, self.h, self._keep = ctx, C.c_void_p(), []
        names = [bytes(x) for x in names]
        assert len(names) == len(np.atleast_1d(tlen))
        name_off = np.concatenate([np.zeros(1, np.int64), np.cumsum([len(x) for x in names], dtype=np.int64)])
        bufs, self.n_targets, self.total_len, n = _depth_inputs(ctx, tlen, segs, len(names) + 1)
        self._keep = bufs[3:] + [ctx.upload(np.frombuffer(b"".join(names) or b"\0", dtype=np.uint8)), ctx.upload(name_off)]
        tb, ln, sm = C.c_uint64(_FILL64), C.c_uint64(_FILL64), C.c_uint64(_FILL64)
        try:
            _check(lib().palace_depth_text_create(ctx.h, n, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, self.n_targets, self._keep[0].ptr, self._keep[1].ptr,
                                                  self.total_len, self._keep[2].ptr, self._keep[3].ptr, C.byref(self.h), C.byref(tb), C.byref(ln),
                                                  C.byref(sm)), "palace_depth_text_create")
        except PalaceError:
            self.close()
            raise
        finally:
            for b in bufs[:3]:
                b.free()
        self.text_bytes, self.lines, self.sum = int(tb.value), int(ln.value), int(sm.value)

    def emit_many(self, ranges, guard: int = 64):
        """every [begin, end) of `ranges` through palace_depth_text_emit, each into a slot of its own of device buffers filled with
        0xA5, `guard` such bytes in front of and behind its end - begin bytes -> [(bytes, guards untouched)].  A refused range raises
        PalaceError; its `untouched` says whether every byte of the buffer is still as it was."""
        ranges = [(int(a), int(b)) for a, b in ranges]
        out, k = [], 0
        while k < len(ranges):
            slots, at = [], 0
            while k + len(slots) < len(ranges) and (not slots or at < (32 << 20)):
                a, b = ranges[k + len(slots)]
                slots.append(at + guard)
                at += guard + max(b - a, 0) + guard
            d_out = self.ctx.upload(np.full(max(at, 1), 0xA5, np.uint8))
            try:
                for (a, b), slot in zip(ranges[k:], slots):
                    rc = lib().palace_depth_text_emit(self.ctx.h, self.h, C.c_uint64(a & (2 ** 64 - 1)), C.c_uint64(b & (2 ** 64 - 1)), d_out.ptr + slot)
                    if rc != 0:
                        err = PalaceError(f"palace_depth_text_emit [{a}, {b}) -> {rc}: {lib().palace_last_error().decode()}")
                        self.ctx.sync()
                        err.untouched = bool((d_out.to_host() == 0xA5).all())
                        raise err
                self.ctx.sync()
                got = d_out.to_host()
            finally:
                d_out.free()
            ends = [s + max(b - a, 0) for (a, b), s in zip(ranges[k:], slots)]
            for s, e, nxt in zip(slots, ends, slots[1:] + [at + guard]):
                out.append((got[s:e].tobytes(), bool((got[s - guard:s] == 0xA5).all() and (got[e:nxt - guard] == 0xA5).all())))
            k += len(slots)
        return out

    def emit(self, begin: int, end: int, guard: int = 64):
        """bytes [begin, end) of the text -> (bytes, whether the `guard` bytes on both sides of them are untouched)"""
        return self.emit_many([(begin, end)], guard)[0]

    def windows(self, beg, end):
        """palace_depth_text_windows -> (text_beg[], text_end[], lines[]) of the ranges [beg[w], end[w]) of global positions"""
        wb, we = np.ascontiguousarray(beg, dtype=np.int64), np.ascontiguousarray(end, dtype=np.int64)
        assert wb.shape == we.shape and wb.ndim == 1
        n = len(wb)
        bufs = [self.ctx.upload(wb), self.ctx.upload(we)] + [self.ctx.upload(np.full(max(n, 1), _FILL64, np.uint64)) for _ in range(3)]
        try:
            _check(lib().palace_depth_text_windows(self.ctx.h, self.h, n, *(b.ptr for b in bufs)), "palace_depth_text_windows")
            self.ctx.sync()
            return tuple(b.to_host()[:n].copy() for b in bufs[2:])
        finally:
            for b in bufs:
                b.free()

    def close(self):
        if self.h:
            _check(lib().palace_depth_text_destroy(self.ctx.h, self.h), "palace_depth_text_destroy")
            self.h = C.c_void_p()
        for b in self._keep:
            b.free()
        self._keep = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def fastq_scratch_bytes(max_window: int) -> int:
    return int(lib().palace_fastq_scratch_bytes(max_window))


def crc32_members(ctx: Ctx, data: bytes, lengths) -> np.ndarray:
    """CRC-32 of consecutive members of `data` (lengths in bytes) computed on the device."""
    lens = np.asarray(lengths, dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)[:-1]]).astype(np.int64) if len(lens) else np.zeros(0, np.int64)
    d_data = ctx.upload(np.frombuffer(bytes(data), dtype=np.uint8) if len(data) else np.zeros(1, np.uint8))
    d_off, d_len, d_crc = ctx.upload(offs), ctx.upload(lens), ctx.empty(max(1, len(lens)), np.uint32)
    try:
        ctx.crc32_members(d_data.ptr, len(lens), d_off, d_len, d_crc)
        return d_crc.to_host()[:len(lens)]
    finally:
        for b in (d_data, d_off, d_len, d_crc):
            b.free()


def bgzf_deflate(ctx: Ctx, pieces, lead: int = 0, lz: bool = False):
    """One BGZF member per piece (bytes, at most 0xff00 each), written on the device: CRC-32, DEFLATE and the compaction to file bytes.
    -> (file bytes, member offsets with the total as last entry).  lead: bytes in front of the first piece (any alignment).
    lz: the hashed matcher (palace_bgzf_deflate_lz) in the place of the previous-line one."""
    lens = np.array([len(p) for p in pieces], dtype=np.int32)
    n = len(lens)
    offs = (lead + np.concatenate([[0], np.cumsum(lens, dtype=np.int64)[:-1]])).astype(np.int64) if n else np.zeros(0, np.int64)
    blob = bytes(lead) + b"".join(bytes(p) for p in pieces) + bytes(4)
    bufs = [ctx.upload(np.frombuffer(blob, dtype=np.uint8)), ctx.upload(offs if n else np.zeros(1, np.int64)),
            ctx.upload(lens if n else np.zeros(1, np.int32)), ctx.empty(max(1, n), np.uint32), ctx.empty(max(1, n) * 65536, np.uint8),
            ctx.empty(max(1, n), np.int32), ctx.empty(max(1, n) * 65536, np.uint8), ctx.empty(n + 1, np.int64)]
    d_text, d_off, d_len, d_crc, d_slots, d_mlen, d_file, d_moff = bufs
    try:
        ctx.crc32_members(d_text.ptr, n, d_off, d_len, d_crc)
        (ctx.bgzf_deflate_lz if lz else ctx.bgzf_deflate)(d_text.ptr, n, d_off, d_len, d_crc, d_slots, d_mlen)
        ctx.bgzf_compact(d_slots, n, d_mlen, d_file, d_moff)
        moff = d_moff.to_host()
        return d_file.to_host()[:int(moff[-1])].tobytes(), moff
    finally:
        for b in bufs:
            b.free()


BGZF_SLOT = 65536


def bgzf_deflate_slots(ctx: Ctx, blob: bytes, offs, lens, crcs, before: int = 1, after: int = 1, fill: int = 0xa5, lz: bool = False):
    """palace_bgzf_deflate (lz: palace_bgzf_deflate_lz) alone, on ranges and CRCs exactly as the caller states them (d_len as it is: nothing is clamped here), into
    slots pre-filled with `fill` with `before` / `after` spare slots around them.  blob: the text, 4 bytes of room behind it are added (the kernel reads whole dwords).
    -> (member_len int32[n], every slot as uint8[before + n + after, 65536]); the guard behind member_len must be intact."""
    lens, offs, crcs = np.ascontiguousarray(lens, np.int32), np.ascontiguousarray(offs, np.int64), np.ascontiguousarray(crcs, np.uint32)
    n = len(lens)
    assert n >= 1 and offs.shape == (n,) and crcs.shape == (n,)
    bufs = [ctx.upload(np.frombuffer(bytes(blob) + bytes(4), np.uint8)), ctx.upload(offs), ctx.upload(lens), ctx.upload(crcs),
            ctx.upload(np.full((before + n + after) * BGZF_SLOT, fill, np.uint8)), _guarded(ctx, n, np.int32)]
    d_text, d_off, d_len, d_crc, d_slots, d_mlen = bufs
    try:
        name = "palace_bgzf_deflate_lz" if lz else "palace_bgzf_deflate"
        _check(getattr(lib(), name)(ctx.h, d_text.ptr, n, d_off.ptr, d_len.ptr, d_crc.ptr, d_slots.ptr + before * BGZF_SLOT, d_mlen.ptr), name)
        ctx.sync()
        return _unguard(d_mlen, n, np.int32, "member lengths"), d_slots.to_host().reshape(before + n + after, BGZF_SLOT)
    finally:
        for b in bufs:
            b.free()


def bgzf_compact_slots(ctx: Ctx, d_slots: DevBuf, member_len, base: int = 0, fill: int = 0x5a, room: int = 64):
    """palace_bgzf_compact alone on slots the caller filled (d_slots: at least len(member_len) slots, raw bytes): d_file lies `base` bytes
    into a buffer of `fill` with `room` bytes behind the sum of the lengths.
    -> (member_off int64[n + 1], the whole buffer as uint8); the guard behind member_off must be intact."""
    member_len = np.ascontiguousarray(member_len, np.int32)
    n = len(member_len)
    total = int(member_len.astype(np.int64).sum())
    bufs = [ctx.upload(member_len if n else np.zeros(1, np.int32)), ctx.upload(np.full(base + total + room, fill, np.uint8)),
            _guarded(ctx, n + 1, np.int64)]
    d_mlen, d_file, d_moff = bufs
    try:
        _check(lib().palace_bgzf_compact(ctx.h, d_slots.ptr, n, d_mlen.ptr, d_file.ptr + base, d_moff.ptr), "palace_bgzf_compact")
        ctx.sync()
        return _unguard(d_moff, n + 1, np.int64, "member offsets"), d_file.to_host()
    finally:
        for b in bufs:
            b.free()


def bgzf_inflate_members(ctx: Ctx, members, sizes):
    """whole BGZF members (18-byte header, DEFLATE, 8-byte trailer) through palace_bgzf_inflate, member k stated as sizes[k] bytes of text
    -> (status int32[n], [bytes])"""
    blob, in_off, out_off, o = bytearray(), [], [], 0
    for m, k in zip(members, sizes):
        in_off.append(len(blob) + 18)
        blob += m
        out_off.append(o)
        o += k
    blob += bytes(8)
    n = len(members)
    bufs = [ctx.upload(np.frombuffer(bytes(blob), np.uint8)), ctx.upload(np.array(in_off, np.int64)),
            ctx.upload(np.array([len(m) - 26 for m in members], np.int32)), ctx.upload(np.array(out_off, np.int64)),
            ctx.upload(np.array(sizes, np.int32)), ctx.upload(np.zeros(o + 8, np.uint8)), ctx.upload(np.full(n, -1, np.int32))]
    try:
        _check(lib().palace_bgzf_inflate(ctx.h, bufs[0].ptr, n, *(b.ptr for b in bufs[1:])), "palace_bgzf_inflate")
        ctx.sync()
        st, out = bufs[6].to_host(), bufs[5].to_host().tobytes()
        return st, [out[a:a + k] for a, k in zip(out_off, sizes)]
    finally:
        for b in bufs:
            b.free()


def gzip_inflate(ctx: Ctx, blob: bytes, stride: int = 0, span: int = 0, text_cap: int = 0, check_guards: bool = False):
    """The text of the gzip file `blob` as palace_gzip_inflate hands it over, and the call's counters as a dict.  The text is None
    when the device path declined the file (counters["fallback"] != 0) or the sink did not see the file's last bytes."""
    blob = bytes(blob)
    parts, seen_last = [], []

    def take(_user, d_text, n, last):
        if n:
            part = np.empty(n, np.uint8)
            if lib().palace_d2h(ctx.h, part.ctypes.data, d_text, n):
                return 1
            parts.append(part.tobytes())
        if last:
            seen_last.append(True)
        return 0

    prm = GzipParams(stride, span, text_cap, int(check_guards))
    st = GzipStats()
    buf = np.frombuffer(blob, dtype=np.uint8) if blob else np.zeros(1, np.uint8)
    _check(lib().palace_gzip_inflate(ctx.h, buf.ctypes.data, len(blob), C.byref(prm), GZIP_SINK(take), None, C.byref(st)), "palace_gzip_inflate")
    stats = {k: getattr(st, k) for k, _ in GzipStats._fields_}
    text = b"".join(parts) if stats["fallback"] == 0 and seen_last else None
    return text, stats


def fastq_read_set(ctx: Ctx, text: bytes, cuts=(), reads0: int = 0, bases0: int = 0):
    """The sequence lines of FASTQ `text` as an ASCII read set made by palace_fastq_parse, the text handed over in windows cut at
    the ascending positions `cuts`.  Returns (bases uint8, offsets int64 of reads + 1 entries starting at bases0, final cursor);
    the first reads0 entries a real caller would have are not part of the result."""
    text = bytes(text)
    bounds = [0] + [c for c in cuts if 0 < c < len(text)] + [len(text)]
    widest = max(b - a for a, b in zip(bounds, bounds[1:])) if len(bounds) > 1 else 0
    bases_cap = bases0 + len(text) + 1
    offsets_cap = reads0 + len(text) // 4 + 3
    d_win = DevBuf(ctx, max(16, widest + 16))
    d_bases, d_offsets = DevBuf(ctx, bases_cap), ctx.empty(offsets_cap, np.int64)
    d_scratch = DevBuf(ctx, fastq_scratch_bytes(widest))
    cur = np.zeros(1, FASTQ_CURSOR_DTYPE)
    cur["reads"], cur["bases"] = reads0, bases0
    d_cur = ctx.upload(cur)
    try:
        first = np.zeros(1, np.int64)
        first[0] = bases0
        _check(lib().palace_h2d(ctx.h, d_offsets.ptr + 8 * reads0, first.ctypes.data, 8), "palace_h2d")
        for k, (a, b) in enumerate(zip(bounds, bounds[1:])):
            chunk = np.frombuffer(text[a:b], dtype=np.uint8)
            if len(chunk):
                _check(lib().palace_h2d(ctx.h, d_win.ptr, chunk.ctypes.data, len(chunk)), "palace_h2d")
            ctx.fastq_parse(d_win.ptr, len(chunk), k == len(bounds) - 2, d_cur, d_bases, bases_cap, d_offsets, offsets_cap, d_scratch)
            ctx.sync()
        cur = d_cur.to_host()[0]
        if cur["error"]:
            raise PalaceError("palace_fastq_parse: capacity exceeded")
        n_reads = int(cur["reads"]) - reads0
        offsets = d_offsets.to_host()[reads0:reads0 + n_reads + 1].copy()
        bases = d_bases.to_host()[bases0:int(cur["bases"])].copy()
        return bases, offsets, cur
    finally:
        for buf in (d_win, d_bases, d_offsets, d_scratch, d_cur):
            buf.free()


def bam_walk(ctx: Ctx, stream: bytes, first: int, n_ref: int, chunk: int = 0):
    """palace_bam_walk on the inflated stream `stream` -> (record starts int64, stop offset, stats dict); the count first, then the
    starts into a buffer of exactly that size, as the loader of `bamdepth --bam-gpu` does."""
    stream = bytes(stream)
    total = len(stream)
    nscr = int(lib().palace_bam_walk_scratch_bytes(total, first, chunk))
    d_stream = ctx.upload(np.frombuffer(stream, dtype=np.uint8) if total else np.zeros(1, np.uint8))
    d_scr = DevBuf(ctx, max(nscr, 8))
    n, stop, stats = C.c_int64(), C.c_int64(), (C.c_int64 * 4)()
    d_starts = None
    try:
        _check(lib().palace_bam_walk(ctx.h, d_stream.ptr, total, first, n_ref, chunk, d_scr.ptr, nscr, None, 0, C.byref(n), C.byref(stop), stats),
               "palace_bam_walk")
        d_starts = ctx.empty(max(1, n.value), np.int64)
        _check(lib().palace_bam_walk_starts(ctx.h, d_stream.ptr, total, first, chunk, d_scr.ptr, nscr, d_starts.ptr, n.value), "palace_bam_walk_starts")
        starts = d_starts.to_host()[:n.value].copy()
        return starts, int(stop.value), dict(zip(("chunks", "held", "repaired", "no_start"), (int(v) for v in stats)))
    finally:
        for b in (d_stream, d_scr, d_starts):
            if b is not None:
                b.free()


def bam_match_segments(ctx: Ctx, stream: bytes, starts, n_ref: int):
    """palace_bam_match_segments -> (tid, pos, len) int32 arrays: the count first, then the segments."""
    stream = bytes(stream)
    st = np.ascontiguousarray(starts, dtype=np.int64)
    d_stream = ctx.upload(np.frombuffer(stream, dtype=np.uint8) if stream else np.zeros(1, np.uint8))
    d_st = ctx.upload(st if len(st) else np.zeros(1, np.int64))
    n = C.c_int64()
    bufs = [d_stream, d_st]
    try:
        _check(lib().palace_bam_match_segments(ctx.h, d_stream.ptr, len(stream), d_st.ptr, len(st), n_ref, None, None, None, 0, C.byref(n)),
               "palace_bam_match_segments")
        want = n.value
        out = [ctx.empty(max(1, want), np.int32) for _ in range(3)]
        bufs += out
        _check(lib().palace_bam_match_segments(ctx.h, d_stream.ptr, len(stream), d_st.ptr, len(st), n_ref, out[0].ptr, out[1].ptr, out[2].ptr,
                                               want, C.byref(n)), "palace_bam_match_segments")
        assert n.value == want
        return tuple(b.to_host()[:want].copy() for b in out)
    finally:
        for b in bufs:
            b.free()


def sort_u64(ctx: Ctx, keys, key_bits: int):
    """palace_sort_u64 -> (the keys sorted by their low key_bits bits, the permutation: input ordinal of the key at each place)"""
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    n = len(k)
    nscr = int(lib().palace_sort_u64_scratch_bytes(n))
    bufs = [ctx.upload(k if n else np.zeros(1, np.uint64)), ctx.empty(max(1, n), np.uint32), DevBuf(ctx, max(nscr, 256))]
    try:
        _check(lib().palace_sort_u64(ctx.h, bufs[0].ptr, bufs[1].ptr, n, key_bits, bufs[2].ptr, nscr), "palace_sort_u64")
        return bufs[0].to_host()[:n].copy(), bufs[1].to_host()[:n].copy()
    finally:
        for b in bufs:
            b.free()


def bam_sort_keys(ctx: Ctx, stream: bytes, starts, n_ref: int):
    """palace_bam_sort_keys -> (keys uint64, records without a key, the first one's ordinal or -1)"""
    stream = bytes(stream)
    st = np.ascontiguousarray(starts, dtype=np.int64)
    bufs = [ctx.upload(np.frombuffer(stream, dtype=np.uint8) if stream else np.zeros(1, np.uint8)), ctx.upload(st if len(st) else np.zeros(1, np.int64)),
            ctx.empty(max(1, len(st)), np.uint64)]
    n_bad, first_bad = C.c_int64(), C.c_int64()
    try:
        _check(lib().palace_bam_sort_keys(ctx.h, bufs[0].ptr, len(stream), bufs[1].ptr, len(st), n_ref, bufs[2].ptr, C.byref(n_bad), C.byref(first_bad)),
               "palace_bam_sort_keys")
        return bufs[2].to_host()[:len(st)].copy(), int(n_bad.value), int(first_bad.value)
    finally:
        for b in bufs:
            b.free()


def bam_gather(ctx: Ctx, stream: bytes, starts, perm, head: bytes):
    """palace_bam_gather_plan and palace_bam_gather_write -> (output offsets int64 (n + 1), the sorted stream's record starts, the output
    stream with `head` in front and 0xAA where nothing may be written: 16 guard bytes behind it)"""
    stream = bytes(stream)
    st, pm = np.ascontiguousarray(starts, dtype=np.int64), np.ascontiguousarray(perm, dtype=np.uint32)
    n = len(st)
    bufs = [ctx.upload(np.frombuffer(stream, dtype=np.uint8) if stream else np.zeros(1, np.uint8)), ctx.upload(st if n else np.zeros(1, np.int64)),
            ctx.upload(pm if n else np.zeros(1, np.uint32)), ctx.empty(n + 1, np.int64), ctx.empty(max(1, n), np.int64)]
    total = C.c_int64()
    try:
        _check(lib().palace_bam_gather_plan(ctx.h, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, n, len(head), bufs[3].ptr, bufs[4].ptr, C.byref(total)),
               "palace_bam_gather_plan")
        image = np.full(total.value + 16, 0xAA, np.uint8)
        image[:len(head)] = np.frombuffer(head, dtype=np.uint8)
        d_out = ctx.upload(image)
        bufs.append(d_out)
        _check(lib().palace_bam_gather_write(ctx.h, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, n, total.value, d_out.ptr), "palace_bam_gather_write")
        return bufs[3].to_host().copy(), bufs[4].to_host()[:n].copy(), d_out.to_host().tobytes()
    finally:
        for b in bufs:
            b.free()


GUARD = b"\xaa" * 16     # behind the last entry of every output the index wrappers allocate; the fill of entries nothing may write


def untouched(arr) -> np.ndarray:
    """per entry of an array a wrapper below returned: every byte still holds the fill"""
    a = np.ascontiguousarray(arr)
    return (a.view(np.uint8).reshape(len(a), a.dtype.itemsize) == GUARD[0]).all(axis=1)


def _guarded(ctx: Ctx, n: int, dtype) -> DevBuf:
    """n entries of the fill and GUARD behind them, on the device"""
    return ctx.upload(np.full(n * np.dtype(dtype).itemsize + len(GUARD), GUARD[0], np.uint8))


def _unguard(buf: DevBuf, n: int, dtype, what: str) -> np.ndarray:
    """the n entries back on the host; the guard behind them must be intact"""
    raw = buf.to_host()
    size = n * np.dtype(dtype).itemsize
    assert raw[size:].tobytes() == GUARD, f"{what}: written behind its {n} entries"
    return raw[:size].view(dtype).copy()


def _stream_and_starts(ctx: Ctx, stream: bytes, starts):
    stream = bytes(stream)
    st = np.ascontiguousarray(starts, dtype=np.int64)
    return [ctx.upload(np.frombuffer(stream, dtype=np.uint8) if stream else np.zeros(1, np.uint8)), ctx.upload(st if len(st) else np.zeros(1, np.int64))], len(st)


def _column(ctx: Ctx, arr, dtype, n: int) -> DevBuf:
    a = np.ascontiguousarray(arr, dtype=dtype)
    assert a.shape == (n,), (a.shape, n)
    return ctx.upload(a if n else np.zeros(1, dtype))


def bai_records(ctx: Ctx, stream: bytes, starts, n_ref: int):
    """palace_bai_records -> (ref, bin, win_beg, win_end int32, unmapped uint8, (n_bad, first_bad, first_unsorted, n_no_coor))"""
    bufs, n = _stream_and_starts(ctx, stream, starts)
    kinds = (np.int32, np.int32, np.int32, np.int32, np.uint8)
    status = BaiStatus()
    try:
        out = [_guarded(ctx, n, t) for t in kinds]
        bufs += out
        _check(lib().palace_bai_records(ctx.h, bufs[0].ptr, bufs[1].ptr, n, n_ref, *(b.ptr for b in out), C.byref(status)), "palace_bai_records")
        cols = tuple(_unguard(b, n, t, "palace_bai_records") for b, t in zip(out, kinds))
        return cols + ((int(status.n_bad), int(status.first_bad), int(status.first_unsorted), int(status.n_no_coor)),)
    finally:
        for b in bufs:
            b.free()


def bai_chunks(ctx: Ctx, stream: bytes, starts, ref, bin, n_ref: int, cap: int | None = None):
    """palace_bai_chunks on columns of the caller's -> (n_runs, chunk_ref, chunk_bin int32, chunk_beg, chunk_end int64).  cap=None: the
    two calls of host/bai.hpp, the count and then the runs into arrays of exactly that size.  cap=0: the count alone, empty arrays.
    Any other cap goes through as it is: the arrays come back with all their cap entries, unwritten ones as untouched() knows them."""
    bufs, n = _stream_and_starts(ctx, stream, starts)
    kinds = (np.int32, np.int32, np.int64, np.int64)
    n_runs = C.c_int64(-1)
    try:
        bufs += [_column(ctx, ref, np.int32, n), _column(ctx, bin, np.int32, n)]
        ins = [b.ptr for b in bufs]
        if cap is None or cap == 0:
            _check(lib().palace_bai_chunks(ctx.h, *ins, n, n_ref, None, None, None, None, 0, C.byref(n_runs)), "palace_bai_chunks")
            if cap == 0:
                return (int(n_runs.value),) + tuple(np.zeros(0, t) for t in kinds)
            cap = int(n_runs.value)
        out = [_guarded(ctx, cap, t) for t in kinds]
        bufs += out
        again = C.c_int64(-1)
        _check(lib().palace_bai_chunks(ctx.h, *ins, n, n_ref, *(b.ptr for b in out), cap, C.byref(again)), "palace_bai_chunks")
        assert n_runs.value in (-1, again.value), "palace_bai_chunks: two counts of one stream differ"
        return (int(again.value),) + tuple(_unguard(b, cap, t, "palace_bai_chunks") for b, t in zip(out, kinds))
    finally:
        for b in bufs:
            b.free()


def bai_linear(ctx: Ctx, stream: bytes, starts, ref, win_beg, win_end, unmapped, n_ref: int):
    """palace_bai_linear, the two calls of host/bai.hpp -> (n_intv int32 (n_ref), ref_stat int64 (4, n_ref), lin_off int64 (n_ref + 1):
    the exclusive sums of n_intv made here, lin int64 (lin_off[-1]))"""
    bufs, n = _stream_and_starts(ctx, stream, starts)
    try:
        bufs += [_column(ctx, ref, np.int32, n), _column(ctx, win_beg, np.int32, n), _column(ctx, win_end, np.int32, n), _column(ctx, unmapped, np.uint8, n)]
        ins = [b.ptr for b in bufs]
        d_n_intv, d_stat = _guarded(ctx, n_ref, np.int32), _guarded(ctx, 4 * n_ref, np.int64)
        bufs += [d_n_intv, d_stat]
        _check(lib().palace_bai_linear(ctx.h, *ins, n, n_ref, d_n_intv.ptr, d_stat.ptr, None, 0, None), "palace_bai_linear")
        n_intv = _unguard(d_n_intv, n_ref, np.int32, "palace_bai_linear: n_intv")
        stat = _unguard(d_stat, 4 * n_ref, np.int64, "palace_bai_linear: ref_stat")
        lin_off = np.concatenate(([0], np.cumsum(n_intv, dtype=np.int64))).astype(np.int64)
        n_lin = int(lin_off[-1])
        d_lin_off, d_lin = ctx.upload(lin_off), _guarded(ctx, n_lin, np.int64)
        bufs += [d_lin_off, d_lin]
        _check(lib().palace_bai_linear(ctx.h, *ins, n, n_ref, d_n_intv.ptr, d_stat.ptr, d_lin_off.ptr, n_lin, d_lin.ptr), "palace_bai_linear")
        lin = _unguard(d_lin, n_lin, np.int64, "palace_bai_linear: lin")
        assert np.array_equal(_unguard(d_n_intv, n_ref, np.int32, "palace_bai_linear: n_intv"), n_intv), "the second call changed n_intv"
        assert np.array_equal(_unguard(d_stat, 4 * n_ref, np.int64, "palace_bai_linear: ref_stat"), stat), "the second call changed ref_stat"
        return n_intv, stat.reshape(4, n_ref), lin_off, lin
    finally:
        for b in bufs:
            b.free()


def bgzf_voffsets(ctx: Ctx, u, member_u, member_c) -> np.ndarray:
    """palace_bgzf_voffsets -> uint64 virtual offsets, one per entry of u"""
    u, mu, mc = (np.ascontiguousarray(a, dtype=np.int64) for a in (u, member_u, member_c))
    assert len(mu) == len(mc)
    bufs = [ctx.upload(a if len(a) else np.zeros(1, np.int64)) for a in (u, mu, mc)]
    try:
        d_v = _guarded(ctx, len(u), np.uint64)
        bufs.append(d_v)
        _check(lib().palace_bgzf_voffsets(ctx.h, bufs[0].ptr, len(u), bufs[1].ptr, bufs[2].ptr, len(mu), d_v.ptr), "palace_bgzf_voffsets")
        return _unguard(d_v, len(u), np.uint64, "palace_bgzf_voffsets")
    finally:
        for b in bufs:
            b.free()


SAM_TILE = 4096          # PALACE_SAM_TILE of include/palace_hip.h


def sam_lines(ctx: Ctx, text: bytes):
    """palace_sam_lines, the count and then the starts -> (line starts int64 (lines + 1), header lines, alignment lines,
    the first faulty line's number or 0, its PALACE_SAM_E* code or 0)"""
    text = bytes(text)
    n = len(text)
    nscr = int(lib().palace_sam_scratch_bytes(n))
    bufs = [ctx.upload(np.frombuffer(text, dtype=np.uint8) if n else np.zeros(1, np.uint8)), ctx.empty(nscr, np.uint8)]
    out = (C.c_int64 * 5)()
    try:
        _check(lib().palace_sam_lines(ctx.h, bufs[0].ptr, n, bufs[1].ptr, nscr, None, 0, out), "palace_sam_lines")
        n_lines = int(out[0])
        assert list(out)[1:] == [-1] * 4
        bufs.append(ctx.empty(n_lines + 1, np.int64))
        _check(lib().palace_sam_lines(ctx.h, bufs[0].ptr, n, bufs[1].ptr, nscr, bufs[2].ptr, n_lines + 1, out), "palace_sam_lines")
        assert int(out[0]) == n_lines
        return bufs[2].to_host()[:n_lines + 1].copy(), int(out[1]), int(out[2]), int(out[3]), int(out[4])
    finally:
        for b in bufs:
            b.free()


def _sam_run(ctx: Ctx, text: bytes, starts, n_header: int, names, mask: int, head: bytes, encode: bool, guard: int = 16):
    text = bytes(text)
    st = np.ascontiguousarray(starts, dtype=np.int64)
    n = len(st) - 1 - n_header
    blob = b"".join(names)
    off = np.zeros(len(names) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in names])
    bufs = [ctx.upload(np.frombuffer(text, dtype=np.uint8) if text else np.zeros(1, np.uint8)), ctx.upload(st[n_header:]),
            ctx.upload(np.frombuffer(blob, dtype=np.uint8) if blob else np.zeros(1, np.uint8)), ctx.upload(off),
            ctx.empty(max(1, n), np.int32), ctx.empty(n + 1, np.int64), ctx.empty(max(1, n), np.int32)]
    d_text, d_st, d_blob, d_off, d_size, d_out_off, d_ord = bufs
    table = C.c_void_p()
    out = (C.c_int64 * 5)()
    try:
        _check(lib().palace_bam_names_create(ctx.h, d_blob.ptr, d_off.ptr, len(names), C.byref(table)), "palace_bam_names_create")
        _check(lib().palace_sam_plan(ctx.h, d_text.ptr, d_st.ptr, n, n_header + 1, table, mask, len(head), d_size.ptr, d_out_off.ptr, d_ord.ptr, out),
               "palace_sam_plan")
        res = {"size": d_size.to_host()[:n].copy(), "off": d_out_off.to_host()[:n + 1].copy(), "ord": d_ord.to_host()[:n].copy(), "kept": int(out[0]),
               "dropped": int(out[1]), "bytes": int(out[2]), "err_line": int(out[3]), "err_code": int(out[4])}
        if not encode or res["err_code"]:
            return res
        image = np.full(res["bytes"] + guard, 0xAA, np.uint8)
        image[:len(head)] = np.frombuffer(head, dtype=np.uint8)
        d_image = ctx.upload(image)
        d_starts = ctx.empty(max(1, res["kept"]), np.int64)
        bufs += [d_image, d_starts]
        _check(lib().palace_sam_encode(ctx.h, d_text.ptr, d_st.ptr, n, table, d_size.ptr, d_out_off.ptr, d_ord.ptr, d_image.ptr, d_starts.ptr), "palace_sam_encode")
        ctx.sync()
        res["stream"] = d_image.to_host().tobytes()
        res["starts"] = d_starts.to_host()[:res["kept"]].copy()
        return res
    finally:
        if table:
            lib().palace_bam_names_destroy(ctx.h, table)
        for b in bufs:
            b.free()


def sam_plan(ctx: Ctx, text: bytes, starts, n_header: int, names, mask: int, head_bytes: int):
    """palace_sam_plan over the alignment lines of `text` (starts / n_header as sam_lines left them; names = the header's targets, bytes,
    in order) -> dict: size int32, off int64 (n + 1), ord int32, kept, dropped, bytes, err_line, err_code"""
    return _sam_run(ctx, text, starts, n_header, names, mask, b"\0" * head_bytes, False)


def sam_encode(ctx: Ctx, text: bytes, starts, n_header: int, names, mask: int, head: bytes, guard: int = 16):
    """palace_sam_plan and palace_sam_encode -> the plan's dict and, for a text without error, stream: `head`, the records, and `guard`
    bytes of 0xAA where nothing may be written; starts: the kept records' starts int64"""
    return _sam_run(ctx, text, starts, n_header, names, mask, head, True, guard)


class Readqc:
    """Two FASTQ texts on the device with their line starts (palace_sam_lines), and the calls of readqc over them:
    records() -> per text (records, bad line, code, seq_len int32); plan(prm) -> dict of len1, len2 int32, off1, off2 int64 (pairs + 1) and
    the READQC_OUT numbers; write(which, lo, hi, guard) -> guard bytes of 0xAA, the window's bytes, guard bytes of 0xAA; the report's
    plan_ex, insert_sizes and cycle_stats."""

    def __init__(self, ctx: Ctx, text1: bytes, text2: bytes):
        self.ctx, self.bufs, self.text, self.starts, self.n_lines = ctx, [], [], [], []
        self.d_len = self.d_off = self.d_cand = None
        for text in (bytes(text1), bytes(text2)):
            n = len(text)
            nscr = int(lib().palace_sam_scratch_bytes(n))
            d_text, d_scr = ctx.upload(np.frombuffer(text, dtype=np.uint8) if n else np.zeros(16, np.uint8)), ctx.empty(max(nscr, 1), np.uint8)
            self.bufs += [d_text, d_scr]
            out = (C.c_int64 * 5)()
            _check(lib().palace_sam_lines(ctx.h, d_text.ptr, n, d_scr.ptr, nscr, None, 0, out), "palace_sam_lines")
            n_lines = int(out[0])
            d_st = ctx.empty(n_lines + 1, np.int64)
            self.bufs.append(d_st)
            _check(lib().palace_sam_lines(ctx.h, d_text.ptr, n, d_scr.ptr, nscr, d_st.ptr, n_lines + 1, out), "palace_sam_lines")
            self.text.append(d_text); self.starts.append(d_st); self.n_lines.append(n_lines)

    def records(self):
        res = []
        for d_text, d_st, n_lines in zip(self.text, self.starts, self.n_lines):
            d_len = self.ctx.empty(max(1, n_lines // 4), np.int32)
            out = (C.c_int64 * 3)()
            try:
                _check(lib().palace_fastq_records(self.ctx.h, d_text.ptr, d_st.ptr, n_lines, d_len.ptr, out), "palace_fastq_records")
                res.append((int(out[0]), int(out[1]), int(out[2]), d_len.to_host()[:n_lines // 4].copy()))
            finally:
                d_len.free()
        return res

    def plan(self, prm: "ReadqcParams | None" = None):
        n = self.n_lines[0] // 4
        assert self.n_lines[1] // 4 == n
        prm = prm or ReadqcParams.default()
        if self.d_len is None:
            self.d_len = [self.ctx.empty(max(1, n), np.int32) for _ in range(2)]
            self.d_off = [self.ctx.empty(n + 1, np.int64) for _ in range(2)]
            self.bufs += self.d_len + self.d_off
        out = (C.c_int64 * len(READQC_OUT))()
        _check(lib().palace_readqc_plan(self.ctx.h, self.text[0].ptr, self.starts[0].ptr, self.text[1].ptr, self.starts[1].ptr, n, C.byref(prm),
                                        self.d_len[0].ptr, self.d_len[1].ptr, self.d_off[0].ptr, self.d_off[1].ptr, out), "palace_readqc_plan")
        res = {k: int(v) for k, v in zip(READQC_OUT, out)}
        res.update(len1=self.d_len[0].to_host()[:n].copy(), len2=self.d_len[1].to_host()[:n].copy(), off1=self.d_off[0].to_host()[:n + 1].copy(),
                   off2=self.d_off[1].to_host()[:n + 1].copy())
        return res

    def plan_ex(self, prm: "ReadqcParams | None" = None, with_cand: bool = True):
        """palace_readqc_plan_ex -> plan()'s dict and, with_cand, cand int32 (the array stays on the device for insert_sizes); without it
        the call is made with NULL"""
        n = self.n_lines[0] // 4
        assert self.n_lines[1] // 4 == n
        prm = prm or ReadqcParams.default()
        if self.d_len is None:
            self.d_len = [self.ctx.empty(max(1, n), np.int32) for _ in range(2)]
            self.d_off = [self.ctx.empty(n + 1, np.int64) for _ in range(2)]
            self.bufs += self.d_len + self.d_off
        if with_cand and self.d_cand is None:
            self.d_cand = self.ctx.upload(np.full(max(1, n), -7, np.int32))     # (an entry the call leaves is seen)
            self.bufs.append(self.d_cand)
        out = (C.c_int64 * len(READQC_OUT))()
        _check(lib().palace_readqc_plan_ex(self.ctx.h, self.text[0].ptr, self.starts[0].ptr, self.text[1].ptr, self.starts[1].ptr, n, C.byref(prm),
                                           self.d_len[0].ptr, self.d_len[1].ptr, self.d_off[0].ptr, self.d_off[1].ptr, self.d_cand.ptr if with_cand else None, out),
               "palace_readqc_plan_ex")
        res = {k: int(v) for k, v in zip(READQC_OUT, out)}
        res.update(len1=self.d_len[0].to_host()[:n].copy(), len2=self.d_len[1].to_host()[:n].copy(), off1=self.d_off[0].to_host()[:n + 1].copy(),
                   off2=self.d_off[1].to_host()[:n + 1].copy())
        if with_cand:
            res["cand"] = self.d_cand.to_host()[:n].copy()
        return res

    def insert_sizes(self, prm: "ReadqcParams | None" = None, cand=None):
        """palace_readqc_insert_sizes over plan_ex's candidates (or `cand`, int32 per pair) -> uint64[513]"""
        n = self.n_lines[0] // 4
        prm = prm or ReadqcParams.default()
        d_cand = self.ctx.upload(np.ascontiguousarray(cand, dtype=np.int32)) if cand is not None and n else self.d_cand
        d_hist = self.ctx.upload(np.full(READQC_ISIZE_MAX + 1, 0xAAAA, np.uint64))       # (the call sets, it does not add)
        try:
            assert n == 0 or d_cand is not None
            _check(lib().palace_readqc_insert_sizes(self.ctx.h, self.starts[0].ptr, self.starts[1].ptr, d_cand.ptr if n else None, n, C.byref(prm), d_hist.ptr),
                   "palace_readqc_insert_sizes")
            self.ctx.sync()
            return d_hist.to_host().copy()
        finally:
            d_hist.free()
            if cand is not None and n:
                d_cand.free()

    def cycle_stats(self, which: int, max_cycles: int, after: bool = True, lens=None, guard: int = 8):
        """palace_readqc_cycle_stats of text `which` -> [before, after] (or [before] where `after` is off: d_len NULL), each a dict of
        cnt, qsum uint64 (max_cycles, 5), q20, q30; `after` takes `lens` (int32 per record) or the kept lengths plan() / plan_ex() left.
        Behind the sections lie `guard` words that the call must leave alone."""
        n = self.n_lines[which] // 4
        words = 10 * max_cycles + 2
        n_sec = 2 if after else 1
        d_len = None
        if after:
            d_len = self.ctx.upload(np.ascontiguousarray(lens, dtype=np.int32)) if lens is not None else self.d_len[which]
        d_out = self.ctx.upload(np.full(n_sec * words + guard, 0xAAAA, np.uint64))
        try:
            _check(lib().palace_readqc_cycle_stats(self.ctx.h, self.text[which].ptr if n else None, self.starts[which].ptr if n else None, n,
                                                   d_len.ptr if after else None, max_cycles, d_out.ptr), "palace_readqc_cycle_stats")
            self.ctx.sync()
            got = d_out.to_host().copy()
        finally:
            d_out.free()
            if after and lens is not None:
                d_len.free()
        assert np.all(got[n_sec * words:] == 0xAAAA), "palace_readqc_cycle_stats wrote behind its sections"
        res = []
        for s in range(n_sec):
            sec = got[s * words:(s + 1) * words]
            res.append({"cnt": sec[:5 * max_cycles].reshape(max_cycles, 5), "qsum": sec[5 * max_cycles:10 * max_cycles].reshape(max_cycles, 5),
                        "q20": int(sec[-2]), "q30": int(sec[-1])})
        return res

    def write(self, which: int, lo: int, hi: int, guard: int = 32) -> bytes:
        assert guard % 16 == 0 and self.d_len is not None
        image = self.ctx.upload(np.full(2 * guard + max(hi - lo, 0), 0xAA, np.uint8))
        try:
            _check(lib().palace_readqc_write(self.ctx.h, self.text[which].ptr, self.starts[which].ptr, self.d_len[which].ptr, self.d_off[which].ptr,
                                             self.n_lines[which] // 4, lo, hi, image.ptr + guard), "palace_readqc_write")
            self.ctx.sync()
            return image.to_host().tobytes()
        finally:
            image.free()

    def close(self):
        for b in self.bufs:
            b.free()
        self.bufs = []


BAM_COLUMNS = (("tid", np.int32), ("pos", np.int32), ("mtid", np.int32), ("mpos", np.int32), ("nm", np.int32), ("ref_len", np.int32),
               ("read_len", np.int32), ("clip_s", np.int32), ("clip_e", np.int32), ("flag", np.uint16), ("mapq", np.uint8), ("qkey", np.uint64))


def bam_decode(ctx: Ctx, stream: bytes, starts, names, key_seed: int = 1):
    """palace_bam_columns and palace_bam_sa_items on the inflated stream -> (dict of column arrays incl. sa_off, SA items as
    SA_ITEM_DTYPE); `names` = the header's contig names (bytes), in tid order.  The items are counted first, then written."""
    stream = bytes(stream)
    st = np.ascontiguousarray(starts, dtype=np.int64)
    n = len(st)
    blob = b"".join(names)
    off = np.zeros(len(names) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in names])
    bufs = [ctx.upload(np.frombuffer(stream, dtype=np.uint8) if stream else np.zeros(1, np.uint8)), ctx.upload(st if n else np.zeros(1, np.int64)),
            ctx.upload(np.frombuffer(blob, dtype=np.uint8) if blob else np.zeros(1, np.uint8)), ctx.upload(off)]
    d_stream, d_st, d_blob, d_off = bufs
    table = C.c_void_p()
    try:
        col = {k: ctx.empty(max(1, n), dt) for k, dt in BAM_COLUMNS}
        col["sa_off"] = ctx.empty(n + 1, np.int32)
        bufs += list(col.values())
        cols = BamCols(n, **{k: b.ptr for k, b in col.items()})
        _check(lib().palace_bam_columns(ctx.h, d_stream.ptr, len(stream), d_st.ptr, n, key_seed, C.byref(cols)), "palace_bam_columns")
        _check(lib().palace_bam_names_create(ctx.h, d_blob.ptr, d_off.ptr, len(names), C.byref(table)), "palace_bam_names_create")
        cnt = C.c_int64()
        _check(lib().palace_bam_sa_items(ctx.h, d_stream.ptr, len(stream), d_st.ptr, n, table, None, None, 0, C.byref(cnt)), "palace_bam_sa_items")
        want = cnt.value
        d_items = ctx.empty(max(1, want), SA_ITEM_DTYPE)
        bufs.append(d_items)
        _check(lib().palace_bam_sa_items(ctx.h, d_stream.ptr, len(stream), d_st.ptr, n, table, col["sa_off"].ptr, d_items.ptr, want, C.byref(cnt)),
               "palace_bam_sa_items")
        assert cnt.value == want
        out = {k: b.to_host()[:n + 1 if k == "sa_off" else n].copy() for k, b in col.items()}
        return out, d_items.to_host()[:want].copy()
    finally:
        if table:
            lib().palace_bam_names_destroy(ctx.h, table)
        for b in bufs:
            b.free()


def bam_name_keys(ctx: Ctx, stream: bytes, starts, key_seed: int):
    """palace_bam_name_keys -> uint64 key per record"""
    stream = bytes(stream)
    st = np.ascontiguousarray(starts, dtype=np.int64)
    bufs = [ctx.upload(np.frombuffer(stream, dtype=np.uint8)), ctx.upload(st), ctx.empty(max(1, len(st)), np.uint64)]
    try:
        _check(lib().palace_bam_name_keys(ctx.h, bufs[0].ptr, len(stream), bufs[1].ptr, len(st), key_seed, bufs[2].ptr), "palace_bam_name_keys")
        return bufs[2].to_host()[:len(st)].copy()
    finally:
        for b in bufs:
            b.free()


def bam_names_differ(ctx: Ctx, stream: bytes, starts, pairs) -> int:
    """palace_bam_names_differ: how many of the (ordinal, ordinal) pairs have different read names"""
    stream = bytes(stream)
    st = np.ascontiguousarray(starts, dtype=np.int64)
    pr = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
    bufs = [ctx.upload(np.frombuffer(stream, dtype=np.uint8)), ctx.upload(st), ctx.upload(pr if len(pr) else np.zeros((1, 2), np.int64))]
    n = C.c_int64()
    try:
        _check(lib().palace_bam_names_differ(ctx.h, bufs[0].ptr, len(stream), bufs[1].ptr, len(st), bufs[2].ptr, len(pr), C.byref(n)),
               "palace_bam_names_differ")
        return int(n.value)
    finally:
        for b in bufs:
            b.free()


_ARC_BUFFERS = {}


def match_arcs_from_edges(cn: np.ndarray, edges: np.ndarray, min_count: int = 5, reuse: bool = False):
    """palace_match_arcs_from_edges (host code of the library) -> (copies, src, dst, weight); `edges` is an
    EDGE_DTYPE array as palace_graph_resolve writes it.  reuse=True hands out the same output arrays on every call
    of this size (valid until the next call) instead of fresh ones."""
    cn = np.ascontiguousarray(cn, dtype=np.int32)
    e = np.ascontiguousarray(edges, dtype=EDGE_DTYPE)
    key = (len(cn), len(e))
    if reuse and key in _ARC_BUFFERS:
        copies, src, dst, w = _ARC_BUFFERS[key]
    else:
        copies = np.empty(len(cn), np.int64)
        src = np.empty(2 * len(e), np.int32); dst = np.empty(2 * len(e), np.int32); w = np.empty(2 * len(e), np.int64)
        if reuse:
            _ARC_BUFFERS.clear()
            _ARC_BUFFERS[key] = (copies, src, dst, w)
    n = C.c_int64()
    _check(lib().palace_match_arcs_from_edges(cn.ctypes.data, len(cn), e.ctypes.data, len(e), min_count, copies.ctypes.data,
                                              src.ctypes.data, dst.ctypes.data, w.ctypes.data, C.byref(n)),
           "palace_match_arcs_from_edges")
    return copies, src[:n.value], dst[:n.value], w[:n.value]


class MatchResult:
    """Views into a palace_match_result (no copies); call free() -- or use as a context manager -- when done."""

    def __init__(self, handle):
        L = lib()
        self._h = handle
        n = self.n = L.palace_match_result_count(handle)
        self.off = np.ctypeslib.as_array(L.palace_match_result_offsets(handle), shape=(n + 1,))
        nv = int(self.off[-1])
        self.verts = np.ctypeslib.as_array(L.palace_match_result_verts(handle), shape=(max(nv, 1),))[:nv]
        mk = lambda f, dt: (np.ctypeslib.as_array(f(handle), shape=(max(n, 1),))[:n] if n else np.zeros(0, dt))
        self.kind = mk(L.palace_match_result_kind, np.uint8)
        self.iter = mk(L.palace_match_result_iter, np.int32)
        self.open_at = mk(L.palace_match_result_open_at, np.int32)

    def free(self):
        if self._h is not None:
            self.off = self.verts = self.kind = self.iter = self.open_at = None
            lib().palace_match_result_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def match_decompose_views(ctx: "Ctx", copies: np.ndarray, src: np.ndarray, dst: np.ndarray, iterations: int = 10,
                          aggressive: bool = False, compact: bool = False) -> MatchResult:
    cp = np.ascontiguousarray(copies, dtype=np.int64)
    s = np.ascontiguousarray(src, dtype=np.int32)
    d = np.ascontiguousarray(dst, dtype=np.int32)
    res = C.c_void_p()
    _check(lib().palace_match_decompose_ex(ctx.h, len(cp), cp.ctypes.data, len(s), s.ctypes.data, d.ctypes.data,
                                           iterations, int(aggressive), int(compact), C.byref(res)), "palace_match_decompose")
    r = MatchResult(res)
    if compact:
        r.n_bare = int(lib().palace_match_result_bare_count(res))
        words = (len(cp) + 63) // 64
        r.bare = np.ctypeslib.as_array(lib().palace_match_result_bare(res), shape=(max(1, words),))[:words]
    return r


def match_decompose(ctx: "Ctx", copies: np.ndarray, src: np.ndarray, dst: np.ndarray, iterations: int = 10,
                    aggressive: bool = False):
    """palace_match_decompose -> (offsets, verts, kind, iter, open_at) as numpy copies."""
    with match_decompose_views(ctx, copies, src, dst, iterations, aggressive) as r:
        return r.off.copy(), r.verts.copy(), r.kind.copy(), r.iter.copy(), r.open_at.copy()


MATCH_KEYS_POSITION, MATCH_KEYS_TWO_WORDS, MATCH_KEYS_ONE_WORD = 0, 1, 2      # palace_match_last_run, info[0]


def match_last_run(ctx: "Ctx") -> dict:
    """palace_match_last_run -> {key_mode, checked_rerun, rounds, iterations} of the last decomposition of this context"""
    info = (C.c_int64 * 4)()
    _check(lib().palace_match_last_run(ctx.h, info), "palace_match_last_run")
    return dict(key_mode=int(info[0]), checked_rerun=bool(info[1]), rounds=int(info[2]), iterations=int(info[3]))


def match_greedy(ctx: "Ctx", n_vertices: int, src, dst, alive=None):
    """palace_match_greedy for arcs given in rank order (arc id = position) -> (next, prev, next_arc, rounds); the two CSR
    lists of arc ids per tail and per head are built here (a stable sort keeps each list ascending in arc id)."""
    s = np.ascontiguousarray(src, dtype=np.int32)
    d = np.ascontiguousarray(dst, dtype=np.int32)
    al = np.ones(n_vertices, np.uint8) if alive is None else np.ascontiguousarray(alive, dtype=np.uint8)
    assert len(s) == len(d) and len(al) == n_vertices
    assert not len(s) or (0 <= min(s.min(), d.min()) and max(s.max(), d.max()) < n_vertices)

    def csr(ends):
        off = np.zeros(n_vertices + 1, np.int64)
        np.cumsum(np.bincount(ends, minlength=n_vertices), out=off[1:])
        return off, np.argsort(ends, kind="stable").astype(np.int32)

    (out_off, out_arcs), (in_off, in_arcs) = csr(s), csr(d)
    bufs = [ctx.upload(a) for a in (s, d, out_off, out_arcs, in_off, in_arcs, al)]
    outs = [ctx.empty(max(1, n_vertices), np.int32) for _ in range(3)]
    rounds = C.c_int32()
    try:
        _check(lib().palace_match_greedy(ctx.h, n_vertices, len(s), *(b.ptr for b in bufs), *(o.ptr for o in outs), C.byref(rounds)),
               "palace_match_greedy")
        nxt, prv, arc = (o.to_host()[:n_vertices] for o in outs)
    finally:
        for b in bufs + outs:
            b.free()
    return nxt, prv, arc, rounds.value


class Stage04:
    """The resident stage-04 object (palace_stage04_*): filter_graph.py's selection + matching on the device."""
    COUNT_NAMES = ("edges", "juncs", "kept_pass2", "kept_pass3_more", "segs_selected", "segs_rescued", "arcs", "segs_filtered")

    def __init__(self, ctx: "Ctx", seed, tlen, rank, name_len, path_off, path_tok, min_count: int = 5):
        self.ctx = ctx
        self._keep = [np.ascontiguousarray(seed, np.uint8), np.ascontiguousarray(tlen, np.int32), np.ascontiguousarray(rank, np.int32),
                      np.ascontiguousarray(name_len, np.int32), np.ascontiguousarray(path_off, np.int64),
                      np.ascontiguousarray(path_tok, np.int32)]
        sd, tl, rk, nl, po, pt = self._keep
        assert len(sd) == len(tl) == len(rk) == len(nl) and len(po) >= 1
        inp = Stage04Inputs(len(sd), min_count, sd.ctypes.data, tl.ctypes.data, rk.ctypes.data, nl.ctypes.data, len(po) - 1,
                            po.ctypes.data, pt.ctypes.data if len(pt) else None)
        h = C.c_void_p()
        _check(lib().palace_stage04_create(ctx.h, C.byref(inp), C.byref(h)), "palace_stage04_create")
        self.h, self.n_segs = h, len(sd)

    def filter(self, d_edges_ptr: int, d_n_edges_ptr: int, edge_bound: int):
        _check(lib().palace_stage04_filter(self.ctx.h, self.h, d_edges_ptr, d_n_edges_ptr, edge_bound), "palace_stage04_filter")

    def counts(self) -> dict:
        out = (C.c_int64 * 8)()
        _check(lib().palace_stage04_counts(self.ctx.h, self.h, out), "palace_stage04_counts")
        return dict(zip(self.COUNT_NAMES, (int(v) for v in out)))

    def flags(self, n_edges: int):
        seg = np.zeros(self.n_segs, np.uint8)
        edge = np.zeros(n_edges, np.uint8)
        _check(lib().palace_stage04_flags(self.ctx.h, self.h, seg.ctypes.data, edge.ctypes.data if n_edges else None, n_edges),
               "palace_stage04_flags")
        return seg, edge

    def match(self, d_edges_ptr: int, d_cn_ptr: int, iterations: int = 10, aggressive: bool = False, use_paths: bool = True):
        _check(lib().palace_stage04_match(self.ctx.h, self.h, d_edges_ptr, d_cn_ptr, iterations, int(aggressive), int(use_paths)), "palace_stage04_match")

    def result(self):
        """-> (MatchResult view with .bare / .n_bare, contig_of array view); valid until the next match() / close()"""
        res, cof, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        _check(lib().palace_stage04_result(self.ctx.h, self.h, C.byref(res), C.byref(cof), C.byref(n)), "palace_stage04_result")
        r = MatchResult(res)
        r.n_bare = int(lib().palace_match_result_bare_count(res))
        words = (n.value + 63) // 64
        r.bare = np.ctypeslib.as_array(lib().palace_match_result_bare(res), shape=(max(1, words),))[:words]
        contig_of = np.ctypeslib.as_array(C.cast(cof, C.POINTER(C.c_int32)), shape=(max(1, n.value),))[: n.value]
        return r, contig_of

    def close(self):
        if self.h:
            lib().palace_stage04_destroy(self.ctx.h, self.h)
            self.h = None


def window_minimums(hit_ratio: float, perfect_ratio: float):
    """int(500 * float32(ratio)) -- the expression of extract_ref.cpp:513-514."""
    w = np.float32(500)
    return int(w * np.float32(hit_ratio)), int(w * np.float32(perfect_ratio))


def fasta_index(ctx: Ctx, text: bytes, recs_cap: int | None = None):
    """FASTA text through palace_fasta_index: (status, records as FASTA_REC_DTYPE or None when they did not fit recs_cap, the text
    on the device, the records on the device).  recs_cap None: asked for first (a call with room for no record), then given."""
    a = np.frombuffer(text, dtype=np.uint8)
    d_text = ctx.upload(a)
    d_scratch = DevBuf(ctx, max(int(lib().palace_fasta_index_scratch_bytes(len(a))), 1))
    st = FastaStatus()
    if recs_cap is None:
        _check(lib().palace_fasta_index(ctx.h, d_text.ptr, len(a), None, 0, d_scratch.ptr, d_scratch.nbytes, C.byref(st)), "palace_fasta_index")
        recs_cap = int(st.n_records)
    d_recs = ctx.empty((max(recs_cap, 1),), FASTA_REC_DTYPE)
    _check(lib().palace_fasta_index(ctx.h, d_text.ptr, len(a), d_recs.ptr, recs_cap, d_scratch.ptr, d_scratch.nbytes, C.byref(st)), "palace_fasta_index")
    d_scratch.free()
    recs = d_recs.to_host()[:int(st.n_records)] if int(st.n_records) <= recs_cap else None
    return st, recs, d_text, d_recs


def fasta_index_at(ctx: Ctx, text_ptr: int, n: int, recs_ptr, recs_cap: int, scratch_ptr: int, scratch_bytes: int) -> FastaStatus:
    """palace_fasta_index on device pointers of the caller's; recs_ptr None with recs_cap 0 asks for the number of records"""
    st = FastaStatus()
    _check(lib().palace_fasta_index(ctx.h, text_ptr, n, recs_ptr, recs_cap, scratch_ptr, scratch_bytes, C.byref(st)), "palace_fasta_index")
    return st


def contig_features_enqueue(ctx: Ctx, text_ptr: int, n: int, recs_ptr: int, r0: int, r1: int, feat_ptr: int, fsum_ptr: int, info_ptr, bad_ptr: int,
                            scratch_ptr: int, scratch_bytes: int):
    """palace_contig_features on device pointers of the caller's (a torch tensor's data_ptr() is one); enqueues only"""
    _check(lib().palace_contig_features(ctx.h, text_ptr, n, recs_ptr, r0, r1, feat_ptr, fsum_ptr, info_ptr, bad_ptr, scratch_ptr, scratch_bytes),
           "palace_contig_features")


def contig_features(ctx: Ctx, text: bytes, r0: int = 0, r1: int | None = None, guard_rows: int = 1, repeat: int = 1):
    """FASTA text through palace_fasta_index and palace_contig_features for records [r0, r1): (index status, records, feat
    [r1 - r0, 12288] float32, fsum [r1 - r0, 64] float32, info as CONTIG_INFO_DTYPE, bad).  The rows lie between guard_rows rows of
    0xA5 bytes on either side, which must come back as they went in.  repeat: the call is made that often into the same buffers."""
    st, recs, d_text, d_recs = fasta_index(ctx, text)
    if st.error:
        return st, recs, None, None, None, None
    n_rec = int(st.n_records)
    r1 = n_rec if r1 is None else r1
    rows = r1 - r0
    outs = []
    for width, dtype in ((CONTIG_FEATURES, np.float32), (CONTIG_FSUMS, np.float32), (1, CONTIG_INFO_DTYPE)):
        outs.append(ctx.upload(np.full((rows + 2 * guard_rows) * width * np.dtype(dtype).itemsize, 0xA5, np.uint8)))
    d_bad = ctx.upload(np.array([12345], np.int64))
    need = int(lib().palace_contig_features_scratch_bytes(len(text), rows))
    d_scratch = DevBuf(ctx, max(need, 1))
    at = [b.ptr + guard_rows * w * isz for b, w, isz in zip(outs, (CONTIG_FEATURES, CONTIG_FSUMS, 1), (4, 4, 16))]
    for _ in range(repeat):
        contig_features_enqueue(ctx, d_text.ptr, len(text), d_recs.ptr, r0, r1, at[0], at[1], at[2], d_bad.ptr, d_scratch.ptr, need)
    ctx.sync()
    got = []
    for b, width, dtype in zip(outs, (CONTIG_FEATURES, CONTIG_FSUMS, 1), (np.float32, np.float32, CONTIG_INFO_DTYPE)):
        raw = b.to_host()
        g = guard_rows * width * np.dtype(dtype).itemsize
        if not ((raw[:g] == 0xA5).all() and (raw[len(raw) - g:] == 0xA5).all()):
            raise PalaceError("palace_contig_features wrote outside its rows")
        got.append(raw[g:len(raw) - g].view(dtype).reshape(rows, width) if width > 1 else raw[g:len(raw) - g].view(dtype))
    bad = int(d_bad.to_host()[0])
    for b in outs + [d_bad, d_scratch, d_text, d_recs]:
        b.free()
    return st, recs, got[0], got[1], got[2], bad


class PathFasta:
    """The chain behind make_fa_from_path at the ABI: an indexed FASTA with its name table, then per paths file resolve ->
    lengths -> write.  The host's part -- tokens, headers, the paths' places in the output -- is the caller's (tests/path_fasta_cases.py)."""

    def __init__(self, ctx: Ctx, text: bytes):
        self.ctx = ctx
        self.status, self.recs, self.d_text, self.d_recs = fasta_index(ctx, text)
        assert self.status.error == 0, (self.status.error, self.status.bad_line)
        self.n = int(self.status.n_records)
        self.d_dup = ctx.empty((max(self.n, 1),), np.uint8)
        self.names = C.c_void_p()
        _check(lib().palace_fasta_names_create(ctx.h, self.d_text.ptr, self.d_recs.ptr, self.n, self.d_dup.ptr, C.byref(self.names)), "palace_fasta_names_create")

    def duplicates(self) -> np.ndarray:
        return self.d_dup.to_host()[:self.n]

    def resolve(self, tokens):
        """tokens: cleaned token bytes in file order -> (codes on the host, device buffer of the codes)"""
        off = np.zeros(len(tokens) + 1, np.int64)
        np.cumsum([len(t) for t in tokens], out=off[1:])
        d_tok = self.ctx.upload(np.frombuffer(b"".join(tokens), np.uint8))
        d_off = self.ctx.upload(off)
        d_code = self.ctx.empty((max(len(tokens), 1),), np.int32)
        _check(lib().palace_path_resolve(self.ctx.h, self.names, d_tok.ptr, d_off.ptr, len(tokens), d_code.ptr), "palace_path_resolve")
        return d_code.to_host()[:len(tokens)], d_code

    def lengths(self, d_code: DevBuf, path_off: np.ndarray):
        n_tok, n_paths = int(path_off[-1]), len(path_off) - 1
        d_path_off = self.ctx.upload(np.asarray(path_off, np.int64))
        d_cum = self.ctx.empty((n_tok + 1,), np.int64)
        d_len = self.ctx.empty((max(n_paths, 1),), np.int64)
        _check(lib().palace_path_fasta_lengths(self.ctx.h, self.d_recs.ptr, d_code.ptr, n_tok, d_path_off.ptr, n_paths, d_cum.ptr, d_len.ptr),
               "palace_path_fasta_lengths")
        return d_len.to_host()[:n_paths], d_cum, d_path_off

    def writer(self, d_code: DevBuf, d_cum: DevBuf, d_path_off: DevBuf, headers, lens):
        """-> (total bytes of the output text, windows(cuts))"""
        n_paths = len(headers)
        hdr_off = np.zeros(n_paths + 1, np.int64)
        np.cumsum([len(h) for h in headers], out=hdr_off[1:])
        path_out = np.zeros(n_paths + 1, np.int64)
        np.cumsum([len(h) + int(l) + 3 for h, l in zip(headers, lens)], out=path_out[1:])
        d_hdr = self.ctx.upload(np.frombuffer(b"".join(headers), np.uint8))
        d_hdr_off, d_path_out = self.ctx.upload(hdr_off), self.ctx.upload(path_out)

        def windows(cuts, guard: int = 32):
            """the text in the windows [0, c1), [c1, c2), ... [ck, total) for the ascending cuts c1 .. ck (equal neighbours: an empty
            window), every window in a slot of its own of one device buffer with `guard` bytes (a multiple of 16) in front of and
            behind it -> (the windows' bytes joined, every guard byte untouched)"""
            total = int(path_out[-1])
            bounds = [0] + [int(c) for c in cuts] + [total]
            slots, at = [], 0
            for lo, hi in zip(bounds, bounds[1:]):
                slots.append(at + guard)
                at += guard + (hi - lo + 15) // 16 * 16 + guard
            d_out = self.ctx.upload(np.full(max(at, 1), 0xA5, np.uint8))
            for (lo, hi), slot in zip(zip(bounds, bounds[1:]), slots):
                _check(lib().palace_path_fasta_write(self.ctx.h, self.d_text.ptr, self.d_recs.ptr, d_code.ptr, d_cum.ptr, d_path_off.ptr, n_paths, d_hdr.ptr,
                                                     d_hdr_off.ptr, d_path_out.ptr, lo, hi, d_out.ptr + slot), "palace_path_fasta_write")
            got = d_out.to_host()
            d_out.free()
            keep = np.zeros(len(got), bool)
            for (lo, hi), slot in zip(zip(bounds, bounds[1:]), slots):
                keep[slot:slot + hi - lo] = True
            return got[keep].tobytes(), bool((got[~keep] == 0xA5).all())
        return int(path_out[-1]), windows

    def close(self):
        _check(lib().palace_fasta_names_destroy(self.ctx.h, self.names), "palace_fasta_names_destroy")


def cycle_trim(ctx: Ctx, node, base, length, path_off, arcs, trim_threshold: int, min_cycle_length: int, guard: int = 8):
    """palace_cycle_trim on host arrays (arcs: uint64 keys, sorted here as the ABI asks) -> (first, last, the guard entries around both
    results untouched)"""
    node, base = np.ascontiguousarray(node, np.int32), np.ascontiguousarray(base, np.int32)
    length, path_off = np.ascontiguousarray(length, np.int64), np.ascontiguousarray(path_off, np.int64)
    arcs = np.sort(np.ascontiguousarray(arcs, np.uint64))
    n_tok, n_paths = len(node), len(path_off) - 1
    assert len(base) == n_tok and len(length) == n_tok and int(path_off[-1]) == n_tok
    bufs = [ctx.upload(a) for a in (node, base, length, path_off, arcs)]
    d_first, d_last = (ctx.upload(np.full(n_paths + 2 * guard, -77, np.int32)) for _ in range(2))
    try:
        _check(lib().palace_cycle_trim(ctx.h, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, n_tok, bufs[3].ptr, n_paths, bufs[4].ptr, len(arcs),
                                       int(trim_threshold), int(min_cycle_length), d_first.ptr + 4 * guard, d_last.ptr + 4 * guard), "palace_cycle_trim")
        first, last = d_first.to_host(), d_last.to_host()
    finally:
        for b in bufs + [d_first, d_last]:
            b.free()
    intact = all(bool((a[:guard] == -77).all() and (a[guard + n_paths:] == -77).all()) for a in (first, last))
    return first[guard:guard + n_paths], last[guard:guard + n_paths], intact


class FinalFasta(PathFasta):
    """The chain behind make_final_fa's output at the ABI: PathFasta's index, names and resolve, then palace_final_fasta_lengths and
    palace_final_fasta_write.  Headers are given for the paths that have text only; the others get no byte."""

    def lengths(self, d_code: DevBuf, path_off: np.ndarray, sep_len: int = 50):
        n_tok, n_paths = int(path_off[-1]), len(path_off) - 1
        d_path_off = self.ctx.upload(np.asarray(path_off, np.int64))
        d_cum = self.ctx.empty((n_tok + 1,), np.int64)
        d_len = self.ctx.empty((max(n_paths, 1),), np.int64)
        _check(lib().palace_final_fasta_lengths(self.ctx.h, self.d_recs.ptr, d_code.ptr, n_tok, d_path_off.ptr, n_paths, sep_len, d_cum.ptr, d_len.ptr),
               "palace_final_fasta_lengths")
        return d_len.to_host()[:n_paths], d_cum, d_path_off

    def writer(self, d_code: DevBuf, d_cum: DevBuf, d_path_off: DevBuf, headers, lens, sep_byte: int = ord("N")):
        """headers[p]: the header of path p, None for a path without text -> (total bytes of the output text, windows(cuts))"""
        n_paths = len(headers)
        hdr_off = np.zeros(n_paths + 1, np.int64)
        np.cumsum([len(h or b"") for h in headers], out=hdr_off[1:])
        path_out = np.zeros(n_paths + 1, np.int64)
        np.cumsum([0 if h is None else len(h) + int(l) + 3 for h, l in zip(headers, lens)], out=path_out[1:])
        d_hdr = self.ctx.upload(np.frombuffer(b"".join(h or b"" for h in headers), np.uint8))
        d_hdr_off, d_path_out = self.ctx.upload(hdr_off), self.ctx.upload(path_out)
        total = int(path_out[-1])

        def windows(cuts, guard: int = 32):
            """as PathFasta.writer's: the text in the windows the ascending cuts give, every window in a slot of its own between
            guards -> (the windows' bytes joined, every guard byte untouched)"""
            bounds = [0] + [int(c) for c in cuts] + [total]
            slots, at = [], 0
            for lo, hi in zip(bounds, bounds[1:]):
                slots.append(at + guard)
                at += guard + (hi - lo + 15) // 16 * 16 + guard
            d_out = self.ctx.upload(np.full(max(at, 1), 0xA5, np.uint8))
            for (lo, hi), slot in zip(zip(bounds, bounds[1:]), slots):
                _check(lib().palace_final_fasta_write(self.ctx.h, self.d_text.ptr, self.d_recs.ptr, d_code.ptr, d_cum.ptr, d_path_off.ptr, n_paths, d_hdr.ptr,
                                                      d_hdr_off.ptr, d_path_out.ptr, sep_byte, lo, hi, d_out.ptr + slot), "palace_final_fasta_write")
            got = d_out.to_host()
            d_out.free()
            keep = np.zeros(len(got), bool)
            for (lo, hi), slot in zip(zip(bounds, bounds[1:]), slots):
                keep[slot:slot + hi - lo] = True
            return got[keep].tobytes(), bool((got[~keep] == 0xA5).all())
        return total, windows


FASTG_EPLUS, FASTG_EHIGH, FASTG_ECR, FASTG_ENOLF, FASTG_EEMPTY, FASTG_ENONAME, FASTG_EBASE = range(6, 13)


class FastgSplit:
    """The chain behind split_fastg at the ABI: palace_fasta_index -> palace_fastg_derive -> palace_fasta_names_create ->
    palace_fastg_plan -> palace_fastg_write, and the `.fai` rows of the output and of the FASTG itself.  verdict: (code, line), the
    smaller of the index's and the FASTG faults' (line, code); with one nothing behind derive is run."""

    def __init__(self, ctx: Ctx, text: bytes):
        self.ctx, self.names, self.whole_names = ctx, C.c_void_p(), C.c_void_p()
        self.index_status, self.recs, self.d_text, self.d_recs = fasta_index(ctx, text)
        self.n = int(self.index_status.n_records)
        self.d_name_recs = ctx.empty((max(self.n, 1),), FASTA_REC_DTYPE)
        self.d_primed = ctx.empty((max(self.n, 1),), np.uint8)
        st = FastaStatus()
        _check(lib().palace_fastg_derive(ctx.h, self.d_text.ptr, len(text), self.d_recs.ptr, self.n, self.d_name_recs.ptr, self.d_primed.ptr, C.byref(st)),
               "palace_fastg_derive")
        self.new_verdict = (int(st.error), int(st.bad_line))
        faults = [(l, c) for c, l in (self.new_verdict, (int(self.index_status.error), int(self.index_status.bad_line))) if c]
        self.verdict = min(faults)[::-1] if faults else (0, 0)
        self.total = self.n_kept = 0
        if self.verdict != (0, 0):
            return
        self.d_dup = ctx.empty((max(self.n, 1),), np.uint8)
        _check(lib().palace_fasta_names_create(ctx.h, self.d_text.ptr, self.d_name_recs.ptr, self.n, self.d_dup.ptr, C.byref(self.names)), "palace_fasta_names_create")
        self.d_out_off = ctx.empty((self.n + 1,), np.int64)
        self.d_out_recs = ctx.empty((max(self.n, 1),), FASTA_REC_DTYPE)
        kept, total = C.c_int64(), C.c_int64()
        _check(lib().palace_fastg_plan(ctx.h, self.d_name_recs.ptr, self.d_dup.ptr, self.n, self.d_out_off.ptr, self.d_out_recs.ptr, C.byref(kept), C.byref(total)),
               "palace_fastg_plan")
        self.n_kept, self.total = int(kept.value), int(total.value)

    def derived(self):
        """-> (name records, primed bits, duplicate flags, output offsets) on the host"""
        return self.d_name_recs.to_host()[:self.n], self.d_primed.to_host()[:self.n], self.d_dup.to_host()[:self.n], self.d_out_off.to_host()

    def windows(self, cuts, guard: int = 32):
        """the output in the windows [0, c1), [c1, c2), ... [ck, total), every window in a slot of its own of one device buffer with
        `guard` bytes in front of and behind it -> (the windows' bytes joined, every guard byte untouched)"""
        bounds = [0] + [int(c) for c in cuts] + [self.total]
        slots, at = [], 0
        for lo, hi in zip(bounds, bounds[1:]):
            slots.append(at + guard)
            at += guard + (hi - lo + 15) // 16 * 16 + guard
        d_out = self.ctx.upload(np.full(max(at, 1), 0xA5, np.uint8))
        for (lo, hi), slot in zip(zip(bounds, bounds[1:]), slots):
            _check(lib().palace_fastg_write(self.ctx.h, self.d_text.ptr, self.d_name_recs.ptr, self.d_primed.ptr, self.d_out_off.ptr, self.n, lo, hi,
                                            d_out.ptr + slot), "palace_fastg_write")
        got = d_out.to_host()
        d_out.free()
        keep = np.zeros(len(got), bool)
        for (lo, hi), slot in zip(zip(bounds, bounds[1:]), slots):
            keep[slot:slot + hi - lo] = True
        return got[keep].tobytes(), bool((got[~keep] == 0xA5).all())

    def _rows(self, d_recs: DevBuf, d_skip: DevBuf) -> bytes:
        d_off = self.ctx.empty((self.n + 1,), np.int64)
        total = C.c_int64()
        _check(lib().palace_fai_rows_plan(self.ctx.h, d_recs.ptr, d_skip.ptr, self.n, d_off.ptr, C.byref(total)), "palace_fai_rows_plan")
        d_out = self.ctx.upload(np.full(int(total.value) + 16, 0xA5, np.uint8))
        _check(lib().palace_fai_rows_write(self.ctx.h, self.d_text.ptr, d_recs.ptr, d_skip.ptr, self.n, d_off.ptr, d_out.ptr), "palace_fai_rows_write")
        got = d_out.to_host()
        assert (got[int(total.value):] == 0xA5).all(), "bytes behind the rows were written"
        return got[:int(total.value)].tobytes()

    def output_fai(self) -> bytes:
        return self._rows(self.d_out_recs, self.d_dup)

    def graph_fai(self):
        """-> (rows, flags of the records left out)"""
        d_skip = self.ctx.empty((max(self.n, 1),), np.uint8)
        if not self.whole_names:
            _check(lib().palace_fasta_names_create(self.ctx.h, self.d_text.ptr, self.d_recs.ptr, self.n, d_skip.ptr, C.byref(self.whole_names)),
                   "palace_fasta_names_create")
        return self._rows(self.d_recs, d_skip), d_skip.to_host()[:self.n]

    def close(self):
        for t in (self.names, self.whole_names):
            if t:
                _check(lib().palace_fasta_names_destroy(self.ctx.h, t), "palace_fasta_names_destroy")
        self.names, self.whole_names = C.c_void_p(), C.c_void_p()


# ---- faidx: regions resolved, planned and written ---------------------------------------------------------------------------------------

def _blob(ctx: Ctx, items):
    """byte strings one behind the other and their len(items) + 1 offsets, on the device"""
    off = np.zeros(len(items) + 1, np.int64)
    np.cumsum([len(t) for t in items], out=off[1:])
    return ctx.upload(np.frombuffer(b"".join(items), np.uint8)), ctx.upload(off)


class Faidx(PathFasta):
    """The chain behind faidx's fetch at the ABI: an indexed FASTA with its name table (PathFasta), then per list of regions
    palace_faidx_resolve -> palace_faidx_plan -> palace_faidx_write.  The expected bytes are the caller's (tests/faidx_cases.py)."""

    def resolve_regions(self, regions, guard: int = 2):
        """-> (the regions as FAIDX_REGION_DTYPE on the host, on the device); `guard` entries behind the last must stay untouched"""
        n = len(regions)
        d_reg, d_off = _blob(self.ctx, regions)
        fill = np.full((n + guard) * FAIDX_REGION_DTYPE.itemsize, 0xA5, np.uint8)
        d_out = self.ctx.upload(fill)
        _check(lib().palace_faidx_resolve(self.ctx.h, self.names, self.d_recs.ptr, d_reg.ptr, d_off.ptr, n, d_out.ptr), "palace_faidx_resolve")
        got = d_out.to_host()
        assert (got[n * FAIDX_REGION_DTYPE.itemsize:] == 0xA5).all(), "palace_faidx_resolve: written behind its regions"
        d_reg.free()
        d_off.free()
        return got[:n * FAIDX_REGION_DTYPE.itemsize].view(FAIDX_REGION_DTYPE).copy(), d_out

    def upload_regions(self, resolved):
        """(rec, beg, len) triples of the caller's -> a device buffer as resolve_regions leaves one"""
        a = np.zeros(max(len(resolved), 1), FAIDX_REGION_DTYPE)
        for i, (r, b, ln) in enumerate(resolved):
            a[i] = (r, b, ln)
        return self.ctx.upload(a)

    def plan(self, d_regions: DevBuf, n_regions: int, headers, line_len: int, skip_failed: bool):
        """-> (offsets on the host, total, first failed, (d_hdr, d_hdr_off, d_out_off))"""
        d_hdr, d_hdr_off = _blob(self.ctx, headers)
        d_out_off = self.ctx.upload(np.full(n_regions + 1 + 2, -7, np.int64))
        total, first = C.c_int64(-5), C.c_int64(-5)
        _check(lib().palace_faidx_plan(self.ctx.h, d_regions.ptr, n_regions, d_hdr_off.ptr, line_len, int(skip_failed), d_out_off.ptr, C.byref(total),
                                       C.byref(first)), "palace_faidx_plan")
        off = d_out_off.to_host()
        assert (off[n_regions + 1:] == -7).all(), "palace_faidx_plan: written behind its offsets"
        return off[:n_regions + 1].copy(), int(total.value), int(first.value), (d_hdr, d_hdr_off, d_out_off)

    def write(self, d_regions: DevBuf, n_regions: int, planned, line_len: int, reverse: bool, bounds, guard: int = 64):
        """the windows [lo, hi) of `bounds`, every one in a slot of its own of one device buffer with `guard` bytes (a multiple of
        16) in front of and behind it -> ([the windows' bytes], every guard byte untouched)"""
        d_hdr, d_hdr_off, d_out_off = planned
        slots, at = [], 0
        for lo, hi in bounds:
            slots.append(at + guard)
            at += guard + (hi - lo + 15) // 16 * 16 + guard
        d_out = self.ctx.upload(np.full(max(at, 1), 0xA5, np.uint8))
        for (lo, hi), slot in zip(bounds, slots):
            _check(lib().palace_faidx_write(self.ctx.h, self.d_text.ptr, self.d_recs.ptr, d_regions.ptr, n_regions, d_hdr.ptr, d_hdr_off.ptr, d_out_off.ptr, line_len,
                                            int(reverse), lo, hi, d_out.ptr + slot), "palace_faidx_write")
        got = d_out.to_host()
        d_out.free()
        keep = np.zeros(len(got), bool)
        pieces = []
        for (lo, hi), slot in zip(bounds, slots):
            keep[slot:slot + hi - lo] = True
            pieces.append(got[slot:slot + hi - lo].tobytes())
        return pieces, bool((got[~keep] == 0xA5).all())


# ---- filter_result: the BLAST groups, the paths' classes, the first of equal paths ----------------------------------------------------

def blast_identity_cuts(threshold: float):
    """palace_blast_identity_cuts -> the seven cuts (host arithmetic; the library need not reach a device)"""
    cut = (C.c_int64 * 7)()
    _check(lib().palace_blast_identity_cuts(float(threshold), cut), "palace_blast_identity_cuts")
    return list(cut)


def blast_groups(ctx: Ctx, fasta: "PathFasta", table: bytes, ratio: float, guard: int = 64):
    """palace_sam_lines and palace_blast_groups over `table` against the names of `fasta` -> dict: lines, groups, flagged, err_line,
    err_code, seg (uint8 per record), intact (the guard bytes around seg came back as they went in)"""
    table = bytes(table)
    n = len(table)
    nscr = int(lib().palace_sam_scratch_bytes(n))
    bufs = [ctx.upload(np.frombuffer(table, dtype=np.uint8) if n else np.zeros(1, np.uint8)), ctx.empty(max(nscr, 1), np.uint8)]
    out = (C.c_int64 * 5)()
    try:
        _check(lib().palace_sam_lines(ctx.h, bufs[0].ptr, n, bufs[1].ptr, nscr, None, 0, out), "palace_sam_lines")
        n_lines = int(out[0])
        bufs.append(ctx.empty(n_lines + 1, np.int64))
        _check(lib().palace_sam_lines(ctx.h, bufs[0].ptr, n, bufs[1].ptr, nscr, bufs[2].ptr, n_lines + 1, out), "palace_sam_lines")
        bufs.append(ctx.upload(np.full(fasta.n + 2 * guard, 0xA5, np.uint8)))
        cut = (C.c_int64 * 7)(*blast_identity_cuts(ratio * 100.0))
        _check(lib().palace_blast_groups(ctx.h, bufs[0].ptr, bufs[2].ptr, n_lines, fasta.names, fasta.n, float(ratio), cut, bufs[3].ptr + guard, out),
               "palace_blast_groups")
        raw = bufs[3].to_host()
        return dict(lines=int(out[0]), groups=int(out[1]), flagged=int(out[2]), err_line=int(out[3]), err_code=int(out[4]),
                    seg=raw[guard:guard + fasta.n].copy(), intact=bool((raw[:guard] == 0xA5).all() and (raw[guard + fasta.n:] == 0xA5).all()))
    finally:
        for b in bufs:
            b.free()


class FilterPlan:
    """Paths as record codes on the device (code = record << 2 | PALACE_PATH_REVERSE, negative: no record) over records of the given
    lengths: plan(tags, rec_bits) -> (class bytes, all_len); first_of_equal(classes, hash_bits) -> the first-of-equal bytes."""

    def __init__(self, ctx: Ctx, code, path_off, rec_len):
        self.ctx = ctx
        self.n_paths = len(path_off) - 1
        recs = np.zeros((max(len(rec_len), 1), 6), np.int64)
        recs[:len(rec_len), 3] = rec_len
        code = np.ascontiguousarray(code, np.int32)
        assert int(path_off[-1]) == len(code)
        self.d_code = ctx.upload(code if len(code) else np.zeros(1, np.int32))
        self.d_off = ctx.upload(np.ascontiguousarray(path_off, np.int64))
        self.d_recs = ctx.upload(recs)
        self.bufs = [self.d_code, self.d_off, self.d_recs]

    def plan(self, tags, rec_bits):
        n = self.n_paths
        d_tag, d_bits = self.ctx.upload(np.ascontiguousarray(tags, np.uint8)), self.ctx.upload(np.ascontiguousarray(rec_bits, np.uint8))
        d_cls, d_all = self.ctx.empty(max(n, 1), np.uint8), self.ctx.empty(max(n, 1), np.int64)
        try:
            _check(lib().palace_filter_result_plan(self.ctx.h, self.d_code.ptr, self.d_off.ptr, n, d_tag.ptr, self.d_recs.ptr, d_bits.ptr, d_cls.ptr, d_all.ptr),
                   "palace_filter_result_plan")
            return d_cls.to_host()[:n].copy(), d_all.to_host()[:n].copy()
        finally:
            for b in (d_tag, d_bits, d_cls, d_all):
                b.free()

    def first_of_equal(self, classes, hash_bits: int = 64):
        n = self.n_paths
        d_cls, d_first = self.ctx.upload(np.ascontiguousarray(classes, np.uint8)), self.ctx.empty(max(n, 1), np.uint8)
        try:
            _check(lib().palace_paths_first_of_equal(self.ctx.h, self.d_code.ptr, self.d_off.ptr, n, d_cls.ptr, hash_bits, d_first.ptr),
                   "palace_paths_first_of_equal")
            return d_first.to_host()[:n].copy()
        finally:
            d_cls.free()
            d_first.free()

    def free(self):
        for b in self.bufs:
            b.free()


# ---- corrected_dup: borders, tandem candidates, the similarity relation, the base-set test --------------------------------------------

PATHS_REL_NONE, PATHS_REL_J_LOSES, PATHS_REL_I_LOSES = 0, 1, 2     # PALACE_PATHS_REL_*


class PathDedup:
    """Paths as integers on the device (one value per token, path p = values[path_off[p]:path_off[p + 1]]) behind the four entry
    points of csrc/path_dedup.hip.  What a value means is the call's: a token id for borders() and tandems(), a length for
    length_relation(), a base id for base_set_in()."""

    def __init__(self, ctx: Ctx, values, path_off, dtype=np.int32):
        self.ctx = ctx
        values = np.ascontiguousarray(values, dtype)
        self.path_off = np.ascontiguousarray(path_off, np.int64)
        self.n_paths, self.n_tok = len(self.path_off) - 1, len(values)
        assert int(self.path_off[-1]) == self.n_tok
        self.d_val = ctx.upload(values if self.n_tok else np.zeros(1, dtype))
        self.d_off = ctx.upload(self.path_off)

    def borders(self):
        """palace_path_borders -> int32 per path"""
        d_out = self.ctx.empty(max(self.n_paths, 1), np.int32)
        try:
            _check(lib().palace_path_borders(self.ctx.h, self.d_val.ptr, self.d_off.ptr, self.n_paths, d_out.ptr), "palace_path_borders")
            return d_out.to_host()[:self.n_paths].copy()
        finally:
            d_out.free()

    def tandems(self, cap=None, guard: int = 48):
        """palace_path_tandems twice, count then fill -> (count, cand_off of the count call, cand_off of the fill call, the candidates
        as rows r, s, c, intact: the guard words around them came back as they went in).  cap: what the fill call is told instead of
        the count (a smaller one must be refused: PalaceError)."""
        n = C.c_int64()
        d_off = [self.ctx.upload(np.full(self.n_paths + 1, -7, np.int64)) for _ in range(2)]
        bufs = list(d_off)
        try:
            _check(lib().palace_path_tandems(self.ctx.h, self.d_val.ptr, self.d_off.ptr, self.n_paths, d_off[0].ptr, None, 0, C.byref(n)), "palace_path_tandems")
            count = int(n.value)
            d_cand = self.ctx.upload(np.full(3 * count + 2 * guard, -5, np.int32))
            bufs.append(d_cand)
            _check(lib().palace_path_tandems(self.ctx.h, self.d_val.ptr, self.d_off.ptr, self.n_paths, d_off[1].ptr, d_cand.ptr + 4 * guard,
                                             count if cap is None else cap, C.byref(n)), "palace_path_tandems")
            raw = d_cand.to_host()
            intact = bool((raw[:guard] == -5).all() and (raw[guard + 3 * count:] == -5).all()) and int(n.value) == count
            return count, d_off[0].to_host(), d_off[1].to_host(), raw[guard:guard + 3 * count].reshape(-1, 3).copy(), intact
        finally:
            for b in bufs:
                b.free()

    def length_relation(self, guard: int = 64):
        """palace_paths_length_relation (the values are int64 lengths) -> (the n_paths x n_paths table of PATHS_REL_* codes, intact)"""
        nb = int(lib().palace_paths_length_relation_bytes(self.n_paths))
        d_rel = self.ctx.upload(np.full(nb + 2 * guard, 0xA5, np.uint8))
        try:
            _check(lib().palace_paths_length_relation(self.ctx.h, self.d_val.ptr, self.n_tok, self.d_off.ptr, self.n_paths, d_rel.ptr + guard),
                   "palace_paths_length_relation")
            raw = d_rel.to_host()
            body = raw[guard:guard + nb]
            codes = np.stack([(body >> (2 * e)) & 3 for e in range(4)], axis=1).reshape(-1)[:self.n_paths * self.n_paths]
            return codes.reshape(self.n_paths, self.n_paths), bool((raw[:guard] == 0xA5).all() and (raw[guard + nb:] == 0xA5).all())
        finally:
            d_rel.free()

    def base_set_in(self, n_cycles: int, hash_bits: int = 64):
        """palace_paths_base_set_in (the values are base ids) -> uint8 per path"""
        d_in = self.ctx.empty(max(self.n_paths, 1), np.uint8)
        try:
            _check(lib().palace_paths_base_set_in(self.ctx.h, self.d_val.ptr, self.n_tok, self.d_off.ptr, self.n_paths, n_cycles, hash_bits, d_in.ptr),
                   "palace_paths_base_set_in")
            return d_in.to_host()[:self.n_paths].copy()
        finally:
            d_in.free()

    def free(self):
        self.d_val.free()
        self.d_off.free()
