"""sage2_amd -- ctypes binding of libsage2ov.so, the MI355X-native SAGE2 read-overlap path (steps 1-3, and the graph simplification of step 4).

The product is the C-ABI library (include/sage2ov.h) built from sage2_amd/csrc by __graft_entry__.build()
or `make -C sage2_amd/csrc`.  This module only loads it and wraps the calls; it never computes anything
itself and has no CPU fallback: if the library is missing, or no GPU is usable, calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SAGE2OV_LIB") or os.path.join(_HERE, "libsage2ov.so")     # override only for A/B builds


class Sage2ovError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"sage2ov error {code}: {msg}")
        self.code = code


class Config(C.Structure):
    _fields_ = [("min_overlap", C.c_uint32), ("device", C.c_int32), ("rank", C.c_uint32), ("world", C.c_uint32),
                ("host_threads", C.c_uint32), ("flags", C.c_uint32)]


class ReadStats(C.Structure):
    _fields_ = [("total_reads", C.c_uint64), ("good_reads", C.c_uint64), ("unique_reads", C.c_uint64), ("total_bp", C.c_uint64),
                ("average_read_length", C.c_uint64), ("max_read_length", C.c_uint32), ("words_per_read", C.c_uint32)]


class IndexStats(C.Structure):
    _fields_ = [("slots", C.c_uint64), ("keys", C.c_uint64), ("csr_entries", C.c_uint64), ("long_buckets", C.c_uint64),
                ("hash_string_length", C.c_uint32), ("rebuilds", C.c_uint32), ("minimiser_groups", C.c_uint32), ("reserved", C.c_uint32)]


class FindStats(C.Structure):
    _fields_ = [("queries", C.c_uint64), ("found", C.c_uint64), ("not_good", C.c_uint64), ("not_found", C.c_uint64),
                ("directory_bits", C.c_uint32), ("launches", C.c_uint32), ("device_ms", C.c_double), ("directory_ms", C.c_double),
                ("pack_ms", C.c_double), ("search_ms", C.c_double), ("route", C.c_uint32), ("reserved", C.c_uint32)]


FIND_ROUTE_HOST, FIND_ROUTE_ID_STORE, FIND_ROUTE_LOCALITY = 0, 1, 2


class MateStats(C.Structure):
    _fields_ = [("pairs_seen", C.c_uint64), ("pairs_added", C.c_uint64), ("pairs_not_good", C.c_uint64), ("pairs_not_found", C.c_uint64),
                ("records", C.c_uint64), ("entries_before", C.c_uint64), ("entries_after", C.c_uint64),
                ("library", C.c_uint32), ("libraries", C.c_uint32), ("chunks", C.c_uint32), ("sort_passes", C.c_uint32), ("flushes", C.c_uint32), ("route", C.c_uint32),
                ("find_ms", C.c_double), ("records_ms", C.c_double), ("sort_ms", C.c_double), ("reduce_ms", C.c_double), ("merge_ms", C.c_double)]


MATE_ROUTE_HOST, MATE_ROUTE_DEVICE = 0, 1
# sage2ov_mate (32 bytes)
MATE_DTYPE = np.dtype([("from", np.uint32), ("to", np.uint32), ("count", np.uint64), ("first", np.uint64), ("freq", np.uint8), ("type1", np.uint8),
                       ("type2", np.uint8), ("library", np.uint8), ("pad", np.uint8, (4,))])


# sage2ov_read_edge (32 bytes): one entry of the read-to-edge table
READ_EDGE_DTYPE = np.dtype([("read", np.uint32), ("pair", np.uint32), ("from", np.uint32), ("to", np.uint32), ("n_forward", np.uint32), ("n_reverse", np.uint32),
                            ("location", np.uint32), ("type", np.uint8), ("pad", np.uint8, (3,))])
INSERT_ROUNDS = 10


class Insert(C.Structure):
    _fields_ = [("valid", C.c_uint32), ("rounds", C.c_uint32), ("final_round", C.c_uint32), ("library", C.c_uint32),
                ("considered", C.c_uint64 * INSERT_ROUNDS), ("mu", C.c_int64 * INSERT_ROUNDS), ("sd", C.c_int64 * INSERT_ROUNDS),
                ("mean", C.c_int64), ("deviation", C.c_int64), ("lower", C.c_int64), ("upper", C.c_int64)]


class ReadMapStats(C.Structure):
    _fields_ = [("entries", C.c_uint64), ("locations", C.c_uint64), ("records", C.c_uint64), ("mate_entries", C.c_uint64), ("distances", C.c_uint64 * 128),
                ("sort_passes", C.c_uint32), ("route", C.c_uint32), ("rounds", C.c_uint32), ("reserved", C.c_uint32),
                ("scan_ms", C.c_double), ("records_ms", C.c_double), ("sort_ms", C.c_double), ("reduce_ms", C.c_double), ("join_ms", C.c_double), ("round_ms", C.c_double)]


# sage2ov_support (24 bytes): one (in-half, out-half) pair of a node with its mate-pair support
SUPPORT_DTYPE = np.dtype([("node", np.uint32), ("pair_in", np.uint32), ("pair_out", np.uint32), ("to_in", np.uint32), ("to_out", np.uint32), ("support", np.uint32)])


class SupportStats(C.Structure):
    _fields_ = [("in_halves", C.c_uint64), ("out_halves", C.c_uint64), ("candidates", C.c_uint64), ("entries_within", C.c_uint64), ("records", C.c_uint64),
                ("keys", C.c_uint64), ("keys2", C.c_uint64), ("sort_passes", C.c_uint32), ("reserved", C.c_uint32),
                ("roles_ms", C.c_double), ("scan_ms", C.c_double), ("records_ms", C.c_double), ("sort_ms", C.c_double), ("reduce_ms", C.c_double)]


# sage2ov_merge (40 bytes): one merge of the last round of extend_round
MERGE_DTYPE = np.dtype([("node", np.uint32), ("from", np.uint32), ("to", np.uint32), ("support", np.uint32), ("pair_in", np.uint32), ("pair_out", np.uint32),
                        ("pair_new", np.uint32), ("flow", np.float32), ("type", np.uint8), ("in_deleted", np.uint8), ("out_deleted", np.uint8), ("pad", np.uint8, (5,))])


class ExtendCounts(C.Structure):
    _fields_ = [("entries", C.c_uint64), ("at_threshold", C.c_uint64), ("refused", C.c_uint64), ("blocked", C.c_uint64), ("merges", C.c_uint64),
                ("entries_copied", C.c_uint64), ("pairs_deleted", C.c_uint64), ("batches", C.c_uint64),
                ("sweep_ms", C.c_double), ("select_ms", C.c_double), ("lists_ms", C.c_double), ("commit_ms", C.c_double)]


class ExtendStats(C.Structure):
    _fields_ = [("rounds", C.c_uint64), ("reserved", C.c_uint64), ("last", ExtendCounts), ("total", ExtendCounts)]


# sage2ov_path_support (28 bytes): one (a enters the node, b leaves it) pair of halves with its path support
PATH_SUPPORT_DTYPE = np.dtype([("node", np.uint32), ("pair_a", np.uint32), ("pair_b", np.uint32), ("from_a", np.uint32), ("to_b", np.uint32), ("support", np.uint32),
                               ("second_a", np.uint8), ("second_b", np.uint8), ("pad", np.uint8, (2,))])


class PathStats(C.Structure):
    _fields_ = [("claimed_reads", C.c_uint64), ("claiming_nodes", C.c_uint64), ("start_nodes", C.c_uint64), ("paths", C.c_uint64), ("capped_nodes", C.c_uint64),
                ("eligible_entries", C.c_uint64), ("voting_entries", C.c_uint64), ("records", C.c_uint64), ("rows", C.c_uint64),
                ("key_collisions", C.c_uint64), ("mirrored", C.c_uint64), ("order_dependent", C.c_uint64), ("sort_passes", C.c_uint32), ("reserved", C.c_uint32),
                ("claim_ms", C.c_double), ("starts_ms", C.c_double), ("walk_ms", C.c_double), ("vote_ms", C.c_double), ("sort_ms", C.c_double), ("reduce_ms", C.c_double)]


# sage2ov_join (48 bytes): one join of the last round of scaffold_round
JOIN_DTYPE = np.dtype([("from", np.uint32), ("to", np.uint32), ("support", np.uint32), ("gap", np.int32), ("pair_first", np.uint32), ("pair_second", np.uint32),
                       ("pair_new", np.uint32), ("overlap_forward", np.int32), ("overlap_twin", np.int32), ("type", np.uint8), ("first_deleted", np.uint8),
                       ("second_deleted", np.uint8), ("how_forward", np.uint8), ("how_twin", np.uint8), ("pad", np.uint8, (7,))])
JOIN_EQUAL, JOIN_OVERLAP, JOIN_CONCAT, JOIN_GAPPED = 0, 1, 2, 3


class ScaffoldCounts(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("below_threshold", C.c_uint64), ("skipped", C.c_uint64), ("blocked", C.c_uint64), ("cycles", C.c_uint64), ("merged", C.c_uint64),
                ("batches", C.c_uint64), ("overlaps", C.c_uint64), ("concatenated", C.c_uint64), ("gapped", C.c_uint64), ("outside_reference", C.c_uint64),
                ("entries_copied", C.c_uint64), ("pairs_deleted", C.c_uint64),
                ("sweep_ms", C.c_double), ("select_ms", C.c_double), ("overlap_ms", C.c_double), ("lists_ms", C.c_double), ("commit_ms", C.c_double)]


class ScaffoldStats(C.Structure):
    _fields_ = [("rounds", C.c_uint64), ("reserved", C.c_uint64), ("last", ScaffoldCounts), ("total", ScaffoldCounts)]


# sage2ov_contig (48 bytes): one row of the contig table
CONTIG_DTYPE = np.dtype([("from", np.uint32), ("to", np.uint32), ("pair", np.uint32), ("edge_length", np.uint32), ("string_length", np.uint32), ("contig_length", np.uint32),
                         ("start", np.uint32), ("gap_count", np.uint32), ("n_count", np.uint32), ("flow", np.float32), ("type", np.uint8), ("pad", np.uint8, (7,))])


class Contig(C.Structure):
    _fields_ = [("from_", C.c_uint32), ("to", C.c_uint32), ("pair", C.c_uint32), ("edge_length", C.c_uint32), ("string_length", C.c_uint32), ("contig_length", C.c_uint32),
                ("start", C.c_uint32), ("gap_count", C.c_uint32), ("n_count", C.c_uint32), ("flow", C.c_float), ("type", C.c_uint8), ("pad", C.c_uint8 * 7)]


class ContigStats(C.Structure):
    _fields_ = [("contigs", C.c_uint64), ("written", C.c_uint64), ("bases", C.c_uint64), ("longest", C.c_uint64), ("n50", C.c_uint64), ("n50_ordinal", C.c_uint64),
                ("n90", C.c_uint64), ("n90_ordinal", C.c_uint64), ("covered", C.c_uint64), ("gaps", C.c_uint64), ("n_bases", C.c_uint64), ("inconsistent", C.c_uint64),
                ("wrapped", C.c_uint64), ("select_ms", C.c_double), ("sort_ms", C.c_double), ("layout_ms", C.c_double), ("spell_ms", C.c_double)]


# sage2ov_link (44 bytes): one ordered pair of half-edges that mate pairs link, with its support and mean gap
LINK_DTYPE = np.dtype([("pair_a", np.uint32), ("pair_b", np.uint32), ("from_a", np.uint32), ("to_a", np.uint32), ("from_b", np.uint32), ("to_b", np.uint32),
                       ("len_a", np.uint32), ("len_b", np.uint32), ("support", np.uint32), ("gap", np.int32),
                       ("second_a", np.uint8), ("second_b", np.uint8), ("type_a", np.uint8), ("type_b", np.uint8)])
LINKS_ALL, LINKS_FINAL, LINKS_SMALL = 0, 1, 2


class LinkStats(C.Structure):
    _fields_ = [("halves", C.c_uint64), ("entries_within", C.c_uint64), ("unique_entries", C.c_uint64), ("mate_entries", C.c_uint64), ("records", C.c_uint64),
                ("keys", C.c_uint64), ("sort_passes", C.c_uint32), ("reserved", C.c_uint32),
                ("halves_ms", C.c_double), ("scan_ms", C.c_double), ("records_ms", C.c_double), ("sort_ms", C.c_double), ("reduce_ms", C.c_double)]


# sage2ov_flow_arc (20 bytes): one arc of the flow network, cost as input.cs2 prints it
FLOW_ARC_DTYPE = np.dtype([("from", np.uint32), ("to", np.uint32), ("lower", np.int32), ("upper", np.int32), ("cost", np.float32)])
GENOME_ROUNDS = 10
MCF_ARC_DTYPE = np.dtype([("from", np.uint32), ("to", np.uint32), ("lower", np.int32), ("upper", np.int32), ("cost", np.int64)])      # sage2ov_mcf_arc
MCF_PHASES = 24
MCF_FORM_LDS, MCF_FORM_LAUNCHES = 1, 2
MCF_HUB_DEG = 65536                      # SAGE2OV_MCF_HUB_DEG: lists longer than this take the hub form of the launches


def wide_prices(words):
    """128-bit prices as the library hands them out (two uint64 words per node, the low one first, two's complement) as Python integers"""
    if words is None: return []
    lo, hi = words[0::2].tolist(), words[1::2].tolist()
    return [((h << 64) | l) - ((h >> 63) << 128) for l, h in zip(lo, hi)]


class GenomeEstimate(C.Structure):
    _fields_ = [("genome_size", C.c_uint64), ("estimate", C.c_uint64 * GENOME_ROUNDS), ("delta_sum", C.c_uint64 * GENOME_ROUNDS), ("k_sum", C.c_uint64 * GENOME_ROUNDS),
                ("rounds", C.c_uint32), ("degenerate", C.c_uint32), ("agreed", C.c_uint32), ("reserved", C.c_uint32)]


class McfStats(C.Structure):
    _fields_ = [("nodes", C.c_uint64), ("arcs", C.c_uint64), ("scale", C.c_uint64), ("phases", C.c_uint64), ("rounds", C.c_uint64), ("pushes", C.c_uint64),
                ("relabels", C.c_uint64), ("price_updates", C.c_uint64), ("total_cost", C.c_int64), ("form", C.c_uint32), ("price_words", C.c_uint32),
                ("build_ms", C.c_double), ("solve_ms", C.c_double), ("refine_rounds", C.c_uint64 * MCF_PHASES), ("refine_ms", C.c_double * MCF_PHASES)]


class CopyCountStats(C.Structure):
    _fields_ = [("genome_size", C.c_uint64), ("estimate", C.c_uint64 * GENOME_ROUNDS), ("rounds", C.c_uint32), ("degenerate", C.c_uint32), ("agreed", C.c_uint32),
                ("reserved", C.c_uint32), ("reads_present", C.c_uint64), ("nodes", C.c_uint64), ("edges", C.c_uint64), ("simple", C.c_uint64), ("once", C.c_uint64),
                ("many", C.c_uint64), ("network_nodes", C.c_uint64), ("network_arcs", C.c_uint64), ("t_to_s_flow", C.c_uint64), ("flow_different", C.c_uint64),
                ("solution_lines", C.c_uint64), ("lines_applied", C.c_uint64), ("prepare_ms", C.c_double), ("rounds_ms", C.c_double), ("order_ms", C.c_double),
                ("classes_ms", C.c_double), ("arcs_ms", C.c_double), ("apply_ms", C.c_double)]


class OverlapStats(C.Structure):
    _fields_ = [("verified_overlaps", C.c_uint64), ("contained_extension", C.c_uint64), ("contained_size", C.c_uint64),
                ("left_to_explore", C.c_uint64), ("edges_inserted", C.c_uint64), ("transitive_removed", C.c_uint64),
                ("edges", C.c_uint64), ("unresolved_hits", C.c_uint64)]


class SimplifyStats(C.Structure):
    _fields_ = [("nodes_contracted", C.c_uint64), ("removed", C.c_uint64), ("loop_iterations", C.c_uint64), ("edges", C.c_uint64),
                ("reads_on_edges", C.c_uint64), ("device_ms", C.c_double)]


class Timings(C.Structure):
    _fields_ = [("index_ms", C.c_double), ("probe_ms", C.c_double), ("reciprocal_ms", C.c_double), ("reduce_ms", C.c_double),
                ("convert_ms", C.c_double), ("total_ms", C.c_double), ("probe_kernel_ms", C.c_double), ("probe_kernel_launches", C.c_uint64), ("sequential_reads", C.c_uint64),
                ("organize_ms", C.c_double), ("probe_fast_launches", C.c_uint64), ("reciprocal_cond_ms", C.c_double), ("reduce_marks_ms", C.c_double)]


class SynthParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("genome_len", C.c_uint64), ("n_reads", C.c_uint64), ("read_len", C.c_uint32),
                ("read_len_min", C.c_uint32), ("err_ppm", C.c_uint32), ("n_repeat_families", C.c_uint32),
                ("repeat_copies", C.c_uint32), ("repeat_len", C.c_uint32)]


EDGE_DTYPE = np.dtype([("from", "<u8"), ("to", "<u8"), ("length", "<u4"), ("length_twin", "<u4"), ("type", "u1"), ("pad", "u1", (7,))])

_lib = None


def _preload_torch_hip():
    """libsage2ov.so and PyTorch-ROCm both need `libamdhip64.so.7`; torch ships its own copy next to its other
    ROCm libraries.  Whichever copy is mapped first serves both, and torch only finds its GPUs with ITS copy, so
    when torch is installed map that one first (no torch import needed).  The C++ CLI uses /opt/rocm's."""
    if os.environ.get("SAGE2OV_NO_TORCH_HIP"):
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec and spec.origin:
            cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
            if os.path.exists(cand):
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def lib():
    """Load libsage2ov.so (fails loudly when it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C sage2_amd/csrc`")
        _preload_torch_hip()
        L = C.CDLL(LIB_PATH)
        L.sage2ov_last_error.restype = C.c_char_p
        L.sage2ov_last_error.argtypes = [C.c_void_p]
        L.sage2ov_version.restype = C.c_char_p
        L.sage2ov_stream.restype = C.c_void_p
        L.sage2ov_stream.argtypes = [C.c_void_p]
        L.sage2ov_synth_read_len.restype = C.c_uint32
        _lib = L
    return _lib


def synth_genome(p: SynthParams) -> np.ndarray:
    g = np.zeros(p.genome_len, dtype=np.uint8)
    rc = lib().sage2ov_synth_genome(C.byref(p), C.c_void_p(g.ctypes.data))
    if rc:
        raise Sage2ovError(rc, "synth_genome")
    return g


def synth_reads_ascii(p: SynthParams, genome: np.ndarray, first=0, n=None):
    n = p.n_reads - first if n is None else n
    bases = np.zeros(n * p.read_len, dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint64)
    rc = lib().sage2ov_synth_reads_ascii(C.byref(p), C.c_void_p(genome.ctypes.data), C.c_uint64(first), C.c_uint64(n),
                                         C.c_void_p(bases.ctypes.data), C.c_void_p(off.ctypes.data))
    if rc:
        raise Sage2ovError(rc, "synth_reads_ascii")
    return bases[: int(off[n])], off


def synth_write_fasta(p: SynthParams, path: str):
    rc = lib().sage2ov_synth_write_fasta(C.byref(p), path.encode())
    if rc:
        raise Sage2ovError(rc, "synth_write_fasta")


def insert_estimate(d, average_read_length) -> Insert:
    """the rounds of MatePair::meanSdEstimation over the distances d (uint32), on the host: no context, no GPU"""
    d = np.ascontiguousarray(d, dtype=np.uint32)
    out = Insert()
    rc = lib().sage2ov_insert_estimate(C.c_void_p(d.ctypes.data), C.c_uint64(len(d)), C.c_uint64(average_read_length), C.byref(out))
    if rc:
        raise Sage2ovError(rc, "insert_estimate")
    return out


def genome_size_rounds(length, k, reads) -> GenomeEstimate:
    """the rounds of CopyCountEstimator::genomeSizeEstimation over lengthOfEdge and k of the non-loop pairs, on the host: no context, no GPU"""
    length = np.ascontiguousarray(length, dtype=np.uint32)
    k = np.ascontiguousarray(k, dtype=np.uint64)
    out = GenomeEstimate()
    rc = lib().sage2ov_genome_size_rounds(C.c_void_p(length.ctypes.data), C.c_void_p(k.ctypes.data), C.c_uint64(len(length)), C.c_uint64(reads), C.byref(out))
    if rc:
        raise Sage2ovError(rc, "genome_size_rounds")
    return out


def extend_threshold(reads, average_read_length, genome_size, iteration=1) -> int:
    """highTh of ContigExtender::extendContigs (mergeContigs.cpp:43-54) in the given iteration of its first loop, on the host: no context, no GPU"""
    out = C.c_int(0)
    rc = lib().sage2ov_extend_threshold(C.c_uint64(reads), C.c_uint64(average_read_length), C.c_uint64(genome_size), C.c_uint32(iteration), C.byref(out))
    if rc:
        raise Sage2ovError(rc, "extend_threshold")
    return int(out.value)


def scaffold_threshold(reads, average_read_length, genome_size, loop, iteration=1) -> int:
    """highTh of ScaffoldMaker::makeScaffolds (scaffolding.cpp:38-94) in the given iteration of loop 1..5, on the host: no context, no GPU"""
    out = C.c_int(0)
    rc = lib().sage2ov_scaffold_threshold(C.c_uint64(reads), C.c_uint64(average_read_length), C.c_uint64(genome_size), C.c_uint32(loop), C.c_uint32(iteration), C.byref(out))
    if rc:
        raise Sage2ovError(rc, "scaffold_threshold")
    return int(out.value)


def extend_short_threshold(reads, average_read_length, genome_size) -> int:
    """highTh of the fourth loop of ContigExtender::extendContigs (mergeContigs.cpp:43, :102), on the host: no context, no GPU"""
    out = C.c_int(0)
    rc = lib().sage2ov_extend_short_threshold(C.c_uint64(reads), C.c_uint64(average_read_length), C.c_uint64(genome_size), C.byref(out))
    if rc:
        raise Sage2ovError(rc, "extend_short_threshold")
    return int(out.value)


class Context:
    """One overlap-detection job on one GPU (sage2ov_ctx).  Method names follow include/sage2ov.h."""

    def __init__(self, min_overlap, device=-1, rank=0, world=1, host_threads=0, flags=0):
        self._h = C.c_void_p()
        cfg = Config(min_overlap, device, rank, world, host_threads, flags)
        rc = lib().sage2ov_ctx_create(C.byref(cfg), C.byref(self._h))
        if rc:
            raise Sage2ovError(rc, lib().sage2ov_last_error(None).decode())

    def close(self):
        if self._h:
            lib().sage2ov_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise Sage2ovError(rc, lib().sage2ov_last_error(self._h).decode())

    # ---- step 1
    def reads_add_ascii(self, bases: np.ndarray, offsets: np.ndarray):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self._chk(lib().sage2ov_reads_add_ascii(self._h, C.c_void_p(bases.ctypes.data), C.c_void_p(offsets.ctypes.data), C.c_uint64(len(offsets) - 1)))

    def reads_add_file(self, path1, path2=None):
        self._chk(lib().sage2ov_reads_add_file(self._h, path1.encode(), path2.encode() if path2 else None))

    def reads_add_list(self, path):
        self._chk(lib().sage2ov_reads_add_list(self._h, path.encode()))

    def reads_add_synth(self, p: SynthParams, genome: np.ndarray, first=0, n=None):
        n = p.n_reads - first if n is None else n
        self._chk(lib().sage2ov_reads_add_synth(self._h, C.byref(p), C.c_void_p(genome.ctypes.data), C.c_uint64(first), C.c_uint64(n)))

    def reads_organize(self):
        self._chk(lib().sage2ov_reads_organize(self._h))

    def reads_stats(self) -> ReadStats:
        s = ReadStats()
        self._chk(lib().sage2ov_reads_stats(self._h, C.byref(s)))
        return s

    def reads_export(self):
        s = self.reads_stats()
        n = s.unique_reads
        stride = (s.max_read_length + 3) // 4 + 1
        packed = np.zeros((n + 1, stride), dtype=np.uint8)
        length = np.zeros(n + 1, dtype=np.uint16)
        freq = np.zeros(n + 1, dtype=np.uint16)
        self._chk(lib().sage2ov_reads_export(self._h, C.c_void_p(packed.ctypes.data), C.c_uint64(stride), C.c_void_p(length.ctypes.data), C.c_void_p(freq.ctypes.data)))
        return packed, length, freq

    def reads_export_words(self):
        s = self.reads_stats()
        words = np.zeros((s.unique_reads + 1) * s.words_per_read, dtype=np.uint64)
        freq = np.zeros(s.unique_reads + 1, dtype=np.uint16)
        self._chk(lib().sage2ov_reads_export_words(self._h, C.c_void_p(words.ctypes.data), C.c_uint64(words.size), C.c_void_p(freq.ctypes.data)))
        return words, freq

    def reads_import_words(self, words, n_unique, words_per_read, max_read_length, freq, good_reads, total_bp):
        words = np.ascontiguousarray(words, dtype=np.uint64)
        freq = np.ascontiguousarray(freq, dtype=np.uint16)
        self._chk(lib().sage2ov_reads_import_words(self._h, C.c_void_p(words.ctypes.data), C.c_uint64(n_unique), C.c_uint32(words_per_read),
                                                   C.c_uint32(max_read_length), C.c_void_p(freq.ctypes.data), C.c_uint64(good_reads), C.c_uint64(total_bp)))

    def reads_save(self, path):
        self._chk(lib().sage2ov_reads_save(self._h, path.encode()))

    def reads_load(self, path):
        self._chk(lib().sage2ov_reads_load(self._h, path.encode()))

    def reads_set_totals(self, good_reads, total_bp):
        self._chk(lib().sage2ov_reads_set_totals(self._h, C.c_uint64(good_reads), C.c_uint64(total_bp)))

    def reads_find_ids(self, bases, offsets) -> np.ndarray:
        """ReadLoader::getIdOfRead for a batch: query r = bases[offsets[r]:offsets[r+1]] -> +id (the read as given is the stored, canonical form),
        -id (its reverse complement is) or 0 (not stored, or not a good read)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = max(len(offsets) - 1, 0)
        ids = np.zeros(n, dtype=np.int64)
        self._chk(lib().sage2ov_reads_find_ids(self._h, C.c_void_p(bases.ctypes.data), C.c_void_p(offsets.ctypes.data), C.c_uint64(n), C.c_void_p(ids.ctypes.data)))
        return ids

    def reads_find_stats(self) -> FindStats:
        s = FindStats()
        self._chk(lib().sage2ov_reads_find_stats_get(self._h, C.byref(s)))
        return s

    # ---- the mate-pair table (MatePair::mapMatePairs, matePair.cpp:125-239)
    def mates_add_ascii(self, bases, offsets, library):
        """processMatePairs for one array of reads: pairs (2j, 2j+1), a trailing odd read is dropped"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = max(len(offsets) - 1, 0)
        self._chk(lib().sage2ov_mates_add_ascii(self._h, C.c_void_p(bases.ctypes.data), C.c_void_p(offsets.ctypes.data), C.c_uint64(n), C.c_int(library)))

    def mates_add_file(self, path1, path2=None, library=1):
        self._chk(lib().sage2ov_mates_add_file(self._h, os.fsencode(path1), os.fsencode(path2) if path2 else None, C.c_int(library)))

    def mates_add_list(self, list_path):
        self._chk(lib().sage2ov_mates_add_list(self._h, os.fsencode(list_path)))

    def mates_count(self, library) -> int:
        n = C.c_uint64(0)
        self._chk(lib().sage2ov_mates_count(self._h, C.c_int(library), C.byref(n)))
        return int(n.value)

    def mates(self, library):
        """(entries, offsets): the library's entries (MATE_DTYPE) in ascending (from, to, type1, type2); the entries of read a are
        entries[offsets[a]:offsets[a + 1]], offsets[N + 1] is the entry count"""
        n = self.mates_count(library)
        out = np.zeros(n, dtype=MATE_DTYPE)
        offsets = np.zeros(self.reads_stats().unique_reads + 2, dtype=np.uint64)
        self._chk(lib().sage2ov_mates_export(self._h, C.c_int(library), C.c_void_p(out.ctypes.data), C.c_uint64(n), C.c_void_p(offsets.ctypes.data)))
        return out, offsets

    def mates_clear(self):
        self._chk(lib().sage2ov_mates_clear(self._h))

    def reads_pair_library(self, library):
        """0: pairing off (the default); 1 .. 127: every later reads_add_ascii / reads_add_file call is also one mates call for that library
        (reads_add_list: dataset i is library i), to be turned into the mate table by mates_from_reads() after reads_organize()"""
        self._chk(lib().sage2ov_reads_pair_library(self._h, C.c_int(library)))

    def mates_from_reads(self):
        """the mate table of the reads this context organised with pairing on: what the matching mates_add_* calls would add, without reading the
        input again or searching the read store; once per organised read set"""
        self._chk(lib().sage2ov_mates_from_reads(self._h))

    def mates_stats(self) -> MateStats:
        s = MateStats()
        self._chk(lib().sage2ov_mates_stats_get(self._h, C.byref(s)))
        return s

    # ---- MatePair::meanSdEstimation (matePair.cpp:244-569): reads on edges, flags, distances, insert sizes
    def mates_map_reads(self):
        """mapReadsToEdges + mapReadLocations over the resident step-4 graph; sets the flag of every mate entry present"""
        self._chk(lib().sage2ov_mates_map_reads(self._h))

    def read_edges(self):
        """(entries, locations, offsets): the read-to-edge table (READ_EDGE_DTYPE) in ascending (read, pair); the entries of read a are
        entries[offsets[a]:offsets[a + 1]]; entry e has locations[e.location : +n_forward] forward and the next n_reverse reverse"""
        ne, nl = C.c_uint64(0), C.c_uint64(0)
        self._chk(lib().sage2ov_mates_read_edges_count(self._h, C.byref(ne), C.byref(nl)))
        out = np.zeros(ne.value, dtype=READ_EDGE_DTYPE)
        loc = np.zeros(nl.value, dtype=np.int32)
        offsets = np.zeros(self.reads_stats().unique_reads + 2, dtype=np.uint64)
        self._chk(lib().sage2ov_mates_read_edges_export(self._h, C.c_void_p(out.ctypes.data), C.c_uint64(ne.value), C.c_void_p(loc.ctypes.data), C.c_uint64(nl.value),
                                                       C.c_void_p(offsets.ctypes.data)))
        return out, loc, offsets

    def mates_flags(self, library) -> np.ndarray:
        """MatePairInfo::flag of the library's entries, parallel to mates(library)"""
        out = np.zeros(self.mates_count(library), dtype=np.uint8)
        self._chk(lib().sage2ov_mates_flags_export(self._h, C.c_int(library), C.c_void_p(out.ctypes.data)))
        return out

    def mates_distances(self, library) -> np.ndarray:
        n = C.c_uint64(0)
        self._chk(lib().sage2ov_mates_distances_export(self._h, C.c_int(library), None, C.c_uint64(0), C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint32)
        self._chk(lib().sage2ov_mates_distances_export(self._h, C.c_int(library), C.c_void_p(out.ctypes.data), C.c_uint64(n.value), C.byref(n)))
        return out

    def mates_estimate(self):
        self._chk(lib().sage2ov_mates_estimate(self._h))

    def mates_insert(self, library) -> Insert:
        out = Insert()
        self._chk(lib().sage2ov_mates_insert_get(self._h, C.c_int(library), C.byref(out)))
        return out

    def mates_bounds(self):
        """(minimumUpperBoundOfInsert, maximumUpperBoundOfInsert)"""
        lo, hi = C.c_uint64(0), C.c_uint64(0)
        self._chk(lib().sage2ov_mates_bounds_get(self._h, C.byref(lo), C.byref(hi)))
        return int(lo.value), int(hi.value)

    def readmap_stats(self) -> ReadMapStats:
        s = ReadMapStats()
        self._chk(lib().sage2ov_readmap_stats_get(self._h, C.byref(s)))
        return s

    # ---- the sweep of ContigExtender::findMatepairSupports (mergeContigs.cpp:959-1110): flows, supports of (in, out) edge pairs at a node
    def graph_flows(self) -> np.ndarray:
        """the flows of the resident step-4 graph: two float32 per record pair (record, twin) in graph4_save's order"""
        s = SimplifyStats()
        n = 2 * s.edges if lib().sage2ov_simplify_stats_get(self._h, C.byref(s)) == 0 else 0          # (no graph: the export says what is missing)
        out = np.zeros(n, dtype=np.float32)
        self._chk(lib().sage2ov_graph_flow_export(self._h, C.c_void_p(out.ctypes.data), C.c_uint64(n)))
        return out

    def graph_set_flows(self, flows):
        flows = np.ascontiguousarray(flows, dtype=np.float32)
        self._chk(lib().sage2ov_graph_flow_import(self._h, C.c_void_p(flows.ctypes.data), C.c_uint64(len(flows))))

    # ---- step 5 around its solver (CopyCountEstimator: genome size, flow network, a solver's flows, P.graph5)
    def genome_size(self) -> int:
        n = C.c_uint64(0)
        self._chk(lib().sage2ov_genome_size_estimate(self._h, C.byref(n)))
        return int(n.value)

    def flow_network_build(self):
        self._chk(lib().sage2ov_flow_network_build(self._h))

    def flow_network(self) -> np.ndarray:
        """the arcs of the flow network (FLOW_ARC_DTYPE) in input.cs2's order, the 2 -> 1 arc first"""
        nodes, arcs = C.c_uint64(0), C.c_uint64(0)
        self._chk(lib().sage2ov_flow_network_count(self._h, C.byref(nodes), C.byref(arcs)))
        out = np.zeros(arcs.value, dtype=FLOW_ARC_DTYPE)
        self._chk(lib().sage2ov_flow_network_export(self._h, C.c_void_p(out.ctypes.data), C.c_uint64(arcs.value)))
        return out

    def flow_network_save(self, path):
        self._chk(lib().sage2ov_flow_network_save(self._h, os.fsencode(path)))

    def flow_apply(self, from_, to, flow):
        """the lines (from, to, flow) of a solver's output, in any order, onto the flows of the resident graph"""
        a = np.ascontiguousarray(from_, dtype=np.uint64); b = np.ascontiguousarray(to, dtype=np.uint64); f = np.ascontiguousarray(flow, dtype=np.uint64)
        if not (len(a) == len(b) == len(f)):
            raise ValueError("from, to and flow have one value per line")
        self._chk(lib().sage2ov_flow_solution_apply(self._h, C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), C.c_void_p(f.ctypes.data), C.c_uint64(len(a))))

    def flow_load(self, path):
        self._chk(lib().sage2ov_flow_solution_load(self._h, os.fsencode(path)))

    def graph5_save(self, path):
        self._chk(lib().sage2ov_graph5_save(self._h, os.fsencode(path)))

    # ---- step 5's solver (main_cs2): min-cost flow on the device
    def mcf_solve(self, n, arcs, max_rounds=0, wide=False):
        """solves the circulation over nodes 1..n with the arcs (MCF_ARC_DTYPE); returns (flow per arc, price per node in scaled units, McfStats).  A failed
        solve raises Sage2ovError; mcf_stats() still tells how far it got.  wide: 128-bit prices on the device; they come back as a list of Python integers"""
        a = np.ascontiguousarray(arcs, dtype=MCF_ARC_DTYPE)
        if wide:
            flow = np.zeros(len(a), dtype=np.int64); st = McfStats()
            words = np.zeros(2 * int(n), dtype=np.uint64) if int(n) < (1 << 28) else None      # (beyond 2^28 nodes no prices are fetched: [])
            self._chk(lib().sage2ov_mcf_solve_wide(self._h, C.c_uint64(int(n)), C.c_void_p(a.ctypes.data), C.c_uint64(len(a)), C.c_uint64(int(max_rounds)),
                                                   C.c_void_p(flow.ctypes.data), C.c_void_p(words.ctypes.data if words is not None else None), C.byref(st)))
            return flow, wide_prices(words), st
        flow = np.zeros(len(a), dtype=np.int64); price = np.zeros(int(n), dtype=np.int64); st = McfStats()
        self._chk(lib().sage2ov_mcf_solve(self._h, C.c_uint64(int(n)), C.c_void_p(a.ctypes.data), C.c_uint64(len(a)), C.c_uint64(int(max_rounds)),
                                          C.c_void_p(flow.ctypes.data), C.c_void_p(price.ctypes.data), C.byref(st)))
        return flow, price, st

    def flow_solve(self, max_rounds=0) -> McfStats:
        """solves the resident flow network; the solution stays on the device"""
        st = McfStats()
        self._chk(lib().sage2ov_flow_solve(self._h, C.c_uint64(int(max_rounds)), C.byref(st)))
        return st

    def flow_solution(self):
        """(flow per arc of flow_network(), price per network node in scaled units, scale) of the resident solution"""
        nodes, arcs, scale = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._chk(lib().sage2ov_flow_network_count(self._h, C.byref(nodes), C.byref(arcs)))
        flow = np.zeros(arcs.value, dtype=np.int64); price = np.zeros(nodes.value, dtype=np.int64)
        self._chk(lib().sage2ov_flow_solution_export(self._h, C.c_void_p(flow.ctypes.data), C.c_uint64(arcs.value), C.c_void_p(price.ctypes.data), C.c_uint64(nodes.value), C.byref(scale)))
        return flow, price, int(scale.value)

    def flow_solution_wide(self):
        """flow_solution() for a solution of either price width: the prices are a list of Python integers"""
        nodes, arcs, scale = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._chk(lib().sage2ov_flow_network_count(self._h, C.byref(nodes), C.byref(arcs)))
        flow = np.zeros(arcs.value, dtype=np.int64); words = np.zeros(2 * nodes.value, dtype=np.uint64)
        self._chk(lib().sage2ov_flow_solution_export_wide(self._h, C.c_void_p(flow.ctypes.data), C.c_uint64(arcs.value), C.c_void_p(words.ctypes.data), C.c_uint64(nodes.value), C.byref(scale)))
        return flow, wide_prices(words), int(scale.value)

    def flow_solution_save(self, path):
        self._chk(lib().sage2ov_flow_solution_save(self._h, os.fsencode(path)))

    def flow_commit(self):
        """the resident solution onto the flows of the graph, as flow_load of its file would"""
        self._chk(lib().sage2ov_flow_solution_commit(self._h))

    def copy_counts(self) -> int:
        """the whole of step 5: estimate, network, solve, commit; returns the genome size"""
        n = C.c_uint64(0)
        self._chk(lib().sage2ov_copy_counts(self._h, C.byref(n)))
        return int(n.value)

    def mcf_stats(self) -> McfStats:
        s = McfStats()
        self._chk(lib().sage2ov_mcf_stats_get(self._h, C.byref(s)))
        return s

    def mcf_hub_stats(self) -> dict:
        """the hub form in the last solve: the threshold in force (0: off), the entries of a tile, hub nodes, tiles, entries pushed along and relabels by the hub form"""
        out = (C.c_uint64 * 6)()
        self._chk(lib().sage2ov_mcf_hub_stats_get(self._h, out))
        return dict(zip(("hub_deg", "tile", "hubs", "tiles", "hub_pushes", "hub_relabels"), (int(x) for x in out)))

    def copycount_stats(self) -> CopyCountStats:
        s = CopyCountStats()
        self._chk(lib().sage2ov_copycount_stats_get(self._h, C.byref(s)))
        return s

    def mates_supports(self, min_support=2) -> np.ndarray:
        """the candidates with support >= min_support (SUPPORT_DTYPE) in ascending (node, pair_in, pair_out); 2 gives findMatepairSupports' list"""
        n = C.c_uint64(0)
        self._chk(lib().sage2ov_mates_supports_count(self._h, C.c_uint32(min_support), C.byref(n)))
        out = np.zeros(n.value, dtype=SUPPORT_DTYPE)
        self._chk(lib().sage2ov_mates_supports_export(self._h, C.c_uint32(min_support), C.c_void_p(out.ctypes.data), C.c_uint64(n.value)))
        return out

    def mates_supports_build(self):
        """builds the table now (mates_supports builds it when it is stale)"""
        self._chk(lib().sage2ov_mates_supports(self._h))

    def support_stats(self) -> SupportStats:
        s = SupportStats()
        self._chk(lib().sage2ov_support_stats_get(self._h, C.byref(s)))
        return s

    # ---- the first loop of ContigExtender::extendContigs (mergeContigs.cpp:47-60): merge rounds by mate-pair support on the resident graph
    def merge_pairs(self, first, second, type_of_merge=1) -> np.ndarray:
        """mergeEdgesAndUpdate for a batch of edge-disjoint merges.  first, second: per merge (pair ordinal in graph4_save's order, reversed) -- reversed 0 means the
        pair's record, 1 its twin; first enters the shared node, second leaves it.  Returns the merged mask (0: a merge the reference refuses)."""
        a = np.asarray(first, dtype=np.int64).reshape(-1, 2); b = np.asarray(second, dtype=np.int64).reshape(-1, 2)
        if len(a) != len(b):
            raise ValueError("one first and one second operand per merge")
        if len(a) and (a.min() < 0 or b.min() < 0 or max(a[:, 0].max(), b[:, 0].max()) >= 1 << 32):
            raise ValueError("pair ordinals are uint32")
        pa = np.ascontiguousarray(a[:, 0], dtype=np.uint32); ra = np.ascontiguousarray(a[:, 1] != 0, dtype=np.uint8)
        pb = np.ascontiguousarray(b[:, 0], dtype=np.uint32); rb = np.ascontiguousarray(b[:, 1] != 0, dtype=np.uint8)
        out = np.zeros(len(a), dtype=np.uint8)
        self._chk(lib().sage2ov_graph_merge_pairs(self._h, C.c_void_p(pa.ctypes.data), C.c_void_p(ra.ctypes.data), C.c_void_p(pb.ctypes.data), C.c_void_p(rb.ctypes.data),
                                                  C.c_uint64(len(a)), C.c_int(type_of_merge), C.c_void_p(out.ctypes.data)))
        return out

    def extend_round(self, high, low=1) -> int:
        """one findMatepairSupports(k, high): sweep, selection, merges; returns the number of merges"""
        n = C.c_uint64(0)
        self._chk(lib().sage2ov_extend_round(self._h, C.c_int(high), C.c_int(low), C.byref(n)))
        return int(n.value)

    def extend_by_supports(self, genome_size=0):
        """rounds until one merges nothing -> (rounds, merges)"""
        r, m = C.c_uint64(0), C.c_uint64(0)
        self._chk(lib().sage2ov_extend_by_supports(self._h, C.c_uint64(genome_size), C.byref(r), C.byref(m)))
        return int(r.value), int(m.value)

    def extend_merges(self) -> np.ndarray:
        """the merges of the last round (MERGE_DTYPE) in selection order"""
        n = C.c_uint64(0)
        self._chk(lib().sage2ov_extend_merges_count(self._h, C.byref(n)))
        out = np.zeros(n.value, dtype=MERGE_DTYPE)
        self._chk(lib().sage2ov_extend_merges_export(self._h, C.c_void_p(out.ctypes.data), C.c_uint64(n.value)))
        return out

    def extend_stats(self) -> ExtendStats:
        s = ExtendStats()
        self._chk(lib().sage2ov_extend_stats_get(self._h, C.byref(s)))
        return s

    def graph6_save(self, path):
        self._chk(lib().sage2ov_graph6_save(self._h, os.fsencode(path)))

    # ---- the second and third loop of extendContigs (mergeContigs.cpp:62-99): path supports and their merge rounds
    def path_supports(self, min_support=1) -> np.ndarray:
        """the rows with support >= min_support (PATH_SUPPORT_DTYPE) in ascending (node, a newest first, b newest first); built when stale"""
        n = C.c_uint64(0)
        self._chk(lib().sage2ov_path_supports_count(self._h, C.c_uint32(min_support), C.byref(n)))
        out = np.zeros(n.value, dtype=PATH_SUPPORT_DTYPE)
        self._chk(lib().sage2ov_path_supports_export(self._h, C.c_uint32(min_support), C.c_void_p(out.ctypes.data), C.c_uint64(n.value)))
        return out

    def path_supports_build(self):
        """builds the table now (path_supports builds it when it is stale)"""
        self._chk(lib().sage2ov_path_supports(self._h))

    def path_stats(self) -> PathStats:
        s = PathStats()
        self._chk(lib().sage2ov_path_stats_get(self._h, C.byref(s)))
        return s

    def extend_paths_round(self, high, low=1, variant=0) -> int:
        """one findPathSupports(high) (variant 0) or findPathSupportsNew(high) (1): sweep, selection, merges; returns the number of merges"""
        n = C.c_uint64(0)
        self._chk(lib().sage2ov_extend_paths_round(self._h, C.c_int(high), C.c_int(low), C.c_int(variant), C.byref(n)))
        return int(n.value)

    def extend_by_paths(self, genome_size=0, variant=0):
        """rounds until one merges no more than the stop value -> (rounds, merges)"""
        r, m = C.c_uint64(0), C.c_uint64(0)
        self._chk(lib().sage2ov_extend_by_paths(self._h, C.c_uint64(genome_size), C.c_int(variant), C.byref(r), C.byref(m)))
        return int(r.value), int(m.value)

    # ---- step 7, ScaffoldMaker::makeScaffolds (scaffolding.cpp:31-98): joins of edges that share no node, by the links below
    def join_pairs(self, first, second, gap):
        """mergeDisconnectedEdges for a batch of edge-disjoint joins.  first, second: per join (pair ordinal in graph4_save's order, reversed), as for merge_pairs;
        gap: one int per join.  Returns (overlap, how): per join the (forward list, twin list) values of stringOverlapSize (-2: equal end nodes) and of JOIN_*."""
        a = np.asarray(first, dtype=np.int64).reshape(-1, 2); b = np.asarray(second, dtype=np.int64).reshape(-1, 2); g = np.ascontiguousarray(gap, dtype=np.int32).reshape(-1)
        if not len(a) == len(b) == len(g):
            raise ValueError("one first operand, one second operand and one gap per join")
        if len(a) and (a.min() < 0 or b.min() < 0 or max(a[:, 0].max(), b[:, 0].max()) >= 1 << 32):
            raise ValueError("pair ordinals are uint32")
        pa = np.ascontiguousarray(a[:, 0], dtype=np.uint32); ra = np.ascontiguousarray(a[:, 1] != 0, dtype=np.uint8)
        pb = np.ascontiguousarray(b[:, 0], dtype=np.uint32); rb = np.ascontiguousarray(b[:, 1] != 0, dtype=np.uint8)
        ov = np.zeros((len(a), 2), dtype=np.int32); how = np.zeros((len(a), 2), dtype=np.uint8)
        self._chk(lib().sage2ov_graph_join_pairs(self._h, C.c_void_p(pa.ctypes.data), C.c_void_p(ra.ctypes.data), C.c_void_p(pb.ctypes.data), C.c_void_p(rb.ctypes.data),
                                                 C.c_void_p(g.ctypes.data), C.c_uint64(len(a)), C.c_void_p(ov.ctypes.data), C.c_void_p(how.ctypes.data)))
        return ov, how

    def scaffold_round(self, high, flag=1, small=False) -> int:
        """one mergeFinal(k, high, flag) (small: mergeFinalSmall): sweep, selection, joins; returns the number of joins"""
        n = C.c_uint64(0)
        self._chk(lib().sage2ov_scaffold_round(self._h, C.c_int(high), C.c_int(flag), C.c_int(1 if small else 0), C.byref(n)))
        return int(n.value)

    def scaffold(self, genome_size=0):
        """the five loops of makeScaffolds -> (rounds, joins)"""
        r, m = C.c_uint64(0), C.c_uint64(0)
        self._chk(lib().sage2ov_scaffold(self._h, C.c_uint64(genome_size), C.byref(r), C.byref(m)))
        return int(r.value), int(m.value)

    def scaffold_merges(self) -> np.ndarray:
        """the joins of the last round (JOIN_DTYPE) in selection order"""
        n = C.c_uint64(0)
        self._chk(lib().sage2ov_scaffold_merges_count(self._h, C.byref(n)))
        out = np.zeros(n.value, dtype=JOIN_DTYPE)
        self._chk(lib().sage2ov_scaffold_merges_export(self._h, C.c_void_p(out.ctypes.data), C.c_uint64(n.value)))
        return out

    def scaffold_stats(self) -> ScaffoldStats:
        s = ScaffoldStats()
        self._chk(lib().sage2ov_scaffold_stats_get(self._h, C.byref(s)))
        return s

    # ---- the fourth loop of extendContigs (mergeContigs.cpp:101-110): mergeShortOverlaps, joins of contigs whose mates give a summed gap of at most 0
    extend_short_threshold = staticmethod(extend_short_threshold)

    def extend_short_round(self, high) -> int:
        """one mergeShortOverlaps(k, high): sweep, selection, joins; returns the number of joins"""
        n = C.c_uint64(0)
        self._chk(lib().sage2ov_extend_short_round(self._h, C.c_int(high), C.byref(n)))
        return int(n.value)

    def extend_by_short_overlaps(self, genome_size=0):
        """rounds until one joins nothing -> (rounds, joins)"""
        r, m = C.c_uint64(0), C.c_uint64(0)
        self._chk(lib().sage2ov_extend_by_short_overlaps(self._h, C.c_uint64(genome_size), C.byref(r), C.byref(m)))
        return int(r.value), int(m.value)

    def extend_contigs(self, genome_size=0):
        """the four loops of extendContigs in the reference's order -> ([rounds of each loop], [merges of each loop])"""
        r, m = (C.c_uint64 * 4)(), (C.c_uint64 * 4)()
        self._chk(lib().sage2ov_extend_contigs(self._h, C.c_uint64(genome_size), r, m))
        return [int(x) for x in r], [int(x) for x in m]

    def extend_short_merges(self) -> np.ndarray:
        """the joins of the last short-overlap round (JOIN_DTYPE) in selection order"""
        n = C.c_uint64(0)
        self._chk(lib().sage2ov_extend_short_merges_count(self._h, C.byref(n)))
        out = np.zeros(n.value, dtype=JOIN_DTYPE)
        self._chk(lib().sage2ov_extend_short_merges_export(self._h, C.c_void_p(out.ctypes.data), C.c_uint64(n.value)))
        return out

    def extend_short_stats(self) -> ScaffoldStats:
        """the counters of the short-overlap rounds; the scaffold's own (scaffold_stats) do not see them"""
        s = ScaffoldStats()
        self._chk(lib().sage2ov_extend_short_stats_get(self._h, C.byref(s)))
        return s

    # ---- the sweep that opens ScaffoldMaker::mergeFinal / mergeFinalSmall (scaffolding.cpp:786-935, :981-1130): support and gap of half-edge pairs linked by mates
    def links(self, mode=0, min_support=1) -> np.ndarray:
        """the rows (LINK_DTYPE) that pass the filter (LINKS_ALL / LINKS_FINAL / LINKS_SMALL) with support >= min_support, in ascending
        (pair_a, second_a, pair_b, second_b)"""
        n = C.c_uint64(0)
        self._chk(lib().sage2ov_links_count(self._h, C.c_uint32(mode), C.c_uint32(min_support), C.byref(n)))
        out = np.zeros(n.value, dtype=LINK_DTYPE)
        self._chk(lib().sage2ov_links_export(self._h, C.c_uint32(mode), C.c_uint32(min_support), C.c_void_p(out.ctypes.data), C.c_uint64(n.value)))
        return out

    def links_gap_sums(self, mode=0, min_support=1) -> np.ndarray:
        """the int32 gapSum of the rows links(mode, min_support) returns, in the same order (a row's gap is gapSum / support, truncated towards zero)"""
        n = C.c_uint64(0)
        self._chk(lib().sage2ov_links_count(self._h, C.c_uint32(mode), C.c_uint32(min_support), C.byref(n)))
        out = np.zeros(n.value, dtype=np.int32)
        self._chk(lib().sage2ov_links_gap_sums(self._h, C.c_uint32(mode), C.c_uint32(min_support), C.c_void_p(out.ctypes.data), C.c_uint64(n.value)))
        return out

    def links_build(self):
        """builds the table now (links builds it when it is stale)"""
        self._chk(lib().sage2ov_links(self._h))

    def link_stats(self) -> LinkStats:
        s = LinkStats()
        self._chk(lib().sage2ov_link_stats_get(self._h, C.byref(s)))
        return s

    # ---- OverlapGraph::printGraph / saveContigsToFile (overlapGraph.cpp:507-784): the contigs of the resident step-4 graph
    def contigs_build(self, threshold=0, genome_size=0):
        """builds the table (the calls below build it when it is stale, with the last threshold and genome size); threshold 0: the reference's contigLengthThreshold"""
        self._chk(lib().sage2ov_contigs_build(self._h, C.c_uint32(threshold), C.c_uint64(genome_size)))

    def contigs_count(self):
        """(rows, summed string length)"""
        n, t = C.c_uint64(0), C.c_uint64(0)
        self._chk(lib().sage2ov_contigs_count(self._h, C.byref(n), C.byref(t)))
        return n.value, t.value

    def contigs(self) -> np.ndarray:
        """the rows (CONTIG_DTYPE) in table order: edge length descending, then `from` ascending, then newest first"""
        n = self.contigs_count()[0]
        out = np.zeros(n, dtype=CONTIG_DTYPE)
        self._chk(lib().sage2ov_contigs_export(self._h, C.c_void_p(out.ctypes.data), C.c_uint64(n)))
        return out

    def contig_sequences(self, first=0, count=None, string_lengths=None):
        """(uint8 array of the whole strings of rows [first, first + count) one after the other, count + 1 uint64 offsets); the device buffer is sized by the range.
        string_lengths: the table's column, when the caller has it already"""
        if string_lengths is None:
            string_lengths = self.contigs()["string_length"]
        count = len(string_lengths) - first if count is None else count
        need = int(np.asarray(string_lengths[first:first + count], dtype=np.uint64).sum())
        out = np.zeros(need, dtype=np.uint8); off = np.zeros(count + 1, dtype=np.uint64)
        self._chk(lib().sage2ov_contigs_sequences(self._h, C.c_uint64(first), C.c_uint64(count), C.c_void_p(out.ctypes.data), C.c_uint64(need), C.c_void_p(off.ctypes.data)))
        return out, off

    def contigs_save(self, path, scaffold=False):
        """P_contig.fasta as saveContigsToFile writes it (scaffold: P_scaffold.fasta's record names)"""
        self._chk(lib().sage2ov_contigs_save(self._h, path.encode(), C.c_int(1 if scaffold else 0)))

    def contig_stats(self) -> ContigStats:
        s = ContigStats()
        self._chk(lib().sage2ov_contig_stats_get(self._h, C.byref(s)))
        return s

    # ---- step 2
    def index_build(self):
        self._chk(lib().sage2ov_index_build(self._h))

    def index_stats(self) -> IndexStats:
        s = IndexStats()
        self._chk(lib().sage2ov_index_stats_get(self._h, C.byref(s)))
        return s

    def hashtable_save(self, path):
        self._chk(lib().sage2ov_hashtable_save(self._h, path.encode()))

    def options_reload(self):
        """re-read the SAGE2OV_* environment switches (the library reads them once, when the context is created)"""
        self._chk(lib().sage2ov_options_reload(self._h))

    def index_lookup(self, v0, v1, cap=128):
        key = (C.c_uint64 * 2)(v0, v1)
        ent = (C.c_uint64 * cap)()
        cnt = C.c_uint32()
        self._chk(lib().sage2ov_index_lookup(self._h, key, ent, C.c_uint32(cap), C.byref(cnt)))
        return [int(ent[i]) for i in range(min(cnt.value, cap))], cnt.value

    # ---- step 3
    def overlap_initial(self):
        self._chk(lib().sage2ov_overlap_initial(self._h))

    def overlap_reduce(self):
        self._chk(lib().sage2ov_overlap_reduce(self._h))

    def overlap_convert(self):
        self._chk(lib().sage2ov_overlap_convert(self._h))

    def run_steps23(self):
        self._chk(lib().sage2ov_run_steps23(self._h))

    def overlap_stats(self) -> OverlapStats:
        s = OverlapStats()
        self._chk(lib().sage2ov_overlap_stats_get(self._h, C.byref(s)))
        return s

    def overlap_export_initial(self):
        n = self.reads_stats().unique_reads
        right = np.zeros(n + 1, dtype=np.uint64)
        left = np.zeros(n + 1, dtype=np.uint64)
        status = np.zeros(n + 1, dtype=np.uint8)
        conn = np.zeros(n + 1, dtype=np.uint32)
        self._chk(lib().sage2ov_overlap_export_initial(self._h, C.c_void_p(right.ctypes.data), C.c_void_p(left.ctypes.data),
                                                       C.c_void_p(status.ctypes.data), C.c_void_p(conn.ctypes.data)))
        return right, left, status, conn

    def edges(self) -> np.ndarray:
        n = C.c_uint64()
        self._chk(lib().sage2ov_edges_count(self._h, C.byref(n)))
        out = np.zeros(n.value, dtype=EDGE_DTYPE)
        if n.value:
            self._chk(lib().sage2ov_edges_export(self._h, C.c_void_p(out.ctypes.data), C.c_uint64(n.value)))
        return out

    def edges_import(self, edges: np.ndarray):
        edges = np.ascontiguousarray(edges, dtype=EDGE_DTYPE)
        self._chk(lib().sage2ov_edges_import(self._h, C.c_void_p(edges.ctypes.data), C.c_uint64(len(edges))))

    def graph_load(self, path):
        self._chk(lib().sage2ov_graph_load(self._h, path.encode()))

    def graph_load_composite(self, path):
        """loadOverlapGraphFromFile for a graph with composite edges (P.graph4 / graph5 / graph6)"""
        self._chk(lib().sage2ov_graph_load_composite(self._h, os.fsencode(path)))

    def graph_save(self, path):
        self._chk(lib().sage2ov_graph_save(self._h, path.encode()))

    # ---- step 4
    def graph_simplify(self):
        self._chk(lib().sage2ov_graph_simplify(self._h))

    def simplify_stats(self) -> SimplifyStats:
        s = SimplifyStats()
        self._chk(lib().sage2ov_simplify_stats_get(self._h, C.byref(s)))
        return s

    def graph4_save(self, path):
        self._chk(lib().sage2ov_graph4_save(self._h, path.encode()))

    def timings(self) -> Timings:
        t = Timings()
        self._chk(lib().sage2ov_timings_get(self._h, C.byref(t)))
        return t

    def probe_run_stats(self):
        """run mode of the last probe pass: (reads answered off the ring, steps, of those reads: records with a lane per read, such steps)"""
        out = (C.c_uint64 * 4)()
        self._chk(lib().sage2ov_probe_run_stats_get(self._h, out))
        return tuple(int(v) for v in out)

    REDUCE_STATS = ("form", "unresolved", "lists_over_128", "lists_over_512", "shortcut_lists", "shortcut_reads", "removed", "potential_over_1024", "slices")

    def reduce_stats(self):
        """which way the last reduce phase went, as a dict over REDUCE_STATS (form: 0 nothing unresolved, 1 symmetric device, 2 ranked device, 3 serial replay on the host)"""
        out = (C.c_uint64 * len(self.REDUCE_STATS))()
        self._chk(lib().sage2ov_reduce_stats_get(self._h, out))
        return dict(zip(self.REDUCE_STATS, (int(v) for v in out)))

    def debug_all_hits(self):
        n = C.c_uint64()
        self._chk(lib().sage2ov_debug_all_hits(self._h, None, C.c_uint64(0), C.byref(n)))
        out = np.zeros((n.value, 5), dtype=np.uint32)
        self._chk(lib().sage2ov_debug_all_hits(self._h, C.c_void_p(out.ctypes.data), C.c_uint64(n.value), C.byref(n)))
        return out

    def timings_reset(self):
        self._chk(lib().sage2ov_timings_reset(self._h))

    def stream(self):
        return lib().sage2ov_stream(self._h)

    def debug_meminfo(self):
        """{free, total, lowest free seen by the library, workspace arena bytes} of the context's GPU"""
        o = (C.c_uint64 * 4)()
        self._chk(lib().sage2ov_debug_meminfo(self._h, o))
        return dict(free=o[0], total=o[1], lowest_free=o[2], arena=o[3])

    # ---- multi-GPU exchange points
    def shard_range(self):
        lo, hi = C.c_uint64(), C.c_uint64()
        self._chk(lib().sage2ov_shard_range(self._h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def overlap_probe_shard(self):
        self._chk(lib().sage2ov_overlap_probe_shard(self._h))

    def shard_export_records(self, dev_ptr, max_reads):
        self._chk(lib().sage2ov_shard_export_records(self._h, C.c_void_p(dev_ptr), C.c_uint64(max_reads)))

    def shard_import_records(self, dev_ptr, first_id, n_reads):
        self._chk(lib().sage2ov_shard_import_records(self._h, C.c_void_p(dev_ptr), C.c_uint64(first_id), C.c_uint64(n_reads)))

    def overlap_reciprocal(self):
        self._chk(lib().sage2ov_overlap_reciprocal(self._h))

    def shard_flags_bytes(self):
        b = C.c_uint64()
        self._chk(lib().sage2ov_shard_flags_bytes(self._h, C.byref(b)))
        return b.value

    def shard_export_flags(self, dev_ptr):
        self._chk(lib().sage2ov_shard_export_flags(self._h, C.c_void_p(dev_ptr)))

    def shard_import_flags(self, dev_ptr):
        self._chk(lib().sage2ov_shard_import_flags(self._h, C.c_void_p(dev_ptr)))

    def shard_edges_count(self):
        n = C.c_uint64()
        self._chk(lib().sage2ov_shard_edges_count(self._h, C.byref(n)))
        return n.value

    def shard_edges_export(self, dev_ptr, cap):
        self._chk(lib().sage2ov_shard_edges_export(self._h, C.c_void_p(dev_ptr), C.c_uint64(cap)))

    def shard_edges_set(self, dev_ptr, n):
        self._chk(lib().sage2ov_shard_edges_set(self._h, C.c_void_p(dev_ptr), C.c_uint64(n)))

    # sharded reduce phase: this rank's survivor bucket (count, removals of its share), export, and the concatenation of all ranks' buckets back in
    def shard_survivors_count(self):
        n, rem = C.c_uint64(), C.c_uint64()
        self._chk(lib().sage2ov_shard_survivors_count(self._h, C.byref(n), C.byref(rem)))
        return n.value, rem.value

    def shard_survivors_export(self, dev_ptr, cap):
        self._chk(lib().sage2ov_shard_survivors_export(self._h, C.c_void_p(dev_ptr), C.c_uint64(cap)))

    def shard_survivors_set(self, dev_ptr, n_total, removed_total):
        self._chk(lib().sage2ov_shard_survivors_set(self._h, C.c_void_p(dev_ptr), C.c_uint64(n_total), C.c_uint64(removed_total)))
