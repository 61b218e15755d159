"""ctypes binding of the C ABI (include/megalania_hip.h) and of the C host library
(megalania_amd/host/mgl_host.h).  Thin: argument marshalling and error translation only.

There is deliberately no CPU fallback: if libmegalania_hip.so is missing, cannot be loaded,
or finds no GPU, every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import enum
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HIP_SO = os.path.join(HERE, "_build", "libmegalania_hip.so")
HOST_SO = os.environ.get("MGL_HOST_SO") or os.path.join(HERE, "_build", "libmegalania_host.so")  # the override: a sanitizer build (tests/test_sanitizers.py)

# lzma_packet.h:13-17 layout
PACKET = np.dtype([("type", "u1"), ("dist", "u4"), ("len", "u2")], align=True)
DIFF = np.dtype([("position", "u4"), ("old", PACKET), ("new", PACKET)], align=True)
assert PACKET.itemsize == 12 and DIFF.itemsize == 28

LITERAL, MATCH, SHORT_REP, LONG_REP = 1, 2, 3, 4
INVALID_COST = (1 << 64) - 1
F_TIMING = 1
F_FULLWALK = 2
F_PROFILE = 4
F_NO_SNAPSHOTS = 8
F_SERIAL_BUILD = 16
F_POSITION_TARGETS = 32
ACCEPT_AUTO, ACCEPT_SINGLE, ACCEPT_BULK = 0, 1, 2
MF_NEAREST, MF_FRONTIER = 0, 1

HIP_SYMBOLS = [
    "mgl_version", "mgl_last_error", "mgl_device_count", "mgl_sa_create", "mgl_sa_destroy", "mgl_sa_begin_epoch",
    "mgl_sa_set_slab", "mgl_sa_seed_greedy", "mgl_sa_seed_optimal", "mgl_optimal_pass", "mgl_optimal_prices", "mgl_sa_seed_adaptive", "mgl_adaptive_pass", "mgl_sa_seed_sweep", "mgl_sa_set_match_finder", "mgl_match_frontier", "mgl_sa_set_temperature", "mgl_sa_set_accept_mode", "mgl_sa_step_modes", "mgl_sa_set_best", "mgl_sa_run", "mgl_sa_current", "mgl_sa_best", "mgl_cost_slab", "mgl_final_state", "mgl_top_k",
    "mgl_substrings", "mgl_neighbours", "mgl_rng_draw_at", "mgl_debug_dump", "mgl_debug_set",
    "mgl_comm_unique_id", "mgl_comm_init", "mgl_comm_init_shm", "mgl_comm_min_u64", "mgl_comm_destroy", "mgl_comm_rank", "mgl_comm_world", "mgl_sa_exchange_best",
    "mgl_sa_best_packed", "mgl_sa_adopt_best_packed", "mgl_props_sweep", "mgl_parse_sweep_props",
    "mgl_crossover", "mgl_sa_cross_best", "mgl_sa_exchange_cross",
    "mgl_comm_allgather_u64", "mgl_slab_hash", "mgl_sa_exchange_cross_all",
    "mgl_sa_set_focus", "mgl_sa_focus", "mgl_focus_slice", "mgl_cost_map",
    "mgl_sa_set_target_weights", "mgl_sa_weight_targets_by_cost", "mgl_sa_target_weights", "mgl_weight_value",
    "mgl_cost_map_live", "mgl_sa_set_live_weights", "mgl_sa_live_weights",
    "mgl_segment_cuts", "mgl_props_sweep_spans", "mgl_segment_partition", "mgl_sa_segment_props",
    "mgl_segment_reparse",
]
LW_SINGLE_ONLY = 1
HOST_SYMBOLS = [
    "mgl_lzma_state_init", "mgl_lzma_state_free", "mgl_lzma_encode_packet", "mgl_lzma_encode_header",
    "mgl_range_encoder_new", "mgl_range_encoder_free", "mgl_perplexity_encoder_new", "mgl_file_output_new",
    "mgl_memory_output_new", "mgl_emit_stream", "mgl_stream_info_read", "mgl_stream_import",
    "mgl_emit_stream_dict", "mgl_bcj_x86", "mgl_emit_xz", "mgl_stream_info_read_x", "mgl_host_cost_map",
    "mgl_host_segment_cost", "mgl_host_segment_packets", "mgl_emit_xz_segments",
]
# segment props (include/megalania_hip.h): most cuts, the .xz writer's bound for one further chunk in cost units, default grain
SEG_MAX_CUTS = 17
SEG_OVERHEAD = 11 * 16384
SEG_DEFAULT_GRAIN = 65536


def span_index(i: int, j: int, m: int) -> int:
    """row of span (i, j), i < j <= m, in a props_sweep_spans table over m + 1 cuts"""
    return i * m - i * (i - 1) // 2 + (j - i - 1)
IMPORT_CLIP_WINDOW = 1
IMPORT_X86 = 2
FILTER_NONE, FILTER_X86 = 0, 4
# the lc/lp/pb triples mgl_sa_create accepts, in the order mgl_props_sweep reports them
PROPS_TRIPLES = [(lc, lp, pb) for lc in range(5) for lp in range(5 - lc) for pb in range(5)]


def best_props(costs):
    """The cheapest triple of a props_sweep table; among equals the first in canonical order (0/0/0 beats 1/0/0 on text)."""
    costs = [int(c) for c in costs]
    assert len(costs) == len(PROPS_TRIPLES)
    return PROPS_TRIPLES[costs.index(min(costs))]
CONTAINER_LZMA, CONTAINER_XZ = 1, 2


def _header_enum(name: str, prefix: str):
    """(NAME, value) of every enumerator of `enum name` in include/megalania_hip.h, the one place they are kept"""
    text = open(os.path.join(HERE, "..", "include", "megalania_hip.h")).read()
    body = re.search(r"enum %s \{(.*?)\n\};" % name, text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    pairs = re.findall(r"\b%s([A-Z0-9_]+) = (?:(\d+)|\(1u << (\d+)\))" % prefix, body)
    return [(n, int(v) if v else 1 << int(k)) for n, v, k in pairs]


def _dump_members():
    """an index family (X_BASE = b, the exact-length orders D = 2..7) becomes X_D2 .. X_D7 = b .. b + 5"""
    for n, v in _header_enum("mgl_dump_selector", "MGL_DUMP_"):
        if n.endswith("_BASE"):
            yield from ((f"{n[:-5]}_D{d}", v + d - 2) for d in range(2, 8))
        else:
            yield n, v


DUMP = enum.IntEnum("DUMP", list(_dump_members()))                               # mgl_debug_dump selectors
KEY = enum.IntEnum("KEY", _header_enum("mgl_debug_key", "MGL_KEY_"))             # mgl_debug_set keys
LIM = enum.IntEnum("LIM", [p for p in _header_enum("mgl_accept_limit", "MGL_LIM_") if p[0] != "COUNT"])  # limit ids of KEY.LIMIT
GU = enum.IntFlag("GU", _header_enum("mgl_giveup_site", "MGL_GU_"))              # give-up sites, the bits of DUMP.GIVEUP_SITES

# BatchHdr::status, from the #defines of csrc/mgl_words.h
BATCH = enum.IntEnum("BATCH", [(n, int(v)) for n, v in re.findall(
    r"#define MGL_BATCH_(NONE|BEGAN|REBUILD|DONE) (\d+)u", open(os.path.join(HERE, "csrc", "mgl_words.h")).read())])

# csrc/mgl_words.h, field for field (tests/test_debug_words_cpu.py compares them with what the C compiler lays out)
_u4 = lambda *names: np.dtype([(n, "u4") if isinstance(n, str) else n for n in names])
BATCH_HDR = _u4("status", "clusters", "n_ins", "n_rem", "failed", "journal", "unused6", "acceptable", "runs", "force_early",
                "touched", "unused11", "force_reached", "force_late", "unused14", "unused15")
BATCH_ACC = np.dtype([(n, "i8") for n in ("cost", "direct", "packets", "pad")])
APPLY_HDR = _u4("n_ins", "n_rem", "n_tctx", "first_pos", "jobs_b", "jobs_c", "span_used", "scratch_used", ("stage_cycles", "u4", 5),
                "walk_cycles0", "walk_cycles1", "walk_cycles2")
PB_ACC = np.dtype([("cost", "u8"), ("packets", "u8"), ("ctx_state", "u8"), ("dists", "u8", 4), ("redone", "u8"), ("left", "u8")])
STEP_COUNTS = _u4("second_pass", "last_resort", "spill_slots", "repair_picks", "unused4", "cancelled", "unused6", "unused7")
PICKSTATE = _u4(("state", "u4", 7), "mutated")  # word 7 = 1: the pick half took the grow/shrink mutation
# element type of what each selector hands out; DUMP.PBUILD_TOTALS stops before PbAcc's last field
DUMP_DTYPE = {d: np.dtype("u4") for d in DUMP}
DUMP_DTYPE.update({
    DUMP.CHAIN_EV: np.dtype("u2"), DUMP.ONWALK: np.dtype("u8"), DUMP.SPECIAL: np.dtype("u8"), DUMP.CHECKPOINTS: np.dtype("u2"),
    DUMP.PHASE_CYCLES: np.dtype("u8"), DUMP.STEP_COUNTS: STEP_COUNTS, DUMP.PBUILD_TOTALS: np.dtype([(n, PB_ACC[n]) for n in PB_ACC.names if n != "left"]),
    DUMP.APPLY_HDR: APPLY_HDR, DUMP.CONTROL: np.dtype("u1"), DUMP.QUAD_NEXT: np.dtype("u2"), DUMP.COSTS: np.dtype("u8"),
    DUMP.PICK_HINTS: np.dtype("u1"), DUMP.PICKSTATE: PICKSTATE, DUMP.OCT_NEXT8: np.dtype("u8"), DUMP.HEX_NEXT8: np.dtype("u8"),
    DUMP.BATCH_COUNTS: np.dtype("u8"), DUMP.BATCH_HDR: BATCH_HDR, DUMP.BATCH_ACC: BATCH_ACC, DUMP.ALLOCATIONS: np.dtype("u8"),
    **{DUMP[f"XNEXT_D{d}"]: np.dtype("u1") for d in range(2, 8)},
})


class MglError(RuntimeError):
    """rc: the MGL_E* code where one is known; error / error_pos: a stream import's first problem."""

    def __init__(self, msg, rc=None, error=None, error_pos=None):
        super().__init__(msg)
        self.rc, self.error, self.error_pos = rc, error, error_pos


class Properties(C.Structure):
    _fields_ = [("lc", C.c_uint8), ("lp", C.c_uint8), ("pb", C.c_uint8)]


class Config(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("neighbours_per_step", C.c_uint32), ("top_k", C.c_uint32),
                ("dict_limit", C.c_uint32), ("max_bucket_scan", C.c_uint32), ("iters_per_epoch", C.c_uint64),
                ("device", C.c_int32), ("flags", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("steps", C.c_uint64), ("evaluations", C.c_uint64), ("failed", C.c_uint64), ("accepted", C.c_uint64),
                ("improved", C.c_uint64), ("current_cost", C.c_uint64), ("best_cost", C.c_uint64),
                ("packets", C.c_uint64), ("packets_evaluated", C.c_uint64), ("gpu_ms_total", C.c_double),
                ("gpu_ms_neighbours", C.c_double), ("gpu_ms_rebuild", C.c_double), ("neighbour_launches", C.c_uint64),
                ("full_rebuilds", C.c_uint64), ("fallback_neighbours", C.c_uint64), ("second_pass_neighbours", C.c_uint64),
                ("bulk_steps", C.c_uint64), ("dropped_neighbours", C.c_uint64), ("improving_neighbours", C.c_uint64),
                ("bulk_rollbacks", C.c_uint64), ("bulk_double_writes", C.c_uint64),
                ("gpu_ms_sim", C.c_double), ("sim_launches", C.c_uint64), ("sim_bytes_counted", C.c_uint64)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


OPT_MAX_PASSES = 16


class OptimalConfig(C.Structure):
    _fields_ = [("passes", C.c_uint32), ("cand", C.c_uint32), ("chunk", C.c_uint32)]


class OptimalStats(C.Structure):
    _fields_ = [("passes", C.c_uint32), ("best_pass", C.c_uint32), ("greedy_cost", C.c_uint64),
                ("cost", C.c_uint64 * OPT_MAX_PASSES), ("objective", C.c_uint64 * OPT_MAX_PASSES),
                ("ms", C.c_double * OPT_MAX_PASSES)]


class AdaptiveConfig(C.Structure):
    _fields_ = [("passes", C.c_uint32), ("cand", C.c_uint32), ("chunk", C.c_uint32), ("segment", C.c_uint32),
                ("ahead", C.c_uint32), ("from_current", C.c_uint32)]


class ParseVariant(C.Structure):
    _fields_ = [("finder", C.c_uint32), ("cand", C.c_uint32), ("segment", C.c_uint32), ("ahead", C.c_uint32)]


class ParseSweepConfig(C.Structure):
    _fields_ = [("passes", C.c_uint32), ("chunk", C.c_uint32), ("depth", C.c_uint32), ("from_current", C.c_uint32)]


# the CLI's --parse-sweep grid (host/main.c: sweep_grid), (finder, cand, segment, ahead); index 0 is the library's default
DEFAULT_SWEEP = [(f, 16, s, a) for f in (MF_NEAREST, MF_FRONTIER) for s in (64, 32, 128, 256) for a in (128, 273)]


class PropsCost(C.Structure):
    _fields_ = [("props", Properties), ("cost", C.c_uint64)]


# mgl_cost_report: the coders a coded bit can belong to (MGL_CC_*) and the packet types, in table order
CC_KIND, CC_LITERAL, CC_LENGTH, CC_REP_LENGTH, CC_DISTANCE, CC_DIRECT = range(6)
COST_CLASSES = ["kind", "literal", "length", "rep_length", "distance", "direct"]
PACKET_TYPES = ["literal", "match", "short_rep", "long_rep"]


class CostReport(C.Structure):
    _fields_ = [("total", C.c_uint64), ("packets", C.c_uint64), ("class_cost", C.c_uint64 * 6), ("class_bits", C.c_uint64 * 6),
                ("type_cost", C.c_uint64 * 4), ("type_packets", C.c_uint64 * 4), ("type_bytes", C.c_uint64 * 4),
                ("gpu_ms", C.c_double)]

    def asdict(self, device: bool):
        d = dict(total=self.total, packets=self.packets, class_cost=list(self.class_cost), class_bits=list(self.class_bits),
                 type_cost=list(self.type_cost), type_packets=list(self.type_packets), type_bytes=list(self.type_bytes))
        if device:
            d["gpu_ms"] = self.gpu_ms
        return d


class Segment(C.Structure):
    _fields_ = [("lo", C.c_uint64), ("hi", C.c_uint64), ("props", Properties), ("cost", C.c_uint64)]

    def asdict(self):
        return dict(lo=self.lo, hi=self.hi, props=(self.props.lc, self.props.lp, self.props.pb), cost=self.cost)


class SegmentParseStats(C.Structure):
    _fields_ = [("passes", C.c_uint32), ("best_pass", C.c_uint32), ("start_cost", C.c_uint64), ("final_cost", C.c_uint64),
                ("pass_cost", C.c_uint64 * OPT_MAX_PASSES), ("objective", C.c_uint64 * OPT_MAX_PASSES)]

    def asdict(self):
        k = self.passes
        return dict(passes=k, best_pass=None if self.best_pass == 0xFFFFFFFF else self.best_pass, start_cost=self.start_cost,
                    final_cost=self.final_cost, pass_cost=list(self.pass_cost[:k]), objective=list(self.objective[:k]))


def _segments(segs):
    """dicts (lo, hi, props[, cost]) or Segment instances as a C array"""
    arr = (Segment * max(len(segs), 1))()
    for k, s in enumerate(segs):
        arr[k] = s if isinstance(s, Segment) else Segment(s["lo"], s["hi"], Properties(*s["props"]), s.get("cost", 0))
    return arr


class LiveWeightsConfig(C.Structure):
    _fields_ = [("every", C.c_uint32), ("floor", C.c_uint32), ("floor_mean", C.c_uint32), ("flags", C.c_uint32)]


class LiveWeightsStats(C.Structure):
    _fields_ = [("refreshes", C.c_uint64), ("skipped", C.c_uint64), ("last_gstep", C.c_uint64), ("last_total", C.c_uint64),
                ("gpu_ms", C.c_double)]


XO_MAX_PARENTS = 8


class CrossStats(C.Structure):
    _fields_ = [("parents", C.c_uint32), ("grain", C.c_uint32), ("parent_cost", C.c_uint64 * XO_MAX_PARENTS),
                ("child_cost", C.c_uint64), ("predicted", C.c_uint64), ("boundaries", C.c_uint64),
                ("regions_from", C.c_uint64 * XO_MAX_PARENTS), ("adopted", C.c_uint32), ("gpu_ms", C.c_double)]

    def asdict(self):
        k = self.parents
        return dict(parents=k, grain=self.grain, parent_cost=list(self.parent_cost[:max(k, 2)]), child_cost=self.child_cost,
                    predicted=self.predicted, boundaries=self.boundaries, regions_from=list(self.regions_from[:max(k, 2)]),
                    adopted=self.adopted, gpu_ms=self.gpu_ms)


class CrossAllStats(C.Structure):
    _fields_ = [("chains_with_best", C.c_uint32), ("distinct", C.c_uint32), ("parent_rank", C.c_uint32 * XO_MAX_PARENTS),
                ("own_parent", C.c_uint32), ("fell_back", C.c_uint32), ("cross", CrossStats)]

    def asdict(self):
        own = self.own_parent
        return dict(chains_with_best=self.chains_with_best, distinct=self.distinct, parent_rank=list(self.parent_rank[:self.distinct]),
                    own_parent=None if own == 0xFFFFFFFF else own, fell_back=self.fell_back, cross=self.cross.asdict())


class StreamInfo(C.Structure):
    _fields_ = [("container", C.c_int), ("props", Properties), ("dict_size", C.c_uint32), ("declared_size", C.c_uint64)]


class ImportStats(C.Structure):
    _fields_ = [("packets", C.c_uint64), ("literals", C.c_uint64), ("matches", C.c_uint64), ("short_reps", C.c_uint64),
                ("long_reps", C.c_uint64 * 4), ("reexpressed", C.c_uint64), ("clipped", C.c_uint64),
                ("props_changes", C.c_uint64), ("error_pos", C.c_uint64), ("error", C.c_char_p)]


class XzOptions(C.Structure):
    _fields_ = [("filter", C.c_uint32), ("dict_size", C.c_uint32), ("check", C.c_uint32)]


class MemorySink(C.Structure):
    _fields_ = [("buf", C.c_void_p), ("cap", C.c_size_t), ("len", C.c_size_t)]


class OutputInterface(C.Structure):
    _fields_ = [("write", C.c_void_p), ("private_data", C.c_void_p)]


_hip = None
_host = None


def hip_lib():
    """Load libmegalania_hip.so.  Raises if it was not built -- no fallback."""
    global _hip
    if _hip is None:
        if not os.path.exists(HIP_SO):
            raise MglError(f"{HIP_SO} is missing: run `python -m megalania_amd.build` (hipcc, gfx950). "
                           "There is no CPU implementation of the search path.")
        # MGL_HIP_SO: another build of the same library (tools/ab_builds.sh compares two builds on one state)
        L = C.CDLL(os.environ.get("MGL_HIP_SO") or HIP_SO)
        L.mgl_version.restype = C.c_char_p
        L.mgl_last_error.restype = C.c_char_p
        L.mgl_device_count.restype = C.c_int
        L.mgl_sa_create.restype = C.c_void_p
        L.mgl_sa_create.argtypes = [C.c_void_p, C.c_size_t, Properties, C.POINTER(Config)]
        L.mgl_sa_destroy.argtypes = [C.c_void_p]
        L.mgl_sa_begin_epoch.argtypes = [C.c_void_p, C.c_uint, C.c_int]
        L.mgl_sa_set_slab.argtypes = [C.c_void_p, C.c_void_p]
        L.mgl_sa_seed_greedy.argtypes = [C.c_void_p, C.c_uint32]
        L.mgl_sa_seed_optimal.argtypes = [C.c_void_p, C.POINTER(OptimalConfig), C.POINTER(OptimalStats)]
        L.mgl_optimal_pass.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p,
                                       C.POINTER(C.c_uint64)]
        L.mgl_optimal_prices.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.mgl_sa_seed_adaptive.argtypes = [C.c_void_p, C.POINTER(AdaptiveConfig), C.POINTER(OptimalStats)]
        L.mgl_adaptive_pass.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                        C.POINTER(C.c_uint64)]
        L.mgl_sa_seed_sweep.argtypes = [C.c_void_p, C.POINTER(ParseSweepConfig), C.POINTER(ParseVariant), C.c_size_t,
                                        C.POINTER(OptimalStats), C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
        L.mgl_parse_sweep_props.argtypes = [C.c_void_p, C.POINTER(ParseSweepConfig), C.POINTER(ParseVariant),
                                            C.POINTER(Properties), C.c_size_t, C.POINTER(OptimalStats), C.POINTER(C.c_uint32),
                                            C.c_void_p, C.POINTER(C.c_double)]
        L.mgl_sa_set_match_finder.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
        L.mgl_match_frontier.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.POINTER(C.c_size_t), C.POINTER(C.c_double)]
        L.mgl_sa_set_temperature.argtypes = [C.c_void_p, C.c_uint64]
        L.mgl_sa_set_best.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.mgl_sa_set_accept_mode.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
        L.mgl_sa_step_modes.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.mgl_sa_run.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(Stats)]
        L.mgl_sa_current.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        L.mgl_sa_best.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        L.mgl_cost_slab.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_size_t)]
        L.mgl_props_sweep.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(PropsCost), C.c_size_t, C.POINTER(C.c_size_t),
                                      C.POINTER(C.c_double)]
        L.mgl_final_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint8), C.c_void_p]
        L.mgl_top_k.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
        L.mgl_substrings.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.POINTER(C.c_size_t)]
        L.mgl_neighbours.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.mgl_debug_dump.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.mgl_debug_set.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64]
        L.mgl_comm_unique_id.argtypes = [C.c_void_p]
        L.mgl_comm_init.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.mgl_comm_init_shm.argtypes = [C.POINTER(C.c_void_p), C.c_char_p, C.c_uint64, C.c_int, C.c_int, C.c_int]
        L.mgl_comm_min_u64.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.mgl_comm_destroy.argtypes = [C.c_void_p]
        L.mgl_comm_rank.argtypes = [C.c_void_p]
        L.mgl_comm_world.argtypes = [C.c_void_p]
        L.mgl_sa_exchange_best.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
        L.mgl_sa_best_packed.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        L.mgl_sa_adopt_best_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.mgl_crossover.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.c_uint32, C.c_void_p, C.POINTER(CrossStats)]
        L.mgl_sa_cross_best.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(CrossStats)]
        L.mgl_sa_exchange_cross.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_uint64),
                                            C.POINTER(CrossStats)]
        L.mgl_comm_allgather_u64.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.mgl_slab_hash.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        L.mgl_sa_exchange_cross_all.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(CrossAllStats)]
        L.mgl_sa_set_focus.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
        L.mgl_sa_focus.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.mgl_focus_slice.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_uint64)]
        L.mgl_cost_map.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Properties), C.c_void_p, C.POINTER(CostReport)]
        L.mgl_sa_set_target_weights.argtypes = [C.c_void_p, C.c_void_p]
        L.mgl_sa_weight_targets_by_cost.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.mgl_sa_target_weights.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.mgl_weight_value.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
        L.mgl_cost_map_live.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(CostReport)]
        L.mgl_sa_set_live_weights.argtypes = [C.c_void_p, C.POINTER(LiveWeightsConfig)]
        L.mgl_sa_live_weights.argtypes = [C.c_void_p, C.POINTER(LiveWeightsConfig), C.POINTER(LiveWeightsStats)]
        L.mgl_segment_cuts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.mgl_props_sweep_spans.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                            C.POINTER(C.c_size_t), C.POINTER(C.c_double)]
        L.mgl_segment_partition.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint64, C.POINTER(Segment),
                                            C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]
        L.mgl_sa_segment_props.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(Segment), C.c_size_t,
                                           C.POINTER(C.c_size_t), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                           C.POINTER(C.c_double)]
        L.mgl_segment_reparse.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Segment), C.c_size_t, C.POINTER(AdaptiveConfig),
                                          C.c_void_p, C.POINTER(Segment), C.POINTER(SegmentParseStats), C.POINTER(C.c_int),
                                          C.POINTER(C.c_double)]
        L.mgl_rng_draw_at.restype = C.c_uint32
        L.mgl_rng_draw_at.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]
        _hip = L
    return _hip


def host_lib():
    global _host
    if _host is None:
        if not os.path.exists(HOST_SO):
            raise MglError(f"{HOST_SO} is missing: run `python -m megalania_amd.build`")
        L = C.CDLL(HOST_SO)
        L.mgl_emit_stream.restype = C.c_bool
        L.mgl_emit_stream.argtypes = [C.c_void_p, C.c_size_t, Properties, C.c_void_p, C.POINTER(OutputInterface)]
        L.mgl_emit_stream_dict.restype = C.c_bool
        L.mgl_emit_stream_dict.argtypes = [C.c_void_p, C.c_size_t, Properties, C.c_void_p, C.c_uint32, C.POINTER(OutputInterface)]
        L.mgl_emit_xz.restype = C.c_bool
        L.mgl_emit_xz.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, Properties, C.c_void_p, C.POINTER(XzOptions),
                                  C.POINTER(OutputInterface)]
        L.mgl_bcj_x86.restype = None
        L.mgl_bcj_x86.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
        L.mgl_stream_info_read_x.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(StreamInfo), C.POINTER(C.c_uint32)]
        L.mgl_memory_output_new.argtypes = [C.POINTER(OutputInterface), C.POINTER(MemorySink)]
        L.mgl_stream_info_read.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(StreamInfo)]
        L.mgl_stream_import.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32,
                                        C.c_void_p, C.POINTER(ImportStats)]
        L.mgl_host_cost_map.argtypes = [C.c_void_p, C.c_size_t, Properties, C.c_void_p, C.c_void_p, C.POINTER(CostReport)]
        L.mgl_host_segment_cost.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint64, C.c_uint64, Properties,
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.mgl_host_segment_packets.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                               C.c_size_t, C.POINTER(C.c_size_t)]
        L.mgl_emit_xz_segments.restype = C.c_bool
        L.mgl_emit_xz_segments.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(Segment), C.c_size_t,
                                           C.POINTER(XzOptions), C.POINTER(OutputInterface)]
        _host = L
    return _host


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def literal_slab(n: int) -> np.ndarray:
    s = np.zeros(n, dtype=PACKET)
    s["type"] = LITERAL
    s["len"] = 1
    return s


def focus_slice(n: int, world: int, rank: int, round: int):
    """(lo, hi): the focus window of chain `rank` of `world` in exchange round `round` (mgl_focus_slice; no device needed).  The
    slices of a round tile [0, n); odd rounds cut half a slice away from even rounds.  Raises MglError (rc -1) for
    rank >= world, world == 0, n < 2 * world."""
    L = hip_lib()
    lo, hi = C.c_uint64(0), C.c_uint64(0)
    rc = L.mgl_focus_slice(n, world, rank, round, C.byref(lo), C.byref(hi))
    if rc != 0:
        raise MglError(f"rc={rc}: {L.mgl_last_error().decode()}", rc=rc)
    return lo.value, hi.value


def weight_value(W: int, K: int, j: int, seed: int, step: int) -> int:
    """The value neighbour j of K draws from a window of weight W in step `step` under target weights (mgl_weight_value; no
    device needed): uniform in slice [j W / K, (j + 1) W / K).  Raises MglError (rc -1) for W == 0, W >= 2^44, K == 0,
    K > 2^20, j >= K."""
    L = hip_lib()
    v = C.c_uint64(0)
    rc = L.mgl_weight_value(W, K, j, seed, step, C.byref(v))
    if rc != 0:
        raise MglError(f"rc={rc}: {L.mgl_last_error().decode()}", rc=rc)
    return v.value


def emit_stream(data: bytes, slab: np.ndarray, lc=0, lp=0, pb=0) -> bytes:
    """Host emission (C): header + range coder over the slab's walk -> .lzma bytes."""
    L = host_lib()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    cap = 2 * len(buf) + 1024
    out = np.zeros(cap, dtype=np.uint8)
    sink = MemorySink(out.ctypes.data, cap, 0)
    oi = OutputInterface()
    L.mgl_memory_output_new(C.byref(oi), C.byref(sink))
    slab = np.ascontiguousarray(slab, dtype=PACKET)
    if not L.mgl_emit_stream(_ptr(buf), len(buf), Properties(lc, lp, pb), _ptr(slab), C.byref(oi)):
        raise MglError("mgl_emit_stream failed (invalid slab?)")
    assert sink.len <= cap
    return out[: sink.len].tobytes()


def emit_stream_dict(data: bytes, slab: np.ndarray, dict_size: int, lc=0, lp=0, pb=0) -> bytes:
    """emit_stream with `dict_size` (0 = 4 MiB) as the header's dictionary and as the window the slab is checked against."""
    L = host_lib()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    cap = 2 * len(buf) + 1024
    out = np.zeros(cap, dtype=np.uint8)
    sink = MemorySink(out.ctypes.data, cap, 0)
    oi = OutputInterface()
    L.mgl_memory_output_new(C.byref(oi), C.byref(sink))
    slab = np.ascontiguousarray(slab, dtype=PACKET)
    if not L.mgl_emit_stream_dict(_ptr(buf), len(buf), Properties(lc, lp, pb), _ptr(slab), dict_size, C.byref(oi)):
        raise MglError("mgl_emit_stream_dict failed (invalid slab?)")
    assert sink.len <= cap
    return out[: sink.len].tobytes()


def bcj_x86(data: bytes, encode: bool = True) -> bytes:
    """The .xz x86 branch/call/jump filter (id 0x04, start offset 0) over the whole of `data`; encode=False inverts it."""
    L = host_lib()
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    L.mgl_bcj_x86(_ptr(buf), len(buf), int(bool(encode)))
    return buf.tobytes()


def emit_xz(original: bytes, coded: bytes, slab: np.ndarray, lc=0, lp=0, pb=0, filter=0, dict_size=0, check=1) -> bytes:
    """Host emission (C, mgl_emit_xz): one .xz stream of one block, [x86,] LZMA2 over the slab's walk.  `coded` is what the
    LZMA layer sees (bcj_x86(original) when filter = 4, else original) and `slab` a parse of it."""
    L = host_lib()
    org = np.frombuffer(bytes(original), dtype=np.uint8)
    cod = np.frombuffer(bytes(coded), dtype=np.uint8)
    if len(org) != len(cod):
        raise MglError("emit_xz: original and coded differ in length", rc=-1)
    cap = 2 * len(org) + (len(org) >> 10) * 16 + 1024
    out = np.zeros(cap, dtype=np.uint8)
    sink = MemorySink(out.ctypes.data, cap, 0)
    oi = OutputInterface()
    L.mgl_memory_output_new(C.byref(oi), C.byref(sink))
    slab = np.ascontiguousarray(slab, dtype=PACKET)
    if len(slab) != len(org):
        raise MglError("emit_xz: the slab must have one entry per input byte", rc=-1)
    opt = XzOptions(filter, dict_size, check)
    if not L.mgl_emit_xz(_ptr(org), _ptr(cod), len(org), Properties(lc, lp, pb), _ptr(slab), C.byref(opt), C.byref(oi)):
        raise MglError("mgl_emit_xz failed (invalid slab or option?)")
    assert sink.len <= cap
    return out[: sink.len].tobytes()


def stream_info(stream: bytes) -> dict:
    """Container, lc/lp/pb, dictionary and declared size of an LZMA-alone or .xz stream
    (declared_size None = unknown, the stream ends with an end marker)."""
    L = host_lib()
    buf = np.frombuffer(bytes(stream), dtype=np.uint8)
    info = StreamInfo()
    rc = L.mgl_stream_info_read(_ptr(buf), len(buf), C.byref(info))
    if rc != 0:
        raise MglError(f"rc={rc}: not an LZMA-alone or .xz stream", rc=rc)
    return dict(container=info.container, lc=info.props.lc, lp=info.props.lp, pb=info.props.pb,
                dict_size=info.dict_size, declared_size=None if info.declared_size == (1 << 64) - 1 else info.declared_size)


def stream_info_x(stream: bytes) -> dict:
    """stream_info that also reads an .xz whose chain is [x86, LZMA2]: `filter` is 4 for it, else 0."""
    L = host_lib()
    buf = np.frombuffer(bytes(stream), dtype=np.uint8)
    info = StreamInfo()
    flt = C.c_uint32(0)
    rc = L.mgl_stream_info_read_x(_ptr(buf), len(buf), C.byref(info), C.byref(flt))
    if rc != 0:
        raise MglError(f"rc={rc}: not an LZMA-alone or .xz stream", rc=rc)
    return dict(container=info.container, lc=info.props.lc, lp=info.props.lp, pb=info.props.pb, dict_size=info.dict_size,
                declared_size=None if info.declared_size == (1 << 64) - 1 else info.declared_size, filter=flt.value)


def stream_import(stream: bytes, data: bytes, window: int = 0x400000, clip: bool = False, x86: bool = False):
    """The parse inside an LZMA-alone / .xz stream of `data` as a position-indexed slab (host C, mgl_stream_import),
    re-expressed for one LZMA1 stream.  x86: an .xz chain [x86, LZMA2] is accepted, and `data` is then the filtered
    input, bcj_x86(original).  Returns (slab, stats dict); raises MglError (rc, error, error_pos)."""
    L = host_lib()
    buf = np.frombuffer(bytes(stream), dtype=np.uint8)
    dat = np.frombuffer(bytes(data), dtype=np.uint8)
    slab = np.zeros(len(dat), dtype=PACKET)
    st = ImportStats()
    rc = L.mgl_stream_import(_ptr(buf), len(buf), _ptr(dat), len(dat), window,
                             (IMPORT_CLIP_WINDOW if clip else 0) | (IMPORT_X86 if x86 else 0), _ptr(slab), C.byref(st))
    err = st.error.decode() if st.error else None
    if rc != 0:
        raise MglError(f"rc={rc}: stream import failed at input position {st.error_pos}: {err}", rc=rc, error=err,
                       error_pos=st.error_pos)
    stats = {k: getattr(st, k) for k, _ in ImportStats._fields_ if k not in ("error", "error_pos", "long_reps")}
    stats["long_reps"] = list(st.long_reps)
    return slab, stats


def host_cost_map(data: bytes, slab: np.ndarray, props=(0, 0, 0)):
    """Where the parse `slab` of `data` spends its bits under props = (lc, lp, pb), on the host (C, mgl_host_cost_map; no
    device needed): (uint32 map, one entry per input byte, summing to the total; report dict: total, packets, class_cost /
    class_bits in COST_CLASSES order, type_cost / type_packets / type_bytes in PACKET_TYPES order).  The same integers as
    SA.cost_map.  Raises MglError (rc -1) for a slab that is no valid parse of `data` or an unsupported triple."""
    L = host_lib()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    slab = np.ascontiguousarray(slab, dtype=PACKET)
    if len(slab) != len(buf):
        raise MglError("host_cost_map: the slab must have one entry per input byte", rc=-1)
    out = np.zeros(len(buf), dtype=np.uint32)
    rep = CostReport()
    rc = L.mgl_host_cost_map(_ptr(buf), len(buf), Properties(*props), _ptr(slab), _ptr(out), C.byref(rep))
    if rc != 0:
        raise MglError(f"rc={rc}: mgl_host_cost_map failed (invalid slab or properties?)", rc=rc)
    return out, rep.asdict(device=False)


def host_segment_cost(data: bytes, slab: np.ndarray, lo: int, hi: int, props=(0, 0, 0)):
    """(cost, reexpressed): the exact cost of the packets of `slab` that start in [lo, hi), coded from an LZMA2 state reset at
    lo under props -- fresh model, ctx_state 0, reps 0, rep packets re-expressed against that stack -- and how many packets
    the re-expression changed (host C, mgl_host_segment_cost; no device needed).  Raises MglError (rc -1) for a slab that is
    no valid parse, a bad triple, or lo / hi off the walk."""
    L = host_lib()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    slab = np.ascontiguousarray(slab, dtype=PACKET)
    if len(slab) != len(buf):
        raise MglError("host_segment_cost: the slab must have one entry per input byte", rc=-1)
    cost, changed = C.c_uint64(0), C.c_uint64(0)
    rc = L.mgl_host_segment_cost(_ptr(buf), len(buf), _ptr(slab), lo, hi, Properties(*props), C.byref(cost), C.byref(changed))
    if rc != 0:
        raise MglError(f"rc={rc}: mgl_host_segment_cost failed (invalid slab, properties or segment?)", rc=rc)
    return cost.value, changed.value


def host_segment_packets(data: bytes, slab: np.ndarray, lo: int, hi: int) -> np.ndarray:
    """The re-expressed packets of segment [lo, hi) in walk order (host C, mgl_host_segment_packets)."""
    L = host_lib()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    slab = np.ascontiguousarray(slab, dtype=PACKET)
    if len(slab) != len(buf):
        raise MglError("host_segment_packets: the slab must have one entry per input byte", rc=-1)
    out = np.zeros(max(hi - lo, 1), dtype=PACKET)
    cnt = C.c_size_t(0)
    rc = L.mgl_host_segment_packets(_ptr(buf), len(buf), _ptr(slab), lo, hi, _ptr(out), len(out), C.byref(cnt))
    if rc != 0:
        raise MglError(f"rc={rc}: mgl_host_segment_packets failed (invalid slab or segment?)", rc=rc)
    return out[: cnt.value].copy()


def emit_xz_segments(original: bytes, coded: bytes, slab: np.ndarray, segments, filter=0, dict_size=0, check=1) -> bytes:
    """emit_xz with a triple per segment (host C, mgl_emit_xz_segments): `segments` is a list of dicts lo, hi, props that tile
    [0, n) at packet starts; every segment after the first opens with an LZMA2 chunk that resets the state and sets its
    props.  Raises MglError when the writer refuses (invalid slab, option, or segments that do not tile)."""
    L = host_lib()
    org = np.frombuffer(bytes(original), dtype=np.uint8)
    cod = np.frombuffer(bytes(coded), dtype=np.uint8)
    if len(org) != len(cod):
        raise MglError("emit_xz_segments: original and coded differ in length", rc=-1)
    cap = 2 * len(org) + (len(org) >> 10) * 16 + 1024 + 16 * len(segments)
    out = np.zeros(cap, dtype=np.uint8)
    sink = MemorySink(out.ctypes.data, cap, 0)
    oi = OutputInterface()
    L.mgl_memory_output_new(C.byref(oi), C.byref(sink))
    slab = np.ascontiguousarray(slab, dtype=PACKET)
    if len(slab) != len(org):
        raise MglError("emit_xz_segments: the slab must have one entry per input byte", rc=-1)
    opt = XzOptions(filter, dict_size, check)
    if not L.mgl_emit_xz_segments(_ptr(org), _ptr(cod), len(org), _ptr(slab), _segments(segments), len(segments), C.byref(opt),
                                  C.byref(oi)):
        raise MglError("mgl_emit_xz_segments failed (invalid slab, option or segments?)")
    assert sink.len <= cap
    return out[: sink.len].tobytes()


def segment_partition(cost, cuts, overhead=SEG_OVERHEAD):
    """(segments, total): the cheapest way to tile [0, n) with spans of `cuts`, each under its cheapest triple, `overhead` per
    segment after the first (mgl_segment_partition; host arithmetic, no device needed).  cost: the table of
    SA.props_sweep_spans, shape (spans, 75).  Segments are dicts lo, hi, props, cost in ascending order."""
    L = hip_lib()
    cost = np.ascontiguousarray(cost, dtype=np.uint64).reshape(-1)
    cuts = np.ascontiguousarray(cuts, dtype=np.uint64)
    m = len(cuts) - 1
    if not 1 <= m < SEG_MAX_CUTS or len(cost) != m * (m + 1) // 2 * len(PROPS_TRIPLES):
        raise MglError("segment_partition: 2..17 cuts and 75 costs per span", rc=-1)
    segs = (Segment * m)()
    nseg, total = C.c_size_t(0), C.c_uint64(0)
    rc = L.mgl_segment_partition(_ptr(cost), len(cuts), _ptr(cuts), overhead, segs, C.byref(nseg), C.byref(total))
    if rc != 0:
        raise MglError(f"rc={rc}: {L.mgl_last_error().decode()}", rc=rc)
    return [segs[k].asdict() for k in range(nseg.value)], total.value


class SA:
    """One mgl_sa handle = one SA chain resident on one GPU."""

    def __init__(self, data: bytes, neighbours_per_step=4096, seed=1673551, top_k=20, lc=0, lp=0, pb=0,
                 dict_limit=0, max_bucket_scan=0, iters_per_epoch=0, device=0, timing=False, fullwalk=False,
                 snapshots=True, serial_build=False, flags=0, accept=None, bulk_threshold=0):
        self.L = hip_lib()
        if self.L.mgl_device_count() < 1:
            raise MglError("no HIP device visible: the search path has no CPU implementation")
        self.data = np.frombuffer(bytes(data), dtype=np.uint8).copy()
        self.n = len(self.data)
        self.K = neighbours_per_step
        self.props = Properties(lc, lp, pb)
        self.cfg = Config(seed, neighbours_per_step, top_k, dict_limit, max_bucket_scan, iters_per_epoch, device,
                          (F_TIMING if timing else 0) | (F_FULLWALK if fullwalk else 0)
                          | (0 if snapshots else F_NO_SNAPSHOTS) | (F_SERIAL_BUILD if serial_build else 0) | flags)
        self.h = self.L.mgl_sa_create(_ptr(self.data), self.n, self.props, C.byref(self.cfg))
        if not self.h:
            raise MglError(self.L.mgl_last_error().decode())
        self.nprobs = 1847 + (0x300 << (lc + lp))
        if accept is not None:
            self.set_accept_mode(accept, bulk_threshold)

    def set_accept_mode(self, mode, bulk_threshold=0):
        """ACCEPT_AUTO (default) / ACCEPT_SINGLE / ACCEPT_BULK, or the strings "auto" / "single" / "bulk"."""
        mode = {"auto": ACCEPT_AUTO, "single": ACCEPT_SINGLE, "bulk": ACCEPT_BULK}.get(mode, mode)
        self._chk(self.L.mgl_sa_set_accept_mode(self.h, mode, bulk_threshold))

    def set_focus(self, lo: int, hi: int):
        """The step's K targets among the packets that start in bytes [lo, hi) (mgl_sa_set_focus); (0, 0) clears the window.
        Nothing below lo is written while it is set.  Stays until changed."""
        self._chk(self.L.mgl_sa_set_focus(self.h, lo, hi))

    def focus(self):
        """(lo, hi, packets): the window in force ((0, 0): none) and the packets of the current walk it holds"""
        lo, hi, pk = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._chk(self.L.mgl_sa_focus(self.h, C.byref(lo), C.byref(hi), C.byref(pk)))
        return lo.value, hi.value, pk.value

    def set_target_weights(self, weights):
        """The step's K targets in proportion to weights[x], one uint32 per input byte (mgl_sa_set_target_weights); None clears.
        Composes with the focus window; a window that weighs 0 falls back on the rule without weights.  Stays until changed."""
        if weights is not None:
            weights = np.ascontiguousarray(weights, dtype=np.uint32)
            if len(weights) != self.n:
                raise MglError("set_target_weights: one weight per input byte", rc=-1)
        self._chk(self.L.mgl_sa_set_target_weights(self.h, _ptr(weights)))

    def weight_targets_by_cost(self, floor=0, slab=None):
        """weights := the cost map of `slab` (None: the current slab) under the handle's lc/lp/pb, plus `floor` per byte, made on
        the device (mgl_sa_weight_targets_by_cost).  Returns (total, gpu_ms): the map's total + floor * n and the map's device
        time."""
        if slab is not None:
            slab = np.ascontiguousarray(slab, dtype=PACKET)
            if len(slab) != self.n:
                raise MglError("weight_targets_by_cost: the slab must have one entry per input byte", rc=-1)
        total, ms = C.c_uint64(0), C.c_double(0)
        self._chk(self.L.mgl_sa_weight_targets_by_cost(self.h, _ptr(slab), floor, C.byref(total), C.byref(ms)))
        return total.value, ms.value

    def target_weights(self):
        """(uint32 weights, total, window): the weights in force (all 0: none), S[n], and W under the focus window in force"""
        out = np.zeros(self.n, dtype=np.uint32)
        total, window = C.c_uint64(0), C.c_uint64(0)
        self._chk(self.L.mgl_sa_target_weights(self.h, _ptr(out), C.byref(total), C.byref(window)))
        return out, total.value, window.value

    def set_live_weights(self, every, floor=0, floor_mean=False, single_only=False):
        """Target weights made again from the live cost map before every step g with g % every == 0, and when the slab was
        replaced from outside a run (mgl_sa_set_live_weights has the rule); every=None turns them off and clears the weights.
        floor_mean: each refresh adds its map's total // n.  single_only: bulk-route steps neither use nor refresh them."""
        if every is None:
            self._chk(self.L.mgl_sa_set_live_weights(self.h, None))
            return
        cfg = LiveWeightsConfig(every, floor, int(bool(floor_mean)), LW_SINGLE_ONLY if single_only else 0)
        self._chk(self.L.mgl_sa_set_live_weights(self.h, C.byref(cfg)))

    def live_weights(self) -> dict:
        """the live weights' configuration (every == 0: off) and what they did since they were enabled"""
        cfg, st = LiveWeightsConfig(), LiveWeightsStats()
        self._chk(self.L.mgl_sa_live_weights(self.h, C.byref(cfg), C.byref(st)))
        return dict(every=cfg.every, floor=cfg.floor, floor_mean=bool(cfg.floor_mean), single_only=bool(cfg.flags & LW_SINGLE_ONLY),
                    flags=cfg.flags, refreshes=st.refreshes, skipped=st.skipped, last_gstep=st.last_gstep, last_total=st.last_total,
                    gpu_ms=st.gpu_ms)

    def step_modes(self) -> np.ndarray:
        """per step of the last run(): 0 single, 1 bulk"""
        cnt = C.c_size_t(0)
        self._chk(self.L.mgl_sa_step_modes(self.h, None, 0, C.byref(cnt)))
        out = np.zeros(max(1, cnt.value), dtype=np.uint8)
        self._chk(self.L.mgl_sa_step_modes(self.h, _ptr(out), cnt.value, C.byref(cnt)))
        return out[: cnt.value]

    def close(self):
        if getattr(self, "h", None):
            self.L.mgl_sa_destroy(self.h)
            self.h = None

    __del__ = close

    def _chk(self, rc):
        if rc != 0:
            raise MglError(f"rc={rc}: {self.L.mgl_last_error().decode()}", rc=rc)

    def begin_epoch(self, phase=0, from_best=False):
        self._chk(self.L.mgl_sa_begin_epoch(self.h, phase, int(from_best)))

    def set_slab(self, slab):
        slab = np.ascontiguousarray(slab, dtype=PACKET)
        self._chk(self.L.mgl_sa_set_slab(self.h, _ptr(slab)))

    def seed_greedy(self, candidates: int = 256):
        """Current slab := greedy LZ parse made on the device (opt-in starting point)."""
        self._chk(self.L.mgl_sa_seed_greedy(self.h, candidates))

    def seed_optimal(self, passes: int = 0, cand: int = 0, chunk: int = 0) -> dict:
        """Current slab := the best of `passes` price-driven optimal parses made on the device (mgl_sa_seed_optimal;
        0 = the library's defaults).  Returns the per-pass stats: exact cost, DP objective and device ms per pass."""
        st = OptimalStats()
        self._chk(self.L.mgl_sa_seed_optimal(self.h, C.byref(OptimalConfig(passes, cand, chunk)), C.byref(st)))
        k = st.passes
        return dict(passes=k, best_pass=st.best_pass, greedy_cost=st.greedy_cost, cost=list(st.cost[:k]),
                    objective=list(st.objective[:k]), ms=list(st.ms[:k]))

    def optimal_prices(self, slab) -> np.ndarray:
        """The static prices (u32 per (slot, bit), index 2 * slot + bit) that the optimal seed derives from `slab`."""
        slab = np.ascontiguousarray(slab, dtype=PACKET)
        out = np.zeros(2 * self.nprobs, dtype=np.uint32)
        self._chk(self.L.mgl_optimal_prices(self.h, _ptr(slab), _ptr(out), len(out)))
        return out

    def optimal_pass(self, prices, cand: int, chunk: int):
        """One DP pass under explicit prices, LZMA initial state at every chunk start (parity hook, SA state untouched).
        Returns (unresolved slab with absolute distances, objective)."""
        prices = np.ascontiguousarray(prices, dtype=np.uint32)
        out = np.zeros(self.n, dtype=PACKET)
        obj = C.c_uint64(0)
        self._chk(self.L.mgl_optimal_pass(self.h, _ptr(prices), len(prices), cand, chunk, _ptr(out), C.byref(obj)))
        return out, obj.value

    def seed_adaptive(self, passes: int = 0, cand: int = 0, chunk: int = 0, segment: int = 0, ahead: int = 0,
                      from_current: bool = False) -> dict:
        """Current slab := the best of `passes` optimal parses under adaptive prices (mgl_sa_seed_adaptive; 0 = the
        library's defaults).  from_current: the re-parse -- pass 0 starts from the current slab, which stays if no pass
        beats it (best_pass is then None and greedy_cost its cost).  Returns the per-pass stats as seed_optimal does."""
        st = OptimalStats()
        cfg = AdaptiveConfig(passes, cand, chunk, segment, ahead, int(from_current))
        self._chk(self.L.mgl_sa_seed_adaptive(self.h, C.byref(cfg), C.byref(st)))
        k = st.passes
        return dict(passes=k, best_pass=None if st.best_pass == 0xFFFFFFFF else st.best_pass, greedy_cost=st.greedy_cost,
                    cost=list(st.cost[:k]), objective=list(st.objective[:k]), ms=list(st.ms[:k]))

    def seed_sweep(self, variants, passes: int = 0, chunk: int = 0, depth: int = 0, from_current: bool = False) -> dict:
        """Current slab := the cheapest parse of a batch of adaptive parses (mgl_sa_seed_sweep).  variants: a list of
        (finder, cand, segment, ahead), finder MF_NEAREST / MF_FRONTIER or their names; each is the parse seed_adaptive
        makes under that finder, all run through the same launches.  Returns results (per variant, the dict seed_adaptive
        returns; ms is the batch's), best_variant (None: from_current, and nothing beat the current slab) and gpu_ms."""
        names = {"nearest": MF_NEAREST, "frontier": MF_FRONTIER}
        nv = len(variants)
        arr = (ParseVariant * max(1, nv))(*[ParseVariant(names.get(f, f), c, s, a) for f, c, s, a in variants])
        st = (OptimalStats * max(1, nv))()
        best, ms = C.c_uint32(0), C.c_double(0)
        cfg = ParseSweepConfig(passes, chunk, depth, int(from_current))
        self._chk(self.L.mgl_sa_seed_sweep(self.h, C.byref(cfg), arr, nv, st, C.byref(best), C.byref(ms)))
        results = [dict(passes=r.passes, best_pass=None if r.best_pass == 0xFFFFFFFF else r.best_pass, greedy_cost=r.greedy_cost,
                        cost=list(r.cost[:r.passes]), objective=list(r.objective[:r.passes]), ms=list(r.ms[:r.passes]))
                   for r in st[:nv]]
        return dict(results=results, best_variant=None if best.value == 0xFFFFFFFF else best.value, gpu_ms=ms.value)

    def parse_sweep_props(self, variants, props, passes: int = 0, chunk: int = 0, depth: int = 0, from_current: bool = False) -> dict:
        """The batch of seed_sweep with a triple per variant (mgl_parse_sweep_props; SA state untouched).  variants as in
        seed_sweep, props one (lc, lp, pb) per variant: each is the parse seed_adaptive makes on a fresh handle at its
        triple, whatever this handle's own.  Returns results (per variant, costs exact under its triple), best_variant,
        slab (the cheapest parse, as current() returns one) and gpu_ms."""
        names = {"nearest": MF_NEAREST, "frontier": MF_FRONTIER}
        nv = len(variants)
        if len(props) != nv:
            raise MglError("parse_sweep_props: one (lc, lp, pb) per variant", rc=-1)
        arr = (ParseVariant * max(1, nv))(*[ParseVariant(names.get(f, f), c, s, a) for f, c, s, a in variants])
        pr = (Properties * max(1, nv))(*[Properties(*t) for t in props])
        st = (OptimalStats * max(1, nv))()
        best, ms = C.c_uint32(0), C.c_double(0)
        slab = np.zeros(self.n, dtype=PACKET)
        cfg = ParseSweepConfig(passes, chunk, depth, int(from_current))
        self._chk(self.L.mgl_parse_sweep_props(self.h, C.byref(cfg), arr, pr, nv, st, C.byref(best), _ptr(slab), C.byref(ms)))
        results = [dict(passes=r.passes, best_pass=None if r.best_pass == 0xFFFFFFFF else r.best_pass, greedy_cost=r.greedy_cost,
                        cost=list(r.cost[:r.passes]), objective=list(r.objective[:r.passes]), ms=list(r.ms[:r.passes]))
                   for r in st[:nv]]
        return dict(results=results, best_variant=best.value, slab=slab, gpu_ms=ms.value)

    def adaptive_pass(self, parse_in, cand: int, chunk: int, segment: int, ahead: int):
        """One adaptive-price pass from the chunk starts of the valid slab `parse_in` (parity hook, SA state untouched).
        Returns (unresolved slab with absolute distances, objective)."""
        parse_in = np.ascontiguousarray(parse_in, dtype=PACKET)
        if len(parse_in) != self.n:
            raise MglError("adaptive_pass: parse_in must have one entry per input byte")
        out = np.zeros(self.n, dtype=PACKET)
        obj = C.c_uint64(0)
        self._chk(self.L.mgl_adaptive_pass(self.h, _ptr(parse_in), cand, chunk, segment, ahead, _ptr(out), C.byref(obj)))
        return out, obj.value

    def set_match_finder(self, finder, depth: int = 0):
        """Where the optimal / adaptive parses take a node's MATCH sources from: MF_NEAREST (default; "nearest") or
        MF_FRONTIER ("frontier": the nearest source of every achievable length, `depth` run entries examined per position,
        0 = the library's default)."""
        finder = {"nearest": MF_NEAREST, "frontier": MF_FRONTIER}.get(finder, finder)
        self._chk(self.L.mgl_sa_set_match_finder(self.h, finder, depth))

    def match_frontier(self, depth: int = 0, cap=None):
        """The MF_FRONTIER lists (parity hook, SA state untouched): (off[n + 1], src, len, device ms of their build).
        cap: the room offered for the entries (default: as many as there are)."""
        cnt, ms = C.c_size_t(0), C.c_double(0)
        if cap is None:
            rc = self.L.mgl_match_frontier(self.h, depth, None, None, None, 0, C.byref(cnt), C.byref(ms))
            if rc != 0 and rc != -4:  # MGL_ERANGE: cnt holds the number of entries
                self._chk(rc)
            cap = cnt.value
        off = np.zeros(self.n + 1, dtype=np.uint32)
        src = np.zeros(max(1, cap), dtype=np.uint32)
        ln = np.zeros(max(1, cap), dtype=np.uint16)
        self._chk(self.L.mgl_match_frontier(self.h, depth, _ptr(off), _ptr(src), _ptr(ln), cap, C.byref(cnt), C.byref(ms)))
        return off, src[: cnt.value].copy(), ln[: cnt.value].copy(), ms.value

    def seed_stream(self, stream: bytes, clip: bool = False) -> int:
        """Best slab := the parse inside an existing .lzma / .xz stream of this input (stream_import, window =
        the handle's dict_limit), costed on the device; returns that cost.  begin_epoch(.., from_best=True) then
        searches from it."""
        slab, _ = stream_import(stream, self.data.tobytes(), window=self.cfg.dict_limit or 0x400000, clip=clip)
        cost = self.cost_slab(slab, want_cum=False)["total"]
        self.set_best(slab, cost)
        return cost

    def set_temperature(self, temperature: int):
        """Opt-in Metropolis accept rule, temperature in cost units (16384 per byte); 0 = reference rule."""
        self._chk(self.L.mgl_sa_set_temperature(self.h, temperature))

    def set_best(self, slab, perplexity: int):
        slab = np.ascontiguousarray(slab, dtype=PACKET)
        self._chk(self.L.mgl_sa_set_best(self.h, _ptr(slab), perplexity))

    def best_packed(self):
        """packets_best in the packed device form (u64 per position) and its cost"""
        out = np.zeros(self.n, dtype=np.uint64)
        cost = C.c_uint64(0)
        self._chk(self.L.mgl_sa_best_packed(self.h, _ptr(out), C.byref(cost)))
        return out, cost.value

    def best_cost(self) -> int:
        cost = C.c_uint64(0)
        self._chk(self.L.mgl_sa_best_packed(self.h, None, C.byref(cost)))
        return cost.value

    def adopt_best_packed(self, packed, perplexity: int):
        packed = np.ascontiguousarray(packed, dtype=np.uint64)
        assert len(packed) == self.n
        self._chk(self.L.mgl_sa_adopt_best_packed(self.h, _ptr(packed), perplexity))

    def exchange_best(self, comm: "Comm"):
        """collective over the communicator's ranks (RCCL); returns (winner rank, winner cost)"""
        w, c = C.c_int(-1), C.c_uint64(0)
        self._chk(self.L.mgl_sa_exchange_best(self.h, comm.h, C.byref(w), C.byref(c)))
        return w.value, c.value

    def crossover(self, parents, grain: int = 0):
        """The child of 2..8 valid parses (mgl_crossover; parity hook, SA state untouched): between the positions where all
        the walks agree (about one cut per `grain` bytes, 0 = 64, 1 = every joint) the entries of whichever parent codes the
        stretch most cheaply.  Returns (child slab, stats dict: parent_cost, child_cost, predicted, boundaries, regions_from,
        gpu_ms)."""
        keep = [np.ascontiguousarray(p, dtype=PACKET) for p in parents]
        if any(len(p) != self.n for p in keep):
            raise MglError("crossover: every parent must have one entry per input byte", rc=-1)
        arr = (C.c_void_p * max(1, len(keep)))(*[p.ctypes.data for p in keep])
        child = np.zeros(self.n, dtype=PACKET)
        st = CrossStats()
        self._chk(self.L.mgl_crossover(self.h, arr, len(keep), grain, _ptr(child), C.byref(st)))
        return child, st.asdict()

    def cross_best(self, slab, grain: int = 0) -> dict:
        """Cross the best slab with `slab` (mgl_sa_cross_best): the child becomes the best slab if it is cheaper than both,
        else `slab` if it is cheaper than the best; stats["adopted"] = 0 own best kept, 1 `slab`, 2 the child."""
        slab = np.ascontiguousarray(slab, dtype=PACKET)
        if len(slab) != self.n:
            raise MglError("cross_best: the slab must have one entry per input byte", rc=-1)
        st = CrossStats()
        self._chk(self.L.mgl_sa_cross_best(self.h, _ptr(slab), grain, C.byref(st)))
        return st.asdict()

    def exchange_cross(self, comm: "Comm", grain: int = 0):
        """exchange_best's collectives, then every rank but the winner crosses its best slab with the winner's
        (mgl_sa_exchange_cross; collective).  Returns (winner rank, winner cost, this rank's stats dict)."""
        w, c = C.c_int(-1), C.c_uint64(0)
        st = CrossStats()
        self._chk(self.L.mgl_sa_exchange_cross(self.h, comm.h, grain, C.byref(w), C.byref(c), C.byref(st)))
        return w.value, c.value, st.asdict()

    def exchange_cross_all(self, comm: "Comm", grain: int = 0) -> dict:
        """Cross the distinct best slabs of all chains, the 8 cheapest at most (mgl_sa_exchange_cross_all; collective): every
        rank makes the same child and takes it if it is cheaper than the cheapest parent, which the dearer ranks adopt
        otherwise.  Returns the stats dict: chains_with_best, distinct, parent_rank, own_parent (None: not a parent),
        fell_back, cross (as from crossover, with adopted = 0 nothing, 1 the cheapest parent, 2 the child)."""
        st = CrossAllStats()
        self._chk(self.L.mgl_sa_exchange_cross_all(self.h, comm.h, grain, C.byref(st)))
        return st.asdict()

    def slab_hash(self, slab=None) -> int:
        """mgl_slab_hash of `slab` (None: the best slab), stale entries included; parity hook, SA state untouched"""
        if slab is not None:
            slab = np.ascontiguousarray(slab, dtype=PACKET)
            if len(slab) != self.n:
                raise MglError("slab_hash: the slab must have one entry per input byte", rc=-1)
        out = C.c_uint64(0)
        self._chk(self.L.mgl_slab_hash(self.h, _ptr(slab), C.byref(out)))
        return out.value

    def run(self, steps: int) -> dict:
        st = Stats()
        self._chk(self.L.mgl_sa_run(self.h, steps, C.byref(st)))
        return st.asdict()

    def current(self):
        out = np.zeros(self.n, dtype=PACKET)
        cost = C.c_uint64(0)
        self._chk(self.L.mgl_sa_current(self.h, _ptr(out), C.byref(cost)))
        return out, cost.value

    def best(self):
        out = np.zeros(self.n, dtype=PACKET)
        cost = C.c_uint64(0)
        self._chk(self.L.mgl_sa_best(self.h, _ptr(out), C.byref(cost)))
        return out, cost.value

    def cost_slab(self, slab, want_cum=True):
        slab = np.ascontiguousarray(slab, dtype=PACKET)
        total, npk = C.c_uint64(0), C.c_size_t(0)
        cum = np.zeros(self.n, dtype=np.uint64) if want_cum else None
        self._chk(self.L.mgl_cost_slab(self.h, _ptr(slab), C.byref(total), _ptr(cum), C.byref(npk)))
        return dict(total=total.value, npackets=npk.value, cum=None if cum is None else cum[: npk.value].copy())

    def props_sweep(self, slab=None):
        """Exact cost of `slab` (None: the current slab) under every triple of PROPS_TRIPLES, whatever the handle's own
        (mgl_props_sweep; SA state untouched).  Returns (75 uint64 costs in canonical order, device ms of the sweep)."""
        if slab is not None:
            slab = np.ascontiguousarray(slab, dtype=PACKET)
        out = (PropsCost * len(PROPS_TRIPLES))()
        cnt, ms = C.c_size_t(0), C.c_double(0)
        self._chk(self.L.mgl_props_sweep(self.h, _ptr(slab), out, len(out), C.byref(cnt), C.byref(ms)))
        assert cnt.value == len(PROPS_TRIPLES)
        assert [(e.props.lc, e.props.lp, e.props.pb) for e in out] == PROPS_TRIPLES
        return np.array([e.cost for e in out], dtype=np.uint64), ms.value

    def _own_slab(self, slab, who):
        if slab is None:
            return None
        slab = np.ascontiguousarray(slab, dtype=PACKET)
        if len(slab) != self.n:
            raise MglError(f"{who}: the slab must have one entry per input byte", rc=-1)
        return slab

    def segment_cuts(self, grain=0, slab=None):
        """The cut points of the grain rule on the walk of `slab` (None: the current slab): 0, then every multiple of
        max(grain, ceil(n / 16)) below n moved up to the next packet start, then n (mgl_segment_cuts; grain 0 = 65536)."""
        slab = self._own_slab(slab, "segment_cuts")
        out = np.zeros(SEG_MAX_CUTS, dtype=np.uint64)
        cnt = C.c_size_t(0)
        self._chk(self.L.mgl_segment_cuts(self.h, _ptr(slab), grain, _ptr(out), len(out), C.byref(cnt)))
        return [int(c) for c in out[: cnt.value]]

    def props_sweep_spans(self, cuts, slab=None):
        """Exact cost of every span [cuts[i], cuts[j]) of `slab` (None: the current slab), coded from a state reset at its
        start, under every triple of PROPS_TRIPLES (mgl_props_sweep_spans; SA state untouched).  Returns (uint64 table of
        shape (spans, 75), row span_index(i, j, len(cuts) - 1); device ms)."""
        slab = self._own_slab(slab, "props_sweep_spans")
        cuts = np.ascontiguousarray(cuts, dtype=np.uint64)
        m = max(len(cuts) - 1, 0)
        spans = m * (m + 1) // 2 if len(cuts) <= SEG_MAX_CUTS else 0
        out = np.zeros(max(spans, 1) * len(PROPS_TRIPLES), dtype=np.uint64)
        cnt, ms = C.c_size_t(0), C.c_double(0)
        self._chk(self.L.mgl_props_sweep_spans(self.h, _ptr(slab), _ptr(cuts), len(cuts), _ptr(out), len(out), C.byref(cnt),
                                               C.byref(ms)))
        assert cnt.value == spans * len(PROPS_TRIPLES)
        return out[: cnt.value].reshape(spans, len(PROPS_TRIPLES)).copy(), ms.value

    def segment_props(self, grain=0, slab=None):
        """The cheapest segmentation of `slab` (None: the current slab) over the grain's cuts, every segment under its own
        triple behind an LZMA2 state reset (mgl_sa_segment_props).  Returns dict(segments=[lo, hi, props, cost ...], total,
        single_best, gpu_ms): total = the segments' costs + SEG_OVERHEAD per segment after the first, never above
        single_best, the cost under the best one triple."""
        slab = self._own_slab(slab, "segment_props")
        segs = (Segment * (SEG_MAX_CUTS - 1))()
        nseg, total, single, ms = C.c_size_t(0), C.c_uint64(0), C.c_uint64(0), C.c_double(0)
        self._chk(self.L.mgl_sa_segment_props(self.h, _ptr(slab), grain, segs, len(segs), C.byref(nseg), C.byref(total),
                                              C.byref(single), C.byref(ms)))
        return dict(segments=[segs[k].asdict() for k in range(nseg.value)], total=total.value, single_best=single.value,
                    gpu_ms=ms.value)

    def segment_reparse(self, segs, slab=None, passes: int = 0, cand: int = 0, chunk: int = 0, segment: int = 0, ahead: int = 0,
                        from_current: bool = False):
        """The adaptive parse made again inside every segment of `segs` (dicts lo, hi, props that tile the input at packet
        starts of `slab`; None: the current slab), each from its LZMA2 state reset and under its own triple
        (mgl_segment_reparse; SA state untouched; the settings are seed_adaptive's, from_current is refused).  Returns
        (slab, segs, stats, taken, gpu_ms): the joined slab and the same segments with cost = final_cost -- what
        emit_xz_segments takes --, per segment dict(passes, best_pass (None: its packets were kept), start_cost, final_cost,
        pass_cost, objective), and whether the result is the joined slab (True) or the input handed back because the
        join did not cost less (False)."""
        slab = self._own_slab(slab, "segment_reparse")
        nseg = len(segs)
        out = np.zeros(self.n, dtype=PACKET)
        segs_out = (Segment * max(nseg, 1))()
        st = (SegmentParseStats * max(nseg, 1))()
        taken, ms = C.c_int(0), C.c_double(0)
        cfg = AdaptiveConfig(passes, cand, chunk, segment, ahead, int(from_current))
        self._chk(self.L.mgl_segment_reparse(self.h, _ptr(slab), _segments(segs), nseg, C.byref(cfg), _ptr(out), segs_out, st,
                                             C.byref(taken), C.byref(ms)))
        return (out, [segs_out[k].asdict() for k in range(nseg)], [st[k].asdict() for k in range(nseg)], bool(taken.value),
                ms.value)

    def cost_map(self, slab=None, props=None):
        """Where `slab` (None: the current slab) spends its bits under props = (lc, lp, pb) (None: the handle's; another
        triple is allowed, as in props_sweep) (mgl_cost_map; SA state untouched).  Returns (uint32 map, report dict) as
        host_cost_map does, the report with gpu_ms, the device time of the call's kernels."""
        if slab is not None:
            slab = np.ascontiguousarray(slab, dtype=PACKET)
            if len(slab) != self.n:
                raise MglError("cost_map: the slab must have one entry per input byte", rc=-1)
        pr = None if props is None else C.byref(Properties(*props))
        out = np.zeros(self.n, dtype=np.uint32)
        rep = CostReport()
        self._chk(self.L.mgl_cost_map(self.h, _ptr(slab), pr, _ptr(out), C.byref(rep)))
        return out, rep.asdict(device=True)

    def cost_map_live(self):
        """cost_map() of the current slab under the handle's triple, read off the engine's event chains instead of walked
        (mgl_cost_map_live; SA state untouched): the same integers, gpu_ms apart."""
        out = np.zeros(self.n, dtype=np.uint32)
        rep = CostReport()
        self._chk(self.L.mgl_cost_map_live(self.h, _ptr(out), C.byref(rep)))
        return out, rep.asdict(device=True)

    def final_state(self, slab):
        slab = np.ascontiguousarray(slab, dtype=PACKET)
        probs = np.zeros(self.nprobs, dtype=np.uint16)
        cs = C.c_uint8(0)
        dists = np.zeros(4, dtype=np.uint32)
        self._chk(self.L.mgl_final_state(self.h, _ptr(slab), _ptr(probs), self.nprobs, C.byref(cs), _ptr(dists)))
        return dict(probs=probs, ctx_state=cs.value, dists=dists)

    def top_k(self, slab, position, form=None):
        """form: probe this form of the search from now on (KEY.PROBE_FORM: 0 batched set-up, 1 in place)"""
        if form is not None:
            self.debug_set(KEY.PROBE_FORM, form)
        slab = np.ascontiguousarray(slab, dtype=PACKET)
        out = np.zeros(64, dtype=PACKET)
        costs = np.zeros(64, dtype=np.uint64)
        cnt = C.c_size_t(0)
        self._chk(self.L.mgl_top_k(self.h, _ptr(slab), position, _ptr(out), _ptr(costs), C.byref(cnt)))
        return out[: cnt.value].copy(), costs[: cnt.value].copy()

    def substrings(self, pos, max_len=273, cap=1 << 20):
        offs = np.zeros(cap, dtype=np.uint32)
        lens = np.zeros(cap, dtype=np.uint32)
        cnt = C.c_size_t(0)
        self._chk(self.L.mgl_substrings(self.h, pos, max_len, _ptr(offs), _ptr(lens), cap, C.byref(cnt)))
        assert cnt.value <= cap
        return offs[: cnt.value].copy(), lens[: cnt.value].copy()

    def batch_counters(self):
        """(bulk steps whose moves were patched into the base by the batch accept, bulk steps that began one and fell back to the rebuild)"""
        v = self.debug_dump(DUMP.BATCH_COUNTS)
        return int(v[0]), int(v[1])

    def batch_giveups(self) -> int:
        """bulk steps that began a batch accept and left the step to the rebuild before anything was touched (a cluster's journal
        or a walk gave up: status 2 with a failure seen)"""
        return int(self.debug_dump(DUMP.BATCH_COUNTS)[2])

    def giveup_sites(self) -> int:
        """give-up sites of the in-place accepts seen since the last call (GU bits); reading clears"""
        return int(self.debug_dump(DUMP.GIVEUP_SITES)[0])

    def set_limit(self, limit_id: int, value: int):
        """KEY.LIMIT: lower limit `limit_id` (LIM) of the in-place accepts; set_limit(0, 0) restores every default"""
        self.debug_set(KEY.LIMIT, limit_id | (value << 8))

    def debug_set(self, key: int, value: int):
        self._chk(self.L.mgl_debug_set(self.h, key, value))

    def debug_dump(self, what: int, dtype=None) -> np.ndarray:
        """one of the engine's structures (DUMP), as elements of `dtype` (default: the selector's own, DUMP_DTYPE)"""
        if dtype is None:
            dtype = DUMP_DTYPE[DUMP(what)]
        need = C.c_size_t(0)
        probe = np.zeros(1, dtype=np.uint8)
        self.L.mgl_debug_dump(self.h, what, _ptr(probe), 0, C.byref(need))
        out = np.zeros(max(1, need.value), dtype=np.uint8)
        self._chk(self.L.mgl_debug_dump(self.h, what, _ptr(out), need.value, C.byref(need)))
        return out[: need.value].view(dtype)

    def neighbours(self, global_step: int, want_diffs=True, diff_cap=64):
        costs = np.zeros(self.K, dtype=np.uint64)
        nd = np.zeros(self.K, dtype=np.uint32)
        diffs = np.zeros((self.K, diff_cap), dtype=DIFF) if want_diffs else None
        self._chk(self.L.mgl_neighbours(self.h, global_step, _ptr(costs), _ptr(diffs), _ptr(nd), diff_cap))
        return costs, nd, diffs


class Comm:
    """One communicator behind the C ABI (mgl_comm_*).  Comm(uid, rank, world, device): RCCL, rank 0 makes the id and
    every rank joins.  Comm.shm(path, nonce, rank, world, device): the library's host shared-memory transport."""

    @classmethod
    def shm(cls, path: str, nonce: int, rank: int, world: int, device: int = 0) -> "Comm":
        self = cls.__new__(cls)
        self.L = hip_lib()
        self.h = C.c_void_p()
        if self.L.mgl_comm_init_shm(C.byref(self.h), os.fsencode(path), nonce, rank, world, device) != 0:
            self.h = None
            raise MglError(self.L.mgl_last_error().decode())
        self.rank, self.world = rank, world
        return self

    def min_u64(self, mine: int) -> int:
        out = C.c_uint64(0)
        if self.L.mgl_comm_min_u64(self.h, mine, C.byref(out)) != 0:
            raise MglError(self.L.mgl_last_error().decode())
        return out.value

    def allgather_u64(self, mine: int) -> list:
        """every rank's word in rank order (mgl_comm_allgather_u64: host transport only)"""
        out = (C.c_uint64 * self.world)()
        if self.L.mgl_comm_allgather_u64(self.h, mine, out) != 0:
            raise MglError(self.L.mgl_last_error().decode())
        return list(out)

    @staticmethod
    def unique_id() -> bytes:
        L = hip_lib()
        buf = (C.c_uint8 * 128)()
        if L.mgl_comm_unique_id(buf) != 0:
            raise MglError(L.mgl_last_error().decode())
        return bytes(buf)

    def __init__(self, uid: bytes, rank: int, world: int, device: int):
        self.L = hip_lib()
        assert len(uid) == 128
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self.h = C.c_void_p()
        if self.L.mgl_comm_init(C.byref(self.h), buf, rank, world, device) != 0:
            raise MglError(self.L.mgl_last_error().decode())
        self.rank, self.world = rank, world

    def close(self):
        if getattr(self, "h", None):
            self.L.mgl_comm_destroy(self.h)
            self.h = None

    __del__ = close
