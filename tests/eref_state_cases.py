"""What the count table of a context accepts in each of its states: ONE table of expectations, used by the CPU test of the state
record (tests/test_host_eref_state.py: csrc/eref_table_state.hpp through its stand-alone selftest) and by the walk of the same matrix
through the C ABI on a device (tests/test_gpu_eref_state.py).

The states, and how a test reaches them (options stay as they were set to reach the state):
    Z   reset
    P   reset, count
    U   P, then invalidate
    T   option final_count 1, no index attached: reset, count
    T0  T with an index attached: channel 0 rides along in the count
    H   T0 with option probe_all_sets 1: every entry set rides along, no plane is written
    C   option probe_all_sets 2 with a count block attached: reset, count -- partial counts
    C0  C with zero reads
    W   C, then entry_hits_from_counts (one part) and entry_hits_complete
Every call gets arguments that do real work (n > 0, a 16-byte all-zero merge part, ten lookup keys, a one-bucket sparse share) and meets a
freshly established state."""

STATES = ("Z", "P", "U", "T", "T0", "H", "C", "C0", "W")
ALL = frozenset(STATES)
ATTACHED = frozenset(("T0", "H", "C", "C0", "W"))      # an index is attached to the context
PARTIAL = frozenset(("C", "C0", "W"))                  # option probe_all_sets is 2


def _all_but(*states):
    return ALL - frozenset(states)


# call -> the states that accept it; every other state refuses it (an error return, the table and the index's blocks untouched)
ACCEPTED = {
    "count_reads": frozenset("ZPU"),
    "count_reads_packed": frozenset("ZPU"),
    "merge_slices": frozenset(("Z", "P", "U", "C0")),
    "merge_slices_packed": frozenset(("Z", "P", "U", "C0")),
    "pack_low": frozenset(("Z", "P", "U", "C0")),
    "lookup": frozenset(("Z", "P", "U", "C0")),
    "table_planes": _all_but("H", "C", "W"),
    "plane_pack": _all_but("H", "C", "W"),
    "plane_unpack": _all_but("H", "C", "W"),
    "popcounts": _all_but("H", "C", "W"),
    "scan_refs": _all_but("H", "C", "W"),
    "scan_refs_indexed": _all_but("C"),                # with the attached index (in Z, P, U, T: the index that would be attached)
    "scan_refs_indexed_other": _all_but("H", "C", "W"),      # with a second build of the same index
    # (W as well: the counts still lie in the index's block, so declaring the hit bits whole a second time is accepted)
    "entry_hits_complete": frozenset(("C", "C0", "W")),
    "reset": ALL,
    "invalidate": ALL,
    "attach_probe_index_null": ALL,
}

TOP_ONLY = frozenset(("T", "T0"))                      # popcounts read [0, 0, n]
ROWS_SURVIVE_REFUSALS = frozenset(("H", "W"))          # after every refused call the indexed scan still returns the rows it returned before

# the planes a reset has to clear in each state (all three even from Z: the step's time depends on it)
FIRST_PLANE_TO_CLEAR = {"Z": 0, "P": 0, "U": 0, "T": 2, "T0": 2, "H": 3, "C": 3, "C0": 0, "W": 3}


def accepted_by_guards(call, state, g):
    """the same answer from the guards of the state record (g: guard name -> int, one line of the selftest's output) and the options the
    state was reached under -- what the entry points of the library ask, in their words"""
    if call in ("count_reads", "count_reads_packed"):
        return bool(g["takes_counts"]) and (state not in PARTIAL or bool(g["partial_allowed"]))
    if call in ("merge_slices", "merge_slices_packed", "pack_low", "lookup"):
        return bool(g["takes_counts"])
    if call in ("table_planes", "plane_pack", "plane_unpack", "popcounts", "scan_refs"):
        return bool(g["planes_readable"])
    if call == "scan_refs_indexed":
        return bool(g["scan_ix"])
    if call == "scan_refs_indexed_other":
        return bool(g["scan_other"])
    if call == "entry_hits_complete":
        return state in PARTIAL and bool(g["counts_in_block"])
    assert call in ("reset", "invalidate", "attach_probe_index_null"), call
    return True
