// eref: what the count table of a context holds, as ONE record with named transitions and guards (no HIP in here: a plain host
// program includes this file on its own -- host/eref_state_selftest_main.cpp).  palace_ctx::table is the only instance; no other
// file assigns or tests its members.
//
//   planes    fused record   reached by                                                  accepts
//   Zero      -              reset                                                       counts, merges, lookups, plane reads, scans
//   Zero      all, unplaced  a partial count of no reads, then hits_whole                the same, and the indexed scan starts from the record
//   Three     -              a count, a merge, an unpack into Zero, attach, invalidate   the same as Zero
//   Top       - / channel 0  a final count (option final_count)                          plane reads, scans
//   Nothing   all, placed    a final count that tested every entry set itself            the indexed scan through that index
//   Nothing   -              ... that left partial counts (probe_all_sets 2)             nothing, until hits_whole
//   Nothing   all, unplaced  ... then hits_whole                                         the indexed scan through that index
//
// Every transition that writes planes drops the fused record -- counts, merges and unpacks alike -- so a record never describes
// planes that have moved on.
//
// Kept exactly as they were, on purpose:
//  * palace_eref_table_reset memsets all three planes even from Zero (first_plane_to_clear is 0 there): it skips planes only after
//    a final count (Top: two) or a plane-less one (Nothing: all three).  Skipping from Zero would change the step's time.
//  * A count call with no reads or positions returns OK before any guard of this file is asked; under probe_all_sets 2 it goes
//    through partial_count_allowed() first and then zeroes the count block (partial_counts_zeroed).
//  * unpacked_sparse() leaves keys_counted as it was: that value picks the pruning order of the indexed scan in the sparse
//    multi-GPU scheme (both orders are exact, one is faster), and the ranks' shares do not change how full the table is known to be.
//  * After partial_counts_zeroed() the planes are still Zero: the table is neither final nor plane-less, and plain scans, merges and
//    lookups are accepted.
// Known hole, left for later: counts_block survives a plain count, so a caller that switches probe_all_sets off, counts, and switches
// it on again after a partial count of no reads can still declare stale (zero) counts whole.
#pragma once
#include <cstdint>

struct palace_eref_probe_index;

namespace palace {

constexpr uint32_t kAllEntrySets = 0xfu;      // channels 0, 1, 2 and the sentinels of a probe index

// the two refusals of a table that is not in the state a call needs (PALACE_REQUIRE puts the caller's name in front)
constexpr char kTableTopOnly[] = "the table holds only its \">= 3\" plane (option final_count): reset it first";
constexpr char kTableHoldsNothing[] =
    "the table holds nothing (option probe_all_sets: its last count tested the attached index and wrote no plane): reset it first";

struct TableState {
    enum class Planes : uint8_t {
        Zero,        // every bit of the three planes is zero, and known to be
        Three,       // three planes: counted, merged, or of unknown content (also: not allocated yet)
        Top,         // only the ">= 3" plane; the two lower ones are all zero
        Nothing      // all zero, but NOT the result: that lives in an index's blocks
    };
    Planes planes = Planes::Three;
    int64_t keys_counted = 0;        // key instances behind the planes since the last reset (an upper bound); -1: unknown
    // the hit bits a count launch (or hits_whole) left in an index's blocks, complete for the table as it stands
    const palace_eref_probe_index *fused_ix = nullptr;
    uint32_t fused_sets = 0;         // bit k: entry set k (bit 0 alone: channel 0 rode along; kAllEntrySets: all four)
    bool sentinels_placed = false;   // ... and the sentinels' hits are in position order already
    const void *counts_block = nullptr;   // probe_all_sets 2: the count block that holds this context's partial counts since the last reset

    // ---- guards -----------------------------------------------------------------------------------------------------
    bool clean() const { return planes == Planes::Zero; }
    bool takes_counts() const { return planes == Planes::Zero || planes == Planes::Three; }     // ... merges, lookups, pack_low
    bool planes_readable() const { return planes != Planes::Nothing; }
    uint32_t hit_sets_for(const palace_eref_probe_index *ix) const { return ix && fused_ix == ix ? fused_sets : 0u; }   // sets the scan may start from
    bool sentinels_placed_for(const palace_eref_probe_index *ix) const { return hit_sets_for(ix) == kAllEntrySets && sentinels_placed; }
    bool scannable_through(const palace_eref_probe_index *ix) const { return planes_readable() || hit_sets_for(ix) == kAllEntrySets; }
    bool partial_count_allowed() const { return clean() && !counts_block; }                     // one partial count per reset
    bool counts_lie_in(const void *block) const { return counts_block && counts_block == block; }
    bool known_sparse() const { return keys_counted >= 0 && keys_counted < static_cast<int64_t>(0.9 * 4294967296.0); }
    int first_plane_to_clear() const { return planes == Planes::Nothing ? 3 : planes == Planes::Top ? 2 : 0; }   // what a reset memsets

    // ---- transitions, one per event -----------------------------------------------------------------------------------
    void reset() { *this = TableState{}; planes = Planes::Zero; }
    void allocated_zeroed() { planes = Planes::Zero; }                          // the planes' first allocation
    void planes_unknown() { *this = TableState{}; keys_counted = -1; }         // attached from outside, or declared unknown
    void keys_added(int64_t n) { if (keys_counted >= 0) keys_counted += n; }
    void count_started() { drop_hits(); }                                       // (the partition kernels' overflow path writes planes at once)
    void counted_direct() { wrote(Planes::Three); }
    void merged() { wrote(Planes::Three); keys_counted = -1; }                  // (other ranks' keys: how many is not known here)
    void unpacked_sparse() { wrote(planes == Planes::Zero ? Planes::Three : planes); }
    // a binned count finished ...
    void counted_plain() { wrote(Planes::Three); }
    void counted_final() { wrote(Planes::Top); }
    void counted_final_channel0(const palace_eref_probe_index *ix) { wrote(Planes::Top); fused_ix = ix; fused_sets = 1u; }
    void counted_final_all_sets(const palace_eref_probe_index *ix)
    {
        wrote(Planes::Nothing); fused_ix = ix; fused_sets = kAllEntrySets; sentinels_placed = true;
    }
    void counted_partial(const void *block) { wrote(Planes::Nothing); counts_block = block; }
    void partial_counts_zeroed(const void *block) { drop_hits(); counts_block = block; }        // a rank without reads
    void hits_whole(const palace_eref_probe_index *ix, int64_t keys_of_all_ranks)
    {
        fused_ix = ix; fused_sets = kAllEntrySets; sentinels_placed = false;
        keys_counted = keys_of_all_ranks;
    }
    void index_gone(const palace_eref_probe_index *ix) { if (fused_ix == ix) drop_hits(); }    // freed, or its buffers re-pointed
    void index_detached() { drop_hits(); }
    void count_block_detached() { counts_block = nullptr; }

private:
    void drop_hits() { fused_ix = nullptr; fused_sets = 0; sentinels_placed = false; }
    void wrote(Planes now) { planes = now; drop_hits(); }
};

}  // namespace palace
