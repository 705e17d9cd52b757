// The count table's state record (csrc/eref_table_state.hpp) on its own: every state of tests/eref_state_cases.py reached by the
// named transitions, every guard's answer printed (tests/test_host_eref_state.py compares them with the table of expectations).
#include <cstdio>

#include "../csrc/eref_table_state.hpp"

using palace::TableState;

static char g_obj[3];
static const palace_eref_probe_index *const IX = reinterpret_cast<const palace_eref_probe_index *>(&g_obj[0]);      // the attached index
static const palace_eref_probe_index *const IX2 = reinterpret_cast<const palace_eref_probe_index *>(&g_obj[1]);     // a second build of it
static const void *const BLOCK = &g_obj[2];                                                                         // IX's count block
constexpr long long N = 36000;                             // positions of the count that reaches the states

static void show(const char *name, const TableState &t)
{
    std::printf("%s clean=%d takes_counts=%d planes_readable=%d scan_ix=%d scan_other=%d hit_sets_ix=%u hit_sets_other=%u sentinels_ix=%d "
                "partial_allowed=%d counts_in_block=%d first_plane=%d keys=%lld sparse=%d\n",
                name, t.clean(), t.takes_counts(), t.planes_readable(), t.scannable_through(IX), t.scannable_through(IX2), t.hit_sets_for(IX),
                t.hit_sets_for(IX2), t.sentinels_placed_for(IX), t.partial_count_allowed(), t.counts_lie_in(BLOCK), t.first_plane_to_clear(),
                static_cast<long long>(t.keys_counted), t.known_sparse());
}

static TableState counting()                               // reset, and a binned count begun
{
    TableState t;
    t.allocated_zeroed();
    t.reset();
    t.keys_added(3 * N);
    t.count_started();
    return t;
}

int main()
{
    TableState t;
    show("new", t);
    t.allocated_zeroed();
    show("allocated", t);
    t.reset();
    show("Z", t);
    t = counting(); t.counted_plain();
    show("P", t);
    t.planes_unknown();
    show("U", t);
    t = counting(); t.counted_final();
    show("T", t);
    t = counting(); t.counted_final_channel0(IX);
    show("T0", t);
    const TableState t0 = t;
    t = counting(); t.counted_final_all_sets(IX);
    show("H", t);
    t = counting(); t.counted_partial(BLOCK);
    show("C", t);
    t.hits_whole(IX, 3 * N);
    show("W", t);
    t.reset();
    t.partial_counts_zeroed(BLOCK);
    show("C0", t);
    t.hits_whole(IX, -1);
    show("C0+whole", t);
    t.merged();                                            // the merge drops the record like every other write of the planes
    show("C0+whole+merged", t);
    // every transition that writes planes, from a table with a fused record: the record is gone afterwards
    t = t0; t.count_started(); show("T0+count_started", t);
    t = t0; t.counted_direct(); show("T0+counted_direct", t);
    t = t0; t.counted_plain(); show("T0+counted_plain", t);
    t = t0; t.merged(); show("T0+merged", t);
    t = t0; t.unpacked_sparse(); show("T0+unpacked", t);    // (stays top-only, keys as they were)
    t = t0; t.counted_final(); show("T0+counted_final", t);
    t = t0; t.counted_partial(BLOCK); show("T0+counted_partial", t);
    t = t0; t.planes_unknown(); show("T0+unknown", t);
    t = t0; t.reset(); show("T0+reset", t);
    // ... and what leaves the planes alone but takes the index or its blocks away
    t = t0; t.index_gone(IX2); show("T0+other_index_gone", t);
    t = t0; t.index_gone(IX); show("T0+index_gone", t);
    t = t0; t.index_detached(); show("T0+detached", t);
    t = counting(); t.counted_partial(BLOCK); t.count_block_detached(); show("C+block_detached", t);
    t.reset(); t.unpacked_sparse(); show("Z+unpacked", t);
    return 0;
}
