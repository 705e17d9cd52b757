/*
 * palace_hip.h -- C ABI of the MI355X (gfx950) conjugate-graph hot path.
 *
 * The reference has no FFI/plugin boundary: its hot path is three executables coupled by files
 * (SURVEY.md section 8(b)).  This library is the layer the replacement executables
 * (palace_amd/host/{eref,generateGraph,matching}_main.cpp) call; each entry point names the
 * reference code it stands in for.  Plain pointers and sizes only; `d_` arguments are device
 * (HBM) pointers, everything else is host memory.  Every function returns 0 on success and a
 * negative PALACE_E* code on failure; palace_last_error() gives the message for the calling
 * thread.  No exceptions cross this boundary.  A context is bound to one device and one HIP
 * stream; calls on one context are ordered, distinct contexts are independent (one process per
 * GPU is the intended deployment).
 */
#ifndef PALACE_HIP_H
#define PALACE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PALACE_OK 0
#define PALACE_EINVAL (-1)   /* bad argument (null pointer, negative size, shape mismatch) */
#define PALACE_EHIP (-2)     /* a HIP runtime call failed */
#define PALACE_ENOMEM (-3)   /* device or host allocation failed */
#define PALACE_ESTATE (-4)   /* call sequence error (e.g. coder not set) */

typedef struct palace_ctx palace_ctx;

const char *palace_last_error(void);
const char *palace_version(void);

/* ---- context, memory, stream plumbing --------------------------------------------------- */
/* A context owns one HIP stream, the eref count table, grow-only device / pinned / host scratch.  Calls on ONE context
 * must come from one thread at a time (they are ordered on its stream); DIFFERENT contexts may be used concurrently from
 * different threads and their work overlaps on the device.  palace_last_error() is per thread. */
int palace_ctx_create(int device, palace_ctx **out);
/* same, with the context's stream at the device's highest priority when high_priority != 0 (for
 * small latency-bound work that runs beside bulk kernels of another context) */
int palace_ctx_create_prio(int device, int high_priority, palace_ctx **out);
/* A context on the CALLER's stream (a hipStream_t): every call of the context enqueues there, so the caller's own work on that
 * stream -- collectives, copies -- is ordered with the library's kernels without events or waits.  The stream is not
 * destroyed with the context. */
int palace_ctx_create_on_stream(int device, void *hip_stream, palace_ctx **out);
int palace_ctx_destroy(palace_ctx *ctx);
int palace_sync(palace_ctx *ctx);
/* raw hipStream_t of the context (for callers that want to order their own work / events) */
void *palace_stream(palace_ctx *ctx);
int palace_malloc(palace_ctx *ctx, size_t bytes, void **d_out);
int palace_free(palace_ctx *ctx, void *d_ptr);
int palace_memset(palace_ctx *ctx, void *d_ptr, int value, size_t bytes);
int palace_h2d(palace_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int palace_d2h(palace_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
int palace_d2d(palace_ctx *ctx, void *d_dst, const void *d_src, size_t bytes);
/* Streaming ingest (the reference reads its inputs with T threads per phase, extract_ref.cpp:1267-1291,
 * and streams the BAM, generate_graph.cpp:644): page-locked host staging buffers, and a host-to-device copy that only
 * enqueues -- the source must stay untouched until a later palace_mark() on the stream has been waited for with
 * palace_mark_wait() (or palace_sync()). */
int palace_host_alloc(palace_ctx *ctx, size_t bytes, void **h_out);
int palace_host_free(palace_ctx *ctx, void *h_ptr);
int palace_h2d_async(palace_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
/* ... and the other way (results of one batch fetched while the next batch is being enqueued): h_dst page-locked, its
 * content is there once a later palace_mark() on the stream has been waited for. */
int palace_d2h_async(palace_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
/* HIP-event timing on the context's stream: begin/end bracket, elapsed in milliseconds. */
int palace_timer_begin(palace_ctx *ctx);
int palace_timer_end(palace_ctx *ctx, float *ms_out);
/* Non-blocking variant for timing kernels inside a longer timed region: mark(i) records event i
 * (0 <= i < 4096) on the stream; mark_elapsed(a, b) waits for event b and returns b - a in ms. */
int palace_mark(palace_ctx *ctx, int i);
int palace_mark_elapsed(palace_ctx *ctx, int a, int b, float *ms_out);
int palace_mark_wait(palace_ctx *ctx, int i);
/* the same with a deadline: polls the mark and gives up after `seconds` (PALACE_ESTATE; the work is still enqueued -- a caller
 * that cannot wait any longer for a device has to leave without touching what that work writes) */
int palace_mark_wait_for(palace_ctx *ctx, int i, double seconds);
/* Orders two contexts on the device without the host: work enqueued on `ctx` after this call starts only when mark i of
 * `other` (recorded before this call) has been reached on other's stream. */
int palace_wait_for_mark(palace_ctx *ctx, palace_ctx *other, int i);

/* ---- eref: k-mer screening of reads against the phage DB (bin/extract_ref.cpp) ---------- */

/* E1. Install the per-position coder permutation from the 400-byte index header
 * (replaces generate_coder/generate_base/generate_complement/saved_random_coder,
 * extract_ref.cpp:1010-1080, 1104-1122). */
int palace_eref_set_coder(palace_ctx *ctx, const uint8_t header400[400]);

/* E2. Index build for `n_refs` sequences resident in HBM (ASCII, 1 B/base, concatenated;
 * d_offsets has n_refs+1 entries).  For ref r and position j < len-31 writes the three canonical
 * 32-mer indices (0 = k-mer holds an invalid base) at d_out[d_out_offsets[r] + 3*j + i]
 * (replaces the index loops of read_ref, extract_ref.cpp:711-738, 773-799). */
int palace_eref_index_refs(palace_ctx *ctx, const uint8_t *d_bases, const int64_t *d_offsets,
                           int64_t n_refs, uint32_t *d_out, const int64_t *d_out_offsets);

/* E4. Count table.  reset zeroes it (extract_ref.cpp:1257); count_reads adds every 32-mer of
 * every read, all three channels, saturating at 3 (read_fastq, extract_ref.cpp:961-1000).
 * d_keep (optional, 1 B/read) carries the E3 subsampling decision (extract_ref.cpp:955-960).
 * total_bases = d_offsets[n_reads] - d_offsets[0] when the caller knows it (keeps the call
 * asynchronous), or -1 to have it read back.
 * The table is held as three 2^32-bit planes "count >= 1 / >= 2 / >= 3".  What it holds, and what it then accepts
 * (options: palace_eref_set_option; every other call in a state fails and changes nothing; reset, invalidate and attach always work):
 *   the table holds   after                                                   accepted
 *   zero planes       reset; a count of no reads under "probe_all_sets" 2     everything
 *   three planes      count, merge, plane_unpack into zero planes,            everything
 *                     table_attach, table_invalidate
 *   its top plane     a final count ("final_count")                           table_planes, plane_pack / _unpack, popcounts (0, 0, n),
 *                                                                             both scans
 *   nothing           a final count that tested every entry set of the        scan_refs_indexed with that index -- under
 *                     attached index ("probe_all_sets" 1 or 2)                "probe_all_sets" 2 only after entry_hits_complete
 * A count call with no reads or positions returns OK without looking at the table (under "probe_all_sets" 2 it is the rank's one
 * count per reset and zeroes the count block).  Hit bits a count launch left in an attached index (palace_eref_attach_probe_index, entry_hits_complete) are used by the
 * next indexed scan only while nothing has written the planes since: any count, merge, unpack, attach or reset drops them. */
int palace_eref_table_reset(palace_ctx *ctx);
/* Optional: allocate the table and the scratch memory a count_reads call over `total_bases` bases will need now (tens of
 * GB at a gigabase; the allocation alone can take from a millisecond to a second), e.g. while the caller is still parsing. */
int palace_eref_reserve(palace_ctx *ctx, int64_t total_bases);
int palace_eref_count_reads(palace_ctx *ctx, const uint8_t *d_bases, const int64_t *d_offsets,
                            int64_t n_reads, const uint8_t *d_keep, int64_t total_bases);

/* E4 with the read set already packed (replaces the same loop, extract_ref.cpp:927-1004, for a caller that packs while it
 * parses: 0.375 bytes per base cross PCIe instead of 1, and the kernels that derive the streams from ASCII do not run).
 * Three bit streams over the positions 0 .. n_positions-1 of the read set (bit p & 31 of 32-bit word p >> 5, little endian):
 *   P0[p] = base p is A or T,  P1[p] = base p is A or C   (either case; together the base itself -- what the reference's
 *           generate_base tables project, extract_ref.cpp:1010-1046);
 *   U[p]  = a 32-mer is counted at p: positions p .. p+31 lie in ONE read that is counted (E3 subsampling) and all are
 *           A/C/G/T -- the `n`/read-end/short-read tests of extract_ref.cpp:963-996.
 * Positions between reads that belong to no read (pads, e.g. to start every parser thread's part on a word) are allowed:
 * U = 0 there and the other two streams are not looked at.  Each stream: palace_eref_packed_bytes(n_positions) bytes of
 * device memory, 8-byte aligned (two words of look-ahead behind the last position are read, their content is ignored).
 * n_reads_hint: number of reads if known (picks the tile shape for short-read sets), else 0.  Same table, same
 * asynchrony as palace_eref_count_reads. */
size_t palace_eref_packed_bytes(int64_t n_positions);
/* The same three streams made on the device from a read set that is in HBM as ASCII (the arguments of
 * palace_eref_count_reads; positions = bases, no gaps): for a caller that counts one read set more than once -- the streams
 * do not depend on the coder, so one packing serves every DB -- or keeps its samples resident in the packed form. */
int palace_eref_pack_reads(palace_ctx *ctx, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_reads,
                           const uint8_t *d_keep, int64_t total_bases, uint32_t *d_p0, uint32_t *d_p1, uint32_t *d_u);
int palace_eref_count_reads_packed(palace_ctx *ctx, const uint32_t *d_p0, const uint32_t *d_p1, const uint32_t *d_u,
                                   int64_t n_positions, int64_t n_reads_hint);

/* Tuning knobs of count_reads (no reference counterpart; results are identical for every setting, which is what the
 * tests use them for).  set_count_mode: mode 0 = automatic (partition + LDS counting for large inputs, direct global
 * atomics for tiny ones), 1 = always direct, 2 = always partitioned; bucket_cap > 0 overrides the per-bucket capacity
 * of the partitioned path (keys beyond it take the direct path).  set_option(name, value):
 *   "slab_bases"  positions per slab that large read sets are processed in (multiple of 64; 0 = default 2^30 / 2^31)
 *   "final_count" 1: every count call from now on is the ONLY one between palace_eref_table_reset and the scan.  Phase B
 *                 reads nothing but the "count >= 3" plane (the slide tests `== least_depth`, extract_ref.cpp:23, :531, of a count that
 *                 saturates there, :995), so such a
 *                 call keeps the two lower planes in LDS only: they are not written (1 GB less per call) and stay zero, and
 *                 the next reset clears one plane instead of three.  Afterwards the table cannot take further counts,
 *                 merges or lookups until it is reset (those calls fail); popcounts report 0, 0, n.  Applies to binned
 *                 counts of one slab into a clean table, otherwise the call behaves as without the option.  0: off (default).
 *   "probe_all_sets" 1: a final count (see "final_count") with a probe index attached (palace_eref_attach_probe_index) tests ALL of the
 *                 index's entries -- the three channels of every DB position and the sentinels -- against each fine bucket's ">= 3"
 *                 slice while it is in LDS, and does not write the slice: the table's planes stay all zero (slices the overflow path of
 *                 the partition kernels had written into are zeroed again), so Phase B of that sample is the index's hit bits alone
 *                 (read_index's table look-ups, extract_ref.cpp:858-870, done where the counts are) and the next reset costs nothing.
 *                 Until that reset the table holds NOTHING: only palace_eref_scan_refs_indexed with the attached index works, every
 *                 other call that reads or extends the table fails.  2: the same, but what is left per entry is its partial COUNT (a rank
 *                 that counted a share of the reads: see palace_eref_entry_layout).  0: off (default).
 *   "scan_ref_lo", "scan_ref_hi"  palace_eref_scan_refs_indexed works on the refs [lo, hi) only (hi = 0: all); the rows of the others
 *                 read n_intervals = el = 0. */
int palace_eref_set_count_mode(palace_ctx *ctx, int mode, int64_t bucket_cap);
/* The count calls that follow take in only the keys whose top 7 bits -- one of 128 buckets of the key space -- are in the set
 * (bit b of mask128 = bucket b; default all).  For N GPUs that each hold all reads (the reference's threads share one table,
 * extract_ref.cpp:1269-1291): rank r counts the keys of its buckets -- its slices of the ">= 3" plane (4 MiB per bucket) are
 * then exact -- and the slices are gathered: no table exchange, no merge; the other keys are dropped where they are made, so
 * the partition kernels move the rank's share of the bytes.  Canonical keys thin out linearly over the key space (bucket b
 * holds (255 - 2b) / 16384 of them), so equal shares take buckets in mirrored pairs, e.g. {r, 2N-1-r} of every 2N. */
int palace_eref_set_key_buckets(palace_ctx *ctx, const uint32_t mask128[4]);
int palace_eref_set_option(palace_ctx *ctx, const char *name, int64_t value);

/* E5 + E6. For each ref: look the three indices of every position up in the table and run the
 * 500-base window scan (read_index + slide_window, extract_ref.cpp:813-903, 504-617).
 * one_min / three_min are int(500 * float(ratio)) as computed by the caller (extract_ref.cpp:
 * 513-514).  d_rows receives n_refs x 4 int32: n_intervals, el, ref_len, reserved(0). */
int palace_eref_scan_refs(palace_ctx *ctx, const uint8_t *d_bases, const int64_t *d_offsets,
                          int64_t n_refs, int64_t total_bases, int one_min, int three_min,
                          int32_t *d_rows);

/* E5 with a per-DB probe index -- the analogue of the index file the reference builds once per DB
 * and then only reads (<fasta>.k32.index.dat, extract_ref.cpp:676-712, 1245-1251).  The index holds
 * the three channel indices of every valid ref position as 16-bit entries grouped by table slice, the
 * maps from a position to its entries, and a quarter of channel 0 once more as "sentinels" with their
 * positions: 19.5 B/position in device memory (3.9 GB for a 200 Mb DB); it depends on the ref set and
 * the coder only, not on the reads.  A DB of up to 2^32 positions.
 * palace_eref_scan_refs_indexed gives exactly the rows of palace_eref_scan_refs for the same table;
 * it replaces the per-position random probes by one sequential pass over 6.5 B/position that leaves a
 * hit BIT per entry (the plane slices in LDS), a scatter of the sentinels that hit, the exact pruning
 * of refs and 64-position chunks on those, and a gather of the three channels' bits for what is left.
 * Meant for a resident DB scanned against many samples; a one-shot run gains nothing from it. */
typedef struct palace_eref_probe_index palace_eref_probe_index;
int palace_eref_probe_index_build(palace_ctx *ctx, const uint8_t *d_bases, const int64_t *d_offsets, int64_t n_refs,
                                  int64_t total_bases, palace_eref_probe_index **out);
int palace_eref_probe_index_free(palace_ctx *ctx, palace_eref_probe_index *ix);
int palace_eref_scan_refs_indexed(palace_ctx *ctx, const palace_eref_probe_index *ix, const uint8_t *d_bases,
                                  const int64_t *d_offsets, int64_t n_refs, int64_t total_bases, int one_min,
                                  int three_min, int32_t *d_rows);

/* Fuse Phase B's channel-0 probe of this DB into the count launch: while such an index is attached, a count call that runs as
 * the FINAL count (option final_count, one slab, the whole key space) tests the DB's positions of every fine bucket against
 * the bucket's final ">= 3" slice while that slice is still in LDS, and the next palace_eref_scan_refs_indexed with the same
 * index starts from those hits: no probe kernel, no second read of the plane.  Results are identical either way (any other
 * count call, a merge, an attach or a reset in between makes the scan probe for itself).  The index keeps the hit bits (one per
 * entry): attach it to ONE context at a time, and scan with it from one context at a time.  ix = NULL detaches. */
int palace_eref_attach_probe_index(palace_ctx *ctx, const palace_eref_probe_index *ix);

/* N GPUs that each counted a SHARE OF THE READS of one sample (no reference counterpart: its threads share one table,
 * extract_ref.cpp:1269-1291).  Phase B reads the table at the DB's keys only (read_index, :858-870), so what the ranks owe each other
 * is not their partial tables but their partial COUNTS of the DB's entries: with option "probe_all_sets" 2 the final count of a rank
 * leaves, for every entry of the attached index (built over the WHOLE DB on every rank), its count 0..3 in two bits -- 16 bits per
 * vector of eight entries, the four entry sets in one block of `counts_bytes` = 2 x `hits_bytes` (multiples of 256 x 840, so that 1 .. 8
 * ranks own equal, aligned shares).  The ranks exchange the block by shares (an all-to-all of counts_bytes / W per peer), each sums the
 * W parts of ITS share -- entry_hits_from_counts(d_parts, n_parts, part_stride, off, bytes): part p's counts of the block's bytes
 * [off, off + bytes) lie at d_parts + p * part_stride (the receive buffer of the all-to-all as it is); bit set iff the counts add up
 * to >= 3, exact because min(3, sum of min(3, c_r)) =
 * min(3, sum of c_r) -- into its share of the hit-bit block, the shares are all-gathered, and entry_hits_complete declares the block
 * whole: palace_eref_scan_refs_indexed then starts from it as from a count that tested every entry itself (options "scan_ref_lo" /
 * "scan_ref_hi": a rank scans its range of the refs).  No plane crosses a link: 162 + 81 MB per 200 Mb of DB instead of 2 x 512 MiB.
 * buffers_attach: the caller's device buffers (what its collectives address; NULL = the index's own, zeroed) stand in for the two blocks.
 * Under option "probe_all_sets" 2 a count call has no other form of result: it takes the binned, fused path whatever the size of the
 * share (one call per reset, one slab, whole key space, clean table) or fails with PALACE_ESTATE; with n = 0 (a rank without reads) it
 * zeroes the block.  entry_counts_valid: 1 when such a call of this context stands behind the block `ix` points at, else 0;
 * entry_hits_complete fails (PALACE_ESTATE) otherwise -- stale counts are never summed silently. */
int palace_eref_entry_layout(const palace_eref_probe_index *ix, size_t *counts_bytes, size_t *hits_bytes);
int palace_eref_entry_buffers_attach(palace_ctx *ctx, palace_eref_probe_index *ix, void *d_counts, void *d_hits);
int palace_eref_entry_buffers(const palace_eref_probe_index *ix, void **d_counts, void **d_hits);     /* where the two blocks lie now (counts: NULL before a first attach) */
int palace_eref_entry_hits_from_counts(palace_ctx *ctx, const palace_eref_probe_index *ix, const void *d_parts, int n_parts, size_t part_stride,
                                       size_t off, size_t bytes);
int palace_eref_entry_hits_complete(palace_ctx *ctx, const palace_eref_probe_index *ix, int64_t keys_counted);
int palace_eref_entry_counts_valid(const palace_ctx *ctx, const palace_eref_probe_index *ix);


/* Multi-GPU exchange of the count table (no reference counterpart: the reference shares one
 * table between std::threads, extract_ref.cpp:1269-1291).  planes() exposes the three device
 * buffers (each 2^29 bytes); merge_slices() folds `n_parts` partial tables laid out as
 * [plane][part][slice_bytes] with the saturating add  (a + b >= t  for t = 1, 2, 3)  done bit-parallel
 * on the planes, and REPLACES bytes [slice_off, slice_off + slice_bytes) of the context's planes by the
 * result: what the slice held before is not added (a rank's own partial table is one of the parts);
 * nothing outside the slice is written. */
int palace_eref_table_planes(palace_ctx *ctx, void **d_planes3, size_t *bytes_per_plane);
/* Use three caller-owned device buffers (each 2^29 bytes, 16-byte aligned) as the table from now on
 * (so a collective library can address them directly); the context no longer frees table memory. */
int palace_eref_table_attach(palace_ctx *ctx, void *const d_planes3[3]);
/* Contract for planes the caller can write (attached ones, or the pointers of palace_eref_table_planes): the library
 * remembers that a table_reset left every bit zero and lets the first count_reads after it skip reading the plane
 * slices.  Between a table_reset and the next count_reads the planes may therefore only be modified through library
 * calls -- or the caller says so: palace_eref_table_invalidate() makes the next count_reads read what is there.
 * (attach itself invalidates; merge_slices and count_reads do as well.) */
int palace_eref_table_invalidate(palace_ctx *ctx);
int palace_eref_table_merge_slices(palace_ctx *ctx, const void *d_parts, int n_parts,
                                   size_t slice_off, size_t slice_bytes);

/* The same exchange with two planes per peer instead of three: the unary planes of a partial table carry two bits per
 * key, the count's low bit (count>=1 ^ count>=2 ^ count>=3) and its high bit (count>=2).  palace_eref_table_pack_low
 * writes the low-bit plane of the context's table into d_low (2^29 bytes, 16-byte aligned); the sender ships d_low and
 * its count>=2 plane; palace_eref_table_merge_slices_packed folds parts laid out [2][n_parts][slice] = (low, high). */
int palace_eref_table_pack_low(palace_ctx *ctx, void *d_low);
int palace_eref_table_merge_slices_packed(palace_ctx *ctx, const void *d_parts, int n_parts, size_t slice_off,
                                          size_t slice_bytes);

/* The ">= 3" plane in sparse form, for exchanges between ranks that each hold a share of the key space (the level-1 buckets of
 * mask128, as in palace_eref_set_key_buckets): the plane of a sample is sparse (the 1M-contig sample sets 24 M of its 2^32 bits),
 * so a fine bucket (2^16 keys = 8 KiB of the plane) travels as the number of its set bits and their 16-bit offsets -- 48 MB for the
 * whole plane instead of 512 MiB.
 * pack:   d_counts[k] = set bits of the k-th fine bucket of the share (the share's level-1 buckets ascending, 512 fine buckets
 *         each: 512 * popcount(mask128) entries), d_first[k] = their exclusive prefix (k = 0 .. n: d_first[n] = total, one more
 *         entry than d_counts), d_keys[d_first[k] ..] = the offsets, ascending.  Keys beyond cap_keys are not written: the
 *         caller reads d_first[n] back (at its leisure) and repeats with more room, or ships the dense slices.
 * unpack: the reverse into THIS context's plane for the buckets of mask128 (every bit of those buckets is rewritten), from
 *         d_counts and d_keys as pack left them; cap_keys = the room d_keys has (keys the sender could not fit are not looked
 *         for: the caller, who sees the counts, discards such a result); d_first is scratch of n + 1 entries.
 * Both are enqueued on the context's stream; nothing is read back. */
int palace_eref_plane_pack(palace_ctx *ctx, const uint32_t mask128[4], uint32_t *d_counts, uint16_t *d_keys, int64_t cap_keys,
                           unsigned long long *d_first);
int palace_eref_plane_unpack(palace_ctx *ctx, const uint32_t mask128[4], const uint32_t *d_counts, const uint16_t *d_keys, int64_t cap_keys,
                             unsigned long long *d_first);

/* Test hooks: counts (0..3) of `n` indices; population count of each plane. */
int palace_eref_table_lookup(palace_ctx *ctx, const uint32_t *d_keys, int64_t n, uint8_t *d_counts);
int palace_eref_table_popcounts(palace_ctx *ctx, uint64_t out3[3]);

/* ---- generateGraph: BAM evidence -> conjugate graph (bin/generate_graph.cpp) ------------ */

/* Options of generate_graph.cpp:20-44 (defaults there; set by its getopt loop :573-593). */
typedef struct {
    int32_t max_end;        /* MAX_END        300 */
    int32_t min_mapq;       /* MIN_MAPQ         0 */
    int32_t max_nm;         /* MAX_NM           5 */
    int32_t enable_paired;  /* ENABLE_PAIRED    1 */
    int32_t both_order;     /* OUTPUT_BOTH_ORDER 0 */
    int32_t reserved;
    double max_span_frac;   /* MAX_SPAN_FRAC 0.80 */
} palace_graph_params;

/* Decoded primary-alignment columns, one entry per BAM record in file order (device pointers).
 * What htslib's bam1_t hands the reference at generate_graph.cpp:644-698, as structure of arrays:
 * ref_len = bam_cigar2rlen; read_len = getReadLength (:385-397); clip_s / clip_e = the soft clips
 * parseCigarReadInterval (:330-383) finds on the record's own CIGAR; nm = NM tag or 0; qkey = a
 * (clip_s = -1 marks a record without CIGAR ops, whose read interval is [0,0], :332); qkey = a
 * 64-bit key of the read name (equal names <=> equal keys, guaranteed by the caller);
 * sa_off[i]..sa_off[i+1] = the record's parsed SA items (empty when the tag is absent). */
typedef struct {
    int64_t n;
    const int32_t *tid, *pos, *mtid, *mpos, *nm, *ref_len, *read_len, *clip_s, *clip_e;
    const uint16_t *flag;
    const uint8_t *mapq;
    const uint64_t *qkey;
    const int32_t *sa_off;
} palace_bam_cols;

/* One parsed SA item (parseSAItem + parseCigarReadInterval on its CIGAR, :185-206, :744;
 * clip_s2 = -1 when the item's CIGAR text is empty).
 * tid2 < 0 when the item must be skipped (name equals the primary's contig :731, or is not in the
 * header :733-734); items that fail to parse are not listed at all. */
typedef struct {
    int32_t tid2, pos2, mapq2, nm2, clip_s2, clip_e2, len2, rev2;
} palace_sa_item;

/* One piece of candidate evidence (classify output / resolve input).  kind 0 = split read,
 * 1 = cross-contig pair.  cls: 0 score is 0 (a mapq is 0), 1 score > 0, 2 decided on the host by
 * libm (exp underflow region of computeLayoutScore, :432-461).  found: a layout exists (:916-938).
 * left/right/oL/oR are already canonical (:855-861); in_fastg is the :863 lookup.  sa_index: which item of
 * the record's SA list a split candidate comes from (0 for pairs) -- with `ord` the order in which the
 * reference meets the evidence (its --debug READS lists, :872, :1008, are in that order). */
typedef struct {
    int64_t ord;
    uint64_t qkey;
    int32_t left, right;
    int32_t mtid, ref_len;
    int32_t dL, dR;
    int32_t nmL, nmR;
    int16_t mapqL, mapqR;
    uint8_t kind, cls, found, in_fastg, oL, oR, pad0, pad1;
    int32_t sa_index;
} palace_graph_cand;

/* Aggregated edge (AggStats, :300-306): counts[0..3] = supplementCount, supplementCountNoFastg,
 * spanCount, spanCountNoFastg.  oL/oR: 0 = '+', 1 = '-'. */
typedef struct {
    int32_t left, right;
    uint32_t counts[4];
    uint8_t oL, oR, pad[6];
} palace_graph_edge;

/* G2-G5 + first half of G6.  Per record: filters (:647-649, :679), depth accumulation into
 * d_consumed[tid] (:654-662), split-read (:684-879) and read-pair (:887-1011) layout search.
 * Appends candidates to d_cands (capacity cand_cap) and returns their number in *n_cands_out.
 * d_tlen / d_trank: target lengths and the dense rank of each target name in byte order (used for
 * the `cR < cL` test :856 and for output order).  d_fastg: sorted keys
 * (tidA << 33 | tidB << 2 | (o1=='-') << 1 | (o2=='-')) of parseFastgFile's set (:119-169).
 * ord_base is the file ordinal of record 0 of this shard. */
int palace_graph_classify(palace_ctx *ctx, const palace_bam_cols *cols, const palace_sa_item *d_sa,
                          int32_t n_targets, const int32_t *d_tlen, const int32_t *d_trank,
                          const uint64_t *d_fastg, int64_t n_fastg, const palace_graph_params *prm,
                          int64_t ord_base, uint64_t *d_consumed, palace_graph_cand *d_cands,
                          int64_t cand_cap, int64_t *n_cands_out);

/* The same, also returning how many of the candidates fall into the exp() underflow zone (cls == 2): the two counters
 * come back in one copy behind one wait, and palace_graph_resolve_ex needs no round trip of its own to learn the second. */
int palace_graph_classify_ex(palace_ctx *ctx, const palace_bam_cols *cols, const palace_sa_item *d_sa,
                             int32_t n_targets, const int32_t *d_tlen, const int32_t *d_trank,
                             const uint64_t *d_fastg, int64_t n_fastg, const palace_graph_params *prm,
                             int64_t ord_base, uint64_t *d_consumed, palace_graph_cand *d_cands,
                             int64_t cand_cap, int64_t *n_cands_out, int64_t *n_border_out);

/* The same with the FASTG search narrowed: d_fastg_first[t] (n_targets + 1 entries, made once per sample by
 * palace_graph_fastg_offsets from the same sorted key array) = index of the first key whose left contig is >= t, so that a
 * candidate's look-up starts inside its left contig's two or three links instead of bisecting the whole set (:863-864 is a
 * std::set find per evidence; here ~22 dependent loads per candidate were most of the kernel's time).  NULL = bisect. */
int palace_graph_fastg_offsets(palace_ctx *ctx, const uint64_t *d_fastg, int64_t n_fastg, int32_t n_targets, uint32_t *d_first);
int palace_graph_classify_ix(palace_ctx *ctx, const palace_bam_cols *cols, const palace_sa_item *d_sa,
                             int32_t n_targets, const int32_t *d_tlen, const int32_t *d_trank,
                             const uint64_t *d_fastg, int64_t n_fastg, const uint32_t *d_fastg_first, const palace_graph_params *prm,
                             int64_t ord_base, uint64_t *d_consumed, palace_graph_cand *d_cands,
                             int64_t cand_cap, int64_t *n_cands_out, int64_t *n_border_out);

/* Second half: decide host-side borderline scores, apply the order-dependent rules
 * (hasSupplementEvidence gating :881-888, processedPairedReads "first in file order wins" and its
 * mate-contig depth quirk :890-893, :938), aggregate per canonical edge (:866-872, :1002-1008).
 * n_records_total bounds candidate ordinals.  Writes up to edge_cap edges (unsorted). */
int palace_graph_resolve(palace_ctx *ctx, palace_graph_cand *d_cands, int64_t n_cands,
                         int64_t n_records_total, const palace_graph_params *prm, uint64_t *d_consumed,
                         palace_graph_edge *d_edges, int64_t edge_cap, int64_t *n_edges_out);

/* The same without the host in the loop.  n_border: number of candidates with cls == 2 (from palace_graph_classify_ex; summed
 * over the ranks whose candidates were gathered), 0 = none, so nothing is copied to the host; < 0 = unknown, look.
 * d_n_edges (device, 8 bytes, optional) receives the edge count in stream order; n_edges_out may be NULL, and then the call
 * only enqueues: no synchronisation (a count above edge_cap is then the reader's to detect: edges beyond it are dropped). */
int palace_graph_resolve_ex(palace_ctx *ctx, palace_graph_cand *d_cands, int64_t n_cands, int64_t n_border,
                            int64_t n_records_total, const palace_graph_params *prm, uint64_t *d_consumed,
                            palace_graph_edge *d_edges, int64_t edge_cap, int64_t *d_n_edges, int64_t *n_edges_out);

/* The host-libm decision alone (computeLayoutScore's exp() underflow gate, :432-461) on the candidates of ONE classify call:
 * every found candidate with cls == 2 becomes cls 0 or 1 in place.  A rank of a multi-GPU run calls it on its own candidates
 * (n_border from palace_graph_classify_ex; 0 = nothing to do, nothing is copied) before they are gathered, so that what every
 * rank resolves carries no undecided candidate and palace_graph_resolve_ex can be given n_border = 0 without an exchange of
 * counts.  Synchronises the stream when n_border != 0. */
int palace_graph_score_border(palace_ctx *ctx, palace_graph_cand *d_cands, int64_t n_cands, int64_t n_border,
                              const palace_graph_params *prm);

/* G6 epilogue numbers (generate_graph.cpp:1029-1031): depth = consumed / max(1, len) and
 * cn = (int)floor(depth / avg_depth + 0.5) (0 when avg_depth <= 0), per target, in IEEE double. */
int palace_graph_copy_numbers(palace_ctx *ctx, const uint64_t *d_consumed, const int32_t *d_tlen,
                              int32_t n_targets, double avg_depth, int32_t *d_cn);

/* ---- N4: BGZF members inflated on the device ------------------------------------------------------------------------------ */

/* What htslib's bgzf layer does inside sam_read1 (generate_graph.cpp:644), for n_members BGZF members at once, one wavefront
 * each: member m's raw DEFLATE data are d_in[d_in_off[m] .. + d_in_len[m]) (behind the member's 18-byte header, in front of
 * its CRC32 / ISIZE trailer), its d_out_len[m] (= ISIZE, <= 65536) bytes go to d_out + d_out_off[m].  d_status[m] = 0: exactly
 * those bytes were written; non-zero: the decoder refused the member (malformed, or a size that does not fit) and the caller
 * lets zlib decide it on the host, as the loader's CPU decoder does.  CRC32 is not checked (the loader never did; htslib does).
 * The buffer behind d_in must extend at least 3 bytes past the last member's data (reads are whole dwords).  Enqueues only. */
int palace_bgzf_inflate(palace_ctx *ctx, const uint8_t *d_in, int64_t n_members, const int64_t *d_in_off, const int32_t *d_in_len,
                        const int64_t *d_out_off, const int32_t *d_out_len, uint8_t *d_out, int32_t *d_status);

/* ---- BGZF members written on the device: the counterpart of palace_bgzf_inflate ------------------------------------------- */

/* One complete BGZF member per piece of device text, one workgroup each: piece m is the d_len[m] (0 .. 0xff00) bytes at
 * d_text + d_off[m]; its member -- the 18-byte header with the BC subfield and BSIZE, one DEFLATE block, CRC-32 (d_crc[m], as
 * palace_crc32_members computes it for the same ranges) and ISIZE -- goes to d_slots + 65536 * m (4-byte aligned; the slot's bytes
 * behind the member are undefined) and its length to d_member_len[m] (28 .. 65311).  The block is dynamic Huffman (BTYPE 10) over
 * tokens whose only match candidate is the byte one previous-line-length back (lines end at LF: the text of `samtools depth`
 * compresses like zlib level 6 this way, other text like its literals alone); a piece that would not become shorter is a stored
 * block (BTYPE 00), an empty piece the 28-byte EOF member.  The contract is the format, not zlib's bytes: every member inflates to
 * its piece in zlib and in palace_bgzf_inflate, and the same input always gives the same bytes.  Enqueues only. */
int palace_bgzf_deflate(palace_ctx *ctx, const uint8_t *d_text, int64_t n_members, const int64_t *d_off, const int32_t *d_len,
                        const uint32_t *d_crc, uint8_t *d_slots, int32_t *d_member_len);

/* The same call for text without lines -- the records of a BAM (`bamsort --lz`, `samview --lz`): the same pieces (0 .. 0xff00 bytes
 * at any alignment), slots (65536 bytes each, 4-byte aligned), member lengths (28 .. 65311), stored fallback and EOF member, and
 * palace_bgzf_compact takes its slots as it takes the other call's.  Only the tokens differ; the rule is a function of the piece's n
 * bytes alone (csrc/deflate_lz.hpp states it, DESIGN.md 8 repeats it): h(p) = the top 14 bits of (the little-endian word of bytes
 * p .. p + 3) * 2654435761 mod 2^32, for p <= n - 4; the piece is taken in rounds of 512 positions and the candidate of p is the
 * greatest q with h(q) == h(p) that lies before p's round and at most 32768 back -- never inside p's own round; thread t of 512
 * parses bytes [t * chunk, (t + 1) * chunk), chunk = ceil(n / 512), greedily from its first byte: the equal bytes at the candidate,
 * at most 258 and never past the chunk's or the piece's end, are a match from 3 bytes on, a literal below.  Not zlib's bytes: every
 * member inflates to its piece in zlib and in palace_bgzf_inflate, and the same input always gives the same bytes.  The distances of
 * the members in flight (131072 bytes for each of min(n_members, 256) workgroups) come from the context's workspace: the call
 * enqueues only, unless that workspace has to grow, which waits for the stream once. */
int palace_bgzf_deflate_lz(palace_ctx *ctx, const uint8_t *d_text, int64_t n_members, const int64_t *d_off, const int32_t *d_len,
                           const uint32_t *d_crc, uint8_t *d_slots, int32_t *d_member_len);

/* The members of such a batch as consecutive file bytes: d_member_off[m] = sum of the lengths in front of member m
 * (n_members + 1 entries, the last = all bytes), member m copied to d_file + d_member_off[m] (room for 65311 bytes per member is
 * always enough).  A batch then leaves the device as one copy of d_member_off[n_members] bytes.  Enqueues only. */
int palace_bgzf_compact(palace_ctx *ctx, const uint8_t *d_slots, int64_t n_members, const int32_t *d_member_len, uint8_t *d_file,
                        int64_t *d_member_off);

/* ---- compressed FASTQ for eref: inflated text parsed in HBM -------------------------------------------------------------- */

/* CRC-32 (the gzip polynomial) of n_members byte ranges of device memory, one wavefront each: d_crc[m] = crc32 of the d_len[m]
 * bytes at d_data + d_off[m] -- what zlib checks against a gzip member's trailer, for the members palace_bgzf_inflate decoded
 * (it checks none).  Enqueues only. */
int palace_crc32_members(palace_ctx *ctx, const uint8_t *d_data, int64_t n_members, const int64_t *d_off, const int32_t *d_len,
                         uint32_t *d_crc);

/* Where a FASTQ parse stands between two windows of one file (device memory, 32 bytes).  line: 0-based index of the line the
 * next byte belongs to; reads / bases: the read set so far (d_offsets[reads] = bases); open: line `line` has begun in an earlier
 * window; error: a window did not fit the capacities given with it (it and every later window are then not parsed).  A file
 * starts at {0, R, B, 0, 0}: its reads follow R reads of B bases of an earlier file in the same read set. */
typedef struct {
    int64_t line, reads, bases;
    int32_t open, error;
} palace_fastq_cursor;

/* The sequence lines of FASTQ text in device memory appended to an ASCII read set (the form palace_eref_count_reads and
 * palace_eref_pack_reads take), with the line semantics of the reference's std::getline loop (extract_ref.cpp:940-1004) that
 * the host's parser has (host/fastx.hpp): a line ends at '\n' only ('\r' stays in the sequence); sequence lines are the lines
 * whose index is 1 mod 4, an empty one included; bytes are copied unchanged.  d_text[0 .. n) (16-byte aligned) is the next
 * window of the file: any cut will do, a line may span any number of windows.  final_window != 0: the file ends with this window,
 * and a last line without '\n' is a line (the empty text behind a final '\n' is not).  Writes the new reads' bytes to
 * d_bases[cursor.bases ..] and their end offsets to d_offsets[cursor.reads + 1 ..] (d_offsets[0] = 0 is the caller's), and moves
 * *d_cursor past the window.  bases_cap / offsets_cap: bytes of d_bases, entries of d_offsets; a window that would write past them
 * writes nothing and sets cursor.error (a read set has at most 1 + n / 4 reads and n bases more after a window of n bytes).
 * d_scratch: palace_fastq_scratch_bytes(n) bytes of device memory, not shared with calls in flight.  Enqueues only. */
size_t palace_fastq_scratch_bytes(int64_t max_window);
int palace_fastq_parse(palace_ctx *ctx, const uint8_t *d_text, int64_t n, int final_window, palace_fastq_cursor *d_cursor,
                       uint8_t *d_bases, int64_t bases_cap, int64_t *d_offsets, int64_t offsets_cap, void *d_scratch,
                       size_t scratch_bytes);

/* ---- `samtools depth` text read back: totals and per-contig runs (bamdepth --from-depth) ---------------------------------- */

#define PALACE_DEPTH_TAIL_BYTES 4096       /* a line has at most this many bytes, its LF counted (csrc/depth_line.hpp) */

/* Where a depth parse stands between two windows of one file (device memory; a file starts at all zeros).  The first 64 bytes are
 * what a caller reads back per window.  lines / sum: the lines so far and the sum of their depths; bad_line: the 1-based number of
 * the file's first line that is not `name<TAB>position<TAB>depth` (0: none so far; sums and runs mean nothing once it is set);
 * win_runs / win_name_bytes: what the last window wrote to d_runs / d_names -- or, when error is set, what it would have written;
 * tail_len, tail_buf, tail: the unterminated end of the text so far, tail[tail_buf][0 .. tail_len); error: the window did not fit
 * runs_cap / names_cap: it and every later window write nothing and leave the cursor as it was but for error, win_runs and
 * win_name_bytes (a caller may clear error and hand the same window over again with more room). */
typedef struct {
    int64_t lines;
    uint64_t sum;
    int64_t bad_line;
    int64_t win_runs, win_name_bytes;
    int32_t tail_len, tail_buf;
    int32_t error, reserved0;
    int64_t reserved1;
    uint8_t tail[2][PALACE_DEPTH_TAIL_BYTES];
} palace_depth_cursor;

/* A run: a maximal stretch of consecutive lines of one window with byte-equal names.  A window's first line always begins one. */
typedef struct {
    uint64_t sum, lines;           /* of the run's lines: their depths, their number */
    uint32_t name_off, name_len;   /* the name: d_names[name_off .. name_off + name_len) */
} palace_depth_run;

/* The text `contig<TAB>position<TAB>depth<LF>` in device memory reduced to totals and runs; the line's grammar is
 * csrc/depth_line.hpp's (strict: 1-10 digits, values up to 2^31 - 1, no CR, no sign, exactly three columns, at most 4096 bytes).
 * d_text[0 .. n) (16-byte aligned, n <= 2^30) is the next window of the file: any cut will do, a line may span any number of
 * windows.  final_window != 0: the file ends with this window, and a last line without LF is a line (the empty text behind a final
 * LF is not).  Moves *d_cursor past the window and writes the window's runs in text order to d_runs[0 .. cursor.win_runs) and their
 * names to d_names[0 .. cursor.win_name_bytes); a line counts in the window in which it ends.  Sums are integers: the result does
 * not depend on scheduling.  d_scratch: palace_depth_parse_scratch_bytes(n) bytes of device memory, not shared with calls in
 * flight.  Three launches (count, scan, emit) whatever the window holds.  Enqueues only. */
size_t palace_depth_parse_scratch_bytes(int64_t max_window);
int palace_depth_parse(palace_ctx *ctx, const uint8_t *d_text, int64_t n, int final_window, palace_depth_cursor *d_cursor,
                       palace_depth_run *d_runs, int64_t runs_cap, uint8_t *d_names, int64_t names_cap, void *d_scratch,
                       size_t scratch_bytes);

/* ---- gzip that is not BGZF: one DEFLATE stream inflated by many wavefronts ------------------------------------------------ */

/* stride: compressed bytes between the places where a block start is searched for (one chunk per place at most); span: compressed
 * bytes uploaded and worked on at a time; text_cap: the most text resolved at a time (at most 1 GiB).  0 = the default
 * (16 KiB, 64 MiB, 512 MiB).  Device memory in flight: span + 3 x text_cap + 32 KiB per chunk of a batch (at most 4096 chunks). */
typedef struct {
    int64_t stride, span, text_cap;
    int64_t check_guards;      /* tests: != 0 puts guard bytes around every output buffer and counts the damaged ones */
} palace_gzip_params;

/* why the device path declined a file (palace_gzip_stats.fallback); the caller then lets zlib decide the file */
enum {
    PALACE_GZ_NONE = 0,
    PALACE_GZ_HEADER = 1,      /* a member header zlib would refuse */
    PALACE_GZ_DECODE = 2,      /* a chunk on the chain did not decode */
    PALACE_GZ_CHAIN_OPEN = 3,  /* more certain starts had to be queued in one span than the bound on rounds allows */
    PALACE_GZ_NO_PROGRESS = 4, /* no block ends inside a whole span */
    PALACE_GZ_TOO_BIG = 5,     /* one chunk inflates to more than text_cap */
    PALACE_GZ_TRUNCATED = 6,   /* the file ends inside a stream or a trailer */
    PALACE_GZ_CRC = 7,
    PALACE_GZ_ISIZE = 8,
    PALACE_GZ_TRAILING = 9,    /* bytes that are no gzip member behind the last one */
    PALACE_GZ_SINK = 10,       /* the sink returned non-zero */
    PALACE_GZ_MARKER = 11      /* a match that reaches before the start of its member (zlib: "invalid distance too far back"),
                                * in whichever chunk of the member: the chain compares every chunk's reach before its own start
                                * with the member's text so far */
};

/* chunks_found: block starts the finder reported; chunks_accepted: chunks on the chain (decoded to text); false_hits: reported
 * starts the chain ran across; rounds: certain starts queued behind the first size pass (a dropped hit, the member behind a
 * trailer); guards_bad: guard bytes found changed (check_guards; always 0); ms_*: wall time of the stages, each waited for. */
typedef struct {
    int64_t chunks_found, chunks_accepted, false_hits, rounds, members, spans, batches, text_bytes;
    int32_t fallback, guards_bad;
    double ms_upload, ms_find, ms_size, ms_decode, ms_chain, ms_resolve, ms_crc, ms_sink;
} palace_gzip_stats;

/* takes the next n bytes of the file's text (device memory, 16-byte aligned, valid until the sink returns); last != 0 with the
 * file's final bytes (n may be 0).  Non-zero return: stop. */
typedef int (*palace_gzip_sink)(void *user, const uint8_t *d_text, int64_t n, int last);

/* The text of a gzip file (host memory, every member of it) handed to `sink` in file order, inflated on the device: block starts
 * found inside the stream at every `stride` (dynamic-Huffman headers that parse completely), the chunks between them sized,
 * chained on the host, decoded to 16-bit symbols (a literal, or a reference into the 32 KiB before the chunk), the references
 * resolved through a chain of windows, CRC-32 and ISIZE of every member checked.  Returns 0 also when the device path declines
 * the file (stats->fallback != 0: damaged input, or a stream it cannot cut): text the sink already took is then void -- a member's
 * CRC is known only at its end -- and the caller decides the file with zlib.  Negative: a device error.  Synchronises. */
int palace_gzip_inflate(palace_ctx *ctx, const uint8_t *file, int64_t size, const palace_gzip_params *prm, palace_gzip_sink sink,
                        void *user, palace_gzip_stats *stats);

/* ---- depth stage: `samtools depth <bam> | awk '{sum+=$3} END {print sum/NR}'` (palace:538-552) ------------------ */

/* The two numbers of that mean.  A match segment is one M / = / X CIGAR operation of a record whose UNMAP, SECONDARY,
 * QCFAIL and DUP flags are clear (samtools depth, default options: deletions and reference skips do not count): target,
 * 0-based reference position, length.  sum_out = total length of the segments (cut at the end of their contig),
 * covered_out = number of distinct reference positions they cover = the NR of the awk line.  d_tbase[t] = sum of the
 * lengths of targets 0..t-1 (int64, n_targets entries), total_len = sum of all lengths. */
int palace_depth_sum_covered(palace_ctx *ctx, int64_t n_segs, const int32_t *d_seg_tid, const int32_t *d_seg_pos,
                             const int32_t *d_seg_len, int32_t n_targets, const int32_t *d_tlen, const int64_t *d_tbase,
                             int64_t total_len, uint64_t *sum_out, uint64_t *covered_out);

/* The same per contig as well: d_contig_sum[t] / d_contig_covered[t] (device, n_targets entries each) = what
 * `tabix fetch(contig)` on the depth file yields, reduced to sum and count (create_sub_graph.py:186-234 reads exactly
 * that: mean = sum / count, weight = count). */
int palace_depth_per_contig(palace_ctx *ctx, int64_t n_segs, const int32_t *d_seg_tid, const int32_t *d_seg_pos,
                            const int32_t *d_seg_len, int32_t n_targets, const int32_t *d_tlen, const int64_t *d_tbase,
                            int64_t total_len, uint64_t *sum_out, uint64_t *covered_out, uint64_t *d_contig_sum,
                            uint64_t *d_contig_covered);

/* The text of `samtools depth` itself (palace:541), resident on the device: one line `contig <TAB> 1-based position <TAB> depth`
 * per position with depth > 0, contigs in header order.  create takes the match segments as palace_depth_sum_covered does, d_tbase
 * with n_targets + 1 entries (the last = total_len), and the contig names as one byte blob: name t = d_names[d_name_off[t] ..
 * d_name_off[t + 1]).  It keeps the depth of every position (4 B per position + 24 B per tile of 1024 positions, allocated here)
 * and returns the size of the text, its lines and the sum of its depths: sum / lines is the awk number.  The caller's arrays
 * other than the segments stay in use until destroy.  Waits for the stream. */
typedef struct palace_depth_text palace_depth_text;
int palace_depth_text_create(palace_ctx *ctx, int64_t n_segs, const int32_t *d_seg_tid, const int32_t *d_seg_pos,
                             const int32_t *d_seg_len, int32_t n_targets, const int32_t *d_tlen, const int64_t *d_tbase,
                             int64_t total_len, const uint8_t *d_names, const int64_t *d_name_off, palace_depth_text **out,
                             uint64_t *text_bytes_out, uint64_t *lines_out, uint64_t *sum_out);
int palace_depth_text_destroy(palace_ctx *ctx, palace_depth_text *dt);
/* bytes [text_begin, text_end) of the text to d_out[0 ..); a line may straddle either end.  Enqueues only. */
int palace_depth_text_emit(palace_ctx *ctx, const palace_depth_text *dt, uint64_t text_begin, uint64_t text_end, uint8_t *d_out);
/* For n_windows ranges [d_win_beg[w], d_win_end[w]) of global positions (contigs end to end: d_tbase[t] + position):
 * d_text_beg[w] / d_text_end[w] = the text offset of the first line at or behind the range's first / end position, d_lines[w] = the
 * lines of the range.  With one range per contig and 16 kb window these are the chunks and the linear index of the file's tabix
 * index.  Enqueues only. */
int palace_depth_text_windows(palace_ctx *ctx, const palace_depth_text *dt, int64_t n_windows, const int64_t *d_win_beg,
                              const int64_t *d_win_end, uint64_t *d_text_beg, uint64_t *d_text_end, uint64_t *d_lines);

/* ---- the BAM's records found and their match segments made where the inflated stream lies ------------------------------------- */

/* The record walk of the BAM loader (what sam_read1's loop does to the stream, generate_graph.cpp:644) on an inflated stream in
 * device memory: d_stream[0 .. total), the first alignment record at `first` (behind the header).  The result is DEFINED as the
 * serial walk from `first`: a record at p needs its 4-byte block_size >= 32, all of its bytes in front of `total`, l_read_name >= 1
 * and name, CIGAR, bases and qualities that fit block_size; the first offset that fails ends the stream (`stop`; == total for a
 * well-formed one).  d_starts receives, in file order, the offset of every record's refID (p + 4) when it has room for them all
 * (cap entries); otherwise -- d_starts may be NULL with cap 0 -- only the count is returned and palace_bam_walk_starts writes them
 * later from the same scratch.  The walk runs as one guess per chunk of `chunk` bytes (0 = 64 KiB, at least 64) that a chain over
 * the chunks confirms or repairs: the result never depends on the guesses, the time does (n_ref, the number of targets, only
 * sharpens them).  stats_out[4] = chunks, guesses that held, chunks the chain walked itself, chunks without a guess.
 * d_scratch: palace_bam_walk_scratch_bytes(total, first, chunk) bytes, 8-byte aligned.  Waits for the stream. */
size_t palace_bam_walk_scratch_bytes(int64_t total, int64_t first, int64_t chunk);
int palace_bam_walk(palace_ctx *ctx, const uint8_t *d_stream, int64_t total, int64_t first, int32_t n_ref, int64_t chunk,
                    void *d_scratch, size_t scratch_bytes, int64_t *d_starts, int64_t cap, int64_t *n_records_out,
                    int64_t *stop_out, int64_t stats_out[4]);
/* the starts of the last palace_bam_walk with these arguments and this scratch (at most cap of them).  Enqueues only. */
int palace_bam_walk_starts(palace_ctx *ctx, const uint8_t *d_stream, int64_t total, int64_t first, int64_t chunk, const void *d_scratch,
                           size_t scratch_bytes, int64_t *d_starts, int64_t cap);

/* The match segments of palace_depth_sum_covered from the records themselves (d_starts as palace_bam_walk leaves them): one entry
 * per M / = / X operation of length > 0 of every record with flags 0x704 clear, 0 <= refID < n_ref and pos >= 0, at pos + the
 * reference consumed in front of it (M, D, N, =, X), in record order, then operation order.  The CIGAR is the record's own, or
 * the CG:B,I tag's behind a <l_seq>S<ref>N placeholder (SAM spec 4.2.2: the first CG tag decides; taken when its type is B with
 * subtype I or i and n_cigar_op <= count < 2^29; the scan of the aux fields stops at one whose size is unknown or past the record).
 * Without the three arrays, or with cap smaller than the count, nothing is written and *n_segs_out is what a second call needs.
 * Waits for the stream for the count; the segments are enqueued. */
int palace_bam_match_segments(palace_ctx *ctx, const uint8_t *d_stream, int64_t total, const int64_t *d_starts, int64_t n_records,
                              int32_t n_ref, int32_t *d_seg_tid, int32_t *d_seg_pos, int32_t *d_seg_len, int64_t cap,
                              int64_t *n_segs_out);

/* ---- the BAM's records decoded where the inflated stream lies: generateGraph's columns and SA items ------------------------------ */

/* Every array of palace_bam_cols except sa_off, for records [0, n_records) of the stream (d_starts as palace_bam_walk leaves them);
 * the arrays `cols` names are WRITTEN (n_records entries each; cols->n and cols->sa_off are not looked at).  The result is DEFINED as
 * what the host loader writes for the same record (BamLoad::decode_range, palace_amd/host/bam.cpp):
 *   tid, pos, mapq, flag, mtid, mpos: the fixed fields.  The CIGAR is the record's own, or the first CG tag's under the conditions of
 *   palace_bam_match_segments and refID >= 0, pos >= 0.  ref_len counts M, D, N, =, X; read_len counts M, I, S, =, X.  clip_s / clip_e:
 *   zero-length ops are dropped, the leading S, the trailing S only when more than one op remains; clip_s = -1 for a record without ops.
 *   nm: the FIRST NM field decides -- types c, C, s, S, i, I are read with their signedness, any other type gives 0 -- default 0.
 *   The aux scan stops at a field of unknown size or one that runs past the record, and once both NM and SA:Z are found.
 *   qkey = the seeded 64-bit key of the read name's C-string view (up to the first NUL inside l_read_name, else l_read_name - 1 bytes):
 *   FNV-1a from 0xcbf29ce484222325 ^ (seed * 0x9e3779b97f4a7c15), then h ^= h >> 32; h *= 0xd6e8feb86659fd93; h ^= h >> 32.
 * Enqueues only. */
int palace_bam_columns(palace_ctx *ctx, const uint8_t *d_stream, int64_t total, const int64_t *d_starts, int64_t n_records,
                       uint64_t key_seed, const palace_bam_cols *cols);
/* qkey alone, with another seed: the way out of a read-name key collision.  Enqueues only. */
int palace_bam_name_keys(palace_ctx *ctx, const uint8_t *d_stream, int64_t total, const int64_t *d_starts, int64_t n_records,
                         uint64_t key_seed, uint64_t *d_qkey);
/* How many of the n_pairs pairs of record ordinals (d_pairs[2k], d_pairs[2k + 1]) have different C-string read names: the exactness
 * guard behind equal keys, without the names leaving the device.  An ordinal outside [0, n_records) counts as different.  Waits. */
int palace_bam_names_differ(palace_ctx *ctx, const uint8_t *d_stream, int64_t total, const int64_t *d_starts, int64_t n_records,
                            const int64_t *d_pairs, int64_t n_pairs, int64_t *n_differ_out);

/* The header's contig names as a hash table in device memory: name t = d_names[d_name_off[t] .. d_name_off[t + 1]) (n_ref + 1
 * offsets; blob and offsets stay the caller's and in use until destroy).  A look-up compares the exact name on a hit; of equal names
 * the LAST one's tid is found.  create allocates the table and enqueues its build; destroy waits for the stream. */
typedef struct palace_bam_names palace_bam_names;
int palace_bam_names_create(palace_ctx *ctx, const uint8_t *d_names, const int64_t *d_name_off, int32_t n_ref, palace_bam_names **out);
int palace_bam_names_destroy(palace_ctx *ctx, palace_bam_names *names);

/* sa_off (n_records + 1 entries) and the parsed SA items, in record order, then list order, as the host loader makes them (bam.cpp:
 * decode_range, parse_sa, clip_from_text).  The first SA field of type Z is taken (an SA of another type does not end the search);
 * items are parsed only when 0 <= tid < n_ref; the text is split at ';', empty items are skipped; six comma fields are needed in
 * getline's sense (a field exists iff at least one byte is left); C-locale white space is trimmed from both ends of every field; an
 * empty name or position fails the item, and failed items are not listed.  rev2 = the strand field is exactly "-".  The CIGAR text:
 * any non-digit byte ends an op, zero-length ops are dropped, empty text gives clip_s2 = -1.  pos2, mapq2 and nm2 are glibc's atoi:
 * optional sign, digits up to the first non-digit, 0 when there are none; beyond the range of long the value saturates (LONG_MAX /
 * LONG_MIN) and the conversion to int keeps the low 32 bits (-1 / 0).  tid2 = -1 when the name is the record's own contig's, else the
 * contig's tid (the last duplicate of a name), -1 for an unknown name.
 * Counted first, written second: without d_sa_off, or with cap smaller than the count, nothing is written and *n_items_out is what a
 * second call needs.  More items than int32 holds is an error.  Waits for the stream for the count; the items are enqueued. */
int palace_bam_sa_items(palace_ctx *ctx, const uint8_t *d_stream, int64_t total, const int64_t *d_starts, int64_t n_records,
                        const palace_bam_names *names, int32_t *d_sa_off, palace_sa_item *d_items, int64_t cap, int64_t *n_items_out);

/* ---- matching: path / cycle decomposition of the conjugate graph ------------------------- */

/* M1. One greedy matching over the arcs of the conjugate graph, computed as rounds of locally
 * dominant arcs (an arc is taken when it is the best remaining arc of both its tail's out-slot
 * and its head's in-slot), which yields exactly the sequential greedy matching in rank order.
 * The reference's `matching` binary is absent; the call it serves is
 * palace:587-590 / 684-688 and the algorithm is this repository's own.
 * Vertices are oriented segments (2*seg + (orient=='-')); arcs are given in rank order
 * (arc id == rank, lower is better; an arc and its conjugate are adjacent), with CSR lists of
 * arc ids per tail (out_off/out_arcs) and per head (in_off/in_arcs).  d_alive: 1 B per vertex.
 * Outputs per vertex: d_next / d_prev (-1 = none) and d_next_arc (id of the arc leaving it). */
int palace_match_greedy(palace_ctx *ctx, int32_t n_vertices, int64_t n_arcs, const int32_t *d_src,
                        const int32_t *d_dst, const int64_t *d_out_off, const int32_t *d_out_arcs,
                        const int64_t *d_in_off, const int32_t *d_in_arcs, const uint8_t *d_alive,
                        int32_t *d_next, int32_t *d_prev, int32_t *d_next_arc, int32_t *rounds_out);

/* Host glue between generateGraph's numbers and palace_match_decompose, i.e. what the matching
 * executable does while it reads the SEG/JUNC text (palace_amd/host/matching_main.cpp): copies[s] =
 * max(1, cn[s]); every edge whose four counters sum to >= min_count (JUNC filter,
 * generateGraph.cpp:1056-1061) becomes the arc (left,oL)->(right,oR) plus its conjugate
 * (right,!oR)->(left,!oL) (make_final_fa.py:20-34), equal arcs merged with their weights added;
 * arcs come out in rank order (weight descending, class {arc, conjugate} ascending, (u, v) ascending).
 * Host arrays; src/dst/weight need room for 2 * n_edges arcs.  Pure host code (no GPU work). */
int palace_match_arcs_from_edges(const int32_t *cn, int32_t n_segs, const palace_graph_edge *edges, int64_t n_edges,
                                 int32_t min_count, int64_t *copies, int32_t *src, int32_t *dst, int64_t *weight,
                                 int64_t *n_arcs_out);

/* M1, whole decomposition: `iterations` rounds of {greedy matching on the GPU, read the paths and
 * cycles off the successor links, charge copy numbers, drop exhausted segments} (+ one copy-number
 * blind round when `aggressive`).  Host arrays in: copies[n_segs] (>= 1), arcs in rank order
 * (src/dst oriented-vertex ids, an arc and its conjugate adjacent).  Result: components in emission
 * order; component c holds verts[off[c] .. off[c+1]) in path order (cycles rotated to their
 * smallest vertex, conjugate representative chosen), kind[c] = 0 path / 1 cycle, iter[c] = round,
 * open_at[c] = position after the cycle's weakest arc (where -b opens it; 0 for paths).
 * Duplicate and later-round singleton components are NOT filtered here (the caller formats). */
typedef struct palace_match_result palace_match_result;
/* Tuning knob (results are identical for every setting).  The decomposition runs on the device, one launch per phase, enqueued
 * a group of rounds at a time with a fixed number of matching iterations per round (7 in the first round, 4 later; the
 * iterations behind a round's fixed point return at once); the host looks at the state after each group, stops as soon as no
 * segment keeps a copy, and redoes the decomposition with a check after every batch of iterations should a round not have
 * settled.  "iters_per_round" overrides the number of iterations (0 = defaults, at most 64; 1 forces the checked path);
 * "decomp_grid" workgroups of the decomposition's arc- and vertex-sized phases (0 = default 2048: chains of dependent random
 * look-ups, bounded by how many are in flight; 256 costs a saturating kernel on another stream less, see bench/step.py).
 * "one_word_keys" 0: palace_stage04_match ranks its arcs by the two-word key in every case (default 1: by a one-word form of
 * the same order -- weight | path-backed | class of (tail, head) -- whenever the sample's arcs fit it, which saves the second
 * proposal pass of every matching iteration: half of the atomics and a third of the look-ups). */
int palace_match_set_option(palace_ctx *ctx, const char *name, int64_t value);
/* Which way the last decomposition whose result this context handed out (palace_match_decompose[_ex], palace_stage04_result)
 * went: info[0] = how it ranked its arcs (0: by the arc's position alone, palace_match_decompose; 1: by the two-word key;
 * 2: by the one-word key), info[1] = 1 when a round did not settle and the run with the host checking every fixed point
 * took over (info[0], [2] and [3] then describe that run; it never uses one-word keys), info[2] = rounds enqueued (fewer than
 * asked for when no segment kept a copy), info[3] = matching iterations enqueued, the ones behind a fixed point included.
 * All zero after a graph without arcs.  Reads what the decomposition brought back anyway: no launch, no wait.  An error
 * before the first decomposition. */
int palace_match_last_run(palace_ctx *ctx, int64_t info[4]);
int palace_match_decompose(palace_ctx *ctx, int32_t n_segs, const int64_t *copies, int64_t n_arcs,
                           const int32_t *src, const int32_t *dst, int32_t iterations, int32_t aggressive,
                           palace_match_result **out);
/* The same with `compact` != 0: only components that hold a segment with at least one arc are listed (same order, same
 * fields); the segments without any arc -- each a one-vertex path of round 0, and again of the extra round when
 * `aggressive`, that a full result lists in first-vertex order between the others -- are given as one bit per segment
 * (palace_match_result_bare: ceil(n_segs / 64) words, bit s of word s / 64; palace_match_result_bare_count of them).  A
 * graph of a million segments of which a few percent touch a junction is the normal case: the full listing is almost
 * all single-vertex entries. */
int palace_match_decompose_ex(palace_ctx *ctx, int32_t n_segs, const int64_t *copies, int64_t n_arcs,
                              const int32_t *src, const int32_t *dst, int32_t iterations, int32_t aggressive,
                              int32_t compact, palace_match_result **out);
const uint64_t *palace_match_result_bare(const palace_match_result *r);
int64_t palace_match_result_bare_count(const palace_match_result *r);
int64_t palace_match_result_count(const palace_match_result *r);
const int64_t *palace_match_result_offsets(const palace_match_result *r);
const int32_t *palace_match_result_verts(const palace_match_result *r);
const uint8_t *palace_match_result_kind(const palace_match_result *r);
const int32_t *palace_match_result_iter(const palace_match_result *r);
const int32_t *palace_match_result_open_at(const palace_match_result *r);
void palace_match_result_free(palace_match_result *r);

/* ---- stage 04 resident in HBM: filter_graph.py + matching without the text files in between ----------------------- */

/* What the pipeline does between generateGraph's numbers and `all_result` (palace:566-600) is a selection on the graph
 * (share/palace/scripts/filter_graph.py) and `matching` on what the selection leaves.  For a sample whose edges are already
 * in HBM (palace_graph_resolve) both run on the device; the host formats.  Per-sample inputs, parsed once like the BAM
 * columns (host arrays; create copies them to the device): */
typedef struct {
    int32_t n_segs;            /* contigs = BAM targets */
    int32_t min_count;         /* MIN_COUNT (generate_graph.cpp:40): a JUNC line exists for an edge whose counters sum to >= it (:1061) */
    const uint8_t *seed;       /* per contig: bit 0 in blast_segs (filter_graph.py:66-94), bit 1 in gene_res (:99-102), bit 2 score > threshold (:104-112) */
    const int32_t *tlen;       /* target lengths: a contig has a SEG line iff its length is > 0 (generate_graph.cpp:1019-1050) */
    const int32_t *rank;       /* dense rank of the names in byte order = order of the SEG lines of `_graph.txt` */
    const int32_t *name_len;   /* the length token of each name (get_edge_len, filter_graph.py:50-52) */
    int64_t n_paths;           /* lines of contigs.paths that are not NODE headers */
    const int64_t *path_off;   /* n_paths + 1 offsets into path_tok */
    const int32_t *path_tok;   /* 2 * contig + (orientation == '-'); -1 = an id no contig has */
} palace_stage04_inputs;

typedef struct palace_stage04 palace_stage04;
int palace_stage04_create(palace_ctx *ctx, const palace_stage04_inputs *in, palace_stage04 **out);
int palace_stage04_destroy(palace_ctx *ctx, palace_stage04 *s);

/* Optional: allocate now what a filter call with this edge bound will need (hundreds of MB for a million contigs; the
 * allocation alone takes tens of milliseconds), e.g. while the caller is still decoding its BAM.  The object's memory belongs
 * to the device: it may be created and reserved through one context and used through another. */
int palace_stage04_reserve(palace_ctx *ctx, palace_stage04 *s, int64_t edge_bound);

/* B2 in memory (filter_graph.py:201-264): which junctions and which SEG lines `_filtered_graph.txt` holds.  d_edges and
 * d_n_edges (device, 8 bytes) are what palace_graph_resolve_ex leaves; edge_bound is a bound on the count the host knows
 * (the number of candidates): it sizes the tables.  Only enqueues.  Per edge a flag byte: 1 = the JUNC line exists,
 * 2 = kept by pass 2 (:223-233), 4 = kept by pass 3 (:237-245); per contig: 1 = its SEG line is selected (seed, or end
 * of a kept junction), 2 = rescued through contigs.paths only (:126-151, written with the ` 0 1.0 0` tail), 4 = core seed.
 * The file lists the selected SEG lines, then the rescued ones, then the pass-2 junctions and the pass-3 junctions that are
 * not pass-2 ones, each group in `_graph.txt` order. */
int palace_stage04_filter(palace_ctx *ctx, palace_stage04 *s, const palace_graph_edge *d_edges, const int64_t *d_n_edges,
                          int64_t edge_bound);
/* the flags on the host (waits for the stream); n_edges <= edge_bound entries of the edge flags */
int palace_stage04_flags(palace_ctx *ctx, palace_stage04 *s, uint8_t *h_seg_flags, uint8_t *h_edge_flags, int64_t n_edges);
/* counts[8] = edges, JUNC lines, junctions kept by pass 2, further junctions kept by pass 3, selected SEG lines, rescued SEG
 * lines, merged arcs (-1 before palace_stage04_match), segments of the filtered graph (waits for the stream); also reports
 * what the reference script dies on: a contigs.paths id that names no contig, a rescued contig without SEG line */
int palace_stage04_counts(palace_ctx *ctx, palace_stage04 *s, int64_t counts[8]);

/* M1 on the filtered graph: `matching -g <filtered graph> -i <iterations> [-l contigs.paths] [--aggressive]` (palace:587-590)
 * on the device.  Segments are numbered as the filtered file lists them; copies = max(1, d_cn[contig]); arcs = kept junctions
 * (weight n1 + n2) + conjugates, and with use_paths the path-backed arcs.  Only enqueues (at most 10 iterations +
 * aggressive per filter call's reservation). */
int palace_stage04_match(palace_ctx *ctx, palace_stage04 *s, const palace_graph_edge *d_edges, const int32_t *d_cn,
                         int32_t iterations, int32_t aggressive, int32_t use_paths);
/* Waits and hands out the result in the compact form of palace_match_decompose_ex (vertices 2 * segment + orientation,
 * segments = ids of the filtered graph; bare segments as bits), owned by `s` (valid until the next match call or destroy;
 * palace_match_result_free on it does nothing), and contig_of[filtered segment] -> contig (n_segs_filtered entries). */
int palace_stage04_result(palace_ctx *ctx, palace_stage04 *s, palace_match_result **out, const int32_t **contig_of_out,
                          int64_t *n_segs_filtered_out);

/* ---- paths -> FASTA: the assembly's index, its names, and the output text gathered on the device (make_fa_from_path) ------- */

#define PALACE_FASTA_TILE_BYTES 4096       /* bytes of text one workgroup of the index kernels looks at */

/* One record of a FASTA text in device memory, what a `.fai` row holds (48 bytes): the name is text[name_off .. name_off +
 * name_len), the bytes behind '>' up to the first space, TAB, CR or LF; seq_off: offset of the byte behind the header line's LF
 * (the text's length when the header line is the text's last and has no LF); length: sequence bytes; line_bases / line_width:
 * those of the record's first sequence line (width = bases + CR + LF as present; both 0 when no line follows the header in the
 * record).  Base p of the record is text[seq_off + p / line_bases * line_width + p % line_bases]. */
typedef struct {
    int64_t name_off, name_len, seq_off, length, line_bases, line_width;
} palace_fasta_rec;

#define PALACE_FASTA_OK 0
#define PALACE_FASTA_ETEXT 1      /* the text does not begin with '>' (reported at line 1) */
#define PALACE_FASTA_ENAME 2      /* a header line without a name */
#define PALACE_FASTA_ERAGGED 3    /* a sequence line behind a line that is not the first line's bases and width, or longer than it */
#define PALACE_FASTA_EBLANK 4     /* a sequence line behind a blank line of its record */
#define PALACE_FASTA_EBYTE 5      /* a sequence byte outside 0x21-0x7E (a CR directly before the LF is not one) */

/* n_records: header lines of the text; error / bad_line: the smallest (1-based line, code) pair among the text's faults, 0 / 0
 * when it has none */
typedef struct {
    int64_t n_records, bad_line;
    int32_t error, reserved;
} palace_fasta_status;

/* The index of the FASTA text d_text[0 .. n) (16-byte aligned), the rules of samtools faidx restated line by line so that every
 * line is judged by itself, its successor and its record's first line -- the verdict does not depend on how the text falls into
 * tiles: lines end at LF, a last line without LF is a line; a line that begins with '>' begins a record; a blank line has no
 * bases.  A sequence line L with bases that is not its record's first is at fault when the line P before it is blank (EBLANK),
 * when P's bases or width differ from the first line's, or when L has more bases than the first line (ERAGGED): a record's last
 * line may be shorter, blank lines may only follow it.  Writes the records in file order to d_recs[0 .. n_records) when
 * n_records <= recs_cap and nothing otherwise (a record is at least 3 bytes of text; a caller may also ask with recs_cap = 0
 * and come back); with a fault the records mean nothing.  Four launches whatever the text holds (count, scan, records, lines)
 * over tiles of PALACE_FASTA_TILE_BYTES; a line or a record may span any number of tiles.  d_scratch:
 * palace_fasta_index_scratch_bytes(n) bytes of device memory.  Waits for the stream (it hands the status back). */
size_t palace_fasta_index_scratch_bytes(int64_t n);
int palace_fasta_index(palace_ctx *ctx, const uint8_t *d_text, int64_t n, palace_fasta_rec *d_recs, int64_t recs_cap, void *d_scratch,
                       size_t scratch_bytes, palace_fasta_status *status_out);

/* The records' names as a hash table on the device, built from the text where it lies (d_text and d_recs stay the caller's and
 * must outlive the table; n_records < 2^29).  Of records with byte-equal names the FIRST is the one a look-up finds; d_dup, when
 * not null, gets one byte per record: 1 when an earlier record has its name.  Enqueues only; destroy waits for the stream. */
typedef struct palace_fasta_names palace_fasta_names;
int palace_fasta_names_create(palace_ctx *ctx, const uint8_t *d_text, const palace_fasta_rec *d_recs, int64_t n_records, uint8_t *d_dup,
                              palace_fasta_names **out);
int palace_fasta_names_destroy(palace_ctx *ctx, palace_fasta_names *names);

#define PALACE_PATH_NOTHING (-1)   /* the token contributes no sequence */
#define PALACE_PATH_NOT_FOUND (-2) /* neither the name nor the name without its last '_' part is a record */
#define PALACE_PATH_REVERSE 1      /* bit 0 of a code >= 0: the record is taken reverse-complemented */
#define PALACE_PATH_SECOND_TRY 2   /* bit 1: found only without its last '_'-separated part; the record is code >> 2 */

/* Tokens of a paths file looked up: token t is d_tok[d_tok_off[t] .. d_tok_off[t + 1]), spaces removed and white space stripped
 * by the host.  A token of at most one byte contributes nothing; a last byte '+' or '-' is the strand and the rest the name,
 * otherwise the whole token is the name, taken forward; a name that is no record is tried once more cut before its last '_' (a
 * name without '_' becomes the empty name, which no record has).  d_code[t] gets one of the values above.  Enqueues only. */
int palace_path_resolve(palace_ctx *ctx, const palace_fasta_names *names, const uint8_t *d_tok, const int64_t *d_tok_off, int64_t n_tok,
                        int32_t *d_code);

/* Path p holds the tokens d_path_off[p] .. d_path_off[p + 1] (n_paths + 1 ascending entries, the last one n_tok).  Writes
 * d_tok_cum[0 .. n_tok]: the sequence bytes of all tokens in front of token t (a token without record has none), and
 * d_path_len[p]: the sequence bytes of path p -- a scan over the tokens, the paths' sums are differences of it.  Enqueues only. */
int palace_path_fasta_lengths(palace_ctx *ctx, const palace_fasta_rec *d_recs, const int32_t *d_code, int64_t n_tok, const int64_t *d_path_off,
                              int64_t n_paths, int64_t *d_tok_cum, int64_t *d_path_len);

/* Bytes [lo, hi) of the output text to d_out[0 .. hi - lo) (d_out 16-byte aligned; nothing outside that range is written).  The
 * text is, path by path, '>' header LF sequence LF: path p begins at byte d_path_out[p] (n_paths + 1 entries: d_path_out[p + 1] =
 * d_path_out[p] + header length + sequence length + 3), its header is d_hdr[d_hdr_off[p] .. d_hdr_off[p + 1]), its sequence the
 * tokens' records one behind the other, a reversed one read from its end with A<->T, C<->G, a<->t, c<->g swapped and every other
 * byte as it is.  d_code, d_tok_cum, d_path_off as palace_path_fasta_lengths left them.  Any 0 <= lo <= hi <= d_path_out[n_paths]
 * will do.  A lane writes 16 aligned bytes of d_out; the path of a tile's first and last byte is searched once per tile, a lane
 * searches its token once and walks on from there.  Enqueues only. */
int palace_path_fasta_write(palace_ctx *ctx, const uint8_t *d_text, const palace_fasta_rec *d_recs, const int32_t *d_code,
                            const int64_t *d_tok_cum, const int64_t *d_path_off, int64_t n_paths, const uint8_t *d_hdr,
                            const int64_t *d_hdr_off, const int64_t *d_path_out, int64_t lo, int64_t hi, uint8_t *d_out);

/* ---- the final FASTA: the cycle test of every path, the trim, and the output text (make_final_fa; the rules: DESIGN.md 8) ---- */

/* The fuzzy cycle test.  Tokens are integers: d_node[t] the id of the whole token, d_base[t] >= 0 the id of its base name,
 * d_len[t] >= 0 its length (n_tok < 2^31 entries each; tokens of equal base have equal lengths -- the caller's promise -- and a
 * path's lengths sum to less than 2^62).  Path p holds the tokens d_path_off[p] .. d_path_off[p + 1] (n_paths + 1 ascending
 * entries, the last one n_tok, which is handed in so that the call need not wait for the device).  d_arcs: n_arcs keys
 * (source node id << 32 | destination node id), ascending, duplicates allowed.  Over all 0 <= i <= j < L of a path of L tokens an
 * interval [i, j] passes when trimmed = sum len[0 .. i) + sum len(j .. L) <= trim_threshold, the arc path[j] -> path[i] exists,
 * and the lengths of the DISTINCT bases of path[i .. j] sum to min_cycle_length at least.  d_first[p] / d_last[p] = i / j of the
 * passing interval of least (trimmed, i, j), both -1 when none passes (a path without tokens, a negative threshold, no arcs).  No
 * length of a path is compiled in: a workgroup owns a path, its waves take values of i, their lanes values of j; the prefix sums
 * bound i from above and j from below before an arc is searched.  The previous token of the same base in the path -- the
 * distinct-base sum of [i, j] adds len[k] where that token lies before i -- comes from a stable palace_sort_u64 of the bases.
 * Temporaries come from the context's workspace.  Enqueues only. */
int palace_cycle_trim(palace_ctx *ctx, const int32_t *d_node, const int32_t *d_base, const int64_t *d_len, int64_t n_tok,
                      const int64_t *d_path_off, int64_t n_paths, const uint64_t *d_arcs, int64_t n_arcs, int64_t trim_threshold,
                      int64_t min_cycle_length, int32_t *d_first, int32_t *d_last);

/* palace_path_fasta_lengths for the final FASTA.  d_code as palace_path_resolve leaves it, except that a code with
 * PALACE_PATH_SECOND_TRY set counts as not found like a negative one.  A found token is preceded by sep_len separator bytes iff
 * the found tokens before it in its path brought at least one byte.  d_tok_cum[0 .. n_tok]: the bytes, separators included, of
 * all tokens in front of token t (token t's own separator lies at d_tok_cum[t], its record behind it); d_path_len[p]: the
 * sequence bytes of path p.  Enqueues only. */
int palace_final_fasta_lengths(palace_ctx *ctx, const palace_fasta_rec *d_recs, const int32_t *d_code, int64_t n_tok, const int64_t *d_path_off,
                               int64_t n_paths, int64_t sep_len, int64_t *d_tok_cum, int64_t *d_path_len);

/* palace_path_fasta_write for the final FASTA: bytes [lo, hi) of the output text to d_out[0 .. hi - lo), nothing outside them.  A
 * path with d_path_out[p + 1] == d_path_out[p] has no text at all (no header either): that is a path whose sequence is empty.
 * Every other path is '>' header LF sequence LF as there, its sequence the tokens' separators (sep_byte) and records as
 * palace_final_fasta_lengths placed them.  A reversed record is read from its end and complemented by the ambiguous-DNA table in
 * either case: A<->T, C<->G, R<->Y, K<->M, B<->V, D<->H; S, W, N and every other byte stay.  A lane writes 16 aligned bytes, the
 * path of a tile's first and last byte is searched once per tile.  Enqueues only. */
int palace_final_fasta_write(palace_ctx *ctx, const uint8_t *d_text, const palace_fasta_rec *d_recs, const int32_t *d_code,
                             const int64_t *d_tok_cum, const int64_t *d_path_off, int64_t n_paths, const uint8_t *d_hdr,
                             const int64_t *d_hdr_off, const int64_t *d_path_out, int32_t sep_byte, int64_t lo, int64_t hi, uint8_t *d_out);

/* ---- filter_result: the BLAST table's groups, the paths' classes, the first of equal paths (the rules: DESIGN.md 8) ---------- */

/* Faults of a line of the BLAST table (csrc/blast_line.hpp states the grammar) */
#define PALACE_BLAST_ECOLUMNS 1   /* fewer than four TAB-separated columns */
#define PALACE_BLAST_ENAME 2      /* an empty query or subject */
#define PALACE_BLAST_EIDENTITY 3  /* column 2 is not digits[.digits] with at most 3 digits before and 6 behind the point */
#define PALACE_BLAST_ELENGTH 4    /* column 3 is not 1-10 digits */
#define PALACE_BLAST_EQUERY 5     /* the query of a group's first line is no record of the FASTA */
#define PALACE_BLAST_EQEMPTY 6    /* ... or a record without bases */

/* cut[k], k = 0 .. 6: the smallest integer N in [0, 10^(3 + k)] with (double)N / 10^k > threshold (10^(3 + k) when there is none):
 * an identity spelt with k decimals, its digits read as the integer V, passes `float(text) > threshold` iff V >= cut[k].  Host
 * arithmetic only. */
int palace_blast_identity_cuts(double threshold, int64_t *cut);

/* The groups of a BLAST table (`-outfmt 6`) that lies on the device, its lines cut by palace_sam_lines (line i =
 * [d_line_start[i], d_line_start[i + 1] - 1), n_lines < 2^29).  Lines are taken in file order; a line begins a new group when its
 * query or its subject differs from the previous line's, compared byte by byte.  A group's sum: the line that begins it by
 * differing adds its alignment length whatever its identity, the table's first line and every line inside a group add theirs when
 * the identity passes cut (palace_blast_identity_cuts of blast_ratio * 100).  A group with (double)sum / (double)length of the
 * query's record > blast_ratio -- an IEEE division -- sets d_seg[record] = 1; d_seg[0 .. n_records) is cleared first (n_records:
 * the records of `names`, whose text and records must still be there).  The query of a group's first line is looked up in `names`.
 * out[0] = lines, out[1] = groups, out[2] = records flagged, out[3] / out[4] = the smallest 1-based number of a faulty line and
 * its PALACE_BLAST_E* code, 0 / 0 for none; with a fault no group is judged and d_seg stays clear.  A wavefront owns a line and
 * finds its TABs by ballot; the sums are two scans over the lines, so a group may span any number of workgroups.  Results are
 * integers and do not depend on scheduling.  Temporaries come from the context's workspace.  Waits for the stream. */
int palace_blast_groups(palace_ctx *ctx, const uint8_t *d_text, const int64_t *d_line_start, int64_t n_lines, const palace_fasta_names *names,
                        int64_t n_records, double blast_ratio, const int64_t *cut, uint8_t *d_seg, int64_t *out);

#define PALACE_FILTERRES_REC_GENE 1    /* a record's byte: its name is in the gene hit list */
#define PALACE_FILTERRES_REC_S07 2     /* its score is > 0.7 */
#define PALACE_FILTERRES_REC_S09 4     /* its score is >= 0.9 */
#define PALACE_FILTERRES_REC_BLAST 8   /* palace_blast_groups flagged it */
#define PALACE_FILTERRES_TAG_SELF 1    /* a path's tag byte: a line beginning with "self" stands before it */
#define PALACE_FILTERRES_TAG_CYCLE 2   /* ... a line beginning with "iter" */
#define PALACE_FILTERRES_WRITE 1       /* a path's class byte: it gets a FASTA record (if it is the first of its equals that do) */
#define PALACE_FILTERRES_PLAIN 2       /* `<joined>` enters the result set */
#define PALACE_FILTERRES_SELFGENE 4    /* `selfgene<joined>` is printed and enters the result set */
#define PALACE_FILTERRES_CYCLEGENE 8   /* `cyclegene<joined>` */
#define PALACE_FILTERRES_CYCLESCORE 16 /* `cyclescore<joined>` */
#define PALACE_FILTERRES_GENESCORE 32  /* `genescore<joined>` is printed */

/* The class of every path (d_code as palace_path_resolve left it, a negative code or one with PALACE_PATH_SECOND_TRY brings
 * nothing; path p holds the tokens d_path_off[p] .. d_path_off[p + 1]; n_paths < 2^31).  gene / s07 / s09: any token's record has
 * the bit; all_len: the records' lengths summed; blast_len: those of the records with PALACE_FILTERRES_REC_BLAST.  A path of one
 * token under TAG_SELF is SELFGENE when gene or s07, else WRITE | PLAIN.  Every other path with tokens: under TAG_CYCLE, gene gives
 * CYCLEGENE and s09 CYCLESCORE; with flags = gene or (all_len != 0 and (double)blast_len / (double)all_len > 0.2) the path is
 * dropped when not flags and (not s09 or all_len < 1000); a path that is not dropped has WRITE, and GENESCORE when gene and s09.
 * d_class[p] / d_all_len[p] get the class and all_len.  A wavefront owns a path, its lanes stride the tokens.  Enqueues only. */
int palace_filter_result_plan(palace_ctx *ctx, const int32_t *d_code, const int64_t *d_path_off, int64_t n_paths, const uint8_t *d_tag,
                              const palace_fasta_rec *d_recs, const uint8_t *d_rec_bits, uint8_t *d_class, int64_t *d_all_len);

/* d_first[p]: the bits of d_class[p] (its low six) for which p is the first path, in file order, with that bit among the paths whose
 * code sequence is IDENTICAL to p's.  Exact and deterministic: the low hash_bits (0 .. 64; an executable passes 64) of a 64-bit
 * hash of the sequences only bring candidates together -- a stable palace_sort_u64 -- and every path then finds the first member of
 * its run that equals it code by code; what is kept per class bit is a minimum of path indices.  Temporaries come from the
 * context's workspace.  Enqueues only. */
int palace_paths_first_of_equal(palace_ctx *ctx, const int32_t *d_code, const int64_t *d_path_off, int64_t n_paths, const uint8_t *d_class,
                                int32_t hash_bits, uint8_t *d_first);

/* ---- corrected_dup: borders, tandem candidates, the similarity relation, the base-set test (the rules: DESIGN.md 8) ---------- */

/* Paths are integers here as for palace_cycle_trim: d_node[t] the id of a whole token, path p the tokens d_path_off[p] ..
 * d_path_off[p + 1] (n_paths + 1 ascending entries; n_paths < 2^31; a path may be empty).  No path length and no path count is
 * compiled in, every result is an integer and none depends on scheduling. */

/* d_border[p] = the largest i in 1 .. n / 2 with path[0 .. i) == path[n - i .. n), token by token, or 0 when there is none (n:
 * the path's tokens).  A workgroup owns a path, its waves take values of i, their lanes stride the i comparisons.  Enqueues only. */
int palace_path_borders(palace_ctx *ctx, const int32_t *d_node, const int64_t *d_path_off, int64_t n_paths, int32_t *d_border);

/* The tandem candidates of every path of fewer than 2^20 tokens.  For a period r = 1 .. n / 2 and a start s = 0 .. n - 2 r, R(r, s)
 * is the number of consecutive q = s, s + 1, .. with q + r < n and path[q] == path[q + r]; (r, s) is a candidate when
 * c = 1 + R / r (integer division) is 2 at least.  d_cand_off[p] (n_paths + 1 entries, always written): the candidates of the
 * paths in front of p, the last entry their number, also in *n_cand_out.  With d_cand and cap >= that number, the candidates
 * follow as three int32 each -- r, s, c -- per path in ascending (r, s); without d_cand nothing else is written, and a cap that is
 * too small is refused: count with one call, fill with a second.  A workgroup owns a path and loops over the periods; R is a
 * segmented suffix scan over the flags path[q] == path[q + r] (ballots inside a wave, the waves and the chunks joined through
 * LDS), so a path of equal tokens costs what any other path of its length does, and no table of n x n entries exists.  The
 * counts come from the context's workspace.  Waits for the stream for the count; the fill is enqueued. */
int palace_path_tandems(palace_ctx *ctx, const int32_t *d_node, const int64_t *d_path_off, int64_t n_paths, int64_t *d_cand_off, int32_t *d_cand,
                        int64_t cap, int64_t *n_cand_out);

#define PALACE_PATHS_REL_NONE 0      /* a pair's two bits: the paths are not similar */
#define PALACE_PATHS_REL_J_LOSES 1   /* similar, and S(i) > S(j) */
#define PALACE_PATHS_REL_I_LOSES 2   /* similar, and S(i) <= S(j) */

/* The similarity relation of n_paths < 2^15 paths over the tokens' lengths (d_len[t] in 0 .. 2^32 - 1, n_tok < 2^31).  D(p): the
 * set of distinct lengths of p's tokens, S(p) their sum, I(i, j) the sum of D(i) intersected with D(j).  i < j are similar when
 * 10 I >= 9 S(i) or 10 I >= 9 S(j) -- for sums below 2^49 exactly `(double)I / (double)S >= 0.9`; a call with a
 * larger S is refused.  d_rel: palace_paths_length_relation_bytes(n_paths) bytes, all written; the pair (i, j), i < j, has the two
 * bits 2 (k & 3) of byte k >> 2, k = i * n_paths + j; every other pair of bits is 0.  The distinct lengths come from one stable
 * palace_sort_u64 of path << 32 | length and a scan of the flags `differs from the key before`; a lane owns a byte of d_rel and
 * searches the shorter set's values in the longer.  Temporaries come from the context's workspace.  Waits for the stream. */
size_t palace_paths_length_relation_bytes(int64_t n_paths);
int palace_paths_length_relation(palace_ctx *ctx, const int64_t *d_len, int64_t n_tok, const int64_t *d_path_off, int64_t n_paths, uint8_t *d_rel);

/* d_in[p] (n_paths entries): 1 when p >= n_cycles and the SET of p's values d_base[t] (>= 0; n_tok < 2^31) equals the set of one
 * of the paths 0 .. n_cycles - 1, else 0.  Exact: the sets are compared as sorted lists of distinct values (the sort and scan of
 * palace_paths_length_relation); the low hash_bits (0 .. 64; an executable passes 64) of a 64-bit hash of a list only bring
 * candidates together, through a stable palace_sort_u64 of the cycles' hashes.  Two empty paths have equal sets.  Temporaries
 * come from the context's workspace.  Waits for the stream once (the values' check). */
int palace_paths_base_set_in(palace_ctx *ctx, const int32_t *d_base, int64_t n_tok, const int64_t *d_path_off, int64_t n_paths, int64_t n_cycles,
                             int32_t hash_bits, uint8_t *d_in);

/* ---- FASTG -> node FASTA and the `.fai` rows of both, on the device (split_fastg; the rules: DESIGN.md 8) -------------------- */

/* Faults of a FASTG text beyond those of palace_fasta_index, reported in a palace_fasta_status like them */
#define PALACE_FASTG_EPLUS 6      /* a sequence line that begins with '+' or '@' */
#define PALACE_FASTG_EHIGH 7      /* a byte of 0x80 or above in a header line */
#define PALACE_FASTG_ECR 8        /* a CR in a header line that is not directly before the LF */
#define PALACE_FASTG_ENOLF 9      /* the text's last byte is not LF (reported at the last line) */
#define PALACE_FASTG_EEMPTY 10    /* the text is empty (reported at line 1) */
#define PALACE_FASTG_ENONAME 11   /* a header whose V (see palace_fastg_derive) is empty */
#define PALACE_FASTG_EBASE 12     /* a byte other than A, C, G, T (either case) in the sequence of a primed record */

/* The records of an indexed FASTG text (d_recs[0 .. n_records) as palace_fasta_index left them; that index's verdict is not asked
 * for: name_off and seq_off hold whatever it is) named by the rule of split_fastg.py.  T: the bytes behind '>' up to the first
 * space or the line's end (a CR directly before the LF is not the line's); U: T without its last byte; V: U up to its first ':'
 * or ','; V ending in ' makes the record primed and the name V without that byte (it may be empty), otherwise the name is V.
 * d_name_recs[r] is d_recs[r] with name_len the derived name's -- palace_fasta_names_create takes them as they are -- and
 * d_primed[r] the primed bit.  status_out: n_records as given, and the smallest (1-based line, code) among the PALACE_FASTG_
 * faults above (0 / 0: none); the caller takes the smaller of it and the index's.  One lane per record for the names, one per
 * 16 bytes of text for everything else (the bases of a primed record are checked where they lie, however long the record); a
 * fault is reduced as the smallest offset per code and its line counted afterwards, so the verdict does not depend on tiling.
 * Waits for the stream. */
int palace_fastg_derive(palace_ctx *ctx, const uint8_t *d_text, int64_t n, const palace_fasta_rec *d_recs, int64_t n_records,
                        palace_fasta_rec *d_name_recs, uint8_t *d_primed, palace_fasta_status *status_out);

/* The output's layout.  d_dup: palace_fasta_names_create's flags over d_name_recs; a record whose flag is set is dropped.  (That
 * table never finds the name of no bytes and flags every record that has it: here the first of those is kept, and d_dup is put
 * right.)  d_out_off[0 .. n_records]: the 64-bit exclusive scan of 1 + name_len + 1 + length + 1 over the kept records, the last
 * entry the output's bytes; d_out_recs (may be null): record r as a record of the OUTPUT text -- name_off and name_len as
 * given (the name's bytes stay in the FASTG text), seq_off its sequence's place in the output, length, and line_bases = length,
 * line_width = length + 1 (both 0 for a record without bases) -- meaningful for kept records.  Waits for the stream. */
int palace_fastg_plan(palace_ctx *ctx, const palace_fasta_rec *d_name_recs, uint8_t *d_dup, int64_t n_records, int64_t *d_out_off,
                      palace_fasta_rec *d_out_recs, int64_t *n_kept_out, int64_t *out_bytes_out);

/* Bytes [lo, hi) of the output text to d_out[0 .. hi - lo) (d_out 16-byte aligned; nothing outside that range is written): per
 * kept record '>' name LF sequence LF in file order.  A forward record's bases are copied as they are; a primed record's are read
 * from the end, upper-cased and complemented (A<->T, C<->G).  Only for a text without fault.  Any 0 <= lo <= hi <=
 * d_out_off[n_records] will do; a lane writes 16 aligned bytes, the records of a tile's first and last byte are searched once
 * per tile; a record may span any number of tiles and a tile may hold any number of records.  Enqueues only. */
int palace_fastg_write(palace_ctx *ctx, const uint8_t *d_text, const palace_fasta_rec *d_name_recs, const uint8_t *d_primed,
                       const int64_t *d_out_off, int64_t n_records, int64_t lo, int64_t hi, uint8_t *d_out);

/* The `.fai` rows of records whose names lie in a text on the device: name TAB length TAB seq_off TAB line_bases TAB line_width LF
 * in decimal, none for a record with d_skip[r] set (d_skip may be null).  plan: d_row_off[0 .. n_records], the 64-bit scan of the
 * rows' lengths, and their sum (waits for the stream); write: all rows to d_out[0 .. that sum), one lane per row (enqueues only). */
int palace_fai_rows_plan(palace_ctx *ctx, const palace_fasta_rec *d_recs, const uint8_t *d_skip, int64_t n_records, int64_t *d_row_off,
                         int64_t *bytes_out);
int palace_fai_rows_write(palace_ctx *ctx, const uint8_t *d_text, const palace_fasta_rec *d_recs, const uint8_t *d_skip, int64_t n_records,
                          const int64_t *d_row_off, uint8_t *d_out);

/* ---- faidx: regions of an indexed FASTA as FASTA text (`samtools faidx <file.fa> region ...`; the rules: DESIGN.md 8) --------- */

/* One resolved region (24 bytes): rec the record, -1 for a region that fails; beg its first base, 0-based; len its bases, after
 * clipping to the record's length. */
typedef struct {
    int64_t rec, beg, len;
} palace_faidx_region;

/* Region i is d_reg[d_reg_off[i] .. d_reg_off[i + 1]) (n_regions + 1 ascending entries).  A region that is a record's name, whole,
 * is that record; otherwise it is cut at its LAST ':' -- the part in front must be a record's name, the part behind is B, B-E, B-
 * or -E: decimal digits in which ',' is ignored, at least one and at most 18 digits a number, 1-based and inclusive, B = 0 counted
 * as 1, a missing B 1, a missing E the record's length.  E beyond the length is the length; B beyond the length gives len = 0 (beg
 * = the length), which is no failure; E < B as written, a range of no bytes and every other byte fail, as does a name no record
 * has (the empty one too).  Of records with equal names the first is found (names: palace_fasta_names_create's table over
 * d_recs, whose lengths are read).  The grammar is csrc/faidx_region.hpp's.  One lane per region.  Enqueues only. */
int palace_faidx_resolve(palace_ctx *ctx, const palace_fasta_names *names, const palace_fasta_rec *d_recs, const uint8_t *d_reg,
                         const int64_t *d_reg_off, int64_t n_regions, palace_faidx_region *d_out);

/* The output's layout for lines of line_len >= 1 bases.  Region i has a header of d_hdr_off[i + 1] - d_hdr_off[i] bytes and takes
 * 1 + header + 1 + len + ceil(len / line_len) bytes, a failed region none.  d_out_off[0 .. n_regions]: the 64-bit exclusive scan of
 * those sizes; *total_out: its last entry; *first_failed_out: the smallest failed region, -1 when there is none.  skip_failed = 0:
 * a failed region leaves no text at all -- every entry of d_out_off and *total_out are 0.  Waits for the stream. */
int palace_faidx_plan(palace_ctx *ctx, const palace_faidx_region *d_regions, int64_t n_regions, const int64_t *d_hdr_off, int64_t line_len,
                      int skip_failed, int64_t *d_out_off, int64_t *total_out, int64_t *first_failed_out);

/* Bytes [lo, hi) of the output text to d_out[0 .. hi - lo) (d_out 16-byte aligned; nothing outside that range is written): per
 * region with text '>' header LF, then its bases in lines of line_len, every line -- the last, possibly shorter, too -- ended by
 * LF; a region of 0 bases is its header line alone.  The header is d_hdr[d_hdr_off[i] .. d_hdr_off[i + 1]).  reverse != 0: every
 * region's bases are read from the range's end through the ambiguous-DNA complement of palace_final_fasta_write.  d_regions and
 * d_out_off as palace_faidx_resolve and palace_faidx_plan left them; any 0 <= lo <= hi <= d_out_off[n_regions] will do.  A lane
 * writes 16 aligned bytes; the regions of a tile's first and last byte are searched once per tile; 16 bases that lie in one output
 * line and one line of the record are one load and one store, everything else is walked byte by byte across line ends, regions
 * and the window's edges.  All offsets are 64-bit.  Enqueues only. */
int palace_faidx_write(palace_ctx *ctx, const uint8_t *d_text, const palace_fasta_rec *d_recs, const palace_faidx_region *d_regions,
                       int64_t n_regions, const uint8_t *d_hdr, const int64_t *d_hdr_off, const int64_t *d_out_off, int64_t line_len,
                       int reverse, int64_t lo, int64_t hi, uint8_t *d_out);

/* ---- the phage scorer's input: k-mer pair features of every record of an indexed FASTA (phage_scoring; the rules: DESIGN.md 8) */

#define PALACE_CONTIG_FEATURES 12288       /* 3 distances x 64 x 64 pairs of 3-mers */
#define PALACE_CONTIG_FSUMS    64          /* row sums of the first distance's matrix */
#define PALACE_CONTIG_CHUNK_BASES 4096     /* positions of a record's sequence (kept or dropped) that one workgroup looks at; a
                                            * record with more of them is counted by several workgroups into one row */

typedef struct { int64_t length, bases; } palace_contig_info;      /* |S| and m: sequence bytes, and those that are A C G T a c g t */

/* The features of records [r0, r1) of the text d_text[0 .. n) under the index d_recs (palace_fasta_index without a fault).  Of a
 * record's sequence bytes S those that are A C G T in either case are kept and coded 0 1 2 3: v[0 .. m); loc[i] = 16 v[i] +
 * 4 v[i+1] + v[i+2]; C[d][loc[i]][loc[i+3+d]] counts 0 <= i < m - 5 - d for d = 0, 1, 2.  Row r - r0 of d_feat (PALACE_CONTIG_FEATURES
 * floats a row, 16-byte aligned) gets float(double(C[d][a][b]) / double(length) * 100.0) at (a * 64 + b) * 3 + d, row r - r0 of
 * d_fsum (PALACE_CONTIG_FSUMS floats) the same of the exact integer sum over b of C[0][a][b]; length 0 gives NaN in both.  d_info,
 * when not null, gets a record's length and m.  *d_bad: the smallest text offset of a byte '0'..'9' in a sequence of [r0, r1),
 * else -1; digits are dropped like every other byte, the caller decides what they mean.  Writes rows [0, r1 - r0) and nothing
 * else; r0 == r1 writes *d_bad alone.  Eleven launches whatever the text holds; the counts are integers added with integer
 * atomics, so the same call gives the same bytes.  d_scratch (16-byte aligned): palace_contig_features_scratch_bytes(n, r1 - r0)
 * bytes.  Enqueues only. */
size_t palace_contig_features_scratch_bytes(int64_t n_text, int64_t n_records);
int palace_contig_features(palace_ctx *ctx, const uint8_t *d_text, int64_t n, const palace_fasta_rec *d_recs, int64_t r0, int64_t r1,
                           float *d_feat, float *d_fsum, palace_contig_info *d_info, int64_t *d_bad, void *d_scratch, size_t scratch_bytes);

/* ---- bamsort: a BAM coordinate-sorted and indexed where its inflated stream lies (the rules: DESIGN.md 8) --------------------- */

/* One sort key per record of the stream (d_starts as palace_bam_walk leaves them): t << 33 | uint32(pos + 1) << 1 | reverse bit,
 * t = n_ref for refID = -1, else refID -- contig order with the records without a contig last, then position with pos = -1 first,
 * then forward before reverse (csrc/bam_record.hpp: sort_key).  A record with refID < -1, refID >= n_ref or pos < -1 has no key:
 * such records are counted into *n_bad_out and the smallest ordinal among them goes to *first_bad_out (-1: none).  Waits. */
int palace_bam_sort_keys(palace_ctx *ctx, const uint8_t *d_stream, int64_t total, const int64_t *d_starts, int64_t n_records,
                         int32_t n_ref, uint64_t *d_key, int64_t *n_bad_out, int64_t *first_bad_out);

#define PALACE_SORT_TILE 4096              /* T: the keys one workgroup of palace_sort_u64 ranks per pass (256 lanes x 16) */

/* A STABLE sort of n 64-bit keys (n < 2^31) by their low key_bits bits (0 .. 64); bits above key_bits may hold anything and are
 * IGNORED: keys that agree in the low key_bits bits keep their input order.  d_key comes out sorted (whole keys, the ignored bits
 * with them), d_perm[k] = the input ordinal of the key now at k (written, not read).  LSD radix sort, ceil(key_bits / 8) passes of
 * 8 bits (the last one narrower), three launches each: every workgroup ranks a tile of T = PALACE_SORT_TILE keys -- a wave takes
 * 64 consecutive keys at a time, the lanes with an equal digit find each other with eight ballots and rank themselves by the lanes
 * below, one lane per digit adds the group to the wave's own counters in LDS (no atomics; 4 KiB per workgroup) -- and leaves its
 * digit counts; one workgroup scans the counts digit-major; the tiles are ranked again and scattered.  The result depends neither
 * on key_bits being tight nor on T.  d_scratch: palace_sort_u64_scratch_bytes(n) bytes, 256-byte aligned.  Enqueues only. */
size_t palace_sort_u64_scratch_bytes(int64_t n);
int palace_sort_u64(palace_ctx *ctx, uint64_t *d_key, uint32_t *d_perm, int64_t n, int32_t key_bits, void *d_scratch,
                    size_t scratch_bytes);

/* The layout of the sorted stream: d_out_off[k] (n_records + 1 entries) = head_bytes + the bytes (4 + block_size each) of the
 * records d_perm[0 .. k), the last entry the stream's length, also in *out_bytes_out; d_out_starts (may be null): d_out_off[k] + 4,
 * the sorted stream's record starts as palace_bam_walk would leave them.  Waits for the stream. */
int palace_bam_gather_plan(palace_ctx *ctx, const uint8_t *d_stream, const int64_t *d_starts, const uint32_t *d_perm, int64_t n_records,
                           int64_t head_bytes, int64_t *d_out_off, int64_t *d_out_starts, int64_t *out_bytes_out);
/* Record d_perm[k]'s bytes, block_size word included, copied unchanged to d_out + d_out_off[k] for every k: bytes
 * [d_out_off[0], d_out_off[n_records]) of d_out (16-byte aligned; out_bytes = d_out_off[n_records] as the plan returned it) are
 * written and no others.  Output-driven: a lane owns 16 aligned bytes of d_out and finds its record in d_out_off, the records of a
 * tile's first and last byte are searched once per tile; source and destination have no alignment to each other.  Enqueues only. */
int palace_bam_gather_write(palace_ctx *ctx, const uint8_t *d_stream, const int64_t *d_starts, const uint32_t *d_perm,
                            const int64_t *d_out_off, int64_t n_records, int64_t out_bytes, uint8_t *d_out);

/* What a .bai (SAM specification 5.2) files each record of a coordinate-sorted stream under.  refID = -1: d_ref = -1 and d_bin =
 * d_win_beg = d_win_end = 0 (so the unplaced tail of a sorted stream is ONE run of palace_bai_chunks), the record is not indexed
 * and counted into n_no_coor.  Else beg = pos, end = pos + the reference bases of the CIGAR the record really has (M, D,
 * N, =, X; the CG tag's behind a placeholder), pos + 1 for flag 0x4, no ops or no reference bases; d_bin = reg2bin(beg, end), the
 * record's own bin field is not looked at; d_win_beg / d_win_end = beg >> 14, (end - 1) >> 14; d_unmapped = flag 0x4.  n_bad /
 * first_bad: the records a .bai cannot hold (refID >= n_ref or < -1, pos < 0 with a refID, end > 2^29) and the first one's
 * ordinal (-1: none); of a record counted in n_bad only d_unmapped is specified, its other four columns may hold anything.
 * first_unsorted: the first ordinal whose sort key is smaller than its predecessor's, a record without a key (palace_bam_sort_keys)
 * being out of order with neither neighbour (-1: the stream is coordinate-sorted).  Waits for the stream. */
typedef struct {
    int64_t n_bad, first_bad, first_unsorted, n_no_coor;
} palace_bai_status;
int palace_bai_records(palace_ctx *ctx, const uint8_t *d_stream, const int64_t *d_starts, int64_t n_records, int32_t n_ref,
                       int32_t *d_ref, int32_t *d_bin, int32_t *d_win_beg, int32_t *d_win_end, uint8_t *d_unmapped,
                       palace_bai_status *status_out);

/* The chunks: a run is a maximal stretch of consecutive records with equal (d_ref, d_bin); *n_runs_out = the number of runs.
 * Counted first, written second: with cap >= that number the runs are listed ordered by (refID, bin, file order) -- the unplaced
 * records' runs, d_chunk_ref = -1, last -- each as refID, bin, the stream offset of its first record's block_size word and the
 * offset behind its last record (four arrays of cap entries).  The run heads are compacted by a scan and ordered with
 * palace_sort_u64.  Temporaries come from the context's workspace.  Waits for the stream. */
int palace_bai_chunks(palace_ctx *ctx, const uint8_t *d_stream, const int64_t *d_starts, const int32_t *d_ref, const int32_t *d_bin,
                      int64_t n_records, int32_t n_ref, int32_t *d_chunk_ref, int32_t *d_chunk_bin, int64_t *d_chunk_beg,
                      int64_t *d_chunk_end, int64_t cap, int64_t *n_runs_out);

/* The linear index and the pseudo-bin's numbers.  Without d_lin: d_n_intv[t] = 1 + the largest d_win_end of reference t's records
 * (0 without records) and d_ref_stat, four arrays of n_ref entries one behind the other: records with flag 0x4 clear, records with
 * it set, the stream offset of the first record's block_size word, the offset behind the last record (the last two undefined for
 * a reference without records).  With d_lin (n_lin entries) and d_lin_off (n_ref + 1 entries, the exclusive sums of d_n_intv, the
 * last one n_lin): d_lin[d_lin_off[t] + w] = the smallest record start (block_size word) among t's records with d_win_beg <= w <=
 * d_win_end; a window no record touches takes the next touched window's value.  Enqueues only. */
int palace_bai_linear(palace_ctx *ctx, const uint8_t *d_stream, const int64_t *d_starts, const int32_t *d_ref, const int32_t *d_win_beg,
                      const int32_t *d_win_end, const uint8_t *d_unmapped, int64_t n_records, int32_t n_ref, int32_t *d_n_intv,
                      int64_t *d_ref_stat, const int64_t *d_lin_off, int64_t n_lin, int64_t *d_lin);

/* Stream offsets to BGZF virtual offsets: member m holds the stream bytes from d_member_u[m] and lies at file offset d_member_c[m]
 * (n_members >= 1 entries, d_member_u ascending; the last entry stands for the stream's end: the EOF member, or the file's end
 * where there is none).  d_voff[k] = c_m << 16 | (d_u[k] - u_m) for the LAST m with u_m <= d_u[k]: an offset on a member boundary
 * belongs to the member that starts there.  An offset outside [u_0, u_last] gives ~0.  Enqueues only. */
int palace_bgzf_voffsets(palace_ctx *ctx, const int64_t *d_u, int64_t n, const int64_t *d_member_u, const int64_t *d_member_c,
                         int64_t n_members, uint64_t *d_voff);

/* ---- samview: SAM text encoded as BAM records where the text lies (the rules: DESIGN.md 8, csrc/sam_line.hpp) ------------------- */

/* What is wrong with a SAM text.  Parity with samtools is UNPINNED: htslib is not at hand, these rules are the behaviour. */
#define PALACE_SAM_EAT 1          /* a line that begins with '@' behind the first alignment line */
#define PALACE_SAM_EEMPTY 2       /* an empty line */
#define PALACE_SAM_EFIELDS 3      /* fewer than 11 TAB-separated fields */
#define PALACE_SAM_EQNAME 4       /* QNAME: not 1 .. 254 bytes of '!' .. '~' */
#define PALACE_SAM_EFLAG 5        /* FLAG: not a decimal in 0 .. 65535 */
#define PALACE_SAM_ERNAME 6       /* RNAME: neither '*' nor a target of the header */
#define PALACE_SAM_EPOS 7         /* POS: not a decimal in 0 .. 2^31 - 1 */
#define PALACE_SAM_EMAPQ 8        /* MAPQ: not a decimal in 0 .. 255 */
#define PALACE_SAM_ECIGAR 9       /* CIGAR: neither '*' nor ([0-9]+[MIDNSHP=X])+, a length of 2^28 or more, more than 65535 ops */
#define PALACE_SAM_ERNEXT 10      /* RNEXT: none of '*', '=' and a target of the header */
#define PALACE_SAM_EPNEXT 11      /* PNEXT: not a decimal in 0 .. 2^31 - 1 */
#define PALACE_SAM_ETLEN 12       /* TLEN: not a decimal with an optional '-' within int32 */
#define PALACE_SAM_ESEQ 13        /* SEQ: an empty field */
#define PALACE_SAM_ECIGLEN 14     /* the CIGAR's query length (M, I, S, =, X) is not SEQ's length */
#define PALACE_SAM_EQUAL 15       /* QUAL: neither '*' nor as many bytes of 33 .. 126 as SEQ has */
#define PALACE_SAM_ETAG 16        /* a tag that is not XX:T:value with a type and a value this converter takes */
#define PALACE_SAM_ETAGRANGE 17   /* an integer of a tag outside its type: i within -2^31 .. 2^32 - 1, a B element within its subtype */
#define PALACE_SAM_ETAGFLOAT 18   /* a tag of type f or B:f: text to float is not done on the device */
#define PALACE_SAM_ETAGHEX 19     /* an H tag with an odd count of digits or a byte that is no hex digit */
#define PALACE_SAM_EHDSQ 20       /* header (host): an @SQ line without SN, or without an LN in 1 .. 2^31 - 1 */
#define PALACE_SAM_EHDDUP 21      /* header (host): two @SQ lines with one SN */

#define PALACE_SAM_TILE 4096               /* T: the text bytes one workgroup of palace_sam_lines takes (256 lanes x 16) */

/* The lines of a text of n bytes on the device (d_text 16-byte aligned): cut at LF, a last line without LF is a line, CR is a byte
 * like any other.  Every workgroup counts the LFs of its tile of T bytes, one workgroup scans the counts, the tiles are taken again
 * and each LF in front of the last byte writes the start behind it.  out[0] = the number of lines, always.  With d_line_start and
 * cap >= out[0] + 1: d_line_start[k] = the offset of line k's first byte, d_line_start[lines] = n + 1 for a text whose last byte is
 * no LF, else n -- so that line k is [d_line_start[k], d_line_start[k + 1] - 1) -- and out[1] = the header lines (the lines beginning
 * with '@' in front of the first line that does not), out[2] = the alignment lines (all others), out[3] / out[4] = the smallest
 * 1-based number of a line that is empty (PALACE_SAM_EEMPTY) or begins with '@' behind an alignment line (PALACE_SAM_EAT) and that
 * code, 0 / 0 for none.  Otherwise (the count) out[1 .. 4] = -1.  A line of more than 2^29 bytes is refused (PALACE_EINVAL).
 * d_scratch: palace_sam_scratch_bytes(n) bytes.  Waits for the stream. */
size_t palace_sam_scratch_bytes(int64_t n);
int palace_sam_lines(palace_ctx *ctx, const uint8_t *d_text, int64_t n, void *d_scratch, size_t scratch_bytes, int64_t *d_line_start,
                     int64_t cap, int64_t *out);

/* Alignment line i = [d_line_start[i], d_line_start[i + 1] - 1) for i < n_lines (the caller passes the entry of the first
 * alignment line; n_lines < 2^31), its number in the text line0 + i.  A wavefront owns a line: its lanes stride the bytes, the TABs
 * are found by ballot and the field cuts kept in LDS; QUAL's bytes, the CIGAR's ops and the tags are checked a lane each.  Every line
 * is validated in full; a valid line whose FLAG as written has a bit of `mask` is dropped.  RNAME and RNEXT are looked up in
 * `names` (palace_bam_names_create over the header's targets).  d_size[i] = the record's bytes with its block_size word, 0 for a
 * dropped line; d_off[0 .. n_lines] = head_bytes + the exclusive sums of d_size, the last entry the stream's length; d_ord[i] = the
 * kept lines in front of line i.  out[0] = kept, out[1] = dropped, out[2] = d_off[n_lines], out[3] / out[4] = the smallest number of
 * a line with an error and that line's code (0 / 0: none; then the other outputs mean nothing).  Waits for the stream. */
int palace_sam_plan(palace_ctx *ctx, const uint8_t *d_text, const int64_t *d_line_start, int64_t n_lines, int64_t line0,
                    const palace_bam_names *names, uint32_t mask, int64_t head_bytes, int32_t *d_size, int64_t *d_off,
                    int32_t *d_ord, int64_t *out);

/* Every kept line's record (SAM specification 4.2) at d_out + d_off[i], and d_starts[d_ord[i]] = d_off[i] + 4, the offset of its
 * refID, as palace_bam_walk would leave it.  Only for a text palace_sam_plan found no error in, with that call's arrays.  Bytes
 * [d_off[0], d_off[n_lines]) of d_out are written and no others; the stream has no alignment, every store is a byte's.  SEQ is
 * packed and QUAL shifted by the lanes of the line's wavefront, a byte of output each; string tags are copied the same way.
 * Enqueues only. */
int palace_sam_encode(palace_ctx *ctx, const uint8_t *d_text, const int64_t *d_line_start, int64_t n_lines,
                      const palace_bam_names *names, const int32_t *d_size, const int64_t *d_off, const int32_t *d_ord,
                      uint8_t *d_out, int64_t *d_starts);

/* ---- readqc: fastp's paired-read trimming and filtering where the two FASTQ texts lie (the rules: DESIGN.md 8, csrc/fastq_rules.hpp) -- */

/* What is wrong with a FASTQ text.  Parity with fastp is UNPINNED: fastp is not at hand, these rules are the behaviour. */
#define PALACE_FASTQ_ELINES 1     /* the text ends inside a record: fewer than 4 lines behind the last complete one (at its first line) */
#define PALACE_FASTQ_EAT 2        /* a record's line 0 does not begin with '@' */
#define PALACE_FASTQ_EPLUS 3      /* a record's line 2 does not begin with '+' */
#define PALACE_FASTQ_ELONG 4      /* SEQ of more than PALACE_FASTQ_MAX_SEQ bases */
#define PALACE_FASTQ_EBASE 5      /* SEQ: a byte that is none of A C G T N (CR included) */
#define PALACE_FASTQ_EQLEN 6      /* QUAL has not SEQ's length */
#define PALACE_FASTQ_EQUAL 7      /* QUAL: a byte outside 33 .. 126 (CR included) */
#define PALACE_FASTQ_ECOUNT 8     /* (host) the two files hold different numbers of records */

#define PALACE_FASTQ_MAX_SEQ 4096 /* the bases of a read: a wavefront of the plan holds both reads of a pair in 2 x 4096 bytes of LDS */

/* The option values of readqc (fastp's names in brackets) and the four constants of its overlap search.  The defaults:
 * {15, 40, 5, 15, 0, 0, 0, 30, 5, 20, 50, 0}. */
typedef struct {
    int32_t qualified_quality;     /* -q: a QUAL byte below 33 + this is a low one */
    int32_t unqualified_percent;   /* -u: a read fails when low * 100 > this * L */
    int32_t n_limit;               /* -n: ... or when it has more N than this */
    int32_t min_length;            /* -l: ... or when L is below this */
    int32_t no_trim;               /* -A */
    int32_t no_quality_filter;     /* -Q: neither the quality nor the N filter */
    int32_t no_length_filter;      /* -L */
    int32_t overlap_require;       /* 30: offsets o < L1 - 30 and k < L2 - 30 are searched */
    int32_t diff_limit;            /* 5 and */
    int32_t diff_pct;              /* 20: a candidate of n bases may have min(5, n * 20 / 100) mismatches */
    int32_t diff_window;           /* 50: ... among its first min(n, 50) positions; later ones are not looked at */
    int32_t reserved;
} palace_readqc_params;

/* the numbers palace_readqc_plan leaves in out[]: counts in reads (two per pair) and bases */
enum {
    PALACE_READQC_READS_BEFORE = 0, PALACE_READQC_BASES_BEFORE = 1, PALACE_READQC_READS_AFTER = 2, PALACE_READQC_BASES_AFTER = 3,
    PALACE_READQC_LOW_QUALITY = 4, PALACE_READQC_TOO_MANY_N = 5, PALACE_READQC_TOO_SHORT = 6,
    PALACE_READQC_TRIMMED_READS = 7,   /* reads that lost bases to the overlap rule (dropped pairs included) */
    PALACE_READQC_TRIMMED_BASES = 8,   /* ... and the bases they lost */
    PALACE_READQC_BYTES_1 = 9, PALACE_READQC_BYTES_2 = 10,    /* d_off1[n_pairs], d_off2[n_pairs] */
    PALACE_READQC_N_OUT = 11
};

/* The records of a FASTQ text whose lines palace_sam_lines has cut (d_line_start[0 .. n_lines], n_lines / 4 < 2^31): record r is the lines
 * 4r .. 4r + 3.  A wavefront owns a record and its lanes stride the bytes of SEQ and QUAL, so a record may lie across any number of
 * tiles.  d_seq_len[r] = SEQ's length.  out[0] = the complete records, out[1] / out[2] = the smallest 1-based number of a faulty line
 * and its PALACE_FASTQ_E* code, 0 / 0 for none.  Waits for the stream. */
int palace_fastq_records(palace_ctx *ctx, const uint8_t *d_text, const int64_t *d_line_start, int64_t n_lines, int32_t *d_seq_len,
                         int64_t *out);

/* Pair i of two texts palace_fastq_records found no fault in (their line starts; n_pairs records each): the overlap search, the trim
 * and the filter of csrc/fastq_rules.hpp, a wavefront per pair.  d_len1[i] / d_len2[i] = the bases read 1 / read 2 keeps, -1 / -1 for a
 * dropped pair; d_off1 / d_off2 [0 .. n_pairs] = the exclusive sums of the records' bytes in the two output texts;
 * out[PALACE_READQC_N_OUT] as the enum above.  Waits for the stream. */
int palace_readqc_plan(palace_ctx *ctx, const uint8_t *d_text1, const int64_t *d_line_start1, const uint8_t *d_text2,
                       const int64_t *d_line_start2, int64_t n_pairs, const palace_readqc_params *prm, int32_t *d_len1, int32_t *d_len2,
                       int64_t *d_off1, int64_t *d_off2, int64_t *out);

/* Bytes [lo, hi) of one output text to d_out[0 .. hi - lo) (16-byte aligned), 0 <= lo <= hi <= d_off[n_pairs]: every kept record is its
 * name line, SEQ[0 : len], line 2 and QUAL[0 : len], each with an LF.  A lane writes 16 bytes with one store; a tile of 4096 bytes
 * searches the record of its first byte once.  Nothing outside the range is written.  Enqueues only. */
int palace_readqc_write(palace_ctx *ctx, const uint8_t *d_text, const int64_t *d_line_start, const int32_t *d_len, const int64_t *d_off,
                        int64_t n_pairs, int64_t lo, int64_t hi, uint8_t *d_out);

/* ---- readqc --full-report: what the QC report counts (the rules: csrc/fastq_rules.hpp, "the report") ---------------------------- */

#define PALACE_READQC_ISIZE_MAX 512   /* insert sizes 0 .. 511 have a slot of their own; slot 512 is "unknown" (no overlap, or longer) */
#define PALACE_READQC_SLOTS 5         /* the base slots of every per-cycle table: A C G T N */

/* palace_readqc_plan with one more output: d_cand (NULL, or n_pairs entries) gets every pair's first accepted candidate in search
 * order, dropped pairs included; -1 for none, under no_trim, and for a pair that is not staged (not a text palace_fastq_records
 * passed).  With NULL it is palace_readqc_plan. */
int palace_readqc_plan_ex(palace_ctx *ctx, const uint8_t *d_text1, const int64_t *d_line_start1, const uint8_t *d_text2,
                          const int64_t *d_line_start2, int64_t n_pairs, const palace_readqc_params *prm, int32_t *d_len1, int32_t *d_len2,
                          int64_t *d_off1, int64_t *d_off2, int32_t *d_cand, int64_t *out);

/* The histogram of the pairs' insert sizes (fastq_insert_size of d_cand[i] and the two SEQ lengths, taken from the line starts):
 * d_hist[0 .. PALACE_READQC_ISIZE_MAX] is set, not added to.  A thread per pair, a histogram in LDS per workgroup.  n_pairs = 0 leaves
 * zeros.  Enqueues only. */
int palace_readqc_insert_sizes(palace_ctx *ctx, const int64_t *d_line_start1, const int64_t *d_line_start2, const int32_t *d_cand,
                               int64_t n_pairs, const palace_readqc_params *prm, uint64_t *d_hist);

/* The per-cycle counts of one text (n_records records of 4 lines, max_cycles in 0 .. PALACE_FASTQ_MAX_SEQ; bases at cycles >=
 * max_cycles are not counted).  d_out is set, not added to: one section "before" (every base of every read), and, where d_len is not
 * NULL, a second one "after" behind it (cycle c of record r iff d_len[r] >= 0 and c < d_len[r]).  A section is
 * PALACE_READQC_SECTION_WORDS(max_cycles) words of 64 bits:
 *     cnt [max_cycles][5]   the bases of slot A C G T N at the cycle
 *     qsum[max_cycles][5]   the sum of their QUAL values (byte - 33)
 *     q20, q30              QUAL bytes >= 33 + 20, >= 33 + 30
 * SEQ and QUAL are read once, 64 neighbouring bytes a wavefront; global memory is written once per thread.  Enqueues only. */
#define PALACE_READQC_SECTION_WORDS(max_cycles) (2 * PALACE_READQC_SLOTS * (int64_t)(max_cycles) + 2)
int palace_readqc_cycle_stats(palace_ctx *ctx, const uint8_t *d_text, const int64_t *d_line_start, int64_t n_records, const int32_t *d_len,
                              int32_t max_cycles, uint64_t *d_out);

#ifdef __cplusplus
}
#endif
#endif /* PALACE_HIP_H */
