/*
 * consent_amd.h -- C ABI of the MI355X window-correction engine (libconsent_amd.so).
 *
 * Drop-in boundary for CONSENT's per-window consensus operator.  Each entry point states the
 * reference interface it stands in for (paths are under the CONSENT source tree, src/):
 *
 *   cw_run / cw_run_device   <- computeConsensusReadCorrection      (correctionMSA.h:8,  correctionMSA.cpp:29-49)
 *                               computeConsensusAssemblyPolishing   (correctionMSA.h:10, correctionMSA.cpp:51-71)
 *                               i.e. MSABMAAC (call sites correctionMSA.cpp:32,54) + weightConsensus
 *                               (correctionMSA.cpp:6-27) + polishCorrection (correctionDBG.h:11)
 *                               -- batched over windows, because one window per call cannot feed a GPU.
 *   cw_poa_run / cw_poa_run_device <- only the POA of that operator (BMEAN's consensus of one segment's pieces, A4d of SURVEY), batched over
 *                               groups of sequences: for callers that have their segments -- or racon-style windows, amplicon / UMI families -- in hand.
 *   cw_sw_run / cw_sw_run_device <- StripedSmithWaterman::Aligner::Align as alignConsensus calls it (correctionAlignment.cpp:90, :110), batched over
 *                               (query, reference) pairs: the local aligner of cw_stitch_device on its own.
 *   cw_sw_path_run / cw_sw_path_run_device <- the same pairs with the alignment itself (ssw's banded traceback, its cigar) as run-length encoded ops.
 *   cw_pileup_run / cw_pileup_run_device <- the same pairs again, their paths counted into the reference's columns on the device (no counterpart: what a caller
 *                               of the above would do with every pair's cigar).
 *   cw_sw_cut_run / cw_sw_cut_run_device <- the same pairs once more, every query cut where its path crosses the reference's window boundaries (no
 *                               counterpart: alignmentWindows.cpp cuts by shifting PAF coordinates, without an alignment).
 *   cw_cut_groups_device     <- those pieces as the POA batch of every (reference, window): what stands between the aligner and cw_poa_run_device when a
 *                               reference is polished window by window.
 *   cw_strand_run / cw_strand_run_device <- which queries of such groups are the reverse complement of their reference, by shared k-mers (no counterpart
 *                               here either: the reference takes the strand from the PAF record, Overlap.h:26-58).
 *   cw_revcomp / cw_revcomp_device <- the batch with those queries reverse-complemented, for any of the runs above.
 *   cw_seed_run / cw_seed_run_device <- which queries belong to their group's reference at all, on which strand and on which diagonal, by k-mers that are
 *                               unique in the reference (no counterpart: the reference takes all three from minimap2's PAF records).
 *   cw_locate_build_device, cw_locate_run_device / cw_locate_run <- the same three for reads against a reference of any length, through one device index of
 *                               the whole reference's unique k-mers: O(read) a read, whatever the reference's length (no counterpart either).
 *   cw_overlap_count_device, cw_overlap_build_device, cw_overlap_run_device / cw_overlap_run, cw_overlap_to_pile_device <- the reads of a set that overlap
 *                               each other, through one device index of every sampled k-mer of the set (no counterpart: the reference reads minimap2's PAF).
 *   cw_sw_span_run, cw_sw_path_span_run, cw_pileup_span_run, cw_sw_cut_span_run (and _device) <- the four alignment runs with every query confined to a span
 *                               of its reference's columns, and cw_seed_spans / cw_seed_spans_device <- those spans from a seed run's rows (no counterpart:
 *                               the reference aligns a read against the window its PAF record names).
 *   cw_window_positions     <- getAlignmentWindowsPositions (alignmentWindows.cpp:27-85), host
 *   cw_extract_piles_device  <- getAlignmentWindowsSequences (alignmentWindows.cpp:87-149) evaluated on the device
 *   cw_stitch_device         <- alignConsensus + trimRead + dropRead (correctionAlignment.cpp:47-140, utils.cpp:96-128, :71-73)
 *   cw_index_reads / cw_paf_next_pile <- indexReads (utils.cpp:166-205) / getNextReadPile (alignmentPiles.cpp:22-58), host
 *   cw_pack_sequence         <- the vector<string> pile handed to those operators
 *                               (CONSENT-correction.cpp:35-37, CONSENT-polishing.cpp:46-49): 2-bit packing
 *                               with the reference's own alphabet (utils.cpp:21-32: A=00 C=01 G=10 else=11).
 *
 * Plain pointers and sizes only; the caller owns every buffer; nothing is retained past return.
 * No C++ exception crosses this boundary.  All functions return 0 on success or a negative cw_status.
 */
#ifndef CONSENT_AMD_H
#define CONSENT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum cw_status {
    CW_OK = 0,
    CW_E_INVALID = -1,   /* bad argument / malformed batch                      */
    CW_E_NO_DEVICE = -2, /* no HIP device, or the HIP runtime reported an error  */
    CW_E_NOMEM = -3,     /* device or host allocation failed                     */
    CW_E_CAPACITY = -4,  /* at least one window overflowed an output or scratch capacity: its win_status says which */
    CW_E_INTERNAL = -5
} cw_status;

/* Per-window outcome (cw_result.win_status). */
enum {
    CW_WIN_CONSENSUS = 0, /* consensus computed (correctionMSA.cpp:38-48)                        */
    CW_WIN_TEMPLATE = 1,  /* MSA empty -> raw template returned (correctionMSA.cpp:34-36)        */
    CW_WIN_OVERFLOW = 2   /* a capacity was exceeded; no output for this window                  */
};

/* The five parameters of the operator that its body actually uses (correctionMSA.cpp:29-49). */
typedef struct cw_params {
    uint32_t k;            /* merSize     -k (main.cpp:20) */
    uint32_t solid;        /* solidThresh -f (main.cpp:23) */
    uint32_t common_kmers; /* commonKMers -c (main.cpp:21) */
    uint32_t min_anchors;  /* minAnchors  -A (main.cpp:22) */
    uint32_t max_msa;      /* maxMSA      -M (main.cpp:25) */
} cw_params;

/*
 * A batch of window piles.  Sequence s of window w has global index win_first_seq[w] + s; index
 * win_first_seq[w] itself is the template (pile[0], alignmentWindows.cpp:100).
 * Bases are 2-bit codes (A=0 C=1 G=2 T=3), 16 per 32-bit word, most significant first: base j of a
 * sequence sits in word seq_word_off[s] + j/16 at bits [30-2*(j%16), 31-2*(j%16)], so that a k-mer read
 * off the words is already in str2num order.  Every sequence starts on a word boundary; unused low
 * bits of its last word are zero.
 * Sequences may SHARE words: two entries of seq_word_off may be equal (with equal lengths, one read that is a
 * member of several groups and packed once); the runs that take groups only read `bases`, and the host forms
 * check every sequence against n_words on its own.  cw_revcomp writes per sequence: give it no shared words.
 */
typedef struct cw_batch {
    uint32_t n_windows;
    uint32_t n_seqs;
    uint64_t n_words;
    const uint32_t* win_first_seq; /* [n_windows + 1] */
    const uint32_t* seq_len;       /* [n_seqs] bases  */
    const uint64_t* seq_word_off;  /* [n_seqs]        */
    const uint32_t* bases;         /* [n_words]       */
} cw_batch;

/*
 * Outputs.  Window w may write cons[cons_off[w] .. cons_off[w+1]) and solid[solid_off[w] .. solid_off[w+1]).
 * cons holds ASCII ACGT/acgt (lower case = weakly supported, correctionMSA.cpp:18-22).
 * solid holds the window's k-mers (2-bit codes, MSB-first, str2num order) whose pile-wide count is
 * >= params.solid, ascending: everything the caller's downstream code asks of merCounts
 * (correctionAlignment.cpp:6-15).  solid/solid_off/solid_len may all be NULL to skip that output.
 */
typedef struct cw_result {
    char* cons;
    const uint64_t* cons_off; /* [n_windows + 1] */
    uint32_t* cons_len;       /* [n_windows]     */
    uint8_t* win_status;      /* [n_windows]     */
    uint32_t* solid;
    const uint64_t* solid_off; /* [n_windows + 1] */
    uint32_t* solid_len;       /* [n_windows]     */
} cw_result;

typedef struct cw_engine cw_engine;

/* Library / build identification: returns a static string such as "consent_amd 0.1 gfx950". */
const char* cw_version(void);
const char* cw_strerror(int status);

/* Engine bound to one HIP device.
 *
 * Threading.  The reference calls its operator from nbThreads pool threads at once (CONSENT-correction.cpp:77, one thread per read;
 * CONSENT-polishing.cpp:37,49 one task per window), with no shared mutable state.  Here an engine owns one scratch arena and one set
 * of streams, and every entry point that takes a cw_engine* locks the engine's mutex for the time it enqueues work: calls from
 * several host threads on ONE engine are safe and are serialised; they do not run concurrently.  For concurrency use one engine per
 * host thread or per device (any number of engines may share a GPU; results do not depend on how windows are spread over engines,
 * batches or GPUs, but for the capacity stops listed at CW_MAX_BATCH_WINDOWS).  cw_run_device is asynchronous: the caller's device buffers must stay valid, and the engine's next call on
 * another stream must be ordered by the caller, until that stream has been synchronised.  The host feeders (cw_index_reads,
 * cw_paf_*) keep their state in their own handles: one thread per handle (cw_paf_open starts parser threads of its own; they end in
 * cw_paf_close, which must come before cw_read_index_free of the index it was opened with).
 * Several engines on one GPU: an engine launches on four streams of its own.  The HIP runtime maps a process's streams onto
 * GPU_MAX_HW_QUEUES hardware queues (default 4), read when the runtime starts; with more engine streams than queues one engine's
 * kernels queue behind another's long-running ones.  Set GPU_MAX_HW_QUEUES >= 4 x engines per GPU in the process environment (8 for
 * the usual two; cw_run_correction and bench.py do so themselves unless the variable is already set). */
int cw_create(const cw_params* params, int device, cw_engine** out);
void cw_destroy(cw_engine* e);

/* Templates longer than 1024 + k - 1 bases (windows beyond the wrappers' `-l 500`: the reference takes any `-l`, src/main.cpp:46-47).  The engine takes
 * templates of up to 2048 + k - 1 bases; its scratch plan provides for 1024 k-mers per template unless told otherwise -- call this once, before the
 * first run, with the longest template the engine will see (the window size): anchor blocks, segment slots and the chain kernel's work-groups are then
 * sized for it (up to twice the scratch).  A window whose template has more k-mers than the plan provides for (1024, or max_template_len - k + 1, at
 * least 128) stops with status 2, CW_WHY_TEMPLATE, in every batch -- never a wrong result, and never an outcome that depends on its neighbours.
 * CW_E_INVALID beyond 2048 + k - 1.  A caller whose windows are all SHORTER than 1024 + k - 1 bases may say so too: the plan shrinks with the number
 * (anchor blocks, segment slots, arena).  The batch limit follows the number (cw_max_batch_windows).  cw_run_correction calls it with its window size. */
int cw_configure(cw_engine* e, uint32_t max_template_len);

/* Largest batch one call accepts (per-window offsets into the engine's scratch are 32-bit); CW_E_INVALID beyond it.  Split larger
 * inputs: results do not depend on the batch composition, with the exceptions below.  cw_max_batch_windows(e) is the limit of an engine
 * under its current configuration, at most CW_MAX_BATCH_WINDOWS: 131 072 up to 1775 template k-mers (cw_configure), 115 704 at 2048;
 * cw_submit, cw_run and cw_run_device refuse a larger batch before anything is copied or launched, and so does every call whose batch has so
 * many bases that its solid table would pass 2^32 entries (16 x n_words / solidThresh).
 * What may depend on the batch.  A window's consensus and solid set never do, and neither does any outcome of a window that does not stop.
 * Three capacities of a window are slices of what the batch's plan holds: its POA tasks and members (status 2, CW_WHY_TASKS), its slice of
 * the segment arena (CW_WHY_ARENA) and the index kernel's position-matrix slot, sized from the batch's mean depth (CW_WHY_MATRIX).  Whether a
 * window stops on one of these may depend on the batch:
 *   - cw_run (and the native driver, cw_run_correction) run a batch again with a larger plan when windows stopped on them: tasks and arena
 *     x4 up to x64, the matrix slot at its full 4100 rows a sequence.  The arena's scale stays inside 32-bit offsets -- x4 for batches of up
 *     to 51 781 windows at the default plan, x2 up to 103 563 -- so a window stopped on CW_WHY_ARENA may be corrected in a small batch and stop
 *     in a large one.  A re-run is also skipped when the larger plan does not fit the device's free memory at that moment (stderr says so):
 *     then every such stop stands.
 *   - cw_run_device and cw_submit + cw_wait run a batch once: a window may stop on CW_WHY_TASKS, CW_WHY_ARENA or CW_WHY_MATRIX in one batch
 *     and be corrected in another (a deep pile among shallow windows, for one).  The caller may run such windows again in a batch of their own.
 * Every other outcome -- a stop for any other reason, a template longer than the plan (CW_WHY_TEMPLATE) and a POA task beyond the last tier's
 * capacities (CW_WHY_POA: 65 534 nodes or edges, pieces of 4 095 bases, an int32 matrix of 135.7 MB) included -- is a function of the
 * window, the parameters and the engine's cw_configure number alone. */
#define CW_MAX_BATCH_WINDOWS 131072u
uint32_t cw_max_batch_windows(cw_engine* e);

/* Host buffers in, host buffers out: H2D, kernels, D2H of the bytes the windows actually produced (not of the reserved
 * capacities), synchronous.  cw_submit + cw_wait, and then -- when windows stopped on a capacity of the batch's plan (CW_WHY_TASKS,
 * CW_WHY_ARENA, CW_WHY_MATRIX) and a larger plan would hold them -- the same batch once more with that plan (see CW_MAX_BATCH_WINDOWS). */
int cw_run(cw_engine* e, const cw_batch* batch, const cw_result* result);

/* The same in two halves, so that a caller can keep the GPU busy: cw_submit enqueues the H2D copies and the kernels of a batch and
 * returns a ticket; cw_wait blocks until that batch is done and fills `result`.  Up to two batches may be in flight per engine
 * (submit n+1, then wait n: the copies of one overlap the kernels of the other); a third cw_submit returns CW_E_INVALID.  Every
 * array named by `batch` and `result` must stay valid and untouched until cw_wait has returned.  Arrays from cw_host_alloc (pinned)
 * are moved by real DMA that overlaps the kernels; plain pageable arrays work too, the runtime then stages them itself.  The batch runs
 * once: no re-run after capacity stops (CW_MAX_BATCH_WINDOWS says which stops that leaves depending on the batch). */
int cw_submit(cw_engine* e, const cw_batch* batch, const cw_result* result, int* ticket);
int cw_wait(cw_engine* e, int ticket);

/* Pinned host memory for batches / results (hipHostMalloc). */
int cw_host_alloc(void** ptr, size_t bytes);
void cw_host_free(void* ptr);

/* Every pointer inside batch/result is a DEVICE pointer; asynchronous on `hip_stream` (a hipStream_t,
 * NULL = the engine's own stream); statuses are checked by the caller after synchronising.  The batch runs once (as cw_submit). */
int cw_run_device(cw_engine* e, const cw_batch* batch, const cw_result* result, void* hip_stream);

/* ---- only the POA: the consensus of every group of a batch of groups ------------------------------------------------------------------------
 * `groups` is a cw_batch read differently: "window" g is a GROUP, sequences win_first_seq[g] .. win_first_seq[g+1], packed as ever.  They are aligned to one
 * partial-order graph in the order given, the first non-empty one the backbone (under CW_POA_CONS_TIE, include/cw_policy.h, base ties go to it, as to a
 * segment's template piece), and the graph's consensus is the group's result: the semantics of ONE segment of the window path (include/cw_policy.h).
 * Zero-length sequences are skipped; the first params.max_msa non-empty ones are aligned; one non-empty sequence gives that sequence, none gives
 * length 0 -- both with status CW_WIN_CONSENSUS.  params.k, solid, common_kmers and min_anchors are not read.
 * `result`: cons, cons_off, cons_len and win_status are used; solid, solid_off and solid_len must be NULL (CW_E_INVALID otherwise).  Output is upper-case
 * ACGT.  Group g's slot is cons_off[g+1] - cons_off[g] bytes; CW_POA_SLOT_BYTES(longest member of the group) is what the segment path itself reserves.
 * A consensus that outgrows its slot is status 2 (CW_WHY_OUT_CONS), never a truncation, and nothing is written to that slot.
 * Stops, each a function of the group alone (status 2, CW_WHY_POA; the other groups of the batch are unaffected): a member of more than 4 095 bases, and
 * a graph beyond the last tier's capacities (CW_MAX_BATCH_WINDOWS above lists them).
 * At most cw_max_batch_windows(e) groups a call, and at most 2^32 bytes of consensus working space (32 bytes a packed word of the batch + 32 a group):
 * CW_E_INVALID beyond either, before anything is launched.  The scratch plan of such a run is exact, so the batch runs once.
 * cw_poa_run_device: every pointer inside groups / result is a DEVICE pointer; asynchronous on `hip_stream` (NULL = the engine's own stream); returns CW_OK
 * also when groups stop: the caller reads the statuses after synchronising.  Threading and stream contract: cw_run_device's.
 * cw_poa_run: host pointers, synchronous; CW_E_CAPACITY when at least one group stopped (its win_status says so; the other groups' results stand).
 * The engine keeps one scratch allocation for both kinds of run: POA runs and window runs on one engine alternate freely.  cw_last_timings names the stages
 * of such a run poa_tasks, the POA tiers' names of a window run, poa_gather. */
#define CW_POA_SLOT_BYTES(longest_member) (2u * (uint32_t)(longest_member) + 2u)
int cw_poa_run_device(cw_engine* e, const cw_batch* groups, const cw_result* result, void* hip_stream);
int cw_poa_run(cw_engine* e, const cw_batch* groups, const cw_result* result);

/* ---- only the local alignment: every sequence of a group against the group's first ---------------------------------------------------------------
 * `groups` is a cw_batch read a third way: "window" g is a GROUP, its first sequence the REFERENCE (as a window's first sequence is its template), every other
 * sequence of it a QUERY that is aligned locally against that reference by the aligner of the read re-assembly (cw_stitch_device; scores and tie rules in
 * include/cw_policy.h, CW_SSW_*: match 2, mismatch 2, a gap 3 + 1 per further base, the first best end wins).  Sequences are packed as ever.  params.* is not read.
 * `rows` holds CW_SW_ROW int32 per SEQUENCE of the batch, row s for sequence s: score, the inclusive 0-based ends of the alignment on the reference and on the
 * query, the totals of inserted (query-only) and deleted (reference-only) bases between them, a status.  Nothing aligns (or the query or the reference is
 * empty): score 0, begins 0, ends -1, status CW_SW_ALIGNED.  The reference's own row: the same numbers with status CW_SW_IS_REF.  A group of one sequence or
 * of none is valid.
 * Indel totals are computed only under CW_SW_WANT_INDELS (0 otherwise): a banded traceback between the ends, serial in parts.  Its band starts at
 * |reference span - query span| + 1 and doubles until the banded score reaches the alignment's; a band of b over a reference span of R and a query span of Q
 * bases needs 3 x min(2b + 1, R + 1) x Q direction bytes -- and 12 x min(2b + 3, R + 3) more, rounded up to 16, once those exceed 4096 (b > 169) -- in the
 * wave's scratch of CW_SW_DIR_BYTES.  A pair whose band outgrows that keeps its five alignment numbers, ins = del = 0, and gets status CW_SW_NO_INDELS: a
 * function of the pair alone, never a wrong number.
 * Capacities, each a function of the pair alone (status CW_SW_STOP, numbers as when nothing aligns; the other pairs are unaffected): a query of more than
 * CW_SW_QMAX bases, a reference of more than CW_SW_RMAX -- a score is at most twice the shorter of the two and, like a reference column, lives in a signed
 * 16-bit field of the sweeps.
 * At most cw_max_batch_windows(e) groups a call; CW_E_INVALID beyond that, for flags other than CW_SW_WANT_INDELS and for NULL arguments, before anything
 * is launched.  The scratch plan of such a run is exact: the batch runs once.
 * cw_sw_run_device: every pointer inside groups, and rows, is a DEVICE pointer; asynchronous on `hip_stream` (NULL = the engine's own stream); CW_OK also
 * when pairs stop.  Threading and stream contract: cw_run_device's.
 * cw_sw_run: host pointers, synchronous; CW_E_CAPACITY when at least one row has CW_SW_STOP (the other rows stand).  CW_SW_NO_INDELS is not an error.
 * One engine alternates window runs, POA runs and alignment runs freely (one scratch allocation for all).  cw_last_timings names the stages of such a run
 * sw_order, sw_align (queries of up to 640 bases), sw_align_wide (up to 2 048), sw_align_long (beyond). */
enum { CW_SW_SCORE, CW_SW_REF_BEGIN, CW_SW_REF_END, CW_SW_QUERY_BEGIN, CW_SW_QUERY_END, CW_SW_INS, CW_SW_DEL, CW_SW_STATUS, CW_SW_ROW = 8 };
enum { CW_SW_ALIGNED = 0, CW_SW_NO_INDELS = 1, CW_SW_STOP = 2, CW_SW_IS_REF = 3 };
#define CW_SW_WANT_INDELS 1u
#define CW_SW_QMAX 32768      /* longest query    */
#define CW_SW_RMAX 16383      /* longest reference */
#define CW_SW_DIR_BYTES (1u << 20) /* banded traceback scratch per wave: the re-assembly's */
int cw_sw_run_device(cw_engine* e, const cw_batch* groups, int32_t* rows /* [n_seqs * CW_SW_ROW] */, uint32_t flags, void* hip_stream);
int cw_sw_run(cw_engine* e, const cw_batch* groups, int32_t* rows, uint32_t flags);

/* ---- the alignment itself: cw_sw_path_run ---------------------------------------------------------------------------------------------------------------
 * `groups` and `rows` as for cw_sw_run; on top of the row, every pair's alignment path as BAM-style ops, `length << 4 | op`: 0 = M, 1 = I (a query base only),
 * 2 = D (a reference base only); under CW_SW_PATH_EQX -- the only flag -- 7 ('=') and 8 ('X') replace 0.  Sequence s may write ops[ops_off[s] .. ops_off[s+1]);
 * n_ops[s] is what it wrote.  Ops come in alignment order (begin to end), run-length encoded: no two neighbouring ops have the same code.  Whenever a path is
 * reported, the lengths of its M (= and X) and I ops add up to the query span and those of its M and D ops to the reference span of the row.
 * The row holds the five alignment numbers of cw_sw_run bit for bit; CW_SW_INS / CW_SW_DEL are always computed: the totals of the path's I and D ops.
 * The path is the one ssw's banded traceback walks between the ends: the band starts at |reference span - query span| + 1 and doubles until the banded score
 * reaches the alignment's (or the band passes both spans together); the walk runs back from the end cell and is closed as ssw closes it: it stops at query row 0,
 * whose cell is one more M.
 * Statuses (none of them but CW_SW_STOP an error; each a function of the pair alone, and of its slot for CW_SW_PATH_SLOT):
 *   CW_SW_ALIGNED    the path is written, n_ops its length (0 when nothing aligns).
 *   CW_SW_NO_PATH    a band of b over a reference span of R and a query span of Q bases needs min(2b + 1, R + 1) x Q direction bytes, one a cell -- and
 *                    12 x min(2b + 3, R + 3) more, rounded up to 16, once those exceed 4096 (b > 169 and R > 338) -- in the wave's scratch of CW_SW_PATH_BYTES;
 *                    the first band that does not fit ends the pair: the five numbers stand, ins = del = 0, n_ops = 0.
 *   CW_SW_PATH_OPEN  the walk did not close at the begin cell (it left the band or the reference before query row 0, or reached that row at another column than
 *                    the first): ins / del are what the walk counted until then, n_ops = 0 -- never a path that does not span the ends.
 *   CW_SW_PATH_SLOT  the ops outgrow the caller's slot: the seven numbers stand, n_ops is the number needed, nothing is written to the slot.
 *                    CW_SW_OPS_BOUND(query length, reference length) ops always do.
 *   CW_SW_IS_REF, CW_SW_STOP and the rows of empty queries or references: as in cw_sw_run, n_ops = 0.
 * CW_E_INVALID for any other flag, NULL arguments (rows, paths and its members) and more than cw_max_batch_windows(e) groups, before anything is launched.  The
 * scratch plan is exact: the batch runs once.
 * cw_sw_path_run_device: every pointer inside groups and paths, and rows, is a DEVICE pointer; asynchronous on `hip_stream` (NULL = the engine's own); CW_OK
 * also when pairs stop.  cw_sw_path_run: host pointers, synchronous, ops_off ascending from any start; CW_E_CAPACITY only when a row has CW_SW_STOP.
 * Such runs alternate freely with window, POA and cw_sw_run runs on one engine.  cw_last_timings names the stages sw_order, sw_path (queries of up to 640
 * bases), sw_path_wide (up to 2 048), sw_path_long (beyond). */
typedef struct cw_sw_paths {
    uint32_t* ops;            /* BAM-style: length << 4 | op */
    const uint64_t* ops_off;  /* [n_seqs + 1]: sequence s may write ops[ops_off[s] .. ops_off[s+1]) */
    uint32_t* n_ops;          /* [n_seqs] */
} cw_sw_paths;
enum { CW_SW_NO_PATH = 4, CW_SW_PATH_OPEN = 5, CW_SW_PATH_SLOT = 6 }; /* row statuses only these entry points write */
enum { CW_SW_OP_M = 0, CW_SW_OP_I = 1, CW_SW_OP_D = 2, CW_SW_OP_EQ = 7, CW_SW_OP_X = 8 };
#define CW_SW_PATH_EQX 4u
#define CW_SW_OPS_BOUND(query_len, ref_len) ((query_len) + (ref_len))  /* every run consumes a base of one of them */
#define CW_SW_PATH_BYTES (2u << 20)   /* direction bytes per wave of the path run */
int cw_sw_path_run_device(cw_engine* e, const cw_batch* groups, int32_t* rows, const cw_sw_paths* paths, uint32_t flags, void* hip_stream);
int cw_sw_path_run(cw_engine* e, const cw_batch* groups, int32_t* rows, const cw_sw_paths* paths, uint32_t flags);

/* ---- what the alignments say about the reference: cw_pileup_run ---------------------------------------------------------------------------------------------
 * `groups` and `rows` as for cw_sw_path_run; in place of every pair's ops, CW_PILE_COL counts per reference column, summed over the group's queries on the
 * device: how many queries put an A, C, G or T on the column, how many skip it, how many insert something after it, how many alignments begin and end on it.
 * The layout is per SEQUENCE, as ops_off is: sequence s, where it is its group's reference, owns columns col_off[s] .. col_off[s+1]; column j of reference r
 * -- j counts the whole reference from 0, not the aligned span -- is the CW_PILE_COL words at counts[(col_off[r] + j) * CW_PILE_COL].  A query's own slot is never
 * read or written and may be empty.
 * Which pairs count: those cw_sw_path_run reports CW_SW_ALIGNED with a positive score -- the pairs with a closed path.  Walking such a path in alignment order,
 * i the query index and j the reference column, both absolute:
 *   an M step                   counts[j][code of query base i] += 1 (codes 0..3 as packed: CW_PILE_A .. CW_PILE_T; a non-ACGT letter packs as T, as everywhere)
 *   a D step                    counts[j][CW_PILE_DEL] += 1
 *   the first step of an I run  counts[j - 1][CW_PILE_INS] += 1, j - 1 the last reference column consumed before the run: the column counts insertion events,
 *                               not inserted bases (a path never begins with an insertion -- the walk closes with an M -- so j - 1 >= ref_begin)
 *   once per pair               counts[ref_begin][CW_PILE_BEGIN] += 1 and counts[ref_end][CW_PILE_END] += 1
 * so that per column A + C + G + T + DEL is the number of counted alignments that cover it.  The counts are integer sums: they depend on no batch
 * composition, order or run.
 * Clearing: without CW_PILE_ACCUMULATE -- the only flag -- the run first zeroes columns 0 .. ref_len - 1 of every reference whose slot holds them; nothing
 * beyond ref_len in a slot is touched, and nothing in a query's slot.  Under the flag nothing is cleared and the run adds to what is there: a reference whose
 * queries do not fit one call can be split over calls.
 * The row: the five alignment numbers and ins / del are cw_sw_path_run's, bit for bit.  Statuses: CW_SW_ALIGNED, CW_SW_NO_PATH, CW_SW_PATH_OPEN, CW_SW_IS_REF and
 * CW_SW_STOP as there -- all but a positive-score CW_SW_ALIGNED count nothing -- and
 *   CW_SW_PILE_SLOT  the reference's slot (col_off[r+1] - col_off[r]) is shorter than the reference: every pair of that group that would have counted
 *                    keeps its seven numbers and has this status; nothing of that slot is cleared or counted; other groups are unaffected.
 * There are no op slots: CW_SW_PATH_SLOT does not occur.
 * CW_E_INVALID, before anything is launched: any flag other than CW_PILE_ACCUMULATE, NULL rows / pile / counts / col_off, more than cw_max_batch_windows(e)
 * groups.  The scratch plan is cw_sw_path_run's without op memory, exact: the batch runs once.
 * cw_pileup_run_device: every pointer inside groups and pile, and rows, is a DEVICE pointer, counts 16-byte aligned (CW_E_INVALID otherwise); asynchronous on
 * `hip_stream` (NULL = the engine's own); CW_OK also when pairs stop.  cw_pileup_run: host pointers, synchronous, col_off ascending from any start, no
 * alignment asked of counts; the caller's counts go up only under the flag, and of the slots only columns 0 .. ref_len - 1 of the references that hold them
 * come back; CW_E_CAPACITY only when a row has CW_SW_STOP.
 * Such runs alternate freely with every other kind of run on one engine.  cw_last_timings names the stages sw_order, pile_clear (absent under the flag), pile
 * (queries of up to 640 bases), pile_wide (up to 2 048), pile_long (beyond). */
enum { CW_PILE_A, CW_PILE_C, CW_PILE_G, CW_PILE_T, CW_PILE_DEL, CW_PILE_INS, CW_PILE_BEGIN, CW_PILE_END, CW_PILE_COL = 8 };
typedef struct cw_pileup {
    uint32_t* counts;         /* CW_PILE_COL uint32 per column */
    const uint64_t* col_off;  /* [n_seqs + 1]: sequence s, where it is its group's reference, owns columns col_off[s] .. col_off[s+1] */
} cw_pileup;
enum { CW_SW_PILE_SLOT = 7 };     /* row status only these entry points write */
#define CW_PILE_ACCUMULATE 8u     /* the only flag */
int cw_pileup_run_device(cw_engine* e, const cw_batch* groups, int32_t* rows, const cw_pileup* pile, uint32_t flags, void* hip_stream);
int cw_pileup_run(cw_engine* e, const cw_batch* groups, int32_t* rows, const cw_pileup* pile, uint32_t flags);

/* ---- where the queries cross the reference's windows: cw_sw_cut_run ------------------------------------------------------------------------------------------
 * `groups` and `rows` as for cw_sw_path_run; in place of every pair's ops, the query's cut points at the reference's window boundaries.  A reference of n
 * columns has T = ceil(n / W) windows of W = cuts->window columns (the last one shorter when W does not divide n); the layout is per SEQUENCE, as ops_off is:
 * sequence s, where it is a query, owns cuts[cut_off[s] .. cut_off[s+1]) and writes words t = 0 .. T of it -- CW_SW_CUTS(reference length, W) words.
 * A pair that counts is cw_pileup_run's: one cw_sw_path_run reports CW_SW_ALIGNED with a positive score.  With every position absolute:
 *   cuts[t] = query_begin       where t x W <= ref_begin
 *   cuts[t] = query_end + 1     where t x W >  ref_end
 *   otherwise                   the number of query bases the path has consumed when it takes the step (an M or a D) that consumes column t x W -- counted
 *                               from the query's first base, so a position in the query.  An insertion run between columns t x W - 1 and t x W therefore
 *                               belongs to window t - 1: the side on which cw_pileup_run counts its INS event.  A deletion that covers column t x W cuts at
 *                               the query base that follows it.
 * cuts is non-decreasing, cuts[0] = query_begin and cuts[T] = query_end + 1.  Piece t of the query is query[cuts[t], cuts[t+1]): what the alignment puts on
 * window t; the pieces concatenate to the aligned query span.  The words are functions of the pair alone: they depend on no batch composition, order or run.
 * Every other pair -- score 0, CW_SW_NO_PATH, CW_SW_PATH_OPEN, CW_SW_STOP, an empty query or reference -- gets T + 1 zeros: all its pieces are empty.
 * The row is cw_sw_path_run's bit for bit, ins / del included, but for
 *   CW_SW_CUT_SLOT   the slot is shorter than T + 1 words: a pair that would have counted keeps its seven numbers and has this status, and nothing is
 *                    written to the slot.  A pair that does not count writes nothing to a short slot either and keeps its status.
 * Never touched: the words of a slot beyond T + 1, a reference's own slot (it may be empty), anything outside the slots.
 * CW_E_INVALID, before anything is launched: window == 0, NULL rows / cuts / cuts->cuts / cuts->cut_off, more than cw_max_batch_windows(e) groups.
 * n_seqs == 0 is CW_OK.  The scratch plan is cw_sw_path_run's without op memory, exact, as for the pileup run: the batch runs once.
 * cw_sw_cut_run_device: every pointer inside groups and cuts, and rows, is a DEVICE pointer; asynchronous on `hip_stream` (NULL = the engine's own); CW_OK
 * also when pairs stop.  cw_sw_cut_run: host pointers, synchronous, cut_off ascending from any start; of the slots only the T + 1 words of the query slots
 * that hold them come back; CW_E_CAPACITY only when a row has CW_SW_STOP.
 * Such runs alternate freely with every other kind of run on one engine.  cw_last_timings names the stages sw_order, cut (queries of up to 640 bases),
 * cut_wide (up to 2 048), cut_long (beyond). */
typedef struct cw_sw_cuts {
    uint32_t* cuts;           /* query positions */
    const uint64_t* cut_off;  /* [n_seqs + 1]: sequence s, where it is a query, owns cuts[cut_off[s] .. cut_off[s+1]) */
    uint32_t window;          /* W >= 1 reference columns a window */
} cw_sw_cuts;
/* words a query's slot needs: the windows of its reference + 1; no 32-bit overflow for any W */
#define CW_SW_CUTS(ref_len, window) ((ref_len) / (window) + ((ref_len) % (window) != 0u) + 1u)
enum { CW_SW_CUT_SLOT = 8 };      /* row status only these entry points write */
int cw_sw_cut_run_device(cw_engine* e, const cw_batch* groups, int32_t* rows, const cw_sw_cuts* cuts, void* hip_stream);
int cw_sw_cut_run(cw_engine* e, const cw_batch* groups, int32_t* rows, const cw_sw_cuts* cuts);

/* The POA batch behind a cut run, built on the device: one output group per (reference, window).  `groups`, `rows` and `cuts` are what cw_sw_cut_run_device
 * took and wrote, all DEVICE pointers, and so are grp_first[groups->n_windows + 1] and the four output arrays laid out as cw_batch (win_first_seq[group_cap + 1],
 * seq_len[seq_cap], seq_word_off[seq_cap], bases[word_cap]).  Input group g with a non-empty reference of T windows gives output groups grp_first[g] + t,
 * t = 0 .. T - 1, input groups in order; a group of none or with an empty reference gives none (grp_first[g + 1] = grp_first[g]).
 *   first sequence of (g, t)   reference columns [t x W, min((t + 1) x W, n))
 *   members, in query order    piece t of every query of g whose row is CW_SW_ALIGNED with a positive score, whose alignment spans the window --
 *                              ref_begin <= t x W and ref_end >= min((t + 1) x W, n) - 1 -- and whose piece is not empty
 * A piece that covers part of a window is no member: it would be aligned end to end against whole-window members (DESIGN.md 4.8 has the figures).  The output
 * is a valid cw_batch: every sequence starts on a word boundary, the unused low bits of its last word are zero.
 * *n_groups / *n_seqs / *n_words (HOST pointers) hold the totals on return; the call synchronises once to read them.  CW_E_CAPACITY when they exceed the
 * capacities, and nothing of the output is then valid: call again with larger arrays (capacities 0 just size the batch; the arrays may then be NULL).
 * CW_E_INVALID for NULL groups / rows / cuts or totals, window == 0, more than cw_max_batch_windows(e) input groups. */
int cw_cut_groups_device(cw_engine* e, const cw_batch* groups, const int32_t* rows, const cw_sw_cuts* cuts,
                         uint32_t* grp_first /* [groups->n_windows + 1] */,
                         uint32_t* win_first_seq, uint32_t* seq_len, uint64_t* seq_word_off, uint32_t* bases,
                         uint32_t group_cap, uint32_t seq_cap, uint64_t word_cap,
                         uint32_t* n_groups, uint32_t* n_seqs, uint64_t* n_words, void* hip_stream);

/* ---- both strands for the alignment operators: cw_strand_run, cw_revcomp ----------------------------------------------------------------------------------------
 * The runs above align a query as it is given.  In a long-read set half the reads are the reverse complement of their reference; these two orient a batch of
 * groups on the device: a strand vote per (query, reference) pair -- shared k-mers in both orientations, O(m + n) a pair where the aligner costs O(m n) -- and a
 * reverse complement over the packed layout, which writes the oriented batch.  Reverse complement keeps every length: the oriented batch shares win_first_seq,
 * seq_len and seq_word_off with the input, only `bases` is new, and every run above takes it unchanged.
 *
 * cw_strand_run.  `groups` is read as in cw_sw_run: the first sequence of a group is its reference, the others are queries; params.* is not read.  With k =
 * out->k (0 = CW_STRAND_K), K the SET of the reference's k-mers (2-bit codes, first base most significant; a non-ACGT letter is already packed as T), m the
 * query's length:
 *   hits[2s]     the query positions i in 0 .. m - k whose k-mer is in K: positions count with multiplicity, K is a set
 *   hits[2s+1]   those whose k-mer's reverse complement is in K -- the forward hits of the reverse-complemented query
 *   strand[s]    CW_STRAND_REV when reverse hits > forward hits, else CW_STRAND_FWD: ties go forward, both zero included
 *   CW_STRAND_IS_REF, hits 0, 0   the reference's own entry
 *   CW_STRAND_NONE, hits 0, 0     no vote is possible: the query or the reference is shorter than k (empty included), the query longer than CW_SW_QMAX or the
 *                                 reference longer than CW_SW_RMAX -- the aligner's own capacities; there is no CW_E_CAPACITY from this run: the alignment run
 *                                 that follows reports those pairs
 * Membership is exact (the table holds the k-mers themselves and compares them), and every number is a function of the pair and k alone: it depends on no batch
 * composition, order or run.  hits may be NULL.
 * CW_E_INVALID, before anything is launched: NULL groups / out / out->strand, k other than 0 or CW_STRAND_KMIN .. CW_STRAND_KMAX, more than
 * cw_max_batch_windows(e) groups.  n_seqs == 0 is CW_OK.  The scratch plan is exact (two counters and a word a group): the batch runs once.
 * cw_strand_run_device: every pointer inside groups and out is a DEVICE pointer; asynchronous on `hip_stream` (NULL = the engine's own), under cw_run_device's
 * threading and stream contract.  cw_strand_run: host pointers, synchronous.
 * Such runs alternate freely with every other kind of run on one engine.  cw_last_timings names the stages strand_order (the units of work: a group's queries in
 * chunks, so that one group of very many queries spreads over the device), strand (references of up to 2 048 bases), strand_wide (beyond).
 *
 * cw_revcomp.  For every sequence s of the batch the words bases_out[seq_word_off[s] .. + ceil(len / 16)) are written:
 *   strand[s] == CW_STRAND_REV   out base j = 3 - in base (len - 1 - j), the unused low bits of the last word zero
 *   any other value              the words are copied
 * strand == NULL: every sequence is reversed.  A flagged reference is reversed too (cw_strand_run never flags one).  Words of bases_out that belong to no
 * sequence are never written.  bases_out must not be groups->bases: CW_E_INVALID when the two pointers are equal; any other overlap of bases_out with the
 * batch's arrays is the caller's responsibility (a sequence's words are read while another's are written).  CW_E_INVALID also for NULL groups or bases_out, more
 * than cw_max_batch_windows(e) groups; n_seqs == 0 is CW_OK.  cw_revcomp_device: device pointers (strand too), asynchronous on `hip_stream`, the contract above;
 * it uses no scratch.  cw_revcomp: host pointers, synchronous.  cw_last_timings names the one stage revcomp.
 * Coordinates in rows, CIGARs, pileups and cuts computed from an oriented batch are the ORIENTED query's: position i there is position len - 1 - i of the
 * original query. */
enum { CW_STRAND_FWD = 0, CW_STRAND_REV = 1, CW_STRAND_IS_REF = 2, CW_STRAND_NONE = 3 }; /* strand[] values */
#define CW_STRAND_K    11u   /* k used when cw_strands.k == 0 */
#define CW_STRAND_KMIN 8u
#define CW_STRAND_KMAX 15u   /* a k-mer is < 2^30: one 32-bit key with a free "empty" value */
typedef struct cw_strands {
    uint8_t*  strand;   /* [n_seqs] */
    uint32_t* hits;     /* [n_seqs * 2]: forward hits, reverse hits; may be NULL */
    uint32_t  k;        /* 0 = CW_STRAND_K, else CW_STRAND_KMIN..CW_STRAND_KMAX */
} cw_strands;
int cw_strand_run_device(cw_engine* e, const cw_batch* groups, const cw_strands* out, void* hip_stream);
int cw_strand_run(cw_engine* e, const cw_batch* groups, const cw_strands* out);
int cw_revcomp_device(cw_engine* e, const cw_batch* groups, const uint8_t* strand, uint32_t* bases_out, void* hip_stream);
int cw_revcomp(cw_engine* e, const cw_batch* groups, const uint8_t* strand, uint32_t* bases_out);

/* ---- reads placed on a reference by unique shared k-mers: cw_seed_run ---------------------------------------------------------------------------------------------
 * Every run above starts from groups: somebody knew which reads belong to which reference.  This one answers that per (query, reference) pair in the strand
 * vote's O(m + n): does the query belong here, on which strand, on which diagonal.  The vote's pass with the place of every hit kept.
 *
 * `groups` is read as in cw_sw_run; params.* is not read.  With k = out->k (0 = CW_STRAND_K), n the reference's length and m the query's:
 *   U        the k-mers that occur at exactly ONE position of the reference, P(K) that position.  A k-mer that occurs twice or more seeds nothing: repeats and
 *            homopolymer runs do not vote.
 *   q_0, q_1 the query as given and its reverse complement
 *   c_o[b]   the positions i in 0 .. m - k of q_o whose k-mer K is in U and whose diagonal d = P(K) - i has the bin b = (d + m) >> CW_SEED_SHIFT (d + m >= k > 0);
 *            bins run 0 .. B - 1 with B = ((n + m) >> CW_SEED_SHIFT) + 1, and c_o[B] = 0
 *   w_o[b]   c_o[b] + c_o[b + 1]: a window of two neighbouring bins, 128 diagonals
 * The best (o, b) maximises w; ties go forward before reverse, then to the lowest b.  Sequence s owns rows[CW_SEED_ROW s ..):
 *   CW_SEED_STATUS   CW_STRAND_FWD or CW_STRAND_REV, the best orientation
 *   CW_SEED_HITS     its w
 *   CW_SEED_DIAG     (b << CW_SEED_SHIFT) - m: the lowest of the window's 128 diagonals.  Negative where the read overhangs the reference's start.  It is the
 *                    DENSEST window, not the read's start: a long read's diagonal drifts by its net indels, and the window holds the most of it
 *   CW_SEED_OTHER    the best w of the other orientation
 *   no hit at all    CW_STRAND_FWD, 0, -m, 0
 *   CW_STRAND_IS_REF, 0, 0, 0   the reference's own row
 *   CW_STRAND_NONE, 0, 0, 0     no vote is possible, as in cw_strand_run: the query or the reference shorter than k, the query longer than CW_SW_QMAX, the
 *                               reference longer than CW_SW_RMAX; never CW_E_CAPACITY
 * strand[s], when given, is the row's status byte: what cw_revcomp takes.  Membership is exact and every number is a function of the pair and k alone.
 * CW_E_INVALID, before anything is launched: NULL groups / out / out->rows, k other than 0 or CW_STRAND_KMIN .. CW_STRAND_KMAX, more than
 * cw_max_batch_windows(e) groups.  n_seqs == 0 is CW_OK.  The scratch plan is the strand run's; the batch runs once.
 * cw_seed_run_device: device pointers, asynchronous on `hip_stream`, cw_strand_run_device's contract.  cw_seed_run: host pointers, synchronous.
 * cw_last_timings names the stages strand_order, seed (references of up to 2 048 bases), seed_wide (beyond).
 * Several groups may hold the same queries: see cw_batch on shared words.  That is how a reference longer than CW_SW_RMAX is searched -- a group per tile of
 * it, every group the tile and all reads -- at the cost of tiles x reads votes; cw_locate_run_device below looks every read up in one index instead. */
enum { CW_SEED_STATUS, CW_SEED_HITS, CW_SEED_DIAG, CW_SEED_OTHER, CW_SEED_ROW = 4 };
#define CW_SEED_SHIFT 6u    /* a bin is 64 diagonals; a window is two neighbouring bins */
typedef struct cw_seeds {
    int32_t* rows;     /* [n_seqs * CW_SEED_ROW] */
    uint8_t* strand;   /* [n_seqs] or NULL: CW_STRAND_* values, what cw_revcomp takes */
    uint32_t k;        /* 0 = CW_STRAND_K, else CW_STRAND_KMIN .. CW_STRAND_KMAX */
} cw_seeds;
int cw_seed_run_device(cw_engine* e, const cw_batch* groups, const cw_seeds* out, void* hip_stream);
int cw_seed_run(cw_engine* e, const cw_batch* groups, const cw_seeds* out);

/* ---- reads placed through a device k-mer index of the whole reference: cw_locate_* ---------------------------------------------------------------------------------
 * cw_seed_run's row with its reference allowed any length.  The seed run rebuilds an LDS table per (reference, chunk of queries) and stops at CW_SW_RMAX bases; a
 * longer reference is searched there by tiles, at tiles x reads votes.  Here the reference's unique k-mers go into ONE table in device memory, built once, and a
 * read is looked up in it: O(m) a read, and the reference's length stops mattering.
 *
 * With n = ref->len (0 .. CW_LOCATE_RMAX), m the read's length and k = ref->k (0 = CW_LOCATE_K; else CW_STRAND_KMIN .. CW_STRAND_KMAX -- 15 because 4^11 k-mers
 * are fewer than the positions of a 4.6 Mbp contig: at the strand vote's 11 about a third of such a contig's k-mers are unique, at 15 nearly all):
 *   U        the k-mers that occur at exactly ONE position of the WHOLE reference, P(K) that position
 *   q_0, q_1 the read as given and its reverse complement
 *   c_o[b]   the positions i in 0 .. m - k of q_o whose k-mer K is in U, counted by the bin b = (P(K) - i + m) >> CW_SEED_SHIFT; bins run 0 .. B - 1 with
 *            B = ((n + m) >> CW_SEED_SHIFT) + 1, and c_o[B] = 0
 *   w_o[b]   c_o[b] + c_o[b + 1]
 * Per orientation the best b maximises w, ties to the lowest b.  Sequence s of `reads` owns rows[CW_SEED_ROW s ..):
 *   CW_SEED_STATUS   CW_STRAND_REV only when w_1's best is LARGER than w_0's, otherwise CW_STRAND_FWD
 *   CW_SEED_HITS     the chosen w
 *   CW_SEED_DIAG     (b << CW_SEED_SHIFT) - m; it fits an int32 because n + m < 2^31
 *   CW_SEED_OTHER    the other orientation's best w
 *   no hit at all    CW_STRAND_FWD, 0, -m, 0
 *   CW_STRAND_NONE, 0, 0, 0     m < k, m > CW_SW_QMAX or n < k; never CW_E_CAPACITY
 * There is no reference row: every sequence of `reads` is a read, and its grouping (n_windows, win_first_seq) is not read.  strand[s], when given, is the status
 * byte.  Every number is a function of (reference, read, k) alone: batch composition, read order, run, and which of the kernels' two routes a read took do not
 * change it.  For n <= CW_SW_RMAX a read's row is bit for bit cw_seed_run's row of that read in a group behind that reference.
 * This is NOT the answer of a tiled seed run (Engine.place): there a k-mer is unique when it is unique in its TILE, here when it is unique in the whole reference.
 * A stretch present twice, 40 000 bases apart, seeds nothing here and seeds in both tiles there.  Neither is changed to match the other.
 *
 * The table is the caller's, cw_locate_table_words(len) words: a power of two, at least twice the reference's positions and at least 1 024; 0 beyond
 * CW_LOCATE_RMAX.  cw_locate_build_device clears it and fills it -- one piece of memory serves one reference after another -- and any number of
 * cw_locate_run_device calls follow.  Its content is private and may differ from build to build (the order of insertion is a race); the rows never do.
 * `bases` is the reference packed as a cw_batch sequence from word 0.
 * CW_E_INVALID, before anything is allocated or launched: NULL ref, bases (while len > 0), table, reads, out or out->rows; NULL seq_len, seq_word_off or bases
 * of reads while n_seqs > 0; len > CW_LOCATE_RMAX; k outside its range; out->k neither 0 nor the reference's k.  n_seqs == 0 is CW_OK.
 * The device forms: device pointers, asynchronous on `hip_stream`, cw_strand_run_device's threading and stream contract.  cw_locate_run: host pointers,
 * synchronous; it uploads the reference and the reads, builds into device memory of the engine's own (CW_E_NOMEM when it cannot have it), runs, and brings the
 * rows and bytes back.  Locate runs share the engine's one scratch allocation and alternate freely with every other run; the scratch plan is exact, the batch
 * runs once.  cw_last_timings names the stages locate_build (the build), locate and locate_dense (a run: the reads whose votes fit a work-group's LDS, and the
 * few that do not). */
#define CW_LOCATE_K 15u                        /* k used when cw_locate_ref.k == 0 */
#define CW_LOCATE_RMAX ((1u << 28) - 1u)       /* longest reference: a position takes 28 bits of a slot */
typedef struct cw_locate_ref {
    const uint32_t* bases;  /* the reference, packed as a cw_batch sequence from word 0 */
    uint64_t len;
    uint32_t* table;        /* [cw_locate_table_words(len)], the caller's */
    uint32_t k;             /* 0 = CW_LOCATE_K, else CW_STRAND_KMIN .. CW_STRAND_KMAX */
} cw_locate_ref;
uint64_t cw_locate_table_words(uint64_t ref_len);
int cw_locate_build_device(cw_engine* e, const cw_locate_ref* ref, void* hip_stream);
int cw_locate_run_device(cw_engine* e, const cw_locate_ref* ref, const cw_batch* reads, const cw_seeds* out, void* hip_stream);
int cw_locate_run(cw_engine* e, const uint32_t* ref_bases, uint64_t ref_len, uint32_t k, const cw_batch* reads, const cw_seeds* out);

/* ---- the reads of a set that overlap each other: cw_overlap_* -------------------------------------------------------------------------------------------------------
 * What the window runs and cw_run_correction take from minimap2's PAF file, found on the device: per read the reads that share enough sampled k-mers with it on one
 * diagonal, with strand, diagonal and PAF-style coordinates.  The locate index keeps a k-mer that is unique in ONE reference; a read set at depth d holds every
 * k-mer d times, so this index keeps EVERY occurrence.  `reads` is a cw_batch whose grouping (n_windows, win_first_seq) is not read; its bases end in one spare
 * word, as everywhere.
 *
 * The function, with prm = {k, sample, max_occ, min_hits} (k: 0 = CW_OVL_K, else CW_STRAND_KMIN .. CW_STRAND_KMAX; sample 0 .. 8, 0 = every k-mer, CW_OVL_SAMPLE
 * the named default; max_occ: 0 = CW_OVL_MAX_OCC, at most 65 535; min_hits >= 1, CW_OVL_MIN_HITS the measured default):
 *   occurrences  position i of read r (0 <= i <= len - k), K the k-mer there, R its reverse complement.  K == R (even k only): skipped.  c = min(K, R), the
 *                occurrence's strand s = (K > R).  Sampled when sample == 0 or ((c * 0x9E3779B1) mod 2^32) >> (32 - sample) == 0.  The index holds (c, r, i, s)
 *                of every sampled position of every read with k <= len <= CW_SW_QMAX; other reads contribute nothing.  occ(c) = the entries of c.
 *   votes        of query q (m bases): every sampled occurrence (c, i, sq) of q with occ(c) <= max_occ, against every entry (c, t, p, st) with t != q (read
 *                INDICES: a second copy of a sequence is a target).  o = sq ^ st; the bin b = (p - i + m) >> CW_SEED_SHIFT for o = 0, (p + k + i) >>
 *                CW_SEED_SHIFT for o = 1 -- cw_locate_run's arithmetic with t as the reference.  c[t, o, b] counts them, w[t, o, b] = c[t, o, b] + c[t, o, b + 1];
 *                per (t, o) the best b maximises w, ties to the lowest b.  A candidate is a (t, o) whose best w >= min_hits; both orientations of a target may be.
 *   rows         the candidates by hits descending, then t, then o ascending, CW_OVL_ROW int32 each: TARGET, STRAND (CW_STRAND_FWD / CW_STRAND_REV), HITS,
 *                DIAG = (b << 6) - m, then with n the target's length c0 = clamp(DIAG + 64, -(m - k), n - k), a = max(0, -c0), z = min(m, n - c0):
 *                T_START = a + c0, T_END = z + c0 - 1; forward Q_START = a, Q_END = z - 1; reverse Q_START = m - z, Q_END = m - 1 - a.  Ends INCLUSIVE, query
 *                coordinates on the query as given: cw_overlap's convention.  These are the dovetail the window's middle diagonal implies, not aligned ends: on
 *                the planted set of tests/test_overlap_cpu.py (10 - 12 % errors) an end lies up to CW_OVL_END_SLACK bases from the true overlap's end.
 *   per query    n_rows[j] the candidates, status[j]: CW_OVL_OK; CW_OVL_NONE (m < k or m > CW_SW_QMAX: 0 rows, never an error); CW_OVL_SLOT (the candidates
 *                outgrow the slot row_off[j + 1] - row_off[j], counted in ROWS: n_rows is the number needed, nothing is written, never a truncation);
 *                CW_OVL_DENSE (the query's distinct (t, o, b) keys pass 131 072, the scratch table's capacity: 0 rows); CW_OVL_BAD_INDEX (the memory was
 *                built with an n_entries that is not the read set's count: 0 rows).  Words of a slot beyond the rows written are never touched.
 * Every number is a function of (read set, prm, query) alone: not of how the queries are batched, their order, the run, or the kernels' route.
 *
 * cw_overlap_count_device: *n_entries (a HOST pointer) = the sampled occurrences; it synchronises once.  cw_overlap_index_words(n_entries): the index's size in
 * 32-bit words (0 beyond the limits).  cw_overlap_build_device: clears and fills index->mem (8-byte aligned, the caller's device memory; one piece serves one read
 * set after another); index->n_entries is what the count gave.  Its content is private and may differ from build to build; the rows never do.
 * cw_overlap_run_device: the queries are reads first_query .. first_query + n_queries - 1 of the indexed set, j = q - first_query indexes out's arrays.
 * cw_overlap_run: host pointers, synchronous; counts, builds into memory of the engine's own, runs every read, brings rows, counts and statuses back;
 * CW_E_CAPACITY when a query has CW_OVL_SLOT or CW_OVL_DENSE.  cw_overlap_to_pile_device: per query the first min(n_rows, max_support, its pile slot) rows as
 * cw_overlap tuples for cw_extract_piles_device -- the rows are in pile order already -- and pile_n[j] how many.
 * Limits: n_seqs < 2^24, n_entries < 2^32, reads beyond CW_SW_QMAX are CW_OVL_NONE and no targets (a bin fits 11 bits).
 * CW_E_INVALID before anything is launched: NULL arguments or members, parameters outside their ranges, n_seqs >= 2^24, a misaligned index, first_query +
 * n_queries beyond the set.  Pointers, streams and threading: cw_locate_*'s contract.  cw_last_timings names the stages ovl_count; ovl_build_count,
 * ovl_build_insert, ovl_build_assign, ovl_build_fill; ovl, ovl_dense; ovl_pile. */
#define CW_OVL_K 15u
#define CW_OVL_SAMPLE 3u
#define CW_OVL_MAX_OCC 512u
#define CW_OVL_MIN_HITS 2u     /* twice the largest HITS of unrelated reads on the planted set (tests/test_overlap_cpu.py) */
#define CW_OVL_END_SLACK 143u  /* the largest distance of a reported end from the true overlap's end on that set, plus one bin */
enum { CW_OVL_TARGET, CW_OVL_STRAND, CW_OVL_HITS, CW_OVL_DIAG, CW_OVL_Q_START, CW_OVL_Q_END, CW_OVL_T_START, CW_OVL_T_END, CW_OVL_ROW = 8 };
enum { CW_OVL_OK = 0, CW_OVL_NONE = 1, CW_OVL_SLOT = 2, CW_OVL_DENSE = 3, CW_OVL_BAD_INDEX = 4 };
typedef struct cw_overlap_params { uint32_t k, sample, max_occ, min_hits; } cw_overlap_params;
typedef struct cw_overlap_index {
    uint32_t* mem;          /* [cw_overlap_index_words(n_entries)], the caller's, 8-byte aligned */
    uint64_t n_entries;     /* cw_overlap_count_device's answer for the read set and prm */
    cw_overlap_params prm;
} cw_overlap_index;
typedef struct cw_overlaps {
    int32_t* rows;
    const uint64_t* row_off; /* [n_queries + 1], in rows, ascending */
    uint32_t* n_rows;        /* [n_queries] */
    uint8_t* status;         /* [n_queries] */
} cw_overlaps;
struct cw_overlap; /* (declared below) */
int cw_overlap_count_device(cw_engine* e, const cw_batch* reads, const cw_overlap_params* prm, uint64_t* n_entries, void* hip_stream);
uint64_t cw_overlap_index_words(uint64_t n_entries);
int cw_overlap_build_device(cw_engine* e, const cw_batch* reads, const cw_overlap_index* index, void* hip_stream);
int cw_overlap_run_device(cw_engine* e, const cw_overlap_index* index, const cw_batch* reads, uint32_t first_query, uint32_t n_queries, const cw_overlaps* out,
                          void* hip_stream);
int cw_overlap_run(cw_engine* e, const cw_batch* reads, const cw_overlap_params* prm, const cw_overlaps* out);
int cw_overlap_to_pile_device(cw_engine* e, const cw_overlaps* rows, uint32_t n_queries, uint32_t max_support, struct cw_overlap* pile, const uint64_t* pile_off,
                              uint32_t* pile_n, void* hip_stream);

/* ---- align a query only where it was placed: reference spans ------------------------------------------------------------------------------------------------------
 * The four alignment runs sweep every query over ALL columns of its reference.  Each has a span form that confines query s to the reference columns
 * [ref_lo[s], ref_hi[s]): cw_sw_span_run, cw_sw_path_span_run, cw_pileup_span_run, cw_sw_cut_span_run and their _device forms -- the counterpart's
 * arguments with `spans` before flags / hip_stream, and the counterpart's pointer conventions (host / device, the two arrays of spans included), stream
 * contract, flags, statuses and stage names.  Per query s with reference r of n bases, each a function of the pair and its two span words alone:
 *   clamping       lo = min(ref_lo[s], n), hi = min(ref_hi[s], n).  The entries of references are not read.
 *   empty span     hi <= lo (lo > hi as given included): the row of an empty reference -- score 0, begins 0, ends -1, CW_SW_ALIGNED -- no ops, nothing counted,
 *                  T + 1 zero cut words.
 *   otherwise      what the counterpart gives for a group whose reference is reference[lo, hi), with lo added to CW_SW_REF_BEGIN and CW_SW_REF_END when the
 *                  score is positive: score, query ends, ins / del, status and ops are identical.  Pileup columns and cut boundaries are ABSOLUTE, on the
 *                  whole reference: col_off slots, T = ceil(n / W), CW_SW_CUTS(n, W), the clearing of columns 0 .. n - 1, CW_SW_PILE_SLOT and CW_SW_CUT_SLOT
 *                  refer to n, and the cut formula above holds with the absolute ref_begin / ref_end.  A base just outside [lo, hi) never takes part, even
 *                  when it would extend the alignment.
 *   capacities     CW_SW_STOP for a query of more than CW_SW_QMAX bases, for a clamped span of more than CW_SW_RMAX columns -- CW_SW_RMAX is a capacity of the
 *                  sweep, which holds a column in 16 bits, not of the reference -- and for n > INT32_MAX (a row holds a column in 32).  A reference of any
 *                  other length is valid here; the entry points without spans keep their stop at n > CW_SW_RMAX.
 * CW_E_INVALID on top of the counterpart's: spans == NULL, or one of its members while n_seqs > 0.  The host forms upload the two arrays with the batch.
 * cw_cut_groups_device takes the rows and cuts of a span run as they come.
 *
 * cw_seed_spans_device: the spans of a seed run, on the device, one thread a sequence.  With m the query's length, n its reference's and
 * P = pad + (m >> pad_shift), in 64-bit signed arithmetic:
 *   a placed query    (CW_SEED_STATUS is CW_STRAND_FWD or CW_STRAND_REV and CW_SEED_HITS >= min_hits)
 *                     lo = clamp(CW_SEED_DIAG - P, 0, n), hi = clamp(CW_SEED_DIAG + (2 << CW_SEED_SHIFT) + m + P, 0, n): the window's 128 diagonals over the
 *                     whole query, and the pad for the drift of a read's diagonal from its densest window
 *   everything else   (CW_STRAND_IS_REF, CW_STRAND_NONE, fewer hits) lo = hi = 0: an unplaced read then costs the aligner nothing
 * CW_SEED_DIAG is in the ORIENTED query's coordinates: the spans are meant for the batch cw_revcomp_device wrote from the seed run's strand bytes, not for the
 * batch the seed run read.  CW_E_INVALID for pad_shift > 31, NULL groups / seed_rows, NULL ref_lo / ref_hi while n_seqs > 0, more than
 * cw_max_batch_windows(e) groups.  Device pointers, asynchronous on `hip_stream`, cw_strand_run_device's contract; no scratch; one stage, seed_spans.
 * cw_seed_spans: host pointers, synchronous.  CW_SPAN_PAD_SHIFT is measured: the smallest pad of pad_shift 4, 3, 2 at pad 64 under which every
 * planted read of the project's tests aligns inside its span exactly as on the whole reference. */
typedef struct cw_sw_spans {
    const uint32_t* ref_lo;   /* [n_seqs] first reference column a query may use       */
    const uint32_t* ref_hi;   /* [n_seqs] one past the last; entries of references are not read */
} cw_sw_spans;
#define CW_SPAN_PAD 64u
#define CW_SPAN_PAD_SHIFT 4u
int cw_sw_span_run_device(cw_engine* e, const cw_batch* groups, int32_t* rows, const cw_sw_spans* spans, uint32_t flags, void* hip_stream);
int cw_sw_span_run(cw_engine* e, const cw_batch* groups, int32_t* rows, const cw_sw_spans* spans, uint32_t flags);
int cw_sw_path_span_run_device(cw_engine* e, const cw_batch* groups, int32_t* rows, const cw_sw_paths* paths, const cw_sw_spans* spans, uint32_t flags, void* hip_stream);
int cw_sw_path_span_run(cw_engine* e, const cw_batch* groups, int32_t* rows, const cw_sw_paths* paths, const cw_sw_spans* spans, uint32_t flags);
int cw_pileup_span_run_device(cw_engine* e, const cw_batch* groups, int32_t* rows, const cw_pileup* pile, const cw_sw_spans* spans, uint32_t flags, void* hip_stream);
int cw_pileup_span_run(cw_engine* e, const cw_batch* groups, int32_t* rows, const cw_pileup* pile, const cw_sw_spans* spans, uint32_t flags);
int cw_sw_cut_span_run_device(cw_engine* e, const cw_batch* groups, int32_t* rows, const cw_sw_cuts* cuts, const cw_sw_spans* spans, void* hip_stream);
int cw_sw_cut_span_run(cw_engine* e, const cw_batch* groups, int32_t* rows, const cw_sw_cuts* cuts, const cw_sw_spans* spans);
int cw_seed_spans_device(cw_engine* e, const cw_batch* groups, const int32_t* seed_rows, uint32_t min_hits, uint32_t pad, uint32_t pad_shift,
                         uint32_t* ref_lo, uint32_t* ref_hi, void* hip_stream);
int cw_seed_spans(cw_engine* e, const cw_batch* groups, const int32_t* seed_rows, uint32_t min_hits, uint32_t pad, uint32_t pad_shift,
                  uint32_t* ref_lo, uint32_t* ref_hi);

/* 1 when everything the last cw_run_device on this engine launched has completed (or nothing was launched yet), 0 while it is
 * still running, 2 while it is running but past the part that fills the GPU (what is left is the tail: a few long alignment tasks on
 * one wave each, then the finish kernel); never blocks.  For callers that keep several engines busy: hand the next batch to an
 * engine that returns 1.  (Waiting for the other engine to reach 2 before starting -- batches staggered instead of side by side --
 * halves a batch's latency and measured 4 % less throughput at depth 150: bench.py, CW_BENCH_STAGGER.) */
int cw_poll(cw_engine* e);

/* Milliseconds spent in each device stage of the last cw_run / cw_run_device on this engine, measured
 * with HIP events on the launch stream.  n_stages entries are written (at most cap); names are static. */
int cw_last_timings(cw_engine* e, float* ms, const char** names, int cap, int* n_stages);

/* Pack one ASCII window pile (n strings, lens[i] bytes each, not NUL-terminated) at the tail of host
 * arrays laid out as cw_batch.  words_cap counts 32-bit words available at bases_out.  Returns the
 * number of words written, or a negative cw_status.  Non-ACGT bytes pack as T (utils.cpp:28). */
int64_t cw_pack_sequence(const char* seq, uint32_t len, uint32_t* bases_out, uint64_t words_cap);

/* ---- device-side pile extraction ------------------------------------------------------------------
 * Stands in for getAlignmentWindowsSequences (src/alignmentWindows.cpp:87-149) + the read decoding of getSequencesMap
 * (src/alignmentPiles.cpp:5-20): piles are cut on the GPU from the 2-bit read set and the overlap tuples. */
typedef struct cw_read_set {      /* the indexed reads (utils.cpp:166-205), 2-bit packed like cw_batch.bases */
    uint32_t n_reads;
    const uint32_t* read_len;      /* [n_reads] */
    const uint64_t* read_word_off; /* [n_reads] */
    const uint32_t* bases;
} cw_read_set;

typedef struct cw_overlap {        /* one PAF record after Overlap(std::string) (src/Overlap.h:26-58): ends INCLUSIVE */
    uint32_t q_start, q_end;
    uint32_t t_read;               /* index of the target read in the read set (its length is tLength)             */
    uint32_t t_start, t_end;
    uint32_t strand;               /* 0 '+', 1 '-' */
} cw_overlap;

typedef struct cw_window_job {     /* one window of one template (pilesPos[i], CONSENT-correction.cpp:35)            */
    uint32_t tpl_read;
    uint32_t q_beg, q_end;         /* inclusive */
    uint32_t ovl_first, ovl_count; /* the template's pile in `overlaps`, in getNextReadPile order                    */
} cw_window_job;

/* HOST function: window positions of one template, getAlignmentWindowsPositions (src/alignmentWindows.cpp:27-85, with
 * getCoverages :5-25).  `overlaps` is the template's pile (only q_start/q_end are read).  Writes (beg,end) pairs, inclusive,
 * in the reference's order (forward windows, then the one trailing window); *n_pairs = how many exist; CW_E_CAPACITY if
 * cap_pairs was too small (call again).  CW_E_INVALID if an overlap ends beyond the template. */
int cw_window_positions(uint32_t tpl_len, const cw_overlap* overlaps, uint32_t n_overlaps, uint32_t min_support, uint32_t window_size,
                        int32_t window_overlap, uint32_t* out_beg_end, uint32_t cap_pairs, uint32_t* n_pairs);

/* All pointers are DEVICE pointers (read set, overlaps, jobs, and the four output arrays laid out as cw_batch:
 * win_first_seq[n_jobs+1], seq_len[seq_cap], seq_word_off[seq_cap], bases[word_cap]).  On return *n_seqs / *n_words hold
 * the totals (the call synchronises once to read them); CW_E_CAPACITY if they exceed the capacities -- call again with
 * larger arrays (capacities 0 just size the batch).  A window beyond its template (alignmentWindows.cpp:95-97) or a
 * piece shorter than k (:141) yields no member, as in the reference. */
int cw_extract_piles_device(cw_engine* e, const cw_read_set* reads, const cw_overlap* overlaps, uint64_t n_overlaps,
                            const cw_window_job* jobs, uint32_t n_jobs, uint32_t k, uint32_t* win_first_seq, uint32_t* seq_len,
                            uint64_t* seq_word_off, uint32_t* bases, uint32_t seq_cap, uint64_t word_cap, uint32_t* n_seqs,
                            uint64_t* n_words, void* hip_stream);

/* Result slots for a device-resident batch (what a caller of cw_run_device has to size before the call): writes the exclusive offsets
 * cons_off[n_windows+1] (CW_CONS_SLOT_BYTES(k, template length) per window) and solid_off[n_windows+1] (k-mers in the window's pile /
 * solidThresh + 16 entries), both DEVICE arrays, and returns their totals (one synchronisation).
 *
 * The consensus slot.  A consensus is about as long as its template; the polish may lengthen it; with k < 9, chance anchors make consensuses of
 * several templates (the finish kernel holds 32768 characters).  Slots are real device memory (and, through cw_submit, twice that per batch in
 * flight), so the rule follows k: k >= 9 -- no window of the randomised testers (5e5 windows, k 9..16) ever went beyond three templates + 256 --
 * gets four templates + 1024, at least 3072; k = 8 sixteen templates + 1024; k < 8 the full 32768.  A consensus that outgrows its slot is a
 * reported capacity (window status 2, CW_WHY_OUT_CONS), never a truncation; a caller that sizes its own slots may give every window 32768. */
#define CW_CONS_SLOT_MAX 32768u
#define CW_CONS_SLOT_BYTES(k, tpl_len) \
    ((k) >= 9u ? (4u * (uint32_t)(tpl_len) + 1024u < 3072u ? 3072u : (4u * (uint32_t)(tpl_len) + 1024u > CW_CONS_SLOT_MAX ? CW_CONS_SLOT_MAX : 4u * (uint32_t)(tpl_len) + 1024u)) \
     : (k) == 8u ? (16u * (uint32_t)(tpl_len) + 1024u > CW_CONS_SLOT_MAX ? CW_CONS_SLOT_MAX : 16u * (uint32_t)(tpl_len) + 1024u) : CW_CONS_SLOT_MAX)
int cw_plan_results_device(cw_engine* e, const cw_batch* batch, uint64_t* cons_off, uint64_t* solid_off, uint64_t* cons_total, uint64_t* solid_total,
                           void* hip_stream);

/* ---- host feeders: read indexer and PAF pile reader, plain host code ------------------------------------
 * cw_index_reads stands in for indexReads (src/utils.cpp:166-205): FASTA or FASTQ (multi-line allowed) -> 2-bit reads keyed by
 * name (header up to the first blank; a later record with the same name replaces the earlier one; bases upper-cased, anything
 * but A/C/G packs as T).  The view's pointers are HOST pointers laid out like the device read set: upload them once. */
typedef struct cw_read_index cw_read_index;
int cw_index_reads(const char* path, cw_read_index** out);
int cw_index_reads_append(cw_read_index* idx, const char* path);   /* a second file into the same index (the proof file, CONSENT-correction.cpp:69-73) */
void cw_read_index_free(cw_read_index* idx);
uint32_t cw_read_index_count(const cw_read_index* idx);
int cw_read_index_view(const cw_read_index* idx, cw_read_set* host_view, uint64_t* n_words);
int32_t cw_read_index_find(const cw_read_index* idx, const char* name);   /* read id or -1 */
const char* cw_read_index_name(const cw_read_index* idx, uint32_t id);

/* cw_paf_next_pile stands in for getNextReadPile (src/alignmentPiles.cpp:22-58) with Overlap(std::string) (src/Overlap.h:26-58):
 * the next run of consecutive PAF lines sharing a query name, ends made inclusive, sorted by residue matches descending with the
 * reference's own std::sort expression (ties in libstdc++'s order), cut to max_support.  *n = overlaps in the pile, 0 at the end
 * of the file; *tpl_read / *tpl_len = the query's id in the index and its length as the PAF states it; res_matches may be NULL.
 * CW_E_CAPACITY when cap < *n (the pile is consumed: size the buffer for max_support); CW_E_INVALID on a malformed line or a
 * name missing from the index. */
typedef struct cw_paf_reader cw_paf_reader;
int cw_paf_open(const char* path, const cw_read_index* idx, uint32_t max_support, cw_paf_reader** out);
int cw_paf_next_pile(cw_paf_reader* r, uint32_t* tpl_read, uint32_t* tpl_len, cw_overlap* out, uint32_t* res_matches, uint32_t cap,
                     uint32_t* n);
void cw_paf_close(cw_paf_reader* r);

/* ---- wrapper plumbing: the small tools CONSENT-correct / CONSENT-polish run around the binary, as host functions.
 * cw_paf_reformat <- src/reformatPAF.cpp:22-46 (swap query and target columns); cw_paf_explode <- src/explode.cpp:14-51 (split so
 * that every query name is one run of lines per file; files are out_prefix_1 .. out_prefix_N); cw_paf_merge <- src/merge.cpp:29-65
 * (gather, in the order of a header file, every read's lines from the exploded chunks). */
int cw_paf_reformat(const char* in_path, const char* out_path);
int cw_paf_explode(const char* in_path, const char* out_prefix, uint32_t* n_files);
int cw_paf_merge(const char* out_path, const char* headers_path, const char* const* in_paths, uint32_t n_in);

/* ---- read re-assembly on the device -------------------------------------------------
 * Stands in for alignConsensus (src/correctionAlignment.cpp:47-140) followed, when do_trim != 0, by trimRead(.,1) and
 * dropRead (src/CONSENT-correction.cpp:47-58, src/utils.cpp:96-128, :71-73): every window consensus of a read is
 * aligned back onto the lower-cased read (local alignment, scores and position rules in include/cw_policy.h) and
 * replaces the aligned stretch in upper case; overlapping windows are reconciled by their solid k-mers. */
typedef struct cw_stitch_read {
    uint32_t read;                 /* the template in the read set (sequences[alignments[0].qName])                  */
    uint32_t win_first, win_count; /* its windows in the batch / result arrays, in pilesPos order                     */
} cw_stitch_read;

#define CW_READ_OK       0
#define CW_READ_DROPPED  1  /* dropRead: fewer than 10 % corrected bases after trimming; out_len = 0                    */
#define CW_READ_CAPACITY 2  /* output slot, consensus (> 32768) or aligned slice (> 2048) too large; out_len = 0         */

/* All pointers are DEVICE pointers.  `win_pos` = (beg,end) per window as cw_window_positions wrote them; `batch` = the piles
 * the consensuses were computed from (the first sequence of a window is its template, CONSENT-correction.cpp:37);
 * `res` = what cw_run_device filled (cons, cons_off, cons_len, win_status, solid, solid_off, solid_len; solid is required).
 * out_off[n_reads+1] gives every read a slot (2*read_len + 1024 is ample); the corrected read is written at its start,
 * out_len[r] characters, upper case = corrected.  Windows with CW_WIN_OVERFLOW are left uncorrected.  Asynchronous on
 * `hip_stream` (NULL = the engine's stream). */
int cw_stitch_device(cw_engine* e, const cw_read_set* reads, const cw_stitch_read* jobs, uint32_t n_reads, const uint32_t* win_pos,
                     const cw_batch* batch, const cw_result* res, uint32_t window_size, uint32_t window_overlap, int32_t do_trim,
                     char* out, const uint64_t* out_off, uint32_t* out_len, uint8_t* read_status, void* hip_stream);

/* ---- the drivers' loop (SURVEY 8b "who calls it", 8e, 8f-4) -----------------------------------------------------------------------
 * cw_run_correction stands in for runCorrection of BOTH reference drivers -- src/CONSENT-correction.cpp:62-135 (with processRead :19-58)
 * when polishing == 0, src/CONSENT-polishing.cpp:107-135 (with processContig :21-105) when polishing != 0 -- called by src/main.cpp:78
 * with the values of its getopt loop (:29-76).  bin/CONSENT-correction and bin/CONSENT-polishing are that main() over this function.
 * FASTA records (">name\nsequence\n") go to the file descriptor out_fd in PAF order; a read without windows, or dropped by the 10 % rule,
 * produces none.  Trimming and dropping happen only for correction without a proof file (CONSENT-correction.cpp:17,69-73).
 * nb_threads (-j) = how many GPUs to use: the first min(nb_threads, visible devices); `devices` / the environment variable CW_DEVICES
 * ("0,1,..", an id may repeat: one worker = one engine per entry) override that; by default every device gets two workers, so that
 * one job's re-assembly overlaps the other's consensus kernels (CW_WORKERS_PER_DEVICE changes the two).  Piles are handed to the devices job by job from one queue, there is no collective, and
 * the output does not depend on the number of devices.  paf_index (-i) and path (-p) are accepted and, as in the reference, never read. */
typedef struct cw_driver_args {
    const char* paf_index;      /* -i */
    const char* alignment_file; /* -a */
    const char* reads_file;     /* -r */
    const char* proof_file;     /* -R, NULL or "" = none */
    const char* path;           /* -p */
    uint32_t min_support, max_support, window_size, mer_size, common_kmers, min_anchors, solid_thresh, window_overlap, nb_threads, max_msa;
    int32_t polishing;
    const int32_t* devices;     /* NULL = choose as described above */
    int32_t n_devices;
    uint32_t windows_per_batch; /* windows per job; 0 = 32768, fewer (down to 4096) when the templates are too few for four such jobs per worker */
} cw_driver_args;

typedef struct cw_driver_stats {
    uint32_t n_devices;
    uint64_t piles, windows, overlaps, jobs, records, bases_out;
    double ms_index, ms_total;
    uint64_t dev_windows[16];
    double dev_ms_extract[16], dev_ms_consensus[16], dev_ms_stitch[16];
} cw_driver_stats;

int cw_run_correction(const cw_driver_args* args, int out_fd, cw_driver_stats* stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* CONSENT_AMD_H */
