/*
 * cw_private.h -- entry points of libconsent_amd.so that are NOT part of the drop-in boundary (include/consent_amd.h):
 * inspection aids for the tests and the synthetic-pile generator of bench.py / the tests.  They are exported from the
 * shared library so that bench.py, tools/ and tests/ can reach them (ctypes / dlsym); no product caller needs them.
 */
#ifndef CW_PRIVATE_H
#define CW_PRIVATE_H

#include "../../include/consent_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* copies the engine's per-window bookkeeping of the last run to host, 16 uint32 per window: status, n_seqs, tpl_len, n_kmers,
 * solid_base, solid_cap, n_solid, seg_base, seg_cap, n_segs, arena_base, arena_cap, arena_used (of a window stopped on CW_WHY_MATRIX: the
 * matrix slot elements it needed), ab_base, ab_cap, why (CW_WHY_*) */
int cw_debug_win_info(cw_engine* e, uint32_t n_windows, uint32_t* out16);
/* the index kernel's count table of one window of the last run: its ascending solid k-mers and their exact pile-wide counts (the window's slice of
 * the solid table, WinInfo::solid_base / n_solid).  *n receives the number of entries, the first min(*n, cap) of them are copied; a window that was
 * stopped before or in the count phase has none.  Valid when cw_debug_win_info is: after a run, until the next one on this engine. */
int cw_debug_solid_table(cw_engine* e, uint32_t window, uint32_t* keys, uint32_t* counts, uint32_t cap, uint32_t* n);
/* the anchor block of one window of the last run, the bytes idx_hand_over wrote (cw_index.h CwAbCarve: header A, N, n_dirty, flags, n_rows; ckey, pres,
 * dirty, badm, rowid, delta, P).  *n receives cw_ab_bytes of the block's own header, the first min(*n, cap) bytes are copied.  CW_E_INVALID for a window the
 * index kernel did not finish (stopped by the setup or index phase, or without a template k-mer), after a POA-only run (no blocks), and for a header that
 * claims more than the window's slice.  Host code only, in both builds; valid when cw_debug_solid_table is.  DESIGN.md says which bytes are specified. */
int cw_debug_anchor_block(cw_engine* e, uint32_t window, uint8_t* out, uint64_t cap, uint64_t* n);
/* the nine offsets of that layout for a block of these numbers -- hdr, ckey, pres, dirty, badm, rowid, delta, P, end -- without an engine or a device */
int cw_debug_ab_layout(uint32_t A, uint32_t N, uint32_t n_dirty, uint32_t n_rows, uint64_t* out9);
/* the chain kernel's segmentation of one window of the last run.  *n_segs: WinInfo::n_segs (chain anchors + 1; 0 for a window without a chain); seg_len: the
 * first min(*n_segs, seg_cap) of the window's segment lengths (of a segment that became a POA task: the length of the tier's consensus); tasks4: four words
 * per task record that names the window, in the order of the task array -- segment index (seg_slot - seg_base), n_members, longest member, index of its
 * first member in members3; members3: three words per member -- sequence (counted from the window's first), start, length.  *n_tasks and *n_members
 * receive what the window has, the first task_cap / member_cap of them are copied.  Host code only, in both builds.  The member array is written by the
 * chain kernel (by cw_poa_tasks_kernel in an operator run) and only read by the tiers, as are the task fields returned here.  Valid when
 * cw_debug_solid_table is, and for a cw_run_device caller while the batch's win_first_seq array is still allocated. */
int cw_debug_segments(cw_engine* e, uint32_t window, uint32_t* n_segs, uint32_t* seg_len, uint32_t seg_cap, uint32_t* tasks4, uint32_t task_cap, uint32_t* n_tasks,
                      uint32_t* members3, uint32_t member_cap, uint32_t* n_members);
/* The scratch plan of a batch of these dimensions on a device of `cus` compute units, in bytes, without a device: out[0] total, then windows' records,
   solid table, segments, arena, tasks + members, tier lists, slabs of tiers S, M1, M2, L, G, tier Q's + H's rows, anchor blocks, position-matrix
   fallbacks, exact-count fallbacks, finish pass buffers (15 numbers; tools/plan_sizes.py). */
int cw_debug_plan(uint32_t k, uint32_t solid, uint32_t n_windows, uint32_t n_seqs, uint64_t n_words, int cus, uint32_t scale, uint32_t tmax, uint64_t* out15);
/* The capacities of that plan (pf_full: the matrix slot of a re-run after CW_WHY_MATRIX), without a device: out[0] total bytes, [1] solid table entries,
   [2] segment slots, [3] arena bytes, [4] the arena's scale after its 32-bit clamp, [5] rows per template k-mer of the matrix slot, [6] the batch limit
   of an engine with this tmax (cw_max_batch_windows), [7] task slots. */
int cw_debug_plan_caps(uint32_t k, uint32_t solid, uint32_t n_windows, uint32_t n_seqs, uint64_t n_words, int cus, uint32_t scale, uint32_t tmax, int pf_full, uint64_t* out8);
/* The scratch plan of a POA-only run (cw_poa_run) of n_groups groups, n_seqs sequences and n_words packed words, without a device: the fifteen numbers of
   cw_debug_plan in the same order -- solid table, anchor blocks, the fallbacks and the finish buffers (indices 2, 13, 14) are 0 in it.  CW_E_INVALID for a
   batch whose arena would pass the 32-bit offsets, as cw_poa_run answers it. */
int cw_debug_poa_plan(uint32_t n_groups, uint32_t n_seqs, uint64_t n_words, int cus, uint64_t* out15);
/* The scratch plan of an alignment run (cw_sw_run) of n_groups groups, n_seqs sequences and n_words packed words under `flags`, without a device: out[0] total
   bytes, [1] the order kernel's counters + a reference index and a place in the order per sequence, [2] unpacked long references, [3] the long launch's buffers
   and sweep state, [4] banded-traceback directions (0 without CW_SW_WANT_INDELS), [5] [6] [7] work-groups of the class-0, class-1 and long launches, [8] waves
   that have direction scratch, [9] its bytes per wave.  CW_E_INVALID for flags cw_sw_run refuses. */
int cw_debug_sw_plan(uint32_t n_groups, uint32_t n_seqs, uint64_t n_words, int cus, uint32_t flags, uint64_t* out10);
/* The scratch plan of a path run (cw_sw_path_run) likewise: out[0] total bytes, [1] counters + reference index, span begin and span length + place in the order, [2] unpacked long references,
   [3] the long launch's state, [4] the traceback's scratch (directions, and rows beyond LDS), [5] the walks' step buffers, [6] [7] [8] work-groups of the class-0,
   class-1 and long launches, [9] waves that have traceback scratch, [10] its bytes per wave, [11] a step buffer's bytes.  CW_E_INVALID for flags other than
   CW_SW_PATH_EQX. */
int cw_debug_sw_path_plan(uint32_t n_groups, uint32_t n_seqs, uint64_t n_words, int cus, uint32_t flags, uint64_t* out12);
/* The scratch plan of a strand run (cw_strand_run) of n_groups groups and n_seqs sequences, without a device: out[0] total bytes, [1] the claim counters and class
   totals, [2] the first unit of every group, [3] [4] work-groups of the narrow and the wide launch. */
int cw_debug_strand_plan(uint32_t n_groups, uint32_t n_seqs, int cus, uint64_t* out5);
/* The same of a seed run (cw_seed_run): plan_strand's arithmetic, the narrow launch at most six work-groups a CU. */
int cw_debug_seed_plan(uint32_t n_groups, uint32_t n_seqs, int cus, uint64_t* out5);
/* The scratch plan of a locate run (cw_locate_run_device) of n_seqs reads, without a device: out[0] total bytes, [1] the counters, [2] the redo list, [3] the
   dense route's tables, [4] [5] work-groups of the LDS and the dense launch. */
int cw_debug_locate_plan(uint32_t n_seqs, int cus, uint64_t* out6);
/* The reads each route took in the engine's last locate run: out[0] the LDS route (the reads without a vote among them), out[1] the dense route.  Waits for the
   device.  CW_E_INVALID before the first locate run. */
int cw_debug_locate_routes(cw_engine* e, uint32_t* out2);
/* The scratch plan of an overlap run (cw_overlap_run_device) of n_queries queries, without a device: out[0] total bytes, [1] the counters, [2] the redo list, [3]
   the dense route's tables, [4] [5] work-groups of the LDS and the dense launch. */
int cw_debug_overlap_plan(uint32_t n_queries, int cus, uint64_t* out6);
/* The queries each route took in the engine's last overlap run: out[0] the LDS route (CW_OVL_NONE among them), out[1] the dense route.  Waits for the device.
   CW_E_INVALID before the first overlap run. */
int cw_debug_overlap_routes(cw_engine* e, uint32_t* out2);
/* cw_max_batch_windows of an engine that cw_configure(max_template_len) will be called on (the native driver sizes its jobs before it has engines) */
uint32_t cw_plan_max_batch_windows(uint32_t k, uint32_t max_template_len);

/* a32[i] += add32 for i < n32 and a64[i] += add64 for i < n64, on the stream: how the driver turns the window -> sequence and sequence -> word
   offsets of a pile extracted in several calls into offsets of one batch (cw_driver.cpp) */
int cw_add_offsets_device(uint32_t* a32, uint64_t n32, uint32_t add32, uint64_t* a64, uint64_t n64, uint64_t add64, void* hip_stream);
/* batch counters of the last run (uint32: tasks, members, next_task, next_window, next_finish, any_overflow, then n_tier, next_tier, n_over,
 * next_over with one entry per POA tier: 6 + 4 * 6 = 30 words) and its GPU cycle counts (uint64, 128 words: index kernel 0-7; POA tier t at
 * 8+5t..12+5t: metadata, fill, traceback, merge, consensus; 36+t: the longest single task of tier t; 63: the index kernel's route bits and 45: the chain
 * kernel's, written by a -DCW_TEST_AIDS build only (cw_index.h CwIdxRoute, cw_chain.h CwChRoute), as are 33-35: the finish kernel's route bits, the frames its
 * fin_link entered and the fin_neighbours calls it made (cw_finish.h CwFinRoute), and 69-71 and 126: the slab POA tiers' route bits, 32 a tier, and the causes of
 * their rc 2, a byte a tier (cw_poa.h CwPoaRoute, CwPoaRc2); 72+12t..: row counts of a -DCW_DIAG build).  The caller passes the capacity of each buffer in words and receives min(capacity, available); the counts come back through
 * counters_n / prof_n when those are not NULL. */
/* cw_run_device + wait for the stream + one more run with larger task / member / arena capacities, or the full matrix slot, when windows stopped on those only */
int cw_run_device_sync(cw_engine* e, const cw_batch* batch, const cw_result* res, void* hip_stream);
int cw_debug_profile(cw_engine* e, uint32_t* counters, uint32_t counters_cap, unsigned long long* prof, uint32_t prof_cap, uint32_t* counters_n, uint32_t* prof_n);
/* tier X's counters of the last run (4 uint32): tasks tier G handed on to it, tasks it aligned, tasks that outgrew it too (their windows stop on
 * CW_WHY_POA), the largest alignment it was asked for in int32 cells (three layers under the affine gap model) */
int cw_debug_tier_x(cw_engine* e, uint32_t* out4);
int cw_debug_tier_q(cw_engine* e, uint32_t* out3); /* tier Q's split (long entries of its list), short tasks finished by the eight-lane loop, short tasks handed on */
/* One routed list of the last run (list: 0 tier Q's, 1 M1, 2 M2, 3 L, 5 H): *n its entries, the first min(*n, cap) of them in `sorted` as the tier sort left
 * them (plain task indices) and -- *kept = 1: a -DCW_TEST_AIDS build run with CW_KEEP_EMITTED set; otherwise 0 -- in `emitted` as the chain kernel
 * (cw_poa_tasks_kernel) wrote them: task index | sort class << 24.  tasks4: four words per task record of the batch in the order of the task array -- window,
 * segment slot, n_members, longest member | mean member length << 16 (what the class is computed from); *n_tasks of them, the first task_cap copied.  A task
 * index equal to the plan's task capacity (cw_debug_plan_caps [7]) names the batch's neutral task. */
int cw_debug_tier_lists(cw_engine* e, uint32_t list, uint32_t* sorted, uint32_t* emitted, uint32_t cap, uint32_t* n, uint32_t* kept, uint32_t* tasks4, uint32_t task_cap,
                        uint32_t* n_tasks);

/* with CW_TASK_TRACE set in the environment: 12 words per POA task of the last run (see cw_engine.cpp); tier 6 = tier X */
int cw_debug_task_trace(cw_engine* e, uint32_t cap_tasks, uint32_t* out12, uint32_t* n_tasks);

/* with CW_STITCH_TRACE set in the environment the last cw_stitch_device call records, per window, 8 words (al_pos, size_al, score,
 * ref_begin, ref_end, query_begin, query_end, query_len); 0xFFFFFFFF = window not aligned */
int cw_debug_stitch_trace(cw_engine* e, uint32_t n_windows, uint32_t* out);
/* the route witness of the same call (cw_stitch.h CwStRoute / CwStBand / CwStRead): 16 words per window (route, band, then beg, end, overlap, s1, s2, the
 * sub-alignment's score, ins, del, cut, cl, cur_pos handed on, the gap's move; 0xFFFFFFFF = not reached) and one word per read of the call, the reads
 * in the order of its jobs.  Returns 1 when they were copied, 0 when nothing was recorded (only a -DCW_TEST_AIDS build records, and only with
 * CW_STITCH_TRACE set), a negative error otherwise. */
int cw_debug_stitch_route(cw_engine* e, uint32_t n_windows, uint32_t n_reads, uint32_t* win_out, uint32_t* read_out);

/* ---- synthetic PacBio/ONT-profile piles (bench + tests; SURVEY 8d generator) --------------------- */
typedef struct cw_synth_spec {
    uint64_t seed;        /* window w draws from seed + first_window + w            */
    uint64_t first_window;
    uint32_t n_windows;
    uint32_t depth;       /* support sequences per window (pile size = depth + 1)     */
    uint32_t window_len;  /* template length, 500                                     */
    uint32_t err_permille;/* total error rate, 120 = 12 %                             */
    uint32_t sub_w, ins_w, del_w; /* error mix, PacBio 10:60:30, ONT 30:30:40          */
    uint32_t seq_stride_words;    /* words reserved per sequence (>= (window_len+60)/16+1) */
} cw_synth_spec;

/* Sizes of the arrays a synthetic batch needs. */
int cw_synth_sizes(const cw_synth_spec* spec, uint32_t* n_seqs, uint64_t* n_words);
/* Fill host arrays (win_first_seq[n_windows+1], seq_len[n_seqs], seq_word_off[n_seqs], bases[n_words]). */
int cw_synth_host(const cw_synth_spec* spec, uint32_t* win_first_seq, uint32_t* seq_len, uint64_t* seq_word_off,
                  uint32_t* bases);
/* Same arrays as DEVICE pointers, generated by a HIP kernel on `hip_stream`. */
int cw_synth_device(cw_engine* e, const cw_synth_spec* spec, uint32_t* win_first_seq, uint32_t* seq_len,
                    uint64_t* seq_word_off, uint32_t* bases, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
