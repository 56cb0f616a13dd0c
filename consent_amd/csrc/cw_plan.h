/* cw_plan.h -- the engine's scratch plan: how large every part of a batch's one device allocation is and where it sits.  Host arithmetic only, no call into
   the HIP runtime: cw_engine.cpp allocates, binds and launches by it, and tests/test_plan_limits.py pins its numbers (cw_debug_plan, cw_debug_plan_caps). */
#ifndef CW_PLAN_H
#define CW_PLAN_H

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "cw_env.h"
#include "cw_index.h"  /* CW_EXG_SLOTS; with each of these: cw_device.h (the records' sizes, CW_TIERS) and include/consent_amd.h */
#include "cw_poa_q.h"  /* slab and graph sizes of every tier (cw_poa.h comes with it) */
#include "cw_sw_path.h" /* the alignment operator's per-wave sizes, the path run's too (cw_sw_op.h and cw_stitch.h come with it) */
#include "cw_strand.h" /* the strand vote's chunk sizes */
#include "cw_seed.h"   /* the seed run's LDS, which bounds its work-groups a CU */
#include "cw_locate.h" /* the locate run's LDS and the dense route's table */
#include "cw_overlap.h" /* the overlap run's the same */
#include "cw_finish.h" /* CW_FIN_*.  (These three are kernel headers, taken for their size macros: nothing here runs on the device, but a translation unit that includes this one is still a HIP one) */

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
struct TierCfg { uint32_t slots; size_t slab_bytes; };
static inline size_t big_slab_bytes() { return align_up((size_t)CW_POAB_HC * 4 + CW_POA_GRAPH_BYTES(CW_POAB_NC, CW_POAB_EC, CW_POAB_LC), 256); }

/* Work-groups per CU of the four concurrent POA tier kernels (S, M1, M2, L).  The tiers share each CU's 160 KiB of LDS, every kernel
   is persistent, and which kernel's work-groups get onto a CU first is up to the hardware dispatcher: whatever is resident keeps its
   LDS until its list is empty.  Measured with the task timeline (tools/task_trace.py): with the shallow mix on depth-150 piles tier S
   (3 x 45 KB) held every CU for the first 27 ms and tier L, the long pole, started late (POA stage 79 ms); with fewer S and M2
   work-groups and one more of tier L it takes 69 ms; the shallow piles of config 2 prefer the old mix (19.6 vs 21.5 ms).  No static mix was
   robustly better than this one (round 4: tier S's work-groups take 24 KB, not 45), so there is one, whatever the batch's depth:
   slabs (tier_config) and grids (the launch) go by the same numbers.  CW_WGS_S / _M1 / _M2 / _L override (experiments). */
struct TierMix { uint32_t s, m1, m2, l; };
static inline TierMix tier_mix() {
    TierMix m{4, 5, 4, 2u};
    auto knob = [](const char* name, uint32_t dflt) { const char* v = CW_AID_ENV(name); if (!v) return dflt; const int x = atoi(v); return x >= 1 && x <= 12 ? (uint32_t)x : dflt; };
    m.s = std::min(knob("CW_WGS_S", m.s), 6u); m.m1 = knob("CW_WGS_M1", m.m1); m.m2 = knob("CW_WGS_M2", m.m2); m.l = std::min(knob("CW_WGS_L", m.l), 8u); /* (a knob is 12 at most) */
    return m;
}

/* Work-groups of tier t (0 = S, 1 = M1, 2 = M2, 3 = L) worth launching for a batch of n_windows: the full persistent grid for a full batch,
   fewer for a small one (a 16384-window batch at depth 150 has ~5 tier-S, ~4 tier-M1, ~0.7 tier-M2 and ~0.25 tier-L tasks per window) --
   and with the grids the slabs: an engine used to hold ~10 GB of them whatever the batch, a 24-window batch now holds ~0.3 GB. */
static inline uint32_t tier_wgs_cap(int t, uint32_t n_windows, uint32_t full) {
    static const uint32_t div[4] = {2, 4, 8, 8};
    const uint64_t want = (uint64_t)n_windows / div[t] + 4u;
    return want < full ? (uint32_t)want : full;
}

static inline void tier_config(int cus, uint32_t big_slots, uint32_t n_windows, TierCfg (&t)[CW_TIERS]) {
    /* slabs: one per wave the hardware can hold at once plus a margin; waves claim them (slot_busy) */
    const TierMix mix = tier_mix();
    const uint32_t pass1 = 64u < (uint32_t)cus * 2u ? 64u : (uint32_t)cus * 2u;
    uint32_t l_wgs = tier_wgs_cap(3, n_windows, (uint32_t)cus * mix.l); /* (3.5 MB a slab: a generous count here was 12 GB, and allocating it stalled an engine's first job by 1-2 s) */
    if (l_wgs < pass1) l_wgs = pass1; /* the overflow pass launches its own tier-L work-groups */
    t[0] = {(tier_wgs_cap(0, n_windows, (uint32_t)cus * mix.s) * 2u + 8u) * CW_POA_WAVES, CW_POA_SLAB2_TOTAL(CW_POA_NC, CW_POA_EC, CW_POA_LC)}; /* tier S (round 4: cold arrays, flagged rows and code words in a slab) */
    /* round 6: a margin of an eighth over the waves the grids hold (a half through round 5): the plan of a 10 240-window job was 16.6 GB, most of it slabs,
       and a fresh process with four workers on a device spent 0.6-1.6 s allocating before its first job ran (tools/plan_sizes.py) */
    t[1] = {(tier_wgs_cap(1, n_windows, (uint32_t)cus * mix.m1) * 9u / 8u + 8u) * CW_POAM1_WAVES, CW_POA_SLAB2_TOTAL(CW_POAM1_NC, CW_POAM1_EC, CW_POAM1_LC)};
    t[2] = {(tier_wgs_cap(2, n_windows, (uint32_t)cus * mix.m2) * 9u / 8u + 8u) * CW_POAM2_WAVES, CW_POA_SLAB2_TOTAL(CW_POAM2_NC, CW_POAM2_EC, CW_POAM2_LC)};
    t[3] = {(l_wgs * 9u / 8u + 8u) * CW_POAL_WAVES, CW_POA_SLAB2_TOTAL(CW_POAL_NC, CW_POAL_EC, CW_POAL_LC)};
    const uint64_t bs = (uint64_t)n_windows / 16u + 8u;
    t[4] = {bs < big_slots ? (uint32_t)bs / 4u * 4u : big_slots, big_slab_bytes()};
    t[5] = {8u, 64u}; /* (tier H's slabs go by resident task, not by claim: ScratchPlan::hslab) */
}

/* what a plan is made from: the engine's parameters and state (cw_engine.cpp plan_input) and a batch's three totals */
struct PlanInput {
    cw_params prm;
    uint32_t n_windows, n_seqs; uint64_t n_words; /* the batch's totals */
    int cus;            /* compute units of the device */
    uint32_t big_slots; /* tier G's slabs at most: 64, the test aid CW_BIG_SLOTS changes it per run */
    uint32_t scale;     /* 1, or 4 / 16 / 64 after a run whose windows stopped on the task / member / arena capacities (see below) */
    uint32_t tmax;      /* template k-mers per window the plan provides for (see below) */
    bool pf_full;       /* the index kernel's global matrix slot at its full kPfRowsMax rows (a re-run after CW_WHY_MATRIX) */
};

struct ScratchPlan {
    size_t win, solid_key, solid_cnt, seg_off, seg_len, arena, tasks, members, ctr, list[CW_TIERS], over[CW_TIERS], slab[CW_TIERS], qslab, hslab, finretry, finbig, pfall, ablock, finvis, exg, tdbg, sbusy[CW_TIERS], total;
    uint64_t pfall_elems, ablock_units;
    uint64_t solid_cap, seg_cap, arena_cap;
    uint32_t task_cap, member_cap, arena_scale;
    TierCfg tier[CW_TIERS];
};

/* tmax: template k-mers per window the plan provides for -- 1024 (templates of up to 1032 bases at k = 9: every window of the wrappers' defaults) unless the
   engine was configured for longer ones (cw_configure, up to CW_TMAX): the index kernel takes any template of up to CW_TMAX k-mers, what grows is the plan */
/* the global position-matrix slot of the index kernel: rows (sequences) per template k-mer at most -- what a re-run after CW_WHY_MATRIX gets */
constexpr uint64_t kPfRowsMax = 4100;

static inline ScratchPlan plan_scratch(const PlanInput& in) {
    const uint32_t n_windows = in.n_windows, n_seqs = in.n_seqs, scale = in.scale, tmax = in.tmax;
    const int cus = in.cus;
    ScratchPlan p;
    memset(&p, 0, sizeof(p));
    p.solid_cap = (16ull * in.n_words) / in.prm.solid + n_windows + 16;
    p.seg_cap = (uint64_t)n_windows * (tmax + 2);
    /* scale: 1, or 4 / 16 / 64 after a run whose windows stopped on the task / member / arena capacities -- heuristics of the batch, which a batch of
       few, heavy windows (900-base windows at depth 100) outgrows: cw_run_device_sync runs such a batch again with the larger plan */
    /* the arena is addressed with 32-bit offsets (WinInfo, PoaTask): its scale is the largest one <= scale that keeps the batch's arena inside them
       (x4 of a 52 000-window batch did not, and the re-run ended in CW_E_INVALID); tasks and members scale on their own */
    const uint64_t arena1 = (uint64_t)n_windows * (16ull * (tmax + 16) + 4096);
    uint64_t as = scale;
    while (as > 1 && arena1 * as > 0xFFFFFFFFull) as /= 2;
    p.arena_scale = (uint32_t)as;
    p.arena_cap = arena1 * as;
    uint64_t tc = (64ull * n_windows + 1024) * scale, mc = (2048ull * n_windows + 4096) * scale;
    if (const char* v = CW_AID_ENV("CW_PLAN_DIV")) { const long x = atol(v); if (x >= 2) { tc = tc / (uint64_t)x + 1; mc = mc / (uint64_t)x + 1; } } /* test aid: a first plan that is too small, so that the growth of cw_run / cw_run_device_sync is exercised */
    p.task_cap = (uint32_t)(tc > 0x7FFFFFFFull ? 0x7FFFFFFFull : tc);
    p.member_cap = (uint32_t)(mc > 0x7FFFFFFFull ? 0x7FFFFFFFull : mc);
    /* test aid: shrink the two heuristic capacities so that the overflow path of the chain kernel's task emission can be exercised */
    if (const char* v = CW_AID_ENV("CW_TASK_CAP")) { const long x = atol(v); if (x >= 1 && (uint64_t)x < p.task_cap) p.task_cap = (uint32_t)x; }
    if (const char* v = CW_AID_ENV("CW_MEMBER_CAP")) { const long x = atol(v); if (x >= 1 && (uint64_t)x < p.member_cap) p.member_cap = (uint32_t)x; }
    tier_config(cus, in.big_slots, n_windows, p.tier);
    size_t o = 0;
    auto put = [&](size_t& slot, size_t bytes) { slot = o; o = align_up(o + bytes, 256); };
    put(p.win, (size_t)n_windows * sizeof(WinInfo));
    put(p.solid_key, p.solid_cap * 4);
    put(p.solid_cnt, p.solid_cap * 4);
    put(p.seg_off, p.seg_cap * 4);
    put(p.seg_len, p.seg_cap * 4);
    put(p.arena, p.arena_cap);
    put(p.tasks, ((size_t)p.task_cap + 1) * sizeof(PoaTask)); /* + the batch's neutral task at index task_cap (cw_setup_kernel; cw_chain.h "cap_ok") */
    put(p.members, (size_t)p.member_cap * sizeof(PoaMember));
    put(p.ctr, sizeof(BatchCounters));
    for (int t = 0; t < CW_TIERS; ++t) put(p.list[t], (size_t)p.task_cap * 4); /* list 0 = tier Q */
    for (int t = 0; t < CW_TIERS; ++t) put(p.over[t], (size_t)p.task_cap * 4);
    for (int t = 0; t < CW_TIERS; ++t) put(p.slab[t], (size_t)p.tier[t].slots * p.tier[t].slab_bytes);
    put(p.qslab, (size_t)cus * CW_POAQ_WAVES * 4 * CW_POAQ_SLAB_BYTES); /* tier Q: kept rows of every task a CU can hold */
    put(p.hslab, (size_t)cus * CW_POAH_WAVES * 2 * CW_POAH_SLAB_BYTES); /* tier H: kept rows and code words */
    /* anchor blocks (cw_ab_bytes): header + keys + presence bitsets + dirty list + the position matrix, 2 bytes per (template k-mer,
       sequence); at most CW_TMAX template k-mers per window, so the bound is per sequence, whatever the pieces' lengths are
       (a pile of many pieces only k bases long has few packed words but a full-width matrix) */
    p.ablock_units = ((uint64_t)n_seqs * (2ull * tmax + 2 + tmax / 8) + (uint64_t)n_windows * (tmax * (4ull + 8 + 8 + 8) + 256)) / 16 + 64;
    put(p.ablock, (size_t)p.ablock_units * 16);
    /* the position matrix of a window whose matrix does not fit LDS: up to tmax anchors x the sequences of a pile -- sixteen times the batch's mean depth, at
       least 1024 and at most ~4096 of them (round 6; 4100 whatever the batch through round 5: 2.1 GB of a driver job's plan at depth 30).  The mean depth
       says nothing about the deepest pile, so a window that stops on this slot (CW_WHY_MATRIX) is run again with the slot at kPfRowsMax rows (pf_full,
       grow_if_that_helps): whether it fits does not depend on its neighbours.  Beyond kPfRowsMax it is a reported capacity, as it always was */
    const uint64_t mean_n = n_windows ? (uint64_t)n_seqs / n_windows + 1 : 1;
    const uint64_t pf_n = in.pf_full ? kPfRowsMax : mean_n * 16 < 1024 ? 1024 : mean_n * 16 > kPfRowsMax ? kPfRowsMax : mean_n * 16;
    p.pfall_elems = (uint64_t)tmax * pf_n;
    const size_t idx_wgs = n_windows < (uint32_t)cus ? n_windows : (size_t)cus; /* work-groups of the index kernel: one fallback slot each */
    put(p.pfall, idx_wgs * p.pfall_elems * 2);
    for (int t = 0; t < CW_TIERS; ++t) put(p.sbusy[t], (size_t)p.tier[t].slots * 4);
    put(p.exg, idx_wgs * CW_EXG_SLOTS * 8);
    put(p.tdbg, getenv("CW_TASK_TRACE") ? (size_t)p.task_cap * 16 : 0);
    /* one visited bitmap per wave of the first finish pass -- and of the second (one wave per work-group, up to 64 of them): the larger of the two */
    put(p.finvis, std::max<size_t>((size_t)cus * CW_FIN_WGS_PER_CU * CW_FIN_WAVES, 64) * CW_FIN_VIS_GLB_WORDS * 4);
    put(p.finretry, (size_t)n_windows * 4);
    put(p.finbig, (size_t)64 * 3 * CW_FIN_CB_BIG);
    p.total = o;
    return p;
}

/* The plan of a POA-only run (cw_poa_run, cw_poa_op.h): G groups of n_seqs sequences in n_words packed words.  Exact, since every group is one task of at most
   its own sequences: WinInfo[G], a segment slot and a task per group (+ the neutral task), a member per sequence, the lists, the slab pools and tier Q's rows
   as plan_scratch sizes them for a batch of G windows -- and none of the solid table, the anchor blocks, the matrix and exact-count fallbacks and the finish
   buffers.  The arena holds every group's slot, CW_POA_SLOT_BYTES of its longest member rounded up to 16 bytes: at most two bytes a base of the batch
   (16 bases a word) and 32 a group; offsets into it are 32-bit (PoaTask::out_off), a batch beyond them is refused before anything is launched (arena_cap). */
static inline ScratchPlan plan_poa(uint32_t n_groups, uint32_t n_seqs, uint64_t n_words, int cus, uint32_t big_slots) {
    ScratchPlan p;
    memset(&p, 0, sizeof(p));
    p.seg_cap = n_groups;
    p.arena_scale = 1;
    p.arena_cap = 32ull * n_words + 32ull * n_groups;
    p.task_cap = n_groups;
    p.member_cap = n_seqs ? n_seqs : 1u;
    tier_config(cus, big_slots, n_groups, p.tier);
    size_t o = 0;
    auto put = [&](size_t& slot, size_t bytes) { slot = o; o = align_up(o + bytes, 256); };
    put(p.win, (size_t)n_groups * sizeof(WinInfo)); /* first, as in plan_scratch: cw_debug_win_info reads it from the start of scratch */
    put(p.solid_key, 0); put(p.solid_cnt, 0);
    put(p.seg_off, p.seg_cap * 4);
    put(p.seg_len, p.seg_cap * 4);
    put(p.arena, p.arena_cap <= 0xFFFFFFFFull ? (size_t)p.arena_cap : 0); /* (a refused plan: its total says nothing) */
    put(p.tasks, ((size_t)p.task_cap + 1) * sizeof(PoaTask));
    put(p.members, (size_t)p.member_cap * sizeof(PoaMember));
    put(p.ctr, sizeof(BatchCounters));
    for (int t = 0; t < CW_TIERS; ++t) put(p.list[t], (size_t)p.task_cap * 4);
    for (int t = 0; t < CW_TIERS; ++t) put(p.over[t], (size_t)p.task_cap * 4);
    for (int t = 0; t < CW_TIERS; ++t) put(p.slab[t], (size_t)p.tier[t].slots * p.tier[t].slab_bytes);
    put(p.qslab, (size_t)cus * CW_POAQ_WAVES * 4 * CW_POAQ_SLAB_BYTES);
    put(p.hslab, (size_t)cus * CW_POAH_WAVES * 2 * CW_POAH_SLAB_BYTES);
    put(p.ablock, 0); put(p.pfall, 0);
    for (int t = 0; t < CW_TIERS; ++t) put(p.sbusy[t], (size_t)p.tier[t].slots * 4); /* contiguous: one memset frees every slab */
    put(p.exg, 0);
    put(p.tdbg, getenv("CW_TASK_TRACE") ? (size_t)p.task_cap * 16 : 0);
    put(p.finvis, 0); put(p.finretry, 0); put(p.finbig, 0);
    p.total = o;
    return p;
}

/* The plan of an alignment run (cw_sw_run, cw_sw_op.h): n_seqs sequences in n_groups groups, at most a pair per sequence.  Exact -- every part is a function of
   the batch's counts, the device and the flags, so there is no run with a larger plan: the order kernel's counters, a reference index and a place in the order
   per sequence, and per wave of the grids the unpacked long reference (cw_sw_kernel), the long launch's buffers and sweep state, and -- only under
   CW_SW_WANT_INDELS -- the banded traceback's CW_ST_DIR_BYTES.  The three alignment launches follow one another on one stream and share the per-wave parts, so
   those are sized for the largest grid.  Grids: class 0 (128 registers, 29 KB of LDS a work-group) four work-groups a CU, class 1 one, the long launch one
   wave a work-group, none larger than the batch has sequences; with the indel totals the grids stop at the stitch's CW_ST_MAX_WGS work-groups, 1 MiB a wave
   being what it is.  The sizes do not depend on the number of bases: a pair's buffers are its wave's. */
struct SwPlan {
    size_t ctr, seq_ref, order, gref, lstate, dir, total;
    uint32_t wgs0, wgs1, wgs_long, dir_waves, dir_bytes;
};
static inline SwPlan plan_sw(uint32_t n_groups, uint32_t n_seqs, uint64_t n_words, int cus, uint32_t flags) {
    (void)n_groups; (void)n_words;
    SwPlan p;
    memset(&p, 0, sizeof(p));
    const bool indels = (flags & CW_SW_WANT_INDELS) != 0u;
    const uint32_t by_seqs = (n_seqs + CW_SW_WAVES - 1) / CW_SW_WAVES;
    const uint32_t most0 = indels ? std::min<uint32_t>((uint32_t)cus * 4u, CW_ST_MAX_WGS) : (uint32_t)cus * 4u;
    const uint32_t most1 = indels ? std::min<uint32_t>((uint32_t)cus, CW_ST_MAX_WGS) : (uint32_t)cus;
    p.wgs0 = std::max(1u, std::min(by_seqs, most0));
    p.wgs1 = std::max(1u, std::min(by_seqs, most1));
    p.wgs_long = std::max(1u, std::min<uint32_t>(n_seqs, CW_SW_LONG_MAX_WGS));
    p.dir_bytes = indels ? CW_ST_DIR_BYTES : 0u;
    p.dir_waves = indels ? std::max(std::max(p.wgs0, p.wgs1) * CW_SW_WAVES, p.wgs_long) : 0u;
    size_t o = 0;
    auto put = [&](size_t& slot, size_t bytes) { slot = o; o = align_up(o + bytes, 256); };
    put(p.ctr, (size_t)CW_SW_CTR_WORDS * 4);
    put(p.seq_ref, (size_t)n_seqs * 12); /* a pair's reference, its span's first column, its span's columns */
    put(p.order, (size_t)n_seqs * 4);
    put(p.gref, (size_t)std::max(p.wgs0, p.wgs1) * CW_SW_WAVES * CW_SW_GREF_BYTES);
    put(p.lstate, (size_t)p.wgs_long * CW_SW_LONG_WAVE_BYTES);
    put(p.dir, (size_t)p.dir_waves * p.dir_bytes);
    p.total = o;
    return p;
}

/* The plan of a path run (cw_sw_path_run, cw_sw_path.h): plan_sw's parts -- counters, pair list, per wave the long reference and the long launch's state --
   and per wave of the largest grid the traceback's CW_SW_PATH_BYTES (directions, a byte a cell, and the rows once they outgrow LDS) and the walk's
   CW_SW_STEP_BYTES.  Exact, like plan_sw.  The grids stop where the direction scratch of a run reaches what plan_sw holds under CW_SW_WANT_INDELS:
   CW_SW_PATH_MAX_WAVES waves x 2 MiB = 1 GiB, so class 0 and class 1 launch at most 128 work-groups of four waves, the long launch its 256 of one. */
struct SwPathPlan : SwPlan { size_t steps; }; /* a plan and the steps: what binds and launches a plain run binds and launches this one */
static inline SwPathPlan plan_sw_path(uint32_t n_groups, uint32_t n_seqs, uint64_t n_words, int cus) {
    (void)n_groups; (void)n_words;
    SwPathPlan p;
    memset(&p, 0, sizeof(p));
    const uint32_t by_seqs = (n_seqs + CW_SW_WAVES - 1) / CW_SW_WAVES, most = CW_SW_PATH_MAX_WAVES / CW_SW_WAVES;
    p.wgs0 = std::max(1u, std::min(by_seqs, std::min<uint32_t>((uint32_t)cus * 4u, most)));
    p.wgs1 = std::max(1u, std::min(by_seqs, std::min<uint32_t>((uint32_t)cus, most)));
    p.wgs_long = std::max(1u, std::min<uint32_t>(n_seqs, CW_SW_LONG_MAX_WGS));
    p.dir_bytes = CW_SW_PATH_BYTES;
    p.dir_waves = std::max(std::max(p.wgs0, p.wgs1) * CW_SW_WAVES, p.wgs_long);
    size_t o = 0;
    auto put = [&](size_t& slot, size_t bytes) { slot = o; o = align_up(o + bytes, 256); };
    put(p.ctr, (size_t)CW_SW_CTR_WORDS * 4);
    put(p.seq_ref, (size_t)n_seqs * 12); /* a pair's reference, its span's first column, its span's columns */
    put(p.order, (size_t)n_seqs * 4);
    put(p.gref, (size_t)std::max(p.wgs0, p.wgs1) * CW_SW_WAVES * CW_SW_GREF_BYTES);
    put(p.lstate, (size_t)p.wgs_long * CW_SW_LONG_WAVE_BYTES);
    put(p.dir, (size_t)p.dir_waves * p.dir_bytes);
    put(p.steps, (size_t)p.dir_waves * CW_SW_STEP_BYTES);
    p.total = o;
    return p;
}

/* The plan of a strand run (cw_strand_run, cw_strand.h): the two claim counters and the class totals, and the first unit of every group.  Exact, and the batch
   runs once.  The grids are fixed and claim units, whose number only the device knows; the host knows its bound -- a group has at most one unit more than its
   queries fill chunks -- and launches no more work-groups than that: 256 threads and 16 KB of LDS allow eight a CU, the wide class's 128 KB table one. */
struct StrandPlan { size_t ctr, unit_off, total; uint32_t wgs, wgs_wide; };
static inline StrandPlan plan_strand(uint32_t n_groups, uint32_t n_seqs, int cus) {
    StrandPlan p;
    memset(&p, 0, sizeof(p));
    const uint64_t most = (uint64_t)n_groups + n_seqs / CW_STR_CHUNK, most_wide = (uint64_t)n_groups + n_seqs / CW_STR_CHUNK_WIDE;
    p.wgs = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(most, (uint64_t)cus * 8u));
    p.wgs_wide = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(most_wide, (uint64_t)cus));
    size_t o = 0;
    auto put = [&](size_t& slot, size_t bytes) { slot = o; o = align_up(o + bytes, 256); };
    put(p.ctr, (size_t)CW_STR_CTR_WORDS * 4);
    put(p.unit_off, ((size_t)n_groups + 1) * 4);
    p.total = o;
    return p;
}

/* The plan of a seed run (cw_seed_run, cw_seed.h) is plan_strand's arithmetic: the same counters, units and chunks.  Only the narrow launch is smaller: 25 KB
   of LDS a work-group allow six a CU, not eight. */
static inline StrandPlan plan_seed(uint32_t n_groups, uint32_t n_seqs, int cus) {
    StrandPlan p = plan_strand(n_groups, n_seqs, cus);
    p.wgs = (uint32_t)std::min<uint64_t>(p.wgs, (uint64_t)cus * 6u);
    return p;
}

/* The plan of a locate run (cw_locate_run_device, cw_locate.h), exact: the counters, the redo list -- every read can be on it -- and one dense table per work-group
   of the dense launch.  The LDS launch: a work-group a read, at most six a CU (24 KB each).  The dense launch: at most CW_LOC_DENSE_WGS work-groups -- the route is
   meant to be rare, and a table is 768 KB. */
#define CW_LOC_DENSE_WGS 64u
struct LocatePlan { size_t ctr, redo, dense, total; uint32_t wgs, wgs_dense; };
static inline LocatePlan plan_locate(uint32_t n_seqs, int cus) {
    LocatePlan p;
    memset(&p, 0, sizeof(p));
    p.wgs = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(n_seqs, (uint64_t)cus * 6u));
    p.wgs_dense = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(n_seqs, CW_LOC_DENSE_WGS));
    size_t o = 0;
    auto put = [&](size_t& slot, size_t bytes) { slot = o; o = align_up(o + bytes, 256); };
    put(p.ctr, (size_t)CW_LOC_CTR_WORDS * 4);
    put(p.redo, (size_t)n_seqs * 4);
    put(p.dense, (size_t)p.wgs_dense * CW_LOC_DENSE_WORDS * 4);
    p.total = o;
    return p;
}

/* The plan of an overlap run (cw_overlap_run_device, cw_overlap.h), exact: plan_locate's shape.  The LDS launch: a work-group a query, at most three a CU (48 KB
   each).  The dense launch: at most CW_OVL_DENSE_WGS work-groups, a pair of tables of 6 MB each.  n_queries == 0 plans the count alone: the counters. */
#define CW_OVL_DENSE_WGS 16u
struct OverlapPlan { size_t ctr, redo, dense, total; uint32_t wgs, wgs_dense; };
static inline OverlapPlan plan_overlap(uint32_t n_queries, int cus) {
    OverlapPlan p;
    memset(&p, 0, sizeof(p));
    p.wgs = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(n_queries, (uint64_t)cus * 3u));
    p.wgs_dense = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(n_queries, CW_OVL_DENSE_WGS));
    size_t o = 0;
    auto put = [&](size_t& slot, size_t bytes) { slot = o; o = align_up(o + bytes, 256); };
    put(p.ctr, (size_t)CW_OVL_CTR_WORDS * 4);
    put(p.redo, (size_t)n_queries * 4);
    put(p.dense, n_queries ? (size_t)p.wgs_dense * CW_OVL_DENSE_WORDS * 4 : 0);
    p.total = o;
    return p;
}

/* The largest batch a plan for templates of tmax k-mers can address: per-window offsets into the segment table and the arena are 32-bit, and
   their totals are n_windows x (tmax + 2) and n_windows x (16 (tmax + 16) + 4096) at scale 1 -- at most CW_MAX_BATCH_WINDOWS (include/consent_amd.h
   cw_max_batch_windows).  115 704 windows at tmax 2048, CW_MAX_BATCH_WINDOWS at the default 1024. */
static inline uint32_t max_batch_windows(uint32_t tmax) {
    const uint64_t per_seg = (uint64_t)tmax + 2, per_arena = 16ull * (tmax + 16) + 4096;
    uint64_t n = CW_MAX_BATCH_WINDOWS;
    n = std::min<uint64_t>(n, 0xFFFFFFFFull / per_seg);
    n = std::min<uint64_t>(n, 0xFFFFFFFFull / per_arena);
    return (uint32_t)n;
}

static inline uint32_t plan_tmax(uint32_t k, uint32_t max_template_len) { /* cw_configure's number */
    uint32_t kmers = max_template_len >= k ? max_template_len - k + 1u : 1u;
    return kmers < 128u ? 128u : kmers;
}

#endif
